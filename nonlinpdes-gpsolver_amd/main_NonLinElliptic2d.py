#%%
"""Nonlinear elliptic equation -Delta u + alpha*u^m = f on [0,1]^2 with the GP solver on an MI355X.
Same command line as the reference's main_NonLinElliptic2d.py (README.md:15 of the reference):
    python main_NonLinElliptic2d.py --kernel Gaussian --kernel_parameter 0.2 --nugget 1e-13 --N_domain 900 --N_boundary 124 --GNsteps 4
The manufactured solution's right-hand side is written out analytically (the reference differentiates u with jax.grad).
--bc neumann / --bc robin [--robin_beta B] (no counterpart in the reference) prescribe du/dn = g or B u + du/dn = g on the boundary
instead of u = g, with g formed from the manufactured solution's gradient and the outward normal.
--operator advection_diffusion (no counterpart in the reference either) solves -div(a grad u) + v . grad u + c u + alpha*u^m = f with the
fields of advection_diffusion_fields() below and the right-hand side that makes the same u* the solution; --operator laplace (the
default) is the equation above.  --bc works with either.
--nonlinearity exp|sinh|sin|cubic [--nl_params=p0,p1[,p2]] (no counterpart in the reference) replaces alpha*u^m by another reaction term
tau(u): p0*exp(p1*u), p0*sinh(p1*u), p0*sin(p1*u) or p0*u + p1*u^2 + p2*u^3; the right-hand side is manufactured with the same tau, so
every --operator / --bc combination works with every kind:
    python main_NonLinElliptic2d.py --nonlinearity exp --nl_params=-1,1 --nugget 1e-8          (Bratu)
    python main_NonLinElliptic2d.py --nonlinearity sinh --nl_params=4,1 --bc robin --nugget 1e-8   (Poisson-Boltzmann)
--kernel periodic_Gaussian --kernel_parameter S1 S2 --period L1 L2 (no counterpart in the reference) makes the solution periodic along the
axes with L_k = 1 (0: not periodic) through a periodic kernel: no boundary points on the faces of that axis, and a manufactured solution
that is periodic there (manufactured_periodic); with the Laplacian and Dirichlet data on the other faces only:
    python main_NonLinElliptic2d.py --kernel periodic_Gaussian --kernel_parameter 0.2 0.2 --period 1 0 --nugget 1e-8 --GNsteps 6"""
import argparse

import numpy as onp

from _driver_common import (add_gn_and_logs, add_kernel_and_sampling, add_nonlinearity, nonlinearity_from, periodic_axes_of, report_test_error,
                            report_test_residual, report_test_variance, report_posterior_samples, solve_forward, tensor_grid)

UNIT_SQUARE = [[0, 1], [0, 1]]


def parse(argv=None):
    parser = argparse.ArgumentParser(description='NonLinElliptic equation GP solver')
    parser.add_argument("--alpha", type=float, default=1.0)
    parser.add_argument("--m", type=float, default=3.0)
    add_kernel_and_sampling(parser, 'Gaussian', 0.2, 1e-13, 900, 124)
    parser.add_argument("--pen_lambda", type=float, default=1e-10)      # for the relaxation approach
    parser.add_argument("--bc", type=str, default='dirichlet', choices=['dirichlet', 'neumann', 'robin'])
    parser.add_argument("--robin_beta", type=float, default=1.0)        # beta of --bc robin: beta u + du/dn = g
    parser.add_argument("--operator", type=str, default='laplace', choices=['laplace', 'advection_diffusion'])
    add_nonlinearity(parser)
    add_gn_and_logs(parser, 'rdm', 4, method_choices=['elimination', 'relaxation'])
    return parser.parse_args(argv)


def reaction(alpha, m=None):
    """the reaction term as a Nonlinearity: `alpha` is one already, or (alpha, m) of the power law"""
    from src.nonlinearity import Nonlinearity
    return alpha if isinstance(alpha, Nonlinearity) else Nonlinearity.power(alpha, m)


def manufactured(alpha, m=None):
    """u* = sin(pi x1) sin(pi x2) + 2 sin(4 pi x1) sin(4 pi x2) and f = -Laplace(u*) + tau(u*); tau: a Nonlinearity, or alpha, m of alpha u^m"""
    pi = onp.pi
    tau = reaction(alpha, m)

    def u(x1, x2):
        return onp.sin(pi * x1) * onp.sin(pi * x2) + 2 * onp.sin(4 * pi * x1) * onp.sin(4 * pi * x2)

    def f(x1, x2):
        lap = -2 * pi ** 2 * onp.sin(pi * x1) * onp.sin(pi * x2) - 64 * pi ** 2 * onp.sin(4 * pi * x1) * onp.sin(4 * pi * x2)
        return -lap + tau.tau(u(x1, x2))
    return u, f


def manufactured_periodic(periodic, alpha, m=None):
    """u* and f = -Laplace(u*) + tau(u*) for a solution with period 1 along the axes of `periodic`: u* = a1 a2 + 2 b1 b2 with, per axis,
    a = sin(2 pi x), b = cos(4 pi x) on a periodic axis (neither vanishes with all derivatives at the faces, so the periodicity is the
    kernel's doing) and a = sin(pi x), b = sin(4 pi x) otherwise, as in manufactured()"""
    pi = onp.pi
    tau = reaction(alpha, m)
    a = [(onp.sin, 2 * pi) if per else (onp.sin, pi) for per in periodic]
    b = [(onp.cos, 4 * pi) if per else (onp.sin, 4 * pi) for per in periodic]

    def u(x1, x2):
        return a[0][0](a[0][1] * x1) * a[1][0](a[1][1] * x2) + 2 * b[0][0](b[0][1] * x1) * b[1][0](b[1][1] * x2)

    def f(x1, x2):
        lap = (-(a[0][1] ** 2 + a[1][1] ** 2) * a[0][0](a[0][1] * x1) * a[1][0](a[1][1] * x2)
               - 2 * (b[0][1] ** 2 + b[1][1] ** 2) * b[0][0](b[0][1] * x1) * b[1][0](b[1][1] * x2))
        return -lap + tau.tau(u(x1, x2))
    return u, f


def manufactured_gradient(x1, x2):
    """gradient of u* of manufactured()"""
    pi = onp.pi
    return (pi * onp.cos(pi * x1) * onp.sin(pi * x2) + 8 * pi * onp.cos(4 * pi * x1) * onp.sin(4 * pi * x2),
            pi * onp.sin(pi * x1) * onp.cos(pi * x2) + 8 * pi * onp.sin(4 * pi * x1) * onp.cos(4 * pi * x2))


def advection_diffusion_fields(x1, x2):
    """(a, a_x1, a_x2, v1, v2, c) of --operator advection_diffusion: diffusivity a = 2 + sin(pi x1) cos(pi x2) in [1, 3] with its gradient,
    a rotating velocity v = (1 + x2, 1 - x1) and the reaction coefficient c = 1 + x1^2 >= 1"""
    pi = onp.pi
    x1 = onp.asarray(x1, dtype=onp.float64); x2 = onp.asarray(x2, dtype=onp.float64)
    return (2 + onp.sin(pi * x1) * onp.cos(pi * x2), pi * onp.cos(pi * x1) * onp.cos(pi * x2), -pi * onp.sin(pi * x1) * onp.sin(pi * x2),
            1 + x2, 1 - x1, 1 + x1 ** 2)


def advection_diffusion(x1, x2):
    """the callable `operator` of Nonlinear_elliptic2d for those fields: six coefficient arrays of psi with -psi[u] = -div(a grad u) + v . grad u + c u"""
    from src.PDEs import divergence_form
    return divergence_form(*advection_diffusion_fields(x1, x2))


OPERATORS = {'laplace': None, 'advection_diffusion': advection_diffusion}


def manufactured_operator_rhs(alpha, m=None):
    """f = -div(a grad u*) + v . grad u* + c u* + tau(u*) for u* of manufactured() and the fields above"""
    pi = onp.pi
    tau = reaction(alpha, m)
    u, _ = manufactured(tau)

    def f(x1, x2):
        a, a1, a2, v1, v2, c = advection_diffusion_fields(x1, x2)
        u1, u2 = manufactured_gradient(x1, x2)
        lap = -2 * pi ** 2 * onp.sin(pi * x1) * onp.sin(pi * x2) - 64 * pi ** 2 * onp.sin(4 * pi * x1) * onp.sin(4 * pi * x2)
        return -(a * lap + a1 * u1 + a2 * u2) + v1 * u1 + v2 * u2 + c * u(x1, x2) + tau.tau(u(x1, x2))
    return f


def boundary_data(u, bc, robin_beta, domain=UNIT_SQUARE):
    """the callback bdy(x1, x2) = value of the boundary operator on u*: u* itself (dirichlet), du*/dn (neumann), beta u* + du*/dn (robin)"""
    if bc == 'dirichlet':
        return u
    from src.sample_points import boundary_normals
    beta = robin_beta if bc == 'robin' else 0.0

    def g(x1, x2):
        x1 = onp.asarray(x1, dtype=onp.float64); x2 = onp.asarray(x2, dtype=onp.float64)
        n = boundary_normals(onp.stack([x1.ravel(), x2.ravel()], axis=1), domain)
        u1, u2 = manufactured_gradient(x1, x2)
        return beta * u(x1, x2) + n[:, 0].reshape(x1.shape) * u1 + n[:, 1].reshape(x1.shape) * u2
    return g


def main(argv=None):
    cfg = parse(argv)
    tau, cfg.nonlinearity = nonlinearity_from(cfg)                      # (None: alpha*u^m of --alpha / --m, the facade's default)
    u, f = manufactured(tau)
    periodic = periodic_axes_of(cfg)
    if any(periodic):
        if cfg.operator != 'laplace' or cfg.bc != 'dirichlet':
            raise SystemExit('--kernel periodic_Gaussian: with --operator laplace and --bc dirichlet only')
        u, f = manufactured_periodic(periodic, tau)
    if cfg.operator != 'laplace':
        f = manufactured_operator_rhs(tau)
        cfg.operator = OPERATORS[cfg.operator]                           # the facade takes the callable (or 'laplace' / None: the Laplacian)
    solver, show = solve_forward(cfg, "Nonlinear_elliptic", boundary_data(u, cfg.bc, cfg.robin_beta), f, UNIT_SQUARE,
                                 solve_kwargs={'method': cfg.method, 'pen_lambda': cfg.pen_lambda}, verbose=cfg.print_hist)
    Xd = solver.eqn.X_domain
    solver.collocation_pts_err(u(Xd[:, 0], Xd[:, 1]))                    # error on the collocation points
    XX, YY, X_test = tensor_grid(60, *UNIT_SQUARE)                       # error on a 60 x 60 test grid
    report_test_error(solver, show, XX, YY, X_test, u(X_test[:, 0], X_test[:, 1]))
    report_test_residual(cfg, solver, X_test)
    report_test_variance(cfg, solver, X_test)
    report_posterior_samples(cfg, solver, X_test)


if __name__ == '__main__':
    main()
