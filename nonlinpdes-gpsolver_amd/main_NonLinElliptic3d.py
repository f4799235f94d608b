#%%
"""Nonlinear elliptic equation -Delta u + alpha*u^m = f on the unit cube [0,1]^3 with the GP solver on an MI355X.
Same flags as main_NonLinElliptic2d.py (the relaxed formulation is not offered in three dimensions):
    python main_NonLinElliptic3d.py --kernel Gaussian --kernel_parameter 0.3 --nugget 1e-8 --N_domain 1000 --N_boundary 486 --GNsteps 6
N_boundary must be divisible by 6 for random points (N_boundary / 6 per face).  --show_figure is accepted and ignored: the plot
helpers draw planar point sets and contours.
--bc neumann / --bc robin [--robin_beta B] prescribe du/dn = g or B u + du/dn = g on the faces instead of u = g.
--operator advection_diffusion solves -div(a grad u) + v . grad u + c u + alpha*u^m = f with the fields of advection_diffusion_fields()
and the right-hand side that makes the same u* the solution (--bc works with it).
--operator parabolic treats axis 3 as time: u_t - nu Laplace_x u + alpha*u^m = f on the unit square x [0,1] by space-time collocation,
initial and lateral data only (no points on the face t = 1; N_boundary divisible by 5 for random points), Dirichlet data:
    python main_NonLinElliptic3d.py --operator advection_diffusion --bc robin --robin_beta 2
    python main_NonLinElliptic3d.py --operator parabolic --nu 0.2 --N_boundary 485
--nonlinearity exp|sinh|sin|cubic [--nl_params=p0,p1[,p2]] replaces alpha*u^m by another reaction term tau(u), as in two dimensions; with
--operator parabolic and a cubic this is time-dependent Allen-Cahn, u_t - nu Laplace_x u - u + u^3 = f:
    python main_NonLinElliptic3d.py --operator parabolic --nonlinearity cubic --nl_params=-1,0,1 --N_boundary 485"""
import argparse

import numpy as onp

from _driver_common import (add_gn_and_logs, add_kernel_and_sampling, add_nonlinearity, nonlinearity_from, report_test_error,
                            report_test_residual, solve_forward)

UNIT_CUBE = [[0, 1], [0, 1], [0, 1]]
GRID = 20                                                                # test grid: GRID^3 points


def parse(argv=None):
    parser = argparse.ArgumentParser(description='NonLinElliptic equation GP solver, three space dimensions')
    parser.add_argument("--alpha", type=float, default=1.0)
    parser.add_argument("--m", type=float, default=3.0)
    add_kernel_and_sampling(parser, 'Gaussian', 0.3, 1e-8, 1000, 486)
    parser.add_argument("--bc", type=str, default='dirichlet', choices=['dirichlet', 'neumann', 'robin'])
    parser.add_argument("--robin_beta", type=float, default=1.0)        # beta of --bc robin: beta u + du/dn = g
    parser.add_argument("--operator", type=str, default='laplace', choices=['laplace', 'advection_diffusion', 'parabolic'])
    parser.add_argument("--nu", type=float, default=0.2)                # diffusivity of --operator parabolic
    add_nonlinearity(parser)
    add_gn_and_logs(parser, 'rdm', 6, method_choices=['elimination'])
    return parser.parse_args(argv)


def reaction(alpha, m=None):
    """the reaction term as a Nonlinearity: `alpha` is one already, or (alpha, m) of the power law"""
    from src.nonlinearity import Nonlinearity
    return alpha if isinstance(alpha, Nonlinearity) else Nonlinearity.power(alpha, m)


def manufactured(alpha, m=None):
    """u* = prod_k sin(pi x_k) + 2 prod_k sin(2 pi x_k) and f = -Laplace(u*) + tau(u*); tau: a Nonlinearity, or alpha, m of alpha u^m"""
    pi = onp.pi
    tau = reaction(alpha, m)

    def modes(x1, x2, x3):
        return (onp.sin(pi * x1) * onp.sin(pi * x2) * onp.sin(pi * x3),
                onp.sin(2 * pi * x1) * onp.sin(2 * pi * x2) * onp.sin(2 * pi * x3))

    def u(x1, x2, x3):
        s1, s2 = modes(x1, x2, x3)
        return s1 + 2 * s2

    def f(x1, x2, x3):
        s1, s2 = modes(x1, x2, x3)
        lap = -3 * pi ** 2 * s1 - 24 * pi ** 2 * s2
        return -lap + tau.tau(u(x1, x2, x3))
    return u, f


def manufactured_gradient(x1, x2, x3):
    """gradient of u* of manufactured()"""
    pi = onp.pi
    out = []
    for k in range(3):
        t1 = [onp.sin(pi * x) for x in (x1, x2, x3)]; t2 = [onp.sin(2 * pi * x) for x in (x1, x2, x3)]
        t1[k] = pi * onp.cos(pi * (x1, x2, x3)[k]); t2[k] = 2 * pi * onp.cos(2 * pi * (x1, x2, x3)[k])
        out.append(t1[0] * t1[1] * t1[2] + 2 * t2[0] * t2[1] * t2[2])
    return tuple(out)


def advection_diffusion_fields(x1, x2, x3):
    """(a, a_x1, a_x2, a_x3, v1, v2, v3, c) of --operator advection_diffusion: diffusivity a = 2 + sin(pi x1) cos(pi x2) cos(pi x3) in
    [1, 3] with its gradient, the velocity v = (1 + x2, 1 - x1, x3 - 1/2) and the reaction coefficient c = 1 + x1^2 >= 1"""
    pi = onp.pi
    x1, x2, x3 = (onp.asarray(x, dtype=onp.float64) for x in (x1, x2, x3))
    s1, c1, s2, c2, s3, c3 = onp.sin(pi * x1), onp.cos(pi * x1), onp.sin(pi * x2), onp.cos(pi * x2), onp.sin(pi * x3), onp.cos(pi * x3)
    return (2 + s1 * c2 * c3, pi * c1 * c2 * c3, -pi * s1 * s2 * c3, -pi * s1 * c2 * s3, 1 + x2, 1 - x1, x3 - 0.5, 1 + x1 ** 2)


def advection_diffusion(x1, x2, x3):
    """the callable `operator` of Nonlinear_elliptic3d for those fields: ten coefficient arrays of psi, -psi[u] = -div(a grad u) + v . grad u + c u"""
    from src.PDEs import divergence_form3d
    return divergence_form3d(*advection_diffusion_fields(x1, x2, x3))


def operator_rhs(fields, u, grad, lap, alpha, m=None):
    """f = -div(a grad u) + v . grad u + c u + tau(u) for the fields (a, grad a, v, c) and a solution given with gradient and Laplacian"""
    tau = reaction(alpha, m)

    def f(x1, x2, x3):
        a, a1, a2, a3, v1, v2, v3, c = fields(x1, x2, x3)
        u1, u2, u3 = grad(x1, x2, x3)
        w = u(x1, x2, x3)
        return -(a * lap(x1, x2, x3) + a1 * u1 + a2 * u2 + a3 * u3) + v1 * u1 + v2 * u2 + v3 * u3 + c * w + tau.tau(w)
    return f


def manufactured_operator_rhs(alpha, m=None):
    """the right-hand side of --operator advection_diffusion for u* of manufactured()"""
    tau = reaction(alpha, m)
    u, f0 = manufactured(tau)
    lap = lambda x1, x2, x3: -(f0(x1, x2, x3) - tau.tau(u(x1, x2, x3)))
    return operator_rhs(advection_diffusion_fields, u, manufactured_gradient, lap, tau)


def parabolic_manufactured(alpha, m, nu=None):
    """u*(x1, x2, t) = e^{-t} sin(pi x1) sin(pi x2) + t/2 sin(2 pi x1) sin(pi x2) and f = u*_t - nu Laplace_x u* + tau(u*); called as
    (alpha, m, nu) for alpha u^m or as (tau, nu) with a Nonlinearity"""
    pi = onp.pi
    if nu is None:
        tau, nu = reaction(alpha), m
    else:
        tau = reaction(alpha, m)

    def modes(x1, x2):
        return onp.sin(pi * x1) * onp.sin(pi * x2), onp.sin(2 * pi * x1) * onp.sin(pi * x2)

    def u(x1, x2, t):
        s1, s2 = modes(x1, x2)
        return onp.exp(-t) * s1 + 0.5 * t * s2

    def f(x1, x2, t):
        s1, s2 = modes(x1, x2)
        ut = -onp.exp(-t) * s1 + 0.5 * s2
        lap = -2 * pi ** 2 * onp.exp(-t) * s1 - 5 * pi ** 2 * 0.5 * t * s2
        return ut - nu * lap + tau.tau(u(x1, x2, t))
    return u, f


def boundary_data(u, grad, bc, robin_beta, domain=UNIT_CUBE):
    """the callback bdy(x1, x2, x3) = value of the boundary operator on u: u itself (dirichlet), du/dn (neumann), beta u + du/dn (robin)"""
    if bc == 'dirichlet':
        return u
    from src.sample_points import boundary_normals3d
    beta = robin_beta if bc == 'robin' else 0.0

    def g(x1, x2, x3):
        x1, x2, x3 = (onp.asarray(x, dtype=onp.float64) for x in (x1, x2, x3))
        n = boundary_normals3d(onp.stack([x1.ravel(), x2.ravel(), x3.ravel()], axis=1), domain)
        return beta * u(x1, x2, x3) + sum(n[:, k].reshape(x1.shape) * gk for k, gk in enumerate(grad(x1, x2, x3)))
    return g


def cube_grid(n=GRID):
    """n^3 tensor grid on the unit cube, faces included: (n^3, 3) points"""
    g = onp.linspace(0.0, 1.0, n)
    return onp.stack([a.ravel() for a in onp.meshgrid(g, g, g, indexing='ij')], axis=1)


def main(argv=None):
    cfg = parse(argv)
    cfg.show_figure = False                                              # accepted and ignored
    tau, cfg.nonlinearity = nonlinearity_from(cfg)                      # (None: alpha*u^m of --alpha / --m, the facade's default)
    u, f = manufactured(tau)
    bdy = u
    if cfg.operator == 'parabolic':
        if cfg.bc != 'dirichlet':
            raise SystemExit('--operator parabolic takes Dirichlet data (initial and lateral values)')
        from src.PDEs import parabolic_form
        u, f = parabolic_manufactured(tau, cfg.nu)
        bdy = u
        cfg.operator = parabolic_form(cfg.nu)                            # the facade takes the callable (or 'laplace' / None: the Laplacian)
        cfg.time_dependent = True
    else:
        if cfg.operator == 'advection_diffusion':
            f = manufactured_operator_rhs(tau)
            cfg.operator = advection_diffusion
        if cfg.bc != 'dirichlet':
            bdy = boundary_data(u, manufactured_gradient, cfg.bc, cfg.robin_beta)
    solver, _ = solve_forward(cfg, "Nonlinear_elliptic3d", bdy, f, UNIT_CUBE, solve_kwargs={'method': cfg.method}, verbose=cfg.print_hist)
    Xd = solver.eqn.X_domain
    solver.collocation_pts_err(u(Xd[:, 0], Xd[:, 1], Xd[:, 2]))          # error on the collocation points
    X_test = cube_grid()
    report_test_error(solver, False, None, None, X_test, u(X_test[:, 0], X_test[:, 1], X_test[:, 2]))
    report_test_residual(cfg, solver, X_test)


if __name__ == '__main__':
    main()
