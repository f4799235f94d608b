#%%
"""Semilinear equation -psi[u] + N(u, grad u) = f with a gradient-dependent nonlinearity in three dimensions, or in two space dimensions
and time, with the GP solver on an MI355X (no counterpart in the reference).
N(u, g) = u (a1 g1 + a2 g2 + a3 g3) + b1 g1^2 + b2 g2^2 + b3 g3^2 + c1 u + c3 u^3, g_k = u_xk:
    python main_Semilinear3d.py --equation burgers --eps 0.3                              -eps Lap u + u (u_x1 + u_x2 + u_x3) = f on the unit cube
    python main_Semilinear3d.py --equation hamilton_jacobi --eps 0.5                      -eps Lap u + |grad u|^2 = f
    python main_Semilinear3d.py --equation eikonal --eps 0.5                              the regularised Eikonal equation
    python main_Semilinear3d.py --operator parabolic --equation burgers --nu 0.2 --N_boundary 485      u_t - nu Lap_x u + u (u_x1 + u_x2) = f
    python main_Semilinear3d.py --operator parabolic --equation hamilton_jacobi --nu 0.2 --N_boundary 485      u_t - nu Lap_x u + |grad_x u|^2 = f
--operator parabolic treats axis 3 as time (space-time collocation on the unit square x [0,1], initial and lateral data only: no points
on the face t = 1; N_boundary divisible by 5 for random points, Dirichlet data); the time derivative does not enter N there (a3 = b3 = 0).
--nl_params=a1,a2,a3,b1,b2,b3,c1,c3 overrides the coefficients of any --equation.  --bc neumann / --bc robin [--robin_beta B] as in
main_NonLinElliptic3d.py (--operator laplacian only).  The manufactured solutions are u* = prod_k sin(pi x_k) on the cube and
u* = e^{-t} sin(pi x1) sin(pi x2) + t/2 sin(2 pi x1) sin(pi x2) in space-time, with f formed analytically.  --show_figure is accepted and
ignored.  Plain Gauss-Newton steps from the zero start: keep --eps / --nu at 0.2 or above, or add --line_search 1."""
import argparse

import numpy as onp

from _driver_common import add_gn_and_logs, add_kernel_and_sampling, report_test_error, report_test_residual, solve_forward
from main_NonLinElliptic3d import UNIT_CUBE, boundary_data, cube_grid

# --equation -> (a1, a2, a3, b1, b2, b3, c1, c3) on the cube; with --operator parabolic a3 and b3 are set to 0
EQUATIONS = {'burgers': (1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0), 'hamilton_jacobi': (0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0.0, 0.0),
             'eikonal': (0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0.0, 0.0)}


def parse(argv=None):
    parser = argparse.ArgumentParser(description='Semilinear equation with a gradient-dependent nonlinearity in three dimensions, GP solver')
    parser.add_argument("--equation", type=str, default='burgers', choices=sorted(EQUATIONS))
    parser.add_argument("--nl_params", type=str, default=None)          # a1,a2,a3,b1,b2,b3,c1,c3
    parser.add_argument("--operator", type=str, default='laplacian', choices=['laplacian', 'parabolic'])
    parser.add_argument("--eps", type=float, default=0.3)               # psi = eps Laplace (--operator laplacian)
    parser.add_argument("--nu", type=float, default=0.2)                # psi = nu Laplace_x - d_t (--operator parabolic)
    parser.add_argument("--bc", type=str, default='dirichlet', choices=['dirichlet', 'neumann', 'robin'])
    parser.add_argument("--robin_beta", type=float, default=1.0)
    add_kernel_and_sampling(parser, 'Gaussian', 0.3, 1e-8, 1000, 486)
    add_gn_and_logs(parser, 'zero', 8, method_choices=['elimination'])
    return parser.parse_args(argv)


def coefficients_from(cfg):
    """(a1, a2, a3, b1, b2, b3, c1, c3) the command line asks for"""
    if cfg.nl_params is None:
        c = list(EQUATIONS[cfg.equation])
    else:
        try:
            c = [float(v) for v in cfg.nl_params.split(',') if v.strip()]
        except ValueError as e:
            raise SystemExit(f'--nl_params: {e}')
        if len(c) != 8:
            raise SystemExit('--nl_params takes the eight coefficients a1,a2,a3,b1,b2,b3,c1,c3')
    if cfg.operator == 'parabolic':
        c[2] = c[5] = 0.0                                                # axis 3 is time: u_t does not enter N
    return tuple(c)


def manufactured(eps, nl):
    """u* = prod_k sin(pi x_k), its gradient, and f = -eps Laplace(u*) + N(u*, grad u*) for the GradientNonlinearity3d nl"""
    pi = onp.pi

    def u(x1, x2, x3):
        return onp.sin(pi * x1) * onp.sin(pi * x2) * onp.sin(pi * x3)

    def grad(x1, x2, x3):
        s, c = [onp.sin(pi * x) for x in (x1, x2, x3)], [onp.cos(pi * x) for x in (x1, x2, x3)]
        return pi * c[0] * s[1] * s[2], pi * s[0] * c[1] * s[2], pi * s[0] * s[1] * c[2]

    def f(x1, x2, x3):
        us = u(x1, x2, x3)
        return 3 * pi ** 2 * eps * us + nl.N(us, *grad(x1, x2, x3))
    return u, grad, f


def parabolic_manufactured(nu, nl):
    """u*(x1, x2, t) = e^{-t} sin(pi x1) sin(pi x2) + t/2 sin(2 pi x1) sin(pi x2) and f = u*_t - nu Laplace_x u* + N(u*, grad_x u*, u*_t)
    (nl with a3 = b3 = 0: the last argument does not enter)"""
    pi = onp.pi

    def parts(x1, x2, t):
        e = onp.exp(-t)
        s1, s2 = onp.sin(pi * x1) * onp.sin(pi * x2), onp.sin(2 * pi * x1) * onp.sin(pi * x2)
        us = e * s1 + 0.5 * t * s2
        u1 = e * pi * onp.cos(pi * x1) * onp.sin(pi * x2) + 0.5 * t * 2 * pi * onp.cos(2 * pi * x1) * onp.sin(pi * x2)
        u2 = e * pi * onp.sin(pi * x1) * onp.cos(pi * x2) + 0.5 * t * pi * onp.sin(2 * pi * x1) * onp.cos(pi * x2)
        ut = -e * s1 + 0.5 * s2
        lap = -2 * pi ** 2 * e * s1 - 5 * pi ** 2 * 0.5 * t * s2
        return us, u1, u2, ut, lap

    def u(x1, x2, t):
        return parts(x1, x2, t)[0]

    def f(x1, x2, t):
        us, u1, u2, ut, lap = parts(x1, x2, t)
        return ut - nu * lap + nl.N(us, u1, u2, ut)
    return u, f


def main(argv=None):
    from src.nonlinearity import GradientNonlinearity3d
    cfg = parse(argv)
    cfg.show_figure = False                                              # accepted and ignored
    nl = GradientNonlinearity3d.make(coefficients_from(cfg))
    cfg.nonlinearity = nl
    if cfg.operator == 'parabolic':
        if cfg.bc != 'dirichlet':
            raise SystemExit('--operator parabolic takes Dirichlet data (initial and lateral values)')
        from src.PDEs import parabolic_form
        u, f = parabolic_manufactured(cfg.nu, nl)
        bdy = u
        cfg.operator = parabolic_form(cfg.nu)                            # the facade takes the callable
        cfg.time_dependent = True
    else:
        u, grad, f = manufactured(cfg.eps, nl)
        bdy = boundary_data(u, grad, cfg.bc, cfg.robin_beta)
        cfg.operator = None                                              # psi = eps Laplace, the class's default
    solver, _ = solve_forward(cfg, "Semilinear3d", bdy, f, UNIT_CUBE, solve_kwargs={'method': cfg.method}, verbose=cfg.print_hist)
    Xd = solver.eqn.X_domain
    solver.collocation_pts_err(u(Xd[:, 0], Xd[:, 1], Xd[:, 2]))          # error on the collocation points
    X_test = cube_grid()
    report_test_error(solver, False, None, None, X_test, u(X_test[:, 0], X_test[:, 1], X_test[:, 2]))
    report_test_residual(cfg, solver, X_test)
    return solver


if __name__ == '__main__':
    main()
