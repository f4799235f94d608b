#%%
"""Semilinear equation -eps*Delta u + N(u, grad u) = f on [0,1]^2, u = g on the boundary, with the GP solver on an MI355X
(no counterpart in the reference).  N(u, p, q) = u (a1 p + a2 q) + b (p^2 + q^2) + c1 u + c3 u^3, p = u_x1, q = u_x2:
    python main_Semilinear2d.py --equation burgers --eps 0.1                         u (u_x1 + u_x2): steady viscous Burgers
    python main_Semilinear2d.py --equation hamilton_jacobi --eps 0.5                 |grad u|^2 + u: viscous Hamilton-Jacobi
    python main_Semilinear2d.py --equation custom --nl_params=1,-1,0.5,1,1 --eps 0.2
--nl_params=a1,a2,b,c1,c3 overrides the coefficients of any --equation.  The manufactured solution is u* = sin(pi x1) sin(pi x2) with f
formed analytically.  Plain Gauss-Newton steps: keep --eps at 0.1 or above (convection-dominated settings do not converge).
--kernel periodic_Gaussian --kernel_parameter S1 S2 --period L1 L2 (L_k = 1 or 0): periodic along the axes with L_k = 1, no boundary points
on their faces; the manufactured solution has sin(2 pi x_k) + cos(2 pi x_k) / 2 in place of sin(pi x_k) there."""
import argparse

import numpy as onp

from _driver_common import (add_gn_and_logs, add_kernel_and_sampling, periodic_axes_of, report_test_error, report_test_residual, report_test_variance,
                            report_posterior_samples, solve_forward, tensor_grid)

UNIT_SQUARE = [[0, 1], [0, 1]]
# --equation -> (a1, a2, b, c1, c3)
EQUATIONS = {'burgers': (1.0, 1.0, 0.0, 0.0, 0.0), 'hamilton_jacobi': (0.0, 0.0, 1.0, 1.0, 0.0), 'custom': (1.0, -1.0, 0.5, 1.0, 1.0)}


def parse(argv=None):
    parser = argparse.ArgumentParser(description='Semilinear equation with a gradient-dependent nonlinearity, GP solver')
    parser.add_argument("--equation", type=str, default='burgers', choices=sorted(EQUATIONS))
    parser.add_argument("--nl_params", type=str, default=None)          # a1,a2,b,c1,c3
    parser.add_argument("--eps", type=float, default=1e-1)
    add_kernel_and_sampling(parser, 'Gaussian', 0.2, 1e-8, 600, 120)
    add_gn_and_logs(parser, 'zero', 8)
    return parser.parse_args(argv)


def coefficients_from(cfg):
    """(a1, a2, b, c1, c3) the command line asks for"""
    if cfg.nl_params is None:
        return EQUATIONS[cfg.equation]
    try:
        params = tuple(float(v) for v in cfg.nl_params.split(',') if v.strip())
    except ValueError as e:
        raise SystemExit(f'--nl_params: {e}')
    if len(params) != 5:
        raise SystemExit('--nl_params takes the five coefficients a1,a2,b,c1,c3')
    return params


def manufactured(eps, nl, periodic=(False, False)):
    """u* = a(x1) a(x2) and f = -eps Laplace(u*) + N(u*, grad u*) for the GradientNonlinearity nl, with a(x) = sin(pi x), or on a periodic
    axis a(x) = sin(2 pi x) + cos(2 pi x) / 2 (period 1, not zero at the faces)"""
    pi = onp.pi

    def factor(per):
        k = 2 * pi if per else pi
        h = 0.5 if per else 0.0
        return (lambda x: onp.sin(k * x) + h * onp.cos(k * x)), (lambda x: k * (onp.cos(k * x) - h * onp.sin(k * x))), k * k

    (a1, da1, k1), (a2, da2, k2) = factor(periodic[0]), factor(periodic[1])

    def u(x1, x2):
        return a1(x1) * a2(x2)

    def f(x1, x2):
        us = u(x1, x2)
        p, q = da1(x1) * a2(x2), a1(x1) * da2(x2)
        return (k1 + k2) * eps * us + nl.N(us, p, q)
    return u, f


def main(argv=None):
    from src.nonlinearity import GradientNonlinearity
    cfg = parse(argv)
    nl = GradientNonlinearity.make(coefficients_from(cfg))
    cfg.nonlinearity = nl
    u, f = manufactured(cfg.eps, nl, periodic_axes_of(cfg))
    solver, show = solve_forward(cfg, "Semilinear2d", u, f, UNIT_SQUARE, verbose=cfg.print_hist)
    Xd = solver.eqn.X_domain
    solver.collocation_pts_err(u(Xd[:, 0], Xd[:, 1]))                    # error on the collocation points
    XX, YY, X_test = tensor_grid(60, *UNIT_SQUARE)                       # error on a 60 x 60 test grid
    report_test_error(solver, show, XX, YY, X_test, u(X_test[:, 0], X_test[:, 1]))
    report_test_residual(cfg, solver, X_test)
    report_test_variance(cfg, solver, X_test)
    report_posterior_samples(cfg, solver, X_test)


if __name__ == '__main__':
    main()
