#%%
"""Nonlinear elliptic equation -Delta u + alpha*u^m = f on the unit cube [0,1]^3 with the GP solver on an MI355X.
Same flags as main_NonLinElliptic2d.py (the relaxed formulation is not offered in three dimensions):
    python main_NonLinElliptic3d.py --kernel Gaussian --kernel_parameter 0.3 --nugget 1e-8 --N_domain 1000 --N_boundary 486 --GNsteps 6
N_boundary must be divisible by 6 for random points (N_boundary / 6 per face).  --show_figure is accepted and ignored: the plot
helpers draw planar point sets and contours."""
import argparse

import numpy as onp

from _driver_common import add_gn_and_logs, add_kernel_and_sampling, report_test_error, report_test_residual, solve_forward

UNIT_CUBE = [[0, 1], [0, 1], [0, 1]]
GRID = 20                                                                # test grid: GRID^3 points


def parse(argv=None):
    parser = argparse.ArgumentParser(description='NonLinElliptic equation GP solver, three space dimensions')
    parser.add_argument("--alpha", type=float, default=1.0)
    parser.add_argument("--m", type=float, default=3.0)
    add_kernel_and_sampling(parser, 'Gaussian', 0.3, 1e-8, 1000, 486)
    add_gn_and_logs(parser, 'rdm', 6, method_choices=['elimination'])
    return parser.parse_args(argv)


def manufactured(alpha, m):
    """u* = prod_k sin(pi x_k) + 2 prod_k sin(2 pi x_k) and f = -Laplace(u*) + alpha u*^m"""
    pi = onp.pi

    def modes(x1, x2, x3):
        return (onp.sin(pi * x1) * onp.sin(pi * x2) * onp.sin(pi * x3),
                onp.sin(2 * pi * x1) * onp.sin(2 * pi * x2) * onp.sin(2 * pi * x3))

    def u(x1, x2, x3):
        s1, s2 = modes(x1, x2, x3)
        return s1 + 2 * s2

    def f(x1, x2, x3):
        s1, s2 = modes(x1, x2, x3)
        lap = -3 * pi ** 2 * s1 - 24 * pi ** 2 * s2
        return -lap + alpha * (u(x1, x2, x3) ** m)
    return u, f


def cube_grid(n=GRID):
    """n^3 tensor grid on the unit cube, faces included: (n^3, 3) points"""
    g = onp.linspace(0.0, 1.0, n)
    return onp.stack([a.ravel() for a in onp.meshgrid(g, g, g, indexing='ij')], axis=1)


def main(argv=None):
    cfg = parse(argv)
    cfg.show_figure = False                                              # accepted and ignored
    u, f = manufactured(cfg.alpha, cfg.m)
    solver, _ = solve_forward(cfg, "Nonlinear_elliptic3d", u, f, UNIT_CUBE, solve_kwargs={'method': cfg.method}, verbose=cfg.print_hist)
    Xd = solver.eqn.X_domain
    solver.collocation_pts_err(u(Xd[:, 0], Xd[:, 1], Xd[:, 2]))          # error on the collocation points
    X_test = cube_grid()
    report_test_error(solver, False, None, None, X_test, u(X_test[:, 0], X_test[:, 1], X_test[:, 2]))
    report_test_residual(cfg, solver, X_test)


if __name__ == '__main__':
    main()
