#%%
"""Monge-Ampere equation det D^2 u = f on [0,1]^2, u = g on the boundary, convex solution, with the GP solver on an MI355X (no
counterpart in the reference).  Solved as Delta u = sqrt((u_11 - u_22)^2 + (2 u_12)^2 + 4 f) on the Hessian Gram layout:
    python main_MongeAmpere2d.py --N_domain 600 --N_boundary 120 --kernel_parameter 0.2 --nugget 1e-8 --GNsteps 8 --show_figure ""
The manufactured solution is u* = exp(|x - c|^2 / 2), c = (1/2, 1/2), with f = (1 + |x - c|^2) exp(|x - c|^2).  --line_search 1 for
configurations in which the plain iteration does not settle."""
import argparse

import numpy as onp

from _driver_common import (add_gn_and_logs, add_kernel_and_sampling, report_test_error, report_test_residual, report_test_variance,
                            report_posterior_samples, solve_forward, tensor_grid)

UNIT_SQUARE = [[0, 1], [0, 1]]


def parse(argv=None):
    parser = argparse.ArgumentParser(description='Monge-Ampere equation det D^2 u = f, GP solver')
    add_kernel_and_sampling(parser, 'Gaussian', 0.3, 1e-8, 600, 120)
    add_gn_and_logs(parser, 'zero', 8)
    return parser.parse_args(argv)


def manufactured():
    """u* = exp(r^2 / 2) and f = det D^2 u* = (1 + r^2) exp(r^2), r = |x - (1/2, 1/2)|"""
    def r2(x1, x2):
        return (x1 - 0.5) ** 2 + (x2 - 0.5) ** 2

    def u(x1, x2):
        return onp.exp(0.5 * r2(x1, x2))

    def f(x1, x2):
        return (1.0 + r2(x1, x2)) * onp.exp(r2(x1, x2))
    return u, f


def main(argv=None):
    cfg = parse(argv)
    u, f = manufactured()
    solver, show = solve_forward(cfg, "MongeAmpere2d", u, f, UNIT_SQUARE, verbose=cfg.print_hist)
    Xd = solver.eqn.X_domain
    solver.collocation_pts_err(u(Xd[:, 0], Xd[:, 1]))                    # error on the collocation points
    XX, YY, X_test = tensor_grid(60, *UNIT_SQUARE)                       # error on a 60 x 60 test grid
    report_test_error(solver, show, XX, YY, X_test, u(X_test[:, 0], X_test[:, 1]))
    report_test_residual(cfg, solver, X_test)
    report_test_variance(cfg, solver, X_test)
    report_posterior_samples(cfg, solver, X_test)


if __name__ == '__main__':
    main()
