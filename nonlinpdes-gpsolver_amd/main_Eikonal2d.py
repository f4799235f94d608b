#%%
"""Regularised Eikonal equation |grad u|^2 = f + eps*Delta u on [0,1]^2 with the GP solver on an MI355X.
Same command line as the reference's main_Eikonal2d.py.
--kernel periodic_Gaussian --kernel_parameter S1 S2 --period 1 0 (or 0 1; no counterpart in the reference): periodic along that axis, u = 0
on the two faces of the other one.  With f = 1 the solution then depends on the other coordinate alone and the Cole-Hopf transform gives
it in closed form (periodic_truth), which is what the test error is taken against."""
import argparse

import numpy as onp

from _driver_common import add_gn_and_logs, add_kernel_and_sampling, periodic_axes_of, report_test_error, report_test_residual, report_test_variance, report_posterior_samples, solve_forward, tensor_grid
from reference_solver.Cole_Hopf_for_Eikonal import solve_Eikonal

UNIT_SQUARE = [[0, 1], [0, 1]]


def parse(argv=None):
    parser = argparse.ArgumentParser(description='Eikonal equation GP solver')
    parser.add_argument("--eps", type=float, default=1e-1)
    add_kernel_and_sampling(parser, 'Gaussian', 0.2, 1e-5, 1000, 200)
    add_gn_and_logs(parser, 'zero', 8)
    return parser.parse_args(argv)


def periodic_truth(eps, x):
    """u = -eps log v with eps^2 v'' = v, v = 1 at x = 0 and x = 1: v = cosh((x - 1/2) / eps) / cosh(1 / (2 eps)), written without overflow"""
    a, b = onp.abs(x - 0.5) / eps, 0.5 / eps
    return -eps * (a - b + onp.log1p(onp.exp(-2 * a)) - onp.log1p(onp.exp(-2 * b)))


def main(argv=None):
    cfg = parse(argv)
    periodic = periodic_axes_of(cfg)
    solver, show = solve_forward(cfg, "Eikonal", lambda x1, x2: 0, lambda x1, x2: 1, UNIT_SQUARE)
    # test points: interior of a 60 x 60 grid; truth by the Cole-Hopf transform + finite differences on the same grid
    n = 60
    _, _, X_test = tensor_grid(n, *UNIT_SQUARE, interior=True)
    XX, YY, truth = solve_Eikonal(n - 2, cfg.eps)
    if any(periodic):
        truth = periodic_truth(cfg.eps, X_test[:, 0 if periodic[1] else 1])
    report_test_error(solver, show, XX, YY, X_test, truth.flatten())
    report_test_residual(cfg, solver, X_test)
    report_test_variance(cfg, solver, X_test)
    report_posterior_samples(cfg, solver, X_test)


if __name__ == '__main__':
    main()
