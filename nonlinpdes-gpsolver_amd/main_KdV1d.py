#%%
"""Korteweg-de Vries equation u_t + alpha u u_x + delta u_xxx = 0 on (t,x) in [0,1]x[-8,8] with the GP solver on an MI355X (no
counterpart in the reference).  The Burgers system on the dispersive Gram layout (rows u_t, u_x, u_xxx, u):
    python main_KdV1d.py --N_domain 1000 --N_boundary 200 --kernel_parameter 0.5 1.0 --nugget 1e-6 --GNsteps 10 --show_figure ""
The truth is the soliton u = (3 c / alpha) sech^2(sqrt(c / delta) (x - c t - x0) / 2), which solves the equation with f = 0; its values
are the data at t = 0 and on the lateral boundaries x = -8, 8.  The lateral boundary carries Dirichlet data only: the equation is of
third order in x and takes three lateral conditions, the third one (u_x at the right end) is not imposed -- the minimum-norm interpolant
supplies it.  --initial_sol rdm (the default) or profile: the data at t = 0 held constant in time.  --test_variance reports that the
posterior is not served for this layout."""
import argparse

import numpy as onp

from _driver_common import add_gn_and_logs, add_kernel_and_sampling, report_test_error, report_test_residual, seed_from, solve_forward, tensor_grid

SPACE_TIME = [[0, 1], [-8, 8]]


def parse(argv=None):
    parser = argparse.ArgumentParser(description='Korteweg-de Vries equation GP solver')
    parser.add_argument("--alpha", type=float, default=6.0)
    parser.add_argument("--delta", type=float, default=1.0)
    parser.add_argument("--c", type=float, default=2.0)          # speed of the soliton (its height is 3 c / alpha)
    parser.add_argument("--x0", type=float, default=-1.0)        # its position at t = 0
    add_kernel_and_sampling(parser, 'anisotropic_Gaussian', [0.5, 1.0], 1e-6, 1000, 200, kp_nargs='+')
    add_gn_and_logs(parser, 'rdm', 10)
    parser.add_argument("--randomseed", type=int, default=0)
    return parser.parse_args(argv)


def soliton(alpha, delta, c, x0):
    if c <= 0 or delta <= 0 or alpha == 0:
        raise SystemExit('--c and --delta must be positive and --alpha non-zero: the soliton is (3c/alpha) sech^2(sqrt(c/delta)(x - ct - x0)/2)')

    def u(t, x):
        return 3.0 * c / alpha / onp.cosh(0.5 * onp.sqrt(c / delta) * (x - c * t - x0)) ** 2
    return u


def main(argv=None):
    cfg = parse(argv)
    seed_from(cfg)
    if cfg.kernel == 'periodic_Gaussian' or cfg.period:
        raise SystemExit('--kernel periodic_Gaussian / --period: the dispersive layout takes Gaussian or anisotropic_Gaussian')
    u = soliton(cfg.alpha, cfg.delta, cfg.c, cfg.x0)
    solver, show = solve_forward(cfg, "KdV", u, lambda x1, x2: 0, SPACE_TIME)
    XX, YY, X_test = tensor_grid(60, *SPACE_TIME)
    report_test_error(solver, show, XX, YY, X_test, u(X_test[:, 0], X_test[:, 1]))
    report_test_residual(cfg, solver, X_test)
    if cfg.test_variance:
        try:
            solver.test_variance(X_test)
        except NotImplementedError as e:
            print(f'[Test variance] not available: {e}')


if __name__ == '__main__':
    main()
