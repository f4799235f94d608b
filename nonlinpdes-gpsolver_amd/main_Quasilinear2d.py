#%%
"""Quasilinear equations on [0,1]^2, u = g on the boundary, with the GP solver on an MI355X (no counterpart in the reference): equations
whose second-order coefficients depend on grad u, on the 2-jet Gram layout (rows d_1 u, d_2 u, (d_11 - d_22) u, 2 d_12 u, Laplace(u), u).
    python main_Quasilinear2d.py --equation mean_curvature --kappa 1.0 --N_domain 600 --N_boundary 120 --GNsteps 8 --show_figure ""
    python main_Quasilinear2d.py --equation p_laplace --m 3 --delta 1.0 --N_domain 600 --N_boundary 120 --GNsteps 8 --show_figure ""
    python main_Quasilinear2d.py --equation gauss_curvature --e 2 --N_domain 600 --N_boundary 120 --GNsteps 8 --show_figure ""
Manufactured solutions: u* = amplitude sin(pi x1) sin(pi x2) for the mean-curvature equation and the p-Laplacian, the convex
u* = exp(|x - c|^2 / 2), c = (1/2, 1/2), for the Gauss-curvature equation; f is the equation's left-hand side at u* (src/quasilinear.py).
--line_search 1 for configurations in which the plain iteration does not settle."""
import argparse

import numpy as onp

from _driver_common import add_gn_and_logs, add_kernel_and_sampling, report_test_error, report_test_residual, solve_forward, tensor_grid

UNIT_SQUARE = [[0, 1], [0, 1]]


def parse(argv=None):
    parser = argparse.ArgumentParser(description='Quasilinear equations (mean curvature, p-Laplacian, Gauss curvature), GP solver')
    parser.add_argument('--equation', type=str, default='mean_curvature', choices=['mean_curvature', 'p_laplace', 'gauss_curvature'])
    parser.add_argument('--kappa', type=float, default=1.0, help='mean_curvature: div(grad u / sqrt(1 + |grad u|^2)) = f + kappa u')
    parser.add_argument('--m', type=float, default=3.0, help='p_laplace: the exponent (m = 2 is Poisson\'s equation)')
    parser.add_argument('--delta', type=float, default=1.0, help='p_laplace: the regularisation delta > 0')
    parser.add_argument('--e', type=float, default=2.0, help='gauss_curvature: det D^2 u = f (1 + |grad u|^2)^e (2: Gauss curvature f)')
    parser.add_argument('--amplitude', type=float, default=0.5, help='amplitude of the manufactured solution (mean_curvature, p_laplace)')
    add_kernel_and_sampling(parser, 'Gaussian', 0.3, 1e-8, 600, 120)
    add_gn_and_logs(parser, 'zero', 8)
    return parser.parse_args(argv)


def equation_of(cfg):
    return {'mean_curvature': ('mean_curvature', cfg.kappa), 'p_laplace': ('p_laplace', cfg.m, cfg.delta),
            'gauss_curvature': ('gauss_curvature', cfg.e)}[cfg.equation]


def manufactured(eq, amplitude=0.5):
    """(u*, f) for the QuasilinearEquation eq: f = the equation's left-hand side at u*"""
    pi = onp.pi
    if eq.kind == 'gauss_curvature':
        def jet(x1, x2):
            a, b = x1 - 0.5, x2 - 0.5
            u = onp.exp(0.5 * (a * a + b * b))
            return u, a * u, b * u, (1.0 + a * a) * u, a * b * u, (1.0 + b * b) * u
    else:
        def jet(x1, x2):
            s1, s2, c1, c2 = onp.sin(pi * x1), onp.sin(pi * x2), onp.cos(pi * x1), onp.cos(pi * x2)
            A = amplitude
            return A * s1 * s2, A * pi * c1 * s2, A * pi * s1 * c2, -A * pi * pi * s1 * s2, A * pi * pi * c1 * c2, -A * pi * pi * s1 * s2

    def u(x1, x2):
        return jet(x1, x2)[0]

    def f(x1, x2):
        return eq.rhs_of(*jet(x1, x2))
    return u, f


def main(argv=None):
    from src.quasilinear import QuasilinearEquation
    cfg = parse(argv)
    cfg.equation = QuasilinearEquation.make(equation_of(cfg))
    u, f = manufactured(cfg.equation, cfg.amplitude)
    solver, show = solve_forward(cfg, "Quasilinear2d", u, f, UNIT_SQUARE, verbose=cfg.print_hist)
    Xd = solver.eqn.X_domain
    solver.collocation_pts_err(u(Xd[:, 0], Xd[:, 1]))                    # error on the collocation points
    XX, YY, X_test = tensor_grid(60, *UNIT_SQUARE)                       # error on a 60 x 60 test grid
    report_test_error(solver, show, XX, YY, X_test, u(X_test[:, 0], X_test[:, 1]))
    report_test_residual(cfg, solver, X_test)
    return solver


if __name__ == '__main__':
    main()
