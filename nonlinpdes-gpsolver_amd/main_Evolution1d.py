#%%
"""Evolution equations u_t + alpha u u_x + Q[u] = f with Q = c2 u_xx + c3 u_xxx + c4 u_xxxx + c5 u_xxxxx on (t,x) in [0,1]x[-1,1] with the
GP solver on an MI355X (no counterpart in the reference).  The Burgers system on the evolution Gram layout (rows u_t, u_x, Q u, u):
    python main_Evolution1d.py --equation kuramoto_sivashinsky --bc clamped --show_figure ""      # u_t + u u_x + u_xx + u_xxxx = f
    python main_Evolution1d.py --equation kawahara 1.0 -0.5 --show_figure ""                    # u_t + u u_x + u_xxx - u_xxxxx / 2 = f
    python main_Evolution1d.py --coeffs -0.1 0.5 0.0 0.0 --show_figure ""                         # KdV-Burgers
The truth is the manufactured smooth solution u* = exp(-t) sin(pi x) with the forcing f = u*_t + alpha u* u*_x + Q[u*]; its values are the
data at t = 0 and on the walls x = -1, 1.  --bc clamped adds u_x = u*_x on the walls (two conditions per wall, what an operator of fourth
order takes: every wall point is used twice); --bc dirichlet leaves the remaining conditions to the minimum-norm interpolant.
--test_variance reports that the posterior is not served for this layout."""
import argparse

import numpy as onp

from _driver_common import add_gn_and_logs, add_kernel_and_sampling, report_test_error, report_test_residual, seed_from, solve_forward, tensor_grid

SPACE_TIME = [[0, 1], [-1, 1]]
_ARITY = {'kuramoto_sivashinsky': 0, 'kawahara': 2, 'kdv_burgers': 2, 'benney_lin': 4}


def parse(argv=None):
    parser = argparse.ArgumentParser(description='Evolution equation (general spatial operator) GP solver')
    parser.add_argument("--alpha", type=float, default=1.0)
    parser.add_argument("--equation", type=str, nargs='+', default=None,
                        help='kuramoto_sivashinsky | kawahara a b | kdv_burgers nu delta | benney_lin c2 c3 c4 c5 (default: kuramoto_sivashinsky)')
    parser.add_argument("--coeffs", type=float, nargs=4, default=None, help='c2 c3 c4 c5, instead of --equation')
    parser.add_argument("--bc", type=str, default=None, choices=['dirichlet', 'clamped'],
                        help='default: clamped where the operator has a fourth or fifth derivative, else dirichlet')
    add_kernel_and_sampling(parser, 'anisotropic_Gaussian', [0.6, 0.5], 1e-8, 1000, 200, kp_nargs='+')
    add_gn_and_logs(parser, 'rdm', 8)
    parser.add_argument("--randomseed", type=int, default=0)
    cfg = parser.parse_args(argv)
    if cfg.coeffs is not None and cfg.equation is not None:
        parser.error('--coeffs and --equation exclude each other')
    if cfg.coeffs is None:
        name, args = (cfg.equation or ['kuramoto_sivashinsky'])[0], (cfg.equation or [None])[1:]
        if name not in _ARITY or len(args) != _ARITY[name]:
            parser.error(f'--equation {name}: takes {_ARITY.get(name, "?")} numbers; names: {", ".join(_ARITY)}')
        cfg.equation = (name,) + tuple(float(v) for v in args)
    return cfg


def manufactured(alpha, c):
    """u* = exp(-t) sin(pi x), u*_x and f = u*_t + alpha u* u*_x + Q[u*]"""
    c2, c3, c4, c5 = c
    pi = onp.pi

    def u(t, x):
        return onp.exp(-t) * onp.sin(pi * x)

    def ux(t, x):
        return pi * onp.exp(-t) * onp.cos(pi * x)

    def f(t, x):
        return -u(t, x) + alpha * u(t, x) * ux(t, x) + (c4 * pi ** 4 - c2 * pi ** 2) * u(t, x) + (c5 * pi ** 4 - c3 * pi ** 2) * ux(t, x)
    return u, ux, f


def main(argv=None):
    cfg = parse(argv)
    seed_from(cfg)
    if cfg.kernel == 'periodic_Gaussian' or cfg.period:
        raise SystemExit('--kernel periodic_Gaussian / --period: the evolution layout takes Gaussian or anisotropic_Gaussian')
    from src.PDEs import Evolution1d
    probe = Evolution1d(alpha=cfg.alpha, coeffs=cfg.coeffs, equation=cfg.equation if cfg.coeffs is None else None)
    if cfg.bc is None:
        cfg.bc = 'clamped' if probe.coeffs[2] != 0.0 or probe.coeffs[3] != 0.0 else 'dirichlet'
    u, ux, f = manufactured(cfg.alpha, probe.coeffs)
    cfg.bdy_x = ux
    if cfg.coeffs is not None:
        cfg.equation = None
    solver, show = solve_forward(cfg, "Evolution1d", u, f, SPACE_TIME)
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
