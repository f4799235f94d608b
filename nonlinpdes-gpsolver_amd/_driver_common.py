"""Shared argparse helpers of the main_*.py drivers (same flag names, types and defaults as the reference's drivers)."""


import argparse


class _ScalarOrList(argparse.Action):
    """--kernel_parameter of the drivers whose default kernel takes one value: one value is stored as a float, as before; several (the
    two length scales of --kernel periodic_Gaussian) as a list"""

    def __call__(self, parser, namespace, values, option_string=None):
        setattr(namespace, self.dest, values[0] if len(values) == 1 else list(values))


def add_kernel_and_sampling(parser, kernel, kernel_parameter, nugget, N_domain, N_boundary, kp_nargs=None):
    parser.add_argument("--kernel", type=str, default=kernel)
    if kp_nargs:
        parser.add_argument("--kernel_parameter", type=float, nargs=kp_nargs, default=kernel_parameter)
    else:
        parser.add_argument("--kernel_parameter", type=float, nargs='+', action=_ScalarOrList, default=kernel_parameter)
    # --kernel periodic_Gaussian --period L1 L2: the period of each axis, 0 = not periodic (solver_GP: cfg.period); a periodic axis
    # gets no boundary points and must be as wide as its period
    parser.add_argument("--period", type=float, nargs=2, default=None)
    parser.add_argument("--nugget", type=float, default=nugget)
    parser.add_argument("--nugget_type", type=str, default="adaptive", choices=["adaptive", "identity", 'none'])
    parser.add_argument("--sampled_type", type=str, default='random', choices=['random', 'grid'])
    parser.add_argument("--N_domain", type=int, default=N_domain)
    parser.add_argument("--N_boundary", type=int, default=N_boundary)


def add_gn_and_logs(parser, initial_sol, GNsteps, method_choices=None):
    if method_choices:
        parser.add_argument("--method", type=str, default='elimination', choices=method_choices)
    else:
        parser.add_argument("--method", type=str, default='elimination')
    parser.add_argument("--initial_sol", type=str, default=initial_sol)
    parser.add_argument("--GNsteps", type=int, default=GNsteps)
    parser.add_argument("--step_size", type=int, default=1)
    # type=bool as in the reference: any non-empty string is True; pass --show_figure "" to disable
    parser.add_argument("--print_hist", type=bool, default=True)
    parser.add_argument("--show_figure", type=bool, default=True)
    # opt-in: also print the PDE residual of the solution on the test grid (no truth solution needed)
    parser.add_argument("--test_residual", type=bool, default=False)
    # opt-in: also print the posterior standard deviation of the solution on the test grid (Gauss-Newton / Laplace form)
    parser.add_argument("--test_variance", type=bool, default=False)
    # opt-in: choose --kernel_parameter among these by the Laplace log evidence (solver_GP.select_kernel_parameter): a comma-separated
    # list of scalars, or per-axis groups separated by ';' ("0.3,0.05;0.2,0.05"); --select_refine K: K golden-section steps (scalars only)
    # opt-in: also draw K samples of the solution on the test grid from its joint posterior (solver_GP.test_samples) and print their
    # spread about the mean; --sample_seed S seeds the standard normals (numpy.random.RandomState(S))
    # opt-in: backtracking line search in every Gauss-Newton step (src/linesearch.py): K trial steps step_size * shrink^k, Armijo constant c1
    parser.add_argument("--line_search", type=bool, default=False)
    parser.add_argument("--ls_trials", type=int, default=8)
    parser.add_argument("--ls_shrink", type=float, default=0.5)
    parser.add_argument("--ls_c1", type=float, default=1e-4)
    parser.add_argument("--posterior_samples", type=int, default=0)
    parser.add_argument("--sample_seed", type=int, default=None)
    parser.add_argument("--select_kernel_parameter", type=str, default=None)
    parser.add_argument("--select_refine", type=int, default=0)


NL_DEFAULTS = {'exp': (-1.0, 1.0), 'sinh': (1.0, 1.0), 'sin': (1.0, 1.0), 'cubic': (-1.0, 0.0, 1.0)}


def add_nonlinearity(parser):
    """--nonlinearity / --nl_params of the elliptic drivers: the reaction term tau(u) of -psi[u] + tau(u) = f (src/nonlinearity.py)"""
    parser.add_argument("--nonlinearity", type=str, default='power', choices=['power', 'exp', 'sinh', 'sin', 'cubic'])
    # comma-separated parameters of tau: p0,p1 (exp, sinh, sin: p0*fn(p1*u); power: alpha,m) or c1,c2,c3 (cubic: c1*u + c2*u^2 + c3*u^3)
    parser.add_argument("--nl_params", type=str, default=None)


def nonlinearity_from(cfg):
    """(tau, spec): the Nonlinearity the command line asks for and what goes into cfg.nonlinearity -- None for `power` without
    --nl_params, which is the equation alpha*u^m of --alpha / --m, untouched"""
    from src.nonlinearity import Nonlinearity
    params = None if cfg.nl_params is None else tuple(float(v) for v in cfg.nl_params.split(',') if v.strip())
    if cfg.nonlinearity == 'power':
        if params is None:
            return Nonlinearity.power(cfg.alpha, cfg.m), None
        if len(params) != 2:
            raise SystemExit('--nonlinearity power takes --nl_params alpha,m')
        cfg.alpha, cfg.m = params
        return Nonlinearity.power(cfg.alpha, cfg.m), None
    try:
        tau = Nonlinearity(cfg.nonlinearity, *(params if params is not None else NL_DEFAULTS[cfg.nonlinearity]))
    except ValueError as e:
        raise SystemExit(f'--nl_params: {e}')
    return tau, tau


def periodic_axes_of(cfg):
    """(axis 1 periodic, axis 2 periodic) of --period; the flag needs --kernel periodic_Gaussian and the kernel needs the flag"""
    period = getattr(cfg, 'period', None)
    if (cfg.kernel == 'periodic_Gaussian') != bool(period and any(period)):
        raise SystemExit('--kernel periodic_Gaussian and --period L1 L2 (one of them > 0) go together')
    return (False, False) if not period else (period[0] > 0, period[1] > 0)


def figures_enabled(cfg):
    """Figures need matplotlib and a display backend; without them the drivers run headless and say so."""
    if not cfg.show_figure:
        return False
    try:
        import matplotlib
        import os
        if not os.environ.get('DISPLAY') and matplotlib.get_backend().lower() not in ('agg',):
            matplotlib.use('Agg')
        return True
    except Exception as e:          # pragma: no cover
        print(f'[Figures] disabled ({e})')
        return False


def tensor_grid(n, range1, range2, interior=False):
    """n x n tensor grid on range1 x range2 (meshgrid order of the reference drivers); interior drops the boundary layer.
    Returns (XX, YY, points) with points of shape (n_eff^2, 2)."""
    import numpy as onp
    a = onp.linspace(range1[0], range1[1], n)
    b = onp.linspace(range2[0], range2[1], n)
    if interior:
        a, b = a[1:-1], b[1:-1]
    XX, YY = onp.meshgrid(a, b)
    return XX, YY, onp.concatenate((XX.reshape(-1, 1), YY.reshape(-1, 1)), axis=1)


def seed_from(cfg):
    """Drivers with --randomseed seed numpy's legacy global generator first (collocation points, noise, initial guess)."""
    from numpy import random
    random.seed(cfg.randomseed)
    print(f"[Seeds] random seeds: {cfg.randomseed}")


def kernel_candidates(text):
    """--select_kernel_parameter: "0.1,0.2,0.3" -> [0.1, 0.2, 0.3]; "0.3,0.05;0.2,0.05" -> [[0.3, 0.05], [0.2, 0.05]]"""
    try:
        groups = [[float(v) for v in g.split(',') if v.strip()] for g in text.split(';') if g.strip()]
    except ValueError as e:
        raise SystemExit(f'--select_kernel_parameter: {e}')
    if not groups or not all(groups):
        raise SystemExit('--select_kernel_parameter: no candidates')
    return groups if ';' in text else groups[0]


def solve_or_select(cfg, solver, **solve_kwargs):
    """solver.solve(), or with --select_kernel_parameter the search over its candidates, which leaves the solver solved at the winner"""
    if getattr(cfg, 'select_kernel_parameter', None):
        # (its lines are what the flag asks for: printed whatever --print_hist says)
        solver.select_kernel_parameter(kernel_candidates(cfg.select_kernel_parameter), refine=cfg.select_refine,
                                       method=solve_kwargs.get('method', 'elimination'), print_option=True)
    else:
        solver.solve(**solve_kwargs)


def solve_forward(cfg, pde_type, bdy, rhs, domain, solve_kwargs=None, verbose=None):
    """The part every forward-problem driver shares: solver, equation, collocation points, Gauss-Newton solve (+ figures)."""
    import numpy as onp
    from src.solver import solver_GP
    show = figures_enabled(cfg)
    solver = solver_GP(cfg, PDE_type=pde_type)
    kw = {} if verbose is None else {'print_option': verbose}
    solver.set_equation(bdy=bdy, rhs=rhs, domain=onp.array(domain), **kw)
    solver.auto_sample(cfg.N_domain, cfg.N_boundary, sampled_type=cfg.sampled_type, **kw)
    if show:
        solver.show_sample()
    solve_or_select(cfg, solver, **dict(solve_kwargs or {}, **kw))
    if show:
        solver.show_loss_hist()
    return solver, show


def report_test_error(solver, show, XX, YY, X_test, truth):
    solver.test(X_test)
    solver.get_test_error(truth)
    if show:
        solver.contour_of_test_err(XX, YY)


def report_test_residual(cfg, solver, X_test):
    """--test_residual: the residual of the equation on the driver's test grid (solver_GP.test_residual)"""
    if cfg.test_residual:
        solver.test_residual(X_test)


def report_test_variance(cfg, solver, X_test):
    """--test_variance: the posterior standard deviation of the solution on the driver's test grid (solver_GP.test_variance)"""
    if cfg.test_variance:
        solver.test_variance(X_test)


def report_posterior_samples(cfg, solver, X_test):
    """--posterior_samples K: K draws of the solution on the driver's test grid from its joint posterior (solver_GP.test_samples)"""
    if getattr(cfg, 'posterior_samples', 0):
        solver.test_samples(X_test, cfg.posterior_samples, cfg.sample_seed)
