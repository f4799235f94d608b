"""gpk_extend_functionals on the device: every layout x both kernels against the host expectation (test_extend_functionals_host.expect),
central differences of gpk_extend, masks and edges, argument checks, and the collocation identity of a real solve."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'nonlinpdes-gpsolver_amd')
if PKG not in sys.path:
    sys.path.insert(0, PKG)

import test_extend_functionals_host as H  # noqa: E402

EPS = H.EPS
LAYOUTS = ('Nonlinear_elliptic', 'Burgers', 'Eikonal', 'Darcy_u', 'Darcy_a')


@pytest.fixture(scope='module')
def ctx():
    from src._runtime import get_context
    return get_context()


def _problem(seed=0, Nd=150, Nb=40, Nt=300):
    """random collocation points, test points that include collocation points and points outside the domain, coefficients of mixed
    signs and magnitudes 1 .. 1e6 (as long as the largest layout needs)"""
    rng = np.random.RandomState(seed)
    Xd = rng.uniform(0, 1, (Nd, 2)); Xb = rng.uniform(0, 1, (Nb, 2))
    Xt = np.concatenate([rng.uniform(-0.3, 1.3, (Nt - 60, 2)), Xd[:40], Xb[:20]], axis=0)
    coeff = rng.choice([-1.0, 1.0], 4 * Nd + Nb) * 10.0 ** rng.uniform(0, 6, 4 * Nd + Nb)
    return Xd, Xb, Xt, coeff


def _ncols(layout, Nd, Nb):
    return {'Nonlinear_elliptic': 2 * Nd + Nb, 'Darcy_a': 3 * Nd}.get(layout, 4 * Nd + Nb)


@pytest.mark.parametrize('kernel,kp', H.KERNELS)
@pytest.mark.parametrize('layout', LAYOUTS)
def test_every_functional_matches_the_host_expectation(ctx, layout, kernel, kp):
    Xd, Xb, Xt, coeff = _problem()
    c = coeff[:_ncols(layout, len(Xd), len(Xb))]
    got = ctx.extend_functionals(layout, kernel, kp, Xt, Xd, Xb, c, which=H.FUNCTIONALS).download()
    assert got.shape == (5, len(Xt))
    worst = 0.0
    for k, fn in enumerate(H.FUNCTIONALS):
        ref, terms = H.expect(layout, fn, Xt, Xd, Xb, c, kernel, kp)
        err = np.abs(got[k] - ref)
        worst = max(worst, float(np.max(err / (EPS * terms))))
        assert np.all(err <= 64 * EPS * terms), (fn, np.max(err / (EPS * terms)))
    ext = ctx.extend(layout, kernel, kp, Xt, Xd, Xb, c).download()
    _, terms0 = H.expect(layout, 'value', Xt, Xd, Xb, c, kernel, kp)
    assert np.all(np.abs(got[0] - ext) <= 64 * EPS * terms0), np.max(np.abs(got[0] - ext) / (EPS * terms0))
    print(f'\n[{layout}/{kernel}] max |dev - ref| / (eps sum|terms|) = {worst:.2f}; value row vs gpk_extend: '
          f'{np.max(np.abs(got[0] - ext)):.2e} (bitwise equal: {np.array_equal(got[0], ext)})')


@pytest.mark.parametrize('kernel,kp', H.KERNELS)
@pytest.mark.parametrize('layout', ('Nonlinear_elliptic', 'Burgers', 'Darcy_a'))
def test_derivatives_match_central_differences_of_the_extension(ctx, layout, kernel, kp):
    """h = 1e-3 x the axis length scale: truncation of the central differences ~1e-7 relative, rounding ~1e-13 (first) / 1e-10 (second)"""
    rng = np.random.RandomState(1)
    Nd, Nb = 120, 30
    Xd = rng.uniform(0, 1, (Nd, 2)); Xb = rng.uniform(0, 1, (Nb, 2)); Xt = rng.uniform(0.1, 0.9, (64, 2))
    c = rng.normal(size=_ncols(layout, Nd, Nb))
    p1, p2 = H.O.kernel_precisions(kernel, kp)
    h = (1e-3 / np.sqrt(p1), 1e-3 / np.sqrt(p2))
    got = ctx.extend_functionals(layout, kernel, kp, Xt, Xd, Xb, c, which=('d1', 'd2', 'd2d2')).download()
    ext = lambda X: ctx.extend(layout, kernel, kp, X, Xd, Xb, c).download()
    u0 = ext(Xt)
    fd = []
    for ax in (0, 1):
        e = np.zeros(2); e[ax] = h[ax]
        up, um = ext(Xt + e), ext(Xt - e)
        fd.append((up - um) / (2 * h[ax]))
        if ax == 1:
            fd.append((up - 2 * u0 + um) / (h[ax] * h[ax]))
    for k, name in enumerate(('d1', 'd2', 'd2d2')):
        rel = np.linalg.norm(got[k] - fd[k]) / np.linalg.norm(got[k])
        print(f'\n[{layout}/{kernel}] {name} vs central difference: {rel:.2e}')
        assert rel < 1e-5, (name, rel)


def test_masks_and_row_order(ctx):
    Xd, Xb, Xt, coeff = _problem(2)
    layout, (kernel, kp) = 'Eikonal', H.KERNELS[0]
    c = coeff[:_ncols(layout, len(Xd), len(Xb))]
    full = ctx.extend_functionals(layout, kernel, kp, Xt, Xd, Xb, c, which=H.FUNCTIONALS).download()
    for k, fn in enumerate(H.FUNCTIONALS):                                # every single-bit mask: the same numbers as in the full mask
        one = ctx.extend_functionals(layout, kernel, kp, Xt, Xd, Xb, c, which=(fn,)).download().reshape(-1)
        assert np.array_equal(one, full[k]), fn
    rev = ctx.extend_functionals(layout, kernel, kp, Xt, Xd, Xb, c, which=('laplacian', 'value', 'd2')).download()
    assert np.array_equal(rev, full[[4, 0, 2]])
    again = ctx.extend_functionals(layout, kernel, kp, Xt, Xd, Xb, c, which=H.FUNCTIONALS).download()
    assert np.array_equal(again, full)                                    # fixed reduction order: bit-identical


@pytest.mark.parametrize('Nd,Nb,Nt', [(150, 40, 1), (200, 57, 5), (300, 212, 7), (1, 0, 3)])
def test_edges_small_counts_and_odd_sizes(ctx, Nd, Nb, Nt):
    """Nt = 1 and Nt not a multiple of the workgroup's test points; M = Nd + Nb not a multiple of 256 (257, 512 + some); one point"""
    rng = np.random.RandomState(Nd + Nt)
    Xd = rng.uniform(0, 1, (Nd, 2)); Xb = rng.uniform(0, 1, (Nb, 2)); Xt = rng.uniform(0, 1, (Nt, 2))
    for layout in ('Nonlinear_elliptic', 'Burgers'):
        c = rng.normal(size=_ncols(layout, Nd, Nb))
        got = ctx.extend_functionals(layout, 'Gaussian', 0.2, Xt, Xd, Xb, c, which=H.FUNCTIONALS).download().reshape(5, Nt)
        for k, fn in enumerate(H.FUNCTIONALS):
            ref, terms = H.expect(layout, fn, Xt, Xd, Xb, c, 'Gaussian', 0.2)
            assert np.all(np.abs(got[k] - ref) <= 64 * EPS * terms), (layout, fn)


def _raw(ctx, Xt, Xd, Xb, c, layout=0, kernel=0, fmask=31, ldo=None, out=None, Nt=None, kp=(0.2, 0.0)):
    lib = ctx.lib
    dXt, dXd, dXb, dc = ctx.points(Xt), ctx.points(Xd), ctx.points(Xb), ctx.array(c)
    Nt = len(Xt) if Nt is None else Nt
    ldo = len(Xt) if ldo is None else ldo
    kpa = (C.c_double * 2)(*kp)
    return lib.gpk_extend_functionals(ctx.h, layout, kernel, kpa, dXt.ptr, Nt, dXd.ptr, len(Xd), dXb.ptr, len(Xb), dc.ptr, fmask,
                                      out.ptr if out is not None else dc.ptr, ldo)


def test_leading_dimension_leaves_the_padding_untouched(ctx):
    Xd, Xb, Xt, coeff = _problem(4, Nt=101)
    c = coeff[:_ncols('Nonlinear_elliptic', len(Xd), len(Xb))]
    Nt, ldo, mask = len(Xt), 128, 1 | 4 | 16
    out = ctx.empty(3, ldo, ld=ldo)
    sentinel = np.full((3, ldo), -7.25e300)
    out.upload(sentinel)
    assert _raw(ctx, Xt, Xd, Xb, c, fmask=mask, ldo=ldo, out=out) == 0
    got = out.download()
    assert np.array_equal(got[:, Nt:], sentinel[:, Nt:])
    ref = ctx.extend_functionals('Nonlinear_elliptic', 'Gaussian', 0.2, Xt, Xd, Xb, c, which=('value', 'd2', 'laplacian')).download()
    assert np.array_equal(got[:, :Nt], ref)


def test_invalid_arguments_return_9001(ctx):
    Xd, Xb, Xt, coeff = _problem(5, Nt=100)
    c = coeff[:_ncols('Nonlinear_elliptic', len(Xd), len(Xb))]
    out = ctx.empty(5, 128, ld=128)
    ok = dict(out=out, ldo=128)
    assert _raw(ctx, Xt, Xd, Xb, c, **ok) == 0
    assert _raw(ctx, Xt, Xd, Xb, c, fmask=0, **ok) == -9001
    assert _raw(ctx, Xt, Xd, Xb, c, fmask=32, **ok) == -9001
    assert _raw(ctx, Xt, Xd, Xb, c, fmask=33, **ok) == -9001
    assert _raw(ctx, Xt, Xd, Xb, c, out=out, ldo=99) == -9001           # ldo < Nt
    assert _raw(ctx, Xt, Xd, Xb, c, Nt=0, **ok) == -9001
    assert _raw(ctx, Xt, Xd, Xb, c, Nt=-1, **ok) == -9001
    assert _raw(ctx, Xt, Xd, Xb, c, layout=4, **ok) == -9001
    assert _raw(ctx, Xt, Xd, Xb, c, layout=-1, **ok) == -9001
    assert _raw(ctx, Xt, Xd, Xb, c, kernel=2, **ok) == -9001
    lib = ctx.lib
    f = ctx.array(np.zeros((4, 16))); r = ctx.empty(16); a = ctx.array(np.zeros((3, 16)))
    p = (C.c_double * 3)(1.0, 3.0, 0.0)
    assert lib.gpk_pde_residual(ctx.h, 0, p, 16, f.ptr, f.ld, None, 0, r.ptr, r.ptr) == 0
    assert lib.gpk_pde_residual(ctx.h, 3, None, 16, f.ptr, f.ld, None, 0, r.ptr, r.ptr) == -9001     # Darcy without fields_a
    assert lib.gpk_pde_residual(ctx.h, 3, None, 16, f.ptr, f.ld, a.ptr, a.ld, r.ptr, r.ptr) == 0
    assert lib.gpk_pde_residual(ctx.h, 5, p, 16, f.ptr, f.ld, None, 0, r.ptr, r.ptr) == -9001
    assert lib.gpk_pde_residual(ctx.h, -1, p, 16, f.ptr, f.ld, None, 0, r.ptr, r.ptr) == -9001
    assert lib.gpk_pde_residual(ctx.h, 0, p, 0, f.ptr, f.ld, None, 0, r.ptr, r.ptr) == -9001
    ctx.synchronize()


# ---- collocation identity of a real solve ------------------------------------------------------------------------------------------
def _solve(name):
    """(eqn, [(layout, L_host, coeff_host, sol_vec, nugget per block)]) after a real solve at driver sizes"""
    from src._runtime import get_context
    from _driver_common import solve_forward, tensor_grid
    ctx = get_context()
    if name == 'Nonlinear_elliptic':
        import main_NonLinElliptic2d as drv
        cfg = drv.parse(['--print_hist', '', '--show_figure', ''])          # 900 / 124, sigma 0.2, nugget 1e-13
        u, f = drv.manufactured(cfg.alpha, cfg.m)
        np.random.seed(0)
        s, _ = solve_forward(cfg, name, u, f, drv.UNIT_SQUARE, solve_kwargs={'method': 'elimination'}, verbose=False)
    elif name == 'Eikonal':
        import main_Eikonal2d as drv
        cfg = drv.parse(['--print_hist', '', '--show_figure', ''])
        np.random.seed(0)
        s, _ = solve_forward(cfg, name, lambda x1, x2: 0, lambda x1, x2: 1, drv.UNIT_SQUARE, verbose=False)
    elif name == 'Burgers':
        import main_Burgers1d as drv
        from _driver_common import seed_from
        cfg = drv.parse(['--print_hist', '', '--show_figure', ''])
        seed_from(cfg)
        s, _ = solve_forward(cfg, name, drv.initial_and_lateral, lambda x1, x2: 0, drv.SPACE_TIME, verbose=False)
    else:
        import main_DarcyFlow2d as drv
        from src.solver import solver_GP
        cfg = drv.parse(['--print_hist', '', '--show_figure', ''])
        np.random.seed(cfg.randomseed)
        s = solver_GP(cfg, PDE_type='Darcy_flow2d')
        s.set_equation(bdy=lambda x1, x2: 0, rhs=drv.source, domain=np.array(drv.UNIT_SQUARE), print_option=False)
        s.auto_sample_IP(cfg.N_domain, cfg.N_boundary, cfg.N_data, print_option=False)
        XX, YY, _ = tensor_grid(drv.GRID, *drv.UNIT_SQUARE)                 # the driver's observations: FD solution, interpolated
        u_grid = drv.FD_Darcy_flow_2d(drv.GRID - 2, drv.permeability, drv.source)
        Xo = s.eqn.X_data
        obs = drv.griddata((XX.flatten(), YY.flatten()), u_grid.reshape(-1, 1), (Xo[:, 0], Xo[:, 1]), method='linear')[:, 0]
        s.get_observed_data(obs, cfg.noise_level, print_option=False)
        s.solve(print_option=False)
    e = s.eqn
    out = []
    parts = ([('Darcy_u', e._dL_u, e.sol_vec_u, e.L_u), ('Darcy_a', e._dL_a, e.sol_vec_a, e.L_a)] if name == 'Darcy_flow2d'
             else [(e._layout, e._dL, e.sol_vec, e.L)])
    for layout, dL, vec, Lh in parts:
        coeff = ctx.array(vec); ctx.potrs(dL, coeff, nrhs=1)
        T, ratios = ctx.assemble(layout, cfg.kernel, cfg.kernel_parameter, e.X_domain, e.X_boundary, cfg.nugget, cfg.nugget_type)
        T.free()
        nb = len(H.BLOCKS[layout])
        nug = [cfg.nugget * (ratios[b] if b < nb - 1 else 1.0) for b in range(nb)]
        out.append((layout, Lh, coeff.download(), np.asarray(vec), nug))
    return e, cfg, out


@pytest.mark.parametrize('name', ('Nonlinear_elliptic', 'Eikonal', 'Burgers', 'Darcy_flow2d'))
def test_collocation_identity_after_a_real_solve(ctx, name):
    """Theta_lambda coeff = sol_vec, Theta_lambda = Theta + diag(nugget_b): the functional of block b evaluated at block b's collocation
    points equals sol_vec_b - nugget_b coeff_b.  Bound: the kernel's rounding (64 eps sum|terms|) plus the backward error of the
    Cholesky solve that produced coeff, (3n+1) eps (|L| |L^T| |coeff|) (Higham, Accuracy and Stability, Thm 10.4)."""
    e, cfg, parts = _solve(name)
    for layout, Lh, coeff, vec, nug in parts:
        n = coeff.size
        chol = np.abs(Lh) @ (np.abs(Lh).T @ np.abs(coeff))
        pts = {'d': e.X_domain, 'db': np.concatenate([e.X_domain, e.X_boundary], axis=0)}
        off, worst = 0, 0.0
        for b, (fn, which) in enumerate(H.BLOCKS[layout]):
            X = pts[which]
            got = ctx.extend_functionals(layout, cfg.kernel, cfg.kernel_parameter, X, e.X_domain, e.X_boundary, coeff,
                                         which=(fn,)).download().reshape(-1)
            sl = slice(off, off + len(X))
            want = vec[sl] - nug[b] * coeff[sl]
            _, terms = H.expect(layout, fn, X, e.X_domain, e.X_boundary, coeff, cfg.kernel, cfg.kernel_parameter)
            bound = 64 * EPS * (terms + nug[b] * np.abs(coeff[sl])) + (3 * n + 1) * EPS * chol[sl]
            err = np.abs(got - want)
            worst = max(worst, float(np.max(err / bound)))
            assert np.all(err <= bound), (layout, fn, np.max(err / bound))
            off += len(X)
        print(f'\n[{name}/{layout}] collocation identity: max error / bound = {worst:.3e}')
