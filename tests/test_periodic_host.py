"""The periodic kernel on the host: the table, the numpy class of src/kernels.py, the samplers, and the preconditions of the gates of
tests/test_gpu_periodic.py and tests/test_gpu_periodic_shapes.py.  No GPU.

  a  the table h0 .. h4 against the symbolic derivatives of kappa (sympy) at random (p, w, d), and its limit w -> 0 against the Hermite
     table of src/kernels.py
  b  every method of Periodic_kernel against the long-double reference of tests/_periodic_reference.py; the diagonal values
  c  the samplers: default arguments reproduce tests/golden/sampling.npz bit for bit, the periodic plans have no point on a dropped face
  d  the block gate rejects a planted error of 1e-11 max|block| in one entry, the extension gate likewise; the row subset of the large
     cases covers every column; KERNEL['periodic_Gaussian'] == 16 and the host refusals
"""
import os

import numpy as np
import pytest
import sympy as sp

import _periodic_reference as PR

from src import kernels as K
from src import sample_points as SP

LD = PR.LD
EPS = PR.EPS
G = os.path.join(os.path.dirname(__file__), 'golden')


# ------------------------------------------------------------------------------------------------ a. the table
def test_table_against_symbolic_derivatives():
    p, w, d = sp.symbols('p w d', positive=True)
    kappa = sp.exp(-(2 * p / w ** 2) * sp.sin(w * d / 2) ** 2)
    h = [sp.lambdify((p, w, d), (-1) ** m * sp.diff(kappa, d, m) / kappa, modules='mpmath') for m in range(5)]
    import mpmath
    mpmath.mp.dps = 40
    rng = np.random.RandomState(0)
    for _ in range(40):
        pv, L, dv = float(rng.uniform(1, 200)), float(rng.uniform(0.5, 3)), float(rng.uniform(-4, 4))
        got, _ = K._periodic_table(pv, L, np.float64(dv))
        wv = 2 * mpmath.pi / mpmath.mpf(L)
        want = [hm(mpmath.mpf(pv), wv, mpmath.mpf(dv)) for hm in h]
        # size of the terms of h_m: |s| <= p / w, |c| <= p, and w^2
        scale = [max(pv, float(wv) ** 2, (pv / float(wv)) ** 2) ** (m / 2) for m in range(5)]
        for m in range(5):
            assert abs(float(got[m] - want[m])) <= 64 * EPS * scale[m] * (1 + abs(float(want[m])) / scale[m]), (pv, L, dv, m)


def test_table_at_zero_and_in_the_limit_of_a_long_period():
    pv, L = 37.0, 1.25
    w = 2 * np.pi / L
    got, z = K._periodic_table(pv, L, np.float64(0.0))
    assert [float(v) for v in got] == [1.0, 0.0, -pv, 0.0, pv * (3 * pv + w * w)] and float(z) == 0.0
    rng = np.random.RandomState(1)
    for _ in range(20):
        pv, dv = float(rng.uniform(1, 100)), float(rng.uniform(-0.5, 0.5))
        L = 1e7                                                          # w^2 d^2 ~ 1e-13: the tables agree to that
        got, _ = K._periodic_table(pv, L, np.float64(dv))
        want = K._hermite(pv, dv)
        for m in range(5):
            assert abs(float(got[m]) - float(want[m])) <= 1e-11 * pv ** (m / 2) * (1 + abs(float(want[m])) / pv ** (m / 2)), (pv, dv, m)


def test_sincospi_reduces_exactly():
    x = np.array([0.0, 0.5, 1.0, 1.5, 2.0, -0.5, 3.0, 1e9 + 0.25, -7.75])
    s, c = K._sincospi(x)
    r = np.sqrt(0.5)
    np.testing.assert_allclose(s, [0, 1, 0, -1, 0, -1, 0, r, r], atol=2 * EPS, rtol=0)
    np.testing.assert_allclose(c, [1, 0, -1, 0, 1, 0, -1, r, r], atol=2 * EPS, rtol=0)
    assert s[2] == 0.0 and c[1] == 0.0                                   # sin(pi) and cos(pi / 2) are exact zeros
    y = np.random.RandomState(2).uniform(-5, 5, 50)
    s1, c1 = K._sincospi(y)
    s2, c2 = K._sincospi(-y)
    assert np.array_equal(s1, -s2) and np.array_equal(c1, c2)           # odd / even to the bit


# ------------------------------------------------------------------------------------------------ b. the numpy class
_F = {'_ID': PR.ID, '_D1': PR.D1, '_D2': PR.D2, '_DD2': PR.DD2, '_LAP': PR.LAP}


def _functional(spec):
    return tuple(tuple(t) for t in spec)


@pytest.mark.parametrize('param', PR.PARAMS)
def test_every_method_against_long_double(param):
    k = K.Periodic_kernel()
    assert set(K._METHODS) <= set(dir(k))
    rng = np.random.RandomState(3)
    L = np.array([param[2] or 1.0, param[3] or 1.0])
    X, Y = rng.uniform(-1, 2, (300, 2)) * L, rng.uniform(0, 1, (300, 2)) * L
    for name, (fx, fy) in K._METHODS.items():
        got = getattr(k, name)(X[:, 0], X[:, 1], Y[:, 0], Y[:, 1], param)
        want = PR.pair(param, _functional(fx), _functional(fy), X[:, 0], X[:, 1], Y[:, 0], Y[:, 1])
        scale = float(np.max(np.abs(want)))
        err = float(np.max(np.abs(got.astype(LD) - want))) / scale
        assert err < PR.NP_PRECONDITION, (name, err)


def test_class_refuses_bad_parameters():
    k = K.Periodic_kernel()
    for bad in ((0.2, 0.2), (0.2, 0.2, 0.0, 0.0), (0.0, 0.2, 1.0, 0.0), (0.2, 0.2, -1.0, 0.0), (0.2, float('nan'), 1.0, 0.0),
                (0.2, 0.2, float('inf'), 0.0)):
        with pytest.raises(ValueError):
            k.kappa(0.0, 0.0, 0.1, 0.1, bad)


@pytest.mark.parametrize('param', PR.PARAMS)
def test_diagonal_values(param):
    (p1, L1), (p2, L2) = PR.axes(param)
    w1 = 2 * PR.PI / L1 if L1 > 0 else LD(0)
    w2 = 2 * PR.PI / L2 if L2 > 0 else LD(0)
    h4 = (3 * p1 * p1 + w1 * w1 * p1, 3 * p2 * p2 + w2 * w2 * p2)
    want = {PR.ID: LD(1), PR.D1: p1, PR.D2: p2, PR.DD2: h4[1], PR.LAP: h4[0] + 2 * p1 * p2 + h4[1]}
    k = K.Periodic_kernel()
    for layout in PR.LAYOUTS:
        got = PR.diagonal_values(param, layout)
        for (f, _), v in zip(PR.LAYOUTS[layout], got):
            assert abs(v - want[f]) <= 8 * LD(np.finfo(LD).eps) * want[f], (layout, f)
            g64 = k._eval(list(f), list(f), 0.3, 0.4, 0.3, 0.4, param)
            assert abs(LD(float(g64)) - want[f]) <= 4 * EPS * want[f], (layout, f)


def test_images_have_the_same_entries():
    param = PR.PARAMS[2]
    rng = np.random.RandomState(4)
    X, Y = rng.uniform(0, 1, (50, 2)), rng.uniform(0, 1, (50, 2))
    shift = np.array([3 * param[2], -2 * param[3]])
    for f in (PR.ID, PR.D1, PR.LAP):
        a = PR.pair(param, f, PR.LAP, X[:, 0], X[:, 1], Y[:, 0], Y[:, 1])
        b = PR.pair(param, f, PR.LAP, (X + shift)[:, 0], (X + shift)[:, 1], Y[:, 0], Y[:, 1])
        assert float(np.max(np.abs(a - b))) <= 64 * EPS * float(np.max(np.abs(a)))     # (x + shift is rounded to float64)


# ------------------------------------------------------------------------------------------------ c. samplers
def test_default_arguments_reproduce_the_golden_points():
    d = np.load(os.path.join(G, 'sampling.npz'))
    for name in sorted({k.split('__')[0] for k in d.files}):
        nd, nb, a, b, c, e, td, seed = d[name + '__args']
        dom = np.array([[a, b], [c, e]])
        for kw in ({}, {'periodic': (False, False)}):
            if name.startswith('grid'):
                Xd, Xb = SP.sampled_pts_grid(int(nd), int(nb), dom, bool(td), **kw)
            else:
                np.random.seed(int(seed))
                Xd, Xb = SP.sampled_pts_rdm(int(nd), int(nb), dom, bool(td), **kw)
                assert np.array_equal(np.random.uniform(0, 1, 3), d[name + '__tail'])
            assert np.array_equal(Xd, d[name + '__Xd']) and np.array_equal(Xb, d[name + '__Xb']), (name, kw)


@pytest.mark.parametrize('time_dependent, periodic', [(False, (True, False)), (False, (False, True)), (True, (False, True))])
def test_periodic_plans_have_no_point_on_a_dropped_face(time_dependent, periodic):
    dom = np.array([[0.0, 1.0], [-1.0, 1.0]])
    axis = periodic.index(True)
    other = 1 - axis
    np.random.seed(5)
    Xd, Xb = SP.sampled_pts_rdm(50, 42, dom, time_dependent, periodic=periodic)
    nfaces = 1 if time_dependent else 2
    assert Xd.shape == (50, 2) and Xb.shape == (42 // nfaces * nfaces, 2)
    assert not np.any((Xb[:, axis] == dom[axis, 0]) | (Xb[:, axis] == dom[axis, 1]))
    faces = [dom[other, 0]] if time_dependent else list(dom[other])
    assert np.all(np.isin(Xb[:, other], faces)) and all(np.sum(Xb[:, other] == v) == 42 // nfaces for v in faces)
    Xd, Xb = SP.sampled_pts_grid(100, 44, dom, time_dependent, periodic=periodic)
    n = 10                                                               # int(sqrt(144)) - 2
    nodes = dom[axis, 0] + np.arange(n + 2) * (dom[axis, 1] - dom[axis, 0]) / (n + 2)
    for X in (Xd, Xb):                                                   # (the nodes to rounding: j L / (n + 2) may be formed in either order)
        np.testing.assert_allclose(np.unique(X[:, axis]), nodes, rtol=0, atol=4 * EPS)
    assert dom[axis, 1] not in Xd[:, axis] and dom[axis, 1] not in Xb[:, axis]
    assert np.all(np.isin(Xb[:, other], faces)) and Xb.shape[0] == nfaces * (n + 2)
    assert Xd.shape[0] == (n + 2) * (n + 1 if time_dependent else n)
    assert not np.any(np.isin(Xd[:, other], faces))
    assert len({tuple(x) for x in np.concatenate([Xd, Xb])}) == Xd.shape[0] + Xb.shape[0]


def test_samplers_refuse_two_periodic_axes():
    dom = np.array([[0.0, 1.0], [0.0, 1.0]])
    for sampler in (SP.sampled_pts_rdm, SP.sampled_pts_grid):
        with pytest.raises(ValueError):
            sampler(50, 40, dom, periodic=(True, True))
        with pytest.raises(ValueError):
            sampler(50, 40, dom, True, periodic=(True, False))          # periodic in time


# ------------------------------------------------------------------------------------------------ d. gates, subset, host API
def test_block_gate_rejects_a_planted_error():
    param, layout = PR.PARAMS[2], 'Eikonal'
    Xd, Xb, _ = PR.points(16, 4, param)
    T = PR.theta(param, layout, Xd, Xb)
    blocks = PR.offsets(layout, 16, 4)
    Tn = np.concatenate([PR.np_rows(param, layout, f, P, Xd, Xb) for f, P in PR.MR._points(layout, Xd, Xb)], axis=0)
    clean = T.astype(np.float64)
    PR.block_gate('clean', clean, T, Tn, blocks, blocks)
    for bi, (ro, rn) in enumerate(blocks):
        for bj, (co, cn) in enumerate(blocks):
            bad = clean.copy()
            scale = float(np.max(np.abs(T[ro:ro + rn, co:co + cn])))
            bad[ro + rn // 2, co + cn // 3] += 1e-11 * scale
            with pytest.raises(AssertionError):
                PR.block_gate('planted', bad, T, Tn, blocks, blocks)
    bad = clean.copy()
    bad[3, 5] = np.nan
    with pytest.raises(AssertionError):
        PR.block_gate('nan', bad, T, Tn, blocks, blocks)


def test_extension_gate_rejects_a_planted_error():
    param, layout = PR.PARAMS[0], 'Burgers'
    Xd, Xb, Xt = PR.points(16, 4, param, nt=7)
    rows = PR.rows(param, layout, PR.LAP, Xt, Xd, Xb)
    coeff = np.random.RandomState(6).normal(size=rows.shape[1])
    np_value = PR.np_rows(param, layout, PR.LAP, Xt, Xd, Xb) @ coeff
    PR.ExtensionGate(np_value, np_value, rows, coeff).check('clean')
    bad = np_value.copy()
    bad[4] += 1e-11 * float((np.abs(rows) @ np.abs(coeff))[4])
    with pytest.raises(AssertionError):
        PR.ExtensionGate(bad, np_value, rows, coeff).check('planted')


def test_row_subset_covers_every_column():
    for layout in PR.LAYOUTS:
        for Nd, Nb in PR.SIZES[1:]:
            subset = PR.row_subset(layout, Nd, Nb)
            assert PR.subset_coverage(layout, Nd, Nb, subset) == PR.MR.SUBSET_ROWS
            param = PR.PARAMS[0]
    Xd, Xb, _ = PR.points(190, 37, PR.PARAMS[0])
    subset = PR.row_subset('Nonlinear_elliptic', 190, 37)
    ref = PR.subset_rows_reference(PR.PARAMS[0], 'Nonlinear_elliptic', Xd, Xb, subset)
    assert ref.shape == (2 * PR.MR.SUBSET_ROWS, 190 + 227)
    full = PR.theta(PR.PARAMS[0], 'Nonlinear_elliptic', Xd, Xb)
    assert np.array_equal(ref, full[np.concatenate(subset)])


def test_planted_pairs_and_underflow_of_the_cases():
    param = PR.PARAMS[2]
    Xd, Xb, Xt = PR.points(190, 37, param)
    L = np.array(param[2:])
    d = Xd[[1, 3, 5, 7, 9, 11, 13, 15]] - Xd[[0, 2, 4, 6, 8, 10, 12, 12]]
    want = [0 * L, 1e-9 + 0 * L, 1e-6 + 0 * L, 1e-3 + 0 * L, L / 2, L - 1e-3, L, 3 * L]
    for got, w in zip(d, want):
        np.testing.assert_allclose(got, w, rtol=0, atol=2e-16 * 4)
    assert np.array_equal(Xd[13], Xd[12] + L) and np.array_equal(Xd[15], Xd[12] + 3 * L)      # exact images
    for axis in (0, 1):
        fparam, Fd, _, _ = PR.far_case(axis)
        k = PR.prior(fparam, Fd[:1], Fd[1:3])[0]
        tiny = float(np.finfo(np.float64).tiny)
        assert 0 < float(k[0]) < tiny and float(k[0]) >= 5e-324          # subnormal in float64
        assert float(k[1]) == 0.0                                        # below the smallest subnormal


def test_device_module_knows_the_kernel():
    import ctypes as C
    import gpk
    from gpk import device as D
    assert gpk.KERNEL['periodic_Gaussian'] == 16
    kp = D.kernel_params('periodic_Gaussian', (0.2, 0.15, 1.0, 0.0))
    assert isinstance(kp, C.Array) and list(kp) == [0.2, 0.15, 1.0, 0.0]
    with pytest.raises(ValueError):
        D.kernel_params('periodic_Gaussian', (0.2, 0.15))
    for what in ('three space dimensions', 'gpk_assemble_bc'):
        with pytest.raises(ValueError, match='periodic_Gaussian'):
            D.require_gaussian_family('periodic_Gaussian', what)
    with pytest.raises(ValueError):
        D.kernel_params3d('periodic_Gaussian', (0.2, 0.2, 0.2))


def test_solver_checks_the_period_against_the_domain():
    import types
    from src.solver import solver_GP
    def cfg(**kw):
        return types.SimpleNamespace(alpha=1.0, m=3.0, kernel='periodic_Gaussian', kernel_parameter=[0.2, 0.2], **kw)
    s = solver_GP(cfg(period=(1.0, 0.0)), 'Nonlinear_elliptic')
    s.set_equation(bdy=lambda a, b: 0 * a, rhs=lambda a, b: 0 * a, domain=np.array([[0, 1], [0, 1]]), print_option=False)
    assert s.config.kernel_parameter == [0.2, 0.2, 1.0, 0.0] and s.eqn._periodic_axes == (True, False)
    np.random.seed(7)
    s.eqn.sampled_pts(30, 10)
    assert s.eqn.X_boundary.shape == (10, 2) and set(s.eqn.X_boundary[:, 1]) == {0.0, 1.0}
    with pytest.raises(ValueError):
        solver_GP(cfg(period=(2.0, 0.0)), 'Nonlinear_elliptic').set_equation(bdy=None, rhs=None, domain=np.array([[0, 1], [0, 1]]), print_option=False)
    c = cfg(period=(1.0, 0.0))
    c.kernel = 'Gaussian'
    with pytest.raises(ValueError):
        solver_GP(c, 'Nonlinear_elliptic').set_equation(bdy=None, rhs=None, domain=np.array([[0, 1], [0, 1]]), print_option=False)
    s = solver_GP(cfg(), 'Nonlinear_elliptic')                           # no cfg.period: nothing changes
    s.set_equation(bdy=None, rhs=None, domain=np.array([[0, 1], [0, 1]]), print_option=False)
    assert s.config.kernel_parameter == [0.2, 0.2] and s.eqn._periodic_axes == (False, False)
