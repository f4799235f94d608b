"""Matern kernels on the host (no GPU): the long-double reference of tests/_matern_reference.py against mpmath.diff, the closed-form
classes of src/kernels.py against that reference, the trace ratios, the rejections of what is out of scope, and the preconditions of
tests/test_gpu_matern_shapes.py: its planted points, its row subset, and its two gates on a planted error."""
import numpy as np
import pytest

import _matern_reference as MR

NUS = (2.5, 3.5, 4.5)
NAMES = {2.5: 'Matern52', 3.5: 'Matern72', 4.5: 'Matern92'}
RHOS = (0.3, (0.3, 0.07))

# (alpha, beta) of every derivative the layouts and the extension functionals combine: per-axis order <= 2 on each side
ORDERS = sorted({(a, b) for fx in MR.FUNCTIONALS.values() for fy in MR.FUNCTIONALS.values() for a in fx for b in fy})

# a dozen fixed pairs (x1, x2, y1, y2): far, on both sides of the switch to the series (t = 0.5), 1e-12 apart, on an axis
PAIRS = [(0.31, 0.72, 0.55, 0.12), (0.9, 0.1, 0.2, 0.8), (0.5, 0.5, 0.52, 0.49), (0.5, 0.5, 0.51, 0.503), (0.25, 0.75, 0.2501, 0.7502),
         (0.4, 0.6, 0.4 + 1e-12, 0.6), (0.4, 0.6, 0.4 + 6e-13, 0.6 - 8e-13), (0.3, 0.3, 0.3, 0.45), (0.3, 0.3, 0.45, 0.3),
         (0.125, 0.875, 0.126, 0.871), (0.7, 0.2, 0.69, 0.21), (0.05, 0.95, 0.95, 0.05)]


def rho_scale(rho, fx, fy):
    """largest rho_1^-n1 rho_2^-n2 over the multi-indices of <fx, fy>: the size of such an entry relative to kappa"""
    r = np.atleast_1d(np.asarray(rho, dtype=np.float64))
    return max(r[0] ** -(a[0] + b[0]) * r[-1] ** -(a[1] + b[1]) for a in fx for b in fy)


@pytest.mark.parametrize('nu', NUS)
def test_reference_against_mpmath(nu):
    """every (alpha, beta) the functionals combine, on fixed pairs, anisotropic scales: relative to (a / rho)^n, the size of a
    derivative of order n, 1e-17 is asked of the reference (long double: eps 1.1e-19)"""
    import mpmath as mp
    m = MR.ORDER[nu]
    rho = (0.3, 0.07)
    worst = 0.0
    with mp.workdps(40):
        a = mp.sqrt(2 * m + 1)
        th = MR._THETA[m]

        def kappa(x1, x2, y1, y2):
            t = a * mp.sqrt(((x1 - y1) / mp.mpf(rho[0])) ** 2 + ((x2 - y2) / mp.mpf(rho[1])) ** 2)
            return mp.exp(-t) * sum(c * t ** j for j, c in enumerate(th)) / th[0]
        for ip, pr in enumerate(PAIRS):
            exact = [mp.mpf(float(v)) for v in pr]                    # the float64 values the reference receives
            for al, be in ORDERS[ip % 3::3]:                          # (every (alpha, beta) on four of the twelve pairs)
                want = mp.diff(kappa, tuple(exact), (al[0], al[1], be[0], be[1]))
                got = MR.partial(nu, al, be, *[np.float64(v) for v in pr], rho)
                scale = (float(a) / rho[0]) ** (al[0] + be[0]) * (float(a) / rho[1]) ** (al[1] + be[1])
                err = abs(mp.mpf(float(got)) + mp.mpf(float(got - MR.LD(float(got)))) - want) / scale
                worst = max(worst, float(err))
    print(f'[matern] reference vs mpmath nu={nu}: worst |diff| / (a/rho)^n = {worst:.2e}')
    assert worst < 1e-17


def test_reference_coincident_limits():
    """values worked out by hand: nu = 5/2, rho = 1: d_d1^4 kappa -> 3 phi''(0) = 25, d_d1^2 d_d2^2 kappa -> 25/3, Delta_x Delta_y kappa = 8 a^4 / 3"""
    z = np.zeros(1)
    assert abs(MR.partial(2.5, (2, 0), (2, 0), z, z, z, z, 1.0)[0] - 25) < 1e-17
    assert abs(MR.partial(2.5, (2, 0), (0, 2), z, z, z, z, 1.0)[0] - MR.LD(25) / 3) < 1e-17
    assert abs(MR.pair(2.5, MR.LAP, MR.LAP, z, z, z, z, 1.0)[0] - MR.LD(200) / 3) < 1e-16


def _random_pairs():
    rng = np.random.RandomState(7)
    x = rng.uniform(0, 1, (4, 60))
    x[2:, 0] = x[:2, 0]                                               # one coincident pair
    x[2, 1], x[3, 1] = x[0, 1] + 6e-13, x[1, 1] - 8e-13               # one pair 1e-12 apart
    x[2:, 2:8] = x[:2, 2:8] + rng.uniform(-0.02, 0.02, (2, 6))        # a few close ones, around the series switch
    return x


@pytest.mark.parametrize('nu', NUS)
@pytest.mark.parametrize('rho', RHOS)
def test_kernel_classes_against_reference(nu, rho):
    from src.kernels import _METHODS, Matern52_kernel, Matern72_kernel, Matern92_kernel, Matern_kernel
    x = _random_pairs()
    thin = {2.5: Matern52_kernel, 3.5: Matern72_kernel, 4.5: Matern92_kernel}[nu]()
    k = Matern_kernel(nu)
    assert thin.m == k.m
    for name, (fx, fy) in _METHODS.items():
        fxt, fyt = tuple(map(tuple, fx)), tuple(map(tuple, fy))
        want = MR.pair(nu, fxt, fyt, *x, rho)
        got = getattr(k, name)(*x, rho)
        assert np.array_equal(got, getattr(thin, name)(*x, rho))
        s = rho_scale(rho, fxt, fyt)
        err = np.abs(got - want)
        assert np.all(np.isfinite(got)), name
        assert np.all(err <= 1e-13 * np.abs(want) + 1e-12 * s), (name, float(np.max(err / (1e-13 * np.abs(want) + 1e-12 * s))))
    assert np.ndim(k.kappa(0.1, 0.2, 0.3, 0.4, 0.3)) == 0            # scalar in, scalar out
    assert k.kappa(0.1, 0.2, 0.1, 0.2, rho) == 1.0


@pytest.mark.parametrize('nu', NUS)
def test_singular_terms_vanish_exactly_at_coincident_points(nu):
    """at d = 0 the class gives the limit, with no NaN on the way: Delta_x Delta_y kappa(x, x) = 8 a^4 / 3 * phi''(0) scaling for rho = 1"""
    from src.kernels import Matern_kernel
    m = MR.ORDER[nu]
    a2 = 2.0 * m + 1.0
    phi2 = a2 ** 2 * {2: 1.0 / 3.0, 3: 1.0 / 15.0, 4: 3.0 / 105.0}[m]                    # phi''(0) = a^4 theta_{m-2}(0) / theta_m(0)
    with np.errstate(all='raise'):
        v = Matern_kernel(nu).Delta_x_Delta_y_kappa(0.3, 0.4, 0.3, 0.4, 1.0)
    assert abs(v - 8.0 * phi2) <= 4e-16 * 8.0 * phi2


@pytest.mark.parametrize('layout', sorted(MR.LAYOUTS))
@pytest.mark.parametrize('nu', NUS)
def test_trace_ratios_against_reference(layout, nu):
    """the analytic diagonal values <d^alpha, d^alpha>(0) = (-1)^|alpha| rho^-2alpha c(2 alpha_1, alpha_1) c(2 alpha_2, alpha_2) phi^(|alpha|)(0)
    through the classes, against the Taylor series of the reference"""
    from src.kernels import Matern_kernel
    k = Matern_kernel(nu)
    for rho in RHOS:
        want = MR.diagonal_values(nu, rho, layout)
        got = [k._eval(f, f, 0.5, 0.5, 0.5, 0.5, rho) for f, _ in MR.LAYOUTS[layout]]
        np.testing.assert_allclose(got, np.asarray(want, dtype=np.float64), rtol=1e-14)
        r = MR.trace_ratios(nu, rho, layout, 64, 36)
        n = [s for _, s in MR.offsets(layout, 64, 36)]
        np.testing.assert_allclose([n[b] * got[b] / (n[-1] * got[-1]) for b in range(len(r))], np.asarray(r, dtype=np.float64), rtol=1e-14)


@pytest.mark.parametrize('nu', [1.5, 0.5, 3.0, 'x', None])
def test_unknown_nu_is_rejected(nu):
    from src.kernels import Matern_kernel
    with pytest.raises(ValueError, match='nu'):
        Matern_kernel(nu)


def test_kernel_parameters():
    from gpk.device import KERNEL, kernel_params
    assert (KERNEL['Matern52'], KERNEL['Matern72'], KERNEL['Matern92']) == (8, 9, 10)
    assert list(kernel_params('Matern52', 0.3)) == [0.3, 0.3]
    assert list(kernel_params('Matern72', [0.3])) == [0.3, 0.3]
    assert list(kernel_params('Matern92', (0.3, 0.05))) == [0.3, 0.05]
    with pytest.raises(ValueError, match='Matern52'):
        kernel_params('Matern52', (0.1, 0.2, 0.3))
    from src.Gram_matrice import _KERNELS
    assert {'Matern52', 'Matern72', 'Matern92'} <= set(_KERNELS)


@pytest.mark.parametrize('kernel', ['Matern52', 'Matern72', 'Matern92'])
def test_out_of_scope_paths_name_the_kernel(kernel, monkeypatch):
    """3-D, boundary-functional and operator paths: ValueError naming the kernel, before any device call (no context can even be created here)"""
    from gpk.device import kernel_params3d
    from src import PDEs
    import src._runtime as RT

    def no_device(*a, **k):
        raise AssertionError('a device call was reached')
    monkeypatch.setattr(RT, 'get_context', no_device)
    monkeypatch.setattr(PDEs, 'get_context', no_device)
    with pytest.raises(ValueError, match=kernel):
        kernel_params3d(kernel, 0.3)
    np.random.seed(0)
    eq = PDEs.Nonlinear_elliptic2d(bdy=lambda x1, x2: 0 * x1, rhs=lambda x1, x2: 0 * x1 + 1.0)
    eq.sampled_pts(20, 8, sampled_type='random')
    eq.set_boundary_operator(np.tile([0.0, 1.0, 0.0], (eq.N_boundary, 1)))
    with pytest.raises(ValueError, match=kernel):
        eq.Gram_matrix(kernel=kernel, kernel_parameter=0.3)
    eq = PDEs.Nonlinear_elliptic2d(bdy=lambda x1, x2: 0 * x1, rhs=lambda x1, x2: 0 * x1 + 1.0)
    eq.sampled_pts(20, 8, sampled_type='random')
    eq.set_domain_operator(np.tile([0.0, 0.0, 0.0, 1.0, 0.0, 1.0], (eq.N_domain, 1)))
    with pytest.raises(ValueError, match=kernel):
        eq.Gram_matrix(kernel=kernel, kernel_parameter=0.3)
    eq3 = PDEs.Nonlinear_elliptic3d(bdy=lambda x1, x2, x3: 0 * x1, rhs=lambda x1, x2, x3: 0 * x1 + 1.0)
    eq3.sampled_pts(20, 12, sampled_type='random')
    with pytest.raises(ValueError, match=kernel):
        eq3.Gram_matrix(kernel=kernel, kernel_parameter=0.3)


# ------------------------------------------------------------------- preconditions of tests/test_gpu_matern_shapes.py (no GPU)
SHAPE_SIZES = ((64, 36), (65, 41))
KERNELS = MR.KERNELS


def _device_test():
    """tests/test_gpu_matern.py, whose points, numpy rows and block gate the shape tests reuse (imported on use: it is a GPU file)"""
    import test_gpu_matern as TM
    return TM


def _block_errors(got, ref, blocks):
    """max |got - ref| / max|block| over the blocks"""
    return max(float(np.max(np.abs(got[ro:ro + rn, co:co + cn].astype(MR.LD) - ref[ro:ro + rn, co:co + cn])) /
                     np.max(np.abs(ref[ro:ro + rn, co:co + cn]))) for ro, rn in blocks for co, cn in blocks)


@pytest.mark.parametrize('size', SHAPE_SIZES)
def test_planted_points_hold_the_separations_they_claim(size):
    TM = _device_test()
    Xd0, Xb0, Xt0 = TM._points(*size)
    Xd, Xb, Xt = MR.planted_points(Xd0, Xb0, Xt0)
    assert all(np.array_equal(a, b) for a, b in zip(TM._points(*size), (Xd0, Xb0, Xt0)))      # (the inputs are left as they were)
    sep = lambda p, q: float(np.hypot(*(np.asarray(p, dtype=MR.LD) - np.asarray(q, dtype=MR.LD))))
    for k, s, d in MR.PLANT_D:
        assert abs(sep(Xd[k], Xd[s]) - np.hypot(*d)) <= 1e-3 * np.hypot(*d), (k, s)       # (an offset of 1e-12 next to 0.5: 1.1e-16 off)
    for k, s, d in MR.PLANT_B:
        assert abs(sep(Xb[k], Xd[s]) - np.hypot(*d)) <= 1e-3 * np.hypot(*d), (k, s)
    for k, which, s, d in MR.PLANT_T:
        assert abs(sep(Xt[k], (Xd if which == 'd' else Xb)[s]) - np.hypot(*d)) <= 1e-3 * np.hypot(*d), (k, s)
    assert np.array_equal(Xd[9], Xd[8]) and np.array_equal(Xb[0], Xd[10])
    assert np.array_equal(Xt[0], Xd[3]) and np.array_equal(Xt[5], Xb[2]) and np.array_equal(Xt[66], Xd[-1])   # the three verbatim ones
    # nothing else moved, and the planted pairs are the only close ones: every other pair keeps the spacing of uniform points
    moved_d, moved_b = {k for k, _, _ in MR.PLANT_D}, {k for k, _, _ in MR.PLANT_B}
    assert all(np.array_equal(Xd[k], Xd0[k]) for k in range(size[0]) if k not in moved_d)
    assert all(np.array_equal(Xb[k], Xb0[k]) for k in range(size[1]) if k not in moved_b)
    seps = sorted({round(float(np.hypot(*d)), 15) for _, _, d in MR.PLANT_D})
    assert seps[0] == 0.0 and 0 < seps[1] <= 1e-12 and 1e-9 < seps[2] < 1e-7 and seps[3] == 1e-5 and 1e-3 < seps[4] < 2e-3


@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('size', SHAPE_SIZES)
def test_far_points_hold_pairs_in_the_band_and_beyond(kernel, size):
    TM = _device_test()
    rho = (0.3, MR.FAR_RHO2)
    Xd, Xb, Xt = MR.far_points(kernel, *TM._points(*size))
    # (exp(-708) is the last normal value, 3.3e-308: the planted pairs sit at 720 and 735, inside the subnormal range)
    assert 0.0 < float(np.exp(-735.0)) < float(np.exp(-720.0)) < np.finfo(np.float64).tiny and float(np.exp(-746.0)) == 0.0
    t = MR.scaled_distance(kernel, rho, Xd, Xd)
    for i, j in ((0, 1), (0, 2)):
        assert MR.FAR_BAND[0] <= t[i, j] <= MR.FAR_BAND[1] and t[i, j] == t[j, i], (i, j, float(t[i, j]))
    assert t[0, 4] > MR.FAR_BAND[1] and t[4, 0] > MR.FAR_BAND[1]
    tt = MR.scaled_distance(kernel, rho, Xt[:67], Xd)
    assert MR.FAR_BAND[0] <= tt[1, 0] <= MR.FAR_BAND[1] and tt[2, 0] > MR.FAR_BAND[1]
    band, beyond = int(np.sum((t >= MR.FAR_BAND[0]) & (t <= MR.FAR_BAND[1]))), int(np.sum(t > MR.FAR_BAND[1]))
    print(f'[matern-shapes] far points {kernel} {size}: {band} domain pairs in the band, {beyond} beyond')
    assert band >= 4 and beyond >= 2
    # the reference and the numpy class are finite there
    T = MR.theta(kernel, rho, 'Burgers', Xd, Xb)
    Tn = np.concatenate([TM._np_rows(kernel, rho, 'Burgers', f, P, Xd, Xb) for f, P in MR._points('Burgers', Xd, Xb)], axis=0)
    assert np.all(np.isfinite(T)) and np.all(np.isfinite(Tn))


@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('layout', ['Nonlinear_elliptic', 'Burgers', 'Eikonal', 'Darcy_a'])
def test_numpy_class_on_the_planted_points_keeps_the_gate_meaningful(layout, kernel):
    """The gate of the shape tests is (4e-15 + 4 e_np) max|block|, e_np measured on the same points.  It means something only while the
    numpy class itself is accurate there: asked here is e_np <= 1e-15 (4.5 eps).  That keeps the class itself more than a factor 2 inside the gate,
    the measured part 4 e_np no larger than the fixed part 4e-15, and so the whole gate below 8e-15, twice the project's Gram-block
    bound.  A larger e_np on the planted points would make the device gate hollow, and this test says so."""
    TM = _device_test()
    for size in SHAPE_SIZES:
        Xd, Xb, Xt = MR.planted_points(*TM._points(*size))
        blocks = MR.offsets(layout, *size)
        for rho in RHOS:
            T = MR.theta(kernel, rho, layout, Xd, Xb)
            Tn = np.concatenate([TM._np_rows(kernel, rho, layout, f, P, Xd, Xb) for f, P in MR._points(layout, Xd, Xb)], axis=0)
            Tt = MR.theta_test(kernel, rho, layout, Xt[:67], Xd, Xb)
            Ttn = TM._np_rows(kernel, rho, layout, MR.ID, Xt[:67], Xd, Xb)
            assert np.all(np.isfinite(T)) and np.all(np.isfinite(Tt)) and np.all(np.isfinite(Tn)) and np.all(np.isfinite(Ttn))
            e_np = max(_block_errors(Tn, T, blocks),
                       max(float(np.max(np.abs(Ttn[:, o:o + n] - Tt[:, o:o + n])) / np.max(np.abs(Tt[:, o:o + n]))) for o, n in blocks))
            print(f'[matern-shapes] numpy class on the planted points {layout} {kernel} rho {rho} {size}: e_np {e_np:.3g}')
            assert e_np <= 1e-15, 'the gate (4e-15 + 4 e_np) would be hollow on these points'


def test_block_gate_rejects_a_relative_1e_11_in_a_near_coincident_entry():
    TM = _device_test()
    Nd, Nb = SHAPE_SIZES[1]
    kernel, rho, layout = 'Matern52', RHOS[1], 'Burgers'
    Xd, Xb, _ = MR.planted_points(*TM._points(Nd, Nb))
    T = MR.theta(kernel, rho, layout, Xd, Xb)
    Tn = np.concatenate([TM._np_rows(kernel, rho, layout, f, P, Xd, Xb) for f, P in MR._points(layout, Xd, Xb)], axis=0)
    blocks = MR.offsets(layout, Nd, Nb)
    good = T.astype(np.float64)
    TM._gate_blocks('rounded reference', good, T, Tn, blocks, blocks)
    for o, _ in blocks:                                               # the pair Xd[1], Xd[0] (1e-12 apart), in every diagonal block
        assert abs(T[o + 1, o]) >= 0.5 * np.max(np.abs(T[o:o + Nd, o:o + Nd])), 'the planted entry is not of the size of the block diagonal'
        bad = good.copy()
        bad[o + 1, o] *= 1.0 + 1e-11
        with pytest.raises(AssertionError):
            TM._gate_blocks('planted error', bad, T, Tn, blocks, blocks)


def test_extension_gate_rejects_1e_11_in_one_row():
    TM = _device_test()
    Nd, Nb = SHAPE_SIZES[1]
    kernel, rho, layout = 'Matern72', RHOS[1], 'Eikonal'
    Xd, Xb, Xt = MR.planted_points(*TM._points(Nd, Nb))
    Xt = Xt[:9]
    for nm in ('value', 'laplacian'):
        rows = MR.rows(kernel, rho, layout, MR.FUNCTIONALS[nm], Xt, Xd, Xb)
        rows_np = TM._np_rows(kernel, rho, layout, MR.FUNCTIONALS[nm], Xt, Xd, Xb)
        coeff = np.random.RandomState(rows.shape[1]).normal(size=rows.shape[1])
        value = rows_np @ coeff
        g = MR.ExtensionGate(value, value, rows, coeff)
        print(f'[matern-shapes] extension gate {nm}: numpy class r_np {g.r_np:.3g}, allowed {g.allowed:.3g}')
        g.check()
        assert g.allowed * MR.EPS <= 1e-12
        t = int(np.argmax(np.abs(value) / g.terms.astype(np.float64)))
        assert abs(value[t]) * 1e-11 > g.allowed * MR.EPS * float(g.terms[t]), 'the planted error is inside the gate: choose another point'
        bad = value.copy()
        bad[t] *= 1.0 + 1e-11
        with pytest.raises(AssertionError):
            MR.ExtensionGate(bad, value, rows, coeff).check()
        with pytest.raises(AssertionError, match='looser'):              # a numpy ratio that would lift the gate above the norm bound
            worse = value + 1e-11 * g.terms.astype(np.float64)
            MR.ExtensionGate(value, worse, rows, coeff).check()


@pytest.mark.parametrize('layout', sorted(MR.LAYOUTS))
def test_row_subset_of_the_large_cases_covers_every_column(layout):
    seen = set()
    for size, (Nd, Nb) in enumerate(MR.LARGE):
        sub = MR.row_subset(layout, Nd, Nb)
        blocks = MR.offsets(layout, Nd, Nb)
        assert len(sub) == len(blocks)
        for (o, n), idx in zip(blocks, sub):
            loc = idx - o
            assert idx.size == MR.SUBSET_ROWS == np.unique(idx).size and loc.min() == 0 and loc.max() == n - 1
            assert {0, 1, n - 2, n - 1} <= set(loc.tolist())
            edges = [int(p) for p in loc if p % MR.TILE == 0 and p - 1 in loc and p > 1]
            assert edges and min(abs(p - n / 2) for p in edges) <= MR.TILE / 2, 'no tile boundary next to the middle of the block'
        assert MR.subset_coverage(layout, Nd, Nb, sub) >= 30
        assert [a.tolist() for a in MR.row_subset(layout, Nd, Nb)] == [a.tolist() for a in sub]      # deterministic
        seen.add(MR.large_case(layout, size))
    assert len(seen) == 2


def test_large_cases_meet_every_nu_at_both_kernel_shapes():
    table = {(layout, size): MR.large_case(layout, size) for layout in MR.LAYOUTS for size in range(len(MR.LARGE))}
    for size in range(len(MR.LARGE)):
        assert {table[l, size][0] for l in MR.LAYOUTS} == set(KERNELS)
    assert {v for v in table.values()} == {(k, r) for k in KERNELS for r in MR.RHOS}
