"""The Matern evaluators (csrc/gpk_assemble_matern.hip) at the shapes and edges their launch code distinguishes, against the long-double
reference of tests/_matern_reference.py.  tests/test_gpu_matern.py, written with the feature, stays at M <= 190 points (one workgroup
along x in every kernel) and at uniform random points (closest pair about 1e-2 apart); this file is its counterpart of
tests/test_gpu_gram_longdouble.py.

Gate of a, b, c, per block: |device - ref| <= (4e-15 + 4 e_np) max|block|, _gate_blocks of tests/test_gpu_matern.py unchanged; e_np is
the error of src.kernels.Matern_kernel on the same points (_np_rows of that file).

  a  more than one workgroup along x.  (Nd, Nb) = (530, 46): M = 576 even (Darcy_a: 530), the two-point kernel with grid2.x = 2;
     (265, 41): M = 306 with odd block sizes (order 1101), the one-point kernel with grid.x = 2.  (nu, rho) by MR.large_case, index layout + size mod 3 and mod 2:

         layout               (530, 46)                     (265, 41)
         Nonlinear_elliptic   Matern52  0.3                 Matern72  (0.3, 0.07)
         Burgers              Matern72  (0.3, 0.07)         Matern92  0.3
         Eikonal              Matern92  0.3                 Matern52  (0.3, 0.07)
         Darcy_u              Matern52  (0.3, 0.07)         Matern72  0.3
         Darcy_a              Matern72  0.3                 Matern92  (0.3, 0.07)

     every nu meets both kernel shapes, every layout both sizes, and the six (nu, rho) occur at layout + size = 0 .. 5.  Theta: finite,
     exactly symmetric, and compared on 30 rows of every block (MR.row_subset: first and last two, both sides of the 32-row tile
     boundary nearest the middle, 24 random) in all columns; asserted: every column is compared in >= 30 rows of every row block.  The
     symmetry carries the result to the transposed entries, so every column workgroup and both `live` edges are compared.  Test rows
     and cross columns (transposed) at Nt in {2, 514, 515}: two workgroups along t in the cross kernel, its 16-byte and its 8-byte form.
  b  coincident and nearly coincident points (MR.planted_points: separations 0, 1e-12, 1e-8, 1e-5, 1.4e-3 among the domain points, a
     boundary point on a domain point and one 3e-7 from one, test points 1e-12, 1e-6 and 1.4e-9 from collocation points), (64, 36) and
     (65, 41), every layout x nu x rho, Nt = 67: the gate, every entry finite, Theta exactly symmetric, and the rows and columns of
     coincident points agree bit for bit in every block.
  c  far pairs: rho = (0.3, 0.002), second coordinates planted so that t = a |u| is 720 and 735 (exp(-t) subnormal) and > 745 (exp(-t)
     = 0) (MR.far_points, per nu); precondition from the points: >= 4 domain pairs in [708, 745], >= 2 beyond.  Finite, and the gate.
  d  store policies at (64, 36), adaptive nugget: gpk_tune(55, 1 / 2 / 3) and (47, 0) give the bits of the default, before and after
     restoring; assemble_cross at Nt = 300 under key 47 = 0 gives the bits of its wide form.
  e  views between canaries (tests/_view_arena.py), classes D (odd offset, odd ld) and A (ld > N, aligned), the three entry points,
     (64, 36), Nt = 67 (D) / 66 (A), one nu per layout: nothing outside is written, the bits are those of the plain call.
  f  gpk_extend and gpk_extend_functionals (all five functionals) per test point, at (65, 41) and (265, 41) (M = 306 > 256: the stride
     loop runs twice), Nt = 67 (a ragged last group of FN_TT = 4), the planted points of b, every layout x nu x rho.  Gate per test
     point and functional: |device - ref| <= C eps (|rows| @ |coeff|)_t, C = 32 r_np + 1 (the rule `allowed` of tests/_gn_reference.py),
     r_np the worst such ratio of the float64 numpy class's rows @ coeff measured in the same test; asserted: C eps (|rows| @ |coeff|)_t
     <= 1e-12 max_t (|rows| @ |coeff|) at every t, the bound of tests/test_gpu_matern.py.  All 31 masks at (65, 41), Nt = 5: every row
     of every mask has the bits of its single-bit call, and a repeat gives the same bits.

Every figure is printed under a [matern-shapes] tag before it is asserted.

RESULTS
  A run on an MI355X (gfx950), every test of this file passing: 140 tests, 965 [matern-shapes] lines, 86 s wall time, of which the long-
  double references on the host are most (the slowest test 4.9 s; tests/test_gpu_matern.py at the parent commit, the same run: 83 tests
  in 40 s).  No defect was found.  Worst per nu -- a, b, c: device / e_np / allowed in units of max|block|, the block that comes closest
  to its allowance; f: device / r_np / allowed in units of eps (|rows| @ |coeff|)_t, over layouts, rho and both sizes:
    a Matern52: assemble 6.04e-16 / 6.04e-16 / 6.42e-15, test rows 5.4e-16 / 5.31e-16 / 6.12e-15, cross columns 5.4e-16 / 5.31e-16 / 6.12e-15
    a Matern72: assemble 8.09e-16 / 8.09e-16 / 7.24e-15, test rows 6.92e-16 / 5.72e-16 / 6.29e-15, cross columns 6.92e-16 / 5.72e-16 / 6.29e-15
    a Matern92: assemble 7.75e-16 / 6.33e-16 / 6.53e-15, test rows 7.31e-16 / 6.29e-16 / 6.52e-15, cross columns 7.31e-16 / 6.29e-16 / 6.52e-15
    b Matern52: assemble 5.97e-16 / 4.62e-16 / 5.85e-15, test rows 7.73e-16 / 7.73e-16 / 7.09e-15, cross columns 7.73e-16 / 7.73e-16 / 7.09e-15
    b Matern72: assemble 6.72e-16 / 5.5e-16 / 6.2e-15, test rows 5.83e-16 / 4.09e-16 / 5.64e-15, cross columns 5.83e-16 / 4.09e-16 / 5.64e-15
    b Matern92: assemble 8.42e-16 / 6.12e-16 / 6.45e-15, test rows 5.8e-16 / 4.89e-16 / 5.96e-15, cross columns 5.8e-16 / 4.89e-16 / 5.96e-15
    c Matern52: assemble 6.01e-16 / 6.01e-16 / 6.4e-15, test rows 3.65e-16 / 4.73e-16 / 5.89e-15, cross columns 3.65e-16 / 4.73e-16 / 5.89e-15
    c Matern72: assemble 5.48e-16 / 4.89e-16 / 5.96e-15, test rows 3.98e-16 / 3.98e-16 / 5.59e-15, cross columns 3.98e-16 / 3.98e-16 / 5.59e-15
    c Matern92: assemble 5.6e-16 / 5.6e-16 / 6.24e-15, test rows 4.94e-16 / 4.94e-16 / 5.98e-15, cross columns 4.94e-16 / 4.94e-16 / 5.98e-15
    f Matern52: extend 1.13 / 1.28 / 41.9, value 1.37 / 1.28 / 41.9, d1 0.798 / 0.785 / 26.1, d2 1.05 / 0.781 / 26, d2d2 2.29 / 2.66 / 86, laplacian 2.56 / 2.25 / 73.1
    f Matern72: extend 1.01 / 0.898 / 29.7, value 1.01 / 0.898 / 29.7, d1 1.31 / 1.31 / 43.1, d2 1.55 / 1.56 / 50.8, d2d2 2.36 / 2.45 / 79.5, laplacian 1.81 / 1.88 / 61.2
    f Matern92: extend 1.37 / 1.09 / 35.8, value 1.37 / 1.09 / 35.8, d1 1.57 / 1.43 / 46.7, d2 2.19 / 1.25 / 41.1, d2d2 0.922 / 0.899 / 29.8, laplacian 1.62 / 1.07 / 35.4
  The largest device figure of a, b, c: 8.42e-16.  f: the largest device ratio 3.26 eps, the largest r_np 3.43, the largest C 111 (the norm
  bound 1e-12 max_t corresponds to 4503 eps at the test point with the largest sum).  d, e, the symmetry, the coincident rows and the 31
  masks: the same bits throughout.
"""
import functools

import numpy as np
import pytest

import _matern_reference as MR
import _view_arena as VA
import test_gpu_matern as TM

pytestmark = pytest.mark.gpu

LD = MR.LD
LAYOUTS = TM.LAYOUTS
KERNELS = MR.KERNELS
RHOS = MR.RHOS
SIZES = TM.SIZES
LARGE = MR.LARGE
SPEC = TM.SPEC
NTS_LARGE = (2, 514, 515)
TAG = '[matern-shapes]'


@pytest.fixture(scope='module')
def ctx():
    import gpk
    c = gpk.Context(0)
    yield c
    c.close()


def _points(Nd, Nb):
    """the points of tests/test_gpu_matern.py with the test points continued to 515"""
    Xd, Xb, Xt = TM._points(Nd, Nb)
    more = np.random.RandomState(7 * Nd + Nb).uniform(0, 1, (max(NTS_LARGE) - Xt.shape[0], 2))
    return Xd, Xb, np.concatenate([Xt, more])


def _np_theta(kernel, rho, layout, Xd, Xb):
    return np.concatenate([TM._np_rows(kernel, rho, layout, f, P, Xd, Xb) for f, P in MR._points(layout, Xd, Xb)], axis=0)


def _allowed(w):
    return 4e-15 + 4 * w[1]


def _figures(got, ref, npv, row_blocks, col_blocks):
    """the worst (device, e_np) that TM._gate_blocks would return, without asserting: the figures are printed first"""
    worst = (0.0, 0.0)
    for ro, rn in row_blocks:
        for co, cn in col_blocks:
            r = ref[ro:ro + rn, co:co + cn]
            scale = float(np.max(np.abs(r)))
            e_dev = float(np.max(np.abs(got[ro:ro + rn, co:co + cn].astype(LD) - r))) / scale
            e_np = float(np.max(np.abs(npv[ro:ro + rn, co:co + cn].astype(LD) - r))) / scale
            if e_dev / (4e-15 + 4 * e_np) >= worst[0] / _allowed(worst):
                worst = (e_dev, e_np)
    return worst


def _gate(kind, case, got, ref, npv, row_blocks, col_blocks):
    assert got.shape == ref.shape == npv.shape, (kind, case, got.shape, ref.shape)
    finite = bool(np.all(np.isfinite(got)))
    w = _figures(got, ref, npv, row_blocks, col_blocks)
    print(f'{TAG} {kind} {case}: finite {finite}, device {w[0]:.3g}, e_np {w[1]:.3g}, allowed {_allowed(w):.3g}')
    assert finite, (kind, case)
    TM._gate_blocks((kind, case), got, ref, npv, row_blocks, col_blocks)
    return w


def _test_and_cross(ctx, case, layout, kernel, rho, Xt, Xd, Xb, Tt, Ttn, blocks):
    Nt = Xt.shape[0]
    dt = ctx.assemble_test(layout, kernel, rho, Xt, Xd, Xb)
    gt = dt.download().reshape(Nt, -1)
    dc = ctx.assemble_cross(layout, kernel, rho, Xt, Xd, Xb)
    gc = dc.download().reshape(-1, Nt)
    dt.free(); dc.free()
    _gate('test rows', f'{case} Nt {Nt}', gt, Tt, Ttn, [(0, Nt)], blocks)
    _gate('cross columns', f'{case} Nt {Nt}', np.ascontiguousarray(gc.T), Tt, Ttn, [(0, Nt)], blocks)


# ------------------------------------------------------------------------------------------------ a. more than one workgroup along x
@functools.lru_cache(maxsize=None)
def _large_reference(layout, kernel, rho, Nd, Nb):
    """long double and numpy class: the rows MR.row_subset of Theta, and Theta_test at all 515 test points"""
    Xd, Xb, Xt = _points(Nd, Nb)
    sub = MR.row_subset(layout, Nd, Nb)
    R = MR.subset_rows_reference(kernel, rho, layout, Xd, Xb, sub)
    Rn = MR.subset_rows_reference(kernel, rho, layout, Xd, Xb, sub, evaluate=lambda f, P: TM._np_rows(kernel, rho, layout, f, P, Xd, Xb))
    return sub, R, Rn, MR.theta_test(kernel, rho, layout, Xt, Xd, Xb), TM._np_rows(kernel, rho, layout, MR.ID, Xt, Xd, Xb)


@pytest.mark.parametrize('size', range(len(LARGE)))
@pytest.mark.parametrize('layout', LAYOUTS)
def test_gram_with_two_workgroups_along_the_columns(ctx, layout, size):
    Nd, Nb = LARGE[size]
    kernel, rho = MR.large_case(layout, size)
    Xd, Xb, _ = _points(Nd, Nb)
    sub, R, Rn, _, _ = _large_reference(SPEC.get(layout, layout), kernel, rho, Nd, Nb)
    blocks = MR.offsets(layout, Nd, Nb)
    N = blocks[-1][0] + blocks[-1][1]
    M = Nd if layout == 'Darcy_a' else Nd + Nb
    pairs = all(n % 2 == 0 for _, n in blocks)                         # (pairs_eligible: the two-point kernel needs every block size even)
    assert pairs == (size == 0) and (M // 2 if pairs else M) > 256, 'precondition: the kernel shape and its second workgroup'
    coverage = MR.subset_coverage(layout, Nd, Nb, sub)
    case = f'{layout} {kernel} rho {rho} ({Nd}, {Nb})'
    dT, _ = ctx.assemble(layout, kernel, rho, Xd, Xb)
    got = dT.download()
    dT.free()
    symmetric = bool(np.array_equal(VA.bits(got), VA.bits(got.T)))
    print(f'\n{TAG} assemble {case}: order {N}, exactly symmetric {symmetric}, every column compared in >= {coverage} rows of every row block')
    assert got.shape == (N, N) and symmetric and coverage >= 30
    idx = np.concatenate(sub)
    _gate('assemble', case, got[idx], R, Rn, [(k * MR.SUBSET_ROWS, MR.SUBSET_ROWS) for k in range(len(sub))], blocks)
    assert np.all(np.isfinite(got))


@pytest.mark.parametrize('Nt', NTS_LARGE)
@pytest.mark.parametrize('size', range(len(LARGE)))
@pytest.mark.parametrize('layout', LAYOUTS)
def test_test_rows_and_cross_columns_with_two_workgroups(ctx, layout, size, Nt):
    Nd, Nb = LARGE[size]
    kernel, rho = MR.large_case(layout, size)
    Xd, Xb, Xt = _points(Nd, Nb)
    _, _, _, Tt, Ttn = _large_reference(SPEC.get(layout, layout), kernel, rho, Nd, Nb)
    print()
    _test_and_cross(ctx, f'{layout} {kernel} rho {rho} ({Nd}, {Nb})', layout, kernel, rho, Xt[:Nt], Xd, Xb, Tt[:Nt], Ttn[:Nt],
                    MR.offsets(layout, Nd, Nb))


# ------------------------------------------------------------------------------------------------ b. coincident and nearly coincident points
NT = 67


@functools.lru_cache(maxsize=None)
def _full_reference(layout, kernel, rho, Nd, Nb, points):
    """(Theta, Theta_test at the first 67 test points) in long double and from the numpy class on the planted / far points"""
    Xd, Xb, Xt = _case_points(points, kernel, Nd, Nb)
    return (MR.theta(kernel, rho, layout, Xd, Xb), MR.theta_test(kernel, rho, layout, Xt, Xd, Xb),
            _np_theta(kernel, rho, layout, Xd, Xb), TM._np_rows(kernel, rho, layout, MR.ID, Xt, Xd, Xb))


def _case_points(points, kernel, Nd, Nb):
    Xd, Xb, Xt = TM._points(Nd, Nb)
    Xd, Xb, Xt = MR.planted_points(Xd, Xb, Xt) if points == 'planted' else MR.far_points(kernel, Xd, Xb, Xt)
    return Xd, Xb, Xt[:NT]


def _parity(ctx, tag, layout, kernel, rho, Nd, Nb, points):
    Xd, Xb, Xt = _case_points(points, kernel, Nd, Nb)
    T, Tt, Tn, Ttn = _full_reference(SPEC.get(layout, layout), kernel, rho, Nd, Nb, points)
    blocks = MR.offsets(layout, Nd, Nb)
    case = f'{tag} {layout} {kernel} rho {rho} ({Nd}, {Nb})'
    dT, _ = ctx.assemble(layout, kernel, rho, Xd, Xb)
    got = dT.download()
    dT.free()
    symmetric = bool(np.array_equal(VA.bits(got), VA.bits(got.T)))
    print(f'\n{TAG} assemble {case}: exactly symmetric {symmetric}')
    _gate('assemble', case, got, T, Tn, blocks, blocks)
    assert symmetric
    _test_and_cross(ctx, case, layout, kernel, rho, Xt, Xd, Xb, Tt, Ttn, blocks)
    return got


@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('layout', LAYOUTS)
def test_coincident_and_nearly_coincident_points(ctx, layout, kernel):
    for rho in RHOS:
        for Nd, Nb in SIZES:
            got = _parity(ctx, '(near)', layout, kernel, rho, Nd, Nb, 'planted')
            blocks = MR.offsets(layout, Nd, Nb)
            twins = [(o + 8, o + 9) for o, _ in blocks]                 # Xd[9] = Xd[8], in every block
            if layout != 'Darcy_a':                                     # Xb[0] = Xd[10], both in the value block
                twins.append((blocks[-1][0] + 10, blocks[-1][0] + Nd))
            same = [bool(np.array_equal(VA.bits(got[i]), VA.bits(got[j])) and np.array_equal(VA.bits(got[:, i]), VA.bits(got[:, j])))
                    for i, j in twins]
            print(f'{TAG} coincident rows and columns {layout} {kernel} rho {rho} ({Nd}, {Nb}): the same bits {same}')
            assert all(same), twins


# ------------------------------------------------------------------------------------------------ c. far pairs
@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('layout', LAYOUTS)
def test_far_pairs_underflow_and_stay_finite(ctx, layout, kernel):
    rho = (0.3, MR.FAR_RHO2)
    for Nd, Nb in SIZES:
        Xd, Xb, Xt = _case_points('far', kernel, Nd, Nb)
        t = MR.scaled_distance(kernel, rho, Xd, Xd)
        band, beyond = int(np.sum((t >= MR.FAR_BAND[0]) & (t <= MR.FAR_BAND[1]))), int(np.sum(t > MR.FAR_BAND[1]))
        print(f'\n{TAG} far pairs {layout} {kernel} ({Nd}, {Nb}): {band} domain pairs with 708 <= t <= 745, {beyond} beyond')
        assert band >= 4 and beyond >= 2, 'precondition: the points hold no pair in the band / beyond it'
        _parity(ctx, '(far)', layout, kernel, rho, Nd, Nb, 'far')


# ------------------------------------------------------------------------------------------------ d. store policies
@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('layout', LAYOUTS)
def test_store_policies_give_the_same_bits(ctx, layout, kernel):
    Nd, Nb = SIZES[0]
    Xd, Xb, Xt = TM._points(Nd, Nb)
    Xt = Xt[:300]                                                      # (even: the 16-byte form of the cross kernel by default)
    for rho in RHOS:
        def run():
            T, _ = ctx.assemble(layout, kernel, rho, Xd, Xb, 1e-6, 'adaptive')
            out = VA.bits(T.download())
            T.free()
            return out

        def run_cross():
            K = ctx.assemble_cross(layout, kernel, rho, Xt, Xd, Xb)
            out = VA.bits(K.download())
            K.free()
            return out
        default, default_c = run(), run_cross()
        same = {}
        try:
            for v in (1, 2, 3):
                ctx.tune(55, v)
                same[f'key 55 = {v}'] = bool(np.array_equal(run(), default))
            ctx.tune(55, 0)
            ctx.tune(47, 0)
            same['key 47 = 0'] = bool(np.array_equal(run(), default))
            same['key 47 = 0, cross'] = bool(np.array_equal(run_cross(), default_c))
        finally:
            ctx.tune(55, 0)
            ctx.tune(47, 1)
        same['restored'] = bool(np.array_equal(run(), default) and np.array_equal(run_cross(), default_c))
        print(f'\n{TAG} store policies {layout} {kernel} rho {rho}: the bits of the default {same}')
        assert all(same.values()), same


# ------------------------------------------------------------------------------------------------ e. views
def _raw(ctx, layout, kernel, rho, Xd, Xb, Xt):
    """the three entry points through the C ABI on a caller's pointer and ld"""
    import gpk
    Nd, Nb = Xd.shape[0], Xb.shape[0]
    dXd, dXb, dXt = ctx.points(Xd), ctx.points(Xb), ctx.points(Xt)
    lay, kid, kpar = gpk.LAYOUT[layout], gpk.KERNEL[kernel], gpk.device.kernel_params(kernel, rho)

    def call(which, ptr, ld):
        if which == 'assemble':
            return ctx.lib.gpk_assemble(ctx.h, lay, kid, kpar, dXd.ptr, Nd, dXb.ptr, Nb, 1e-6, gpk.NUGGET['adaptive'], ptr, ld, None)
        entry = ctx.lib.gpk_assemble_test if which == 'assemble_test' else ctx.lib.gpk_assemble_cross
        return entry(ctx.h, lay, kid, kpar, dXt.ptr, Xt.shape[0], dXd.ptr, Nd, dXb.ptr, Nb, ptr, ld)
    return call


@pytest.mark.parametrize('cls', ['D', 'A'])
@pytest.mark.parametrize('layout', LAYOUTS)
def test_views_between_canaries(ctx, layout, cls):
    """class D: odd base offset and odd ld (8-byte stores everywhere); class A with ld > N: the 16-byte stores of the two-point kernel and
    of the cross kernel next to canaries"""
    Nd, Nb = SIZES[0]
    kernel = KERNELS[LAYOUTS.index(layout) % 3]
    rho = RHOS[1]
    Xd, Xb, Xt = TM._points(Nd, Nb)
    Nt = 67 if cls == 'D' else 66
    Xt = Xt[:Nt]
    blocks = MR.offsets(layout, Nd, Nb)
    N = blocks[-1][0] + blocks[-1][1]
    call = _raw(ctx, layout, kernel, rho, Xd, Xb, Xt)
    plain, _ = ctx.assemble(layout, kernel, rho, Xd, Xb, 1e-6, 'adaptive')
    plain_t = ctx.assemble_test(layout, kernel, rho, Xt, Xd, Xb)
    plain_c = ctx.assemble_cross(layout, kernel, rho, Xt, Xd, Xb)
    want = {'assemble': plain.download().reshape(N, N), 'assemble_test': plain_t.download().reshape(Nt, N),
            'assemble_cross': plain_c.download().reshape(N, Nt)}
    for which, (m, n) in (('assemble', (N, N)), ('assemble_test', (Nt, N)), ('assemble_cross', (N, Nt))):
        v = VA.class_view(ctx, m, n, cls, ld_min=n + 8)
        assert v.cls == cls and v.ld > n
        ctx._chk(call(which, v.ptr, v.ld))
        ctx.synchronize()
        same = bool(np.array_equal(VA.bits(v.arena.get(v)), VA.bits(want[which])))
        print(f'\n{TAG} view class {cls} {which} {layout} {kernel}: ld {v.ld} for {n} columns, the bits of the plain call {same}')
        v.arena.assert_outside_untouched([v])
        assert same, which
        v.arena.free()
    for a in (plain, plain_t, plain_c):
        a.free()


# ------------------------------------------------------------------------------------------------ f. extension
NAMES = tuple(MR.FUNCTIONALS)
EXT_SIZES = (SIZES[1], LARGE[1])


@functools.lru_cache(maxsize=None)
def _extension_reference(layout, kernel, rho, Nd, Nb):
    """per functional the rows at the 67 planted test points, long double and numpy class"""
    Xd, Xb, Xt = _case_points('planted', kernel, Nd, Nb)
    return ({nm: MR.rows(kernel, rho, layout, MR.FUNCTIONALS[nm], Xt, Xd, Xb) for nm in NAMES},
            {nm: TM._np_rows(kernel, rho, layout, MR.FUNCTIONALS[nm], Xt, Xd, Xb) for nm in NAMES})


@pytest.mark.parametrize('rho', RHOS, ids=('isotropic', 'anisotropic'))
@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('layout', LAYOUTS)
def test_extension_per_test_point(ctx, layout, kernel, rho):
    for Nd, Nb in EXT_SIZES:
        Xd, Xb, Xt = _case_points('planted', kernel, Nd, Nb)
        rows, rows_np = _extension_reference(SPEC.get(layout, layout), kernel, rho, Nd, Nb)
        N = rows['value'].shape[1]
        coeff = np.random.RandomState(N).normal(size=N)
        case = f'{layout} {kernel} rho {rho} ({Nd}, {Nb})'
        got = ctx.extend(layout, kernel, rho, Xt, Xd, Xb, coeff).download()
        out = ctx.extend_functionals(layout, kernel, rho, Xt, Xd, Xb, coeff, which=NAMES).download().reshape(len(NAMES), NT)
        assert got.shape == (NT,) and np.all(np.isfinite(got)) and np.all(np.isfinite(out))
        gates = [('extend', MR.ExtensionGate(got, rows_np['value'] @ coeff, rows['value'], coeff))]
        gates += [(f'extend_functionals {nm}', MR.ExtensionGate(out[k], rows_np[nm] @ coeff, rows[nm], coeff)) for k, nm in enumerate(NAMES)]
        print()
        for kind, g in gates:
            print(f'{TAG} {kind} {case}: device {g.device:.3g}, r_np {g.r_np:.3g}, allowed {g.allowed:.3g}')
        for kind, g in gates:
            g.check((kind, case))


@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('layout', LAYOUTS)
def test_extension_rows_do_not_depend_on_the_mask(ctx, layout, kernel):
    import gpk
    Nd, Nb = SIZES[1]
    rho = RHOS[(LAYOUTS.index(layout) + KERNELS.index(kernel)) % 2]
    Xd, Xb, Xt = _case_points('planted', kernel, Nd, Nb)
    Xt = Xt[:5]                                                         # (holds Xd[3] verbatim and three near-coincident points)
    N = sum(n for _, n in MR.offsets(layout, Nd, Nb))
    coeff = np.random.RandomState(N).normal(size=N)

    def run(which):
        return VA.bits(ctx.extend_functionals(layout, kernel, rho, Xt, Xd, Xb, coeff, which=which).download().reshape(len(which), 5))
    single = {nm: run((nm,))[0] for nm in NAMES}
    differ = []
    for mask in range(1, 32):
        which = tuple(nm for nm in NAMES if mask & gpk.device.FUNCTIONAL[nm])
        out, again = run(which), run(which)
        if not np.array_equal(out, again):
            differ.append((mask, 'repeat'))
        differ += [(mask, nm) for k, nm in enumerate(which) if not np.array_equal(out[k], single[nm])]
    print(f'\n{TAG} masks 1 .. 31 {layout} {kernel} rho {rho}: rows that differ from their single-bit call or from a repeat {differ}')
    assert not differ
