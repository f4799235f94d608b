"""The Gaussian and the anisotropic Gaussian Gram evaluators of the reference layouts on the device, per block, against the long-double
reference of tests/_gauss_reference.py (a three-term recurrence, not the expanded Hermite polynomials the kernels and the oracle share).

Kernels ('Gaussian', 0.2) and ('anisotropic_Gaussian', (0.3, 0.05)); the five layout names; points uniform on the unit square from
RandomState(100 Nd + Nb), three test points equal to collocation points.

  a  gpk_assemble, gpk_assemble_test, gpk_assemble_cross (compared transposed).  (Nd, Nb) = (64, 36): the two-point kernel, a row tail of 4
     behind the 32 rows of a workgroup; (65, 41): the one-point kernel; (1, 0) for the elliptic layout; (530, 46) and (265, 41): two and
     three workgroups along the columns (one kernel per layout, alternating).  Nt in {1, 2, 67, 300, 514, 515}: the tail of the test rows,
     one and two workgroups along t in the cross kernel, even Nt (16-byte stores) and odd Nt (8-byte stores, the last lane computes its
     point twice).  Gate per block: |device - ref| <= (4e-15 + 4 e_np) max|block|.  4e-15 is the project's Gram-block bound; e_np is the
     error of oracle/gp_oracle.py (float64) against the same reference in the same block, measured here; the factor 4 allows for
     contraction and for the device's exp against glibc's.  Theta is exactly symmetric and finite.
  b  nugget none / identity / adaptive: the diagonal of every block against diagonal_values + block_nuggets to 4e-15 of its own magnitude,
     the returned ratios against trace_ratios (rtol 1e-14), unused entries 0
  c  anisotropic (0.3, 0.02): pairs with p2 d2^2 / 2 between 700 and 760 (kappa subnormal in float64) and beyond (kappa = 0): every entry
     finite, and the gate of a
  d  store policies gpk_tune(55, 1 / 2 / 3) and the one-point kernel (gpk_tune(47, 0)): the bits of the default; gpk_assemble_cross under
     key 47 = 0: the bits of its 16-byte form
  e  the three entry points on an unaligned view (odd offset, odd ld) and on an aligned view with ld > N, between canaries: nothing
     outside the view is written, and the bits are those of the plain call
  f  gpk_extend against reference rows @ coeff accumulated in long double: per test point within 64 eps (|rows| @ |coeff|), the form of
     tests/test_gpu_extend_functionals.py (a float64 numpy product of the oracle's rows is within 1.7 eps of it:
     tests/test_gauss_reference_host.py); a repeat gives the same bits
  g  refusals: ld < N (gpk_assemble, gpk_assemble_test), ld < Nt (gpk_assemble_cross): -9001, and nothing is written

Every figure is printed under a [gauss] tag.

RESULTS
  A run on an MI355X (gfx950), every test of this file passing: 339 [gauss] lines.  Per layout and kernel the worst device / e_np / allowed
  (in units of max|block|; the block that comes closest to its allowance, over all sizes and Nt) and the worst extend ratio:
    [gauss] Nonlinear_elliptic Gaussian: assemble 4.1e-16 / 4.1e-16 / 5.64e-15, test rows 2.44e-16 / 2.44e-16 / 4.97e-15, cross columns 2.44e-16 / 2.44e-16 / 4.97e-15, extend 0.593 eps of 64
    [gauss] Nonlinear_elliptic anisotropic_Gaussian: assemble 3.56e-16 / 3.8e-16 / 5.52e-15, test rows 2.61e-16 / 2.57e-16 / 5.03e-15, cross columns 2.27e-16 / 2.27e-16 / 4.91e-15, extend 1.32 eps of 64
    [gauss] Burgers Gaussian: assemble 3.63e-16 / 4.1e-16 / 5.64e-15, test rows 2.93e-16 / 2.82e-16 / 5.13e-15, cross columns 2.99e-16 / 2.7e-16 / 5.08e-15, extend 0.547 eps of 64
    [gauss] Burgers anisotropic_Gaussian: assemble 3.85e-16 / 4.33e-16 / 5.73e-15, test rows 3.29e-16 / 3.29e-16 / 5.31e-15, cross columns 3.4e-16 / 3.03e-16 / 5.21e-15, extend 1.13 eps of 64
    [gauss] Eikonal Gaussian: assemble 4.1e-16 / 4.1e-16 / 5.64e-15, test rows 2.85e-16 / 2.75e-16 / 5.1e-15, cross columns 2.99e-16 / 2.7e-16 / 5.08e-15, extend 0.7 eps of 64
    [gauss] Eikonal anisotropic_Gaussian: assemble 3.51e-16 / 2.75e-16 / 5.1e-15, test rows 3.29e-16 / 3.29e-16 / 5.31e-15, cross columns 3.29e-16 / 3.29e-16 / 5.31e-15, extend 0.948 eps of 64
    [gauss] Darcy_u Gaussian: assemble 3.93e-16 / 3.5e-16 / 5.4e-15, test rows 2.93e-16 / 2.82e-16 / 5.13e-15, cross columns 2.99e-16 / 2.7e-16 / 5.08e-15, extend 0.7 eps of 64
    [gauss] Darcy_u anisotropic_Gaussian: assemble 4.28e-16 / 3.85e-16 / 5.54e-15, test rows 3.29e-16 / 3.29e-16 / 5.31e-15, cross columns 3.4e-16 / 3.03e-16 / 5.21e-15, extend 0.948 eps of 64
    [gauss] Darcy_a Gaussian: assemble 3.71e-16 / 4.51e-16 / 5.81e-15, test rows 2.85e-16 / 2.75e-16 / 5.1e-15, cross columns 2.99e-16 / 2.7e-16 / 5.08e-15, extend 0.3 eps of 64
    [gauss] Darcy_a anisotropic_Gaussian: assemble 3.43e-16 / 3.95e-16 / 5.58e-15, test rows 3.29e-16 / 3.29e-16 / 5.31e-15, cross columns 3.29e-16 / 3.29e-16 / 5.31e-15, extend 0.914 eps of 64
  The far-pair cases (c): worst device 3.93e-16 of max|block|.  The largest device figure printed in the run: 4.28e-16.
"""
import functools

import numpy as np
import pytest

import _gauss_reference as GR
import _view_arena as VA

pytestmark = pytest.mark.gpu

LD = GR.LD
EPS = float(np.finfo(np.float64).eps)
LAYOUTS = tuple(GR.LAYOUTS)
KERNELS = GR.KERNELS
PARAMS = GR.PARAMS
SIZES, LARGE, NTS = GR.SIZES, GR.LARGE, GR.NTS
SPEC = {'Darcy_u': 'Eikonal'}                      # (the same layout id: one reference serves both names)
FAR = ('anisotropic_Gaussian', (0.3, 0.02))


@pytest.fixture(scope='module')
def ctx():
    import gpk
    c = gpk.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _reference(layout, kernel, kp, Nd, Nb):
    """(Theta, Theta_test at all test points) in long double and from the oracle, shared by the tests of one case"""
    Xd, Xb, Xt = GR.case_points(Nd, Nb)
    return (GR.theta(kernel, kp, layout, Xd, Xb), GR.theta_test(kernel, kp, layout, Xt, Xd, Xb),
            GR.oracle_theta(layout, kernel, kp, Xd, Xb), GR.oracle_theta_test(layout, kernel, kp, Xt, Xd, Xb))


def _allowed(w):
    return GR.BOUND + 4 * w[1]


def _parity(ctx, layout, kernel, kp, Nd, Nb, points=None, nts=NTS, tag=''):
    """assemble, assemble_test and assemble_cross of one case through the gate; returns the worst (device, e_np) of each kind"""
    Xd, Xb, Xt = points if points is not None else GR.case_points(Nd, Nb)
    if points is None:
        T, Tt, Tn, Ttn = _reference(SPEC.get(layout, layout), kernel, kp, Nd, Nb)
    else:
        T, Tt = GR.theta(kernel, kp, layout, Xd, Xb), GR.theta_test(kernel, kp, layout, Xt, Xd, Xb)
        Tn, Ttn = GR.oracle_theta(layout, kernel, kp, Xd, Xb), GR.oracle_theta_test(layout, kernel, kp, Xt, Xd, Xb)
    blocks = GR.offsets(layout, Nd, Nb)
    N = T.shape[0]
    dT, _ = ctx.assemble(layout, kernel, kp, Xd, Xb)
    got = dT.download()
    dT.free()
    assert got.shape == (N, N) and np.all(np.isfinite(got))
    assert np.array_equal(got, got.T)
    w = GR.gate_blocks(got, T, Tn, blocks, blocks, ('assemble', layout, kernel, Nd, Nb))
    print(f'\n[gauss] assemble{tag} {layout} {kernel} {kp} ({Nd}, {Nb}): device {w[0]:.3g}, e_np {w[1]:.3g}, allowed {_allowed(w):.3g}')
    worst_t, worst_c = (0.0, 0.0), (0.0, 0.0)
    for Nt in nts:
        rows = [(0, Nt)]
        dt = ctx.assemble_test(layout, kernel, kp, Xt[:Nt], Xd, Xb)
        gt = dt.download().reshape(Nt, N)
        dc = ctx.assemble_cross(layout, kernel, kp, Xt[:Nt], Xd, Xb)
        gc = dc.download().reshape(N, Nt)
        dt.free(); dc.free()
        assert np.all(np.isfinite(gt)) and np.all(np.isfinite(gc))
        wt = GR.gate_blocks(gt, Tt[:Nt], Ttn[:Nt], rows, blocks, ('assemble_test', layout, kernel, Nd, Nb, Nt))
        wc = GR.gate_blocks(gc.T, Tt[:Nt], Ttn[:Nt], rows, blocks, ('assemble_cross', layout, kernel, Nd, Nb, Nt))
        print(f'[gauss] test rows / cross columns{tag} {layout} {kernel} {kp} ({Nd}, {Nb}) Nt {Nt}: device {wt[0]:.3g} / {wc[0]:.3g}, '
              f'e_np {wt[1]:.3g}, allowed {_allowed(wt):.3g}')
        worst_t = max(worst_t, wt, key=lambda v: v[0] / _allowed(v))
        worst_c = max(worst_c, wc, key=lambda v: v[0] / _allowed(v))
    return w, worst_t, worst_c


# ------------------------------------------------------------------------------------------------ a. parity
@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('layout', LAYOUTS)
def test_gram_test_rows_and_cross_columns(ctx, layout, kernel):
    sizes = SIZES + (((1, 0),) if layout == 'Nonlinear_elliptic' else ())
    worst = [_parity(ctx, layout, kernel, PARAMS[kernel], Nd, Nb) for Nd, Nb in sizes]
    for k, kind in enumerate(('assemble', 'test rows', 'cross columns')):
        w = max((v[k] for v in worst), key=lambda v: v[0] / _allowed(v))
        print(f'[gauss] worst {kind} {layout} {kernel}: device {w[0]:.3g}, e_np {w[1]:.3g}, allowed {_allowed(w):.3g}')


@pytest.mark.parametrize('size', range(len(LARGE)))
@pytest.mark.parametrize('layout', LAYOUTS)
def test_gram_with_more_than_one_workgroup_along_the_columns(ctx, layout, size):
    Nd, Nb = LARGE[size]
    kernel = GR.large_kernel(layout, size)
    worst = _parity(ctx, layout, kernel, PARAMS[kernel], Nd, Nb)
    for k, kind in enumerate(('assemble', 'test rows', 'cross columns')):
        w = worst[k]
        print(f'[gauss] worst {kind} {layout} {kernel} ({Nd}, {Nb}): device {w[0]:.3g}, e_np {w[1]:.3g}, allowed {_allowed(w):.3g}')


# ------------------------------------------------------------------------------------------------ b. diagonal and nugget
@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('layout', LAYOUTS)
def test_nugget_diagonal_and_ratios(ctx, layout, kernel):
    kp = PARAMS[kernel]
    for Nd, Nb in SIZES:
        Xd, Xb, _ = GR.case_points(Nd, Nb)
        blocks = GR.offsets(layout, Nd, Nb)
        diag = GR.diagonal_values(kernel, kp, layout)
        want_r = np.asarray(GR.trace_ratios(kernel, kp, layout, Nd, Nb), dtype=np.float64)
        for nugget_type in ('none', 'identity', 'adaptive'):
            dT, ratios = ctx.assemble(layout, kernel, kp, Xd, Xb, 1e-6, nugget_type)
            got = np.diag(dT.download()).astype(LD)
            dT.free()
            np.testing.assert_allclose(ratios[:len(want_r)], want_r, rtol=1e-14)
            assert all(r == 0.0 for r in ratios[len(want_r):])
            nug = GR.block_nuggets(kernel, kp, layout, Nd, Nb, 1e-6, nugget_type)
            for (o, n), c, v in zip(blocks, diag, nug):
                want = c + v
                err = float(np.max(np.abs(got[o:o + n] - want)) / abs(want))
                assert err <= 4e-15, (nugget_type, (Nd, Nb), o, err)


# ------------------------------------------------------------------------------------------------ c. far pairs
def _far_points(Nd, Nb):
    """the points of the case, with the second coordinate of the first domain points set so that the band 700 <= p2 d2^2 / 2 <= 760
    (|d2| in 0.5292 .. 0.5514 for sigma_2 = 0.02) is hit by construction and not only by chance"""
    Xd, Xb, Xt = (X.copy() for X in GR.case_points(Nd, Nb))
    Xd[0, 1], Xd[1, 1], Xd[2, 1], Xd[4, 1] = 0.01, 0.55, 0.5525, 0.999
    Xt[1, 1], Xt[2, 1] = 0.55, 0.999
    return Xd, Xb, Xt[:67]


@pytest.mark.parametrize('layout', LAYOUTS)
def test_far_pairs_underflow_to_zero_and_stay_finite(ctx, layout):
    kernel, kp = FAR
    p2 = float(GR.precisions(kernel, kp)[1])
    for Nd, Nb in SIZES:
        Xd, Xb, Xt = _far_points(Nd, Nb)
        e = 0.5 * p2 * (Xd[:, None, 1] - Xd[None, :, 1]) ** 2
        band, beyond = int(np.sum((e >= 700) & (e <= 760))), int(np.sum(e > 760))
        assert band >= 4 and beyond >= 2, 'precondition: the points hold no pair in the band / beyond it'
        print(f'\n[gauss] far pairs {layout} ({Nd}, {Nb}): {band} domain pairs with 700 <= p2 d2^2 / 2 <= 760, {beyond} beyond')
        _parity(ctx, layout, kernel, kp, Nd, Nb, points=(Xd, Xb, Xt), nts=(67,), tag=' (far)')


# ------------------------------------------------------------------------------------------------ d. store policies, kernel variants
@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('layout', LAYOUTS)
def test_store_policies_and_kernel_variants_give_the_same_bits(ctx, layout, kernel):
    Nd, Nb = SIZES[0]
    kp = PARAMS[kernel]
    Xd, Xb, Xt = GR.case_points(Nd, Nb)
    Xt = Xt[:300]                                                      # (even: the 16-byte form of the cross kernel by default)

    def run():
        T, _ = ctx.assemble(layout, kernel, kp, Xd, Xb, 1e-6, 'adaptive')
        out = VA.bits(T.download())
        T.free()
        return out

    def run_cross():
        K = ctx.assemble_cross(layout, kernel, kp, Xt, Xd, Xb)
        out = VA.bits(K.download())
        K.free()
        return out
    default, default_c = run(), run_cross()
    try:
        for v in (1, 2, 3):
            ctx.tune(55, v)
            assert np.array_equal(run(), default), ('key 55', v)
        ctx.tune(55, 0)
        ctx.tune(47, 0)
        assert np.array_equal(run(), default), 'key 47 = 0'
        assert np.array_equal(run_cross(), default_c), 'key 47 = 0, cross'
    finally:
        ctx.tune(55, 0)
        ctx.tune(47, 1)
    assert np.array_equal(run(), default)                              # (both keys are back)


# ------------------------------------------------------------------------------------------------ e. views
def _raw(ctx, layout, kernel, kp, Xd, Xb, Xt):
    """the three entry points through the C ABI on a caller's pointer and ld: (N, call(which, ptr, ld, Nt) -> return code)"""
    import gpk
    Nd, Nb = Xd.shape[0], Xb.shape[0]
    N = sum(n for _, n in GR.offsets(layout, Nd, Nb))
    dXd, dXb, dXt = ctx.points(Xd), ctx.points(Xb), ctx.points(Xt)
    lay, kid, kpar = gpk.LAYOUT[layout], gpk.KERNEL[kernel], gpk.device.kernel_params(kernel, kp)

    def call(which, ptr, ld, Nt=None):
        if which == 'assemble':
            return ctx.lib.gpk_assemble(ctx.h, lay, kid, kpar, dXd.ptr, Nd, dXb.ptr, Nb, 1e-6, gpk.NUGGET['adaptive'], ptr, ld, None)
        entry = ctx.lib.gpk_assemble_test if which == 'assemble_test' else ctx.lib.gpk_assemble_cross
        return entry(ctx.h, lay, kid, kpar, dXt.ptr, Nt, dXd.ptr, Nd, dXb.ptr, Nb, ptr, ld)
    return N, call


@pytest.mark.parametrize('cls', ['D', 'A'])
@pytest.mark.parametrize('layout', LAYOUTS)
def test_views_between_canaries(ctx, layout, cls):
    """class D: odd base offset and odd ld (8-byte stores everywhere); class A with ld > N: the 16-byte stores of the two-point kernel and
    of the cross kernel next to canaries"""
    Nd, Nb = SIZES[0]
    kernel = KERNELS[LAYOUTS.index(layout) % 2]
    kp = PARAMS[kernel]
    Xd, Xb, Xt = GR.case_points(Nd, Nb)
    Nt = 67 if cls == 'D' else 66
    Xt = Xt[:Nt]
    N, call = _raw(ctx, layout, kernel, kp, Xd, Xb, Xt)
    plain, _ = ctx.assemble(layout, kernel, kp, Xd, Xb, 1e-6, 'adaptive')
    plain_t = ctx.assemble_test(layout, kernel, kp, Xt, Xd, Xb)
    plain_c = ctx.assemble_cross(layout, kernel, kp, Xt, Xd, Xb)
    want = {'assemble': plain.download().reshape(N, N), 'assemble_test': plain_t.download().reshape(Nt, N),
            'assemble_cross': plain_c.download().reshape(N, Nt)}
    for which, (m, n) in (('assemble', (N, N)), ('assemble_test', (Nt, N)), ('assemble_cross', (N, Nt))):
        v = VA.class_view(ctx, m, n, cls, ld_min=n + 8)
        assert v.cls == cls and v.ld > n
        ctx._chk(call(which, v.ptr, v.ld, Nt))
        ctx.synchronize()
        v.arena.assert_outside_untouched([v])
        assert np.array_equal(VA.bits(v.arena.get(v)), VA.bits(want[which])), which
        v.arena.free()
    for a in (plain, plain_t, plain_c):
        a.free()


# ------------------------------------------------------------------------------------------------ f. extension
@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('layout', LAYOUTS)
def test_extend_against_long_double_rows(ctx, layout, kernel):
    """(65, 41): the lanes' stride loop runs once, partly filled; (265, 41), for the kernel of that size: M = 306 > 256, it runs twice"""
    kp = PARAMS[kernel]
    sizes = [SIZES[1]] + [s for k, s in enumerate(LARGE) if s[0] % 2 and GR.large_kernel(layout, k) == kernel]
    Nt = 67                                                            # (holds collocation points: Xt[0], Xt[5], Xt[66])
    worst = 0.0
    for Nd, Nb in sizes:
        Xd, Xb, Xt = GR.case_points(Nd, Nb)
        Xt = Xt[:Nt]
        rows = GR.theta_test(kernel, kp, SPEC.get(layout, layout), Xt, Xd, Xb)
        N = rows.shape[1]
        coeff = np.random.RandomState(N).normal(size=N)
        want = rows @ coeff.astype(LD)
        terms = np.abs(rows) @ np.abs(coeff).astype(LD)
        got = ctx.extend(layout, kernel, kp, Xt, Xd, Xb, coeff).download()
        assert got.shape == (Nt,) and np.all(np.isfinite(got))
        ratio = float(np.max(np.abs(got.astype(LD) - want) / (EPS * terms)))
        print(f'\n[gauss] extend {layout} {kernel} {kp} ({Nd}, {Nb}): worst |device - ref| / (eps |rows| @ |coeff|) = {ratio:.3g}, allowed 64')
        worst = max(worst, ratio)
        assert ratio <= 64, (Nd, Nb)
        again = ctx.extend(layout, kernel, kp, Xt, Xd, Xb, coeff).download()
        assert np.array_equal(VA.bits(again), VA.bits(got))
    print(f'[gauss] worst extend {layout} {kernel}: {worst:.3g} eps')


# ------------------------------------------------------------------------------------------------ g. refusals
@pytest.mark.parametrize('layout', LAYOUTS)
def test_a_leading_dimension_below_the_row_length_is_refused(ctx, layout):
    """The arena holds the full m x n region (ld = n) between two canary rows above and two below, so rows of a shorter ld written by a
    call that did not refuse would still lie inside the allocation: the test finds them as changed canaries, and can never write out of
    bounds."""
    Nd, Nb = SIZES[1]
    kernel = KERNELS[LAYOUTS.index(layout) % 2]
    Xd, Xb, Xt = GR.case_points(Nd, Nb)
    Nt = 67
    N, call = _raw(ctx, layout, kernel, PARAMS[kernel], Xd, Xb, Xt[:Nt])
    for which, (m, n), text in (('assemble_test', (Nt, N), b'assemble_test: ld < N'), ('assemble', (N, N), b'assemble: ld < N'),
                                ('assemble_cross', (N, Nt), b'assemble_cross: ld < Nt')):
        arena = VA.Arena(ctx, m + 4, n)
        v = arena.view(2, 0, m, n)
        assert v.ld == n and arena.size - v.offset >= m * n
        for ld in (n - 1, 1, 0, -1):
            assert call(which, v.ptr, ld, Nt) == -9001, (which, ld)
            assert text in ctx.lib.gpk_last_error(ctx.h), (which, ld)
        ctx.synchronize()
        arena.assert_outside_untouched([])                             # (no view was written: every element is still the canary)
        assert call(which, v.ptr, n, Nt) == 0                          # ld = n exactly is served
        ctx.synchronize()
        arena.assert_outside_untouched([v])
        assert np.all(np.isfinite(arena.get(v)))
        arena.free()


def test_assemble_test_names_its_refusals(ctx):
    Nd, Nb = 8, 4
    Xd, Xb, Xt = GR.case_points(Nd, Nb)
    N, call = _raw(ctx, 'Burgers', 'Gaussian', 0.2, Xd, Xb, Xt[:5])
    out = ctx.empty(5, N)
    assert call('assemble_test', None, out.ld, 5) == -9001 and b'assemble_test: pointers' in ctx.lib.gpk_last_error(ctx.h)
    for Nt in (0, -3):
        assert call('assemble_test', out.ptr, out.ld, Nt) == -9001 and b'assemble_test: Nt <= 0' in ctx.lib.gpk_last_error(ctx.h)
    assert call('assemble_test', out.ptr, out.ld, 5) == 0
    ctx.synchronize()
    out.free()
