"""The evolution Gram layout (gpk_assemble_evo, gpk_extend_functionals_evo), the Burgers system on it and the class Evolution1d on the
device, against tests/_evo_reference.py.

  a. Gram, per block, against long double.  (N_d, N_b) = (1, 1), (31, 3), (32, 32), (33, 7), (200, 57), (480, 34): N_d = 31, 32, 33 around the
     32 row points of a workgroup, M = N_d + N_b = 257 past the 256 column points of a workgroup of the one-point kernel, M = 514 (all
     even) past the 512 of the two-point kernel.  Coefficient sets: Kuramoto-Sivashinsky, Kawahara and a set with all of c2..c5; bc NULL
     and a mixed (N_b, 3) array; both kernels; coincident points.  Gate per block: |device - ref| <= 8 e_np max|block| with e_np the error
     of the float64 numpy twin of the reference on the same inputs (at least eps / 2: _evo_reference.allowance).  Bitwise symmetric,
     bitwise repeatable; the one-point and the two-point kernel and the two store policies give the same bits; the ratios are the
     analytic values.
  b. views with an odd ld and a base offset by one double, between canaries; refusals, each with its message, write nothing.
  c. with c = (0, delta, 0, 0) and no bc, Theta against gpk_assemble_disp's scaled by delta in the rows and columns of block 2.
  d. the extension: every subset of the five rows at N_t = 1, 3, 4, 5, 9 (four test points per workgroup) against long double, relative
     to the largest value of the row on the nine test points, 8 x the twin's error; a repeated call gives the same bits; refusals.
  e. one gpk_gn_step on the factor of the device's own Theta, system Burgers with nu = -1, against the long-double reference of
     tests/_gn_reference.py by its gates (32 x the float64 pipeline's own figure + 1): the modes of tests/test_gpu_kdv.py.
  f. the class Evolution1d on a manufactured solution: Kuramoto-Sivashinsky with clamped walls, Kawahara with Dirichlet data.
Every test prints what it measures under an [evo] tag.  RESULTS: DESIGN.md section K, "Evolution equations: the general spatial operator"."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import _evo_reference as E
import _gn_reference as R
import _kdv_reference as K
import _view_arena as VA

pytestmark = pytest.mark.gpu

LD, EPS = E.LD, E.EPS
PARAMS = {'Gaussian': 0.2, 'anisotropic_Gaussian': (0.3, 0.15)}
SIZES = ((1, 1), (31, 3), (32, 32), (33, 7), (200, 57), (480, 34))
SETS = {'ks': E.KS, 'kawahara': E.KAWAHARA, 'full': E.FULL}
NAMES5 = E.FUNCTIONAL_NAMES


@pytest.fixture(scope='module')
def ctx():
    import gpk
    c = gpk.Context(0)
    yield c
    c.close()


def gram_points(Nd, Nb):
    """uniform points on the unit square; where there is room a coincident domain pair and a boundary point on a domain point"""
    rng = np.random.RandomState(1000 * Nd + Nb)
    Xd, Xb = rng.uniform(0, 1, (Nd, 2)), rng.uniform(0, 1, (Nb, 2))
    if Nd > 6:
        Xd[6] = Xd[5]
    if Nb:
        Xb[Nb - 1] = Xd[Nd - 1]
    return Xd, Xb


def mixed_bc(Nb):
    """rows (c0, c1, c2): Dirichlet, d_x, d_t and Robin-like rows in turn, then random ones"""
    bc = np.random.RandomState(Nb).normal(size=(Nb, 3))
    for b, row in enumerate(((1, 0, 0), (0, 0, 1), (0, 1, 0), (0.5, 0, -2.0))):
        if b < Nb:
            bc[b] = row
    return bc


@functools.lru_cache(maxsize=None)
def _reference(kernel, cset, mixed, Nd, Nb):
    Xd, Xb = gram_points(Nd, Nb)
    bc = mixed_bc(Nb) if mixed else None
    c = SETS[cset]
    return Xd, Xb, bc, E.theta(kernel, PARAMS[kernel], c, Xd, Xb, bc), E.theta(kernel, PARAMS[kernel], c, Xd, Xb, bc, np.float64)


def _download(ctx, *args, **kw):
    T, ratios = ctx.assemble_evo(*args, **kw)
    out = T.download()
    T.free()
    return out, ratios


# ------------------------------------------------------------------------------------------------ a. Gram entries
GRAM_CASES = [(K.KERNELS[(i + j + k) % 2], cset, bool(mixed), size) for i, size in enumerate(SIZES) for j, cset in enumerate(SETS)
              for k, mixed in enumerate((0, 1))]


@pytest.mark.parametrize('kernel,cset,mixed,size', GRAM_CASES,
                         ids=[f'{k}-{c}-{"bc" if m else "delta"}-{s[0]}-{s[1]}' for k, c, m, s in GRAM_CASES])
def test_gram_blocks_against_long_double(ctx, kernel, cset, mixed, size):
    Nd, Nb = size
    Xd, Xb, bc, T, Tn = _reference(kernel, cset, mixed, Nd, Nb)
    N = 4 * Nd + Nb
    got, ratios = _download(ctx, kernel, PARAMS[kernel], SETS[cset], Xd, Xb, bc)
    again, _ = _download(ctx, kernel, PARAMS[kernel], SETS[cset], Xd, Xb, bc)
    assert got.shape == (N, N) and np.all(np.isfinite(got))
    assert np.array_equal(VA.bits(got), VA.bits(again)), 'not repeatable to the bit'
    assert np.array_equal(VA.bits(got), VA.bits(np.ascontiguousarray(got.T))), 'not symmetric to the bit'
    np.testing.assert_allclose(ratios, np.asarray(E.trace_ratios(kernel, PARAMS[kernel], SETS[cset], Nd, Nb, bc), dtype=np.float64), rtol=4 * EPS)
    errs = E.block_errors(got, T, Tn, Nd, Nb)
    print()
    bad = []
    for (i, j), (e, en) in sorted(errs.items()):               # every figure before the gate
        print(f'[evo gram] {kernel} {cset} bc {mixed} ({Nd}, {Nb}) <{E.NAMES[i]},{E.NAMES[j]}>: device {e / EPS:.3g} eps, numpy {en / EPS:.3g} eps '
              f'of max|block|, allowed {E.allowance(en) / EPS:.3g} eps')
        if not e <= E.allowance(en):
            bad.append((E.NAMES[i], E.NAMES[j], e / EPS, en / EPS))
    assert not bad, bad


@pytest.mark.parametrize('kernel,cset,size', [('Gaussian', 'full', (64, 36)), ('anisotropic_Gaussian', 'ks', (32, 32)),
                                              ('anisotropic_Gaussian', 'kawahara', (480, 34))])
def test_kernels_and_store_paths_give_the_same_bits(ctx, kernel, cset, size):
    """everything even and the base aligned: the two-point kernel runs; key 47 = 0 sends the same call to the one-point kernel"""
    Nd, Nb = size
    Xd, Xb = gram_points(Nd, Nb)
    bc = mixed_bc(Nb)

    def run():
        return VA.bits(_download(ctx, kernel, PARAMS[kernel], SETS[cset], Xd, Xb, bc, 1e-6, 'adaptive')[0])
    default = run()
    try:
        ctx.tune(55, 1)
        assert np.array_equal(run(), default), 'non-temporal 16-byte stores'
        ctx.tune(55, 0)
        ctx.tune(47, 0)
        assert np.array_equal(run(), default), 'one-point kernel (key 47 = 0)'
    finally:
        ctx.tune(55, 0)
        ctx.tune(47, 1)
    assert np.array_equal(run(), default)


@pytest.mark.parametrize('kernel', K.KERNELS)
def test_nugget_diagonal_and_ratios(ctx, kernel):
    kp, c = PARAMS[kernel], E.FULL
    for (Nd, Nb), mixed in (((33, 7), True), ((32, 32), False), ((1, 1), True)):
        Xd, Xb = gram_points(Nd, Nb)
        bc = mixed_bc(Nb) if mixed else None
        want_r = np.asarray(E.trace_ratios(kernel, kp, c, Nd, Nb, bc), dtype=np.float64)
        plain, _ = _download(ctx, kernel, kp, c, Xd, Xb, bc)
        for nugget_type in ('none', 'identity', 'adaptive'):
            full, ratios = _download(ctx, kernel, kp, c, Xd, Xb, bc, 1e-6, nugget_type)
            np.testing.assert_allclose(ratios, want_r, rtol=4 * EPS)              # written for every nugget type
            for (o, n), v in zip(E.offsets(Nd, Nb), E.block_nuggets(kernel, kp, c, Nd, Nb, 1e-6, nugget_type, bc)):
                d0 = np.diag(plain)[o:o + n]
                assert np.max(np.abs(np.diag(full)[o:o + n].astype(LD) - (d0.astype(LD) + v)) / np.abs(d0)) <= 2 * EPS, (nugget_type, (Nd, Nb), o)
            off = full - np.diag(np.diag(full))
            assert np.array_equal(VA.bits(off), VA.bits(plain - np.diag(np.diag(plain)))), 'the nugget touches the diagonal only'


# ------------------------------------------------------------------------------------------------ b. views and refusals
@pytest.mark.parametrize('cls,Nd,Nb', [('D', 33, 7), ('D', 26, 6), ('A', 26, 6), ('B', 26, 6), ('C', 2, 3)])
def test_views_between_canaries(ctx, cls, Nd, Nb):
    """class D: base offset by one double and odd ld; B / C: one of the two; A with ld > N: the 16-byte stores next to canaries"""
    import gpk
    kernel, c = 'anisotropic_Gaussian', E.FULL
    kp = gpk.device.kernel_params(kernel, PARAMS[kernel])
    c4 = (C.c_double * 4)(*c)
    Xd, Xb = gram_points(Nd, Nb)
    bc = mixed_bc(Nb)
    N = 4 * Nd + Nb
    want, _ = _download(ctx, kernel, PARAMS[kernel], c, Xd, Xb, bc, 1e-6, 'adaptive')
    dXd, dXb, dbc = ctx.points(Xd), ctx.points(Xb), ctx._boundary_coeffs(bc, Nb)     # (Nb, 3) with ld = 3, as the C ABI expects
    v = VA.class_view(ctx, N, N, cls, ld_min=N + 8)
    assert v.cls == cls and v.ld > N
    fn = ctx.lib.gpk_assemble_evo
    kid, adaptive = gpk.KERNEL[kernel], gpk.NUGGET['adaptive']
    ctx._chk(fn(ctx.h, kid, kp, c4, dXd.ptr, Nd, dXb.ptr, Nb, dbc.ptr, 1e-6, adaptive, v.ptr, v.ld, None))
    ctx.synchronize()
    v.arena.assert_outside_untouched([v])
    assert np.array_equal(VA.bits(v.arena.get(v)), VA.bits(want))
    # refusals write nothing
    def refused(message, *args):
        assert fn(ctx.h, *args) == -9001, message
        assert message in ctx.lib.gpk_last_error(ctx.h), (message, ctx.lib.gpk_last_error(ctx.h))
    refused(b'assemble_evo: ld < N', kid, kp, c4, dXd.ptr, Nd, dXb.ptr, Nb, dbc.ptr, 1e-6, adaptive, v.ptr, N - 1, None)
    refused(b'assemble_evo: nugget_type', kid, kp, c4, dXd.ptr, Nd, dXb.ptr, Nb, dbc.ptr, 1e-6, 7, v.ptr, v.ld, None)
    refused(b'assemble_evo: sizes/pointers', kid, kp, c4, dXd.ptr, 0, dXb.ptr, Nb, dbc.ptr, 1e-6, 0, v.ptr, v.ld, None)
    refused(b'assemble_evo: sizes/pointers', kid, kp, c4, dXd.ptr, Nd, dXb.ptr, -1, dbc.ptr, 1e-6, 0, v.ptr, v.ld, None)
    refused(b'assemble_evo: sizes/pointers', kid, kp, c4, dXd.ptr, Nd, None, Nb, dbc.ptr, 1e-6, 0, v.ptr, v.ld, None)
    for bad in ((0.0, 0.0, 0.0, 0.0), (1.0, np.nan, 0.0, 0.0), (0.0, 0.0, np.inf, 1.0)):
        refused(b'assemble_evo: c2..c5 must be finite and not all zero', kid, kp, (C.c_double * 4)(*bad), dXd.ptr, Nd, dXb.ptr, Nb, dbc.ptr,
                1e-6, 0, v.ptr, v.ld, None)
    refused(b'assemble_evo: c2..c5 must be finite and not all zero', kid, kp, None, dXd.ptr, Nd, dXb.ptr, Nb, dbc.ptr, 1e-6, 0, v.ptr, v.ld, None)
    for other in (8, 9, 10, 16, 2):                                     # the Matern ids, the periodic kernel, an unknown id
        refused(b'assemble_evo: kernel id', other, (C.c_double * 4)(0.5, 0.5, 0.0, 1.0), c4, dXd.ptr, Nd, dXb.ptr, Nb, dbc.ptr, 0.0, 0, v.ptr, v.ld, None)
    ctx.synchronize()
    v.arena.assert_outside_untouched([v])
    assert np.array_equal(VA.bits(v.arena.get(v)), VA.bits(want))
    v.arena.free()


# ------------------------------------------------------------------------------------------------ c. reduction to the dispersive layout
@pytest.mark.parametrize('kernel,size,delta', [('Gaussian', (33, 7), 1.0), ('anisotropic_Gaussian', (200, 57), 0.02), ('anisotropic_Gaussian', (64, 36), -3.0)])
def test_reduces_to_the_dispersive_layout(ctx, kernel, size, delta):
    Nd, Nb = size
    Xd, Xb = gram_points(Nd, Nb)
    c = (0.0, delta, 0.0, 0.0)
    got, ratios = _download(ctx, kernel, PARAMS[kernel], c, Xd, Xb, None)
    dT, dr = ctx.assemble_disp(kernel, PARAMS[kernel], Xd, Xb)
    disp = dT.download()
    dT.free()
    s = np.ones(4 * Nd + Nb)
    s[2 * Nd:3 * Nd] = delta
    want = disp * s[:, None] * s[None, :]                                # (exact for delta = 1; one rounding per factor otherwise)
    ref = E.theta(kernel, PARAMS[kernel], c, Xd, Xb)
    twin = E.theta(kernel, PARAMS[kernel], c, Xd, Xb, None, np.float64)
    errs = E.block_errors(want, ref, twin, Nd, Nb)
    print()
    for (i, j), (_, en) in sorted(errs.items()):
        o = E.offsets(Nd, Nb)
        (ro, rn), (co, cn) = o[i], o[j]
        diff = float(np.max(np.abs(got[ro:ro + rn, co:co + cn] - want[ro:ro + rn, co:co + cn]))) / float(np.max(np.abs(ref[ro:ro + rn, co:co + cn])))
        print(f'[evo kdv] {kernel} ({Nd}, {Nb}) delta {delta} <{E.NAMES[i]},{E.NAMES[j]}>: evo - scaled disp {diff / EPS:.3g} eps of max|block|, '
              f'allowed {E.allowance(en) / EPS:.3g}')
        assert diff <= E.allowance(en), (i, j)
    np.testing.assert_allclose(ratios, [dr[0], dr[1], dr[2] * delta * delta], rtol=4 * EPS)


# ------------------------------------------------------------------------------------------------ d. extension
MASKS = [tuple(n for n, on in zip(NAMES5, sel) if on) for sel in itertools.product((0, 1), repeat=5) if any(sel)]
EXT = (265, 41)                                                      # M = 306: the lanes' stride loop runs twice, the second time partly filled
NT_ALL = 9


@functools.lru_cache(maxsize=None)
def _extension_reference(kernel, cset, mixed):
    Nd, Nb = EXT
    Xd, Xb = gram_points(Nd, Nb)
    bc = mixed_bc(Nb) if mixed else None
    c = SETS[cset]
    N = 4 * Nd + Nb
    rng = np.random.RandomState(N)
    coeff = rng.normal(size=N)
    Xt = rng.uniform(0, 1, (NT_ALL, 2))
    Xt[0], Xt[2], Xt[8] = Xd[3], Xb[2], Xd[Nd - 1]                     # collocation points among the test points
    want, allowed = {}, {}
    for name in NAMES5:
        w = E.rows(kernel, PARAMS[kernel], c, name, Xt, Xd, Xb, bc) @ coeff.astype(LD)
        twin = E.rows(kernel, PARAMS[kernel], c, name, Xt, Xd, Xb, bc, np.float64) @ coeff
        scale = float(np.max(np.abs(w)))
        want[name] = w
        allowed[name] = (scale, E.allowance(float(np.max(np.abs(twin.astype(LD) - w))) / scale))
    return Xd, Xb, bc, Xt, coeff, want, allowed


@pytest.mark.parametrize('Nt', (1, 3, 4, 5, 9))
@pytest.mark.parametrize('kernel,cset,mixed', [('Gaussian', 'ks', True), ('anisotropic_Gaussian', 'kawahara', False), ('anisotropic_Gaussian', 'full', True)])
def test_extension_every_mask(ctx, kernel, cset, mixed, Nt):
    kp, c = PARAMS[kernel], SETS[cset]
    Xd, Xb, bc, Xt_all, coeff, want, allowed = _extension_reference(kernel, cset, mixed)
    Xt = Xt_all[:Nt]
    dc = ctx.array(coeff)
    single = {n: ctx.extend_functionals_evo(kernel, kp, c, Xt, Xd, Xb, bc, dc, which=(n,)).download().reshape(Nt) for n in NAMES5}
    print()
    for n in NAMES5:
        scale, allow = allowed[n]
        err = float(np.max(np.abs(single[n].astype(LD) - want[n][:Nt]))) / scale
        print(f'[evo extend] {kernel} {cset} bc {mixed} Nt {Nt} {n}: error {err / EPS:.3g} eps of max|row|, allowed {allow / EPS:.3g}')
        assert np.all(np.isfinite(single[n])) and err <= allow, (n, Nt, err / EPS, allow / EPS)
    for mask in MASKS:
        out = ctx.extend_functionals_evo(kernel, kp, c, Xt, Xd, Xb, bc, dc, which=mask).download().reshape(len(mask), Nt)
        for k, n in enumerate(mask):
            assert np.array_equal(VA.bits(out[k]), VA.bits(single[n])), (mask, n, 'the bits of a row depend on the other rows')
    again = ctx.extend_functionals_evo(kernel, kp, c, Xt, Xd, Xb, bc, dc, which=NAMES5).download().reshape(5, Nt)
    for k, n in enumerate(NAMES5):
        assert np.array_equal(VA.bits(again[k]), VA.bits(single[n])), 'not repeatable to the bit'
    pair = ctx.extend_functionals_evo(kernel, kp, c, Xt, Xd, Xb, bc, dc, which=('q', 'd1')).download().reshape(2, Nt)   # the caller's order
    assert np.array_equal(VA.bits(pair[0]), VA.bits(single['q'])) and np.array_equal(VA.bits(pair[1]), VA.bits(single['d1']))


def test_extension_refusals_leave_out_untouched(ctx):
    import gpk
    Nd, Nb, Nt = 33, 7, 5
    Xd, Xb = gram_points(Nd, Nb)
    dXd, dXb, dXt, dbc = ctx.points(Xd), ctx.points(Xb), ctx.points(Xd[:Nt]), ctx._boundary_coeffs(mixed_bc(Nb), Nb)
    coeff = ctx.array(np.ones(4 * Nd + Nb))
    out = ctx.empty(5, 8, ld=8)
    canary = np.full((5, 8), 3.25)
    out.upload(canary)
    kp = gpk.device.kernel_params('Gaussian', 0.2)
    c4 = (C.c_double * 4)(*E.FULL)
    fn = ctx.lib.gpk_extend_functionals_evo
    full = 1 | 2 | 4 | 8 | 128

    def refused(message, *args):
        assert fn(ctx.h, *args) == -9001, message
        assert message in ctx.lib.gpk_last_error(ctx.h), (message, ctx.lib.gpk_last_error(ctx.h))
    refused(b'extend_functionals_evo: ldo < Nt', 0, kp, c4, dXt.ptr, Nt, dXd.ptr, Nd, dXb.ptr, Nb, dbc.ptr, coeff.ptr, full, out.ptr, Nt - 1)
    for mask in (0, -1, 16, 32, 64, 128 | 64, 1 | 32, 256 | 1):          # empty, negative, the Laplacian, d/dx3, u_xxx, bits above
        refused(b'extend_functionals_evo: fmask', 0, kp, c4, dXt.ptr, Nt, dXd.ptr, Nd, dXb.ptr, Nb, dbc.ptr, coeff.ptr, mask, out.ptr, 8)
    for other in (8, 9, 10, 16, 2):                                      # Matern, periodic, unknown
        refused(b'extend_functionals_evo: kernel id', other, (C.c_double * 4)(0.5, 0.5, 0.0, 1.0), c4, dXt.ptr, Nt, dXd.ptr, Nd, dXb.ptr, Nb,
                dbc.ptr, coeff.ptr, full, out.ptr, 8)
    for bad in ((0.0, 0.0, 0.0, 0.0), (np.nan, 1.0, 0.0, 0.0)):
        refused(b'extend_functionals_evo: c2..c5 must be finite and not all zero', 0, kp, (C.c_double * 4)(*bad), dXt.ptr, Nt, dXd.ptr, Nd,
                dXb.ptr, Nb, dbc.ptr, coeff.ptr, full, out.ptr, 8)
    refused(b'extend_functionals_evo: Nt <= 0', 0, kp, c4, dXt.ptr, 0, dXd.ptr, Nd, dXb.ptr, Nb, dbc.ptr, coeff.ptr, full, out.ptr, 8)
    refused(b'extend_functionals_evo: pointers', 0, kp, c4, None, Nt, dXd.ptr, Nd, dXb.ptr, Nb, dbc.ptr, coeff.ptr, full, out.ptr, 8)
    refused(b'extend_functionals_evo: sizes/pointers', 0, kp, c4, dXt.ptr, Nt, dXd.ptr, 0, dXb.ptr, Nb, dbc.ptr, coeff.ptr, full, out.ptr, 8)
    # every other call refuses the new bit
    o4 = ctx.empty(5, 8, ld=8)
    assert ctx.lib.gpk_extend_functionals(ctx.h, 1, 0, kp, dXt.ptr, Nt, dXd.ptr, Nd, dXb.ptr, Nb, coeff.ptr, 128, o4.ptr, 8) == -9001
    assert ctx.lib.gpk_extend_functionals(ctx.h, 1, 0, kp, dXt.ptr, Nt, dXd.ptr, Nd, dXb.ptr, Nb, coeff.ptr, 1 | 128, o4.ptr, 8) == -9001
    assert ctx.lib.gpk_extend_functionals_disp(ctx.h, 0, kp, dXt.ptr, Nt, dXd.ptr, Nd, dXb.ptr, Nb, coeff.ptr, 1 | 128, o4.ptr, 8) == -9001
    assert ctx.lib.gpk_extend_functionals_bc(ctx.h, 0, kp, dXt.ptr, Nt, dXd.ptr, Nd, dXb.ptr, Nb, dbc.ptr, coeff.ptr, 1 | 128, o4.ptr, 8) == -9001
    assert ctx.lib.gpk_extend_functionals_hess(ctx.h, 0, kp, dXt.ptr, Nt, dXd.ptr, Nd, dXb.ptr, Nb, coeff.ptr, 1 | 128, o4.ptr, 8) == -9001
    ctx.synchronize()
    assert np.array_equal(out.download(), canary)
    assert fn(ctx.h, 0, kp, c4, dXt.ptr, Nt, dXd.ptr, Nd, dXb.ptr, Nb, dbc.ptr, coeff.ptr, 1 | 128, out.ptr, 8) == 0     # rows 0, 1; entries past Nt untouched
    ctx.synchronize()
    got = out.download()
    assert np.all(got[:2, :Nt] != 3.25) and np.array_equal(got[:2, Nt:], canary[:2, Nt:]) and np.array_equal(got[2:], canary[2:])


# ------------------------------------------------------------------------------------------------ e. one Gauss-Newton step
STEP = (65, 13)
STEP_KERNEL = ('Gaussian', 0.15)
STEP_ALPHA = 6.0


@pytest.fixture(scope='module')
def step_case(ctx):
    """the factor of the device's own Theta (gpk_assemble_evo + gpk_potrf), downloaded: the step is judged on exactly this factor"""
    Nd, Nb = STEP
    rng = np.random.RandomState(65)
    Xd, Xb = rng.uniform(0, 1, (Nd, 2)), rng.uniform(0, 1, (Nb, 2))
    dT, _ = ctx.assemble_evo(*STEP_KERNEL, E.KS, Xd, Xb, mixed_bc(Nb), 1e-6, 'adaptive')
    assert ctx.potrf(dT) == 0
    L = np.tril(dT.download())
    f, g = rng.uniform(0.5, 1.5, Nd), rng.uniform(0.5, 1.5, Nb)
    z0 = rng.uniform(0.3, 1.2, 3 * Nd) * rng.choice([-1.0, 1.0], 3 * Nd)
    cs = E.Case(Nd, Nb, f, g, STEP_ALPHA, L, z0)
    return cs, dT, R.VectorReference(cs, z0)


@pytest.mark.parametrize('dinv,structured', [(256, False), (False, False), (256, 1), (256, 2)],
                         ids=['dinv', 'substitution', 'structured-1', 'structured-2'])
def test_step_against_the_reference(ctx, step_case, dinv, structured):
    import gpk
    cs, dL, ref = step_case
    prob = gpk.GNProblem(ctx, 'Burgers', cs.Nd, cs.Nb, cs.f, cs.g, dL, p0=cs.p0, p1=cs.p1, dinv=dinv, structured=structured)
    assert cs.p1 == -1.0
    z = ctx.array(cs.z0)
    loss, info = ctx.gn_step(prob, z, 1.0)
    delta, z_out = prob.workspace()[2].download().copy(), z.download().copy()
    prob.free()
    print()
    bad = [] if info == 0 else [f'info = {info}']
    for name, (r, a) in (('loss', R.gate_loss(ref, loss)), ('backward', R.gate_backward_vec(ref, delta)), ('forward', R.gate_forward(ref, delta)),
                         ('update', R.gate_update(cs.z0, 1.0, delta, z_out))):
        print(f'[evo step] dinv {dinv} structured {structured} {name}: device {r:.3g}, allowed {a:.3g}')
        if not r <= a:
            bad.append(f'{name}: {r:.4g} > {a:.4g}')
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ f. the class
CLASS = dict(Nd=200, Nb=80, kernel='anisotropic_Gaussian', kp=(0.6, 0.5), nugget=1e-8, steps=8, alpha=1.0)


@pytest.mark.parametrize('equation,bc', [(('kuramoto_sivashinsky',), 'clamped'), (('kawahara', 1.0, -0.5), 'dirichlet')], ids=['ks-clamped', 'kawahara'])
def test_class_on_a_manufactured_solution(equation, bc):
    from scipy.linalg import cho_solve
    import _evidence_reference as EV
    from src.PDEs import Evolution1d
    Nd, Nb, kernel, kp, steps, alpha = (CLASS[k] for k in ('Nd', 'Nb', 'kernel', 'kp', 'steps', 'alpha'))
    c = tuple(E.equation_coeffs(equation))
    Xd, Xb = E.class_points(Nd, Nb)
    f = E.smooth_rhs(alpha, c)
    e = Evolution1d(alpha=alpha, equation=equation, bdy=E.smooth_truth, rhs=f, domain=E.DOMAIN, bc=bc, bdy_x=E.smooth_truth_x if bc == 'clamped' else None)
    e.get_sampled_points(Xd, Xb)
    # the numpy pipeline's boundary: points, rows and data
    if bc == 'clamped':
        Xb2, rows, wall = E.clamped_boundary(Xb, E.DOMAIN)
        g = np.concatenate([E.smooth_truth(Xb[:, 0], Xb[:, 1]), E.smooth_truth_x(Xb[wall, 0], Xb[wall, 1])])
        assert wall.size > 0
    else:
        Xb2, rows, g = Xb, None, E.smooth_truth(Xb[:, 0], Xb[:, 1])
    Nb2 = Xb2.shape[0]
    assert e.N_boundary == Nb2 and np.array_equal(e.X_boundary, Xb2) and np.array_equal(e.bdy_g, g)
    assert (e.boundary_coeffs is None) if rows is None else np.array_equal(e.boundary_coeffs, rows)
    e.Gram_matrix(kernel=kernel, kernel_parameter=list(kp), nugget=CLASS['nugget'], nugget_type='adaptive')
    e.Gram_Cholesky()
    assert e.chol_info == 0
    np.testing.assert_allclose(e.ratio, np.asarray(E.trace_ratios(kernel, kp, c, Nd, Nb2, rows), dtype=np.float64), rtol=4 * EPS)
    z0 = np.zeros(3 * Nd)
    e.GN_method(max_iter=steps, step_size=1, initial_sol=z0, print_hist=False)
    assert all(i == 0 for i in e.step_info) and len(e.loss_hist) == steps + 1
    # the reference iteration on the device's own Theta, factored by LAPACK
    L = np.linalg.cholesky(e.Theta)
    cs = E.Case(Nd, Nb2, f(Xd[:, 0], Xd[:, 1]), g, alpha, L)
    z_ref, hist = E.gn_float64(cs, z0, steps)
    z_dev = e._z_star[1]
    rel = float(np.linalg.norm(z_dev - z_ref) / np.linalg.norm(z_ref))
    print(f'\n[evo class] {equation[0]} {bc}: parity of the iterate {rel:.3g}; loss history {[float("%.6g" % v) for v in e.loss_hist]}, reference {hist[-1]:.9g}')
    assert rel <= 1e-6
    assert np.max(np.abs(e.sol_vec - E.sol_vec(cs, z_dev))) <= 1e-13 * np.max(np.abs(e.sol_vec))
    # error at 200 interior test points against the numpy pipeline's own
    Xt = np.random.RandomState(5).uniform([0.05, -0.95], [0.95, 0.95], (200, 2))
    ut = E.smooth_truth(Xt[:, 0], Xt[:, 1])
    coeff_ref = cho_solve((L, True), E.sol_vec(cs, z_ref))
    u_ref = E.rows(kernel, kp, c, 'value', Xt, Xd, Xb2, rows, np.float64) @ coeff_ref
    e.extend_sol(Xt)
    l2_dev, l2_ref = (float(np.sqrt(np.mean((v - ut) ** 2))) for v in (e.extended_sol, u_ref))
    print(f'[evo class] L2 error at the test points: device {l2_dev:.3g}, numpy pipeline {l2_ref:.3g}')
    assert l2_dev <= 2 * l2_ref
    # derivatives and residual
    d = e.extend_derivatives(Xt)
    assert tuple(d) == Evolution1d._deriv_names and np.array_equal(VA.bits(d['value']), VA.bits(e.extended_sol))
    res = e.PDE_residual(Xt)
    f_t = f(Xt[:, 0], Xt[:, 1])
    want = (d['d1'] + alpha * d['value'] * d['d2'] + d['q']) - f_t
    rms_r, rms_f = float(np.sqrt(np.mean(res ** 2))), float(np.sqrt(np.mean(f_t ** 2)))
    q_err = float(np.sqrt(np.mean((d['q'] - E.smooth_q(c)(Xt[:, 0], Xt[:, 1])) ** 2)))
    print(f'[evo class] residual RMS {rms_r:.3g} (RMS of f {rms_f:.3g}), RMS error of Q[u] {q_err:.3g}, max test error {np.max(np.abs(e.extended_sol - ut)):.3g}')
    assert np.all(np.isfinite(res))
    assert np.max(np.abs(res - want)) <= 64 * EPS * float(np.max(np.abs(d['d1']) + np.abs(d['value'] * d['d2']) + np.abs(d['q']) + np.abs(f_t)))
    # log evidence against the reference formula
    lz = e.log_evidence()
    want_lz = float(EV.terms_np64(cs, z_dev).value['log_Z'])
    print(f'[evo class] log evidence {lz:.12g}, reference {want_lz:.12g}, relative difference {abs(lz - want_lz) / abs(want_lz):.3g}')
    assert abs(lz - want_lz) <= 1e-8 * abs(want_lz)
    for call in (e.posterior_variance, e.posterior_covariance, e.posterior_sample):
        with pytest.raises(NotImplementedError):
            call(Xt)
    # the line search of the base class is honoured
    from src.linesearch import LineSearch
    e.line_search = LineSearch()
    e.GN_method(max_iter=3, step_size=1, initial_sol=z0, print_hist=False)
    print(f'[evo class] line search: steps {e.step_hist}, loss history {[float("%.6g" % v) for v in e.loss_hist]}')
    assert all(k >= 0 for k in e.ls_accepted) and e.loss_hist[-1] < e.loss_hist[0]
