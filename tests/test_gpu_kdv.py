"""The dispersive Gram layout (gpk_assemble_disp, gpk_extend_functionals_disp), the Burgers system on it and the class KdV on the device,
against tests/_kdv_reference.py.

  a. Gram, per block, against long double.  (N_d, N_b) = (1, 0), (1, 1), (2, 3), (33, 7); M = N_d + N_b = 31, 32, 33 around the 32 row points
     of a workgroup; M = 255, 256, 257 around the 256 column points of a workgroup of the one-point kernel (an odd count among N_d, N_b) and
     M = 510, 512, 514 around the 512 of the two-point kernel (both even).  Both kernels, coincident points.  Gate: the form of
     tests/test_gpu_gram_longdouble.py, per block |device - ref| <= (4e-15 + 4 e_np) max|block| with e_np the error of a float64 numpy
     evaluation of the reference's own formulas in the same block (_gauss_reference.gate_blocks): the project's Gram-block bound, about
     ten times what the evaluators of that file measure, and nothing taken from the evaluator under test.  Bitwise symmetric, bitwise
     repeatable; the store paths give the same bits.
  b. the three nugget types: diagonal and ratios.   c. views with an odd ld and a base offset by one double, between canaries.
  d. the extension: every subset of the five functionals at N_t = 1, 2, 3, 257 against reference rows @ coeff in long double, within
     64 eps (|rows| @ |coeff|) per test point (the form of tests/test_gpu_gram_longdouble.py, item f); a row has the same bits whichever
     other rows are requested; refusals.
  e. one gpk_gn_step on the factor of the device's own Theta, system Burgers with nu = -delta, against the long-double reference of
     tests/_gn_reference.py by its gates (32 x the float64 pipeline's own figure + 1), structured mode off, 1 and 2.
  f. the class KdV on a manufactured smooth solution with forcing.
Every test prints what it measures under a [kdv] tag.  RESULTS: DESIGN.md section K, "Dispersive equations: the third-order layout"."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import _gauss_reference as GR
import _gn_reference as R
import _kdv_reference as K
import _view_arena as VA

pytestmark = pytest.mark.gpu

LD, EPS = K.LD, K.EPS
PARAMS = {'Gaussian': 0.2, 'anisotropic_Gaussian': (0.3, 0.15)}
SMALL = ((1, 0), (1, 1), (2, 3), (33, 7))
ROW_TILE = ((25, 6), (26, 6), (27, 6))                       # M = 31, 32, 33: the 32 row points of a workgroup
COL_TILE_1 = ((200, 55), (201, 55), (201, 56))               # M = 255, 256, 257, an odd count: the one-point kernel, 256 columns per workgroup
COL_TILE_2 = ((400, 110), (400, 112), (400, 114))            # M = 510, 512, 514, all even: the two-point kernel, 512 columns per workgroup
NAMES5 = ('value', 'd1', 'd2', 'd2d2', 'd2d2d2')


@pytest.fixture(scope='module')
def ctx():
    import gpk
    c = gpk.Context(0)
    yield c
    c.close()


def gram_points(Nd, Nb):
    """uniform points on the unit square; where there is room a coincident domain pair and coincident domain / boundary points"""
    rng = np.random.RandomState(1000 * Nd + Nb)
    Xd, Xb = rng.uniform(0, 1, (Nd, 2)), rng.uniform(0, 1, (Nb, 2))
    if Nd > 6:
        Xd[6] = Xd[5]
    if Nb:
        Xb[Nb - 1] = Xd[Nd - 1]
    return Xd, Xb


@functools.lru_cache(maxsize=None)
def _reference(kernel, Nd, Nb):
    Xd, Xb = gram_points(Nd, Nb)
    return Xd, Xb, K.theta(kernel, PARAMS[kernel], Xd, Xb), K.theta(kernel, PARAMS[kernel], Xd, Xb, np.float64)


# ------------------------------------------------------------------------------------------------ a. Gram entries
GRAM_CASES = ([(k, s) for k in K.KERNELS for s in SMALL + ROW_TILE]
              + [(K.KERNELS[i % 2], s) for i, s in enumerate(COL_TILE_1 + COL_TILE_2)])


@pytest.mark.parametrize('kernel,size', GRAM_CASES, ids=lambda v: v if isinstance(v, str) else f'{v[0]}-{v[1]}')
def test_gram_blocks_against_long_double(ctx, kernel, size):
    Nd, Nb = size
    Xd, Xb, T, Tn = _reference(kernel, Nd, Nb)
    N = 4 * Nd + Nb
    dT, _ = ctx.assemble_disp(kernel, PARAMS[kernel], Xd, Xb)
    got = dT.download()
    dT.free()
    dT, _ = ctx.assemble_disp(kernel, PARAMS[kernel], Xd, Xb)
    again = dT.download()
    dT.free()
    assert got.shape == (N, N) and np.all(np.isfinite(got))
    assert np.array_equal(VA.bits(got), VA.bits(again)), 'not repeatable to the bit'
    assert np.array_equal(VA.bits(got), VA.bits(np.ascontiguousarray(got.T))), 'not symmetric to the bit'
    blocks = [b for b in K.offsets(Nd, Nb)]
    print()
    for i, (ro, rn) in enumerate(blocks):                      # every figure before the gate
        for j, (co, cn) in enumerate(blocks):
            r = T[ro:ro + rn, co:co + cn]
            scale = float(np.max(np.abs(r)))
            if scale > 0:
                e = float(np.max(np.abs(got[ro:ro + rn, co:co + cn].astype(LD) - r))) / scale
                en = float(np.max(np.abs(Tn[ro:ro + rn, co:co + cn].astype(LD) - r))) / scale
                print(f'[kdv gram] {kernel} ({Nd}, {Nb}) <{K.NAMES[i]},{K.NAMES[j]}>: device {e / EPS:.3g} eps, numpy {en / EPS:.3g} eps of max|block|')
    w = GR.gate_blocks(got, T, Tn, blocks, blocks, ('assemble_disp', kernel, Nd, Nb))
    print(f'[kdv gram] {kernel} ({Nd}, {Nb}): worst block device {w[0]:.3g} ({w[0] / EPS:.3g} eps), e_np {w[1]:.3g}, allowed {GR.BOUND + 4 * w[1]:.3g}')


@pytest.mark.parametrize('kernel', K.KERNELS)
def test_store_paths_give_the_same_bits(ctx, kernel):
    Nd, Nb = 64, 36
    Xd, Xb = gram_points(Nd, Nb)

    def run():
        T, _ = ctx.assemble_disp(kernel, PARAMS[kernel], Xd, Xb, 1e-6, 'adaptive')
        out = VA.bits(T.download())
        T.free()
        return out
    default = run()
    try:
        ctx.tune(55, 1)
        assert np.array_equal(run(), default), 'non-temporal 16-byte stores'
        ctx.tune(55, 0)
        ctx.tune(47, 0)
        assert np.array_equal(run(), default), '8-byte stores (key 47 = 0)'
    finally:
        ctx.tune(55, 0)
        ctx.tune(47, 1)
    assert np.array_equal(run(), default)


# ------------------------------------------------------------------------------------------------ b. nugget and ratios
@pytest.mark.parametrize('kernel', K.KERNELS)
def test_nugget_diagonal_and_ratios(ctx, kernel):
    kp = PARAMS[kernel]
    for Nd, Nb in ((33, 7), (26, 6), (1, 0)):
        Xd, Xb = gram_points(Nd, Nb)
        diag = K.diagonal_values(kernel, kp)
        want_r = np.asarray(K.trace_ratios(kernel, kp, Nd, Nb), dtype=np.float64)
        for nugget_type in ('none', 'identity', 'adaptive'):
            dT, ratios = ctx.assemble_disp(kernel, kp, Xd, Xb, 1e-6, nugget_type)
            full = dT.download()
            dT.free()
            got = np.diag(full).astype(LD)
            np.testing.assert_allclose(ratios, want_r, rtol=1e-14)             # written for every nugget type
            for (o, n), c, v in zip(K.offsets(Nd, Nb), diag, K.block_nuggets(kernel, kp, Nd, Nb, 1e-6, nugget_type)):
                want = c + v
                assert float(np.max(np.abs(got[o:o + n] - want)) / abs(want)) <= 4e-15, (nugget_type, (Nd, Nb), o)
            off = full - np.diag(np.diag(full))
            plain, _ = ctx.assemble_disp(kernel, kp, Xd, Xb)
            p = plain.download()
            plain.free()
            assert np.array_equal(VA.bits(off), VA.bits(p - np.diag(np.diag(p)))), 'the nugget touches the diagonal only'


# ------------------------------------------------------------------------------------------------ c. views
@pytest.mark.parametrize('cls,Nd,Nb', [('D', 33, 7), ('D', 26, 6), ('A', 26, 6), ('B', 26, 6), ('C', 2, 3)])
def test_views_between_canaries(ctx, cls, Nd, Nb):
    """class D: base offset by one double and odd ld; B / C: one of the two; A with ld > N: the 16-byte stores next to canaries"""
    import gpk
    kernel = 'anisotropic_Gaussian'
    kp = gpk.device.kernel_params(kernel, PARAMS[kernel])
    Xd, Xb = gram_points(Nd, Nb)
    N = 4 * Nd + Nb
    plain, _ = ctx.assemble_disp(kernel, PARAMS[kernel], Xd, Xb, 1e-6, 'adaptive')
    want = plain.download()
    plain.free()
    dXd, dXb = ctx.points(Xd), ctx.points(Xb)
    v = VA.class_view(ctx, N, N, cls, ld_min=N + 8)
    assert v.cls == cls and v.ld > N
    fn = ctx.lib.gpk_assemble_disp
    ctx._chk(fn(ctx.h, gpk.KERNEL[kernel], kp, dXd.ptr, Nd, dXb.ptr, Nb, 1e-6, gpk.NUGGET['adaptive'], v.ptr, v.ld, None))
    ctx.synchronize()
    v.arena.assert_outside_untouched([v])
    assert np.array_equal(VA.bits(v.arena.get(v)), VA.bits(want))
    # refusals write nothing
    assert fn(ctx.h, gpk.KERNEL[kernel], kp, dXd.ptr, Nd, dXb.ptr, Nb, 1e-6, gpk.NUGGET['adaptive'], v.ptr, N - 1, None) == -9001
    assert b'assemble_disp: ld < N' in ctx.lib.gpk_last_error(ctx.h)
    assert fn(ctx.h, gpk.KERNEL[kernel], kp, dXd.ptr, Nd, dXb.ptr, Nb, 1e-6, 7, v.ptr, v.ld, None) == -9001
    assert b'assemble_disp: nugget_type' in ctx.lib.gpk_last_error(ctx.h)
    assert fn(ctx.h, gpk.KERNEL[kernel], kp, dXd.ptr, 0, dXb.ptr, Nb, 1e-6, 0, v.ptr, v.ld, None) == -9001
    for kid in (8, 9, 10, 16, 2):                                       # the Matern ids, the periodic kernel, an unknown id
        assert fn(ctx.h, kid, (C.c_double * 4)(0.5, 0.5, 0.0, 1.0), dXd.ptr, Nd, dXb.ptr, Nb, 0.0, 0, v.ptr, v.ld, None) == -9001
        assert b'assemble_disp: kernel id' in ctx.lib.gpk_last_error(ctx.h)
    ctx.synchronize()
    v.arena.assert_outside_untouched([v])
    assert np.array_equal(VA.bits(v.arena.get(v)), VA.bits(want))
    v.arena.free()


# ------------------------------------------------------------------------------------------------ d. extension
MASKS = [tuple(n for n, on in zip(NAMES5, sel) if on) for sel in itertools.product((0, 1), repeat=5) if any(sel)]
EXT = (265, 41)                                                      # M = 306: the lanes' stride loop runs twice, the second time partly filled


@functools.lru_cache(maxsize=None)
def _extension_reference(kernel):
    Nd, Nb = EXT
    Xd, Xb = gram_points(Nd, Nb)
    N = 4 * Nd + Nb
    rng = np.random.RandomState(N)
    coeff = rng.normal(size=N)
    Xt = rng.uniform(0, 1, (257, 2))
    Xt[0], Xt[2], Xt[256] = Xd[3], Xb[2], Xd[Nd - 1]                   # collocation points among the test points
    want, allowed = {}, {}
    for name in NAMES5:
        rows = K.rows(kernel, PARAMS[kernel], name, Xt, Xd, Xb)
        want[name] = rows @ coeff.astype(LD)
        allowed[name] = 64 * LD(EPS) * (np.abs(rows) @ np.abs(coeff).astype(LD))
    return Xd, Xb, Xt, coeff, want, allowed


@pytest.mark.parametrize('Nt', (1, 2, 3, 257))
@pytest.mark.parametrize('kernel', K.KERNELS)
def test_extension_every_mask(ctx, kernel, Nt):
    kp = PARAMS[kernel]
    Xd, Xb, Xt_all, coeff, want, allowed = _extension_reference(kernel)
    Xt = Xt_all[:Nt]
    dc = ctx.array(coeff)
    single = {n: ctx.extend_functionals_disp(kernel, kp, Xt, Xd, Xb, dc, which=(n,)).download().reshape(Nt) for n in NAMES5}
    print()
    for n in NAMES5:
        ratio = float(np.max(np.abs(single[n].astype(LD) - want[n][:Nt]) / allowed[n][:Nt]))
        print(f'[kdv extend] {kernel} Nt {Nt} {n}: worst error {64 * ratio:.3g} eps of |rows| @ |coeff| (allowed 64)')
        assert np.all(np.isfinite(single[n])) and ratio <= 1.0, (n, Nt, ratio)
    for mask in MASKS:
        out = ctx.extend_functionals_disp(kernel, kp, Xt, Xd, Xb, dc, which=mask).download().reshape(len(mask), Nt)
        for k, n in enumerate(mask):
            assert np.array_equal(VA.bits(out[k]), VA.bits(single[n])), (mask, n, 'the bits of a row depend on the other rows')
    again = ctx.extend_functionals_disp(kernel, kp, Xt, Xd, Xb, dc, which=NAMES5).download().reshape(5, Nt)
    for k, n in enumerate(NAMES5):
        assert np.array_equal(VA.bits(again[k]), VA.bits(single[n])), 'not repeatable to the bit'
    pair = ctx.extend_functionals_disp(kernel, kp, Xt, Xd, Xb, dc, which=('d2d2d2', 'd1')).download().reshape(2, Nt)   # the caller's order
    assert np.array_equal(VA.bits(pair[0]), VA.bits(single['d2d2d2'])) and np.array_equal(VA.bits(pair[1]), VA.bits(single['d1']))


def test_extension_refusals_leave_out_untouched(ctx):
    import gpk
    Nd, Nb, Nt = 33, 7, 5
    Xd, Xb = gram_points(Nd, Nb)
    dXd, dXb, dXt = ctx.points(Xd), ctx.points(Xb), ctx.points(Xd[:Nt])
    coeff = ctx.array(np.ones(4 * Nd + Nb))
    out = ctx.empty(5, 8, ld=8)
    canary = np.full((5, 8), 3.25)
    out.upload(canary)
    kp = gpk.device.kernel_params('Gaussian', 0.2)
    fn = ctx.lib.gpk_extend_functionals_disp
    full = 1 | 2 | 4 | 8 | 64
    assert fn(ctx.h, 0, kp, dXt.ptr, Nt, dXd.ptr, Nd, dXb.ptr, Nb, coeff.ptr, full, out.ptr, Nt - 1) == -9001
    assert b'extend_functionals_disp: ldo < Nt' in ctx.lib.gpk_last_error(ctx.h)
    for mask in (0, -1, 16, 32, 128, 64 | 16, 1 | 32, 256 | 1):         # empty, negative, the Laplacian, d/dx3, bits above
        assert fn(ctx.h, 0, kp, dXt.ptr, Nt, dXd.ptr, Nd, dXb.ptr, Nb, coeff.ptr, mask, out.ptr, 8) == -9001, mask
        assert b'extend_functionals_disp: fmask' in ctx.lib.gpk_last_error(ctx.h)
    for kid in (8, 9, 10, 16, 2):                                       # Matern, periodic, unknown
        assert fn(ctx.h, kid, (C.c_double * 4)(0.5, 0.5, 0.0, 1.0), dXt.ptr, Nt, dXd.ptr, Nd, dXb.ptr, Nb, coeff.ptr, full, out.ptr, 8) == -9001
        assert b'extend_functionals_disp: kernel id' in ctx.lib.gpk_last_error(ctx.h)
    assert fn(ctx.h, 0, kp, dXt.ptr, 0, dXd.ptr, Nd, dXb.ptr, Nb, coeff.ptr, full, out.ptr, 8) == -9001
    assert fn(ctx.h, 0, kp, None, Nt, dXd.ptr, Nd, dXb.ptr, Nb, coeff.ptr, full, out.ptr, 8) == -9001
    # the calls that exist keep refusing the new bit
    o4 = ctx.empty(4, 8, ld=8)
    assert ctx.lib.gpk_extend_functionals(ctx.h, 1, 0, kp, dXt.ptr, Nt, dXd.ptr, Nd, dXb.ptr, Nb, coeff.ptr, 64, o4.ptr, 8) == -9001
    assert ctx.lib.gpk_extend_functionals(ctx.h, 1, 0, kp, dXt.ptr, Nt, dXd.ptr, Nd, dXb.ptr, Nb, coeff.ptr, 1 | 64, o4.ptr, 8) == -9001
    ctx.synchronize()
    assert np.array_equal(out.download(), canary)
    assert fn(ctx.h, 0, kp, dXt.ptr, Nt, dXd.ptr, Nd, dXb.ptr, Nb, coeff.ptr, 1 | 64, out.ptr, 8) == 0     # rows 0, 1; entries past Nt untouched
    ctx.synchronize()
    got = out.download()
    assert np.all(got[:2, :Nt] != 3.25) and np.array_equal(got[:2, Nt:], canary[:2, Nt:]) and np.array_equal(got[2:], canary[2:])


# ------------------------------------------------------------------------------------------------ e. one Gauss-Newton step
STEP = (65, 13)
STEP_KERNEL = ('Gaussian', 0.15)
STEP_PARAMS = (6.0, 1.0)                                              # alpha, delta


@pytest.fixture(scope='module')
def step_case(ctx):
    """the factor of the device's own Theta (gpk_assemble_disp + gpk_potrf), downloaded: the step is judged on exactly this factor"""
    Nd, Nb = STEP
    rng = np.random.RandomState(65)
    Xd, Xb = rng.uniform(0, 1, (Nd, 2)), rng.uniform(0, 1, (Nb, 2))
    dT, _ = ctx.assemble_disp(*STEP_KERNEL, Xd, Xb, 1e-6, 'adaptive')
    assert ctx.potrf(dT) == 0
    L = np.tril(dT.download())
    f, g = rng.uniform(0.5, 1.5, Nd), rng.uniform(0.5, 1.5, Nb)
    z0 = rng.uniform(0.3, 1.2, 3 * Nd) * rng.choice([-1.0, 1.0], 3 * Nd)
    cs = K.Case(Nd, Nb, f, g, *STEP_PARAMS, L, z0)
    return cs, dT, R.VectorReference(cs, z0)


@pytest.mark.parametrize('dinv,structured', [(256, False), (False, False), (256, 1), (256, 2)],
                         ids=['dinv', 'substitution', 'structured-1', 'structured-2'])
def test_step_against_the_reference(ctx, step_case, dinv, structured):
    import gpk
    cs, dL, ref = step_case
    prob = gpk.GNProblem(ctx, 'Burgers', cs.Nd, cs.Nb, cs.f, cs.g, dL, p0=cs.p0, p1=cs.p1, dinv=dinv, structured=structured)
    z = ctx.array(cs.z0)
    loss, info = ctx.gn_step(prob, z, 1.0)
    delta, z_out = prob.workspace()[2].download().copy(), z.download().copy()
    prob.free()
    print()
    bad = [] if info == 0 else [f'info = {info}']
    for name, (r, a) in (('loss', R.gate_loss(ref, loss)), ('backward', R.gate_backward_vec(ref, delta)), ('forward', R.gate_forward(ref, delta)),
                         ('update', R.gate_update(cs.z0, 1.0, delta, z_out))):
        print(f'[kdv step] dinv {dinv} structured {structured} {name}: device {r:.3g}, allowed {a:.3g}')
        if not r <= a:
            bad.append(f'{name}: {r:.4g} > {a:.4g}')
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ f. the class
CLASS = dict(Nd=300, Nb=100, kernel='anisotropic_Gaussian', kp=(0.6, 0.5), nugget=1e-6, steps=10)


def test_class_on_a_manufactured_solution():
    from scipy.linalg import cho_solve
    import _evidence_reference as E
    from src.PDEs import KdV
    Nd, Nb, kernel, kp, steps = CLASS['Nd'], CLASS['Nb'], CLASS['kernel'], CLASS['kp'], CLASS['steps']
    Xd, Xb = K.class_points(Nd, Nb)
    e = KdV(alpha=K.ALPHA, delta=K.DELTA, bdy=K.smooth_truth, rhs=K.smooth_rhs)
    e.get_sampled_points(Xd, Xb)
    e.Gram_matrix(kernel=kernel, kernel_parameter=list(kp), nugget=CLASS['nugget'], nugget_type='adaptive')
    e.Gram_Cholesky()
    assert e.chol_info == 0
    np.testing.assert_allclose(e.ratio, np.asarray(K.trace_ratios(kernel, kp, Nd, Nb), dtype=np.float64), rtol=1e-14)
    z0 = np.zeros(3 * Nd)
    e.GN_method(max_iter=steps, step_size=1, initial_sol=z0, print_hist=False)
    assert all(i == 0 for i in e.step_info) and len(e.loss_hist) == steps + 1
    # the reference iteration on the device's own Theta, factored by LAPACK
    L = np.linalg.cholesky(e.Theta)
    cs = K.Case(Nd, Nb, e.rhs_f, e.bdy_g, K.ALPHA, K.DELTA, L)
    z_ref, hist = K.gn_float64(cs, z0, steps)
    z_dev = e._z_star[1]
    rel = float(np.linalg.norm(z_dev - z_ref) / np.linalg.norm(z_ref))
    print(f'\n[kdv class] parity of the iterate {rel:.3g}; loss history {[float("%.6g" % v) for v in e.loss_hist]}, reference {hist[-1]:.9g}')
    assert rel <= 1e-6
    assert np.max(np.abs(e.sol_vec - K.sol_vec(cs, z_dev))) <= 1e-13 * np.max(np.abs(e.sol_vec))
    # error at 200 interior test points against the reference's own
    Xt = np.random.RandomState(5).uniform([0.05, -0.95], [0.95, 0.95], (200, 2))
    ut = K.smooth_truth(Xt[:, 0], Xt[:, 1])
    u_ref = K.rows(kernel, kp, 'value', Xt, Xd, Xb, np.float64) @ cho_solve((L, True), K.sol_vec(cs, z_ref))
    e.extend_sol(Xt)
    l2_dev, l2_ref = (float(np.sqrt(np.mean((v - ut) ** 2))) for v in (e.extended_sol, u_ref))
    print(f'[kdv class] L2 error at the test points: device {l2_dev:.3g}, reference {l2_ref:.3g}')
    assert l2_dev <= 2 * l2_ref
    # derivatives and residual
    d = e.extend_derivatives(Xt)
    assert tuple(d) == KdV._deriv_names and np.array_equal(VA.bits(d['value']), VA.bits(e.extended_sol))
    res = e.PDE_residual(Xt)
    f_t = K.smooth_rhs(Xt[:, 0], Xt[:, 1])
    want = (d['d1'] + K.ALPHA * d['value'] * d['d2'] + K.DELTA * d['d2d2d2']) - f_t
    rms_r, rms_f = float(np.sqrt(np.mean(res ** 2))), float(np.sqrt(np.mean(K.smooth_rhs(Xt[:, 0], Xt[:, 1]) ** 2)))
    print(f'[kdv class] residual RMS {rms_r:.3g} (RMS of f {rms_f:.3g}), max test error {np.max(np.abs(e.extended_sol - ut)):.3g}')
    assert np.all(np.isfinite(res))
    assert np.max(np.abs(res - want)) <= 64 * EPS * float(np.max(np.abs(d['d1']) + np.abs(d['value'] * d['d2']) + K.DELTA * np.abs(d['d2d2d2']) + np.abs(f_t)))
    # log evidence against the reference formula
    lz = e.log_evidence()
    want_lz = float(E.terms_np64(cs, z_dev).value['log_Z'])
    print(f'[kdv class] log evidence {lz:.12g}, reference {want_lz:.12g}, relative difference {abs(lz - want_lz) / abs(want_lz):.3g}')
    assert abs(lz - want_lz) <= 1e-8 * abs(want_lz)
    for call in (e.posterior_variance, e.posterior_covariance, e.posterior_sample):
        with pytest.raises(NotImplementedError):
            call(Xt)
    # the line search of the base class is honoured
    from src.linesearch import LineSearch
    e.line_search = LineSearch()
    e.GN_method(max_iter=3, step_size=1, initial_sol=z0, print_hist=False)
    print(f'[kdv class] line search: steps {e.step_hist}, loss history {[float("%.6g" % v) for v in e.loss_hist]}')
    assert all(k >= 0 for k in e.ls_accepted) and e.loss_hist[-1] < e.loss_hist[0]
