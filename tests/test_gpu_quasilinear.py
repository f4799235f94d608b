"""The 2-jet Gram layout (gpk_assemble_jet2, gpk_extend_functionals_jet2), the system GPK_GN_QUASILINEAR, gpk_pde_residual_ql and the class
Quasilinear2d on the device, against tests/_quasilinear_reference.py.

  a. Gram entries at _gauss_reference.SIZES = (64, 36) (16-byte stores), (65, 41) (8-byte stores) and LARGE = (530, 46) (more than one
     workgroup along the columns, N = 3226), both kernels, with coincident points and pairs at a root of h_2: per entry
     |device - ref| <= (4e-15 + 4 eps arg) x magnitude sum (gram_allowed), per block.  Symmetric to the bit; 16-byte, non-temporal and
     8-byte store paths give the same bits; an unaligned view between canaries is written inside N x N only; the five ratios and the
     nugget on the right diagonals for the three nugget types; Matern and periodic ids refused.
  b. extension rows against long-double rows @ coeff, bound 64 eps + 4 eps arg of the magnitude sums @ |coeff| (the sibling's bound,
     tests/test_gpu_monge_ampere.py), N_t in {1, 2, 67, 514, 515}; repeatable to the bit, a row's bits independent of the mask.
  c. gpk_gn_build / gpk_gn_build_rev entry by entry per kind (exact pattern, values within C_BUILD eps of their magnitude sums), one step
     per kind on synthetic factors judged by the float64 pipeline x MARGIN = 32 (substitution path and inverted blocks, leading-zero
     schedule on and off), the linear case m = 2, the line search's accepted point, the refusals.
  d. the residual entry.   e. Quasilinear2d end to end per kind, log evidence, the driver.
Every test prints what it measures under a [quasilinear] tag.

RESULTS (MI355X): see the docstrings of the tests and DESIGN.md section K, "Quasilinear equations: the 2-jet layout"."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import _gauss_reference as GR
import _quasilinear_reference as Q
import _view_arena as VA

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'nonlinpdes-gpsolver_amd')
if PKG not in sys.path:
    sys.path.insert(0, PKG)

LD, EPS = Q.LD, Q.EPS
PARAMS = GR.PARAMS                                 # ('Gaussian', 0.2), ('anisotropic_Gaussian', (0.3, 0.05))
SIZES = GR.SIZES                                   # (64, 36): the two-point kernel; (65, 41): the one-point kernel
LARGE = (530, 46)                                  # M = 576 > 512: more than one workgroup along the columns in both kernels
NAMES6 = ('value', 'd1', 'd2', 'd11', 'd12', 'd22')
KINDS = tuple(Q.KINDS)


@pytest.fixture(scope='module')
def ctx():
    import gpk
    c = gpk.Context(0)
    yield c
    c.close()


def gram_points(kernel, Nd, Nb):
    """uniform points with a coincident domain / boundary pair, a coincident domain pair, and two domain pairs at a root of h_2 on one
    axis (p d^2 = 1) and distance 0 on the other (the points of tests/test_gpu_monge_ampere.py)"""
    rng = np.random.RandomState(1000 * Nd + Nb)
    Xd, Xb = rng.uniform(0, 1, (Nd, 2)), rng.uniform(0, 1, (Nb, 2))
    p1, p2 = (float(v) for v in GR.precisions(kernel, PARAMS[kernel]))
    Xd[3] = (0.3, 0.4); Xd[2] = (0.3 + 1.0 / np.sqrt(p1), 0.4); Xd[4] = (0.3, 0.4 + 1.0 / np.sqrt(p2))
    Xd[6] = Xd[5]
    Xb[0] = Xd[1]; Xb[Nb - 1] = Xd[Nd - 1]
    return Xd, Xb


@functools.lru_cache(maxsize=None)
def _reference(kernel, Nd, Nb):
    Xd, Xb = gram_points(kernel, Nd, Nb)
    return (Xd, Xb) + Q.theta(kernel, PARAMS[kernel], Xd, Xb)


# ------------------------------------------------------------------------------------------------ a. Gram entries
@pytest.mark.parametrize('kernel', Q.KERNELS)
@pytest.mark.parametrize('Nd,Nb', SIZES + (LARGE,))
def test_gram_entries_against_long_double(ctx, kernel, Nd, Nb):
    """RESULTS (MI355X): worst ratio to the per-entry bound, Gaussian / anisotropic: (64, 36) 0.211 / 0.345, (65, 41) 0.214 / 0.263,
    (530, 46) 0.252 / 0.325."""
    Xd, Xb, T, mag, arg = _reference(kernel, Nd, Nb)
    N = 6 * Nd + Nb
    dT, ratios = ctx.assemble_jet2(kernel, PARAMS[kernel], Xd, Xb)
    got = dT.download()
    dT.free()
    assert got.shape == (N, N) and np.all(np.isfinite(got))
    assert np.array_equal(VA.bits(got), VA.bits(got.T.copy())), 'Theta is not symmetric to the bit'
    blocks = Q.offsets(Nd, Nb)
    err = np.abs(got.astype(LD) - T)
    allowed = Q.gram_allowed(mag, arg)
    print()
    worst = 0.0
    for i, (ro, rn) in enumerate(blocks):
        for j, (co, cn) in enumerate(blocks):
            e, a, m = err[ro:ro + rn, co:co + cn], allowed[ro:ro + rn, co:co + cn], mag[ro:ro + rn, co:co + cn]
            r = float(np.max(np.where(a > 0, e / np.where(a > 0, a, 1), np.where(e > 0, np.inf, 0))))
            u = float(np.max(np.where(m > 0, e / np.where(m > 0, m, 1), 0))) / EPS
            print(f'[quasilinear gram] {kernel} ({Nd}, {Nb}) <{Q.NAMES[i]},{Q.NAMES[j]}>: worst error {u:.3g} eps of the magnitude sum, '
                  f'{r:.3g} of the bound')
            worst = max(worst, r)
    print(f'[quasilinear gram] {kernel} ({Nd}, {Nb}): worst ratio to the per-entry bound {worst:.3g}')
    assert worst <= 1.0
    # the special pairs are in the set: a root of h_2 and coincident points
    assert abs(float(T[3 * Nd + 2, 3 * Nd + 3])) <= 1e-12 * float(mag[3 * Nd + 2, 3 * Nd + 3]) and float(arg[5, 6]) == 0.0


@pytest.mark.parametrize('kernel', Q.KERNELS)
def test_hessian_blocks_are_the_hessian_layout(ctx, kernel):
    """blocks 2..5 against gpk_assemble_hess on the same points, to the Gram bound (they are spelled alike: in fact the same bits)"""
    Nd, Nb = SIZES[0]
    Xd, Xb, T, mag, arg = _reference(kernel, Nd, Nb)
    dT, _ = ctx.assemble_jet2(kernel, PARAMS[kernel], Xd, Xb, 1e-6, 'adaptive')
    dH, _ = ctx.assemble_hess(kernel, PARAMS[kernel], Xd, Xb, 1e-6, 'adaptive')
    got, hess = dT.download()[2 * Nd:, 2 * Nd:], dH.download()
    dT.free(); dH.free()
    a = Q.gram_allowed(mag, arg)[2 * Nd:, 2 * Nd:].astype(np.float64)
    off = ~np.eye(got.shape[0], dtype=bool)                              # (the nugget: other ratios on the diagonal, block 5 against block 3)
    diff = np.abs(got - hess)
    print(f'\n[quasilinear gram] {kernel}: blocks 2..5 against assemble_hess: max |difference| / bound {np.max(diff[off] / np.maximum(a[off], 1e-300)):.3g}, '
          f'bit-identical off the diagonal: {np.array_equal(got[off], hess[off])}')
    assert np.all(diff[off] <= 2 * a[off])
    assert np.all(np.abs(np.diag(got) - np.diag(hess)) <= 2e-6 * np.abs(np.diag(hess)))


@pytest.mark.parametrize('kernel', Q.KERNELS)
def test_store_paths_give_the_same_bits(ctx, kernel):
    Nd, Nb = SIZES[0]
    Xd, Xb = gram_points(kernel, Nd, Nb)

    def run():
        T, _ = ctx.assemble_jet2(kernel, PARAMS[kernel], Xd, Xb, 1e-6, 'adaptive')
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


@pytest.mark.parametrize('cls,Nd,Nb', [('D', 65, 41), ('D', 64, 36), ('A', 64, 36)])
def test_views_between_canaries(ctx, cls, Nd, Nb):
    """class D: odd base offset and odd ld (8-byte stores); class A with ld > N: the 16-byte stores next to canaries"""
    import gpk
    kernel = 'anisotropic_Gaussian'
    Xd, Xb = gram_points(kernel, Nd, Nb)
    N = 6 * Nd + Nb
    plain, _ = ctx.assemble_jet2(kernel, PARAMS[kernel], Xd, Xb, 1e-6, 'adaptive')
    want = plain.download()
    plain.free()
    dXd, dXb = ctx.points(Xd), ctx.points(Xb)
    v = VA.class_view(ctx, N, N, cls, ld_min=N + 8)
    assert v.cls == cls and v.ld > N and (cls != 'D' or v.ld % 2 == 1)
    kp = gpk.device.kernel_params(kernel, PARAMS[kernel])
    fn = ctx.lib.gpk_assemble_jet2
    ctx._chk(fn(ctx.h, gpk.KERNEL[kernel], kp, dXd.ptr, Nd, dXb.ptr, Nb, 1e-6, gpk.NUGGET['adaptive'], v.ptr, v.ld, None))
    ctx.synchronize()
    v.arena.assert_outside_untouched([v])
    assert np.array_equal(VA.bits(v.arena.get(v)), VA.bits(want))
    # ld < N, the Matern ids and the periodic id are refused (-9001, named) and nothing is written
    assert fn(ctx.h, gpk.KERNEL[kernel], kp, dXd.ptr, Nd, dXb.ptr, Nb, 1e-6, gpk.NUGGET['adaptive'], v.ptr, N - 1, None) == -9001
    assert b'assemble_jet2: ld < N' in ctx.lib.gpk_last_error(ctx.h)
    for kid in (8, 9, 10, 16):
        assert fn(ctx.h, kid, (C.c_double * 4)(0.5, 0.5, 1.0, 1.0), dXd.ptr, Nd, dXb.ptr, Nb, 0.0, 0, v.ptr, v.ld, None) == -9001
        assert b'assemble_jet2: kernel id' in ctx.lib.gpk_last_error(ctx.h)
    ctx.synchronize()
    v.arena.assert_outside_untouched([v])
    assert np.array_equal(VA.bits(v.arena.get(v)), VA.bits(want))
    v.arena.free()


@pytest.mark.parametrize('kernel', Q.KERNELS)
def test_nugget_diagonal_and_ratios(ctx, kernel):
    kp = PARAMS[kernel]
    for Nd, Nb in SIZES:
        Xd, Xb = gram_points(kernel, Nd, Nb)
        diag = Q.diagonal_values(kernel, kp)
        want_r = np.asarray(Q.trace_ratios(kernel, kp, Nd, Nb), dtype=np.float64)
        for nugget_type in ('none', 'identity', 'adaptive'):
            dT, ratios = ctx.assemble_jet2(kernel, kp, Xd, Xb, 1e-6, nugget_type)
            got = np.diag(dT.download()).astype(LD)
            dT.free()
            assert len(ratios) == 5
            np.testing.assert_allclose(ratios, want_r, rtol=1e-14)
            for (o, n), c, v in zip(Q.offsets(Nd, Nb), diag, Q.block_nuggets(kernel, kp, Nd, Nb, 1e-6, nugget_type)):
                want = c + v
                err = float(np.max(np.abs(got[o:o + n] - want)) / abs(want))
                assert err <= 4e-15, (nugget_type, (Nd, Nb), o, err)


# ------------------------------------------------------------------------------------------------ b. extension
@pytest.mark.parametrize('kernel', Q.KERNELS)
@pytest.mark.parametrize('Nd,Nb', [SIZES[1], (265, 41)])                # the lanes' stride loop runs once, partly filled / twice (M = 306)
def test_extension_rows(ctx, kernel, Nd, Nb):
    kp = PARAMS[kernel]
    Xd, Xb = gram_points(kernel, Nd, Nb)
    N = 6 * Nd + Nb
    rng = np.random.RandomState(N)
    coeff = rng.normal(size=N)
    Xt_all = rng.uniform(0, 1, (515, 2))
    Xt_all[0], Xt_all[1], Xt_all[66] = Xd[3], Xb[2], Xd[Nd - 1]          # collocation points among the test points
    refs = {name: Q.monomial_rows(kernel, kp, name, Xt_all, Xd, Xb) for name in NAMES6}
    print()
    for Nt in (1, 2, 67, 514, 515):                                      # ragged groups of 4; odd and even; more than one workgroup
        Xt = Xt_all[:Nt]
        full = ctx.extend_functionals_jet2(kernel, kp, Xt, Xd, Xb, coeff).download().reshape(6, Nt)
        again = ctx.extend_functionals_jet2(kernel, kp, Xt, Xd, Xb, coeff).download().reshape(6, Nt)
        assert np.array_equal(VA.bits(full), VA.bits(again)) and np.all(np.isfinite(full))
        for k, name in enumerate(NAMES6):
            rows, mag, arg = (a[:Nt] for a in refs[name])
            want = rows @ coeff.astype(LD)
            allowed = ((64 * LD(EPS) + 4 * LD(EPS) * arg) * mag) @ np.abs(coeff).astype(LD)
            ratio = float(np.max(np.abs(full[k].astype(LD) - want) / allowed))
            if Nt in (67, 515):
                single = ctx.extend_functionals_jet2(kernel, kp, Xt, Xd, Xb, coeff, which=(name,)).download().reshape(Nt)
                assert np.array_equal(VA.bits(single), VA.bits(full[k])), (name, 'the bits of a row depend on the mask')
            print(f'[quasilinear extend] {kernel} ({Nd}, {Nb}) Nt {Nt} {name}: worst error / bound {ratio:.3g} '
                  f'(bound: 64 eps + 4 eps arg of the magnitude sums @ |coeff|)')
            assert ratio <= 1.0, (name, Nt)
        if Nt == 67:
            pair = ctx.extend_functionals_jet2(kernel, kp, Xt, Xd, Xb, coeff, which=('d22', 'd1')).download().reshape(2, Nt)
            assert np.array_equal(VA.bits(pair[0]), VA.bits(full[5])) and np.array_equal(VA.bits(pair[1]), VA.bits(full[1]))


def test_extension_refusals_leave_out_untouched(ctx):
    import gpk
    Nd, Nb, Nt = 33, 11, 5
    Xd, Xb = gram_points('Gaussian', Nd, Nb)
    dXd, dXb, dXt = ctx.points(Xd), ctx.points(Xb), ctx.points(Xd[:Nt])
    coeff = ctx.array(np.ones(6 * Nd + Nb))
    out = ctx.empty(6, 8, ld=8)
    canary = np.full((6, 8), 3.25)
    out.upload(canary)
    kp = gpk.device.kernel_params('Gaussian', 0.2)
    fn = ctx.lib.gpk_extend_functionals_jet2
    assert fn(ctx.h, 0, kp, dXt.ptr, Nt, dXd.ptr, Nd, dXb.ptr, Nb, coeff.ptr, 63, out.ptr, Nt - 1) == -9001
    assert b'extend_functionals_jet2: ldo < Nt' in ctx.lib.gpk_last_error(ctx.h)
    for mask in (0, 64, -1):
        assert fn(ctx.h, 0, kp, dXt.ptr, Nt, dXd.ptr, Nd, dXb.ptr, Nb, coeff.ptr, mask, out.ptr, 8) == -9001
        assert b'fmask' in ctx.lib.gpk_last_error(ctx.h)
    for kid in (8, 9, 10, 16, 2):
        assert fn(ctx.h, kid, (C.c_double * 4)(0.5, 0.5, 1.0, 1.0), dXt.ptr, Nt, dXd.ptr, Nd, dXb.ptr, Nb, coeff.ptr, 63, out.ptr, 8) == -9001
    ctx.synchronize()
    assert np.array_equal(out.download(), canary)
    assert fn(ctx.h, 0, kp, dXt.ptr, Nt, dXd.ptr, Nd, dXb.ptr, Nb, coeff.ptr, 1 | 8, out.ptr, 8) == 0     # rows 0, 1; entries past Nt untouched
    ctx.synchronize()
    got = out.download()
    assert np.all(got[:2, :Nt] != 3.25) and np.array_equal(got[:2, Nt:], canary[:2, Nt:]) and np.array_equal(got[2:], canary[2:])


# ------------------------------------------------------------------------------------------------ c. the system
def _upload_factor(ctx, L):
    n = L.shape[0]
    d = ctx.empty(n, n + Q.R.LD_PAD, ld=n + Q.R.LD_PAD)
    d.upload(Q.poisoned(L))
    d.cols = n
    return d


def _problem(ctx, cs, dinv=256):
    import gpk
    L = _upload_factor(ctx, cs.L)
    prob = gpk.GNProblem(ctx, 'Quasilinear2d', cs.Nd, cs.Nb, cs.f, cs.g, L, dinv=dinv, p0=cs.prm[0], p1=cs.prm[1], p2=cs.prm[2], nonlin=cs.kind)
    prob.keep.append(L)
    return prob


def _first_nonzero_rows(A):
    nzm = A != 0
    return np.where(nzm.any(axis=0), nzm.argmax(axis=0), A.shape[0])


BUILD = (37, 11)


@pytest.mark.parametrize('kind', KINDS)
def test_build_values_and_canaries(ctx, kind):
    Nd, Nb = BUILD
    cs = Q.case(kind, Nd, Nb)
    lin = Q.linearise(cs, cs.z0)
    prob = _problem(ctx, cs, dinv=False)
    z = ctx.array(cs.z0)
    nz, rows = cs.nz, cs.rows
    assert (prob.nz, prob.rows) == (nz, rows) == (5 * Nd, 6 * Nd + Nb) and prob.struct.nonlin == Q.KINDS[kind]
    r0, c0, ld = 2, 3, nz + 1 + 9                                          # an unaligned view inside a larger buffer
    col = Q.stair_col(Nd)
    print()
    for name, fn in (('gpk_gn_build', ctx.lib.gpk_gn_build), ('gpk_gn_build_rev', ctx.lib.gpk_gn_build_rev)):
        buf = ctx.empty(rows + 4, ld, ld=ld)
        canary = np.full((rows + 4, ld), 3.25)
        buf.upload(canary)
        ctx._chk(fn(ctx.h, C.byref(prob.struct), z.ptr, buf.at(r0, c0), ld))
        ctx.synchronize()
        got = buf.download()
        view = got[r0:r0 + rows, c0:c0 + nz + 1].copy()
        inside = np.zeros_like(got, dtype=bool)                            # (the S buffer is cleared as rows of lds doubles)
        inside.reshape(-1)[r0 * ld + c0:r0 * ld + c0 + rows * ld] = True
        assert np.array_equal(got[~inside], canary[~inside]), f'{name} wrote outside its S buffer'
        A = view[:, :nz] if name == 'gpk_gn_build' else view[:, col]
        worst = Q.check_build(lin, A, view[:, nz], (name, kind))
        print(f'[quasilinear build] {kind} {name}: worst |dev - ld| / (eps sum|terms|) = {worst:.2f} of {Q.C_BUILD}')
        if name == 'gpk_gn_build_rev':                                     # the promised leading zeros: column c has nothing above row n_z - 1 - c
            first = _first_nonzero_rows(view[:, :nz])
            assert np.all(first >= nz - 1 - np.arange(nz))
            if kind == 'mean_curvature':                                   # dG/dv0 != 0: attained in every column
                assert np.array_equal(first, nz - 1 - np.arange(nz))
        buf.free()
    assert Q.check_build(lin, lin.dense(np.float64), ctx.gn_measurement(prob, z), ('gpk_gn_measurement', kind)) <= Q.C_BUILD
    prob.free()


def _report(tag, res):
    bad = []
    for name, (r, a) in res.items():
        print(f'[quasilinear {tag}] {name}: device {r / EPS:.3g} eps, allowed {a / EPS:.3g} eps, ratio to the bound {r / a:.3g}')
        if not r <= a:
            bad.append((name, r, a))
    return bad


STEP = (150, 40)


def _one_step(ctx, cs, dinv):
    prob = _problem(ctx, cs, dinv)
    z = ctx.array(cs.z0)
    H, g = ctx.gn_hessian_grad(prob, z)
    loss = ctx.gn_loss(prob, z)
    step_loss, info = ctx.gn_step(prob, z, 1.0)
    delta, z_out = prob.workspace()[2].download().copy(), z.download().copy()
    prob.free()
    return H, g, loss, step_loss, info, delta, z_out


@pytest.mark.parametrize('dinv', [False, 256])
@pytest.mark.parametrize('kind', KINDS)
def test_step_hessian_grad_loss(ctx, kind, dinv):
    """one gpk_gn_step on the synthetic well-conditioned factor against the long-double step, judged by what the float64 numpy pipeline
    takes on the same inputs x MARGIN = 32; with the leading-zero schedule on (layout 6, the closed-form profile) and off (dense).
    RESULTS (MI355X): worst ratio to the bound over the three kinds, both solve paths and both schedules: H 0.066, g 0.082, loss 0.034,
    delta 0.079, z 0.079 (cond(H) about 3.4); the build entries within 1.6 eps of their magnitude sums (C_BUILD 20)."""
    cs, ref = Q.case(kind, *STEP), Q.full_reference(kind, *STEP)
    H, g, loss, step_loss, info, delta, z_out = _one_step(ctx, cs, dinv)
    print(f'\n[quasilinear step] {kind} dinv {dinv}: cond(H) {ref.cond:.3g}')
    assert info == 0 and np.array_equal(H, H.T)
    bad = _report(f'step {kind} dinv {dinv}', Q.gates(ref, H=H, g=g, loss=loss, delta=delta, z_out=z_out))
    bad += _report(f'step {kind} dinv {dinv} in-step', Q.gates(ref, loss=step_loss))
    try:
        ctx.tune(23, 0)                                                    # the dense schedule
        _, _, _, step_loss0, info0, delta0, z_out0 = _one_step(ctx, cs, dinv)
    finally:
        ctx.tune(23, 1)
    assert info0 == 0
    bad += _report(f'step {kind} dinv {dinv} dense schedule', Q.gates(ref, loss=step_loss0, delta=delta0, z_out=z_out0))
    assert not bad, bad


def test_linear_case_reaches_its_solution_in_one_step(ctx):
    """m = 2: Poisson's equation, F is affine in z, so one step from zero is the minimiser and a second one moves nothing.
    RESULTS (MI355X): first step at 0.047 of its gate; second step max |delta| / max |z| = 3.4e-15 at cond(H) 3.4 (allowed 32 cond eps)."""
    cs = Q.Case('p_laplace', *STEP, prm=(2.0, 0.8, 0.0), z0=np.zeros(5 * STEP[0]))
    ref = Q.FullReference(cs, cs.z0)
    prob = _problem(ctx, cs, 256)
    z = ctx.array(cs.z0)
    loss, info = ctx.gn_step(prob, z, 1.0)
    delta, z1 = prob.workspace()[2].download().copy(), z.download().copy()
    print()
    bad = _report('linear case', Q.gates(ref, loss=loss, delta=delta, z_out=z1))
    _, pred, info2 = ctx.gn_direction(prob, z)
    d2 = prob.workspace()[2].download()
    scale = float(np.max(np.abs(z1)))
    print(f'[quasilinear linear case] second step max |delta| / max |z| = {np.max(np.abs(d2)) / scale:.3g}, cond(H) {ref.cond:.3g}')
    prob.free()
    assert info == 0 and info2 == 0 and not bad, bad
    assert np.max(np.abs(d2)) <= Q.MARGIN * ref.cond * EPS * scale        # z1 solves the normal equations to cond(H) eps


@pytest.mark.parametrize('kind', KINDS)
def test_line_search_accepts_the_measured_point(dev_ctx, kind):
    ctx, cs = dev_ctx, Q.case(kind, *BUILD)
    prob = _problem(ctx, cs, 256)
    z, zin = ctx.array(cs.z0), ctx.array(cs.z0)
    loss0 = ctx.gn_loss(prob, z)
    loss, info, k, t_acc, trial = ctx.gn_step_ls(prob, z, trials=8, t0=7.0, shrink=0.3, c1=1e-4)
    t = np.empty(8); t[0] = 7.0                                            # t_k = t0 beta^k by repeated multiplication, as the library forms them
    for i in range(1, 8):
        t[i] = t[i - 1] * 0.3
    print(f'\n[quasilinear line search] {kind}: k = {k}, t = {t_acc}, loss {loss0:.6g} -> {ctx.gn_loss(prob, z):.6g}, trial losses {trial}')
    assert info == 0 and k >= 0 and t_acc == t[k] and abs(loss - loss0) <= 1e-12 * loss0
    assert np.isfinite(trial[k]) and trial[k] < loss0
    delta = prob.workspace()[2]
    W = ctx.empty(prob.rows, 8, ld=8)
    ctx._chk(ctx.lib.gpk_debug_gn_trial_build(ctx.h, C.byref(prob.struct), zin.ptr, delta.ptr, t.ctypes.data_as(C.POINTER(C.c_double)), 8, W.ptr, 8))
    assert np.array_equal(W.download()[:, k], ctx.gn_measurement(prob, z)), 'the accepted iterate is not the point whose loss was measured'
    prob.free()


def test_refusals(ctx):
    import gpk
    cs = Q.case('p_laplace', *BUILD)
    prob = _problem(ctx, cs, 256)
    S, Hb, delta, work = prob.workspace()
    err = lambda: ctx.lib.gpk_last_error(ctx.h)
    W1, W2, v0 = ctx.empty(prob.rows, S.ld, ld=S.ld), ctx.empty(prob.rows, S.ld, ld=S.ld), ctx.empty(prob.rows)
    assert ctx.lib.gpk_gn_structured_prepare(ctx.h, C.byref(prob.struct), S.ptr, S.ld, W1.ptr, W2.ptr, v0.ptr, S.ld) == -9001
    assert b'GPK_GN_QUASILINEAR' in err()
    G, pvec = ctx.empty(4 * prob.nz, prob.nz), ctx.empty(2 * prob.nz + 1)
    prob.struct.W1, prob.struct.W2, prob.struct.ldw = W1.ptr, W2.ptr, S.ld
    assert ctx.lib.gpk_gn_gram_prepare(ctx.h, C.byref(prob.struct), G.ptr, G.ld, pvec.ptr) == -9001 and b'GPK_GN_QUASILINEAR' in err()
    prob.struct.W1 = prob.struct.W2 = None
    z = ctx.array(cs.z0)
    loss = C.c_double()
    canary = np.full(prob.rows, 3.25)
    work.upload(canary)
    good = (prob.struct.nonlin, prob.struct.p0, prob.struct.p1, prob.struct.p2)
    for nonlin, p0, p1, p2 in ((3, 3.0, 0.8, 0.0), (-1, 3.0, 0.8, 0.0), (1, float('nan'), 0.8, 0.0), (1, 3.0, float('inf'), 0.0),
                               (1, 3.0, 0.8, float('nan')), (1, 3.0, 0.0, 0.0), (1, 3.0, -0.5, 0.0), (1, 0.0, 0.8, 0.0), (1, -2.0, 0.8, 0.0),
                               (0, float('nan'), 0.0, 0.0), (2, float('inf'), 0.0, 0.0)):
        prob.struct.nonlin, prob.struct.p0, prob.struct.p1, prob.struct.p2 = nonlin, p0, p1, p2
        assert ctx.lib.gpk_gn_loss(ctx.h, C.byref(prob.struct), z.ptr, work.ptr, C.byref(loss)) == -9001, (nonlin, p0, p1, p2)
        assert b'GPK_GN_QUASILINEAR' in err()
        assert ctx.lib.gpk_gn_build(ctx.h, C.byref(prob.struct), z.ptr, S.ptr, S.ld) == -9001
    ctx.synchronize()
    assert np.array_equal(work.download(), canary), 'a refused call launched something'
    prob.struct.nonlin, prob.struct.p0, prob.struct.p1, prob.struct.p2 = good
    assert ctx.lib.gpk_gn_loss(ctx.h, C.byref(prob.struct), z.ptr, work.ptr, C.byref(loss)) == 0 and np.isfinite(loss.value)
    # the other systems keep "nonlin = 0 only", and the residual entry refuses what the system refuses
    L = prob.L
    sl = gpk.GNProblem(ctx, 'MongeAmpere2d', 10, 4, np.ones(10), np.ones(4), L, dinv=False)
    sl.struct.nonlin = 2
    assert ctx.lib.gpk_gn_loss(ctx.h, C.byref(sl.struct), z.ptr, work.ptr, C.byref(loss)) == -9001 and b'GPK_GN_MONGE_AMPERE' in err()
    with pytest.raises(ValueError):
        ctx.assemble_jet2('Matern52', 0.3, np.zeros((4, 2)), np.zeros((2, 2)))
    prob.free()


# ------------------------------------------------------------------------------------------------ d. the residual entry
@pytest.mark.parametrize('kind', KINDS)
def test_residual_entry(ctx, kind):
    rng = np.random.RandomState(9)
    Nt = 300
    fields, f = rng.normal(size=(6, Nt)), rng.uniform(0.5, 2, Nt)
    prm = Q.PRM[kind]
    want, mag = Q.divergence_form(kind, tuple(LD(v) for v in prm), f.astype(LD), *(r.astype(LD) for r in fields))
    a = ctx.pde_residual_ql(kind, prm, fields, f).download().ravel()
    b = ctx.pde_residual_ql(Q.KINDS[kind], prm, fields, f).download().ravel()
    assert np.array_equal(VA.bits(a), VA.bits(b))
    ratio = float(np.max(np.abs(a.astype(LD) - want) / (LD(EPS) * mag)))
    # the longest chain (p-Laplacian): g2 (2), s (1), pow (2 ulp of the library + the exponent's share: 3), T (5), lap, s lap, +, *, - f:
    # under 32 half-roundings of magnitudes that are at most the sum
    print(f'\n[quasilinear residual] {kind}: worst |device - long double| = {ratio:.3g} eps of the magnitude sum (allowed 16)')
    assert ratio <= 16.0
    du, dr, out = ctx.array(fields), ctx.array(f), ctx.empty(Nt)
    fn = ctx.lib.gpk_pde_residual_ql
    p3 = (C.c_double * 3)(*prm)
    assert fn(ctx.h, Q.KINDS[kind], p3, 0, du.ptr, du.ld, dr.ptr, out.ptr) == -9001 and b'pde_residual_ql: Nt <= 0' in ctx.lib.gpk_last_error(ctx.h)
    assert fn(ctx.h, Q.KINDS[kind], p3, Nt, du.ptr, Nt - 1, dr.ptr, out.ptr) == -9001
    assert fn(ctx.h, 3, p3, Nt, du.ptr, du.ld, dr.ptr, out.ptr) == -9001 and b'GPK_GN_QUASILINEAR' in ctx.lib.gpk_last_error(ctx.h)
    for args in ((None, du.ld, dr.ptr, out.ptr), (du.ptr, du.ld, None, out.ptr), (du.ptr, du.ld, dr.ptr, None)):
        assert fn(ctx.h, Q.KINDS[kind], p3, Nt, *args) == -9001


# ------------------------------------------------------------------------------------------------ e. end to end through the class
ND, NB, SIGMA, NUGGET_E2E, STEPS, AMPLITUDE = 150, 40, 0.3, 1e-8, 8, 0.5      # the configuration of tests/golden/gen/make_quasilinear.py
# what the float64 numpy pipeline reaches on this configuration (CPU, measured before the device ran): L2 error at the collocation points
NUMPY_L2 = {'mean_curvature': 1.89e-06, 'p_laplace': 4.07e-06, 'gauss_curvature': 1.15e-05}


@functools.lru_cache(maxsize=None)
def _solved(kind):
    import main_Quasilinear2d as drv
    from src.PDEs import Quasilinear2d
    args = Q.PRM[kind][:2 if kind == 'p_laplace' else 1]
    e = Quasilinear2d(equation=(kind,) + tuple(args))
    u, f = drv.manufactured(e.equation, AMPLITUDE)
    e.bdy, e.rhs = u, f
    Xd, Xb = Q.points(ND, NB)
    e.get_sampled_points(Xd, Xb)
    e.Gram_matrix(kernel='Gaussian', kernel_parameter=SIGMA, nugget=NUGGET_E2E, nugget_type='adaptive')
    e.Gram_Cholesky()
    e.GN_method(max_iter=STEPS, step_size=1, initial_sol='zero', print_hist=False)
    z, hist, L, sysm = Q.numpy_pipeline('Gaussian', SIGMA, Xd, Xb, NUGGET_E2E, kind, e.equation.params, e.rhs_f, e.bdy_g, e.init_sol, STEPS)
    twin = np.load(os.path.join(ROOT, 'tests', 'golden', 'quasilinear_twin.npz'))[kind]
    return dict(e=e, z=z, hist=np.asarray(hist), L=L, sysm=sysm, u=u, f=f, twin=twin)


@pytest.mark.parametrize('kind', KINDS)
def test_class_end_to_end(kind):
    """RESULTS, float64 numpy pipeline on the CPU (measured first) / MI355X, N_d 150, N_b 40, sigma 0.3, nugget 1e-8, 8 steps from zero:
      mean_curvature   L2 1.890e-06 / 1.890e-06, residual RMS 1.264e-04 / 1.264e-04, distance to the long-double twin 1.31e-10 / 1.29e-10
      p_laplace        L2 4.068e-06 / 4.068e-06, residual RMS 4.315e-04 / 4.315e-04, distance 4.6e-11 / 1.32e-10
      gauss_curvature  L2 1.153e-05 / 1.153e-05, residual RMS 1.160e-03 / 1.160e-03, distance 4.45e-09 / 5.21e-09
    (distances relative to max |z|; allowed: 32 x numpy's).  Log evidence agrees with the numpy formulas to 1e-9 relative."""
    s = _solved(kind)
    e, z, hist, u, twin = s['e'], s['z'], s['hist'], s['u'], s['twin']
    Xd = e.X_domain
    assert e.chol_info == 0 and e.step_info == [0] * STEPS and len(e.loss_hist) == STEPS + 1
    np.testing.assert_allclose(e.ratio, np.asarray(Q.trace_ratios('Gaussian', SIGMA, ND, NB), dtype=np.float64), rtol=1e-14)
    zs = e._z_star[1]
    scale = float(np.max(np.abs(twin)))
    d_dev, d_np = float(np.max(np.abs(zs - twin))) / scale, float(np.max(np.abs(z - twin))) / scale
    ut = u(*Xd.T)
    l2_dev, l2_np = float(np.sqrt(np.mean((e.sol_sampled_pts - ut) ** 2))), float(np.sqrt(np.mean((z[:ND] - ut) ** 2)))
    print(f'\n[quasilinear {kind}] distance to the long-double twin / max |z|: device {d_dev:.3g}, numpy {d_np:.3g} (allowed {Q.MARGIN} x numpy); '
          f'L2 error: device {l2_dev:.3e}, numpy {l2_np:.3e}; loss device {e.loss_hist[-1]:.8g}, numpy {hist[-1]:.8g}')
    assert d_dev <= Q.MARGIN * d_np
    assert abs(l2_np - NUMPY_L2[kind]) <= 0.05 * NUMPY_L2[kind]             # the recorded CPU figure is this configuration's
    assert np.isfinite(l2_dev) and l2_dev <= 10 * l2_np
    fz = s['sysm'].F(zs)[0]
    assert np.max(np.abs(e.sol_vec - fz)) <= 1e-12 * np.max(np.abs(fz))
    # residual at interior test points: the entry point against numpy on the device's own rows, and against the numpy pipeline's level
    Xt = np.random.RandomState(5).uniform(0.05, 0.95, (200, 2))
    rows = e.extend_derivatives(Xt)
    assert tuple(rows) == NAMES6
    e.extend_sol(Xt)
    assert np.array_equal(VA.bits(e.extended_sol), VA.bits(rows['value']))
    res = e.PDE_residual(Xt)
    ft = s['f'](*Xt.T)
    want, mag = Q.divergence_form(kind, e.equation.params, ft, *(rows[n] for n in NAMES6))
    assert np.all(np.isfinite(res)) and np.max(np.abs(res - want) / mag) <= 16 * EPS
    # the numpy pipeline's residual: its solution vector extended with long-double rows rounded to float64
    coef = np.linalg.solve(s['L'].T, np.linalg.solve(s['L'], s['sysm'].F(z)[0]))
    np_rows = [(Q.monomial_rows('Gaussian', SIGMA, n, Xt, Xd, e.X_boundary)[0].astype(np.float64) @ coef) for n in NAMES6]
    res_np = Q.divergence_form(kind, e.equation.params, ft, *np_rows)[0]
    rms_dev, rms_np = float(np.sqrt(np.mean(res ** 2))), float(np.sqrt(np.mean(res_np ** 2)))
    print(f'[quasilinear {kind}] test-point residual RMS: device {rms_dev:.3e}, numpy {rms_np:.3e}; max test error '
          f'{np.max(np.abs(e.extended_sol - u(*Xt.T))):.3g}')
    assert rms_dev <= 10 * rms_np
    # log evidence at the device's iterate against the numpy formulas with LAPACK's factors
    _, Rf, _ = Q.posterior_prepare(s['sysm'], s['L'], zs)
    want_e = Q.log_evidence(s['sysm'], s['L'], zs, Rf)
    got = e.log_evidence()
    t = e.log_evidence_terms
    print(f'[quasilinear {kind}] log Z device {got:.12g}, numpy {want_e["log_Z"]:.12g}; J {t["J"]:.10g} / {want_e["J"]:.10g}')
    assert t['info'] == 0 and np.isfinite(got)
    for k in ('J', 'logdet_theta', 'logdet_H', 'two_pi_term'):
        assert abs(t[k] - want_e[k]) <= 1e-6 * max(abs(want_e[k]), 1.0), (k, t[k], want_e[k])
    assert abs(got - want_e['log_Z']) <= 1e-6 * (abs(want_e['J']) + abs(want_e['logdet_theta']) + abs(want_e['logdet_H']))
    for call in (lambda: e.posterior_variance(Xt), lambda: e.posterior_covariance(Xt), lambda: e.posterior_sample(Xt)):
        with pytest.raises(NotImplementedError):
            call()


def test_line_search_works_through_the_base_class():
    from src.linesearch import LineSearch
    s = _solved('gauss_curvature')
    e = s['e']
    e.line_search = LineSearch()
    try:
        e.GN_method(max_iter=4, initial_sol='zero', print_hist=False)
    finally:
        del e.line_search
    lh = np.asarray(e.loss_hist)
    print(f'\n[quasilinear line search] steps {e.step_hist}, loss {[float(f"{v:.4g}") for v in lh]}')
    assert len(e.step_hist) == 4 and not e.ls_failed and np.all(np.diff(lh) <= 1e-9 * lh[:-1])


# ------------------------------------------------------------------------------------------------ f. the driver
@pytest.mark.parametrize('args', [['--equation', 'mean_curvature', '--kappa', '1.0'], ['--equation', 'p_laplace', '--m', '3', '--delta', '1.0'],
                                  ['--equation', 'gauss_curvature', '--e', '2']])
def test_driver_runs(args, capsys):
    """the command lines of the README at a smaller size"""
    import main_Quasilinear2d as drv
    np.random.seed(1)
    solver = drv.main(args + ['--N_domain', '150', '--N_boundary', '40', '--GNsteps', '8', '--show_figure', '', '--test_residual', '1',
                              '--print_hist', ''])
    out = capsys.readouterr().out
    print(out[-600:])
    assert solver.eqn.N_domain == 150 and '[Test error] L2 error' in out and '[Test residual] L2 residual' in out
    assert np.isfinite(solver.test_L2_err) and solver.test_L2_err < 1e-2 and np.isfinite(solver.test_res_L2)
