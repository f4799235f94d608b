"""The Hessian Gram layout (gpk_assemble_hess, gpk_extend_functionals_hess), the system GPK_GN_MONGE_AMPERE, gpk_pde_residual_ma and the
class MongeAmpere2d on the device, against tests/_monge_ampere_reference.py.

  a. Gram entries, (N_d, N_b) = (33, 11) (crosses the 32-row tile; odd: 8-byte stores) and (64, 32) (16-byte stores), both kernels, with
     coincident domain / boundary points and pairs at a root of h_2 on one axis and distance 0 on the other.  Two gates: per entry
     |device - ref| <= (4e-15 + 4 eps arg) x magnitude sum of the entry's terms (MA.gram_allowed), and per block pair the gate of
     tests/test_gpu_gram_longdouble.py (4e-15 of max|block|).  Exactly symmetric; both store paths and the non-temporal policy give the
     same bits; an odd-ld sub-view between canaries is written inside N x N only; nugget and host_ratios3 match the reference.
  b. extension rows against long-double rows @ coeff for every single bit and the full mask, N_t = 5 and 130; repeatable to the bit, a
     row's bits independent of the mask; refusals leave `out` untouched.
  c. one Gauss-Newton step at N_d = 150, N_b = 40 by the method and bound of tests/test_gpu_semilinear.py (SL.gates), substitution path
     and inverted blocks of 256 and 512; the same step and gates at (N_d, N_b) = (64, 7) and (129, 3), substitution path and blocks of
     256, where the ends of the second segment of the two-segment profile (columns N_d and 3 N_d) sit on / one past the 64 / 128 edges;
     gpk_gn_direction / gpk_gn_step_ls from the iterate after two steps; the prepares refuse.
  d. the residual entry.   e. MongeAmpere2d end to end.
Every test prints what it measures under a [monge-ampere] tag.

RESULTS (MI355X): see DESIGN.md section K, "Fully nonlinear: Monge-Ampere".  The step at the block edges, worst ratio to the bound over
both sizes and both paths: H 0.177, g 0.221, loss 0.0351, delta 0.262, z 0.262 (cond(H) 3.6)."""
import ctypes as C

import numpy as np
import pytest

import _gauss_reference as GR
import _monge_ampere_reference as MA
import _view_arena as VA
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

LD, EPS = MA.LD, MA.EPS
PARAMS = GR.PARAMS                                 # ('Gaussian', 0.2), ('anisotropic_Gaussian', (0.3, 0.05))
SIZES = ((33, 11), (64, 32))
NAMES6 = ('value', 'd1', 'd2', 'd11', 'd12', 'd22')


@pytest.fixture(scope='module')
def ctx():
    import gpk
    c = gpk.Context(0)
    yield c
    c.close()


def gram_points(kernel, Nd, Nb):
    """uniform points with a coincident domain / boundary pair, a coincident domain pair, and two domain pairs at a root of h_2 on one
    axis (p d^2 = 1; the Gaussian kernel: d = sigma) and distance 0 on the other"""
    rng = np.random.RandomState(1000 * Nd + Nb)
    Xd, Xb = rng.uniform(0, 1, (Nd, 2)), rng.uniform(0, 1, (Nb, 2))
    p1, p2 = (float(v) for v in GR.precisions(kernel, PARAMS[kernel]))
    r1 = PARAMS[kernel] if kernel == 'Gaussian' else 1.0 / np.sqrt(p1)
    r2 = PARAMS[kernel] if kernel == 'Gaussian' else 1.0 / np.sqrt(p2)
    Xd[3] = (0.3, 0.4); Xd[2] = (0.3 + r1, 0.4); Xd[4] = (0.3, 0.4 + r2)
    Xd[6] = Xd[5]
    Xb[0] = Xd[1]; Xb[Nb - 1] = Xd[Nd - 1]
    return Xd, Xb


_REF = {}


def _reference(kernel, Nd, Nb):
    key = (kernel, Nd, Nb)
    if key not in _REF:
        Xd, Xb = gram_points(kernel, Nd, Nb)
        _REF[key] = (Xd, Xb) + MA.theta(kernel, PARAMS[kernel], Xd, Xb)
    return _REF[key]


# ------------------------------------------------------------------------------------------------ a. Gram entries
@pytest.mark.parametrize('kernel', MA.KERNELS)
@pytest.mark.parametrize('Nd,Nb', SIZES)
def test_gram_entries_against_long_double(ctx, kernel, Nd, Nb):
    Xd, Xb, T, mag, arg = _reference(kernel, Nd, Nb)
    N = 4 * Nd + Nb
    dT, ratios = ctx.assemble_hess(kernel, PARAMS[kernel], Xd, Xb)
    got = dT.download()
    dT.free()
    assert got.shape == (N, N) and np.all(np.isfinite(got)) and np.array_equal(got, got.T)
    blocks = MA.offsets(Nd, Nb)
    err = np.abs(got.astype(LD) - T)
    allowed = MA.gram_allowed(mag, arg)
    print()
    worst = 0.0
    for i, (ro, rn) in enumerate(blocks):
        for j, (co, cn) in enumerate(blocks):
            e, a, m = err[ro:ro + rn, co:co + cn], allowed[ro:ro + rn, co:co + cn], mag[ro:ro + rn, co:co + cn]
            r = float(np.max(np.where(a > 0, e / np.where(a > 0, a, 1), np.where(e > 0, np.inf, 0))))
            u = float(np.max(np.where(m > 0, e / np.where(m > 0, m, 1), 0))) / EPS
            print(f'[monge-ampere gram] {kernel} ({Nd}, {Nb}) <{MA.NAMES[i]},{MA.NAMES[j]}>: worst error {u:.3g} eps of the magnitude sum, '
                  f'{r:.3g} of the bound')
            worst = max(worst, r)
    w = GR.gate_blocks(got, T, None, blocks, blocks, ('assemble_hess', kernel, Nd, Nb))
    print(f'[monge-ampere gram] {kernel} ({Nd}, {Nb}): worst ratio to the per-entry bound {worst:.3g}; per block {w[0]:.3g} of max|block| '
          f'(allowed {GR.BOUND:.3g})')
    assert worst <= 1.0
    # the special pairs are in the set: a root of h_2 (<M,M> tiny against its magnitude sum) and coincident points
    assert abs(float(T[Nd + 2, Nd + 3])) <= 1e-12 * float(mag[Nd + 2, Nd + 3]) and float(arg[5, 6]) == 0.0 and float(arg[1, 3 * Nd + Nd]) == 0.0


@pytest.mark.parametrize('kernel', MA.KERNELS)
def test_store_paths_give_the_same_bits(ctx, kernel):
    Nd, Nb = 64, 32
    Xd, Xb = gram_points(kernel, Nd, Nb)

    def run():
        T, _ = ctx.assemble_hess(kernel, PARAMS[kernel], Xd, Xb, 1e-6, 'adaptive')
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


@pytest.mark.parametrize('cls,Nd,Nb', [('D', 33, 11), ('D', 64, 32), ('A', 64, 32)])
def test_views_between_canaries(ctx, cls, Nd, Nb):
    """class D: odd base offset and odd ld (8-byte stores); class A with ld > N: the 16-byte stores next to canaries"""
    import gpk
    kernel = 'anisotropic_Gaussian'
    Xd, Xb = gram_points(kernel, Nd, Nb)
    N = 4 * Nd + Nb
    plain, _ = ctx.assemble_hess(kernel, PARAMS[kernel], Xd, Xb, 1e-6, 'adaptive')
    want = plain.download()
    plain.free()
    dXd, dXb = ctx.points(Xd), ctx.points(Xb)
    v = VA.class_view(ctx, N, N, cls, ld_min=N + 8)
    assert v.cls == cls and v.ld > N and (cls != 'D' or v.ld % 2 == 1)
    ctx._chk(ctx.lib.gpk_assemble_hess(ctx.h, gpk.KERNEL[kernel], gpk.device.kernel_params(kernel, PARAMS[kernel]), dXd.ptr, Nd, dXb.ptr, Nb,
                                       1e-6, gpk.NUGGET['adaptive'], v.ptr, v.ld, None))
    ctx.synchronize()
    v.arena.assert_outside_untouched([v])
    assert np.array_equal(VA.bits(v.arena.get(v)), VA.bits(want))
    # ld < N is refused and nothing is written
    rc = ctx.lib.gpk_assemble_hess(ctx.h, gpk.KERNEL[kernel], gpk.device.kernel_params(kernel, PARAMS[kernel]), dXd.ptr, Nd, dXb.ptr, Nb,
                                   1e-6, gpk.NUGGET['adaptive'], v.ptr, N - 1, None)
    assert rc == -9001 and b'assemble_hess: ld < N' in ctx.lib.gpk_last_error(ctx.h)
    for kid in (8, 9, 10):                                             # the Matern ids
        assert ctx.lib.gpk_assemble_hess(ctx.h, kid, (C.c_double * 2)(0.5, 0.5), dXd.ptr, Nd, dXb.ptr, Nb, 0.0, 0, v.ptr, v.ld, None) == -9001
    ctx.synchronize()
    v.arena.assert_outside_untouched([v])
    assert np.array_equal(VA.bits(v.arena.get(v)), VA.bits(want))
    v.arena.free()


@pytest.mark.parametrize('kernel', MA.KERNELS)
def test_nugget_diagonal_and_ratios(ctx, kernel):
    kp = PARAMS[kernel]
    for Nd, Nb in SIZES:
        Xd, Xb = gram_points(kernel, Nd, Nb)
        diag = MA.diagonal_values(kernel, kp)
        want_r = np.asarray(MA.trace_ratios(kernel, kp, Nd, Nb), dtype=np.float64)
        for nugget_type in ('none', 'identity', 'adaptive'):
            dT, ratios = ctx.assemble_hess(kernel, kp, Xd, Xb, 1e-6, nugget_type)
            got = np.diag(dT.download()).astype(LD)
            dT.free()
            np.testing.assert_allclose(ratios, want_r, rtol=1e-14)
            for (o, n), c, v in zip(MA.offsets(Nd, Nb), diag, MA.block_nuggets(kernel, kp, Nd, Nb, 1e-6, nugget_type)):
                want = c + v
                err = float(np.max(np.abs(got[o:o + n] - want)) / abs(want))
                assert err <= 4e-15, (nugget_type, (Nd, Nb), o, err)


# ------------------------------------------------------------------------------------------------ b. extension
@pytest.mark.parametrize('kernel', MA.KERNELS)
@pytest.mark.parametrize('Nd,Nb', [(33, 11), (265, 41)])               # the lanes' stride loop runs once, partly filled / twice (M = 306)
def test_extension_rows(ctx, kernel, Nd, Nb):
    kp = PARAMS[kernel]
    Xd, Xb = gram_points(kernel, Nd, Nb)
    N = 4 * Nd + Nb
    rng = np.random.RandomState(N)
    coeff = rng.normal(size=N)
    Xt_all = rng.uniform(0, 1, (130, 2))
    Xt_all[0], Xt_all[3], Xt_all[129] = Xd[3], Xb[2], Xd[Nd - 1]       # collocation points among the test points
    print()
    for Nt in (5, 130):                                                # a ragged last group of 4 (one point); more than one workgroup
        Xt = Xt_all[:Nt] if Nt == 130 else Xt_all[[0, 3, 7, 8, 129]]
        full = ctx.extend_functionals_hess(kernel, kp, Xt, Xd, Xb, coeff).download().reshape(6, Nt)
        again = ctx.extend_functionals_hess(kernel, kp, Xt, Xd, Xb, coeff).download().reshape(6, Nt)
        assert np.array_equal(VA.bits(full), VA.bits(again)) and np.all(np.isfinite(full))
        for k, name in enumerate(NAMES6):
            rows, mag, arg = MA.monomial_rows(kernel, kp, name, Xt, Xd, Xb)
            want = rows @ coeff.astype(LD)
            allowed = ((64 * LD(EPS) + 4 * LD(EPS) * arg) * mag) @ np.abs(coeff).astype(LD)
            single = ctx.extend_functionals_hess(kernel, kp, Xt, Xd, Xb, coeff, which=(name,)).download().reshape(Nt)
            assert np.array_equal(VA.bits(single), VA.bits(full[k])), (name, 'the bits of a row depend on the mask')
            ratio = float(np.max(np.abs(single.astype(LD) - want) / allowed))
            print(f'[monge-ampere extend] {kernel} ({Nd}, {Nb}) Nt {Nt} {name}: worst error / bound {ratio:.3g} '
                  f'(bound: 64 eps + 4 eps arg of the magnitude sums @ |coeff|)')
            assert ratio <= 1.0, (name, Nt)
        pair = ctx.extend_functionals_hess(kernel, kp, Xt, Xd, Xb, coeff, which=('d22', 'd1')).download().reshape(2, Nt)
        assert np.array_equal(VA.bits(pair[0]), VA.bits(full[5])) and np.array_equal(VA.bits(pair[1]), VA.bits(full[1]))


def test_extension_refusals_leave_out_untouched(ctx):
    import gpk
    Nd, Nb, Nt = 33, 11, 5
    Xd, Xb = gram_points('Gaussian', Nd, Nb)
    dXd, dXb, dXt = ctx.points(Xd), ctx.points(Xb), ctx.points(Xd[:Nt])
    coeff = ctx.array(np.ones(4 * Nd + Nb))
    out = ctx.empty(6, 8, ld=8)
    canary = np.full((6, 8), 3.25)
    out.upload(canary)
    kp = gpk.device.kernel_params('Gaussian', 0.2)
    fn = ctx.lib.gpk_extend_functionals_hess
    assert fn(ctx.h, 0, kp, dXt.ptr, Nt, dXd.ptr, Nd, dXb.ptr, Nb, coeff.ptr, 63, out.ptr, Nt - 1) == -9001
    assert b'extend_functionals_hess: ldo < Nt' in ctx.lib.gpk_last_error(ctx.h)
    for mask in (0, 64, -1):
        assert fn(ctx.h, 0, kp, dXt.ptr, Nt, dXd.ptr, Nd, dXb.ptr, Nb, coeff.ptr, mask, out.ptr, 8) == -9001
        assert b'fmask' in ctx.lib.gpk_last_error(ctx.h)
    for kid in (8, 9, 10, 2):
        assert fn(ctx.h, kid, (C.c_double * 2)(0.5, 0.5), dXt.ptr, Nt, dXd.ptr, Nd, dXb.ptr, Nb, coeff.ptr, 63, out.ptr, 8) == -9001
    assert fn(ctx.h, 0, kp, dXt.ptr, 0, dXd.ptr, Nd, dXb.ptr, Nb, coeff.ptr, 63, out.ptr, 8) == -9001
    ctx.synchronize()
    assert np.array_equal(out.download(), canary)
    assert fn(ctx.h, 0, kp, dXt.ptr, Nt, dXd.ptr, Nd, dXb.ptr, Nb, coeff.ptr, 1 | 8, out.ptr, 8) == 0     # rows 0, 1; entries past Nt untouched
    ctx.synchronize()
    got = out.download()
    assert np.all(got[:2, :Nt] != 3.25) and np.array_equal(got[:2, Nt:], canary[:2, Nt:]) and np.array_equal(got[2:], canary[2:])


# ------------------------------------------------------------------------------------------------ c. one Gauss-Newton step
def _upload_factor(ctx, L):
    n = L.shape[0]
    d = ctx.empty(n, n + MA.R.LD_PAD, ld=n + MA.R.LD_PAD)
    d.upload(MA.poisoned(L))
    d.cols = n
    return d


def _problem(ctx, cs, dinv, system='MongeAmpere2d', **kw):
    import gpk
    L = _upload_factor(ctx, cs.L)
    prob = gpk.GNProblem(ctx, system, cs.Nd, cs.Nb, cs.f, cs.g, L, dinv=dinv, **kw)
    prob.keep.append(L)
    return prob


def _report(tag, res):
    bad = []
    for name, (r, a) in res.items():
        print(f'[monge-ampere {tag}] {name}: device {r / EPS:.3g} eps, allowed {a / EPS:.3g} eps, ratio to the bound {r / a:.3g}')
        if not r <= a:
            bad.append((name, r, a))
    return bad


STEP = (150, 40)


@pytest.mark.parametrize('dinv', [False, 256, 512])
def test_step_hessian_grad_loss(ctx, dinv):
    cs, ref = MA.case(*STEP), MA.full_reference(*STEP)
    prob = _problem(ctx, cs, dinv)
    assert (prob.nz, prob.rows) == (450, 640)
    z = ctx.array(cs.z0)
    H, g = ctx.gn_hessian_grad(prob, z)
    loss = ctx.gn_loss(prob, z)
    step_loss, info = ctx.gn_step(prob, z, 1.0)
    delta, z_out = prob.workspace()[2].download().copy(), z.download().copy()
    prob.free()
    print(f'\n[monge-ampere step] dinv {dinv}: cond(H) {ref.cond:.3g}')
    assert info == 0 and np.array_equal(H, H.T)
    bad = _report(f'step dinv {dinv}', MA.gates(ref, H=H, g=g, loss=loss, delta=delta, z_out=z_out))
    bad += _report(f'step dinv {dinv} in-step', MA.gates(ref, loss=step_loss))
    assert not bad, bad


# N_d on a 64-edge and one past a 128-edge: the second segment of the two-segment profile (dinv) starts at column N_d and ends at 3 N_d,
# so its ends sit on / next to the 64 / 128 / 256 tile and block edges (columns 64, 192; 129, 387); N_b of _gn_reference.NB where defined
STEP_EDGES = tuple((Nd, MA.R.NB.get(Nd, 7)) for Nd in (64, 129))


@pytest.mark.parametrize('dinv', [False, 256])
@pytest.mark.parametrize('Nd,Nb', STEP_EDGES)
def test_step_at_the_block_edges_of_the_profile(ctx, Nd, Nb, dinv):
    """the step of test_step_hessian_grad_loss, same gates, at (N_d, N_b) = (64, 7) and (129, 3): dinv = 256 runs the two-segment
    profile, dinv = False the conservative closed form"""
    cs, ref = MA.case(Nd, Nb), MA.full_reference(Nd, Nb)
    prob = _problem(ctx, cs, dinv)
    assert (prob.nz, prob.rows) == (3 * Nd, 4 * Nd + Nb)
    z = ctx.array(cs.z0)
    H, g = ctx.gn_hessian_grad(prob, z)
    loss = ctx.gn_loss(prob, z)
    step_loss, info = ctx.gn_step(prob, z, 1.0)
    delta, z_out = prob.workspace()[2].download().copy(), z.download().copy()
    prob.free()
    print(f'\n[monge-ampere step] N_d {Nd} N_b {Nb} dinv {dinv}: cond(H) {ref.cond:.3g}')
    assert info == 0 and np.array_equal(H, H.T)
    bad = _report(f'step {Nd} dinv {dinv}', MA.gates(ref, H=H, g=g, loss=loss, delta=delta, z_out=z_out))
    bad += _report(f'step {Nd} dinv {dinv} in-step', MA.gates(ref, loss=step_loss))
    assert not bad, bad


def test_direction_and_line_searched_step(ctx):
    cs = MA.case(*STEP)
    prob = _problem(ctx, cs, 256)
    z = ctx.array(cs.z0)
    for _ in range(2):
        ctx.gn_step(prob, z, 1.0)
    z2 = z.download().copy()
    loss0 = ctx.gn_loss(prob, z)
    loss_d, pred, info = ctx.gn_direction(prob, z)
    assert info == 0 and np.array_equal(z.download(), z2)              # the direction call does not write z
    ref = MA.FullReference(cs, z2)
    delta = prob.workspace()[2].download().copy()
    print()
    bad = _report('direction', MA.gates(ref, loss=loss_d, delta=delta))
    loss_in, info, k, t, trial = ctx.gn_step_ls(prob, z, 8, 1.0, 0.5, 1e-4)
    loss1 = ctx.gn_loss(prob, z)
    prob.free()
    print(f'[monge-ampere line search] loss {loss0:.17g} -> {loss1:.17g}, accepted k {k}, t {t}, pred {pred:.3g}, trial losses {trial}')
    assert not bad, bad
    assert info == 0 and abs(loss_in - loss0) <= 1e-12 * loss0 and pred >= 0
    assert k >= 0 and loss1 < loss0                                    # the one hard condition: the line-searched step decreases the loss


def test_prepares_and_nonlin_are_refused(ctx):
    cs = MA.case(*STEP)
    prob = _problem(ctx, cs, 256)
    S, H, delta, _ = prob.workspace()
    W = ctx.empty(prob.rows, prob.nz + 2)
    rc = ctx.lib.gpk_gn_structured_prepare(ctx.h, C.byref(prob.struct), S.ptr, S.ld, W.ptr, W.ptr, None, W.ld)
    assert rc == -9001 and b'GPK_GN_MONGE_AMPERE' in ctx.lib.gpk_last_error(ctx.h)
    rc = ctx.lib.gpk_gn_gram_prepare(ctx.h, C.byref(prob.struct), W.ptr, W.ld, delta.ptr)
    assert rc == -9001 and b'GPK_GN_MONGE_AMPERE' in ctx.lib.gpk_last_error(ctx.h)
    prob.struct.nonlin = 1
    loss = C.c_double()
    z = ctx.array(cs.z0)
    assert ctx.lib.gpk_gn_loss(ctx.h, C.byref(prob.struct), z.ptr, prob.workspace()[3].ptr, C.byref(loss)) == -9001
    prob.struct.nonlin = 0
    # the ids next to the new ones stay refused
    out = ctx.empty(4, 8)
    assert ctx.lib.gpk_pde_residual(ctx.h, 6, (C.c_double * 3)(1, 1, 0), 4, out.ptr, 8, None, 0, out.ptr, out.ptr) == -9001
    prob.free()


# ------------------------------------------------------------------------------------------------ d. the residual entry
def test_residual_entry(ctx):
    rng = np.random.RandomState(9)
    Nt = 300
    fields, f = rng.normal(size=(3, Nt)), rng.uniform(0.5, 2, Nt)
    want = (fields[0] * fields[2] - fields[1] * fields[1]) - f       # the entry's order of operations: equal to the bit
    a = ctx.pde_residual_ma(fields, f).download().ravel()
    b = ctx.pde_residual_ma(fields, f).download().ravel()
    assert np.array_equal(VA.bits(a), VA.bits(b)) and np.array_equal(VA.bits(a), VA.bits(want))
    du, dr, out = ctx.array(fields), ctx.array(f), ctx.empty(Nt)
    fn = ctx.lib.gpk_pde_residual_ma
    assert fn(ctx.h, 0, du.ptr, du.ld, dr.ptr, out.ptr) == -9001 and b'pde_residual_ma: Nt <= 0' in ctx.lib.gpk_last_error(ctx.h)
    assert fn(ctx.h, Nt, du.ptr, Nt - 1, dr.ptr, out.ptr) == -9001
    for args in ((None, du.ld, dr.ptr, out.ptr), (du.ptr, du.ld, None, out.ptr), (du.ptr, du.ld, dr.ptr, None)):
        assert fn(ctx.h, Nt, *args) == -9001


# ------------------------------------------------------------------------------------------------ e. end to end through the class
def test_class_end_to_end():
    from src.PDEs import MongeAmpere2d
    Nd, Nb, steps = 300, 80, 8
    Xd, Xb = MA.points(Nd, Nb)
    e = MongeAmpere2d(bdy=MA.truth, rhs=MA.rhs)
    e.get_sampled_points(Xd, Xb)
    e.Gram_matrix(kernel='Gaussian', kernel_parameter=0.3, nugget=1e-8, nugget_type='adaptive')
    e.Gram_Cholesky()
    assert e.chol_info == 0
    np.testing.assert_allclose(e.ratio, np.asarray(MA.trace_ratios('Gaussian', 0.3, Nd, Nb), dtype=np.float64), rtol=1e-14)
    e.GN_method(max_iter=steps, step_size=1, initial_sol='zero', print_hist=False)
    assert all(i == 0 for i in e.step_info) and len(e.loss_hist) == steps + 1
    # the reference iteration on the device's own Theta, factored by LAPACK
    L = O.cholesky(e.Theta)
    sysm = MA.System(e.rhs_f, e.bdy_g)
    z_ref, hist = MA.gn_float64(sysm, L, np.zeros(3 * Nd), steps)
    z_dev = e._z_star[1]
    rel = float(np.linalg.norm(z_dev - z_ref) / np.linalg.norm(z_ref))
    us = MA.truth(Xd[:, 0], Xd[:, 1])
    l2 = float(np.sqrt(np.mean((e.sol_sampled_pts - us) ** 2)))
    print(f'\n[monge-ampere class] parity of the iterate {rel:.3g}, L2 error {l2:.3g}, loss history {[float("%.9g" % v) for v in e.loss_hist]}, '
          f'reference {hist[-1]:.9g}')
    assert rel <= 1e-6
    assert l2 < 1e-4
    assert np.max(np.abs(e.sol_vec - sysm.F(z_dev)[0])) <= 1e-13 * np.max(np.abs(e.sol_vec))
    # residual at 200 interior test points
    Xt = np.random.RandomState(5).uniform(0.05, 0.95, (200, 2))
    res = e.PDE_residual(Xt)
    rows = e.extend_derivatives(Xt)
    f_t = MA.rhs(Xt[:, 0], Xt[:, 1])
    rms_r, rms_f = float(np.sqrt(np.mean(res ** 2))), float(np.sqrt(np.mean(f_t ** 2)))
    print(f'[monge-ampere class] residual RMS {rms_r:.3g}, RMS of f {rms_f:.3g}, ratio {rms_f / rms_r:.3g}')
    assert np.all(np.isfinite(res)) and rms_r * 1e2 <= rms_f
    want = (rows['d11'] * rows['d22'] - rows['d12'] * rows['d12']) - f_t
    assert np.array_equal(VA.bits(res), VA.bits(want))
    e.extend_sol(Xt)
    assert np.array_equal(VA.bits(e.extended_sol), VA.bits(rows['value']))
    ut = MA.truth(Xt[:, 0], Xt[:, 1])
    print(f'[monge-ampere class] max test error {np.max(np.abs(e.extended_sol - ut)):.3g}')
    assert np.max(np.abs(e.extended_sol - ut)) < 1e-3
    # log evidence against the reference formula
    lz = e.log_evidence()
    _, Rf, _ = MA.posterior_prepare(sysm, L, z_dev)
    want_lz = MA.log_evidence(sysm, L, z_dev, Rf)
    want_lz = want_lz['log_Z'] if isinstance(want_lz, dict) else want_lz[0]
    print(f'[monge-ampere class] log evidence {lz:.12g}, reference {want_lz:.12g}, relative difference {abs(lz - want_lz) / abs(want_lz):.3g}')
    assert abs(lz - want_lz) <= 1e-8 * abs(want_lz)
    for call in (e.posterior_variance, e.posterior_covariance, e.posterior_sample):
        with pytest.raises(NotImplementedError):
            call(Xt)
    # the line search is honoured
    from src.linesearch import LineSearch
    e.line_search = LineSearch()
    e.GN_method(max_iter=3, step_size=1, initial_sol='zero', print_hist=False)
    print(f'[monge-ampere class] line search: steps {e.step_hist}, loss history {[float("%.9g" % v) for v in e.loss_hist]}')
    assert all(k >= 0 for k in e.ls_accepted) and e.loss_hist[-1] < e.loss_hist[0]
