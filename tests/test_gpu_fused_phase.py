"""The fused product + Cholesky phase of the Gauss-Newton step, entry by entry (gate and row sample: tests/_fused_phase_reference.py; the
gate is shown to bite in tests/test_fused_phase_host.py).

The phase Hb = chol(W^T W) -- gpk_i_syrk_potrf -> potrf_pipelined (csrc/gpk_factor.hip), Darcy's own assembly of H and the Gram-level
modes (csrc/gpk_gn.hip) -- is gated on the factored Hb itself: factor, border row y = L_H^-1 g / 2 and corner, for <= 48 sampled rows and
every column left of the diagonal, against the device's OWN solved block W in long double, at the smallest shapes where each schedule is
active.  Synthetic well-conditioned factors of _gn_reference (upper triangle and padding poisoned), random start, N_b = 40 (elliptic
N_d = 1100 is the case of test_gpu_gn_rounding.py section d, N_b = 160).  The constant is 32 x the figure of the float64 host rendition
on the same W + 1, computed at run time.

  a. substitution form (dinv=False: the solve is in place, prob.workspace()[0] holds W, [1] the factored Hb) of gpk_gn_direction, three
     repeats on one handle (same bits of Hb and delta): elliptic nc = n_z + 1 = 1025, 1088, 1101, 1536, 1537; Burgers and Eikonal
     N_d = 342, 512 (nc = 1027, 1537); relaxed N_d = 513 (nc = 1027); Semilinear and Monge-Ampere N_d = 342 (nc = 1027).  info = 0, loss =
     gpk_gn_loss bit for bit, pred within the allowed ratio of |y|^2 of the downloaded border row, and -- one more gpk_gn_step with the
     profiler on -- the phase ran pipelined (a handle that could not create its CU-masked streams fails here with that message).
     Row 0 of W: with a leading-zero layout gpk_i_gn_finish uses the first n_z doubles of S as scratch for the reversed-order solution,
     after the phase has read them; they are restored as (row 0 of the device's own gpk_gn_build_rev) / L[0][0] -- the first row of a
     forward substitution.  Should the device round that one quotient differently, the entry (i, j) moves by eps |W_0i W_0j|, one term
     of the several thousand in s_ij.
  b. a. under every entry of test_gpu_variants.VARIANTS and under forced tile lists ({42: 2}) at elliptic nc = 1101, 1537 and Burgers
     nc = 1027 (one call each; the sample follows the block widths of keys 28 / 29); not pipelined exactly for {12: 0}.
  c. Darcy N_d = 171 (n_z = 1026: its own assembly of H -- leading-zero product, add_lower_kernel / the a-part product, border launches --
     over three 512-blocks) with the inverted blocks, cache_a on and off (bit for bit the same Hb, delta, loss, pred), and with
     gpk_i_potrf on the pipelined schedule.  That layout exists only with the inverted blocks, whose W lives in the handle's workspace:
     the operand is the W of a substitution-form gpk_gn_direction at the same z on the same handle (dense layout), its columns permuted
     into the step's order.  {20: 100000} alone does not move gpk_i_potrf onto the pipeline at order 1027 (key 19, its lower limit, is
     2048): the case sets {19: 1024, 20: 100000}.  The profiler's flag belongs to gpk_i_syrk_potrf and stays 0 for Darcy.
  d. Gram-level mode (structured=2), elliptic n_z = 257, 513, 1025 (second trip of the stride loops of gram_gemv_kernel / gram_form_kernel /
     gram_loss_kernel) and Eikonal N_d = 342: Hb against the W of a substitution-form call on the same handle, the scale widened by the
     magnitude sum of what gram_form_kernel adds, |d_c||G11||d_c'| + |d_c||G12| + |G21||d_c'| + |G22| (G: the device's own blocks), and for
     the border row by the magnitude sums of its terms (elliptic: d_c q1_c + q2_c with q = G [a; z] + p and the corner p0 + a.(p1 + q1) +
     z.(p2 + q2); Eikonal: d_c (W1^T w)_c + (W2^T w)_c).  The host rendition is gated with the same scale.
  e. structured level 1, elliptic n_z = 513, 1025 (second trip of structured_form_kernel) and the dinv forms of the systems and sizes of
     a. and c.: their W lives in the handle's workspace, which the development library does not expose, so these are gated by the loss and
     delta against _gn_reference.VectorReference, as section d of test_gpu_gn_rounding.py.  Semilinear and Monge-Ampere N_d = 342
     (nc = 1027) with inverted blocks of 256 and 512, against the VectorReference of _semilinear_reference / _monge_ampere_reference:
     the two-partition pipeline plus the GEMM-only solve, where Monge-Ampere runs Eikonal's two-segment profile and Semilinear must not
     (the gates reject the dropped N_u / eps entries: tests/test_semilinear_host.py); three steps on one handle give the same bits.

RESULTS: every test prints `device, allowed (numpy); worst so far` under its tag.  Worst lines of a run on an MI355X, as "tag: device
of allowed (numpy)":
  [fused] 8.6 of 196 (6.09), relaxed nc 1027;   [fused pred] 0.517 of 33 (1);
  [fused variants] 13.5 of 119 (3.69);          [fused variants pred] 0.748 of 33 (1);
  [fused darcy] 6.22 of 115 (3.56);             [fused darcy pred] 0.172 of 33 (1);
  [fused gram] 7.98 of 106 (3.28), Eikonal;     [fused gram pred] 0.458 of 33 (1);
  [fused vector loss] 0.716 of 33 (1);  [fused vector backward] 2.11 of 26.1 (0.784);  [fused vector forward] 9.43 of 126 (3.91).
  Semilinear N_d 342, dinv 256 / 512: [fused vector loss] 0.306 of 39.4 (1.2), backward 0.381 of 12.8 (0.368), forward 277 of 8.43e3 (263:
  its H has the larger condition; the device is at 1.05 x the float64 rendition);  Monge-Ampere N_d 342: loss 0.106 of 33 (1), backward
  1.5 of 43 (1.31), forward 4.47 of 128 (3.96).  Both repeat their bits over three steps and ran pipelined.
The device stays within a factor 4 of the float64 host rendition everywhere; Darcy's loss - |y|^2 is 5e-7 of the loss at this start.
No variant of test_gpu_variants.VARIANTS is documented as not bit-repeatable; the repeat-bits assertions run on the default schedule only.
"""
import ctypes as C

import numpy as np
import pytest

import _fused_phase_reference as FP
import _gn_reference as R
import _staircase_model as M
from test_gpu_variants import DEFAULTS, VARIANTS

pytestmark = pytest.mark.gpu

LD, EPS = R.LD, R.EPS
WORST = {}
NO_STREAMS = ('the fused phase did not run on the two-partition pipeline: the handle could not create its CU-masked streams '
              '(hipExtStreamCreateWithCUMask) or the schedule fell back to one stream')


def _note(tag, ratio, allowed, what, numpy=None):
    w = WORST.setdefault(tag, (0.0, 0.0, allowed))
    if not ratio / allowed < w[0]:
        WORST[tag] = (ratio / allowed, ratio, allowed)
    numpy = (allowed - 1.0) / R.MARGIN if numpy is None else numpy
    print(f'[{tag}] {what}: device {ratio:.3g}, allowed {allowed:.3g} (numpy {numpy:.3g}); '
          f'worst so far {WORST[tag][1]:.3g} of {WORST[tag][2]:.3g}')


# ------------------------------------------------------------------------------------------------ cases and problems
def _case(kind, Nd):
    if kind == 'semilinear':
        import _semilinear_reference as SL
        return SL.Case(Nd, FP.NB_FUSED)
    if kind == 'monge_ampere':
        import _monge_ampere_reference as MA
        return MA.case(Nd, FP.NB_FUSED)
    return FP.case(kind, Nd)


_FACTORS = {}


def _factors(ctx, kind, cs):
    """the uploaded (poisoned) factors of a case, once per handle"""
    key = (id(ctx), kind, cs.Nd)
    if key not in _FACTORS:
        def up(L):
            n = L.shape[0]
            d = ctx.empty(n, n + R.LD_PAD, ld=n + R.LD_PAD)
            d.upload(R.poisoned(L))
            d.cols = n
            return d
        L2 = getattr(cs, 'L2', None)
        _FACTORS[key] = (up(cs.L), up(L2) if L2 is not None else None)
    return _FACTORS[key]


def _problem(ctx, kind, cs, **form):
    import gpk
    L, L2 = _factors(ctx, kind, cs)
    if kind == 'semilinear':
        return gpk.GNProblem(ctx, 'Semilinear2d', cs.Nd, cs.Nb, cs.f, cs.g, L, p0=cs.eps, gq=cs.gq, **form)
    if kind == 'monge_ampere':
        return gpk.GNProblem(ctx, 'MongeAmpere2d', cs.Nd, cs.Nb, cs.f, cs.g, L, **form)
    return gpk.GNProblem(ctx, R.SYSTEM_NAME[kind], cs.Nd, cs.Nb, cs.f, cs.g, L, p0=cs.p0, p1=cs.p1, pen_lambda=cs.lam, data_u=cs.data,
                         L2=L2, **form)


def _column_order(kind, Nd):
    return M.column_of_unknown({'semilinear': 'eikonal', 'monge_ampere': 'eikonal'}.get(kind, kind), Nd)


def _direction(ctx, prob, z):
    loss, pred, info = ctx.gn_direction(prob, z)
    _, H, delta, _ = prob.workspace()
    # (the strict upper triangle of the Hb buffer is scratch of the product launches, never read: not part of the result)
    return loss, pred, info, np.tril(H.download()), delta.download().copy()


def _operand(ctx, kind, cs, sub, z):
    """W of the substitution-form problem `sub` after a call at z, in the step's internal column order (F column last)"""
    S = sub.workspace()[0]
    nz = cs.nz
    W = S.download()
    if kind == 'darcy':                                              # dense layout without the inverted blocks: natural column order, S untouched
        out = np.empty_like(W)
        out[:, _column_order(kind, cs.Nd)] = W[:, :nz]
        out[:, nz] = W[:, nz]
        return out
    B = ctx.empty(sub.rows, nz + 1)                                  # row 0, columns < n_z: scratch of gpk_i_gn_finish (module docstring)
    if kind == 'relaxed':
        ctx._chk(ctx.lib.gpk_gn_build(ctx.h, C.byref(sub.struct), z.ptr, B.ptr, B.ld))
        row0 = B.download(rows=1)[0, :nz][::-1]
    else:
        ctx._chk(ctx.lib.gpk_gn_build_rev(ctx.h, C.byref(sub.struct), z.ptr, B.ptr, B.ld))
        row0 = B.download(rows=1)[0, :nz]
    B.free()
    W[0, :nz] = row0 / cs.L[0, 0]
    return W


def _set(ctx, variant):
    for k, v in DEFAULTS.items():
        ctx.lib.gpk_debug_set(k, v)
    for k, v in variant.items():
        ctx.lib.gpk_debug_set(k, v)


def _reset(ctx):
    _set(ctx, {42: 1, 19: 2048})


def _pipelined_step(ctx, prob, z0):
    z = ctx.array(z0)
    ctx.prof_enable()
    try:
        _, info = ctx.gn_step(prob, z, 0.5)
        prof = ctx.prof_read()
    finally:
        ctx.prof_enable(False)
        z.free()
    assert info == 0
    return prof['pipelined']


def _gate_call(tag, what, W, call, widths=(512, 512), extra=None):
    """the checks of one gpk_gn_direction call against its operand; returns the failures"""
    loss, pred, info, Hb, delta = call
    nz = W.shape[1] - 1
    bad = []
    if info != 0:
        bad.append(f'info = {info}')
    r, a, npr, where, rows = FP.gate(W, Hb, *widths, extra=extra)
    assert len(rows) <= FP.MAX_ROWS
    _note(tag, r, a, f'{what} at {where}', npr)
    if not r <= a:
        bad.append(f'Hb: {r:.4g} > {a:.4g} at {where}')
    rp, ap = FP.pred_gate(pred, Hb[nz, :nz])
    _note(f'{tag} pred', rp, ap, what)
    if not rp <= ap:
        bad.append(f'pred: {rp:.4g} > {ap:.4g}')
    # the border pivot loss - |y|^2 has to stand clear of its own rounding error: the gate lets the corner entry move by allowed eps s with
    # s = 2 loss and allowed of a few hundred at the most, i.e. by 1e-13 loss; four orders of magnitude above that counts as comfortable
    if not loss - pred > 1e-9 * loss:
        bad.append(f'loss - |y|^2 is not comfortably positive: {loss} - {pred}')
    return bad


# ------------------------------------------------------------------------------------------------ a. substitution form
SUBSTITUTION = [('elliptic', 1024), ('elliptic', 1087), ('elliptic', 1100), ('elliptic', 1535), ('elliptic', 1536),
                ('burgers', 342), ('burgers', 512), ('eikonal', 342), ('eikonal', 512), ('relaxed', 513),
                ('semilinear', 342), ('monge_ampere', 342)]


@pytest.mark.parametrize('kind,Nd', SUBSTITUTION)
def test_substitution_form(dev_ctx, kind, Nd):
    ctx, cs = dev_ctx, _case(kind, Nd)
    assert cs.nz + 1 >= 1025
    prob = _problem(ctx, kind, cs, dinv=False)
    z = ctx.array(cs.z0)
    print()
    try:
        calls = [_direction(ctx, prob, z) for _ in range(3)]
        W = _operand(ctx, kind, cs, prob, z)
        bad = _gate_call('fused', f'{kind} nc {cs.nz + 1}', W, calls[0])
        assert calls[0][0] == ctx.gn_loss(prob, z), 'the reported loss is not gpk_gn_loss'
        assert np.array_equal(z.download(), cs.z0)
        for c in calls[1:]:
            assert c[:3] == calls[0][:3] and np.array_equal(c[3], calls[0][3]) and np.array_equal(c[4], calls[0][4]), 'not repeatable'
        assert _pipelined_step(ctx, prob, cs.z0), NO_STREAMS
    finally:
        prob.free(); z.free()
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ b. schedule variants
SCHEDULES = list(VARIANTS) + [('forced tile lists', {42: 2})]
VARIANT_CASES = [('elliptic', 1100), ('elliptic', 1536), ('burgers', 342)]


@pytest.mark.parametrize('sched', range(len(SCHEDULES)), ids=lambda i: '-'.join(f'{k}={v}' for k, v in SCHEDULES[i][1].items()) or 'default')
@pytest.mark.parametrize('kind,Nd', VARIANT_CASES)
def test_substitution_form_under_schedule_variants(dev_ctx, kind, Nd, sched):
    ctx, cs = dev_ctx, _case(kind, Nd)
    name, variant = SCHEDULES[sched]
    widths = (variant.get(28, 512), variant.get(29, 512))
    print()
    try:
        _set(ctx, {42: 1, **variant})
        prob = _problem(ctx, kind, cs, dinv=False)
        z = ctx.array(cs.z0)
        call = _direction(ctx, prob, z)
        W = _operand(ctx, kind, cs, prob, z)
        bad = _gate_call('fused variants', f'{kind} nc {cs.nz + 1} {name}', W, call, widths)
        assert call[0] == ctx.gn_loss(prob, z), 'the reported loss is not gpk_gn_loss'
        pipelined = _pipelined_step(ctx, prob, cs.z0)
        prob.free(); z.free()
    finally:
        _reset(ctx)
    if variant.get(12, 1) == 0:
        assert not pipelined
    else:
        assert pipelined, NO_STREAMS
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ c. Darcy's own assembly of H
def test_darcy_assembly(dev_ctx):
    ctx, cs = dev_ctx, _case('darcy', 171)
    assert cs.nz == 1026
    z = ctx.array(cs.z0)
    sub = _problem(ctx, 'darcy', cs, dinv=False, cache_a=False)
    print()
    bad = []
    try:
        _direction(ctx, sub, z)
        W = _operand(ctx, 'darcy', cs, sub, z)
        out = {}
        for cached in (True, False):
            prob = _problem(ctx, 'darcy', cs, dinv=256, cache_a=cached)
            assert (prob.Wa is not None) == cached
            mode, product = C.c_int(), C.c_int()
            ctx._chk(ctx.lib.gpk_debug_step_mode(ctx.h, C.byref(prob.struct), C.byref(mode), C.byref(product)))
            assert product.value == 2, 'the Darcy step does not run its own assembly of H'
            calls = [_direction(ctx, prob, z) for _ in range(3)]
            bad += _gate_call('fused darcy', f'darcy nc {cs.nz + 1} cache_a={cached}', W, calls[0])
            assert calls[0][0] == ctx.gn_loss(prob, z), 'the reported loss is not gpk_gn_loss'
            for c in calls[1:]:
                assert c[:3] == calls[0][:3] and np.array_equal(c[3], calls[0][3]) and np.array_equal(c[4], calls[0][4]), 'not repeatable'
            out[cached] = calls[0]
            prob.free()
        a, b = out[True], out[False]
        assert a[:3] == b[:3] and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4]), 'cache_a changes bits'
        try:                                                         # gpk_i_potrf of the order-1027 matrix on the two-partition pipeline
            _set(ctx, {42: 1, 19: 1024, 20: 100000})
            prob = _problem(ctx, 'darcy', cs, dinv=256, cache_a=True)
            bad += _gate_call('fused darcy', f'darcy nc {cs.nz + 1} pipelined gpk_i_potrf', W, _direction(ctx, prob, z))
            prob.free()
        finally:
            _reset(ctx)
    finally:
        sub.free(); z.free()
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ d. Gram-level mode
def _gram_extra(kind, cs, prob, W):
    """rows -> the scale the Gram-level mode adds (module docstring, d.)"""
    nz = cs.nz
    G = prob.G.download()
    col = _column_order(kind, cs.Nd)
    z = cs.z0.astype(LD)
    absl = lambda v: np.abs(np.asarray(v, dtype=np.float64)).astype(LD)
    if kind == 'elliptic':
        p0, p1 = LD(cs.p0), LD(cs.p1)
        dcol, acol, zcol = np.zeros(nz, dtype=LD), np.zeros(nz, dtype=LD), np.zeros(nz, dtype=LD)
        dcol[col], acol[col], zcol[col] = p0 * p1 * z ** (p1 - 1), p0 * z ** p1, z
        pv = absl(prob.pvec.download())
        g11, g12, g21, g22 = (absl(G[k * nz:(k + 1) * nz]) for k in range(4))
        q1 = pv[:nz] + g11 @ np.abs(acol) + g12 @ np.abs(zcol)
        q2 = pv[nz:2 * nz] + g21 @ np.abs(acol) + g22 @ np.abs(zcol)
        corner = pv[2 * nz] + np.abs(acol) @ (pv[:nz] + q1) + np.abs(zcol) @ (pv[nz:2 * nz] + q2)
        border = np.concatenate([np.abs(dcol) * q1 + q2, [corner]])
    else:                                                            # Eikonal: v0 columns 0, the others 2 v / eps
        v = np.where(np.arange(nz) < cs.Nd, LD(0), LD(2) * z / LD(cs.p0))
        dcol = np.zeros(nz, dtype=LD)
        dcol[col] = v
        w = np.abs(W[:, nz])
        t1 = np.abs(prob.W1.download()[:, :nz]).T @ w
        t2 = np.abs(prob.W2.download()[:, :nz]).T @ w
        border = np.concatenate([np.abs(dcol) * t1.astype(LD) + t2.astype(LD), [LD(0)]])
    return lambda rows: FP.gram_scale_rows(G, dcol, rows, border)


GRAM = [('elliptic', 257), ('elliptic', 513), ('elliptic', 1025), ('eikonal', 342)]


@pytest.mark.parametrize('kind,Nd', GRAM)
def test_gram_level_mode(dev_ctx, kind, Nd):
    ctx, cs = dev_ctx, _case(kind, Nd)
    z = ctx.array(cs.z0)
    sub = _problem(ctx, kind, cs, dinv=False)
    prob = _problem(ctx, kind, cs, dinv=256, structured=2)
    print()
    try:
        mode, product = C.c_int(), C.c_int()
        ctx._chk(ctx.lib.gpk_debug_step_mode(ctx.h, C.byref(prob.struct), C.byref(mode), C.byref(product)))
        assert mode.value in (2, 4) and product.value == 0, 'not the Gram-level mode'
        _direction(ctx, sub, z)
        W = _operand(ctx, kind, cs, sub, z)
        calls = [_direction(ctx, prob, z) for _ in range(3)]
        bad = _gate_call('fused gram', f'{kind} n_z {cs.nz}', W, calls[0], extra=_gram_extra(kind, cs, prob, W))
        assert calls[0][0] == ctx.gn_loss(prob, z), 'the reported loss is not gpk_gn_loss'
        for c in calls[1:]:
            assert c[:3] == calls[0][:3] and np.array_equal(c[3], calls[0][3]) and np.array_equal(c[4], calls[0][4]), 'not repeatable'
    finally:
        prob.free(); sub.free(); z.free()
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ e. forms whose W is not observable
_VREF = {}


def _vector_reference(kind, Nd):
    if kind == 'semilinear':
        import _semilinear_reference as SL
        return SL.vector_reference(Nd, FP.NB_FUSED)
    if kind == 'monge_ampere':
        import _monge_ampere_reference as MA
        return MA.vector_reference(Nd, FP.NB_FUSED)
    cs = _case(kind, Nd)
    if Nd in R.NB:                                                   # (the case of test_gpu_gn_rounding.py: its cached reference)
        return R.vector_reference(kind, Nd)
    if (kind, Nd) not in _VREF:
        _VREF[(kind, Nd)] = R.VectorReference(cs, cs.z0)
    return _VREF[(kind, Nd)]


VECTOR = ([(k, n, dict(dinv=256)) for k, n in SUBSTITUTION if k in R.SYSTEMS] + [('darcy', 171, dict(dinv=256))]
          + [('elliptic', 513, dict(dinv=256, structured=1)), ('elliptic', 1025, dict(dinv=256, structured=1))]
          # the two systems that reach Eikonal's kernels through step_layout / step_profile (csrc/gpk_gn.hip), at the smallest pipelined
          # size, n_c = 1027: Semilinear must keep the closed form there, Monge-Ampere runs the two-segment profile
          + [(k, 342, dict(dinv=b)) for k in ('semilinear', 'monge_ampere') for b in (256, 512)])


@pytest.mark.parametrize('kind,Nd,form', VECTOR, ids=lambda v: '-'.join(f'{k}={x}' for k, x in v.items()) if isinstance(v, dict) else str(v))
def test_forms_with_the_solved_block_in_the_workspace(dev_ctx, kind, Nd, form):
    ctx = dev_ctx
    ref = _vector_reference(kind, Nd)
    cs = ref.case
    prob = _problem(ctx, kind, cs, **form)
    z = ctx.array(cs.z0)
    print()
    try:
        if form.get('structured'):
            mode, product = C.c_int(), C.c_int()
            ctx._chk(ctx.lib.gpk_debug_step_mode(ctx.h, C.byref(prob.struct), C.byref(mode), C.byref(product)))
            assert mode.value == 1, 'not the structured level 1 of the elliptic system'
        loss, info = ctx.gn_step(prob, z, 0.5)
        delta, z_out = prob.workspace()[2].download().copy(), z.download().copy()
        if kind in ('semilinear', 'monge_ampere'):                   # repeat bits on one handle
            for _ in range(2):
                z.upload(cs.z0)
                again = ctx.gn_step(prob, z, 0.5)
                assert again == (loss, info) and np.array_equal(prob.workspace()[2].download(), delta) \
                    and np.array_equal(z.download(), z_out), 'not repeatable'
        if kind != 'darcy' and cs.nz + 1 >= 1025:
            assert _pipelined_step(ctx, prob, cs.z0), NO_STREAMS
    finally:
        prob.free(); z.free()
    bad = [f'info = {info}'] if info != 0 else []
    what = f'{kind} n_z {cs.nz} {form}'
    for name, (r, a) in (('loss', R.gate_loss(ref, loss)), ('backward', R.gate_backward_vec(ref, delta)), ('forward', R.gate_forward(ref, delta))):
        _note(f'fused vector {name}', r, a, what)
        if not r <= a:
            bad.append(f'{name}: {r:.4g} > {a:.4g}')
    u, ua = R.gate_update(cs.z0, 0.5, delta, z_out)
    if not u <= ua:
        bad.append(f'update of z: {u:.4g} roundings')
    assert not bad, bad
