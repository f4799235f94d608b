"""One Gauss-Newton step of every system to rounding, against a long-double reference (tests/_gn_reference.py).

The trajectory tests (test_gpu_parity / _structured / _variants / _fullsize_oracle / _end_to_end_oracle) run on Gram factors with a
nugget of 1e-9 .. 1e-13, whose conditioning forces gates of 1e-5 .. 1e-9: they guard the ill-conditioned regime.  This file guards
the ARITHMETIC.  The factors are synthetic and well conditioned (tril(normal) + diag(uniform(3, 4) sqrt(n)), strict upper triangle and
the padding of the ld = n + 16 buffer poisoned with 1e30), so that [A(z) | F(z)], H, g, the loss, delta and the update are determined to
rounding; the relaxed system runs at the penalty lambda = 100 (cond(H) < 1e4, see _gn_reference.RELAXED_LAMBDA).  Every gate is shown
to reject an error of 1e-11 in tests/test_gn_reference_host.py.

  a. gpk_gn_build / gpk_gn_build_rev / gpk_gn_measurement entry by entry: zeros, constants and copies exact, the rest within
     C_BUILD = 5 eps of the magnitude sum of its terms (budget derived in _gn_reference.py: the largest entry costs 9/2 eps).
  b. gpk_gn_hessian_grad: H exactly symmetric, |H - H_ld| <= C eps 2 |S|^T |S| and |g - g_ld| <= C eps 2 |S|^T |w| entry by entry.
  c. gpk_gn_step, two consecutive calls on one handle (steps 1.0 and 0.5; the reference of the second call is recomputed at the
     device's own z): info, the in-step loss, delta backward and forward, the update of z, bit-identical repeat on a fresh handle; for
     every problem form of GNProblem (dinv on / off, structured False / 1 / 2, Darcy cache_a on / off, these two bit-identical).
     The loss chain of the step runs on the handle's side stream in BOTH calls: the CU-masked streams are created with the handle.
  d. the step under every schedule variant of test_gpu_variants.VARIANTS at a size where variants are active, against the vector-only
     long-double reference (agreement between variants is not enough).

C is never fixed in advance: the same figure of the float64 numpy pipeline (scipy triangular solves, BLAS products, LAPACK Cholesky)
is computed at run time and the device may take 32 x that + 1 (_gn_reference.allowed).  Every test prints both.

Which variants are active in d (csrc/gpk_gn.hip, gpk_factor.hip, gpk_gemm.hip):
  elliptic (1100, 160): order 2360, n_z + 1 = 1101 = 3 blocks of 512 columns -> the step runs gpk_i_syrk_potrf on the two-partition
    pipeline, so the pipeline keys (12, 13, 17, 18, 24, 26, 28, 29, 34) are active, as are the solve keys (3, 10), the tile keys (0, 33,
    38, 35, 36), 16 and 6 (leading-zero products), 4 (TRSV blocks) and 41 (panel kernel).  Not active: 20 (it switches gpk_i_potrf onto the pipeline
    for orders >= 2048 only, and the step's own phase is pipelined already).
  Burgers, Eikonal (N_d = 333): n_z + 1 = 1000 < 1025 -> gpk_i_syrk_potrf takes the one-stream product + factorisation: the pipeline
    keys 12, 13, 17, 18, 24, 26, 28, 29, 34 and 20 (order 1000 < 2048) are NOT active; the solve, tile, leading-zero, TRSV and panel keys are.
  relaxed (N_d = 333): n_z + 1 = 667: as Burgers.
  Darcy (N_d = 333): the leading-zero layout forms H by its own launches and calls gpk_i_potrf: the pipeline keys of the fused phase are
    NOT active, nor is 20 (n_z + 1 = 1999 < 2048); key 10 = 0 additionally switches the layout to the dense schedule (step_layout needs the inverted blocks).
Variants that are not active at a size run the default schedule there; they are run all the same (cheap) but do not count as coverage.

Budgets: C_BUILD = 5 (derived: 9/2 for the relaxed system's F entry, device pow / exp / sqrt taken at 1 ulp -- unmeasured, so the [build]
lines below are the first measurement of it); every other constant is 32 x numpy + 1 at run time.

RESULTS: every test prints its ratios under the tags [build], [H], [g], [step loss / backward / forward / update] and [variants ...],
each with the worst so far.  Worst ratios of a run on an MI355X, as "tag: device ratio of allowed":
  build 1.37 of C_BUILD = 5;  H 536 of 4.64e+03;  g 11.3 of 41.9;  step loss 0.991 of 33;  step backward 1.82 of 15.5;
  step forward 7.84 of 109;  step update and variants update 0.500 of 1;  variants loss 0.539 of 33;  variants backward 1.04 of 8.62;
  variants forward 12.4 of 124 (numpy figure = (allowed - 1) / 32).
"""
import ctypes as C

import numpy as np
import pytest

import _gn_reference as R
import _staircase_model as M
from test_gpu_variants import DEFAULTS, VARIANTS

pytestmark = pytest.mark.gpu

LD, EPS = R.LD, R.EPS
SIZES = (65, 129)
CASES = [(s, Nd) for s in R.SYSTEMS for Nd in SIZES]
WORST = {}


def _note(tag, ratio, allowed, what):
    w = WORST.setdefault(tag, (0.0, 0.0, allowed))
    if not ratio / allowed < w[0]:
        WORST[tag] = (ratio / allowed, ratio, allowed)
    print(f'[{tag}] {what}: device {ratio:.3g}, allowed {allowed:.3g} (numpy {(allowed - 1.0) / R.MARGIN:.3g}); '
          f'worst so far {WORST[tag][1]:.3g} of {WORST[tag][2]:.3g}')


def _upload_factor(ctx, L):
    n = L.shape[0]
    d = ctx.empty(n, n + R.LD_PAD, ld=n + R.LD_PAD)
    d.upload(R.poisoned(L))
    d.cols = n
    return d


def _problem(ctx, cs, dinv=256, structured=False, cache_a=False):
    import gpk
    L = _upload_factor(ctx, cs.L)
    L2 = _upload_factor(ctx, cs.L2) if cs.L2 is not None else None
    prob = gpk.GNProblem(ctx, R.SYSTEM_NAME[cs.system], cs.Nd, cs.Nb, cs.f, cs.g, L, p0=cs.p0, p1=cs.p1, pen_lambda=cs.lam,
                         data_u=cs.data, L2=L2, dinv=dinv, structured=structured, cache_a=cache_a)
    prob.keep += [L] + ([L2] if L2 is not None else [])
    return prob


# ------------------------------------------------------------------------------------------------ a. linearisation values
@pytest.mark.parametrize('system,Nd', CASES)
def test_build_values(dev_ctx, system, Nd):
    ctx, cs = dev_ctx, R.case(system, Nd)
    lin = R.full_reference(system, Nd).lin
    prob = _problem(ctx, cs)
    z = ctx.array(cs.z0)
    nz = cs.nz
    S = ctx.empty(prob.rows, nz + 1)
    ctx._chk(ctx.lib.gpk_gn_build(ctx.h, C.byref(prob.struct), z.ptr, S.ptr, S.ld))
    nat = S.download()
    worst = R.check_build(lin, nat[:, :nz], nat[:, nz], (system, Nd, 'gpk_gn_build'))
    col = M.column_of_unknown(system, Nd)
    if system == 'relaxed':                       # gpk_gn_build_rev refuses it; the step runs the natural build in the slope-1 layout
        perm = np.zeros_like(nat[:, :nz])
        perm[:, col] = nat[:, :nz]
        assert np.array_equal(M.first_nonzero_rows(perm), M.promised_profile('relaxed', Nd, cs.Nb))
    else:
        S.upload(np.full((prob.rows, nz + 1), 3.25))
        ctx._chk(ctx.lib.gpk_gn_build_rev(ctx.h, C.byref(prob.struct), z.ptr, S.ptr, S.ld))
        rev = S.download()
        worst = max(worst, R.check_build(lin, rev[:, col], rev[:, nz], (system, Nd, 'gpk_gn_build_rev')))
    worst = max(worst, R.check_build(lin, None, ctx.gn_measurement(prob, z), (system, Nd, 'gpk_gn_measurement')))
    WORST['build'] = max(WORST.get('build', 0.0), worst)
    print(f'\n[build {system} {Nd}] worst |dev - ld| / (eps sum|terms|) = {worst:.2f} of C_BUILD = {R.C_BUILD}; worst so far {WORST["build"]:.2f}')
    prob.free()


# ------------------------------------------------------------------------------------------------ b. H and g
@pytest.mark.parametrize('dinv', [256, False], ids=['dinv', 'substitution'])
@pytest.mark.parametrize('system,Nd', CASES)
def test_hessian_grad(dev_ctx, system, Nd, dinv):
    ctx, cs = dev_ctx, R.case(system, Nd)
    ref = R.full_reference(system, Nd)
    prob = _problem(ctx, cs, dinv=dinv)
    H, g = ctx.gn_hessian_grad(prob, ctx.array(cs.z0))
    print()
    rH, aH = R.gate_H(ref, H)
    _note('H', rH, aH, f'{system} {Nd} dinv={dinv} max |H - H_ld| / (eps 2|S|^T|S|)')
    rg, ag = R.gate_g(ref, g)
    _note('g', rg, ag, f'{system} {Nd} dinv={dinv} max |g - g_ld| / (eps 2|S|^T|w|)')
    prob.free()
    assert np.array_equal(H, H.T), 'H is not exactly symmetric'
    assert rH <= aH and rg <= ag


# ------------------------------------------------------------------------------------------------ c. the step
def _forms(system):
    base = [dict(dinv=256), dict(dinv=False)]
    if system == 'relaxed':
        return base
    extra = [dict(dinv=256, structured=1), dict(dinv=256, structured=2)]
    if system == 'darcy':
        return base + [dict(dinv=256, cache_a=True)] + extra
    return base + extra


STEP_CASES = [(s, Nd, f) for s, Nd in CASES for f in _forms(s)]
STEPS = (1.0, 0.5)


def _two_steps(ctx, cs, form, z0):
    """two consecutive gpk_gn_step calls on ctx: [(z_in, step, loss, info, delta, z_out)]"""
    prob = _problem(ctx, cs, **form)
    z = ctx.array(z0)
    out = []
    for step in STEPS:
        z_in = z.download().copy()
        loss, info = ctx.gn_step(prob, z, step)
        out.append((z_in, step, loss, info, prob.workspace()[2].download().copy(), z.download().copy()))
    prob.free()
    return out


def _check_step(tag, what, ref, call):
    """the gates of one call against the (vector-only) reference at its z_in; returns the failures"""
    z_in, step, loss, info, delta, z_out = call
    assert np.array_equal(ref.z, z_in)
    bad = []
    if info != 0:
        bad.append(f'info = {info}')
    for name, (r, a) in (('loss', R.gate_loss(ref, loss)), ('backward', R.gate_backward_vec(ref, delta)),
                         ('forward', R.gate_forward(ref, delta))):
        _note(f'{tag} {name}', r, a, what)
        if not r <= a:
            bad.append(f'{name}: {r:.4g} > {a:.4g}')
    u, ua = R.gate_update(z_in, step, delta, z_out)
    WORST[f'{tag} update'] = max(WORST.get(f'{tag} update', 0.0), u)
    print(f'[{tag} update] {what}: {u:.3f} of {ua:g}')
    if not u <= ua:
        bad.append(f'update of z: {u:.4g} roundings')
    return bad


@pytest.mark.parametrize('system,Nd,form', STEP_CASES, ids=lambda v: '-'.join(f'{k}={x}' for k, x in v.items()) if isinstance(v, dict) else str(v))
def test_step(dev_ctx, system, Nd, form):
    import gpk
    ctx, cs = dev_ctx, R.case(system, Nd)
    calls = _two_steps(ctx, cs, form, cs.z0)
    print()
    bad = []
    for k, call in enumerate(calls):
        ref = R.vector_reference(system, Nd) if k == 0 else R.VectorReference(cs, call[0])
        bad += [f'call {k + 1}: {b}' for b in _check_step('step', f'{system} {Nd} {form} call {k + 1}', ref, call)]
    assert not bad, bad
    # the same two calls from the same start on a fresh handle: bit for bit
    fresh = gpk.Context(0, dev=True)
    try:
        again = _two_steps(fresh, cs, form, cs.z0)
        if form.get('cache_a'):                                      # Darcy: the cached a-part changes no bit either
            uncached = _two_steps(fresh, cs, dict(form, cache_a=False), cs.z0)
    finally:
        fresh.close()
    for a, b in zip(calls, again):
        assert a[2] == b[2] and a[3] == b[3] and np.array_equal(a[4], b[4]) and np.array_equal(a[5], b[5]), 'not reproducible'
    if form.get('cache_a'):
        for a, b in zip(calls, uncached):
            assert a[2] == b[2] and a[3] == b[3] and np.array_equal(a[4], b[4]) and np.array_equal(a[5], b[5]), 'cache_a changes bits'


# ------------------------------------------------------------------------------------------------ d. schedule variants
VARIANT_CASES = [('elliptic', 1100), ('relaxed', 333), ('burgers', 333), ('eikonal', 333), ('darcy', 333)]


@pytest.mark.parametrize('system,Nd', VARIANT_CASES)
def test_step_under_every_schedule_variant(dev_ctx, system, Nd):
    """one gpk_gn_step (step 0.5) from the shared start under every entry of test_gpu_variants.VARIANTS, each against the vector-only
    long-double reference: info, loss, normal-equations residual of delta, delta itself, update of z (the module docstring names the
    variants that are active at these sizes)"""
    ctx, cs = dev_ctx, R.case(system, Nd)
    ref = R.vector_reference(system, Nd)
    bad = []
    print()
    try:
        for name, variant in VARIANTS:
            for k, v in DEFAULTS.items():
                ctx.lib.gpk_debug_set(k, v)
            for k, v in variant.items():
                ctx.lib.gpk_debug_set(k, v)
            prob = _problem(ctx, cs, dinv=True)
            z = ctx.array(cs.z0)
            loss, info = ctx.gn_step(prob, z, 0.5)
            call = (cs.z0, 0.5, loss, info, prob.workspace()[2].download().copy(), z.download().copy())
            prob.free(); z.free()
            bad += [f'{name}: {b}' for b in _check_step('variants', f'{system} {Nd} {name}', ref, call)]
    finally:
        for k, v in DEFAULTS.items():
            ctx.lib.gpk_debug_set(k, v)
    assert not bad, bad
