"""The long-double reference of one Gauss-Newton step (tests/_gn_reference.py) against the float64 oracle, its vector-only form against
its full form, and NEGATIVE CONTROLS: every gate the helper offers for a device result (entries of [A | F], H, g, loss, delta backward
and forward, update of z) must reject an error of 1e-11 -- a thousand times below what the trajectory tests can see -- on the CPU,
where the float64 numpy pipeline stands in for the device."""
import numpy as np
import pytest

import _gn_reference as R
from oracle import gp_oracle as O

LD, EPS = R.LD, R.EPS
CASES = [(s, Nd) for s in R.SYSTEMS for Nd in (65, 129)]
TINY = 1e-11                                     # the error every gate must reject


def _rel(a, b, scale):
    return float(np.max(np.abs(np.asarray(a, dtype=LD) - np.asarray(b, dtype=LD))) / scale)


@pytest.mark.parametrize('system,Nd', CASES)
def test_reference_agrees_with_the_oracle(system, Nd):
    """H, g, loss of the helper against O.gn_quantities / O.loss to 1e-13 of their scale; delta against one step of O.gn_method to
    100 cond(H) eps (the float64 pipeline deviates by 5e-16 .. 1.4e-13 from long double on these inputs)."""
    cs, ref = R.case(system, Nd), R.full_reference(system, Nd)
    sysm, Ls = cs.oracle()
    H, g = O.gn_quantities(sysm, Ls, cs.z0)
    assert _rel(H, ref.H, float(np.max(np.abs(H)))) <= 1e-13
    assert _rel(g, ref.g, float(np.max(np.abs(g)))) <= 1e-13
    loss = O.loss(sysm, Ls, cs.z0)
    assert abs(LD(loss) - ref.loss) <= 1e-13 * loss
    sol, hist = O.gn_method(sysm, Ls, cs.z0, 1, 1)
    assert abs(LD(hist[0]) - ref.loss) <= 1e-13 * loss
    delta = cs.z0 - sol
    dn = float(np.linalg.norm(ref.delta.astype(np.float64)))
    dev = float(np.linalg.norm((delta.astype(LD) - ref.delta).astype(np.float64))) / dn
    print(f'\n[{system} {Nd}] cond(H) = {ref.cond:.1e}, |delta_oracle - delta_ld| / |delta_ld| = {dev:.1e}')
    assert dev <= 100 * ref.cond * EPS
    # the refinement converged: the long-double residual of delta is at the long-double rounding level
    res = (ref.H @ ref.delta - ref.g).astype(np.float64)
    assert np.linalg.norm(res) <= 1e-3 * EPS * (ref.normH * dn + np.linalg.norm(ref.g.astype(np.float64)))


@pytest.mark.parametrize('Nd', (65, 129, 333))
def test_relaxed_penalty_keeps_the_step_determined(Nd):
    cs = R.case('relaxed', Nd)
    ev = np.linalg.eigvalsh(R.Pipeline64(cs, cs.z0).H)
    assert ev[-1] / ev[0] < 1e4, (R.RELAXED_LAMBDA, ev[-1] / ev[0])


@pytest.mark.parametrize('system,Nd', [('elliptic', 1100), ('relaxed', 333), ('burgers', 333), ('eikonal', 333), ('darcy', 333)])
def test_vector_form_at_the_variant_sizes(system, Nd):
    """the sizes of the schedule-variant test, too large for the full form: the refined delta leaves a long-double residual at the
    long-double rounding level, the float64 pipeline passes every gate and a delta moved by 1e-11 does not"""
    vec = R.vector_reference(system, Nd)
    d = vec.delta
    scale = vec.normH * float(np.linalg.norm(d.astype(np.float64))) + float(np.linalg.norm(vec.g.astype(np.float64)))
    assert np.linalg.norm(vec.residual(d).astype(np.float64)) <= 1e-3 * EPS * scale
    p = vec.p64
    assert not _rejects(R.gate_loss, vec, p.loss) and not _rejects(R.gate_backward_vec, vec, p.delta) and not _rejects(R.gate_forward, vec, p.delta)
    u = np.random.RandomState(Nd).normal(size=vec.case.nz); u /= np.linalg.norm(u)
    bad = p.delta + TINY * np.linalg.norm(p.delta) * u
    assert _rejects(R.gate_forward, vec, bad) and _rejects(R.gate_backward_vec, vec, bad)
    assert _rejects(R.gate_loss, vec, p.loss * (1.0 + TINY))


@pytest.mark.parametrize('system,Nd', CASES)
def test_vector_form_agrees_with_the_full_form(system, Nd):
    """loss, g, delta and the normal-equations residual r(d) = 2 A^T L^-T L^-1 (A d - F) of the vector-only form against H d - g of the
    full form, at delta_ld and at a random d: two long-double evaluations in different orders, within 0.05 eps of the scale"""
    ref, vec = R.full_reference(system, Nd), R.vector_reference(system, Nd)
    gn = float(np.linalg.norm(ref.g.astype(np.float64)))
    assert abs(vec.loss - ref.loss) <= 0.05 * EPS * ref.loss
    assert np.linalg.norm((vec.g - ref.g).astype(np.float64)) <= 0.05 * EPS * gn
    assert 0.5 * ref.normH <= vec.normH <= 1.001 * ref.normH              # (the power iteration is a scale)
    rng = np.random.RandomState(Nd)
    for d in (ref.delta, rng.normal(size=ref.case.nz).astype(LD)):
        scale = ref.normH * float(np.linalg.norm(d.astype(np.float64))) + gn
        diff = (vec.residual(d) - (ref.H @ d - ref.g)).astype(np.float64)
        assert np.linalg.norm(diff) <= 0.05 * EPS * scale
        assert np.linalg.norm((vec.apply_H(d) - ref.H @ d).astype(np.float64)) <= 0.05 * EPS * scale
    dn = float(np.linalg.norm(ref.delta.astype(np.float64)))
    assert np.linalg.norm((vec.delta - ref.delta).astype(np.float64)) <= 0.05 * EPS * ref.cond * dn


def _rejects(gate, *args):
    ratio, allowed = gate(*args)
    return ratio > allowed


@pytest.mark.parametrize('form', ['full', 'vector'])
@pytest.mark.parametrize('system,Nd', CASES)
def test_gates_reject_an_error_of_1e_11(system, Nd, form):
    """Negative controls.  The float64 numpy pipeline passes every gate (by construction); the same values moved by 1e-11 do not:
    delta moved by 1e-11 ||delta|| in a random direction (forward and backward gate), a loss off by 1e-11 relative, an entry of H and
    of g off by 1e-11 of its magnitude bound, an entry of [A | F] off by 1e-11 relative, and an update with step 1.0 instead of 0.5."""
    cs = R.case(system, Nd)
    ref = R.full_reference(system, Nd) if form == 'full' else R.vector_reference(system, Nd)
    backward = R.gate_backward if form == 'full' else R.gate_backward_vec
    p = ref.p64
    rng = np.random.RandomState(7 * Nd)
    # delta
    assert not _rejects(R.gate_forward, ref, p.delta) and not _rejects(backward, ref, p.delta)
    u = rng.normal(size=cs.nz); u /= np.linalg.norm(u)
    bad = p.delta + TINY * np.linalg.norm(p.delta) * u
    assert _rejects(R.gate_forward, ref, bad), R.gate_forward(ref, bad)
    assert _rejects(backward, ref, bad), backward(ref, bad)
    # loss
    assert not _rejects(R.gate_loss, ref, p.loss)
    for sgn in (1.0, -1.0):
        assert _rejects(R.gate_loss, ref, p.loss * (1.0 + sgn * TINY))
    # update of z
    z_out = cs.z0 - 0.5 * p.delta
    assert not _rejects(R.gate_update, cs.z0, 0.5, p.delta, z_out)
    assert _rejects(R.gate_update, cs.z0, 0.5, p.delta, cs.z0 - 1.0 * p.delta)
    assert _rejects(R.gate_update, cs.z0, 0.5, p.delta, z_out * (1.0 + TINY))
    if form == 'vector':
        return
    # H and g, entry by entry
    assert not _rejects(R.gate_H, ref, p.H) and not _rejects(R.gate_g, ref, p.g)
    for _ in range(4):
        i, j = rng.randint(cs.nz, size=2)
        Hb = p.H.copy(); Hb[i, j] += TINY * ref.scaleH[i, j]
        assert _rejects(R.gate_H, ref, Hb), (i, j)
        gb = p.g.copy(); gb[i] -= TINY * ref.scaleg[i]
        assert _rejects(R.gate_g, ref, gb), i
    # [A | F]: the float64 evaluation of the same expressions passes, an entry moved by 1e-11 does not, nor does a lost constant
    lin = ref.lin
    A, F = lin.dense(np.float64), lin.F.astype(np.float64)
    assert R.check_build(lin, A, F) <= 0.5
    k = int(np.nonzero(~lin.const)[0][rng.randint(np.count_nonzero(~lin.const))])
    Ab = A.copy(); Ab[lin.r[k], lin.c[k]] *= 1.0 + TINY
    with pytest.raises(AssertionError):
        R.check_build(lin, Ab, F)
    k = int(np.nonzero(~lin.Fcopy)[0][0])
    Fb = F.copy(); Fb[k] += TINY * float(lin.Fmag[k])
    with pytest.raises(AssertionError):
        R.check_build(lin, A, Fb)
    k = int(np.nonzero(lin.const)[0][0])
    Ab = A.copy(); Ab[lin.r[k], lin.c[k]] = 0.0
    with pytest.raises(AssertionError):
        R.check_build(lin, Ab, F)
    pattern = np.zeros(A.shape, dtype=bool); pattern[lin.r, lin.c] = True
    outside = np.argwhere(~pattern)
    i, j = outside[rng.randint(len(outside))]                        # a structural zero: any non-zero there is rejected
    Ab = A.copy(); Ab[i, j] = 1e-300
    with pytest.raises(AssertionError):
        R.check_build(lin, Ab, F)


def test_poisoned_factor_layout():
    L = R.case('elliptic', 65).L
    P = R.poisoned(L)
    n = L.shape[0]
    assert P.shape == (n, n + R.LD_PAD) and np.array_equal(np.tril(P[:, :n]), L)
    assert np.all(P[:, :n][np.triu_indices(n, 1)] == R.POISON) and np.all(P[:, n:] == R.POISON)
