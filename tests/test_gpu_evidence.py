"""Log evidence on the device: gpk_chol_logdet, gpk_log_evidence, the class API and solver_GP.select_kernel_parameter.

  a  the log-determinant reduction against long double, judged by what 2 np.sum(np.log(diag)) achieves on the same data; the same bits
     on a repeat, on a fresh handle and on an odd-offset view between canaries; the count of bad pivots; the -9001 cases
  b  the six terms of gpk_log_evidence on the synthetic, well-conditioned factors of tests/_gn_reference.py against long double, each
     judged by the float64 numpy pipeline (tests/_evidence_reference.py) measured in the same test; P and R bit for bit those of
     gpk_posterior_prepare
  c  the affine identity on real Gram matrices through the class API: with alpha = 0 the evidence is the Gaussian log likelihood of the
     data rows under their own block of Theta (Dirichlet, Robin, three dimensions)
  d  the nonlinear case of every system at the sizes of test_gpu_posterior.REAL: the long-double formula at the device's own final
     iterate on the oracle's Theta
  e  selection: the table against a CPU run with the oracle, refinement, failed candidates, posterior_variance afterwards, the drivers

No gate is a constant: the device may take R.MARGIN = 32 times what the float64 numpy pipeline takes on the same inputs against long
double (b, d, e: plus one eps, and the numpy figure of a single number counted as at least one eps, as _gn_reference.gate_loss does:
the rounding error of one number can vanish by cancellation).  Units in a, b, d, e: eps x the sum of the magnitudes of the summands.
Every gate has a precondition, asserted in front of it: what the float64 numpy pipeline itself loses on the same inputs (counted as at
least one eps) stays below PRECONDITION = 1e-9 of the value -- the figure the issue sets for the affine case -- so that MARGIN times it
is still a result nobody would call wrong.  Every figure is printed under an [evidence] tag.

RESULTS
  The [evidence] lines of a run on an MI355X (gfx950), every test of this file passing:
    [evidence] chol_logdet n 1: device 0.401, allowed 33
    [evidence] chol_logdet n 63: device 0.095, allowed 33
    [evidence] chol_logdet n 257: device 0.177, allowed 33
    [evidence] chol_logdet n 2049: device 0.0128, allowed 33
    [evidence] log_Z elliptic 65 dinv 256: device 0.325, allowed 33
    [evidence] J elliptic 65 dinv 256: device 0.565, allowed 35.4
    [evidence] logdet_theta elliptic 65 dinv 256: device 0.416, allowed 33
    [evidence] logdet_H elliptic 65 dinv 256: device 0.378, allowed 33
    [evidence] gamma_term elliptic 65 dinv 256: device 0, allowed 33
    [evidence] two_pi_term elliptic 65 dinv 256: device 0.075, allowed 33
    [evidence] log_Z elliptic 65 dinv False: device 0.325, allowed 33
    [evidence] J elliptic 65 dinv False: device 0.565, allowed 35.4
    [evidence] logdet_theta elliptic 65 dinv False: device 0.416, allowed 33
    [evidence] logdet_H elliptic 65 dinv False: device 0.264, allowed 33
    [evidence] gamma_term elliptic 65 dinv False: device 0, allowed 33
    [evidence] two_pi_term elliptic 65 dinv False: device 0.075, allowed 33
    [evidence] log_Z elliptic 129 dinv 256: device 0.315, allowed 33
    [evidence] J elliptic 129 dinv 256: device 0.63, allowed 33
    [evidence] logdet_theta elliptic 129 dinv 256: device 0.433, allowed 33
    [evidence] logdet_H elliptic 129 dinv 256: device 0.24, allowed 33
    [evidence] gamma_term elliptic 129 dinv 256: device 0, allowed 33
    [evidence] two_pi_term elliptic 129 dinv 256: device 0.156, allowed 33
    [evidence] log_Z elliptic 129 dinv False: device 0.315, allowed 33
    [evidence] J elliptic 129 dinv False: device 0.63, allowed 33
    [evidence] logdet_theta elliptic 129 dinv False: device 0.433, allowed 33
    [evidence] logdet_H elliptic 129 dinv False: device 0.24, allowed 33
    [evidence] gamma_term elliptic 129 dinv False: device 0, allowed 33
    [evidence] two_pi_term elliptic 129 dinv False: device 0.156, allowed 33
    [evidence] log_Z burgers 65 dinv 256: device 0.0877, allowed 33
    [evidence] J burgers 65 dinv 256: device 0.171, allowed 33
    [evidence] logdet_theta burgers 65 dinv 256: device 0.439, allowed 33
    [evidence] logdet_H burgers 65 dinv 256: device 0.174, allowed 33
    [evidence] gamma_term burgers 65 dinv 256: device 0, allowed 33
    [evidence] two_pi_term burgers 65 dinv 256: device 0.075, allowed 33
    [evidence] log_Z burgers 65 dinv False: device 0.0877, allowed 33
    [evidence] J burgers 65 dinv False: device 0.171, allowed 33
    [evidence] logdet_theta burgers 65 dinv False: device 0.439, allowed 33
    [evidence] logdet_H burgers 65 dinv False: device 0.174, allowed 33
    [evidence] gamma_term burgers 65 dinv False: device 0, allowed 33
    [evidence] two_pi_term burgers 65 dinv False: device 0.075, allowed 33
    [evidence] log_Z burgers 129 dinv 256: device 0.198, allowed 33
    [evidence] J burgers 129 dinv 256: device 0.373, allowed 70.7
    [evidence] logdet_theta burgers 129 dinv 256: device 0.158, allowed 33
    [evidence] logdet_H burgers 129 dinv 256: device 0.384, allowed 33
    [evidence] gamma_term burgers 129 dinv 256: device 0, allowed 33
    [evidence] two_pi_term burgers 129 dinv 256: device 0.156, allowed 33
    [evidence] log_Z burgers 129 dinv False: device 0.0547, allowed 33
    [evidence] J burgers 129 dinv False: device 0.373, allowed 70.7
    [evidence] logdet_theta burgers 129 dinv False: device 0.158, allowed 33
    [evidence] logdet_H burgers 129 dinv False: device 0.232, allowed 33
    [evidence] gamma_term burgers 129 dinv False: device 0, allowed 33
    [evidence] two_pi_term burgers 129 dinv False: device 0.156, allowed 33
    [evidence] log_Z eikonal 65 dinv 256: device 0.75, allowed 89.8
    [evidence] J eikonal 65 dinv 256: device 0.364, allowed 33
    [evidence] logdet_theta eikonal 65 dinv 256: device 0.0144, allowed 33
    [evidence] logdet_H eikonal 65 dinv 256: device 2.38, allowed 271
    [evidence] gamma_term eikonal 65 dinv 256: device 0, allowed 33
    [evidence] two_pi_term eikonal 65 dinv 256: device 0.075, allowed 33
    [evidence] log_Z eikonal 65 dinv False: device 1.04, allowed 89.8
    [evidence] J eikonal 65 dinv False: device 0.364, allowed 33
    [evidence] logdet_theta eikonal 65 dinv False: device 0.0144, allowed 33
    [evidence] logdet_H eikonal 65 dinv False: device 3.25, allowed 271
    [evidence] gamma_term eikonal 65 dinv False: device 0, allowed 33
    [evidence] two_pi_term eikonal 65 dinv False: device 0.075, allowed 33
    [evidence] log_Z eikonal 129 dinv 256: device 0.588, allowed 37.6
    [evidence] J eikonal 129 dinv 256: device 0.639, allowed 33
    [evidence] logdet_theta eikonal 129 dinv 256: device 0.236, allowed 33
    [evidence] logdet_H eikonal 129 dinv 256: device 1.92, allowed 113
    [evidence] gamma_term eikonal 129 dinv 256: device 0, allowed 33
    [evidence] two_pi_term eikonal 129 dinv 256: device 0.156, allowed 33
    [evidence] log_Z eikonal 129 dinv False: device 0.588, allowed 37.6
    [evidence] J eikonal 129 dinv False: device 0.639, allowed 33
    [evidence] logdet_theta eikonal 129 dinv False: device 0.236, allowed 33
    [evidence] logdet_H eikonal 129 dinv False: device 1.92, allowed 113
    [evidence] gamma_term eikonal 129 dinv False: device 0, allowed 33
    [evidence] two_pi_term eikonal 129 dinv False: device 0.156, allowed 33
    [evidence] log_Z darcy 65 dinv 256: device 0.315, allowed 33
    [evidence] J darcy 65 dinv 256: device 0.138, allowed 33
    [evidence] logdet_theta darcy 65 dinv 256: device 0.118, allowed 33
    [evidence] logdet_H darcy 65 dinv 256: device 0.711, allowed 33
    [evidence] gamma_term darcy 65 dinv 256: device 0.126, allowed 33
    [evidence] two_pi_term darcy 65 dinv 256: device 0.201, allowed 33
    [evidence] log_Z darcy 65 dinv False: device 0.315, allowed 33
    [evidence] J darcy 65 dinv False: device 0.138, allowed 33
    [evidence] logdet_theta darcy 65 dinv False: device 0.118, allowed 33
    [evidence] logdet_H darcy 65 dinv False: device 0.711, allowed 33
    [evidence] gamma_term darcy 65 dinv False: device 0.126, allowed 33
    [evidence] two_pi_term darcy 65 dinv False: device 0.201, allowed 33
    [evidence] log_Z darcy 129 dinv 256: device 1.96, allowed 33
    [evidence] J darcy 129 dinv 256: device 1.06, allowed 47.2
    [evidence] logdet_theta darcy 129 dinv 256: device 0.065, allowed 33
    [evidence] logdet_H darcy 129 dinv 256: device 0.0772, allowed 33
    [evidence] gamma_term darcy 129 dinv 256: device 0.214, allowed 33
    [evidence] two_pi_term darcy 129 dinv 256: device 0.0956, allowed 33
    [evidence] log_Z darcy 129 dinv False: device 1.96, allowed 33
    [evidence] J darcy 129 dinv False: device 1.06, allowed 47.2
    [evidence] logdet_theta darcy 129 dinv False: device 0.065, allowed 33
    [evidence] logdet_H darcy 129 dinv False: device 0.0772, allowed 33
    [evidence] gamma_term darcy 129 dinv False: device 0.214, allowed 33
    [evidence] two_pi_term darcy 129 dinv False: device 0.0956, allowed 33
    [evidence] affine dirichlet sigma 0.1: log Z -885.57572596, numpy relative error 3.28e-13, device 2.12e-13, allowed 1.05e-11
    [evidence] affine dirichlet sigma 0.2: log Z -2634.46759342, numpy relative error 4.84e-12, device 5.51e-13, allowed 1.55e-10
    [evidence] affine robin sigma 0.2: log Z -10603.0804412, numpy relative error 6.01e-12, device 3.31e-13, allowed 1.92e-10
    [evidence] affine 3d sigma 0.3: log Z -395.156276393, numpy relative error 1.21e-14, device 5.61e-15, allowed 3.87e-13
    [evidence] real Burgers: log Z -433.097314625 = -(6.00566 + 1119.32 + -556.872) / 2 - 0 - 148.868
    [evidence] log_Z real Burgers: device 306, allowed 3.12e+03
    [evidence] J real Burgers: device 0.026, allowed 33
    [evidence] logdet_theta real Burgers: device 15.1, allowed 2.32e+03
    [evidence] logdet_H real Burgers: device 225, allowed 5.73e+03
    [evidence] gamma_term real Burgers: device 0, allowed 33
    [evidence] two_pi_term real Burgers: device 0.274, allowed 33
    [evidence] real Darcy_flow2d: log Z -134.087663251 = -(3.11551 + -4407.2 + 4654.51) / 2 - -138.155 - 147.03
    [evidence] log_Z real Darcy_flow2d: device 36.3, allowed 1.05e+04
    [evidence] J real Darcy_flow2d: device 2.74e+04, allowed 5.61e+05
    [evidence] logdet_theta real Darcy_flow2d: device 410, allowed 1.48e+04
    [evidence] logdet_H real Darcy_flow2d: device 465, allowed 6.4e+03
    [evidence] gamma_term real Darcy_flow2d: device 0.141, allowed 33
    [evidence] two_pi_term real Darcy_flow2d: device 0.789, allowed 33
    [evidence] real Eikonal: log Z -204.414524054 = -(6.97042 + -3959.02 + 4066.82) / 2 - 0 - 147.03
    [evidence] log_Z real Eikonal: device 2.22e+03, allowed 2.44e+04
    [evidence] J real Eikonal: device 8.13e+04, allowed 1.19e+07
    [evidence] logdet_theta real Eikonal: device 9.81e+03, allowed 2.39e+05
    [evidence] logdet_H real Eikonal: device 5.49e+03, allowed 2.12e+05
    [evidence] gamma_term real Eikonal: device 0, allowed 33
    [evidence] two_pi_term real Eikonal: device 0.789, allowed 33
    [evidence] real Nonlinear_elliptic: log Z -2750.00148479 = -(5153.52 + -2014.47 + 2011.75) / 2 - 0 - 174.598
    [evidence] log_Z real Nonlinear_elliptic: device 4.48e+03, allowed 6.37e+04
    [evidence] J real Nonlinear_elliptic: device 6.21e+03, allowed 1.42e+05
    [evidence] logdet_theta real Nonlinear_elliptic: device 499, allowed 2.72e+05
    [evidence] logdet_H real Nonlinear_elliptic: device 4.59e+03, allowed 4.56e+05
    [evidence] gamma_term real Nonlinear_elliptic: device 0, allowed 33
    [evidence] two_pi_term real Nonlinear_elliptic: device 0.0562, allowed 33
    [evidence] selection sigma 0.08: device log Z -991.536670523, oracle -991.536670523, J 67.518; device 923, allowed 4.28e+04
    [evidence] selection sigma 0.1: device log Z -879.365729276, oracle -879.365729276, J 113.291; device 67.1, allowed 3.47e+03
    [evidence] selection sigma 0.15: device log Z -722.562197576, oracle -722.562197575, J 500.774; device 943, allowed 2.8e+04
    [evidence] selection sigma 0.2: device log Z -2750.00148479, oracle -2750.00148478, J 5153.52; device 4.48e+03, allowed 6.41e+04
    [evidence] selection sigma 0.3: device log Z -2378102.72641, oracle -2378102.72641, J 4.75658e+06; device 1.23e+03, allowed 6.25e+05
    [evidence] selection: oracle argmax sigma 0.15, nearest competitor 156.8 log units below
    [evidence] selection: test L2 error at the winner 0.0142
    [evidence] selection refine 3: sigma 0.141384, log Z -718.965571121 (grid: -722.562197576)
    [evidence] failed candidate: info [(57, None, None), (0, 0, 0)], log Z [np.float64(nan), np.float64(-1180.3931513638304)]
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import _evidence_reference as ER
import _gn_reference as R
import _posterior_reference as PR
import _view_arena as VA
import test_gpu_posterior as TP                       # its problems: _problem, _solve, _real_case, REAL, QUIET (the issue asks for the sizes of REAL)
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'nonlinpdes-gpsolver_amd')
if PKG not in sys.path:
    sys.path.insert(0, PKG)

LD, EPS = R.LD, R.EPS
QUIET = TP.QUIET


PRECONDITION = 1e-9                                # relative error the float64 numpy yardstick may have for a gate to mean something


def _say(what, device, allowed):
    print(f'\n[evidence] {what}: device {device:.3g}, allowed {allowed:.3g}')


def _precondition(what, numpy_ratio, scale, value):
    """numpy_ratio is in units of eps x scale: as a fraction of |value| it must stay below PRECONDITION (a value that is exactly zero has
    scale 0 and is gated for exactness)"""
    if scale == 0:
        return
    rel = EPS * max(numpy_ratio, 1.0) * float(scale) / abs(float(value))
    assert rel < PRECONDITION, f'precondition of {what}: the numpy yardstick is off by {rel:.3g} of the value; the gate could hide a wrong result'


# ------------------------------------------------------------------------------------------------ a. gpk_chol_logdet
PAD = 3


def _factor(n, seed=None):
    """random lower-triangular L, diagonal 10^U(-7, 3), in an n x (n + PAD) buffer whose padding and strict upper triangle are 1e30"""
    rng = np.random.RandomState(n if seed is None else seed)
    L = np.tril(rng.normal(size=(n, n)), -1) + np.diag(10.0 ** rng.uniform(-7, 3, n))
    full = np.full((n, n + PAD), R.POISON)
    full[:, :n] = np.where(np.tri(n, dtype=bool), L, R.POISON)
    return L, full


def _upload(ctx, full, n):
    d = ctx.empty(n, n + PAD, ld=n + PAD)
    d.upload(full)
    d.cols = n
    return d


@pytest.mark.parametrize('n', [1, 63, 257, 2049])
def test_chol_logdet(dev_ctx, n):
    import gpk
    ctx = dev_ctx
    L, full = _factor(n)
    got, bad = ctx.chol_logdet(_upload(ctx, full, n), n)
    assert bad == 0
    t = LD(2) * np.log(np.diag(L).astype(LD))
    ref, scale = np.sum(t), LD(EPS) * np.sum(np.abs(t))
    ratio = lambda x: float(abs(LD(x) - ref) / scale)
    ratio_np = ratio(2.0 * np.sum(np.log(np.diag(L))))
    _precondition(f'chol_logdet n {n}', ratio_np, np.sum(np.abs(t)), ref)
    allowed = ER.allowed_scalar(ratio_np)
    _say(f'chol_logdet n {n}', ratio(got), allowed)
    assert ratio(got) <= allowed                                      # (a leaked 1e30 would add 138 to a sum of magnitude ~10 n)
    again, _ = ctx.chol_logdet(_upload(ctx, full, n), n)
    assert VA.bits(again) == VA.bits(got)
    fresh = gpk.Context(0, dev=True)
    try:
        other, _ = fresh.chol_logdet(_upload(fresh, full, n), n)
    finally:
        fresh.close()
    assert VA.bits(other) == VA.bits(got)
    # an odd base offset and an odd leading dimension between canaries: the same bits, nothing written
    v = VA.class_view(ctx, n, n, 'D')
    v.arena.put(v, full[:, :n])
    value, nbad = C.c_double(), C.c_int()
    ctx._chk(ctx.lib.gpk_chol_logdet(ctx.h, v.ptr, n, v.ld, C.byref(value), C.byref(nbad)))
    v.arena.assert_outside_untouched([])
    assert VA.bits(value.value) == VA.bits(got) and nbad.value == 0
    v.arena.free()


def test_chol_logdet_counts_bad_pivots_and_rejects_bad_arguments(dev_ctx):
    import gpk
    ctx = dev_ctx
    n = 300
    L, full = _factor(n)
    for i, v in ((5, 0.0), (130, -2.0), (299, np.nan)):
        full[i, i] = v
    got, bad = ctx.chol_logdet(_upload(ctx, full, n), n)
    assert bad == 3 and np.isnan(got)
    full[299, 299], full[130, 130] = 1.0, 1.0
    got, bad = ctx.chol_logdet(_upload(ctx, full, n), n)
    assert bad == 1 and got == -np.inf                                 # log 0
    d = _upload(ctx, _factor(8)[1], 8)
    value, nbad = C.c_double(), C.c_int()
    call = lambda *a: ctx._chk(ctx.lib.gpk_chol_logdet(ctx.h, *a))
    for args, word in (((None, 8, d.ld, C.byref(value), C.byref(nbad)), 'pointers'), ((d.ptr, 8, d.ld, None, C.byref(nbad)), 'pointers'),
                       ((d.ptr, 8, d.ld, C.byref(value), None), 'pointers'), ((d.ptr, 0, d.ld, C.byref(value), C.byref(nbad)), 'n <= 0'),
                       ((d.ptr, -1, d.ld, C.byref(value), C.byref(nbad)), 'n <= 0'), ((d.ptr, 8, 7, C.byref(value), C.byref(nbad)), 'ldl < n')):
        with pytest.raises(gpk.GpkError, match='-9001.*' + word):
            call(*args)
    assert ctx.lib.gpk_chol_logdet(None, d.ptr, 8, d.ld, C.byref(value), C.byref(nbad)) == -9001


# ------------------------------------------------------------------------------------------------ b. the six terms, synthetic factors
@functools.lru_cache(maxsize=None)
def _synthetic_reference(system, Nd):
    """per (system, N_d), shared by the dinv variants: the long-double terms (H/2 via full_reference, as the posterior test) and the
    float64 numpy terms"""
    cs = R.case(system, Nd)
    full = R.full_reference(system, Nd)
    prepared = (full.S, PR.cholesky_ld(full.H / LD(2)))
    return ER.terms_ld(cs, cs.z0, prepared=prepared), ER.terms_np64(cs, cs.z0)


def _gate_terms(tag, terms, ld, np64):
    for name in ER.TERMS:
        ratio_np = ER.term_ratio(name, np64.value[name], ld)
        _precondition(f'{name} {tag}', ratio_np, ld.scale[name], ld.value[name])
        ratio, allowed = ER.term_ratio(name, terms[name], ld), ER.allowed_scalar(ratio_np)
        _say(f'{name} {tag}', ratio, allowed)
        assert ratio <= allowed, (tag, name, terms[name], float(ld.value[name]))


@pytest.mark.parametrize('dinv', [256, False])
@pytest.mark.parametrize('Nd', [65, 129])
@pytest.mark.parametrize('system', ['elliptic', 'burgers', 'eikonal', 'darcy'])
def test_terms_on_synthetic_factors(dev_ctx, system, Nd, dinv):
    ctx, cs = dev_ctx, R.case(system, Nd)
    prob = TP._problem(ctx, cs, dinv)
    z = ctx.array(cs.z0)
    terms, P, Rf, info = ctx.log_evidence(prob, z)
    assert info == 0 and set(terms) == set(ER.TERMS)
    ld, np64 = _synthetic_reference(system, Nd)
    _gate_terms(f'{system} {Nd} dinv {dinv}', terms, ld, np64)
    # P (its nz columns) and the factor R: exactly what gpk_posterior_prepare leaves
    P2, R2, info2 = ctx.posterior_prepare(prob, z)
    ctx.synchronize()
    assert info2 == 0
    assert np.array_equal(VA.bits(P.download()[:, :cs.nz]), VA.bits(P2.download()[:, :cs.nz]))
    assert np.array_equal(VA.bits(np.tril(Rf.download())), VA.bits(np.tril(R2.download())))
    again = ctx.log_evidence(prob, z)[0]
    assert all(VA.bits(again[k]) == VA.bits(terms[k]) for k in ER.TERMS)
    prob.free()


def _raw_log_evidence(ctx, prob, z, P, R, work, terms, info):
    """gpk_log_evidence itself with caller-sized buffers: (return code, gpk_last_error)"""
    ptr = lambda a: a.ptr if a is not None else None
    rc = ctx.lib.gpk_log_evidence(ctx.h, C.byref(prob.struct) if prob is not None else None, ptr(z), ptr(P), P.ld if P is not None else 0,
                                  ptr(R), R.ld if R is not None else 0, ptr(work), terms, C.byref(info) if info is not None else None)
    return rc, ctx.lib.gpk_last_error(ctx.h).decode()


def test_relaxed_system_and_null_pointers_are_rejected_by_the_entry_point(dev_ctx):
    """the C call directly: Context.log_evidence sizes its buffers with gpk_posterior_worksize, which turns the relaxed system away
    before gpk_log_evidence is reached"""
    ctx = dev_ctx
    cs = R.case('relaxed', 65)
    prob = TP._problem(ctx, cs, False)
    z, work = ctx.array(cs.z0), prob.workspace()[3]
    P, Rf = ctx.empty(prob.rows, prob.nz + 1), ctx.empty(prob.nz, prob.nz)
    P.upload(np.full((prob.rows, prob.nz + 1), 7.0))
    terms, info = (C.c_double * 6)(*([-1.0] * 6)), C.c_int(-5)
    rc, msg = _raw_log_evidence(ctx, prob, z, P, Rf, work, terms, info)
    assert rc == -9001 and msg == 'invalid argument: posterior: the relaxed elliptic system is not served', (rc, msg)   # (the text gpk_posterior_prepare gives)
    rc2 = ctx.lib.gpk_posterior_prepare(ctx.h, C.byref(prob.struct), z.ptr, P.ptr, P.ld, Rf.ptr, Rf.ld, C.byref(info))
    assert rc2 == -9001 and ctx.lib.gpk_last_error(ctx.h).decode() == msg
    assert list(terms) == [-1.0] * 6 and info.value == -5 and np.all(P.download() == 7.0)               # nothing was written
    prob.free()
    # a served system: every NULL argument is -9001 with a name; the problem and z, P, R are prepare's to check
    cs = R.case('elliptic', 65)
    prob = TP._problem(ctx, cs, False)
    z, work = ctx.array(cs.z0), prob.workspace()[3]
    P, Rf = ctx.empty(prob.rows, prob.nz + 1), ctx.empty(prob.nz, prob.nz)
    good = dict(prob=prob, z=z, P=P, R=Rf, work=work, terms=terms, info=info)
    for missing, word in (('work', 'log_evidence: null work'), ('terms', 'log_evidence: null work'), ('info', 'log_evidence: null work'),
                          ('prob', 'null problem'), ('z', 'null z / P / R'), ('P', 'null z / P / R'), ('R', 'null z / P / R')):
        rc, msg = _raw_log_evidence(ctx, **dict(good, **{missing: None}))
        assert rc == -9001 and word in msg, (missing, rc, msg)
    assert ctx.lib.gpk_log_evidence(None, C.byref(prob.struct), z.ptr, P.ptr, P.ld, Rf.ptr, Rf.ld, work.ptr, terms, C.byref(info)) == -9001
    small = ctx.empty(prob.nz, prob.nz)
    small.ld = prob.nz - 1
    rc, msg = _raw_log_evidence(ctx, **dict(good, R=small))
    assert rc == -9001 and 'ldr < nz' in msg, (rc, msg)
    rc, msg = _raw_log_evidence(ctx, **good)                           # and the same arguments, all present, are served
    assert rc == 0 and info.value == 0 and np.isfinite(terms[0])
    prob.free()


def test_class_api_after_the_relaxed_method_says_so():
    import main_NonLinElliptic2d as drv
    from _driver_common import solve_forward
    cfg = drv.parse(['--N_domain', '60', '--N_boundary', '20', '--GNsteps', '2'] + QUIET)
    u, f = drv.manufactured(cfg.alpha, cfg.m)
    np.random.seed(0)
    s, _ = solve_forward(cfg, 'Nonlinear_elliptic', u, f, drv.UNIT_SQUARE, solve_kwargs={'method': 'relaxation'}, verbose=False)
    with pytest.raises(NotImplementedError, match='relaxed'):
        s.eqn.log_evidence()
    with pytest.raises(NotImplementedError, match='relaxed'):
        s.log_evidence(print_option=False)
    assert '_posterior' not in s.eqn.__dict__ and 'log_evidence_terms' not in s.eqn.__dict__
    s.eqn.GN_method(max_iter=2, print_hist=False)                      # the elimination solve of the same object is served
    assert np.isfinite(s.eqn.log_evidence())


# ------------------------------------------------------------------------------------------------ c. the affine identity, class API
def _affine_gate(tag, eqn, T):
    """log_evidence() of the solved alpha = 0 problem against log N(d; 0, Theta_dd), d = [-f; g], T the host Gram matrix with nugget"""
    Nd, Nb = eqn.N_domain, eqn.N_boundary
    rows = ER.elliptic_data_rows(Nd, Nb)
    d = np.concatenate([-eqn.rhs_f, eqn.bdy_g])
    Tdd = T[np.ix_(rows, rows)]
    want = ER.gaussian_loglik_ld(Tdd, d)
    rel = lambda v: float(abs(LD(v) - want) / abs(want))
    cs = ER.elliptic_case(Nd, Nb, eqn.rhs_f, eqn.bdy_g, T)
    err_np = max(rel(ER.gaussian_loglik_np64(Tdd, d)), rel(ER.terms_np64(cs, eqn._z_star[1], cs.factors()[1]).value['log_Z']))
    got = eqn.log_evidence()
    print(f'\n[evidence] affine {tag}: log Z {got:.12g}, numpy relative error {err_np:.3g}, device {rel(got):.3g}, '
          f'allowed {R.MARGIN * err_np:.3g}')
    assert err_np < 1e-9, 'precondition: the gate could hide a wrong result'
    assert rel(got) <= R.MARGIN * err_np, (tag, got, float(want))
    t = eqn.log_evidence_terms
    assert t['info'] == 0 and t['log_Z'] == got and t['gamma_term'] == 0.0


def _solve_affine(eqn, Nd, Nb, kernel_parameter):
    np.random.seed(3)
    eqn.sampled_pts(Nd, Nb)
    eqn.Gram_matrix(kernel='Gaussian', kernel_parameter=kernel_parameter, nugget=1e-6, nugget_type='adaptive')
    eqn.Gram_Cholesky()
    assert eqn.chol_info == 0
    eqn.GN_method(max_iter=1, print_hist=False)                         # affine F: one step from anywhere reaches the minimiser
    assert eqn.step_info == [0]


@pytest.mark.parametrize('sigma', [0.1, 0.2])
def test_affine_identity_dirichlet(sigma):
    import main_NonLinElliptic2d as drv
    from src.PDEs import Nonlinear_elliptic2d
    u, f = drv.manufactured(0.0, 3.0)
    eqn = Nonlinear_elliptic2d(alpha=0.0, m=3.0, bdy=u, rhs=f, domain=np.array(drv.UNIT_SQUARE))
    _solve_affine(eqn, 150, 40, sigma)
    T, _ = O.add_nugget(O.gram_matrix_assembly(eqn.X_domain, eqn.X_boundary, 'Nonlinear_elliptic', 'Gaussian', sigma),
                        'Nonlinear_elliptic', 150, 40, 1e-6)
    _affine_gate(f'dirichlet sigma {sigma}', eqn, T)


def test_affine_identity_robin():
    """Theta of the boundary-functional layout from the host reference of tests/test_robin_host.py"""
    import test_robin_host as RH
    from src.PDEs import Nonlinear_elliptic2d
    beta, sigma = 2.0, 0.2
    eqn = Nonlinear_elliptic2d(alpha=0.0, m=3.0, bdy=RH.bdy_for('robin', beta), rhs=RH.rhs_for(0.0, 3), domain=np.array(RH.UNIT_SQUARE),
                               bc='robin', robin_beta=beta)
    _solve_affine(eqn, 150, 40, sigma)
    p = RH.precisions('Gaussian', sigma)
    T = RH.theta(eqn.X_domain, eqn.X_boundary, eqn.boundary_coeffs, p)[0]
    T = T + np.diag(RH.nugget_diag(p, 150, 40, eqn.boundary_coeffs, 1e-6, 'adaptive'))
    _affine_gate('robin sigma 0.2', eqn, T)
    with pytest.raises(NotImplementedError, match='gpk_assemble_bc'):    # the variance of this layout is still not served
        eqn.posterior_variance(np.full((3, 2), 0.5))


def test_affine_identity_three_dimensions():
    """Theta of the three-dimensional layout from the host reference of tests/test_elliptic3d_host.py"""
    import test_elliptic3d_host as E3
    from src.PDEs import Nonlinear_elliptic3d
    sigma = 0.3
    eqn = Nonlinear_elliptic3d(alpha=0.0, m=3.0, bdy=E3.truth, rhs=E3.rhs_for(0.0, 3), domain=np.array(E3.UNIT_CUBE))
    _solve_affine(eqn, 125, 54, sigma)
    p = E3.precisions('Gaussian', sigma)
    T = E3.theta(eqn.X_domain, eqn.X_boundary, p)[0] + np.diag(E3.nugget_diag(p, 125, 54, 1e-6, 'adaptive'))
    _affine_gate('3d sigma 0.3', eqn, T)


# ------------------------------------------------------------------------------------------------ d. the nonlinear case, every system
@pytest.mark.parametrize('name', sorted(TP.REAL))
def test_class_api_on_real_gram_matrices(name):
    s, cfg = TP._solve(name)
    e = s.eqn
    got = s.log_evidence(print_option=False)
    terms = e.log_evidence_terms
    assert terms['info'] == 0 and got == terms['log_Z'] and np.isfinite(got)
    cs = TP._real_case(name, e, cfg)
    z = e._z_star[1]
    ld, f64 = cs.factors()
    ref = ER.terms_ld(cs, z, ld, PR.prepare_ld(cs, z, ld))
    np64 = ER.terms_np64(cs, z, f64)
    print(f'\n[evidence] real {name}: log Z {got:.12g} = -({terms["J"]:.6g} + {terms["logdet_theta"]:.6g} + {terms["logdet_H"]:.6g}) / 2 '
          f'- {terms["gamma_term"]:.6g} - {terms["two_pi_term"]:.6g}')
    if name == 'Darcy_flow2d':
        assert terms['gamma_term'] == pytest.approx(e.N_data * np.log(e.noise_level), rel=1e-15) and terms['gamma_term'] != 0
    _gate_terms(f'real {name}', terms, ref, np64)


# ------------------------------------------------------------------------------------------------ e. selection
CANDIDATES = (0.08, 0.1, 0.15, 0.2, 0.3)
ELLIPTIC = ['--N_domain', '150', '--N_boundary', '40', '--nugget', '1e-6']


def _elliptic_solver(extra=()):
    import main_NonLinElliptic2d as drv
    from src.solver import solver_GP
    cfg = drv.parse(ELLIPTIC + list(extra) + QUIET)
    u, f = drv.manufactured(cfg.alpha, cfg.m)
    np.random.seed(0)
    s = solver_GP(cfg, PDE_type='Nonlinear_elliptic')
    s.set_equation(bdy=u, rhs=f, domain=np.array(drv.UNIT_SQUARE), print_option=False)
    s.auto_sample(cfg.N_domain, cfg.N_boundary, sampled_type=cfg.sampled_type, print_option=False)
    return s, cfg, u


def _cpu_selection(e, cfg, z0):
    """the same selection with the oracle: per candidate the float64 Gauss-Newton iterate from z0, then the long-double and the float64
    numpy terms at that iterate"""
    out = []
    for sigma in CANDIDATES:
        T, _ = O.add_nugget(O.gram_matrix_assembly(e.X_domain, e.X_boundary, 'Nonlinear_elliptic', cfg.kernel, sigma),
                            'Nonlinear_elliptic', e.N_domain, e.N_boundary, cfg.nugget)
        z, _ = O.gn_method(O.EllipticSystem(cfg.alpha, cfg.m, e.rhs_f, e.bdy_g), [O.cholesky(T)], z0, cfg.GNsteps, cfg.step_size)
        cs = PR.RealCase('elliptic', e.N_domain, e.N_boundary, e.rhs_f, e.bdy_g, float(cfg.alpha), float(cfg.m), T)
        ld, f64 = cs.factors()
        out.append((ER.terms_ld(cs, z, ld), ER.terms_np64(cs, z, f64)))
    return out


def test_selection_against_the_oracle():
    s, cfg, u = _elliptic_solver()
    e = s.eqn
    winner = s.select_kernel_parameter(CANDIDATES, print_option=False)
    sel = s.kernel_selection
    assert sel['candidates'] == list(CANDIDATES) and sel['info'] == [(0, 0, 0)] * len(CANDIDATES) and not any(sel['refined'])
    cpu = _cpu_selection(e, cfg, e.init_sol)
    cpu_logz = [float(ld.value['log_Z']) for ld, _ in cpu]
    for k, sigma in enumerate(CANDIDATES):
        ld, np64 = cpu[k]
        ratio_np = ER.term_ratio('log_Z', np64.value['log_Z'], ld)
        _precondition(f'selection sigma {sigma}', ratio_np, ld.scale['log_Z'], ld.value['log_Z'])
        ratio, allowed = ER.term_ratio('log_Z', sel['log_Z'][k], ld), ER.allowed_scalar(ratio_np)
        print(f'\n[evidence] selection sigma {sigma}: device log Z {sel["log_Z"][k]:.12g}, oracle {cpu_logz[k]:.12g}, J {sel["J"][k]:.6g}; '
              f'device {ratio:.3g}, allowed {allowed:.3g}')
        assert ratio <= allowed, (sigma, sel['log_Z'][k], cpu_logz[k])
    best = int(np.argmax(cpu_logz))
    gaps = [cpu_logz[best] - v for k, v in enumerate(cpu_logz) if k != best]
    print(f'\n[evidence] selection: oracle argmax sigma {CANDIDATES[best]}, nearest competitor {min(gaps):.4g} log units below')
    assert sel['best'] == best and winner == CANDIDATES[best] == cfg.kernel_parameter == e.kernel_parameter
    # left solved at the winner, ready for test(); posterior_variance after log_evidence: the bits it gives when it prepares itself
    Xt = np.random.RandomState(8).uniform(0, 1, (67, 2))
    s.test(Xt, print_option=False)
    s.get_test_error(u(Xt[:, 0], Xt[:, 1]), print_option=False)
    print(f'\n[evidence] selection: test L2 error at the winner {s.test_L2_err:.3g}')
    assert e.__dict__.get('_posterior') is not None
    after = e.posterior_variance(Xt).copy()
    e._drop_posterior()
    alone = e.posterior_variance(Xt)
    assert np.array_equal(VA.bits(after), VA.bits(alone))
    # refinement from the same table: inside the bracket of the winner's grid neighbours, never below the grid's best
    s2, cfg2, _ = _elliptic_solver()
    w2 = s2.select_kernel_parameter(CANDIDATES, refine=3, print_option=False)
    sel2 = s2.kernel_selection
    lo, hi = CANDIDATES[best - 1], CANDIDATES[best + 1]
    assert len(sel2['candidates']) == len(CANDIDATES) + 3 and all(lo < p < hi for p in sel2['candidates'][len(CANDIDATES):])
    assert all(VA.bits(a) == VA.bits(b) for a, b in zip(sel2['log_Z'][:len(CANDIDATES)], sel['log_Z']))   # one initial iterate, fixed-order sums
    assert lo < w2 < hi and sel2['log_Z'][sel2['best']] >= sel['log_Z'][best] and cfg2.kernel_parameter == w2
    print(f'\n[evidence] selection refine 3: sigma {w2:.6g}, log Z {sel2["log_Z"][sel2["best"]]:.12g} (grid: {sel["log_Z"][best]:.12g})')


def test_failed_candidate_is_listed_and_never_chosen():
    """without a nugget the Gram matrix at sigma = 0.8 is numerically singular; at sigma = 0.05 it is well conditioned"""
    s, cfg, _ = _elliptic_solver(['--nugget_type', 'none'])
    w = s.select_kernel_parameter([0.8, 0.05], print_option=False)
    sel = s.kernel_selection
    print(f'\n[evidence] failed candidate: info {sel["info"]}, log Z {list(sel["log_Z"])}')
    assert w == 0.05 and sel['best'] == 1 and sel['info'][1] == (0, 0, 0)
    assert sel['info'][0] != (0, 0, 0) and sel['candidates'][0] == 0.8


def test_driver_flag(capsys):
    import main_NonLinElliptic2d as drv
    from src._runtime import get_context
    base = ELLIPTIC + QUIET
    np.random.seed(0)
    drv.main(base)
    plain = capsys.readouterr().out.splitlines()
    np.random.seed(0)
    drv.main(base + ['--select_kernel_parameter', '0.2'])
    one = capsys.readouterr().out.splitlines()
    np.random.seed(0)
    drv.main(base + ['--select_kernel_parameter', '0.15,0.2', '--select_refine', '1'])
    two = capsys.readouterr().out.splitlines()
    tagged = lambda lines: [x for x in lines if x.startswith('[Kernel selection]')]
    errors = lambda lines: [x for x in lines if 'error]' in x]
    assert not tagged(plain) and len(errors(plain)) == 4
    # the only candidate is the default parameter, solved from the iterate solve() draws: the same numbers on every error line
    assert len(tagged(one)) == 2 and 'chosen kernel_parameter 0.2' in tagged(one)[1] and errors(one) == errors(plain)
    # and the flag changes nothing but its own lines: every other character of the output is the default run's, numbers included
    assert [x for x in one if not x.startswith('[Kernel selection]')] == plain
    assert one[:2] == tagged(one)                                      # its lines stand where the solve is, in front of the reports
    rest = [x for x in two if not x.startswith('[Kernel selection]')]
    assert [x.split(']')[0] for x in rest] == [x.split(']')[0] for x in plain]   # another winner: the same lines, other numbers
    assert len(tagged(two)) == 3 and 'an end of the candidate grid' in tagged(two)[2]
    get_context().synchronize()
