"""Joint posterior covariance and posterior samples on the device: gpk_assemble_prior, gpk_posterior_covariance, gpk_posterior_sample
and the class API above them.

  a  the prior evaluator against the long-double kernel formulas (4e-15 max|block|, the bound of gate_blocks for Theta_test), bitwise
     symmetric with unit diagonal on a square call, 16-byte against 8-byte stores bit for bit, on an unaligned view between canaries,
     bad arguments by name
  b  the covariance arithmetic on the synthetic, well-conditioned factors of tests/_gn_reference.py against long double, entrywise in
     units of eps S_st (tests/_posterior_cov_reference.py): the conditional covariance (with_gn = 0, scale |Ktt| + |V|^T |V|) and the
     whole covariance (with_gn = 1, scale S), each judged by the float64 numpy pipeline measured in the same test; the diagonal against
     gpk_posterior_variance; symmetry, repeatability and a fresh handle to the bit
  c  the class API on real Gram matrices against the long-double formula at the device's own final iterate and the oracle's Theta
  d  samples: the factor, the identity sample = mean + L xi, seeds, shapes, a failed pivot
  e  the surface: what is not served, the drivers' flag

Gates b and c are not constants: the device may take R.MARGIN = 32 times what the float64 numpy pipeline takes on the same inputs (plus
one eps in b).  Every figure is printed under a [posterior-cov] tag before it is asserted.

The four REAL configurations are those of tests/test_gpu_posterior.py, with the same arguments.

RESULTS
  The [posterior-cov] lines of a run on an MI355X (gfx950):
    [posterior-cov] prior Gaussian: worst |error| / max|block| 1.33e-16, bound 4e-15
    [posterior-cov] prior anisotropic_Gaussian: worst |error| / max|block| 1.72e-16, bound 4e-15
    [posterior-cov] prior Matern52: worst |error| / max|block| 3.27e-16, bound 4e-15
    [posterior-cov] prior Matern72: worst |error| / max|block| 3.19e-16, bound 4e-15
    [posterior-cov] prior Matern92: worst |error| / max|block| 3.02e-16, bound 4e-15
    [posterior-cov] cov_cond elliptic 65 field 0 dinv 256: device 0.667, allowed 45.7
    [posterior-cov] cov elliptic 65 field 0 dinv 256: device 0.874, allowed 29.1
    [posterior-cov] diag elliptic 65 field 0 dinv 256: cond 0.469 of 45.7, whole 0.859 of 29.1
    [posterior-cov] cov_cond elliptic 65 field 0 dinv False: device 1.07, allowed 45.7
    [posterior-cov] cov elliptic 65 field 0 dinv False: device 1.24, allowed 29.1
    [posterior-cov] diag elliptic 65 field 0 dinv False: cond 0.469 of 45.7, whole 0.859 of 29.1
    [posterior-cov] cov_cond elliptic 129 field 0 dinv 256: device 0.71, allowed 30.8
    [posterior-cov] cov elliptic 129 field 0 dinv 256: device 0.779, allowed 26.4
    [posterior-cov] diag elliptic 129 field 0 dinv 256: cond 0.915 of 30.8, whole 0.884 of 26.4
    [posterior-cov] cov_cond elliptic 129 field 0 dinv False: device 1.63, allowed 30.8
    [posterior-cov] cov elliptic 129 field 0 dinv False: device 0.956, allowed 26.4
    [posterior-cov] diag elliptic 129 field 0 dinv False: cond 0.463 of 30.8, whole 0.884 of 26.4
    [posterior-cov] cov_cond burgers 65 field 0 dinv 256: device 0.611, allowed 21.2
    [posterior-cov] cov burgers 65 field 0 dinv 256: device 0.891, allowed 27.7
    [posterior-cov] diag burgers 65 field 0 dinv 256: cond 0.468 of 21.2, whole 0.886 of 27.7
    [posterior-cov] cov_cond burgers 65 field 0 dinv False: device 1.47, allowed 21.2
    [posterior-cov] cov burgers 65 field 0 dinv False: device 0.833, allowed 27.7
    [posterior-cov] diag burgers 65 field 0 dinv False: cond 0.466 of 21.2, whole 0.872 of 27.7
    [posterior-cov] cov_cond burgers 129 field 0 dinv 256: device 0.864, allowed 18.5
    [posterior-cov] cov burgers 129 field 0 dinv 256: device 0.877, allowed 29.1
    [posterior-cov] diag burgers 129 field 0 dinv 256: cond 0.927 of 18.5, whole 0.878 of 29.1
    [posterior-cov] cov_cond burgers 129 field 0 dinv False: device 0.978, allowed 18.5
    [posterior-cov] cov burgers 129 field 0 dinv False: device 0.877, allowed 29.1
    [posterior-cov] diag burgers 129 field 0 dinv False: cond 0.923 of 18.5, whole 0.874 of 29.1
    [posterior-cov] cov_cond eikonal 65 field 0 dinv 256: device 0.671, allowed 22.5
    [posterior-cov] cov eikonal 65 field 0 dinv 256: device 69.6, allowed 1.52e+03
    [posterior-cov] diag eikonal 65 field 0 dinv 256: cond 0.467 of 22.5, whole 0.87 of 1.52e+03
    [posterior-cov] cov_cond eikonal 65 field 0 dinv False: device 0.743, allowed 22.5
    [posterior-cov] cov eikonal 65 field 0 dinv False: device 78.7, allowed 1.52e+03
    [posterior-cov] diag eikonal 65 field 0 dinv False: cond 0.914 of 22.5, whole 0.87 of 1.52e+03
    [posterior-cov] cov_cond eikonal 129 field 0 dinv 256: device 0.855, allowed 18.7
    [posterior-cov] cov eikonal 129 field 0 dinv 256: device 46.2, allowed 1.05e+03
    [posterior-cov] diag eikonal 129 field 0 dinv 256: cond 0.925 of 18.7, whole 0.879 of 1.05e+03
    [posterior-cov] cov_cond eikonal 129 field 0 dinv False: device 0.895, allowed 18.7
    [posterior-cov] cov eikonal 129 field 0 dinv False: device 40.3, allowed 1.05e+03
    [posterior-cov] diag eikonal 129 field 0 dinv False: cond 0.925 of 18.7, whole 0.873 of 1.05e+03
    [posterior-cov] cov_cond darcy 65 field 0 dinv 256: device 0.801, allowed 38.3
    [posterior-cov] cov darcy 65 field 0 dinv 256: device 0.821, allowed 30.3
    [posterior-cov] diag darcy 65 field 0 dinv 256: cond 0.467 of 38.3, whole 0.449 of 30.3
    [posterior-cov] cov_cond darcy 65 field 1 dinv 256: device 0.707, allowed 29.6
    [posterior-cov] cov darcy 65 field 1 dinv 256: device 0.944, allowed 27.8
    [posterior-cov] diag darcy 65 field 1 dinv 256: cond 0.465 of 29.6, whole 0.861 of 27.8
    [posterior-cov] cov_cond darcy 65 field 0 dinv False: device 0.83, allowed 38.3
    [posterior-cov] cov darcy 65 field 0 dinv False: device 1.1, allowed 30.3
    [posterior-cov] diag darcy 65 field 0 dinv False: cond 0.47 of 38.3, whole 0.88 of 30.3
    [posterior-cov] cov_cond darcy 65 field 1 dinv False: device 0.893, allowed 29.6
    [posterior-cov] cov darcy 65 field 1 dinv False: device 0.785, allowed 27.8
    [posterior-cov] diag darcy 65 field 1 dinv False: cond 0.465 of 29.6, whole 0.859 of 27.8
    [posterior-cov] cov_cond darcy 129 field 0 dinv 256: device 0.693, allowed 15.8
    [posterior-cov] cov darcy 129 field 0 dinv 256: device 0.847, allowed 28.1
    [posterior-cov] diag darcy 129 field 0 dinv 256: cond 0.466 of 15.8, whole 0.891 of 28.1
    [posterior-cov] cov_cond darcy 129 field 1 dinv 256: device 0.835, allowed 17.1
    [posterior-cov] cov darcy 129 field 1 dinv 256: device 1.61, allowed 26.2
    [posterior-cov] diag darcy 129 field 1 dinv 256: cond 0.919 of 17.1, whole 1.72 of 26.2
    [posterior-cov] cov_cond darcy 129 field 0 dinv False: device 1.06, allowed 15.8
    [posterior-cov] cov darcy 129 field 0 dinv False: device 0.934, allowed 28.1
    [posterior-cov] diag darcy 129 field 0 dinv False: cond 0.466 of 15.8, whole 0.891 of 28.1
    [posterior-cov] cov_cond darcy 129 field 1 dinv False: device 1.24, allowed 17.1
    [posterior-cov] cov darcy 129 field 1 dinv False: device 1.23, allowed 26.2
    [posterior-cov] diag darcy 129 field 1 dinv False: cond 0.921 of 17.1, whole 1.3 of 26.2
    [posterior-cov] real Burgers: numpy error cond 4.81e-13, whole 1.56e-11; min var 0.052, max var 0.937
    [posterior-cov] real Burgers: device cond 1.56e-13 of 1.54e-11, whole 2.03e-11 of 5.01e-10
    [posterior-cov] real Burgers: diagonal against posterior_variance cond 1.44e-15, whole 1.5e-15
    [posterior-cov] real Darcy_flow2d_u: numpy error cond 2.33e-15, whole 4.27e-14; min var 3.77e-06, max var 0.00173
    [posterior-cov] real Darcy_flow2d_u: device cond 7.7e-15 of 7.44e-14, whole 2.79e-14 of 1.37e-12
    [posterior-cov] real Darcy_flow2d_u: diagonal against posterior_variance cond 1.55e-15, whole 1.55e-15
    [posterior-cov] real Darcy_flow2d_a: numpy error cond 1.62e-14, whole 6.41e-11; min var 0.144, max var 0.851
    [posterior-cov] real Darcy_flow2d_a: device cond 2.48e-14 of 5.18e-13, whole 1.16e-10 of 2.05e-09
    [posterior-cov] real Darcy_flow2d_a: diagonal against posterior_variance cond 1.89e-15, whole 1.78e-15
    [posterior-cov] real Eikonal: numpy error cond 1.64e-15, whole 7.12e-14; min var 5.96e-07, max var 0.00108
    [posterior-cov] real Eikonal: device cond 1.31e-14 of 5.24e-14, whole 1.13e-13 of 2.28e-12
    [posterior-cov] real Eikonal: diagonal against posterior_variance cond 2.44e-15, whole 2.44e-15
    [posterior-cov] real Nonlinear_elliptic: numpy error cond 1.89e-15, whole 6.73e-14; min var 5.36e-07, max var 0.000212
    [posterior-cov] real Nonlinear_elliptic: device cond 4.53e-14 of 6.06e-14, whole 3.36e-14 of 2.15e-12
    [posterior-cov] real Nonlinear_elliptic: diagonal against posterior_variance cond 1.67e-15, whole 1.67e-15
    [posterior-cov] samples Burgers: N_t x numpy error 1.05e-09, jitter / 4 2.5e-07
    [posterior-cov] factor Burgers: |L L^T - (Sigma + jitter I)| 6.62e-16, bound 4.53e-13
    [posterior-cov] sample Burgers: |sample - mean - L xi| / (eps (|mean| + |L||xi|)) 1.76, bound 69
    [posterior-cov] samples Darcy_flow2d_u: N_t x numpy error 2.86e-12, jitter / 4 2.5e-07
    [posterior-cov] factor Darcy_flow2d_u: |L L^T - (Sigma + jitter I)| 1.45e-19, bound 8.36e-16
    [posterior-cov] sample Darcy_flow2d_u: |sample - mean - L xi| / (eps (|mean| + |L||xi|)) 1.14, bound 69
    [posterior-cov] samples Darcy_flow2d_a: N_t x numpy error 4.3e-09, jitter / 4 2.5e-07
    [posterior-cov] factor Darcy_flow2d_a: |L L^T - (Sigma + jitter I)| 1.54e-16, bound 4.11e-13
    [posterior-cov] sample Darcy_flow2d_a: |sample - mean - L xi| / (eps (|mean| + |L||xi|)) 1.3, bound 69
    [posterior-cov] samples Eikonal: N_t x numpy error 4.77e-12, jitter / 4 2.5e-07
    [posterior-cov] factor Eikonal: |L L^T - (Sigma + jitter I)| 5.13e-20, bound 5.21e-16
    [posterior-cov] sample Eikonal: |sample - mean - L xi| / (eps (|mean| + |L||xi|)) 0.96, bound 69
    [posterior-cov] samples Nonlinear_elliptic: N_t x numpy error 4.51e-12, jitter / 4 2.5e-07
    [posterior-cov] factor Nonlinear_elliptic: |L L^T - (Sigma + jitter I)| 1.92e-20, bound 1.03e-16
    [posterior-cov] sample Nonlinear_elliptic: |sample - mean - L xi| / (eps (|mean| + |L||xi|)) 0.491, bound 69
    [posterior-cov] driver: [Test samples] 3 samples, RMS spread 0.004538949770477255, max spread 0.0635619711184004
"""
import functools
import os
import sys

import numpy as np
import pytest

import _gn_reference as R
import _posterior_reference as PR
import _posterior_cov_reference as CR
import _view_arena as VA
from _gauss_reference import BOUND
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'nonlinpdes-gpsolver_amd')
if PKG not in sys.path:
    sys.path.insert(0, PKG)

LD, EPS = R.LD, R.EPS


def _say(text):
    print(f'\n[posterior-cov] {text}')


def _pts(rng, n):
    return rng.uniform(0, 1, (n, 2))


def _same(a, b):
    return np.array_equal(VA.bits(a), VA.bits(b))


# ------------------------------------------------------------------------------------------------ a. gpk_assemble_prior
KERNELS = (('Gaussian', 0.2), ('anisotropic_Gaussian', [0.3, 0.07]), ('Matern52', 0.3), ('Matern72', [0.3, 0.2]), ('Matern92', 0.25))
SIZES = (1, 67, 300)


def _prior(ctx, kernel, kp, Xa, Xb=None):
    na, nb = Xa.shape[0], (Xa if Xb is None else Xb).shape[0]
    return ctx.assemble_prior(kernel, kp, Xa, Xb).download(na, nb).reshape(na, nb)


@pytest.mark.parametrize('kernel,kp', KERNELS)
def test_assemble_prior_against_long_double(dev_ctx, kernel, kp):
    ctx = dev_ctx
    rng = np.random.RandomState(29)
    worst = 0.0
    for na in SIZES:
        for nb in SIZES:
            Xa, Xb = _pts(rng, na), _pts(rng, nb)
            # The bound is relative to max|block| and presumes a block with an entry of order 1, as every Gram block has.  Any float64
            # evaluation rounds the exponent x = (p1 d1^2 + p2 d2^2) / 2 to about 4 eps x (p, d, two products, the sum), so a lone
            # entry exp(-x) of two far points is off by 4 eps x of ITSELF -- 30 eps at x = 8 -- while its absolute error never exceeds
            # 4 eps / e.  One pair a hundredth of a length scale apart puts that entry of order 1 into every block, the 1 x 1 one too.
            Xb[0] = Xa[0] + 0.01 * np.min(np.atleast_1d(kp))
            got = _prior(ctx, kernel, kp, Xa, Xb)
            ref = CR.prior_ld(kernel, kp, Xa, Xb)
            err = float(np.max(np.abs(got.astype(LD) - ref))) / float(np.max(np.abs(ref)))
            worst = max(worst, err)
            assert err <= BOUND, (kernel, na, nb, err)
            try:                                                      # the 8-byte store path: the same bits
                ctx.tune(47, 0)
                narrow = _prior(ctx, kernel, kp, Xa, Xb)
            finally:
                ctx.tune(47, 1)
            assert _same(narrow, got), (kernel, na, nb)
    _say(f'prior {kernel}: worst |error| / max|block| {worst:.3g}, bound {BOUND:.3g}')


@pytest.mark.parametrize('kernel,kp', KERNELS)
def test_assemble_prior_square_call_is_symmetric_with_unit_diagonal(dev_ctx, kernel, kp):
    ctx = dev_ctx
    rng = np.random.RandomState(31)
    for n in SIZES + (514, 515):                                      # (two workgroups along j, even and odd)
        X = _pts(rng, n)
        X[n // 2] = X[0]                                              # a coincident pair off the diagonal
        got = _prior(ctx, kernel, kp, X)
        assert _same(got, got.T), (kernel, n)
        assert np.all(VA.bits(np.diag(got)) == VA.bits(np.ones(n))), (kernel, n)
        assert got[n // 2, 0] == 1.0
        assert _same(got, _prior(ctx, kernel, kp, X, X.copy()))       # Xa == Xb by value or by pointer


@pytest.mark.parametrize('kernel,kp', KERNELS)
def test_assemble_prior_on_an_unaligned_view(dev_ctx, kernel, kp):
    import gpk
    ctx = dev_ctx
    rng = np.random.RandomState(37)
    na, nb = 67, 300
    Xa, Xb = _pts(rng, na), _pts(rng, nb)
    aligned = _prior(ctx, kernel, kp, Xa, Xb)
    v = VA.class_view(ctx, na, nb, 'D')                               # odd base offset, odd ld
    dXa, dXb = ctx.points(Xa), ctx.points(Xb)
    ctx._chk(ctx.lib.gpk_assemble_prior(ctx.h, gpk.KERNEL[kernel], gpk.device.kernel_params(kernel, kp), dXa.ptr, na, dXb.ptr, nb, v.ptr, v.ld))
    ctx.synchronize()
    v.arena.assert_outside_untouched([v])
    assert _same(v.arena.get(v), aligned)
    v.arena.free()


def test_assemble_prior_rejects_bad_arguments(dev_ctx):
    import gpk
    ctx = dev_ctx
    X = ctx.points(_pts(np.random.RandomState(1), 8))
    out = ctx.empty(8, 8)
    kp = gpk.device.kernel_params('Gaussian', 0.2)
    call = lambda *a: ctx._chk(ctx.lib.gpk_assemble_prior(ctx.h, 0, kp, *a))
    with pytest.raises(gpk.GpkError, match='-9001.*assemble_prior: ld < nb'):
        call(X.ptr, 8, X.ptr, 8, out.ptr, 7)
    with pytest.raises(gpk.GpkError, match='-9001.*assemble_prior: na <= 0'):
        call(X.ptr, 0, X.ptr, 8, out.ptr, out.ld)
    with pytest.raises(gpk.GpkError, match='-9001.*assemble_prior: nb <= 0'):
        call(X.ptr, 8, X.ptr, -1, out.ptr, out.ld)
    for args in ((None, 8, X.ptr, 8, out.ptr, out.ld), (X.ptr, 8, None, 8, out.ptr, out.ld), (X.ptr, 8, X.ptr, 8, None, out.ld)):
        with pytest.raises(gpk.GpkError, match='-9001.*assemble_prior: pointers'):
            call(*args)
    with pytest.raises(gpk.GpkError, match='-9001.*assemble_prior: kernel id'):
        ctx._chk(ctx.lib.gpk_assemble_prior(ctx.h, 99, kp, X.ptr, 8, X.ptr, 8, out.ptr, out.ld))


# ------------------------------------------------------------------------------------------------ b. covariance arithmetic, synthetic factors
NT_B = 70


def _padded(ctx, A, pad, poison=R.POISON):
    rows, cols = A.shape
    full = np.full((rows, cols + pad), poison)
    full[:, :cols] = A
    d = ctx.empty(rows, cols + pad, ld=cols + pad)
    d.upload(full)
    d.cols = cols
    return d


def _upload_factor(ctx, L):
    n = L.shape[0]
    d = ctx.empty(n, n + R.LD_PAD, ld=n + R.LD_PAD)
    d.upload(R.poisoned(L))
    d.cols = n
    return d


def _problem(ctx, cs, dinv):
    import gpk
    L = _upload_factor(ctx, cs.L)
    L2 = _upload_factor(ctx, cs.L2) if cs.L2 is not None else None
    prob = gpk.GNProblem(ctx, R.SYSTEM_NAME[cs.system], cs.Nd, cs.Nb, cs.f, cs.g, L, p0=cs.p0, p1=cs.p1, pen_lambda=cs.lam,
                         data_u=cs.data, L2=L2, dinv=dinv, structured=False, cache_a=False)
    prob.keep += [L] + ([L2] if L2 is not None else [])
    return prob


@functools.lru_cache(maxsize=None)
def _synthetic_reference(system, Nd):
    """per (system, N_d), shared by the dinv variants: K, the prior, long-double and float64-numpy results of every field"""
    cs = R.case(system, Nd)
    full = R.full_reference(system, Nd)
    prepared = (full.S, PR.cholesky_ld(full.H / LD(2)))
    out = {}
    for field in ((0, 1) if system == 'darcy' else (0,)):
        n = PR.field_group(cs, field)[1]
        rng = np.random.RandomState(1000 * Nd + field)
        K = rng.normal(size=(n, NT_B))
        G = rng.normal(size=(NT_B, NT_B))
        Ktt = (G + G.T) / 2                                           # any symmetric matrix: the arithmetic does not ask for more;
        np.fill_diagonal(Ktt, 1.0)                                    # unit diagonal, as gpk_posterior_variance assumes of the prior
        out[field] = (K, Ktt, CR.covariance_ld(cs, cs.z0, K, Ktt, field, prepared=prepared), CR.covariance_np64(cs, cs.z0, K, Ktt, field))
    return out


def _cov(ctx, prob, P, Rf, K, Ktt, field, with_gn):
    Cm = ctx.posterior_covariance(prob, P, Rf, _padded(ctx, K, 5), _padded(ctx, Ktt, 3), field=field, with_gn=with_gn)
    ctx.synchronize()
    return Cm.download(NT_B, NT_B)


@pytest.mark.parametrize('dinv', [256, False])
@pytest.mark.parametrize('Nd', [65, 129])
@pytest.mark.parametrize('system', ['elliptic', 'burgers', 'eikonal', 'darcy'])
def test_covariance_arithmetic(dev_ctx, system, Nd, dinv):
    import gpk
    ctx, cs = dev_ctx, R.case(system, Nd)
    prob = _problem(ctx, cs, dinv)
    P, Rf, info = ctx.posterior_prepare(prob, ctx.array(cs.z0))
    assert info == 0
    fresh = gpk.Context(0, dev=True)
    try:
        fprob = _problem(fresh, cs, dinv)
        fP, fR, _ = fresh.posterior_prepare(fprob, fresh.array(cs.z0))
        for field, (K, Ktt, ld, np64) in _synthetic_reference(system, Nd).items():
            tag = f'{system} {Nd} field {field} dinv {dinv}'
            cond = _cov(ctx, prob, P, Rf, K, Ktt, field, False)
            cov = _cov(ctx, prob, P, Rf, K, Ktt, field, True)
            r1 = lambda x: R.ratio_entries(x, ld.cond, ld.scale_cond)
            r2 = lambda x: R.ratio_entries(x, ld.cov, ld.scale)
            a1, a2 = R.allowed(r1(np64.cond)), R.allowed(r2(np64.cond + np64.gn))
            _say(f'cov_cond {tag}: device {r1(cond):.3g}, allowed {a1:.3g}')
            _say(f'cov {tag}: device {r2(cov):.3g}, allowed {a2:.3g}')
            assert r1(cond) <= a1, tag
            assert r2(cov) <= a2, tag
            # the diagonal is gpk_posterior_variance's, within the same gates
            vc, v = ctx.posterior_variance(prob, P, Rf, _padded(ctx, K, 5), field=field)
            ctx.synchronize()
            dc = np.abs(np.diag(cond) - vc.download()) / (EPS * np.diag(ld.scale_cond).astype(np.float64))
            dv = np.abs(np.diag(cov) - v.download()) / (EPS * np.diag(ld.scale).astype(np.float64))
            _say(f'diag {tag}: cond {dc.max():.3g} of {a1:.3g}, whole {dv.max():.3g} of {a2:.3g}')
            assert dc.max() <= a1 and dv.max() <= a2, tag
            # both triangles, the same bits; a repeat and a fresh handle: the same bits
            assert _same(cond, cond.T) and _same(cov, cov.T), tag
            assert _same(_cov(ctx, prob, P, Rf, K, Ktt, field, True), cov), tag
            assert _same(_cov(fresh, fprob, fP, fR, K, Ktt, field, True), cov), tag
            # with_gn = 0 reads none of P, R, W
            assert _same(_cov(ctx, prob, None, None, K, Ktt, field, False), cond), tag
    finally:
        fresh.close()
    prob.free()


def test_covariance_rejects_relaxed_system_wrong_field_and_short_ld(dev_ctx):
    import gpk
    ctx = dev_ctx
    cs = R.case('relaxed', 65)
    prob = _problem(ctx, cs, False)
    K, Cm = ctx.array(np.zeros((prob.rows, 4))), ctx.array(np.eye(4))
    with pytest.raises(gpk.GpkError, match='-9001.*relaxed'):
        ctx.posterior_covariance(prob, None, None, K, Cm, with_gn=False)
    prob.free()
    cs = R.case('elliptic', 65)
    prob = _problem(ctx, cs, False)
    P, Rf, _ = ctx.posterior_prepare(prob, ctx.array(cs.z0))
    K = ctx.array(np.zeros((prob.rows, 4)))
    with pytest.raises(gpk.GpkError, match='-9001.*field 1'):
        ctx.posterior_covariance(prob, P, Rf, K, Cm, field=1)
    with pytest.raises(gpk.GpkError, match='-9001.*with_gn needs P, R and W'):
        ctx.posterior_covariance(prob, None, None, K, Cm, W=None, with_gn=True)
    Cm.ld = 3
    with pytest.raises(gpk.GpkError, match='-9001.*ldc < nt'):
        ctx.posterior_covariance(prob, P, Rf, K, Cm, with_gn=False)
    prob.free()


# ------------------------------------------------------------------------------------------------ c. real Gram matrices, class API
NT_C = 67
REAL = {
    'Nonlinear_elliptic': ['--N_domain', '150', '--N_boundary', '40', '--kernel_parameter', '0.2', '--nugget', '1e-6', '--GNsteps', '4'],
    'Burgers': ['--N_domain', '120', '--N_boundary', '42', '--nugget', '1e-5', '--GNsteps', '4'],
    'Eikonal': ['--N_domain', '120', '--N_boundary', '40', '--nugget', '1e-6', '--GNsteps', '4'],
    'Darcy_flow2d': ['--N_domain', '100', '--N_boundary', '40', '--N_data', '20', '--nugget', '1e-5', '--GNsteps', '4'],
}
QUIET = ['--print_hist', '', '--show_figure', '']
JITTER_D = 1e-6


def _solve(name):
    """(solver, cfg) of the class API at the sizes of REAL, seed fixed"""
    from _driver_common import solve_forward
    if name == 'Nonlinear_elliptic':
        import main_NonLinElliptic2d as drv
        cfg = drv.parse(REAL[name] + QUIET)
        u, f = drv.manufactured(cfg.alpha, cfg.m)
        np.random.seed(0)
        s, _ = solve_forward(cfg, name, u, f, drv.UNIT_SQUARE, solve_kwargs={'method': 'elimination'}, verbose=False)
    elif name == 'Eikonal':
        import main_Eikonal2d as drv
        cfg = drv.parse(REAL[name] + QUIET)
        np.random.seed(0)
        s, _ = solve_forward(cfg, name, lambda x1, x2: 0, lambda x1, x2: 1, drv.UNIT_SQUARE, verbose=False)
    elif name == 'Burgers':
        import main_Burgers1d as drv
        cfg = drv.parse(REAL[name] + QUIET)
        np.random.seed(0)
        s, _ = solve_forward(cfg, name, drv.initial_and_lateral, lambda x1, x2: 0, drv.SPACE_TIME, verbose=False)
    else:
        import main_DarcyFlow2d as drv
        from src.solver import solver_GP
        cfg = drv.parse(REAL[name] + QUIET)
        np.random.seed(0)
        s = solver_GP(cfg, PDE_type='Darcy_flow2d')
        s.set_equation(bdy=lambda x1, x2: 0, rhs=drv.source, domain=np.array(drv.UNIT_SQUARE), print_option=False)
        s.auto_sample_IP(cfg.N_domain, cfg.N_boundary, cfg.N_data, print_option=False)
        Xo = s.eqn.X_data
        s.get_observed_data(np.sin(np.pi * Xo[:, 0]) * np.sin(np.pi * Xo[:, 1]) / 20.0, cfg.noise_level, print_option=False)
        s.solve(print_option=False)
    return s, cfg


def _real_case(name, e, cfg):
    """the problem the device solved, on the oracle's Gram matrices, in the reference's shape"""
    Nd, Nb = e.N_domain, e.N_boundary
    if name == 'Darcy_flow2d':
        Tu, Ta = O.gram_matrix_assembly(e.X_domain, e.X_boundary, name, cfg.kernel, cfg.kernel_parameter)
        Tu, _ = O.add_nugget(Tu, 'Darcy_u', Nd, Nb, cfg.nugget)
        Ta, _ = O.add_nugget(Ta, 'Darcy_a', Nd, Nb, cfg.nugget)
        return PR.RealCase('darcy', Nd, Nb, e.rhs_f, e.bdy_g, float(e.noise_level), 0.0, Tu, Ta, data=e.data_u)
    T, _ = O.add_nugget(O.gram_matrix_assembly(e.X_domain, e.X_boundary, name, cfg.kernel, cfg.kernel_parameter), name, Nd, Nb, cfg.nugget)
    system = {'Nonlinear_elliptic': 'elliptic', 'Burgers': 'burgers', 'Eikonal': 'eikonal'}[name]
    p0, p1, _ = e._gn_params()
    return PR.RealCase(system, Nd, Nb, e.rhs_f, e.bdy_g, p0, p1, T)


class _Real:
    """one solve per configuration and its references, shared by the tests of c and d and left unchanged by them"""

    def __init__(self, name):
        self.name = name
        self.s, self.cfg = _solve(name)
        e = self.e = self.s.eqn
        rng = np.random.RandomState(42)
        lo, hi = np.asarray(e.domain, dtype=float).T
        self.Xt = lo + (hi - lo) * rng.uniform(0, 1, (NT_C, 2))
        self.darcy = name == 'Darcy_flow2d'
        self.tags = ('_u', '_a') if self.darcy else ('',)
        cs = _real_case(name, e, self.cfg)
        z = e._z_star[1]
        ld, f64 = cs.factors()
        prepared = PR.prepare_ld(cs, z, ld)
        Kt = O.construct_theta_test(self.Xt, e.X_domain, e.X_boundary, name, self.cfg.kernel, self.cfg.kernel_parameter)
        Ktt = CR.prior_ld(self.cfg.kernel, self.cfg.kernel_parameter, self.Xt)
        self.ref, self.err_np = {}, {}
        for field, t in enumerate(self.tags):
            K = (Kt[field] if self.darcy else Kt).T
            ref = CR.covariance_ld(cs, z, K, Ktt, field, ld, prepared)
            np64 = CR.covariance_np64(cs, z, K, Ktt.astype(np.float64), field, f64)
            self.ref[t] = ref
            self.err_np[t] = (float(np.max(np.abs(np64.cond.astype(LD) - ref.cond))),
                              float(np.max(np.abs((np64.cond + np64.gn).astype(LD) - ref.cov))))


@functools.lru_cache(maxsize=None)
def _real(name):
    return _Real(name)


def _public(e):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in e.__dict__.items() if not k.startswith('_')}


def _assert_unchanged(e, keep):
    for k, v in keep.items():                                          # arrays bit for bit
        w = e.__dict__[k]
        assert (_same(v, w) if isinstance(v, np.ndarray) and v.dtype == np.float64 else
                np.array_equal(v, w) if isinstance(v, np.ndarray) else v is w or v == w), k


@pytest.mark.parametrize('name', sorted(REAL))
def test_class_covariance_on_real_gram_matrices(name):
    rc = _real(name)
    e, Xt, tags = rc.e, rc.Xt, rc.tags
    e.extend_sol(Xt)
    e.posterior_variance(Xt)
    for n in ('extended_cov', 'extended_cov_cond', 'extended_samples'):
        for t in tags:
            e.__dict__.pop(n + t, None)                                # (what an earlier test of this file may have left)
    keep = _public(e)
    got = e.posterior_covariance(Xt)
    grab = lambda: {t: (getattr(e, 'extended_cov_cond' + t).copy(), getattr(e, 'extended_cov' + t).copy()) for t in tags}
    first = grab()
    assert all(got_t is getattr(e, 'extended_cov' + t) for got_t, t in zip(got if rc.darcy else (got,), tags))
    e.posterior_covariance(Xt)
    for t in tags:                                                     # a second call: the same bits
        assert all(_same(a, b) for a, b in zip(first[t], grab()[t]))
    _assert_unchanged(e, keep)
    added = {k for k in e.__dict__ if not k.startswith('_')} - set(keep)
    assert added == {n + t for n in ('extended_cov', 'extended_cov_cond') for t in tags}, added
    for t in tags:
        cc, c = first[t]
        ref, (err_c, err_np) = rc.ref[t], rc.err_np[t]
        assert cc.shape == c.shape == (NT_C, NT_C)
        assert _same(c, c.T) and _same(cc, cc.T)
        vmin = float(np.min(np.diag(ref.cov)))
        _say(f'real {name}{t}: numpy error cond {err_c:.3g}, whole {err_np:.3g}; min var {vmin:.3g}, max var {float(np.max(np.diag(ref.cov))):.3g}')
        assert max(err_c, err_np) < 1e-3 * vmin, 'precondition: the gate could hide a wrong result'
        dev_c, dev = float(np.max(np.abs(cc.astype(LD) - ref.cond))), float(np.max(np.abs(c.astype(LD) - ref.cov)))
        _say(f'real {name}{t}: device cond {dev_c:.3g} of {R.MARGIN * err_c:.3g}, whole {dev:.3g} of {R.MARGIN * err_np:.3g}')
        assert dev_c <= R.MARGIN * err_c and dev <= R.MARGIN * err_np, (name, t)
        # the diagonal against posterior_variance, within the same gate
        dvar = float(np.max(np.abs(np.diag(c) - getattr(e, 'extended_var' + t))))
        dvc = float(np.max(np.abs(np.diag(cc) - getattr(e, 'extended_var_cond' + t))))
        _say(f'real {name}{t}: diagonal against posterior_variance cond {dvc:.3g}, whole {dvar:.3g}')
        assert dvc <= R.MARGIN * err_c and dvar <= R.MARGIN * err_np, (name, t)


# ------------------------------------------------------------------------------------------------ d. samples
@pytest.mark.parametrize('name', sorted(REAL))
def test_samples_on_real_gram_matrices(name):
    from src._runtime import get_context
    rc = _real(name)
    e, Xt, tags, ctx = rc.e, rc.Xt, rc.tags, get_context()
    e.extend_sol(Xt)
    for t in tags:
        e.__dict__.pop('extended_samples' + t, None)
    keep = _public(e)
    ns = 5
    xis = [np.random.RandomState(7 + k).standard_normal((NT_C, ns)) for k in range(len(tags))]
    P, Rf, _, prob = e._posterior_state()
    for (t, field, layout), xi in zip(e._posterior_fields, xis):
        err_np = max(rc.err_np[t])
        _say(f'samples {name}{t}: N_t x numpy error {NT_C * err_np:.3g}, jitter / 4 {JITTER_D / 4:.3g}')
        assert NT_C * err_np < JITTER_D / 4, 'precondition: the jitter must dominate the error of Sigma'
        _, cov, dC = ctx.posterior_covariance_points(prob, P, Rf, field, layout or e._layout, e.kernel, e.kernel_parameter, Xt, e.X_domain,
                                                     e.X_boundary, keep=True)
        mean = getattr(e, 'extended_sol' + t)
        smp, info, L = ctx.posterior_sample(dC, mean, xi, JITTER_D, return_factor=True)
        dC.free()
        assert info == 0 and smp.shape == (NT_C, ns)
        assert np.all(np.triu(L, 1) == 0)                             # gpk_tril: the factor alone
        target = cov.astype(LD) + LD(JITTER_D) * np.eye(NT_C, dtype=LD)
        dev = float(np.max(np.abs(L.astype(LD) @ L.astype(LD).T - target)))
        bound = 32 * (NT_C + 1) * EPS * float(np.max(np.diag(target)))
        _say(f'factor {name}{t}: |L L^T - (Sigma + jitter I)| {dev:.3g}, bound {bound:.3g}')
        assert dev <= bound
        # sample = mean + L xi: the float64 product of N_t terms and one addition, entrywise (N_t + 2) eps (|mean| + |L| |xi|)
        want = mean.astype(LD)[:, None] + L.astype(LD) @ xi.astype(LD)
        scale = np.abs(mean)[:, None] + np.abs(L) @ np.abs(xi)
        ratio = float(np.max(np.abs(smp.astype(LD) - want) / (EPS * scale)))
        _say(f'sample {name}{t}: |sample - mean - L xi| / (eps (|mean| + |L||xi|)) {ratio:.3g}, bound {NT_C + 2}')
        assert ratio <= NT_C + 2
        # the class gives these very samples, transposed
        got = e.posterior_sample(Xt, n_samples=ns, xi=xis if rc.darcy else xis[0], jitter=JITTER_D)
        assert _same((got[field] if rc.darcy else got), smp.T)
    _assert_unchanged(e, keep)
    added = {k for k in e.__dict__ if not k.startswith('_')} - set(keep)
    assert added == {'extended_samples' + t for t in tags}, added
    # seeds and shapes
    grab = lambda: [getattr(e, 'extended_samples' + t).copy() for t in tags]
    e.posterior_sample(Xt, n_samples=3, seed=3, jitter=JITTER_D); a = grab()
    e.posterior_sample(Xt, n_samples=3, seed=3, jitter=JITTER_D); b = grab()
    e.posterior_sample(Xt, n_samples=3, seed=4, jitter=JITTER_D); c = grab()
    e.posterior_sample(Xt, jitter=JITTER_D, seed=3); one = grab()
    for x, y, z, o in zip(a, b, c, one):
        assert x.shape == (3, NT_C) and o.shape == (1, NT_C)
        assert _same(x, y) and not _same(x, z)
    if rc.darcy:                                                       # one generator: u first, then a
        rng = np.random.RandomState(3)
        xu, xa = rng.standard_normal((NT_C, 3)), rng.standard_normal((NT_C, 3))
        e.posterior_sample(Xt, n_samples=3, xi=(xu, xa), jitter=JITTER_D)
        assert all(_same(x, y) for x, y in zip(a, grab()))
    with pytest.raises(ValueError, match='N_test, n_samples'):
        e.posterior_sample(Xt, n_samples=2, xi=xis if rc.darcy else xis[0], jitter=JITTER_D)
    _assert_unchanged(e, keep)


def test_a_failed_pivot_leaves_out_unwritten_and_raises_at_class_level(dev_ctx, monkeypatch):
    from src._runtime import get_context
    ctx, nt, ns = dev_ctx, NT_C, 5
    xi = np.random.RandomState(0).standard_normal((nt, ns))
    v = VA.class_view(ctx, nt, ns, 'A')
    dC = ctx.array(-np.eye(nt))
    smp, info = ctx.posterior_sample(dC, np.zeros(nt), xi, JITTER_D, out=v)
    assert info == 1 and smp is None
    v.arena.assert_outside_untouched([])                               # the view itself included: nothing was written
    v.arena.free()
    rc = _real('Nonlinear_elliptic')
    cls_ctx = get_context()
    real = cls_ctx.posterior_covariance_points

    def minus_identity(*args, **kw):
        cc, c, d = real(*args, **kw)
        d.upload(-np.eye(d.rows))
        return cc, c, d
    monkeypatch.setattr(cls_ctx, 'posterior_covariance_points', minus_identity)
    with pytest.raises(RuntimeError, match=r'non-positive pivot at index 1 with jitter = 1e-06'):
        rc.e.posterior_sample(rc.Xt, n_samples=2, seed=0, jitter=JITTER_D)


# ------------------------------------------------------------------------------------------------ e. surface
def test_what_is_not_served_says_so():
    from src.PDEs import Nonlinear_elliptic2d, Nonlinear_elliptic3d
    one = lambda *x: 1.0
    Xt = np.full((3, 2), 0.5)
    for method in ('posterior_covariance', 'posterior_sample'):
        with pytest.raises(NotImplementedError, match='gpk_assemble_bc'):
            getattr(Nonlinear_elliptic2d(bdy=one, rhs=one, bc='robin'), method)(Xt)
        with pytest.raises(NotImplementedError, match='gpk_assemble_op'):
            getattr(Nonlinear_elliptic2d(bdy=one, rhs=one, operator=lambda x1, x2: (0, 0, 0, 1, 0, 1)), method)(Xt)
        with pytest.raises(NotImplementedError, match='three-dimensional'):
            getattr(Nonlinear_elliptic3d(bdy=one, rhs=one), method)(np.full((3, 3), 0.5))
    import main_NonLinElliptic2d as drv
    from _driver_common import solve_forward
    cfg = drv.parse(['--N_domain', '60', '--N_boundary', '20', '--GNsteps', '2'] + QUIET)
    u, f = drv.manufactured(cfg.alpha, cfg.m)
    np.random.seed(0)
    s, _ = solve_forward(cfg, 'Nonlinear_elliptic', u, f, drv.UNIT_SQUARE, solve_kwargs={'method': 'relaxation'}, verbose=False)
    for method in ('posterior_covariance', 'posterior_sample'):
        with pytest.raises(NotImplementedError, match='relaxed'):
            getattr(s.eqn, method)(Xt)
    s.eqn.GN_method(max_iter=2, print_hist=False)                      # the elimination solve of the same object is served
    Xt = np.random.RandomState(0).uniform(0.2, 0.8, (3, 2))
    assert s.eqn.posterior_covariance(Xt).shape == (3, 3)
    assert s.eqn.posterior_sample(Xt, n_samples=2, seed=0).shape == (2, 3)


def test_driver_flag(capsys):
    import main_NonLinElliptic2d as drv
    from src._runtime import get_context
    base = ['--N_domain', '150', '--N_boundary', '40', '--nugget', '1e-6'] + QUIET
    np.random.seed(0)
    drv.main(base)
    plain = capsys.readouterr().out
    np.random.seed(0)
    drv.main(base + ['--posterior_samples', '3', '--sample_seed', '1'])
    with_smp = capsys.readouterr().out
    pl, ws = plain.splitlines(), with_smp.splitlines()
    assert not any('samples' in line for line in pl)
    assert any('[Test error]' in line for line in pl)
    # the flag changes nothing in front of its own lines: every character of the default output, numbers included
    assert ws[:len(pl)] == pl, [(a, b) for a, b in zip(pl, ws) if a != b][:3]
    tag = lambda line: line.split(']')[0]
    assert [tag(x) for x in ws[len(pl):]] == ['[Testing posterior samples...', '[Test samples'], ws[len(pl):]
    last = ws[-1]
    assert last.startswith('[Test samples] 3 samples, RMS spread ') and ', max spread ' in last
    rms = float(last.split('RMS spread ')[1].split(',')[0])
    mx = float(last.split('max spread ')[1].split()[0])
    with capsys.disabled():
        _say(f'driver: {last}')
    assert 0 < rms <= mx
    get_context().synchronize()
