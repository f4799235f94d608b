"""Times the posterior-covariance entry points with HIP events ("Posterior covariance and samples"):
gpk_assemble_prior, one batch of gpk_posterior_covariance (without and with the Gauss-Newton term) and gpk_posterior_sample -- each whole
call, and the phases of the covariance issued one by one through the public dense entry points.  Warm calls, median of --reps.  Default
size: BASELINE config 2 (elliptic, N_d 4000, N_b 400: N 8400, n_z 4000), one batch of 1024 test points, 16 samples.

    python tools/posterior_cov_timing.py [--Nd 4000 --Nb 400 --nt 1024 --ns 16 --reps 12]
"""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'nonlinpdes-gpsolver_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--Nd', type=int, default=4000)
    ap.add_argument('--Nb', type=int, default=400)
    ap.add_argument('--nt', type=int, default=1024)
    ap.add_argument('--ns', type=int, default=16)
    ap.add_argument('--reps', type=int, default=12)
    ap.add_argument('--sigma', type=float, default=0.2)
    ap.add_argument('--nugget', type=float, default=1e-8)
    ap.add_argument('--jitter', type=float, default=1e-5)
    a = ap.parse_args(argv)
    import gpk
    from oracle import gp_oracle as O
    ctx = gpk.Context(0)
    rng = np.random.RandomState(0)
    Nd, Nb, nt, ns = a.Nd, a.Nb, a.nt, a.ns
    Xd, Xb, Xt = rng.uniform(0, 1, (Nd, 2)), rng.uniform(0, 1, (Nb, 2)), rng.uniform(0, 1, (nt, 2))
    T, _ = ctx.assemble('Nonlinear_elliptic', 'Gaussian', a.sigma, Xd, Xb, a.nugget, 'adaptive')
    info = ctx.potrf(T)
    prob = gpk.GNProblem(ctx, 'Nonlinear_elliptic', Nd, Nb, O.elliptic_rhs(Xd[:, 0], Xd[:, 1]), O.elliptic_truth(Xb[:, 0], Xb[:, 1]), T, p0=1.0, p1=3.0)
    z = ctx.array(O.elliptic_truth(Xd[:, 0], Xd[:, 1]))
    N, nz = prob.rows, prob.nz
    P, R, pinfo = ctx.posterior_prepare(prob, z)
    print(f'N {N}, n_z {nz}, nt {nt}, ns {ns}, potrf info {info}, prepare info {pinfo}, dinv block {prob.struct.dinv_block}')

    def timed(fn, before=None):
        ms = []
        for _ in range(a.reps + 2):
            if before:
                before()
            ctx.synchronize()
            ctx.timer_start()
            fn()
            ms.append(ctx.timer_stop())
        return statistics.median(ms[2:])

    dXt, dXd, dXb = ctx.points(Xt), ctx.points(Xd), ctx.points(Xb)
    K, V, W, Cm = ctx.empty(N, nt), ctx.empty(N, nt), ctx.empty(nz, nt), ctx.empty(nt, nt)
    kp = gpk.device.kernel_params('Gaussian', a.sigma)
    S = prob.struct
    cross = lambda: ctx._chk(ctx.lib.gpk_assemble_cross(ctx.h, 0, 0, kp, dXt.ptr, nt, dXd.ptr, Nd, dXb.ptr, Nb, K.ptr, K.ld))
    prior = lambda: ctx._chk(ctx.lib.gpk_assemble_prior(ctx.h, 0, kp, dXt.ptr, nt, dXt.ptr, nt, Cm.ptr, Cm.ld))
    t = timed(prior)
    print(f'gpk_assemble_prior ({nt} x {nt})   {t:8.3f} ms   {8e-9 * nt * nt / t:6.2f} TB/s written')

    def cov(gn):
        return lambda: ctx._chk(ctx.lib.gpk_posterior_covariance(ctx.h, ctypes.byref(S), P.ptr, P.ld, R.ptr, R.ld, 0, K.ptr, K.ld, nt,
                                                                 W.ptr, W.ld, Cm.ptr, Cm.ld, gn))
    refill = lambda: (prior(), cross())
    flops_c = N * N * nt + N * nt * nt
    flops = flops_c + 2 * N * nz * nt + nz * nz * nt + nz * nt * nt
    t = timed(cov(0), before=refill)
    print(f'gpk_posterior_covariance, with_gn = 0   {t:8.3f} ms   {1e-9 * flops_c / t:6.2f} TFLOP/s')
    t = timed(cov(1), before=refill)
    print(f'gpk_posterior_covariance, with_gn = 1   {t:8.3f} ms   {1e-9 * flops / t:6.2f} TFLOP/s')
    t = timed(lambda: (prior(), cross(), cov(1)()))
    print(f'prior + cross + covariance, one batch   {t:8.3f} ms   {1e-9 * flops / t:6.2f} TFLOP/s')
    phases = [
        ('1 V = L^-1 K (gpk_trsm_dinv)', lambda: ctx.trsm_dinv(prob.L, prob.Dinv, K, V, n=N, nrhs=nt), N * N * nt),
        ('2 C -= V^T V (gpk_syrk, lower)', lambda: ctx.syrk(nt, N, -1.0, V, 1.0, Cm), N * nt * nt),
        ('3 W = P^T V (gpk_gemm)', lambda: ctx.gemm(True, False, nz, nt, N, 1.0, P, V, 0.0, W), 2 * N * nz * nt),
        ('4 W <- R^-1 W (gpk_trsm)', lambda: ctx.trsm(R, W, n=nz, nrhs=nt), nz * nz * nt),
        ('5 C += W^T W (gpk_syrk, lower)', lambda: ctx.syrk(nt, nz, 1.0, W, 1.0, Cm), nz * nt * nt),
        ('6 gpk_symmetrize_lower', lambda: ctx.symmetrize(Cm, nt), 0),
    ]
    # the solve leaves K as scratch and phase 4 solves W in place: both are refilled (evaluator / product) outside the timed region
    before = {0: cross, 3: phases[2][1]}
    for k, (name, fn, fl) in enumerate(phases):
        prior()
        cross()
        phases[0][1]()                                               # V for the phases behind the solve
        t = timed(fn, before=before.get(k))
        print(f'  {name:34s} {t:8.3f} ms' + (f'   {1e-9 * fl / t:6.2f} TFLOP/s' if fl else ''))
    # samples: the factorisation of Sigma + jitter I and the product with ns columns of normals (Sigma is rebuilt outside the timed region)
    mean, xi, out = ctx.array(np.zeros(nt)), ctx.array(rng.standard_normal((nt, ns))), ctx.empty(nt, ns, ld=gpk.device.pad_ld(ns))
    sinfo = ctypes.c_int()
    sample = lambda: ctx._chk(ctx.lib.gpk_posterior_sample(ctx.h, Cm.ptr, Cm.ld, nt, a.jitter, mean.ptr, xi.ptr, xi.ld, ns, out.ptr, out.ld,
                                                           ctypes.byref(sinfo)))
    t = timed(sample, before=lambda: (prior(), cross(), cov(1)()))
    print(f'gpk_posterior_sample ({ns} samples)   {t:8.3f} ms   info {sinfo.value}   {1e-9 * (nt ** 3 / 3 + 2 * nt * nt * ns) / t:6.2f} TFLOP/s '
          '(one host read of the pivot status included)')
    ctx.close()


if __name__ == '__main__':
    main()
