"""Times the posterior-variance entry points with HIP events ("Posterior variance"): gpk_assemble_cross,
gpk_col_sumsq, gpk_posterior_prepare and one batch of gpk_posterior_variance -- the whole call and its phases issued one by one through
the public dense entry points.  Warm calls, median of --reps.  Default size: BASELINE config 2 (elliptic, N_d 4000, N_b 400: N 8400,
n_z 4000), one batch of 1024 test points.

    python tools/posterior_timing.py [--Nd 4000 --Nb 400 --nt 1024 --reps 12]
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
    ap.add_argument('--reps', type=int, default=12)
    ap.add_argument('--sigma', type=float, default=0.2)
    ap.add_argument('--nugget', type=float, default=1e-8)
    a = ap.parse_args(argv)
    import gpk
    from oracle import gp_oracle as O
    ctx = gpk.Context(0)
    rng = np.random.RandomState(0)
    Nd, Nb, nt = a.Nd, a.Nb, a.nt
    Xd, Xb, Xt = rng.uniform(0, 1, (Nd, 2)), rng.uniform(0, 1, (Nb, 2)), rng.uniform(0, 1, (nt, 2))
    T, _ = ctx.assemble('Nonlinear_elliptic', 'Gaussian', a.sigma, Xd, Xb, a.nugget, 'adaptive')
    info = ctx.potrf(T)
    prob = gpk.GNProblem(ctx, 'Nonlinear_elliptic', Nd, Nb, O.elliptic_rhs(Xd[:, 0], Xd[:, 1]), O.elliptic_truth(Xb[:, 0], Xb[:, 1]), T, p0=1.0, p1=3.0)
    z = ctx.array(O.elliptic_truth(Xd[:, 0], Xd[:, 1]))
    N, nz = prob.rows, prob.nz
    print(f'N {N}, n_z {nz}, nt {nt}, potrf info {info}, dinv block {prob.struct.dinv_block}')

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
    K = ctx.empty(N, nt)
    kp = gpk.device.kernel_params('Gaussian', a.sigma)
    cross = lambda: ctx._chk(ctx.lib.gpk_assemble_cross(ctx.h, 0, 0, kp, dXt.ptr, nt, dXd.ptr, Nd, dXb.ptr, Nb, K.ptr, K.ld))
    t = timed(cross)
    print(f'gpk_assemble_cross      {t:8.3f} ms   {8e-9 * N * nt / t:6.2f} TB/s written')
    V, W, out = ctx.empty(N, nt), ctx.empty(nz, nt), ctx.empty(nt)
    t = timed(lambda: ctx._chk(ctx.lib.gpk_col_sumsq(ctx.h, K.ptr, N, nt, K.ld, 1.0, None, out.ptr)))
    print(f'gpk_col_sumsq ({N} rows) {t:8.3f} ms   {8e-9 * N * nt / t:6.2f} TB/s read')
    holder = {}

    def prepare():
        for x in holder.pop('PR', ()):
            x.free()
        P, R, _ = ctx.posterior_prepare(prob, z)
        holder['PR'] = (P, R)
    t = timed(prepare)
    print(f'gpk_posterior_prepare   {t:8.3f} ms   {1e-9 * (N * N * nz + N * nz * nz + nz ** 3 / 3) / t:6.2f} TFLOP/s (dense counts N^2 nz + N nz^2 + nz^3/3)')
    P, R = holder['PR']
    vc, v = ctx.empty(nt), ctx.empty(nt)
    S = prob.struct

    def whole():
        cross()
        ctx._chk(ctx.lib.gpk_posterior_variance(ctx.h, ctypes.byref(S), P.ptr, P.ld, R.ptr, R.ld, 0, K.ptr, K.ld, nt, W.ptr, W.ld, vc.ptr, v.ptr))
    t_whole = timed(whole)
    print(f'cross + gpk_posterior_variance, one batch   {t_whole:8.3f} ms   {1e-9 * (N * N * nt + 2 * N * nz * nt + nz * nz * nt) / t_whole:6.2f} TFLOP/s')
    phases = [
        ('1 V = L^-1 K (gpk_trsm_dinv)', lambda: ctx.trsm_dinv(prob.L, prob.Dinv, K, V, n=N, nrhs=nt), N * N * nt),
        ('2 var_cond (gpk_col_sumsq)', lambda: ctx._chk(ctx.lib.gpk_col_sumsq(ctx.h, V.ptr, N, nt, V.ld, -1.0, None, vc.ptr)), 0),
        ('3 W = P^T V (gpk_gemm)', lambda: ctx.gemm(True, False, nz, nt, N, 1.0, P, V, 0.0, W), 2 * N * nz * nt),
        ('4 W <- R^-1 W (gpk_trsm)', lambda: ctx.trsm(R, W, n=nz, nrhs=nt), nz * nz * nt),
        ('5 var (gpk_col_sumsq)', lambda: ctx._chk(ctx.lib.gpk_col_sumsq(ctx.h, W.ptr, nz, nt, W.ld, 1.0, vc.ptr, v.ptr)), 0),
    ]
    # the solve leaves K as scratch and phase 4 solves W in place: both are refilled (evaluator / product) outside the timed region
    refill = {0: cross, 3: phases[2][1]}
    for k, (name, fn, flops) in enumerate(phases):
        cross()
        phases[0][1]()                                               # V for the phases behind the solve
        t = timed(fn, before=refill.get(k))
        print(f'  {name:34s} {t:8.3f} ms' + (f'   {1e-9 * flops / t:6.2f} TFLOP/s' if flops else ''))
    ctx.close()


if __name__ == '__main__':
    main()
