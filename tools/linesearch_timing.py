"""Times one gpk_gn_step_ls next to one gpk_gn_step on the same handle state ("Line search"), for K = 4, 8, 16 trial
steps.  Both calls are synchronous (they return host scalars), so each is timed with the host clock between two synchronisations: launch
latency and the final copy are part of the figure.  Every timed call starts from the same iterate (one device copy of z, included in both
figures).  Warm calls, median of --reps.  Default size: BASELINE config 2 (elliptic, N_d 4000, N_b 400: N 8400, n_z 4000).  No gate.

    python tools/linesearch_timing.py [--Nd 4000 --Nb 400 --reps 10]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'nonlinpdes-gpsolver_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--Nd', type=int, default=4000)
    ap.add_argument('--Nb', type=int, default=400)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--sigma', type=float, default=0.2)
    ap.add_argument('--nugget', type=float, default=1e-8)
    a = ap.parse_args(argv)
    import gpk
    from oracle import gp_oracle as O
    ctx = gpk.Context(0)
    rng = np.random.RandomState(0)
    Nd, Nb = a.Nd, a.Nb
    Xd, Xb = O.sampled_pts_rdm(Nd, Nb, np.array([[0, 1], [0, 1]]), rng=rng)
    T, _ = ctx.assemble('Nonlinear_elliptic', 'Gaussian', a.sigma, Xd, Xb, a.nugget, 'adaptive')
    info = ctx.potrf(T)
    prob = gpk.GNProblem(ctx, 'Nonlinear_elliptic', Nd, Nb, O.elliptic_rhs(Xd[:, 0], Xd[:, 1]), O.elliptic_truth(Xb[:, 0], Xb[:, 1]), T, p0=1.0, p1=3.0)
    z = ctx.array(rng.normal(size=Nd))
    ctx.gn_step(prob, z)                                             # one step away from the random start: the iterate every timed call starts from
    zc = ctx.array(z.download())
    prob.trial_workspace(16)
    print(f'N {prob.rows}, n_z {prob.nz}, potrf info {info}')

    def timed(fn):
        ms = []
        for _ in range(a.reps + 3):
            ctx.synchronize()
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0))
        return statistics.median(ms[3:]), min(ms[3:]), max(ms[3:])

    def step():
        ctx._chk(ctx.lib.gpk_memcpy_d2d(ctx.h, zc.ptr, z.ptr, Nd * 8))
        ctx.gn_step(prob, zc)

    def step_ls(K):
        def fn():
            ctx._chk(ctx.lib.gpk_memcpy_d2d(ctx.h, zc.ptr, z.ptr, Nd * 8))
            fn.out = ctx.gn_step_ls(prob, zc, trials=K)
        return fn

    calls = [('gpk_gn_step (+ one copy of z)', step)] + [(f'gpk_gn_step_ls K = {K} (+ one copy of z)', step_ls(K)) for K in (4, 8, 16)]
    base = None
    for name, fn in calls:
        med, lo, hi = timed(fn)
        base = med if base is None else base
        extra = '' if fn is step else f'   + {med - base:6.3f} ms   accepted k = {fn.out[2]}'
        print(f'{name:44s} {med:8.3f} ms  (min {lo:.3f}, max {hi:.3f}){extra}')
    ctx.close()


if __name__ == '__main__':
    main()
