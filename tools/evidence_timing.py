"""Times one gpk_log_evidence next to one gpk_gn_step and the calls it is made of ("Log evidence"):
gpk_posterior_prepare, gpk_gn_loss and gpk_chol_logdet on the factor of Theta.  Every call is synchronous (it returns host scalars),
so each is timed with the host clock between two synchronisations: launch latency and the final copy are part of the figure.  Warm
calls, median of --reps.  Default size: BASELINE config 2 (elliptic, N_d 4000, N_b 400: N 8400, n_z 4000).

    python tools/evidence_timing.py [--Nd 4000 --Nb 400 --reps 10]
"""
import argparse
import ctypes as C
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
    for _ in range(4):                                               # four Gauss-Newton steps: the iterate the evidence is taken at
        ctx.gn_step(prob, z)
    terms, P, R, einfo = ctx.log_evidence(prob, z)
    print(f'N {prob.rows}, n_z {prob.nz}, potrf info {info}, H/2 info {einfo}, log Z {terms["log_Z"]:.10g}')

    def timed(fn):
        ms = []
        for _ in range(a.reps + 2):
            ctx.synchronize()
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0))
        return statistics.median(ms[2:])

    S, work = prob.struct, prob.workspace()[3]
    zc = ctx.array(z.download())                                     # the step moves its iterate: every timed step starts from z
    out, inf = (C.c_double * 6)(), C.c_int()

    def step():
        ctx._chk(ctx.lib.gpk_memcpy_d2d(ctx.h, zc.ptr, z.ptr, Nd * 8))
        ctx.gn_step(prob, zc)
    calls = [
        ('gpk_gn_step (+ one copy of z)', step),
        ('gpk_log_evidence', lambda: ctx._chk(ctx.lib.gpk_log_evidence(ctx.h, C.byref(S), z.ptr, P.ptr, P.ld, R.ptr, R.ld, work.ptr, out, C.byref(inf)))),
        ('  gpk_posterior_prepare', lambda: ctx._chk(ctx.lib.gpk_posterior_prepare(ctx.h, C.byref(S), z.ptr, P.ptr, P.ld, R.ptr, R.ld, C.byref(inf)))),
        ('  gpk_gn_loss', lambda: ctx.gn_loss(prob, z)),
        (f'  gpk_chol_logdet (order {T.rows})', lambda: ctx.chol_logdet(T)),
    ]
    for name, fn in calls:
        print(f'{name:36s} {timed(fn):8.3f} ms')
    ctx.close()


if __name__ == '__main__':
    main()
