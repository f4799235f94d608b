"""Times gpk_extend against gpk_extend_functionals (value only, and all five functionals) at the config-2 point sets of BASELINE
(elliptic layout, N_domain 4000 + N_boundary 400 = M 4400 column points, Theta order N = 8400), for Nt = 3600 (the drivers' 60 x 60 grid)
and Nt = 90000 test points.  HIP events around `reps` back-to-back launches after a warm-up; prints ms per call, (test, column) pairs
per second, and the fraction of the fp64 vector rate (78.6 TFLOP/s, datasheet) at an ESTIMATED operation count per pair:
    distance + exponent 6, the fp64 exp sequence ~20, two Hermite evaluations 16  = 42 shared by all functionals,
    + ~8 per functional (pair coefficients of the 2 column blocks, coefficient products, the exp factor, the accumulation).
One line of JSON per case; --out FILE also writes them there.

    python tools/extend_functionals_probe.py [--reps 20] [--out probe.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'nonlinpdes-gpsolver_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

FP64_VECTOR_PEAK = 78.6e12
BASE_OPS, PER_FUNCTIONAL_OPS = 42, 8


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--nt', type=int, nargs='+', default=[3600, 90000])
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    import gpk
    ctx = gpk.Context(0)
    lib = ctx.lib
    rng = np.random.RandomState(0)
    Nd, Nb = 4000, 400
    Xd = rng.uniform(0, 1, (Nd, 2)); Xb = rng.uniform(0, 1, (Nb, 2))
    N, M = 2 * Nd + Nb, Nd + Nb
    coeff = ctx.array(rng.normal(size=N))
    dXd, dXb = ctx.points(Xd), ctx.points(Xb)
    kp = (C.c_double * 2)(0.2, 0.0)
    rows = []
    for Nt in a.nt:
        g = int(np.ceil(np.sqrt(Nt)))
        t = np.linspace(0, 1, g)
        Xt = np.stack(np.meshgrid(t, t), -1).reshape(-1, 2)[:Nt]
        dXt = ctx.points(Xt)
        out = ctx.empty(5, Nt, ld=Nt)
        calls = {
            'gpk_extend': lambda: lib.gpk_extend(ctx.h, 0, 0, kp, dXt.ptr, Nt, dXd.ptr, Nd, dXb.ptr, Nb, coeff.ptr, out.ptr),
            'functionals value': lambda: lib.gpk_extend_functionals(ctx.h, 0, 0, kp, dXt.ptr, Nt, dXd.ptr, Nd, dXb.ptr, Nb, coeff.ptr, 1,
                                                                    out.ptr, Nt),
            'functionals all five': lambda: lib.gpk_extend_functionals(ctx.h, 0, 0, kp, dXt.ptr, Nt, dXd.ptr, Nd, dXb.ptr, Nb, coeff.ptr,
                                                                       31, out.ptr, Nt),
        }
        nfun = {'gpk_extend': 1, 'functionals value': 1, 'functionals all five': 5}
        for name, fn in calls.items():
            for _ in range(3):
                assert fn() == 0
            ctx.synchronize()
            ctx.timer_start()
            for _ in range(a.reps):
                fn()
            ms = ctx.timer_stop() / a.reps
            pairs = float(Nt) * M
            ops = pairs * (BASE_OPS + PER_FUNCTIONAL_OPS * nfun[name])
            row = dict(case=name, Nt=Nt, M=M, ms=round(ms, 4), pairs_per_s=pairs / (ms * 1e-3),
                       est_fp64_fraction=round(ops / (ms * 1e-3) / FP64_VECTOR_PEAK, 3))
            rows.append(row)
            print(json.dumps(row), flush=True)
        out.free(); dXt.free()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(rows, f, indent=1)
    ctx.close()


if __name__ == '__main__':
    main()
