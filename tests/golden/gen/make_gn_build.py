#!/usr/bin/env python3
"""Write tests/golden/gn_build.npz: [A(z) | F(z)] as gpk_gn_build and gpk_gn_build_rev write them on the device, for the cases and
the seeded inputs of tests/test_gpu_gn_build_pinned.py.  Needs an MI355X and the built libraries; run it at the commit whose build
output is to be pinned -- only when a system's arithmetic is changed on purpose.

    python -B tests/golden/gen/make_gn_build.py [output.npz]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
while not os.path.exists(os.path.join(ROOT, '__graft_entry__.py')):
    ROOT = os.path.dirname(ROOT)
for p in (ROOT, os.path.join(ROOT, 'nonlinpdes-gpsolver_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

import gpk  # noqa: E402
import test_gpu_gn_build_pinned as T  # noqa: E402

out = {'cases': np.array(json.dumps({k: list(v) for k, v in T.CASES.items()}))}
ctx = gpk.Context(0, dev=True)
for name, Nd, Nb in T.KEYS:
    k = T.key_of(name, Nd, Nb)
    inp = T.make_inputs(name, Nd, Nb)
    built, prob, _ = T.build_outputs(ctx, name, Nd, Nb, inp)
    prob.free()
    for part, v in inp.items():
        out[f'{k}/in/{part}'] = v
    for tag, res in built.items():
        for part, v in res.items():
            out[f'{k}/{tag}/{part}'] = v
    print(k, {tag: int(res['vals'].size) for tag, res in built.items()})
ctx.close()
path = sys.argv[1] if len(sys.argv) > 1 else T.FIXTURE
np.savez_compressed(path, **out)
print('wrote', path, os.path.getsize(path), 'bytes')
