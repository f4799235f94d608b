#!/usr/bin/env python3
"""Write tests/golden/pdes_surface.json from the equation classes as they are in the tree: run it at the commit whose surface is to be
pinned (tests/test_pdes_surface.py holds what is recorded).

    python -B tests/golden/gen/make_pdes_surface.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
for p in (ROOT, os.path.join(ROOT, 'nonlinpdes-gpsolver_amd')):
    sys.path.insert(0, p)

from tests.test_pdes_surface import FIXTURE, surface  # noqa: E402

with open(FIXTURE, 'w') as f:
    json.dump(surface(), f, indent=1, sort_keys=True)
    f.write('\n')
print('wrote', FIXTURE)
