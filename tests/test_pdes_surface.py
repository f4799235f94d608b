"""The surface of the equation classes, pinned (no GPU): public names, signatures and the class attributes the device layer is
addressed with, against tests/golden/pdes_surface.json (written by tests/golden/gen/make_pdes_surface.py before the two elliptic
classes were put on one base; Semilinear2d, MongeAmpere2d and Semilinear3d added before the Gauss-Newton methods of the classes were
put on one driver and one mixin, the five earlier entries unchanged).  A refactoring of src/PDEs.py must reproduce it exactly."""
import inspect
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'pdes_surface.json')

CLASS_ATTRS = ('_layout', '_system', '_deriv_names', '_blocks_per_point')
OPTIONAL_ATTRS = ('_op_names', '_BC')


def _classes():
    from src import InverseProblems, PDEs
    return {'Nonlinear_elliptic2d': PDEs.Nonlinear_elliptic2d, 'Nonlinear_elliptic3d': PDEs.Nonlinear_elliptic3d,
            'Burgers': PDEs.Burgers, 'Eikonal': PDEs.Eikonal, 'Darcy_flow2d': InverseProblems.Darcy_flow2d,
            'Semilinear2d': PDEs.Semilinear2d, 'MongeAmpere2d': PDEs.MongeAmpere2d, 'Semilinear3d': PDEs.Semilinear3d}


def surface():
    """what the fixture holds, as JSON stores it (tuples as lists)"""
    classes = _classes()
    out = {}
    for name, cls in classes.items():
        public = sorted(n for n in dir(cls) if not n.startswith('_'))
        callables = [n for n in public if callable(getattr(cls, n))] + ['__init__']
        attrs = {a: getattr(cls, a) for a in CLASS_ATTRS}
        attrs.update({a: getattr(cls, a) for a in OPTIONAL_ATTRS if hasattr(cls, a)})
        out[name] = {'public': public, 'signatures': {n: str(inspect.signature(getattr(cls, n))) for n in callables}, 'attrs': attrs}
    e2, e3 = classes['Nonlinear_elliptic2d'], classes['Nonlinear_elliptic3d']
    out['relations'] = {'elliptic3d_is_subclass_of_elliptic2d': issubclass(e3, e2), 'elliptic2d_is_subclass_of_elliptic3d': issubclass(e2, e3)}
    return json.loads(json.dumps(out))


def test_surface_matches_the_fixture():
    want = json.load(open(FIXTURE))
    got = surface()
    assert sorted(got) == sorted(want)
    for name in want:
        for part in want[name]:
            assert got[name][part] == want[name][part], (name, part)
        assert got[name] == want[name], name


def test_fixture_covers_what_it_is_meant_to():
    want = json.load(open(FIXTURE))
    assert sorted(want) == sorted(list(_classes()) + ['relations'])
    assert want['relations'] == {'elliptic3d_is_subclass_of_elliptic2d': False, 'elliptic2d_is_subclass_of_elliptic3d': False}
    for name in _classes():
        assert set(CLASS_ATTRS) <= set(want[name]['attrs']) and '__init__' in want[name]['signatures'], name
        assert {'Gram_matrix', 'GN_method', 'extend_sol', 'sampled_pts'} <= set(want[name]['signatures']), name
    for name in ('Nonlinear_elliptic2d', 'Nonlinear_elliptic3d'):
        assert set(OPTIONAL_ATTRS) <= set(want[name]['attrs']), name
