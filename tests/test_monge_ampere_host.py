"""Host side of the Monge-Ampere feature, no GPU: the reference of tests/_monge_ampere_reference.py against sympy, the trace ratios, the
identity behind the convex-branch form, the Jacobian, the convergence of the float64 reference iteration, the binding against the header,
the class surface, the facade and the driver's parser."""
import ctypes
import os
import re

import numpy as np
import pytest

import _monge_ampere_reference as MA
from oracle import gp_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = MA.LD
PARAMS = {'Gaussian': 0.3, 'anisotropic_Gaussian': (0.3, 0.07)}


# ------------------------------------------------------------------------------------------------ 1. the table against sympy
@pytest.mark.parametrize('kernel', MA.KERNELS)
def test_table_equals_sympy_differentiation(kernel):
    import sympy as sp
    kp = PARAMS[kernel]
    x1, x2, y1, y2 = sp.symbols('x1 x2 y1 y2', real=True)
    s = [sp.Rational(*float(v).as_integer_ratio()) for v in np.atleast_1d(kp)]    # (the float64 parameter, exactly)
    p = (1 / s[0] ** 2, 1 / s[0] ** 2) if kernel == 'Gaussian' else (2 / s[0] ** 2, 2 / s[1] ** 2)
    kappa = sp.exp(-(p[0] * (x1 - y1) ** 2 + p[1] * (x2 - y2) ** 2) / 2)

    def apply(name, e, a, b):
        if name == 'D':
            return sp.diff(e, a, 2) - sp.diff(e, b, 2)
        if name == 'M':
            return 2 * sp.diff(e, a, b)
        if name == 'L':
            return sp.diff(e, a, 2) + sp.diff(e, b, 2)
        return e
    rng = np.random.RandomState(11)
    pts = [tuple(rng.uniform(0, 1, 4)) for _ in range(4)] + [(0.25, 0.75, 0.25, 0.75), (0.5, 0.125, 0.5, 0.375)]
    worst = 0.0
    for f in MA.NAMES:
        for g in MA.NAMES:
            expr = apply(f, apply(g, kappa, y1, y2), x1, x2)
            for pt in pts:
                # the coordinates as the exact rationals of their float64 values: the reference forms d from those
                sub = {v: sp.Rational(*float(c).as_integer_ratio()) for v, c in zip((x1, x2, y1, y2), pt)}
                want = float(expr.subs(sub).evalf(40))
                t, _ = MA.table(kernel, kp, *(np.array([c]) for c in pt))
                got, mag = (float(v[0]) for v in t[(f, g)])
                assert mag >= abs(got) * (1 - 1e-15)
                if mag == 0.0:
                    assert want == 0.0
                    continue
                worst = max(worst, abs(got - want) / mag)
                assert abs(got - want) <= 4 * MA.EPS * mag, (f, g, pt, got, want)          # (float() of both sides: 2 roundings)
    print(f'\n[monge-ampere host] {kernel}: worst |table - sympy| / magnitude sum = {worst / MA.EPS:.3g} eps')


# ------------------------------------------------------------------------------------------------ 2. trace ratios
@pytest.mark.parametrize('kernel', MA.KERNELS)
def test_trace_ratios_equal_the_closed_forms(kernel):
    kp = PARAMS[kernel]
    Nd, Nb = 7, 3
    Xd, Xb = MA.points(Nd, 4)[0][:Nd], MA.points(8, 4)[1][:Nb]
    T = MA.theta(kernel, kp, Xd, Xb)[0]
    d = np.diag(T)
    tr = [np.sum(d[o:o + n]) for o, n in MA.offsets(Nd, Nb)]
    p1, p2 = (float(v) for v in MA.GR.precisions(kernel, kp))
    closed = [3 * p1 * p1 - 2 * p1 * p2 + 3 * p2 * p2, 4 * p1 * p2, 3 * p1 * p1 + 2 * p1 * p2 + 3 * p2 * p2]
    for k in range(3):
        assert abs(float(tr[k] / tr[3]) - Nd * closed[k] / (Nd + Nb)) <= 1e-14 * Nd * closed[k] / (Nd + Nb)
        assert abs(float(MA.trace_ratios(kernel, kp, Nd, Nb)[k] - tr[k] / tr[3])) <= 1e-17 * float(tr[k] / tr[3])
    Tn = MA.theta_nugget(kernel, kp, Xd, Xb, 1e-6)
    assert float(Tn[0, 0] - T[0, 0]) == pytest.approx(1e-6 * Nd * closed[0] / (Nd + Nb), rel=1e-12)
    assert float(Tn[-1, -1] - T[-1, -1]) == pytest.approx(1e-6, rel=1e-12)


# ------------------------------------------------------------------------------------------------ 3. identity and Jacobian
def test_identity_and_jacobian():
    rng = np.random.RandomState(4)
    h11, h12, h22 = rng.normal(size=(3, 50))
    Du, Mu, Lu = h11 - h22, 2 * h12, h11 + h22
    assert np.allclose(Lu ** 2 - Du ** 2 - Mu ** 2, 4 * (h11 * h22 - h12 ** 2), rtol=0, atol=1e-13)
    Nd, Nb = 6, 3
    f, g = rng.uniform(0.5, 1.5, Nd), rng.normal(size=Nb)
    z = rng.normal(size=3 * Nd)
    Az = MA.A(f, Nb, z)
    h = 1e-6
    for j in range(3 * Nd):
        e = np.zeros(3 * Nd); e[j] = h
        fd = (MA.F(f, g, z + e) - MA.F(f, g, z - e)) / (2 * h)
        assert np.max(np.abs(fd - Az[:, j])) <= 1e-8
    assert np.count_nonzero(Az) == 5 * Nd and Az.shape == (4 * Nd + Nb, 3 * Nd)
    first = np.array([np.nonzero(Az[:, j])[0][0] for j in range(3 * Nd)])            # v0 does not enter the PDE row
    assert np.array_equal(first, np.concatenate([3 * Nd + np.arange(Nd), np.arange(Nd), Nd + np.arange(Nd)]))


def test_vector_reference_and_its_gates_at_the_pipelined_size():
    """N_d = 342, N_b = 40 (n_z + 1 = 1027; tests/test_gpu_fused_phase.py section e): the vector-only reference against the full form at
    N_d = 65 (two long-double evaluations in different orders), its refined delta's residual at the long-double rounding level; the
    float64 pipeline passes the gates, a delta moved by 1e-11 and a loss off by 1e-11 do not"""
    R = MA.R
    full, small = MA.full_reference(65, 13), MA.vector_reference(65, 13)
    gn = float(np.linalg.norm(full.g.astype(np.float64)))
    assert abs(small.loss - full.loss) <= 0.05 * R.EPS * full.loss
    assert np.linalg.norm((small.g - full.g).astype(np.float64)) <= 0.05 * R.EPS * gn
    dn = float(np.linalg.norm(full.delta.astype(np.float64)))
    assert np.linalg.norm((small.apply_H(full.delta) - full.H @ full.delta).astype(np.float64)) <= 0.05 * R.EPS * (full.normH * dn + gn)
    assert np.linalg.norm((small.delta - full.delta).astype(np.float64)) <= 0.05 * R.EPS * full.cond * dn
    vec = MA.vector_reference(342, 40)
    cs, p, d = vec.case, vec.p64, vec.delta
    assert cs.nz + 1 == 1027
    scale = vec.normH * float(np.linalg.norm(d.astype(np.float64))) + float(np.linalg.norm(vec.g.astype(np.float64)))
    assert np.linalg.norm(vec.residual(d).astype(np.float64)) <= 1e-3 * R.EPS * scale
    for gate, v in ((R.gate_loss, p.loss), (R.gate_backward_vec, p.delta), (R.gate_forward, p.delta)):
        r, a = gate(vec, v)
        assert r <= a, (gate.__name__, r, a)
    u = np.random.RandomState(342).normal(size=cs.nz); u /= np.linalg.norm(u)
    moved = p.delta + 1e-11 * np.linalg.norm(p.delta) * u
    print()
    for gate, v in ((R.gate_backward_vec, moved), (R.gate_forward, moved), (R.gate_loss, p.loss * (1 + 1e-11))):
        r, a = gate(vec, v)
        print(f'[monge-ampere host] moved by 1e-11: {gate.__name__} {r:.3g}, allowed {a:.3g}: fails by a factor {r / a:.3g}')
        assert r > a, (gate.__name__, r, a)


# ------------------------------------------------------------------------------------------------ 4. the reference iteration converges
# 3.66e-6 after 8 steps on the point set of the issue; 1e-4 asks for that order of magnitude with room for another point set, a system
# that fails stays above 1e-2.  Measured on the points of MA.points (printed below): L2 8.27e-07 from both starts, loss
# 27.5454945 from step 5 / 7 on.
def test_reference_iteration_converges():
    Nd, Nb = 300, 80
    Xd, Xb = MA.points(Nd, Nb)
    L = O.cholesky(MA.gram_float64('Gaussian', 0.3, Xd, Xb, 1e-8))
    sysm = MA.System(MA.rhs(Xd[:, 0], Xd[:, 1]), MA.truth(Xb[:, 0], Xb[:, 1]))
    us = MA.truth(Xd[:, 0], Xd[:, 1])
    for name, start in (('zero', np.zeros(3 * Nd)), ('N(0,1)', np.random.RandomState(1).normal(size=3 * Nd))):
        z, hist = MA.gn_float64(sysm, L, start, 10)
        l2 = float(np.sqrt(np.mean((z[:Nd] - us) ** 2)))
        print(f'\n[monge-ampere host] start {name}: L2 error {l2:.3g}, loss history {[float("%.9g" % v) for v in hist]}')
        assert l2 < 1e-4
        assert max(abs(hist[k] - hist[10]) for k in (7, 8, 9)) <= 1e-6 * abs(hist[10])


# ------------------------------------------------------------------------------------------------ 5. binding and header
def test_binding_matches_the_header():
    import gpk
    import gpk._lib as L
    hdr = open(os.path.join(ROOT, 'include', 'gpk.h')).read()
    assert re.search(r'GPK_GN_MONGE_AMPERE = 6', hdr) and gpk.SYSTEM['MongeAmpere2d'] == 6
    for name in ('gpk_assemble_hess', 'gpk_extend_functionals_hess', 'gpk_pde_residual_ma'):
        assert f'int {name}(' in hdr and name in gpk.declared_symbols() and name in gpk.declared_symbols(dev=True)
    body = re.search(r'typedef struct \{(.*?)\} gpk_gn_problem;', hdr, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = []
    for decl in filter(None, (d.strip() for d in body.split(';'))):
        m = re.match(r'(const\s+double\s*\*|int|double)\s*(.*)', decl)
        names += [(n.strip().lstrip('*').strip(), {'int': ctypes.c_int, 'double': ctypes.c_double}.get(m.group(1), ctypes.c_void_p))
                  for n in m.group(2).split(',')]
    assert names == list(L.GNProblemStruct._fields_)
    assert [n for n, _ in names][-7:] == ['gq_a1', 'gq_a2', 'gq_b', 'gq_c1', 'gq_c3', 'nonlin', 'p2'] and len(names) == 35   # unchanged
    assert L.PROTOTYPES['gpk_assemble_hess'][1] == L.PROTOTYPES['gpk_assemble3d'][1]                # the same argument list
    assert L.PROTOTYPES['gpk_extend_functionals_hess'][1] == L.PROTOTYPES['gpk_extend_functionals3d'][1]


# ------------------------------------------------------------------------------------------------ 6. class, facade, driver
def test_class_surface_without_a_device():
    from src.PDEs import MongeAmpere2d, _GPEquation
    e = MongeAmpere2d(bdy=MA.truth, rhs=MA.rhs)
    assert isinstance(e, _GPEquation)
    assert (e._layout, e._system, e._blocks_per_point, e._structured_optin) == ('Hessian', 'MongeAmpere2d', 3, False)
    assert e._deriv_names == ('value', 'd1', 'd2', 'd11', 'd12', 'd22') and e._gn_params() == (0.0, 0.0, 0.0) and e._nl_args() == {}
    assert np.array_equal(e._initial('zero', 6), np.zeros(6)) and e._initial('rdm', 6).shape == (6,)
    assert 'Hessian layout' in e._posterior_unserved()
    for call in (e.posterior_variance, e.posterior_covariance, e.posterior_sample):
        with pytest.raises(NotImplementedError):
            call(np.zeros((2, 2)))
    Xd, Xb = MA.points(12, 8)
    e.get_sampled_points(Xd, Xb)
    assert np.array_equal(e.rhs_f, MA.rhs(Xd[:, 0], Xd[:, 1])) and np.array_equal(e.bdy_g, MA.truth(Xb[:, 0], Xb[:, 1]))
    with pytest.raises(ValueError, match='Matern52'):
        e.Gram_matrix(kernel='Matern52', kernel_parameter=0.5)
    import inspect
    sig = inspect.signature(MongeAmpere2d.Gram_matrix).parameters
    assert [sig[k].default for k in ('kernel', 'kernel_parameter', 'nugget', 'nugget_type')] == ['Gaussian', 0.3, 1e-8, 'adaptive']
    sig = inspect.signature(MongeAmpere2d.GN_method).parameters
    assert [sig[k].default for k in ('max_iter', 'step_size', 'initial_sol')] == [8, 1, 'zero']


def test_facade_routes_and_driver_parses(capsys):
    import main_MongeAmpere2d as drv
    from src.PDEs import MongeAmpere2d
    from src.solver import solver_GP
    cfg = drv.parse(['--show_figure', ''])
    assert (cfg.N_domain, cfg.N_boundary, cfg.GNsteps, cfg.initial_sol, cfg.kernel, cfg.kernel_parameter, cfg.nugget) == \
        (600, 120, 8, 'zero', 'Gaussian', 0.3, 1e-8)
    assert cfg.test_residual is False and cfg.select_kernel_parameter is None and cfg.line_search is False and cfg.show_figure is False
    cfg = drv.parse(['--N_domain', '600', '--N_boundary', '120', '--kernel_parameter', '0.2', '--nugget', '1e-8', '--GNsteps', '8',
                     '--show_figure', '', '--test_residual', '1', '--line_search', '1', '--select_kernel_parameter', '0.2,0.3'])
    assert cfg.kernel_parameter == 0.2 and cfg.test_residual and cfg.line_search and cfg.select_kernel_parameter == '0.2,0.3'
    u, f = drv.manufactured()
    x = np.random.RandomState(3).uniform(0, 1, (2, 9))
    assert np.allclose(f(*x), MA.rhs(*x), rtol=1e-15) and np.allclose(u(*x), MA.truth(*x), rtol=1e-15)
    s = solver_GP(cfg, 'MongeAmpere2d')
    s.set_equation(bdy=u, rhs=f)
    out = capsys.readouterr().out
    assert isinstance(s.eqn, MongeAmpere2d) and '[Equation type] Monge-Ampere' in out and 'det D^2 u = f' in out
