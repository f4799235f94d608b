"""The semilinear system with a gradient-dependent nonlinearity on the host (no GPU): the nonlinearity and its derivatives, the
long-double reference against the oracle's Eikonal system, convergence of the reference Gauss-Newton iteration on the problems the GPU
test solves, the binding, the facade and the driver's command line."""
import ctypes
import os
import re

import numpy as np
import pytest

import _semilinear_reference as SL
from oracle import gp_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = SL.LD


def test_dN_is_the_derivative_of_N():
    """complex step: Im N(x + ih) / h is the partial derivative to rounding for a polynomial"""
    from src.nonlinearity import GradientNonlinearity
    rng = np.random.RandomState(0)
    u, p, q = rng.normal(size=(3, 50))
    h = 1e-30
    for gq in (SL.GQ, (1.0, 1.0, 0.0, 0.0, 0.0), (0.0, 0.0, 1.0, 1.0, 0.0), (1.0, -1.0, 0.5, 1.0, 1.0)):
        nl = GradientNonlinearity(*gq)
        assert nl.params == tuple(float(v) for v in gq)
        want = (SL.N(gq, u + 1j * h, p, q).imag / h, SL.N(gq, u, p + 1j * h, q).imag / h, SL.N(gq, u, p, q + 1j * h).imag / h)
        for got_ref, got_host, w in zip(SL.dN(gq, u, p, q), nl.dN(u, p, q), want):
            assert np.allclose(got_ref, w, rtol=1e-14, atol=1e-14) and np.allclose(got_host, w, rtol=1e-14, atol=1e-14)
        assert np.allclose(nl.N(u, p, q), SL.N(gq, u, p, q), rtol=1e-14, atol=1e-14)


def test_presets_and_specs():
    from src.nonlinearity import GradientNonlinearity as G
    assert G.make(('burgers', 2.0, -1.0)).params == (2.0, -1.0, 0.0, 0.0, 0.0)
    assert G.make(('hamilton_jacobi', 0.5, 1.0)).params == (0.0, 0.0, 0.5, 1.0, 0.0)
    assert G.make(('eikonal',)).params == (0.0, 0.0, 1.0, 0.0, 0.0)
    assert G.make((1, 2, 3, 4, 5)).params == (1.0, 2.0, 3.0, 4.0, 5.0)
    nl = G(a1=1.0)
    assert G.make(nl) is nl
    for bad in ('burgers', ('burgers', 1.0), ('kpz', 1.0), (1.0, 2.0), 3.0):
        with pytest.raises(ValueError):
            G.make(bad)


def test_eikonal_special_case_matches_the_oracle():
    """gq = (0, 0, 1, 0, 0) and f -> f^2: the entries of A and the copied rows of F exactly, the PDE row to 2 ulp"""
    cs0 = SL.case(65)
    cs = SL.Case(cs0.Nd, cs0.Nb, gq=(0, 0, 1, 0, 0), eps=0.1, like=cs0)
    lin = SL.linearise(cs, cs.z0, f=cs.f ** 2)
    ref = O.EikonalSystem(0.1, cs.f, cs.g)
    A = lin.dense(np.float64)
    Ao = ref.A(cs.z0)[0]
    # the Eikonal system has no entry at (2 N_d + t, v0_t): here it is N_u / eps = 0, a stored zero
    assert np.array_equal(A, Ao)
    F, Fo = lin.F.astype(np.float64), ref.F(cs.z0)[0]
    assert np.array_equal(F[lin.Fcopy], Fo[lin.Fcopy])
    m = ~lin.Fcopy                                                    # (ulp of the magnitude sum (f^2 + v1^2 + v2^2) / eps: the row cancels)
    assert np.all(np.abs(F[m].astype(LD) - Fo[m]) <= 2 * SL.EPS * lin.Fmag[m])


def test_reference_build_gate_accepts_itself_and_rejects_an_error():
    cs = SL.case(65)
    lin = SL.linearise(cs, cs.z0)
    A, F = lin.dense(np.float64), lin.F.astype(np.float64)
    assert SL.check_build(lin, A, F) <= 0.5 + 1e-9
    k = 2 * cs.Nd
    bad = A.copy(); bad[k, 0] *= 1 + 1e-11
    with pytest.raises(AssertionError):
        SL.check_build(lin, bad, F)
    bad = A.copy(); bad[k, 0] = 0.0                                   # dN/du dropped
    with pytest.raises(AssertionError):
        SL.check_build(lin, bad, F)
    badF = F.copy(); badF[k] *= 1 + 1e-11
    with pytest.raises(AssertionError):
        SL.check_build(lin, A, badF)


def test_step_gates_reject_a_dropped_dN_du():
    """what a two-segment (Eikonal) profile would do to this system -- lose the entries N_u / eps of A -- fails every gate of the step"""
    cs = SL.case(65)
    ref = SL.full_reference(65)
    assert ref.cond < 1e8
    A = ref.lin.dense(np.float64)
    i = np.arange(cs.Nd)
    A[2 * cs.Nd + i, i] = 0.0
    from scipy.linalg import solve_triangular
    Sb = solve_triangular(cs.L, np.concatenate([A, ref.lin.F.astype(np.float64)[:, None]], axis=1), lower=True)
    H, g = 2 * Sb[:, :-1].T @ Sb[:, :-1], 2 * Sb[:, :-1].T @ Sb[:, -1]
    d = np.linalg.solve(H, g)
    res = SL.gates(ref, H=H, g=g, delta=d, z_out=cs.z0 - d)
    for name in ('H', 'g', 'delta', 'z'):
        assert res[name][0] > 1e6 * res[name][1], (name, res[name])
    ok = SL.gates(ref, H=ref.p64.H, g=ref.p64.g, loss=ref.p64.loss, delta=ref.p64.delta, z_out=cs.z0 - ref.p64.delta)
    for name, (r, a) in ok.items():
        assert r <= a, (name, r, a)


def test_vector_gates_reject_a_dropped_dN_du_at_the_pipelined_size():
    """N_d = 342, N_b = 40 (n_z + 1 = 1027, the smallest pipelined size; tests/test_gpu_fused_phase.py section e): the vector-only
    reference agrees with itself (the refined delta leaves a residual at the long-double rounding level, the float64 pipeline passes
    the gates); a float64 step whose v0 columns are cut off above row 3 N_d + t -- rows [2 N_d + t, 3 N_d + t), what Eikonal's
    two-segment profile would skip -- fails the backward and the forward gate, and so does a delta moved by 1e-11."""
    import _gn_reference as R
    from scipy.linalg import cho_factor, cho_solve, solve_triangular
    Nd, Nb = 342, 40
    vec = SL.vector_reference(Nd, Nb)
    cs = vec.case
    assert cs.nz + 1 == 1027
    d = vec.delta
    scale = vec.normH * float(np.linalg.norm(d.astype(np.float64))) + float(np.linalg.norm(vec.g.astype(np.float64)))
    assert np.linalg.norm(vec.residual(d).astype(np.float64)) <= 1e-3 * R.EPS * scale
    p = vec.p64
    for gate, v in ((R.gate_loss, p.loss), (R.gate_backward_vec, p.delta), (R.gate_forward, p.delta)):
        r, a = gate(vec, v)
        assert r <= a, (gate.__name__, r, a)
    A = vec.lin.dense(np.float64)
    t = np.arange(Nd)
    for tt in (0, Nd - 1):                                            # the only entry of a v0 column in those rows is N_u / eps
        assert np.count_nonzero(A[2 * Nd + tt:3 * Nd + tt, tt]) == 1 and A[2 * Nd + tt, tt] != 0
    A[2 * Nd + t, t] = 0.0
    Sb = solve_triangular(cs.L, np.concatenate([A, vec.lin.F.astype(np.float64)[:, None]], axis=1), lower=True, check_finite=False)
    H, g = 2 * Sb[:, :-1].T @ Sb[:, :-1], 2 * Sb[:, :-1].T @ Sb[:, -1]
    wrong = cho_solve(cho_factor(H, lower=True), g)
    u = np.random.RandomState(Nd).normal(size=cs.nz); u /= np.linalg.norm(u)
    moved = p.delta + 1e-11 * np.linalg.norm(p.delta) * u
    print()
    for what, dd, factor in (('dropped dN/du', wrong, 1e6), ('delta moved by 1e-11', moved, 1.0)):
        for gate in (R.gate_backward_vec, R.gate_forward):
            r, a = gate(vec, dd)
            print(f'[semilinear host] {what}: {gate.__name__} {r:.3g}, allowed {a:.3g}: fails by a factor {r / a:.3g}')
            assert r > factor * a, (what, gate.__name__, r, a)
    r, a = R.gate_loss(vec, p.loss * (1 + 1e-11))
    assert r > a


# (gq, eps): the three problems of the issue's table at N_d 300, N_b 80, Gaussian sigma 0.2, nugget 1e-6.  L2 errors at the collocation
# points reached by the float64 reference iteration after 10 steps, from zero and from a standard normal start alike (this test prints
# them): 1.69e-5, 1.11e-5, 1.09e-5 on the points of SL.points (the issue's table, on other points: 1.4e-5, 1.3e-5, 1.3e-5).  The bound
# 1e-4 asks for that order of magnitude: a system that does not converge stays at 0.1 .. 0.4
ROWS = [((1.0, 1.0, 0.0, 0.0, 0.0), 0.1, 1e-4), ((0.0, 0.0, 1.0, 1.0, 0.0), 0.5, 1e-4), ((1.0, -1.0, 0.5, 1.0, 1.0), 0.2, 1e-4)]


@pytest.mark.parametrize('gq,eps,bound', ROWS)
def test_reference_iteration_converges(gq, eps, bound):
    Xd, Xb = SL.points(300, 80)
    T, _ = O.add_nugget(O.gram_matrix_assembly(Xd, Xb, 'Eikonal', 'Gaussian', 0.2), 'Eikonal', 300, 80, 1e-6)
    L = O.cholesky(T)
    sysm = SL.System(eps, gq, SL.manufactured_rhs(eps, gq, Xd[:, 0], Xd[:, 1]), SL.truth(Xb[:, 0], Xb[:, 1]))
    us = SL.truth(Xd[:, 0], Xd[:, 1])
    for start in (np.zeros(900), np.random.RandomState(1).normal(size=900)):
        z, hist = SL.gn_float64(sysm, L, start, 10)
        l2 = float(np.sqrt(np.mean((z[:300] - us) ** 2)))
        print(f'\n[semilinear host] gq {gq} eps {eps}: L2 error {l2:.3g}, loss {hist[-1]:.6g}, loss after 6 steps {hist[6]:.6g}')
        assert l2 < bound
        assert abs(hist[-1] - hist[6]) <= 1e-6 * abs(hist[-1])       # flat after 6 steps


def test_binding_matches_the_header():
    import gpk
    import gpk._lib as L
    hdr = open(os.path.join(ROOT, 'include', 'gpk.h')).read()
    assert re.search(r'GPK_GN_SEMILINEAR = 5', hdr) and gpk.SYSTEM['Semilinear2d'] == 5
    assert 'int gpk_pde_residual_sl(' in hdr and 'gpk_pde_residual_sl' in gpk.declared_symbols()
    body = re.search(r'typedef struct \{(.*?)\} gpk_gn_problem;', hdr, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = []
    for decl in filter(None, (d.strip() for d in body.split(';'))):
        m = re.match(r'(const\s+double\s*\*|int|double)\s*(.*)', decl)
        names += [(n.strip().lstrip('*').strip(), {'int': ctypes.c_int, 'double': ctypes.c_double}.get(m.group(1), ctypes.c_void_p))
                  for n in m.group(2).split(',')]
    assert names == list(L.GNProblemStruct._fields_)
    f = [n for n, _ in names]
    k = f.index('gq_a1')
    assert f[k:k + 5] == ['gq_a1', 'gq_a2', 'gq_b', 'gq_c1', 'gq_c3']   # five consecutive doubles
    off = [getattr(L.GNProblemStruct, n).offset for n in f[k:k + 5]]
    assert off == [off[0] + 8 * i for i in range(5)]


def test_class_surface_without_a_device():
    from src.PDEs import Eikonal, Semilinear2d
    e = Semilinear2d(eps=0.2, nonlinearity=('hamilton_jacobi', 0.5, 1.0))
    assert e._system == 'Semilinear2d' and e._layout == Eikonal._layout and e._blocks_per_point == 3 and e._structured_optin is False
    assert e._gn_params() == (0.2, 0.0, 0.0) and e._nl_args() == {'gq': (0.0, 0.0, 0.5, 1.0, 0.0)}
    assert Semilinear2d().nonlinearity.params == (1.0, 1.0, 0.0, 0.0, 0.0) and Semilinear2d().eps == 0.1
    for bad in (0, 0.0, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            Semilinear2d(eps=bad)
    assert np.array_equal(e._initial('zero', 6), np.zeros(6)) and e._initial('rdm', 6).shape == (6,)
    assert np.array_equal(e._initial(np.arange(6.0), 6), np.arange(6.0))


def test_facade_routes_and_driver_parses(capsys):
    import main_Semilinear2d as drv
    from src.nonlinearity import GradientNonlinearity
    from src.PDEs import Semilinear2d
    from src.solver import solver_GP
    cfg = drv.parse(['--equation', 'hamilton_jacobi', '--eps', '0.5', '--show_figure', ''])
    assert (cfg.N_domain, cfg.N_boundary, cfg.GNsteps, cfg.initial_sol, cfg.kernel, cfg.kernel_parameter) == (600, 120, 8, 'zero', 'Gaussian', 0.2)
    assert cfg.test_residual is False and cfg.test_variance is False and cfg.posterior_samples == 0 and cfg.select_kernel_parameter is None
    assert drv.coefficients_from(cfg) == (0.0, 0.0, 1.0, 1.0, 0.0)
    assert drv.coefficients_from(drv.parse([])) == (1.0, 1.0, 0.0, 0.0, 0.0)
    assert drv.coefficients_from(drv.parse(['--equation', 'custom', '--nl_params=1,2,3,4,5'])) == (1.0, 2.0, 3.0, 4.0, 5.0)
    with pytest.raises(SystemExit):
        drv.coefficients_from(drv.parse(['--nl_params=1,2']))
    nl = GradientNonlinearity.make(drv.coefficients_from(cfg))
    u, f = drv.manufactured(cfg.eps, nl)
    x = np.random.RandomState(3).uniform(0, 1, (2, 9))
    assert np.allclose(f(*x), SL.manufactured_rhs(cfg.eps, nl.params, *x), rtol=1e-14) and np.array_equal(u(*x), SL.truth(*x))
    cfg.nonlinearity = nl
    s = solver_GP(cfg, 'Semilinear2d')
    s.set_equation(bdy=u, rhs=f)
    out = capsys.readouterr().out
    assert isinstance(s.eqn, Semilinear2d) and s.eqn.eps == 0.5 and s.eqn.nonlinearity is nl
    assert '[Equation parameter] eps = 0.5' in out
    cfg.nonlinearity, cfg.nl_params = None, (1.0, 1.0, 0.0, 0.0, 0.0)         # the other way a configuration names the coefficients
    s = solver_GP(cfg, 'Semilinear2d')
    s.set_equation(bdy=u, rhs=f, print_option=False)
    assert s.eqn.nonlinearity.params == (1.0, 1.0, 0.0, 0.0, 0.0)
