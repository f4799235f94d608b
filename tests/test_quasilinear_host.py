"""Host checks (no GPU) of the 2-jet Gram layout, the quasilinear Gauss-Newton system GPK_GN_QUASILINEAR and the class Quasilinear2d:
the reference module tests/_quasilinear_reference.py against sympy and against itself, the header against the bindings, the pure host
entry points gpk_gn_dims / gpk_gn_worksize, the class surface and the facade."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _monge_ampere_reference as MA
import _quasilinear_reference as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'nonlinpdes-gpsolver_amd')
LD, EPS = Q.LD, Q.EPS
KINDS = tuple(Q.KINDS)


# ------------------------------------------------------------------------------------------------ 1. the Gram layout of the reference
def test_theta_entries_against_sympy_derivatives_of_the_kernel():
    sp = pytest.importorskip('sympy')
    x1, x2, y1, y2 = sp.symbols('x1 x2 y1 y2')
    sx, sy = (x1, x2), (y1, y2)
    for kernel, kp in (('Gaussian', 0.4), ('anisotropic_Gaussian', (0.5, 0.3))):
        p1, p2 = (sp.Rational(float(v).as_integer_ratio()[0], float(v).as_integer_ratio()[1]) for v in Q.GR.precisions(kernel, kp))
        kap = sp.exp(-(p1 * (x1 - y1) ** 2 + p2 * (x2 - y2) ** 2) / 2)

        def apply(expr, func, s):
            out = 0
            for c, (a, b) in func:
                t = expr
                for v, n in ((s[0], a), (s[1], b)):
                    if n:
                        t = sp.diff(t, v, n)
                out += c * t
            return out
        pts = [((0.3, 0.7), (0.55, 0.2)), ((0.1, 0.1), (0.1, 0.4)), ((0.25, 0.5), (0.25, 0.5))]
        for X, Y in pts:
            P = MA.Pairs(kernel, kp, np.array([X[0]]), np.array([X[1]]), np.array([Y[0]]), np.array([Y[1]]))
            sub = {x1: sp.Rational(*X[0].as_integer_ratio()), x2: sp.Rational(*X[1].as_integer_ratio()),
                   y1: sp.Rational(*Y[0].as_integer_ratio()), y2: sp.Rational(*Y[1].as_integer_ratio())}
            for f in Q.NAMES:
                for g in Q.NAMES:
                    want = float(sp.N(apply(apply(kap, Q.FUNC[f], sx), Q.FUNC[g], sy).subs(sub), 30))
                    got, mag = P.functional_pair(Q.FUNC[f], Q.FUNC[g])
                    assert abs(float(got[0]) - want) <= 1e-15 * float(mag[0]) + 1e-300, (kernel, f, g, X, Y)


def test_theta_is_symmetric_and_contains_the_hessian_layout():
    rng = np.random.RandomState(3)
    Nd, Nb = 9, 4
    Xd, Xb = rng.uniform(0, 1, (Nd, 2)), rng.uniform(0, 1, (Nb, 2))
    for kernel, kp in (('Gaussian', 0.3), ('anisotropic_Gaussian', (0.4, 0.2))):
        T, mag, arg = Q.theta(kernel, kp, Xd, Xb)
        tol = 8 * float(np.finfo(LD).eps)                                            # (term-by-term sums in another order: long-double rounding)
        assert T.shape == (6 * Nd + Nb,) * 2 and np.all(mag * (1 + tol) >= np.abs(T)) and np.array_equal(mag, mag.T)
        safe = np.where(mag > 0, mag, 1)                                             # (mag = 0: an odd factor at d = 0, the entry is exactly 0)
        assert np.all(T[mag == 0] == 0) and float(np.max(np.abs(T - T.T) / safe)) <= tol
        Th, magh, _ = MA.theta(kernel, kp, Xd, Xb)
        assert np.array_equal(T[2 * Nd:, 2 * Nd:], Th) and np.array_equal(mag[2 * Nd:, 2 * Nd:], magh)
        # ... and the term-by-term evaluation of those blocks agrees with the closed forms
        X = np.concatenate([Xd, Xb])
        P = MA.Pairs(kernel, kp, X[:, None, 0], X[:, None, 1], X[None, :, 0], X[None, :, 1])
        for i, f in enumerate(MA.NAMES):
            for j, g in enumerate(MA.NAMES):
                (ro, rn), (co, cn) = MA.offsets(Nd, Nb)[i], MA.offsets(Nd, Nb)[j]
                v, m = P.functional_pair(Q.FUNC[f], Q.FUNC[g])
                blk, mb = Th[ro:ro + rn, co:co + cn], magh[ro:ro + rn, co:co + cn]
                assert float(np.max(np.abs(v[:rn, :cn] - blk) / np.where(mb > 0, mb, 1))) <= tol
        d = np.diag(T)
        for (o, n), c in zip(Q.offsets(Nd, Nb), Q.diagonal_values(kernel, kp)):
            assert np.max(np.abs(d[o:o + n] - c)) <= 4 * EPS * float(c)
        # the gradient blocks against central differences of the value block's kernel in the row point
        h = 1e-5
        for k in range(2):
            e = np.zeros(2); e[k] = h
            X = np.concatenate([Xd, Xb])
            Pp = MA.Pairs(kernel, kp, (Xd + e)[:, None, 0], (Xd + e)[:, None, 1], X[None, :, 0], X[None, :, 1])
            Pm = MA.Pairs(kernel, kp, (Xd - e)[:, None, 0], (Xd - e)[:, None, 1], X[None, :, 0], X[None, :, 1])
            fd = (Pp.kappa - Pm.kappa) / (2 * h)
            assert np.max(np.abs(T[k * Nd:(k + 1) * Nd, 5 * Nd:] - fd)) <= 1e-7 * float(np.max(np.abs(fd)) + 1)


# ------------------------------------------------------------------------------------------------ 2. the three equations
def _jets(n, seed=0):
    rng = np.random.RandomState(seed)
    f = rng.uniform(0.5, 1.5, n).astype(LD)
    v = tuple(rng.uniform(-1.2, 1.2, n).astype(LD) for _ in range(5))
    return f, v


@pytest.mark.parametrize('kind', KINDS)
def test_partials_equal_central_differences_in_long_double(kind):
    prm = tuple(LD(t) for t in Q.PRM[kind])
    f, v = _jets(40)
    d = Q.dG(kind, prm, f, *v)
    # h = 2^-21: truncation h^2 G''' / 6 ~ 4e-14 |G'''| and rounding eps_LD |G| / h ~ 2e-13 |G|; with |G'''|, |G| of a few tens: 1e-11
    h = LD(2) ** -21
    for k in range(5):
        vp, vm = list(v), list(v)
        vp[k] = v[k] + h; vm[k] = v[k] - h
        fd = (Q.G(kind, prm, f, *vp) - Q.G(kind, prm, f, *vm)) / (2 * h)
        scale = Q.dG_mag(kind, prm, f, *v)[k] + 1
        assert float(np.max(np.abs(fd - d[k]) / scale)) <= 1e-11, (kind, k)
        assert np.all(Q.dG_mag(kind, prm, f, *v)[k] >= np.abs(d[k]) * (1 - 1e-15))
    assert np.all(Q.G_mag(kind, prm, f, *v) >= np.abs(Q.G(kind, prm, f, *v)) * (1 - 1e-15))


@pytest.mark.parametrize('kind', KINDS)
def test_G_is_the_divergence_form_solved_for_the_laplacian(kind):
    """at a random jet with Laplace(u) := G the divergence / determinant form vanishes; perturbing the Laplacian moves it"""
    prm = tuple(LD(t) for t in Q.PRM[kind])
    f, (v0, p, q, D, M) = _jets(40, seed=1)
    lap = Q.G(kind, prm, f, v0, p, q, D, M)
    u11, u22, u12 = (lap + D) / 2, (lap - D) / 2, M / 2
    r, mag = Q.divergence_form(kind, prm, f, v0, p, q, u11, u12, u22)
    assert float(np.max(np.abs(r) / mag)) <= 64 * float(np.finfo(LD).eps)
    r2, _ = Q.divergence_form(kind, prm, f, v0, p, q, u11 + LD(0.01), u12, u22 + LD(0.01))
    assert float(np.min(np.abs(r2) / mag)) >= 1e-4
    if kind == 'gauss_curvature':
        assert np.all(lap > 0)                                                       # the convex branch


def test_special_parameters():
    f, v = _jets(30, seed=2)
    g_lin = Q.G('p_laplace', (LD(2), LD(0.7), LD(0)), f, *v)                         # m = 2: Poisson's equation
    assert float(np.max(np.abs(g_lin - f) / f)) <= 8 * float(np.finfo(LD).eps)
    for d in Q.dG('p_laplace', (LD(2), LD(0.7), LD(0)), f, *v):
        assert float(np.max(np.abs(d))) <= 64 * float(np.finfo(LD).eps)
    g_ma = Q.G('gauss_curvature', (LD(0), LD(0), LD(0)), f, *v)                      # e = 0: Monge-Ampere's root
    assert np.array_equal(g_ma, np.sqrt(v[3] * v[3] + v[4] * v[4] + 4 * f))
    z = np.zeros(30, dtype=LD)                                                       # the zero start is admissible for all three kinds
    for kind in KINDS:
        prm = tuple(LD(t) for t in Q.PRM[kind])
        assert np.all(np.isfinite(Q.G(kind, prm, f, z, z, z, z, z).astype(np.float64)))
        assert all(np.all(np.isfinite(d.astype(np.float64))) for d in Q.dG(kind, prm, f, z, z, z, z, z))


@pytest.mark.parametrize('kind', KINDS)
def test_host_equation_object_agrees_with_the_reference(kind):
    from src.quasilinear import QuasilinearEquation
    eq = QuasilinearEquation.make((kind,) + tuple(Q.PRM[kind][:2 if kind == 'p_laplace' else 1]))
    assert eq.id == Q.KINDS[kind] and eq.params == Q.PRM[kind]
    f, v = _jets(25, seed=4)
    f64, v64 = f.astype(np.float64), tuple(t.astype(np.float64) for t in v)
    assert np.allclose(eq.G(f64, *v64), Q.G(kind, Q.PRM[kind], f64, *v64), rtol=1e-13)
    for got, want, m in zip(eq.dG(f64, *v64), Q.dG(kind, Q.PRM[kind], f64, *v64), Q.dG_mag(kind, Q.PRM[kind], f64, *v64)):
        assert np.max(np.abs(got - want)) <= 1e-13 * np.max(m + 1)
    # rhs_of inverts the residual
    u, u1, u2, D, M = v64
    lap = rng_lap = np.abs(f64) + 1.0
    u11, u22, u12 = (lap + D) / 2, (rng_lap - D) / 2, M / 2
    if kind == 'gauss_curvature':
        u11, u22, u12 = 2.0 + np.abs(D), 2.0 + np.abs(M), 0.5 * M / (1 + np.abs(M))  # convex
    rhs = eq.rhs_of(u, u1, u2, u11, u12, u22)
    r, mag = Q.divergence_form(kind, Q.PRM[kind], rhs, u, u1, u2, u11, u12, u22)
    assert np.max(np.abs(r) / mag) <= 16 * EPS
    for bad in (('minimal',), ('p_laplace', -1.0), ('p_laplace', 3.0, 0.0), ('gauss_curvature', float('nan')), ('mean_curvature', 1, 2)):
        with pytest.raises(ValueError):
            QuasilinearEquation.make(bad)


# ------------------------------------------------------------------------------------------------ 3. the system of the reference
@pytest.mark.parametrize('kind', KINDS)
def test_jacobian_and_staircase_positions(kind):
    Nd, Nb = 7, 3
    cs = Q.Case(kind, Nd, Nb)
    lin = Q.linearise(cs, cs.z0)
    sysm = Q.System(kind, cs.prm, cs.f, cs.g)
    A = sysm.A(cs.z0)[0]
    assert A.shape == (6 * Nd + Nb, 5 * Nd) and np.allclose(A, lin.dense(np.float64), rtol=1e-14, atol=0)
    assert np.allclose(sysm.F(cs.z0)[0], lin.F.astype(np.float64), rtol=1e-14)
    h = 1e-6
    for j in range(0, 5 * Nd, 3):                                                    # A = dF/dz by central differences
        e = np.zeros(5 * Nd); e[j] = h
        fd = (sysm.F(cs.z0 + e)[0] - sysm.F(cs.z0 - e)[0]) / (2 * h)
        assert np.max(np.abs(fd - A[:, j])) <= 1e-7 * (1 + np.max(np.abs(A[:, j])))
    # the leading-zero layout: unknown j at position pos(j) has no non-zero above row pos(j); the pattern puts its first entry exactly there
    pos = Q.stair_pos(Nd)
    assert sorted(pos) == list(range(5 * Nd))
    pattern = np.zeros(A.shape, dtype=bool)
    pattern[lin.r, lin.c] = True
    assert np.array_equal(pattern.argmax(axis=0), pos)
    first = np.where((A != 0).any(axis=0), (A != 0).argmax(axis=0), A.shape[0])      # brute-force scan of the values
    assert np.all(first >= pos)
    if kind == 'mean_curvature':                                                     # dG/dv0 != 0: the profile is attained
        assert np.array_equal(first, pos)
    else:                                                                            # dG/dv0 = 0: v0's first VALUE sits N_d rows later
        assert np.array_equal(first[:Nd], pos[:Nd] + Nd) and np.array_equal(first[Nd:], pos[Nd:])
    assert np.array_equal(Q.stair_col(Nd), 5 * Nd - 1 - pos)


# ------------------------------------------------------------------------------------------------ 4. header, bindings, host entry points
def test_binding_matches_the_header():
    import gpk
    import gpk._lib as L
    hdr = open(os.path.join(ROOT, 'include', 'gpk.h')).read()
    assert re.search(r'GPK_GN_QUASILINEAR = 9', hdr) and gpk.SYSTEM['Quasilinear2d'] == 9 and 8 not in gpk.SYSTEM.values()
    assert re.search(r'GPK_QL_MEAN_CURVATURE = 0, GPK_QL_P_LAPLACE = 1, GPK_QL_GAUSS_CURVATURE = 2', hdr)
    assert gpk.QL_KIND == {'mean_curvature': 0, 'p_laplace': 1, 'gauss_curvature': 2} == Q.KINDS
    for name in ('gpk_assemble_jet2', 'gpk_extend_functionals_jet2', 'gpk_pde_residual_ql'):
        assert f'int {name}(' in hdr and name in gpk.declared_symbols() and name in gpk.declared_symbols(dev=True)
    fields = [n for n, _ in L.GNProblemStruct._fields_]
    assert len(fields) == 35
    body = re.search(r'typedef struct \{(.*?)\} gpk_gn_problem;', hdr, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    assert len(re.findall(r'[\w\*]+\s*[,;]', body)) == 35
    assert L.PROTOTYPES['gpk_assemble_jet2'][1] == L.PROTOTYPES['gpk_assemble_hess'][1]
    assert L.PROTOTYPES['gpk_extend_functionals_jet2'][1] == L.PROTOTYPES['gpk_extend_functionals_hess'][1]
    assert L.PROTOTYPES['gpk_pde_residual_ql'][1] == L.PROTOTYPES['gpk_pde_residual_nl'][1]
    mk = open(os.path.join(PKG, 'csrc', 'Makefile')).read()
    assert 'gpk_assemble_jet2.hip' in mk
    lib, dev = gpk.load_library(), gpk.load_library(dev=True)                        # (raises where a library is not built)
    for name in ('gpk_assemble_jet2', 'gpk_extend_functionals_jet2', 'gpk_pde_residual_ql'):
        assert getattr(lib, name) is not None and getattr(dev, name) is not None


def test_gn_dims_and_worksize_serve_system_9_without_a_device():
    import gpk
    from gpk._lib import GNProblemStruct
    lib = gpk.load_library()
    for Nd, Nb in ((900, 124), (37, 0)):
        ps = GNProblemStruct()
        ps.system, ps.Nd, ps.Nb = 9, Nd, Nb
        nz, rows = C.c_int(), C.c_int()
        assert lib.gpk_gn_dims(C.byref(ps), C.byref(nz), C.byref(rows)) == 0
        assert (nz.value, rows.value) == (5 * Nd, 6 * Nd + Nb)
        ld = C.c_int(); sb, hb, db, wb = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t()
        assert lib.gpk_gn_worksize(C.byref(ps), 0, C.byref(ld), C.byref(sb), C.byref(hb), C.byref(db), C.byref(wb)) == 0
        assert ld.value % 16 == 0 and nz.value + 1 <= ld.value < nz.value + 17
        assert sb.value == rows.value * ld.value * 8 and hb.value == (nz.value + 1) * ld.value * 8 and db.value == nz.value * 8
        assert wb.value == rows.value * 8
        ps.L, ps.ldl, ps.Dinv, ps.dinv_block = 4096, rows.value, 8192, 256          # (never dereferenced: host function)
        assert lib.gpk_gn_worksize(C.byref(ps), 0, None, None, None, None, C.byref(wb)) == 0
        assert wb.value == rows.value * ld.value * 8 + rows.value * 8
        tb = C.c_size_t()
        assert lib.gpk_gn_trial_worksize(C.byref(ps), 8, 0, C.byref(ld), C.byref(tb)) == 0 and tb.value >= 2 * rows.value * 16 * 8
    ps = GNProblemStruct(); ps.system = 8; ps.Nd = 10
    assert lib.gpk_gn_dims(C.byref(ps), None, None) < 0


# ------------------------------------------------------------------------------------------------ 5. class, facade, driver
def test_class_surface_without_a_device():
    from src.PDEs import Quasilinear2d, _GPEquation, _GradientUnknowns
    import main_Quasilinear2d as drv
    for kind in KINDS:
        args = Q.PRM[kind][:2 if kind == 'p_laplace' else 1]
        e = Quasilinear2d(equation=(kind,) + tuple(args))
        u, f = drv.manufactured(e.equation)
        e.bdy, e.rhs = u, f
        assert isinstance(e, _GradientUnknowns) and isinstance(e, _GPEquation)
        assert (e._system, e._blocks_per_point, e._zero_start, e._structured_optin) == ('Quasilinear2d', 5, True, False)
        assert e._deriv_names == ('value', 'd1', 'd2', 'd11', 'd12', 'd22')
        assert e.log_evidence.__func__ is _GPEquation.log_evidence and e.GN_loss.__func__ is _GradientUnknowns.GN_loss
        Xd, Xb = Q.points(20, 12)
        e.get_sampled_points(Xd, Xb)
        assert e._n_unknowns() == 100
        assert e._gn_params() == (Q.PRM[kind][0], Q.PRM[kind][1], 0.0) and e._nl_args() == dict(nonlin=Q.KINDS[kind], p2=0.0)
        # the two hooks against the reference's F and its linearisation
        rng = np.random.RandomState(5)
        z, zo = rng.uniform(-0.5, 0.5, 100), rng.uniform(-0.5, 0.5, 100)
        sysm = Q.System(kind, Q.PRM[kind], e.rhs_f, e.bdy_g)
        with np.errstate(invalid='ignore'):
            row = e._pde_row(e._split(z))
            want = sysm.F(z)[0][80:100]
        assert np.allclose(row, want, rtol=1e-13, equal_nan=True)
        if kind != 'gauss_curvature' or np.all(np.isfinite(sysm.F(zo)[0])):
            lin = e._pde_row_linearised(e._split(z), e._split(zo))
            want = (sysm.F(zo)[0] + sysm.A(zo)[0] @ (z - zo))[80:100]
            assert np.allclose(lin, want, rtol=1e-12, atol=1e-13)
        sv, s0 = e._sol_vec(z)
        assert sv.shape == (6 * 20 + 12,) and np.array_equal(s0, z[:20]) and np.allclose(sv, sysm.F(z)[0], rtol=1e-13, equal_nan=True)
        for call in (lambda: e.posterior_variance(Xd), lambda: e.posterior_covariance(Xd), lambda: e.posterior_sample(Xd)):
            with pytest.raises(NotImplementedError, match='no rectangular cross evaluator for the 2-jet layout'):
                call()
        for kernel in ('Matern52', 'periodic_Gaussian'):
            with pytest.raises(ValueError):
                e.Gram_matrix(kernel=kernel)
    with pytest.raises(ValueError):
        Quasilinear2d(equation=('p_laplace', 3.0, -1.0))


def test_facade_routes_and_driver_parses():
    import main_Quasilinear2d as drv
    from src.PDEs import Quasilinear2d
    from src.solver import solver_GP
    cfg = drv.parse(['--equation', 'p_laplace', '--m', '4', '--delta', '0.5', '--N_domain', '100'])
    assert drv.equation_of(cfg) == ('p_laplace', 4.0, 0.5) and cfg.initial_sol == 'zero'
    assert drv.equation_of(drv.parse(['--equation', 'mean_curvature', '--kappa', '2'])) == ('mean_curvature', 2.0)
    assert drv.equation_of(drv.parse(['--equation', 'gauss_curvature', '--e', '1.5'])) == ('gauss_curvature', 1.5)

    class Cfg:
        equation = ('gauss_curvature', 2.0)
    s = solver_GP(Cfg(), 'Quasilinear2d')
    s.set_equation(bdy=lambda a, b: a, rhs=lambda a, b: b, domain=np.array([[0, 1], [0, 1]]), print_option=False)
    assert isinstance(s.eqn, Quasilinear2d) and s.eqn.equation.kind == 'gauss_curvature' and s.eqn.equation.params == (2.0, 0.0, 0.0)
    # the driver's manufactured right-hand sides: the divergence / determinant form at u* by central differences of u*
    from src.quasilinear import QuasilinearEquation
    X = np.random.RandomState(0).uniform(0.1, 0.9, (6, 2))
    h = 1e-4
    for kind in KINDS:
        eq = QuasilinearEquation.make((kind,) + tuple(Q.PRM[kind][:2 if kind == 'p_laplace' else 1]))
        us, fs = drv.manufactured(eq, 0.5)
        E = np.eye(2)
        d = lambda k: (us(*(X + h * E[k]).T) - us(*(X - h * E[k]).T)) / (2 * h)
        dd = lambda k: (us(*(X + h * E[k]).T) - 2 * us(*X.T) + us(*(X - h * E[k]).T)) / h ** 2
        d12 = (us(*(X + h * E[0] + h * E[1]).T) - us(*(X + h * E[0] - h * E[1]).T) - us(*(X - h * E[0] + h * E[1]).T)
               + us(*(X - h * E[0] - h * E[1]).T)) / (4 * h * h)
        r, mag = Q.divergence_form(kind, Q.PRM[kind], fs(*X.T), us(*X.T), d(0), d(1), dd(0), d12, dd(1))
        assert np.max(np.abs(r) / mag) <= 1e-5, kind
