"""The reference of the evolution layout (tests/_evo_reference.py) and the surface of the class Evolution1d, without a device.

  a. Theta of the reference is symmetric, positive definite at a small size for random c, and reproduces the closed form of <Q,Q> at d = 0
  b. with c = (0, 1, 0, 0) it is the reference of the dispersive layout (tests/_kdv_reference.py); with c = (1, 0, 0, 0) the Burgers
     layout of the oracle; a boundary row (c0, c1, c2) is that combination of the rows delta, d_t, d_x
  c. the ABI: symbols, prototypes, the functional bit
  d. the class Evolution1d: construction, the equation= shorthands, the doubling of the wall points under 'clamped', _sol_vec, refusals;
     solver_GP knows the equation; the driver's manufactured solution solves the equation
"""
import numpy as np
import pytest

import _evo_reference as E
import _kdv_reference as K

LD = E.LD
PARAMS = {'Gaussian': 0.4, 'anisotropic_Gaussian': (0.6, 0.3)}


def _points(Nd=12, Nb=5, seed=3):
    rng = np.random.RandomState(seed)
    return rng.uniform(0, 1, (Nd, 2)), rng.uniform(0, 1, (Nb, 2)), rng


# ------------------------------------------------------------------------------------------------ a. Theta
@pytest.mark.parametrize('kernel', E.KERNELS)
@pytest.mark.parametrize('mixed', (False, True))
def test_theta_symmetric_positive_definite(kernel, mixed):
    kp = PARAMS[kernel]
    Xd, Xb, rng = _points()
    Nd, Nb = 12, 5
    for trial in range(3):
        c = tuple(rng.normal(size=4))
        bc = rng.normal(size=(Nb, 3)) if mixed else None
        T = E.theta(kernel, kp, c, Xd, Xb, bc)
        N = 4 * Nd + Nb
        assert T.shape == (N, N) and T.dtype == LD
        assert np.max(np.abs(T - T.T)) <= 8 * float(np.finfo(LD).eps) * np.max(np.abs(T))
        Tn = E.theta_nugget(kernel, kp, c, Xd, Xb, 1e-10, 'adaptive', bc, base=(T + T.T) / 2)
        s = 1 / np.sqrt(np.diag(Tn))
        C = (Tn * s[:, None] * s[None, :]).astype(np.float64)
        np.linalg.cholesky(C)
        assert np.linalg.eigvalsh(C)[0] > 0


@pytest.mark.parametrize('kernel', E.KERNELS)
@pytest.mark.parametrize('c', (E.KS, E.KAWAHARA, E.FULL, (0.0, 0.0, 0.0, 2.0)))
def test_values_at_coincident_points(kernel, c):
    kp = PARAMS[kernel]
    p1, p2 = K.precisions(kernel, kp)
    d = E.diagonal_values(kernel, kp, c)
    want = [p1, p2, E.qq_at_zero(p2, c), LD(1)]
    for got, w in zip(d, want):
        assert abs(got - w) <= 64 * float(np.finfo(LD).eps) * abs(w), (got, w)
    assert d[2] > 0
    Nd, Nb = 9, 4
    bc = np.array([[1, 0, 0], [0, 0, 1], [0.5, -2.0, 0.25], [0, 1, 0]], dtype=np.float64)
    trb = 1 + p2 + (LD(0.25) + 4 * p1 + p2 / 16) + p1
    r = E.trace_ratios(kernel, kp, c, Nd, Nb, bc)
    for k in range(3):
        assert abs(r[k] - Nd * want[k] / (Nd + trb)) <= 64 * float(np.finfo(LD).eps) * r[k]
    r0 = E.trace_ratios(kernel, kp, c, Nd, Nb)
    assert abs(r0[0] - Nd * p1 / (Nd + Nb)) <= 1e-17 * r0[0]


# ------------------------------------------------------------------------------------------------ b. reductions
@pytest.mark.parametrize('kernel', E.KERNELS)
def test_reduces_to_the_dispersive_reference(kernel):
    kp = PARAMS[kernel]
    Xd, Xb, rng = _points()
    assert np.array_equal(E.theta(kernel, kp, (0.0, 1.0, 0.0, 0.0), Xd, Xb), K.theta(kernel, kp, Xd, Xb))
    Xt = rng.uniform(0, 1, (4, 2))
    for n, m in (('value', 'value'), ('d1', 'd1'), ('d2', 'd2'), ('d2d2', 'd2d2'), ('q', 'd2d2d2')):
        assert np.array_equal(E.rows(kernel, kp, (0.0, 1.0, 0.0, 0.0), n, Xt, Xd, Xb), K.rows(kernel, kp, m, Xt, Xd, Xb))
    # delta in front: Theta is linear in c in the rows and columns of Q
    T2 = E.theta(kernel, kp, (0.0, 0.25, 0.0, 0.0), Xd, Xb)
    s = np.ones(4 * 12 + 5, dtype=LD)
    s[24:36] = LD(0.25)
    assert np.array_equal(T2, K.theta(kernel, kp, Xd, Xb) * s[:, None] * s[None, :])


@pytest.mark.parametrize('kernel', E.KERNELS)
def test_reduces_to_the_burgers_layout_of_the_oracle(kernel):
    from oracle import gp_oracle as O
    kp = PARAMS[kernel]
    Xd, Xb, _ = _points()
    T = E.theta(kernel, kp, (1.0, 0.0, 0.0, 0.0), Xd, Xb, dtype=np.float64)
    want = O.gram_matrix_assembly(Xd, Xb, 'Burgers', kernel, kp)
    assert T.shape == want.shape
    for (ro, rn) in E.offsets(12, 5):
        for (co, cn) in E.offsets(12, 5):
            w = want[ro:ro + rn, co:co + cn]
            assert np.max(np.abs(T[ro:ro + rn, co:co + cn] - w)) <= 64 * E.EPS * np.max(np.abs(w))


def test_boundary_rows_are_combinations():
    kernel, kp, c = 'anisotropic_Gaussian', PARAMS['anisotropic_Gaussian'], E.FULL
    Xd, Xb, rng = _points(6, 3)
    bc = rng.normal(size=(3, 3))
    T = E.theta(kernel, kp, c, Xd, Xb, bc)
    parts = [E.rows(kernel, kp, c, n, Xb, Xd, Xb, bc) for n in ('value', 'd1', 'd2')]
    want = sum(bc[:, j, None].astype(LD) * parts[j] for j in range(3))
    assert np.max(np.abs(T[3 * 6 + 6:] - want)) <= 8 * float(np.finfo(LD).eps) * np.max(np.abs(want))
    assert np.array_equal(E.rows(kernel, kp, c, 'q', Xd, Xd, Xb, bc), T[12:18])
    # bc = (1, 0, 0) everywhere is bc = None
    assert np.array_equal(E.theta(kernel, kp, c, Xd, Xb, np.tile([1.0, 0.0, 0.0], (3, 1))), E.theta(kernel, kp, c, Xd, Xb))
    assert E.rows(kernel, kp, c, 'd2d2', Xd[:2], Xd, Xb, bc).shape == (2, 27)


# ------------------------------------------------------------------------------------------------ c. the ABI
def test_functional_bit_and_prototypes():
    import os
    import gpk
    assert gpk.device.FUNCTIONAL_EVO == {'value': 1, 'd1': 2, 'd2': 4, 'd2d2': 8, 'q': 128}
    for table in (gpk.device.FUNCTIONAL, gpk.device.FUNCTIONAL3D, gpk.device.FUNCTIONAL_DISP):
        assert 128 not in table.values() and 'q' not in table
    names = set(gpk.declared_symbols())
    assert {'gpk_assemble_evo', 'gpk_extend_functionals_evo'} <= names
    lib = gpk.load_library()
    assert len(lib.gpk_assemble_evo.argtypes) == 14 and len(lib.gpk_extend_functionals_evo.argtypes) == 15
    assert hasattr(gpk.Context, 'assemble_evo') and hasattr(gpk.Context, 'extend_functionals_evo')
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'gpk.h')) as fh:
        header = fh.read()
    assert '#define GPK_FN_Q 128' in header and 'int gpk_assemble_evo(' in header and 'int gpk_extend_functionals_evo(' in header


# ------------------------------------------------------------------------------------------------ d. the class
def _equation(bc='dirichlet', **kw):
    from src.PDEs import Evolution1d
    kw = kw or {'equation': ('kuramoto_sivashinsky',)}
    e = Evolution1d(alpha=2.0, bdy=E.smooth_truth, rhs=lambda t, x: 0.0 * x + 0.25, bc=bc, bdy_x=E.smooth_truth_x if bc == 'clamped' else None, **kw)
    rng = np.random.RandomState(0)
    Xd = np.column_stack([rng.uniform(0, 1, 7), rng.uniform(-1, 1, 7)])
    Xb = np.array([[0.0, -1.0], [0.0, 0.3], [0.0, 1.0], [0.4, -1.0], [0.7, 1.0], [0.0, -0.5]])
    e.get_sampled_points(Xd, Xb)
    return e, Xd, Xb


def test_class_surface():
    from src.PDEs import Burgers, Evolution1d
    e, Xd, Xb = _equation()
    assert isinstance(e, Burgers) and Evolution1d._system == 'Burgers' and Evolution1d._deriv_names == ('value', 'd1', 'd2', 'q')
    assert (e.N_domain, e.N_boundary, e._n_unknowns()) == (7, 6, 21)
    assert e._gn_params() == (2.0, -1.0, 0.0) and e._residual_params() == (2.0, -1.0)
    assert e.coeffs == (1.0, 0.0, 1.0, 0.0) and e.boundary_coeffs is None
    z = np.random.RandomState(5).normal(size=21)
    vec, v0 = e._sol_vec(z)
    assert vec.shape == (4 * 7 + 6,) and np.array_equal(v0, z[:7])
    want = np.concatenate([-z[14:] + e.rhs_f - 2.0 * z[:7] * z[7:14], z[7:14], z[14:], z[:7], e.bdy_g])
    assert np.array_equal(vec, want)
    cs = E.Case(7, 6, e.rhs_f, e.bdy_g, 2.0, np.eye(34))
    np.testing.assert_allclose(vec, E.sol_vec(cs, z), rtol=0, atol=4 * E.EPS * np.max(np.abs(vec)))


@pytest.mark.parametrize('equation,want', [(('kuramoto_sivashinsky',), (1.0, 0.0, 1.0, 0.0)), (('kawahara', 1.5, -0.5), (0.0, 1.5, 0.0, -0.5)),
                                           (('kdv_burgers', 0.1, 0.02), (-0.1, 0.02, 0.0, 0.0)), (('benney_lin', 1, 2, 3, 4), (1.0, 2.0, 3.0, 4.0))])
def test_class_equation_shorthands(equation, want):
    from src.PDEs import Evolution1d
    assert Evolution1d(equation=equation).coeffs == want == tuple(E.equation_coeffs(equation))
    assert Evolution1d(coeffs=want).coeffs == want


def test_class_construction_refusals():
    from src.PDEs import Evolution1d
    for kw in ({}, {'coeffs': (1, 0, 1, 0), 'equation': ('kuramoto_sivashinsky',)}, {'coeffs': (0, 0, 0, 0)}, {'coeffs': (1, 2, 3)},
               {'coeffs': (1, np.nan, 0, 0)}, {'coeffs': (1, np.inf, 0, 0)}, {'equation': ('kawahara', 1.0)}, {'equation': ('heat',)},
               {'equation': ('kuramoto_sivashinsky',), 'bc': 'neumann'}, {'equation': ('kuramoto_sivashinsky',), 'bc': 'clamped'}):
        with pytest.raises(ValueError, match='Evolution1d'):
            Evolution1d(**kw)


def test_class_clamped_doubles_the_wall_points():
    e, Xd, Xb = _equation('clamped')
    wall = np.array([0, 2, 3, 4])
    assert e.N_boundary == 6 + 4 and np.array_equal(e.wall_points, wall)
    assert np.array_equal(e.X_boundary[:6], Xb) and np.array_equal(e.X_boundary[6:], Xb[wall])
    rows = np.zeros((10, 3))
    rows[:6, 0] = 1
    rows[6:, 2] = 1
    assert np.array_equal(e.boundary_coeffs, rows)
    assert np.array_equal(e.bdy_g[:6], E.smooth_truth(Xb[:, 0], Xb[:, 1]))
    assert np.array_equal(e.bdy_g[6:], E.smooth_truth_x(Xb[wall, 0], Xb[wall, 1]))
    pts, rows_ref, wall_ref = E.clamped_boundary(Xb, e.domain)
    assert np.array_equal(pts, e.X_boundary) and np.array_equal(rows_ref, rows) and np.array_equal(wall_ref, wall)
    vec, _ = e._sol_vec(np.zeros(21))
    assert vec.shape == (4 * 7 + 10,)
    # a custom operator: shape checked, dropped with the points
    with pytest.raises(ValueError, match=r'\(10, 3\)'):
        e.set_boundary_operator(np.ones((6, 3)))
    custom = np.tile([0.5, 0.0, 1.0], (10, 1))
    e.set_boundary_operator(custom)
    assert np.array_equal(e.boundary_coeffs, custom)
    d, _, _ = _equation()
    d.set_boundary_operator(np.tile([1.0, 0.0, 2.0], (6, 1)))
    d.get_sampled_points(Xd, Xb)
    assert d.boundary_coeffs is None and d.N_boundary == 6


def test_class_refusals():
    e, _, _ = _equation()
    Xt = np.array([[0.5, 0.0]])
    for call in (e.posterior_variance, e.posterior_covariance, e.posterior_sample):
        with pytest.raises(NotImplementedError, match='no rectangular evaluator for the evolution layout'):
            call(Xt)
    for kernel, kp in (('Matern52', 0.3), ('periodic_Gaussian', (0.3, 0.3, 0.0, 2.0))):
        with pytest.raises(ValueError, match='Gaussian or anisotropic_Gaussian'):
            e.Gram_matrix(kernel=kernel, kernel_parameter=kp)
    with pytest.raises(RuntimeError):
        e.log_evidence()
    with pytest.raises(UnboundLocalError):
        e._initial('zero', 21)


def test_solver_knows_the_equation():
    from types import SimpleNamespace
    from src.PDEs import Evolution1d
    from src.solver import solver_GP
    cfg = SimpleNamespace(alpha=1.0, equation=('kuramoto_sivashinsky',), bc='clamped', bdy_x=E.smooth_truth_x, kernel='anisotropic_Gaussian',
                          kernel_parameter=[0.6, 0.5])
    s = solver_GP(cfg, 'Evolution1d')
    s.set_equation(bdy=E.smooth_truth, rhs=E.smooth_rhs(1.0, E.KS), domain=E.DOMAIN, print_option=False)
    assert isinstance(s.eqn, Evolution1d) and s.eqn.coeffs == E.KS and s.eqn.bc == 'clamped'
    s.auto_sample(50, 20, print_option=False)
    n_wall = s.eqn.wall_points.size
    n0 = s.eqn.N_boundary - n_wall                                      # the points the sampler gave
    assert s.eqn.N_domain == 50 and n_wall > 0 and n0 > n_wall
    assert n_wall == int(np.sum(np.abs(s.eqn.X_boundary[:n0, 1]) == 1.0)) and np.all(np.abs(s.eqn.X_boundary[n0:, 1]) == 1.0)
    assert np.all(s.eqn.boundary_coeffs[:n0] == [1.0, 0.0, 0.0]) and np.all(s.eqn.boundary_coeffs[n0:] == [0.0, 0.0, 1.0])


@pytest.mark.parametrize('c', (E.KS, E.KAWAHARA, E.FULL))
def test_manufactured_solution_and_its_forcing(c):
    """the forcing of the reference and of the driver against central differences of u* (h = 0.05: the stencils of order four and five
    lose h^-4, h^-5 of the rounding, the truncation error is O(h^2))"""
    import main_Evolution1d as M
    rng = np.random.RandomState(2)
    t, x = rng.uniform(0, 1, 50), rng.uniform(-1, 1, 50)
    h = 0.05
    u = E.smooth_truth
    s = {k: u(t, x + k * h) for k in range(-3, 4)}
    ux = (s[1] - s[-1]) / (2 * h)
    uxx = (s[1] - 2 * s[0] + s[-1]) / h ** 2
    uxxx = (s[2] - 2 * s[1] + 2 * s[-1] - s[-2]) / (2 * h ** 3)
    u4 = (s[2] - 4 * s[1] + 6 * s[0] - 4 * s[-1] + s[-2]) / h ** 4
    u5 = (s[3] - 4 * s[2] + 5 * s[1] - 5 * s[-1] + 4 * s[-2] - s[-3]) / (2 * h ** 5)
    ut = (u(t + 1e-4, x) - u(t - 1e-4, x)) / 2e-4
    fd = ut + 1.5 * s[0] * ux + c[0] * uxx + c[1] * uxxx + c[2] * u4 + c[3] * u5
    scale = np.pi ** 5
    assert np.max(np.abs(fd - E.smooth_rhs(1.5, c)(t, x))) <= 0.02 * scale
    um, uxm, fm = M.manufactured(1.5, c)
    assert np.array_equal(um(t, x), u(t, x)) and np.array_equal(uxm(t, x), E.smooth_truth_x(t, x))
    np.testing.assert_allclose(fm(t, x), E.smooth_rhs(1.5, c)(t, x), rtol=0, atol=64 * E.EPS * scale)
