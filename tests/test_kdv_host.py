"""The reference of the dispersive layout (tests/_kdv_reference.py) and the surface of the class KdV, without a device.

  a. the entries of the reference against central finite differences of the kernel at a few separations, coincident points included
  b. Theta of the reference is symmetric, positive definite at a small size, and its diagonal and trace ratios are p1, p2, 15 p2^3, 1
  c. the soliton solves the equation: the residual of the closed form is at rounding level, and its closed-form derivatives are those of
     the function the driver uses
  d. the class KdV: sizes, _gn_params, _sol_vec, the start 'profile', the refusals; solver_GP knows the equation
"""
import numpy as np
import pytest

import _kdv_reference as K

LD = K.LD
PARAMS = {'Gaussian': 0.4, 'anisotropic_Gaussian': (0.6, 0.3)}


# ------------------------------------------------------------------------------------------------ a. finite differences
@pytest.mark.parametrize('kernel', K.KERNELS)
def test_entries_against_finite_differences(kernel):
    kp = PARAMS[kernel]
    p1, p2 = (float(v) for v in K.precisions(kernel, kp))
    x = np.array([0.31, -0.12])
    seps = [(0.0, 0.0), (0.17, 0.0), (0.0, -0.23), (0.11, 0.29), (-0.4, 0.35), (0.05, 1.0 / np.sqrt(p2))]
    h = 2e-3
    worst = 0.0
    for s in seps:
        y = x - np.asarray(s)
        P = K.Pairs(kernel, kp, x[0:1], x[1:2], y[0:1], y[1:2])
        for m in K.BLOCKS + ((0, 2),):
            for n in K.BLOCKS:
                got = float(P.entry(m, n)[0])
                fd = float(K.finite_difference(kernel, kp, m, n, x, y, h))
                scale = p1 ** ((m[0] + n[0]) / 2) * p2 ** ((m[1] + n[1]) / 2)      # the size of such an entry
                worst = max(worst, abs(got - fd) / scale)
                # second-order differences: the error is ~ h^2 p (order^2 / 24) of the scale, below 2e-3 here; a wrong sign or a wrong
                # coefficient of a Hermite polynomial is an error of order one
                assert abs(got - fd) <= 5e-3 * scale, (kernel, s, m, n, got, fd)
    print(f'\n[kdv host] {kernel}: worst |entry - finite difference| / scale = {worst:.3g}')


def test_parity_of_the_odd_blocks():
    """<d_x^3, delta> and <d_x^3, d_t> are odd in d_2; <delta, F> = -<F, delta> for the odd functionals"""
    kernel, kp = 'anisotropic_Gaussian', PARAMS['anisotropic_Gaussian']
    a, b = np.array([0.25]), np.array([0.5])                            # (separations that are exact in binary)
    P = K.Pairs(kernel, kp, a, b, a - 0.125, b - 0.375)
    Q = K.Pairs(kernel, kp, a, b, a - 0.125, b + 0.375)
    for n in ((0, 0), (1, 0)):
        assert float(P.entry((0, 3), n)[0]) == -float(Q.entry((0, 3), n)[0]) != 0.0
    for m in ((1, 0), (0, 1), (0, 3)):
        assert float(P.entry(m, (0, 0))[0]) == -float(P.entry((0, 0), m)[0]) != 0.0


# ------------------------------------------------------------------------------------------------ b. Theta
@pytest.mark.parametrize('kernel', K.KERNELS)
def test_theta_symmetric_positive_definite(kernel):
    kp = PARAMS[kernel]
    Nd, Nb = 12, 5
    rng = np.random.RandomState(3)
    Xd, Xb = rng.uniform(0, 1, (Nd, 2)), rng.uniform(0, 1, (Nb, 2))
    T = K.theta(kernel, kp, Xd, Xb)
    N = 4 * Nd + Nb
    assert T.shape == (N, N) and T.dtype == LD
    assert np.array_equal(T, T.T)
    p1, p2 = K.precisions(kernel, kp)
    want = [p1, p2, 15 * p2 ** 3, LD(1)]
    for (o, n), w, c in zip(K.offsets(Nd, Nb), want, K.diagonal_values(kernel, kp)):
        assert abs(c - w) <= 1e-17 * w
        assert np.max(np.abs(np.diag(T)[o:o + n] - w)) <= 1e-17 * w
    r = K.trace_ratios(kernel, kp, Nd, Nb)
    for k in range(3):
        assert abs(r[k] - LD(Nd) * want[k] / LD(Nd + Nb)) <= 1e-17 * r[k]
    # positive definite: scaled to a unit diagonal, the float64 Cholesky factorisation succeeds and the smallest eigenvalue is positive
    Tn = K.theta_nugget(kernel, kp, Xd, Xb, 1e-10, 'adaptive', base=T)
    s = 1 / np.sqrt(np.diag(Tn))
    C = (Tn * s[:, None] * s[None, :]).astype(np.float64)
    np.linalg.cholesky(C)
    assert np.linalg.eigvalsh(C)[0] > 0
    for nugget_type, expect in (('none', [0, 0, 0, 0]), ('identity', [1e-3] * 4), ('adaptive', [1e-3 * float(v) for v in r] + [1e-3])):
        got = K.block_nuggets(kernel, kp, Nd, Nb, 1e-3, nugget_type)
        np.testing.assert_allclose(np.asarray(got, dtype=np.float64), expect, rtol=1e-15)


def test_rows_are_the_rows_of_theta():
    kernel, kp = 'Gaussian', PARAMS['Gaussian']
    rng = np.random.RandomState(4)
    Xd, Xb = rng.uniform(0, 1, (6, 2)), rng.uniform(0, 1, (3, 2))
    T = K.theta(kernel, kp, Xd, Xb)
    for name, o in (('d1', 0), ('d2', 6), ('d2d2d2', 12), ('value', 18)):
        assert np.array_equal(K.rows(kernel, kp, name, Xd, Xd, Xb), T[o:o + 6])
    assert K.rows(kernel, kp, 'd2d2', Xd[:2], Xd, Xb).shape == (2, 27)


# ------------------------------------------------------------------------------------------------ c. the soliton
@pytest.mark.parametrize('alpha,delta,c,x0', [(6.0, 1.0, 1.0, 0.0), (6.0, 1.0, 4.0, -2.0), (1.0, 0.0025, 0.3, -0.4)])
def test_soliton_solves_the_equation(alpha, delta, c, x0):
    rng = np.random.RandomState(1)
    w = 6.0 / np.sqrt(c / delta)
    t, x = rng.uniform(0, 1, 200), x0 + rng.uniform(-w, w + c, 200)
    res, mag = K.soliton_residual(alpha, delta, c, x0, t, x)
    ratio = float(np.max(np.abs(res) / mag))
    print(f'\n[kdv host] soliton ({alpha}, {delta}, {c}, {x0}): worst |residual| / sum|terms| = {ratio:.3g}')
    assert ratio <= 64 * float(np.finfo(LD).eps)
    # the function the driver uses has these derivatives: central differences of it in x and t (float64 values, h = 1e-3 widths)
    u = K.soliton(alpha, delta, c, x0)
    h = 1e-3 * w
    ux = (u(t, x + h) - u(t, x - h)) / (2 * h)
    ut = (u(t + h / c, x) - u(t - h / c, x)) / (2 * h / c)
    uxxx = (u(t, x + 2 * h) - 2 * u(t, x + h) + 2 * u(t, x - h) - u(t, x - 2 * h)) / (2 * h ** 3)
    r = ut + alpha * u(t, x) * ux + delta * uxxx
    assert np.max(np.abs(r)) <= 1e-4 * float(np.max(mag))


def test_smooth_solution_and_its_forcing():
    rng = np.random.RandomState(2)
    t, x = rng.uniform(0, 1, 100), rng.uniform(-1, 1, 100)
    h = 1e-3
    u = K.smooth_truth
    ux = (u(t, x + h) - u(t, x - h)) / (2 * h)
    ut = (u(t + h, x) - u(t - h, x)) / (2 * h)
    uxxx = (u(t, x + 2 * h) - 2 * u(t, x + h) + 2 * u(t, x - h) - u(t, x - 2 * h)) / (2 * h ** 3)
    assert np.max(np.abs(ut + K.ALPHA * u(t, x) * ux + K.DELTA * uxxx - K.smooth_rhs(t, x))) <= 1e-4


# ------------------------------------------------------------------------------------------------ d. the class
def _equation(Nd=7, Nb=4):
    from src.PDEs import KdV
    e = KdV(alpha=2.0, delta=0.5, bdy=K.soliton(2.0, 0.5, 1.0, 0.0), rhs=lambda t, x: 0.0 * x + 0.25)
    rng = np.random.RandomState(0)
    e.get_sampled_points(np.column_stack([rng.uniform(0, 1, Nd), rng.uniform(-1, 1, Nd)]),
                         np.column_stack([np.zeros(Nb), np.linspace(-1, 1, Nb)]))
    return e


def test_class_surface():
    from src.PDEs import Burgers, KdV
    e = _equation()
    assert isinstance(e, Burgers) and KdV._system == 'Burgers' and KdV._deriv_names == ('value', 'd1', 'd2', 'd2d2d2')
    assert (e.N_domain, e.N_boundary, e._n_unknowns()) == (7, 4, 21)
    assert e._gn_params() == (2.0, -0.5, 0.0)
    assert e._residual_params() == (2.0, -0.5)
    d = KdV()
    assert (d.alpha, d.delta) == (6.0, 1.0) and d._gn_params() == (6.0, -1.0, 0.0)
    rng = np.random.RandomState(5)
    z = rng.normal(size=21)
    vec, v0 = e._sol_vec(z)
    assert vec.shape == (4 * 7 + 4,) and np.array_equal(v0, z[:7])
    want = np.concatenate([-0.5 * z[14:] + e.rhs_f - 2.0 * z[:7] * z[7:14], z[7:14], z[14:], z[:7], e.bdy_g])
    assert np.array_equal(vec, want)
    # the same vector as the Burgers system of the Gauss-Newton reference with nu = -delta
    cs = K.Case(7, 4, e.rhs_f, e.bdy_g, 2.0, 0.5, np.eye(32))
    np.testing.assert_allclose(vec, K.sol_vec(cs, z), rtol=0, atol=4 * K.EPS * np.max(np.abs(vec)))


def test_class_start_from_the_initial_profile():
    e = _equation()
    z = e._initial('profile', 21)
    x = e.X_domain[:, 1]
    u = K.soliton(2.0, 0.5, 1.0, 0.0)
    res, _ = K.soliton_residual(2.0, 0.5, 1.0, 0.0, np.zeros(7), x)
    k = np.sqrt(1.0 / 0.5) / 2
    S, T = 1 / np.cosh(k * x) ** 2, np.tanh(k * x)
    assert np.array_equal(z[:7], u(np.zeros(7), x))
    np.testing.assert_allclose(z[7:14], -2 * k * 1.5 * S * T, atol=1e-5)
    np.testing.assert_allclose(z[14:], 8 * k ** 3 * 1.5 * S * T * (3 * S - 1), atol=1e-4)
    assert e._initial('rdm', 21).shape == (21,)
    with pytest.raises(UnboundLocalError):
        e._initial('zero', 21)
    with pytest.raises(ValueError):
        e._initial(np.zeros(20), 21)


def test_class_refusals():
    e = _equation()
    Xt = np.array([[0.5, 0.0]])
    for call in (e.posterior_variance, e.posterior_covariance, e.posterior_sample):
        with pytest.raises(NotImplementedError, match='no rectangular evaluator for the dispersive layout'):
            call(Xt)
    for kernel, kp in (('Matern52', 0.3), ('periodic_Gaussian', (0.3, 0.3, 0.0, 2.0))):
        with pytest.raises(ValueError, match='Gaussian or anisotropic_Gaussian'):
            e.Gram_matrix(kernel=kernel, kernel_parameter=kp)
    with pytest.raises(RuntimeError):
        e.log_evidence()


def test_functional_bit_and_prototypes():
    import os
    import gpk
    assert gpk.device.FUNCTIONAL_DISP == {'value': 1, 'd1': 2, 'd2': 4, 'd2d2': 8, 'd2d2d2': 64}
    assert 'd2d2d2' not in gpk.device.FUNCTIONAL and 64 not in gpk.device.FUNCTIONAL.values()
    names = set(gpk.declared_symbols())
    assert {'gpk_assemble_disp', 'gpk_extend_functionals_disp'} <= names
    assert hasattr(gpk.Context, 'assemble_disp') and hasattr(gpk.Context, 'extend_functionals_disp')
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'gpk.h')) as fh:
        header = fh.read()
    assert '#define GPK_FN_D2D2D2 64' in header


def test_solver_knows_the_equation():
    from types import SimpleNamespace
    from src.PDEs import KdV
    from src.solver import solver_GP
    cfg = SimpleNamespace(alpha=6.0, delta=1.0, kernel='anisotropic_Gaussian', kernel_parameter=[0.5, 1.0])
    s = solver_GP(cfg, 'KdV')
    s.set_equation(bdy=K.soliton(6.0, 1.0, 1.0, 0.0), rhs=lambda t, x: 0 * x, domain=np.array([[0, 1], [-8, 8]]), print_option=False)
    assert isinstance(s.eqn, KdV) and (s.eqn.alpha, s.eqn.delta) == (6.0, 1.0)
    s.auto_sample(50, 20, print_option=False)
    assert s.eqn.N_domain == 50 and s.eqn.X_domain[:, 1].min() >= -8 and s.eqn.X_domain[:, 1].max() <= 8
