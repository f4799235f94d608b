"""Matern kernels on the host (no GPU): the long-double reference of tests/_matern_reference.py against mpmath.diff, the closed-form
classes of src/kernels.py against that reference, the trace ratios, and the rejections of what is out of scope."""
import numpy as np
import pytest

import _matern_reference as MR

NUS = (2.5, 3.5, 4.5)
NAMES = {2.5: 'Matern52', 3.5: 'Matern72', 4.5: 'Matern92'}
RHOS = (0.3, (0.3, 0.07))

# (alpha, beta) of every derivative the layouts and the extension functionals combine: per-axis order <= 2 on each side
ORDERS = sorted({(a, b) for fx in MR.FUNCTIONALS.values() for fy in MR.FUNCTIONALS.values() for a in fx for b in fy})

# a dozen fixed pairs (x1, x2, y1, y2): far, on both sides of the switch to the series (t = 0.5), 1e-12 apart, on an axis
PAIRS = [(0.31, 0.72, 0.55, 0.12), (0.9, 0.1, 0.2, 0.8), (0.5, 0.5, 0.52, 0.49), (0.5, 0.5, 0.51, 0.503), (0.25, 0.75, 0.2501, 0.7502),
         (0.4, 0.6, 0.4 + 1e-12, 0.6), (0.4, 0.6, 0.4 + 6e-13, 0.6 - 8e-13), (0.3, 0.3, 0.3, 0.45), (0.3, 0.3, 0.45, 0.3),
         (0.125, 0.875, 0.126, 0.871), (0.7, 0.2, 0.69, 0.21), (0.05, 0.95, 0.95, 0.05)]


def rho_scale(rho, fx, fy):
    """largest rho_1^-n1 rho_2^-n2 over the multi-indices of <fx, fy>: the size of such an entry relative to kappa"""
    r = np.atleast_1d(np.asarray(rho, dtype=np.float64))
    return max(r[0] ** -(a[0] + b[0]) * r[-1] ** -(a[1] + b[1]) for a in fx for b in fy)


@pytest.mark.parametrize('nu', NUS)
def test_reference_against_mpmath(nu):
    """every (alpha, beta) the functionals combine, on fixed pairs, anisotropic scales: relative to (a / rho)^n, the size of a
    derivative of order n, 1e-17 is asked of the reference (long double: eps 1.1e-19)"""
    import mpmath as mp
    m = MR.ORDER[nu]
    rho = (0.3, 0.07)
    worst = 0.0
    with mp.workdps(40):
        a = mp.sqrt(2 * m + 1)
        th = MR._THETA[m]

        def kappa(x1, x2, y1, y2):
            t = a * mp.sqrt(((x1 - y1) / mp.mpf(rho[0])) ** 2 + ((x2 - y2) / mp.mpf(rho[1])) ** 2)
            return mp.exp(-t) * sum(c * t ** j for j, c in enumerate(th)) / th[0]
        for ip, pr in enumerate(PAIRS):
            exact = [mp.mpf(float(v)) for v in pr]                    # the float64 values the reference receives
            for al, be in ORDERS[ip % 3::3]:                          # (every (alpha, beta) on four of the twelve pairs)
                want = mp.diff(kappa, tuple(exact), (al[0], al[1], be[0], be[1]))
                got = MR.partial(nu, al, be, *[np.float64(v) for v in pr], rho)
                scale = (float(a) / rho[0]) ** (al[0] + be[0]) * (float(a) / rho[1]) ** (al[1] + be[1])
                err = abs(mp.mpf(float(got)) + mp.mpf(float(got - MR.LD(float(got)))) - want) / scale
                worst = max(worst, float(err))
    print(f'[matern] reference vs mpmath nu={nu}: worst |diff| / (a/rho)^n = {worst:.2e}')
    assert worst < 1e-17


def test_reference_coincident_limits():
    """values worked out by hand: nu = 5/2, rho = 1: d_d1^4 kappa -> 3 phi''(0) = 25, d_d1^2 d_d2^2 kappa -> 25/3, Delta_x Delta_y kappa = 8 a^4 / 3"""
    z = np.zeros(1)
    assert abs(MR.partial(2.5, (2, 0), (2, 0), z, z, z, z, 1.0)[0] - 25) < 1e-17
    assert abs(MR.partial(2.5, (2, 0), (0, 2), z, z, z, z, 1.0)[0] - MR.LD(25) / 3) < 1e-17
    assert abs(MR.pair(2.5, MR.LAP, MR.LAP, z, z, z, z, 1.0)[0] - MR.LD(200) / 3) < 1e-16


def _random_pairs():
    rng = np.random.RandomState(7)
    x = rng.uniform(0, 1, (4, 60))
    x[2:, 0] = x[:2, 0]                                               # one coincident pair
    x[2, 1], x[3, 1] = x[0, 1] + 6e-13, x[1, 1] - 8e-13               # one pair 1e-12 apart
    x[2:, 2:8] = x[:2, 2:8] + rng.uniform(-0.02, 0.02, (2, 6))        # a few close ones, around the series switch
    return x


@pytest.mark.parametrize('nu', NUS)
@pytest.mark.parametrize('rho', RHOS)
def test_kernel_classes_against_reference(nu, rho):
    from src.kernels import _METHODS, Matern52_kernel, Matern72_kernel, Matern92_kernel, Matern_kernel
    x = _random_pairs()
    thin = {2.5: Matern52_kernel, 3.5: Matern72_kernel, 4.5: Matern92_kernel}[nu]()
    k = Matern_kernel(nu)
    assert thin.m == k.m
    for name, (fx, fy) in _METHODS.items():
        fxt, fyt = tuple(map(tuple, fx)), tuple(map(tuple, fy))
        want = MR.pair(nu, fxt, fyt, *x, rho)
        got = getattr(k, name)(*x, rho)
        assert np.array_equal(got, getattr(thin, name)(*x, rho))
        s = rho_scale(rho, fxt, fyt)
        err = np.abs(got - want)
        assert np.all(np.isfinite(got)), name
        assert np.all(err <= 1e-13 * np.abs(want) + 1e-12 * s), (name, float(np.max(err / (1e-13 * np.abs(want) + 1e-12 * s))))
    assert np.ndim(k.kappa(0.1, 0.2, 0.3, 0.4, 0.3)) == 0            # scalar in, scalar out
    assert k.kappa(0.1, 0.2, 0.1, 0.2, rho) == 1.0


@pytest.mark.parametrize('nu', NUS)
def test_singular_terms_vanish_exactly_at_coincident_points(nu):
    """at d = 0 the class gives the limit, with no NaN on the way: Delta_x Delta_y kappa(x, x) = 8 a^4 / 3 * phi''(0) scaling for rho = 1"""
    from src.kernels import Matern_kernel
    m = MR.ORDER[nu]
    a2 = 2.0 * m + 1.0
    phi2 = a2 ** 2 * {2: 1.0 / 3.0, 3: 1.0 / 15.0, 4: 3.0 / 105.0}[m]                    # phi''(0) = a^4 theta_{m-2}(0) / theta_m(0)
    with np.errstate(all='raise'):
        v = Matern_kernel(nu).Delta_x_Delta_y_kappa(0.3, 0.4, 0.3, 0.4, 1.0)
    assert abs(v - 8.0 * phi2) <= 4e-16 * 8.0 * phi2


@pytest.mark.parametrize('layout', sorted(MR.LAYOUTS))
@pytest.mark.parametrize('nu', NUS)
def test_trace_ratios_against_reference(layout, nu):
    """the analytic diagonal values <d^alpha, d^alpha>(0) = (-1)^|alpha| rho^-2alpha c(2 alpha_1, alpha_1) c(2 alpha_2, alpha_2) phi^(|alpha|)(0)
    through the classes, against the Taylor series of the reference"""
    from src.kernels import Matern_kernel
    k = Matern_kernel(nu)
    for rho in RHOS:
        want = MR.diagonal_values(nu, rho, layout)
        got = [k._eval(f, f, 0.5, 0.5, 0.5, 0.5, rho) for f, _ in MR.LAYOUTS[layout]]
        np.testing.assert_allclose(got, np.asarray(want, dtype=np.float64), rtol=1e-14)
        r = MR.trace_ratios(nu, rho, layout, 64, 36)
        n = [s for _, s in MR.offsets(layout, 64, 36)]
        np.testing.assert_allclose([n[b] * got[b] / (n[-1] * got[-1]) for b in range(len(r))], np.asarray(r, dtype=np.float64), rtol=1e-14)


@pytest.mark.parametrize('nu', [1.5, 0.5, 3.0, 'x', None])
def test_unknown_nu_is_rejected(nu):
    from src.kernels import Matern_kernel
    with pytest.raises(ValueError, match='nu'):
        Matern_kernel(nu)


def test_kernel_parameters():
    from gpk.device import KERNEL, kernel_params
    assert (KERNEL['Matern52'], KERNEL['Matern72'], KERNEL['Matern92']) == (8, 9, 10)
    assert list(kernel_params('Matern52', 0.3)) == [0.3, 0.3]
    assert list(kernel_params('Matern72', [0.3])) == [0.3, 0.3]
    assert list(kernel_params('Matern92', (0.3, 0.05))) == [0.3, 0.05]
    with pytest.raises(ValueError, match='Matern52'):
        kernel_params('Matern52', (0.1, 0.2, 0.3))
    from src.Gram_matrice import _KERNELS
    assert {'Matern52', 'Matern72', 'Matern92'} <= set(_KERNELS)


@pytest.mark.parametrize('kernel', ['Matern52', 'Matern72', 'Matern92'])
def test_out_of_scope_paths_name_the_kernel(kernel, monkeypatch):
    """3-D, boundary-functional and operator paths: ValueError naming the kernel, before any device call (no context can even be created here)"""
    from gpk.device import kernel_params3d
    from src import PDEs
    import src._runtime as RT

    def no_device(*a, **k):
        raise AssertionError('a device call was reached')
    monkeypatch.setattr(RT, 'get_context', no_device)
    monkeypatch.setattr(PDEs, 'get_context', no_device)
    with pytest.raises(ValueError, match=kernel):
        kernel_params3d(kernel, 0.3)
    np.random.seed(0)
    eq = PDEs.Nonlinear_elliptic2d(bdy=lambda x1, x2: 0 * x1, rhs=lambda x1, x2: 0 * x1 + 1.0)
    eq.sampled_pts(20, 8, sampled_type='random')
    eq.set_boundary_operator(np.tile([0.0, 1.0, 0.0], (eq.N_boundary, 1)))
    with pytest.raises(ValueError, match=kernel):
        eq.Gram_matrix(kernel=kernel, kernel_parameter=0.3)
    eq = PDEs.Nonlinear_elliptic2d(bdy=lambda x1, x2: 0 * x1, rhs=lambda x1, x2: 0 * x1 + 1.0)
    eq.sampled_pts(20, 8, sampled_type='random')
    eq.set_domain_operator(np.tile([0.0, 0.0, 0.0, 1.0, 0.0, 1.0], (eq.N_domain, 1)))
    with pytest.raises(ValueError, match=kernel):
        eq.Gram_matrix(kernel=kernel, kernel_parameter=0.3)
    eq3 = PDEs.Nonlinear_elliptic3d(bdy=lambda x1, x2, x3: 0 * x1, rhs=lambda x1, x2, x3: 0 * x1 + 1.0)
    eq3.sampled_pts(20, 12, sampled_type='random')
    with pytest.raises(ValueError, match=kernel):
        eq3.Gram_matrix(kernel=kernel, kernel_parameter=0.3)
