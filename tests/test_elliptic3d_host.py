"""The nonlinear elliptic equation in three space dimensions: the host-side expectation and its CPU checks.

The expectation is the closed form of DESIGN.md section K, "Three dimensions": with d = x - y, kappa = exp(-sum_k p_k d_k^2 / 2) and the
1-D Hermite factors h0..h4,
    <F at x, G at y> kappa = sum_{alpha in F} sum_{beta in G} (-1)^{|alpha|} prod_k h_{alpha_k+beta_k}(p_k, d_k) kappa,
over multi-index lists (`blk`).  It is checked here against symbolic differentiation of kappa.  The GPU tests
(test_gpu_elliptic3d.py) import `blk`, `theta`, `extend_rows`, `NumpyPipeline` and the tables from this module."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'nonlinpdes-gpsolver_amd')
if PKG not in sys.path:
    sys.path.insert(0, PKG)

EPS = np.finfo(np.float64).eps
LD = np.longdouble

# multi-index lists of the functionals (names of gpk.device.FUNCTIONAL3D)
MULTI = {'value': [(0, 0, 0)], 'd1': [(1, 0, 0)], 'd2': [(0, 1, 0)], 'd3': [(0, 0, 1)], 'laplacian': [(2, 0, 0), (0, 2, 0), (0, 0, 2)]}
FN_BITS = {'value': 1, 'd1': 2, 'd2': 4, 'laplacian': 16, 'd3': 32}
KERNELS = (('Gaussian', 0.3), ('anisotropic_Gaussian', (0.5, 0.3, 0.7)))
UNIT_CUBE = [[0, 1], [0, 1], [0, 1]]


def precisions(kernel, kp):
    """p_k of kappa = exp(-sum p_k d_k^2 / 2): Gaussian 1/sigma^2 on every axis; anisotropic 2/sigma_k^2 (the reference's convention)"""
    if kernel == 'Gaussian':
        return (1.0 / (kp * kp),) * 3
    return tuple(2.0 / (s * s) for s in kp)


def hermite(p, d):
    q = p * d
    q2 = q * q
    return (np.ones_like(d), q, q2 - p, q * (q2 - 3 * p), q2 * (q2 - 6 * p) + 3 * p * p)


def blk(fx, fy, X, Y, p, dtype=np.float64):
    """(value, sum of |terms|) of <fx at X[i], fy at Y[j]> kappa, both (len(X), len(Y)); fx, fy: multi-index lists.  dtype = longdouble
    gives the expectation three digits below fp64 rounding (the differences d are exact in either: X, Y are fp64)."""
    X = np.asarray(X, dtype=dtype).reshape(-1, 3); Y = np.asarray(Y, dtype=dtype).reshape(-1, 3)
    p = [dtype(v) for v in p]
    d = [X[:, None, k] - Y[None, :, k] for k in range(3)]
    kap = np.exp(-(p[0] * d[0] * d[0] + p[1] * d[1] * d[1] + p[2] * d[2] * d[2]) / 2)
    h = [hermite(p[k], d[k]) for k in range(3)]
    val = np.zeros_like(kap); mag = np.zeros_like(kap)
    for a in fx:
        for b in fy:
            t = (-1) ** sum(a) * h[0][a[0] + b[0]] * h[1][a[1] + b[1]] * h[2][a[2] + b[2]] * kap
            val += t
            mag += np.abs(t)
    return val, mag


def diag_lap_lap(p):
    """<Lap, Lap> at d = 0: 3 sum p_k^2 + sum_{i != j} p_i p_j (15 p^2 when isotropic)"""
    return 3 * sum(v * v for v in p) + sum(p[i] * p[j] for i in range(3) for j in range(3) if i != j)


def trace_ratio(p, Nd, Nb):
    return Nd * diag_lap_lap(p) / (Nd + Nb)


def theta(Xd, Xb, p, dtype=np.float64):
    """(Theta without nugget, sum of |terms| per entry) in the ELLIPTIC3D layout: Laplacian on Xd, delta on [Xd; Xb]"""
    Xd = np.asarray(Xd, dtype=np.float64).reshape(-1, 3); Xb = np.asarray(Xb, dtype=np.float64).reshape(-1, 3)
    Xa = np.concatenate([Xd, Xb], axis=0)
    L, D = MULTI['laplacian'], MULTI['value']
    parts = [[blk(L, L, Xd, Xd, p, dtype), blk(L, D, Xd, Xa, p, dtype)], [blk(D, L, Xa, Xd, p, dtype), blk(D, D, Xa, Xa, p, dtype)]]
    return (np.block([[q[0] for q in row] for row in parts]), np.block([[q[1] for q in row] for row in parts]))


def nugget_diag(p, Nd, Nb, nugget, nugget_type):
    r = trace_ratio(p, Nd, Nb)
    n0 = {'none': 0.0, 'identity': nugget, 'adaptive': nugget * r}[nugget_type]
    n1 = 0.0 if nugget_type == 'none' else nugget
    return np.concatenate([np.full(Nd, n0), np.full(Nd + Nb, n1)])


def extend_rows(names, Xt, Xd, Xb, coeff, p, dtype=np.float64):
    """({name: K_F @ coeff}, {name: sum of |terms| |coeff|}, {name: ||K_F||_2}) for the row functionals `names` at Xt"""
    Xd = np.asarray(Xd, dtype=np.float64).reshape(-1, 3); Xb = np.asarray(Xb, dtype=np.float64).reshape(-1, 3)
    Xa = np.concatenate([Xd, Xb], axis=0)
    coeff = np.asarray(coeff, dtype=dtype)
    out, terms, norms = {}, {}, {}
    for n in names:
        V0, A0 = blk(MULTI[n], MULTI['laplacian'], Xt, Xd, p, dtype)
        V1, A1 = blk(MULTI[n], MULTI['value'], Xt, Xa, p, dtype)
        K = np.concatenate([V0, V1], axis=1)
        out[n] = K @ coeff
        terms[n] = np.concatenate([A0, A1], axis=1) @ np.abs(coeff)
        norms[n] = float(np.linalg.norm(K.astype(np.float64), 2))
    return out, terms, norms


class NumpyPipeline:
    """The whole solve in numpy: Cholesky of Theta + nugget, Gauss-Newton by normal equations on S = L^{-1} A(z), loss history as the
    class API reports it (J(z_0) .. J(z_steps)).  -Delta u + alpha u^m = f, elimination formulation."""

    def __init__(self, Xd, Xb, p, nugget, f, g, alpha=1.0, m=3):
        self.Xd, self.Xb, self.p = Xd, Xb, p
        self.Nd, self.Nb = len(Xd), len(Xb)
        self.f, self.g, self.alpha, self.m = f, g, alpha, m
        self.T0, _ = theta(Xd, Xb, p)
        self.nug = nugget_diag(p, self.Nd, self.Nb, nugget, 'adaptive')

    def measurement(self, z):
        return np.concatenate([self.alpha * z ** self.m - self.f, z, self.g])

    def run(self, z0, steps, E=None):
        """(z, loss history, L); E: entrywise relative perturbation of Theta"""
        from scipy.linalg import solve_triangular
        T = self.T0 if E is None else self.T0 * (1.0 + E)
        L = np.linalg.cholesky(T + np.diag(self.nug))
        Nd, N = self.Nd, 2 * self.Nd + self.Nb
        z = np.array(z0, dtype=np.float64); hist = []
        for it in range(steps + 1):
            w = solve_triangular(L, self.measurement(z), lower=True)
            hist.append(float(w @ w))
            if it == steps:
                break
            A = np.zeros((N, Nd))
            A[:Nd] = np.diag(self.alpha * self.m * z ** (self.m - 1))
            A[Nd:2 * Nd] = np.eye(Nd)
            S = solve_triangular(L, A, lower=True)
            z = z - np.linalg.solve(S.T @ S, S.T @ w)
        return z, np.array(hist), L

    def sensitivity(self, z0, steps, z, hist, seed=7, reruns=3):
        """largest relative change of the final iterate (s_z) and of the loss history (s_J) under symmetric entrywise perturbations
        |E| <= 4 eps of Theta"""
        rng = np.random.RandomState(seed)
        s_z = s_J = 0.0
        for _ in range(reruns):
            E = rng.uniform(-4 * EPS, 4 * EPS, self.T0.shape)
            E = np.triu(E) + np.triu(E, 1).T
            z2, h2, _ = self.run(z0, steps, E)
            s_z = max(s_z, float(np.linalg.norm(z2 - z) / np.linalg.norm(z)))
            s_J = max(s_J, float(np.max(np.abs(h2 - hist) / hist)))
        return s_z, s_J


def truth(x1, x2, x3):
    return np.sin(np.pi * x1) * np.sin(np.pi * x2) * np.sin(np.pi * x3)


def rhs_for(alpha, m):
    return lambda x1, x2, x3: 3 * np.pi ** 2 * truth(x1, x2, x3) + alpha * truth(x1, x2, x3) ** m


# ---- CPU tests --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kernel,kp', KERNELS)
def test_closed_form_matches_symbolic_differentiation(kernel, kp):
    """all four blocks (and the first-derivative rows of the extension) at random pairs against sympy derivatives of kappa evaluated
    with 40 digits.  Bound 32 eps x sum|terms|: a Hermite factor carries at most 6 roundings, a product of three 20 half-ulps, the
    exp argument |arg| <= 17 here at 2 half-ulps per unit plus the exp itself -- about 30 eps in all; the two are computed from the
    same fp64 points, so the differences d are exact on both sides."""
    import sympy as sp
    import mpmath
    p = precisions(kernel, kp)
    xs = sp.symbols('x1:4'); ys = sp.symbols('y1:4')
    kap = sp.exp(-sum(sp.Rational(1, 2) * sp.Symbol(f'p{k}') * (xs[k] - ys[k]) ** 2 for k in range(3)))
    ps = [sp.Symbol(f'p{k}') for k in range(3)]

    def apply(expr, multi, var):
        return sum(sp.diff(expr, *[v for k in range(3) for v in [var[k]] * a[k]]) if sum(a) else expr for a in multi)

    rng = np.random.RandomState(11)
    X = rng.uniform(0, 1, (12, 3)); Y = rng.uniform(0, 1, (12, 3))
    Y[:2] = X[:2]                                                         # coincident points (d = 0)
    pairs = [('laplacian', 'laplacian'), ('laplacian', 'value'), ('value', 'laplacian'), ('value', 'value'),
             ('d1', 'laplacian'), ('d2', 'laplacian'), ('d3', 'laplacian'), ('d3', 'value'), ('d1', 'value'), ('d2', 'value')]
    mpmath.mp.dps = 40
    for fx, fy in pairs:
        expr = apply(apply(kap, MULTI[fx], xs), MULTI[fy], ys)
        fn = sp.lambdify(list(xs) + list(ys) + ps, expr, 'mpmath')
        V, A = blk(MULTI[fx], MULTI[fy], X, Y, p)
        for i in range(len(X)):
            args = [mpmath.mpf(float(v)) for v in list(X[i]) + list(Y[i]) + list(p)]
            want = fn(*args)
            err = abs(mpmath.mpf(float(V[i, i])) - want)
            assert err <= 32 * EPS * A[i, i] + 1e-300, (fx, fy, i, float(err / (EPS * A[i, i])))


@pytest.mark.parametrize('kernel,kp', KERNELS)
def test_diagonal_values_and_trace_ratio(kernel, kp):
    p = precisions(kernel, kp)
    rng = np.random.RandomState(2)
    Nd, Nb = 23, 12
    Xd = rng.uniform(0, 1, (Nd, 3)); Xb = rng.uniform(0, 1, (Nb, 3))
    T, _ = theta(Xd, Xb, p)
    assert np.allclose(np.diag(T)[:Nd], diag_lap_lap(p), rtol=8 * EPS, atol=0)
    assert np.array_equal(np.diag(T)[Nd:], np.ones(Nd + Nb))
    if kernel == 'Gaussian':
        assert abs(diag_lap_lap(p) - 15 * p[0] ** 2) <= 8 * EPS * 15 * p[0] ** 2
    r = np.trace(T[:Nd, :Nd]) / np.trace(T[Nd:, Nd:])
    assert abs(r - trace_ratio(p, Nd, Nb)) <= 64 * EPS * r               # (np.trace sums Nd rounded values)
    assert np.array_equal(T, T.T)


def _faces_hit(X, dom):
    dom = np.asarray(dom, dtype=float)
    return sum((X[:, k] == dom[k, s]).astype(int) for k in range(3) for s in range(2))


def test_random_sampler_3d():
    from src.sample_points import sampled_pts_rdm3d
    dom = [[0, 1], [-1, 2], [0.5, 0.75]]
    np.random.seed(5)
    Xd, Xb = sampled_pts_rdm3d(150, 96, dom)
    assert Xd.shape == (150, 3) and Xb.shape == (96, 3)
    d = np.asarray(dom)
    assert np.all(Xd > d[:, 0]) and np.all(Xd < d[:, 1])                 # strictly inside
    assert np.all(Xb >= d[:, 0]) and np.all(Xb <= d[:, 1])
    assert np.array_equal(_faces_hit(Xb, dom), np.ones(96, dtype=int))   # every boundary point on exactly one face
    per_face = [int(np.sum(Xb[:, k] == d[k, s])) for k in range(3) for s in range(2)]
    assert per_face == [16] * 6
    np.random.seed(5)
    Xd2, Xb2 = sampled_pts_rdm3d(150, 96, dom)
    assert np.array_equal(Xd, Xd2) and np.array_equal(Xb, Xb2)           # a fixed seed is deterministic
    with pytest.raises(ValueError, match='divisible by 6'):
        sampled_pts_rdm3d(150, 100, dom)
    with pytest.raises(ValueError, match=r'\(3, 2\)'):
        sampled_pts_rdm3d(10, 6, [[0, 1], [0, 1]])


def test_grid_sampler_3d():
    from src.sample_points import sampled_pts_grid3d
    dom = [[0, 1], [0, 2], [-1, 1]]
    Xd, Xb = sampled_pts_grid3d(512, 488, dom)                            # 10^3 nodes: 8^3 inside
    assert Xd.shape == (512, 3) and Xb.shape == (488, 3)
    d = np.asarray(dom, dtype=float)
    assert np.all(Xd > d[:, 0]) and np.all(Xd < d[:, 1])
    assert np.all(_faces_hit(Xb, dom) >= 1)                              # faces, edges (2 faces) and corners (3 faces), each node once
    assert sorted(np.bincount(_faces_hit(Xb, dom))[1:].tolist()) == sorted([6 * 64, 12 * 8, 8])
    allp = np.concatenate([Xd, Xb])
    assert len(np.unique(allp, axis=0)) == 1000
    assert np.allclose(np.unique(allp[:, 1]), np.linspace(0, 2, 10))
    Xd2, Xb2 = sampled_pts_grid3d(600, 500, dom)                          # rounded down to the same grid
    assert np.array_equal(Xd, Xd2) and np.array_equal(Xb, Xb2)
    with pytest.raises(ValueError):
        sampled_pts_grid3d(10, 6, dom)


def test_prototypes_hold_the_two_new_entry_points():
    from gpk import _lib
    from gpk.device import FUNCTIONAL3D
    assert len(_lib.PROTOTYPES['gpk_assemble3d'][1]) == 12
    assert len(_lib.PROTOTYPES['gpk_extend_functionals3d'][1]) == 13
    assert FUNCTIONAL3D == FN_BITS
    hdr = open(os.path.join(ROOT, 'include', 'gpk.h')).read()
    assert '#define GPK_FN_D3 32' in hdr
    import re
    for name in ('gpk_assemble3d', 'gpk_extend_functionals3d'):
        assert re.search(r'\bint\s+' + name + r'\s*\(', hdr), name


def test_class_and_facade_are_importable_and_fail_loudly_without_a_device():
    import gpk
    from src.PDEs import Nonlinear_elliptic3d
    from src.solver import _EQUATIONS, solver_GP
    assert 'Nonlinear_elliptic3d' in _EQUATIONS
    eqn = Nonlinear_elliptic3d(alpha=1.0, m=3, bdy=truth, rhs=rhs_for(1.0, 3), domain=np.array(UNIT_CUBE))
    assert eqn._system == 'Nonlinear_elliptic'
    np.random.seed(0)
    eqn.sampled_pts(30, 12)
    assert eqn.X_domain.shape == (30, 3) and eqn.X_boundary.shape == (12, 3)
    assert np.array_equal(eqn.bdy_g, truth(*eqn.X_boundary.T)) and np.array_equal(eqn.rhs_f, rhs_for(1.0, 3)(*eqn.X_domain.T))
    with pytest.raises(ValueError):
        eqn.get_sampled_points(np.zeros((4, 2)), np.zeros((6, 3)))         # planar points are refused
    for name in ('Gram_matrix', 'Gram_Cholesky', 'loss', 'grad_loss', 'Hessian_GN', 'GN_loss', 'GN_method', 'extend_sol',
                 'extend_derivatives', 'PDE_residual'):
        assert callable(getattr(eqn, name)), name

    class Cfg:
        alpha, m = 1.0, 3
    s = solver_GP(Cfg(), 'Nonlinear_elliptic3d')
    s.set_equation(bdy=truth, rhs=rhs_for(1.0, 3), domain=np.array(UNIT_CUBE), print_option=False)
    assert isinstance(s.eqn, Nonlinear_elliptic3d)
    with pytest.raises(NotImplementedError):
        s.show_sample()
    try:
        eqn.Gram_matrix(kernel='Gaussian', kernel_parameter=0.3, nugget=1e-8)
    except gpk.GpkError as e:                                             # no device (or no library): loud, and no CPU route
        assert 'no CPU fallback' in str(e)
    else:                                                                 # a GPU is present: the call is the real one
        assert eqn.Theta.shape == (72, 72) and eqn.ratio == pytest.approx(trace_ratio(precisions('Gaussian', 0.3), 30, 12), rel=1e-14)


def test_driver_manufactured_solution_is_consistent():
    """f of main_NonLinElliptic3d is -Laplace(u*) + alpha u*^m: checked by central differences of u*"""
    import main_NonLinElliptic3d as drv
    u, f = drv.manufactured(1.0, 3.0)
    rng = np.random.RandomState(0)
    X = rng.uniform(0.1, 0.9, (20, 3)); h = 1e-4
    lap = sum((u(*(X + h * e).T) - 2 * u(*X.T) + u(*(X - h * e).T)) / h ** 2 for e in np.eye(3))
    assert np.allclose(f(*X.T), -lap + u(*X.T) ** 3, rtol=0, atol=1e-4)
    assert drv.cube_grid().shape == (8000, 3)
    cfg = drv.parse(['--show_figure', ''])
    assert (cfg.kernel, cfg.N_domain, cfg.N_boundary, cfg.GNsteps) == ('Gaussian', 1000, 486, 6)
