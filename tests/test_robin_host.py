"""Neumann / Robin / mixed boundary functionals for the 2-D elliptic equation: the host-side expectation and its CPU checks.

The expectation is the closed form of DESIGN.md section K, "Boundary functionals".  Every point q of the second block carries
phi_q = c0 delta + c1 d_1 + c2 d_2 -- (1,0,0) at a domain point, `coeffs[b]` at boundary point b -- and with d = x - y,
kappa = exp(-(p1 d1^2 + p2 d2^2) / 2) and the 1-D Hermite factors h0..h4
    <F at x, G at y> kappa = sum_{(w, alpha) in F} sum_{(w', beta) in G} w w' (-1)^{|alpha|} h_{alpha1+beta1}(p1, d1) h_{alpha2+beta2}(p2, d2) kappa
over weighted multi-index lists (`blk`).  It is checked here against the oracle's closed forms under their reference names
(oracle.gp_oracle.deriv_kernel) and against the oracle's Dirichlet assembly.  The GPU tests (test_gpu_robin.py) import `theta`,
`nugget_diag`, `extend_rows`, `NumpyPipeline` and the tables from this module."""
import os
import re
import sys

import numpy as np
import pytest

from oracle import gp_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'nonlinpdes-gpsolver_amd')
if PKG not in sys.path:
    sys.path.insert(0, PKG)

EPS = np.finfo(np.float64).eps
LD = np.longdouble

MULTI = {'value': [(0, 0)], 'd1': [(1, 0)], 'd2': [(0, 1)], 'd2d2': [(0, 2)], 'laplacian': [(2, 0), (0, 2)]}
FN_BITS = {'value': 1, 'd1': 2, 'd2': 4, 'd2d2': 8, 'laplacian': 16}
PHI = ((0, 0), (1, 0), (0, 1))                                             # multi-indices of the three parts of phi
KERNELS = (('Gaussian', 0.2), ('anisotropic_Gaussian', (0.3, 0.25)))
UNIT_SQUARE = [[0, 1], [0, 1]]
COEFF_SETS = ('dirichlet', 'neumann', 'robin', 'mixed')
# (part of phi at x, part of phi at y) -> method of src/kernels.py (oracle.deriv_kernel)
PHI_PHI_NAME = [['kappa', 'D_y1_kappa', 'D_y2_kappa'],
                ['D_x1_kappa', 'D_x1_D_y1_kappa', 'D_x1_D_y2_kappa'],
                ['D_x2_kappa', 'D_x2_D_y1_kappa', 'D_x2_D_y2_kappa']]
LAP_PHI_NAME = ['Delta_x_kappa', 'Delta_x_D_y1_kappa', 'Delta_x_D_y2_kappa']


def precisions(kernel, kp):
    return O.kernel_precisions(kernel, kp)


def hermite(p, d):
    q = p * d
    q2 = q * q
    return (np.ones_like(d), q, q2 - p, q * (q2 - 3 * p), q2 * (q2 - 6 * p) + 3 * p * p)


def plain(name, n):
    """functional `name` of MULTI at n points as a weighted multi-index list"""
    return [(np.ones(n), a) for a in MULTI[name]]


def phi(coeffs):
    """c0 delta + c1 d_1 + c2 d_2 per point, coeffs (n,3)"""
    coeffs = np.asarray(coeffs, dtype=np.float64).reshape(-1, 3)
    return [(coeffs[:, k], PHI[k]) for k in range(3)]


def blk(fx, fy, X, Y, p, dtype=np.float64):
    """(value, sum of |terms|) of <fx at X[i], fy at Y[j]> kappa, both (len(X), len(Y)); fx, fy: weighted multi-index lists.  dtype =
    longdouble gives the expectation three digits below fp64 rounding (the differences d are exact in either: X, Y are fp64)."""
    X = np.asarray(X, dtype=dtype).reshape(-1, 2); Y = np.asarray(Y, dtype=dtype).reshape(-1, 2)
    p = [dtype(v) for v in p]
    d = [X[:, None, k] - Y[None, :, k] for k in range(2)]
    kap = np.exp(-(p[0] * d[0] * d[0] + p[1] * d[1] * d[1]) / 2)
    h = [hermite(p[k], d[k]) for k in range(2)]
    val = np.zeros_like(kap); mag = np.zeros_like(kap)
    for wx, a in fx:
        for wy, b in fy:
            t = (-1) ** sum(a) * np.asarray(wx, dtype=dtype)[:, None] * np.asarray(wy, dtype=dtype)[None, :] \
                * h[0][a[0] + b[0]] * h[1][a[1] + b[1]] * kap
            val += t
            mag += np.abs(t)
    return val, mag


def all_coeffs(Nd, coeffs, Nb):
    """(Nd+Nb, 3): (1,0,0) at the domain points, then the boundary coefficients (None: (1,0,0) there too)"""
    c = np.zeros((Nd + Nb, 3)); c[:, 0] = 1.0
    if coeffs is not None:
        c[Nd:] = np.asarray(coeffs, dtype=np.float64).reshape(Nb, 3)
    return c


def theta(Xd, Xb, coeffs, p, dtype=np.float64):
    """(Theta without nugget, T = sum of |terms| kappa per entry) in the elliptic layout: Laplacian on Xd, phi on [Xd; Xb]"""
    Xd = np.asarray(Xd, dtype=np.float64).reshape(-1, 2); Xb = np.asarray(Xb, dtype=np.float64).reshape(-1, 2)
    Xa = np.concatenate([Xd, Xb], axis=0)
    L, F = plain('laplacian', len(Xd)), phi(all_coeffs(len(Xd), coeffs, len(Xb)))
    parts = [[blk(L, L, Xd, Xd, p, dtype), blk(L, F, Xd, Xa, p, dtype)], [blk(F, L, Xa, Xd, p, dtype), blk(F, F, Xa, Xa, p, dtype)]]
    return (np.block([[q[0] for q in row] for row in parts]), np.block([[q[1] for q in row] for row in parts]))


def diag_lap_lap(p):
    return 3 * p[0] * p[0] + 2 * p[0] * p[1] + 3 * p[1] * p[1]


def trace_ratio(p, Nd, Nb, coeffs, dtype=np.float64):
    """Nd (3 p1^2 + 2 p1 p2 + 3 p2^2) / (Nd + sum_b (c0_b^2 + p1 c1_b^2 + p2 c2_b^2)), the boundary sum in index order"""
    p = [dtype(v) for v in p]
    c = all_coeffs(Nd, coeffs, Nb)[Nd:].astype(dtype)
    s = dtype(0)
    for b in range(Nb):
        s += c[b, 0] * c[b, 0] + p[0] * c[b, 1] * c[b, 1] + p[1] * c[b, 2] * c[b, 2]
    return dtype(Nd) * diag_lap_lap(p) / (dtype(Nd) + s)


def nugget_diag(p, Nd, Nb, coeffs, nugget, nugget_type):
    r = float(trace_ratio(p, Nd, Nb, coeffs, LD))
    n0 = {'none': 0.0, 'identity': nugget, 'adaptive': nugget * r}[nugget_type]
    n1 = 0.0 if nugget_type == 'none' else nugget
    return np.concatenate([np.full(Nd, n0), np.full(Nd + Nb, n1)])


def extend_rows(names, Xt, Xd, Xb, coeffs, cvec, p, dtype=np.float64):
    """({name: K_F @ cvec}, {name: sum of |terms| |cvec|}, {name: ||K_F||_2}): the extension rows for the row functionals `names` at Xt"""
    Xd = np.asarray(Xd, dtype=np.float64).reshape(-1, 2); Xb = np.asarray(Xb, dtype=np.float64).reshape(-1, 2)
    Xa = np.concatenate([Xd, Xb], axis=0)
    cvec = np.asarray(cvec, dtype=dtype)
    L, F = plain('laplacian', len(Xd)), phi(all_coeffs(len(Xd), coeffs, len(Xb)))
    out, terms, norms = {}, {}, {}
    for n in names:
        V0, A0 = blk(plain(n, len(Xt)), L, Xt, Xd, p, dtype)
        V1, A1 = blk(plain(n, len(Xt)), F, Xt, Xa, p, dtype)
        K = np.concatenate([V0, V1], axis=1)
        out[n] = K @ cvec
        terms[n] = np.concatenate([A0, A1], axis=1) @ np.abs(cvec)
        norms[n] = float(np.linalg.norm(K.astype(np.float64), 2))
    return out, terms, norms


class NumpyPipeline:
    """The whole solve in numpy: Cholesky of Theta + nugget, Gauss-Newton by normal equations on S = L^{-1} A(z), loss history as the
    class API reports it (J(z_0) .. J(z_steps)).  -Delta u + alpha u^m = f, elimination formulation; g = the prescribed values of phi_b u."""

    def __init__(self, Xd, Xb, coeffs, p, nugget, f, g, alpha=1.0, m=3):
        self.Xd, self.Xb, self.coeffs, self.p = Xd, Xb, coeffs, p
        self.Nd, self.Nb = len(Xd), len(Xb)
        self.f, self.g, self.alpha, self.m = f, g, alpha, m
        self.T0, _ = theta(Xd, Xb, coeffs, p)
        self.nug = nugget_diag(p, self.Nd, self.Nb, coeffs, nugget, 'adaptive')

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


# ---- the manufactured problem of the end-to-end tests ------------------------------------------------------------------------------
AMP = 4.0                                                                  # amplitude of the 4 pi mode


def truth(x1, x2):
    pi = np.pi
    return np.sin(pi * x1) * np.sin(pi * x2) + AMP * np.sin(4 * pi * x1) * np.sin(4 * pi * x2)


def truth_grad(x1, x2):
    pi = np.pi
    return (pi * np.cos(pi * x1) * np.sin(pi * x2) + 4 * pi * AMP * np.cos(4 * pi * x1) * np.sin(4 * pi * x2),
            pi * np.sin(pi * x1) * np.cos(pi * x2) + 4 * pi * AMP * np.sin(4 * pi * x1) * np.cos(4 * pi * x2))


def rhs_for(alpha, m):
    pi = np.pi

    def f(x1, x2):
        lap = -2 * pi ** 2 * np.sin(pi * x1) * np.sin(pi * x2) - 32 * pi ** 2 * AMP * np.sin(4 * pi * x1) * np.sin(4 * pi * x2)
        return -lap + alpha * truth(x1, x2) ** m
    return f


def operator_value(coeffs, X):
    """c0 u* + c1 u*_x1 + c2 u*_x2 at the points X (n,2) with coeffs (n,3)"""
    u1, u2 = truth_grad(X[:, 0], X[:, 1])
    return coeffs[:, 0] * truth(X[:, 0], X[:, 1]) + coeffs[:, 1] * u1 + coeffs[:, 2] * u2


def bdy_for(bc, beta, domain=UNIT_SQUARE):
    """the class's bdy callback: the value of the boundary operator on u* (normals from the point itself)"""
    def g(x1, x2):
        X = np.stack([np.asarray(x1, dtype=np.float64).ravel(), np.asarray(x2, dtype=np.float64).ravel()], axis=1)
        return operator_value(operator_coeffs(bc, beta, X, domain), X).reshape(np.shape(x1))
    return g


def operator_coeffs(bc, beta, Xb, domain=UNIT_SQUARE):
    from src.sample_points import boundary_normals
    Xb = np.asarray(Xb, dtype=np.float64).reshape(-1, 2)
    c = np.zeros((len(Xb), 3))
    if bc == 'dirichlet':
        c[:, 0] = 1.0
        return c
    c[:, 0] = beta if bc == 'robin' else 0.0
    c[:, 1:] = boundary_normals(Xb, domain)
    return c


def face_points(rng, Nb, domain=UNIT_SQUARE):
    """Nb points on the boundary of the rectangle, point b on face b % 4 (any Nb, unlike the samplers)"""
    d = np.asarray(domain, dtype=float)
    X = np.empty((Nb, 2))
    for b in range(Nb):
        axis, side = (b % 4) // 2, b % 2
        X[b, axis] = d[axis, side]
        X[b, 1 - axis] = rng.uniform(d[1 - axis, 0], d[1 - axis, 1])
    return X


def coeff_set(name, Xb, rng=None, domain=UNIT_SQUARE):
    """the coefficient sets of the GPU tests: all Dirichlet, all Neumann, Robin beta = 2, a random mixture with |c| <= 3"""
    if name == 'mixed':
        return rng.uniform(-3.0, 3.0, (len(Xb), 3))
    return operator_coeffs(name, 2.0, Xb, domain)


# ---- CPU tests --------------------------------------------------------------------------------------------------------
def _points(seed, Nd, Nb):
    rng = np.random.RandomState(seed)
    Xd = rng.uniform(0, 1, (Nd, 2))
    Xb = face_points(rng, Nb)
    return rng, Xd, Xb


@pytest.mark.parametrize('name', COEFF_SETS)
@pytest.mark.parametrize('kernel,kp', KERNELS)
def test_theta_is_the_sum_of_the_oracles_named_kernels(kernel, kp, name):
    """Theta assembled block by block from oracle.deriv_kernel under the reference's method names, weighted by the coefficients.  Both
    sides are fp64 with the same kappa (the same expression); they differ in the order of the Hermite arithmetic and of the sum: at most
    ~3 eps per Hermite product and 4 eps for a nine-term sum on either side -- 16 eps T."""
    Nd, Nb = 19, 12
    rng, Xd, Xb = _points(3, Nd, Nb)
    Xd[0] = Xb[0]                                                          # a coincident pair off the diagonal
    c = coeff_set(name, Xb, rng)
    p = precisions(kernel, kp)
    T, mag = theta(Xd, Xb, c, p)
    Xa = np.concatenate([Xd, Xb]); ca = all_coeffs(Nd, c, Nb)
    P = lambda nm, X, Y: O._pairs(nm, X, Y, kernel, kp)
    want = np.zeros_like(T)
    want[:Nd, :Nd] = P('Delta_x_Delta_y_kappa', Xd, Xd)
    lp = sum(ca[None, :, j] * P(LAP_PHI_NAME[j], Xd, Xa) for j in range(3))
    want[:Nd, Nd:] = lp
    want[Nd:, :Nd] = lp.T
    want[Nd:, Nd:] = sum(ca[:, None, i] * ca[None, :, j] * P(PHI_PHI_NAME[i][j], Xa, Xa) for i in range(3) for j in range(3))
    assert np.all(np.abs(T - want) <= 16 * EPS * mag), float(np.max(np.abs(T - want) / (EPS * mag + 1e-300)))
    assert np.allclose(T, T.T, rtol=0, atol=16 * EPS * np.max(mag))
    # the diagonal of the phi block: c0^2 + p1 c1^2 + p2 c2^2
    dg = ca[:, 0] ** 2 + p[0] * ca[:, 1] ** 2 + p[1] * ca[:, 2] ** 2
    assert np.allclose(np.diag(T)[Nd:], dg, rtol=8 * EPS, atol=0)
    assert np.allclose(np.diag(T)[:Nd], diag_lap_lap(p), rtol=8 * EPS, atol=0)


@pytest.mark.parametrize('kernel,kp', KERNELS)
def test_dirichlet_coefficients_give_the_oracles_elliptic_assembly(kernel, kp):
    Nd, Nb = 23, 9
    rng, Xd, Xb = _points(4, Nd, Nb)
    p = precisions(kernel, kp)
    want = O.gram_matrix_assembly(Xd, Xb, 'Nonlinear_elliptic', kernel, kp)
    for c in (None, coeff_set('dirichlet', Xb)):
        T, mag = theta(Xd, Xb, c, p)
        assert np.all(np.abs(T - want) <= 16 * EPS * mag)
        assert np.array_equal(T[Nd:, Nd:], want[Nd:, Nd:])                # products by 1 and sums with 0 are exact
    # the longdouble expectation sees the fp64 oracle's rounding of the exp argument as well (2 eps |arg|, |arg| <= 27.1 here): the
    # budget of the device test, 128 eps T (test_gpu_robin.py)
    Tl, _ = theta(Xd, Xb, None, p, dtype=LD)
    assert np.all(np.abs(Tl - want.astype(LD)) <= 128 * EPS * mag)


@pytest.mark.parametrize('name', COEFF_SETS)
@pytest.mark.parametrize('kernel,kp', KERNELS)
def test_adaptive_ratio_against_the_oracles_nugget(kernel, kp, name):
    Nd, Nb = 21, 14
    rng, Xd, Xb = _points(5, Nd, Nb)
    c = coeff_set(name, Xb, rng)
    p = precisions(kernel, kp)
    T, _ = theta(Xd, Xb, c, p)
    Tn, ratios = O.add_nugget(T, 'Nonlinear_elliptic', Nd, Nb, 1e-3, 'adaptive')
    r = float(trace_ratio(p, Nd, Nb, c, LD))
    assert abs(ratios[0] - r) <= 64 * EPS * r                             # (np.trace sums Nd and Nd+Nb rounded values)
    assert np.allclose(np.diag(Tn) - np.diag(T), nugget_diag(p, Nd, Nb, c, 1e-3, 'adaptive'), rtol=1e-9, atol=0)
    assert np.array_equal(nugget_diag(p, Nd, Nb, c, 1e-3, 'identity'), np.full(2 * Nd + Nb, 1e-3))
    assert not np.any(nugget_diag(p, Nd, Nb, c, 1e-3, 'none'))
    if name == 'dirichlet':
        assert r == pytest.approx(Nd * diag_lap_lap(p) / (Nd + Nb), rel=4 * EPS)


def test_extension_rows_reduce_to_theta_rows_at_collocation_points():
    """value / laplacian rows at the domain points are rows of Theta; the operator rows at the boundary points likewise"""
    kernel, kp = KERNELS[1]
    Nd, Nb = 11, 8
    rng, Xd, Xb = _points(6, Nd, Nb)
    c = coeff_set('mixed', Xb, rng)
    p = precisions(kernel, kp)
    T, mag = theta(Xd, Xb, c, p)
    cvec = rng.normal(size=2 * Nd + Nb)
    rows, terms, _ = extend_rows(('value', 'laplacian'), Xd, Xd, Xb, c, cvec, p)
    assert np.all(np.abs(rows['laplacian'] - T[:Nd] @ cvec) <= 16 * EPS * terms['laplacian'])
    assert np.all(np.abs(rows['value'] - T[Nd:2 * Nd] @ cvec) <= 16 * EPS * terms['value'])
    rows, terms, _ = extend_rows(('value', 'd1', 'd2'), Xb, Xd, Xb, c, cvec, p)
    got = c[:, 0] * rows['value'] + c[:, 1] * rows['d1'] + c[:, 2] * rows['d2']
    scale = np.abs(c[:, 0]) * terms['value'] + np.abs(c[:, 1]) * terms['d1'] + np.abs(c[:, 2]) * terms['d2']
    assert np.all(np.abs(got - T[2 * Nd:] @ cvec) <= 16 * EPS * scale)


def test_boundary_normals_on_both_samplers_corners_and_off_boundary_points():
    from src.sample_points import boundary_normals, sampled_pts_grid, sampled_pts_rdm
    dom = np.array([[0, 1], [-1, 2]])
    np.random.seed(3)
    _, Xb = sampled_pts_rdm(50, 40, dom)
    state = np.random.get_state()[1].copy()
    n = boundary_normals(Xb, dom)
    assert np.array_equal(np.random.get_state()[1], state)                # draws nothing
    # the random sampler's faces in its order: bottom, right, top, left
    want = np.repeat(np.array([[0.0, -1.0], [1.0, 0.0], [0.0, 1.0], [-1.0, 0.0]]), 10, axis=0)
    assert n.shape == (40, 2) and np.array_equal(n, want)
    _, Xg = sampled_pts_grid(49, 32, dom)                                  # 9 x 9 nodes, 32 on the boundary, corners included
    ng = boundary_normals(Xg, dom)
    assert np.array_equal(np.abs(ng).sum(axis=1), np.ones(len(Xg)))       # unit, axis-aligned
    for x, nrm in zip(Xg, ng):
        on1 = x[0] in (0.0, 1.0)
        if on1:                                                           # x1 faces are tested first: they decide the corners
            assert tuple(nrm) == ((-1.0, 0.0) if x[0] == 0.0 else (1.0, 0.0))
        else:
            assert tuple(nrm) == ((0.0, -1.0) if x[1] == -1.0 else (0.0, 1.0))
    corners = np.array([[0.0, -1.0], [0.0, 2.0], [1.0, -1.0], [1.0, 2.0]])
    assert sum(any(np.array_equal(x, c) for x in Xg) for c in corners) >= 3   # (the grid sampler's edges hold at least three corners)
    assert np.array_equal(boundary_normals(corners, dom), [[-1.0, 0.0], [-1.0, 0.0], [1.0, 0.0], [1.0, 0.0]])
    assert boundary_normals(np.zeros((0, 2)), dom).shape == (0, 2)
    with pytest.raises(ValueError, match='no face'):
        boundary_normals(np.array([[0.0, 0.5], [0.5, 0.5]]), dom)
    with pytest.raises(ValueError, match='no face'):
        boundary_normals(np.array([[np.nextafter(1.0, 0.0), 0.5]]), dom)  # exact equality, no tolerance


def test_prototypes_and_header_hold_the_two_new_entry_points():
    from gpk import _lib
    assert len(_lib.PROTOTYPES['gpk_assemble_bc'][1]) == 13
    assert len(_lib.PROTOTYPES['gpk_extend_functionals_bc'][1]) == 14
    hdr = open(os.path.join(ROOT, 'include', 'gpk.h')).read()
    for name in ('gpk_assemble_bc', 'gpk_extend_functionals_bc'):
        assert re.search(r'\bint\s+' + name + r'\s*\(', hdr), name
    import gpk
    for name in ('assemble_bc', 'extend_functionals_bc'):
        assert callable(getattr(gpk.Context, name)), name


class _FakeArray:
    def free(self):
        pass


class _FakeContext:
    """records which assembly entry point the class takes"""

    def __init__(self):
        self.calls = []

    def assemble(self, layout, kernel, kp, Xd, Xb, nugget, nugget_type):
        self.calls.append(('assemble', layout))
        return _FakeArray(), [123.0, 0.0, 0.0]

    def assemble_bc(self, kernel, kp, Xd, Xb, bc, nugget, nugget_type):
        self.calls.append(('assemble_bc', np.array(bc)))
        return _FakeArray(), 77.0


def test_class_arguments_and_selection_of_the_code_path(monkeypatch):
    import src.PDEs as P
    from src.PDEs import Nonlinear_elliptic2d
    fake = _FakeContext()
    monkeypatch.setattr(P, 'get_context', lambda: fake)
    f = rhs_for(1.0, 3)
    with pytest.raises(ValueError):
        Nonlinear_elliptic2d(bdy=truth, rhs=f, bc='periodic')
    np.random.seed(0)
    Xd, Xb = P.sampled_pts_rdm(30, 16, np.array(UNIT_SQUARE))

    # default: Dirichlet, no coefficients, today's entry point
    eqn = Nonlinear_elliptic2d(alpha=1.0, m=3, bdy=truth, rhs=f, domain=np.array(UNIT_SQUARE))
    assert (eqn.bc, eqn.robin_beta, eqn.boundary_coeffs) == ('dirichlet', 1.0, None)
    eqn.get_sampled_points(Xd, Xb)
    assert eqn.boundary_coeffs is None and np.array_equal(eqn.bdy_g, truth(Xb[:, 0], Xb[:, 1]))
    eqn.Gram_matrix(kernel='Gaussian', kernel_parameter=0.2, nugget=1e-8, nugget_type='adaptive')
    assert fake.calls == [('assemble', 'Nonlinear_elliptic')] and eqn.ratio == 123.0

    # Neumann / Robin: coefficients from the normals, the new entry point
    for bc, beta in (('neumann', 0.0), ('robin', 2.0)):
        fake.calls.clear()
        eqn = Nonlinear_elliptic2d(alpha=1.0, m=3, bdy=bdy_for(bc, 2.0), rhs=f, domain=np.array(UNIT_SQUARE), bc=bc, robin_beta=2.0)
        eqn.get_sampled_points(Xd, Xb)
        want = operator_coeffs(bc, 2.0, Xb)
        assert np.array_equal(eqn.boundary_coeffs, want) and np.all(want[:, 0] == beta)
        assert np.array_equal(eqn.bdy_g, operator_value(want, Xb))         # bdy returns the value of the boundary operator
        eqn.Gram_matrix(kernel='Gaussian', kernel_parameter=0.2, nugget=1e-8, nugget_type='adaptive')
        assert [c[0] for c in fake.calls] == ['assemble_bc'] and np.array_equal(fake.calls[0][1], want) and eqn.ratio == 77.0
        with pytest.raises(AttributeError):
            eqn.Gram_matrix(nugget_type='other')

    # a custom operator: set after sampling, dropped when the points change
    fake.calls.clear()
    eqn = Nonlinear_elliptic2d(alpha=1.0, m=3, bdy=truth, rhs=f, domain=np.array(UNIT_SQUARE))
    eqn.get_sampled_points(Xd, Xb)
    custom = np.random.RandomState(1).uniform(-3, 3, (16, 3))
    with pytest.raises(ValueError):
        eqn.set_boundary_operator(custom[:5])
    eqn.set_boundary_operator(custom)
    eqn.Gram_matrix()
    assert [c[0] for c in fake.calls] == ['assemble_bc'] and np.array_equal(fake.calls[0][1], custom)
    eqn.get_sampled_points(Xd, Xb)
    assert eqn.boundary_coeffs is None
    eqn.Gram_matrix()
    assert fake.calls[-1][0] == 'assemble'
    assert callable(eqn.boundary_residual)


def test_facade_passes_the_boundary_condition_through(capsys):
    from src.PDEs import Nonlinear_elliptic2d
    from src.solver import solver_GP

    class Old:                                                              # a configuration that knows nothing about bc
        alpha, m = 1.0, 3

    class New(Old):
        bc, robin_beta = 'robin', 2.0
    s = solver_GP(Old(), 'Nonlinear_elliptic')
    s.set_equation(bdy=truth, rhs=rhs_for(1.0, 3), domain=np.array(UNIT_SQUARE))
    assert isinstance(s.eqn, Nonlinear_elliptic2d) and s.eqn.bc == 'dirichlet'
    assert 'Boundary condition' not in capsys.readouterr().out            # the Dirichlet header is the reference's
    s = solver_GP(New(), 'Nonlinear_elliptic')
    s.set_equation(bdy=bdy_for('robin', 2.0), rhs=rhs_for(1.0, 3), domain=np.array(UNIT_SQUARE))
    assert (s.eqn.bc, s.eqn.robin_beta) == ('robin', 2.0)
    assert '[Boundary condition] Robin' in capsys.readouterr().out
    np.random.seed(1)
    s.auto_sample(40, 16, print_option=False)
    assert np.array_equal(s.eqn.boundary_coeffs, operator_coeffs('robin', 2.0, s.eqn.X_boundary))


def test_driver_boundary_data_is_the_operator_on_the_manufactured_solution():
    import main_NonLinElliptic2d as drv
    cfg = drv.parse([])
    assert (cfg.bc, cfg.robin_beta) == ('dirichlet', 1.0)
    cfg = drv.parse(['--bc', 'robin', '--robin_beta', '2.5'])
    assert (cfg.bc, cfg.robin_beta) == ('robin', 2.5)
    u, _ = drv.manufactured(1.0, 3.0)
    assert drv.boundary_data(u, 'dirichlet', 1.0) is u
    rng = np.random.RandomState(0)
    Xb = face_points(rng, 40)
    from src.sample_points import boundary_normals
    n = boundary_normals(Xb, UNIT_SQUARE)
    h = 1e-6                                                                # central difference of u* along the normal
    dudn = (u(*(Xb + h * n).T) - u(*(Xb - h * n).T)) / (2 * h)
    assert np.allclose(drv.boundary_data(u, 'neumann', 1.0)(Xb[:, 0], Xb[:, 1]), dudn, rtol=0, atol=1e-6)
    assert np.allclose(drv.boundary_data(u, 'robin', 2.5)(Xb[:, 0], Xb[:, 1]), 2.5 * u(*Xb.T) + dudn, rtol=0, atol=1e-6)


def test_manufactured_problem_of_the_end_to_end_tests_is_consistent():
    rng = np.random.RandomState(0)
    X = rng.uniform(0.1, 0.9, (20, 2)); h = 1e-4
    lap = sum((truth(*(X + h * e).T) - 2 * truth(*X.T) + truth(*(X - h * e).T)) / h ** 2 for e in np.eye(2))
    assert np.allclose(rhs_for(1.0, 3)(*X.T), -lap + truth(*X.T) ** 3, rtol=0, atol=1e-3)
    g1, g2 = truth_grad(*X.T)
    assert np.allclose(g1, (truth(X[:, 0] + h, X[:, 1]) - truth(X[:, 0] - h, X[:, 1])) / (2 * h), rtol=0, atol=1e-4)
    assert np.allclose(g2, (truth(X[:, 0], X[:, 1] + h) - truth(X[:, 0], X[:, 1] - h)) / (2 * h), rtol=0, atol=1e-4)
