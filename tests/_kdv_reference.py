"""Reference of the dispersive Gram layout and of the KdV Gauss-Newton iteration (CPU only).

1.  The Gram entries of gpk_assemble_disp in long double.  Not the expanded polynomials of csrc/gpk_assemble_disp.hip: the probabilists'
    Hermite polynomials come from numpy.polynomial.hermite_e (Clenshaw recursion on the basis coefficients) at s = sqrt(p) d, and
        d_x^m d_y^n exp(-p (x - y)^2 / 2) = (-1)^m p^((m+n)/2) He_(m+n)(sqrt(p) (x - y)) exp(-p (x - y)^2 / 2)
    per axis (d/dx = d/dd and d/dy = -d/dd on g(d) = exp(-p d^2 / 2), g^(k) = (-1)^k p^(k/2) He_k(sqrt(p) d) g).  Points are (t, x) rows;
    the blocks are d_t, d_x, d_x^3 on the domain points and delta on the domain and boundary points, N = 4 N_d + N_b.  With the nugget,
    the trace ratios and the rows of the extension (u, u_t, u_x, u_xx, u_xxx at test points).  tests/test_kdv_host.py checks the
    entries against central finite differences of the kernel.

2.  The float64 pipeline of the Gauss-Newton iteration: KdV is the Burgers system of tests/_gn_reference.py with nu = -delta, so a case
    in the shape of _gn_reference.Case (system 'burgers', p0 = alpha, p1 = -delta) goes through its linearise / Pipeline64 /
    VectorReference unchanged.

3.  The soliton u = (3 c / alpha) sech^2(sqrt(c / delta) (x - c t - x0) / 2) and a manufactured smooth solution with its forcing.
"""
import numpy as np
from numpy.polynomial import hermite_e as H

import _gn_reference as R

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
KERNELS = ('Gaussian', 'anisotropic_Gaussian')
NAMES = ('d_t', 'd_x', 'd_x^3', 'delta')
# multi-indices (order in t, order in x) of the four blocks, and of the row functionals of the extension in the bit order of
# gpk.device.FUNCTIONAL_DISP
BLOCKS = ((1, 0), (0, 1), (0, 3), (0, 0))
FUNCTIONALS = {'value': (0, 0), 'd1': (1, 0), 'd2': (0, 1), 'd2d2': (0, 2), 'd2d2d2': (0, 3)}


def precisions(kernel, kp, dtype=LD):
    """(p1, p2): 1 / sigma^2 on both axes (Gaussian), 2 / sigma_k^2 (anisotropic_Gaussian)"""
    s = np.atleast_1d(np.asarray(kp, dtype=np.float64)).astype(dtype)
    if kernel == 'Gaussian':
        return dtype(1) / (s[0] * s[0]), dtype(1) / (s[0] * s[0])
    if kernel == 'anisotropic_Gaussian':
        return dtype(2) / (s[0] * s[0]), dtype(2) / (s[1] * s[1])
    raise ValueError(f'unknown kernel {kernel!r}')


def _he(k, s):
    """He_k(s) through numpy.polynomial.hermite_e, in the dtype of s"""
    c = np.zeros(k + 1)
    c[k] = 1.0
    return H.hermeval(s, c)


class Pairs:
    """kappa and the Hermite values of every pair (x, y) of two broadcastable point sets, in `dtype`"""

    def __init__(self, kernel, kp, x1, x2, y1, y2, dtype=LD):
        self.p = precisions(kernel, kp, dtype)
        d1 = np.asarray(x1, dtype=np.float64).astype(dtype) - np.asarray(y1, dtype=np.float64).astype(dtype)
        d2 = np.asarray(x2, dtype=np.float64).astype(dtype) - np.asarray(y2, dtype=np.float64).astype(dtype)
        self.d = np.broadcast_arrays(d1, d2)
        self.s = [np.sqrt(self.p[k]) * self.d[k] for k in range(2)]
        self.kappa = np.exp(-(self.p[0] * self.d[0] ** 2 + self.p[1] * self.d[1] ** 2) / 2)

    def entry(self, m, n):
        """<d^m at x, d^n at y> kappa for the multi-indices m, n"""
        v = self.kappa
        for k in range(2):
            o = m[k] + n[k]
            if o:
                v = v * np.sqrt(self.p[k]) ** o * _he(o, self.s[k])
        return -v if (m[0] + m[1]) & 1 else v


def offsets(Nd, Nb):
    return [(0, Nd), (Nd, Nd), (2 * Nd, Nd), (3 * Nd, Nd + Nb)]


def _all_points(Xd, Xb):
    Xd = np.asarray(Xd, dtype=np.float64).reshape(-1, 2)
    Xb = np.asarray(Xb, dtype=np.float64).reshape(-1, 2)
    return Xd, Xb, np.concatenate([Xd, Xb])


def rows(kernel, kp, name, Xt, Xd, Xb, dtype=LD):
    """(Nt, N): the functional `name` of FUNCTIONALS at the points Xt against the column functionals of the layout"""
    Xt = np.asarray(Xt, dtype=np.float64).reshape(-1, 2)
    Xd, Xb, Xall = _all_points(Xd, Xb)
    P = Pairs(kernel, kp, Xt[:, None, 0], Xt[:, None, 1], Xall[None, :, 0], Xall[None, :, 1], dtype)
    m = FUNCTIONALS[name] if isinstance(name, str) else name
    return np.concatenate([P.entry(m, n)[:, :(Xall.shape[0] if n == (0, 0) else Xd.shape[0])] for n in BLOCKS], axis=1)


def theta(kernel, kp, Xd, Xb, dtype=LD):
    """Theta without nugget, (N, N)"""
    Xd, Xb, Xall = _all_points(Xd, Xb)
    Nd = Xd.shape[0]
    return np.concatenate([rows(kernel, kp, m, Xall if m == (0, 0) else Xd, Xd, Xb, dtype) for m in BLOCKS], axis=0)


def diagonal_values(kernel, kp):
    """<f, f> at coincident points for the four blocks: p1, p2, 15 p2^3, 1 -- from the Hermite values at 0, not from these formulas"""
    z = np.zeros(1)
    P = Pairs(kernel, kp, z, z, z, z)
    return [P.entry(m, m)[0] for m in BLOCKS]


def trace_ratios(kernel, kp, Nd, Nb):
    c = diagonal_values(kernel, kp)
    return [(LD(Nd) * c[k]) / (LD(Nd + Nb) * c[3]) for k in range(3)]


def block_nuggets(kernel, kp, Nd, Nb, nugget, nugget_type):
    if nugget_type == 'adaptive':
        return [LD(nugget) * r for r in trace_ratios(kernel, kp, Nd, Nb)] + [LD(nugget)]
    return [LD(nugget if nugget_type == 'identity' else 0.0)] * 4


def theta_nugget(kernel, kp, Xd, Xb, nugget, nugget_type='adaptive', base=None):
    Xd, Xb, _ = _all_points(Xd, Xb)
    Nd, Nb = Xd.shape[0], Xb.shape[0]
    T = (theta(kernel, kp, Xd, Xb) if base is None else base).copy()
    for (o, n), v in zip(offsets(Nd, Nb), block_nuggets(kernel, kp, Nd, Nb, nugget, nugget_type)):
        T[np.arange(o, o + n), np.arange(o, o + n)] += v
    return T


def finite_difference(kernel, kp, m, n, x, y, h):
    """d_x^m d_y^n kappa at the points x, y (each (2,)) by central differences of step h in long double: the k-th central difference
    sum_j (-1)^j C(k, j) f(. + (k/2 - j) h) / h^k on each of the four arguments, second-order accurate"""
    from math import comb
    p1, p2 = precisions(kernel, kp)

    def stencil(k):
        return [((-1) ** j * comb(k, j), (LD(k) / 2 - j) * LD(h)) for j in range(k + 1)]
    total = LD(0)
    for c0, o0 in stencil(m[0]):
        for c1, o1 in stencil(m[1]):
            for c2, o2 in stencil(n[0]):
                for c3, o3 in stencil(n[1]):
                    d1 = (LD(x[0]) + o0) - (LD(y[0]) + o2)
                    d2 = (LD(x[1]) + o1) - (LD(y[1]) + o3)
                    total += c0 * c1 * c2 * c3 * np.exp(-(p1 * d1 * d1 + p2 * d2 * d2) / 2)
    return total / LD(h) ** (sum(m) + sum(n))


# ------------------------------------------------------------------------------------------------ the Gauss-Newton pipeline
class Case:
    """A KdV problem in the shape of _gn_reference.Case: the Burgers system with p0 = alpha, p1 = nu = -delta and the factor L of the
    dispersive Theta in the one row group"""

    def __init__(self, Nd, Nb, f, g, alpha, delta, L, z0=None):
        self.system, self.Nd, self.Nb = 'burgers', Nd, Nb
        self.f, self.g = np.asarray(f, dtype=np.float64), np.asarray(g, dtype=np.float64)
        self.p0, self.p1, self.lam = float(alpha), -float(delta), 0.0
        self.data, self.Ndata, self.L2 = None, 0, None
        self.nz = 3 * Nd
        self.L = np.tril(np.asarray(L, dtype=np.float64))
        n = self.L.shape[0]
        assert n == 4 * Nd + Nb
        self.groups = [(0, n, self.L)]
        self.rows = n
        self.z0 = None if z0 is None else np.asarray(z0, dtype=np.float64)


def gn_float64(cs, z0, steps, step_size=1.0):
    """`steps` Gauss-Newton steps of the float64 pipeline (_gn_reference.Pipeline64): (final iterate, losses J(z_0) .. J(z_steps))"""
    z = np.array(z0, dtype=np.float64)
    hist = []
    for _ in range(steps):
        p = R.Pipeline64(cs, z)
        hist.append(p.loss)
        z = z - step_size * p.delta
    hist.append(R.Pipeline64(cs, z).loss)
    return z, hist


def sol_vec(cs, z):
    """[-delta v3 + f - alpha v0 v2; v2; v3; v0; g] at the iterate z, float64"""
    return R.linearise(cs, z).F.astype(np.float64)


# ------------------------------------------------------------------------------------------------ solutions
def soliton(alpha, delta, c, x0):
    """u(t, x) = (3 c / alpha) sech^2(sqrt(c / delta) (x - c t - x0) / 2): u_t + alpha u u_x + delta u_xxx = 0"""
    def u(t, x):
        return 3.0 * c / alpha / np.cosh(0.5 * np.sqrt(c / delta) * (x - c * t - x0)) ** 2
    return u


def soliton_residual(alpha, delta, c, x0, t, x):
    """the residual of the closed form from its closed-form derivatives, in long double: with k = sqrt(c / delta) / 2, xi = k (x - c t - x0),
    S = sech^2 xi, T = tanh xi and A = 3 c / alpha:  u = A S,  u_x = -2 k A S T,  u_t = -c u_x,  u_xxx = 8 k^3 A S T (3 S - 1)
    (from S' = -2 S T, T' = S, T^2 = 1 - S).  Returns (residual, the magnitude sum of its three terms)."""
    alpha, delta, c, x0 = LD(alpha), LD(delta), LD(c), LD(x0)
    t, x = np.asarray(t, dtype=np.float64).astype(LD), np.asarray(x, dtype=np.float64).astype(LD)
    k = np.sqrt(c / delta) / 2
    xi = k * (x - c * t - x0)
    S, T, A = 1 / np.cosh(xi) ** 2, np.tanh(xi), 3 * c / alpha
    u, ux = A * S, -2 * k * A * S * T
    ut, uxxx = -c * ux, 8 * k ** 3 * A * S * T * (3 * S - 1)
    terms = (ut, alpha * u * ux, delta * uxxx)
    return sum(terms), sum(np.abs(v) for v in terms)


ALPHA, DELTA = 1.0, 0.02                           # the manufactured problem of the class-level test


def smooth_truth(t, x):
    """u* = exp(-t) sin(pi x) on [0, 1] x [-1, 1]"""
    return np.exp(-t) * np.sin(np.pi * x)


def smooth_rhs(t, x):
    """f = u*_t + ALPHA u* u*_x + DELTA u*_xxx"""
    u = smooth_truth(t, x)
    ux = np.pi * np.exp(-t) * np.cos(np.pi * x)
    return -u + ALPHA * u * ux - DELTA * np.pi ** 2 * ux


def class_points(Nd, Nb, seed=7):
    """domain points uniform in (0, 1) x (-1, 1); boundary points on t = 0 and on x = -1, 1 (the parabolic boundary of the Burgers sampler)"""
    rng = np.random.RandomState(seed)
    Xd = np.column_stack([rng.uniform(0, 1, Nd), rng.uniform(-1, 1, Nd)])
    nb0 = Nb // 2
    side = Nb - nb0
    Xb = np.concatenate([np.column_stack([np.zeros(nb0), np.linspace(-1, 1, nb0)]),
                         np.column_stack([rng.uniform(0, 1, side), np.where(np.arange(side) % 2 == 0, -1.0, 1.0)])])
    return Xd, Xb
