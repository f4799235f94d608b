"""Reference of the evolution Gram layout (general spatial operator Q = c2 d_x^2 + c3 d_x^3 + c4 d_x^4 + c5 d_x^5, boundary functionals
c0 delta + c1 d_t + c2 d_x) and of the Gauss-Newton iteration on it (CPU only).

1.  The Gram entries of gpk_assemble_evo in long double, built on tests/_kdv_reference.py: every entry is a sum of
        <d^m at x, d^n at y> kappa = (-1)^|m| p1^((m1+n1)/2) p2^((m2+n2)/2) He_(m1+n1)(s1) He_(m2+n2)(s2) kappa
    over the multi-indices of the two functionals, with the probabilists' Hermite polynomials of numpy.polynomial.hermite_e -- no even /
    odd parts, no combined coefficients, none of the groupings of csrc/gpk_assemble_evo.hip.  Points are (t, x) rows; the blocks are
    d_t, d_x, Q on the domain points and delta (domain points) / B_b (boundary points) in block 3, N = 4 N_d + N_b.  With the nugget, the
    trace ratios and the rows of the extension (u, u_t, u_x, u_xx, Q[u] at test points).
    The float64 twin is the same code with dtype = numpy.float64: its error against the long-double values is the yardstick of the
    device tests (allowance 8 x that error).

2.  The float64 pipeline of the Gauss-Newton iteration: the Burgers system of tests/_gn_reference.py with nu = -1 (_kdv_reference.Case with
    delta = 1), and the numpy pipeline of the class: the doubling of the wall points under 'clamped', the data vector, the iteration.

3.  A manufactured smooth solution with its forcing for any (alpha, c2..c5).
"""
import numpy as np

import _kdv_reference as K

LD, EPS, KERNELS = K.LD, K.EPS, K.KERNELS
NAMES = ('d_t', 'd_x', 'Q', 'B')
FUNCTIONAL_NAMES = ('value', 'd1', 'd2', 'd2d2', 'q')          # the bit order of gpk.device.FUNCTIONAL_EVO

KS = (1.0, 0.0, 1.0, 0.0)                                     # Kuramoto-Sivashinsky
KAWAHARA = (0.0, 1.0, 0.0, -0.5)                              # Kawahara: u_t + alpha u u_x + a u_xxx + b u_xxxxx, (a, b) = (1, -1/2)
FULL = (-0.3, 0.7, 0.45, -0.2)                                # a Benney-Lin set with all four coefficients


def equation_coeffs(equation):
    """(c2, c3, c4, c5) of the shorthands of Evolution1d"""
    name, args = equation[0], tuple(float(v) for v in equation[1:])
    if name == 'kuramoto_sivashinsky' and not args:
        return 1.0, 0.0, 1.0, 0.0
    if name == 'kawahara' and len(args) == 2:
        return 0.0, args[0], 0.0, args[1]
    if name == 'kdv_burgers' and len(args) == 2:
        return -args[0], args[1], 0.0, 0.0
    if name == 'benney_lin' and len(args) == 4:
        return args
    raise ValueError(equation)


def terms(name, c):
    """the functional `name` as a list of (coefficient, multi-index)"""
    if name == 'q':
        return [(c[k - 2], (0, k)) for k in (2, 3, 4, 5) if c[k - 2] != 0.0]
    return [(1.0, {'value': (0, 0), 'd1': (1, 0), 'd2': (0, 1), 'd2d2': (0, 2)}[name])]


def _points(Xd, Xb):
    return K._all_points(Xd, Xb)


def weights(Nd, Nb, bc):
    """(Nd + Nb, 3): (1, 0, 0) at the domain points, row b of bc at boundary point b (None: delta)"""
    W = np.zeros((Nd + Nb, 3))
    W[:, 0] = 1.0
    if bc is not None and Nb:
        W[Nd:] = np.asarray(bc, dtype=np.float64).reshape(Nb, 3)
    return W


def _columns(P, m, c, Nd, W, dtype):
    """(Nt, N): the monomial functional d^m at the row points against the column functionals of the layout"""
    blocks = [P.entry(m, (1, 0))[:, :Nd], P.entry(m, (0, 1))[:, :Nd]]
    q = 0
    for ck, n in terms('q', c):
        q = q + dtype(ck) * P.entry(m, n)[:, :Nd]
    blocks.append(q)
    Wd = W.astype(dtype)
    blocks.append(Wd[None, :, 0] * P.entry(m, (0, 0)) + Wd[None, :, 1] * P.entry(m, (1, 0)) + Wd[None, :, 2] * P.entry(m, (0, 1)))
    return np.concatenate(blocks, axis=1)


def rows(kernel, kp, c, name, Xt, Xd, Xb, bc=None, dtype=LD, row_weights=None):
    """(Nt, N): the functional `name` of FUNCTIONAL_NAMES at the points Xt against the column functionals of the layout;
    name = 'b': the functional v0 delta + v1 d_t + v2 d_x with row_weights[t] = (v0, v1, v2) at test point t"""
    Xt = np.asarray(Xt, dtype=np.float64).reshape(-1, 2)
    Xd, Xb, Xall = _points(Xd, Xb)
    Nd, Nb = Xd.shape[0], Xb.shape[0]
    W = weights(Nd, Nb, bc)
    P = K.Pairs(kernel, kp, Xt[:, None, 0], Xt[:, None, 1], Xall[None, :, 0], Xall[None, :, 1], dtype)
    if name == 'b':
        V = np.asarray(row_weights, dtype=np.float64).astype(dtype)
        return sum(V[:, j, None] * _columns(P, m, c, Nd, W, dtype) for j, m in enumerate(((0, 0), (1, 0), (0, 1))))
    out = 0
    for ck, m in terms(name, c):
        out = out + dtype(ck) * _columns(P, m, c, Nd, W, dtype)
    return out


def offsets(Nd, Nb):
    return K.offsets(Nd, Nb)


def theta(kernel, kp, c, Xd, Xb, bc=None, dtype=LD):
    """Theta without nugget, (N, N)"""
    Xd, Xb, Xall = _points(Xd, Xb)
    Nd, Nb = Xd.shape[0], Xb.shape[0]
    top = [rows(kernel, kp, c, n, Xd, Xd, Xb, bc, dtype) for n in ('d1', 'd2', 'q')]
    return np.concatenate(top + [rows(kernel, kp, c, 'b', Xall, Xd, Xb, bc, dtype, row_weights=weights(Nd, Nb, bc))], axis=0)


def qq_at_zero(p2, c):
    """<Q,Q> at coincident points, the closed form"""
    c2, c3, c4, c5 = (LD(v) for v in c)
    p = LD(p2)
    return (3 * c2 ** 2 * p ** 2 + 15 * c3 ** 2 * p ** 3 + 105 * c4 ** 2 * p ** 4 + 945 * c5 ** 2 * p ** 5
            - 30 * c2 * c4 * p ** 3 - 210 * c3 * c5 * p ** 4)


def diagonal_values(kernel, kp, c):
    """<f, f> at coincident points for T, X, Q, delta -- from the Hermite values at 0, not from the closed form"""
    z = np.zeros((1, 2))
    T = theta(kernel, kp, c, z, np.zeros((0, 2)))
    return [T[k, k] for k in range(4)]


def boundary_trace(kernel, kp, Nb, bc):
    p1, p2 = K.precisions(kernel, kp)
    if bc is None:
        return LD(Nb)
    b = np.asarray(bc, dtype=np.float64).reshape(Nb, 3).astype(LD)
    return np.sum(b[:, 0] ** 2 + p1 * b[:, 1] ** 2 + p2 * b[:, 2] ** 2)


def trace_ratios(kernel, kp, c, Nd, Nb, bc=None):
    d = diagonal_values(kernel, kp, c)
    return [(LD(Nd) * d[k]) / (LD(Nd) + boundary_trace(kernel, kp, Nb, bc)) for k in range(3)]


def block_nuggets(kernel, kp, c, Nd, Nb, nugget, nugget_type, bc=None):
    if nugget_type == 'adaptive':
        return [LD(nugget) * r for r in trace_ratios(kernel, kp, c, Nd, Nb, bc)] + [LD(nugget)]
    return [LD(nugget if nugget_type == 'identity' else 0.0)] * 4


def theta_nugget(kernel, kp, c, Xd, Xb, nugget, nugget_type='adaptive', bc=None, base=None):
    Xd, Xb, _ = _points(Xd, Xb)
    Nd, Nb = Xd.shape[0], Xb.shape[0]
    T = (theta(kernel, kp, c, Xd, Xb, bc) if base is None else base).copy()
    for (o, n), v in zip(offsets(Nd, Nb), block_nuggets(kernel, kp, c, Nd, Nb, nugget, nugget_type, bc)):
        T[np.arange(o, o + n), np.arange(o, o + n)] += v
    return T


def block_errors(got, ref, twin, Nd, Nb):
    """per block (i, j): (error of `got`, error of the float64 twin), both against the long-double `ref` and relative to max|block|;
    blocks that are identically zero are left out"""
    out = {}
    for i, (ro, rn) in enumerate(offsets(Nd, Nb)):
        for j, (co, cn) in enumerate(offsets(Nd, Nb)):
            r = ref[ro:ro + rn, co:co + cn]
            scale = float(np.max(np.abs(r))) if r.size else 0.0
            if scale > 0:
                out[i, j] = tuple(float(np.max(np.abs(a[ro:ro + rn, co:co + cn].astype(LD) - r))) / scale for a in (got, twin))
    return out


# The allowance of the device tests: 8 x the error of the float64 twin on the same inputs, the margin the dispersive layout was given.
# The twin's error is taken as at least eps / 2: a float64 value cannot be expected closer than half a unit of the last place to the
# long-double one, and a twin that is nearer than that (a block of one entry whose value happens to be a float64 number) is so by accident.
MARGIN = 8.0


def allowance(e_twin):
    return MARGIN * max(float(e_twin), 0.5 * EPS)


# ------------------------------------------------------------------------------------------------ the Gauss-Newton pipeline
def Case(Nd, Nb, f, g, alpha, L, z0=None):
    """the Burgers system with p0 = alpha, p1 = nu = -1: F = [-v3 + f - alpha v0 v2; v2; v3; v0; g] with v3 = Q[u]"""
    return K.Case(Nd, Nb, f, g, alpha, 1.0, L, z0)


gn_float64 = K.gn_float64
sol_vec = K.sol_vec


def clamped_boundary(Xb, domain):
    """the boundary points and rows of Evolution1d(bc='clamped'): every point with x at either end of the domain once more behind the
    given points, the first copy with the row (1, 0, 0), the second with (0, 0, 1).  -> (points, rows, index of the wall points)"""
    Xb = np.asarray(Xb, dtype=np.float64).reshape(-1, 2)
    wall = np.flatnonzero((Xb[:, 1] == float(domain[1][0])) | (Xb[:, 1] == float(domain[1][1])))
    bc = np.zeros((Xb.shape[0] + wall.size, 3))
    bc[:Xb.shape[0], 0] = 1.0
    bc[Xb.shape[0]:, 2] = 1.0
    return np.concatenate([Xb, Xb[wall]]), bc, wall


# ------------------------------------------------------------------------------------------------ a manufactured solution
DOMAIN = np.array([[0.0, 1.0], [-1.0, 1.0]])


def smooth_truth(t, x):
    """u* = exp(-t) sin(pi x) on [0, 1] x [-1, 1]"""
    return np.exp(-t) * np.sin(np.pi * x)


def smooth_truth_x(t, x):
    return np.pi * np.exp(-t) * np.cos(np.pi * x)


def smooth_q(c):
    """Q[u*]: u*_xx = -pi^2 u*, u*_xxx = -pi^2 u*_x, u*_xxxx = pi^4 u*, u*_xxxxx = pi^4 u*_x"""
    c2, c3, c4, c5 = c

    def q(t, x):
        u, ux = smooth_truth(t, x), smooth_truth_x(t, x)
        return (-c2 * np.pi ** 2 + c4 * np.pi ** 4) * u + (-c3 * np.pi ** 2 + c5 * np.pi ** 4) * ux
    return q


def smooth_rhs(alpha, c):
    """f = u*_t + alpha u* u*_x + Q[u*]"""
    q = smooth_q(c)

    def f(t, x):
        u = smooth_truth(t, x)
        return -u + alpha * u * smooth_truth_x(t, x) + q(t, x)
    return f


class_points = K.class_points
