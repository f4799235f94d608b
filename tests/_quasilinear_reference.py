"""Reference of the 2-jet Gram layout and of the Gauss-Newton system GPK_GN_QUASILINEAR (CPU only, numpy; long double where a bound is "to
rounding").  The Pairs / FUNC scheme of tests/_monge_ampere_reference.py with the two first-order functionals added.

Layout.  Blocks [d1; d2; D; M; L] on the N_d domain points (D = d_11 - d_22, M = 2 d_12, L = d_11 + d_22), delta on the N_d + N_b domain and
boundary points, N = 6 N_d + N_b.  An entry is <F at x, G at y> of kappa, term by term through Pairs.functional_pair (value and the
magnitude sum of tests/_monge_ampere_reference.py).

System (include/gpk.h): unknowns z = [v0 | v1 | v2 | v3 | v4] = [u | d_1 u | d_2 u | D u | M u],
    F(z) = [v1; v2; v3; v4; G(f; v); v0; g],   A(z) = dF/dz,   G of the three kinds GPK_QL_* with prm = (p0, p1, p2).
G, dG: the formulas of include/gpk.h, written here independently of src/quasilinear.py; G_mag, dG_mag: the magnitude sums of their
terms (every product and sum taken with absolute values; a quotient divides by the exact denominator, a root is its own scale).
"""
import functools
import zlib

import numpy as np

import _gauss_reference as GR
import _gn_reference as R
import _monge_ampere_reference as MA
import _semilinear_reference as SL
from _gn_reference import poisoned, synthetic_factor  # noqa: F401  (shared with the device tests)

LD, EPS = MA.LD, MA.EPS
KERNELS = GR.KERNELS
MARGIN = 32.0                 # the project's margin of a device step over the float64 numpy pipeline on the same inputs
GRAM_BOUND = MA.GRAM_BOUND
gram_allowed = MA.gram_allowed
NAMES = ('d1', 'd2', 'D', 'M', 'L', 'delta')
FUNC = dict(MA.FUNC, d1=((1, (1, 0)),), d2=((1, (0, 1)),))
MONOMIALS = MA.MONOMIALS
KINDS = {'mean_curvature': 0, 'p_laplace': 1, 'gauss_curvature': 2}
# one parameter set per kind for the device tests: every entry of A live where the kind has one
PRM = {'mean_curvature': (0.7, 0.0, 0.0), 'p_laplace': (3.0, 0.8, 0.0), 'gauss_curvature': (1.5, 0.0, 0.0)}
# Rounding budget of a computed entry of [A(z) | F(z)] in units of eps x the magnitude sum of its terms (the convention of
# _semilinear_reference.C_BUILD: each correctly rounded operation costs eps / 2 of a magnitude that is at most the sum; pow and sqrt of
# the device library are allowed 2 ulp and 1 ulp).  Longest chain, dG/dp of the p-Laplacian as ql_dG spells it: g2 (2), s (1), pow (4: the
# exponent a - 1 multiplies the relative error of s by |a - 1| <= 1, plus 2 ulp), k (3 products), k p, Qp (3), c Qp, -, G (chain of ~10
# on its own), 2 m p G (3), -, / E (E: 3): under 40 half-roundings.
C_BUILD = 20.0


def offsets(Nd, Nb):
    return [(k * Nd, Nd) for k in range(5)] + [(5 * Nd, Nd + Nb)]


def theta(kernel, kp, Xd, Xb):
    """(Theta without nugget, magnitude sums, exponent arguments), each (N, N) long double"""
    Xd = np.asarray(Xd, dtype=np.float64).reshape(-1, 2)
    Xb = np.asarray(Xb, dtype=np.float64).reshape(-1, 2)
    Nd, Nb = Xd.shape[0], Xb.shape[0]
    X = np.concatenate([Xd, Xb])
    P = MA.Pairs(kernel, kp, X[:, None, 0], X[:, None, 1], X[None, :, 0], X[None, :, 1])
    n = [Nd] * 5 + [Nd + Nb]
    parts = [[P.functional_pair(FUNC[f], FUNC[g]) for g in NAMES] for f in NAMES]
    T = np.block([[parts[i][j][0][:n[i], :n[j]] for j in range(6)] for i in range(6)])
    Mg = np.block([[parts[i][j][1][:n[i], :n[j]] for j in range(6)] for i in range(6)])
    Ag = np.block([[P.arg[:n[i], :n[j]] for j in range(6)] for i in range(6)])
    # the blocks 2..5 ARE the Hessian layout: its closed forms and their (in <D,L> smaller: a4 - b4 has no a2 b2 terms) magnitude sums
    Th, Mh, _ = MA.theta(kernel, kp, Xd, Xb)
    T[2 * Nd:, 2 * Nd:], Mg[2 * Nd:, 2 * Nd:] = Th, Mh
    return T, Mg, Ag


def diagonal_values(kernel, kp):
    """<F, F> at d = 0 for d1, d2, D, M, L, delta by the closed forms of include/gpk.h, long double"""
    p1, p2 = GR.precisions(kernel, kp)
    return [p1, p2] + MA.diagonal_values(kernel, kp)


def trace_ratios(kernel, kp, Nd, Nb):
    """trace(block k) / trace(block 5), k = 0..4"""
    c = diagonal_values(kernel, kp)
    return [(Nd * c[k]) / (LD(Nd + Nb)) for k in range(5)]


def block_nuggets(kernel, kp, Nd, Nb, nugget, nugget_type):
    if nugget_type == 'adaptive':
        return [LD(nugget) * r for r in trace_ratios(kernel, kp, Nd, Nb)] + [LD(nugget)]
    return [LD(nugget if nugget_type == 'identity' else 0.0)] * 6


def theta_nugget(kernel, kp, Xd, Xb, nugget, nugget_type='adaptive', base=None):
    Nd, Nb = np.asarray(Xd).reshape(-1, 2).shape[0], np.asarray(Xb).reshape(-1, 2).shape[0]
    T = (theta(kernel, kp, Xd, Xb)[0] if base is None else base).copy()
    for (o, n), v in zip(offsets(Nd, Nb), block_nuggets(kernel, kp, Nd, Nb, nugget, nugget_type)):
        T[np.arange(o, o + n), np.arange(o, o + n)] += v
    return T


def monomial_rows(kernel, kp, name, Xt, Xd, Xb):
    """(rows, magnitude sums, exponent arguments), each (Nt, N) long double: the monomial derivative `name` (MONOMIALS) at the points Xt
    against the column functionals of the layout"""
    Xt = np.asarray(Xt, dtype=np.float64).reshape(-1, 2)
    Xd = np.asarray(Xd, dtype=np.float64).reshape(-1, 2)
    Xb = np.asarray(Xb, dtype=np.float64).reshape(-1, 2)
    X = np.concatenate([Xd, Xb])
    P = MA.Pairs(kernel, kp, Xt[:, None, 0], Xt[:, None, 1], X[None, :, 0], X[None, :, 1])
    fx = ((1, MONOMIALS[name]),)
    Nd = Xd.shape[0]
    n = [Nd] * 5 + [X.shape[0]]
    parts = [P.functional_pair(fx, FUNC[g]) for g in NAMES]
    return (np.concatenate([v[:, :k] for (v, _), k in zip(parts, n)], axis=1), np.concatenate([m[:, :k] for (_, m), k in zip(parts, n)], axis=1),
            np.concatenate([P.arg[:, :k] for k in n], axis=1))


# ------------------------------------------------------------------------------------------------ the three equations
def _Q(p, q, D, M):
    return D * (p * p - q * q) + 2 * p * q * M


def G(kind, prm, f, v0, p, q, D, M):
    g2 = p * p + q * q
    if kind == 'gauss_curvature':
        return np.sqrt(D * D + M * M + 4 * f * (1 + g2) ** prm[0])
    if kind == 'p_laplace':
        m, dd = prm[0], prm[1] * prm[1]
        return (2 * f * (dd + g2) ** ((4 - m) / 2) - (m - 2) * _Q(p, q, D, M)) / (2 * dd + m * g2)
    W2 = 1 + g2
    return (2 * W2 * np.sqrt(W2) * (f + prm[0] * v0) + _Q(p, q, D, M)) / (1 + W2)


def G_mag(kind, prm, f, v0, p, q, D, M):
    f, v0, p, q, D, M = (np.abs(t) for t in (f, v0, p, q, D, M))
    g2 = p * p + q * q
    Qm = D * g2 + 2 * p * q * M
    if kind == 'gauss_curvature':
        return np.sqrt(D * D + M * M + 4 * f * (1 + g2) ** prm[0])
    if kind == 'p_laplace':
        m, dd = prm[0], prm[1] * prm[1]
        return (2 * f * (dd + g2) ** ((4 - m) / 2) + abs(m - 2) * Qm) / (2 * dd + m * g2)
    W2 = 1 + g2
    return (2 * W2 * np.sqrt(W2) * (f + abs(prm[0]) * v0) + Qm) / (1 + W2)


def dG(kind, prm, f, v0, p, q, D, M):
    """(dG/dv0, dG/dp, dG/dq, dG/dD, dG/dM)"""
    g2 = p * p + q * q
    zero = 0 * g2
    if kind == 'gauss_curvature':
        e, W2 = prm[0], 1 + g2
        s = G(kind, prm, f, v0, p, q, D, M)
        c = 4 * f * e * W2 ** (e - 1)
        return zero, c * p / s, c * q / s, D / s, M / s
    Qp, Qq = 2 * (p * D + q * M), 2 * (p * M - q * D)
    Gv = G(kind, prm, f, v0, p, q, D, M)
    if kind == 'p_laplace':
        m, dd = prm[0], prm[1] * prm[1]
        s, a, c = dd + g2, (4 - m) / 2, m - 2
        E = 2 * dd + m * g2
        k = 4 * f * a * s ** (a - 1)
        return zero, (k * p - c * Qp - 2 * m * p * Gv) / E, (k * q - c * Qq - 2 * m * q * Gv) / E, -c * (p * p - q * q) / E, -c * 2 * p * q / E
    W2 = 1 + g2
    W, r, E = np.sqrt(W2), f + prm[0] * v0, 1 + W2
    return 2 * W2 * W * prm[0] / E + zero, (6 * W * p * r + Qp - 2 * p * Gv) / E, (6 * W * q * r + Qq - 2 * q * Gv) / E, (p * p - q * q) / E, 2 * p * q / E


def dG_mag(kind, prm, f, v0, p, q, D, M):
    Gm = G_mag(kind, prm, f, v0, p, q, D, M)
    f, v0, p, q, D, M = (np.abs(t) for t in (f, v0, p, q, D, M))
    g2 = p * p + q * q
    zero = 0 * g2
    if kind == 'gauss_curvature':
        e, W2 = prm[0], 1 + g2
        c = 4 * f * abs(e) * W2 ** (e - 1)
        return zero, c * p / Gm, c * q / Gm, D / Gm, M / Gm
    Qp, Qq = 2 * (p * D + q * M), 2 * (p * M + q * D)
    if kind == 'p_laplace':
        m, dd = prm[0], prm[1] * prm[1]
        s, a, c = dd + g2, (4 - m) / 2, abs(m - 2)
        E = 2 * dd + m * g2
        k = 4 * f * abs(a) * s ** (a - 1)
        return zero, (k * p + c * Qp + 2 * m * p * Gm) / E, (k * q + c * Qq + 2 * m * q * Gm) / E, c * g2 / E, c * 2 * p * q / E
    W2 = 1 + g2
    W, r, E = np.sqrt(W2), f + abs(prm[0]) * v0, 1 + W2
    return 2 * W2 * W * abs(prm[0]) / E + zero, (6 * W * p * r + Qp + 2 * p * Gm) / E, (6 * W * q * r + Qq + 2 * q * Gm) / E, g2 / E, 2 * p * q / E


def divergence_form(kind, prm, f, u, u1, u2, u11, u12, u22):
    """the residual of the equation in its divergence / determinant form (gpk_pde_residual_ql) and the magnitude sum of its terms"""
    g2 = u1 * u1 + u2 * u2
    T = u1 * u1 * u11 + 2 * u1 * u2 * u12 + u2 * u2 * u22
    Tm = u1 * u1 * np.abs(u11) + 2 * np.abs(u1 * u2 * u12) + u2 * u2 * np.abs(u22)
    lap, lapm = u11 + u22, np.abs(u11) + np.abs(u22)
    if kind == 'gauss_curvature':
        w = f * (1 + g2) ** prm[0]
        return (u11 * u22 - u12 * u12) - w, np.abs(u11 * u22) + u12 * u12 + np.abs(w)
    if kind == 'p_laplace':
        m, s = prm[0], prm[1] * prm[1] + g2
        k = s ** ((m - 4) / 2)
        return k * (s * lap + (m - 2) * T) - f, k * (s * lapm + abs(m - 2) * Tm) + np.abs(f)
    W2 = 1 + g2
    W3 = W2 * np.sqrt(W2)
    return (W2 * lap - T) / W3 - (f + prm[0] * u), (W2 * lapm + Tm) / W3 + np.abs(f) + np.abs(prm[0] * u)


# ------------------------------------------------------------------------------------------------ F(z), A(z), one step
def split(z, Nd):
    return tuple(z[k * Nd:(k + 1) * Nd] for k in range(5))


class Case:
    """inputs of one (kind, N_d, N_b): parameters, right-hand sides, a synthetic well-conditioned factor, start point; f > 0, so the
    radicand of the Gauss-curvature kind is positive.  groups, nz, rows: what _gn_reference's Pipeline64 and solvers read"""
    system = 'quasilinear'

    def __init__(self, kind, Nd, Nb, prm=None, z0=None):
        self.kind, self.Nd, self.Nb = kind, Nd, Nb
        self.prm = tuple(float(v) for v in (PRM[kind] if prm is None else prm))
        self.nz, n = 5 * Nd, 6 * Nd + Nb
        rng = np.random.RandomState(zlib.crc32(repr(('quasilinear', Nd, Nb)).encode()))
        self.f = rng.uniform(0.5, 1.5, Nd)
        self.g = rng.uniform(0.5, 1.5, Nb)
        z = rng.uniform(0.3, 1.2, self.nz) * rng.choice([-1.0, 1.0], self.nz)
        self.z0 = z if z0 is None else np.asarray(z0, dtype=np.float64)
        self.L = synthetic_factor(rng, n)
        self.groups = [(0, n, self.L)]
        self.rows = n


@functools.lru_cache(maxsize=None)
def case(kind, Nd, Nb):
    return Case(kind, Nd, Nb)


def linearise(cs, z):
    """[A(z) | F(z)] at the float64 point z with long-double entries (SL.Lin: values and magnitude sums).  The v0 entry of the PDE row
    is part of the pattern for every kind, also where it is 0."""
    Nd = cs.Nd
    z = np.asarray(z, dtype=np.float64).astype(LD)
    f, g = cs.f.astype(LD), cs.g.astype(LD)
    prm, one = tuple(LD(v) for v in cs.prm), LD(1)
    v = split(z, Nd)
    lin = SL.Lin(cs.rows, cs.nz)
    for k in range(4):
        lin.put_f(k * Nd, v[k + 1])
    lin.put_f(4 * Nd, G(cs.kind, prm, f, *v), G_mag(cs.kind, prm, f, *v))
    lin.put_f(5 * Nd, v[0]); lin.put_f(6 * Nd, g)
    d, m = dG(cs.kind, prm, f, *v), dG_mag(cs.kind, prm, f, *v)
    for k in range(4):
        lin.put_a(k * Nd, (k + 1) * Nd, one, Nd, True)
    for k in range(5):
        exact_zero = k == 0 and cs.kind != 'mean_curvature'
        lin.put_a(4 * Nd, k * Nd, d[k], Nd, exact_zero, mag=None if exact_zero else m[k])
    lin.put_a(5 * Nd, 0, one, Nd, True)
    return lin.finish()


class FullReference(SL.FullReference):
    """SL.FullReference (one step in long double, rounding scales, the float64 pipeline) on this system's linearisation"""

    def __init__(self, cs, z):
        self.case, self.z = cs, np.array(z, dtype=np.float64)
        lin = self.lin = linearise(cs, z)
        nz = cs.nz
        Sb = R._group_solve(cs, np.concatenate([lin.dense(), lin.F[:, None]], axis=1))
        self.S, self.w = Sb[:, :nz], Sb[:, nz]
        Gm = R.gram_lower(Sb)
        self.H, self.g, self.loss = LD(2) * Gm[:nz, :nz], LD(2) * Gm[nz, :nz], self.w @ self.w
        Sa = np.abs(Sb).astype(np.float64)
        self.scaleH = 2.0 * (Sa[:, :nz].T @ Sa[:, :nz])
        self.scaleg = 2.0 * (Sa[:, :nz].T @ Sa[:, nz])
        self.p64 = R.Pipeline64(cs, z, lin)
        self.delta = R.refine(self.p64.solve, lambda d: self.g - self.H @ d, self.g.astype(np.float64))
        ev = np.linalg.eigvalsh(self.H.astype(np.float64))
        self.normH, self.cond = float(ev[-1]), float(ev[-1] / ev[0])


@functools.lru_cache(maxsize=None)
def full_reference(kind, Nd, Nb):
    cs = case(kind, Nd, Nb)
    return FullReference(cs, cs.z0)


def gates(ref, **kw):
    """SL.gates with this project's MARGIN = 32 in place of SL.MARGIN: {quantity: (device error, allowed)}"""
    return {k: (r, a * (MARGIN / SL.MARGIN)) for k, (r, a) in SL.gates(ref, **kw).items()}


def check_build(lin, A, F, what=''):
    """SL.check_build under this module's C_BUILD"""
    old = SL.C_BUILD
    SL.C_BUILD = C_BUILD
    try:
        return SL.check_build(lin, A, F, what)
    finally:
        SL.C_BUILD = old


def stair_pos(Nd):
    """position of unknown j in the leading-zero layout of gpk_gn_step: groups in the order v1, v2, v3, v4, v0"""
    j = np.arange(5 * Nd)
    return ((j // Nd + 4) % 5) * Nd + j % Nd


def stair_col(Nd):
    """its storage column: the positions reversed"""
    return 5 * Nd - 1 - stair_pos(Nd)


# ------------------------------------------------------------------------------------------------ float64 Gauss-Newton on a Gram factor
class System:
    """F and A of the system as the numpy oracle's gn_method takes them"""

    def __init__(self, kind, prm, rhs_f, bdy_g):
        self.kind, self.prm = kind, tuple(float(v) for v in prm)
        self.f, self.g = np.asarray(rhs_f, dtype=np.float64), np.asarray(bdy_g, dtype=np.float64)
        self.Nd, self.Nb = self.f.size, self.g.size
        self.nz = 5 * self.Nd

    def F(self, z):
        v = split(z, self.Nd)
        return [np.concatenate([v[1], v[2], v[3], v[4], G(self.kind, self.prm, self.f, *v), v[0], self.g])]

    def A(self, z):
        Nd = self.Nd
        d = dG(self.kind, self.prm, self.f, *split(z, Nd))
        A = np.zeros((6 * Nd + self.Nb, 5 * Nd))
        i = np.arange(Nd)
        for k in range(4):
            A[k * Nd + i, (k + 1) * Nd + i] = 1.0
        for k in range(5):
            A[4 * Nd + i, k * Nd + i] = d[k]
        A[5 * Nd + i, i] = 1.0
        return [A]

    def extra(self, z):
        return 0.0, None, None

    def sol_vec(self, z):
        return self.F(z)


gn_float64 = SL.gn_float64
posterior_prepare = SL.posterior_prepare
log_evidence = SL.log_evidence
points = SL.points


def gn_long_double(sysm, L, z0, steps):
    """the float64 pipeline's long-double twin: the same Gauss-Newton iteration with F, A, the solves and the normal equations in long
    double (the factor L is the float64 one, as given); H is solved in float64 and refined twice in long double"""
    Ll = np.asarray(L, dtype=np.float64).astype(LD)
    z = np.asarray(z0, dtype=np.float64).astype(LD)
    for _ in range(steps):
        A, Fv = sysm.A(z)[0].astype(LD), sysm.F(z)[0].astype(LD)
        d = dG(sysm.kind, tuple(LD(v) for v in sysm.prm), sysm.f.astype(LD), *split(z, sysm.Nd))
        i = np.arange(sysm.Nd)
        for k in range(5):
            A[4 * sysm.Nd + i, k * sysm.Nd + i] = d[k]
        Fv[4 * sysm.Nd:5 * sysm.Nd] = G(sysm.kind, tuple(LD(v) for v in sysm.prm), sysm.f.astype(LD), *split(z, sysm.Nd))
        Sb = R.solve_lower(Ll, np.concatenate([A, Fv[:, None]], axis=1))
        S, w = Sb[:, :-1], Sb[:, -1]
        H, g = S.T @ S, S.T @ w
        H64 = H.astype(np.float64)
        delta = np.linalg.solve(H64, g.astype(np.float64)).astype(LD)
        for _ in range(2):
            delta = delta + np.linalg.solve(H64, (g - H @ delta).astype(np.float64)).astype(LD)
        z = z - delta
    return z


def numpy_pipeline(kernel, kp, Xd, Xb, nugget, kind, prm, f, g, z0, steps):
    """(z, loss history, L, system): Theta (long double, rounded) + adaptive nugget, LAPACK Cholesky, float64 Gauss-Newton"""
    T = theta_nugget(kernel, kp, Xd, Xb, nugget).astype(np.float64)
    L = np.linalg.cholesky(T)
    sysm = System(kind, prm, f, g)
    z, hist = gn_float64(sysm, L, np.array(z0, dtype=np.float64), steps)
    return z, hist, L, sysm
