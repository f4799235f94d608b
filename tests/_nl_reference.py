"""Long-double reference for the reaction terms tau(u) of the elliptic systems (gpk.h, GPK_NL_*; csrc/gpk_common.h nl_tau / nl_dtau;
src/nonlinearity.py) -- CPU only.  Built on tests/_gn_reference.py: the same synthetic factors, the same row layout, the same gates.

  tau_ld / dtau_ld      tau, tau' and the magnitude sum of their terms in long double
  NLCase                inputs of one (kind, system, N_d, N_b): the construction of _gn_reference.Case with z drawn from (-1.2, 1.2)
  linearise             [A(z) | F(z)] with long-double entries and a magnitude per entry (the cubic's tau' has three terms)
  check_build           the rule of _gn_reference.check_build with a budget per kind and a magnitude per entry of A
  FullReference / VectorReference   those of _gn_reference.py on this linearisation
  cpu_chain             the whole solve in float64: numpy.linalg.cholesky of a given Theta, then the Gauss-Newton loop

Rounding budget of one entry of [A(z) | F(z)] in units of eps x (magnitude sum of its terms), by the counting rule of _gn_reference.py
(eps / 2 per + - * / or fused multiply-add; rs = 1 / sqrt(lambda) costs 3/2):

  exp, sinh, sin   elliptic  A: (p0 p1) fn'(p1 u): 2/2 + U';            F: p0 fn(p1 u) - f: 1/2 + U + 1/2
                   relaxed   A: ... rs: 2/2 + U' + 3/2 + 1/2 = 3 + U';  F: (-v + p0 fn(p1 u) - f) rs: (1/2 + U) + 2/2 + 3/2 + 1/2 = 7/2 + U
  cubic            tau = u (p0 + u (p1 + p2 u)): five operations, each at most eps / 2 of sum |c_k u^k| (Horner) = 5/2; tau' = p0 + u (2 p1 +
                   3 p2 u): five = 5/2;  elliptic F: 3;  relaxed A: 5/2 + 3/2 + 1/2 = 9/2;  F: 5/2 + 2/2 + 3/2 + 1/2 = 11/2

p1 u is exact in every test (p1 is a power of two), so the argument of fn carries no rounding of its own.  U, U' = the error of the
device's exp / sinh / cosh / sin / cos relative to the value, in eps.  The ROCm installation ships no table of the accuracy of the double-precision
device math functions (its documentation directory has none), so the figures are MEASURED: each function alone on an MI355X
against long double at 262144 arguments in (-2.4, 2.4) -- the range of p1 u of these tests -- (DEVICE_FN_ERR below; DESIGN.md section K,
"Reaction terms"), and the budget allows TWICE the observed maximum.
"""
import functools
import zlib

import numpy as np

import _gn_reference as R

LD, EPS = R.LD, R.EPS
KINDS = ('exp', 'sinh', 'sin', 'cubic')
KIND_ID = {'power': 0, 'exp': 1, 'sinh': 2, 'sin': 3, 'cubic': 4}
# (p0, p1, p2): p1 a power of two for the transcendental kinds (p1 u exact); the cubic -1.1 u + 0.3 u^2 + 0.8 u^3 changes sign on (-1.2, 1.2)
# and so does its derivative
PARAMS = {'exp': (-0.7, 1.0, 0.0), 'sinh': (1.3, 0.5, 0.0), 'sin': (0.9, 2.0, 0.0), 'cubic': (-1.1, 0.3, 0.8)}
SIZES = ((37, 12), (300, 68))
# max |device - long double| / (eps |value|) observed on an MI355X (gfx950, ROCm device library), 262144 arguments in (-2.4, 2.4)
DEVICE_FN_ERR = {'exp': 0.604, 'sinh': 0.661, 'cosh': 0.513, 'sin': 0.568, 'cos': 0.570}
_FN = {'exp': ('exp', 'exp'), 'sinh': ('sinh', 'cosh'), 'sin': ('sin', 'cos')}          # kind -> (function of tau, of tau')


def build_budget(kind):
    """the largest entry of either system, in eps x magnitude sum: the relaxed system's F"""
    if kind == 'cubic':
        return 5.5
    f, df = _FN[kind]
    return max(3.5 + 2.0 * DEVICE_FN_ERR[f], 3.0 + 2.0 * DEVICE_FN_ERR[df])


def tau_ld(kind, params, u):
    """(tau(u), sum of the magnitudes of its terms) in long double"""
    p0, p1, p2 = (LD(p) for p in params)
    u = np.asarray(u, dtype=np.float64).astype(LD)
    if kind == 'power':
        v = p0 * u ** p1
    elif kind == 'exp':
        v = p0 * np.exp(p1 * u)
    elif kind == 'sinh':
        v = p0 * np.sinh(p1 * u)
    elif kind == 'sin':
        v = p0 * np.sin(p1 * u)
    elif kind == 'cubic':
        return p0 * u + p1 * u * u + p2 * u * u * u, np.abs(p0 * u) + np.abs(p1 * u * u) + np.abs(p2 * u * u * u)
    else:
        raise ValueError(kind)
    return v, np.abs(v)


def dtau_ld(kind, params, u):
    """(tau'(u), sum of the magnitudes of its terms) in long double"""
    p0, p1, p2 = (LD(p) for p in params)
    u = np.asarray(u, dtype=np.float64).astype(LD)
    if kind == 'power':
        v = p0 * p1 * u ** (p1 - LD(1))
    elif kind == 'exp':
        v = p0 * p1 * np.exp(p1 * u)
    elif kind == 'sinh':
        v = p0 * p1 * np.cosh(p1 * u)
    elif kind == 'sin':
        v = p0 * p1 * np.cos(p1 * u)
    elif kind == 'cubic':
        return (p0 + LD(2) * p1 * u + LD(3) * p2 * u * u,
                np.abs(p0) + np.abs(LD(2) * p1 * u) + np.abs(LD(3) * p2 * u * u))
    else:
        raise ValueError(kind)
    return v, np.abs(v)


class NLCase:
    """_gn_reference.Case for the systems 'elliptic' / 'relaxed' with a reaction term: same factor construction, own sizes, z in (-1.2, 1.2)"""

    def __init__(self, kind, system, Nd, Nb, params=None):
        assert system in ('elliptic', 'relaxed')
        self.kind, self.system, self.Nd, self.Nb = kind, system, Nd, Nb
        self.params = PARAMS[kind] if params is None else tuple(params)
        self.nonlin = KIND_ID[kind]
        self.p0, self.p1, self.p2 = self.params
        self.lam = R.RELAXED_LAMBDA if system == 'relaxed' else 0.0
        self.Ndata, self.data, self.L2 = 0, None, None
        rng = np.random.RandomState(zlib.crc32(repr(('nl', system, Nd, Nb)).encode()))       # (one factor and one start per size: shared by the kinds)
        self.f = rng.uniform(0.5, 1.5, Nd)
        self.g = rng.uniform(0.5, 1.5, Nb)
        self.nz = R.n_unknowns(system, Nd)
        self.z0 = rng.uniform(-1.2, 1.2, self.nz)
        n = R.factor_order(system, Nd, Nb)
        self.L = R.synthetic_factor(rng, n)
        self.groups = [(0, n, self.L), (n, Nd, None)] if system == 'relaxed' else [(0, n, self.L)]
        self.rows = sum(g[1] for g in self.groups)


@functools.lru_cache(maxsize=None)
def case(kind, system, Nd, Nb):
    return NLCase(kind, system, Nd, Nb)


def linearise(cs, z):
    """[A(z) | F(z)] of the case at the float64 point z: a _gn_reference.Lin with Amag, the magnitude sum of every entry of A"""
    Nd, Nb = cs.Nd, cs.Nb
    z = np.asarray(z, dtype=np.float64).astype(LD)
    f, g = cs.f.astype(LD), cs.g.astype(LD)
    one = LD(1)
    lin = R.Lin(cs.rows, cs.nz)
    mags = []

    def put_a(r0, c0, vals, n, const=False, mag=None):
        lin.put_a(r0, c0, vals, n, const)
        mags.append(np.abs(lin.v[-1]) if mag is None else np.broadcast_to(np.asarray(mag, dtype=LD), (n,)).copy())

    if cs.system == 'elliptic':                      # rows [tau(u) - f; u; g]
        t, tm = tau_ld(cs.kind, cs.params, z)
        d, dm = dtau_ld(cs.kind, cs.params, z)
        lin.put_f(0, t - f, tm + np.abs(f)); lin.put_f(Nd, z); lin.put_f(2 * Nd, g)
        put_a(0, 0, d, Nd, mag=dm)
        put_a(Nd, 0, one, Nd, True)
    else:                                            # rows [v; w; g | (-v + tau(w) - f) / sqrt(lambda)]
        v, w = z[:Nd], z[Nd:]
        rs = one / np.sqrt(LD(cs.lam))
        P = 2 * Nd + Nb
        t, tm = tau_ld(cs.kind, cs.params, w)
        d, dm = dtau_ld(cs.kind, cs.params, w)
        lin.put_f(0, v); lin.put_f(Nd, w); lin.put_f(2 * Nd, g)
        lin.put_f(P, (-v + t - f) * rs, (np.abs(v) + tm + np.abs(f)) * rs)
        put_a(0, 0, one, 2 * Nd, True)
        put_a(P, 0, -rs, Nd)
        put_a(P, Nd, d * rs, Nd, mag=dm * rs)
    lin.finish()
    lin.Amag = np.concatenate(mags)
    return lin


def check_build(lin, A, F, budget, what=''):
    """_gn_reference.check_build with `budget` in the place of C_BUILD and lin.Amag in the place of |v|: structural zeros, constants and
    copies exactly, every other entry within budget x eps of the magnitude sum of its terms.  Returns the worst ratio."""
    worst = 0.0
    if A is not None:
        A = np.asarray(A, dtype=np.float64)
        assert A.shape == (lin.rows, lin.nz), (what, A.shape)
        pattern = np.zeros(A.shape, dtype=bool)
        pattern[lin.r, lin.c] = True
        assert np.all(A[~pattern] == 0.0), (what, 'non-zero outside the pattern of A(z)', np.argwhere(~pattern & (A != 0))[:4])
        got = A[lin.r, lin.c]
        k = lin.const
        assert np.array_equal(got[k], lin.v[k].astype(np.float64)), (what, 'a constant entry of A(z) is not exact')
        assert np.all(lin.Amag[~k] > 0)
        ra = np.abs(got[~k].astype(LD) - lin.v[~k]) / (LD(EPS) * lin.Amag[~k])
        worst = float(np.max(ra)) if ra.size else 0.0
        assert worst <= budget, (what, 'A(z)', worst, budget, int(lin.r[~k][np.argmax(ra)]), int(lin.c[~k][np.argmax(ra)]))
    F = np.asarray(F, dtype=np.float64)
    assert F.shape == (lin.rows,), (what, F.shape)
    assert np.array_equal(F[lin.Fcopy], lin.F[lin.Fcopy].astype(np.float64)), (what, 'a copied entry of F(z) is not exact')
    m = ~lin.Fcopy
    rf = np.abs(F[m].astype(LD) - lin.F[m]) / (LD(EPS) * lin.Fmag[m])
    wf = float(np.max(rf))
    assert wf <= budget, (what, 'F(z)', wf, budget, int(np.nonzero(m)[0][np.argmax(rf)]))
    return max(worst, wf)


class FullReference(R.FullReference):
    """_gn_reference.FullReference on linearise() above (same quantities, same scales)"""

    def __init__(self, cs, z):
        self.case, self.z = cs, np.array(z, dtype=np.float64)
        lin = self.lin = linearise(cs, z)
        nz = cs.nz
        Sb = R._group_solve(cs, np.concatenate([lin.dense(), lin.F[:, None]], axis=1))
        self.S, self.w = Sb[:, :nz], Sb[:, nz]
        G = R.gram_lower(Sb)
        self.H = LD(2) * G[:nz, :nz]
        self.g = LD(2) * G[nz, :nz]
        self.loss = self.w @ self.w
        Sa = np.abs(Sb).astype(np.float64)
        self.scaleH = 2.0 * (Sa[:, :nz].T @ Sa[:, :nz])
        self.scaleg = 2.0 * (Sa[:, :nz].T @ Sa[:, nz])
        self.p64 = R.Pipeline64(cs, z, lin)
        self.delta = R.refine(self.p64.solve, lambda d: self.g - self.H @ d, self.g.astype(np.float64))
        ev = np.linalg.eigvalsh(self.H.astype(np.float64))
        self.normH, self.cond = float(ev[-1]), float(ev[-1] / ev[0])


class VectorReference(R.VectorReference):
    """_gn_reference.VectorReference on linearise() above"""

    def __init__(self, cs, z, want_delta=True):
        self.case, self.z = cs, np.array(z, dtype=np.float64)
        lin = self.lin = linearise(cs, z)
        self.w = R._group_solve(cs, lin.F)
        self.loss = self.w @ self.w
        self.g = LD(2) * lin.tmul(R._group_solve(cs, self.w, trans=True))
        self.p64 = R.Pipeline64(cs, z, lin)
        self.normH = R.norm2_power(lambda x: self.p64.H @ x, cs.nz)
        self.delta = R.refine(self.p64.solve, lambda d: -self.residual(d), self.g.astype(np.float64)) if want_delta else None


@functools.lru_cache(maxsize=None)
def full_reference(kind, system, Nd, Nb):
    cs = case(kind, system, Nd, Nb)
    return FullReference(cs, cs.z0)


@functools.lru_cache(maxsize=None)
def vector_reference(kind, system, Nd, Nb):
    cs = case(kind, system, Nd, Nb)
    return VectorReference(cs, cs.z0)


# ------------------------------------------------------------------------------------------------ the whole solve in float64
def cpu_chain(Theta, tau, f, g, z0, steps):
    """numpy.linalg.cholesky of Theta (nugget included), then `steps` Gauss-Newton steps of the elimination formulation in float64 with
    the host reaction term `tau` (src/nonlinearity.Nonlinearity): (z, loss history J(z_0) .. J(z_steps), L, sol_vec)"""
    from scipy.linalg import cho_factor, cho_solve, solve_triangular
    f, g = np.asarray(f, dtype=np.float64), np.asarray(g, dtype=np.float64)
    Nd, N = f.size, Theta.shape[0]
    L = np.linalg.cholesky(Theta)
    z = np.array(z0, dtype=np.float64)
    hist = []
    meas = lambda u: np.concatenate([tau.tau(u) - f, u, g])
    for it in range(steps + 1):
        w = solve_triangular(L, meas(z), lower=True, check_finite=False)
        hist.append(float(w @ w))
        if it == steps:
            break
        A = np.zeros((N, Nd))
        A[np.arange(Nd), np.arange(Nd)] = tau.dtau(z)
        A[Nd + np.arange(Nd), np.arange(Nd)] = 1.0
        S = solve_triangular(L, A, lower=True, check_finite=False)
        z = z - cho_solve(cho_factor(2.0 * (S.T @ S), lower=True, check_finite=False), 2.0 * (S.T @ w), check_finite=False)
    return z, np.array(hist), L, meas(z)


def extend_cpu(L, Theta_test, sol_vec):
    from scipy.linalg import solve_triangular
    c = solve_triangular(L, solve_triangular(L, sol_vec, lower=True, check_finite=False), lower=True, trans='T', check_finite=False)
    return Theta_test @ c


def space_time_boundary(rng, Nb):
    """Nb points on the faces of the unit cube other than x3 = 1 (initial and lateral data of a space-time problem), face by face in turn"""
    X = rng.uniform(0, 1, (Nb, 3))
    for b in range(Nb):
        axis, side = ((0, 0.0), (0, 1.0), (1, 0.0), (1, 1.0), (2, 0.0))[b % 5]
        X[b, axis] = side
    return X
