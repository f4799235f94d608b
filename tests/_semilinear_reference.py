"""Reference of the semilinear system GPK_GN_SEMILINEAR (CPU only), in the manner of tests/_gn_reference.py, whose synthetic factors,
poisoned upload and sizes it shares:

    -eps Laplace(u) + N(u, grad u) = f,   N(u, p, q) = u (a1 p + a2 q) + b (p^2 + q^2) + c1 u + c3 u^3,   gq = (a1, a2, b, c1, c3)
    unknowns z = [v0 | v1 | v2],   F(z) = [v1; v2; (N(v0, v1, v2) - f) / eps; v0; g],   A(z) = dF/dz   (include/gpk.h)

  N, dN               the nonlinearity and its partial derivatives for any dtype (long double, complex for the complex-step check)
  linearise           F(z), the magnitude sums of its entries and the entries of A(z) with their magnitude sums, long double
  check_build         [A | F] as a kernel wrote it against those entries: copies and constants exact, the rest within 4 ulp
  FullReference       S, H, g, loss, delta of one step in long double, with the float64 pipeline (_gn_reference.Pipeline64) next to it
  VectorReference     the same step without L^-1 A (_gn_reference.VectorReference on this linearise): loss, g, delta, H as an operator
  gn_float64          the float64 Gauss-Newton iteration on a Gram factor (the oracle's gn_method with this system)
  posterior_*, log_evidence   the numpy formulas of include/gpk.h with the reference's P and R, in the dtype asked for
"""
import functools
import zlib

import numpy as np

import _gn_reference as R
from _gn_reference import NB, poisoned, synthetic_factor  # noqa: F401  (shared with the device tests)

LD, EPS = R.LD, R.EPS
GQ = (0.7, -0.4, 0.3, 0.5, 0.2)                  # every entry of A live, dN/du != 0
EPS_PDE = 0.1
SIZES = (65, 129, 333)
# Rounding budget of a computed entry of [A(z) | F(z)], in units of eps = 2^-52 of the magnitude sum of its terms (the convention of
# _gn_reference.C_BUILD: an entry that is a sum can cancel, and no float64 evaluation is then within a few ulp of the RESULT).  Each
# correctly rounded operation costs eps / 2 of a magnitude that is at most the sum.  As sl_N / sl_dN of csrc/gpk_common.h are written:
#   F: c3 u^3 takes u u, c3 *, c1 +, u * = 2; then (conv + grad), + reac, - f, / eps = 2 more: 4.   N_u / eps: 3;   N_p / eps, N_q / eps: 2.
C_BUILD = 4.0
MARGIN = 8.0                                     # device error <= 8 x max(float64 pipeline error, eps x scale)


def N(gq, u, p, q):
    a1, a2, b, c1, c3 = gq
    return u * (a1 * p + a2 * q) + b * (p * p + q * q) + c1 * u + c3 * u * u * u


def dN(gq, u, p, q):
    a1, a2, b, c1, c3 = gq
    return a1 * p + a2 * q + c1 + 3 * c3 * u * u, a1 * u + 2 * b * p, a2 * u + 2 * b * q


def N_mag(gq, u, p, q):
    a1, a2, b, c1, c3 = (abs(v) for v in gq)
    u, p, q = np.abs(u), np.abs(p), np.abs(q)
    return u * (a1 * p + a2 * q) + b * (p * p + q * q) + c1 * u + c3 * u * u * u


def dN_mag(gq, u, p, q):
    a1, a2, b, c1, c3 = (abs(v) for v in gq)
    u, p, q = np.abs(u), np.abs(p), np.abs(q)
    return a1 * p + a2 * q + c1 + 3 * c3 * u * u, a1 * u + 2 * b * p, a2 * u + 2 * b * q


class Case:
    """inputs of one N_d: coefficients, right-hand sides, factor, start point; seeded per (gq, eps, N_d).  The attributes _gn_reference's
    Pipeline64 and solvers read (groups, nz, rows) are those of its own Case."""
    system = 'semilinear'

    def __init__(self, Nd, Nb, gq=GQ, eps=EPS_PDE, like=None):
        self.Nd, self.Nb, self.gq, self.eps = Nd, Nb, tuple(float(v) for v in gq), float(eps)
        self.nz, n = 3 * Nd, 4 * Nd + Nb
        if like is None:
            rng = np.random.RandomState(zlib.crc32(repr(('semilinear', Nd, Nb)).encode()))
            self.f = rng.uniform(0.5, 1.5, Nd)
            self.g = rng.uniform(0.5, 1.5, Nb)
            self.z0 = rng.uniform(0.3, 1.2, self.nz) * rng.choice([-1.0, 1.0], self.nz)
            self.L = synthetic_factor(rng, n)
        else:                                    # the same factor, data and start point under other coefficients
            self.f, self.g, self.z0, self.L = like.f, like.g, like.z0, like.L
        self.groups = [(0, n, self.L)]
        self.rows = n


@functools.lru_cache(maxsize=None)
def case(Nd):
    return Case(Nd, NB[Nd])


class Lin(R.Lin):
    """_gn_reference.Lin with a magnitude sum per entry of A as well (an entry of this system's A(z) is a sum of several terms)"""

    def __init__(self, rows, nz):
        super().__init__(rows, nz)
        self.amag = []

    def put_a(self, r0, c0, vals, n, const=False, mag=None):
        super().put_a(r0, c0, vals, n, const)
        self.amag.append(np.abs(self.v[-1]) if mag is None else np.broadcast_to(np.asarray(mag, dtype=LD), (n,)).copy())

    def finish(self):
        self.amag = np.concatenate(self.amag)
        return super().finish()


def linearise(cs, z, f=None):
    """[A(z) | F(z)] at the float64 point z with long-double entries"""
    Nd = cs.Nd
    z = np.asarray(z, dtype=np.float64).astype(LD)
    f = (cs.f if f is None else np.asarray(f, dtype=np.float64)).astype(LD)
    g = cs.g.astype(LD)
    gq, eps, one = tuple(LD(v) for v in cs.gq), LD(cs.eps), LD(1)
    v0, v1, v2 = z[:Nd], z[Nd:2 * Nd], z[2 * Nd:]
    lin = Lin(cs.rows, cs.nz)
    lin.put_f(0, v1); lin.put_f(Nd, v2)
    lin.put_f(2 * Nd, (N(gq, v0, v1, v2) - f) / eps, (N_mag(gq, v0, v1, v2) + np.abs(f)) / np.abs(eps))
    lin.put_f(3 * Nd, v0); lin.put_f(4 * Nd, g)
    Nu, Np, Nq = dN(gq, v0, v1, v2)
    mu, mp, mq = dN_mag(gq, v0, v1, v2)
    lin.put_a(0, Nd, one, Nd, True); lin.put_a(Nd, 2 * Nd, one, Nd, True)
    lin.put_a(2 * Nd, 0, Nu / eps, Nd, mag=mu / np.abs(eps))
    lin.put_a(2 * Nd, Nd, Np / eps, Nd, mag=mp / np.abs(eps))
    lin.put_a(2 * Nd, 2 * Nd, Nq / eps, Nd, mag=mq / np.abs(eps))
    lin.put_a(3 * Nd, 0, one, Nd, True)
    return lin.finish()


def check_build(lin, A, F, what=''):
    """[A | F] as a kernel wrote it (A in the natural order of the unknowns) against the long-double entries: structural zeros, constants
    and copies exactly, every computed entry within C_BUILD ulp (eps x the magnitude sum of its terms).  Returns the worst ratio."""
    A = np.asarray(A, dtype=np.float64)
    assert A.shape == (lin.rows, lin.nz), (what, A.shape)
    pattern = np.zeros(A.shape, dtype=bool)
    pattern[lin.r, lin.c] = True
    assert np.all(A[~pattern] == 0.0), (what, 'non-zero outside the pattern of A(z)', np.argwhere(~pattern & (A != 0))[:4])
    got, k = A[lin.r, lin.c], lin.const
    assert np.array_equal(got[k], lin.v[k].astype(np.float64)), (what, 'a constant entry of A(z) is not exact')
    ra = np.abs(got[~k].astype(LD) - lin.v[~k]) / (LD(EPS) * lin.amag[~k])
    worst = float(np.max(ra))
    assert worst <= C_BUILD, (what, 'A(z)', worst, int(lin.r[~k][np.argmax(ra)]), int(lin.c[~k][np.argmax(ra)]))
    F = np.asarray(F, dtype=np.float64)
    assert np.array_equal(F[lin.Fcopy], lin.F[lin.Fcopy].astype(np.float64)), (what, 'a copied entry of F(z) is not exact')
    m = ~lin.Fcopy
    rf = np.abs(F[m].astype(LD) - lin.F[m]) / (LD(EPS) * lin.Fmag[m])
    assert float(np.max(rf)) <= C_BUILD, (what, 'F(z)', float(np.max(rf)), int(np.nonzero(m)[0][np.argmax(rf)]))
    return max(worst, float(np.max(rf)))


class FullReference:
    """one step at z in long double -- S = L^-1 A, w = L^-1 F, H = 2 S^T S, g = 2 S^T w, loss = w^T w, delta (float64 Cholesky + long-double
    refinement) -- with the rounding scales 2 |S|^T |S| and 2 |S|^T |w|, and the float64 pipeline p64 on the same inputs"""

    def __init__(self, cs, z, f=None):
        self.case, self.z = cs, np.array(z, dtype=np.float64)
        lin = self.lin = linearise(cs, z, f)
        nz = cs.nz
        Sb = R._group_solve(cs, np.concatenate([lin.dense(), lin.F[:, None]], axis=1))
        self.S, self.w = Sb[:, :nz], Sb[:, nz]
        G = R.gram_lower(Sb)
        self.H, self.g, self.loss = LD(2) * G[:nz, :nz], LD(2) * G[nz, :nz], self.w @ self.w
        Sa = np.abs(Sb).astype(np.float64)
        self.scaleH = 2.0 * (Sa[:, :nz].T @ Sa[:, :nz])
        self.scaleg = 2.0 * (Sa[:, :nz].T @ Sa[:, nz])
        self.p64 = R.Pipeline64(cs, z, lin)
        self.delta = R.refine(self.p64.solve, lambda d: self.g - self.H @ d, self.g.astype(np.float64))
        ev = np.linalg.eigvalsh(self.H.astype(np.float64))
        self.normH, self.cond = float(ev[-1]), float(ev[-1] / ev[0])


@functools.lru_cache(maxsize=None)
def full_reference(Nd):
    cs = case(Nd)
    return FullReference(cs, cs.z0)


class VectorReference(R.VectorReference):
    """_gn_reference.VectorReference (w, loss, g, p64, normH, delta, apply_H, residual: the step without L^-1 A, O(N^2)) on this
    module's linearise, for the sizes the full form is too slow for; the gates gate_loss, gate_backward_vec, gate_forward of
    _gn_reference apply to it unchanged"""

    def __init__(self, cs, z, want_delta=True):
        super().__init__(cs, z, want_delta, lin_fn=linearise)


@functools.lru_cache(maxsize=None)
def vector_reference(Nd, Nb):
    cs = case(Nd) if NB.get(Nd) == Nb else Case(Nd, Nb)
    return VectorReference(cs, cs.z0)


def err(got, ref):
    return np.abs(np.asarray(got).astype(LD) - ref).astype(np.float64)


def gates(ref, H=None, g=None, loss=None, delta=None, z_out=None, step=1.0):
    """{quantity: (device error, allowed)} with allowed = MARGIN x max(error of the float64 pipeline, eps x rounding scale), each as the
    maximum over the entries of error / scale: H and g per entry against 2 |S|^T |S| and 2 |S|^T |w|, the loss against itself, delta
    and the updated z against max |delta_ld| (resp. max |z| + |step delta|)"""
    p = ref.p64
    out = {}

    def put(name, e_dev, e_64, scale):
        scale = np.where(np.asarray(scale) == 0, 1.0, scale)
        out[name] = (float(np.max(e_dev / scale)), MARGIN * max(float(np.max(e_64 / scale)), EPS))
    if H is not None:
        put('H', err(H, ref.H), err(p.H, ref.H), ref.scaleH)
    if g is not None:
        put('g', err(g, ref.g), err(p.g, ref.g), ref.scaleg)
    if loss is not None:
        put('loss', err(loss, ref.loss), err(p.loss, ref.loss), float(ref.loss))
    if delta is not None:
        dn = float(np.max(np.abs(ref.delta.astype(np.float64))))
        put('delta', err(delta, ref.delta), err(p.delta, ref.delta), dn)
    if z_out is not None:
        want = ref.z.astype(LD) - LD(step) * ref.delta
        zn = float(np.max(np.abs(ref.z) + abs(step) * np.abs(ref.delta.astype(np.float64))))
        put('z', err(z_out, want), err(ref.z - step * p.delta, want), zn)
    return out


# ------------------------------------------------------------------------------------------------ float64 Gauss-Newton on a Gram factor
class System:
    """F and A of the system as the numpy oracle's gn_method takes them (oracle/gp_oracle.py: EikonalSystem is the model)"""

    def __init__(self, eps, gq, rhs_f, bdy_g):
        self.eps, self.gq = float(eps), tuple(float(v) for v in gq)
        self.f, self.g = np.asarray(rhs_f, dtype=np.float64), np.asarray(bdy_g, dtype=np.float64)
        self.Nd, self.Nb = self.f.size, self.g.size
        self.nz = 3 * self.Nd

    def _split(self, z):
        Nd = self.Nd
        return z[:Nd], z[Nd:2 * Nd], z[2 * Nd:]

    def F(self, z):
        v0, v1, v2 = self._split(z)
        return [np.concatenate([v1, v2, (N(self.gq, v0, v1, v2) - self.f) / self.eps, v0, self.g])]

    def A(self, z):
        Nd = self.Nd
        v0, v1, v2 = self._split(z)
        Nu, Np, Nq = dN(self.gq, v0, v1, v2)
        A = np.zeros((4 * Nd + self.Nb, 3 * Nd))
        i = np.arange(Nd)
        A[i, Nd + i] = 1.0; A[Nd + i, 2 * Nd + i] = 1.0; A[3 * Nd + i, i] = 1.0
        A[2 * Nd + i, i] = Nu / self.eps; A[2 * Nd + i, Nd + i] = Np / self.eps; A[2 * Nd + i, 2 * Nd + i] = Nq / self.eps
        return [A]

    def extra(self, z):
        return 0.0, None, None

    def sol_vec(self, z):
        return self.F(z)


def gn_float64(sysm, L, z0, steps):
    """(z, loss history) of `steps` plain Gauss-Newton steps in float64: the oracle's gn_method (scipy triangular solves, BLAS product,
    LAPACK Cholesky) with this system"""
    from oracle import gp_oracle as O
    return O.gn_method(sysm, [L], z0, steps, 1)


def truth(x1, x2):
    return np.sin(np.pi * x1) * np.sin(np.pi * x2)


def manufactured_rhs(eps, gq, x1, x2):
    """f = -eps Laplace(u*) + N(u*, grad u*) for u* = sin(pi x1) sin(pi x2)"""
    pi = np.pi
    u = truth(x1, x2)
    return 2 * pi ** 2 * eps * u + N(gq, u, pi * np.cos(pi * x1) * np.sin(pi * x2), pi * np.sin(pi * x1) * np.cos(pi * x2))


def points(Nd, Nb, seed=7):
    """interior and boundary points of the unit square (Nb a multiple of 4)"""
    rng = np.random.RandomState(seed)
    Xd = rng.uniform(0.0, 1.0, (Nd, 2))
    s = rng.uniform(0.0, 1.0, Nb)
    k = Nb // 4
    Xb = np.concatenate([np.stack([s[:k], np.zeros(k)], 1), np.stack([s[k:2 * k], np.ones(k)], 1),
                         np.stack([np.zeros(k), s[2 * k:3 * k]], 1), np.stack([np.ones(Nb - 3 * k), s[3 * k:]], 1)])
    return Xd, Xb


# ------------------------------------------------------------------------------------------------ posterior and evidence (include/gpk.h)
def _solve_l(L, B, dtype):
    if dtype is LD:
        return R.solve_lower(L, B)
    from scipy.linalg import solve_triangular
    return solve_triangular(L, np.asarray(B, dtype=np.float64), lower=True, check_finite=False)


def posterior_prepare(sysm, L, z, dtype=np.float64):
    """(P, R): P = L^-1 A(z), R R^T = P^T P = H/2.  dtype LD: P and the product in long double, R from the float64 Cholesky of the
    rounded product refined by nothing -- H/2 is well conditioned relative to the tolerance at the sizes used (checked by the caller
    through the float64 figure)."""
    A = sysm.A(z)[0]
    P = _solve_l(L, A.astype(dtype), dtype)
    G = P.T @ P
    Rf = np.linalg.cholesky(G.astype(np.float64))
    return P, Rf, G


def posterior_covariance(L, P, G, K, Ktt, dtype=np.float64):
    """Sigma = Ktt - V^T V + W^T (H/2)^-1 W,  V = L^-1 K,  W = P^T V  (K: N x nt, Ktt: nt x nt); its diagonal is the variance"""
    V = _solve_l(L, K.astype(dtype), dtype)
    W = P.T @ V
    X = np.linalg.solve(G.astype(np.float64), W.astype(np.float64))
    if dtype is LD:                              # one step of refinement in long double
        X = X.astype(LD) + np.linalg.solve(G.astype(np.float64), (W - G @ X.astype(LD)).astype(np.float64)).astype(LD)
    cond = Ktt.astype(dtype) - V.T @ V
    return cond, cond + W.T @ X


def log_evidence(sysm, L, z, Rf):
    """the six terms of gpk_log_evidence in float64"""
    w = _solve_l(L, sysm.F(z)[0], np.float64)
    J = float(w @ w)
    ldt = 2.0 * float(np.sum(np.log(np.diag(L))))
    ldh = 2.0 * float(np.sum(np.log(np.diag(Rf))))
    two_pi = 0.5 * (L.shape[0] - sysm.nz) * np.log(2 * np.pi)
    return dict(log_Z=-(J + ldt + ldh) / 2 - two_pi, J=J, logdet_theta=ldt, logdet_H=ldh, gamma_term=0.0, two_pi_term=two_pi)
