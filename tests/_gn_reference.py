"""Long-double reference of one Gauss-Newton step on synthetic, well-conditioned factors (CPU only).

The kernels of the step do not care where the factor L comes from.  With L = tril(normal) + diag(uniform(3, 4) sqrt(n)) (the
construction of test_gpu_parity.py::test_trsm) the Gauss-Newton matrix H = 2 A^T L^-T L^-1 A (+ the rows without a factor) has a
condition number of 1e1 .. 1e6 instead of the 1e10 .. 1e12 of a Gram factor, so the whole step -- [A(z) | F(z)], the solved block, H, g,
the loss, delta and the update -- is determined to rounding and a long-double evaluation decides it.

Everything is written from the equations (oracle/gp_oracle.py: EllipticSystem, EllipticRelaxedSystem, BurgersSystem, EikonalSystem,
DarcySystem) with np.longdouble ENTRIES -- the oracle's own arrays are float64 -- in the stacked row layout of the library
(csrc/gpk_gn.hip, gn_dims): the row groups of a system below each other, each with its factor or without one (the relaxed system's
penalty rows; the Darcy data misfit (v0 - data) / gamma written as rows, so that the data term is part of S^T S and of its scale).

  linearise(case, z)    F(z), the magnitude sum of the terms of every entry of F, and A(z) as a list of entries (row, unknown, value,
                        constant or z-dependent)
  full_reference        S = L^-1 [A | F], H, g, loss in long double and their rounding scales (N_d <= 129: O(N^3) long-double work)
  VectorReference       the same step without L^-1 A: loss, g, the normal-equations residual r(d) = 2 A^T L^-T L^-1 (A d - F) = H d - g
                        and delta by float64 Cholesky + long-double refinement; two single-vector solves per factor and product
  Pipeline64            the float64 pipeline the device is judged against (scipy triangular solves, BLAS products, LAPACK Cholesky)
"""
import functools
import zlib

import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
POISON = 1e30                                    # strict upper triangle and padding of every uploaded factor
LD_PAD = 16                                      # the factor lives in a buffer with ld = n + LD_PAD

SYSTEMS = ('elliptic', 'relaxed', 'burgers', 'eikonal', 'darcy')
SYSTEM_NAME = {'elliptic': 'Nonlinear_elliptic', 'relaxed': 'Nonlinear_elliptic_relaxed', 'burgers': 'Burgers', 'eikonal': 'Eikonal',
               'darcy': 'Darcy_flow2d'}
# N_b and N_data of tests/test_gpu_staircase.py; (1100, 160) is the size of test_gpu_variants.py::test_schedule_variants_agree
NB = {65: 13, 129: 3, 333: 17, 1100: 160}
NDATA = {65: 64, 129: 129, 333: 50, 1100: 60}
# The relaxed system at the penalty 1e-3 of test_gpu_staircase._problem has cond(H) = 5e7 .. 9e7 with these factors (the penalty rows carry
# 1 / lambda against 1 / (12 n) of the factor's rows), and delta is then only determined to cond(H) eps = 1e-9.  cond(H) falls like
# 1 / lambda: with lambda = 100 it is 5e2, 9e2, 2.4e3 at N_d = 65, 129, 333 (tests/test_gn_reference_host.py asserts < 1e4).
RELAXED_LAMBDA = 100.0
# (p0, p1, pen_lambda): the parameters of tests/test_gpu_staircase._problem, except the relaxed penalty
PARAMS = {'elliptic': (1.0, 3.0, 0.0), 'relaxed': (1.0, 3.0, RELAXED_LAMBDA), 'burgers': (0.7, 0.02, 0.0), 'eikonal': (0.1, 0.0, 0.0),
          'darcy': (0.05, 0.0, 0.0)}


def n_unknowns(system, Nd):
    return {'elliptic': Nd, 'relaxed': 2 * Nd, 'burgers': 3 * Nd, 'eikonal': 3 * Nd, 'darcy': 6 * Nd}[system]


def factor_order(system, Nd, Nb):
    return {'elliptic': 2 * Nd + Nb, 'relaxed': 2 * Nd + Nb}.get(system, 4 * Nd + Nb)


def synthetic_factor(rng, n):
    return np.tril(rng.normal(size=(n, n))) + np.diag(rng.uniform(3, 4, n) * np.sqrt(n))


class Case:
    """inputs of one (system, N_d): parameters, right-hand sides, factors, start point; seeded per (system, N_d)"""

    def __init__(self, system, Nd):
        self.system, self.Nd, self.Nb = system, Nd, NB[Nd]
        self.Ndata = NDATA[Nd] if system == 'darcy' else 0
        self.p0, self.p1, self.lam = PARAMS[system]
        rng = np.random.RandomState(zlib.crc32(repr((system, Nd)).encode()))
        self.f = rng.uniform(0.5, 1.5, Nd)
        self.g = rng.uniform(0.5, 1.5, self.Nb)
        self.data = rng.uniform(0.5, 1.5, self.Ndata) if system == 'darcy' else None
        self.nz = n_unknowns(system, Nd)
        self.z0 = rng.uniform(0.3, 1.2, self.nz) * rng.choice([-1.0, 1.0], self.nz)     # no zero entries: every entry of A(z) is non-zero
        n = factor_order(system, Nd, self.Nb)
        self.L = synthetic_factor(rng, n)
        self.L2 = synthetic_factor(rng, 3 * Nd) if system == 'darcy' else None
        # row groups (offset, rows, factor) in the library's stacked order
        if system == 'darcy':
            self.groups = [(0, 3 * Nd, self.L2), (3 * Nd, n, self.L), (3 * Nd + n, self.Ndata, None)]
        elif system == 'relaxed':
            self.groups = [(0, n, self.L), (n, Nd, None)]
        else:
            self.groups = [(0, n, self.L)]
        self.rows = sum(g[1] for g in self.groups)

    def oracle(self):
        """(the float64 oracle's system, its factor list) for the same inputs"""
        from oracle import gp_oracle as O
        s = self.system
        if s == 'elliptic':
            return O.EllipticSystem(self.p0, self.p1, self.f, self.g), [self.L]
        if s == 'relaxed':
            return O.EllipticRelaxedSystem(self.p0, self.p1, self.f, self.g, self.lam), [self.L, None]
        if s == 'burgers':
            return O.BurgersSystem(self.p0, self.p1, self.f, self.g), [self.L]
        if s == 'eikonal':
            return O.EikonalSystem(self.p0, self.f, self.g), [self.L]
        return O.DarcySystem(self.f, self.g, self.data, self.p0), [self.L2, self.L]


@functools.lru_cache(maxsize=None)
def case(system, Nd):
    return Case(system, Nd)


def poisoned(L):
    """the factor as it is uploaded: n x (n + LD_PAD), strict upper triangle and padding = POISON (nothing may read either)"""
    n = L.shape[0]
    out = np.full((n, n + LD_PAD), POISON)
    out[:, :n] = np.where(np.tri(n, dtype=bool), L, POISON)
    return out


# ------------------------------------------------------------------------------------------------ F(z), A(z) in long double
class Lin:
    """F (rows,), Fmag (rows,: sum of the magnitudes of the terms of each entry), and the entries of A: r, c (natural unknown order), v,
    const (True: a structural constant +-1 / nu that the device must reproduce exactly)"""

    def __init__(self, rows, nz):
        self.rows, self.nz = rows, nz
        self.F = np.zeros(rows, dtype=LD)
        self.Fmag = np.zeros(rows, dtype=LD)
        self.Fcopy = np.zeros(rows, dtype=bool)              # a plain copy of an input (z, g): the device must reproduce it exactly
        self.r, self.c, self.v, self.const = [], [], [], []

    def put_f(self, r0, vals, mag=None):
        vals = np.asarray(vals, dtype=LD)
        self.F[r0:r0 + vals.size] = vals
        self.Fmag[r0:r0 + vals.size] = np.abs(vals) if mag is None else mag
        self.Fcopy[r0:r0 + vals.size] = mag is None

    def put_a(self, r0, c0, vals, n, const=False):
        self.r.append(r0 + np.arange(n)); self.c.append(c0 + np.arange(n))
        self.v.append(np.broadcast_to(np.asarray(vals, dtype=LD), (n,)).copy())
        self.const.append(np.full(n, const))

    def finish(self):
        self.r, self.c = np.concatenate(self.r), np.concatenate(self.c)
        self.v, self.const = np.concatenate(self.v), np.concatenate(self.const)
        return self

    def dense(self, dtype=LD):
        A = np.zeros((self.rows, self.nz), dtype=dtype)
        A[self.r, self.c] = self.v.astype(dtype)
        return A

    def mul(self, d):
        """A d (long double)"""
        out = np.zeros(self.rows, dtype=LD)
        np.add.at(out, self.r, self.v * np.asarray(d, dtype=LD)[self.c])
        return out

    def tmul(self, y):
        """A^T y (long double)"""
        out = np.zeros(self.nz, dtype=LD)
        np.add.at(out, self.c, self.v * np.asarray(y, dtype=LD)[self.r])
        return out


def linearise(cs, z):
    """[A(z) | F(z)] of the case at the float64 point z with long-double entries (the float64 inputs are exact long doubles)"""
    Nd, Nb, s = cs.Nd, cs.Nb, cs.system
    z = np.asarray(z, dtype=np.float64).astype(LD)
    f, g = cs.f.astype(LD), cs.g.astype(LD)
    p0, p1 = LD(cs.p0), LD(cs.p1)
    one = LD(1)
    lin = Lin(cs.rows, cs.nz)
    if s == 'elliptic':                            # rows [alpha u^m - f; u; g]
        t1 = p0 * z ** p1
        lin.put_f(0, t1 - f, np.abs(t1) + np.abs(f)); lin.put_f(Nd, z); lin.put_f(2 * Nd, g)
        lin.put_a(0, 0, p0 * p1 * z ** (p1 - one), Nd)
        lin.put_a(Nd, 0, one, Nd, True)
    elif s == 'relaxed':                           # rows [v; w; g | (-v + alpha w^m - f) / sqrt(lambda)]
        v, w = z[:Nd], z[Nd:]
        rs = one / np.sqrt(LD(cs.lam))
        P = 2 * Nd + Nb
        t1 = p0 * w ** p1
        lin.put_f(0, v); lin.put_f(Nd, w); lin.put_f(2 * Nd, g)
        lin.put_f(P, (-v + t1 - f) * rs, (np.abs(v) + np.abs(t1) + np.abs(f)) * rs)
        lin.put_a(0, 0, one, 2 * Nd, True)
        lin.put_a(P, 0, -rs, Nd)
        lin.put_a(P, Nd, p0 * p1 * w ** (p1 - one) * rs, Nd)
    elif s == 'burgers':                           # unknowns [v0 | v2 | v3]; rows [nu v3 + f - alpha v0 v2; v2; v3; v0; g]
        v0, v2, v3 = z[:Nd], z[Nd:2 * Nd], z[2 * Nd:]
        lin.put_f(0, p1 * v3 + f - p0 * v0 * v2, np.abs(p1 * v3) + np.abs(f) + np.abs(p0 * v0 * v2))
        lin.put_f(Nd, v2); lin.put_f(2 * Nd, v3); lin.put_f(3 * Nd, v0); lin.put_f(4 * Nd, g)
        lin.put_a(0, 0, -p0 * v2, Nd); lin.put_a(0, Nd, -p0 * v0, Nd); lin.put_a(0, 2 * Nd, p1, Nd, True)
        lin.put_a(Nd, Nd, one, Nd, True); lin.put_a(2 * Nd, 2 * Nd, one, Nd, True); lin.put_a(3 * Nd, 0, one, Nd, True)
    elif s == 'eikonal':                           # unknowns [v0 | v1 | v2]; rows [v1; v2; -(f^2 - v1^2 - v2^2) / eps; v0; g]
        v0, v1, v2 = z[:Nd], z[Nd:2 * Nd], z[2 * Nd:]
        lin.put_f(0, v1); lin.put_f(Nd, v2)
        lin.put_f(2 * Nd, -(f * f - v1 * v1 - v2 * v2) / p0, (f * f + v1 * v1 + v2 * v2) / p0)
        lin.put_f(3 * Nd, v0); lin.put_f(4 * Nd, g)
        lin.put_a(0, Nd, one, Nd, True); lin.put_a(Nd, 2 * Nd, one, Nd, True)
        lin.put_a(2 * Nd, Nd, LD(2) * v1 / p0, Nd); lin.put_a(2 * Nd, 2 * Nd, LD(2) * v2 / p0, Nd)
        lin.put_a(3 * Nd, 0, one, Nd, True)
    elif s == 'darcy':                             # unknowns [w0 w1 w2 v0 v1 v2]; rows [w1; w2; w0 | v1; v2; v3; v0; g | (v0 - data) / gamma]
        w0, w1, w2, v0, v1, v2 = (z[k * Nd:(k + 1) * Nd] for k in range(6))
        fe = f * np.exp(-w0)
        U, D, nd = 3 * Nd, 7 * Nd + Nb, cs.Ndata
        lin.put_f(0, w1); lin.put_f(Nd, w2); lin.put_f(2 * Nd, w0)
        lin.put_f(U, v1); lin.put_f(U + Nd, v2)
        lin.put_f(U + 2 * Nd, -v1 * w1 - v2 * w2 - fe, np.abs(v1 * w1) + np.abs(v2 * w2) + np.abs(fe))
        lin.put_f(U + 3 * Nd, v0); lin.put_f(U + 4 * Nd, g)
        data = cs.data.astype(LD)
        lin.put_f(D, (v0[:nd] - data) / p0, (np.abs(v0[:nd]) + np.abs(data)) / p0)
        lin.put_a(0, Nd, one, Nd, True); lin.put_a(Nd, 2 * Nd, one, Nd, True); lin.put_a(2 * Nd, 0, one, Nd, True)
        lin.put_a(U, 4 * Nd, one, Nd, True); lin.put_a(U + Nd, 5 * Nd, one, Nd, True)
        lin.put_a(U + 2 * Nd, 0, fe, Nd); lin.put_a(U + 2 * Nd, Nd, -v1, Nd); lin.put_a(U + 2 * Nd, 2 * Nd, -v2, Nd)
        lin.put_a(U + 2 * Nd, 4 * Nd, -w1, Nd); lin.put_a(U + 2 * Nd, 5 * Nd, -w2, Nd)
        lin.put_a(U + 3 * Nd, 3 * Nd, one, Nd, True)
        lin.put_a(D, 3 * Nd, one / p0, nd)
    else:
        raise ValueError(s)
    return lin.finish()


# ------------------------------------------------------------------------------------------------ long-double substitution
def solve_lower(L, B):
    """L^-1 B in long double: a loop over the rows, vectorised over the columns of B (L float64, its entries exact long doubles)"""
    X = np.array(B, dtype=LD)
    for i in range(L.shape[0]):
        if i:
            X[i] -= L[i, :i].astype(LD) @ X[:i]
        X[i] /= LD(L[i, i])
    return X


def solve_lower_t(L, B):
    """L^-T B in long double, reading L by rows (column-oriented back substitution)"""
    X = np.array(B, dtype=LD)
    for i in range(L.shape[0] - 1, -1, -1):
        X[i] /= LD(L[i, i])
        if i:
            X[:i] -= np.multiply.outer(L[i, :i].astype(LD), X[i]) if X.ndim > 1 else L[i, :i].astype(LD) * X[i]
    return X


def gram_lower(S, block=128):
    """S^T S in long double: the lower block triangle by column blocks (einsum is several times faster than matmul for long double),
    mirrored, so that the result is exactly symmetric"""
    n = S.shape[1]
    G = np.zeros((n, n), dtype=LD)
    for j0 in range(0, n, block):
        j1 = min(j0 + block, n)
        G[j0:, j0:j1] = np.einsum('ki,kj->ij', S[:, j0:], S[:, j0:j1])
    iu = np.triu_indices(n, 1)
    G[iu] = G.T[iu]
    return G


def _group_solve(cs, B, trans=False):
    out = np.array(B, dtype=LD)
    for off, n, L in cs.groups:
        if L is not None and n:
            out[off:off + n] = (solve_lower_t if trans else solve_lower)(L, out[off:off + n])
    return out


def refine(solve64, residual, rhs64):
    """delta with H delta = g: float64 Cholesky solves corrected by long-double residuals until the residual stops shrinking.
    solve64(r) applies the float64 factorisation, residual(d) returns g - H d in long double."""
    d = solve64(rhs64).astype(LD)
    r = residual(d)
    best = np.linalg.norm(r.astype(np.float64))
    for _ in range(20):
        d_new = d + solve64(r.astype(np.float64)).astype(LD)
        r_new = residual(d_new)
        nrm = np.linalg.norm(r_new.astype(np.float64))
        if not nrm < best:
            break
        d, r, best = d_new, r_new, nrm
        if nrm == 0.0:
            break
    return d


def norm2_power(apply, n, steps=8, seed=0):
    """||H||_2 of a symmetric positive semi-definite operator by a few float64 power steps (only used as a scale)"""
    x = np.random.RandomState(seed).normal(size=n)
    lam = 0.0
    for _ in range(steps):
        x /= np.linalg.norm(x)
        y = np.asarray(apply(x), dtype=np.float64)
        lam = float(np.linalg.norm(y))
        x = y
    return lam


# ------------------------------------------------------------------------------------------------ the float64 pipeline
class Pipeline64:
    """what plain float64 numpy gives on the same inputs: scipy triangular solves, BLAS products, LAPACK Cholesky"""

    def __init__(self, cs, z, lin=None):
        from scipy.linalg import cho_factor, cho_solve, solve_triangular
        lin = lin or linearise(cs, z)
        Sb = np.concatenate([lin.dense(np.float64), lin.F.astype(np.float64)[:, None]], axis=1)
        for off, n, L in cs.groups:
            if L is not None:
                Sb[off:off + n] = solve_triangular(L, Sb[off:off + n], lower=True, check_finite=False)
        nz = cs.nz
        Hb = Sb.T @ Sb
        self.S, self.w = Sb[:, :nz], Sb[:, nz]
        self.H, self.g, self.loss = 2.0 * Hb[:nz, :nz], 2.0 * Hb[:nz, nz], float(Hb[nz, nz])
        self.chol = cho_factor(self.H, lower=True, check_finite=False)
        self.solve = lambda r: cho_solve(self.chol, r, check_finite=False)
        self.delta = self.solve(self.g)


# ------------------------------------------------------------------------------------------------ full form (N_d <= 129)
class FullReference:
    """S = L^-1 A, w = L^-1 F, H = 2 S^T S, g = 2 S^T w, loss = w^T w in long double; scaleH = 2 |S|^T |S|, scaleg = 2 |S|^T |w| (float64:
    they are scales); delta by float64 Cholesky of H + long-double refinement"""

    def __init__(self, cs, z):
        self.case, self.z = cs, np.array(z, dtype=np.float64)
        lin = self.lin = linearise(cs, z)
        nz = cs.nz
        Sb = _group_solve(cs, np.concatenate([lin.dense(), lin.F[:, None]], axis=1))
        self.S, self.w = Sb[:, :nz], Sb[:, nz]
        G = gram_lower(Sb)                                           # (nz + 1) x (nz + 1), long double, symmetric
        self.H = LD(2) * G[:nz, :nz]
        self.g = LD(2) * G[nz, :nz]
        self.loss = self.w @ self.w
        Sa = np.abs(Sb).astype(np.float64)
        self.scaleH = 2.0 * (Sa[:, :nz].T @ Sa[:, :nz])
        self.scaleg = 2.0 * (Sa[:, :nz].T @ Sa[:, nz])
        self.p64 = Pipeline64(cs, z, lin)
        self.delta = refine(self.p64.solve, lambda d: self.g - self.H @ d, self.g.astype(np.float64))
        H64 = self.H.astype(np.float64)
        ev = np.linalg.eigvalsh(H64)
        self.normH, self.cond = float(ev[-1]), float(ev[-1] / ev[0])


@functools.lru_cache(maxsize=None)
def full_reference(system, Nd):
    cs = case(system, Nd)
    return FullReference(cs, cs.z0)


# ------------------------------------------------------------------------------------------------ vector-only form
class VectorReference:
    """The step at z without L^-1 A: w = L^-1 F(z) and loss = w^T w; apply_H(d) = 2 A^T L^-T L^-1 A d; g = 2 A^T L^-T w;
    residual(d) = apply_H(d) - g = 2 A^T L^-T L^-1 (A d - F); delta by float64 Cholesky (Pipeline64) + refinement with these long-double
    residuals.  Two single-vector long-double solves per factor and product: O(N^2).
    lin_fn: the linearisation (default: linearise of this module; _semilinear_reference and _monge_ampere_reference pass their own)."""

    def __init__(self, cs, z, want_delta=True, lin_fn=None):
        self.case, self.z = cs, np.array(z, dtype=np.float64)
        lin = self.lin = (lin_fn or linearise)(cs, z)
        self.w = _group_solve(cs, lin.F)
        self.loss = self.w @ self.w
        self.g = LD(2) * lin.tmul(_group_solve(cs, self.w, trans=True))
        self.p64 = Pipeline64(cs, z, lin)
        self.normH = norm2_power(lambda x: self.p64.H @ x, cs.nz)
        self.delta = refine(self.p64.solve, lambda d: -self.residual(d), self.g.astype(np.float64)) if want_delta else None

    def apply_H(self, d):
        y = _group_solve(self.case, self.lin.mul(d))
        return LD(2) * self.lin.tmul(_group_solve(self.case, y, trans=True))

    def residual(self, d):
        y = _group_solve(self.case, self.lin.mul(d) - self.lin.F)
        return LD(2) * self.lin.tmul(_group_solve(self.case, y, trans=True))


@functools.lru_cache(maxsize=None)
def vector_reference(system, Nd):
    cs = case(system, Nd)
    return VectorReference(cs, cs.z0)


# ------------------------------------------------------------------------------------------------ the gates a device result has to pass
# Rounding budget of one entry of [A(z) | F(z)] (gn_build_kernel of csrc/gpk_gn.hip), relative to the sum of the magnitudes of its terms,
# in units of eps = 2^-52.  The expectation is long double, so all of it is the device's.  A correctly rounded operation (+ - * / and a
# fused multiply-add) costs eps / 2 of its result, which is at most the magnitude sum; the device's pow, exp and sqrt are taken at a
# maximum error of 1 ulp, i.e. <= eps of their value: the figure the HIP programming guide's table of double-precision device math
# functions gives for all three.  It is NOT measured here; tests/test_gpu_gn_rounding.py prints the worst ratio it observes, and the
# relaxed system (9/2 of 5) is where a less accurate pow would show first.  m - 1 is exact for the exponents used.
#   elliptic   A: alpha m pow(u, m-1): 1 + 2/2 = 2;            F: alpha pow(u, m) - f: 1 + 1/2 + 1/2 = 2
#   Burgers    A: -alpha v: 1/2;                               F: nu v3 + f - alpha v0 v2: five operations = 5/2
#   Eikonal    A: 2 v / eps: 1/2 (2 v is exact);               F: -(f f - v1 v1 - v2 v2) / eps: six operations = 3
#   Darcy      A: f exp(-w0): 1 + 1/2 = 3/2, 1 / gamma: 1/2;   F: -v1 w1 - v2 w2 - f exp(-w0): 3/2 on its largest term + 2/2 = 5/2;
#              (v0 - data) / gamma: 1
#   relaxed    rs = 1 / sqrt(lambda): 1 + 1/2 = 3/2;  A: alpha m pow(w, m-1) rs: 1 + 3/2 + 3/2 = 4;  -rs: 3/2;
#              F: (-v + alpha pow(w, m) - f) rs: (1 + 1/2) + 2/2 + 3/2 + 1/2 = 9/2
# The largest is 9/2; second-order terms are below 1e-15 of that.
C_BUILD = 5.0


def check_build(lin, A, F, what=''):
    """[A | F] as a kernel wrote it (A: rows x nz in the natural order of the unknowns, or None; F: rows) against the long-double
    entries: structural zeros, the constant entries and the plain copies exactly, every other entry within C_BUILD eps of the magnitude
    sum of its terms.  Returns the worst ratio (units of eps x magnitude); raises AssertionError."""
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
        assert np.all(lin.v[~k] != 0)
        # (every z-dependent entry of A(z) of the five systems is ONE product: the magnitude sum of its terms is |v| itself; an entry
        # with several terms would need a magnitude of its own, as F has in Fmag)
        ra = np.abs(got[~k].astype(LD) - lin.v[~k]) / (LD(EPS) * np.abs(lin.v[~k]))
        worst = float(np.max(ra)) if ra.size else 0.0
        assert worst <= C_BUILD, (what, 'A(z)', worst, int(lin.r[~k][np.argmax(ra)]), int(lin.c[~k][np.argmax(ra)]))
    F = np.asarray(F, dtype=np.float64)
    assert F.shape == (lin.rows,), (what, F.shape)
    assert np.array_equal(F[lin.Fcopy], lin.F[lin.Fcopy].astype(np.float64)), (what, 'a copied entry of F(z) is not exact')
    m = ~lin.Fcopy
    if m.any():
        rf = np.abs(F[m].astype(LD) - lin.F[m]) / (LD(EPS) * lin.Fmag[m])
        wf = float(np.max(rf))
        assert wf <= C_BUILD, (what, 'F(z)', wf, int(np.nonzero(m)[0][np.argmax(rf)]))
        worst = max(worst, wf)
    return worst


# Each gate returns (ratio, allowed): the measured figure in units of eps x its scale and the largest admissible one.  The constant is
# not fixed in advance: the same figure of the float64 numpy pipeline is computed at run time, and the device may take 32 x that plus
# one eps -- it sums in MFMA K-chunks and split-K order and solves through explicitly inverted diagonal blocks, whose error constant
# carries the condition of those blocks (tens, with these factors).
MARGIN = 32.0


def allowed(numpy_ratio):
    return MARGIN * numpy_ratio + 1.0


def ratio_entries(got, ref, scale):
    """max |got - ref| / (eps scale) over the entries (an entry with scale 0 must be exact)"""
    err = np.abs(np.asarray(got).astype(LD) - ref).astype(np.float64)
    scale = np.asarray(scale, dtype=np.float64)
    if np.any((scale == 0) & (err != 0)):
        return np.inf
    return float(np.max(err / (EPS * np.where(scale == 0, 1.0, scale))))


def gate_H(ref, H):
    return ratio_entries(H, ref.H, ref.scaleH), allowed(ratio_entries(ref.p64.H, ref.H, ref.scaleH))


def gate_g(ref, g):
    return ratio_entries(g, ref.g, ref.scaleg), allowed(ratio_entries(ref.p64.g, ref.g, ref.scaleg))


def gate_loss(ref, loss):
    """|loss - loss_ld| / (eps sum |terms|): the terms are the squares w_i^2, their magnitude sum is the loss itself.  A single number's
    rounding error can vanish by cancellation, so the numpy figure counts as at least one eps."""
    r = lambda v: float(abs(LD(v) - ref.loss) / (LD(EPS) * ref.loss))
    return r(loss), allowed(max(r(ref.p64.loss), 1.0))


def gate_backward(ref, delta, Hmul=None):
    """||H_ld delta - g_ld|| / (eps (||H|| ||delta|| + ||g||))"""
    Hmul = Hmul or (lambda d: ref.H @ d)
    gn = float(np.linalg.norm(ref.g.astype(np.float64)))

    def r(d):
        res = (Hmul(np.asarray(d).astype(LD)) - ref.g).astype(np.float64)
        return float(np.linalg.norm(res) / (EPS * (ref.normH * np.linalg.norm(d) + gn)))
    return r(delta), allowed(r(ref.p64.delta))


def gate_backward_vec(ref, delta):
    return gate_backward(ref, delta, ref.apply_H)


def gate_forward(ref, delta):
    """||delta - delta_ld|| / (eps ||delta_ld||)"""
    dn = np.linalg.norm(ref.delta.astype(np.float64))
    r = lambda d: float(np.linalg.norm((np.asarray(d).astype(LD) - ref.delta).astype(np.float64)) / (EPS * dn))
    return r(delta), allowed(r(ref.p64.delta))


def gate_update(z_in, step, delta, z_out):
    """(ratio, allowed) of the update of z: update_ratio against one rounding of each term"""
    return update_ratio(z_in, step, delta, z_out), 1.0


def update_ratio(z_in, step, delta, z_out):
    """max |z_out - (z_in - step delta)| / (eps (|z_in| + |step delta|)) with the right-hand side in long double: <= 1 when the update is
    the one rounding of the product and the one of the sum (or the single one of a fused multiply-add)"""
    sd = LD(step) * np.asarray(delta).astype(LD)
    want = np.asarray(z_in).astype(LD) - sd
    err = np.abs(np.asarray(z_out).astype(LD) - want)
    return float(np.max(err / (LD(EPS) * (np.abs(np.asarray(z_in).astype(LD)) + np.abs(sd)))))
