"""Reference of the posterior variance in the Gauss-Newton (Laplace) form (CPU only).

For a system with measurement vector F(z), Jacobian A = dF/dz at the iterate z and factors L_k L_k^T = Theta_k of its row groups,

    H/2      = A^T Theta^-1 A = P^T P,   P = L^-1 A  (every row group with its own factor, rows without a factor as they are)
    var(x)   = 1 - ||L_f^-1 k_x||^2  +  ||L_H^-1 P_f^T L_f^-1 k_x||^2,    L_H L_H^T = H/2
               `---- var_cond ----'     `------------ var_gn ------------'

with f the row group of the field u (or a, Darcy) and k_x the covariances of the field at x with that group's functionals.

  variance_ld     the formula in long double: an unblocked Cholesky of its own (cholesky_ld; numpy has none in long double) and the
                  row-wise substitution of _gn_reference.solve_lower
  variance_np64   the same as the float64 pipeline the device is judged against: LAPACK Cholesky, scipy solve_triangular, BLAS products
  RealCase        a problem on a real Gram matrix in the shape _gn_reference.linearise takes (A(z) of every system in long double)

Both return a Result: var_cond, var_gn (nt,), and the sums sv = sum V^2, sw = sum W^2 that scale their rounding errors.
"""
import numpy as np

import _gn_reference as R

LD = R.LD


def cholesky_ld(A):
    """lower Cholesky factor in long double, unblocked, column by column (one vectorised update per column); reads the lower triangle
    only; raises on a non-positive pivot"""
    A = np.asarray(A, dtype=LD)
    n = A.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0:
            raise np.linalg.LinAlgError(f'non-positive pivot {float(d):.3e} at column {j}')
        L[j, j] = np.sqrt(d)
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


class Result:
    def __init__(self, var_cond, var_gn, sv, sw, P=None, LH=None):
        self.var_cond, self.var_gn, self.sv, self.sw, self.P, self.LH = var_cond, var_gn, sv, sw, P, LH

    @property
    def var(self):
        return self.var_cond + self.var_gn


def field_group(cs, field):
    """(offset, rows, factor) of the row group of field 0 = u / 1 = a in the stacked layout of the library"""
    if cs.system == 'darcy':
        return cs.groups[1 - field]
    assert field == 0
    return cs.groups[0]


def prepare_ld(cs, z, factors_ld=None):
    """(P, L_H) in long double: what does not depend on the test points"""
    get = lambda L: L.astype(LD) if factors_ld is None else factors_ld[id(L)]
    P = np.array(R.linearise(cs, z).dense(), dtype=LD)
    for off, n, L in cs.groups:
        if L is not None and n:
            P[off:off + n] = R.solve_lower(get(L), P[off:off + n])
    return P, cholesky_ld(R.gram_lower(P))


def variance_ld(cs, z, K, field=0, factors_ld=None, prepared=None):
    """long double.  K: (rows of the field's group, nt) float64.  factors_ld: {id(L): long-double factor} to use instead of the
    float64 factors of cs.groups (real Gram matrices: the factor of the float64 Theta in long double).  prepared: prepare_ld's
    result for the same cs, z, factors_ld (shared between calls)"""
    get = lambda L: L.astype(LD) if factors_ld is None else factors_ld[id(L)]
    P, LH = prepared if prepared is not None else prepare_ld(cs, z, factors_ld)
    off, n, L = field_group(cs, field)
    V = R.solve_lower(get(L), np.asarray(K, dtype=np.float64).astype(LD))
    sv = np.sum(V * V, axis=0)
    W = R.solve_lower(LH, P[off:off + n].T @ V)
    sw = np.sum(W * W, axis=0)
    return Result(LD(1) - sv, sw, sv, sw, P, LH)


def variance_np64(cs, z, K, field=0, factors64=None):
    """the float64 numpy / scipy pipeline on the same inputs.  factors64: {id(L): float64 factor} (default: the factors of cs.groups)"""
    from scipy.linalg import solve_triangular
    lin = R.linearise(cs, z)
    get = lambda L: L if factors64 is None else factors64[id(L)]
    P = lin.dense(np.float64)
    for off, n, L in cs.groups:
        if L is not None and n:
            P[off:off + n] = solve_triangular(get(L), P[off:off + n], lower=True, check_finite=False)
    LH = np.linalg.cholesky(P.T @ P)
    off, n, L = field_group(cs, field)
    V = solve_triangular(get(L), np.asarray(K, dtype=np.float64), lower=True, check_finite=False)
    sv = np.sum(V * V, axis=0)
    W = solve_triangular(LH, P[off:off + n].T @ V, lower=True, check_finite=False)
    sw = np.sum(W * W, axis=0)
    return Result(1.0 - sv, sw, sv, sw, P, LH)


class RealCase:
    """A problem on real Gram matrices in the shape of _gn_reference.Case: system in R.SYSTEMS (not 'relaxed'), the right-hand sides, and
    the row groups with the float64 matrices Theta_k in the factor's place (self.thetas; the factors are made by factors())."""

    def __init__(self, system, Nd, Nb, f, g, p0, p1, Theta, Theta_a=None, data=None):
        self.system, self.Nd, self.Nb = system, Nd, Nb
        self.f, self.g = np.asarray(f, dtype=np.float64), np.asarray(g, dtype=np.float64)
        self.p0, self.p1, self.lam = p0, p1, 0.0
        self.data = None if data is None else np.asarray(data, dtype=np.float64)
        self.Ndata = 0 if data is None else self.data.size
        self.nz = R.n_unknowns(system, Nd)
        n = Theta.shape[0]
        self.L = Theta                     # (placeholders with the identity of the groups; never used as factors)
        self.L2 = Theta_a
        if system == 'darcy':
            self.groups = [(0, 3 * Nd, Theta_a), (3 * Nd, n, Theta), (3 * Nd + n, self.Ndata, None)]
        else:
            self.groups = [(0, n, Theta)]
        self.rows = sum(gr[1] for gr in self.groups)

    def factors(self):
        """({id: long-double factor}, {id: float64 LAPACK factor}) of the Gram matrices of the groups"""
        ld, f64 = {}, {}
        for _, _, T in self.groups:
            if T is not None:
                ld[id(T)] = cholesky_ld(T)
                f64[id(T)] = np.linalg.cholesky(T)
        return ld, f64
