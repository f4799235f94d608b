"""Reference of the joint posterior covariance between test points in the Gauss-Newton (Laplace) form (CPU only).

With the notation of tests/_posterior_reference.py (P = L^-1 A, L_H L_H^T = H/2 = P^T P, f the row group of the field) and k_s the
covariances of the field at the test point x_s with that group's functionals,

    Sigma[s, t] = k(x_s, x_t) - (L_f^-1 k_s)^T (L_f^-1 k_t)  +  (L_H^-1 P_f^T L_f^-1 k_s)^T (L_H^-1 P_f^T L_f^-1 k_t)
                  `---------------- Sigma_cond ------------'     `------------------- Sigma_gn ----------------------'

whose diagonal is var_cond + var_gn of variance_ld.

  prior_ld          k(xa_i, xb_j) in long double from the kernel formulas of tests/_gauss_reference.py / tests/_matern_reference.py
  covariance_ld     the formula in long double (the factors, P and L_H of _posterior_reference.prepare_ld)
  covariance_np64   the same as the float64 numpy / scipy pipeline the device is judged against

Both return a CovResult: cond, gn (nt x nt) and the entrywise scale S_st = |Ktt_st| + sum_r |V_rs V_rt| + sum_r |W_rs W_rt| of their
rounding errors.
"""
import numpy as np

import _gn_reference as R
import _posterior_reference as PR

LD = R.LD
MATERN = ('Matern52', 'Matern72', 'Matern92')


def prior_ld(kernel, kp, Xa, Xb=None):
    """(na, nb) long double: k(xa_i, xb_j), the value functional on both sides (Xb=None: Xa against itself)"""
    Xa = np.asarray(Xa, dtype=np.float64).reshape(-1, 2)
    Xb = Xa if Xb is None else np.asarray(Xb, dtype=np.float64).reshape(-1, 2)
    x1, x2, y1, y2 = Xa[:, None, 0], Xa[:, None, 1], Xb[None, :, 0], Xb[None, :, 1]
    if kernel in MATERN:
        import _matern_reference as MR
        return MR.pair(kernel, MR.ID, MR.ID, x1, x2, y1, y2, kp)
    import _gauss_reference as GR
    return GR.pair(kernel, kp, GR.ID, GR.ID, x1, x2, y1, y2)


class CovResult:
    def __init__(self, cond, gn, scale_cond, scale):
        self.cond, self.gn, self.scale_cond, self.scale = cond, gn, scale_cond, scale

    @property
    def cov(self):
        return self.cond + self.gn


def _absgram(V):
    """sum_r |V_rs| |V_rt|, in the precision of V"""
    A = np.abs(V)
    return R.gram_lower(A) if V.dtype == LD else A.T @ A


def covariance_ld(cs, z, K, Ktt, field=0, factors_ld=None, prepared=None):
    """long double.  K: (rows of the field's group, nt) float64; Ktt: (nt, nt) prior (float64 or long double).  factors_ld, prepared:
    as _posterior_reference.variance_ld"""
    get = lambda L: L.astype(LD) if factors_ld is None else factors_ld[id(L)]
    P, LH = prepared if prepared is not None else PR.prepare_ld(cs, z, factors_ld)
    off, n, L = PR.field_group(cs, field)
    Ktt = np.asarray(Ktt).astype(LD)
    V = R.solve_lower(get(L), np.asarray(K, dtype=np.float64).astype(LD))
    W = R.solve_lower(LH, P[off:off + n].T @ V)
    sc = np.abs(Ktt) + _absgram(V)
    return CovResult(Ktt - R.gram_lower(V), R.gram_lower(W), sc, sc + _absgram(W))


def covariance_np64(cs, z, K, Ktt, field=0, factors64=None):
    """the float64 numpy / scipy pipeline on the same inputs (factors64: as _posterior_reference.variance_np64)"""
    from scipy.linalg import solve_triangular
    lin = R.linearise(cs, z)
    get = lambda L: L if factors64 is None else factors64[id(L)]
    P = lin.dense(np.float64)
    for off, n, L in cs.groups:
        if L is not None and n:
            P[off:off + n] = solve_triangular(get(L), P[off:off + n], lower=True, check_finite=False)
    LH = np.linalg.cholesky(P.T @ P)
    off, n, L = PR.field_group(cs, field)
    Ktt = np.asarray(Ktt, dtype=np.float64)
    V = solve_triangular(get(L), np.asarray(K, dtype=np.float64), lower=True, check_finite=False)
    W = solve_triangular(LH, P[off:off + n].T @ V, lower=True, check_finite=False)
    sc = np.abs(Ktt) + _absgram(V)
    return CovResult(Ktt - V.T @ V, W.T @ W, sc, sc + _absgram(W))
