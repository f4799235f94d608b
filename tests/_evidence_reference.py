"""Reference of the Laplace log evidence at a Gauss-Newton iterate (CPU only).

For a system with measurement vector F(z) (rows), Jacobian A = dF/dz at z, factors L_k L_k^T = Theta_k of its row groups,
J(z) = sum_k ||L_k^-1 F_k(z)||^2 + ||rows of F without a factor||^2 (Darcy: (v0 - data) / gamma) and H/2 = A^T Theta^-1 A = R R^T,

    log Z = -J/2 - sum_k log|Theta_k| / 2 - log|H/2| / 2 - N_data log gamma - (rows - n_z)/2 log 2 pi
            log|Theta_k| = 2 sum_i log (L_k)_ii,   log|H/2| = 2 sum_i log R_ii.

When F is affine in z (the elliptic system with alpha = 0: F = [-f; z; g]) the formula is exact and equal, whatever z, to the Gaussian
log likelihood of the data rows d = [-f; g] under their own block Theta_dd, because |Theta| |A^T Theta^-1 A| = |Theta_dd| and
min_z F^T Theta^-1 F = d^T Theta_dd^-1 d is reached after one Gauss-Newton step.

  terms_ld      the six terms in long double (Cholesky and substitution of tests/_posterior_reference.py), with the magnitude sums
                that scale their rounding errors
  terms_np64    the same as the float64 pipeline the device is judged against: LAPACK Cholesky, scipy solve_triangular, BLAS
                products, np.sum(np.log(diag))
  gaussian_loglik_ld / _np64   log N(d; 0, T), the other side of the affine identity

Both terms_* return a Terms: .value[name] for name in TERMS and .scale[name], the sum of the magnitudes of the summands of that term
(for log_Z: of the five terms as they enter it).
"""
import numpy as np

import _gn_reference as R
import _posterior_reference as PR

LD = R.LD
TERMS = ('log_Z', 'J', 'logdet_theta', 'logdet_H', 'gamma_term', 'two_pi_term')   # the order of gpk_log_evidence's host_terms
LOG_2PI_LD = np.log(LD(8) * np.arctan(LD(1)))


class Terms:
    def __init__(self, J, Jscale, ldt, ldt_scale, ldh, ldh_scale, gam, tpi):
        self.value = {'J': J, 'logdet_theta': ldt, 'logdet_H': ldh, 'gamma_term': gam, 'two_pi_term': tpi,
                      'log_Z': -(J + ldt + ldh) / 2 - gam - tpi}
        self.scale = {'J': Jscale, 'logdet_theta': ldt_scale, 'logdet_H': ldh_scale, 'gamma_term': abs(gam), 'two_pi_term': abs(tpi),
                      'log_Z': (abs(J) + abs(ldt) + abs(ldh)) / 2 + abs(gam) + abs(tpi)}


def logdet_factor(L, dtype=LD):
    """(log |L L^T|, sum of the magnitudes of its summands) from the diagonal of the lower factor"""
    t = dtype(2) * np.log(np.diag(np.asarray(L)).astype(dtype))
    return np.sum(t), np.sum(np.abs(t))


def _constants(cs, dtype):
    gam = dtype(cs.Ndata) * np.log(dtype(cs.p0)) if cs.system == 'darcy' and cs.Ndata else dtype(0)
    tpi = dtype(cs.rows - cs.nz) / dtype(2) * (LOG_2PI_LD if dtype is LD else dtype(np.log(2.0 * np.pi)))
    return gam, tpi


def terms_ld(cs, z, factors_ld=None, prepared=None):
    """long double.  factors_ld / prepared: as tests/_posterior_reference.variance_ld takes them"""
    get = lambda L: L.astype(LD) if factors_ld is None else factors_ld[id(L)]
    _, LH = prepared if prepared is not None else PR.prepare_ld(cs, z, factors_ld)
    w = np.array(R.linearise(cs, z).F, dtype=LD)
    ldt = ldt_scale = LD(0)
    for off, n, L in cs.groups:
        if L is not None and n:
            w[off:off + n] = R.solve_lower(get(L), w[off:off + n])
            v, s = logdet_factor(get(L))
            ldt, ldt_scale = ldt + v, ldt_scale + s
    J = w @ w
    ldh, ldh_scale = logdet_factor(LH)
    return Terms(J, J, ldt, ldt_scale, ldh, ldh_scale, *_constants(cs, LD))


def terms_np64(cs, z, factors64=None):
    """the float64 numpy / scipy pipeline on the same inputs"""
    from scipy.linalg import solve_triangular
    get = lambda L: L if factors64 is None else factors64[id(L)]
    lin = R.linearise(cs, z)
    P, w = lin.dense(np.float64), lin.F.astype(np.float64)
    ldt = ldt_scale = 0.0
    for off, n, L in cs.groups:
        if L is not None and n:
            P[off:off + n] = solve_triangular(get(L), P[off:off + n], lower=True, check_finite=False)
            w[off:off + n] = solve_triangular(get(L), w[off:off + n], lower=True, check_finite=False)
            v, s = logdet_factor(get(L), np.float64)
            ldt, ldt_scale = ldt + v, ldt_scale + s
    J = float(w @ w)
    ldh, ldh_scale = logdet_factor(np.linalg.cholesky(P.T @ P), np.float64)
    return Terms(J, J, ldt, ldt_scale, ldh, ldh_scale, *_constants(cs, np.float64))


def term_ratio(name, got, ref):
    """|got - ref| / (eps x the magnitude sum of the term) against the long-double Terms `ref`; a term that is exactly zero (no gamma
    term outside Darcy) must be exact"""
    err, scale = abs(LD(got) - ref.value[name]), ref.scale[name]
    if scale == 0:
        return 0.0 if err == 0 else np.inf
    return float(err / (LD(R.EPS) * scale))


def allowed_scalar(numpy_ratio):
    """the gate of ONE number: R.allowed, with the numpy figure counted as at least one eps -- a single number's rounding error can
    vanish by cancellation (as _gn_reference.gate_loss)"""
    return R.allowed(max(numpy_ratio, 1.0))


# ------------------------------------------------------------------------------------------------ the affine identity
def elliptic_data_rows(Nd, Nb):
    """rows of F = [tau(z) - f; z; g] that hold data: the PDE rows and the boundary rows"""
    return np.concatenate([np.arange(Nd), 2 * Nd + np.arange(Nb)])


def gaussian_loglik_ld(T, d):
    """log N(d; 0, T) in long double (T float64, symmetric positive definite)"""
    L = PR.cholesky_ld(T)
    w = R.solve_lower(L, np.asarray(d, dtype=np.float64).astype(LD))
    return -(w @ w) / LD(2) - np.sum(np.log(np.diag(L))) - LD(len(w)) / LD(2) * LOG_2PI_LD


def gaussian_loglik_np64(T, d):
    from scipy.linalg import solve_triangular
    L = np.linalg.cholesky(T)
    w = solve_triangular(L, np.asarray(d, dtype=np.float64), lower=True, check_finite=False)
    return float(-(w @ w) / 2.0 - np.sum(np.log(np.diag(L))) - len(w) / 2.0 * np.log(2.0 * np.pi))


def elliptic_case(Nd, Nb, f, g, Theta, alpha=0.0, m=3.0):
    """the elliptic problem on a real Gram matrix in the shape terms_* take"""
    return PR.RealCase('elliptic', Nd, Nb, f, g, alpha, m, Theta)
