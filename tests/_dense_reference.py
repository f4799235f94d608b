"""Componentwise backward-error gates of the dense factorisation and solves, on the matrices the product meets (CPU only).

Cholesky and substitution are componentwise backward stable (Higham, Accuracy and Stability of Numerical Algorithms, Thms 10.3 and 8.5):
the computed factor satisfies |L L^T - A| <= c eps |L||L^T| and a computed solution |L X - B| <= c eps |L||X|, ENTRY BY ENTRY, whatever
the scaling of the rows.  A norm-wise residual (||L L^T - A||_F <= 1e-13 ||A||_F, ||L X - B||_F <= 1e-12 ||L||_F ||X||_F) cannot see a
row whose entries are 1e-6 of the largest one; the blocks of one Theta have diagonals from 1 to 1.9e6.  This module provides

  families    gram (Theta with the adaptive nugget from tests/_gauss_reference.py, condition 1e10 .. 1e15), graded (D (M M^T + n I) D,
              D = diag(10^U(-3, 3))), graded_factor (D (tril(normal) + diag(U(3, 4) sqrt n))) and right-hand sides with scaled columns,
              one row block of small entries and, on request, the leading-zero profile of [A | F]; all deterministic and cached
  residuals   in numpy long double (eps 1.1e-19), each with the scale |L||L^T|, |L||X|, ... of its bound; only the lower triangle of L
              is read
  the gate    err_ij <= c eps scale_ij as an INEQUALITY for every entry (Theta has exact zeros: no quotient is formed where the scale
              vanishes, and an entry whose scale is 0 has to be reproduced as exactly 0); worst() reports max err / (eps scale)
  yardsticks  the same figure of the float64 host rendition of the operation (numpy.linalg.cholesky, scipy.linalg.solve_triangular,
              numpy's @; for the inverted-block solve the same algorithm in numpy).  c is never fixed in advance: the device may take
              _gn_reference.allowed(numpy figure) = 32 x numpy + 1, the margin of the Gauss-Newton step tests (a different but equally
              valid order of summation).  tests/test_dense_reference_host.py asserts that the numpy figure is at most CAP = 64 for every
              case handed out here, so no gate exceeds about 2000 eps.

The forward error L - L_ref is NOT gated on these families: it is governed by the conditioning.
Host-only: nothing here imports the GPU package.
"""
import functools
import zlib

import numpy as np
import scipy.linalg as sla

import _gauss_reference as G
import _gn_reference as R

LD, EPS = R.LD, R.EPS
allowed, poisoned, LD_PAD = R.allowed, R.poisoned, R.LD_PAD
CAP = 64.0                                        # the numpy figure of every case (asserted by the host test)
NB, SB, OB = 64, 256, 512                         # panels, strips, outer blocks of csrc/gpk_factor.hip

# (layout, N_d, N_b) -> orders 460, 520, 480, 450 and 577 (> 512: the right-looking factorisation has a trailing update)
GRAM_CASES = (('Nonlinear_elliptic', 200, 60), ('Burgers', 120, 40), ('Eikonal', 110, 40), ('Darcy_a', 150, 40), ('Nonlinear_elliptic', 250, 77))
GRAM_KERNEL = {'Burgers': 'anisotropic_Gaussian'}
# 1e-12 is excluded: the smallest relative pivot min_i l_ii^2 / a_ii is then only about 10 n eps, where a correct float64 factorisation
# may legitimately meet a non-positive pivot; at 1e-10 it is about 1000 n eps
NUGGETS = (1e-8, 1e-10)
PIVOT_MARGIN = 100.0                              # precondition of every gram case: min_i l_ii^2 / a_ii >= 100 n eps
GRADED_ORDERS = (1, 63, 64, 65, 129, 256, 320, 513, 576, 645)
# 64: base kernel; 240, 256: strip kernel (n <= 256, n % 16 == 0); 250: base kernel + recursion; 520: recursion over strips
FACTOR_ORDERS = (64, 240, 250, 256, 520)
DINV_BLOCK = 256
DINV_ORDERS = (256, 300, 520, 577)                # one block, a ragged second block, three blocks with a ragged last one (twice)
NRHS = (1, 37, 130)


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def ld(a):
    return np.asarray(a, dtype=LD)


def mm(A, B):
    """A B in long double (einsum over contiguous rows: several times faster than matmul for this type)"""
    A, B = ld(A), ld(B)
    if A.shape[1] == 0:
        return np.zeros((A.shape[0], B.shape[1]), dtype=LD)
    return np.einsum('ik,jk->ij', np.ascontiguousarray(A), np.ascontiguousarray(B.T))


def lower(L):
    """the n x n lower triangle of a stored factor (n rows; padding columns and the strict upper triangle are dropped unread)"""
    L = np.asarray(L)
    n = L.shape[0]
    return np.where(np.tri(n, dtype=bool), L[:, :n], 0.0)


def scales(n, rng):
    return 10.0 ** rng.uniform(-3, 3, n)


# ---------------------------------------------------------------------------------------------------------------- families
def cholesky_ld(A, block=64):
    """lower Cholesky factor in long double, blocked left-looking; reads the lower triangle only; a non-positive pivot gives NaN"""
    A = ld(A)
    n = A.shape[0]
    L = np.zeros((n, n), dtype=LD)
    with np.errstate(invalid='ignore'):
        for j0 in range(0, n, block):
            j1 = min(j0 + block, n)
            P = A[j0:, j0:j1] - mm(L[j0:, :j0], L[j0:j1, :j0].T)
            for j in range(j1 - j0):
                P[j, j] = np.sqrt(P[j, j] - P[j, :j] @ P[j, :j])
                P[j + 1:, j] = (P[j + 1:, j] - P[j + 1:, :j] @ P[j, :j]) / P[j, j]
                P[j, j + 1:] = 0
            L[j0:, j0:j1] = P
    return L


def relative_pivot(A, L):
    """min_i l_ii^2 / a_ii: how far the factorisation is from a non-positive pivot"""
    return float(np.min(ld(np.diag(L)) ** 2 / ld(np.diag(A))))


def _symmetric(T):
    T = np.tril(T)
    return T + np.tril(T, -1).T


@functools.lru_cache(maxsize=None)
def _theta(layout, Nd, Nb):
    Xd, Xb, _ = G.case_points(Nd, Nb)
    kernel = GRAM_KERNEL.get(layout, 'Gaussian')
    return kernel, Xd, Xb, G.theta(kernel, G.PARAMS[kernel], layout, Xd, Xb)


@functools.lru_cache(maxsize=None)
def gram(layout, Nd, Nb, nugget):
    """Theta + adaptive nugget of the layout at _gauss_reference.case_points(Nd, Nb), rounded to float64, symmetric from its lower
    triangle.  Asserts the pivot precondition on the long-double factor."""
    kernel, Xd, Xb, base = _theta(layout, Nd, Nb)
    T = G.theta_nugget(kernel, G.PARAMS[kernel], layout, Xd, Xb, nugget, 'adaptive', base=base)
    A = _symmetric(T.astype(np.float64))
    n = A.shape[0]
    piv = relative_pivot(A, cholesky_ld(A))
    assert piv >= PIVOT_MARGIN * n * EPS, (layout, Nd, Nb, nugget, piv, PIVOT_MARGIN * n * EPS)
    A.setflags(write=False)
    return A


def gram_cases():
    return [c + (nug,) for c in GRAM_CASES for nug in NUGGETS]


def gram_id(c):
    return f'{c[0]}-{c[1]}-{c[2]}-{c[3]:g}'


@functools.lru_cache(maxsize=None)
def graded(n, seed=0):
    """D (M M^T + n I) D with D = diag(10^U(-3, 3)): well conditioned after scaling, rows of very different size"""
    rng = np.random.RandomState(_seed('graded', n, seed))
    M = rng.normal(size=(n, n))
    d = scales(n, rng)
    A = _symmetric(d[:, None] * (M @ M.T + n * np.eye(n)) * d[None, :])
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def graded_factor(n, seed=0):
    """D (tril(normal) + diag(U(3, 4) sqrt n)); upload it through poisoned()"""
    rng = np.random.RandomState(_seed('factor', n, seed))
    L = scales(n, rng)[:, None] * R.synthetic_factor(rng, n)
    L.setflags(write=False)
    return L


def lead_mask(n, nrhs, lead):
    """True where the leading-zero profile of [A | F] promises a zero: column c < lead above row lead - 1 - c"""
    rows, cols = np.arange(n)[:, None], np.arange(nrhs)[None, :]
    return (cols < lead) & (rows < lead - 1 - cols)


@functools.lru_cache(maxsize=None)
def rhs(n, nrhs, lead=0, seed=0):
    """normal entries, columns scaled by 10^U(-3, 3), the rows [n / 3, n / 3 + n / 8] scaled by 1e-6; lead > 0: the zeros of lead_mask"""
    rng = np.random.RandomState(_seed('rhs', n, nrhs, lead, seed))
    B = rng.normal(size=(n, nrhs)) * scales(nrhs, rng)[None, :]
    B[n // 3:n // 3 + n // 8 + 1] *= 1e-6
    if lead > 0:
        B[lead_mask(n, nrhs, lead)] = 0.0
    B.setflags(write=False)
    return B


# --------------------------------------------------------------------------------------------------- residuals and scales
def res_cholesky(L, A, rows=None):
    """(|L L^T - A|, |L||L^T|) on the lower triangle (zeros above it); rows: only these rows (a full product is out of reach at
    large orders), returned as (len(rows), n)"""
    L = ld(lower(L))
    n = L.shape[0]
    idx = np.arange(n) if rows is None else np.asarray(rows)
    keep = np.arange(n)[None, :] <= idx[:, None]
    err = np.abs(mm(L[idx], L.T) - ld(A)[idx][:, :n])
    scale = mm(np.abs(L[idx]), np.abs(L.T))
    return np.where(keep, err, 0), np.where(keep, scale, 0)


def res_solve(kind, L, X, B):
    """kind 'N': L X - B against |L||X|;  'T': L^T X - B against |L^T||X|;  'R': X L^T - B against |X||L^T|;
    'P': L L^T X - B against |L|(|L^T||X|) + |L||Y|, Y = L^T X (two substitutions: the errors of both steps)"""
    L = ld(lower(L))
    aL = np.abs(L)
    X, B = ld(X), ld(B)
    if X.ndim == 1:
        X, B = X[:, None], B[:, None]
    aX = np.abs(X)
    if kind == 'N':
        return np.abs(mm(L, X) - B), mm(aL, aX)
    if kind == 'T':
        return np.abs(mm(L.T, X) - B), mm(aL.T, aX)
    if kind == 'R':
        return np.abs(mm(X, L.T) - B), mm(aX, aL.T)
    if kind == 'P':
        Y = mm(L.T, X)
        return np.abs(mm(L, Y) - B), mm(aL, mm(aL.T, aX)) + mm(aL, np.abs(Y))
    raise ValueError(kind)


def res_product(opA, opB, alpha, beta, C0, got):
    """(|got - (alpha opA opB + beta C0)|, |alpha||opA||opB| + |beta C0|)"""
    want = LD(alpha) * mm(opA, opB)
    scale = abs(LD(alpha)) * mm(np.abs(opA), np.abs(opB))
    if beta != 0.0:
        want = want + LD(beta) * ld(C0)
        scale = scale + np.abs(LD(beta) * ld(C0))
    return np.abs(ld(got) - want), scale


# ---------------------------------------------------------------------------------------------------------------- products
PRODUCT_SHAPES = ((257, 193, 100), (130, 70, 577))       # edge tiles in m and n with a partial K slab; a long K with a partial last slab


@functools.lru_cache(maxsize=None)
def product_cases(m, n, k):
    """The calls of the product test at one shape, as dicts: entry ('gemm' | 'gemm_lz' | 'syrk'), the operands as stored (A, B, C0), the
    scalars, and opA (m x k), opB (k x n).  Rows of op(A), columns of op(B) and rows and columns of C are scaled by 10^U(-3, 3), so that
    entry (i, j) of the result has its own size.  gemm_lz: B has the leading-zero profile `lead`; at the first shape lead > k, so
    the columns c < lead - k of B are zero throughout: with beta = 0 those columns of C have scale 0 and must come out as exact zeros."""
    rng = np.random.RandomState(_seed('product', m, n, k))
    dr, dc = scales(m, rng), scales(n, rng)
    out = []

    def operands(lead=0):
        opA = dr[:, None] * rng.normal(size=(m, k))
        opB = rng.normal(size=(k, n)) * dc[None, :]
        if lead:
            opB[lead_mask(k, n, lead)] = 0.0
        return opA, opB, dr[:, None] * rng.normal(size=(m, n)) * dc[None, :]

    for ta, tb, alpha, beta in ((0, 0, 1.7, -0.3), (0, 1, 1.7, -0.3), (1, 0, 1.7, -0.3), (1, 1, 1.7, -0.3), (0, 1, -1.0, 1.0), (1, 0, 1.7, 0.0)):
        opA, opB, C0 = operands()
        out.append(dict(name=f'gemm ta={ta} tb={tb} alpha={alpha} beta={beta}', entry='gemm', ta=ta, tb=tb, alpha=alpha, beta=beta,
                        A=np.ascontiguousarray(opA.T) if ta else opA, B=np.ascontiguousarray(opB.T) if tb else opB, C0=C0, opA=opA, opB=opB))
    lead = min(n - 1, k + 50)
    for ta, beta in ((0, 0.0), (1, 1.0), (0, 1.0), (1, 0.0)):
        opA, opB, C0 = operands(lead)
        out.append(dict(name=f'gemm_lz ta={ta} lead={lead} beta={beta}', entry='gemm_lz', ta=ta, tb=0, alpha=-1.0, beta=beta, lead=lead,
                        A=np.ascontiguousarray(opA.T) if ta else opA, B=opB, C0=C0, opA=opA, opB=opB))
    for full in (0, 1):                                                # C <- alpha A^T A + beta C, A is k x m, C is m x m
        A = rng.normal(size=(k, m)) * dr[None, :]
        C0 = _symmetric(dr[:, None] * rng.normal(size=(m, m)) * dr[None, :])       # symmetric: full = 1 mirrors the lower triangle
        out.append(dict(name=f'syrk full={full}', entry='syrk', alpha=0.7, beta=-1.3, full=full, A=A, C0=C0, opA=np.ascontiguousarray(A.T), opB=A))
    return out


def np_product(case):
    out = case['alpha'] * (case['opA'] @ case['opB'])
    return out + case['beta'] * case['C0'] if case['beta'] != 0.0 else out


# ------------------------------------------------------------------------------------------------------------- the gate
def check(err, scale, c):
    """err_ij <= c eps scale_ij for every entry -- an inequality, no quotient: an entry whose scale is 0 has to be exact, a NaN fails"""
    return bool(np.all(err <= LD(c) * LD(EPS) * scale))


def worst(err, scale):
    """max err / (eps scale) over the entries with a scale; inf if an entry without one is not exact or if anything is NaN"""
    err, scale = ld(err), ld(scale)
    if err.size == 0:
        return 0.0
    if np.isnan(err).any() or np.isnan(scale).any() or np.any((scale == 0) & (err != 0)):
        return float('inf')
    has = scale > 0
    if not has.any():
        return 0.0
    return float(np.max(err[has] / (LD(EPS) * scale[has])))


def gate(dev, numpy_ratio, zeros=None):
    """dev: (err, scale) of the device result; numpy_ratio: worst(err, scale) of the float64 host rendition of the same operation.
    zeros: the entries of the device result that the structure promises to be zero (an array of them): each has to be exactly 0.
    Returns (device ratio, allowed ratio, every entry within the allowed ratio)."""
    a = allowed(numpy_ratio)
    ok = check(dev[0], dev[1], a)
    r = worst(*dev)
    if zeros is not None and np.any(np.asarray(zeros) != 0.0):
        ok, r = False, float('inf')
    return r, a, ok


# ------------------------------------------------------------------------------------------------------- host renditions
def np_cholesky(A):
    return np.linalg.cholesky(np.asarray(A))


def np_solve(kind, L, B):
    L = lower(L)
    B = np.asarray(B)
    if kind == 'N':
        return sla.solve_triangular(L, B, lower=True, trans=0)
    if kind == 'T':
        return sla.solve_triangular(L, B, lower=True, trans=1)
    if kind == 'R':
        return sla.solve_triangular(L, B.T, lower=True, trans=0).T
    if kind == 'P':
        return sla.solve_triangular(L, sla.solve_triangular(L, B, lower=True, trans=0), lower=True, trans=1)
    raise ValueError(kind)


def np_trtri_diag(L, block=DINV_BLOCK):
    """(n, block): the inverse of diagonal block k in rows [k block, k block + n_k), columns [0, n_k), by substitution on the identity;
    zeros elsewhere -- the layout of gpk_trtri_diag"""
    L = lower(L)
    n = L.shape[0]
    D = np.zeros((n, block))
    for k0 in range(0, n, block):
        nk = min(block, n - k0)
        D[k0:k0 + nk, :nk] = np.tril(sla.solve_triangular(L[k0:k0 + nk, k0:k0 + nk], np.eye(nk), lower=True))
    return D


def np_solve_dinv(L, D, B, block=DINV_BLOCK):
    """the inverted-block forward solve in float64: X_k = inv(L_kk) (B_k - L_k,<k X_<k), products only"""
    L = lower(L)
    n = L.shape[0]
    X = np.zeros_like(np.asarray(B), dtype=np.float64)
    for k0 in range(0, n, block):
        nk = min(block, n - k0)
        X[k0:k0 + nk] = D[k0:k0 + nk, :nk] @ (B[k0:k0 + nk] - L[k0:k0 + nk, :k0] @ X[:k0])
    return X


def res_dinv_blocks(L, D, block=DINV_BLOCK):
    """(err, scale, above) of all inverted blocks stacked: |L_kk Dinv_k - I| against |L_kk||Dinv_k|, and the entries of Dinv above the
    diagonal of each block (they have to be exact zeros)"""
    Lt = lower(L)
    n = Lt.shape[0]
    errs, scs, above = [], [], []
    for k0 in range(0, n, block):
        nk = min(block, n - k0)
        blk = np.asarray(D)[k0:k0 + nk, :nk]
        e, s = res_solve('N', Lt[k0:k0 + nk, k0:k0 + nk], blk, np.eye(nk))
        errs.append(e.ravel()); scs.append(s.ravel()); above.append(blk[np.triu_indices(nk, 1)])
    return np.concatenate(errs), np.concatenate(scs), np.concatenate(above)


# ----------------------------------------------------------------------- the old, norm-wise asserts (copied for the injection tests)
def old_potrf_assert(L, A):
    """tests/test_gpu_parity.py::test_potrf"""
    return bool(np.linalg.norm(L @ L.T - A) <= 1e-13 * np.linalg.norm(A))


def old_solve_assert(L, X, B):
    """tests/test_gpu_parity.py::test_trsm (trans = 0)"""
    return bool(np.linalg.norm(L @ X - B) <= 1e-12 * np.linalg.norm(L) * np.linalg.norm(X))


def smallest_row(M):
    """the row of smallest scale (largest entry)"""
    return int(np.argmin(np.max(np.abs(M), axis=1)))
