"""tests/_dense_reference.py itself, on the CPU: its long-double residual against mpmath, the preconditions of every case that
tests/test_gpu_dense_componentwise.py hands to the device, and NEGATIVE CONTROLS -- an error of 1e-11 in the row of smallest scale,
or a non-zero where the structure promises a zero, is rejected by the componentwise gate while the norm-wise asserts of
tests/test_gpu_parity.py (copied verbatim into _dense_reference.old_*_assert) accept it.  The float64 numpy rendition stands in for
the device; where the device test solves with the device's own factor of a Gram matrix, numpy's factor stands in for that."""
import numpy as np
import pytest

import _dense_reference as D

LD, EPS = D.LD, D.EPS
TINY = 1e-11


def _mp_matrix(mp, a):
    return mp.matrix([[mp.mpf(float(v)) for v in row] for row in np.atleast_2d(a)])


def test_long_double_residuals_agree_with_mpmath():
    """every residual kind on one order-40 case against 40-digit arithmetic: the long-double residual differs from the exact one by
    at most 1e-3 eps of its scale (long double carries 11 more bits than float64), and the scales agree to 1e-12"""
    import mpmath as mp
    n, nrhs = 40, 5
    A, L, B = D.graded(n), D.graded_factor(n), D.rhs(n, nrhs)
    Lc = D.np_cholesky(A)
    worst = 0.0
    with mp.workdps(40):
        def compare(err, scale, exact_res, exact_scale, mask=None):
            nonlocal worst
            for i in range(err.shape[0]):
                for j in range(err.shape[1]):
                    if mask is not None and not mask[i, j]:
                        continue
                    hi = float(err[i, j]); lo = float(err[i, j] - LD(hi))
                    d = abs(mp.mpf(hi) + mp.mpf(lo) - abs(exact_res[i, j])) / (mp.mpf(EPS) * exact_scale[i, j])
                    worst = max(worst, float(d))
                    assert abs(mp.mpf(float(scale[i, j])) - exact_scale[i, j]) <= mp.mpf(1e-12) * exact_scale[i, j]

        def absm(M):
            return M.apply(abs)

        mLc, mA = _mp_matrix(mp, np.tril(Lc)), _mp_matrix(mp, A)
        err, scale = D.res_cholesky(Lc, A)
        compare(err, scale, mLc * mLc.T - mA, absm(mLc) * absm(mLc.T), np.tri(n, dtype=bool))
        mL, mB = _mp_matrix(mp, np.tril(L)), _mp_matrix(mp, B)
        for kind in 'NTP':
            X = D.np_solve(kind, L, B)
            mX = _mp_matrix(mp, X)
            err, scale = D.res_solve(kind, D.poisoned(L), X, B)           # (only the lower triangle of the stored factor is read)
            if kind == 'N':
                compare(err, scale, mL * mX - mB, absm(mL) * absm(mX))
            elif kind == 'T':
                compare(err, scale, mL.T * mX - mB, absm(mL.T) * absm(mX))
            else:
                mY = mL.T * mX
                compare(err, scale, mL * mY - mB, absm(mL) * (absm(mL.T) * absm(mX)) + absm(mL) * absm(mY))
        B2 = D.rhs(nrhs, n)
        X = D.np_solve('R', L, B2)
        mX = _mp_matrix(mp, X)
        err, scale = D.res_solve('R', L, X, B2)
        compare(err, scale, mX * mL.T - _mp_matrix(mp, B2), absm(mX) * absm(mL.T))
    print(f'\n[dense reference] long double vs mpmath: worst difference of a residual entry {worst:.2e} eps of its scale')
    assert worst <= 1e-3


NP_WORST = {}


def _note(tag, what, r):
    NP_WORST[tag] = max(NP_WORST.get(tag, 0.0), r)
    print(f'[numpy {tag}] {what}: {r:.3g} eps; worst so far {NP_WORST[tag]:.3g}')
    assert r <= D.CAP, (tag, what, r)


def _solve_figures(tag, what, L, n):
    for kind in 'NT':
        for nrhs in D.NRHS:
            B = D.rhs(n, nrhs)
            _note(f'trsm {kind}', f'{what} nrhs {nrhs}', D.worst(*D.res_solve(kind, L, D.np_solve(kind, L, B), B)))
    B = D.rhs(n, 130)
    for lead in (129, 64, 100):
        Bl = D.rhs(n, 130, lead)
        X = D.np_solve('N', L, Bl)
        assert np.all(X[D.lead_mask(n, 130, lead)] == 0.0)
        _note('trsm_lz', f'{what} lead {lead}', D.worst(*D.res_solve('N', L, X, Bl)))
    for m in (1, 70):
        B2 = D.rhs(m, n)
        _note('trsm_right_lt', f'{what} m {m}', D.worst(*D.res_solve('R', L, D.np_solve('R', L, B2), B2)))
    _note('potrs', what, D.worst(*D.res_solve('P', L, D.np_solve('P', L, B), B)))


@pytest.mark.parametrize('case', D.gram_cases(), ids=D.gram_id)
def test_preconditions_gram(case):
    """the pivot condition (asserted by gram() itself) and numpy's own ratio <= CAP for every operation of the device test"""
    A = D.gram(*case)
    n = A.shape[0]
    assert np.array_equal(A, A.T)
    Lld = D.cholesky_ld(A)
    piv = D.relative_pivot(A, Lld)
    print(f'\n[gram {D.gram_id(case)}] order {n}, exact zeros {np.count_nonzero(A == 0.0)}, diagonal {np.min(np.diag(A)):.3g} .. '
          f'{np.max(np.diag(A)):.3g}, min l_ii^2 / a_ii = {piv:.3g} = {piv / (n * EPS):.3g} n eps')
    assert piv >= D.PIVOT_MARGIN * n * EPS
    assert D.worst(*D.res_cholesky(Lld.astype(np.float64), A)) <= 2.0          # the long-double factor rounded: the reference is sound
    L = D.np_cholesky(A)
    _note('potrf', D.gram_id(case), D.worst(*D.res_cholesky(L, A)))
    _solve_figures('gram', D.gram_id(case), L, n)


@pytest.mark.parametrize('n', D.GRADED_ORDERS)
def test_preconditions_graded(n):
    A = D.graded(n)
    print()
    _note('potrf', f'graded {n}', D.worst(*D.res_cholesky(D.np_cholesky(A), A)))


@pytest.mark.parametrize('n', D.FACTOR_ORDERS)
def test_preconditions_graded_factor(n):
    print()
    _solve_figures('graded_factor', f'graded_factor {n}', D.graded_factor(n), n)


def _dinv_sources():
    return [('graded_factor', n) for n in D.DINV_ORDERS] + [('gram', c) for c in D.gram_cases()]


def _dinv_id(s):
    return f'graded_factor-{s[1]}' if s[0] == 'graded_factor' else 'gram-' + D.gram_id(s[1])


def _dinv_factor(source):
    return D.graded_factor(source[1]) if source[0] == 'graded_factor' else D.np_cholesky(D.gram(*source[1]))


@pytest.mark.parametrize('source', _dinv_sources(), ids=_dinv_id)
def test_inverted_block_solve_figures(source):
    """The GEMM-only solve through inverted 256-row diagonal blocks is only conditionally stable: its residual
    carries the condition of the diagonal blocks.  On these cases its numpy rendition stays within CAP all the same (measured: at most
    4.1 eps on graded_factor, 14.6 eps on the factors of the Gram cases, whose solutions are large against their right-hand sides)."""
    L = _dinv_factor(source)
    n = L.shape[0]
    Dn = D.np_trtri_diag(L)
    e, s, above = D.res_dinv_blocks(L, Dn)
    assert np.all(above == 0.0)
    print()
    _note('trtri_diag', _dinv_id(source), D.worst(e, s))
    for lead in (0, 129):
        B = D.rhs(n, 130, lead)
        X = D.np_solve_dinv(L, Dn, B)
        assert np.all(X[D.lead_mask(n, 130, lead)] == 0.0)
        _note('trsm_dinv ' + source[0], f'{_dinv_id(source)} lead {lead}', D.worst(*D.res_solve('N', L, X, B)))


@pytest.mark.parametrize('m,n,k', D.PRODUCT_SHAPES)
def test_preconditions_products(m, n, k):
    print()
    for case in D.product_cases(m, n, k):
        err, scale = D.res_product(case['opA'], case['opB'], case['alpha'], case['beta'], case['C0'], D.np_product(case))
        if case['entry'] == 'gemm_lz' and case['beta'] == 0.0 and case['lead'] > k:
            assert np.count_nonzero(scale == 0) == m * (case['lead'] - k)           # whole columns of exact zeros
        _note('product', f'{case["name"]} {(m, n, k)}', D.worst(err, scale))


# ------------------------------------------------------------------------------------------------------ negative controls
INJECT = [('gram', ('Nonlinear_elliptic', 200, 60, 1e-10)), ('graded', 320)]


def _inject_matrix(which):
    return D.gram(*which[1]) if which[0] == 'gram' else D.graded(which[1])


@pytest.mark.parametrize('which', INJECT, ids=lambda w: w[0])
def test_gate_rejects_a_scaled_row_of_the_factor(which):
    """the smallest-scale row of numpy's factor times (1 + 1e-11): rejected entry by entry, accepted by ||L L^T - A|| <= 1e-13 ||A||"""
    A = _inject_matrix(which)
    L = D.np_cholesky(A)
    host = D.res_cholesky(L, A)
    r_np = D.worst(*host)
    r, a, ok = D.gate(host, r_np)
    assert ok and r == r_np and D.old_potrf_assert(L, A)
    bad = L.copy()
    bad[D.smallest_row(L)] *= 1.0 + TINY
    r, a, ok = D.gate(D.res_cholesky(bad, A), r_np)
    print(f'\n[inject factor {which[0]}] numpy {r_np:.3g}, allowed {a:.3g}, injected {r:.3g}; the norm-wise assert accepts: {D.old_potrf_assert(bad, A)}')
    assert not ok and r > a
    assert D.old_potrf_assert(bad, A)


def _inject_factor(which):
    return D.np_cholesky(D.gram(*which[1])) if which[0] == 'gram' else D.graded_factor(which[1])


@pytest.mark.parametrize('which', INJECT, ids=lambda w: w[0])
def test_gate_rejects_a_scaled_row_of_a_solution(which):
    """the smallest-scale row of a numpy solution times (1 + 1e-11): rejected, while ||L X - B|| <= 1e-12 ||L|| ||X|| accepts it"""
    L = _inject_factor(which)
    n = L.shape[0]
    B = D.rhs(n, 37)
    X = D.np_solve('N', L, B)
    host = D.res_solve('N', L, X, B)
    r_np = D.worst(*host)
    assert D.gate(host, r_np)[2] and D.old_solve_assert(L, X, B)
    bad = X.copy()
    bad[D.smallest_row(X)] *= 1.0 + TINY
    r, a, ok = D.gate(D.res_solve('N', L, bad, B), r_np)
    print(f'\n[inject solution {which[0]}] numpy {r_np:.3g}, allowed {a:.3g}, injected {r:.3g}; the norm-wise assert accepts: {D.old_solve_assert(L, bad, B)}')
    assert not ok and r > a
    assert D.old_solve_assert(L, bad, B)


@pytest.mark.parametrize('which', INJECT, ids=lambda w: w[0])
def test_gate_rejects_a_non_zero_in_a_structural_zero(which):
    """a leading-zero solution with 1e-11 of its smallest non-zero magnitude written into a structural zero: rejected by the residual
    of that entry (its scale without the stray value is 0) and by the zeros argument, accepted by the norm-wise residual"""
    L = _inject_factor(which)
    n, nrhs, lead = L.shape[0], 130, 100
    B = D.rhs(n, nrhs, lead)
    X = D.np_solve('N', L, B)
    mask = D.lead_mask(n, nrhs, lead)
    host = D.res_solve('N', L, X, B)
    r_np = D.worst(*host)
    assert np.all(X[mask] == 0.0) and np.all(host[1][mask] == 0) and D.gate(host, r_np, X[mask])[2]
    bad = X.copy()
    bad[0, 0] = TINY * np.min(np.abs(X[X != 0.0]))
    assert mask[0, 0]
    r, a, ok = D.gate(D.res_solve('N', L, bad, B), r_np)
    print(f'\n[inject zero {which[0]}] stray {bad[0, 0]:.3g}: ratio {r:.3g}, allowed {a:.3g}; the norm-wise assert accepts: {D.old_solve_assert(L, bad, B)}')
    assert not ok and r > a
    assert not D.gate(host, r_np, bad[mask])[2]
    assert D.old_solve_assert(L, bad, B)
    # a result that is exact everywhere except for a stray value where the scale vanishes: no quotient, still rejected
    err, scale = host[0].copy(), host[1].copy()
    err[0, 0] = 1e-300
    assert scale[0, 0] == 0 and not D.check(err, scale, 1e6) and D.worst(err, scale) == float('inf')
