"""The checker behind tests/test_gpu_dense_views.py, exercised without a GPU: a numpy array stands in for the device buffer.

The arena must notice a single stray write one element past each edge of a view, a canary replaced by a DIFFERENT NaN (so the
comparison is on bits, not on isnan), and a changed read-only operand; it must pass on a clean run.  The longdouble references
must agree with scipy.linalg / numpy.linalg (double) to a few eps on well-conditioned inputs."""
import numpy as np
import pytest
import scipy.linalg as sla

import _view_arena as VA

EPS = np.finfo(np.float64).eps


def _arena_with_view():
    arena = VA.Arena(None, 12, 17, 19)
    v = arena.view(3, 4, 5, 6)
    arena.put(v, np.arange(30.0).reshape(5, 6))
    return arena, v


def test_canary_is_a_quiet_nan_with_payload():
    assert np.isnan(VA.CANARY)
    b = int(VA.CANARY_BITS)
    assert (b >> 52) & 0x7FF == 0x7FF and (b >> 51) & 1 == 1 and b & ((1 << 51) - 1) != 0
    assert int(VA.bits(np.array([np.nan]))[0]) != b               # not the NaN arithmetic produces


def test_clean_run_passes():
    arena, v = _arena_with_view()
    arena.assert_outside_untouched([])                            # nothing written at all: the view counts as read-only
    arena.dev.buf[v.index] = 7.0                                  # the routine writes its whole output region
    arena.assert_outside_untouched([v])
    assert np.array_equal(arena.get(v), np.full((5, 6), 7.0))


@pytest.mark.parametrize('where,di,dj', [('above', -1, 2), ('below', 5, 2), ('left', 1, -1), ('right', 1, 6),
                                         ('corner', 5, 6), ('first element of the buffer', -3, -4)])
def test_single_stray_write_is_caught(where, di, dj):
    arena, v = _arena_with_view()
    arena.dev.buf[v.index] = 1.0
    arena.dev.buf[(v.r0 + di) * arena.ld + v.c0 + dj] = 0.0
    with pytest.raises(AssertionError, match='canary region'):
        arena.assert_outside_untouched([v])


def test_padding_columns_between_cols_and_ld_are_guarded():
    arena, v = _arena_with_view()
    arena.dev.buf[2 * arena.ld + 18] = 1.0                        # column 18 >= cols = 17: padding of the leading dimension
    with pytest.raises(AssertionError):
        arena.assert_outside_untouched([v])


def test_foreign_nan_is_caught():
    arena, v = _arena_with_view()
    arena.dev.buf[0] = np.nan                                     # a NaN, but not the canary
    assert np.isnan(arena.dev.read()).sum() == arena.size - 30    # a float comparison could not tell
    with pytest.raises(AssertionError, match='canary region'):
        arena.assert_outside_untouched([v])


def test_changed_read_only_operand_is_caught():
    arena = VA.Arena(None, 10, 20)
    a = arena.view(1, 1, 4, 4); b = arena.view(1, 8, 4, 4)
    arena.put(a, VA.with_canary_upper(np.ones((4, 4)))); arena.put(b, np.zeros((4, 4)))
    arena.dev.buf[b.index] = 3.0
    arena.assert_outside_untouched([b])
    arena.dev.buf[a.index[0, 1]] = np.nan                         # the canary in the operand's upper triangle replaced
    with pytest.raises(AssertionError, match='read-only'):
        arena.assert_outside_untouched([b])


def test_views_must_fit_and_not_overlap():
    arena = VA.Arena(None, 10, 20)
    arena.view(1, 1, 4, 4)
    with pytest.raises(ValueError):
        arena.view(2, 2, 4, 4)
    with pytest.raises(ValueError):
        arena.view(8, 0, 3, 4)
    with pytest.raises(ValueError):
        arena.view(0, 18, 2, 4)


@pytest.mark.parametrize('cls', VA.CLASSES)
@pytest.mark.parametrize('m,n', [(1, 1), (5, 7), (64, 64), (65, 3)])
def test_class_view_builds_the_named_class(cls, m, n):
    v = VA.class_view(None, m, n, cls)
    assert v.cls == cls
    assert ((v.ptr & 15) != 0) == (cls in 'BD') and ((v.ld & 1) != 0) == (cls in 'CD')
    a = v.arena
    assert v.r0 >= 2 and v.c0 >= 2 and a.rows - v.r0 - m >= 2 and a.ld - v.c0 - n >= 2
    for odd in (False, True):
        assert ((VA.vector_view(None, 9, odd).ptr & 15) != 0) == odd
        f = VA.flat_view(None, 6, 4, odd)
        assert ((f.ptr & 15) != 0) == odd and f.ld == 4
        f.arena.put(f, np.arange(24.0).reshape(6, 4))
        assert np.array_equal(f.arena.dev.buf[f.offset:f.offset + 24], np.arange(24.0))   # contiguous


# ------------------------------------------------------------------------------------------------------------- references
def _well_conditioned_L(rng, n):
    return np.tril(rng.normal(size=(n, n))) + np.diag(rng.uniform(3, 4, n) * np.sqrt(n))


def test_reference_products_match_numpy():
    rng = np.random.RandomState(0)
    A = rng.normal(size=(70, 33)); B = rng.normal(size=(33, 50))
    bound = 33 * EPS * (np.abs(A) @ np.abs(B))
    assert np.all(np.abs(VA.ref_matmul(A, B).astype(np.float64) - A @ B) <= bound)
    assert VA.ref_matmul(A, B).dtype == np.longdouble
    assert np.all(np.abs(VA.ref_ata(A).astype(np.float64) - A.T @ A) <= 70 * EPS * (np.abs(A.T) @ np.abs(A)))


@pytest.mark.parametrize('n,nrhs', [(1, 1), (5, 3), (64, 7), (200, 31)])
def test_reference_solves_match_scipy(n, nrhs):
    rng = np.random.RandomState(n)
    L = _well_conditioned_L(rng, n)
    B = rng.normal(size=(n, nrhs)); Xr = rng.normal(size=(nrhs, n))
    Lnan = VA.with_canary_upper(L)                                # the references read the lower triangle only
    for got, want in ((VA.ref_forward(Lnan, B), sla.solve_triangular(L, B, lower=True)),
                      (VA.ref_backward(Lnan, B), sla.solve_triangular(L, B, lower=True, trans='T')),
                      (VA.ref_right_lt(Lnan, Xr), sla.solve_triangular(L, Xr.T, lower=True).T)):
        assert got.dtype == np.longdouble and got.shape == want.shape
        # cond(L) is a small constant here (diagonal ~ 3.5 sqrt n against a strict lower part of norm ~ sqrt(n / 2))
        assert np.linalg.norm(got.astype(np.float64) - want) <= 16 * EPS * np.linalg.cond(L) * np.linalg.norm(want)


@pytest.mark.parametrize('n', [1, 5, 64, 130])
def test_reference_cholesky_matches_numpy(n):
    rng = np.random.RandomState(n)
    M = rng.normal(size=(n, n))
    A = M @ M.T + n * np.eye(n)
    got = VA.ref_cholesky(VA.with_canary_upper(A))                # reads the lower triangle only
    want = np.linalg.cholesky(A)
    assert got.dtype == np.longdouble
    assert np.all(np.triu(got, 1) == 0)
    assert np.linalg.norm(got.astype(np.float64) - want) <= 16 * EPS * np.linalg.cond(A) * np.linalg.norm(want)
    A[n // 2, n // 2] = -1.0                                      # a non-positive pivot: NaN from that column on
    bad = VA.ref_cholesky(A)
    assert np.isnan(bad[n // 2, n // 2]) and not np.isnan(bad[:n // 2, :n // 2]).any()
