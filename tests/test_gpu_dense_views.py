"""The dense entry points of include/gpk.h on unaligned sub-matrix views, with canaries around every operand.

include/gpk.h promises of every dense routine that (1) any alignment is accepted -- 16-byte loads only "when pointer and leading
dimension allow" --, (2) operands are views (device pointer + leading dimension in elements) of which the routine writes its declared
output region and nothing else, and (3) triangular routines use only the lower triangle of L.  Here every routine is called through
the C ABI (ctx.lib.gpk_*) on views placed in canary-filled arenas (tests/_view_arena.py) in the four alignment classes

    A  aligned base, even ld (control)     B  odd element offset, even ld     C  aligned base, odd ld     D  odd offset, odd ld

and every case asserts the return code, the result against a numpy longdouble reference, and -- bit for bit -- that nothing outside
the output views changed (canaries and read-only operands).

Bounds: the ones the project states in tests/test_gpu_parity.py, the same for every alignment class:
  * products (GEMM / SYRK), PER ROW i:  max_j |err_ij| <= 1e-13 * max_j (|op A||op B| + |beta C|)_ij
  * POTRF / panel:  ||L L^T - A||_F <= 1e-13 ||A||_F;  ||L - L_ref||_F <= 1e-11 ||L_ref||_F (test_potrf's bound)
  * solves:  ||L X - B||_F <= 1e-12 ||L||_F ||X||_F  (residual formed in longdouble with the lower triangle of L);
    gpk_potrs is two such solves, L Y = B then L^T X = Y:  L L^T X - B = L (L^T X - Y) + (L Y - B), and ||Y|| <= ||L|| ||X|| up to
    rounding, so its residual is bounded by 2e-12 ||L||_F^2 ||X||_F
  * gpk_tril, gpk_symmetrize_lower, gpk_memcpy2d_d2d: exact; gpk_axpy: one fma or one multiply and one add, nothing else
  * "the upper triangle of L is never used": the same call with zeros and with NaN canaries above the diagonal gives bit-identical,
    NaN-free output.
L is well conditioned (tril(randn) + diag(U(3, 4) sqrt n), as in test_trsm) so that the residual bounds are sharp.
Orders follow the dispatch conditions of csrc/gpk_factor.hip: the 256-row strip kernel (n <= 256, n % 16 == 0), the 64-row base kernel,
the recursion above them, the transposed and right-side base kernels, the single-vector kernel (nrhs == 1, ldb == 1).
The tight, entry-by-entry gates of the same routines (componentwise backward error on Gram and row-scaled matrices) live in
tests/test_gpu_dense_componentwise.py; the subject here is views and canaries, so the norm-wise bounds above are kept.
"""
import ctypes as C
import functools
from fractions import Fraction

import numpy as np
import pytest

import _view_arena as VA

pytestmark = pytest.mark.gpu

LD = np.longdouble


@pytest.fixture(scope='module')
def ctx():
    import gpk
    c = gpk.Context(0)
    yield c
    c.lib.gpk_debug_set(0, 0)
    c.close()


class Maker:
    """views of one test: built on demand, checked together, freed at the end"""

    def __init__(self, ctx):
        self.ctx, self.arenas, self.written = ctx, [], []

    def _keep(self, v, data):
        self.arenas.append(v.arena)
        if data is not None:
            v.arena.put(v, data)
        return v

    def mat(self, m, n, cls, data=None):
        return self._keep(VA.class_view(self.ctx, m, n, cls), data)

    def vec(self, n, odd, data=None):
        return self._keep(VA.vector_view(self.ctx, n, odd), data)

    def flat(self, m, n, odd, data=None):
        return self._keep(VA.flat_view(self.ctx, m, n, odd), data)

    def check(self, written):
        """canaries and read-only operands of EVERY arena of this test intact; `written`: the output views of the call just made
        (output views of earlier calls of the same test stay exempt)"""
        self.written += [v for v in written if not any(v is w for w in self.written)]
        for a in self.arenas:
            a.assert_outside_untouched([v for v in self.written if v.arena is a])

    def free(self):
        for a in self.arenas:
            a.free()
        self.arenas = []


@pytest.fixture
def mk(ctx):
    m = Maker(ctx)
    yield m
    m.free()


def get(v):
    return v.arena.get(v)


def _assert_rows(got, want, scale, mask=None, what=''):
    """per-row product bound: max_j |got - want|_ij <= 1e-13 max_j scale_ij (over the entries of `mask`)"""
    err = np.abs(got.astype(LD) - want)
    if mask is not None:
        err = np.where(mask, err, 0); scale = np.where(mask, scale, 0)
        assert not np.isnan(got[mask]).any(), what
    else:
        assert not np.isnan(got).any(), what
    e, s = err.max(axis=1), 1e-13 * scale.max(axis=1)
    worst = int(np.argmax(e - s))
    assert np.all(e <= s), f'{what}: row {worst}: error {float(e[worst]):.3e} > bound {float(s[worst]):.3e}'


def _well_conditioned_L(rng, n):
    return np.tril(rng.normal(size=(n, n))) + np.diag(rng.uniform(3, 4, n) * np.sqrt(n))


def _spd(rng, n):
    M = rng.normal(size=(n, n))
    return M @ M.T + n * np.eye(n)


# ================================================================================================================= GEMM
GEMM_SHAPES = [(64, 64, 16), (130, 70, 33), (257, 193, 100)]           # interior tiles, edge tiles, a partial K slab
GEMM_SCALARS = [(1.7, 0.0), (1.7, -0.3), (-1.0, 1.0)]                  # beta = 0: C holds canaries and must not be read
GEMM_CLASSES = ([('A', 'A', 'A')] + [tuple(c if i == k else 'A' for i in range(3)) for k in range(3) for c in 'BCD']
                + [('D', 'D', 'D')])


@functools.lru_cache(maxsize=None)
def _gemm_case(ta, tb, m, n, k, alpha, beta, lead=0):
    rng = np.random.RandomState(1000 * ta + 100 * tb + m + n + k)
    A = rng.normal(size=(k, m) if ta else (m, k))                       # asymmetric operands catch transposed maps
    B = rng.normal(size=(n, k) if tb else (k, n))
    if lead:                                                            # column c < lead of B is zero above row lead - 1 - c
        rows = np.arange(k)[:, None]; cols = np.arange(n)[None, :]
        B[(cols < lead) & (rows < lead - 1 - cols)] = 0.0
    if ta:                                                              # one row of small entries in op(A) ...
        A[:, m // 3] *= 1e-6
    else:
        A[m // 3, :] *= 1e-6
    C0 = rng.normal(size=(m, n))
    C0[m // 3, :] *= 1e-6                                               # ... and in C: the per-row bound must hold there too
    opA, opB = (A.T if ta else A), (B.T if tb else B)
    want = alpha * VA.ref_matmul(opA, opB)
    scale = VA.ref_matmul(np.abs(opA), np.abs(opB))
    if beta != 0.0:
        want = want + LD(beta) * C0.astype(LD)
        scale = scale + abs(beta) * np.abs(C0).astype(LD)
    return A, B, C0, want, scale


def _run_gemm(ctx, mk, ta, tb, m, n, k, alpha, beta, classes, lead=0, lz=False):
    A, B, C0, want, scale = _gemm_case(ta, tb, m, n, k, alpha, beta, lead)
    ca, cb, cc = classes
    vA = mk.mat(A.shape[0], A.shape[1], ca, A)
    vB = mk.mat(B.shape[0], B.shape[1], cb, B)
    vC = mk.mat(m, n, cc, C0 if beta != 0.0 else None)                  # beta = 0: canaries in C
    assert (vA.cls, vB.cls, vC.cls) == classes
    if lz:
        rc = ctx.lib.gpk_gemm_lz(ctx.h, ta, m, n, k, alpha, vA.ptr, vA.ld, vB.ptr, vB.ld, beta, vC.ptr, vC.ld, lead)
    else:
        rc = ctx.lib.gpk_gemm(ctx.h, ta, tb, m, n, k, alpha, vA.ptr, vA.ld, vB.ptr, vB.ld, beta, vC.ptr, vC.ld)
    assert rc == 0
    _assert_rows(get(vC), want, scale, what=f'gemm {classes}')
    mk.check([vC])


@pytest.mark.parametrize('classes', GEMM_CLASSES, ids=['-'.join(c) for c in GEMM_CLASSES])
@pytest.mark.parametrize('alpha,beta', GEMM_SCALARS)
@pytest.mark.parametrize('m,n,k', GEMM_SHAPES)
@pytest.mark.parametrize('ta,tb', [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_gemm_views(ctx, mk, ta, tb, m, n, k, alpha, beta, classes):
    _run_gemm(ctx, mk, ta, tb, m, n, k, alpha, beta, classes)


@pytest.mark.parametrize('cfg', [1, 2, 3, 4])
@pytest.mark.parametrize('m,n,k', GEMM_SHAPES)
@pytest.mark.parametrize('ta,tb', [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_gemm_views_forced_tile_configurations_D(ctx, mk, ta, tb, m, n, k, cfg):
    """gpk_debug_set(0, 1..4): every tile configuration of the kernel template on the all-D case"""
    ctx.lib.gpk_debug_set(0, cfg)
    try:
        _run_gemm(ctx, mk, ta, tb, m, n, k, 1.7, -0.3, ('D', 'D', 'D'))
    finally:
        ctx.lib.gpk_debug_set(0, 0)


@pytest.mark.parametrize('classes', [('A', 'A', 'A'), ('A', 'D', 'A'), ('D', 'D', 'D')], ids=lambda c: '-'.join(c))
@pytest.mark.parametrize('beta', [0.0, 1.0])
@pytest.mark.parametrize('ta', [0, 1])
@pytest.mark.parametrize('m,n,k,lead', [(130, 150, 200, 140), (70, 257, 300, 250)])
def test_gemm_lz_views(ctx, mk, ta, m, n, k, lead, beta, classes):
    """leading zeros of B skipped (late K start per tile): same result as the dense product"""
    _run_gemm(ctx, mk, ta, 0, m, n, k, -1.0, beta, classes, lead=lead, lz=True)


# ================================================================================================================= SYRK
@functools.lru_cache(maxsize=None)
def _syrk_case(n, k, alpha, beta):
    rng = np.random.RandomState(n + k)
    A = rng.normal(size=(k, n))
    A[:, n // 2] *= 1e-6                                                # a row (and column) of small entries in A^T A
    C0 = rng.normal(size=(n, n))
    C0[n // 2, :] *= 1e-6
    want = alpha * VA.ref_ata(A) + LD(beta) * C0.astype(LD)
    scale = VA.ref_ata(np.abs(A)) + abs(beta) * np.abs(C0).astype(LD)
    return A, C0, want, scale


@pytest.mark.parametrize('ca,cc', [('A', 'A'), ('D', 'A'), ('A', 'D'), ('D', 'D')], ids=lambda c: c)
@pytest.mark.parametrize('full', [0, 1])
@pytest.mark.parametrize('n,k', [(100, 300), (130, 77), (257, 100), (63, 20)])
def test_syrk_views(ctx, mk, n, k, full, ca, cc):
    alpha, beta = 0.7, -1.3
    A, C0, want, scale = _syrk_case(n, k, alpha, beta)
    vA, vC = mk.mat(k, n, ca, A), mk.mat(n, n, cc, C0)
    assert ctx.lib.gpk_syrk(ctx.h, n, k, alpha, vA.ptr, vA.ld, beta, vC.ptr, vC.ld, full) == 0
    got = get(vC)
    lower = np.tril(np.ones((n, n), dtype=bool))
    _assert_rows(got, want, scale, mask=lower, what=f'syrk {ca}{cc}')
    if full:
        assert np.array_equal(VA.bits(got), VA.bits(got.T.copy()))      # C == C^T bit for bit
    else:
        ii, jj = np.triu_indices(n, 1)
        out = (ii // 64) < (jj // 64)                                   # (diagonal 64 x 64 tiles are written whole)
        assert np.array_equal(VA.bits(got[ii[out], jj[out]]), VA.bits(C0[ii[out], jj[out]]))
    mk.check([vC])


# ============================================================================================== exact element-wise routines
EXACT_N = [1, 63, 64, 65, 257]


@pytest.mark.parametrize('cls', ['A', 'D'])
@pytest.mark.parametrize('n', EXACT_N)
def test_tril_and_symmetrize_views(ctx, mk, n, cls):
    rng = np.random.RandomState(n)
    M = rng.normal(size=(n, n))
    v = mk.mat(n, n, cls, M)
    assert ctx.lib.gpk_symmetrize_lower(ctx.h, v.ptr, n, v.ld) == 0
    want = np.tril(M) + np.tril(M, -1).T
    assert np.array_equal(VA.bits(get(v)), VA.bits(want))
    mk.check([v])
    w = mk.mat(n, n, cls, VA.with_canary_upper(M))                      # the upper triangle is overwritten, never read
    assert ctx.lib.gpk_tril(ctx.h, w.ptr, n, w.ld) == 0
    assert np.array_equal(VA.bits(get(w)), VA.bits(np.tril(M)))
    mk.check([v, w])


@pytest.mark.parametrize('cs,cd', [('A', 'A'), ('D', 'A'), ('A', 'D'), ('D', 'D')], ids=lambda c: c)
@pytest.mark.parametrize('n', EXACT_N)
def test_memcpy2d_d2d_views(ctx, mk, n, cs, cd):
    rng = np.random.RandomState(n)
    M = rng.normal(size=(n, n + 3))
    src, dst = mk.mat(n, n + 3, cs, M), mk.mat(n, n + 3, cd)
    assert ctx.lib.gpk_memcpy2d_d2d(ctx.h, dst.ptr, dst.ld * 8, src.ptr, src.ld * 8, (n + 3) * 8, n) == 0
    assert np.array_equal(VA.bits(get(dst)), VA.bits(M))
    mk.check([dst])


@pytest.mark.parametrize('ox,oy', [(0, 0), (1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize('n', EXACT_N)
def test_axpy_views(ctx, mk, n, ox, oy):
    rng = np.random.RandomState(n)
    x, y, alpha = rng.normal(size=n), rng.normal(size=n), -0.37
    vx, vy = mk.vec(n, ox, x), mk.vec(n, oy, y)
    assert ctx.lib.gpk_axpy(ctx.h, n, alpha, vx.ptr, vy.ptr) == 0
    got = get(vy)[:, 0]
    fused = np.array([float(Fraction(alpha) * Fraction(a) + Fraction(b)) for a, b in zip(x, y)])   # one rounding
    plain = alpha * x + y                                                                           # two roundings
    ok = (VA.bits(got) == VA.bits(fused)) | (VA.bits(got) == VA.bits(plain))
    assert ok.all()
    mk.check([vy])


# ============================================================================================================== solves
SOLVE_CLASSES = [('A', 'A'), ('B', 'A'), ('C', 'A'), ('D', 'A'), ('A', 'B'), ('A', 'C'), ('A', 'D'), ('D', 'D')]
SOLVE_IDS = ['L' + a + '-B' + b for a, b in SOLVE_CLASSES]
# strip kernel: 16, 64, 240, 256; 64-row base kernel: 1, 5, 65 (64 + 1), 250 (192 + 58); recursion above them: 272, 513, 600
TRSM_ORDERS = [1, 5, 16, 64, 65, 240, 250, 256, 272, 513, 600]


def _nrhs_for(n):
    return 70 if n % 2 == 0 else 37                                    # several column blocks with a partial last one


@functools.lru_cache(maxsize=None)
def _solve_case(n, nrhs, lead=0, seed=0):
    rng = np.random.RandomState(n + nrhs + seed)
    L = _well_conditioned_L(rng, n)
    B = rng.normal(size=(n, nrhs))
    if lead:
        rows = np.arange(n)[:, None]; cols = np.arange(nrhs)[None, :]
        B[(cols < lead) & (rows < lead - 1 - cols)] = 0.0
    return L, B


def _assert_residual(L, X, B, kind, what='', factor=1e-12):
    """kind 'N': L X = B, 'T': L^T X = B, 'R': X L^T = B, 'P': L L^T X = B -- residual in longdouble, lower triangle of L only"""
    assert not np.isnan(X).any(), what
    Lt = VA.ref_tril(L)
    if kind == 'N':
        R = VA.ref_matmul(Lt, X)
    elif kind == 'T':
        R = VA.ref_matmul(Lt.T, X)
    elif kind == 'R':
        R = VA.ref_matmul(X, Lt.T)
    else:
        R = VA.ref_matmul(Lt, VA.ref_matmul(Lt.T, X))
    res = VA.fro(R - np.asarray(B, dtype=LD))
    lim = factor * VA.fro(Lt) * VA.fro(X) * (2.0 * VA.fro(Lt) if kind == 'P' else 1.0)
    assert res <= lim, f'{what}: residual {res:.3e} > bound {lim:.3e}'


@pytest.mark.parametrize('cl,cb', SOLVE_CLASSES, ids=SOLVE_IDS)
@pytest.mark.parametrize('trans', [0, 1])
@pytest.mark.parametrize('n', TRSM_ORDERS)
def test_trsm_views(ctx, mk, n, trans, cl, cb):
    nrhs = _nrhs_for(n)
    L, B = _solve_case(n, nrhs)
    vL, vB = mk.mat(n, n, cl, L), mk.mat(n, nrhs, cb, B)
    assert ctx.lib.gpk_trsm(ctx.h, trans, vL.ptr, n, vL.ld, vB.ptr, nrhs, vB.ld) == 0
    _assert_residual(L, get(vB), B, 'T' if trans else 'N', f'trsm n={n} L{cl} B{cb}')
    mk.check([vB])


@pytest.mark.parametrize('cl,cb', SOLVE_CLASSES, ids=SOLVE_IDS)
@pytest.mark.parametrize('trans', [0, 1])
@pytest.mark.parametrize('n', [16, 64, 65, 256, 513])
def test_trsm_one_column_with_ld_views(ctx, mk, n, trans, cl, cb):
    """nrhs == 1 with ldb > 1: the matrix kernels, not the single-vector one"""
    L, B = _solve_case(n, 1)
    vL, vB = mk.mat(n, n, cl, L), mk.mat(n, 1, cb, B)
    assert vB.ld > 1
    assert ctx.lib.gpk_trsm(ctx.h, trans, vL.ptr, n, vL.ld, vB.ptr, 1, vB.ld) == 0
    _assert_residual(L, get(vB), B, 'T' if trans else 'N', f'trsm n={n} one column')
    mk.check([vB])


@pytest.mark.parametrize('cl', VA.CLASSES)
@pytest.mark.parametrize('odd', [0, 1], ids=['Beven', 'Bodd'])
@pytest.mark.parametrize('trans', [0, 1])
@pytest.mark.parametrize('n', [1, 64, 100, 600])
def test_trsv_views(ctx, mk, n, trans, odd, cl):
    """nrhs == 1, ldb == 1: the single-vector kernel"""
    L, B = _solve_case(n, 1)
    vL, vB = mk.mat(n, n, cl, L), mk.vec(n, odd, B)
    assert ctx.lib.gpk_trsm(ctx.h, trans, vL.ptr, n, vL.ld, vB.ptr, 1, 1) == 0
    _assert_residual(L, get(vB), B, 'T' if trans else 'N', f'trsv n={n}')
    mk.check([vB])


@pytest.mark.parametrize('cl,cb', SOLVE_CLASSES, ids=SOLVE_IDS)
@pytest.mark.parametrize('n', [5, 64, 250, 256, 513])
def test_potrs_views(ctx, mk, n, cl, cb):
    nrhs = 37
    L, B = _solve_case(n, nrhs)
    vL, vB = mk.mat(n, n, cl, L), mk.mat(n, nrhs, cb, B)
    assert ctx.lib.gpk_potrs(ctx.h, vL.ptr, n, vL.ld, vB.ptr, nrhs, vB.ld) == 0
    _assert_residual(L, get(vB), B, 'P', f'potrs n={n}')
    mk.check([vB])


# (n, nrhs, lead): with lead - n >= 64 the first diagonal solve starts at a column offset > 0 (16: strip kernel, 64 with an odd
# order: base kernel); lead = 0 is the dense routine
LZ_CASES = [(16, 100, 90), (64, 230, 200), (63, 230, 200), (250, 100, 90), (256, 100, 90), (272, 100, 90), (513, 100, 90), (600, 100, 90),
            (65, 37, 0)]


@pytest.mark.parametrize('cl,cb', SOLVE_CLASSES, ids=SOLVE_IDS)
@pytest.mark.parametrize('n,nrhs,lead', LZ_CASES)
def test_trsm_lz_views(ctx, mk, n, nrhs, lead, cl, cb):
    L, B = _solve_case(n, nrhs, lead)
    vL, vB = mk.mat(n, n, cl, L), mk.mat(n, nrhs, cb, B)
    assert ctx.lib.gpk_trsm_lz(ctx.h, vL.ptr, n, vL.ld, vB.ptr, nrhs, vB.ld, lead) == 0
    X = get(vB)
    _assert_residual(L, X, B, 'N', f'trsm_lz n={n}')
    if lead:                                                            # structural zeros of the solution stay exact zeros
        rows = np.arange(n)[:, None]; cols = np.arange(nrhs)[None, :]
        assert np.all(X[(cols < lead) & (rows < lead - 1 - cols)] == 0.0)
    mk.check([vB])


@pytest.mark.parametrize('cl,cb', SOLVE_CLASSES, ids=['L' + a + '-X' + b for a, b in SOLVE_CLASSES])
@pytest.mark.parametrize('n,m', [(1, 37), (5, 70), (16, 64), (64, 150), (65, 37), (130, 70), (250, 37)])
def test_trsm_right_lt_views(ctx, mk, n, m, cl, cb):
    """X <- X L^{-T}: the right-side base kernel (n <= 64) and the recursion above it"""
    rng = np.random.RandomState(n + m)
    L, X0 = _well_conditioned_L(rng, n), rng.normal(size=(m, n))
    vL, vX = mk.mat(n, n, cl, L), mk.mat(m, n, cb, X0)
    assert ctx.lib.gpk_trsm_right_lt(ctx.h, vL.ptr, n, vL.ld, vX.ptr, m, vX.ld) == 0
    _assert_residual(L, get(vX), X0, 'R', f'trsm_right_lt n={n}')
    mk.check([vX])


# (L, B, X, Dinv at an odd offset); Dinv is contiguous (ld = block), so only its offset varies
DINV_CLASSES = [('A', 'A', 'A', 0), ('B', 'A', 'A', 0), ('C', 'A', 'A', 0), ('D', 'A', 'A', 0), ('A', 'B', 'A', 0), ('A', 'C', 'A', 0),
                ('A', 'D', 'A', 0), ('A', 'A', 'D', 0), ('A', 'A', 'A', 1), ('D', 'D', 'D', 1)]


def _run_dinv(ctx, mk, L_host, L_ref, B, n, nrhs, lead, classes, block=256):
    cl, cb, cx, od = classes
    vL, vB = mk.mat(n, n, cl, L_host), mk.mat(n, nrhs, cb, B)
    vX = mk.mat(n, nrhs, cx, np.zeros((n, nrhs)))                       # (lead > 0: the zero part of X is not written)
    vD = mk.flat(n, block, od)
    assert ctx.lib.gpk_trtri_diag(ctx.h, vL.ptr, n, vL.ld, vD.ptr, block) == 0
    mk.check([vD])
    D = get(vD)
    assert ctx.lib.gpk_trsm_dinv(ctx.h, vL.ptr, vD.ptr, block, n, vL.ld, vB.ptr, nrhs, vB.ld, vX.ptr, vX.ld, lead) == 0
    X = get(vX)
    mk.check([vD, vB, vX])
    assert np.array_equal(VA.bits(get(vD)), VA.bits(D))                 # the solve only reads Dinv
    return D, X


@pytest.mark.parametrize('classes', DINV_CLASSES, ids=lambda c: f'L{c[0]}-B{c[1]}-X{c[2]}-D{"odd" if c[3] else "even"}')
@pytest.mark.parametrize('nrhs,lead', [(70, 0), (100, 90)])
@pytest.mark.parametrize('n', [250, 256, 513, 600])
def test_trtri_diag_trsm_dinv_views(ctx, mk, n, nrhs, lead, classes):
    block = 256
    L, B = _solve_case(n, nrhs, lead)
    D, X = _run_dinv(ctx, mk, L, L, B, n, nrhs, lead, classes, block)
    for k0 in range(0, n, block):                                       # each block: inverse of the diagonal block, exact zeros above
        nk = min(block, n - k0)
        blk = D[k0:k0 + nk, :nk]
        assert np.all(np.triu(blk, 1) == 0.0)
        R = VA.ref_matmul(np.tril(L[k0:k0 + nk, k0:k0 + nk]), blk) - np.eye(nk)
        assert VA.fro(R) <= 1e-12 * nk                                  # (the bound of test_trsm_dinv)
    _assert_residual(L, X, B, 'N', f'trsm_dinv n={n}')
    if lead:
        rows = np.arange(n)[:, None]; cols = np.arange(nrhs)[None, :]
        assert np.all(X[(cols < lead) & (rows < lead - 1 - cols)] == 0.0)


# --------------------------------------------------------------------------------- the upper triangle of L is never used
def _twice(run, L):
    """run(L as stored) with zeros and with NaN canaries in the strict upper triangle: bit-identical, NaN-free outputs"""
    out0 = run(np.tril(L))
    out1 = run(VA.with_canary_upper(L))
    for a, b in zip(out0, out1):
        assert not np.isnan(b).any()
        assert np.array_equal(VA.bits(a), VA.bits(b))


@pytest.mark.parametrize('cls', ['A', 'D'])
@pytest.mark.parametrize('trans', [0, 1])
@pytest.mark.parametrize('n', [5, 64, 256, 600])
def test_trsm_ignores_upper_triangle(ctx, mk, n, trans, cls):
    nrhs = _nrhs_for(n)
    L, B = _solve_case(n, nrhs)

    def run(Ls):
        vL, vB = mk.mat(n, n, cls, Ls), mk.mat(n, nrhs, cls, B)
        assert ctx.lib.gpk_trsm(ctx.h, trans, vL.ptr, n, vL.ld, vB.ptr, nrhs, vB.ld) == 0
        mk.check([vB])
        return [get(vB)]
    _twice(run, L)


@pytest.mark.parametrize('cls', ['A', 'D'])
@pytest.mark.parametrize('trans', [0, 1])
@pytest.mark.parametrize('n', [64, 600])
def test_trsv_ignores_upper_triangle(ctx, mk, n, trans, cls):
    L, B = _solve_case(n, 1)

    def run(Ls):
        vL, vB = mk.mat(n, n, cls, Ls), mk.vec(n, cls == 'D', B)
        assert ctx.lib.gpk_trsm(ctx.h, trans, vL.ptr, n, vL.ld, vB.ptr, 1, 1) == 0
        mk.check([vB])
        return [get(vB)]
    _twice(run, L)


@pytest.mark.parametrize('cls', ['A', 'D'])
@pytest.mark.parametrize('n', [16, 272])
def test_trsm_one_column_ignores_upper_triangle(ctx, mk, n, cls):
    L, B = _solve_case(n, 1)

    def run(Ls):
        vL, vB = mk.mat(n, n, cls, Ls), mk.mat(n, 1, cls, B)
        assert ctx.lib.gpk_trsm(ctx.h, 0, vL.ptr, n, vL.ld, vB.ptr, 1, vB.ld) == 0
        mk.check([vB])
        return [get(vB)]
    _twice(run, L)


@pytest.mark.parametrize('cls', ['A', 'D'])
def test_potrs_ignores_upper_triangle(ctx, mk, cls):
    n, nrhs = 272, 37
    L, B = _solve_case(n, nrhs)

    def run(Ls):
        vL, vB = mk.mat(n, n, cls, Ls), mk.mat(n, nrhs, cls, B)
        assert ctx.lib.gpk_potrs(ctx.h, vL.ptr, n, vL.ld, vB.ptr, nrhs, vB.ld) == 0
        mk.check([vB])
        return [get(vB)]
    _twice(run, L)


@pytest.mark.parametrize('cls', ['A', 'D'])
@pytest.mark.parametrize('n,nrhs,lead', [(64, 230, 200), (600, 100, 90)])
def test_trsm_lz_ignores_upper_triangle(ctx, mk, n, nrhs, lead, cls):
    L, B = _solve_case(n, nrhs, lead)

    def run(Ls):
        vL, vB = mk.mat(n, n, cls, Ls), mk.mat(n, nrhs, cls, B)
        assert ctx.lib.gpk_trsm_lz(ctx.h, vL.ptr, n, vL.ld, vB.ptr, nrhs, vB.ld, lead) == 0
        mk.check([vB])
        return [get(vB)]
    _twice(run, L)


@pytest.mark.parametrize('cls', ['A', 'D'])
@pytest.mark.parametrize('n,m', [(64, 150), (130, 70)])
def test_trsm_right_lt_ignores_upper_triangle(ctx, mk, n, m, cls):
    rng = np.random.RandomState(n + m)
    L, X0 = _well_conditioned_L(rng, n), rng.normal(size=(m, n))

    def run(Ls):
        vL, vX = mk.mat(n, n, cls, Ls), mk.mat(m, n, cls, X0)
        assert ctx.lib.gpk_trsm_right_lt(ctx.h, vL.ptr, n, vL.ld, vX.ptr, m, vX.ld) == 0
        mk.check([vX])
        return [get(vX)]
    _twice(run, L)


@pytest.mark.parametrize('cls', ['A', 'D'])
@pytest.mark.parametrize('nrhs,lead', [(70, 0), (100, 90)])
def test_trsm_dinv_ignores_upper_triangle(ctx, mk, nrhs, lead, cls):
    n = 600
    L, B = _solve_case(n, nrhs, lead)
    _twice(lambda Ls: _run_dinv(ctx, mk, Ls, L, B, n, nrhs, lead, (cls, cls, cls, cls == 'D')), L)


# ====================================================================================================== factorisation
def _potrf(ctx, v, n):
    info = C.c_int(-7)
    assert ctx.lib.gpk_potrf(ctx.h, v.ptr, n, v.ld, C.byref(info)) == 0
    return info.value


@functools.lru_cache(maxsize=None)
def _potrf_case(n):
    A = _spd(np.random.RandomState(n), n)
    return A, VA.ref_cholesky(A)


@pytest.mark.parametrize('cls', VA.CLASSES)
@pytest.mark.parametrize('n', [1, 5, 63, 64, 65, 130, 333, 577])        # 577 crosses the 512-column outer block
def test_potrf_views(ctx, mk, n, cls):
    """Factor, residual and reference; the lower triangle does not depend on what the upper triangle of the input holds; on return
    the strict upper triangle of the view is UNSPECIFIED (include/gpk.h: the blocked updates write whole tiles above the diagonal of
    the diagonal blocks -- measured on an MI355X with the symmetric input: 0 strict-upper entries changed up to order 129, 1 of 8385
    at order 130, 20910 of 55278 at 333, 75552 of 166176 at 577, the same in classes A and D), and nothing outside the n x n view is
    written."""
    A, Lref = _potrf_case(n)
    v = mk.mat(n, n, cls, A)
    assert _potrf(ctx, v, n) == 0
    mk.check([v])
    got = get(v)
    L = np.tril(got)
    assert not np.isnan(L).any()
    LLt = VA.ref_matmul(L, L.T)
    assert VA.fro(LLt - A) <= 1e-13 * VA.fro(A)
    assert VA.fro(L - Lref) <= 1e-11 * VA.fro(Lref)
    w = mk.mat(n, n, cls, VA.with_canary_upper(A))                      # the factorisation does not read the upper triangle
    assert _potrf(ctx, w, n) == 0
    mk.check([v, w])
    L2 = np.tril(get(w))
    assert not np.isnan(L2).any()
    assert np.array_equal(VA.bits(L), VA.bits(L2))


@functools.lru_cache(maxsize=None)
def _panel_case(nrows, ncols):
    rng = np.random.RandomState(nrows + ncols)
    P = np.vstack([_spd(rng, ncols), rng.normal(size=(nrows - ncols, ncols))])
    L11 = VA.ref_cholesky(P[:ncols])
    return P, L11, VA.ref_right_lt(L11, P[ncols:])


def _panel_mask(nrows, ncols):
    """output region of a panel step that carries a contract: lower triangle of the top block, every row below"""
    return np.arange(nrows)[:, None] >= np.arange(ncols)[None, :]


@pytest.mark.parametrize('cls', VA.CLASSES)
@pytest.mark.parametrize('entry', ['panel', 'panel_at'])
@pytest.mark.parametrize('nrows,ncols', [(64, 64), (65, 1), (300, 64), (333, 130), (640, 512), (600, 257)])
def test_potrf_panel_views(ctx, mk, nrows, ncols, entry, cls):
    """top block = chol(A11), rows below = A21 L11^{-T}; independent of the strict upper triangle of A11; nothing outside the
    nrows x ncols view written"""
    P, L11ref, Xref = _panel_case(nrows, ncols)

    def run(data):
        v = mk.mat(nrows, ncols, cls, data)
        if entry == 'panel':
            info = C.c_int(-7)
            assert ctx.lib.gpk_potrf_panel(ctx.h, v.ptr, nrows, ncols, v.ld, C.byref(info)) == 0
        else:
            info = C.c_int(-7)
            assert ctx.lib.gpk_info_reset(ctx.h) == 0
            assert ctx.lib.gpk_potrf_panel_at(ctx.h, v.ptr, nrows, ncols, v.ld, 1000) == 0
            assert ctx.lib.gpk_info_read(ctx.h, C.byref(info)) == 0
        assert info.value == 0
        mk.check([v])
        return get(v)

    got = run(P)
    mask = _panel_mask(nrows, ncols)
    assert not np.isnan(got[mask]).any()
    L11, X = np.tril(got[:ncols]), got[ncols:]
    A11 = P[:ncols]
    assert VA.fro(VA.ref_matmul(L11, L11.T) - A11) <= 1e-13 * VA.fro(A11)
    assert VA.fro(L11 - L11ref) <= 1e-11 * VA.fro(L11ref)
    if nrows > ncols:
        _assert_residual(L11, X, P[ncols:], 'R', 'panel rows below')
    Pn = P.copy()
    Pn[:ncols] = VA.with_canary_upper(P[:ncols])
    got2 = run(Pn)
    assert np.array_equal(VA.bits(got[mask]), VA.bits(got2[mask]))


@functools.lru_cache(maxsize=None)
def _spd577():
    return _spd(np.random.RandomState(577), 577)


@pytest.mark.parametrize('cls', ['A', 'D'])
@pytest.mark.parametrize('bad', [(0,), (63,), (64,), (511,), (512,), (576,), (100, 300), (64, 65)], ids=lambda b: 'j' + '_'.join(map(str, b)))
def test_potrf_info_index(ctx, mk, bad, cls):
    """leading minor SPD, then A[j, j] = -1: info = j + 1 (1-based) -- first column, last column, either side of the 64-column panel
    and of the 512-column outer block; two bad pivots: the first wins"""
    n = 577
    A = _spd577().copy()
    for j in bad:
        A[j, j] = -1.0
    v = mk.mat(n, n, cls, A)
    assert _potrf(ctx, v, n) == bad[0] + 1
    mk.check([v])
    j = bad[0]
    if j:                                                               # the columns in front of the bad pivot are the factor of the minor
        L = np.tril(get(v))[:j, :j]
        assert VA.fro(VA.ref_matmul(L, L.T) - A[:j, :j]) <= 1e-13 * VA.fro(A[:j, :j])


@pytest.mark.parametrize('cls', ['A', 'D'])
def test_panel_info_word(ctx, mk, cls):
    """gpk_potrf_panel_at accumulates in the handle's info word: pivot_base offsets the index, the first failure is kept across
    calls, gpk_info_reset clears it, a clean panel after a reset reads 0; gpk_potrf_panel(host_info = NULL) does not fail"""
    nrows, ncols = 300, 64
    P, _, _ = _panel_case(nrows, ncols)
    lib, h = ctx.lib, ctx.h
    info = C.c_int(-7)

    def panel(j, base):
        Q = P.copy()
        if j is not None:
            Q[j, j] = -1.0
        v = mk.mat(nrows, ncols, cls, Q)
        assert lib.gpk_potrf_panel_at(h, v.ptr, nrows, ncols, v.ld, base) == 0
        return v

    assert lib.gpk_info_reset(h) == 0
    v1 = panel(10, 1000)
    assert lib.gpk_info_read(h, C.byref(info)) == 0 and info.value == 1011
    v2 = panel(5, 2000)                                                 # no reset in between: the first failure is kept
    assert lib.gpk_info_read(h, C.byref(info)) == 0 and info.value == 1011
    assert lib.gpk_info_reset(h) == 0
    assert lib.gpk_info_read(h, C.byref(info)) == 0 and info.value == 0
    v3 = panel(5, 2000)
    assert lib.gpk_info_read(h, C.byref(info)) == 0 and info.value == 2006
    assert lib.gpk_info_reset(h) == 0
    v4 = panel(None, 3000)
    assert lib.gpk_info_read(h, C.byref(info)) == 0 and info.value == 0
    v5 = mk.mat(nrows, ncols, cls, P)
    assert lib.gpk_potrf_panel(h, v5.ptr, nrows, ncols, v5.ld, None) == 0      # host_info = NULL: no host synchronisation
    ctx.synchronize()
    assert np.array_equal(VA.bits(get(v5)[_panel_mask(nrows, ncols)]), VA.bits(get(v4)[_panel_mask(nrows, ncols)]))
    Q = P.copy(); Q[63, 63] = -1.0                                      # last column of the panel, through the host_info path
    v6 = mk.mat(nrows, ncols, cls, Q)
    assert lib.gpk_potrf_panel(h, v6.ptr, nrows, ncols, v6.ld, C.byref(info)) == 0 and info.value == 64
    mk.check([v1, v2, v3, v4, v5, v6])


# ===================================================================================================== argument checks
def test_argument_checks_refuse_without_writing(ctx, mk):
    """each: a return code < 0 and no write (canaries and operands intact)"""
    lib, h = ctx.lib, ctx.h
    n, nrhs = 40, 12
    rng = np.random.RandomState(0)
    vL = mk.mat(n, n, 'A', _well_conditioned_L(rng, n))
    vB = mk.mat(n, nrhs, 'A', rng.normal(size=(n, nrhs)))
    vX = mk.mat(n, nrhs, 'A', np.zeros((n, nrhs)))
    vD = mk.flat(n, 256, 0)
    vP = mk.mat(n, n, 'D', _spd(rng, n))
    vx, vy = mk.vec(n, 0, rng.normal(size=n)), mk.vec(n, 1, rng.normal(size=n))
    info = C.c_int(-7)
    L, B, X, D, P = vL.ptr, vB.ptr, vX.ptr, vD.ptr, vP.ptr
    ldl, ldb, ldx, ldp = vL.ld, vB.ld, vX.ld, vP.ld
    calls = {
        'trsm ldl < n': lambda: lib.gpk_trsm(h, 0, L, n, n - 1, B, nrhs, ldb),
        'trsm ldb < nrhs': lambda: lib.gpk_trsm(h, 1, L, n, ldl, B, nrhs, nrhs - 1),
        'trsm L null': lambda: lib.gpk_trsm(h, 0, None, n, ldl, B, nrhs, ldb),
        'trsm B null': lambda: lib.gpk_trsm(h, 0, L, n, ldl, None, nrhs, ldb),
        'trsm null handle': lambda: lib.gpk_trsm(None, 0, L, n, ldl, B, nrhs, ldb),
        'trsm n < 0': lambda: lib.gpk_trsm(h, 0, L, -1, ldl, B, nrhs, ldb),
        'trsm_lz ldl < n': lambda: lib.gpk_trsm_lz(h, L, n, n - 1, B, nrhs, ldb, 5),
        'trsm_lz ldb < nrhs': lambda: lib.gpk_trsm_lz(h, L, n, ldl, B, nrhs, nrhs - 1, 5),
        'trsm_lz B null': lambda: lib.gpk_trsm_lz(h, L, n, ldl, None, nrhs, ldb, 5),
        'potrs ldl < n': lambda: lib.gpk_potrs(h, L, n, n - 1, B, nrhs, ldb),
        'potrs ldb < nrhs': lambda: lib.gpk_potrs(h, L, n, ldl, B, nrhs, nrhs - 1),
        'potrs L null': lambda: lib.gpk_potrs(h, None, n, ldl, B, nrhs, ldb),
        'trsm_right_lt ldl < n': lambda: lib.gpk_trsm_right_lt(h, L, n, n - 1, P, n, ldp),
        'trsm_right_lt ldx < n': lambda: lib.gpk_trsm_right_lt(h, L, n, ldl, P, n, n - 1),
        'trsm_right_lt X null': lambda: lib.gpk_trsm_right_lt(h, L, n, ldl, None, n, ldp),
        'trtri_diag ldl < n': lambda: lib.gpk_trtri_diag(h, L, n, n - 1, D, 256),
        'trtri_diag block': lambda: lib.gpk_trtri_diag(h, L, n, ldl, D, 100),
        'trtri_diag Dinv null': lambda: lib.gpk_trtri_diag(h, L, n, ldl, None, 256),
        'trsm_dinv ldb < nrhs': lambda: lib.gpk_trsm_dinv(h, L, D, 256, n, ldl, B, nrhs, nrhs - 1, X, ldx, 0),
        'trsm_dinv ldx < nrhs': lambda: lib.gpk_trsm_dinv(h, L, D, 256, n, ldl, B, nrhs, ldb, X, nrhs - 1, 0),
        'trsm_dinv ldl < n': lambda: lib.gpk_trsm_dinv(h, L, D, 256, n, n - 1, B, nrhs, ldb, X, ldx, 0),
        'trsm_dinv X aliases B': lambda: lib.gpk_trsm_dinv(h, L, D, 256, n, ldl, B, nrhs, ldb, B, ldb, 0),
        'trsm_dinv X null': lambda: lib.gpk_trsm_dinv(h, L, D, 256, n, ldl, B, nrhs, ldb, None, ldx, 0),
        'potrf lda < n': lambda: lib.gpk_potrf(h, P, n, n - 1, C.byref(info)),
        'potrf A null': lambda: lib.gpk_potrf(h, None, n, ldp, C.byref(info)),
        'potrf_panel nrows < ncols': lambda: lib.gpk_potrf_panel(h, P, n - 1, n, ldp, C.byref(info)),
        'potrf_panel lda < ncols': lambda: lib.gpk_potrf_panel(h, P, n, n, n - 1, C.byref(info)),
        'potrf_panel A null': lambda: lib.gpk_potrf_panel(h, None, n, n, ldp, C.byref(info)),
        'potrf_panel_at nrows < ncols': lambda: lib.gpk_potrf_panel_at(h, P, n - 1, n, ldp, 0),
        'potrf_panel_at pivot_base < 0': lambda: lib.gpk_potrf_panel_at(h, P, n, n, ldp, -1),
        'potrf_panel_at A null': lambda: lib.gpk_potrf_panel_at(h, None, n, n, ldp, 0),
        'info_read null': lambda: lib.gpk_info_read(h, None),
        'info_reset null handle': lambda: lib.gpk_info_reset(None),
        'tril lda < n': lambda: lib.gpk_tril(h, P, n, n - 1),
        'tril A null': lambda: lib.gpk_tril(h, None, n, ldp),
        'symmetrize_lower lda < n': lambda: lib.gpk_symmetrize_lower(h, P, n, n - 1),
        'symmetrize_lower A null': lambda: lib.gpk_symmetrize_lower(h, None, n, ldp),
        'gemm A null': lambda: lib.gpk_gemm(h, 0, 0, n, nrhs, n, 1.0, None, ldl, B, ldb, 0.0, X, ldx),
        'gemm B null': lambda: lib.gpk_gemm(h, 0, 0, n, nrhs, n, 1.0, L, ldl, None, ldb, 0.0, X, ldx),
        'gemm C null': lambda: lib.gpk_gemm(h, 0, 0, n, nrhs, n, 1.0, L, ldl, B, ldb, 0.0, None, ldx),
        'gemm k < 0': lambda: lib.gpk_gemm(h, 0, 0, n, nrhs, -1, 1.0, L, ldl, B, ldb, 0.0, X, ldx),
        'gemm_lz C null': lambda: lib.gpk_gemm_lz(h, 0, n, nrhs, n, 1.0, L, ldl, B, ldb, 0.0, None, ldx, 3),
        'syrk A null': lambda: lib.gpk_syrk(h, n, n, 1.0, None, ldl, 0.0, P, ldp, 1),
        'syrk C null': lambda: lib.gpk_syrk(h, n, n, 1.0, L, ldl, 0.0, None, ldp, 0),
        'axpy x null': lambda: lib.gpk_axpy(h, n, 1.0, None, vy.ptr),
        'axpy y null': lambda: lib.gpk_axpy(h, n, 1.0, vx.ptr, None),
        'axpy n < 0': lambda: lib.gpk_axpy(h, -1, 1.0, vx.ptr, vy.ptr),
    }
    for name, call in calls.items():
        rc = call()
        assert rc < 0, f'{name}: returned {rc}'
    assert info.value == -7                                             # no refused call touched the host info either
    ctx.synchronize()
    mk.check([])
