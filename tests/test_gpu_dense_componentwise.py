"""Cholesky, the triangular solves and the products ENTRY BY ENTRY, on Gram matrices and on badly row-scaled matrices.

tests/test_gpu_parity.py and tests/test_gpu_dense_views.py gate these routines norm-wise (||L L^T - A||_F <= 1e-13 ||A||_F,
||L X - B||_F <= 1e-12 ||L||_F ||X||_F) on matrices whose rows all have the same size.  The matrices the product factors are Gram
matrices whose blocks have diagonals from 1 to 1.9e6 and a condition number of 1e10 .. 1e15: an error of 1e-9 in the rows of the value
block is invisible to a norm.  Cholesky and substitution are componentwise backward stable (Higham, Thms 10.3 and 8.5); here that
property is tested for every entry, |L L^T - A|_ij <= c eps (|L||L^T|)_ij and |L X - B|_ij <= c eps (|L||X|)_ij, with residuals and
scales in long double (tests/_dense_reference.py; tests/test_dense_reference_host.py shows that these gates reject an error of 1e-11 in
one row and a stray non-zero in a structural zero, both of which the norm-wise asserts accept).

c is never fixed in advance: the same figure of the float64 host rendition (numpy.linalg.cholesky, scipy.linalg.solve_triangular with
the SAME factor, numpy's @, the inverted-block algorithm in numpy) is taken at run time and the device may take 32 x that + 1
(_gn_reference.allowed).  An entry whose scale is 0 has to be exactly 0.  Every test prints `[tag] case: device, allowed (numpy); worst
so far`.  The forward error L - L_ref is not gated here (it is governed by the conditioning; test_potrf keeps its 1e-11 on its matrices).

Families (tests/_dense_reference.py): gram = Theta + adaptive nugget 1e-8 / 1e-10 of five layouts (orders 450 .. 577, Burgers with 1200
exact zeros); graded = D (M M^T + n I) D and graded_factor = D (tril(normal) + diag(U(3, 4) sqrt n)), D = diag(10^U(-3, 3)), the factor
uploaded with its strict upper triangle and padding poisoned; right-hand sides with columns scaled by 10^U(-3, 3), one row block
scaled by 1e-6 and, for the `lead` entry points, the leading-zero profile of [A | F].  The solves run on graded_factor AND on the device's
own factor of every Gram case: the real L is what the product solves with.

What each test guards, and the kernels its orders reach (csrc/gpk_factor.hip: NB = 64 panels, SB = 256 strips, 512-column outer blocks):
  test_potrf                  gpk_potrf, default schedule: info == 0 and the lower triangle of L L^T - A.  Orders 1, 63, 64: one panel kernel
                              (partial / full); 65, 129: a second, ragged panel with the fused rank-64 update; 256, 320, 450 .. 480: several
                              panels in one outer block; 513, 520, 576, 577, 645: a second outer block after a trailing rank-512 update
                              (ragged by 1, 8, 64, 65 and 133 columns).
  test_potrf_variants         the same gate at orders 320 and 576 under the entries of test_gpu_variants.VARIANTS that reach this code: 64-row
                              base solves ({3: 0}), the rolled panel kernel ({41: 0}, which also leaves the fused schedule), forced GEMM tiles
                              ({0: 1}, {0: 3}, {0: 4}) for the rank-64 and trailing updates.
  test_potrf_2112             order 2112 = four outer blocks + a 64-column tail, one-stream schedule and {20: 100000}, the pipelined
                              left-looking factorisation of Theta; 64 sampled rows of L L^T (the 16 of smallest scale, the first row of every
                              outer block, random ones), the numpy yardstick on the same rows.
  test_potrf_panel            gpk_potrf_panel / gpk_potrf_panel_at on the leading 128 columns of graded 320 and 645 and the leading 512 of 645
                              (order 320 has no 512 columns): the top block as a factorisation, the rows below as X L11^T - A21.
  test_trsm                   gpk_trsm, trans 0 / 1, nrhs 1 (ldb > 1), 37, 130.  64: base kernel; 240, 256: strip kernel (trans 0; the base
                              kernel + recursion for trans 1); 250: base kernel + recursion; 450 .. 577: recursion over strips.
  test_trsm_lz                gpk_trsm_lz, nrhs 130, lead 129 / 64 / 100; structural zeros of the solution exactly 0.
  test_trsm_right_lt          gpk_trsm_right_lt, m 1 / 70.
  test_trsv                   the single-vector path (nrhs == 1, ldb == 1), trans 0 / 1, data-tagged hand-offs and two launches per block
                              (tune key 4 = 1 / 0).
  test_potrs                  gpk_potrs with 37 columns and with one contiguous vector, against |L|(|L^T||X|) + |L||L^T X|.
  test_trtri_diag_trsm_dinv   block 256, orders 256, 300, 520 (three blocks, ragged last), 577 and the Gram factors, lead 0 / 129: every
                              inverted block as a solve (L_kk Dinv_k - I against |L_kk||Dinv_k|, exact zeros above the diagonal), the solve
                              against the numpy rendition of the same algorithm.  The GEMM-only solve is only conditionally stable
                              (DESIGN.md section 4); on these cases its numpy rendition stays below 15 eps, so it keeps the common gate.
  test_products               gpk_gemm (four transposition cases, beta = 0 with NaN in C), gpk_gemm_lz (whole zero columns -> exact zeros in
                              C) and gpk_syrk (lower / full) at (257, 193, 100) and (130, 70, 577), rows and columns scaled: every entry
                              against |alpha||op A||op B| + |beta C|.

RESULTS (MI355X, the case of each tag that comes closest to its gate, as "device ratio of allowed (numpy)"; 159 cases, all pass):
  potrf gram                   13 of 398 (12.4)      elliptic (250, 77), nugget 1e-8
  potrf graded                 4.7 of 37.2 (1.13)    order 65
  potrf variants               13.5 of 58.5 (1.8)    order 576, rolled panel kernel ({41: 0})
  potrf 2112                   5.5 of 61.5 (1.89)    one-stream schedule
  panel top / below            5.46 of 43.2 (1.32) / 5.28 of 81.5 (2.52)
  trsm N  graded_factor / gram 5.07 of 24.6 (0.738) / 1.98 of 24.3 (0.729)
  trsm T  graded_factor / gram 5.03 of 61.5 (1.89) / 7.12 of 90.2 (2.79)
  trsm_lz graded_factor / gram 11.1 of 85.7 (2.65) / 2.99 of 49.3 (1.51)
  trsm_right_lt                5.02 of 38.1 (1.16) / 2.9 of 37.8 (1.15)
  trsv N  graded_factor / gram 3.15 of 24.6 (0.738) / 2.04 of 24.3 (0.729)
  trsv T  graded_factor / gram 2.99 of 96.3 (2.98) / 4.51 of 85 (2.62)
  potrs   graded_factor / gram 3.78 of 48.3 (1.48) / 0.66 of 6.31 (0.166)
  trtri_diag                   3.75 of 115 (3.57) / 2.19 of 64 (1.97)
  trsm_dinv graded_factor/gram 3.29 of 93.3 (2.89) / 11.3 of 254 (7.91, Eikonal at nugget 1e-10)
  product gemm / gemm_lz / syrk  2.01 of 29.2 (0.88) / 2.14 of 32.1 (0.972) / 8.13 of 129 (4.01)
No kernel missed its gate: the device stays within 14 eps of the componentwise scale everywhere, a factor 4 .. 30 inside the gates.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import _dense_reference as D
from test_gpu_variants import DEFAULTS, VARIANTS

pytestmark = pytest.mark.gpu

WORST = {}
GRAM = D.gram_cases()
POTRF_VARIANTS = [(name, v) for name, v in VARIANTS if v in ({3: 0}, {41: 0}, {0: 1}, {0: 3}, {0: 4})]
assert len(POTRF_VARIANTS) == 5


@pytest.fixture(scope='module')
def ctx():
    import gpk
    c = gpk.Context(0)
    yield c
    c.close()


def _note(tag, what, r, a, r_np):
    w = WORST.setdefault(tag, (0.0, 0.0, a, r_np))
    if not r / a < w[0]:
        WORST[tag] = (r / a, r, a, r_np)
    print(f'[{tag}] {what}: device {r:.3g}, allowed {a:.3g} (numpy {r_np:.3g}); worst so far {WORST[tag][1]:.3g} of {WORST[tag][2]:.3g}')


def _gate(bad, tag, what, dev, r_np, zeros=None):
    r, a, ok = D.gate(dev, r_np, zeros)
    _note(tag, what, r, a, r_np)
    if not ok:
        bad.append(f'{tag} {what}: {r:.4g} > {a:.4g}')


# ------------------------------------------------------------------------------------------------------------- operands
def _matrix(src):
    return D.gram(*src[1]) if src[0] == 'gram' else D.graded(src[1])


def _src_id(src):
    return f'{src[0]}-{D.gram_id(src[1])}' if src[0] == 'gram' else f'{src[0]}-{src[1]}'


def _factor_device(ctx, A):
    dA = ctx.array(A)
    info = ctx.potrf(dA)
    L = dA.download().reshape(A.shape)                                 # (order 1 comes back as a vector)
    dA.free()
    return info, L


def _upload_factor(ctx, L):
    """strict upper triangle and the padding of the ld = n + 16 buffer poisoned"""
    n = L.shape[0]
    d = ctx.empty(n, n + D.LD_PAD, ld=n + D.LD_PAD)
    d.upload(D.poisoned(L))
    d.cols = n
    return d


def _upload(ctx, B, ld=None):
    B = np.asarray(B)
    if B.ndim == 1:
        return ctx.array(B)
    return ctx.empty(B.shape[0], B.shape[1], ld=ld).upload(B)


GRAM_FACTORS = {}


def _factor(ctx, src):
    """the lower-triangular factor of a solve test: graded_factor, or the DEVICE's factor of a Gram case (default schedule)"""
    if src[0] == 'graded_factor':
        return np.asarray(D.graded_factor(src[1]))
    if src[1] not in GRAM_FACTORS:
        info, L = _factor_device(ctx, D.gram(*src[1]))
        assert info == 0
        GRAM_FACTORS[src[1]] = D.lower(L)
    return GRAM_FACTORS[src[1]]


SOLVE_SOURCES = [('graded_factor', n) for n in D.FACTOR_ORDERS] + [('gram', c) for c in GRAM]
DINV_SOURCES = [('graded_factor', n) for n in D.DINV_ORDERS] + [('gram', c) for c in GRAM]


@functools.lru_cache(maxsize=None)
def _np_potrf_ratio(src, ncols=None):
    A = _matrix(src)
    A = A if ncols is None else A[:ncols, :ncols]
    return D.worst(*D.res_cholesky(D.np_cholesky(A), A))


# ---------------------------------------------------------------------------------------------------------------- potrf
POTRF_SOURCES = [('gram', c) for c in GRAM] + [('graded', n) for n in D.GRADED_ORDERS]


def _check_potrf(ctx, src, tag, what):
    A = _matrix(src)
    info, L = _factor_device(ctx, A)
    bad = [] if info == 0 else [f'{what}: info = {info}']
    _gate(bad, tag, what, D.res_cholesky(L, A), _np_potrf_ratio(src))
    return bad


@pytest.mark.parametrize('src', POTRF_SOURCES, ids=_src_id)
def test_potrf(ctx, src):
    print()
    bad = _check_potrf(ctx, src, f'potrf {src[0]}', _src_id(src))
    assert not bad, bad


def _set(ctx, variant):
    for k, v in DEFAULTS.items():
        ctx.lib.gpk_debug_set(k, v)
    for k, v in variant.items():
        ctx.lib.gpk_debug_set(k, v)


@pytest.mark.parametrize('name,variant', POTRF_VARIANTS, ids=[str(v) for _, v in POTRF_VARIANTS])
@pytest.mark.parametrize('n', [320, 576])
def test_potrf_variants(dev_ctx, n, name, variant):
    print()
    try:
        _set(dev_ctx, variant)
        bad = _check_potrf(dev_ctx, ('graded', n), 'potrf variants', f'graded {n} {name}')
    finally:
        _set(dev_ctx, {})
    assert not bad, bad


@functools.lru_cache(maxsize=None)
def _case_2112():
    n = 2112
    A = D.graded(n)
    rng = np.random.RandomState(n)
    small = np.argsort(np.max(np.abs(A), axis=1))[:16]
    first = np.arange(0, n, D.OB)
    rest = np.setdiff1d(np.arange(n), np.concatenate([small, first]))
    rows = np.sort(np.concatenate([small, first, rng.choice(rest, 64 - small.size - first.size, replace=False)]))
    assert rows.size == 64 and np.unique(rows).size == 64
    return A, rows, D.worst(*D.res_cholesky(D.np_cholesky(A), A, rows))


@pytest.mark.parametrize('variant', [{}, {20: 100000}], ids=['one-stream', 'pipelined'])
def test_potrf_2112(dev_ctx, variant):
    A, rows, r_np = _case_2112()
    print()
    try:
        _set(dev_ctx, variant)
        info, L = _factor_device(dev_ctx, A)
    finally:
        _set(dev_ctx, {})
    bad = [] if info == 0 else [f'info = {info}']
    _gate(bad, 'potrf 2112', f'graded 2112 {variant} (64 rows)', D.res_cholesky(L, A, rows), r_np)
    assert not bad, bad


@pytest.mark.parametrize('entry', ['panel', 'panel_at'])
@pytest.mark.parametrize('n,ncols', [(320, 128), (645, 128), (645, 512)])
def test_potrf_panel(ctx, n, ncols, entry):
    A = D.graded(n)
    P = np.ascontiguousarray(A[:, :ncols])
    dP = _upload(ctx, P)
    info = C.c_int(-7)
    if entry == 'panel':
        ctx._chk(ctx.lib.gpk_potrf_panel(ctx.h, dP.ptr, n, ncols, dP.ld, C.byref(info)))
    else:
        ctx._chk(ctx.lib.gpk_info_reset(ctx.h))
        ctx._chk(ctx.lib.gpk_potrf_panel_at(ctx.h, dP.ptr, n, ncols, dP.ld, 1000))
        ctx._chk(ctx.lib.gpk_info_read(ctx.h, C.byref(info)))
    got = dP.download()
    dP.free()
    print()
    bad = [] if info.value == 0 else [f'info = {info.value}']
    L11, X, A21 = D.lower(got[:ncols]), got[ncols:], P[ncols:]
    _gate(bad, 'panel top', f'graded {n} x {ncols} {entry}', D.res_cholesky(L11, P[:ncols]), _np_potrf_ratio(('graded', n), ncols))
    r_np = D.worst(*D.res_solve('R', L11, D.np_solve('R', L11, A21), A21))
    _gate(bad, 'panel below', f'graded {n} x {ncols} {entry}', D.res_solve('R', L11, X, A21), r_np)
    assert not bad, bad


# --------------------------------------------------------------------------------------------------------------- solves
def _np_ratio(kind, L, B):
    return D.worst(*D.res_solve(kind, L, D.np_solve(kind, L, B), B))


@pytest.mark.parametrize('trans', [0, 1])
@pytest.mark.parametrize('src', SOLVE_SOURCES, ids=_src_id)
def test_trsm(ctx, src, trans):
    L = _factor(ctx, src)
    n, kind = L.shape[0], 'NT'[trans]
    dL = _upload_factor(ctx, L)
    bad = []
    print()
    for nrhs in D.NRHS:
        B = D.rhs(n, nrhs)
        dB = _upload(ctx, B, ld=3 if nrhs == 1 else None)              # one column with ldb > 1: the matrix kernels
        assert dB.ld > 1
        ctx.trsm(dL, dB, trans=bool(trans), n=n, nrhs=nrhs)
        X = dB.download().reshape(n, nrhs)
        dB.free()
        _gate(bad, f'trsm {kind} {src[0]}', f'{_src_id(src)} nrhs {nrhs}', D.res_solve(kind, L, X, B), _np_ratio(kind, L, B))
    dL.free()
    assert not bad, bad


@pytest.mark.parametrize('src', SOLVE_SOURCES, ids=_src_id)
def test_trsm_lz(ctx, src):
    L = _factor(ctx, src)
    n, nrhs = L.shape[0], 130
    dL = _upload_factor(ctx, L)
    bad = []
    print()
    for lead in (nrhs - 1, 64, 100):
        B = D.rhs(n, nrhs, lead)
        dB = _upload(ctx, B)
        ctx._chk(ctx.lib.gpk_trsm_lz(ctx.h, dL.ptr, n, dL.ld, dB.ptr, nrhs, dB.ld, lead))
        X = dB.download()
        dB.free()
        _gate(bad, f'trsm_lz {src[0]}', f'{_src_id(src)} lead {lead}', D.res_solve('N', L, X, B), _np_ratio('N', L, B),
              zeros=X[D.lead_mask(n, nrhs, lead)])
    dL.free()
    assert not bad, bad


@pytest.mark.parametrize('src', SOLVE_SOURCES, ids=_src_id)
def test_trsm_right_lt(ctx, src):
    L = _factor(ctx, src)
    n = L.shape[0]
    dL = _upload_factor(ctx, L)
    bad = []
    print()
    for m in (1, 70):
        B = D.rhs(m, n)
        dX = _upload(ctx, B)
        ctx._chk(ctx.lib.gpk_trsm_right_lt(ctx.h, dL.ptr, n, dL.ld, dX.ptr, m, dX.ld))
        X = dX.download().reshape(m, n)
        dX.free()
        _gate(bad, f'trsm_right_lt {src[0]}', f'{_src_id(src)} m {m}', D.res_solve('R', L, X, B), _np_ratio('R', L, B))
    dL.free()
    assert not bad, bad


@pytest.mark.parametrize('mode', [1, 0], ids=['tagged', 'two-launch'])
@pytest.mark.parametrize('src', SOLVE_SOURCES, ids=_src_id)
def test_trsv(dev_ctx, src, mode):
    ctx = dev_ctx
    L = _factor(ctx, src)
    n = L.shape[0]
    b = np.asarray(D.rhs(n, 1))[:, 0]
    dL = _upload_factor(ctx, L)
    bad = []
    print()
    try:
        _set(ctx, {4: mode})
        for trans in (0, 1):
            db = ctx.array(b)                                           # contiguous vector: the single-vector path
            assert db.ld == 1
            ctx.trsm(dL, db, trans=bool(trans), n=n, nrhs=1)
            x = db.download()
            db.free()
            kind = 'NT'[trans]
            _gate(bad, f'trsv {kind} {src[0]}', f'{_src_id(src)} key 4 = {mode}', D.res_solve(kind, L, x, b), _np_ratio(kind, L, b[:, None]))
    finally:
        _set(ctx, {})
    dL.free()
    assert not bad, bad


@pytest.mark.parametrize('src', SOLVE_SOURCES, ids=_src_id)
def test_potrs(ctx, src):
    L = _factor(ctx, src)
    n = L.shape[0]
    dL = _upload_factor(ctx, L)
    bad = []
    print()
    for nrhs in (37, 1):
        B = D.rhs(n, nrhs)
        dB = _upload(ctx, B[:, 0] if nrhs == 1 else B)                  # one contiguous vector: two single-vector solves
        ctx.potrs(dL, dB, n=n, nrhs=nrhs)
        X = dB.download().reshape(n, nrhs)
        dB.free()
        _gate(bad, f'potrs {src[0]}', f'{_src_id(src)} nrhs {nrhs}', D.res_solve('P', L, X, B), _np_ratio('P', L, B))
    dL.free()
    assert not bad, bad


@pytest.mark.parametrize('src', DINV_SOURCES, ids=_src_id)
def test_trtri_diag_trsm_dinv(ctx, src):
    L = _factor(ctx, src)
    n, nrhs, block = L.shape[0], 130, D.DINV_BLOCK
    dL = _upload_factor(ctx, L)
    Dd = ctx.trtri_diag(dL, n=n, block=block)
    Dh = Dd.download()
    Dn = D.np_trtri_diag(L, block)
    bad = []
    print()
    e, s, above = D.res_dinv_blocks(L, Dh, block)
    e_np, s_np, _ = D.res_dinv_blocks(L, Dn, block)
    _gate(bad, f'trtri_diag {src[0]}', _src_id(src), (e, s), D.worst(e_np, s_np), zeros=above)
    for lead in (0, nrhs - 1):
        B = D.rhs(n, nrhs, lead)
        dB, dX = _upload(ctx, B), ctx.empty(n, nrhs)
        dX.zero()                                                       # (lead > 0: the zero part of X is not written)
        ctx.trsm_dinv(dL, Dd, dB, dX, n=n, nrhs=nrhs, lead=lead)
        X = dX.download()
        dB.free(); dX.free()
        r_np = D.worst(*D.res_solve('N', L, D.np_solve_dinv(L, Dn, B, block), B))
        _gate(bad, f'trsm_dinv {src[0]}', f'{_src_id(src)} lead {lead}', D.res_solve('N', L, X, B), r_np,
              zeros=X[D.lead_mask(n, nrhs, lead)])
    assert np.array_equal(Dd.download(), Dh)                            # the solve only reads Dinv
    Dd.free(); dL.free()
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------- products
@pytest.mark.parametrize('m,n,k', D.PRODUCT_SHAPES)
def test_products(ctx, m, n, k):
    bad = []
    print()
    for case in D.product_cases(m, n, k):
        entry, alpha, beta, C0 = case['entry'], case['alpha'], case['beta'], case['C0']
        dA = _upload(ctx, case['A'])
        dC = _upload(ctx, C0 if beta != 0.0 else np.full(C0.shape, np.nan))        # beta = 0: C must not be read
        lower_only = False
        if entry == 'syrk':
            ctx.syrk(m, k, alpha, dA, beta, dC, full=bool(case['full']))
            lower_only = not case['full']
        else:
            dB = _upload(ctx, case['B'])
            if entry == 'gemm':
                ctx.gemm(case['ta'], case['tb'], m, n, k, alpha, dA, dB, beta, dC)
            else:
                ctx._chk(ctx.lib.gpk_gemm_lz(ctx.h, case['ta'], m, n, k, alpha, dA.ptr, dA.ld, dB.ptr, dB.ld, beta, dC.ptr, dC.ld, case['lead']))
            dB.free()
        got = dC.download()
        dA.free(); dC.free()
        err, scale = D.res_product(case['opA'], case['opB'], alpha, beta, C0, got)
        e_np, s_np = D.res_product(case['opA'], case['opB'], alpha, beta, C0, D.np_product(case))
        if lower_only:
            keep = np.tri(m, dtype=bool)
            err, scale, e_np, s_np = (np.where(keep, v, 0) for v in (err, scale, e_np, s_np))
        elif entry == 'syrk' and not np.array_equal(got, got.T):
            bad.append(f'{case["name"]}: C is not exactly symmetric')
        _gate(bad, f'product {entry}', f'{case["name"]} {(m, n, k)}', (err, scale), D.worst(e_np, s_np))
    assert not bad, bad
