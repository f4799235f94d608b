"""The entrywise gate of tests/_fused_phase_reference.py is shown to bite, on a numpy model of the phase at nc = 1101 (CPU only).

The model W (1570 x 1101, F column last) is built so that the four planted errors fall where the row rules of the sample look, not where
a seed happens to look:
  - columns 0..511, 512..1023 and 1024..1099 live on three disjoint row sets, coupled only through the first panel (columns 0..63, a
    coupling of 1e-8) and the F column: the fill-in of tile (16, 8) -- rows 1024.., the first row of block 2, columns 512..575 -- is the
    rank-64 update by panel 0 alone, of size 1e-16 of ||H||;
  - eight columns (700..707) of magnitude 1e-4 live on rows of their own where F is zero: the eight smallest-scale rows, with y = 0 and
    delta = 0 there whatever their rows of the factor hold;
  - the rows of W are ordered so that the last K chunk of the product belongs to block column 1 (columns 512..1023).
(a) and (b) pass the delta gates of _gn_reference (gate_backward, gate_forward) -- that is why the entrywise gate exists."""
import types

import numpy as np
import pytest

import _fused_phase_reference as FP
import _gn_reference as R

LD = R.LD
NC, NZ = 1101, 1100
SMALL = np.arange(700, 708)
WIDTHS = [(512, 512), (128, 256), (64, 192)]         # defaults, {28: 128, 29: 256}, {28: 64, 29: 192}


def _model(theta=1e-8):
    rng = np.random.RandomState(1101)
    r1, r3, r4, r2 = slice(0, 700), slice(700, 850), slice(850, 870), slice(870, 1570)
    W = np.zeros((1570, NC))
    W[r1, :512] = rng.normal(size=(700, 512))
    c2 = np.setdiff1d(np.arange(512, 1024), SMALL)
    W[870:1570, c2] = rng.normal(size=(700, c2.size))
    W[r3, 1024:NZ] = rng.normal(size=(150, NZ - 1024))
    W[850:870, SMALL] = 1e-4 * rng.normal(size=(20, SMALL.size))
    W[r2, :64] += theta * rng.normal(size=(700, 64))
    W[r3, :64] += theta * rng.normal(size=(150, 64))
    for r in (r1, r2, r3):
        W[r, NZ] = rng.normal(size=r.stop - r.start)
    return W


@pytest.fixture(scope='module')
def model():
    W = _model()
    Wa = np.abs(W)
    rows = FP.sample_rows(NC, np.einsum('ki,ki->i', Wa, Wa))
    R64 = FP.host_rendition(W)
    return types.SimpleNamespace(W=W, rows=rows, R64=R64, numpy=FP.gate_ratio(W, R64, rows)[0])


@pytest.fixture(scope='module')
def vector_ref(model):
    """what gate_backward / gate_forward of _gn_reference read, for the model: g, H d, ||H||, delta in long double"""
    from scipy.linalg import solve_triangular
    Wl = model.W.astype(LD)
    A, w = Wl[:, :NZ], Wl[:, NZ]
    ref = types.SimpleNamespace()
    ref.g = LD(2) * (A.T @ w)
    ref.Hmul = lambda d: LD(2) * (A.T @ (A @ np.asarray(d).astype(LD)))
    R0 = model.R64[:NZ, :NZ]
    solve64 = lambda r: 0.5 * solve_triangular(R0, solve_triangular(R0, r, lower=True, check_finite=False), lower=True, trans='T',
                                               check_finite=False)
    ref.p64 = types.SimpleNamespace(delta=FP.delta_from_factor(model.R64))
    A64 = model.W[:, :NZ]
    ref.normH = R.norm2_power(lambda x: 2.0 * (A64.T @ (A64 @ x)), NZ)
    ref.delta = R.refine(solve64, lambda d: ref.g - ref.Hmul(d), ref.g.astype(np.float64))
    return ref


def _delta_gates_pass(ref, Rb):
    d = FP.delta_from_factor(Rb)
    rb, ab = R.gate_backward(ref, d, ref.Hmul)
    rf, af = R.gate_forward(ref, d)
    print(f'delta gates: backward {rb:.3g} of {ab:.3g}, forward {rf:.3g} of {af:.3g}')
    return rb <= ab and rf <= af


# ------------------------------------------------------------------------------------------------ the row sample
@pytest.mark.parametrize('nc', [1025, 1027, 1088, 1101, 1536, 1537])
@pytest.mark.parametrize('w0,ob', WIDTHS)
def test_sample_holds_every_block_boundary(nc, w0, ob):
    diag = np.random.RandomState(nc).uniform(1.0, 2.0, nc)
    diag[[5, 77, 300, 301, 640, 641, 900, nc - 2]] = 1e-9
    rows = FP.sample_rows(nc, diag, w0, ob)
    assert len(rows) <= FP.MAX_ROWS == 48 and len(set(rows)) == len(rows) and rows == sorted(rows)
    b = FP.pipe_blocks(nc, w0, ob)
    assert b[0] == 0 and b[-1] == nc and all(0 < y - x <= 512 for x, y in zip(b[:-1], b[1:]))
    assert all((y - x) % 64 == 0 for x, y in zip(b[:-2], b[1:-1]))           # only the last block can be ragged
    for b0, b1 in zip(b[:-1], b[1:]):
        assert b0 in rows and b1 - 1 in rows
        if (b1 - b0) % 64:
            assert b0 + (b1 - b0) // 64 * 64 in rows
    assert nc - 1 in rows and {5, 77, 300, 301, 640, 641, 900, nc - 2} <= set(rows)
    assert rows == FP.sample_rows(nc, diag, w0, ob)                           # a fixed seed


def test_default_blocks_are_the_ones_of_the_library():
    assert FP.pipe_blocks(1101) == [0, 512, 1024, 1101] and FP.pipe_blocks(1025) == [0, 512, 1024, 1025]
    assert FP.pipe_blocks(1101, 128, 256) == [0, 128, 384, 640, 896, 1101]
    assert FP.pipe_blocks(1101, 64, 192) == [0, 64, 256, 448, 640, 832, 1024, 1101]
    assert FP.pipe_blocks(700, 100, 1000) == [0, 64, 576, 700]                # widths rounded down to panels, at most 512


def test_model_rows_fall_where_the_rules_look(model):
    assert set(SMALL) <= set(model.rows) and {512, 1023, 1024, 1088, 1100} <= set(model.rows)


# ------------------------------------------------------------------------------------------------ accepted
def test_float64_rendition_and_tile_cholesky_are_accepted(model):
    a = R.allowed(model.numpy)
    Rt = FP.tile_cholesky(model.W.T @ model.W)
    rt = FP.gate_ratio(model.W, Rt, model.rows)[0]
    print(f'\nnumpy {model.numpy:.3g}, tile Cholesky {rt:.3g}, allowed {a:.3g}')
    assert model.numpy <= a and rt <= a
    assert model.numpy < 64                                                   # the margin is 32 x a figure of a few eps, not of thousands
    # the exact zeros of the product (disjoint supports, no fill-in before panel 8 ... ) are exact zeros of the factor
    assert np.all(model.R64[SMALL, :700] == 0.0)
    r, a2, npr, _, rows = FP.gate(model.W, model.R64)
    assert rows == model.rows and npr == model.numpy and r == npr and a2 == a


# ------------------------------------------------------------------------------------------------ rejected
def test_a_relative_error_of_1e_11_in_a_smallest_scale_row(model, vector_ref):
    Rb = model.R64.copy()
    i = 703
    j = 700 + int(np.argmax(np.abs(Rb[i, 700:703])))
    Rb[i, j] *= 1.0 + 1e-11
    r, where = FP.gate_ratio(model.W, Rb, model.rows)
    print(f'\n(a) ratio {r:.3g} at {where}, allowed {R.allowed(model.numpy):.3g}')
    assert r > R.allowed(model.numpy) and where[0] == i
    assert _delta_gates_pass(vector_ref, Rb)


def test_b_rank_64_update_of_one_tile_left_out(model, vector_ref):
    H = model.W.T @ model.W
    Rb = FP.tile_cholesky(H, omit=(16, 8, 0))
    good = FP.tile_cholesky(H)
    assert np.array_equal(Rb[:1024], good[:1024]) and not np.array_equal(Rb[1024:1088, 512:576], good[1024:1088, 512:576])
    r, where = FP.gate_ratio(model.W, Rb, model.rows)
    print(f'\n(b) ratio {r:.3g} at {where}, allowed {R.allowed(model.numpy):.3g}')
    assert r > 1e6 * R.allowed(model.numpy) and 1024 <= where[0] < 1088
    # the row the rules put into the sample (first row of block 2) sees it on its own, whatever the random rows are
    assert 1024 in FP.boundary_rows(NC) and FP.gate_ratio(model.W, Rb, [1024])[0] > 1e6 * R.allowed(model.numpy)
    assert _delta_gates_pass(vector_ref, Rb)


def test_c_block_column_from_a_product_without_its_last_k_chunk(model):
    W = model.W
    H = W.T @ W
    cut = W.shape[0] - 64                                                     # the last split-K chunk: 64 rows
    H[512:, 512:1024] = W[:cut, 512:].T @ W[:cut, 512:1024]
    H[512:1024, 512:] = H[512:, 512:1024].T
    Rb = np.linalg.cholesky(H)
    r, where = FP.gate_ratio(W, Rb, model.rows)
    print(f'\n(c) ratio {r:.3g} at {where}, allowed {R.allowed(model.numpy):.3g}')
    assert r > 1e6 * R.allowed(model.numpy) and 512 <= where[0]
    # both boundary rows of the block see it
    for i in (512, 1023):
        assert FP.gate_ratio(W, Rb, [i])[0] > 1e6 * R.allowed(model.numpy)


def test_d_stray_non_zero_where_the_scale_is_zero(model):
    W0 = _model(theta=0.0)                                                    # no coupling: (W^T W)[512:1024, :512] and its scale are exact zeros
    Wa = np.abs(W0)
    rows = FP.sample_rows(NC, np.einsum('ki,ki->i', Wa, Wa))
    R0 = FP.host_rendition(W0)
    assert np.all(R0[512:1024, :512] == 0.0) and 512 in rows
    npr = FP.gate_ratio(W0, R0, rows)[0]
    assert npr <= R.allowed(npr) and np.isfinite(npr)
    # in the factor: the stray entry is its own scale, the ratio is 1 / eps-sized
    Rb = R0.copy()
    Rb[512, 5] = 1e-200
    r, where = FP.gate_ratio(W0, Rb, rows)
    print(f'\n(d) ratio {r:.3g} at {where}')
    assert r > 1e12 and where == (512, 5)
    # in the product: an error where s = 0 is refused whatever its size
    p, pm = FP.product_rows(W0, [512])[0]
    q, qm = FP.factor_rows(R0, [512])[0]
    assert pm[5] + qm[5] == 0.0 and p[5] == 0 and q[5] == 0
    err = np.abs(q - p)
    assert np.isfinite(FP.ratio_rows(err, pm + qm)[0])
    err[5] = LD(1e-300)
    assert FP.ratio_rows(err, pm + qm) == (np.inf, 5)
    # a NaN in a sampled row is refused as well
    Rb = R0.copy()
    Rb[1100, 17] = np.nan
    assert FP.gate_ratio(W0, Rb, rows)[0] == np.inf


def test_pred_gate():
    y = np.random.RandomState(3).normal(size=1100)
    r, a = FP.pred_gate(float(y @ y), y)
    assert r <= a
    r, a = FP.pred_gate(float(y @ y) * (1 + 1e-13), y)
    assert r > a


def test_gram_scale_rows_is_the_magnitude_sum_of_gram_form():
    rng = np.random.RandomState(4)
    nz = 5
    G = rng.normal(size=(4 * nz, nz))
    d = rng.normal(size=nz)
    out = FP.gram_scale_rows(G, d, [0, 3, nz], border=np.ones(nz + 1))
    assert len(out) == 3 and out[0].shape == (1,) and out[1].shape == (4,) and out[2].shape == (nz + 1,)
    c, k = 3, 2
    want = abs(d[c]) * abs(G[c, k]) * abs(d[k]) + abs(d[c]) * abs(G[nz + c, k]) + abs(G[2 * nz + c, k]) * abs(d[k]) + abs(G[3 * nz + c, k])
    assert abs(float(out[1][k]) - want) <= 1e-15 * want
