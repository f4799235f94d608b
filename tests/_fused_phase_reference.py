"""Entrywise backward-error gate of the fused product + Cholesky phase of the Gauss-Newton step (CPU only).

The phase turns the solved block W = [L^-1 A(z) | L^-1 F(z)] into the factored bordered matrix Hb = chol(W^T W): gpk_i_syrk_potrf ->
potrf_pipelined (csrc/gpk_factor.hip), Darcy's own assembly of H and the two Gram-level modes (csrc/gpk_gn.hip).  The operand is taken as
given -- the float64 W the device itself solved -- so the gate measures the phase alone and needs no O(N^2 n_z) long-double solve.

For the sampled rows i of the lower triangle and every j <= i, with R = tril(Hb):

    E_ij = |(R R^T)_ij - (W^T W)_ij|          in long double
    s_ij = (|R| |R^T|)_ij + (|W|^T |W|)_ij     (+ what a caller adds, see gram_scale_rows)
    ratio = max E_ij / (eps s_ij),             an entry with s_ij = 0 has to be exactly 0

The scales are evaluated by float64 BLAS products of the magnitudes (all terms positive: a relative error of n eps of a SCALE); the error
terms are long double throughout.  The constant is not fixed: the same figure of the float64 host rendition on the same W (BLAS W^T W,
numpy.linalg.cholesky) is computed at run time and the device may take _gn_reference.allowed() of it, i.e. 32 x that + 1.

Row sample (sample_rows), at most MAX_ROWS = 48: the border row nc - 1; the first and the last row of every column block of the
pipelined schedule (pipe_blocks, the function of that name in csrc/gpk_factor.hip); the first row of every 64-column panel that starts a
ragged tail of a block; the 8 rows with the smallest (|W|^T |W|)_ii; random rows from a fixed seed to fill up.

A stray non-zero of R can never meet s_ij = 0 -- (|R| |R^T|)_ij >= |R_ij| R_jj -- so it is rejected through the ratio (about 1 / (2 eps));
the s = 0 rule guards a product entry that has to be an exact zero (disjoint supports) against a factor row that is not: it is what
ratio_rows returns inf for.  tests/test_fused_phase_host.py shows both.
"""
import hashlib
import zlib

import numpy as np

import _gn_reference as R

LD, EPS = R.LD, R.EPS
MAX_ROWS = 48
PANEL = 64                                       # NB of csrc/gpk_factor.hip
SMALLEST = 8
NB_FUSED = 40                                    # boundary count of the cases of tests/test_gpu_fused_phase.py


# ------------------------------------------------------------------------------------------------ cases
class Case(R.Case):
    """_gn_reference.Case (same construction, same attribute names) at a free (N_d, N_b, N_data); seeded per (system, N_d, N_b)"""

    def __init__(self, system, Nd, Nb=NB_FUSED, Ndata=None):
        self.system, self.Nd, self.Nb = system, Nd, Nb
        self.Ndata = (min(60, Nd) if Ndata is None else Ndata) if system == 'darcy' else 0
        self.p0, self.p1, self.lam = R.PARAMS[system]
        rng = np.random.RandomState(zlib.crc32(repr((system, Nd, Nb, 'fused')).encode()))
        self.f = rng.uniform(0.5, 1.5, Nd)
        self.g = rng.uniform(0.5, 1.5, Nb)
        self.data = rng.uniform(0.5, 1.5, self.Ndata) if system == 'darcy' else None
        self.nz = R.n_unknowns(system, Nd)
        self.z0 = rng.uniform(0.3, 1.2, self.nz) * rng.choice([-1.0, 1.0], self.nz)
        n = R.factor_order(system, Nd, Nb)
        self.L = R.synthetic_factor(rng, n)
        self.L2 = R.synthetic_factor(rng, 3 * Nd) if system == 'darcy' else None
        if system == 'darcy':
            self.groups = [(0, 3 * Nd, self.L2), (3 * Nd, n, self.L), (3 * Nd + n, self.Ndata, None)]
        elif system == 'relaxed':
            self.groups = [(0, n, self.L), (n, Nd, None)]
        else:
            self.groups = [(0, n, self.L)]
        self.rows = sum(g[1] for g in self.groups)


_CASES = {}


def case(system, Nd):
    """the shared case of (system, N_d): elliptic 1100 is the case section d of tests/test_gpu_gn_rounding.py uses (N_b = 160, its vector
    reference is shared through _gn_reference's cache); every other size has N_b = 40"""
    if system in R.SYSTEMS and Nd in R.NB:
        return R.case(system, Nd)
    if (system, Nd) not in _CASES:
        _CASES[(system, Nd)] = Case(system, Nd)
    return _CASES[(system, Nd)]


# ------------------------------------------------------------------------------------------------ the row sample
def pipe_blocks(nc, w0=512, ob=512):
    """column-block boundaries of the pipelined factorisation for gpk_tune keys 28 (first block) and 29 (the others)"""
    norm = lambda w: min(max((w // PANEL) * PANEL, PANEL), 512)
    b, w = [0], norm(w0)
    while b[-1] < nc:
        b.append(min(b[-1] + w, nc))
        w = norm(ob)
    return b


def boundary_rows(nc, w0=512, ob=512):
    """the rows the schedule makes special: border, first / last row of every block, first row of a ragged tail panel"""
    b = pipe_blocks(nc, w0, ob)
    rows = [nc - 1]
    for b0, b1 in zip(b[:-1], b[1:]):
        rows += [b0, b1 - 1]
        if (b1 - b0) % PANEL:
            rows.append(b0 + ((b1 - b0) // PANEL) * PANEL)
    return list(dict.fromkeys(rows))


def sample_rows(nc, diag_scale, w0=512, ob=512, seed=0, limit=MAX_ROWS):
    """sorted rows of the sample; diag_scale[i] = (|W|^T |W|)_ii.  Raises if the rows the rules demand do not fit."""
    rows = boundary_rows(nc, w0, ob)
    small = np.argsort(np.asarray(diag_scale, dtype=np.float64), kind='stable')[:SMALLEST]
    rows = list(dict.fromkeys(rows + [int(i) for i in small]))
    if len(rows) > limit:
        raise ValueError(f'{len(rows)} mandatory rows for nc = {nc}, blocks ({w0}, {ob}): more than {limit}')
    rng = np.random.RandomState(seed)
    for i in rng.permutation(nc):
        if len(rows) >= min(limit, nc):
            break
        if int(i) not in rows:
            rows.append(int(i))
    return sorted(rows)


# ------------------------------------------------------------------------------------------------ error and scale
_PRODUCT_CACHE = {}


def _digest(W, rows):
    h = hashlib.sha1(np.ascontiguousarray(W).view(np.uint8))
    h.update(np.asarray(rows, dtype=np.int64).tobytes())
    return h.hexdigest()


def product_rows(W, rows):
    """[(W^T W)_i,0..i in long double, (|W|^T |W|)_i,0..i] for the rows; cached on the bits of W (schedule variants share their operand)"""
    key = _digest(W, rows)
    if key not in _PRODUCT_CACHE:
        if len(_PRODUCT_CACHE) >= 4:
            _PRODUCT_CACHE.pop(next(iter(_PRODUCT_CACHE)))
        Wl = np.asarray(W, dtype=np.float64).astype(LD)
        Wa = np.abs(np.asarray(W, dtype=np.float64))
        mag = Wa[:, rows].T @ Wa
        _PRODUCT_CACHE[key] = [(np.einsum('k,kj->j', Wl[:, i], Wl[:, :i + 1]), mag[n, :i + 1]) for n, i in enumerate(rows)]
    return _PRODUCT_CACHE[key]


def factor_rows(Hb, rows):
    """[(R R^T)_i,0..i in long double, (|R| |R^T|)_i,0..i] with R = tril(Hb)"""
    Rf = np.tril(np.asarray(Hb, dtype=np.float64))
    Rl = Rf.astype(LD)
    Ra = np.abs(Rf)
    mag = Ra[rows] @ Ra.T
    return [(np.einsum('k,jk->j', Rl[i, :i + 1], Rl[:i + 1, :i + 1]), mag[n, :i + 1]) for n, i in enumerate(rows)]


def ratio_rows(err, scale):
    """(max err / (eps scale), its index); inf where scale == 0 and err != 0"""
    err = np.asarray(err).astype(np.float64)
    scale = np.asarray(scale, dtype=np.float64)
    if not np.all(np.isfinite(err)):
        return np.inf, int(np.argmax(~np.isfinite(err)))
    bad = (scale == 0) & (err != 0)
    if bad.any():
        return np.inf, int(np.argmax(bad))
    r = err / (EPS * np.where(scale == 0, 1.0, scale))
    return float(np.max(r)), int(np.argmax(r))


def gate_ratio(W, Hb, rows, extra_scale=None):
    """(ratio, (i, j)) of the factored Hb against the operand W over the sampled rows; extra_scale: per row a vector (0..i) added to s"""
    worst, where = 0.0, None
    for n, ((p, pm), (q, qm)) in enumerate(zip(product_rows(W, rows), factor_rows(Hb, rows))):
        s = pm + qm + (0.0 if extra_scale is None else np.asarray(extra_scale[n], dtype=np.float64))
        r, j = ratio_rows(np.abs(q - p), s)
        if not r <= worst:
            worst, where = r, (rows[n], j)
    return worst, where


def host_rendition(W):
    """the float64 rendition of the phase: BLAS W^T W, numpy.linalg.cholesky"""
    W = np.asarray(W, dtype=np.float64)
    return np.linalg.cholesky(W.T @ W)


_NUMPY_CACHE = {}


def numpy_ratio(W, rows, extra_scale=None):
    key = _digest(W, rows) if extra_scale is None else None
    if key in _NUMPY_CACHE:
        return _NUMPY_CACHE[key]
    r = gate_ratio(W, host_rendition(W), rows, extra_scale)[0]
    if key is not None:
        if len(_NUMPY_CACHE) >= 64:
            _NUMPY_CACHE.pop(next(iter(_NUMPY_CACHE)))
        _NUMPY_CACHE[key] = r
    return r


def gate(W, Hb, w0=512, ob=512, extra=None):
    """(device ratio, allowed, numpy ratio, (i, j), rows).  extra(rows) -> the per-row scale vectors a Gram-level mode adds."""
    W = np.asarray(W, dtype=np.float64)
    nc = W.shape[1]
    Wa = np.abs(W)
    rows = sample_rows(nc, np.einsum('ki,ki->i', Wa, Wa), w0, ob)
    es = extra(rows) if extra is not None else None
    npr = numpy_ratio(W, rows, es)
    r, where = gate_ratio(W, Hb, rows, es)
    return r, R.allowed(npr), npr, where, rows


def pred_gate(pred, y):
    """(ratio, allowed) of pred = |y|^2 against the long-double sum over the downloaded border row (terms are squares: the magnitude sum is
    the value; a single number's error can vanish by cancellation, so the numpy figure counts as at least one eps -- as gate_loss)"""
    y = np.asarray(y, dtype=np.float64)
    yl = y.astype(LD)
    ref = yl @ yl
    r = lambda v: float(abs(LD(v) - ref) / (LD(EPS) * ref))
    return r(pred), R.allowed(max(r(float(y @ y)), 1.0))


# ------------------------------------------------------------------------------------------------ what the Gram-level modes add
def gram_scale_rows(G, dcol, rows, border=None):
    """gram_form_kernel writes Hb[c][c'] = d_c G11 d_c' + d_c G12 + G21 d_c' + G22 from the four nz x nz Gram blocks (G: 4 nz x nz, stacked as
    the device stores them): the magnitude sum |d_c||G11||d_c'| + |d_c||G12| + |G21||d_c'| + |G22| per entry of the sampled rows, long double.
    border: the magnitude sum of the entries 0..nz of the border row nz (the caller knows how its mode forms them)."""
    nz = G.shape[1]
    d = np.abs(np.asarray(dcol, dtype=np.float64)).astype(LD)
    out = []
    for i in rows:
        if i == nz:
            out.append(np.asarray(border, dtype=LD))
            continue
        g11, g12, g21, g22 = (np.abs(G[k * nz + i, :i + 1]).astype(LD) for k in range(4))
        out.append(d[i] * g11 * d[:i + 1] + d[i] * g12 + g21 * d[:i + 1] + g22)
    return out


# ------------------------------------------------------------------------------------------------ a numpy model of the phase (host tests)
def tile_cholesky(H, omit=None):
    """left-looking Cholesky by 64 x 64 tiles of the lower triangle of H (float64); omit = (i, j, k): the rank-64 update of tile (i, j) by
    tile column k is left out"""
    from scipy.linalg import solve_triangular
    n = H.shape[0]
    nt = -(-n // PANEL)
    sl = lambda t: slice(t * PANEL, min((t + 1) * PANEL, n))
    Lf = np.zeros_like(H)
    for j in range(nt):
        for i in range(j, nt):
            blk = H[sl(i), sl(j)].copy()
            for k in range(j):
                if (i, j, k) != omit:
                    blk -= Lf[sl(i), sl(k)] @ Lf[sl(j), sl(k)].T
            if i == j:
                Lf[sl(j), sl(j)] = np.linalg.cholesky(np.tril(blk) + np.tril(blk, -1).T)
            else:
                Lf[sl(i), sl(j)] = solve_triangular(Lf[sl(j), sl(j)], blk.T, lower=True, check_finite=False).T
    return Lf


def delta_from_factor(Rb):
    """delta as gpk_i_gn_finish takes it from the factored bordered matrix: R_H^T delta = y (the border row)"""
    from scipy.linalg import solve_triangular
    nz = Rb.shape[0] - 1
    return solve_triangular(Rb[:nz, :nz], Rb[nz, :nz], lower=True, trans='T', check_finite=False)
