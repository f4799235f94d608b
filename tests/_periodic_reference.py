"""Long-double reference of the periodic kernel and of the Gram matrices, test rows and priors built on it (CPU only).

Written from the formulas of the kernel ("Periodic kernel"), not from the device code.  Per axis k, with precision
p_k = 2 / sigma_k^2, period L_k > 0 and w_k = 2 pi / L_k,
    kappa_k(d) = exp(-(2 p_k / w_k^2) sin^2(w_k d / 2)),
and with s = (p / w) sin w d, c = p cos w d the factors h_m = (-1)^m kappa^(m) / kappa are
    h0 = 1, h1 = s, h2 = s^2 - c, h3 = s (s^2 - 3 c - w^2), h4 = s^4 - 6 s^2 c + 3 c^2 - 4 w^2 s^2 + w^2 c;
an axis with L_k = 0 has the Gaussian factor exp(-p d^2 / 2) and the Hermite factors.  Then
    d_x^alpha d_y^beta kappa = (-1)^{|alpha|} h_{a1+b1}(axis 1) h_{a2+b2}(axis 2) kappa.
Everything is evaluated in long double from the exact difference of the float64 coordinates; the argument of the sine is reduced as
d / L mod 2 in long double before sin(pi .), so images x + k L are handled to long-double accuracy.

Error of the reference itself: long double (eps 1.1e-19) through a dozen operations per factor: a few 1e-19 relative to p^(n/2), the
size of an entry of order n -- three orders below what the gates built on it resolve.

Also here: Theta, Theta_test, the prior and the adaptive trace ratios assembled from these entries (the nugget as in
tests/_matern_reference.py, whose layouts, block offsets, row subset and extension gate are used as they are), the cases of
tests/test_gpu_periodic.py and tests/test_gpu_periodic_shapes.py, and the block gate both share with tests/test_periodic_host.py.
"""
import numpy as np

import _matern_reference as MR

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
PI = LD(4) * np.arctan(LD(1))
ID, D1, D2, DD2, LAP = MR.ID, MR.D1, MR.D2, MR.DD2, MR.LAP
FUNCTIONALS = MR.FUNCTIONALS
LAYOUTS = MR.LAYOUTS
offsets = MR.offsets
row_subset = MR.row_subset
subset_coverage = MR.subset_coverage
ExtensionGate = MR.ExtensionGate


def axes(param):
    """[(p, L)] in long double of param = (sigma_1, sigma_2, L_1, L_2)"""
    v = [LD(float(t)) for t in param]
    assert len(v) == 4
    return [(LD(2) / (v[k] * v[k]), v[2 + k]) for k in range(2)]


def table(p, L, d):
    """((h0 .. h4), exponent) of one axis at d (long double arrays): kappa_axis = exp(-exponent)"""
    one = np.ones_like(d)
    if L > 0:
        w = LD(2) * PI / L
        r = np.fmod(d / L, LD(2))
        sh, ch = np.sin(PI * r), np.cos(PI * r)
        s = (p / w) * (LD(2) * sh * ch)
        c = p * (LD(1) - LD(2) * sh * sh)
        w2 = w * w
        h = (one, s, s * s - c, s * (s * s - LD(3) * c - w2), s ** 4 - LD(6) * s * s * c + LD(3) * c * c - LD(4) * w2 * s * s + w2 * c)
        return h, (LD(2) * p / w2) * sh * sh
    q = p * d
    h = (one, q, q * q - p, q ** 3 - LD(3) * p * q, q ** 4 - LD(6) * p * q * q + LD(3) * p * p)
    return h, p * d * d / LD(2)


def partial(param, alpha, beta, x1, x2, y1, y2):
    """d_x^alpha d_y^beta kappa in long double (arrays broadcast)"""
    x1, x2, y1, y2 = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64).astype(LD) for v in (x1, x2, y1, y2)))
    (p1, L1), (p2, L2) = axes(param)
    a, ea = table(p1, L1, x1 - y1)
    b, eb = table(p2, L2, x2 - y2)
    v = a[alpha[0] + beta[0]] * b[alpha[1] + beta[1]] * np.exp(-(ea + eb))
    return -v if (alpha[0] + alpha[1]) & 1 else v


def pair(param, fx, fy, x1, x2, y1, y2):
    """<functional fx in x, functional fy in y> of kappa, long double"""
    total = 0
    for a in fx:
        for b in fy:
            total = total + partial(param, a, b, x1, x2, y1, y2)
    return total


def rows(param, layout, fx, Xt, Xd, Xb):
    """(Nt, N) long double: functional fx at the points Xt against the column functionals of the layout (fx = ID: Theta_test)"""
    Xt = np.asarray(Xt, dtype=np.float64).reshape(-1, 2)
    return np.concatenate([pair(param, fx, f, Xt[:, None, 0], Xt[:, None, 1], P[None, :, 0], P[None, :, 1])
                           for f, P in MR._points(layout, Xd, Xb)], axis=1)


def theta_test(param, layout, Xt, Xd, Xb):
    return rows(param, layout, ID, Xt, Xd, Xb)


def theta(param, layout, Xd, Xb):
    """Theta without nugget, (N, N) long double"""
    return np.concatenate([rows(param, layout, f, P, Xd, Xb) for f, P in MR._points(layout, Xd, Xb)], axis=0)


def prior(param, Xa, Xb):
    """k(xa_i, xb_j), (na, nb) long double"""
    Xa, Xb = (np.asarray(X, dtype=np.float64).reshape(-1, 2) for X in (Xa, Xb))
    return pair(param, ID, ID, Xa[:, None, 0], Xa[:, None, 1], Xb[None, :, 0], Xb[None, :, 1])


def diagonal_values(param, layout):
    """<f_b, f_b> at coincident points for each block b, long double"""
    z = np.zeros(1)
    return [pair(param, f, f, z, z, z, z)[0] for f, _ in LAYOUTS[layout]]


def trace_ratios(param, layout, Nd, Nb):
    """trace(block b) / trace(last block), b < nb - 1, long double"""
    c = diagonal_values(param, layout)
    n = [s for _, s in offsets(layout, Nd, Nb)]
    return [(n[b] * c[b]) / (n[-1] * c[-1]) for b in range(len(c) - 1)]


def block_nuggets(param, layout, Nd, Nb, nugget, nugget_type):
    """the value added to the diagonal of each block"""
    nb = len(LAYOUTS[layout])
    if nugget_type == 'adaptive':
        return [LD(nugget) * r for r in trace_ratios(param, layout, Nd, Nb)] + [LD(nugget)]
    return [LD(nugget if nugget_type == 'identity' else 0.0)] * nb


def theta_nugget(param, layout, Xd, Xb, nugget, nugget_type='adaptive', base=None):
    """Theta with the nugget of *.Gram_matrix; base: a Theta without nugget to start from (left unchanged)"""
    Nd, Nb = np.asarray(Xd).reshape(-1, 2).shape[0], np.asarray(Xb).reshape(-1, 2).shape[0]
    T = (theta(param, layout, Xd, Xb) if base is None else base).copy()
    for (o, n), v in zip(offsets(layout, Nd, Nb), block_nuggets(param, layout, Nd, Nb, nugget, nugget_type)):
        T[np.arange(o, o + n), np.arange(o, o + n)] += v
    return T


def subset_rows_reference(param, layout, Xd, Xb, subset, evaluate=None):
    """the rows `subset` of Theta stacked block after block: long double through rows(), or through evaluate(fx, Xt) -> (Nt, N)"""
    evaluate = evaluate or (lambda fx, P: rows(param, layout, fx, P, Xd, Xb))
    return np.concatenate([evaluate(f, P[idx - o]) for (f, P), (o, _), idx in
                           zip(MR._points(layout, Xd, Xb), offsets(layout, len(Xd), len(Xb)), subset)], axis=0)


def np_rows(param, layout, fx, Xt, Xd, Xb):
    """the float64 class of src/kernels.py on the entries of rows()"""
    from src.kernels import Periodic_kernel
    k = Periodic_kernel()
    Xt = np.asarray(Xt, dtype=np.float64).reshape(-1, 2)
    return np.concatenate([k._eval(list(fx), list(f), Xt[:, None, 0], Xt[:, None, 1], P[None, :, 0], P[None, :, 1], param)
                           for f, P in MR._points(layout, Xd, Xb)], axis=1)


# ------------------------------------------------------------------------------------------------------------------- the cases
SIGMA = (0.2, 0.15)
PERIODS = ((0.0, 1.0), (1.0, 0.0), (1.0, 0.75))
PARAMS = tuple(SIGMA + P for P in PERIODS)
# (8, 4); (190, 37): odd, the 8-byte kernel; (300, 40): even, the 16-byte kernel, M = 340 > 256 (blockIdx.x > 0 in the one-point frame
# under gpk_tune(47, 0)); (480, 40): M / 2 = 260 > 256, two workgroups along x in the two-point frame
SIZES = ((8, 4), (190, 37), (300, 40), (480, 40))
NTS = (2, 514, 515)
GRID = 2.0 ** -30                                  # planted sources lie on this grid, so that x + L and x + 3 L are exact
# (target, source, multiple of L, offset) along every periodic axis, in the domain set: d = 0; 1e-9 .. 1e-3; L / 2 (sin(w d / 2) = 1);
# L - 1e-3; the images x + L and x + 3 L
PLANT = ((1, 0, 0.0, 0.0), (3, 2, 0.0, 1e-9), (5, 4, 0.0, 1e-6), (7, 6, 0.0, 1e-3), (9, 8, 0.5, 0.0), (11, 10, 1.0, -1e-3),
         (13, 12, 1.0, 0.0), (15, 12, 3.0, 0.0))
IMAGE_ROWS = (12, 13, 15)                          # a point and its images


def points(Nd, Nb, param, nt=max(NTS)):
    """(Xd, Xb, Xt): uniform on [0, L_1) x [0, L_2) (1 for an axis that is not periodic) with the pairs of PLANT along every periodic
    axis (those whose target exists), a boundary point on a domain point's image, and test points on collocation points and on images"""
    rng = np.random.RandomState(100 * Nd + Nb)
    L = np.array([param[2] or 1.0, param[3] or 1.0])
    Xd, Xb, Xt = rng.uniform(0, 1, (Nd, 2)) * L, rng.uniform(0, 1, (Nb, 2)) * L, rng.uniform(0, 1, (nt, 2)) * L
    per = np.array([1.0 if param[2] > 0 else 0.0, 1.0 if param[3] > 0 else 0.0])
    for tgt, src, mult, off in PLANT:
        if tgt < Nd:
            Xd[src] = np.round(Xd[src] / GRID) * GRID
            Xd[tgt] = Xd[src] + per * (mult * L + off)
    Xb[0] = Xd[2] + per * L
    Xt[0] = Xd[3]
    if nt > 1:
        Xt[1] = Xd[0] - per * 2.0 * L
    return Xd, Xb, Xt


# kappa underflows along a periodic axis when 2 p / w^2 = p L^2 / (2 pi^2) > 745: sigma = L / 90 gives 820 at d = L / 2 (kappa = 0 in
# float64) and 820 sin^2(pi d / L) = 726 at d = 0.3899 L (subnormal)
FAR_SIGMA = 1.0 / 90.0
FAR_D = (0.3899, 0.5)


def far_case(axis):
    """(param, Xd, Xb, Xt) with L = 1 and sigma = L / 90 on `axis`, and domain pairs (0, 1), (0, 2) at the distances FAR_D along it"""
    sig, per = [0.2, 0.2], [0.0, 0.0]
    sig[axis], per[axis] = FAR_SIGMA, 1.0
    param = tuple(sig + per)
    Xd, Xb, Xt = points(16, 4, param, nt=4)
    e = np.eye(2)[axis]
    Xd[1] = Xd[0] + FAR_D[0] * e
    Xd[2] = Xd[0] + FAR_D[1] * e
    Xt[2] = Xd[0] + FAR_D[0] * e
    Xt[3] = Xd[0] - FAR_D[1] * e
    return param, Xd, Xb, Xt


def natural_scales(param, layout, row_values=False):
    """sqrt(<f_i, f_i>(0) <f_j, f_j>(0)) per block pair, the Cauchy-Schwarz bound of an entry; row_values: one row block of values"""
    c = [float(v) for v in diagonal_values(param, layout)]
    return [[np.sqrt(ci * cj) for cj in c] for ci in ([1.0] if row_values else c)]


# ------------------------------------------------------------------------------------------------------------------- the block gate
NP_PRECONDITION = 8e-15                            # the float64 class against long double, in units of max|block| (tests/test_matern_host.py)


def block_gate(what, got, ref, npv, row_blocks, col_blocks, figures=None, scales=None):
    """Per block: max|got - ref| <= C eps max|block| with C = 32 r_np + 1, r_np the error of the float64 class of src/kernels.py (npv) on
    the same entries in eps of max|block|; the numpy figure itself must stay below NP_PRECONDITION.  Returns the worst (device error in
    eps of max|block|, C); figures: a list that receives (row block, column block, device, r_np) per block.  scales[bi][bj]: a scale to
    use in place of max|block| (the underflow cases, where a block can hold next to nothing: natural_scales)."""
    worst = (0.0, 1.0)
    for bi, (ro, rn) in enumerate(row_blocks):
        for bj, (co, cn) in enumerate(col_blocks):
            r = ref[ro:ro + rn, co:co + cn]
            scale = float(np.max(np.abs(r))) if scales is None else float(scales[bi][bj])
            assert scale > 0
            dev = float(np.max(np.abs(np.asarray(got[ro:ro + rn, co:co + cn]).astype(LD) - r))) / scale / EPS
            r_np = float(np.max(np.abs(np.asarray(npv[ro:ro + rn, co:co + cn]).astype(LD) - r))) / scale / EPS
            C = 32.0 * r_np + 1.0
            if figures is not None:
                figures.append((bi, bj, dev, r_np))
            assert r_np * EPS < NP_PRECONDITION, (what, 'precondition: the numpy class', (bi, bj), r_np)
            assert dev <= C, (what, (bi, bj), dev, r_np, C)
            if dev / C >= worst[0] / worst[1]:
                worst = (dev, C)
    return worst
