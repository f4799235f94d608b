"""Independent reference of the Gaussian and the anisotropic Gaussian kernel and of the Gram matrices built on them (CPU only).

Not the expansion the library and oracle/gp_oracle.py use (the 1-D Hermite factors written out as polynomials in p and d): here the
derivatives of g(d) = exp(-p d^2 / 2) come from the three-term recurrence

    g_0 = 1,  g_1 = -p d,  g_{k+1} = -p d g_k - k p g_{k-1}            (g^(k) = g_k g: differentiate g' = -p d g  k times, Leibniz)

in numpy long double, and with kappa = exp(-(p1 d1^2 + p2 d2^2) / 2), d = x - y,

    d_x^a d_y^b kappa = (-1)^|b| g_{a1+b1}(p1, d1) g_{a2+b2}(p2, d2) kappa      (d/dx = d/dd, d/dy = -d/dd).

The differences are formed in long double from the float64 coordinates (exact), the precisions in long double from the float64 kernel
parameters.  tests/test_gauss_reference_host.py checks partial() against mpmath.diff at 40 digits and theta / theta_test against the
reference project's own outputs (tests/golden/theta_small.npz).

Error of the reference itself: long double (eps 1.1e-19) and about ten roundings per entry: a few 1e-18 relative to
p1^((a1+b1)/2) p2^((a2+b2)/2), the size of such an entry.

The surface is that of tests/_matern_reference.py (the kernel parameter where that one has rho): the layouts (functional of each block,
which point set it lives on), Theta, Theta_test, extension rows, the adaptive trace ratios and the nugget.  Also here: the per-block gate
of the Gram tests (gate_blocks), and the point sets and oracle calls that the host test and the device test of this reference share.
"""
import numpy as np

LD = np.longdouble
KERNELS = ('Gaussian', 'anisotropic_Gaussian')

# functionals as lists of multi-indices; layouts as (functional, lives on boundary points too) per block -- the tables of
# tests/_matern_reference.py, repeated: importing that module compiles its sympy expressions
ID, D1, D2, DD2, LAP = ((0, 0),), ((1, 0),), ((0, 1),), ((0, 2),), ((2, 0), (0, 2))
FUNCTIONALS = {'value': ID, 'd1': D1, 'd2': D2, 'd2d2': DD2, 'laplacian': LAP}          # in the bit order of gpk.device.FUNCTIONAL
LAYOUTS = {
    'Nonlinear_elliptic': ((LAP, False), (ID, True)),
    'Burgers': ((D1, False), (D2, False), (DD2, False), (ID, True)),
    'Eikonal': ((D1, False), (D2, False), (LAP, False), (ID, True)),
    'Darcy_u': ((D1, False), (D2, False), (LAP, False), (ID, True)),
    'Darcy_a': ((D1, False), (D2, False), (ID, False)),
}


def precisions(kernel, kp):
    """(p1, p2) in long double: 1 / sigma^2 on both axes (Gaussian), 2 / sigma_k^2 (anisotropic_Gaussian: the reference's exponent has
    no factor 1/2) -- the convention of csrc/gpk_assemble_common.h::precisions"""
    s = np.atleast_1d(np.asarray(kp, dtype=np.float64)).astype(LD)
    if kernel == 'Gaussian':
        return LD(1) / (s[0] * s[0]), LD(1) / (s[0] * s[0])
    if kernel == 'anisotropic_Gaussian':
        return LD(2) / (s[0] * s[0]), LD(2) / (s[1] * s[1])
    raise ValueError(f'unknown kernel {kernel!r}')


def _chain(p, d, n):
    """[g_0 .. g_n] of the recurrence, long double"""
    g = [np.ones_like(d), -p * d]
    for k in range(1, n):
        g.append(-p * d * g[k] - k * p * g[k - 1])
    return g[:n + 1]


class _Pairs:
    """kappa and both chains for every pair (x, y) of two broadcastable coordinate sets: what every entry of these pairs is made of"""

    def __init__(self, kernel, kp, x1, x2, y1, y2, order=4):
        p1, p2 = precisions(kernel, kp)
        d1 = np.asarray(x1, dtype=np.float64).astype(LD) - np.asarray(y1, dtype=np.float64).astype(LD)
        d2 = np.asarray(x2, dtype=np.float64).astype(LD) - np.asarray(y2, dtype=np.float64).astype(LD)
        d1, d2 = np.broadcast_arrays(d1, d2)
        self.g1, self.g2 = _chain(p1, d1, order), _chain(p2, d2, order)
        self.kappa = np.exp(-(p1 * d1 * d1 + p2 * d2 * d2) / 2)

    def partial(self, alpha, beta):
        v = self.g1[alpha[0] + beta[0]] * self.g2[alpha[1] + beta[1]] * self.kappa
        return -v if (beta[0] + beta[1]) & 1 else v

    def pair(self, fx, fy):
        total = 0
        for a in fx:
            for b in fy:
                total = total + self.partial(a, b)
        return total


def partial(kernel, kp, alpha, beta, x1, x2, y1, y2):
    """d_x^alpha d_y^beta kappa in long double (arrays broadcast)"""
    return _Pairs(kernel, kp, x1, x2, y1, y2, max(alpha[0] + beta[0], alpha[1] + beta[1], 1)).partial(alpha, beta)


def pair(kernel, kp, fx, fy, x1, x2, y1, y2):
    """<functional fx in x, functional fy in y> of kappa, long double"""
    return _Pairs(kernel, kp, x1, x2, y1, y2).pair(fx, fy)


def _points(layout, Xd, Xb):
    Xd = np.asarray(Xd, dtype=np.float64).reshape(-1, 2)
    Xb = np.asarray(Xb, dtype=np.float64).reshape(-1, 2)
    Xall = np.concatenate([Xd, Xb])
    return [(f, Xall if on_b else Xd) for f, on_b in LAYOUTS[layout]]


def offsets(layout, Nd, Nb):
    """[(offset, size)] of the blocks"""
    out, o = [], 0
    for _, on_b in LAYOUTS[layout]:
        n = Nd + Nb if on_b else Nd
        out.append((o, n)); o += n
    return out


def _rows(kernel, kp, layout, row_functionals, Xt, Xd, Xb):
    """one (Nt, N) block row per functional of row_functionals at the points Xt, from ONE evaluation of the point pairs (the blocks of a
    layout live on Xd or on [Xd; Xb]: slices of the same pairs)"""
    Xt = np.asarray(Xt, dtype=np.float64).reshape(-1, 2)
    cols = _points(layout, Xd, Xb)
    Xall = np.concatenate([np.asarray(Xd, dtype=np.float64).reshape(-1, 2), np.asarray(Xb, dtype=np.float64).reshape(-1, 2)])
    P = _Pairs(kernel, kp, Xt[:, None, 0], Xt[:, None, 1], Xall[None, :, 0], Xall[None, :, 1])
    return [np.concatenate([P.pair(fx, f)[:, :Y.shape[0]] for f, Y in cols], axis=1) for fx in row_functionals]


def rows(kernel, kp, layout, fx, Xt, Xd, Xb):
    """(Nt, N) long double: functional fx at the points Xt against the column functionals of the layout (fx = ID: Theta_test)"""
    return _rows(kernel, kp, layout, (fx,), Xt, Xd, Xb)[0]


def theta_test(kernel, kp, layout, Xt, Xd, Xb):
    return rows(kernel, kp, layout, ID, Xt, Xd, Xb)


def theta(kernel, kp, layout, Xd, Xb):
    """Theta without nugget, (N, N) long double"""
    cols = _points(layout, Xd, Xb)
    Xall = np.concatenate([np.asarray(Xd, dtype=np.float64).reshape(-1, 2), np.asarray(Xb, dtype=np.float64).reshape(-1, 2)])
    full = _rows(kernel, kp, layout, [f for f, _ in cols], Xall, Xd, Xb)      # (Xd is the head of [Xd; Xb]: a block's rows are a slice)
    return np.concatenate([r[:Y.shape[0]] for r, (_, Y) in zip(full, cols)], axis=0)


def diagonal_values(kernel, kp, layout):
    """<f_b, f_b> at coincident points for each block b, long double"""
    z = np.zeros(1)
    return [pair(kernel, kp, f, f, z, z, z, z)[0] for f, _ in LAYOUTS[layout]]


def trace_ratios(kernel, kp, layout, Nd, Nb):
    """trace(block b) / trace(last block), b < nb - 1, long double"""
    c = diagonal_values(kernel, kp, layout)
    n = [s for _, s in offsets(layout, Nd, Nb)]
    return [(n[b] * c[b]) / (n[-1] * c[-1]) for b in range(len(c) - 1)]


def block_nuggets(kernel, kp, layout, Nd, Nb, nugget, nugget_type):
    """the value added to the diagonal of each block"""
    nb = len(LAYOUTS[layout])
    if nugget_type == 'adaptive':
        return [LD(nugget) * r for r in trace_ratios(kernel, kp, layout, Nd, Nb)] + [LD(nugget)]
    return [LD(nugget if nugget_type == 'identity' else 0.0)] * nb


def theta_nugget(kernel, kp, layout, Xd, Xb, nugget, nugget_type='adaptive', base=None):
    """Theta with the nugget of *.Gram_matrix; base: a Theta without nugget to start from (left unchanged)"""
    Nd, Nb = np.asarray(Xd).reshape(-1, 2).shape[0], np.asarray(Xb).reshape(-1, 2).shape[0]
    T = (theta(kernel, kp, layout, Xd, Xb) if base is None else base).copy()
    for (o, n), v in zip(offsets(layout, Nd, Nb), block_nuggets(kernel, kp, layout, Nd, Nb, nugget, nugget_type)):
        T[np.arange(o, o + n), np.arange(o, o + n)] += v
    return T


# ---------------------------------------------------------------------------------------------------------------- the gate
BOUND = 4e-15                                                         # the project's Gram-block bound (tests/test_gpu_parity.py)


def gate_blocks(got, ref, npv, row_blocks, col_blocks, what=''):
    """Per block (row_blocks x col_blocks, each [(offset, size)]): |got - ref| <= (4e-15 + 4 e_np) max|block of ref|, where e_np is the
    error of npv (a float64 evaluation of the same entries by other code, or None: e_np = 0) against ref in the same block, scaled the
    same way; the factor 4 allows for contraction and for the device's exp against glibc's.  Returns the worst (e_got, e_np) in units of
    max|block|: the block whose e_got comes closest to what it is allowed.  A block that is 0 throughout has to be reproduced as 0."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    worst = (0.0, 0.0)
    for ro, rn in row_blocks:
        for co, cn in col_blocks:
            if rn == 0 or cn == 0:
                continue
            r = ref[ro:ro + rn, co:co + cn].astype(LD)
            scale = float(np.max(np.abs(r)))
            d_got = float(np.max(np.abs(got[ro:ro + rn, co:co + cn].astype(LD) - r)))
            d_np = 0.0 if npv is None else float(np.max(np.abs(np.asarray(npv)[ro:ro + rn, co:co + cn].astype(LD) - r)))
            if scale == 0.0:
                assert d_got == 0.0, (what, (ro, co), d_got)
                continue
            e_got, e_np = d_got / scale, d_np / scale
            if e_got / (BOUND + 4 * e_np) >= worst[0] / (BOUND + 4 * worst[1]):
                worst = (e_got, e_np)
            assert e_got <= BOUND + 4 * e_np, (what, (ro, co), e_got, e_np)
    return worst


# ------------------------------------------------------------------------------------------- cases of the host and the device test
SIZES = ((64, 36), (65, 41))                       # all counts even: the two-point kernel, M = 100 = 3 * 32 + 4; odd: the one-point kernel
LARGE = ((530, 46), (265, 41))                     # M = 576 > 2 * 256 (Darcy_a: 530 > 512) even, M = 306 > 256 odd: more than one workgroup in x
NTS = (1, 2, 67, 300, 514, 515)                    # tail of the 32 test rows; one and two workgroups along t in the cross kernel; even and odd
PARAMS = {'Gaussian': 0.2, 'anisotropic_Gaussian': (0.3, 0.05)}
ORACLE_EQN = {'Darcy_u': 'Darcy_flow2d', 'Darcy_a': 'Darcy_flow2d'}


def case_points(Nd, Nb):
    """(Xd, Xb, Xt): uniform on the unit square; three test points are collocation points verbatim (the first: Nt = 1 has one)"""
    rng = np.random.RandomState(100 * Nd + Nb)
    Xd, Xb = rng.uniform(0, 1, (Nd, 2)), rng.uniform(0, 1, (Nb, 2))
    Xt = rng.uniform(0, 1, (max(NTS), 2))
    Xt[0], Xt[5], Xt[66] = Xd[3 % Nd], (Xb[2] if Nb > 2 else Xd[0]), Xd[Nd - 1]
    return Xd, Xb, Xt


def large_kernel(layout, k):
    """the kernel of the k-th large size for this layout: one kernel per layout and size, alternating so that both occur"""
    return KERNELS[(list(LAYOUTS).index(layout) + k) % 2]


def oracle_theta(layout, kernel, kp, Xd, Xb):
    """oracle/gp_oracle.py's float64 Theta of the layout (Darcy: the matrix of u or of a)"""
    from oracle import gp_oracle as O
    T = O.gram_matrix_assembly(Xd, Xb, ORACLE_EQN.get(layout, layout), kernel, kp)
    return T[layout == 'Darcy_a'] if isinstance(T, tuple) else T


def oracle_theta_test(layout, kernel, kp, Xt, Xd, Xb):
    from oracle import gp_oracle as O
    T = O.construct_theta_test(Xt, Xd, Xb, ORACLE_EQN.get(layout, layout), kernel, kp)
    return T[layout == 'Darcy_a'] if isinstance(T, tuple) else T
