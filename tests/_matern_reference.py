"""Independent reference of the Matern kernels (nu = 5/2, 7/2, 9/2) and of the Gram matrices built on them (CPU only).

Not the expansion the library and src/kernels.py use (phi^(k) with reverse Bessel polynomials of shifted index): here the scalar
kappa(x1, x2, y1, y2) itself is differentiated symbolically (sympy) in x and in y, one expression per (alpha, beta), and evaluated in
long double.

  r > 0 and t = sqrt(2 nu) |u| >= T_SERIES   the derivative of the closed form theta_m(0) kappa = exp(-t) theta_m(t), written with integer
                                             coefficients only (a non-dyadic rational would reach the evaluation as a float64)
  0 < t < T_SERIES                           the Taylor series of kappa in t to order J_SERIES, differentiated term by term and summed
                                             numerically: the closed form's fourth derivatives
                                             cancel like t^-3 there, the terms of the series do not cancel at all
  coincident points                          the derivative of the terms c0 + c2 t^2 + c4 t^4 of that series: a polynomial in x - y (c1 =
                                             c3 = 0, and t^j, j >= 5, vanishes to order > 4)
Both branches are checked against mpmath.diff at 40 digits in tests/test_matern_host.py.

Error of the reference itself: long double (eps 1.1e-19); the closed form is used where t^-3 <= 8, the series is truncated where its
terms are below J^6 T^(J-4) / J! = 3e-22: a few 1e-18 relative to (a / rho)^n, the size of an entry of order n.

Also here: the layouts (functional of each block, which point set it lives on), and Theta, Theta_test, extension rows and the adaptive
trace ratios assembled from these entries; and the cases of tests/test_gpu_matern_shapes.py that its host preconditions
(tests/test_matern_host.py) share: the (nu, rho) of the large sizes, the row subset compared there, the planted near-coincident and far
points, and the per-test-point gate of the extension.
"""
import functools

import numpy as np
import sympy as sp

LD = np.longdouble
ORDER = {'Matern52': 2, 'Matern72': 3, 'Matern92': 4, 2.5: 2, 3.5: 3, 4.5: 4}
T_SERIES = 0.5
J_SERIES = 24

# functionals as lists of multi-indices; layouts as (functional, lives on boundary points too) per block
ID, D1, D2, DD2, LAP = ((0, 0),), ((1, 0),), ((0, 1),), ((0, 2),), ((2, 0), (0, 2))
FUNCTIONALS = {'value': ID, 'd1': D1, 'd2': D2, 'd2d2': DD2, 'laplacian': LAP}          # in the bit order of gpk.device.FUNCTIONAL
LAYOUTS = {
    'Nonlinear_elliptic': ((LAP, False), (ID, True)),
    'Burgers': ((D1, False), (D2, False), (DD2, False), (ID, True)),
    'Eikonal': ((D1, False), (D2, False), (LAP, False), (ID, True)),
    'Darcy_u': ((D1, False), (D2, False), (LAP, False), (ID, True)),
    'Darcy_a': ((D1, False), (D2, False), (ID, False)),
}

_THETA = {2: (3, 3, 1), 3: (15, 15, 6, 1), 4: (105, 105, 45, 10, 1)}
_x1, _x2, _y1, _y2, _r1, _r2, _A = sp.symbols('x1 x2 y1 y2 r1 r2 A', real=True)
_W = ((_x1 - _y1) * _r1) ** 2 + ((_x2 - _y2) * _r2) ** 2            # |u|^2, r_i = 1 / rho_i (a symbol: its value arrives in long double)


def series_coefficients(m):
    """Taylor coefficients c_0 .. c_J of exp(-t) theta_m(t) / theta_m(0) in t, exact rationals"""
    t = sp.Symbol('t')
    poly = sum(sp.Integer(c) * t ** j for j, c in enumerate(_THETA[m])) / _THETA[m][0]
    out = []
    for j in range(J_SERIES + 1):                                     # coefficient of t^j in poly * sum (-t)^i / i!
        out.append(sum(poly.coeff(t, k) * sp.Rational((-1) ** (j - k), sp.factorial(j - k)) for k in range(min(j, m) + 1)))
    return out


def _ld(q):
    return LD(int(q.p)) / LD(int(q.q))


def _diff(e, a1, a2, b1, b2):
    for v, n in ((_x1, a1), (_x2, a2), (_y1, b1), (_y2, b2)):
        if n:
            e = sp.diff(e, v, n)
    return e


@functools.lru_cache(maxsize=None)
def _closed(m, a1, a2, b1, b2):
    """d_x^(a1,a2) d_y^(b1,b2) of theta_m(0) kappa = exp(-t) theta_m(t) as a numpy function of (x1, x2, y1, y2, r1, r2, A)"""
    t = _A * sp.sqrt(_W)
    e = sp.exp(-t) * sum(sp.Integer(c) * t ** j for j, c in enumerate(_THETA[m]))
    return sp.lambdify((_x1, _x2, _y1, _y2, _r1, _r2, _A), _diff(e, a1, a2, b1, b2), modules='numpy')


_TERMS = [j for j in range(J_SERIES + 1) if j not in (1, 3)]          # c1 = c3 = 0 for nu >= 5/2 (asserted where they are used)


@functools.lru_cache(maxsize=None)
def _series(a1, a2, b1, b2):
    """the same derivative of every term t^j = A^j W^(j/2), j in _TERMS, of the Taylor series, each differentiated on its own (integer and
    half-integer powers of W with exact coefficients: an even power is a polynomial, whose high derivatives vanish symbolically):
    (x1, x2, y1, y2, r1, r2, A) -> list"""
    terms = [_diff(_A ** j * _W ** sp.Rational(j, 2), a1, a2, b1, b2) for j in _TERMS]
    return sp.lambdify((_x1, _x2, _y1, _y2, _r1, _r2, _A), terms, modules='numpy')


@functools.lru_cache(maxsize=None)
def _origin(a1, a2, b1, b2):
    """the same derivative of c0 + c2 t^2 + c4 t^4, the terms of the series that have a derivative of order <= 4 other than 0 at
    coincident points (c1 = c3 = 0 for nu >= 5/2; t^j, j >= 5, vanishes there to order > 4): (x1, x2, y1, y2, r1, r2, A, c0, c2, c4)"""
    c0, c2, c4 = sp.symbols('c0 c2 c4', real=True)
    e = c0 + c2 * _A ** 2 * _W + c4 * _A ** 4 * _W ** 2
    return sp.lambdify((_x1, _x2, _y1, _y2, _r1, _r2, _A, c0, c2, c4), _diff(e, a1, a2, b1, b2), modules='numpy')


def partial(kernel, alpha, beta, x1, x2, y1, y2, rho):
    """d_x^alpha d_y^beta kappa in long double (arrays broadcast); rho: a scalar or (rho_1, rho_2)"""
    m = ORDER[kernel]
    rho = np.atleast_1d(np.asarray(rho, dtype=LD))
    r1, r2 = LD(1) / rho[0], LD(1) / rho[-1]
    A = np.sqrt(LD(2 * m + 1))
    x1, x2, y1, y2 = np.broadcast_arrays(*(np.asarray(v, dtype=LD) for v in (x1, x2, y1, y2)))
    shape = x1.shape
    x1, x2, y1, y2 = (v.ravel() for v in (x1, x2, y1, y2))
    w = ((x1 - y1) * r1) ** 2 + ((x2 - y2) * r2) ** 2
    far, zero = A * np.sqrt(w) >= T_SERIES, w == 0
    near = ~far & ~zero
    key = (alpha[0], alpha[1], beta[0], beta[1])
    c = series_coefficients_cached(m)
    out = np.zeros(x1.shape, dtype=LD)
    if far.any():
        out[far] = _closed(m, *key)(x1[far], x2[far], y1[far], y2[far], r1, r2, A) / LD(_THETA[m][0])
    if near.any():
        terms = _series(*key)(x1[near], x2[near], y1[near], y2[near], r1, r2, A)
        acc = np.zeros(int(near.sum()), dtype=LD)
        for jt, term in zip(_TERMS, terms):
            acc = acc + c[jt] * term
        out[near] = acc
    if zero.any():
        assert c[1] == 0 and c[3] == 0
        out[zero] = _origin(*key)(x1[zero], x2[zero], y1[zero], y2[zero], r1, r2, A, c[0], c[2], c[4])
    return out.reshape(shape)


@functools.lru_cache(maxsize=None)
def series_coefficients_cached(m):
    return tuple(_ld(q) for q in series_coefficients(m))


def pair(kernel, fx, fy, x1, x2, y1, y2, rho):
    """<functional fx in x, functional fy in y> of kappa, long double"""
    total = 0
    for a in fx:
        for b in fy:
            total = total + partial(kernel, a, b, x1, x2, y1, y2, rho)
    return total


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


def rows(kernel, rho, layout, fx, Xt, Xd, Xb):
    """(Nt, N) long double: functional fx at the points Xt against the column functionals of the layout (fx = ID: Theta_test)"""
    Xt = np.asarray(Xt, dtype=np.float64).reshape(-1, 2)
    return np.concatenate([pair(kernel, fx, f, Xt[:, None, 0], Xt[:, None, 1], P[None, :, 0], P[None, :, 1], rho)
                           for f, P in _points(layout, Xd, Xb)], axis=1)


def theta_test(kernel, rho, layout, Xt, Xd, Xb):
    return rows(kernel, rho, layout, ID, Xt, Xd, Xb)


def theta(kernel, rho, layout, Xd, Xb):
    """Theta without nugget, (N, N) long double"""
    return np.concatenate([rows(kernel, rho, layout, f, P, Xd, Xb) for f, P in _points(layout, Xd, Xb)], axis=0)


def diagonal_values(kernel, rho, layout):
    """<f_b, f_b> at coincident points for each block b, long double (from the Taylor series)"""
    z = np.zeros(1)
    return [pair(kernel, f, f, z, z, z, z, rho)[0] for f, _ in LAYOUTS[layout]]


def trace_ratios(kernel, rho, layout, Nd, Nb):
    """trace(block b) / trace(last block), b < nb - 1, long double"""
    c = diagonal_values(kernel, rho, layout)
    n = [s for _, s in offsets(layout, Nd, Nb)]
    return [(n[b] * c[b]) / (n[-1] * c[-1]) for b in range(len(c) - 1)]


def block_nuggets(kernel, rho, layout, Nd, Nb, nugget, nugget_type):
    """the value added to the diagonal of each block"""
    nb = len(LAYOUTS[layout])
    if nugget_type == 'adaptive':
        return [LD(nugget) * r for r in trace_ratios(kernel, rho, layout, Nd, Nb)] + [LD(nugget)]
    return [LD(nugget if nugget_type == 'identity' else 0.0)] * nb


# ------------------------------------------------------------------- cases of tests/test_gpu_matern_shapes.py and of its host preconditions
KERNELS = ('Matern52', 'Matern72', 'Matern92')
RHOS = (0.3, (0.3, 0.07))
LARGE = ((530, 46), (265, 41))                     # M = 576, blocks even (two-point kernel, grid2.x = 2; Darcy_a: 530); M = 306, blocks odd (one-point kernel, grid.x = 2)
EPS = float(np.finfo(np.float64).eps)
TILE = 32                                          # rows of Theta per workgroup (TP of csrc/gpk_assemble_ref.h)
SUBSET_ROWS = 30                                   # rows of every block that the large cases compare: 4 edge + 2 tile boundary + 24 random


def large_case(layout, size):
    """(kernel, rho) of the size-th large size for this layout: index (layout + size) mod 3 into KERNELS and mod 2 into RHOS, so
    layout + size = 0 .. 5 meets the six (nu, rho) once each, every nu meets both sizes (both kernel shapes), every layout both sizes"""
    k = list(LAYOUTS).index(layout) + size
    return KERNELS[k % 3], RHOS[k % 2]


def row_subset(layout, Nd, Nb):
    """per block the SUBSET_ROWS rows (indices into Theta, ascending) whose reference the large cases build: the first and the last two
    rows of the block, both sides of the 32-row tile boundary (of the point index, which is what a workgroup's blockIdx.y counts)
    nearest the block's middle, and 24 random others"""
    out = []
    for b, (o, n) in enumerate(offsets(layout, Nd, Nb)):
        edge = TILE * max(1, int(round(n / 2 / TILE)))
        fixed = [0, 1, n - 2, n - 1, edge - 1, edge]
        assert len(set(fixed)) == 6 and 0 < edge < n - 2, (layout, Nd, Nb, b)
        rest = np.setdiff1d(np.arange(n), fixed)
        rng = np.random.RandomState(1000 * Nd + 10 * Nb + b)
        pick = rng.choice(rest, SUBSET_ROWS - len(fixed), replace=False)
        out.append(o + np.sort(np.concatenate([fixed, pick])))
    return out


def subset_coverage(layout, Nd, Nb, subset):
    """the smallest number of rows of a row block in which a column of Theta is compared, over all columns and row blocks: a row of the
    subset compares all its columns; the exact symmetry of Theta carries the result to the transposed entries, which adds nothing to
    this count (it is the count of direct comparisons)"""
    worst = None
    for (o, n), rows in zip(offsets(layout, Nd, Nb), subset):
        rows = np.unique(rows)
        assert np.all((rows >= o) & (rows < o + n))
        worst = rows.size if worst is None else min(worst, rows.size)
    return worst


def subset_rows_reference(kernel, rho, layout, Xd, Xb, subset, evaluate=None):
    """the rows `subset` of Theta stacked block after block, (sum of the subset sizes, N): long double through rows(), or through
    evaluate(fx, Xt) -> (Nt, N) (the float64 numpy class)"""
    evaluate = evaluate or (lambda fx, P: rows(kernel, rho, layout, fx, P, Xd, Xb))
    return np.concatenate([evaluate(f, P[idx - o]) for (f, P), (o, _), idx in zip(_points(layout, Xd, Xb), offsets(layout, len(Xd), len(Xb)), subset)],
                          axis=0)


# offsets of the planted near-coincident points: (target, source, offset) in the domain set, the boundary set (source in the domain set)
# and the test set (source named)
PLANT_D = ((1, 0, (1e-12, 0.0)), (3, 2, (6e-9, -8e-9)), (5, 4, (0.0, 1e-5)), (7, 6, (1e-3, 1e-3)), (9, 8, (0.0, 0.0)))
PLANT_B = ((0, 10, (0.0, 0.0)), (1, 11, (3e-7, 0.0)))
PLANT_T = ((1, 'd', 12, (1e-12, 0.0)), (2, 'd', 13, (0.0, -1e-6)), (3, 'b', 2, (1e-9, 1e-9)))


def planted_points(Xd, Xb, Xt):
    """copies of the points with coincident and nearly coincident ones planted (separations 0, 1e-12, 1e-8, 1e-5, 1.4e-3 in the domain
    set; a boundary point on a domain point and one 3e-7 from one; test points 1e-12, 1e-6 and 1.4e-9 from collocation points)"""
    Xd, Xb, Xt = (np.array(X, dtype=np.float64, copy=True) for X in (Xd, Xb, Xt))
    for k, s, d in PLANT_D:
        Xd[k] = Xd[s] + np.asarray(d)
    for k, s, d in PLANT_B:
        Xb[k] = Xd[s] + np.asarray(d)
    for k, which, s, d in PLANT_T:
        Xt[k] = (Xd if which == 'd' else Xb)[s] + np.asarray(d)
    Xt[0] = Xd[3]                                                       # (the verbatim test point of the cases follows its domain point)
    return Xd, Xb, Xt


FAR_RHO2 = 0.002                                   # a / rho_2 > 745: pairs a unit apart in the second coordinate are beyond the underflow of exp
FAR_BAND = (708.0, 745.0)                          # exp(-t) is subnormal in float64 for t in the band, 0 beyond


def far_points(kernel, Xd, Xb, Xt):
    """copies of the points with second coordinates set so that t = a |u| of rho = (0.3, FAR_RHO2) is 720 and 735 (in the band: the
    first coordinate adds less than 0.05 to either) for the domain pairs (0, 1), (0, 2) and a test point against Xd[0], and beyond
    the band (t > 1100) for the domain pair (0, 4) and a test point against Xd[0]"""
    a = float(np.sqrt(2.0 * ORDER[kernel] + 1.0))
    Xd, Xb, Xt = (np.array(X, dtype=np.float64, copy=True) for X in (Xd, Xb, Xt))
    Xd[0, 1], Xd[1, 1], Xd[2, 1], Xd[4, 1] = 0.01, 0.01 + 720.0 * FAR_RHO2 / a, 0.01 + 735.0 * FAR_RHO2 / a, 0.999
    Xt[1], Xt[2] = (Xd[0, 0], Xd[1, 1]), (Xd[0, 0], 0.999)
    return Xd, Xb, Xt


def scaled_distance(kernel, rho, X, Y):
    """t = a |u| for every pair of the two point sets, long double"""
    rho = np.atleast_1d(np.asarray(rho, dtype=LD))
    a = np.sqrt(LD(2 * ORDER[kernel] + 1))
    X, Y = np.asarray(X, dtype=LD), np.asarray(Y, dtype=LD)
    return a * np.sqrt(((X[:, None, 0] - Y[None, :, 0]) / rho[0]) ** 2 + ((X[:, None, 1] - Y[None, :, 1]) / rho[-1]) ** 2)


def extension_ratios(got, rows_ld, coeff):
    """per test point |got - rows @ coeff| / (eps |rows| @ |coeff|), with the product accumulated in long double"""
    c = np.asarray(coeff, dtype=np.float64).astype(LD)
    err = np.abs(np.asarray(got).astype(LD) - rows_ld @ c)
    terms = np.abs(rows_ld) @ np.abs(c)
    assert np.all(terms > 0)
    return (err / (LD(EPS) * terms)).astype(np.float64), terms


class ExtensionGate:
    """Per test point: |got - ref| <= C eps (|rows| @ |coeff|)_t with C = 32 r_np + 1, r_np the worst such ratio of np_value (the float64
    numpy class's rows @ coeff) over the test points -- the rule `allowed` of tests/_gn_reference.py.  The bound may at no test point
    exceed 1e-12 max_t (|rows| @ |coeff|), the bound of tests/test_gpu_matern.py.  The figures (device: the worst device ratio) are there
    to be printed before check() asserts both."""

    def __init__(self, got, np_value, rows_ld, coeff):
        self.ratios, self.terms = extension_ratios(got, rows_ld, coeff)
        self.device = float(np.max(self.ratios))
        self.r_np = float(np.max(extension_ratios(np_value, rows_ld, coeff)[0]))
        self.allowed = 32.0 * self.r_np + 1.0

    def check(self, what=''):
        assert np.all(LD(self.allowed) * LD(EPS) * self.terms <= LD(1e-12) * np.max(self.terms)), \
            (what, 'the per-point bound is looser than the norm bound', self.r_np)
        assert np.all(self.ratios <= self.allowed), (what, int(np.argmax(self.ratios)), self.device, self.r_np, self.allowed)


def theta_nugget(kernel, rho, layout, Xd, Xb, nugget, nugget_type='adaptive', base=None):
    """Theta with the nugget of *.Gram_matrix; base: a Theta without nugget to start from (left unchanged)"""
    Nd, Nb = np.asarray(Xd).reshape(-1, 2).shape[0], np.asarray(Xb).reshape(-1, 2).shape[0]
    T = (theta(kernel, rho, layout, Xd, Xb) if base is None else base).copy()
    for (o, n), v in zip(offsets(layout, Nd, Nb), block_nuggets(kernel, rho, layout, Nd, Nb, nugget, nugget_type)):
        T[np.arange(o, o + n), np.arange(o, o + n)] += v
    return T
