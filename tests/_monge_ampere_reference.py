"""Reference of the Hessian Gram layout and of the Monge-Ampere Gauss-Newton system GPK_GN_MONGE_AMPERE (CPU only, numpy; long double
where a bound is "to rounding").  The numpy oracle has no Hessian layout, so this module brings its own, as tests/_semilinear_reference.py.

Layout.  D = d_11 - d_22, M = 2 d_12, L = d_11 + d_22; blocks [D; M; L] on the N_d domain points, delta on the N_d + N_b domain and
boundary points, N = 4 N_d + N_b.  With d = x - y, a_n = g_n(p1, d1), b_n = g_n(p2, d2) of the three-term recurrence of
tests/_gauss_reference.py (g^(n) = g_n g for g = exp(-p d^2 / 2)) the closed forms of include/gpk.h are, times kappa,

    <D,D> = a4 - 2 a2 b2 + b4     <D,M> = 2 (a3 b1 - a1 b3)     <D,L> = a4 - b4     <D,delta> = a2 - b2
    <M,M> = 4 a2 b2               <M,L> = 2 (a3 b1 + a1 b3)     <M,delta> = 2 a1 b1
    <L,L> = a4 + 2 a2 b2 + b4     <L,delta> = a2 + b2           <delta,delta> = 1

(every functional is of even order: no sign, and the table is symmetric).  tests/test_monge_ampere_host.py checks table() against sympy
differentiation of the kernel.

Magnitude sum of an entry: the sum of the absolute values of its terms with every Hermite factor expanded into its monomials in
q = p d and p -- m_1 = |q|, m_2 = q^2 + p, m_3 = |q| (q^2 + 3 p), m_4 = q^4 + 6 p q^2 + 3 p^2 -- times kappa.  That is the scale of the
rounding error of ANY float64 evaluation: the coordinates' difference d is itself rounded (relative eps / 2), which moves h_2 = q^2 - p by
about eps p even where h_2 vanishes.

The Gauss-Newton system (include/gpk.h): unknowns z = [v0 | v1 | v2] = [u | D u | M u],
    F(z) = [v1; v2; s; v0; g],  s = sqrt(v1^2 + v2^2 + 4 f),   A(z): 1 at (t, v1_t), (N_d + t, v2_t), (3 N_d + t, v0_t); v1 / s, v2 / s at
    (2 N_d + t, v1_t / v2_t).
"""
import functools
import zlib

import numpy as np

import _gauss_reference as GR
import _gn_reference as R
import _semilinear_reference as SL
from _gn_reference import poisoned, synthetic_factor  # noqa: F401  (shared with the device tests)

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
KERNELS = GR.KERNELS
NAMES = ('D', 'M', 'L', 'delta')
# functionals as (coefficient, multi-index) lists
FUNC = {'D': ((1, (2, 0)), (-1, (0, 2))), 'M': ((2, (1, 1)),), 'L': ((1, (2, 0)), (1, (0, 2))), 'delta': ((1, (0, 0)),)}
MONOMIALS = {'value': (0, 0), 'd1': (1, 0), 'd2': (0, 1), 'd11': (2, 0), 'd12': (1, 1), 'd22': (0, 2)}   # gpk.device.FUNCTIONAL_OP order


def _mags(p, d):
    """[m_0 .. m_4]: the monomial magnitude sums of the Hermite factors"""
    q = np.abs(p * d)
    q2 = q * q
    return [np.ones_like(q), q, q2 + p, q * (q2 + 3 * p), q2 * q2 + 6 * p * q2 + 3 * p * p]


class Pairs(GR._Pairs):
    """kappa, both chains and their magnitudes for every pair of two broadcastable coordinate sets"""

    def __init__(self, kernel, kp, x1, x2, y1, y2):
        super().__init__(kernel, kp, x1, x2, y1, y2, order=4)
        p1, p2 = GR.precisions(kernel, kp)
        d1 = np.asarray(x1, dtype=np.float64).astype(LD) - np.asarray(y1, dtype=np.float64).astype(LD)
        d2 = np.asarray(x2, dtype=np.float64).astype(LD) - np.asarray(y2, dtype=np.float64).astype(LD)
        d1, d2 = np.broadcast_arrays(d1, d2)
        self.m1, self.m2 = _mags(p1, d1), _mags(p2, d2)
        self.arg = (p1 * d1 * d1 + p2 * d2 * d2) / 2

    def functional_pair(self, fx, fy):
        """(<fx at x, fy at y> kappa, its magnitude sum) for two (coefficient, multi-index) lists, term by term"""
        total, mag = 0, 0
        for cx, a in fx:
            for cy, b in fy:
                total = total + cx * cy * self.partial(a, b)
                mag = mag + abs(cx * cy) * self.m1[a[0] + b[0]] * self.m2[a[1] + b[1]] * self.kappa
        return total, mag


def table(kernel, kp, x1, x2, y1, y2):
    """{(F, G): (value, magnitude sum)} of the 4 x 4 table of a point pair by the closed forms of the module docstring"""
    P = Pairs(kernel, kp, x1, x2, y1, y2)
    a, b, ma, mb, k = P.g1, P.g2, P.m1, P.m2, P.kappa
    t = {
        ('D', 'D'): (a[4] - 2 * a[2] * b[2] + b[4], ma[4] + 2 * ma[2] * mb[2] + mb[4]),
        ('D', 'M'): (2 * (a[3] * b[1] - a[1] * b[3]), 2 * (ma[3] * mb[1] + ma[1] * mb[3])),
        ('D', 'L'): (a[4] - b[4], ma[4] + mb[4]),
        ('D', 'delta'): (a[2] - b[2], ma[2] + mb[2]),
        ('M', 'M'): (4 * a[2] * b[2], 4 * ma[2] * mb[2]),
        ('M', 'L'): (2 * (a[3] * b[1] + a[1] * b[3]), 2 * (ma[3] * mb[1] + ma[1] * mb[3])),
        ('M', 'delta'): (2 * a[1] * b[1], 2 * ma[1] * mb[1]),
        ('L', 'L'): (a[4] + 2 * a[2] * b[2] + b[4], ma[4] + 2 * ma[2] * mb[2] + mb[4]),
        ('L', 'delta'): (a[2] + b[2], ma[2] + mb[2]),
        ('delta', 'delta'): (np.ones_like(k), np.ones_like(k)),
    }
    out = {}
    for (f, g), (v, m) in t.items():
        out[(f, g)] = out[(g, f)] = (v * k, m * k)
    return out, P.arg


def offsets(Nd, Nb):
    return [(0, Nd), (Nd, Nd), (2 * Nd, Nd), (3 * Nd, Nd + Nb)]


def theta(kernel, kp, Xd, Xb):
    """(Theta without nugget, magnitude sums, exponent arguments), each (N, N) long double"""
    Xd = np.asarray(Xd, dtype=np.float64).reshape(-1, 2)
    Xb = np.asarray(Xb, dtype=np.float64).reshape(-1, 2)
    Nd, Nb = Xd.shape[0], Xb.shape[0]
    X = np.concatenate([Xd, Xb])
    t, arg = table(kernel, kp, X[:, None, 0], X[:, None, 1], X[None, :, 0], X[None, :, 1])
    n = [Nd, Nd, Nd, Nd + Nb]
    T = np.block([[t[(f, g)][0][:n[i], :n[j]] for j, g in enumerate(NAMES)] for i, f in enumerate(NAMES)])
    Mg = np.block([[t[(f, g)][1][:n[i], :n[j]] for j, g in enumerate(NAMES)] for i, f in enumerate(NAMES)])
    Ag = np.block([[arg[:n[i], :n[j]] for j in range(4)] for i in range(4)])
    return T, Mg, Ag


def diagonal_values(kernel, kp):
    """<F, F> at d = 0 for D, M, L, delta by the closed forms of include/gpk.h, long double"""
    p1, p2 = GR.precisions(kernel, kp)
    return [3 * p1 * p1 - 2 * p1 * p2 + 3 * p2 * p2, 4 * p1 * p2, 3 * p1 * p1 + 2 * p1 * p2 + 3 * p2 * p2, LD(1)]


def trace_ratios(kernel, kp, Nd, Nb):
    """trace(block k) / trace(block 3), k = 0, 1, 2"""
    c = diagonal_values(kernel, kp)
    return [(Nd * c[k]) / (LD(Nd + Nb)) for k in range(3)]


def block_nuggets(kernel, kp, Nd, Nb, nugget, nugget_type):
    if nugget_type == 'adaptive':
        return [LD(nugget) * r for r in trace_ratios(kernel, kp, Nd, Nb)] + [LD(nugget)]
    return [LD(nugget if nugget_type == 'identity' else 0.0)] * 4


def theta_nugget(kernel, kp, Xd, Xb, nugget, nugget_type='adaptive', base=None):
    Nd, Nb = np.asarray(Xd).reshape(-1, 2).shape[0], np.asarray(Xb).reshape(-1, 2).shape[0]
    T = (theta(kernel, kp, Xd, Xb)[0] if base is None else base).copy()
    for (o, n), v in zip(offsets(Nd, Nb), block_nuggets(kernel, kp, Nd, Nb, nugget, nugget_type)):
        T[np.arange(o, o + n), np.arange(o, o + n)] += v
    return T


def monomial_rows(kernel, kp, name, Xt, Xd, Xb):
    """(rows, magnitude sums, exponent arguments), each (Nt, N) long double: the monomial derivative `name` (MONOMIALS) at the points Xt
    against the column functionals of the layout"""
    Xt = np.asarray(Xt, dtype=np.float64).reshape(-1, 2)
    Xd = np.asarray(Xd, dtype=np.float64).reshape(-1, 2)
    Xb = np.asarray(Xb, dtype=np.float64).reshape(-1, 2)
    X = np.concatenate([Xd, Xb])
    P = Pairs(kernel, kp, Xt[:, None, 0], Xt[:, None, 1], X[None, :, 0], X[None, :, 1])
    fx = ((1, MONOMIALS[name]),)
    Nd = Xd.shape[0]
    n = [Nd, Nd, Nd, X.shape[0]]
    parts = [P.functional_pair(fx, FUNC[g]) for g in NAMES]
    return (np.concatenate([v[:, :k] for (v, _), k in zip(parts, n)], axis=1), np.concatenate([m[:, :k] for (_, m), k in zip(parts, n)], axis=1),
            np.concatenate([P.arg[:, :k] for k in n], axis=1))


# ------------------------------------------------------------------------------------------------ the Gauss-Newton system
def F(f, g, z):
    Nd = f.size
    v0, v1, v2 = z[:Nd], z[Nd:2 * Nd], z[2 * Nd:]
    return np.concatenate([v1, v2, np.sqrt(v1 * v1 + v2 * v2 + 4 * f), v0, g])


def A(f, Nb, z):
    Nd = f.size
    v1, v2 = z[Nd:2 * Nd], z[2 * Nd:]
    s = np.sqrt(v1 * v1 + v2 * v2 + 4 * f)
    out = np.zeros((4 * Nd + Nb, 3 * Nd), dtype=z.dtype)
    i = np.arange(Nd)
    out[i, Nd + i] = 1; out[Nd + i, 2 * Nd + i] = 1; out[3 * Nd + i, i] = 1
    out[2 * Nd + i, Nd + i] = v1 / s; out[2 * Nd + i, 2 * Nd + i] = v2 / s
    return out


class System:
    """F and A as the numpy oracle's gn_method takes them (oracle/gp_oracle.py: EikonalSystem is the model)"""

    def __init__(self, rhs_f, bdy_g):
        self.f, self.g = np.asarray(rhs_f, dtype=np.float64), np.asarray(bdy_g, dtype=np.float64)
        self.Nd, self.Nb = self.f.size, self.g.size
        self.nz = 3 * self.Nd

    def F(self, z):
        return [F(self.f, self.g, z)]

    def A(self, z):
        return [A(self.f, self.Nb, z)]

    def extra(self, z):
        return 0.0, None, None

    def sol_vec(self, z):
        return self.F(z)


gn_float64 = SL.gn_float64
posterior_prepare = SL.posterior_prepare
log_evidence = SL.log_evidence
points = SL.points


def truth(x1, x2):
    return np.exp(0.5 * ((x1 - 0.5) ** 2 + (x2 - 0.5) ** 2))


def rhs(x1, x2):
    r2 = (x1 - 0.5) ** 2 + (x2 - 0.5) ** 2
    return (1.0 + r2) * np.exp(r2)


def gram_float64(kernel, kp, Xd, Xb, nugget):
    """Theta with the adaptive nugget, rounded to float64 from the long-double entries"""
    return theta_nugget(kernel, kp, Xd, Xb, nugget).astype(np.float64)


# ------------------------------------------------------------------------------------------------ one step to rounding (the method of SL)
class Case:
    """inputs of one step on a synthetic, well-conditioned factor (tests/_gn_reference.py): f > 0, so the radicand is positive"""
    system = 'monge_ampere'

    def __init__(self, Nd, Nb):
        self.Nd, self.Nb = Nd, Nb
        self.nz, n = 3 * Nd, 4 * Nd + Nb
        rng = np.random.RandomState(zlib.crc32(repr(('monge_ampere', Nd, Nb)).encode()))
        self.f = rng.uniform(0.5, 1.5, Nd)
        self.g = rng.uniform(0.5, 1.5, Nb)
        self.z0 = rng.uniform(0.3, 1.2, self.nz) * rng.choice([-1.0, 1.0], self.nz)
        self.L = synthetic_factor(rng, n)
        self.groups = [(0, n, self.L)]
        self.rows = n


@functools.lru_cache(maxsize=None)
def case(Nd, Nb):
    return Case(Nd, Nb)


def linearise(cs, z, f=None):
    """[A(z) | F(z)] at the float64 point z with long-double entries (SL.Lin: values and magnitude sums)"""
    Nd = cs.Nd
    z = np.asarray(z, dtype=np.float64).astype(LD)
    f = (cs.f if f is None else np.asarray(f, dtype=np.float64)).astype(LD)
    g, one = cs.g.astype(LD), LD(1)
    v0, v1, v2 = z[:Nd], z[Nd:2 * Nd], z[2 * Nd:]
    s = np.sqrt(v1 * v1 + v2 * v2 + 4 * f)
    lin = SL.Lin(cs.rows, cs.nz)
    lin.put_f(0, v1); lin.put_f(Nd, v2)
    lin.put_f(2 * Nd, s, s)
    lin.put_f(3 * Nd, v0); lin.put_f(4 * Nd, g)
    lin.put_a(0, Nd, one, Nd, True); lin.put_a(Nd, 2 * Nd, one, Nd, True)
    lin.put_a(2 * Nd, Nd, v1 / s, Nd); lin.put_a(2 * Nd, 2 * Nd, v2 / s, Nd)
    lin.put_a(3 * Nd, 0, one, Nd, True)
    return lin.finish()


class FullReference(SL.FullReference):
    """SL.FullReference (one step in long double, rounding scales, the float64 pipeline) on this system's linearisation"""

    def __init__(self, cs, z):
        self.case, self.z = cs, np.array(z, dtype=np.float64)
        lin = self.lin = linearise(cs, z)
        nz = cs.nz
        Sb = R._group_solve(cs, np.concatenate([lin.dense(), lin.F[:, None]], axis=1))
        self.S, self.w = Sb[:, :nz], Sb[:, nz]
        G = R.gram_lower(Sb)
        self.H, self.g, self.loss = LD(2) * G[:nz, :nz], LD(2) * G[nz, :nz], self.w @ self.w
        Sa = np.abs(Sb).astype(np.float64)
        self.scaleH = 2.0 * (Sa[:, :nz].T @ Sa[:, :nz])
        self.scaleg = 2.0 * (Sa[:, :nz].T @ Sa[:, nz])
        self.p64 = R.Pipeline64(cs, z, lin)
        self.delta = R.refine(self.p64.solve, lambda d: self.g - self.H @ d, self.g.astype(np.float64))
        ev = np.linalg.eigvalsh(self.H.astype(np.float64))
        self.normH, self.cond = float(ev[-1]), float(ev[-1] / ev[0])


@functools.lru_cache(maxsize=None)
def full_reference(Nd, Nb):
    cs = case(Nd, Nb)
    return FullReference(cs, cs.z0)


gates = SL.gates


class VectorReference(R.VectorReference):
    """_gn_reference.VectorReference (the step without L^-1 A, O(N^2)) on this module's linearise; gated by gate_loss,
    gate_backward_vec and gate_forward of _gn_reference"""

    def __init__(self, cs, z, want_delta=True):
        super().__init__(cs, z, want_delta, lin_fn=linearise)


@functools.lru_cache(maxsize=None)
def vector_reference(Nd, Nb):
    cs = case(Nd, Nb)
    return VectorReference(cs, cs.z0)


# ------------------------------------------------------------------------------------------------ the Gram gate
GRAM_BOUND = 4e-15            # the project's Gram-block bound (tests/_gauss_reference.py BOUND), here per entry, in units of its magnitude sum


def gram_allowed(mag, arg):
    """Per entry: GRAM_BOUND x magnitude sum for the polynomial factor, plus the error of kappa = exp(-arg): the float64 evaluation
    rounds d1, d2 (eps / 2 each, doubled by the square), the two products and the sum -- at most 4 eps relative on arg, i.e. 4 eps arg
    relative on kappa."""
    return (LD(GRAM_BOUND) + 4 * LD(EPS) * arg) * mag
