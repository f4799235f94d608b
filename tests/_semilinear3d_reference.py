"""Reference of the 3-D gradient layout and of the system GPK_GN_SEMILINEAR3D (CPU only, numpy).

  Layout (include/gpk.h, gpk_assemble_grad3d): blocks 0, 1, 2 = d_1, d_2, d_3 on the Nd domain points, block 3 = psi_i (op3, MI3 order) on
  the domain points, block 4 = delta on the domain points then phi_b (bc3) on the boundary points; N = 5 Nd + Nb.
    theta, nugget_diag, trace_ratios, extend_rows     from the Hermite formulas of tests/test_operator3d_host.py (Pairs.blk: weighted
                                                      multi-index lists, value and magnitude per entry), float64 or long double
  System: -psi[u] + N(u, g) = f,  N = u (a1 g1 + a2 g2 + a3 g3) + b1 g1^2 + b2 g2^2 + b3 g3^2 + c1 u + c3 u^3,  gq8 = (a1, a2, a3, b1, b2, b3, c1, c3)
    unknowns z = [v0 | v1 | v2 | v3],   F(z) = [v1; v2; v3; N(v0, v1, v2, v3) - f; v0; g],   A(z) = dF/dz
    N, dN, linearise, FullReference, System, gn_float64     as tests/_semilinear_reference.py does for the planar system, whose Lin,
                                                            check_build (C_BUILD) and gates (MARGIN) apply unchanged
    PlanarCase, linearise_planar, slab_factor               the same step computed WITHOUT the third axis: with a3 = b3 = 0 and a factor in
                                                            which the d_3 block is decoupled (points in a plane x3 = const) the unknowns
                                                            v3 leave the problem (their step is v3 itself) and the rest is a system on
                                                            the rows [d_1 u; d_2 u; psi[u]; u]
"""
import functools
import zlib

import numpy as np

import _gn_reference as R
import _semilinear_reference as SL
import test_elliptic3d_host as H3
import test_operator3d_host as H
from _gn_reference import poisoned, synthetic_factor  # noqa: F401  (shared with the device tests)

LD, EPS = R.LD, R.EPS
C_BUILD, MARGIN = SL.C_BUILD, SL.MARGIN
# Rounding count of sl3_N / sl3_dN (csrc/gpk_common.h, uncontracted) in the convention of _semilinear_reference.C_BUILD: the longest chain of
# F = N - f is a1 g1, + a2 g2, + a3 g3, u *, + grad, + reac, - f: 7 roundings of 1/2 eps = 3.5 <= C_BUILD; N_u: 4 roundings = 2; N_gk: 2 = 1.
GQ8 = (0.7, -0.4, 0.6, 0.3, -0.2, 0.5, 0.5, 0.2)         # every entry of A live
NB = {37: 11, 150: 28, 300: 28}
KERNELS = H.KERNELS
C_ENTRY3, C_EXTEND3 = H.C_ENTRY3, H.C_EXTEND3
NAMES = H.NAMES


# ------------------------------------------------------------------------------------------------ the Gram matrix of the layout
def functionals(Nd, Nb, op3, bc3):
    """the five row / column functionals as weighted multi-index lists over [Xd; Xb], and the points each lives on"""
    dom, every = slice(0, Nd), slice(None)
    one = np.ones(Nd)
    return [([(one, H.MI3[1])], dom), ([(one, H.MI3[2])], dom), ([(one, H.MI3[3])], dom), (H.psi(H.all_op(Nd, op3)), dom),
            (H.phi(H.all_coeffs(Nd, bc3, Nb)), every)]


def theta(Xd, Xb, op3, bc3, p, dtype=np.float64):
    """(Theta without nugget, mag per entry)"""
    Xd = np.asarray(Xd, dtype=np.float64).reshape(-1, 3); Xb = np.asarray(Xb, dtype=np.float64).reshape(-1, 3)
    Nd, Nb = len(Xd), len(Xb)
    Xa = np.concatenate([Xd, Xb], axis=0)
    P = H.Pairs(Xa, Xa, p, dtype)
    fs = functionals(Nd, Nb, op3, bc3)
    parts = [[P.blk(fi, fj, ri, rj) for fj, rj in fs] for fi, ri in fs]
    return (np.block([[q[0] for q in row] for row in parts]), np.block([[q[1] for q in row] for row in parts]))


def trace_ratios(p, Nd, Nb, op3, bc3, dtype=LD):
    """trace(block k) / trace(block 4), k = 0..3, with the values at d = 0: <d_k, d_k> = p_k, <psi, psi> and <phi, phi> of the operator layout"""
    q = [dtype(v) for v in p]
    r3 = H.trace_ratio(p, Nd, Nb, op3, bc3, dtype)                      # sum <psi, psi> / (Nd + sum <phi, phi>)
    c = H.all_coeffs(Nd, bc3, Nb)[Nd:].astype(dtype)
    s1 = dtype(0)
    for b in range(Nb):
        s1 += c[b, 0] * c[b, 0] + q[0] * c[b, 1] * c[b, 1] + q[1] * c[b, 2] * c[b, 2] + q[2] * c[b, 3] * c[b, 3]
    den = dtype(Nd) + s1
    return [dtype(Nd) * q[0] / den, dtype(Nd) * q[1] / den, dtype(Nd) * q[2] / den, r3]


def nugget_diag(p, Nd, Nb, op3, bc3, nugget, nugget_type):
    r = [float(v) for v in trace_ratios(p, Nd, Nb, op3, bc3, LD)]
    n = [{'none': 0.0, 'identity': nugget, 'adaptive': nugget * rk}[nugget_type] for rk in r]
    n4 = 0.0 if nugget_type == 'none' else nugget
    return np.concatenate([np.full(Nd, n[0]), np.full(Nd, n[1]), np.full(Nd, n[2]), np.full(Nd, n[3]), np.full(Nd + Nb, n4)])


@functools.lru_cache(maxsize=None)
def gram_case(kernel, kp, Nd, Nb, oset, bset):
    """points, coefficients, precisions and the long-double expectation of one case of the device tests (the points and coefficient sets
    of tests/test_operator3d_host.py)"""
    Xd, Xb = H.points(Nd, Nb)
    op3 = None if oset is None else H.op_set(oset, Xd, np.random.RandomState(11 * Nd + Nb))
    bc3 = H.bc_set(bset, Xb, np.random.RandomState(7 * Nd + Nb))
    p = H3.precisions(kernel, kp)
    T, mag = theta(Xd, Xb, op3, bc3, p, dtype=LD)
    return Xd, Xb, op3, bc3, p, T, mag


def extend_rows(names, Xt, Xd, Xb, op3, bc3, cvec, p, dtype=np.float64):
    """({name: K_F @ cvec}, {name: mag @ |cvec|}) for the row monomials `names` at Xt, cvec over the 5 Nd + Nb columns"""
    Xd = np.asarray(Xd, dtype=np.float64).reshape(-1, 3); Xb = np.asarray(Xb, dtype=np.float64).reshape(-1, 3)
    Nd, Nb = len(Xd), len(Xb)
    Xa = np.concatenate([Xd, Xb], axis=0)
    cvec = np.asarray(cvec, dtype=dtype)
    P = H.Pairs(Xt, Xa, p, dtype)
    fs = functionals(Nd, Nb, op3, bc3)
    out, terms = {}, {}
    for n in names:
        blocks = [P.blk(H.monomial(n, len(Xt)), fj, slice(None), rj) for fj, rj in fs]
        out[n] = np.concatenate([b[0] for b in blocks], axis=1) @ cvec
        terms[n] = np.concatenate([b[1] for b in blocks], axis=1) @ np.abs(cvec)
    return out, terms


# ------------------------------------------------------------------------------------------------ the nonlinearity
def N(gq, u, g1, g2, g3):
    a1, a2, a3, b1, b2, b3, c1, c3 = gq
    return u * (a1 * g1 + a2 * g2 + a3 * g3) + b1 * g1 * g1 + b2 * g2 * g2 + b3 * g3 * g3 + c1 * u + c3 * u * u * u


def dN(gq, u, g1, g2, g3):
    a1, a2, a3, b1, b2, b3, c1, c3 = gq
    return a1 * g1 + a2 * g2 + a3 * g3 + c1 + 3 * c3 * u * u, a1 * u + 2 * b1 * g1, a2 * u + 2 * b2 * g2, a3 * u + 2 * b3 * g3


def N_mag(gq, u, g1, g2, g3):
    return N(tuple(abs(v) for v in gq), np.abs(u), np.abs(g1), np.abs(g2), np.abs(g3))


def dN_mag(gq, u, g1, g2, g3):
    return dN(tuple(abs(v) for v in gq), np.abs(u), np.abs(g1), np.abs(g2), np.abs(g3))


# ------------------------------------------------------------------------------------------------ F(z), A(z), one step
class Case:
    """inputs of one N_d: coefficients, right-hand sides, factor, start point; seeded per (N_d, N_b).  groups, nz, rows: what
    _gn_reference's Pipeline64 and solvers read"""
    system = 'semilinear3d'

    def __init__(self, Nd, Nb, gq=GQ8, L=None, seed=None):
        self.Nd, self.Nb, self.gq = Nd, Nb, tuple(float(v) for v in gq)
        self.nz, n = 4 * Nd, 5 * Nd + Nb
        rng = np.random.RandomState(zlib.crc32(repr(('semilinear3d', Nd, Nb, seed)).encode()))
        self.f = rng.uniform(0.5, 1.5, Nd)
        self.g = rng.uniform(0.5, 1.5, Nb)
        self.z0 = rng.uniform(0.3, 1.2, self.nz) * rng.choice([-1.0, 1.0], self.nz)
        self.L = synthetic_factor(rng, n) if L is None else L
        self.groups = [(0, n, self.L)]
        self.rows = n


@functools.lru_cache(maxsize=None)
def case(Nd):
    return Case(Nd, NB[Nd])


def split(z, Nd):
    return z[:Nd], z[Nd:2 * Nd], z[2 * Nd:3 * Nd], z[3 * Nd:]


def linearise(cs, z):
    """[A(z) | F(z)] at the float64 point z with long-double entries"""
    Nd = cs.Nd
    z = np.asarray(z, dtype=np.float64).astype(LD)
    f, g = cs.f.astype(LD), cs.g.astype(LD)
    gq, one = tuple(LD(v) for v in cs.gq), LD(1)
    v = split(z, Nd)
    lin = SL.Lin(cs.rows, cs.nz)
    lin.put_f(0, v[1]); lin.put_f(Nd, v[2]); lin.put_f(2 * Nd, v[3])
    lin.put_f(3 * Nd, N(gq, *v) - f, N_mag(gq, *v) + np.abs(f))
    lin.put_f(4 * Nd, v[0]); lin.put_f(5 * Nd, g)
    d, m = dN(gq, *v), dN_mag(gq, *v)
    for k in range(3):
        lin.put_a(k * Nd, (k + 1) * Nd, one, Nd, True)
    for k in range(4):
        lin.put_a(3 * Nd, k * Nd, d[k], Nd, mag=m[k])
    lin.put_a(4 * Nd, 0, one, Nd, True)
    return lin.finish()


class FullReference:
    """one step at z in long double (S, w, H, g, loss, delta) with the rounding scales and the float64 pipeline p64 on the same inputs:
    _semilinear_reference.FullReference on this module's linearise"""

    def __init__(self, cs, z, lin_fn=None):
        self.case, self.z = cs, np.array(z, dtype=np.float64)
        lin = self.lin = (lin_fn or linearise)(cs, z)
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
def full_reference(Nd):
    cs = case(Nd)
    return FullReference(cs, cs.z0)


gates = SL.gates
check_build = SL.check_build
err = SL.err


def stair_col(Nd):
    """storage column of unknown j in the leading-zero layout of gpk_gn_step: groups in the order v1, v2, v3, v0, reversed"""
    j = np.arange(4 * Nd)
    pos = ((j // Nd + 3) % 4) * Nd + j % Nd
    return 4 * Nd - 1 - pos


# ------------------------------------------------------------------------------------------------ the planar computation
class PlanarCase:
    """the system without its third axis: unknowns [v0 | v1 | v2], rows [d_1 u; d_2 u; psi[u]; u; g] with the factor L_pl"""
    system = 'semilinear3d-planar'

    def __init__(self, cs, L_pl):
        Nd = cs.Nd
        self.Nd, self.Nb, self.gq, self.f, self.g = Nd, cs.Nb, cs.gq, cs.f, cs.g
        self.nz, n = 3 * Nd, 4 * Nd + cs.Nb
        self.z0 = cs.z0[:3 * Nd]
        self.L = L_pl
        self.groups = [(0, n, L_pl)]
        self.rows = n


def linearise_planar(cs, z):
    Nd = cs.Nd
    z = np.asarray(z, dtype=np.float64).astype(LD)
    f, g = cs.f.astype(LD), cs.g.astype(LD)
    gq, one, zero = tuple(LD(v) for v in cs.gq), LD(1), np.zeros(Nd, dtype=LD)
    v = (z[:Nd], z[Nd:2 * Nd], z[2 * Nd:], zero)
    lin = SL.Lin(cs.rows, cs.nz)
    lin.put_f(0, v[1]); lin.put_f(Nd, v[2])
    lin.put_f(2 * Nd, N(gq, *v) - f, N_mag(gq, *v) + np.abs(f))
    lin.put_f(3 * Nd, v[0]); lin.put_f(4 * Nd, g)
    d, m = dN(gq, *v), dN_mag(gq, *v)
    lin.put_a(0, Nd, one, Nd, True); lin.put_a(Nd, 2 * Nd, one, Nd, True)
    for k in range(3):
        lin.put_a(2 * Nd, k * Nd, d[k], Nd, mag=m[k])
    lin.put_a(3 * Nd, 0, one, Nd, True)
    return lin.finish()


def slab_factor(Nd, Nb, eps=0.3, kernel='Gaussian', kp=0.3, nugget=1e-4, x3=0.4):
    """(L, keep): the float64 Cholesky factor of Theta + nugget on points of the plane x3 = const with psi = eps Laplace, and the indices of
    the rows that are not d_3 rows.  At d_3 = 0 every entry between a d_3 functional and one of even order along axis 3 vanishes exactly
    (h_1(0) = h_3(0) = 0), so the d_3 block of Theta is decoupled, the factor has exact zeros there, and its sub-matrix on `keep` is the
    factor of the planar problem."""
    rng = np.random.RandomState(5 * Nd + Nb)
    Xd = np.concatenate([rng.uniform(0, 1, (Nd, 2)), np.full((Nd, 1), x3)], axis=1)
    Xb = H.face_points(rng, Nb, faces=4)
    Xb[:, 2] = x3
    p = H3.precisions(kernel, kp)
    op3 = np.tile(eps * np.asarray(H.LAPLACE), (Nd, 1))
    T = theta(Xd, Xb, op3, None, p, dtype=LD)[0].astype(np.float64)
    T = T + np.diag(nugget_diag(p, Nd, Nb, op3, None, nugget, 'adaptive'))
    L = np.linalg.cholesky(T)
    keep = np.concatenate([np.arange(0, 2 * Nd), np.arange(3 * Nd, 5 * Nd + Nb)])
    return L, keep


# ------------------------------------------------------------------------------------------------ float64 Gauss-Newton on a Gram factor
class System:
    """F and A of the system as the numpy oracle's gn_method takes them"""

    def __init__(self, gq, rhs_f, bdy_g):
        self.gq = tuple(float(v) for v in gq)
        self.f, self.g = np.asarray(rhs_f, dtype=np.float64), np.asarray(bdy_g, dtype=np.float64)
        self.Nd, self.Nb = self.f.size, self.g.size
        self.nz = 4 * self.Nd

    def F(self, z):
        v = split(z, self.Nd)
        return [np.concatenate([v[1], v[2], v[3], N(self.gq, *v) - self.f, v[0], self.g])]

    def A(self, z):
        Nd = self.Nd
        d = dN(self.gq, *split(z, Nd))
        A = np.zeros((5 * Nd + self.Nb, 4 * Nd))
        i = np.arange(Nd)
        for k in range(3):
            A[k * Nd + i, (k + 1) * Nd + i] = 1.0
        for k in range(4):
            A[3 * Nd + i, k * Nd + i] = d[k]
        A[4 * Nd + i, i] = 1.0
        return [A]

    def extra(self, z):
        return 0.0, None, None

    def sol_vec(self, z):
        return self.F(z)


def gn_float64(sysm, L, z0, steps):
    """(z, loss history) of `steps` plain Gauss-Newton steps in float64 (the oracle's gn_method with this system)"""
    from oracle import gp_oracle as O
    return O.gn_method(sysm, [L], z0, steps, 1)


def numpy_pipeline(Xd, Xb, op3, bc3, p, nugget, gq, f, g, z0, steps):
    """(z, loss history, L, system): Theta (long double, rounded) + adaptive nugget, LAPACK Cholesky, float64 Gauss-Newton"""
    Nd, Nb = len(Xd), len(Xb)
    T = theta(Xd, Xb, op3, bc3, p, dtype=LD)[0].astype(np.float64) + np.diag(nugget_diag(p, Nd, Nb, op3, bc3, nugget, 'adaptive'))
    L = np.linalg.cholesky(T)
    sysm = System(gq, f, g)
    z, hist = gn_float64(sysm, L, np.array(z0, dtype=np.float64), steps)
    return z, hist, L, sysm


log_evidence = SL.log_evidence
posterior_prepare = SL.posterior_prepare


# ------------------------------------------------------------------------------------------------ manufactured problems
def truth3(x1, x2, x3):
    return np.sin(np.pi * x1) * np.sin(np.pi * x2) * np.sin(np.pi * x3)


def steady_problem(eps, gq):
    """(u*, f) with f = -eps Laplace(u*) + N(u*, grad u*), u* = prod_k sin(pi x_k)"""
    def f(x1, x2, x3):
        return 3 * np.pi ** 2 * eps * truth3(x1, x2, x3) + N(gq, truth3(x1, x2, x3), *H.truth_grad(x1, x2, x3))
    return truth3, f


def parabolic_problem(nu, gq):
    """(u*, f) of the driver's --operator parabolic: f = u*_t - nu Laplace_x u* + N(u*, grad_x u*, .) (a3 = b3 = 0)"""
    import main_Semilinear3d as drv
    from src.nonlinearity import GradientNonlinearity3d
    return drv.parabolic_manufactured(nu, GradientNonlinearity3d.make(gq))
