"""Gaussian and anisotropic-Gaussian kernels with the method names of the reference's src/kernels.py, and the Matern family
(nu = 5/2, 7/2, 9/2; not in the reference) with the same method names.

The reference obtains every derivative by nested jax.grad of the scalar kappa (src/kernels.py:15-89, 102-178).  Here each
method is the closed form  d_x^alpha d_y^beta kappa = (-1)^{|alpha|} h_{a1+b1}(p1, x1-y1) h_{a2+b2}(p2, x2-y2) kappa
with the Hermite factors h0..h4 of exp(-p d^2/2); the same formula is what the HIP Gram evaluator
(csrc/gpk_assemble.hip) computes per point pair.  Methods accept scalars or numpy arrays.
"""
import numpy as np


def _hermite(p, d):
    q = p * d
    q2 = q * q
    return (1.0, q, q2 - p, q * (q2 - 3.0 * p), q2 * (q2 - 6.0 * p) + 3.0 * p * p)


# functionals as lists of derivative multi-indices (order in x1/y1, order in x2/y2)
_ID, _D1, _D2, _DD2, _LAP = [(0, 0)], [(1, 0)], [(0, 1)], [(0, 2)], [(2, 0), (0, 2)]

# method name -> (functional applied in x, functional applied in y)
_METHODS = {
    'kappa': (_ID, _ID),
    'D_x1_kappa': (_D1, _ID), 'D_x2_kappa': (_D2, _ID), 'DD_x2_kappa': (_DD2, _ID),
    'D_y1_kappa': (_ID, _D1), 'D_y2_kappa': (_ID, _D2), 'DD_y2_kappa': (_ID, _DD2),
    'D_x1_D_y1_kappa': (_D1, _D1), 'D_x1_D_y2_kappa': (_D1, _D2), 'D_x1_DD_y2_kappa': (_D1, _DD2),
    'D_x2_D_y2_kappa': (_D2, _D2), 'D_x2_D_y1_kappa': (_D2, _D1), 'D_x2_DD_y2_kappa': (_D2, _DD2),
    'DD_x2_DD_y2_kappa': (_DD2, _DD2),
    'Delta_x_kappa': (_LAP, _ID), 'Delta_y_kappa': (_ID, _LAP), 'Delta_x_Delta_y_kappa': (_LAP, _LAP),
    'Delta_x_D_y1_kappa': (_LAP, _D1), 'Delta_x_D_y2_kappa': (_LAP, _D2),
}


class _ClosedFormKernel(object):
    def __init__(self):
        pass

    def _precisions(self, sigma):
        raise NotImplementedError

    def _eval(self, fx, fy, x1, x2, y1, y2, sigma):
        p1, p2 = self._precisions(sigma)
        d1 = np.asarray(x1, dtype=np.float64) - np.asarray(y1, dtype=np.float64)
        d2 = np.asarray(x2, dtype=np.float64) - np.asarray(y2, dtype=np.float64)
        a, b = _hermite(p1, d1), _hermite(p2, d2)
        total = 0.0
        for (a1, a2) in fx:
            for (b1, b2) in fy:
                term = a[a1 + b1] * b[a2 + b2]
                total = total - term if (a1 + a2) & 1 else total + term
        return total * np.exp(-0.5 * (p1 * d1 * d1 + p2 * d2 * d2))


def _make(name):
    fx, fy = _METHODS[name]

    def method(self, x1, x2, y1, y2, sigma):
        return self._eval(fx, fy, x1, x2, y1, y2, sigma)
    method.__name__ = name
    return method


for _n in _METHODS:
    setattr(_ClosedFormKernel, _n, _make(_n))


class Gaussian_kernel(_ClosedFormKernel):
    """kappa = exp(-((x1-y1)^2 + (x2-y2)^2) / (2 sigma^2))   (reference src/kernels.py:8-89)"""

    def _precisions(self, sigma):
        p = 1.0 / (float(sigma) ** 2)
        return p, p


class Anisotropic_Gaussian_kernel(_ClosedFormKernel):
    """kappa = exp(-((x1-y1)/sigma[0])^2 - ((x2-y2)/sigma[1])^2)   (reference src/kernels.py:91-179; no factor 1/2)"""

    def _precisions(self, sigma):
        return 2.0 / (float(sigma[0]) ** 2), 2.0 / (float(sigma[1]) ** 2)

    Delta_x_y_kappa = _make('Delta_x_Delta_y_kappa')      # duplicate of the reference class (src/kernels.py:163-166)


# ---- Matern family, nu = m + 1/2 with m = 2, 3, 4 ("Matern kernels") ----------------------------------------
# reverse Bessel polynomials theta_0 .. theta_4, coefficients in ascending powers of t
_THETA = ((1.0,), (1.0, 1.0), (3.0, 3.0, 1.0), (15.0, 15.0, 6.0, 1.0), (105.0, 105.0, 45.0, 10.0, 1.0))


def _theta(n, t):
    v = _THETA[n][-1] + 0.0 * t
    for c in _THETA[n][-2::-1]:
        v = v * t + c
    return v


def _matern_partials(m, r1, r2, d1, d2):
    """{(n1, n2): d_{d1}^{n1} d_{d2}^{n2} kappa} for n1 + n2 <= 4, r_i = 1 / rho_i: the arithmetic of matern_partials in
    csrc/gpk_assemble_matern.hip.  kappa = phi(|u|^2 / 2), u_i = d_i r_i, t = a |u|, a^2 = 2 nu, and with
    G_k = phi^(k) = (-a^2)^k exp(-t) theta_{m-k}(t) / theta_m(0) the chain rule gives
        P[n1, n2] = sum_{j1, j2} c(n1, j1) c(n2, j2) G_{n1+n2-j1-j2} u1^{n1-2 j1} u2^{n2-2 j2},  c(n, j) = n! / (j! (n-2j)! 2^j).
    G_3 (m = 2) and G_4 (m = 2, 3) are singular at t = 0 (theta_{-1} = 1/t, theta_{-2} = (1+t)/t^3) and only ever multiply monomials of
    degree >= 2 and 4: their products are formed with the unit direction n = u / |u| (bounded) and vanish with t; at |u| = 0 the
    direction is taken as 0, which makes them exactly 0, their limit."""
    a2 = 2.0 * m + 1.0
    a = float(np.sqrt(a2))
    th0 = _THETA[m][0]
    x, y = d1 * r1, d2 * r2
    xx, yy, xy = x * x, y * y, x * y
    w = xx + yy
    un = np.sqrt(w)
    t = a * un
    e = np.exp(-t)
    G = [e * ((-a2) ** k / th0) * _theta(m - k, t) for k in range(min(m, 4) + 1)]
    G0, G1, G2 = G[0], G[1], G[2]
    if m == 4:
        T3 = {'xx': G[3] * xx, 'xy': G[3] * xy, 'yy': G[3] * yy}
        T4 = [G[4] * (xx * xx), G[4] * (xx * xy), G[4] * (xx * yy), G[4] * (xy * yy), G[4] * (yy * yy)]
    else:
        with np.errstate(divide='ignore', invalid='ignore'):
            inv = np.where(w > 0.0, 1.0 / un, 0.0)
        nx, ny = x * inv, y * inv
        qxx, qxy, qyy = nx * x, nx * y, ny * y
        if m == 3:
            K4 = (a2 ** 3 * a / th0) * e
            T3 = {'xx': G[3] * xx, 'xy': G[3] * xy, 'yy': G[3] * yy}
            T4 = [K4 * (qxx * xx), K4 * (qxx * xy), K4 * (qxx * yy), K4 * (qyy * xy), K4 * (qyy * yy)]
        else:
            k3 = a2 ** 2 * a / th0
            K3, K4 = -k3 * e, (k3 * e) * (1.0 + t)
            T3 = {'xx': K3 * qxx, 'xy': K3 * qxy, 'yy': K3 * qyy}
            nxx, nxy, nyy = nx * nx, nx * ny, ny * ny
            T4 = [K4 * (nxx * qxx), K4 * (nxx * qxy), K4 * (nxy * qxy), K4 * (nyy * qxy), K4 * (nyy * qyy)]
    r11, r22, r12 = r1 * r1, r2 * r2, r1 * r2
    return {
        (0, 0): G0,
        (1, 0): r1 * (G1 * x), (0, 1): r2 * (G1 * y),
        (2, 0): r11 * (G2 * xx + G1), (1, 1): r12 * (G2 * xy), (0, 2): r22 * (G2 * yy + G1),
        (3, 0): (r11 * r1) * (x * (3.0 * G2 + T3['xx'])), (2, 1): (r11 * r2) * (y * (T3['xx'] + G2)),
        (1, 2): (r22 * r1) * (x * (T3['yy'] + G2)), (0, 3): (r22 * r2) * (y * (3.0 * G2 + T3['yy'])),
        (4, 0): (r11 * r11) * (T4[0] + (6.0 * T3['xx'] + 3.0 * G2)), (3, 1): (r11 * r12) * (3.0 * T3['xy'] + T4[1]),
        (2, 2): (r11 * r22) * (T4[2] + ((T3['xx'] + T3['yy']) + G2)),
        (1, 3): (r22 * r12) * (3.0 * T3['xy'] + T4[3]), (0, 4): (r22 * r22) * (T4[4] + (6.0 * T3['yy'] + 3.0 * G2)),
    }


class Matern_kernel(_ClosedFormKernel):
    """kappa = exp(-t) theta_m(t) / theta_m(0) with nu = m + 1/2 in (5/2, 7/2, 9/2), t = sqrt(2 nu) |((x1-y1)/rho_1, (x2-y2)/rho_2)|;
    nu = 5/2: (1 + t + t^2/3) exp(-t).  The last argument of every method is the length scale rho (both axes) or a pair.  Every method
    name of the Gaussian classes; d_x^alpha d_y^beta kappa = (-1)^{|beta|} d_d^{alpha+beta} kappa with the partials of _matern_partials.
    nu = 3/2 is not offered: that kernel is not C^4 at coincident points, so Delta_x Delta_y kappa(x, x) -- the diagonal of a Laplacian
    block -- does not exist."""
    _ORDERS = {2.5: 2, 3.5: 3, 4.5: 4}

    def __init__(self, nu):
        try:
            self.m = self._ORDERS[float(nu)]
        except (KeyError, TypeError, ValueError):
            raise ValueError(f'Matern_kernel: nu = {nu!r} is not available; 2.5, 3.5 or 4.5 (nu = 1.5 is not C^4 at coincident points)')
        self.nu = float(nu)

    @staticmethod
    def _scales(rho):
        rho = np.atleast_1d(np.asarray(rho, dtype=np.float64))
        if rho.size not in (1, 2) or not np.all(np.isfinite(rho)) or not np.all(rho > 0):
            raise ValueError(f'Matern_kernel: length scale(s) {rho!r}: one or two finite values > 0')
        return 1.0 / float(rho[0]), 1.0 / float(rho[-1])

    def _eval(self, fx, fy, x1, x2, y1, y2, rho):
        r1, r2 = self._scales(rho)
        d1 = np.asarray(x1, dtype=np.float64) - np.asarray(y1, dtype=np.float64)
        d2 = np.asarray(x2, dtype=np.float64) - np.asarray(y2, dtype=np.float64)
        D = _matern_partials(self.m, r1, r2, d1, d2)
        total = 0.0
        for (a1, a2) in fx:
            for (b1, b2) in fy:
                term = D[(a1 + b1, a2 + b2)]
                total = total - term if (b1 + b2) & 1 else total + term
        return total


class Matern52_kernel(Matern_kernel):
    def __init__(self):
        Matern_kernel.__init__(self, 2.5)


class Matern72_kernel(Matern_kernel):
    def __init__(self):
        Matern_kernel.__init__(self, 3.5)


class Matern92_kernel(Matern_kernel):
    def __init__(self):
        Matern_kernel.__init__(self, 4.5)


# ---- periodic kernel ("Periodic kernel") ----------------------------------------------------------------------
def _sincospi(x):
    """(sin pi x, cos pi x) with exact argument reduction, as sincospi on the device: x is reduced to r in [-1, 1] modulo 2 and then to
    t = r - q / 2 in [-1/4, 1/4], q the nearest half-integer count -- both steps exact in floating point -- so that the only rounding is
    that of pi t and of the sine / cosine of a small argument."""
    x = np.asarray(x, dtype=np.float64)
    r = x - 2.0 * np.round(0.5 * x)
    q = np.round(2.0 * r)
    t = np.pi * (r - 0.5 * q)
    s, c = np.sin(t), np.cos(t)
    k = q.astype(np.int64) % 4
    return np.choose(k, [s, c, -s, -c]), np.choose(k, [c, -s, -c, s])


def _periodic_table(p, L, d):
    """(h0..h4, z) of one axis with precision p and period L > 0 at d, h_m = (-1)^m kappa^(m) / kappa for
    kappa(d) = exp(-(2 p / w^2) sin^2(w d / 2)), w = 2 pi / L, and z = sin(w d / 2): with s = (p / w) sin w d, c = p cos w d
        h1 = s, h2 = s^2 - c, h3 = s (s^2 - 3 c - w^2), h4 = s^4 - 6 s^2 c + 3 c^2 - 4 w^2 s^2 + w^2 c.
    At d = 0 the table is (1, 0, -p, 0, 3 p^2 + w^2 p), and it tends to the Hermite table as w -> 0."""
    w = 2.0 * np.pi / L
    sh, ch = _sincospi(d / L)
    s = (p / w) * (2.0 * sh * ch)
    c = p * (1.0 - 2.0 * sh * sh)
    s2, w2 = s * s, w * w
    return (1.0, s, s2 - c, s * (s2 - 3.0 * c - w2), s2 * (s2 - 6.0 * c - 4.0 * w2) + c * (3.0 * c + w2)), sh


class Periodic_kernel(_ClosedFormKernel):
    """Product over the two axes of kappa_k(d) = exp(-(2 p_k / w_k^2) sin^2(w_k d / 2)), p_k = 2 / sigma_k^2, w_k = 2 pi / L_k, on an axis
    with period L_k > 0, and of the anisotropic Gaussian factor exp(-p_k d^2 / 2) on an axis with L_k = 0.  The last argument of every
    method is (sigma_1, sigma_2, L_1, L_2).  Every method name of the Gaussian classes; the same closed form with the table of
    _periodic_table in place of the Hermite table on a periodic axis -- what csrc/gpk_assemble_periodic.hip computes per point pair."""

    @staticmethod
    def _axes(param):
        v = np.atleast_1d(np.asarray(param, dtype=np.float64))
        if v.size != 4 or not np.all(np.isfinite(v)) or not np.all(v[:2] > 0) or not np.all(v[2:] >= 0) or not np.any(v[2:] > 0):
            raise ValueError(f'Periodic_kernel: (sigma_1, sigma_2, L_1, L_2) = {param!r}: two finite length scales > 0 and two finite '
                             'periods >= 0, not both 0 (that kernel is Anisotropic_Gaussian_kernel)')
        return [(2.0 / float(v[k]) ** 2, float(v[2 + k])) for k in range(2)]

    def _eval(self, fx, fy, x1, x2, y1, y2, param):
        d = (np.asarray(x1, dtype=np.float64) - np.asarray(y1, dtype=np.float64),
             np.asarray(x2, dtype=np.float64) - np.asarray(y2, dtype=np.float64))
        tables, expo = [], 0.0
        for (p, L), dk in zip(self._axes(param), d):
            if L > 0.0:
                h, z = _periodic_table(p, L, dk)
                expo = expo + (2.0 * p / (2.0 * np.pi / L) ** 2) * z * z
            else:
                h = _hermite(p, dk)
                expo = expo + 0.5 * p * dk * dk
            tables.append(h)
        a, b = tables
        total = 0.0
        for (a1, a2) in fx:
            for (b1, b2) in fy:
                term = a[a1 + b1] * b[a2 + b2]
                total = total - term if (a1 + a2) & 1 else total + term
        return total * np.exp(-expo)
