"""The quasilinear equations of Quasilinear2d (src/PDEs.py) on the host: each equation solved for the Laplacian, Laplace(u) = G(f; v), with
v = (v0, p, q, D, M) = (u, d_1 u, d_2 u, (d_11 - d_22) u, 2 d_12 u), its five partial derivatives, and the equation in its divergence /
determinant form.  The device's spelling is ql_G / ql_dG / ql_residual of csrc/gpk_common.h (include/gpk.h, GPK_QL_*); this module is
what GN_loss and the manufactured right-hand sides of main_Quasilinear2d.py evaluate in numpy.

    mean_curvature   (kappa)      div(grad u / sqrt(1 + |grad u|^2)) = f + kappa u
    p_laplace        (m, delta)   div((delta^2 + |grad u|^2)^((m-2)/2) grad u) = f
    gauss_curvature  (e)          det D^2 u = f (1 + |grad u|^2)^e, convex branch
"""
import math

import numpy as onp

from gpk.device import QL_KIND


class QuasilinearEquation(object):
    """kind: a name of QL_KIND; params: the three doubles (p0, p1, p2) that travel in gpk_gn_problem"""

    def __init__(self, kind, params):
        self.kind = kind
        self.id = QL_KIND[kind]
        self.params = tuple(float(v) for v in params)

    @classmethod
    def make(cls, equation):
        """('mean_curvature', kappa) | ('p_laplace', m, delta) | ('gauss_curvature', e), missing parameters at their defaults
        (kappa = 0: the minimal-surface equation with a source; delta = 1; e = 2: prescribed Gauss curvature), or a QuasilinearEquation"""
        if isinstance(equation, cls):
            return equation
        if isinstance(equation, str):
            equation = (equation,)
        kind, args = equation[0], [float(v) for v in equation[1:]]
        if kind not in QL_KIND:
            raise ValueError(f'Quasilinear2d: unknown equation {kind!r}; one of {sorted(QL_KIND)}')
        defaults = {'mean_curvature': [0.0], 'p_laplace': [3.0, 1.0], 'gauss_curvature': [2.0]}[kind]
        if len(args) > len(defaults):
            raise ValueError(f'Quasilinear2d: {kind} takes at most {len(defaults)} parameter(s), got {len(args)}')
        args = args + defaults[len(args):]
        if not all(math.isfinite(v) for v in args):
            raise ValueError(f'Quasilinear2d: the parameters of {kind} must be finite, got {args}')
        if kind == 'p_laplace' and not (args[0] > 0 and args[1] > 0):
            raise ValueError(f'Quasilinear2d: p_laplace needs m > 0 and delta > 0, got m = {args[0]}, delta = {args[1]}')
        return cls(kind, (args + [0.0, 0.0])[:3])

    def G(self, f, v0, p, q, D, M):
        g2 = p * p + q * q
        if self.kind == 'gauss_curvature':
            with onp.errstate(invalid='ignore'):
                return onp.sqrt(D * D + M * M + 4.0 * f * (1.0 + g2) ** self.params[0])
        Q = D * (p * p - q * q) + 2.0 * p * q * M
        if self.kind == 'p_laplace':
            m, dd = self.params[0], self.params[1] ** 2
            return (2.0 * f * (dd + g2) ** (0.5 * (4.0 - m)) - (m - 2.0) * Q) / (2.0 * dd + m * g2)
        W2 = 1.0 + g2
        return (2.0 * W2 * onp.sqrt(W2) * (f + self.params[0] * v0) + Q) / (1.0 + W2)

    def dG(self, f, v0, p, q, D, M):
        """(dG/dv0, dG/dp, dG/dq, dG/dD, dG/dM)"""
        g2 = p * p + q * q
        zero = 0.0 * g2
        if self.kind == 'gauss_curvature':
            e, W2 = self.params[0], 1.0 + g2
            G = self.G(f, v0, p, q, D, M)
            c = 4.0 * f * e * W2 ** (e - 1.0)
            return zero, c * p / G, c * q / G, D / G, M / G
        Q = D * (p * p - q * q) + 2.0 * p * q * M
        Qp, Qq = 2.0 * (p * D + q * M), 2.0 * (p * M - q * D)
        if self.kind == 'p_laplace':
            m, dd = self.params[0], self.params[1] ** 2
            s, a, c = dd + g2, 0.5 * (4.0 - m), m - 2.0
            E = 2.0 * dd + m * g2
            G = (2.0 * f * s ** a - c * Q) / E
            k = 4.0 * f * a * s ** (a - 1.0)
            return zero, (k * p - c * Qp - 2.0 * m * p * G) / E, (k * q - c * Qq - 2.0 * m * q * G) / E, -c * (p * p - q * q) / E, -c * 2.0 * p * q / E
        kappa = self.params[0]
        W2 = 1.0 + g2
        W, r, E = onp.sqrt(W2), f + kappa * v0, 1.0 + W2
        G = (2.0 * W2 * W * r + Q) / E
        return (2.0 * W2 * W * kappa / E + zero, (6.0 * W * p * r + Qp - 2.0 * p * G) / E, (6.0 * W * q * r + Qq - 2.0 * q * G) / E,
                (p * p - q * q) / E, 2.0 * p * q / E)

    def operator(self, u, u1, u2, u11, u12, u22):
        """the left-hand side of the equation in its divergence / determinant form WITHOUT f: what a manufactured solution is put into
        to get its right-hand side (mean curvature: f = operator - kappa u; Gauss curvature: f = operator / (1 + |grad u|^2)^e)"""
        g2 = u1 * u1 + u2 * u2
        T = u1 * u1 * u11 + 2.0 * u1 * u2 * u12 + u2 * u2 * u22
        lap = u11 + u22
        if self.kind == 'gauss_curvature':
            return u11 * u22 - u12 * u12
        if self.kind == 'p_laplace':
            m, s = self.params[0], self.params[1] ** 2 + g2
            return s ** (0.5 * (m - 4.0)) * (s * lap + (m - 2.0) * T)
        W2 = 1.0 + g2
        return (W2 * lap - T) / (W2 * onp.sqrt(W2))

    def rhs_of(self, u, u1, u2, u11, u12, u22):
        """f for which (u, its derivatives) solves the equation"""
        op = self.operator(u, u1, u2, u11, u12, u22)
        if self.kind == 'gauss_curvature':
            return op / (1.0 + u1 * u1 + u2 * u2) ** self.params[0]
        if self.kind == 'mean_curvature':
            return op - self.params[0] * u
        return op
