"""The reaction term tau(u) of the semilinear equation -psi[u] + tau(u) = f and its derivative on the host (numpy): the mirror of
nl_tau / nl_dtau of csrc/gpk_common.h.  Every host expression of the elliptic classes that involves tau goes through one of these
objects; the device evaluates the same family (gpk.h, GPK_NL_*).

    power   p0 u^p1                      (alpha u^m: the reference's equation)
    exp     p0 exp(p1 u)                 Bratu / Liouville
    sinh    p0 sinh(p1 u)                Poisson-Boltzmann
    sin     p0 sin(p1 u)                 sine-Gordon
    cubic   p0 u + p1 u^2 + p2 u^3       Allen-Cahn (-1, 0, 1) / eps^2, Fisher-KPP (-r, r, 0)
"""
import numpy as onp

KINDS = {'power': 0, 'exp': 1, 'sinh': 2, 'sin': 3, 'cubic': 4}            # name -> GPK_NL_*
ARITY = {'power': 2, 'exp': 2, 'sinh': 2, 'sin': 2, 'cubic': 3}
_FORM = {'power': '{0}*u^{1}', 'exp': '{0}*exp({1}*u)', 'sinh': '{0}*sinh({1}*u)', 'sin': '{0}*sin({1}*u)',
         'cubic': '{0}*u + {1}*u^2 + {2}*u^3'}


class Nonlinearity(object):
    """tau(u), dtau(u) for numpy arrays; name, kind (GPK_NL_*), params (p0, p1, p2)"""

    def __init__(self, name, *params):
        if name not in KINDS:
            raise ValueError(f'nonlinearity {name!r}: one of {tuple(KINDS)}')
        if len(params) != ARITY[name]:
            raise ValueError(f'nonlinearity {name!r} takes {ARITY[name]} parameters, got {len(params)}')
        self.name = name
        self.kind = KINDS[name]
        self.raw = tuple(params)                                         # as given (the power law keeps the user's alpha and m untouched)
        self.params = tuple(float(p) for p in params) + (0.0,) * (3 - len(params))

    @classmethod
    def power(cls, alpha, m):
        return cls('power', alpha, m)

    @classmethod
    def make(cls, spec, alpha=1.0, m=3):
        """spec: None (the power law alpha u^m), a Nonlinearity, or a sequence (name, parameters...)"""
        if spec is None:
            return cls.power(alpha, m)
        if isinstance(spec, cls):
            return spec
        if isinstance(spec, str) or not hasattr(spec, '__len__') or len(spec) < 1 or not isinstance(spec[0], str):
            raise ValueError(f"nonlinearity {spec!r}: None or (name, parameters...), e.g. ('exp', -1.0, 1.0)")
        return cls(spec[0], *spec[1:])

    def tau(self, u):
        p0, p1, p2 = self.raw + (0.0,) * (3 - len(self.raw))
        if self.name == 'power':
            return p0 * (u ** p1)
        if self.name == 'exp':
            return p0 * onp.exp(p1 * u)
        if self.name == 'sinh':
            return p0 * onp.sinh(p1 * u)
        if self.name == 'sin':
            return p0 * onp.sin(p1 * u)
        return u * (p0 + u * (p1 + p2 * u))

    def dtau(self, u):
        p0, p1, p2 = self.raw + (0.0,) * (3 - len(self.raw))
        if self.name == 'power':
            return p0 * p1 * (u ** (p1 - 1))
        if self.name == 'exp':
            return p0 * p1 * onp.exp(p1 * u)
        if self.name == 'sinh':
            return p0 * p1 * onp.cosh(p1 * u)
        if self.name == 'sin':
            return p0 * p1 * onp.cos(p1 * u)
        return p0 + u * (2.0 * p1 + 3.0 * p2 * u)

    def describe(self):
        """tau(u) as text, e.g. -1.0*exp(1.0*u)"""
        return _FORM[self.name].format(*self.params)


class GradientNonlinearity(object):
    """N(u, p, q) = u (a1 p + a2 q) + b (p^2 + q^2) + c1 u + c3 u^3 of the semilinear equation -eps Laplace(u) + N(u, grad u) = f
    (p = d_1 u, q = d_2 u) and its partial derivatives on the host (numpy): the mirror of sl_N / sl_dN of csrc/gpk_common.h, written in
    the same order of operations.  params = (a1, a2, b, c1, c3), what gpk_gn_problem carries as gq_a1 .. gq_c3.

        ('burgers', a1, a2)           u (a1 p + a2 q)              steady viscous Burgers / convection along (a1, a2)
        ('hamilton_jacobi', b, c1)    b (p^2 + q^2) + c1 u         viscous Hamilton-Jacobi, stationary KPZ
        ('eikonal',)                  p^2 + q^2                    the regularised Eikonal equation (with f^2 as right-hand side)
    """
    PRESETS = {'burgers': 2, 'hamilton_jacobi': 2, 'eikonal': 0}

    def __init__(self, a1=0.0, a2=0.0, b=0.0, c1=0.0, c3=0.0):
        self.params = tuple(float(v) for v in (a1, a2, b, c1, c3))
        if not all(onp.isfinite(self.params)):
            raise ValueError(f'GradientNonlinearity: the coefficients must be finite, got {self.params}')
        self.a1, self.a2, self.b, self.c1, self.c3 = self.params

    @classmethod
    def make(cls, spec):
        """spec: a GradientNonlinearity, the five coefficients (a1, a2, b, c1, c3), or a preset (name, parameters...) of PRESETS"""
        if isinstance(spec, cls):
            return spec
        if isinstance(spec, str) or not hasattr(spec, '__len__') or len(spec) < 1:
            raise ValueError(f"nonlinearity {spec!r}: a GradientNonlinearity, (a1, a2, b, c1, c3) or a preset such as ('burgers', 1.0, 1.0)")
        if isinstance(spec[0], str):
            name, args = spec[0], tuple(spec[1:])
            if name not in cls.PRESETS:
                raise ValueError(f'nonlinearity preset {name!r}: one of {tuple(cls.PRESETS)}')
            if len(args) != cls.PRESETS[name]:
                raise ValueError(f'nonlinearity preset {name!r} takes {cls.PRESETS[name]} parameters, got {len(args)}')
            if name == 'burgers':
                return cls(a1=args[0], a2=args[1])
            if name == 'hamilton_jacobi':
                return cls(b=args[0], c1=args[1])
            return cls(b=1.0)
        if len(spec) != 5:
            raise ValueError(f'nonlinearity {spec!r}: five coefficients (a1, a2, b, c1, c3), got {len(spec)}')
        return cls(*spec)

    def N(self, u, p, q):
        a1, a2, b, c1, c3 = self.params
        return (u * (a1 * p + a2 * q) + b * (p * p + q * q)) + u * (c1 + c3 * (u * u))

    def dN(self, u, p, q):
        """(N_u, N_p, N_q)"""
        a1, a2, b, c1, c3 = self.params
        return (a1 * p + a2 * q) + (c1 + 3.0 * c3 * (u * u)), a1 * u + 2.0 * b * p, a2 * u + 2.0 * b * q

    def describe(self):
        a1, a2, b, c1, c3 = self.params
        return f'u*({a1}*u_x1 + {a2}*u_x2) + {b}*|grad u|^2 + {c1}*u + {c3}*u^3'


class GradientNonlinearity3d(object):
    """N(u, g) = u (a1 g1 + a2 g2 + a3 g3) + b1 g1^2 + b2 g2^2 + b3 g3^2 + c1 u + c3 u^3 of -psi[u] + N(u, grad u) = f in three dimensions
    (g_k = d_k u; with axis 3 as time set a3 = b3 = 0) and its four partial derivatives on the host (numpy): the mirror of sl3_N / sl3_dN
    of csrc/gpk_common.h, written in the same order of operations.  params = (a1, a2, a3, b1, b2, b3, c1, c3), what GNProblem takes as gq8.

        ('burgers', a1, a2[, a3])            u (a . g)                 viscous Burgers / convection along a
        ('hamilton_jacobi', b1, b2[, b3])    sum_k b_k g_k^2           viscous Hamilton-Jacobi, KPZ
        ('eikonal',)                         g1^2 + g2^2 + g3^2        the regularised Eikonal equation (with f^2 as right-hand side)
    """
    PRESETS = {'burgers': (2, 3), 'hamilton_jacobi': (2, 3), 'eikonal': (0,)}

    def __init__(self, a1=0.0, a2=0.0, a3=0.0, b1=0.0, b2=0.0, b3=0.0, c1=0.0, c3=0.0):
        self.params = tuple(float(v) for v in (a1, a2, a3, b1, b2, b3, c1, c3))
        if not all(onp.isfinite(self.params)):
            raise ValueError(f'GradientNonlinearity3d: the coefficients must be finite, got {self.params}')
        self.a1, self.a2, self.a3, self.b1, self.b2, self.b3, self.c1, self.c3 = self.params

    @classmethod
    def make(cls, spec):
        """spec: a GradientNonlinearity3d, the eight coefficients (a1, a2, a3, b1, b2, b3, c1, c3), or a preset (name, parameters...)"""
        if isinstance(spec, cls):
            return spec
        if isinstance(spec, str) or not hasattr(spec, '__len__') or len(spec) < 1:
            raise ValueError(f"nonlinearity {spec!r}: a GradientNonlinearity3d, (a1, a2, a3, b1, b2, b3, c1, c3) or a preset such as "
                             "('burgers', 1.0, 1.0)")
        if isinstance(spec[0], str):
            name, args = spec[0], tuple(spec[1:])
            if name not in cls.PRESETS:
                raise ValueError(f'nonlinearity preset {name!r}: one of {tuple(cls.PRESETS)}')
            if len(args) not in cls.PRESETS[name]:
                raise ValueError(f'nonlinearity preset {name!r} takes {" or ".join(str(n) for n in cls.PRESETS[name])} parameters, got {len(args)}')
            args = args + (0.0,) * (3 - len(args))
            if name == 'burgers':
                return cls(a1=args[0], a2=args[1], a3=args[2])
            if name == 'hamilton_jacobi':
                return cls(b1=args[0], b2=args[1], b3=args[2])
            return cls(b1=1.0, b2=1.0, b3=1.0)
        if len(spec) != 8:
            raise ValueError(f'nonlinearity {spec!r}: eight coefficients (a1, a2, a3, b1, b2, b3, c1, c3), got {len(spec)}')
        return cls(*spec)

    def N(self, u, g1, g2, g3):
        a1, a2, a3, b1, b2, b3, c1, c3 = self.params
        conv = u * ((a1 * g1 + a2 * g2) + a3 * g3)
        grad = (b1 * (g1 * g1) + b2 * (g2 * g2)) + b3 * (g3 * g3)
        return (conv + grad) + u * (c1 + c3 * (u * u))

    def dN(self, u, g1, g2, g3):
        """(N_u, N_g1, N_g2, N_g3)"""
        a1, a2, a3, b1, b2, b3, c1, c3 = self.params
        return (((a1 * g1 + a2 * g2) + a3 * g3) + (c1 + 3.0 * c3 * (u * u)), a1 * u + 2.0 * b1 * g1, a2 * u + 2.0 * b2 * g2,
                a3 * u + 2.0 * b3 * g3)

    def describe(self):
        a1, a2, a3, b1, b2, b3, c1, c3 = self.params
        return f'u*({a1}*u_x1 + {a2}*u_x2 + {a3}*u_x3) + {b1}*u_x1^2 + {b2}*u_x2^2 + {b3}*u_x3^2 + {c1}*u + {c3}*u^3'
