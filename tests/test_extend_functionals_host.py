"""Derivatives of the extension (gpk_extend_functionals) and the PDE residual (gpk_pde_residual): the host-side expectation and its CPU checks.

The expectation restates DESIGN.md section K from the oracle's pieces (oracle.gp_oracle.hermite, kernel_precisions) and the multi-index rule
    <F at x, G at y> kappa = sum_{alpha in F} sum_{beta in G} (-1)^{|alpha|} h_{alpha1+beta1}(p1, d1) h_{alpha2+beta2}(p2, d2) kappa,  d = x - y,
and is checked here against every closed form of the oracle that has a reference name (oracle.deriv_kernel).  The GPU tests
(test_gpu_extend_functionals.py, test_gpu_pde_residual.py) import `expect`, `residual` and the tables from this module."""
import os
import re

import numpy as np
import pytest

from oracle import gp_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps

FUNCTIONALS = ('value', 'd1', 'd2', 'd2d2', 'laplacian')                      # bit k of the GPK_FN_* mask = FUNCTIONALS[k]
MULTI = {'value': [(0, 0)], 'd1': [(1, 0)], 'd2': [(0, 1)], 'd2d2': [(0, 2)], 'laplacian': [(2, 0), (0, 2)]}
# column blocks of each layout: (functional, points) with points 'd' = domain, 'db' = domain + boundary (src/Gram_matrice.py:190-289)
BLOCKS = {
    'Nonlinear_elliptic': [('laplacian', 'd'), ('value', 'db')],
    'Burgers': [('d1', 'd'), ('d2', 'd'), ('d2d2', 'd'), ('value', 'db')],
    'Eikonal': [('d1', 'd'), ('d2', 'd'), ('laplacian', 'd'), ('value', 'db')],
    'Darcy_u': [('d1', 'd'), ('d2', 'd'), ('laplacian', 'd'), ('value', 'db')],
    'Darcy_a': [('d1', 'd'), ('d2', 'd'), ('value', 'd')],
}
# (row functional at x, column functional at y) -> method of src/kernels.py (oracle.deriv_kernel); pairs without one are not named there
REF_NAME = {
    ('value', 'value'): 'kappa',
    ('d1', 'value'): 'D_x1_kappa', ('d2', 'value'): 'D_x2_kappa', ('d2d2', 'value'): 'DD_x2_kappa', ('laplacian', 'value'): 'Delta_x_kappa',
    ('value', 'd1'): 'D_y1_kappa', ('value', 'd2'): 'D_y2_kappa', ('value', 'd2d2'): 'DD_y2_kappa', ('value', 'laplacian'): 'Delta_y_kappa',
    ('d1', 'd1'): 'D_x1_D_y1_kappa', ('d1', 'd2'): 'D_x1_D_y2_kappa', ('d1', 'd2d2'): 'D_x1_DD_y2_kappa',
    ('d2', 'd2'): 'D_x2_D_y2_kappa', ('d2', 'd1'): 'D_x2_D_y1_kappa', ('d2', 'd2d2'): 'D_x2_DD_y2_kappa',
    ('d2d2', 'd2d2'): 'DD_x2_DD_y2_kappa',
    ('laplacian', 'laplacian'): 'Delta_x_Delta_y_kappa', ('laplacian', 'd1'): 'Delta_x_D_y1_kappa', ('laplacian', 'd2'): 'Delta_x_D_y2_kappa',
}
KERNELS = (('Gaussian', 0.2), ('anisotropic_Gaussian', [0.3, 0.05]))


def pair(fx, fy, Xt, Y, kernel, kp):
    """(value, sum of |terms|) of <fx at Xt[i], fy at Y[j]> kappa, both (len(Xt), len(Y))"""
    p1, p2 = O.kernel_precisions(kernel, kp)
    Xt = np.asarray(Xt, dtype=np.float64).reshape(-1, 2); Y = np.asarray(Y, dtype=np.float64).reshape(-1, 2)
    d1 = Xt[:, None, 0] - Y[None, :, 0]
    d2 = Xt[:, None, 1] - Y[None, :, 1]
    kap = np.exp(-0.5 * (p1 * d1 * d1 + p2 * d2 * d2))
    one = np.ones_like(d1)
    h1 = (one,) + O.hermite(p1, d1)
    h2 = (one,) + O.hermite(p2, d2)
    val = np.zeros_like(d1); mag = np.zeros_like(d1)
    for a1, a2 in MULTI[fx]:
        for b1, b2 in MULTI[fy]:
            t = (-1.0) ** (a1 + a2) * h1[a1 + b1] * h2[a2 + b2] * kap
            val += t
            mag += np.abs(t)
    return val, mag


def expect(layout, fn, Xt, Xd, Xb, coeff, kernel, kp):
    """(out, terms): out[t] = sum over the layout's blocks and column points of <fn at Xt[t], block functional at y> kappa coeff, and
    terms[t] = the sum of the absolute values of its terms (the scale of the rounding bound)"""
    Xd = np.asarray(Xd, dtype=np.float64).reshape(-1, 2); Xb = np.asarray(Xb, dtype=np.float64).reshape(-1, 2)
    pts = {'d': Xd, 'db': np.concatenate([Xd, Xb], axis=0)}
    coeff = np.asarray(coeff, dtype=np.float64)
    out = np.zeros(len(Xt)); terms = np.zeros(len(Xt)); off = 0
    for fy, which in BLOCKS[layout]:
        Y = pts[which]
        c = coeff[off:off + len(Y)]
        V, A = pair(fn, fy, Xt, Y, kernel, kp)
        out += V @ c
        terms += A @ np.abs(c)
        off += len(Y)
    assert off == coeff.size, (layout, off, coeff.size)
    return out, terms


def residual(system, params, U, A, f):
    """(r, terms) of gpk_pde_residual in numpy: U rows value, d1, d2, laplacian (Burgers: value, u_t, u_x, u_xx); A rows value, d1, d2 of a"""
    u0, u1, u2, u3 = (np.asarray(U[k], dtype=np.float64) for k in range(4))
    f = np.asarray(f, dtype=np.float64)
    if system in ('Nonlinear_elliptic', 'Nonlinear_elliptic_relaxed'):
        al, m = params[0], params[1]
        t = [-u3, al * np.power(u0, m), -f]
    elif system == 'Burgers':
        al, nu = params[0], params[1]
        t = [u1, al * u0 * u2, -nu * u3, -f]
    elif system == 'Eikonal':
        t = [u1 * u1, u2 * u2, -f * f, -params[0] * u3]
    elif system == 'Darcy_flow2d':
        a0, a1, a2 = (np.asarray(A[k], dtype=np.float64) for k in range(3))
        ea = np.exp(a0)
        t = [-ea * u3, -ea * a1 * u1, -ea * a2 * u2, -f]
    else:
        raise ValueError(system)
    return sum(t), sum(np.abs(x) for x in t)


# ---- CPU tests --------------------------------------------------------------------------------------------------------
def test_header_declares_extend_functionals_and_residual():
    hdr = open(os.path.join(ROOT, 'include', 'gpk.h')).read()
    for name in ('gpk_extend_functionals', 'gpk_pde_residual'):
        assert re.search(r'\bint\s+' + name + r'\s*\(', hdr), name
    vals = dict(re.findall(r'\b(GPK_FN_[A-Z0-9]+)\s*=\s*(\d+)', hdr))
    assert vals == {'GPK_FN_VALUE': '1', 'GPK_FN_D1': '2', 'GPK_FN_D2': '4', 'GPK_FN_D2D2': '8', 'GPK_FN_LAPLACIAN': '16'}, vals


def test_ctypes_table_has_both_entry_points():
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'nonlinpdes-gpsolver_amd'))
    from gpk import _lib
    from gpk.device import FUNCTIONAL
    assert len(_lib.PROTOTYPES['gpk_extend_functionals'][1]) == 14
    assert len(_lib.PROTOTYPES['gpk_pde_residual'][1]) == 10
    assert FUNCTIONAL == {n: 1 << k for k, n in enumerate(FUNCTIONALS)}


@pytest.mark.parametrize('kernel,kp', KERNELS)
def test_pair_expectation_matches_the_oracle_closed_forms(kernel, kp):
    rng = np.random.RandomState(3)
    X = rng.uniform(-0.2, 1.2, (40, 2)); Y = rng.uniform(0, 1, (50, 2))
    Y[:5] = X[:5]                                                        # coincident points (d = 0)
    for (fx, fy), name in REF_NAME.items():
        V, A = pair(fx, fy, X, Y, kernel, kp)
        R = O.deriv_kernel(name, X[:, None, 0], X[:, None, 1], Y[None, :, 0], Y[None, :, 1], kernel, kp)
        assert np.all(np.abs(V - R) <= 16 * EPS * A + 1e-300), (fx, fy, name, np.max(np.abs(V - R) / (A + 1e-300)))
    assert len(REF_NAME) == 19


@pytest.mark.parametrize('layout', sorted(BLOCKS))
def test_value_row_is_construct_theta_test_times_coeff(layout):
    """the value row of the expectation is the reference's extension Theta_test @ coeff (oracle.construct_theta_test)"""
    rng = np.random.RandomState(5)
    Xd = rng.uniform(0, 1, (30, 2)); Xb = rng.uniform(0, 1, (8, 2)); Xt = rng.uniform(0, 1, (25, 2))
    kernel, kp = KERNELS[0]
    eqn = 'Darcy_flow2d' if layout.startswith('Darcy') else layout
    T = O.construct_theta_test(Xt, Xd, Xb, eqn, kernel, kp)
    if eqn == 'Darcy_flow2d':
        T = T[0] if layout == 'Darcy_u' else T[1]
    c = rng.normal(size=T.shape[1])
    out, terms = expect(layout, 'value', Xt, Xd, Xb, c, kernel, kp)
    assert np.all(np.abs(out - T @ c) <= 64 * EPS * terms)


def test_residual_formulas_vanish_on_exact_fields():
    """residual() of an exact solution's fields is zero: -Lap u + u^3 = f for the manufactured elliptic solution, and the
    Darcy relation for a = 0.3 x, u = x y (so -(e^a)(0 + 0.3 y) = f)"""
    pi = np.pi
    x = np.linspace(0.1, 0.9, 7); y = np.linspace(0.2, 0.8, 7)
    u = np.sin(pi * x) * np.sin(pi * y)
    lap = -2 * pi ** 2 * u
    U = [u, pi * np.cos(pi * x) * np.sin(pi * y), pi * np.sin(pi * x) * np.cos(pi * y), lap]
    r, terms = residual('Nonlinear_elliptic', (1.0, 3.0), U, None, -lap + u ** 3)
    assert np.all(np.abs(r) <= 8 * EPS * terms)
    Ua = [x * y, y, x, 0 * x]; Aa = [0.3 * x, 0.3 + 0 * x, 0 * x]
    r, terms = residual('Darcy_flow2d', None, Ua, Aa, -np.exp(0.3 * x) * 0.3 * y)
    assert np.all(np.abs(r) <= 8 * EPS * terms)
