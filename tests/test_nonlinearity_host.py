"""Reaction terms beyond alpha u^m (src/nonlinearity.py, gpk.h GPK_NL_*) without a device: the host tau / tau' against long double, the
arguments of the elliptic classes, the facade's log lines, the drivers' flags, the binding's struct mirror and symbol list."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'nonlinpdes-gpsolver_amd')
if PKG not in sys.path:
    sys.path.insert(0, PKG)

import _nl_reference as NL  # noqa: E402
from src.nonlinearity import Nonlinearity  # noqa: E402

LD, EPS = NL.LD, NL.EPS
# p1 a power of two for the transcendental kinds: p1 u is then exact, and 2 eps covers the function (1 ulp) and the two products
SPECS = [('power', 1.3, 3.0), ('exp', -0.7, 2.0), ('sinh', 1.3, 0.5), ('sin', 0.9, 2.0), ('cubic', -1.1, 0.3, 0.8)]


def _u(name):
    rng = np.random.RandomState(3)
    u = rng.uniform(-1.2, 1.2, 4000)
    return np.abs(u) + 0.05 if name == 'power' else u                   # (the power law on positive arguments: u^m with real m)


@pytest.mark.parametrize('spec', SPECS, ids=lambda s: s[0])
def test_host_tau_and_dtau_against_long_double(spec):
    """<= 2 eps of the magnitude sum of the terms (= |value| for every kind but the cubic)"""
    tau = Nonlinearity.make(spec)
    u = _u(spec[0])
    for got, (ref, mag) in ((tau.tau(u), NL.tau_ld(spec[0], tau.params, u)), (tau.dtau(u), NL.dtau_ld(spec[0], tau.params, u))):
        err = np.abs(got.astype(LD) - ref)
        assert np.all(err <= 2 * EPS * mag), (spec, float(np.max(err / (EPS * mag))))


@pytest.mark.parametrize('spec', SPECS, ids=lambda s: s[0])
def test_dtau_is_the_derivative_of_tau(spec):
    """central difference of tau in long double, step 1e-6, agreement 1e-9 (relative to 1 + |tau'|)"""
    tau = Nonlinearity.make(spec)
    u = _u(spec[0]).astype(LD)
    h = LD(1e-6)
    fd = (NL.tau_ld(spec[0], tau.params, u + h)[0] - NL.tau_ld(spec[0], tau.params, u - h)[0]) / (2 * h)
    d = tau.dtau(u.astype(np.float64))
    # (u + h is not a float64: evaluate the long-double tau directly on long doubles)
    assert np.all(np.abs(d.astype(LD) - fd) <= 1e-9 * (1 + np.abs(fd))), float(np.max(np.abs(d.astype(LD) - fd)))


def test_cubic_with_only_the_third_coefficient_is_the_power_law():
    u = _u('cubic')
    a = 1.7
    c, p = Nonlinearity('cubic', 0, 0, a), Nonlinearity.power(a, 3)
    assert np.all(np.abs(c.tau(u) - p.tau(u)) <= 4 * EPS * np.abs(p.tau(u)))
    assert np.all(np.abs(c.dtau(u) - p.dtau(u)) <= 4 * EPS * np.abs(p.dtau(u)))


def test_power_mirror_spells_the_expressions_of_the_classes():
    """None -> the power law with the user's alpha and m untouched (an int m stays an int: u ** 3, not u ** 3.0)"""
    u = _u('cubic')
    t = Nonlinearity.make(None, alpha=2, m=3)
    assert np.array_equal(t.tau(u), 2 * (u ** 3)) and np.array_equal(t.dtau(u), 2 * 3 * (u ** (3 - 1)))
    assert t.kind == 0 and t.params == (2.0, 3.0, 0.0)


def test_argument_validation():
    from src.PDEs import Nonlinear_elliptic2d, Nonlinear_elliptic3d
    for cls in (Nonlinear_elliptic2d, Nonlinear_elliptic3d):
        for bad in (('tanh', 1.0, 1.0), ('exp', 1.0), ('exp', 1.0, 2.0, 3.0), ('cubic', 1.0, 2.0), 'exp', ()):
            with pytest.raises(ValueError):
                cls(nonlinearity=bad)
        e = cls(alpha=2.0, m=5)
        assert e.nonlinearity is None and e._gn_params() == (2.0, 5.0, 0.0) and e._nl_args() == {}
        e = cls(nonlinearity=('exp', -1.0, 1.0))
        assert e._gn_params() == (1.0, 3.0, 0.0)                      # the tuple keeps what it returns for the power law
        assert e._nl_args() == dict(p0=-1.0, p1=1.0, p2=0.0, nonlin=1)
        e = cls(nonlinearity=('cubic', -1, 0, 1))
        assert e._nl_args() == dict(p0=-1.0, p1=0.0, p2=1.0, nonlin=4)
        assert cls(nonlinearity=('power', 2.0, 3.0))._nl_args() == {}


class _Cfg:
    alpha, m = 1.0, 3.0


def _header(cfg, pde):
    from src.solver import _EQUATIONS
    _, header, params = _EQUATIONS[pde]
    return header(cfg) + [params(cfg)]


def test_facade_log_lines():
    cfg = _Cfg()
    assert _header(cfg, 'Nonlinear_elliptic') == ['[Equation type] Nonlinear elliptic equation', '[Equation form] - \\Delta u + alpha*u^m = f',
                                                 '[Equation parameter] alpha = 1.0, m = 3.0']
    assert _header(cfg, 'Nonlinear_elliptic3d') == ['[Equation type] Nonlinear elliptic equation in three space dimensions',
                                                   '[Equation form] - \\Delta u + alpha*u^m = f', '[Equation parameter] alpha = 1.0, m = 3.0']
    cfg.nonlinearity = None
    assert _header(cfg, 'Nonlinear_elliptic')[1:] == ['[Equation form] - \\Delta u + alpha*u^m = f', '[Equation parameter] alpha = 1.0, m = 3.0']
    cfg.nonlinearity = 'power'                                           # what the drivers' parser leaves there by default
    assert _header(cfg, 'Nonlinear_elliptic')[1:] == ['[Equation form] - \\Delta u + alpha*u^m = f', '[Equation parameter] alpha = 1.0, m = 3.0']
    cfg.nonlinearity = 'exp'                                             # a bare name of another kind is not a specification
    with pytest.raises(ValueError):
        _header(cfg, 'Nonlinear_elliptic')
    cfg.nonlinearity = ('sinh', 4.0, 1.0)
    for pde in ('Nonlinear_elliptic', 'Nonlinear_elliptic3d'):
        lines = _header(cfg, pde)
        assert lines[1] == '[Equation form] - \\Delta u + tau(u) = f, tau(u) = 4.0*sinh(1.0*u)'
        assert lines[-1] == "[Equation parameter] nonlinearity = sinh, parameters = (4.0, 1.0)"
    cfg.operator = lambda *x: None
    assert _header(cfg, 'Nonlinear_elliptic3d')[1].startswith('[Equation form] - psi[u] + tau(u) = f')


def test_facade_passes_the_nonlinearity_to_the_class():
    from src.solver import solver_GP
    cfg = _Cfg()
    cfg.nonlinearity = ('cubic', -4, 0, 4)
    s = solver_GP(cfg, PDE_type='Nonlinear_elliptic')
    s.set_equation(bdy=lambda a, b: 0 * a, rhs=lambda a, b: 0 * a, print_option=False)
    assert s.eqn.nonlinearity.name == 'cubic' and s.eqn.nonlinearity.params == (-4.0, 0.0, 4.0)
    s = solver_GP(_Cfg(), PDE_type='Nonlinear_elliptic')
    s.set_equation(bdy=lambda a, b: 0 * a, rhs=lambda a, b: 0 * a, print_option=False)
    assert s.eqn.nonlinearity is None


@pytest.mark.parametrize('driver', ('main_NonLinElliptic2d.py', 'main_NonLinElliptic3d.py'))
def test_driver_help_lists_the_flags(driver):
    out = subprocess.run([sys.executable, os.path.join(PKG, driver), '--help'], capture_output=True, text=True, cwd=PKG, timeout=120)
    assert out.returncode == 0, out.stderr
    assert '--nonlinearity' in out.stdout and '--nl_params' in out.stdout
    assert re.search(r'power,\s*exp,\s*sinh,\s*sin,\s*cubic', out.stdout)


def test_driver_right_hand_sides_take_tau():
    import main_NonLinElliptic2d as d2
    import main_NonLinElliptic3d as d3
    rng = np.random.RandomState(0)
    x = rng.uniform(0, 1, (3, 50))
    tau = Nonlinearity('exp', -1.0, 1.0)
    u, f = d2.manufactured(tau)
    _, f0 = d2.manufactured(1.0, 3.0)
    assert np.allclose(f(x[0], x[1]) - tau.tau(u(x[0], x[1])), f0(x[0], x[1]) - u(x[0], x[1]) ** 3.0, rtol=0, atol=1e-9)
    u3, f3 = d3.parabolic_manufactured(tau, 0.2)
    _, f30 = d3.parabolic_manufactured(1.0, 3.0, 0.2)
    assert np.allclose(f3(*x) - tau.tau(u3(*x)), f30(*x) - u3(*x) ** 3.0, rtol=0, atol=1e-9)
    cfg = d2.parse(['--nonlinearity', 'cubic', '--nl_params=-1,0,1'])
    from _driver_common import nonlinearity_from
    t, spec = nonlinearity_from(cfg)
    assert spec is t and t.params == (-1.0, 0.0, 1.0)
    cfg = d2.parse([])
    t, spec = nonlinearity_from(cfg)
    assert spec is None and t.kind == 0
    with pytest.raises(SystemExit):
        nonlinearity_from(d2.parse(['--nonlinearity', 'exp', '--nl_params', '1,2,3']))


def test_binding_declares_the_fields_and_the_entry():
    import gpk
    import gpk._lib as L
    names = [n for n, _ in L.GNProblemStruct._fields_]
    assert names[-2:] == ['nonlin', 'p2']
    assert 'gpk_pde_residual_nl' in gpk.declared_symbols()
    assert gpk.NONLIN == {'power': 0, 'exp': 1, 'sinh': 2, 'sin': 3, 'cubic': 4}
    hdr = open(os.path.join(ROOT, 'include', 'gpk.h')).read()
    assert re.search(r'GPK_NL_POWER = 0, GPK_NL_EXP = 1, GPK_NL_SINH = 2, GPK_NL_SIN = 3, GPK_NL_CUBIC = 4', hdr)
    assert 'int gpk_pde_residual_nl(' in hdr


def test_budgets_and_reference_linearisation():
    """the budgets follow from the measured figures, and the long-double linearisation agrees with the host mirror"""
    assert NL.build_budget('cubic') == 5.5
    for k in ('exp', 'sinh', 'sin'):
        assert 4.5 < NL.build_budget(k) < 5.0
    for kind in NL.KINDS:
        for system in ('elliptic', 'relaxed'):
            cs = NL.case(kind, system, 37, 12)
            lin = NL.linearise(cs, cs.z0)
            tau = Nonlinearity(kind, *cs.params[:3 if kind == 'cubic' else 2])
            w = cs.z0[-37:]
            rs = 1.0 if system == 'elliptic' else 1.0 / np.sqrt(cs.lam)
            A = lin.dense(np.float64)
            r0 = 0 if system == 'elliptic' else 2 * 37 + 12
            c0 = 0 if system == 'elliptic' else 37
            assert np.allclose(A[r0 + np.arange(37), c0 + np.arange(37)], tau.dtau(w) * rs, rtol=1e-14, atol=1e-15)
            NL.check_build(lin, A, lin.F.astype(np.float64), 1.0, (kind, system))       # the rounded reference passes its own gate
            bad = lin.F.astype(np.float64).copy(); bad[r0] *= 1 + 1e-11
            with pytest.raises(AssertionError):
                NL.check_build(lin, A, bad, NL.build_budget(kind))
