"""The periodic kernel (GPK_KERNEL_PERIODIC = 16) on the device: nugget, rejections, the class API end to end and the driver (modelled
on tests/test_gpu_matern.py; the shapes and edges of the evaluators are in tests/test_gpu_periodic_shapes.py).

  a  adaptive / identity nugget: the diagonal and host_ratios to 4e-15 relative, against tests/_periodic_reference.py
  b  rejections: id 16 with every bad parameter set gives -9001 from all six calls with `periods` in gpk_last_error; id 16 gives -9001
     from the bc, op, hess, 3-D and op3d evaluators; the host layer raises ValueError for those classes
  c  the class API end to end -- elliptic 150 / 40 with L = (1, 0), Burgers 120 / 42 with L = (0, 2), Eikonal 120 / 40 with L = (1, 0):
     loss history against a float64 numpy Gauss-Newton on the reference Theta (rtol 1e-6), a finite PDE residual, the posterior variance
     inside R.MARGIN x the numpy error; for the elliptic case extend_sol and extend_derivatives at 20 points on x1 = 0 and the same
     points on x1 = 1 agree within 64 eps max|.| -- the property no other kernel has
  d  main_NonLinElliptic2d.py --kernel periodic_Gaussian --period 1 0 prints its kernel line and finite test errors

Every figure is printed under a [periodic] tag before it is asserted.

RESULTS
  A run on an MI355X (gfx950), every test of this file passing:
    loss history against numpy, worst relative difference: Burgers 1.0e-9, Eikonal 1.6e-9, Nonlinear_elliptic 2.6e-10
    posterior variance, device error / allowed: Burgers 2.5e-11 / 5.4e-10, Eikonal 4.6e-11 / 1.8e-9, Nonlinear_elliptic 1.7e-12 / 1.3e-10
    Nonlinear_elliptic u, d1, d2, laplacian on x1 = 0 against x1 = 1: 0 eps each (max 1.99, 6.29, 25, 625)
    elliptic driver, sigma 0.2, L (1, 0), 150 / 40: test errors (max, L2) 0.118, 0.0231
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import _gn_reference as R
import _periodic_reference as PR
import _posterior_reference as PO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'nonlinpdes-gpsolver_amd')
if PKG not in sys.path:
    sys.path.insert(0, PKG)

LD = PR.LD
KERNEL = 'periodic_Gaussian'
LAYOUTS = ('Nonlinear_elliptic', 'Burgers', 'Eikonal', 'Darcy_u', 'Darcy_a')


@pytest.fixture(scope='module')
def ctx():
    import gpk
    c = gpk.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ a. nugget
@pytest.mark.parametrize('param', PR.PARAMS)
@pytest.mark.parametrize('layout', LAYOUTS)
def test_nugget_diagonal_and_ratios(ctx, layout, param):
    Nd, Nb = 65, 41
    Xd, Xb, _ = PR.points(Nd, Nb, param)
    diag = np.concatenate([np.full(n, v) for (_, n), v in zip(PR.offsets(layout, Nd, Nb), PR.diagonal_values(param, layout))])
    want_r = np.asarray(PR.trace_ratios(param, layout, Nd, Nb), dtype=np.float64)
    for nugget_type in ('adaptive', 'identity'):
        dT, ratios = ctx.assemble(layout, KERNEL, param, Xd, Xb, 1e-3, nugget_type)
        got = np.diag(dT.download()).astype(LD)
        dT.free()
        np.testing.assert_allclose(ratios[:len(want_r)], want_r, rtol=4e-15)
        assert all(r == 0.0 for r in ratios[len(want_r):])
        nug = PR.block_nuggets(param, layout, Nd, Nb, 1e-3, nugget_type)
        for (o, n), v in zip(PR.offsets(layout, Nd, Nb), nug):
            want = diag[o:o + n] + v
            assert float(np.max(np.abs(got[o:o + n] - want) / np.abs(want))) <= 4e-15, (nugget_type, o)


# ------------------------------------------------------------------------------------------------ b. rejections
def _six_calls(ctx, lay, kid, kp):
    """return codes of the six calls of the reference layouts for the kernel id kid and host_kparams kp"""
    rng = np.random.RandomState(3)
    Nd, Nb, Nt = 8, 4, 5
    dXd, dXb, dXt = ctx.points(rng.uniform(0, 1, (Nd, 2))), ctx.points(rng.uniform(0, 1, (Nb, 2))), ctx.points(rng.uniform(0, 1, (Nt, 2)))
    N = 4 * Nd + Nb
    out, vec, co = ctx.empty(N, N), ctx.empty(5 * Nt), ctx.array(np.ones(N))
    kp = (C.c_double * 4)(*kp)
    lib, h = ctx.lib, ctx.h
    rc = [lib.gpk_assemble(h, lay, kid, kp, dXd.ptr, Nd, dXb.ptr, Nb, 0.0, 0, out.ptr, out.ld, None),
          lib.gpk_assemble_test(h, lay, kid, kp, dXt.ptr, Nt, dXd.ptr, Nd, dXb.ptr, Nb, out.ptr, out.ld),
          lib.gpk_assemble_cross(h, lay, kid, kp, dXt.ptr, Nt, dXd.ptr, Nd, dXb.ptr, Nb, out.ptr, out.ld),
          lib.gpk_assemble_prior(h, kid, kp, dXt.ptr, Nt, dXd.ptr, Nd, out.ptr, out.ld),
          lib.gpk_extend(h, lay, kid, kp, dXt.ptr, Nt, dXd.ptr, Nd, dXb.ptr, Nb, co.ptr, vec.ptr),
          lib.gpk_extend_functionals(h, lay, kid, kp, dXt.ptr, Nt, dXd.ptr, Nd, dXb.ptr, Nb, co.ptr, 31, vec.ptr, Nt)]
    ctx.synchronize()
    for a in (dXd, dXb, dXt, out, vec, co):
        a.free()
    return rc


BAD = ((0.0, 0.2, 1.0, 0.0), (0.2, -0.1, 1.0, 0.0), (float('nan'), 0.2, 1.0, 0.0), (0.2, float('inf'), 0.0, 1.0), (0.2, 0.2, -1.0, 0.0),
       (0.2, 0.2, 1.0, -0.5), (0.2, 0.2, float('nan'), 1.0), (0.2, 0.2, 1.0, float('inf')), (0.2, 0.2, 0.0, 0.0))


def test_bad_parameters_are_rejected_by_all_six_calls(ctx):
    for lay in (0, 1, 2, 3):
        for good in PR.PARAMS:
            assert _six_calls(ctx, lay, 16, good) == [0] * 6, (lay, good)
        for kp in BAD:
            assert _six_calls(ctx, lay, 16, kp) == [-9001] * 6, (lay, kp)
            assert b'periods' in ctx.lib.gpk_last_error(ctx.h), kp
        for kid in (2, 7, 11, 15, 17, -1, 99):
            assert _six_calls(ctx, lay, kid, PR.PARAMS[0]) == [-9001] * 6, (lay, kid)


def test_other_evaluators_reject_the_id(ctx):
    rng = np.random.RandomState(4)
    Nd, Nb, Nt = 8, 4, 5
    N = 4 * Nd + Nb
    out, vec, co = ctx.empty(N, N), ctx.empty(12 * Nt), ctx.array(np.ones(N))
    kp = (C.c_double * 4)(0.3, 0.3, 1.0, 0.0)
    ratio = C.c_double()
    lib, h = ctx.lib, ctx.h
    for dim in (2, 3):
        dXd, dXb, dXt = (ctx.points(rng.uniform(0, 1, (n, dim)), dim) for n in (Nd, Nb, Nt))
        gram = (lib.gpk_assemble_bc, lib.gpk_assemble_op) if dim == 2 else (lib.gpk_assemble3d, lib.gpk_assemble_op3d)
        ext = (lib.gpk_extend_functionals_bc, lib.gpk_extend_functionals_op) if dim == 2 else (lib.gpk_extend_functionals3d, lib.gpk_extend_functionals_op3d)
        for f in gram:
            extra = {'gpk_assemble_bc': (None,), 'gpk_assemble3d': ()}.get(f.__name__, (None, None))
            assert f(h, 16, kp, dXd.ptr, Nd, dXb.ptr, Nb, *extra, 0.0, 0, out.ptr, out.ld, C.byref(ratio)) == -9001, f.__name__
        for f in ext:
            extra = {'gpk_extend_functionals_bc': (None,), 'gpk_extend_functionals3d': ()}.get(f.__name__, (None, None))
            assert f(h, 16, kp, dXt.ptr, Nt, dXd.ptr, Nd, dXb.ptr, Nb, *extra, co.ptr, 1, vec.ptr, Nt) == -9001, f.__name__
        if dim == 2:
            assert lib.gpk_assemble_hess(h, 16, kp, dXd.ptr, Nd, dXb.ptr, Nb, 0.0, 0, out.ptr, out.ld, None) == -9001
            assert lib.gpk_extend_functionals_hess(h, 16, kp, dXt.ptr, Nt, dXd.ptr, Nd, dXb.ptr, Nb, co.ptr, 1, vec.ptr, Nt) == -9001
    ctx.synchronize()
    Xd, Xb = rng.uniform(0, 1, (Nd, 2)), rng.uniform(0, 1, (Nb, 2))
    for call in (lambda: ctx.assemble_bc(KERNEL, PR.PARAMS[0], Xd, Xb, np.ones((Nb, 3))), lambda: ctx.assemble_hess(KERNEL, PR.PARAMS[0], Xd, Xb),
                 lambda: ctx.assemble3d(KERNEL, PR.PARAMS[0], rng.uniform(0, 1, (Nd, 3)), rng.uniform(0, 1, (Nb, 3)))):
        with pytest.raises(ValueError, match='periodic_Gaussian'):
            call()


# ------------------------------------------------------------------------------------------------ c. end to end, class API
NT_F = 67
QUIET = ['--print_hist', '', '--show_figure', '']
REAL = {
    'Nonlinear_elliptic': ['--N_domain', '150', '--N_boundary', '40', '--kernel', KERNEL, '--kernel_parameter', '0.2', '0.2', '--period', '1', '0',
                           '--nugget', '1e-6', '--GNsteps', '4'],
    'Burgers': ['--N_domain', '120', '--N_boundary', '42', '--kernel', KERNEL, '--kernel_parameter', '0.3', '0.05', '--period', '0', '2',
                '--nugget', '1e-5', '--GNsteps', '4'],
    'Eikonal': ['--N_domain', '120', '--N_boundary', '40', '--kernel', KERNEL, '--kernel_parameter', '0.2', '0.2', '--period', '1', '0',
                '--nugget', '1e-6', '--GNsteps', '4'],
}


def _solve(name):
    from _driver_common import solve_forward
    if name == 'Nonlinear_elliptic':
        import main_NonLinElliptic2d as drv
        cfg = drv.parse(REAL[name] + QUIET)
        u, f = drv.manufactured_periodic((True, False), cfg.alpha, cfg.m)
        np.random.seed(0)
        s, _ = solve_forward(cfg, name, u, f, drv.UNIT_SQUARE, solve_kwargs={'method': 'elimination'}, verbose=False)
    elif name == 'Eikonal':
        import main_Eikonal2d as drv
        cfg = drv.parse(REAL[name] + QUIET)
        np.random.seed(0)
        s, _ = solve_forward(cfg, name, lambda x1, x2: 0, lambda x1, x2: 1, drv.UNIT_SQUARE, verbose=False)
    else:
        import main_Burgers1d as drv
        cfg = drv.parse(REAL[name] + QUIET)
        np.random.seed(0)
        s, _ = solve_forward(cfg, name, drv.initial_and_lateral, lambda x1, x2: 0, drv.SPACE_TIME, verbose=False)
    return s, cfg


def _numpy_gauss_newton(cs, L, z0, steps, step_size):
    """float64 Gauss-Newton on the factor L of the reference Theta (tests/test_gpu_matern.py): the loss history J(z_0) .. J(z_steps)"""
    from scipy.linalg import solve_triangular
    z = np.asarray(z0, dtype=np.float64).copy()
    hist = []
    for k in range(steps + 1):
        lin = R.linearise(cs, z)
        v = solve_triangular(L, lin.F.astype(np.float64), lower=True, check_finite=False)
        hist.append(float(v @ v))
        if k == steps:
            break
        P = solve_triangular(L, lin.dense(np.float64), lower=True, check_finite=False)
        d = np.linalg.lstsq(P, -v, rcond=None)[0]
        z = z + step_size * d
    return np.array(hist), z


@pytest.mark.parametrize('name', sorted(REAL))
def test_class_api_end_to_end(name):
    s, cfg = _solve(name)
    e = s.eqn
    Nd, Nb = e.N_domain, e.N_boundary
    param = tuple(cfg.kernel_parameter)
    assert len(param) == 4 and Nb == {'Nonlinear_elliptic': 40, 'Burgers': 42, 'Eikonal': 40}[name]
    axis = 0 if param[2] > 0 else 1
    lo, hi = np.asarray(e.domain, dtype=float).T
    assert not np.any((e.X_boundary[:, axis] == lo[axis]) | (e.X_boundary[:, axis] == hi[axis])), 'boundary points on a periodic face'
    T = PR.theta_nugget(param, name, e.X_domain, e.X_boundary, cfg.nugget, cfg.nugget_type).astype(np.float64)
    system = {'Nonlinear_elliptic': 'elliptic', 'Burgers': 'burgers', 'Eikonal': 'eikonal'}[name]
    p0, p1, _ = e._gn_params()
    cs = PO.RealCase(system, Nd, Nb, e.rhs_f, e.bdy_g, p0, p1, T)
    ld, f64 = cs.factors()
    hist, _ = _numpy_gauss_newton(cs, f64[id(T)], e.init_sol, cfg.GNsteps, cfg.step_size)
    got = np.asarray(e.loss_hist, dtype=np.float64)
    print(f'\n[periodic] {name} L {param[2:]} loss history: device {got}, numpy {hist}, worst rel. diff {float(np.max(np.abs(got - hist) / np.abs(hist))):.3g}')
    assert got.shape == hist.shape
    np.testing.assert_allclose(got, hist, rtol=1e-6)
    r = e.PDE_residual(e.X_domain)
    assert r.shape == (Nd,) and np.all(np.isfinite(r))
    print(f'[periodic] {name} PDE residual at the collocation points: max {float(np.max(np.abs(r))):.3g}')
    rng = np.random.RandomState(42)
    Xt = lo + (hi - lo) * rng.uniform(0, 1, (NT_F, 2))
    var = e.posterior_variance(Xt, nt_chunk=32)
    z = e._z_star[1]
    K = PR.theta_test(param, name, Xt, e.X_domain, e.X_boundary).astype(np.float64).T
    prepared = PO.prepare_ld(cs, z, ld)
    ref = PO.variance_ld(cs, z, K, 0, ld, prepared).var
    np64 = PO.variance_np64(cs, z, K, 0, f64).var
    err_np = float(np.max(np.abs(np64.astype(LD) - ref)))
    vmin = float(np.min(ref))
    err = float(np.max(np.abs(var.astype(LD) - ref)))
    print(f'[periodic] {name} posterior variance: numpy error {err_np:.3g}, min var {vmin:.3g}, max var {float(np.max(ref)):.3g}, '
          f'device {err:.3g}, allowed {R.MARGIN * err_np:.3g}')
    assert err_np < 1e-3 * vmin, 'precondition: the gate could hide a wrong result'
    assert err <= R.MARGIN * err_np
    if name == 'Nonlinear_elliptic':                                    # the solution and its derivatives close across the periodic faces
        x2 = np.random.RandomState(43).uniform(0, 1, 20)
        left, right = np.stack([np.zeros(20), x2], axis=1), np.stack([np.ones(20), x2], axis=1)
        e.extend_sol(left)
        ul = e.extended_sol.copy()
        e.extend_sol(right)
        ur = e.extended_sol.copy()
        gap = float(np.max(np.abs(ul - ur))) / float(np.max(np.abs(ul)))
        print(f'[periodic] {name} u(0, .) against u(1, .): {gap / PR.EPS:.3g} eps of max|u| = {float(np.max(np.abs(ul))):.3g}')
        assert gap <= 64 * PR.EPS
        dl, dr = e.extend_derivatives(left), e.extend_derivatives(right)
        for nm in dl:
            gap = float(np.max(np.abs(dl[nm] - dr[nm]))) / float(np.max(np.abs(dl[nm])))
            print(f'[periodic] {name} {nm}(0, .) against {nm}(1, .): {gap / PR.EPS:.3g} eps of max = {float(np.max(np.abs(dl[nm]))):.3g}')
            assert gap <= 64 * PR.EPS, nm


# ------------------------------------------------------------------------------------------------ d. driver
def test_elliptic_driver_with_the_periodic_kernel(capsys):
    import main_NonLinElliptic2d as drv
    np.random.seed(0)
    drv.main(['--kernel', KERNEL, '--kernel_parameter', '0.2', '0.2', '--period', '1', '0', '--N_domain', '150', '--N_boundary', '40',
              '--nugget', '1e-8', '--GNsteps', '4', '--show_figure', ''])
    out = capsys.readouterr().out
    assert '[Kernel] periodic_Gaussian' in out
    errs = [float(line.split()[-1]) for line in out.splitlines() if line.startswith('[Test error]')]
    print(f'\n[periodic] elliptic driver, sigma 0.2, L (1, 0), 150 / 40: test errors (max, L2) {errs}')
    assert len(errs) == 2 and all(np.isfinite(v) and v >= 0 for v in errs)
