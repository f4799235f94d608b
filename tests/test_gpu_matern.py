"""Matern kernels (nu = 5/2, 7/2, 9/2) on the device, against the long-double reference of tests/_matern_reference.py.

  a  gpk_assemble, gpk_assemble_test, gpk_assemble_cross: every layout x nu, rho = 0.3 and (0.3, 0.07), (Nd, Nb) = (64, 36) (two-point
     kernel, 16-byte stores) and (65, 41) (one-point kernel), Nt in {1, 67, 300} with three collocation points among the test points.
     Gate per block: |device - ref| <= (4e-15 + 4 e_np) max|block|.  4e-15 is the project's Gram-block bound; e_np is the error of the
     numpy class of src/kernels.py against the same reference on the same points, scaled the same way and measured here; the factor 4
     allows for contraction and for the device's exp / sqrt against glibc's.
  b  the 8-byte store path (gpk_tune(47, 0)) against the 16-byte one, and an unaligned view between canaries: the same bits
  c  adaptive / identity nugget: diagonal and trace ratios
  d  gpk_extend, gpk_extend_functionals (masks 1, 21, 31) against reference rows @ coeff, bound 1e-12 max(|rows| @ |coeff|) as in
     tests/test_gpu_parity.py; a test point equal to a collocation point; a repeat gives the same bits
  e  rejections: ids 2..7 and 11, rho <= 0 / not finite, the Matern ids on the 3-D / bc / op / op3d entries
  f  the class API end to end at the sizes of REAL in tests/test_gpu_posterior.py: loss history against a float64 numpy Gauss-Newton on
     the reference Theta (rtol 1e-6), PDE_residual, posterior_variance with the gate of tests/test_gpu_posterior.py
  g  the Eikonal driver with --kernel Matern52

Every figure is printed under a [matern] tag.

RESULTS
  A run on an MI355X (gfx950), every test of this file passing: 550 [matern] lines.  Of the parity and extension lines the worst
  (device error over what is allowed) per nu and kind, then the end-to-end and driver lines in full:
    [matern] assemble Burgers Matern52 rho 0.3 (65, 41): device 5.97e-16, e_np 4.62e-16, allowed 5.85e-15
    [matern] test rows / cross columns Burgers Matern52 rho 0.3 (65, 41) Nt 67: device 7.73e-16 / 7.73e-16, e_np 7.73e-16, allowed 7.09e-15
    [matern] extend Nonlinear_elliptic Matern52 rho (0.3, 0.07): device 3.8e-13, allowed 1.54e-09
    [matern] extend_functionals Burgers Matern52 rho (0.3, 0.07) mask 31 d2d2: device 1e-09, allowed 2.3e-06
    [matern] assemble Burgers Matern72 rho 0.3 (64, 36): device 6.71e-16, e_np 5.49e-16, allowed 6.2e-15
    [matern] test rows / cross columns Burgers Matern72 rho (0.3, 0.07) (64, 36) Nt 67: device 5.83e-16 / 5.83e-16, e_np 4.21e-16, allowed 5.68e-15
    [matern] extend Eikonal Matern72 rho (0.3, 0.07): device 4.1e-13, allowed 1.63e-09
    [matern] extend_functionals Nonlinear_elliptic Matern72 rho (0.3, 0.07) mask 31 d2d2: device 4.44e-10, allowed 1.49e-06
    [matern] assemble Burgers Matern92 rho 0.3 (65, 41): device 8.42e-16, e_np 6.12e-16, allowed 6.45e-15
    [matern] test rows / cross columns Burgers Matern92 rho 0.3 (65, 41) Nt 300: device 6.48e-16 / 6.48e-16, e_np 4.91e-16, allowed 5.96e-15
    [matern] extend Eikonal Matern92 rho (0.3, 0.07): device 3.88e-13, allowed 1.62e-09
    [matern] extend_functionals Eikonal Matern92 rho (0.3, 0.07) mask 21 laplacian: device 4.48e-10, allowed 1.28e-06
    [matern] Burgers Matern52 loss history: device [1.61860537e+05 2.24129744e+02 5.15620828e+00 4.83737699e+00 4.83737677e+00], numpy [1.61860537e+05 2.24129744e+02 5.15620828e+00 4.83737699e+00 4.83737677e+00], worst rel. diff 2.86e-11
    [matern] Burgers Matern52 PDE residual at the collocation points: max 7.23e-05
    [matern] Burgers Matern52 posterior variance: numpy error 3.5e-12, min var 0.0689, max var 0.987, device 2.68e-12, allowed 1.12e-10
    [matern] Eikonal Matern72 loss history: device [3.26605422e+02 2.28449694e+03 7.24852739e+01 9.71705911e-01 5.63413268e-01], numpy [3.26605422e+02 2.28449694e+03 7.24852739e+01 9.71705911e-01 5.63413268e-01], worst rel. diff 5.88e-10
    [matern] Eikonal Matern72 PDE residual at the collocation points: max 3.36e-06
    [matern] Eikonal Matern72 posterior variance: numpy error 4.24e-13, min var 1.03e-05, max var 0.0523, device 2.82e-13, allowed 1.36e-11
    [matern] Nonlinear_elliptic Matern72 loss history: device [1.86137707e+07 3.85564531e+03 3.62751529e+03 3.62553259e+03 3.62549980e+03], numpy [1.86137707e+07 3.85564531e+03 3.62751529e+03 3.62553259e+03 3.62549980e+03], worst rel. diff 1.35e-10
    [matern] Nonlinear_elliptic Matern72 PDE residual at the collocation points: max 0.00258
    [matern] Nonlinear_elliptic Matern72 posterior variance: numpy error 1.55e-13, min var 6.43e-05, max var 0.069, device 3.08e-13, allowed 4.95e-12
    [matern] Eikonal driver, Matern52 rho 0.3, 120 / 40: test errors (max, L2) [0.022422004659072597, 0.009290067307137946]
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import _gn_reference as R
import _matern_reference as MR
import _posterior_reference as PR
import _view_arena as VA

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'nonlinpdes-gpsolver_amd')
if PKG not in sys.path:
    sys.path.insert(0, PKG)

LD = MR.LD
LAYOUTS = ('Nonlinear_elliptic', 'Burgers', 'Eikonal', 'Darcy_u', 'Darcy_a')
KERNELS = ('Matern52', 'Matern72', 'Matern92')
RHOS = (0.3, (0.3, 0.07))
SIZES = ((64, 36), (65, 41))
NTS = (1, 67, 300)
SPEC = {'Darcy_u': 'Eikonal'}                      # (the same layout id: one reference serves both names)


@pytest.fixture(scope='module')
def ctx():
    import gpk
    c = gpk.Context(0)
    yield c
    c.close()


def _points(Nd, Nb):
    rng = np.random.RandomState(100 * Nd + Nb)
    Xd, Xb = rng.uniform(0, 1, (Nd, 2)), rng.uniform(0, 1, (Nb, 2))
    Xt = rng.uniform(0, 1, (max(NTS), 2))
    Xt[0], Xt[5], Xt[66] = Xd[3], Xb[2], Xd[Nd - 1]                    # three collocation points verbatim (the first: Nt = 1 has one)
    return Xd, Xb, Xt


def _np_rows(kernel, rho, layout, fx, Xt, Xd, Xb):
    """the numpy class of src/kernels.py on the entries of MR.rows"""
    from src.kernels import Matern_kernel
    k = Matern_kernel({'Matern52': 2.5, 'Matern72': 3.5, 'Matern92': 4.5}[kernel])
    Xt = np.asarray(Xt, dtype=np.float64).reshape(-1, 2)
    return np.concatenate([k._eval(fx, f, Xt[:, None, 0], Xt[:, None, 1], P[None, :, 0], P[None, :, 1], rho)
                           for f, P in MR._points(layout, Xd, Xb)], axis=1)


@functools.lru_cache(maxsize=None)
def _reference(layout, kernel, rho, Nd, Nb):
    """(Theta, Theta_test at all test points) in long double and from the numpy class, shared by the tests of one case"""
    Xd, Xb, Xt = _points(Nd, Nb)
    T = MR.theta(kernel, rho, layout, Xd, Xb)
    Tt = MR.theta_test(kernel, rho, layout, Xt, Xd, Xb)
    Tn = np.concatenate([_np_rows(kernel, rho, layout, f, P, Xd, Xb) for f, P in MR._points(layout, Xd, Xb)], axis=0)
    Ttn = _np_rows(kernel, rho, layout, MR.ID, Xt, Xd, Xb)
    return T, Tt, Tn, Ttn


def _gate_blocks(what, got, ref, npv, row_blocks, col_blocks):
    """per block: |device - ref| <= (4e-15 + 4 e_np) max|block|; returns the worst (device, e_np) in units of max|block|"""
    worst = (0.0, 0.0)
    for ro, rn in row_blocks:
        for co, cn in col_blocks:
            r = ref[ro:ro + rn, co:co + cn]
            scale = float(np.max(np.abs(r)))
            e_dev = float(np.max(np.abs(got[ro:ro + rn, co:co + cn].astype(LD) - r))) / scale
            e_np = float(np.max(np.abs(npv[ro:ro + rn, co:co + cn].astype(LD) - r))) / scale
            if e_dev / (4e-15 + 4 * e_np) >= worst[0] / (4e-15 + 4 * worst[1]):
                worst = (e_dev, e_np)
            assert e_dev <= 4e-15 + 4 * e_np, (what, (ro, co), e_dev, e_np)
    return worst


# ------------------------------------------------------------------------------------------------ a. parity
@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('layout', LAYOUTS)
def test_gram_test_rows_and_cross_columns(ctx, layout, kernel):
    for rho in RHOS:
        for Nd, Nb in SIZES:
            Xd, Xb, Xt = _points(Nd, Nb)
            T, Tt, Tn, Ttn = _reference(SPEC.get(layout, layout), kernel, rho, Nd, Nb)
            blocks = MR.offsets(layout, Nd, Nb)
            dT, _ = ctx.assemble(layout, kernel, rho, Xd, Xb)
            got = dT.download()
            assert np.all(np.isfinite(got))
            w = _gate_blocks('assemble', got, T, Tn, blocks, blocks)
            print(f'\n[matern] assemble {layout} {kernel} rho {rho} ({Nd}, {Nb}): device {w[0]:.3g}, e_np {w[1]:.3g}, allowed {4e-15 + 4 * w[1]:.3g}')
            dT.free()
            for Nt in NTS:
                rows = [(0, Nt)]
                dt = ctx.assemble_test(layout, kernel, rho, Xt[:Nt], Xd, Xb)
                gt = dt.download().reshape(Nt, -1)
                w = _gate_blocks('assemble_test', gt, Tt[:Nt], Ttn[:Nt], rows, blocks)
                dc = ctx.assemble_cross(layout, kernel, rho, Xt[:Nt], Xd, Xb)
                gc = dc.download().reshape(-1, Nt)
                wc = _gate_blocks('assemble_cross', gc.T, Tt[:Nt], Ttn[:Nt], rows, blocks)
                print(f'[matern] test rows / cross columns {layout} {kernel} rho {rho} ({Nd}, {Nb}) Nt {Nt}: device {w[0]:.3g} / {wc[0]:.3g}, '
                      f'e_np {w[1]:.3g}, allowed {4e-15 + 4 * w[1]:.3g}')
                dt.free(); dc.free()


# ------------------------------------------------------------------------------------------------ b. store paths, views
@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('layout', LAYOUTS)
def test_narrow_store_path_gives_the_bits_of_the_wide_one(ctx, layout, kernel):
    Nd, Nb = SIZES[0]
    Xd, Xb, Xt = _points(Nd, Nb)
    for rho in RHOS:
        wide, _ = ctx.assemble(layout, kernel, rho, Xd, Xb, 1e-6, 'adaptive')
        wide_c = ctx.assemble_cross(layout, kernel, rho, Xt, Xd, Xb)
        try:
            ctx.tune(47, 0)
            narrow, _ = ctx.assemble(layout, kernel, rho, Xd, Xb, 1e-6, 'adaptive')
            narrow_c = ctx.assemble_cross(layout, kernel, rho, Xt, Xd, Xb)
        finally:
            ctx.tune(47, 1)
        assert np.array_equal(VA.bits(narrow.download()), VA.bits(wide.download()))
        assert np.array_equal(VA.bits(narrow_c.download()), VA.bits(wide_c.download()))
        for a in (wide, wide_c, narrow, narrow_c):
            a.free()


@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('layout', LAYOUTS)
def test_assemble_on_an_unaligned_view(ctx, layout, kernel):
    import gpk
    Nd, Nb = SIZES[0]
    Xd, Xb, _ = _points(Nd, Nb)
    rho = RHOS[1]
    aligned, _ = ctx.assemble(layout, kernel, rho, Xd, Xb, 1e-6, 'adaptive')          # (16-byte stores)
    N = aligned.rows
    v = VA.class_view(ctx, N, N, 'D')                                  # odd base offset, odd ld: the one-point kernel
    dXd, dXb = ctx.points(Xd), ctx.points(Xb)
    ctx._chk(ctx.lib.gpk_assemble(ctx.h, gpk.LAYOUT[layout], gpk.KERNEL[kernel], gpk.device.kernel_params(kernel, rho), dXd.ptr, Nd,
                                  dXb.ptr, Nb, 1e-6, gpk.NUGGET['adaptive'], v.ptr, v.ld, None))
    ctx.synchronize()
    v.arena.assert_outside_untouched([v])
    assert np.array_equal(VA.bits(v.arena.get(v)), VA.bits(aligned.download()))
    v.arena.free(); aligned.free()


# ------------------------------------------------------------------------------------------------ c. nugget
@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('layout', LAYOUTS)
def test_nugget_diagonal_and_ratios(ctx, layout, kernel):
    Nd, Nb = SIZES[1]
    Xd, Xb, _ = _points(Nd, Nb)
    for rho in RHOS:
        T = _reference(SPEC.get(layout, layout), kernel, rho, Nd, Nb)[0]
        blocks = MR.offsets(layout, Nd, Nb)
        want_r = np.asarray(MR.trace_ratios(kernel, rho, layout, Nd, Nb), dtype=np.float64)
        for nugget_type in ('adaptive', 'identity'):
            dT, ratios = ctx.assemble(layout, kernel, rho, Xd, Xb, 1e-3, nugget_type)
            got = np.diag(dT.download()).astype(LD)
            dT.free()
            np.testing.assert_allclose(ratios[:len(want_r)], want_r, rtol=1e-14)
            assert all(r == 0.0 for r in ratios[len(want_r):])
            nug = MR.block_nuggets(kernel, rho, layout, Nd, Nb, 1e-3, nugget_type)
            for (o, n), v in zip(blocks, nug):
                want = np.diag(T)[o:o + n] + v
                assert float(np.max(np.abs(got[o:o + n] - want))) <= 4e-15 * float(np.max(np.abs(want))), (nugget_type, o)


# ------------------------------------------------------------------------------------------------ d. extension
MASKS = (1, 21, 31)


@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('layout', LAYOUTS)
def test_extension(ctx, layout, kernel):
    import gpk
    Nd, Nb = SIZES[1]
    Xd, Xb, Xt = _points(Nd, Nb)
    Nt = 67
    Xt = Xt[:Nt]                                                        # (holds collocation points: Xt[0], Xt[5], Xt[66])
    names = list(MR.FUNCTIONALS)
    for rho in RHOS:
        N = sum(n for _, n in MR.offsets(layout, Nd, Nb))
        coeff = np.random.RandomState(N).normal(size=N)
        rows = {nm: MR.rows(kernel, rho, SPEC.get(layout, layout), MR.FUNCTIONALS[nm], Xt, Xd, Xb) for nm in names}
        want = {nm: rows[nm] @ coeff.astype(LD) for nm in names}
        bound = {nm: 1e-12 * np.max(np.abs(rows[nm]) @ np.abs(coeff).astype(LD)) for nm in names}
        got = ctx.extend(layout, kernel, rho, Xt, Xd, Xb, coeff).download()
        err = float(np.max(np.abs(got.astype(LD) - want['value'])))
        print(f'\n[matern] extend {layout} {kernel} rho {rho}: device {err:.3g}, allowed {float(bound["value"]):.3g}')
        assert err <= bound['value']
        again = ctx.extend(layout, kernel, rho, Xt, Xd, Xb, coeff).download()
        assert np.array_equal(VA.bits(again), VA.bits(got))
        for mask in MASKS:
            which = tuple(nm for nm in names if mask & gpk.device.FUNCTIONAL[nm])
            out = ctx.extend_functionals(layout, kernel, rho, Xt, Xd, Xb, coeff, which=which).download().reshape(len(which), Nt)
            for k, nm in enumerate(which):
                err = float(np.max(np.abs(out[k].astype(LD) - want[nm])))
                print(f'[matern] extend_functionals {layout} {kernel} rho {rho} mask {mask} {nm}: device {err:.3g}, allowed {float(bound[nm]):.3g}')
                assert err <= bound[nm], (mask, nm)
            rep = ctx.extend_functionals(layout, kernel, rho, Xt, Xd, Xb, coeff, which=which).download().reshape(len(which), Nt)
            assert np.array_equal(VA.bits(rep), VA.bits(out))


# ------------------------------------------------------------------------------------------------ e. rejections
def _five_calls(ctx, lay, kid, kp):
    """return codes of the five calls of the reference layouts for the kernel id kid and host_kparams kp"""
    rng = np.random.RandomState(3)
    Nd, Nb, Nt = 8, 4, 5
    dXd, dXb, dXt = ctx.points(rng.uniform(0, 1, (Nd, 2))), ctx.points(rng.uniform(0, 1, (Nb, 2))), ctx.points(rng.uniform(0, 1, (Nt, 2)))
    N = 4 * Nd + Nb
    out, vec, co = ctx.empty(N, N), ctx.empty(5 * Nt), ctx.array(np.ones(N))
    kp = (C.c_double * 2)(*kp)
    lib, h = ctx.lib, ctx.h
    rc = [lib.gpk_assemble(h, lay, kid, kp, dXd.ptr, Nd, dXb.ptr, Nb, 0.0, 0, out.ptr, out.ld, None),
          lib.gpk_assemble_test(h, lay, kid, kp, dXt.ptr, Nt, dXd.ptr, Nd, dXb.ptr, Nb, out.ptr, out.ld),
          lib.gpk_extend(h, lay, kid, kp, dXt.ptr, Nt, dXd.ptr, Nd, dXb.ptr, Nb, co.ptr, vec.ptr),
          lib.gpk_extend_functionals(h, lay, kid, kp, dXt.ptr, Nt, dXd.ptr, Nd, dXb.ptr, Nb, co.ptr, 31, vec.ptr, Nt),
          lib.gpk_assemble_cross(h, lay, kid, kp, dXt.ptr, Nt, dXd.ptr, Nd, dXb.ptr, Nb, out.ptr, out.ld)]
    ctx.synchronize()
    for a in (dXd, dXb, dXt, out, vec, co):
        a.free()
    return rc


def test_invalid_kernel_ids_and_length_scales_are_rejected(ctx):
    for lay in (0, 1, 2, 3):
        for kid in (2, 3, 4, 5, 6, 7, 11, -1):
            assert _five_calls(ctx, lay, kid, (0.3, 0.3)) == [-9001] * 5, (lay, kid)
        for kid in (8, 9, 10):
            assert _five_calls(ctx, lay, kid, (0.3, 0.07)) == [0] * 5, (lay, kid)
            for kp in ((0.0, 0.3), (0.3, 0.0), (-0.3, 0.3), (0.3, -1.0), (float('nan'), 0.3), (0.3, float('inf'))):
                assert _five_calls(ctx, lay, kid, kp) == [-9001] * 5, (lay, kid, kp)
    assert b'length scales' in ctx.lib.gpk_last_error(ctx.h)


@pytest.mark.parametrize('kid', [8, 9, 10])
def test_matern_ids_are_rejected_by_the_other_evaluators(ctx, kid):
    rng = np.random.RandomState(4)
    Nd, Nb, Nt = 8, 4, 5
    N = 2 * Nd + Nb
    out, vec, co = ctx.empty(N, N), ctx.empty(12 * Nt), ctx.array(np.ones(N))
    kp = (C.c_double * 3)(0.3, 0.3, 0.3)
    ratio = C.c_double()
    lib, h = ctx.lib, ctx.h
    for dim in (2, 3):
        dXd, dXb, dXt = (ctx.points(rng.uniform(0, 1, (n, dim)), dim) for n in (Nd, Nb, Nt))
        gram = (lib.gpk_assemble_bc, lib.gpk_assemble_op) if dim == 2 else (lib.gpk_assemble3d, lib.gpk_assemble_op3d)
        ext = (lib.gpk_extend_functionals_bc, lib.gpk_extend_functionals_op) if dim == 2 else (lib.gpk_extend_functionals3d, lib.gpk_extend_functionals_op3d)
        for f in gram:
            extra = {'gpk_assemble_bc': (None,), 'gpk_assemble3d': ()}.get(f.__name__, (None, None))
            assert f(h, kid, kp, dXd.ptr, Nd, dXb.ptr, Nb, *extra, 0.0, 0, out.ptr, out.ld, C.byref(ratio)) == -9001, f.__name__
        for f in ext:
            extra = {'gpk_extend_functionals_bc': (None,), 'gpk_extend_functionals3d': ()}.get(f.__name__, (None, None))
            assert f(h, kid, kp, dXt.ptr, Nt, dXd.ptr, Nd, dXb.ptr, Nb, *extra, co.ptr, 1, vec.ptr, Nt) == -9001, f.__name__
    ctx.synchronize()


# ------------------------------------------------------------------------------------------------ f. end to end, class API
NT_F = 67
QUIET = ['--print_hist', '', '--show_figure', '']
REAL = {
    'Nonlinear_elliptic': ['--N_domain', '150', '--N_boundary', '40', '--kernel', 'Matern72', '--kernel_parameter', '0.3', '--nugget', '1e-6',
                           '--GNsteps', '4'],
    'Burgers': ['--N_domain', '120', '--N_boundary', '42', '--kernel', 'Matern52', '--kernel_parameter', '0.3', '0.05', '--nugget', '1e-5',
                '--GNsteps', '4'],
    'Eikonal': ['--N_domain', '120', '--N_boundary', '40', '--kernel', 'Matern72', '--kernel_parameter', '0.3', '--nugget', '1e-6',
                '--GNsteps', '4'],
}


def _solve(name):
    from _driver_common import solve_forward
    if name == 'Nonlinear_elliptic':
        import main_NonLinElliptic2d as drv
        cfg = drv.parse(REAL[name] + QUIET)
        u, f = drv.manufactured(cfg.alpha, cfg.m)
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
    """float64 Gauss-Newton on the factor L of the reference Theta: the loss history J(z_0) .. J(z_steps), J = F^T Theta^-1 F, each step
    the least-squares solution of L^-1 (F(z) + A(z) d) = 0 (the linearisation of tests/_gn_reference.py)"""
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
    T = MR.theta_nugget(cfg.kernel, cfg.kernel_parameter, name, e.X_domain, e.X_boundary, cfg.nugget, cfg.nugget_type).astype(np.float64)
    system = {'Nonlinear_elliptic': 'elliptic', 'Burgers': 'burgers', 'Eikonal': 'eikonal'}[name]
    p0, p1, _ = e._gn_params()
    cs = PR.RealCase(system, Nd, Nb, e.rhs_f, e.bdy_g, p0, p1, T)
    ld, f64 = cs.factors()
    # loss history
    hist, _ = _numpy_gauss_newton(cs, f64[id(T)], e.init_sol, cfg.GNsteps, cfg.step_size)
    got = np.asarray(e.loss_hist, dtype=np.float64)
    print(f'\n[matern] {name} {cfg.kernel} loss history: device {got}, numpy {hist}, worst rel. diff {float(np.max(np.abs(got - hist) / np.abs(hist))):.3g}')
    assert got.shape == hist.shape
    np.testing.assert_allclose(got, hist, rtol=1e-6)
    # residual at the collocation points
    r = e.PDE_residual(e.X_domain)
    assert r.shape == (Nd,) and np.all(np.isfinite(r))
    print(f'[matern] {name} {cfg.kernel} PDE residual at the collocation points: max {float(np.max(np.abs(r))):.3g}')
    # posterior variance: the gate of tests/test_gpu_posterior.py with K from the reference
    rng = np.random.RandomState(42)
    lo, hi = np.asarray(e.domain, dtype=float).T
    Xt = lo + (hi - lo) * rng.uniform(0, 1, (NT_F, 2))
    var = e.posterior_variance(Xt, nt_chunk=32)
    z = e._z_star[1]
    K = MR.theta_test(cfg.kernel, cfg.kernel_parameter, name, Xt, e.X_domain, e.X_boundary).astype(np.float64).T
    prepared = PR.prepare_ld(cs, z, ld)
    ref = PR.variance_ld(cs, z, K, 0, ld, prepared).var
    np64 = PR.variance_np64(cs, z, K, 0, f64).var
    err_np = float(np.max(np.abs(np64.astype(LD) - ref)))
    vmin = float(np.min(ref))
    err = float(np.max(np.abs(var.astype(LD) - ref)))
    print(f'[matern] {name} {cfg.kernel} posterior variance: numpy error {err_np:.3g}, min var {vmin:.3g}, max var {float(np.max(ref)):.3g}, '
          f'device {err:.3g}, allowed {R.MARGIN * err_np:.3g}')
    assert err_np < 1e-3 * vmin, 'precondition: the gate could hide a wrong result'
    assert err <= R.MARGIN * err_np


# ------------------------------------------------------------------------------------------------ g. driver
def test_eikonal_driver_with_a_matern_kernel(capsys):
    import main_Eikonal2d as drv
    np.random.seed(0)
    drv.main(['--kernel', 'Matern52', '--kernel_parameter', '0.3', '--N_domain', '120', '--N_boundary', '40', '--show_figure', ''])
    out = capsys.readouterr().out
    assert '[Kernel] Matern52' in out
    errs = [float(line.split()[-1]) for line in out.splitlines() if line.startswith('[Test error]')]
    print(f'\n[matern] Eikonal driver, Matern52 rho 0.3, 120 / 40: test errors (max, L2) {errs}')
    assert len(errs) == 2 and all(np.isfinite(v) and v >= 0 for v in errs)
