"""The periodic kernel's evaluators at multi-workgroup shapes and at the edges of the kernel, against the long-double reference of
tests/_periodic_reference.py (modelled on tests/test_gpu_matern_shapes.py).

  a  gpk_assemble for every layout and the periods (0, L), (L, 0), (L_1, L_2) at (N_d, N_b) = (8, 4), (190, 37) (odd: 8-byte stores),
     (300, 40) (even: 16-byte stores; M = 340 > 256) and (480, 40) (M / 2 > 256: two workgroups along x in the two-point frame), on
     points with planted pairs along every periodic axis: d = 0, 1e-9, 1e-6, 1e-3, L / 2, L - 1e-3, the images x + L and x + 3 L.
     30 rows of every block (all rows at (8, 4)) are compared in all columns.  Gate per block: max|dev - ld| <= C eps max|block|,
     C = 32 r_np + 1 with r_np the float64 class of src/kernels.py on the same entries, which must itself stay below 8e-15 max|block|.
     Theta is exactly symmetric; 16-byte and 8-byte stores (gpk_tune(47, 0)) give the same bits; a repeat gives the same bits; the rows
     of a point and of its images agree within the gate.
  b  gpk_assemble_test, gpk_assemble_cross and gpk_assemble_prior at N_t = 2, 514, 515 with the same gate; cross is the transpose of the
     test rows bit for bit, the prior of a set with itself is exactly symmetric with unit diagonal
  c  a view between canaries stays untouched outside N x N and holds the bits of the aligned call
  d  kappa underflowing to a subnormal and to 0 along a periodic axis (sigma = L / 90: most of a block is 0 there, so the gate is taken
     relative to the Cauchy-Schwarz bound sqrt(<f_i, f_i>(0) <f_j, f_j>(0)) of the block's entries, not to max|block|)
  e  gpk_extend and the five functionals within C = 32 r_np + 1 eps of (|rows| @ |coeff|)_t; all 31 masks against their single-bit calls
     bit for bit

Every figure is printed under a [periodic] tag before it is asserted.

RESULTS
  A run on an MI355X (gfx950), every test of this file passing (16 s with tests/test_gpu_periodic.py).  Worst device error over the sizes
  and periods in eps of max|block| / the C allowed there, then the worst extension ratio in eps (|rows| @ |coeff|)_t / its C:
    Nonlinear_elliptic   Gram 15.9 / 455    extension 2.66 / 92.8
    Burgers              Gram 10.3 / 329    extension 0.78 / 26.0
    Eikonal              Gram 7.34 / 220    extension 1.14 / 49.1
    Darcy_a              Gram 7.77 / 250    extension 0.725 / 30.0
  Underflow cases: device 31.8 eps of the Cauchy-Schwarz scale (the numpy class's own figure), C = 1020; subnormal entries 2.6e-303,
  -9.5e-310, 1.7e-314, and exact zeros beyond.
"""
import functools
import os
import sys

import numpy as np
import pytest

import _periodic_reference as PR
import _view_arena as VA

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'nonlinpdes-gpsolver_amd')
if PKG not in sys.path:
    sys.path.insert(0, PKG)

LD = PR.LD
KERNEL = 'periodic_Gaussian'
LAYOUTS = ('Nonlinear_elliptic', 'Burgers', 'Eikonal', 'Darcy_a')      # the four layout ids (Darcy_u is the Eikonal id)


@pytest.fixture(scope='module')
def ctx():
    import gpk
    c = gpk.Context(0)
    yield c
    c.close()


def _subset(layout, Nd, Nb):
    if Nd < 64:
        return [o + np.arange(n) for o, n in PR.offsets(layout, Nd, Nb)]
    return PR.row_subset(layout, Nd, Nb)


@functools.lru_cache(maxsize=None)
def _reference(layout, param, Nd, Nb):
    """(rows of the subset in long double, the same from the numpy class, the subset, row blocks of the stacked subset)"""
    Xd, Xb, _ = PR.points(Nd, Nb, param)
    subset = _subset(layout, Nd, Nb)
    ref = PR.subset_rows_reference(param, layout, Xd, Xb, subset)
    npv = PR.subset_rows_reference(param, layout, Xd, Xb, subset, evaluate=lambda fx, P: PR.np_rows(param, layout, fx, P, Xd, Xb))
    rb, o = [], 0
    for idx in subset:
        rb.append((o, len(idx))); o += len(idx)
    return ref, npv, subset, rb


# ------------------------------------------------------------------------------------------------ a. Gram matrix
@pytest.mark.parametrize('param', PR.PARAMS)
@pytest.mark.parametrize('layout', LAYOUTS)
def test_gram_at_every_size(ctx, layout, param):
    for Nd, Nb in PR.SIZES:
        Xd, Xb, _ = PR.points(Nd, Nb, param)
        ref, npv, subset, rb = _reference(layout, param, Nd, Nb)
        blocks = PR.offsets(layout, Nd, Nb)
        dT, _ = ctx.assemble(layout, KERNEL, param, Xd, Xb)
        got = dT.download()
        dT.free()
        assert np.all(np.isfinite(got))
        w = PR.block_gate('assemble', got[np.concatenate(subset)], ref, npv, rb, blocks)
        print(f'\n[periodic] assemble {layout} L {param[2:]} ({Nd}, {Nb}): device {w[0]:.3g} eps, allowed C = {w[1]:.3g}')
        assert np.array_equal(VA.bits(got), VA.bits(got.T.copy())), 'Theta is not exactly symmetric'
        dT2, _ = ctx.assemble(layout, KERNEL, param, Xd, Xb)
        assert np.array_equal(VA.bits(dT2.download()), VA.bits(got)), 'a repeat gives other bits'
        dT2.free()
        try:
            ctx.tune(47, 0)                                             # the one-point kernel, 8-byte stores
            dT3, _ = ctx.assemble(layout, KERNEL, param, Xd, Xb)
        finally:
            ctx.tune(47, 1)
        assert np.array_equal(VA.bits(dT3.download()), VA.bits(got)), 'wide and narrow stores give other bits'
        dT3.free()
        if Nd > max(PR.IMAGE_ROWS):                                     # a point and its images x + L, x + 3 L: the same rows
            for (o, n), (ro, rn) in zip(blocks, rb):
                src = got[o + PR.IMAGE_ROWS[0]]
                for k in PR.IMAGE_ROWS[1:]:
                    for co, cn in blocks:
                        scale = float(np.max(np.abs(ref[ro:ro + rn, co:co + cn])))
                        diff = float(np.max(np.abs(got[o + k, co:co + cn] - src[co:co + cn])))
                        assert diff <= w[1] * PR.EPS * scale, ('image', layout, (o, co), k, diff / PR.EPS / scale, w[1])


# ------------------------------------------------------------------------------------------------ b. test rows, cross columns, prior
@pytest.mark.parametrize('param', PR.PARAMS)
@pytest.mark.parametrize('layout', LAYOUTS)
def test_rows_cross_and_prior(ctx, layout, param):
    Nd, Nb = PR.SIZES[1]
    Xd, Xb, Xt = PR.points(Nd, Nb, param)
    blocks = PR.offsets(layout, Nd, Nb)
    Tt = PR.theta_test(param, layout, Xt, Xd, Xb)
    Ttn = PR.np_rows(param, layout, PR.ID, Xt, Xd, Xb)
    for Nt in PR.NTS:
        rows = [(0, Nt)]
        dt = ctx.assemble_test(layout, KERNEL, param, Xt[:Nt], Xd, Xb)
        gt = dt.download().reshape(Nt, -1)
        w = PR.block_gate('assemble_test', gt, Tt[:Nt], Ttn[:Nt], rows, blocks)
        dc = ctx.assemble_cross(layout, KERNEL, param, Xt[:Nt], Xd, Xb)
        gc = dc.download().reshape(-1, Nt)
        assert np.array_equal(VA.bits(gc.T.copy()), VA.bits(gt)), 'cross columns are not the transposed test rows'
        try:
            ctx.tune(47, 0)
            dn = ctx.assemble_cross(layout, KERNEL, param, Xt[:Nt], Xd, Xb)
        finally:
            ctx.tune(47, 1)
        assert np.array_equal(VA.bits(dn.download()), VA.bits(dc.download()))
        print(f'\n[periodic] test rows / cross columns {layout} L {param[2:]} Nt {Nt}: device {w[0]:.3g} eps, allowed C = {w[1]:.3g}')
        for a in (dt, dc, dn):
            a.free()
    if layout == LAYOUTS[0]:                                            # (no layout in the prior: once per parameter set)
        P = PR.prior(param, Xt, Xd)
        Pn = PR.np_rows(param, 'Darcy_a', PR.ID, Xt, Xd, Xb)[:, 2 * Nd:]
        for Nt in PR.NTS:
            dp = ctx.assemble_prior(KERNEL, param, Xt[:Nt], Xd)
            gp = dp.download().reshape(Nt, Nd)
            w = PR.block_gate('assemble_prior', gp, P[:Nt], Pn[:Nt], [(0, Nt)], [(0, Nd)])
            ds = ctx.assemble_prior(KERNEL, param, Xt[:Nt])
            gs = ds.download().reshape(Nt, Nt)
            assert np.array_equal(VA.bits(gs), VA.bits(gs.T.copy())) and np.all(np.diag(gs) == 1.0)
            print(f'[periodic] prior L {param[2:]} Nt {Nt}: device {w[0]:.3g} eps, allowed C = {w[1]:.3g}')
            dp.free(); ds.free()


# ------------------------------------------------------------------------------------------------ c. views
@pytest.mark.parametrize('layout', LAYOUTS)
def test_assemble_on_an_unaligned_view(ctx, layout):
    import gpk
    Nd, Nb = 64, 36
    param = PR.PARAMS[2]
    Xd, Xb, _ = PR.points(Nd, Nb, param)
    aligned, _ = ctx.assemble(layout, KERNEL, param, Xd, Xb, 1e-6, 'adaptive')          # (16-byte stores)
    N = aligned.rows
    v = VA.class_view(ctx, N, N, 'D')                                  # odd base offset, odd ld: the one-point kernel
    dXd, dXb = ctx.points(Xd), ctx.points(Xb)
    ctx._chk(ctx.lib.gpk_assemble(ctx.h, gpk.LAYOUT[layout], gpk.KERNEL[KERNEL], gpk.device.kernel_params(KERNEL, param), dXd.ptr, Nd,
                                  dXb.ptr, Nb, 1e-6, gpk.NUGGET['adaptive'], v.ptr, v.ld, None))
    ctx.synchronize()
    v.arena.assert_outside_untouched([v])
    assert np.array_equal(VA.bits(v.arena.get(v)), VA.bits(aligned.download()))
    v.arena.free(); aligned.free()


# ------------------------------------------------------------------------------------------------ d. underflow
@pytest.mark.parametrize('axis', [0, 1])
def test_kappa_underflows_to_subnormal_and_to_zero(ctx, axis):
    param, Xd, Xb, Xt = PR.far_case(axis)
    Nd, Nb = len(Xd), len(Xb)
    for layout in LAYOUTS:
        blocks = PR.offsets(layout, Nd, Nb)
        T = PR.theta(param, layout, Xd, Xb)
        Tn = np.concatenate([PR.np_rows(param, layout, f, P, Xd, Xb) for f, P in PR.MR._points(layout, Xd, Xb)], axis=0)
        dT, _ = ctx.assemble(layout, KERNEL, param, Xd, Xb)
        got = dT.download()
        dT.free()
        assert np.all(np.isfinite(got))
        w = PR.block_gate('far', got, T, Tn, blocks, blocks, scales=PR.natural_scales(param, layout))
        tiny = float(np.finfo(np.float64).tiny)
        for o, n in blocks:
            for co, cn in blocks:
                scale = float(np.max(np.abs(T[o:o + n, co:co + cn])))
                assert abs(got[o, co + 1]) <= 1e-290 * scale and got[o, co + 2] == 0.0, (layout, o, co, got[o, co + 1], got[o, co + 2])
        dt = ctx.assemble_test(layout, KERNEL, param, Xt, Xd, Xb)
        gt = dt.download().reshape(len(Xt), -1)
        dt.free()
        assert np.all(np.isfinite(gt))
        PR.block_gate('far rows', gt, PR.theta_test(param, layout, Xt, Xd, Xb), PR.np_rows(param, layout, PR.ID, Xt, Xd, Xb),
                      [(0, len(Xt))], blocks, scales=PR.natural_scales(param, layout, row_values=True))
        print(f'\n[periodic] underflow axis {axis + 1} {layout}: device {w[0]:.3g} eps, allowed C = {w[1]:.3g}, subnormal entry {got[0, 1]:.3g} '
              f'(tiny {tiny:.3g})')


# ------------------------------------------------------------------------------------------------ e. extension
@pytest.mark.parametrize('param', PR.PARAMS)
@pytest.mark.parametrize('layout', LAYOUTS)
def test_extension_and_all_masks(ctx, layout, param):
    import gpk
    Nd, Nb = PR.SIZES[1]
    Xd, Xb, Xt = PR.points(Nd, Nb, param)
    Nt = 9                                                              # (not a multiple of the 4 test points of a workgroup)
    Xt = Xt[:Nt]
    names = list(PR.FUNCTIONALS)
    N = sum(n for _, n in PR.offsets(layout, Nd, Nb))
    coeff = np.random.RandomState(N).normal(size=N)
    rows = {nm: PR.rows(param, layout, PR.FUNCTIONALS[nm], Xt, Xd, Xb) for nm in names}
    npval = {nm: PR.np_rows(param, layout, PR.FUNCTIONALS[nm], Xt, Xd, Xb) @ coeff for nm in names}
    got = ctx.extend(layout, KERNEL, param, Xt, Xd, Xb, coeff).download()
    gate = PR.ExtensionGate(got, npval['value'], rows['value'], coeff)
    print(f'\n[periodic] extend {layout} L {param[2:]}: device {gate.device:.3g} eps, r_np {gate.r_np:.3g}, allowed C = {gate.allowed:.3g}')
    gate.check('extend')
    again = ctx.extend(layout, KERNEL, param, Xt, Xd, Xb, coeff).download()
    assert np.array_equal(VA.bits(again), VA.bits(got))
    single = {}
    for nm in names:
        out = ctx.extend_functionals(layout, KERNEL, param, Xt, Xd, Xb, coeff, which=(nm,)).download().reshape(1, Nt)
        single[nm] = out[0].copy()
        gate = PR.ExtensionGate(out[0], npval[nm], rows[nm], coeff)
        print(f'[periodic] extend_functionals {layout} L {param[2:]} {nm}: device {gate.device:.3g} eps, r_np {gate.r_np:.3g}, '
              f'allowed C = {gate.allowed:.3g}')
        gate.check(nm)
    for mask in range(1, 32):
        which = tuple(nm for nm in names if mask & gpk.device.FUNCTIONAL[nm])
        out = ctx.extend_functionals(layout, KERNEL, param, Xt, Xd, Xb, coeff, which=which).download().reshape(len(which), Nt)
        for k, nm in enumerate(which):
            assert np.array_equal(VA.bits(out[k].copy()), VA.bits(single[nm])), (mask, nm)
