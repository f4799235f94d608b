"""Posterior variance on the device: gpk_assemble_cross, gpk_col_sumsq, gpk_posterior_prepare / gpk_posterior_variance and the class API.

  a  the cross-covariance evaluator against the transpose of gpk_assemble_test (bound of tests/test_gpu_parity.py for Theta_test), on
     an unaligned view between canaries, 16-byte against 8-byte stores bit for bit
  b  the column reduction against long double, judged by what np.sum(V * V, axis=0) achieves on the same data; repeatable to the bit
  c  prepare + variance on the synthetic, well-conditioned factors of tests/_gn_reference.py against long double, var_cond and var_gn
     separately, judged by the float64 numpy pipeline (tests/_posterior_reference.py) measured in the same test
  d  the class API on real Gram matrices against the long-double formula at the device's own final iterate and the oracle's Theta
  e  the surface: attributes, what is not served, the drivers' flag

Gates c and d are not constants: the device may take R.MARGIN = 32 times what the float64 numpy pipeline takes on the same inputs (plus
one eps in c), the project's factor for blocked / MFMA summation order against LAPACK.  Every figure is printed under a [posterior]
tag with the worst so far.

RESULTS
  The [posterior] lines of a run on an MI355X (gfx950), every test of this file passing:
    [posterior] col_sumsq 1 x 1: device 0.167, allowed 6.35; worst so far 0.167 of 6.35
    [posterior] col_sumsq 63 x 67: device 1.04, allowed 136; worst so far 0.167 of 6.35
    [posterior] col_sumsq 340 x 300: device 1.98, allowed 175; worst so far 0.167 of 6.35
    [posterior] col_sumsq 2049 x 65: device 3.93, allowed 653; worst so far 0.167 of 6.35
    [posterior] var_cond elliptic 65 field 0 dinv 256: device 0.27, allowed 10.6; worst so far 0.27 of 10.6
    [posterior] var_gn elliptic 65 field 0 dinv 256: device 8.53, allowed 104; worst so far 8.53 of 104
    [posterior] var_cond elliptic 65 field 0 dinv False: device 0.372, allowed 10.6; worst so far 0.372 of 10.6
    [posterior] var_gn elliptic 65 field 0 dinv False: device 9.33, allowed 104; worst so far 9.33 of 104
    [posterior] var_cond elliptic 129 field 0 dinv 256: device 0.295, allowed 10.2; worst so far 0.372 of 10.6
    [posterior] var_gn elliptic 129 field 0 dinv 256: device 6.68, allowed 72.5; worst so far 6.68 of 72.5
    [posterior] var_cond elliptic 129 field 0 dinv False: device 0.295, allowed 10.2; worst so far 0.372 of 10.6
    [posterior] var_gn elliptic 129 field 0 dinv False: device 7.17, allowed 72.5; worst so far 7.17 of 72.5
    [posterior] var_cond burgers 65 field 0 dinv 256: device 0.312, allowed 10.2; worst so far 0.372 of 10.6
    [posterior] var_gn burgers 65 field 0 dinv 256: device 5.02, allowed 65.7; worst so far 7.17 of 72.5
    [posterior] var_cond burgers 65 field 0 dinv False: device 0.37, allowed 10.2; worst so far 0.37 of 10.2
    [posterior] var_gn burgers 65 field 0 dinv False: device 4.94, allowed 65.7; worst so far 7.17 of 72.5
    [posterior] var_cond burgers 129 field 0 dinv 256: device 0.362, allowed 9.76; worst so far 0.362 of 9.76
    [posterior] var_gn burgers 129 field 0 dinv 256: device 6.23, allowed 51.3; worst so far 6.23 of 51.3
    [posterior] var_cond burgers 129 field 0 dinv False: device 0.336, allowed 9.76; worst so far 0.362 of 9.76
    [posterior] var_gn burgers 129 field 0 dinv False: device 5.4, allowed 51.3; worst so far 6.23 of 51.3
    [posterior] var_cond eikonal 65 field 0 dinv 256: device 0.281, allowed 10.5; worst so far 0.362 of 9.76
    [posterior] var_gn eikonal 65 field 0 dinv 256: device 167, allowed 4.15e+03; worst so far 6.23 of 51.3
    [posterior] var_cond eikonal 65 field 0 dinv False: device 0.326, allowed 10.5; worst so far 0.362 of 9.76
    [posterior] var_gn eikonal 65 field 0 dinv False: device 142, allowed 4.15e+03; worst so far 6.23 of 51.3
    [posterior] var_cond eikonal 129 field 0 dinv 256: device 0.306, allowed 10.1; worst so far 0.362 of 9.76
    [posterior] var_gn eikonal 129 field 0 dinv 256: device 86, allowed 3.64e+03; worst so far 6.23 of 51.3
    [posterior] var_cond eikonal 129 field 0 dinv False: device 0.306, allowed 10.1; worst so far 0.362 of 9.76
    [posterior] var_gn eikonal 129 field 0 dinv False: device 95.6, allowed 3.64e+03; worst so far 6.23 of 51.3
    [posterior] var_cond darcy 65 field 0 dinv 256: device 0.3, allowed 10.3; worst so far 0.362 of 9.76
    [posterior] var_gn darcy 65 field 0 dinv 256: device 6.44, allowed 70.6; worst so far 6.23 of 51.3
    [posterior] var_cond darcy 65 field 1 dinv 256: device 0.299, allowed 10.4; worst so far 0.362 of 9.76
    [posterior] var_gn darcy 65 field 1 dinv 256: device 6.17, allowed 71.7; worst so far 6.23 of 51.3
    [posterior] var_cond darcy 65 field 0 dinv False: device 0.416, allowed 10.3; worst so far 0.416 of 10.3
    [posterior] var_gn darcy 65 field 0 dinv False: device 6.67, allowed 70.6; worst so far 6.23 of 51.3
    [posterior] var_cond darcy 65 field 1 dinv False: device 0.318, allowed 10.4; worst so far 0.416 of 10.3
    [posterior] var_gn darcy 65 field 1 dinv False: device 6.28, allowed 71.7; worst so far 6.23 of 51.3
    [posterior] var_cond darcy 129 field 0 dinv 256: device 0.302, allowed 9.99; worst so far 0.416 of 10.3
    [posterior] var_gn darcy 129 field 0 dinv 256: device 7.15, allowed 47.7; worst so far 7.15 of 47.7
    [posterior] var_cond darcy 129 field 1 dinv 256: device 0.304, allowed 10.4; worst so far 0.416 of 10.3
    [posterior] var_gn darcy 129 field 1 dinv 256: device 6.54, allowed 82.1; worst so far 7.15 of 47.7
    [posterior] var_cond darcy 129 field 0 dinv False: device 0.302, allowed 9.99; worst so far 0.416 of 10.3
    [posterior] var_gn darcy 129 field 0 dinv False: device 7.15, allowed 47.7; worst so far 7.15 of 47.7
    [posterior] var_cond darcy 129 field 1 dinv False: device 0.312, allowed 10.4; worst so far 0.416 of 10.3
    [posterior] var_gn darcy 129 field 1 dinv False: device 6.47, allowed 82.1; worst so far 7.15 of 47.7
    [posterior] real Burgers: numpy error 1.56e-11, min var 0.052, max var 0.937
    [posterior] real Burgers nt_chunk 32: device 2.03e-11, allowed 5.01e-10; worst so far 2.03e-11 of 5.01e-10
    [posterior] real Burgers nt_chunk 1024: device 2.03e-11, allowed 5.01e-10; worst so far 2.03e-11 of 5.01e-10
    [posterior] real Darcy_flow2d_u: numpy error 4.23e-14, min var 3.77e-06, max var 0.00173
    [posterior] real Darcy_flow2d_u nt_chunk 32: device 2.06e-14, allowed 1.35e-12; worst so far 2.03e-11 of 5.01e-10
    [posterior] real Darcy_flow2d_u nt_chunk 1024: device 2.06e-14, allowed 1.35e-12; worst so far 2.03e-11 of 5.01e-10
    [posterior] real Darcy_flow2d_a: numpy error 6.41e-11, min var 0.144, max var 0.851
    [posterior] real Darcy_flow2d_a nt_chunk 32: device 1.16e-10, allowed 2.05e-09; worst so far 1.16e-10 of 2.05e-09
    [posterior] real Darcy_flow2d_a nt_chunk 1024: device 1.16e-10, allowed 2.05e-09; worst so far 1.16e-10 of 2.05e-09
    [posterior] real Eikonal: numpy error 7.06e-14, min var 5.96e-07, max var 0.00108
    [posterior] real Eikonal nt_chunk 32: device 1.11e-13, allowed 2.26e-12; worst so far 1.16e-10 of 2.05e-09
    [posterior] real Eikonal nt_chunk 1024: device 1.11e-13, allowed 2.26e-12; worst so far 1.16e-10 of 2.05e-09
    [posterior] real Nonlinear_elliptic: numpy error 6.73e-14, min var 5.36e-07, max var 0.000212
    [posterior] real Nonlinear_elliptic nt_chunk 32: device 1.21e-14, allowed 2.15e-12; worst so far 1.16e-10 of 2.05e-09
    [posterior] real Nonlinear_elliptic nt_chunk 1024: device 1.21e-14, allowed 2.15e-12; worst so far 1.16e-10 of 2.05e-09
"""
import functools
import os
import sys

import numpy as np
import pytest

import _gn_reference as R
import _posterior_reference as PR
import _view_arena as VA
from _gauss_reference import gate_blocks, offsets
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'nonlinpdes-gpsolver_amd')
if PKG not in sys.path:
    sys.path.insert(0, PKG)

LD, EPS = R.LD, R.EPS
WORST = {}


def _note(tag, ratio, allowed, what):
    w = WORST.setdefault(tag, (0.0, 0.0, allowed))
    if not ratio / allowed < w[0]:
        WORST[tag] = (ratio / allowed, ratio, allowed)
    print(f'[posterior] {tag} {what}: device {ratio:.3g}, allowed {allowed:.3g}; worst so far {WORST[tag][1]:.3g} of {WORST[tag][2]:.3g}')


# ------------------------------------------------------------------------------------------------ a. gpk_assemble_cross
LAYOUTS = ('Nonlinear_elliptic', 'Burgers', 'Eikonal', 'Darcy_u', 'Darcy_a')
KERNELS = (('Gaussian', 0.2), ('anisotropic_Gaussian', [0.3, 0.07]))


def _pts(rng, n):
    return rng.uniform(0, 1, (n, 2))


@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('kernel,kp', KERNELS)
def test_assemble_cross_is_the_transpose_of_assemble_test(dev_ctx, layout, kernel, kp):
    ctx = dev_ctx
    rng = np.random.RandomState(17)
    for Nd in (65, 129):
        for Nb in (36, 41):
            Xd, Xb = _pts(rng, Nd), _pts(rng, Nb)
            for Nt in (1, 67, 300):
                Xt = _pts(rng, Nt)
                want = ctx.assemble_test(layout, kernel, kp, Xt, Xd, Xb).download().T
                got = ctx.assemble_cross(layout, kernel, kp, Xt, Xd, Xb).download().reshape(-1, Nt)   # (one column downloads as a vector)
                assert got.shape == want.shape
                gate_blocks(got, want, None, offsets(layout, Nd, Nb), [(0, Nt)], (Nd, Nb, Nt))   # (per block: 4e-15 max|block|)
                try:                                                  # the 8-byte store path: the same bits
                    ctx.tune(47, 0)
                    narrow = ctx.assemble_cross(layout, kernel, kp, Xt, Xd, Xb).download().reshape(-1, Nt)
                finally:
                    ctx.tune(47, 1)
                assert np.array_equal(VA.bits(narrow), VA.bits(got)), (Nd, Nb, Nt)


@pytest.mark.parametrize('layout', LAYOUTS)
def test_assemble_cross_on_an_unaligned_view(dev_ctx, layout):
    import gpk
    ctx = dev_ctx
    rng = np.random.RandomState(23)
    Nd, Nb, Nt = 65, 41, 300
    Xd, Xb, Xt = _pts(rng, Nd), _pts(rng, Nb), _pts(rng, Nt)
    aligned = ctx.assemble_cross(layout, 'Gaussian', 0.2, Xt, Xd, Xb)      # (16-byte stores: aligned base, even ld, even Nt)
    N = aligned.rows
    v = VA.class_view(ctx, N, Nt, 'D')                                 # odd base offset, odd ld
    dXt, dXd, dXb = ctx.points(Xt), ctx.points(Xd), ctx.points(Xb)
    ctx._chk(ctx.lib.gpk_assemble_cross(ctx.h, gpk.LAYOUT[layout], 0, gpk.device.kernel_params('Gaussian', 0.2), dXt.ptr, Nt, dXd.ptr, Nd,
                                        dXb.ptr, Nb, v.ptr, v.ld))
    ctx.synchronize()
    v.arena.assert_outside_untouched([v])
    assert np.array_equal(VA.bits(v.arena.get(v)), VA.bits(aligned.download()))
    v.arena.free()


def test_assemble_cross_rejects_bad_arguments(dev_ctx):
    import gpk
    ctx = dev_ctx
    Xd, Xb, Xt = _pts(np.random.RandomState(1), 8), _pts(np.random.RandomState(2), 4), _pts(np.random.RandomState(3), 5)
    out = ctx.empty(20, 4)
    out.ld = 4                                                         # ld < Nt
    with pytest.raises(gpk.GpkError, match='ld < Nt'):
        ctx.assemble_cross('Nonlinear_elliptic', 'Gaussian', 0.2, Xt, Xd, Xb, out=out)


# ------------------------------------------------------------------------------------------------ b. gpk_col_sumsq
def _padded(ctx, A, pad, poison=R.POISON):
    rows, cols = A.shape
    full = np.full((rows, cols + pad), poison)
    full[:, :cols] = A
    d = ctx.empty(rows, cols + pad, ld=cols + pad)
    d.upload(full)
    d.cols = cols
    return d


@pytest.mark.parametrize('rows,cols', [(1, 1), (63, 67), (340, 300), (2049, 65)])
def test_col_sumsq(dev_ctx, rows, cols):
    import gpk
    ctx = dev_ctx
    rng = np.random.RandomState(rows * 7 + cols)
    V = 10.0 ** rng.uniform(-8, 3, (rows, cols)) * rng.choice([-1.0, 1.0], (rows, cols))
    base = rng.normal(size=cols) * 10.0 ** rng.uniform(-3, 6, cols)
    dV, db = _padded(ctx, V, 3), ctx.array(base)
    got = ctx.col_sumsq(dV, alpha=-1.0, base=db).download()
    ssq = np.sum(V.astype(LD) ** 2, axis=0)
    ref = base.astype(LD) - ssq
    scale = LD(EPS) * (np.abs(base).astype(LD) + ssq)
    ratio = lambda x: float(np.max(np.abs(np.asarray(x).astype(LD) - ref) / scale))
    allowed = R.allowed(ratio(base - np.sum(V * V, axis=0)))
    _note('col_sumsq', ratio(got), allowed, f'{rows} x {cols}')
    assert ratio(got) <= allowed                                       # (a leaked 1e30 of the padding would be 1e60 here)
    again = ctx.col_sumsq(dV, alpha=-1.0, base=db).download()
    assert np.array_equal(VA.bits(again), VA.bits(got))
    fresh = gpk.Context(0, dev=True)
    try:
        other = fresh.col_sumsq(_padded(fresh, V, 3), alpha=-1.0, base=fresh.array(base)).download()
    finally:
        fresh.close()
    assert np.array_equal(VA.bits(other), VA.bits(got))
    plain = ctx.col_sumsq(dV).download()                               # no base, alpha = 1
    assert float(np.max(np.abs(plain.astype(LD) - ssq) / (LD(EPS) * ssq))) <= allowed


# ------------------------------------------------------------------------------------------------ c. prepare + variance, synthetic factors
NT_C = 70


def _upload_factor(ctx, L):
    n = L.shape[0]
    d = ctx.empty(n, n + R.LD_PAD, ld=n + R.LD_PAD)
    d.upload(R.poisoned(L))
    d.cols = n
    return d


def _problem(ctx, cs, dinv):
    import gpk
    L = _upload_factor(ctx, cs.L)
    L2 = _upload_factor(ctx, cs.L2) if cs.L2 is not None else None
    prob = gpk.GNProblem(ctx, R.SYSTEM_NAME[cs.system], cs.Nd, cs.Nb, cs.f, cs.g, L, p0=cs.p0, p1=cs.p1, pen_lambda=cs.lam,
                         data_u=cs.data, L2=L2, dinv=dinv, structured=False, cache_a=False)
    prob.keep += [L] + ([L2] if L2 is not None else [])
    return prob


@functools.lru_cache(maxsize=None)
def _synthetic_reference(system, Nd):
    """per (system, N_d), shared by the dinv variants: K, long-double and float64-numpy results of every field"""
    cs = R.case(system, Nd)
    full = R.full_reference(system, Nd)                                # S = L^-1 A and H in long double (shared with test_gpu_gn_rounding)
    prepared = (full.S, PR.cholesky_ld(full.H / LD(2)))
    out = {}
    for field in ((0, 1) if system == 'darcy' else (0,)):
        n = PR.field_group(cs, field)[1]
        K = np.random.RandomState(1000 * Nd + field).normal(size=(n, NT_C))
        out[field] = (K, PR.variance_ld(cs, cs.z0, K, field, prepared=prepared), PR.variance_np64(cs, cs.z0, K, field))
    return out


@pytest.mark.parametrize('dinv', [256, False])
@pytest.mark.parametrize('Nd', [65, 129])
@pytest.mark.parametrize('system', ['elliptic', 'burgers', 'eikonal', 'darcy'])
def test_prepare_and_variance_arithmetic(dev_ctx, system, Nd, dinv):
    ctx, cs = dev_ctx, R.case(system, Nd)
    prob = _problem(ctx, cs, dinv)
    P, Rf, info = ctx.posterior_prepare(prob, ctx.array(cs.z0))
    assert info == 0
    for field, (K, ld, np64) in _synthetic_reference(system, Nd).items():
        vc, v = ctx.posterior_variance(prob, P, Rf, _padded(ctx, K, 5), field=field)
        ctx.synchronize()
        vc, v = vc.download(), v.download()
        s1 = LD(EPS) * (LD(1) + ld.sv)
        s2 = LD(EPS) * ld.sw
        r1 = lambda x: float(np.max(np.abs(np.asarray(x).astype(LD) - ld.var_cond) / s1))
        r2 = lambda x: float(np.max(np.abs(np.asarray(x).astype(LD) - ld.var_gn) / s2))
        tag = f'{system} {Nd} field {field} dinv {dinv}'
        _note('var_cond', r1(vc), R.allowed(r1(np64.var_cond)), tag)
        _note('var_gn', r2(v - vc), R.allowed(r2(np64.var_gn)), tag)
        assert r1(vc) <= R.allowed(r1(np64.var_cond)), tag
        assert r2(v - vc) <= R.allowed(r2(np64.var_gn)), tag
        # either output alone: the same bits
        only_c, none = ctx.posterior_variance(prob, None, None, _padded(ctx, K, 5), field=field, want_var=False)
        none2, only_v = ctx.posterior_variance(prob, P, Rf, _padded(ctx, K, 5), field=field, want_cond=False)
        ctx.synchronize()
        assert none is None and none2 is None
        assert np.array_equal(VA.bits(only_c.download()), VA.bits(vc)) and np.array_equal(VA.bits(only_v.download()), VA.bits(v))
    prob.free()


def test_relaxed_system_and_wrong_field_are_rejected(dev_ctx):
    import gpk
    ctx = dev_ctx
    cs = R.case('relaxed', 65)
    prob = _problem(ctx, cs, False)
    with pytest.raises(gpk.GpkError, match='-9001.*relaxed'):
        ctx.posterior_prepare(prob, ctx.array(cs.z0))
    prob.free()
    cs = R.case('elliptic', 65)
    prob = _problem(ctx, cs, False)
    P, Rf, _ = ctx.posterior_prepare(prob, ctx.array(cs.z0))
    K = ctx.array(np.zeros((prob.rows, 4)))
    with pytest.raises(gpk.GpkError, match='-9001.*field 1'):
        ctx.posterior_variance(prob, P, Rf, K, field=1)
    with pytest.raises(gpk.GpkError, match='-9001.*field'):
        ctx.posterior_variance(prob, P, Rf, K, field=2)
    prob.free()


@pytest.mark.parametrize('system,dinv', [('elliptic', 256), ('darcy', 256), ('darcy', False)])
def test_worksize_is_what_the_calls_use(system, dinv):
    """gpk_posterior_worksize against the buffers of the Python layer and against what a fresh handle's workspace has grown to after
    prepare and one batch of every field (development build: gpk_debug_workspace_bytes)"""
    import ctypes as C
    import gpk
    ctx = gpk.Context(0, dev=True)
    try:
        cs = R.case(system, 65)
        prob = _problem(ctx, cs, dinv)
        ws = ctx.posterior_worksize(prob, NT_C)
        assert (ws['ldp'], ws['ldr'], ws['ldk']) == (gpk.device.pad_ld(cs.nz + 1), gpk.device.pad_ld(cs.nz), gpk.device.pad_ld(NT_C))
        cap = C.c_size_t()
        ctx._chk(ctx.lib.gpk_debug_workspace_bytes(ctx.h, C.byref(cap)))
        before = cap.value                                             # (what building the problem left: the query speaks of the two calls)
        P, Rf, info = ctx.posterior_prepare(prob, ctx.array(cs.z0))
        assert info == 0 and P.nbytes == ws['P_bytes'] and Rf.nbytes == ws['R_bytes']
        for field in ((0, 1) if system == 'darcy' else (0,)):
            n = PR.field_group(cs, field)[1]
            K, W = ctx.empty(n, NT_C, ld=ws['ldk']), ctx.empty(cs.nz, NT_C, ld=ws['ldk'])
            K.upload(np.random.RandomState(field).normal(size=(n, NT_C)))
            assert W.nbytes == ws['W_bytes'] and K.nbytes <= ws['K_bytes'] and (field == 1 or K.nbytes == ws['K_bytes'])
            ctx.posterior_variance(prob, P, Rf, K, field=field, W=W)
        ctx.synchronize()
        ctx._chk(ctx.lib.gpk_debug_workspace_bytes(ctx.h, C.byref(cap)))
        assert cap.value == max(before, ws['handle_bytes']), (cap.value, before, ws)
        assert ws['handle_bytes'] >= ((ws['P_bytes'] if dinv else 0))
        with pytest.raises(gpk.GpkError, match='-9001'):
            ctx.posterior_worksize(prob, NT_C, ldk=NT_C - 1)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ d. real Gram matrices, class API
NT_D = 67
# driver arguments of each case.  Sizes and nuggets are the smallest at which the precondition of the gate holds with room (numpy error
# below 1e-3 of the smallest variance: checked on the CPU with tests/_posterior_reference.py at the oracle's iterate, ratios 1e-7 .. 6e-10)
# while cond(Theta) is still that of a real problem (5e7 .. 8e11); the kernel parameters are the drivers' defaults (elliptic: sigma 0.2)
REAL = {
    'Nonlinear_elliptic': ['--N_domain', '150', '--N_boundary', '40', '--kernel_parameter', '0.2', '--nugget', '1e-6', '--GNsteps', '4'],
    'Burgers': ['--N_domain', '120', '--N_boundary', '42', '--nugget', '1e-5', '--GNsteps', '4'],
    'Eikonal': ['--N_domain', '120', '--N_boundary', '40', '--nugget', '1e-6', '--GNsteps', '4'],
    'Darcy_flow2d': ['--N_domain', '100', '--N_boundary', '40', '--N_data', '20', '--nugget', '1e-5', '--GNsteps', '4'],
}
QUIET = ['--print_hist', '', '--show_figure', '']


def _solve(name):
    """(solver, cfg) of the class API at the sizes of REAL, seed fixed"""
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
    elif name == 'Burgers':
        import main_Burgers1d as drv
        cfg = drv.parse(REAL[name] + QUIET)
        np.random.seed(0)
        s, _ = solve_forward(cfg, name, drv.initial_and_lateral, lambda x1, x2: 0, drv.SPACE_TIME, verbose=False)
    else:
        import main_DarcyFlow2d as drv
        from src.solver import solver_GP
        cfg = drv.parse(REAL[name] + QUIET)
        np.random.seed(0)
        s = solver_GP(cfg, PDE_type='Darcy_flow2d')
        s.set_equation(bdy=lambda x1, x2: 0, rhs=drv.source, domain=np.array(drv.UNIT_SQUARE), print_option=False)
        s.auto_sample_IP(cfg.N_domain, cfg.N_boundary, cfg.N_data, print_option=False)
        Xo = s.eqn.X_data
        s.get_observed_data(np.sin(np.pi * Xo[:, 0]) * np.sin(np.pi * Xo[:, 1]) / 20.0, cfg.noise_level, print_option=False)
        s.solve(print_option=False)
    return s, cfg


def _real_case(name, e, cfg):
    """the problem the device solved, on the oracle's Gram matrices, in the reference's shape"""
    Nd, Nb = e.N_domain, e.N_boundary
    if name == 'Darcy_flow2d':
        Tu, Ta = O.gram_matrix_assembly(e.X_domain, e.X_boundary, name, cfg.kernel, cfg.kernel_parameter)
        Tu, _ = O.add_nugget(Tu, 'Darcy_u', Nd, Nb, cfg.nugget)
        Ta, _ = O.add_nugget(Ta, 'Darcy_a', Nd, Nb, cfg.nugget)
        return PR.RealCase('darcy', Nd, Nb, e.rhs_f, e.bdy_g, float(e.noise_level), 0.0, Tu, Ta, data=e.data_u)
    T, _ = O.add_nugget(O.gram_matrix_assembly(e.X_domain, e.X_boundary, name, cfg.kernel, cfg.kernel_parameter), name, Nd, Nb, cfg.nugget)
    system = {'Nonlinear_elliptic': 'elliptic', 'Burgers': 'burgers', 'Eikonal': 'eikonal'}[name]
    p0, p1, _ = e._gn_params()
    return PR.RealCase(system, Nd, Nb, e.rhs_f, e.bdy_g, p0, p1, T)


@pytest.mark.parametrize('name', sorted(REAL))
def test_class_api_on_real_gram_matrices(name):
    s, cfg = _solve(name)
    e = s.eqn
    rng = np.random.RandomState(42)
    lo, hi = np.asarray(e.domain, dtype=float).T
    Xt = lo + (hi - lo) * rng.uniform(0, 1, (NT_D, 2))
    e.extend_sol(Xt)                                                   # (Darcy: both fields, extended_sol_u / extended_sol_a)
    darcy = name == 'Darcy_flow2d'
    for k in (('extended_sol_u', 'extended_sol_a') if darcy else ('extended_sol',)) + ('X_test', 'N_test'):
        assert k in e.__dict__, k
    keep = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in e.__dict__.items() if not k.startswith('_')}
    tags = ('_u', '_a') if darcy else ('',)
    grab = lambda: {t: (getattr(e, 'extended_var_cond' + t).copy(), getattr(e, 'extended_var' + t).copy()) for t in tags}
    e.posterior_variance(Xt, nt_chunk=32)                              # two full batches and a remainder of 3
    small = grab()
    e.posterior_variance(Xt, nt_chunk=32)
    for t in tags:                                                     # a repeat: the same bits
        assert all(np.array_equal(VA.bits(a), VA.bits(b)) for a, b in zip(small[t], grab()[t]))
    e.posterior_variance(Xt, nt_chunk=1024)
    big = grab()
    e.posterior_variance(Xt, nt_chunk=1024)
    for t in tags:
        assert all(np.array_equal(VA.bits(a), VA.bits(b)) for a, b in zip(big[t], grab()[t]))
    # surface: std, and nothing extend_sol / GN_method set has changed
    for t in tags:
        assert np.array_equal(getattr(e, 'extended_std' + t), np.sqrt(np.maximum(getattr(e, 'extended_var' + t), 0.0)))
    for k, v in keep.items():                                          # arrays bit for bit
        w = e.__dict__[k]
        assert (np.array_equal(VA.bits(v), VA.bits(w)) if isinstance(v, np.ndarray) and v.dtype == np.float64 else
                np.array_equal(v, w) if isinstance(v, np.ndarray) else v is w or v == w), k
    added = {k for k in e.__dict__ if not k.startswith('_')} - set(keep)
    assert added == {n + t for n in ('extended_var', 'extended_var_cond', 'extended_std') for t in tags}, added
    e.extend_sol(Xt)                                                   # and extend_sol itself gives what it gave
    for k in ('extended_sol_u', 'extended_sol_a') if darcy else ('extended_sol',):
        assert np.array_equal(VA.bits(keep[k]), VA.bits(e.__dict__[k])), k
    # the long-double formula at the device's own final iterate, on the oracle's Theta
    cs = _real_case(name, e, cfg)
    z = e._z_star[1]
    ld, f64 = cs.factors()
    prepared = PR.prepare_ld(cs, z, ld)
    Kt = O.construct_theta_test(Xt, e.X_domain, e.X_boundary, name, cfg.kernel, cfg.kernel_parameter)
    for field, t in enumerate(tags):
        K = (Kt[field] if darcy else Kt).T
        ref = PR.variance_ld(cs, z, K, field, ld, prepared).var
        np64 = PR.variance_np64(cs, z, K, field, f64).var
        err_np = float(np.max(np.abs(np64.astype(LD) - ref)))
        vmin = float(np.min(ref))
        print(f'\n[posterior] real {name}{t}: numpy error {err_np:.3g}, min var {vmin:.3g}, max var {float(np.max(ref)):.3g}')
        assert err_np < 1e-3 * vmin, 'precondition: the gate could hide a wrong result'
        for what, res in (('nt_chunk 32', small), ('nt_chunk 1024', big)):
            err = float(np.max(np.abs(res[t][1].astype(LD) - ref)))
            _note('real', err, R.MARGIN * err_np, f'{name}{t} {what}')
            assert err <= R.MARGIN * err_np, (name, t, what, err, err_np)


# ------------------------------------------------------------------------------------------------ e. surface
def test_what_is_not_served_says_so():
    from src.PDEs import Nonlinear_elliptic2d, Nonlinear_elliptic3d
    one = lambda *x: 1.0
    Xt = np.full((3, 2), 0.5)
    with pytest.raises(NotImplementedError, match='gpk_assemble_bc'):
        Nonlinear_elliptic2d(bdy=one, rhs=one, bc='robin').posterior_variance(Xt)
    with pytest.raises(NotImplementedError, match='gpk_assemble_op'):
        Nonlinear_elliptic2d(bdy=one, rhs=one, operator=lambda x1, x2: (0, 0, 0, 1, 0, 1)).posterior_variance(Xt)
    with pytest.raises(NotImplementedError, match='three-dimensional'):
        Nonlinear_elliptic3d(bdy=one, rhs=one).posterior_variance(np.full((3, 3), 0.5))
    import main_NonLinElliptic2d as drv
    from _driver_common import solve_forward
    cfg = drv.parse(['--N_domain', '60', '--N_boundary', '20', '--GNsteps', '2'] + QUIET)
    u, f = drv.manufactured(cfg.alpha, cfg.m)
    np.random.seed(0)
    s, _ = solve_forward(cfg, 'Nonlinear_elliptic', u, f, drv.UNIT_SQUARE, solve_kwargs={'method': 'relaxation'}, verbose=False)
    with pytest.raises(NotImplementedError, match='relaxed'):
        s.eqn.posterior_variance(Xt)
    s.eqn.GN_method(max_iter=2, print_hist=False)                      # the elimination solve of the same object is served
    assert s.eqn.posterior_variance(Xt).shape == (3,)


def test_driver_flag(capsys):
    import main_NonLinElliptic2d as drv
    from src._runtime import get_context
    base = ['--N_domain', '150', '--N_boundary', '40', '--nugget', '1e-6'] + QUIET
    np.random.seed(0)
    drv.main(base)
    plain = capsys.readouterr().out
    np.random.seed(0)
    drv.main(base + ['--test_variance', 'True'])
    with_var = capsys.readouterr().out
    pl, wv = plain.splitlines(), with_var.splitlines()
    assert not any('variance' in line for line in pl)
    assert any('[Test error]' in line for line in pl) and any('Loss' in line or 'error' in line for line in pl)
    # the flag changes nothing in front of its own lines: every character of the default output, numbers included (same seed, same
    # handle, fixed-order reductions: two solves give the same bits)
    assert wv[:len(pl)] == pl, [(a, b) for a, b in zip(pl, wv) if a != b][:3]
    tag = lambda line: line.split(']')[0]
    assert [tag(x) for x in wv[len(pl):]] == ['[Testing posterior variance...', '[Test variance', '[Test variance'], wv[len(pl):]
    assert 'Mean posterior std' in wv[-2] and 'Max posterior std' in wv[-1]
    assert 0 < float(wv[-2].split()[-1]) <= float(wv[-1].split()[-1]) < 1
    get_context().synchronize()
