"""Neumann / Robin / mixed boundary functionals on the device: gpk_assemble_bc entry by entry (both store variants, unaligned views
between canaries, Dirichlet coefficients against gpk_assemble), gpk_extend_functionals_bc, the class API and the facade end to end
against a numpy pipeline with a measured sensitivity, and no interference with the 2-D and 3-D calls that share the handle's point
scratch.  The expectation lives in test_robin_host.py."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'nonlinpdes-gpsolver_amd')
if PKG not in sys.path:
    sys.path.insert(0, PKG)

import _view_arena as VA  # noqa: E402
import test_elliptic3d_host as H3  # noqa: E402
import test_robin_host as HR  # noqa: E402

EPS = HR.EPS
LD = HR.LD
# Rounding budget of one entry relative to T = sum of |terms| x kappa (u = eps / 2 per rounding; the expectation is longdouble, so all
# of it is the device's), by the count of test_gpu_elliptic3d.py:
#   exp argument  -(p1 d1^2 + p2 d2^2)/2: positive terms, 2 products + at most 2 additions each -> relative error <= 4 u of the
#                 argument = 2 eps |arg|, which the exponential turns into a RELATIVE error 2 eps |arg| of kappa;
#                 |arg| <= (p1 + p2)/2 on the unit square = 27.1 for the anisotropic pair (p = 2/0.3^2, 2/0.25^2; 25 for sigma = 0.2)  <= 55 eps
#   the exponential itself (1 ulp), the product with kappa (1 u), the nugget addition (1 u)                                           <=  2 eps
#   a Hermite factor: at most 6 roundings; two factors and the product joining them 2 x 6 + 1 = 13 u                                 <=  7 eps
#   the two coefficient products (2 u)                                                                                                <=  1 eps
#   the sum of up to nine terms, 8 additions                                                                                          <=  4 eps
# together <= 69 eps T.  As there, T does not see a cancellation INSIDE one Hermite factor (h2 near p d^2 = 1); the factor ~1.5 left
# between the count and C covers it.
C_ENTRY = 128
# the extension adds the product with the coefficient-vector entry (1 u) and the sum over the columns: per lane 2 column points, then
# 6 shuffle steps and 2 LDS additions -- under 16 u = 8 eps of sum|terms| for the sizes here: the same constant holds
C_EXTEND = 128
SHAPES = [(1, 0), (1, 1), (37, 17), (256, 96), (300, 150)]
NUGGET = 1e-3                                                           # large enough to be visible in every diagonal entry
WORST = {}


@pytest.fixture(scope='module')
def ctx():
    from src._runtime import get_context
    return get_context()


@functools.lru_cache(maxsize=None)
def _points(Nd, Nb):
    rng = np.random.RandomState(1000 * Nd + Nb)
    Xd = rng.uniform(0, 1, (Nd, 2))
    Xb = HR.face_points(rng, Nb)
    return Xd, Xb


@functools.lru_cache(maxsize=None)
def _case(kernel, kp, Nd, Nb, cset):
    """points, coefficients and the longdouble expectation (Theta without nugget, sum of |terms|), once per (kernel, shape, set)"""
    Xd, Xb = _points(Nd, Nb)
    c = HR.coeff_set(cset, Xb, np.random.RandomState(7 * Nd + Nb))
    p = HR.precisions(kernel, kp)
    T, mag = HR.theta(Xd, Xb, c, p, dtype=LD)
    return Xd, Xb, c, p, T, mag


def _check_theta(got, kernel, kp, Nd, Nb, cset, nugget_type, tag):
    Xd, Xb, c, p, T, mag = _case(kernel, kp, Nd, Nb, cset)
    nug = np.diag(HR.nugget_diag(p, Nd, Nb, c, NUGGET, nugget_type)).astype(LD)
    err = np.abs(got.astype(LD) - (T + nug))
    ratio = float(np.max(err / (EPS * (mag + nug))))
    WORST[tag] = max(WORST.get(tag, 0.0), ratio)
    print(f'\n[{tag} {kernel} ({Nd},{Nb}) {cset} {nugget_type}] max |dev - ref| / (eps (T + nugget)) = {ratio:.2f}')
    assert np.all(err <= C_ENTRY * EPS * (mag + nug)), (kernel, Nd, Nb, cset, nugget_type, ratio)


@pytest.mark.parametrize('cset', HR.COEFF_SETS)
@pytest.mark.parametrize('Nd,Nb', SHAPES)
@pytest.mark.parametrize('kernel,kp', HR.KERNELS)
def test_theta_entrywise(ctx, kernel, kp, Nd, Nb, cset):
    Xd, Xb, c, p, _, _ = _case(kernel, kp, Nd, Nb, cset)
    N = 2 * Nd + Nb
    analytic = HR.trace_ratio(p, Nd, Nb, c, LD)
    for nugget_type in ('none', 'identity', 'adaptive'):
        T, ratio = ctx.assemble_bc(kernel, kp, Xd, Xb, c, NUGGET, nugget_type)
        assert (T.rows, T.cols) == (N, N)
        got = T.download()
        T.free()
        _check_theta(got, kernel, kp, Nd, Nb, cset, nugget_type, 'theta')
        assert abs(LD(ratio) - analytic) <= 4 * EPS * analytic, (ratio, float(analytic))
    print(f'[theta] worst ratio so far {WORST["theta"]:.2f} of {C_ENTRY}')


@pytest.mark.parametrize('Nd,Nb', SHAPES)
@pytest.mark.parametrize('kernel,kp', HR.KERNELS)
def test_dirichlet_coefficients_and_null_against_gpk_assemble(ctx, kernel, kp, Nd, Nb):
    Xd, Xb, c, p, _, mag = _case(kernel, kp, Nd, Nb, 'dirichlet')
    assert np.array_equal(c, np.tile([1.0, 0.0, 0.0], (Nb, 1)))
    for nugget_type in ('none', 'adaptive'):
        Ta, ra = ctx.assemble('Nonlinear_elliptic', kernel, kp, Xd, Xb, NUGGET, nugget_type)
        Tn, rn = ctx.assemble_bc(kernel, kp, Xd, Xb, None, NUGGET, nugget_type)
        Te, re_ = ctx.assemble_bc(kernel, kp, Xd, Xb, c, NUGGET, nugget_type)
        a, n, e = Ta.download(), Tn.download(), Te.download()
        for t in (Ta, Tn, Te):
            t.free()
        nug = np.diag(HR.nugget_diag(p, Nd, Nb, c, NUGGET, nugget_type))
        bound = C_ENTRY * EPS * (mag.astype(np.float64) + nug)
        assert np.all(np.abs(n - a) <= bound) and np.all(np.abs(e - a) <= bound)
        print(f'\n[dirichlet {kernel} ({Nd},{Nb}) {nugget_type}] bit-identical to gpk_assemble: {np.array_equal(n, a)}; '
              f'max |bc - assemble| / (eps (T + nugget)) = {float(np.max(np.abs(n - a) / (EPS * (mag.astype(np.float64) + nug)))):.2f}')
        assert np.array_equal(n, e)                                       # NULL and explicit (1,0,0): the same bits
        assert rn == re_ and abs(rn - ra[0]) <= 4 * EPS * rn
        _check_theta(n, kernel, kp, Nd, Nb, 'dirichlet', nugget_type, 'null')


def test_paired_and_single_point_variants_agree(ctx):
    """the same even-sized problem through the 16-byte-store kernel, its non-temporal form (gpk_tune key 55) and the one-point kernel
    (key 47 = 0): the same per-pair arithmetic, so the same bits"""
    kernel, kp = HR.KERNELS[1]
    Xd, Xb, c, _, _, _ = _case(kernel, kp, 256, 96, 'mixed')
    outs = []
    try:
        for key, val in ((47, 1), (55, 1), (47, 0)):
            ctx.tune(key, val)
            T, _ = ctx.assemble_bc(kernel, kp, Xd, Xb, c, NUGGET, 'adaptive')
            outs.append(T.download()); T.free()
    finally:
        ctx.tune(47, 1); ctx.tune(55, 0)
    _check_theta(outs[1], kernel, kp, 256, 96, 'mixed', 'adaptive', 'nt')
    _check_theta(outs[2], kernel, kp, 256, 96, 'mixed', 'adaptive', 'single')
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])


@pytest.mark.parametrize('Nd,Nb', [(37, 17), (256, 96)])
@pytest.mark.parametrize('kernel,kp', HR.KERNELS)
def test_theta_into_unaligned_view_between_canaries(ctx, kernel, kp, Nd, Nb):
    """every alignment class of the arena: only 'A' (16-byte aligned base, even leading dimension) may take the two-point path on the even
    sizes; an odd base alone ('B'), an odd leading dimension alone ('C') and both ('D') must each send it to the one-point kernel --
    a 16-byte store there is misaligned or crosses into the canaries"""
    from gpk.device import KERNEL, NUGGET as NUG, kernel_params
    Xd, Xb, c, p, _, _ = _case(kernel, kp, Nd, Nb, 'mixed')
    N = 2 * Nd + Nb
    dXd, dXb, dbc = ctx.points(Xd), ctx.points(Xb), ctx._boundary_coeffs(c, Nb)
    for cls in VA.CLASSES:
        v = VA.class_view(ctx, N, N, cls)
        assert v.cls == cls
        ratio = C.c_double()
        rc = ctx.lib.gpk_assemble_bc(ctx.h, KERNEL[kernel], kernel_params(kernel, kp), dXd.ptr, Nd, dXb.ptr, Nb, dbc.ptr, NUGGET,
                                     NUG['adaptive'], v.ptr, v.ld, C.byref(ratio))
        assert rc == 0
        ctx.synchronize()
        v.arena.assert_outside_untouched([v])
        _check_theta(v.arena.get(v), kernel, kp, Nd, Nb, 'mixed', 'adaptive', 'view')
        v.arena.free()


# ---- gpk_extend_functionals_bc -----------------------------------------------------------------------------------------------------
ALL5 = ('value', 'd1', 'd2', 'd2d2', 'laplacian')                         # ascending bit order


@pytest.mark.parametrize('cset', ('mixed', 'robin'))
@pytest.mark.parametrize('which', [('value',), ('value', 'd1', 'd2'), ALL5])
@pytest.mark.parametrize('Nt', (1, 5, 257))
def test_extend_functionals_bc(ctx, Nt, which, cset):
    kernel, kp = HR.KERNELS[1]
    Nd, Nb = 300, 150                                                     # 450 column points: two strides of the 256 lanes
    Xd, Xb, c, p, _, _ = _case(kernel, kp, Nd, Nb, cset)
    rng = np.random.RandomState(Nt)
    Xt = rng.uniform(0, 1, (Nt, 2))
    Xt[0] = Xd[3]                                                         # a coincident point
    coeff = rng.normal(size=2 * Nd + Nb) * 10.0 ** rng.uniform(0, 4, 2 * Nd + Nb)
    got = ctx.extend_functionals_bc(kernel, kp, Xt, Xd, Xb, c, coeff, which=which).download().reshape(len(which), Nt)
    ref, terms, _ = HR.extend_rows(which, Xt, Xd, Xb, c, coeff, p, dtype=LD)
    for k, n in enumerate(which):
        err = np.abs(got[k].astype(LD) - ref[n])
        ratio = float(np.max(err / (EPS * terms[n])))
        WORST['extend'] = max(WORST.get('extend', 0.0), ratio)
        print(f'\n[extend_bc {cset} Nt={Nt} {n}] max |dev - ref| / (eps sum|terms|) = {ratio:.2f}')
        assert np.all(err <= C_EXTEND * EPS * terms[n]), (n, ratio)
    again = ctx.extend_functionals_bc(kernel, kp, Xt, Xd, Xb, c, coeff, which=which).download().reshape(len(which), Nt)
    assert np.array_equal(got, again)                                     # fixed reduction order: bit-identical


def test_extend_functionals_bc_null_is_the_dirichlet_extension(ctx):
    kernel, kp = HR.KERNELS[0]
    Nd, Nb = 37, 17
    Xd, Xb, c, p, _, _ = _case(kernel, kp, Nd, Nb, 'dirichlet')
    rng = np.random.RandomState(2)
    Xt = rng.uniform(0, 1, (9, 2)); coeff = rng.normal(size=2 * Nd + Nb)
    a = ctx.extend_functionals_bc(kernel, kp, Xt, Xd, Xb, None, coeff, which=ALL5).download()
    b = ctx.extend_functionals_bc(kernel, kp, Xt, Xd, Xb, c, coeff, which=ALL5).download()
    d = ctx.extend_functionals('Nonlinear_elliptic', kernel, kp, Xt, Xd, Xb, coeff, which=ALL5).download()
    assert np.array_equal(a, b)
    _, terms, _ = HR.extend_rows(ALL5, Xt, Xd, Xb, c, coeff, p)
    for k, n in enumerate(ALL5):                                         # (each side within C_EXTEND eps of the exact row)
        assert np.all(np.abs(a.reshape(5, -1)[k] - d.reshape(5, -1)[k]) <= 2 * C_EXTEND * EPS * terms[n]), n
    # the caller's order of the rows
    r = ctx.extend_functionals_bc(kernel, kp, Xt, Xd, Xb, c, coeff, which=('laplacian', 'value')).download().reshape(2, -1)
    assert np.array_equal(r[0], b.reshape(5, -1)[4]) and np.array_equal(r[1], b.reshape(5, -1)[0])


def test_rejected_arguments(ctx):
    from gpk.device import kernel_params
    rng = np.random.RandomState(0)
    Xd, Xb, Xt = rng.uniform(0, 1, (20, 2)), HR.face_points(rng, 6), rng.uniform(0, 1, (8, 2))
    dXt, dXd, dXb, dc = ctx.points(Xt), ctx.points(Xd), ctx.points(Xb), ctx.array(rng.normal(size=46))
    dbc = ctx._boundary_coeffs(HR.coeff_set('robin', Xb), 6)
    out = ctx.empty(5, 8, ld=8)
    T = ctx.empty(46, 46)
    kp = kernel_params('Gaussian', 0.2)
    ext = lambda mask, Nt=8, ldo=8, Nd=20, Nb=6: ctx.lib.gpk_extend_functionals_bc(ctx.h, 0, kp, dXt.ptr, Nt, dXd.ptr, Nd, dXb.ptr, Nb,
                                                                                   dbc.ptr, dc.ptr, mask, out.ptr, ldo)
    assert ext(31) == 0 and ext(1) == 0
    for bad in (dict(mask=0), dict(mask=32), dict(mask=64), dict(mask=-1), dict(mask=1, Nt=0), dict(mask=1, ldo=7), dict(mask=1, Nd=0),
                dict(mask=1, Nb=-1)):
        assert ext(**bad) == -9001, bad
        assert b'extend_functionals_bc' in ctx.lib.gpk_last_error(ctx.h), bad
    asm = lambda Nd=20, Nb=6, ld=T.ld, nt=2, kernel=0: ctx.lib.gpk_assemble_bc(ctx.h, kernel, kp, dXd.ptr, Nd, dXb.ptr, Nb, dbc.ptr, 1e-3, nt,
                                                                               T.ptr, ld, None)
    assert asm() == 0                                                     # (host_ratio may be NULL)
    for bad in (dict(Nd=0), dict(Nb=-1), dict(ld=45), dict(nt=3), dict(kernel=2)):
        assert asm(**bad) == -9001, bad
        assert b'assemble_bc' in ctx.lib.gpk_last_error(ctx.h), bad
    ctx.synchronize()


# ---- the other evaluators on the same handle -------------------------------------------------------------------------------------
def test_2d_and_3d_calls_are_unaffected_by_a_bc_call(ctx):
    """the point scratch is shared and re-packed per call (5 arrays here, 2 and 3 there): the 2-D and 3-D calls give the bits they gave
    before a _bc call came in between"""
    kernel, kp = HR.KERNELS[1]
    Xdb, Xbb, cb, _, _, _ = _case(kernel, kp, 300, 150, 'mixed')
    rng = np.random.RandomState(9)
    Nd, Nb = 37, 17
    Xd, Xb, Xt = rng.uniform(0, 1, (Nd, 2)), rng.uniform(0, 1, (Nb, 2)), rng.uniform(0, 1, (11, 2))
    c = rng.normal(size=2 * Nd + Nb)
    kernel3, kp3 = H3.KERNELS[0]
    Xd3, Xb3, Xt3 = rng.uniform(0, 1, (Nd, 3)), rng.uniform(0, 1, (Nb, 3)), rng.uniform(0, 1, (11, 3))

    def others():
        T, _ = ctx.assemble('Nonlinear_elliptic', kernel, kp, Xd, Xb, 1e-3, 'adaptive')
        e = ctx.extend('Nonlinear_elliptic', kernel, kp, Xt, Xd, Xb, c).download()
        T3, _ = ctx.assemble3d(kernel3, kp3, Xd3, Xb3, 1e-3, 'adaptive')
        e3 = ctx.extend_functionals3d(kernel3, kp3, Xt3, Xd3, Xb3, c).download()
        out = (T.download(), e, T3.download(), e3)
        T.free(); T3.free()
        return out

    def bc_call():
        T, _ = ctx.assemble_bc(kernel, kp, Xdb, Xbb, cb, 1e-3, 'adaptive')
        got = T.download(); T.free()
        return got

    before = others()
    first = bc_call()
    T, _ = ctx.assemble('Nonlinear_elliptic', kernel, kp, Xd, Xb, 1e-3, 'adaptive')
    a = T.download(); T.free()
    assert np.array_equal(a, before[0])
    bc_call()
    assert np.array_equal(ctx.extend('Nonlinear_elliptic', kernel, kp, Xt, Xd, Xb, c).download(), before[1])
    bc_call()
    T3, _ = ctx.assemble3d(kernel3, kp3, Xd3, Xb3, 1e-3, 'adaptive')
    a3 = T3.download(); T3.free()
    assert np.array_equal(a3, before[2])
    ctx.extend_functionals_bc(kernel, kp, Xt, Xdb, Xbb, cb, rng.normal(size=750), which=('value',))
    assert np.array_equal(ctx.extend_functionals3d(kernel3, kp3, Xt3, Xd3, Xb3, c).download(), before[3])
    assert np.array_equal(bc_call(), first)                               # and the other way round
    _check_theta(first, kernel, kp, 300, 150, 'mixed', 'adaptive', 'interleaved')


def test_assembly_timing_covers_the_bc_launch(ctx):
    kernel, kp = HR.KERNELS[0]
    Xd, Xb, c, _, _, _ = _case(kernel, kp, 300, 150, 'robin')
    ctx.prof_enable(True)
    try:
        T, _ = ctx.assemble_bc(kernel, kp, Xd, Xb, c, 1e-3, 'adaptive'); T.free()
        ms = ctx.prof_read_assembly()
    finally:
        ctx.prof_enable(False)
    assert ms > 0.0, ms


# ---- end to end through the class API and the facade ---------------------------------------------------------------------------------
# SEED: of the sampler seeds 0..5 the one whose numpy pipeline is least sensitive (s_J between 1.2e-6 and 9.5e-6 over those seeds, a noisy
# maximum over three perturbations; 100 s_J must stay under the 1e-3 sanity gate on any BLAS) -- chosen from the numpy pipeline alone
ND, NB, SIGMA, NUGGET_E2E, STEPS, SEED, BETA = 400, 160, 0.2, 1e-8, 6, 4, 2.0
# Nd 8 p^2 / (Nd + Nb (beta^2 + p)), p = 25: beta = 0 (Neumann) and beta = 2 (Robin)
RATIO = {'neumann': 400 * 8 * 625 / (400 + 160 * 25.0), 'robin': 400 * 8 * 625 / (400 + 160 * 29.0)}


def _cfg(bc):
    class Cfg:
        alpha, m = 1.0, 3
        kernel, kernel_parameter, nugget, nugget_type = 'Gaussian', SIGMA, NUGGET_E2E, 'adaptive'
        GNsteps, step_size, initial_sol, print_hist = STEPS, 1, 'rdm', False
    Cfg.bc, Cfg.robin_beta = bc, BETA
    return Cfg()


@functools.lru_cache(maxsize=None)
def _solved(bc):
    """the class solve on the device and the numpy pipeline on the same points and initial guess, with the pipeline's own sensitivity"""
    from src.PDEs import Nonlinear_elliptic2d
    eqn = Nonlinear_elliptic2d(alpha=1.0, m=3, bdy=HR.bdy_for(bc, BETA), rhs=HR.rhs_for(1.0, 3), domain=np.array(HR.UNIT_SQUARE), bc=bc,
                               robin_beta=BETA)
    np.random.seed(SEED)
    eqn.sampled_pts(ND, NB, sampled_type='random')
    eqn.Gram_matrix(kernel='Gaussian', kernel_parameter=SIGMA, nugget=NUGGET_E2E, nugget_type='adaptive')
    eqn.Gram_Cholesky()
    eqn.GN_method(max_iter=STEPS, step_size=1, initial_sol='rdm', print_hist=False)
    p = HR.precisions('Gaussian', SIGMA)
    pipe = HR.NumpyPipeline(eqn.X_domain, eqn.X_boundary, eqn.boundary_coeffs, p, NUGGET_E2E, eqn.rhs_f, eqn.bdy_g)
    z, hist, L = pipe.run(eqn.init_sol, STEPS)
    s_z, s_J = pipe.sensitivity(eqn.init_sol, STEPS, z, hist)
    return dict(eqn=eqn, pipe=pipe, z=z, hist=hist, L=L, s_z=s_z, s_J=s_J, p=p)


@pytest.fixture(params=('neumann', 'robin'))
def solved(request, ctx):
    return dict(_solved(request.param), bc=request.param)


def test_end_to_end_against_the_numpy_pipeline(solved):
    """CPU trial of this configuration (numpy pipeline alone, the class's initial guess at seed 4): s_z = 1.7e-10 / 9.8e-11 and
    s_J = 2.8e-6 / 3.5e-6 (Neumann / Robin), cond Theta = 1.4e13, L2 error at the collocation points 4.5e-4 / 2.2e-4."""
    eqn, z, hist, s_z, s_J, bc = (solved[k] for k in ('eqn', 'z', 'hist', 's_z', 's_J', 'bc'))
    print(f'\n[{bc} e2e] s_z = {s_z:.3e}, s_J = {s_J:.3e}')
    assert 100 * s_z <= 1e-7 and 100 * s_J <= 1e-3, ('gate mis-set: the numpy pipeline itself is too sensitive', s_z, s_J)
    assert np.array_equal(eqn.boundary_coeffs, HR.operator_coeffs(bc, BETA, eqn.X_boundary))
    assert eqn.chol_info == 0
    assert eqn.step_info == [0] * STEPS
    assert abs(eqn.ratio - RATIO[bc]) <= 1e-12 * RATIO[bc], (eqn.ratio, RATIO[bc])
    dz = float(np.linalg.norm(eqn.sol_sampled_pts - z) / np.linalg.norm(z))
    dJ = float(np.max(np.abs(np.asarray(eqn.loss_hist) - hist) / hist))
    print(f'[{bc} e2e] |z_gpu - z_np| / |z_np| = {dz:.3e} (gate {100 * s_z:.3e}); max rel. loss difference = {dJ:.3e} (gate {100 * s_J:.3e})')
    assert len(eqn.loss_hist) == STEPS + 1
    assert dz <= 100 * s_z
    assert dJ <= 100 * s_J
    u = HR.truth(*eqn.X_domain.T)
    err_np = float(np.sqrt(np.mean((z - u) ** 2)))
    err_gpu = float(np.sqrt(np.mean((eqn.sol_sampled_pts - u) ** 2)))
    print(f'[{bc} e2e] L2 error at the collocation points: device {err_gpu:.3e}, numpy {err_np:.3e}')
    assert err_gpu <= 2 * err_np


def test_boundary_and_pde_residual_of_the_solution(solved):
    """device rows against numpy rows built from the pipeline's own factor: ||dev - numpy|| <= gate ||K|| ||c|| per row functional with the
    measured gate 100 s_z, combined for the two residuals by their (linearised) dependence on the rows"""
    from scipy.linalg import cho_solve
    eqn, pipe, z, p, bc = solved['eqn'], solved['pipe'], solved['z'], solved['p'], solved['bc']
    gate = 100 * solved['s_z']
    c_np = cho_solve((solved['L'], True), pipe.measurement(z))          # Theta^{-1} sol_vec, sol_vec = [alpha z^m - f; z; g] = F(z)
    cn = float(np.linalg.norm(c_np))
    # 200 fresh boundary points
    rng = np.random.RandomState(3)
    Xbt = HR.face_points(rng, 200)
    ct = HR.operator_coeffs(bc, BETA, Xbt)
    gt = HR.operator_value(ct, Xbt)
    ref, _, norms = HR.extend_rows(('value', 'd1', 'd2'), Xbt, eqn.X_domain, eqn.X_boundary, eqn.boundary_coeffs, c_np, p)
    r_np = ct[:, 0] * ref['value'] + ct[:, 1] * ref['d1'] + ct[:, 2] * ref['d2'] - gt
    r = eqn.boundary_residual(Xbt, ct, gt)
    assert r.shape == (200,) and r is eqn.bdy_residual
    scale = sum(float(np.max(np.abs(ct[:, k]))) * norms[n] for k, n in enumerate(('value', 'd1', 'd2')))
    err = float(np.linalg.norm(r - r_np))
    print(f'\n[{bc}] boundary residual: |dev - numpy| = {err:.3e}, gate {gate * scale * cn:.3e}; max |residual| = {np.max(np.abs(r)):.3e}')
    assert err <= gate * scale * cn
    # 500 interior points: r = -Lap u + u^3 - f; d(u^3) = 3 u^2 du
    Xt = rng.uniform(0.02, 0.98, (500, 2))
    ref, _, norms = HR.extend_rows(('value', 'laplacian'), Xt, eqn.X_domain, eqn.X_boundary, eqn.boundary_coeffs, c_np, p)
    r_np = -ref['laplacian'] + ref['value'] ** 3 - HR.rhs_for(1.0, 3)(*Xt.T)
    r = eqn.PDE_residual(Xt)
    scale = norms['laplacian'] + 3 * float(np.max(ref['value'] ** 2)) * norms['value']
    err = float(np.linalg.norm(r - r_np))
    print(f'[{bc}] PDE residual: |dev - numpy| = {err:.3e}, gate {gate * scale * cn:.3e}; max |residual| = {np.max(np.abs(r)):.3e}')
    assert err <= gate * scale * cn
    # extend_sol and extend_derivatives go through the same entry point
    eqn.extend_sol(Xt)
    rows = eqn.extend_derivatives(Xt)
    assert tuple(rows) == ('value', 'd1', 'd2', 'laplacian') and np.array_equal(rows['value'], eqn.extended_sol)
    assert float(np.linalg.norm(rows['value'] - ref['value'])) <= gate * norms['value'] * cn


def test_facade_gives_the_class_result_bitwise(solved):
    from src.solver import solver_GP
    bc = solved['bc']
    s = solver_GP(_cfg(bc), 'Nonlinear_elliptic')
    s.set_equation(bdy=HR.bdy_for(bc, BETA), rhs=HR.rhs_for(1.0, 3), domain=np.array(HR.UNIT_SQUARE), print_option=False)
    np.random.seed(SEED)
    s.auto_sample(ND, NB, sampled_type='random', print_option=False)
    s.solve(method='elimination', print_option=False)
    assert (s.eqn.bc, s.eqn.robin_beta) == (bc, BETA)
    assert np.array_equal(s.eqn.sol_sampled_pts, solved['eqn'].sol_sampled_pts)
    assert np.array_equal(np.asarray(s.eqn.loss_hist), np.asarray(solved['eqn'].loss_hist)) and s.eqn.ratio == solved['eqn'].ratio
    Xt = np.random.RandomState(4).uniform(0, 1, (64, 2))
    s.test(Xt, print_option=False)
    s.get_test_error(HR.truth(*Xt.T), print_option=False)
    s.test_residual(Xt, print_option=False)
    assert np.isfinite(s.test_L2_err) and np.isfinite(s.test_res_L2)
