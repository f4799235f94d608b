"""Variable-coefficient operator on the device: gpk_assemble_op entry by entry (every store variant, unaligned views between canaries,
the Laplacian against gpk_assemble_bc), gpk_extend_functionals_op, the class API and the facade end to end against a numpy pipeline
with a measured sensitivity, and no interference with the other evaluators that share the handle's point scratch.  The expectation
lives in test_operator_host.py."""
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
import test_operator_host as HO  # noqa: E402
import test_robin_host as HR  # noqa: E402

EPS = HR.EPS
LD = HR.LD
# Rounding budget of one entry relative to mag = sum of |coefficients| x H~ H~ kappa (the expectation is longdouble, so all of it is the
# device's): exp argument <= 55 eps (|arg| <= 27.1 on the unit square, relative error 2 eps |arg| of kappa); the exponential, the
# product with kappa and the nugget addition 2 eps; two Hermite factors and their product 7 eps; the coefficient products 1 eps; up to
# 35 additions <= 18 eps: together <= 83 eps.
C_ENTRY = HO.C_ENTRY
# the extension: the weights w = op_q c[q] + bc_q c[Nd + q] (2 roundings), then the sum over the columns -- per lane 2 column points, 6
# shuffle steps and 2 LDS additions, under 8 eps of the magnitude: the same constant holds
C_EXTEND = 128
NUGGET = 1e-3                                                           # large enough to be visible in every diagonal entry
WORST = {}


@pytest.fixture(scope='module')
def ctx():
    from src._runtime import get_context
    return get_context()


@functools.lru_cache(maxsize=None)
def _case(kernel, kp, Nd, Nb, oset, bset):
    """points, coefficients and the longdouble expectation (Theta without nugget, mag), once per (kernel, shape, sets)"""
    return HO.case(kernel, kp, Nd, Nb, oset, bset)


def _check_theta(got, kernel, kp, Nd, Nb, oset, bset, nugget_type, tag):
    Xd, Xb, op, bc, p, T, mag = _case(kernel, kp, Nd, Nb, oset, bset)
    nug = np.diag(HO.nugget_diag(p, Nd, Nb, op, bc, NUGGET, nugget_type)).astype(LD)
    err = np.abs(got.astype(LD) - (T + nug))
    ratio = float(np.max(err / (EPS * (mag + nug))))
    WORST[tag] = max(WORST.get(tag, 0.0), ratio)
    print(f'\n[{tag} {kernel} ({Nd},{Nb}) {oset} {bset} {nugget_type}] max |dev - ref| / (eps (mag + nugget)) = {ratio:.2f}')
    assert np.all(err <= C_ENTRY * EPS * (mag + nug)), (kernel, Nd, Nb, oset, bset, nugget_type, ratio)


@pytest.mark.parametrize('bset', HO.BC_SETS)
@pytest.mark.parametrize('oset', HO.OP_SETS)
@pytest.mark.parametrize('Nd,Nb', HO.SHAPES)
@pytest.mark.parametrize('kernel,kp', HR.KERNELS)
def test_theta_entrywise(ctx, kernel, kp, Nd, Nb, oset, bset):
    Xd, Xb, op, bc, p, _, _ = _case(kernel, kp, Nd, Nb, oset, bset)
    N = 2 * Nd + Nb
    analytic = HO.trace_ratio(p, Nd, Nb, op, bc, LD)
    for nugget_type in ('none', 'identity', 'adaptive'):
        T, ratio = ctx.assemble_op(kernel, kp, Xd, Xb, op, bc, NUGGET, nugget_type)
        assert (T.rows, T.cols) == (N, N)
        got = T.download()
        T.free()
        _check_theta(got, kernel, kp, Nd, Nb, oset, bset, nugget_type, 'theta')
        assert abs(LD(ratio) - analytic) <= 4 * EPS * analytic, (ratio, float(analytic))
    if oset == 'random':                                                  # a Gram matrix of linear functionals: positive semi-definite
        assert np.linalg.eigvalsh(got)[0] >= -C_ENTRY * EPS * N * float(np.max(np.abs(got)))
    print(f'[theta] worst ratio so far {WORST["theta"]:.2f} of {C_ENTRY}')


@pytest.mark.parametrize('bset', HO.BC_SETS)
@pytest.mark.parametrize('Nd,Nb', HO.SHAPES)
@pytest.mark.parametrize('kernel,kp', HR.KERNELS)
def test_null_and_laplacian_rows_against_gpk_assemble_bc(ctx, kernel, kp, Nd, Nb, bset):
    Xd, Xb, op, bc, p, _, mag = _case(kernel, kp, Nd, Nb, 'laplace', bset)
    assert np.array_equal(op, np.tile(HO.LAPLACE, (Nd, 1)))
    for nugget_type in ('none', 'adaptive'):
        Tb, rb = ctx.assemble_bc(kernel, kp, Xd, Xb, bc, NUGGET, nugget_type)
        Tn, rn = ctx.assemble_op(kernel, kp, Xd, Xb, None, bc, NUGGET, nugget_type)
        Te, re_ = ctx.assemble_op(kernel, kp, Xd, Xb, op, bc, NUGGET, nugget_type)
        b, n, e = Tb.download(), Tn.download(), Te.download()
        for t in (Tb, Tn, Te):
            t.free()
        assert np.array_equal(n, e) and rn == re_                         # NULL and explicit (0,0,0,1,0,1): the same bits
        nug = np.diag(HO.nugget_diag(p, Nd, Nb, op, bc, NUGGET, nugget_type))
        scale = EPS * (mag.astype(np.float64) + nug)
        print(f'\n[laplace {kernel} ({Nd},{Nb}) {bset} {nugget_type}] bit-identical to gpk_assemble_bc: {np.array_equal(n, b)}; '
              f'max |op - bc| / (eps (mag + nugget)) = {float(np.max(np.abs(n - b) / scale)):.2f}')
        assert np.all(np.abs(n - b) <= C_ENTRY * scale)
        assert abs(rn - rb) <= 4 * EPS * rn
        _check_theta(n, kernel, kp, Nd, Nb, 'laplace', bset, nugget_type, 'null')


def test_paired_nontemporal_and_single_point_variants_agree(ctx):
    """the same even-sized problem through the 16-byte-store kernel, its non-temporal form (gpk_tune key 55) and the one-point kernel
    (key 47 = 0): the same per-pair arithmetic, so the same bits"""
    kernel, kp = HR.KERNELS[1]
    Xd, Xb, op, bc, _, _, _ = _case(kernel, kp, 256, 96, 'random', 'mixed')
    outs = []
    try:
        for key, val in ((47, 1), (55, 1), (47, 0)):
            ctx.tune(key, val)
            T, _ = ctx.assemble_op(kernel, kp, Xd, Xb, op, bc, NUGGET, 'adaptive')
            outs.append(T.download()); T.free()
    finally:
        ctx.tune(47, 1); ctx.tune(55, 0)
    _check_theta(outs[1], kernel, kp, 256, 96, 'random', 'mixed', 'adaptive', 'nt')
    _check_theta(outs[2], kernel, kp, 256, 96, 'random', 'mixed', 'adaptive', 'single')
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])


@pytest.mark.parametrize('Nd,Nb', [(37, 17), (256, 96)])
@pytest.mark.parametrize('kernel,kp', HR.KERNELS)
def test_theta_into_unaligned_view_between_canaries(ctx, kernel, kp, Nd, Nb):
    """every alignment class of the arena: only 'A' (16-byte aligned base, even leading dimension) may take the two-point path on the even
    sizes; 'B', 'C' and 'D' must each send it to the one-point kernel"""
    from gpk.device import KERNEL, NUGGET as NUG, kernel_params
    Xd, Xb, op, bc, p, _, _ = _case(kernel, kp, Nd, Nb, 'advdiff', 'mixed')
    N = 2 * Nd + Nb
    dXd, dXb, dop, dbc = ctx.points(Xd), ctx.points(Xb), ctx._domain_coeffs(op, Nd), ctx._boundary_coeffs(bc, Nb)
    for cls in VA.CLASSES:
        v = VA.class_view(ctx, N, N, cls)
        assert v.cls == cls
        ratio = C.c_double()
        rc = ctx.lib.gpk_assemble_op(ctx.h, KERNEL[kernel], kernel_params(kernel, kp), dXd.ptr, Nd, dXb.ptr, Nb, dop.ptr, dbc.ptr, NUGGET,
                                     NUG['adaptive'], v.ptr, v.ld, C.byref(ratio))
        assert rc == 0
        ctx.synchronize()
        v.arena.assert_outside_untouched([v])
        _check_theta(v.arena.get(v), kernel, kp, Nd, Nb, 'advdiff', 'mixed', 'adaptive', 'view')
        v.arena.free()


# ---- gpk_extend_functionals_op -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _extend_case(Nt, oset, bset):
    """test points (one coincident), a coefficient vector over 4 decades, the full-mask device rows and the longdouble rows"""
    kernel, kp = HR.KERNELS[1]
    Nd, Nb = 300, 150                                                     # 450 column points: two strides of the 256 lanes
    Xd, Xb, op, bc, p, _, _ = _case(kernel, kp, Nd, Nb, oset, bset)
    rng = np.random.RandomState(Nt)
    Xt = rng.uniform(0, 1, (Nt, 2))
    Xt[0] = Xd[3]                                                         # a coincident point
    coeff = rng.normal(size=2 * Nd + Nb) * 10.0 ** rng.uniform(0, 4, 2 * Nd + Nb)
    ref, terms, _ = HO.extend_rows(HO.NAMES, Xt, Xd, Xb, op, bc, coeff, p, dtype=LD)
    return kernel, kp, Xd, Xb, op, bc, Xt, coeff, ref, terms


@pytest.mark.parametrize('oset,bset', [('advdiff', 'mixed'), ('random', None)])
@pytest.mark.parametrize('which', [('value',), ('value', 'd1', 'd2'), HO.NAMES])
@pytest.mark.parametrize('Nt', (1, 5, 257))
def test_extend_functionals_op(ctx, Nt, which, oset, bset):
    kernel, kp, Xd, Xb, op, bc, Xt, coeff, ref, terms = _extend_case(Nt, oset, bset)
    got = ctx.extend_functionals_op(kernel, kp, Xt, Xd, Xb, op, bc, coeff, which=which).download().reshape(len(which), Nt)
    for k, n in enumerate(which):
        err = np.abs(got[k].astype(LD) - ref[n])
        ratio = float(np.max(err / (EPS * terms[n])))
        WORST['extend'] = max(WORST.get('extend', 0.0), ratio)
        print(f'\n[extend_op {oset} {bset} Nt={Nt} {n}] max |dev - ref| / (eps sum|terms|) = {ratio:.2f}')
        assert np.all(err <= C_EXTEND * EPS * terms[n]), (n, ratio)
    again = ctx.extend_functionals_op(kernel, kp, Xt, Xd, Xb, op, bc, coeff, which=which).download().reshape(len(which), Nt)
    assert np.array_equal(got, again)                                     # fixed reduction order: bit-identical


def test_single_bit_masks_agree_with_the_full_mask(ctx):
    kernel, kp, Xd, Xb, op, bc, Xt, coeff, ref, terms = _extend_case(5, 'advdiff', 'mixed')
    full = ctx.extend_functionals_op(kernel, kp, Xt, Xd, Xb, op, bc, coeff, which=HO.NAMES).download().reshape(6, -1)
    for k, n in enumerate(HO.NAMES):
        one = ctx.extend_functionals_op(kernel, kp, Xt, Xd, Xb, op, bc, coeff, which=(n,)).download().reshape(-1)
        print(f'\n[extend_op single {n}] bit-identical to the row of the full mask: {np.array_equal(one, full[k])}')
        assert np.all(np.abs(one - full[k]) <= 2 * C_EXTEND * EPS * terms[n].astype(np.float64)), n
        assert np.all(np.abs(one.astype(LD) - ref[n]) <= C_EXTEND * EPS * terms[n]), n
    # the caller's order of the rows
    r = ctx.extend_functionals_op(kernel, kp, Xt, Xd, Xb, op, bc, coeff, which=('d22', 'value')).download().reshape(2, -1)
    assert np.array_equal(r[0], full[5]) and np.array_equal(r[1], full[0])


def test_rejected_arguments(ctx):
    from gpk.device import kernel_params
    rng = np.random.RandomState(0)
    Xd, Xb, Xt = rng.uniform(0, 1, (20, 2)), HR.face_points(rng, 6), rng.uniform(0, 1, (8, 2))
    dXt, dXd, dXb, dc = ctx.points(Xt), ctx.points(Xd), ctx.points(Xb), ctx.array(rng.normal(size=46))
    dop = ctx._domain_coeffs(HO.op_set('random', Xd, rng), 20)
    dbc = ctx._boundary_coeffs(HR.coeff_set('robin', Xb), 6)
    out = ctx.empty(6, 8, ld=8)
    T = ctx.empty(46, 46)
    kp = kernel_params('Gaussian', 0.2)
    ext = lambda mask, Nt=8, ldo=8, Nd=20, Nb=6, kernel=0: ctx.lib.gpk_extend_functionals_op(
        ctx.h, kernel, kp, dXt.ptr, Nt, dXd.ptr, Nd, dXb.ptr, Nb, dop.ptr, dbc.ptr, dc.ptr, mask, out.ptr, ldo)
    assert ext(63) == 0 and ext(1) == 0 and ext(32) == 0
    for bad in (dict(mask=0), dict(mask=64), dict(mask=-1), dict(mask=1, Nt=0), dict(mask=1, ldo=7), dict(mask=1, Nd=0),
                dict(mask=1, Nb=-1), dict(mask=1, kernel=2)):
        assert ext(**bad) == -9001, bad
        assert b'extend_functionals_op' in ctx.lib.gpk_last_error(ctx.h), bad
    asm = lambda Nd=20, Nb=6, ld=T.ld, nt=2, kernel=0: ctx.lib.gpk_assemble_op(ctx.h, kernel, kp, dXd.ptr, Nd, dXb.ptr, Nb, dop.ptr, dbc.ptr,
                                                                               1e-3, nt, T.ptr, ld, None)
    assert asm() == 0                                                     # (host_ratio may be NULL)
    for bad in (dict(Nd=0), dict(Nb=-1), dict(ld=45), dict(nt=3), dict(kernel=2)):
        assert asm(**bad) == -9001, bad
        assert b'assemble_op' in ctx.lib.gpk_last_error(ctx.h), bad
    ctx.synchronize()


# ---- the other evaluators on the same handle -------------------------------------------------------------------------------------
def test_other_evaluators_are_unaffected_by_op_calls(ctx):
    """the point scratch is shared and re-packed per call (11 arrays here, 5, 2 and 3 there): every other call gives the bits it gave
    before an _op call came in between, and the other way round"""
    kernel, kp = HR.KERNELS[1]
    Xdo, Xbo, opo, bco, _, _, _ = _case(kernel, kp, 300, 150, 'random', 'mixed')
    rng = np.random.RandomState(9)
    Nd, Nb = 37, 17
    Xd, Xb, Xt = rng.uniform(0, 1, (Nd, 2)), rng.uniform(0, 1, (Nb, 2)), rng.uniform(0, 1, (11, 2))
    c = rng.normal(size=2 * Nd + Nb)
    bcs = rng.uniform(-3, 3, (Nb, 3))
    kernel3, kp3 = H3.KERNELS[0]
    Xd3, Xb3, Xt3 = rng.uniform(0, 1, (Nd, 3)), rng.uniform(0, 1, (Nb, 3)), rng.uniform(0, 1, (11, 3))

    def dl(T):
        a = T.download(); T.free()
        return a
    others = [lambda: dl(ctx.assemble('Nonlinear_elliptic', kernel, kp, Xd, Xb, 1e-3, 'adaptive')[0]),
              lambda: ctx.extend('Nonlinear_elliptic', kernel, kp, Xt, Xd, Xb, c).download(),
              lambda: dl(ctx.assemble3d(kernel3, kp3, Xd3, Xb3, 1e-3, 'adaptive')[0]),
              lambda: ctx.extend_functionals3d(kernel3, kp3, Xt3, Xd3, Xb3, c).download(),
              lambda: dl(ctx.assemble_bc(kernel, kp, Xd, Xb, bcs, 1e-3, 'adaptive')[0])]
    op_call = lambda: dl(ctx.assemble_op(kernel, kp, Xdo, Xbo, opo, bco, 1e-3, 'adaptive')[0])
    coeffo = rng.normal(size=750)
    ext_call = lambda: ctx.extend_functionals_op(kernel, kp, Xt, Xdo, Xbo, opo, bco, coeffo).download()
    before = [f() for f in others]
    first, first_ext = op_call(), ext_call()
    for k, f in enumerate(others):
        (op_call if k % 2 == 0 else ext_call)()
        assert np.array_equal(f(), before[k]), k
    assert np.array_equal(op_call(), first) and np.array_equal(ext_call(), first_ext)
    _check_theta(first, kernel, kp, 300, 150, 'random', 'mixed', 'adaptive', 'interleaved')


def test_assembly_timing_covers_the_op_launch(ctx):
    kernel, kp = HR.KERNELS[0]
    Xd, Xb, op, bc, _, _, _ = _case(kernel, kp, 300, 150, 'advdiff', 'mixed')
    ctx.prof_enable(True)
    try:
        T, _ = ctx.assemble_op(kernel, kp, Xd, Xb, op, bc, 1e-3, 'adaptive'); T.free()
        ms = ctx.prof_read_assembly()
    finally:
        ctx.prof_enable(False)
    assert ms > 0.0, ms


# ---- end to end through the class API and the facade ---------------------------------------------------------------------------------
# SEED: of the sampler seeds 0..5 the one whose numpy pipeline is least sensitive (Robin is the more sensitive of the two solves: s_z between
# 1.0e-10 and 5.1e-10 and s_J between 3.8e-6 and 9.9e-6 over those seeds, both smallest at seed 4; Dirichlet: s_z 2.0e-11 .. 2.7e-11, s_J
# 5.5e-8 .. 2.5e-7) -- chosen from the numpy pipeline alone
ND, NB, SIGMA, NUGGET_E2E, STEPS, SEED, BETA = 400, 160, 0.2, 1e-8, 6, 4, 2.0


def _cfg(bc):
    class Cfg:
        alpha, m = 1.0, 3
        kernel, kernel_parameter, nugget, nugget_type = 'Gaussian', SIGMA, NUGGET_E2E, 'adaptive'
        GNsteps, step_size, initial_sol, print_hist = STEPS, 1, 'rdm', False
        operator = staticmethod(HO.adr_operator)
    Cfg.bc, Cfg.robin_beta = bc, BETA
    return Cfg()


@functools.lru_cache(maxsize=None)
def _solved(bc):
    """the class solve on the device and the numpy pipeline on the same points and initial guess, with the pipeline's own sensitivity"""
    from src.PDEs import Nonlinear_elliptic2d
    eqn = Nonlinear_elliptic2d(alpha=1.0, m=3, bdy=HR.bdy_for(bc, BETA), rhs=HO.rhs_for(1.0, 3), domain=np.array(HR.UNIT_SQUARE), bc=bc,
                               robin_beta=BETA, operator=HO.adr_operator)
    np.random.seed(SEED)
    eqn.sampled_pts(ND, NB, sampled_type='random')
    eqn.Gram_matrix(kernel='Gaussian', kernel_parameter=SIGMA, nugget=NUGGET_E2E, nugget_type='adaptive')
    eqn.Gram_Cholesky()
    eqn.GN_method(max_iter=STEPS, step_size=1, initial_sol='rdm', print_hist=False)
    p = HR.precisions('Gaussian', SIGMA)
    pipe = HO.NumpyPipeline(eqn.X_domain, eqn.X_boundary, eqn.domain_coeffs, eqn.boundary_coeffs, p, NUGGET_E2E, eqn.rhs_f, eqn.bdy_g)
    z, hist, L = pipe.run(eqn.init_sol, STEPS)
    s_z, s_J = pipe.sensitivity(eqn.init_sol, STEPS, z, hist)
    return dict(eqn=eqn, pipe=pipe, z=z, hist=hist, L=L, s_z=s_z, s_J=s_J, p=p)


@pytest.fixture(params=('dirichlet', 'robin'))
def solved(request, ctx):
    return dict(_solved(request.param), bc=request.param)


def test_end_to_end_against_the_numpy_pipeline(solved):
    """CPU trial of this configuration (numpy pipeline alone, the class's initial guess at seed 4): s_z = 2.0e-11 / 1.0e-10 and
    s_J = 1.2e-7 / 3.8e-6 (Dirichlet / Robin), cond Theta = 9.2e13, L2 error at the collocation points 5.8e-5 / 3.2e-4.  The loss of the
    converged iterates (2.8e4) is itself only known to s_J: "non-increasing" is asserted up to the loss gate 100 s_J (in that trial the
    numpy pipeline's own last losses go up and down by less than that)."""
    eqn, pipe, z, hist, s_z, s_J, bc = (solved[k] for k in ('eqn', 'pipe', 'z', 'hist', 's_z', 's_J', 'bc'))
    print(f'\n[{bc} e2e] s_z = {s_z:.3e}, s_J = {s_J:.3e}')
    assert 100 * s_z <= 1e-7 and 100 * s_J <= 1e-3, ('gate mis-set: the numpy pipeline itself is too sensitive', s_z, s_J)
    assert np.array_equal(eqn.domain_coeffs, np.stack(HO.adr_operator(*eqn.X_domain.T), axis=1))
    if bc == 'dirichlet':
        assert eqn.boundary_coeffs is None
    else:
        assert np.array_equal(eqn.boundary_coeffs, HR.operator_coeffs(bc, BETA, eqn.X_boundary))
    assert eqn.chol_info == 0
    assert eqn.step_info == [0] * STEPS
    want = float(HO.trace_ratio(solved['p'], ND, NB, eqn.domain_coeffs, eqn.boundary_coeffs, LD))
    assert abs(eqn.ratio - want) <= 4 * EPS * want, (eqn.ratio, want)
    dz = float(np.linalg.norm(eqn.sol_sampled_pts - z) / np.linalg.norm(z))
    dJ = float(np.max(np.abs(np.asarray(eqn.loss_hist) - hist) / hist))
    print(f'[{bc} e2e] |z_gpu - z_np| / |z_np| = {dz:.3e} (gate {100 * s_z:.3e}); max rel. loss difference = {dJ:.3e} (gate {100 * s_J:.3e})')
    assert len(eqn.loss_hist) == STEPS + 1
    assert dz <= 100 * s_z
    assert dJ <= 100 * s_J
    lh = np.asarray(eqn.loss_hist)
    assert np.all(np.diff(lh[1:]) <= 100 * s_J * lh[1:-1]), eqn.loss_hist  # non-increasing after the first step
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
    args = (eqn.X_domain, eqn.X_boundary, eqn.domain_coeffs, eqn.boundary_coeffs, c_np, p)
    # 200 fresh boundary points
    rng = np.random.RandomState(3)
    Xbt = HR.face_points(rng, 200)
    ct = HR.operator_coeffs(bc, BETA, Xbt)
    gt = HR.operator_value(ct, Xbt)
    ref, _, norms = HO.extend_rows(HO.NAMES[:3], Xbt, *args)
    r_np = ct[:, 0] * ref['value'] + ct[:, 1] * ref['d1'] + ct[:, 2] * ref['d2'] - gt
    r = eqn.boundary_residual(Xbt, ct, gt)
    assert r.shape == (200,) and r is eqn.bdy_residual
    scale = sum(float(np.max(np.abs(ct[:, k]))) * norms[n] for k, n in enumerate(HO.NAMES[:3]))
    err = float(np.linalg.norm(r - r_np))
    print(f'\n[{bc}] boundary residual: |dev - numpy| = {err:.3e}, gate {gate * scale * cn:.3e}; max |residual| = {np.max(np.abs(r)):.3e}')
    assert err <= gate * scale * cn
    # 500 interior points: r = -psi_t[u] + u^3 - f, psi_t[u] = sum_k coeffs_t[:, k] row_k; d(u^3) = 3 u^2 du
    Xt = rng.uniform(0.02, 0.98, (500, 2))
    kt = np.stack(HO.adr_operator(*Xt.T), axis=1)
    ref, _, norms = HO.extend_rows(HO.NAMES, Xt, *args)
    r_np = -sum(kt[:, k] * ref[n] for k, n in enumerate(HO.NAMES)) + ref['value'] ** 3 - HO.rhs_for(1.0, 3)(*Xt.T)
    r = eqn.PDE_residual(Xt)
    scale = sum(float(np.max(np.abs(kt[:, k]))) * norms[n] for k, n in enumerate(HO.NAMES)) + 3 * float(np.max(ref['value'] ** 2)) * norms['value']
    err = float(np.linalg.norm(r - r_np))
    print(f'[{bc}] PDE residual: |dev - numpy| = {err:.3e}, gate {gate * scale * cn:.3e}; max |residual| = {np.max(np.abs(r)):.3e}')
    assert err <= gate * scale * cn
    assert np.array_equal(eqn.PDE_residual(Xt, coeffs_t=kt), r)          # explicit coefficients at the test points: the same call
    # extend_sol and extend_derivatives go through the same entry point
    eqn.extend_sol(Xt)
    rows = eqn.extend_derivatives(Xt)
    assert tuple(rows) == ('value', 'd1', 'd2', 'laplacian', 'd11', 'd12', 'd22') and np.array_equal(rows['value'], eqn.extended_sol)
    assert np.array_equal(rows['laplacian'], rows['d11'] + rows['d22'])
    for n in HO.NAMES:
        assert float(np.linalg.norm(rows[n] - ref[n])) <= gate * norms[n] * cn, n


def test_facade_gives_the_class_result_bitwise(solved):
    from src.solver import solver_GP
    bc = solved['bc']
    s = solver_GP(_cfg(bc), 'Nonlinear_elliptic')
    s.set_equation(bdy=HR.bdy_for(bc, BETA), rhs=HO.rhs_for(1.0, 3), domain=np.array(HR.UNIT_SQUARE), print_option=False)
    np.random.seed(SEED)
    s.auto_sample(ND, NB, sampled_type='random', print_option=False)
    s.solve(method='elimination', print_option=False)
    assert (s.eqn.bc, s.eqn.robin_beta) == (bc, BETA) and s.eqn.operator is HO.adr_operator
    assert np.array_equal(s.eqn.sol_sampled_pts, solved['eqn'].sol_sampled_pts)
    assert np.array_equal(np.asarray(s.eqn.loss_hist), np.asarray(solved['eqn'].loss_hist)) and s.eqn.ratio == solved['eqn'].ratio
    Xt = np.random.RandomState(4).uniform(0, 1, (64, 2))
    s.test(Xt, print_option=False)
    s.get_test_error(HR.truth(*Xt.T), print_option=False)
    s.test_residual(Xt, print_option=False)
    assert np.isfinite(s.test_L2_err) and np.isfinite(s.test_res_L2)
