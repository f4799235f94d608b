"""The 3-D elliptic path on the device: gpk_assemble3d entry by entry (both store variants, unaligned views between canaries),
gpk_extend_functionals3d, the class API end to end against a numpy pipeline with a measured sensitivity, and no interference with
the 2-D calls that share the handle's point scratch.  The expectation lives in test_elliptic3d_host.py."""
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
import test_extend_functionals_host as H2  # noqa: E402

EPS = H3.EPS
LD = H3.LD
# Rounding budget of one entry relative to T = sum of |terms| x kappa (u = eps / 2 per rounding; the expectation is longdouble, so all
# of it is the device's):
#   exp argument  -(p1 d1^2 + p2 d2^2 + p3 d3^2)/2: positive terms, 2 products + at most 2 additions each -> relative error <= 4 u of
#                 the argument = 2 eps |arg|, which the exponential turns into a RELATIVE error 2 eps |arg| of kappa;
#                 |arg| <= 3 max p / 2 on the unit cube = 33.4 for the anisotropic kernel (p = 2 / 0.3^2 = 22.2)       <= 67 eps
#   the exponential itself (1 ulp), the product with kappa (1 u), the nugget addition (1 u)                               <=  2 eps
#   a Hermite factor: at most 6 roundings (q, q^2, the bracket, two products, the last addition); three factors and the two
#                 products joining them 3 x 6 + 2 = 20 u                                                               <= 10 eps
#   the sum of up to nine terms, 8 additions                                                                             <=  4 eps
# together <= 83 eps T.  T does not see a cancellation INSIDE one Hermite factor (h2 near p d^2 = 1, where |h2| is small but its
# rounding error stays ~eps p); an entry is exposed only where all the factors of all its terms are small at once, and the factor 1.5
# left between 83 and C covers h2 down to a few percent of p on every axis simultaneously.
C_ENTRY = 128
# the extension adds the product with the coefficient (1 u) and the sum over the columns: per lane 2 terms per column point, then 6
# shuffle steps and 2 LDS additions -- under 16 u = 8 eps of sum|terms| for the sizes here: the same constant holds
C_EXTEND = 128
SHAPES = [(1, 0), (37, 17), (256, 96), (300, 150)]
WORST = {}


@pytest.fixture(scope='module')
def ctx():
    from src._runtime import get_context
    return get_context()


@functools.lru_cache(maxsize=None)
def _case(kernel, kp, Nd, Nb):
    """points and the longdouble expectation (Theta without nugget, sum of |terms|), computed once per (kernel, shape)"""
    rng = np.random.RandomState(1000 * Nd + Nb)
    Xd = rng.uniform(0, 1, (Nd, 3)); Xb = rng.uniform(0, 1, (Nb, 3))
    p = H3.precisions(kernel, kp)
    T, mag = H3.theta(Xd, Xb, p, dtype=LD)
    return Xd, Xb, p, T, mag


def _check_theta(got, kernel, kp, Nd, Nb, nugget, nugget_type, tag):
    Xd, Xb, p, T, mag = _case(kernel, kp, Nd, Nb)
    nug = H3.nugget_diag(p, Nd, Nb, nugget, nugget_type)
    want = T + np.diag(nug.astype(LD))
    bound = C_ENTRY * EPS * (mag + np.diag(nug).astype(LD))
    err = np.abs(got.astype(LD) - want)
    ratio = float(np.max(err / (EPS * (mag + np.diag(nug).astype(LD)))))
    WORST[tag] = max(WORST.get(tag, 0.0), ratio)
    print(f'\n[{tag} {kernel} ({Nd},{Nb}) {nugget_type}] max |dev - ref| / (eps T) = {ratio:.2f}')
    assert np.all(err <= bound), (kernel, Nd, Nb, nugget_type, ratio)


@pytest.mark.parametrize('nugget_type', ('none', 'identity', 'adaptive'))
@pytest.mark.parametrize('Nd,Nb', SHAPES)
@pytest.mark.parametrize('kernel,kp', H3.KERNELS)
def test_theta_entrywise(ctx, kernel, kp, Nd, Nb, nugget_type):
    Xd, Xb, p, _, _ = _case(kernel, kp, Nd, Nb)
    nugget = 1e-3                                                       # large enough to be visible in every diagonal entry
    T, ratio = ctx.assemble3d(kernel, kp, Xd, Xb, nugget, nugget_type)
    N = 2 * Nd + Nb
    assert (T.rows, T.cols) == (N, N)
    got = T.download()
    T.free()
    _check_theta(got, kernel, kp, Nd, Nb, nugget, nugget_type, 'theta')
    pl = [LD(v) for v in p]
    analytic = LD(Nd) * (3 * sum(v * v for v in pl) + 2 * (pl[0] * pl[1] + pl[0] * pl[2] + pl[1] * pl[2])) / LD(Nd + Nb)
    assert abs(LD(ratio) - analytic) <= 4 * EPS * analytic, (ratio, float(analytic))


@pytest.mark.parametrize('Nd,Nb', [(37, 17), (256, 96)])
@pytest.mark.parametrize('kernel,kp', H3.KERNELS)
def test_theta_into_unaligned_view_between_canaries(ctx, kernel, kp, Nd, Nb):
    """odd leading dimension and a base that is 8- but not 16-byte aligned: the one-point path also on even sizes"""
    Xd, Xb, p, _, _ = _case(kernel, kp, Nd, Nb)
    N = 2 * Nd + Nb
    v = VA.class_view(ctx, N, N, 'D')
    assert v.cls == 'D' and v.ld % 2 == 1 and v.ptr % 16 == 8
    dXd, dXb = ctx.points(Xd, 3), ctx.points(Xb, 3)
    from gpk.device import KERNEL, NUGGET, kernel_params3d
    ratio = C.c_double()
    rc = ctx.lib.gpk_assemble3d(ctx.h, KERNEL[kernel], kernel_params3d(kernel, kp), dXd.ptr, Nd, dXb.ptr, Nb, 1e-3, NUGGET['adaptive'],
                                v.ptr, v.ld, C.byref(ratio))
    assert rc == 0
    ctx.synchronize()
    v.arena.assert_outside_untouched([v])
    _check_theta(v.arena.get(v), kernel, kp, Nd, Nb, 1e-3, 'adaptive', 'view')
    v.arena.free()


def test_paired_and_single_point_variants_agree(ctx):
    """the same even-sized problem through the 16-byte-store kernel, its non-temporal form (gpk_tune key 55) and the one-point kernel
    (key 47 = 0): the same per-pair arithmetic, so the same bits"""
    kernel, kp = H3.KERNELS[1]
    Xd, Xb, _, _, _ = _case(kernel, kp, 256, 96)
    outs = []
    try:
        for key, val in ((47, 1), (55, 1), (47, 0)):
            ctx.tune(key, val)
            T, _ = ctx.assemble3d(kernel, kp, Xd, Xb, 1e-3, 'adaptive')
            outs.append(T.download()); T.free()
    finally:
        ctx.tune(47, 1); ctx.tune(55, 0)
    _check_theta(outs[1], kernel, kp, 256, 96, 1e-3, 'adaptive', 'nt')
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])


# ---- gpk_extend_functionals3d ----------------------------------------------------------------------------------------------------
ALL5 = ('value', 'd1', 'd2', 'laplacian', 'd3')                           # ascending bit order


@pytest.mark.parametrize('which', [('value',), ('laplacian',), ALL5, ('d3', 'value', 'laplacian', 'd1')])
@pytest.mark.parametrize('Nt', (1, 5, 130))
def test_extend_functionals3d(ctx, Nt, which):
    kernel, kp = H3.KERNELS[1]
    Nd, Nb = 300, 150                                                     # 450 column points: two strides of the 256 lanes
    Xd, Xb, p, _, _ = _case(kernel, kp, Nd, Nb)
    rng = np.random.RandomState(Nt)
    Xt = rng.uniform(0, 1, (Nt, 3))
    Xt[0] = Xd[3]                                                         # a coincident point
    coeff = rng.normal(size=2 * Nd + Nb) * 10.0 ** rng.uniform(0, 4, 2 * Nd + Nb)
    got = ctx.extend_functionals3d(kernel, kp, Xt, Xd, Xb, coeff, which=which).download().reshape(len(which), Nt)
    ref, terms, _ = H3.extend_rows(which, Xt, Xd, Xb, coeff, p, dtype=LD)
    for k, n in enumerate(which):
        err = np.abs(got[k].astype(LD) - ref[n])
        ratio = float(np.max(err / (EPS * terms[n])))
        WORST['extend'] = max(WORST.get('extend', 0.0), ratio)
        print(f'\n[extend3d Nt={Nt} {n}] max |dev - ref| / (eps sum|terms|) = {ratio:.2f}')
        assert np.all(err <= C_EXTEND * EPS * terms[n]), (n, ratio)
    again = ctx.extend_functionals3d(kernel, kp, Xt, Xd, Xb, coeff, which=which).download().reshape(len(which), Nt)
    assert np.array_equal(got, again)                                     # fixed reduction order: bit-identical


def test_extend_functionals3d_rejects_other_bits(ctx):
    from gpk.device import kernel_params3d
    rng = np.random.RandomState(0)
    Xd, Xb, Xt = rng.uniform(0, 1, (20, 3)), rng.uniform(0, 1, (6, 3)), rng.uniform(0, 1, (8, 3))
    dXt, dXd, dXb, dc = ctx.points(Xt, 3), ctx.points(Xd, 3), ctx.points(Xb, 3), ctx.array(rng.normal(size=46))
    out = ctx.empty(6, 8, ld=8)
    call = lambda mask, Nt=8, ldo=8: ctx.lib.gpk_extend_functionals3d(ctx.h, 0, kernel_params3d('Gaussian', 0.3), dXt.ptr, Nt, dXd.ptr, 20,
                                                                      dXb.ptr, 6, dc.ptr, mask, out.ptr, ldo)
    assert call(1 | 2 | 4 | 16 | 32) == 0
    assert call(8) == -9001 and call(1 | 8) == -9001                      # GPK_FN_D2D2 has no meaning here
    assert call(64) == -9001 and call(0) == -9001
    assert call(1, Nt=0) == -9001 and call(1, ldo=7) == -9001
    assert b'extend_functionals3d' in ctx.lib.gpk_last_error(ctx.h)
    ctx.synchronize()


# ---- end to end through the class API -----------------------------------------------------------------------------------------------
ND, NB, SIGMA, NUGGET_E2E, STEPS, SEED = 400, 216, 0.3, 1e-8, 6, 1


class _Cfg:
    alpha, m = 1.0, 3
    kernel, kernel_parameter, nugget, nugget_type = 'Gaussian', SIGMA, NUGGET_E2E, 'adaptive'
    GNsteps, step_size, initial_sol, print_hist = STEPS, 1, 'rdm', False


@pytest.fixture(scope='module')
def solved(ctx):
    """the class solve on the device and the numpy pipeline on the same points and initial guess, with the pipeline's own sensitivity"""
    from src.PDEs import Nonlinear_elliptic3d
    eqn = Nonlinear_elliptic3d(alpha=1.0, m=3, bdy=H3.truth, rhs=H3.rhs_for(1.0, 3), domain=np.array(H3.UNIT_CUBE))
    np.random.seed(SEED)
    eqn.sampled_pts(ND, NB, sampled_type='random')
    eqn.Gram_matrix(kernel='Gaussian', kernel_parameter=SIGMA, nugget=NUGGET_E2E, nugget_type='adaptive')
    eqn.Gram_Cholesky()
    eqn.GN_method(max_iter=STEPS, step_size=1, initial_sol='rdm', print_hist=False)
    p = H3.precisions('Gaussian', SIGMA)
    pipe = H3.NumpyPipeline(eqn.X_domain, eqn.X_boundary, p, NUGGET_E2E, eqn.rhs_f, eqn.bdy_g)
    z, hist, L = pipe.run(eqn.init_sol, STEPS)
    s_z, s_J = pipe.sensitivity(eqn.init_sol, STEPS, z, hist)
    return dict(eqn=eqn, pipe=pipe, z=z, hist=hist, L=L, s_z=s_z, s_J=s_J, p=p)


def test_end_to_end_against_the_numpy_pipeline(solved):
    eqn, z, hist, s_z, s_J = (solved[k] for k in ('eqn', 'z', 'hist', 's_z', 's_J'))
    print(f'\n[3d e2e] s_z = {s_z:.3e}, s_J = {s_J:.3e}')
    assert 100 * s_z <= 1e-7 and 100 * s_J <= 1e-4, ('gate mis-set: the numpy pipeline itself is too sensitive', s_z, s_J)
    assert eqn.chol_info == 0
    assert eqn.step_info == [0] * STEPS
    dz = float(np.linalg.norm(eqn.sol_sampled_pts - z) / np.linalg.norm(z))
    dJ = float(np.max(np.abs(np.asarray(eqn.loss_hist) - hist) / hist))
    print(f'[3d e2e] |z_gpu - z_np| / |z_np| = {dz:.3e} (gate {100 * s_z:.3e}); max rel. loss difference = {dJ:.3e} (gate {100 * s_J:.3e})')
    assert len(eqn.loss_hist) == STEPS + 1
    assert dz <= 100 * s_z
    assert dJ <= 100 * s_J
    u = H3.truth(*eqn.X_domain.T)
    err_np = float(np.sqrt(np.mean((z - u) ** 2)))
    err_gpu = float(np.sqrt(np.mean((eqn.sol_sampled_pts - u) ** 2)))
    print(f'[3d e2e] L2 error at the collocation points: device {err_gpu:.3e}, numpy {err_np:.3e}')
    assert err_gpu <= 2 * err_np


def test_extension_derivatives_and_residual_of_the_solution(solved):
    from scipy.linalg import cho_solve
    eqn, pipe, z, p = solved['eqn'], solved['pipe'], solved['z'], solved['p']
    rng = np.random.RandomState(3)
    Xt = rng.uniform(0.02, 0.98, (500, 3))
    c_np = cho_solve((solved['L'], True), pipe.measurement(z))          # Theta^{-1} sol_vec, sol_vec = [alpha z^m - f; z; g] = F(z)
    names = ('value', 'd1', 'd2', 'd3', 'laplacian')
    ref, _, norms = H3.extend_rows(names, Xt, eqn.X_domain, eqn.X_boundary, c_np, p)
    gate = max(100 * solved['s_z'], 1e-9)
    eqn.extend_sol(Xt)
    rows = eqn.extend_derivatives(Xt)
    assert tuple(rows) == names
    cn = float(np.linalg.norm(c_np))
    for n in names:
        err = float(np.linalg.norm(rows[n] - ref[n]))
        print(f'\n[3d extension] {n}: |dev - numpy| = {err:.3e}, gate {gate * norms[n] * cn:.3e}')
        assert err <= gate * norms[n] * cn, n
    assert float(np.linalg.norm(eqn.extended_sol - ref['value'])) <= gate * norms['value'] * cn
    # the residual kernel on the device's own rows
    r = eqn.PDE_residual(Xt)
    f = H3.rhs_for(1.0, 3)(*Xt.T)
    t = [-rows['laplacian'], rows['value'] ** 3, -f]
    assert np.all(np.abs(r - sum(t)) <= 8 * EPS * sum(np.abs(x) for x in t))
    # a wrong axis would show here: d3 of the manufactured solution against its analytic value, next to d1
    pi = np.pi
    e1 = float(np.linalg.norm(rows['d1'] - pi * np.cos(pi * Xt[:, 0]) * np.sin(pi * Xt[:, 1]) * np.sin(pi * Xt[:, 2])))
    e3 = float(np.linalg.norm(rows['d3'] - pi * np.cos(pi * Xt[:, 2]) * np.sin(pi * Xt[:, 0]) * np.sin(pi * Xt[:, 1])))
    print(f'[3d extension] d1 error {e1:.3e}, d3 error {e3:.3e}')
    assert e3 <= 2 * e1


def test_facade_gives_the_same_solution_bitwise(solved):
    from src.solver import solver_GP
    s = solver_GP(_Cfg(), 'Nonlinear_elliptic3d')
    s.set_equation(bdy=H3.truth, rhs=H3.rhs_for(1.0, 3), domain=np.array(H3.UNIT_CUBE), print_option=False)
    np.random.seed(SEED)
    s.auto_sample(ND, NB, sampled_type='random', print_option=False)
    s.solve(method='elimination', print_option=False)
    assert np.array_equal(s.eqn.sol_sampled_pts, solved['eqn'].sol_sampled_pts)
    s.collocation_pts_err(H3.truth(*s.eqn.X_domain.T), print_option=False)
    Xt = np.random.RandomState(4).uniform(0, 1, (64, 3))
    s.test(Xt, print_option=False)
    s.get_test_error(H3.truth(*Xt.T), print_option=False)
    s.test_residual(Xt, print_option=False)
    assert s.pts_L2_err < 2e-4 and s.test_L2_err < 1e-3 and np.isfinite(s.test_res_L2)
    with pytest.raises(NotImplementedError):
        s.contour_of_test_err(None, None)


# ---- the 2-D calls on the same handle ------------------------------------------------------------------------------------------------
def test_2d_calls_are_unaffected_by_a_3d_assemble(ctx):
    """the point scratch is shared and re-packed per call: a 2-D assemble and a 2-D extend right after a 3-D assemble"""
    kernel3, kp3 = H3.KERNELS[0]
    Xd3, Xb3, _, _, _ = _case(kernel3, kp3, 300, 150)
    T3, _ = ctx.assemble3d(kernel3, kp3, Xd3, Xb3, 1e-3, 'adaptive'); T3.free()
    rng = np.random.RandomState(9)
    Nd, Nb = 37, 17
    Xd, Xb, Xt = rng.uniform(0, 1, (Nd, 2)), rng.uniform(0, 1, (Nb, 2)), rng.uniform(0, 1, (11, 2))
    kernel, kp = H2.KERNELS[0]
    T, _ = ctx.assemble('Nonlinear_elliptic', kernel, kp, Xd, Xb, 0.0, 'none')
    got = T.download(); T.free()
    Xa = np.concatenate([Xd, Xb])
    parts = [[H2.pair('laplacian', 'laplacian', Xd, Xd, kernel, kp), H2.pair('laplacian', 'value', Xd, Xa, kernel, kp)],
             [H2.pair('value', 'laplacian', Xa, Xd, kernel, kp), H2.pair('value', 'value', Xa, Xa, kernel, kp)]]
    want = np.block([[q[0] for q in row] for row in parts]); mag = np.block([[q[1] for q in row] for row in parts])
    assert np.all(np.abs(got - want) <= 64 * EPS * mag)
    T3, _ = ctx.assemble3d(kernel3, kp3, Xd3, Xb3, 1e-3, 'adaptive'); T3.free()
    c = rng.normal(size=2 * Nd + Nb)
    ext = ctx.extend('Nonlinear_elliptic', kernel, kp, Xt, Xd, Xb, c).download()
    ref, terms = H2.expect('Nonlinear_elliptic', 'value', Xt, Xd, Xb, c, kernel, kp)
    assert np.all(np.abs(ext - ref) <= 64 * EPS * terms)


def test_assembly_timing_covers_the_3d_launch(ctx):
    kernel, kp = H3.KERNELS[0]
    Xd, Xb, _, _, _ = _case(kernel, kp, 300, 150)
    ctx.prof_enable(True)
    try:
        T, _ = ctx.assemble3d(kernel, kp, Xd, Xb, 1e-3, 'adaptive'); T.free()
        ms = ctx.prof_read_assembly()
    finally:
        ctx.prof_enable(False)
    assert 0.0 < ms < 100.0, ms
