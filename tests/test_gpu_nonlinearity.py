"""Reaction terms beyond alpha u^m on the device (gpk.h GPK_NL_*: exp, sinh, sin, cubic): the build kernels to rounding, one Gauss-Newton
step against long double, the structured and Gram modes, the power law untouched, the residual entry, whole solves against a float64
CPU chain, and the argument checks.  References, budgets and the CPU chain: tests/_nl_reference.py.

Sizes (N_d, N_b) = (37, 12): one partial 256-thread block, n_z + 1 no multiple of 16; (300, 68): a block boundary inside the domain range
and another inside the boundary range.  z is drawn from (-1.2, 1.2).

End to end (test_end_to_end_2d): the CPU chain alone, seed 0, 400 / 80 points, sigma 0.2, nugget 1e-8, 6 steps, gives
  Bratu ('exp', -1, 1)             loss 7.2e10 -> 7020.846, L2 error at the collocation points 9.77e-5, on the 20 x 20 grid 2.48e-4
  Poisson-Boltzmann ('sinh', 4, 1) loss 7.5e10 -> 7019.950, 9.56e-5, 2.50e-4
  Allen-Cahn ('cubic', -4, 0, 4)   loss 7.6e10 -> 7016.747, 9.57e-5, 2.52e-4
(the loss falls in every step until it is flat to 9 digits from step 4 on); the device may be at most twice as far from u*.
Inherited classes (test_inherited_classes): parabolic Allen-Cahn on 216 / 152 random space-time points, seed 1 of 0..2 (the smallest final
loss of the CPU chain: 5.1e9 -> 11.1 in 4 steps, L2 error 5.7e-4); advection-diffusion with Robin data and sin, seed 0: 8.0e10 -> 7278.74."""
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

import _gn_reference as R  # noqa: E402
import _nl_reference as NL  # noqa: E402
import _staircase_model as M  # noqa: E402
from oracle import gp_oracle as O  # noqa: E402
from test_gpu_gn_rounding import _check_step, _note, _upload_factor  # noqa: E402

LD, EPS = R.LD, R.EPS
WORST = {}
BUILD_CASES = [(k, s, Nd, Nb) for k in NL.KINDS for s in ('elliptic', 'relaxed') for Nd, Nb in NL.SIZES]
STEP_CASES = [(k, s, Nd, Nb) for k in NL.KINDS for s in ('elliptic', 'relaxed') for Nd, Nb in NL.SIZES]


@pytest.fixture(scope='module')
def ctx():
    from src._runtime import get_context
    return get_context()


def _problem(ctx, cs, dinv=256, structured=False, **kw):
    import gpk
    L = _upload_factor(ctx, cs.L)
    args = dict(p0=cs.p0, p1=cs.p1, p2=cs.p2, nonlin=cs.nonlin)
    args.update(kw)
    prob = gpk.GNProblem(ctx, R.SYSTEM_NAME[cs.system], cs.Nd, cs.Nb, cs.f, cs.g, L, pen_lambda=cs.lam, dinv=dinv, structured=structured, **args)
    prob.keep.append(L)
    return prob


# ------------------------------------------------------------------------------------------------ 4. build parity to rounding
@pytest.mark.parametrize('kind,system,Nd,Nb', BUILD_CASES)
def test_build_values(dev_ctx, kind, system, Nd, Nb):
    """gpk_gn_build, gpk_gn_build_rev (un-permuted) and gpk_gn_measurement entry by entry against long double: zeros, constants and copies
    exact, every other entry within NL.build_budget(kind) eps of the magnitude sum of its terms"""
    ctx, cs = dev_ctx, NL.case(kind, system, Nd, Nb)
    lin = NL.linearise(cs, cs.z0)
    budget = NL.build_budget(kind)
    prob = _problem(ctx, cs)
    z = ctx.array(cs.z0)
    nz = cs.nz
    S = ctx.empty(prob.rows, nz + 1)
    ctx._chk(ctx.lib.gpk_gn_build(ctx.h, C.byref(prob.struct), z.ptr, S.ptr, S.ld))
    nat = S.download()
    worst = NL.check_build(lin, nat[:, :nz], nat[:, nz], budget, (kind, system, Nd, 'gpk_gn_build'))
    if system == 'elliptic':                          # (gpk_gn_build_rev refuses the relaxed system)
        col = M.column_of_unknown(system, Nd)
        S.upload(np.full((prob.rows, nz + 1), 3.25))
        ctx._chk(ctx.lib.gpk_gn_build_rev(ctx.h, C.byref(prob.struct), z.ptr, S.ptr, S.ld))
        rev = S.download()
        worst = max(worst, NL.check_build(lin, rev[:, col], rev[:, nz], budget, (kind, system, Nd, 'gpk_gn_build_rev')))
    worst = max(worst, NL.check_build(lin, None, ctx.gn_measurement(prob, z), budget, (kind, system, Nd, 'gpk_gn_measurement')))
    WORST[kind] = max(WORST.get(kind, 0.0), worst)
    print(f'\n[build {kind} {system} {Nd}] worst |dev - ld| / (eps sum|terms|) = {worst:.2f} of {budget:.2f}; worst of {kind} so far {WORST[kind]:.2f}')
    prob.free()


# ------------------------------------------------------------------------------------------------ 5. one Gauss-Newton step
@pytest.mark.parametrize('kind,Nd,Nb', [(k, Nd, Nb) for k in NL.KINDS for Nd, Nb in NL.SIZES])
def test_hessian_grad(dev_ctx, kind, Nd, Nb):
    """H and g of the elliptic system against long double: the gates of tests/test_gpu_gn_rounding.py (32 x the numpy pipeline + 1)"""
    ctx, cs = dev_ctx, NL.case(kind, 'elliptic', Nd, Nb)
    ref = NL.full_reference(kind, 'elliptic', Nd, Nb)
    prob = _problem(ctx, cs)
    H, g = ctx.gn_hessian_grad(prob, ctx.array(cs.z0))
    print()
    rH, aH = R.gate_H(ref, H)
    _note('nl H', rH, aH, f'{kind} {Nd} max |H - H_ld| / (eps 2|S|^T|S|)')
    rg, ag = R.gate_g(ref, g)
    _note('nl g', rg, ag, f'{kind} {Nd} max |g - g_ld| / (eps 2|S|^T|w|)')
    prob.free()
    assert np.array_equal(H, H.T), 'H is not exactly symmetric'
    assert rH <= aH and rg <= ag


def _one_step(ctx, cs, step=1.0, **kw):
    prob = _problem(ctx, cs, **kw)
    z = ctx.array(cs.z0)
    loss, info = ctx.gn_step(prob, z, step)
    out = (cs.z0.copy(), step, loss, info, prob.workspace()[2].download().copy(), z.download().copy())
    prob.free(); z.free()
    return out


@pytest.mark.parametrize('kind,system,Nd,Nb', STEP_CASES)
def test_step(dev_ctx, kind, system, Nd, Nb):
    """info, the in-step loss, delta backward and forward and the update of z: _check_step of tests/test_gpu_gn_rounding.py"""
    cs = NL.case(kind, system, Nd, Nb)
    ref = NL.vector_reference(kind, system, Nd, Nb)
    print()
    bad = _check_step('nl step', f'{kind} {system} {Nd}', ref, _one_step(dev_ctx, cs))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 6. structured and Gram modes
def _gram_case(kind, Nd=300, Nb=60, nugget=1e-9):
    """the first case of tests/test_gpu_structured.py::test_structured_step_matches_default_and_oracle with the reaction term `kind`"""
    rng = np.random.RandomState(Nd)
    Xd = rng.uniform(0, 1, (Nd, 2)); Xb = rng.uniform(0, 1, (Nb, 2))
    f = O.elliptic_rhs(Xd[:, 0], Xd[:, 1]); g = O.elliptic_truth(Xb[:, 0], Xb[:, 1])
    return Xd, Xb, f, g, rng.uniform(-1.2, 1.2, Nd), nugget


@pytest.mark.parametrize('kind', NL.KINDS)
def test_structured_and_gram_modes_match_the_default_path(kind):
    """three steps with structured = 1 and 2 against the per-step solve, at the bounds of tests/test_gpu_structured.py for the elliptic
    system (iterates 1e-9 / 1e-8, loss histories 1e-7 / 1e-6); exp has tau(0) = p0 in v0; with the switch off: the default path's bits"""
    import gpk
    ctx = gpk.Context(0)
    try:
        Xd, Xb, f, g, z0, nugget = _gram_case(kind)
        Nd, Nb = len(Xd), len(Xb)
        T, _ = ctx.assemble('Nonlinear_elliptic', 'Gaussian', 0.2, Xd, Xb, nugget, 'adaptive')
        assert ctx.potrf(T) == 0
        p0, p1, p2 = NL.PARAMS[kind]
        out = []
        for structured in (False, True, 2):
            prob = gpk.GNProblem(ctx, 'Nonlinear_elliptic', Nd, Nb, f, g, T, p0=p0, p1=p1, p2=p2, nonlin=kind, structured=structured)
            z = ctx.array(z0)
            hist = []
            for _ in range(3):
                loss, info = ctx.gn_step(prob, z, 1.0)
                assert info == 0
                hist.append(loss)
            hist.append(ctx.gn_loss(prob, z))
            out.append((z.download().ravel().copy(), np.array(hist)))
        (za, ha), (zb, hb), (zc, hc) = out
        rb, rc = np.linalg.norm(zb - za) / np.linalg.norm(za), np.linalg.norm(zc - za) / np.linalg.norm(za)
        print(f'\n[structured {kind}] iterates: structured {rb:.2e} (1e-9), Gram level {rc:.2e} (1e-8); losses {ha}')
        assert rb <= 1e-9 and rc <= 1e-8
        np.testing.assert_allclose(hb, ha, rtol=1e-7)
        np.testing.assert_allclose(hc, ha, rtol=1e-6)
        ctx.lib.gpk_debug_set(40, 0)
        try:
            z = ctx.array(z0)
            for _ in range(3):
                ctx.gn_step(prob, z, 1.0)
            assert np.array_equal(z.download().ravel(), za)
        finally:
            ctx.lib.gpk_debug_set(40, 1)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 7. kind 0 untouched
@pytest.mark.parametrize('system', ('elliptic', 'relaxed'))
def test_power_law_is_untouched(dev_ctx, system):
    """nonlin = 0 with a stray p2 has the bits of a problem built without the new arguments"""
    cs = R.case(system, 129)
    import gpk

    def run(**kw):
        L = _upload_factor(dev_ctx, cs.L)
        prob = gpk.GNProblem(dev_ctx, R.SYSTEM_NAME[system], cs.Nd, cs.Nb, cs.f, cs.g, L, p0=cs.p0, p1=cs.p1, pen_lambda=cs.lam, dinv=256, **kw)
        z = dev_ctx.array(cs.z0)
        loss, info = dev_ctx.gn_step(prob, z, 1.0)
        out = loss, info, z.download().copy(), dev_ctx.gn_measurement(prob, z)
        prob.free(); L.free(); z.free()
        return out
    a, b = run(), run(nonlin=0, p2=123.0)
    assert a[0] == b[0] and a[1] == b[1] == 0 and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


@pytest.mark.parametrize('Nd,Nb', NL.SIZES)
def test_cubic_reproduces_the_power_law(dev_ctx, Nd, Nb):
    """('cubic', 0, 0, 1) against alpha = 1, m = 3: the step of the cubic passes the gates against the long-double reference of u^3"""
    cs = NL.NLCase('cubic', 'elliptic', Nd, Nb, params=(0.0, 0.0, 1.0))
    pw = NL.NLCase('power', 'elliptic', Nd, Nb, params=(1.0, 3.0, 0.0))
    ref = NL.VectorReference(pw, pw.z0)
    print()
    bad = _check_step('nl cubic=power', f'{Nd}', ref, _one_step(dev_ctx, cs))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 8. residual
@pytest.mark.parametrize('kind', ('power',) + NL.KINDS)
def test_residual_kernel_matches_numpy(ctx, kind):
    """gpk_pde_residual_nl against long double: <= 4 eps of |u3| + sum |terms of tau| + |f|, N_t = 300 (a second, partial block)"""
    rng = np.random.RandomState(11)
    Nt = 300
    U = rng.normal(size=(4, Nt)) * 10.0 ** rng.uniform(-2, 2, (4, Nt))
    U[0] = rng.uniform(-1.2, 1.2, Nt) if kind != 'power' else rng.uniform(0.05, 1.2, Nt)
    f = rng.normal(size=Nt) * 10.0 ** rng.uniform(-2, 2, Nt)
    params = (1.3, 3.0, 0.0) if kind == 'power' else NL.PARAMS[kind]
    got = ctx.pde_residual_nl(kind, params, U, f).download().ravel()
    t, tm = NL.tau_ld(kind, params, U[0])
    ref = -U[3].astype(LD) + t - f.astype(LD)
    mag = np.abs(U[3]).astype(LD) + tm + np.abs(f).astype(LD)
    ratio = float(np.max(np.abs(got.astype(LD) - ref) / (LD(EPS) * mag)))
    print(f'\n[residual {kind}] max |dev - ld| / (eps sum|terms|) = {ratio:.2f} of 4')
    assert ratio <= 4
    if kind == 'power':                                                  # kind 0 = the numbers of gpk_pde_residual
        assert np.array_equal(got, ctx.pde_residual('Nonlinear_elliptic', params, U, None, f).download().ravel())


def test_collocation_identity_with_sinh_and_robin(ctx):
    """PDE_residual at the domain collocation points after a real solve with ('sinh', 2, 1) and bc = 'robin'.  Theta_lambda coeff =
    sol_vec, so the rows of the extension there are Delta u = sol_vec[:N_d] - n0 c[:N_d] and u = z - n1 c[N_d:2 N_d], and the residual is
    -(tau(z) - f - n0 c0) + tau(z - n1 c1) - f.  Bound as in tests/test_gpu_extend_functionals.py: 64 eps sum|terms| of the kernel sums
    (|Theta| |c|) plus the Cholesky solve's (3n + 1) eps |L| |L^T| |c|, the u-row's share multiplied by |tau'|."""
    from src.PDEs import Nonlinear_elliptic2d
    import main_NonLinElliptic2d as drv
    from src.nonlinearity import Nonlinearity
    tau = Nonlinearity('sinh', 2.0, 1.0)
    u, f = drv.manufactured(tau)
    e = Nonlinear_elliptic2d(bdy=drv.boundary_data(u, 'robin', 1.0), rhs=f, domain=np.array(drv.UNIT_SQUARE), bc='robin', robin_beta=1.0,
                             nonlinearity=('sinh', 2.0, 1.0))
    np.random.seed(0)
    e.sampled_pts(400, 80)
    nugget = 1e-8
    e.Gram_matrix(kernel='Gaussian', kernel_parameter=0.2, nugget=nugget, nugget_type='adaptive')
    e.Gram_Cholesky()
    e.GN_method(max_iter=6, print_hist=False)
    Nd, N = 400, 880
    r = e.PDE_residual(e.X_domain)
    c = e._coeff(e._dL, e.sol_vec).download().ravel()
    Lh = e.L
    Tl = e.Theta
    n0, n1 = nugget * e.ratio, nugget
    z = e.sol_sampled_pts
    want = -(tau.tau(z) - e.rhs_f - n0 * c[:Nd]) + tau.tau(z - n1 * c[Nd:2 * Nd]) - e.rhs_f
    terms = np.abs(Tl) @ np.abs(c)
    chol = np.abs(Lh) @ (np.abs(Lh).T @ np.abs(c))
    row = 64 * EPS * terms + (3 * N + 1) * EPS * chol
    bound = row[:Nd] + np.abs(tau.dtau(z)) * row[Nd:2 * Nd] + 8 * EPS * (np.abs(tau.tau(z)) + np.abs(e.rhs_f) + np.abs(e.sol_vec[:Nd]))
    worst = float(np.max(np.abs(r - want) / bound))
    print(f'\n[collocation identity sinh/robin] max |r - expected| / bound = {worst:.3e}; max |r| = {np.max(np.abs(r)):.3e}')
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ 9. end to end in two dimensions
E2E = {'bratu': ('exp', -1.0, 1.0), 'poisson_boltzmann': ('sinh', 4.0, 1.0), 'allen_cahn': ('cubic', -4.0, 0.0, 4.0)}


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


@pytest.mark.parametrize('name', sorted(E2E))
def test_end_to_end_2d(ctx, name):
    """solver_GP on the device against the CPU chain (oracle Theta -> numpy.linalg.cholesky -> the same Gauss-Newton loop in float64) on the
    same points and start: iterate, extension on a 20 x 20 grid and loss history within the parity bound 1e-6; the L2 errors against u* at
    most twice the CPU chain's own"""
    import main_NonLinElliptic2d as drv
    from _driver_common import tensor_grid
    from src.nonlinearity import Nonlinearity
    from src.solver import solver_GP
    spec = E2E[name]
    tau = Nonlinearity.make(spec)
    u, f = drv.manufactured(tau)

    class Cfg:
        alpha, m = 1.0, 3.0
        kernel, kernel_parameter, nugget, nugget_type = 'Gaussian', 0.2, 1e-8, 'adaptive'
        GNsteps, step_size, initial_sol, print_hist = 6, 1, 'rdm', False
        nonlinearity = spec
    np.random.seed(0)
    s = solver_GP(Cfg(), PDE_type='Nonlinear_elliptic')
    s.set_equation(bdy=u, rhs=f, domain=np.array(drv.UNIT_SQUARE), print_option=False)
    s.auto_sample(400, 80, print_option=False)
    e = s.eqn
    Xd, Xb = e.X_domain, e.X_boundary
    # the CPU chain first: it needs the points and the start only (the start is drawn here exactly as GN_method draws it)
    state = np.random.get_state()
    z0 = np.random.normal(0.0, 1.0, 400)
    np.random.set_state(state)
    Theta = O.add_nugget(O.gram_matrix_assembly(Xd, Xb, 'Nonlinear_elliptic', 'Gaussian', 0.2), 'Nonlinear_elliptic', 400, 80, 1e-8)[0]
    zc, hc, L, sv = NL.cpu_chain(Theta, tau, e.rhs_f, e.bdy_g, z0, 6)
    assert np.all(np.diff(hc) <= 1e-6 * hc[:-1]) and hc[-1] < 1e-6 * hc[0], ('the CPU chain does not converge', hc)
    Xt = tensor_grid(20, *drv.UNIT_SQUARE)[2]
    ext_c = NL.extend_cpu(L, O.construct_theta_test(Xt, Xd, Xb, 'Nonlinear_elliptic', 'Gaussian', 0.2), sv)
    s.solve(print_option=False)
    assert np.array_equal(e.init_sol, z0)
    s.test(Xt, print_option=False)
    ut, ud = u(Xt[:, 0], Xt[:, 1]), u(Xd[:, 0], Xd[:, 1])
    l2 = lambda a, b: float(np.sqrt(np.mean((a - b) ** 2)))
    figs = dict(z=_rel(e.sol_sampled_pts, zc), ext=_rel(e.extended_sol, ext_c), hist=float(np.max(np.abs(np.array(e.loss_hist) - hc) / hc)),
                l2_pts=(l2(e.sol_sampled_pts, ud), l2(zc, ud)), l2_grid=(l2(e.extended_sol, ut), l2(ext_c, ut)))
    print(f'\n[e2e {name}] {figs}; CPU losses {hc}')
    assert figs['z'] <= 1e-6 and figs['ext'] <= 1e-6 and figs['hist'] <= 1e-6
    assert figs['l2_pts'][0] <= 2 * figs['l2_pts'][1] and figs['l2_grid'][0] <= 2 * figs['l2_grid'][1]


# ------------------------------------------------------------------------------------------------ 10. inherited classes
def test_inherited_parabolic_allen_cahn(ctx):
    """Nonlinear_elliptic3d(operator=parabolic_form(0.2), nonlinearity=('cubic', -1, 0, 1)) on 216 / 152 space-time points, 4 steps"""
    import main_NonLinElliptic3d as d3
    import test_elliptic3d_host as H3
    import test_operator3d_host as H3O
    from src.PDEs import Nonlinear_elliptic3d, parabolic_form
    from src.nonlinearity import Nonlinearity
    tau = Nonlinearity('cubic', -1.0, 0.0, 1.0)
    u, f = d3.parabolic_manufactured(tau, 0.2)
    rng = np.random.RandomState(1)
    Xd = rng.uniform(0, 1, (216, 3)); Xb = NL.space_time_boundary(rng, 152)
    z0 = rng.normal(size=216)
    e = Nonlinear_elliptic3d(bdy=u, rhs=f, operator=parabolic_form(0.2), nonlinearity=('cubic', -1, 0, 1))
    e.get_sampled_points(Xd, Xb)
    p = H3.precisions('Gaussian', 0.3)
    Theta = H3O.theta(Xd, Xb, e.domain_coeffs, None, p)[0] + np.diag(H3O.nugget_diag(p, 216, 152, e.domain_coeffs, None, 1e-8, 'adaptive'))
    zc, hc, _, _ = NL.cpu_chain(Theta, tau, e.rhs_f, e.bdy_g, z0, 4)
    e.Gram_matrix(kernel='Gaussian', kernel_parameter=0.3, nugget=1e-8, nugget_type='adaptive')
    e.Gram_Cholesky()
    e._initial = lambda initial_sol, n: z0.copy()
    e.GN_method(max_iter=4, print_hist=False)
    rel = _rel(e.sol_sampled_pts, zc)
    print(f'\n[inherited parabolic cubic] iterate vs CPU chain {rel:.2e}; losses {e.loss_hist}; CPU {hc}')
    assert np.all(np.diff(e.loss_hist) < 0) and np.all(np.diff(hc) < 0)
    assert rel <= 1e-6


def test_inherited_advection_diffusion_robin_sin(ctx):
    """Nonlinear_elliptic2d(operator=advection_diffusion, bc='robin', nonlinearity=('sin', 1, 2)) at 400 / 80, 6 steps"""
    import main_NonLinElliptic2d as d2
    import test_operator_host as HO
    import test_robin_host as HR
    from src.PDEs import Nonlinear_elliptic2d
    from src.nonlinearity import Nonlinearity
    tau = Nonlinearity('sin', 1.0, 2.0)
    u, _ = d2.manufactured(tau)
    e = Nonlinear_elliptic2d(bdy=d2.boundary_data(u, 'robin', 1.0), rhs=d2.manufactured_operator_rhs(tau), domain=np.array(d2.UNIT_SQUARE),
                             bc='robin', robin_beta=1.0, operator=d2.advection_diffusion, nonlinearity=('sin', 1, 2))
    np.random.seed(0)
    e.sampled_pts(400, 80)
    state = np.random.get_state()
    z0 = np.random.normal(0.0, 1.0, 400)
    np.random.set_state(state)
    p = HR.precisions('Gaussian', 0.2)
    Theta = (HO.theta(e.X_domain, e.X_boundary, e.domain_coeffs, e.boundary_coeffs, p)[0]
             + np.diag(HO.nugget_diag(p, 400, 80, e.domain_coeffs, e.boundary_coeffs, 1e-8, 'adaptive')))
    zc, hc, _, _ = NL.cpu_chain(Theta, tau, e.rhs_f, e.bdy_g, z0, 6)
    e.Gram_matrix(kernel='Gaussian', kernel_parameter=0.2, nugget=1e-8, nugget_type='adaptive')
    e.Gram_Cholesky()
    e.GN_method(max_iter=6, print_hist=False)
    assert np.array_equal(e.init_sol, z0)
    rel = _rel(e.sol_sampled_pts, zc)
    print(f'\n[inherited advdiff robin sin] iterate vs CPU chain {rel:.2e}; losses {e.loss_hist}; CPU {hc}')
    assert np.all(np.diff(e.loss_hist) <= 1e-6 * np.array(e.loss_hist[:-1])) and e.loss_hist[-1] < 1e-6 * e.loss_hist[0]
    assert rel <= 1e-6


# ------------------------------------------------------------------------------------------------ 11. argument errors
def test_argument_errors(ctx):
    """nonlin = 7, nonlin = 2 on the Burgers system and gpk_pde_residual_nl with nonlin = -1: a negative return code with text in
    gpk_last_error, a GpkError from the class layer, and nothing launched (the outputs keep their canary)"""
    import gpk
    cs = NL.case('sinh', 'elliptic', 37, 12)
    L = _upload_factor(ctx, cs.L)
    z = ctx.array(cs.z0)
    prob = gpk.GNProblem(ctx, 'Nonlinear_elliptic', cs.Nd, cs.Nb, cs.f, cs.g, L, p0=1.0, p1=1.0, nonlin=2, dinv=False)
    S, H, delta, work = prob.workspace()
    canary = np.full((prob.rows, prob.nz + 1), 7.5)
    for what, mutate in (('nonlin = 7', lambda s: setattr(s, 'nonlin', 7)), ('Burgers', lambda s: setattr(s, 'system', gpk.SYSTEM['Burgers']))):
        bl = None
        if what == 'Burgers':                                           # (the Burgers factor has order 4 N_d + N_b)
            bl = ctx.empty(4 * cs.Nd + cs.Nb, 4 * cs.Nd + cs.Nb)
            prob.struct.L, prob.struct.ldl = bl.ptr, bl.ld
        mutate(prob.struct)
        S.upload(canary)
        loss, info = C.c_double(), C.c_int()
        calls = {
            'gpk_gn_step': lambda: ctx.lib.gpk_gn_step(ctx.h, C.byref(prob.struct), z.ptr, 1.0, S.ptr, S.ld, H.ptr, H.ld, delta.ptr, C.byref(loss), C.byref(info)),
            'gpk_gn_loss': lambda: ctx.lib.gpk_gn_loss(ctx.h, C.byref(prob.struct), z.ptr, work.ptr, C.byref(loss)),
            'gpk_gn_build': lambda: ctx.lib.gpk_gn_build(ctx.h, C.byref(prob.struct), z.ptr, S.ptr, S.ld),
            'gpk_gn_measurement': lambda: ctx.lib.gpk_gn_measurement(ctx.h, C.byref(prob.struct), z.ptr, work.ptr),
        }
        for name, call in calls.items():
            rc = call()
            assert rc == -9001, (what, name, rc)
            assert b'nonlin' in ctx.lib.gpk_last_error(ctx.h), (what, name, ctx.lib.gpk_last_error(ctx.h))
        with pytest.raises(gpk.GpkError):
            ctx.gn_step(prob, z)
        ctx.synchronize()
        assert np.array_equal(S.download(), canary) and np.array_equal(z.download().ravel(), cs.z0), (what, 'something was launched')
        prob.struct.nonlin, prob.struct.system = 2, gpk.SYSTEM['Nonlinear_elliptic']
        prob.struct.L, prob.struct.ldl = L.ptr, L.ld
        if bl is not None:
            bl.free()
    U = ctx.array(np.ones((4, 300)))
    f = ctx.array(np.ones(300))
    out = ctx.array(np.full(300, 7.5))
    p = (C.c_double * 3)(1.0, 1.0, 0.0)
    for bad in (-1, 5):
        rc = ctx.lib.gpk_pde_residual_nl(ctx.h, bad, p, 300, U.ptr, U.ld, f.ptr, out.ptr)
        assert rc == -9001 and b'nonlin' in ctx.lib.gpk_last_error(ctx.h)
    with pytest.raises(gpk.GpkError):
        ctx.pde_residual_nl(-1, (1.0, 1.0, 0.0), np.ones((4, 300)), np.ones(300))
    ctx.synchronize()
    assert np.array_equal(out.download().ravel(), np.full(300, 7.5))
    assert ctx.gn_step(prob, z)[1] == 0                               # the handle is still usable
    prob.free(); L.free()
