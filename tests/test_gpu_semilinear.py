"""The semilinear system GPK_GN_SEMILINEAR and the class Semilinear2d on the device, against tests/_semilinear_reference.py.

a-c run on the synthetic, well-conditioned factors of tests/_gn_reference.py (poisoned upper triangle and padding) with
gq = (0.7, -0.4, 0.3, 0.5, 0.2), eps = 0.1 -- every entry of A(z) live, dN/du != 0 -- at (N_d, N_b) = (65, 13), (129, 3), (333, 17).
  a. gpk_gn_build / gpk_gn_build_rev into an unaligned view surrounded by canaries: copies and constants exact, computed entries within
     4 ulp (eps x the magnitude sum of the entry's terms: _semilinear_reference.C_BUILD), nothing outside the view touched.
  b. gpk_gn_step, gpk_gn_hessian_grad, gpk_gn_loss with the inverted diagonal blocks (GEMM-only path) and without: delta, the updated z,
     g, H and the loss within 8 x max(error of the float64 pipeline, eps x rounding scale) of the long-double values.  The library
     takes inverted blocks of 256, 512, 1024 or 2048 rows only (a block of 64 rows is refused with -9001), so the two block sizes are
     256 and, where the factor is larger than one such block, 512.  A profile that skips the entries N_u / eps (Eikonal's two-segment
     profile) misses every gate by more than 1e6 (tests/test_semilinear_host.py shows it on the CPU).
  c. with gq = (0, 0, 1, 0, 0) and f^2 in place of f the step agrees with GPK_GN_EIKONAL's on the same factor under the bound of b.
  d. Semilinear2d end to end on the device Gram matrix against the float64 reference iteration.   e. extension rows and PDE residual.
  f. posterior variance / covariance / samples and log evidence.   g. refusals.   h. the driver.
Every test prints what it measures."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _semilinear_reference as SL
import _staircase_model as M
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD, EPS = SL.LD, SL.EPS


def _upload_factor(ctx, L):
    n = L.shape[0]
    d = ctx.empty(n, n + SL.R.LD_PAD, ld=n + SL.R.LD_PAD)
    d.upload(SL.poisoned(L))
    d.cols = n
    return d


def _problem(ctx, cs, dinv=256, system='Semilinear2d', f=None):
    import gpk
    L = _upload_factor(ctx, cs.L)
    prob = gpk.GNProblem(ctx, system, cs.Nd, cs.Nb, cs.f if f is None else f, cs.g, L, p0=cs.eps, dinv=dinv,
                         gq=cs.gq if system == 'Semilinear2d' else None)
    prob.keep.append(L)
    return prob


def _report(tag, res):
    bad = []
    for name, (r, a) in res.items():
        print(f'[semilinear {tag}] {name}: device {r / EPS:.3g} eps, allowed {a / EPS:.3g} eps, ratio to the bound {r / a:.3g}')
        if not r <= a:
            bad.append((name, r, a))
    return bad


# ------------------------------------------------------------------------------------------------ a. the build kernels
@pytest.mark.parametrize('Nd', SL.SIZES)
def test_build_values_and_canaries(dev_ctx, Nd):
    ctx, cs = dev_ctx, SL.case(Nd)
    lin = SL.linearise(cs, cs.z0)
    prob = _problem(ctx, cs, dinv=False)
    z = ctx.array(cs.z0)
    nz, rows = cs.nz, cs.rows
    assert (prob.nz, prob.rows) == (nz, rows)
    r0, c0, ld = 2, 3, nz + 1 + 9                                      # an unaligned view inside a larger buffer
    col = M.column_of_unknown('eikonal', Nd)                           # the staircase order of the step: v1, v2, v0
    print()
    for name, fn in (('gpk_gn_build', ctx.lib.gpk_gn_build), ('gpk_gn_build_rev', ctx.lib.gpk_gn_build_rev)):
        buf = ctx.empty(rows + 4, ld, ld=ld)
        canary = np.full((rows + 4, ld), 3.25)
        buf.upload(canary)
        ctx._chk(fn(ctx.h, C.byref(prob.struct), z.ptr, buf.at(r0, c0), ld))
        ctx.synchronize()
        got = buf.download()
        view = got[r0:r0 + rows, c0:c0 + nz + 1].copy()
        got[r0:r0 + rows, c0:c0 + nz + 1] = 3.25
        # (the S buffer is cleared as rows of lds doubles: the padding right of the view inside those rows belongs to the call)
        inside = np.zeros_like(got, dtype=bool)
        flat = inside.reshape(-1)
        flat[r0 * ld + c0:r0 * ld + c0 + rows * ld] = True
        assert np.array_equal(got[~inside], canary[~inside]), f'{name} wrote outside its S buffer'
        A = view[:, :nz] if name == 'gpk_gn_build' else view[:, col]
        worst = SL.check_build(lin, A, view[:, nz], (name, Nd))
        print(f'[semilinear build] {name} N_d {Nd}: worst |dev - ld| / (eps sum|terms|) = {worst:.2f} of {SL.C_BUILD}')
        if name == 'gpk_gn_build_rev':                                 # the promised leading zeros: the closed form, lead = n_z, slope 1
            first = M.first_nonzero_rows(view[:, :nz])
            assert np.all(first >= nz - 1 - np.arange(nz)) and np.array_equal(first[:Nd], nz - 1 - np.arange(Nd))
        buf.free()
    assert SL.check_build(lin, lin.dense(np.float64), ctx.gn_measurement(prob, z), ('gpk_gn_measurement', Nd)) <= SL.C_BUILD
    prob.free()


# ------------------------------------------------------------------------------------------------ b. step, Hessian, gradient, loss
FORMS = [(Nd, dinv) for Nd in SL.SIZES for dinv in ((256, False) if Nd < 333 else (256, 512, False))]


@pytest.mark.parametrize('Nd,dinv', FORMS)
def test_step_hessian_grad_loss(dev_ctx, Nd, dinv):
    ctx, cs = dev_ctx, SL.case(Nd)
    ref = SL.full_reference(Nd)
    prob = _problem(ctx, cs, dinv=dinv)
    z = ctx.array(cs.z0)
    H, g = ctx.gn_hessian_grad(prob, z)
    loss = ctx.gn_loss(prob, z)
    step_loss, info = ctx.gn_step(prob, z, 1.0)
    delta, z_out = prob.workspace()[2].download().copy(), z.download().copy()
    prob.free()
    print(f'\n[semilinear step] N_d {Nd} dinv {dinv}: cond(H) {ref.cond:.3g}')
    assert info == 0 and np.array_equal(H, H.T)
    bad = _report(f'N_d {Nd} dinv {dinv}', SL.gates(ref, H=H, g=g, loss=loss, delta=delta, z_out=z_out))
    bad += _report(f'N_d {Nd} dinv {dinv} in-step', SL.gates(ref, loss=step_loss))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ c. the Eikonal special case
@pytest.mark.parametrize('Nd', SL.SIZES)
def test_eikonal_special_case_agrees_with_the_eikonal_system(dev_ctx, Nd):
    ctx, cs0 = dev_ctx, SL.case(Nd)
    cs = SL.Case(cs0.Nd, cs0.Nb, gq=(0, 0, 1, 0, 0), eps=0.1, like=cs0)
    ref = SL.FullReference(cs, cs.z0, f=cs.f ** 2)
    out = {}
    for system, f in (('Semilinear2d', cs.f ** 2), ('Eikonal', cs.f)):
        prob = _problem(ctx, cs, dinv=256, system=system, f=f)
        z = ctx.array(cs.z0)
        loss, info = ctx.gn_step(prob, z, 1.0)
        out[system] = (loss, info, prob.workspace()[2].download().copy(), z.download().copy())
        prob.free()
    (ls, i_s, ds, zs), (le, ie, de, ze) = out['Semilinear2d'], out['Eikonal']
    assert i_s == 0 and ie == 0
    print()
    # both against the long-double step of this problem, then against each other: each within the bound of b, so twice that apart
    bad = _report(f'special case N_d {Nd} semilinear', SL.gates(ref, loss=ls, delta=ds, z_out=zs))
    bad += _report(f'special case N_d {Nd} eikonal', SL.gates(ref, loss=le, delta=de, z_out=ze))
    assert not bad, bad
    scale_d = float(np.max(np.abs(ref.delta.astype(np.float64))))
    p64 = float(np.max(SL.err(ref.p64.delta, ref.delta))) / scale_d
    diff = float(np.max(np.abs(ds - de))) / scale_d
    allowed = 2 * SL.MARGIN * max(p64, EPS)
    print(f'[semilinear special case] N_d {Nd}: max |delta_sl - delta_eik| / max |delta| = {diff / EPS:.3g} eps, allowed {allowed / EPS:.3g} eps')
    assert diff <= allowed and abs(ls - le) <= 2 * SL.MARGIN * EPS * abs(le)


# ------------------------------------------------------------------------------------------------ d. end to end through the class
def _solve_class(gq, eps, kernel='Gaussian', kp=0.2, Nd=300, Nb=80, nugget=1e-6, steps=8):
    from src.PDEs import Semilinear2d
    Xd, Xb = SL.points(Nd, Nb)
    e = Semilinear2d(eps=eps, nonlinearity=gq, bdy=SL.truth, rhs=lambda x1, x2: SL.manufactured_rhs(eps, gq, x1, x2))
    e.get_sampled_points(Xd, Xb)
    e.Gram_matrix(kernel=kernel, kernel_parameter=kp, nugget=nugget, nugget_type='adaptive')
    e.Gram_Cholesky()
    assert e.chol_info == 0
    e.GN_method(max_iter=steps, step_size=1, initial_sol='zero', print_hist=False)
    if kernel == 'Gaussian':
        T, _ = O.add_nugget(O.gram_matrix_assembly(Xd, Xb, 'Eikonal', kernel, kp), 'Eikonal', Nd, Nb, nugget)
    else:
        # the numpy oracle has the Gaussian family only, and the long-double Matern assembly of tests/_matern_reference.py takes half a
        # minute at this size: the reference iteration runs on the device's own Gram matrix (judged entry by entry in
        # tests/test_gpu_matern.py), factored by LAPACK -- the Gauss-Newton system is what this case is about
        T = e.Theta
    L = O.cholesky(T)
    sysm = SL.System(eps, gq, e.rhs_f, e.bdy_g)
    z_ref, hist = SL.gn_float64(sysm, L, np.zeros(3 * Nd), steps)
    return e, sysm, L, z_ref, hist


@pytest.mark.parametrize('gq,eps,kernel,kp', [((1.0, 1.0, 0.0, 0.0, 0.0), 0.1, 'Gaussian', 0.2), ((1.0, -1.0, 0.5, 1.0, 1.0), 0.2, 'Gaussian', 0.2),
                                              ((1.0, 1.0, 0.0, 0.0, 0.0), 0.1, 'Matern72', 0.5)])
def test_class_end_to_end(gq, eps, kernel, kp):
    e, sysm, L, z_ref, hist = _solve_class(gq, eps, kernel, kp)
    Nd = e.N_domain
    u_ref = z_ref[:Nd]
    rel = float(np.linalg.norm(e.sol_sampled_pts - u_ref) / np.linalg.norm(u_ref))
    us = SL.truth(e.X_domain[:, 0], e.X_domain[:, 1])
    l2_dev = float(np.sqrt(np.mean((e.sol_sampled_pts - us) ** 2)))
    l2_ref = float(np.sqrt(np.mean((u_ref - us) ** 2)))
    print(f'\n[semilinear class] {kernel} gq {gq} eps {eps}: parity {rel:.3g}, L2 error device {l2_dev:.3g}, reference {l2_ref:.3g}, '
          f'loss {e.loss_hist[-1]:.8g} / {hist[-1]:.8g}')
    assert all(i == 0 for i in e.step_info)
    assert rel <= 1e-6
    want = sysm.F(e._z_star[1])[0]                                     # sol_vec = F(z*): the host spells N in the device's order, the
    assert np.max(np.abs(e.sol_vec - want)) <= 1e-13 * np.max(np.abs(want))   # reference term by term -- equal to rounding, not to the bit
    if kernel == 'Gaussian':
        assert l2_dev <= 2 * l2_ref


# ------------------------------------------------------------------------------------------------ e. extension and residual
def test_extension_rows_and_residual(dev_ctx):
    gq, eps = (1.0, -1.0, 0.5, 1.0, 1.0), 0.2
    e, sysm, L, _, _ = _solve_class(gq, eps, Nd=150, Nb=40, steps=6)
    Xt = np.random.RandomState(5).uniform(0, 1, (37, 2))
    rows = e.extend_derivatives(Xt)
    Kt = O.construct_theta_test(Xt, e.X_domain, e.X_boundary, 'Eikonal', 'Gaussian', 0.2)
    Ld = e.L
    coeff = O._tri_solve(Ld, O._tri_solve(Ld, e.sol_vec), trans=True)
    e.extend_sol(Xt)
    want_u = Kt @ coeff
    print(f'\n[semilinear extend] max |value - numpy| = {np.max(np.abs(rows["value"] - want_u)):.3g}')
    scale = float(np.max(np.abs(Kt) @ np.abs(coeff)))
    assert np.max(np.abs(rows['value'] - want_u)) <= 1e-12 * scale and np.max(np.abs(e.extended_sol - want_u)) <= 1e-12 * scale
    res = e.PDE_residual(Xt)
    f_t = SL.manufactured_rhs(eps, gq, Xt[:, 0], Xt[:, 1])
    want = -eps * rows['laplacian'] + SL.N(gq, rows['value'], rows['d1'], rows['d2']) - f_t
    rscale = float(np.max(eps * np.abs(rows['laplacian']) + SL.N_mag(gq, rows['value'], rows['d1'], rows['d2']) + np.abs(f_t)))
    print(f'[semilinear residual] max |r| = {np.max(np.abs(res)):.3g}, max |r - numpy| = {np.max(np.abs(res - want)):.3g}, scale {rscale:.3g}')
    assert np.max(np.abs(res - want)) <= 1e-12 * rscale
    # the entry point itself: bit-repeatable, and on a fresh handle's buffers too
    ctx = dev_ctx
    fields = np.stack([rows[k] for k in ('value', 'd1', 'd2', 'laplacian')])
    a = ctx.pde_residual_sl(eps, gq, fields, f_t).download()
    b = ctx.pde_residual_sl(eps, gq, fields, f_t).download()
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)) and np.max(np.abs(a.ravel() - want)) <= 1e-12 * rscale


# ------------------------------------------------------------------------------------------------ f. posterior and evidence
def test_posterior_and_evidence():
    gq, eps = (1.0, -1.0, 0.5, 1.0, 1.0), 0.2
    e, sysm, _, _, _ = _solve_class(gq, eps, Nd=60, Nb=20, steps=6)
    Xt = np.random.RandomState(9).uniform(0, 1, (7, 2))
    z = e._z_star[1]
    T, _ = O.add_nugget(O.gram_matrix_assembly(e.X_domain, e.X_boundary, 'Eikonal', 'Gaussian', 0.2), 'Eikonal', 60, 20, 1e-6)
    L = O.cholesky(T)
    K = O.construct_theta_test(Xt, e.X_domain, e.X_boundary, 'Eikonal', 'Gaussian', 0.2).T
    d = Xt[:, None, :] - Xt[None, :, :]
    Ktt = np.exp(-np.sum(d * d, axis=2) / (2 * 0.2 ** 2))
    ref = SL.posterior_covariance(L, *SL.posterior_prepare(sysm, L, z, LD)[::2], K, Ktt, LD)
    P64, R64, G64 = SL.posterior_prepare(sysm, L, z, np.float64)
    np64 = SL.posterior_covariance(L, P64, G64, K, Ktt, np.float64)
    var = e.posterior_variance(Xt)
    cov = e.posterior_covariance(Xt)
    err_np = float(np.max(np.abs(np64[1].astype(LD) - ref[1])))
    vmin = float(np.min(np.diag(ref[1].astype(np.float64))))
    err_v = float(np.max(np.abs(var.astype(LD) - np.diag(ref[1]))))
    err_c = float(np.max(np.abs(cov.astype(LD) - ref[1])))
    print(f'\n[semilinear posterior] numpy error {err_np:.3g}, min var {vmin:.3g}; device variance {err_v:.3g}, covariance {err_c:.3g}, '
          f'allowed {32 * err_np:.3g}')
    assert err_np < 1e-3 * vmin, 'precondition: the gate could hide a wrong result'
    assert err_v <= 32 * err_np and err_c <= 32 * err_np               # tests/test_gpu_posterior.py, class API: MARGIN = 32 x numpy
    assert np.array_equal(cov, cov.T)
    s1 = e.posterior_sample(Xt, n_samples=3, seed=11).copy()
    s2 = e.posterior_sample(Xt, n_samples=3, seed=11)
    assert s1.shape == (3, 7) and np.array_equal(s1.view(np.uint64), s2.view(np.uint64))
    want = SL.log_evidence(sysm, L, z, R64)
    got = e.log_evidence()
    t = e.log_evidence_terms
    print(f'[semilinear evidence] log Z device {got:.12g}, numpy {want["log_Z"]:.12g}; J {t["J"]:.10g} / {want["J"]:.10g}')
    assert t['info'] == 0
    # |log Z| is a sum of the three terms below: cond(Theta) = 1e8-ish moves each by cond x eps relative; 1e-6 is the project's parity bound
    for k in ('J', 'logdet_theta', 'logdet_H', 'two_pi_term'):
        assert abs(t[k] - want[k]) <= 1e-6 * max(abs(want[k]), 1.0), (k, t[k], want[k])
    assert abs(got - want['log_Z']) <= 1e-6 * (abs(want['J']) + abs(want['logdet_theta']) + abs(want['logdet_H']))


# ------------------------------------------------------------------------------------------------ g. refusals
def test_refusals(dev_ctx):
    import gpk
    from src.PDEs import Semilinear2d
    ctx, cs = dev_ctx, SL.case(65)
    prob = _problem(ctx, cs, dinv=256)
    S, _, _, _ = prob.workspace()
    canary = np.full((prob.rows, prob.nz + 1), 5.5)
    S.upload(canary)
    z = ctx.array(cs.z0)
    W1, W2 = ctx.empty(prob.rows, prob.nz + 1, ld=S.ld), ctx.empty(prob.rows, prob.nz + 1, ld=S.ld)
    v0 = ctx.empty(prob.rows, 1)
    rc = ctx.lib.gpk_gn_structured_prepare(ctx.h, C.byref(prob.struct), S.ptr, S.ld, W1.ptr, W2.ptr, v0.ptr, S.ld)
    assert rc == -9001 and b'GPK_GN_SEMILINEAR' in ctx.lib.gpk_last_error(ctx.h)
    G, pv = ctx.empty(4 * prob.nz, prob.nz), ctx.empty(2 * prob.nz + 1, 1)
    rc = ctx.lib.gpk_gn_gram_prepare(ctx.h, C.byref(prob.struct), G.ptr, G.ld, pv.ptr)
    assert rc == -9001 and b'GPK_GN_SEMILINEAR' in ctx.lib.gpk_last_error(ctx.h)
    with pytest.raises(gpk.GpkError):
        prob.prepare_structured()
    for field, value, word in (('nonlin', 1, b'nonlin'), ('p0', 0.0, b'eps'), ('p0', float('nan'), b'eps'), ('p0', float('inf'), b'eps')):
        old = getattr(prob.struct, field)
        setattr(prob.struct, field, value)
        loss, info = C.c_double(), C.c_int()
        _, H, delta, work = prob.workspace()
        calls = {'step': lambda: ctx.lib.gpk_gn_step(ctx.h, C.byref(prob.struct), z.ptr, 1.0, S.ptr, S.ld, H.ptr, H.ld, delta.ptr, C.byref(loss), C.byref(info)),
                 'build': lambda: ctx.lib.gpk_gn_build(ctx.h, C.byref(prob.struct), z.ptr, S.ptr, S.ld),
                 'build_rev': lambda: ctx.lib.gpk_gn_build_rev(ctx.h, C.byref(prob.struct), z.ptr, S.ptr, S.ld),
                 'loss': lambda: ctx.lib.gpk_gn_loss(ctx.h, C.byref(prob.struct), z.ptr, work.ptr, C.byref(loss)),
                 'hessian': lambda: ctx.lib.gpk_gn_hessian_grad(ctx.h, C.byref(prob.struct), z.ptr, S.ptr, S.ld, H.ptr, H.ld, None),
                 'measurement': lambda: ctx.lib.gpk_gn_measurement(ctx.h, C.byref(prob.struct), z.ptr, work.ptr)}
        for name, call in calls.items():
            rc = call()
            assert rc == -9001 and word in ctx.lib.gpk_last_error(ctx.h), (field, value, name, rc, ctx.lib.gpk_last_error(ctx.h))
        setattr(prob.struct, field, old)
    ctx.synchronize()
    assert np.array_equal(S.download(), canary) and np.array_equal(z.download().ravel(), cs.z0), 'something was launched'
    U, f, out = ctx.array(np.ones((4, 30))), ctx.array(np.ones(30)), ctx.array(np.full(30, 7.5))
    gq = (C.c_double * 5)(*cs.gq)
    for bad in (0.0, float('nan')):
        rc = ctx.lib.gpk_pde_residual_sl(ctx.h, bad, gq, 30, U.ptr, U.ld, f.ptr, out.ptr)
        assert rc == -9001 and b'eps' in ctx.lib.gpk_last_error(ctx.h)
    assert ctx.lib.gpk_pde_residual_sl(ctx.h, 0.1, None, 30, U.ptr, U.ld, f.ptr, out.ptr) == -9001
    assert ctx.lib.gpk_pde_residual_sl(ctx.h, 0.1, gq, 30, U.ptr, 29, f.ptr, out.ptr) == -9001
    ctx.synchronize()
    assert np.array_equal(out.download().ravel(), np.full(30, 7.5))
    with pytest.raises(ValueError):
        Semilinear2d(eps=0)
    assert ctx.gn_step(prob, z)[1] == 0                                # the handle is still usable
    prob.free()


# ------------------------------------------------------------------------------------------------ h. the driver
def test_driver_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'nonlinpdes-gpsolver_amd', 'main_Semilinear2d.py'), '--equation', 'burgers',
                        '--N_domain', '300', '--N_boundary', '80', '--nugget', '1e-6', '--GNsteps', '8', '--show_figure', ''],
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-1500:], r.stderr[-1500:])
    assert r.returncode == 0
    vals = {}
    for line in r.stdout.splitlines():
        for tag in ('[Collocation point error] Max error', '[Collocation point error] L2 error', '[Test error] Max error', '[Test error] L2 error'):
            if line.startswith(tag):
                vals[tag] = float(line[len(tag):])
    assert len(vals) == 4 and all(np.isfinite(v) for v in vals.values()), vals
