"""Equation classes with the reference's public API (src/PDEs.py): Nonlinear_elliptic2d, Burgers, Eikonal -- and Nonlinear_elliptic3d, the
same elliptic equation on a box in three space dimensions, and Semilinear2d, the semilinear equation with a gradient-dependent
nonlinearity on the Eikonal layout, and Semilinear3d, its counterpart in three dimensions and in time on the gradient layout, and
MongeAmpere2d and Quasilinear2d on the Hessian and the 2-jet layout, and KdV and Evolution1d, the Burgers system on the dispersive
layout and on the evolution layout with a general spatial operator (none has a counterpart in the reference).  The classes stand on _GPEquation; the two
elliptic ones are siblings on _EllipticEquation, which holds everything they share, and each says in its class attributes and in
_family() what sets it apart.

Same constructor arguments, methods and attributes; no JAX.  The Gram matrix, its Cholesky factor and the Gauss-Newton
iterate live in GPU memory (libgpk.so); `Theta`, `L`, ... are materialised as numpy arrays only when read.
Differences that are deliberate: no stale jit cache when Gram_matrix is called twice; user callbacks
may be numpy-vectorised or plain scalar Python functions.
"""
import os

import numpy as onp
from numpy import random

import gpk

from gpk.device import require_gaussian_family
from ._runtime import eval_callback, get_context
from .nonlinearity import GradientNonlinearity, GradientNonlinearity3d, Nonlinearity
from .quasilinear import QuasilinearEquation
from .sample_points import boundary_normals, boundary_normals3d, sampled_pts_grid, sampled_pts_grid3d, sampled_pts_rdm, sampled_pts_rdm3d

_NAN_MSG = '[Error] Loss is nan: maybe nugget is too small!'

# Default jitter of posterior_sample, absolute, in units of the prior variance k(x,x) = 1: the next power of ten above
# 32 * N_t * (largest entrywise error of the device's Sigma against long double) at N_t = 1024 -- measured, DESIGN.md section K
# ("Posterior covariance and samples").
POSTERIOR_JITTER = 1e-5


def divergence_form(a, a_x1, a_x2, v1, v2, c):
    """The six coefficients (c0, b1, b2, a11, a12, a22) of psi = a Laplace + (grad a - v) . grad - c, for which
    -psi[u] = -div(a grad u) + v . grad u + c u: scalar diffusivity a with gradient (a_x1, a_x2), velocity (v1, v2), reaction c
    (arrays over the points, or scalars).  What Nonlinear_elliptic2d(operator=...) returns for an advection-diffusion-reaction operator."""
    a, a_x1, a_x2, v1, v2, c = onp.broadcast_arrays(*(onp.asarray(t, dtype=onp.float64) for t in (a, a_x1, a_x2, v1, v2, c)))
    return -c, a_x1 - v1, a_x2 - v2, a, onp.zeros_like(a), a


def divergence_form3d(a, a_x1, a_x2, a_x3, v1, v2, v3, c):
    """The ten coefficients (c0, b1, b2, b3, a11, a12, a13, a22, a23, a33) of psi = a Laplace + (grad a - v) . grad - c in three
    dimensions, for which -psi[u] = -div(a grad u) + v . grad u + c u (arrays over the points, or scalars).  What
    Nonlinear_elliptic3d(operator=...) returns for an advection-diffusion-reaction operator."""
    a, a_x1, a_x2, a_x3, v1, v2, v3, c = onp.broadcast_arrays(*(onp.asarray(t, dtype=onp.float64) for t in (a, a_x1, a_x2, a_x3, v1, v2, v3, c)))
    z = onp.zeros_like(a)
    return -c, a_x1 - v1, a_x2 - v2, a_x3 - v3, a, z, z, a, z, a


def parabolic_form(nu, v1=0.0, v2=0.0, c=0.0):
    """A callable operator(x1, x2, t) for Nonlinear_elliptic3d with axis 3 as time: the ten coefficients of
    psi = nu Laplace_x - v . grad_x - c - d_t, for which -psi[u] = u_t - nu Laplace_x u + v . grad_x u + c u (constant nu, v1, v2, c)."""
    def operator(x1, x2, t):
        one = onp.ones(onp.shape(onp.asarray(x1, dtype=onp.float64)))
        z = 0.0 * one
        return -c * one, -v1 * one, -v2 * one, -one, nu * one, z, z, nu * one, z, z
    return operator


class _GPEquation(object):
    """Machinery shared by every equation class: Burgers, Eikonal, the two elliptic classes (through _EllipticEquation) and
    InverseProblems.Darcy_flow2d -- points and user callbacks, the Gram matrix and its factor on the device, loss / gradient / Hessian,
    the Gauss-Newton iteration, extension to test points, posterior and log evidence."""
    _layout = None              # Gram layout name
    _system = None              # Gauss-Newton system name
    _time_dependent = False
    _periodic_axes = (False, False)   # set on an instance (solver_GP: cfg.period): sampled_pts() leaves the faces of a periodic axis out
    _blocks_per_point = 1       # unknown groups per collocation point
    _dim = 2                    # columns of a point
    _structured_optin = True    # _problem() honours GPK_STRUCTURED
    _zero_start = False         # GN_method accepts initial_sol='zero'
    _bad_nugget_type = 'the reference leaves self.Theta unset here'

    # ---- user data -------------------------------------------------------------------------------------------------
    def get_bd(self, x1, x2):
        return self.bdy(x1, x2)

    def get_rhs(self, x1, x2):
        return self.rhs(x1, x2)

    @staticmethod
    def _pts(X):
        """points as the class takes them: an array, its shape unchecked as in the reference"""
        return onp.asarray(X, dtype=onp.float64)

    def _columns(self, X):
        return [X[:, k] for k in range(self._dim)]

    def _set_points(self, X_domain, X_boundary):
        self.X_domain = self._pts(X_domain)
        self.N_domain = self.X_domain.shape[0]
        self.X_boundary = self._pts(X_boundary)
        self.N_boundary = self.X_boundary.shape[0]
        self.rhs_f = eval_callback(self.get_rhs, *self._columns(self.X_domain))
        self.bdy_g = eval_callback(self.get_bd, *self._columns(self.X_boundary))
        self._drop_device_state()

    def sampled_pts(self, N_domain, N_boundary, sampled_type='random'):
        kw = {'periodic': tuple(self._periodic_axes)} if any(self._periodic_axes) else {}
        if sampled_type == 'random':
            X_domain, X_boundary = sampled_pts_rdm(N_domain, N_boundary, self.domain, time_dependent=self._time_dependent, **kw)
        elif sampled_type == 'grid':
            X_domain, X_boundary = sampled_pts_grid(N_domain, N_boundary, self.domain, time_dependent=self._time_dependent, **kw)
        else:
            raise UnboundLocalError("local variable 'X_domain' referenced before assignment")
        self._set_points(X_domain, X_boundary)

    def get_sampled_points(self, X_domain, X_boundary):
        self._set_points(X_domain, X_boundary)

    # ---- device state ----------------------------------------------------------------------------------------------
    def _drop_device_state(self):
        for name in ('_dTheta', '_dL'):
            a = self.__dict__.pop(name, None)
            if a is not None:
                a.free()
        p = self.__dict__.pop('_prob', None)
        if p is not None:
            p.free()                                           # (workspace, inverted blocks, prepared operators: everything but the factors)
        self.__dict__.pop('_Theta_host', None)
        self.__dict__.pop('_L_host', None)
        self._drop_posterior()
        self.__dict__.pop('_z_star', None)

    def _drop_posterior(self):
        """free what posterior_variance prepared (P = L^{-1} A(z*), the factor of H/2): it belongs to one iterate of one problem"""
        st = self.__dict__.pop('_posterior', None)
        if st is not None:
            for a in st[:2]:
                a.free()

    def _n_unknowns(self):
        return self._blocks_per_point * self.N_domain

    def _gn_params(self):
        raise NotImplementedError

    def _nl_args(self):
        """GNProblem keywords of the reaction term: none unless an elliptic class carries one other than the power law (whose alpha, m
        travel as p0, p1 of _gn_params(), as they always did)"""
        if getattr(self, 'nonlinearity', None) is None:
            return {}
        tau = self._tau()
        if tau.kind == 0:
            return {}
        return dict(p0=tau.params[0], p1=tau.params[1], p2=tau.params[2], nonlin=tau.kind)

    def _problem(self):
        if getattr(self, '_prob', None) is None:
            if getattr(self, '_dL', None) is None:
                raise RuntimeError('call Gram_matrix() and Gram_Cholesky() first')
            p0, p1, lam = self._gn_params()
            # GPK_STRUCTURED=1 / 2 (opt-in, elliptic system only; 2 adds the Gram level, gpk_gn_gram_prepare): the z-independent solves are done once and every step forms
            # [L^{-1}A(z) | L^{-1}F(z)] from them (gpk_gn_structured_prepare) -- same iterates, about half the time per step
            # (round 6: GPK_STRUCTURED=1 also for the Burgers and Eikonal systems, and the Darcy system in InverseProblems.py: A(z) = A1 diag(d(z)) + A2)
            # (2 = the Gram level: since round 6 for every system with a structured form).  A class with _structured_optin = False
            # ignores the variable: every step runs the reference's operation sequence.
            structured = int(os.environ.get('GPK_STRUCTURED', '0') or 0) if self._structured_optin else False
            self._prob = gpk.GNProblem(get_context(), self._system, self.N_domain, self.N_boundary, self.rhs_f, self.bdy_g,
                                       self._dL, **dict(dict(p0=p0, p1=p1), **self._nl_args()), pen_lambda=lam, structured=structured)
        return self._prob

    # ---- Gram matrix + Cholesky ------------------------------------------------------------------------------------
    def _assemble(self, kernel, kernel_parameter, nugget, nugget_type):
        if nugget_type not in ('adaptive', 'identity', 'none'):
            raise AttributeError(f"nugget_type {nugget_type!r}: {self._bad_nugget_type}")
        ctx = get_context()
        self._drop_device_state()
        self.nugget_type = nugget_type
        self.nugget = nugget
        self.kernel = kernel
        self.kernel_parameter = kernel_parameter
        self._dTheta, ratios = self._evaluate_gram(ctx, kernel, kernel_parameter, nugget, nugget_type)
        return ratios

    def _evaluate_gram(self, ctx, kernel, kernel_parameter, nugget, nugget_type):
        """the evaluator call of _assemble: (device matrix, trace ratios)"""
        return ctx.assemble(self._layout, kernel, kernel_parameter, self.X_domain, self.X_boundary, nugget, nugget_type)

    @property
    def Theta(self):
        """nugget-regularised Gram matrix as a numpy array (downloaded on first access)"""
        if '_Theta_host' not in self.__dict__:
            src = self.__dict__.get('_dTheta')
            if src is None:
                raise AttributeError('Theta: call Gram_matrix() first')
            self._Theta_host = src.download()
        return self._Theta_host

    def Gram_Cholesky(self):
        ctx = get_context()
        if getattr(self, '_dTheta', None) is None:
            raise AttributeError("Theta: call Gram_matrix() first")
        old = self.__dict__.pop('_dL', None)
        if old is not None:
            old.free()
        self.__dict__.pop('_L_host', None)
        self._dL = self._dTheta.clone()                   # Theta stays readable, as in the reference (HBM is plentiful)
        self.chol_info = ctx.potrf(self._dL)              # >0: first non-positive pivot; NaNs propagate like JAX
        if self.chol_info != 0:
            # the reference's try/except never fires under JAX: it carries on with NaNs, and so do we
            print('[Warning] Cholesky factorization met a non-positive pivot at index', self.chol_info,
                  '(the reference would silently continue with NaNs): maybe nugget is too small!')

    @property
    def L(self):
        if '_L_host' not in self.__dict__:
            if getattr(self, '_dL', None) is None:
                raise AttributeError('L: call Gram_Cholesky() first')
            self._L_host = onp.tril(self._dL.download())
        return self._L_host

    # ---- loss / gradient / Hessian -----------------------------------------------------------------------------------
    def _z(self, z):
        return get_context().array(onp.asarray(z, dtype=onp.float64).ravel())

    def loss(self, z):
        return get_context().gn_loss(self._problem(), self._z(z))

    def grad_loss(self, z):
        _, g = get_context().gn_hessian_grad(self._problem(), self._z(z))
        return g

    def _hessian(self, z):
        H, _ = get_context().gn_hessian_grad(self._problem(), self._z(z))
        return H

    def _measurement(self, z):
        return get_context().gn_measurement(self._problem(), self._z(z))

    def _tri_loss(self, vec):
        """||L^{-1} vec||^2 for a host vector (used by GN_loss)."""
        ctx = get_context()
        d = ctx.array(vec)
        ctx.trsm(self._dL, d, trans=False, nrhs=1)
        w = d.download()
        return float(w @ w)

    # ---- Gauss-Newton ----------------------------------------------------------------------------------------------
    def _initial(self, initial_sol, n):
        if isinstance(initial_sol, onp.ndarray):               # a given iterate (solver_GP.select_kernel_parameter: one draw for every candidate)
            if initial_sol.shape != (n,):
                raise ValueError(f'initial_sol: {initial_sol.shape} values for {n} unknowns')
            return onp.array(initial_sol, dtype=onp.float64)
        if self._zero_start and isinstance(initial_sol, str) and initial_sol == 'zero':
            return onp.zeros(n)
        if initial_sol == 'rdm':
            return random.normal(0.0, 1.0, (n))
        raise UnboundLocalError("local variable 'sol' referenced before assignment")   # as the reference

    def _check_step_info(self, it, info):
        """info > 0: the Cholesky of the Gauss-Newton matrix H of step `it` met a non-positive pivot (LAPACK numbering).  The reference
        solves H with jnp.linalg.solve (src/PDEs.py:118), which never reports anything and carries on with whatever comes out; here the step
        has been taken with NaNs from that pivot on, exactly as visible in the next loss -- say so at once, in the reference's wording."""
        self.step_info = getattr(self, 'step_info', [])
        self.step_info.append(int(info))
        if info > 0:
            print('[Error] Cholesky factorization of the Gauss-Newton matrix failed at step', it, '(non-positive pivot at index', info,
                  '): maybe nugget is too small!')

    def _gn_iterate(self, prob, sol, max_iter, step_size, print_hist, check_nan=True):
        self.step_info = []
        self._drop_posterior()
        ctx = get_context()
        z = ctx.array(sol)
        loss_hist = []

        def record(it, value):
            loss_hist.append(value)
            if check_nan and onp.isnan(value):
                print(_NAN_MSG)
            if print_hist:
                if it == 0:
                    print('iter = 0', 'Loss =', value)
                else:
                    print('iter = ', it, 'Gauss-Newton step size =', step_size, ' Loss = ', value)
        # The loss history is the reference's: J(z_0), then J(z_k) after every update (src/PDEs.py:108-124).  gpk_gn_step returns the
        # loss of the iterate it STARTS from -- since round 5 by true substitution with the factor (one vector; its chain runs on the handle's side
        # stream beside the end of the step: exact to rounding, like gpk_gn_loss; round 6: in the structured modes too) -- so max_iter steps yield
        # J(z_0) .. J(z_{max_iter-1}) and one gpk_gn_loss closes the history.  Rounds 2-4 took that number from the F column of the
        # GEMM-only solve (~1e-8 relative error at nugget <= 1e-12 near convergence: gpk_tune(52, 0)) and round 4 therefore called
        # gpk_gn_loss after every step; GPK_SEPARATE_LOSS=1 keeps that sequence (same numbers to rounding, one more solve per step).
        ls = getattr(self, 'line_search', None)                  # a run-time instance attribute (src/linesearch.py); None: the loop below
        if ls is not None:
            # gpk_gn_step_ls: direction, the K trial losses (one K-column solve) and the acceptance on the device, one synchronisation per
            # step; like gpk_gn_step it returns the loss of the iterate it starts from, so the history keeps the reference's shape
            t0 = ls.first_step(step_size)
            self.step_hist, self.trial_loss_hist, self.ls_failed, self.ls_accepted = [], [], [], []
            for it in range(max_iter):
                loss_in, info, k, t_acc, trial = ctx.gn_step_ls(prob, z, ls.trials, t0, ls.shrink, ls.c1)
                record(it, loss_in)
                self._check_step_info(it + 1, info)
                self.step_hist.append(t_acc if k >= 0 else 0.0)
                self.ls_accepted.append(k)
                self.trial_loss_hist.append(trial)
                if k < 0:
                    self.ls_failed.append(it + 1)
                    print('[Error] line search failed at step', it + 1, ': none of the', ls.trials, 'trial steps from', t0,
                          'down reduces the loss; the iterate is kept')
            record(max_iter, ctx.gn_loss(prob, z))
        elif os.environ.get('GPK_SEPARATE_LOSS', '0') != '1':
            for it in range(max_iter):
                loss_in, info = ctx.gn_step(prob, z, step_size)   # loss of the iterate the step starts from
                record(it, loss_in)
                self._check_step_info(it + 1, info)
            record(max_iter, ctx.gn_loss(prob, z))
        else:
            record(0, ctx.gn_loss(prob, z))
            for it in range(1, max_iter + 1):
                _, info = ctx.gn_step(prob, z, step_size)
                self._check_step_info(it, info)
                record(it, ctx.gn_loss(prob, z))
        self.max_iter = max_iter
        self.step_size = step_size
        self.loss_hist = loss_hist
        self._z_star = (prob, z.download())                   # the final iterate and the system it belongs to (posterior_variance)
        return self._z_star[1]

    def _gn_solve(self, n_unknowns, max_iter, step_size, initial_sol, print_hist, problem=None, finish=None):
        """what every GN_method does: the start, the iteration on the device, then (sol_vec, sol_sampled_pts) of the final iterate from the
        class's _sol_vec.  problem / finish: the relaxed formulation's own system and closing step in place of _problem / _sol_vec."""
        sol = self._initial(initial_sol, n_unknowns)
        self.init_sol = sol
        sol = self._gn_iterate((problem or self._problem)(), sol, max_iter, step_size, print_hist)
        self.sol_vec, self.sol_sampled_pts = (finish or self._sol_vec)(sol)

    def extend_sol(self, X_test):
        ctx = get_context()
        X_test = onp.asarray(X_test, dtype=onp.float64)
        coeff = ctx.array(self.sol_vec)
        ctx.potrs(self._dL, coeff, nrhs=1)                         # L^{-T} L^{-1} sol_vec
        self.X_test = X_test
        self.N_test = X_test.shape[0]
        self.extended_sol = ctx.extend(self._layout, self.kernel, self.kernel_parameter, X_test, self.X_domain,
                                       self.X_boundary, coeff).download()

    # ---- derivatives and PDE residual of the solution away from the collocation points (gpk_extend_functionals, gpk_pde_residual) --
    # Both leave every attribute of extend_sol / GN_method as it is; they set extended_derivatives / test_residual only.
    _deriv_names = ('value', 'd1', 'd2', 'laplacian')           # rows of the u-field handed to gpk_pde_residual

    def _coeff(self, Ld, vec):
        """Theta^{-1} vec on the device, as extend_sol computes it (L^{-T} L^{-1} vec)"""
        coeff = get_context().array(vec)
        get_context().potrs(Ld, coeff, nrhs=1)
        return coeff

    def _derivative_fields(self, X_test):
        """{'u': (len(_deriv_names), Nt) DeviceArray}"""
        coeff = self._coeff(self._dL, self.sol_vec)
        return {'u': get_context().extend_functionals(self._layout, self.kernel, self.kernel_parameter, X_test, self.X_domain,
                                                      self.X_boundary, coeff, which=self._deriv_names)}

    @staticmethod
    def _rows(d, names):
        a = d.download().reshape(len(names), -1)
        return {n: a[k].copy() for k, n in enumerate(names)}

    def extend_derivatives(self, X_test):
        """value, d1, d2 and laplacian (Burgers: value, d1 = u_t, d2 = u_x, d2d2 = u_xx) of the GP solution at X_test (numpy arrays)"""
        X_test = onp.asarray(X_test, dtype=onp.float64)
        self.extended_derivatives = self._rows(self._derivative_fields(X_test)['u'], self._deriv_names)
        return self.extended_derivatives

    def _residual_params(self):
        return self._gn_params()[:2]

    def _residual(self, fields_u, fields_a, rhs):
        """the residual kernel on rows of the extension: gpk_pde_residual, or gpk_pde_residual_nl when a reaction term other than the
        power law is set (elliptic classes)"""
        tau = self._tau() if getattr(self, 'nonlinearity', None) is not None else None
        if tau is not None and tau.kind != 0:
            return get_context().pde_residual_nl(tau.kind, tau.params, fields_u, rhs).download().reshape(-1)
        return get_context().pde_residual(self._system, self._residual_params(), fields_u, fields_a, rhs).download().reshape(-1)

    def PDE_residual(self, X_test):
        """pointwise residual of the equation at X_test from the derivatives of the GP solution (rhs evaluated at X_test)"""
        X_test = onp.asarray(X_test, dtype=onp.float64)
        fields = self._derivative_fields(X_test)
        rhs = eval_callback(self.get_rhs, X_test[:, 0], X_test[:, 1])
        self.test_residual = self._residual(fields['u'], fields.get('a'), rhs)
        return self.test_residual

    # ---- posterior variance of the solution at test points (gpk_posterior_prepare, gpk_assemble_cross, gpk_posterior_variance) -------
    _posterior_fields = (('', 0, None),)                        # (attribute suffix, field id, Gram layout or None = self._layout)

    def _posterior_unserved(self):
        """why posterior_variance is not available for this object, or None"""
        return None

    def _final_iterate(self, caller, what, entry):
        """(prob, z*) of the last GN_method for `caller` (the prefix of its messages); the relaxed system, which the device entry point
        `entry` does not serve, is refused as having no `what` entry point"""
        star = self.__dict__.get('_z_star')
        if star is None:
            raise RuntimeError(f'{caller}: call GN_method() first')
        prob, z = star
        if prob.struct.system == gpk.SYSTEM['Nonlinear_elliptic_relaxed']:
            raise NotImplementedError(f'{caller}: the relaxed formulation (GN_relaxed_method) has no {what} entry point '
                                      f'({entry} returns -9001 for GPK_GN_ELLIPTIC_RELAXED); solve with GN_method')
        return prob, z

    @staticmethod
    def _warn_pivot(info, undefined):
        if info != 0:
            print('[Warning] Cholesky factorization of the Gauss-Newton matrix at the final iterate met a non-positive pivot at index',
                  info, f': the {undefined} not defined there')

    def _posterior_state(self):
        """(P, R, info, prob): prepared once per final iterate, dropped with the device state and at the next GN_method"""
        reason = self._posterior_unserved()
        if reason is not None:
            raise NotImplementedError('posterior_variance: ' + reason)
        prob, z = self._final_iterate('posterior_variance', 'variance', 'gpk_posterior_prepare')
        if self.__dict__.get('_posterior') is None:
            ctx = get_context()
            dz = ctx.array(z)
            P, R, info = ctx.posterior_prepare(prob, dz)
            dz.free()
            self._warn_pivot(info, 'posterior variance is')
            self._posterior = (P, R, info, prob)
        return self._posterior

    def _posterior_compute(self, X_test, nt_chunk):
        """{suffix: (var_cond, var)} as numpy arrays for every field of the equation"""
        P, R, _, prob = self._posterior_state()
        X_test = onp.asarray(X_test, dtype=onp.float64)
        out = {}
        for tag, field, layout in self._posterior_fields:
            out[tag] = get_context().posterior_variance_points(prob, P, R, field, layout or self._layout, self.kernel, self.kernel_parameter,
                                                               X_test, self.X_domain, self.X_boundary, nt_chunk)
        return out

    def posterior_variance(self, X_test, nt_chunk=1024):
        """Posterior variance of the GP solution u at X_test, Gauss-Newton (Laplace) form at the final iterate of GN_method:
        var = var_cond + var_gn with var_cond = k(x,x) - k^T Theta^{-1} k (the collocation values taken as known) and var_gn the
        contribution of their own covariance (A^T Theta^{-1} A)^{-1}.  Sets extended_var, extended_var_cond (raw values: rounding can leave
        either slightly negative where the variance is at the nugget level) and extended_std = sqrt(max(extended_var, 0)); returns
        extended_var.  X_test is processed in batches of nt_chunk points, so the workspace is (N + n_z) * nt_chunk doubles whatever
        the number of test points.  The value of u only; Nonlinear_elliptic2d (Dirichlet data, the Laplacian, any nonlinearity),
        Burgers, Eikonal and Darcy_flow2d -- NotImplementedError with bc / operator set, for Nonlinear_elliptic3d and after
        GN_relaxed_method.  No attribute of extend_sol or GN_method is touched."""
        vc, v = self._posterior_compute(X_test, nt_chunk)['']
        self.extended_var_cond = vc
        self.extended_var = v
        self.extended_std = onp.sqrt(onp.maximum(v, 0.0))
        return self.extended_var

    # ---- joint posterior covariance and samples at test points (gpk_assemble_prior, gpk_posterior_covariance, gpk_posterior_sample) ----
    def _posterior_cov_compute(self, X_test, keep=False):
        """{suffix: (cov_cond, cov[, device array of cov])} for every field of the equation, all of X_test in one batch"""
        P, R, _, prob = self._posterior_state()
        X_test = onp.asarray(X_test, dtype=onp.float64)
        out = {}
        for tag, field, layout in self._posterior_fields:
            out[tag] = get_context().posterior_covariance_points(prob, P, R, field, layout or self._layout, self.kernel,
                                                                 self.kernel_parameter, X_test, self.X_domain, self.X_boundary, keep=keep)
        return out

    def posterior_covariance(self, X_test):
        """Joint posterior covariance of the GP solution u at the points X_test, Gauss-Newton (Laplace) form at the final iterate of
        GN_method: Sigma = Sigma_cond + Sigma_gn, the matrix whose diagonal posterior_variance returns ("Posterior
        covariance and samples").  Sets extended_cov and extended_cov_cond (N_test x N_test, raw values, bitwise symmetric); returns
        extended_cov.  All of X_test is one batch: (N + n_z + N_test) N_test doubles on the device, ValueError if they do not fit.
        Served and refused exactly as posterior_variance.  No attribute of extend_sol, posterior_variance or GN_method is touched."""
        cc, c = self._posterior_cov_compute(X_test)['']
        self.extended_cov_cond = cc
        self.extended_cov = c
        return self.extended_cov

    def _posterior_means(self, X_test):
        """{suffix: posterior mean at X_test} through the class's own extend_sol, whose attributes are then put back as they were"""
        names = ('X_test', 'N_test') + tuple('extended_sol' + tag for tag, _, _ in self._posterior_fields)
        before = {n: self.__dict__[n] for n in names if n in self.__dict__}
        try:
            self.extend_sol(X_test)
            return {tag: onp.array(getattr(self, 'extended_sol' + tag), dtype=onp.float64).ravel() for tag, _, _ in self._posterior_fields}
        finally:
            for n in names:
                self.__dict__.pop(n, None)
            self.__dict__.update(before)

    def _posterior_xi(self, xi, n_fields, N_test, n_samples, seed):
        """the standard normals of posterior_sample, one (N_test, n_samples) array per field, in the order of _posterior_fields"""
        if xi is None:
            rng = onp.random.RandomState(seed)
            return [rng.standard_normal((N_test, n_samples)) for _ in range(n_fields)]
        xs = [onp.asarray(xi, dtype=onp.float64)] if n_fields == 1 else [onp.asarray(x, dtype=onp.float64) for x in xi]
        if len(xs) != n_fields or any(x.shape != (N_test, n_samples) for x in xs):
            raise ValueError(f'posterior_sample: xi must be {"one array" if n_fields == 1 else f"{n_fields} arrays (u, a)"} of shape '
                             f'({N_test}, {n_samples}) = (N_test, n_samples); got {[x.shape for x in xs]}')
        return xs

    def _posterior_sample_compute(self, X_test, n_samples, seed, xi, jitter):
        """{suffix: (n_samples, N_test) samples}"""
        X_test = onp.asarray(X_test, dtype=onp.float64)
        n_samples, N_test = int(n_samples), X_test.shape[0]
        if n_samples < 1:
            raise ValueError('posterior_sample: n_samples must be at least 1')
        jitter = POSTERIOR_JITTER if jitter is None else float(jitter)
        self._posterior_state()                                # (refusals first: before anything is computed or drawn)
        xs = self._posterior_xi(xi, len(self._posterior_fields), N_test, n_samples, seed)
        means = self._posterior_means(X_test)
        covs = self._posterior_cov_compute(X_test, keep=True)
        out, failed = {}, None
        for (tag, _, _), x in zip(self._posterior_fields, xs):
            dC = covs[tag][2]
            if failed is None:
                samples, info = get_context().posterior_sample(dC, means[tag], x, jitter, nt=N_test)
                if info != 0:
                    failed = (tag, info)
                else:
                    out[tag] = onp.ascontiguousarray(samples.T)
            dC.free()
        if failed is not None:
            raise RuntimeError(f'posterior_sample: the Cholesky factorisation of the posterior covariance{" of " + failed[0][1:] if failed[0] else ""} '
                               f'met a non-positive pivot at index {failed[1]} with jitter = {jitter:g}; pass a larger jitter')
        return out

    def posterior_sample(self, X_test, n_samples=1, seed=None, xi=None, jitter=None):
        """n_samples draws of the GP solution at X_test from N(mean, Sigma + jitter I): mean the extension of extend_sol (whose
        attributes are left as they are), Sigma of posterior_covariance, sample = mean + L xi with L L^T = Sigma + jitter I on the device.
        xi: the (N_test, n_samples) standard normals to use; None: numpy.random.RandomState(seed).standard_normal((N_test, n_samples)) --
        nothing is drawn on the device, so the same seed (or xi) gives the same bits.  jitter: absolute, in units of the prior variance
        k(x,x) = 1; None: POSTERIOR_JITTER.  Sets and returns extended_samples (n_samples x N_test).
        RuntimeError when the factorisation meets a non-positive pivot; served and refused exactly as posterior_variance."""
        self.extended_samples = self._posterior_sample_compute(X_test, n_samples, seed, xi, jitter)['']
        return self.extended_samples

    # ---- log evidence of the kernel at the final iterate (gpk_log_evidence) ----------------------------------------------------------
    def log_evidence(self):
        """Laplace approximation of the log evidence log Z of the data f, g (Darcy: and the observations) under the kernel the Gram
        matrix was built with, at the final iterate z* of GN_method ("Log evidence"):
            log Z = -J(z*)/2 - sum_k log|Theta_k|/2 - log|H/2|/2 - N_data log gamma - (N_d + N_b + N_data)/2 log 2 pi.
        Sets log_evidence_terms (log_Z, J, logdet_theta, logdet_H, gamma_term, two_pi_term, info) and returns log Z -- NaN when the
        factorisation of H/2 fails (info != 0) or a pivot of a factor is not positive.  Served for every class whose Gauss-Newton system
        gpk_posterior_prepare serves, bc= / operator= and Nonlinear_elliptic3d included (their system is the elliptic one on their own
        Theta); NotImplementedError after GN_relaxed_method.  P = L^{-1} A(z*) and the factor of H/2 are kept where posterior_variance
        looks for them, so a following posterior_variance does not prepare again."""
        prob, z = self._final_iterate('log_evidence', 'evidence', 'gpk_log_evidence')
        ctx = get_context()
        dz = ctx.array(z)
        terms, P, R, info = ctx.log_evidence(prob, dz)
        dz.free()
        self._warn_pivot(info, 'log evidence and the posterior variance are')   # (the posterior slot is filled here: said for both)
        self._drop_posterior()
        self._posterior = (P, R, info, prob)
        self.log_evidence_terms = dict(terms, info=info)
        return terms['log_Z']


class _EllipticEquation(_GPEquation):
    """-psi[u] + tau(u) = f on a box, B u = g on its faces: everything Nonlinear_elliptic2d and Nonlinear_elliptic3d share.  psi is the
    Laplacian, or any second-order linear operator with variable coefficients (operator= / set_domain_operator: a row of len(_op_names)
    coefficients per domain point, kept in domain_coeffs); B is the identity, or a first-order functional (bc= / set_boundary_operator: a
    row of _dim + 1 coefficients per boundary point, kept in boundary_coeffs); tau is alpha u^m, or the `nonlinearity` given.
    A subclass gives the attributes below, its __init__ and Gram_matrix (their defaults and docstrings), _posterior_unserved, and ONE
    routing point: _family() names the evaluator family that serves the object as it stands -- 'plain', 'bc' or 'op' -- and
    _evaluate_gram and _fields turn that name into the device calls.  No other method chooses an evaluator; where one below reads
    domain_coeffs, it asks whether psi is the Laplacian (which rows to return, which coefficients to expect), not whom to call."""
    _system = 'Nonlinear_elliptic'
    _BC = ('dirichlet', 'neumann', 'robin')
    _op_names = None            # rows of the operator evaluator: value, the _dim first derivatives, the second derivatives
    _laplacian_row = None       # the Laplacian as a coefficient row over _op_names
    _normals = None             # outward unit normals: f(X_boundary, domain)
    _xs = _count = _coeff_names = None      # fragments of the messages: callback arguments, len(_op_names) in words, the coefficients

    def __init__(self, alpha, m, bdy, rhs, domain, bc, robin_beta, operator, nonlinearity):
        if bc not in self._BC:
            raise ValueError(f'bc {bc!r}: one of {self._BC}')
        if operator is not None and not callable(operator):
            raise ValueError(f'operator {operator!r}: a callable operator{self._xs} returning {self._count} coefficient arrays, or None')
        self.alpha = alpha
        self.m = m
        self.bdy = bdy
        self.rhs = rhs
        self.domain = domain
        self.bc = bc
        self.robin_beta = robin_beta
        self.operator = operator
        self.boundary_coeffs = None
        self.domain_coeffs = None
        self.nonlinearity = None if nonlinearity is None else Nonlinearity.make(nonlinearity)

    def _gn_params(self):
        return float(self.alpha), float(self.m), 0.0

    def _tau(self):
        """the reaction term: the one given, or the power law of the current alpha, m"""
        return self.nonlinearity if self.nonlinearity is not None else Nonlinearity.power(self.alpha, self.m)

    # ---- the routing point and the two methods that act on it: each subclass's own -------------------------------------------------
    def _family(self):
        raise NotImplementedError

    def _fields(self, X_test, which):
        """rows `which` of the extension at X_test, from the evaluator of _family(): a (len(which), Nt) DeviceArray"""
        raise NotImplementedError

    # ---- boundary operator (N_boundary, _dim + 1), domain operator (N_domain, len(_op_names)); None = Dirichlet / the Laplacian ----
    def _set_points(self, X_domain, X_boundary):
        super()._set_points(X_domain, X_boundary)
        self.boundary_coeffs = None                        # custom operators belong to the points they were set for
        if self.bc != 'dirichlet':
            n = self._normals(self.X_boundary, self.domain)
            beta = float(self.robin_beta) if self.bc == 'robin' else 0.0
            self.boundary_coeffs = onp.concatenate([onp.full((self.N_boundary, 1), beta), n], axis=1)
        self.domain_coeffs = None
        if self.operator is not None:
            self.domain_coeffs = self._operator_at(self.X_domain)

    def _operator_at(self, X):
        """the callable `operator` at the points X (n, _dim) as an (n, len(_op_names)) array"""
        rows = self.operator(*self._columns(X))
        if len(rows) != len(self._op_names):
            raise ValueError(f'operator must return {self._count} coefficient arrays {self._coeff_names}, got {len(rows)}')
        return onp.stack([onp.broadcast_to(onp.asarray(r, dtype=onp.float64), (X.shape[0],)) for r in rows], axis=1)

    def set_domain_operator(self, coeffs):
        """Row i of coeffs (N_domain, len(_op_names)) holds the coefficients of psi_i over _op_names -- (c0, b1, b2, a11, a12, a22) in two
        dimensions, (c0, b1, b2, b3, a11, a12, a13, a22, a23, a33) in three; a mixed coefficient multiplies its mixed derivative once --
        and the equation at domain point i reads -psi_i[u] + alpha u^m = rhs_f[i].  Call after the points are set; dropped when they
        change.  Discards the Gram matrix and everything derived from it."""
        coeffs = onp.array(coeffs, dtype=onp.float64)
        if coeffs.shape != (self.N_domain, len(self._op_names)):
            raise ValueError(f'coeffs must have shape ({self.N_domain}, {len(self._op_names)}), got {coeffs.shape}')
        self.domain_coeffs = coeffs
        self._drop_device_state()

    def set_boundary_operator(self, coeffs):
        """Row b of coeffs (N_boundary, _dim + 1) = (c0, c1, ..): the condition at boundary point b reads c0 u + c . grad u = bdy_g[b].
        Call after the points are set; dropped when they change.  Discards the Gram matrix and everything derived from it."""
        coeffs = onp.array(coeffs, dtype=onp.float64)
        if coeffs.shape != (self.N_boundary, self._dim + 1):
            raise ValueError(f'coeffs must have shape ({self.N_boundary}, {self._dim + 1}), got {coeffs.shape}')
        self.boundary_coeffs = coeffs
        self._drop_device_state()

    # ---- Gauss-Newton (elimination formulation) --------------------------------------------------------------------------------------
    def GN_loss(self, z, z_old):
        z = onp.asarray(z, float); z_old = onp.asarray(z_old, float)
        zz = onp.concatenate([self._tau().dtau(z_old) * (z - z_old), z, self.bdy_g])
        return self._tri_loss(zz)

    def Hessian_GN(self, z, z_old):
        return self._hessian(z_old)          # hessian(GN_loss)(z, z_old) does not depend on z (quadratic in z)

    def GN_method(self, max_iter=3, step_size=1, initial_sol='rdm', print_hist=True):
        """initial_sol: 'rdm' (standard normal draw), or an ndarray with one value per unknown: the iterate to start from."""
        self._gn_solve(self._n_unknowns(), max_iter, step_size, initial_sol, print_hist)

    def _sol_vec(self, sol):
        return onp.concatenate([self._tau().tau(sol) - self.rhs_f, sol, self.bdy_g]), sol

    # ---- the solution away from the collocation points -------------------------------------------------------------------------------
    def extend_sol(self, X_test):
        X_test = self._pts(X_test)
        self.X_test = X_test
        self.N_test = X_test.shape[0]
        self.extended_sol = self._fields(X_test, ('value',)).download().reshape(-1)

    def _laplacian(self, r):
        lap = r['d11'] + r['d22']
        return lap if self._dim == 2 else lap + r['d33']

    def extend_derivatives(self, X_test):
        """the rows _deriv_names of the GP solution at X_test (numpy arrays): value, first derivatives, laplacian; with a domain operator
        additionally every second derivative of _op_names (laplacian = their trace)"""
        X_test = self._pts(X_test)
        first, second = self._op_names[:self._dim + 1], self._op_names[self._dim + 1:]
        if self.domain_coeffs is not None:
            r = self._rows(self._fields(X_test, self._op_names), self._op_names)
            self.extended_derivatives = dict({n: r[n] for n in first}, laplacian=self._laplacian(r), **{n: r[n] for n in second})
        elif self._family() == 'op':         # a boundary condition served by the operator family (3-D), which has no laplacian row
            names = first + tuple(n for n in second if n[1] == n[2])      # d11, d22, d33: the pure second derivatives
            r = self._rows(self._fields(X_test, names), names)
            self.extended_derivatives = dict({n: r[n] for n in first}, laplacian=self._laplacian(r))
        else:
            self.extended_derivatives = self._rows(self._fields(X_test, self._deriv_names), self._deriv_names)
        return self.extended_derivatives

    _residual_rows = ('value', 'd1', 'd2', 'laplacian')         # the rows gpk_pde_residual takes; it reads value and laplacian

    def _psi_fields(self, X_test, coeffs_t):
        """_residual_rows with psi_t[u] in the Laplacian's place, from the operator family: psi_t from coeffs_t (Nt, len(_op_names)), from
        the callable `operator`, or the Laplacian when only the boundary condition is general"""
        n = len(self._op_names)
        if coeffs_t is None:
            if self.domain_coeffs is None:
                coeffs_t = onp.tile(self._laplacian_row, (X_test.shape[0], 1))
            elif self.operator is None:
                raise ValueError('the domain operator was set per point (set_domain_operator): pass its coefficients at the test '
                                 f'points as coeffs_t (Nt,{n})')
            else:
                coeffs_t = self._operator_at(X_test)
        coeffs_t = onp.asarray(coeffs_t, dtype=onp.float64)
        if coeffs_t.shape != (X_test.shape[0], n):
            raise ValueError(f'coeffs_t must have shape ({X_test.shape[0]}, {n}), got {coeffs_t.shape}')
        rows = self._fields(X_test, self._op_names).download().reshape(n, -1)
        psi = (coeffs_t.T * rows).sum(axis=0)                     # psi_t[u]: a combination of the rows, per test point
        return get_context().array(onp.stack([rows[0], rows[1], rows[2], psi]))

    def _derivative_fields(self, X_test, coeffs_t=None):
        """{'u': the rows _residual_rows at X_test as a DeviceArray}"""
        if self._family() == 'op':
            return {'u': self._psi_fields(X_test, coeffs_t)}
        return {'u': self._fields(X_test, self._residual_rows)}

    def PDE_residual(self, X_test, coeffs_t=None):
        """pointwise residual -Delta u + tau(u) - f at X_test from the derivatives of the GP solution (rhs evaluated at X_test); with a
        domain operator -psi_t[u] + tau(u) - f, psi_t from the callable `operator` or from coeffs_t (Nt, len(_op_names)) (needed when the
        operator was set per point; ValueError otherwise)"""
        X_test = self._pts(X_test)
        if self.domain_coeffs is None and coeffs_t is not None:
            raise ValueError('coeffs_t given, but no domain operator is set')
        fields = self._derivative_fields(X_test, coeffs_t)
        rhs = eval_callback(self.get_rhs, *self._columns(X_test))
        self.test_residual = self._residual(fields['u'], None, rhs)
        return self.test_residual

    def boundary_residual(self, X_bt, coeffs_t, g_t):
        """c0 u + c . grad u - g of the GP solution at the points X_bt (n, _dim), with coeffs_t (n, _dim + 1) = (c0, c1, ..) and g_t (n,)
        given per point: how well the boundary condition holds between the boundary collocation points (numpy array, also `bdy_residual`)."""
        X_bt = self._pts(onp.asarray(X_bt, dtype=onp.float64).reshape(-1, self._dim))
        coeffs_t = onp.asarray(coeffs_t, dtype=onp.float64).reshape(-1, self._dim + 1)
        g_t = onp.asarray(g_t, dtype=onp.float64).ravel()
        if coeffs_t.shape[0] != X_bt.shape[0] or g_t.size != X_bt.shape[0]:
            raise ValueError(f'{X_bt.shape[0]} points against {coeffs_t.shape[0]} coefficient rows and {g_t.size} values')
        names = self._op_names[:self._dim + 1]                  # value, d1, .. d_dim
        r = self._rows(self._fields(X_bt, names), names)
        res = coeffs_t[:, 0] * r['value']
        for k in range(1, self._dim + 1):
            res = res + coeffs_t[:, k] * r[names[k]]
        self.bdy_residual = res - g_t
        return self.bdy_residual


class Nonlinear_elliptic2d(_EllipticEquation):
    """-Delta u + alpha*u^m = f on a rectangle (reference src/PDEs.py:18-208); with operator=... / set_domain_operator() the semilinear
    equation -psi[u] + alpha*u^m = f for any second-order linear operator psi with variable coefficients (no counterpart in the reference).
    Three evaluator families (_family); the plain one is the reference's layout, which alone takes the Matern kernels, stores `ratio`
    only for the adaptive nugget, honours GPK_STRUCTURED and serves the posterior.  The relaxed formulation exists here only."""
    _layout = 'Nonlinear_elliptic'
    _op_names = ('value', 'd1', 'd2', 'd11', 'd12', 'd22')      # rows of gpk_extend_functionals_op
    _laplacian_row = (0.0, 0.0, 0.0, 1.0, 0.0, 1.0)
    _normals = staticmethod(boundary_normals)
    _xs, _count, _coeff_names = '(x1, x2)', 'six', '(c0, b1, b2, a11, a12, a22)'

    def __init__(self, alpha=1.0, m=3, bdy=None, rhs=None, domain=onp.array([[0, 1], [0, 1]]), bc='dirichlet', robin_beta=1.0,
                 operator=None, nonlinearity=None):
        """nonlinearity (no counterpart in the reference): the reaction term tau of -psi[u] + tau(u) = f as (name, parameters...) --
        ('exp', p0, p1) p0 exp(p1 u); ('sinh', p0, p1); ('sin', p0, p1); ('cubic', c1, c2, c3) c1 u + c2 u^2 + c3 u^3; ('power', alpha, m)
        -- or None: alpha u^m with the arguments alpha, m, and every call goes the way it always went (src/nonlinearity.py).
        bc (no counterpart in the reference, which imposes Dirichlet data only): the operator B on the boundary, whose prescribed value
        g = B u is what `bdy(x1, x2)` returns -- 'dirichlet' B u = u; 'neumann' B u = du/dn; 'robin' B u = robin_beta u + du/dn, n the
        outward unit normal (sample_points.boundary_normals).  set_boundary_operator() takes an arbitrary first-order operator per
        boundary point.  With 'dirichlet' and no custom operator every call goes the way it always went.
        operator (no counterpart in the reference either): a callable operator(x1, x2) returning the six coefficient arrays
        (c0, b1, b2, a11, a12, a22) of psi = c0 + b1 d_1 + b2 d_2 + a11 d_1 d_1 + a12 d_1 d_2 + a22 d_2 d_2; the equation solved is then
        -psi[u] + alpha u^m = f (divergence_form() gives the coefficients of -div(a grad u) + v . grad u + c u; a12 multiplies the mixed
        derivative once).  Evaluated at the domain points when they are set and at the test points by PDE_residual.  None: the
        Laplacian, and every call goes the way it always went."""
        super().__init__(alpha, m, bdy, rhs, domain, bc, robin_beta, operator, nonlinearity)

    # ---- which evaluator serves this object: decided here and nowhere else -----------------------------------------------------------
    def _family(self):
        """'op': gpk_assemble_op / gpk_extend_functionals_op, with a domain operator (and whatever boundary condition);
        'bc': gpk_assemble_bc / gpk_extend_functionals_bc, with a boundary functional alone;
        'plain': the reference's layout through gpk_assemble / gpk_extend / gpk_extend_functionals"""
        if self.domain_coeffs is not None:
            return 'op'
        return 'plain' if self.boundary_coeffs is None else 'bc'

    def _evaluate_gram(self, ctx, kernel, kernel_parameter, nugget, nugget_type):
        family = self._family()
        if family == 'plain':
            return super()._evaluate_gram(ctx, kernel, kernel_parameter, nugget, nugget_type)
        if family == 'op':
            T, ratio = ctx.assemble_op(kernel, kernel_parameter, self.X_domain, self.X_boundary, self.domain_coeffs, self.boundary_coeffs,
                                       nugget, nugget_type)
        else:
            T, ratio = ctx.assemble_bc(kernel, kernel_parameter, self.X_domain, self.X_boundary, self.boundary_coeffs, nugget, nugget_type)
        return T, [ratio]

    def _fields(self, X_test, which):
        ctx, family = get_context(), self._family()
        args = (self.kernel, self.kernel_parameter, X_test, self.X_domain, self.X_boundary)
        coeff = self._coeff(self._dL, self.sol_vec)
        if family == 'op':
            return ctx.extend_functionals_op(*args, self.domain_coeffs, self.boundary_coeffs, coeff, which=which)
        if family == 'bc':
            return ctx.extend_functionals_bc(*args, self.boundary_coeffs, coeff, which=which)
        return ctx.extend_functionals(self._layout, *args, coeff, which=which)

    def extend_sol(self, X_test):
        if self._family() == 'plain':
            return _GPEquation.extend_sol(self, X_test)           # gpk_extend, as the reference's other layouts
        return super().extend_sol(X_test)

    def Gram_matrix(self, kernel='Gaussian', kernel_parameter=0.2, nugget=1e-8, nugget_type='adaptive'):
        if self._family() != 'plain':
            require_gaussian_family(kernel, 'Nonlinear_elliptic2d with an operator or boundary conditions')
        ratios = self._assemble(kernel, kernel_parameter, nugget, nugget_type)
        if nugget_type == 'adaptive':
            self.ratio = ratios[0]

    def _posterior_unserved(self):
        if self.bc != 'dirichlet' or self.boundary_coeffs is not None:      # (what was asked for, points set or not: not the routing)
            return ('boundary functionals (bc / set_boundary_operator): gpk_assemble_cross has no rectangular evaluator for the layout of '
                    'gpk_assemble_bc yet')
        if self.operator is not None or self.domain_coeffs is not None:
            return ('domain operator (operator / set_domain_operator): gpk_assemble_cross has no rectangular evaluator for the layout of '
                    'gpk_assemble_op yet')
        return None

    # ---- relaxed (penalised) formulation, reference src/PDEs.py:137-201 ----
    def _relaxed_problem(self, pen_lambda):
        key = ('_prob_relaxed', float(pen_lambda))
        if getattr(self, '_prob_relaxed_key', None) != key:
            self._prob_relaxed = gpk.GNProblem(get_context(), 'Nonlinear_elliptic_relaxed', self.N_domain, self.N_boundary,
                                               self.rhs_f, self.bdy_g, self._dL,
                                               **dict(dict(p0=float(self.alpha), p1=float(self.m)), **self._nl_args()),
                                               pen_lambda=float(pen_lambda))
            self._prob_relaxed_key = key
        return self._prob_relaxed

    def loss_relaxed(self, z, pen_lambda):
        return get_context().gn_loss(self._relaxed_problem(pen_lambda), self._z(z))

    def grad_loss_relaxed(self, z, pen_lambda):
        return get_context().gn_hessian_grad(self._relaxed_problem(pen_lambda), self._z(z))[1]

    def GN_loss_relaxed(self, z, z_old, pen_lambda):
        z = onp.asarray(z, float); z_old = onp.asarray(z_old, float)
        Nd = self.N_domain
        v, w, w_old = z[:Nd], z[Nd:], z_old[Nd:]
        ss2 = -v + self._tau().dtau(w_old) * (w - w_old) - self.rhs_f
        return self._tri_loss(onp.concatenate([v, w, self.bdy_g])) + float(ss2 @ ss2) / pen_lambda

    def Hessian_GN_relaxed(self, z, z_old, pen_lambda):
        return get_context().gn_hessian_grad(self._relaxed_problem(pen_lambda), self._z(z_old))[0]

    def GN_relaxed_method(self, max_iter=3, step_size=1, initial_sol='rdm', pen_lambda=1e-10, print_hist=True):
        """initial_sol: 'rdm' (standard normal draw), or an ndarray with one value per unknown: the iterate to start from."""
        print(f'Relaxed approach: penalization parameter = {pen_lambda}')
        self._gn_solve(2 * self.N_domain, max_iter, step_size, initial_sol, print_hist, problem=lambda: self._relaxed_problem(pen_lambda),
                       finish=lambda sol: (onp.concatenate([sol, self.bdy_g]), sol[self.N_domain:]))


class Nonlinear_elliptic3d(_EllipticEquation):
    """-Delta u + alpha*u^m = f on a box in R^3, u = g on its six faces.  Same methods and attributes as Nonlinear_elliptic2d (elimination
    formulation only; the relaxed formulation is not offered); points are (n,3), callbacks take (x1, x2, x3).  The Gram matrix has the
    2-D elliptic block structure -- Laplacian on the domain points, delta on domain + boundary points, N = 2 N_domain + N_boundary --
    so the factorisation and the Gauss-Newton system ('Nonlinear_elliptic') are the 2-D ones; only the point-pair evaluator
    (gpk_assemble3d, gpk_extend_functionals3d) knows about the third coordinate.  GPK_STRUCTURED is ignored here: every step runs the
    reference's operation sequence.
    With operator=... / set_domain_operator() the equation is -psi[u] + alpha*u^m = f for any second-order linear operator psi with
    variable coefficients, and with bc='neumann' / 'robin' / set_boundary_operator() the boundary rows are first-order functionals
    (gpk_assemble_op3d, gpk_extend_functionals_op3d).  With axis 3 as time this covers u_t - nu Laplace_x u + alpha u^m = f in two space
    dimensions (parabolic_form(), sampled_pts(time_dependent=True)).
    Against Nonlinear_elliptic2d: two evaluator families (_family), points checked to be (n,3), the Gaussian kernels only, `ratio`
    stored for every nugget type, its own sampled_pts, no posterior variance, covariance or samples."""
    _layout = 'Nonlinear_elliptic3d'
    _dim = 3
    _deriv_names = ('value', 'd1', 'd2', 'd3', 'laplacian')
    _op_names = ('value', 'd1', 'd2', 'd3', 'd11', 'd12', 'd13', 'd22', 'd23', 'd33')    # rows of gpk_extend_functionals_op3d
    _laplacian_row = (0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0)
    _normals = staticmethod(boundary_normals3d)
    _xs, _count, _coeff_names = '(x1, x2, x3)', 'ten', '(c0, b1, b2, b3, a11, a12, a13, a22, a23, a33)'
    _structured_optin = False
    _bad_nugget_type = 'adaptive, identity or none'

    def __init__(self, alpha=1.0, m=3, bdy=None, rhs=None, domain=onp.array([[0, 1], [0, 1], [0, 1]]), bc='dirichlet', robin_beta=1.0,
                 operator=None, nonlinearity=None):
        """nonlinearity: the reaction term tau of -psi[u] + tau(u) = f as (name, parameters...), as for Nonlinear_elliptic2d; None:
        alpha u^m.  With parabolic_form() and ('cubic', -1, 0, 1) the equation is time-dependent Allen-Cahn.
        bc: the operator B on the boundary, whose prescribed value g = B u is what `bdy(x1, x2, x3)` returns -- 'dirichlet' B u = u;
        'neumann' B u = du/dn; 'robin' B u = robin_beta u + du/dn, n the outward unit normal (sample_points.boundary_normals3d).
        operator: a callable operator(x1, x2, x3) returning the ten coefficient arrays (c0, b1, b2, b3, a11, a12, a13, a22, a23, a33) of
        psi; the equation solved is then -psi[u] + alpha u^m = f (divergence_form3d(), parabolic_form(); a mixed coefficient multiplies
        its mixed derivative once).  With 'dirichlet' and None every call goes the way it always went."""
        super().__init__(alpha, m, bdy, rhs, domain, bc, robin_beta, operator, nonlinearity)

    def get_bd(self, x1, x2, x3):
        return self.bdy(x1, x2, x3)

    def get_rhs(self, x1, x2, x3):
        return self.rhs(x1, x2, x3)

    @staticmethod
    def _pts(X):
        X = onp.asarray(X, dtype=onp.float64)
        if X.ndim != 2 or X.shape[1] != 3:
            raise ValueError(f'points must have shape (n, 3), got {X.shape}')
        return X

    def sampled_pts(self, N_domain, N_boundary, sampled_type='random', time_dependent=False):
        """time_dependent: axis 3 is time -- no boundary points on the face x3 = max (sample_points.sampled_pts_rdm3d)"""
        kw = {'time_dependent': True} if time_dependent else {}
        if sampled_type == 'random':
            X_domain, X_boundary = sampled_pts_rdm3d(N_domain, N_boundary, self.domain, **kw)
        elif sampled_type == 'grid':
            X_domain, X_boundary = sampled_pts_grid3d(N_domain, N_boundary, self.domain, **kw)
        else:
            raise ValueError(f'sampled_type {sampled_type!r}: random or grid')
        self._set_points(X_domain, X_boundary)

    # ---- which evaluator serves this object: decided here and nowhere else -----------------------------------------------------------
    def _family(self):
        """'op': gpk_assemble_op3d / gpk_extend_functionals_op3d, with a domain operator or any non-Dirichlet condition (there is no
        'bc' family in three dimensions); 'plain': gpk_assemble3d / gpk_extend_functionals3d"""
        return 'plain' if self.domain_coeffs is None and self.boundary_coeffs is None else 'op'

    def _evaluate_gram(self, ctx, kernel, kernel_parameter, nugget, nugget_type):
        if self._family() == 'op':
            T, ratio = ctx.assemble_op3d(kernel, kernel_parameter, self.X_domain, self.X_boundary, self.domain_coeffs, self.boundary_coeffs,
                                         nugget, nugget_type)
        else:
            T, ratio = ctx.assemble3d(kernel, kernel_parameter, self.X_domain, self.X_boundary, nugget, nugget_type)
        return T, [ratio]

    def _fields(self, X_test, which):
        ctx = get_context()
        args = (self.kernel, self.kernel_parameter, X_test, self.X_domain, self.X_boundary)
        coeff = self._coeff(self._dL, self.sol_vec)
        if self._family() == 'op':
            return ctx.extend_functionals_op3d(*args, self.domain_coeffs, self.boundary_coeffs, coeff, which=which)
        return ctx.extend_functionals3d(*args, coeff, which=which)

    def Gram_matrix(self, kernel='Gaussian', kernel_parameter=0.3, nugget=1e-8, nugget_type='adaptive'):
        """kernel_parameter: sigma (Gaussian) or three length scales (anisotropic_Gaussian); stores the trace ratio in `ratio`"""
        require_gaussian_family(kernel, 'Nonlinear_elliptic3d')
        self.ratio = self._assemble(kernel, kernel_parameter, nugget, nugget_type)[0]

    def _posterior_unserved(self):
        return 'Nonlinear_elliptic3d: gpk_assemble_cross has no rectangular evaluator for the three-dimensional layouts yet'


class Burgers(_GPEquation):
    """u_t + alpha u u_x - nu u_xx = 0 on (t,x) in a rectangle (reference src/PDEs.py:211-350)."""
    _layout = 'Burgers'
    _system = 'Burgers'
    _time_dependent = True
    _blocks_per_point = 3

    def __init__(self, alpha=1.0, nu=0.2, bdy=None, rhs=None, domain=onp.array([[0, 1], [-1, 1]])):
        self.alpha = alpha
        self.nu = nu
        self.bdy = bdy
        self.rhs = rhs
        self.domain = domain

    _deriv_names = ('value', 'd1', 'd2', 'd2d2')              # u, u_t, u_x, u_xx

    def _gn_params(self):
        return float(self.alpha), float(self.nu), 0.0

    def Gram_matrix(self, kernel='anisotropic_Gaussian', kernel_parameter=[1 / 3, 1 / 20], nugget=1e-5, nugget_type='adaptive'):
        ratios = self._assemble(kernel, kernel_parameter, nugget, nugget_type)
        if nugget_type == 'adaptive':
            self.ratio = list(ratios[:3])

    def Hessian_GN(self, z):                 # ONE argument in the reference (src/PDEs.py:295)
        return self._hessian(z)

    def GN_method(self, max_iter=10, step_size=1, initial_sol='rdm', print_hist=True):
        """initial_sol: 'rdm' (standard normal draw), or an ndarray with one value per unknown: the iterate to start from."""
        self._gn_solve(self._n_unknowns(), max_iter, step_size, initial_sol, print_hist)

    def _sol_vec(self, sol):
        Nd = self.N_domain
        v0, v2, v3 = sol[:Nd], sol[Nd:2 * Nd], sol[2 * Nd:]
        return onp.concatenate((self.nu * v3 + self.rhs_f - self.alpha * v0 * v2, v2, v3, v0, self.bdy_g), axis=0), v0


class KdV(Burgers):
    """u_t + alpha u u_x + delta u_xxx = f on (t,x) in a rectangle: equations of Korteweg-de Vries type (solitons, shallow-water and
    plasma waves).  No counterpart in the reference.  It is the Burgers system with one row functional exchanged: rows
    [u_t; u_x; u_xxx; u] per domain point, then u on the boundary (the dispersive Gram layout, gpk_assemble_disp, Gaussian kernels only),
    unknowns [u | u_x | u_xxx], and GPK_GN_BURGERS with nu = -delta is the Gauss-Newton system -- loss, step, line search, the structured
    modes (GPK_STRUCTURED) and log_evidence are the base class's.  The boundary carries Dirichlet data only: the third boundary condition
    of the equation is not imposed, the minimum-norm interpolant supplies it.  posterior_variance / posterior_covariance /
    posterior_sample raise NotImplementedError (the layout has no rectangular cross evaluator yet)."""
    _layout = 'Dispersive'                                    # (no GPK_LAYOUT_* id: the evaluator is a call of its own)
    _system = 'Burgers'
    _deriv_names = ('value', 'd1', 'd2', 'd2d2d2')            # u, u_t, u_x, u_xxx: the rows gpk_pde_residual(GPK_GN_BURGERS) reads

    def __init__(self, alpha=6.0, delta=1.0, bdy=None, rhs=None, domain=onp.array([[0, 1], [-1, 1]])):
        super().__init__(alpha=alpha, nu=-delta, bdy=bdy, rhs=rhs, domain=domain)
        self.delta = delta

    def _gn_params(self):
        return float(self.alpha), -float(self.delta), 0.0

    def Gram_matrix(self, kernel='anisotropic_Gaussian', kernel_parameter=[1 / 3, 1 / 5], nugget=1e-8, nugget_type='adaptive'):
        """kernel: Gaussian or anisotropic_Gaussian (the Matern family and the periodic kernel are refused: the dispersive layout has no
        evaluator for them)"""
        require_gaussian_family(kernel, 'KdV.Gram_matrix')
        super().Gram_matrix(kernel, kernel_parameter, nugget, nugget_type)

    def _evaluate_gram(self, ctx, kernel, kernel_parameter, nugget, nugget_type):
        return ctx.assemble_disp(kernel, kernel_parameter, self.X_domain, self.X_boundary, nugget, nugget_type)

    def _initial(self, initial_sol, n):
        """'profile': the data at the first time of the domain held constant in time -- u = u_0(x) at every domain point, with u_x and
        u_xxx of u_0 by central differences of the boundary callback (a start, not data: O(h^2) is ample)"""
        if isinstance(initial_sol, str) and initial_sol == 'profile':
            t0 = float(self.domain[0][0])
            x = self.X_domain[:, 1]
            h = 1e-3 * (float(self.domain[1][1]) - float(self.domain[1][0]))
            u = {k: onp.asarray(eval_callback(self.get_bd, onp.full_like(x, t0), x + k * h), dtype=onp.float64) for k in (-2, -1, 0, 1, 2)}
            return onp.concatenate((u[0], (u[1] - u[-1]) / (2 * h), (u[2] - 2 * u[1] + 2 * u[-1] - u[-2]) / (2 * h ** 3)))
        return super()._initial(initial_sol, n)

    def GN_method(self, max_iter=10, step_size=1, initial_sol='rdm', print_hist=True):
        """initial_sol: 'rdm' (standard normal draw), 'profile' (the initial data held constant in time), or an ndarray with one value
        per unknown: the iterate to start from."""
        super().GN_method(max_iter, step_size, initial_sol, print_hist)

    def _sol_vec(self, sol):
        Nd = self.N_domain
        v0, v2, v3 = sol[:Nd], sol[Nd:2 * Nd], sol[2 * Nd:]
        return onp.concatenate((-self.delta * v3 + self.rhs_f - self.alpha * v0 * v2, v2, v3, v0, self.bdy_g), axis=0), v0

    def _fields(self, X_test, which):
        return get_context().extend_functionals_disp(self.kernel, self.kernel_parameter, X_test, self.X_domain, self.X_boundary,
                                                     self._coeff(self._dL, self.sol_vec), which=which)

    def extend_sol(self, X_test):
        X_test = onp.asarray(X_test, dtype=onp.float64)
        self.X_test = X_test
        self.N_test = X_test.shape[0]
        self.extended_sol = self._fields(X_test, ('value',)).download().reshape(-1)

    def _derivative_fields(self, X_test):
        return {'u': self._fields(X_test, self._deriv_names)}

    def extend_derivatives(self, X_test):
        """value, d1 = u_t, d2 = u_x and d2d2d2 = u_xxx of the GP solution at X_test (numpy arrays)"""
        return super().extend_derivatives(X_test)

    def PDE_residual(self, X_test):
        """u_t + alpha u u_x + delta u_xxx - f at X_test from the derivatives of the GP solution: gpk_pde_residual(GPK_GN_BURGERS) with
        (alpha, -delta) and u_xxx in the fourth row (f evaluated at X_test)"""
        return super().PDE_residual(X_test)

    def _posterior_unserved(self):
        return 'KdV: gpk_assemble_cross has no rectangular evaluator for the dispersive layout yet'


class Evolution1d(Burgers):
    """u_t + alpha u u_x + Q[u] = f on (t,x) in a rectangle with Q = c2 d_x^2 + c3 d_x^3 + c4 d_x^4 + c5 d_x^5 (constant coefficients):
    Kuramoto-Sivashinsky (c2 = c4 = 1), Kawahara (c3, c5), KdV-Burgers (c2 = -nu, c3 = delta), Benney-Lin (all four); viscous Burgers
    and KdV are special cases.  No counterpart in the reference.  It is the Burgers system with the row functional d_x^2 exchanged for
    Q: rows [u_t; u_x; Q u; u] per domain point, then the boundary functionals (the evolution Gram layout, gpk_assemble_evo, Gaussian
    kernels only), unknowns [u | u_x | Q u], and GPK_GN_BURGERS with nu = -1 is the Gauss-Newton system -- loss, step, line search, the
    structured modes (GPK_STRUCTURED) and log_evidence are the base class's.

    coeffs = (c2, c3, c4, c5), or equation = ('kuramoto_sivashinsky',) | ('kawahara', a, b): a u_xxx + b u_xxxxx |
    ('kdv_burgers', nu, delta): -nu u_xx + delta u_xxx | ('benney_lin', c2, c3, c4, c5).
    bc = 'dirichlet': u = bdy on every boundary point.  bc = 'clamped' (two conditions per wall, what an operator of fourth order
    takes): every boundary point with x at either end of the domain appears twice, behind the given points a second copy that carries
    u_x = bdy_x(t, x); the points of the initial line keep u alone.  set_boundary_operator(rows) sets any (N_boundary, 3) array of rows
    (c0, c1, c2): c0 u + c1 u_t + c2 u_x = bdy_g[b].
    posterior_variance / posterior_covariance / posterior_sample raise NotImplementedError (the layout has no rectangular cross
    evaluator)."""
    _layout = 'Evolution'                                     # (no GPK_LAYOUT_* id: the evaluator is a call of its own)
    _system = 'Burgers'
    _deriv_names = ('value', 'd1', 'd2', 'q')                 # u, u_t, u_x, Q[u]: the rows gpk_pde_residual(GPK_GN_BURGERS) reads
    _equations = {'kuramoto_sivashinsky': (0, lambda: (1.0, 0.0, 1.0, 0.0)), 'kawahara': (2, lambda a, b: (0.0, a, 0.0, b)),
                  'kdv_burgers': (2, lambda nu, delta: (-nu, delta, 0.0, 0.0)), 'benney_lin': (4, lambda *c: c)}

    def __init__(self, alpha=1.0, coeffs=None, equation=None, bdy=None, rhs=None, domain=onp.array([[0, 1], [-1, 1]]), bc='dirichlet',
                 bdy_x=None):
        super().__init__(alpha=alpha, nu=-1.0, bdy=bdy, rhs=rhs, domain=domain)
        if (coeffs is None) == (equation is None):
            raise ValueError('Evolution1d: give coeffs=(c2, c3, c4, c5) or equation=(name, ...), one of the two')
        if equation is not None:
            name, args = equation[0], tuple(float(v) for v in equation[1:])
            if name not in self._equations or len(args) != self._equations[name][0]:
                raise ValueError(f'Evolution1d: equation {equation!r}: one of ' + ', '.join(
                    f'({n!r}' + ', ..' * k + ')' for n, (k, _) in self._equations.items()))
            coeffs = self._equations[name][1](*args)
        c = onp.asarray(coeffs, dtype=onp.float64).ravel()
        if c.shape != (4,) or not onp.all(onp.isfinite(c)) or not onp.any(c != 0.0):
            raise ValueError(f'Evolution1d: coeffs must be four finite numbers (c2, c3, c4, c5), not all zero, got {coeffs!r}')
        if bc not in ('dirichlet', 'clamped'):
            raise ValueError(f"Evolution1d: bc must be 'dirichlet' or 'clamped', got {bc!r}")
        if bc == 'clamped' and bdy_x is None:
            raise ValueError("Evolution1d: bc='clamped' needs bdy_x(t, x), the data of u_x on the walls")
        self.coeffs = tuple(float(v) for v in c)
        self.bc = bc
        self.bdy_x = bdy_x
        self.boundary_coeffs = None

    def _gn_params(self):
        return float(self.alpha), -1.0, 0.0

    def _set_points(self, X_domain, X_boundary):
        X_boundary = self._pts(X_boundary)
        if self.bc != 'clamped':
            super()._set_points(X_domain, X_boundary)
            self.boundary_coeffs = None                       # a custom operator belongs to the points it was set for
            return
        lo, hi = float(self.domain[1][0]), float(self.domain[1][1])
        wall = onp.flatnonzero((X_boundary[:, 1] == lo) | (X_boundary[:, 1] == hi))
        n = X_boundary.shape[0]
        super()._set_points(X_domain, onp.concatenate([X_boundary, X_boundary[wall]]))
        self.wall_points = wall
        rows = onp.zeros((n + wall.size, 3))
        rows[:n, 0] = 1.0
        rows[n:, 2] = 1.0
        self.boundary_coeffs = rows
        gx = eval_callback(self.bdy_x, X_boundary[wall, 0], X_boundary[wall, 1])
        self.bdy_g = onp.concatenate((onp.asarray(self.bdy_g)[:n], onp.asarray(gx, dtype=onp.float64).reshape(-1)))

    def set_boundary_operator(self, coeffs):
        """Row b of coeffs (N_boundary, 3) = (c0, c1, c2): the condition at boundary point b reads c0 u + c1 u_t + c2 u_x = bdy_g[b]
        (bdy_g stays as it is: set it to the data of these conditions).  Call after the points are set; dropped when they change.
        Discards the Gram matrix and everything derived from it."""
        coeffs = onp.array(coeffs, dtype=onp.float64)
        if coeffs.shape != (self.N_boundary, 3):
            raise ValueError(f'coeffs must have shape ({self.N_boundary}, 3), got {coeffs.shape}')
        self.boundary_coeffs = coeffs
        self._drop_device_state()

    def Gram_matrix(self, kernel='anisotropic_Gaussian', kernel_parameter=[1 / 3, 1 / 5], nugget=1e-8, nugget_type='adaptive'):
        """kernel: Gaussian or anisotropic_Gaussian (the Matern family and the periodic kernel are refused: the evolution layout has no
        evaluator for them)"""
        require_gaussian_family(kernel, 'Evolution1d.Gram_matrix')
        super().Gram_matrix(kernel, kernel_parameter, nugget, nugget_type)

    def _evaluate_gram(self, ctx, kernel, kernel_parameter, nugget, nugget_type):
        return ctx.assemble_evo(kernel, kernel_parameter, self.coeffs, self.X_domain, self.X_boundary, self.boundary_coeffs, nugget, nugget_type)

    def _sol_vec(self, sol):
        Nd = self.N_domain
        v0, v2, v3 = sol[:Nd], sol[Nd:2 * Nd], sol[2 * Nd:]
        return onp.concatenate((-v3 + self.rhs_f - self.alpha * v0 * v2, v2, v3, v0, self.bdy_g), axis=0), v0

    def _fields(self, X_test, which):
        return get_context().extend_functionals_evo(self.kernel, self.kernel_parameter, self.coeffs, X_test, self.X_domain, self.X_boundary,
                                                    self.boundary_coeffs, self._coeff(self._dL, self.sol_vec), which=which)

    def extend_sol(self, X_test):
        X_test = onp.asarray(X_test, dtype=onp.float64)
        self.X_test = X_test
        self.N_test = X_test.shape[0]
        self.extended_sol = self._fields(X_test, ('value',)).download().reshape(-1)

    def _derivative_fields(self, X_test):
        return {'u': self._fields(X_test, self._deriv_names)}

    def extend_derivatives(self, X_test):
        """value, d1 = u_t, d2 = u_x and q = Q[u] of the GP solution at X_test (numpy arrays)"""
        return super().extend_derivatives(X_test)

    def PDE_residual(self, X_test):
        """u_t + alpha u u_x + Q[u] - f at X_test from the derivatives of the GP solution: gpk_pde_residual(GPK_GN_BURGERS) with
        (alpha, -1) and Q[u] in the fourth row (f evaluated at X_test)"""
        return super().PDE_residual(X_test)

    def _posterior_unserved(self):
        return 'Evolution1d: gpk_assemble_cross has no rectangular evaluator for the evolution layout'


class _GradientUnknowns(object):
    """Mixin of the equations whose unknowns per domain point are the value v_0 and k further fields v_1 .. v_k (derivatives of u) that
    have Gram rows of their own: _blocks_per_point = k + 1, unknowns [v_0 | v_1 | .. | v_k], rows [v_1; ..; v_k; PDE row; v_0; g] --
    Eikonal, Semilinear2d, MongeAmpere2d (k = 2), Semilinear3d (k = 3) and Quasilinear2d (k = 4).  A class says what its PDE row is, in two hooks:
    _pde_row(v) at an iterate and _pde_row_linearised(v, o), the row linearised at the iterate o and evaluated at v (v, o: tuples
    (v_0, .., v_k)).  Everything else about its Gauss-Newton iteration is written here, once."""
    _zero_start = True

    def _split(self, z):
        Nd, k = self.N_domain, self._blocks_per_point - 1
        return tuple(z[j * Nd:(j + 1) * Nd] for j in range(k)) + (z[k * Nd:],)

    def GN_loss(self, z, z_old):
        """the quadratic model of the loss at z_old, evaluated at z: ||L^{-1} (F(z_old) + A(z_old) (z - z_old))||^2"""
        z = onp.asarray(z, float); z_old = onp.asarray(z_old, float)
        v = self._split(z)
        return self._tri_loss(onp.concatenate([*v[1:], self._pde_row_linearised(v, self._split(z_old)), v[0], self.bdy_g]))

    def Hessian_GN(self, z, z_old):
        return self._hessian(z_old)          # hessian(GN_loss)(z, z_old) does not depend on z (quadratic in z)

    def _sol_vec(self, sol):
        v = self._split(sol)
        return onp.concatenate([*v[1:], self._pde_row(v), v[0], self.bdy_g]), v[0]


class Eikonal(_GradientUnknowns, _GPEquation):
    """|grad u|^2 = f^2 + eps*Delta u (reference src/PDEs.py:352-505)."""
    _layout = 'Eikonal'
    _system = 'Eikonal'
    _blocks_per_point = 3

    def __init__(self, eps=3, bdy=None, rhs=None, domain=onp.array([[0, 1], [0, 1]])):
        self.eps = eps
        self.bdy = bdy
        self.rhs = rhs
        self.domain = domain

    def _gn_params(self):
        return float(self.eps), 0.0, 0.0

    def Gram_matrix(self, kernel='Gaussian', kernel_parameter=0.2, nugget=1e-8, nugget_type='adaptive'):
        self._assemble(kernel, kernel_parameter, nugget, nugget_type)     # the reference does not store `ratio` here

    def _pde_row(self, v):
        _, v1, v2 = v
        return -(self.rhs_f ** 2 - v1 ** 2 - v2 ** 2) / self.eps

    def _pde_row_linearised(self, v, o):
        (_, v1, v2), (_, v1o, v2o) = v, o
        return -(self.rhs_f ** 2 - 2 * v1 * v1o - 2 * v2 * v2o) / self.eps      # the reference's spelling (src/PDEs.py:441-449)

    def GN_method(self, max_iter=3, step_size=1, initial_sol='rdm', print_hist=True):
        """initial_sol: 'rdm' (standard normal draw) or 'zero', or an ndarray with one value per unknown: the iterate to start from."""
        self._gn_solve(self._n_unknowns(), max_iter, step_size, initial_sol, print_hist)


class Semilinear2d(_GradientUnknowns, _GPEquation):
    """-eps Laplace(u) + N(u, grad u) = f on a rectangle, u = g on its boundary, with the gradient-dependent nonlinearity
    N(u, p, q) = u (a1 p + a2 q) + b (p^2 + q^2) + c1 u + c3 u^3 (src/nonlinearity.py, GradientNonlinearity): steady viscous Burgers /
    convection, viscous Hamilton-Jacobi and stationary KPZ, the regularised Eikonal equation (b = 1, f -> f^2), Allen-Cahn-type reaction
    terms next to any of them.  No counterpart in the reference.  The Gram matrix is the Eikonal layout's (rows d_1 u, d_2 u, Laplace(u),
    u per domain point), so all five kernels serve it; the Gauss-Newton system is GPK_GN_SEMILINEAR with unknowns [u | d_1 u | d_2 u].
    posterior_variance, posterior_covariance, posterior_sample and log_evidence are the base class's and work as for Eikonal
    (tests/test_gpu_semilinear.py).  GPK_STRUCTURED is ignored: the system has no structured form yet.
    Plain Gauss-Newton steps: convection-dominated settings (eps well below 0.1 with |a| = O(1)) do not converge; use eps >= 0.1."""
    _layout = 'Eikonal'
    _system = 'Semilinear2d'
    _blocks_per_point = 3
    _structured_optin = False

    def __init__(self, eps=0.1, nonlinearity=('burgers', 1.0, 1.0), bdy=None, rhs=None, domain=onp.array([[0, 1], [0, 1]])):
        """nonlinearity: a GradientNonlinearity, the five coefficients (a1, a2, b, c1, c3), or a preset -- ('burgers', a1, a2),
        ('hamilton_jacobi', b, c1), ('eikonal',).  eps: the viscosity, finite and not 0 (ValueError)."""
        if not (onp.isfinite(eps) and eps != 0):
            raise ValueError(f'Semilinear2d: eps must be finite and not 0 (the PDE row is divided by it), got {eps!r}')
        self.eps = eps
        self.nonlinearity = GradientNonlinearity.make(nonlinearity)
        self.bdy = bdy
        self.rhs = rhs
        self.domain = domain

    def _gn_params(self):
        return float(self.eps), 0.0, 0.0

    def _nl_args(self):
        return dict(gq=self.nonlinearity.params)

    def Gram_matrix(self, kernel='Gaussian', kernel_parameter=0.2, nugget=1e-8, nugget_type='adaptive'):
        """kernel: Gaussian, anisotropic_Gaussian, Matern52, Matern72 or Matern92 (the Eikonal layout takes all five)"""
        self._assemble(kernel, kernel_parameter, nugget, nugget_type)

    def _pde_row(self, v):
        return (self.nonlinearity.N(*v) - self.rhs_f) / self.eps

    def _pde_row_linearised(self, v, o):
        (v0, v1, v2), (u, p, q) = v, o
        Nu, Np, Nq = self.nonlinearity.dN(u, p, q)
        return (self.nonlinearity.N(u, p, q) + Nu * (v0 - u) + Np * (v1 - p) + Nq * (v2 - q) - self.rhs_f) / self.eps

    def GN_method(self, max_iter=8, step_size=1, initial_sol='zero', print_hist=True):
        """initial_sol: 'zero', 'rdm' (standard normal draw), or an ndarray with one value per unknown: the iterate to start from."""
        self._gn_solve(self._n_unknowns(), max_iter, step_size, initial_sol, print_hist)

    def _residual(self, fields_u, fields_a, rhs):
        """-eps Laplace(u) + N(u, grad u) - f on rows of the extension (gpk_pde_residual_sl)"""
        return get_context().pde_residual_sl(self.eps, self.nonlinearity.params, fields_u, rhs).download().reshape(-1)


class MongeAmpere2d(_GradientUnknowns, _GPEquation):
    """det D^2 u = f (f > 0) on a rectangle, u = g on its boundary: the Monge-Ampere equation, convex solution.  Fully nonlinear (the
    equation is nonlinear in the second derivatives), no counterpart in the reference.  Solved in the convex-branch form
        Laplace(u) = sqrt((D u)^2 + (M u)^2 + 4 f),   D = d_11 - d_22,  M = 2 d_12      ((Laplace u)^2 = (D u)^2 + (M u)^2 + 4 det D^2 u)
    -- no division, smooth for f > 0, and the positive root selects the convex branch, so the zero start is admissible.  The Gram matrix
    is the Hessian layout's (rows D u, M u, Laplace(u), u per domain point, then u on the boundary: gpk_assemble_hess, Gaussian kernels
    only), the Gauss-Newton system is GPK_GN_MONGE_AMPERE with unknowns [u | D u | M u].  Where an iterate makes the radicand negative the
    loss is NaN, reported like every other NaN.  log_evidence is the base class's; posterior_variance / posterior_covariance /
    posterior_sample raise NotImplementedError (the layout has no rectangular cross evaluator yet).  GPK_STRUCTURED is ignored: the
    structured form is not served yet.  eq.line_search (src/linesearch.py) is honoured; DESIGN.md section K names a configuration that needs it."""
    _layout = 'Hessian'
    _system = 'MongeAmpere2d'
    _blocks_per_point = 3
    _structured_optin = False
    _deriv_names = ('value', 'd1', 'd2', 'd11', 'd12', 'd22')

    def __init__(self, bdy=None, rhs=None, domain=onp.array([[0, 1], [0, 1]])):
        self.bdy = bdy
        self.rhs = rhs
        self.domain = domain

    def _gn_params(self):
        return 0.0, 0.0, 0.0

    def Gram_matrix(self, kernel='Gaussian', kernel_parameter=0.3, nugget=1e-8, nugget_type='adaptive'):
        """kernel: Gaussian or anisotropic_Gaussian (the Matern family is refused: the Hessian layout has no evaluator for it)"""
        require_gaussian_family(kernel, 'MongeAmpere2d.Gram_matrix')
        ratios = self._assemble(kernel, kernel_parameter, nugget, nugget_type)
        if nugget_type == 'adaptive':
            self.ratio = list(ratios[:3])

    def _evaluate_gram(self, ctx, kernel, kernel_parameter, nugget, nugget_type):
        return ctx.assemble_hess(kernel, kernel_parameter, self.X_domain, self.X_boundary, nugget, nugget_type)

    def _root(self, v1, v2):
        with onp.errstate(invalid='ignore'):
            return onp.sqrt(v1 * v1 + v2 * v2 + 4.0 * self.rhs_f)

    def _pde_row(self, v):
        return self._root(v[1], v[2])

    def _pde_row_linearised(self, v, o):
        (_, v1, v2), (_, p, q) = v, o
        s = self._root(p, q)
        return s + (p * (v1 - p) + q * (v2 - q)) / s

    def GN_method(self, max_iter=8, step_size=1, initial_sol='zero', print_hist=True):
        """initial_sol: 'zero', 'rdm' (standard normal draw), or an ndarray with one value per unknown: the iterate to start from."""
        self._gn_solve(self._n_unknowns(), max_iter, step_size, initial_sol, print_hist)

    def extend_sol(self, X_test):
        ctx = get_context()
        X_test = onp.asarray(X_test, dtype=onp.float64)
        coeff = self._coeff(self._dL, self.sol_vec)
        self.X_test = X_test
        self.N_test = X_test.shape[0]
        self.extended_sol = ctx.extend_functionals_hess(self.kernel, self.kernel_parameter, X_test, self.X_domain, self.X_boundary,
                                                        coeff, which=('value',)).download().reshape(-1)

    def _derivative_fields(self, X_test):
        coeff = self._coeff(self._dL, self.sol_vec)
        return {'u': get_context().extend_functionals_hess(self.kernel, self.kernel_parameter, X_test, self.X_domain, self.X_boundary,
                                                           coeff, which=self._deriv_names)}

    def extend_derivatives(self, X_test):
        """value, d1, d2, d11, d12 and d22 of the GP solution at X_test (numpy arrays)"""
        return super().extend_derivatives(X_test)

    def PDE_residual(self, X_test):
        """det D^2 u - f at X_test from the second derivatives of the GP solution (gpk_pde_residual_ma; f evaluated at X_test)"""
        X_test = onp.asarray(X_test, dtype=onp.float64)
        coeff = self._coeff(self._dL, self.sol_vec)
        hess = get_context().extend_functionals_hess(self.kernel, self.kernel_parameter, X_test, self.X_domain, self.X_boundary,
                                                     coeff, which=('d11', 'd12', 'd22'))
        rhs = eval_callback(self.get_rhs, X_test[:, 0], X_test[:, 1])
        self.test_residual = get_context().pde_residual_ma(hess, rhs).download().reshape(-1)
        return self.test_residual

    def _posterior_unserved(self):
        return 'MongeAmpere2d: gpk_assemble_cross has no rectangular evaluator for the Hessian layout yet'


class Quasilinear2d(_GradientUnknowns, _GPEquation):
    """A quasilinear equation on a rectangle, u = g on its boundary: its second-order coefficients depend on grad u.  No counterpart in
    the reference.  equation (src/quasilinear.py):
        ('mean_curvature', kappa)   div(grad u / sqrt(1 + |grad u|^2)) = f + kappa u     (minimal surface, prescribed mean curvature, capillarity)
        ('p_laplace', m, delta)     div((delta^2 + |grad u|^2)^((m-2)/2) grad u) = f     (m > 0, delta > 0; m = 2: Poisson's equation)
        ('gauss_curvature', e)      det D^2 u = f (1 + |grad u|^2)^e, f > 0, convex      (e = 2: prescribed Gauss curvature; e = 0: Monge-Ampere)
    Each is solved for the Laplacian, Laplace(u) = G(x; u, grad u, D u, M u) with D = d_11 - d_22, M = 2 d_12, so the zero start is
    admissible.  The Gram matrix is the 2-jet layout's (rows d_1 u, d_2 u, D u, M u, Laplace(u), u per domain point, then u on the
    boundary: gpk_assemble_jet2, Gaussian kernels only), the Gauss-Newton system is GPK_GN_QUASILINEAR with unknowns
    [u | d_1 u | d_2 u | D u | M u].  Dirichlet data only.  log_evidence and eq.line_search (src/linesearch.py) are the base class's;
    posterior_variance / posterior_covariance / posterior_sample raise NotImplementedError (no rectangular cross evaluator for the
    2-jet layout).  GPK_STRUCTURED is ignored: the system has no structured form."""
    _layout = 'Jet2'
    _system = 'Quasilinear2d'
    _blocks_per_point = 5
    _structured_optin = False
    _deriv_names = ('value', 'd1', 'd2', 'd11', 'd12', 'd22')

    def __init__(self, equation=('mean_curvature', 0.0), bdy=None, rhs=None, domain=onp.array([[0, 1], [0, 1]])):
        self.equation = QuasilinearEquation.make(equation)
        self.bdy = bdy
        self.rhs = rhs
        self.domain = domain

    def _gn_params(self):
        return self.equation.params[0], self.equation.params[1], 0.0

    def _nl_args(self):
        return dict(nonlin=self.equation.id, p2=self.equation.params[2])

    def Gram_matrix(self, kernel='Gaussian', kernel_parameter=0.3, nugget=1e-8, nugget_type='adaptive'):
        """kernel: Gaussian or anisotropic_Gaussian (the Matern family and the periodic kernel are refused: the 2-jet layout has no
        evaluator for them)"""
        require_gaussian_family(kernel, 'Quasilinear2d.Gram_matrix')
        ratios = self._assemble(kernel, kernel_parameter, nugget, nugget_type)
        if nugget_type == 'adaptive':
            self.ratio = list(ratios[:5])

    def _evaluate_gram(self, ctx, kernel, kernel_parameter, nugget, nugget_type):
        return ctx.assemble_jet2(kernel, kernel_parameter, self.X_domain, self.X_boundary, nugget, nugget_type)

    def _pde_row(self, v):
        return self.equation.G(self.rhs_f, *v)

    def _pde_row_linearised(self, v, o):
        return self.equation.G(self.rhs_f, *o) + sum(d * (a - b) for d, a, b in zip(self.equation.dG(self.rhs_f, *o), v, o))

    def GN_method(self, max_iter=8, step_size=1, initial_sol='zero', print_hist=True):
        """initial_sol: 'zero', 'rdm' (standard normal draw), or an ndarray with one value per unknown: the iterate to start from."""
        self._gn_solve(self._n_unknowns(), max_iter, step_size, initial_sol, print_hist)

    def extend_sol(self, X_test):
        ctx = get_context()
        X_test = onp.asarray(X_test, dtype=onp.float64)
        coeff = self._coeff(self._dL, self.sol_vec)
        self.X_test = X_test
        self.N_test = X_test.shape[0]
        self.extended_sol = ctx.extend_functionals_jet2(self.kernel, self.kernel_parameter, X_test, self.X_domain, self.X_boundary,
                                                        coeff, which=('value',)).download().reshape(-1)

    def _derivative_fields(self, X_test):
        coeff = self._coeff(self._dL, self.sol_vec)
        return {'u': get_context().extend_functionals_jet2(self.kernel, self.kernel_parameter, X_test, self.X_domain, self.X_boundary,
                                                           coeff, which=self._deriv_names)}

    def extend_derivatives(self, X_test):
        """value, d1, d2, d11, d12 and d22 of the GP solution at X_test (numpy arrays)"""
        return super().extend_derivatives(X_test)

    def _residual(self, fields_u, fields_a, rhs):
        """the equation in its divergence / determinant form on the six rows of the extension (gpk_pde_residual_ql)"""
        return get_context().pde_residual_ql(self.equation.id, self.equation.params, fields_u, rhs).download().reshape(-1)

    def _posterior_unserved(self):
        return 'Quasilinear2d: no rectangular cross evaluator for the 2-jet layout'


class Semilinear3d(_GradientUnknowns, Nonlinear_elliptic3d):
    """-psi[u] + N(u, grad u) = f on a box in R^3, B u = g on its faces, with the gradient-dependent nonlinearity
    N(u, g) = u (a1 g1 + a2 g2 + a3 g3) + b1 g1^2 + b2 g2^2 + b3 g3^2 + c1 u + c3 u^3 (src/nonlinearity.py, GradientNonlinearity3d): the
    3-D counterpart of Semilinear2d -- viscous Burgers / convection, viscous Hamilton-Jacobi and KPZ, the regularised Eikonal equation --
    and, with axis 3 as time (operator=parabolic_form(nu), sampled_pts(time_dependent=True), a3 = b3 = 0), their time-dependent forms in
    two space dimensions: u_t - nu Laplace_x u + u (a1 u_x1 + a2 u_x2) = f, u_t - nu Laplace_x u + b |grad_x u|^2 = f.  No counterpart in
    the reference.  psi is eps Laplace by default; operator= / set_domain_operator and bc= / set_boundary_operator behave exactly as on
    Nonlinear_elliptic3d, whose points, samplers, callbacks and operator handling this class inherits.  The Gram matrix is the gradient
    layout's (rows d_1 u, d_2 u, d_3 u, psi[u], u per domain point, then the boundary functionals: gpk_assemble_grad3d, Gaussian kernels
    only), the Gauss-Newton system is GPK_GN_SEMILINEAR3D with unknowns [u | d_1 u | d_2 u | d_3 u].  log_evidence is the base class's;
    posterior_variance / posterior_covariance / posterior_sample raise NotImplementedError (the layout has no rectangular cross evaluator);
    there is no relaxed formulation.  eq.line_search (src/linesearch.py) is honoured.  Plain Gauss-Newton steps: convection-dominated
    settings do not converge from the zero start, as for Semilinear2d."""
    _layout = 'Gradient3d'
    _system = 'Semilinear3d'
    _blocks_per_point = 4

    def __init__(self, eps=0.1, nonlinearity=('burgers', 1.0, 1.0), bdy=None, rhs=None, domain=onp.array([[0, 1], [0, 1], [0, 1]]),
                 bc='dirichlet', robin_beta=1.0, operator=None):
        """nonlinearity: a GradientNonlinearity3d, the eight coefficients (a1, a2, a3, b1, b2, b3, c1, c3), or a preset -- ('burgers', a1,
        a2[, a3]), ('hamilton_jacobi', b1, b2[, b3]), ('eikonal',).  eps: psi = eps Laplace when no operator is given (finite; not read
        otherwise).  bc, robin_beta, operator: as for Nonlinear_elliptic3d."""
        if operator is None and not onp.isfinite(eps):
            raise ValueError(f'Semilinear3d: eps must be finite, got {eps!r}')
        _EllipticEquation.__init__(self, None, None, bdy, rhs, domain, bc, robin_beta, operator, None)
        del self.alpha, self.m                                 # (the elliptic classes' reaction term: this equation has none)
        self.eps = eps
        self.nonlinearity = GradientNonlinearity3d.make(nonlinearity)

    def _gn_params(self):
        return 0.0, 0.0, 0.0                                   # (p0, p1, pen_lambda carry a3, b2, b3: GNProblem fills them from gq8)

    def _nl_args(self):
        return dict(gq8=self.nonlinearity.params)

    def _tau(self):
        raise NotImplementedError('Semilinear3d has no reaction term tau(u): its nonlinearity is N(u, grad u)')

    # ---- psi: the operator given, or eps Laplace ---------------------------------------------------------------------------------------
    def _default_psi(self, n):
        return onp.tile(float(self.eps) * onp.asarray(self._laplacian_row), (n, 1))

    def _set_points(self, X_domain, X_boundary):
        super()._set_points(X_domain, X_boundary)
        self._psi_is_default = self.domain_coeffs is None
        if self._psi_is_default:
            self.domain_coeffs = self._default_psi(self.N_domain)

    def set_domain_operator(self, coeffs):
        super().set_domain_operator(coeffs)
        self._psi_is_default = False

    # ---- one evaluator family ----------------------------------------------------------------------------------------------------------
    def _family(self):
        return 'grad'

    def _evaluate_gram(self, ctx, kernel, kernel_parameter, nugget, nugget_type):
        return ctx.assemble_grad3d(kernel, kernel_parameter, self.X_domain, self.X_boundary, self.domain_coeffs, self.boundary_coeffs,
                                   nugget, nugget_type)

    def _fields(self, X_test, which):
        coeff = self._coeff(self._dL, self.sol_vec)
        return get_context().extend_functionals_grad3d(self.kernel, self.kernel_parameter, X_test, self.X_domain, self.X_boundary,
                                                       self.domain_coeffs, self.boundary_coeffs, coeff, which=which)

    def Gram_matrix(self, kernel='Gaussian', kernel_parameter=0.3, nugget=1e-8, nugget_type='adaptive'):
        """kernel_parameter: sigma (Gaussian) or three length scales (anisotropic_Gaussian); stores the four trace ratios in `ratio`"""
        require_gaussian_family(kernel, 'Semilinear3d')
        self.ratio = list(self._assemble(kernel, kernel_parameter, nugget, nugget_type)[:4])

    # ---- Gauss-Newton ------------------------------------------------------------------------------------------------------------------
    def _pde_row(self, v):
        return self.nonlinearity.N(*v) - self.rhs_f

    def _pde_row_linearised(self, v, o):
        d = self.nonlinearity.dN(*o)
        return self.nonlinearity.N(*o) + sum(dk * (vk - ok) for dk, vk, ok in zip(d, v, o)) - self.rhs_f

    def GN_method(self, max_iter=8, step_size=1, initial_sol='zero', print_hist=True):
        """initial_sol: 'zero', 'rdm' (standard normal draw), or an ndarray with one value per unknown: the iterate to start from."""
        self._gn_solve(self._n_unknowns(), max_iter, step_size, initial_sol, print_hist)

    # ---- residual ----------------------------------------------------------------------------------------------------------------------
    def PDE_residual(self, X_test, coeffs_t=None):
        """pointwise residual -psi_t[u] + N(u, grad u) - f at X_test from the derivatives of the GP solution (gpk_pde_residual_sl3d; rhs
        evaluated at X_test): psi_t from the callable `operator`, eps Laplace when none was given, or coeffs_t (Nt, 10) (needed when the
        operator was set per point; ValueError otherwise)"""
        X_test = self._pts(X_test)
        n = len(self._op_names)
        if coeffs_t is None:
            if self.operator is not None:
                coeffs_t = self._operator_at(X_test)
            elif self._psi_is_default:
                coeffs_t = self._default_psi(X_test.shape[0])
            else:
                raise ValueError('the domain operator was set per point (set_domain_operator): pass its coefficients at the test '
                                 f'points as coeffs_t (Nt,{n})')
        coeffs_t = onp.asarray(coeffs_t, dtype=onp.float64)
        if coeffs_t.shape != (X_test.shape[0], n):
            raise ValueError(f'coeffs_t must have shape ({X_test.shape[0]}, {n}), got {coeffs_t.shape}')
        rows = self._fields(X_test, self._op_names).download().reshape(n, -1)
        psi = (coeffs_t.T * rows).sum(axis=0)                     # psi_t[u]: a combination of the rows, per test point
        rhs = eval_callback(self.get_rhs, *self._columns(X_test))
        self.test_residual = get_context().pde_residual_sl3d(self.nonlinearity.params, rows[:4], psi, rhs).download().reshape(-1)
        return self.test_residual

    def _posterior_unserved(self):
        return 'Semilinear3d: gpk_assemble_cross has no rectangular evaluator for the gradient layout in three dimensions'
