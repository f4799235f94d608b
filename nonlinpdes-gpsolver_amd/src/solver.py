"""solver_GP facade with the reference's interface (src/solver.py:41-206): set_equation -> auto_sample -> solve -> test
-> errors, same bracket-tagged log lines.  Plot helpers use matplotlib when it is importable (no LaTeX requirement)."""
import numpy as onp

from ._runtime import get_context
from .InverseProblems import Darcy_flow2d
from .PDEs import Burgers, Eikonal, Evolution1d, KdV, MongeAmpere2d, Nonlinear_elliptic2d, Nonlinear_elliptic3d, Quasilinear2d, Semilinear2d, Semilinear3d
from .quasilinear import QuasilinearEquation
from .nonlinearity import GradientNonlinearity, Nonlinearity


def _operator_of(c):
    """cfg.operator as the equation class takes it: a callable -- operator(x1, x2) -> six coefficient arrays in two dimensions,
    operator(x1, x2, x3) -> ten in three -- or None for the Laplacian (absent, None, or the name 'laplace', which is what a driver's
    command line leaves there by default)"""
    op = getattr(c, 'operator', None)
    if op is None or (isinstance(op, str) and op == 'laplace'):
        return None
    if not callable(op):
        raise ValueError(f"cfg.operator {op!r}: a callable operator(x1, x2) / operator(x1, x2, x3), None or 'laplace'")
    return op


def _operator_lines(c):
    """header line of a variable-coefficient domain operator (nothing for the Laplacian: the reference's header)"""
    if _operator_of(c) is not None:
        if _tau_of(c) is not None:
            return ['[Domain operator] - psi[u] + tau(u) = f, psi a second-order operator with variable coefficients given by the user']
        return ['[Domain operator] - psi[u] + alpha*u^m = f, psi a second-order operator with variable coefficients given by the user']
    return []


def _tau_of(c):
    """cfg.nonlinearity as a Nonlinearity, or None: the power law alpha*u^m of cfg.alpha, cfg.m with the reference's header (absent, None, or
    the name 'power', which is what a driver's command line leaves there by default)"""
    spec = getattr(c, 'nonlinearity', None)
    if spec is None or (isinstance(spec, str) and spec == 'power'):
        return None
    return Nonlinearity.make(spec)


_QL_FORMS = {'mean_curvature': 'div(grad u / sqrt(1 + |grad u|^2)) = f + kappa*u',
             'p_laplace': 'div((delta^2 + |grad u|^2)^((m-2)/2) grad u) = f',
             'gauss_curvature': 'det D^2 u = f*(1 + |grad u|^2)^e, convex solution'}


def _quasilinear_of(c):
    """the QuasilinearEquation of a Quasilinear2d configuration: cfg.equation, else the class's default ('mean_curvature', 0)"""
    return QuasilinearEquation.make(getattr(c, 'equation', None) or ('mean_curvature', 0.0))


def _gradient_nl_of(c):
    """the GradientNonlinearity of a Semilinear2d configuration: cfg.nonlinearity (an instance, five coefficients or a preset), else
    cfg.nl_params = (a1, a2, b, c1, c3), else the class's default ('burgers', 1, 1)"""
    spec = getattr(c, 'nonlinearity', None)
    if spec is None:
        spec = getattr(c, 'nl_params', None)
    return GradientNonlinearity.make(('burgers', 1.0, 1.0) if spec is None else spec)


def _gradient_nl3_of(c):
    """the GradientNonlinearity3d of a Semilinear3d configuration: cfg.nonlinearity (an instance, eight coefficients or a preset), else
    cfg.nl_params = (a1, a2, a3, b1, b2, b3, c1, c3), else the class's default ('burgers', 1, 1)"""
    from .nonlinearity import GradientNonlinearity3d
    spec = getattr(c, 'nonlinearity', None)
    if spec is None:
        spec = getattr(c, 'nl_params', None)
    return GradientNonlinearity3d.make(('burgers', 1.0, 1.0) if spec is None else spec)


def _form_line(c, default):
    """the [Equation form] line: `default` (the reference's text) unless a reaction term is set, which is then named"""
    tau = _tau_of(c)
    if tau is None:
        return default
    lhs = '- \\Delta u' if _operator_of(c) is None else '- psi[u]'
    return f'[Equation form] {lhs} + tau(u) = f, tau(u) = {tau.describe()}'


def _param_line(c):
    tau = _tau_of(c)
    if tau is None:
        return f'[Equation parameter] alpha = {c.alpha}, m = {c.m}'
    return f'[Equation parameter] nonlinearity = {tau.name}, parameters = {tau.raw}'


def _elliptic_kwargs(c):
    """constructor arguments both elliptic classes read from the configuration"""
    kw = dict(alpha=c.alpha, m=c.m, bc=getattr(c, 'bc', 'dirichlet'), robin_beta=getattr(c, 'robin_beta', 1.0), operator=_operator_of(c))
    if _tau_of(c) is not None:
        kw['nonlinearity'] = _tau_of(c)
    return kw


def _time_lines(c):
    """header line of a space-time problem in the 3-D class (cfg.time_dependent: axis 3 is time)"""
    if getattr(c, 'time_dependent', False):
        return ['[Time axis] x3 is time: no collocation data on the face x3 = max']
    return []


def _bc_lines(c):
    """header line of a non-Dirichlet boundary operator (nothing for Dirichlet: the reference's header)"""
    bc = getattr(c, 'bc', 'dirichlet')
    if bc == 'neumann':
        return ['[Boundary condition] Neumann: du/dn = g']
    if bc == 'robin':
        return [f"[Boundary condition] Robin: beta*u + du/dn = g, beta = {getattr(c, 'robin_beta', 1.0)}"]
    return []


# PDE_type -> (factory, header lines printed by set_equation)
_EQUATIONS = {
    'Nonlinear_elliptic': (
        # (cfg.bc / cfg.robin_beta: Neumann / Robin boundary operator; configurations without them are Dirichlet, as in the reference;
        #  cfg.operator: a callable operator(x1, x2) -> six coefficient arrays, or None / absent = the Laplacian, as in the reference)
        #  cfg.nonlinearity: (name, parameters...) of the reaction term, or None / absent = alpha*u^m, as in the reference
        lambda c, **k: Nonlinear_elliptic2d(**_elliptic_kwargs(c), **k),
        lambda c: ['[Equation type] Nonlinear elliptic equation', _form_line(c, '[Equation form] - \\Delta u + alpha*u^m = f')]
        + _operator_lines(c) + _bc_lines(c),
        _param_line),
    'Nonlinear_elliptic3d': (
        # (cfg.bc / cfg.robin_beta / cfg.operator as for two dimensions, the callable taking (x1, x2, x3) and returning ten arrays;
        #  cfg.time_dependent: axis 3 is time, auto_sample() places no boundary points on the face x3 = max)
        lambda c, **k: Nonlinear_elliptic3d(**_elliptic_kwargs(c), **k),
        lambda c: ['[Equation type] Nonlinear elliptic equation in three space dimensions',
                   _form_line(c, '[Equation form] - \\Delta u + alpha*u^m = f' if _operator_of(c) is None
                              else '[Equation form] - psi[u] + alpha*u^m = f')]
        + _operator_lines(c) + _time_lines(c) + _bc_lines(c),
        _param_line),
    'Burgers': (
        lambda c, **k: Burgers(alpha=c.alpha, nu=c.nu, **k),
        lambda c: ['[Equation type] Burgers equation', '[Equation form] u_t+ alpha u u_x- nu u_xx=0'],
        lambda c: f'[Equation parameter] alpha = {c.alpha}, m = {c.nu}'),        # sic: the reference prints "m ="
    'KdV': (
        lambda c, **k: KdV(alpha=c.alpha, delta=c.delta, **k),
        lambda c: ['[Equation type] Korteweg-de Vries equation (dispersive)', '[Equation form] u_t+ alpha u u_x+ delta u_xxx=f'],
        lambda c: f'[Equation parameter] alpha = {c.alpha}, delta = {c.delta}'),
    'Evolution1d': (
        # cfg: alpha; equation (name, ...) or coeffs (c2, c3, c4, c5); bc 'dirichlet' | 'clamped' and, for 'clamped', bdy_x: the callable u_x(t, x)
        lambda c, **k: Evolution1d(alpha=c.alpha, coeffs=getattr(c, 'coeffs', None), equation=getattr(c, 'equation', None),
                                   bc=getattr(c, 'bc', 'dirichlet'), bdy_x=getattr(c, 'bdy_x', None), **k),
        lambda c: ['[Equation type] evolution equation with a general spatial operator',
                   '[Equation form] u_t+ alpha u u_x+ c2 u_xx+ c3 u_xxx+ c4 u_xxxx+ c5 u_xxxxx=f'],
        lambda c: f"[Equation parameter] alpha = {c.alpha}, " + (f"coeffs = {tuple(c.coeffs)}" if getattr(c, 'coeffs', None) is not None
                                                                  else f"equation = {tuple(c.equation)}") + f", bc = {getattr(c, 'bc', 'dirichlet')}"),
    'Eikonal': (
        lambda c, **k: Eikonal(eps=c.eps, **k),
        lambda c: ['[Equation type] Eikonal equation', '[Equation form] |grad u|^2 = f + eps*Delta u'],
        lambda c: f'[Equation parameter] eps = {c.eps}'),
    'Semilinear2d': (
        # (cfg.eps; cfg.nonlinearity: a GradientNonlinearity, five coefficients or a preset; or cfg.nl_params = (a1, a2, b, c1, c3))
        lambda c, **k: Semilinear2d(eps=c.eps, nonlinearity=_gradient_nl_of(c), **k),
        lambda c: ['[Equation type] Semilinear equation with a gradient-dependent nonlinearity',
                   f'[Equation form] - eps*Delta u + N(u, grad u) = f, N = {_gradient_nl_of(c).describe()}'],
        lambda c: f'[Equation parameter] eps = {c.eps}, (a1, a2, b, c1, c3) = {_gradient_nl_of(c).params}'),
    'Semilinear3d': (
        # (cfg.eps; cfg.nonlinearity / cfg.nl_params as for Semilinear2d with eight coefficients; cfg.bc / cfg.robin_beta / cfg.operator /
        #  cfg.time_dependent as for Nonlinear_elliptic3d)
        lambda c, **k: Semilinear3d(eps=getattr(c, 'eps', 0.1), nonlinearity=_gradient_nl3_of(c), bc=getattr(c, 'bc', 'dirichlet'),
                                    robin_beta=getattr(c, 'robin_beta', 1.0), operator=_operator_of(c), **k),
        lambda c: ['[Equation type] Semilinear equation with a gradient-dependent nonlinearity in three dimensions',
                   ('[Equation form] - eps*Delta u' if _operator_of(c) is None else '[Equation form] - psi[u]')
                   + f' + N(u, grad u) = f, N = {_gradient_nl3_of(c).describe()}']
        + _operator_lines(c) + _time_lines(c) + _bc_lines(c),
        lambda c: f"[Equation parameter] eps = {getattr(c, 'eps', 0.1)}, (a1, a2, a3, b1, b2, b3, c1, c3) = {_gradient_nl3_of(c).params}"),
    'MongeAmpere2d': (
        lambda c, **k: MongeAmpere2d(**k),
        lambda c: ['[Equation type] Monge-Ampere equation (fully nonlinear)',
                   '[Equation form] det D^2 u = f, convex solution: Delta u = sqrt((u_11 - u_22)^2 + (2 u_12)^2 + 4 f)'],
        None),
    'Quasilinear2d': (
        # (cfg.equation: ('mean_curvature', kappa) | ('p_laplace', m, delta) | ('gauss_curvature', e), or a QuasilinearEquation)
        lambda c, **k: Quasilinear2d(equation=_quasilinear_of(c), **k),
        lambda c: ['[Equation type] Quasilinear equation (second-order coefficients depend on grad u)',
                   '[Equation form] ' + _QL_FORMS[_quasilinear_of(c).kind]],
        lambda c: f'[Equation parameter] {_quasilinear_of(c).kind}: (p0, p1, p2) = {_quasilinear_of(c).params}'),
    'Darcy_flow2d': (
        lambda c, **k: Darcy_flow2d(**k),
        lambda c: ['[Inverse problem type] Darcy flow 2d', '[Inverse problem form] -div(a grad u) = f, infer a from f and some observed u'],
        None),
}


# every bracket-tagged log line of the facade, keyed by event (texts are the reference's, src/solver.py:41-206)
_LOG = {
    'start': '\n Solver started',
    'domain': '[Equation domain] [{d[0][0]},{d[0][1]}]*[{d[1][0]},{d[1][1]}]',
    'domain3d': '[Equation domain] [{d[0][0]},{d[0][1]}]*[{d[1][0]},{d[1][1]}]*[{d[2][0]},{d[2][1]}]',
    'data': '[Equation data] Right hand side and boundary values set by the user',
    'pts_user': '[Sample points] Collocation points sampled, specified by the user',
    'pts_auto': '[Sample points] Collocation points sampled, type {kind}',
    'pts_n': '[Sample points] N_domain = {e.N_domain}, N_boundary = {e.N_boundary}',
    'pts_n_ip': '[Sample points] N_domain = {e.N_domain}, N_boundary = {e.N_boundary}, N_data = {e.N_data}',
    'obs': '[Observed Data] Get observed data from solving the PDE using FD and interpolation',
    'obs_noise': '[Observed Data] Noise level {noise}',
    'kernel': '[Kernel] {c.kernel}',
    'kernel_par': '[Kernel parameter]: {c.kernel_parameter}',
    'gram': '[Gram matrix] Finish assembly of the Gram matrix, nugget {c.nugget}, type {c.nugget_type}',
    'chol': '[Gram matrix] Finish Cholesky factorization of the Gram matrix',
    'gn_start': '[Gauss Newton] Start Gauss Newton iteration',
    'gn_method': '[Gauss Newton] {method} approaches',
    'gn_done': '[Gauss Newton] Gauss Newton iteration finished',
    'pts_err': '[Calculating collocation errors...]',
    'pts_max': '[Collocation point error] Max error {v}',
    'pts_l2': '[Collocation point error] L2 error {v}',
    'testing': '[Testing...] Number of test points: {n}',
    'test_max': '[Test error] Max error {v}',
    'test_l2': '[Test error] L2 error {v}',
    'res_n': '[Testing PDE residual...] Number of test points: {n}',
    'res_max': '[Test residual] Max residual {v}',
    'res_l2': '[Test residual] L2 residual {v}',
    'var_n': '[Testing posterior variance...] Number of test points: {n}',
    'var_mean': '[Test variance] Mean posterior std{tag} {v}',
    'var_max': '[Test variance] Max posterior std{tag} {v}',
    'smp_n': '[Testing posterior samples...] Number of test points: {n}',
    'smp': '[Test samples] {k} samples, RMS spread {rms}, max spread {mx}{tag}',
    'evidence': '[Log evidence] log Z {v}, J {J}, log|Theta| {lt}, log|H/2| {lh}',
    'sel_row': '[Kernel selection] kernel_parameter {p}{how}: log Z {v}, J {J}, info (Cholesky, Gauss-Newton, H/2) {info}',
    'sel_best': '[Kernel selection] chosen kernel_parameter {p}, log Z {v}{note}',
}


def _say(enabled, *keys, **fmt):
    if enabled:
        for k in keys:
            print(_LOG[k].format(**fmt))


def _periods_of(c, domain):
    """cfg.period = (L_1, L_2) as two floats, or None (absent, None, or both 0); L_k = 0: axis k is not periodic.  A period other than
    the width of the domain on its axis is refused: the solution would be asked to repeat inside the domain, or not to close at its
    faces."""
    period = getattr(c, 'period', None)
    if period is None:
        return None
    L = [float(v) for v in onp.atleast_1d(onp.asarray(period, dtype=onp.float64))]
    if len(L) != 2 or len(domain) != 2:
        raise ValueError(f'cfg.period {period!r}: one period per axis of a two-dimensional domain (0: the axis is not periodic)')
    if not any(L):
        return None
    for k in range(2):
        width = float(domain[k][1]) - float(domain[k][0])
        if L[k] != 0.0 and L[k] != width:
            raise ValueError(f'cfg.period: the period {L[k]} of axis {k + 1} differs from the width {width} of the domain on that axis')
    return L


def _as_vector(truth, n):
    """the user's truth as n float64 values (a scalar truth -- e.g. 0 -- is broadcast like under jnp)"""
    t = onp.asarray(truth, dtype=onp.float64)
    return onp.full(n, float(t)) if t.ndim == 0 else t.ravel()


class solver_GP(object):
    """Same public surface as the reference's solver_GP; the work happens in the equation objects (src/PDEs.py,
    src/InverseProblems.py), which drive libgpk."""

    def __init__(self, cfg=None, PDE_type="Nonlinear_elliptic"):
        self.config = cfg
        self.PDE_type = PDE_type

    def set_equation(self, bdy=None, rhs=None, domain=onp.array([[0, 1], [0, 1]]), print_option=True):
        if self.PDE_type not in _EQUATIONS:
            return
        make, header, params = _EQUATIONS[self.PDE_type]
        self.eqn = make(self.config, bdy=bdy, rhs=rhs, domain=domain)
        # cfg.period = (L_1, L_2): the periodic kernel's periods -- auto_sample() leaves the faces of a periodic axis out, and the
        # periods join the two length scales of cfg.kernel_parameter
        periods = _periods_of(self.config, domain)
        if periods is not None:
            if self.config.kernel != 'periodic_Gaussian':
                raise ValueError(f"cfg.period needs cfg.kernel = 'periodic_Gaussian', got {self.config.kernel!r}")
            self.eqn._periodic_axes = (periods[0] > 0.0, periods[1] > 0.0)
            kp = [float(v) for v in onp.atleast_1d(onp.asarray(self.config.kernel_parameter, dtype=onp.float64))]
            if len(kp) == 1:
                kp = kp * 2
            if len(kp) == 2:
                self.config.kernel_parameter = kp + periods
            elif len(kp) != 4 or kp[2:] != periods:
                raise ValueError(f'cfg.kernel_parameter {self.config.kernel_parameter!r}: (sigma_1, sigma_2), or with the periods of cfg.period appended')
        if print_option:
            print(_LOG['start'])
            for line in header(self.config):
                print(line)
            _say(True, 'domain3d' if len(domain) == 3 else 'domain', d=domain)
            if params is not None:
                print(params(self.config))
            _say(True, 'data')

    # ---- collocation (and data) points: given by the caller or drawn by the equation object's sampler -------------------
    def get_sample(self, X_domain, X_boundary, print_option=True):
        # (the reference passes `self` twice here and raises TypeError; this one works)
        self.eqn.get_sampled_points(X_domain, X_boundary)
        _say(print_option, 'pts_user', 'pts_n', e=self.eqn)

    def auto_sample(self, N_domain, N_boundary, sampled_type='random', print_option=True):
        if self.PDE_type in ('Nonlinear_elliptic3d', 'Semilinear3d') and getattr(self.config, 'time_dependent', False):
            self.eqn.sampled_pts(N_domain, N_boundary, sampled_type=sampled_type, time_dependent=True)
        else:
            self.eqn.sampled_pts(N_domain, N_boundary, sampled_type=sampled_type)
        _say(print_option, 'pts_auto', 'pts_n', e=self.eqn, kind=sampled_type)

    def get_sample_IP(self, X_domain, X_boundary, X_data, print_option=True):
        self.eqn.get_sampled_points(X_domain, X_boundary, X_data)
        _say(print_option, 'pts_user', 'pts_n_ip', e=self.eqn)

    def auto_sample_IP(self, N_domain, N_boundary, N_data, sampled_type='random', print_option=True):
        self.eqn.sampled_pts(N_domain, N_boundary, N_data, sampled_type=sampled_type)
        _say(print_option, 'pts_auto', 'pts_n_ip', e=self.eqn, kind=sampled_type)

    def get_observed_data(self, data_u, noise_level, print_option=True):
        self.eqn.get_observation(data_u, noise_level)
        _say(print_option, 'obs', 'obs_noise', noise=noise_level)

    # ---- Gram matrix -> Cholesky -> Gauss-Newton -------------------------------------------------------------------------
    def solve(self, method='elimination', pen_lambda=1e-10, print_option=True):
        c, eqn = self.config, self.eqn
        _say(print_option, 'kernel', 'kernel_par', c=c)
        eqn.Gram_matrix(kernel=c.kernel, kernel_parameter=c.kernel_parameter, nugget=c.nugget, nugget_type=c.nugget_type)
        _say(print_option, 'gram', c=c)
        eqn.Gram_Cholesky()
        _say(print_option, 'chol', 'gn_start', 'gn_method', method=method)
        gn = dict(max_iter=c.GNsteps, step_size=c.step_size, initial_sol=c.initial_sol, print_hist=c.print_hist)
        # cfg.line_search (bool or LineSearch; cfg.ls_trials / ls_shrink / ls_c1): the equation object takes it as an instance attribute
        from .linesearch import from_config
        ls = from_config(c)
        if ls is not None:
            eqn.line_search = ls
        if method == 'elimination':
            eqn.GN_method(**gn)
        elif method == 'relaxation':
            eqn.GN_relaxed_method(pen_lambda=pen_lambda, **gn)
        if ls is not None and print_option:
            print('line search: step_hist =', [float(t) for t in eqn.step_hist])
        _say(print_option, 'gn_done')

    # ---- model evidence of the kernel parameter (eqn.log_evidence; no counterpart in the reference) ------------------------------------
    def log_evidence(self, print_option=True):
        """Laplace log evidence of the solved problem under cfg.kernel / cfg.kernel_parameter (eqn.log_evidence): returns log Z, the
        terms are in eqn.log_evidence_terms.  Needs solve(method='elimination')."""
        v = self.eqn.log_evidence()
        t = self.eqn.log_evidence_terms
        _say(print_option, 'evidence', v=v, J=t['J'], lt=t['logdet_theta'], lh=t['logdet_H'])
        return v

    def _evidence_at(self, parameter, initial, how, print_option):
        """Gram matrix, Cholesky, GN_method (cfg's settings, the given initial iterate) and log evidence at one kernel parameter: one
        row of kernel_selection"""
        c, eqn = self.config, self.eqn
        eqn.Gram_matrix(kernel=c.kernel, kernel_parameter=parameter, nugget=c.nugget, nugget_type=c.nugget_type)
        eqn.Gram_Cholesky()
        chol = int(onp.max(onp.abs(onp.atleast_1d(eqn.chol_info))))   # (Darcy: one status per factor)
        row = dict(parameter=parameter, log_Z=float('nan'), J=float('nan'), info=(chol, None, None), initial=initial, refined=bool(how))
        if chol == 0:                                               # (a failed factor: nothing downstream of it is defined)
            eqn.GN_method(max_iter=c.GNsteps, step_size=c.step_size, initial_sol=c.initial_sol if initial is None else initial,
                          print_hist=False)
            row['initial'] = eqn.init_sol
            log_Z = eqn.log_evidence()
            t = eqn.log_evidence_terms
            row.update(log_Z=float(log_Z), J=t['J'], info=(chol, max([0] + [int(i) for i in eqn.step_info]), int(t['info'])))
        row['ok'] = row['info'] == (0, 0, 0) and not onp.isnan(row['log_Z'])
        _say(print_option, 'sel_row', p=parameter, how=how, v=row['log_Z'], J=row['J'], info=row['info'])
        return row

    def select_kernel_parameter(self, candidates, refine=0, method='elimination', print_option=True):
        """Choose cfg.kernel_parameter among `candidates` -- scalars, or per-axis lists for the anisotropic and per-axis Matern forms --
        by the Laplace log evidence (eqn.log_evidence).  Every candidate is solved with cfg's settings (Gram_matrix, Gram_Cholesky,
        GN_method) from ONE initial iterate, drawn for the first candidate as solve() draws it, so the table does not depend on how many
        candidates there are.  A candidate whose Cholesky factorisation (chol_info), Gauss-Newton steps (any step_info > 0) or
        factorisation of H/2 fails, or whose log Z is NaN, is listed and never chosen.  refine = k (scalar candidates only, ValueError
        otherwise): k golden-section steps in log(parameter) between the grid neighbours of the best candidate; skipped, and said so,
        when the best candidate is an end of the grid.  Sets kernel_selection (candidates, log_Z, J, info, refined, best), sets
        cfg.kernel_parameter to the winner, leaves the solver solved there (ready for test()) and returns the winner.  The evidence ranks
        models, not errors."""
        if method != 'elimination':
            raise NotImplementedError("select_kernel_parameter: the log evidence is defined for method='elimination' only")
        cands = [list(map(float, p)) if onp.ndim(p) else float(p) for p in candidates]
        if not cands:
            raise ValueError('select_kernel_parameter: no candidates')
        refine = int(refine)
        scalar = all(not isinstance(p, list) for p in cands)
        if refine > 0 and not scalar:
            raise ValueError('select_kernel_parameter: refine > 0 needs scalar candidates')
        rows, initial = [], None
        for p in cands:
            rows.append(self._evidence_at(p, initial, '', print_option))
            initial = rows[-1]['initial'] if initial is None else initial
        value = lambda r: r['log_Z'] if r['ok'] else -onp.inf
        best = max(range(len(rows)), key=lambda k: value(rows[k]))
        if not rows[best]['ok']:
            self.kernel_selection = self._selection_table(rows, None)
            raise RuntimeError('select_kernel_parameter: no candidate could be solved and factored (kernel_selection has the table)')
        note = ''
        if refine > 0:
            order = sorted(range(len(cands)), key=lambda k: cands[k])
            at = order.index(best)
            if at == 0 or at == len(order) - 1:
                note = ' (an end of the candidate grid: not refined; widen the candidates)'
            else:
                # golden section in t = log(parameter) on (a, x, b) with the best value at x: every step evaluates one point of the larger
                # half and keeps the triple around the best point seen, so the result never leaves the bracket and never gets worse
                inv_phi2 = (3.0 - 5.0 ** 0.5) / 2.0
                a, x, b = (float(onp.log(cands[order[k]])) for k in (at - 1, at, at + 1))
                for _ in range(refine):
                    t = x + inv_phi2 * (b - x) if b - x >= x - a else x - inv_phi2 * (x - a)
                    rows.append(self._evidence_at(float(onp.exp(t)), initial, ' (refined)', print_option))
                    if value(rows[-1]) > value(rows[best]):
                        a, b = (x, b) if t > x else (a, x)
                        x, best = t, len(rows) - 1
                    else:
                        a, b = (a, t) if t > x else (t, b)
        winner = rows[best]['parameter']
        if best != len(rows) - 1:                                    # leave the solver solved at the winner: the same solve again
            self._evidence_at(winner, initial, '', False)
        self.config.kernel_parameter = winner
        self.kernel_selection = self._selection_table(rows, best)
        _say(print_option, 'sel_best', p=winner, v=rows[best]['log_Z'], note=note)
        return winner

    @staticmethod
    def _selection_table(rows, best):
        return dict(candidates=[r['parameter'] for r in rows], log_Z=onp.array([r['log_Z'] for r in rows]),
                    J=onp.array([r['J'] for r in rows]), info=[r['info'] for r in rows], refined=[r['refined'] for r in rows], best=best)

    # ---- errors (definitions of src/solver.py:175,191: root of the sum of squares over N_domain / N_test), reduced on the device
    # (gpk_error_metrics: |truth - value| per point, its maximum and sqrt(sum of squares / n) in one pass) ------------------------------
    def collocation_pts_err(self, truth, print_option=True):
        _say(print_option, 'pts_err')
        self.pts_err_all, self.pts_max_err, self.pts_L2_err = get_context().error_metrics(_as_vector(truth, self.eqn.N_domain),
                                                                                             self.eqn.sol_sampled_pts)
        _say(print_option, 'pts_max', v=self.pts_max_err)
        _say(print_option, 'pts_l2', v=self.pts_L2_err)

    def test(self, X_test, print_option=True):
        _say(print_option, 'testing', n=X_test.shape[0])
        self.eqn.extend_sol(X_test)

    def get_test_error(self, truth, print_option=True):
        self.truth = truth
        self.test_err_all, self.test_max_err, self.test_L2_err = get_context().error_metrics(_as_vector(truth, self.eqn.N_test),
                                                                                               self.eqn.extended_sol)
        _say(print_option, 'test_max', v=self.test_max_err)
        _say(print_option, 'test_l2', v=self.test_L2_err)

    def test_residual(self, X_test, print_option=True):
        """How well the GP solution satisfies the PDE between the collocation points -- no truth solution needed: the residual of the
        equation at X_test from the derivatives of the solution (eqn.PDE_residual), reduced like get_test_error against zero."""
        _say(print_option, 'res_n', n=X_test.shape[0])
        r = self.eqn.PDE_residual(X_test)
        _, self.test_res_max, self.test_res_L2 = get_context().error_metrics(onp.zeros(r.size), r)
        _say(print_option, 'res_max', v=self.test_res_max)
        _say(print_option, 'res_l2', v=self.test_res_L2)

    def test_variance(self, X_test, print_option=True):
        """The error bar of the GP solution between the collocation points: its posterior standard deviation at X_test in the
        Gauss-Newton (Laplace) form (eqn.posterior_variance), reduced to mean and maximum.  Darcy flow: both fields u and a."""
        _say(print_option, 'var_n', n=X_test.shape[0])
        self.eqn.posterior_variance(X_test)
        self.test_std_mean, self.test_std_max = {}, {}
        for tag in ('', '_u', '_a'):
            std = getattr(self.eqn, 'extended_std' + tag, None)
            if std is None:
                continue
            self.test_std_mean[tag], self.test_std_max[tag] = float(onp.mean(std)), float(onp.max(std))
            label = ' of ' + tag[1:] if tag else ''
            _say(print_option, 'var_mean', tag=label, v=self.test_std_mean[tag])
            _say(print_option, 'var_max', tag=label, v=self.test_std_max[tag])

    def test_samples(self, X_test, n_samples=1, seed=None, print_option=True):
        """Draws of plausible solutions between the collocation points: n_samples samples of the joint posterior at X_test
        (eqn.posterior_sample, standard normals from numpy.random.RandomState(seed)), reduced to the RMS and the maximum of their
        spread |sample - mean| over the test points.  Darcy flow: both fields u and a.  extend_sol's attributes stay as they are."""
        _say(print_option, 'smp_n', n=X_test.shape[0])
        self.eqn.posterior_sample(X_test, n_samples=n_samples, seed=seed)
        means = self.eqn._posterior_means(X_test)
        self.test_spread_rms, self.test_spread_max = {}, {}
        for tag in ('', '_u', '_a'):
            smp = getattr(self.eqn, 'extended_samples' + tag, None)
            if smp is None or tag not in means:
                continue
            spread = onp.abs(smp - means[tag][None, :])
            self.test_spread_rms[tag], self.test_spread_max[tag] = float(onp.sqrt(onp.mean(spread ** 2))), float(onp.max(spread))
            _say(print_option, 'smp', k=smp.shape[0], tag=f' (field {tag[1:]})' if tag else '', rms=self.test_spread_rms[tag],
                 mx=self.test_spread_max[tag])

    # ---- figures (cosmetic; need matplotlib only): src/_figures.py ---------------------------------------------------------
    def _planar_only(self):
        if self.PDE_type in ('Nonlinear_elliptic3d', 'Semilinear3d'):
            raise NotImplementedError(f'the plot helpers draw planar point sets and contours; not available for {self.PDE_type}')

    def show_sample(self):
        self._planar_only()
        from . import _figures
        _figures.scatter_points(self.eqn, False, 'Collocation points')

    def show_sample_IP(self):
        from . import _figures
        _figures.scatter_points(self.eqn, True, 'Collocation and data points')

    def show_loss_hist(self):
        from . import _figures
        _figures.loss_history(self.eqn)

    def contour_of_test_err(self, XX, YY):
        self._planar_only()
        from . import _figures
        self.XX, self.YY = XX, YY
        _figures.error_contour(XX, YY, self.test_err_all)
