"""The posterior-variance reference (tests/_posterior_reference.py) against facts that do not depend on it -- no GPU.

  linear equation     with m = 1 the elliptic system is linear, A does not depend on z, and the Laplace formula must give the exact
                      conditional variance of the linear GP, computed here by another route: the Gram matrix of the N_d + N_b
                      functionals (Delta - alpha) delta_{x_i}, delta_{x_b} built from the oracle's Theta blocks by linear combination
  collocation points  at x = a domain collocation point k_x is a column of Theta without its nugget: var_cond is nugget-sized and
                      var_gn is the diagonal entry of (H/2)^-1 = Cov(z)
  bounds              0 <= var <= 1 and var >= var_cond on a small real case of every system
  symbols             the five entry points are declared (fails on a tree without the feature)
"""
import numpy as np
import pytest

from oracle import gp_oracle as O
import _gn_reference as R
import _posterior_reference as PR

LD = PR.LD
DOMAIN = np.array([[0.0, 1.0], [0.0, 1.0]])


def _points(Nd, Nb, seed, time_dependent=False):
    rng = np.random.RandomState(seed)
    return O.sampled_pts_rdm(Nd, Nb, DOMAIN, time_dependent=time_dependent, rng=rng), rng


def _elliptic_case(Nd, Nb, sigma, nugget, nugget_type, alpha, m, seed=3):
    (Xd, Xb), rng = _points(Nd, Nb, seed)
    T0 = O.gram_matrix_assembly(Xd, Xb, 'Nonlinear_elliptic', 'Gaussian', sigma)
    T, ratios = O.add_nugget(T0, 'Nonlinear_elliptic', Nd, Nb, nugget, nugget_type)
    cs = PR.RealCase('elliptic', Nd, Nb, rng.uniform(0.5, 1.5, Nd), rng.uniform(0.5, 1.5, Nb), alpha, m, T)
    return cs, Xd, Xb, T0, T, ratios, rng


def test_linear_equation_gives_the_exact_conditional_variance():
    Nd, Nb, sigma, alpha = 24, 12, 0.3, 1.7
    cs, Xd, Xb, _, T, _, rng = _elliptic_case(Nd, Nb, sigma, 1e-3, 'identity', alpha, 1.0)
    Xt = rng.uniform(0, 1, (17, 2))
    K = O.construct_theta_test(Xt, Xd, Xb, 'Nonlinear_elliptic', 'Gaussian', sigma).T        # N x Nt
    ld, _ = cs.factors()
    z = rng.uniform(0.3, 1.2, Nd)                                    # (A = [alpha I; I; 0] whatever z is)
    got = PR.variance_ld(cs, z, K, factors_ld=ld).var
    # the other route: the data are the N_d + N_b linear functionals B [Delta u; u; u_b] with rows (Delta - alpha) delta_{x_i} and
    # delta_{x_b}; their Gram matrix is B Theta B^T, their covariances with u(x) are B k_x
    N = 2 * Nd + Nb
    B = np.zeros((Nd + Nb, N), dtype=LD)
    B[np.arange(Nd), np.arange(Nd)] = 1
    B[np.arange(Nd), Nd + np.arange(Nd)] = -LD(alpha)
    B[Nd + np.arange(Nb), 2 * Nd + np.arange(Nb)] = 1
    G = B @ T.astype(LD) @ B.T
    c = R.solve_lower(PR.cholesky_ld(G), B @ K.astype(LD))
    want = LD(1) - np.sum(c * c, axis=0)
    rel = float(np.max(np.abs(got - want) / np.abs(want)))
    print(f'\n[posterior-host] linear equation: max relative deviation {rel:.2e}, variances {float(want.min()):.2e} .. {float(want.max()):.2e}')
    assert rel <= 1e-12


def test_at_the_domain_collocation_points():
    Nd, Nb, sigma, nugget = 40, 16, 0.2, 1e-6
    cs, Xd, Xb, _, T, ratios, rng = _elliptic_case(Nd, Nb, sigma, nugget, 'adaptive', 1.0, 3.0)
    K = O.construct_theta_test(Xd, Xd, Xb, 'Nonlinear_elliptic', 'Gaussian', sigma).T        # test points = domain points
    ld, _ = cs.factors()
    z = rng.uniform(0.3, 1.2, Nd)
    res = PR.variance_ld(cs, z, K, factors_ld=ld)
    L = ld[id(T)]
    # Theta^-1 k by two long-double substitutions
    X = R.solve_lower_t(L, R.solve_lower(L, K.astype(LD)))
    bound = LD(nugget) * LD(max(ratios + [1.0])) * np.sum(X * X, axis=0)
    worst_c = float(np.max(res.var_cond / bound))
    # Cov(z) = (H/2)^-1: its diagonal from the factor
    n = cs.nz
    Linv = R.solve_lower(res.LH, np.eye(n, dtype=LD))
    covd = np.sum(Linv * Linv, axis=0)
    worst_g = float(np.max(np.abs(res.var_gn - covd) / bound))
    print(f'\n[posterior-host] collocation points: var_cond / bound <= {worst_c:.3g}, |var_gn - diag Cov(z)| / bound <= {worst_g:.3g}; '
          f'bound {float(bound.min()):.2e} .. {float(bound.max()):.2e}, var_gn {float(res.var_gn.min()):.2e} .. {float(res.var_gn.max()):.2e}')
    assert np.all(res.var_cond <= bound)
    assert np.all(np.abs(res.var_gn - covd) <= bound)


def small_real_case(system, seed=11):
    """(case, X_domain, X_boundary, kernel, kernel_parameter, z) of a small problem on the oracle's Gram matrices"""
    rng = np.random.RandomState(seed)
    if system == 'elliptic':
        Nd, Nb, kernel, kp, nugget, eqn = 30, 12, 'Gaussian', 0.25, 1e-6, 'Nonlinear_elliptic'
    elif system == 'burgers':
        Nd, Nb, kernel, kp, nugget, eqn = 24, 12, 'anisotropic_Gaussian', [1 / 3, 1 / 6], 1e-5, 'Burgers'
    elif system == 'eikonal':
        Nd, Nb, kernel, kp, nugget, eqn = 24, 12, 'Gaussian', 0.25, 1e-6, 'Eikonal'
    else:
        Nd, Nb, kernel, kp, nugget, eqn = 20, 12, 'Gaussian', 0.25, 1e-5, 'Darcy_flow2d'
    Xd, Xb = O.sampled_pts_rdm(Nd, Nb, DOMAIN, time_dependent=system == 'burgers', rng=rng)
    f, g = rng.uniform(0.5, 1.5, Nd), rng.uniform(0.5, 1.5, Nb)
    p0, p1 = R.PARAMS[system][:2]
    if system == 'darcy':
        Tu, Ta = O.gram_matrix_assembly(Xd, Xb, eqn, kernel, kp)
        Tu, _ = O.add_nugget(Tu, 'Darcy_u', Nd, Nb, nugget)
        Ta, _ = O.add_nugget(Ta, 'Darcy_a', Nd, Nb, nugget)
        cs = PR.RealCase(system, Nd, Nb, f, g, p0, p1, Tu, Ta, data=rng.uniform(0.5, 1.5, 8))
    else:
        T, _ = O.add_nugget(O.gram_matrix_assembly(Xd, Xb, eqn, kernel, kp), eqn, Nd, Nb, nugget)
        cs = PR.RealCase(system, Nd, Nb, f, g, p0, p1, T)
    z = rng.uniform(0.3, 1.2, cs.nz) * rng.choice([-1.0, 1.0], cs.nz)
    return cs, Xd, Xb, eqn, kernel, kp, z


@pytest.mark.parametrize('system', ['elliptic', 'burgers', 'eikonal', 'darcy'])
def test_bounds(system):
    cs, Xd, Xb, eqn, kernel, kp, z = small_real_case(system)
    Xt = np.random.RandomState(5).uniform(0, 1, (23, 2))
    Kt = O.construct_theta_test(Xt, Xd, Xb, eqn, kernel, kp)
    ld, _ = cs.factors()
    tol = 1e-9                                                       # cond(Theta) eps_longdouble: 1e10 x 1e-19
    for field, K in enumerate(Kt if system == 'darcy' else [Kt]):     # (construct_theta_test returns (u, a) for Darcy: field 0, 1)
        res = PR.variance_ld(cs, z, K.T, field=field, factors_ld=ld)
        print(f'\n[posterior-host] {system} field {field}: var_cond {float(res.var_cond.min()):.2e} .. {float(res.var_cond.max()):.2e}, '
              f'var {float(res.var.min()):.2e} .. {float(res.var.max()):.2e}')
        assert np.all(res.var >= -tol) and np.all(res.var <= 1 + tol)
        assert np.all(res.var >= res.var_cond)
        assert np.all(res.var_cond >= -tol)


def test_symbols_are_declared():
    import gpk
    names = set(gpk.declared_symbols())
    for s in ('gpk_assemble_cross', 'gpk_col_sumsq', 'gpk_posterior_worksize', 'gpk_posterior_prepare', 'gpk_posterior_variance'):
        assert s in names, s
        assert s in set(gpk.declared_symbols(dev=True)), s
