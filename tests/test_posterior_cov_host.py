"""The posterior-covariance reference (tests/_posterior_cov_reference.py) against facts that do not depend on it -- no GPU.

  linear equation   with alpha = 0 the elliptic system is -Delta u = f, u = g: the data are rows of Theta themselves (the Laplacian block
                    and the boundary block), A does not depend on z, and the Laplace formula must give the exact conditional
                    covariance of the linear GP, K_tt - K_td^T Theta_dd^-1 K_td, computed here from those rows alone.  Both sides in
                    long double; the tolerance is the 1e-12 relative of tests/test_posterior_host.py for the variance, carried to the
                    entries by |Sigma_st| <= sqrt(Sigma_ss Sigma_tt): an entry may deviate by 1e-12 sqrt(Sigma_ss Sigma_tt)
  diagonal          diag Sigma_cond, diag Sigma_gn are variance_ld's var_cond, var_gn (another summation order: n eps_longdouble of scale)
  symmetric, PSD    exactly symmetric; smallest eigenvalue >= -N_t eps max|Sigma| (the float64 eigensolver's own rounding)
  sampling          L = cholesky_ld(Sigma + jitter I) reproduces Sigma + jitter I, so mean + L xi has that covariance
  symbols           the three entry points are declared (fails on a tree without the feature)
"""
import numpy as np
import pytest

from oracle import gp_oracle as O
import _gn_reference as R
import _posterior_reference as PR
import _posterior_cov_reference as CR
from test_posterior_host import _elliptic_case, small_real_case

LD = PR.LD
EPS_LD = float(np.finfo(LD).eps)
EQN_KERNEL_LAYOUTS = {'Darcy_flow2d': ('Darcy_u', 'Darcy_a')}


def test_linear_equation_gives_the_exact_conditional_covariance():
    Nd, Nb, sigma = 24, 12, 0.3
    cs, Xd, Xb, _, T, _, rng = _elliptic_case(Nd, Nb, sigma, 1e-3, 'identity', 0.0, 3.0)
    Xt = rng.uniform(0, 1, (17, 2))
    K = O.construct_theta_test(Xt, Xd, Xb, 'Nonlinear_elliptic', 'Gaussian', sigma).T        # N x Nt
    Ktt = CR.prior_ld('Gaussian', sigma, Xt)
    ld, _ = cs.factors()
    z = rng.uniform(0.3, 1.2, Nd)                                    # (A = [0; I; 0] whatever z is)
    got = CR.covariance_ld(cs, z, K, Ktt, factors_ld=ld).cov
    data = np.concatenate([np.arange(Nd), 2 * Nd + np.arange(Nb)])  # the rows Delta delta_{x_i} and delta_{x_b}
    G = T.astype(LD)[np.ix_(data, data)]
    c = R.solve_lower(PR.cholesky_ld(G), K.astype(LD)[data])
    want = Ktt - R.gram_lower(c)
    d = np.sqrt(np.diag(want))
    rel = float(np.max(np.abs(got - want) / np.outer(d, d)))
    print(f'\n[posterior-cov-host] linear equation: max deviation {rel:.2e} of sqrt(S_ss S_tt), variances {float(d.min() ** 2):.2e} .. '
          f'{float(d.max() ** 2):.2e}')
    assert rel <= 1e-12


@pytest.mark.parametrize('system', ['elliptic', 'burgers', 'eikonal', 'darcy'])
def test_diagonal_symmetry_definiteness_and_sampling(system):
    cs, Xd, Xb, eqn, kernel, kp, z = small_real_case(system)
    nt = 23
    Xt = np.random.RandomState(5).uniform(0, 1, (nt, 2))
    Kt = O.construct_theta_test(Xt, Xd, Xb, eqn, kernel, kp)
    Ktt = CR.prior_ld(kernel, kp, Xt)
    assert np.array_equal(Ktt, Ktt.T) and np.all(np.diag(Ktt) == 1)
    ld, _ = cs.factors()
    prepared = PR.prepare_ld(cs, z, ld)
    for field, K in enumerate(Kt if system == 'darcy' else [Kt]):
        res = CR.covariance_ld(cs, z, K.T, Ktt, field, ld, prepared)
        var = PR.variance_ld(cs, z, K.T, field, ld, prepared)
        n = max(K.shape[1], cs.nz)
        tol = n * EPS_LD
        assert np.all(np.abs(np.diag(res.cond) - var.var_cond) <= tol * (1 + var.sv))
        assert np.all(np.abs(np.diag(res.gn) - var.var_gn) <= tol * var.sw)
        S = res.cov
        assert np.array_equal(S, S.T) and np.array_equal(res.cond, res.cond.T)
        assert np.all(res.scale >= np.abs(S)) and np.all(res.scale >= res.scale_cond)
        lam = np.linalg.eigvalsh(S.astype(np.float64))
        floor = -nt * R.EPS * float(np.max(np.abs(S)))
        print(f'\n[posterior-cov-host] {system} field {field}: eigenvalues {lam[0]:.2e} .. {lam[-1]:.2e}, floor {floor:.2e}')
        assert lam[0] >= floor
        jitter = LD(1e-6)
        Sj = S + jitter * np.eye(nt, dtype=LD)
        L = PR.cholesky_ld(Sj)
        back = L @ L.T
        assert float(np.max(np.abs(back - Sj))) <= (nt + 1) * EPS_LD * float(np.max(np.diag(Sj)))
        xi = np.random.RandomState(field).standard_normal((nt, 4)).astype(LD)
        # covariance of mean + L xi over the draws is L E[xi xi^T] L^T: with xi xi^T replaced by I this is `back`; the identity itself
        smp = L @ xi
        assert float(np.max(np.abs(R.solve_lower(L, smp) - xi))) <= 1e-6   # (cond(L) <= 1e3 at jitter 1e-6: eps_longdouble x 1e3 x slack)


def test_symbols_are_declared():
    import gpk
    names = set(gpk.declared_symbols())
    for s in ('gpk_assemble_prior', 'gpk_posterior_covariance', 'gpk_posterior_sample'):
        assert s in names, s
        assert s in set(gpk.declared_symbols(dev=True)), s
