"""CPU reference of the backtracking line search ("Line search"): the acceptance rule, the trial step sizes, the
Gauss-Newton model along delta in long double on the synthetic cases of _gn_reference, and the line-searched iteration in float64 over
the numpy oracle's systems (oracle/gp_oracle.py: loss, gn_quantities)."""
import numpy as np

import _gn_reference as R

LD = R.LD


def steps(t0, beta, K):
    """t_k = t0 beta^k by repeated multiplication (one rounding per trial, as gpk_gn_step_ls forms them)"""
    t = [float(t0)]
    for _ in range(1, K):
        t.append(t[-1] * float(beta))
    return np.array(t)


def accept(losses, t, loss_in, pred, c1):
    """Trials in the order given: the first k whose loss is finite and <= loss_in - 2 c1 t_k pred; if there is none, the k of the
    smallest finite loss (the first of equals) provided that loss is < loss_in; otherwise -1."""
    best = -1
    for k, (l, tk) in enumerate(zip(losses, t)):
        if not np.isfinite(l):
            continue
        if l <= loss_in - 2.0 * c1 * tk * pred:
            return k
        if best < 0 or l < losses[best]:
            best = k
    if best >= 0 and losses[best] < loss_in:
        return best
    return -1


def thresholds(t, loss_in, pred, c1):
    return np.array([loss_in - 2.0 * c1 * tk * pred for tk in t])


# ------------------------------------------------------------------------------------------------ the model along delta (long double)
def model_terms(ref):
    """(J, pred) of a VectorReference with delta: pred = g . delta / 2 = |y|^2 in long double"""
    return ref.loss, (ref.g @ ref.delta) / LD(2)


def linearised_loss(ref, t):
    """|L^-1 (F - t A delta)|^2 in long double: the loss of the system linearised at ref.z, at z - t delta"""
    w = R._group_solve(ref.case, ref.lin.F - LD(t) * ref.lin.mul(ref.delta))
    return w @ w


def model(J, pred, t):
    t = LD(t)
    return J - LD(2) * t * pred + t * t * pred


# ------------------------------------------------------------------------------------------------ the iteration (float64, oracle systems)
def ls_iterate(sysm, Ls, z0, max_iter, K=8, t0=1.0, beta=0.5, c1=1e-4):
    """The line-searched Gauss-Newton iteration: dict with z, loss_hist (J(z_0) .. J(z_max_iter)), k (accepted index per step),
    step_hist (accepted t, 0.0 where k = -1), trial (the K losses per step), pred"""
    from scipy.linalg import cho_factor, cho_solve
    from oracle import gp_oracle as O
    z = np.array(z0, dtype=np.float64)
    t = steps(t0, beta, K)
    out = dict(loss_hist=[O.loss(sysm, Ls, z)], k=[], step_hist=[], trial=[], pred=[])
    for _ in range(max_iter):
        H, g = O.gn_quantities(sysm, Ls, z)
        d = cho_solve(cho_factor(H, lower=True, check_finite=False), g, check_finite=False)
        pred = 0.5 * float(g @ d)
        with np.errstate(all='ignore'):
            trial = np.array([O.loss(sysm, Ls, z - tk * d) for tk in t])
        k = accept(trial, t, out['loss_hist'][-1], pred, c1)
        if k >= 0:
            z = z - t[k] * d
        out['k'].append(k); out['step_hist'].append(float(t[k]) if k >= 0 else 0.0); out['trial'].append(trial); out['pred'].append(pred)
        out['loss_hist'].append(float(trial[k]) if k >= 0 else out['loss_hist'][-1])
    out['z'] = z
    return out


class ReactionSystem:
    """F and A of the elliptic system -Delta u + tau(u) = f with a reaction term given as two callables (tau, dtau), in the form the
    numpy oracle's loss / gn_quantities take (oracle/gp_oracle.py: EllipticSystem is the model): rows [tau(u) - f; u; g]"""

    def __init__(self, tau, dtau, rhs_f, bdy_g):
        self.tau, self.dtau = tau, dtau
        self.f, self.g = np.asarray(rhs_f, dtype=np.float64), np.asarray(bdy_g, dtype=np.float64)
        self.Nd, self.Nb = self.f.size, self.g.size
        self.nz = self.Nd

    def F(self, z):
        return [np.concatenate([self.tau(z) - self.f, z, self.g])]

    def A(self, z):
        Nd = self.Nd
        A = np.zeros((2 * Nd + self.Nb, Nd))
        i = np.arange(Nd)
        A[i, i] = self.dtau(z)
        A[Nd + i, i] = 1.0
        return [A]

    def extra(self, z):
        return 0.0, None, None


def plain_iterate(sysm, Ls, z0, max_iter, step_size=1.0):
    """(z, loss history) of the plain iteration: the oracle's gn_method, float64"""
    from oracle import gp_oracle as O
    with np.errstate(all='ignore'):
        return O.gn_method(sysm, Ls, z0, max_iter, step_size)
