"""Backtracking line search for the Gauss-Newton iteration ("Line search"; no counterpart in the reference, whose
loop takes a fixed step size).

    eq.line_search = LineSearch(trials=8, t0=1.0, shrink=0.5, c1=1e-4)      # an INSTANCE attribute, set at run time
    eq.GN_method(...)                                                        # same call, same signature

Every step then tries t_k = t0 shrink^k, k < trials, along delta = H^{-1} g and takes the first one whose loss is finite and satisfies
the Armijo test  J(z - t_k delta) <= J(z) - 2 c1 t_k pred,  pred = g . delta / 2;  if none does, the trial with the smallest finite
loss provided it is below J(z); otherwise the step fails (k = -1) and z stays.  All of it runs on the device (gpk_gn_step_ls): the K
trial losses are one K-column forward solve against the fixed factor of Theta, one host synchronisation per step.
eq.line_search absent or None: the loop the equation always ran.

A line-searched run leaves these run-time attributes on the equation object next to loss_hist (J(z_0) .. J(z_max_iter), as always):
step_hist (accepted t per step, 0.0 for a failed one), ls_accepted (the accepted index k per step, -1 for a failed one),
trial_loss_hist (the K trial losses per step) and ls_failed (the 1-based steps with k = -1, each also printed once)."""


class LineSearch:
    MAX_TRIALS = 16                       # GPK_LS_MAX_TRIALS of include/gpk.h

    def __init__(self, trials=8, t0=1.0, shrink=0.5, c1=1e-4):
        if isinstance(trials, bool) or int(trials) != trials or not 1 <= int(trials) <= self.MAX_TRIALS:
            raise ValueError(f'LineSearch: trials must be an integer in 1 .. {self.MAX_TRIALS}, got {trials!r}')
        if not 0.0 < float(shrink) < 1.0:
            raise ValueError(f'LineSearch: shrink must lie in (0, 1), got {shrink!r}')
        if not 0.0 < float(c1) < 1.0:
            raise ValueError(f'LineSearch: c1 must lie in (0, 1), got {c1!r}')
        if not (float(t0) > 0.0 and float(t0) != float('inf')):
            raise ValueError(f'LineSearch: t0 must be positive and finite, got {t0!r}')
        self.trials, self.t0, self.shrink, self.c1 = int(trials), float(t0), float(shrink), float(c1)

    def first_step(self, step_size):
        """t0 of an iteration: GN_method's step_size argument takes its place while t0 is left at the default 1.0"""
        return float(step_size) if self.t0 == 1.0 else self.t0

    def steps(self, t0=None):
        """the trial step sizes, by repeated multiplication (one rounding per trial, as the library forms them)"""
        t = [self.t0 if t0 is None else float(t0)]
        for _ in range(1, self.trials):
            t.append(t[-1] * self.shrink)
        return t

    def __repr__(self):
        return f'LineSearch(trials={self.trials}, t0={self.t0}, shrink={self.shrink}, c1={self.c1})'


def from_config(cfg):
    """cfg.line_search (bool or LineSearch) with cfg.ls_trials / ls_shrink / ls_c1 -> LineSearch or None"""
    ls = getattr(cfg, 'line_search', None)
    if isinstance(ls, LineSearch) or ls is None:
        return ls
    if not ls:
        return None
    given = {name: getattr(cfg, key, None) for name, key in (('trials', 'ls_trials'), ('shrink', 'ls_shrink'), ('c1', 'ls_c1'))}
    return LineSearch(**{name: v for name, v in given.items() if v is not None})    # (an explicit 0 reaches LineSearch and is refused)
