"""Host tests of the line search (no GPU): the CPU reference itself (tests/_linesearch_reference.py), the Gauss-Newton model identity in
long double, LineSearch validation, and the branch _gn_iterate takes with and without eq.line_search.

Model identity.  With delta = H^-1 g and pred = g . delta / 2, the loss of the system LINEARISED at z is, at z - t delta,
    |L^-1 (F - t A delta)|^2 = J - t g . delta + t^2 delta^T (H / 2) delta = J - 2 t pred + t^2 pred,
because H delta = g.  Both sides are evaluated in long double on the synthetic cases of _gn_reference; delta is the refined long-double
solution, whose residual enters as t^2 delta . (H delta - g) / 2, far below the bound of 64 eps J (eps = 2^-52).
"""
import numpy as np
import pytest

import _gn_reference as R
import _linesearch_reference as LS

LD, EPS = R.LD, R.EPS


@pytest.mark.parametrize('system', R.SYSTEMS)
def test_model_identity_long_double(system):
    ref = R.vector_reference(system, 65)
    J, pred = LS.model_terms(ref)
    assert pred > 0
    tol = 64 * EPS * float(J)
    for t in (1.0, 0.25, 2.0):
        lin = LS.linearised_loss(ref, t)
        err = float(abs(lin - LS.model(J, pred, t)))
        print(f'[model {system}] t = {t}: |linearised - model| = {err:.3g}, bound {tol:.3g}')
        assert err <= tol
    assert float(abs(LS.linearised_loss(ref, 1.0) - (J - pred))) <= tol          # J - pred: the minimum of the linearised loss


def test_steps_are_repeated_products():
    t = LS.steps(8.0, 0.5, 8)
    assert np.array_equal(t, 8.0 * 0.5 ** np.arange(8))
    t = LS.steps(1.0, 0.3, 5)
    assert t[3] == ((1.0 * 0.3) * 0.3) * 0.3 and t.size == 5


# (losses, t, loss_in, pred, c1) -> k
ACCEPT_CASES = {
    'first Armijo index': ([12.0, 9.9, 9.0, 8.0], [1, .5, .25, .125], 10.0, 1.0, 1e-4, 1),
    'full step accepted': ([1.0, 0.5], [1, .5], 10.0, 5.0, 1e-4, 0),
    'NaN and +inf skipped': ([np.nan, np.inf, 9.0, 8.0], [1, .5, .25, .125], 10.0, 1.0, 1e-4, 2),
    '-inf is not finite either': ([-np.inf, 9.0], [1, .5], 10.0, 1.0, 1e-4, 1),
    'fall-back to the smallest loss': ([9.99, 9.95, 9.97], [1, .5, .25], 10.0, 100.0, 0.5, 1),
    'fall-back takes the first of equal losses': ([9.95, 9.95], [1, .5], 10.0, 100.0, 0.5, 0),
    'all >= loss_in': ([10.0, 11.0, 10.5], [1, .5, .25], 10.0, 1.0, 1e-4, -1),
    'all non-finite': ([np.nan, np.inf], [1, .5], 10.0, 1.0, 1e-4, -1),
    'K = 1 accepted': ([3.0], [1], 10.0, 1.0, 1e-4, 0),
    'K = 1 refused': ([10.0], [1], 10.0, 1.0, 1e-4, -1),
    'equality satisfies Armijo': ([10.0 - 2 * 0.25 * 1.0 * 2.0], [1.0], 10.0, 2.0, 0.25, 0),
}


@pytest.mark.parametrize('name', list(ACCEPT_CASES))
def test_acceptance_rule(name):
    losses, t, loss_in, pred, c1, want = ACCEPT_CASES[name]
    assert LS.accept(np.array(losses, dtype=float), np.array(t, dtype=float), loss_in, pred, c1) == want


def test_reference_iteration_on_a_quadratic_takes_the_full_step():
    """a linear system: the model is exact, the full step satisfies Armijo and reaches the minimum in one step"""
    class Linear:
        nz = 3
        Amat = np.array([[2.0, 0.0, 1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 3.0], [0.5, 0.5, 0.5]])
        b = np.array([1.0, -2.0, 0.5, 0.25])
        def F(self, z): return [self.Amat @ z - self.b]
        def A(self, z): return [self.Amat]
        def extra(self, z): return 0.0, None, None
    L = np.tril(np.arange(1.0, 17.0).reshape(4, 4)) + 4 * np.eye(4)
    out = LS.ls_iterate(Linear(), [L], np.ones(3), 2)
    assert out['k'][0] == 0 and out['step_hist'][0] == 1.0
    assert abs(out['loss_hist'][1] - (out['loss_hist'][0] - out['pred'][0])) <= 1e-12 * out['loss_hist'][0]
    assert len(out['loss_hist']) == 3 and len(out['trial'][0]) == 8


def test_linesearch_validation():
    from src.linesearch import LineSearch, from_config
    ls = LineSearch()
    assert (ls.trials, ls.t0, ls.shrink, ls.c1) == (8, 1.0, 0.5, 1e-4)
    assert ls.steps() == list(LS.steps(1.0, 0.5, 8))
    assert ls.first_step(0.5) == 0.5 and LineSearch(t0=2.0).first_step(0.5) == 2.0
    LineSearch(trials=1); LineSearch(trials=16)
    for bad in (dict(trials=0), dict(trials=17), dict(trials=2.5), dict(shrink=0.0), dict(shrink=1.0), dict(c1=0.0), dict(c1=1.0),
                dict(t0=0.0), dict(t0=-1.0), dict(t0=float('inf')), dict(t0=float('nan'))):
        with pytest.raises(ValueError):
            LineSearch(**bad)
    import types
    assert from_config(types.SimpleNamespace()) is None
    assert from_config(types.SimpleNamespace(line_search=False)) is None
    got = from_config(types.SimpleNamespace(line_search=True, ls_trials=4, ls_shrink=0.25, ls_c1=0.1))
    assert (got.trials, got.shrink, got.c1) == (4, 0.25, 0.1)
    assert from_config(types.SimpleNamespace(line_search=ls)) is ls
    for bad in (dict(ls_trials=0), dict(ls_shrink=0.0), dict(ls_c1=0.0)):                 # an explicit 0 is refused, not replaced by the default
        with pytest.raises(ValueError):
            from_config(types.SimpleNamespace(line_search=True, **bad))
    assert from_config(types.SimpleNamespace(line_search=True, ls_trials=None)).trials == 8


class _StubArray:
    def download(self):
        return np.zeros(3)


class _StubContext:
    def __init__(self):
        self.calls = []

    def array(self, a):
        return _StubArray()

    def gn_step(self, prob, z, step_size=1.0):
        self.calls.append(('gn_step', step_size))
        return 1.0, 0

    def gn_step_ls(self, prob, z, trials, t0, shrink, c1):
        self.calls.append(('gn_step_ls', trials, t0, shrink, c1))
        k = -1 if len(self.calls) == 2 else 1
        return 2.0, 0, k, (t0 * shrink if k >= 0 else 0.0), np.full(trials, 1.5)

    def gn_loss(self, prob, z):
        self.calls.append(('gn_loss',))
        return 0.5


def test_gn_iterate_branches(monkeypatch, capsys):
    """eq.line_search absent or None: the loop the equation always ran (gn_step only); set: gn_step_ls only, with the history attributes"""
    import src.PDEs as P
    from src.linesearch import LineSearch
    stub = _StubContext()
    monkeypatch.setattr(P, 'get_context', lambda: stub)
    monkeypatch.delenv('GPK_SEPARATE_LOSS', raising=False)
    eq = P._GPEquation.__new__(P._GPEquation)
    eq._drop_posterior = lambda: None
    eq._gn_iterate('prob', np.zeros(3), 2, 0.5, False)
    assert stub.calls == [('gn_step', 0.5), ('gn_step', 0.5), ('gn_loss',)] and eq.loss_hist == [1.0, 1.0, 0.5]
    assert not hasattr(eq, 'step_hist')
    eq.line_search = None
    stub.calls.clear()
    eq._gn_iterate('prob', np.zeros(3), 1, 1, False)
    assert stub.calls == [('gn_step', 1), ('gn_loss',)]
    eq.line_search = LineSearch(trials=4, shrink=0.25, c1=0.1)
    stub.calls.clear()
    eq._gn_iterate('prob', np.zeros(3), 3, 0.5, False)
    assert stub.calls == [('gn_step_ls', 4, 0.5, 0.25, 0.1)] * 3 + [('gn_loss',)]
    assert eq.loss_hist == [2.0, 2.0, 2.0, 0.5]
    assert eq.step_hist == [0.125, 0.0, 0.125] and eq.ls_failed == [2] and len(eq.trial_loss_hist) == 3
    assert capsys.readouterr().out.count('line search failed at step 2') == 1
    del eq.line_search
    stub.calls.clear()
    eq._gn_iterate('prob', np.zeros(3), 1, 1, False)
    assert stub.calls == [('gn_step', 1), ('gn_loss',)]


def test_sharded_step_refuses_a_line_search():
    from gpk.sharded import ShardedFactorSolve
    from src.linesearch import LineSearch
    s = ShardedFactorSolve.__new__(ShardedFactorSolve)
    with pytest.raises(NotImplementedError, match='line search'):
        s.gn_step(None, 1, 1, None, None, None, None, None, 1.0, line_search=LineSearch())
