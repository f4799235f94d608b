"""CPU tier: the numpy model of the leading-zero layouts (tests/_staircase_model.py) is self-consistent -- the profiles it promises
are non-increasing, never above the exact first rows, exact where the layouts claim so, and the segment encodings the GPU tests hand
to the library evaluate to the same profiles.  tests/test_gpu_staircase.py compares the library against this model."""
import numpy as np
import pytest

import _staircase_model as M

ND = (64, 65, 127, 128, 129, 333)


@pytest.mark.parametrize('Nd', ND)
@pytest.mark.parametrize('system,variant', [('elliptic', 'exact'), ('relaxed', 'exact'), ('burgers', 'exact'), ('eikonal', 'exact'),
                                            ('eikonal', 'conservative'), ('darcy', 'u'), ('darcy', 'a'), ('semilinear', 'exact'),
                                            ('monge_ampere', 'exact'), ('monge_ampere', 'conservative')])
def test_promised_profile_is_non_increasing_and_below_the_exact_rows(system, variant, Nd):
    Nb = 11
    fr = M.promised_profile(system, Nd, Nb, variant)
    exact = M.exact_first_rows(system, Nd, Nb, 'a' if variant == 'a' else 'u')
    assert fr.shape == (M.n_unknowns(system, Nd),)
    if variant == 'a':                             # the closed form on the sub-range [N_d, 4 N_d); no entries elsewhere
        sub = slice(Nd, 4 * Nd)
        assert np.all(np.diff(fr[sub]) <= 0)
        assert np.array_equal(fr[sub], exact[sub])
        assert np.all(exact[:Nd] == M.NONE) and np.all(exact[4 * Nd:] == M.NONE)
        return
    assert np.all(np.diff(fr) <= 0)
    assert np.all(fr <= exact)
    assert np.all(exact < M.NONE)                  # every unknown has an entry in the factor's rows


@pytest.mark.parametrize('Nd', ND)
def test_where_the_layouts_are_exact(Nd):
    Nb = 7
    for system in ('elliptic', 'relaxed', 'burgers', 'eikonal'):
        assert np.array_equal(M.promised_profile(system, Nd, Nb), M.exact_first_rows(system, Nd, Nb)), system
    # closed forms: slope 1 (elliptic systems), slope 1/3 (Burgers)
    assert np.array_equal(M.promised_profile('elliptic', Nd, Nb), M.closed_form(Nd, Nd))
    assert np.array_equal(M.promised_profile('relaxed', Nd, Nb), M.closed_form(2 * Nd, 2 * Nd))
    assert np.array_equal(M.promised_profile('burgers', Nd, Nb), M.closed_form(3 * Nd, 3 * Nd, 3))
    # the Eikonal conservative form overstates the v0 columns (c < N_d) by N_d rows and is exact on the others
    ex = M.exact_first_rows('eikonal', Nd, Nb)
    cons = M.promised_profile('eikonal', Nd, Nb, 'conservative')
    assert np.array_equal(ex[:Nd] - cons[:Nd], np.full(Nd, Nd)) and np.array_equal(ex[Nd:], cons[Nd:])
    # Darcy u-part: exact over the v0, w0 columns and the v2, v1 columns; the flat step over w2, w1 is the non-increasing envelope
    # (the exact rows there, 2 N_d + t, rise again after the w0 columns)
    ex = M.exact_first_rows('darcy', Nd, Nb, 'u')
    fu = M.promised_profile('darcy', Nd, Nb, 'u')
    assert np.array_equal(fu[:2 * Nd], ex[:2 * Nd]) and np.array_equal(fu[4 * Nd:], ex[4 * Nd:])
    assert np.all(fu[2 * Nd:4 * Nd] == 2 * Nd) and np.all(ex[2 * Nd:4 * Nd] >= 2 * Nd) and ex[3 * Nd - 1] == 2 * Nd


@pytest.mark.parametrize('Nd', ND)
def test_semilinear_keeps_the_closed_form(Nd):
    """The semilinear system shares Eikonal's column order, but v0_t enters its PDE row 2 N_d + t: its exact rows are the slope-1 closed
    form over all n_z columns, on every solve path, and Eikonal's two-segment profile would promise zeros where N_u / eps sits -- on
    every v0 column (c < N_d), by exactly N_d rows."""
    Nb, nz = 7, 3 * Nd
    ex = M.exact_first_rows('semilinear', Nd, Nb)
    want = M.closed_form(nz, nz)
    for variant in ('exact', 'conservative'):
        assert np.array_equal(M.promised_profile('semilinear', Nd, Nb, variant), want)
    assert np.array_equal(want, M.envelope(ex)) and np.array_equal(want, ex)
    assert np.array_equal(M.column_of_unknown('semilinear', Nd), M.column_of_unknown('eikonal', Nd))
    two = M.promised_profile('eikonal', Nd, Nb)
    assert np.all(two[:Nd] > ex[:Nd]) and np.array_equal(two[:Nd] - ex[:Nd], np.full(Nd, Nd))     # it would be wrong there ...
    assert np.array_equal(two[Nd:], ex[Nd:])                                                       # ... and only there
    # the entries it would drop are those of the PDE row: (2 N_d + t, v0_t), t = N_d - 1 - c
    c = np.arange(Nd)
    assert np.array_equal(ex[:Nd], 2 * Nd + (Nd - 1 - c))


@pytest.mark.parametrize('Nd', ND)
def test_monge_ampere_has_the_eikonal_profiles(Nd):
    """v0 does not enter the Monge-Ampere PDE row: the exact rows are Eikonal's, the exact profile is the two-segment encoding, and the
    conservative closed form overstates the v0 columns by N_d rows"""
    Nb, nz = 7, 3 * Nd
    ex = M.exact_first_rows('monge_ampere', Nd, Nb)
    assert np.array_equal(ex, M.exact_first_rows('eikonal', Nd, Nb))
    two = M.promised_profile('monge_ampere', Nd, Nb)
    assert np.array_equal(two, M.stair_eval(M.stair_encoding('eikonal', Nd), nz))
    assert np.array_equal(two, M.envelope(ex)) and np.array_equal(two, ex)
    cons = M.promised_profile('monge_ampere', Nd, Nb, 'conservative')
    assert np.array_equal(cons, M.closed_form(nz, nz))
    assert np.array_equal(ex[:Nd] - cons[:Nd], np.full(Nd, Nd)) and np.array_equal(ex[Nd:], cons[Nd:])


@pytest.mark.parametrize('Nd', ND)
@pytest.mark.parametrize('system', ['eikonal', 'darcy'])
def test_segment_encoding_matches_the_profile(system, Nd):
    seg = M.stair_encoding(system, Nd)
    nz = M.n_unknowns(system, Nd)
    prof = M.promised_profile(system, Nd, 5, 'u' if system == 'darcy' else 'exact')
    assert np.array_equal(M.stair_eval(seg, nz), prof)
    assert np.all(M.stair_eval(seg, nz + 1)[nz:] == 0)         # the F column is dense


def test_staircase_positions_are_a_permutation():
    for system in M.systems():
        for Nd in (1, 2, 64, 65):
            pos = M.staircase_position(system, Nd)
            assert np.array_equal(np.sort(pos), np.arange(M.n_unknowns(system, Nd))), (system, Nd)


def test_first_nonzero_rows():
    A = np.array([[0, 1, 0], [2, 0, 0], [3, 4, 0]], dtype=float)
    assert list(M.first_nonzero_rows(A)) == [1, 0, M.NONE]
