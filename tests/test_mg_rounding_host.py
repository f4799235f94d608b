"""CPU side of tests/test_gpu_mg_rounding.py: the gate of the exchanged block S2 = L^-1 [A | F] does its job, the case list contains the
shard edges it is there for, and every case is one a rounding-level gate can decide.

  * The float64 scipy rendition of the sharded solve (every rank solves its columns [c0, c1) only, the shards are assembled into a
    zeroed block) passes _mg_rounding.gate_s2.  One column scaled by 1 + 1e-11, a shard written one column to the right and a stray
    1e-300 left of the leading-zero boundary are each rejected.  The old assert of tests/test_gpu_mg.py -- the iterate within 1e-8 of
    the one-GPU step in the 2-norm -- accepts the scaled column and the stray entry.  It does NOT accept the shifted shard: with the
    owner's first column left at zero the Gauss-Newton matrix loses a row and a column, so the iterate is off by far more than 1e-8;
    the test asserts that verdict as it is (the old file guards that error, the new gate guards it too).
  * The four shard edges of the elliptic case list, from gpk.mg.column_bounds (a pure host function of the library): a rank with an
    empty shard that is not the last, a shard that starts at an odd column, a rank that owns only the F column or only the last two
    columns, a rank without a block row of Hb.
  * For every (system, N_d) of the case list the numpy figure of the S2 gate is finite and at most _dense_reference.CAP, the promised
    profile covers only zeros of [A | F], cond(H) eps <= 1e-9 (the step is then determined to a tenth of the old 1e-8 gate or better; _gn_reference.py
    states 1e1 .. 1e6 for these factors, the Darcy system at N_d = 65 has 2e6) and the float64 pipeline passes the step gates.
"""
import numpy as np
import pytest

import _dense_reference as D
import _gn_reference as R
import _mg_rounding as MR
import _staircase_model as M

CASES = [(s, Nd) for s in MR.SYSTEMS for Nd in MR.SIZES]


def _iterate(cs, ref, S2, z):
    """one full step from the block S2 in float64 (data rows and the Darcy a-part from the float64 pipeline: they are not sharded)"""
    p = R.Pipeline64(cs, z)
    col = M.column_of_unknown(cs.system, cs.Nd)
    Sb = np.concatenate([p.S[:, np.argsort(col)], p.w[:, None]], axis=1)        # the pipeline's block in the step's column order
    Sb[ref.xoff:ref.xoff + ref.xrows] = S2[ref.xoff:ref.xoff + ref.xrows, :ref.nc]
    Hb = Sb.T @ Sb
    nz = cs.nz
    with np.errstate(all='ignore'):
        try:
            d = np.linalg.solve(2.0 * Hb[:nz, :nz], 2.0 * Hb[:nz, nz])
        except np.linalg.LinAlgError:
            d = np.full(nz, np.inf)
    return z - d[col]


@pytest.mark.parametrize('system,Nd', CASES)
def test_s2_gate_on_the_sharded_rendition(system, Nd):
    cs = R.case(system, Nd)
    ref = MR.SolveRef(cs, cs.z0)
    bounds = [0, ref.nc // 3 | 1, 2 * ref.nc // 3, ref.nc]            # an odd start among them
    good = MR.sharded_rendition(ref, bounds)
    r, a, ok = MR.gate_s2(ref, good)
    assert ok and r <= a and r == ref.np_ratio, (r, a, ref.np_ratio)
    z_good = _iterate(cs, ref, good, cs.z0)
    p = R.Pipeline64(cs, cs.z0)
    assert np.linalg.norm(z_good - (cs.z0 - p.delta)) <= 1e-10 * np.linalg.norm(z_good)     # (_iterate is the pipeline's step)
    rng = np.random.RandomState(Nd)
    # one column scaled by 1 + 1e-11
    bad = good.copy()
    c = int(rng.randint(ref.nc))
    bad[ref.xoff:, c] *= 1.0 + 1e-11
    assert not MR.gate_s2(ref, bad)[2]
    assert MR.old_iterate_assert(_iterate(cs, ref, bad, cs.z0), z_good)
    # the middle shard written one column to the right (the later shard then lands on its own columns)
    bad = np.zeros_like(good)
    c0, c1 = bounds[1], bounds[2]
    bad[:, :c0] = good[:, :c0]
    bad[:, c0 + 1:c1 + 1] = good[:, c0:c1]
    bad[:, c1:] = good[:, c1:]
    assert not MR.gate_s2(ref, bad)[2]
    assert not MR.old_iterate_assert(_iterate(cs, ref, bad, cs.z0), z_good)      # (a gross error: see the module docstring)
    # a stray 1e-300 left of the leading-zero boundary
    bad = good.copy()
    rows, cols = np.nonzero(ref.zero_mask)
    k = int(rng.randint(rows.size))
    bad[ref.xoff + rows[k], cols[k]] = 1e-300
    r, a, ok = MR.gate_s2(ref, bad)
    assert not ok and r == float('inf')
    assert MR.old_iterate_assert(_iterate(cs, ref, bad, cs.z0), z_good)
    if system == 'darcy':                                              # the a-part's F column under its own factor
        S2 = good.copy()
        from scipy.linalg import solve_triangular
        S2[:ref.xoff, ref.nc - 1] = solve_triangular(cs.L2, ref.Ba.astype(np.float64), lower=True)
        r, a, ok = MR.gate_s2_apart(ref, S2)
        assert ok and r == ref.np_ratio_a
        S2[:ref.xoff, ref.nc - 1] *= 1.0 + 1e-11
        assert not MR.gate_s2_apart(ref, S2)[2]


def test_elliptic_case_list_contains_the_shard_edges():
    found = MR.shard_edges()
    print()
    for k, v in found.items():
        print(f'[mg edges] {k}: (N_d, world, align, bounds, rank) = {v}')
    assert all(v is not None for v in found.values()), found
    # the table of the issue, from the library's host function
    assert MR.elliptic_bounds(129, 3, 128) == [0, 128, 128, 130]
    assert MR.elliptic_bounds(129, 3, 1) == [0, 63, 101, 130]
    assert MR.elliptic_bounds(65, 4, 64) == [0, 64, 64, 64, 66]
    assert MR.elliptic_bounds(65, 4, 128) == [0, 66, 66, 66, 66]
    # every world runs every alignment, every exchange form and both factorisations of Hb for every system
    for world in MR.WORLDS:
        cases = MR.step_cases(world)
        for s in MR.SYSTEMS:
            assert any(c['system'] == s and c['align'] is None for c in cases)              # (all options at their defaults)
            # (the defaults are col_align 128, overlap_s -1 and, from four ranks on, the panel-sharded Hb: gpk_mg_create)
            mine = [(c['align'], c['shard_hb'], c['overlap_s']) if c['align'] is not None else (128, int(world >= 4), -1)
                    for c in cases if c['system'] == s]
            assert {m[0] for m in mine} == set(MR.ALIGNS)
            assert {m[2] for m in mine} == {0, 1, 2, -1} and {m[1] for m in mine} == {0, 1}
            if world == 2:
                assert {c['Nd'] for c in cases if c['system'] == s and c['align'] is not None} == set(MR.SIZES)
        assert len({MR.case_id(c) for c in cases}) == len(cases)


@pytest.mark.parametrize('system,Nd', CASES)
def test_cases_are_decidable_to_rounding(system, Nd):
    cs = R.case(system, Nd)
    ref = MR.SolveRef(cs, cs.z0)
    assert np.isfinite(ref.np_ratio) and 0 < ref.np_ratio <= D.CAP, ref.np_ratio
    if system == 'darcy':
        assert np.isfinite(ref.np_ratio_a) and ref.np_ratio_a <= D.CAP
    vec = R.vector_reference(system, Nd)
    p = vec.p64
    ev = np.linalg.eigvalsh(p.H)
    print(f'\n[mg host {system} {Nd}] S2 numpy figure {ref.np_ratio:.3g}, cond(H) {ev[-1] / ev[0]:.3g}')
    assert ev[0] > 0 and ev[-1] / ev[0] * R.EPS <= 1e-9
    for gate, val in ((R.gate_loss, p.loss), (R.gate_backward_vec, p.delta), (R.gate_forward, p.delta)):
        r, a = gate(vec, val)
        assert np.isfinite(r) and np.isfinite(a) and r <= a


def test_bad_pivot_cases_name_lapacks_index():
    for world in MR.WORLDS + (1,):
        for name, (A, info) in MR.bad_pivot_cases(world).items():
            idx = info - 1
            with pytest.raises(np.linalg.LinAlgError):
                np.linalg.cholesky(A[:info, :info])                     # numpy's failing leading minor ...
            if idx:
                np.linalg.cholesky(A[:idx, :idx])                       # ... and the one before it does not fail
            panel = idx // MR.PANEL
            if name == 'bad_ragged_last_panel':
                assert panel == (MR.BAD_ORDER - 1) // MR.PANEL and MR.BAD_ORDER % MR.PANEL != 0
            else:
                assert panel % world == world - 1
