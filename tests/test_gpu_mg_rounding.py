"""The sharded Cholesky and the sharded Gauss-Newton step (include/gpk_mg.h) to rounding, against long double.

tests/test_gpu_mg.py gates the multi-GPU path norm-wise on ill-conditioned Gram factors (1e-9 of the factor, 1e-6 .. 1e-8 of the
iterate) at one size and one alignment per system.  This file puts gpk_mg_gn_step in front of the long-double reference of
tests/_gn_reference.py (synthetic well-conditioned factors, poisoned upper triangles and padding) at N_d = 65 and 129, where ranks own
empty shards, shards that start at odd columns, shards that hold only the last two columns and no block row of Hb at all, and
gpk_mg_potrf in front of the componentwise gate of tests/_dense_reference.py.  tests/test_mg_rounding_host.py shows on the CPU that the
gates reject an error of 1e-11, asserts those shard edges from gpk.mg.column_bounds and that every case is decidable to rounding.

Process shape (tests/_mg_rounding.py): ONE launch per world size 2, 3, 4, several ranks on the one GPU with the host-staged
collectives over gloo (comm='staged', as tests/test_gpu_mg.py).  The ranks assert nothing; they write raw outputs and the parent applies
every gate.  The parent polls, terminates every rank as soon as one fails or the limit passes, and never retries.

  a. the step: elliptic, Burgers, Eikonal, Darcy (cache_a, Dinv2) x N_d {65, 129} x col_align {1, 64, 128} x (shard_hb, overlap_s)
     {(0, 0), (0, 1), (1, 2), (1, -1)}, panel width 64, dinv 256, plus every (system, N_d) with all options at their defaults on the
     fresh handle; two calls (steps 1.0, 0.5) on one S2 that is zeroed once.  Per call: info == 0; gate_loss, gate_backward_vec,
     gate_forward, gate_update of _gn_reference (the reference of the second call at the device's own z); S2 on the exchanged rows
     |L X - B| <= C eps |L||X| entry by entry with B the long-double [A | F] in the step's column order and every entry left of the
     leading-zero boundary exactly 0.0 (after the second call this is the reuse promise of gpk_mg.h); Darcy: the replicated data rows
     equal gpk_gn_build_rev's bit for bit and the a-part's F column passes the same gate with L2; all ranks agree bit for bit on loss,
     info, delta, z and S2.  The deviation from the one-GPU gpk_gn_step is printed, not gated.
  b. gpk_mg_potrf, panels of 64 and 128 columns, look-ahead off and on, on Theta (adaptive nugget 1e-8 and 1e-10) and the row-scaled
     family at orders 450, 577 and 513 (ragged last panel at both widths): |L L^T - A| <= C eps |L||L^T| on the lower triangle, identical on
     all ranks; world 1 in process (with look-ahead 0 one rank runs gpk_potrf itself, with 1 the plan), worlds 2 .. 4 inside the launches.
     A non-positive pivot in the ragged last panel and in a panel of the last rank: LAPACK's index on every rank (in the launches with
     look-ahead on, the default; world 1 with both).
  c. refusals of gpk_mg_gn_step at world 2 (relaxed system, no Dinv, Darcy without its cached a-part, lds < nz + 1): -9001 with a text on
     both ranks, before any collective (the staged collectives are counted), z untouched.

Every C is 32 x the numpy / scipy figure + 1 at run time (_gn_reference.allowed); nothing is taken from the device.

Shard bounds.  For the elliptic system they are gpk.mg.column_bounds (asserted to contain the four edges).  The library has no host
entry point for the piecewise profiles of the other systems; the ranks log what the staged collectives carry, and in the broadcast form
the bytes per root are the shard widths: those are printed under [mg bounds].

Time.  tests/test_gpu_mg.py::test_native_schedule_several_ranks_one_gpu[3] takes 3.90 s on the MI355X box at the parent commit; each
launch here gets three times that, _mg_rounding.LIMIT = 11.7 s, in the parent's poll loop.  A step case costs 0.03 s with two ranks
and 0.2 s with four (the processes share the queues of one GPU): the whole cross product took 5.8 / 8.8 / 27.6 s at world 2 / 3 / 4,
so worlds 3 and 4 run a cut list (_mg_rounding.step_cases says which; every alignment, every exchange form, both factorisations of Hb
and the shard edges stay for every system).  With it the launches take 6.3 / 6.3 / 7.5 s (104 / 40 / 16 step cases; 2.3 s of each go
before the process group is up), 10.3 s at world 4 in the slowest of four runs.  The in-process world-1 tests take 2 s and 0.1 s.

RESULTS (MI355X; tag: worst device ratio of allowed (numpy figure), units of eps x the gate's scale; printed by test_zz_worst_ratios):
  mg step loss        0.772 of 33 (1)          mg step backward  1.48 of 15.5 (0.453)       mg step forward  1.96e+03 of 3.13e+04 (978)
  mg step update      0.500 of 1               mg step S2        5.97 of 136 (4.2)          mg step S2 a-part F  1.27 of 16.5 (0.485)
  mg potrf gram       9.4 of 308 (9.58)        mg potrf graded   7.02 of 62.4 (1.92)
No gate was missed and no library change was needed: on odd shard starts, empty shards, ranks without a block row and on the reused S2
the sharded step stays within 6 eps of the componentwise scale of S2, a factor 10 .. 40 inside the gates, and all ranks agree bit for
bit.  The iterate deviates from the one-GPU gpk_gn_step by at most 7.3e-14 (Eikonal) in the 2-norm.
Defaults at world 4 (N_d = 65, col_align 128): every system exchanged S by broadcasts ((world - 1) x widest shard > columns: shards
[0, 66, 66, 66, 66] elliptic, [0, 128, 128, 196, 196] Burgers, [0, 128, 196, 196, 196] Eikonal, [0, 256, 384, 384, 391] Darcy) and
factored Hb panel-sharded.  (In the untrimmed list Burgers at N_d = 129 resolved overlap_s = -1 to the all-gather.)
gpk_mg_potrf against gpk_potrf: bit-identical only at world 1 without look-ahead, where it IS gpk_potrf (6 of 6); the plan with panels
of 64 or 128 columns (world 1 with look-ahead, worlds 2 .. 4) differs in the last bits in all 42 cases, so equality is printed
([mg potrf one-gpu]) and NOT asserted at these orders; every rank of a launch holds the same bits.
"""
import hashlib

import numpy as np
import pytest

import _dense_reference as D
import _gn_reference as R
import _mg_rounding as MR

pytestmark = pytest.mark.gpu

LD, EPS = R.LD, R.EPS
WORST = {}
RUNS = {}
KIND = {0: 'broadcasts', 1: 'all-gather', 2: 'direct', 3: 'direct'}


def _note(tag, what, r, a, r_np=None):
    r_np = (a - 1.0) / R.MARGIN if r_np is None else r_np
    w = WORST.setdefault(tag, (0.0, 0.0, a, r_np))
    if not r / a < w[0]:
        WORST[tag] = (r / a, r, a, r_np)
    print(f'[{tag}] {what}: device {r:.3g}, allowed {a:.3g} (numpy {r_np:.3g}); worst so far {WORST[tag][1]:.3g} of {WORST[tag][2]:.3g} '
          f'(numpy {WORST[tag][3]:.3g})')


def _key(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


# ------------------------------------------------------------------------------------------------ the launches
def _matrices(world):
    arrays = {MR.potrf_name(src): MR.potrf_matrix(src) for src in MR.POTRF_SOURCES}
    bad = MR.bad_pivot_cases(world)
    arrays.update({k: v[0] for k, v in bad.items()})
    return arrays, bad


def _run(world, tmp_path_factory):
    """the launch of this world size: once per session, a failure is kept and raised again (no second launch)"""
    if world not in RUNS:
        arrays, bad = _matrices(world)
        spec = dict(step_cases=MR.step_cases(world), potrf=[MR.potrf_name(s) for s in MR.POTRF_SOURCES], bad=sorted(bad), refusals=world == 2)
        try:
            ranks, elapsed = MR.launch(world, spec, arrays, tmp_path_factory.mktemp(f'mg_world{world}'), MR.LIMIT)
            print(f'\n[mg launch] world {world}: {len(spec["step_cases"])} step cases, {elapsed:.1f} s of {MR.LIMIT:.1f} s; rank 0, seconds since its '
                  f'program began: {ranks[0].meta["seconds"]}')
            RUNS[world] = (ranks, bad)
        except Exception as e:                                           # noqa: BLE001
            RUNS[world] = e
    if isinstance(RUNS[world], Exception):
        raise RUNS[world]
    return RUNS[world]


@pytest.fixture(scope='module', params=MR.WORLDS)
def run(request, tmp_path_factory):
    ranks, bad = _run(request.param, tmp_path_factory)
    assert all(b.meta['aborted'] is None for b in ranks), [b.meta['aborted'] for b in ranks]
    return request.param, ranks, bad


# ------------------------------------------------------------------------------------------------ a. the step
REFS = {}


def _refs(cs, z):
    """(vector reference, S2 reference) at z, shared by every case and world that reaches the same z"""
    k = (cs.system, cs.Nd, _key(z))
    if k not in REFS:
        vec = R.vector_reference(cs.system, cs.Nd) if np.array_equal(z, cs.z0) else R.VectorReference(cs, z)
        REFS[k] = (vec, MR.SolveRef(cs, z, vec.lin))
    return REFS[k]


S2_GATES = {}


def _s2_gates(cs, ref, S2):
    k = (cs.system, cs.Nd, _key(ref.B64), _key(S2))
    if k not in S2_GATES:
        S2_GATES[k] = (MR.gate_s2(ref, S2), MR.gate_s2_apart(ref, S2) if cs.system == 'darcy' else None)
    return S2_GATES[k]


def _forms(log, world, xrows):
    """(exchange form of S, Cholesky of Hb, shard widths or None) from the log of one call"""
    s_form = KIND[log[0][0]]
    hb = 'panel-sharded' if tuple(log[-1][:2]) == (1, 4) else 'replicated'
    widths = None
    if s_form == 'broadcasts':
        widths = [0] * world
        for kind, nbytes, root in log:
            if kind != 0:
                break
            widths[root] = nbytes // (8 * xrows)
    return s_form, hb, widths


def test_step(run):
    world, ranks, _ = run
    print()
    found = MR.shard_edges()
    assert all(v is not None for v in found.values()), found          # the elliptic case list contains the four shard edges
    bad = []
    base = ranks[0]
    for c in MR.step_cases(world):
        cid = MR.case_id(c)
        cs = R.case(c['system'], c['Nd'])
        calls = base.meta['steps'][cid]
        for r, other in enumerate(ranks[1:], 1):                         # bit for bit on every rank: equal hashes of the stored arrays
            for a, b in zip(calls, other.meta['steps'][cid]):
                for f in ('rc', 'info', 'loss', 'delta', 'z_in', 'z_out', 'S2'):
                    if a[f] != b[f]:
                        bad.append(f'{cid} step {a["step"]}: rank {r} differs from rank 0 in {f}')
        z_one = [base.get(k) for k in base.meta['one_gpu'][f'{c["system"]}-{c["Nd"]}']]
        for k, call in enumerate(calls):
            what = f'world {world} {cid} call {k + 1}'
            z_in, z_out, delta, S2 = (base.get(call[f]) for f in ('z_in', 'z_out', 'delta', 'S2'))
            loss = float.fromhex(call['loss'])
            if call['info'] != 0 or call['rc'] != 0:
                bad.append(f'{what}: rc = {call["rc"]}, info = {call["info"]}')
            vec, ref = _refs(cs, z_in)
            for name, (r, a) in (('loss', R.gate_loss(vec, loss)), ('backward', R.gate_backward_vec(vec, delta)), ('forward', R.gate_forward(vec, delta))):
                _note(f'mg step {name}', what, r, a)
                if not r <= a:
                    bad.append(f'{what} {name}: {r:.4g} > {a:.4g}')
            u, ua = R.gate_update(z_in, call['step'], delta, z_out)
            WORST['mg step update'] = max(WORST.get('mg step update', 0.0), u)
            if not u <= ua:
                bad.append(f'{what} update of z: {u:.4g} roundings')
            (r, a, ok), apart = _s2_gates(cs, ref, S2)
            _note('mg step S2', what, r, a, ref.np_ratio)
            if not ok:
                bad.append(f'{what} S2: {r:.4g} > {a:.4g} (inf: a non-zero left of the leading-zero boundary, or a NaN)')
            if apart is not None:
                r, a, ok = apart
                _note('mg step S2 a-part F', what, r, a, ref.np_ratio_a)
                if not ok:
                    bad.append(f'{what} S2 a-part F column: {r:.4g} > {a:.4g}')
                rows = S2[ref.data_row0:ref.data_row0 + ref.ndata, :ref.nc]
                if not np.array_equal(rows, base.get(call['data_rows'])):
                    bad.append(f'{what}: the replicated data rows differ from the built rows')
            dev1 = float(np.linalg.norm(z_out - z_one[k]) / np.linalg.norm(z_one[k]))
            s_form, hb, widths = _forms(call['log'], world, ref.xrows)
            print(f'[mg step forms] {what}: S by {s_form}, Hb {hb}; |z - z_one_gpu| / |z_one_gpu| = {dev1:.2e} (update {u:.3f} of {ua:g})')
            if widths is not None and k == 0:
                bounds = list(np.concatenate([[0], np.cumsum(widths)]))
                print(f'[mg bounds] world {world} {cid}: {[int(b) for b in bounds]}')
                if c['system'] == 'elliptic':
                    want = MR.elliptic_bounds(c['Nd'], world, 128 if c['align'] is None else c['align'])
                    if [int(b) for b in bounds] != want:
                        bad.append(f'{what}: shards on the wire {bounds} are not gpk.mg.column_bounds {want}')
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ b. the Cholesky
POTRF = {}


def _potrf_np(src):
    A = MR.potrf_matrix(src)
    return D.worst(*D.res_cholesky(D.np_cholesky(A), A))


def _potrf_gate(src, L):
    k = (MR.potrf_name(src), _key(L))
    if k not in POTRF:
        if ('np', src) not in POTRF:
            POTRF[('np', src)] = _potrf_np(src)
        POTRF[k] = D.gate(D.res_cholesky(L, MR.potrf_matrix(src)), POTRF[('np', src)]) + (POTRF[('np', src)],)
    return POTRF[k]


def _check_factor(bad, what, src, info, L):
    if info != 0:
        bad.append(f'{what}: info = {info}')
        return
    r, a, ok, r_np = _potrf_gate(src, L)
    _note('mg potrf ' + src[0], what, r, a, r_np)
    if not ok:
        bad.append(f'{what}: {r:.4g} > {a:.4g}')


@pytest.mark.parametrize('lookahead', [0, 1])
def test_potrf_world1(lookahead):
    import gpk
    from gpk.mg import MultiGpu
    ctx = gpk.Context(0)
    bad = []
    print()
    try:
        for pw in MR.POTRF_PANELS:
            mgpu = MultiGpu(ctx, 0, 1, panel=pw)
            mgpu.set_option('lookahead', lookahead)
            for src in MR.POTRF_SOURCES:
                A = MR.potrf_matrix(src)
                T = ctx.array(A)
                info = mgpu.potrf(T.ptr, A.shape[0], T.ld)
                L = np.tril(T.download())
                T.free()
                _check_factor(bad, f'world 1 {MR.potrf_name(src)} panel {pw} look-ahead {lookahead}', src, info, L)
                T = ctx.array(A)
                same = ctx.potrf(T) == 0 and np.array_equal(np.tril(T.download()), L)
                T.free()
                print(f'[mg potrf one-gpu] world 1 {MR.potrf_name(src)} panel {pw} look-ahead {lookahead}: equals gpk_potrf bit for bit: {same}')
            if pw == MR.PANEL:
                for name, (A, want) in MR.bad_pivot_cases(1).items():
                    T = ctx.array(A)
                    info = mgpu.potrf(T.ptr, A.shape[0], T.ld)
                    T.free()
                    if info != want:
                        bad.append(f'world 1 {name} look-ahead {lookahead}: info {info}, LAPACK {want}')
            mgpu.close()
    finally:
        ctx.close()
    assert not bad, bad


def test_potrf(run):
    world, ranks, bad_cases = run
    print()
    bad = []
    base = ranks[0]
    for src in MR.POTRF_SOURCES:
        name = MR.potrf_name(src)
        one = base.meta['potrf'][f'{name}/one_gpu']
        for pw in MR.POTRF_PANELS:
            for la in (0, 1):
                k = f'{name}/panel{pw}/la{la}'
                what = f'world {world} {name} panel {pw} look-ahead {la}'
                rec = base.meta['potrf'][k]
                for r, other in enumerate(ranks[1:], 1):
                    o = other.meta['potrf'][k]
                    if (o['rc'], o['info'], o['L']) != (rec['rc'], rec['info'], rec['L']):
                        bad.append(f'{what}: rank {r} differs from rank 0')
                if rec['rc'] != 0:
                    bad.append(f'{what}: rc = {rec["rc"]} {rec["text"]}')
                    continue
                _check_factor(bad, what, src, rec['info'], base.get(rec['L']))
                print(f'[mg potrf one-gpu] {what}: equals gpk_potrf bit for bit: {rec["L"] == one["L"]}')
    for name, (_, want) in bad_cases.items():
        got = [b.meta['bad'][name] for b in ranks]
        if any(g['rc'] != 0 or g['info'] != want for g in got):
            bad.append(f'world {world} {name}: (rc, info) per rank {[(g["rc"], g["info"]) for g in got]}, LAPACK {want}')
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ c. refusals
REFUSALS = {'relaxed': 'elliptic, Eikonal, Burgers and Darcy systems only', 'no_dinv': 'needs the inverted diagonal blocks',
            'darcy_uncached': 'needs its cached a-part', 'short_lds': 'lds/ldh < nz+1'}


def test_refusals_world2(tmp_path_factory):
    ranks, _ = _run(2, tmp_path_factory)
    bad = []
    for name, text in REFUSALS.items():
        for r, b in enumerate(ranks):
            rec = b.meta['refusals'].get(name)
            if rec is None or rec['rc'] != MR.ERR_ARG or text not in rec['text'] or rec['collectives'] != 0 or not rec['z_unchanged']:
                bad.append(f'{name} rank {r}: {rec}')
    assert not bad, bad


def test_zz_worst_ratios():
    """prints the worst device ratio, allowed ratio and numpy figure per tag of this session (the RESULTS block of the docstring)"""
    print()
    for tag, w in sorted(WORST.items()):
        print(f'[mg worst] {tag}: ' + (f'{w:.3f}' if isinstance(w, float) else f'{w[1]:.3g} of {w[2]:.3g} (numpy {w[3]:.3g})'))
