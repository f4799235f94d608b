"""Shared by tests/test_gpu_mg_rounding.py and tests/test_mg_rounding_host.py: the case lists of the sharded step and the sharded
Cholesky, the gate of the exchanged block S2 = L^-1 [A | F], the launch of several ranks on one GPU and the rank program itself.

Parent and ranks.  A rank that asserts between two collectives leaves its peers waiting in gloo, so the ranks assert NOTHING: each runs
its list of cases (`python _mg_rounding.py spec.json`), writes raw outputs -- return codes, info, loss, delta, z before and after, S2
after the call, factors -- to rank_<r>.npz and prints `ok`.  Arrays are stored once per content (SHA-1 of their bytes), so equal hashes
ARE bit equality and the step cases of a launch cost a few S2 images, not two per case.  A negative return code of a gpk_mg_* call is recorded
and the rank goes straight to its final barrier.  launch() polls the children; as soon as one has exited non-zero or the limit has
passed it terminates the others and raises with their stderr.  It never retries.  The parent computes every reference and applies
every gate.

What a rank can tell about the schedule without new library entry points: the staged collectives of gpk.mg.MultiGpu go through
torch.distributed, so the rank wraps broadcast / all_gather / isend / irecv there and logs (kind, bytes, peer) per call of
gpk_mg_gn_step.  The first entry is the exchange form of S that was taken (all-gather, broadcasts, grouped send / recv); in the
broadcast form the bytes per root are the widths of the column shards (an empty shard issues no broadcast); a closing 4-byte
all-gather is gather_info, i.e. the panel-sharded Cholesky of Hb.
"""
import hashlib
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

import _gn_reference as R

if __name__ != '__main__':                        # (the parent's side: a rank needs neither the dense families nor scipy)
    import _dense_reference as D
    import _staircase_model as M

LD, EPS = R.LD, R.EPS
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

PANEL = 64                                        # panel width of the step's handle: Hb of order 66 .. 775 has 2 .. 13 block rows
SYSTEMS = ('elliptic', 'burgers', 'eikonal', 'darcy')
SIZES = (65, 129)
ALIGNS = (1, 64, 128)
FORMS = ((0, 0), (0, 1), (1, 2), (1, -1))         # (shard_hb, overlap_s)
STEPS = (1.0, 0.5)
WORLDS = (2, 3, 4)
ERR_ARG = -9001                                   # GPK_ERR_ARG of include/gpk.h
# seconds per launch: three times the 3.90 s of tests/test_gpu_mg.py::test_native_schedule_several_ranks_one_gpu[3] on the MI355X box
LIMIT = 3 * 3.90


def _latin(Nd):
    """four of the twelve (col_align, form) pairs: every form once and every alignment at least once"""
    return [(a, f) for ia, a in enumerate(ALIGNS) for jf, f in enumerate(FORMS) if (ia + jf) % 3 == SIZES.index(Nd)]


def step_cases(world):
    """The step cases of one launch, in the order they run: first (system, N_d) with every option left at its default (the handle is
    fresh: col_align 128, overlap_s -1, Hb panel-sharded from four ranks on), then col_align x (shard_hb, overlap_s).  World 2 runs
    the whole cross product at both sizes (104 cases, 6 s of the 11.7 s a launch may take).  A staged collective costs 1.5 ms with two
    ranks and 3 .. 10 ms with three and four (the processes share the queues of one GPU; the whole list took 8.8 s with three ranks and
    27.6 s with four), so it is cut there, keeping for every system every alignment and every exchange form, and the shard edges:
      world 3  N_d = 129 only: the defaults, col_align 1 and 128 (the odd starts and the empty inner shard) with every form, 64 with one;
      world 4  N_d = 65 only (two empty shards, two ranks without a block row of Hb; with the defaults rank 0 owns everything): the
               defaults, which are the pair (128, (1, -1)), and three more pairs per system."""
    full = [(a, f) for a in ALIGNS for f in FORMS]
    if world == 2:
        defaults = [(s, Nd) for s in SYSTEMS for Nd in SIZES]
        pairs = {65: full, 129: full}
    elif world == 3:
        defaults = [(s, 129) for s in SYSTEMS]
        pairs = {65: [], 129: [(a, f) for a, f in full if a != 64 or f == FORMS[1]]}
    else:
        defaults = [(s, 65) for s in SYSTEMS]
        pairs = {65: [(a, f) for a, f in _latin(65) if f != (1, -1)], 129: []}
    out = [dict(system=s, Nd=Nd, align=None, shard_hb=None, overlap_s=None) for s, Nd in defaults]
    out += [dict(system=s, Nd=Nd, align=a, shard_hb=f[0], overlap_s=f[1]) for s in SYSTEMS for Nd in SIZES for a, f in pairs[Nd]]
    return out


def case_id(c):
    if c['align'] is None:
        return f"{c['system']}-{c['Nd']}-defaults"
    return f"{c['system']}-{c['Nd']}-align{c['align']}-hb{c['shard_hb']}-s{c['overlap_s']}"


def elliptic_bounds(Nd, world, align):
    """the column shards gpk_mg_gn_step cuts for the elliptic system (its closed-form profile is the one gpk_mg_column_bounds takes)"""
    from gpk import mg
    return mg.column_bounds(Nd + 1, Nd, 2 * Nd + R.NB[Nd], world, align)


def shard_edges():
    """The four edges the elliptic case list has to contain, each with the (N_d, world, align, bounds, rank) of a case of step_cases that
    shows it (or None)."""
    found = dict(empty_inner=None, odd_start=None, tail_only=None, no_block_row=None)
    for world in WORLDS:
        for c in step_cases(world):
            if c['system'] != 'elliptic':
                continue
            Nd, align = c['Nd'], 128 if c['align'] is None else c['align']          # (128: the default of gpk_mg_set_option key 2)
            nc = Nd + 1
            nblk = -(-nc // PANEL)
            b = elliptic_bounds(Nd, world, align)
            if found['no_block_row'] is None and nblk < world:
                found['no_block_row'] = (Nd, world, align, b, nblk)                # ranks nblk .. world - 1 own no block row of Hb
            for r in range(world):
                c0, c1 = b[r], b[r + 1]
                hit = (Nd, world, align, b, r)
                if found['empty_inner'] is None and c1 == c0 and r < world - 1:
                    found['empty_inner'] = hit
                if found['odd_start'] is None and c1 > c0 and c0 % 2 == 1:
                    found['odd_start'] = hit
                if found['tail_only'] is None and c1 == nc and c0 in (nc - 1, nc - 2):   # only F, or only the last two columns
                    found['tail_only'] = hit
    return found


# ------------------------------------------------------------------------------------------------ the gate of S2
class SolveRef:
    """The exchanged rows of S2 at the point z: B = the long-double [A(z) | F(z)] in the step's column order (unknown j in column
    _staircase_model.column_of_unknown, F last), restricted to the rows of the sharded factor L (all rows; Darcy: the u-part), the
    promised leading-zero profile, and the figure of the float64 scipy substitution under the gate |L X - B| <= C eps |L||X|.
    Darcy: also the a-part's F column (factor L2) and the position of the replicated data rows."""

    def __init__(self, cs, z, lin=None):
        from scipy.linalg import solve_triangular
        lin = lin or R.linearise(cs, z)
        nz = cs.nz
        col = M.column_of_unknown(cs.system, cs.Nd)
        full = np.zeros((cs.rows, nz + 1), dtype=LD)
        full[:, col] = lin.dense()
        full[:, nz] = lin.F
        darcy = cs.system == 'darcy'
        self.xoff = 3 * cs.Nd if darcy else 0
        self.xrows = cs.L.shape[0]
        self.nc, self.L = nz + 1, cs.L
        self.B = full[self.xoff:self.xoff + self.xrows]
        self.first = np.concatenate([M.promised_profile(cs.system, cs.Nd, cs.Nb), [0]])
        self.zero_mask = np.arange(self.xrows)[:, None] < self.first[None, :]
        assert np.all(self.B[self.zero_mask] == 0)
        self.B64 = self.B.astype(np.float64)
        self.X64 = solve_triangular(cs.L, self.B64, lower=True, check_finite=False)
        self.np_ratio = D.worst(*residual(cs.L, self.X64, self.B))
        if darcy:
            self.L2, self.Ba = cs.L2, full[:self.xoff, nz]
            Xa = solve_triangular(cs.L2, self.Ba.astype(np.float64), lower=True, check_finite=False)
            self.np_ratio_a = D.worst(*residual(cs.L2, Xa[:, None], self.Ba[:, None]))
            self.data_row0, self.ndata = self.xoff + self.xrows, cs.Ndata


def residual(L, X, B):
    """(|L X - B| in long double, |L||X|): _dense_reference.res_solve('N') with the scale, a sum of non-negative float64 terms, formed
    by BLAS (relative error n eps = 1e-13 of a bound that carries a factor 32)"""
    L = D.lower(L)
    return np.abs(D.mm(L, X) - D.ld(B)), np.abs(L) @ np.abs(np.asarray(X, dtype=np.float64))


def gate_s2(ref, S2):
    """S2: the whole s_rows x (nz + 1) block a rank holds after the call.  Returns (ratio, allowed, ok): every entry of the exchanged
    rows within allowed() of the numpy figure and every entry left of the leading-zero boundary exactly 0.0."""
    X = np.asarray(S2)[ref.xoff:ref.xoff + ref.xrows, :ref.nc]
    return D.gate(residual(ref.L, X, ref.B), ref.np_ratio, zeros=X[ref.zero_mask])


def gate_s2_apart(ref, S2):
    """Darcy: the a-part's F column L2^-1 [w1; w2; w0] in column nz of the rows [0, 3 N_d)"""
    X = np.asarray(S2)[:ref.xoff, ref.nc - 1]
    return D.gate(residual(ref.L2, X[:, None], ref.Ba[:, None]), ref.np_ratio_a)


def sharded_rendition(ref, bounds):
    """float64 scipy rendition of the sharded solve: every rank solves its columns [c0, c1) only, the shards are assembled into a
    block that was zero before"""
    from scipy.linalg import solve_triangular
    S2 = np.zeros((ref.xoff + ref.xrows, ref.nc))
    for c0, c1 in zip(bounds, bounds[1:]):
        if c1 > c0:
            S2[ref.xoff:, c0:c1] = solve_triangular(ref.L, ref.B64[:, c0:c1], lower=True, check_finite=False)
    return S2


def old_iterate_assert(z, z_ref):
    """tests/test_gpu_mg.py: the iterate of the sharded step within 1e-8 of the one-GPU step in the 2-norm"""
    return bool(np.linalg.norm(z - z_ref) <= 1e-8 * np.linalg.norm(z_ref))


# ------------------------------------------------------------------------------------------------ the Cholesky cases
# Theta with the adaptive nugget at both sizes of it, and the row-scaled family; orders 450, 577 and 513: with panels of 64 and of 128
# columns every one has a ragged last panel (2, 1, 1 and 66, 65, 1 columns)
POTRF_SOURCES = (('gram', ('Darcy_a', 150, 40, 1e-8)), ('gram', ('Nonlinear_elliptic', 250, 77, 1e-10)), ('graded', 513))
POTRF_PANELS = (64, 128)
BAD_ORDER = 513                                   # graded(513), panels of 64: nine panels, the last one is column 512 alone


def potrf_name(src):
    return f'{src[0]}-{D.gram_id(src[1])}' if src[0] == 'gram' else f'{src[0]}-{src[1]}'


def potrf_matrix(src):
    return np.asarray(D.gram(*src[1]) if src[0] == 'gram' else D.graded(src[1]))


def bad_pivot_cases(world):
    """{name: (matrix, LAPACK's info)}: a non-positive pivot in the ragged last panel, and one in a panel the last rank owns"""
    from scipy.linalg.lapack import dpotrf
    out = {}
    for name, idx in (('bad_ragged_last_panel', BAD_ORDER - 1), ('bad_panel_of_last_rank', (world - 1) * PANEL + 5)):
        A = np.array(D.graded(BAD_ORDER))
        A[idx, idx] = -1.0
        info = int(dpotrf(A, lower=1)[1])
        assert info == idx + 1
        out[name] = (A, info)
    return out


# ------------------------------------------------------------------------------------------------ launch
def _free_port():
    s = socket.socket(); s.bind(('127.0.0.1', 0)); p = s.getsockname()[1]; s.close(); return p


class Blobs:
    """the arrays of one rank_<r>.npz: meta (the records of the cases) and the arrays by hash"""

    def __init__(self, path):
        with np.load(path) as f:
            self.arrays = {k: f[k] for k in f.files if k != 'meta'}
            self.meta = json.loads(str(f['meta']))

    def get(self, key):
        return self.arrays[key]


def launch(world, spec, arrays, workdir, limit):
    """Run `world` ranks of this file's rank program on the one GPU; returns [Blobs per rank].  spec: JSON-able dict; arrays: the
    matrices the ranks read (written once to inputs.npz).  Raises RuntimeError with the ranks' stderr if one exits non-zero or the limit
    (seconds) passes; no rank is left running either way."""
    workdir = str(workdir)
    np.savez(os.path.join(workdir, 'inputs.npz'), **arrays)
    spec = dict(spec, workdir=workdir)
    with open(os.path.join(workdir, 'spec.json'), 'w') as f:
        json.dump(spec, f)
    port = _free_port()
    procs, logs = [], []
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
        out = open(os.path.join(workdir, f'rank_{rank}.out'), 'w')
        err = open(os.path.join(workdir, f'rank_{rank}.err'), 'w')
        logs.append((out, err))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), os.path.join(workdir, 'spec.json')], env=env, stdout=out, stderr=err))
    t0 = time.monotonic()
    why = None
    while True:
        codes = [p.poll() for p in procs]
        if all(c == 0 for c in codes):
            break
        if any(c not in (None, 0) for c in codes):
            why = f'a rank exited with {[c for c in codes]}'
        elif time.monotonic() - t0 > limit:
            why = f'the limit of {limit:.0f} s passed with exit codes {codes}'
        if why:
            for p in procs:
                if p.poll() is None:
                    p.terminate()
            for p in procs:
                try:
                    p.wait(timeout=10)
                except subprocess.TimeoutExpired:
                    p.kill(); p.wait()
            break
        time.sleep(0.05)
    for out, err in logs:
        out.close(); err.close()
    elapsed = time.monotonic() - t0

    def tail(name, n=3000):
        with open(os.path.join(workdir, name)) as f:
            return f.read()[-n:]
    if why:
        recorded = []
        for r in range(world):
            p = os.path.join(workdir, f'rank_{r}.npz')
            if os.path.exists(p):
                recorded.append((r, Blobs(p).meta.get('aborted')))
        raise RuntimeError(f'world {world}: {why} after {elapsed:.1f} s; recorded refusals {recorded}; stderr per rank: '
                           + repr([tail(f'rank_{r}.err') for r in range(world)]))
    for r in range(world):
        if 'ok' not in tail(f'rank_{r}.out'):
            raise RuntimeError(f'world {world}: rank {r} did not print ok: {tail(f"rank_{r}.out")!r} {tail(f"rank_{r}.err")!r}')
    return [Blobs(os.path.join(workdir, f'rank_{r}.npz')) for r in range(world)], elapsed


# ------------------------------------------------------------------------------------------------ the rank program
class Aborted(Exception):
    pass


def rank_main(spec_path):
    import ctypes as C
    t_start = time.monotonic()
    with open(spec_path) as f:
        spec = json.load(f)
    for p in (ROOT, os.path.join(ROOT, 'nonlinpdes-gpsolver_amd')):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    import torch.distributed as dist
    import gpk
    from gpk.mg import MultiGpu
    torch.cuda.set_device(0)
    dist.init_process_group('gloo')
    rank, world = dist.get_rank(), dist.get_world_size()
    t_group = round(time.monotonic() - t_start, 2)

    # ---- what the staged collectives put on the wire, per call
    log = []
    real = dict(broadcast=dist.broadcast, all_gather=dist.all_gather, isend=dist.isend, irecv=dist.irecv)
    nbytes = lambda t: int(t.numel() * t.element_size())

    def broadcast(t, src=0, **kw):
        log.append((0, nbytes(t), int(src))); return real['broadcast'](t, src=src, **kw)

    def all_gather(outs, t, **kw):
        log.append((1, nbytes(t), -1)); return real['all_gather'](outs, t, **kw)

    def isend(t, dst=None, **kw):
        log.append((2, nbytes(t), int(dst))); return real['isend'](t, dst=dst, **kw)

    def irecv(t, src=None, **kw):
        log.append((3, nbytes(t), int(src))); return real['irecv'](t, src=src, **kw)
    dist.broadcast, dist.all_gather, dist.isend, dist.irecv = broadcast, all_gather, isend, irecv

    arrays, meta = {}, dict(rank=rank, world=world, steps={}, potrf={}, bad={}, refusals={}, aborted=None, seconds=dict(process_group=t_group))

    def put(a):
        a = np.ascontiguousarray(a)
        key = 'a' + hashlib.sha1(a.tobytes() + repr((a.shape, a.dtype.str)).encode()).hexdigest()
        arrays.setdefault(key, a)
        return key

    ctx = gpk.Context(0)
    lib = ctx.lib
    inputs = np.load(os.path.join(spec['workdir'], 'inputs.npz'))
    handles = {pw: MultiGpu(ctx, rank, world, panel=pw, comm='staged') for pw in POTRF_PANELS}
    mg = handles[PANEL]

    def upload_factor(L):
        n = L.shape[0]
        d = ctx.empty(n, n + R.LD_PAD, ld=n + R.LD_PAD)
        d.upload(R.poisoned(L))
        d.cols = n
        return d

    def problem(cs, system=None, dinv=256, cache_a=True):
        L = upload_factor(cs.L)
        L2 = upload_factor(cs.L2) if cs.L2 is not None else None
        prob = gpk.GNProblem(ctx, R.SYSTEM_NAME[system or cs.system], cs.Nd, cs.Nb, cs.f, cs.g, L, p0=cs.p0, p1=cs.p1, pen_lambda=cs.lam,
                             data_u=cs.data, L2=L2, dinv=dinv, cache_a=cache_a)
        prob.keep += [L] + ([L2] if L2 is not None else [])
        return prob

    def mg_step(h, prob, z, step, S, lds, S2, H, delta):
        loss, info = C.c_double(), C.c_int()
        rc = lib.gpk_mg_gn_step(h.h, C.byref(prob.struct), z.ptr, float(step), S.ptr, int(lds), S2.ptr, H.ptr, H.ld, delta.ptr,
                                C.byref(loss), C.byref(info))
        return rc, loss.value, info.value, (lib.gpk_last_error(ctx.h).decode(errors='replace') if rc < 0 else '')

    def run_steps():
        probs = {}
        for c in spec['step_cases']:
            key = (c['system'], c['Nd'])
            cs = R.case(*key)
            if key not in probs:
                prob = problem(cs)
                S, H, delta, _ = prob.workspace()
                probs[key] = (prob, ctx.empty(S.rows, S.cols, S.ld), ctx.empty(S.rows, S.cols, S.ld))
            prob, S2, Sb = probs[key]
            S, H, delta, _ = prob.workspace()
            if c['align'] is not None:
                mg.set_option('col_align', c['align']); mg.set_option('shard_hb', c['shard_hb']); mg.set_option('overlap_s', c['overlap_s'])
            S2.zero()                                                    # once per case: the second call reuses it
            z = ctx.array(cs.z0)
            calls = []
            for step in STEPS:
                rec = dict(step=step, z_in=put(z.download()))
                if cs.system == 'darcy':                                 # the built data rows the step has to replicate
                    ctx._chk(lib.gpk_gn_build_rev(ctx.h, C.byref(prob.struct), z.ptr, Sb.ptr, Sb.ld))
                    rec['data_rows'] = put(Sb.download(rows=cs.Ndata, row0=7 * cs.Nd + cs.Nb))
                del log[:]
                rc, loss, info, text = mg_step(mg, prob, z, step, S, S.ld, S2, H, delta)
                rec.update(rc=rc, info=info, loss=float(loss).hex(), text=text, log=[list(e) for e in log])
                if rc < 0:
                    calls.append(rec); meta['steps'][case_id(c)] = calls
                    raise Aborted(f'gpk_mg_gn_step {case_id(c)}: {rc} {text}')
                rec.update(delta=put(delta.download()), z_out=put(z.download()), S2=put(S2.download()))
                calls.append(rec)
            meta['steps'][case_id(c)] = calls
            z.free()
        if rank == 0:                                                    # the one-GPU step of the same problems (printed, not gated)
            meta['one_gpu'] = {}
            for (system, Nd), (prob, _, _) in probs.items():
                z = ctx.array(R.case(system, Nd).z0)
                outs = []
                for step in STEPS:
                    ctx.gn_step(prob, z, step)
                    outs.append(put(z.download()))
                meta['one_gpu'][f'{system}-{Nd}'] = outs
                z.free()
        for prob, S2, Sb in probs.values():
            S2.free(); Sb.free(); prob.free()

    def mg_potrf(h, A, n):
        info = C.c_int()
        T = ctx.array(A)
        rc = lib.gpk_mg_potrf(h.h, T.ptr, n, T.ld, C.byref(info))
        text = lib.gpk_last_error(ctx.h).decode(errors='replace') if rc < 0 else ''
        got = np.tril(T.download()) if rc >= 0 else None              # (the strict upper triangle is not part of the factor)
        T.free()
        return rc, info.value, text, got

    def run_potrf():
        for name in spec['potrf']:
            A = inputs[name]
            n = A.shape[0]
            for pw in POTRF_PANELS:
                for la in (0, 1):
                    handles[pw].set_option('lookahead', la)
                    rc, info, text, got = mg_potrf(handles[pw], A, n)
                    meta['potrf'][f'{name}/panel{pw}/la{la}'] = dict(rc=rc, info=info, text=text, L=put(got) if got is not None else None)
                    if rc < 0:
                        raise Aborted(f'gpk_mg_potrf {name} panel {pw} lookahead {la}: {rc} {text}')
                handles[pw].set_option('lookahead', 1)
            if rank == 0:                                                # gpk_potrf of the same matrix (recorded, see the test)
                T = ctx.array(A)
                info = ctx.potrf(T)
                meta['potrf'][f'{name}/one_gpu'] = dict(info=info, L=put(np.tril(T.download())))
                T.free()

    def run_bad():
        for name in spec['bad']:                                         # (look-ahead on, the default; world 1 runs both in process)
            A = inputs[name]
            rc, info, text, _ = mg_potrf(mg, A, A.shape[0])
            meta['bad'][name] = dict(rc=rc, info=info, text=text)
            if rc < 0:
                raise Aborted(f'gpk_mg_potrf {name}: {rc} {text}')

    def run_refusals():
        """every one is refused by gpk_mg_gn_step before its first collective, so no rank waits for another"""
        def attempt(name, cs, prob, short_lds=False):
            S, H, delta, _ = prob.workspace()
            S2 = ctx.empty(S.rows, S.cols, S.ld); S2.zero()
            z = ctx.array(cs.z0)
            del log[:]
            rc, _, _, _ = mg_step(mg, prob, z, 1.0, S, cs.nz if short_lds else S.ld, S2, H, delta)
            meta['refusals'][name] = dict(rc=rc, text=lib.gpk_last_error(ctx.h).decode(errors='replace'), collectives=len(log),
                                          z_unchanged=bool(np.array_equal(z.download(), cs.z0)))
            S2.free(); z.free(); prob.free()
        cs = R.case('relaxed', 65)
        attempt('relaxed', cs, problem(cs))
        cs = R.case('elliptic', 65)
        attempt('no_dinv', cs, problem(cs, dinv=False))
        attempt('short_lds', cs, problem(cs), short_lds=True)
        cs = R.case('darcy', 65)
        attempt('darcy_uncached', cs, problem(cs, cache_a=False))

    try:
        for name, part in (('handles', None), ('steps', run_steps), ('potrf', run_potrf), ('refusals', run_refusals if spec.get('refusals') else None),
                           ('bad', run_bad)):
            if part:
                part()
            meta['seconds'][name] = round(time.monotonic() - t_start, 2)       # (since the rank program began)
    except Aborted as e:
        meta['aborted'] = str(e)
    np.savez(os.path.join(spec['workdir'], f'rank_{rank}.npz'), meta=np.array(json.dumps(meta)), **arrays)
    dist.barrier()
    for h in handles.values():
        h.close()
    dist.destroy_process_group()
    ctx.close()
    print('rank', rank, 'ok', flush=True)


if __name__ == '__main__':
    rank_main(sys.argv[1])
