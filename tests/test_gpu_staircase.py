"""Kernel-level tests of the leading-zero ("staircase") layouts of the Gauss-Newton step (development handle).

gpk_gn_build_rev writes [A(z) | F] in a column order where column c is promised to be zero above row first_row(c); the product of the
solved block (gpk_i_gemm with `lead`, its lower-triangular SYRK form), the substitution solve and the GEMM-only solve through the
inverted diagonal blocks skip work from that promise.  This file checks

  A. the promise: gpk_debug_first_rows against the numpy model of tests/_staircase_model.py (written from the equations), and the
     non-zeros gpk_gn_build_rev actually writes against it.  The two systems that reach Eikonal's layout 2 through the dispatch of
     step_layout / step_profile (csrc/gpk_gn.hip) have tests of their own, at all six N_d: Semilinear (with and without the inverted
     blocks: the closed form, explicitly not Eikonal's two-segment profile; random z, z = 0 and the Eikonal special case
     gq = (0, 0, 1, 0, 0)), Monge-Ampere with the inverted blocks (the two-segment profile; random z and z = 0) and its conservative
     twin (substitution path, gpk_tune key 23 = 2: the closed form).  All comparisons are exact integer comparisons; on an MI355X the
     device agrees with the model in every column at every size;
  B. every consumer of every profile against a dense reference, with operands that are non-zero exactly AT first_row(c): products on
     small integers (exact in fp64 whatever the summation order: compared bit for bit), solves against the same entry point with
     lead = 0 and by their residual in long double; under each launch form (gpk_tune keys) that changes the schedule of these paths.
     Semilinear and Monge-Ampere add nothing here: their profiles are 'eikonal_conservative' and 'eikonal' of PROFILES, at the same
     factor order 4 N_d + N_b;
  C. the column-shard frames of the sharded step (stair_base = c0 for a piecewise profile, lead = n_z - c0 for a closed form).
"""
import contextlib
import ctypes as C
import zlib

import numpy as np
import pytest

import _staircase_model as M

pytestmark = pytest.mark.gpu

ND = (64, 65, 127, 128, 129, 333)                # segment boundaries on and one off the 64 / 128 / 256 edges
NB = {64: 7, 65: 13, 127: 5, 128: 11, 129: 3, 333: 17}
NDATA = {64: 9, 65: 64, 127: 1, 128: 31, 129: 129, 333: 50}
SENT = -7777.25                                  # sentinel of memory a kernel must not write
POISON = 5.0                                     # operand padding: an integer, so that reading it into a result breaks exactness
EPS = np.finfo(np.float64).eps

# gpk_tune keys that change the launch shape of these paths, with their defaults (csrc/gpk_common.h, GpkTune)
DEFAULTS = {0: 0, 3: 1, 6: 0, 16: 0, 30: 0, 33: 1500, 35: 192, 36: 256, 38: 6000, 42: 1, 50: 8000}
FORMS = [None, (0, 1), (0, 2), (0, 3), (0, 4), (33, 1), (38, 1), (50, 1), (35, 1), (36, 1), (6, 1), (16, 1), (30, 4), (3, 0)]
FORM_ND = (65, 129)                              # the launch-form sweep runs at these sizes (every size runs the default form)


@contextlib.contextmanager
def tuned(ctx, form):
    if form is None:
        yield
        return
    key, value = form
    ctx.tune(key, value)
    try:
        yield
    finally:
        ctx.tune(key, DEFAULTS[key])


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _ints(v):
    v = [int(x) for x in v]
    return (C.c_int * max(len(v), 1))(*v)


def set_profile(ctx, lead_div=1, seg=None, base=0):
    seg = seg or ([], [], [], [])
    ctx._chk(ctx.lib.gpk_debug_set_profile(ctx.h, int(lead_div), len(seg[0]), _ints(seg[0]), _ints(seg[1]), _ints(seg[2]),
                                           _ints(seg[3]), int(base)))


def reset_profile(ctx):
    set_profile(ctx)


# ------------------------------------------------------------------------------------------------ A. the promise
SYSTEM_NAME = {'elliptic': 'Nonlinear_elliptic', 'relaxed': 'Nonlinear_elliptic_relaxed', 'burgers': 'Burgers', 'eikonal': 'Eikonal',
               'darcy': 'Darcy_flow2d', 'semilinear': 'Semilinear2d', 'monge_ampere': 'MongeAmpere2d'}
LAYOUT = {'elliptic': 1, 'relaxed': 1, 'burgers': 3, 'eikonal': 2, 'darcy': 4, 'semilinear': 2, 'monge_ampere': 2}
GQ_EIKONAL = (0.0, 0.0, 1.0, 0.0, 0.0)           # N = p^2 + q^2: the Eikonal special case of the semilinear system, dN/du = 0 for every z


def _problem(ctx, system, Nd, dinv=True, gq=None):
    """a GNProblem with identity factors (the build and the layout do not read them) and random, non-zero data (f > 0: the radicand of
    the Monge-Ampere row is positive at every z); gq: the coefficients of the semilinear system (default: _semilinear_reference.GQ)"""
    import gpk
    Nb = NB[Nd]
    rng = np.random.RandomState(Nd)
    order = 2 * Nd + Nb if system in ('elliptic', 'relaxed') else 4 * Nd + Nb
    L = ctx.array(np.eye(order))
    L2 = ctx.array(np.eye(3 * Nd)) if system == 'darcy' else None
    p = dict(elliptic=(1.0, 3.0, 0.0), relaxed=(1.0, 3.0, 1e-3), burgers=(0.7, 0.02, 0.0), eikonal=(0.1, 0.0, 0.0), darcy=(0.05, 0.0, 0.0),
             semilinear=(0.1, 0.0, 0.0), monge_ampere=(0.0, 0.0, 0.0))[system]
    f = rng.uniform(0.5, 1.5, Nd); g = rng.uniform(0.5, 1.5, Nb)
    data = rng.uniform(0.5, 1.5, NDATA[Nd]) if system == 'darcy' else None
    if system == 'semilinear':
        import _semilinear_reference as SL
        gq = SL.GQ if gq is None else gq
    prob = gpk.GNProblem(ctx, SYSTEM_NAME[system], Nd, Nb, f, g, L, p0=p[0], p1=p[1], pen_lambda=p[2], data_u=data, L2=L2,
                         dinv=256 if dinv else False, cache_a=False, gq=gq)
    prob.keep += [L] + ([L2] if L2 is not None else [])
    return prob


def first_rows(ctx, prob):
    nz = prob.nz
    out_u, out_a = (C.c_int * nz)(), (C.c_int * nz)()
    rev = ctx._chk(ctx.lib.gpk_debug_first_rows(ctx.h, C.byref(prob.struct), out_u, out_a))
    return rev, np.array(out_u[:], dtype=np.int64), np.array(out_a[:], dtype=np.int64)


def build(ctx, prob, z, rev=True):
    S = ctx.empty(prob.rows, prob.nz + 1)
    fn = ctx.lib.gpk_gn_build_rev if rev else ctx.lib.gpk_gn_build
    ctx._chk(fn(ctx.h, C.byref(prob.struct), z.ptr, S.ptr, S.ld))
    return S.download()


def _starts(Nd, nz):
    rng = np.random.RandomState(1000 + Nd)
    z = rng.uniform(0.3, 1.2, nz) * rng.choice([-1.0, 1.0], nz)  # no zero entries: every entry of A(z) is non-zero
    assert np.all(z != 0.0)
    return (('random', z), ('zero', np.zeros(nz)))


@pytest.mark.parametrize('Nd', ND)
@pytest.mark.parametrize('system', ['elliptic', 'burgers', 'eikonal', 'darcy'])
def test_build_rev_stays_inside_the_promised_profile(dev_ctx, system, Nd):
    """first_row(c) of the layout gpk_gn_step enters equals the model; it is non-increasing; the first non-zero row gpk_gn_build_rev
    writes in every column is never above it (random z without zeros, and z = 0), and equals it where the profile is exact."""
    ctx = dev_ctx
    Nb = NB[Nd]
    prob = _problem(ctx, system, Nd)
    nz = prob.nz
    rev, fu, fa = first_rows(ctx, prob)
    assert rev == LAYOUT[system]
    assert np.array_equal(fu, M.promised_profile(system, Nd, Nb, 'u' if system == 'darcy' else 'exact'))
    assert np.all(np.diff(fu) <= 0)                              # gpk_stair_first_col bisects on a non-increasing profile
    if system == 'darcy':
        assert np.array_equal(fa, M.promised_profile(system, Nd, Nb, 'a'))
    for name, z0 in _starts(Nd, nz):
        S = build(ctx, prob, ctx.array(z0))[:, :nz]
        if system == 'darcy':
            na = 3 * Nd
            got_a = M.first_nonzero_rows(S[:na])                 # a-part rows (factor L2)
            got_u = M.first_nonzero_rows(S[na:])                 # u-part rows and the data rows below them (factor L, identity)
            assert np.all(got_a >= fa), (name, np.nonzero(got_a < fa)[0][:8])
            assert np.all(got_u >= fu), (name, np.nonzero(got_u < fu)[0][:8])
            if name == 'random':
                assert np.array_equal(got_a, M.exact_first_rows(system, Nd, Nb, 'a'))
                assert np.array_equal(got_u, M.exact_first_rows(system, Nd, Nb, 'u'))
                # the profile is exact over the v0, w0 columns and the v2, v1 columns (the flat step over w2, w1 is the envelope)
                assert np.array_equal(got_u[:2 * Nd], fu[:2 * Nd]) and np.array_equal(got_u[4 * Nd:], fu[4 * Nd:])
                sub = slice(Nd, 4 * Nd)
                assert np.array_equal(got_a[sub], fa[sub])
        else:
            got = M.first_nonzero_rows(S)
            assert np.all(got >= fu), (name, np.nonzero(got < fu)[0][:8])
            if name == 'random':                                 # exact for these layouts
                assert np.array_equal(got, fu)


@pytest.mark.parametrize('Nd', (64, 129, 333))
def test_eikonal_conservative_profile(dev_ctx, Nd):
    """The Eikonal system on the substitution path (no inverted blocks) and under gpk_tune key 23 = 2 keeps the conservative closed form
    (slope 1 over all n_z columns); the build stays inside it."""
    ctx = dev_ctx
    Nb = NB[Nd]
    want = M.promised_profile('eikonal', Nd, Nb, 'conservative')
    for prob, form in ((_problem(ctx, 'eikonal', Nd, dinv=False), None), (_problem(ctx, 'eikonal', Nd), (23, 2))):
        ctx.tune(23, form[1] if form else 1)
        try:
            rev, fu, _ = first_rows(ctx, prob)
            S = build(ctx, prob, ctx.array(_starts(Nd, prob.nz)[0][1]))[:, :prob.nz]
        finally:
            ctx.tune(23, 1)
        assert rev == 2 and np.array_equal(fu, want)
        assert np.all(M.first_nonzero_rows(S) >= fu)


@pytest.mark.parametrize('dinv', [True, False], ids=['dinv', 'substitution'])
@pytest.mark.parametrize('Nd', ND)
def test_semilinear_keeps_the_closed_form(dev_ctx, Nd, dinv):
    """The semilinear system runs Eikonal's layout 2 and, with and without the inverted blocks, the slope-1 closed form -- NOT Eikonal's
    two-segment profile, which would promise zeros over the entries N_u / eps of the v0 columns.  Random z without zeros: the build's
    first non-zeros ARE the profile.  z = 0, and the Eikonal special case gq = (0, 0, 1, 0, 0) (dN/du = 0 for every z: those entries
    are stored zeros): nowhere above it, and the reported profile does not follow the data."""
    ctx = dev_ctx
    Nb = NB[Nd]
    want = M.promised_profile('semilinear', Nd, Nb)
    assert np.array_equal(want, M.closed_form(3 * Nd, 3 * Nd))
    prob = _problem(ctx, 'semilinear', Nd, dinv=dinv)
    nz = prob.nz
    rev, fu, _ = first_rows(ctx, prob)
    assert rev == LAYOUT['semilinear'] == 2
    assert np.array_equal(fu, want), np.nonzero(fu != want)[0][:8]
    assert not np.array_equal(fu, M.promised_profile('eikonal', Nd, Nb))
    assert np.all(np.diff(fu) <= 0)
    for name, z0 in _starts(Nd, nz):
        got = M.first_nonzero_rows(build(ctx, prob, ctx.array(z0))[:, :nz])
        assert np.all(got >= fu), (name, np.nonzero(got < fu)[0][:8])
        if name == 'random':
            assert np.array_equal(got, fu), np.nonzero(got != fu)[0][:8]
            assert np.array_equal(got, M.exact_first_rows('semilinear', Nd, Nb))
    special = _problem(ctx, 'semilinear', Nd, dinv=dinv, gq=GQ_EIKONAL)
    rev, fs, _ = first_rows(ctx, special)
    assert rev == 2 and np.array_equal(fs, want)
    got = M.first_nonzero_rows(build(ctx, special, ctx.array(_starts(Nd, nz)[0][1]))[:, :nz])
    assert np.all(got >= fs)
    assert np.array_equal(got, M.exact_first_rows('eikonal', Nd, Nb))    # (what is left when N_u vanishes: Eikonal's pattern)


@pytest.mark.parametrize('Nd', ND)
def test_monge_ampere_two_segment_profile(dev_ctx, Nd):
    """Monge-Ampere on the GEMM-only solve path: layout 2 with Eikonal's two-segment profile; random z: the build's first non-zeros are
    the profile; z = 0 (v1 / s = v2 / s = 0 with s = 2 sqrt(f) > 0): nowhere above it."""
    ctx = dev_ctx
    Nb = NB[Nd]
    want = M.stair_eval(M.stair_encoding('eikonal', Nd), 3 * Nd)
    assert np.array_equal(want, M.promised_profile('monge_ampere', Nd, Nb))
    prob = _problem(ctx, 'monge_ampere', Nd)
    nz = prob.nz
    rev, fu, _ = first_rows(ctx, prob)
    assert rev == LAYOUT['monge_ampere'] == 2
    assert np.array_equal(fu, want), np.nonzero(fu != want)[0][:8]
    assert np.all(np.diff(fu) <= 0)
    for name, z0 in _starts(Nd, nz):
        S = build(ctx, prob, ctx.array(z0))
        assert np.all(np.isfinite(S))
        got = M.first_nonzero_rows(S[:, :nz])
        assert np.all(got >= fu), (name, np.nonzero(got < fu)[0][:8])
        if name == 'random':
            assert np.array_equal(got, fu), np.nonzero(got != fu)[0][:8]


@pytest.mark.parametrize('Nd', (64, 129, 333))
def test_monge_ampere_conservative_profile(dev_ctx, Nd):
    """The twin of test_eikonal_conservative_profile: Monge-Ampere on the substitution path and under gpk_tune key 23 = 2 reports the
    conservative closed form; the build stays inside it."""
    ctx = dev_ctx
    Nb = NB[Nd]
    want = M.promised_profile('monge_ampere', Nd, Nb, 'conservative')
    assert np.array_equal(want, M.closed_form(3 * Nd, 3 * Nd))
    for prob, form in ((_problem(ctx, 'monge_ampere', Nd, dinv=False), None), (_problem(ctx, 'monge_ampere', Nd), (23, 2))):
        ctx.tune(23, form[1] if form else 1)
        try:
            rev, fu, _ = first_rows(ctx, prob)
            S = build(ctx, prob, ctx.array(_starts(Nd, prob.nz)[0][1]))[:, :prob.nz]
        finally:
            ctx.tune(23, 1)
        assert rev == 2 and np.array_equal(fu, want)
        assert np.all(M.first_nonzero_rows(S) >= fu)


@pytest.mark.parametrize('Nd', (64, 65, 333))
def test_relaxed_system_layout(dev_ctx, Nd):
    """The relaxed elliptic system: gpk_gn_build_rev refuses it; gpk_gn_step still runs it in the slope-1 layout (unknown j in column
    n_z - 1 - j), and its natural-order build, so permuted, stays inside that profile."""
    ctx = dev_ctx
    Nb = NB[Nd]
    prob = _problem(ctx, 'relaxed', Nd)
    z = ctx.array(_starts(Nd, prob.nz)[0][1])
    with pytest.raises(Exception):
        build(ctx, prob, z)
    rev, fu, _ = first_rows(ctx, prob)
    assert rev == 1 and np.array_equal(fu, M.promised_profile('relaxed', Nd, Nb))
    nat = build(ctx, prob, z, rev=False)[:, :prob.nz]
    S = np.zeros_like(nat)
    S[:, M.column_of_unknown('relaxed', Nd)] = nat
    assert np.array_equal(M.first_nonzero_rows(S), fu)


def test_dense_schedule_has_no_profile(dev_ctx):
    """Darcy without inverted blocks runs the dense schedule: there is no leading-zero layout to report."""
    ctx = dev_ctx
    prob = _problem(ctx, 'darcy', 64, dinv=False)
    with pytest.raises(Exception):
        first_rows(ctx, prob)


# ------------------------------------------------------------------------------------------------ B. every consumer
PROFILES = ('elliptic', 'burgers', 'eikonal', 'eikonal_conservative', 'darcy_u', 'darcy_a')


def _case(name, Nd):
    """the operand shape of one profile as the step hands it to the kernels: n = order of the factor, ncols = columns the kernels see
    (the F column included), width = columns of the buffer, off = the kernels' column 0 in it; lead / lead_div / seg as the step
    passes them; fr = first_row of each of the ncols columns (the model)"""
    Nb = NB[Nd]
    if name == 'elliptic':
        n, nz, ld, seg = 2 * Nd + Nb, Nd, 1, None
        fr = M.closed_form(nz + 1, nz)
        assert np.array_equal(fr[:nz], M.promised_profile('elliptic', Nd, Nb))
        return dict(n=n, ncols=nz + 1, width=nz + 1, off=0, lead=nz, lead_div=1, seg=None, fr=fr)
    if name == 'burgers':
        nz = 3 * Nd
        fr = M.closed_form(nz + 1, nz, 3)
        assert np.array_equal(fr[:nz], M.promised_profile('burgers', Nd, Nb))
        return dict(n=4 * Nd + Nb, ncols=nz + 1, width=nz + 1, off=0, lead=nz, lead_div=3, seg=None, fr=fr)
    if name == 'eikonal_conservative':
        nz = 3 * Nd
        return dict(n=4 * Nd + Nb, ncols=nz + 1, width=nz + 1, off=0, lead=nz, lead_div=1, seg=None, fr=M.closed_form(nz + 1, nz))
    if name in ('eikonal', 'darcy_u'):
        system = name.split('_')[0]
        nz = M.n_unknowns(system, Nd)
        seg = M.stair_encoding(system, Nd)
        fr = M.stair_eval(seg, nz + 1)
        assert np.array_equal(fr[:nz], M.promised_profile(system, Nd, Nb, 'u' if system == 'darcy' else 'exact'))
        return dict(n=4 * Nd + Nb, ncols=nz + 1, width=nz + 1, off=0, lead=1, lead_div=1, seg=seg, fr=fr)
    if name == 'darcy_a':                        # slope 1 on the sub-range [N_d, 4 N_d) of the 6 N_d + 1 columns
        fr = M.closed_form(3 * Nd, 3 * Nd)
        assert np.array_equal(fr, M.promised_profile('darcy', Nd, Nb, 'a')[Nd:4 * Nd])
        return dict(n=3 * Nd, ncols=3 * Nd, width=6 * Nd + 1, off=Nd, lead=3 * Nd, lead_div=1, seg=None, fr=fr)
    raise ValueError(name)


def _staircase(rng, rows, case):
    """rows x width integers in [-8, 8], zero above first_row(c), NON-zero at first_row(c) in every column the kernels see"""
    B = rng.integers(-8, 9, size=(rows, case['width'])).astype(np.float64)
    off, fr = case['off'], case['fr']
    r = np.arange(rows)[:, None]
    Bk = B[:, off:off + case['ncols']]
    Bk[r < fr[None, :]] = 0.0
    Bk[fr, np.arange(case['ncols'])] = rng.choice([-8, -5, -3, -1, 1, 2, 4, 7], size=case['ncols'])
    return B


def _upload_padded(ctx, host, ld, pad_value):
    """device array of host's shape with leading dimension ld, the padding columns filled with pad_value"""
    full = np.full((host.shape[0], ld), pad_value)
    full[:, :host.shape[1]] = host
    d = ctx.empty(host.shape[0], ld, ld=ld)
    d.upload(full)
    return d


def _set(ctx, case, base=0):
    set_profile(ctx, case['lead_div'], case['seg'], base)


ALPHA_BETA = [(1.0, 0.0), (-1.0, 1.0), (2.0, -1.0), (0.5, 2.0), (0.0, 0.5), (1.0, 1.0)]


def _products(ctx, name, Nd, form):
    case = _case(name, Nd)
    rng = np.random.default_rng(_seed(name, Nd))
    k = case['n'] + 5                             # (the step's products also run over rows below the factor's: data / penalty rows)
    S = _staircase(rng, k, case)
    off, n = case['off'], case['ncols']
    lds = case['width'] + 3                       # odd padding: the 16-byte paths see unaligned rows
    dS = _upload_padded(ctx, S, lds, POISON)
    Sk = S[:, off:off + n]
    m = 130
    A = rng.integers(-8, 9, size=(k, m)).astype(np.float64)
    dA = _upload_padded(ctx, A, m + 2, POISON)
    i = ND.index(Nd) + PROFILES.index(name)
    with tuned(ctx, form):
        # gpk_gemm_lz(ta = 1): C (m x n) <- alpha A^T S + beta C
        for alpha, beta in (ALPHA_BETA[i % 6], ALPHA_BETA[(i + 3) % 6]):
            C0 = rng.integers(-8, 9, size=(m, n)).astype(np.float64)
            ldc = n + 5
            dC = _upload_padded(ctx, C0, ldc, SENT)
            _set(ctx, case)
            ctx._chk(ctx.lib.gpk_gemm_lz(ctx.h, 1, m, n, k, alpha, dA.ptr, dA.ld, dS.at(0, off), dS.ld, beta, dC.ptr, dC.ld, case['lead']))
            got = dC.download()
            want = alpha * (A.T @ Sk) + beta * C0                # every partial sum is an integer below 2^53: exact
            assert np.array_equal(got[:, :n], want), ('gemm_lz', name, Nd, form, alpha, beta, np.argwhere(got[:, :n] != want)[:4])
            assert np.all(got[:, n:] == SENT), ('gemm_lz wrote the padding', name, Nd, form)
        # gpk_debug_syrk_lz: lower tiles of C (n x n) <- alpha S^T S + beta C
        for alpha, beta in (ALPHA_BETA[(i + 1) % 6], ALPHA_BETA[(i + 4) % 6]):
            C0 = rng.integers(-8, 9, size=(n, n)).astype(np.float64)
            C0[np.triu_indices(n, 1)] = SENT
            ldc = n + 3
            dC = _upload_padded(ctx, C0, ldc, SENT)
            _set(ctx, case)
            ctx._chk(ctx.lib.gpk_debug_syrk_lz(ctx.h, n, k, alpha, dS.at(0, off), dS.ld, beta, dC.ptr, dC.ld, case['lead']))
            got = dC.download()
            full = alpha * (Sk.T @ Sk)
            want = full + beta * np.tril(C0)
            lo = np.tril_indices(n)
            assert np.array_equal(got[lo], want[lo]), ('syrk_lz', name, Nd, form, alpha, beta,
                                                        np.argwhere(np.tril(got[:, :n] != want))[:4])
            assert np.all(got[:, n:] == SENT), ('syrk_lz wrote the padding', name, Nd, form)
            # strictly upper entries: untouched outside the diagonal tiles (<= 128 x 128, aligned); a diagonal tile may store its upper
            # part, and then with the values of the full product
            up = np.triu(np.ones((n, n), dtype=bool), 1)
            same_tile = (np.arange(n)[:, None] // 128) == (np.arange(n)[None, :] // 128)
            g = got[:, :n]
            assert np.all(g[up & ~same_tile] == SENT), ('syrk_lz wrote above the diagonal tiles', name, Nd, form)
            w = up & same_tile & (g != SENT)
            assert np.array_equal(g[w], (full + beta * SENT)[w]) or np.array_equal(g[w], full[w]) or not w.any(), \
                ('syrk_lz: wrong values in the upper part of a diagonal tile', name, Nd, form)
    reset_profile(ctx)


_FACTORS = {}


def _factor(ctx, n, kind, Nd):
    """(host L, device L): 'spd' = Cholesky factor of a random SPD matrix; 'gram' = a device-assembled, device-factored Gram matrix
    (Eikonal layout, order 4 N_d + N_b)"""
    key = (id(ctx), n, kind, Nd)
    if key not in _FACTORS:
        if kind == 'spd':
            rng = np.random.RandomState(n)
            G = rng.normal(size=(n, n))
            L = np.linalg.cholesky(G @ G.T / n + np.eye(n))
            dL = ctx.array(L)
        else:
            rng = np.random.RandomState(77)
            Xd = rng.uniform(0, 1, (Nd, 2)); Xb = rng.uniform(0, 1, (NB[Nd], 2))
            dL, _ = ctx.assemble('Eikonal', 'Gaussian', 0.2, Xd, Xb, 1e-8, 'adaptive')
            assert dL.rows == n and ctx.potrf(dL) == 0
            ctx.tril(dL)
            L = dL.download()
        _FACTORS[key] = (L, dL, {})
    return _FACTORS[key]


def _dinv(ctx, fac, block):
    L, dL, cache = fac
    if block not in cache:
        cache[block] = ctx.trtri_diag(dL, block=block)
    return cache[block]


def _solve(ctx, case, dL, B, entry, lead, block=None, Dinv=None, col0=0, ncols=None, base=0):
    """solve the columns [col0, col0 + ncols) of the case's operand (the kernels' frame) with one entry point; returns the full n x width
    X as downloaded (sentinel outside those columns and in the padding: checked here)"""
    n, off, width = case['n'], case['off'], case['width']
    ncols = case['ncols'] - col0 if ncols is None else ncols
    ld = width + 3
    dB = _upload_padded(ctx, B, ld, POISON)
    c = off + col0
    if entry == 'lz':
        _set(ctx, case, 0)
        ctx._chk(ctx.lib.gpk_trsm_lz(ctx.h, dL.ptr, n, dL.ld, dB.at(0, c), ncols, dB.ld, lead))
        X = dB.download()
        X[:, :c] = SENT; X[:, c + ncols:] = SENT            # (in place: B's other columns are not the solve's business)
    else:
        X0 = np.full((n, ld), SENT)
        X0[:, c:c + ncols] = 0.0                             # the solve's own columns: zero on entry (gpk_trsm_dinv's contract)
        dX = ctx.empty(n, ld, ld=ld)
        dX.upload(X0)
        _set(ctx, case, base)
        ctx._chk(ctx.lib.gpk_trsm_dinv(ctx.h, dL.ptr, Dinv.ptr, block, n, dL.ld, dB.at(0, c), ncols, dB.ld, dX.at(0, c), dX.ld, lead))
        X = dX.download()
        assert np.all(X[:, :c] == SENT) and np.all(X[:, c + ncols:] == SENT), ('trsm_dinv wrote outside its columns', case['off'], col0)
    reset_profile(ctx)
    return X


def _check_solution(case, L, B, X, tol, what):
    """X exactly zero above the boundary; the residual L X - B in long double on a sample of columns (the boundary columns of every
    tile and segment edge and some random ones), componentwise: |L X - B| <= tol (|L| |X| + |B|)"""
    off, n, fr = case['off'], case['ncols'], case['fr']
    Xk, Bk = X[:, off:off + n], B[:, off:off + n]
    r = np.arange(case['n'])[:, None]
    above = r < fr[None, :]
    assert np.all(Xk[above] == 0.0), (what, 'non-zero above the boundary', np.argwhere(above & (Xk != 0))[:4])
    cols = {0, n - 1}
    for e in range(64, n + 1, 64):
        cols.update({e - 2, e - 1, e} & set(range(n)))
    if case['seg']:
        for b in case['seg'][0]:
            cols.update({b - 1, b, b + 1} & set(range(n)))
    cols = sorted(cols | set(np.random.RandomState(n).choice(n, min(n, 16), replace=False).tolist()))
    Ll = L.astype(np.longdouble)
    Xs = Xk[:, cols].astype(np.longdouble)
    R = np.abs(Ll @ Xs - Bk[:, cols])
    bound = tol * (np.abs(Ll) @ np.abs(Xs) + np.abs(Bk[:, cols]))
    bad = R > bound
    assert not bad.any(), (what, 'residual', np.argwhere(bad)[:4], float(np.max(R / np.maximum(bound, 1e-300))))


def _solves(ctx, name, Nd, form, kind='spd', blocks=(256, 1024)):
    case = _case(name, Nd)
    n = case['n']
    fac = _factor(ctx, n, kind, Nd)
    L, dL, _ = fac
    rng = np.random.default_rng(_seed(name, Nd, 'solve'))
    B = _staircase(rng, n, case)
    off, nc = case['off'], case['ncols']
    # componentwise backward error of the substitution solve ~ n eps; the inverted-block solve multiplies it by the condition of the
    # diagonal blocks, small for the random SPD factor.  The Gram factor (condition ~1e8) is checked normwise against the lead = 0 solve.
    tol = 8 * n * EPS
    with tuned(ctx, form):
        if case['seg'] is None:                   # the substitution solve understands the closed forms only (as in gpk_gn_step)
            X0 = _solve(ctx, case, dL, B, 'lz', 0)
            X = _solve(ctx, case, dL, B, 'lz', case['lead'])
            _compare(case, X, X0, kind, ('trsm_lz', name, Nd, form, kind))
            if kind == 'spd' and form is None:
                _check_solution(case, L, B, X, tol, ('trsm_lz', name, Nd))
        for block in blocks:
            D = _dinv(ctx, fac, block)
            X0 = _solve(ctx, case, dL, B, 'dinv', 0, block, D)
            X = _solve(ctx, case, dL, B, 'dinv', case['lead'], block, D)
            _compare(case, X, X0, kind, ('trsm_dinv', block, name, Nd, form, kind))
            if kind == 'spd' and form is None:
                _check_solution(case, L, B, X, tol, ('trsm_dinv', block, name, Nd))
    return case, B


def _compare(case, X, X0, kind, what):
    off, n, fr = case['off'], case['ncols'], case['fr']
    Xk, X0k = X[:, off:off + n], X0[:, off:off + n]
    above = np.arange(case['n'])[:, None] < fr[None, :]
    assert np.all(Xk[above] == 0.0), (what, 'non-zero above the boundary')
    # skipping exact zeros changes the launch shapes (active column ranges, K starts, tile lists): same solution to rounding
    scale = np.max(np.abs(X0k), axis=0)
    tol = 1e-13 if kind == 'spd' else 1e-9
    dev = np.max(np.abs(Xk - X0k), axis=0)
    assert np.all(dev <= tol * scale), (what, 'differs from the lead = 0 solve', int(np.argmax(dev / np.maximum(scale, 1e-300))),
                                        float(np.max(dev / np.maximum(scale, 1e-300))))


@pytest.mark.parametrize('Nd', ND)
@pytest.mark.parametrize('name', PROFILES)
def test_products_default_form(dev_ctx, name, Nd):
    _products(dev_ctx, name, Nd, None)


@pytest.mark.parametrize('form', FORMS[1:], ids=lambda f: f'key{f[0]}={f[1]}')
@pytest.mark.parametrize('Nd', FORM_ND)
@pytest.mark.parametrize('name', PROFILES)
def test_products_launch_forms(dev_ctx, name, Nd, form):
    _products(dev_ctx, name, Nd, form)


@pytest.mark.parametrize('Nd', ND)
@pytest.mark.parametrize('name', PROFILES)
def test_solves_default_form(dev_ctx, name, Nd):
    _solves(dev_ctx, name, Nd, None)


@pytest.mark.parametrize('form', FORMS[1:], ids=lambda f: f'key{f[0]}={f[1]}')
@pytest.mark.parametrize('Nd', FORM_ND)
@pytest.mark.parametrize('name', PROFILES)
def test_solves_launch_forms(dev_ctx, name, Nd, form):
    _solves(dev_ctx, name, Nd, form, blocks=(256,))


@pytest.mark.parametrize('name', ['burgers', 'eikonal', 'eikonal_conservative', 'darcy_u'])
def test_solves_with_a_gram_factor(dev_ctx, name):
    """the same solves against a device-assembled, device-factored Gram matrix (order 4 N_d + N_b, N_d = 129)"""
    _solves(dev_ctx, name, 129, None, kind='gram')


# ------------------------------------------------------------------------------------------------ C. shard frames
def _cuts(case):
    n = case['ncols']
    cuts = {0, 63, 65, 127, 129}
    if case['seg']:
        for b in case['seg'][0]:
            cuts.update({b - 1, b + 1})
    else:
        cuts.update({case['lead'] - 1, case['lead'] + 1})   # the end of the staircase (columns >= lead are dense)
    cuts.add(int(np.random.RandomState(n).randint(1, n - 1)))
    return sorted(c for c in cuts if 0 <= c < n)


@pytest.mark.parametrize('bitwise', [False, True], ids=['default', 'no-tile-lists'])
@pytest.mark.parametrize('Nd', (65, 129))
@pytest.mark.parametrize('name', ['elliptic', 'burgers', 'eikonal', 'eikonal_conservative', 'darcy_u'])
def test_shard_frames(dev_ctx, name, Nd, bitwise):
    """The sharded step solves the columns [c0, c1) of [A | F] on its own: a piecewise profile with stair_base = c0, a closed form with
    lead = n_z - c0 (gpk_mg_gn_step).  Two shards cut at c0 must give the columns of the unsharded solve.  With tile lists off (gpk_tune
    key 42 = 0) and no split-K, every entry is the same sequence of MFMA slabs whatever the tile it lands in -- only exact zeros are
    skipped in addition -- so the shards must agree BIT FOR BIT; with tile lists on (default) a launch of another shape may cut its K
    range differently, and the shards must agree to 1e-13 relative."""
    ctx = dev_ctx
    case = _case(name, Nd)
    fac = _factor(ctx, case['n'], 'spd', Nd)
    L, dL, _ = fac
    D = _dinv(ctx, fac, 256)
    B = _staircase(np.random.default_rng(_seed(name, Nd, 'shard')), case['n'], case)
    off, nc = case['off'], case['ncols']
    form = (42, 0) if bitwise else None
    with tuned(ctx, form):
        full = _solve(ctx, case, dL, B, 'dinv', case['lead'], 256, D)[:, off:off + nc]
        for c0 in _cuts(case):
            parts = []
            for a0, a1 in ((0, c0), (c0, nc)):
                if a1 <= a0:
                    continue
                if case['seg']:
                    lead, base = 1, a0
                else:
                    lead, base = max(case['lead'] - a0, 0), 0
                X = _solve(ctx, case, dL, B, 'dinv', lead, 256, D, col0=a0, ncols=a1 - a0, base=base)
                parts.append(X[:, off + a0:off + a1])
            got = np.concatenate(parts, axis=1)
            if bitwise:
                assert np.array_equal(got, full), (name, Nd, c0, np.argwhere(got != full)[:4])
            else:
                scale = np.max(np.abs(full), axis=0)
                assert np.all(np.abs(got - full) <= 1e-13 * scale), (name, Nd, c0)
