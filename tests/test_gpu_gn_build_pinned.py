"""[A(z) | F(z)] of every Gauss-Newton system as gpk_gn_build and gpk_gn_build_rev write it, pinned bit for bit against
tests/golden/gn_build.npz (written on an MI355X by tests/golden/gen/make_gn_build.py).

The fixture holds the inputs (one seeded iterate z, seeded f, g and Darcy data; the parameters of CASES as JSON) and, per case, the F column
plus (row, col, value) of the non-zero entries of A, for the natural layout and -- every system but the relaxed one -- for the leading-zero
layout.  The factor L is the identity of the right order: the build kernel never reads it.  Shapes: N_d = 37, N_b = 11 (one ragged
workgroup) and N_d = 300, N_b = 21 (the collocation index crosses a 256-thread block inside the domain points and the domain / boundary
split falls inside the second block).  One Monge-Ampere case has a negative radicand: its NaN entries are pinned as NaN.

The fixture is regenerated ONLY when a system's arithmetic is changed on purpose: a refactoring of the build must reproduce it exactly."""
import ctypes as C
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'gn_build.npz')
SHAPES = ((37, 11), (300, 21))
SL_GQ = (0.7, -0.4, 0.3, 1.1, 0.6)                                   # (a1, a2, b, c1, c3): all non-zero
SL3_GQ8 = (0.7, -0.4, 0.9, 0.3, -0.5, 0.8, 1.1, 0.6)                 # (a1, a2, a3, b1, b2, b3, c1, c3): all non-zero
# name -> (system of gpk.SYSTEM, unknown groups per point, keyword arguments of gpk.GNProblem, has a leading-zero layout)
CASES = {
    'elliptic_power': ('Nonlinear_elliptic', 1, dict(p0=1.3, p1=3.0), True),
    'elliptic_sinh': ('Nonlinear_elliptic', 1, dict(nonlin='sinh', p0=0.8, p1=1.2), True),
    'relaxed_power': ('Nonlinear_elliptic_relaxed', 2, dict(p0=1.3, p1=3.0, pen_lambda=7.0), False),
    'relaxed_cubic': ('Nonlinear_elliptic_relaxed', 2, dict(nonlin='cubic', p0=0.8, p1=-0.6, p2=0.4, pen_lambda=7.0), False),
    'burgers': ('Burgers', 3, dict(p0=1.1, p1=0.02), True),
    'eikonal': ('Eikonal', 3, dict(p0=0.1), True),
    'darcy': ('Darcy_flow2d', 6, dict(p0=0.05), True),
    'semilinear': ('Semilinear2d', 3, dict(p0=0.3, gq=SL_GQ), True),
    'monge_ampere': ('MongeAmpere2d', 3, dict(), True),
    'monge_ampere_nan': ('MongeAmpere2d', 3, dict(), True),          # f[5] < 0 far enough for a negative radicand (first shape only)
    'semilinear3d': ('Semilinear3d', 4, dict(gq8=SL3_GQ8), True),
}
KEYS = [(name, Nd, Nb) for name in CASES for Nd, Nb in SHAPES if not (name == 'monge_ampere_nan' and Nd != SHAPES[0][0])]


def key_of(name, Nd, Nb):
    return f'{name}/{Nd}x{Nb}'


def make_inputs(name, Nd, Nb):
    """the seeded inputs of one case (the generator stores them; the test reads them back from the fixture)"""
    system, groups, _, _ = CASES[name]
    rng = np.random.RandomState(1000 + 17 * sorted(CASES).index(name) + Nd)
    sign = np.where(rng.uniform(size=groups * Nd) < 0.5, -1.0, 1.0)
    inp = {'z': sign * rng.uniform(0.25, 1.5, groups * Nd), 'f': rng.uniform(0.5, 1.5, Nd), 'g': rng.normal(size=Nb)}
    if system == 'Darcy_flow2d':
        inp['data'] = rng.normal(size=Nd // 2 + 1)
    if name == 'monge_ampere_nan':
        inp['f'][5] = -10.0
    return inp


def _identity(ctx, n):
    d = ctx.empty(n, n)
    d.zero()
    d.upload(np.eye(n))
    return d


def _problem(ctx, name, Nd, Nb, inp):
    import gpk
    system, _, kw, _ = CASES[name]
    darcy = system == 'Darcy_flow2d'
    rows = {1: 2, 2: 2, 3: 4, 4: 5, 6: 4}[CASES[name][1]] * Nd + Nb
    L = _identity(ctx, rows)
    L2 = _identity(ctx, 3 * Nd) if darcy else None
    # (Darcy's leading-zero layout is entered only with the inverted diagonal blocks at hand: those of the identity)
    prob = gpk.GNProblem(ctx, system, Nd, Nb, inp['f'], inp['g'], L, data_u=inp.get('data'), L2=L2, dinv=256 if darcy else False,
                         cache_a=False, **kw)
    prob.keep += [L] + ([L2] if darcy else [])
    return prob


def _sparse(S, nz):
    A = S[:, :nz]
    r, c = np.nonzero(A != 0)                                        # (NaN != 0: a NaN entry is part of the pattern)
    return {'F': S[:, nz].copy(), 'rows': r.astype(np.int32), 'cols': c.astype(np.int32), 'vals': A[r, c]}


def build_outputs(ctx, name, Nd, Nb, inp):
    """{'nat': ..., 'rev': ...}: gpk_gn_build and (systems with a leading-zero layout) gpk_gn_build_rev of one case, from a poisoned buffer"""
    prob = _problem(ctx, name, Nd, Nb, inp)
    z = ctx.array(inp['z'])
    nz = prob.nz
    assert nz == z.rows
    S = ctx.empty(prob.rows, nz + 1)
    out = {}
    for tag, fn in (('nat', ctx.lib.gpk_gn_build), ('rev', ctx.lib.gpk_gn_build_rev)):
        if tag == 'rev' and not CASES[name][3]:
            continue
        S.upload(np.full((prob.rows, nz + 1), 3.25))
        ctx._chk(fn(ctx.h, C.byref(prob.struct), z.ptr, S.ptr, S.ld))
        out[tag] = _sparse(S.download(), nz)
    return out, prob, z


def _same_bits(got, want):
    """equal bit for bit, NaN equal to NaN"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    ok = ~np.isnan(want)
    return np.array_equal(got[ok].view(np.uint64), want[ok].view(np.uint64))


@pytest.fixture(scope='module')
def pinned():
    with np.load(FIXTURE) as f:
        return {k: f[k] for k in f.files}


def test_fixture_holds_every_case(pinned):
    assert json.loads(str(pinned['cases'])) == json.loads(json.dumps({k: list(v) for k, v in CASES.items()}))
    for name, Nd, Nb in KEYS:
        k = key_of(name, Nd, Nb)
        for tag in ('nat', 'rev') if CASES[name][3] else ('nat',):
            assert {f'{k}/{tag}/{part}' for part in ('F', 'rows', 'cols', 'vals')} <= set(pinned), (k, tag)
        assert f'{k}/rev/F' in pinned or not CASES[name][3]
    nan = key_of('monge_ampere_nan', *SHAPES[0])
    assert np.isnan(pinned[f'{nan}/nat/F']).sum() == 1 and np.isnan(pinned[f'{nan}/nat/vals']).sum() == 2
    assert np.isnan(pinned[f'{nan}/rev/F']).sum() == 1 and np.isnan(pinned[f'{nan}/rev/vals']).sum() == 2


@pytest.mark.parametrize('name,Nd,Nb', KEYS, ids=lambda v: str(v))
def test_build_reproduces_the_fixture(dev_ctx, pinned, name, Nd, Nb):
    ctx, k = dev_ctx, key_of(name, Nd, Nb)
    inp = {part: pinned[f'{k}/in/{part}'] for part in ('z', 'f', 'g', 'data') if f'{k}/in/{part}' in pinned}
    for part, v in make_inputs(name, Nd, Nb).items():                # the stored inputs are the seeded ones
        assert np.array_equal(inp[part], v), (k, part)
    out, prob, z = build_outputs(ctx, name, Nd, Nb, inp)
    try:
        for tag, got in out.items():
            assert np.array_equal(got['rows'], pinned[f'{k}/{tag}/rows']) and np.array_equal(got['cols'], pinned[f'{k}/{tag}/cols']), \
                (k, tag, 'non-zero pattern of A')
            assert _same_bits(got['vals'], pinned[f'{k}/{tag}/vals']), (k, tag, 'values of A')
            assert _same_bits(got['F'], pinned[f'{k}/{tag}/F']), (k, tag, 'F column')
        if Nd == SHAPES[0][0]:                                       # the trial build of the line search at t = 0: the same F, column by column
            delta = ctx.array(np.random.RandomState(5).normal(size=prob.nz))
            W = ctx.empty(prob.rows, 8, ld=8)
            W.zero()
            t = np.zeros(2)
            ctx._chk(ctx.lib.gpk_debug_gn_trial_build(ctx.h, C.byref(prob.struct), z.ptr, delta.ptr, t.ctypes.data_as(C.POINTER(C.c_double)),
                                                      2, W.ptr, 8))
            built = W.download()
            for col in range(2):
                assert _same_bits(built[:, col], out['nat']['F']), (k, 'trial build, column', col)
    finally:
        prob.free()
