"""Which of its five modes gpk_gn_step chooses for a problem struct, and the product that follows it (select_mode / select_product of
csrc/gpk_gn.hip), asked through gpk_debug_step_mode of the development build: no step runs, nothing is launched and no pointer of the
struct is dereferenced, so the prepared fields are filled and nulled by hand with any device pointer.  The table is the one of DESIGN.md
('How gpk_gn_step reads'): a mode is chosen only if everything it reads is there, anything less falls through, in the end to Plain."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PLAIN, STRUCT_ELL, GRAM_ELL, STRUCT_GEN, GRAM_GEN = range(5)          # StepMode
NONE, SYRK_POTRF, DARCY = range(3)                                    # StepProduct

ND, NB, NDATA = 64, 16, 8


@pytest.fixture(scope='module')
def problems(dev_ctx):
    """one tiny problem per system, each with the inverted diagonal blocks of its factor(s) and nothing else prepared"""
    import gpk
    ctx = dev_ctx
    rng = np.random.RandomState(40)
    Xd = rng.uniform(0, 1, (ND, 2)); Xb = rng.uniform(0, 1, (NB, 2))
    f = np.ones(ND); g = np.zeros(NB)

    def factor(layout, kernel='Gaussian', par=0.2):
        T, _ = ctx.assemble(layout, kernel, par, Xd, Xb, 1e-6, 'adaptive')
        assert ctx.potrf(T) == 0
        return T
    Te, Tk, Tb, Tu, Ta = (factor('Nonlinear_elliptic'), factor('Eikonal'), factor('Burgers', 'anisotropic_Gaussian', [0.3, 0.05]),
                          factor('Darcy_u'), factor('Darcy_a'))
    probs = {
        'elliptic': gpk.GNProblem(ctx, 'Nonlinear_elliptic', ND, NB, f, g, Te, p0=1.0, p1=3.0, dinv=256),
        'relaxed': gpk.GNProblem(ctx, 'Nonlinear_elliptic_relaxed', ND, NB, f, g, Te, p0=1.0, p1=3.0, pen_lambda=1e-4, dinv=256),
        'eikonal': gpk.GNProblem(ctx, 'Eikonal', ND, NB, f, g, Tk, p0=0.1, dinv=256),
        'burgers': gpk.GNProblem(ctx, 'Burgers', ND, NB, f, g, Tb, p0=1.0, p1=0.02, dinv=256),
        'darcy': gpk.GNProblem(ctx, 'Darcy_flow2d', ND, NB, f, g, Tu, p0=1e-3, data_u=np.zeros(NDATA), L2=Ta, dinv=256, cache_a=False),
    }
    for p in probs.values():
        s = p.struct
        assert s.Dinv and s.dinv_block == 256 and not (s.W1 or s.W2 or s.v0 or s.G or s.pvec)
    assert probs['darcy'].struct.Dinv2
    return probs


# Prepared fields, as offsets from the smallest adequate leading dimensions (ldw = nz + 1 + dw, ldg = nz + dg); a name in `null` is zeroed.
OPS = ('W1', 'W2', 'v0')                  # gpk_gn_structured_prepare (v0: elliptic system only)
GRAM = ('G', 'pvec')                      # gpk_gn_gram_prepare (pvec: elliptic system only)


def _case(fields=(), null=(), dw=0, dg=0, tune=()):
    return dict(fields=tuple(fields), null=tuple(null), dw=dw, dg=dg, tune=tuple(tune))


ELLIPTIC = [
    ('nothing prepared', _case(), PLAIN),
    ('structured', _case(OPS), STRUCT_ELL),
    ('gram wins over structured', _case(OPS + GRAM), GRAM_ELL),
    ('neither needs the inverted blocks', _case(OPS + GRAM, null=('Dinv',)), GRAM_ELL),
    ('structured without inverted blocks', _case(OPS, null=('Dinv',)), STRUCT_ELL),
    ('ldw one short', _case(OPS, dw=-1), PLAIN),
    ('ldw one short, gram', _case(OPS + GRAM, dw=-1), PLAIN),
    ('ldg one short -> structured', _case(OPS + GRAM, dg=-1), STRUCT_ELL),
    ('pvec missing -> structured', _case(OPS + ('G',)), STRUCT_ELL),
    ('v0 missing', _case(('W1', 'W2') + GRAM), PLAIN),
    ('W2 missing', _case(('W1', 'v0') + GRAM), PLAIN),
    ('G and pvec without the operators the Gram level reads', _case(('W2', 'v0') + GRAM), PLAIN),      # the soundness rule
    ('G and pvec alone', _case(GRAM), PLAIN),
    ('switched off', _case(OPS + GRAM, tune=((40, 0),)), PLAIN),
    ('any non-zero value of the switch', _case(OPS + GRAM, tune=((40, 2),)), GRAM_ELL),
]
GENERAL = [
    ('nothing prepared', _case(), PLAIN),
    ('structured, no v0', _case(('W1', 'W2')), STRUCT_GEN),
    ('gram wins over structured, no pvec', _case(('W1', 'W2', 'G')), GRAM_GEN),
    ('everything set', _case(OPS + GRAM), GRAM_GEN),
    ('ldw one short', _case(('W1', 'W2'), dw=-1), PLAIN),
    ('ldw one short, gram', _case(('W1', 'W2', 'G'), dw=-1), PLAIN),
    ('ldg one short -> structured', _case(('W1', 'W2', 'G'), dg=-1), STRUCT_GEN),
    ('W1 missing', _case(('W2', 'G')), PLAIN),
    ('W2 missing', _case(('W1', 'G')), PLAIN),
    ('inverted blocks missing', _case(('W1', 'W2'), null=('Dinv',)), PLAIN),
    ('inverted blocks missing, gram', _case(('W1', 'W2', 'G'), null=('Dinv',)), PLAIN),
    ('block size missing', _case(('W1', 'W2', 'G'), null=('dinv_block',)), PLAIN),
    ('GEMM-only solve switched off', _case(('W1', 'W2', 'G'), tune=((10, 0),)), PLAIN),
    ('dense schedule', _case(('W1', 'W2', 'G'), tune=((23, 0),)), PLAIN),
    ('switched off', _case(('W1', 'W2', 'G'), tune=((40, 0),)), PLAIN),
]
DARCY_ONLY = [
    ('second factor without inverted blocks', _case(('W1', 'W2', 'G'), null=('Dinv2',)), PLAIN),
]
# cases after which Darcy is no longer in its layout 4 (step_layout): the pipelined product instead of its own
DARCY_LEAVES_LAYOUT_4 = {'inverted blocks missing', 'inverted blocks missing, gram', 'block size missing', 'GEMM-only solve switched off',
                         'dense schedule', 'second factor without inverted blocks'}

ROWS = ([('elliptic', n, c, m) for n, c, m in ELLIPTIC]
        + [('relaxed', n, c, PLAIN) for n, c, _ in ELLIPTIC]                                  # the relaxed system: always Plain
        + [(s, n, c, m) for s in ('eikonal', 'burgers', 'darcy') for n, c, m in GENERAL]
        + [('darcy', n, c, m) for n, c, m in DARCY_ONLY])


def _expected_product(system, name, mode):
    if mode in (GRAM_ELL, GRAM_GEN):
        return NONE
    return DARCY if system == 'darcy' and name not in DARCY_LEAVES_LAYOUT_4 else SYRK_POTRF


@pytest.mark.parametrize('system,name,case,mode', ROWS, ids=[f'{r[0]}-{r[1]}'.replace(' ', '_') for r in ROWS])
def test_step_mode_table(dev_ctx, problems, system, name, case, mode):
    from gpk._lib import GNProblemStruct
    ctx, prob = dev_ctx, problems[system]
    s = GNProblemStruct()
    C.memmove(C.byref(s), C.byref(prob.struct), C.sizeof(s))          # a copy: the problem itself stays as built
    some_ptr = prob.struct.L                                          # never dereferenced by the selector
    for name_ in case['fields']:
        setattr(s, name_, some_ptr)
    s.ldw = prob.nz + 1 + case['dw'] if set(case['fields']) & set(OPS) else 0
    s.ldg = prob.nz + case['dg'] if 'G' in case['fields'] else 0
    for name_ in case['null']:
        setattr(s, name_, 0 if name_ == 'dinv_block' else None)
    got_mode, got_product = C.c_int(-1), C.c_int(-1)
    defaults = {40: 1, 10: 1, 23: 1}
    try:
        for k, v in case['tune']:
            ctx.tune(k, v)
        ctx._chk(ctx.lib.gpk_debug_step_mode(ctx.h, C.byref(s), C.byref(got_mode), C.byref(got_product)))
    finally:
        for k, _ in case['tune']:
            ctx.tune(k, defaults[k])
    assert (got_mode.value, got_product.value) == (mode, _expected_product(system, name, mode))


def test_step_mode_argument_checks(dev_ctx, problems):
    """the step's own checks come first (check_prob), and null outputs are refused"""
    from gpk._lib import GNProblemStruct
    ctx, prob = dev_ctx, problems['elliptic']
    m, q = C.c_int(), C.c_int()
    assert ctx.lib.gpk_debug_step_mode(ctx.h, C.byref(prob.struct), None, C.byref(q)) < 0
    assert ctx.lib.gpk_debug_step_mode(ctx.h, C.byref(prob.struct), C.byref(m), None) < 0
    s = GNProblemStruct()
    C.memmove(C.byref(s), C.byref(prob.struct), C.sizeof(s))
    s.L = None
    assert ctx.lib.gpk_debug_step_mode(ctx.h, C.byref(s), C.byref(m), C.byref(q)) < 0
