"""The long-double reference of tests/_gauss_reference.py on the host (no GPU), and the gate the device tests apply with it.

  - partial() against mpmath.diff of kappa itself at 40 digits
  - theta / theta_test against every array of tests/golden/theta_small.npz (outputs of the reference project's own code), per block
  - oracle/gp_oracle.py's float64 Theta and Theta_test against the reference, per block, on the point sets of
    tests/test_gpu_gram_longdouble.py: the worst figure is the e_np of the device gate
  - a float64 product of the oracle's rows with the coefficients against the long-double one: the bound of the extension test is reachable
  - gate_blocks: rejects an error of 1e-12 in one entry that the whole-matrix assert accepts

Every figure is printed under a [gauss] tag.
"""
import os

import numpy as np
import pytest

import _gauss_reference as GR

LD = GR.LD
G = os.path.join(os.path.dirname(__file__), 'golden')
EPS = float(np.finfo(np.float64).eps)

# (alpha, beta) of every derivative the layouts and the extension functionals combine: per-axis order <= 2 on each side
ORDERS = sorted({(a, b) for fx in GR.FUNCTIONALS.values() for fy in GR.FUNCTIONALS.values() for a in fx for b in fy})


def _mp_pairs(p1, p2):
    """(x1, x2, y1, y2): eight random pairs, one coincident pair, and pairs with p d^2 at 3 - sqrt 6 and 3 + sqrt 6 (the roots of the
    fourth Hermite factor, where its terms cancel) on either axis and on both"""
    rng = np.random.RandomState(11)
    pairs = [tuple(rng.uniform(0, 1, 4)) for _ in range(8)]
    pairs.append((0.3125, 0.71, 0.3125, 0.71))
    r_lo, r_hi = np.sqrt((3 - np.sqrt(6.0)) / p1), np.sqrt((3 + np.sqrt(6.0)) / p1)
    s_lo, s_hi = np.sqrt((3 - np.sqrt(6.0)) / p2), np.sqrt((3 + np.sqrt(6.0)) / p2)
    pairs += [(0.2 + r_lo, 0.4, 0.2, 0.37), (0.2, 0.4, 0.2 + r_hi, 0.43), (0.6, 0.3 + s_hi, 0.58, 0.3), (0.1 + r_hi, 0.5, 0.1, 0.5 + s_lo)]
    return [tuple(float(v) for v in pr) for pr in pairs]


@pytest.mark.parametrize('kernel', GR.KERNELS)
def test_reference_against_mpmath(kernel):
    """Every (alpha, beta) the functionals combine on every pair of _mp_pairs, kp = 0.2 / (0.3, 0.05).  Relative to
    p1^((a1+b1)/2) p2^((a2+b2)/2), the size of such an entry, 4e-18 is asked of the reference: long double has eps 1.1e-19, an entry is
    about ten rounded operations on intermediate values of at most a few times that size (max |He_4(x)| exp(-x^2 / 2) = 3).
    Measured worst: Gaussian 1.1e-19, anisotropic_Gaussian 4.4e-19."""
    import mpmath as mp
    kp = GR.PARAMS[kernel]
    p1f, p2f = (float(v) for v in GR.precisions(kernel, kp))
    worst = 0.0
    with mp.workdps(40):
        s = [mp.mpf(float(v)) for v in np.atleast_1d(kp)]
        p1, p2 = (1 / s[0] ** 2, 1 / s[0] ** 2) if kernel == 'Gaussian' else (2 / s[0] ** 2, 2 / s[1] ** 2)

        def kappa(x1, x2, y1, y2):
            return mp.exp(-(p1 * (x1 - y1) ** 2 + p2 * (x2 - y2) ** 2) / 2)
        for pr in _mp_pairs(p1f, p2f):
            exact = tuple(mp.mpf(v) for v in pr)                      # the float64 values the reference receives
            for al, be in ORDERS:
                want = mp.diff(kappa, exact, (al[0], al[1], be[0], be[1]))
                got = GR.partial(kernel, kp, al, be, *[np.float64(v) for v in pr])
                hi = float(got)
                lo = float(got - LD(hi))                              # long double = hi + lo exactly: no rounding on the way to mpmath
                scale = mp.sqrt(p1) ** (al[0] + be[0]) * mp.sqrt(p2) ** (al[1] + be[1])
                worst = max(worst, float(abs(mp.mpf(hi) + mp.mpf(lo) - want) / scale))
    print(f'\n[gauss] reference vs mpmath {kernel}: worst |diff| / (p1^(n1/2) p2^(n2/2)) = {worst:.2e}')
    assert worst < 4e-18


def test_reference_coincident_values():
    """by hand, p = 1 / sigma^2: <Delta, Delta>(0) = 3 p^2 + 2 p^2 + 3 p^2 = 8 p^2, <d1, d1>(0) = p, <d2^2, d2^2>(0) = 3 p^2"""
    def close(got, want):
        return all(abs(g / w - 1) < 1e-18 for g, w in zip(got, want))
    p = GR.precisions('Gaussian', 0.2)[0]
    assert abs(p - LD(1) / (LD(0.2) * LD(0.2))) < 1e-17 and abs(float(p) - 25.0) < 1e-14
    assert close(GR.diagonal_values('Gaussian', 0.2, 'Nonlinear_elliptic'), [8 * p * p, LD(1)])
    assert close(GR.diagonal_values('Gaussian', 0.2, 'Burgers'), [p, p, 3 * p * p, LD(1)])
    p1, p2 = GR.precisions('anisotropic_Gaussian', (0.3, 0.05))
    assert float(p2) == pytest.approx(800.0, rel=1e-15) and float(p1) == pytest.approx(2 / 0.09, rel=1e-15)
    assert close(GR.diagonal_values('anisotropic_Gaussian', (0.3, 0.05), 'Eikonal'), [p1, p2, 3 * p1 * p1 + 2 * p1 * p2 + 3 * p2 * p2, LD(1)])
    assert close(GR.trace_ratios('Gaussian', 0.2, 'Nonlinear_elliptic', 900, 124), [LD(900) * 8 * p * p / 1024])


# ------------------------------------------------------------------------------------------------ the reference project's outputs
def _fixtures():
    d = np.load(os.path.join(G, 'theta_small.npz'))
    for name in sorted({k.split('__')[0] for k in d.files}):
        kp = d[name + '__kp']
        kernel, kp = ('Gaussian', float(kp[0])) if name.endswith('gauss') else ('anisotropic_Gaussian', (float(kp[0]), float(kp[1])))
        layouts = ('Darcy_u', 'Darcy_a') if name.startswith('darcy') else \
            ({'elliptic': 'Nonlinear_elliptic', 'burgers': 'Burgers', 'eikonal': 'Eikonal'}[name.split('_')[0]],)
        for lay in layouts:
            key = {'Darcy_u': 'Theta_u', 'Darcy_a': 'Theta_a'}.get(lay, 'Theta')
            yield name, lay, kernel, kp, d[name + '__Xd'], d[name + '__Xb'], d[name + '__Xt'], d[f'{name}__{key}'], d[f'{name}__{key}_test']


def test_reference_against_the_golden_fixtures():
    """Theta and Theta_test of all eight fixtures, both Darcy matrices: per block within 4e-15 max|block| (measured worst: 3.7e-16)"""
    worst, count = 0.0, 0
    for name, lay, kernel, kp, Xd, Xb, Xt, want, want_t in _fixtures():
        blocks = GR.offsets(lay, Xd.shape[0], Xb.shape[0])
        T = GR.theta(kernel, kp, lay, Xd, Xb)
        Tt = GR.theta_test(kernel, kp, lay, Xt, Xd, Xb)
        assert T.dtype == LD and np.array_equal(T, T.T)
        w = GR.gate_blocks(want, T, None, blocks, blocks, (name, lay))
        wt = GR.gate_blocks(want_t, Tt, None, [(0, Xt.shape[0])], blocks, (name, lay, 'test'))
        print(f'\n[gauss] fixture {name} {lay}: Theta {w[0]:.3g}, Theta_test {wt[0]:.3g} of max|block|')
        worst = max(worst, w[0], wt[0]); count += 1
    print(f'[gauss] fixtures: worst {worst:.3g} over {count} matrices and their test rows')
    assert count >= 8


# ------------------------------------------------------------------------------------------------ the oracle: e_np of the device gate
def _cases():
    for layout in GR.LAYOUTS:
        for kernel in GR.KERNELS:
            for Nd, Nb in GR.SIZES:
                yield layout, kernel, Nd, Nb
        for k, (Nd, Nb) in enumerate(GR.LARGE):
            yield layout, GR.large_kernel(layout, k), Nd, Nb
    for kernel in GR.KERNELS:
        yield 'Nonlinear_elliptic', kernel, 1, 0


def test_oracle_against_reference_per_block():
    """oracle/gp_oracle.py (float64, the expanded Hermite polynomials) on the point sets of the device test: every block of Theta and of
    Theta_test within 4e-15 max|block| of the reference.  Measured worst e_np: 4.5e-16 (Theta), 3.0e-16 (Theta_test)."""
    worst, worst_t = 0.0, 0.0
    for layout, kernel, Nd, Nb in _cases():
        kp = GR.PARAMS[kernel]
        Xd, Xb, Xt = GR.case_points(Nd, Nb)
        blocks = GR.offsets(layout, Nd, Nb)
        w = GR.gate_blocks(GR.oracle_theta(layout, kernel, kp, Xd, Xb), GR.theta(kernel, kp, layout, Xd, Xb), None, blocks, blocks,
                           (layout, kernel, Nd, Nb))
        wt = GR.gate_blocks(GR.oracle_theta_test(layout, kernel, kp, Xt, Xd, Xb), GR.theta_test(kernel, kp, layout, Xt, Xd, Xb), None,
                            [(0, Xt.shape[0])], blocks, (layout, kernel, Nd, Nb, 'test'))
        print(f'\n[gauss] oracle {layout} {kernel} ({Nd}, {Nb}): e_np {w[0]:.3g} (Theta), {wt[0]:.3g} (Theta_test)')
        worst, worst_t = max(worst, w[0]), max(worst_t, wt[0])
    print(f'[gauss] oracle: worst e_np {worst:.3g} (Theta), {worst_t:.3g} (Theta_test)')


def test_float64_product_meets_the_extension_bound():
    """the bound of the device's gpk_extend test, 64 eps (|rows| @ |coeff|) per test point, is met by a float64 numpy product of the
    oracle's float64 rows with the same inputs (measured worst: 1.7 eps, so the device's other summation order has room)"""
    worst = 0.0
    for layout in GR.LAYOUTS:
        for kernel in GR.KERNELS:
            kp = GR.PARAMS[kernel]
            Nd, Nb = GR.SIZES[1]
            Xd, Xb, Xt = GR.case_points(Nd, Nb)
            Xt = Xt[:67]
            rows = GR.theta_test(kernel, kp, layout, Xt, Xd, Xb)
            coeff = np.random.RandomState(rows.shape[1]).normal(size=rows.shape[1])
            want = rows @ coeff.astype(LD)
            terms = np.abs(rows) @ np.abs(coeff).astype(LD)
            got = GR.oracle_theta_test(layout, kernel, kp, Xt, Xd, Xb) @ coeff
            ratio = float(np.max(np.abs(got.astype(LD) - want) / (EPS * terms)))
            print(f'\n[gauss] float64 rows @ coeff {layout} {kernel}: worst |diff| / (eps |rows| @ |coeff|) = {ratio:.3g}')
            worst = max(worst, ratio)
            assert ratio <= 64
    print(f'[gauss] float64 rows @ coeff: worst {worst:.3g} eps')


# ------------------------------------------------------------------------------------------------ the gate
def test_per_block_gate_rejects_what_the_whole_matrix_assert_accepts():
    """Burgers / anisotropic (0.3, 0.05): max|Theta| is 1.9e6 (the <d2^2, d2^2> block), the value block and the <d1, d1> block have
    maxima 1 and 22.  1e-12 added to one entry of either passes |got - want| <= 4e-15 max|Theta| = 7.7e-9 and fails the per-block gate."""
    Nd, Nb = GR.SIZES[0]
    kernel, kp = 'anisotropic_Gaussian', (0.3, 0.05)
    Xd, Xb, _ = GR.case_points(Nd, Nb)
    ref = GR.theta(kernel, kp, 'Burgers', Xd, Xb)
    want = GR.oracle_theta('Burgers', kernel, kp, Xd, Xb)
    blocks = GR.offsets('Burgers', Nd, Nb)
    assert float(np.max(np.abs(want))) > 1e6
    GR.gate_blocks(want, ref, want, blocks, blocks)                    # unperturbed: passes, with e_np measured as in the device test
    for (ro, _), (co, _), i, j in ((blocks[3], blocks[3], 5, 17), (blocks[0], blocks[0], 9, 2)):
        bad = want.copy()
        bad[ro + i, co + j] += 1e-12
        assert np.max(np.abs(bad - want)) <= 4e-15 * np.max(np.abs(want))                 # the whole-matrix form: accepted
        with pytest.raises(AssertionError):
            GR.gate_blocks(bad, ref, want, blocks, blocks)
        with pytest.raises(AssertionError):
            GR.gate_blocks(bad, want, None, blocks, blocks)            # and in the form tests/test_gpu_parity.py uses
    with pytest.raises(AssertionError):
        GR.gate_blocks(np.full((2, 2), 1e-300), np.zeros((2, 2)), None, [(0, 2)], [(0, 2)])   # a zero block is to be reproduced as zero


def test_gate_reports_the_worst_block():
    ref = np.array([[1.0, 0.0], [0.0, 1000.0]], dtype=LD)
    got = np.array([[1.0 + 2e-15, 0.0], [0.0, 1000.0 + 1e-12]])
    npv = np.array([[1.0 + 4e-16, 0.0], [0.0, 1000.0]])
    e_got, e_np = GR.gate_blocks(got, ref, npv, [(0, 1), (1, 1)], [(0, 1), (1, 1)])
    assert e_got == pytest.approx(2e-15, rel=0.2) and e_np == pytest.approx(4e-16, rel=0.6)
