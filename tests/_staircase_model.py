"""Independent numpy model of the leading-zero ("staircase") layouts of the Gauss-Newton step.

Written from the equations, not from csrc/: for every unknown, the rows of A(z) in which it has an entry (src/PDEs.py and
src/InverseProblems.py of the reference, summarised at the top of csrc/gpk_gn.hip), and the staircase order in which gpk_gn_step
stores the unknowns (column c of [A(z) | F] holds the unknown at staircase position n_z - 1 - c).  From those two facts:

  exact_first_rows   the first row of every column that can be non-zero for a generic z,
  promised_profile   what the kernels are told: the largest non-increasing profile below the exact one (gpk_stair_first_col bisects on
                     a non-increasing profile), or, for the closed forms, the formula the layout uses;
  stair_encoding     the same profile written as the segments (c1, a, b, sd) of a piecewise profile, and stair_eval, which evaluates
                     such segments (the tests check the encoding against the profile, then hand it to the library).

Row numbers are relative to the first row of the factor's row group.  NONE marks a column without a non-zero in the group.
"""
import numpy as np

NONE = np.iinfo(np.int64).max
FLAT = 1 << 30                        # slope divisor of a flat segment


def systems():
    return ('elliptic', 'relaxed', 'burgers', 'eikonal', 'darcy', 'semilinear', 'monge_ampere')


def n_unknowns(system, Nd):
    return {'elliptic': Nd, 'relaxed': 2 * Nd, 'burgers': 3 * Nd, 'eikonal': 3 * Nd, 'darcy': 6 * Nd, 'semilinear': 3 * Nd,
            'monge_ampere': 3 * Nd}[system]


def _entries(system, Nd, Nb, group='u'):
    """(unknown index in the natural order, row) of every entry of A(z) that is non-zero for a generic z, in the row group `group`
    ('u' = the factor L, 'a' = the Darcy a-part's factor L2, 'data' = the Darcy data rows), rows relative to the group."""
    t = np.arange(Nd)
    out = []
    if system == 'elliptic':                       # unknowns u_t; rows [PDE; u; g]: alpha m u^(m-1) in row t, 1 in row Nd + t
        out += [(t, t), (t, Nd + t)]
    elif system == 'relaxed':                      # unknowns [v; w]; rows [v; w; g] of Theta, then the penalty rows (own group)
        out += [(t, t), (Nd + t, Nd + t)]
    elif system == 'burgers':                      # unknowns [v0 | v2 | v3]; rows [PDE; v2; v3; v0; g]
        out += [(t, t), (Nd + t, t), (2 * Nd + t, t), (Nd + t, Nd + t), (2 * Nd + t, 2 * Nd + t), (t, 3 * Nd + t)]
    elif system == 'eikonal':                      # unknowns [v0 | v1 | v2]; rows [v1; v2; PDE; v0; g]
        out += [(Nd + t, t), (2 * Nd + t, Nd + t), (Nd + t, 2 * Nd + t), (2 * Nd + t, 2 * Nd + t), (t, 3 * Nd + t)]
    elif system == 'semilinear':                   # unknowns [v0 | v1 | v2]; rows [v1; v2; PDE; v0; g] (include/gpk.h, GPK_GN_SEMILINEAR):
        # the PDE row (N(v0, v1, v2) - f) / eps of point t depends on all three unknowns of t -- N_u, N_p, N_q -- so v0_t enters in
        # row 2 N_d + t already, N_d rows above its unit entry
        out += [(Nd + t, t), (2 * Nd + t, Nd + t), (t, 2 * Nd + t), (Nd + t, 2 * Nd + t), (2 * Nd + t, 2 * Nd + t), (t, 3 * Nd + t)]
    elif system == 'monge_ampere':                 # unknowns [u | D u | M u]; rows [D u; M u; Delta u; u; g] (GPK_GN_MONGE_AMPERE):
        # the PDE row s = sqrt(v1^2 + v2^2 + 4 f) has the entries v1 / s, v2 / s and none for v0: Eikonal's pattern
        out += [(Nd + t, t), (2 * Nd + t, Nd + t), (Nd + t, 2 * Nd + t), (2 * Nd + t, 2 * Nd + t), (t, 3 * Nd + t)]
    elif system == 'darcy':                        # unknowns [w0 | w1 | w2 | v0 | v1 | v2]
        if group == 'a':                           # rows [w1; w2; w0]
            out += [(Nd + t, t), (2 * Nd + t, Nd + t), (t, 2 * Nd + t)]
        elif group == 'u':                         # rows [v1; v2; v3; v0; g]; v3 = the PDE row: every unknown but v0
            out += [(4 * Nd + t, t), (5 * Nd + t, Nd + t), (3 * Nd + t, 3 * Nd + t)]
            out += [(j * Nd + t, 2 * Nd + t) for j in (0, 1, 2, 4, 5)]
        elif group == 'data':                      # (v0 - data) / gamma
            out += [(3 * Nd + t, t)]
    else:
        raise ValueError(system)
    return [(np.asarray(j), np.asarray(r)) for j, r in out]


def staircase_position(system, Nd):
    """pos[j]: staircase position of unknown j (natural order); it is stored in column n_z - 1 - pos[j]."""
    nz = n_unknowns(system, Nd)
    j = np.arange(nz)
    g, t = j // Nd, j % Nd
    if system in ('elliptic', 'relaxed'):
        return j
    if system == 'burgers':                        # the three unknowns of point t interleaved
        return 3 * t + g
    if system in ('eikonal', 'semilinear', 'monge_ampere'):    # groups taken in the order v1, v2, v0
        return np.choose(g, [2, 0, 1]) * Nd + t
    if system == 'darcy':                          # groups taken in the order v1, v2, w1, w2, w0, v0
        return np.choose(g, [4, 2, 3, 5, 0, 1]) * Nd + t
    raise ValueError(system)


def column_of_unknown(system, Nd):
    return n_unknowns(system, Nd) - 1 - staircase_position(system, Nd)


def exact_first_rows(system, Nd, Nb, group='u'):
    """first row of every column (storage order, c < n_z) with an entry for a generic z; NONE: no entry in this row group"""
    nz = n_unknowns(system, Nd)
    col = column_of_unknown(system, Nd)
    fr = np.full(nz, NONE, dtype=np.int64)
    for j, r in _entries(system, Nd, Nb, group):
        np.minimum.at(fr, col[j], r)
    return fr


def envelope(fr):
    """the largest non-increasing profile that is nowhere above fr (running minimum from the left)"""
    return np.minimum.accumulate(fr)


def closed_form(n, lead, lead_div=1):
    """column c < lead zero above row (lead - 1 - c) // lead_div, columns >= lead dense (the `lead` argument of the kernels)"""
    c = np.arange(n)
    return np.where(c < lead, (lead - 1 - c) // lead_div, 0).astype(np.int64)


def promised_profile(system, Nd, Nb, variant='exact'):
    """first_row(c), c < n_z, that the layout of gpk_gn_step must promise.  variant: 'exact' (GEMM-only solve path), 'conservative'
    (Eikonal and Monge-Ampere on the substitution path: the slope-1 closed form over all columns); Darcy: 'u' or 'a' (the a-part:
    slope 1 on its columns [N_d, 4 N_d) only, 3 N_d = no entry).  The semilinear system has ONE profile on every path, the closed form
    (exact for it); Monge-Ampere's exact profile is Eikonal's two-segment one, written as such."""
    nz = n_unknowns(system, Nd)
    if system == 'darcy':
        if variant == 'a':
            fr = exact_first_rows(system, Nd, Nb, 'a')
            sub = np.arange(Nd, 4 * Nd)
            assert np.all(fr[:Nd] == NONE) and np.all(fr[4 * Nd:] == NONE)
            out = np.full(nz, 3 * Nd, dtype=np.int64)
            out[sub] = closed_form(3 * Nd, 3 * Nd)    # (equal to the exact rows there: tests/test_staircase_model.py)
            return out
        return envelope(exact_first_rows(system, Nd, Nb, 'u'))
    if system == 'semilinear' or (system in ('eikonal', 'monge_ampere') and variant == 'conservative'):
        return closed_form(nz, nz)
    if system == 'monge_ampere':
        return stair_eval(stair_encoding('eikonal', Nd), nz)
    return envelope(exact_first_rows(system, Nd, Nb))


def stair_eval(seg, ncols):
    """first_row(c), c < ncols, of the piecewise profile seg = (c1, a, b, sd): segment s covers [c1[s-1], c1[s]) with
    a[s] + (b[s] - c) // sd[s]; columns from c1[-1] on are dense"""
    c1, a, b, sd = seg
    out = np.zeros(ncols, dtype=np.int64)
    lo = 0
    for s in range(len(c1)):
        c = np.arange(lo, min(c1[s], ncols))
        out[c] = a[s] + (b[s] - c) // sd[s]
        lo = c1[s]
    return out


def stair_encoding(system, Nd):
    """the promised piecewise profiles as segments: Eikonal (exact, two slope-1 segments) and the Darcy u-part (slope 1, flat, slope 1)"""
    if system == 'eikonal':
        return ([Nd, 3 * Nd], [0, 0], [4 * Nd - 1, 3 * Nd - 1], [1, 1])
    if system == 'darcy':
        return ([2 * Nd, 4 * Nd, 6 * Nd], [0, 2 * Nd, 0], [4 * Nd - 1, 4 * Nd, 6 * Nd - 1], [1, FLAT, 1])
    raise ValueError(system)


def first_nonzero_rows(M):
    """first row with a non-zero entry of every column of M (NONE for an all-zero column)"""
    nz = M != 0
    return np.where(nz.any(axis=0), nz.argmax(axis=0), NONE).astype(np.int64)
