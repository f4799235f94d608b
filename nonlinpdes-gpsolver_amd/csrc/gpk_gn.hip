// gpk_gn.hip -- device-resident Gauss-Newton step.
//
// Reference: *.GN_method / Hessian_GN / grad_loss / loss of src/PDEs.py:82-135,278-343,418-498,137-201 and
// src/InverseProblems.py:105-186.  There, per step: H = hessian(GN_loss) by forward-over-reverse autodiff through a
// general LU solve of the triangular L, g = grad(loss) through another LU solve, delta = LU-solve(H, g), and a third
// LU solve for the new loss.  Here:
//     S  = [ L^{-1} A(z) | L^{-1} F(z) ]          one blocked TRSM, nz+1 right-hand sides       (N^2 nz flops)
//     Hb = S^T S = [[H/2, g/2], [g^T/2, loss]]    one SYRK on the MFMA units                    (N nz^2 flops)
//     chol(Hb) = [[L_H, 0], [y^T, .]], y = L_H^{-1} g/2: the forward solve of POTRS comes free   (nz^3/3 flops)
//     delta = L_H^{-T} y ;  z <- z - step * delta
// A(z) is diagonal/identity/zero blocks: it is written straight into the S buffer, never built densely
// on the host.  Several row groups with their own factor are stacked (Darcy: L_a, L_u, and the data misfit as rows
// with identity factor; relaxed elliptic: the penalty rows).
#include "gpk_common.h"

namespace {

struct Group { const double* L; int ldl; int n; int off; const double* Dinv; };

struct Dims { int nz; int rows; int ngroups; Group g[3]; };

// ---- what a Gauss-Newton system IS: one record per GPK_GN_* id, read by everything below and by gpk_mg.hip (gpk_i_gn_sharded) ----------
// A new system is described here, in one PDE-row record (Row* below, if it is of the gradient-unknown form) and nowhere else.
struct GnTraits {
    int unknowns;       // unknown groups per collocation point: n_z = unknowns * N_d (0: not a system id)
    int rows;           // rows per domain point of the group factored with L: it has rows * N_d + N_b rows.  Darcy (a second factored group,
                        // data rows) and the relaxed system (penalty rows) add their further groups by hand in gn_dims
    int grad_k;         // the gradient-unknown form with k = 2, 3 or 4 (0: another form): unknowns [v_0 | v_1 | .. | v_k], rows [v_1; ..; v_k; PDE row;
                        // v_0; g] with unit entries everywhere but in the PDE row -- written by ONE frame, gn_build_gradient_rows
    int lz_layout;      // the column layout (BuildArgs::rev) gpk_gn_step runs the system in when the leading-zero schedule is on
                        // (tune.eikonal_lz; the elliptic systems' layout 1 does not ask): 1 elliptic, 2 the gradient-unknown form with k = 2,
                        // 3 Burgers, 4 Darcy (on the GEMM-only solve path only, see step_layout), 5 the gradient-unknown form with k = 3,
                        // 6 the gradient-unknown form with k = 4
    bool v0_free_pde_row;   // v_0 does not enter the PDE row, so that the v_0 columns start N_d rows LATER, in the value row: Eikonal's exact
                        // two-segment profile (eikonal_profile) holds.  The Monge-Ampere system has exactly Eikonal's pattern and takes it.
                        // The semilinear system shares Eikonal's layout 2 but must NEVER take that profile: its v_0 columns carry N_u / eps in
                        // row 2 N_d + t, N_d rows above Eikonal's first entry, which the second segment would skip -- dropping dN/du from H
                        // with no other symptom.  Its exact profile is the closed form (column c < N_d holds v0_t, t = N_d - 1 - c, first row
                        // 2 N_d + t = n_z - 1 - c).  The semilinear system in three dimensions (layout 5, order v1, v2, v3, v0): the column at
                        // position pos holds its first non-zero in row pos -- the 1 of the rows d_k u for the gradient unknowns, N_u in the PDE
                        // row 3 N_d + t for v0_t -- so the closed form with lead = n_z is exact, as for the elliptic system.  The quasilinear
                        // system (layout 6, order v1, v2, v3, v4, v0) likewise: dG/dv0 is written in the PDE row 4 N_d + t = pos for EVERY
                        // equation kind, also where it is 0, so that its profile is the closed form and never Eikonal's two-segment one.
    bool sharded;       // gpk_mg_gn_step admits it (in its leading-zero layout)
    bool p2_reserved;   // p2 must be 0 as well where nonlin must be GPK_NL_POWER
    const char* no_reaction;    // the system has no reaction term of the GPK_NL_* family: the refusal of nonlin != GPK_NL_POWER (nullptr: it has one)
    const char* bad_eps;        // its PDE row is divided by eps = p0, checked to be finite and not 0: the refusal (nullptr: not checked)
    const char* no_structured;  // why gpk_gn_structured_prepare does not serve it (nullptr: served; gpk_gn_step then looks for the prepared forms)
    const char* no_gram;        // why gpk_gn_gram_prepare does not
    bool ql_kind = false;       // nonlin is a GPK_QL_* equation kind with the parameters p0, p1, p2 (gpk_ql_invalid), not a reaction term
};

__host__ __device__ constexpr GnTraits gn_traits(int system) {
    constexpr const char* other_nl = "gn: nonlin != GPK_NL_POWER needs GPK_GN_ELLIPTIC or GPK_GN_ELLIPTIC_RELAXED";
    switch (system) {
        case GPK_GN_ELLIPTIC: return {1, 2, 0, 1, false, true, false, nullptr, nullptr, nullptr, nullptr};
        case GPK_GN_ELLIPTIC_RELAXED:
            return {2, 2, 0, 1, false, false, false, nullptr, nullptr, "structured solve: not for the relaxed system",
                    "gram_prepare: needs W1/W2 (and v0 for the elliptic system) of gpk_gn_structured_prepare; not for the relaxed system"};
        case GPK_GN_BURGERS: return {3, 4, 0, 3, false, true, false, other_nl, nullptr, nullptr, nullptr};
        case GPK_GN_EIKONAL: return {3, 4, 2, 2, true, true, false, other_nl, nullptr, nullptr, nullptr};
        case GPK_GN_DARCY: return {6, 4, 0, 4, false, true, false, other_nl, nullptr, nullptr, nullptr};
        case GPK_GN_SEMILINEAR:
            return {3, 4, 2, 2, false, false, false, "gn: GPK_GN_SEMILINEAR takes nonlin = 0 only (its nonlinearity is gq_a1 .. gq_c3)",
                    "gn: GPK_GN_SEMILINEAR needs a finite eps (p0) other than 0",
                    "structured solve: GPK_GN_SEMILINEAR is not served (its PDE row has three z-dependent entries per point)",
                    "gram_prepare: GPK_GN_SEMILINEAR is not served (it has no structured form)"};
        case GPK_GN_MONGE_AMPERE:
            return {3, 4, 2, 2, true, false, false, "gn: GPK_GN_MONGE_AMPERE takes nonlin = 0 only", nullptr,
                    "structured solve: GPK_GN_MONGE_AMPERE is not served yet (its structured form exists: A(z) = A_1 diag(d(z)) + A_2 as for Eikonal)",
                    "gram_prepare: GPK_GN_MONGE_AMPERE is not served yet (no structured prepare)"};
        case GPK_GN_SEMILINEAR3D:
            return {4, 5, 3, 5, false, false, true,
                    "gn: GPK_GN_SEMILINEAR3D takes nonlin = 0 and p2 = 0 only (its nonlinearity is gq_a1 .. gq_c3, p0, p1, pen_lambda)", nullptr,
                    "structured solve: GPK_GN_SEMILINEAR3D is not served (its PDE row has four z-dependent entries per point)",
                    "gram_prepare: GPK_GN_SEMILINEAR3D is not served (it has no structured form)"};
        case GPK_GN_QUASILINEAR:
            return {5, 6, 4, 6, false, false, false, nullptr, nullptr,
                    "structured solve: GPK_GN_QUASILINEAR is not served (its PDE row has five z-dependent entries per point)",
                    "gram_prepare: GPK_GN_QUASILINEAR is not served (it has no structured form)", true};
        default: return {0, 0, 0, 0, false, false, false, nullptr, nullptr, nullptr, nullptr};
    }
}

int gn_dims(const gpk_gn_problem* p, Dims& d) {
    const int Nd = p->Nd, Nb = p->Nb;
    const GnTraits t = gn_traits(p->system);
    if (Nd <= 0 || Nb < 0 || t.unknowns == 0) return GPK_ERR_ARG;
    d.nz = t.unknowns * Nd; d.ngroups = 1; d.g[0] = {p->L, p->ldl, t.rows * Nd + Nb, 0, p->Dinv}; d.rows = t.rows * Nd + Nb;
    if (p->system == GPK_GN_DARCY) {                                 // the a-part with its own factor in front, the data rows behind
        if (p->Ndata < 0 || p->Ndata > Nd) return GPK_ERR_ARG;
        d.ngroups = 3;
        d.g[0] = {p->L2, p->ldl2, 3 * Nd, 0, p->Dinv2};
        d.g[1] = {p->L, p->ldl, 4 * Nd + Nb, 3 * Nd, p->Dinv};
        d.g[2] = {nullptr, 0, p->Ndata, 7 * Nd + Nb, nullptr};
        d.rows = 7 * Nd + Nb + p->Ndata;
    } else if (p->system == GPK_GN_ELLIPTIC_RELAXED) {               // the penalty rows, without a factor
        d.ngroups = 2;
        d.g[1] = {nullptr, 0, Nd, 2 * Nd + Nb, nullptr};
        d.rows = 3 * Nd + Nb;
    }
    return 0;
}

// the GEMM-only solve is available: there is a factored row group and every one comes with its inverted diagonal blocks
bool every_factor_has_dinv(const Dims& d) {
    bool any = false;
    for (int k = 0; k < d.ngroups; ++k) if (d.g[k].L) { if (!d.g[k].Dinv) return false; any = true; }
    return any;
}

struct BuildArgs {
    int system, Nd, Nb, Ndata;
    double p0, p1, lam;
    int nonlin; double p2;   // reaction term of the elliptic systems (GPK_NL_*; nl_tau / nl_dtau of gpk_common.h); GPK_GN_QUASILINEAR: its
                             // equation kind GPK_QL_* with the parameters (p0, p1, p2) (ql_G / ql_dG)
    double gq[8];            // GPK_GN_SEMILINEAR: (a1, a2, b, c1, c3) of N(u, grad u) (sl_N / sl_dN of gpk_common.h); GPK_GN_SEMILINEAR3D: (a1, a2,
                             // a3, b1, b2, b3, c1, c3) (sl3_N / sl3_dN), gathered from the doubles of gpk_gn_problem by build_args
    const double* f; const double* gb; const double* data; const double* z;
    double* S; long lds; int fcol; int write_A;
    int rev;           // leading-zero layout of gn_step: unknown j is stored in column nz-1-pos(j), and that column of A(z) is zero above
                       // row pos(j).  1: pos(j) = j (elliptic systems).  2: Eikonal, unknown groups [v0 | v1 | v2] taken in the
                       // order v1, v2, v0: their first non-zeros sit in rows t, N_d + t, 3 N_d + t >= pos (the semilinear system runs the
                       // same order; its v0 columns start in row 2 N_d + t = pos, see GnTraits::v0_free_pde_row).  3: Burgers, the three
                       // unknowns of point t (columns t, N_d + t, 2 N_d + t all start in row t) interleaved: pos(j) = 3t + group,
                       // a staircase of slope 1/3 (column zero above row pos/3; GpkLz::div = 3).  4: Darcy (round 4), unknown groups
                       // [w0 | w1 | w2 | v0 | v1 | v2] taken in the order v1, v2, w1, w2, w0, v0 -- see darcy_profiles below.  5: the semilinear
                       // system in three dimensions, unknown groups [v0 | v1 | v2 | v3] taken in the order v1, v2, v3, v0: their first
                       // non-zeros sit in rows t, N_d + t, 2 N_d + t and 3 N_d + t (N_u in the PDE row) = pos exactly.  6: the quasilinear
                       // system, unknown groups [v0 | v1 | .. | v4] taken in the order v1, .., v4, v0: first non-zeros in rows t, .., 3 N_d + t
                       // and 4 N_d + t (dG/dv0 in the PDE row) = pos exactly
    int nz;
    int family;        // elliptic system, gpk_gn_structured_prepare: 1 = only the unit entries of the first row group ([I; 0; 0], no F),
                       // 2 = only those of the second ([0; I; 0]) together with F(z); 0 = the normal [A(z) | F(z)]
};

// the layouts 2 (k = 2), 5 (k = 3) and 6 (k = 4) of the gradient-unknown form: the groups [v0 | v1 | .. | vk] taken in the order v1, .., vk, v0
// (k a compile-time constant: the remainder is then no division)
template <int k>
__host__ __device__ __forceinline__ int stair_pos_gradient(int Nd, int j) { return ((j / Nd + k) % (k + 1)) * Nd + j % Nd; }

// position of unknown j in the staircase order (see BuildArgs::rev)
__host__ __device__ __forceinline__ int stair_pos(int rev, int Nd, int j) {
    if (rev == 4) {                                                   // natural group (w0 w1 w2 v0 v1 v2) -> block of the staircase order
        const int blk = j / Nd;
        const int to = blk == 0 ? 4 : blk == 1 ? 2 : blk == 2 ? 3 : blk == 3 ? 5 : blk == 4 ? 0 : 1;
        return to * Nd + j % Nd;
    }
    if (rev == 2) return stair_pos_gradient<2>(Nd, j);
    if (rev == 5) return stair_pos_gradient<3>(Nd, j);
    if (rev == 6) return stair_pos_gradient<4>(Nd, j);
    return rev == 3 ? 3 * (j % Nd) + j / Nd : j;
}

// Darcy system, leading-zero layout (round 4).  Column c of S holds the unknown at staircase position p = n_z - 1 - c, blocks
// [v1 | v2 | w1 | w2 | w0 | v0] of N_d positions each.  First non-zero rows of A(z) (src/InverseProblems.py:127-143 of the reference):
//   u-part (rows [v1; v2; v3; v0; g], factor L_u):  v1_t: t,  v2_t: N_d + t,  w0_t, w1_t, w2_t: 2 N_d + t (the v3 row),  v0_t: 3 N_d + t
//   a-part (rows [w1; w2; w0], factor L_a):         w1_t: t,  w2_t: N_d + t,  w0_t: 2 N_d + t;  the v columns are zero there
// In column order that is, for the u-part, slope 1 over the v0 and w0 columns (c < 2 N_d: row 4 N_d - 1 - c), a flat step at 2 N_d over
// the w2, w1 columns, slope 1 again over v2, v1 (row 6 N_d - 1 - c) -- three segments of a GpkStair -- and for the a-part ONE slope-1
// staircase over the contiguous columns [N_d, 4 N_d) (row 4 N_d - 1 - c: the closed form with lead = 3 N_d on that sub-range), all
// other columns zero.  Executed flops of the solve: 27 % of the dense count; of the product: 38 %.
// Eikonal system (round 4): unknown groups in the order v1, v2, v0, i.e. columns [v0 | v2 v1] in memory.  First non-zero rows of A(z)
// (src/PDEs.py:441-449 of the reference): v1_t: t, v2_t: N_d + t, v0_t: 3 N_d + t -- slope 1 over the v2, v1 columns (row 3 N_d - 1 - c)
// and slope 1 again, N_d rows LATER, over the v0 columns (row 4 N_d - 1 - c).  Until round 3 the closed form treated the v0 columns as if
// they started at row 2 N_d + t (conservative: N_d rows of zeros were multiplied through); the two-segment profile is exact.
inline GpkStair eikonal_profile(int Nd) {
    GpkStair st;
    st.nseg = 2;
    st.c1[0] = Nd;     st.a[0] = 0; st.b[0] = 4 * Nd - 1; st.sd[0] = 1;
    st.c1[1] = 3 * Nd; st.a[1] = 0; st.b[1] = 3 * Nd - 1; st.sd[1] = 1;
    return st;
}

inline GpkStair darcy_u_profile(int Nd) {
    GpkStair st;
    st.nseg = 3;
    st.c1[0] = 2 * Nd; st.a[0] = 0;      st.b[0] = 4 * Nd - 1; st.sd[0] = 1;
    st.c1[1] = 4 * Nd; st.a[1] = 2 * Nd; st.b[1] = 4 * Nd;     st.sd[1] = 1 << 30;      // flat
    st.c1[2] = 6 * Nd; st.a[2] = 0;      st.b[2] = 6 * Nd - 1; st.sd[2] = 1;
    return st;
}

__device__ __forceinline__ void putA(const BuildArgs& a, int r, int c, double v) {
    if (a.write_A) a.S[(long)r * a.lds + (a.rev ? a.nz - 1 - stair_pos(a.rev, a.Nd, c) : c)] = v;
}
__device__ __forceinline__ void putF(const BuildArgs& a, int r, double v) { a.S[(long)r * a.lds + a.fcol] = v; }

// The ONE expression of an updated point z - t delta (alpha = -t), as the update kernels have always written it (y += alpha x): the
// update kernels below, the trial points of the line search (ZTrial) and its accepting update all go through it, so that an accepted
// iterate is bit for bit the point whose loss was measured.
__device__ __forceinline__ double gn_point(double y, double alpha, double x) { return y + alpha * x; }

// how the build reads the iterate: z itself (gn_build_kernel), or the trial point z - t_k delta formed in registers (gn_trial_build_kernel)
struct ZPlain {
    const double* z;
    __device__ __forceinline__ double operator[](int i) const { return z[i]; }
};
struct ZTrial {
    const double* z; const double* delta; double alpha;
    __device__ __forceinline__ double operator[](int i) const { return gn_point(z[i], alpha, delta[i]); }
};

// ---- the PDE row of the gradient-unknown systems at collocation point t, v = (v_0, .., v_k): one record per system with its id and k, its
// partial derivatives dR[j] = dR / dv_j (j >= 1, and j = 0 where has_v0 says that v_0 enters the row) and its value.  Where has_v0 is
// false the frame writes NO entry in the v_0 column of the row -- not a zero: under a leading-zero layout it would land above the
// two-segment profile (GnTraits::v0_free_pde_row).  Two functions, not one: the frame evaluates the partials in front of the stores of
// A and the value behind them, where they always stood, and each system's arithmetic is spelled as it always was -- the compiler fuses
// products into sums per basic block, so moving the value in front of those (conditional) stores changes its last bit.
struct RowEikonal {                                         // src/PDEs.py:420-428 (F), :441-449 (A)
    static constexpr int system = GPK_GN_EIKONAL, k = 2; static constexpr bool has_v0 = false;
    static __device__ __forceinline__ void partials(const BuildArgs& a, int, const double* v, double* dR) {
        const double eps = a.p0, v1 = v[1], v2 = v[2];
        dR[1] = 2.0 * v1 / eps; dR[2] = 2.0 * v2 / eps;
    }
    static __device__ __forceinline__ double value(const BuildArgs& a, int t, const double* v) {
        const double eps = a.p0, v1 = v[1], v2 = v[2], ft = a.f[t];
        return -(ft * ft - v1 * v1 - v2 * v2) / eps;
    }
};
struct RowSemilinear {                                      // gpk.h, GPK_GN_SEMILINEAR: the Eikonal rows, PDE row (N(v0, v1, v2) - f) / eps
    static constexpr int system = GPK_GN_SEMILINEAR, k = 2; static constexpr bool has_v0 = true;
    static __device__ __forceinline__ void partials(const BuildArgs& a, int, const double* v, double* dR) {
        const double eps = a.p0;
        double Nu, Np, Nq;
        sl_dN(a.gq, v[0], v[1], v[2], &Nu, &Np, &Nq);
        dR[0] = Nu / eps; dR[1] = Np / eps; dR[2] = Nq / eps;
    }
    static __device__ __forceinline__ double value(const BuildArgs& a, int t, const double* v) {
        const double eps = a.p0;
        return (sl_N(a.gq, v[0], v[1], v[2]) - a.f[t]) / eps;
    }
};
struct RowMongeAmpere {                                     // gpk.h, GPK_GN_MONGE_AMPERE: rows [D u; M u; Delta u; u], PDE row s = sqrt(v1^2 + v2^2 + 4 f)
    static constexpr int system = GPK_GN_MONGE_AMPERE, k = 2; static constexpr bool has_v0 = false;
    static __device__ __forceinline__ double value(const BuildArgs& a, int t, const double* v) {
        const double v1 = v[1], v2 = v[2];
        return sqrt(v1 * v1 + v2 * v2 + 4.0 * a.f[t]);      // (a negative radicand gives NaN, which the step carries like any other)
    }
    static __device__ __forceinline__ void partials(const BuildArgs& a, int t, const double* v, double* dR) {
        const double s = value(a, t, v);
        dR[1] = v[1] / s; dR[2] = v[2] / s;
    }
};
struct RowSemilinear3d {                                    // gpk.h, GPK_GN_SEMILINEAR3D: rows [d_1 u; d_2 u; d_3 u; psi[u]; u], PDE row N(v0, v1, v2, v3) - f
    static constexpr int system = GPK_GN_SEMILINEAR3D, k = 3; static constexpr bool has_v0 = true;
    static __device__ __forceinline__ void partials(const BuildArgs& a, int, const double* v, double* dR) {
        sl3_dN(a.gq, v[0], v[1], v[2], v[3], &dR[0], &dR[1], &dR[2], &dR[3]);
    }
    static __device__ __forceinline__ double value(const BuildArgs& a, int t, const double* v) {
        return sl3_N(a.gq, v[0], v[1], v[2], v[3]) - a.f[t];
    }
};

struct RowQuasilinear {                                     // gpk.h, GPK_GN_QUASILINEAR: rows [d_1 u; d_2 u; D u; M u; Delta u; u], PDE row G(x; v) of the kind a.nonlin
    static constexpr int system = GPK_GN_QUASILINEAR, k = 4; static constexpr bool has_v0 = true;
    static __device__ __forceinline__ void partials(const BuildArgs& a, int t, const double* v, double* dR) {
        const double prm[3] = {a.p0, a.p1, a.p2};
        ql_dG(a.nonlin, prm, a.f[t], v[0], v[1], v[2], v[3], v[4], dR);
    }
    static __device__ __forceinline__ double value(const BuildArgs& a, int t, const double* v) {
        const double prm[3] = {a.p0, a.p1, a.p2};
        return ql_G(a.nonlin, prm, a.f[t], v[0], v[1], v[2], v[3], v[4]);
    }
};

// The ONE frame of the gradient-unknown systems (GnTraits::grad_k = Row::k), collocation index t: unit entries and F = v_j in the rows of
// v_j, the PDE row, the unit entry and v_0 in the value row; g on the boundary.  v[] and dR[] are indexed by unrolled constants only: registers.
template <class Row, class Z>
__device__ __forceinline__ void gn_build_gradient_rows(const BuildArgs& a, const int t, const Z z) {
    constexpr int K = Row::k;
    static_assert(gn_traits(Row::system).grad_k == K && gn_traits(Row::system).v0_free_pde_row == !Row::has_v0, "the PDE row and the record of its system agree");
    const int Nd = a.Nd;
    if (t < Nd) {
        double v[K + 1], dR[K + 1];
#pragma unroll
        for (int j = 0; j <= K; ++j) v[j] = z[j * Nd + t];
        Row::partials(a, t, v, dR);
#pragma unroll
        for (int j = 1; j <= K; ++j) putA(a, (j - 1) * Nd + t, j * Nd + t, 1.0);
        if (Row::has_v0) putA(a, K * Nd + t, t, dR[0]);
#pragma unroll
        for (int j = 1; j <= K; ++j) putA(a, K * Nd + t, j * Nd + t, dR[j]);
        putA(a, (K + 1) * Nd + t, t, 1.0);
#pragma unroll
        for (int j = 1; j <= K; ++j) putF(a, (j - 1) * Nd + t, v[j]);
        putF(a, K * Nd + t, Row::value(a, t, v));
        putF(a, (K + 1) * Nd + t, v[0]);
    } else if (t < Nd + a.Nb) putF(a, (K + 2) * Nd + (t - Nd), a.gb[t - Nd]);
}

// collocation index t: writes the few non-zeros of A(z) and the entries of F(z) it owns
template <class Z>
__device__ __forceinline__ void gn_build_rows(const BuildArgs& a, const int t, const Z z) {
    const int Nd = a.Nd, Nb = a.Nb;
    if (a.system == GPK_GN_ELLIPTIC) {                      // src/PDEs.py:84-85 (F), :95-96 (A)
        if (a.family == 1) {
            if (t < Nd) putA(a, t, t, 1.0);
        } else if (t < Nd) {
            const double zi = z[t];
            if (a.nonlin == GPK_NL_POWER) {                 // the reference's equation, spelled as it always was: same bits
                const double alpha = a.p0, m = a.p1;
                if (a.family == 0) putA(a, t, t, alpha * m * pow(zi, m - 1.0));
                putF(a, t, alpha * pow(zi, m) - a.f[t]);
            } else {
                if (a.family == 0) putA(a, t, t, nl_dtau(a.nonlin, a.p0, a.p1, a.p2, zi));
                putF(a, t, nl_tau(a.nonlin, a.p0, a.p1, a.p2, zi) - a.f[t]);
            }
            putA(a, Nd + t, t, 1.0);
            putF(a, Nd + t, zi);
        } else if (t < Nd + Nb) putF(a, 2 * Nd + (t - Nd), a.gb[t - Nd]);
    } else if (a.family != 0) {
        // gpk_gn_structured_prepare, systems other than the elliptic one (round 6).  Every column of A(z) has at most ONE entry that
        // depends on z -- Burgers: the PDE row t (src/PDEs.py:297-299 of the reference); Eikonal: the row 2 N_d + t (:443-445); Darcy: the
        // v3 row of the u-part (src/InverseProblems.py:131-135) -- so A(z) = A_1 diag(d(z)) + A_2 with 0/1 patterns A_1 (family 1: those
        // entries as ones) and A_2 (family 2: the entries that are constants; Darcy's 1/gamma in the data rows included).  No F column.
        if (t >= Nd) return;
        if (a.system == GPK_GN_BURGERS) {
            if (a.family == 1) { putA(a, t, t, 1.0); putA(a, t, Nd + t, 1.0); putA(a, t, 2 * Nd + t, 1.0); }
            else { putA(a, Nd + t, Nd + t, 1.0); putA(a, 2 * Nd + t, 2 * Nd + t, 1.0); putA(a, 3 * Nd + t, t, 1.0); }
        } else if (a.system == GPK_GN_EIKONAL) {
            if (a.family == 1) { putA(a, 2 * Nd + t, Nd + t, 1.0); putA(a, 2 * Nd + t, 2 * Nd + t, 1.0); }
            else { putA(a, t, Nd + t, 1.0); putA(a, Nd + t, 2 * Nd + t, 1.0); putA(a, 3 * Nd + t, t, 1.0); }
        } else if (a.system == GPK_GN_DARCY) {
            const int U = 3 * Nd, D = 7 * Nd + Nb;
            if (a.family == 1) {
                putA(a, U + 2 * Nd + t, t, 1.0); putA(a, U + 2 * Nd + t, Nd + t, 1.0); putA(a, U + 2 * Nd + t, 2 * Nd + t, 1.0);
                putA(a, U + 2 * Nd + t, 4 * Nd + t, 1.0); putA(a, U + 2 * Nd + t, 5 * Nd + t, 1.0);
            } else {
                putA(a, t, Nd + t, 1.0); putA(a, Nd + t, 2 * Nd + t, 1.0); putA(a, 2 * Nd + t, t, 1.0);
                putA(a, U + t, 4 * Nd + t, 1.0); putA(a, U + Nd + t, 5 * Nd + t, 1.0); putA(a, U + 3 * Nd + t, 3 * Nd + t, 1.0);
                if (t < a.Ndata) putA(a, D + t, 3 * Nd + t, 1.0 / a.p0);
            }
        }
    } else if (a.system == GPK_GN_BURGERS) {                // src/PDEs.py:280-287 (F), :297-305 (A)
        const double alpha = a.p0, nu = a.p1;
        if (t < Nd) {
            const double v0 = z[t], v2 = z[Nd + t], v3 = z[2 * Nd + t];
            putA(a, t, t, -alpha * v2); putA(a, t, Nd + t, -alpha * v0); putA(a, t, 2 * Nd + t, nu);
            putA(a, Nd + t, Nd + t, 1.0); putA(a, 2 * Nd + t, 2 * Nd + t, 1.0); putA(a, 3 * Nd + t, t, 1.0);
            putF(a, t, nu * v3 + a.f[t] - alpha * v0 * v2);
            putF(a, Nd + t, v2); putF(a, 2 * Nd + t, v3); putF(a, 3 * Nd + t, v0);
        } else if (t < Nd + Nb) putF(a, 4 * Nd + (t - Nd), a.gb[t - Nd]);
    } else if (gn_traits(a.system).grad_k != 0) {           // the gradient-unknown form: one frame, the system's PDE row and its k
        if (a.system == GPK_GN_EIKONAL) gn_build_gradient_rows<RowEikonal>(a, t, z);
        else if (a.system == GPK_GN_SEMILINEAR) gn_build_gradient_rows<RowSemilinear>(a, t, z);
        else if (a.system == GPK_GN_MONGE_AMPERE) gn_build_gradient_rows<RowMongeAmpere>(a, t, z);
        else if (a.system == GPK_GN_SEMILINEAR3D) gn_build_gradient_rows<RowSemilinear3d>(a, t, z);
        else if (a.system == GPK_GN_QUASILINEAR) gn_build_gradient_rows<RowQuasilinear>(a, t, z);
    } else if (a.system == GPK_GN_DARCY) {                  // src/InverseProblems.py:106-117 (F), :127-143 (A)
        const double gam = a.p0;                            // noise_level
        const int U = 3 * Nd, D = 7 * Nd + Nb;
        if (t < Nd) {
            const double w0 = z[t], w1 = z[Nd + t], w2 = z[2 * Nd + t];
            const double v0 = z[3 * Nd + t], v1 = z[4 * Nd + t], v2 = z[5 * Nd + t];
            const double fe = a.f[t] * exp(-w0);
            putA(a, t, Nd + t, 1.0);          putF(a, t, w1);                 // a-part rows [w1; w2; w0]
            putA(a, Nd + t, 2 * Nd + t, 1.0); putF(a, Nd + t, w2);
            putA(a, 2 * Nd + t, t, 1.0);      putF(a, 2 * Nd + t, w0);
            putA(a, U + t, 4 * Nd + t, 1.0);          putF(a, U + t, v1);      // u-part rows [v1; v2; v3; v0; g]
            putA(a, U + Nd + t, 5 * Nd + t, 1.0);     putF(a, U + Nd + t, v2);
            putA(a, U + 2 * Nd + t, t, fe);
            putA(a, U + 2 * Nd + t, Nd + t, -v1);
            putA(a, U + 2 * Nd + t, 2 * Nd + t, -v2);
            putA(a, U + 2 * Nd + t, 4 * Nd + t, -w1);
            putA(a, U + 2 * Nd + t, 5 * Nd + t, -w2);
            putF(a, U + 2 * Nd + t, -v1 * w1 - v2 * w2 - fe);
            putA(a, U + 3 * Nd + t, 3 * Nd + t, 1.0); putF(a, U + 3 * Nd + t, v0);
            if (t < a.Ndata) {                                                  // (1/gamma^2) sum (v0 - data)^2 as rows
                putA(a, D + t, 3 * Nd + t, 1.0 / gam);
                putF(a, D + t, (v0 - a.data[t]) / gam);
            }
        } else if (t < Nd + Nb) putF(a, U + 4 * Nd + (t - Nd), a.gb[t - Nd]);
    } else if (a.system == GPK_GN_ELLIPTIC_RELAXED) {       // src/PDEs.py:138-147 (loss), :153-165 (GN_loss)
        const double alpha = a.p0, m = a.p1, rs = 1.0 / sqrt(a.lam);
        const int P = 2 * Nd + Nb;
        if (t < Nd) {
            const double v = z[t], w = z[Nd + t];
            putA(a, t, t, 1.0); putF(a, t, v);
            putA(a, Nd + t, Nd + t, 1.0); putF(a, Nd + t, w);
            putA(a, P + t, t, -rs);
            if (a.nonlin == GPK_NL_POWER) {
                putA(a, P + t, Nd + t, alpha * m * pow(w, m - 1.0) * rs);
                putF(a, P + t, (-v + alpha * pow(w, m) - a.f[t]) * rs);
            } else {
                putA(a, P + t, Nd + t, nl_dtau(a.nonlin, a.p0, a.p1, a.p2, w) * rs);
                putF(a, P + t, (-v + nl_tau(a.nonlin, a.p0, a.p1, a.p2, w) - a.f[t]) * rs);
            }
        } else if (t < Nd + Nb) putF(a, 2 * Nd + (t - Nd), a.gb[t - Nd]);
    }
}

// one thread per collocation index
__global__ __launch_bounds__(256) void gn_build_kernel(BuildArgs a) {
    gn_build_rows(a, blockIdx.x * 256 + threadIdx.x, ZPlain{a.z});
}

// ---- line search: the K trial measurement vectors F(z - t_k delta) in one launch -----------------------------------------------------
// W (rows x ldw, row-major) receives them as its columns k < K: the right-hand-side layout of the multi-RHS solves.  One thread per
// (collocation index, trial), the trial running fastest: the K lanes of an index share its loads of z, delta, f and write K adjacent
// doubles of a row.  No LDS, nothing but the F entries is written (write_A = 0).  The step sizes travel by value in the kernel arguments.
constexpr int LS_MAX = GPK_LS_MAX_TRIALS;
struct TrialT { double t[LS_MAX]; };

__global__ __launch_bounds__(256) void gn_trial_build_kernel(BuildArgs a, const double* __restrict__ delta, TrialT ts, int K) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const int k = (int)(idx % K);
    const long t = idx / K;
    if (t >= (long)a.Nd + a.Nb) return;
    BuildArgs b = a;
    b.fcol = k;                                                      // (putF: column k of row r)
    gn_build_rows(b, (int)t, ZTrial{a.z, delta, -ts.t[k]});
}

__global__ void axpy_kernel(int n, double alpha, const double* __restrict__ x, double* __restrict__ y) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) y[i] = gn_point(y[i], alpha, x[i]);
}

// y[j] += alpha * x[n-1-pos(j)]  (back from the staircase order of gn_step to the natural order of the unknowns)
__global__ void axpy_rev_kernel(int n, double alpha, const double* __restrict__ x, double* __restrict__ y, int rev, int Nd) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) y[i] = gn_point(y[i], alpha, x[n - 1 - stair_pos(rev, Nd, i)]);
}

// Acceptance rule of the line search ("Line search"): trials in the order given; the first k whose loss is finite
// and <= loss_in - 2 c1 t_k pred; else the k of the smallest finite loss if that is < loss_in; else -1.  A failed factorisation of H
// (d_info set: neither 0 nor the border pivot nzp1) gives -1.  One lane; K <= 16.
__global__ void ls_select_kernel(const double* __restrict__ losses, TrialT ts, int K, const double* d_loss_in, const double* d_pred,
                                 double loss_in, double pred, double c1, const int* d_info, int nzp1, int* __restrict__ d_k,
                                 double* __restrict__ d_t) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (d_loss_in) loss_in = *d_loss_in;
    if (d_pred) pred = *d_pred;
    int k = -1;
    const int info = d_info ? *d_info : 0;
    if (info == 0 || info == nzp1) {
        int best = -1;
        for (int i = 0; i < K; ++i) {
            const double l = losses[i];
            if (!isfinite(l)) continue;
            if (l <= loss_in - 2.0 * c1 * ts.t[i] * pred) { k = i; break; }
            if (best < 0 || l < losses[best]) best = i;
        }
        if (k < 0 && best >= 0 && losses[best] < loss_in) k = best;
    }
    *d_k = k;
    *d_t = k >= 0 ? ts.t[k] : 0.0;
}

// z <- z - t_k delta for the accepted k (device scalar; -1: z is not touched), delta in the natural order of the unknowns
__global__ void ls_update_kernel(int n, const int* __restrict__ d_k, TrialT ts, const double* __restrict__ delta, double* __restrict__ z) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int k = *d_k;
    if (k < 0 || i >= n) return;
    z[i] = gn_point(z[i], -ts.t[k], delta[i]);
}

__global__ void reverse_copy_kernel(int n, const double* __restrict__ x, double* __restrict__ y, int rev, int Nd) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) y[i] = x[n - 1 - stair_pos(rev, Nd, i)];
}

__global__ void scale_kernel(int n, double alpha, double* __restrict__ x) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) x[i] *= alpha;
}

BuildArgs build_args(const gpk_gn_problem* p, const double* z, double* S, long lds, int fcol, int write_A, int rev, int family) {
    BuildArgs a;
    a.rev = rev; a.nz = fcol; a.family = family;
    a.system = p->system; a.Nd = p->Nd; a.Nb = p->Nb; a.Ndata = p->Ndata;
    a.p0 = p->p0; a.p1 = p->p1; a.lam = p->pen_lambda;
    a.nonlin = p->nonlin; a.p2 = p->p2;
    a.gq[0] = p->gq_a1; a.gq[1] = p->gq_a2; a.gq[2] = p->gq_b; a.gq[3] = p->gq_c1; a.gq[4] = p->gq_c3; a.gq[5] = a.gq[6] = a.gq[7] = 0.0;
    if (p->system == GPK_GN_SEMILINEAR3D) {                          // (a1, a2, a3) = (gq_a1, gq_a2, p0), (b1, b2, b3) = (gq_b, p1, pen_lambda)
        const double c[8] = {p->gq_a1, p->gq_a2, p->p0, p->gq_b, p->p1, p->pen_lambda, p->gq_c1, p->gq_c3};
        for (int k = 0; k < 8; ++k) a.gq[k] = c[k];
    }
    a.f = p->rhs_f; a.gb = p->bdy_g; a.data = p->data_u; a.z = z;
    a.S = S; a.lds = lds; a.fcol = fcol; a.write_A = write_A;
    return a;
}

int build(gpk_handle h, const gpk_gn_problem* p, const double* z, double* S, long lds, int fcol, int write_A, int rev = 0, int family = 0) {
    const BuildArgs a = build_args(p, z, S, lds, fcol, write_A, rev, family);
    gn_build_kernel<<<gpk_ceil_div(p->Nd + p->Nb, 256), 256, 0, h->stream>>>(a);
    GPK_LAUNCH_CHECK(h);
    return 0;
}

// the reaction term is one of the family, and only the systems whose record says so have one; a PDE row divided by eps needs a usable eps
int check_nonlin(gpk_handle h, const gpk_gn_problem* p) {
    if (gn_traits(p->system).ql_kind) {                              // nonlin is the equation kind, read as such for this system only
        const char* bad = gpk_ql_invalid(p->nonlin, p->p0, p->p1, p->p2);
        return bad ? gpk_bad_arg(h, bad) : 0;
    }
    if (!gpk_nl_valid(p->nonlin)) return gpk_bad_arg(h, "gn: nonlin is not one of GPK_NL_POWER .. GPK_NL_CUBIC");
    const GnTraits t = gn_traits(p->system);
    if (t.no_reaction && (p->nonlin != GPK_NL_POWER || (t.p2_reserved && p->p2 != 0.0))) return gpk_bad_arg(h, t.no_reaction);
    if (t.bad_eps && !(std::isfinite(p->p0) && p->p0 != 0.0)) return gpk_bad_arg(h, t.bad_eps);
    return 0;
}

int check_prob(gpk_handle h, const gpk_gn_problem* p, Dims& d) {
    if (!p) return gpk_bad_arg(h, "gn: null problem");
    if (gn_dims(p, d) != 0) return gpk_bad_arg(h, "gn: system id / sizes");
    GPK_TRY(check_nonlin(h, p));
    if (!p->rhs_f || (p->Nb > 0 && !p->bdy_g) || !p->L) return gpk_bad_arg(h, "gn: null rhs_f/bdy_g/L");
    if (p->system == GPK_GN_DARCY && (!p->L2 || (p->Ndata > 0 && !p->data_u))) return gpk_bad_arg(h, "gn: Darcy needs L2 and data_u");
    return 0;
}


// loss(z) = sum_k || L_k^{-1} F_k(z) ||^2 (+ the rows without a factor) by true substitution, one vector, on h->stream: `work` (rows
// doubles) receives F(z) and then the solved vector, d_out (device) the scalar.  gpk_gn_loss; the exact in-step loss of gpk_gn_step.
int substitution_loss(gpk_handle h, const gpk_gn_problem* p, const Dims& d, const double* z, double* work, double* d_out) {
    GPK_HIP(h, hipMemsetAsync(work, 0, (size_t)d.rows * sizeof(double), h->stream));
    GPK_TRY(build(h, p, z, work, 1, 0, 0));
    for (int k = 0; k < d.ngroups; ++k)
        if (d.g[k].L) GPK_TRY(gpk_i_trsv(h, false, d.g[k].L, d.g[k].n, d.g[k].ldl, work + d.g[k].off));
    return gpk_i_dot(h, work, work, d.rows, d_out);
}

// the exact in-step loss of gpk_gn_step / gpk_mg_gn_step (gpk_tune key 52): the same on the handle's own scratch vector, -> d_scalars[8]
int loss_work_reserve(gpk_handle h, const Dims& d) {
    if (h->loss_work_cap >= (size_t)d.rows) return 0;
    if (h->d_loss_work) {
        GPK_HIP(h, hipStreamSynchronize(h->stream));
        if (h->pipe_g) GPK_HIP(h, hipStreamSynchronize(h->pipe_g));
        (void)hipFree(h->d_loss_work); h->d_loss_work = nullptr; h->loss_work_cap = 0;
    }
    GPK_HIP(h, hipMalloc((void**)&h->d_loss_work, (size_t)d.rows * sizeof(double)));
    h->loss_work_cap = (size_t)d.rows;
    return 0;
}

int exact_loss(gpk_handle h, const gpk_gn_problem* p, const Dims& d, const double* z) {
    GPK_TRY(loss_work_reserve(h, d));
    return substitution_loss(h, p, d, z, h->d_loss_work, h->d_scalars + 8);
}

// The same in two halves (gpk_tune key 52 = 1): F(z) is written at the START of the step on the main stream (z is overwritten at its end);
// the chain -- one single-vector solve per factor, then the dot product -- is issued LATE, on the GEMM partition's stream: behind that
// stream's last product of the pipelined phase, or (after_main != 0: no pipelined phase) behind an event of the main stream, so that it
// runs next to the last panel chain (other partition) and the backward solve of the tail (main stream), not next to GEMM launches.
int exact_loss_build(gpk_handle h, const gpk_gn_problem* p, const Dims& d, const double* z) {
    GPK_TRY(loss_work_reserve(h, d));
    for (int i = 0; i < 2; ++i) if (!h->ev_loss[i]) GPK_HIP(h, hipEventCreateWithFlags(&h->ev_loss[i], hipEventDisableTiming));
    GPK_HIP(h, hipMemsetAsync(h->d_loss_work, 0, (size_t)d.rows * sizeof(double), h->stream));
    GPK_TRY(build(h, p, z, h->d_loss_work, 1, 0, 0));
    GPK_HIP(h, hipEventRecord(h->ev_loss[0], h->stream));            // F(z) is written
    return 0;
}

// after_main: the phase before the tail ran on the main stream (no two-partition pipeline): the chain waits for it; otherwise it only waits
// for F(z) and queues behind the GEMM partition's own last launch of the pipelined phase
int exact_loss_chain(gpk_handle h, const Dims& d, bool after_main, bool* on_side) {
    const hipStream_t main_s = h->stream, side = h->pipe_g;
    *on_side = false;
    if (!side || h->pipe_unavailable) {
        // the side stream went away between the decision at the start of the step and here (the pipelined phase re-created its streams and
        // failed: gpk_i_syrk_potrf, gpk_tune key 13): F(z) is in d_loss_work already, finish on the main stream -- never on the NULL stream
        for (int k = 0; k < d.ngroups; ++k)
            if (d.g[k].L) GPK_TRY(gpk_i_trsv(h, false, d.g[k].L, d.g[k].n, d.g[k].ldl, h->d_loss_work + d.g[k].off));
        return gpk_i_dot(h, h->d_loss_work, h->d_loss_work, d.rows, h->d_scalars + 8);
    }
    *on_side = true;
    if (after_main) GPK_HIP(h, hipEventRecord(h->ev_loss[0], main_s));
    GPK_HIP(h, hipStreamWaitEvent(side, h->ev_loss[0], 0));
    int rc = 0;
    {
        GpkStreamScope scope(h);                                     // (single-vector solves and a dot product: no use for the GEMM workspace)
        scope.use(side, false);
        h->trsv_alt = 1;
        for (int k = 0; k < d.ngroups && rc == 0; ++k)
            if (d.g[k].L) rc = gpk_i_trsv(h, false, d.g[k].L, d.g[k].n, d.g[k].ldl, h->d_loss_work + d.g[k].off);
        if (rc == 0) rc = gpk_i_dot(h, h->d_loss_work, h->d_loss_work, d.rows, h->d_scalars + 8);
        h->trsv_alt = 0;
    }
    if (rc) { (void)hipStreamSynchronize(side); return rc; }
    GPK_HIP(h, hipEventRecord(h->ev_loss[1], side));
    return 0;
}

// The column layout gpk_gn_step runs a system in (BuildArgs::rev): GnTraits::lz_layout -- the elliptic systems' layout 1 always, the
// others when the leading-zero schedule is on, Darcy's layout 4 on the GEMM-only solve path only -- or 0 = dense schedule.
int step_layout(gpk_handle h, const gpk_gn_problem* p) {
    const int lz = gn_traits(p->system).lz_layout;
    if (lz == 1) return 1;
    if (!h->tune.eikonal_lz) return 0;
    if (lz == 4 && !(h->tune.use_dinv && p->Dinv && p->Dinv2 && p->dinv_block > 0)) return 0;
    return lz;
}

// The leading-zero profile of [A(z) | F] under that layout, a pure function of the problem and the handle's switches: the closed form
// with lead = n_z (slope 1/3 for Burgers); for Eikonal on the GEMM-only solve path the exact two-segment profile for the solve and the
// products (the substitution path keeps the conservative closed form).  Dense for the layouts 0 and 4: Darcy's two factors have a
// profile each (darcy_u_profile; the a-part's closed form on its own columns), passed where they are used.
// Which systems of layout 2 may take the two-segment profile, and why the others must not: GnTraits::v0_free_pde_row.
GpkLz step_profile(gpk_handle h, const gpk_gn_problem* p, int nz, int rev) {
    if (rev == 2 && gn_traits(p->system).v0_free_pde_row && h->tune.use_dinv && p->Dinv && p->dinv_block > 0 && h->tune.eikonal_lz != 2) return GpkLz::piecewise(eikonal_profile(p->Nd));
    return ((rev >= 1 && rev <= 3) || rev == 5 || rev == 6) ? GpkLz::closed(nz, rev == 3 ? 3 : 1) : GpkLz();
}

// the GEMM-only solve path is available and switched on, with the block size given (the structured modes of the other systems need it)
bool all_dinv(gpk_handle h, const gpk_gn_problem* p, const Dims& d) {
    return h->tune.use_dinv && p->dinv_block > 0 && every_factor_has_dinv(d);
}

#define GPK_PROF_MARK(h, i) do { if ((h)->prof) { (h)->prof_phase = (i); GPK_HIP((h), hipEventRecord((h)->pev[i], (h)->stream)); } } while (0)

// S <- [L^{-1}A | L^{-1}F], Hb <- alpha * S^T S (lower triangle, bordered).
// rev != 0 (elliptic system only): unknown j is stored in column nz-1-j; column c < nz of [A | F] is then zero above row
// nz-1-c, which the solve and the SYRK exploit (about a third of the TRSM flops and a quarter of the SYRK flops).
// With the inverses of the diagonal blocks of every factor at hand (gpk_trtri_diag, gpk_gn_problem::Dinv) the solve runs
// out of place into the handle's workspace W (all-GEMM, see gpk_i_trsm_left_dinv) and the SYRK reads W; S is scratch then.
int assemble_normal_equations(gpk_handle h, const gpk_gn_problem* p, const Dims& d, const double* z, double* S, int lds,
                              double* Hb, int ldh, double alpha, int rev, double** Wout = nullptr, int family = 0) {
    const int nc = d.nz + 1;
    if (lds < nc || ldh < nc) return gpk_bad_arg(h, "gn: lds/ldh < nz+1");
    const GpkLz lz = step_profile(h, p, d.nz, rev);
    const bool dinv = h->tune.use_dinv && every_factor_has_dinv(d);
    const int db = p->dinv_block > 0 ? p->dinv_block : 256;
    if (!dinv_block_ok(db)) return gpk_bad_arg(h, "gn: dinv_block must be 256, 512, 1024 or 2048");
    double* W = S;
    if (dinv) {
        GPK_TRY(gpk_i_workspace(h, (size_t)d.rows * lds * sizeof(double), &W));
        // the solve never writes W left of the leading-zero boundary (rev) -- zero it unless the previous solve into W had
        // exactly this shape, in which case those zeros are still there
        // (the signature carries the inverted-block size -- the never-written region depends on it -- and is dropped again if the
        // solve below fails to be issued, so that a later step never trusts zeros this one did not leave behind)
        const long sig[5] = {d.rows, lds, nc, rev ? d.nz : 0, (long)(p->system + 1) * 4096 + db};
        if (memcmp(sig, h->work_sig, sizeof sig) != 0) {
            h->work_sig[0] = -1;
            GPK_HIP(h, hipMemsetAsync(W, 0, (size_t)d.rows * lds * sizeof(double), h->stream));
            memcpy(h->work_sig, sig, sizeof sig);
        }
    }
    struct SigGuard {                                                // any early return below invalidates the cached zero region
        gpk_handle h; bool armed; ~SigGuard() { if (armed) h->work_sig[0] = -1; }
    } sig_guard{h, dinv};
    GPK_PROF_MARK(h, 0);
    // (Darcy with the cached a-part: of the a-part rows of S only the F column is read -- build writes it for every row -- so those
    // 3 N_d rows, a third of the buffer, need not be cleared; the A entries build drops there are never looked at)
    const long skip = (rev == 4 && dinv && family == 0 && p->Wa && p->Ha) ? d.g[0].n : 0;
    GPK_HIP(h, hipMemsetAsync(S + skip * lds, 0, (size_t)(d.rows - skip) * lds * sizeof(double), h->stream));
    GPK_TRY(build(h, p, z, S, lds, d.nz, 1, rev, family));
    for (int k = 0; k < d.ngroups; ++k) {
        const Group& g = d.g[k];
        double* Sg = S + (long)g.off * lds;
        if (!g.L) {                                                  // identity factor (data misfit / penalty rows)
            if (dinv && g.n > 0)
                GPK_HIP(h, hipMemcpy2DAsync(W + (long)g.off * lds, (size_t)lds * 8, Sg, (size_t)lds * 8, (size_t)nc * 8, g.n,
                                            hipMemcpyDeviceToDevice, h->stream));
        } else if (dinv && rev == 4) {
            double* Wg = W + (long)g.off * lds;
            const int Nd = p->Nd;
            if (k == 0) {
                // a-part: only the columns [N_d, 4 N_d) are non-zero, a slope-1 staircase of their own (closed form on the sub-range),
                // and the dense F column as a one-column solve; the v columns of these rows stay zero in W.
                // The 3 N_d columns do not depend on z (a permutation matrix against a fixed factor): with the result of
                // gpk_gn_darcy_prepare at hand (p->Wa) that solve is not repeated -- the product below reads p->Wa / p->Ha instead
                if (!(p->Wa && p->Ha))
                    GPK_TRY(gpk_i_trsm_left_dinv(h, g.L, g.Dinv, db, g.n, g.ldl, Sg + Nd, lds, Wg + Nd, lds, 3 * Nd, GpkLz::closed(3 * Nd)));
                GPK_TRY(gpk_i_trsm_left_dinv(h, g.L, g.Dinv, db, g.n, g.ldl, Sg + d.nz, lds, Wg + d.nz, lds, 1, GpkLz()));
            } else {                                                 // u-part: three segments
                GPK_TRY(gpk_i_trsm_left_dinv(h, g.L, g.Dinv, db, g.n, g.ldl, Sg, lds, Wg, lds, nc, GpkLz::piecewise(darcy_u_profile(Nd))));
            }
        } else if (dinv) {
            GPK_TRY(gpk_i_trsm_left_dinv(h, g.L, g.Dinv, db, g.n, g.ldl, Sg, lds, W + (long)g.off * lds, lds, nc, lz));
        } else if (rev) {
            GPK_TRY(gpk_i_trsm_left_lz(h, g.L, g.n, g.ldl, Sg, nc, lds, lz));
        } else {
            GPK_TRY(gpk_i_trsm_left_mt(h, false, g.L, g.n, g.ldl, Sg, nc, lds));
        }
    }
    GPK_PROF_MARK(h, 1);
    sig_guard.armed = false;                                         // the solve was issued completely
    if (Wout) { *Wout = W; return 0; }                               // gn_step: product and factorisation are pipelined by the caller
    GPK_TRY(gpk_i_gemm(h, true, false, nc, nc, d.rows, alpha, W, lds, W, lds, 0.0, Hb, ldh, true, lz));
    GPK_PROF_MARK(h, 2);
    return 0;
}

// ---- structured solve of the elliptic system (optional, gpk_gn_structured_prepare) -------------------------------------------
// per-column coefficients in the internal (reversed) column order: column c holds unknown u = nz-1-c
// dcol = tau'(z), acol = tau(z) - tau(0): v0 = L^{-1}F(0) of gpk_gn_structured_prepare already carries tau(0) (p0 for GPK_NL_EXP, 0 for
// every other kind; the power law keeps its own expression, to the bit)
__global__ void structured_coeff_kernel(int nz, int nonlin, double p0, double p1, double p2, const double* __restrict__ z,
                                        double* __restrict__ dcol, double* __restrict__ acol, double* __restrict__ zcol) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= nz) return;
    const double zi = z[nz - 1 - c];
    if (nonlin == GPK_NL_POWER) {
        const double alpha = p0, m = p1;
        dcol[c] = alpha * m * pow(zi, m - 1.0);
        acol[c] = alpha * pow(zi, m);
    } else {
        dcol[c] = nl_dtau(nonlin, p0, p1, p2, zi);
        acol[c] = nonlin == GPK_NL_EXP ? p0 * expm1(p1 * zi) : nl_tau(nonlin, p0, p1, p2, zi) - nl_tau(nonlin, p0, p1, p2, 0.0);
    }
    zcol[c] = zi;
}

// one workgroup per row r: S[r][c] = d[c] W1[r][c] + W2[r][c] (c < nz), S[r][nz] = v0[r] + sum_c (a[c] W1[r][c] + z[c] W2[r][c]).
// Columns left of the leading-zero boundary (c < nz-1-r) are zero in W1, W2 and are written as zeros.
__global__ __launch_bounds__(256) void structured_form_kernel(int nz, const double* __restrict__ W1, const double* __restrict__ W2, long ldw,
                                                              const double* __restrict__ v0, const double* __restrict__ dcol,
                                                              const double* __restrict__ acol, const double* __restrict__ zcol,
                                                              double* __restrict__ S, long lds) {
    __shared__ double red[4];
    const long r = blockIdx.x;
    const double* w1 = W1 + r * ldw;
    const double* w2 = W2 + r * ldw;
    double* s = S + r * lds;
    const int cz = (int)max(0L, (long)nz - 1 - r) & ~1;             // first column that can be non-zero (even: 16-byte pairs)
    double acc = 0.0;
    for (int c = 2 * (int)threadIdx.x; c < nz; c += 512) {
        if (c + 1 < cz) { s[c] = 0.0; s[c + 1] = 0.0; continue; }
        const double a0 = w1[c], b0 = w2[c];
        s[c] = fma(dcol[c], a0, b0);
        acc = fma(acol[c], a0, fma(zcol[c], b0, acc));
        if (c + 1 < nz) {
            const double a1 = w1[c + 1], b1 = w2[c + 1];
            s[c + 1] = fma(dcol[c + 1], a1, b1);
            acc = fma(acol[c + 1], a1, fma(zcol[c + 1], b1, acc));
        }
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) s[nz] = v0[r] + ((red[0] + red[1]) + (red[2] + red[3]));
}

// w[r] = v0[r] + sum_c (a[c] W1[r][c] + z[c] W2[r][c]) = (L^{-1}F(z))[r]: the Gram level's loss ||w||^2 is taken from w itself -- as
// the quadratic form v0^T v0 + ... of terms of size 1e16 it keeps three digits near convergence (loss 1e4)
__global__ __launch_bounds__(256) void structured_w_kernel(int nz, const double* __restrict__ W1, const double* __restrict__ W2, long ldw,
                                                           const double* __restrict__ v0, const double* __restrict__ acol,
                                                           const double* __restrict__ zcol, double* __restrict__ w) {
    __shared__ double red[4];
    const long r = blockIdx.x;
    const double* w1 = W1 + r * ldw;
    const double* w2 = W2 + r * ldw;
    const int cz = (int)max(0L, (long)nz - 1 - r);                   // W1, W2 are zero left of this column
    double acc = 0.0;
    for (int c = cz + (int)threadIdx.x; c < nz; c += 256) acc = fma(acol[c], w1[c], fma(zcol[c], w2[c], acc));
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) w[r] = v0[r] + ((red[0] + red[1]) + (red[2] + red[3]));
}

// Structured solve of the other systems (round 6): d(z) per column, in the step's internal column order (column c holds the unknown at
// staircase position nz-1-c).  The z-dependent entry of unknown j's column (see gn_build_kernel, family 1):
//   Burgers  (src/PDEs.py:297-299):            v0_t: -alpha v2_t    v2_t: -alpha v0_t    v3_t: nu
//   Eikonal  (src/PDEs.py:443-445):            v0_t: 0              v1_t: 2 v1_t / eps   v2_t: 2 v2_t / eps
//   Darcy    (src/InverseProblems.py:131-135): w0_t: f_t exp(-w0_t) w1_t: -v1_t  w2_t: -v2_t  v0_t: 0  v1_t: -w1_t  v2_t: -w2_t
__global__ void structured_coeff_general_kernel(int system, int Nd, int nz, int rev, double p0, double p1, const double* __restrict__ f,
                                                const double* __restrict__ z, double* __restrict__ dcol) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= nz) return;
    const int blk = j / Nd, t = j - blk * Nd;
    double v = 0.0;
    if (system == GPK_GN_BURGERS) v = blk == 0 ? -p0 * z[Nd + t] : blk == 1 ? -p0 * z[t] : p1;
    else if (system == GPK_GN_EIKONAL) v = blk == 0 ? 0.0 : 2.0 * z[j] / p0;
    else if (system == GPK_GN_DARCY)
        v = blk == 0 ? f[t] * exp(-z[t]) : blk == 1 ? -z[4 * Nd + t] : blk == 2 ? -z[5 * Nd + t] : blk == 3 ? 0.0 : blk == 4 ? -z[Nd + t] : -z[2 * Nd + t];
    dcol[nz - 1 - stair_pos(rev, Nd, j)] = v;
}

// one workgroup per row r: W[r][c] = d[c] W1[r][c] + W2[r][c] for c < nz (16-byte pairs: ldw, lds even; nz may be odd).  The F column is
// not touched (solved separately, one column, by the caller).  Above the staircase W1 and W2 hold zeros and zeros are written.
__global__ __launch_bounds__(256) void structured_form_general_kernel(int nz, const double* __restrict__ W1, const double* __restrict__ W2, long ldw,
                                                                      const double* __restrict__ dcol, double* __restrict__ W, long lds) {
    typedef double d2 __attribute__((ext_vector_type(2)));
    const long r = blockIdx.x;
    const double* w1 = W1 + r * ldw;
    const double* w2 = W2 + r * ldw;
    double* w = W + r * lds;
    for (int c = 2 * (int)threadIdx.x; c < nz; c += 512) {
        if (c + 1 < nz) {
            const d2 a = *reinterpret_cast<const d2*>(w1 + c), b = *reinterpret_cast<const d2*>(w2 + c);
            const d2 d = *reinterpret_cast<const d2*>(dcol + c);
            *reinterpret_cast<d2*>(w + c) = (d2){fma(d.x, a.x, b.x), fma(d.y, a.y, b.y)};
        } else w[c] = fma(dcol[c], w1[c], w2[c]);
    }
}

// C[i][j] += A[i][j] for j <= i (one workgroup per row): the cached a-part contribution of the Darcy step (gpk_gn_darcy_prepare)
__global__ __launch_bounds__(256) void add_lower_kernel(int n, const double* __restrict__ A, long lda, double* __restrict__ Cm, long ldc) {
    const long i = blockIdx.x;
    const double* a = A + i * lda;
    double* c = Cm + i * ldc;
    for (int j = threadIdx.x; j <= (int)i; j += 256) c[j] += a[j];
}

__global__ void sub_kernel(long n, const double* __restrict__ a, const double* __restrict__ b, double* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = a[i] - b[i];
}

// ---- second level: the bordered matrix straight from the Gram blocks of W (optional, gpk_gn_gram_prepare) -----------------------
// one workgroup per column index c (a row of the four blocks): q1[c] = G11[c,:] a + G12[c,:] z + p1[c], q2[c] = G21[c,:] a + G22[c,:] z + p2[c]
__global__ __launch_bounds__(256) void gram_gemv_kernel(int nz, const double* __restrict__ G, long ldg, const double* __restrict__ pvec,
                                                        const double* __restrict__ acol, const double* __restrict__ zcol,
                                                        double* __restrict__ q) {
    __shared__ double red[2][4];
    const long c = blockIdx.x;
    const double* g11 = G + c * ldg;
    const double* g12 = G + ((long)nz + c) * ldg;
    const double* g21 = G + (2L * nz + c) * ldg;
    const double* g22 = G + (3L * nz + c) * ldg;
    double s1 = 0.0, s2 = 0.0;
    for (int k = threadIdx.x; k < nz; k += 256) {
        const double a = acol[k], z = zcol[k];
        s1 = fma(g11[k], a, fma(g12[k], z, s1));
        s2 = fma(g21[k], a, fma(g22[k], z, s2));
    }
    for (int off = 32; off > 0; off >>= 1) { s1 += __shfl_down(s1, off, 64); s2 += __shfl_down(s2, off, 64); }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = s1; red[1][threadIdx.x >> 6] = s2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        q[c] = pvec[c] + ((red[0][0] + red[0][1]) + (red[0][2] + red[0][3]));
        q[nz + c] = pvec[nz + c] + ((red[1][0] + red[1][1]) + (red[1][2] + red[1][3]));
    }
}

// Hb[c][c'] (c' <= c) = d_c G11 d_c' + d_c G12 + G21 d_c' + G22; border row Hb[nz][c] = d_c q1[c] + q2[c]; one workgroup per row
__global__ __launch_bounds__(256) void gram_form_kernel(int nz, const double* __restrict__ G, long ldg, const double* __restrict__ dcol,
                                                        const double* __restrict__ q, double* __restrict__ Hb, long ldh) {
    const long c = blockIdx.x;
    if (c == nz) {
        for (int k = threadIdx.x; k < nz; k += 256) Hb[(long)nz * ldh + k] = fma(dcol[k], q[k], q[nz + k]);
        return;
    }
    const double* g11 = G + c * ldg;
    const double* g12 = G + ((long)nz + c) * ldg;
    const double* g21 = G + (2L * nz + c) * ldg;
    const double* g22 = G + (3L * nz + c) * ldg;
    const double dc = dcol[c];
    double* hrow = Hb + c * ldh;
    for (int k = threadIdx.x; k <= c; k += 256) {
        const double dk = dcol[k];
        hrow[k] = fma(dc, fma(g11[k], dk, g12[k]), fma(g21[k], dk, g22[k]));
    }
}

// loss = pvec[2nz] + a.p1 + z.p2 + a.q1 + z.q2 -> Hb[nz][nz] and d_loss
__global__ __launch_bounds__(1024) void gram_loss_kernel(int nz, const double* __restrict__ pvec, const double* __restrict__ acol,
                                                         const double* __restrict__ zcol, const double* __restrict__ q,
                                                         double* __restrict__ corner, double* __restrict__ d_loss) {
    __shared__ double red[16];
    double s = 0.0;
    for (int k = threadIdx.x; k < nz; k += 1024) s += acol[k] * (pvec[k] + q[k]) + zcol[k] * (pvec[nz + k] + q[nz + k]);
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < 16; ++i) t += red[i];
        t += pvec[2 * nz];
        *corner = t; *d_loss = t;
    }
}

// ---- the five ways gpk_gn_step runs a step, and what follows the mode (None: the Gram modes factor Hb themselves) ----------------
enum class StepMode { Plain, StructuredElliptic, GramElliptic, StructuredGeneral, GramGeneral };
enum class StepProduct { None, SyrkPotrf, Darcy };

// No side effects.  A mode is chosen only when everything it reads has been prepared; an incomplete preparation falls through to the
// next line and in the end to Plain.  (The elliptic system has layout 1, and its relaxed form is a system of its own: always Plain.)
StepMode select_mode(gpk_handle h, const gpk_gn_problem* p, const Dims& d, int rev) {
    if (!h->tune.structured || gn_traits(p->system).no_structured) return StepMode::Plain;   // (no structured form served)
    const bool ops = p->W1 && p->W2 && p->ldw >= d.nz + 1;           // gpk_gn_structured_prepare
    const bool gram = p->G && p->ldg >= d.nz;                        // gpk_gn_gram_prepare
    if (p->system == GPK_GN_ELLIPTIC && ops && p->v0) return gram && p->pvec ? StepMode::GramElliptic : StepMode::StructuredElliptic;
    if (rev >= 2 && ops && all_dinv(h, p, d)) return gram ? StepMode::GramGeneral : StepMode::StructuredGeneral;
    return StepMode::Plain;
}
StepProduct select_product(StepMode m, int rev) {
    return (m == StepMode::GramElliptic || m == StepMode::GramGeneral) ? StepProduct::None : rev == 4 ? StepProduct::Darcy : StepProduct::SyrkPotrf;
}

// what a mode hands back: the solved block [L^{-1}A | L^{-1}F] (not the Gram modes), exact loss started, its chain still to be issued
struct ModeOut { double* W = nullptr; bool exact = false, exact_late = false; };

// the loss of the iterate the step starts from by substitution (gpk_tune key 52): late on the side stream if allowed and there is one, else at once
int start_exact_loss(gpk_handle h, const gpk_gn_problem* p, const Dims& d, const double* z, bool allow_late, bool* exact, bool* exact_late) {
    if (!h->tune.exact_loss) return 0;
    *exact = true;
    *exact_late = h->tune.exact_loss == 1 && allow_late && h->pipe_g && !h->pipe_unavailable;
    return *exact_late ? exact_loss_build(h, p, d, z) : exact_loss(h, p, d, z);
}

// w = L^{-1}F(z) from the F column of S (every row has an entry) -> dst[row * dst_stride]: one single-column solve per factor, other rows copied
int solve_f_column(gpk_handle h, const gpk_gn_problem* p, const Dims& d, double* S, int lds, double* dst, int dst_stride) {
    for (int k = 0; k < d.ngroups; ++k) {
        const Group& g = d.g[k];
        if (g.n <= 0) continue;
        double* src = S + (long)g.off * lds + d.nz;
        double* out = dst + (long)g.off * dst_stride;
        if (g.L) GPK_TRY(gpk_i_trsm_left_dinv(h, g.L, g.Dinv, p->dinv_block, g.n, g.ldl, src, lds, out, dst_stride, 1, GpkLz()));
        else GPK_HIP(h, hipMemcpy2DAsync(out, (size_t)dst_stride * 8, src, (size_t)lds * 8, 8, g.n, hipMemcpyDeviceToDevice, h->stream));
    }
    return 0;
}

int mode_plain(gpk_handle h, const gpk_gn_problem* p, const Dims& d, double* z, double* S, int lds, double* Hb, int ldh, int rev, ModeOut& o) {
    GPK_TRY(start_exact_loss(h, p, d, z, true, &o.exact, &o.exact_late));     // in front of the solve
    return assemble_normal_equations(h, p, d, z, S, lds, Hb, ldh, 1.0, rev, &o.W);
}

// gpk_gn_structured_prepare, elliptic system: one memory-bound pass over W1, W2 instead of the triangular solve
int mode_structured_elliptic(gpk_handle h, const gpk_gn_problem* p, const Dims& d, double* z, double* S, int lds, double*, int, int, ModeOut& o) {
    const int nz = d.nz;
    GPK_PROF_MARK(h, 0);
    double* coef = S;                                                // 3 nz doubles of scratch (S is free in this mode)
    GPK_TRY(gpk_i_workspace(h, (size_t)d.rows * lds * sizeof(double), &o.W));
    h->work_sig[0] = -1;                                             // (the workspace no longer holds a solve of a known shape)
    structured_coeff_kernel<<<gpk_ceil_div(nz, 256), 256, 0, h->stream>>>(nz, p->nonlin, p->p0, p->p1, p->p2, z, coef, coef + nz, coef + 2 * nz);
    structured_form_kernel<<<d.rows, 256, 0, h->stream>>>(nz, p->W1, p->W2, p->ldw, p->v0, coef, coef + nz, coef + 2 * nz, o.W, lds);
    GPK_LAUNCH_CHECK(h);
    GPK_TRY(start_exact_loss(h, p, d, z, false, &o.exact, &o.exact_late));    // reported loss: true substitution (round 6), as in the plain mode
    GPK_PROF_MARK(h, 1);
    return 0;
}

// gpk_gn_gram_prepare, elliptic system: the bordered matrix assembled in O(nz^2), no solve and no product this step
int mode_gram_elliptic(gpk_handle h, const gpk_gn_problem* p, const Dims& d, double* z, double* S, int, double* Hb, int ldh, int, ModeOut& o) {
    const int nz = d.nz;
    double* d_loss = h->d_scalars;
    GPK_PROF_MARK(h, 0);
    double* coef = S;                                                // d, a, z (column order), then q1, q2: 5 nz doubles of scratch
    structured_coeff_kernel<<<gpk_ceil_div(nz, 256), 256, 0, h->stream>>>(nz, p->nonlin, p->p0, p->p1, p->p2, z, coef, coef + nz, coef + 2 * nz);
    gram_gemv_kernel<<<nz, 256, 0, h->stream>>>(nz, p->G, p->ldg, p->pvec, coef + nz, coef + 2 * nz, coef + 3 * nz);
    GPK_PROF_MARK(h, 1);
    gram_form_kernel<<<nz + 1, 256, 0, h->stream>>>(nz, p->G, p->ldg, coef, coef + 3 * nz, Hb, ldh);
    gram_loss_kernel<<<1, 1024, 0, h->stream>>>(nz, p->pvec, coef + nz, coef + 2 * nz, coef + 3 * nz, Hb + (long)nz * ldh + nz, d_loss);
    // (the level's own loss from w = L^{-1}F(z) itself, see structured_w_kernel; w lives behind the five coefficient vectors in S)
    structured_w_kernel<<<d.rows, 256, 0, h->stream>>>(nz, p->W1, p->W2, p->ldw, p->v0, coef + nz, coef + 2 * nz, coef + 5 * nz);
    GPK_LAUNCH_CHECK(h);
    GPK_TRY(gpk_i_dot(h, coef + 5 * nz, coef + 5 * nz, d.rows, d_loss));
    h->pipe_tev_used = 0; h->prof_pipelined = 0;
    GPK_TRY(gpk_i_potrf(h, Hb, nz + 1, ldh, 0));
    // the REPORTED loss by true substitution here too (round 6; the class API takes its history from this number): one vector on
    // the main stream behind the factorisation -- the level's own d_loss (above) stays the corner of Hb
    return start_exact_loss(h, p, d, z, false, &o.exact, &o.exact_late);
}

// gpk_gn_structured_prepare, Burgers / Eikonal / Darcy (round 6): W = W1 diag(d(z)) + W2 in one memory-bound pass; the F column solved (exact)
int mode_structured_general(gpk_handle h, const gpk_gn_problem* p, const Dims& d, double* z, double* S, int lds, double*, int, int rev, ModeOut& o) {
    const int nz = d.nz;
    GPK_TRY(start_exact_loss(h, p, d, z, true, &o.exact, &o.exact_late));
    GPK_PROF_MARK(h, 0);
    GPK_TRY(gpk_i_workspace(h, (size_t)d.rows * lds * sizeof(double), &o.W));
    h->work_sig[0] = -1;                                             // (the workspace no longer holds a solve of a known shape)
    double* coef = S;                                                // nz doubles of scratch: row 0 of S left of its F column
    structured_coeff_general_kernel<<<gpk_ceil_div(nz, 256), 256, 0, h->stream>>>(p->system, p->Nd, nz, rev, p->p0, p->p1, p->rhs_f, z, coef);
    structured_form_general_kernel<<<d.rows, 256, 0, h->stream>>>(nz, p->W1, p->W2, p->ldw, coef, o.W, lds);
    GPK_LAUNCH_CHECK(h);
    GPK_TRY(build(h, p, z, S, lds, nz, 0));                          // F(z) into column nz of S
    GPK_TRY(solve_f_column(h, p, d, S, lds, o.W + nz, lds));
    GPK_PROF_MARK(h, 1);
    return 0;
}

// gpk_gn_gram_prepare, Burgers / Eikonal / Darcy (round 6): H/2 = D G11 D + D G12 + G21 D + G22 from the Gram blocks of W1 = L^{-1}A1,
// W2 = L^{-1}A2; the border from the SOLVED column w = L^{-1}F(z): g/2 = D W1^T w + W2^T w, loss = w^T w
int mode_gram_general(gpk_handle h, const gpk_gn_problem* p, const Dims& d, double* z, double* S, int lds, double* Hb, int ldh, int rev, ModeOut& o) {
    const int nz = d.nz;
    GPK_TRY(start_exact_loss(h, p, d, z, true, &o.exact, &o.exact_late));
    GPK_PROF_MARK(h, 0);
    double* wv = nullptr;                                            // [w (rows) | d (nz) | q1 (nz) | q2 (nz)]
    GPK_TRY(gpk_i_workspace(h, ((size_t)d.rows + 3 * (size_t)nz + 16) * sizeof(double), &wv));
    h->work_sig[0] = -1;
    double* dcol = wv + ((d.rows + 1) & ~1L);                        // (16-byte aligned)
    double* q = dcol + nz;
    structured_coeff_general_kernel<<<gpk_ceil_div(nz, 256), 256, 0, h->stream>>>(p->system, p->Nd, nz, rev, p->p0, p->p1, p->rhs_f, z, dcol);
    GPK_LAUNCH_CHECK(h);
    GPK_TRY(build(h, p, z, S, lds, nz, 0));                          // F(z) into column nz of S
    GPK_TRY(solve_f_column(h, p, d, S, lds, wv, 1));
    GPK_PROF_MARK(h, 1);
    GPK_TRY(gpk_i_gemm(h, true, false, nz, 1, d.rows, 1.0, p->W1, p->ldw, wv, 1, 0.0, q, 1, false));          // q1 = W1^T w
    GPK_TRY(gpk_i_gemm(h, true, false, nz, 1, d.rows, 1.0, p->W2, p->ldw, wv, 1, 0.0, q + nz, 1, false));     // q2 = W2^T w
    gram_form_kernel<<<nz + 1, 256, 0, h->stream>>>(nz, p->G, p->ldg, dcol, q, Hb, ldh);
    GPK_LAUNCH_CHECK(h);
    GPK_TRY(gpk_i_dot(h, wv, wv, d.rows, Hb + (long)nz * ldh + nz));
    GPK_HIP(h, hipMemcpyAsync(h->d_scalars, Hb + (long)nz * ldh + nz, sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    h->pipe_tev_used = 0; h->prof_pipelined = 0;
    return gpk_i_potrf(h, Hb, nz + 1, ldh, 0);
}

// Darcy (layout 4): Hb = W_u^T W_u (u-part rows + the data rows below them, piecewise profile) + W_a^T W_a (the a-part's own staircase on
// its sub-square of columns, its F column as a border row), d_loss = its corner, then the factorisation
int darcy_product(gpk_handle h, const gpk_gn_problem* p, const Dims& d, const double* W, int lds, double* Hb, int ldh, double* d_loss) {
    const int Nd = p->Nd, nz = d.nz, nc = nz + 1;
    const Group& ga = d.g[0];
    const Group& gu = d.g[1];
    const double* Wa = W + (long)ga.off * lds;
    const double* Wu = W + (long)gu.off * lds;
    const int ph = h->prof_phase;
    h->prof_phase = 2;                                               // (flop accounting: the product)
    h->pipe_tev_used = 0; h->prof_pipelined = 0;
    if (h->prof) {
        while (h->pipe_tev.size() < 2) { hipEvent_t e; GPK_HIP(h, hipEventCreate(&e)); h->pipe_tev.push_back(e); }
        GPK_HIP(h, hipEventRecord(h->pipe_tev[0], h->stream));
    }
    const GpkLz lz_a = GpkLz::closed(3 * Nd);                        // (the a-part's own columns [N_d, 4 N_d))
    int rc = gpk_i_gemm(h, true, false, nc, nc, d.rows - gu.off, 1.0, Wu, lds, Wu, lds, 0.0, Hb, ldh, true, GpkLz::piecewise(darcy_u_profile(Nd)));
    const bool cached_a = p->Wa && p->Ha;                            // (checked: ldwa, ldha >= 3 N_d)
    if (rc == 0 && cached_a) {
        add_lower_kernel<<<3 * Nd, 256, 0, h->stream>>>(3 * Nd, p->Ha, p->ldha, Hb + (long)Nd * ldh + Nd, ldh);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) rc = gpk_fail(h, e, "add_lower_kernel", __FILE__, __LINE__);
    } else if (rc == 0)
        rc = gpk_i_gemm(h, true, false, 3 * Nd, 3 * Nd, ga.n, 1.0, Wa + Nd, lds, Wa + Nd, lds, 1.0, Hb + (long)Nd * ldh + Nd, ldh, true, lz_a);
    if (rc == 0) rc = gpk_i_gemm(h, true, false, 1, 3 * Nd, ga.n, 1.0, Wa + nz, lds, cached_a ? p->Wa : Wa + Nd, cached_a ? p->ldwa : lds, 1.0,
                                 Hb + (long)nz * ldh + Nd, ldh, false, lz_a);
    if (rc == 0) rc = gpk_i_gemm(h, true, false, 1, 1, ga.n, 1.0, Wa + nz, lds, Wa + nz, lds, 1.0, Hb + (long)nz * ldh + nz, ldh, false);
    h->prof_phase = ph;
    GPK_TRY(rc);
    if (h->prof) { GPK_HIP(h, hipEventRecord(h->pipe_tev[1], h->stream)); h->pipe_tev_used = 2; }
    GPK_HIP(h, hipMemcpyAsync(d_loss, Hb + (long)nz * ldh + nz, sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    return gpk_i_potrf(h, Hb, nc, ldh, 0);
}

}  // namespace


extern "C" int gpk_gn_structured_prepare(gpk_handle h, const gpk_gn_problem* p, double* S, int lds, double* W1, double* W2, double* v0, int ldw) {
    if (!h || !S || !W1 || !W2) return GPK_ERR_ARG;
    Dims d;
    GPK_TRY(check_prob(h, p, d));
    const bool elliptic = p->system == GPK_GN_ELLIPTIC;
    if (gn_traits(p->system).no_structured) return gpk_bad_arg(h, gn_traits(p->system).no_structured);
    if (elliptic && !v0) return GPK_ERR_ARG;
    const int nc = d.nz + 1;
    if (lds < nc || ldw < nc) return gpk_bad_arg(h, "structured solve: lds/ldw < nz+1");
    // the other systems (round 6) are prepared -- and later stepped -- in the leading-zero layout of their GEMM-only solve path
    const int rev = elliptic ? 1 : step_layout(h, p);
    if (!elliptic && (rev < 2 || !all_dinv(h, p, d)))
        return gpk_bad_arg(h, "structured solve: this system needs the inverted diagonal blocks of every factor (Dinv, dinv_block) and the leading-zero layout");
    if (!elliptic && (ldw & 1)) return gpk_bad_arg(h, "structured solve: ldw must be even");
    gpk_gn_problem q = *p;                                           // (the Darcy a-part is solved here like everything else: no cache)
    q.Wa = nullptr; q.Ha = nullptr;
    double* zero = nullptr;
    GPK_HIP(h, hipMalloc((void**)&zero, (size_t)d.nz * sizeof(double)));
    hipError_t e = hipMemsetAsync(zero, 0, (size_t)d.nz * sizeof(double), h->stream);
    int rc = e == hipSuccess ? 0 : gpk_fail(h, e, "hipMemsetAsync", __FILE__, __LINE__);
    // elliptic: [I; 0; 0] -> W1;  [0; I; 0] with F(0) -> W2, v0.  Others: the 0/1 pattern of the z-dependent entries -> W1, the constant
    // entries -> W2 (gn_build_kernel, family 1 / 2), all row groups, no F column
    for (int fam = 1; fam <= 2 && rc == 0; ++fam) {
        double* W = nullptr;
        rc = assemble_normal_equations(h, &q, d, zero, S, lds, nullptr, nc, 1.0, rev, &W, fam);   // (no product: Wout is set)
        if (rc) break;
        e = hipMemcpy2DAsync(fam == 1 ? W1 : W2, (size_t)ldw * 8, W, (size_t)lds * 8, (size_t)nc * 8, d.rows, hipMemcpyDeviceToDevice, h->stream);
        if (e == hipSuccess && fam == 2 && elliptic)
            e = hipMemcpy2DAsync(v0, 8, W + d.nz, (size_t)lds * 8, 8, d.rows, hipMemcpyDeviceToDevice, h->stream);
        if (e != hipSuccess) rc = gpk_fail(h, e, "hipMemcpy2DAsync", __FILE__, __LINE__);
    }
    (void)hipStreamSynchronize(h->stream);
    (void)hipFree(zero);
    return rc;
}

extern "C" int gpk_gn_gram_prepare(gpk_handle h, const gpk_gn_problem* p, double* G, int ldg, double* pvec) {
    if (!h || !G || !pvec) return GPK_ERR_ARG;
    Dims d;
    GPK_TRY(check_prob(h, p, d));
    const bool elliptic = p->system == GPK_GN_ELLIPTIC;
    if (gn_traits(p->system).no_gram) return gpk_bad_arg(h, gn_traits(p->system).no_gram);
    if (!p->W1 || !p->W2 || (elliptic && !p->v0))
        return gpk_bad_arg(h, "gram_prepare: needs W1/W2 (and v0 for the elliptic system) of gpk_gn_structured_prepare; not for the relaxed system");
    const int nz = d.nz;
    if (ldg < nz || p->ldw < nz + 1) return gpk_bad_arg(h, "gram_prepare: ldg/ldw");
    const double* Wm[2] = {p->W1, p->W2};
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j)                                  // Gij = Wi^T Wj (full blocks: the gemv reads rows of all four)
            GPK_TRY(gpk_i_gemm(h, true, false, nz, nz, d.rows, 1.0, Wm[i], p->ldw, Wm[j], p->ldw, 0.0, G + (long)(2 * i + j) * nz * ldg, ldg, false));
    if (elliptic) {
        for (int i = 0; i < 2; ++i)                                  // p_i = Wi^T v0 (a one-column product)
            GPK_TRY(gpk_i_gemm(h, true, false, nz, 1, d.rows, 1.0, Wm[i], p->ldw, p->v0, 1, 0.0, pvec + (long)i * nz, 1, false));
        GPK_TRY(gpk_i_dot(h, p->v0, p->v0, d.rows, pvec + 2L * nz));
    } else {
        // the other systems (round 6) solve the column w = L^{-1}F(z) every step and take the border from it: pvec is not used
        GPK_HIP(h, hipMemsetAsync(pvec, 0, (2 * (size_t)nz + 1) * sizeof(double), h->stream));
    }
    GPK_HIP(h, hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int gpk_gn_darcy_prepare(gpk_handle h, const gpk_gn_problem* p, double* S, int lds, double* Wa, int ldwa, double* Ha, int ldha) {
    if (!h || !S || !Wa || !Ha) return GPK_ERR_ARG;
    Dims d;
    GPK_TRY(check_prob(h, p, d));
    if (p->system != GPK_GN_DARCY) return gpk_bad_arg(h, "darcy_prepare: Darcy system only");
    if (!p->Dinv || !p->Dinv2 || p->dinv_block <= 0) return gpk_bad_arg(h, "darcy_prepare: needs Dinv, Dinv2 and dinv_block (the GEMM-only solve path)");
    const int Nd = p->Nd, na = 3 * Nd, nc = d.nz + 1, db = p->dinv_block;
    if (lds < nc || ldwa < na || ldha < na) return gpk_bad_arg(h, "darcy_prepare: lds/ldwa/ldha");
    if (!dinv_block_ok(db)) return gpk_bad_arg(h, "gn: dinv_block must be 256, 512, 1024 or 2048");
    const Group& ga = d.g[0];
    double* zero = nullptr;
    GPK_HIP(h, hipMalloc((void**)&zero, (size_t)d.nz * sizeof(double)));
    int rc = 0;
    hipError_t e = hipMemsetAsync(zero, 0, (size_t)d.nz * sizeof(double), h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(S, 0, (size_t)d.rows * lds * sizeof(double), h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(Wa, 0, (size_t)na * ldwa * sizeof(double), h->stream);   // (never written left of the staircase)
    if (e != hipSuccess) rc = gpk_fail(h, e, "hipMemsetAsync", __FILE__, __LINE__);
    // exactly the step's launches for this block (assemble_normal_equations, rev = 4, k = 0; the product of gpk_gn_step): same
    // kernels, same shapes, same tile configurations -- only the destinations differ, hence bit-identical results
    if (rc == 0) rc = build(h, p, zero, S, lds, d.nz, 1, 4, 0);
    if (rc == 0) rc = gpk_i_trsm_left_dinv(h, ga.L, ga.Dinv, db, ga.n, ga.ldl, S + (long)ga.off * lds + Nd, lds, Wa, ldwa, na, GpkLz::closed(na));
    if (rc == 0) rc = gpk_i_gemm(h, true, false, na, na, ga.n, 1.0, Wa, ldwa, Wa, ldwa, 0.0, Ha, ldha, true, GpkLz::closed(na));
    (void)hipStreamSynchronize(h->stream);
    (void)hipFree(zero);
    return rc;
}

extern "C" int gpk_gn_dims(const gpk_gn_problem* p, int* nz, int* s_rows) {
    Dims d;
    if (!p || gn_dims(p, d) != 0) return GPK_ERR_ARG;
    if (nz) *nz = d.nz;
    if (s_rows) *s_rows = d.rows;
    return 0;
}

extern "C" int gpk_gn_worksize(const gpk_gn_problem* p, int lds, int* host_lds, size_t* S_bytes, size_t* Hb_bytes, size_t* delta_bytes,
                               size_t* handle_bytes) {
    Dims d;
    if (!p || gn_dims(p, d) != 0) return GPK_ERR_ARG;
    const int nc = d.nz + 1;
    if (lds == 0) lds = ((nc + 15) / 16) * 16;
    if (lds < nc) return GPK_ERR_ARG;
    // as assemble_normal_equations decides it (dinv_block = 0 means 256 there too); the figure assumes the default gpk_tune(10, 1) -- with
    // the substitution schedule forced the handle reserves nothing
    const bool dinv = every_factor_has_dinv(d);
    if (host_lds) *host_lds = lds;
    if (S_bytes) *S_bytes = (size_t)d.rows * lds * sizeof(double);
    if (Hb_bytes) *Hb_bytes = (size_t)nc * lds * sizeof(double);
    if (delta_bytes) *delta_bytes = (size_t)d.nz * sizeof(double);
    if (handle_bytes) *handle_bytes = (dinv ? (size_t)d.rows * lds * sizeof(double) : 0) + (size_t)d.rows * sizeof(double);
    return 0;
}

namespace {

// What a caller of step_core wants of the step: gpk_gn_step {update, no pred, finish}; gpk_gn_direction {no update, pred, finish};
// gpk_gn_step_ls {no update, pred, no finish: it goes on issuing work and reads the scalars itself after ITS one synchronisation}.
struct StepWant { bool update; double step_size; bool pred; bool finish; };

// after the step's synchronisation: the per-phase timings of a handle with profiling on
int step_read_prof(gpk_handle h) {
    if (!h->prof) return 0;
    for (int i = 0; i < 4; ++i) {
        float ms = 0.f;
        GPK_HIP(h, hipEventElapsedTime(&ms, h->pev[i], h->pev[i + 1]));
        h->prof_ms[i] += (double)ms;
    }
    h->prof_cnt += 1;
    for (int i = 0; i + 1 < h->pipe_tev_used; i += 2) {              // SYRK launches of the pipelined product (GEMM stream)
        float ms = 0.f;
        GPK_HIP(h, hipEventElapsedTime(&ms, h->pipe_tev[i], h->pipe_tev[i + 1]));
        h->prof_syrk_ms += (double)ms;
    }
    return 0;
}

// One Gauss-Newton step up to (want.update: and including) the update of z.  *d_loss_out: the device scalar that holds the loss of the
// input iterate once the handle's stream has passed the point where this function returns (want.finish == false), h->d_scalars[9]: pred.
int step_core(gpk_handle h, const gpk_gn_problem* p, double* z, const StepWant& want, double* S, int lds, double* Hb, int ldh, double* delta,
              double* host_loss_in, double* host_pred, int* host_info, const double** d_loss_out) {
    Dims d;
    GPK_TRY(check_prob(h, p, d));
    const int nz = d.nz;
    if (p->system == GPK_GN_DARCY && p->Wa && p->Ha && (p->ldwa < 3 * p->Nd || p->ldha < 3 * p->Nd))
        return gpk_bad_arg(h, "gn: ldwa/ldha < 3 Nd (gpk_gn_darcy_prepare)");
    const int rev = step_layout(h, p);
    const StepMode mode = select_mode(h, p, d, rev);
    double* d_loss = h->d_scalars;
    GPK_HIP(h, hipMemsetAsync(h->d_info, 0, sizeof(int), h->stream));
    if (h->tune.structured && p->W1 && (long)d.rows * lds < 5L * nz + d.rows)   // (every structured mode has W1; S is their scratch)
        return gpk_bad_arg(h, "gn: S too small for the scratch vectors of the structured modes");
    ModeOut o;
    switch (mode) {
        case StepMode::Plain:              GPK_TRY(mode_plain(h, p, d, z, S, lds, Hb, ldh, rev, o)); break;
        case StepMode::StructuredElliptic: GPK_TRY(mode_structured_elliptic(h, p, d, z, S, lds, Hb, ldh, rev, o)); break;
        case StepMode::GramElliptic:       GPK_TRY(mode_gram_elliptic(h, p, d, z, S, lds, Hb, ldh, rev, o)); break;
        case StepMode::StructuredGeneral:  GPK_TRY(mode_structured_general(h, p, d, z, S, lds, Hb, ldh, rev, o)); break;
        case StepMode::GramGeneral:        GPK_TRY(mode_gram_general(h, p, d, z, S, lds, Hb, ldh, rev, o)); break;
    }
    // Hb = W^T W and its Cholesky factor, pipelined by column blocks (gpk_factor.hip); d_loss = Hb[nz][nz] before factoring;
    // the last row of the factor is (L_H^{-1} g/2)^T
    const StepProduct product = select_product(mode, rev);
    if (product == StepProduct::Darcy) GPK_TRY(darcy_product(h, p, d, o.W, lds, Hb, ldh, d_loss));
    else if (product == StepProduct::SyrkPotrf) GPK_TRY(gpk_i_syrk_potrf(h, o.W, lds, d.rows, nz + 1, step_profile(h, p, nz, rev), Hb, ldh, d_loss));
    GPK_PROF_MARK(h, 2);
    GPK_PROF_MARK(h, 3);
    // the chain of the exact loss: on the GEMM partition's stream from here on (pipelined phase: that stream's last product finished before the
    // last panel chain did, so it starts early; otherwise behind the factorisation just issued), next to the tail below
    // (any error return from here to the end of the call first drains the side stream: the next call's exact_loss_build memsets d_loss_work
    // on the main stream, which must not happen under a chain that is still reading it)
    struct ChainGuard {
        gpk_handle h; bool armed;
        ~ChainGuard() { if (armed && h->pipe_g) (void)hipStreamSynchronize(h->pipe_g); }
    } chain_guard{h, false};
    bool chain_on_side = false;
    if (o.exact_late) {
        GPK_TRY(exact_loss_chain(h, d, !h->prof_pipelined, &chain_on_side));
        chain_guard.armed = chain_on_side;
    }
    GPK_TRY(gpk_i_gn_finish(h, p, nz, rev, Hb, ldh, S, delta, z, want.step_size, want.update));   // (S is free now: scratch for the reversed-order solution)
    // pred = |y|^2 = g . delta / 2 over the last row of the factored Hb (the backward solve above worked on a copy of it)
    if (want.pred) GPK_TRY(gpk_i_dot(h, Hb + (long)nz * ldh, Hb + (long)nz * ldh, nz, h->d_scalars + 9));
    GPK_PROF_MARK(h, 4);
    const double* d_loss_final = o.exact ? h->d_scalars + 8 : d_loss;
    if (d_loss_out) *d_loss_out = d_loss_final;
    if (!want.finish) {
        // the caller goes on on the handle's stream: join the chain there (everything issued later, the next call's memset of d_loss_work
        // included, is ordered behind it) and leave the scalars on the device
        if (chain_on_side) GPK_HIP(h, hipStreamWaitEvent(h->stream, h->ev_loss[1], 0));
        chain_guard.armed = false;
        return 0;
    }
    // the two host scalars of the step through pinned memory (h_pinned[0] = loss, the int behind h_pinned[1] = pivot status)
    GPK_HIP(h, hipMemcpyAsync(h->h_pinned + 1, h->d_info, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (want.pred) GPK_HIP(h, hipMemcpyAsync(h->h_pinned + 2, h->d_scalars + 9, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (chain_on_side) GPK_HIP(h, hipStreamWaitEvent(h->stream, h->ev_loss[1], 0));
    GPK_HIP(h, hipMemcpyAsync(h->h_pinned, d_loss_final, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    GPK_HIP(h, hipStreamSynchronize(h->stream));
    chain_guard.armed = false;                                       // the main stream waited for the chain's event: it is complete
    int info = *reinterpret_cast<const int*>(h->h_pinned + 1);
    const double loss = h->h_pinned[0];
    GPK_TRY(step_read_prof(h));
    if (info == nz + 1) info = 0;          // the border pivot loss - y^T y is not part of H (may round below zero)
    if (host_info) *host_info = info;
    if (host_loss_in) *host_loss_in = loss;
    if (host_pred) *host_pred = h->h_pinned[2];
    return 0;
}

}  // namespace

extern "C" int gpk_gn_step(gpk_handle h, const gpk_gn_problem* p, double* z, double step_size, double* S, int lds,
                           double* Hb, int ldh, double* delta, double* host_loss_in, int* host_info) {
    if (!h || !z || !S || !Hb || !delta) return GPK_ERR_ARG;
    return step_core(h, p, z, StepWant{true, step_size, false, true}, S, lds, Hb, ldh, delta, host_loss_in, nullptr, host_info, nullptr);
}

extern "C" int gpk_gn_direction(gpk_handle h, const gpk_gn_problem* p, const double* z, double* S, int lds, double* Hb, int ldh,
                                double* delta, double* host_loss_in, double* host_pred, int* host_info) {
    if (!h) return GPK_ERR_ARG;
    if (!z || !S || !Hb || !delta) return gpk_bad_arg(h, "gn_direction: null z / S / Hb / delta");
    // (z is read only: want.update = false takes the update launch out of the tail and nothing else writes it)
    return step_core(h, p, const_cast<double*>(z), StepWant{false, 0.0, true, true}, S, lds, Hb, ldh, delta, host_loss_in, host_pred, host_info,
                     nullptr);
}

// ---- line search ("Line search") ---------------------------------------------------------------------------------
namespace {

// The caller's trial workspace W: [B: rows x ldw, the K right-hand sides | X: rows x ldw, the out-of-place result of the GEMM-only solve,
// present when every factor comes with its inverted diagonal blocks | the partial sums of the column reduction].  A function of the
// problem, K and ldw alone: gpk_gn_trial_worksize and the calls agree on it whatever the handle's switches say.
struct TrialLayout { int ldw; size_t b_doubles, x_doubles, red_bytes; };

int trial_layout(const Dims& d, int K, int ldw, TrialLayout& t) {
    if (K < 1 || K > LS_MAX) return GPK_ERR_ARG;
    if (ldw == 0) ldw = ((K + 15) / 16) * 16;
    if (ldw < K) return GPK_ERR_ARG;
    t.ldw = ldw;
    t.b_doubles = (size_t)d.rows * ldw;
    t.x_doubles = every_factor_has_dinv(d) ? t.b_doubles : 0;
    t.red_bytes = gpk_i_col_sumsq_scratch_bytes(d.rows, K);
    return 0;
}

int trial_steps(gpk_handle h, const double* host_t, int K, TrialT& ts) {
    if (K < 1 || K > LS_MAX) return gpk_bad_arg(h, "line search: K must be 1 .. GPK_LS_MAX_TRIALS (16)");
    if (!host_t) return gpk_bad_arg(h, "line search: null step sizes");
    for (int k = 0; k < LS_MAX; ++k) ts.t[k] = k < K ? host_t[k] : 0.0;
    for (int k = 0; k < K; ++k) if (!std::isfinite(ts.t[k])) return gpk_bad_arg(h, "line search: a step size is not finite");
    return 0;
}

// F(z - t_k delta), k < K, into the columns of W (rows x ldw); nothing else of W is written
int trial_build(gpk_handle h, const gpk_gn_problem* p, const double* z, const double* delta, const TrialT& ts, int K, double* W, int ldw) {
    const BuildArgs a = build_args(p, z, W, ldw, 0, 0, 0, 0);
    const long threads = (long)(p->Nd + p->Nb) * K;
    gn_trial_build_kernel<<<(unsigned)((threads + 255) / 256), 256, 0, h->stream>>>(a, delta, ts, K);
    GPK_LAUNCH_CHECK(h);
    return 0;
}

// dev_losses[k] = J(z - t_k delta): the build, one K-column forward solve per factor, the column sums of squares; all on h->stream
int trial_losses_issue(gpk_handle h, const gpk_gn_problem* p, const Dims& d, const double* z, const double* delta, const TrialT& ts, int K,
                       double* W, const TrialLayout& t, double* dev_losses) {
    const bool dinv = h->tune.use_dinv && t.x_doubles > 0;
    const int db = p->dinv_block > 0 ? p->dinv_block : 256;
    if (dinv && !dinv_block_ok(db)) return gpk_bad_arg(h, "gn: dinv_block must be 256, 512, 1024 or 2048");
    const int ldw = t.ldw;
    double* B = W;
    double* X = W + t.b_doubles;
    double* red = W + t.b_doubles + t.x_doubles;
    GPK_TRY(trial_build(h, p, z, delta, ts, K, B, ldw));
    for (int k = 0; k < d.ngroups; ++k) {
        const Group& g = d.g[k];
        if (g.n <= 0) continue;
        double* Bg = B + (long)g.off * ldw;
        if (!g.L) {                                                  // rows without a factor: the build scaled them (1 / sqrt(lambda), 1 / gamma)
            if (dinv) GPK_HIP(h, hipMemcpy2DAsync(X + (long)g.off * ldw, (size_t)ldw * 8, Bg, (size_t)ldw * 8, (size_t)K * 8, g.n,
                                                  hipMemcpyDeviceToDevice, h->stream));
        } else if (dinv) {
            GPK_TRY(gpk_i_trsm_left_dinv(h, g.L, g.Dinv, db, g.n, g.ldl, Bg, ldw, X + (long)g.off * ldw, ldw, K, GpkLz()));
        } else {
            GPK_TRY(gpk_i_trsm_left_mt(h, false, g.L, g.n, g.ldl, Bg, K, ldw));
        }
    }
    return gpk_i_col_sumsq(h, dinv ? X : B, d.rows, K, ldw, dev_losses, red);
}

// the accepted index (-> the int at d_scalars[11]) and step (-> d_scalars[10]) from the K losses, then the update of z
int accept_issue(gpk_handle h, int nz, double* z, const double* delta, const double* dev_losses, const TrialT& ts, int K, const double* d_loss_in,
                 const double* d_pred, double loss_in, double pred, double c1, const int* d_info) {
    int* d_k = reinterpret_cast<int*>(h->d_scalars + 11);
    ls_select_kernel<<<1, 64, 0, h->stream>>>(dev_losses, ts, K, d_loss_in, d_pred, loss_in, pred, c1, d_info, nz + 1, d_k, h->d_scalars + 10);
    GPK_LAUNCH_CHECK(h);
    ls_update_kernel<<<gpk_ceil_div(nz, 256), 256, 0, h->stream>>>(nz, d_k, ts, delta, z);
    GPK_LAUNCH_CHECK(h);
    GPK_HIP(h, hipMemcpyAsync(h->h_pinned + 3, d_k, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    GPK_HIP(h, hipMemcpyAsync(h->h_pinned + 4, h->d_scalars + 10, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    return 0;
}

}  // namespace

extern "C" int gpk_gn_trial_worksize(const gpk_gn_problem* p, int K, int ldw, int* host_ldw, size_t* bytes) {
    Dims d;
    TrialLayout t;
    if (!p || gn_dims(p, d) != 0 || trial_layout(d, K, ldw, t) != 0) return GPK_ERR_ARG;
    if (host_ldw) *host_ldw = t.ldw;
    if (bytes) *bytes = (t.b_doubles + t.x_doubles) * sizeof(double) + t.red_bytes;
    return 0;
}

extern "C" int gpk_gn_trial_losses(gpk_handle h, const gpk_gn_problem* p, const double* z, const double* delta, const double* host_t, int K,
                                   double* W, int ldw, double* dev_losses, double* host_losses) {
    if (!h) return GPK_ERR_ARG;
    if (!z || !delta || !W || !dev_losses) return gpk_bad_arg(h, "gn_trial_losses: null z / delta / W / dev_losses");
    Dims d;
    GPK_TRY(check_prob(h, p, d));
    TrialT ts;
    GPK_TRY(trial_steps(h, host_t, K, ts));
    TrialLayout t;
    if (ldw <= 0 || trial_layout(d, K, ldw, t) != 0) return gpk_bad_arg(h, "gn_trial_losses: ldw < K");
    GPK_TRY(trial_losses_issue(h, p, d, z, delta, ts, K, W, t, dev_losses));
    if (!host_losses) return 0;                                      // nothing is downloaded, nothing synchronises
    GPK_HIP(h, hipMemcpyAsync(h->h_pinned + 8, dev_losses, (size_t)K * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    GPK_HIP(h, hipStreamSynchronize(h->stream));
    for (int k = 0; k < K; ++k) host_losses[k] = h->h_pinned[8 + k];
    return 0;
}

extern "C" int gpk_gn_trial_accept(gpk_handle h, int nz, double* z, const double* delta, const double* dev_losses, const double* host_t, int K,
                                   double loss_in, double pred, double c1, int* host_k, double* host_t_acc) {
    if (!h) return GPK_ERR_ARG;
    if (nz <= 0 || !z || !delta || !dev_losses) return gpk_bad_arg(h, "gn_trial_accept: nz <= 0 or null z / delta / dev_losses");
    if (!(c1 > 0.0 && c1 < 1.0)) return gpk_bad_arg(h, "gn_trial_accept: c1 must lie in (0, 1)");
    TrialT ts;
    GPK_TRY(trial_steps(h, host_t, K, ts));
    GPK_TRY(accept_issue(h, nz, z, delta, dev_losses, ts, K, nullptr, nullptr, loss_in, pred, c1, nullptr));
    GPK_HIP(h, hipStreamSynchronize(h->stream));
    if (host_k) *host_k = *reinterpret_cast<const int*>(h->h_pinned + 3);
    if (host_t_acc) *host_t_acc = h->h_pinned[4];
    return 0;
}

extern "C" int gpk_gn_step_ls(gpk_handle h, const gpk_gn_problem* p, double* z, const gpk_ls_options* opt, double* S, int lds, double* Hb, int ldh,
                              double* delta, double* W, int ldw, double* host_loss_in, double* host_losses, int* host_k, double* host_t_acc,
                              int* host_info) {
    if (!h) return GPK_ERR_ARG;
    if (!z || !S || !Hb || !delta || !W) return gpk_bad_arg(h, "gn_step_ls: null z / S / Hb / delta / W");
    const int K = (opt && opt->K) ? opt->K : 8;
    const double t0 = (opt && opt->t0 != 0.0) ? opt->t0 : 1.0, beta = (opt && opt->beta != 0.0) ? opt->beta : 0.5;
    const double c1 = (opt && opt->c1 != 0.0) ? opt->c1 : 1e-4;
    if (K < 1 || K > LS_MAX) return gpk_bad_arg(h, "line search: K must be 1 .. GPK_LS_MAX_TRIALS (16)");
    if (!(t0 > 0.0 && std::isfinite(t0))) return gpk_bad_arg(h, "line search: t0 must be positive and finite");
    if (!(beta > 0.0 && beta < 1.0)) return gpk_bad_arg(h, "line search: beta must lie in (0, 1)");
    if (!(c1 > 0.0 && c1 < 1.0)) return gpk_bad_arg(h, "line search: c1 must lie in (0, 1)");
    Dims d;
    GPK_TRY(check_prob(h, p, d));
    TrialLayout t;
    if (ldw <= 0 || trial_layout(d, K, ldw, t) != 0) return gpk_bad_arg(h, "gn_step_ls: ldw < K");
    TrialT ts;
    for (int k = 0; k < LS_MAX; ++k) ts.t[k] = 0.0;
    ts.t[0] = t0;
    for (int k = 1; k < K; ++k) ts.t[k] = ts.t[k - 1] * beta;        // t_k = t0 beta^k by repeated multiplication: one rounding per trial
    const double* d_loss = nullptr;
    GPK_TRY(step_core(h, p, z, StepWant{false, 0.0, true, false}, S, lds, Hb, ldh, delta, nullptr, nullptr, nullptr, &d_loss));
    double* dev_losses = h->d_scalars + 32;
    GPK_TRY(trial_losses_issue(h, p, d, z, delta, ts, K, W, t, dev_losses));
    // the Armijo test uses the exact substituted loss: step_core has joined its chain to the handle's stream already, in FRONT of the trial
    // build and solve (the acceptance is its only consumer; joining there instead would let the chain run beside the K-column solve -- not
    // measured, DESIGN.md section K "Line search")
    GPK_TRY(accept_issue(h, d.nz, z, delta, dev_losses, ts, K, d_loss, h->d_scalars + 9, 0.0, 0.0, c1, h->d_info));
    GPK_HIP(h, hipMemcpyAsync(h->h_pinned + 1, h->d_info, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    GPK_HIP(h, hipMemcpyAsync(h->h_pinned, d_loss, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    GPK_HIP(h, hipMemcpyAsync(h->h_pinned + 8, dev_losses, (size_t)K * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    GPK_HIP(h, hipStreamSynchronize(h->stream));                     // the one host synchronisation of the call
    GPK_TRY(step_read_prof(h));
    int info = *reinterpret_cast<const int*>(h->h_pinned + 1);
    if (info == d.nz + 1) info = 0;
    if (host_info) *host_info = info;
    if (host_loss_in) *host_loss_in = h->h_pinned[0];
    if (host_losses) for (int k = 0; k < K; ++k) host_losses[k] = h->h_pinned[8 + k];
    if (host_k) *host_k = *reinterpret_cast<const int*>(h->h_pinned + 3);
    if (host_t_acc) *host_t_acc = h->h_pinned[4];
    return 0;
}

extern "C" int gpk_gn_loss(gpk_handle h, const gpk_gn_problem* p, const double* z, double* work, double* host_loss) {
    if (!h || !z || !work || !host_loss) return GPK_ERR_ARG;
    Dims d;
    GPK_TRY(check_prob(h, p, d));
    GPK_TRY(substitution_loss(h, p, d, z, work, h->d_scalars + 1));
    GPK_HIP(h, hipMemcpyAsync(host_loss, h->d_scalars + 1, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    GPK_HIP(h, hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int gpk_gn_hessian_grad(gpk_handle h, const gpk_gn_problem* p, const double* z, double* S, int lds, double* H,
                                   int ldh, double* g) {
    if (!h || !z || !S || !H) return GPK_ERR_ARG;
    Dims d;
    GPK_TRY(check_prob(h, p, d));
    GPK_TRY(assemble_normal_equations(h, p, d, z, S, lds, H, ldh, 2.0, 0));   // H = 2 S^T S, g = 2 S^T w in the border row
    if (g) GPK_HIP(h, hipMemcpyAsync(g, H + (long)d.nz * ldh, (size_t)d.nz * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    return gpk_symmetrize_lower(h, H, d.nz, ldh);
}

extern "C" int gpk_gn_build(gpk_handle h, const gpk_gn_problem* p, const double* z, double* S, int lds) {
    if (!h || !z || !S) return GPK_ERR_ARG;
    Dims d;
    gpk_gn_problem q = *p;
    if (gn_dims(&q, d) != 0) return gpk_bad_arg(h, "gn: system id / sizes");
    GPK_TRY(check_nonlin(h, &q));
    if (lds < d.nz + 1) return gpk_bad_arg(h, "gn: lds < nz+1");
    GPK_HIP(h, hipMemsetAsync(S, 0, (size_t)d.rows * lds * sizeof(double), h->stream));
    return build(h, &q, z, S, lds, d.nz, 1);
}

extern "C" int gpk_gn_build_rev(gpk_handle h, const gpk_gn_problem* p, const double* z, double* S, int lds) {
    if (!h || !z || !S || !p) return GPK_ERR_ARG;
    // (round 6: also the Eikonal and Burgers systems in the staircase orders of their gpk_gn_step -- the sharded step uses them)
    const int rev = step_layout(h, p);
    if (rev < 1 || rev > 6 || p->system == GPK_GN_ELLIPTIC_RELAXED) return gpk_bad_arg(h, "gn_build_rev: not for the relaxed system / needs the leading-zero layout");
    Dims d;
    gpk_gn_problem q = *p;
    if (gn_dims(&q, d) != 0) return gpk_bad_arg(h, "gn: system id / sizes");
    GPK_TRY(check_nonlin(h, &q));
    if (lds < d.nz + 1) return gpk_bad_arg(h, "gn: lds < nz+1");
    GPK_HIP(h, hipMemsetAsync(S, 0, (size_t)d.rows * lds * sizeof(double), h->stream));
    return build(h, &q, z, S, lds, d.nz, 1, rev);
}

extern "C" int gpk_axpy(gpk_handle h, int n, double alpha, const double* x, double* y) {
    if (!h || !x || !y || n < 0) return GPK_ERR_ARG;
    if (n == 0) return 0;
    axpy_kernel<<<gpk_ceil_div(n, 256), 256, 0, h->stream>>>(n, alpha, x, y);
    GPK_LAUNCH_CHECK(h);
    return 0;
}

extern "C" int gpk_gn_measurement(gpk_handle h, const gpk_gn_problem* p, const double* z, double* out) {
    if (!h || !z || !out) return GPK_ERR_ARG;
    Dims d;
    gpk_gn_problem q = *p;
    if (gn_dims(&q, d) != 0) return gpk_bad_arg(h, "gn: system id / sizes");
    GPK_TRY(check_nonlin(h, &q));
    GPK_HIP(h, hipMemsetAsync(out, 0, (size_t)d.rows * sizeof(double), h->stream));
    return build(h, &q, z, out, 1, 0, 0);
}

// ---- building blocks of the multi-GPU step (gpk_mg.hip) ---------------------------------------------------------------------
// exact in-step loss for the sharded step (replicated on every rank: one vector), on h->stream; the device scalar comes back
int gpk_i_gn_exact_loss(gpk_handle h, const gpk_gn_problem* p, const double* z, double** d_out) {
    Dims d;
    GPK_TRY(check_prob(h, p, d));
    GPK_TRY(exact_loss(h, p, d, z));
    *d_out = h->d_scalars + 8;
    return 0;
}

int gpk_i_gn_layout(gpk_handle h, const gpk_gn_problem* p) { return step_layout(h, p); }
bool gpk_i_gn_sharded(const gpk_gn_problem* p) { return gn_traits(p->system).sharded; }
GpkLz gpk_i_gn_profile(gpk_handle h, const gpk_gn_problem* p, int rev) {
    Dims d;
    return gn_dims(p, d) == 0 ? step_profile(h, p, d.nz, rev) : GpkLz();
}

// Darcy pieces of the sharded step (gpk_mg.hip): the u-part's three-segment profile ...
GpkLz gpk_i_gn_darcy_u_profile(int Nd) { return GpkLz::piecewise(darcy_u_profile(Nd)); }

// ... and the cached a-part added to the rows [r0, r1) of Hb a rank has just computed from the u-part and data rows: H_a on the rows that lie
// in [N_d, 4 N_d) and, if row n_z is among them, the border terms (L_a^{-1}F_a)^T W_a and |L_a^{-1}F_a|^2 (aF: the solved a-part F column,
// 3 N_d entries with stride ldaf) -- the launches of gpk_gn_step's rev = 4 branch, restricted to those rows
__global__ __launch_bounds__(256) void add_lower_rows_kernel(int row0, const double* __restrict__ A, long lda, double* __restrict__ Cm, long ldc) {
    const long i = row0 + blockIdx.x;                                 // row of the 3 N_d x 3 N_d lower triangle
    const double* a = A + i * lda;
    double* c = Cm + i * ldc;
    for (int j = threadIdx.x; j <= (int)i; j += 256) c[j] += a[j];
}

int gpk_i_gn_darcy_add_a(gpk_handle h, const gpk_gn_problem* p, double* Hb, int ldh, int r0, int r1, const double* aF, int ldaf) {
    const int Nd = p->Nd, na = 3 * Nd, nz = 6 * Nd;
    const int a0 = std::max(r0, Nd), a1 = std::min(r1, 4 * Nd);
    if (a1 > a0) {
        add_lower_rows_kernel<<<a1 - a0, 256, 0, h->stream>>>(a0 - Nd, p->Ha, p->ldha, Hb + (long)Nd * ldh + Nd, ldh);
        GPK_LAUNCH_CHECK(h);
    }
    if (r0 <= nz && nz < r1) {
        // (closed-form staircase of the a-part's own columns, as on one GPU)
        GPK_TRY(gpk_i_gemm(h, true, false, 1, na, na, 1.0, aF, ldaf, p->Wa, p->ldwa, 1.0, Hb + (long)nz * ldh + Nd, ldh, false, GpkLz::closed(na)));
        GPK_TRY(gpk_i_gemm(h, true, false, 1, 1, na, 1.0, aF, ldaf, aF, ldaf, 1.0, Hb + (long)nz * ldh + nz, ldh, false));
    }
    return 0;
}

// n_z and the row count of the system handled by the sharded step
int gpk_i_gn_dims(gpk_handle h, const gpk_gn_problem* p, int* nz, int* rows) {
    Dims d;
    GPK_TRY(check_prob(h, p, d));
    *nz = d.nz; *rows = d.rows;
    return 0;
}

// The tail of a step once the bordered matrix Hb is factored (its last row = (L_H^{-1} g/2)^T): backward solve, back to the natural
// order of the unknowns (rev: the staircase order of gpk_gn_step), update of z.  scratch: nz doubles (rev only).
int gpk_i_gn_finish(gpk_handle h, const gpk_gn_problem* p, int nz, int rev, const double* Hb, int ldh, double* scratch, double* delta,
                    double* z, double step_size, bool update) {
    double* dl = rev ? scratch : delta;
    GPK_HIP(h, hipMemcpyAsync(dl, Hb + (long)nz * ldh, (size_t)nz * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    GPK_TRY(gpk_i_trsv(h, true, Hb, nz, ldh, dl));
    if (rev) {
        reverse_copy_kernel<<<gpk_ceil_div(nz, 256), 256, 0, h->stream>>>(nz, dl, delta, rev, p->Nd);
        if (update) axpy_rev_kernel<<<gpk_ceil_div(nz, 256), 256, 0, h->stream>>>(nz, -step_size, dl, z, rev, p->Nd);
    } else if (update) {
        axpy_kernel<<<gpk_ceil_div(nz, 256), 256, 0, h->stream>>>(nz, -step_size, delta, z);
    }
    GPK_LAUNCH_CHECK(h);
    return 0;
}


#ifdef GPK_DEV
#include "dev/gpk_gn_dev_abi.inc"        // gpk_debug_set_profile, gpk_debug_syrk_lz, gpk_debug_first_rows, gpk_debug_step_mode (include/gpk_dev.h): development build only
#endif
