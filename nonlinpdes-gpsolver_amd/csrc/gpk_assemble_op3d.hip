// gpk_assemble_op3d.hip -- the fused derivative-kernel evaluator of the 3-D elliptic layout with a general second-order linear functional
// at every domain point and a first-order one at every boundary point: the Gram matrix and the matrix-free extension with all
// derivatives up to order two.  It serves 3-D advection-diffusion-reaction with Dirichlet / Neumann / Robin data and, with axis 3 as
// time, parabolic equations in two space dimensions by space-time collocation (psi = nu Lap_x - d_t).
//
// No reference call site (the reference is 2-D and knows the Laplacian only).  The elliptic Gauss-Newton system sees block 0 through
// sol_vec = [alpha z^m - f, z, g] alone, so any linear psi with psi[u] = alpha u^m - f reuses gpk_potrf, gpk_gn_step, gpk_potrs and
// gpk_pde_residual unchanged (src/PDEs.py, Nonlinear_elliptic3d(operator=...)).
//
// Math (DESIGN.md §K "Operator and boundary functionals in three dimensions").  Multi-indices, in the order of op3:
//   MI3 = {(0,0,0), (1,0,0),(0,1,0),(0,0,1), (2,0,0),(1,1,0),(1,0,1),(0,2,0),(0,1,1),(0,0,2)}
// Domain point i carries psi_i = sum_j op3[i][j] d^MI3_j in block 0 and delta in block 1; boundary point b carries phi_b = bc3[b][0] delta
// + sum_k bc3[b][k] d_k in block 1.  With d = x - y, d_x^alpha d_y^beta kappa = (-1)^{|alpha|} prod_k h_{alpha_k+beta_k}(p_k, d_k) kappa:
//   <F, G'> = sum_i r_i (-1)^{|alpha_i|} C[alpha_i],   C[m] = sum_j k_j a[m1 + beta1_j] b[m2 + beta2_j] c[m3 + beta3_j],  |m| <= 2
// r the coefficients of the row functional (at x), k those of the column functional (at y), a / b / c the Hermite tables of the three
// axes.  The column's coefficients are contracted with the tables first, axis by axis (108 operations for psi', 50 for phi'), then the
// rows with C (10 or 4 operations per entry): ~190 operations for the four entries of a point pair instead of 196 separate
// three-factor terms.  Per-axis order <= 2 + 2: h0..h4 suffice; one exp and three Hermite evaluations per POINT PAIR feed all blocks.
//
// Mapping to the hardware, as assemble_op_kernel / assemble_op2_kernel: SoA-packed points and coefficients in the handle's point
// scratch (3 + 4 + 10 arrays of Nd+Nb), a workgroup owns TP row points x 256 column points (two-point variant: x 512), lane <-> column
// point (its coordinates and 14 coefficients stay in registers), the row point and its coefficients are wave-uniform and arrive by scalar
// loads: the Gram kernels read the packed scratch through the constant address space (cdouble_p), so the compiler knows that the stores
// to Theta cannot change it (through a plain pointer it issues vector loads at a uniform address and keeps the row in VGPRs).
// The two-point variant evaluates its two column points one after the other and keeps the four finished entries of the first only.
// No inline assembly.
//
// Shared with the other evaluators (gpk_assemble_common.h): hermite_compensated, the frame of the extension kernel, store2 and the
// host side of a call (precisions, nugget, boundary trace, timing, launch); shared with gpk_assemble_grad3d.hip (gpk_assemble_op3.h): the
// tables of the contraction, the packed scratch and the domain trace.
#include "gpk_assemble_op3.h"

using namespace gpk_asm;

// One-point and two-point evaluator must give the same bits for the same point pair: explicit fma, no contraction by the compiler.
// The extension kernels share the table arithmetic and are written the same way.
#pragma clang fp contract(off)

namespace {

struct Op3Args {
    const double* s;                      // packed scratch: array k (x, y, z, phi 0..3, psi 0..9) at s + k * M; domain points first
    int Nd, M;                            // M = Nd + Nb
    double p1, p2, p3;
    double* out; long ld;
    double nug[2];
    __device__ cdouble_p arr(int k) const { return (cdouble_p)(s + (size_t)k * (size_t)M); }
};

// the column point of a lane: coordinates, coefficients of phi' and of psi'
struct Col3 {
    double y[3], k[NC], ko[NO];
    __device__ __forceinline__ void load(const Op3Args& g, int q, bool live) {
#pragma unroll
        for (int j = 0; j < 3; ++j) y[j] = live ? g.arr(j)[q] : 0.0;
#pragma unroll
        for (int j = 0; j < NC; ++j) k[j] = live ? g.arr(3 + j)[q] : 0.0;
#pragma unroll
        for (int j = 0; j < NO; ++j) ko[j] = live ? g.arr(3 + NC + j)[q] : 0.0;
    }
};

// the row point of a workgroup's step (wave-uniform)
struct Row3 {
    double x[3], r[NC], ro[NO];
    __device__ __forceinline__ void load(const Op3Args& g, int p) {                 // uniform address -> scalar loads
#pragma unroll
        for (int j = 0; j < 3; ++j) x[j] = g.arr(j)[p];
#pragma unroll
        for (int j = 0; j < NC; ++j) r[j] = g.arr(3 + j)[p];
#pragma unroll
        for (int j = 0; j < NO; ++j) ro[j] = g.arr(3 + NC + j)[p];
    }
};

// The four entries one point pair contributes: v[0] = <psi, psi'>, v[1] = <psi, phi'>, v[2] = <phi, psi'>, v[3] = <phi, phi'> (psi
// rows: when `top`; psi' columns: when `dom`; the others are left as they are).  One function for both evaluators: the same operations.
__device__ __forceinline__ void pair_entries(const Op3Args& g, const Row3& w, const Col3& u, bool top, bool dom, double (&v)[4]) {
    const double d1 = w.x[0] - u.y[0], d2 = w.x[1] - u.y[1], d3 = w.x[2] - u.y[2];
    const double e = kappa3_fma(g.p1, g.p2, g.p3, d1, d2, d3);
    double a[5], b[5], c[5], t[NO];
    hermite_compensated(g.p1, d1, a);
    hermite_compensated(g.p2, d2, b);
    hermite_compensated(g.p3, d3, c);
    table_phi3(a, b, c, u.k, t);
    if (top) v[1] = row_psi3(t, w.ro) * e;
    v[3] = row_phi3(t, w.r) * e;
    if (dom) {
        table_psi3<>(a, b, c, u.ko, t);
        if (top) v[0] = row_psi3(t, w.ro) * e;
        v[2] = row_phi3(t, w.r) * e;
    }
}

// one column point per lane, 8-byte stores: any alignment, any Nd / Nb
__global__ __launch_bounds__(256) void assemble_op3_kernel(Op3Args g) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    const bool live = q < g.M;
    const bool dom = q < g.Nd;
    Col3 u;
    u.load(g, q, live);
    const int p0 = blockIdx.y * TP;
    const int pend = min(p0 + TP, g.M);
    double* const col_psi = g.out + q;                      // column q of the psi block (q < Nd only)
    double* const col_phi = g.out + g.Nd + q;               // column q of the phi block
    for (int p = p0; p < pend; ++p) {
        Row3 w;
        w.load(g, p);
        if (!live) continue;
        const bool top = p < g.Nd;                          // wave-uniform: row p of the psi block exists
        double v[4];
        pair_entries(g, w, u, top, dom, v);
        if (top) {
            const long row = (long)p * g.ld;
            if (dom) col_psi[row] = v[0] + (p == q ? g.nug[0] : 0.0);
            col_phi[row] = v[1];
        }
        const long row = (long)(g.Nd + p) * g.ld;           // row p of the phi block (p < M always)
        if (dom) col_psi[row] = v[2];
        col_phi[row] = v[3] + (p == q ? g.nug[1] : 0.0);
    }
}

// Two column points per lane, one 16-byte store per (row block, column block, row point).  Needs Nd, Nb and the leading dimension
// even and a 16-byte aligned base (checked by the launcher; otherwise the one-point-per-lane kernel above runs).  The two points are
// evaluated one after the other: only the four entries of the first stay live while the second is computed.
// NT: the policy of store2 (0 plain, 1 non-temporal).
template <int NT>
__global__ __launch_bounds__(256) void assemble_op3_2_kernel(Op3Args g) {
    const int q = 2 * (blockIdx.x * 256 + threadIdx.x);
    const bool live = q < g.M;                              // (M even: q + 1 < M as well)
    const bool dom = q < g.Nd;                              // (Nd even: q and q + 1 are both inside the psi block or both outside)
    Col3 ua, ub;
    ua.load(g, q, live);
    ub.load(g, q + 1, live);
    const int p0 = blockIdx.y * TP;
    const int pend = min(p0 + TP, g.M);
    double* const col_psi = g.out + q;
    double* const col_phi = g.out + g.Nd + q;
    for (int p = p0; p < pend; ++p) {
        Row3 w;
        w.load(g, p);
        if (!live) continue;
        const bool top = p < g.Nd;                          // wave-uniform
        double va[4], vb[4];
        pair_entries(g, w, ua, top, dom, va);
        pair_entries(g, w, ub, top, dom, vb);
        if (top) {
            const long row = (long)p * g.ld;
            if (dom) store2<NT>(col_psi + row, va[0] + (p == q ? g.nug[0] : 0.0), vb[0] + (p == q + 1 ? g.nug[0] : 0.0));
            store2<NT>(col_phi + row, va[1], vb[1]);
        }
        const long row = (long)(g.Nd + p) * g.ld;
        if (dom) store2<NT>(col_psi + row, va[2], vb[2]);
        store2<NT>(col_phi + row, va[3] + (p == q ? g.nug[1] : 0.0), vb[3] + (p == q + 1 ? g.nug[1] : 0.0));
    }
}

// ---- the extension with all derivatives up to order two -----------------------------------------------------------------------------
// out[row(f)][t] = sum_q <d^MI3_f at x_t, psi_q> kappa c[q] + sum_q <d^MI3_f at x_t, phi_q> kappa c[Nd + q], f over the set bits of mask
// (the GPK_OP3FN_* bits).  Mapping as extend_fn_op_kernel: a workgroup owns FN_TT test points (wave-uniform), its 256 lanes stride over
// the column points.  Both blocks of a column point act through ONE second-order functional with the weights
// w = op3_q c[q] + (bc3_q, 0...0) c[Nd + q], formed once per column point and contracted with the Hermite tables as above; a row is
// (-1)^{|alpha_f|} C[f] kappa.  Three instantiations, not one per mask: NE = 1 (value), 4 (value and gradient), 10 (all); a request is
// served by the smallest that contains it and the rows it did not ask for are skipped at the store.  The operations behind an entry
// of C do not depend on NE, so a row has the same bits whichever other rows are requested.  Reduction by wave shuffles, then LDS across
// the 4 waves, in a fixed order (no atomics: a repeated call gives bit-identical output).

struct FnOp3Args {
    const double* s;
    int Nd, M;
    double p1, p2, p3;
    const double* tx; int Nt;             // (Nt,3) row-major test points
    const double* coeff;                  // (2 Nd + Nb): psi block, then phi block
    int mask;                             // the rows to store
    double* out; long ldo;
    __host__ __device__ const double* arr(int k) const { return s + (size_t)k * (size_t)M; }
};

template <int NE>
__global__ __launch_bounds__(256) void extend_fn_op3_kernel(FnOp3Args g) {
    const int t0 = blockIdx.x * FN_TT;
    double x1[FN_TT], x2[FN_TT], x3[FN_TT], s[FN_TT][NE];
    GPK_FN_LOAD_POINTS3(x1, x2, x3, g.tx, t0, g.Nt);
    fn_zero(s);
    for (int q = threadIdx.x; q < g.M; q += 256) {
        const double y1 = g.arr(0)[q], y2 = g.arr(1)[q], y3 = g.arr(2)[q];
        const double cl = q < g.Nd ? g.coeff[q] : 0.0;               // psi block: domain points only (psi is packed as 0 elsewhere)
        const double cd = g.coeff[g.Nd + q];                         // phi block: every point
        double w[NO];
#pragma unroll
        for (int j = 0; j < NC; ++j) w[j] = __builtin_fma(g.arr(3 + j)[q], cd, g.arr(3 + NC + j)[q] * cl);
#pragma unroll
        for (int j = NC; j < NO; ++j) w[j] = g.arr(3 + NC + j)[q] * cl;
#pragma unroll
        for (int i = 0; i < FN_TT; ++i) {
            const double d1 = x1[i] - y1, d2 = x2[i] - y2, d3 = x3[i] - y3;
            const double e = kappa3_fma(g.p1, g.p2, g.p3, d1, d2, d3);
            double a[5], b[5], c[5], t[NO];
            hermite_compensated(g.p1, d1, a);
            hermite_compensated(g.p2, d2, b);
            hermite_compensated(g.p3, d3, c);
            table_psi3<NE>(a, b, c, w, t);
#pragma unroll
            for (int f = 0; f < NE; ++f) s[i][f] = __builtin_fma((f >= 1 && f <= 3) ? -t[f] : t[f], e, s[i][f]);
        }
    }
    GPK_FN_REDUCE_STORE_MASKED(s, NE, g.mask, t0, g.Nt, g.out, g.ldo);
}

}  // namespace


extern "C" int gpk_assemble_op3d(gpk_handle h, int kernel, const double* kp, const double* Xd, int Nd, const double* Xb, int Nb,
                                 const double* op3, const double* bc3, double nugget, int nugget_type, double* Theta, int ld,
                                 double* host_ratio) {
    if (!h) return GPK_ERR_ARG;
    if (!Theta) return gpk_bad_arg(h, "assemble_op3d: Theta");
    if (!nugget_type_valid(nugget_type)) return gpk_bad_arg(h, "assemble_op3d: nugget_type");
    if ((long)2 * Nd + Nb > 0x7fffffffL) return gpk_bad_arg(h, "assemble_op3d: N exceeds int");
    if (Nd > 0 && Nb >= 0 && ld < 2 * Nd + Nb) return gpk_bad_arg(h, "assemble_op3d: ld < N");
    Op3Args g;
    double p[3];
    GPK_TRY(fill_common_op3(h, "assemble_op3d: sizes/pointers", "assemble_op3d: kernel id", kernel, kp, Xd, Nd, Xb, Nb, op3, bc3, p, &g.s));
    g.p1 = p[0]; g.p2 = p[1]; g.p3 = p[2];
    g.Nd = Nd; g.M = Nd + Nb;
    // Both traces are point sums taken on the host from the coefficient arrays, in index order and in long double, so that the
    // returned ratio is the analytic value to an ulp and the same on every call (op3 == NULL: the same sum over Laplacian rows, so
    // NULL and an explicit Laplacian give the same ratio).
    const long double q[3] = {p[0], p[1], p[2]};
    long double tr0;
    GPK_TRY(domain_trace3(h, op3, Nd, q, &tr0));
    long double trb;
    GPK_TRY(boundary_trace3(h, bc3, Nb, q, &trb));
    const double r0 = (double)(tr0 / ((long double)Nd + trb));   // trace(block 0) / trace(block 1)
    if (host_ratio) *host_ratio = r0;
    two_block_nugget(nugget_type, nugget, r0, g.nug);
    g.out = Theta; g.ld = ld;
    return launch_two_block(h, pairs_eligible(h, Theta, ld, Nd, Nb), g, assemble_op3_kernel, assemble_op3_2_kernel<0>, assemble_op3_2_kernel<1>);
}

extern "C" int gpk_extend_functionals_op3d(gpk_handle h, int kernel, const double* kp, const double* Xt, int Nt,
                                           const double* Xd, int Nd, const double* Xb, int Nb, const double* op3, const double* bc3,
                                           const double* coeff, int fmask, double* out, int ldo) {
    if (!h) return GPK_ERR_ARG;
    if (!out || !Xt || !coeff) return gpk_bad_arg(h, "extend_functionals_op3d: pointers");
    if (fmask <= 0 || fmask > 1023) return gpk_bad_arg(h, "extend_functionals_op3d: fmask must be a non-empty subset of the GPK_OP3FN_* bits");
    if (Nt <= 0) return gpk_bad_arg(h, "extend_functionals_op3d: Nt <= 0");
    if (ldo < Nt) return gpk_bad_arg(h, "extend_functionals_op3d: ldo < Nt");
    FnOp3Args g;
    double p[3];
    GPK_TRY(fill_common_op3(h, "extend_functionals_op3d: sizes/pointers", "extend_functionals_op3d: kernel id", kernel, kp, Xd, Nd, Xb, Nb,
                            op3, bc3, p, &g.s));
    g.p1 = p[0]; g.p2 = p[1]; g.p3 = p[2];
    g.Nd = Nd; g.M = Nd + Nb;
    g.tx = Xt; g.Nt = Nt; g.coeff = coeff; g.mask = fmask; g.out = out; g.ldo = ldo;
    const int grid = gpk_ceil_div(Nt, FN_TT);
    if (fmask == 1) extend_fn_op3_kernel<1><<<grid, 256, 0, h->stream>>>(g);            // value
    else if (fmask < 16) extend_fn_op3_kernel<4><<<grid, 256, 0, h->stream>>>(g);       // value and gradient
    else extend_fn_op3_kernel<NO><<<grid, 256, 0, h->stream>>>(g);                      // all ten
    GPK_LAUNCH_CHECK(h);
    return 0;
}
