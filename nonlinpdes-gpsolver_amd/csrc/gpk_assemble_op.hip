// gpk_assemble_op.hip -- the fused derivative-kernel evaluator of the 2-D elliptic layout with a second-order linear functional at every
// domain point (variable-coefficient diffusion, advection, reaction) and a first-order one at every boundary point: the Gram matrix and
// the matrix-free extension with all derivatives up to order two.
//
// No reference call site: the reference's Gram_matrix_assembly (src/Gram_matrice.py) knows the Laplacian only.  The elliptic
// Gauss-Newton system sees block 0 through sol_vec = [alpha z^m - f, z, g] alone, so any linear functional psi at the domain points with
// psi[u] = alpha u^m - f reuses the factorisation, gpk_gn_step, gpk_potrs and gpk_pde_residual unchanged; the point-pair evaluator
// below is all a solve of -psi[u] + alpha u^m = f needs (src/PDEs.py, Nonlinear_elliptic2d(operator=...)).
//
// Math (DESIGN.md §K "Variable-coefficient operator").  Multi-indices MI = {(0,0),(1,0),(0,1),(2,0),(1,1),(0,2)}.  Domain point i
// carries psi_i = sum_j op[i][j] d^MI_j in block 0 and delta in block 1; boundary point b carries phi_b = bc[b][0] delta + bc[b][1] d_1
// + bc[b][2] d_2 in block 1.  With d = x - y, d_x^alpha d_y^beta kappa = (-1)^{|alpha|} h_{a1+b1}(p1,d1) h_{a2+b2}(p2,d2) kappa:
//   <F, G'> = sum_i r_i (-1)^{|alpha_i|} C[alpha_i],   C[m1][m2] = sum_j k_j h_{m1+b1_j}(p1,d1) h_{m2+b2_j}(p2,d2)
// r the coefficients of the row functional (at x), k those of the column functional (at y).  The column's coefficients are contracted
// with the Hermite tables first, per axis (C: the six entries m1 + m2 <= 2 of a 3 x 3 table, 36 operations for psi', 21 for phi'), then
// the rows with C (6 or 3 operations per entry): ~95 operations for the four entries of a point pair instead of 81 separate term
// evaluations.  Per-axis order <= 2 + 2: h0..h4 suffice, and one exp and one pair of Hermite evaluations per POINT PAIR feed all blocks.
//
// Mapping to the hardware, as assemble_bc_kernel / assemble_bc2_kernel: SoA-packed points and coefficients in the handle's point
// scratch (2 + 3 + 6 arrays of Nd+Nb), a workgroup owns TP row points x 256 column points (two-point variant: x 512), lane <-> column
// point (its coordinates and nine coefficients stay in registers), the row point and its coefficients are wave-uniform (scalar loads).
//
// Shared with the other evaluators (gpk_assemble_common.h): hermite_compensated and kappa2_fma (with gpk_assemble_bc.hip: the same
// bits there), the frame of the extension kernel, store2 and the host side of a call (precisions, nugget, boundary trace, timing,
// launch).
#include "gpk_assemble_common.h"

using namespace gpk_asm;

// One-point and two-point evaluator must give the same bits for the same point pair: explicit fma, no contraction by the compiler
// (whether it contracts a * b + c depends on the uses of the product after inlining, which differ between the two).  The extension
// kernels share the pair arithmetic and are written the same way.
#pragma clang fp contract(off)

namespace {

// index in MI of the multi-index (m1, m2), m1 + m2 <= 2
__host__ __device__ constexpr int mi(int m1, int m2) { return m1 == 0 ? (m2 == 0 ? 0 : (m2 == 1 ? 2 : 5)) : (m1 == 1 ? (m2 == 0 ? 1 : 4) : 3); }
__host__ __device__ constexpr int mi_a1(int f) { return f == 1 || f == 4 ? 1 : (f == 3 ? 2 : 0); }
__host__ __device__ constexpr int mi_a2(int f) { return f == 2 || f == 4 ? 1 : (f == 5 ? 2 : 0); }

// C[mi(m1,m2)] = sum_j k_j a[m1 + b1_j] b[m2 + b2_j] for the second-order column functional k (MI order), axis 1 first:
//   A0[m1] = k0 a[m1] + k1 a[m1+1] + k3 a[m1+2]   (the parts without d_2),  A1[m1] = k2 a[m1] + k4 a[m1+1]  (d_2),  A2[m1] = k5 a[m1]  (d_22)
// MASK: the entries wanted (bit f = entry f); the others are not computed.
template <int MASK = 63>
__host__ __device__ __forceinline__ void table_psi(const double (&a)[5], const double (&b)[5], const double (&k)[6], double (&c)[6]) {
#pragma unroll
    for (int m1 = 0; m1 < 3; ++m1) {
        const double A0 = __builtin_fma(k[3], a[m1 + 2], __builtin_fma(k[1], a[m1 + 1], k[0] * a[m1]));
        const double A1 = __builtin_fma(k[4], a[m1 + 1], k[2] * a[m1]);
        const double A2 = k[5] * a[m1];
#pragma unroll
        for (int m2 = 0; m1 + m2 < 3; ++m2)
            if ((MASK >> mi(m1, m2)) & 1) c[mi(m1, m2)] = __builtin_fma(b[m2 + 2], A2, __builtin_fma(b[m2 + 1], A1, b[m2] * A0));
    }
}

// the same for the first-order column functional k = (c0, c1, c2)
__host__ __device__ __forceinline__ void table_phi(const double (&a)[5], const double (&b)[5], const double (&k)[3], double (&c)[6]) {
#pragma unroll
    for (int m1 = 0; m1 < 3; ++m1) {
        const double A0 = __builtin_fma(k[1], a[m1 + 1], k[0] * a[m1]);
        const double A1 = k[2] * a[m1];
#pragma unroll
        for (int m2 = 0; m1 + m2 < 3; ++m2) c[mi(m1, m2)] = __builtin_fma(b[m2 + 1], A1, b[m2] * A0);
    }
}

// sum_i r_i (-1)^{|alpha_i|} C[alpha_i]: the odd row functionals d_1, d_2 enter with a minus sign (exact)
template <int NR>
__host__ __device__ __forceinline__ double row_phi(const double (&c)[6], const double (&r)[NR]) {
    return __builtin_fma(-r[2], c[2], __builtin_fma(-r[1], c[1], r[0] * c[0]));
}

__host__ __device__ __forceinline__ double row_psi(const double (&c)[6], const double (&r)[6]) {
    return __builtin_fma(r[5], c[5], __builtin_fma(r[4], c[4], __builtin_fma(r[3], c[3], row_phi(c, r))));
}

struct OpArgs {
    const double* px; const double* py;                     // SoA points: domain first, then boundary
    const double* c[3];                                     // SoA coefficients of phi, same order ((1,0,0) at the domain points)
    const double* o[6];                                     // SoA coefficients of psi (zero at the boundary points)
    int Nd, M;                                              // M = Nd + Nb
    double p1, p2;
    double* out; long ld;
    double nug[2];
};

// domain point i: phi = (1,0,0), psi = op[6i..6i+5] or the Laplacian (0,0,0,1,0,1) when op == NULL; boundary point b: phi = bc[3b..3b+2]
// or (1,0,0) when bc == NULL, psi = 0 (never used)
__global__ void pack_op_kernel(const double* __restrict__ Xd, int Nd, const double* __restrict__ Xb, int Nb, const double* __restrict__ op,
                               const double* __restrict__ bc, double* __restrict__ s) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t M = (size_t)Nd + (size_t)Nb;
    if (i < Nd) {
        s[i] = Xd[2 * i]; s[M + i] = Xd[2 * i + 1];
        s[2 * M + i] = 1.0; s[3 * M + i] = 0.0; s[4 * M + i] = 0.0;
#pragma unroll
        for (int j = 0; j < 6; ++j) s[(5 + j) * M + i] = op ? op[6 * (size_t)i + j] : ((j == 3 || j == 5) ? 1.0 : 0.0);
    } else if (i < Nd + Nb) {
        const int b = i - Nd;
        s[i] = Xb[2 * b]; s[M + i] = Xb[2 * b + 1];
#pragma unroll
        for (int j = 0; j < 3; ++j) s[(2 + j) * M + i] = bc ? bc[3 * (size_t)b + j] : (j == 0 ? 1.0 : 0.0);
#pragma unroll
        for (int j = 0; j < 6; ++j) s[(5 + j) * M + i] = 0.0;
    }
}

// everything one point pair contributes: d = x - y, column coefficients k (phi') and ko (psi', domain columns only)
struct PairOp {
    double cf[6], cp[6], e;               // tables of phi' and of psi' (cp: set when the column is a domain point)
    __device__ __forceinline__ void eval(double p1, double p2, double d1, double d2, const double (&k)[3], const double (&ko)[6], bool dom) {
        double a[5], b[5];
        e = kappa2_fma(p1, p2, d1, d2);
        hermite_compensated(p1, d1, a);
        hermite_compensated(p2, d2, b);
        table_phi(a, b, k, cf);
        if (dom) table_psi<>(a, b, ko, cp);
    }
    __device__ __forceinline__ double psi_psi(const double (&ro)[6]) const { return row_psi(cp, ro) * e; }
    __device__ __forceinline__ double psi_phi(const double (&ro)[6]) const { return row_psi(cf, ro) * e; }
    __device__ __forceinline__ double phi_psi(const double (&r)[3]) const { return row_phi(cp, r) * e; }
    __device__ __forceinline__ double phi_phi(const double (&r)[3]) const { return row_phi(cf, r) * e; }
};

// one column point per lane, 8-byte stores: any alignment, any Nd / Nb
__global__ __launch_bounds__(256) void assemble_op_kernel(OpArgs g) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    const bool live = q < g.M;
    const bool dom = q < g.Nd;
    const double y1 = live ? g.px[q] : 0.0, y2 = live ? g.py[q] : 0.0;
    double k[3], ko[6];
#pragma unroll
    for (int j = 0; j < 3; ++j) k[j] = live ? g.c[j][q] : 0.0;
#pragma unroll
    for (int j = 0; j < 6; ++j) ko[j] = live ? g.o[j][q] : 0.0;
    const int p0 = blockIdx.y * TP;
    const int pend = min(p0 + TP, g.M);
    double* const col_psi = g.out + q;                      // column q of the psi block (q < Nd only)
    double* const col_phi = g.out + g.Nd + q;               // column q of the phi block
    for (int p = p0; p < pend; ++p) {
        const double x1 = g.px[p], x2 = g.py[p];            // uniform address -> scalar loads
        const double r[3] = {g.c[0][p], g.c[1][p], g.c[2][p]};
        const double ro[6] = {g.o[0][p], g.o[1][p], g.o[2][p], g.o[3][p], g.o[4][p], g.o[5][p]};
        if (!live) continue;
        PairOp u;
        u.eval(g.p1, g.p2, x1 - y1, x2 - y2, k, ko, dom);
        if (p < g.Nd) {                                     // wave-uniform: row p of the psi block
            const long row = (long)p * g.ld;
            if (dom) col_psi[row] = u.psi_psi(ro) + (p == q ? g.nug[0] : 0.0);
            col_phi[row] = u.psi_phi(ro);
        }
        const long row = (long)(g.Nd + p) * g.ld;           // row p of the phi block (p < M always)
        if (dom) col_psi[row] = u.phi_psi(r);
        col_phi[row] = u.phi_phi(r) + (p == q ? g.nug[1] : 0.0);
    }
}

// Two column points per lane, one 16-byte store per (row block, column block, row point).  Needs Nd, Nb and the leading dimension
// even and a 16-byte aligned base (checked by the launcher; otherwise the one-point-per-lane kernel above runs).
// NT: the policy of store2 (0 plain, 1 non-temporal).

template <int NT>
__global__ __launch_bounds__(256) void assemble_op2_kernel(OpArgs g) {
    const int q = 2 * (blockIdx.x * 256 + threadIdx.x);
    const bool live = q < g.M;                              // (M even: q + 1 < M as well)
    const bool dom = q < g.Nd;                              // (Nd even: q and q + 1 are both inside the psi block or both outside)
    const double y1a = live ? g.px[q] : 0.0, y2a = live ? g.py[q] : 0.0;
    const double y1b = live ? g.px[q + 1] : 0.0, y2b = live ? g.py[q + 1] : 0.0;
    double ka[3], kb[3], koa[6], kob[6];
#pragma unroll
    for (int j = 0; j < 3; ++j) { ka[j] = live ? g.c[j][q] : 0.0; kb[j] = live ? g.c[j][q + 1] : 0.0; }
#pragma unroll
    for (int j = 0; j < 6; ++j) { koa[j] = live ? g.o[j][q] : 0.0; kob[j] = live ? g.o[j][q + 1] : 0.0; }
    const int p0 = blockIdx.y * TP;
    const int pend = min(p0 + TP, g.M);
    double* const col_psi = g.out + q;
    double* const col_phi = g.out + g.Nd + q;
    for (int p = p0; p < pend; ++p) {
        const double x1 = g.px[p], x2 = g.py[p];            // uniform address -> scalar loads
        const double r[3] = {g.c[0][p], g.c[1][p], g.c[2][p]};
        const double ro[6] = {g.o[0][p], g.o[1][p], g.o[2][p], g.o[3][p], g.o[4][p], g.o[5][p]};
        if (!live) continue;
        PairOp u0, u1;
        u0.eval(g.p1, g.p2, x1 - y1a, x2 - y2a, ka, koa, dom);
        u1.eval(g.p1, g.p2, x1 - y1b, x2 - y2b, kb, kob, dom);
        if (p < g.Nd) {                                     // wave-uniform
            const long row = (long)p * g.ld;
            if (dom) store2<NT>(col_psi + row, u0.psi_psi(ro) + (p == q ? g.nug[0] : 0.0), u1.psi_psi(ro) + (p == q + 1 ? g.nug[0] : 0.0));
            store2<NT>(col_phi + row, u0.psi_phi(ro), u1.psi_phi(ro));
        }
        const long row = (long)(g.Nd + p) * g.ld;
        if (dom) store2<NT>(col_psi + row, u0.phi_psi(r), u1.phi_psi(r));
        store2<NT>(col_phi + row, u0.phi_phi(r) + (p == q ? g.nug[1] : 0.0), u1.phi_phi(r) + (p == q + 1 ? g.nug[1] : 0.0));
    }
}

// ---- the extension with all derivatives up to order two (DESIGN.md §K "Variable-coefficient operator") ------------------------------
// out[f][t] = sum_q <d^MI_f at x_t, psi_q> kappa c[q] + sum_q <d^MI_f at x_t, phi_q> kappa c[Nd + q], f over the set bits of MASK (the
// GPK_OPFN_* bits).  Mapping as extend_fn_bc_kernel: a workgroup owns FN_TT test points (wave-uniform), its 256 lanes stride over the
// column points.  Both blocks of a column point act through ONE second-order functional with the weights
// w = op_q c[q] + (bc_q, 0, 0, 0) c[Nd + q], formed once per column point and contracted with the Hermite tables as above; a row is
// (-1)^{|alpha_f|} C[f] kappa, the same operations whichever other rows are requested.  Each lane keeps FN_TT x popcount(MASK)
// accumulators.  Reduction by wave shuffles, then LDS across the 4 waves, in a fixed order (no atomics: a repeated call gives
// bit-identical output).

struct FnOpArgs {
    const double* px; const double* py;
    const double* c[3];
    const double* o[6];
    int Nd, M;
    double p1, p2;
    const double* tx; int Nt;             // (Nt,2) row-major test points
    const double* coeff;                  // (2 Nd + Nb): psi block, then phi block
    double* out; long ldo;
};

template <int MASK>
__global__ __launch_bounds__(256) void extend_fn_op_kernel(FnOpArgs g) {
    constexpr int NF = fn_popc(MASK);
    const int t0 = blockIdx.x * FN_TT;
    double x1[FN_TT], x2[FN_TT], s[FN_TT][NF];
    GPK_FN_LOAD_POINTS2(x1, x2, g.tx, t0, g.Nt);
    fn_zero(s);
    for (int q = threadIdx.x; q < g.M; q += 256) {
        const double y1 = g.px[q], y2 = g.py[q];
        const double cl = q < g.Nd ? g.coeff[q] : 0.0;               // psi block: domain points only (psi is packed as 0 elsewhere)
        const double cd = g.coeff[g.Nd + q];                         // phi block: every point
        double w[6];
#pragma unroll
        for (int j = 0; j < 3; ++j) w[j] = __builtin_fma(g.c[j][q], cd, g.o[j][q] * cl);
#pragma unroll
        for (int j = 3; j < 6; ++j) w[j] = g.o[j][q] * cl;
#pragma unroll
        for (int i = 0; i < FN_TT; ++i) {
            const double d1 = x1[i] - y1, d2 = x2[i] - y2;
            const double e = exp(-0.5 * __builtin_fma(g.p2 * d2, d2, g.p1 * d1 * d1));
            double a[5], b[5], c[6];
            hermite_compensated(g.p1, d1, a);
            hermite_compensated(g.p2, d2, b);
            table_psi<MASK>(a, b, w, c);
#pragma unroll
            for (int f = 0; f < 6; ++f)
                if ((MASK >> f) & 1) s[i][fn_row(MASK, f)] = __builtin_fma(((mi_a1(f) + mi_a2(f)) & 1) ? -c[f] : c[f], e, s[i][fn_row(MASK, f)]);
        }
    }
    GPK_FN_REDUCE_STORE(s, NF, t0, g.Nt, g.out, g.ldo);
}

// one instantiation per mask (63)
void launch_extend_fn_op(int mask, int grid, hipStream_t st, const FnOpArgs& g) {
    with_mask<63>(mask, [&](auto m) { extend_fn_op_kernel<decltype(m)::value><<<grid, 256, 0, st>>>(g); });
}

// precisions, packed points and coefficients (the handle's point scratch: 11 arrays of Nd + Nb, re-packed by every call)
int fill_common_op(gpk_handle h, const char* who, const char* who_kernel, int kernel, const double* kp, const double* Xd, int Nd,
                   const double* Xb, int Nb, const double* op, const double* bc, double (&p)[2], const double* (&arr)[11]) {
    if (Nd <= 0 || Nb < 0 || !kp || !Xd || (Nb > 0 && !Xb)) return gpk_bad_arg(h, who);
    GPK_TRY(precisions(h, who_kernel, kernel, kp, 2, p));
    const size_t Mall = (size_t)Nd + (size_t)Nb;
    GPK_TRY(gpk_i_ensure_points(h, 11 * Mall));
    double* s = h->d_pts;
    for (int k = 0; k < 11; ++k) arr[k] = s + k * Mall;
    pack_op_kernel<<<gpk_ceil_div((int)Mall, 256), 256, 0, h->stream>>>(Xd, Nd, Xb, Nb, op, bc, s);
    GPK_LAUNCH_CHECK(h);
    return 0;
}

template <class Args>
void set_arrays(Args& g, const double* (&arr)[11]) {
    g.px = arr[0]; g.py = arr[1];
    for (int j = 0; j < 3; ++j) g.c[j] = arr[2 + j];
    for (int j = 0; j < 6; ++j) g.o[j] = arr[5 + j];
}

}  // namespace


extern "C" int gpk_assemble_op(gpk_handle h, int kernel, const double* kp, const double* Xd, int Nd, const double* Xb, int Nb,
                               const double* op, const double* bc, double nugget, int nugget_type, double* Theta, int ld,
                               double* host_ratio) {
    if (!h || !Theta) return GPK_ERR_ARG;
    if (!nugget_type_valid(nugget_type)) return gpk_bad_arg(h, "assemble_op: nugget_type");
    if ((long)2 * Nd + Nb > 0x7fffffffL) return gpk_bad_arg(h, "assemble_op: N exceeds int");
    if (Nd > 0 && Nb >= 0 && ld < 2 * Nd + Nb) return gpk_bad_arg(h, "assemble_op: ld < N");
    OpArgs g;
    double p[2];
    const double* arr[11];
    GPK_TRY(fill_common_op(h, "assemble_op: sizes/pointers", "assemble_op: kernel id", kernel, kp, Xd, Nd, Xb, Nb, op, bc, p, arr));
    set_arrays(g, arr);
    g.p1 = p[0]; g.p2 = p[1];
    g.Nd = Nd; g.M = Nd + Nb;
    // values at d = 0 (h0 = 1, h2 = -p, h4 = 3 p^2, odd orders vanish):
    //   <psi, psi> = c0^2 + p1 b1^2 + p2 b2^2 + 3 p1^2 a11^2 + 3 p2^2 a22^2 + p1 p2 (a12^2 + 2 a11 a22) - 2 c0 (p1 a11 + p2 a22)
    //   <phi, phi> = c0^2 + p1 c1^2 + p2 c2^2 (1 at a domain point)
    // Both traces are point sums taken on the host from the coefficient arrays, in index order and in long double, so that the
    // returned ratio is the analytic value to an ulp and the same on every call.
    const long double q1 = p[0], q2 = p[1];
    long double tr0;
    if (op) {
        std::vector<double> ho(6 * (size_t)Nd);
        GPK_HIP(h, hipMemcpyAsync(ho.data(), op, ho.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        GPK_HIP(h, hipStreamSynchronize(h->stream));
        tr0 = 0.0L;
        for (int i = 0; i < Nd; ++i) {
            const double* o = ho.data() + 6 * (size_t)i;
            const long double c0 = o[0], b1 = o[1], b2 = o[2], a11 = o[3], a12 = o[4], a22 = o[5];
            tr0 += c0 * c0 + q1 * b1 * b1 + q2 * b2 * b2 + 3.0L * q1 * q1 * a11 * a11 + 3.0L * q2 * q2 * a22 * a22
                   + q1 * q2 * (a12 * a12 + 2.0L * a11 * a22) - 2.0L * c0 * (q1 * a11 + q2 * a22);
        }
    } else {
        tr0 = (long double)Nd * (3.0L * (q1 * q1 + q2 * q2) + 2.0L * q1 * q2);
    }
    long double trb;
    GPK_TRY(boundary_trace(h, bc, Nb, q1, q2, &trb));
    const double r0 = (double)(tr0 / ((long double)Nd + trb));   // trace(block 0) / trace(block 1)
    if (host_ratio) *host_ratio = r0;
    two_block_nugget(nugget_type, nugget, r0, g.nug);
    g.out = Theta; g.ld = ld;
    return launch_two_block(h, pairs_eligible(h, Theta, ld, Nd, Nb), g, assemble_op_kernel, assemble_op2_kernel<0>, assemble_op2_kernel<1>);
}

extern "C" int gpk_extend_functionals_op(gpk_handle h, int kernel, const double* kp, const double* Xt, int Nt,
                                         const double* Xd, int Nd, const double* Xb, int Nb, const double* op, const double* bc,
                                         const double* coeff, int fmask, double* out, int ldo) {
    if (!h) return GPK_ERR_ARG;
    if (!out || !Xt || !coeff) return gpk_bad_arg(h, "extend_functionals_op: pointers");
    if (fmask <= 0 || fmask > 63) return gpk_bad_arg(h, "extend_functionals_op: fmask must be a non-empty subset of the GPK_OPFN_* bits");
    if (Nt <= 0) return gpk_bad_arg(h, "extend_functionals_op: Nt <= 0");
    if (ldo < Nt) return gpk_bad_arg(h, "extend_functionals_op: ldo < Nt");
    FnOpArgs g;
    double p[2];
    const double* arr[11];
    GPK_TRY(fill_common_op(h, "extend_functionals_op: sizes/pointers", "extend_functionals_op: kernel id", kernel, kp, Xd, Nd, Xb, Nb,
                           op, bc, p, arr));
    set_arrays(g, arr);
    g.p1 = p[0]; g.p2 = p[1];
    g.Nd = Nd; g.M = Nd + Nb;
    g.tx = Xt; g.Nt = Nt; g.coeff = coeff; g.out = out; g.ldo = ldo;
    launch_extend_fn_op(fmask, gpk_ceil_div(Nt, FN_TT), h->stream, g);
    GPK_LAUNCH_CHECK(h);
    return 0;
}
