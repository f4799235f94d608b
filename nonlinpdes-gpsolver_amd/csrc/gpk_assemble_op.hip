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
#include "gpk_common.h"

#include <vector>

// One-point and two-point evaluator must give the same bits for the same point pair: explicit fma, no contraction by the compiler
// (whether it contracts a * b + c depends on the uses of the product after inlining, which differ between the two).  The extension
// kernels share the pair arithmetic and are written the same way.
#pragma clang fp contract(off)

namespace {

// index in MI of the multi-index (m1, m2), m1 + m2 <= 2
__host__ __device__ constexpr int mi(int m1, int m2) { return m1 == 0 ? (m2 == 0 ? 0 : (m2 == 1 ? 2 : 5)) : (m1 == 1 ? (m2 == 0 ? 1 : 4) : 3); }
__host__ __device__ constexpr int mi_a1(int f) { return f == 1 || f == 4 ? 1 : (f == 3 ? 2 : 0); }
__host__ __device__ constexpr int mi_a2(int f) { return f == 2 || f == 4 ? 1 : (f == 5 ? 2 : 0); }

// h2 = q^2 - p and h3 = q (q^2 - 3p), q = p d, cancel near q^2 = p and q^2 = 3p; an entry here can consist of one such factor alone
// (<d11, delta'> = h2 kappa), so both brackets carry the rounding errors of q and q^2 along (explicit fma: exact error of a product),
// the compensated form of gpk_assemble_bc.hip.  h4 stays plain.
__host__ __device__ __forceinline__ void hermite(double p, double d, double (&h)[5]) {
    const double q = p * d;
    const double qe = __builtin_fma(p, d, -q);                    // p d = q + qe exactly
    const double q2 = q * q;
    const double q2e = __builtin_fma(2.0 * q, qe, __builtin_fma(q, q, -q2));   // (p d)^2 = q2 + q2e up to second order
    const double t = 3.0 * p;
    const double te = __builtin_fma(3.0, p, -t);                  // 3 p = t + te exactly
    h[0] = 1.0;
    h[1] = q;
    h[2] = (q2 - p) + q2e;
    h[3] = q * ((q2 - t) + (q2e - te));
    h[4] = __builtin_fma(q2, q2 - 6.0 * p, 3.0 * p * p);
}

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

constexpr int TP = 32;                    // row points per workgroup

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
        e = exp(-0.5 * __builtin_fma(p2 * d2, d2, p1 * d1 * d1));
        hermite(p1, d1, a);
        hermite(p2, d2, b);
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
typedef double op_d2 __attribute__((ext_vector_type(2)));

template <int NT>
__device__ __forceinline__ void store2(double* dst, double v0, double v1) {
    const op_d2 v = (op_d2){v0, v1};
    // NT (gpk_tune key 55 = 1): Theta is written once and not read by this kernel -- a non-temporal store
    if (NT) __builtin_nontemporal_store(v, reinterpret_cast<op_d2*>(dst));
    else *reinterpret_cast<op_d2*>(dst) = v;
}

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
constexpr int FN_TT = 4;                  // test points per workgroup

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

__host__ __device__ constexpr int fn_popc(int m) { return m ? (m & 1) + fn_popc(m >> 1) : 0; }
__host__ __device__ constexpr int fn_row(int mask, int f) { return fn_popc(mask & ((1 << f) - 1)); }

template <int MASK>
__global__ __launch_bounds__(256) void extend_fn_op_kernel(FnOpArgs g) {
    constexpr int NF = fn_popc(MASK);
    __shared__ double red[4][FN_TT * NF];
    const int t0 = blockIdx.x * FN_TT;
    double x1[FN_TT], x2[FN_TT];
#pragma unroll
    for (int i = 0; i < FN_TT; ++i) {                 // past the end: repeat the last point (computed, never stored)
        const int t = min(t0 + i, g.Nt - 1);
        x1[i] = g.tx[2 * t]; x2[i] = g.tx[2 * t + 1];
    }
    double s[FN_TT][NF];
#pragma unroll
    for (int i = 0; i < FN_TT; ++i)
#pragma unroll
        for (int k = 0; k < NF; ++k) s[i][k] = 0.0;
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
            hermite(g.p1, d1, a);
            hermite(g.p2, d2, b);
            table_psi<MASK>(a, b, w, c);
#pragma unroll
            for (int f = 0; f < 6; ++f)
                if ((MASK >> f) & 1) s[i][fn_row(MASK, f)] = __builtin_fma(((mi_a1(f) + mi_a2(f)) & 1) ? -c[f] : c[f], e, s[i][fn_row(MASK, f)]);
        }
    }
#pragma unroll
    for (int i = 0; i < FN_TT; ++i)
#pragma unroll
        for (int k = 0; k < NF; ++k) {
            double v = s[i][k];
            for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
            if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][i * NF + k] = v;
        }
    __syncthreads();
    if (threadIdx.x < FN_TT * NF) {
        const int i = threadIdx.x / NF, k = threadIdx.x % NF, t = t0 + i;
        if (t < g.Nt) g.out[k * g.ldo + t] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
    }
}

// one instantiation per mask (63): a functional that is not requested costs nothing
template <int MASK = 1>
void launch_extend_fn_op(int mask, int grid, hipStream_t st, const FnOpArgs& g) {
    if constexpr (MASK <= 63) {
        if (mask == MASK) extend_fn_op_kernel<MASK><<<grid, 256, 0, st>>>(g);
        else launch_extend_fn_op<MASK + 1>(mask, grid, st, g);
    }
}

// precisions, packed points and coefficients (the handle's point scratch: 11 arrays of Nd + Nb, re-packed by every call)
int fill_common_op(gpk_handle h, const char* who, const char* who_kernel, int kernel, const double* kp, const double* Xd, int Nd,
                   const double* Xb, int Nb, const double* op, const double* bc, double (&p)[2], const double* (&arr)[11]) {
    if (Nd <= 0 || Nb < 0 || !kp || !Xd || (Nb > 0 && !Xb)) return gpk_bad_arg(h, who);
    if (kernel == GPK_KERNEL_GAUSSIAN) { p[0] = p[1] = 1.0 / (kp[0] * kp[0]); }
    else if (kernel == GPK_KERNEL_ANISOTROPIC) { p[0] = 2.0 / (kp[0] * kp[0]); p[1] = 2.0 / (kp[1] * kp[1]); }   // no factor 1/2: the reference's convention
    else return gpk_bad_arg(h, who_kernel);
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
    if (nugget_type != GPK_NUGGET_NONE && nugget_type != GPK_NUGGET_IDENTITY && nugget_type != GPK_NUGGET_ADAPTIVE)
        return gpk_bad_arg(h, "assemble_op: nugget_type");
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
    long double tr0, tr1 = (long double)Nd;
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
    if (bc && Nb > 0) {
        std::vector<double> hb(3 * (size_t)Nb);
        GPK_HIP(h, hipMemcpyAsync(hb.data(), bc, hb.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        GPK_HIP(h, hipStreamSynchronize(h->stream));
        long double sb = 0.0L;
        for (int b = 0; b < Nb; ++b) {
            const long double b0 = hb[3 * (size_t)b], b1 = hb[3 * (size_t)b + 1], b2 = hb[3 * (size_t)b + 2];
            sb += b0 * b0 + q1 * b1 * b1 + q2 * b2 * b2;
        }
        tr1 += sb;
    } else {
        tr1 += (long double)Nb;
    }
    const double r0 = (double)(tr0 / tr1);                       // trace(block 0) / trace(block 1)
    if (host_ratio) *host_ratio = r0;
    g.nug[0] = nugget_type == GPK_NUGGET_ADAPTIVE ? nugget * r0 : (nugget_type == GPK_NUGGET_IDENTITY ? nugget : 0.0);
    g.nug[1] = nugget_type == GPK_NUGGET_NONE ? 0.0 : nugget;
    g.out = Theta; g.ld = ld;
    // two column points per lane (16-byte stores) when every pair (q, q + 1) stays inside one block and is 16-byte aligned
    const bool pairs = h->tune.asm_pairs && (ld % 2 == 0) && (((uintptr_t)Theta & 15) == 0) && (Nd % 2 == 0) && (Nb % 2 == 0);
    // (per-phase timing on: HIP events around the evaluator launch alone, as in gpk_assemble -- gpk_prof_read_assembly reads them)
    if (h->prof) {
        if (!h->asm_ev[0]) for (int i = 0; i < 2; ++i) GPK_HIP(h, hipEventCreate(&h->asm_ev[i]));
        GPK_HIP(h, hipEventRecord(h->asm_ev[0], h->stream));
    }
    struct AsmStop {
        gpk_handle h; ~AsmStop() { if (h->prof && h->asm_ev[1]) h->asm_timed = hipEventRecord(h->asm_ev[1], h->stream) == hipSuccess; }
    } asm_stop{h};
    if (pairs) {
        dim3 grid2(gpk_ceil_div(g.M / 2, 256), gpk_ceil_div(g.M, TP));
        // key 55: 0 plain, 1 non-temporal (the write-through variants 2 / 3 of gpk_assemble are not offered here: plain)
        if (h->tune.asm_nt == 1) assemble_op2_kernel<1><<<grid2, 256, 0, h->stream>>>(g);
        else assemble_op2_kernel<0><<<grid2, 256, 0, h->stream>>>(g);
    } else {
        dim3 grid(gpk_ceil_div(g.M, 256), gpk_ceil_div(g.M, TP));
        assemble_op_kernel<<<grid, 256, 0, h->stream>>>(g);
    }
    GPK_LAUNCH_CHECK(h);
    return 0;
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
    launch_extend_fn_op<>(fmask, gpk_ceil_div(Nt, FN_TT), h->stream, g);
    GPK_LAUNCH_CHECK(h);
    return 0;
}
