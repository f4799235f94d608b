// gpk_assemble.hip -- fused derivative-kernel Gram block evaluator (HBM-write bound).
//
// Replaces Gram_matrix_assembly / construct_Theta_test (reference src/Gram_matrice.py:11-289) and the nugget of
// *.Gram_matrix (src/PDEs.py:56-73,250-269,391-409; src/InverseProblems.py:66-99).
//
// Math.  kappa = exp(-(p1 d1^2 + p2 d2^2)/2), d = x - y.  With the 1-D Hermite factors
//   h0 = 1, h1 = p d, h2 = p^2 d^2 - p, h3 = p^3 d^3 - 3 p^2 d, h4 = p^4 d^4 - 6 p^3 d^2 + 3 p^2
// every mixed partial is  d_x^alpha d_y^beta kappa = (-1)^{|alpha|} h_{a1+b1}(p1,d1) h_{a2+b2}(p2,d2) kappa.
// A Theta entry is <row functional, column functional> where a functional is a short list of multi-indices
// (delta, d1, d2, d2^2, Laplacian).  One exp per POINT PAIR feeds every block that pair contributes to
// (up to 16 entries), instead of one autodiff'd exp per entry per block as in the reference.
//
// Mapping to the hardware: a workgroup owns TP row points x 256 column points.  Lane <-> column point, so for a
// fixed (row functional, column functional, row point) the 64 lanes of a wave store 512 contiguous bytes; the row
// point is wave-uniform (scalar loads, no LDS needed: 16 B per point).  No symmetry trick: the ALU cost per pair
// (~1 exp + ~60 flops) is >10x below the HBM write time of its 32..128 output bytes.
//
// The functional tables, the Hermite evaluation (hermite_plain), the frame of the extension kernel, the 16-byte store and the host side
// of a call (precisions, nugget, timing) are shared with the other evaluators: gpk_assemble_common.h.  The layouts, the argument structs and
// the layout dispatch are shared with the Matern family and the periodic kernel of these layouts (gpk_assemble_matern.hip, gpk_assemble_periodic.hip, launched from the entry points below): gpk_assemble_ref.h.
#include "gpk_assemble_ref.h"

using namespace gpk_asm;

namespace {

// plain accumulation: the compiler may contract (gpk_assemble_bc.hip has the explicit-fma form, which rounds differently on purpose)
template <int FX, int FY>
__host__ __device__ __forceinline__ double pair_coeff(const double (&a)[5], const double (&b)[5]) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < f_count(FX); ++i) {
#pragma unroll
        for (int j = 0; j < f_count(FY); ++j) {
            const int n1 = f_a1(FX, i) + f_a1(FY, j);
            const int n2 = f_a2(FX, i) + f_a2(FY, j);
            const double t = a[n1] * b[n2];
            if ((f_a1(FX, i) + f_a2(FX, i)) & 1) s -= t; else s += t;
        }
    }
    return s;
}

__global__ void pack_points_kernel(const double* __restrict__ Xd, int Nd, const double* __restrict__ Xb, int Nb,
                                   double* __restrict__ px, double* __restrict__ py) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < Nd) { px[i] = Xd[2 * i]; py[i] = Xd[2 * i + 1]; }
    else if (i < Nd + Nb) { px[i] = Xb[2 * (i - Nd)]; py[i] = Xb[2 * (i - Nd) + 1]; }
}

template <int L, int BI, int BJ>
__device__ __forceinline__ void store_block(const AsmArgs& g, int p, int q, const double (&a)[5], const double (&b)[5], double e) {
    if (q < g.size[BJ]) {
        double v = pair_coeff<Lay<L>::f[BI], Lay<L>::f[BJ]>(a, b) * e;
        if (BI == BJ && p == q) v += g.nug[BI];
        g.out[(long)(g.off[BI] + p) * g.ld + g.off[BJ] + q] = v;
    }
}

template <int L, int BI>
__device__ __forceinline__ void store_row(const AsmArgs& g, int p, int q, const double (&a)[5], const double (&b)[5], double e) {
    if (p < g.size[BI]) {                               // wave-uniform
        store_block<L, BI, 0>(g, p, q, a, b, e);
        if (Lay<L>::nb > 1) store_block<L, BI, 1>(g, p, q, a, b, e);
        if (Lay<L>::nb > 2) store_block<L, BI, 2>(g, p, q, a, b, e);
        if (Lay<L>::nb > 3) store_block<L, BI, 3>(g, p, q, a, b, e);
    }
}

// Two column points per lane, one 16-byte store per (row functional, column functional, row point): a wave writes 1 KB contiguous
// per store instruction and issues half as many of them.  Needs every block offset, the leading dimension and the base address to
// be even multiples of 8 bytes (checked by the launcher; otherwise the one-point-per-lane kernel below runs).  NT: the store policy of
// store2 (gpk_tune key 55; all four are instantiated here, see the table at gpk_assemble below).

template <int L, int BI, int BJ, int NT>
__device__ __forceinline__ void store_block2(const AsmArgs& g, int p, int q, const double (&a0)[5], const double (&b0)[5], double e0,
                                             const double (&a1)[5], const double (&b1)[5], double e1) {
    if (q < g.size[BJ]) {                                            // (sizes are even here: q and q + 1 are both inside or both outside)
        double v0 = pair_coeff<Lay<L>::f[BI], Lay<L>::f[BJ]>(a0, b0) * e0;
        double v1 = pair_coeff<Lay<L>::f[BI], Lay<L>::f[BJ]>(a1, b1) * e1;
        if (BI == BJ) { if (p == q) v0 += g.nug[BI]; if (p == q + 1) v1 += g.nug[BI]; }
        store2<NT>(g.out + (long)(g.off[BI] + p) * g.ld + g.off[BJ] + q, v0, v1);
    }
}

template <int L, int BI, int NT>
__device__ __forceinline__ void store_row2(const AsmArgs& g, int p, int q, const double (&a0)[5], const double (&b0)[5], double e0,
                                           const double (&a1)[5], const double (&b1)[5], double e1) {
    if (p < g.size[BI]) {                               // wave-uniform
        store_block2<L, BI, 0, NT>(g, p, q, a0, b0, e0, a1, b1, e1);
        if (Lay<L>::nb > 1) store_block2<L, BI, 1, NT>(g, p, q, a0, b0, e0, a1, b1, e1);
        if (Lay<L>::nb > 2) store_block2<L, BI, 2, NT>(g, p, q, a0, b0, e0, a1, b1, e1);
        if (Lay<L>::nb > 3) store_block2<L, BI, 3, NT>(g, p, q, a0, b0, e0, a1, b1, e1);
    }
}

template <int L, int NT>
__global__ __launch_bounds__(256) void assemble2_kernel(AsmArgs g) {
    const int q = 2 * (blockIdx.x * 256 + threadIdx.x);
    const bool live = q < g.M;                                       // (M even: q + 1 < M as well)
    const double y1a = live ? g.px[q] : 0.0, y2a = live ? g.py[q] : 0.0;
    const double y1b = live ? g.px[q + 1] : 0.0, y2b = live ? g.py[q + 1] : 0.0;
    const int p0 = blockIdx.y * TP;
    const int pend = min(p0 + TP, g.M);
    for (int p = p0; p < pend; ++p) {
        const double x1 = g.px[p], x2 = g.py[p];        // uniform address -> scalar loads
        if (!live) continue;
        const double d1a = x1 - y1a, d2a = x2 - y2a, d1b = x1 - y1b, d2b = x2 - y2b;
        const double e0 = exp(-0.5 * (g.p1 * d1a * d1a + g.p2 * d2a * d2a));
        const double e1 = exp(-0.5 * (g.p1 * d1b * d1b + g.p2 * d2b * d2b));
        double a0[5], b0[5], a1[5], b1[5];
        hermite_plain(g.p1, d1a, a0); hermite_plain(g.p2, d2a, b0);
        hermite_plain(g.p1, d1b, a1); hermite_plain(g.p2, d2b, b1);
        store_row2<L, 0, NT>(g, p, q, a0, b0, e0, a1, b1, e1);
        if (Lay<L>::nb > 1) store_row2<L, 1, NT>(g, p, q, a0, b0, e0, a1, b1, e1);
        if (Lay<L>::nb > 2) store_row2<L, 2, NT>(g, p, q, a0, b0, e0, a1, b1, e1);
        if (Lay<L>::nb > 3) store_row2<L, 3, NT>(g, p, q, a0, b0, e0, a1, b1, e1);
    }
}

template <int L>
__global__ __launch_bounds__(256) void assemble_kernel(AsmArgs g) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    const bool live = q < g.M;
    const double y1 = live ? g.px[q] : 0.0, y2 = live ? g.py[q] : 0.0;
    const int p0 = blockIdx.y * TP;
    const int pend = min(p0 + TP, g.M);
    for (int p = p0; p < pend; ++p) {
        const double x1 = g.px[p], x2 = g.py[p];        // uniform address -> scalar loads
        if (!live) continue;
        const double d1 = x1 - y1, d2 = x2 - y2;
        const double e = exp(-0.5 * (g.p1 * d1 * d1 + g.p2 * d2 * d2));
        double a[5], b[5];
        hermite_plain(g.p1, d1, a);
        hermite_plain(g.p2, d2, b);
        store_row<L, 0>(g, p, q, a, b, e);
        if (Lay<L>::nb > 1) store_row<L, 1>(g, p, q, a, b, e);
        if (Lay<L>::nb > 2) store_row<L, 2>(g, p, q, a, b, e);
        if (Lay<L>::nb > 3) store_row<L, 3>(g, p, q, a, b, e);
    }
}

// test rows: functional delta at the test point, column functionals of the layout
template <int L, int BJ>
__device__ __forceinline__ void store_test(const AsmArgs& g, int t, int q, const double (&a)[5], const double (&b)[5], double e) {
    if (q < g.size[BJ]) g.out[(long)t * g.ld + g.off[BJ] + q] = pair_coeff<F_DELTA, Lay<L>::f[BJ]>(a, b) * e;
}

template <int L>
__global__ __launch_bounds__(256) void assemble_test_kernel(AsmArgs g) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= g.M) return;
    const double y1 = g.px[q], y2 = g.py[q];
    const int t0 = blockIdx.y * TP;
    const int tend = min(t0 + TP, g.Nt);
    for (int t = t0; t < tend; ++t) {
        const double d1 = g.tx[2 * t] - y1, d2 = g.tx[2 * t + 1] - y2;
        const double e = exp(-0.5 * (g.p1 * d1 * d1 + g.p2 * d2 * d2));
        double a[5], b[5];
        hermite_plain(g.p1, d1, a);
        hermite_plain(g.p2, d2, b);
        store_test<L, 0>(g, t, q, a, b, e);
        if (Lay<L>::nb > 1) store_test<L, 1>(g, t, q, a, b, e);
        if (Lay<L>::nb > 2) store_test<L, 2>(g, t, q, a, b, e);
        if (Lay<L>::nb > 3) store_test<L, 3>(g, t, q, a, b, e);
    }
}

// cross-covariance columns (gpk_assemble_cross): the entries of assemble_test_kernel, transposed -- out[(off[BJ] + p) * ld + t] for the
// column point p of block BJ and the test point t.  Lanes run along t, two test points per lane (t, t + 1): for a fixed (block, column
// point) a wave stores 1 KB contiguous with the 16-byte store (WIDE: base and ld even, Nt even), or the same two values as two
// 8-byte stores (any alignment, odd Nt).  One kernel body for both: the values are the same bits either way.  The column point is
// wave-uniform (scalar loads), and one exp + one pair of Hermite evaluations per point pair feeds every block of the layout.
template <int L, int BJ, bool WIDE>
__device__ __forceinline__ void store_cross(const AsmArgs& g, int p, int t, const double (&a0)[5], const double (&b0)[5], double e0,
                                            const double (&a1)[5], const double (&b1)[5], double e1) {
    if (p < g.size[BJ]) {                               // wave-uniform
        const double v0 = pair_coeff<F_DELTA, Lay<L>::f[BJ]>(a0, b0) * e0;
        const double v1 = pair_coeff<F_DELTA, Lay<L>::f[BJ]>(a1, b1) * e1;
        double* const dst = g.out + (long)(g.off[BJ] + p) * g.ld + t;
        if constexpr (WIDE) store2<0>(dst, v0, v1);
        else { dst[0] = v0; if (t + 1 < g.Nt) dst[1] = v1; }
    }
}

template <int L, bool WIDE>
__global__ __launch_bounds__(256) void assemble_cross_kernel(AsmArgs g) {
    const int t = 2 * (blockIdx.x * 256 + threadIdx.x);
    const bool live = t < g.Nt;
    const int tb = min(t + 1, g.Nt - 1);                // odd Nt: the last lane computes its point twice and stores it once
    const double x1a = live ? g.tx[2 * t] : 0.0, x2a = live ? g.tx[2 * t + 1] : 0.0;
    const double x1b = live ? g.tx[2 * tb] : 0.0, x2b = live ? g.tx[2 * tb + 1] : 0.0;
    const int p0 = blockIdx.y * CROSS_TP;
    const int pend = min(p0 + CROSS_TP, g.M);
    for (int p = p0; p < pend; ++p) {
        const double y1 = g.px[p], y2 = g.py[p];        // uniform address -> scalar loads
        if (!live) continue;
        const double d1a = x1a - y1, d2a = x2a - y2, d1b = x1b - y1, d2b = x2b - y2;
        const double e0 = exp(-0.5 * (g.p1 * d1a * d1a + g.p2 * d2a * d2a));
        const double e1 = exp(-0.5 * (g.p1 * d1b * d1b + g.p2 * d2b * d2b));
        double a0[5], b0[5], a1[5], b1[5];
        hermite_plain(g.p1, d1a, a0); hermite_plain(g.p2, d2a, b0);
        hermite_plain(g.p1, d1b, a1); hermite_plain(g.p2, d2b, b1);
        store_cross<L, 0, WIDE>(g, p, t, a0, b0, e0, a1, b1, e1);
        if (Lay<L>::nb > 1) store_cross<L, 1, WIDE>(g, p, t, a0, b0, e0, a1, b1, e1);
        if (Lay<L>::nb > 2) store_cross<L, 2, WIDE>(g, p, t, a0, b0, e0, a1, b1, e1);
        if (Lay<L>::nb > 3) store_cross<L, 3, WIDE>(g, p, t, a0, b0, e0, a1, b1, e1);
    }
}

// prior between two point sets (gpk_assemble_prior): out[i * ld + j] = k(xa_i, xb_j), the value functional on both sides.  The shape of
// assemble_cross_kernel: lanes along j, two columns per lane (16-byte store when WIDE, the same two values as 8-byte stores otherwise),
// the row point wave-uniform (scalar loads), one exp per pair, a workgroup owns 512 columns x CROSS_TP rows.  Write-bound: 8 na nb bytes.
// kappa is even in d and every entry is computed from its own d = xa_i - xb_j, with the one fma written out (kappa2_fma): the two
// columns of a lane and the two triangles of a square call (xa == xb) go through the same roundings, so out[i][j] and out[j][i] are
// the same bits and the diagonal is exp(-0) = 1.
__device__ __forceinline__ double prior_value(double p1, double p2, double d1, double d2) {
    double a[5], b[5];
    hermite_plain(p1, d1, a);
    hermite_plain(p2, d2, b);
    return pair_coeff<F_DELTA, F_DELTA>(a, b) * kappa2_fma(p1, p2, d1, d2);
}

template <bool WIDE>
__global__ __launch_bounds__(256) void assemble_prior_kernel(PriorArgs g) {
    const int j = 2 * (blockIdx.x * 256 + threadIdx.x);
    const bool live = j < g.nb;
    const int jb = min(j + 1, g.nb - 1);                // odd nb: the last lane computes its point twice and stores it once
    const double y1a = live ? g.xb[2 * j] : 0.0, y2a = live ? g.xb[2 * j + 1] : 0.0;
    const double y1b = live ? g.xb[2 * jb] : 0.0, y2b = live ? g.xb[2 * jb + 1] : 0.0;
    const int i0 = blockIdx.y * CROSS_TP;
    const int iend = min(i0 + CROSS_TP, g.na);
    for (int i = i0; i < iend; ++i) {
        const double x1 = g.xa[2 * i], x2 = g.xa[2 * i + 1];   // uniform address -> scalar loads
        if (!live) continue;
        const double v0 = prior_value(g.p1, g.p2, x1 - y1a, x2 - y2a);
        const double v1 = prior_value(g.p1, g.p2, x1 - y1b, x2 - y2b);
        double* const dst = g.out + (long)i * g.ld + j;
        if constexpr (WIDE) store2<0>(dst, v0, v1);
        else { dst[0] = v0; if (j + 1 < g.nb) dst[1] = v1; }
    }
}

template <int L, int BJ>
__device__ __forceinline__ double acc_test(const AsmArgs& g, int q, const double (&a)[5], const double (&b)[5]) {
    return (q < g.size[BJ]) ? pair_coeff<F_DELTA, Lay<L>::f[BJ]>(a, b) * g.coeff[g.off[BJ] + q] : 0.0;
}

// out[t] = sum_c Theta_test[t, c] * coeff[c]; one workgroup per test point, lanes stride over column points.
template <int L>
__global__ __launch_bounds__(256) void extend_kernel(AsmArgs g) {
    __shared__ double red[4];
    const int t = blockIdx.x;
    const double x1 = g.tx[2 * t], x2 = g.tx[2 * t + 1];
    double s = 0.0;
    for (int q = threadIdx.x; q < g.M; q += 256) {
        const double d1 = x1 - g.px[q], d2 = x2 - g.py[q];
        const double e = exp(-0.5 * (g.p1 * d1 * d1 + g.p2 * d2 * d2));
        double a[5], b[5];
        hermite_plain(g.p1, d1, a);
        hermite_plain(g.p2, d2, b);
        double v = acc_test<L, 0>(g, q, a, b);
        if (Lay<L>::nb > 1) v += acc_test<L, 1>(g, q, a, b);
        if (Lay<L>::nb > 2) v += acc_test<L, 2>(g, q, a, b);
        if (Lay<L>::nb > 3) v += acc_test<L, 3>(g, q, a, b);
        s += v * e;
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) g.out[t] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- multi-functional extension (DESIGN.md §K "Row functionals of the extension") ------------------------------------------------
// out[k][t] = sum_b sum_q pair_coeff<F_k, f[b]>(h(p1,d1), h(p2,d2)) kappa(d) c[off_b + q], d = x_t - y_q, F_k over the functionals of
// MASK (bit F = functional F: delta, d1, d2, d2^2, Laplacian; the GPK_FN_* bits of gpk.h).  Every row functional has per-axis order
// <= 2 and so has every column functional: the pair needs h0..h4 only, and ONE exp + one pair of Hermite evaluations feeds all of them.
// Mapping: a workgroup owns FN_TT test points (wave-uniform: scalar loads) and its 256 lanes stride over the column points as in
// extend_kernel; each column point's coordinates and its nb coefficient slices are loaded once and serve all FN_TT test points, and each
// lane keeps FN_TT x popcount(MASK) accumulators.  Points, zeroing and reduction: the frame of gpk_assemble_common.h.
// sum_b pair_coeff<F, f[b]> c[b] (c[b] = 0 outside block b, as acc_test in extend_kernel)
template <int L, int F>
__device__ __forceinline__ double fn_sum(const double (&a)[5], const double (&b)[5], const double (&c)[4]) {
    double v = pair_coeff<F, Lay<L>::f[0]>(a, b) * c[0];
    if (Lay<L>::nb > 1) v += pair_coeff<F, Lay<L>::f[1]>(a, b) * c[1];
    if (Lay<L>::nb > 2) v += pair_coeff<F, Lay<L>::f[2]>(a, b) * c[2];
    if (Lay<L>::nb > 3) v += pair_coeff<F, Lay<L>::f[3]>(a, b) * c[3];
    return v;
}

template <int L, int MASK, int F>
__device__ __forceinline__ void fn_acc(double (&s)[fn_popc(MASK)], const double (&a)[5], const double (&b)[5], const double (&c)[4], double e) {
    if ((MASK >> F) & 1) s[fn_row(MASK, F)] += fn_sum<L, F>(a, b, c) * e;
}

template <int L, int MASK>
__global__ __launch_bounds__(256) void extend_fn_kernel(FnArgs g) {
    constexpr int NF = fn_popc(MASK);
    const int t0 = blockIdx.x * FN_TT;
    double x1[FN_TT], x2[FN_TT], s[FN_TT][NF];
    GPK_FN_LOAD_POINTS2(x1, x2, g.tx, t0, g.Nt);
    fn_zero(s);
    for (int q = threadIdx.x; q < g.M; q += 256) {
        const double y1 = g.px[q], y2 = g.py[q];
        double c[4];
#pragma unroll
        for (int bk = 0; bk < 4; ++bk) c[bk] = (bk < Lay<L>::nb && q < g.size[bk]) ? g.coeff[g.off[bk] + q] : 0.0;
#pragma unroll
        for (int i = 0; i < FN_TT; ++i) {
            const double d1 = x1[i] - y1, d2 = x2[i] - y2;
            const double e = exp(-0.5 * (g.p1 * d1 * d1 + g.p2 * d2 * d2));
            double a[5], b[5];
            hermite_plain(g.p1, d1, a);
            hermite_plain(g.p2, d2, b);
            fn_acc<L, MASK, F_DELTA>(s[i], a, b, c, e);
            fn_acc<L, MASK, F_D1>(s[i], a, b, c, e);
            fn_acc<L, MASK, F_D2>(s[i], a, b, c, e);
            fn_acc<L, MASK, F_DD2>(s[i], a, b, c, e);
            fn_acc<L, MASK, F_LAP>(s[i], a, b, c, e);
        }
    }
    GPK_FN_REDUCE_STORE(s, NF, t0, g.Nt, g.out, g.ldo);
}

// one instantiation per (layout, mask)
template <int L>
void launch_extend_fn(int mask, int grid, hipStream_t st, const FnArgs& g) {
    with_mask<31>(mask, [&](auto m) { extend_fn_kernel<L, decltype(m)::value><<<grid, 256, 0, st>>>(g); });
}

// r = residual of the equation at each test point from the extension's rows: the relations the Gauss-Newton systems eliminate
// (reference src/PDEs.py:132 elliptic, :341 Burgers, :491 Eikonal; src/InverseProblems.py:185 Darcy; gpk.h, gpk_pde_residual)
__global__ __launch_bounds__(256) void pde_residual_kernel(int sys, double p0, double p1, int Nt, const double* __restrict__ u, long ldu,
                                                           const double* __restrict__ a, long lda, const double* __restrict__ f,
                                                           double* __restrict__ out) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= Nt) return;
    const double u0 = u[t], u1 = u[ldu + t], u2 = u[2 * ldu + t], u3 = u[3 * ldu + t], ft = f[t];
    double r;
    switch (sys) {
        case GPK_GN_BURGERS:  r = u1 + p0 * u0 * u2 - p1 * u3 - ft; break;                 // u_t + alpha u u_x - nu u_xx - f
        case GPK_GN_EIKONAL:  r = u1 * u1 + u2 * u2 - ft * ft - p0 * u3; break;            // |grad u|^2 - f^2 - eps Delta u
        case GPK_GN_DARCY: {                                                                // -e^a (Delta u + grad a . grad u) - f
            const double a0 = a[t], a1 = a[lda + t], a2 = a[2 * lda + t];
            r = -exp(a0) * (u3 + a1 * u1 + a2 * u2) - ft;
            break;
        }
        default:              r = -u3 + p0 * pow(u0, p1) - ft; break;                      // -Delta u + alpha u^m - f (also relaxed)
    }
    out[t] = r;
}

// the elliptic equation with a reaction term of the family (gpk.h, gpk_pde_residual_nl): r = -u3 + tau(u0) - f
__global__ __launch_bounds__(256) void pde_residual_nl_kernel(int nonlin, double p0, double p1, double p2, int Nt, const double* __restrict__ u,
                                                              long ldu, const double* __restrict__ f, double* __restrict__ out) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= Nt) return;
    const double u0 = u[t], u3 = u[3 * ldu + t], ft = f[t];
    out[t] = -u3 + nl_tau(nonlin, p0, p1, p2, u0) - ft;
}

// the equation of GPK_GN_SEMILINEAR (gpk.h, gpk_pde_residual_sl): r = -eps u3 + N(u0, u1, u2) - f
struct SlCoeff { double v[5]; };
__global__ __launch_bounds__(256) void pde_residual_sl_kernel(double eps, SlCoeff gq, int Nt, const double* __restrict__ u, long ldu,
                                                              const double* __restrict__ f, double* __restrict__ out) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= Nt) return;
    const double u0 = u[t], u1 = u[ldu + t], u2 = u[2 * ldu + t], u3 = u[3 * ldu + t], ft = f[t];
    out[t] = (sl_N(gq.v, u0, u1, u2) - eps * u3) - ft;
}

template <int L> constexpr int lay_size(int b, int Nd, int Nb) { return b < Lay<L>::nb ? (Lay<L>::db[b] ? Nd + Nb : Nd) : 0; }
template <int L> constexpr int lay_N(int Nd, int Nb) { return lay_size<L>(0, Nd, Nb) + lay_size<L>(1, Nd, Nb) + lay_size<L>(2, Nd, Nb) + lay_size<L>(3, Nd, Nb); }

// precisions, block offsets / sizes and the packed points: the fields AsmArgs and FnArgs share (the others are the caller's); the axes
// of the periodic kernel
template <class Args>
int fill_common(gpk_handle h, Args& g, int layout, int kernel, const double* kp, const double* Xd, int Nd, const double* Xb, int Nb,
                PerArgs& per) {
    if (Nd <= 0 || Nb < 0 || !kp || !Xd) return gpk_bad_arg(h, "assemble: sizes/pointers");
    double p[2];
    if (matern_order(kernel)) GPK_TRY(matern_scales(h, kp, p));      // (the Matern family: inverse length scales)
    else if (kernel == GPK_KERNEL_PERIODIC) { GPK_TRY(periodic_axes(h, kp, per)); p[0] = per.ax[0].p; p[1] = per.ax[1].p; }   // (per: read by the periodic kernels only)
    else GPK_TRY(precisions(h, "assemble: kernel id", kernel, kp, 2, p));
    g.p1 = p[0]; g.p2 = p[1];
    const bool known = with_layout(layout, [&](auto l) {
        constexpr int L = decltype(l)::value;
        int o = 0;
        for (int b = 0; b < 4; ++b) { g.size[b] = lay_size<L>(b, Nd, Nb); g.off[b] = o; o += g.size[b]; }
    });
    if (!known) return gpk_bad_arg(h, "assemble: layout id");
    const int Mall = Nd + Nb;
    GPK_TRY(gpk_i_ensure_points(h, 2 * (size_t)Mall));
    g.px = h->d_pts; g.py = h->d_pts + Mall;
    pack_points_kernel<<<gpk_ceil_div(Mall, 256), 256, 0, h->stream>>>(Xd, Nd, Xb, Nb, h->d_pts, h->d_pts + Mall);
    GPK_LAUNCH_CHECK(h);
    g.M = (layout == GPK_LAYOUT_DARCY_A) ? Nd : Mall;
    if constexpr (std::is_same<Args, AsmArgs>::value) g.Nd = Nd;
    return 0;
}

// value of <f, f> at d = 0 (SURVEY §8a-K last column): makes the adaptive trace ratios analytic
template <int L> void diag_values(double p1, double p2, double (&c)[4]) {
    double a[5], b[5];
    hermite_plain(p1, 0.0, a);
    hermite_plain(p2, 0.0, b);
    c[0] = pair_coeff<Lay<L>::f[0], Lay<L>::f[0]>(a, b);
    c[1] = pair_coeff<Lay<L>::f[1], Lay<L>::f[1]>(a, b);
    c[2] = pair_coeff<Lay<L>::f[2], Lay<L>::f[2]>(a, b);
    c[3] = pair_coeff<Lay<L>::f[3], Lay<L>::f[3]>(a, b);
}

}  // namespace


extern "C" int gpk_assemble(gpk_handle h, int layout, int kernel, const double* kp, const double* Xd, int Nd,
                            const double* Xb, int Nb, double nugget, int nugget_type, double* Theta, int ld,
                            double* ratios) {
    if (!h || !Theta) return GPK_ERR_ARG;
    AsmArgs g{};
    PerArgs per{};
    GPK_TRY(fill_common(h, g, layout, kernel, kp, Xd, Nd, Xb, Nb, per));
    const int matern = matern_order(kernel);                         // the kernel family is chosen here, on the host: 0 = Gaussian
    const bool periodic = kernel == GPK_KERNEL_PERIODIC;
    int nb = 0, N = 0;
    double c[4] = {0, 0, 0, 0};
    with_layout(layout, [&](auto l) {
        constexpr int L = decltype(l)::value;
        nb = Lay<L>::nb; N = lay_N<L>(Nd, Nb);
        if (!matern && !periodic) diag_values<L>(g.p1, g.p2, c);
    });
    if (matern) gpk_i_matern_diag(matern, layout, g.p1, g.p2, c);
    if (periodic) gpk_i_periodic_diag(layout, per, c);
    if (ld < N) return gpk_bad_arg(h, "assemble: ld < N");
    // ratio_k = trace(block k) / trace(last block)   (src/PDEs.py:62-66, 256-262, 397-402; IP.py:72-87)
    double r[4] = {0, 0, 0, 1.0};
    const double tr_last = (double)g.size[nb - 1] * c[nb - 1];
    for (int b = 0; b < nb - 1; ++b) r[b] = ((double)g.size[b] * c[b]) / tr_last;
    if (ratios) { ratios[0] = ratios[1] = ratios[2] = 0.0; for (int b = 0; b < nb - 1; ++b) ratios[b] = r[b]; }
    if (!nugget_type_valid(nugget_type)) return gpk_bad_arg(h, "assemble: nugget_type");
    for (int b = 0; b < nb; ++b) g.nug[b] = block_nugget(nugget_type, nugget, b == nb - 1 ? 1.0 : r[b]);
    g.out = Theta; g.ld = ld;
    const bool pairs = pairs_eligible(h, Theta, ld, g.M, g.size[0], g.size[1], g.size[2], g.size[3]);   // (even sizes: even offsets)
    TimedLaunch timed(h);
    GPK_TRY(timed.start());
    if (matern) gpk_i_matern_gram(matern, layout, pairs, h->tune.asm_nt, h->stream, g);
    else if (periodic) gpk_i_periodic_gram(layout, pairs, h->tune.asm_nt, h->stream, g, per);
    else with_layout(layout, [&](auto l) {
        constexpr int L = decltype(l)::value;
        const dim3 grid(gpk_ceil_div(g.M, 256), gpk_ceil_div(g.M, TP)), grid2(gpk_ceil_div(g.M / 2, 256), gpk_ceil_div(g.M, TP));
        if (!pairs) assemble_kernel<L><<<grid, 256, 0, h->stream>>>(g);
        else switch (h->tune.asm_nt) {
            case 1: assemble2_kernel<L, 1><<<grid2, 256, 0, h->stream>>>(g); break;
            case 2: assemble2_kernel<L, 2><<<grid2, 256, 0, h->stream>>>(g); break;
            case 3: assemble2_kernel<L, 3><<<grid2, 256, 0, h->stream>>>(g); break;
            default: assemble2_kernel<L, 0><<<grid2, 256, 0, h->stream>>>(g); break;
        }
    });
    GPK_LAUNCH_CHECK(h);
    return 0;
}

extern "C" int gpk_assemble_test(gpk_handle h, int layout, int kernel, const double* kp, const double* Xt, int Nt,
                                 const double* Xd, int Nd, const double* Xb, int Nb, double* out, int ld) {
    if (!h) return GPK_ERR_ARG;
    if (!out || !Xt) return gpk_bad_arg(h, "assemble_test: pointers");
    if (Nt <= 0) return gpk_bad_arg(h, "assemble_test: Nt <= 0");
    AsmArgs g{};
    PerArgs per{};
    GPK_TRY(fill_common(h, g, layout, kernel, kp, Xd, Nd, Xb, Nb, per));
    int N = 0;
    with_layout(layout, [&](auto l) { N = lay_N<decltype(l)::value>(Nd, Nb); });
    if (ld < N) return gpk_bad_arg(h, "assemble_test: ld < N");      // (rows would overlap and the last one leave the Nt x ld region)
    g.out = out; g.ld = ld; g.tx = Xt; g.Nt = Nt;
    const dim3 grid(gpk_ceil_div(g.M, 256), gpk_ceil_div(Nt, TP));
    if (const int matern = matern_order(kernel)) gpk_i_matern_test(matern, layout, h->stream, g);
    else if (kernel == GPK_KERNEL_PERIODIC) gpk_i_periodic_test(layout, h->stream, g, per);
    else with_layout(layout, [&](auto l) { assemble_test_kernel<decltype(l)::value><<<grid, 256, 0, h->stream>>>(g); });
    GPK_LAUNCH_CHECK(h);
    return 0;
}

// The block of gpk_assemble_test, transposed: N x Nt, the right-hand-side layout of gpk_trsm / gpk_trsm_dinv (gpk.h, "Posterior variance").
// It lives here, not in gpk_posterior.hip, because Lay<L>, the plain pair_coeff and fill_common are this file's.
extern "C" int gpk_assemble_cross(gpk_handle h, int layout, int kernel, const double* kp, const double* Xt, int Nt,
                                  const double* Xd, int Nd, const double* Xb, int Nb, double* out, int ld) {
    if (!h) return GPK_ERR_ARG;
    if (!out || !Xt) return gpk_bad_arg(h, "assemble_cross: pointers");
    if (Nt <= 0) return gpk_bad_arg(h, "assemble_cross: Nt <= 0");
    if (ld < Nt) return gpk_bad_arg(h, "assemble_cross: ld < Nt");
    AsmArgs g{};
    PerArgs per{};
    GPK_TRY(fill_common(h, g, layout, kernel, kp, Xd, Nd, Xb, Nb, per));
    g.out = out; g.ld = ld; g.tx = Xt; g.Nt = Nt;
    const bool wide = pairs_eligible(h, out, ld, Nt);
    const dim3 grid(gpk_ceil_div(gpk_ceil_div(Nt, 2), 256), gpk_ceil_div(g.M, CROSS_TP));
    if (const int matern = matern_order(kernel)) gpk_i_matern_cross(matern, layout, wide, h->stream, g);
    else if (kernel == GPK_KERNEL_PERIODIC) gpk_i_periodic_cross(layout, wide, h->stream, g, per);
    else with_layout(layout, [&](auto l) {                           // (not timed: gpk_prof_read_assembly keeps reporting the Gram launch)
        constexpr int L = decltype(l)::value;
        if (wide) assemble_cross_kernel<L, true><<<grid, 256, 0, h->stream>>>(g);
        else assemble_cross_kernel<L, false><<<grid, 256, 0, h->stream>>>(g);
    });
    GPK_LAUNCH_CHECK(h);
    return 0;
}

// The prior k(xa_i, xb_j) between two sets of points (gpk.h, "Posterior covariance and samples"): no collocation points, no layout.
extern "C" int gpk_assemble_prior(gpk_handle h, int kernel, const double* kp, const double* Xa, int na, const double* Xb, int nb,
                                  double* out, int ld) {
    if (!h) return GPK_ERR_ARG;
    if (!out || !Xa || !Xb || !kp) return gpk_bad_arg(h, "assemble_prior: pointers");
    if (na <= 0) return gpk_bad_arg(h, "assemble_prior: na <= 0");
    if (nb <= 0) return gpk_bad_arg(h, "assemble_prior: nb <= 0");
    if (ld < nb) return gpk_bad_arg(h, "assemble_prior: ld < nb");
    PriorArgs g{};
    double p[2];
    const int matern = matern_order(kernel);
    PerArgs per{};
    if (matern) GPK_TRY(matern_scales(h, kp, p));
    else if (kernel == GPK_KERNEL_PERIODIC) { GPK_TRY(periodic_axes(h, kp, per)); p[0] = per.ax[0].p; p[1] = per.ax[1].p; }
    else GPK_TRY(precisions(h, "assemble_prior: kernel id", kernel, kp, 2, p));
    g.p1 = p[0]; g.p2 = p[1];
    g.xa = Xa; g.na = na; g.xb = Xb; g.nb = nb; g.out = out; g.ld = ld;
    const bool wide = pairs_eligible(h, out, ld, nb);
    const dim3 grid(gpk_ceil_div(gpk_ceil_div(nb, 2), 256), gpk_ceil_div(na, CROSS_TP));
    if (matern) gpk_i_matern_prior(matern, wide, h->stream, g);
    else if (kernel == GPK_KERNEL_PERIODIC) gpk_i_periodic_prior(wide, h->stream, g, per);
    else if (wide) assemble_prior_kernel<true><<<grid, 256, 0, h->stream>>>(g);
    else assemble_prior_kernel<false><<<grid, 256, 0, h->stream>>>(g);
    GPK_LAUNCH_CHECK(h);
    return 0;
}

// err[i] = |truth[i] - approx[i]|, its maximum and its sum of squares in one pass (one workgroup: n is a point count, at most a
// few 10^4; fixed summation order, so the figures are reproducible)
__global__ __launch_bounds__(1024) void error_metrics_kernel(int n, const double* __restrict__ truth, const double* __restrict__ approx,
                                                              double* __restrict__ err, double* __restrict__ out2) {
    __shared__ double smax[16], ssum[16];
    double m = 0.0, q = 0.0;
    for (int i = threadIdx.x; i < n; i += 1024) {
        const double e = fabs(truth[i] - approx[i]);
        if (err) err[i] = e;
        m = (e > m || e != e) ? e : m;                               // NaNs propagate, as under jnp.max
        q = fma(e, e, q);
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double mo = __shfl_down(m, off, 64);
        m = (mo > m || mo != mo) ? mo : m;
        q += __shfl_down(q, off, 64);
    }
    if ((threadIdx.x & 63) == 0) { smax[threadIdx.x >> 6] = m; ssum[threadIdx.x >> 6] = q; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double mm = 0.0, qq = 0.0;
        for (int w = 0; w < 16; ++w) { mm = (smax[w] > mm || smax[w] != smax[w]) ? smax[w] : mm; qq += ssum[w]; }
        out2[0] = mm; out2[1] = qq;
    }
}

extern "C" int gpk_error_metrics(gpk_handle h, int n, const double* truth, const double* approx, double* err_all,
                                 double* host_max, double* host_l2) {
    if (!h || !truth || !approx || n <= 0 || !host_max || !host_l2) return GPK_ERR_ARG;
    error_metrics_kernel<<<1, 1024, 0, h->stream>>>(n, truth, approx, err_all, h->d_scalars + 2);
    GPK_LAUNCH_CHECK(h);
    double r[2] = {0.0, 0.0};
    GPK_HIP(h, hipMemcpyAsync(r, h->d_scalars + 2, sizeof r, hipMemcpyDeviceToHost, h->stream));
    GPK_HIP(h, hipStreamSynchronize(h->stream));
    *host_max = r[0];
    *host_l2 = sqrt(r[1] / (double)n);
    return 0;
}

extern "C" int gpk_extend(gpk_handle h, int layout, int kernel, const double* kp, const double* Xt, int Nt,
                          const double* Xd, int Nd, const double* Xb, int Nb, const double* coeff, double* out) {
    if (!h || !out || !Xt || !coeff || Nt <= 0) return GPK_ERR_ARG;
    AsmArgs g{};
    PerArgs per{};
    GPK_TRY(fill_common(h, g, layout, kernel, kp, Xd, Nd, Xb, Nb, per));
    g.out = out; g.ld = 0; g.tx = Xt; g.Nt = Nt; g.coeff = coeff;
    if (const int matern = matern_order(kernel)) gpk_i_matern_extend(matern, layout, h->stream, g);
    else if (kernel == GPK_KERNEL_PERIODIC) gpk_i_periodic_extend(layout, h->stream, g, per);
    else with_layout(layout, [&](auto l) { extend_kernel<decltype(l)::value><<<Nt, 256, 0, h->stream>>>(g); });
    GPK_LAUNCH_CHECK(h);
    return 0;
}

extern "C" int gpk_extend_functionals(gpk_handle h, int layout, int kernel, const double* kp, const double* Xt, int Nt,
                                      const double* Xd, int Nd, const double* Xb, int Nb, const double* coeff, int fmask,
                                      double* out, int ldo) {
    if (!h) return GPK_ERR_ARG;
    if (!out || !Xt || !coeff) return gpk_bad_arg(h, "extend_functionals: pointers");
    if (fmask <= 0 || fmask > 31) return gpk_bad_arg(h, "extend_functionals: fmask must be a non-empty subset of the GPK_FN_* bits");
    if (Nt <= 0) return gpk_bad_arg(h, "extend_functionals: Nt <= 0");
    if (ldo < Nt) return gpk_bad_arg(h, "extend_functionals: ldo < Nt");
    FnArgs g;
    PerArgs per{};
    GPK_TRY(fill_common(h, g, layout, kernel, kp, Xd, Nd, Xb, Nb, per));
    g.tx = Xt; g.Nt = Nt; g.coeff = coeff; g.out = out; g.ldo = ldo;
    if (const int matern = matern_order(kernel)) gpk_i_matern_extend_fn(matern, layout, fmask, h->stream, g);
    else if (kernel == GPK_KERNEL_PERIODIC) gpk_i_periodic_extend_fn(layout, fmask, h->stream, g, per);
    else with_layout(layout, [&](auto l) { launch_extend_fn<decltype(l)::value>(fmask, gpk_ceil_div(Nt, FN_TT), h->stream, g); });
    GPK_LAUNCH_CHECK(h);
    return 0;
}

extern "C" int gpk_pde_residual(gpk_handle h, int system, const double* params3, int Nt, const double* fields_u, int ldu,
                                const double* fields_a, int lda, const double* rhs, double* out) {
    if (!h) return GPK_ERR_ARG;
    if (system < GPK_GN_ELLIPTIC || system > GPK_GN_ELLIPTIC_RELAXED) return gpk_bad_arg(h, "pde_residual: system id");
    if (Nt <= 0) return gpk_bad_arg(h, "pde_residual: Nt <= 0");
    if (!fields_u || !rhs || !out || ldu < Nt) return gpk_bad_arg(h, "pde_residual: fields_u / rhs / out / ldu");
    if (system == GPK_GN_DARCY && (!fields_a || lda < Nt)) return gpk_bad_arg(h, "pde_residual: Darcy needs fields_a (3 rows, lda >= Nt)");
    if (system != GPK_GN_DARCY && !params3) return gpk_bad_arg(h, "pde_residual: host_params3");
    const double p0 = params3 ? params3[0] : 0.0, p1 = params3 ? params3[1] : 0.0;
    pde_residual_kernel<<<gpk_ceil_div(Nt, 256), 256, 0, h->stream>>>(system, p0, p1, Nt, fields_u, ldu,
                                                                      system == GPK_GN_DARCY ? fields_a : nullptr, lda, rhs, out);
    GPK_LAUNCH_CHECK(h);
    return 0;
}

extern "C" int gpk_pde_residual_nl(gpk_handle h, int nonlin, const double* params3, int Nt, const double* fields_u, int ldu,
                                   const double* rhs, double* out) {
    if (!h) return GPK_ERR_ARG;
    if (!gpk_nl_valid(nonlin)) return gpk_bad_arg(h, "pde_residual_nl: nonlin is not one of GPK_NL_POWER .. GPK_NL_CUBIC");
    if (Nt <= 0) return gpk_bad_arg(h, "pde_residual_nl: Nt <= 0");
    if (!fields_u || !rhs || !out || ldu < Nt) return gpk_bad_arg(h, "pde_residual_nl: fields_u / rhs / out / ldu");
    if (!params3) return gpk_bad_arg(h, "pde_residual_nl: host_params3");
    if (nonlin == GPK_NL_POWER)                                       // the power law: the kernel of gpk_pde_residual, hence its numbers
        pde_residual_kernel<<<gpk_ceil_div(Nt, 256), 256, 0, h->stream>>>(GPK_GN_ELLIPTIC, params3[0], params3[1], Nt, fields_u, ldu, nullptr, 0, rhs, out);
    else
        pde_residual_nl_kernel<<<gpk_ceil_div(Nt, 256), 256, 0, h->stream>>>(nonlin, params3[0], params3[1], params3[2], Nt, fields_u, ldu, rhs, out);
    GPK_LAUNCH_CHECK(h);
    return 0;
}

extern "C" int gpk_pde_residual_sl(gpk_handle h, double eps, const double* gq5, int Nt, const double* fields, int ldf,
                                   const double* rhs, double* out) {
    if (!h) return GPK_ERR_ARG;
    if (!(std::isfinite(eps) && eps != 0.0)) return gpk_bad_arg(h, "pde_residual_sl: eps must be finite and not 0");
    if (!gq5) return gpk_bad_arg(h, "pde_residual_sl: host_gq5");
    if (Nt <= 0) return gpk_bad_arg(h, "pde_residual_sl: Nt <= 0");
    if (!fields || !rhs || !out || ldf < Nt) return gpk_bad_arg(h, "pde_residual_sl: fields / rhs / out / ldf");
    SlCoeff gq;
    for (int k = 0; k < 5; ++k) gq.v[k] = gq5[k];
    pde_residual_sl_kernel<<<gpk_ceil_div(Nt, 256), 256, 0, h->stream>>>(eps, gq, Nt, fields, ldf, rhs, out);
    GPK_LAUNCH_CHECK(h);
    return 0;
}
