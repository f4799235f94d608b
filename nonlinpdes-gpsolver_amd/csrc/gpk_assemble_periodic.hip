// gpk_assemble_periodic.hip -- the periodic kernel in the fused Gram evaluator of the reference layouts.
//
// One counterpart for each kernel shape of gpk_assemble.hip -- one-point and two-point Gram kernel, test rows, cross columns, prior,
// extension, multi-functional extension -- with the same lane-to-point mapping, the same grids, the same store pattern and the same
// fixed-order reductions; the entry points of gpk_assemble.hip choose the family on the host and launch these through
// gpk_assemble_ref.h.  A translation unit of its own: nothing here is seen by the compiler when it generates the Gaussian or the
// Matern kernels, and the axes travel in an argument of their own (PerArgs), so the argument structs of those kernels do not change.
//
// Math (DESIGN.md §K "Periodic kernel").  The kernel is a product over the axes; an axis with period L > 0, w = 2 pi / L, has
//   kappa(d) = exp(-(2 p / w^2) sin^2(w d / 2)) = exp(-p d^2 / 2) (1 + O(w^2 d^2)),
// and with s = (p / w) sin w d, c = p cos w d the factors h_m = (-1)^m kappa^(m) / kappa (the sign convention of hermite_plain) are
//   h0 = 1, h1 = s, h2 = s^2 - c, h3 = s (s^2 - 3 c - w^2), h4 = s^4 - 6 s^2 c + 3 c^2 - 4 w^2 s^2 + w^2 c,
// which tend to the Hermite table as w -> 0; an axis with L = 0 keeps the Gaussian factor and the Hermite table.  An entry is
// pair_coeff(a, b) e with a, b the tables of the two axes and e the product of the two factors: as in gpk_assemble.hip, one exp per
// point pair feeds every block.
//
// Evaluation.  d = x - y, then sincospi(d / L) = (sin, cos)(w d / 2) with exact argument reduction -- odd / even in d to the bit and
// right for any |d|, images x + k L included -- then sin w d = 2 s_h c_h, cos w d = 1 - 2 s_h^2, and the exponent -(2 p / w^2) s_h^2.
// Whether an axis is periodic is a wave-uniform branch on a kernel argument (PerAxis::L), not a template parameter: the three
// combinations would triple the 4 x 31 instantiations of the extension kernels for a scalar compare per axis and pair, in kernels
// that are bound by their stores.
//
// Every kernel computes an entry with the same bits for the same point pair: the per-pair arithmetic is written with explicit fma and
// compiled without contraction (as the bc / op evaluators and the Matern family), so the 8-byte and the 16-byte store paths agree.
// Every term of an entry is odd or even in d to the bit, so Theta[i][j] and Theta[j][i] are the same bits.
#include "gpk_assemble_ref.h"

using namespace gpk_asm;

namespace {

// h[0..4] of one axis at d; returns z with kappa_axis = exp(-g z^2): sin(w d / 2), or d on an axis that is not periodic
__device__ __forceinline__ double axis_table(const PerAxis& k, double d, double (&h)[5]) {
#pragma clang fp contract(off)
    h[0] = 1.0;
    if (k.L > 0.0) {                                    // wave-uniform: a kernel argument
        double sh, ch;
        sincospi(d / k.L, &sh, &ch);                    // sin, cos of w d / 2
        const double sw = (2.0 * sh) * ch;              // sin w d
        const double cw = __builtin_fma(-2.0 * sh, sh, 1.0);   // cos w d
        const double s = k.pw * sw, c = k.p * cw;
        const double s2 = s * s;
        h[1] = s;
        h[2] = s2 - c;
        h[3] = s * ((s2 - 3.0 * c) - k.w2);
        h[4] = __builtin_fma(s2, (s2 - 6.0 * c) - 4.0 * k.w2, c * __builtin_fma(3.0, c, k.w2));
        return sh;
    }
    const double q = k.p * d;
    const double q2 = q * q;
    h[1] = q;
    h[2] = q2 - k.p;
    h[3] = q * (q2 - 3.0 * k.p);
    h[4] = __builtin_fma(q2, q2 - 6.0 * k.p, 3.0 * k.p * k.p);
    return d;
}

// the two tables and e = kappa of a point pair
__device__ __forceinline__ double pair_tables(const PerArgs& k, double d1, double d2, double (&a)[5], double (&b)[5]) {
#pragma clang fp contract(off)
    const double z1 = axis_table(k.ax[0], d1, a);
    const double z2 = axis_table(k.ax[1], d2, b);
    return exp(-__builtin_fma(k.ax[1].g * z2, z2, k.ax[0].g * z1 * z1));
}

// pair_coeff of gpk_assemble.hip without contraction
template <int FX, int FY>
__host__ __device__ __forceinline__ double pair_coeff_p(const double (&a)[5], const double (&b)[5]) {
#pragma clang fp contract(off)
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < f_count(FX); ++i) {
#pragma unroll
        for (int j = 0; j < f_count(FY); ++j) {
            const double t = a[f_a1(FX, i) + f_a1(FY, j)] * b[f_a2(FX, i) + f_a2(FY, j)];
            if ((f_a1(FX, i) + f_a2(FX, i)) & 1) s -= t; else s += t;
        }
    }
    return s;
}

template <int FX, int FY>
__device__ __forceinline__ double entry(const double (&a)[5], const double (&b)[5], double e) {
#pragma clang fp contract(off)
    return pair_coeff_p<FX, FY>(a, b) * e;
}

// ---- Gram kernels: the frames of assemble_kernel / assemble2_kernel (gpk_assemble.hip) -----------------------------------------------
template <int L, int BI, int BJ>
__device__ __forceinline__ void store_block(const AsmArgs& g, int p, int q, const double (&a)[5], const double (&b)[5], double e) {
    if (q < g.size[BJ]) {
        double v = entry<Lay<L>::f[BI], Lay<L>::f[BJ]>(a, b, e);
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

template <int L, int BI, int BJ, int NT>
__device__ __forceinline__ void store_block2(const AsmArgs& g, int p, int q, const double (&a0)[5], const double (&b0)[5], double e0,
                                             const double (&a1)[5], const double (&b1)[5], double e1) {
    if (q < g.size[BJ]) {                                            // (sizes are even here: q and q + 1 are both inside or both outside)
        double v0 = entry<Lay<L>::f[BI], Lay<L>::f[BJ]>(a0, b0, e0);
        double v1 = entry<Lay<L>::f[BI], Lay<L>::f[BJ]>(a1, b1, e1);
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
__global__ __launch_bounds__(256) void periodic_assemble2_kernel(AsmArgs g, PerArgs k) {
    const int q = 2 * (blockIdx.x * 256 + threadIdx.x);
    const bool live = q < g.M;                                       // (M even: q + 1 < M as well)
    const double y1a = live ? g.px[q] : 0.0, y2a = live ? g.py[q] : 0.0;
    const double y1b = live ? g.px[q + 1] : 0.0, y2b = live ? g.py[q + 1] : 0.0;
    const int p0 = blockIdx.y * TP;
    const int pend = min(p0 + TP, g.M);
    for (int p = p0; p < pend; ++p) {
        const double x1 = g.px[p], x2 = g.py[p];        // uniform address -> scalar loads
        if (!live) continue;
        double a0[5], b0[5], a1[5], b1[5];
        const double e0 = pair_tables(k, x1 - y1a, x2 - y2a, a0, b0);
        const double e1 = pair_tables(k, x1 - y1b, x2 - y2b, a1, b1);
        store_row2<L, 0, NT>(g, p, q, a0, b0, e0, a1, b1, e1);
        if (Lay<L>::nb > 1) store_row2<L, 1, NT>(g, p, q, a0, b0, e0, a1, b1, e1);
        if (Lay<L>::nb > 2) store_row2<L, 2, NT>(g, p, q, a0, b0, e0, a1, b1, e1);
        if (Lay<L>::nb > 3) store_row2<L, 3, NT>(g, p, q, a0, b0, e0, a1, b1, e1);
    }
}

template <int L>
__global__ __launch_bounds__(256) void periodic_assemble_kernel(AsmArgs g, PerArgs k) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    const bool live = q < g.M;
    const double y1 = live ? g.px[q] : 0.0, y2 = live ? g.py[q] : 0.0;
    const int p0 = blockIdx.y * TP;
    const int pend = min(p0 + TP, g.M);
    for (int p = p0; p < pend; ++p) {
        const double x1 = g.px[p], x2 = g.py[p];        // uniform address -> scalar loads
        if (!live) continue;
        double a[5], b[5];
        const double e = pair_tables(k, x1 - y1, x2 - y2, a, b);
        store_row<L, 0>(g, p, q, a, b, e);
        if (Lay<L>::nb > 1) store_row<L, 1>(g, p, q, a, b, e);
        if (Lay<L>::nb > 2) store_row<L, 2>(g, p, q, a, b, e);
        if (Lay<L>::nb > 3) store_row<L, 3>(g, p, q, a, b, e);
    }
}

// ---- test rows: functional delta at the test point, column functionals of the layout (assemble_test_kernel) ---------------------------
template <int L, int BJ>
__device__ __forceinline__ void store_test(const AsmArgs& g, int t, int q, const double (&a)[5], const double (&b)[5], double e) {
    if (q < g.size[BJ]) g.out[(long)t * g.ld + g.off[BJ] + q] = entry<F_DELTA, Lay<L>::f[BJ]>(a, b, e);
}

template <int L>
__global__ __launch_bounds__(256) void periodic_assemble_test_kernel(AsmArgs g, PerArgs k) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= g.M) return;
    const double y1 = g.px[q], y2 = g.py[q];
    const int t0 = blockIdx.y * TP;
    const int tend = min(t0 + TP, g.Nt);
    for (int t = t0; t < tend; ++t) {
        double a[5], b[5];
        const double e = pair_tables(k, g.tx[2 * t] - y1, g.tx[2 * t + 1] - y2, a, b);
        store_test<L, 0>(g, t, q, a, b, e);
        if (Lay<L>::nb > 1) store_test<L, 1>(g, t, q, a, b, e);
        if (Lay<L>::nb > 2) store_test<L, 2>(g, t, q, a, b, e);
        if (Lay<L>::nb > 3) store_test<L, 3>(g, t, q, a, b, e);
    }
}

// ---- cross-covariance columns: the test rows transposed, two test points per lane (assemble_cross_kernel) -----------------------------
template <int L, int BJ, bool WIDE>
__device__ __forceinline__ void store_cross(const AsmArgs& g, int p, int t, const double (&a0)[5], const double (&b0)[5], double e0,
                                            const double (&a1)[5], const double (&b1)[5], double e1) {
    if (p < g.size[BJ]) {                               // wave-uniform
        const double v0 = entry<F_DELTA, Lay<L>::f[BJ]>(a0, b0, e0);
        const double v1 = entry<F_DELTA, Lay<L>::f[BJ]>(a1, b1, e1);
        double* const dst = g.out + (long)(g.off[BJ] + p) * g.ld + t;
        if constexpr (WIDE) store2<0>(dst, v0, v1);
        else { dst[0] = v0; if (t + 1 < g.Nt) dst[1] = v1; }
    }
}

template <int L, bool WIDE>
__global__ __launch_bounds__(256) void periodic_assemble_cross_kernel(AsmArgs g, PerArgs k) {
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
        double a0[5], b0[5], a1[5], b1[5];
        const double e0 = pair_tables(k, x1a - y1, x2a - y2, a0, b0);
        const double e1 = pair_tables(k, x1b - y1, x2b - y2, a1, b1);
        store_cross<L, 0, WIDE>(g, p, t, a0, b0, e0, a1, b1, e1);
        if (Lay<L>::nb > 1) store_cross<L, 1, WIDE>(g, p, t, a0, b0, e0, a1, b1, e1);
        if (Lay<L>::nb > 2) store_cross<L, 2, WIDE>(g, p, t, a0, b0, e0, a1, b1, e1);
        if (Lay<L>::nb > 3) store_cross<L, 3, WIDE>(g, p, t, a0, b0, e0, a1, b1, e1);
    }
}

// ---- prior between two point sets: out[i * ld + j] = k(xa_i, xb_j) (assemble_prior_kernel) ---------------------------------------------
// Only e is used (h0 = 1), so the tables are dead code here.  e depends on d through squares alone, so a square call (xa == xb) gives
// out[i][j] and out[j][i] the same bits, and at d = 0 it is exp(-0) = 1.
template <bool WIDE>
__global__ __launch_bounds__(256) void periodic_assemble_prior_kernel(PriorArgs g, PerArgs k) {
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
        double a0[5], b0[5], a1[5], b1[5];
        const double e0 = pair_tables(k, x1 - y1a, x2 - y2a, a0, b0);
        const double e1 = pair_tables(k, x1 - y1b, x2 - y2b, a1, b1);
        const double v0 = entry<F_DELTA, F_DELTA>(a0, b0, e0), v1 = entry<F_DELTA, F_DELTA>(a1, b1, e1);
        double* const dst = g.out + (long)i * g.ld + j;
        if constexpr (WIDE) store2<0>(dst, v0, v1);
        else { dst[0] = v0; if (j + 1 < g.nb) dst[1] = v1; }
    }
}

// ---- extension: out[t] = sum_c Theta_test[t, c] * coeff[c] (extend_kernel) --------------------------------------------------------------
template <int L, int BJ>
__device__ __forceinline__ double acc_test(const AsmArgs& g, int q, const double (&a)[5], const double (&b)[5]) {
    return (q < g.size[BJ]) ? pair_coeff_p<F_DELTA, Lay<L>::f[BJ]>(a, b) * g.coeff[g.off[BJ] + q] : 0.0;
}

template <int L>
__global__ __launch_bounds__(256) void periodic_extend_kernel(AsmArgs g, PerArgs k) {
    __shared__ double red[4];
    const int t = blockIdx.x;
    const double x1 = g.tx[2 * t], x2 = g.tx[2 * t + 1];
    double s = 0.0;
    for (int q = threadIdx.x; q < g.M; q += 256) {
        double a[5], b[5];
        const double e = pair_tables(k, x1 - g.px[q], x2 - g.py[q], a, b);
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

// ---- multi-functional extension (extend_fn_kernel): the row functional F in place of delta ------------------------------------------------
// sum_b pair_coeff_p<F, f[b]> c[b] (c[b] = 0 outside block b)
template <int L, int F>
__device__ __forceinline__ double fn_sum(const double (&a)[5], const double (&b)[5], const double (&c)[4]) {
#pragma clang fp contract(off)
    double v = pair_coeff_p<F, Lay<L>::f[0]>(a, b) * c[0];
    if (Lay<L>::nb > 1) v += pair_coeff_p<F, Lay<L>::f[1]>(a, b) * c[1];
    if (Lay<L>::nb > 2) v += pair_coeff_p<F, Lay<L>::f[2]>(a, b) * c[2];
    if (Lay<L>::nb > 3) v += pair_coeff_p<F, Lay<L>::f[3]>(a, b) * c[3];
    return v;
}

// (without contraction: a mask and its single-bit calls accumulate a functional through the same roundings)
template <int L, int MASK, int F>
__device__ __forceinline__ void fn_acc(double (&s)[fn_popc(MASK)], const double (&a)[5], const double (&b)[5], const double (&c)[4], double e) {
#pragma clang fp contract(off)
    if ((MASK >> F) & 1) s[fn_row(MASK, F)] += fn_sum<L, F>(a, b, c) * e;
}

template <int L, int MASK>
__global__ __launch_bounds__(256) void periodic_extend_fn_kernel(FnArgs g, PerArgs k) {
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
            double a[5], b[5];
            const double e = pair_tables(k, x1[i] - y1, x2[i] - y2, a, b);
            fn_acc<L, MASK, F_DELTA>(s[i], a, b, c, e);
            fn_acc<L, MASK, F_D1>(s[i], a, b, c, e);
            fn_acc<L, MASK, F_D2>(s[i], a, b, c, e);
            fn_acc<L, MASK, F_DD2>(s[i], a, b, c, e);
            fn_acc<L, MASK, F_LAP>(s[i], a, b, c, e);
        }
    }
    GPK_FN_REDUCE_STORE(s, NF, t0, g.Nt, g.out, g.ldo);
}

}  // namespace

void gpk_i_periodic_gram(int layout, bool pairs, int nt, hipStream_t st, const AsmArgs& g, const PerArgs& k) {
    const dim3 grid(gpk_ceil_div(g.M, 256), gpk_ceil_div(g.M, TP)), grid2(gpk_ceil_div(g.M / 2, 256), gpk_ceil_div(g.M, TP));
    with_layout(layout, [&](auto l) {
        constexpr int L = decltype(l)::value;
        if (!pairs) periodic_assemble_kernel<L><<<grid, 256, 0, st>>>(g, k);
        else if (nt == 1) periodic_assemble2_kernel<L, 1><<<grid2, 256, 0, st>>>(g, k);
        else periodic_assemble2_kernel<L, 0><<<grid2, 256, 0, st>>>(g, k);
    });
}

void gpk_i_periodic_test(int layout, hipStream_t st, const AsmArgs& g, const PerArgs& k) {
    const dim3 grid(gpk_ceil_div(g.M, 256), gpk_ceil_div(g.Nt, TP));
    with_layout(layout, [&](auto l) { periodic_assemble_test_kernel<decltype(l)::value><<<grid, 256, 0, st>>>(g, k); });
}

void gpk_i_periodic_cross(int layout, bool wide, hipStream_t st, const AsmArgs& g, const PerArgs& k) {
    const dim3 grid(gpk_ceil_div(gpk_ceil_div(g.Nt, 2), 256), gpk_ceil_div(g.M, CROSS_TP));
    with_layout(layout, [&](auto l) {
        constexpr int L = decltype(l)::value;
        if (wide) periodic_assemble_cross_kernel<L, true><<<grid, 256, 0, st>>>(g, k);
        else periodic_assemble_cross_kernel<L, false><<<grid, 256, 0, st>>>(g, k);
    });
}

void gpk_i_periodic_prior(bool wide, hipStream_t st, const PriorArgs& g, const PerArgs& k) {
    const dim3 grid(gpk_ceil_div(gpk_ceil_div(g.nb, 2), 256), gpk_ceil_div(g.na, CROSS_TP));
    if (wide) periodic_assemble_prior_kernel<true><<<grid, 256, 0, st>>>(g, k);
    else periodic_assemble_prior_kernel<false><<<grid, 256, 0, st>>>(g, k);
}

void gpk_i_periodic_extend(int layout, hipStream_t st, const AsmArgs& g, const PerArgs& k) {
    with_layout(layout, [&](auto l) { periodic_extend_kernel<decltype(l)::value><<<g.Nt, 256, 0, st>>>(g, k); });
}

// one instantiation per (layout, mask)
void gpk_i_periodic_extend_fn(int layout, int mask, hipStream_t st, const FnArgs& g, const PerArgs& k) {
    const int grid = gpk_ceil_div(g.Nt, FN_TT);
    with_layout(layout, [&](auto l) {
        with_mask<31>(mask, [&](auto m) {
            periodic_extend_fn_kernel<decltype(l)::value, decltype(m)::value><<<grid, 256, 0, st>>>(g, k);
        });
    });
}

void gpk_i_periodic_diag(int layout, const PerArgs& k, double (&c)[4]) {
    double a[5], b[5];
    const PerAxis& x = k.ax[0];
    const PerAxis& y = k.ax[1];
    a[0] = 1.0; a[1] = 0.0; a[2] = -x.p; a[3] = 0.0; a[4] = x.p * (3.0 * x.p + x.w2);
    b[0] = 1.0; b[1] = 0.0; b[2] = -y.p; b[3] = 0.0; b[4] = y.p * (3.0 * y.p + y.w2);
    with_layout(layout, [&](auto l) {
        constexpr int L = decltype(l)::value;
        c[0] = pair_coeff_p<Lay<L>::f[0], Lay<L>::f[0]>(a, b);
        c[1] = pair_coeff_p<Lay<L>::f[1], Lay<L>::f[1]>(a, b);
        c[2] = pair_coeff_p<Lay<L>::f[2], Lay<L>::f[2]>(a, b);
        c[3] = pair_coeff_p<Lay<L>::f[3], Lay<L>::f[3]>(a, b);
    });
}
