// gpk_assemble_frames.h -- the kernel frames of the reference layouts, each once: one-point and two-point Gram kernel, test rows, cross
// columns, prior, extension, multi-functional extension, with their store and accumulate helpers and their launches.  Lane-to-point
// mapping, grids, bounds, store pattern and reduction are the same for every kernel family; what a family computes per point pair is
// its policy P, and each of gpk_assemble.hip, gpk_assemble_matern.hip and gpk_assemble_periodic.hip instantiates the frames for its own
// policies in its own translation unit and exports them as a Family (gpk_assemble_ref.h).
//
// A policy supplies (K...: what its kernels take beside the argument struct -- nothing, or PerArgs):
//   State                                    what one point pair yields (two 5-entry tables and kappa; the 5 x 5 table of partials)
//   eval(p1, p2, d1, d2, State&, K...)       its evaluation at d = x - y
//   eval2(p1, p2, d1a, d2a, State&, d1b, d2b, State&, K...)   two pairs (the two-point frames), in the order the family wants them
//   entry<FX, FY>(State)                     <FX applied in x, FY applied in y> of the kernel: a Theta entry
//   scaled<FX, FY>(State, c)                 the term of the extension kernels: c times the entry, without the weight below
//   weigh(State, v), weigh_fn(State, v)      v times the weight that the entries of a pair have in common (kappa), applied once to the
//                                            sum over the blocks (extension, multi-functional extension); v itself where there is none
//   prior(p1, p2, d1, d2, K...)              the kernel's value, as the prior frame stores it
//   at_zero(p1, p2, State&, K...)            (host) State at d = 0 for the trace ratios
//   write_through                            whether the store policies 2 / 3 of gpk_tune key 55 are instantiated
// Every floating-point operation of a family's arithmetic stands in its policy functions, which carry the contraction pragmas where
// the family needs them; the frames themselves only add the nugget and accumulate, under the including file's default.
#pragma once
#include "gpk_assemble_ref.h"

namespace gpk_asm {

// ---- Gram kernels --------------------------------------------------------------------------------------------------------------------
// Mapping to the hardware: a workgroup owns TP row points x 256 column points.  Lane <-> column point, so for a fixed (row functional,
// column functional, row point) the 64 lanes of a wave store 512 contiguous bytes; the row point is wave-uniform (scalar loads, no LDS
// needed: 16 B per point).  One evaluation per POINT PAIR feeds every block that pair contributes to (up to 16 entries).
template <class P, int L, int BI, int BJ>
__device__ __forceinline__ void store_block(const AsmArgs& g, int p, int q, const typename P::State& s) {
    if (q < g.size[BJ]) {
        double v = P::template entry<Lay<L>::f[BI], Lay<L>::f[BJ]>(s);
        if (BI == BJ && p == q) v += g.nug[BI];
        g.out[(long)(g.off[BI] + p) * g.ld + g.off[BJ] + q] = v;
    }
}

template <class P, int L, int BI>
__device__ __forceinline__ void store_row(const AsmArgs& g, int p, int q, const typename P::State& s) {
    if (p < g.size[BI]) {                               // wave-uniform
        store_block<P, L, BI, 0>(g, p, q, s);
        if (Lay<L>::nb > 1) store_block<P, L, BI, 1>(g, p, q, s);
        if (Lay<L>::nb > 2) store_block<P, L, BI, 2>(g, p, q, s);
        if (Lay<L>::nb > 3) store_block<P, L, BI, 3>(g, p, q, s);
    }
}

// Two column points per lane, one 16-byte store per (row functional, column functional, row point): a wave writes 1 KB contiguous
// per store instruction and issues half as many of them.  Needs every block offset, the leading dimension and the base address to
// be even multiples of 8 bytes (checked by the launcher; otherwise the one-point-per-lane kernel below runs).  NT: the store policy of
// store2 (gpk_tune key 55).
template <class P, int L, int BI, int BJ, int NT>
__device__ __forceinline__ void store_block2(const AsmArgs& g, int p, int q, const typename P::State& s0, const typename P::State& s1) {
    if (q < g.size[BJ]) {                                            // (sizes are even here: q and q + 1 are both inside or both outside)
        double v0 = P::template entry<Lay<L>::f[BI], Lay<L>::f[BJ]>(s0);
        double v1 = P::template entry<Lay<L>::f[BI], Lay<L>::f[BJ]>(s1);
        if (BI == BJ) { if (p == q) v0 += g.nug[BI]; if (p == q + 1) v1 += g.nug[BI]; }
        store2<NT>(g.out + (long)(g.off[BI] + p) * g.ld + g.off[BJ] + q, v0, v1);
    }
}

template <class P, int L, int BI, int NT>
__device__ __forceinline__ void store_row2(const AsmArgs& g, int p, int q, const typename P::State& s0, const typename P::State& s1) {
    if (p < g.size[BI]) {                               // wave-uniform
        store_block2<P, L, BI, 0, NT>(g, p, q, s0, s1);
        if (Lay<L>::nb > 1) store_block2<P, L, BI, 1, NT>(g, p, q, s0, s1);
        if (Lay<L>::nb > 2) store_block2<P, L, BI, 2, NT>(g, p, q, s0, s1);
        if (Lay<L>::nb > 3) store_block2<P, L, BI, 3, NT>(g, p, q, s0, s1);
    }
}

template <class P, int L, int NT, class... K>
__global__ __launch_bounds__(256) void assemble2_kernel(AsmArgs g, K... k) {
    const int q = 2 * (blockIdx.x * 256 + threadIdx.x);
    const bool live = q < g.M;                                       // (M even: q + 1 < M as well)
    const double y1a = live ? g.px[q] : 0.0, y2a = live ? g.py[q] : 0.0;
    const double y1b = live ? g.px[q + 1] : 0.0, y2b = live ? g.py[q + 1] : 0.0;
    const int p0 = blockIdx.y * TP;
    const int pend = min(p0 + TP, g.M);
    for (int p = p0; p < pend; ++p) {
        const double x1 = g.px[p], x2 = g.py[p];        // uniform address -> scalar loads
        if (!live) continue;
        typename P::State s0, s1;
        P::eval2(g.p1, g.p2, x1 - y1a, x2 - y2a, s0, x1 - y1b, x2 - y2b, s1, k...);
        store_row2<P, L, 0, NT>(g, p, q, s0, s1);
        if (Lay<L>::nb > 1) store_row2<P, L, 1, NT>(g, p, q, s0, s1);
        if (Lay<L>::nb > 2) store_row2<P, L, 2, NT>(g, p, q, s0, s1);
        if (Lay<L>::nb > 3) store_row2<P, L, 3, NT>(g, p, q, s0, s1);
    }
}

template <class P, int L, class... K>
__global__ __launch_bounds__(256) void assemble_kernel(AsmArgs g, K... k) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    const bool live = q < g.M;
    const double y1 = live ? g.px[q] : 0.0, y2 = live ? g.py[q] : 0.0;
    const int p0 = blockIdx.y * TP;
    const int pend = min(p0 + TP, g.M);
    for (int p = p0; p < pend; ++p) {
        const double x1 = g.px[p], x2 = g.py[p];        // uniform address -> scalar loads
        if (!live) continue;
        typename P::State s;
        P::eval(g.p1, g.p2, x1 - y1, x2 - y2, s, k...);
        store_row<P, L, 0>(g, p, q, s);
        if (Lay<L>::nb > 1) store_row<P, L, 1>(g, p, q, s);
        if (Lay<L>::nb > 2) store_row<P, L, 2>(g, p, q, s);
        if (Lay<L>::nb > 3) store_row<P, L, 3>(g, p, q, s);
    }
}

// ---- test rows: functional delta at the test point, column functionals of the layout ----------------------------------------------------
template <class P, int L, int BJ>
__device__ __forceinline__ void store_test(const AsmArgs& g, int t, int q, const typename P::State& s) {
    if (q < g.size[BJ]) g.out[(long)t * g.ld + g.off[BJ] + q] = P::template entry<F_DELTA, Lay<L>::f[BJ]>(s);
}

template <class P, int L, class... K>
__global__ __launch_bounds__(256) void assemble_test_kernel(AsmArgs g, K... k) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= g.M) return;
    const double y1 = g.px[q], y2 = g.py[q];
    const int t0 = blockIdx.y * TP;
    const int tend = min(t0 + TP, g.Nt);
    for (int t = t0; t < tend; ++t) {
        typename P::State s;
        P::eval(g.p1, g.p2, g.tx[2 * t] - y1, g.tx[2 * t + 1] - y2, s, k...);
        store_test<P, L, 0>(g, t, q, s);
        if (Lay<L>::nb > 1) store_test<P, L, 1>(g, t, q, s);
        if (Lay<L>::nb > 2) store_test<P, L, 2>(g, t, q, s);
        if (Lay<L>::nb > 3) store_test<P, L, 3>(g, t, q, s);
    }
}

// ---- cross-covariance columns (gpk_assemble_cross) --------------------------------------------------------------------------------------
// The entries of assemble_test_kernel, transposed -- out[(off[BJ] + p) * ld + t] for the column point p of block BJ and the test point
// t.  Lanes run along t, two test points per lane (t, t + 1): for a fixed (block, column point) a wave stores 1 KB contiguous with the
// 16-byte store (WIDE: base and ld even, Nt even), or the same two values as two 8-byte stores (any alignment, odd Nt).  One kernel
// body for both: the values are the same bits either way.  The column point is wave-uniform (scalar loads), and one evaluation per
// point pair feeds every block of the layout.
template <class P, int L, int BJ, bool WIDE>
__device__ __forceinline__ void store_cross(const AsmArgs& g, int p, int t, const typename P::State& s0, const typename P::State& s1) {
    if (p < g.size[BJ]) {                               // wave-uniform
        const double v0 = P::template entry<F_DELTA, Lay<L>::f[BJ]>(s0);
        const double v1 = P::template entry<F_DELTA, Lay<L>::f[BJ]>(s1);
        double* const dst = g.out + (long)(g.off[BJ] + p) * g.ld + t;
        if constexpr (WIDE) store2<0>(dst, v0, v1);
        else { dst[0] = v0; if (t + 1 < g.Nt) dst[1] = v1; }
    }
}

template <class P, int L, bool WIDE, class... K>
__global__ __launch_bounds__(256) void assemble_cross_kernel(AsmArgs g, K... k) {
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
        typename P::State s0, s1;
        P::eval2(g.p1, g.p2, x1a - y1, x2a - y2, s0, x1b - y1, x2b - y2, s1, k...);
        store_cross<P, L, 0, WIDE>(g, p, t, s0, s1);
        if (Lay<L>::nb > 1) store_cross<P, L, 1, WIDE>(g, p, t, s0, s1);
        if (Lay<L>::nb > 2) store_cross<P, L, 2, WIDE>(g, p, t, s0, s1);
        if (Lay<L>::nb > 3) store_cross<P, L, 3, WIDE>(g, p, t, s0, s1);
    }
}

// ---- prior between two point sets (gpk_assemble_prior) ----------------------------------------------------------------------------------
// out[i * ld + j] = k(xa_i, xb_j), the value functional on both sides.  The shape of assemble_cross_kernel: lanes along j, two columns
// per lane (16-byte store when WIDE, the same two values as 8-byte stores otherwise), the row point wave-uniform (scalar loads), a
// workgroup owns 512 columns x CROSS_TP rows.  Write-bound: 8 na nb bytes.  Every entry is computed from its own d = xa_i - xb_j by a
// P::prior that is even in d to the bit: the two columns of a lane and the two triangles of a square call (xa == xb) go through the
// same roundings, so out[i][j] and out[j][i] are the same bits and the diagonal is 1.
template <class P, bool WIDE, class... K>
__global__ __launch_bounds__(256) void assemble_prior_kernel(PriorArgs g, K... k) {
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
        const double v0 = P::prior(g.p1, g.p2, x1 - y1a, x2 - y2a, k...);
        const double v1 = P::prior(g.p1, g.p2, x1 - y1b, x2 - y2b, k...);
        double* const dst = g.out + (long)i * g.ld + j;
        if constexpr (WIDE) store2<0>(dst, v0, v1);
        else { dst[0] = v0; if (j + 1 < g.nb) dst[1] = v1; }
    }
}

// ---- extension: out[t] = sum_c Theta_test[t, c] * coeff[c]; one workgroup per test point, lanes stride over column points -------------
template <class P, int L, int BJ>
__device__ __forceinline__ double acc_test(const AsmArgs& g, int q, const typename P::State& s) {
    return (q < g.size[BJ]) ? P::template scaled<F_DELTA, Lay<L>::f[BJ]>(s, g.coeff[g.off[BJ] + q]) : 0.0;
}

template <class P, int L, class... K>
__global__ __launch_bounds__(256) void extend_kernel(AsmArgs g, K... k) {
    __shared__ double red[4];
    const int t = blockIdx.x;
    const double x1 = g.tx[2 * t], x2 = g.tx[2 * t + 1];
    double s = 0.0;
    for (int q = threadIdx.x; q < g.M; q += 256) {
        typename P::State st;
        P::eval(g.p1, g.p2, x1 - g.px[q], x2 - g.py[q], st, k...);
        double v = acc_test<P, L, 0>(g, q, st);
        if (Lay<L>::nb > 1) v += acc_test<P, L, 1>(g, q, st);
        if (Lay<L>::nb > 2) v += acc_test<P, L, 2>(g, q, st);
        if (Lay<L>::nb > 3) v += acc_test<P, L, 3>(g, q, st);
        s += P::weigh(st, v);
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) g.out[t] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- multi-functional extension (DESIGN.md §K "Row functionals of the extension") ------------------------------------------------
// out[k][t] = sum_b sum_q <F_k, f[b]> k(x_t, y_q) c[off_b + q], F_k over the functionals of MASK (bit F = functional F: delta, d1, d2,
// d2^2, Laplacian; the GPK_FN_* bits of gpk.h).  Every row functional has per-axis order <= 2 and so has every column functional: the
// State of the Gram kernels serves, and ONE evaluation per point pair feeds all of them.  Mapping: a workgroup owns FN_TT test points
// (wave-uniform: scalar loads) and its 256 lanes stride over the column points as in extend_kernel; each column point's coordinates
// and its nb coefficient slices are loaded once and serve all FN_TT test points, and each lane keeps FN_TT x popcount(MASK)
// accumulators.  Points, zeroing and reduction: the frame of gpk_assemble_common.h.
// sum_b scaled<F, f[b]>(c[b]) (c[b] = 0 outside block b, as acc_test in extend_kernel)
template <class P, int L, int F>
__device__ __forceinline__ double fn_sum(const typename P::State& st, const double (&c)[4]) {
    double v = P::template scaled<F, Lay<L>::f[0]>(st, c[0]);
    if (Lay<L>::nb > 1) v += P::template scaled<F, Lay<L>::f[1]>(st, c[1]);
    if (Lay<L>::nb > 2) v += P::template scaled<F, Lay<L>::f[2]>(st, c[2]);
    if (Lay<L>::nb > 3) v += P::template scaled<F, Lay<L>::f[3]>(st, c[3]);
    return v;
}

template <class P, int L, int MASK, int F>
__device__ __forceinline__ void fn_acc(double (&s)[fn_popc(MASK)], const typename P::State& st, const double (&c)[4]) {
    if ((MASK >> F) & 1) s[fn_row(MASK, F)] += P::weigh_fn(st, fn_sum<P, L, F>(st, c));
}

template <class P, int L, int MASK, class... K>
__global__ __launch_bounds__(256) void extend_fn_kernel(FnArgs g, K... k) {
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
            typename P::State st;
            P::eval(g.p1, g.p2, x1[i] - y1, x2[i] - y2, st, k...);
            fn_acc<P, L, MASK, F_DELTA>(s[i], st, c);
            fn_acc<P, L, MASK, F_D1>(s[i], st, c);
            fn_acc<P, L, MASK, F_D2>(s[i], st, c);
            fn_acc<P, L, MASK, F_DD2>(s[i], st, c);
            fn_acc<P, L, MASK, F_LAP>(s[i], st, c);
        }
    }
    GPK_FN_REDUCE_STORE(s, NF, t0, g.Nt, g.out, g.ldo);
}

// ---- launches on stream st: the grid of each frame, in one place (k: the tail of the family's kernels) -----------------------------------
template <class P, class... K>
void launch_gram(int layout, bool pairs, int nt, hipStream_t st, const AsmArgs& g, const K&... k) {
    const dim3 grid(gpk_ceil_div(g.M, 256), gpk_ceil_div(g.M, TP)), grid2(gpk_ceil_div(g.M / 2, 256), gpk_ceil_div(g.M, TP));
    with_layout(layout, [&](auto l) {
        constexpr int L = decltype(l)::value;
        const int policy = (nt == 1 || (P::write_through && (nt == 2 || nt == 3))) ? nt : 0;
        if (!pairs) assemble_kernel<P, L><<<grid, 256, 0, st>>>(g, k...);
        else if (policy == 1) assemble2_kernel<P, L, 1><<<grid2, 256, 0, st>>>(g, k...);
        else if (policy == 0) assemble2_kernel<P, L, 0><<<grid2, 256, 0, st>>>(g, k...);
        else if constexpr (P::write_through) {
            if (policy == 2) assemble2_kernel<P, L, 2><<<grid2, 256, 0, st>>>(g, k...);
            else assemble2_kernel<P, L, 3><<<grid2, 256, 0, st>>>(g, k...);
        }
    });
}

template <class P, class... K>
void launch_test(int layout, hipStream_t st, const AsmArgs& g, const K&... k) {
    const dim3 grid(gpk_ceil_div(g.M, 256), gpk_ceil_div(g.Nt, TP));
    with_layout(layout, [&](auto l) { assemble_test_kernel<P, decltype(l)::value><<<grid, 256, 0, st>>>(g, k...); });
}

template <class P, class... K>
void launch_cross(int layout, bool wide, hipStream_t st, const AsmArgs& g, const K&... k) {
    const dim3 grid(gpk_ceil_div(gpk_ceil_div(g.Nt, 2), 256), gpk_ceil_div(g.M, CROSS_TP));
    with_layout(layout, [&](auto l) {
        constexpr int L = decltype(l)::value;
        if (wide) assemble_cross_kernel<P, L, true><<<grid, 256, 0, st>>>(g, k...);
        else assemble_cross_kernel<P, L, false><<<grid, 256, 0, st>>>(g, k...);
    });
}

template <class P, class... K>
void launch_prior(bool wide, hipStream_t st, const PriorArgs& g, const K&... k) {
    const dim3 grid(gpk_ceil_div(gpk_ceil_div(g.nb, 2), 256), gpk_ceil_div(g.na, CROSS_TP));
    if (wide) assemble_prior_kernel<P, true><<<grid, 256, 0, st>>>(g, k...);
    else assemble_prior_kernel<P, false><<<grid, 256, 0, st>>>(g, k...);
}

template <class P, class... K>
void launch_extend(int layout, hipStream_t st, const AsmArgs& g, const K&... k) {
    with_layout(layout, [&](auto l) { extend_kernel<P, decltype(l)::value><<<g.Nt, 256, 0, st>>>(g, k...); });
}

// one instantiation per (policy, layout, mask)
template <class P, class... K>
void launch_extend_fn(int layout, int mask, hipStream_t st, const FnArgs& g, const K&... k) {
    const int grid = gpk_ceil_div(g.Nt, FN_TT);
    with_layout(layout, [&](auto l) {
        with_mask<31>(mask, [&](auto m) { extend_fn_kernel<P, decltype(l)::value, decltype(m)::value><<<grid, 256, 0, st>>>(g, k...); });
    });
}

// value of <f_b, f_b> at d = 0 for the blocks of the layout
template <class P, class... K>
void diag_values(int layout, double p1, double p2, double (&c)[4], const K&... k) {
    typename P::State s;
    P::at_zero(p1, p2, s, k...);
    with_layout(layout, [&](auto l) {
        constexpr int L = decltype(l)::value;
        c[0] = P::template entry<Lay<L>::f[0], Lay<L>::f[0]>(s);
        c[1] = P::template entry<Lay<L>::f[1], Lay<L>::f[1]>(s);
        c[2] = P::template entry<Lay<L>::f[2], Lay<L>::f[2]>(s);
        c[3] = P::template entry<Lay<L>::f[3], Lay<L>::f[3]>(s);
    });
}

// The table of a family.  B::with(KernelParams, f) calls f(policy{}, tail...) with the policy and the kernel tail that the parameters
// select (the Matern order becomes the policy type there).
template <class B>
Family family_of() {
    return {
        [](int layout, bool pairs, int nt, hipStream_t st, const AsmArgs& g, const KernelParams& kp) {
            B::with(kp, [&](auto pol, const auto&... k) { launch_gram<decltype(pol)>(layout, pairs, nt, st, g, k...); });
        },
        [](int layout, hipStream_t st, const AsmArgs& g, const KernelParams& kp) {
            B::with(kp, [&](auto pol, const auto&... k) { launch_test<decltype(pol)>(layout, st, g, k...); });
        },
        [](int layout, bool wide, hipStream_t st, const AsmArgs& g, const KernelParams& kp) {
            B::with(kp, [&](auto pol, const auto&... k) { launch_cross<decltype(pol)>(layout, wide, st, g, k...); });
        },
        [](bool wide, hipStream_t st, const PriorArgs& g, const KernelParams& kp) {
            B::with(kp, [&](auto pol, const auto&... k) { launch_prior<decltype(pol)>(wide, st, g, k...); });
        },
        [](int layout, hipStream_t st, const AsmArgs& g, const KernelParams& kp) {
            B::with(kp, [&](auto pol, const auto&... k) { launch_extend<decltype(pol)>(layout, st, g, k...); });
        },
        [](int layout, int mask, hipStream_t st, const FnArgs& g, const KernelParams& kp) {
            B::with(kp, [&](auto pol, const auto&... k) { launch_extend_fn<decltype(pol)>(layout, mask, st, g, k...); });
        },
        [](int layout, const KernelParams& kp, double (&c)[4]) {
            B::with(kp, [&](auto pol, const auto&... k) { diag_values<decltype(pol)>(layout, kp.p[0], kp.p[1], c, k...); });
        },
    };
}

}  // namespace gpk_asm
