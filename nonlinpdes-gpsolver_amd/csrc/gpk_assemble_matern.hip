// gpk_assemble_matern.hip -- the Matern family (nu = 5/2, 7/2, 9/2) in the fused Gram evaluator of the reference layouts.
//
// One counterpart for each kernel shape of gpk_assemble.hip -- one-point and two-point Gram kernel, test rows, cross columns, extension,
// multi-functional extension -- with the same lane-to-point mapping, the same store pattern and the same fixed-order reductions; the
// entry points of gpk_assemble.hip choose the family on the host and launch these through gpk_assemble_ref.h.  A translation unit of its
// own: nothing here is seen by the compiler when it generates the Gaussian kernels.
//
// Math (DESIGN.md §K "Matern kernels").  nu = m + 1/2, a^2 = 2 nu, u_i = (x_i - y_i) / rho_i, t = a |u|, theta_j the reverse Bessel
// polynomials.  kappa = phi(s), s = |u|^2 / 2, and
//   phi^(k)(s) = (-a^2)^k exp(-t) theta_{m-k}(t) / theta_m(0),  theta_{-j}(t) = theta_{j-1}(t) / t^{2j-1},
// so that with G_k = phi^(k) the chain rule gives every partial in d = x - y the functionals need (n1 + n2 <= 4):
//   P[n1][n2] = sum_{j1 <= n1/2, j2 <= n2/2} c(n1,j1) c(n2,j2) G_{n1+n2-j1-j2} u1^{n1-2j1} u2^{n2-2j2},  c(n,j) = n! / (j! (n-2j)! 2^j),
//   d_x^alpha d_y^beta kappa = (-1)^{|beta|} rho_1^{-n1} rho_2^{-n2} P[n1][n2],  n = alpha + beta.
// ONE sqrt and ONE exp per point pair give G_0..G_4, which feed every block of the layout.
//
// Coincident and nearly coincident points.  G_3 (m = 2) and G_4 (m = 2, 3) are singular at t = 0: theta_{-1} = 1/t, theta_{-2} = (1+t)/t^3.
// G_3 only ever multiplies monomials of degree >= 2 and G_4 monomials of degree 4, so with the unit direction n_i = u_i / |u|
//   m = 2:  G_3 u_a u_b = -(a^5/3) e^{-t} n_a u_b,   G_4 u_a u_b u_c u_d = (a^5/3) e^{-t} (1 + t) n_a n_b n_c u_d,
//   m = 3:  G_4 u_a u_b u_c u_d = (a^7/15) e^{-t} n_a u_b u_c u_d:
// bounded factors (|n_i| <= 1) times factors that vanish with t -- no 0/0, no overflow.  At |u| = 0 the direction is taken as 0 and
// these terms are exactly 0, their limit.
//
// Every kernel computes the partials with the same bits for the same point pair: the per-pair arithmetic is written with explicit fma
// and compiled without contraction (as the bc / op evaluators, gpk_assemble_common.h), so the 8-byte and the 16-byte store paths agree.
#include "gpk_assemble_ref.h"

using namespace gpk_asm;

namespace {

template <int M> struct Mat;
template <> struct Mat<2> { static constexpr double a2 = 5.0, a = 2.23606797749978969641, th0 = 3.0; };
template <> struct Mat<3> { static constexpr double a2 = 7.0, a = 2.64575131106459059050, th0 = 15.0; };
template <> struct Mat<4> { static constexpr double a2 = 9.0, a = 3.0, th0 = 105.0; };

// coefficient of t^j in theta_n, n = 0..4
__host__ __device__ constexpr double theta_c(int n, int j) {
    constexpr double c[5][5] = {{1, 0, 0, 0, 0}, {1, 1, 0, 0, 0}, {3, 3, 1, 0, 0}, {15, 15, 6, 1, 0}, {105, 105, 45, 10, 1}};
    return c[n][j];
}
__host__ __device__ constexpr double ipow(double x, int n) { return n <= 0 ? 1.0 : x * ipow(x, n - 1); }

// G_k / e^{-t} for k <= m: (-a^2)^k theta_{m-k}(t) / theta_m(0), Horner in t with the constants folded at compile time
template <int M, int K>
__host__ __device__ __forceinline__ double g_poly(double t) {
#pragma clang fp contract(off)
    constexpr int n = M - K;
    constexpr double s = ipow(-Mat<M>::a2, K) / Mat<M>::th0;
    double v = s * theta_c(n, n);
#pragma unroll
    for (int j = n - 1; j >= 0; --j) v = __builtin_fma(v, t, s * theta_c(n, j));
    return v;
}

// D[n1][n2] = d_{d1}^{n1} d_{d2}^{n2} kappa for n1 + n2 <= 4 (the other entries are not written), r_i = 1 / rho_i.  Everything is
// inlined into straight-line code, so an entry that no block of the layout uses costs nothing.
template <int M>
__host__ __device__ __forceinline__ void matern_partials(double r1, double r2, double d1, double d2, double (&D)[5][5]) {
#pragma clang fp contract(off)
    const double x = d1 * r1, y = d2 * r2;
    const double xx = x * x, yy = y * y, xy = x * y;
    const double w = __builtin_fma(y, y, xx);
    const double un = sqrt(w);                                       // |u|
    const double t = Mat<M>::a * un;
    const double e = exp(-t);
    const double G0 = e * g_poly<M, 0>(t), G1 = e * g_poly<M, 1>(t), G2 = e * g_poly<M, 2>(t);
    // T3ab = G_3 u_a u_b,  T4[i] = G_4 x^{4-i} y^i
    double T3xx, T3xy, T3yy, T40, T31, T22, T13, T04;
    if constexpr (M == 4) {
        const double G3 = e * g_poly<M, 3>(t), G4 = e * g_poly<M, 4>(t);
        T3xx = G3 * xx; T3xy = G3 * xy; T3yy = G3 * yy;
        T40 = G4 * (xx * xx); T31 = G4 * (xx * xy); T22 = G4 * (xx * yy); T13 = G4 * (xy * yy); T04 = G4 * (yy * yy);
    } else {
        const double inv = w > 0.0 ? 1.0 / un : 0.0;                 // direction n = u / |u|; 0 at coincident points: the limit of every term below
        const double nx = x * inv, ny = y * inv;
        const double qxx = nx * x, qxy = nx * y, qyy = ny * y;       // u_a u_b / |u|
        if constexpr (M == 3) {
            const double G3 = e * g_poly<M, 3>(t);
            constexpr double k4 = ipow(Mat<M>::a2, 3) * Mat<M>::a / Mat<M>::th0;      // a^7 / theta_3(0)
            const double K4 = k4 * e;
            T3xx = G3 * xx; T3xy = G3 * xy; T3yy = G3 * yy;
            T40 = K4 * (qxx * xx); T31 = K4 * (qxx * xy); T22 = K4 * (qxx * yy); T13 = K4 * (qyy * xy); T04 = K4 * (qyy * yy);
        } else {
            constexpr double k3 = ipow(Mat<M>::a2, 2) * Mat<M>::a / Mat<M>::th0;      // a^5 / theta_2(0)
            const double K3 = -k3 * e;
            const double K4 = (k3 * e) * (1.0 + t);
            T3xx = K3 * qxx; T3xy = K3 * qxy; T3yy = K3 * qyy;
            const double nxx = nx * nx, nxy = nx * ny, nyy = ny * ny;
            T40 = K4 * (nxx * qxx); T31 = K4 * (nxx * qxy); T22 = K4 * (nxy * qxy); T13 = K4 * (nyy * qxy); T04 = K4 * (nyy * qyy);
        }
    }
    const double r11 = r1 * r1, r22 = r2 * r2, r12 = r1 * r2;
    D[0][0] = G0;
    D[1][0] = r1 * (G1 * x);
    D[0][1] = r2 * (G1 * y);
    D[2][0] = r11 * __builtin_fma(G2, xx, G1);
    D[1][1] = r12 * (G2 * xy);
    D[0][2] = r22 * __builtin_fma(G2, yy, G1);
    D[3][0] = (r11 * r1) * (x * __builtin_fma(3.0, G2, T3xx));
    D[2][1] = (r11 * r2) * (y * (T3xx + G2));
    D[1][2] = (r22 * r1) * (x * (T3yy + G2));
    D[0][3] = (r22 * r2) * (y * __builtin_fma(3.0, G2, T3yy));
    D[4][0] = (r11 * r11) * (T40 + __builtin_fma(6.0, T3xx, 3.0 * G2));
    D[3][1] = (r11 * r12) * __builtin_fma(3.0, T3xy, T31);
    D[2][2] = (r11 * r22) * (T22 + ((T3xx + T3yy) + G2));
    D[1][3] = (r22 * r12) * __builtin_fma(3.0, T3xy, T13);
    D[0][4] = (r22 * r22) * (T04 + __builtin_fma(6.0, T3yy, 3.0 * G2));
}

// <FX applied in x, FY applied in y>: sum over the multi-indices of (-1)^{|beta|} D[alpha + beta]
template <int FX, int FY>
__host__ __device__ __forceinline__ double pair_coeff_m(const double (&D)[5][5]) {
#pragma clang fp contract(off)
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < f_count(FX); ++i) {
#pragma unroll
        for (int j = 0; j < f_count(FY); ++j) {
            const double t = D[f_a1(FX, i) + f_a1(FY, j)][f_a2(FX, i) + f_a2(FY, j)];
            if ((f_a1(FY, j) + f_a2(FY, j)) & 1) s -= t; else s += t;
        }
    }
    return s;
}

// ---- Gram kernels: the frames of assemble_kernel / assemble2_kernel (gpk_assemble.hip) -----------------------------------------------
template <int L, int BI, int BJ>
__device__ __forceinline__ void store_block(const AsmArgs& g, int p, int q, const double (&D)[5][5]) {
    if (q < g.size[BJ]) {
        double v = pair_coeff_m<Lay<L>::f[BI], Lay<L>::f[BJ]>(D);
        if (BI == BJ && p == q) v += g.nug[BI];
        g.out[(long)(g.off[BI] + p) * g.ld + g.off[BJ] + q] = v;
    }
}

template <int L, int BI>
__device__ __forceinline__ void store_row(const AsmArgs& g, int p, int q, const double (&D)[5][5]) {
    if (p < g.size[BI]) {                               // wave-uniform
        store_block<L, BI, 0>(g, p, q, D);
        if (Lay<L>::nb > 1) store_block<L, BI, 1>(g, p, q, D);
        if (Lay<L>::nb > 2) store_block<L, BI, 2>(g, p, q, D);
        if (Lay<L>::nb > 3) store_block<L, BI, 3>(g, p, q, D);
    }
}

template <int L, int BI, int BJ, int NT>
__device__ __forceinline__ void store_block2(const AsmArgs& g, int p, int q, const double (&D0)[5][5], const double (&D1)[5][5]) {
    if (q < g.size[BJ]) {                                            // (sizes are even here: q and q + 1 are both inside or both outside)
        double v0 = pair_coeff_m<Lay<L>::f[BI], Lay<L>::f[BJ]>(D0);
        double v1 = pair_coeff_m<Lay<L>::f[BI], Lay<L>::f[BJ]>(D1);
        if (BI == BJ) { if (p == q) v0 += g.nug[BI]; if (p == q + 1) v1 += g.nug[BI]; }
        store2<NT>(g.out + (long)(g.off[BI] + p) * g.ld + g.off[BJ] + q, v0, v1);
    }
}

template <int L, int BI, int NT>
__device__ __forceinline__ void store_row2(const AsmArgs& g, int p, int q, const double (&D0)[5][5], const double (&D1)[5][5]) {
    if (p < g.size[BI]) {                               // wave-uniform
        store_block2<L, BI, 0, NT>(g, p, q, D0, D1);
        if (Lay<L>::nb > 1) store_block2<L, BI, 1, NT>(g, p, q, D0, D1);
        if (Lay<L>::nb > 2) store_block2<L, BI, 2, NT>(g, p, q, D0, D1);
        if (Lay<L>::nb > 3) store_block2<L, BI, 3, NT>(g, p, q, D0, D1);
    }
}

template <int M, int L, int NT>
__global__ __launch_bounds__(256) void matern_assemble2_kernel(AsmArgs g) {
    const int q = 2 * (blockIdx.x * 256 + threadIdx.x);
    const bool live = q < g.M;                                       // (M even: q + 1 < M as well)
    const double y1a = live ? g.px[q] : 0.0, y2a = live ? g.py[q] : 0.0;
    const double y1b = live ? g.px[q + 1] : 0.0, y2b = live ? g.py[q + 1] : 0.0;
    const int p0 = blockIdx.y * TP;
    const int pend = min(p0 + TP, g.M);
    for (int p = p0; p < pend; ++p) {
        const double x1 = g.px[p], x2 = g.py[p];        // uniform address -> scalar loads
        if (!live) continue;
        double D0[5][5], D1[5][5];
        matern_partials<M>(g.p1, g.p2, x1 - y1a, x2 - y2a, D0);
        matern_partials<M>(g.p1, g.p2, x1 - y1b, x2 - y2b, D1);
        store_row2<L, 0, NT>(g, p, q, D0, D1);
        if (Lay<L>::nb > 1) store_row2<L, 1, NT>(g, p, q, D0, D1);
        if (Lay<L>::nb > 2) store_row2<L, 2, NT>(g, p, q, D0, D1);
        if (Lay<L>::nb > 3) store_row2<L, 3, NT>(g, p, q, D0, D1);
    }
}

template <int M, int L>
__global__ __launch_bounds__(256) void matern_assemble_kernel(AsmArgs g) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    const bool live = q < g.M;
    const double y1 = live ? g.px[q] : 0.0, y2 = live ? g.py[q] : 0.0;
    const int p0 = blockIdx.y * TP;
    const int pend = min(p0 + TP, g.M);
    for (int p = p0; p < pend; ++p) {
        const double x1 = g.px[p], x2 = g.py[p];        // uniform address -> scalar loads
        if (!live) continue;
        double D[5][5];
        matern_partials<M>(g.p1, g.p2, x1 - y1, x2 - y2, D);
        store_row<L, 0>(g, p, q, D);
        if (Lay<L>::nb > 1) store_row<L, 1>(g, p, q, D);
        if (Lay<L>::nb > 2) store_row<L, 2>(g, p, q, D);
        if (Lay<L>::nb > 3) store_row<L, 3>(g, p, q, D);
    }
}

// ---- test rows: functional delta at the test point, column functionals of the layout (assemble_test_kernel) ---------------------------
template <int L, int BJ>
__device__ __forceinline__ void store_test(const AsmArgs& g, int t, int q, const double (&D)[5][5]) {
    if (q < g.size[BJ]) g.out[(long)t * g.ld + g.off[BJ] + q] = pair_coeff_m<F_DELTA, Lay<L>::f[BJ]>(D);
}

template <int M, int L>
__global__ __launch_bounds__(256) void matern_assemble_test_kernel(AsmArgs g) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= g.M) return;
    const double y1 = g.px[q], y2 = g.py[q];
    const int t0 = blockIdx.y * TP;
    const int tend = min(t0 + TP, g.Nt);
    for (int t = t0; t < tend; ++t) {
        double D[5][5];
        matern_partials<M>(g.p1, g.p2, g.tx[2 * t] - y1, g.tx[2 * t + 1] - y2, D);
        store_test<L, 0>(g, t, q, D);
        if (Lay<L>::nb > 1) store_test<L, 1>(g, t, q, D);
        if (Lay<L>::nb > 2) store_test<L, 2>(g, t, q, D);
        if (Lay<L>::nb > 3) store_test<L, 3>(g, t, q, D);
    }
}

// ---- cross-covariance columns: the test rows transposed, two test points per lane (assemble_cross_kernel) -----------------------------
template <int L, int BJ, bool WIDE>
__device__ __forceinline__ void store_cross(const AsmArgs& g, int p, int t, const double (&D0)[5][5], const double (&D1)[5][5]) {
    if (p < g.size[BJ]) {                               // wave-uniform
        const double v0 = pair_coeff_m<F_DELTA, Lay<L>::f[BJ]>(D0);
        const double v1 = pair_coeff_m<F_DELTA, Lay<L>::f[BJ]>(D1);
        double* const dst = g.out + (long)(g.off[BJ] + p) * g.ld + t;
        if constexpr (WIDE) store2<0>(dst, v0, v1);
        else { dst[0] = v0; if (t + 1 < g.Nt) dst[1] = v1; }
    }
}

template <int M, int L, bool WIDE>
__global__ __launch_bounds__(256) void matern_assemble_cross_kernel(AsmArgs g) {
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
        double D0[5][5], D1[5][5];
        matern_partials<M>(g.p1, g.p2, x1a - y1, x2a - y2, D0);
        matern_partials<M>(g.p1, g.p2, x1b - y1, x2b - y2, D1);
        store_cross<L, 0, WIDE>(g, p, t, D0, D1);
        if (Lay<L>::nb > 1) store_cross<L, 1, WIDE>(g, p, t, D0, D1);
        if (Lay<L>::nb > 2) store_cross<L, 2, WIDE>(g, p, t, D0, D1);
        if (Lay<L>::nb > 3) store_cross<L, 3, WIDE>(g, p, t, D0, D1);
    }
}

// ---- prior between two point sets: out[i * ld + j] = k(xa_i, xb_j) (assemble_prior_kernel) ---------------------------------------------
// Only D[0][0] = G_0 is used, so the rest of matern_partials is dead code here: one sqrt and one exp per pair.  G_0 depends on d through
// squares alone, so a square call (xa == xb) gives out[i][j] and out[j][i] the same bits, and at d = 0 it is theta_m(0) / theta_m(0) = 1.
template <int M, bool WIDE>
__global__ __launch_bounds__(256) void matern_assemble_prior_kernel(PriorArgs g) {
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
        double D0[5][5], D1[5][5];
        matern_partials<M>(g.p1, g.p2, x1 - y1a, x2 - y2a, D0);
        matern_partials<M>(g.p1, g.p2, x1 - y1b, x2 - y2b, D1);
        const double v0 = pair_coeff_m<F_DELTA, F_DELTA>(D0), v1 = pair_coeff_m<F_DELTA, F_DELTA>(D1);
        double* const dst = g.out + (long)i * g.ld + j;
        if constexpr (WIDE) store2<0>(dst, v0, v1);
        else { dst[0] = v0; if (j + 1 < g.nb) dst[1] = v1; }
    }
}

// ---- extension: out[t] = sum_c Theta_test[t, c] * coeff[c] (extend_kernel) --------------------------------------------------------------
template <int L, int BJ>
__device__ __forceinline__ double acc_test(const AsmArgs& g, int q, const double (&D)[5][5]) {
    return (q < g.size[BJ]) ? pair_coeff_m<F_DELTA, Lay<L>::f[BJ]>(D) * g.coeff[g.off[BJ] + q] : 0.0;
}

template <int M, int L>
__global__ __launch_bounds__(256) void matern_extend_kernel(AsmArgs g) {
    __shared__ double red[4];
    const int t = blockIdx.x;
    const double x1 = g.tx[2 * t], x2 = g.tx[2 * t + 1];
    double s = 0.0;
    for (int q = threadIdx.x; q < g.M; q += 256) {
        double D[5][5];
        matern_partials<M>(g.p1, g.p2, x1 - g.px[q], x2 - g.py[q], D);
        double v = acc_test<L, 0>(g, q, D);
        if (Lay<L>::nb > 1) v += acc_test<L, 1>(g, q, D);
        if (Lay<L>::nb > 2) v += acc_test<L, 2>(g, q, D);
        if (Lay<L>::nb > 3) v += acc_test<L, 3>(g, q, D);
        s += v;
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) g.out[t] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- multi-functional extension (extend_fn_kernel): the row functional F in place of delta ------------------------------------------------
// sum_b pair_coeff_m<F, f[b]> c[b] (c[b] = 0 outside block b)
template <int L, int F>
__device__ __forceinline__ double fn_sum(const double (&D)[5][5], const double (&c)[4]) {
    double v = pair_coeff_m<F, Lay<L>::f[0]>(D) * c[0];
    if (Lay<L>::nb > 1) v += pair_coeff_m<F, Lay<L>::f[1]>(D) * c[1];
    if (Lay<L>::nb > 2) v += pair_coeff_m<F, Lay<L>::f[2]>(D) * c[2];
    if (Lay<L>::nb > 3) v += pair_coeff_m<F, Lay<L>::f[3]>(D) * c[3];
    return v;
}

template <int L, int MASK, int F>
__device__ __forceinline__ void fn_acc(double (&s)[fn_popc(MASK)], const double (&D)[5][5], const double (&c)[4]) {
    if ((MASK >> F) & 1) s[fn_row(MASK, F)] += fn_sum<L, F>(D, c);
}

template <int M, int L, int MASK>
__global__ __launch_bounds__(256) void matern_extend_fn_kernel(FnArgs g) {
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
            double D[5][5];
            matern_partials<M>(g.p1, g.p2, x1[i] - y1, x2[i] - y2, D);
            fn_acc<L, MASK, F_DELTA>(s[i], D, c);
            fn_acc<L, MASK, F_D1>(s[i], D, c);
            fn_acc<L, MASK, F_D2>(s[i], D, c);
            fn_acc<L, MASK, F_DD2>(s[i], D, c);
            fn_acc<L, MASK, F_LAP>(s[i], D, c);
        }
    }
    GPK_FN_REDUCE_STORE(s, NF, t0, g.Nt, g.out, g.ldo);
}

// f(std::integral_constant<int, M>) for m = 2, 3, 4 (the callers pass matern_order of a Matern id)
template <class F>
void with_order(int m, F&& f) {
    switch (m) {
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 3: f(std::integral_constant<int, 3>{}); break;
        default: f(std::integral_constant<int, 4>{}); break;
    }
}

// f(M, L) as integral constants
template <class F>
void with_order_layout(int m, int layout, F&& f) {
    with_order(m, [&](auto mm) { with_layout(layout, [&](auto l) { f(mm, l); }); });
}

}  // namespace

void gpk_i_matern_gram(int m, int layout, bool pairs, int nt, hipStream_t st, const AsmArgs& g) {
    const dim3 grid(gpk_ceil_div(g.M, 256), gpk_ceil_div(g.M, TP)), grid2(gpk_ceil_div(g.M / 2, 256), gpk_ceil_div(g.M, TP));
    with_order_layout(m, layout, [&](auto mm, auto l) {
        constexpr int M = decltype(mm)::value, L = decltype(l)::value;
        if (!pairs) matern_assemble_kernel<M, L><<<grid, 256, 0, st>>>(g);
        else if (nt == 1) matern_assemble2_kernel<M, L, 1><<<grid2, 256, 0, st>>>(g);
        else matern_assemble2_kernel<M, L, 0><<<grid2, 256, 0, st>>>(g);
    });
}

void gpk_i_matern_test(int m, int layout, hipStream_t st, const AsmArgs& g) {
    const dim3 grid(gpk_ceil_div(g.M, 256), gpk_ceil_div(g.Nt, TP));
    with_order_layout(m, layout, [&](auto mm, auto l) {
        matern_assemble_test_kernel<decltype(mm)::value, decltype(l)::value><<<grid, 256, 0, st>>>(g);
    });
}

void gpk_i_matern_cross(int m, int layout, bool wide, hipStream_t st, const AsmArgs& g) {
    const dim3 grid(gpk_ceil_div(gpk_ceil_div(g.Nt, 2), 256), gpk_ceil_div(g.M, CROSS_TP));
    with_order_layout(m, layout, [&](auto mm, auto l) {
        constexpr int M = decltype(mm)::value, L = decltype(l)::value;
        if (wide) matern_assemble_cross_kernel<M, L, true><<<grid, 256, 0, st>>>(g);
        else matern_assemble_cross_kernel<M, L, false><<<grid, 256, 0, st>>>(g);
    });
}

void gpk_i_matern_prior(int m, bool wide, hipStream_t st, const PriorArgs& g) {
    const dim3 grid(gpk_ceil_div(gpk_ceil_div(g.nb, 2), 256), gpk_ceil_div(g.na, CROSS_TP));
    with_order(m, [&](auto mm) {
        constexpr int M = decltype(mm)::value;
        if (wide) matern_assemble_prior_kernel<M, true><<<grid, 256, 0, st>>>(g);
        else matern_assemble_prior_kernel<M, false><<<grid, 256, 0, st>>>(g);
    });
}

void gpk_i_matern_extend(int m, int layout, hipStream_t st, const AsmArgs& g) {
    with_order_layout(m, layout, [&](auto mm, auto l) {
        matern_extend_kernel<decltype(mm)::value, decltype(l)::value><<<g.Nt, 256, 0, st>>>(g);
    });
}

// one instantiation per (nu, layout, mask)
void gpk_i_matern_extend_fn(int m, int layout, int mask, hipStream_t st, const FnArgs& g) {
    const int grid = gpk_ceil_div(g.Nt, FN_TT);
    with_order_layout(m, layout, [&](auto mm, auto l) {
        with_mask<31>(mask, [&](auto k) {
            matern_extend_fn_kernel<decltype(mm)::value, decltype(l)::value, decltype(k)::value><<<grid, 256, 0, st>>>(g);
        });
    });
}

void gpk_i_matern_diag(int m, int layout, double r1, double r2, double (&c)[4]) {
    with_order_layout(m, layout, [&](auto mm, auto l) {
        constexpr int M = decltype(mm)::value, L = decltype(l)::value;
        double D[5][5];
        matern_partials<M>(r1, r2, 0.0, 0.0, D);
        c[0] = pair_coeff_m<Lay<L>::f[0], Lay<L>::f[0]>(D);
        c[1] = pair_coeff_m<Lay<L>::f[1], Lay<L>::f[1]>(D);
        c[2] = pair_coeff_m<Lay<L>::f[2], Lay<L>::f[2]>(D);
        c[3] = pair_coeff_m<Lay<L>::f[3], Lay<L>::f[3]>(D);
    });
}
