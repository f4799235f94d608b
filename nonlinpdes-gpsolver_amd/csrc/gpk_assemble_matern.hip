// gpk_assemble_matern.hip -- the Matern family (nu = 5/2, 7/2, 9/2) in the fused Gram evaluator of the reference layouts.
//
// The mathematics of the family and its policy; the kernels are the frames of gpk_assemble_frames.h -- one-point and two-point Gram
// kernel, test rows, cross columns, prior, extension, multi-functional extension -- instantiated here for the three orders and exported
// as a table (gpk_i_family_matern, gpk_assemble_ref.h), through which the entry points of gpk_assemble.hip launch them.  A translation
// unit of its own: nothing here is seen by the compiler when it generates the Gaussian kernels.
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
#include "gpk_assemble_frames.h"

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

// The policy of nu = M + 1/2 (gpk_assemble_frames.h).  The partials carry the whole entry: there is no weight to factor out, so the
// extension kernels sum entry * c.  The products with c and the sums of the frames stay outside the pragma, as they always were.
template <int M>
struct Matern {
    struct State { double D[5][5]; };
    static constexpr bool write_through = false;

    __host__ __device__ __forceinline__ static void eval(double r1, double r2, double d1, double d2, State& s) {
        matern_partials<M>(r1, r2, d1, d2, s.D);
    }
    __device__ __forceinline__ static void eval2(double r1, double r2, double d1a, double d2a, State& s0, double d1b, double d2b, State& s1) {
        eval(r1, r2, d1a, d2a, s0);
        eval(r1, r2, d1b, d2b, s1);
    }
    template <int FX, int FY>
    __host__ __device__ __forceinline__ static double entry(const State& s) { return pair_coeff_m<FX, FY>(s.D); }
    template <int FX, int FY>
    __device__ __forceinline__ static double scaled(const State& s, double c) { return pair_coeff_m<FX, FY>(s.D) * c; }
    __device__ __forceinline__ static double weigh(const State&, double v) { return v; }
    __device__ __forceinline__ static double weigh_fn(const State&, double v) { return v; }
    // Only D[0][0] = G_0 is used, so the rest of matern_partials is dead code here: one sqrt and one exp per pair.  G_0 depends on d
    // through squares alone (even in d to the bit), and at d = 0 it is theta_m(0) / theta_m(0) = 1.
    __device__ __forceinline__ static double prior(double r1, double r2, double d1, double d2) {
        State s;
        eval(r1, r2, d1, d2, s);
        return entry<F_DELTA, F_DELTA>(s);
    }
    static void at_zero(double r1, double r2, State& s) { eval(r1, r2, 0.0, 0.0, s); }
};

// the order of the parameters becomes the policy type
struct MaternFamily {
    template <class F> static void with(const KernelParams& k, F&& f) {
        switch (k.m) {
            case 2: f(Matern<2>{}); break;
            case 3: f(Matern<3>{}); break;
            default: f(Matern<4>{}); break;
        }
    }
};

}  // namespace

const Family gpk_i_family_matern = family_of<MaternFamily>();
