// gpk_assemble3d.hip -- the fused derivative-kernel evaluator in THREE space dimensions (HBM-write bound): the Gram matrix of the
// nonlinear elliptic equation on a box in R^3 and the matrix-free extension of its solution with derivatives.
//
// No reference call site: the reference's Gram_matrix_assembly / construct_Theta_test (src/Gram_matrice.py) are written for (n,2)
// points.  The method does not depend on the dimension; the dense factorisation, the Gauss-Newton system GPK_GN_ELLIPTIC and
// gpk_pde_residual are dimension-free, so the point-pair evaluator below is all a 3-D solve needs (src/PDEs.py, Nonlinear_elliptic3d).
//
// Math (DESIGN.md §K "Three dimensions").  kappa = exp(-(p1 d1^2 + p2 d2^2 + p3 d3^2)/2), d = x - y.  With the 1-D Hermite factors
//   h0 = 1, h1 = p d, h2 = p^2 d^2 - p, h3 = p^3 d^3 - 3 p^2 d, h4 = p^4 d^4 - 6 p^3 d^2 + 3 p^2
// (hermite_plain of gpk_assemble_common.h) every mixed partial is  d_x^alpha d_y^beta kappa = (-1)^{|alpha|} prod_k h_{alpha_k+beta_k}(p_k, d_k) kappa.
// Layout ELLIPTIC3D: block 0 = Laplacian = {(2,0,0), (0,2,0), (0,0,2)} on the Nd domain points, block 1 = delta on the Nd+Nb
// domain+boundary points, N = 2 Nd + Nb; <Lap, Lap> has nine terms.  One exp and three Hermite evaluations per POINT PAIR feed all
// four blocks.
//
// Mapping to the hardware, as in 2-D: SoA-packed points in the handle's point scratch, a workgroup owns TP row points x 256 column
// points (two-point variant: x 512), lane <-> column point, the row point is wave-uniform (scalar loads).  No inline assembly.
//
// Shared with the other evaluators (gpk_assemble_common.h): hermite_plain, the frame of the extension kernel, store2 and the host side
// of a call (precisions, nugget, timing, launch).
#include "gpk_assemble_common.h"

using namespace gpk_asm;

namespace {

enum { G_DELTA = 0, G_D1 = 1, G_D2 = 2, G_D3 = 3, G_LAP = 4 };

// multi-index lists of the five functionals: entry i of functional f has order g_ord(f, i, k) along axis k
__host__ __device__ constexpr int g_count(int f) { return f == G_LAP ? 3 : 1; }
__host__ __device__ constexpr int g_ord(int f, int i, int k) {
    return f == G_LAP ? (i == k ? 2 : 0) : ((f == G_D1 && k == 0) || (f == G_D2 && k == 1) || (f == G_D3 && k == 2) ? 1 : 0);
}
__host__ __device__ constexpr int g_total(int f, int i) { return g_ord(f, i, 0) + g_ord(f, i, 1) + g_ord(f, i, 2); }

template <int FX, int FY>
__host__ __device__ __forceinline__ double pair_coeff3(const double (&a)[5], const double (&b)[5], const double (&c)[5]) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < g_count(FX); ++i) {
#pragma unroll
        for (int j = 0; j < g_count(FY); ++j) {
            const double t = a[g_ord(FX, i, 0) + g_ord(FY, j, 0)] * b[g_ord(FX, i, 1) + g_ord(FY, j, 1)] * c[g_ord(FX, i, 2) + g_ord(FY, j, 2)];
            if (g_total(FX, i) & 1) s -= t; else s += t;
        }
    }
    return s;
}

__host__ __device__ __forceinline__ double kappa3(double p1, double p2, double p3, double d1, double d2, double d3) {
    return exp(-0.5 * (p1 * d1 * d1 + p2 * d2 * d2 + p3 * d3 * d3));
}

// the two blocks of ELLIPTIC3D: functional, and whether the block lives on domain points only (size Nd) or domain+boundary (Nd+Nb)
constexpr int LAY_F[2] = {G_LAP, G_DELTA};

struct Asm3Args {
    const double* px; const double* py; const double* pz;   // SoA points: domain first, then boundary
    int M;                                                  // Nd + Nb
    double p1, p2, p3;
    double* out; long ld;
    int off[2]; int size[2];
    double nug[2];
};

__global__ void pack_points3_kernel(const double* __restrict__ Xd, int Nd, const double* __restrict__ Xb, int Nb,
                                    double* __restrict__ px, double* __restrict__ py, double* __restrict__ pz) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < Nd) { px[i] = Xd[3 * i]; py[i] = Xd[3 * i + 1]; pz[i] = Xd[3 * i + 2]; }
    else if (i < Nd + Nb) { px[i] = Xb[3 * (i - Nd)]; py[i] = Xb[3 * (i - Nd) + 1]; pz[i] = Xb[3 * (i - Nd) + 2]; }
}

template <int BI, int BJ>
__device__ __forceinline__ void store_block(const Asm3Args& g, int p, int q, const double (&a)[5], const double (&b)[5],
                                            const double (&c)[5], double e) {
    if (q < g.size[BJ]) {
        double v = pair_coeff3<LAY_F[BI], LAY_F[BJ]>(a, b, c) * e;
        if (BI == BJ && p == q) v += g.nug[BI];
        g.out[(long)(g.off[BI] + p) * g.ld + g.off[BJ] + q] = v;
    }
}

__global__ __launch_bounds__(256) void assemble3d_kernel(Asm3Args g) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    const bool live = q < g.M;
    const double y1 = live ? g.px[q] : 0.0, y2 = live ? g.py[q] : 0.0, y3 = live ? g.pz[q] : 0.0;
    const int p0 = blockIdx.y * TP;
    const int pend = min(p0 + TP, g.M);
    for (int p = p0; p < pend; ++p) {
        const double x1 = g.px[p], x2 = g.py[p], x3 = g.pz[p];       // uniform address -> scalar loads
        if (!live) continue;
        const double d1 = x1 - y1, d2 = x2 - y2, d3 = x3 - y3;
        const double e = kappa3(g.p1, g.p2, g.p3, d1, d2, d3);
        double a[5], b[5], c[5];
        hermite_plain(g.p1, d1, a); hermite_plain(g.p2, d2, b); hermite_plain(g.p3, d3, c);
        if (p < g.size[0]) {                                          // wave-uniform
            store_block<0, 0>(g, p, q, a, b, c, e);
            store_block<0, 1>(g, p, q, a, b, c, e);
        }
        store_block<1, 0>(g, p, q, a, b, c, e);                      // (p < M = size[1] always)
        store_block<1, 1>(g, p, q, a, b, c, e);
    }
}

// Two column points per lane, one 16-byte store per (row functional, column functional, row point): a wave writes 1 KB contiguous
// per store instruction and issues half as many of them.  Needs every block offset and size, the leading dimension and the base
// address to be even multiples of 8 bytes (checked by the launcher; otherwise the one-point-per-lane kernel above runs).

struct Pair3 { double a[5], b[5], c[5], e; };

template <int BI, int BJ, int NT>
__device__ __forceinline__ void store_block2(const Asm3Args& g, int p, int q, const Pair3& u0, const Pair3& u1) {
    if (q < g.size[BJ]) {                                             // (sizes are even here: q and q + 1 are both inside or both outside)
        double v0 = pair_coeff3<LAY_F[BI], LAY_F[BJ]>(u0.a, u0.b, u0.c) * u0.e;
        double v1 = pair_coeff3<LAY_F[BI], LAY_F[BJ]>(u1.a, u1.b, u1.c) * u1.e;
        if (BI == BJ) { if (p == q) v0 += g.nug[BI]; if (p == q + 1) v1 += g.nug[BI]; }
        store2<NT>(g.out + (long)(g.off[BI] + p) * g.ld + g.off[BJ] + q, v0, v1);   // NT: 0 plain, 1 non-temporal (gpk_tune key 55)
    }
}

template <int NT>
__global__ __launch_bounds__(256) void assemble3d2_kernel(Asm3Args g) {
    const int q = 2 * (blockIdx.x * 256 + threadIdx.x);
    const bool live = q < g.M;                                        // (M even: q + 1 < M as well)
    const double y1a = live ? g.px[q] : 0.0, y2a = live ? g.py[q] : 0.0, y3a = live ? g.pz[q] : 0.0;
    const double y1b = live ? g.px[q + 1] : 0.0, y2b = live ? g.py[q + 1] : 0.0, y3b = live ? g.pz[q + 1] : 0.0;
    const int p0 = blockIdx.y * TP;
    const int pend = min(p0 + TP, g.M);
    for (int p = p0; p < pend; ++p) {
        const double x1 = g.px[p], x2 = g.py[p], x3 = g.pz[p];       // uniform address -> scalar loads
        if (!live) continue;
        Pair3 u0, u1;
        {
            const double d1 = x1 - y1a, d2 = x2 - y2a, d3 = x3 - y3a;
            u0.e = kappa3(g.p1, g.p2, g.p3, d1, d2, d3);
            hermite_plain(g.p1, d1, u0.a); hermite_plain(g.p2, d2, u0.b); hermite_plain(g.p3, d3, u0.c);
        }
        {
            const double d1 = x1 - y1b, d2 = x2 - y2b, d3 = x3 - y3b;
            u1.e = kappa3(g.p1, g.p2, g.p3, d1, d2, d3);
            hermite_plain(g.p1, d1, u1.a); hermite_plain(g.p2, d2, u1.b); hermite_plain(g.p3, d3, u1.c);
        }
        if (p < g.size[0]) {                                          // wave-uniform
            store_block2<0, 0, NT>(g, p, q, u0, u1);
            store_block2<0, 1, NT>(g, p, q, u0, u1);
        }
        store_block2<1, 0, NT>(g, p, q, u0, u1);
        store_block2<1, 1, NT>(g, p, q, u0, u1);
    }
}

// ---- multi-functional extension (DESIGN.md §K "Three dimensions") ----------------------------------------------------------------
// out[k][t] = sum_b sum_q pair_coeff3<F_k, f[b]>(h(p1,d1), h(p2,d2), h(p3,d3)) kappa(d) c[off_b + q], d = x_t - y_q, F_k over the
// functionals of the mask.  Row and column functionals have per-axis order <= 2: h0..h4 suffice and ONE exp serves every requested
// functional.  Mapping as every extension kernel (the frame of gpk_assemble_common.h): a workgroup owns FN_TT test points (wave-uniform), its 256 lanes
// stride over the column points, each lane keeps FN_TT x popcount(mask) accumulators; reduction by wave shuffles, then LDS across
// the 4 waves, in a fixed order (no atomics: a repeated call gives bit-identical output).
// CM is the COMPACT mask: bit k set = functional k of {delta, d1, d2, Laplacian, d3} -- the GPK_FN_* bits in ascending order with the
// unused bit GPK_FN_D2D2 squeezed out -- so output row order = ascending GPK_FN_* bit order.
constexpr int CM_F[5] = {G_DELTA, G_D1, G_D2, G_LAP, G_D3};

struct Fn3Args {
    const double* px; const double* py; const double* pz;
    int M, Nd;
    double p1, p2, p3;
    const double* tx; int Nt;             // (Nt,3) row-major test points
    const double* coeff;                  // (2 Nd + Nb): Laplacian block, then delta block
    double* out; long ldo;
};

template <int CM, int K>
__device__ __forceinline__ void fn_acc(double (&s)[fn_popc(CM)], const double (&a)[5], const double (&b)[5], const double (&c)[5],
                                       double cl, double cd, double e) {
    if ((CM >> K) & 1)
        s[fn_row(CM, K)] += (pair_coeff3<CM_F[K], G_LAP>(a, b, c) * cl + pair_coeff3<CM_F[K], G_DELTA>(a, b, c) * cd) * e;
}

template <int CM>
__global__ __launch_bounds__(256) void extend_fn3d_kernel(Fn3Args g) {
    constexpr int NF = fn_popc(CM);
    const int t0 = blockIdx.x * FN_TT;
    double x1[FN_TT], x2[FN_TT], x3[FN_TT], s[FN_TT][NF];
    GPK_FN_LOAD_POINTS3(x1, x2, x3, g.tx, t0, g.Nt);
    fn_zero(s);
    for (int q = threadIdx.x; q < g.M; q += 256) {
        const double y1 = g.px[q], y2 = g.py[q], y3 = g.pz[q];
        const double cl = q < g.Nd ? g.coeff[q] : 0.0;               // Laplacian block: domain points only
        const double cd = g.coeff[g.Nd + q];                         // delta block: every point
#pragma unroll
        for (int i = 0; i < FN_TT; ++i) {
            const double d1 = x1[i] - y1, d2 = x2[i] - y2, d3 = x3[i] - y3;
            const double e = kappa3(g.p1, g.p2, g.p3, d1, d2, d3);
            double a[5], b[5], c[5];
            hermite_plain(g.p1, d1, a); hermite_plain(g.p2, d2, b); hermite_plain(g.p3, d3, c);
            fn_acc<CM, 0>(s[i], a, b, c, cl, cd, e);
            fn_acc<CM, 1>(s[i], a, b, c, cl, cd, e);
            fn_acc<CM, 2>(s[i], a, b, c, cl, cd, e);
            fn_acc<CM, 3>(s[i], a, b, c, cl, cd, e);
            fn_acc<CM, 4>(s[i], a, b, c, cl, cd, e);
        }
    }
    GPK_FN_REDUCE_STORE(s, NF, t0, g.Nt, g.out, g.ldo);
}

// one instantiation per compact mask (31)
void launch_extend_fn3d(int cm, int grid, hipStream_t st, const Fn3Args& g) {
    with_mask<31>(cm, [&](auto m) { extend_fn3d_kernel<decltype(m)::value><<<grid, 256, 0, st>>>(g); });
}

// precisions, packed points
int fill_common3(gpk_handle h, const char* who, int kernel, const double* kp, const double* Xd, int Nd, const double* Xb, int Nb,
                 double (&p)[3], const double** px, const double** py, const double** pz) {
    if (Nd <= 0 || Nb < 0 || !kp || !Xd || (Nb > 0 && !Xb)) return gpk_bad_arg(h, who);
    GPK_TRY(precisions(h, "assemble3d: kernel id", kernel, kp, 3, p));
    const int Mall = Nd + Nb;
    GPK_TRY(gpk_i_ensure_points(h, 3 * (size_t)Mall));
    *px = h->d_pts; *py = h->d_pts + Mall; *pz = h->d_pts + 2 * (size_t)Mall;
    pack_points3_kernel<<<gpk_ceil_div(Mall, 256), 256, 0, h->stream>>>(Xd, Nd, Xb, Nb, h->d_pts, h->d_pts + Mall, h->d_pts + 2 * (size_t)Mall);
    GPK_LAUNCH_CHECK(h);
    return 0;
}

}  // namespace


extern "C" int gpk_assemble3d(gpk_handle h, int kernel, const double* kp, const double* Xd, int Nd, const double* Xb, int Nb,
                              double nugget, int nugget_type, double* Theta, int ld, double* host_ratio) {
    if (!h || !Theta) return GPK_ERR_ARG;
    if (!nugget_type_valid(nugget_type)) return gpk_bad_arg(h, "assemble3d: nugget_type");
    if ((long)2 * Nd + Nb > 0x7fffffffL) return gpk_bad_arg(h, "assemble3d: N exceeds int");
    Asm3Args g;
    double p[3];
    GPK_TRY(fill_common3(h, "assemble3d: sizes/pointers", kernel, kp, Xd, Nd, Xb, Nb, p, &g.px, &g.py, &g.pz));
    g.p1 = p[0]; g.p2 = p[1]; g.p3 = p[2];
    g.M = Nd + Nb;
    g.off[0] = 0; g.size[0] = Nd; g.off[1] = Nd; g.size[1] = Nd + Nb;
    const int N = 2 * Nd + Nb;
    if (ld < N) return gpk_bad_arg(h, "assemble3d: ld < N");
    // values of <f, f> at d = 0: <Lap, Lap> = 3 sum p_k^2 + sum_{i != j} p_i p_j, <delta, delta> = 1 -> the trace ratio is analytic.
    // Host scalar, evaluated in long double so that the returned ratio is the correctly rounded analytic value (to an ulp).
    const long double q1 = p[0], q2 = p[1], q3 = p[2];
    const long double c0 = 3.0L * (q1 * q1 + q2 * q2 + q3 * q3) + 2.0L * (q1 * q2 + q1 * q3 + q2 * q3);
    const double r0 = (double)(((long double)g.size[0] * c0) / (long double)g.size[1]);   // trace(block 0) / trace(block 1)
    if (host_ratio) *host_ratio = r0;
    two_block_nugget(nugget_type, nugget, r0, g.nug);
    g.out = Theta; g.ld = ld;
    return launch_two_block(h, pairs_eligible(h, Theta, ld, Nd, Nb), g, assemble3d_kernel, assemble3d2_kernel<0>, assemble3d2_kernel<1>);
}

extern "C" int gpk_extend_functionals3d(gpk_handle h, int kernel, const double* kp, const double* Xt, int Nt,
                                        const double* Xd, int Nd, const double* Xb, int Nb, const double* coeff, int fmask,
                                        double* out, int ldo) {
    if (!h) return GPK_ERR_ARG;
    if (!out || !Xt || !coeff) return gpk_bad_arg(h, "extend_functionals3d: pointers");
    const int accepted = GPK_FN_VALUE | GPK_FN_D1 | GPK_FN_D2 | GPK_FN_D3 | GPK_FN_LAPLACIAN;
    if (fmask <= 0 || (fmask & ~accepted))
        return gpk_bad_arg(h, "extend_functionals3d: fmask must be a non-empty subset of GPK_FN_VALUE | D1 | D2 | D3 | LAPLACIAN");
    if (Nt <= 0) return gpk_bad_arg(h, "extend_functionals3d: Nt <= 0");
    if (ldo < Nt) return gpk_bad_arg(h, "extend_functionals3d: ldo < Nt");
    Fn3Args g;
    double p[3];
    GPK_TRY(fill_common3(h, "extend_functionals3d: sizes/pointers", kernel, kp, Xd, Nd, Xb, Nb, p, &g.px, &g.py, &g.pz));
    g.p1 = p[0]; g.p2 = p[1]; g.p3 = p[2];
    g.M = Nd + Nb; g.Nd = Nd;
    g.tx = Xt; g.Nt = Nt; g.coeff = coeff; g.out = out; g.ldo = ldo;
    // compact mask: value, d1, d2 keep bits 0..2; Laplacian (16) -> bit 3, d3 (32) -> bit 4
    const int cm = (fmask & 7) | ((fmask & GPK_FN_LAPLACIAN) ? 8 : 0) | ((fmask & GPK_FN_D3) ? 16 : 0);
    launch_extend_fn3d(cm, gpk_ceil_div(Nt, FN_TT), h->stream, g);
    GPK_LAUNCH_CHECK(h);
    return 0;
}
