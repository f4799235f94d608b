// gpk_assemble_bc.hip -- the fused derivative-kernel evaluator of the 2-D elliptic layout with a first-order linear functional at every
// boundary point (Neumann, Robin, mixed) instead of delta: the Gram matrix and the matrix-free extension with derivatives.
//
// No reference call site: the reference's Gram_matrix_assembly / construct_Theta_test (src/Gram_matrice.py) put delta on the boundary
// rows (Dirichlet data only).  The method does not depend on which linear functional sits there; the dense factorisation, the
// Gauss-Newton system GPK_GN_ELLIPTIC and gpk_pde_residual only see a factor and a data vector, so the point-pair evaluator below is
// all a Neumann / Robin solve needs (src/PDEs.py, Nonlinear_elliptic2d(bc=...)).
//
// Math (DESIGN.md §K "Boundary functionals").  Every point q of the second block carries phi_q = c0 delta + c1 d_1 + c2 d_2: (1,0,0) at
// the Nd domain points, (beta, gamma n1, gamma n2) at the Nb boundary points.  With pair_coeff<F, G> of gpk_assemble.hip
// (d_x^alpha d_y^beta kappa = (-1)^{|alpha|} h_{a1+b1}(p1,d1) h_{a2+b2}(p2,d2) kappa) and PHI = {delta, d1, d2}:
//   <Lap, Lap'> = pair_coeff<Lap, Lap>                                     (unchanged)
//   <Lap, phi'> = sum_j c'_j pair_coeff<Lap, PHI_j>       <phi, Lap'> = sum_i c_i pair_coeff<PHI_i, Lap>
//   <phi, phi'> = sum_i c_i (sum_j c'_j pair_coeff<PHI_i, PHI_j>)
// Per-axis order <= 2 + 2: h0..h4 suffice, and one exp and one pair of Hermite evaluations per POINT PAIR feed all four blocks.
// With every coefficient (1,0,0) the sums collapse to the entries of GPK_LAYOUT_ELLIPTIC (products by 1 and 0 are exact).
//
// Mapping to the hardware, as assemble_kernel / assemble2_kernel: SoA-packed points AND coefficients in the handle's point scratch
// (5 arrays of Nd+Nb), a workgroup owns TP row points x 256 column points (two-point variant: x 512), lane <-> column point (its
// coordinates and three coefficients stay in registers), the row point and its coefficients are wave-uniform (scalar loads).
//
// Shared with the other evaluators (gpk_assemble_common.h): the functional tables, hermite_compensated and kappa2_fma (with
// gpk_assemble_op.hip: the same bits there), the frame of the extension kernel, store2 and the host side of a call (precisions,
// nugget, boundary trace, timing, launch).
#include "gpk_assemble_common.h"

using namespace gpk_asm;

// The pair evaluation shared by the one-point and the two-point evaluator is written with explicit fma and compiled without
// contraction (down to the extension kernels, which have one variant each): whether the compiler contracts a given a * b + c depends on
// how many uses the product has after inlining, which differs between the two evaluators -- and the two must give the same bits for
// the same point pair.  Written out, both fuse the same operations, and every rounding is one the error budget of DESIGN.md counts.
#pragma clang fp contract(off)

namespace {

// explicit-fma accumulation (gpk_assemble.hip has the plain form, which the compiler may contract: they round differently on purpose)
template <int FX, int FY>
__host__ __device__ __forceinline__ double pair_coeff(const double (&a)[5], const double (&b)[5]) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < f_count(FX); ++i) {
#pragma unroll
        for (int j = 0; j < f_count(FY); ++j) {
            const int n1 = f_a1(FX, i) + f_a1(FY, j);
            const int n2 = f_a2(FX, i) + f_a2(FY, j);
            const double t = ((f_a1(FX, i) + f_a2(FX, i)) & 1) ? -a[n1] : a[n1];      // (the sign of an odd row functional: exact)
            s = (i == 0 && j == 0) ? t * b[n2] : __builtin_fma(t, b[n2], s);
        }
    }
    return s;
}

// <F, phi'> / kappa: the column functional phi' = k[0] delta + k[1] d_1 + k[2] d_2 at y
template <int F>
__host__ __device__ __forceinline__ double coeff_f_phi(const double (&a)[5], const double (&b)[5], const double (&k)[3]) {
    return __builtin_fma(k[2], pair_coeff<F, F_D2>(a, b), __builtin_fma(k[1], pair_coeff<F, F_D1>(a, b), k[0] * pair_coeff<F, F_DELTA>(a, b)));
}

// <phi, F'> / kappa: the row functional phi = r[0] delta + r[1] d_1 + r[2] d_2 at x
template <int F>
__host__ __device__ __forceinline__ double coeff_phi_f(const double (&a)[5], const double (&b)[5], const double (&r)[3]) {
    return __builtin_fma(r[2], pair_coeff<F_D2, F>(a, b), __builtin_fma(r[1], pair_coeff<F_D1, F>(a, b), r[0] * pair_coeff<F_DELTA, F>(a, b)));
}

__host__ __device__ __forceinline__ double coeff_phi_phi(const double (&a)[5], const double (&b)[5], const double (&r)[3],
                                                         const double (&k)[3]) {
    return __builtin_fma(r[2], coeff_f_phi<F_D2>(a, b, k), __builtin_fma(r[1], coeff_f_phi<F_D1>(a, b, k), r[0] * coeff_f_phi<F_DELTA>(a, b, k)));
}

struct BcArgs {
    const double* px; const double* py;                     // SoA points: domain first, then boundary
    const double* c0; const double* c1; const double* c2;   // SoA coefficients of phi, same order
    int Nd, M;                                              // M = Nd + Nb
    double p1, p2;
    double* out; long ld;
    double nug[2];
};

// domain points carry (1,0,0); boundary point b carries bc[3b..3b+2], or (1,0,0) when bc == NULL
__global__ void pack_bc_kernel(const double* __restrict__ Xd, int Nd, const double* __restrict__ Xb, int Nb, const double* __restrict__ bc,
                               double* __restrict__ px, double* __restrict__ py, double* __restrict__ c0, double* __restrict__ c1,
                               double* __restrict__ c2) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < Nd) {
        px[i] = Xd[2 * i]; py[i] = Xd[2 * i + 1];
        c0[i] = 1.0; c1[i] = 0.0; c2[i] = 0.0;
    } else if (i < Nd + Nb) {
        const int b = i - Nd;
        px[i] = Xb[2 * b]; py[i] = Xb[2 * b + 1];
        c0[i] = bc ? bc[3 * b] : 1.0; c1[i] = bc ? bc[3 * b + 1] : 0.0; c2[i] = bc ? bc[3 * b + 2] : 0.0;
    }
}

// everything one point pair contributes: d = x - y, row coefficients r (at x), column coefficients k (at y)
struct PairBc {
    double a[5], b[5], e;
    __device__ __forceinline__ void eval(double p1, double p2, double d1, double d2) {
        e = kappa2_fma(p1, p2, d1, d2);
        hermite_compensated(p1, d1, a);
        hermite_compensated(p2, d2, b);
    }
    __device__ __forceinline__ double lap_lap() const { return pair_coeff<F_LAP, F_LAP>(a, b) * e; }
    __device__ __forceinline__ double lap_phi(const double (&k)[3]) const { return coeff_f_phi<F_LAP>(a, b, k) * e; }
    __device__ __forceinline__ double phi_lap(const double (&r)[3]) const { return coeff_phi_f<F_LAP>(a, b, r) * e; }
    __device__ __forceinline__ double phi_phi(const double (&r)[3], const double (&k)[3]) const { return coeff_phi_phi(a, b, r, k) * e; }
};

// one column point per lane, 8-byte stores: any alignment, any Nd / Nb
__global__ __launch_bounds__(256) void assemble_bc_kernel(BcArgs g) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    const bool live = q < g.M;
    const double y1 = live ? g.px[q] : 0.0, y2 = live ? g.py[q] : 0.0;
    const double k[3] = {live ? g.c0[q] : 0.0, live ? g.c1[q] : 0.0, live ? g.c2[q] : 0.0};
    const int p0 = blockIdx.y * TP;
    const int pend = min(p0 + TP, g.M);
    double* const col_lap = g.out + q;                      // column q of the Laplacian block (q < Nd only)
    double* const col_phi = g.out + g.Nd + q;               // column q of the phi block
    for (int p = p0; p < pend; ++p) {
        const double x1 = g.px[p], x2 = g.py[p];            // uniform address -> scalar loads
        const double r[3] = {g.c0[p], g.c1[p], g.c2[p]};
        if (!live) continue;
        PairBc u;
        u.eval(g.p1, g.p2, x1 - y1, x2 - y2);
        if (p < g.Nd) {                                     // wave-uniform: row p of the Laplacian block
            const long row = (long)p * g.ld;
            if (q < g.Nd) col_lap[row] = u.lap_lap() + (p == q ? g.nug[0] : 0.0);
            col_phi[row] = u.lap_phi(k);
        }
        const long row = (long)(g.Nd + p) * g.ld;           // row p of the phi block (p < M always)
        if (q < g.Nd) col_lap[row] = u.phi_lap(r);
        col_phi[row] = u.phi_phi(r, k) + (p == q ? g.nug[1] : 0.0);
    }
}

// Two column points per lane, one 16-byte store per (row block, column block, row point).  Needs Nd, Nb and the leading dimension
// even and a 16-byte aligned base (checked by the launcher; otherwise the one-point-per-lane kernel above runs).
// NT: the policy of store2 (0 plain, 1 non-temporal).

template <int NT>
__global__ __launch_bounds__(256) void assemble_bc2_kernel(BcArgs g) {
    const int q = 2 * (blockIdx.x * 256 + threadIdx.x);
    const bool live = q < g.M;                              // (M even: q + 1 < M as well)
    const double y1a = live ? g.px[q] : 0.0, y2a = live ? g.py[q] : 0.0;
    const double y1b = live ? g.px[q + 1] : 0.0, y2b = live ? g.py[q + 1] : 0.0;
    const double ka[3] = {live ? g.c0[q] : 0.0, live ? g.c1[q] : 0.0, live ? g.c2[q] : 0.0};
    const double kb[3] = {live ? g.c0[q + 1] : 0.0, live ? g.c1[q + 1] : 0.0, live ? g.c2[q + 1] : 0.0};
    const int p0 = blockIdx.y * TP;
    const int pend = min(p0 + TP, g.M);
    double* const col_lap = g.out + q;                      // (Nd even: q and q + 1 are both inside the Laplacian block or both outside)
    double* const col_phi = g.out + g.Nd + q;
    for (int p = p0; p < pend; ++p) {
        const double x1 = g.px[p], x2 = g.py[p];            // uniform address -> scalar loads
        const double r[3] = {g.c0[p], g.c1[p], g.c2[p]};
        if (!live) continue;
        PairBc u0, u1;
        u0.eval(g.p1, g.p2, x1 - y1a, x2 - y2a);
        u1.eval(g.p1, g.p2, x1 - y1b, x2 - y2b);
        if (p < g.Nd) {                                     // wave-uniform
            const long row = (long)p * g.ld;
            if (q < g.Nd)
                store2<NT>(col_lap + row, u0.lap_lap() + (p == q ? g.nug[0] : 0.0), u1.lap_lap() + (p == q + 1 ? g.nug[0] : 0.0));
            store2<NT>(col_phi + row, u0.lap_phi(ka), u1.lap_phi(kb));
        }
        const long row = (long)(g.Nd + p) * g.ld;
        if (q < g.Nd) store2<NT>(col_lap + row, u0.phi_lap(r), u1.phi_lap(r));
        store2<NT>(col_phi + row, u0.phi_phi(r, ka) + (p == q ? g.nug[1] : 0.0), u1.phi_phi(r, kb) + (p == q + 1 ? g.nug[1] : 0.0));
    }
}

#pragma clang fp contract(fast)            // one variant per mask below: nothing to keep identical, the compiler may fuse

// ---- multi-functional extension (DESIGN.md §K "Boundary functionals") ------------------------------------------------------------
// out[f][t] = sum_q <F_f at x_t, Lap at y_q> kappa c[q] + sum_q <F_f at x_t, phi_q> kappa c[Nd + q], F_f over the functionals of
// MASK (the GPK_FN_* bits: delta, d1, d2, d2^2, Laplacian).  Mapping as every extension kernel (the frame of gpk_assemble_common.h): a workgroup owns FN_TT
// test points (wave-uniform), its 256 lanes stride over the column points; a column point's coordinates, its three coefficients and
// its two slices of c are loaded once and serve all FN_TT test points (the coefficients enter as w_j = c'_j c[Nd + q], formed once per
// column point); each lane keeps FN_TT x popcount(MASK) accumulators.  Reduction by wave shuffles, then LDS across the 4 waves, in a
// fixed order (no atomics: a repeated call gives bit-identical output).

struct FnBcArgs {
    const double* px; const double* py;
    const double* c0; const double* c1; const double* c2;
    int Nd, M;
    double p1, p2;
    const double* tx; int Nt;             // (Nt,2) row-major test points
    const double* coeff;                  // (2 Nd + Nb): Laplacian block, then phi block
    double* out; long ldo;
};

template <int MASK, int F>
__device__ __forceinline__ void fn_acc(double (&s)[fn_popc(MASK)], const double (&a)[5], const double (&b)[5], double cl,
                                       const double (&w)[3], double e) {
    if ((MASK >> F) & 1) s[fn_row(MASK, F)] += (pair_coeff<F, F_LAP>(a, b) * cl + coeff_f_phi<F>(a, b, w)) * e;
}

template <int MASK>
__global__ __launch_bounds__(256) void extend_fn_bc_kernel(FnBcArgs g) {
    constexpr int NF = fn_popc(MASK);
    const int t0 = blockIdx.x * FN_TT;
    double x1[FN_TT], x2[FN_TT], s[FN_TT][NF];
    GPK_FN_LOAD_POINTS2(x1, x2, g.tx, t0, g.Nt);
    fn_zero(s);
    for (int q = threadIdx.x; q < g.M; q += 256) {
        const double y1 = g.px[q], y2 = g.py[q];
        const double cl = q < g.Nd ? g.coeff[q] : 0.0;               // Laplacian block: domain points only
        const double cd = g.coeff[g.Nd + q];                         // phi block: every point
        const double w[3] = {g.c0[q] * cd, g.c1[q] * cd, g.c2[q] * cd};
#pragma unroll
        for (int i = 0; i < FN_TT; ++i) {
            const double d1 = x1[i] - y1, d2 = x2[i] - y2;
            const double e = exp(-0.5 * __builtin_fma(g.p2 * d2, d2, g.p1 * d1 * d1));
            double a[5], b[5];
            hermite_compensated(g.p1, d1, a);
            hermite_compensated(g.p2, d2, b);
            fn_acc<MASK, F_DELTA>(s[i], a, b, cl, w, e);
            fn_acc<MASK, F_D1>(s[i], a, b, cl, w, e);
            fn_acc<MASK, F_D2>(s[i], a, b, cl, w, e);
            fn_acc<MASK, F_DD2>(s[i], a, b, cl, w, e);
            fn_acc<MASK, F_LAP>(s[i], a, b, cl, w, e);
        }
    }
    GPK_FN_REDUCE_STORE(s, NF, t0, g.Nt, g.out, g.ldo);
}

// one instantiation per mask (31)
void launch_extend_fn_bc(int mask, int grid, hipStream_t st, const FnBcArgs& g) {
    with_mask<31>(mask, [&](auto m) { extend_fn_bc_kernel<decltype(m)::value><<<grid, 256, 0, st>>>(g); });
}

// precisions, packed points and coefficients (the handle's point scratch: 5 arrays of Nd + Nb, re-packed by every call)
int fill_common_bc(gpk_handle h, const char* who, int kernel, const double* kp, const double* Xd, int Nd, const double* Xb, int Nb,
                   const double* bc, double (&p)[2], const double* (&arr)[5]) {
    if (Nd <= 0 || Nb < 0 || !kp || !Xd || (Nb > 0 && !Xb)) return gpk_bad_arg(h, who);
    GPK_TRY(precisions(h, "assemble_bc: kernel id", kernel, kp, 2, p));   // (this text from gpk_extend_functionals_bc as well)
    const size_t Mall = (size_t)Nd + (size_t)Nb;
    GPK_TRY(gpk_i_ensure_points(h, 5 * Mall));
    double* s = h->d_pts;
    for (int k = 0; k < 5; ++k) arr[k] = s + k * Mall;
    pack_bc_kernel<<<gpk_ceil_div((int)Mall, 256), 256, 0, h->stream>>>(Xd, Nd, Xb, Nb, bc, s, s + Mall, s + 2 * Mall, s + 3 * Mall,
                                                                         s + 4 * Mall);
    GPK_LAUNCH_CHECK(h);
    return 0;
}

}  // namespace


extern "C" int gpk_assemble_bc(gpk_handle h, int kernel, const double* kp, const double* Xd, int Nd, const double* Xb, int Nb,
                               const double* bc, double nugget, int nugget_type, double* Theta, int ld, double* host_ratio) {
    if (!h || !Theta) return GPK_ERR_ARG;
    if (!nugget_type_valid(nugget_type)) return gpk_bad_arg(h, "assemble_bc: nugget_type");
    if ((long)2 * Nd + Nb > 0x7fffffffL) return gpk_bad_arg(h, "assemble_bc: N exceeds int");
    if (Nd > 0 && Nb >= 0 && ld < 2 * Nd + Nb) return gpk_bad_arg(h, "assemble_bc: ld < N");
    BcArgs g;
    double p[2];
    const double* arr[5];
    GPK_TRY(fill_common_bc(h, "assemble_bc: sizes/pointers", kernel, kp, Xd, Nd, Xb, Nb, bc, p, arr));
    g.px = arr[0]; g.py = arr[1]; g.c0 = arr[2]; g.c1 = arr[3]; g.c2 = arr[4];
    g.p1 = p[0]; g.p2 = p[1];
    g.Nd = Nd; g.M = Nd + Nb;
    // values at d = 0: <Lap, Lap> = 3 p1^2 + 2 p1 p2 + 3 p2^2 and <phi, phi> = c0^2 + p1 c1^2 + p2 c2^2 (1 at a domain point), so
    // trace(block 1) = Nd + sum_b (c0_b^2 + p1 c1_b^2 + p2 c2_b^2): the boundary sum is taken on the host from the coefficient array, in
    // index order and in long double, so that the returned ratio is the analytic value to an ulp and the same on every call.
    const long double q1 = p[0], q2 = p[1];
    long double trb;
    GPK_TRY(boundary_trace(h, bc, Nb, q1, q2, &trb));
    const long double tr0 = (long double)Nd * (3.0L * (q1 * q1 + q2 * q2) + 2.0L * q1 * q2);
    const double r0 = (double)(tr0 / ((long double)Nd + trb));   // trace(block 0) / trace(block 1)
    if (host_ratio) *host_ratio = r0;
    two_block_nugget(nugget_type, nugget, r0, g.nug);
    g.out = Theta; g.ld = ld;
    return launch_two_block(h, pairs_eligible(h, Theta, ld, Nd, Nb), g, assemble_bc_kernel, assemble_bc2_kernel<0>, assemble_bc2_kernel<1>);
}

extern "C" int gpk_extend_functionals_bc(gpk_handle h, int kernel, const double* kp, const double* Xt, int Nt,
                                         const double* Xd, int Nd, const double* Xb, int Nb, const double* bc,
                                         const double* coeff, int fmask, double* out, int ldo) {
    if (!h) return GPK_ERR_ARG;
    if (!out || !Xt || !coeff) return gpk_bad_arg(h, "extend_functionals_bc: pointers");
    if (fmask <= 0 || fmask > 31) return gpk_bad_arg(h, "extend_functionals_bc: fmask must be a non-empty subset of the GPK_FN_* bits");
    if (Nt <= 0) return gpk_bad_arg(h, "extend_functionals_bc: Nt <= 0");
    if (ldo < Nt) return gpk_bad_arg(h, "extend_functionals_bc: ldo < Nt");
    FnBcArgs g;
    double p[2];
    const double* arr[5];
    GPK_TRY(fill_common_bc(h, "extend_functionals_bc: sizes/pointers", kernel, kp, Xd, Nd, Xb, Nb, bc, p, arr));
    g.px = arr[0]; g.py = arr[1]; g.c0 = arr[2]; g.c1 = arr[3]; g.c2 = arr[4];
    g.p1 = p[0]; g.p2 = p[1];
    g.Nd = Nd; g.M = Nd + Nb;
    g.tx = Xt; g.Nt = Nt; g.coeff = coeff; g.out = out; g.ldo = ldo;
    launch_extend_fn_bc(fmask, gpk_ceil_div(Nt, FN_TT), h->stream, g);
    GPK_LAUNCH_CHECK(h);
    return 0;
}
