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
// The kernels are the frames of gpk_assemble_frames.h, instantiated here for the Gaussian policy below; the Matern family and the periodic
// kernel instantiate them in gpk_assemble_matern.hip and gpk_assemble_periodic.hip, and the entry points below launch whichever family
// the kernel id names through its table (gpk_assemble_ref.h).  The functional tables, the Hermite evaluation (hermite_plain), the
// 16-byte store and the host side of a call (precisions, nugget, timing) are shared with the other evaluators: gpk_assemble_common.h.
#include "gpk_assemble_frames.h"

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

// The Gaussian and the anisotropic Gaussian kernel: the Hermite tables of the two axes and kappa, an entry is pair_coeff(a, b) kappa.
// No pragma anywhere: the compiler may contract across these functions and the frames, as it always has here.
struct Gauss {
    struct State { double a[5], b[5], e; };
    static constexpr bool write_through = true;      // all four store policies of key 55 (measured here)

    __host__ __device__ __forceinline__ static void eval(double p1, double p2, double d1, double d2, State& s) {
        s.e = exp(-0.5 * (p1 * d1 * d1 + p2 * d2 * d2));
        hermite_plain(p1, d1, s.a);
        hermite_plain(p2, d2, s.b);
    }
    // both kappa first, then the tables: the order of the two-point kernels (register assignment follows it)
    __device__ __forceinline__ static void eval2(double p1, double p2, double d1a, double d2a, State& s0, double d1b, double d2b, State& s1) {
        s0.e = exp(-0.5 * (p1 * d1a * d1a + p2 * d2a * d2a));
        s1.e = exp(-0.5 * (p1 * d1b * d1b + p2 * d2b * d2b));
        hermite_plain(p1, d1a, s0.a); hermite_plain(p2, d2a, s0.b);
        hermite_plain(p1, d1b, s1.a); hermite_plain(p2, d2b, s1.b);
    }
    template <int FX, int FY>
    __host__ __device__ __forceinline__ static double entry(const State& s) { return pair_coeff<FX, FY>(s.a, s.b) * s.e; }
    // the extension kernels sum coefficient * c over the blocks and multiply by kappa once
    template <int FX, int FY>
    __device__ __forceinline__ static double scaled(const State& s, double c) { return pair_coeff<FX, FY>(s.a, s.b) * c; }
    __device__ __forceinline__ static double weigh(const State& s, double v) { return v * s.e; }
    __device__ __forceinline__ static double weigh_fn(const State& s, double v) { return v * s.e; }
    // kappa with the one fma written out (kappa2_fma): even in d to the bit, exp(-0) = 1 on the diagonal
    __device__ __forceinline__ static double prior(double p1, double p2, double d1, double d2) {
        double a[5], b[5];
        hermite_plain(p1, d1, a);
        hermite_plain(p2, d2, b);
        return pair_coeff<F_DELTA, F_DELTA>(a, b) * kappa2_fma(p1, p2, d1, d2);
    }
    static void at_zero(double p1, double p2, State& s) { eval(p1, p2, 0.0, 0.0, s); }

    template <class F> static void with(const KernelParams&, F&& f) { f(Gauss{}); }
};

__global__ void pack_points_kernel(const double* __restrict__ Xd, int Nd, const double* __restrict__ Xb, int Nb,
                                   double* __restrict__ px, double* __restrict__ py) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < Nd) { px[i] = Xd[2 * i]; py[i] = Xd[2 * i + 1]; }
    else if (i < Nd + Nb) { px[i] = Xb[2 * (i - Nd)]; py[i] = Xb[2 * (i - Nd) + 1]; }
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

// the family and its parameters, block offsets / sizes and the packed points: the fields AsmArgs and FnArgs share (the others are the
// caller's)
template <class Args>
int fill_common(gpk_handle h, Args& g, KernelParams& k, int layout, int kernel, const double* kp, const double* Xd, int Nd,
                const double* Xb, int Nb) {
    if (Nd <= 0 || Nb < 0 || !kp || !Xd) return gpk_bad_arg(h, "assemble: sizes/pointers");
    GPK_TRY(kernel_params(h, "assemble: kernel id", kernel, kp, k));
    g.p1 = k.p[0]; g.p2 = k.p[1];
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

}  // namespace

const Family gpk_i_family_gauss = family_of<Gauss>();

extern "C" int gpk_assemble(gpk_handle h, int layout, int kernel, const double* kp, const double* Xd, int Nd,
                            const double* Xb, int Nb, double nugget, int nugget_type, double* Theta, int ld,
                            double* ratios) {
    if (!h || !Theta) return GPK_ERR_ARG;
    AsmArgs g{};
    KernelParams k;
    GPK_TRY(fill_common(h, g, k, layout, kernel, kp, Xd, Nd, Xb, Nb));
    int nb = 0, N = 0;
    with_layout(layout, [&](auto l) {
        constexpr int L = decltype(l)::value;
        nb = Lay<L>::nb; N = lay_N<L>(Nd, Nb);
    });
    double c[4] = {0, 0, 0, 0};
    k.family->diag(layout, k, c);
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
    k.family->gram(layout, pairs, h->tune.asm_nt, h->stream, g, k);
    GPK_LAUNCH_CHECK(h);
    return 0;
}

extern "C" int gpk_assemble_test(gpk_handle h, int layout, int kernel, const double* kp, const double* Xt, int Nt,
                                 const double* Xd, int Nd, const double* Xb, int Nb, double* out, int ld) {
    if (!h) return GPK_ERR_ARG;
    if (!out || !Xt) return gpk_bad_arg(h, "assemble_test: pointers");
    if (Nt <= 0) return gpk_bad_arg(h, "assemble_test: Nt <= 0");
    AsmArgs g{};
    KernelParams k;
    GPK_TRY(fill_common(h, g, k, layout, kernel, kp, Xd, Nd, Xb, Nb));
    int N = 0;
    with_layout(layout, [&](auto l) { N = lay_N<decltype(l)::value>(Nd, Nb); });
    if (ld < N) return gpk_bad_arg(h, "assemble_test: ld < N");      // (rows would overlap and the last one leave the Nt x ld region)
    g.out = out; g.ld = ld; g.tx = Xt; g.Nt = Nt;
    k.family->test(layout, h->stream, g, k);
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
    KernelParams k;
    GPK_TRY(fill_common(h, g, k, layout, kernel, kp, Xd, Nd, Xb, Nb));
    g.out = out; g.ld = ld; g.tx = Xt; g.Nt = Nt;
    const bool wide = pairs_eligible(h, out, ld, Nt);
    k.family->cross(layout, wide, h->stream, g, k);                  // (not timed: gpk_prof_read_assembly keeps reporting the Gram launch)
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
    KernelParams k;
    GPK_TRY(kernel_params(h, "assemble_prior: kernel id", kernel, kp, k));
    g.p1 = k.p[0]; g.p2 = k.p[1];
    g.xa = Xa; g.na = na; g.xb = Xb; g.nb = nb; g.out = out; g.ld = ld;
    const bool wide = pairs_eligible(h, out, ld, nb);
    k.family->prior(wide, h->stream, g, k);
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
    KernelParams k;
    GPK_TRY(fill_common(h, g, k, layout, kernel, kp, Xd, Nd, Xb, Nb));
    g.out = out; g.ld = 0; g.tx = Xt; g.Nt = Nt; g.coeff = coeff;
    k.family->extend(layout, h->stream, g, k);
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
    KernelParams k;
    GPK_TRY(fill_common(h, g, k, layout, kernel, kp, Xd, Nd, Xb, Nb));
    g.tx = Xt; g.Nt = Nt; g.coeff = coeff; g.out = out; g.ldo = ldo;
    k.family->extend_fn(layout, fmask, h->stream, g, k);
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
