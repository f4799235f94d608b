// gpk_assemble_hess.hip -- the fused derivative-kernel evaluator of the Hessian layout: the second derivatives of u at every domain point
// as three separate row blocks, for equations that are nonlinear in D^2 u (Monge-Ampere, DESIGN.md §K "Fully nonlinear: Monge-Ampere").
// The Gram matrix, the matrix-free extension with all derivatives up to order two, and the pointwise residual det D^2 u - f.
//
// No reference call site: the reference's Gram_matrix_assembly (src/Gram_matrice.py) carries the second derivatives through the
// Laplacian (or d_22) alone.
//
// Math.  D = d_11 - d_22, M = 2 d_12, L = d_11 + d_22 (the Laplacian): (L u)^2 = (D u)^2 + (M u)^2 + 4 det D^2 u.  Domain point i carries
// D, M, L and delta (blocks 0, 1, 2, 3), boundary point b carries delta (block 3); N = 4 N_d + N_b.  With d = x - y and a_n = h_n(p1, d1),
// b_n = h_n(p2, d2) the 1-D Hermite factors (d_y^n exp(-p d^2 / 2) = h_n exp(-p d^2 / 2)), every functional here is of even order, so no
// sign enters, <F, G'> = <G, F'>, and the 16 entries of a point pair are the 10 values (times kappa)
//   <D,D> = a4 - 2 a2 b2 + b4      <D,M> = 2 (a3 b1 - a1 b3)      <D,L> = a4 - b4      <D,delta> = a2 - b2
//   <M,M> = 4 a2 b2                <M,L> = 2 (a3 b1 + a1 b3)      <M,delta> = 2 a1 b1
//   <L,L> = a4 + 2 a2 b2 + b4      <L,delta> = a2 + b2            <delta,delta> = 1
// from ONE exp and one pair of Hermite evaluations; no derivative above order 4 per axis occurs.  <D,delta>, <M,M>, <M,delta>, <D,M> and
// <M,L> consist of h1 / h2 / h3 factors alone, hence hermite_compensated (gpk_assemble_common.h).  d -> -d flips a1, a3, b1, b3 exactly
// and every value above is even in it: Theta is symmetric to the bit.
//
// Mapping to the hardware, as assemble_op_kernel / assemble_op2_kernel: SoA-packed points in the handle's point scratch (2 arrays of
// Nd+Nb), a workgroup owns TP row points x 256 column points (two-point variant: x 512), lane <-> column point (its coordinates stay in
// registers), the row point is wave-uniform (scalar loads).  The kernel is bound by its stores: 16 (two-point: 16 of 16 bytes) per
// pair of points in the domain-domain part, against ~90 flops.
#include "gpk_assemble_common.h"

using namespace gpk_asm;

// One-point and two-point evaluator must give the same bits for the same point pair: explicit fma, no contraction by the compiler (as
// gpk_assemble_bc.hip / gpk_assemble_op.hip).  The extension kernels and the residual are written the same way.
#pragma clang fp contract(off)

namespace {

struct HessArgs {
    const double* px; const double* py;                     // SoA points: domain first, then boundary
    int Nd, M;                                              // M = Nd + Nb
    double p1, p2;
    double* out; long ld;
    double nug[4];
};

__global__ void pack_hess_kernel(const double* __restrict__ Xd, int Nd, const double* __restrict__ Xb, int Nb, double* __restrict__ s) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t M = (size_t)Nd + (size_t)Nb;
    if (i < Nd) { s[i] = Xd[2 * i]; s[M + i] = Xd[2 * i + 1]; }
    else if (i < Nd + Nb) { const int b = i - Nd; s[i] = Xb[2 * b]; s[M + i] = Xb[2 * b + 1]; }
}

// the ten values of one point pair, d = x - y
struct PairHess {
    double DD, DM, DL, Dd, MM, ML, Md, LL, Ld, dd;
    // deriv: one of the two points is a domain point (the <., delta> values are needed); both: both are (all ten)
    __device__ __forceinline__ void eval(double p1, double p2, double d1, double d2, bool deriv, bool both) {
        double a[5], b[5];
        const double e = kappa2_fma(p1, p2, d1, d2);
        dd = e;
        if (!deriv) return;
        hermite_compensated(p1, d1, a);
        hermite_compensated(p2, d2, b);
        Dd = (a[2] - b[2]) * e;
        Md = 2.0 * (a[1] * b[1]) * e;
        Ld = (a[2] + b[2]) * e;
        if (!both) return;
        const double t22 = a[2] * b[2], s4 = a[4] + b[4], t31 = a[3] * b[1], t13 = a[1] * b[3];
        DD = __builtin_fma(-2.0, t22, s4) * e;
        DM = 2.0 * (t31 - t13) * e;
        DL = (a[4] - b[4]) * e;
        MM = 4.0 * t22 * e;
        ML = 2.0 * (t31 + t13) * e;
        LL = __builtin_fma(2.0, t22, s4) * e;
    }
};

// one column point per lane, 8-byte stores: any alignment, any Nd / Nb
__global__ __launch_bounds__(256) void assemble_hess_kernel(HessArgs g) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    const bool live = q < g.M;
    const bool dom = q < g.Nd;
    const double y1 = live ? g.px[q] : 0.0, y2 = live ? g.py[q] : 0.0;
    const int p0 = blockIdx.y * TP;
    const int pend = min(p0 + TP, g.M);
    const long Nd = g.Nd;
    double* const cD = g.out + q;                           // column q of the blocks D, M, L (q < Nd only) and delta
    double* const cM = g.out + Nd + q;
    double* const cL = g.out + 2 * Nd + q;
    double* const cd = g.out + 3 * Nd + q;
    for (int p = p0; p < pend; ++p) {
        const double x1 = g.px[p], x2 = g.py[p];            // uniform address -> scalar loads
        if (!live) continue;
        PairHess u;
        u.eval(g.p1, g.p2, x1 - y1, x2 - y2, dom || p < g.Nd, dom && p < g.Nd);
        const bool diag = p == q;
        if (p < g.Nd) {                                     // wave-uniform: rows p of the blocks D, M, L
            const long rD = (long)p * g.ld, rM = (Nd + p) * g.ld, rL = (2 * Nd + p) * g.ld;
            if (dom) {
                cD[rD] = u.DD + (diag ? g.nug[0] : 0.0); cM[rD] = u.DM; cL[rD] = u.DL;
                cD[rM] = u.DM; cM[rM] = u.MM + (diag ? g.nug[1] : 0.0); cL[rM] = u.ML;
                cD[rL] = u.DL; cM[rL] = u.ML; cL[rL] = u.LL + (diag ? g.nug[2] : 0.0);
            }
            cd[rD] = u.Dd; cd[rM] = u.Md; cd[rL] = u.Ld;
        }
        const long rd = (3 * Nd + p) * g.ld;                // row p of the delta block (p < M always)
        if (dom) { cD[rd] = u.Dd; cM[rd] = u.Md; cL[rd] = u.Ld; }
        cd[rd] = u.dd + (diag ? g.nug[3] : 0.0);
    }
}

// Two column points per lane, one 16-byte store per (row block, column block, row point).  Needs Nd, Nb and the leading dimension
// even and a 16-byte aligned base (checked by the launcher; otherwise the one-point-per-lane kernel above runs).
// NT: the policy of store2 (0 plain, 1 non-temporal).
template <int NT>
__global__ __launch_bounds__(256) void assemble_hess2_kernel(HessArgs g) {
    const int q = 2 * (blockIdx.x * 256 + threadIdx.x);
    const bool live = q < g.M;                              // (M even: q + 1 < M as well)
    const bool dom = q < g.Nd;                              // (Nd even: q and q + 1 are both domain points or both boundary points)
    const double y1a = live ? g.px[q] : 0.0, y2a = live ? g.py[q] : 0.0;
    const double y1b = live ? g.px[q + 1] : 0.0, y2b = live ? g.py[q + 1] : 0.0;
    const int p0 = blockIdx.y * TP;
    const int pend = min(p0 + TP, g.M);
    const long Nd = g.Nd;
    double* const cD = g.out + q;
    double* const cM = g.out + Nd + q;
    double* const cL = g.out + 2 * Nd + q;
    double* const cd = g.out + 3 * Nd + q;
    for (int p = p0; p < pend; ++p) {
        const double x1 = g.px[p], x2 = g.py[p];            // uniform address -> scalar loads
        if (!live) continue;
        PairHess u, v;
        u.eval(g.p1, g.p2, x1 - y1a, x2 - y2a, dom || p < g.Nd, dom && p < g.Nd);
        v.eval(g.p1, g.p2, x1 - y1b, x2 - y2b, dom || p < g.Nd, dom && p < g.Nd);
        const bool du = p == q, dv = p == q + 1;
        if (p < g.Nd) {                                     // wave-uniform
            const long rD = (long)p * g.ld, rM = (Nd + p) * g.ld, rL = (2 * Nd + p) * g.ld;
            if (dom) {
                store2<NT>(cD + rD, u.DD + (du ? g.nug[0] : 0.0), v.DD + (dv ? g.nug[0] : 0.0));
                store2<NT>(cM + rD, u.DM, v.DM);
                store2<NT>(cL + rD, u.DL, v.DL);
                store2<NT>(cD + rM, u.DM, v.DM);
                store2<NT>(cM + rM, u.MM + (du ? g.nug[1] : 0.0), v.MM + (dv ? g.nug[1] : 0.0));
                store2<NT>(cL + rM, u.ML, v.ML);
                store2<NT>(cD + rL, u.DL, v.DL);
                store2<NT>(cM + rL, u.ML, v.ML);
                store2<NT>(cL + rL, u.LL + (du ? g.nug[2] : 0.0), v.LL + (dv ? g.nug[2] : 0.0));
            }
            store2<NT>(cd + rD, u.Dd, v.Dd);
            store2<NT>(cd + rM, u.Md, v.Md);
            store2<NT>(cd + rL, u.Ld, v.Ld);
        }
        const long rd = (3 * Nd + p) * g.ld;
        if (dom) {
            store2<NT>(cD + rd, u.Dd, v.Dd);
            store2<NT>(cM + rd, u.Md, v.Md);
            store2<NT>(cL + rd, u.Ld, v.Ld);
        }
        store2<NT>(cd + rd, u.dd + (du ? g.nug[3] : 0.0), v.dd + (dv ? g.nug[3] : 0.0));
    }
}

// ---- the extension with all derivatives up to order two -------------------------------------------------------------------------------
// out[f][t] = sum_q <d^MI_f at x_t, (cD D + cM M + cL L + cd delta)_q> kappa, MI = {(0,0),(1,0),(0,1),(2,0),(1,1),(0,2)}, f over the set
// bits of MASK (the GPK_OPFN_* bits).  Mapping and contract as extend_fn_op_kernel.  The four blocks of a column point act through ONE
// second-order functional with the weights w0 = cd (delta), w11 = cL + cD (d_11), w12 = 2 cM (d_12), w22 = cL - cD (d_22), formed once per
// column point:  C[m1][m2] = w0 a[m1] b[m2] + w11 a[m1+2] b[m2] + w12 a[m1+1] b[m2+1] + w22 a[m1] b[m2+2],  row f = (-1)^{|MI_f|} C[MI_f] kappa,
// the same operations whichever other rows are requested.
struct FnHessArgs {
    const double* px; const double* py;
    int Nd, M;
    double p1, p2;
    const double* tx; int Nt;             // (Nt,2) row-major test points
    const double* coeff;                  // (4 Nd + Nb): D, M, L blocks, then the delta block
    double* out; long ldo;
};

__host__ __device__ constexpr int hmi_a1(int f) { return f == 1 || f == 4 ? 1 : (f == 3 ? 2 : 0); }
__host__ __device__ constexpr int hmi_a2(int f) { return f == 2 || f == 4 ? 1 : (f == 5 ? 2 : 0); }

template <int MASK>
__global__ __launch_bounds__(256) void extend_fn_hess_kernel(FnHessArgs g) {
    constexpr int NF = fn_popc(MASK);
    const int t0 = blockIdx.x * FN_TT;
    double x1[FN_TT], x2[FN_TT], s[FN_TT][NF];
    GPK_FN_LOAD_POINTS2(x1, x2, g.tx, t0, g.Nt);
    fn_zero(s);
    const long Nd = g.Nd;
    for (int q = threadIdx.x; q < g.M; q += 256) {
        const double y1 = g.px[q], y2 = g.py[q];
        const bool dom = q < g.Nd;
        const double cD = dom ? g.coeff[q] : 0.0, cM = dom ? g.coeff[Nd + q] : 0.0, cL = dom ? g.coeff[2 * Nd + q] : 0.0;
        const double w0 = g.coeff[3 * Nd + q], w11 = cL + cD, w12 = 2.0 * cM, w22 = cL - cD;
#pragma unroll
        for (int i = 0; i < FN_TT; ++i) {
            const double d1 = x1[i] - y1, d2 = x2[i] - y2;
            const double e = kappa2_fma(g.p1, g.p2, d1, d2);
            double a[5], b[5];
            hermite_compensated(g.p1, d1, a);
            hermite_compensated(g.p2, d2, b);
#pragma unroll
            for (int f = 0; f < 6; ++f)
                if ((MASK >> f) & 1) {
                    const int m1 = hmi_a1(f), m2 = hmi_a2(f);
                    const double A0 = __builtin_fma(w11, a[m1 + 2], w0 * a[m1]);
                    const double A1 = w12 * a[m1 + 1];
                    const double A2 = w22 * a[m1];
                    const double c = __builtin_fma(b[m2 + 2], A2, __builtin_fma(b[m2 + 1], A1, b[m2] * A0));
                    s[i][fn_row(MASK, f)] = __builtin_fma(((m1 + m2) & 1) ? -c : c, e, s[i][fn_row(MASK, f)]);
                }
        }
    }
    GPK_FN_REDUCE_STORE(s, NF, t0, g.Nt, g.out, g.ldo);
}

// one instantiation per mask (63)
void launch_extend_fn_hess(int mask, int grid, hipStream_t st, const FnHessArgs& g) {
    with_mask<63>(mask, [&](auto m) { extend_fn_hess_kernel<decltype(m)::value><<<grid, 256, 0, st>>>(g); });
}

// precisions and packed points (the handle's point scratch: 2 arrays of Nd + Nb, re-packed by every call)
int fill_common_hess(gpk_handle h, const char* who, const char* who_kernel, int kernel, const double* kp, const double* Xd, int Nd,
                     const double* Xb, int Nb, double (&p)[2], const double** px, const double** py) {
    if (Nd <= 0 || Nb < 0 || !kp || !Xd || (Nb > 0 && !Xb)) return gpk_bad_arg(h, who);
    GPK_TRY(precisions(h, who_kernel, kernel, kp, 2, p));
    const size_t Mall = (size_t)Nd + (size_t)Nb;
    GPK_TRY(gpk_i_ensure_points(h, 2 * Mall));
    double* s = h->d_pts;
    *px = s; *py = s + Mall;
    pack_hess_kernel<<<gpk_ceil_div((int)Mall, 256), 256, 0, h->stream>>>(Xd, Nd, Xb, Nb, s);
    GPK_LAUNCH_CHECK(h);
    return 0;
}

// out[t] = (d11 d22 - d12^2) - f: two products, two subtractions, in this order (no contraction in this file)
__global__ __launch_bounds__(256) void pde_residual_ma_kernel(int Nt, const double* __restrict__ u, long ldu, const double* __restrict__ rhs,
                                                              double* __restrict__ out) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= Nt) return;
    const double d11 = u[t], d12 = u[ldu + t], d22 = u[2 * ldu + t];
    const double m = d11 * d22, c = d12 * d12;
    out[t] = (m - c) - rhs[t];
}

}  // namespace


extern "C" int gpk_assemble_hess(gpk_handle h, int kernel, const double* kp, const double* Xd, int Nd, const double* Xb, int Nb,
                                 double nugget, int nugget_type, double* Theta, int ld, double* host_ratios3) {
    if (!h || !Theta) return GPK_ERR_ARG;
    if (!nugget_type_valid(nugget_type)) return gpk_bad_arg(h, "assemble_hess: nugget_type");
    if ((long)4 * Nd + Nb > 0x7fffffffL) return gpk_bad_arg(h, "assemble_hess: N exceeds int");
    if (Nd > 0 && Nb >= 0 && ld < 4 * Nd + Nb) return gpk_bad_arg(h, "assemble_hess: ld < N");
    HessArgs g;
    double p[2];
    GPK_TRY(fill_common_hess(h, "assemble_hess: sizes/pointers", "assemble_hess: kernel id", kernel, kp, Xd, Nd, Xb, Nb, p, &g.px, &g.py));
    g.p1 = p[0]; g.p2 = p[1];
    g.Nd = Nd; g.M = Nd + Nb;
    // values at d = 0 (h0 = 1, h2 = -p, h4 = 3 p^2, odd orders vanish), in long double: the ratios are the analytic values to an ulp
    const long double q1 = p[0], q2 = p[1];
    const long double s = 3.0L * (q1 * q1 + q2 * q2), x = 2.0L * q1 * q2;
    const long double diag[3] = {s - x, 2.0L * x, s + x};   // <D,D>, <M,M>, <L,L>;  <delta,delta> = 1
    for (int k = 0; k < 3; ++k) {
        const double r = (double)(((long double)Nd * diag[k]) / ((long double)Nd + (long double)Nb));
        if (host_ratios3) host_ratios3[k] = r;
        g.nug[k] = block_nugget(nugget_type, nugget, r);
    }
    g.nug[3] = block_nugget(nugget_type, nugget, 1.0);
    g.out = Theta; g.ld = ld;
    return launch_two_block(h, pairs_eligible(h, Theta, ld, Nd, Nb), g, assemble_hess_kernel, assemble_hess2_kernel<0>, assemble_hess2_kernel<1>);
}

extern "C" int gpk_extend_functionals_hess(gpk_handle h, int kernel, const double* kp, const double* Xt, int Nt,
                                           const double* Xd, int Nd, const double* Xb, int Nb,
                                           const double* coeff, int fmask, double* out, int ldo) {
    if (!h) return GPK_ERR_ARG;
    if (!out || !Xt || !coeff) return gpk_bad_arg(h, "extend_functionals_hess: pointers");
    if (fmask <= 0 || fmask > 63) return gpk_bad_arg(h, "extend_functionals_hess: fmask must be a non-empty subset of the GPK_OPFN_* bits");
    if (Nt <= 0) return gpk_bad_arg(h, "extend_functionals_hess: Nt <= 0");
    if (ldo < Nt) return gpk_bad_arg(h, "extend_functionals_hess: ldo < Nt");
    FnHessArgs g;
    double p[2];
    GPK_TRY(fill_common_hess(h, "extend_functionals_hess: sizes/pointers", "extend_functionals_hess: kernel id", kernel, kp, Xd, Nd, Xb, Nb,
                             p, &g.px, &g.py));
    g.p1 = p[0]; g.p2 = p[1];
    g.Nd = Nd; g.M = Nd + Nb;
    g.tx = Xt; g.Nt = Nt; g.coeff = coeff; g.out = out; g.ldo = ldo;
    launch_extend_fn_hess(fmask, gpk_ceil_div(Nt, FN_TT), h->stream, g);
    GPK_LAUNCH_CHECK(h);
    return 0;
}

extern "C" int gpk_pde_residual_ma(gpk_handle h, int Nt, const double* fields, int ldf, const double* rhs, double* out) {
    if (!h) return GPK_ERR_ARG;
    if (Nt <= 0) return gpk_bad_arg(h, "pde_residual_ma: Nt <= 0");
    if (!fields || !rhs || !out || ldf < Nt) return gpk_bad_arg(h, "pde_residual_ma: fields / rhs / out / ldf");
    pde_residual_ma_kernel<<<gpk_ceil_div(Nt, 256), 256, 0, h->stream>>>(Nt, fields, ldf, rhs, out);
    GPK_LAUNCH_CHECK(h);
    return 0;
}
