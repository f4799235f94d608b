// gpk_assemble_jet2.hip -- the fused derivative-kernel evaluator of the 2-JET layout: the whole 2-jet of u at every domain point -- the
// two first derivatives and the three second derivatives as five separate row blocks next to the value -- for equations whose
// second-order coefficients depend on grad u (quasilinear: minimal surface / mean curvature, p-Laplacian, prescribed Gauss curvature;
// DESIGN.md §K "Quasilinear equations: the 2-jet layout").  The Gram matrix, the matrix-free extension with all derivatives up to order
// two, and the pointwise residual of the three equations in their divergence / determinant form.
//
// No reference call site: the reference's layouts carry grad u (Eikonal) or one second-order functional, never both.
//
// Layout.  Blocks 0, 1 = d_1, d_2, blocks 2, 3, 4 = D = d_11 - d_22, M = 2 d_12, L = d_11 + d_22 on the Nd domain points, block 5 = delta on
// the domain points followed by the Nb boundary points: N = 6 Nd + Nb.  Blocks 2..5 are the blocks 0..3 of gpk_assemble_hess, spelled as
// there.  With d = x - y, a_n = h_n(p1, d1), b_n = h_n(p2, d2) (d_y^n exp(-p d^2 / 2) = h_n exp(-p d^2 / 2)) a row functional of order m
// carries (-1)^m.  A pair of domain points has 36 entries, which are 21 values (times kappa) and their negatives:
//   the ten of the Hessian layout  <D,D> .. <delta,delta>                                       (even x even: <F, G'> = <G, F'>)
//   g11 = a2, g12 = a1 b1, g22 = b2:               <d_k, d_l'> = -g_kl                          (odd x odd:   <F, G'> = <G, F'>)
//   o1D = a3 - a1 b2   o1M = 2 a2 b1   o1L = a3 + a1 b2   o1d = a1
//   o2D = a2 b1 - b3   o2M = 2 a1 b2   o2L = a2 b1 + b3   o2d = b1:  <d_k, X'> = -o_kX,  <X, d_k'> = +o_kX   (odd x even)
// from ONE exp and one pair of Hermite evaluations (hermite_compensated: several values consist of h1 / h2 / h3 factors alone); no
// derivative above order 4 per axis occurs.  d -> -d flips a1, a3, b1, b3 exactly and leaves the rest: the o values change sign, all
// others do not, and Theta is symmetric to the bit.
//
// Mapping to the hardware, as assemble_hess_kernel / assemble_grad3_kernel: SoA-packed points in the handle's point scratch (2 arrays of
// Nd+Nb), a workgroup owns TP row points x 256 column points (two-point variant: x 512), lane <-> column point (its coordinates stay in
// registers), the row point is wave-uniform (scalar loads).  No LDS in the Gram kernels, no inline assembly.  The kernel is bound by its
// stores: 36 (two-point: 36 of 16 bytes) per pair of points in the domain-domain part, against ~130 flops.  The two-point variant
// evaluates its two column points one after the other and keeps the 21 values of the first, not its 36 entries: a negation is part of
// the store's operand.
#include "gpk_assemble_common.h"

using namespace gpk_asm;

// One-point and two-point evaluator must give the same bits for the same point pair: explicit fma, no contraction by the compiler (as
// gpk_assemble_hess.hip).  The extension kernels and the residual are written the same way.
#pragma clang fp contract(off)

namespace {

constexpr int NB = 6;                     // row / column blocks

struct Jet2Args {
    const double* px; const double* py;                     // SoA points: domain first, then boundary
    int Nd, M;                                              // M = Nd + Nb
    double p1, p2;
    double* out; long ld;
    double nug[NB];
};

__global__ void pack_jet2_kernel(const double* __restrict__ Xd, int Nd, const double* __restrict__ Xb, int Nb, double* __restrict__ s) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t M = (size_t)Nd + (size_t)Nb;
    if (i < Nd) { s[i] = Xd[2 * i]; s[M + i] = Xd[2 * i + 1]; }
    else if (i < Nd + Nb) { const int b = i - Nd; s[i] = Xb[2 * b]; s[M + i] = Xb[2 * b + 1]; }
}

// the 21 values of one point pair, d = x - y
struct PairJet {
    double he[10];                        // DD, DM, DL, Dd, MM, ML, Md, LL, Ld, dd: the upper triangle of the even 4 x 4 part, row by row
    double gg[3];                         // g11, g12, g22
    double od[2][4];                      // o_kX, X = D, M, L, delta
    // deriv: one of the two points is a domain point (the values against delta are needed); both: both are (all 21)
    __device__ __forceinline__ void eval(double p1, double p2, double d1, double d2, bool deriv, bool both) {
        double a[5], b[5];
        const double e = kappa2_fma(p1, p2, d1, d2);
        he[9] = e;
        if (!deriv) return;
        hermite_compensated(p1, d1, a);
        hermite_compensated(p2, d2, b);
        const double t11 = a[1] * b[1];
        he[3] = (a[2] - b[2]) * e;
        he[6] = 2.0 * t11 * e;
        he[8] = (a[2] + b[2]) * e;
        od[0][3] = a[1] * e;
        od[1][3] = b[1] * e;
        if (!both) return;
        const double t22 = a[2] * b[2], s4 = a[4] + b[4], t31 = a[3] * b[1], t13 = a[1] * b[3];
        he[0] = __builtin_fma(-2.0, t22, s4) * e;
        he[1] = 2.0 * (t31 - t13) * e;
        he[2] = (a[4] - b[4]) * e;
        he[4] = 4.0 * t22 * e;
        he[5] = 2.0 * (t31 + t13) * e;
        he[7] = __builtin_fma(2.0, t22, s4) * e;
        const double t12 = a[1] * b[2], t21 = a[2] * b[1];
        gg[0] = a[2] * e;
        gg[1] = t11 * e;
        gg[2] = b[2] * e;
        od[0][0] = (a[3] - t12) * e;
        od[0][1] = 2.0 * t21 * e;
        od[0][2] = (a[3] + t12) * e;
        od[1][0] = (t21 - b[3]) * e;
        od[1][1] = 2.0 * t12 * e;
        od[1][2] = (t21 + b[3]) * e;
    }
    // <row block i at x, column block j at y>; i, j are constants after unrolling
    __device__ __forceinline__ double entry(int i, int j) const {
        if (i < 2 && j < 2) return -gg[i + j];
        if (i < 2) return -od[i][j - 2];
        if (j < 2) return od[j][i - 2];
        const int r = (i < j ? i : j) - 2, c = (i < j ? j : i) - 2;
        return he[r * 4 - (r * (r - 1)) / 2 + (c - r)];
    }
};

// one column point per lane, 8-byte stores: any alignment, any Nd / Nb
__global__ __launch_bounds__(256) void assemble_jet2_kernel(Jet2Args g) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    const bool live = q < g.M;
    const bool dom = q < g.Nd;
    const double y1 = live ? g.px[q] : 0.0, y2 = live ? g.py[q] : 0.0;
    const int p0 = blockIdx.y * TP;
    const int pend = min(p0 + TP, g.M);
    const long Nd = g.Nd;
    double* const col = g.out + q;                          // column q of block j at col + j * Nd (j < 5: q < Nd only)
    for (int p = p0; p < pend; ++p) {
        const double x1 = g.px[p], x2 = g.py[p];            // uniform address -> scalar loads
        if (!live) continue;
        const bool top = p < g.Nd;                          // wave-uniform: row p of the blocks 0..4 exists
        PairJet u;
        u.eval(g.p1, g.p2, x1 - y1, x2 - y2, dom || top, dom && top);
        const bool diag = p == q;
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            if (i < 5 && !top) continue;
            const long row = (i * Nd + p) * g.ld;
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                if (j < 5 && !dom) continue;
                col[row + j * Nd] = u.entry(i, j) + (i == j && diag ? g.nug[i] : 0.0);
            }
        }
    }
}

// Two column points per lane, one 16-byte store per (row block, column block, row point).  Needs Nd, Nb and the leading dimension
// even and a 16-byte aligned base (checked by the launcher; otherwise the one-point-per-lane kernel above runs).  The two points are
// evaluated one after the other: only the 21 values of the first stay live while the second is computed.
// NT: the policy of store2 (0 plain, 1 non-temporal).
template <int NT>
__global__ __launch_bounds__(256) void assemble_jet2_2_kernel(Jet2Args g) {
    const int q = 2 * (blockIdx.x * 256 + threadIdx.x);
    const bool live = q < g.M;                              // (M even: q + 1 < M as well)
    const bool dom = q < g.Nd;                              // (Nd even: q and q + 1 are both domain points or both boundary points)
    const double y1a = live ? g.px[q] : 0.0, y2a = live ? g.py[q] : 0.0;
    const double y1b = live ? g.px[q + 1] : 0.0, y2b = live ? g.py[q + 1] : 0.0;
    const int p0 = blockIdx.y * TP;
    const int pend = min(p0 + TP, g.M);
    const long Nd = g.Nd;
    double* const col = g.out + q;
    for (int p = p0; p < pend; ++p) {
        const double x1 = g.px[p], x2 = g.py[p];            // uniform address -> scalar loads
        if (!live) continue;
        const bool top = p < g.Nd;                          // wave-uniform
        PairJet u, v;
        u.eval(g.p1, g.p2, x1 - y1a, x2 - y2a, dom || top, dom && top);
        v.eval(g.p1, g.p2, x1 - y1b, x2 - y2b, dom || top, dom && top);
        const bool du = p == q, dv = p == q + 1;
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            if (i < 5 && !top) continue;
            const long row = (i * Nd + p) * g.ld;
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                if (j < 5 && !dom) continue;
                store2<NT>(col + row + j * Nd, u.entry(i, j) + (i == j && du ? g.nug[i] : 0.0), v.entry(i, j) + (i == j && dv ? g.nug[i] : 0.0));
            }
        }
    }
}

// ---- the extension with all derivatives up to order two -------------------------------------------------------------------------------
// out[f][t] = sum_q <d^MI_f at x_t, (c1 d_1 + c2 d_2 + cD D + cM M + cL L + cd delta)_q> kappa, MI = {(0,0),(1,0),(0,1),(2,0),(1,1),(0,2)}, f
// over the set bits of MASK (the GPK_OPFN_* bits).  Mapping and contract as extend_fn_hess_kernel.  The six blocks of a column point act
// through ONE second-order functional with the weights w0 = cd (delta), w1 = c1, w2 = c2 (d_1, d_2), w11 = cL + cD (d_11), w12 = 2 cM
// (d_12), w22 = cL - cD (d_22), formed once per column point:
//   C[m1][m2] = w0 a[m1] b[m2] + w1 a[m1+1] b[m2] + w2 a[m1] b[m2+1] + w11 a[m1+2] b[m2] + w12 a[m1+1] b[m2+1] + w22 a[m1] b[m2+2],
// row f = (-1)^{|MI_f|} C[MI_f] kappa, the same operations whichever other rows are requested.
struct FnJet2Args {
    const double* px; const double* py;
    int Nd, M;
    double p1, p2;
    const double* tx; int Nt;             // (Nt,2) row-major test points
    const double* coeff;                  // (6 Nd + Nb): d_1, d_2, D, M, L blocks, then the delta block
    double* out; long ldo;
};

__host__ __device__ constexpr int jmi_a1(int f) { return f == 1 || f == 4 ? 1 : (f == 3 ? 2 : 0); }
__host__ __device__ constexpr int jmi_a2(int f) { return f == 2 || f == 4 ? 1 : (f == 5 ? 2 : 0); }

template <int MASK>
__global__ __launch_bounds__(256) void extend_fn_jet2_kernel(FnJet2Args g) {
    constexpr int NF = fn_popc(MASK);
    const int t0 = blockIdx.x * FN_TT;
    double x1[FN_TT], x2[FN_TT], s[FN_TT][NF];
    GPK_FN_LOAD_POINTS2(x1, x2, g.tx, t0, g.Nt);
    fn_zero(s);
    const long Nd = g.Nd;
    for (int q = threadIdx.x; q < g.M; q += 256) {
        const double y1 = g.px[q], y2 = g.py[q];
        const bool dom = q < g.Nd;
        const double w1 = dom ? g.coeff[q] : 0.0, w2 = dom ? g.coeff[Nd + q] : 0.0;
        const double cD = dom ? g.coeff[2 * Nd + q] : 0.0, cM = dom ? g.coeff[3 * Nd + q] : 0.0, cL = dom ? g.coeff[4 * Nd + q] : 0.0;
        const double w0 = g.coeff[5 * Nd + q], w11 = cL + cD, w12 = 2.0 * cM, w22 = cL - cD;
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
                    const int m1 = jmi_a1(f), m2 = jmi_a2(f);
                    const double A0 = __builtin_fma(w11, a[m1 + 2], __builtin_fma(w1, a[m1 + 1], w0 * a[m1]));
                    const double A1 = __builtin_fma(w12, a[m1 + 1], w2 * a[m1]);
                    const double A2 = w22 * a[m1];
                    const double c = __builtin_fma(b[m2 + 2], A2, __builtin_fma(b[m2 + 1], A1, b[m2] * A0));
                    s[i][fn_row(MASK, f)] = __builtin_fma(((m1 + m2) & 1) ? -c : c, e, s[i][fn_row(MASK, f)]);
                }
        }
    }
    GPK_FN_REDUCE_STORE(s, NF, t0, g.Nt, g.out, g.ldo);
}

// one instantiation per mask (63)
void launch_extend_fn_jet2(int mask, int grid, hipStream_t st, const FnJet2Args& g) {
    with_mask<63>(mask, [&](auto m) { extend_fn_jet2_kernel<decltype(m)::value><<<grid, 256, 0, st>>>(g); });
}

// precisions and packed points (the handle's point scratch: 2 arrays of Nd + Nb, re-packed by every call)
int fill_common_jet2(gpk_handle h, const char* who, const char* who_kernel, int kernel, const double* kp, const double* Xd, int Nd,
                     const double* Xb, int Nb, double (&p)[2], const double** px, const double** py) {
    if (Nd <= 0 || Nb < 0 || !kp || !Xd || (Nb > 0 && !Xb)) return gpk_bad_arg(h, who);
    GPK_TRY(precisions(h, who_kernel, kernel, kp, 2, p));
    const size_t Mall = (size_t)Nd + (size_t)Nb;
    GPK_TRY(gpk_i_ensure_points(h, 2 * Mall));
    double* s = h->d_pts;
    *px = s; *py = s + Mall;
    pack_jet2_kernel<<<gpk_ceil_div((int)Mall, 256), 256, 0, h->stream>>>(Xd, Nd, Xb, Nb, s);
    GPK_LAUNCH_CHECK(h);
    return 0;
}

// out[t] = the residual of the equation in its divergence / determinant form (ql_residual of gpk_common.h) from the rows u, u_1, u_2,
// u_11, u_12, u_22 of the extension; one fixed order of operations (no contraction in this file)
struct QlPrm { double c[3]; };
__global__ __launch_bounds__(256) void pde_residual_ql_kernel(int kind, QlPrm prm, int Nt, const double* __restrict__ u, long ldu,
                                                              const double* __restrict__ rhs, double* __restrict__ out) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= Nt) return;
    out[t] = ql_residual(kind, prm.c, rhs[t], u[t], u[ldu + t], u[2 * ldu + t], u[3 * ldu + t], u[4 * ldu + t], u[5 * ldu + t]);
}

}  // namespace


extern "C" int gpk_assemble_jet2(gpk_handle h, int kernel, const double* kp, const double* Xd, int Nd, const double* Xb, int Nb,
                                 double nugget, int nugget_type, double* Theta, int ld, double* host_ratios5) {
    if (!h || !Theta) return GPK_ERR_ARG;
    if (!nugget_type_valid(nugget_type)) return gpk_bad_arg(h, "assemble_jet2: nugget_type");
    if ((long)6 * Nd + Nb > 0x7fffffffL) return gpk_bad_arg(h, "assemble_jet2: N exceeds int");
    if (Nd > 0 && Nb >= 0 && ld < 6 * Nd + Nb) return gpk_bad_arg(h, "assemble_jet2: ld < N");
    Jet2Args g;
    double p[2];
    GPK_TRY(fill_common_jet2(h, "assemble_jet2: sizes/pointers", "assemble_jet2: kernel id", kernel, kp, Xd, Nd, Xb, Nb, p, &g.px, &g.py));
    g.p1 = p[0]; g.p2 = p[1];
    g.Nd = Nd; g.M = Nd + Nb;
    // values at d = 0 (h0 = 1, h2 = -p, h4 = 3 p^2, odd orders vanish), in long double: the ratios are the analytic values to an ulp
    const long double q1 = p[0], q2 = p[1];
    const long double s = 3.0L * (q1 * q1 + q2 * q2), x = 2.0L * q1 * q2;
    const long double diag[5] = {q1, q2, s - x, 2.0L * x, s + x};   // <d_1,d_1>, <d_2,d_2>, <D,D>, <M,M>, <L,L>;  <delta,delta> = 1
    for (int k = 0; k < 5; ++k) {
        const double r = (double)(((long double)Nd * diag[k]) / ((long double)Nd + (long double)Nb));
        if (host_ratios5) host_ratios5[k] = r;
        g.nug[k] = block_nugget(nugget_type, nugget, r);
    }
    g.nug[5] = block_nugget(nugget_type, nugget, 1.0);
    g.out = Theta; g.ld = ld;
    return launch_two_block(h, pairs_eligible(h, Theta, ld, Nd, Nb), g, assemble_jet2_kernel, assemble_jet2_2_kernel<0>, assemble_jet2_2_kernel<1>);
}

extern "C" int gpk_extend_functionals_jet2(gpk_handle h, int kernel, const double* kp, const double* Xt, int Nt,
                                           const double* Xd, int Nd, const double* Xb, int Nb,
                                           const double* coeff, int fmask, double* out, int ldo) {
    if (!h) return GPK_ERR_ARG;
    if (!out || !Xt || !coeff) return gpk_bad_arg(h, "extend_functionals_jet2: pointers");
    if (fmask <= 0 || fmask > 63) return gpk_bad_arg(h, "extend_functionals_jet2: fmask must be a non-empty subset of the GPK_OPFN_* bits");
    if (Nt <= 0) return gpk_bad_arg(h, "extend_functionals_jet2: Nt <= 0");
    if (ldo < Nt) return gpk_bad_arg(h, "extend_functionals_jet2: ldo < Nt");
    FnJet2Args g;
    double p[2];
    GPK_TRY(fill_common_jet2(h, "extend_functionals_jet2: sizes/pointers", "extend_functionals_jet2: kernel id", kernel, kp, Xd, Nd, Xb, Nb,
                             p, &g.px, &g.py));
    g.p1 = p[0]; g.p2 = p[1];
    g.Nd = Nd; g.M = Nd + Nb;
    g.tx = Xt; g.Nt = Nt; g.coeff = coeff; g.out = out; g.ldo = ldo;
    launch_extend_fn_jet2(fmask, gpk_ceil_div(Nt, FN_TT), h->stream, g);
    GPK_LAUNCH_CHECK(h);
    return 0;
}

extern "C" int gpk_pde_residual_ql(gpk_handle h, int kind, const double* host_params3, int Nt, const double* fields, int ldf,
                                   const double* rhs, double* out) {
    if (!h) return GPK_ERR_ARG;
    if (Nt <= 0) return gpk_bad_arg(h, "pde_residual_ql: Nt <= 0");
    if (!host_params3 || !fields || !rhs || !out || ldf < Nt) return gpk_bad_arg(h, "pde_residual_ql: host_params3 / fields / rhs / out / ldf");
    if (const char* bad = gpk_ql_invalid(kind, host_params3[0], host_params3[1], host_params3[2])) return gpk_bad_arg(h, bad);
    QlPrm prm;
    for (int k = 0; k < 3; ++k) prm.c[k] = host_params3[k];
    pde_residual_ql_kernel<<<gpk_ceil_div(Nt, 256), 256, 0, h->stream>>>(kind, prm, Nt, fields, ldf, rhs, out);
    GPK_LAUNCH_CHECK(h);
    return 0;
}
