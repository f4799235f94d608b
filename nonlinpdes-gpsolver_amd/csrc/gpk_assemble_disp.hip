// gpk_assemble_disp.hip -- the fused derivative-kernel evaluator of the dispersive layout: the Burgers layout with the second space
// derivative exchanged for the third, for equations of Korteweg-de Vries type u_t + alpha u u_x + delta u_xxx = f (DESIGN.md §K
// "Dispersive equations: the third-order layout").  The Gram matrix and the matrix-free extension with u, u_t, u_x, u_xx, u_xxx.
//
// No reference call site: the reference's Gram_matrix_assembly (src/Gram_matrice.py) stops at second derivatives.
//
// Math.  Points are (t, x): axis 1 is time, axis 2 is space.  Domain point i carries T = d_t, X = d_x, Q = d_x^3 and delta (blocks 0, 1,
// 2, 3), boundary point b carries delta (block 3); N = 4 N_d + N_b.  With d = x - y (row point minus column point) and a_n = h_n(p1, d1),
// b_n = h_n(p2, d2) the 1-D Hermite factors (d_y^n exp(-p d^2 / 2) = h_n exp(-p d^2 / 2), h_n = p^(n/2) He_n(sqrt(p) d)), a row functional
// of order (m1, m2) against a column functional of order (n1, n2) is (-1)^(m1+m2) a_(m1+n1) b_(m2+n2) kappa.  T, X and Q are of odd order,
// delta of even order, so the 16 entries of a point pair are the 10 values (times kappa)
//   <T,T> = -a2      <T,X> = -a1 b1      <T,Q> = -a1 b3      <T,delta> = -a1
//   <X,X> = -b2      <X,Q> = -b4         <X,delta> = -b1
//   <Q,Q> = -b6      <Q,delta> = -b3     <delta,delta> = 1
// and <delta,F> = -<F,delta> for F = T, X, Q, from ONE exp and one pair of Hermite evaluations: order 2 in t, order 6 in x.  d -> -d flips
// a1, b1, b3 (and b5, which no entry uses) exactly and leaves a2, b2, b4, b6 and kappa as they are; every value is formed as 0.0 - v, so a zero
// is +0 on both sides of the diagonal: Theta is symmetric to the bit.
// At d = 0: <T,T> = p1, <X,X> = p2, <Q,Q> = 15 p2^3.
//
// Mapping to the hardware, as assemble_hess_kernel: SoA-packed points in the handle's point scratch (2 arrays of Nd+Nb), a workgroup
// owns TP row points x 256 column points (two-point variant: x 512), lane <-> column point (its coordinates stay in registers), the row
// point is wave-uniform (scalar loads).  Ten values per point pair, as the Hessian layout: the same tile, the same register budget.
// The kernel is bound by its stores.
#include "gpk_assemble_common.h"

using namespace gpk_asm;

// One-point and two-point evaluator must give the same bits for the same point pair: explicit fma, no contraction by the compiler (as
// gpk_assemble_hess.hip).  The extension kernels are written the same way.
#pragma clang fp contract(off)

namespace {

struct DispArgs {
    const double* px; const double* py;                     // SoA points (t, x): domain first, then boundary
    int Nd, M;                                              // M = Nd + Nb
    double p1, p2;
    double* out; long ld;
    double nug[4];
};

__global__ void pack_disp_kernel(const double* __restrict__ Xd, int Nd, const double* __restrict__ Xb, int Nb, double* __restrict__ s) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t M = (size_t)Nd + (size_t)Nb;
    if (i < Nd) { s[i] = Xd[2 * i]; s[M + i] = Xd[2 * i + 1]; }
    else if (i < Nd + Nb) { const int b = i - Nd; s[i] = Xb[2 * b]; s[M + i] = Xb[2 * b + 1]; }
}

// h0..h6 of the space axis: h0..h4 compensated (an entry can consist of h1, h2 or h3 alone), h5 and h6 by Horner in q^2 = (p d)^2.
// h6 has a constant term (-15 p^3) that no root of the lower factors shares, h5 occurs in the extension only, next to other terms.
__device__ __forceinline__ void hermite7(double p, double d, double (&h)[7]) {
    double l[5];
    hermite_compensated(p, d, l);
#pragma unroll
    for (int n = 0; n < 5; ++n) h[n] = l[n];
    const double q = p * d;
    const double q2 = q * q;
    const double pp = p * p;
    h[5] = q * __builtin_fma(q2, q2 - 10.0 * p, 15.0 * pp);
    h[6] = __builtin_fma(q2, __builtin_fma(q2, q2 - 15.0 * p, 45.0 * pp), -15.0 * (pp * p));
}

// the ten values of one point pair, d = x - y (row point minus column point); the values <F, delta> are those of the ROW functional F
struct PairDisp {
    double TT, TX, TQ, Td, XX, XQ, Xd, QQ, Qd, dd;
    // deriv: one of the two points is a domain point (the <., delta> values are needed); both: both are (all ten)
    __device__ __forceinline__ void eval(double p1, double p2, double d1, double d2, bool deriv, bool both) {
        double a[5], b[7];
        const double e = kappa2_fma(p1, p2, d1, d2);
        dd = e;
        if (!deriv) return;
        hermite_compensated(p1, d1, a);
        hermite7(p2, d2, b);
        // 0.0 - v, not -v: a zero comes out as +0 whichever sign its factors gave it.  With d1 = 0 in both directions (two points at the same
        // time) a1 = +0 both ways while b1, b3 flip, and -(a1 b3) would be -0 on one side of the diagonal and +0 on the other.
        Td = 0.0 - a[1] * e;
        Xd = 0.0 - b[1] * e;
        Qd = 0.0 - b[3] * e;
        if (!both) return;
        TT = 0.0 - a[2] * e;
        TX = 0.0 - (a[1] * b[1]) * e;
        TQ = 0.0 - (a[1] * b[3]) * e;
        XX = 0.0 - b[2] * e;
        XQ = 0.0 - b[4] * e;
        QQ = 0.0 - b[6] * e;
    }
};

// one column point per lane, 8-byte stores: any alignment, any Nd / Nb
__global__ __launch_bounds__(256) void assemble_disp_kernel(DispArgs g) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    const bool live = q < g.M;
    const bool dom = q < g.Nd;
    const double y1 = live ? g.px[q] : 0.0, y2 = live ? g.py[q] : 0.0;
    const int p0 = blockIdx.y * TP;
    const int pend = min(p0 + TP, g.M);
    const long Nd = g.Nd;
    double* const cT = g.out + q;                           // column q of the blocks T, X, Q (q < Nd only) and delta
    double* const cX = g.out + Nd + q;
    double* const cQ = g.out + 2 * Nd + q;
    double* const cd = g.out + 3 * Nd + q;
    for (int p = p0; p < pend; ++p) {
        const double x1 = g.px[p], x2 = g.py[p];            // uniform address -> scalar loads
        if (!live) continue;
        PairDisp u;
        u.eval(g.p1, g.p2, x1 - y1, x2 - y2, dom || p < g.Nd, dom && p < g.Nd);
        const bool diag = p == q;
        if (p < g.Nd) {                                     // wave-uniform: rows p of the blocks T, X, Q
            const long rT = (long)p * g.ld, rX = (Nd + p) * g.ld, rQ = (2 * Nd + p) * g.ld;
            if (dom) {
                cT[rT] = u.TT + (diag ? g.nug[0] : 0.0); cX[rT] = u.TX; cQ[rT] = u.TQ;
                cT[rX] = u.TX; cX[rX] = u.XX + (diag ? g.nug[1] : 0.0); cQ[rX] = u.XQ;
                cT[rQ] = u.TQ; cX[rQ] = u.XQ; cQ[rQ] = u.QQ + (diag ? g.nug[2] : 0.0);
            }
            cd[rT] = u.Td; cd[rX] = u.Xd; cd[rQ] = u.Qd;
        }
        const long rd = (3 * Nd + p) * g.ld;                // row p of the delta block (p < M always)
        if (dom) { cT[rd] = 0.0 - u.Td; cX[rd] = 0.0 - u.Xd; cQ[rd] = 0.0 - u.Qd; }   // the odd functional on the column side: the other sign (+0 stays +0)
        cd[rd] = u.dd + (diag ? g.nug[3] : 0.0);
    }
}

// Two column points per lane, one 16-byte store per (row block, column block, row point).  Needs Nd, Nb and the leading dimension
// even and a 16-byte aligned base (checked by the launcher; otherwise the one-point-per-lane kernel above runs).
// NT: the policy of store2 (0 plain, 1 non-temporal).
template <int NT>
__global__ __launch_bounds__(256) void assemble_disp2_kernel(DispArgs g) {
    const int q = 2 * (blockIdx.x * 256 + threadIdx.x);
    const bool live = q < g.M;                              // (M even: q + 1 < M as well)
    const bool dom = q < g.Nd;                              // (Nd even: q and q + 1 are both domain points or both boundary points)
    const double y1a = live ? g.px[q] : 0.0, y2a = live ? g.py[q] : 0.0;
    const double y1b = live ? g.px[q + 1] : 0.0, y2b = live ? g.py[q + 1] : 0.0;
    const int p0 = blockIdx.y * TP;
    const int pend = min(p0 + TP, g.M);
    const long Nd = g.Nd;
    double* const cT = g.out + q;
    double* const cX = g.out + Nd + q;
    double* const cQ = g.out + 2 * Nd + q;
    double* const cd = g.out + 3 * Nd + q;
    for (int p = p0; p < pend; ++p) {
        const double x1 = g.px[p], x2 = g.py[p];            // uniform address -> scalar loads
        if (!live) continue;
        PairDisp u, v;
        u.eval(g.p1, g.p2, x1 - y1a, x2 - y2a, dom || p < g.Nd, dom && p < g.Nd);
        v.eval(g.p1, g.p2, x1 - y1b, x2 - y2b, dom || p < g.Nd, dom && p < g.Nd);
        const bool du = p == q, dv = p == q + 1;
        if (p < g.Nd) {                                     // wave-uniform
            const long rT = (long)p * g.ld, rX = (Nd + p) * g.ld, rQ = (2 * Nd + p) * g.ld;
            if (dom) {
                store2<NT>(cT + rT, u.TT + (du ? g.nug[0] : 0.0), v.TT + (dv ? g.nug[0] : 0.0));
                store2<NT>(cX + rT, u.TX, v.TX);
                store2<NT>(cQ + rT, u.TQ, v.TQ);
                store2<NT>(cT + rX, u.TX, v.TX);
                store2<NT>(cX + rX, u.XX + (du ? g.nug[1] : 0.0), v.XX + (dv ? g.nug[1] : 0.0));
                store2<NT>(cQ + rX, u.XQ, v.XQ);
                store2<NT>(cT + rQ, u.TQ, v.TQ);
                store2<NT>(cX + rQ, u.XQ, v.XQ);
                store2<NT>(cQ + rQ, u.QQ + (du ? g.nug[2] : 0.0), v.QQ + (dv ? g.nug[2] : 0.0));
            }
            store2<NT>(cd + rT, u.Td, v.Td);
            store2<NT>(cd + rX, u.Xd, v.Xd);
            store2<NT>(cd + rQ, u.Qd, v.Qd);
        }
        const long rd = (3 * Nd + p) * g.ld;
        if (dom) {
            store2<NT>(cT + rd, 0.0 - u.Td, 0.0 - v.Td);
            store2<NT>(cX + rd, 0.0 - u.Xd, 0.0 - v.Xd);
            store2<NT>(cQ + rd, 0.0 - u.Qd, 0.0 - v.Qd);
        }
        store2<NT>(cd + rd, u.dd + (du ? g.nug[3] : 0.0), v.dd + (dv ? g.nug[3] : 0.0));
    }
}

// ---- the extension with u, u_t, u_x, u_xx, u_xxx ----------------------------------------------------------------------------------------
// out[f][t] = sum_q <d^MI_f at x_t, (cT d_t + cX d_x + cQ d_x^3 + cd delta)_q> kappa, MI = {(0,0),(1,0),(0,1),(0,2),(0,3)}, f over the set
// bits of MASK (the compact mask of the launcher: bit 4 = GPK_FN_D2D2D2).  Mapping and contract as extend_fn_hess_kernel.  With
// (m1, m2) = MI_f:  C = b[m2] (cd a[m1] + cT a[m1+1]) + a[m1] (cX b[m2+1] + cQ b[m2+3]),  row f = (-1)^(m1+m2) C kappa, the same operations
// whichever other rows are requested; the highest factor is b6 (u_xxx against the d_x^3 column).
struct FnDispArgs {
    const double* px; const double* py;
    int Nd, M;
    double p1, p2;
    const double* tx; int Nt;             // (Nt,2) row-major test points
    const double* coeff;                  // (4 Nd + Nb): T, X, Q blocks, then the delta block
    double* out; long ldo;
};

__host__ __device__ constexpr int dmi_a1(int f) { return f == 1 ? 1 : 0; }
__host__ __device__ constexpr int dmi_a2(int f) { return f >= 2 ? f - 1 : 0; }

template <int MASK>
__global__ __launch_bounds__(256) void extend_fn_disp_kernel(FnDispArgs g) {
    constexpr int NF = fn_popc(MASK);
    const int t0 = blockIdx.x * FN_TT;
    double x1[FN_TT], x2[FN_TT], s[FN_TT][NF];
    GPK_FN_LOAD_POINTS2(x1, x2, g.tx, t0, g.Nt);
    fn_zero(s);
    const long Nd = g.Nd;
    for (int q = threadIdx.x; q < g.M; q += 256) {
        const double y1 = g.px[q], y2 = g.py[q];
        const bool dom = q < g.Nd;
        const double cT = dom ? g.coeff[q] : 0.0, cX = dom ? g.coeff[Nd + q] : 0.0, cQ = dom ? g.coeff[2 * Nd + q] : 0.0;
        const double w0 = g.coeff[3 * Nd + q];
#pragma unroll
        for (int i = 0; i < FN_TT; ++i) {
            const double d1 = x1[i] - y1, d2 = x2[i] - y2;
            const double e = kappa2_fma(g.p1, g.p2, d1, d2);
            double a[5], b[7];
            hermite_compensated(g.p1, d1, a);
            hermite7(g.p2, d2, b);
#pragma unroll
            for (int f = 0; f < 5; ++f)
                if ((MASK >> f) & 1) {
                    const int m1 = dmi_a1(f), m2 = dmi_a2(f);
                    const double A = __builtin_fma(cT, a[m1 + 1], w0 * a[m1]);
                    const double B = __builtin_fma(cQ, b[m2 + 3], cX * b[m2 + 1]);
                    const double c = __builtin_fma(a[m1], B, b[m2] * A);
                    s[i][fn_row(MASK, f)] = __builtin_fma(((m1 + m2) & 1) ? -c : c, e, s[i][fn_row(MASK, f)]);
                }
        }
    }
    GPK_FN_REDUCE_STORE(s, NF, t0, g.Nt, g.out, g.ldo);
}

// one instantiation per compact mask (31)
void launch_extend_fn_disp(int mask, int grid, hipStream_t st, const FnDispArgs& g) {
    with_mask<31>(mask, [&](auto m) { extend_fn_disp_kernel<decltype(m)::value><<<grid, 256, 0, st>>>(g); });
}

// precisions and packed points (the handle's point scratch: 2 arrays of Nd + Nb, re-packed by every call)
int fill_common_disp(gpk_handle h, const char* who, const char* who_kernel, int kernel, const double* kp, const double* Xd, int Nd,
                     const double* Xb, int Nb, double (&p)[2], const double** px, const double** py) {
    if (Nd <= 0 || Nb < 0 || !kp || !Xd || (Nb > 0 && !Xb)) return gpk_bad_arg(h, who);
    GPK_TRY(precisions(h, who_kernel, kernel, kp, 2, p));
    const size_t Mall = (size_t)Nd + (size_t)Nb;
    GPK_TRY(gpk_i_ensure_points(h, 2 * Mall));
    double* s = h->d_pts;
    *px = s; *py = s + Mall;
    pack_disp_kernel<<<gpk_ceil_div((int)Mall, 256), 256, 0, h->stream>>>(Xd, Nd, Xb, Nb, s);
    GPK_LAUNCH_CHECK(h);
    return 0;
}

}  // namespace


extern "C" int gpk_assemble_disp(gpk_handle h, int kernel, const double* kp, const double* Xd, int Nd, const double* Xb, int Nb,
                                 double nugget, int nugget_type, double* Theta, int ld, double* host_ratios3) {
    if (!h || !Theta) return GPK_ERR_ARG;
    if (!nugget_type_valid(nugget_type)) return gpk_bad_arg(h, "assemble_disp: nugget_type");
    if ((long)4 * Nd + Nb > 0x7fffffffL) return gpk_bad_arg(h, "assemble_disp: N exceeds int");
    if (Nd > 0 && Nb >= 0 && ld < 4 * Nd + Nb) return gpk_bad_arg(h, "assemble_disp: ld < N");
    DispArgs g;
    double p[2];
    GPK_TRY(fill_common_disp(h, "assemble_disp: sizes/pointers", "assemble_disp: kernel id", kernel, kp, Xd, Nd, Xb, Nb, p, &g.px, &g.py));
    g.p1 = p[0]; g.p2 = p[1];
    g.Nd = Nd; g.M = Nd + Nb;
    // values at d = 0 (-h2 = p, -h6 = 15 p^3), in long double: the ratios are the analytic values to an ulp
    const long double q1 = p[0], q2 = p[1];
    const long double diag[3] = {q1, q2, 15.0L * q2 * q2 * q2};   // <T,T>, <X,X>, <Q,Q>;  <delta,delta> = 1
    for (int k = 0; k < 3; ++k) {
        const double r = (double)(((long double)Nd * diag[k]) / ((long double)Nd + (long double)Nb));
        if (host_ratios3) host_ratios3[k] = r;
        g.nug[k] = block_nugget(nugget_type, nugget, r);
    }
    g.nug[3] = block_nugget(nugget_type, nugget, 1.0);
    g.out = Theta; g.ld = ld;
    return launch_two_block(h, pairs_eligible(h, Theta, ld, Nd, Nb), g, assemble_disp_kernel, assemble_disp2_kernel<0>, assemble_disp2_kernel<1>);
}

extern "C" int gpk_extend_functionals_disp(gpk_handle h, int kernel, const double* kp, const double* Xt, int Nt,
                                           const double* Xd, int Nd, const double* Xb, int Nb,
                                           const double* coeff, int fmask, double* out, int ldo) {
    if (!h) return GPK_ERR_ARG;
    if (!out || !Xt || !coeff) return gpk_bad_arg(h, "extend_functionals_disp: pointers");
    constexpr int low = GPK_FN_VALUE | GPK_FN_D1 | GPK_FN_D2 | GPK_FN_D2D2;
    if (fmask <= 0 || (fmask & ~(low | GPK_FN_D2D2D2)))
        return gpk_bad_arg(h, "extend_functionals_disp: fmask must be a non-empty subset of GPK_FN_VALUE, _D1, _D2, _D2D2, _D2D2D2");
    if (Nt <= 0) return gpk_bad_arg(h, "extend_functionals_disp: Nt <= 0");
    if (ldo < Nt) return gpk_bad_arg(h, "extend_functionals_disp: ldo < Nt");
    FnDispArgs g;
    double p[2];
    GPK_TRY(fill_common_disp(h, "extend_functionals_disp: sizes/pointers", "extend_functionals_disp: kernel id", kernel, kp, Xd, Nd, Xb, Nb,
                             p, &g.px, &g.py));
    g.p1 = p[0]; g.p2 = p[1];
    g.Nd = Nd; g.M = Nd + Nb;
    g.tx = Xt; g.Nt = Nt; g.coeff = coeff; g.out = out; g.ldo = ldo;
    // compact mask: the four low bits as they are, GPK_FN_D2D2D2 next to them (the ascending order of the rows is kept)
    const int mask = (fmask & low) | ((fmask & GPK_FN_D2D2D2) ? 16 : 0);
    launch_extend_fn_disp(mask, gpk_ceil_div(Nt, FN_TT), h->stream, g);
    GPK_LAUNCH_CHECK(h);
    return 0;
}
