// gpk_assemble_evo.hip -- the fused derivative-kernel evaluator of the evolution layout: the Burgers layout with the second space
// derivative exchanged for a general spatial operator Q = c2 d_x^2 + c3 d_x^3 + c4 d_x^4 + c5 d_x^5 with constant coefficients, for
// u_t + alpha u u_x + Q[u] = f (Kuramoto-Sivashinsky, Kawahara, KdV-Burgers, Benney-Lin; DESIGN.md §K "Evolution equations: the general
// spatial operator"), and with a boundary functional c0 delta + c1 d_t + c2 d_x per boundary point.  The Gram matrix and the matrix-free
// extension with u, u_t, u_x, u_xx, Q[u].
//
// No reference call site: the reference's Gram_matrix_assembly (src/Gram_matrice.py) stops at second derivatives.
//
// Math.  Points are (t, x), notation of gpk_assemble_disp.hip: d = x - y (row point minus column point), a_n = h_n(p1, d1), b_n = h_n(p2, d2),
// a row functional of order (m1, m2) against a column functional of order (n1, n2) is (-1)^(m1+m2) a_(m1+n1) b_(m2+n2) kappa.  Domain point
// i carries T = d_t, X = d_x, Q and B = delta (blocks 0, 1, 2, 3), boundary point b carries B_b = w0 delta + w1 d_t + w2 d_x (block 3);
// N = 4 N_d + N_b.  A domain point is a point with the weights (1, 0, 0), so block 3 has ONE formula.  The sums over k = 2..5 are kept
// in their parts of even and odd order,
//   Se = c2 b2 + c4 b4,  So = c3 b3 + c5 b5      (sum c_k b_k = Se + So,      sum (-1)^k c_k b_k     = Se - So)
//   Ue = c3 b4 + c5 b6,  Uo = c2 b3 + c4 b5      (sum c_k b_(k+1) = Ue + Uo,  sum (-1)^k c_k b_(k+1) = Uo - Ue)
// and the entries of a pair of domain points are (times kappa)
//   <T,T> = -a2   <T,X> = <X,T> = -a1 b1   <X,X> = -b2   <T,Q> = -a1 (Se + So)   <Q,T> = a1 (Se - So)   <X,Q> = -(Ue + Uo)   <Q,X> = Uo - Ue
//   <Q,Q> = g4 b4 + g6 b6 + g8 b8 + g10 b10,   g4 = c2^2, g6 = 2 c2 c4 - c3^2, g8 = c4^2 - 2 c3 c5, g10 = -c5^2
// (the cross terms of odd order cancel; the g are formed once on the host, in long double).  Against a column B with the weights w:
//   <T,B> = -(w0 a1 + w1 a2 + w2 a1 b1)   <X,B> = -(w0 b1 + w1 a1 b1 + w2 b2)   <Q,B> = (w0 + w1 a1)(Se - So) + w2 (Uo - Ue)
// and <B,F> at d is <F,B> at -d with the weights of the row point: the SAME function is called with the odd quantities (a1, b1, So, Uo)
// negated -- h_n(-d) = (-1)^n h_n(d) holds to the bit -- so the entry and its mirror image are the same operations on the same bits.
// <B,B> is written in the grouping that a swap of the two points leaves as it is (v the weights of the row point):
//   v0 w0 + (v0 w1 - v1 w0) a1 + (v0 w2 - v2 w0) b1 - v1 w1 a2 - (v1 w2 + v2 w1) a1 b1 - v2 w2 b2.
// Every value is formed as 0.0 - v, so a zero is +0 on both sides of the diagonal: Theta is symmetric to the bit.
// At d = 0: <Q,Q> = 3 c2^2 p2^2 + 15 c3^2 p2^3 + 105 c4^2 p2^4 + 945 c5^2 p2^5 - 30 c2 c4 p2^3 - 210 c3 c5 p2^4.
//
// Mapping to the hardware, as assemble_disp_kernel: SoA-packed points and weights in the handle's point scratch (5 arrays of Nd+Nb), a
// workgroup owns TP row points x 256 column points (two-point variant: x 512), lane <-> column point (its coordinates and weights stay in
// registers), the row point is wave-uniform (scalar loads).  Fifteen values per point pair.  The kernel is bound by its stores.
#include "gpk_assemble_common.h"

#include <cmath>

using namespace gpk_asm;

// One-point and two-point evaluator must give the same bits for the same point pair: explicit fma, no contraction by the compiler (as
// gpk_assemble_disp.hip).  The extension kernels are written the same way.
#pragma clang fp contract(off)

namespace {

struct EvoOp {                                              // Q: c[k - 2] = c_k, ng = -(g4, g6, g8, g10)
    double c[4];
    double ng[4];
};

struct EvoArgs {
    const double* px; const double* py;                     // SoA points (t, x): domain first, then boundary
    const double* w0; const double* w1; const double* w2;   // weights of the functional of block 3 at every point
    int Nd, M;                                              // M = Nd + Nb
    double p1, p2;
    EvoOp op;
    double* out; long ld;
    double nug[4];
};

// points and the weights of block 3: (1, 0, 0) at a domain point and where bc == NULL
__global__ void pack_evo_kernel(const double* __restrict__ Xd, int Nd, const double* __restrict__ Xb, int Nb, const double* __restrict__ bc,
                                double* __restrict__ s) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t M = (size_t)Nd + (size_t)Nb;
    if (i >= Nd + Nb) return;
    const int b = i - Nd;
    const double* const x = i < Nd ? Xd + 2 * (size_t)i : Xb + 2 * (size_t)b;
    s[i] = x[0]; s[M + i] = x[1];
    const bool given = b >= 0 && bc;
    s[2 * M + i] = given ? bc[3 * (size_t)b] : 1.0;
    s[3 * M + i] = given ? bc[3 * (size_t)b + 1] : 0.0;
    s[4 * M + i] = given ? bc[3 * (size_t)b + 2] : 0.0;
}

// what the entries against block 3 are made of, at d; flipped(): the same at -d, exactly
struct EvoHerm {
    double a1, a2, b1, b2, ab, Se, So, Ue, Uo;
    __host__ __device__ __forceinline__ EvoHerm flipped() const { return EvoHerm{-a1, a2, -b1, b2, ab, Se, -So, Ue, -Uo}; }
};

// the NEGATED entries <T,B>, <X,B>, <Q,B> (row functional at the row point, B with the weights w at the column point), without kappa
__host__ __device__ __forceinline__ double evo_nTB(const EvoHerm& H, double w0, double w1, double w2) {
    return __builtin_fma(w2, H.ab, __builtin_fma(w1, H.a2, w0 * H.a1));
}
__host__ __device__ __forceinline__ double evo_nXB(const EvoHerm& H, double w0, double w1, double w2) {
    return __builtin_fma(w2, H.b2, __builtin_fma(w1, H.ab, w0 * H.b1));
}
__host__ __device__ __forceinline__ double evo_nQB(const EvoHerm& H, double w0, double w1, double w2) {
    return __builtin_fma(w2, H.Ue - H.Uo, __builtin_fma(w1, H.a1, w0) * (H.So - H.Se));
}

// the fifteen values of one point pair, d = x - y (row point minus column point); v: weights of the row point, w: of the column point
struct PairEvo {
    double TT, TX, TQ, QT, XX, XQ, QX, QQ;                  // both points are domain points
    double TB, XB, QB;                                      // the row point is a domain point
    double BT, BX, BQ;                                      // the column point is a domain point
    double BB;
    __host__ __device__ __forceinline__ void eval(double p1, double p2, const EvoOp& op, double d1, double d2,
                                                  double v0, double v1, double v2, double w0, double w1, double w2, bool rowdom, bool coldom) {
        double a[5];
        const double e = kappa2_fma(p1, p2, d1, d2);
        hermite_compensated(p1, d1, a);
        EvoHerm H;
        H.a1 = a[1]; H.a2 = a[2];
        if (!(rowdom || coldom)) {                          // two boundary points: first order in x
            double b[5];
            hermite_compensated(p2, d2, b);
            H.b1 = b[1]; H.b2 = b[2]; H.ab = a[1] * b[1];
        } else {
            double b[11];
            hermite_recurrence(p2, d2, b);
            H.b1 = b[1]; H.b2 = b[2]; H.ab = a[1] * b[1];
            H.Se = __builtin_fma(op.c[2], b[4], op.c[0] * b[2]);
            H.So = __builtin_fma(op.c[3], b[5], op.c[1] * b[3]);
            H.Ue = __builtin_fma(op.c[3], b[6], op.c[1] * b[4]);
            H.Uo = __builtin_fma(op.c[2], b[5], op.c[0] * b[3]);
            if (rowdom && coldom) {
                // 0.0 - v, not -v: a zero comes out as +0 whichever sign its factors gave it (gpk_assemble_disp.hip)
                TT = 0.0 - a[2] * e;
                TX = 0.0 - H.ab * e;
                XX = 0.0 - b[2] * e;
                TQ = 0.0 - (a[1] * (H.Se + H.So)) * e;
                QT = 0.0 - (a[1] * (H.So - H.Se)) * e;
                XQ = 0.0 - (H.Ue + H.Uo) * e;
                QX = 0.0 - (H.Ue - H.Uo) * e;
                QQ = 0.0 - __builtin_fma(op.ng[3], b[10], __builtin_fma(op.ng[2], b[8], __builtin_fma(op.ng[1], b[6], op.ng[0] * b[4]))) * e;
            }
            if (rowdom) {
                TB = 0.0 - evo_nTB(H, w0, w1, w2) * e;
                XB = 0.0 - evo_nXB(H, w0, w1, w2) * e;
                QB = 0.0 - evo_nQB(H, w0, w1, w2) * e;
            }
            if (coldom) {                                   // <B,F> at d = <F,B> at -d with the weights of the row point
                const EvoHerm F = H.flipped();
                BT = 0.0 - evo_nTB(F, v0, v1, v2) * e;
                BX = 0.0 - evo_nXB(F, v0, v1, v2) * e;
                BQ = 0.0 - evo_nQB(F, v0, v1, v2) * e;
            }
        }
        double s = -(v0 * w0);                              // the negated sum, in the grouping a swap of the points leaves as it is
        s = __builtin_fma(v1 * w0 - v0 * w1, H.a1, s);
        s = __builtin_fma(v2 * w0 - v0 * w2, H.b1, s);
        s = __builtin_fma(v1 * w1, H.a2, s);
        s = __builtin_fma(v1 * w2 + v2 * w1, H.ab, s);
        s = __builtin_fma(v2 * w2, H.b2, s);
        BB = 0.0 - s * e;
    }
};

// one column point per lane, 8-byte stores: any alignment, any Nd / Nb
__global__ __launch_bounds__(256) void assemble_evo_kernel(EvoArgs g) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    const bool live = q < g.M;
    const bool dom = q < g.Nd;
    const double y1 = live ? g.px[q] : 0.0, y2 = live ? g.py[q] : 0.0;
    const double w0 = live ? g.w0[q] : 0.0, w1 = live ? g.w1[q] : 0.0, w2 = live ? g.w2[q] : 0.0;
    const int p0 = blockIdx.y * TP;
    const int pend = min(p0 + TP, g.M);
    const long Nd = g.Nd;
    double* const cT = g.out + q;                           // column q of the blocks T, X, Q (q < Nd only) and B
    double* const cX = g.out + Nd + q;
    double* const cQ = g.out + 2 * Nd + q;
    double* const cB = g.out + 3 * Nd + q;
    for (int p = p0; p < pend; ++p) {
        const double x1 = g.px[p], x2 = g.py[p];            // uniform address -> scalar loads
        const double v0 = g.w0[p], v1 = g.w1[p], v2 = g.w2[p];
        if (!live) continue;
        PairEvo u;
        u.eval(g.p1, g.p2, g.op, x1 - y1, x2 - y2, v0, v1, v2, w0, w1, w2, p < g.Nd, dom);
        const bool diag = p == q;
        if (p < g.Nd) {                                     // wave-uniform: rows p of the blocks T, X, Q
            const long rT = (long)p * g.ld, rX = (Nd + p) * g.ld, rQ = (2 * Nd + p) * g.ld;
            if (dom) {
                cT[rT] = u.TT + (diag ? g.nug[0] : 0.0); cX[rT] = u.TX; cQ[rT] = u.TQ;
                cT[rX] = u.TX; cX[rX] = u.XX + (diag ? g.nug[1] : 0.0); cQ[rX] = u.XQ;
                cT[rQ] = u.QT; cX[rQ] = u.QX; cQ[rQ] = u.QQ + (diag ? g.nug[2] : 0.0);
            }
            cB[rT] = u.TB; cB[rX] = u.XB; cB[rQ] = u.QB;
        }
        const long rB = (3 * Nd + p) * g.ld;                // row p of block 3 (p < M always)
        if (dom) { cT[rB] = u.BT; cX[rB] = u.BX; cQ[rB] = u.BQ; }
        cB[rB] = u.BB + (diag ? g.nug[3] : 0.0);
    }
}

// Two column points per lane, one 16-byte store per (row block, column block, row point).  Needs Nd, Nb and the leading dimension
// even and a 16-byte aligned base (checked by the launcher; otherwise the one-point-per-lane kernel above runs).
// NT: the policy of store2 (0 plain, 1 non-temporal).
template <int NT>
__global__ __launch_bounds__(256) void assemble_evo2_kernel(EvoArgs g) {
    const int q = 2 * (blockIdx.x * 256 + threadIdx.x);
    const bool live = q < g.M;                              // (M even: q + 1 < M as well)
    const bool dom = q < g.Nd;                              // (Nd even: q and q + 1 are both domain points or both boundary points)
    const double y1a = live ? g.px[q] : 0.0, y2a = live ? g.py[q] : 0.0;
    const double y1b = live ? g.px[q + 1] : 0.0, y2b = live ? g.py[q + 1] : 0.0;
    const double w0a = live ? g.w0[q] : 0.0, w1a = live ? g.w1[q] : 0.0, w2a = live ? g.w2[q] : 0.0;
    const double w0b = live ? g.w0[q + 1] : 0.0, w1b = live ? g.w1[q + 1] : 0.0, w2b = live ? g.w2[q + 1] : 0.0;
    const int p0 = blockIdx.y * TP;
    const int pend = min(p0 + TP, g.M);
    const long Nd = g.Nd;
    double* const cT = g.out + q;
    double* const cX = g.out + Nd + q;
    double* const cQ = g.out + 2 * Nd + q;
    double* const cB = g.out + 3 * Nd + q;
    for (int p = p0; p < pend; ++p) {
        const double x1 = g.px[p], x2 = g.py[p];            // uniform address -> scalar loads
        const double v0 = g.w0[p], v1 = g.w1[p], v2 = g.w2[p];
        if (!live) continue;
        PairEvo u, v;
        u.eval(g.p1, g.p2, g.op, x1 - y1a, x2 - y2a, v0, v1, v2, w0a, w1a, w2a, p < g.Nd, dom);
        v.eval(g.p1, g.p2, g.op, x1 - y1b, x2 - y2b, v0, v1, v2, w0b, w1b, w2b, p < g.Nd, dom);
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
                store2<NT>(cT + rQ, u.QT, v.QT);
                store2<NT>(cX + rQ, u.QX, v.QX);
                store2<NT>(cQ + rQ, u.QQ + (du ? g.nug[2] : 0.0), v.QQ + (dv ? g.nug[2] : 0.0));
            }
            store2<NT>(cB + rT, u.TB, v.TB);
            store2<NT>(cB + rX, u.XB, v.XB);
            store2<NT>(cB + rQ, u.QB, v.QB);
        }
        const long rB = (3 * Nd + p) * g.ld;
        if (dom) {
            store2<NT>(cT + rB, u.BT, v.BT);
            store2<NT>(cX + rB, u.BX, v.BX);
            store2<NT>(cQ + rB, u.BQ, v.BQ);
        }
        store2<NT>(cB + rB, u.BB + (du ? g.nug[3] : 0.0), v.BB + (dv ? g.nug[3] : 0.0));
    }
}

// ---- the extension with u, u_t, u_x, u_xx, Q[u] -------------------------------------------------------------------------------------------
// out[f][t] = sum_q <row functional f at x_t, (cT d_t + cX d_x + cQ Q + cB B)_q> kappa, f over the set bits of MASK (the compact mask of
// the launcher: bit 4 = GPK_FN_Q).  Mapping and contract as extend_fn_disp_kernel.  With eT = cT + cB w1, eX = cX + cB w2, e0 = cB w0 the
// column functional is e0 delta + eT d_t + eX d_x + cQ Q, and for the rows of order (m1, m2) = (0,0), (1,0), (0,1), (0,2)
//   C = b[m2] (e0 a[m1] + eT a[m1+1]) + a[m1] (eX b[m2+1] + cQ sum_k c_k b[m2+k]),  row f = (-1)^(m1+m2) C kappa  (highest factor b7),
// for the row Q:  C = (e0 + eT a1)(Se - So) + eX (Uo - Ue) + cQ <Q,Q>  (highest factor b10; computed only where the row is requested).
struct FnEvoArgs {
    const double* px; const double* py;
    const double* w0; const double* w1; const double* w2;
    int Nd, M;
    double p1, p2;
    EvoOp op;
    const double* tx; int Nt;             // (Nt,2) row-major test points
    const double* coeff;                  // (4 Nd + Nb): T, X, Q blocks, then block 3
    double* out; long ldo;
};

__host__ __device__ constexpr int emi_a1(int f) { return f == 1 ? 1 : 0; }
__host__ __device__ constexpr int emi_a2(int f) { return f >= 2 ? f - 1 : 0; }

template <int MASK>
__global__ __launch_bounds__(256) void extend_fn_evo_kernel(FnEvoArgs g) {
    constexpr int NF = fn_popc(MASK);
    constexpr int NB = (MASK & 16) ? 11 : 8;               // Hermite factors of the space axis
    const int t0 = blockIdx.x * FN_TT;
    double x1[FN_TT], x2[FN_TT], s[FN_TT][NF];
    GPK_FN_LOAD_POINTS2(x1, x2, g.tx, t0, g.Nt);
    fn_zero(s);
    const long Nd = g.Nd;
    const double c2 = g.op.c[0], c3 = g.op.c[1], c4 = g.op.c[2], c5 = g.op.c[3];
    for (int q = threadIdx.x; q < g.M; q += 256) {
        const double y1 = g.px[q], y2 = g.py[q];
        const bool dom = q < g.Nd;
        const double cT = dom ? g.coeff[q] : 0.0, cX = dom ? g.coeff[Nd + q] : 0.0, cQ = dom ? g.coeff[2 * Nd + q] : 0.0;
        const double cB = g.coeff[3 * Nd + q];
        const double e0 = cB * g.w0[q], eT = __builtin_fma(cB, g.w1[q], cT), eX = __builtin_fma(cB, g.w2[q], cX);
#pragma unroll
        for (int i = 0; i < FN_TT; ++i) {
            const double d1 = x1[i] - y1, d2 = x2[i] - y2;
            const double e = kappa2_fma(g.p1, g.p2, d1, d2);
            double a[5], b[NB];
            hermite_compensated(g.p1, d1, a);
            hermite_recurrence(g.p2, d2, b);
#pragma unroll
            for (int f = 0; f < 4; ++f)
                if ((MASK >> f) & 1) {
                    const int m1 = emi_a1(f), m2 = emi_a2(f);
                    const double W = __builtin_fma(c5, b[m2 + 5], __builtin_fma(c4, b[m2 + 4], __builtin_fma(c3, b[m2 + 3], c2 * b[m2 + 2])));
                    const double A = __builtin_fma(eT, a[m1 + 1], e0 * a[m1]);
                    const double B = __builtin_fma(cQ, W, eX * b[m2 + 1]);
                    const double c = __builtin_fma(a[m1], B, b[m2] * A);
                    s[i][fn_row(MASK, f)] = __builtin_fma(((m1 + m2) & 1) ? -c : c, e, s[i][fn_row(MASK, f)]);
                }
            if (MASK & 16) {
                constexpr int L = NB - 1;                  // (10; written so that b[L] is in range where the branch is not compiled)
                const double Se = __builtin_fma(c4, b[4], c2 * b[2]), So = __builtin_fma(c5, b[5], c3 * b[3]);
                const double Ue = __builtin_fma(c5, b[6], c3 * b[4]), Uo = __builtin_fma(c4, b[5], c2 * b[3]);
                const double nqq = __builtin_fma(g.op.ng[3], b[L], __builtin_fma(g.op.ng[2], b[L - 2], __builtin_fma(g.op.ng[1], b[6], g.op.ng[0] * b[4])));
                const double A = __builtin_fma(eT, a[1], e0);
                const double c = __builtin_fma(cQ, -nqq, __builtin_fma(eX, Uo - Ue, A * (Se - So)));
                s[i][fn_row(MASK, 4)] = __builtin_fma(c, e, s[i][fn_row(MASK, 4)]);
            }
        }
    }
    GPK_FN_REDUCE_STORE(s, NF, t0, g.Nt, g.out, g.ldo);
}

// one instantiation per compact mask (31)
void launch_extend_fn_evo(int mask, int grid, hipStream_t st, const FnEvoArgs& g) {
    with_mask<31>(mask, [&](auto m) { extend_fn_evo_kernel<decltype(m)::value><<<grid, 256, 0, st>>>(g); });
}

// the operator: c2..c5 finite and not all zero; -(g4, g6, g8, g10) in long double
int fill_operator_evo(gpk_handle h, const char* who, const double* c4, EvoOp* op) {
    if (!c4) return gpk_bad_arg(h, who);
    bool any = false;
    for (int k = 0; k < 4; ++k) {
        if (!std::isfinite(c4[k])) return gpk_bad_arg(h, who);
        any = any || c4[k] != 0.0;
        op->c[k] = c4[k];
    }
    if (!any) return gpk_bad_arg(h, who);
    const long double c2 = c4[0], c3 = c4[1], c4_ = c4[2], c5 = c4[3];
    op->ng[0] = (double)(-(c2 * c2));
    op->ng[1] = (double)(c3 * c3 - 2.0L * c2 * c4_);
    op->ng[2] = (double)(2.0L * c3 * c5 - c4_ * c4_);
    op->ng[3] = (double)(c5 * c5);
    return 0;
}

// precisions, packed points and weights (the handle's point scratch: 5 arrays of Nd + Nb, re-packed by every call)
int fill_common_evo(gpk_handle h, const char* who, const char* who_kernel, int kernel, const double* kp, const double* Xd, int Nd,
                    const double* Xb, int Nb, const double* bc, double (&p)[2], const double** s5) {
    if (Nd <= 0 || Nb < 0 || !kp || !Xd || (Nb > 0 && !Xb)) return gpk_bad_arg(h, who);
    GPK_TRY(precisions(h, who_kernel, kernel, kp, 2, p));
    const size_t Mall = (size_t)Nd + (size_t)Nb;
    GPK_TRY(gpk_i_ensure_points(h, 5 * Mall));
    double* s = h->d_pts;
    for (int k = 0; k < 5; ++k) s5[k] = s + k * Mall;
    pack_evo_kernel<<<gpk_ceil_div((int)Mall, 256), 256, 0, h->stream>>>(Xd, Nd, Xb, Nb, Nb > 0 ? bc : nullptr, s);
    GPK_LAUNCH_CHECK(h);
    return 0;
}

}  // namespace


extern "C" int gpk_assemble_evo(gpk_handle h, int kernel, const double* kp, const double* host_c4, const double* Xd, int Nd,
                                const double* Xb, int Nb, const double* bc, double nugget, int nugget_type, double* Theta, int ld,
                                double* host_ratios3) {
    if (!h || !Theta) return GPK_ERR_ARG;
    if (!nugget_type_valid(nugget_type)) return gpk_bad_arg(h, "assemble_evo: nugget_type");
    if ((long)4 * Nd + Nb > 0x7fffffffL) return gpk_bad_arg(h, "assemble_evo: N exceeds int");
    if (Nd > 0 && Nb >= 0 && ld < 4 * Nd + Nb) return gpk_bad_arg(h, "assemble_evo: ld < N");
    EvoArgs g;
    GPK_TRY(fill_operator_evo(h, "assemble_evo: c2..c5 must be finite and not all zero", host_c4, &g.op));
    double p[2];
    const double* s5[5];
    GPK_TRY(fill_common_evo(h, "assemble_evo: sizes/pointers", "assemble_evo: kernel id", kernel, kp, Xd, Nd, Xb, Nb, bc, p, s5));
    g.px = s5[0]; g.py = s5[1]; g.w0 = s5[2]; g.w1 = s5[3]; g.w2 = s5[4];
    g.p1 = p[0]; g.p2 = p[1];
    g.Nd = Nd; g.M = Nd + Nb;
    // values at d = 0 in long double: the ratios are the analytic values to an ulp.  <Q,Q> = sum g_n b_n(0) with b4 = 3 p^2, b6 = -15 p^3,
    // b8 = 105 p^4, b10 = -945 p^5; trace(block 3) = Nd + sum_b (c0^2 + p1 c1^2 + p2 c2^2)
    const long double q1 = p[0], q2 = p[1];
    const long double c2 = host_c4[0], c3 = host_c4[1], c4 = host_c4[2], c5 = host_c4[3];
    const long double qq = 3.0L * c2 * c2 * q2 * q2 + 15.0L * (c3 * c3 - 2.0L * c2 * c4) * q2 * q2 * q2
                           + 105.0L * (c4 * c4 - 2.0L * c3 * c5) * q2 * q2 * q2 * q2 + 945.0L * c5 * c5 * q2 * q2 * q2 * q2 * q2;
    const long double diag[3] = {q1, q2, qq};               // <T,T>, <X,X>, <Q,Q>
    long double trb;
    GPK_TRY(boundary_trace(h, bc, Nb, q1, q2, &trb));
    for (int k = 0; k < 3; ++k) {
        const double r = (double)(((long double)Nd * diag[k]) / ((long double)Nd + trb));
        if (host_ratios3) host_ratios3[k] = r;
        g.nug[k] = block_nugget(nugget_type, nugget, r);
    }
    g.nug[3] = block_nugget(nugget_type, nugget, 1.0);
    g.out = Theta; g.ld = ld;
    return launch_two_block(h, pairs_eligible(h, Theta, ld, Nd, Nb), g, assemble_evo_kernel, assemble_evo2_kernel<0>, assemble_evo2_kernel<1>);
}

extern "C" int gpk_extend_functionals_evo(gpk_handle h, int kernel, const double* kp, const double* host_c4, const double* Xt, int Nt,
                                          const double* Xd, int Nd, const double* Xb, int Nb, const double* bc,
                                          const double* coeff, int fmask, double* out, int ldo) {
    if (!h) return GPK_ERR_ARG;
    if (!out || !Xt || !coeff) return gpk_bad_arg(h, "extend_functionals_evo: pointers");
    constexpr int low = GPK_FN_VALUE | GPK_FN_D1 | GPK_FN_D2 | GPK_FN_D2D2;
    if (fmask <= 0 || (fmask & ~(low | GPK_FN_Q)))
        return gpk_bad_arg(h, "extend_functionals_evo: fmask must be a non-empty subset of GPK_FN_VALUE, _D1, _D2, _D2D2, GPK_FN_Q");
    if (Nt <= 0) return gpk_bad_arg(h, "extend_functionals_evo: Nt <= 0");
    if (ldo < Nt) return gpk_bad_arg(h, "extend_functionals_evo: ldo < Nt");
    FnEvoArgs g;
    GPK_TRY(fill_operator_evo(h, "extend_functionals_evo: c2..c5 must be finite and not all zero", host_c4, &g.op));
    double p[2];
    const double* s5[5];
    GPK_TRY(fill_common_evo(h, "extend_functionals_evo: sizes/pointers", "extend_functionals_evo: kernel id", kernel, kp, Xd, Nd, Xb, Nb, bc,
                            p, s5));
    g.px = s5[0]; g.py = s5[1]; g.w0 = s5[2]; g.w1 = s5[3]; g.w2 = s5[4];
    g.p1 = p[0]; g.p2 = p[1];
    g.Nd = Nd; g.M = Nd + Nb;
    g.tx = Xt; g.Nt = Nt; g.coeff = coeff; g.out = out; g.ldo = ldo;
    // compact mask: the four low bits as they are, GPK_FN_Q next to them (the ascending order of the rows is kept)
    const int mask = (fmask & low) | ((fmask & GPK_FN_Q) ? 16 : 0);
    launch_extend_fn_evo(mask, gpk_ceil_div(Nt, FN_TT), h->stream, g);
    GPK_LAUNCH_CHECK(h);
    return 0;
}
