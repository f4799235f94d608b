// gpk_assemble_grad3d.hip -- the fused derivative-kernel evaluator of the 3-D GRADIENT layout: the three first derivatives of u at every
// domain point as row blocks of their own, next to a general second-order functional psi_i and the value (boundary points: a first-order
// functional phi_b).  The Gram matrix, the matrix-free extension with all derivatives up to order two, and the pointwise residual of
// -psi[u] + N(u, grad u) = f.  It is what an equation that is nonlinear in grad u needs in three dimensions -- and, with axis 3 as time,
// a time-dependent one in two space dimensions (GPK_GN_SEMILINEAR3D, src/PDEs.py: Semilinear3d).
//
// No reference call site (the reference is 2-D; its Eikonal layout is the planar counterpart with psi = the Laplacian).
//
// Layout (DESIGN.md §K "Gradient layout in three dimensions").  Blocks 0, 1, 2 = d_1, d_2, d_3 on the Nd domain points, block 3 = psi_i =
// sum_j op3[i][j] d^MI3_j on the domain points, block 4 = delta on the domain points followed by phi_b = bc3[b][0] delta + sum_k bc3[b][k]
// d_k on the Nb boundary points: N = 5 Nd + Nb.  op3 / bc3 exactly as for gpk_assemble_op3d, whose blocks 0 and 1 are the blocks 3 and 4
// here.  Per point pair, with C_G[m] = the contraction of the column functional G with the three Hermite tables (gpk_assemble_op3.h):
//   <d_k, G'> = -C_G[e_k] kappa,   <psi, G'> = sum_i ro_i (-1)^{|MI3_i|} C_G[MI3_i] kappa,   <phi, G'> likewise over the first four.
// The column functional d_k' is the unit-coefficient case of table_phi3: C[m] = a[m1 + (k=1)] b[m2 + (k=2)] c[m3 + (k=3)], which is what
// that table returns for k = e_k operation by operation (its other terms are products with 0) -- written as that product of three
// factors, one loop over MI3 for the three axes, because a multiplication by a literal 0 is not folded away under IEEE rules.
// One exp and three Hermite evaluations per POINT PAIR feed all blocks of that pair: 25 entries domain-domain, 5 against a boundary
// column or row, 1 boundary-boundary.
//
// Mapping to the hardware, as assemble_op3_kernel / assemble_op3_2_kernel: the packed scratch of gpk_assemble_op3.h (3 + 4 + 10 arrays of
// Nd+Nb), a workgroup owns TP row points x 256 column points (two-point variant: x 512), lane <-> column point (coordinates and 14
// coefficients in registers), the row point and its coefficients are wave-uniform and arrive by scalar loads through the constant
// address space.  The two-point variant evaluates its two column points one after the other and keeps the 25 finished entries of the
// first only.  No inline assembly, no LDS in the Gram kernels.
#include "gpk_assemble_op3.h"

using namespace gpk_asm;

// One-point and two-point evaluator must give the same bits for the same point pair: explicit fma, no contraction by the compiler.
// The extension kernels and the residual are written the same way.
#pragma clang fp contract(off)

namespace {

constexpr int NB = 5;                     // row / column blocks

struct Grad3Args {
    const double* s;                      // packed scratch: array k (x, y, z, phi 0..3, psi 0..9) at s + k * M; domain points first
    int Nd, M;                            // M = Nd + Nb
    double p1, p2, p3;
    double* out; long ld;
    double nug[NB];
    __device__ cdouble_p arr(int k) const { return (cdouble_p)(s + (size_t)k * (size_t)M); }
};

// the column point of a lane: coordinates, coefficients of phi' and of psi'
struct ColG {
    double y[3], k[NC], ko[NO];
    __device__ __forceinline__ void load(const Grad3Args& g, int q, bool live) {
#pragma unroll
        for (int j = 0; j < 3; ++j) y[j] = live ? g.arr(j)[q] : 0.0;
#pragma unroll
        for (int j = 0; j < NC; ++j) k[j] = live ? g.arr(3 + j)[q] : 0.0;
#pragma unroll
        for (int j = 0; j < NO; ++j) ko[j] = live ? g.arr(3 + NC + j)[q] : 0.0;
    }
};

// the row point of a workgroup's step (wave-uniform)
struct RowG {
    double x[3], r[NC], ro[NO];
    __device__ __forceinline__ void load(const Grad3Args& g, int p) {               // uniform address -> scalar loads
#pragma unroll
        for (int j = 0; j < 3; ++j) x[j] = g.arr(j)[p];
#pragma unroll
        for (int j = 0; j < NC; ++j) r[j] = g.arr(3 + j)[p];
#pragma unroll
        for (int j = 0; j < NO; ++j) ro[j] = g.arr(3 + NC + j)[p];
    }
};

// table_phi3 for the column functional d_K' (k = e_K, K = 1, 2, 3): the one term that unit vector leaves, axis 1 first
template <int K>
__device__ __forceinline__ void table_grad3(const double (&a)[5], const double (&b)[5], const double (&c)[5], double (&t)[NO]) {
#pragma unroll
    for (int m1 = 0; m1 < 3; ++m1)
#pragma unroll
        for (int m2 = 0; m1 + m2 < 3; ++m2) {
            const double B = b[m2 + (K == 2)] * a[m1 + (K == 1)];
#pragma unroll
            for (int m3 = 0; m1 + m2 + m3 < 3; ++m3) t[mi3(m1, m2, m3)] = c[m3 + (K == 3)] * B;
        }
}

// the rows of one column functional from its table: v[0..2] = <d_k, .>, v[3] = <psi, .> (when `top`), v[4] = <phi, .>
__device__ __forceinline__ void column_rows(const double (&t)[NO], const RowG& w, bool top, double e, double (&v)[NB]) {
    if (top) {
        v[0] = -t[1] * e;
        v[1] = -t[2] * e;
        v[2] = -t[3] * e;
        v[3] = row_psi3(t, w.ro) * e;
    }
    v[4] = row_phi3(t, w.r) * e;
}

// The entries one point pair contributes: v[j][i] = <row block i at x, column block j at y> (row blocks 0..3: when `top`; column blocks
// 0..3: when `dom`; the others are left as they are).  One function for both evaluators: the same operations.
__device__ __forceinline__ void pair_entries(const Grad3Args& g, const RowG& w, const ColG& u, bool top, bool dom, double (&v)[NB][NB]) {
    const double d1 = w.x[0] - u.y[0], d2 = w.x[1] - u.y[1], d3 = w.x[2] - u.y[2];
    const double e = kappa3_fma(g.p1, g.p2, g.p3, d1, d2, d3);
    double a[5], b[5], c[5], t[NO];
    hermite_compensated(g.p1, d1, a);
    hermite_compensated(g.p2, d2, b);
    hermite_compensated(g.p3, d3, c);
    table_phi3(a, b, c, u.k, t);
    column_rows(t, w, top, e, v[4]);
    if (dom) {
        table_grad3<1>(a, b, c, t);
        column_rows(t, w, top, e, v[0]);
        table_grad3<2>(a, b, c, t);
        column_rows(t, w, top, e, v[1]);
        table_grad3<3>(a, b, c, t);
        column_rows(t, w, top, e, v[2]);
        table_psi3<>(a, b, c, u.ko, t);
        column_rows(t, w, top, e, v[3]);
    }
}

// one column point per lane, 8-byte stores: any alignment, any Nd / Nb
__global__ __launch_bounds__(256) void assemble_grad3_kernel(Grad3Args g) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    const bool live = q < g.M;
    const bool dom = q < g.Nd;
    ColG u;
    u.load(g, q, live);
    const int p0 = blockIdx.y * TP;
    const int pend = min(p0 + TP, g.M);
    const long Nd = g.Nd;
    double* const col = g.out + q;                          // column q of block j at col + j * Nd (j < 4: q < Nd only)
    for (int p = p0; p < pend; ++p) {
        RowG w;
        w.load(g, p);
        if (!live) continue;
        const bool top = p < g.Nd;                          // wave-uniform: row p of the blocks 0..3 exists
        const bool diag = p == q;
        double v[NB][NB];
        pair_entries(g, w, u, top, dom, v);
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            if (i < 4 && !top) continue;
            const long row = (i * Nd + p) * g.ld;
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                if (j < 4 && !dom) continue;
                col[row + j * Nd] = v[j][i] + (i == j && diag ? g.nug[i] : 0.0);
            }
        }
    }
}

// Two column points per lane, one 16-byte store per (row block, column block, row point).  Needs Nd, Nb and the leading dimension
// even and a 16-byte aligned base (checked by the launcher; otherwise the one-point-per-lane kernel above runs).  The two points are
// evaluated one after the other: only the 25 entries of the first stay live while the second is computed.
// NT: the policy of store2 (0 plain, 1 non-temporal).
template <int NT>
__global__ __launch_bounds__(256) void assemble_grad3_2_kernel(Grad3Args g) {
    const int q = 2 * (blockIdx.x * 256 + threadIdx.x);
    const bool live = q < g.M;                              // (M even: q + 1 < M as well)
    const bool dom = q < g.Nd;                              // (Nd even: q and q + 1 are both domain points or both boundary points)
    ColG ua, ub;
    ua.load(g, q, live);
    ub.load(g, q + 1, live);
    const int p0 = blockIdx.y * TP;
    const int pend = min(p0 + TP, g.M);
    const long Nd = g.Nd;
    double* const col = g.out + q;
    for (int p = p0; p < pend; ++p) {
        RowG w;
        w.load(g, p);
        if (!live) continue;
        const bool top = p < g.Nd;                          // wave-uniform
        const bool da = p == q, db = p == q + 1;
        double va[NB][NB], vb[NB][NB];
        pair_entries(g, w, ua, top, dom, va);
        pair_entries(g, w, ub, top, dom, vb);
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            if (i < 4 && !top) continue;
            const long row = (i * Nd + p) * g.ld;
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                if (j < 4 && !dom) continue;
                store2<NT>(col + row + j * Nd, va[j][i] + (i == j && da ? g.nug[i] : 0.0), vb[j][i] + (i == j && db ? g.nug[i] : 0.0));
            }
        }
    }
}

// ---- the extension with all derivatives up to order two -----------------------------------------------------------------------------
// out[row(f)][t] = sum_q <d^MI3_f at x_t, (c_1 d_1 + c_2 d_2 + c_3 d_3 + c_psi psi_q + c_phi phi_q)> kappa, f over the set bits of mask (the
// GPK_OP3FN_* bits), coeff = [c_1 | c_2 | c_3 | c_psi | c_phi] in the order of the blocks.  Frame, instantiations (NE = 1, 4, 10) and contract
// as extend_fn_op3_kernel: all five blocks of a column point act through ONE second-order functional with the weights
// w = op3_q c_psi[q] + (bc3_q, 0...0) c_phi[q], then w_k += c_k[q] for the three first derivatives, formed once per column point.  The
// operations behind an entry do not depend on NE, so a row has the same bits whichever other rows are requested.  Reduction by wave
// shuffles, then LDS across the 4 waves, in a fixed order (no atomics: a repeated call gives bit-identical output).
struct FnGrad3Args {
    const double* s;
    int Nd, M;
    double p1, p2, p3;
    const double* tx; int Nt;             // (Nt,3) row-major test points
    const double* coeff;                  // (5 Nd + Nb)
    int mask;                             // the rows to store
    double* out; long ldo;
    __host__ __device__ const double* arr(int k) const { return s + (size_t)k * (size_t)M; }
};

template <int NE>
__global__ __launch_bounds__(256) void extend_fn_grad3_kernel(FnGrad3Args g) {
    const int t0 = blockIdx.x * FN_TT;
    double x1[FN_TT], x2[FN_TT], x3[FN_TT], s[FN_TT][NE];
    GPK_FN_LOAD_POINTS3(x1, x2, x3, g.tx, t0, g.Nt);
    fn_zero(s);
    const long Nd = g.Nd;
    for (int q = threadIdx.x; q < g.M; q += 256) {
        const double y1 = g.arr(0)[q], y2 = g.arr(1)[q], y3 = g.arr(2)[q];
        const bool dom = q < g.Nd;
        const double cl = dom ? g.coeff[3 * Nd + q] : 0.0;            // psi block: domain points only (psi is packed as 0 elsewhere)
        const double cd = g.coeff[4 * Nd + q];                        // phi block: every point
        double w[NO];
#pragma unroll
        for (int j = 0; j < NC; ++j) w[j] = __builtin_fma(g.arr(3 + j)[q], cd, g.arr(3 + NC + j)[q] * cl);
#pragma unroll
        for (int j = NC; j < NO; ++j) w[j] = g.arr(3 + NC + j)[q] * cl;
#pragma unroll
        for (int k = 0; k < 3; ++k) w[1 + k] = w[1 + k] + (dom ? g.coeff[k * Nd + q] : 0.0);   // gradient blocks: domain points only
#pragma unroll
        for (int i = 0; i < FN_TT; ++i) {
            const double d1 = x1[i] - y1, d2 = x2[i] - y2, d3 = x3[i] - y3;
            const double e = kappa3_fma(g.p1, g.p2, g.p3, d1, d2, d3);
            double a[5], b[5], c[5], t[NO];
            hermite_compensated(g.p1, d1, a);
            hermite_compensated(g.p2, d2, b);
            hermite_compensated(g.p3, d3, c);
            table_psi3<NE>(a, b, c, w, t);
#pragma unroll
            for (int f = 0; f < NE; ++f) s[i][f] = __builtin_fma((f >= 1 && f <= 3) ? -t[f] : t[f], e, s[i][f]);
        }
    }
    GPK_FN_REDUCE_STORE_MASKED(s, NE, g.mask, t0, g.Nt, g.out, g.ldo);
}

// out[t] = -psi_u + N(u0, u1, u2, u3) - f, one fixed order of operations (sl3_N of gpk_common.h; no contraction in this file)
__global__ __launch_bounds__(256) void pde_residual_sl3d_kernel(Sl3Coef gq, int Nt, const double* __restrict__ u, long ldu,
                                                                const double* __restrict__ psi_u, const double* __restrict__ rhs,
                                                                double* __restrict__ out) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= Nt) return;
    const double n = sl3_N(gq.c, u[t], u[ldu + t], u[2 * ldu + t], u[3 * ldu + t]);
    out[t] = (n - psi_u[t]) - rhs[t];
}

}  // namespace


extern "C" int gpk_assemble_grad3d(gpk_handle h, int kernel, const double* kp, const double* Xd, int Nd, const double* Xb, int Nb,
                                   const double* op3, const double* bc3, double nugget, int nugget_type, double* Theta, int ld,
                                   double* host_ratios4) {
    if (!h) return GPK_ERR_ARG;
    if (!Theta) return gpk_bad_arg(h, "assemble_grad3d: Theta");
    if (!nugget_type_valid(nugget_type)) return gpk_bad_arg(h, "assemble_grad3d: nugget_type");
    if ((long)5 * Nd + Nb > 0x7fffffffL) return gpk_bad_arg(h, "assemble_grad3d: N exceeds int");
    if (Nd > 0 && Nb >= 0 && ld < 5 * Nd + Nb) return gpk_bad_arg(h, "assemble_grad3d: ld < N");
    Grad3Args g;
    double p[3];
    GPK_TRY(fill_common_op3(h, "assemble_grad3d: sizes/pointers", "assemble_grad3d: kernel id", kernel, kp, Xd, Nd, Xb, Nb, op3, bc3, p, &g.s));
    g.p1 = p[0]; g.p2 = p[1]; g.p3 = p[2];
    g.Nd = Nd; g.M = Nd + Nb;
    // values at d = 0: <d_k, d_k> = p_k, <psi, psi> and <phi, phi> as gpk_assemble_op3d; the point sums on the host in index order and in
    // long double, so that the ratios are the analytic values to an ulp and the same on every call
    const long double q[3] = {p[0], p[1], p[2]};
    long double tr[4], trb;
    for (int k = 0; k < 3; ++k) tr[k] = (long double)Nd * q[k];
    GPK_TRY(domain_trace3(h, op3, Nd, q, &tr[3]));
    GPK_TRY(boundary_trace3(h, bc3, Nb, q, &trb));
    for (int k = 0; k < 4; ++k) {
        const double r = (double)(tr[k] / ((long double)Nd + trb));   // trace(block k) / trace(block 4)
        if (host_ratios4) host_ratios4[k] = r;
        g.nug[k] = block_nugget(nugget_type, nugget, r);
    }
    g.nug[4] = block_nugget(nugget_type, nugget, 1.0);
    g.out = Theta; g.ld = ld;
    return launch_two_block(h, pairs_eligible(h, Theta, ld, Nd, Nb), g, assemble_grad3_kernel, assemble_grad3_2_kernel<0>, assemble_grad3_2_kernel<1>);
}

extern "C" int gpk_extend_functionals_grad3d(gpk_handle h, int kernel, const double* kp, const double* Xt, int Nt,
                                             const double* Xd, int Nd, const double* Xb, int Nb, const double* op3, const double* bc3,
                                             const double* coeff, int fmask, double* out, int ldo) {
    if (!h) return GPK_ERR_ARG;
    if (!out || !Xt || !coeff) return gpk_bad_arg(h, "extend_functionals_grad3d: pointers");
    if (fmask <= 0 || fmask > 1023) return gpk_bad_arg(h, "extend_functionals_grad3d: fmask must be a non-empty subset of the GPK_OP3FN_* bits");
    if (Nt <= 0) return gpk_bad_arg(h, "extend_functionals_grad3d: Nt <= 0");
    if (ldo < Nt) return gpk_bad_arg(h, "extend_functionals_grad3d: ldo < Nt");
    FnGrad3Args g;
    double p[3];
    GPK_TRY(fill_common_op3(h, "extend_functionals_grad3d: sizes/pointers", "extend_functionals_grad3d: kernel id", kernel, kp, Xd, Nd, Xb, Nb,
                            op3, bc3, p, &g.s));
    g.p1 = p[0]; g.p2 = p[1]; g.p3 = p[2];
    g.Nd = Nd; g.M = Nd + Nb;
    g.tx = Xt; g.Nt = Nt; g.coeff = coeff; g.mask = fmask; g.out = out; g.ldo = ldo;
    const int grid = gpk_ceil_div(Nt, FN_TT);
    if (fmask == 1) extend_fn_grad3_kernel<1><<<grid, 256, 0, h->stream>>>(g);          // value
    else if (fmask < 16) extend_fn_grad3_kernel<4><<<grid, 256, 0, h->stream>>>(g);     // value and gradient
    else extend_fn_grad3_kernel<NO><<<grid, 256, 0, h->stream>>>(g);                    // all ten
    GPK_LAUNCH_CHECK(h);
    return 0;
}

extern "C" int gpk_pde_residual_sl3d(gpk_handle h, const double* host_gq8, int Nt, const double* fields, int ldf, const double* psi_u,
                                     const double* rhs, double* out) {
    if (!h) return GPK_ERR_ARG;
    if (Nt <= 0) return gpk_bad_arg(h, "pde_residual_sl3d: Nt <= 0");
    if (!host_gq8 || !fields || !psi_u || !rhs || !out || ldf < Nt) return gpk_bad_arg(h, "pde_residual_sl3d: host_gq8 / fields / psi_u / rhs / out / ldf");
    Sl3Coef gq;
    for (int k = 0; k < 8; ++k) gq.c[k] = host_gq8[k];
    pde_residual_sl3d_kernel<<<gpk_ceil_div(Nt, 256), 256, 0, h->stream>>>(gq, Nt, fields, ldf, psi_u, rhs, out);
    GPK_LAUNCH_CHECK(h);
    return 0;
}
