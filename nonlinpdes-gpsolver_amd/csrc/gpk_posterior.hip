// gpk_posterior.hip -- posterior variance of the GP solution at test points, Gauss-Newton / Laplace form ("Posterior variance").
//
// No reference call site: the reference returns the posterior mean only.  With A = dF/dz at the final iterate, L L^T = Theta and
// H/2 = A^T Theta^{-1} A (the matrix gpk_gn_hessian_grad returns, halved; Darcy's data rows included),
//     var(x) = 1 - ||L^{-1} k_x||^2  +  ||L_H^{-1} A^T Theta^{-1} k_x||^2,       L_H L_H^T = H/2,
//              `---- var_cond ----'     `---------- var_gn ----------'
// where k_x is the column of gpk_assemble_cross for x.  The first term conditions on the collocation values z as if they were known;
// the second puts back their own covariance (H/2)^{-1}.
//
//   gpk_posterior_prepare    once per iterate:  P = L^{-1} A(z) (every row group with its own factor),  R = chol(P^T P)
//   gpk_posterior_variance   per batch of nt test points:  V = L_f^{-1} K,  W = R^{-1} (P_f^T V),  column sums of squares of V and W
//   gpk_posterior_covariance the same V and W kept whole:  C <- C - V^T V + W^T W on the prior block of gpk_assemble_prior (nt x nt)
//   gpk_posterior_sample     out = mean 1^T + chol(C + jitter I) Xi with the caller's standard normals Xi ("Posterior
//                            covariance and samples")
//
// H/2 is formed as P^T P with the rows that have no factor (Darcy's data misfit, 1 / gamma) kept in P: the product
// gpk_gn_hessian_grad issues on the same block, without its border column and without the factor 2.
// The dense work is the library's (gpk_i_trsm_left_dinv / gpk_i_trsm_left_mt, gpk_i_gemm, gpk_i_potrf) on the paths gpk_gn_hessian_grad
// takes; what is new here is the column reduction.  The cross-covariance evaluator gpk_assemble_cross stands with its family in
// gpk_assemble.hip.
#include "gpk_common.h"

namespace {

// ---- out[t] = (base ? base[t] : c0) + alpha * sum_r V[r, t]^2 -------------------------------------------------------------------------
// One read-only pass over V, lanes along t: a wave reads 512 contiguous bytes of a row, its 4 sister waves take the rows r, r + 1, r + 2,
// r + 3 of a stride-4 sweep, four loads in flight each.  The rows are cut into `nslab` slabs -- a function of (rows, cols) alone, sized
// for about 8 workgroups per CU of a 256-CU chip (64 KB in flight per CU; a streaming read needs ~72 KB to hide an HBM miss) -- whose
// partial sums go to a scratch array and are added in slab order by a second kernel: no atomics, a repeated call gives the same bits.
constexpr int CS_COLS = 64;
constexpr int CS_TARGET_WG = 2048;

struct Slabs { int n; int rows_per; };

Slabs col_slabs(int rows, int cols) {
    const int colblocks = gpk_ceil_div(cols, CS_COLS);
    int n = gpk_ceil_div(CS_TARGET_WG, colblocks);
    const int most = gpk_ceil_div(rows, 16);                         // at least 16 rows per slab: 4 per wave
    if (n > most) n = most;
    if (n > 256) n = 256;
    if (n < 1) n = 1;
    const int rows_per = gpk_ceil_div(rows, n);
    return {gpk_ceil_div(rows, rows_per), rows_per};
}

size_t col_scratch_bytes(int rows, int cols) { return (size_t)col_slabs(rows, cols).n * cols * sizeof(double); }

__global__ __launch_bounds__(256) void col_sumsq_partial_kernel(const double* __restrict__ V, int rows, int cols, long ldv, int rows_per,
                                                                double* __restrict__ partial) {
    __shared__ double red[4][CS_COLS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int t = blockIdx.x * CS_COLS + lane;
    const int r0 = blockIdx.y * rows_per;
    const int r1 = min(r0 + rows_per, rows);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    if (t < cols) {
        const double* const col = V + t;
        int r = r0 + w;
        for (; r + 12 < r1; r += 16) {
            const double v0 = col[(long)r * ldv], v1 = col[(long)(r + 4) * ldv], v2 = col[(long)(r + 8) * ldv], v3 = col[(long)(r + 12) * ldv];
            s0 = fma(v0, v0, s0); s1 = fma(v1, v1, s1); s2 = fma(v2, v2, s2); s3 = fma(v3, v3, s3);
        }
        for (; r < r1; r += 4) {
            const double v = col[(long)r * ldv];
            s0 = fma(v, v, s0);
        }
    }
    red[w][lane] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (w == 0 && t < cols) partial[(long)blockIdx.y * cols + t] = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
}

__global__ __launch_bounds__(256) void col_sumsq_finish_kernel(const double* __restrict__ partial, int nslab, int cols, double alpha,
                                                               const double* base, double c0, double* out) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= cols) return;
    double s = 0.0;
    for (int k = 0; k < nslab; ++k) s += partial[(long)k * cols + t];
    out[t] = (base ? base[t] : c0) + alpha * s;                      // (out may be base: one read, one write per entry)
}

// scratch: col_scratch_bytes(rows, cols) of device memory
int col_sumsq(gpk_handle h, const double* V, int rows, int cols, long ldv, double alpha, const double* base, double c0, double* out,
              double* scratch) {
    const Slabs s = col_slabs(rows, cols);
    col_sumsq_partial_kernel<<<dim3(gpk_ceil_div(cols, CS_COLS), s.n), 256, 0, h->stream>>>(V, rows, cols, ldv, s.rows_per, scratch);
    GPK_LAUNCH_CHECK(h);
    col_sumsq_finish_kernel<<<gpk_ceil_div(cols, 256), 256, 0, h->stream>>>(scratch, s.n, cols, alpha, base, c0, out);
    GPK_LAUNCH_CHECK(h);
    return 0;
}

// ---- row groups of P = L^{-1} A(z): the stacked layout of gpk_gn_build (gpk_gn.hip, gn_dims) --------------------------------------------
struct Group { const double* L; int ldl; int n; int off; const double* Dinv; };

struct Layout { int nz, rows, ngroups; Group g[3]; };

int posterior_layout(const gpk_gn_problem* p, Layout& d) {
    if (!p || p->system == GPK_GN_ELLIPTIC_RELAXED) return GPK_ERR_ARG;
    if (gpk_gn_dims(p, &d.nz, &d.rows) != 0) return GPK_ERR_ARG;
    const int Nd = p->Nd, Nb = p->Nb;
    if (p->system == GPK_GN_DARCY) {
        d.ngroups = 3;
        d.g[0] = {p->L2, p->ldl2, 3 * Nd, 0, p->Dinv2};               // field a
        d.g[1] = {p->L, p->ldl, 4 * Nd + Nb, 3 * Nd, p->Dinv};        // field u
        d.g[2] = {nullptr, 0, p->Ndata, 7 * Nd + Nb, nullptr};        // data rows: no factor
    } else {
        d.ngroups = 1;
        d.g[0] = {p->L, p->ldl, d.rows, 0, p->Dinv};
    }
    return 0;
}

const char* const RELAXED_MSG = "posterior: the relaxed elliptic system is not served";

int check_problem(gpk_handle h, const gpk_gn_problem* p, Layout& d) {
    if (!p) return gpk_bad_arg(h, "posterior: null problem");
    if (p->system == GPK_GN_ELLIPTIC_RELAXED) return gpk_bad_arg(h, RELAXED_MSG);
    if (posterior_layout(p, d) != 0) return gpk_bad_arg(h, "posterior: system id / sizes");
    if (!p->rhs_f || (p->Nb > 0 && !p->bdy_g) || !p->L) return gpk_bad_arg(h, "posterior: null rhs_f/bdy_g/L");
    if (p->system == GPK_GN_DARCY && (!p->L2 || (p->Ndata > 0 && !p->data_u))) return gpk_bad_arg(h, "posterior: Darcy needs L2 and data_u");
    return 0;
}

// the GEMM-only solve runs for a group when the handle allows it and the problem carries that factor's inverted diagonal blocks
bool use_dinv(gpk_handle h, const gpk_gn_problem* p, const Group& g) { return h->tune.use_dinv && p->dinv_block > 0 && g.Dinv; }

bool dinv_block_valid(int db) { return db == 256 || db == 512 || db == 1024 || db == 2048; }

int pad16(int n) { return ((n + 15) / 16) * 16; }

// What the two calls ask of the handle's workspace -- the one place that knows, shared with gpk_posterior_worksize.
// prepare: [A(z) | F(z)] in front of the out-of-place GEMM-only solve (nothing on the substitution path)
size_t prepare_ws_bytes(int rows, int ldp, bool dinv) { return dinv ? (size_t)rows * ldp * sizeof(double) : 0; }
// variance: the out-of-place V of the GEMM-only solve (nf x ldk), then the partial sums of the larger of the two reductions
size_t variance_v_bytes(int nf, int ldk, bool dinv) { return dinv ? (size_t)nf * ldk * sizeof(double) : 0; }
size_t variance_red_bytes(int nf, int nz, int nt) {
    const size_t a = col_scratch_bytes(nf, nt), b = col_scratch_bytes(nz, nt);
    return a > b ? a : b;
}

// ---- the two kernels of gpk_posterior_sample -----------------------------------------------------------------------------------------------
// C[i][i] += jitter: one lane per diagonal entry (stride ldc + 1)
__global__ __launch_bounds__(256) void diag_shift_kernel(double* __restrict__ C, int n, long ldc, double jitter) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) C[(long)i * (ldc + 1)] += jitter;
}

// out[t][s] = mean[t]: a lane owns two adjacent columns of one row -- one 16-byte store when WIDE (base 16-byte aligned, ldo and ns even),
// the same values as 8-byte stores otherwise.  npair = ceil(ns / 2) lanes per row.
template <bool WIDE>
__global__ __launch_bounds__(256) void bcast_rows_kernel(const double* __restrict__ mean, int nt, int ns, int npair, double* __restrict__ out,
                                                         long ldo) {
    typedef double d2 __attribute__((ext_vector_type(2)));
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)nt * npair) return;
    const int t = (int)(idx / npair), s = 2 * (int)(idx % npair);
    const double m = mean[t];
    double* const dst = out + (long)t * ldo + s;
    if constexpr (WIDE) *reinterpret_cast<d2*>(dst) = (d2){m, m};
    else { dst[0] = m; if (s + 1 < ns) dst[1] = m; }
}

}  // namespace

// the same reduction for the trial losses of the line search (gpk_gn.hip): the caller's scratch, the handle's workspace is not touched
size_t gpk_i_col_sumsq_scratch_bytes(int rows, int cols) { return col_scratch_bytes(rows, cols); }
int gpk_i_col_sumsq(gpk_handle h, const double* V, int rows, int cols, int ldv, double* out, double* scratch) {
    return col_sumsq(h, V, rows, cols, ldv, 1.0, nullptr, 0.0, out, scratch);
}

extern "C" int gpk_col_sumsq(gpk_handle h, const double* V, int rows, int cols, int ldv, double alpha, const double* base, double* out) {
    if (!h) return GPK_ERR_ARG;
    if (!V || !out) return gpk_bad_arg(h, "col_sumsq: pointers");
    if (rows <= 0 || cols <= 0) return gpk_bad_arg(h, "col_sumsq: rows / cols <= 0");
    if (ldv < cols) return gpk_bad_arg(h, "col_sumsq: ldv < cols");
    double* scratch = nullptr;
    GPK_TRY(gpk_i_workspace(h, col_scratch_bytes(rows, cols), &scratch));
    h->work_sig[0] = -1;                                             // the workspace no longer holds the zero region of a solve
    return col_sumsq(h, V, rows, cols, ldv, alpha, base, 0.0, out, scratch);
}

extern "C" int gpk_posterior_worksize(const gpk_gn_problem* p, int nt, int ldp, int ldr, int ldk, int* host_ldp, int* host_ldr,
                                      int* host_ldk, size_t* P_bytes, size_t* R_bytes, size_t* K_bytes, size_t* W_bytes,
                                      size_t* handle_bytes) {
    Layout d;
    if (posterior_layout(p, d) != 0 || nt <= 0) return GPK_ERR_ARG;
    if (ldp == 0) ldp = pad16(d.nz + 1);
    if (ldr == 0) ldr = pad16(d.nz);
    if (ldk == 0) ldk = pad16(nt);
    if (ldp < d.nz + 1 || ldr < d.nz || ldk < nt) return GPK_ERR_ARG;
    // as the two calls decide it (with the handle's default gpk_tune(10, 1); with the substitution schedule forced they ask for less):
    // prepare solves through the inverted diagonal blocks when EVERY factor has them, variance when the field's factor has them
    int nf = 0;                                                      // rows of the largest field
    bool all_dinv = p->dinv_block > 0;
    size_t var = 0;
    for (int k = 0; k < d.ngroups; ++k) {
        const Group& g = d.g[k];
        if (!g.L) continue;
        nf = g.n > nf ? g.n : nf;
        if (!g.Dinv) all_dinv = false;
        const size_t v = variance_v_bytes(g.n, ldk, p->dinv_block > 0 && g.Dinv) + variance_red_bytes(g.n, d.nz, nt);
        var = v > var ? v : var;
    }
    if (host_ldp) *host_ldp = ldp;
    if (host_ldr) *host_ldr = ldr;
    if (host_ldk) *host_ldk = ldk;
    if (P_bytes) *P_bytes = (size_t)d.rows * ldp * sizeof(double);
    if (R_bytes) *R_bytes = (size_t)d.nz * ldr * sizeof(double);
    if (K_bytes) *K_bytes = (size_t)nf * ldk * sizeof(double);
    if (W_bytes) *W_bytes = (size_t)d.nz * ldk * sizeof(double);
    if (handle_bytes) {
        const size_t prep = prepare_ws_bytes(d.rows, ldp, all_dinv);
        *handle_bytes = var > prep ? var : prep;
    }
    return 0;
}

extern "C" int gpk_posterior_prepare(gpk_handle h, const gpk_gn_problem* p, const double* z, double* P, int ldp, double* R, int ldr,
                                     int* host_info) {
    if (!h) return GPK_ERR_ARG;
    Layout d;
    GPK_TRY(check_problem(h, p, d));
    if (!z || !P || !R) return gpk_bad_arg(h, "posterior_prepare: null z / P / R");
    if (ldp < d.nz + 1) return gpk_bad_arg(h, "posterior_prepare: ldp < nz + 1");
    if (ldr < d.nz) return gpk_bad_arg(h, "posterior_prepare: ldr < nz");
    bool dinv = true;
    for (int k = 0; k < d.ngroups; ++k) if (d.g[k].L && !use_dinv(h, p, d.g[k])) dinv = false;
    if (dinv && !dinv_block_valid(p->dinv_block)) return gpk_bad_arg(h, "posterior_prepare: dinv_block must be 256, 512, 1024 or 2048");
    if (dinv) {
        // out of place, as the solve of gpk_gn_hessian_grad: [A(z) | F(z)] into the handle's workspace, L^{-1} A(z) into P
        double* B = nullptr;
        GPK_TRY(gpk_i_workspace(h, prepare_ws_bytes(d.rows, ldp, true), &B));
        h->work_sig[0] = -1;
        GPK_TRY(gpk_gn_build(h, p, z, B, ldp));
        for (int k = 0; k < d.ngroups; ++k) {
            const Group& g = d.g[k];
            if (g.n <= 0) continue;
            if (g.L) GPK_TRY(gpk_i_trsm_left_dinv(h, g.L, g.Dinv, p->dinv_block, g.n, g.ldl, B + (long)g.off * ldp, ldp, P + (long)g.off * ldp, ldp, d.nz, GpkLz()));
            else GPK_HIP(h, hipMemcpy2DAsync(P + (long)g.off * ldp, (size_t)ldp * 8, B + (long)g.off * ldp, (size_t)ldp * 8, (size_t)d.nz * 8, g.n,
                                             hipMemcpyDeviceToDevice, h->stream));
        }
    } else {
        GPK_TRY(gpk_gn_build(h, p, z, P, ldp));                      // (column nz receives F(z): scratch)
        for (int k = 0; k < d.ngroups; ++k) {
            const Group& g = d.g[k];
            if (g.L && g.n > 0) GPK_TRY(gpk_i_trsm_left_mt(h, false, g.L, g.n, g.ldl, P + (long)g.off * ldp, d.nz, ldp));
        }
    }
    GPK_TRY(gpk_i_gemm(h, true, false, d.nz, d.nz, d.rows, 1.0, P, ldp, P, ldp, 0.0, R, ldr, true));
    GPK_HIP(h, hipMemsetAsync(h->d_info, 0, sizeof(int), h->stream));
    GPK_TRY(gpk_i_potrf(h, R, d.nz, ldr, 0));
    if (host_info) {
        GPK_HIP(h, hipMemcpyAsync(host_info, h->d_info, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        GPK_HIP(h, hipStreamSynchronize(h->stream));
    }
    return 0;
}

extern "C" int gpk_posterior_variance(gpk_handle h, const gpk_gn_problem* p, const double* P, int ldp, const double* R, int ldr, int field,
                                      double* K, int ldk, int nt, double* W, int ldw, double* var_cond, double* var) {
    if (!h) return GPK_ERR_ARG;
    Layout d;
    GPK_TRY(check_problem(h, p, d));
    if (field != 0 && field != 1) return gpk_bad_arg(h, "posterior_variance: field must be 0 (u) or 1 (a)");
    if (field == 1 && p->system != GPK_GN_DARCY) return gpk_bad_arg(h, "posterior_variance: field 1 (a) exists for GPK_GN_DARCY only");
    if (nt <= 0) return gpk_bad_arg(h, "posterior_variance: nt <= 0");
    if (!K || ldk < nt) return gpk_bad_arg(h, "posterior_variance: K / ldk < nt");
    if (var && (!P || !R || !W)) return gpk_bad_arg(h, "posterior_variance: var needs P, R and W");
    if (var && (ldp < d.nz || ldr < d.nz || ldw < nt)) return gpk_bad_arg(h, "posterior_variance: ldp / ldr < nz or ldw < nt");
    const Group& g = d.g[p->system == GPK_GN_DARCY ? 1 - field : 0];
    const bool dinv = use_dinv(h, p, g);
    if (dinv && !dinv_block_valid(p->dinv_block)) return gpk_bad_arg(h, "posterior_variance: dinv_block must be 256, 512, 1024 or 2048");
    const size_t red = variance_red_bytes(g.n, d.nz, nt), vbytes = variance_v_bytes(g.n, ldk, dinv);
    double* ws = nullptr;
    GPK_TRY(gpk_i_workspace(h, vbytes + red, &ws));
    h->work_sig[0] = -1;
    double* const scratch = ws + vbytes / sizeof(double);
    // 1. V = L_f^{-1} K
    const double* V = K;
    if (dinv) {
        GPK_TRY(gpk_i_trsm_left_dinv(h, g.L, g.Dinv, p->dinv_block, g.n, g.ldl, K, ldk, ws, ldk, nt, GpkLz()));
        V = ws;
    } else {
        GPK_TRY(gpk_trsm(h, 0, g.L, g.n, g.ldl, K, nt, ldk));
    }
    // 2. var_cond = 1 - colsumsq(V)   (into var when only var is asked for: step 5 then adds in place)
    double* const cond = var_cond ? var_cond : var;
    if (cond) GPK_TRY(col_sumsq(h, V, g.n, nt, ldk, -1.0, nullptr, 1.0, cond, scratch));
    if (!var) return 0;
    // 3. W = P_f^T V    4. W <- R^{-1} W    5. var = var_cond + colsumsq(W)
    GPK_TRY(gpk_i_gemm(h, true, false, d.nz, nt, g.n, 1.0, P + (long)g.off * ldp, ldp, V, ldk, 0.0, W, ldw, false));
    GPK_TRY(gpk_trsm(h, 0, R, d.nz, ldr, W, nt, ldw));
    return col_sumsq(h, W, d.nz, nt, ldw, 1.0, cond, 0.0, var, scratch);
}

// C <- C - V^T V (+ W^T W): the products of gpk_posterior_variance kept whole instead of reduced to their column sums of squares.  V and
// W are formed by the very calls of gpk_posterior_variance; the two products are the routine under gpk_syrk (lower triangle, beta = 1)
// and ONE gpk_symmetrize_lower at the end copies the finished lower triangle up, so C[s][t] and C[t][s] are the same bits.
extern "C" int gpk_posterior_covariance(gpk_handle h, const gpk_gn_problem* p, const double* P, int ldp, const double* R, int ldr, int field,
                                        double* K, int ldk, int nt, double* W, int ldw, double* C, int ldc, int with_gn) {
    if (!h) return GPK_ERR_ARG;
    Layout d;
    GPK_TRY(check_problem(h, p, d));
    if (field != 0 && field != 1) return gpk_bad_arg(h, "posterior_covariance: field must be 0 (u) or 1 (a)");
    if (field == 1 && p->system != GPK_GN_DARCY) return gpk_bad_arg(h, "posterior_covariance: field 1 (a) exists for GPK_GN_DARCY only");
    if (nt <= 0) return gpk_bad_arg(h, "posterior_covariance: nt <= 0");
    if (!K || ldk < nt) return gpk_bad_arg(h, "posterior_covariance: K / ldk < nt");
    if (!C || ldc < nt) return gpk_bad_arg(h, "posterior_covariance: C / ldc < nt");
    if (with_gn && (!P || !R || !W)) return gpk_bad_arg(h, "posterior_covariance: with_gn needs P, R and W");
    if (with_gn && (ldp < d.nz || ldr < d.nz || ldw < nt)) return gpk_bad_arg(h, "posterior_covariance: ldp / ldr < nz or ldw < nt");
    const Group& g = d.g[p->system == GPK_GN_DARCY ? 1 - field : 0];
    const bool dinv = use_dinv(h, p, g);
    if (dinv && !dinv_block_valid(p->dinv_block)) return gpk_bad_arg(h, "posterior_covariance: dinv_block must be 256, 512, 1024 or 2048");
    double* ws = nullptr;
    GPK_TRY(gpk_i_workspace(h, variance_v_bytes(g.n, ldk, dinv), &ws));   // (no reduction scratch: within gpk_posterior_worksize's figure)
    h->work_sig[0] = -1;
    // 1. V = L_f^{-1} K
    const double* V = K;
    if (dinv) {
        GPK_TRY(gpk_i_trsm_left_dinv(h, g.L, g.Dinv, p->dinv_block, g.n, g.ldl, K, ldk, ws, ldk, nt, GpkLz()));
        V = ws;
    } else {
        GPK_TRY(gpk_trsm(h, 0, g.L, g.n, g.ldl, K, nt, ldk));
    }
    // 2. C <- C - V^T V (lower)
    GPK_TRY(gpk_i_gemm(h, true, false, nt, nt, g.n, -1.0, V, ldk, V, ldk, 1.0, C, ldc, true));
    if (with_gn) {
        // 3. W = P_f^T V    4. W <- R^{-1} W    5. C <- C + W^T W (lower)
        GPK_TRY(gpk_i_gemm(h, true, false, d.nz, nt, g.n, 1.0, P + (long)g.off * ldp, ldp, V, ldk, 0.0, W, ldw, false));
        GPK_TRY(gpk_trsm(h, 0, R, d.nz, ldr, W, nt, ldw));
        GPK_TRY(gpk_i_gemm(h, true, false, nt, nt, d.nz, 1.0, W, ldw, W, ldw, 1.0, C, ldc, true));
    }
    return gpk_symmetrize_lower(h, C, nt, ldc);
}

// out = mean 1^T + chol(C + jitter I) Xi.  The normals are the caller's: nothing is drawn here, so a sample is a function of its inputs.
// The pivot status is read back (one synchronisation) before anything is written to out: a failed factorisation leaves out untouched.
extern "C" int gpk_posterior_sample(gpk_handle h, double* C, int ldc, int nt, double jitter, const double* mean, const double* Xi, int ldxi,
                                    int ns, double* out, int ldo, int* host_info) {
    if (!h) return GPK_ERR_ARG;
    if (nt <= 0 || ns <= 0) return gpk_bad_arg(h, "posterior_sample: nt / ns <= 0");
    if (!C || ldc < nt) return gpk_bad_arg(h, "posterior_sample: C / ldc < nt");
    if (!mean || !Xi || !out) return gpk_bad_arg(h, "posterior_sample: null mean / Xi / out");
    if (ldxi < ns || ldo < ns) return gpk_bad_arg(h, "posterior_sample: ldxi / ldo < ns");
    if (!(jitter >= 0.0)) return gpk_bad_arg(h, "posterior_sample: jitter must be >= 0");
    diag_shift_kernel<<<gpk_ceil_div(nt, 256), 256, 0, h->stream>>>(C, nt, ldc, jitter);
    GPK_LAUNCH_CHECK(h);
    GPK_HIP(h, hipMemsetAsync(h->d_info, 0, sizeof(int), h->stream));
    GPK_TRY(gpk_i_potrf(h, C, nt, ldc, 0));
    GPK_TRY(gpk_tril(h, C, nt, ldc));
    int info = 0;
    GPK_HIP(h, hipMemcpyAsync(&info, h->d_info, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    GPK_HIP(h, hipStreamSynchronize(h->stream));
    if (host_info) *host_info = info;
    if (info != 0) return 0;
    const int npair = gpk_ceil_div(ns, 2);
    const long lanes = (long)nt * npair;
    const int grid = (int)((lanes + 255) / 256);
    if ((ldo % 2 == 0) && (ns % 2 == 0) && (((uintptr_t)out & 15) == 0)) bcast_rows_kernel<true><<<grid, 256, 0, h->stream>>>(mean, nt, ns, npair, out, ldo);
    else bcast_rows_kernel<false><<<grid, 256, 0, h->stream>>>(mean, nt, ns, npair, out, ldo);
    GPK_LAUNCH_CHECK(h);
    return gpk_i_gemm(h, false, false, nt, ns, nt, 1.0, C, ldc, Xi, ldxi, 1.0, out, ldo, false);
}
