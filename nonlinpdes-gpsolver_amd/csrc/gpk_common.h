// gpk_common.h -- internal declarations shared by the libgpk translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/gpk.h"
#include "../../include/gpk_debug.h"
#ifdef GPK_DEV
#include "../../include/gpk_dev.h"
#endif
#include "../../include/gpk_mg.h"

#define GPK_ERR_ARG (-9001)
#define GPK_ERR_NODEV (-9002)

constexpr int GPK_MAX_TRSV_BLOCKS = 4096;
constexpr int GPK_SCALARS_EVIDENCE = 16;         // first of the 6 slots of gpk_ctx::d_scalars that gpk_evidence.hip owns

// Piecewise-linear leading-zero profile ("staircase") of a block of right-hand sides: column c (storage order) is known to be zero
// above row first_row(c).  Segment s covers the columns [c1[s-1], c1[s]) (c1[-1] = 0) with first_row(c) = a[s] + (b[s] - c) / sd[s]
// (b[s] >= every c of the segment; sd huge = a flat step); columns from c1[nseg-1] on are dense.  The elliptic, Eikonal and Burgers
// systems have ONE segment and keep the closed form of GpkLz (below); the Darcy system's u-part has three (round 4):
// slope 1 over the v1, v2 columns, flat over w1, w2, slope 1 over w0, v0 (gpk_gn.hip).  nseg = 0: no profile.
struct GpkStair {
    int nseg = 0;
    int c1[4] = {0, 0, 0, 0};
    int a[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0}, sd[4] = {1, 1, 1, 1};
};
// smallest first_row over the columns [n0, n1) -- the row from which a tile with those columns has to start its K loop
__host__ __device__ inline int gpk_stair_min(const GpkStair& st, int n0, int n1) {
    int best = 0x7fffffff, lo = 0;
    for (int s = 0; s < st.nseg; ++s) {
        const int hi = st.c1[s];
        const int x0 = n0 > lo ? n0 : lo, x1 = n1 < hi ? n1 : hi;    // overlap of the tile with the segment
        if (x1 > x0) {                                               // non-increasing inside a segment: the right-most column decides
            const int d = st.b[s] - (x1 - 1);
            const int v = st.a[s] + (d > 0 ? d / st.sd[s] : 0);
            best = v < best ? v : best;
        }
        lo = hi;
    }
    if (n1 > lo) best = 0;                                           // dense columns behind the last segment
    return best == 0x7fffffff ? 0 : best;
}
// first column that can be non-zero in the rows [0, rows_end): the smallest c with first_row(c) < rows_end (profiles used by the
// triangular solve are non-increasing in c); ncols if there is none
inline int gpk_stair_first_col(const GpkStair& st, int rows_end, int ncols) {
    int lo = 0, hi = ncols;                                          // invariant: first_row(c) >= rows_end for c < lo, < rows_end for c >= hi
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (gpk_stair_min(st, mid, mid + 1) < rows_end) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// The leading-zero profile of a block of right-hand sides (the operand B of a product, stored [k][n]) as a VALUE: every building block that
// exploits leading zeros takes one as an argument, and nothing keeps one on the handle.  It is one of three things, and says which:
//   dense      (the default)     nothing is known to be zero;
//   closed     lead > 0          column c < lead is zero above row (lead - 1 - c) / div, columns >= lead are dense (div 1: the elliptic systems
//                                and the conservative Eikonal form; 3: Burgers);
//   piecewise  pw.nseg > 0       a GpkStair in whose frame the block's column 0 is column col0 and its row 0 is row row0 (Eikonal, Darcy u-part).
// sub() is the same profile seen from a sub-block; the closed form folds the offsets into `lead`, so col0 / row0 stay 0 there.
struct GpkLz {
    int lead = 0, div = 1;
    GpkStair pw;
    int col0 = 0, row0 = 0;
    static GpkLz closed(int lead, int div = 1) {
        GpkLz z;
        if (lead > 0) { z.lead = lead; z.div = div > 0 ? div : 1; }
        return z;
    }
    static GpkLz piecewise(const GpkStair& st) { GpkLz z; z.pw = st; return z; }
    bool is_piecewise() const { return pw.nseg > 0; }
    bool is_dense() const { return lead <= 0 && pw.nseg == 0; }
    // first row of the block's column c that can be non-zero
    int first_row(int c) const {
        if (is_piecewise()) { const int r = gpk_stair_min(pw, col0 + c, col0 + c + 1) - row0; return r > 0 ? r : 0; }
        return c < lead ? (lead - 1 - c) / div : 0;
    }
    // the block's rows [0, rows_end) are zero left of this column (of its ncols columns; the closed form is not clamped: <= 0 = none)
    int first_col(int rows_end, int ncols) const {
        if (is_piecewise()) return gpk_stair_first_col(pw, row0 + rows_end, col0 + ncols) - col0;
        return lead - div * rows_end;
    }
    // the profile of the sub-block that starts dc columns to the right and dr rows below (dense once no column of a staircase is left)
    GpkLz sub(int dc, int dr) const {
        if (is_piecewise()) {
            GpkLz z = *this;
            z.col0 += dc; z.row0 += dr;
            return z.col0 < pw.c1[pw.nseg - 1] ? z : GpkLz();
        }
        return closed(lead - dc - div * dr, div);
    }
};

// Development / tuning switches of ONE handle (round 4: they used to be process-wide globals).  Defaults are the measured choices;
// gpk_tune(handle, key, value) (include/gpk_debug.h) changes one -- tests force every kernel variant through it, A/B measurements
// flip one switch at a time.  The product path never calls gpk_tune.  "key N" = the key of gpk_tune.
struct GpkTune {
    int asm_pairs = 1;                  // key 47: 0 = one column point per lane (8-byte stores) always
    int seq_left_looking = 0;           // key 56: 1 = left-looking rank-64 work inside the 512-blocks of the one-stream Cholesky (experiment, round 6; with key 48 = 2)
    int asm_nt = 0;                     // key 55: 1 = non-temporal 16-byte stores in the two-point evaluator (round 6 A/B, tools/assembly_store_ab.py)
    int dbg = 0;                        // 
    int mt_trsm = 0;                    // key 2: 
    int persistent_ob = 0;              // key 7: 1 = persistent outer-block kernel (slower, see its header)
    int left_looking_panels = 1;        // key 18: 0 = right-looking rank-64 updates also in the pipelined chain
    int panel_mfma = 1;                 // key 21: 0 = first-design panel kernel (potf2_tile: two columns per barrier)
    int panel_unrolled = 1;             // key 41: 0 = the rolled instantiation of the panel kernel
    int fused_panel = 1;                // key 5: 0 = potf2 + trsm launches
    int panel_fused = 1;                // key 48: 0 = rank-64 updates as launches of their own between the panel kernels (round 2)
    int strip = 1;                      // key 3: 0 = 64-row base solves only
    int solve_splitk = 0;               // key 30: largest split-K factor tried for the updates of the inverted-block solve (0 = off)
    int potrf_pipeline_min_n = 2048;    // key 19: plain Cholesky pipelined for orders in [min, max] (max = 0: off, see gpk_i_potrf)
    int potrf_pipeline_max_n = 0;       // key 20: plain Cholesky pipelined for orders in [min, max] (max = 0: off, see gpk_i_potrf)
    int potrf_lookahead = 0;            // key 54 (development build only): 1 = the two-partition plain Cholesky (orders of keys 19 / 20) in its right-looking look-ahead form (round 5: measured, not adopted) instead of the left-looking pipeline
    int potrf_ob = 512;                 // key 51: outer block width of the right-looking factorisation (multiple of 64)
    int pipeline = 1;                   // key 12: 0 = SYRK, then right-looking Cholesky, on one stream
    int pipeline_chain_cus = 32;        // key 13: CUs of the chain partition (rounded to a multiple of 32)
    int pipeline_pre = 1;               // key 17: blocks of the product computed before the fork
    int pipeline_tile = 64;             // key 34: 64 / 128 = tile height of the pipeline's products (parallelism from split-K alone), 0 = automatic (32 rows below 512 tiles).  Phase time at config 2: automatic 3.18-3.23 ms, 64 rows 3.12-3.14, 128 rows 3.47
    int pipeline_lookahead = 0;         // key 26: 0 = block j's update with block j-1 as ONE product after the chain of j-1
    int pipeline_units = 1000;          // key 24: workgroups aimed at per product launch of the pipeline (split-K; 0 = no split).  Measured at config 2, phase time: 0 / 1000 / 1500 / 2000 / 3000 -> 3.85 / 3.57 / 3.58 / 3.60 / 3.62 ms
    int pipeline_max_n = 7000;          // key 14: pipelined only up to this order (with the split-K products, product + factorisation per step: order 6001 7.18 -> 6.50 ms, 7001 13.7 -> 13.6, 8501 22.3 -> 23.3, 10001 35.8 -> 38.6)
    int pipeline_w0 = 512;              // key 28: 
    int pipeline_ob = 512;              // key 29: 
    int probe_chain_cus = 0;            // key 11: overlap probe with a CU-mask partition
    int fused_trsv = 1;                 // key 4: 0 = two launches per block, 1 = fused with data-tagged hand-offs (round 3), 2 = fused with flags (round 1)
    int gemm_extra_lds = 0;             // key 9: bytes of dynamic LDS requested on top (occupancy throttle for overlap experiments)
    int k64_small = 1;                  // key 8: 0 = 64-row tiles only in the K <= 64 kernel
    int band_mb = 192;                  // key 35: MB of A per band of a tall leading-zero launch (0 = no bands).  North-star size, solve phase: no bands 45.2 ms, 48 MB 44.9, 96 MB 43.2, 192 MB 42.6-43.1, 288 MB 43.9, 400 MB 45.4
    int syrk_band = 256;                // key 36: MB of S per band of a large leading-zero SYRK launch (0 = column-major over all rows).  North-star size, the product S^T S: no bands 24.15 ms, 192 MB 23.4, 256 MB 22.9, 384 MB 23.55, 512 MB 24.3
    int big_min = 6000;                 // key 38: launches with at least this many 64 x 64 tiles use the 128 x 128 tile with 16 waves, one workgroup per CU (0 = never).  tools/gemm_big_probe.py, 64 x 64 -> 128 x 64 -> this: NN 10500^3 60.0 / 58.6 / 65.2 TF/s, 8192^3 62.2 / 60.9 / 69.1 on a slow box; north-star solve phase 44.6 -> 43.7 ms with thresholds 3000 .. 6000; at config 2 (threshold 2000) the solve phase loses 5 %
    int big_lower_min = 8000;           // key 50: lower-triangular leading-zero launches (S^T S) with at least this many lower 64 x 64 tiles use the 128 x 128 / 16-wave tile (0 = never)
    int tall_min = 1500;                // key 33: launches with at least this many 64 x 64 tiles use the 128 x 64 / 8-wave tile (0 = never).  Measured (tools/gemm_big_probe.py, 64 x 64 -> 128 x 64): NN 10500^3 64.5 -> 67.9 TF/s, TN 4001^2 x 8400 61.3 -> 66.4, NN 2048 x 16001 x 2048 61.2 -> 65.0, 8192^3 68.6 -> 69.2; in the solve phase at config 2 the 1568-tile update 397 -> 352 us, the 3276-tile one -2 %, the 1260-tile one +10 % (hence the threshold); north-star size: solve 46.0 -> 44.7 ms
    int force_splitk = 0;               // key 25: split K of every eligible gpk_gemm launch into this many chunks (tests)
    int rev_k = 0;                      // key 16: 
    int stagger = 0;                    // key 15: start-time stagger of co-resident GEMM workgroups (experiment)
    int supertile = 0;                  // key 6: 1 = supertile schedule for the leading-zero SYRK (below)
    int sk = 1;                         // key 42: 0 = never, 1 = automatic, 2 = every eligible launch
    int sk_rounds = 6;                  // key 43: automatic mode uses tile lists for launches of fewer than this many rounds of resident workgroups
    int sk_stagger = 2;                 // key 45: start stagger of the co-resident workgroups of a tile-list launch (slot x this x 512 cycles; every workgroup starts at once and has the same amount of work -- without it the four workgroups of a CU run in lock-step, see the kernel)
    int sk_rowclass = 1;                // key 46: 0 = keep the launch's tile order when cutting shares (experiment)
    int row_order = 0;                  // key 49: 1 = row-major, per-XCD-contiguous tile order for the narrow leading-zero products of the pipelined phase (experiment, round 3: fewer re-reads of S by construction, but slower -- sum of the product launches 2.14 -> 2.31 ms, phase 3.20 -> 3.39 ms at config 2, tools/row_order_ab.sh: longest-column-first matters more than the traffic)
    int sk_snap = 4;                    // key 44: a share boundary closer than this many slabs to a tile boundary moves there
    int force_cfg = 0;                  // key 0: development aid (): 0 auto, 1 = 128x128 tiles, 2 = 64x64 tiles
    int use_dinv = 1;                   // key 10: 0 = substitution strips even when the inverses are supplied
    int eikonal_lz = 1;                 // key 23: 0 = dense schedule for the Eikonal, Burgers and Darcy systems; 2 = leading-zero layout with the conservative closed-form staircase for Eikonal (round 2-3) instead of the exact two-segment profile
    int exact_loss = 1;                 // key 52: 1 = gpk_gn_step reports the loss of the iterate it starts from by TRUE SUBSTITUTION (round 5): F(z) is written at the start of the
                                        // step and solved with the factor(s) as a single vector on the GEMM partition's stream next to the END of the step (last panel chain of the
                                        // pipelined phase on the other partition, then the backward solve of the tail on the main stream -- latency chains on an idle chip);
                                        // 2 = the same chain on the main stream in front of the solve phase (+0.43 ms at config 2, what a gpk_gn_loss call costs);
                                        // 0 = the squared norm of the F column of the GEMM-only solve (free, ~1e-8 relative error at nugget <= 1e-12 near convergence; rounds 2-4).
                                        // Measured and lost: the chain next to the SOLVE phase -- on the 32-CU chain partition beside whole-chip GEMM launches the solve grows by
                                        // 0.67 ms, with the first solve launches moved to the 224-CU partition meanwhile by 0.63 ms (the chain alone takes 0.93 ms on 32 CUs)
    int structured = 1;                 // key 40: 0 = ignore everything prepared (always the triangular solve); non-zero = honour what has been prepared: W1/W2/v0, and the Gram level whenever G is set as well
};

struct gpk_ctx {
    GpkTune tune;                   // development / tuning switches of this handle (gpk_tune)
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int* d_info = nullptr;          // device int: first non-positive pivot (1-based), 0 = none
    double* d_scalars = nullptr;    // small device scratch for reductions (64 doubles).  Slots: [0] in-step loss / border pivot, [1] gpk_gn_loss,
                                    // [2..3] gpk_error_metrics, [8] exact in-step loss (and the development micro-benchmarks), [9] pred = |y|^2 of gpk_gn_direction,
                                    // [10] accepted t, [11] accepted index (int) and [32 .. 47] the trial losses of gpk_gn_step_ls,
                                    // [GPK_SCALARS_EVIDENCE .. + 5] the (log-determinant, bad-pivot count) pairs of gpk_evidence.hip
    double* h_pinned = nullptr;     // 32 doubles of pinned host memory: where the end-of-step scalars (loss, pivot status) land -- a copy into
                                    // pageable memory goes through a staging buffer and a second synchronisation.  The line search
                                    // (gpk_gn.hip) adds [2] pred, [3] accepted index (int), [4] accepted t, [8 .. 23] the trial losses
    int* d_flags = nullptr;         // per-block "solved" epochs of the fused single-vector triangular solve (GPK_MAX_TRSV_BLOCKS ints)
    int trsv_epoch = 0;
    void* d_trsv_gran = nullptr;    // {value, epoch} granules of the fused triangular solve with data-tagged hand-offs (64 per block), allocated on first use
    long long trsv_gran_epoch = 0;
    double* d_loss_work = nullptr;  // F(z) as one contiguous vector for the exact in-step loss (rows doubles, grown on demand)
    size_t loss_work_cap = 0;       // doubles
    // the exact in-step loss runs its chain on the GEMM partition's stream NEXT TO the end of the step (the last panel chain of the pipelined
    // phase on the chain partition -- disjoint CUs -- and the backward single-vector solve of the tail on the main stream: latency chains on an
    // otherwise idle chip): a second granule set for that concurrent solve, and the events main -> side (F(z) is built; side may start) and
    // side -> main (the scalar is there)
    void* d_trsv_gran2 = nullptr;
    long long trsv_gran2_epoch = 0;
    int trsv_alt = 0;
    hipEvent_t ev_loss[2] = {nullptr, nullptr};
    int* d_obflags = nullptr;       // 64 flags of the persistent outer-block Cholesky kernel (epoch-tagged)
    int ob_epoch = 0;
    unsigned panel_loaded = 0;      // running total of "diagonal block loaded" tickets issued to the Cholesky panel kernel (d_flags[GPK_MAX_TRSV_BLOCKS])
    double* d_work = nullptr;       // scratch of the Gauss-Newton step: the out-of-place solution of the Dinv solve
    size_t work_cap = 0;            // bytes
    long work_sig[5] = {0, 0, 0, 0, 0};   // (rows, ld, nrhs, lead, system) of the last solve into d_work: its never-written
                                    // zero region is still valid when the next solve has the same shape
    // SYRK/Cholesky pipeline of the Gauss-Newton step (gpk_i_syrk_potrf): two streams with disjoint CU masks -- the GEMM stream
    // and the "chain" stream that runs the latency-bound panel kernels -- and the events that order them
    hipStream_t pipe_g = nullptr, pipe_c = nullptr;
    int pipe_chain_cus = 0;
    bool pipe_unavailable = false;          // creating the CU-masked streams failed once: this handle stays on the one-stream schedule
    std::vector<hipEvent_t> pipe_ev;        // ordering events (timing disabled)
    std::vector<hipEvent_t> pipe_tev;       // timing events around the SYRK launches (only while prof is on)
    int pipe_tev_used = 0;
    double prof_syrk_ms = 0;                // accumulated duration of the SYRK launches on the GEMM stream (pipelined mode)
    int prof_pipelined = 0;
    // split-K GEMM launches (gpk_gemm.hip, GemmArgs::splitk; the caller asks for them with the `splitk` argument of gpk_i_gemm): the
    // partial-sum workspace and the per-tile arrival counters.  One workspace: only one stream at a time may issue launches that use it
    double* d_splitk_ws = nullptr;
    size_t splitk_ws_cap = 0;       // bytes
    unsigned* d_splitk_cnt = nullptr;
    int splitk_cnt_cap = 0;         // counters
    void* sk_cache = nullptr;       // tile-list ("stream-K") plans of the GEMM launches, by launch shape (gpk_gemm.hip)
    bool ws_owner = true;           // launches on `stream` may use tile lists (their partial-sum workspace and counters are the split-K ones: one
                                    // stream of a handle at a time).  Written by GpkStreamScope only, together with `stream`
    double* d_pts = nullptr;        // packed collocation points (SoA), grown on demand
    size_t pts_cap = 0;
    int num_cu = 256;
#ifdef GPK_DEV
    GpkLz debug_profile;            // development build only: the profile last given to gpk_debug_set_profile (`lead` not set).  Read by the
                                    // extern "C" wrappers alone (gpk_debug_lz), never by a gpk_i_* function
#endif
    hipStream_t side[3] = {nullptr, nullptr, nullptr};   // column-group streams of the multi-RHS triangular solve
    hipEvent_t ev_fork = nullptr, ev_join[3] = {nullptr, nullptr, nullptr};
    // per-phase HIP-event timing of gpk_gn_step (bench.py roofline): 0 TRSM, 1 SYRK launch, 2 POTRF, 3 TRSV+update
    bool prof = false;
    hipEvent_t pev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    double prof_ms[4] = {0, 0, 0, 0};
    int prof_cnt = 0;
    hipEvent_t asm_ev[2] = {nullptr, nullptr};   // around the last gpk_assemble evaluator launch while prof is on (gpk_prof_read_assembly)
    bool asm_timed = false;
    int prof_phase = 0;             // phase the step is issuing right now (last GPK_PROF_MARK index): 0 solve, 1 product + factorisation of Hb, ...
    double prof_flops[4] = {0, 0, 0, 0};   // flops EXECUTED by the GEMM launches of each phase while prof is on (gpk_gemm.hip, prof_count)
    long prof_launches[4] = {0, 0, 0, 0};
    std::string err;
};

int gpk_fail(gpk_handle h, hipError_t e, const char* what, const char* file, int line);
int gpk_bad_arg(gpk_handle h, const char* what);

#define GPK_HIP(h, call)                                                          \
    do {                                                                          \
        hipError_t e__ = (call);                                                  \
        if (e__ != hipSuccess) return gpk_fail((h), e__, #call, __FILE__, __LINE__); \
    } while (0)
#define GPK_TRY(expr)               \
    do {                            \
        int r__ = (expr);           \
        if (r__ != 0) return r__;   \
    } while (0)
#define GPK_LAUNCH_CHECK(h) GPK_HIP((h), hipGetLastError())

// Which stream the building blocks issue on, and whether launches on it may use the tile-list / split-K workspace, for the lifetime of the
// scope: use() switches both, the destructor puts both back on every way out.  Apart from gpk_create / gpk_set_stream nothing else
// assigns gpk_ctx::stream, and nothing else writes gpk_ctx::ws_owner.
class GpkStreamScope {
    gpk_handle h;
    const hipStream_t stream0;
    const bool owner0;
public:
    explicit GpkStreamScope(gpk_handle hh) : h(hh), stream0(hh->stream), owner0(hh->ws_owner) {}
    ~GpkStreamScope() { h->stream = stream0; h->ws_owner = owner0; }
    GpkStreamScope(const GpkStreamScope&) = delete;
    GpkStreamScope& operator=(const GpkStreamScope&) = delete;
    void use(hipStream_t s, bool ws_owner) { h->stream = s; h->ws_owner = ws_owner; }
    void back() { use(stream0, owner0); }
};

#ifdef GPK_DEV
// development build only: the argument the extern "C" entry points that take a bare `lead` (gpk_gemm_lz, gpk_trsm_lz, gpk_trsm_dinv,
// gpk_debug_syrk_lz) make of it and of the profile last given to gpk_debug_set_profile
inline GpkLz gpk_debug_lz(gpk_handle h, int lead) {
    if (lead <= 0) return GpkLz();
    return h->debug_profile.is_piecewise() ? h->debug_profile : GpkLz::closed(lead, h->debug_profile.div);
}
#else
inline GpkLz gpk_debug_lz(gpk_handle, int lead) { return GpkLz::closed(lead); }
#endif

// ---- internal (stream-ordered, no host sync) building blocks -------------------------------------------------
// C <- alpha*op(A)*op(B) + beta*C.  lower_only: skip tiles strictly above the diagonal (square C).  lz: leading zeros of B (tb = false;
// with lower_only only for the product A^T A).  splitk: split-K factor asked for (0 / 1 = none); tile: 64 / 128 = 64 x 64 / 128 x 64 tiles
// whatever the tile count (the caller gets its parallelism from split-K), 0 = automatic
int gpk_i_gemm(gpk_handle h, bool ta, bool tb, int m, int n, int k, double alpha, const double* A, int lda,
               const double* B, int ldb, double beta, double* C, int ldc, bool lower_only, const GpkLz& lz = GpkLz(), bool tri_a = false,
               bool skip_upper = false, int splitk = 0, int tile = 0);
int gpk_i_potrf(gpk_handle h, double* A, int n, int lda, int pivot_base);               // info -> h->d_info
int gpk_i_potrf_panel(gpk_handle h, double* A, int nrows, int ob, int lda, int pivot_base, bool left_looking = false,
                      void* ev_wait_p1 = nullptr, void* ev_rec_pre = nullptr);   // (hipEvent_t; see gpk_factor.hip)
// Hb <- chol(W^T W) (lower, nc x nc; W is rows x nc with the leading-zero profile lz), the product and the
// factorisation pipelined by 512-column blocks on two CU partitions (gpk_factor.hip); d_loss (device, may be null) receives
// the unfactored last diagonal entry (W^T W)[nc-1][nc-1]
int gpk_i_syrk_potrf(gpk_handle h, const double* W, int ldw, int rows, int nc, const GpkLz& lz, double* Hb, int ldh, double* d_loss);
int gpk_i_trsm_left(gpk_handle h, bool trans, const double* L, int n, int ldl, double* B, int nrhs, int ldb);
// forward solve exploiting leading zeros of the right-hand side columns (see gpk_factor.hip)
int gpk_i_trsm_left_lz(gpk_handle h, const double* L, int n, int ldl, double* B, int nrhs, int ldb, const GpkLz& lz);
// same, right-hand sides split into independent column groups that run on concurrent streams
int gpk_i_trsm_left_mt(gpk_handle h, bool trans, const double* L, int n, int ldl, double* B, int nrhs, int ldb);
// explicit inverses of the db x db diagonal blocks of L (Dinv: n x db, ld db; db = 256, 512 or 1024) and the all-GEMM forward
// solve built on them: X <- L^{-1} B out of place, B is scratch afterwards (see gpk_factor.hip)
int gpk_i_trtri_diag(gpk_handle h, const double* L, int n, int ldl, double* Dinv, int db);
int gpk_i_trsm_left_dinv(gpk_handle h, const double* L, const double* Dinv, int db, int n, int ldl, double* B, int ldb,
                         double* X, int ldx, int nrhs, const GpkLz& lz);
int gpk_i_pipe_streams(gpk_handle h);                                                   // the two CU-masked streams of the pipeline (gpk_factor.hip); called by gpk_create
void gpk_i_sk_free(gpk_handle h);                                                      // tile-list plans (gpk_gemm.hip)
int gpk_i_splitk_reserve(gpk_handle h);                                                 // workspace + counters of the split-K launches
int gpk_i_workspace(gpk_handle h, size_t bytes, double** out);                          // handle-owned scratch, grown on demand
int gpk_i_trsm_right_lt(gpk_handle h, const double* L, int n, int ldl, double* X, int m, int ldx);
int gpk_i_trsv(gpk_handle h, bool trans, const double* L, int n, int ldl, double* x);   // x contiguous
int gpk_i_dot(gpk_handle h, const double* x, const double* y, int n, double* d_out);    // d_out device scalar
size_t gpk_i_col_sumsq_scratch_bytes(int rows, int cols);                               // gpk_posterior.hip: partial sums of the reduction below
int gpk_i_col_sumsq(gpk_handle h, const double* V, int rows, int cols, int ldv, double* out, double* scratch);   // out[t] = sum_r V[r, t]^2 (gpk_col_sumsq's kernels, caller's scratch)
int gpk_i_ensure_points(gpk_handle h, size_t doubles);
// pieces of the Gauss-Newton step used by the multi-GPU schedule (gpk_gn.hip)
int gpk_i_gn_dims(gpk_handle h, const gpk_gn_problem* p, int* nz, int* rows);
// the column layout gpk_gn_step runs a system in (1 elliptic, 2 Eikonal, 3 Burgers, 4 Darcy, 0 dense) and the leading-zero profile of
// [A(z) | F] (storage order) under it: Eikonal its two-segment profile on the GEMM-only solve path, Burgers the closed form of slope 1/3;
// dense for the layouts 0 and 4 (Darcy's two factors have a profile each: the u-part's is gpk_i_gn_darcy_u_profile)
int gpk_i_gn_layout(gpk_handle h, const gpk_gn_problem* p);
bool gpk_i_gn_sharded(const gpk_gn_problem* p);                                        // gpk_mg_gn_step admits the system (GnTraits::sharded)
GpkLz gpk_i_gn_profile(gpk_handle h, const gpk_gn_problem* p, int rev);
GpkLz gpk_i_gn_darcy_u_profile(int Nd);
int gpk_i_gn_darcy_add_a(gpk_handle h, const gpk_gn_problem* p, double* Hb, int ldh, int r0, int r1, const double* aF, int ldaf);
int gpk_i_gn_exact_loss(gpk_handle h, const gpk_gn_problem* p, const double* z, double** d_out);   // gpk_tune key 52: loss(z) by substitution on h->stream
int gpk_i_gn_finish(gpk_handle h, const gpk_gn_problem* p, int nz, int rev, const double* Hb, int ldh, double* scratch, double* delta,
                    double* z, double step_size, bool update = true);   // update = false: delta only, z is not written (line search)

static inline int gpk_ceil_div(int a, int b) { return (a + b - 1) / b; }
inline bool dinv_block_ok(int db) { return db == 256 || db == 512 || db == 1024 || db == 2048; }   // block sizes of gpk_i_trtri_diag / gpk_i_trsm_left_dinv

// Reaction term tau(u) of the elliptic systems and its derivative (gpk.h, GPK_NL_*; DESIGN.md section K, "Reaction terms").  The one
// place that knows the family: gn_build_kernel, structured_coeff_kernel and pde_residual_nl_kernel call it.  GPK_NL_POWER spells
// alpha * pow(u, m) and alpha * m * pow(u, m - 1.0) exactly as the kernels did before there was a family: same bits.
__device__ __forceinline__ double nl_tau(int kind, double p0, double p1, double p2, double u) {
    switch (kind) {
        case GPK_NL_EXP:   return p0 * exp(p1 * u);
        case GPK_NL_SINH:  return p0 * sinh(p1 * u);
        case GPK_NL_SIN:   return p0 * sin(p1 * u);
        case GPK_NL_CUBIC: return u * (p0 + u * (p1 + p2 * u));
        default:           return p0 * pow(u, p1);
    }
}
__device__ __forceinline__ double nl_dtau(int kind, double p0, double p1, double p2, double u) {
    switch (kind) {
        case GPK_NL_EXP:   return p0 * p1 * exp(p1 * u);
        case GPK_NL_SINH:  return p0 * p1 * cosh(p1 * u);
        case GPK_NL_SIN:   return p0 * p1 * cos(p1 * u);
        case GPK_NL_CUBIC: return p0 + u * (2.0 * p1 + 3.0 * p2 * u);
        default:           return p0 * p1 * pow(u, p1 - 1.0);
    }
}
static inline bool gpk_nl_valid(int kind) { return kind >= GPK_NL_POWER && kind <= GPK_NL_CUBIC; }

// Gradient-dependent nonlinearity of GPK_GN_SEMILINEAR (gpk.h; DESIGN.md section K, "Gradient-dependent nonlinearity"), gq = (a1, a2, b,
// c1, c3):  N(u, p, q) = u (a1 p + a2 q) + b (p p + q q) + u (c1 + c3 u u)  and its partial derivatives (N_u, N_p, N_q).  The one place
// that knows the form: gn_build_kernel and pde_residual_sl_kernel call it.  Every sum and product is written in ONE order, left to right
// as spelled (the compiler may fuse a product into the sum that follows it, never reassociate): a repeated call is bit-identical.
__host__ __device__ __forceinline__ double sl_N(const double* gq, double u, double p, double q) {
    const double conv = u * (gq[0] * p + gq[1] * q);
    const double grad = gq[2] * (p * p + q * q);
    const double reac = u * (gq[3] + gq[4] * (u * u));
    return (conv + grad) + reac;
}
__host__ __device__ __forceinline__ void sl_dN(const double* gq, double u, double p, double q, double* Nu, double* Np, double* Nq) {
    *Nu = (gq[0] * p + gq[1] * q) + (gq[3] + 3.0 * gq[4] * (u * u));
    *Np = gq[0] * u + 2.0 * gq[2] * p;
    *Nq = gq[1] * u + 2.0 * gq[2] * q;
}

// Gradient-dependent nonlinearity of GPK_GN_SEMILINEAR3D (gpk.h; DESIGN.md section K, "Gradient layout in three dimensions"), c = (a1, a2,
// a3, b1, b2, b3, c1, c3):  N(u, g) = u (a1 g1 + a2 g2 + a3 g3) + (b1 g1 g1 + b2 g2 g2 + b3 g3 g3) + u (c1 + c3 u u)  and its partial
// derivatives.  The one place that knows the form: gn_build_kernel and pde_residual_sl3d_kernel call it.  ONE order of operations, left to
// right as spelled, and no contraction (the pragma at the head of each body): the build and the residual give the same bits for the same
// arguments.
struct Sl3Coef { double c[8]; };
__host__ __device__ __forceinline__ double sl3_N(const double* c, double u, double g1, double g2, double g3) {
#pragma clang fp contract(off)
    const double conv = u * ((c[0] * g1 + c[1] * g2) + c[2] * g3);
    const double grad = (c[3] * (g1 * g1) + c[4] * (g2 * g2)) + c[5] * (g3 * g3);
    const double reac = u * (c[6] + c[7] * (u * u));
    return (conv + grad) + reac;
}
__host__ __device__ __forceinline__ void sl3_dN(const double* c, double u, double g1, double g2, double g3, double* Nu, double* N1, double* N2,
                                                double* N3) {
#pragma clang fp contract(off)
    *Nu = ((c[0] * g1 + c[1] * g2) + c[2] * g3) + (c[6] + 3.0 * c[7] * (u * u));
    *N1 = c[0] * u + 2.0 * c[3] * g1;
    *N2 = c[1] * u + 2.0 * c[4] * g2;
    *N3 = c[2] * u + 2.0 * c[5] * g3;
}

// Quasilinear equations of GPK_GN_QUASILINEAR (gpk.h, GPK_QL_*; DESIGN.md section K, "Quasilinear equations: the 2-jet layout"), solved for
// the Laplacian: Laplace(u) = G(f; v0, p, q, D, M) with v0 = u, (p, q) = grad u, D = u_11 - u_22, M = 2 u_12.  g2 = p p + q q, W2 = 1 + g2,
// Q = D (p p - q q) + 2 p q M (= 2 (p p u_11 + 2 p q u_12 + q q u_22) - g2 Laplace(u)), prm = (p0, p1, p2) of gpk_gn_problem:
//   GPK_QL_MEAN_CURVATURE  (kappa = prm[0])            G = (2 W^3 (f + kappa v0) + Q) / (1 + W2)
//   GPK_QL_P_LAPLACE       (m = prm[0], delta = prm[1]) G = (2 f s^((4 - m) / 2) - (m - 2) Q) / (2 delta^2 + m g2),  s = delta^2 + g2
//   GPK_QL_GAUSS_CURVATURE (e = prm[0])                G = sqrt(D D + M M + 4 f W2^e)         (a negative radicand gives NaN)
// ql_dG: dG[0..4] = the partial derivatives by v0, p, q, D, M.  ql_residual: the equation in its divergence / determinant form from
// (u, u_1, u_2, u_11, u_12, u_22).  The one place that knows the three forms: gn_build_kernel, the trial build of the line search and
// pde_residual_ql_kernel call it.  ONE order of operations, left to right as spelled, and no contraction.
__host__ __device__ __forceinline__ double ql_G(int kind, const double* prm, double f, double v0, double p, double q, double D, double M) {
#pragma clang fp contract(off)
    const double pp = p * p, qq = q * q, g2 = pp + qq;
    if (kind == GPK_QL_GAUSS_CURVATURE) return sqrt((D * D + M * M) + 4.0 * f * pow(1.0 + g2, prm[0]));
    const double Q = D * (pp - qq) + 2.0 * (p * q) * M;
    if (kind == GPK_QL_P_LAPLACE) {
        const double m = prm[0], dd = prm[1] * prm[1], s = dd + g2;
        return (2.0 * f * pow(s, 0.5 * (4.0 - m)) - (m - 2.0) * Q) / (2.0 * dd + m * g2);
    }
    const double W2 = 1.0 + g2, W = sqrt(W2);
    return (2.0 * (W2 * W) * (f + prm[0] * v0) + Q) / (1.0 + W2);
}
__host__ __device__ __forceinline__ void ql_dG(int kind, const double* prm, double f, double v0, double p, double q, double D, double M,
                                               double* dG) {
#pragma clang fp contract(off)
    const double pp = p * p, qq = q * q, g2 = pp + qq;
    if (kind == GPK_QL_GAUSS_CURVATURE) {
        const double e = prm[0], W2 = 1.0 + g2;
        const double G = sqrt((D * D + M * M) + 4.0 * f * pow(W2, e));
        const double c = 4.0 * f * e * pow(W2, e - 1.0);
        dG[0] = 0.0; dG[1] = c * p / G; dG[2] = c * q / G; dG[3] = D / G; dG[4] = M / G;
        return;
    }
    const double Q = D * (pp - qq) + 2.0 * (p * q) * M;
    const double Qp = 2.0 * (p * D + q * M), Qq = 2.0 * (p * M - q * D);
    if (kind == GPK_QL_P_LAPLACE) {
        const double m = prm[0], dd = prm[1] * prm[1], s = dd + g2, a = 0.5 * (4.0 - m), c = m - 2.0;
        const double E = 2.0 * dd + m * g2;
        const double G = (2.0 * f * pow(s, a) - c * Q) / E;
        const double k = 4.0 * f * a * pow(s, a - 1.0);
        dG[0] = 0.0;
        dG[1] = ((k * p - c * Qp) - 2.0 * m * p * G) / E;
        dG[2] = ((k * q - c * Qq) - 2.0 * m * q * G) / E;
        dG[3] = -c * (pp - qq) / E;
        dG[4] = -c * (2.0 * (p * q)) / E;
        return;
    }
    const double W2 = 1.0 + g2, W = sqrt(W2), r = f + prm[0] * v0, E = 1.0 + W2;
    const double G = (2.0 * (W2 * W) * r + Q) / E;
    dG[0] = 2.0 * (W2 * W) * prm[0] / E;
    dG[1] = ((6.0 * W * p * r + Qp) - 2.0 * p * G) / E;
    dG[2] = ((6.0 * W * q * r + Qq) - 2.0 * q * G) / E;
    dG[3] = (pp - qq) / E;
    dG[4] = 2.0 * (p * q) / E;
}
__host__ __device__ __forceinline__ double ql_residual(int kind, const double* prm, double f, double u, double u1, double u2, double u11,
                                                       double u12, double u22) {
#pragma clang fp contract(off)
    const double g2 = u1 * u1 + u2 * u2;
    if (kind == GPK_QL_GAUSS_CURVATURE) return (u11 * u22 - u12 * u12) - f * pow(1.0 + g2, prm[0]);
    const double T = (u1 * u1) * u11 + 2.0 * (u1 * u2) * u12 + (u2 * u2) * u22, lap = u11 + u22;
    if (kind == GPK_QL_P_LAPLACE) {
        const double m = prm[0], s = prm[1] * prm[1] + g2;
        return pow(s, 0.5 * (m - 4.0)) * (s * lap + (m - 2.0) * T) - f;
    }
    const double W2 = 1.0 + g2;
    return (W2 * lap - T) / (W2 * sqrt(W2)) - (f + prm[0] * u);
}
// why (kind, p0, p1, p2) is not an equation of the family, or nullptr
static inline const char* gpk_ql_invalid(int kind, double p0, double p1, double p2) {
    if (kind < GPK_QL_MEAN_CURVATURE || kind > GPK_QL_GAUSS_CURVATURE)
        return "GPK_GN_QUASILINEAR: nonlin is not one of GPK_QL_MEAN_CURVATURE .. GPK_QL_GAUSS_CURVATURE";
    if (!(std::isfinite(p0) && std::isfinite(p1) && std::isfinite(p2))) return "GPK_GN_QUASILINEAR: a parameter (p0, p1, p2) is not finite";
    if (kind == GPK_QL_P_LAPLACE && !(p0 > 0.0 && p1 > 0.0)) return "GPK_GN_QUASILINEAR: GPK_QL_P_LAPLACE needs m (p0) > 0 and delta (p1) > 0";
    return nullptr;
}
