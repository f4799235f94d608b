/* gpk_dev.h -- entry points of libgpk_dev.so, the DEVELOPMENT build of the library (csrc/Makefile): the product sources compiled with
 * -DGPK_DEV plus csrc/dev/.  It exports everything libgpk.so exports (include/gpk.h, gpk_mg.h, gpk_debug.h) and, on top,
 *   - the look-ahead factorisation of round 5 (measured, not adopted: gpk_tune key 54) -- the superseded kernel designs of rounds 1-2
 *     (gpk_tune keys 5 = 0, 7 = 1, 21 = 0 / 2, 4 = 2) were removed in round 6,
 *   - the shader-clock stamps of the diagonal-block kernels,
 *   - probes that documented hardware behaviour and the micro-benchmarks that fix the roofline denominators.
 * tests/ and tools/ load it explicitly (gpk.Context(dev=True)); bench.py, the drivers and the host API never do.
 */
#ifndef GPK_DEV_H
#define GPK_DEV_H

#include "gpk.h"
#include "gpk_debug.h"

#ifdef __cplusplus
extern "C" {
#endif

/* development aid: enable/disable and read the shader-clock phase stamps of the 64-wide diagonal-block kernels */
int gpk_debug_stamps(gpk_handle h, unsigned long long* host16, int enable);

/* ---- micro-benchmarks used to fix the roofline denominators ------------------------------------------------ */
int gpk_ubench_mfma_f64(gpk_handle h, int iters, double* host_tflops);      /* v_mfma_f64_16x16x4_f64 issue rate */
int gpk_ubench_hbm_write(gpk_handle h, size_t bytes, int iters, double* host_gbps);
int gpk_ubench_latency(gpk_handle h, int mode, double* host_cycles_per_op);
int gpk_ubench_xcc_map(gpk_handle h, int nblocks, int mode, int* host_out);   /* XCD id (HW_REG_XCC_ID) each workgroup ran on; mode 1: odd workgroups linger */   /* 0 dep. v_fma_f64, 1 indep. v_fma_f64, 2 dep. ds_read, 3 indep. ds_read, 4 dep. mfma_f64 (shader cycles per op, one wave) */
/* which CUs a stream created with hipExtStreamCreateWithCUMask(bits [first_bit, first_bit + nbits)) dispatches to: per
 * workgroup XCC_ID | HW_REG_HW_ID << 8 (tools/cu_mask_probe.py) */
int gpk_ubench_cu_census(gpk_handle h, int first_bit, int nbits, int nblocks, int* host_out);
/* development probe (tools/overlap_probe.py): C2 <- S^T S on a low-priority side stream while potrf(copy of H) runs on the
 * handle's stream; host_ms3 = {potrf alone, syrk alone, both concurrently}.  Round-1 finding: no overlap (5.5 vs 2.9 + 2.5 ms). */
int gpk_debug_overlap_probe(gpk_handle h, double* H, int n, int ldh, const double* S, int k, int lds, double* C2, int ldc,
                            double* host_ms3);

/* EXPERIMENT (round 3): plain NN product C = A B with the operand feed through LDS-DMA (global_load_lds) instead of global ->
 * VGPR -> LDS; same tile as the product kernel.  M, N multiples of 64, K of 16, even leading dimensions, 16-byte aligned A, B.
 * csrc/gpk_gemm_dma_probe.hip, tools/gemm_dma_probe.py. */
int gpk_debug_gemm_dma(gpk_handle h, int m, int n, int k, const double* A, int lda, const double* B, int ldb, double* C, int ldc);

/* ---- leading-zero ("staircase") profiles, for kernel-level tests of their consumers (csrc/dev/gpk_gn_dev_abi.inc) ---- */
/* Inside the library a profile is an ARGUMENT of the building blocks (GpkLz in csrc/gpk_common.h), never handle state.  The entry points
 * below and gpk_gemm_lz, gpk_trsm_lz, gpk_trsm_dinv take a bare `lead`; in this build they complete it with the profile given here:
 * closed form of slope 1/slope_div (nseg = 0), or a piecewise profile of nseg <= 4 segments (c1, a, b, sd: nseg ints each, see GpkStair)
 * whose column `base` is column 0 of the operands, used whenever lead > 0.  nseg = 0, slope_div = 1 resets it.  A call never changes
 * it: it holds until the next gpk_debug_set_profile. */
int gpk_debug_set_profile(gpk_handle h, int slope_div, int nseg, const int* c1, const int* a, const int* b, const int* sd, int base);
/* C <- alpha A^T A + beta C on the lower tiles only, A (k x n) with leading zeros (lead, or the profile of gpk_debug_set_profile):
 * the product that forms Hb = S^T S inside gpk_gn_step */
int gpk_debug_syrk_lz(gpk_handle h, int n, int k, double alpha, const double* A, int lda, double beta, double* C, int ldc, int lead);
/* first_row(c) for the n_z columns of [A(z) | F] under the layout gpk_gn_step enters for host_prob -> out_u; Darcy: out_a (may be
 * null) the a-part's closed form on the columns [N_d, 4 N_d), 3 N_d elsewhere.  Returns the layout (1 elliptic systems, 2 Eikonal,
 * 3 Burgers, 4 Darcy); a problem on the dense schedule is refused. */
int gpk_debug_first_rows(gpk_handle h, const gpk_gn_problem* host_prob, int* out_u, int* out_a);
/* Which way gpk_gn_step would run host_prob on this handle, without running it: *mode = 0 plain solve, 1 structured solve of the elliptic
 * system, 2 its Gram level, 3 structured solve of the Burgers / Eikonal / Darcy systems, 4 their Gram level; *product = what follows the
 * mode: 0 nothing (the Gram levels factor the bordered matrix themselves), 1 the pipelined product + Cholesky, 2 Darcy's two-factor
 * product.  Nothing is launched and no device pointer is dereferenced. */
int gpk_debug_step_mode(gpk_handle h, const gpk_gn_problem* host_prob, int* mode, int* product);
/* The first launch of gpk_gn_trial_losses alone: column k < K of W (s_rows x ldw) <- F(z - host_t[k] delta), built and not solved. */
int gpk_debug_gn_trial_build(gpk_handle h, const gpk_gn_problem* host_prob, const double* z, const double* delta, const double* host_t, int K,
                             double* W, int ldw);
/* *host_bytes = current size of the handle's workspace (gpk_i_workspace: the out-of-place solve buffers, partial sums of gpk_col_sumsq): what
 * tests hold against the handle_bytes of gpk_gn_worksize / gpk_posterior_worksize. */
int gpk_debug_workspace_bytes(gpk_handle h, size_t* host_bytes);

#ifdef __cplusplus
}
#endif
#endif /* GPK_DEV_H */
