// gpk_evidence.hip -- Laplace log evidence of a factored problem at its Gauss-Newton iterate ("Log evidence").
//
// No reference call site: the reference takes the kernel parameter by hand.  With F(z) the stacked measurement vector, A = dF/dz at z*,
// L_k L_k^T = Theta_k, J(z) = sum_k ||L_k^{-1} F_k(z)||^2 (+ Darcy's data misfit) and H/2 = A^T Theta^{-1} A = R R^T,
//     log Z = -J(z*)/2 - sum_k sum_i log (L_k)_ii - sum_i log R_ii - N_data log gamma - (rows - n_z)/2 log 2 pi.
// Every piece is the library's: J is gpk_gn_loss, R is gpk_posterior_prepare's.  What is new here is the log-determinant of a Cholesky
// factor: a reduction over its diagonal in a fixed order.
#include "gpk_common.h"
#include <cmath>

namespace {

// ---- sum_i log L_ii and the count of entries that are not > 0 -----------------------------------------------------------------------------
// Workgroup b takes the diagonal entries [b LOGDET_CHUNK, (b + 1) LOGDET_CHUNK): lane t sums the entries t, t + 256, ... of the chunk,
// the 64 lanes of a wave are folded by shuffles, the 4 waves through LDS.  A second kernel adds the workgroups' partial sums in index
// order: no atomics, the order depends on n alone, a repeated call gives the same bits.  Only the diagonal is read (stride ldl + 1).
constexpr int LOGDET_CHUNK = 2048;

int logdet_blocks(int n) { return gpk_ceil_div(n, LOGDET_CHUNK); }
size_t logdet_scratch_bytes(int n) { return (size_t)logdet_blocks(n) * 2 * sizeof(double); }

__global__ __launch_bounds__(256) void diag_logsum_partial_kernel(const double* __restrict__ L, int n, long stride,
                                                                  double* __restrict__ partial) {
    __shared__ double red_s[4];
    __shared__ int red_b[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int i0 = blockIdx.x * LOGDET_CHUNK;
    const int i1 = min(i0 + LOGDET_CHUNK, n);
    double s = 0.0;
    int bad = 0;
    for (int i = i0 + (int)threadIdx.x; i < i1; i += 256) {
        const double d = L[(long)i * stride];
        s += log(d);
        bad += !(d > 0.0);                                           // zero, negative, NaN
    }
    for (int off = 32; off > 0; off >>= 1) {
        s += __shfl_down(s, off, 64);
        bad += __shfl_down(bad, off, 64);
    }
    if (lane == 0) { red_s[w] = s; red_b[w] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = (red_s[0] + red_s[1]) + (red_s[2] + red_s[3]);
        partial[2 * blockIdx.x + 1] = (double)((red_b[0] + red_b[1]) + (red_b[2] + red_b[3]));   // (a count below 2^31: exact)
    }
}

// out[0] = 2 sum_b partial sums (log |L L^T|), out[1] = the count, as a double
__global__ void diag_logsum_finish_kernel(const double* __restrict__ partial, int nb, double* __restrict__ out) {
    double s = 0.0, bad = 0.0;
    for (int b = 0; b < nb; ++b) { s += partial[2 * b]; bad += partial[2 * b + 1]; }
    out[0] = 2.0 * s;
    out[1] = bad;
}

// stream-ordered: d_out[0..1] on the device; scratch: logdet_scratch_bytes(n)
int chol_logdet(gpk_handle h, const double* L, int n, int ldl, double* scratch, double* d_out) {
    const int nb = logdet_blocks(n);
    diag_logsum_partial_kernel<<<nb, 256, 0, h->stream>>>(L, n, (long)ldl + 1, scratch);
    GPK_LAUNCH_CHECK(h);
    diag_logsum_finish_kernel<<<1, 1, 0, h->stream>>>(scratch, nb, d_out);
    GPK_LAUNCH_CHECK(h);
    return 0;
}

double* evidence_scalars(gpk_handle h) { return h->d_scalars + GPK_SCALARS_EVIDENCE; }   // 6 of the handle's 64 reduction scalars: up to three (value, count) pairs

}  // namespace

extern "C" int gpk_chol_logdet(gpk_handle h, const double* L, int n, int ldl, double* host_logdet, int* host_bad) {
    if (!h) return GPK_ERR_ARG;
    if (!L || !host_logdet || !host_bad) return gpk_bad_arg(h, "chol_logdet: pointers");
    if (n <= 0) return gpk_bad_arg(h, "chol_logdet: n <= 0");
    if (ldl < n) return gpk_bad_arg(h, "chol_logdet: ldl < n");
    double* scratch = nullptr;
    GPK_TRY(gpk_i_workspace(h, logdet_scratch_bytes(n), &scratch));
    h->work_sig[0] = -1;                                             // the workspace no longer holds the zero region of a solve
    GPK_TRY(chol_logdet(h, L, n, ldl, scratch, evidence_scalars(h)));
    double r[2];
    GPK_HIP(h, hipMemcpyAsync(r, evidence_scalars(h), sizeof r, hipMemcpyDeviceToHost, h->stream));
    GPK_HIP(h, hipStreamSynchronize(h->stream));
    *host_logdet = r[0];
    *host_bad = (int)r[1];
    return 0;
}

extern "C" int gpk_log_evidence(gpk_handle h, const gpk_gn_problem* p, const double* z, double* P, int ldp, double* R, int ldr,
                                double* work, double* host_terms, int* host_info) {
    if (!h) return GPK_ERR_ARG;
    if (!work || !host_terms || !host_info) return gpk_bad_arg(h, "log_evidence: null work / host_terms / host_info");
    // P = L^{-1} A(z*), R = chol(H/2): every check of the problem and of z, P, R is prepare's (the relaxed system: -9001 with its message)
    GPK_TRY(gpk_posterior_prepare(h, p, z, P, ldp, R, ldr, host_info));
    int nz = 0, rows = 0;
    GPK_TRY(gpk_gn_dims(p, &nz, &rows));
    double J = 0.0;
    GPK_TRY(gpk_gn_loss(h, p, z, work, &J));
    // log |Theta_k| of every factor, then log |H/2|
    const bool darcy = p->system == GPK_GN_DARCY;
    struct { const double* L; int n, ld; } fac[3];
    int nfac = 0;
    fac[nfac++] = {p->L, darcy ? 4 * p->Nd + p->Nb : rows, p->ldl};
    if (darcy) fac[nfac++] = {p->L2, 3 * p->Nd, p->ldl2};
    fac[nfac++] = {R, nz, ldr};
    size_t bytes = 0;
    for (int k = 0; k < nfac; ++k) bytes = logdet_scratch_bytes(fac[k].n) > bytes ? logdet_scratch_bytes(fac[k].n) : bytes;
    double* scratch = nullptr;
    GPK_TRY(gpk_i_workspace(h, bytes, &scratch));
    h->work_sig[0] = -1;
    double* const d_out = evidence_scalars(h);
    for (int k = 0; k < nfac; ++k) GPK_TRY(chol_logdet(h, fac[k].L, fac[k].n, fac[k].ld, scratch, d_out + 2 * k));   // (stream-ordered: one scratch)
    double r[6];
    GPK_HIP(h, hipMemcpyAsync(r, d_out, (size_t)nfac * 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    GPK_HIP(h, hipStreamSynchronize(h->stream));
    double logdet_theta = 0.0, bad = 0.0;
    for (int k = 0; k + 1 < nfac; ++k) { logdet_theta += r[2 * k]; bad += r[2 * k + 1]; }
    const double logdet_h = r[2 * (nfac - 1)];
    bad += r[2 * (nfac - 1) + 1];
    const double lgamma_term = darcy && p->Ndata > 0 ? (double)p->Ndata * std::log(p->p0) : 0.0;
    const double l2pi_term = 0.5 * (double)(rows - nz) * std::log(6.283185307179586476925);
    host_terms[1] = J;
    host_terms[2] = logdet_theta;
    host_terms[3] = logdet_h;
    host_terms[4] = lgamma_term;
    host_terms[5] = l2pi_term;
    host_terms[0] = (*host_info != 0 || bad != 0.0) ? std::nan("") : -0.5 * J - 0.5 * logdet_theta - 0.5 * logdet_h - lgamma_term - l2pi_term;
    return 0;
}
