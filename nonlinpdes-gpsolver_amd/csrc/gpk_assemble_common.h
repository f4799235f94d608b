// gpk_assemble_common.h -- what the twelve Gram-evaluator translation units share (gpk_assemble.hip: the reference layouts and their
// Gaussian family, gpk_assemble_matern.hip: their Matern family, gpk_assemble_periodic.hip: their periodic kernel, gpk_assemble3d.hip,
// gpk_assemble_bc.hip: Neumann / Robin, gpk_assemble_op.hip: variable-coefficient operator, gpk_assemble_op3d.hip: the operator and the
// boundary functionals in three dimensions, gpk_assemble_hess.hip: the Hessian layout, gpk_assemble_jet2.hip: the 2-jet layout, gpk_assemble_disp.hip: the dispersive layout,
// gpk_assemble_evo.hip: the evolution layout with the general spatial operator,
// gpk_assemble_grad3d.hip: the gradient layout in three
// dimensions, which shares gpk_assemble_op3.h with gpk_assemble_op3d.hip).  The kernels and the per-pair arithmetic that
// differs between them (pair_coeff in its roundings, pair_coeff3, the tables of the operator) stay in those files -- the kernels of the
// reference layouts, which three of them share, in gpk_assemble_frames.h; here is the scaffolding around them, each piece once:
// functional tables, the two Hermite evaluations, the frame of the extension kernels, the 16-byte store, and the host side of an
// evaluator call (precisions, nugget, trace, timing, launch).
#pragma once
#include "gpk_common.h"

#include <type_traits>

namespace gpk_asm {

// ---- functionals of the 2-D evaluators: multi-index lists (F_LAP = d11 + d22, the others one multi-index each) ----------------------
enum { F_DELTA = 0, F_D1 = 1, F_D2 = 2, F_DD2 = 3, F_LAP = 4 };

__host__ __device__ constexpr int f_count(int f) { return f == F_LAP ? 2 : 1; }
__host__ __device__ constexpr int f_a1(int f, int i) { return f == F_D1 ? 1 : (f == F_LAP && i == 0 ? 2 : 0); }
__host__ __device__ constexpr int f_a2(int f, int i) { return f == F_D2 ? 1 : (f == F_DD2 ? 2 : (f == F_LAP && i == 1 ? 2 : 0)); }

// ---- 1-D Hermite factors h0..h4 of p and d, q = p d ----------------------------------------------------------------
// Plain form (reference layouts, 3-D), compiled under the including file's default: the compiler may contract.
__host__ __device__ __forceinline__ void hermite_plain(double p, double d, double (&h)[5]) {
    const double q = p * d;
    const double q2 = q * q;
    h[0] = 1.0;
    h[1] = q;
    h[2] = q2 - p;
    h[3] = q * (q2 - 3.0 * p);
    h[4] = q2 * (q2 - 6.0 * p) + 3.0 * p * p;
}

// What the one-point and the two-point evaluator of bc / op must compute with the same bits for the same point pair is written with
// explicit fma and compiled without contraction: whether the compiler contracts a given a * b + c depends on how many uses the product
// has after inlining, which differs between the two evaluators.  The pragma stands at the head of each function body, so it ends with
// the body: the including file keeps the state it had.

// Compensated form (bc, op).  h2 = q^2 - p and h3 = q (q^2 - 3p) cancel near q^2 = p and q^2 = 3p, where the roundings of q and q^2
// (~eps p) would be all that is left of the factor.  In the reference layouts another term of the entry always covers that; with a
// first- or second-order functional an entry can consist of such factors alone (Neumann column against a Laplacian row: a3 + a1 b2;
// <d11, delta'> = h2 kappa), so both brackets carry the rounding errors of q and q^2 along (explicit fma: exact error of a product): h2
// and h3 are accurate relative to THEMSELVES, for ~8 more operations per axis.  h4 has no partner that vanishes with it (its roots are
// not those of h2), so it stays plain.
__host__ __device__ __forceinline__ void hermite_compensated(double p, double d, double (&h)[5]) {
#pragma clang fp contract(off)
    const double q = p * d;
    const double qe = __builtin_fma(p, d, -q);                    // p d = q + qe exactly
    const double q2 = q * q;
    const double q2e = __builtin_fma(2.0 * q, qe, __builtin_fma(q, q, -q2));   // (p d)^2 = q2 + q2e up to second order
    const double t = 3.0 * p;
    const double te = __builtin_fma(3.0, p, -t);                  // 3 p = t + te exactly
    h[0] = 1.0;
    h[1] = q;
    h[2] = (q2 - p) + q2e;
    h[3] = q * ((q2 - t) + (q2e - te));
    h[4] = __builtin_fma(q2, q2 - 6.0 * p, 3.0 * p * p);
}

// Orders 0..N-1, N up to 11 (evo: <Q,Q> with a fifth derivative reaches order ten).  h0..h4 are hermite_compensated's; from there the
// three-term recurrence h_(n+1) = q h_n - n p h_(n-1), one fma per order.  Not Horner in q^2: the monomials of He_10 reach 6e5 where the
// polynomial is 1e4 (s = sqrt(p) d near 2.5), and their roundings would be ~7 eps of the value at d = 0 after the Gaussian factor; the
// terms of the recurrence are of the size of the polynomials themselves.  q is odd in d, so h_n(-d) = (-1)^n h_n(d) to the bit.
template <int N>
__host__ __device__ __forceinline__ void hermite_recurrence(double p, double d, double (&h)[N]) {
#pragma clang fp contract(off)
    static_assert(N >= 5 && N <= 11, "orders 4 .. 10");
    double l[5];
    hermite_compensated(p, d, l);
#pragma unroll
    for (int n = 0; n < 5; ++n) h[n] = l[n];
    const double q = p * d;
#pragma unroll
    for (int n = 4; n + 1 < N; ++n) h[n + 1] = __builtin_fma(q, h[n], -(((double)n * p) * h[n - 1]));
}

// kappa of bc / op: exp(-(p1 d1^2 + p2 d2^2) / 2) with the one fma written out
__host__ __device__ __forceinline__ double kappa2_fma(double p1, double p2, double d1, double d2) {
#pragma clang fp contract(off)
    return exp(-0.5 * __builtin_fma(p2 * d2, d2, p1 * d1 * d1));
}

// ---- frame of the extension kernels (DESIGN.md §K "Row functionals of the extension") -------------------------------------------------
// A workgroup of 256 lanes owns FN_TT test points (wave-uniform: scalar loads) and strides over the column points; each lane keeps
// FN_TT x NF accumulators, NF = popcount(mask).  Reduction: wave shuffles, then LDS across the 4 waves, in a fixed order (no atomics:
// a repeated call gives bit-identical output).
constexpr int TP = 32;                    // row points per workgroup (Gram and test-row evaluators)
constexpr int FN_TT = 4;                  // test points per workgroup (extension kernels)

__host__ __device__ constexpr int fn_popc(int m) { return m ? (m & 1) + fn_popc(m >> 1) : 0; }
// output row of functional F under MASK: the number of set bits below bit F
__host__ __device__ constexpr int fn_row(int mask, int f) { return fn_popc(mask & ((1 << f) - 1)); }

// The loading of the test points and the reduction are macros, not functions: inlined functions of the same text compile to other
// register assignments and load placements in a part of the extension kernels (the argument struct's loads move), and a change of
// these kernels' code is a change of their cost that nothing here wants.  The zeroing is a function; it takes the rows by pointer for
// the same reason.
// x1[i], x2[i] (, x3[i]) = coordinates of test point t0 + i of the (Nt, 2) or (Nt, 3) row-major tx, i < FN_TT; past the end: repeat the
// last point (computed, never stored)
#define GPK_FN_LOAD_POINTS2(x1, x2, tx, t0, Nt)                                                                            \
    _Pragma("unroll") for (int i = 0; i < FN_TT; ++i) {                                                                    \
        const int t = min((t0) + i, (Nt) - 1);                                                                             \
        (x1)[i] = (tx)[2 * t]; (x2)[i] = (tx)[2 * t + 1];                                                                  \
    }
#define GPK_FN_LOAD_POINTS3(x1, x2, x3, tx, t0, Nt)                                                                        \
    _Pragma("unroll") for (int i = 0; i < FN_TT; ++i) {                                                                    \
        const int t = min((t0) + i, (Nt) - 1);                                                                             \
        (x1)[i] = (tx)[3 * t]; (x2)[i] = (tx)[3 * t + 1]; (x3)[i] = (tx)[3 * t + 2];                                       \
    }

template <int NF>
__device__ __forceinline__ void fn_zero(double (*s)[NF]) {
#pragma unroll
    for (int i = 0; i < FN_TT; ++i)
#pragma unroll
        for (int k = 0; k < NF; ++k) s[i][k] = 0.0;
}

// out[k * ldo + t0 + i] = sum over the workgroup of s[i][k] (double s[FN_TT][NF]); every lane of the workgroup must reach it
#define GPK_FN_REDUCE_STORE(s, NF, t0, Nt, out, ldo)                                                                       \
    do {                                                                                                                   \
        __shared__ double red[4][FN_TT * (NF)];                                                                            \
        _Pragma("unroll") for (int i = 0; i < FN_TT; ++i)                                                                  \
            _Pragma("unroll") for (int k = 0; k < (NF); ++k) {                                                             \
                double v = (s)[i][k];                                                                                      \
                for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);                                               \
                if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][i * (NF) + k] = v;                                      \
            }                                                                                                              \
        __syncthreads();                                                                                                   \
        if (threadIdx.x < FN_TT * (NF)) {                                                                                  \
            const int i = threadIdx.x / (NF), k = threadIdx.x % (NF), t = (t0) + i;                                        \
            if (t < (Nt)) (out)[k * (ldo) + t] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]); \
        }                                                                                                                  \
    } while (0)

// f(std::integral_constant<int, MASK>) for the MASK in 1..MAX that equals mask: one kernel instantiation per mask, so a functional
// that is not requested costs nothing
template <int MAX, int MASK = 1, class F>
void with_mask(int mask, F&& f) {
    if constexpr (MASK <= MAX) {
        if (mask == MASK) f(std::integral_constant<int, MASK>{});
        else with_mask<MAX, MASK + 1>(mask, f);
    }
}

// ---- the 16-byte store of the two-point evaluators ------------------------------------------------------------------------------------
// NT (gpk_tune key 55): Theta is written once and not read by the evaluator -- 1: a non-temporal store (global_store_dwordx4 ... nt)
// tells L2 / the Infinity Cache not to keep the line; 2 / 3: write-through scopes sc0 sc1 without / with nt, inline assembly (measured
// next to it; instantiated by gpk_assemble.hip only); 0: plain.
template <int NT>
__device__ __forceinline__ void store2(double* dst, double v0, double v1) {
    typedef double d2 __attribute__((ext_vector_type(2)));
    d2* const p = reinterpret_cast<d2*>(dst);
    const d2 v = (d2){v0, v1};
    if (NT == 1) __builtin_nontemporal_store(v, p);
    else if (NT == 2) asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" :: "v"(p), "v"(v) : "memory");
    else if (NT == 3) asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1 nt" :: "v"(p), "v"(v) : "memory");
    else *p = v;
}

// ---- host side of an evaluator call ---------------------------------------------------------------------------------------------------
// precisions p[0..dim) of the kernel: 1/sigma^2 (Gaussian, src/kernels.py:12-13) or 2/sigma_k^2 (anisotropic, :95-99 -- no factor 1/2:
// the reference's convention); an unknown kernel id is reported as `who`
inline int precisions(gpk_handle h, const char* who, int kernel, const double* kp, int dim, double* p) {
    if (kernel == GPK_KERNEL_GAUSSIAN) { for (int k = 0; k < dim; ++k) p[k] = 1.0 / (kp[0] * kp[0]); }
    else if (kernel == GPK_KERNEL_ANISOTROPIC) { for (int k = 0; k < dim; ++k) p[k] = 2.0 / (kp[k] * kp[k]); }
    else return gpk_bad_arg(h, who);
    return 0;
}

inline bool nugget_type_valid(int nugget_type) {
    return nugget_type == GPK_NUGGET_NONE || nugget_type == GPK_NUGGET_IDENTITY || nugget_type == GPK_NUGGET_ADAPTIVE;
}

// nugget of a block whose trace is `ratio` times that of the last block (the last block itself: ratio = 1)
inline double block_nugget(int nugget_type, double nugget, double ratio) {
    return nugget_type == GPK_NUGGET_ADAPTIVE ? nugget * ratio : (nugget_type == GPK_NUGGET_IDENTITY ? nugget : 0.0);
}

// the two-block layouts (3-D, bc, op): r0 = trace(block 0) / trace(block 1)
inline void two_block_nugget(int nugget_type, double nugget, double r0, double (&nug)[2]) {
    nug[0] = block_nugget(nugget_type, nugget, r0);
    nug[1] = block_nugget(nugget_type, nugget, 1.0);
}

// *tr = sum_b <phi_b, phi_b> at d = 0 = sum_b (c0_b^2 + p1 c1_b^2 + p2 c2_b^2) over the Nb boundary functionals bc (device, (Nb,3)), Nb
// when bc == NULL (delta everywhere).  Taken on the host from the coefficient array, in index order and in long double, so that a
// trace ratio built on it is the analytic value to an ulp and the same on every call.  Synchronises the stream.
inline int boundary_trace(gpk_handle h, const double* bc, int Nb, long double p1, long double p2, long double* tr) {
    *tr = (long double)Nb;
    if (!bc || Nb <= 0) return 0;
    std::vector<double> hb(3 * (size_t)Nb);
    GPK_HIP(h, hipMemcpyAsync(hb.data(), bc, hb.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    GPK_HIP(h, hipStreamSynchronize(h->stream));
    long double sb = 0.0L;
    for (int b = 0; b < Nb; ++b) {
        const long double b0 = hb[3 * (size_t)b], b1 = hb[3 * (size_t)b + 1], b2 = hb[3 * (size_t)b + 2];
        sb += b0 * b0 + p1 * b1 * b1 + p2 * b2 * b2;
    }
    *tr = sb;
    return 0;
}

// the same in three dimensions: bc (device, (Nb,4)) rows (c0, c1, c2, c3), *tr = sum_b (c0_b^2 + sum_k p_k ck_b^2); Nb when bc == NULL
inline int boundary_trace3(gpk_handle h, const double* bc, int Nb, const long double (&p)[3], long double* tr) {
    *tr = (long double)Nb;
    if (!bc || Nb <= 0) return 0;
    std::vector<double> hb(4 * (size_t)Nb);
    GPK_HIP(h, hipMemcpyAsync(hb.data(), bc, hb.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    GPK_HIP(h, hipStreamSynchronize(h->stream));
    long double sb = 0.0L;
    for (int b = 0; b < Nb; ++b) {
        const double* c = hb.data() + 4 * (size_t)b;
        const long double b0 = c[0], b1 = c[1], b2 = c[2], b3 = c[3];
        sb += b0 * b0 + p[0] * b1 * b1 + p[1] * b2 * b2 + p[2] * b3 * b3;
    }
    *tr = sb;
    return 0;
}

// Two column points per lane (16-byte stores) need every pair (q, q + 1) inside one block and 16-byte aligned: an even leading
// dimension, an aligned base and every one of `counts` (point counts, block sizes) even.  gpk_tune key 47 = 0 turns the variant off.
template <class... Counts>
bool pairs_eligible(gpk_handle h, const double* Theta, int ld, Counts... counts) {
    return h->tune.asm_pairs && (ld % 2 == 0) && (((uintptr_t)Theta & 15) == 0) && (... && (counts % 2 == 0));
}

// Per-phase timing (h->prof): HIP events around the evaluator launch alone -- the point packing and the host work before it stay
// outside; gpk_prof_read_assembly reads them.  start() records the first event, leaving the scope records the second.
class TimedLaunch {
public:
    explicit TimedLaunch(gpk_handle handle) : h(handle) {}
    TimedLaunch(const TimedLaunch&) = delete;
    int start() {
        if (h->prof) {
            if (!h->asm_ev[0]) for (int i = 0; i < 2; ++i) GPK_HIP(h, hipEventCreate(&h->asm_ev[i]));
            GPK_HIP(h, hipEventRecord(h->asm_ev[0], h->stream));
        }
        started = true;
        return 0;
    }
    ~TimedLaunch() {
        if (started && h->prof && h->asm_ev[1]) h->asm_timed = hipEventRecord(h->asm_ev[1], h->stream) == hipSuccess;
    }
private:
    gpk_handle h;
    bool started = false;
};

// The Gram launch of a two-block evaluator, timed: the two-point kernel (plain, or non-temporal under key 55 = 1; the write-through
// values 2 / 3 of gpk_assemble are inline assembly and not offered here: plain) when pairs, else the one-point kernel.
template <class Args>
int launch_two_block(gpk_handle h, bool pairs, const Args& g, void (*one)(Args), void (*two)(Args), void (*two_nt)(Args)) {
    TimedLaunch timed(h);
    GPK_TRY(timed.start());
    if (pairs) (h->tune.asm_nt == 1 ? two_nt : two)<<<dim3(gpk_ceil_div(g.M / 2, 256), gpk_ceil_div(g.M, TP)), 256, 0, h->stream>>>(g);
    else one<<<dim3(gpk_ceil_div(g.M, 256), gpk_ceil_div(g.M, TP)), 256, 0, h->stream>>>(g);
    GPK_LAUNCH_CHECK(h);
    return 0;
}

}  // namespace gpk_asm
