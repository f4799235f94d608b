// gpk_assemble_op3.h -- what the two 3-D evaluators with per-point functionals share (gpk_assemble_op3d.hip: psi and phi in the elliptic
// layout; gpk_assemble_grad3d.hip: the same two with the three first derivatives of u as row blocks of their own): the order MI3 of the
// ten monomials, kappa, the contraction of a column functional with the three Hermite tables (table_psi3 / table_phi3), the rows taken from
// it (row_psi3 / row_phi3), the packed scratch with its packing kernel, the masked reduction of the extension kernels and the values
// <psi, psi>(0).  Math: DESIGN.md §K "Operator and boundary functionals in three dimensions".
//
// What the one-point and the two-point evaluator of a layout must compute with the same bits is written with explicit fma; the pragma
// stands at the head of each function body (as in gpk_assemble_common.h), so the including file keeps the state it had.
#pragma once
#include "gpk_assemble_common.h"

namespace gpk_asm {
namespace {

constexpr int NO = 10;                    // coefficients of psi
constexpr int NC = 4;                     // coefficients of phi
constexpr int NARR = 3 + NC + NO;         // packed arrays: x, y, z, phi, psi

// index in MI3 of (m1, m2, m3), m1 + m2 + m3 <= 2
__host__ __device__ constexpr int mi3(int m1, int m2, int m3) {
    return m1 + m2 + m3 == 0 ? 0
         : m1 + m2 + m3 == 1 ? (m1 ? 1 : (m2 ? 2 : 3))
         : m1 == 2 ? 4 : (m1 == 1 ? (m2 ? 5 : 6) : (m2 == 2 ? 7 : (m2 == 1 ? 8 : 9)));
}

// kappa: exp(-(p1 d1^2 + p2 d2^2 + p3 d3^2) / 2), the argument one fma chain over the three axes
__host__ __device__ __forceinline__ double kappa3_fma(double p1, double p2, double p3, double d1, double d2, double d3) {
#pragma clang fp contract(off)
    return exp(-0.5 * __builtin_fma(p3 * d3, d3, __builtin_fma(p2 * d2, d2, p1 * d1 * d1)));
}

// C[mi3(m)] = sum_j k_j a[m1 + b1_j] b[m2 + b2_j] c[m3 + b3_j] for the second-order column functional k (MI3 order), axis 1 first.  The
// parts of k grouped by their orders (b2, b3) along axes 2 and 3:
//   A00 = k0 a[m1] + k1 a[m1+1] + k4 a[m1+2],  A10 = k2 a[m1] + k5 a[m1+1],  A01 = k3 a[m1] + k6 a[m1+1],  A20 = k7 a[m1],  A11 = k8 a[m1],  A02 = k9 a[m1]
// then axis 2, grouped by b3:  B0 = b[m2] A00 + b[m2+1] A10 + b[m2+2] A20,  B1 = b[m2] A01 + b[m2+1] A11,  B2 = b[m2] A02
// then axis 3:  C = c[m3] B0 + c[m3+1] B1 + c[m3+2] B2.
// NE: the entries wanted are the first NE of MI3 (1: value, 4: up to the gradient, 10: all); the others are not computed.
template <int NE = NO>
__host__ __device__ __forceinline__ void table_psi3(const double (&a)[5], const double (&b)[5], const double (&c)[5], const double (&k)[NO],
                                                    double (&t)[NO]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int m1 = 0; m1 < 3; ++m1) {
        if (mi3(m1, 0, 0) >= NE) continue;
        const double A00 = __builtin_fma(k[4], a[m1 + 2], __builtin_fma(k[1], a[m1 + 1], k[0] * a[m1]));
        const double A10 = __builtin_fma(k[5], a[m1 + 1], k[2] * a[m1]);
        const double A01 = __builtin_fma(k[6], a[m1 + 1], k[3] * a[m1]);
        const double A20 = k[7] * a[m1];
        const double A11 = k[8] * a[m1];
        const double A02 = k[9] * a[m1];
#pragma unroll
        for (int m2 = 0; m1 + m2 < 3; ++m2) {
            if (mi3(m1, m2, 0) >= NE) continue;
            const double B0 = __builtin_fma(b[m2 + 2], A20, __builtin_fma(b[m2 + 1], A10, b[m2] * A00));
            const double B1 = __builtin_fma(b[m2 + 1], A11, b[m2] * A01);
            const double B2 = b[m2] * A02;
#pragma unroll
            for (int m3 = 0; m1 + m2 + m3 < 3; ++m3)
                if (mi3(m1, m2, m3) < NE) t[mi3(m1, m2, m3)] = __builtin_fma(c[m3 + 2], B2, __builtin_fma(c[m3 + 1], B1, c[m3] * B0));
        }
    }
}

// the same for the first-order column functional k = (c0, c1, c2, c3)
__host__ __device__ __forceinline__ void table_phi3(const double (&a)[5], const double (&b)[5], const double (&c)[5], const double (&k)[NC],
                                                    double (&t)[NO]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int m1 = 0; m1 < 3; ++m1) {
        const double A00 = __builtin_fma(k[1], a[m1 + 1], k[0] * a[m1]);
        const double A10 = k[2] * a[m1];
        const double A01 = k[3] * a[m1];
#pragma unroll
        for (int m2 = 0; m1 + m2 < 3; ++m2) {
            const double B0 = __builtin_fma(b[m2 + 1], A10, b[m2] * A00);
            const double B1 = b[m2] * A01;
#pragma unroll
            for (int m3 = 0; m1 + m2 + m3 < 3; ++m3) t[mi3(m1, m2, m3)] = __builtin_fma(c[m3 + 1], B1, c[m3] * B0);
        }
    }
}

// sum_i r_i (-1)^{|alpha_i|} C[alpha_i]: the odd row functionals d_1, d_2, d_3 enter with a minus sign (exact)
template <int NR>
__host__ __device__ __forceinline__ double row_phi3(const double (&t)[NO], const double (&r)[NR]) {
#pragma clang fp contract(off)
    return __builtin_fma(-r[3], t[3], __builtin_fma(-r[2], t[2], __builtin_fma(-r[1], t[1], r[0] * t[0])));
}

__host__ __device__ __forceinline__ double row_psi3(const double (&t)[NO], const double (&r)[NO]) {
#pragma clang fp contract(off)
    double s = row_phi3(t, r);
#pragma unroll
    for (int j = 4; j < NO; ++j) s = __builtin_fma(r[j], t[j], s);
    return s;
}

// The packed scratch as the Gram kernels see it: written by pack_op3_kernel in an earlier launch, read-only here.  In the constant
// address space a load at a wave-uniform address (the row point) becomes a scalar load; one at a per-lane address (the column point)
// stays a vector load.
typedef const __attribute__((address_space(4))) double* cdouble_p;

// domain point i: phi = (1,0,0,0), psi = op3[10i..10i+9] or the Laplacian (0,0,0,0,1,0,0,1,0,1) when op3 == NULL; boundary point b:
// phi = bc3[4b..4b+3] or (1,0,0,0) when bc3 == NULL, psi = 0 (never used)
__global__ void pack_op3_kernel(const double* __restrict__ Xd, int Nd, const double* __restrict__ Xb, int Nb, const double* __restrict__ op,
                                const double* __restrict__ bc, double* __restrict__ s) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t M = (size_t)Nd + (size_t)Nb;
    if (i < Nd) {
#pragma unroll
        for (int k = 0; k < 3; ++k) s[k * M + i] = Xd[3 * (size_t)i + k];
#pragma unroll
        for (int j = 0; j < NC; ++j) s[(3 + j) * M + i] = j == 0 ? 1.0 : 0.0;
#pragma unroll
        for (int j = 0; j < NO; ++j) s[(3 + NC + j) * M + i] = op ? op[NO * (size_t)i + j] : ((j == 4 || j == 7 || j == 9) ? 1.0 : 0.0);
    } else if (i < Nd + Nb) {
        const int b = i - Nd;
#pragma unroll
        for (int k = 0; k < 3; ++k) s[k * M + i] = Xb[3 * (size_t)b + k];
#pragma unroll
        for (int j = 0; j < NC; ++j) s[(3 + j) * M + i] = bc ? bc[NC * (size_t)b + j] : (j == 0 ? 1.0 : 0.0);
#pragma unroll
        for (int j = 0; j < NO; ++j) s[(3 + NC + j) * M + i] = 0.0;
    }
}

// GPK_FN_REDUCE_STORE with a run-time mask over the NF accumulated rows: row k is stored when bit k of `mask` is set, at the output row
// given by the number of set bits below it; the reduction itself is that of the shared macro, operation by operation
#define GPK_FN_REDUCE_STORE_MASKED(s, NF, mask, t0, Nt, out, ldo)                                                          \
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
            if (t < (Nt) && (((mask) >> k) & 1))                                                                           \
                (out)[(long)__popc((unsigned)((mask) & ((1 << k) - 1))) * (ldo) + t] =                                     \
                    (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);             \
        }                                                                                                                  \
    } while (0)

// precisions, packed points and coefficients (the handle's point scratch: 17 arrays of Nd + Nb, re-packed by every call)
inline int fill_common_op3(gpk_handle h, const char* who, const char* who_kernel, int kernel, const double* kp, const double* Xd, int Nd,
                           const double* Xb, int Nb, const double* op, const double* bc, double (&p)[3], const double** s) {
    if (Nd <= 0 || Nb < 0 || !kp || !Xd || (Nb > 0 && !Xb)) return gpk_bad_arg(h, who);
    GPK_TRY(precisions(h, who_kernel, kernel, kp, 3, p));
    const size_t Mall = (size_t)Nd + (size_t)Nb;
    GPK_TRY(gpk_i_ensure_points(h, NARR * Mall));
    *s = h->d_pts;
    pack_op3_kernel<<<gpk_ceil_div((int)Mall, 256), 256, 0, h->stream>>>(Xd, Nd, Xb, Nb, op, bc, h->d_pts);
    GPK_LAUNCH_CHECK(h);
    return 0;
}

// <psi, psi> at d = 0 (h0 = 1, h2 = -p, h4 = 3 p^2, odd orders vanish):
//   c0^2 + sum_k p_k b_k^2 + 3 sum_k p_k^2 a_kk^2 + sum_{k<l} p_k p_l (a_kl^2 + 2 a_kk a_ll) - 2 c0 sum_k p_k a_kk
inline long double psi3_diag(const double* o, const long double (&q)[3]) {
    const long double c0 = o[0], b[3] = {o[1], o[2], o[3]}, akk[3] = {o[4], o[7], o[9]};
    const long double a12 = o[5], a13 = o[6], a23 = o[8];
    long double v = c0 * c0;
    for (int k = 0; k < 3; ++k) v += q[k] * b[k] * b[k];
    for (int k = 0; k < 3; ++k) v += 3.0L * q[k] * q[k] * akk[k] * akk[k];
    v += q[0] * q[1] * (a12 * a12 + 2.0L * akk[0] * akk[1]);
    v += q[0] * q[2] * (a13 * a13 + 2.0L * akk[0] * akk[2]);
    v += q[1] * q[2] * (a23 * a23 + 2.0L * akk[1] * akk[2]);
    v -= 2.0L * c0 * (q[0] * akk[0] + q[1] * akk[1] + q[2] * akk[2]);
    return v;
}

// sum_i <psi_i, psi_i>(0) over the Nd domain functionals op3 (device, (Nd,10); NULL: the Laplacian at every point), on the host from the
// coefficient array, in index order and in long double: a trace ratio built on it is the analytic value to an ulp and the same on every
// call, and NULL and an explicit Laplacian give the same sum.  Synchronises the stream when op3 != NULL.
inline int domain_trace3(gpk_handle h, const double* op3, int Nd, const long double (&q)[3], long double* tr) {
    long double tr0 = 0.0L;
    if (op3) {
        std::vector<double> ho(NO * (size_t)Nd);
        GPK_HIP(h, hipMemcpyAsync(ho.data(), op3, ho.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        GPK_HIP(h, hipStreamSynchronize(h->stream));
        for (int i = 0; i < Nd; ++i) tr0 += psi3_diag(ho.data() + NO * (size_t)i, q);
    } else {
        const double lap[NO] = {0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0};
        const long double v = psi3_diag(lap, q);
        for (int i = 0; i < Nd; ++i) tr0 += v;
    }
    *tr = tr0;
    return 0;
}

}  // namespace
}  // namespace gpk_asm
