// gpk_assemble_periodic.hip -- the periodic kernel in the fused Gram evaluator of the reference layouts.
//
// The mathematics of the kernel and its policy; the kernels are the frames of gpk_assemble_frames.h -- one-point and two-point Gram
// kernel, test rows, cross columns, prior, extension, multi-functional extension -- instantiated here and exported as a table
// (gpk_i_family_periodic, gpk_assemble_ref.h), through which the entry points of gpk_assemble.hip launch them.  A translation unit of
// its own: nothing here is seen by the compiler when it generates the Gaussian or the Matern kernels, and the axes travel in an
// argument of their own (PerArgs, the tail of the frames), so the argument structs of those kernels do not change.
//
// Math (DESIGN.md §K "Periodic kernel").  The kernel is a product over the axes; an axis with period L > 0, w = 2 pi / L, has
//   kappa(d) = exp(-(2 p / w^2) sin^2(w d / 2)) = exp(-p d^2 / 2) (1 + O(w^2 d^2)),
// and with s = (p / w) sin w d, c = p cos w d the factors h_m = (-1)^m kappa^(m) / kappa (the sign convention of hermite_plain) are
//   h0 = 1, h1 = s, h2 = s^2 - c, h3 = s (s^2 - 3 c - w^2), h4 = s^4 - 6 s^2 c + 3 c^2 - 4 w^2 s^2 + w^2 c,
// which tend to the Hermite table as w -> 0; an axis with L = 0 keeps the Gaussian factor and the Hermite table.  An entry is
// pair_coeff(a, b) e with a, b the tables of the two axes and e the product of the two factors: as in gpk_assemble.hip, one exp per
// point pair feeds every block.
//
// Evaluation.  d = x - y, then sincospi(d / L) = (sin, cos)(w d / 2) with exact argument reduction -- odd / even in d to the bit and
// right for any |d|, images x + k L included -- then sin w d = 2 s_h c_h, cos w d = 1 - 2 s_h^2, and the exponent -(2 p / w^2) s_h^2.
// Whether an axis is periodic is a wave-uniform branch on a kernel argument (PerAxis::L), not a template parameter: the three
// combinations would triple the 4 x 31 instantiations of the extension kernels for a scalar compare per axis and pair, in kernels
// that are bound by their stores.
//
// Every kernel computes an entry with the same bits for the same point pair: the per-pair arithmetic is written with explicit fma and
// compiled without contraction (as the bc / op evaluators and the Matern family), so the 8-byte and the 16-byte store paths agree.
// Every term of an entry is odd or even in d to the bit, so Theta[i][j] and Theta[j][i] are the same bits.
#include "gpk_assemble_frames.h"

using namespace gpk_asm;

namespace {

// h[0..4] of one axis at d; returns z with kappa_axis = exp(-g z^2): sin(w d / 2), or d on an axis that is not periodic
__device__ __forceinline__ double axis_table(const PerAxis& k, double d, double (&h)[5]) {
#pragma clang fp contract(off)
    h[0] = 1.0;
    if (k.L > 0.0) {                                    // wave-uniform: a kernel argument
        double sh, ch;
        sincospi(d / k.L, &sh, &ch);                    // sin, cos of w d / 2
        const double sw = (2.0 * sh) * ch;              // sin w d
        const double cw = __builtin_fma(-2.0 * sh, sh, 1.0);   // cos w d
        const double s = k.pw * sw, c = k.p * cw;
        const double s2 = s * s;
        h[1] = s;
        h[2] = s2 - c;
        h[3] = s * ((s2 - 3.0 * c) - k.w2);
        h[4] = __builtin_fma(s2, (s2 - 6.0 * c) - 4.0 * k.w2, c * __builtin_fma(3.0, c, k.w2));
        return sh;
    }
    const double q = k.p * d;
    const double q2 = q * q;
    h[1] = q;
    h[2] = q2 - k.p;
    h[3] = q * (q2 - 3.0 * k.p);
    h[4] = __builtin_fma(q2, q2 - 6.0 * k.p, 3.0 * k.p * k.p);
    return d;
}

// the two tables and e = kappa of a point pair
__device__ __forceinline__ double pair_tables(const PerArgs& k, double d1, double d2, double (&a)[5], double (&b)[5]) {
#pragma clang fp contract(off)
    const double z1 = axis_table(k.ax[0], d1, a);
    const double z2 = axis_table(k.ax[1], d2, b);
    return exp(-__builtin_fma(k.ax[1].g * z2, z2, k.ax[0].g * z1 * z1));
}

// pair_coeff of gpk_assemble.hip without contraction
template <int FX, int FY>
__host__ __device__ __forceinline__ double pair_coeff_p(const double (&a)[5], const double (&b)[5]) {
#pragma clang fp contract(off)
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < f_count(FX); ++i) {
#pragma unroll
        for (int j = 0; j < f_count(FY); ++j) {
            const double t = a[f_a1(FX, i) + f_a1(FY, j)] * b[f_a2(FX, i) + f_a2(FY, j)];
            if ((f_a1(FX, i) + f_a2(FX, i)) & 1) s -= t; else s += t;
        }
    }
    return s;
}

// The policy (gpk_assemble_frames.h): the tables of the two axes and e, as the Gaussian family, without contraction.  The kernels take
// the axes beside their argument struct and do not read its p1, p2.
struct Periodic {
    struct State { double a[5], b[5], e; };
    static constexpr bool write_through = false;

    __device__ __forceinline__ static void eval(double, double, double d1, double d2, State& s, const PerArgs& k) {
        s.e = pair_tables(k, d1, d2, s.a, s.b);
    }
    __device__ __forceinline__ static void eval2(double p1, double p2, double d1a, double d2a, State& s0, double d1b, double d2b, State& s1,
                                                 const PerArgs& k) {
        eval(p1, p2, d1a, d2a, s0, k);
        eval(p1, p2, d1b, d2b, s1, k);
    }
    template <int FX, int FY>
    __host__ __device__ __forceinline__ static double entry(const State& s) {
#pragma clang fp contract(off)
        return pair_coeff_p<FX, FY>(s.a, s.b) * s.e;
    }
    // the extension kernels sum coefficient * c over the blocks and multiply by e once.  Without contraction in the multi-functional
    // kernel (weigh_fn): a mask and its single-bit calls accumulate a functional through the same roundings
    template <int FX, int FY>
    __device__ __forceinline__ static double scaled(const State& s, double c) {
#pragma clang fp contract(off)
        return pair_coeff_p<FX, FY>(s.a, s.b) * c;
    }
    __device__ __forceinline__ static double weigh(const State& s, double v) { return v * s.e; }
    __device__ __forceinline__ static double weigh_fn(const State& s, double v) {
#pragma clang fp contract(off)
        return v * s.e;
    }
    // Only e is used (h0 = 1), so the tables are dead code here.  e depends on d through squares alone (even in d to the bit), and at
    // d = 0 it is exp(-0) = 1.
    __device__ __forceinline__ static double prior(double p1, double p2, double d1, double d2, const PerArgs& k) {
        State s;
        eval(p1, p2, d1, d2, s, k);
        return entry<F_DELTA, F_DELTA>(s);
    }
    // the table of an axis at d = 0 is (1, 0, -p, 0, 3 p^2 + w^2 p)
    static void at_zero(double, double, State& s, const PerArgs& k) {
        const PerAxis& x = k.ax[0];
        const PerAxis& y = k.ax[1];
        s.a[0] = 1.0; s.a[1] = 0.0; s.a[2] = -x.p; s.a[3] = 0.0; s.a[4] = x.p * (3.0 * x.p + x.w2);
        s.b[0] = 1.0; s.b[1] = 0.0; s.b[2] = -y.p; s.b[3] = 0.0; s.b[4] = y.p * (3.0 * y.p + y.w2);
        s.e = 1.0;
    }

    template <class F> static void with(const KernelParams& k, F&& f) { f(Periodic{}, k.per); }
};

}  // namespace

const Family gpk_i_family_periodic = family_of<Periodic>();
