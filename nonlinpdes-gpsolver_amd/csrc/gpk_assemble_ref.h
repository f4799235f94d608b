// gpk_assemble_ref.h -- what the three translation units of the reference layouts share besides the kernel frames: gpk_assemble.hip (the
// Gaussian family, the host side of every entry point), gpk_assemble_matern.hip (the Matern family) and gpk_assemble_periodic.hip (the
// periodic kernel per axis).  The layouts, the argument structs of the kernels, the layout dispatch, and the description of a kernel
// family as the host sees it: its parameters (KernelParams, kernel_params) and its table of launch functions (Family).  The kernels
// are the frames of gpk_assemble_frames.h, instantiated by each file for its own family: each family is compiled on its own, so that
// nothing added for one changes the code generated for another.
#pragma once
#include "gpk_assemble_common.h"

namespace gpk_asm {

// layouts: functional of each Theta block and whether it lives on domain points only (0) or domain+boundary (1)
template <int LAYOUT> struct Lay;
template <> struct Lay<GPK_LAYOUT_ELLIPTIC> { static constexpr int nb = 2; static constexpr int f[4] = {F_LAP, F_DELTA, 0, 0};          static constexpr int db[4] = {0, 1, 0, 0}; };
template <> struct Lay<GPK_LAYOUT_BURGERS>  { static constexpr int nb = 4; static constexpr int f[4] = {F_D1, F_D2, F_DD2, F_DELTA};   static constexpr int db[4] = {0, 0, 0, 1}; };
template <> struct Lay<GPK_LAYOUT_EIKONAL>  { static constexpr int nb = 4; static constexpr int f[4] = {F_D1, F_D2, F_LAP, F_DELTA};   static constexpr int db[4] = {0, 0, 0, 1}; };
template <> struct Lay<GPK_LAYOUT_DARCY_A>  { static constexpr int nb = 3; static constexpr int f[4] = {F_D1, F_D2, F_DELTA, 0};       static constexpr int db[4] = {0, 0, 0, 0}; };

// p1, p2: the precisions of the Gaussian family (gpk_assemble_common.h, precisions), the inverse length scales 1/rho_k of the Matern family
struct AsmArgs {
    const double* px; const double* py;   // SoA points: domain first, then boundary
    int Nd, M;                            // M = number of points visited (Nd+Nb, or Nd for DARCY_A)
    double p1, p2;
    double* out; long ld;
    int off[4]; int size[4];
    double nug[4];
    const double* tx; int Nt;             // test mode: (Nt,2) row-major test points
    const double* coeff;                  // extend mode
};

struct FnArgs {
    const double* px; const double* py;   // SoA column points (fill_common)
    int M;
    double p1, p2;
    int off[4]; int size[4];
    const double* tx; int Nt;
    const double* coeff;
    double* out; long ldo;
};

// the prior between two point sets (gpk_assemble_prior): out[i * ld + j] = k(xa_i, xb_j), both (n, 2) row-major; p1, p2 as in AsmArgs
struct PriorArgs {
    const double* xa; int na;
    const double* xb; int nb;
    double p1, p2;
    double* out; long ld;
};

constexpr int CROSS_TP = 8;               // column points per workgroup: the grid is N_t / 512 wide, so the rows supply the parallelism

// f(std::integral_constant<int, L>) for the layout id: the one place that turns it into a template argument; false: not a layout
template <class F>
bool with_layout(int layout, F&& f) {
    switch (layout) {
        case GPK_LAYOUT_ELLIPTIC: f(std::integral_constant<int, GPK_LAYOUT_ELLIPTIC>{}); return true;
        case GPK_LAYOUT_BURGERS:  f(std::integral_constant<int, GPK_LAYOUT_BURGERS>{}); return true;
        case GPK_LAYOUT_EIKONAL:  f(std::integral_constant<int, GPK_LAYOUT_EIKONAL>{}); return true;
        case GPK_LAYOUT_DARCY_A:  f(std::integral_constant<int, GPK_LAYOUT_DARCY_A>{}); return true;
        default: return false;
    }
}

// ---- the Matern family (DESIGN.md §K "Matern kernels"): nu = m + 1/2 ------------------------------------------------------------------
// m of a kernel id (2, 3, 4), 0: not a Matern id
inline int matern_order(int kernel) {
    return kernel == GPK_KERNEL_MATERN52 ? 2 : (kernel == GPK_KERNEL_MATERN72 ? 3 : (kernel == GPK_KERNEL_MATERN92 ? 4 : 0));
}

// inverse length scales r[k] = 1 / rho_k of host_kparams = {rho_1, rho_2}
inline int matern_scales(gpk_handle h, const double* kp, double (&r)[2]) {
    for (int k = 0; k < 2; ++k) {
        if (!(kp[k] > 0.0) || !(kp[k] <= 1.79769313486231570e308)) return gpk_bad_arg(h, "assemble: a Matern kernel needs two finite length scales > 0");
        r[k] = 1.0 / kp[k];
    }
    return 0;
}

// ---- the periodic kernel (DESIGN.md §K "Periodic kernel"): kappa_k(d) = exp(-(2 p_k / w_k^2) sin^2(w_k d / 2)), w_k = 2 pi / L_k -------
// One axis of the product kernel, as the periodic kernels read it.  L = 0: the Gaussian factor exp(-p d^2 / 2) and the Hermite table
// (w2 = pw = 0, g = p / 2); L > 0: the periodic factor, exponent -g sin^2(w d / 2).  Passed to the kernels beside AsmArgs / FnArgs /
// PriorArgs (the variadic tail of the frames), which therefore stay as the Gaussian and the Matern kernels know them.
struct PerAxis {
    double p;                             // precision 2 / sigma^2
    double L;                             // period, 0: not periodic
    double w2;                            // w^2
    double pw;                            // p / w
    double g;                             // factor of the exponent: 2 p / w^2, or p / 2
};
struct PerArgs { PerAxis ax[2]; };

// host_kparams = {sigma_1, sigma_2, L_1, L_2} -> the two axes; -9001 (and nothing launched) unless both sigma are finite and > 0, both
// periods finite and >= 0 and one of them > 0 (none: that is GPK_KERNEL_ANISOTROPIC)
inline int periodic_axes(gpk_handle h, const double* kp, PerArgs& k) {
    constexpr double big = 1.79769313486231570e308, two_pi = 6.28318530717958647692;
    for (int a = 0; a < 2; ++a) {
        const double sigma = kp[a], L = kp[2 + a];
        if (!(sigma > 0.0) || !(sigma <= big) || !(L >= 0.0) || !(L <= big))
            return gpk_bad_arg(h, "assemble: the periodic kernel needs two finite length scales > 0 and two finite periods >= 0");
        PerAxis& x = k.ax[a];
        x.p = 2.0 / (sigma * sigma); x.L = L;
        if (L > 0.0) { const double w = two_pi / L; x.w2 = w * w; x.pw = x.p / w; x.g = 2.0 * x.p / x.w2; }
        else { x.w2 = 0.0; x.pw = 0.0; x.g = 0.5 * x.p; }
    }
    if (!(k.ax[0].L > 0.0) && !(k.ax[1].L > 0.0))
        return gpk_bad_arg(h, "assemble: the periodic kernel with both periods 0 is the anisotropic Gaussian kernel: use its id");
    return 0;
}

// ---- a kernel family as the host sees it ------------------------------------------------------------------------------------------
// The launch functions of one family on stream st, for a valid layout id: each translation unit exports one table (family_of,
// gpk_assemble_frames.h).  gram: pairs as pairs_eligible, nt the store policy of gpk_tune key 55 (the write-through policies 2 / 3 exist
// for the Gaussian family only: plain elsewhere); cross, prior: wide as pairs_eligible; diag: c[b] = <f_b, f_b> at d = 0 for the blocks
// of the layout (SURVEY §8a-K last column: makes the adaptive trace ratios analytic).
struct KernelParams;
struct Family {
    void (*gram)(int layout, bool pairs, int nt, hipStream_t st, const AsmArgs& g, const KernelParams& k);
    void (*test)(int layout, hipStream_t st, const AsmArgs& g, const KernelParams& k);
    void (*cross)(int layout, bool wide, hipStream_t st, const AsmArgs& g, const KernelParams& k);
    void (*prior)(bool wide, hipStream_t st, const PriorArgs& g, const KernelParams& k);   // (no layout: the value functional on both sides)
    void (*extend)(int layout, hipStream_t st, const AsmArgs& g, const KernelParams& k);
    void (*extend_fn)(int layout, int mask, hipStream_t st, const FnArgs& g, const KernelParams& k);
    void (*diag)(int layout, const KernelParams& k, double (&c)[4]);
};

// the family parameters of a call: p the precisions (Gaussian, periodic) or the inverse length scales (Matern), the p1, p2 of the
// argument structs; m the Matern order (0: not Matern); per the axes of the periodic kernel (read by that family only)
struct KernelParams {
    const Family* family;
    double p[2];
    int m;
    PerArgs per;
};

}  // namespace gpk_asm

extern const gpk_asm::Family gpk_i_family_gauss;      // gpk_assemble.hip
extern const gpk_asm::Family gpk_i_family_matern;     // gpk_assemble_matern.hip
extern const gpk_asm::Family gpk_i_family_periodic;   // gpk_assemble_periodic.hip

namespace gpk_asm {

// (kernel id, host_kparams) -> the family and its parameters; an id that belongs to no family is reported as `who`
inline int kernel_params(gpk_handle h, const char* who, int kernel, const double* kp, KernelParams& k) {
    k = KernelParams{};
    if ((k.m = matern_order(kernel))) { k.family = &gpk_i_family_matern; return matern_scales(h, kp, k.p); }
    if (kernel == GPK_KERNEL_PERIODIC) {
        k.family = &gpk_i_family_periodic;
        GPK_TRY(periodic_axes(h, kp, k.per));
        k.p[0] = k.per.ax[0].p; k.p[1] = k.per.ax[1].p;
        return 0;
    }
    k.family = &gpk_i_family_gauss;
    return precisions(h, who, kernel, kp, 2, k.p);
}

}  // namespace gpk_asm
