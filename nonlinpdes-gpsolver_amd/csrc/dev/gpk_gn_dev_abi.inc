// gpk_gn_dev_abi.inc -- development entry points that reach the leading-zero ("staircase") state of a handle (included in gpk_gn.hip
// under -DGPK_DEV): tests/test_gpu_staircase.py drives every consumer of a profile with them.  Declared in include/gpk_dev.h.

// The profile the development entry points that take a bare `lead` (gpk_gemm_lz, gpk_trsm_lz, gpk_trsm_dinv, gpk_debug_syrk_lz) hand to
// the building blocks as their GpkLz argument (gpk_debug_lz, gpk_common.h): slope 1/slope_div of the closed form, or a GpkStair of nseg
// segments (arrays of nseg ints) with the operands' column 0 at column `base` of its frame.  nseg = 0 with slope_div = 1 resets it.
// Kept in gpk_ctx::debug_profile, which no gpk_i_* function reads; a call never changes it.
extern "C" int gpk_debug_set_profile(gpk_handle h, int slope_div, int nseg, const int* c1, const int* a, const int* b, const int* sd, int base) {
    if (!h) return GPK_ERR_ARG;
    if (slope_div < 1 || nseg < 0 || nseg > 4 || base < 0 || (nseg > 0 && (!c1 || !a || !b || !sd)))
        return gpk_bad_arg(h, "debug_set_profile: slope divisor >= 1, 0 <= nseg <= 4, base >= 0, segment arrays");
    GpkStair st;
    st.nseg = nseg;
    for (int s = 0; s < nseg; ++s) {
        if (sd[s] < 1 || (s > 0 && c1[s] < c1[s - 1])) return gpk_bad_arg(h, "debug_set_profile: sd >= 1, c1 non-decreasing");
        st.c1[s] = c1[s]; st.a[s] = a[s]; st.b[s] = b[s]; st.sd[s] = sd[s];
    }
    h->debug_profile = GpkLz::piecewise(st);
    h->debug_profile.div = slope_div;
    h->debug_profile.col0 = nseg > 0 ? base : 0;
    return 0;
}

// the lower-triangular leading-zero product that forms Hb = S^T S in gpk_gn_step (C <- alpha A^T A + beta C, lower tiles only; A is k x n,
// column c zero above the profile of gpk_debug_set_profile / its closed form with `lead`)
extern "C" int gpk_debug_syrk_lz(gpk_handle h, int n, int k, double alpha, const double* A, int lda, double beta, double* C, int ldc, int lead) {
    if (!h || !A || !C || n < 0 || k < 0 || lda < n || ldc < n) return GPK_ERR_ARG;
    return gpk_i_gemm(h, true, false, n, n, k, alpha, A, lda, A, lda, beta, C, ldc, true, gpk_debug_lz(h, lead));
}

// first_row(c), c < n_z, under the layout gpk_gn_step enters for host_prob -> out_u (n_z ints); Darcy: the u-part's profile, and in out_a
// (may be null) the a-part's closed form on its columns [N_d, 4 N_d) (3 N_d = the column has no non-zero in the a-part rows).  Returns the
// layout (gpk_i_gn_layout: 1 elliptic systems, 2 Eikonal, 3 Burgers, 4 Darcy); the dense schedule (0) is refused.
extern "C" int gpk_debug_first_rows(gpk_handle h, const gpk_gn_problem* p, int* out_u, int* out_a) {
    if (!h || !p || !out_u) return GPK_ERR_ARG;
    int nz = 0, rows = 0;
    GPK_TRY(gpk_i_gn_dims(h, p, &nz, &rows));
    const int rev = gpk_i_gn_layout(h, p);
    if (rev == 0) return gpk_bad_arg(h, "debug_first_rows: this problem runs the dense schedule (no leading-zero layout)");
    const GpkLz lz = rev == 4 ? gpk_i_gn_darcy_u_profile(p->Nd) : gpk_i_gn_profile(h, p, rev);
    for (int c = 0; c < nz; ++c) out_u[c] = lz.first_row(c);
    if (rev == 4 && out_a) {
        const int Nd = p->Nd;
        const GpkLz lz_a = GpkLz::closed(3 * Nd);                    // (the a-part's closed form, lead = 3 N_d on the sub-range)
        for (int c = 0; c < nz; ++c) out_a[c] = (c >= Nd && c < 4 * Nd) ? lz_a.first_row(c - Nd) : 3 * Nd;
    }
    return rev;
}

// The mode gpk_gn_step would run host_prob in and the product that follows it, as ints in the order of StepMode / StepProduct (gpk_gn.hip).
// Asks the step's own selector after the step's own checks; launches nothing and dereferences no device pointer.
extern "C" int gpk_debug_step_mode(gpk_handle h, const gpk_gn_problem* p, int* mode, int* product) {
    if (!h || !mode || !product) return GPK_ERR_ARG;
    Dims d;
    GPK_TRY(check_prob(h, p, d));
    const int rev = step_layout(h, p);
    const StepMode m = select_mode(h, p, d, rev);
    *mode = (int)m;
    *product = (int)select_product(m, rev);
    return 0;
}

// The first launch of gpk_gn_trial_losses alone: W[:, k] <- F(z - host_t[k] delta), built and NOT solved (tests hold the accepted column
// against gpk_gn_measurement of the accepted iterate, bit for bit).
extern "C" int gpk_debug_gn_trial_build(gpk_handle h, const gpk_gn_problem* p, const double* z, const double* delta, const double* host_t, int K,
                                        double* W, int ldw) {
    if (!h || !z || !delta || !W) return GPK_ERR_ARG;
    Dims d;
    GPK_TRY(check_prob(h, p, d));
    TrialT ts;
    GPK_TRY(trial_steps(h, host_t, K, ts));
    if (ldw < K) return gpk_bad_arg(h, "debug_gn_trial_build: ldw < K");
    return trial_build(h, p, z, delta, ts, K, W, ldw);
}
