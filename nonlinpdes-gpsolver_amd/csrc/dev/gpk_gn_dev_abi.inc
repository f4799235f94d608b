// gpk_gn_dev_abi.inc -- development entry points that reach the leading-zero ("staircase") state of a handle (included in gpk_gn.hip
// under -DGPK_DEV): tests/test_gpu_staircase.py drives every consumer of a profile with them.  Declared in include/gpk_dev.h.

// the leading-zero state gpk_i_gn_layout_enter / gpk_i_gn_darcy_profile / the sharded step put on a handle: slope 1/lead_div of the closed
// form, or a GpkStair of nseg segments (arrays of nseg ints), B's column 0 at column `base` of the profile's frame (stair_base for the
// solve, stair_col0 for a product).  nseg = 0 with lead_div = 1 resets it (gpk_i_gn_layout_leave).  gpk_trsm_dinv moves stair_col0 /
// stair_row0 while it runs: set the profile again before the next consumer.
extern "C" int gpk_debug_set_profile(gpk_handle h, int lead_div, int nseg, const int* c1, const int* a, const int* b, const int* sd, int base) {
    if (!h) return GPK_ERR_ARG;
    if (lead_div < 1 || nseg < 0 || nseg > 4 || base < 0 || (nseg > 0 && (!c1 || !a || !b || !sd)))
        return gpk_bad_arg(h, "debug_set_profile: lead_div >= 1, 0 <= nseg <= 4, base >= 0, segment arrays");
    GpkStair st;
    st.nseg = nseg;
    for (int s = 0; s < nseg; ++s) {
        if (sd[s] < 1 || (s > 0 && c1[s] < c1[s - 1])) return gpk_bad_arg(h, "debug_set_profile: sd >= 1, c1 non-decreasing");
        st.c1[s] = c1[s]; st.a[s] = a[s]; st.b[s] = b[s]; st.sd[s] = sd[s];
    }
    gpk_i_gn_layout_leave(h);
    h->stair = st;
    h->lead_div = lead_div;
    h->stair_base = base; h->stair_col0 = base; h->stair_row0 = 0;
    return 0;
}

// the lower-triangular leading-zero product that forms Hb = S^T S in gpk_gn_step (C <- alpha A^T A + beta C, lower tiles only; A is k x n,
// column c zero above the handle's profile / the closed form (lead, lead_div))
extern "C" int gpk_debug_syrk_lz(gpk_handle h, int n, int k, double alpha, const double* A, int lda, double beta, double* C, int ldc, int lead) {
    if (!h || !A || !C || n < 0 || k < 0 || lda < n || ldc < n) return GPK_ERR_ARG;
    return gpk_i_gemm(h, true, false, n, n, k, alpha, A, lda, A, lda, beta, C, ldc, true, lead > 0 ? lead : 0);
}

// first_row(c), c < n_z, under the layout gpk_gn_step enters for host_prob -> out_u (n_z ints); Darcy: the u-part's profile, and in out_a
// (may be null) the a-part's closed form on its columns [N_d, 4 N_d) (3 N_d = the column has no non-zero in the a-part rows).  Returns the
// layout (gpk_i_gn_layout: 1 elliptic systems, 2 Eikonal, 3 Burgers, 4 Darcy); the dense schedule (0) is refused.  The handle's
// leading-zero state is reset on return.
extern "C" int gpk_debug_first_rows(gpk_handle h, const gpk_gn_problem* p, int* out_u, int* out_a) {
    if (!h || !p || !out_u) return GPK_ERR_ARG;
    int nz = 0, rows = 0;
    GPK_TRY(gpk_i_gn_dims(h, p, &nz, &rows));
    const int rev = gpk_i_gn_layout(h, p);
    if (rev == 0) return gpk_bad_arg(h, "debug_first_rows: this problem runs the dense schedule (no leading-zero layout)");
    gpk_i_gn_layout_enter(h, p, rev);
    if (rev == 4) gpk_i_gn_darcy_profile(h, p->Nd);
    for (int c = 0; c < nz; ++c) out_u[c] = gpk_i_gn_first_row(h, nz, c);
    if (rev == 4 && out_a) {
        const int Nd = p->Nd;
        h->stair = GpkStair();                                       // (the a-part's closed form, lead = 3 N_d on the sub-range)
        for (int c = 0; c < nz; ++c) out_a[c] = (c >= Nd && c < 4 * Nd) ? gpk_i_gn_first_row(h, 3 * Nd, c - Nd) : 3 * Nd;
    }
    gpk_i_gn_layout_leave(h);
    return rev;
}
