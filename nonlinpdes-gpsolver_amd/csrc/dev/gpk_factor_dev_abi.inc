// gpk_factor_dev_abi.inc -- development entry points that need the internals of gpk_factor.hip (included there under -DGPK_DEV):
// shader-clock stamps of the diagonal-block kernels and the stream-overlap probe of round 1.  Declared in include/gpk_dev.h.

extern "C" int gpk_debug_stamps(gpk_handle h, unsigned long long* host16, int enable) {
    if (!h) return GPK_ERR_ARG;
    h->tune.dbg = enable;
    if (host16) GPK_HIP(h, hipMemcpyFromSymbol(host16, HIP_SYMBOL(gpk_dbg_stamps), 16 * sizeof(unsigned long long)));
    return 0;
}

// development probe: does a big GEMM on a low-priority side stream hide behind the latency-bound Cholesky panel chain?
// Runs  C2 <- S^T S  (n x n, k rows) on a side stream while  potrf(H)  runs on the handle's stream; returns the three
// times in ms: potrf alone, syrk alone, both concurrently (wall).
extern "C" int gpk_debug_overlap_probe(gpk_handle h, double* H, int n, int ldh, const double* S, int k, int lds, double* C2, int ldc,
                                       double* host_ms3) {
    if (!h || !H || !S || !C2 || !host_ms3) return GPK_ERR_ARG;
    hipStream_t side = nullptr, main_s = h->stream, chain = nullptr;
    GpkStreamScope scope(h);                                         // (the handle's stream goes back on every way out; the workspace flag stays as it is)
    const bool owner = h->ws_owner;
    int lo = 0, hi = 0;
    GPK_HIP(h, hipDeviceGetStreamPriorityRange(&lo, &hi));
    if (h->tune.probe_chain_cus > 0) {
        // spatial partition: the chain (potrf) stream gets the first h->tune.probe_chain_cus bits of the CU mask (bit i -> XCD i % 8 on
        // this chip, so a multiple of 8 takes the same number of CUs from every XCD), the GEMM stream gets the rest
        uint32_t ma[8] = {0, 0, 0, 0, 0, 0, 0, 0}, mb[8];
        for (int i = 0; i < h->tune.probe_chain_cus && i < 256; ++i) ma[i >> 5] |= 1u << (i & 31);
        for (int i = 0; i < 8; ++i) mb[i] = ~ma[i];
        GPK_HIP(h, hipExtStreamCreateWithCUMask(&chain, 8, ma));
        GPK_HIP(h, hipExtStreamCreateWithCUMask(&side, 8, mb));
        main_s = chain;
        scope.use(chain, owner);
    } else
    GPK_HIP(h, hipStreamCreateWithPriority(&side, hipStreamNonBlocking, lo));
    hipEvent_t e0, e1, ef;
    GPK_HIP(h, hipEventCreate(&e0)); GPK_HIP(h, hipEventCreate(&e1)); GPK_HIP(h, hipEventCreateWithFlags(&ef, hipEventDisableTiming));
    double* Hc = nullptr;
    GPK_HIP(h, hipMalloc((void**)&Hc, (size_t)n * ldh * sizeof(double)));
    float ms = 0.f;
    for (int mode = 0; mode < 3; ++mode) {
        GPK_HIP(h, hipMemcpyAsync(Hc, H, (size_t)n * ldh * sizeof(double), hipMemcpyDeviceToDevice, main_s));
        GPK_HIP(h, hipStreamSynchronize(main_s));
        GPK_HIP(h, hipEventRecord(e0, main_s));
        if (mode == 1 || mode == 2) {
            GPK_HIP(h, hipStreamWaitEvent(side, e0, 0));
            scope.use(side, owner);
            int rc = gpk_i_gemm(h, true, false, n, n, k, 1.0, S, lds, S, lds, 0.0, C2, ldc, true);
            scope.use(main_s, owner);
            if (rc) return rc;
            GPK_HIP(h, hipEventRecord(ef, side));
        }
        if (mode == 0 || mode == 2) GPK_TRY(gpk_i_potrf(h, Hc, n, ldh, 0));
        if (mode == 1 || mode == 2) GPK_HIP(h, hipStreamWaitEvent(main_s, ef, 0));
        GPK_HIP(h, hipEventRecord(e1, main_s));
        GPK_HIP(h, hipEventSynchronize(e1));
        GPK_HIP(h, hipEventElapsedTime(&ms, e0, e1));
        host_ms3[mode] = ms;
    }
    GPK_HIP(h, hipFree(Hc));
    if (chain) GPK_HIP(h, hipStreamDestroy(chain));
    GPK_HIP(h, hipStreamDestroy(side));
    GPK_HIP(h, hipEventDestroy(e0)); GPK_HIP(h, hipEventDestroy(e1)); GPK_HIP(h, hipEventDestroy(ef));
    return 0;
}
