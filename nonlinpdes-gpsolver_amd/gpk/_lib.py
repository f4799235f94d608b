"""Loader and prototypes for libgpk.so (the product: include/gpk.h, gpk_mg.h, gpk_debug.h) and libgpk_dev.so (the development build:
the same plus include/gpk_dev.h -- superseded kernel variants, probes, micro-benchmarks; loaded only on request, by tests and tools)."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(os.path.dirname(_HERE), 'csrc', 'libgpk.so')
_DEV_LIB_PATH = os.path.join(os.path.dirname(_HERE), 'csrc', 'libgpk_dev.so')


class GpkError(RuntimeError):
    pass


class GNProblemStruct(C.Structure):
    _fields_ = [('system', C.c_int), ('Nd', C.c_int), ('Nb', C.c_int), ('Ndata', C.c_int),
                ('p0', C.c_double), ('p1', C.c_double), ('pen_lambda', C.c_double),
                ('rhs_f', C.c_void_p), ('bdy_g', C.c_void_p), ('data_u', C.c_void_p),
                ('L', C.c_void_p), ('ldl', C.c_int), ('L2', C.c_void_p), ('ldl2', C.c_int),
                ('Dinv', C.c_void_p), ('Dinv2', C.c_void_p), ('dinv_block', C.c_int),
                ('W1', C.c_void_p), ('W2', C.c_void_p), ('v0', C.c_void_p), ('ldw', C.c_int),
                ('G', C.c_void_p), ('ldg', C.c_int), ('pvec', C.c_void_p),
                ('Wa', C.c_void_p), ('ldwa', C.c_int), ('Ha', C.c_void_p), ('ldha', C.c_int),
                ('gq_a1', C.c_double), ('gq_a2', C.c_double), ('gq_b', C.c_double), ('gq_c1', C.c_double), ('gq_c3', C.c_double),
                ('nonlin', C.c_int), ('p2', C.c_double)]


class LSOptionsStruct(C.Structure):
    """gpk_ls_options: zeros mean the defaults 8, 1.0, 0.5, 1e-4"""
    _fields_ = [('K', C.c_int), ('t0', C.c_double), ('beta', C.c_double), ('c1', C.c_double)]


_vp, _i, _d, _sz = C.c_void_p, C.c_int, C.c_double, C.c_size_t
_pi, _pd, _pvp = C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_void_p)
_pp = C.POINTER(GNProblemStruct)

# collective entry points of include/gpk_mg.h: exactly the signatures of ncclBroadcast / ncclAllGather
MG_BCAST_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p)
MG_ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p)
# ncclSend / ncclRecv / ncclGroupStart / ncclGroupEnd (the direct exchange of the sharded step)
MG_SEND_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p)
MG_RECV_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p)
MG_GROUP_FN = C.CFUNCTYPE(C.c_int)

# name -> (restype, argtypes); one entry per function of include/gpk.h, include/gpk_mg.h and include/gpk_debug.h
PROTOTYPES = {
    'gpk_mg_create': (_i, [_vp, _i, _i, _i, _pvp]),
    'gpk_mg_destroy': (_i, [_vp]),
    'gpk_mg_set_comm': (_i, [_vp, _vp, MG_BCAST_FN, MG_ALLGATHER_FN]),
    'gpk_mg_set_p2p': (_i, [_vp, MG_SEND_FN, MG_RECV_FN, MG_GROUP_FN, MG_GROUP_FN]),
    'gpk_mg_has_p2p': (_i, [_vp]),
    'gpk_mg_preflight_p2p': (_i, [_vp, _sz, _i, _pd]),
    'gpk_mg_rccl_probe': (_i, [C.c_char_p, C.c_char_p, _i]),
    'gpk_mg_rccl_unique_id': (_i, [C.c_char_p, _vp]),
    'gpk_mg_rccl_init': (_i, [_vp, C.c_char_p, _vp]),
    'gpk_mg_set_option': (_i, [_vp, _i, _i]),
    'gpk_mg_selftest': (_i, [_vp, _pi]),
    'gpk_mg_preflight': (_i, [_vp, _sz, _i, _pd, _pd, _pi]),
    'gpk_mg_potrf': (_i, [_vp, _vp, _i, _i, _pi]),
    'gpk_mg_gn_step': (_i, [_vp, _pp, _vp, _d, _vp, _i, _vp, _vp, _i, _vp, _pd, _pi]),
    'gpk_mg_plan_potrf': (_i, [_i, _i, _i, _i, _i, _pi, _i, _pi]),
    'gpk_mg_column_bounds': (_i, [_i, _i, _i, _i, _i, _pi]),
    'gpk_create': (_i, [_i, _pvp]),
    'gpk_destroy': (_i, [_vp]),
    'gpk_last_error': (C.c_char_p, [_vp]),
    'gpk_version': (C.c_char_p, []),
    'gpk_set_stream': (_i, [_vp, _vp]),
    'gpk_synchronize': (_i, [_vp]),
    'gpk_device_info': (_i, [_vp, C.c_char_p, _i, _pi, C.POINTER(_sz), _pi]),
    'gpk_malloc': (_i, [_vp, _sz, _pvp]),
    'gpk_free': (_i, [_vp, _vp]),
    'gpk_memset': (_i, [_vp, _vp, _i, _sz]),
    'gpk_memcpy_h2d': (_i, [_vp, _vp, _vp, _sz]),
    'gpk_memcpy_d2h': (_i, [_vp, _vp, _vp, _sz]),
    'gpk_memcpy_d2d': (_i, [_vp, _vp, _vp, _sz]),
    'gpk_memcpy2d_h2d': (_i, [_vp, _vp, _sz, _vp, _sz, _sz, _sz]),
    'gpk_memcpy2d_d2h': (_i, [_vp, _vp, _sz, _vp, _sz, _sz, _sz]),
    'gpk_memcpy2d_d2d': (_i, [_vp, _vp, _sz, _vp, _sz, _sz, _sz]),
    'gpk_timer_start': (_i, [_vp]),
    'gpk_timer_stop': (_i, [_vp, _pd]),
    'gpk_prof_enable': (_i, [_vp, _i]),
    'gpk_prof_read': (_i, [_vp, _pd, _pi]),
    'gpk_prof_read_pipeline': (_i, [_vp, _pi, _pd, _pi]),
    'gpk_prof_read_flops': (_i, [_vp, _pd, C.POINTER(C.c_long)]),
    'gpk_prof_read_assembly': (_i, [_vp, _pd]),
    'gpk_assemble': (_i, [_vp, _i, _i, _pd, _vp, _i, _vp, _i, _d, _i, _vp, _i, _pd]),
    'gpk_assemble_test': (_i, [_vp, _i, _i, _pd, _vp, _i, _vp, _i, _vp, _i, _vp, _i]),
    'gpk_extend': (_i, [_vp, _i, _i, _pd, _vp, _i, _vp, _i, _vp, _i, _vp, _vp]),
    'gpk_error_metrics': (_i, [_vp, _i, _vp, _vp, _vp, _pd, _pd]),
    'gpk_extend_functionals': (_i, [_vp, _i, _i, _pd, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _i]),
    'gpk_assemble3d': (_i, [_vp, _i, _pd, _vp, _i, _vp, _i, _d, _i, _vp, _i, _pd]),
    'gpk_extend_functionals3d': (_i, [_vp, _i, _pd, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _i]),
    'gpk_assemble_bc': (_i, [_vp, _i, _pd, _vp, _i, _vp, _i, _vp, _d, _i, _vp, _i, _pd]),
    'gpk_extend_functionals_bc': (_i, [_vp, _i, _pd, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _i, _vp, _i]),
    'gpk_assemble_op': (_i, [_vp, _i, _pd, _vp, _i, _vp, _i, _vp, _vp, _d, _i, _vp, _i, _pd]),
    'gpk_extend_functionals_op': (_i, [_vp, _i, _pd, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _i, _vp, _i]),
    'gpk_assemble_op3d': (_i, [_vp, _i, _pd, _vp, _i, _vp, _i, _vp, _vp, _d, _i, _vp, _i, _pd]),
    'gpk_extend_functionals_op3d': (_i, [_vp, _i, _pd, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _i, _vp, _i]),
    'gpk_assemble_hess': (_i, [_vp, _i, _pd, _vp, _i, _vp, _i, _d, _i, _vp, _i, _pd]),
    'gpk_extend_functionals_hess': (_i, [_vp, _i, _pd, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _i]),
    'gpk_assemble_disp': (_i, [_vp, _i, _pd, _vp, _i, _vp, _i, _d, _i, _vp, _i, _pd]),
    'gpk_extend_functionals_disp': (_i, [_vp, _i, _pd, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _i]),
    'gpk_assemble_evo': (_i, [_vp, _i, _pd, _pd, _vp, _i, _vp, _i, _vp, _d, _i, _vp, _i, _pd]),
    'gpk_extend_functionals_evo': (_i, [_vp, _i, _pd, _pd, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _i, _vp, _i]),
    'gpk_pde_residual_ma': (_i, [_vp, _i, _vp, _i, _vp, _vp]),
    'gpk_assemble_jet2': (_i, [_vp, _i, _pd, _vp, _i, _vp, _i, _d, _i, _vp, _i, _pd]),
    'gpk_extend_functionals_jet2': (_i, [_vp, _i, _pd, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _i]),
    'gpk_pde_residual_ql': (_i, [_vp, _i, _pd, _i, _vp, _i, _vp, _vp]),
    'gpk_assemble_grad3d': (_i, [_vp, _i, _pd, _vp, _i, _vp, _i, _vp, _vp, _d, _i, _vp, _i, _pd]),
    'gpk_extend_functionals_grad3d': (_i, [_vp, _i, _pd, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _i, _vp, _i]),
    'gpk_pde_residual_sl3d': (_i, [_vp, _pd, _i, _vp, _i, _vp, _vp, _vp]),
    'gpk_pde_residual': (_i, [_vp, _i, _pd, _i, _vp, _i, _vp, _i, _vp, _vp]),
    'gpk_pde_residual_nl': (_i, [_vp, _i, _pd, _i, _vp, _i, _vp, _vp]),
    'gpk_pde_residual_sl': (_i, [_vp, _d, _pd, _i, _vp, _i, _vp, _vp]),
    'gpk_potrf': (_i, [_vp, _vp, _i, _i, _pi]),
    'gpk_tril': (_i, [_vp, _vp, _i, _i]),
    'gpk_symmetrize_lower': (_i, [_vp, _vp, _i, _i]),
    'gpk_potrf_panel': (_i, [_vp, _vp, _i, _i, _i, _pi]),
    'gpk_potrf_panel_at': (_i, [_vp, _vp, _i, _i, _i, _i]),
    'gpk_info_reset': (_i, [_vp]),
    'gpk_info_read': (_i, [_vp, _pi]),
    'gpk_trsm': (_i, [_vp, _i, _vp, _i, _i, _vp, _i, _i]),
    'gpk_trsm_lz': (_i, [_vp, _vp, _i, _i, _vp, _i, _i, _i]),
    'gpk_trtri_diag': (_i, [_vp, _vp, _i, _i, _vp, _i]),
    'gpk_trsm_dinv': (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _i, _i, _vp, _i, _i]),
    'gpk_gemm_lz': (_i, [_vp, _i, _i, _i, _i, _d, _vp, _i, _vp, _i, _d, _vp, _i, _i]),
    'gpk_trsm_right_lt': (_i, [_vp, _vp, _i, _i, _vp, _i, _i]),
    'gpk_potrs': (_i, [_vp, _vp, _i, _i, _vp, _i, _i]),
    'gpk_gemm': (_i, [_vp, _i, _i, _i, _i, _i, _d, _vp, _i, _vp, _i, _d, _vp, _i]),
    'gpk_syrk': (_i, [_vp, _i, _i, _d, _vp, _i, _d, _vp, _i, _i]),
    'gpk_gn_dims': (_i, [_pp, _pi, _pi]),
    'gpk_gn_worksize': (_i, [_pp, _i, _pi, C.POINTER(_sz), C.POINTER(_sz), C.POINTER(_sz), C.POINTER(_sz)]),
    'gpk_gn_step': (_i, [_vp, _pp, _vp, _d, _vp, _i, _vp, _i, _vp, _pd, _pi]),
    'gpk_gn_direction': (_i, [_vp, _pp, _vp, _vp, _i, _vp, _i, _vp, _pd, _pd, _pi]),
    'gpk_gn_trial_worksize': (_i, [_pp, _i, _i, _pi, C.POINTER(_sz)]),
    'gpk_gn_trial_losses': (_i, [_vp, _pp, _vp, _vp, _pd, _i, _vp, _i, _vp, _pd]),
    'gpk_gn_trial_accept': (_i, [_vp, _i, _vp, _vp, _vp, _pd, _i, _d, _d, _d, _pi, _pd]),
    'gpk_gn_step_ls': (_i, [_vp, _pp, _vp, C.POINTER(LSOptionsStruct), _vp, _i, _vp, _i, _vp, _vp, _i, _pd, _pd, _pi, _pd, _pi]),
    'gpk_gn_structured_prepare': (_i, [_vp, _pp, _vp, _i, _vp, _vp, _vp, _i]),
    'gpk_gn_gram_prepare': (_i, [_vp, _pp, _vp, _i, _vp]),
    'gpk_gn_darcy_prepare': (_i, [_vp, _pp, _vp, _i, _vp, _i, _vp, _i]),
    'gpk_gn_build': (_i, [_vp, _pp, _vp, _vp, _i]),
    'gpk_gn_build_rev': (_i, [_vp, _pp, _vp, _vp, _i]),
    'gpk_axpy': (_i, [_vp, _i, _d, _vp, _vp]),
    'gpk_gn_loss': (_i, [_vp, _pp, _vp, _vp, _pd]),
    'gpk_gn_hessian_grad': (_i, [_vp, _pp, _vp, _vp, _i, _vp, _i, _vp]),
    'gpk_gn_measurement': (_i, [_vp, _pp, _vp, _vp]),
    'gpk_assemble_cross': (_i, [_vp, _i, _i, _pd, _vp, _i, _vp, _i, _vp, _i, _vp, _i]),
    'gpk_col_sumsq': (_i, [_vp, _vp, _i, _i, _i, _d, _vp, _vp]),
    'gpk_posterior_worksize': (_i, [_pp, _i, _i, _i, _i, _pi, _pi, _pi] + [C.POINTER(_sz)] * 5),
    'gpk_posterior_prepare': (_i, [_vp, _pp, _vp, _vp, _i, _vp, _i, _pi]),
    'gpk_posterior_variance': (_i, [_vp, _pp, _vp, _i, _vp, _i, _i, _vp, _i, _i, _vp, _i, _vp, _vp]),
    'gpk_assemble_prior': (_i, [_vp, _i, _pd, _vp, _i, _vp, _i, _vp, _i]),
    'gpk_posterior_covariance': (_i, [_vp, _pp, _vp, _i, _vp, _i, _i, _vp, _i, _i, _vp, _i, _vp, _i, _i]),
    'gpk_posterior_sample': (_i, [_vp, _vp, _i, _i, _d, _vp, _vp, _i, _i, _vp, _i, _pi]),
    'gpk_chol_logdet': (_i, [_vp, _vp, _i, _i, _pd, _pi]),
    'gpk_log_evidence': (_i, [_vp, _pp, _vp, _vp, _i, _vp, _i, _vp, _pd, _pi]),
    'gpk_tune': (_i, [_vp, _i, _i]),
}

# entry points that exist only in the development build libgpk_dev.so (include/gpk_dev.h)
DEV_PROTOTYPES = {
    'gpk_debug_stamps': (_i, [_vp, C.POINTER(C.c_ulonglong), _i]),
    'gpk_ubench_mfma_f64': (_i, [_vp, _i, _pd]),
    'gpk_ubench_hbm_write': (_i, [_vp, _sz, _i, _pd]),
    'gpk_ubench_latency': (_i, [_vp, _i, _pd]),
    'gpk_ubench_xcc_map': (_i, [_vp, _i, _i, _pi]),
    'gpk_ubench_cu_census': (_i, [_vp, _i, _i, _i, _pi]),
    'gpk_debug_gemm_dma': (_i, [_vp, _i, _i, _i, _vp, _i, _vp, _i, _vp, _i]),
    'gpk_debug_overlap_probe': (_i, [_vp, _vp, _i, _i, _vp, _i, _i, _vp, _i, _pd]),
    'gpk_debug_set_profile': (_i, [_vp, _i, _i, _pi, _pi, _pi, _pi, _i]),
    'gpk_debug_syrk_lz': (_i, [_vp, _i, _i, _d, _vp, _i, _d, _vp, _i, _i]),
    'gpk_debug_first_rows': (_i, [_vp, _pp, _pi, _pi]),
    'gpk_debug_step_mode': (_i, [_vp, _pp, _pi, _pi]),
    'gpk_debug_gn_trial_build': (_i, [_vp, _pp, _vp, _vp, _pd, _i, _vp, _i]),
    'gpk_debug_workspace_bytes': (_i, [_vp, C.POINTER(_sz)]),
}

_lib = None
_dev_lib = None


def library_path(dev=False):
    return _DEV_LIB_PATH if dev else _LIB_PATH


def declared_symbols(dev=False):
    return sorted(set(PROTOTYPES) | set(DEV_PROTOTYPES)) if dev else sorted(PROTOTYPES)


def load_library(dev=False):
    """dlopen libgpk.so (dev=True: libgpk_dev.so) and attach prototypes.  Raises GpkError when the library has not been built."""
    global _lib, _dev_lib
    if dev and _dev_lib is not None:
        return _dev_lib
    if not dev and _lib is not None:
        return _lib
    path = library_path(dev)
    if not os.path.exists(path):
        raise GpkError(f'{path} not found: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                       '(hipcc --offload-arch=gfx950); there is no CPU fallback')
    try:
        lib = C.CDLL(path)
    except OSError as e:
        raise GpkError(f'cannot load {path}: {e}') from e
    protos = dict(PROTOTYPES, **DEV_PROTOTYPES) if dev else PROTOTYPES
    for name, (res, args) in protos.items():
        fn = getattr(lib, name)          # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    # development aid: GPK_DEBUG_SET="6=0,0=1" -> gpk_tune(handle, key, value) on every Context created in this process (A/B runs of
    # bench.py).  The LIBRARY has no process-wide switches since round 4 (gpk_tune is per handle); what is process-wide here is this
    # Python-side table of defaults, and `lib.gpk_debug_set(key, value)` -- the call the tests and tools have always used -- is a Python
    # function attached to the loaded library object that records the pair and applies it to every live Context.
    for kv in filter(None, os.environ.get('GPK_DEBUG_SET', '').split(',')):
        k, v = kv.split('=')
        TUNE_DEFAULTS[int(k)] = int(v)
    lib.gpk_debug_set = debug_set
    if dev:
        _dev_lib = lib
    else:
        _lib = lib
    return lib


TUNE_DEFAULTS = {}                      # key -> value applied to every new Context (GPK_DEBUG_SET, debug_set)
LIVE_CONTEXTS = __import__('weakref').WeakSet()


def debug_set(key, value):
    """gpk_tune(handle, key, value) on every live Context, and on every Context created later in this process.  Returns 0, or the
    library's error code if a handle rejects the key."""
    TUNE_DEFAULTS[int(key)] = int(value)
    rc = 0
    for ctx in list(LIVE_CONTEXTS):
        if getattr(ctx, 'h', None):
            rc = ctx.lib.gpk_tune(ctx.h, int(key), int(value)) or rc
    return rc
