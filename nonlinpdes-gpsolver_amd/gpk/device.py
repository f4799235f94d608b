"""Thin object layer over the C ABI: a context (handle + stream), device arrays with a padded leading dimension,
and the calls of include/gpk.h with numpy-friendly signatures."""
import ctypes as C
import os
import weakref

import numpy as np

from . import _lib as _libmod
from ._lib import GNProblemStruct, GpkError, load_library

LAYOUT = {'Nonlinear_elliptic': 0, 'Burgers': 1, 'Eikonal': 2, 'Darcy_u': 2, 'Darcy_a': 3}
KERNEL = {'Gaussian': 0, 'anisotropic_Gaussian': 1, 'Matern52': 8, 'Matern72': 9, 'Matern92': 10, 'periodic_Gaussian': 16}      # GPK_KERNEL_*
MATERN = ('Matern52', 'Matern72', 'Matern92')     # nu = 5/2, 7/2, 9/2: the reference layouts only (assemble .. assemble_cross)
PERIODIC = 'periodic_Gaussian'                    # (sigma_1, sigma_2, L_1, L_2), L_k = 0: axis k is not periodic; the reference layouts only
NUGGET = {'none': 0, 'identity': 1, 'adaptive': 2}
FUNCTIONAL = {'value': 1, 'd1': 2, 'd2': 4, 'd2d2': 8, 'laplacian': 16}      # GPK_FN_* bits of gpk_extend_functionals
FUNCTIONAL3D = {'value': 1, 'd1': 2, 'd2': 4, 'laplacian': 16, 'd3': 32}          # bits accepted by gpk_extend_functionals3d (GPK_FN_D3 = 32)
FUNCTIONAL_OP = {'value': 1, 'd1': 2, 'd2': 4, 'd11': 8, 'd12': 16, 'd22': 32}   # GPK_OPFN_* bits of gpk_extend_functionals_op
FUNCTIONAL_DISP = {'value': 1, 'd1': 2, 'd2': 4, 'd2d2': 8, 'd2d2d2': 64}         # bits accepted by gpk_extend_functionals_disp (GPK_FN_D2D2D2 = 64)
FUNCTIONAL_EVO = {'value': 1, 'd1': 2, 'd2': 4, 'd2d2': 8, 'q': 128}                # bits accepted by gpk_extend_functionals_evo (GPK_FN_Q = 128)
OP3_NAMES = ('value', 'd1', 'd2', 'd3', 'd11', 'd12', 'd13', 'd22', 'd23', 'd33')   # the monomials of op3, in its order
FUNCTIONAL_OP3 = {n: 1 << k for k, n in enumerate(OP3_NAMES)}                    # GPK_OP3FN_* bits of gpk_extend_functionals_op3d
DINV_BLOCK = int(__import__('os').environ.get('GPK_DINV_BLOCK', '0'))   # rows per inverted diagonal block of a factor (256 .. 2048); 0 = by size


def dinv_block_for(n):
    """Rows per inverted diagonal block for a factor of order n: GPK_DINV_BLOCK when set, else 1024, or 2048 from order 6000 on (the
    solve phase then has 5 instead of 9 triangular products at BASELINE config 2: 3.3 -> 3.15 ms per step; iterates agree with the
    substitution path to ~1e-12 there, tests/test_gpu_parity.py::test_trsm_dinv and DESIGN.md section 4 'Numerics') -- but never more
    than a quarter of the order (round 3, advisor): multiplying by an explicit inverse is only conditionally stable, and a block that
    is half the matrix (1024 rows at BASELINE config 1, order 1924) made the iterates differ from the substitution path by 3e-10
    instead of 3e-13.  Orders up to 1024 get 256-row blocks."""
    if DINV_BLOCK:
        return DINV_BLOCK
    db = 2048 if n >= 6000 else 1024
    while db > 256 and db > n // 4:
        db //= 2
    return db
SYSTEM = {'Nonlinear_elliptic': 0, 'Burgers': 1, 'Eikonal': 2, 'Darcy_flow2d': 3, 'Nonlinear_elliptic_relaxed': 4, 'Semilinear2d': 5,
          'MongeAmpere2d': 6, 'Semilinear3d': 7, 'Quasilinear2d': 9}
QL_KIND = {'mean_curvature': 0, 'p_laplace': 1, 'gauss_curvature': 2}             # GPK_QL_*: equation kind of the system 'Quasilinear2d'
NONLIN = {'power': 0, 'exp': 1, 'sinh': 2, 'sin': 3, 'cubic': 4}                  # GPK_NL_*: reaction term of the elliptic systems
EVIDENCE_TERMS = ('log_Z', 'J', 'logdet_theta', 'logdet_H', 'gamma_term', 'two_pi_term')   # host_terms[6] of gpk_log_evidence


def pad_ld(n, mult=16):
    """Leading dimension in elements: multiple of 16 doubles (128 B) so rows start on cache-line boundaries and the
    GEMM's 16-byte loads apply to every sub-block the recursion produces."""
    return ((int(n) + mult - 1) // mult) * mult


def kernel_params(kernel, kernel_parameter):
    if kernel == 'Gaussian':
        return (C.c_double * 2)(float(kernel_parameter), 0.0)
    if kernel == 'anisotropic_Gaussian':
        return (C.c_double * 2)(float(kernel_parameter[0]), float(kernel_parameter[1]))
    if kernel in MATERN:                                   # {rho_1, rho_2}: a scalar serves both axes
        kp = [float(v) for v in np.atleast_1d(np.asarray(kernel_parameter, dtype=np.float64))]
        if len(kp) not in (1, 2):
            raise ValueError(f'{kernel} needs one length scale or one per axis, got {len(kp)}')
        return (C.c_double * 2)(kp[0], kp[-1])
    if kernel == PERIODIC:                                 # {sigma_1, sigma_2, L_1, L_2}
        kp = [float(v) for v in np.atleast_1d(np.asarray(kernel_parameter, dtype=np.float64))]
        if len(kp) != 4:
            raise ValueError(f'{kernel} needs (sigma_1, sigma_2, L_1, L_2), got {len(kp)} value(s)')
        return (C.c_double * 4)(*kp)
    raise ValueError(f'unknown kernel {kernel!r}')


def require_gaussian_family(kernel, what):
    """The 3-D, boundary-functional and operator evaluators serve the Gaussian family only: say so before any device call."""
    if kernel in MATERN or kernel == PERIODIC:
        raise ValueError(f'{what}: the kernel {kernel!r} is available for the layouts Nonlinear_elliptic, Burgers, Eikonal and Darcy '
                         'only; the 3-D, boundary-functional and operator evaluators take Gaussian or anisotropic_Gaussian')


def kernel_params3d(kernel, kernel_parameter):
    """host_kparams of the 3-D calls: Gaussian {sigma}; anisotropic_Gaussian {sigma_1, sigma_2, sigma_3}"""
    require_gaussian_family(kernel, 'three space dimensions')
    if kernel == 'Gaussian':
        return (C.c_double * 3)(float(kernel_parameter), 0.0, 0.0)
    if kernel == 'anisotropic_Gaussian':
        kp = [float(v) for v in kernel_parameter]
        if len(kp) != 3:
            raise ValueError(f'anisotropic_Gaussian in three dimensions needs 3 length scales, got {len(kp)}')
        return (C.c_double * 3)(*kp)
    raise ValueError(f'unknown kernel {kernel!r}')


class DeviceArray:
    """Row-major float64 device buffer, (rows, cols) with leading dimension ld >= cols (vectors: cols == ld == 1)."""

    def __init__(self, ctx, rows, cols=1, ld=None, zero=False):
        self.ctx = ctx
        self.rows, self.cols = int(rows), int(cols)
        self.ld = int(ld) if ld is not None else (1 if self.cols == 1 else pad_ld(self.cols))
        self.nbytes = max(self.rows, 1) * self.ld * 8
        p = C.c_void_p()
        ctx._chk(ctx.lib.gpk_malloc(ctx.h, self.nbytes, C.byref(p)))
        self.ptr = p.value
        ctx._live.add(self)
        if zero:
            self.zero()

    def zero(self):
        self.ctx._chk(self.ctx.lib.gpk_memset(self.ctx.h, self.ptr, 0, self.nbytes))

    def upload(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        a2 = a.reshape(self.rows, self.cols)
        self.ctx._chk(self.ctx.lib.gpk_memcpy2d_h2d(self.ctx.h, self.ptr, self.ld * 8, a2.ctypes.data, self.cols * 8,
                                                    self.cols * 8, self.rows))
        return self

    def download(self, rows=None, cols=None, row0=0, col0=0):
        rows = self.rows - row0 if rows is None else rows
        cols = self.cols - col0 if cols is None else cols
        out = np.empty((rows, cols), dtype=np.float64)
        if rows and cols:
            src = self.ptr + (row0 * self.ld + col0) * 8
            self.ctx._chk(self.ctx.lib.gpk_memcpy2d_d2h(self.ctx.h, out.ctypes.data, cols * 8, src, self.ld * 8, cols * 8, rows))
        return out[:, 0] if (self.cols == 1 and cols == 1) else out

    def clone(self):
        """device-to-device copy (same shape and leading dimension)"""
        out = DeviceArray(self.ctx, self.rows, self.cols, self.ld)
        self.ctx._chk(self.ctx.lib.gpk_memcpy_d2d(self.ctx.h, out.ptr, self.ptr, self.nbytes))
        return out

    def at(self, row=0, col=0):
        return self.ptr + (row * self.ld + col) * 8

    def free(self):
        """Release the buffer.  Context.close() frees every array still alive, so after close() this is a no-op."""
        ptr, self.ptr = getattr(self, 'ptr', None), None
        if ptr and self.ctx.h:
            self.ctx._live.discard(self)
            self.ctx._chk(self.ctx.lib.gpk_free(self.ctx.h, ptr))

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class GNProblem:
    """Device-side description of one equation's Gauss-Newton system (gpk_gn_problem)."""

    def __init__(self, ctx, system, Nd, Nb, rhs_f, bdy_g, L, p0=0.0, p1=0.0, pen_lambda=0.0, data_u=None, L2=None, dinv=True, structured=False,
                 cache_a=None, nonlin=0, p2=0.0, gq=None, gq8=None):
        """nonlin, p2 (elliptic systems only): the reaction term tau(u) -- a GPK_NL_* id or its name in NONLIN -- with the parameters
        p0, p1, p2; 0 / 'power' is p0 u^p1, the reference's equation.  System 'Quasilinear2d': nonlin is the equation kind -- a GPK_QL_* id
        or its name in QL_KIND -- with the parameters p0, p1, p2.
        gq ('Semilinear2d' only): the coefficients (a1, a2, b, c1, c3) of N(u, grad u); p0 is eps there.
        gq8 ('Semilinear3d' only): the coefficients (a1, a2, a3, b1, b2, b3, c1, c3) of its N(u, grad u).  The struct has no fields of
        their own for a3, b2, b3: they travel in p0, p1, pen_lambda (include/gpk.h), so those three arguments must be left at 0.
        structured: False (default: the reference's operation sequence every step), True / 1 (prepare_structured), 2 (+ prepare_gram).
        cache_a (Darcy only): keep the iteration-independent a-part of the step (prepare_darcy: bit-identical iterates, less work per step);
        None = on unless GPK_DARCY_CACHE=0.
        dinv: also compute the inverses of the diagonal blocks of the factor(s) once (gpk_trtri_diag; True = blocks of
        dinv_block_for(order) rows, or 256 / 512 / 1024 / 2048), so that the solve S = L^{-1}[A | F] of every step runs as GEMMs only."""
        self.ctx = ctx
        self.keep = []
        def dev(v):
            v = np.asarray(v, dtype=np.float64).ravel()
            d = DeviceArray(ctx, max(v.size, 1)).upload(v) if v.size else DeviceArray(ctx, 1)
            self.keep.append(d)
            return d
        self.rhs_f, self.bdy_g = dev(rhs_f), dev(bdy_g)
        self.data_u = dev(data_u) if data_u is not None else None
        self.L, self.L2 = L, L2
        s = GNProblemStruct()
        s.system = SYSTEM[system] if isinstance(system, str) else int(system)
        s.Nd, s.Nb = int(Nd), int(Nb)
        s.Ndata = 0 if data_u is None else int(np.asarray(data_u).size)
        s.p0, s.p1, s.pen_lambda = float(p0), float(p1), float(pen_lambda)
        names = QL_KIND if s.system == SYSTEM['Quasilinear2d'] else NONLIN
        s.nonlin, s.p2 = (names[nonlin] if isinstance(nonlin, str) else int(nonlin)), float(p2)
        if gq is not None:
            gq = [float(v) for v in gq]
            if len(gq) != 5:
                raise ValueError(f'gq: the five coefficients (a1, a2, b, c1, c3), got {len(gq)}')
            s.gq_a1, s.gq_a2, s.gq_b, s.gq_c1, s.gq_c3 = gq
        if gq8 is not None:
            gq8 = [float(v) for v in gq8]
            if len(gq8) != 8:
                raise ValueError(f'gq8: the eight coefficients (a1, a2, a3, b1, b2, b3, c1, c3), got {len(gq8)}')
            if s.system != SYSTEM['Semilinear3d'] or gq is not None or (s.p0, s.p1, s.pen_lambda) != (0.0, 0.0, 0.0):
                raise ValueError("gq8: for the system 'Semilinear3d' only, without gq and with p0 = p1 = pen_lambda = 0 (they carry a3, b2, b3)")
            s.gq_a1, s.gq_a2, s.p0, s.gq_b, s.p1, s.pen_lambda, s.gq_c1, s.gq_c3 = gq8
        s.rhs_f, s.bdy_g = self.rhs_f.ptr, self.bdy_g.ptr
        s.data_u = self.data_u.ptr if self.data_u is not None else None
        s.L, s.ldl = L.ptr, L.ld
        s.L2, s.ldl2 = (L2.ptr, L2.ld) if L2 is not None else (None, 0)
        block = dinv_block_for(L.rows) if dinv is True else int(dinv)
        self.Dinv = ctx.trtri_diag(L, block=block) if dinv else None
        self.Dinv2 = ctx.trtri_diag(L2, block=block) if (dinv and L2 is not None) else None
        s.Dinv = self.Dinv.ptr if self.Dinv is not None else None
        s.Dinv2 = self.Dinv2.ptr if self.Dinv2 is not None else None
        s.dinv_block = block if dinv else 0
        self.struct = s
        nz, rows = C.c_int(), C.c_int()
        ctx._chk(ctx.lib.gpk_gn_dims(C.byref(s), C.byref(nz), C.byref(rows)))
        self.nz, self.rows = nz.value, rows.value
        self._S = self._H = self._delta = self._work = None
        self.W1 = self.W2 = self.v0 = self.G = self.pvec = None
        self.Wa = self.Ha = None
        self.darcy_prepare_ms = self.structured_prepare_ms = None
        if cache_a is None:
            cache_a = os.environ.get('GPK_DARCY_CACHE', '1') != '0'
        if cache_a and s.system == SYSTEM['Darcy_flow2d'] and dinv:
            self.prepare_darcy()
        if structured:
            self.prepare_structured()
            if int(structured) == 2:
                self.prepare_gram()

    def prepare_structured(self):
        """OPTIONAL: precompute the z-independent solves once (gpk_gn_structured_prepare).  Elliptic system: W1 = L^{-1}[I;0;0],
        W2 = L^{-1}[0;I;0], v0 = L^{-1}F(0); every later gn_step forms [L^{-1}A(z) | L^{-1}F(z)] = [W1 diag(d) + W2 | v0 + W1 a + W2 z]
        in one memory-bound pass instead of the triangular solve.  Burgers / Eikonal / Darcy (round 6): A(z) = A1 diag(d(z)) + A2 with
        constant 0/1 patterns, W1 = L^{-1}A1, W2 = L^{-1}A2; the step forms L^{-1}A(z) = W1 diag(d(z)) + W2 and solves only the F column.
        Not the reference's per-step operation sequence: opt-in."""
        import time
        if self.struct.system == SYSTEM['Nonlinear_elliptic_relaxed']:
            raise GpkError('structured solve: not available for the relaxed system')
        self.ctx.synchronize(); t0 = time.perf_counter()
        S, _, _, _ = self.workspace()
        ld = S.ld
        self.W1 = DeviceArray(self.ctx, self.rows, self.nz + 1, ld)
        self.W2 = DeviceArray(self.ctx, self.rows, self.nz + 1, ld)
        self.v0 = DeviceArray(self.ctx, self.rows)
        self.ctx._chk(self.ctx.lib.gpk_gn_structured_prepare(self.ctx.h, C.byref(self.struct), S.ptr, S.ld, self.W1.ptr, self.W2.ptr,
                                                             self.v0.ptr, ld))
        self.struct.W1, self.struct.W2, self.struct.v0, self.struct.ldw = self.W1.ptr, self.W2.ptr, self.v0.ptr, ld
        self.ctx.synchronize(); self.structured_prepare_ms = 1e3 * (time.perf_counter() - t0)

    def prepare_darcy(self):
        """Darcy: the a-part rows of GN_loss ([w1; w2; w0] against L_a, reference src/InverseProblems.py:137-146) do not involve z_old, so
        W_a = L_a^{-1} A_a and W_a^T W_a are the same in every step: computed once here with the step's own launches (gpk_gn_darcy_prepare),
        after which every gn_step skips that solve and that product.  Bit-identical iterates; 2 x (3 N_d)^2 doubles."""
        import time
        S, _, _, _ = self.workspace()
        na = 3 * self.struct.Nd
        ld = pad_ld(na)
        self.Wa = DeviceArray(self.ctx, na, na, ld)
        self.Ha = DeviceArray(self.ctx, na, na, ld)
        self.ctx.synchronize(); t0 = time.perf_counter()
        self.ctx._chk(self.ctx.lib.gpk_gn_darcy_prepare(self.ctx.h, C.byref(self.struct), S.ptr, S.ld, self.Wa.ptr, ld, self.Ha.ptr, ld))
        self.ctx.synchronize(); self.darcy_prepare_ms = 1e3 * (time.perf_counter() - t0)
        self.struct.Wa, self.struct.ldwa, self.struct.Ha, self.struct.ldha = self.Wa.ptr, ld, self.Ha.ptr, ld

    def prepare_gram(self):
        """OPTIONAL second level (needs prepare_structured): the Gram blocks G = [W1 W2]^T [W1 W2] and W^T v0 once
        (gpk_gn_gram_prepare); every later gn_step assembles the bordered matrix in O(nz^2) -- no solve, no product."""
        ldg = pad_ld(self.nz)
        self.G = DeviceArray(self.ctx, 4 * self.nz, self.nz, ldg)
        self.pvec = DeviceArray(self.ctx, 2 * self.nz + 1)
        self.ctx._chk(self.ctx.lib.gpk_gn_gram_prepare(self.ctx.h, C.byref(self.struct), self.G.ptr, ldg, self.pvec.ptr))
        self.struct.G, self.struct.ldg, self.struct.pvec = self.G.ptr, ldg, self.pvec.ptr

    def workspace(self):
        if self._S is None:
            ld = pad_ld(self.nz + 1)
            self._S = DeviceArray(self.ctx, self.rows, self.nz + 1, ld)
            self._H = DeviceArray(self.ctx, self.nz + 1, self.nz + 1, ld)
            self._delta = DeviceArray(self.ctx, self.nz)
            self._work = DeviceArray(self.ctx, self.rows)
        return self._S, self._H, self._delta, self._work

    def trial_workspace(self, K=16):
        """(W, ldw, dev_losses) for up to K trial steps of the line search (gpk_gn_trial_worksize); grown when a larger K is asked for"""
        K = int(K)
        if getattr(self, '_trial', None) is None or self._trial[3] < K:
            self.release_trial_workspace()
            ldw, nbytes = C.c_int(), C.c_size_t()
            rc = self.ctx.lib.gpk_gn_trial_worksize(C.byref(self.struct), K, 0, C.byref(ldw), C.byref(nbytes))
            if rc != 0:
                raise GpkError(f'gpk_gn_trial_worksize: {rc} (1 <= K <= 16, got {K})')
            self._trial = (DeviceArray(self.ctx, (nbytes.value + 7) // 8), ldw.value, DeviceArray(self.ctx, 16), K)
        return self._trial[:3]

    def release_trial_workspace(self):
        t, self._trial = getattr(self, '_trial', None), None
        if t is not None:
            t[0].free(); t[2].free()

    def release_workspace(self):
        self.release_trial_workspace()
        for a in (self._S, self._H, self._delta, self._work):
            if a is not None:
                a.free()
        self._S = self._H = self._delta = self._work = None

    def free(self):
        """Release everything this problem allocated (workspace, inverted diagonal blocks, the prepared operators of the structured modes,
        the cached Darcy a-part, its copies of the right-hand sides); the factors L / L2 belong to the caller.  The struct is inert afterwards."""
        self.release_workspace()
        for name in ('Dinv', 'Dinv2', 'W1', 'W2', 'v0', 'G', 'pvec', 'Wa', 'Ha'):
            a = getattr(self, name, None)
            if a is not None:
                a.free()
            setattr(self, name, None)
        for a in self.keep:
            a.free()
        self.keep = []
        s = self.struct
        s.Dinv = s.Dinv2 = s.W1 = s.W2 = s.v0 = s.G = s.pvec = s.Wa = s.Ha = None
        s.rhs_f = s.bdy_g = s.data_u = None


class Context:
    """One handle = one device + one stream.  Raises GpkError if the library or the device is missing."""

    def __init__(self, device=0, dev=False):
        """dev=True: the handle lives in libgpk_dev.so, the development build with the superseded kernel variants, probes and
        micro-benchmarks (include/gpk_dev.h) -- tests and tools only"""
        self.dev = bool(dev)
        self.lib = load_library(dev=self.dev)
        h = C.c_void_p()
        rc = self.lib.gpk_create(int(device), C.byref(h))
        if rc != 0:
            raise GpkError(f'gpk_create(device={device}) failed with {rc}: no usable gfx950 device '
                           '(this library has no CPU fallback)')
        self.h = h
        self._live = weakref.WeakSet()          # device arrays allocated through this context and not yet freed
        self.tune_rejected = {}
        for k, v in _libmod.TUNE_DEFAULTS.items():        # development switches in force for this process (GPK_DEBUG_SET / gpk.debug_set)
            if self.lib.gpk_tune(self.h, int(k), int(v)) != 0:
                # (a value that selects a superseded design while this handle lives in the product library, which does not contain it)
                self.tune_rejected[int(k)] = int(v)
                import warnings
                warnings.warn(f'gpk: tuning key {k} = {v} is not available in {"libgpk_dev.so" if self.dev else "libgpk.so"}; this handle keeps its default')
        _libmod.LIVE_CONTEXTS.add(self)

    def tune(self, key, value):
        """per-handle development / tuning switch (gpk_tune; keys: GpkTune in csrc/gpk_common.h, tools/README.md)"""
        self._chk(self.lib.gpk_tune(self.h, int(key), int(value)))

    def _chk(self, rc):
        if rc < 0:
            raise GpkError(f'libgpk error {rc}: {self.lib.gpk_last_error(self.h).decode()}')
        return rc

    def close(self):
        """Free every device array still alive (their handles become inert), then destroy the handle."""
        if getattr(self, 'h', None):
            for a in list(self._live):
                a.free()
            self.lib.gpk_destroy(self.h)
            self.h = None

    def synchronize(self):
        self._chk(self.lib.gpk_synchronize(self.h))

    def device_info(self):
        name = C.create_string_buffer(256)
        cus, clk, hbm = C.c_int(), C.c_int(), C.c_size_t()
        self._chk(self.lib.gpk_device_info(self.h, name, 256, C.byref(cus), C.byref(hbm), C.byref(clk)))
        return dict(name=name.value.decode(), compute_units=cus.value, hbm_bytes=hbm.value, clock_khz=clk.value)

    # ---- arrays ----
    def empty(self, rows, cols=1, ld=None):
        return DeviceArray(self, rows, cols, ld)

    def array(self, a):
        a = np.asarray(a, dtype=np.float64)
        if a.ndim == 1:
            return DeviceArray(self, a.size).upload(a)
        return DeviceArray(self, a.shape[0], a.shape[1]).upload(a)

    def points(self, X, dim=2):
        """(n,dim) point set, contiguous (ld = dim) as the C ABI expects (dim = 3: the *3d calls)"""
        X = np.ascontiguousarray(X, dtype=np.float64).reshape(-1, dim)
        return DeviceArray(self, max(X.shape[0], 1), dim, ld=dim).upload(X) if X.shape[0] else DeviceArray(self, 1, dim, ld=dim)

    def timer_start(self):
        self._chk(self.lib.gpk_timer_start(self.h))

    def timer_stop(self):
        ms = C.c_double()
        self._chk(self.lib.gpk_timer_stop(self.h, C.byref(ms)))
        return ms.value

    # ---- assembly ----
    def assemble(self, layout, kernel, kernel_parameter, Xd, Xb, nugget=0.0, nugget_type='none', out=None):
        Xd = np.ascontiguousarray(Xd, dtype=np.float64); Xb = np.ascontiguousarray(Xb, dtype=np.float64).reshape(-1, 2)
        Nd, Nb = Xd.shape[0], Xb.shape[0]
        lay = LAYOUT[layout]
        N = {0: 2 * Nd + Nb, 1: 4 * Nd + Nb, 2: 4 * Nd + Nb, 3: 3 * Nd}[lay]
        dXd, dXb = self.points(Xd), self.points(Xb)
        T = out if out is not None else DeviceArray(self, N, N)
        ratios = (C.c_double * 3)()
        self._chk(self.lib.gpk_assemble(self.h, lay, KERNEL[kernel], kernel_params(kernel, kernel_parameter),
                                        dXd.ptr, Nd, dXb.ptr, Nb, float(nugget), NUGGET[nugget_type], T.ptr, T.ld, ratios))
        self.synchronize()
        return T, list(ratios)

    def assemble_test(self, layout, kernel, kernel_parameter, Xt, Xd, Xb):
        Xt = np.ascontiguousarray(Xt, dtype=np.float64); Xd = np.ascontiguousarray(Xd, dtype=np.float64)
        Xb = np.ascontiguousarray(Xb, dtype=np.float64).reshape(-1, 2)
        Nt, Nd, Nb = Xt.shape[0], Xd.shape[0], Xb.shape[0]
        lay = LAYOUT[layout]
        N = {0: 2 * Nd + Nb, 1: 4 * Nd + Nb, 2: 4 * Nd + Nb, 3: 3 * Nd}[lay]
        dXt, dXd, dXb = self.points(Xt), self.points(Xd), self.points(Xb)
        out = DeviceArray(self, Nt, N)
        self._chk(self.lib.gpk_assemble_test(self.h, lay, KERNEL[kernel], kernel_params(kernel, kernel_parameter),
                                             dXt.ptr, Nt, dXd.ptr, Nd, dXb.ptr, Nb, out.ptr, out.ld))
        self.synchronize()
        return out

    def extend(self, layout, kernel, kernel_parameter, Xt, Xd, Xb, coeff):
        Xt = np.ascontiguousarray(Xt, dtype=np.float64); Xd = np.ascontiguousarray(Xd, dtype=np.float64)
        Xb = np.ascontiguousarray(Xb, dtype=np.float64).reshape(-1, 2)
        Nt, Nd, Nb = Xt.shape[0], Xd.shape[0], Xb.shape[0]
        dXt, dXd, dXb = self.points(Xt), self.points(Xd), self.points(Xb)
        dc = coeff if isinstance(coeff, DeviceArray) else self.array(coeff)
        out = DeviceArray(self, Nt)
        self._chk(self.lib.gpk_extend(self.h, LAYOUT[layout], KERNEL[kernel], kernel_params(kernel, kernel_parameter),
                                      dXt.ptr, Nt, dXd.ptr, Nd, dXb.ptr, Nb, dc.ptr, out.ptr))
        self.synchronize()
        return out

    def extend_functionals(self, layout, kernel, kernel_parameter, Xt, Xd, Xb, coeff, which=('value', 'd1', 'd2', 'laplacian')):
        """Derivatives of the extension at Xt (gpk_extend_functionals): a (len(which), Nt) DeviceArray, row k = functional which[k]
        (names: FUNCTIONAL; for Burgers d1 = d/dt, d2 = d/dx, d2d2 = d^2/dx^2).  coeff = Theta^{-1} sol_vec, as for extend()."""
        return self._extend_functionals('extend_functionals', FUNCTIONAL, 2, self.lib.gpk_extend_functionals, (LAYOUT[layout],),
                                        kernel, kernel_parameter, Xt, Xd, Xb, None, coeff, which)

    def _extend_functionals(self, name, table, dim, entry, lead, kernel, kernel_parameter, Xt, Xd, Xb, coeffs, coeff, which):
        """The four extend_functionals* calls: functional names `which` through `table` to the mask, points (n, dim) and the expansion
        coefficients to the device, the library `entry` (its arguments: handle, `lead`, kernel, points, the device arrays or None of
        coeffs(Nd, Nb), expansion coefficients, mask, output), then the rows from ascending bit order into the caller's order."""
        if name != 'extend_functionals':
            require_gaussian_family(kernel, name)
        which = tuple(which)
        bits = [table[w] for w in which]
        if len(set(bits)) != len(bits):
            raise ValueError(f'{name}: repeated functional in {which!r}')
        Xt, Xd, Xb = (np.ascontiguousarray(X, dtype=np.float64).reshape(-1, dim) for X in (Xt, Xd, Xb))
        Nt, Nd, Nb = Xt.shape[0], Xd.shape[0], Xb.shape[0]
        dXt, dXd, dXb = self.points(Xt, dim), self.points(Xd, dim), self.points(Xb, dim)
        held = coeffs(Nd, Nb) if coeffs else ()                               # (kept alive until the call has been issued)
        extra = [a.ptr if a is not None else None for a in held]
        dc = coeff if isinstance(coeff, DeviceArray) else self.array(coeff)
        mask = sum(bits)
        full = DeviceArray(self, len(bits), Nt, ld=Nt)                      # rows in ascending bit order
        kp = (kernel_params3d if dim == 3 else kernel_params)(kernel, kernel_parameter)
        self._chk(entry(self.h, *lead, KERNEL[kernel], kp, dXt.ptr, Nt, dXd.ptr, Nd, dXb.ptr, Nb, *extra, dc.ptr, mask, full.ptr, full.ld))
        order = sorted(bits)
        if bits == order:
            out = full
        else:                                                             # the caller's order
            out = DeviceArray(self, len(bits), Nt, ld=Nt)
            for k, b in enumerate(bits):
                self._chk(self.lib.gpk_memcpy_d2d(self.h, out.at(k), full.at(order.index(b)), Nt * 8))
        self.synchronize()
        return out

    def _assemble_blocks(self, entry, dim, kernel, kernel_parameter, Xd, Xb, coeffs, nugget, nugget_type, out, rows=2, nratios=None):
        """The Gram calls of the Gaussian-only layouts (assemble3d / assemble_bc / assemble_op / assemble_op3d: two blocks; assemble_hess,
        assemble_grad3d: `rows` rows per domain point, N = rows Nd + Nb): points (n, dim) to the device, the library `entry` (its
        arguments: handle, kernel, points, the device arrays or None of coeffs(Nd, Nb), nugget, Theta, ratios) -> (Theta, the trace ratio
        of the two-block layouts, or the list of the `nratios` ratios)."""
        require_gaussian_family(kernel, entry.__name__)
        Xd, Xb = (np.ascontiguousarray(X, dtype=np.float64).reshape(-1, dim) for X in (Xd, Xb))
        Nd, Nb = Xd.shape[0], Xb.shape[0]
        N = rows * Nd + Nb
        dXd, dXb = self.points(Xd, dim), self.points(Xb, dim)
        held = coeffs(Nd, Nb) if coeffs else ()                               # (kept alive until the call has been issued)
        extra = [a.ptr if a is not None else None for a in held]
        T = out if out is not None else DeviceArray(self, N, N)
        ratios = (C.c_double * (nratios or 1))()
        kp = (kernel_params3d if dim == 3 else kernel_params)(kernel, kernel_parameter)
        self._chk(entry(self.h, KERNEL[kernel], kp, dXd.ptr, Nd, dXb.ptr, Nb, *extra, float(nugget), NUGGET[nugget_type], T.ptr, T.ld, ratios))
        self.synchronize()
        return T, (list(ratios) if nratios else ratios[0])

    # ---- three space dimensions (gpk_assemble3d, gpk_extend_functionals3d) ----
    def assemble3d(self, kernel, kernel_parameter, Xd, Xb, nugget=0.0, nugget_type='none', out=None):
        """Gram matrix of the 3-D elliptic layout (Laplacian on Xd, delta on [Xd; Xb]; points (n,3)): (DeviceArray N x N with
        N = 2 Nd + Nb, trace ratio of block 0).  out: a DeviceArray to write into (any leading dimension >= N)."""
        return self._assemble_blocks(self.lib.gpk_assemble3d, 3, kernel, kernel_parameter, Xd, Xb, None, nugget, nugget_type, out)

    def extend_functionals3d(self, kernel, kernel_parameter, Xt, Xd, Xb, coeff, which=('value', 'd1', 'd2', 'd3', 'laplacian')):
        """Value / derivatives of the 3-D extension at Xt (gpk_extend_functionals3d): a (len(which), Nt) DeviceArray, row k = functional
        which[k] (names: FUNCTIONAL3D).  coeff = Theta^{-1} sol_vec (2 Nd + Nb values).  which = ('value',) is the plain extension."""
        return self._extend_functionals('extend_functionals3d', FUNCTIONAL3D, 3, self.lib.gpk_extend_functionals3d, (),
                                        kernel, kernel_parameter, Xt, Xd, Xb, None, coeff, which)

    # ---- boundary functionals: Neumann / Robin / mixed conditions for the 2-D elliptic layout (gpk_assemble_bc, gpk_extend_functionals_bc) ----
    def _boundary_coeffs(self, bc, Nb):
        """(Nb,3) coefficients (c0, c1, c2) of the boundary functionals on the device, or None (= NULL: all (1,0,0))"""
        return self._coeff_rows(bc, Nb, 3, 'boundary coefficients', ': (c0, c1, c2) per boundary point')

    def assemble_bc(self, kernel, kernel_parameter, Xd, Xb, bc, nugget=0.0, nugget_type='none', out=None):
        """Gram matrix of the 2-D elliptic layout with the functional bc[b] = (c0, c1, c2) -> c0 delta + c1 d/dx1 + c2 d/dx2 at boundary
        point b (bc = None: delta everywhere): (DeviceArray N x N with N = 2 Nd + Nb, trace ratio of block 0).  out: a DeviceArray to
        write into (any leading dimension >= N)."""
        return self._assemble_blocks(self.lib.gpk_assemble_bc, 2, kernel, kernel_parameter, Xd, Xb,
                                        lambda Nd, Nb: (self._boundary_coeffs(bc, Nb),), nugget, nugget_type, out)

    def extend_functionals_bc(self, kernel, kernel_parameter, Xt, Xd, Xb, bc, coeff, which=('value', 'd1', 'd2', 'laplacian')):
        """Value / derivatives of the extension under the boundary functionals bc at Xt (gpk_extend_functionals_bc): a (len(which), Nt)
        DeviceArray, row k = functional which[k] (names: FUNCTIONAL).  coeff = Theta^{-1} sol_vec with the Theta of assemble_bc."""
        return self._extend_functionals('extend_functionals_bc', FUNCTIONAL, 2, self.lib.gpk_extend_functionals_bc, (),
                                        kernel, kernel_parameter, Xt, Xd, Xb, lambda Nd, Nb: (self._boundary_coeffs(bc, Nb),), coeff, which)

    # ---- variable-coefficient operator on the domain points of the 2-D elliptic layout (gpk_assemble_op, gpk_extend_functionals_op) ----
    def _domain_coeffs(self, op, Nd):
        """(Nd,6) coefficients (c0, b1, b2, a11, a12, a22) of the domain functionals on the device, or None (= NULL: the Laplacian)"""
        return self._coeff_rows(op, Nd, 6, 'domain coefficients', ': (c0, b1, b2, a11, a12, a22) per domain point')

    def assemble_op(self, kernel, kernel_parameter, Xd, Xb, op, bc, nugget=0.0, nugget_type='none', out=None):
        """Gram matrix of the 2-D elliptic layout with the functional op[i] = (c0, b1, b2, a11, a12, a22) -> c0 delta + b1 d/dx1 +
        b2 d/dx2 + a11 d2/dx1^2 + a12 d2/dx1dx2 + a22 d2/dx2^2 at domain point i (op = None: the Laplacian) and bc[b] at boundary point b
        as in assemble_bc: (DeviceArray N x N with N = 2 Nd + Nb, trace ratio of block 0).  out: a DeviceArray to write into (any
        leading dimension >= N)."""
        return self._assemble_blocks(self.lib.gpk_assemble_op, 2, kernel, kernel_parameter, Xd, Xb,
                                        lambda Nd, Nb: (self._domain_coeffs(op, Nd), self._boundary_coeffs(bc, Nb)), nugget, nugget_type, out)

    def extend_functionals_op(self, kernel, kernel_parameter, Xt, Xd, Xb, op, bc, coeff, which=('value', 'd1', 'd2', 'd11', 'd12', 'd22')):
        """Value / derivatives up to order two of the extension under the domain functionals op and the boundary functionals bc at Xt
        (gpk_extend_functionals_op): a (len(which), Nt) DeviceArray, row k = functional which[k] (names: FUNCTIONAL_OP).
        coeff = Theta^{-1} sol_vec with the Theta of assemble_op."""
        return self._extend_functionals('extend_functionals_op', FUNCTIONAL_OP, 2, self.lib.gpk_extend_functionals_op, (),
                                        kernel, kernel_parameter, Xt, Xd, Xb,
                                        lambda Nd, Nb: (self._domain_coeffs(op, Nd), self._boundary_coeffs(bc, Nb)), coeff, which)

    # ---- Hessian layout: D = d11 - d22, M = 2 d12, Laplacian, delta (gpk_assemble_hess, gpk_extend_functionals_hess, gpk_pde_residual_ma) ----
    def assemble_hess(self, kernel, kernel_parameter, Xd, Xb, nugget=0.0, nugget_type='none', out=None):
        """Gram matrix of the Hessian layout (blocks D, M, Laplacian on Xd, delta on [Xd; Xb]): (DeviceArray N x N with N = 4 Nd + Nb,
        [trace(block k) / trace(block 3) for k = 0, 1, 2]).  out: a DeviceArray to write into (any leading dimension >= N)."""
        return self._assemble_blocks(self.lib.gpk_assemble_hess, 2, kernel, kernel_parameter, Xd, Xb, None, nugget, nugget_type, out,
                                     rows=4, nratios=3)

    def extend_functionals_hess(self, kernel, kernel_parameter, Xt, Xd, Xb, coeff, which=('value', 'd1', 'd2', 'd11', 'd12', 'd22')):
        """Value / derivatives up to order two of the extension on the Hessian layout at Xt (gpk_extend_functionals_hess): a
        (len(which), Nt) DeviceArray, row k = functional which[k] (names: FUNCTIONAL_OP).  coeff = Theta^{-1} sol_vec (4 Nd + Nb values)
        with the Theta of assemble_hess."""
        return self._extend_functionals('extend_functionals_hess', FUNCTIONAL_OP, 2, self.lib.gpk_extend_functionals_hess, (),
                                        kernel, kernel_parameter, Xt, Xd, Xb, None, coeff, which)

    # ---- dispersive layout: d_t, d_x, d_x^3, delta on (t, x) points (gpk_assemble_disp, gpk_extend_functionals_disp) ----
    def assemble_disp(self, kernel, kernel_parameter, Xd, Xb, nugget=0.0, nugget_type='none', out=None):
        """Gram matrix of the dispersive layout (blocks d_t, d_x, d_x^3 on Xd, delta on [Xd; Xb]; points (t, x)): (DeviceArray N x N
        with N = 4 Nd + Nb, [trace(block k) / trace(block 3) for k = 0, 1, 2]).  out: a DeviceArray to write into (any leading
        dimension >= N)."""
        return self._assemble_blocks(self.lib.gpk_assemble_disp, 2, kernel, kernel_parameter, Xd, Xb, None, nugget, nugget_type, out,
                                     rows=4, nratios=3)

    def extend_functionals_disp(self, kernel, kernel_parameter, Xt, Xd, Xb, coeff, which=('value', 'd1', 'd2', 'd2d2', 'd2d2d2')):
        """u, u_t, u_x, u_xx, u_xxx of the extension on the dispersive layout at Xt (gpk_extend_functionals_disp): a (len(which), Nt)
        DeviceArray, row k = functional which[k] (names: FUNCTIONAL_DISP).  coeff = Theta^{-1} sol_vec (4 Nd + Nb values) with the
        Theta of assemble_disp."""
        return self._extend_functionals('extend_functionals_disp', FUNCTIONAL_DISP, 2, self.lib.gpk_extend_functionals_disp, (),
                                        kernel, kernel_parameter, Xt, Xd, Xb, None, coeff, which)

    # ---- evolution layout: d_t, d_x, Q = sum c_k d_x^k, delta / boundary functionals on (t, x) points (gpk_assemble_evo, gpk_extend_functionals_evo) ----
    @staticmethod
    def _operator_c4(coeffs):
        c = np.asarray(coeffs, dtype=np.float64).ravel()
        if c.shape != (4,):
            raise ValueError(f'coeffs must be (c2, c3, c4, c5), got {coeffs!r}')
        return (C.c_double * 4)(*c)

    def _evo_entry(self, entry, coeffs, lead):
        """the library entry with host_c4 in its place behind host_kparams, in the argument order _assemble_blocks / _extend_functionals use"""
        c4 = self._operator_c4(coeffs)

        def call(h, *args):
            return entry(h, *args[:lead], c4, *args[lead:])
        call.__name__ = entry.__name__
        return call

    def assemble_evo(self, kernel, kernel_parameter, coeffs, Xd, Xb, bc=None, nugget=0.0, nugget_type='none', out=None):
        """Gram matrix of the evolution layout (blocks d_t, d_x, Q = c2 d_x^2 + c3 d_x^3 + c4 d_x^4 + c5 d_x^5 on Xd with coeffs =
        (c2, c3, c4, c5); block 3: delta on Xd, bc[b] = (c0, c1, c2) -> c0 delta + c1 d_t + c2 d_x at boundary point b, bc = None: delta;
        points (t, x)): (DeviceArray N x N with N = 4 Nd + Nb, [trace(block k) / trace(block 3) for k = 0, 1, 2]).  out: a DeviceArray
        to write into (any leading dimension >= N)."""
        return self._assemble_blocks(self._evo_entry(self.lib.gpk_assemble_evo, coeffs, 2), 2, kernel, kernel_parameter, Xd, Xb,
                                     lambda Nd, Nb: (self._boundary_coeffs(bc, Nb),), nugget, nugget_type, out, rows=4, nratios=3)

    def extend_functionals_evo(self, kernel, kernel_parameter, coeffs, Xt, Xd, Xb, bc, coeff, which=('value', 'd1', 'd2', 'd2d2', 'q')):
        """u, u_t, u_x, u_xx, Q[u] of the extension on the evolution layout at Xt (gpk_extend_functionals_evo): a (len(which), Nt)
        DeviceArray, row k = functional which[k] (names: FUNCTIONAL_EVO).  coeff = Theta^{-1} sol_vec (4 Nd + Nb values) with the
        Theta of assemble_evo (the same coeffs and bc)."""
        return self._extend_functionals('extend_functionals_evo', FUNCTIONAL_EVO, 2, self._evo_entry(self.lib.gpk_extend_functionals_evo, coeffs, 2),
                                        (), kernel, kernel_parameter, Xt, Xd, Xb, lambda Nd, Nb: (self._boundary_coeffs(bc, Nb),), coeff, which)

    def _on_device(self, a, fields=False):
        """a DeviceArray as it is; a host array uploaded as (rows, Nt) fields or as one vector"""
        if isinstance(a, DeviceArray):
            return a
        return self.array(np.atleast_2d(a) if fields else np.asarray(a, dtype=np.float64).ravel())

    def _pde_residual(self, entry, const, fields, rhs, more=()):
        """The five pde_residual* calls: the fields (rows, Nt) and the rhs to the device, the library `entry` (its arguments: handle, the
        constant block `const`, Nt, the fields and their leading dimension, the arguments `more`, rhs, output) -> the (Nt,) DeviceArray."""
        du = self._on_device(fields, fields=True)
        Nt = du.cols
        dr = self._on_device(rhs)
        out = DeviceArray(self, Nt)
        self._chk(entry(self.h, *const, Nt, du.ptr, du.ld, *more, dr.ptr, out.ptr))
        self.synchronize()
        return out

    def pde_residual_ma(self, fields, rhs):
        """Pointwise residual d11 d22 - d12^2 - f of the Monge-Ampere equation (gpk_pde_residual_ma), as an (Nt,) DeviceArray.
        fields: (3, Nt) d11, d12, d22 of the extension; rhs as for pde_residual."""
        return self._pde_residual(self.lib.gpk_pde_residual_ma, (), fields, rhs)

    # ---- 2-jet layout: d1, d2, D = d11 - d22, M = 2 d12, Laplacian, delta (gpk_assemble_jet2, gpk_extend_functionals_jet2, gpk_pde_residual_ql) ----
    def assemble_jet2(self, kernel, kernel_parameter, Xd, Xb, nugget=0.0, nugget_type='none', out=None):
        """Gram matrix of the 2-jet layout (blocks d1, d2, D, M, Laplacian on Xd, delta on [Xd; Xb]): (DeviceArray N x N with
        N = 6 Nd + Nb, [trace(block k) / trace(block 5) for k = 0..4]).  out: a DeviceArray to write into (any leading dimension >= N)."""
        return self._assemble_blocks(self.lib.gpk_assemble_jet2, 2, kernel, kernel_parameter, Xd, Xb, None, nugget, nugget_type, out,
                                     rows=6, nratios=5)

    def extend_functionals_jet2(self, kernel, kernel_parameter, Xt, Xd, Xb, coeff, which=('value', 'd1', 'd2', 'd11', 'd12', 'd22')):
        """Value / derivatives up to order two of the extension on the 2-jet layout at Xt (gpk_extend_functionals_jet2): a
        (len(which), Nt) DeviceArray, row k = functional which[k] (names: FUNCTIONAL_OP).  coeff = Theta^{-1} sol_vec (6 Nd + Nb values)
        with the Theta of assemble_jet2."""
        return self._extend_functionals('extend_functionals_jet2', FUNCTIONAL_OP, 2, self.lib.gpk_extend_functionals_jet2, (),
                                        kernel, kernel_parameter, Xt, Xd, Xb, None, coeff, which)

    def pde_residual_ql(self, kind, params, fields, rhs):
        """Pointwise residual of a quasilinear equation in its divergence / determinant form (gpk_pde_residual_ql), as an (Nt,)
        DeviceArray.  kind: a GPK_QL_* id or its name in QL_KIND; params = (p0, p1, p2); fields: (6, Nt) value, d1, d2, d11, d12, d22 of
        the extension; rhs as for pde_residual."""
        p = (C.c_double * 3)(*[float(v) for v in (list(params) + [0.0, 0.0, 0.0])[:3]])
        k = QL_KIND[kind] if isinstance(kind, str) else int(kind)
        return self._pde_residual(self.lib.gpk_pde_residual_ql, (k, p), fields, rhs)

    # ---- operator and boundary functionals in three dimensions (gpk_assemble_op3d, gpk_extend_functionals_op3d) ----
    def _coeff_rows(self, c, n, width, what, per_point=''):
        """(n, width) coefficient rows on the device (n = 0: a placeholder row), or None (= NULL: the library's default functional)"""
        if c is None:
            return None
        c = np.ascontiguousarray(c, dtype=np.float64)
        if c.shape != (n, width):
            raise ValueError(f'{what} must have shape ({n}, {width}){per_point}, got {c.shape}')
        return DeviceArray(self, n, width, ld=width).upload(c) if n else DeviceArray(self, 1, width, ld=width)

    def _coeffs3(self, op3, bc3):
        return lambda Nd, Nb: (self._coeff_rows(op3, Nd, 10, 'domain coefficients (c0, b1, b2, b3, a11, a12, a13, a22, a23, a33)'),
                               self._coeff_rows(bc3, Nb, 4, 'boundary coefficients (c0, c1, c2, c3)'))

    def assemble_op3d(self, kernel, kernel_parameter, Xd, Xb, op3, bc3, nugget=0.0, nugget_type='none', out=None):
        """Gram matrix of the 3-D elliptic layout with the functional op3[i] = (c0, b1, b2, b3, a11, a12, a13, a22, a23, a33) at domain
        point i (op3 = None: the Laplacian) and bc3[b] = (c0, c1, c2, c3) -> c0 delta + c . grad at boundary point b (None: delta):
        (DeviceArray N x N with N = 2 Nd + Nb, trace ratio of block 0).  A mixed coefficient multiplies its mixed derivative once.
        out: a DeviceArray to write into (any leading dimension >= N)."""
        return self._assemble_blocks(self.lib.gpk_assemble_op3d, 3, kernel, kernel_parameter, Xd, Xb, self._coeffs3(op3, bc3),
                                        nugget, nugget_type, out)

    def extend_functionals_op3d(self, kernel, kernel_parameter, Xt, Xd, Xb, op3, bc3, coeff, which=OP3_NAMES):
        """Value / derivatives up to order two of the 3-D extension under op3 and bc3 at Xt (gpk_extend_functionals_op3d): a
        (len(which), Nt) DeviceArray, row k = functional which[k] (names: FUNCTIONAL_OP3).  coeff = Theta^{-1} sol_vec with the Theta
        of assemble_op3d."""
        return self._extend_functionals('extend_functionals_op3d', FUNCTIONAL_OP3, 3, self.lib.gpk_extend_functionals_op3d, (),
                                        kernel, kernel_parameter, Xt, Xd, Xb, self._coeffs3(op3, bc3), coeff, which)

    # ---- gradient layout in three dimensions (gpk_assemble_grad3d, gpk_extend_functionals_grad3d, gpk_pde_residual_sl3d) ----
    def assemble_grad3d(self, kernel, kernel_parameter, Xd, Xb, op3, bc3, nugget=0.0, nugget_type='none', out=None):
        """Gram matrix of the 3-D gradient layout (blocks d1, d2, d3, psi on Xd, delta / phi on [Xd; Xb]; op3 and bc3 as for
        assemble_op3d): (DeviceArray N x N with N = 5 Nd + Nb, [trace(block k) / trace(block 4) for k = 0..3]).  out: a DeviceArray to
        write into (any leading dimension >= N)."""
        return self._assemble_blocks(self.lib.gpk_assemble_grad3d, 3, kernel, kernel_parameter, Xd, Xb, self._coeffs3(op3, bc3),
                                     nugget, nugget_type, out, rows=5, nratios=4)

    def extend_functionals_grad3d(self, kernel, kernel_parameter, Xt, Xd, Xb, op3, bc3, coeff, which=OP3_NAMES):
        """Value / derivatives up to order two of the extension on the 3-D gradient layout at Xt (gpk_extend_functionals_grad3d): a
        (len(which), Nt) DeviceArray, row k = functional which[k] (names: FUNCTIONAL_OP3).  coeff = Theta^{-1} sol_vec (5 Nd + Nb
        values) with the Theta of assemble_grad3d."""
        return self._extend_functionals('extend_functionals_grad3d', FUNCTIONAL_OP3, 3, self.lib.gpk_extend_functionals_grad3d, (),
                                        kernel, kernel_parameter, Xt, Xd, Xb, self._coeffs3(op3, bc3), coeff, which)

    def pde_residual_sl3d(self, gq8, fields, psi_u, rhs):
        """Pointwise residual -psi_u + N(u0, u1, u2, u3) - f of the 3-D semilinear equation with gq8 = (a1, a2, a3, b1, b2, b3, c1, c3)
        (gpk_pde_residual_sl3d), as an (Nt,) DeviceArray.  fields: (4, Nt) value, d1, d2, d3; psi_u: (Nt,) psi[u] at the test points;
        rhs as for pde_residual."""
        gq8 = [float(v) for v in gq8]
        if len(gq8) != 8:
            raise ValueError(f'gq8: the eight coefficients (a1, a2, a3, b1, b2, b3, c1, c3), got {len(gq8)}')
        dp = self._on_device(psi_u)
        return self._pde_residual(self.lib.gpk_pde_residual_sl3d, ((C.c_double * 8)(*gq8),), fields, rhs, (dp.ptr,))

    def pde_residual(self, system, params, fields_u, fields_a, rhs):
        """Pointwise residual of the equation (gpk_pde_residual) as an (Nt,) DeviceArray.  fields_u: (4, Nt) DeviceArray or host array
        with rows value, d1, d2, laplacian (Burgers: value, u_t, u_x, u_xx); fields_a: (3, Nt) value, d1, d2 of a (Darcy_flow2d only,
        else None); params: the equation's _gn_params() (its first two entries are used); rhs: f at the test points."""
        da = self._on_device(fields_a, fields=True) if fields_a is not None else None
        p = (C.c_double * 3)(*[float(v) for v in (list(params) + [0.0, 0.0, 0.0])[:3]]) if params is not None else None
        return self._pde_residual(self.lib.gpk_pde_residual, (SYSTEM[system], p), fields_u, rhs, (da.ptr, da.ld) if da is not None else (None, 0))

    def pde_residual_nl(self, nonlin, params, fields_u, rhs):
        """Pointwise residual -u3 + tau(u0) - f of the elliptic equation with the reaction term `nonlin` (a GPK_NL_* id or its name in
        NONLIN) and params = (p0, p1, p2) (gpk_pde_residual_nl), as an (Nt,) DeviceArray.  fields_u, rhs as for pde_residual."""
        p = (C.c_double * 3)(*[float(v) for v in (list(params) + [0.0, 0.0, 0.0])[:3]])
        kind = NONLIN[nonlin] if isinstance(nonlin, str) else int(nonlin)
        return self._pde_residual(self.lib.gpk_pde_residual_nl, (kind, p), fields_u, rhs)

    def pde_residual_sl(self, eps, gq, fields, rhs):
        """Pointwise residual -eps u3 + N(u0, u1, u2) - f of the semilinear equation with gq = (a1, a2, b, c1, c3)
        (gpk_pde_residual_sl), as an (Nt,) DeviceArray.  fields: (4, Nt) value, d1, d2, laplacian; rhs as for pde_residual."""
        gq = [float(v) for v in gq]
        if len(gq) != 5:
            raise ValueError(f'gq: the five coefficients (a1, a2, b, c1, c3), got {len(gq)}')
        return self._pde_residual(self.lib.gpk_pde_residual_sl, (float(eps), (C.c_double * 5)(*gq)), fields, rhs)

    def error_metrics(self, truth, approx):
        """(|truth - approx| as a numpy array, its maximum, sqrt(sum of squares / n)) computed on the device (gpk_error_metrics);
        truth / approx: host arrays or DeviceArrays of the same length"""
        dt = truth if isinstance(truth, DeviceArray) else self.array(np.asarray(truth, dtype=np.float64).ravel())
        da = approx if isinstance(approx, DeviceArray) else self.array(np.asarray(approx, dtype=np.float64).ravel())
        n = dt.rows
        if da.rows != n:
            raise ValueError(f'error_metrics: {n} truth values against {da.rows} approximations')
        err = DeviceArray(self, n)
        mx, l2 = C.c_double(), C.c_double()
        self._chk(self.lib.gpk_error_metrics(self.h, n, dt.ptr, da.ptr, err.ptr, C.byref(mx), C.byref(l2)))
        return err.download(), mx.value, l2.value

    # ---- dense ----
    def potrf(self, A, n=None):
        n = A.rows if n is None else n
        info = C.c_int()
        self._chk(self.lib.gpk_potrf(self.h, A.ptr, n, A.ld, C.byref(info)))
        return self._chk_info(info.value)

    @staticmethod
    def _chk_info(info):
        """> 0 is LAPACK's info (first non-positive pivot); < 0 means a bounded device-side wait expired (lost launch)."""
        if info < 0:
            raise GpkError(f'libgpk: a device-side wait expired inside the factorisation (info = {info}); the result is invalid')
        return info

    def tril(self, A, n=None):
        self._chk(self.lib.gpk_tril(self.h, A.ptr, A.rows if n is None else n, A.ld))

    def symmetrize(self, A, n=None):
        self._chk(self.lib.gpk_symmetrize_lower(self.h, A.ptr, A.rows if n is None else n, A.ld))

    def trsm(self, L, B, trans=False, n=None, nrhs=None):
        n = L.rows if n is None else n
        nrhs = B.cols if nrhs is None else nrhs
        self._chk(self.lib.gpk_trsm(self.h, int(trans), L.ptr, n, L.ld, B.ptr, nrhs, B.ld))

    def trtri_diag(self, L, n=None, block=None):
        """inverses of the block x block diagonal blocks of the factor L -> (n, block) device array (gpk_trtri_diag)"""
        n = L.rows if n is None else n
        block = dinv_block_for(n) if block is None else int(block)
        D = DeviceArray(self, n, block, ld=block)
        self._chk(self.lib.gpk_trtri_diag(self.h, L.ptr, n, L.ld, D.ptr, block))
        return D

    def trsm_dinv(self, L, Dinv, B, X, n=None, nrhs=None, lead=0):
        """X <- L^{-1} B through the inverted diagonal blocks (B becomes scratch; X zero on entry when lead > 0)"""
        n = L.rows if n is None else n
        nrhs = B.cols if nrhs is None else nrhs
        self._chk(self.lib.gpk_trsm_dinv(self.h, L.ptr, Dinv.ptr, Dinv.ld, n, L.ld, B.ptr, nrhs, B.ld, X.ptr, X.ld, int(lead)))

    def potrs(self, L, B, n=None, nrhs=None):
        n = L.rows if n is None else n
        nrhs = B.cols if nrhs is None else nrhs
        self._chk(self.lib.gpk_potrs(self.h, L.ptr, n, L.ld, B.ptr, nrhs, B.ld))

    def gemm(self, ta, tb, m, n, k, alpha, A, B, beta, Cm):
        self._chk(self.lib.gpk_gemm(self.h, int(ta), int(tb), m, n, k, float(alpha), A.ptr, A.ld, B.ptr, B.ld, float(beta), Cm.ptr, Cm.ld))

    def syrk(self, n, k, alpha, A, beta, Cm, full=False):
        self._chk(self.lib.gpk_syrk(self.h, n, k, float(alpha), A.ptr, A.ld, float(beta), Cm.ptr, Cm.ld, int(full)))

    # ---- Gauss-Newton ----
    def gn_step(self, prob, z, step_size=1.0):
        S, H, delta, _ = prob.workspace()
        loss, info = C.c_double(), C.c_int()
        self._chk(self.lib.gpk_gn_step(self.h, C.byref(prob.struct), z.ptr, float(step_size), S.ptr, S.ld, H.ptr, H.ld,
                                       delta.ptr, C.byref(loss), C.byref(info)))
        return loss.value, self._chk_info(info.value)

    # ---- line search (gpk_gn_direction, gpk_gn_trial_losses, gpk_gn_trial_accept, gpk_gn_step_ls) ----
    def gn_direction(self, prob, z):
        """(loss(z), pred, info): gn_step without the update -- delta = H^{-1} g is left in prob.workspace()[2], z is not written;
        pred = g . delta / 2, so loss - pred is the minimum of the linearised loss"""
        S, H, delta, _ = prob.workspace()
        loss, pred, info = C.c_double(), C.c_double(), C.c_int()
        self._chk(self.lib.gpk_gn_direction(self.h, C.byref(prob.struct), z.ptr, S.ptr, S.ld, H.ptr, H.ld, delta.ptr,
                                            C.byref(loss), C.byref(pred), C.byref(info)))
        return loss.value, pred.value, self._chk_info(info.value)

    def gn_trial_losses(self, prob, z, t, delta=None, download=True):
        """J(z - t_k delta) for the step sizes t (1 .. 16 of them): numpy array, or (download=False: no synchronisation) the DeviceArray
        that holds them in its first len(t) entries.  delta: a DeviceArray, default the direction of the last gn_direction / gn_step."""
        t = np.ascontiguousarray(t, dtype=np.float64).ravel()
        delta = prob.workspace()[2] if delta is None else delta
        W, ldw, dl = prob.trial_workspace(max(t.size, 1))
        out = np.empty(t.size) if download else None
        self._chk(self.lib.gpk_gn_trial_losses(self.h, C.byref(prob.struct), z.ptr, delta.ptr, t.ctypes.data_as(C.POINTER(C.c_double)), t.size,
                                               W.ptr, ldw, dl.ptr, out.ctypes.data_as(C.POINTER(C.c_double)) if download else None))
        return out if download else dl

    def gn_trial_accept(self, prob, z, losses, t, loss_in, pred, c1=1e-4, delta=None):
        """(k, t_k): the acceptance rule on the device over `losses` (a DeviceArray, as gn_trial_losses(download=False) returns it) and
        z <- z - t_k delta; k = -1 (t = 0.0) leaves z untouched"""
        t = np.ascontiguousarray(t, dtype=np.float64).ravel()
        delta = prob.workspace()[2] if delta is None else delta
        k, ta = C.c_int(), C.c_double()
        self._chk(self.lib.gpk_gn_trial_accept(self.h, prob.nz, z.ptr, delta.ptr, losses.ptr, t.ctypes.data_as(C.POINTER(C.c_double)), t.size,
                                               float(loss_in), float(pred), float(c1), C.byref(k), C.byref(ta)))
        return k.value, ta.value

    def gn_step_ls(self, prob, z, trials=8, t0=1.0, shrink=0.5, c1=1e-4):
        """One line-searched Gauss-Newton step, one host synchronisation: (loss(z_in), info, k, t_k, trial losses).  k = -1: no trial
        reduced the loss (or the factorisation of H failed) and z is unchanged."""
        S, H, delta, _ = prob.workspace()
        W, ldw, _ = prob.trial_workspace(trials)
        opt = _libmod.LSOptionsStruct(int(trials), float(t0), float(shrink), float(c1))
        loss, info, k, ta = C.c_double(), C.c_int(), C.c_int(), C.c_double()
        losses = np.empty(int(trials))
        self._chk(self.lib.gpk_gn_step_ls(self.h, C.byref(prob.struct), z.ptr, C.byref(opt), S.ptr, S.ld, H.ptr, H.ld, delta.ptr, W.ptr, ldw,
                                          C.byref(loss), losses.ctypes.data_as(C.POINTER(C.c_double)), C.byref(k), C.byref(ta), C.byref(info)))
        return loss.value, self._chk_info(info.value), k.value, ta.value, losses

    def gn_loss(self, prob, z):
        _, _, _, work = prob.workspace()
        loss = C.c_double()
        self._chk(self.lib.gpk_gn_loss(self.h, C.byref(prob.struct), z.ptr, work.ptr, C.byref(loss)))
        return loss.value

    def gn_hessian_grad(self, prob, z):
        S, H, delta, _ = prob.workspace()
        self._chk(self.lib.gpk_gn_hessian_grad(self.h, C.byref(prob.struct), z.ptr, S.ptr, S.ld, H.ptr, H.ld, delta.ptr))
        self.synchronize()
        return H.download(prob.nz, prob.nz), delta.download()

    def gn_measurement(self, prob, z):
        _, _, _, work = prob.workspace()
        self._chk(self.lib.gpk_gn_measurement(self.h, C.byref(prob.struct), z.ptr, work.ptr))
        self.synchronize()
        return work.download()

    # ---- posterior variance (gpk_assemble_cross, gpk_col_sumsq, gpk_posterior_prepare, gpk_posterior_variance) ----
    def assemble_cross(self, layout, kernel, kernel_parameter, Xt, Xd, Xb, out=None):
        """Cross-covariances of u at the test points Xt with the N collocation functionals of `layout`: the block of assemble_test
        transposed, an (N, Nt) DeviceArray -- the right-hand-side layout of trsm / trsm_dinv.  out: a DeviceArray to write into
        (rows >= N, leading dimension >= Nt)."""
        Xt, Xd, Xb = (np.ascontiguousarray(X, dtype=np.float64).reshape(-1, 2) for X in (Xt, Xd, Xb))
        Nt, Nd, Nb = Xt.shape[0], Xd.shape[0], Xb.shape[0]
        dXt, dXd, dXb = self.points(Xt), self.points(Xd), self.points(Xb)
        lay = LAYOUT[layout]
        N = {0: 2 * Nd + Nb, 1: 4 * Nd + Nb, 2: 4 * Nd + Nb, 3: 3 * Nd}[lay]
        K = out if out is not None else DeviceArray(self, N, Nt)
        self._chk(self.lib.gpk_assemble_cross(self.h, lay, KERNEL[kernel], kernel_params(kernel, kernel_parameter),
                                              dXt.ptr, Nt, dXd.ptr, Nd, dXb.ptr, Nb, K.ptr, K.ld))
        self.synchronize()
        return K

    def col_sumsq(self, V, alpha=1.0, base=None, rows=None, cols=None):
        """(cols,) DeviceArray: base + alpha * column sums of squares of the DeviceArray V (gpk_col_sumsq; base: DeviceArray or None)"""
        rows = V.rows if rows is None else rows
        cols = V.cols if cols is None else cols
        out = DeviceArray(self, cols)
        self._chk(self.lib.gpk_col_sumsq(self.h, V.ptr, rows, cols, V.ld, float(alpha), base.ptr if base is not None else None, out.ptr))
        return out

    def posterior_worksize(self, prob, nt, ldp=0, ldr=0, ldk=0):
        """gpk_posterior_worksize for batches of nt test points: dict with the leading dimensions ldp, ldr, ldk (0 = the smallest
        admissible, padded) and P_bytes, R_bytes, K_bytes, W_bytes, handle_bytes.  Pure host query."""
        ld = [C.c_int() for _ in range(3)]
        sz = [C.c_size_t() for _ in range(5)]
        rc = self.lib.gpk_posterior_worksize(C.byref(prob.struct), int(nt), int(ldp), int(ldr), int(ldk),
                                             *[C.byref(x) for x in ld], *[C.byref(x) for x in sz])
        if rc != 0:                                                       # (a host function: it leaves no text in gpk_last_error)
            raise GpkError(f'libgpk error {rc}: gpk_posterior_worksize rejected the problem or the sizes (the relaxed elliptic system '
                           'is not served; nt > 0; leading dimensions at least nz + 1, nz, nt)')
        return dict(zip(('ldp', 'ldr', 'ldk', 'P_bytes', 'R_bytes', 'K_bytes', 'W_bytes', 'handle_bytes'), [x.value for x in ld + sz]))

    def posterior_prepare(self, prob, z):
        """Once per converged iterate z (DeviceArray): (P, R, info) with P = L^{-1} A(z) and R the Cholesky factor of H/2
        (gpk_posterior_prepare); info as potrf.  Buffers as gpk_posterior_worksize sizes them."""
        ws = self.posterior_worksize(prob, 1)
        P = DeviceArray(self, prob.rows, prob.nz + 1, ld=ws['ldp'])
        R = DeviceArray(self, prob.nz, prob.nz, ld=ws['ldr'])
        info = C.c_int()
        self._chk(self.lib.gpk_posterior_prepare(self.h, C.byref(prob.struct), z.ptr, P.ptr, P.ld, R.ptr, R.ld, C.byref(info)))
        return P, R, self._chk_info(info.value)

    def posterior_variance(self, prob, P, R, K, field=0, nt=None, W=None, want_cond=True, want_var=True):
        """One batch of test points: K (N_field, nt) from assemble_cross is overwritten; returns (var_cond, var) as (nt,) DeviceArrays
        (None where not asked for) -- gpk_posterior_variance.  field: 0 = u, 1 = a (Darcy only).  W: (nz, >= nt) scratch."""
        nt = K.cols if nt is None else int(nt)
        if W is None and want_var:
            W = DeviceArray(self, prob.nz, nt)
        vc = DeviceArray(self, nt) if want_cond else None
        v = DeviceArray(self, nt) if want_var else None
        self._chk(self.lib.gpk_posterior_variance(self.h, C.byref(prob.struct), P.ptr if P is not None else None, P.ld if P is not None else 0,
                                                  R.ptr if R is not None else None, R.ld if R is not None else 0, int(field),
                                                  K.ptr, K.ld, nt, W.ptr if W is not None else None, W.ld if W is not None else 0,
                                                  vc.ptr if vc is not None else None, v.ptr if v is not None else None))
        return vc, v

    def posterior_variance_points(self, prob, P, R, field, layout, kernel, kernel_parameter, X_test, Xd, Xb, nt_chunk=1024):
        """(var_cond, var) as numpy arrays at all of X_test, in batches of nt_chunk points: one K (N_field x nt_chunk) and one W
        (nz x nt_chunk) buffer serve every batch, so the workspace does not grow with the number of test points."""
        X_test = np.ascontiguousarray(X_test, dtype=np.float64).reshape(-1, 2)
        Xb = np.ascontiguousarray(Xb, dtype=np.float64).reshape(-1, 2)
        Nt, Nd, Nb = X_test.shape[0], np.asarray(Xd).shape[0], Xb.shape[0]
        nt_chunk = max(1, min(int(nt_chunk), Nt))
        lay = LAYOUT[layout]
        N = {0: 2 * Nd + Nb, 1: 4 * Nd + Nb, 2: 4 * Nd + Nb, 3: 3 * Nd}[lay]
        dXt, dXd, dXb = self.points(X_test), self.points(Xd), self.points(Xb)
        ldk = self.posterior_worksize(prob, nt_chunk)['ldk']
        K, W = DeviceArray(self, N, nt_chunk, ld=ldk), DeviceArray(self, prob.nz, nt_chunk, ld=ldk)
        vc, v = DeviceArray(self, Nt), DeviceArray(self, Nt)
        kp = kernel_params(kernel, kernel_parameter)
        for t0 in range(0, Nt, nt_chunk):
            nt = min(nt_chunk, Nt - t0)
            self._chk(self.lib.gpk_assemble_cross(self.h, lay, KERNEL[kernel], kp, dXt.at(t0), nt, dXd.ptr, Nd, dXb.ptr, Nb, K.ptr, K.ld))
            self._chk(self.lib.gpk_posterior_variance(self.h, C.byref(prob.struct), P.ptr, P.ld, R.ptr, R.ld, int(field), K.ptr, K.ld, nt,
                                                      W.ptr, W.ld, vc.ptr + 8 * t0, v.ptr + 8 * t0))
        self.synchronize()
        out = vc.download(), v.download()
        for a in (K, W, vc, v, dXt, dXd, dXb):
            a.free()
        return out

    # ---- posterior covariance and samples (gpk_assemble_prior, gpk_posterior_covariance, gpk_posterior_sample) ----
    def assemble_prior(self, kernel, kernel_parameter, Xa, Xb=None, out=None):
        """Prior k(xa_i, xb_j) between two sets of 2-D points as an (na, nb) DeviceArray (gpk_assemble_prior).  Xb=None: Xa against
        itself -- bitwise symmetric, unit diagonal.  out: a DeviceArray to write into (rows >= na, leading dimension >= nb)."""
        Xa = np.ascontiguousarray(Xa, dtype=np.float64).reshape(-1, 2)
        dXa = self.points(Xa)
        if Xb is None:
            dXb, nb = dXa, Xa.shape[0]
        else:
            Xb = np.ascontiguousarray(Xb, dtype=np.float64).reshape(-1, 2)
            dXb, nb = self.points(Xb), Xb.shape[0]
        Cm = out if out is not None else DeviceArray(self, Xa.shape[0], nb)
        self._chk(self.lib.gpk_assemble_prior(self.h, KERNEL[kernel], kernel_params(kernel, kernel_parameter), dXa.ptr, Xa.shape[0],
                                              dXb.ptr, nb, Cm.ptr, Cm.ld))
        self.synchronize()
        for a in {id(dXa): dXa, id(dXb): dXb}.values():
            a.free()
        return Cm

    def posterior_covariance(self, prob, P, R, K, Cm, field=0, nt=None, W=None, with_gn=True):
        """One batch of test points: Cm (nt, nt) holds the prior on entry and C - V^T V (+ W^T W with with_gn) on return, both triangles,
        bitwise symmetric; K (N_field, nt) from assemble_cross is overwritten (gpk_posterior_covariance).  field: 0 = u, 1 = a (Darcy
        only).  with_gn=False: P, R and W may be None.  Returns Cm."""
        nt = K.cols if nt is None else int(nt)
        if W is None and with_gn:
            W = DeviceArray(self, prob.nz, nt)
        opt = lambda a: (a.ptr, a.ld) if a is not None else (None, 0)
        (pp, ldp), (rp, ldr), (wp, ldw) = opt(P), opt(R), opt(W)
        self._chk(self.lib.gpk_posterior_covariance(self.h, C.byref(prob.struct), pp, ldp, rp, ldr, int(field), K.ptr, K.ld, nt,
                                                    wp, ldw, Cm.ptr, Cm.ld, int(bool(with_gn))))
        return Cm

    def posterior_sample(self, Cm, mean, xi, jitter, nt=None, out=None, return_factor=False):
        """Samples of N(mean, Cm + jitter I): (samples, info), samples an (nt, ns) numpy array -- mean[t] + (L xi)[t, s] with L the lower
        Cholesky factor, computed on the device (gpk_posterior_sample) -- or None when info != 0 (potrf's info: the first non-positive
        pivot).  Cm (DeviceArray, nt x nt) is overwritten with the factor; xi: (nt, ns) standard normals, the caller's.  out: a
        DeviceArray to write into (left untouched when info != 0).  return_factor=True: (samples, info, L) with L the factor as a numpy
        array."""
        nt = Cm.rows if nt is None else int(nt)
        xi = np.ascontiguousarray(xi, dtype=np.float64).reshape(nt, -1)
        ns = xi.shape[1]
        dxi = DeviceArray(self, nt, ns, ld=pad_ld(ns)).upload(xi)
        dmean = mean if isinstance(mean, DeviceArray) else self.array(np.asarray(mean, dtype=np.float64).ravel())
        dout = out if out is not None else DeviceArray(self, nt, ns, ld=pad_ld(ns))
        info = C.c_int()
        self._chk(self.lib.gpk_posterior_sample(self.h, Cm.ptr, Cm.ld, nt, float(jitter), dmean.ptr, dxi.ptr, dxi.ld, ns, dout.ptr, dout.ld,
                                                C.byref(info)))
        self.synchronize()
        code = self._chk_info(info.value)
        samples = dout.download(nt, ns).reshape(nt, ns) if code == 0 else None
        dxi.free()
        if dmean is not mean:
            dmean.free()
        if dout is not out:
            dout.free()
        if return_factor:
            return samples, code, Cm.download(nt, nt)
        return samples, code

    def posterior_covariance_points(self, prob, P, R, field, layout, kernel, kernel_parameter, X_test, Xd, Xb, keep=False):
        """(cov_cond, cov) as (N_t, N_t) numpy arrays at all of X_test in ONE batch (the covariance couples every pair of test points):
        prior, cross-covariances and gpk_posterior_covariance twice, without and with the Gauss-Newton term.  ValueError when the
        (N + n_z + N_t) N_t doubles of K, W and the covariance do not fit the device.  keep=True: (cov_cond, cov, dC) with dC the
        DeviceArray of cov (for posterior_sample; the caller frees it)."""
        X_test = np.ascontiguousarray(X_test, dtype=np.float64).reshape(-1, 2)
        Xb = np.ascontiguousarray(Xb, dtype=np.float64).reshape(-1, 2)
        Nt, Nd, Nb = X_test.shape[0], np.asarray(Xd).shape[0], Xb.shape[0]
        lay = LAYOUT[layout]
        N = {0: 2 * Nd + Nb, 1: 4 * Nd + Nb, 2: 4 * Nd + Nb, 3: 3 * Nd}[lay]
        need, have = 8 * (N + prob.nz + Nt) * Nt, self.device_info()['hbm_bytes']
        if need > have:
            raise ValueError(f'posterior_covariance: one batch of {Nt} test points needs (N + n_z + N_t) N_t doubles = {need} bytes '
                             f'(N = {N}, n_z = {prob.nz}) and the device has {have} bytes; the covariance is not computed in '
                             'pieces -- use fewer test points')
        dXt, dXd, dXb = self.points(X_test), self.points(Xd), self.points(Xb)
        ldk = self.posterior_worksize(prob, Nt)['ldk']
        K, W = DeviceArray(self, N, Nt, ld=ldk), DeviceArray(self, prob.nz, Nt, ld=ldk)
        Cc, Cg = DeviceArray(self, Nt, Nt, ld=ldk), DeviceArray(self, Nt, Nt, ld=ldk)
        kp = kernel_params(kernel, kernel_parameter)
        for Cm, gn in ((Cc, 0), (Cg, 1)):
            self._chk(self.lib.gpk_assemble_prior(self.h, KERNEL[kernel], kp, dXt.ptr, Nt, dXt.ptr, Nt, Cm.ptr, Cm.ld))
            self._chk(self.lib.gpk_assemble_cross(self.h, lay, KERNEL[kernel], kp, dXt.ptr, Nt, dXd.ptr, Nd, dXb.ptr, Nb, K.ptr, K.ld))
            self._chk(self.lib.gpk_posterior_covariance(self.h, C.byref(prob.struct), P.ptr, P.ld, R.ptr, R.ld, int(field), K.ptr, K.ld, Nt,
                                                        W.ptr, W.ld, Cm.ptr, Cm.ld, gn))
        self.synchronize()
        out = Cc.download(Nt, Nt), Cg.download(Nt, Nt)
        for a in (K, W, Cc, dXt, dXd, dXb):
            a.free()
        if keep:
            return out + (Cg,)
        Cg.free()
        return out

    # ---- log evidence (gpk_chol_logdet, gpk_log_evidence) ----
    def chol_logdet(self, L, n=None):
        """(log |L L^T|, bad) of the lower factor in the DeviceArray L: 2 sum_i log L_ii over its diagonal and the number of diagonal
        entries that are not > 0 (gpk_chol_logdet).  Fixed reduction order: the same bits on every call."""
        n = L.rows if n is None else int(n)
        value, bad = C.c_double(), C.c_int()
        self._chk(self.lib.gpk_chol_logdet(self.h, L.ptr, n, L.ld, C.byref(value), C.byref(bad)))
        return value.value, bad.value

    def log_evidence(self, prob, z):
        """Laplace log evidence at the iterate z (DeviceArray): (terms, P, R, info) with terms = dict(log_Z, J, logdet_theta, logdet_H,
        gamma_term, two_pi_term), log_Z = -(J + logdet_theta + logdet_H) / 2 - gamma_term - two_pi_term (NaN when info != 0 or a pivot of a
        factor is not > 0), and P, R, info exactly those of posterior_prepare (gpk_log_evidence)."""
        ws = self.posterior_worksize(prob, 1)
        P = DeviceArray(self, prob.rows, prob.nz + 1, ld=ws['ldp'])
        R = DeviceArray(self, prob.nz, prob.nz, ld=ws['ldr'])
        _, _, _, work = prob.workspace()
        terms, info = (C.c_double * 6)(), C.c_int()
        self._chk(self.lib.gpk_log_evidence(self.h, C.byref(prob.struct), z.ptr, P.ptr, P.ld, R.ptr, R.ld, work.ptr, terms, C.byref(info)))
        return dict(zip(EVIDENCE_TERMS, (float(t) for t in terms))), P, R, self._chk_info(info.value)

    # ---- per-phase timing of gn_step ----
    def prof_enable(self, on=True):
        self._chk(self.lib.gpk_prof_enable(self.h, int(on)))

    def prof_read(self):
        ms = (C.c_double * 4)()
        n = C.c_int()
        self._chk(self.lib.gpk_prof_read(self.h, ms, C.byref(n)))
        pipelined, cus, syrk_launch = C.c_int(), C.c_int(), C.c_double()
        self._chk(self.lib.gpk_prof_read_pipeline(self.h, C.byref(pipelined), C.byref(syrk_launch), C.byref(cus)))
        # pipelined: syrk_ms is the wall time of the fused product + factorisation phase and potrf_ms is 0;
        # syrk_launch_ms = the SYRK launches themselves (events on the stream they ran on)
        # flops the matrix-product launches of those steps executed, counted by the launch logic itself (gpk_prof_read_flops)
        fl, nl = (C.c_double * 4)(), (C.c_long * 4)()
        self._chk(self.lib.gpk_prof_read_flops(self.h, fl, nl))
        return dict(steps=n.value, trsm_ms=ms[0], syrk_ms=ms[1], potrf_ms=ms[2], trsv_update_ms=ms[3],
                    pipelined=bool(pipelined.value), syrk_launch_ms=syrk_launch.value, chain_cus=cus.value,
                    solve_flops=fl[0], potrf_update_flops=fl[1], product_flops=fl[2],
                    solve_launches=nl[0], potrf_update_launches=nl[1], product_launches=nl[2])

    def prof_read_assembly(self):
        """milliseconds of the evaluator launch of the last assemble call issued with prof_enable(True)"""
        ms = C.c_double()
        self._chk(self.lib.gpk_prof_read_assembly(self.h, C.byref(ms)))
        return ms.value

    # ---- micro-benchmarks (development build only: Context(dev=True)) ----
    def ubench_mfma_f64(self, iters=20000):
        v = C.c_double()
        self._chk(self.lib.gpk_ubench_mfma_f64(self.h, iters, C.byref(v)))
        return v.value

    def ubench_latency(self, mode):
        v = C.c_double()
        self._chk(self.lib.gpk_ubench_latency(self.h, int(mode), C.byref(v)))
        return v.value

    def ubench_hbm_write(self, nbytes=1 << 30, iters=10):
        v = C.c_double()
        self._chk(self.lib.gpk_ubench_hbm_write(self.h, nbytes, iters, C.byref(v)))
        return v.value
