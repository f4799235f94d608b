"""Sub-matrix views inside a canary-filled buffer, and plain high-precision references, for the dense entry points of include/gpk.h.

Every dense routine takes VIEWS: a device pointer plus a leading dimension in elements (the multi-GPU schedules pass pointers into
the interior of one big matrix).  An Arena is one buffer filled with a canary -- a quiet NaN with a fixed payload, always compared
as uint64, never as a float -- in which rectangular views are placed at a chosen alignment class:

    A   base 16-byte aligned, ld even      (what ctx.array() produces: the control)
    B   odd element offset,   ld even
    C   base 16-byte aligned, ld odd
    D   odd element offset,   ld odd

After a call, assert_outside_untouched(views_written) checks bit for bit that every element outside the views still holds the
canary and that every view that was NOT written (a read-only operand) still holds exactly what was put there.

The buffer lives on the device (ctx given) or in a numpy array (ctx = None: tests/test_view_arena_host.py exercises the checker
itself that way).  Host-only module: nothing here imports the GPU package.

References are numpy longdouble (64-bit mantissa on x86, eps = 1.08e-19): three decimal digits below anything the fp64 kernels are
asked for, by the textbook algorithm, reading only the triangle the routine is allowed to read.  A 700^3 longdouble product takes
about 1.4 s, so callers keep reference operands at or below about 640 on a side.
"""
import ctypes as C

import numpy as np

CANARY_BITS = np.uint64(0x7FF8C0DEFACE5EED)         # quiet NaN (exponent all ones, top mantissa bit set) + a recognisable payload
CANARY = np.array([CANARY_BITS], dtype=np.uint64).view(np.float64)[0]
CLASSES = ('A', 'B', 'C', 'D')
LD = np.longdouble


# ---------------------------------------------------------------------------------------------------------------- buffers
class _HostBuffer:
    """numpy stand-in for the device buffer"""

    def __init__(self, size):
        self.buf = np.empty(size, dtype=np.float64)
        self.ptr = self.buf.ctypes.data

    def write(self, flat):
        self.buf[:] = flat

    def read(self):
        return self.buf.copy()


class _DeviceBuffer:
    def __init__(self, ctx, size):
        from gpk.device import DeviceArray                      # (imported on use: this module stays host-only)
        self.ctx = ctx
        self.arr = DeviceArray(ctx, size, 1, ld=1)
        self.ptr = self.arr.ptr
        self.size = size

    def write(self, flat):
        flat = np.ascontiguousarray(flat, dtype=np.float64)
        self.ctx._chk(self.ctx.lib.gpk_memcpy_h2d(self.ctx.h, self.ptr, flat.ctypes.data, self.size * 8))

    def read(self):
        out = np.empty(self.size, dtype=np.float64)
        self.ctx.synchronize()
        self.ctx._chk(self.ctx.lib.gpk_memcpy_d2h(self.ctx.h, out.ctypes.data, self.ptr, self.size * 8))
        return out

    def free(self):
        self.arr.free()


# ------------------------------------------------------------------------------------------------------------------ views
class View:
    """m x n elements at (r0, c0) of an arena: element (i, j) at flat index (r0 + i) * ld + c0 + j.  `wrap`: a contiguous operand
    (ld == n) placed at a column offset, whose rows run over the arena's row ends (the n x block array of gpk_trtri_diag)."""

    def __init__(self, arena, r0, c0, m, n):
        self.arena, self.r0, self.c0, self.m, self.n = arena, int(r0), int(c0), int(m), int(n)
        self.ld = arena.ld
        self.offset = self.r0 * self.ld + self.c0
        self.ptr = arena.ptr + 8 * self.offset
        self.index = (self.offset + np.arange(self.m)[:, None] * self.ld + np.arange(self.n)[None, :]).astype(np.int64)

    @property
    def cls(self):
        return alignment_class(self.ptr, self.ld)

    def at(self, i, j):
        return self.ptr + 8 * (i * self.ld + j)


def alignment_class(ptr, ld):
    odd_base, odd_ld = (ptr & 15) != 0, (ld & 1) != 0
    if ptr & 7:
        raise ValueError('pointer is not a multiple of 8 bytes')
    return {(False, False): 'A', (True, False): 'B', (False, True): 'C', (True, True): 'D'}[(odd_base, odd_ld)]


class Arena:
    def __init__(self, ctx, rows, cols, ld=None):
        self.ctx = ctx
        self.rows, self.cols = int(rows), int(cols)
        self.ld = int(ld) if ld is not None else self.cols
        if self.ld < self.cols:
            raise ValueError('ld < cols')
        self.size = self.rows * self.ld
        self.mirror = np.full(self.size, CANARY_BITS, dtype=np.uint64).view(np.float64)   # what the buffer is expected to hold
        self.dev = _HostBuffer(self.size) if ctx is None else _DeviceBuffer(ctx, self.size)
        self.ptr = self.dev.ptr
        if self.ptr & 15:
            raise ValueError('arena base is not 16-byte aligned')
        self.views = []
        self.dev.write(self.mirror)

    def view(self, r0, c0, m, n, wrap=False):
        v = View(self, r0, c0, m, n)
        if m and n:
            if v.index.min() < 0 or v.index.max() >= self.size:
                raise ValueError('view leaves the arena')
            if not wrap and c0 + n > self.ld:
                raise ValueError('view wider than the leading dimension')
            for o in self.views:
                if o.m and o.n and np.intersect1d(o.index.ravel(), v.index.ravel()).size:
                    raise ValueError('views overlap')
        self.views.append(v)
        return v

    def put(self, view, a):
        a = np.asarray(a, dtype=np.float64).reshape(view.m, view.n)
        self.mirror[view.index] = a
        self.dev.write(self.mirror)
        return view

    def get(self, view):
        return self.dev.read()[view.index].reshape(view.m, view.n)

    def assert_outside_untouched(self, views_written):
        """Bit for bit: canaries everywhere outside the arena's views, and every view that is not in views_written unchanged."""
        got = self.dev.read().view(np.uint64)
        want = self.mirror.view(np.uint64)
        check = np.ones(self.size, dtype=bool)
        for v in views_written:
            if v.arena is not self:
                raise ValueError('view of another arena')
            check[v.index.ravel()] = False
        inside = np.zeros(self.size, dtype=bool)
        for v in self.views:
            inside[v.index.ravel()] = True
        bad = np.flatnonzero(check & (got != want))
        if bad.size:
            k = int(bad[0])
            where = 'a read-only view' if inside[k] else 'the canary region'
            raise AssertionError(f'{bad.size} element(s) changed in {where}; first at row {k // self.ld}, column {k % self.ld} '
                                 f'(ld {self.ld}): {int(got[k]):#018x}, expected {int(want[k]):#018x}')

    def free(self):
        if hasattr(self.dev, 'free'):
            self.dev.free()


def class_view(ctx, m, n, cls, margin=2, ld_min=0):
    """A private arena holding one m x n view of alignment class `cls`, `margin` canary rows above and below and at least `margin`
    canary columns on either side."""
    if cls not in CLASSES:
        raise ValueError(cls)
    odd_off, odd_ld = cls in 'BD', cls in 'CD'
    r0 = 2 * ((margin + 1) // 2)                                 # even row offset: the column offset alone decides the parity
    c0 = margin + ((margin & 1) != odd_off)
    ld = max(c0 + n + margin, ld_min)
    ld += (ld & 1) != odd_ld
    arena = Arena(ctx, r0 + m + margin, ld, ld)
    v = arena.view(r0, c0, m, n)
    if m and n and v.cls != cls:
        raise AssertionError(f'built class {v.cls}, wanted {cls}')
    return v


def vector_view(ctx, n, odd_offset, margin=4):
    """A contiguous vector (ld = 1) at an even or odd element offset."""
    arena = Arena(ctx, n + 2 * margin + 1, 1, 1)
    return arena.view(margin + ((margin & 1) != bool(odd_offset)), 0, n, 1)


def flat_view(ctx, m, n, odd_offset, margin=4):
    """A contiguous m x n operand (ld = n) at an even or odd element offset of a flat buffer."""
    arena = Arena(ctx, m + 2, n, n)
    off = margin + ((margin & 1) != bool(odd_offset))
    return arena.view(0, off, m, n, wrap=True)


def with_canary_upper(L):
    """L with the canary NaN in its strict upper triangle"""
    out = np.array(L, dtype=np.float64, copy=True)
    out[np.triu_indices(out.shape[0], 1, out.shape[1])] = CANARY
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------------------- references
def ref_matmul(A, B):
    return np.matmul(np.asarray(A, dtype=LD), np.asarray(B, dtype=LD))


def ref_ata(A):
    A = np.asarray(A, dtype=LD)
    return np.matmul(A.T, A)


def ref_forward(L, B):
    """X with L X = B, row by row; reads the lower triangle of L only"""
    L = np.asarray(L, dtype=LD); X = np.array(B, dtype=LD, copy=True)
    if X.ndim == 1:
        X = X[:, None]
    for i in range(L.shape[0]):
        if i:
            X[i] -= L[i, :i] @ X[:i]
        X[i] /= L[i, i]
    return X


def ref_backward(L, B):
    """X with L^T X = B, row by row from the bottom; reads the lower triangle of L only"""
    L = np.asarray(L, dtype=LD); X = np.array(B, dtype=LD, copy=True)
    if X.ndim == 1:
        X = X[:, None]
    n = L.shape[0]
    for i in range(n - 1, -1, -1):
        if i + 1 < n:
            X[i] -= L[i + 1:, i] @ X[i + 1:]
        X[i] /= L[i, i]
    return X


def ref_right_lt(L, X):
    """X L^{-T}"""
    return ref_forward(L, np.asarray(X, dtype=LD).T).T


def ref_cholesky(A):
    """lower Cholesky factor, column by column; reads the lower triangle of A only.  A non-positive pivot gives NaN from there on."""
    A = np.asarray(A, dtype=LD)
    n = A.shape[0]
    L = np.zeros((n, n), dtype=LD)
    with np.errstate(invalid='ignore'):
        for j in range(n):
            d = A[j, j] - L[j, :j] @ L[j, :j]
            L[j, j] = np.sqrt(d)
            if j + 1 < n:
                L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def ref_tril(L):
    return np.tril(np.asarray(L, dtype=LD))


def fro(a):
    return float(np.sqrt(np.sum(np.square(np.asarray(a, dtype=LD)))))
