"""Device array / operator types: the backend's answer to the reference's implicit array protocol
(layer L1; section 8b "methods the unchanged solvers call").

  Context       rls_ctx: one per GPU (device + stream + reduction workspace)
  DeviceVector  the vector type of b and of every solver state vector (`similar(b, n)`)
  DeviceMatrix  the operator type of A: column-major dense matrix; `A.H @ A`-style normal operators
                are lazy (`NormalOperator`) so the unchanged constructors land in matrix-free mode
  SamplingOp, FFTOp, ProdOp(SamplingOp, FFTOp)
                matrix-free operators (csrc/fft.hip): no stored matrix, served by CGNR and FISTA
  RadonOp       the matrix-free parallel-beam projector of the computed-tomography example (csrc/radon.hip), served likewise
  NFFTOp        matrix-free non-uniform Fourier sampling (csrc/nfft.hip), served likewise
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional

import numpy as np

from . import _lib
from ._lib import C32, C64, F32, F64, OP_C, OP_N, OP_T, RLSError, check

_DT = {np.dtype(np.float32): F32, np.dtype(np.complex64): C32, np.dtype(np.float64): F64, np.dtype(np.complex128): C64}
_NP = {F32: np.dtype(np.float32), C32: np.dtype(np.complex64), F64: np.dtype(np.float64), C64: np.dtype(np.complex128)}


def dtype_code(dt) -> int:
    dt = np.dtype(dt)
    if dt not in _DT:
        raise TypeError(f"the MI355X backend computes in Float32 / ComplexF32 (tuned path) and Float64 / ComplexF64 (L1 protocol); got {dt}")
    return _DT[dt]


def is_double(code: int) -> bool:
    """Float64 / ComplexF64: the *_d entry points -- the L1 protocol with double scalars (rls_fill_d ... rls_gemv_d, the prox maps)
    and, for CGNR and FISTA, the streaming device plans rls_cgnr_*_d / rls_fista_*_d (scalars on the device, no read-back inside a
    solve without callbacks).  No resident or matrix-core kernels; every other solver runs its loop on the primitives."""
    return code in (F64, C64)


class Context:
    """rls_ctx wrapper.  `stream=None` creates a private non-blocking stream; pass a hipStream_t
    handle (e.g. torch.cuda.current_stream().cuda_stream) to share one."""

    def __init__(self, device: int = 0, stream: Optional[int] = None):
        self.lib = _lib.load()
        h = C.c_void_p()
        if stream is None:
            st = self.lib.rls_ctx_create(device, C.byref(h))
        else:
            st = self.lib.rls_ctx_create_on_stream(device, C.c_void_p(stream), C.byref(h))
        if st != 0 or not h:
            raise RLSError(f"rls_ctx_create(device={device}) failed with status {st}: no usable MI355X device? "
                           "(there is no CPU fallback)")
        self.handle = h
        self.device = device

    def sync(self):
        check(self.handle, self.lib.rls_ctx_sync(self.handle), "rls_ctx_sync")

    def tune(self, **kw):
        for k, v in kw.items():
            check(self.handle, self.lib.rls_tune_set(self.handle, k.encode(), int(v)), f"rls_tune_set({k})")

    def tuned(self, key: str) -> int:
        """the context's value of a switch the host side acts on (rls_tune_get)"""
        v = C.c_int32()
        check(self.handle, self.lib.rls_tune_get(self.handle, key.encode(), C.byref(v)), f"rls_tune_get({key})")
        return v.value

    @property
    def stream(self) -> int:
        return self.lib.rls_ctx_stream(self.handle) or 0

    def timer_start(self):
        check(self.handle, self.lib.rls_timer_start(self.handle), "rls_timer_start")

    def timer_stop_ms(self) -> float:
        ms = C.c_float()
        check(self.handle, self.lib.rls_timer_stop_ms(self.handle, C.byref(ms)), "rls_timer_stop_ms")
        return float(ms.value)

    def close(self):
        if getattr(self, "handle", None):
            self.lib.rls_ctx_destroy(self.handle)
            self.handle = None


_default_ctx: Dict[int, Context] = {}


def default_context(device: int = 0) -> Context:
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]


class _DeviceBuffer:
    """owning device allocation (the Julia side would attach a finalizer calling rls_free)"""

    _GUARD = 2 << 20  # RLS_GUARD_ALLOC=1 (test runs): own 2 MiB-granular allocation, data at its END

    def __init__(self, ctx: Context, nbytes: int):
        self.ctx = ctx
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        if os.environ.get("RLS_GUARD_ALLOC") == "1":
            # out-of-bounds reads past the end of a vector / matrix then leave the allocation and fault instead of
            # silently reading a neighbour (how the slab_load overrun for N < 128 was found)
            used = (max(self.nbytes, 1) + 15) // 16 * 16
            total = (used + self._GUARD - 1) // self._GUARD * self._GUARD
            check(ctx.handle, ctx.lib.rls_malloc(ctx.handle, total, C.byref(p)), "rls_malloc")
            self._base = p.value
            self.ptr = p.value + total - used
        else:
            check(ctx.handle, ctx.lib.rls_malloc(ctx.handle, max(self.nbytes, 1), C.byref(p)), "rls_malloc")
            self._base = self.ptr = p.value

    def __del__(self):
        try:
            if self._base and self.ctx.handle:
                self.ctx.lib.rls_free(self.ctx.handle, C.c_void_p(self._base))
        except Exception:
            pass
        self.ptr = self._base = None


class _BorrowedBuffer:
    def __init__(self, ptr: int, keep=None):
        self.ptr, self._keep = int(ptr), keep


class DeviceVector:
    """Length-n Float32 / ComplexF32 vector in HBM."""

    def __init__(self, n: int, dtype, ctx: Optional[Context] = None, _buf=None, _offset=0):
        self.ctx = ctx or default_context()
        self.n = int(n)
        self.dtype = np.dtype(dtype)
        self.code = dtype_code(self.dtype)
        self._buf = _buf or _DeviceBuffer(self.ctx, self.n * self.dtype.itemsize)
        self.ptr = self._buf.ptr + _offset

    # --- construction -----------------------------------------------------------------------
    @classmethod
    def from_host(cls, a, ctx: Optional[Context] = None) -> "DeviceVector":
        a = np.ascontiguousarray(a)
        if a.ndim != 1:
            raise ValueError("DeviceVector.from_host expects a 1-D array")
        v = cls(a.shape[0], a.dtype, ctx)
        v.copy_from_host(a)
        return v

    @classmethod
    def borrow(cls, ptr: int, n: int, dtype, ctx: Optional[Context] = None, keep=None) -> "DeviceVector":
        """view of device memory owned by someone else (e.g. a torch tensor that torch.distributed all-reduces in
        place); `keep` is held so the owner outlives the view"""
        return cls(n, dtype, ctx, _buf=_BorrowedBuffer(ptr, keep))

    def similar(self, n: Optional[int] = None) -> "DeviceVector":
        return DeviceVector(self.n if n is None else n, self.dtype, self.ctx)

    def copy(self) -> "DeviceVector":
        out = self.similar()
        out.copy_from(self)
        return out

    # --- transfers --------------------------------------------------------------------------
    def copy_from_host(self, a):
        a = np.ascontiguousarray(a, dtype=self.dtype)
        if a.size != self.n:
            raise ValueError(f"size mismatch: {a.size} vs {self.n}")
        lib, h = self.ctx.lib, self.ctx.handle
        check(h, lib.rls_memcpy_h2d(h, self.ptr, a.ctypes.data, a.nbytes), "rls_memcpy_h2d")

    def to_host(self) -> np.ndarray:
        out = np.empty(self.n, dtype=self.dtype)
        lib, h = self.ctx.lib, self.ctx.handle
        check(h, lib.rls_memcpy_d2h(h, out.ctypes.data, self.ptr, out.nbytes), "rls_memcpy_d2h")
        return out

    def copy_from(self, other: "DeviceVector"):
        if other.n != self.n or other.dtype != self.dtype:
            raise ValueError("copy_from: shape/dtype mismatch")
        lib, h = self.ctx.lib, self.ctx.handle
        check(h, lib.rls_memcpy_d2d(h, self.ptr, other.ptr, self.n * self.dtype.itemsize), "rls_memcpy_d2d")

    # --- BLAS-1 (names follow LinearAlgebra) ----------------------------------------------------
    # (Float64 / ComplexF64 vectors take the rls_*_d entry points: double scalars in, double results out)
    def fill_(self, value):
        value = complex(value)
        lib, h = self.ctx.lib, self.ctx.handle
        if is_double(self.code):
            check(h, lib.rls_fill_d(h, self.code, self.n, self.ptr, value.real, value.imag), "rls_fill_d")
        else:
            check(h, lib.rls_fill(h, self.code, self.n, self.ptr, value.real, value.imag), "rls_fill")
        return self

    def _reduce(self, name, *ptrs):
        lib, h = self.ctx.lib, self.ctx.handle
        if is_double(self.code):
            r = (C.c_double * 2)()
            check(h, getattr(lib, name + "_d")(h, self.code, self.n, *ptrs, r), name + "_d")
        else:
            r = (C.c_float * 2)()
            check(h, getattr(lib, name)(h, self.code, self.n, *ptrs, r), name)
        return r

    def _same(self, *others):
        """operands of one launch share the element type (two precisions coexist since round 6: a Float32 vector handed to a
        Float64 kernel would be read past its end)"""
        for o in others:
            if o.dtype != self.dtype:
                raise TypeError(f"element types differ: {self.dtype} and {o.dtype} (no mixed-precision broadcasts; convert on the host)")

    def norm(self) -> float:
        return float(self._reduce("rls_nrm2", self.ptr)[0])

    def norm1(self) -> float:
        return float(self._reduce("rls_asum", self.ptr)[0])

    def dot(self, other: "DeviceVector"):
        """dot(self, other) = conj(self) . other"""
        self._same(other)
        r = self._reduce("rls_dotc", self.ptr, other.ptr)
        return complex(r[0], r[1]) if self.code in (C32, C64) else float(r[0])

    def rmul_(self, a):
        a = complex(a)
        lib, h = self.ctx.lib, self.ctx.handle
        if is_double(self.code):
            check(h, lib.rls_scal_d(h, self.code, self.n, a.real, a.imag, self.ptr), "rls_scal_d")
        else:
            check(h, lib.rls_scal(h, self.code, self.n, a.real, a.imag, self.ptr), "rls_scal")
        return self

    def axpy_(self, a, x: "DeviceVector"):
        """self .+= a .* x"""
        self._same(x)
        a = complex(a)
        lib, h = self.ctx.lib, self.ctx.handle
        if is_double(self.code):
            check(h, lib.rls_axpy_d(h, self.code, self.n, a.real, a.imag, x.ptr, self.ptr), "rls_axpy_d")
        else:
            check(h, lib.rls_axpy(h, self.code, self.n, a.real, a.imag, x.ptr, self.ptr), "rls_axpy")
        return self

    def axpby_(self, a, x: "DeviceVector", b):
        """self = a x + b self"""
        return self.lincomb_(a, x, b, self)

    def lincomb_(self, a, x: "DeviceVector", b, y: "DeviceVector"):
        """self = a x + b y"""
        self._same(x, y)
        a, b = complex(a), complex(b)
        lib, h = self.ctx.lib, self.ctx.handle
        if is_double(self.code):
            check(h, lib.rls_lincomb_d(h, self.code, self.n, a.real, a.imag, x.ptr, b.real, b.imag, y.ptr, self.ptr), "rls_lincomb_d")
        else:
            check(h, lib.rls_lincomb(h, self.code, self.n, a.real, a.imag, x.ptr, b.real, b.imag, y.ptr, self.ptr),
                  "rls_lincomb")
        return self

    def stats(self):
        """(min, max, sum, sum of squares) of the real parts and max |x|, one device pass (rls_stats)"""
        out = (C.c_double * 5)()
        check(self.ctx.handle, self.ctx.lib.rls_stats(self.ctx.handle, self.code, self.n, self.ptr, out), "rls_stats")
        return [float(v) for v in out]

    def shift_scale_(self, shift, scale, inverse: bool = False):
        """Float32 only: x = (x - shift) / scale, or with inverse: x = x * scale + shift (src/Transforms.jl)"""
        if self.dtype != np.float32:
            raise TypeError("shift_scale_ acts on Float32 vectors")
        check(self.ctx.handle, self.ctx.lib.rls_shift_scale(self.ctx.handle, self.n, self.ptr, float(shift), float(scale),
                                                            1 if inverse else 0), "rls_shift_scale")
        return self

    def __len__(self):
        return self.n


class DeviceMatrix:
    """Dense M x N operator in HBM, column-major with leading dimension lda (Julia `Matrix`)."""

    def __init__(self, M: int, N: int, dtype, ctx: Optional[Context] = None, lda: Optional[int] = None):
        self.ctx = ctx or default_context()
        self.M, self.N = int(M), int(N)
        self.lda = int(lda if lda is not None else max(self.M, 1))
        self.dtype = np.dtype(dtype)
        self.code = dtype_code(self.dtype)
        self._buf = _DeviceBuffer(self.ctx, self.lda * self.N * self.dtype.itemsize)
        self.ptr = self._buf.ptr
        self._op = None

    @classmethod
    def from_host(cls, A, ctx: Optional[Context] = None) -> "DeviceMatrix":
        A = np.asarray(A)
        if A.ndim != 2:
            raise ValueError("DeviceMatrix.from_host expects a 2-D array")
        Af = np.asfortranarray(A)
        m = cls(A.shape[0], A.shape[1], Af.dtype, ctx)
        lib, h = m.ctx.lib, m.ctx.handle
        check(h, lib.rls_memcpy_h2d(h, m.ptr, Af.ctypes.data, Af.nbytes), "rls_memcpy_h2d")
        return m

    def to_host(self) -> np.ndarray:
        out = np.empty((self.lda, self.N), dtype=self.dtype, order="F")
        lib, h = self.ctx.lib, self.ctx.handle
        check(h, lib.rls_memcpy_d2h(h, out.ctypes.data, self.ptr, out.nbytes), "rls_memcpy_d2h")
        return out[: self.M, :]

    @property
    def shape(self):
        return (self.M, self.N)

    def size(self, i: int) -> int:  # 1-based like Julia's size(A, i)
        return (self.M, self.N)[i - 1]

    def fill_(self, value):
        """A .= value (every stored element, padding rows of lda included)"""
        value = complex(value)
        lib, h = self.ctx.lib, self.ctx.handle
        if is_double(self.code):
            check(h, lib.rls_fill_d(h, self.code, self.lda * self.N, self.ptr, value.real, value.imag), "rls_fill_d")
        else:
            check(h, lib.rls_fill(h, dtype_code(self.dtype), self.lda * self.N, self.ptr, value.real, value.imag), "rls_fill")
        return self

    def column(self, j: int) -> DeviceVector:
        """b[:, j] (0-based j) as a fresh vector: the reference copies columns (src/MultiThreading.jl:35)"""
        v = DeviceVector(self.M, self.dtype, self.ctx)
        lib, h = self.ctx.lib, self.ctx.handle
        off = j * self.lda * self.dtype.itemsize
        check(h, lib.rls_memcpy_d2d(h, v.ptr, self.ptr + off, self.M * self.dtype.itemsize), "rls_memcpy_d2d")
        return v

    def column_view(self, j: int) -> DeviceVector:
        """view(b, :, j): shares the matrix's memory (in-place operations on one column)"""
        off = (self.ptr - self._buf.ptr) + j * self.lda * self.dtype.itemsize
        return DeviceVector(self.M, self.dtype, self.ctx, _buf=self._buf, _offset=off)

    # --- mul! -------------------------------------------------------------------------------
    def gemv_(self, op: int, x: DeviceVector, y: DeviceVector, alpha=1.0, beta=0.0):
        """y = alpha * op(A) * x + beta * y     (5-arg mul!)"""
        alpha, beta = complex(alpha), complex(beta)
        nx, ny = (self.N, self.M) if op == OP_N else (self.M, self.N)
        if x.n != nx or y.n != ny:
            raise ValueError(f"gemv: dimension mismatch: A is {self.M}x{self.N}, x {x.n}, y {y.n}, op {op}")
        if x.dtype != self.dtype or y.dtype != self.dtype:
            raise TypeError(f"gemv: element types differ: A {self.dtype}, x {x.dtype}, y {y.dtype}")
        lib, h = self.ctx.lib, self.ctx.handle
        if is_double(self.code):
            check(h, lib.rls_gemv_d(h, self.code, op, self.M, self.N, alpha.real, alpha.imag, self.ptr, self.lda, x.ptr,
                                    beta.real, beta.imag, y.ptr), "rls_gemv_d")
        else:
            check(h, lib.rls_gemv(h, self.code, op, self.M, self.N, alpha.real, alpha.imag, self.ptr, self.lda, x.ptr,
                                  beta.real, beta.imag, y.ptr), "rls_gemv")
        return y

    def mul_(self, y: DeviceVector, x: DeviceVector, alpha=1.0, beta=0.0):
        return self.gemv_(OP_N, x, y, alpha, beta)

    def mul_adj_(self, x: DeviceVector, y: DeviceVector, alpha=1.0, beta=0.0):
        return self.gemv_(OP_C, y, x, alpha, beta)

    def mul_transpose_(self, x: DeviceVector, y: DeviceVector, alpha=1.0, beta=0.0):
        return self.gemv_(OP_T, y, x, alpha, beta)

    def __matmul__(self, x: DeviceVector) -> DeviceVector:  # allocating A * x  (src/ADMM.jl:203)
        return self.mul_(DeviceVector(self.M, self.dtype, self.ctx), x)

    def gram(self) -> "DeviceMatrix":
        """explicit AHA = A' * A on device (src/CGNR.jl:49); pass as AHA= for Gram mode"""
        G = DeviceMatrix(self.N, self.N, self.dtype, self.ctx)
        lib, h = self.ctx.lib, self.ctx.handle
        check(h, lib.rls_gram(h, self.code, self.M, self.N, self.ptr, self.lda, G.ptr, G.lda), "rls_gram")
        return G

    def rownorm2(self) -> "DeviceVector":
        """rownorm²(A, m) for every row m (src/Utils.jl:20-23; GPU ext NormalizedRegularization.jl:1-5): real vector"""
        lib, h = self.ctx.lib, self.ctx.handle
        if is_double(self.code):
            out = DeviceVector(self.M, np.float64, self.ctx)
            check(h, lib.rls_rownorm2_d(h, self.code, self.M, self.N, self.ptr, self.lda, out.ptr), "rls_rownorm2_d")
            return out
        out = DeviceVector(self.M, np.float32, self.ctx)
        check(h, lib.rls_rownorm2(h, self.code, self.M, self.N, self.ptr, self.lda, out.ptr), "rls_rownorm2")
        return out

    def scale_rows(self, w: "DeviceVector") -> "DeviceMatrix":
        """diag(w) * A as a new dense matrix (ProdOp(WeightingOp(w), A) materialised)"""
        if w.n != self.M or w.dtype != self.dtype:
            raise ValueError("scale_rows: weights must have length size(A, 1) and the element type of A")
        B = DeviceMatrix(self.M, self.N, self.dtype, self.ctx)
        lib, h = self.ctx.lib, self.ctx.handle
        fn = lib.rls_scale_rows_d if is_double(self.code) else lib.rls_scale_rows
        check(h, fn(h, self.code, self.M, self.N, w.ptr, self.ptr, self.lda, B.ptr, B.lda), "rls_scale_rows")
        return B

    def normal_operator(self) -> "NormalOperator":
        """A' * A as the unchanged constructors evaluate it: lazy, matrix-free (two GEMVs per apply)"""
        return NormalOperator(self)


def _csc_from_host(S):
    """(colptr int64[N + 1], rowval int32[nnz], nzval, (M, N)) -- contiguous, 0-based -- from that tuple or from a scipy.sparse
    matrix (converted to CSC with sorted indices, duplicates summed).  scipy is imported only for the second form."""
    if isinstance(S, (tuple, list)):
        if len(S) != 4:
            raise ValueError("DeviceSparseMatrix.from_host expects (colptr, rowval, nzval, (M, N)) or a scipy.sparse matrix")
        colptr, rowval, nzval, shape = S
    elif hasattr(S, "tocsc"):
        S = S.tocsc(copy=True)
        S.sum_duplicates()
        S.sort_indices()
        colptr, rowval, nzval, shape = S.indptr, S.indices, S.data, S.shape
    else:
        raise TypeError("DeviceSparseMatrix.from_host expects (colptr, rowval, nzval, (M, N)) or a scipy.sparse matrix")
    M, N = (int(s) for s in shape)
    nzval = np.ascontiguousarray(nzval)
    dtype_code(nzval.dtype)   # (TypeError for an element type the backend does not compute in)
    colptr, rowval = np.asarray(colptr), np.asarray(rowval)
    if colptr.ndim != 1 or rowval.ndim != 1 or nzval.ndim != 1 or colptr.dtype.kind not in "iu" or rowval.dtype.kind not in "iu":
        raise ValueError("colptr, rowval and nzval are 1-D arrays, colptr and rowval of integers")
    if M < 1 or N < 1 or M >= 2 ** 31 or N >= 2 ** 31 or colptr.size != N + 1:
        raise ValueError(f"a sparse {M} x {N} matrix needs 1 <= M, N < 2^31 and {N + 1} column pointers, got {colptr.size}")
    if colptr[-1] != rowval.size or rowval.size != nzval.size:
        raise ValueError(f"nnz = colptr[N] = {int(colptr[-1])}, but rowval has {rowval.size} and nzval {nzval.size} entries")
    if rowval.size and (rowval.min() < 0 or rowval.max() >= 2 ** 31):
        raise ValueError("row indices must lie in [0, M)")
    return np.ascontiguousarray(colptr, dtype=np.int64), np.ascontiguousarray(rowval, dtype=np.int32), nzval, (M, N)


class DeviceSparseMatrix:
    """Sparse M x N operator in HBM (Julia `SparseMatrixCSC`): the CSC triple as given and a CSR copy, so that A x, A^T y and A^H y
    are all gathers (rls_sparse, csrc/sparse.hip).  Served by CGNR, FISTA and Kaczmarz; `to_dense()` is the way to everything else."""

    def __init__(self, csc, ctx: Optional[Context] = None):
        colptr, rowval, nzval, (M, N) = csc
        lib = _lib.load()
        # validation runs on the host, ahead of any context: a malformed matrix is a ValueError on a machine without a device, too
        # (no outputs: the checks alone; the one transpose of a construction is the one inside rls_sparse_create)
        nnz = int(nzval.size)
        if lib.rls_sparse_csr_from_csc_host(dtype_code(nzval.dtype), M, N, colptr.ctypes.data, rowval.ctypes.data, nzval.ctypes.data,
                                            None, None, None) != 0:
            raise ValueError("not a valid CSC matrix: colptr[0] = 0 and non-decreasing, row indices in [0, M) and strictly "
                             "increasing inside a column (no duplicates)")
        self.ctx = ctx or default_context()
        self.M, self.N, self.nnz = M, N, nnz
        self.dtype = np.dtype(nzval.dtype)
        self.code = dtype_code(self.dtype)
        self.double = is_double(self.code)
        h = C.c_void_p()
        check(self.ctx.handle, lib.rls_sparse_create(self.ctx.handle, self.code, M, N, colptr.ctypes.data, rowval.ctypes.data,
                                                     nzval.ctypes.data, C.byref(h)), "rls_sparse_create")
        self.handle = h

    @classmethod
    def from_host(cls, S, ctx: Optional[Context] = None) -> "DeviceSparseMatrix":
        return cls(_csc_from_host(S), ctx)

    def to_host(self):
        """(colptr, rowval, nzval, (M, N)): the CSC triple, downloaded from the device (no host copy is kept)"""
        colptr, rowval, nzval = np.empty(self.N + 1, np.int64), np.empty(self.nnz, np.int32), np.empty(self.nnz, self.dtype)
        check(self.ctx.handle, self.ctx.lib.rls_sparse_to_host(self.handle, colptr.ctypes.data, rowval.ctypes.data if self.nnz else None,
                                                               nzval.ctypes.data if self.nnz else None), "rls_sparse_to_host")
        return colptr, rowval, nzval, (self.M, self.N)

    @property
    def shape(self):
        return (self.M, self.N)

    def size(self, i: int) -> int:  # 1-based like Julia's size(A, i)
        return (self.M, self.N)[i - 1]

    def variant(self, op: int) -> int:
        """lanes per output row a product in direction `op` runs with (rls_sparse_variant)"""
        v = C.c_int32()
        check(self.ctx.handle, self.ctx.lib.rls_sparse_variant(self.handle, op, C.byref(v)), "rls_sparse_variant")
        return v.value

    def spmv_(self, op: int, x: DeviceVector, y: DeviceVector, alpha=1.0, beta=0.0):
        """y = alpha * op(A) * x + beta * y     (5-arg mul!)"""
        alpha, beta = complex(alpha), complex(beta)
        nx, ny = (self.N, self.M) if op == OP_N else (self.M, self.N)
        if x.n != nx or y.n != ny:
            raise ValueError(f"mul: dimension mismatch: A is {self.M}x{self.N}, x {x.n}, y {y.n}, op {op}")
        if x.dtype != self.dtype or y.dtype != self.dtype:
            raise TypeError(f"mul: element types differ: A {self.dtype}, x {x.dtype}, y {y.dtype}")
        check(self.ctx.handle, self.ctx.lib.rls_sparse_mul(self.handle, op, alpha.real, alpha.imag, x.ptr, beta.real, beta.imag, y.ptr),
              "rls_sparse_mul")
        return y

    def mul_(self, y: DeviceVector, x: DeviceVector, alpha=1.0, beta=0.0):
        return self.spmv_(OP_N, x, y, alpha, beta)

    def mul_adj_(self, x: DeviceVector, y: DeviceVector, alpha=1.0, beta=0.0):
        return self.spmv_(OP_C, y, x, alpha, beta)

    def mul_transpose_(self, x: DeviceVector, y: DeviceVector, alpha=1.0, beta=0.0):
        return self.spmv_(OP_T, y, x, alpha, beta)

    def __matmul__(self, x: DeviceVector) -> DeviceVector:
        return self.mul_(DeviceVector(self.M, self.dtype, self.ctx), x)

    def rownorm2(self) -> "DeviceVector":
        """rownorm²(A, m) for every row m (src/Utils.jl:26-33): vector of the element type's real type"""
        out = DeviceVector(self.M, np.float64 if self.double else np.float32, self.ctx)
        check(self.ctx.handle, self.ctx.lib.rls_sparse_rownorm2(self.handle, out.ptr), "rls_sparse_rownorm2")
        return out

    def to_dense(self) -> DeviceMatrix:
        """Matrix(A): the way to Gram mode (`A.to_dense().gram()`) and to the solvers that take dense operators only"""
        D = DeviceMatrix(self.M, self.N, self.dtype, self.ctx)
        check(self.ctx.handle, self.ctx.lib.rls_sparse_to_dense(self.handle, D.ptr, D.lda), "rls_sparse_to_dense")
        return D

    def normal_operator(self) -> "SparseNormalOperator":
        """A' * A, lazy: two sparse products per apply"""
        return SparseNormalOperator(self)

    def __del__(self):
        try:
            if self.handle and self.ctx.handle:
                self.ctx.lib.rls_sparse_destroy(self.handle)
        except Exception:
            pass
        self.handle = None


class SparseNormalOperator:
    """Lazy A^H A of a DeviceSparseMatrix: size N x N, eltype of A.  It is also the operator object the primitive loops of CGNR
    and FISTA run on: M, N, code, double, mul_normal_, and no plan handle."""

    handle = None   # no rls_operator: the device plans take dense operators only
    sparse = True
    primitives = True   # CGNR and FISTA run their loops on the primitives (solvers._sparse_primitives)
    gram = None

    def __init__(self, A: DeviceSparseMatrix):
        self.A = A
        self.dtype, self.code, self.double = A.dtype, A.code, A.double
        self.ctx = A.ctx
        self.M, self.N = A.M, A.N
        self.shape = (A.N, A.N)
        self._t = None

    def size(self, i: int) -> int:
        return self.A.N

    def mul_normal_(self, v: DeviceVector, p: DeviceVector):
        if self._t is None:
            self._t = DeviceVector(self.M, self.dtype, self.ctx)
        self.A.mul_(self._t, p)
        return self.A.mul_adj_(v, self._t)

    def mul_(self, v: DeviceVector, p: DeviceVector):
        return self.mul_normal_(v, p)


class _MatrixFreeOperator:
    """What SamplingOp, FFTOp and their product share: the operator protocol (size, mul_, mul_adj_, normal_operator) and what the
    primitive loops of CGNR and FISTA read from an operator object -- M, N, code, double, dtype, ctx, mul_normal_ -- with no plan
    handle and no Gram matrix: the device plans take dense operators only."""

    handle = None       # no rls_operator
    gram = None
    primitives = True   # CGNR and FISTA run their loops on the primitives (solvers._sparse_primitives)
    matrix_free = True

    @property
    def shape(self):
        return (self.M, self.N)

    def size(self, i: int) -> int:  # 1-based like Julia's size(A, i)
        return (self.M, self.N)[i - 1]

    def _check(self, out: DeviceVector, n_out: int, inp: DeviceVector, n_in: int):
        if inp.n != n_in or out.n != n_out:
            raise ValueError(f"mul: dimension mismatch: the operator is {self.M}x{self.N}, input {inp.n}, output {out.n}")
        if inp.dtype != self.dtype or out.dtype != self.dtype:
            raise TypeError(f"mul: element types differ: operator {self.dtype}, input {inp.dtype}, output {out.dtype}")

    def __matmul__(self, x: DeviceVector) -> DeviceVector:
        return self.mul_(DeviceVector(self.M, self.dtype, self.ctx), x)

    def normal_operator(self) -> "MatrixFreeNormalOperator":
        """A' * A, lazy: one call of the operator's own normal product per apply"""
        return MatrixFreeNormalOperator(self)


def _sampling_pattern(pattern, n: int) -> np.ndarray:
    """the 0-based sampling indices as a contiguous int32 array: every one inside [0, n), none twice (ValueError otherwise)"""
    if isinstance(pattern, DeviceVector):
        raise TypeError("SamplingOp: the pattern is a host array of integers (device vectors hold the four floating-point element types)")
    idx = np.asarray(pattern)
    if idx.ndim != 1 or idx.size < 1 or idx.dtype.kind not in "iu":
        raise ValueError("SamplingOp: pattern is a non-empty 1-D array of 0-based integer indices")
    if idx.min() < 0 or idx.max() >= n:
        raise ValueError(f"SamplingOp: an index lies outside [0, {n})")
    if np.unique(idx).size != idx.size:
        raise ValueError("SamplingOp: an index is repeated")
    return np.ascontiguousarray(idx, dtype=np.int32)


class SamplingOp(_MatrixFreeOperator):
    """LinearOperatorCollection.SamplingOp(T; pattern, shape) (docs/src/literate/examples/compressed_sensing.jl): y = x[pattern], size
    (len(pattern), prod(shape)).  `pattern` holds 0-based indices into the column-major image."""

    def __init__(self, dtype, pattern, shape, ctx: Optional[Context] = None):
        self.dtype = np.dtype(dtype)
        self.code = dtype_code(self.dtype)
        self.double = is_double(self.code)
        self.image_shape = tuple(int(s_) for s_ in np.atleast_1d(shape))
        if not self.image_shape or min(self.image_shape) < 1:
            raise ValueError("SamplingOp: shape must hold positive extents")
        self.N = int(np.prod(self.image_shape))
        if self.N >= 2 ** 31:
            raise ValueError("SamplingOp: prod(shape) must be below 2^31")
        idx = _sampling_pattern(pattern, self.N)   # (on the host, ahead of any context)
        self.M = int(idx.size)
        self.ctx = ctx or default_context()
        h = C.c_void_p()
        check(self.ctx.handle, self.ctx.lib.rls_sampling_create(self.ctx.handle, self.code, self.N, self.M, idx.ctypes.data, C.byref(h)),
              "rls_sampling_create")
        self._h = h

    def _mul(self, op: int, x: DeviceVector, y: DeviceVector, alpha, beta):
        alpha, beta = complex(alpha), complex(beta)
        check(self.ctx.handle, self.ctx.lib.rls_sampling_mul(self._h, op, alpha.real, alpha.imag, x.ptr, beta.real, beta.imag, y.ptr),
              "rls_sampling_mul")
        return y

    def mul_(self, y: DeviceVector, x: DeviceVector, alpha=1.0, beta=0.0):
        self._check(y, self.M, x, self.N)
        return self._mul(OP_N, x, y, alpha, beta)

    def mul_adj_(self, x: DeviceVector, y: DeviceVector, alpha=1.0, beta=0.0):
        self._check(x, self.N, y, self.M)
        return self._mul(OP_C, y, x, alpha, beta)

    def mul_transpose_(self, x: DeviceVector, y: DeviceVector, alpha=1.0, beta=0.0):
        self._check(x, self.N, y, self.M)
        return self._mul(OP_T, y, x, alpha, beta)

    def mul_normal_(self, v: DeviceVector, p: DeviceVector):
        """v = mask .* p"""
        self._check(v, self.N, p, self.N)
        check(self.ctx.handle, self.ctx.lib.rls_sampling_mul_normal(self._h, p.ptr, v.ptr), "rls_sampling_mul_normal")
        return v

    def __del__(self):
        try:
            if self._h and self.ctx.handle:
                self.ctx.lib.rls_sampling_destroy(self._h)
        except Exception:
            pass
        self._h = None


class FFTOp(_MatrixFreeOperator):
    """LinearOperatorCollection.FFTOp(T; shape, shift = true, unitary = true) on 1-D and 2-D power-of-two shapes: with the image
    column-major, F x = fftshift(fftn(ifftshift(x))) / sqrt(n); `shift=False` drops the two shifts, `unitary=False` the scale.  The
    adjoint is the conjugate transpose."""

    def __init__(self, dtype, shape, shift: bool = True, unitary: bool = True, ctx: Optional[Context] = None):
        self.dtype = np.dtype(dtype)
        self.code = dtype_code(self.dtype)
        if self.dtype.kind != "c":
            raise TypeError(f"FFTOp: a complex element type is required, got {self.dtype}")
        self.double = is_double(self.code)
        self.image_shape = tuple(int(s_) for s_ in np.atleast_1d(shape))
        if not self.image_shape or min(self.image_shape) < 1:
            raise ValueError("FFTOp: shape must hold positive extents")
        ext = [s_ for s_ in self.image_shape if s_ != 1]
        if len(ext) > 2:
            raise ValueError("FFTOp: 1-D and 2-D shapes only")
        if any(s_ & (s_ - 1) for s_ in ext):
            raise ValueError(f"FFTOp: extents must be powers of two, got {self.image_shape}")
        self.shift, self.unitary = bool(shift), bool(unitary)
        self.M = self.N = int(np.prod(self.image_shape))
        self.ctx = ctx or default_context()
        cs = (C.c_int64 * len(self.image_shape))(*self.image_shape)
        h = C.c_void_p()
        flags = (_lib.FFT_SHIFT if self.shift else 0) | (_lib.FFT_UNITARY if self.unitary else 0)
        st = self.ctx.lib.rls_fft_create(self.ctx.handle, self.code, len(self.image_shape), cs, flags, C.byref(h))
        if st == -2:   # RLS_E_UNSUPPORTED: a line longer than the kernels' LDS holds
            raise ValueError(f"FFTOp: shape {self.image_shape} is not supported: " + (self.ctx.lib.rls_last_error_string(self.ctx.handle) or b"").decode())
        check(self.ctx.handle, st, "rls_fft_create")
        self._h = h
        self._t = None

    def variant(self) -> int:
        """1: a transform is one single-workgroup launch, 0: one launch per dimension (rls_fft_variant)"""
        v = C.c_int32()
        check(self.ctx.handle, self.ctx.lib.rls_fft_variant(self._h, C.byref(v)), "rls_fft_variant")
        return v.value

    def mul_(self, y: DeviceVector, x: DeviceVector):
        self._check(y, self.N, x, self.N)
        check(self.ctx.handle, self.ctx.lib.rls_fft_apply(self._h, 0, x.ptr, y.ptr), "rls_fft_apply")
        return y

    def mul_adj_(self, x: DeviceVector, y: DeviceVector):
        self._check(x, self.N, y, self.N)
        check(self.ctx.handle, self.ctx.lib.rls_fft_apply(self._h, 1, y.ptr, x.ptr), "rls_fft_apply")
        return x

    def mul_normal_(self, v: DeviceVector, p: DeviceVector):
        """v = F^H (F p): the forward into v, the adjoint in place"""
        self.mul_(v, p)
        return self.mul_adj_(v, v)

    def __del__(self):
        try:
            if self._h and self.ctx.handle:
                self.ctx.lib.rls_fft_destroy(self._h)
        except Exception:
            pass
        self._h = None


class SampledFFTOp(_MatrixFreeOperator):
    """ProdOp(SamplingOp, FFTOp): y = S (F x), the operator of the reference's compressed-sensing example behind a Fourier transform
    (rls_fft_sampled_mul); its normal operator F^H diag(mask) F is one launch where the image fits a workgroup's LDS."""

    def __init__(self, S: SamplingOp, F: FFTOp):
        if S.ctx is not F.ctx or S.dtype != F.dtype or S.N != F.N:
            raise ValueError(f"ProdOp: SamplingOp ({S.M}x{S.N}, {S.dtype}) and FFTOp ({F.M}x{F.N}, {F.dtype}) must share context, element type "
                             "and prod(shape)")
        self.S, self.F = S, F
        self.dtype, self.code, self.double, self.ctx = F.dtype, F.code, F.double, F.ctx
        self.M, self.N = S.M, F.N
        self.image_shape = F.image_shape

    def mul_(self, y: DeviceVector, x: DeviceVector):
        self._check(y, self.M, x, self.N)
        check(self.ctx.handle, self.ctx.lib.rls_fft_sampled_mul(self.F._h, self.S._h, OP_N, x.ptr, y.ptr), "rls_fft_sampled_mul")
        return y

    def mul_adj_(self, x: DeviceVector, y: DeviceVector):
        self._check(x, self.N, y, self.M)
        check(self.ctx.handle, self.ctx.lib.rls_fft_sampled_mul(self.F._h, self.S._h, OP_C, y.ptr, x.ptr), "rls_fft_sampled_mul")
        return x

    def mul_normal_(self, v: DeviceVector, p: DeviceVector):
        self._check(v, self.N, p, self.N)
        check(self.ctx.handle, self.ctx.lib.rls_fft_sampled_mul_normal(self.F._h, self.S._h, p.ptr, v.ptr), "rls_fft_sampled_mul_normal")
        return v


class RadonOp(_MatrixFreeOperator):
    """RadonOp(T; angles, shape) of the reference's computed-tomography example (docs/src/literate/examples/computed_tomography.jl): the
    exact parallel-beam line integral of a piecewise-constant image (csrc/radon.hip).  The image is column-major,
    `angles` in radians; the sinogram is detectors x len(angles), detector fastest.  `detectors=None`: 2 ceil(hypot(shape) / 2) + 1
    bins of unit spacing, every ray that meets the image.  Unlike RadonKA.jl: no inscribed-circle mask, no attenuation, and the default
    detector count is not shape[0] - 1."""

    def __init__(self, dtype, angles, shape, detectors=None, ctx: Optional[Context] = None):
        self.dtype = np.dtype(dtype)
        self.code = dtype_code(self.dtype)
        self.double = is_double(self.code)
        try:
            self.image_shape = tuple(int(s_) for s_ in np.atleast_1d(shape))
        except (TypeError, ValueError):
            raise ValueError("RadonOp: shape must hold two positive extents") from None
        if len(self.image_shape) != 2 or min(self.image_shape) < 1:
            raise ValueError("RadonOp: shape must hold two positive extents")
        try:
            ang = np.ascontiguousarray(np.atleast_1d(np.asarray(angles, dtype=np.float64)))
        except (TypeError, ValueError):
            raise ValueError("RadonOp: angles is a non-empty 1-D array of finite angles in radians") from None
        if ang.ndim != 1 or ang.size < 1 or not np.all(np.isfinite(ang)):
            raise ValueError("RadonOp: angles is a non-empty 1-D array of finite angles in radians")
        if detectors is None:
            detectors = 2 * int(np.ceil(np.hypot(*self.image_shape) / 2)) + 1
        if int(detectors) != detectors or detectors < 1:
            raise ValueError("RadonOp: detectors must be a positive integer")
        self.angles, self.detectors = ang, int(detectors)
        self.M, self.N = self.detectors * int(ang.size), self.image_shape[0] * self.image_shape[1]
        if self.M >= 2 ** 31 or self.N >= 2 ** 31:
            raise ValueError("RadonOp: detectors * len(angles) and prod(shape) must be below 2^31")
        self.ctx = ctx or default_context()   # (every refusal above is raised ahead of any context)
        h = C.c_void_p()
        check(self.ctx.handle, self.ctx.lib.rls_radon_create(self.ctx.handle, self.code, self.image_shape[0], self.image_shape[1], ang.size,
                                                             ang.ctypes.data, self.detectors, C.byref(h)), "rls_radon_create")
        self._h = h

    def _mul(self, op: int, x: DeviceVector, y: DeviceVector, alpha, beta):
        alpha, beta = complex(alpha), complex(beta)
        check(self.ctx.handle, self.ctx.lib.rls_radon_mul(self._h, op, alpha.real, alpha.imag, x.ptr, beta.real, beta.imag, y.ptr),
              "rls_radon_mul")
        return y

    def mul_(self, y: DeviceVector, x: DeviceVector, alpha=1.0, beta=0.0):
        self._check(y, self.M, x, self.N)
        return self._mul(OP_N, x, y, alpha, beta)

    def mul_adj_(self, x: DeviceVector, y: DeviceVector, alpha=1.0, beta=0.0):
        self._check(x, self.N, y, self.M)
        return self._mul(OP_C, y, x, alpha, beta)

    def mul_transpose_(self, x: DeviceVector, y: DeviceVector, alpha=1.0, beta=0.0):
        self._check(x, self.N, y, self.M)
        return self._mul(OP_T, y, x, alpha, beta)

    def mul_normal_(self, v: DeviceVector, p: DeviceVector):
        """v = A^T (A p): the forward into the handle's workspace, then the adjoint"""
        self._check(v, self.N, p, self.N)
        check(self.ctx.handle, self.ctx.lib.rls_radon_mul_normal(self._h, p.ptr, v.ptr), "rls_radon_mul_normal")
        return v

    def to_dense(self) -> DeviceMatrix:
        """Matrix(A), every entry the bits the products use: for small operators and tests (M x N elements)"""
        A = DeviceMatrix(self.M, self.N, self.dtype, self.ctx)
        check(self.ctx.handle, self.ctx.lib.rls_radon_to_dense(self._h, A.ptr, A.lda), "rls_radon_to_dense")
        return A

    def lanes(self) -> int:
        """lanes per pixel the adjoint runs with under the context's current tune (rls_radon_lanes)"""
        v = C.c_int32()
        check(self.ctx.handle, self.ctx.lib.rls_radon_lanes(self._h, C.byref(v)), "rls_radon_lanes")
        return v.value

    def __del__(self):
        try:
            if self._h and self.ctx.handle:
                self.ctx.lib.rls_radon_destroy(self._h)
        except Exception:
            pass
        self._h = None


class NFFTOp(_MatrixFreeOperator):
    """NFFTOp(T; nodes, shape): non-uniform Fourier sampling without a stored matrix (csrc/nfft.hip),
    y_j = sum_k x_k exp(-2 pi i k . nodes[:, j]) over k_d in {-floor(N_d / 2), ..., ceil(N_d / 2) - 1}, no scale factor.  The image is
    column-major with one or two extents (unit extents are dropped; they need not be powers of two); `nodes` is a host array d x J
    (a 1-D array of J nodes for a signal) with every entry in [-0.5, 0.5); `m` in 1 ... 8 is the half-width of the Kaiser-Bessel
    window, 2 m taps per dimension on a grid of the smallest power of two >= 2 N_d points.  The adjoint is the exact conjugate
    transpose of what the forward computes.  Unlike NFFT.jl: the oversampling is not a parameter, the window is fixed, nodes at 0.5
    are refused rather than wrapped, and there is no density compensation (ProdOp(WeightingOp, NFFTOp) stays refused) and no
    Toeplitz form of the normal operator."""

    MAX_EXTENT = {8: 4096, 16: 2048}   # by element size: the grid line 2 N_d must fit the FFT's 8192 / 4096 points

    def __init__(self, dtype, nodes, shape, m=4, ctx: Optional[Context] = None):
        self.dtype = np.dtype(dtype)
        self.code = dtype_code(self.dtype)
        if self.dtype.kind != "c":
            raise TypeError(f"NFFTOp: a complex element type is required, got {self.dtype}")
        self.double = is_double(self.code)
        try:
            self.image_shape = tuple(int(s_) for s_ in np.atleast_1d(shape))
        except (TypeError, ValueError):
            raise ValueError("NFFTOp: shape must hold one or two positive extents") from None
        if not self.image_shape or min(self.image_shape) < 1:
            raise ValueError("NFFTOp: shape must hold one or two positive extents")
        ext = [s_ for s_ in self.image_shape if s_ != 1] or [1]
        if len(ext) > 2:
            raise ValueError("NFFTOp: 1-D and 2-D shapes only")
        if max(ext) > self.MAX_EXTENT[self.dtype.itemsize]:
            raise ValueError(f"NFFTOp: an extent of {max(ext)} needs a grid line beyond the FFT's "
                             f"{2 * self.MAX_EXTENT[self.dtype.itemsize]} points for {self.dtype}")
        try:
            nu = np.asarray(nodes, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("NFFTOp: nodes is a d x J array of numbers in [-0.5, 0.5)") from None
        if nu.ndim == 1 and len(ext) == 1:
            nu = nu[None, :]
        if nu.ndim != 2 or nu.shape[0] != len(ext) or nu.shape[1] < 1:
            raise ValueError(f"NFFTOp: nodes must be {len(ext)} x J with J >= 1, got shape {nu.shape}")
        if nu.shape[1] >= 2 ** 31:
            raise ValueError("NFFTOp: the number of nodes must be below 2^31")
        if not np.all((nu >= -0.5) & (nu < 0.5)):   # (a NaN fails both)
            raise ValueError("NFFTOp: every node coordinate must lie in [-0.5, 0.5)")
        if isinstance(m, bool) or int(m) != m or not 1 <= m <= 8:
            raise ValueError("NFFTOp: m must be an integer in 1 ... 8")
        self.nodes, self.m = np.ascontiguousarray(nu), int(m)
        self.M, self.N = int(nu.shape[1]), int(np.prod(self.image_shape))
        self.ctx = ctx or default_context()   # (every refusal above is raised ahead of any context)
        cs = (C.c_int64 * len(self.image_shape))(*self.image_shape)
        h = C.c_void_p()
        st = self.ctx.lib.rls_nfft_create(self.ctx.handle, self.code, len(self.image_shape), cs, self.M, self.nodes.ctypes.data, self.m, C.byref(h))
        if st == -2:   # RLS_E_UNSUPPORTED
            raise ValueError(f"NFFTOp: shape {self.image_shape}, m = {self.m} is not supported: "
                             + (self.ctx.lib.rls_last_error_string(self.ctx.handle) or b"").decode())
        check(self.ctx.handle, st, "rls_nfft_create")
        self._h = h
        n = C.c_int64()
        check(self.ctx.handle, self.ctx.lib.rls_nfft_info(self._h, None, None, C.byref(n)), "rls_nfft_info")
        self.grid_points = n.value

    def _mul(self, op: int, x: DeviceVector, y: DeviceVector):
        check(self.ctx.handle, self.ctx.lib.rls_nfft_mul(self._h, op, x.ptr, y.ptr), "rls_nfft_mul")
        return y

    def mul_(self, y: DeviceVector, x: DeviceVector):
        self._check(y, self.M, x, self.N)
        return self._mul(OP_N, x, y)

    def mul_adj_(self, x: DeviceVector, y: DeviceVector):
        self._check(x, self.N, y, self.M)
        return self._mul(OP_C, y, x)

    def mul_transpose_(self, x: DeviceVector, y: DeviceVector):
        """refused (RLS_E_UNSUPPORTED): the operator is complex, its transpose is not its adjoint and nothing needs it"""
        self._check(x, self.N, y, self.M)
        return self._mul(OP_T, y, x)

    def mul_normal_(self, v: DeviceVector, p: DeviceVector):
        """v = A^H (A p): the forward into the handle's workspace, then the adjoint; the bits of the two calls.  v may be p"""
        self._check(v, self.N, p, self.N)
        check(self.ctx.handle, self.ctx.lib.rls_nfft_mul_normal(self._h, p.ptr, v.ptr), "rls_nfft_mul_normal")
        return v

    def to_dense(self) -> DeviceMatrix:
        """Matrix(A) by N forward applications to unit vectors, every entry the bits the product gives: for small operators and tests"""
        A = np.empty((self.M, self.N), self.dtype, order="F")
        y = DeviceVector(self.M, self.dtype, self.ctx)
        for k in range(self.N):
            e = np.zeros(self.N, self.dtype)
            e[k] = 1
            A[:, k] = self.mul_(y, DeviceVector.from_host(e, self.ctx)).to_host()
        return DeviceMatrix.from_host(A, self.ctx)

    def __del__(self):
        try:
            if self._h and self.ctx.handle:
                self.ctx.lib.rls_nfft_destroy(self._h)
        except Exception:
            pass
        self._h = None


class MatrixFreeNormalOperator:
    """Lazy A^H A of a SamplingOp, an FFTOp or their product: size N x N, eltype of A; mul_ is the operator's own normal product.
    Like SparseNormalOperator it is the operator object the primitive loops of CGNR and FISTA run on."""

    handle = None
    gram = None
    primitives = True
    matrix_free = True

    def __init__(self, A: _MatrixFreeOperator):
        self.A = A
        self.dtype, self.code, self.double, self.ctx = A.dtype, A.code, A.double, A.ctx
        self.M, self.N = A.M, A.N
        self.shape = (A.N, A.N)

    def size(self, i: int) -> int:
        return self.A.N

    def mul_normal_(self, v: DeviceVector, p: DeviceVector):
        return self.A.mul_normal_(v, p)

    def mul_(self, v: DeviceVector, p: DeviceVector):
        return self.A.mul_normal_(v, p)


class WeightingOp:
    """LinearOperatorCollection.WeightingOp(weights): diag(weights) (docs/src/literate/howto/normal_operator.jl:41)"""

    def __init__(self, weights: "DeviceVector"):
        self.weights = weights


def ProdOp(W, A):
    """ProdOp(SamplingOp, FFTOp): the matrix-free product S o F (SampledFFTOp).

    ProdOp(WeightingOp(w), A) (docs/src/literate/howto/normal_operator.jl:42, src/Utils.jl:23,102).  On a GPU with
    288 GB the weighted operator is materialised once as diag(w) A: A, its adjoint and the normal operator
    A^H W^H W A (`normalOperator`) then run on the same one-pass / matrix-core kernels as any dense matrix,
    instead of carrying a diagonal scale through every kernel."""
    if isinstance(W, SamplingOp) and isinstance(A, FFTOp):
        return SampledFFTOp(W, A)
    if not isinstance(W, WeightingOp) or isinstance(A, _MatrixFreeOperator):
        raise TypeError("ProdOp: only ProdOp(WeightingOp(w), A) with a dense A and ProdOp(SamplingOp, FFTOp) are supported")
    if isinstance(A, DeviceSparseMatrix):
        raise TypeError("ProdOp: a sparse A is not supported (ProdOp(WeightingOp(w), A.to_dense()) is the dense route)")
    w = W.weights
    if w.dtype != A.dtype:
        w = DeviceVector.from_host(w.to_host().astype(A.dtype), A.ctx)
    WA = A.scale_rows(w)
    WA.weights, WA.B = W.weights, A
    return WA


def normalOperator(A: DeviceMatrix) -> "NormalOperator":
    """LinearOperatorCollection.normalOperator(A) (docs/src/literate/howto/normal_operator.jl:43)"""
    return A.normal_operator()


class OperatorHandle:
    """rls_operator: forward matrix and/or Gram matrix bound to a context."""

    def __init__(self, A: Optional[DeviceMatrix], gram: Optional[DeviceMatrix] = None):
        src = A if A is not None else gram
        if src is None:
            raise ValueError("OperatorHandle needs A or a Gram matrix")
        self.ctx = src.ctx
        self.A, self.gram = A, gram
        self.dtype, self.code = src.dtype, src.code
        self.M = A.M if A is not None else 0
        self.N = A.N if A is not None else gram.N
        lib, h = self.ctx.lib, self.ctx.handle
        if gram is not None and (gram.M != self.N or gram.N != self.N):
            raise ValueError("Gram matrix must be N x N")
        self.double = is_double(self.code)
        self._t = None
        if self.double:
            # Float64 / ComplexF64: no rls_operator (the double-precision plans take raw pointers): v = AHA p is the explicit Gram GEMV
            # or the two GEMVs of the matrix-free normal operator, through rls_gemv_d
            self.handle = None
            return
        o = C.c_void_p()
        check(h, lib.rls_operator_create(h, self.code, self.M, self.N, A.ptr if A is not None else None,
                                         A.lda if A is not None else 0, C.byref(o)), "rls_operator_create")
        self.handle = o
        if gram is not None:
            check(h, lib.rls_operator_set_gram(o, gram.ptr, gram.lda), "rls_operator_set_gram")

    def mul_normal_(self, v: DeviceVector, p: DeviceVector):
        if self.double:
            if self.gram is not None:
                return self.gram.mul_(v, p)
            if self._t is None:
                self._t = DeviceVector(self.M, self.dtype, self.ctx)
            self.A.mul_(self._t, p)
            return self.A.mul_adj_(v, self._t)
        check(self.ctx.handle, self.ctx.lib.rls_operator_mul_normal(self.handle, p.ptr, v.ptr), "rls_operator_mul_normal")
        return v

    def __del__(self):
        try:
            if self.handle and self.ctx.handle:
                self.ctx.lib.rls_operator_destroy(self.handle)
        except Exception:
            pass
        self.handle = None


class NormalOperator:
    """Lazy A^H A (LinearOperatorCollection.normalOperator): size N x N, eltype of A."""

    def __init__(self, A: DeviceMatrix):
        self.A = A
        self.dtype = A.dtype
        self.ctx = A.ctx
        self.shape = (A.N, A.N)
        self._handle = None

    def size(self, i: int) -> int:
        return self.A.N

    def handle(self) -> OperatorHandle:
        if self._handle is None:
            self._handle = OperatorHandle(self.A)
        return self._handle

    def mul_(self, v: DeviceVector, p: DeviceVector):
        return self.handle().mul_normal_(v, p)
