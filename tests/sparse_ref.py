"""Sparse test inputs and their float64 restatements, NumPy only (no scipy): a CSC triple in the layout of Julia's SparseMatrixCSC
(0-based), its dense float64 / complex128 twin, the NumPy transpose to CSR and the sparse row sweep of Kaczmarz in float64.
tests/test_sparse_abi.py checks this file on the CPU first -- the sweep against the dense Kaczmarz restatement of
oracle/rls_oracle.py -- and the GPU tests compare the device against it."""
import numpy as np

DTYPES = (np.float32, np.complex64, np.float64, np.complex128)


def wide(dtype):
    """the float64 twin's element type"""
    return np.complex128 if np.dtype(dtype).kind == "c" else np.float64


def values(rng, n, dtype):
    """n values of `dtype`, away from zero, complex ones with non-zero imaginary parts"""
    dtype = np.dtype(dtype)
    rt = np.float32 if dtype in (np.float32, np.complex64) else np.float64
    v = (rng.uniform(0.25, 1.0, n) * rng.choice([-1.0, 1.0], n)).astype(rt)
    if dtype.kind == "c":
        v = v + 1j * (rng.uniform(0.25, 1.0, n) * rng.choice([-1.0, 1.0], n)).astype(rt)
    return v.astype(dtype)


def from_pattern(mask, dtype, seed):
    """CSC triple with the non-zero pattern `mask` (M x N booleans) and seeded values; returns (csc, dense twin)"""
    mask = np.asarray(mask, dtype=bool)
    M, N = mask.shape
    rng = np.random.default_rng(seed)
    cols, rows = np.nonzero(mask.T)            # column-major order: rows ascend inside a column
    nz = values(rng, rows.size, dtype)
    colptr = np.zeros(N + 1, np.int64)
    np.cumsum(np.bincount(cols, minlength=N), out=colptr[1:])
    D = np.zeros((M, N), wide(dtype))
    D[rows, cols] = nz
    return (colptr, rows.astype(np.int32), nz, (M, N)), D


def random_csc(M, N, fill, dtype, seed):
    rng = np.random.default_rng(seed)
    return from_pattern(rng.random((M, N)) < fill, dtype, seed + 1)


def row_lengths(lengths, N, dtype, seed):
    """row m has exactly lengths[m] non-zeros, at seeded columns"""
    rng = np.random.default_rng(seed)
    mask = np.zeros((len(lengths), N), bool)
    for m, n in enumerate(lengths):
        mask[m, rng.choice(N, size=int(n), replace=False)] = True
    return from_pattern(mask, dtype, seed + 1)


def with_holes(M, N, dtype, seed, long_row=None):
    """about one non-zero per row; rows 0, M - 1 and one in the middle empty, columns 0, N - 1 and one in the middle empty;
    `long_row`: that row gets min(200, N - 3) non-zeros"""
    rng = np.random.default_rng(seed)
    mask = np.zeros((M, N), bool)
    if N > 3:
        mask[np.arange(M), rng.integers(1, N - 1, M)] = True
    if long_row is not None and N > 3:
        mask[long_row, 1 + rng.choice(N - 2, size=min(200, N - 3), replace=False)] = True
    mask[[0, M // 2, M - 1], :] = False
    if long_row is not None:
        mask[long_row, 0] = False
    mask[:, [0, N // 2, N - 1]] = False
    return from_pattern(mask, dtype, seed + 1)


def csr_from_csc(csc):
    """(rowptr, colval, nzval): the NumPy transpose -- a stable sort by row keeps the columns ascending inside every row"""
    colptr, rowval, nzval, (M, N) = csc
    cols = np.repeat(np.arange(N, dtype=np.int32), np.diff(colptr))
    order = np.argsort(rowval, kind="stable")
    rowptr = np.zeros(M + 1, np.int64)
    np.cumsum(np.bincount(rowval, minlength=M), out=rowptr[1:])
    return rowptr, cols[order], nzval[order]


def dense(csc):
    colptr, rowval, nzval, (M, N) = csc
    D = np.zeros((M, N), wide(nzval.dtype))
    D[rowval, np.repeat(np.arange(N), np.diff(colptr))] = nzval
    return D


def rownorm2(csc):
    return (np.abs(dense(csc)) ** 2).sum(axis=1)


def sparse_sweep(csc, x, u, vl, rows, denom, eps_w, n_sweeps):
    """the row steps of rls_sparse_kaczmarz_sweep in float64, on the CSR rows, in place on copies: returns (x, vl)
    (tau: src/Utils.jl:89-100, alpha: src/Kaczmarz.jl:305, update: :532-539, vl: :307)"""
    rowptr, colval, nz = csr_from_csc(csc)
    W = wide(nz.dtype)
    nz = nz.astype(W)
    x, vl, u = np.array(x, dtype=W), np.array(vl, dtype=W), np.asarray(u).astype(W)
    denom = np.asarray(denom, dtype=np.float64)
    for _ in range(n_sweeps):
        for i, row in enumerate(rows):
            k = slice(rowptr[row], rowptr[row + 1])
            tau = np.sum(nz[k] * x[colval[k]])
            alpha = denom[i] * (u[row] - tau - eps_w * vl[row])
            x[colval[k]] += alpha * np.conj(nz[k])
            vl[row] += alpha * eps_w
    return x, vl


MALFORMED = ("colptr0", "decreasing", "row_range", "unsorted", "duplicate")


def malformed(kind):
    """a 4 x 3 Float32 triple that is wrong in exactly one way"""
    colptr = np.array([0, 2, 3, 5], np.int64)
    rowval = np.array([0, 2, 1, 1, 3], np.int32)
    nz = np.arange(1, 6, dtype=np.float32)
    if kind == "colptr0":
        colptr = np.array([1, 2, 3, 5], np.int64)
    elif kind == "decreasing":
        colptr = np.array([0, 3, 2, 5], np.int64)
    elif kind == "row_range":
        rowval[4] = 4
    elif kind == "unsorted":
        rowval[0], rowval[1] = 2, 0
    elif kind == "duplicate":
        rowval[3], rowval[4] = 3, 3
    else:
        raise KeyError(kind)
    return colptr, rowval, nz, (4, 3)
