"""CPU tests of the sparse operator's surface -- header, export table, ctypes table, null handles, the host transpose
rls_sparse_csr_from_csc_host, the Python class and its validation ahead of any context -- and of tests/sparse_ref.py, whose
float64 row sweep the GPU tests compare against: it is held to the dense Kaczmarz restatement of the oracle here first."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import rls_oracle as O
import sparse_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rls_mi355x.h")
SYMBOLS = ("rls_sparse_csr_from_csc_host", "rls_sparse_create", "rls_sparse_destroy", "rls_sparse_info", "rls_sparse_to_host", "rls_sparse_variant",
           "rls_sparse_mul", "rls_sparse_rownorm2", "rls_sparse_to_dense", "rls_sparse_kaczmarz_sweep")
CODE = {np.dtype(np.float32): 0, np.dtype(np.complex64): 1, np.dtype(np.float64): 2, np.dtype(np.complex128): 3}


def test_symbols_in_header_export_table_and_binding(rls):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    from rls_amd import _lib

    out = subprocess.run(["nm", "-D", "--defined-only", rls.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (rls_[a-z0-9_]+)", out))
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), f"{s} is not declared in the header"
        assert s in exported, f"{s} is not exported"
        assert s in _lib.PROTOTYPES, f"{s} is not in the ctypes table"
    assert sorted(s for s in _lib.PROTOTYPES if s.startswith("rls_sparse_")) == sorted(SYMBOLS)


def test_null_handles_are_invalid(rls):
    lib = rls.load()
    out = C.c_void_p()
    i64 = (C.c_int64 * 3)()
    v = C.c_int32()
    assert lib.rls_sparse_create(None, 0, 1, 1, None, None, None, C.byref(out)) == -1   # no context
    assert lib.rls_sparse_destroy(None) == -1
    assert lib.rls_sparse_info(None, i64, None, None) == -1
    assert lib.rls_sparse_variant(None, 0, C.byref(v)) == -1
    assert lib.rls_sparse_to_host(None, i64, None, None) == -1
    assert lib.rls_sparse_mul(None, 0, 1.0, 0.0, None, 0.0, 0.0, None) == -1
    assert lib.rls_sparse_rownorm2(None, None) == -1
    assert lib.rls_sparse_to_dense(None, None, 1) == -1
    assert lib.rls_sparse_kaczmarz_sweep(None, 1, None, 1, None, 1, None, 1, None, None, 1, 0.0, 1) == -1


def _transpose(lib, csc):
    colptr, rowval, nz, (M, N) = csc
    nnz = nz.size
    rp = np.full(M + 1, -7, np.int64)
    cv = np.full(max(nnz, 1), -7, np.int32)
    out = np.zeros(max(nnz, 1), nz.dtype)
    st = lib.rls_sparse_csr_from_csc_host(CODE[nz.dtype], M, N, colptr.ctypes.data, rowval.ctypes.data, nz.ctypes.data, rp.ctypes.data,
                                          cv.ctypes.data, out.ctypes.data)
    return st, rp, cv[:nnz], out[:nnz]


def _cases(dtype):
    """name -> CSC triple: the edge cases of the host transpose"""
    one = np.zeros((1, 1), bool)
    one[0, 0] = True
    full_row = np.zeros((6, 9), bool)
    full_row[2, :] = True
    full_row[4, 3] = True
    full_col = np.zeros((9, 6), bool)
    full_col[:, 3] = True
    full_col[5, 0] = True
    rng = np.random.default_rng(5)
    edges = rng.random((11, 13)) < 0.4
    edges[[0, -1], :] = False      # empty first and last row
    edges[:, [0, -1]] = False      # empty first and last column
    return {"1x1": SR.from_pattern(one, dtype, 1)[0], "nnz0": SR.from_pattern(np.zeros((7, 5), bool), dtype, 2)[0],
            "empty_edges": SR.from_pattern(edges, dtype, 3)[0], "full_row": SR.from_pattern(full_row, dtype, 4)[0],
            "full_col": SR.from_pattern(full_col, dtype, 5)[0], "random": SR.random_csc(37, 29, 0.2, dtype, 6)[0]}


@pytest.mark.parametrize("dtype", SR.DTYPES)
def test_host_transpose_equals_the_numpy_transpose(rls, dtype):
    lib = rls.load()
    for name, csc in _cases(dtype).items():
        st, rp, cv, nz = _transpose(lib, csc)
        assert st == 0, name
        rp_ref, cv_ref, nz_ref = SR.csr_from_csc(csc)
        assert np.array_equal(rp, rp_ref), name
        assert np.array_equal(cv, cv_ref), name
        assert nz.tobytes() == nz_ref.tobytes(), name
        for m in range(csc[3][0]):   # columns ascend strictly inside every row
            assert np.all(np.diff(cv[rp[m]:rp[m + 1]]) > 0), (name, m)


@pytest.mark.parametrize("kind", SR.MALFORMED)
def test_host_transpose_refuses_malformed_input(rls, kind):
    assert _transpose(rls.load(), SR.malformed(kind))[0] == -1   # RLS_E_INVALID


def test_host_transpose_refuses_bad_arguments(rls):
    lib = rls.load()
    csc = SR.random_csc(5, 4, 0.5, np.float32, 1)[0]
    colptr, rowval, nz, (M, N) = csc
    rp, cv, out = np.zeros(M + 1, np.int64), np.zeros(nz.size, np.int32), np.zeros(nz.size, nz.dtype)
    args = [0, M, N, colptr.ctypes.data, rowval.ctypes.data, nz.ctypes.data, rp.ctypes.data, cv.ctypes.data, out.ctypes.data]
    assert lib.rls_sparse_csr_from_csc_host(*args) == 0
    for pos, bad in ((0, 4), (0, -1), (1, 0), (2, 0), (1, 2 ** 31), (3, None), (4, None), (6, None)):
        a = list(args)
        a[pos] = bad
        assert lib.rls_sparse_csr_from_csc_host(*a) == -1, (pos, bad)
    # all three outputs null: the checks alone
    assert lib.rls_sparse_csr_from_csc_host(*args[:6], None, None, None) == 0
    for kind in SR.MALFORMED:
        cp, rv, nz_, (m, n) = SR.malformed(kind)
        assert lib.rls_sparse_csr_from_csc_host(0, m, n, cp.ctypes.data, rv.ctypes.data, nz_.ctypes.data, None, None, None) == -1, kind


def test_multigpu_classes_refuse_sparse_operators(rls):
    """ahead of any device work: a scipy-like object (anything with `tocsc`) stands in for a sparse matrix on a machine without a GPU"""
    class Sparse:
        def tocsc(self):
            raise AssertionError("must not be converted")

    mg = rls.multigpu
    for make in (lambda: mg.HipLocalOps(rls, Sparse(), 0), lambda: mg.HipFistaOps(rls, Sparse(), 0), lambda: mg.HipAdmmOps(rls, Sparse(), 0),
                 lambda: mg.CommRowShardedCGNR(rls, [np.eye(4, dtype=np.float32), Sparse()]),
                 lambda: mg.CommRowShardedFISTA(rls, [Sparse()]), lambda: mg.CommRowShardedADMM(rls, [Sparse()], None, 4)):
        with pytest.raises(TypeError, match="sparse"):
            make()


def test_python_class_is_exported_and_validates_ahead_of_the_context(rls):
    import torch

    assert rls.DeviceSparseMatrix.__name__ == "DeviceSparseMatrix" and hasattr(rls.DeviceSparseMatrix, "from_host")
    for name in ("mul_", "mul_adj_", "mul_transpose_", "rownorm2", "to_dense", "to_host", "normal_operator", "size"):
        assert callable(getattr(rls.DeviceSparseMatrix, name)), name
    # a malformed triple is a ValueError whether or not a device exists: nothing asks for a context before the check
    for kind in SR.MALFORMED:
        with pytest.raises(ValueError):
            rls.DeviceSparseMatrix.from_host(SR.malformed(kind))
    colptr, rowval, nz, shape = SR.random_csc(5, 4, 0.5, np.float32, 1)[0]
    for bad in ((colptr[:-1], rowval, nz, shape), (colptr, rowval[:-1], nz, shape), (colptr, rowval, nz, (0, 4)), (colptr, rowval, nz)):
        with pytest.raises(ValueError):
            rls.DeviceSparseMatrix.from_host(bad)
    with pytest.raises(TypeError):
        rls.DeviceSparseMatrix.from_host((colptr, rowval, nz.astype(np.float16), shape))
    with pytest.raises(TypeError):
        rls.DeviceSparseMatrix.from_host(np.eye(3, dtype=np.float32))
    if not torch.cuda.is_available():   # a well-formed triple gets as far as the context, and no further
        with pytest.raises(rls.RLSError, match="no CPU fallback"):
            rls.DeviceSparseMatrix.from_host((colptr, rowval, nz, shape))


# ---- the helper itself ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", SR.DTYPES)
def test_reference_twin_and_transpose_agree(dtype):
    csc, D = SR.random_csc(23, 17, 0.3, dtype, 11)
    assert np.array_equal(SR.dense(csc), D) and D.dtype == SR.wide(dtype)
    rowptr, colval, nz = SR.csr_from_csc(csc)
    R = np.zeros_like(D)
    for m in range(23):
        R[m, colval[rowptr[m]:rowptr[m + 1]]] = nz[rowptr[m]:rowptr[m + 1]]
    assert np.array_equal(R, D)
    if np.dtype(dtype).kind == "c":
        assert np.all(csc[2].imag != 0)
    csc_h, D_h = SR.with_holes(63, 129, dtype, 3, long_row=7)
    nnz_row, nnz_col = (D_h != 0).sum(axis=1), (D_h != 0).sum(axis=0)
    assert nnz_row[0] == nnz_row[-1] == nnz_row[31] == 0 and nnz_col[0] == nnz_col[-1] == nnz_col[64] == 0
    assert nnz_row[7] >= 120 and np.median(nnz_row) == 1
    lens = [0, 3, 4, 5, 9, 200]
    assert list((SR.row_lengths(lens, 256, dtype, 1)[1] != 0).sum(axis=1)) == lens


@pytest.mark.parametrize("dtype", (np.complex64, np.float64))
@pytest.mark.parametrize("lam", (0.0, 0.05))
def test_reference_sweep_equals_the_dense_kaczmarz_restatement(dtype, lam):
    """three sweeps of the sparse row sweep in float64 against oracle.Kaczmarz on the dense twin (natural order, L2 only)"""
    csc, D = SR.random_csc(40, 24, 0.3, dtype, 21)
    D[5, :] = 0   # (a row without energy: the oracle skips it, the sparse order leaves it out)
    mask = D != 0
    csc = SR.from_pattern(mask, dtype, 22)[0]
    D = SR.dense(csc)
    rng = np.random.default_rng(3)
    b = (D @ (rng.standard_normal(24) + (1j * rng.standard_normal(24) if D.dtype.kind == "c" else 0))).astype(D.dtype)
    ref = O.Kaczmarz(D, reg=O.L2Regularization(lam), iterations=3)
    O.solve(ref, b)
    s2 = SR.rownorm2(csc)
    rows = np.flatnonzero(s2 > 0)
    assert np.array_equal(rows, ref.rowindex) and 5 not in rows
    denom = 1.0 / (s2[rows] + lam)
    x, vl = SR.sparse_sweep(csc, np.zeros(24), b, np.zeros(40), rows, denom, np.sqrt(lam), 3)
    assert np.linalg.norm(x - ref.x) <= 1e-13 * np.linalg.norm(ref.x)
    assert np.linalg.norm(vl - ref.vl) <= 1e-13 * max(np.linalg.norm(ref.vl), 1.0)
