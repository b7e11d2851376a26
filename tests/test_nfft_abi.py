"""CPU tests of NFFTOp's boundary (csrc/nfft.hip): the new symbols in the header, the export table and the
binding; null handles; every refusal of the Python class raised ahead of the context; the TypeError of every solver that does not
serve the operator.  The restatement the GPU tests compare against is held on the CPU by tests/test_nfft_ref.py."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

from test_abi import header_symbols

SYMBOLS = ("rls_nfft_create", "rls_nfft_destroy", "rls_nfft_info", "rls_nfft_mul", "rls_nfft_mul_normal")


def test_symbols_in_header_export_table_and_binding(rls):
    from rls_amd import _lib

    out = subprocess.run(["nm", "-D", "--defined-only", rls.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (rls_[a-z0-9_]+)", out))
    for s in SYMBOLS:
        assert s in header_symbols() and s in exported and s in _lib.PROTOTYPES, s
    assert rls.load().rls_abi_version() == 2
    assert hasattr(rls, "NFFTOp")


def test_null_handles_return_invalid(rls):
    lib = rls.load()
    out, n = C.c_void_p(), C.c_int64()
    nodes = np.zeros(1, np.float64)
    shape = (C.c_int64 * 1)(4)
    assert lib.rls_nfft_create(None, 1, 1, shape, 1, nodes.ctypes.data, 4, C.byref(out)) == -1
    assert lib.rls_nfft_destroy(None) == -1
    assert lib.rls_nfft_info(None, C.byref(n), C.byref(n), C.byref(n)) == -1
    assert lib.rls_nfft_mul(None, 0, None, None) == -1
    assert lib.rls_nfft_mul_normal(None, None, None) == -1


def test_refusals_are_raised_ahead_of_the_context(rls):
    import torch

    ok1, ok2 = [0.0, 0.25, -0.5], [[0.0, 0.25], [-0.5, 0.1]]
    for dt in (np.float32, np.float64, np.float16, np.int32):   # real or integer element types
        with pytest.raises(TypeError):
            rls.NFFTOp(dt, ok1, (8,))
    for shape in ((), (4, 4, 4), (0, 4), (4, -1), (0,), (-3,)):
        with pytest.raises(ValueError):
            rls.NFFTOp(np.complex64, ok2 if len(shape) == 2 else ok1, shape)
    for nodes, shape in ((ok1, (4, 4)), (ok2, (8,)), (np.zeros((3, 2)), (4, 4)), (np.zeros((2, 2, 2)), (4, 4)),   # the wrong leading dimension
                         ([], (8,)), (np.zeros((2, 0)), (4, 4)),                                                  # empty
                         ([0.0, 0.5], (8,)), ([-0.51], (8,)), ([0.1, np.nan], (8,)), ([[0.0], [0.5]], (4, 4)), ([[np.nan], [0.0]], (4, 4))):
        with pytest.raises(ValueError):
            rls.NFFTOp(np.complex64, nodes, shape)
    for m in (0, 9, 2.5, -1):
        with pytest.raises(ValueError):
            rls.NFFTOp(np.complex64, ok1, (8,), m=m)
    for dt, N in ((np.complex64, 4097), (np.complex128, 2049)):   # the grid line 2 N_d past the FFT's limit
        with pytest.raises(ValueError):
            rls.NFFTOp(dt, ok1, (N,))
        with pytest.raises(ValueError):
            rls.NFFTOp(dt, ok2, (8, N))
    if not torch.cuda.is_available():   # well-formed arguments get as far as the context, and no further
        for dt, N in ((np.complex64, 4096), (np.complex128, 2048)):
            with pytest.raises(rls.RLSError, match="no CPU fallback"):
                rls.NFFTOp(dt, ok1, (N,))
        with pytest.raises(rls.RLSError, match="no CPU fallback"):
            rls.NFFTOp(np.complex64, ok2, (8, 6), m=8)
        with pytest.raises(rls.RLSError, match="no CPU fallback"):
            rls.NFFTOp(np.complex128, [np.nextafter(0.5, 0.0)], (1,), m=1)


def _stub(rls, dtype, M, N):
    """an operator object without a device behind it: what the solvers' constructors look at before they refuse"""
    A = rls.NFFTOp.__new__(rls.NFFTOp)
    A.dtype, A.M, A.N = np.dtype(dtype), M, N
    A.code, A.double, A.ctx, A._h = 1, False, None, None
    return A


def test_other_solvers_and_multigpu_refuse_with_a_type_error(rls):
    A = _stub(rls, np.complex64, 70, 48)
    assert A.handle is None and A.gram is None and A.size(1) == 70 and A.size(2) == 48 and A.shape == (70, 48)
    for T in (rls.ADMM, rls.SplitBregman, rls.OptISTA, rls.POGM, rls.Kaczmarz, rls.DirectSolver, rls.PseudoInverse):
        with pytest.raises(TypeError, match="CGNR and FISTA"):
            rls.createLinearSolver(T, A, reg=rls.L2Regularization(0.01))
    for T in (rls.ADMM, rls.OptISTA, rls.POGM, rls.SplitBregman):
        with pytest.raises(TypeError, match="CGNR and FISTA"):
            rls.createLinearSolver(T, None, AHA=A.normal_operator(), reg=rls.L2Regularization(0.01))
    with pytest.raises(TypeError, match="CGNR and FISTA"):   # no explicit-Gram route
        rls.createLinearSolver(rls.CGNR, A, AHA="a Gram matrix")
    mg = rls.multigpu
    for make in (lambda: mg.HipLocalOps(rls, A, 0), lambda: mg.CommRowShardedCGNR(rls, [A])):
        with pytest.raises(TypeError, match="CGNR and FISTA"):
            make()
    with pytest.raises(TypeError):   # density compensation stays refused
        rls.ProdOp(rls.WeightingOp(None), A)
