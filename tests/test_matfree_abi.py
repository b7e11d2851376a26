"""CPU tests of the matrix-free operators' boundary (csrc/fft.hip): the new symbols in the header, the
export table and the binding; null handles; every refusal of the Python classes raised ahead of the context; the numpy restatement
(tests/matfree_ref.py) the GPU tests compare against; and the TypeError of every solver that does not serve these operators."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import matfree_ref as MR
from test_abi import header_symbols

SYMBOLS = ("rls_sampling_create", "rls_sampling_destroy", "rls_sampling_mul", "rls_sampling_mul_normal", "rls_fft_create",
           "rls_fft_destroy", "rls_fft_apply", "rls_fft_variant", "rls_fft_sampled_mul", "rls_fft_sampled_mul_normal")


def test_symbols_in_header_export_table_and_binding(rls):
    from rls_amd import _lib

    out = subprocess.run(["nm", "-D", "--defined-only", rls.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (rls_[a-z0-9_]+)", out))
    for s in SYMBOLS:
        assert s in header_symbols() and s in exported and s in _lib.PROTOTYPES, s
    assert rls.load().rls_abi_version() == 2


def test_null_handles_return_invalid(rls):
    lib = rls.load()
    out, v = C.c_void_p(), C.c_int32()
    idx = np.zeros(1, np.int32)
    shape = (C.c_int64 * 1)(8)
    assert lib.rls_sampling_create(None, 0, 4, 1, idx.ctypes.data, C.byref(out)) == -1
    assert lib.rls_sampling_destroy(None) == -1
    assert lib.rls_sampling_mul(None, 0, 1.0, 0.0, None, 0.0, 0.0, None) == -1
    assert lib.rls_sampling_mul_normal(None, None, None) == -1
    assert lib.rls_fft_create(None, 1, 1, shape, 3, C.byref(out)) == -1
    assert lib.rls_fft_destroy(None) == -1
    assert lib.rls_fft_apply(None, 0, None, None) == -1
    assert lib.rls_fft_variant(None, C.byref(v)) == -1
    assert lib.rls_fft_sampled_mul(None, None, 0, None, None) == -1
    assert lib.rls_fft_sampled_mul_normal(None, None, None, None) == -1


def test_refusals_are_raised_ahead_of_the_context(rls):
    import torch

    for bad in ([0, 1, 1], [0, 16], [-1, 2], np.zeros((2, 2), np.int32), [], [0.5, 1.0]):
        with pytest.raises(ValueError):
            rls.SamplingOp(np.float32, bad, (4, 4))
    with pytest.raises(ValueError):
        rls.SamplingOp(np.float32, [0], (0, 4))
    with pytest.raises(TypeError):
        rls.SamplingOp(np.float16, [0, 1], (4, 4))
    for real in (np.float32, np.float64):
        with pytest.raises(TypeError):
            rls.FFTOp(real, (8, 8))
    for shape in ((6, 8), (8, 12), (3,), (2, 2, 2), (4, 2, 8)):
        with pytest.raises(ValueError):
            rls.FFTOp(np.complex64, shape)
    with pytest.raises(TypeError):
        rls.ProdOp("S", "F")
    if not torch.cuda.is_available():   # well-formed arguments get as far as the context, and no further
        with pytest.raises(rls.RLSError, match="no CPU fallback"):
            rls.SamplingOp(np.float32, [0, 3], (2, 2))
        with pytest.raises(rls.RLSError, match="no CPU fallback"):
            rls.FFTOp(np.complex64, (4, 4))


@pytest.mark.parametrize("shape", [(8,), (4, 8), (2, 2), (1, 4)])
@pytest.mark.parametrize("shift", [False, True])
def test_restatement_unitary_fft_is_unitary_and_adjoints_are_adjoints(shape, shift):
    n = int(np.prod(shape))
    F = MR.fft_dense(shape, shift, True)
    assert np.abs(F.conj().T @ F - np.eye(n)).max() <= 1e-12
    for unitary in (False, True):
        Fd = MR.fft_dense(shape, shift, unitary)
        Fa = MR.dense(lambda e: MR.fft_adj(e, shape, shift, unitary), n)
        assert np.abs(Fa - Fd.conj().T).max() <= 1e-12
    # the shifts of an even extent are sign patterns: the claim the kernels fold into their loads and stores
    if shift and all(s % 2 == 0 for s in shape):
        k = np.indices(shape).sum(axis=0).ravel(order="F")
        sgn = (-1.0) ** k
        g = np.prod([-1.0 if s == 2 else 1.0 for s in shape])
        assert np.abs(F - g * sgn[:, None] * MR.fft_dense(shape, False, True) * sgn[None, :]).max() <= 1e-12


@pytest.mark.parametrize("shape", [(16,), (4, 8)])
def test_restatement_product_is_the_product_of_the_matrices(shape):
    n = int(np.prod(shape))
    pat = MR.pattern(n, n // 2, 3)
    assert pat[0] == 0 and pat[-1] == n - 1 and np.unique(pat).size == n // 2
    S, F = MR.sampling_dense(pat, n), MR.fft_dense(shape)
    P = MR.sampled_fft_dense(pat, shape)
    assert np.abs(P - S @ F).max() <= 1e-12
    Pa = MR.dense(lambda e: MR.sampled_fft_adj(e, pat, shape), n // 2)
    assert np.abs(Pa - P.conj().T).max() <= 1e-12
    assert np.array_equal(np.diag(S.T @ S), MR.sampling_mask(pat, n))
    x = np.arange(n, dtype=np.float64)
    assert np.array_equal(MR.sampling_adj(MR.sampling(x, pat), pat, n), MR.sampling_mask(pat, n) * x)


def _stub(rls, cls, dtype, M, N):
    """an operator object without a device behind it: what the solvers' constructors look at before they refuse"""
    A = cls.__new__(cls)
    A.dtype, A.M, A.N = np.dtype(dtype), M, N
    A.code, A.double, A.ctx = 1, False, None
    return A


def test_other_solvers_and_multigpu_refuse_with_a_type_error(rls):
    ops = [_stub(rls, rls.SamplingOp, np.complex64, 8, 16), _stub(rls, rls.FFTOp, np.complex64, 16, 16),
           _stub(rls, rls.SampledFFTOp, np.complex64, 8, 16)]
    for A in ops:
        assert A.handle is None and A.gram is None and A.size(1) == A.M and A.size(2) == 16
        for T in (rls.ADMM, rls.OptISTA, rls.POGM, rls.SplitBregman, rls.Kaczmarz, rls.DirectSolver, rls.PseudoInverse):
            with pytest.raises(TypeError, match="CGNR and FISTA"):
                rls.createLinearSolver(T, A, reg=rls.L2Regularization(0.01))
        for T in (rls.ADMM, rls.OptISTA, rls.POGM, rls.SplitBregman):
            with pytest.raises(TypeError, match="CGNR and FISTA"):
                rls.createLinearSolver(T, None, AHA=A.normal_operator(), reg=rls.L2Regularization(0.01))
        with pytest.raises(TypeError, match="CGNR and FISTA"):   # no explicit-Gram route
            rls.createLinearSolver(rls.CGNR, A, AHA="a Gram matrix")
        mg = rls.multigpu
        for make in (lambda: mg.HipLocalOps(rls, A, 0), lambda: mg.HipFistaOps(rls, A, 0), lambda: mg.HipAdmmOps(rls, A, 0),
                     lambda: mg.CommRowShardedCGNR(rls, [A]), lambda: mg.CommRowShardedFISTA(rls, [A])):
            with pytest.raises(TypeError, match="CGNR and FISTA"):
                make()
        with pytest.raises(TypeError):
            rls.ProdOp(rls.WeightingOp(None), A)
