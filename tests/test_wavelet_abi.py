"""CPU tests of the wavelet operator's surface -- header, export table, ctypes table, the Python class and its refusals -- and of
the float64 reference matrix the GPU tests compare against (tests/wavelet_ref.py): it is checked here, on its own, first."""
import os
import re
import subprocess

import numpy as np
import pytest

import wavelet_ref as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rls_mi355x.h")
SYMBOLS = ("rls_wavelet_create", "rls_wavelet_destroy", "rls_wavelet_levels", "rls_wavelet_apply", "rls_prox_wavelet_l1",
           "rls_fista_set_reg_wavelet")

# (shape, levels) of tests/test_gpu_wavelet.py whose dense matrix is affordable, and the two that go through `apply`
SMALL = [((2,), None), ((4,), None), ((64,), None), ((24,), None), ((2, 2), None), ((8, 4), None), ((16, 16), None),
         ((32, 8), 1), ((96, 40), None), ((1, 16), None)]
LARGE = [((256, 256), None), ((128, 256), None)]
FILTERS = ("haar", "db2")


def test_symbols_in_header_export_table_and_binding(rls):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    from rls_amd import _lib

    out = subprocess.run(["nm", "-D", "--defined-only", rls.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (rls_[a-z0-9_]+)", out))
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), f"{s} is not declared in the header"
        assert s in exported, f"{s} is not exported"
        assert s in _lib.PROTOTYPES, f"{s} is not in the ctypes table"
    assert "RLS_REG_WAVELET = 5" in text and _lib.REG_WAVELET == 5
    assert "RLS_WT_HAAR = 0" in text and "RLS_WT_DB2 = 1" in text and (_lib.WT_HAAR, _lib.WT_DB2) == (0, 1)


def test_null_handles_are_invalid(rls):
    import ctypes as C

    lib = rls.load()
    assert lib.rls_wavelet_destroy(None) == -1
    assert lib.rls_wavelet_levels(None, None) == -1
    assert lib.rls_wavelet_apply(None, 0, None, None) == -1
    assert lib.rls_prox_wavelet_l1(None, None, 0.5) == -1
    assert lib.rls_fista_set_reg_wavelet(None, None, 0.5, 0) == -1
    out = C.c_void_p()
    assert lib.rls_wavelet_create(None, 0, 1, (C.c_int64 * 1)(8), 1, -1, C.byref(out)) == -1   # no context


def test_python_class_geometry_and_refusals(rls):
    op = rls.WaveletOp((96, 40))
    assert (op.levels, op.n_in, op.n_out, op.size(1), op.size(2), op.wt) == (3, 3840, 3840, 3840, 3840, "db2")
    for shape, levels in SMALL + LARGE:
        assert rls.WaveletOp(shape, levels=levels).levels == (WR.default_levels(shape) if levels is None else levels)
    assert rls.WaveletOp((1, 16)).levels == 4 and rls.WaveletOp((8, 4)).levels == 2 and rls.WaveletOp((24,)).levels == 3
    assert rls.WaveletOp((32, 8), levels=0).levels == 0
    for bad in (dict(shape=(3,), levels=1), dict(shape=(6,), levels=2), dict(shape=(8, 6), levels=2), dict(shape=(4, 4, 4)),
                dict(shape=(8,), levels=-1), dict(shape=(8,), wt="sym4"), dict(shape=(0,)), dict(shape=(8, 8), levels=4)):
        with pytest.raises(ValueError):
            rls.WaveletOp(**bad)


@pytest.mark.parametrize("wt", FILTERS)
def test_reference_taps_and_level_matrix(wt):
    h, g = WR.taps(wt)
    assert abs(h.sum() - np.sqrt(2)) < 1e-15 and abs(g.sum()) < 1e-15 and abs(h @ h - 1) < 1e-15
    for n in (2, 4, 6, 10, 24, 96):
        M = WR.level_matrix(n, wt)
        assert np.abs(M.T @ M - np.eye(n)).max() < 1e-13, (wt, n)


@pytest.mark.parametrize("wt", FILTERS)
@pytest.mark.parametrize("shape,levels", SMALL)
def test_reference_matrix_is_orthogonal_and_sees_constants(shape, levels, wt):
    W = WR.dense(shape, wt, levels)
    N = W.shape[0]
    assert N == int(np.prod(shape))
    assert np.abs(W.T @ W - np.eye(N)).max() < 1e-13
    rng = np.random.default_rng(N)
    x = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    assert abs(np.linalg.norm(W @ x) - np.linalg.norm(x)) < 1e-12 * np.linalg.norm(x)          # Parseval
    if levels is None:   # full depth of the shorter side: sum g = 0 leaves a constant in the approximation band alone
        c = W @ np.full(N, 0.75)
        J = WR.default_levels(shape)
        ext = WR.extents(shape)
        na = int(np.prod([e >> J for e in ext]))   # approximation coefficients left after J levels
        nz = np.flatnonzero(np.abs(c) > 1e-13)
        assert len(nz) == na
        if na == 1:
            assert nz[0] == 0 and abs(c[0] - 0.75 * np.sqrt(N)) < 1e-12
    # the separable form is the same operator
    assert np.abs(WR.apply(x, shape, wt, levels) - W @ x).max() < 1e-12
    assert np.abs(WR.apply(x, shape, wt, levels, adjoint=True) - W.T @ x).max() < 1e-12


@pytest.mark.parametrize("wt", FILTERS)
@pytest.mark.parametrize("shape,levels", LARGE)
def test_reference_separable_form_at_the_large_shapes(shape, levels, wt):
    """the dense matrix of these is 34 GB: orthogonality of every level factor, the round trip, Parseval and the constant signal
    through `apply`, which the small shapes tie to the dense matrix"""
    N = int(np.prod(shape))
    for j in range(WR.default_levels(shape)):
        for e in shape:
            M = WR.level_matrix(e >> j, wt)
            assert np.abs(M.T @ M - np.eye(e >> j)).max() < 1e-13
    rng = np.random.default_rng(7)
    x = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    y = WR.apply(x, shape, wt, levels)
    assert abs(np.linalg.norm(y) - np.linalg.norm(x)) < 1e-12 * np.linalg.norm(x)
    assert np.abs(WR.apply(y, shape, wt, levels, adjoint=True) - x).max() < 1e-12
    c = WR.apply(np.full(N, 0.75), shape, wt, levels)
    ext, J = WR.extents(shape), WR.default_levels(shape)
    assert len(np.flatnonzero(np.abs(c) > 1e-12)) == int(np.prod([e >> J for e in ext]))
