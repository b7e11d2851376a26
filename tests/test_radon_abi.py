"""CPU tests of RadonOp's boundary (csrc/radon.hip): the new symbols in the header, the export table and the
binding; null handles; every refusal of the Python class raised ahead of the context; the TypeError of every solver that does not serve
the operator; and the numpy restatement (tests/radon_ref.py) the GPU tests compare against, held to an independent computation of
the chord: the line clipped parametrically against each pixel's square (Liang-Barsky)."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import radon_ref as RR
from test_abi import header_symbols

SYMBOLS = ("rls_radon_create", "rls_radon_destroy", "rls_radon_info", "rls_radon_mul", "rls_radon_mul_normal", "rls_radon_to_dense",
           "rls_radon_lanes")
# the angle set of tests/test_gpu_radon.py: snapped axes and their exact ties, |c| = |s|, near-axis, negative, above pi
ANGLES = [0.0, np.pi / 2, np.pi, np.pi / 4, 3 * np.pi / 4, 0.05, np.pi / 2 - 0.05, -0.4, 3.5, 1.0, 2.0, 0.3, 2.9]


def test_symbols_in_header_export_table_and_binding(rls):
    from rls_amd import _lib

    out = subprocess.run(["nm", "-D", "--defined-only", rls.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (rls_[a-z0-9_]+)", out))
    for s in SYMBOLS:
        assert s in header_symbols() and s in exported and s in _lib.PROTOTYPES, s
    assert rls.load().rls_abi_version() == 2
    assert hasattr(rls, "RadonOp")


def test_null_handles_return_invalid(rls):
    lib = rls.load()
    out, v, n = C.c_void_p(), C.c_int32(), C.c_int64()
    ang = np.zeros(1, np.float64)
    assert lib.rls_radon_create(None, 0, 4, 4, 1, ang.ctypes.data, 0, C.byref(out)) == -1
    assert lib.rls_radon_destroy(None) == -1
    assert lib.rls_radon_info(None, C.byref(n), C.byref(n), C.byref(n)) == -1
    assert lib.rls_radon_mul(None, 0, 1.0, 0.0, None, 0.0, 0.0, None) == -1
    assert lib.rls_radon_mul_normal(None, None, None) == -1
    assert lib.rls_radon_to_dense(None, None, 4) == -1
    assert lib.rls_radon_lanes(None, C.byref(v)) == -1


def test_refusals_are_raised_ahead_of_the_context(rls):
    import torch

    for dt in (np.float16, np.int32):
        with pytest.raises(TypeError):
            rls.RadonOp(dt, [0.0, 1.0], (4, 4))
    for shape in ((4,), (4, 4, 4), (0, 4), (4, -1), ()):
        with pytest.raises(ValueError):
            rls.RadonOp(np.float32, [0.0, 1.0], shape)
    for angles in ([], [np.nan], [0.0, np.inf], np.zeros((2, 2))):
        with pytest.raises(ValueError):
            rls.RadonOp(np.float32, angles, (4, 4))
    for detectors in (0, -3, 2.5):
        with pytest.raises(ValueError):
            rls.RadonOp(np.float32, [0.0], (4, 4), detectors=detectors)
    if not torch.cuda.is_available():   # well-formed arguments get as far as the context, and no further
        for dt in (np.float32, np.complex64, np.float64, np.complex128):
            with pytest.raises(rls.RLSError, match="no CPU fallback"):
                rls.RadonOp(dt, [0.0, 0.5], (4, 3))
        with pytest.raises(rls.RLSError, match="no CPU fallback"):
            rls.RadonOp(np.float32, np.linspace(0, np.pi, 5), (4, 3), detectors=7)


def _stub(rls, dtype, M, N):
    """an operator object without a device behind it: what the solvers' constructors look at before they refuse"""
    A = rls.RadonOp.__new__(rls.RadonOp)
    A.dtype, A.M, A.N = np.dtype(dtype), M, N
    A.code, A.double, A.ctx, A._h = 0, False, None, None
    return A


def test_other_solvers_and_multigpu_refuse_with_a_type_error(rls):
    A = _stub(rls, np.float32, 21, 16)
    assert A.handle is None and A.gram is None and A.size(1) == 21 and A.size(2) == 16 and A.shape == (21, 16)
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


def _chord(t, theta, xr, yr):
    """length of {t (cos, sin) + u (-sin, cos)} inside the unit square centred at (xr, yr): Liang-Barsky on the parameter u"""
    c, s = np.cos(theta), np.sin(theta)
    px, py, dx, dy = t * c, t * s, -s, c
    u0, u1 = -np.inf, np.inf
    for p, q in ((-dx, px - (xr - 0.5)), (dx, (xr + 0.5) - px), (-dy, py - (yr - 0.5)), (dy, (yr + 0.5) - py)):   # p u <= q
        if p == 0:
            if q < 0:
                return 0.0
        elif p < 0:
            u0 = max(u0, q / p)
        else:
            u1 = min(u1, q / p)
    return max(0.0, u1 - u0)


def test_restatement_weights_are_the_chord_lengths():
    """5 x 4 image, the GPU test's angles, the default detector count: 1e-12, and the 0.5 rule on the exact ties (a ray along a pixel
    edge at a snapped angle, where the clipped length is a matter of which side of the edge rounding puts the ray)"""
    shape = (5, 4)
    D = RR.default_detectors(shape)
    assert D == 2 * 4 + 1
    A = RR.dense(shape, ANGLES, D)
    c, s, mx, mn, hi = RR.table(ANGLES)
    assert [bool(v) for v in mn == 0] == [True, True, True] + [False] * 10 and np.all(mx[:3] == 1) and np.all(mn[3:] >= 0.049)
    ties = worst = 0
    for q, theta in enumerate(ANGLES):
        for k in range(D):
            t = k - (D - 1) / 2
            for j in range(shape[1]):
                for i in range(shape[0]):
                    xr, yr = i - (shape[0] - 1) / 2, j - (shape[1] - 1) / 2
                    got = A[k + D * q, i + shape[0] * j]
                    if mn[q] == 0 and abs(t - (xr * c[q] + yr * s[q])) == hi[q]:
                        ties += 1
                        assert got == 0.5 / mx[q], (q, k, i, j, got)
                        continue
                    worst = max(worst, abs(got - _chord(t, theta, xr, yr)))
    assert ties > 0, "the even extent at theta = pi / 2 has rays along pixel edges"
    assert worst <= 1e-12, worst


@pytest.mark.parametrize("shape,D", [((5, 4), None), ((3, 5), 5), ((8, 8), 1)])
def test_restatement_adjoint_is_the_transpose_of_forward(shape, D):
    n = shape[0] * shape[1]
    A = RR.dense(shape, ANGLES, D)
    m = A.shape[0]
    assert m == (RR.default_detectors(shape) if D is None else D) * len(ANGLES)
    F = np.stack([RR.forward(e, shape, ANGLES, D) for e in np.eye(n)], axis=1)
    T = np.stack([RR.adjoint(e, shape, ANGLES, D) for e in np.eye(m)], axis=1)
    assert np.array_equal(F, A) and np.array_equal(T, A.T)
    rng = np.random.default_rng(3)
    x, y = rng.standard_normal(n) + 1j * rng.standard_normal(n), rng.standard_normal(m) + 1j * rng.standard_normal(m)
    assert abs(np.vdot(y, RR.forward(x, shape, ANGLES, D)) - np.vdot(RR.adjoint(y, shape, ANGLES, D), x)) <= 1e-12 * np.linalg.norm(x) * np.linalg.norm(y)
    A32 = RR.dense(shape, ANGLES, D, np.float32)
    assert A32.dtype == np.float32 and np.abs(A32 - A).max() <= 1e-4
