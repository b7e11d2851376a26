"""CPU tests of the PseudoInverse surface: the rls_pinv_* entry points are declared, exported and bound, they refuse null
arguments without touching them, the Python classes are public and sit under AbstractDirectSolver, linearSolverList() is what it
was, the constructor sorts `reg` as src/Direct.jl:85-102 does (the function DirectSolver's constructor calls, error text
verbatim), and Float64 / a Gram matrix without A are refused.  The sweep cap (info = 1) cannot be reached without a device: its
part here is the status struct's layout."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rls_mi355x.h")
ENTRY_POINTS = ("rls_pinv_create", "rls_pinv_factor", "rls_pinv_solve", "rls_pinv_singular_values", "rls_pinv_get_status",
                "rls_pinv_destroy")


def _args(text, sym):
    m = re.search(r"int32_t\s+%s\s*\(([^)]*)\)\s*;" % sym, text)
    return [re.sub(r"\s*\w+$", "", a.strip()) for a in m.group(1).split(",")]


def test_entry_points_declared_exported_and_bound(rls):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", rls.LIB_PATH], capture_output=True, text=True, check=True).stdout
    from rls_amd import _lib

    for sym in ENTRY_POINTS + ("rls_pinv_get_factor",):
        assert re.search(r"int32_t\s+%s\s*\(" % sym, text), f"{sym} is not declared in the header"
        assert re.search(r" T %s$" % sym, out, flags=re.M), f"{sym} is not exported"
        assert sym in _lib.PROTOTYPES
    # lambda is an argument of the solve, and the factorisation takes none
    assert _args(text, "rls_pinv_solve") == ["rls_pinv*", "float", "int64_t", "const void*", "int64_t", "void*", "int64_t", "int32_t"]
    assert _args(text, "rls_pinv_factor") == ["rls_pinv*"]
    assert _args(text, "rls_pinv_singular_values") == ["rls_pinv*", "float*"]
    m = re.search(r"typedef struct rls_pinv_status \{(.*?)\} rls_pinv_status;", text, flags=re.S)
    assert [d.split()[0] for d in m.group(1).split(";") if d.strip()] == ["float", "int32_t", "int32_t", "int32_t"]
    assert [(n, t) for n, t in _lib.PinvStatus._fields_] == [("lambda_", C.c_float), ("factorizations", C.c_int32), ("sweeps", C.c_int32),
                                                             ("info", C.c_int32)]
    assert C.sizeof(_lib.PinvStatus) == 16


def test_null_arguments_are_errors_not_crashes(rls):
    lib = rls.load()
    out, st, buf = C.c_void_p(), rls._lib.PinvStatus(), (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    ld = C.c_int64()
    assert lib.rls_pinv_create(None, C.byref(out)) == -1   # RLS_E_INVALID
    assert lib.rls_pinv_factor(None) == -1
    assert lib.rls_pinv_solve(None, 0.5, 1, p, 16, p, 16, 0) == -1
    assert lib.rls_pinv_singular_values(None, buf) == -1
    assert lib.rls_pinv_get_status(None, C.byref(st)) == -1
    assert lib.rls_pinv_get_factor(None, C.byref(out), C.byref(ld), C.byref(out), C.byref(ld)) == -1
    assert lib.rls_pinv_destroy(None) == -1
    assert not out.value and (st.factorizations, st.sweeps, st.info) == (0, 0, 0)


def test_classes_are_public(rls):
    assert issubclass(rls.PseudoInverse, rls.AbstractDirectSolver) and issubclass(rls.AbstractDirectSolver, rls.AbstractLinearSolver)
    assert not issubclass(rls.PseudoInverse, rls.DirectSolver)
    assert issubclass(rls.PseudoInverseBatchedState, rls.BatchedState)
    assert rls.PseudoInverseState().x is None and rls.PseudoInverseState().convergence() == {}
    from rls_amd.solvers import _PinvPlan  # noqa: F401  (the plan belongs to the solver)
    assert not rls.isapplicable(rls.PseudoInverse, [rls.L2Regularization(0.1)])
    for cat in (rls.AbstractKrylovSolver, rls.AbstractRowActionSolver, rls.AbstractPrimalDualSolver, rls.AbstractProximalGradientSolver):
        assert not issubclass(rls.PseudoInverse, cat)


def test_linear_solver_list_is_unchanged(rls):
    assert rls.linearSolverList() == [rls.CGNR, rls.Kaczmarz, rls.FISTA, rls.OptISTA, rls.POGM, rls.ADMM, rls.SplitBregman]
    assert rls.PseudoInverse not in rls.applicableSolverList([rls.L2Regularization(0.1)])


def test_constructor_sorts_reg_and_keeps_the_error_text(rls):
    """PseudoInverse.__init__ goes through _direct_sort_regs: in the one function both direct solvers' constructors end in (the
    source says so: no device is needed to read it)"""
    import inspect

    from rls_amd.solvers import _direct_sort_regs

    assert rls.PseudoInverse._setup is rls.DirectSolver._setup is rls.AbstractDirectSolver._setup
    assert "self._setup(A, AHA, reg, normalizeReg)" in inspect.getsource(rls.PseudoInverse.__init__)
    assert "self._setup(A, AHA, reg, normalizeReg)" in inspect.getsource(rls.DirectSolver.__init__)
    src = inspect.getsource(rls.AbstractDirectSolver._setup)
    assert "_direct_sort_regs(reg, self.normalizeReg, self.A)" in src
    assert list(inspect.signature(rls.PseudoInverse.__init__).parameters) == list(inspect.signature(rls.DirectSolver.__init__).parameters)
    given, pos, real, l1 = rls.L2Regularization(0.25), rls.PositiveRegularization(), rls.RealRegularization(), rls.L1Regularization(0.3)
    l2, proj = _direct_sort_regs([real, l1, given, pos])
    assert l2 is given and proj == [real, pos, l1]
    with pytest.raises(ValueError, match="PseudoInverse does not allow for more than one L2 regularization term, found 2"):
        _direct_sort_regs([given, l1, rls.L21Regularization(0.1, slices=2)])


def test_refusals_need_no_device(rls):
    with pytest.raises(ValueError, match="needs the matrix A"):
        rls.PseudoInverse(AHA=object())          # a Gram matrix alone: refused before anything is looked at
    with pytest.raises(ValueError, match="needs the matrix A"):
        rls.PseudoInverse()

    class _FakeDouble(rls.DeviceMatrix):          # the element-type check reads `code` and nothing else
        def __init__(self, dt):
            self.dtype = np.dtype(dt)
            self.code = rls.arrays.dtype_code(self.dtype)

    for dt in (np.float64, np.complex128):
        with pytest.raises(NotImplementedError, match="Float32 / ComplexF32"):
            rls.PseudoInverse(_FakeDouble(dt))
