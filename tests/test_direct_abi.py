"""CPU tests of the DirectSolver surface: the five rls_direct_* entry points are declared, exported and bound, they refuse null
arguments without touching them, the Python classes are public, linearSolverList() is what it was, and the constructor's sorting
of `reg` (src/Direct.jl:18-35) does what the reference's does -- on the function the constructor calls, which needs no device."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rls_mi355x.h")
ENTRY_POINTS = ("rls_direct_create", "rls_direct_factor", "rls_direct_solve", "rls_direct_get_status", "rls_direct_destroy",
                "rls_direct_get_factor")


def test_entry_points_declared_exported_and_bound(rls):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", rls.LIB_PATH], capture_output=True, text=True, check=True).stdout
    from rls_amd import _lib

    for sym in ENTRY_POINTS:
        assert re.search(r"int32_t\s+%s\s*\(" % sym, text), f"{sym} is not declared in the header"
        assert re.search(r" T %s$" % sym, out, flags=re.M), f"{sym} is not exported"
        assert sym in _lib.PROTOTYPES
    m = re.search(r"int32_t\s+rls_direct_solve\s*\(([^)]*)\)\s*;", text)
    assert [re.sub(r"\s*\w+$", "", a.strip()) for a in m.group(1).split(",")] == ["rls_direct*", "int64_t", "const void*", "int64_t", "void*",
                                                                                   "int64_t", "int32_t"]
    m = re.search(r"typedef struct rls_direct_status \{(.*?)\} rls_direct_status;", text, flags=re.S)
    assert [d.split()[0] for d in m.group(1).split(";") if d.strip()] == ["float", "int32_t", "int32_t"]
    assert [(n, t) for n, t in _lib.DirectStatus._fields_] == [("lambda_", C.c_float), ("factorizations", C.c_int32), ("info", C.c_int32)]


def test_null_arguments_are_errors_not_crashes(rls):
    lib = rls.load()
    out, st, buf = C.c_void_p(), rls._lib.DirectStatus(), (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    assert lib.rls_direct_create(None, C.byref(out)) == -1   # RLS_E_INVALID
    assert lib.rls_direct_factor(None, 0.5) == -1
    assert lib.rls_direct_solve(None, 1, p, 16, p, 16, 0) == -1
    assert lib.rls_direct_get_status(None, C.byref(st)) == -1
    assert lib.rls_direct_destroy(None) == -1
    ld = C.c_int64(-7)
    assert lib.rls_direct_get_factor(None, C.byref(out), C.byref(ld), C.byref(out)) == -1
    assert lib.rls_direct_get_factor(p, None, C.byref(ld), C.byref(out)) == -1      # (refused before the plan is looked at)
    assert lib.rls_direct_get_factor(p, C.byref(out), None, C.byref(out)) == -1
    assert lib.rls_direct_get_factor(p, C.byref(out), C.byref(ld), None) == -1
    assert not out.value and ld.value == -7


def test_classes_are_public(rls):
    assert issubclass(rls.DirectSolver, rls.AbstractDirectSolver) and issubclass(rls.AbstractDirectSolver, rls.AbstractLinearSolver)
    assert issubclass(rls.DirectBatchedState, rls.BatchedState)
    assert rls.DirectSolverState().x is None and rls.DirectSolverState().convergence() == {}
    # the categories stay apart: no isapplicable rule covers the direct solvers (src/RegularizedLeastSquares.jl:223-258)
    assert not rls.isapplicable(rls.DirectSolver, [rls.L2Regularization(0.1)])
    for cat in (rls.AbstractKrylovSolver, rls.AbstractRowActionSolver, rls.AbstractPrimalDualSolver, rls.AbstractProximalGradientSolver):
        assert not issubclass(rls.DirectSolver, cat)


def test_the_two_direct_solvers_share_one_python_path(rls):
    """DirectSolver and PseudoInverse differ in their plans and refusals; the rest is ONE function each, held by the category"""
    from rls_amd.solvers import _DirectPlan, _PinvPlan

    D, P = rls.DirectSolver, rls.PseudoInverse
    for name in ("init_", "iterate", "_run", "_init_batched", "_new_state", "_the_plan"):
        assert getattr(D, name) is getattr(P, name) is getattr(rls.AbstractDirectSolver, name), name
    assert _DirectPlan.__del__ is _PinvPlan.__del__ and _DirectPlan.__init__ is _PinvPlan.__init__
    assert _DirectPlan.solve is not _PinvPlan.solve and _DirectPlan.status is not _PinvPlan.status
    for name in ("_step", "fits", "init", "status", "convergence", "_max_steps", "_plain"):
        assert getattr(rls.DirectBatchedState, name) is getattr(rls.PseudoInverseBatchedState, name), name
    assert rls.DirectSolverState.convergence is rls.PseudoInverseState.convergence
    assert rls.DirectSolverState is not rls.PseudoInverseState and rls.DirectBatchedState is not rls.PseudoInverseBatchedState
    assert not issubclass(P, D) and not issubclass(D, P)
    assert not issubclass(rls.PseudoInverseBatchedState, rls.DirectBatchedState)
    # the category stays a category: it names no plan and has no constructor of its own
    assert rls.AbstractDirectSolver._plan_cls is None and "__init__" not in vars(rls.AbstractDirectSolver)
    assert not rls.isapplicable(rls.AbstractDirectSolver, [rls.L2Regularization(0.1)])


def test_linear_solver_list_is_unchanged(rls):
    assert rls.linearSolverList() == [rls.CGNR, rls.Kaczmarz, rls.FISTA, rls.OptISTA, rls.POGM, rls.ADMM, rls.SplitBregman]
    assert rls.DirectSolver not in rls.applicableSolverList([rls.L2Regularization(0.1)])


def test_constructor_sorts_reg_like_the_reference(rls):
    from rls_amd.solvers import _direct_fused_projection, _direct_sort_regs

    l2, proj = _direct_sort_regs(None)                       # the default: [L2Regularization(0)]
    assert isinstance(l2, rls.L2Regularization) and l2.lam == 0.0 and proj == []
    pos, real, l1 = rls.PositiveRegularization(), rls.RealRegularization(), rls.L1Regularization(0.3)
    l2, proj = _direct_sort_regs([pos])                      # no L2 sink: lambda = 0
    assert l2.lam == 0.0 and proj == [pos]
    given = rls.L2Regularization(0.25)
    l2, proj = _direct_sort_regs([real, l1, given, pos])     # the projections in their order, then the one further term
    assert l2 is given and proj == [real, pos, l1]
    l2, proj = _direct_sort_regs(given)                      # a single term, not a list
    assert l2 is given and proj == []
    with pytest.raises(ValueError, match="does not allow for more than one L2 regularization term, found 2"):
        _direct_sort_regs([given, l1, rls.L21Regularization(0.1, slices=2)])
    with pytest.raises(ValueError, match="unambigiously"):   # two L2 sinks: findsink's own error
        _direct_sort_regs([given, rls.L2Regularization(1.0)])
    # MeasurementBasedNormalization without b: factor one
    l2, _ = _direct_sort_regs([given], rls.MeasurementBasedNormalization())
    assert l2.lam == 0.25
    # which projection rides on the solve's last kernel
    assert _direct_fused_projection([pos, l1]) == (2, [l1]) and _direct_fused_projection([real]) == (1, [])
    assert _direct_fused_projection([l1]) == (0, [l1]) and _direct_fused_projection([]) == (0, [])
