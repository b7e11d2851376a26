"""CPU tests of the surface of PseudoInverse's blocked sweeps: rls_pinv_get_block_status is declared, exported and bound (Python
and Julia), refuses null arguments without touching them, rls_pinv_block_status is the 16-byte struct of the header,
solverconvergence carries "block" and "block_sweeps", and the Float64 refusal of the constructor is what it was."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rls_mi355x.h")
FIELDS = ["block", "block_sweeps", "block_rounds", "reserved"]


def test_entry_point_declared_exported_and_bound(rls):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", rls.LIB_PATH], capture_output=True, text=True, check=True).stdout
    from rls_amd import _lib

    sym = "rls_pinv_get_block_status"
    m = re.search(r"int32_t\s+%s\s*\(([^)]*)\)\s*;" % sym, text)
    assert m, f"{sym} is not declared in the header"
    assert [re.sub(r"\s*\w+$", "", a.strip()) for a in m.group(1).split(",")] == ["rls_pinv*", "rls_pinv_block_status*"]
    assert re.search(r" T %s$" % sym, out, flags=re.M), f"{sym} is not exported"
    assert sym in _lib.PROTOTYPES
    julia = open(os.path.join(ROOT, "julia", "RLSMI355X", "src", "RLSMI355X.jl")).read()
    assert "(:%s, librls[])" % sym in julia


def test_block_status_struct_layout(rls):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"typedef struct rls_pinv_block_status \{(.*?)\} rls_pinv_block_status;", text, flags=re.S)
    decls = [d.split() for d in m.group(1).split(";") if d.strip()]
    assert decls == [["int32_t", f] for f in FIELDS]
    st = rls._lib.PinvBlockStatus
    assert [(n, t) for n, t in st._fields_] == [(f, C.c_int32) for f in FIELDS]
    assert C.sizeof(st) == 16
    # rls_pinv_status is what it was
    assert C.sizeof(rls._lib.PinvStatus) == 16 and [n for n, _ in rls._lib.PinvStatus._fields_] == ["lambda_", "factorizations", "sweeps", "info"]


def test_null_arguments_are_errors_and_the_output_is_untouched(rls):
    lib = rls.load()
    st = rls._lib.PinvBlockStatus(7, 8, 9, 10)
    assert lib.rls_pinv_get_block_status(None, C.byref(st)) == -1      # RLS_E_INVALID
    assert (st.block, st.block_sweeps, st.block_rounds, st.reserved) == (7, 8, 9, 10)
    assert lib.rls_pinv_get_block_status(None, None) == -1


def test_convergence_reports_the_blocked_sweeps(rls):
    from rls_amd.solvers import _pinv_info

    st = rls._lib.PinvStatus(0.5, 1, 7, 0)
    st.block, st.block_sweeps = 16, 3
    assert _pinv_info(st) == {"info": 0, "lambda": 0.5, "factorizations": 1, "sweeps": 7, "block": 16, "block_sweeps": 3}
    assert _pinv_info(None) == {}
    assert hasattr(rls.solvers._PinvPlan, "block_status")


def test_float64_is_still_refused_with_the_same_text(rls):
    class _FakeDouble(rls.DeviceMatrix):          # the element-type check reads `code` and nothing else
        def __init__(self, dt):
            self.dtype = np.dtype(dt)
            self.code = rls.arrays.dtype_code(self.dtype)

    for dt in (np.float64, np.complex128):
        with pytest.raises(NotImplementedError, match="Float32 / ComplexF32"):
            rls.PseudoInverse(_FakeDouble(dt))
