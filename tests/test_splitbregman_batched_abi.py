"""CPU tests of the batched SplitBregman surface: the C entry point is declared, exported and bound under the same name, it
refuses a null plan without touching it, and the scheduler state is public."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rls_mi355x.h")


def test_entry_point_declared_exported_and_bound(rls):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"int32_t\s+rls_admm_set_bregman\s*\(([^)]*)\)\s*;", text)
    assert m, "rls_admm_set_bregman is not declared in the header"
    assert [re.sub(r"\s*\w+$", "", a.strip()) for a in m.group(1).split(",")] == ["rls_admm*", "int32_t", "void*", "int64_t"]
    out = subprocess.run(["nm", "-D", "--defined-only", rls.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T rls_admm_set_bregman$", out, flags=re.M)
    from rls_amd import _lib

    assert "rls_admm_set_bregman" in _lib.PROTOTYPES
    # rls_admm_params is ABI: the Bregman mode came as a new entry point, not as new fields
    m = re.search(r"typedef struct rls_admm_params \{(.*?)\} rls_admm_params;", text, flags=re.S)
    assert "iterations_inner" not in m.group(1) and "breg" not in m.group(1)


def test_null_plan_is_an_error_not_a_crash(rls):
    import ctypes as C

    lib = rls.load()
    y = (C.c_float * 16)()
    assert lib.rls_admm_set_bregman(None, 4, C.cast(y, C.c_void_p), 16) == -1   # RLS_E_INVALID
    assert lib.rls_admm_set_bregman(None, 0, None, 0) == -1


def test_state_is_public_and_an_admm_batched_state(rls):
    assert issubclass(rls.SplitBregmanBatchedState, rls.AdmmBatchedState)
    assert rls.SplitBregmanBatchedState is not rls.AdmmBatchedState
    assert rls.SplitBregman._init_batched is not rls.ADMM._init_batched
