"""CPU checks of the Float64 / ComplexF64 plan ABI (rls_cgnr_*_d, rls_fista_*_d): the header declares every symbol and the library
exports it, the two new status structs agree field for field between the header, the ctypes binding and the Julia mirrors, every
symbol is `ccall`ed from the Julia package, and a null plan is RLS_E_INVALID."""
import ctypes as C
import re
import subprocess

from test_julia_binding import _ct_class, header_prototypes, header_structs, julia_ccalls, julia_structs

PLAN_SYMBOLS = [
    "rls_cgnr_create_d", "rls_cgnr_destroy_d", "rls_cgnr_init_d", "rls_cgnr_step_d", "rls_cgnr_get_status_d", "rls_cgnr_step_status_d",
    "rls_cgnr_path_d", "rls_fista_create_d", "rls_fista_destroy_d", "rls_fista_set_reg_d", "rls_fista_init_d", "rls_fista_set_start_d",
    "rls_fista_step_d", "rls_fista_get_status_d", "rls_fista_step_status_d", "rls_fista_solution_d", "rls_fista_path_d",
]


def test_header_declares_and_library_exports_the_plan_family(rls):
    protos = header_prototypes()
    lib = rls.load()
    out = subprocess.run(["nm", "-D", "--defined-only", rls.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (rls_[a-z0-9_]+)", out))
    for sym in PLAN_SYMBOLS:
        assert sym in protos, f"{sym} is not declared in include/rls_mi355x.h"
        assert sym in exported and hasattr(lib, sym), f"{sym} is not exported"
        assert protos[sym][0] == "i32"
    # the scalars cross the boundary as doubles, the operands as raw pointers
    assert protos["rls_cgnr_create_d"][1] == ["ptr", "i32", "i64", "i64", "ptr", "i64", "ptr", "i64", "ptr", "ptr", "ptr", "ptr", "ptr"]
    assert protos["rls_fista_create_d"][1] == protos["rls_cgnr_create_d"][1]
    assert protos["rls_cgnr_init_d"][1] == ["ptr", "ptr", "f64", "f64", "i32"]
    assert protos["rls_fista_set_reg_d"][1] == ["ptr", "i32", "f64", "i64", "i32"]
    assert protos["rls_fista_init_d"][1] == ["ptr", "ptr", "f64", "f64", "f64", "i32", "i32"]
    assert lib.rls_abi_version() == 2


def test_status_structs_match_the_header(rls):
    from rls_amd import _lib
    hs = header_structs()
    assert hs["rls_cgnr_status_d"] == ["i32", "i32"] + ["f64"] * 7
    assert hs["rls_fista_status_d"] == ["i32", "i32"] + ["f64"] * 5
    for cls, hname in ((_lib.CgnrStatusD, "rls_cgnr_status_d"), (_lib.FistaStatusD, "rls_fista_status_d")):
        assert [_ct_class(t) for _, t in cls._fields_] == hs[hname], cls.__name__
    assert [n for n, _ in _lib.CgnrStatusD._fields_] == ["iteration", "done", "alpha_re", "alpha_im", "beta_re", "beta_im", "zeta", "residual", "z0"]
    assert [n for n, _ in _lib.FistaStatusD._fields_] == ["iteration", "done", "theta", "theta_old", "rel_res_norm", "residual", "norm_x0"]
    # the Float32 structs keep their float fields
    assert hs["rls_cgnr_status"].count("f32") == 7 and hs["rls_fista_status"].count("f32") == 5
    for sym in PLAN_SYMBOLS:
        assert sym in _lib.PROTOTYPES


def test_julia_mirrors_and_ccalls():
    hs, js = header_structs(), julia_structs()
    for jname, hname in (("CgnrStatusD", "rls_cgnr_status_d"), ("FistaStatusD", "rls_fista_status_d")):
        assert jname in js, f"julia struct {jname} not found"
        assert js[jname] == hs[hname], f"{jname} {js[jname]} != {hname} {hs[hname]}"
    bound = {c[2] for c in julia_ccalls()}
    missing = [s for s in PLAN_SYMBOLS if s not in bound]
    assert not missing, f"not called anywhere in julia/RLSMI355X: {missing}"


def test_null_plan_is_invalid(rls):
    lib = rls.load()
    from rls_amd import _lib
    stc, stf, i32, vp = _lib.CgnrStatusD(), _lib.FistaStatusD(), C.c_int32(0), C.c_void_p()
    assert lib.rls_cgnr_destroy_d(None) == -1
    assert lib.rls_cgnr_init_d(None, None, 0.0, 0.0, 1) == -1
    assert lib.rls_cgnr_step_d(None, 1) == -1
    assert lib.rls_cgnr_get_status_d(None, C.byref(stc)) == -1
    assert lib.rls_cgnr_step_status_d(None, 1, C.byref(stc)) == -1
    assert lib.rls_cgnr_path_d(None, C.byref(i32)) == -1
    assert lib.rls_fista_destroy_d(None) == -1
    assert lib.rls_fista_set_reg_d(None, 1, 0.1, 1, 0) == -1
    assert lib.rls_fista_init_d(None, None, 1.0, 1.0, 0.0, 1, 0) == -1
    assert lib.rls_fista_set_start_d(None, None, 0) == -1
    assert lib.rls_fista_step_d(None, 1) == -1
    assert lib.rls_fista_get_status_d(None, C.byref(stf)) == -1
    assert lib.rls_fista_step_status_d(None, 1, C.byref(stf)) == -1
    assert lib.rls_fista_solution_d(None, C.byref(vp)) == -1
    assert lib.rls_fista_path_d(None, C.byref(i32)) == -1
    # no context, no plan
    assert lib.rls_cgnr_create_d(None, 3, 4, 2, None, 4, None, 0, None, None, None, None, C.byref(vp)) == -1
    assert lib.rls_fista_create_d(None, 3, 4, 2, None, 4, None, 0, None, None, None, None, C.byref(vp)) == -1
