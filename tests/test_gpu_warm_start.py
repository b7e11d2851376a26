"""Warm starts -- init!(solver, b; x0, theta) -- on every solver path, against the float64 oracle started from the same x0 and theta.

Float32 / ComplexF32 results go through the parity gate of tests/conftest.py (1e-5 against the float64 oracle, or twice the
working-precision oracle's own error); Float64 / ComplexF64 results are held to the bars of test_gpu_f64_plans.py.  Every warm-started
reference is first shown, on the two oracle runs alone, to differ from the cold-start reference by more than 100 x the bar the device
result is then held to: a path that drops x0 returns the cold-start answer and cannot pass.  Each test asserts the kernel path it
was written for.  The start vectors: a Gaussian vector of the size of the planted solution (handed over as a device vector), the
scalar 0.25 (broadcast), and the float64 oracle's own iterate after 40 cold iterations (handed over as a host array).  rho is an
explicit 0.9 / (sqrt M + sqrt N)^2 (sigma_max of a Gaussian matrix is sqrt M + sqrt N to a per cent: no SVD of the large shapes)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import rls_oracle as O
from conftest import PARITY_TOL, _rel, parity_check as parity
from test_gpu_f64_plans import GRAM_TOL, ITER_TOL, SCALAR_TOL, close, plan_path
from test_gpu_parity import _fista_path, _resident_unavailable, hi

pytestmark = pytest.mark.gpu

ALL_STARTS = [(k, th) for k in ("gauss", "scalar", "near") for th in (1.0, 1.7)]
FEW_STARTS = [("gauss", 1.7), ("scalar", 1.0), ("near", 1.7)]   # the large (resident) shapes: every start and both thetas once
NO_THETA = [("gauss", None), ("scalar", None), ("near", None)]  # ADMM, SplitBregman, Kaczmarz: init! takes x0 only
NEAR_ITS = 40


def is_double(dt):
    return np.dtype(dt).itemsize // (2 if np.dtype(dt).kind == "c" else 1) == 8


@functools.lru_cache(maxsize=3)
def problem(M, N, dtname, seed):
    """(A, b, A in float64, b in float64, rho, lam1, the Gaussian start) -- made once per shape and shared, never written to"""
    dt = np.dtype(dtname)
    A, xt, b = O.make_problem(M, N, dt, seed)
    A64, b64 = A.astype(hi(dt)), b.astype(hi(dt))
    rho = 0.9 / (math.sqrt(M) + math.sqrt(N)) ** 2
    lam1 = 0.02 * float(np.max(np.abs(A64.conj().T @ b64)))
    rng = np.random.default_rng(seed + 1000)
    g = rng.standard_normal(N) + (1j * rng.standard_normal(N) if dt.kind == "c" else 0)
    g = (g * (np.linalg.norm(xt) / np.linalg.norm(g))).astype(dt)
    for a in (A, b, A64, b64, g):
        a.setflags(write=False)
    return A, b, A64, b64, rho, lam1, g


def run_oracle(ref, rhs, watch=(), **init_kw):
    """ref.init(rhs, **init_kw), iterate until None; ({iteration: x}, the solver)"""
    ref.init(rhs, **init_kw)
    seen, k = {}, 0
    while ref.iterate() is not None:
        k += 1   # (counted here: SplitBregman's `iteration` is its inner counter)
        if k in watch:
            seen[k] = np.array(ref.solution(), copy=True)
    seen["last"] = np.array(ref.solution(), copy=True)
    return seen, ref


def start_value(kind, mk_ref, A64, rhs64, g, dt):
    """the start in the WORKING precision (what the device is handed); the oracle gets these same values, widened"""
    if kind == "scalar":
        return 0.25
    if kind == "gauss":
        return g
    probe = mk_ref(A64, NEAR_ITS)
    return np.asarray(run_oracle(probe, rhs64)[0]["last"]).astype(dt)


def widen(x0, dt):
    return x0 if np.ndim(x0) == 0 else np.asarray(x0).astype(hi(dt))


def hand_over(rls, ctx, kind, x0):
    """Gaussian: a device vector; near: a host array; scalar: itself"""
    return rls.DeviceVector.from_host(np.array(x0), ctx) if kind == "gauss" else x0


def apart_enough(tag, want, cold, bar, want_work=None):
    """the precondition, on oracle runs alone and BEFORE the device runs: the warm-started reference is further from the cold-start
    reference (same iteration) than 100 x the bar the device result is then held to.  `bar` a float: that relative bar.  `bar`
    None: the Float32 parity gate, whose bar is 1e-5 or, failing that, 2 x the working-precision oracle's own error (`want_work`:
    its result) -- so the larger of the two."""
    apart = _rel(cold, want)
    if bar is None:
        bar = max(PARITY_TOL, 2 * _rel(want_work, want)) if want_work is not None else PARITY_TOL
    print(f"{tag}: warm oracle vs cold oracle {apart:.3e}, bar {bar:.1e}")
    assert apart > 100 * bar, f"{tag}: the warm and cold references are only {apart:.3e} apart (bar {bar:.1e}): change the seed or x0"


def held(tag, got, want, bar, want_work=None):
    """the gate for one warm-started result: the Float32 parity gate (`bar` None; recorded like every other parity comparison), or a
    relative bar"""
    if bar is None:
        return parity(tag, got, want, want_work)
    e = _rel(got, want)
    print(f"{tag}: device vs oracle {e:.3e}")
    assert e < bar, f"{tag}: {e:.3e} >= {bar:.0e}"


def warm_cases(rls, ctx, tag, dt, A, rhs, A64, rhs64, g, mk_ref, mk_dev, starts, its, bar=None, after=None, whole=True, stepwise=True):
    """For each (start, theta): the float64 oracle warm and cold at iterations 1, 2 and `its` and the working-precision oracle
    warm, the precondition on those; then a whole solve_(S, b, x0, theta) and a callback-driven solve_ (one step call per iterate)
    compared at iterates 1, 2 and last.  mk_ref(A_, iterations) builds the oracle on a matrix of either precision, mk_dev() a
    fresh device solver; after(S, ref, work) asserts the path and the counts (ref / work: the float64 / working-precision oracle
    after its warm run)."""
    bd = rls.DeviceVector.from_host(np.array(rhs), ctx)
    watch = (1, 2)
    keys = watch + ("last",)
    cold, _ = run_oracle(mk_ref(A64, its), rhs64, watch)
    near = None
    for kind, theta in starts:
        if kind == "near":
            near = x0 = start_value(kind, mk_ref, A64, rhs64, g, dt) if near is None else near
        else:
            x0 = start_value(kind, mk_ref, A64, rhs64, g, dt)
        kw_d = {} if theta is None else {"theta": theta}
        want, ref = run_oracle(mk_ref(A64, its), rhs64, watch, x0=widen(x0, dt), **kw_d)
        # (in double precision the working-precision oracle IS the float64 oracle)
        ww, work = (want, ref) if is_double(dt) else run_oracle(mk_ref(A, its), rhs, watch, x0=x0, **kw_d)
        t = f"{tag}_{kind}" + ("" if theta is None else f"_theta{theta}")
        for i in keys:
            apart_enough(f"{t}_it{i}", want[i], cold[i], bar, ww[i] if bar is None else None)
        if whole:
            S = mk_dev()
            x = rls.solve_(S, bd, x0=hand_over(rls, ctx, kind, x0), **kw_d).to_host()
            held(t + "_whole", x, want["last"], bar, ww["last"])
            if after:
                after(S, ref, work)
        if stepwise:
            S = mk_dev()
            seen = {}
            x = rls.solve_(S, bd, x0=hand_over(rls, ctx, kind, x0),
                           callbacks=lambda sv, i: seen.__setitem__(i, rls.solversolution(sv).to_host()) if i in watch else None, **kw_d).to_host()
            for i in watch:
                held(f"{t}_it{i}", seen[i], want[i], bar, ww[i])
            held(t + "_callbacks_last", x, want["last"], bar, ww["last"])
            if after:
                after(S, ref, work)


def fista_pair(rls, regs, restart="none", gram=False):
    """(mk_ref, mk_dev factory): regs(R) builds the regulariser list from either module"""
    def mk_ref(rho):
        return lambda A_, its: O.FISTA(A_, reg=regs(O), rho=rho, iterations=its, relTol=0.0, restart=restart,
                                       normal="gram" if gram else "matrixfree")

    def mk_dev(Ad, rho, its, Gd=None):
        return lambda: rls.createLinearSolver(rls.FISTA, Ad, AHA=Gd, reg=regs(rls), rho=rho, iterations=its, relTol=0.0, restart=restart)
    return mk_ref, mk_dev


def fista_on_path(ctx, want_path, resident=False):
    def after(S, ref, work):
        got = _fista_path(ctx, S)
        if resident and got != want_path:
            _resident_unavailable()
        assert got == want_path, (got, want_path)
        assert S.state.iteration == ref.iteration and getattr(S.state, "fallbacks", 0) == 0
    return after


# ------------------------------------------------------------------------------------------------------------------
# 1. FISTA, Float32 / ComplexF32: one test per kernel path
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("restart", ["none", "gradient"])
@pytest.mark.parametrize("dt,M,N", [(np.float32, 256, 128), (np.complex64, 250, 61)])
def test_fista_small_system_kernel(rls, ctx, dt, M, N, restart):
    """fista_small_kernel (path 8): the single-workgroup launch rebuilds iteration 0 from buf[0] and y"""
    A, b, A64, b64, rho, lam, g = problem(M, N, np.dtype(dt).name, 67)
    regs = lambda R: [R.L1Regularization(lam)]
    mk_ref, mk_dev = fista_pair(rls, regs, restart)
    Ad = rls.DeviceMatrix.from_host(np.array(A, order="F"), ctx)
    warm_cases(rls, ctx, f"warm_fista_small_{M}x{N}_{np.dtype(dt).name}_{restart}", dt, A, b, A64, b64, g, mk_ref(rho),
               mk_dev(Ad, rho, 10), ALL_STARTS, 10, after=fista_on_path(ctx, 8))


def test_fista_streaming_pipeline(rls, ctx):
    """the slab pipeline (path 1: resident = 0 at a shape the resident kernel would take)"""
    M, N, dt = 4000, 2002, np.complex64
    A, b, A64, b64, rho, lam, g = problem(M, N, np.dtype(dt).name, 2)
    mk_ref, mk_dev = fista_pair(rls, lambda R: [R.L1Regularization(lam)], "gradient")
    Ad = rls.DeviceMatrix.from_host(np.array(A, order="F"), ctx)
    ctx.tune(resident=0)
    try:
        warm_cases(rls, ctx, f"warm_fista_pipeline_{M}x{N}_c64", dt, A, b, A64, b64, g, mk_ref(rho), mk_dev(Ad, rho, 8), FEW_STARTS, 8,
                   after=fista_on_path(ctx, 1))
    finally:
        ctx.tune(resident=1)


@pytest.mark.parametrize("ahead", [1, 0])
@pytest.mark.parametrize("dt,M,N,restart", [(np.complex64, 4096, 2048, "none"), (np.float32, 4000, 2200, "gradient")])   # full; ragged = masked
def test_fista_resident_kernel_and_server(rls, ctx, dt, M, N, restart, ahead):
    """fista_resident_kernel (path 4).  The whole solve_ is ONE launch; the callback-driven run is the listening kernel served one
    iterate per command, with and without the iteration computed ahead; and the first command after a warm-started init_ may
    ask for several iterations"""
    A, b, A64, b64, rho, lam, g = problem(M, N, np.dtype(dt).name, 2)
    regs = lambda R: [R.L1Regularization(lam)] + ([R.PositiveRegularization()] if restart == "gradient" else [])
    mk_ref, mk_dev = fista_pair(rls, regs, restart)
    Ad = rls.DeviceMatrix.from_host(np.array(A, order="F"), ctx)
    tag = f"warm_fista_resident_{M}x{N}_{np.dtype(dt).name}_ahead{ahead}"
    ctx.tune(resident_server=1, resident_ahead=ahead)
    try:
        warm_cases(rls, ctx, tag, dt, A, b, A64, b64, g, mk_ref(rho), mk_dev(Ad, rho, 8), FEW_STARTS, 8,
                   after=fista_on_path(ctx, 4, resident=True), whole=ahead == 1)
        # the first command after a warm-started init_: three iterations at once, then one
        cold, _ = run_oracle(mk_ref(rho)(A64, 8), b64, (3, 4))
        want, _ = run_oracle(mk_ref(rho)(A64, 8), b64, (3, 4), x0=g.astype(hi(dt)), theta=1.7)
        ww, _ = run_oracle(mk_ref(rho)(A, 8), b, (3, 4), x0=g, theta=1.7)
        for total in (3, 4):
            apart_enough(f"{tag}_first_command_it{total}", want[total], cold[total], None, ww[total])
        S = mk_dev(Ad, rho, 8)()
        rls.init_(S, rls.DeviceVector.from_host(np.array(b), ctx), x0=np.array(g), theta=1.7)
        st = rls._lib.FistaStatus()
        for n, total in ((3, 3), (1, 4)):
            assert ctx.lib.rls_fista_step_status(S.state._plan, n, C.byref(st)) == 0 and st.iteration == total
            S.state._refresh(ctx.lib)
            held(f"{tag}_first_command_it{total}", S.state.x.to_host(), want[total], None, ww[total])
        assert _fista_path(ctx, S) == 4 and st.fallbacks == 0
    finally:
        ctx.tune(resident_server=1, resident_ahead=1)


@pytest.mark.parametrize("pipe", [2, 1, 0])
@pytest.mark.parametrize("dt,M,N,restart", [(np.float32, 300, 120, "gradient"), (np.complex64, 70, 34, "none")])
def test_fista_gram_mode(rls, ctx, dt, M, N, restart, pipe):
    """FISTA(A; AHA = A' * A): pipe 2 the resident Gram kernel (path 5; under callbacks its listening mode), pipe 1 one launch per
    iteration (path 2), pipe 0 the unfused sequence (path 0)"""
    A, b, A64, b64, rho, lam, g = problem(M, N, np.dtype(dt).name, 9)
    regs = lambda R: [R.L1Regularization(lam)] + ([R.PositiveRegularization()] if restart == "gradient" else [])
    mk_ref, mk_dev = fista_pair(rls, regs, restart, gram=True)
    Ad = rls.DeviceMatrix.from_host(np.array(A, order="F"), ctx)
    Gd = Ad.gram()
    ctx.tune(gram_pipeline=1 if pipe else 0, resident=1 if pipe == 2 else 0)
    try:
        warm_cases(rls, ctx, f"warm_fista_gram_{M}x{N}_{np.dtype(dt).name}_pipe{pipe}", dt, A, b, A64, b64, g, mk_ref(rho),
                   mk_dev(Ad, rho, 10, Gd), ALL_STARTS, 10, after=fista_on_path(ctx, {2: 5, 1: 2, 0: 0}[pipe], resident=pipe == 2))
    finally:
        ctx.tune(gram_pipeline=1, resident=1)


def test_fista_gram_resident_server_without_the_iteration_ahead(rls, ctx):
    """the listening resident Gram kernel with resident_ahead = 0 (the default, 1, is what test_fista_gram_mode serves)"""
    dt, M, N = np.complex64, 70, 34
    A, b, A64, b64, rho, lam, g = problem(M, N, np.dtype(dt).name, 9)
    mk_ref, mk_dev = fista_pair(rls, lambda R: [R.L1Regularization(lam)], "none", gram=True)
    Ad = rls.DeviceMatrix.from_host(np.array(A, order="F"), ctx)
    ctx.tune(resident_server=1, resident_ahead=0)
    try:
        warm_cases(rls, ctx, "warm_fista_gram_server_ahead0", dt, A, b, A64, b64, g, mk_ref(rho), mk_dev(Ad, rho, 10, Ad.gram()), ALL_STARTS,
                   10, after=fista_on_path(ctx, 5, resident=True), whole=False)
    finally:
        ctx.tune(resident_server=1, resident_ahead=1)


REGS = {
    # name: (dtype, M, N, regulariser list, the path the plan reports -- None: no plan, the primitive sequence)
    "l1": (np.float32, 160, 64, lambda R, lam: [R.L1Regularization(lam)], 8),
    "l2": (np.complex64, 96, 36, lambda R, lam: [R.L2Regularization(0.3)], 8),
    "none": (np.float32, 160, 64, lambda R, lam: None, 8),
    "l1pos": (np.complex64, 96, 36, lambda R, lam: [R.L1Regularization(lam), R.PositiveRegularization()], 8),
    "l21": (np.float32, 160, 64, lambda R, lam: [R.L21Regularization(lam, slices=4)], 0),   # no elementwise update: the two-GEMV plan
    "tv": (np.float32, 160, 64, lambda R, lam: [R.TVRegularization(lam, shape=(8, 8))], 0),  # the FGP launch inside the plan
    # an image too large for the single-workgroup FGP launch: the plan refuses, the primitives run
    "tv_large": (np.float32, 4608, 4096, lambda R, lam: [R.TVRegularization(lam, shape=(16, 16, 16))], None),
}


@pytest.mark.parametrize("name", list(REGS))
def test_fista_regularisers(rls, ctx, name):
    dt, M, N, regs_of, want_path = REGS[name]
    A, b, A64, b64, rho, lam, g = problem(M, N, np.dtype(dt).name, 12)
    mk_ref, mk_dev = fista_pair(rls, lambda R: regs_of(R, lam))
    Ad = rls.DeviceMatrix.from_host(np.array(A, order="F"), ctx)
    its = 6

    def after(S, ref, work):
        assert S.state.iteration == ref.iteration
        if want_path is None:
            assert not S.state._plan and S._tv_unfused
        else:
            assert _fista_path(ctx, S) == want_path
    warm_cases(rls, ctx, f"warm_fista_{name}", dt, A, b, A64, b64, g, mk_ref(rho), mk_dev(Ad, rho, its),
               FEW_STARTS if name == "tv_large" else ALL_STARTS, its, after=after)


# ------------------------------------------------------------------------------------------------------------------
# 2. FISTA, Float64 / ComplexF64 (rls_fista_set_start_d)
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["plan", "gram", "primitives", "tv"])
@pytest.mark.parametrize("restart", ["none", "gradient"])
@pytest.mark.parametrize("dt", [np.float64, np.complex128])
def test_fista_f64(rls, ctx, dt, restart, mode):
    """the Float64 / ComplexF64 plan on A (paths 0 / 1) and on AHA (path 2), the primitive loops (use_device_plan_f64 = False), and TV
    (the plan refuses: primitives)"""
    M, N = 96, 40
    A, b, A64, b64, rho, lam, g = problem(M, N, np.dtype(dt).name, 21)
    regs = (lambda R: [R.TVRegularization(lam, shape=(8, 5))]) if mode == "tv" else (lambda R: [R.L1Regularization(lam)])
    mk_ref, mk_dev_of = fista_pair(rls, regs, restart, gram=mode == "gram")
    Ad = rls.DeviceMatrix.from_host(np.array(A, order="F"), ctx)
    Gd = rls.DeviceMatrix.from_host(np.asfortranarray(A.conj().T @ A), ctx) if mode == "gram" else None
    plain = mk_dev_of(Ad, rho, 10, Gd)

    def mk_dev():
        S = plain()
        S.use_device_plan_f64 = mode != "primitives"
        return S

    def after(S, ref, how):
        assert S.state.iteration == ref.iteration
        if mode in ("plan", "gram"):
            assert S.state._plan_d and plan_path(rls, ctx, S) in ((2,) if mode == "gram" else (0, 1))
            assert close(S.state.theta, ref.theta) and close(S.state.rel_res_norm, ref.rel_res_norm), (S.state.theta, ref.theta)
        else:
            assert not S.state._plan
    warm_cases(rls, ctx, f"warm_fista_f64_{np.dtype(dt).name}_{restart}_{mode}", dt, A, b, A64, b64, g, mk_ref(rho), mk_dev, ALL_STARTS,
               10, bar=GRAM_TOL if mode == "gram" else ITER_TOL, after=after)


@pytest.mark.parametrize("dt", [np.float64, np.complex128])
def test_fista_set_start_d_through_the_abi(rls, ctx, dt):
    """rls_fista_set_start_d after rls_fista_init_d, then step_status_d: the vector behind rls_fista_solution_d against the oracle
    at an odd and an even iteration count, theta 1.7; set_start_d after a step is RLS_E_STATE"""
    from rls_amd import _lib
    A, b, A64, b64, rho, lam, g = problem(96, 40, np.dtype(dt).name, 21)
    Ad, bd = rls.DeviceMatrix.from_host(np.array(A, order="F"), ctx), rls.DeviceVector.from_host(np.array(b), ctx)
    lib, h = ctx.lib, ctx.handle
    x, x0, xold, res = (rls.DeviceVector(Ad.N, dt, ctx) for _ in range(4))
    gd = rls.DeviceVector.from_host(np.array(g), ctx)
    plan = C.c_void_p()
    assert lib.rls_fista_create_d(h, Ad.code, Ad.M, Ad.N, Ad.ptr, Ad.lda, None, 0, x.ptr, x0.ptr, xold.ptr, res.ptr, C.byref(plan)) == 0
    try:
        assert lib.rls_fista_set_reg_d(plan, 1, lam, 1, 0) == 0   # RLS_REG_L1
        assert lib.rls_fista_init_d(plan, bd.ptr, rho, 1.7, 0.0, 50, 0) == 0
        assert lib.rls_fista_set_start_d(plan, gd.ptr, Ad.N) == 0
        mk = lambda: O.FISTA(A, reg=O.L1Regularization(lam), rho=rho, iterations=50, relTol=0.0)
        ref, cold = mk(), mk()
        ref.init(b, x0=g, theta=1.7)
        cold.init(b, theta=1.7)
        st, sol = _lib.FistaStatusD(), C.c_void_p()
        for n, total in ((7, 7), (3, 10)):
            for _ in range(n):
                ref.iterate(), cold.iterate()
            apart_enough(f"warm_fista_abi_d_{np.dtype(dt).name}_it{total}", ref.x, cold.x, ITER_TOL)
            assert lib.rls_fista_step_status_d(plan, n, C.byref(st)) == 0 and st.iteration == total and not st.done
            assert lib.rls_fista_solution_d(plan, C.byref(sol)) == 0
            cur = xold if total & 1 else x
            assert sol.value == cur.ptr
            held(f"warm_fista_abi_d_{np.dtype(dt).name}_it{total}", cur.to_host(), ref.x, ITER_TOL)
            assert close(st.rel_res_norm, ref.rel_res_norm) and close(st.theta, ref.theta)
            assert not close(cold.rel_res_norm, ref.rel_res_norm, 100 * SCALAR_TOL)
        assert lib.rls_fista_set_start_d(plan, gd.ptr, Ad.N) == -4     # RLS_E_STATE: only right after init_d
        assert lib.rls_fista_set_start_d(plan, gd.ptr, Ad.N - 1) != 0
    finally:
        assert lib.rls_fista_destroy_d(plan) == 0


# ------------------------------------------------------------------------------------------------------------------
# 3. the other solvers
# ------------------------------------------------------------------------------------------------------------------
ADMM_CASES = {
    # name: (dtype, M, N, kind, gram, device plan, resident inner cg!)
    "plan_l1": (np.float32, 120, 48, "l1", False, True, False),
    "plan_tv": (np.float32, 128, 64, "tv", False, True, False),
    "per_call_l1": (np.float32, 120, 48, "l1", False, False, False),
    "per_call_tv": (np.complex64, 96, 36, "tv", False, False, False),
    "gram_l1": (np.float32, 120, 48, "l1", True, True, False),
    "gram_tv": (np.complex64, 96, 36, "tv", True, True, False),
    "resident_cg_l1": (np.complex64, 4096, 2048, "l1", False, True, True),
    "resident_cg_tv": (np.complex64, 4096, 2048, "tv", False, True, True),
    "f64_l1": (np.float64, 96, 40, "l1", False, False, False),
    "f64_tv": (np.complex128, 96, 40, "tv", False, False, False),
}
TV_SHAPES = {64: (8, 8), 36: (6, 6), 40: (8, 5), 2048: (64, 32)}


@pytest.mark.parametrize("name", list(ADMM_CASES))
def test_admm(rls, ctx, name):
    """ADMM + L1 / TV from x0 (z = Phi x0, u = 0, the first cg! warm-started at x0): the device plan (rls_admm_step), the per-call
    path, Gram mode, the inner cg! on the resident kernel, Float64; the outer iteration count and the inner cg! counts are those of
    the working-precision oracle"""
    dt, M, N, kind, gram, use_plan, resident = ADMM_CASES[name]
    A, b, A64, b64, _, _, g = problem(M, N, np.dtype(dt).name, 2)
    regs = (lambda R: R.L1Regularization(0.05)) if kind == "l1" else (lambda R: R.TVRegularization(2e-2, shape=TV_SHAPES[N]))
    # (two inner cg! iterations: a full inner solve forgets its warm start, and with it x0, within a few outer iterations)
    its = 6
    kw = dict(rho=0.3, iterationsCG=2, tolInner=1e-4)
    mk_ref = lambda A_, n: O.ADMM(A_, reg=regs(O), iterations=n, normal="gram" if gram else "matrixfree", **kw)
    Ad = rls.DeviceMatrix.from_host(np.array(A, order="F"), ctx)
    Gd = Ad.gram() if gram else None

    def mk_dev():
        S = rls.createLinearSolver(rls.ADMM, Ad, AHA=Gd, reg=regs(rls), iterations=its, **kw)
        S.use_device_plan = use_plan
        return S
    def after(S, ref, work):
        assert bool(S.state._plan_ok) == (use_plan and not is_double(dt))
        # (the counts are the working-precision oracle's: tolInner is tested on working-precision residuals)
        assert S.state.iteration == work.iteration == ref.iteration
        assert list(S.state.cg_iterations) == list(work.cg_iters)
    warm_cases(rls, ctx, f"warm_admm_{name}", dt, A, b, A64, b64, g, mk_ref, mk_dev, NO_THETA, its,
               bar=(ITER_TOL if is_double(dt) else None), after=after)


@pytest.mark.parametrize("dt,M,N,kind", [(np.float32, 128, 64, "tv"), (np.complex64, 120, 48, "l1")])
def test_split_bregman_on_the_device_plan(rls, ctx, dt, M, N, kind):
    A, b, A64, b64, _, _, g = problem(M, N, np.dtype(dt).name, 33)
    regs = (lambda R: R.L1Regularization(0.05)) if kind == "l1" else (lambda R: R.TVRegularization(2e-2, shape=(8, 8)))
    kw = dict(rho=0.5, iterationsInner=2, iterationsCG=2)   # (short inner solves: x0 stays visible, as in test_admm)
    mk_ref = lambda A_, n: O.SplitBregman(A_, reg=regs(O), iterations=n, **kw)
    Ad = rls.DeviceMatrix.from_host(np.array(A, order="F"), ctx)
    mk_dev = lambda: rls.createLinearSolver(rls.SplitBregman, Ad, reg=regs(rls), iterations=3, **kw)

    def after(S, ref, work):
        assert S.state._plan_ok and S.state.iter_cnt == ref.iter_cnt
    warm_cases(rls, ctx, f"warm_splitbregman_{kind}", dt, A, b, A64, b64, g, mk_ref, mk_dev, NO_THETA, 3, after=after)


PGM = {"OptISTA": ("OptISTA", {}), "POGM": ("POGM", {}), "POGM-restart": ("POGM", {"restart": "gradient"})}


def pgm_pair(rls, name, regs, rho):
    cls, kw = PGM[name]
    mk_ref = lambda A_, n: getattr(O, cls)(A_, reg=regs(O), rho=rho, iterations=n, relTol=0.0, **kw)
    mk_dev = lambda Ad, n: (lambda: rls.createLinearSolver(getattr(rls, cls), Ad, reg=regs(rls), rho=rho, iterations=n, relTol=0.0, **kw))
    return mk_ref, mk_dev


def pgm_on_path(rls, want):
    """which iteration OptISTA / POGM took.  "fused": the one-launch update (stepwise or deferred), no resident plan; "resident":
    pgm_resident_kernel; "generic": a regulariser outside the fused kernels, from the primitives; "double": Float64 / ComplexF64,
    from the rls_*_d primitives"""
    from rls_amd import solvers

    def after(S, ref, work):
        assert S.state.iteration == ref.iteration
        fus = solvers._fusable_kinds(S.reg, S.proj if isinstance(S, rls.POGM) else [])
        plan = (getattr(S, "_pgm", None) or (None, None))[1]
        if want == "resident":
            if plan is None:
                _resident_unavailable()
            assert fus is not None and not plan.off and plan.fallbacks == 0
        else:
            assert plan is None and bool(S._op.double) == (want == "double") and (fus is None) == (want == "generic")
    return after


@pytest.mark.parametrize("name", list(PGM))
@pytest.mark.parametrize("dt,M,N", [(np.complex64, 256, 96), (np.float32, 128, 64)])
def test_optista_pogm_stepwise_and_deferred(rls, ctx, name, dt, M, N):
    """the fused update launch per iteration under callbacks, and the deferred run (every launch enqueued at once) without"""
    A, b, A64, b64, rho, lam, g = problem(M, N, np.dtype(dt).name, 31)
    mk_ref, mk_dev = pgm_pair(rls, name, lambda R: R.L1Regularization(lam), rho)
    Ad = rls.DeviceMatrix.from_host(np.array(A, order="F"), ctx)
    warm_cases(rls, ctx, f"warm_{name}_{M}x{N}", dt, A, b, A64, b64, g, mk_ref, mk_dev(Ad, 9), ALL_STARTS, 9, after=pgm_on_path(rls, "fused"))


@pytest.mark.parametrize("name", list(PGM))
@pytest.mark.parametrize("dt,M,N", [(np.complex64, 4096, 2048), (np.float32, 4000, 2200)])
def test_optista_pogm_resident_launch(rls, ctx, name, dt, M, N):
    """pgm_resident_kernel: the whole solve as ONE launch that starts from x (and y, z, zold = x for OptISTA)"""
    A, b, A64, b64, rho, lam, g = problem(M, N, np.dtype(dt).name, 2)
    mk_ref, mk_dev = pgm_pair(rls, name, lambda R: R.L1Regularization(lam), rho)
    Ad = rls.DeviceMatrix.from_host(np.array(A, order="F"), ctx)
    warm_cases(rls, ctx, f"warm_{name}_resident_{M}x{N}", dt, A, b, A64, b64, g, mk_ref, mk_dev(Ad, 9), FEW_STARTS, 9,
               after=pgm_on_path(rls, "resident"), stepwise=False)


@pytest.mark.parametrize("name", list(PGM))
def test_optista_pogm_generic_l21(rls, ctx, name):
    """a regulariser the fused update kernels do not take: the primitive-by-primitive iteration"""
    A, b, A64, b64, rho, lam, g = problem(192, 64, "complex64", 37)
    mk_ref, mk_dev = pgm_pair(rls, name, lambda R: R.L21Regularization(lam, slices=4), rho)
    Ad = rls.DeviceMatrix.from_host(np.array(A, order="F"), ctx)
    warm_cases(rls, ctx, f"warm_{name}_l21", np.complex64, A, b, A64, b64, g, mk_ref, mk_dev(Ad, 8), ALL_STARTS, 8,
               after=pgm_on_path(rls, "generic"))


@pytest.mark.parametrize("name", list(PGM))
@pytest.mark.parametrize("dt", [np.float64, np.complex128])
def test_optista_pogm_f64(rls, ctx, name, dt):
    A, b, A64, b64, rho, lam, g = problem(96, 40, np.dtype(dt).name, 21)
    mk_ref, mk_dev = pgm_pair(rls, name, lambda R: R.L1Regularization(lam), rho)
    Ad = rls.DeviceMatrix.from_host(np.array(A, order="F"), ctx)
    warm_cases(rls, ctx, f"warm_{name}_{np.dtype(dt).name}", dt, A, b, A64, b64, g, mk_ref, mk_dev(Ad, 9), ALL_STARTS, 9, bar=ITER_TOL,
               after=pgm_on_path(rls, "double"))


@pytest.mark.parametrize("dt,M,N", [(np.float32, 96, 256), (np.complex64, 96, 250), (np.float64, 40, 96), (np.complex128, 40, 96)])
def test_kaczmarz(rls, ctx, dt, M, N):
    """x0 in the sweep kernels (rls_kaczmarz_sweep and its _d twin).  Wide systems: the sweeps never touch the start's component in
    the null space of A, while a tall consistent system forgets its start within two sweeps"""
    A, b, A64, b64, _, _, g = problem(M, N, np.dtype(dt).name, 51)
    mk_ref = lambda A_, n: O.Kaczmarz(np.array(A_), reg=O.L2Regularization(0.05), iterations=n)
    Ad = rls.DeviceMatrix.from_host(np.array(A, order="F"), ctx)
    mk_dev = lambda: rls.createLinearSolver(rls.Kaczmarz, Ad, reg=rls.L2Regularization(0.05), iterations=6)
    # which sweep kernel ran: counting proxies on the two entry points
    calls = {"rls_kaczmarz_sweep": 0, "rls_kaczmarz_sweep_d": 0}
    orig = {n: getattr(ctx.lib, n) for n in calls}

    def proxy(n):
        def f(*a):
            calls[n] += 1
            return orig[n](*a)
        return f
    for n in calls:
        setattr(ctx.lib, n, proxy(n))
    try:
        warm_cases(rls, ctx, f"warm_kaczmarz_{np.dtype(dt).name}", dt, A, b, A64, b64, g, mk_ref, mk_dev, NO_THETA, 6,
                   bar=ITER_TOL if is_double(dt) else None)
    finally:
        for n in calls:
            setattr(ctx.lib, n, orig[n])
    mine, other = ("rls_kaczmarz_sweep_d", "rls_kaczmarz_sweep") if is_double(dt) else ("rls_kaczmarz_sweep", "rls_kaczmarz_sweep_d")
    assert calls[mine] > 0 and calls[other] == 0, calls


@pytest.mark.parametrize("which", ["f32", "f64", "gram"])
def test_cgnr_refuses_a_start_and_leaves_b_alone(rls, ctx, which):
    dt = np.float64 if which == "f64" else np.float32
    A, b, A64, b64, _, _, g = problem(96, 40, np.dtype(dt).name, 21)
    Ad, bd = rls.DeviceMatrix.from_host(np.array(A, order="F"), ctx), rls.DeviceVector.from_host(np.array(b), ctx)
    S = rls.createLinearSolver(rls.CGNR, Ad, AHA=Ad.gram() if which == "gram" else None, iterations=5, relTol=0.0)
    cold = rls.solve_(S, bd).to_host()
    for x0 in (np.array(g), rls.DeviceVector.from_host(np.array(g), ctx), 0.25):
        with pytest.raises(NotImplementedError):
            rls.solve_(S, bd, x0=x0)
        with pytest.raises(NotImplementedError):
            rls.init_(S, bd, x0=x0)
    assert np.array_equal(bd.to_host(), b)
    assert np.array_equal(rls.solve_(S, bd).to_host(), cold)


# ------------------------------------------------------------------------------------------------------------------
# 4. properties
# ------------------------------------------------------------------------------------------------------------------
def _solver_zoo(rls, ctx, which):
    """(dtype, problem, oracle factory, device factory, init keywords' theta?, path check) for the stale-state and aliasing tests"""
    shapes = {"fista_small": (np.float32, 256, 128), "fista_resident": (np.complex64, 4096, 2048), "fista_gram_resident": (np.float32, 300, 120),
              "fista_f64": (np.float64, 96, 40), "pogm_resident": (np.complex64, 4096, 2048), "admm": (np.float32, 120, 48), "pogm": (np.complex64, 256, 96)}
    dt, M, N = shapes[which]
    P = problem(M, N, np.dtype(dt).name, 2)
    A, b, A64, b64, rho, lam, g = P
    Ad = rls.DeviceMatrix.from_host(np.array(A, order="F"), ctx)
    its = 8
    if which.startswith("fista"):
        gram = which == "fista_gram_resident"
        Gd = Ad.gram() if gram else None
        mk_ref = lambda A_: O.FISTA(A_, reg=O.L1Regularization(lam), rho=rho, iterations=its, relTol=0.0, normal="gram" if gram else "matrixfree")
        mk_dev = lambda: rls.createLinearSolver(rls.FISTA, Ad, AHA=Gd, reg=rls.L1Regularization(lam), rho=rho, iterations=its, relTol=0.0)
        want = {"fista_small": 8, "fista_resident": 4, "fista_gram_resident": 5, "fista_f64": None}[which]

        def check(S):
            if want is None:
                assert S.state._plan_d and plan_path(rls, ctx, S) in (0, 1)
            elif _fista_path(ctx, S) != want:
                _resident_unavailable() if want in (4, 5) else pytest.fail(f"path {_fista_path(ctx, S)}, not {want}")
        return dt, P, mk_ref, mk_dev, True, check
    if which.startswith("pogm"):
        mk_ref = lambda A_: O.POGM(A_, reg=O.L1Regularization(lam), rho=rho, iterations=its, relTol=0.0)
        mk_dev = lambda: rls.createLinearSolver(rls.POGM, Ad, reg=rls.L1Regularization(lam), rho=rho, iterations=its, relTol=0.0)

        on_path = pgm_on_path(rls, "resident" if which == "pogm_resident" else "fused")
        return dt, P, mk_ref, mk_dev, True, lambda S: on_path(S, S.state, None)   # (ref = the state itself: the path alone)
    kw = dict(rho=0.3, iterations=6, iterationsCG=2, tolInner=1e-4)
    mk_ref = lambda A_: O.ADMM(A_, reg=O.L1Regularization(0.05), **kw)
    mk_dev = lambda: rls.createLinearSolver(rls.ADMM, Ad, reg=rls.L1Regularization(0.05), **kw)
    return dt, P, mk_ref, mk_dev, False, lambda S: S.state._plan_ok or pytest.fail("no device plan")


@pytest.mark.parametrize("which", ["fista_small", "fista_resident", "fista_gram_resident", "fista_f64", "pogm_resident"])
def test_a_warm_solve_leaves_no_state_behind(rls, ctx, which):
    """solve_(S, b, x0, theta = 1.7) and then solve_(S, b): the second result is, bit for bit, a fresh solver's cold solve"""
    dt, (A, b, A64, b64, rho, lam, g), mk_ref, mk_dev, _, check = _solver_zoo(rls, ctx, which)
    bd = rls.DeviceVector.from_host(np.array(b), ctx)
    fresh = mk_dev()
    cold = rls.solve_(fresh, bd).to_host()
    check(fresh)
    S = mk_dev()
    warm = rls.solve_(S, bd, x0=np.array(g), theta=1.7).to_host()
    check(S)
    assert not np.array_equal(warm, cold)
    again = rls.solve_(S, bd).to_host()
    check(S)
    assert np.array_equal(again, cold)
    assert S.state.theta == fresh.state.theta and S.state.iteration == fresh.state.iteration


@pytest.mark.parametrize("through", ["returned", "solversolution"])
@pytest.mark.parametrize("which", ["fista_resident", "fista_small", "fista_f64", "admm", "pogm"])
def test_start_aliasing_the_solvers_own_buffers(rls, ctx, which, through):
    """x1 = solve_(S, b1), not downloaded, then solve_(S, b2, x0 = x1): x1 lives in the state's own buffers, which init! resets;
    the result is the oracle's started from x1's values (taken from a copy made before the second call)"""
    dt, (A, b, A64, b64, rho, lam, g), mk_ref, mk_dev, _, check = _solver_zoo(rls, ctx, which)
    b2 = (2 * b[::-1] - 1).astype(dt)     # another right-hand side
    b2_64 = b2.astype(hi(dt))
    S = mk_dev()
    x1 = rls.solve_(S, rls.DeviceVector.from_host(np.array(b), ctx))
    if through == "solversolution":
        x1 = rls.solversolution(S)
    x1_host = x1.copy().to_host()
    want, _ = run_oracle(mk_ref(A64), b2_64, x0=x1_host.astype(hi(dt)))
    cold, _ = run_oracle(mk_ref(A64), b2_64)
    ww = want if is_double(dt) else run_oracle(mk_ref(A), b2, x0=x1_host)[0]
    bar = ITER_TOL if is_double(dt) else None
    apart_enough(f"warm_alias_{which}_{through}", want["last"], cold["last"], bar, ww["last"])
    x2 = rls.solve_(S, rls.DeviceVector.from_host(b2, ctx), x0=x1).to_host()
    check(S)
    held(f"warm_alias_{which}_{through}", x2, want["last"], bar, ww["last"])


@pytest.mark.parametrize("scheduler", ["BatchedState", "SequentialState", "MultiThreadingState"])
@pytest.mark.parametrize("solver", ["FISTA", "OptISTA", "POGM", "ADMM"])
def test_matrix_right_hand_side_with_a_start(rls, ctx, solver, scheduler):
    """solve_(S, B, x0 = ..., scheduler = ...): every column is the oracle's warm-started column solve -- never the cold-start
    columns.  The shared-A batched plans take no start vector: with x0 a BatchedState request is served by the per-column
    MultiThreadingState (one plan per column), the two per-column schedulers as asked for."""
    dt, M, N, K = np.complex64, 128, 48, 3
    A, b, A64, b64, rho, lam, g = problem(M, N, "complex64", 71)
    rng = np.random.default_rng(72)
    B = np.asfortranarray(np.stack([b, 2 * b - 1, (A @ rng.standard_normal(N)).astype(dt)], axis=1))
    if solver == "ADMM":
        kw = dict(rho=0.3, iterations=6, iterationsCG=2, tolInner=1e-4)
        mk_ref = lambda A_: O.ADMM(A_, reg=O.L1Regularization(0.05), **kw)
        S = rls.createLinearSolver(rls.ADMM, rls.DeviceMatrix.from_host(np.array(A, order="F"), ctx), reg=rls.L1Regularization(0.05), **kw)
        init_kw = {}
    else:
        mk_ref = lambda A_: getattr(O, solver)(A_, reg=O.L1Regularization(lam), rho=rho, iterations=8, relTol=0.0)
        S = rls.createLinearSolver(getattr(rls, solver), rls.DeviceMatrix.from_host(np.array(A, order="F"), ctx), reg=rls.L1Regularization(lam),
                                   rho=rho, iterations=8, relTol=0.0)
        init_kw = {"theta": 1.7}
    refs = [(run_oracle(mk_ref(A64), B[:, j].astype(hi(dt)), x0=g.astype(hi(dt)), **init_kw)[0]["last"],
             run_oracle(mk_ref(A64), B[:, j].astype(hi(dt)), **init_kw)[0]["last"],
             run_oracle(mk_ref(A), B[:, j].copy(), x0=g, **init_kw)[0]["last"]) for j in range(K)]
    for j in range(K):
        apart_enough(f"warm_matrix_{solver}_{scheduler}_col{j}", refs[j][0], refs[j][1], None, refs[j][2])
    X = rls.solve_(S, rls.DeviceMatrix.from_host(B, ctx), x0=rls.DeviceVector.from_host(np.array(g), ctx),
                   scheduler=getattr(rls, scheduler), **init_kw)
    want_state = rls.MultiThreadingState if scheduler == "BatchedState" else getattr(rls, scheduler)
    assert type(S.state) is want_state and len(S.state.states) == K
    for st in S.state.states:   # one single-column state per column, on its own device plan where the solver has one
        assert st.iteration == (6 if solver == "ADMM" else 8)
        assert {"FISTA": lambda: bool(st._plan), "ADMM": lambda: st._plan_ok}.get(solver, lambda: True)()
    X = X.to_host() if hasattr(X, "to_host") else np.stack([c.to_host() for c in X], axis=1)
    for j in range(K):
        held(f"warm_matrix_{solver}_{scheduler}_col{j}", X[:, j], refs[j][0], None, refs[j][2])


@pytest.mark.parametrize("solver", ["FISTA", "FISTA-tv-primitives", "FISTA-f64", "OptISTA", "POGM", "ADMM", "SplitBregman", "Kaczmarz"])
def test_wrong_length_or_element_type_of_the_start(rls, ctx, solver):
    """a DimensionMismatch, before anything is solved: a host array and a device vector of the wrong length, a device vector of
    another element type, complex values for a real solution"""
    dt = np.float64 if solver == "FISTA-f64" else np.float32
    other = np.float32 if solver == "FISTA-f64" else np.complex64
    A, b, A64, b64, rho, lam, g = problem(96, 40, np.dtype(dt).name, 21)
    Ad, bd = rls.DeviceMatrix.from_host(np.array(A, order="F"), ctx), rls.DeviceVector.from_host(np.array(b), ctx)
    if solver.startswith("FISTA"):
        reg = rls.TVRegularization(lam, shape=(8, 5)) if "tv" in solver else rls.L1Regularization(lam)
        S = rls.createLinearSolver(rls.FISTA, Ad, reg=reg, rho=rho, iterations=4)
        if "tv" in solver:
            S._tv_unfused = True
    elif solver in ("OptISTA", "POGM"):
        S = rls.createLinearSolver(getattr(rls, solver), Ad, reg=rls.L1Regularization(lam), rho=rho, iterations=4)
    elif solver == "Kaczmarz":
        S = rls.createLinearSolver(rls.Kaczmarz, Ad, reg=rls.L2Regularization(0.05), iterations=2)
    else:
        S = rls.createLinearSolver(getattr(rls, solver), Ad, reg=rls.L1Regularization(0.05), rho=0.3, iterations=3)
    bad = [np.array(g[:10]), rls.DeviceVector.from_host(np.array(g[:10]), ctx), np.zeros((40, 2), dt),
           rls.DeviceVector.from_host(np.array(g).astype(other), ctx), (1j * g).astype(np.complex128)]
    for x0 in bad:
        with pytest.raises(ValueError, match="DimensionMismatch"):
            rls.init_(S, bd, x0=x0)
        with pytest.raises(ValueError, match="DimensionMismatch"):
            rls.solve_(S, bd, x0=x0)
    assert rls.solve_(S, bd, x0=np.array(g)).to_host().shape == (40,)   # and the right one is taken
