"""A plan's blocks are zero-filled where its kernels rely on it, whatever the memory held before.

Every solver plan takes its scratch from the context's stream-ordered pool, which hands freed blocks out again as they are.
Each case below solves, destroys the solver, fills a few MiB of that pool with NaN through the same context, frees them, and
creates and solves again -- three times.  Every path here is fixed-order, so the later results must be the bits of the first;
a block whose zero-fill got lost (padding columns of an operand panel, rows >= N of an exchange buffer, partial-dot slots of
absent workgroups, arrival counters, the scalars) shows up as other bits or as NaN.  The shapes are the smallest ones the tests
of the individual paths pin to them (rls_cgnr_path / rls_fista_path / the *_d variants)."""
import ctypes as C
import gc

import numpy as np
import pytest

import rls_oracle as O

pytestmark = pytest.mark.gpu

CYCLES = 3


def dirty_pool(rls, ctx):
    """a few MiB of the context's pool written with NaN, in blocks from 4 KiB to 4 MiB, and given back"""
    blocks = [rls.DeviceVector.from_host(np.full(n, np.nan, dtype=np.float32), ctx) for n in (1 << 10, 1 << 12, 1 << 14, 1 << 16, 1 << 18, 1 << 20)]
    blocks += [rls.DeviceVector.from_host(np.full(1 << 12, np.nan, dtype=np.float32), ctx) for _ in range(32)]
    ctx.sync()
    del blocks
    gc.collect()
    ctx.sync()


def cycle(rls, ctx, solve_once):
    """`solve_once()` creates a solver, solves and returns (host arrays, path); the solver dies with its frame"""
    first, path = solve_once()
    assert all(np.all(np.isfinite(x)) for x in first)
    for k in range(CYCLES):
        gc.collect()
        dirty_pool(rls, ctx)
        again, path_k = solve_once()
        assert path_k == path
        for j, (a, b) in enumerate(zip(first, again)):
            assert np.array_equal(a, b), (k, j, float(np.max(np.abs(a - b))))


def plan_path(ctx, S, fn):
    out = C.c_int32(-1)
    assert getattr(ctx.lib, fn)(S.state._plan, C.byref(out)) == 0
    return out.value


def columns(xs):
    return [x.to_host() for x in xs]


# name, M, N, K (0: one right-hand side), explicit Gram matrix, resident tuning, expected rls_cgnr_path
CGNR = [("pipeline", 1024, 2048, 0, False, 0, 1), ("resident", 1024, 2048, 0, False, 1, 4), ("gram pipeline", 90, 46, 0, True, 0, 2),
        ("gram resident", 90, 46, 0, True, 1, 5), ("small system", 96, 24, 0, False, 1, 8), ("batched skinny", 1040, 208, 7, False, 1, 3),
        ("batched gramk", 4096, 2048, 8, True, 1, 7)]


@pytest.mark.parametrize("name,M,N,K,gram,resident,want", CGNR, ids=[c[0] for c in CGNR])
def test_cgnr_plan_recreated_on_dirty_memory(rls, ctx, name, M, N, K, gram, resident, want):
    A, _, B = O.make_problem(M, N, np.complex64, 11, n_rhs=max(K, 1)) if K else O.make_problem(M, N, np.complex64, 11)
    Ad = rls.DeviceMatrix.from_host(A, ctx)
    Gd = Ad.gram() if gram else None
    Bd = rls.DeviceMatrix.from_host(np.asfortranarray(B), ctx) if K else rls.DeviceVector.from_host(B, ctx)
    ctx.tune(resident=resident)

    def solve_once():
        S = rls.createLinearSolver(rls.CGNR, Ad, AHA=Gd, reg=rls.L2Regularization(1e-3), iterations=8, relTol=0.0)
        xs = columns(rls.solve_(S, Bd, scheduler=rls.BatchedState)) if K else [rls.solve_(S, Bd).to_host()]
        return xs, plan_path(ctx, S, "rls_cgnr_path")

    try:
        cycle(rls, ctx, solve_once)
        assert solve_once()[1] == want
    finally:
        ctx.tune(resident=1)


# name, M, N, K, explicit Gram matrix, resident tuning, expected rls_fista_path
FISTA = [("pipeline", 4096, 2048, 0, False, 0, 1), ("resident", 4096, 2048, 0, False, 1, 4), ("gram pipeline", 70, 34, 0, True, 0, 2),
         ("gram resident", 70, 34, 0, True, 1, 5), ("small system", 96, 24, 0, False, 1, 8), ("batched", 1040, 208, 7, False, 1, 3),
         ("batched fgramk", 1040, 208, 7, True, 1, 7)]


@pytest.mark.parametrize("name,M,N,K,gram,resident,want", FISTA, ids=[c[0] for c in FISTA])
def test_fista_plan_recreated_on_dirty_memory(rls, ctx, name, M, N, K, gram, resident, want):
    A, _, B = O.make_problem(M, N, np.complex64, 13, n_rhs=max(K, 1)) if K else O.make_problem(M, N, np.complex64, 13)
    rho = 0.9 / (np.sqrt(M) + np.sqrt(N)) ** 2 / 2  # (sigma_max of the Gaussian matrix is below sqrt M + sqrt N; complex: variance 2)
    Ad = rls.DeviceMatrix.from_host(A, ctx)
    Gd = Ad.gram() if gram else None
    Bd = rls.DeviceMatrix.from_host(np.asfortranarray(B), ctx) if K else rls.DeviceVector.from_host(B, ctx)
    ctx.tune(resident=resident)

    def solve_once():
        S = rls.createLinearSolver(rls.FISTA, Ad, AHA=Gd, reg=rls.L1Regularization(1e-2), rho=float(rho), iterations=10, relTol=0.0)
        xs = columns(rls.solve_(S, Bd, scheduler=rls.BatchedState)) if K else [rls.solve_(S, Bd).to_host()]
        return xs, plan_path(ctx, S, "rls_fista_path")

    try:
        cycle(rls, ctx, solve_once)
        assert solve_once()[1] == want
    finally:
        ctx.tune(resident=1)


@pytest.mark.parametrize("K", [0, 3], ids=["single", "batched"])
def test_admm_plan_recreated_on_dirty_memory(rls, ctx, K):
    """rls_cg (slab pipeline / resident; batched: the operand panels) and rls_admm with its log"""
    M, N = (128, 64) if K == 0 else (128, 48)
    A, _, B = O.make_problem(M, N, np.float32, 17, n_rhs=K) if K else O.make_problem(M, N, np.float32, 17)
    Ad = rls.DeviceMatrix.from_host(A, ctx)
    Bd = rls.DeviceMatrix.from_host(np.asfortranarray(B), ctx) if K else rls.DeviceVector.from_host(B, ctx)
    reg = rls.TVRegularization(1e-2, shape=(8, 8)) if K == 0 else rls.L1Regularization(0.05)

    def solve_once():
        S = rls.createLinearSolver(rls.ADMM, Ad, reg=reg, rho=0.3, iterations=5, iterationsCG=5, tolInner=1e-5)
        xs = columns(rls.solve_(S, Bd, scheduler=rls.BatchedState)) if K else [rls.solve_(S, Bd).to_host()]
        return xs, type(S.state).__name__

    cycle(rls, ctx, solve_once)
    assert solve_once()[1] == ("AdmmBatchedState" if K else "ADMMState")


@pytest.mark.parametrize("solver", ["OptISTA", "POGM"])
def test_pgm_batched_plan_recreated_on_dirty_memory(rls, ctx, solver):
    M, N, K = 128, 48, 3
    A, _, B = O.make_problem(M, N, np.complex64, 19, n_rhs=K)
    rho = 0.9 / np.linalg.norm(A.astype(np.complex128), 2) ** 2
    Ad, Bd = rls.DeviceMatrix.from_host(A, ctx), rls.DeviceMatrix.from_host(np.asfortranarray(B), ctx)

    def solve_once():
        S = rls.createLinearSolver(getattr(rls, solver), Ad, reg=rls.L1Regularization(1e-2), rho=float(rho), iterations=10, relTol=0.0)
        xs = columns(rls.solve_(S, Bd, scheduler=rls.BatchedState))
        return xs, type(S.state).__name__

    cycle(rls, ctx, solve_once)
    assert solve_once()[1] == "PgmBatchedState"


@pytest.mark.parametrize("dt", [np.float64, np.complex128], ids=["f64", "c64"])
@pytest.mark.parametrize("solver", ["CGNR", "FISTA"])
@pytest.mark.parametrize("gram", [False, True], ids=["matrix-free", "gram"])
def test_double_precision_plan_recreated_on_dirty_memory(rls, ctx, dt, solver, gram):
    A, _, b = O.make_problem(96, 40, dt, 23)
    rho = 0.9 / np.linalg.norm(A, 2) ** 2
    Ad, bd = rls.DeviceMatrix.from_host(A, ctx), rls.DeviceVector.from_host(b, ctx)
    Gd = rls.DeviceMatrix.from_host(np.asfortranarray(A.conj().T @ A), ctx) if gram else None

    def solve_once():
        if solver == "CGNR":
            S = rls.createLinearSolver(rls.CGNR, Ad, AHA=Gd, reg=rls.L2Regularization(1e-2), iterations=10, relTol=0.0)
        else:
            S = rls.createLinearSolver(rls.FISTA, Ad, AHA=Gd, reg=rls.L1Regularization(1e-2), rho=float(rho), iterations=10, relTol=0.0)
        x = rls.solve_(S, bd).to_host()
        return [x], plan_path(ctx, S, "rls_cgnr_path_d" if solver == "CGNR" else "rls_fista_path_d")

    cycle(rls, ctx, solve_once)
    assert solve_once()[1] == (2 if gram else 0)
