"""solve!(solver::SplitBregman, B) with the shared-A scheduler: the batched ADMM plan in its Bregman mode
(rls_admm_set_bregman, SplitBregmanBatchedState).  Every column against its own oracle solve (src/SplitBregman.jl:205-281):
the solution through the parity gate, the number of inner iterations and the inner cg! counts against the Float32 oracle.

The oracle solves of a case are computed once (functools.lru_cache) and shared by the tests that use the case."""
import functools
import math

import numpy as np
import pytest

import rls_oracle as O

pytestmark = pytest.mark.gpu

F32, C64 = np.float32, np.complex64
COMMON = dict(rho=0.3, iterations=3, iterationsInner=4, iterationsCG=6, tolInner=1e-4, absTol=0.0, relTol=0.0)


def hi(dt):
    return np.complex128 if np.dtype(dt).kind == "c" else np.float64


def rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def regs(R, kind):
    if kind == "l1":
        return R.L1Regularization(0.05)
    if kind == "l1pos":
        return [R.L1Regularization(0.05), R.PositiveRegularization()]
    if kind == "tv":
        return R.TVRegularization(2e-2, shape=(8, 8))
    return R.L2Regularization(0.3)


def settings(iterations=3, inner=4):
    return dict(COMMON, iterations=iterations, iterationsInner=inner)


@functools.lru_cache(maxsize=None)
def case(dt, M, N, K, kind, iterations=3, inner=4):
    """the problem and, per column, the Float32 oracle (the reference's own path: counts, the fallback bound of the gate)
    and the float64 oracle's solution"""
    A, _, B = O.make_problem(M, N, dt, 61, n_rhs=K)
    B = np.asfortranarray(B * (3.0 ** (np.arange(K) % 4))[None, :]).astype(dt)  # columns of different scales
    kw = settings(iterations, inner)
    ref32, x64 = [], []
    for j in range(K):
        r = O.SplitBregman(A, reg=regs(O, kind), **kw)
        O.solve(r, np.ascontiguousarray(B[:, j]))
        ref32.append(r)
        x64.append(np.array(O.solve(O.SplitBregman(A.astype(hi(dt)), reg=regs(O, kind), **kw), B[:, j].astype(hi(dt)))))
    for a in [A, B] + x64:
        a.setflags(write=False)
    return A, B, kw, ref32, x64


def solve_batched(rls, ctx, A, B, kind, kw, **more):
    S = rls.createLinearSolver(rls.SplitBregman, rls.DeviceMatrix.from_host(A, ctx), reg=regs(rls, kind), **kw)
    xs = rls.solve_(S, rls.DeviceMatrix.from_host(B, ctx), scheduler=rls.BatchedState, **more)
    return S, [x.to_host() for x in xs]


# ---- 1. parity per column ----------------------------------------------------------------------------------------------
# K = 20: two operand groups of 16 columns, the second ragged.  iterationsInner = 1: a Bregman update in front of every
# inner iteration but the first.  iterationsInner = 3: blocks of odd length, so the z buffer the update writes alternates.
@pytest.mark.parametrize("dt,M,N,K,kind,iterations,inner", [(C64, 128, 48, 3, "l1", 3, 4), (F32, 320, 144, 4, "l2", 3, 4),
                                                            (F32, 512, 256, 20, "l1pos", 3, 4), (C64, 128, 48, 3, "l1", 3, 1),
                                                            (F32, 320, 144, 4, "l2", 3, 3)])
def test_columns_against_the_oracle(rls, ctx, parity, dt, M, N, K, kind, iterations, inner):
    A, B, kw, ref32, x64 = case(dt, M, N, K, kind, iterations, inner)
    S, xs = solve_batched(rls, ctx, A, B, kind, kw)
    assert type(S.state).__name__ == "SplitBregmanBatchedState"
    stat, cgits, counters = S.state.status(), S.state.cg_iterations(), S.state.counters()
    for j in range(K):
        r = ref32[j]
        assert stat[j].iteration == iterations * inner == len(r.cg_iters) and stat[j].done, (j, stat[j].iteration)
        assert cgits[j] == r.cg_iters, (j, cgits[j], r.cg_iters)
        assert counters[j] == (r.iter_cnt, r.iteration), (j, counters[j], r.iter_cnt, r.iteration)
        parity(f"splitbregman_batched_{kind}_{M}x{N}_{np.dtype(dt).name}_K{K}_inner{inner}_col{j}", xs[j], x64[j], r.x, record=(j < 2))


# ---- 2. early retirement ----------------------------------------------------------------------------------------------
def test_a_column_that_converges_retires_alone(rls, ctx, parity):
    """Column 1 is a thousand times smaller.  absTol comes from the float64 oracle's own history of max(rk, sk) with the
    stopping rule off: column 1 meets `converged` at its 7th inner iteration -- the third of its second block, so it has
    taken one Bregman update -- and no other column meets it while that matters.  The retired column keeps the x of that
    iteration; the other columns are, to the bit, what they are when column 1 holds other data."""
    dt, M, N, K = C64, 128, 48, 3
    A, _, B0 = O.make_problem(M, N, dt, 61, n_rhs=K)
    B0 = np.asfortranarray(B0).astype(dt)
    B = B0.copy(order="F")
    B[:, 1] *= 1e-3
    kw = dict(rho=1.0, iterations=3, iterationsInner=4, iterationsCG=3, tolInner=1e-4, relTol=0.0)
    reg = lambda R: R.L1Regularization(1e-4)
    total, stop = 12, 7
    hist = []
    for j in range(K):
        o = O.SplitBregman(A.astype(hi(dt)), reg=reg(O), absTol=0.0, **kw)
        o.init(B[:, j].astype(hi(dt)))
        h = []
        while o.iterate() is not None:
            h.append(max(float(o.rk[0]), float(o.sk[0])))
        assert len(h) == total
        hist.append(h)
    # (a value of the last inner iteration is never tested: the column is done by its count there)
    below, above = hist[1][stop - 1], min(hist[1][:stop - 1] + hist[0][:total - 1] + hist[2][:total - 1])
    assert below < 0.5 * above, (hist, "column 1 must cross a threshold that nothing else crosses")
    absTol = math.sqrt(below * above) / math.sqrt(M)
    want = []
    for j in range(K):
        r = O.SplitBregman(A, reg=reg(O), absTol=absTol, **kw)
        O.solve(r, np.ascontiguousarray(B[:, j]))
        want.append(r)
    assert [len(r.cg_iters) for r in want] == [total, stop, total]
    S = rls.createLinearSolver(rls.SplitBregman, rls.DeviceMatrix.from_host(A, ctx), reg=reg(rls), absTol=absTol, **kw)
    xs = [x.to_host() for x in rls.solve_(S, rls.DeviceMatrix.from_host(B, ctx), scheduler=rls.BatchedState)]
    assert type(S.state).__name__ == "SplitBregmanBatchedState"
    stat = S.state.status()
    assert [s.iteration for s in stat] == [len(r.cg_iters) for r in want] and all(s.done for s in stat)
    assert S.state.cg_iterations() == [r.cg_iters for r in want]
    assert S.state.counters() == [(r.iter_cnt, r.iteration) for r in want]
    # the retired column: an oracle solve stopped at that count
    o = O.SplitBregman(A.astype(hi(dt)), reg=reg(O), absTol=0.0, **kw)
    o.init(B[:, 1].astype(hi(dt)))
    for _ in range(stop):
        o.iterate()
    parity("splitbregman_batched_retired_column", xs[1], np.array(o.x), want[1].x, record=False)
    for j in (0, 2):
        o64 = O.SplitBregman(A.astype(hi(dt)), reg=reg(O), absTol=0.0, **kw)
        parity(f"splitbregman_batched_beside_a_retired_column_col{j}", xs[j], np.array(O.solve(o64, B[:, j].astype(hi(dt)))), want[j].x,
               record=False)
    # one column's data changes no other column
    S2 = rls.createLinearSolver(rls.SplitBregman, rls.DeviceMatrix.from_host(A, ctx), reg=reg(rls), absTol=absTol, **kw)
    ys = [x.to_host() for x in rls.solve_(S2, rls.DeviceMatrix.from_host(B0, ctx), scheduler=rls.BatchedState)]
    assert S2.state.status()[1].iteration > stop   # (column 1 at full scale goes on)
    for j in (0, 2):
        assert np.array_equal(xs[j], ys[j]), j


# ---- 3. agreement with the per-column path --------------------------------------------------------------------------
def test_per_column_scheduler_gives_the_same_columns(rls, ctx):
    A, B, kw, _, _ = case(C64, 128, 48, 3, "l1")
    _, xs = solve_batched(rls, ctx, A, B, "l1", kw)
    S = rls.createLinearSolver(rls.SplitBregman, rls.DeviceMatrix.from_host(A, ctx), reg=regs(rls, "l1"), **kw)
    ys = rls.solve_(S, rls.DeviceMatrix.from_host(B, ctx), scheduler=rls.MultiThreadingState)
    assert type(S.state).__name__ == "MultiThreadingState"
    for j in range(3):
        assert rel(xs[j], ys[j].to_host()) < 2e-5, j  # two device paths, each gated against the oracle (test 1 and test_gpu_parity)


# ---- 4. lifecycle -------------------------------------------------------------------------------------------------------
def test_one_solver_object_through_batched_vector_batched(rls, ctx):
    A, B, kw, _, _ = case(C64, 128, 48, 3, "l1")
    Ad = rls.DeviceMatrix.from_host(A, ctx)
    make = lambda: rls.createLinearSolver(rls.SplitBregman, Ad, reg=regs(rls, "l1"), **kw)

    def solve(S, k):
        if k is None:
            return rls.solve_(S, rls.DeviceVector.from_host(np.ascontiguousarray(B[:, 1]), ctx)).to_host()
        out = rls.solve_(S, rls.DeviceMatrix.from_host(np.asfortranarray(B[:, :k]), ctx), scheduler=rls.BatchedState)
        return np.stack([x.to_host() for x in out], axis=1)

    steps = [3, None, 3, 3, 2]
    fresh = {k: solve(make(), k) for k in set(steps)}
    S, seen = make(), []
    for step, k in enumerate(steps):
        assert np.array_equal(solve(S, k), fresh[k]), (step, k)
        assert type(S.state).__name__ == ("ADMMState" if k is None else "SplitBregmanBatchedState")
        if k is not None:
            assert S.state.K == k and (S.state.absTol, S.state.relTol, S.state.tolInner) == (0.0, 0.0, np.float32(1e-4))
        seen.append(S.state)
    assert seen[2] is not seen[0]   # the vector solve in between put a plain state in its place
    assert seen[3] is seen[2]       # taken over, plan and state matrices, while K stays
    assert seen[4] is not seen[3]


# ---- 5. fallbacks still fall back -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["tv", "x0", "precon", "n1025", "gram_only"])
def test_what_the_plan_does_not_cover_runs_column_by_column(rls, ctx, parity, what):
    dt, K = F32, 2
    M, N = {"tv": (256, 64), "n1025": (1089, 1025)}.get(what, (128, 48))
    kind = "tv" if what == "tv" else "l1"
    A, _, B = O.make_problem(M, N, dt, 67, n_rhs=K)
    B = np.asfortranarray(B).astype(dt)
    kw = settings(2, 3)
    A64 = A.astype(hi(dt))
    okw, okw64, skw, init_kw = {}, {}, {}, {}
    A_dev = rls.DeviceMatrix.from_host(A, ctx)
    if what == "x0":
        g = np.linspace(0.5, 1.5, N).astype(dt)
        init_kw = dict(x0=rls.DeviceVector.from_host(g, ctx))
    elif what == "precon":
        d = np.sum(np.abs(A64) ** 2, axis=0) + kw["rho"]
        okw, okw64 = dict(precon=lambda r: (r / d).astype(dt)), dict(precon=lambda r: r / d)
        skw = dict(precon=rls.DiagonalPreconditioner(rls.DeviceVector.from_host(d.astype(dt), ctx)))
    elif what == "gram_only":
        G64 = A64.T @ A64
        G = np.asfortranarray(G64.astype(dt))
        B = np.asfortranarray(A.T @ B).astype(dt)   # b = A' b of the full problem: the right-hand side of the Gram-only solver
        okw, okw64 = dict(AHA=G), dict(AHA=G.astype(hi(dt)))
        skw = dict(AHA=rls.DeviceMatrix.from_host(G, ctx))
        A = A64 = A_dev = None
    S = rls.createLinearSolver(rls.SplitBregman, A_dev, reg=regs(rls, kind), **kw, **skw)
    xs = rls.solve_(S, rls.DeviceMatrix.from_host(B, ctx), scheduler=rls.BatchedState, **init_kw)
    assert type(S.state).__name__ == "MultiThreadingState" and len(S.state.states) == K
    for j in range(K):
        o64 = O.SplitBregman(A64, reg=regs(O, kind), **kw, **okw64)
        o32 = O.SplitBregman(A, reg=regs(O, kind), **kw, **okw)
        start = dict(x0=g) if what == "x0" else {}
        o64.init(B[:, j].astype(hi(dt)), **{k: v.astype(hi(dt)) for k, v in start.items()})
        o32.init(np.ascontiguousarray(B[:, j]), **start)
        for o in (o64, o32):
            while o.iterate() is not None:
                pass
        parity(f"splitbregman_fallback_{what}_col{j}", xs[j].to_host(), np.array(o64.x), np.array(o32.x), record=False)


# ---- 6. callbacks -------------------------------------------------------------------------------------------------------
def test_callbacks_see_every_inner_iteration(rls, ctx):
    A, B, kw, _, _ = case(C64, 128, 48, 3, "l1")
    _, want = solve_batched(rls, ctx, A, B, "l1", kw)
    cb = rls.StoreSolutionCallback()
    S, xs = solve_batched(rls, ctx, A, B, "l1", kw, callbacks=cb)
    assert type(S.state).__name__ == "SplitBregmanBatchedState"
    assert len(cb.solutions) == kw["iterations"] * kw["iterationsInner"] + 1
    assert all(np.array_equal(a, b) for a, b in zip(cb.solutions[-1], xs))
    assert all(np.array_equal(a, b) for a, b in zip(xs, want))   # stepped one by one or enqueued at once: the same launches
    assert not np.any(cb.solutions[0][0]) and not np.array_equal(cb.solutions[1][0], cb.solutions[2][0])
    assert S.state.active == [False] * 3
