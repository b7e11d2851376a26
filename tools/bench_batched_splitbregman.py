"""solve!(solver::SplitBregman, B) with K columns sharing A (the batched ADMM plan in its Bregman mode, rls_admm_set_bregman)
against the per-column path (MultiThreadingState: K plans, one read-back per column and block of inner iterations) in the same
process: 4096 x 2048 CF32 + L1, iterations = 4, iterationsInner = 5, iterationsCG = 10, stopping rule off.  Whole solves timed
with hipEvents; one warm-up solve per scheduler outside the timed region (plan creation, code objects), then the two
schedulers alternate and the median of each is taken.  Machines of one pool differ by up to 15 %: only the ratio of the two
legs of one run says anything.   usage: bench_batched_splitbregman.py [K,K,...] [--once]   (--once: one batched solve per K and
nothing else, for a kernel trace)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # noqa
import rls_amd as rls
from bench import make_A
ctx = rls.Context(0)
M, N, REPS = 4096, 2048, 9
KW = dict(rho=0.3, iterations=4, iterationsInner=5, iterationsCG=10, tolInner=1e-6, absTol=0.0, relTol=0.0)
INNER = KW["iterations"] * KW["iterationsInner"]
A = make_A(M, N, 4); Ad = rls.DeviceMatrix.from_host(A, ctx)
rng = np.random.default_rng(5)
args = [a for a in sys.argv[1:] if not a.startswith("--")]
Ks = tuple(int(k) for k in args[0].split(",")) if args else (8, 16)
LEGS = [("BatchedState", rls.BatchedState, "SplitBregmanBatchedState"), ("MultiThreadingState", rls.MultiThreadingState, "MultiThreadingState")]


def timed_solve(S, Bd, scheduler, want):
    ctx.sync(); ctx.timer_start()
    xs = rls.solve_(S, Bd, scheduler=scheduler)
    ms = ctx.timer_stop_ms()
    assert type(S.state).__name__ == want, type(S.state).__name__
    return ms, xs


for K in Ks:
    X = (rng.standard_normal((N, K)) + 1j * rng.standard_normal((N, K))).astype(np.complex64)
    Bd = rls.DeviceMatrix.from_host(np.asfortranarray((A @ X).astype(np.complex64)), ctx)
    solvers = {leg: rls.createLinearSolver(rls.SplitBregman, Ad, reg=rls.L1Regularization(1e-2), **KW) for leg, _, _ in LEGS}
    if "--once" in sys.argv:
        timed_solve(solvers["BatchedState"], Bd, rls.BatchedState, "SplitBregmanBatchedState")
        continue
    out = {leg: timed_solve(solvers[leg], Bd, sched, want)[1] for leg, sched, want in LEGS}  # warm-up, and the two results
    err = max(float(np.linalg.norm(a.to_host() - b.to_host()) / np.linalg.norm(b.to_host()))
              for a, b in zip(out["BatchedState"], out["MultiThreadingState"]))
    times = {leg: [] for leg, _, _ in LEGS}
    for _ in range(REPS):
        for leg, sched, want in LEGS:
            times[leg].append(timed_solve(solvers[leg], Bd, sched, want)[0])
    ms = {leg: float(np.median(t)) for leg, t in times.items()}
    for leg, _, _ in LEGS:
        print(f"K={K:2d} {leg:21s}: {ms[leg]:8.3f} ms per solve (min {min(times[leg]):.3f}, max {max(times[leg]):.3f}) = "
              f"{ms[leg] * 1e3 / INNER:8.2f} us per inner iteration of all columns", flush=True)
    print(f"K={K:2d} MultiThreadingState / BatchedState: {ms['MultiThreadingState'] / ms['BatchedState']:.2f}x   "
          f"(largest column difference between the two: {err:.2e})", flush=True)
