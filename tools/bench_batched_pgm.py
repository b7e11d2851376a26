"""solve!(solver, B) for OptISTA / POGM / POGM + gradient restart with K columns sharing A on the matrix cores
(rls_pgm_*_batched) against the per-column path (MultiThreadingState) in the same process: 4096 x 2048 CF32 + L1, relTol = 0,
whole solves timed with hipEvents, median of repeated solves after a warm-up solve; us per batched iteration and
solve-iterations per second.  usage: bench_batched_pgm.py [K,K,...] [--forms]   (--forms: also the strided update kernel)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # noqa
import rls_amd as rls
from bench import make_A
ctx = rls.Context(0)
M, N, ITERS, REPS = 4096, 2048, 48, 7
A = make_A(M, N, 4); Ad = rls.DeviceMatrix.from_host(A, ctx)
rng = np.random.default_rng(5)
rho = 0.95 / (np.sqrt(M) + np.sqrt(N)) ** 2
args = [a for a in sys.argv[1:] if not a.startswith("--")]
Ks = tuple(int(k) for k in args[0].split(",")) if args else (8, 16, 64)
VARIANTS = [("OptISTA", rls.OptISTA, {}), ("POGM", rls.POGM, {}), ("POGM+restart", rls.POGM, {"restart": "gradient", "sigma_fac": 0.96})]


def median_ms(S, Bd, scheduler, want):
    times = []
    for rep in range(REPS + 1):  # the first solve is the warm-up (plan creation, graph capture, code objects)
        ctx.sync(); ctx.timer_start()
        rls.solve_(S, Bd, scheduler=scheduler)
        ms = ctx.timer_stop_ms()
        assert type(S.state).__name__ == want, type(S.state).__name__
        if rep:
            times.append(ms)
    return float(np.median(times))


for K in Ks:
    X = (rng.standard_normal((N, K)) + 1j * rng.standard_normal((N, K))).astype(np.complex64)
    Bd = rls.DeviceMatrix.from_host(np.asfortranarray((A @ X).astype(np.complex64)), ctx)
    for label, T, kw in VARIANTS:
        legs = [("BatchedState", rls.BatchedState, "PgmBatchedState", {}), ("MultiThreadingState", rls.MultiThreadingState, "MultiThreadingState", {})]
        if "--forms" in sys.argv:
            legs.insert(1, ("BatchedState/strided", rls.BatchedState, "PgmBatchedState", {"pgm_batched_reg": 0}))
        ms = {}
        for leg, sched, want, tune in legs:
            S = rls.createLinearSolver(T, Ad, reg=rls.L1Regularization(1e-2), rho=rho, iterations=ITERS, relTol=0.0, **kw)
            ctx.tune(**tune)
            try:
                ms[leg] = median_ms(S, Bd, sched, want)
            finally:
                ctx.tune(pgm_batched_reg=1)
            us = ms[leg] * 1e3 / ITERS
            print(f"K={K:2d} {label:13s} {leg:21s}: {us:8.2f} us per batched iteration = {us / K:6.2f} us per solve-iteration "
                  f"({K * 1e6 / us:8.0f} solve-it/s)", flush=True)
        print(f"K={K:2d} {label:13s} speed-up of BatchedState over MultiThreadingState: {ms['MultiThreadingState'] / ms['BatchedState']:.2f}x", flush=True)
