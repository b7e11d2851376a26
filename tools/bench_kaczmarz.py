"""Kaczmarz row sweeps at 4096 x 2048 ComplexF32: row steps per second for one right-hand side
(latency-bound: one workgroup) and for K independent right-hand sides in one launch (one workgroup each).
Then the regularised / randomised solves as ONE launch (rls_kaczmarz_solve) against the host loop -- a launch per sweep and
per prox and column, ctx.tune(kaczmarz_fused=0) -- in the same process, at 4096 x 2048 and at 256 x 128: the minimum of 5
solves behind a warm-up solve, with the spread of the 5."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # noqa
import rls_amd as rls
from bench import make_A
from oracle import rls_oracle as O
ctx = rls.Context(0)
M, N = 4096, 2048
A = make_A(M, N, 2); Ad = rls.DeviceMatrix.from_host(A, ctx)
rng = np.random.default_rng(5)
sweeps = 10
if len(sys.argv) > 1:
    ctx.tune(kaczmarz_nt=int(sys.argv[1]))


def timed(S, b, kw):
    rls.solve_(S, b, **kw); ctx.sync()
    dts = []
    for _ in range(5):
        t0 = time.perf_counter(); rls.solve_(S, b, **kw); ctx.sync(); dts.append(time.perf_counter() - t0)
    return min(dts), sorted(dts)[2], max(dts)


for K in (1, 256):
    X = (rng.standard_normal((N, K)) + 1j * rng.standard_normal((N, K))).astype(np.complex64)
    B = np.asfortranarray((A @ X).astype(np.complex64))
    S = rls.createLinearSolver(rls.Kaczmarz, Ad, reg=rls.L2Regularization(1e-3), iterations=sweeps)
    b = rls.DeviceMatrix.from_host(B, ctx) if K > 1 else rls.DeviceVector.from_host(B[:, 0], ctx)
    kw = dict(scheduler=rls.BatchedState) if K > 1 else {}
    dt, med, worst = timed(S, b, kw)
    rows = sweeps * M
    print(f"K={K:4d}: {dt*1e3:8.2f} ms for {sweeps} sweeps = {dt/rows*1e6:6.3f} us per row step, "
          f"{K*rows/dt/1e6:8.2f} M row-updates/s, A stream {K*rows*N*8/dt/1e9:8.1f} GB/s   (median {med*1e3:.2f}, max {worst*1e3:.2f} ms)", flush=True)

# one launch against the host loop
for (m, n) in ((M, N), (256, 128)):
    Am = A if (m, n) == (M, N) else make_A(m, n, 2)
    Amd = Ad if (m, n) == (M, N) else rls.DeviceMatrix.from_host(Am, ctx)
    cases = [("L2 + Positive", K, dict(reg=[rls.L2Regularization(1e-3), rls.PositiveRegularization()])) for K in (1, 256)]
    cases.append(("randomized", 1, dict(reg=rls.L2Regularization(1e-3), randomized=True)))
    for name, K, skw in cases:
        X = (rng.standard_normal((n, K)) + 1j * rng.standard_normal((n, K))).astype(np.complex64)
        B = np.asfortranarray((Am @ X).astype(np.complex64))
        b = rls.DeviceMatrix.from_host(B, ctx) if K > 1 else rls.DeviceVector.from_host(B[:, 0], ctx)
        kw = dict(scheduler=rls.BatchedState) if K > 1 else {}
        out = {}
        for fused in (1, 0):
            ctx.tune(kaczmarz_fused=fused)
            S = rls.createLinearSolver(rls.Kaczmarz, Amd, iterations=sweeps, **skw)
            out[fused] = timed(S, b, kw)
        ctx.tune(kaczmarz_fused=1)
        (f, fm, fx), (h, hm, hx) = out[1], out[0]
        print(f"{m}x{n} {name:14s} K={K:4d}, {sweeps} sweeps: one launch {f*1e3:8.3f} ms (median {fm*1e3:.3f}, max {fx*1e3:.3f})   "
              f"host loop {h*1e3:8.3f} ms (median {hm*1e3:.3f}, max {hx*1e3:.3f})   x{h/f:5.2f}", flush=True)

# CPU: the oracle's NumPy loop on the same matrix (one sweep)
X = (rng.standard_normal((N, 1)) + 1j * rng.standard_normal((N, 1))).astype(np.complex64)
ref = O.Kaczmarz(A, reg=O.L2Regularization(1e-3), iterations=1)
t0 = time.perf_counter(); O.solve(ref, (A @ X[:, 0]).astype(np.complex64)); dt = time.perf_counter() - t0
print(f"CPU (NumPy port, 1 thread): {dt/M*1e6:.2f} us per row step")
