"""PseudoInverse (csrc/pinv.hip) beside DirectSolver and the host, in one process, at 4096 x 2048 ComplexF32 and 256 x 128 Float32:

  * the factorisation (a fresh plan per repetition: rls_pinv_factor is a no-op on a plan that holds its factor) and its sweeps;
  * one rls_pinv_solve at K = 1 and K = 64 on the factor (hipEvents around the call, one warm-up, median of REPS);
  * 16 solves with 16 different lambda -- on the one factor, and by DirectSolver, which factors 16 times;
  * DirectSolver's solve on its factor;
  * the host route: download A, numpy.linalg.svd in the element type, the formula, upload (wall clock).

Every step runs under a time limit of its own (SIGALRM with its default action: the process ends there, a hung device call
included), sized from the cost estimate of one round -- W and V moved once each way, about 200 MB at 4096 x 2048 ComplexF32 --
times N - 1 rounds times at most 40 sweeps, at a pessimistic 500 GB/s.  Lines are written as they are measured.
Times of different machines of one pool differ by up to 15 %: compare the legs of one run.   usage: bench_pinv.py [out.txt]
       bench_pinv.py --block b:tol_exp:cap[,b:tol_exp:cap...] [out.txt]   the blocked sweeps against the plain ones (block_ab below)"""
import os
import signal
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # noqa: F401
import rls_amd as rls
from bench import make_A

REPS, LAM = 9, 1e-2
LAMS = [float(l) for l in np.logspace(-4, 0, 16)]
ctx = rls.Context(0)
lib, h = ctx.lib, ctx.handle
out_path = sys.argv[1] if len(sys.argv) > 1 and sys.argv[1] != "--block" else None
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").close()


def say(s):
    print(s, flush=True)
    if out_path:
        with open(out_path, "a") as f:
            f.write(s + "\n")


class limit:
    """with limit(seconds): the process is killed when the step takes longer"""

    def __init__(self, seconds):
        self.seconds = max(1, int(np.ceil(seconds)))

    def __enter__(self):
        signal.signal(signal.SIGALRM, signal.SIG_DFL)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)


def timed(fn):
    ctx.sync()
    ctx.timer_start()
    fn()
    return ctx.timer_stop_ms()


def median_ms(fn, reps=REPS):
    timed(fn)
    t = [timed(fn) for _ in range(reps)]
    return float(np.median(t)), min(t), max(t)


def wall_ms(fn, reps):
    t = []
    for _ in range(reps):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), min(t), max(t)


def rel(a, b):
    return float(np.linalg.norm(a.astype(np.complex128) - b) / np.linalg.norm(b))


def block_ab(settings):
    """--block: the blocked sweeps against the plain ones, alternately in this process, median of 5 factorisations
    each, at 4096 x 2048 ComplexF32 and 1024 x 512 Float32.  A setting is b:tol_exp:cap (tau_b = 10^-tol_exp).  The time of
    phase 2 is the plain sweeps times the plain run's time per sweep, and phase 1 is the rest: the library times neither."""
    for M, N, dt in ((4096, 2048, np.complex64), (2048, 1024, np.complex64), (1024, 512, np.float32)):
        name = f"{M} x {N} {np.dtype(dt).name}"
        es = np.dtype(dt).itemsize
        factor_limit = max(20.0, 2 * (M + N) * N * es * (N - 1) * 40 / 500e9 + 40 * (N - 1) * 20e-6)
        A = make_A(M, N, 4, dt)
        rng = np.random.default_rng(5)
        x0 = rng.standard_normal(N) + (1j * rng.standard_normal(N) if np.dtype(dt).kind == "c" else 0)
        A64 = A.astype(np.complex128 if np.dtype(dt).kind == "c" else np.float64)
        b = (A64 @ x0).astype(dt)
        truth = np.linalg.solve(A64.conj().T @ A64 + LAM * np.eye(N), A64.conj().T @ b.astype(A64.dtype))
        Ad, bd = rls.DeviceMatrix.from_host(A, ctx), rls.DeviceVector.from_host(b, ctx)

        def one(block, tol, cap):
            ctx.tune(pinv_block=block, pinv_block_tol=tol, pinv_block_cap=cap)
            solver = rls.PseudoInverse(Ad, reg=[rls.L2Regularization(LAM)])
            ctx.sync()
            t0 = time.perf_counter()
            solver._the_plan().factor()
            ctx.sync()
            ms = (time.perf_counter() - t0) * 1e3
            st, bs = solver._plan.status(), solver._plan.block_status()
            return ms, st.sweeps, bs.block_sweeps, rel(rls.solve_(solver, bd).to_host(), truth)

        say(f"{name}: b tau_b cap | blocked sweeps, plain sweeps | total ms (median of 5; min, max) = phase 1 + phase 2 | error vs float64 || "
            f"plain alone: sweeps, ms, error | blocked / plain")
        with limit(2 * factor_limit):
            one(0, 0, 0)
        for b_, tol, cap in settings:
            with limit(12 * factor_limit):
                one(b_, tol, cap)                      # warm-up (the scratch, the kernels' first launch)
                tb, tp = [], []
                for _ in range(5):
                    tp.append(one(0, 0, 0))
                    tb.append(one(b_, tol, cap))
            mb_, mp = float(np.median([t[0] for t in tb])), float(np.median([t[0] for t in tp]))
            per_sweep = mp / tp[0][1]
            p2 = tb[0][1] * per_sweep
            say(f"{name}: {b_:2d} 1e-{tol} {cap:2d} | {tb[0][2]:2d}, {tb[0][1]:2d} | {mb_:8.2f} ({min(t[0] for t in tb):.2f}, {max(t[0] for t in tb):.2f}) "
                f"= {mb_ - p2:7.2f} + {p2:7.2f} | {tb[0][3]:.2e} || {tp[0][1]:2d}, {mp:8.2f}, {tp[0][3]:.2e} | {mb_ / mp:.3f}")
        ctx.tune(pinv_block=-1, pinv_block_tol=0, pinv_block_cap=0)


if "--block" in sys.argv:
    i = sys.argv.index("--block")
    spec = sys.argv[i + 1]
    out_path = sys.argv[i + 2] if len(sys.argv) > i + 2 else None
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        open(out_path, "a").close()
    block_ab([tuple(int(v) for v in s.split(":")) for s in spec.split(",")])
    sys.exit(0)

for M, N, dt in ((4096, 2048, np.complex64), (256, 128, np.float32)):
    name = f"{M} x {N} {np.dtype(dt).name}"
    es = np.dtype(dt).itemsize
    # one factorisation at the sweep cap: (W + V) read and written per round, N - 1 rounds, 40 sweeps, 500 GB/s; at least 20 s
    factor_limit = max(20.0, 2 * (M + N) * N * es * (N - 1) * 40 / 500e9 + 40 * (N - 1) * 20e-6)
    A = make_A(M, N, 4, dt)
    rng = np.random.default_rng(5)
    X = rng.standard_normal((N, 64)) + (1j * rng.standard_normal((N, 64)) if np.dtype(dt).kind == "c" else 0)
    A64 = A.astype(np.complex128 if np.dtype(dt).kind == "c" else np.float64)
    B = np.asfortranarray((A64 @ X).astype(dt))
    truth = np.linalg.solve(A64.conj().T @ A64 + LAM * np.eye(N), A64.conj().T @ B[:, 0].astype(A64.dtype))
    Ad, Bd, bd = rls.DeviceMatrix.from_host(A, ctx), rls.DeviceMatrix.from_host(B, ctx), rls.DeviceVector.from_host(B[:, 0].copy(), ctx)
    Xd = rls.DeviceMatrix(N, 64, dt, ctx)

    # ---- the factorisation ---------------------------------------------------------------------------------------------
    solver = rls.PseudoInverse(Ad, reg=[rls.L2Regularization(LAM)])
    with limit(factor_limit):
        t0 = time.perf_counter()
        x = rls.solve_(solver, bd)
        first = (time.perf_counter() - t0) * 1e3
    st = solver._plan.status()
    e_pinv = rel(x.to_host(), truth)
    say(f"{name}: PseudoInverse  error vs float64 {e_pinv:.2e};  {st.sweeps} sweeps of {N - 1 + (N & 1)} launches, one read-back per sweep; "
        f"2 launches per solved column")
    say(f"{name}:   first solve_ (factorisation included, wall clock) {first:9.1f} ms")
    f_reps = 3 if M * N > 1 << 20 else REPS
    plans = []

    def factor():
        plans.append(rls.solvers._PinvPlan(solver._op))
        plans[-1].factor()
        del plans[:-1]

    with limit((f_reps + 1) * factor_limit):
        f_ms = wall_ms(factor, f_reps)
    say(f"{name}:   factorisation alone      {f_ms[0]:9.3f} ms (min {f_ms[1]:.3f}, max {f_ms[2]:.3f}; wall clock, {f_reps} fresh plans)  "
        f"= {f_ms[0] / max(st.sweeps, 1):.3f} ms per sweep, {1e3 * f_ms[0] / max(st.sweeps, 1) / (N - 1 + (N & 1)):.2f} us per round")
    del plans[:]

    # ---- solves on the factor ------------------------------------------------------------------------------------------
    plan = solver._plan.handle

    def psolve(K, lam=LAM):
        rls._lib.check(h, lib.rls_pinv_solve(plan, float(lam), K, Bd.ptr, Bd.lda, Xd.ptr, Xd.lda, 0), "rls_pinv_solve")

    with limit(30):
        s1 = median_ms(lambda: psolve(1))
        s64 = median_ms(lambda: psolve(64))
        assert Xd.column(0).to_host().tobytes() == x.to_host().tobytes()
        sweep16 = median_ms(lambda: [psolve(1, l) for l in LAMS])
        whole = median_ms(lambda: rls.solve_(solver, bd))
    say(f"{name}:   solve on the factor K=1  {s1[0]:9.3f} ms (min {s1[1]:.3f}, max {s1[2]:.3f})")
    say(f"{name}:   solve on the factor K=64 {s64[0]:9.3f} ms (min {s64[1]:.3f}, max {s64[2]:.3f}) = {s64[0] / 64:.4f} ms per column")
    say(f"{name}:   16 solves, 16 lambdas    {sweep16[0]:9.3f} ms (min {sweep16[1]:.3f}, max {sweep16[2]:.3f}); factorisations so far: "
        f"{solver._plan.status().factorizations}")
    say(f"{name}:   solve_(solver, b) (init!, solve, status) {whole[0]:9.3f} ms")

    # ---- DirectSolver doing the same -------------------------------------------------------------------------------------
    direct = rls.DirectSolver(Ad, AHA=Ad.gram(), reg=[rls.L2Regularization(LAM)])
    with limit(30):
        xd = rls.solve_(direct, bd)
        dplan = direct._plan.handle

        def dsolve(lam):
            rls._lib.check(h, lib.rls_direct_factor(dplan, float(lam)), "rls_direct_factor")
            rls._lib.check(h, lib.rls_direct_solve(dplan, 1, Bd.ptr, Bd.lda, Xd.ptr, Xd.lda, 0), "rls_direct_solve")

        d16 = median_ms(lambda: [dsolve(l) for l in LAMS])
        dsolve(LAM)
        assert direct._plan.status().info == 0
        d1 = median_ms(lambda: rls._lib.check(h, lib.rls_direct_solve(dplan, 1, Bd.ptr, Bd.lda, Xd.ptr, Xd.lda, 0), "rls_direct_solve"))
    say(f"{name}: DirectSolver   error vs float64 {rel(xd.to_host(), truth):.2e}")
    say(f"{name}:   16 solves, 16 lambdas    {d16[0]:9.3f} ms (min {d16[1]:.3f}, max {d16[2]:.3f}): 16 factorisations")
    say(f"{name}:   solve on the factor K=1  {d1[0]:9.3f} ms (min {d1[1]:.3f}, max {d1[2]:.3f})")

    # ---- the host route ----------------------------------------------------------------------------------------------------
    def host_route():
        Ah = Ad.to_host()
        U, s, Vh = np.linalg.svd(Ah, full_matrices=False)
        xh = Vh.conj().T @ ((s / (s * s + s.dtype.type(LAM))).astype(s.dtype) * (U.conj().T @ bd.to_host()))
        return rls.DeviceVector.from_host(xh.astype(dt), ctx)

    with limit(300):
        xh = host_route()
        h_ms = wall_ms(host_route, 2 if M * N > 1 << 20 else REPS)
    say(f"{name}: host route (download A, numpy.linalg.svd, the formula, upload) {h_ms[0]:9.3f} ms (min {h_ms[1]:.3f}, max {h_ms[2]:.3f}); "
        f"error vs float64 {rel(xh.to_host(), truth):.2e}")
    say(f"{name}: one new lambda: PseudoInverse {s1[0]:.3f} ms  |  DirectSolver {d16[0] / 16:.3f} ms  |  host (a new SVD) {h_ms[0]:.3f} ms;  "
        f"paid once per A: PseudoInverse {f_ms[0]:.1f} ms")
