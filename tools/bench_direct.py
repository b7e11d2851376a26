"""DirectSolver (csrc/direct.hip) beside what a user had before it, in one process, at 4096 x 2048 ComplexF32 and 256 x 128 Float32
(lambda = 1e-2):

  * the factorisation alone (rls_direct_factor; lambda alternates between two values so that every call factors) and one
    rls_direct_solve at K = 1 and K = 64 on the factor: hipEvents around the call, one warm-up, median of REPS;
  * Gram-mode CGNR (AHA = A.gram()) run until it reaches the direct solution's error against the float64 solution: the
    iterations needed (error per iteration from ONE solve with a callback) and the time of a solve of that many iterations;
  * the host route: download G and A'b, numpy.linalg.solve in the element type, upload (wall clock, it ends in a synchronising copy).

Times of different machines of one pool differ by up to 15 %: compare the legs of one run.   usage: bench_direct.py [out.txt]"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # noqa: F401
import rls_amd as rls
from bench import make_A

REPS, LAM = 9, 1e-2
ctx = rls.Context(0)
lib, h = ctx.lib, ctx.handle
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn):
    ctx.sync()
    ctx.timer_start()
    fn()
    return ctx.timer_stop_ms()


def median_ms(fn):
    timed(fn)
    t = [timed(fn) for _ in range(REPS)]
    return float(np.median(t)), min(t), max(t)


def rel(a, b):
    return float(np.linalg.norm(a.astype(np.complex128) - b) / np.linalg.norm(b))


for M, N, dt in ((4096, 2048, np.complex64), (256, 128, np.float32)):
    name = f"{M} x {N} {np.dtype(dt).name}"
    A = make_A(M, N, 4, dt)
    rng = np.random.default_rng(5)
    X = rng.standard_normal((N, 64)) + (1j * rng.standard_normal((N, 64)) if np.dtype(dt).kind == "c" else 0)
    B = np.asfortranarray((A.astype(np.complex128) @ X).astype(dt))
    A64 = A.astype(np.complex128 if np.dtype(dt).kind == "c" else np.float64)
    truth = np.linalg.solve(A64.conj().T @ A64 + LAM * np.eye(N), A64.conj().T @ B[:, 0].astype(A64.dtype))
    Ad, Bd, bd = rls.DeviceMatrix.from_host(A, ctx), rls.DeviceMatrix.from_host(B, ctx), rls.DeviceVector.from_host(B[:, 0].copy(), ctx)
    Gd = Ad.gram()
    nb = (N + 63) // 64

    # ---- the direct solver -------------------------------------------------------------------------------------------
    solver = rls.DirectSolver(Ad, AHA=Gd, reg=[rls.L2Regularization(LAM)])
    x = rls.solve_(solver, bd)
    e_direct = rel(x.to_host(), truth)
    plan = solver._plan.handle
    flip = [0]

    def factor():
        flip[0] ^= 1
        rls._lib.check(h, lib.rls_direct_factor(plan, float(LAM * (1 + flip[0]))), "rls_direct_factor")

    f_ms = median_ms(factor)
    rls._lib.check(h, lib.rls_direct_factor(plan, float(LAM)), "rls_direct_factor")
    Xd = rls.DeviceMatrix(N, 64, dt, ctx)
    s1 = median_ms(lambda: rls._lib.check(h, lib.rls_direct_solve(plan, 1, Bd.ptr, Bd.lda, Xd.ptr, Xd.lda, 0), "rls_direct_solve"))
    s64 = median_ms(lambda: rls._lib.check(h, lib.rls_direct_solve(plan, 64, Bd.ptr, Bd.lda, Xd.ptr, Xd.lda, 0), "rls_direct_solve"))
    assert solver._plan.status().info == 0 and Xd.column(0).to_host().tobytes() == x.to_host().tobytes()
    whole = median_ms(lambda: rls.solve_(solver, bd))
    say(f"{name}: DirectSolver   error vs float64 {e_direct:.2e};  launches: {2 * nb} per factorisation, K + {2 * nb} per solve")
    say(f"{name}:   factorisation alone      {f_ms[0]:9.3f} ms (min {f_ms[1]:.3f}, max {f_ms[2]:.3f})")
    say(f"{name}:   solve on the factor K=1  {s1[0]:9.3f} ms (min {s1[1]:.3f}, max {s1[2]:.3f})")
    say(f"{name}:   solve on the factor K=64 {s64[0]:9.3f} ms (min {s64[1]:.3f}, max {s64[2]:.3f}) = {s64[0] / 64:.4f} ms per column")
    say(f"{name}:   solve_(solver, b), same lambda (init!, solve, status read-back) {whole[0]:9.3f} ms")

    # ---- Gram-mode CGNR to the same error ------------------------------------------------------------------------------
    cap = min(N, 400)
    cmp = rls.CompareSolutionCallback(truth)
    rls.solve_(rls.CGNR(Ad, AHA=Gd, reg=[rls.L2Regularization(LAM)], iterations=cap, relTol=0.0), bd, callbacks=cmp)
    errs = cmp.results
    need = next((i for i, e in enumerate(errs) if e <= e_direct), None)
    best = int(np.argmin(errs))
    its = need if need is not None else best
    cg = rls.CGNR(Ad, AHA=Gd, reg=[rls.L2Regularization(LAM)], iterations=max(its, 1), relTol=0.0)
    c_ms = median_ms(lambda: rls.solve_(cg, bd))
    reached = f"reaches it after {need} iterations" if need is not None else \
        f"does not reach it within {cap} iterations (best {errs[best]:.2e} after {best}: timed at {best})"
    say(f"{name}: Gram-mode CGNR {reached}: {c_ms[0]:9.3f} ms per solve (min {c_ms[1]:.3f}, max {c_ms[2]:.3f})")

    # ---- the host route --------------------------------------------------------------------------------------------------
    rhs_d = rls.DeviceVector(N, dt, ctx)

    def host_route():
        Ad.mul_adj_(rhs_d, bd)
        G = Gd.to_host()
        xh = np.linalg.solve(G + (LAM * np.eye(N)).astype(dt), rhs_d.to_host())
        return rls.DeviceVector.from_host(xh, ctx)

    host_route()
    t = []
    for _ in range(REPS):
        ctx.sync()
        t0 = time.perf_counter()
        xh = host_route()
        ctx.sync()
        t.append((time.perf_counter() - t0) * 1e3)
    say(f"{name}: host route (download G, numpy.linalg.solve, upload) {float(np.median(t)):9.3f} ms (min {min(t):.3f}, max {max(t):.3f}); "
        f"error vs float64 {rel(xh.to_host(), truth):.2e}")
    say(f"{name}: repeated solve, new b: DirectSolver {s1[0]:.3f} ms  |  CGNR {c_ms[0]:.3f} ms  |  host {float(np.median(t)):.3f} ms")

if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
