"""WaveletOp (csrc/wavelet.hip) in one process, hipEvents around K back-to-back calls on the context's stream, one warm-up round, median of
REPS rounds, reported per call:

  * rls_wavelet_apply (forward) and rls_prox_wavelet_l1 (db2, full depth) at 64 x 64, 128 x 128, 256 x 256 and 1024 x 1024, Float32
    and ComplexF32, on the single-workgroup path and on the general path (wavelet_fused = 0) wherever the image fits the former;
  * the same prox through a dense DeviceMatrix trafo (two GEMVs over the 4096 x 4096 matrix and rls_prox_l1) at 64 x 64;
  * FISTA + wavelet-L1 at 4096 x 4096 Float32 (a 64 x 64 image), 50 iterations, solve_ end to end (wall clock around the call, which
    ends in a status read-back): the device plan against the primitive loop (use_device_plan = False);
  * VGPRs / LDS / scratch of the new kernels, from the code objects inside the shipped library.

There is no parent to compare with (the parent commit has no wavelet operator): the basis is the primitive / dense routes of this run.
Times of different machines of one pool differ by up to 15 %: compare the legs of one run.   usage: bench_wavelet.py [out.txt]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch  # noqa: F401
import rls_amd as rls

REPS, K = 9, 50
ctx = rls.Context(0)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def per_call_us(fn, k=K):
    def round_():
        ctx.sync()
        ctx.timer_start()
        for _ in range(k):
            fn()
        return ctx.timer_stop_ms() * 1e3 / k
    round_()
    t = [round_() for _ in range(REPS)]
    return float(np.median(t)), min(t), max(t)


def fmt(t):
    return f"{t[0]:9.1f} us  (min {t[1]:.1f}, max {t[2]:.1f})"


say(f"# tools/bench_wavelet.py: median of {REPS} rounds of {K} back-to-back calls, hipEvents, per call; db2, full depth")
say("")
say("## rls_wavelet_apply (forward) and rls_prox_wavelet_l1")
for n in (64, 128, 256, 1024):
    for dt in (np.float32, np.complex64):
        rng = np.random.default_rng(n)
        x = rng.standard_normal(n * n) + (1j * rng.standard_normal(n * n) if np.dtype(dt).kind == "c" else 0)
        xd = rls.DeviceVector.from_host(x.astype(dt), ctx)
        yd = rls.DeviceVector(n * n, dt, ctx)
        op = rls.WaveletOp((n, n))
        fits = 2 * n * n * np.dtype(dt).itemsize <= 160 * 1024 - 512
        for fused in ((1, 0) if fits else (0,)):
            ctx.tune(wavelet_fused=fused)
            path = "single workgroup" if fused else "general (%d launches)" % (2 * op.levels)
            ta = per_call_us(lambda: op.mul_(yd, xd))
            tp = per_call_us(lambda: op.prox_l1_(yd, 0.1))
            say(f"{n:5d} x {n:<5d} {np.dtype(dt).name:10s} {path:24s} apply {fmt(ta)}   prox {fmt(tp)}")
        ctx.tune(wavelet_fused=1)
say("")
say("## the same prox through a dense DeviceMatrix trafo (the only route before), 64 x 64")
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import wavelet_ref  # noqa: E402  (the float64 matrix the tests compare against)

W = wavelet_ref.dense((64, 64), "db2")
for dt in (np.float32, np.complex64):
    Wd = rls.DeviceMatrix.from_host(np.asfortranarray(W.astype(dt)), ctx)
    x = np.random.default_rng(1).standard_normal(4096).astype(dt)
    xd = rls.DeviceVector.from_host(x, ctx)
    reg_d = rls.TransformedRegularization(rls.L1Regularization(0.1), Wd)
    reg_w = rls.TransformedRegularization(rls.L1Regularization(0.1), rls.WaveletOp((64, 64)))
    td = per_call_us(lambda: rls.prox_(reg_d, xd), k=10)
    tw = per_call_us(lambda: rls.prox_(reg_w, xd))
    say(f"   64 x 64    {np.dtype(dt).name:10s} dense trafo {fmt(td)}   WaveletOp {fmt(tw)}   ratio {td[0] / tw[0]:.1f}")
say("")
say("## FISTA + wavelet-L1, 4096 x 4096 Float32 (64 x 64 image), 50 iterations, solve_ end to end (wall clock)")
rng = np.random.default_rng(3)
A = np.asfortranarray((rng.standard_normal((4096, 4096)) / 64).astype(np.float32))
b = (A @ rng.standard_normal(4096).astype(np.float32)).astype(np.float32)
Ad, bd = rls.DeviceMatrix.from_host(A, ctx), rls.DeviceVector.from_host(b, ctx)
rho = 0.95 / np.linalg.norm(A.astype(np.float64), 2) ** 2
res = {}
for plan in (True, False):
    sol = rls.createLinearSolver(rls.FISTA, Ad, reg=rls.TransformedRegularization(rls.L1Regularization(0.05), rls.WaveletOp((64, 64))),
                                 rho=rho, iterations=50, relTol=0.0)
    sol.use_device_plan = plan
    t = []
    for _ in range(REPS + 1):
        ctx.sync()
        t0 = time.perf_counter()
        x = rls.solve_(sol, bd)
        ctx.sync()
        t.append((time.perf_counter() - t0) * 1e3)
    assert bool(sol.state._plan) == plan and sol.state.iteration == 50
    res[plan] = (float(np.median(t[1:])), x.to_host())
    say(f"   {'device plan   ' if plan else 'primitive loop'}  {res[plan][0]:8.3f} ms per solve (min {min(t[1:]):.3f}, max {max(t[1:]):.3f})")
say(f"   plan / primitives: {res[False][0] / res[True][0]:.2f} x;  iterates differ by "
    f"{np.linalg.norm(res[True][1] - res[False][1]) / np.linalg.norm(res[False][1]):.1e} relative")
say("")
say("## kernel resources (gfx950 code objects of the shipped library)")
import kernel_metadata  # noqa: E402

ks = {k: v for k, v in kernel_metadata.kernels().items() if "wavelet" in k}
for fam in ("wavelet_fused_kernel", "wavelet_level_kernel"):
    sel = {k: v for k, v in ks.items() if k.startswith(fam)}
    say(f"   {fam}: {len(sel)} instantiations, VGPRs {min(v['vgprs'] for v in sel.values())}-{max(v['vgprs'] for v in sel.values())}, "
        f"SGPRs <= {max(v['sgprs'] for v in sel.values())}, static LDS {max(v['lds'] for v in sel.values())} B, "
        f"scratch {max(v['scratch'] for v in sel.values())} B")
say("   wavelet_fused_kernel: dynamic LDS 2 N sizeof(element) (32 KiB at 64 x 64 Float32, 128 KiB at 128 x 128 Float32), 256 threads up to "
    "2048 elements, 1024 beyond")
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    open(sys.argv[1], "w").write("\n".join(lines) + "\n")
