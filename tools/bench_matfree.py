"""The matrix-free operators (csrc/fft.hip) in one process, ComplexF32 at 16 x 16 ... 1024 x 1024:

  * FFTOp forward and the normal operator of ProdOp(SamplingOp, FFTOp) (a third of the samples): the single-workgroup path against
    the general one (rls_tune_set("fft_fused", 2) against 0) wherever the image fits a workgroup's LDS;
  * the same two products through a dense DeviceMatrix of the sampled DFT at 64 x 64 (1365 x 4096: the only route without these
    operators; the full 4096 x 4096 DFT is 128 MiB);
  * torch.fft.fft2 on the same device, where it runs;
  * the reference's compressed-sensing example end to end: 256 x 256 Float32, a third of the pixels, FISTA + TV, 20 iterations.

Each figure is the median of REPS timings of ITERS back-to-back calls between two events on the context's stream (launch overhead
included, no host wait in between), after one warm-up.  Times of different machines of one pool differ by up to 15 %: compare the
legs of one run.   usage: bench_matfree.py [out.txt]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import rls_amd as rls

REPS, ITERS = 9, 20
ctx = rls.Context(0)
out_path = sys.argv[1] if len(sys.argv) > 1 else None
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").close()


def say(s):
    print(s, flush=True)
    if out_path:
        with open(out_path, "a") as f:
            f.write(s + "\n")


def med_us(fn, iters=ITERS):
    """microseconds per call"""
    fn()
    ts = []
    for _ in range(REPS):
        ctx.sync()
        ctx.timer_start()
        for _ in range(iters):
            fn()
        ts.append(ctx.timer_stop_ms() * 1e3 / iters)
    return float(np.median(ts))


def vec(rng, n):
    return rls.DeviceVector.from_host((rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64), ctx)


def dft1(n):
    """the shifted unitary 1-D DFT as a matrix"""
    eye = np.eye(n)
    return np.fft.fftshift(np.fft.fft(np.fft.ifftshift(eye, axes=0), axis=0), axes=0) / np.sqrt(n)


say(f"# bench_matfree: ComplexF32, median of {REPS} x {ITERS} calls, microseconds per call; device {torch.cuda.get_device_name(0)}")
say("# shape        op       single-workgroup   general   torch.fft.fft2   dense DeviceMatrix")
rng = np.random.default_rng(0)
for n1 in (16, 32, 64, 128, 256, 1024):   # (16 and 32: where the single-workgroup path is expected to pay)
    shape, n = (n1, n1), n1 * n1
    pat = np.sort(rng.choice(n, n // 3, replace=False)).astype(np.int32)
    F = rls.FFTOp(np.complex64, shape, ctx=ctx)
    P = rls.ProdOp(rls.SamplingOp(np.complex64, pat, shape, ctx), F)
    x, y, v = vec(rng, n), rls.DeviceVector(n, np.complex64, ctx), rls.DeviceVector(n, np.complex64, ctx)
    ctx.tune(fft_fused=2)   # (2: the single-workgroup path for every image that fits, not only the small ones of the default)
    fits = F.variant() == 1
    row = {}
    for name, fn in (("forward", lambda: F.mul_(y, x)), ("normal", lambda: P.mul_normal_(v, x))):
        ctx.tune(fft_fused=2)
        one = med_us(fn) if fits else None
        ctx.tune(fft_fused=0)
        row[name] = (one, med_us(fn))
    ctx.tune(fft_fused=1)
    try:
        tx = torch.randn(n1, n1, dtype=torch.complex64, device="cuda")
        torch.fft.fft2(tx)
        torch.cuda.synchronize()
        ts = []
        for _ in range(REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(ITERS):
                torch.fft.fft2(tx)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3 / ITERS)
        t_torch = f"{np.median(ts):9.1f}"
    except Exception as e:  # noqa: BLE001  (reported, not hidden)
        t_torch = f"did not run ({type(e).__name__})"
    dense = {"forward": "-", "normal": "-"}
    if n1 == 64:
        D = np.kron(dft1(n1), dft1(n1))[pat].astype(np.complex64)   # column-major image: F2 = F_dim2 (x) F_dim1
        A = rls.DeviceMatrix.from_host(D, ctx)
        ym = rls.DeviceVector(pat.size, np.complex64, ctx)
        NA = A.normal_operator()
        dense = {"forward": f"{med_us(lambda: A.mul_(ym, x)):9.1f}", "normal": f"{med_us(lambda: NA.mul_(v, x)):9.1f}"}
    for name in ("forward", "normal"):
        one, gen = row[name]
        say(f"{n1:5d}x{n1:<5d} {name:8s} {('%9.1f' % one) if one is not None else '   (no fit)':>16s} {gen:9.1f}   "
            f"{t_torch if name == 'forward' else '-':>14s}   {dense[name]:>12s}")

# the reference example end to end (wall clock, solver construction with its power iterations included)
shape, n = (256, 256), 65536
pat = np.sort(rng.choice(n, n // 3, replace=False)).astype(np.int32)
yy, xx = np.mgrid[-1:1:256j, -1:1:256j]
img = (xx ** 2 + (yy / 1.3) ** 2 < 0.6).astype(np.float32)
A = rls.SamplingOp(np.float32, pat, shape, ctx)
b = rls.DeviceVector.from_host(img.ravel(order="F")[pat], ctx)
ts = []
for _ in range(6):
    ctx.sync()
    t0 = time.perf_counter()
    S = rls.createLinearSolver(rls.FISTA, A, reg=rls.TVRegularization(0.01, shape=shape), iterations=20)
    xs = rls.solve_(S, b)
    ctx.sync()
    ts.append((time.perf_counter() - t0) * 1e3)
say(f"# compressed-sensing example, 256x256 Float32, m = n/3, FISTA + TV, 20 iterations (primitive loop, default rho): "
    f"{np.median(ts[1:]):.2f} ms per createLinearSolver + solve (median of 5, first run {ts[0]:.2f} ms)")
