"""RadonOp (csrc/radon.hip) in one process, Float32, at 64 x 64 / 64 angles, 128 x 128 / 128 and 256 x 256 / 256 (angles in [0, pi),
the default detector count):

  * microseconds per forward, adjoint and normal call; the adjoint at every lanes-per-pixel instantiation
    (rls_tune_set("radon_lanes", L)) and under the automatic rule;
  * the same three products through a DeviceSparseMatrix holding the same matrix (built on the host from the operator's definition:
    about 2 non-zeros per pixel and angle, kept twice on the device), with its host build time and size;
  * the reference's computed-tomography example end to end: 256 x 256 Float32, 256 angles, CGNR + L2(0.001), 20 iterations.

Each figure is the median of REPS timings of ITERS back-to-back calls between two events on the context's stream (launch overhead
included, no host wait in between), after one warm-up.  Times of different machines of one pool differ by up to 15 %: compare the
legs of one run.   usage: bench_radon.py [out.txt]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import rls_amd as rls

REPS, ITERS = 9, 20
LANES = (1, 4, 16, 64)
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


def radon_csc(shape, angles, D):
    """the operator's matrix as (colptr, rowval, nzval Float32, (M, N)), from its definition: per pixel and angle the three bins around
    the pixel centre's projection, the non-zero ones kept (rows ascend inside a column: angle by angle, bin by bin)"""
    n1, n2 = shape
    nA, N = len(angles), n1 * n2
    xr = np.tile(np.arange(n1) - (n1 - 1) / 2, n2)
    yr = np.repeat(np.arange(n2) - (n2 - 1) / 2, n1)
    rows = np.empty((N, nA, 3), np.int32)
    vals = np.empty((N, nA, 3), np.float32)
    for q, th in enumerate(angles):
        c, s = np.cos(th), np.sin(th)
        if min(abs(c), abs(s)) <= 2.0 ** -40:
            c, s = (np.sign(c), 0.0) if abs(c) > abs(s) else (0.0, np.sign(s))
        mx, mn, hi = max(abs(c), abs(s)), min(abs(c), abs(s)), (abs(c) + abs(s)) / 2
        p = xr * c + yr * s
        k = np.rint(p + (D - 1) / 2).astype(np.int64)[:, None] + np.arange(-1, 2)[None, :]
        d = np.abs(k - (D - 1) / 2 - p[:, None])
        w = (np.where(d < hi, 1.0, np.where(d == hi, 0.5, 0.0)) if mn == 0 else np.clip((hi - d) / mn, 0.0, 1.0)) / mx
        w[(k < 0) | (k >= D)] = 0.0
        rows[:, q, :] = np.clip(k, 0, D - 1) + D * q
        vals[:, q, :] = w
    keep = vals > 0
    colptr = np.concatenate([[0], np.cumsum(keep.reshape(N, -1).sum(axis=1))]).astype(np.int64)
    return colptr, rows[keep], vals[keep], (D * nA, N)


say(f"# bench_radon: Float32, median of {REPS} x {ITERS} calls, microseconds per call; device {torch.cuda.get_device_name(0)}")
say("# RadonOp: forward | adjoint at L = 1, 4, 16, 64 lanes per pixel | automatic L: adjoint, normal (forward + adjoint, two launches)")
say("# DeviceSparseMatrix of the same matrix: forward, adjoint, normal (two products), non-zeros, device bytes (CSC + CSR), host build")
rng = np.random.default_rng(0)
for n1, nA in ((64, 64), (128, 128), (256, 256)):
    shape, n = (n1, n1), n1 * n1
    angles = np.linspace(0.0, np.pi, nA, endpoint=False)
    A = rls.RadonOp(np.float32, angles, shape, ctx=ctx)
    x = rls.DeviceVector.from_host(rng.standard_normal(n).astype(np.float32), ctx)
    y = rls.DeviceVector.from_host(rng.standard_normal(A.M).astype(np.float32), ctx)
    yo, xo = rls.DeviceVector(A.M, np.float32, ctx), rls.DeviceVector(n, np.float32, ctx)
    fwd = med_us(lambda: A.mul_(yo, x))
    adj = {}
    for L in LANES:
        ctx.tune(radon_lanes=L)
        adj[L] = med_us(lambda: A.mul_adj_(xo, y))
    ctx.tune(radon_lanes=0)
    auto = A.lanes()
    adj_auto, nrm = med_us(lambda: A.mul_adj_(xo, y)), med_us(lambda: A.mul_normal_(xo, x))
    say(f"{n1:4d}x{n1:<4d} {nA:4d} angles  D = {A.detectors:4d}  M = {A.M:6d}  RadonOp  forward {fwd:8.1f} | adjoint "
        + "  ".join(f"L={L}: {adj[L]:8.1f}" for L in LANES) + f" | automatic L = {auto}: adjoint {adj_auto:8.1f}  normal {nrm:8.1f}")
    try:
        t0 = time.perf_counter()
        csc = radon_csc(shape, angles, A.detectors)
        Sp = rls.DeviceSparseMatrix.from_host(csc, ctx)
        ctx.sync()
        build = time.perf_counter() - t0
        NS = Sp.normal_operator()
        sf, sa, sn = med_us(lambda: Sp.mul_(yo, x)), med_us(lambda: Sp.mul_adj_(xo, y)), med_us(lambda: NS.mul_(xo, x))
        # the two routes hold the same matrix: one product of each, compared on the scale of the result
        ref = Sp.mul_(rls.DeviceVector(A.M, np.float32, ctx), x).to_host()
        got = A.mul_(rls.DeviceVector(A.M, np.float32, ctx), x).to_host()
        dev = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
        say(f"{'':30s}  M = {A.M:6d}  sparse   forward {sf:8.1f} | adjoint {sa:8.1f} | normal {sn:8.1f} | nnz {Sp.nnz}  "
            f"{2 * Sp.nnz * 8 + (A.M + n + 2) * 8} bytes  host build {build:.2f} s  (RadonOp forward differs by {dev:.1e} relative)")
        del Sp, NS, csc
    except Exception as e:  # noqa: BLE001  (reported, not hidden)
        say(f"{'':30s}  sparse route did not run ({type(e).__name__}: {e})")

# the reference example end to end (wall clock, solver construction included)
shape = (256, 256)
yy, xx = np.mgrid[-1:1:256j, -1:1:256j]
img = ((xx ** 2 + (yy / 1.3) ** 2 < 0.6).astype(np.float32) + 0.5 * ((xx - 0.2) ** 2 + (yy + 0.1) ** 2 < 0.05)).astype(np.float32)
A = rls.RadonOp(np.float32, np.linspace(0.0, np.pi, 256, endpoint=False), shape, ctx=ctx)
b = A.mul_(rls.DeviceVector(A.M, np.float32, ctx), rls.DeviceVector.from_host(img.ravel(order="F"), ctx))
ts = []
for _ in range(6):
    ctx.sync()
    t0 = time.perf_counter()
    S = rls.createLinearSolver(rls.CGNR, A, reg=rls.L2Regularization(0.001), iterations=20)
    xs = rls.solve_(S, b)
    ctx.sync()
    ts.append((time.perf_counter() - t0) * 1e3)
r = A.mul_(rls.DeviceVector(A.M, np.float32, ctx), xs).to_host() - b.to_host()
say(f"# computed-tomography example, 256x256 Float32, 256 angles, CGNR + L2(0.001), 20 iterations (primitive loop): "
    f"{np.median(ts[1:]):.2f} ms per createLinearSolver + solve (median of 5, first run {ts[0]:.2f} ms); "
    f"{S.state.iteration} iterations, ||A x - b|| / ||b|| = {np.linalg.norm(r) / np.linalg.norm(b.to_host()):.3e}")
