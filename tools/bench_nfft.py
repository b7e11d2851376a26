"""NFFTOp (csrc/nfft.hip) in one process, ComplexF32, m = 4, a radial trajectory of N_1 spokes with N_1 samples each (J = N_1 N_2) at
64 x 64, 128 x 128 and 256 x 256:

  * microseconds per forward, adjoint and normal call;
  * at 64 x 64 the same three products through a dense DeviceMatrix of the operator (A.to_dense(): 4096 x 4096 ComplexF32, 128 MiB),
    with the time to_dense() takes;
  * on the CPU, from tests/nfft_ref.py: the truncation error of the restatement in complex128 against the dense non-uniform DFT for
    every (shape, m) the tests run, relative to ||x||_1, next to the published bound.

Each time is the median of REPS timings of ITERS back-to-back calls between two events on the context's stream (launch overhead
included, no host wait in between), after one warm-up.  Times of different machines of one pool differ by up to 15 %: compare the
legs of one run.   usage: bench_nfft.py [out.txt]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import rls_amd as rls
import nfft_ref as NR

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


def radial(n):
    """n spokes over [0, pi), n samples each on [-0.5, 0.5): 2 x n^2"""
    r = np.arange(n) / n - 0.5
    th = np.pi * np.arange(n) / n
    return np.stack([np.outer(np.cos(th), r).ravel(), np.outer(np.sin(th), r).ravel()])


dt = np.complex64
say(f"# bench_nfft: ComplexF32, m = 4, median of {REPS} x {ITERS} calls, microseconds per call; device {torch.cuda.get_device_name(0)}")
say("# NFFTOp on a radial trajectory (J = N_1 N_2): forward (embed, FFT, gather) | adjoint (spread, FFT^H, crop) | normal (the two chains)")
rng = np.random.default_rng(0)
for n1 in (64, 128, 256):
    shape, N = (n1, n1), n1 * n1
    nodes = radial(n1)
    t0 = time.perf_counter()
    A = rls.NFFTOp(dt, nodes, shape, m=4, ctx=ctx)
    create = time.perf_counter() - t0
    x = rls.DeviceVector.from_host(NR.gauss(N, 1).astype(dt), ctx)
    y = rls.DeviceVector.from_host(NR.gauss(A.M, 2).astype(dt), ctx)
    yo, xo = rls.DeviceVector(A.M, dt, ctx), rls.DeviceVector(N, dt, ctx)
    fwd, adj, nrm = med_us(lambda: A.mul_(yo, x)), med_us(lambda: A.mul_adj_(xo, y)), med_us(lambda: A.mul_normal_(xo, x))
    say(f"{n1:4d}x{n1:<4d} J = {A.M:6d}  grid {A.grid_points:7d} points  NFFTOp  forward {fwd:8.1f} | adjoint {adj:8.1f} | normal {nrm:8.1f} "
        f"| create {create * 1e3:.1f} ms")
    if n1 == 64:
        t0 = time.perf_counter()
        Dm = A.to_dense()
        ctx.sync()
        build = time.perf_counter() - t0
        NO = Dm.normal_operator()
        df, da, dn = med_us(lambda: Dm.mul_(yo, x)), med_us(lambda: Dm.mul_adj_(xo, y)), med_us(lambda: NO.mul_(xo, x))
        ref = Dm.mul_(rls.DeviceVector(A.M, dt, ctx), x).to_host()
        got = A.mul_(rls.DeviceVector(A.M, dt, ctx), x).to_host()
        say(f"{'':9s} J = {A.M:6d}  {'':20s}  dense   forward {df:8.1f} | adjoint {da:8.1f} | normal {dn:8.1f} | {A.M * N * 8} bytes  "
            f"to_dense {build:.2f} s  (the two forwards differ by {np.linalg.norm(got - ref) / np.linalg.norm(ref):.1e} relative)")
        del Dm, NO

say("# truncation error of the restatement in complex128 against the dense non-uniform DFT, worst over the tests' node sets, forward and")
say("# adjoint and matrix entries, relative to ||x||_1; the bound is Potts & Steidl's Kaiser-Bessel estimate at sigma = 2 times d")
for shape in NR.SHAPES:
    for m in NR.ms_of(np.complex128):
        worst = 0.0
        for name, nd in NR.node_sets(shape, m):
            E, P = NR.exact(nd, shape), NR.restated(nd, shape, m)
            xs, ys = NR.gauss(P.size, 5), NR.gauss(P.J, 6)
            worst = max(worst, np.abs(P.forward(xs) - E @ xs).max() / np.abs(xs).sum(),
                        np.abs(P.adjoint(ys) - E.conj().T @ ys).max() / np.abs(ys).sum(), np.abs(P.dense() - E).max())
        bound = NR.truncation(m, len(NR.extents(shape)))
        say(f"truncation {'x'.join(map(str, shape)):>6s}  m = {m}  measured {worst:.3e}  bound {bound:.3e}  {'met' if worst <= bound else 'NOT MET'}")
