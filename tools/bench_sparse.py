"""The sparse operator (csrc/sparse.hip) in one process, hipEvents around K back-to-back calls on the context's stream (K = 200 for the
products: a window of about a millisecond; K = 3 for the calls of ten sweeps, tens of milliseconds each), one warm-up round, median
of REPS rounds, reported per call.  Every timed leg is also COMPARED: the sparse product with the dense one, every forced
instantiation with the automatic one, the sparse sweeps with the dense sweeps (relative differences printed; the tool fails
above 1e-4 for a product and 1e-2 for ten sweeps, which accumulate Float32 rounding in different orders).

  * rls_sparse_mul, N and C, at 4096 x 2048 ComplexF32 and 8192 x 4096 Float32, densities 0.1 %, 1 %, 5 % and 25 %: every lanes
    instantiation forced in turn, the automatic choice, and the dense rls_gemv on to_dense() of the same matrix (the only route
    before).  Effective bandwidth on the algorithmic bytes: nnz (sizeof(elt) + 4) plus both vectors (dense: M N sizeof(elt) plus
    both vectors).  "auto" must be the best instantiation, or within the run-to-run spread of it: the thresholds of sp_pick_lanes
    come from this table.
  * the same product (N) on a tall 524288 x 1024 Float32 matrix with exactly 1, 2, 4, 8 and 16 non-zeros per row: far above the
    launch floor, so the short-row end of the lane rule is decided by bandwidth, not by noise (no dense leg: 2 GiB);
  * ten Kaczmarz sweeps, rls_sparse_kaczmarz_sweep against the dense rls_kaczmarz_sweep on to_dense(), the same matrices, one and
    16 right-hand sides: microseconds per row step (all columns advance together, one workgroup each).

There is no parent to compare with (the parent commit has no sparse operator): the basis is the dense route of this run.
Times of different machines of one pool differ by up to 15 %: compare the legs of one run.   usage: bench_sparse.py [out.txt]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # noqa: F401
import rls_amd as rls

REPS, K = 7, 200
LANES = (1, 4, 16, 64)
SHAPES = ((4096, 2048, np.complex64), (8192, 4096, np.float32))
DENSITIES = (0.001, 0.01, 0.05, 0.25)
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


def random_csc(M, N, density, dtype, seed):
    rng = np.random.default_rng(seed)
    mask = rng.random((N, M)) < density                  # (N x M: np.nonzero walks it column of A by column of A)
    cols, rows = np.nonzero(mask)
    nz = rng.standard_normal(rows.size)
    if np.dtype(dtype).kind == "c":
        nz = nz + 1j * rng.standard_normal(rows.size)
    colptr = np.zeros(N + 1, np.int64)
    np.cumsum(mask.sum(axis=1), out=colptr[1:])
    return colptr, rows.astype(np.int32), nz.astype(dtype), (M, N)


def rel(a, b):
    a, b = np.asarray(a, np.complex128), np.asarray(b, np.complex128)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def checked(what, err, bound):
    if not err <= bound:   # (NaN fails, too)
        raise SystemExit(f"{what}: relative difference {err:.3e} above {bound:.0e}")
    return err


def tall_csc(M, N, per_row, dtype, seed):
    """exactly per_row non-zeros in every row, at distinct columns"""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(M, dtype=np.int64), per_row)
    cols = (np.repeat(rng.integers(0, N, M), per_row) + 37 * np.tile(np.arange(per_row), M)) % N   # 37 and N = 1024 are coprime
    order = np.lexsort((rows, cols))
    colptr = np.zeros(N + 1, np.int64)
    np.cumsum(np.bincount(cols, minlength=N), out=colptr[1:])
    return colptr, rows[order].astype(np.int32), rng.standard_normal(rows.size).astype(dtype), (M, N)


def vec(n, dtype, seed):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(n) + (1j * rng.standard_normal(n) if np.dtype(dtype).kind == "c" else 0)
    return rls.DeviceVector.from_host(v.astype(dtype), ctx)


say(f"# tools/bench_sparse.py: median of {REPS} rounds of {K} back-to-back calls, hipEvents, per call")
mats = {}
say("")
say("## rls_sparse_mul: us per product (GB/s on the algorithmic bytes); lanes forced in turn, auto, dense rls_gemv on to_dense()")
for M, N, dt in SHAPES:
    es = np.dtype(dt).itemsize
    for d in DENSITIES:
        A = rls.DeviceSparseMatrix.from_host(random_csc(M, N, d, dt, int(d * 1e4) + M), ctx)
        D = A.to_dense()
        mats[(M, N, d)] = (A, D)
        xN, yM = vec(N, dt, 1), vec(M, dt, 2)
        outM, outN = rls.DeviceVector(M, dt, ctx), rls.DeviceVector(N, dt, ctx)
        for opname, op, x, y in (("N", 0, xN, outM), ("C", 2, yM, outN)):
            sbytes = A.nnz * (es + 4) + (M + N) * es
            dbytes = (M * N + M + N) * es
            row = []
            best = None
            ctx.tune(sparse_lanes=0)
            ta = per_call_us(lambda: A.spmv_(op, x, y))
            ya = y.to_host()
            err_l = 0.0
            for L in LANES:
                ctx.tune(sparse_lanes=L)
                t = per_call_us(lambda: A.spmv_(op, x, y))
                err_l = max(err_l, checked(f"L={L} against auto", rel(y.to_host(), ya), 1e-4))
                row.append(f"L={L}: {t[0]:7.1f}")
                best = (t, L) if best is None or t[0] < best[0][0] else best
            ctx.tune(sparse_lanes=0)
            td = per_call_us(lambda: D.gemv_(op, x, y))
            err_d = checked("sparse against dense product", rel(ya, y.to_host()), 1e-4)
            mean = A.nnz / (M if op == 0 else N)
            say(f"{M}x{N} {np.dtype(dt).name:9s} {100 * d:5.1f}% op {opname} nnz/row {mean:7.1f} | " + "  ".join(row) +
                f" | auto L={A.variant(op):2d}: {ta[0]:7.1f} (min {ta[1]:.1f}, max {ta[2]:.1f}) {sbytes / ta[0] / 1e3:7.1f} GB/s"
                f" | best L={best[1]:2d} (min {best[0][1]:.1f}, max {best[0][2]:.1f})"
                f" | dense {td[0]:7.1f} {dbytes / td[0] / 1e3:7.1f} GB/s | dense/sparse {td[0] / ta[0]:6.2f}x"
                f" | diff sparse-dense {err_d:.1e}, lanes-auto {err_l:.1e}")

say("")
say("## rls_sparse_mul (N) on a tall matrix, 524288 x 1024 float32, exactly k non-zeros per row: us per product, lanes forced in turn")
TM, TN = 524288, 1024
for per_row in (1, 2, 4, 8, 16):
    A = rls.DeviceSparseMatrix.from_host(tall_csc(TM, TN, per_row, np.float32, per_row), ctx)
    x, y = vec(TN, np.float32, 1), rls.DeviceVector(TM, np.float32, ctx)
    ctx.tune(sparse_lanes=0)
    ta = per_call_us(lambda: A.spmv_(0, x, y), k=50)
    ya = y.to_host()
    row, best, err_l = [], None, 0.0
    for L in LANES:
        ctx.tune(sparse_lanes=L)
        t = per_call_us(lambda: A.spmv_(0, x, y), k=50)
        err_l = max(err_l, checked(f"tall, L={L} against auto", rel(y.to_host(), ya), 1e-4))
        row.append(f"L={L}: {t[0]:7.1f} (min {t[1]:.1f}, max {t[2]:.1f})")
        best = (t, L) if best is None or t[0] < best[0][0] else best
    ctx.tune(sparse_lanes=0)
    sbytes = A.nnz * 8 + (TM + TN) * 4 + (TM + 1) * 8
    say(f"nnz/row {per_row:3d} | " + "  ".join(row) + f" | auto L={A.variant(0):2d}: {ta[0]:7.1f} (min {ta[1]:.1f}, max {ta[2]:.1f})"
        f" {sbytes / ta[0] / 1e3:7.1f} GB/s (with the row pointers) | best L={best[1]:2d} | diff lanes-auto {err_l:.1e}")
    del A

say("")
say("## ten Kaczmarz sweeps (L2, lambda = 0.01, natural order): ms per call and us per row step, sparse against dense on to_dense()")
for M, N, dt in SHAPES:
    for d in DENSITIES:
        A, D = mats[(M, N, d)]
        for nrhs in (1, 16):
            rng = np.random.default_rng(3)
            B = rng.standard_normal((M, nrhs)) + (1j * rng.standard_normal((M, nrhs)) if np.dtype(dt).kind == "c" else 0)
            b = (rls.DeviceVector.from_host(B[:, 0].astype(dt), ctx) if nrhs == 1
                 else rls.DeviceMatrix.from_host(np.asfortranarray(B.astype(dt)), ctx))
            res, sol = [], []
            for op in (A, D):
                S = rls.Kaczmarz(op, reg=rls.L2Regularization(0.01), iterations=10)
                S.init_(S.state, b)
                t = per_call_us(lambda: S._sweep(S.state, 10), k=3)
                res.append((t, len(S.state.usedIndices)))
                S.init_(S.state, b)      # ten sweeps from a fresh start: what the two routes are compared on
                S._sweep(S.state, 10)
                sol.append(S.state.x.to_host())
            (ts, ns), (td, nd) = res
            err_s = checked("sparse against dense sweeps", rel(sol[0], sol[1]), 1e-2)
            say(f"{M}x{N} {np.dtype(dt).name:9s} {100 * d:5.1f}% nrhs {nrhs:2d} | sparse {ts[0] / 1e3:8.2f} ms (min {ts[1] / 1e3:.2f}, max {ts[2] / 1e3:.2f})"
                f" {ts[0] / (10 * ns):7.3f} us/row step | dense {td[0] / 1e3:8.2f} ms {td[0] / (10 * nd):7.3f} us/row step"
                f" | dense/sparse {td[0] / ts[0]:6.2f}x | diff sparse-dense {err_s:.1e}")
    mats = {k: v for k, v in mats.items() if k[0] != M}   # (free the dense twins of this shape)

if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
