"""Float64 / ComplexF64 CGNR and FISTA + L1: the device plans (rls_cgnr_*_d / rls_fista_*_d) against the primitive loops
(use_device_plan_f64 = False) in ONE process, 32 iterations each.

Per leg: microseconds per iteration = a whole `solve_` without callbacks (init! included, ending in the download of x: a device
synchronise) on the host clock, divided by the 32 iterations; median of --repeats after a warm-up solve.  Kernel launches per
iteration: for the plan the pipeline's design count (two products + update, FISTA one more; the kernel trace in
profiles/f64_plans_kernel_stats.csv is the observed count), for the primitives the rls_*_d calls
of the solve (init!'s few included) / 32.  For the plan, `fraction_of_8TBps` is an ALGORITHMIC-bytes figure: the bytes one
matrix-free iteration has to move at least -- A twice, t written and read, and the update's passes over the N-vectors (CGNR:
p 3x, r 2x, x 2x, v 1x read or written, p, r, x written back = 12 N elements; FISTA with the extrapolation 14 N) -- over the
measured time per iteration, against the 8 TB/s HBM peak.  It is a whole-iteration rate (launch gaps, init! and the
single-workgroup update kernel are inside it), not a kernel's share of peak, and reads served by the Infinity Cache count as bytes.  With --errors the 4096 x 2048 ComplexF64 legs also report both
paths' error against the complex128 oracle (the yardstick of tests/test_gpu_f64_plans.py::test_full_size_complexf64).

    python tools/bench_f64_plans.py [--errors] [--out profiles/f64_plans.txt] [--only plan] [--shapes big]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
HBM_PEAK = 8.0e12
ITER = 32
REDUCTIONS = ("rls_nrm2_d", "rls_dotc_d", "rls_asum_d")
LAUNCHING = REDUCTIONS + ("rls_gemv_d", "rls_axpy_d", "rls_scal_d", "rls_lincomb_d", "rls_fill_d", "rls_prox_l1_d", "rls_prox_l2_d",
                          "rls_prox_l21_d", "rls_prox_positive_d", "rls_prox_real_d")


def plan_bytes(solver, M, N, es):
    """algorithmic bytes of one matrix-free iteration (see the module docstring)"""
    return 2 * M * N * es + 2 * M * es + (12 if solver == "cgnr" else 14) * N * es


def plan_launches(solver):
    return 3 + (1 if solver == "fista" else 0)


class CallCounter:
    """kernel launches behind the primitive loop: one per rls_*_d call, two for a reduction over more than 8192 elements"""

    def __init__(self, lib):
        self.lib, self.launches, self.orig = lib, 0, {n: getattr(lib, n) for n in LAUNCHING}

    def __enter__(self):
        for n, f in self.orig.items():
            def proxy(*a, _n=n, _f=f):
                self.launches += 2 if (_n in REDUCTIONS and a[2] > 8192) else 1
                return _f(*a)
            setattr(self.lib, n, proxy)
        return self

    def __exit__(self, *exc):
        for n, f in self.orig.items():
            setattr(self.lib, n, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--errors", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--shapes", choices=("all", "big", "small"), default="all")
    ap.add_argument("--only", choices=("plan", "primitives"), default=None, help="one path only (the kernel trace of the plan leg)")
    args = ap.parse_args()
    import rls_amd as rls
    import rls_oracle as O

    ctx = rls.default_context(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# Float64 / ComplexF64 plans vs primitive loops, {ITER} iterations, median of {args.repeats} (one process)")
    say("# shape dtype solver path us_per_iteration launches_per_iteration bytes_per_iteration fraction_of_8TBps")
    for M, N in {"all": ((4096, 2048), (256, 128)), "big": ((4096, 2048),), "small": ((256, 128),)}[args.shapes]:
        for dt in (np.complex128, np.float64):
            A, xt, b = O.make_problem(M, N, dt, 4)
            Ad, bd = rls.DeviceMatrix.from_host(A, ctx), rls.DeviceVector.from_host(b, ctx)
            rho = 0.9 / np.linalg.norm(A, 2) ** 2
            lam1 = 0.02 * float(np.max(np.abs(A.conj().T @ b)))
            es = np.dtype(dt).itemsize
            mks = {"cgnr": lambda: rls.createLinearSolver(rls.CGNR, Ad, reg=rls.L2Regularization(1e-3), iterations=ITER, relTol=0.0),
                   "fista": lambda: rls.createLinearSolver(rls.FISTA, Ad, reg=rls.L1Regularization(lam1), rho=rho, iterations=ITER, relTol=0.0)}
            for name, mk in mks.items():
                us = {}
                for plan in (False, True):
                    if args.only and (args.only == "plan") != plan:
                        continue
                    S = mk()
                    S.use_device_plan_f64 = plan
                    rls.solve_(S, bd)   # warm-up: code objects, the plan, the pool
                    assert bool(S.state._plan) == plan and S.state.iteration == ITER
                    ts = []
                    for _ in range(args.repeats):
                        ctx.sync()
                        t0 = time.perf_counter()
                        rls.solve_(S, bd).to_host()   # the plan: init_d + one step_status_d for all iterations; the primitives: the host loop
                        ts.append((time.perf_counter() - t0) / ITER * 1e6)
                    us[plan] = statistics.median(ts)
                    if plan:
                        nb = plan_bytes(name, M, N, es)
                        say(f"{M}x{N} {np.dtype(dt).name} {name} plan {us[plan]:.2f} {plan_launches(name)} {nb} {nb / (us[plan] * 1e-6) / HBM_PEAK:.3f}")
                    else:
                        with CallCounter(ctx.lib) as cc:
                            rls.solve_(S, bd)
                        say(f"{M}x{N} {np.dtype(dt).name} {name} primitives {us[plan]:.2f} {cc.launches / ITER:.1f} - -")
                if len(us) == 2:
                    say(f"#   {M}x{N} {np.dtype(dt).name} {name}: plan / primitives = {us[True] / us[False]:.3f}")
                if args.errors and (M, N) == (4096, 2048) and dt is np.complex128:
                    ref = (O.CGNR(A, reg=O.L2Regularization(1e-3), iterations=ITER, relTol=0.0) if name == "cgnr" else
                           O.FISTA(A, reg=O.L1Regularization(lam1), rho=rho, iterations=ITER, relTol=0.0))
                    O.solve(ref, b)
                    for plan in (False, True):
                        S = mk()
                        S.use_device_plan_f64 = plan
                        x = rls.solve_(S, bd).to_host()
                        e = float(np.linalg.norm(x - ref.x) / np.linalg.norm(ref.x))
                        say(f"#   error vs complex128 oracle, {M}x{N} {name} {'plan' if plan else 'primitives'}: {e:.3e}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
