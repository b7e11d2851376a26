"""The single-workgroup update kernels of csrc/solvers.hip and csrc/plan_fista.hip one launch at a time, against tests/upd_ref.py
(anchored to the oracle and held to its own gates in tests/test_upd_ref.py; the gates and their derivation: the docstring of upd_ref.py).

Every vector is a guarded buffer the test owns (a sentinel zone in front of and behind it, checked at every read), every plan is created
with resident = small = cgnr_pipeline = gram_pipeline = 0 and must report path 0 (two products + update kernel), and one launch is
isolated by reading everything before and after it:

  CGNR   rls_cgnr_init (cgnr_init_kernel), then rls_cgnr_step_status(s, 1) three times: the restatement is fed the device's own
         v = AHA p of that step, so only cgnr_update_reg_kernel<E, 1|2|4|8> (N <= 8192) / cgnr_update_kernel (N > 8192) is judged.
  FISTA  rls_fista_init (fista_init_kernel), then rls_fista_step_local_a (the product alone: res = AHA y is read back) and
         rls_fista_step_local_b (the update launch alone: fista_update_reg_kernel<E, 1|2|4>, or fista_update_kernel past 4096 and for
         L21).  y is the plan's own vector: it is restated from the x, xold that came back (exactly for the first two iterations, where
         c1 = 0, c2 = 1) and its bound joins the gate of x.
  cg!    rls_cg_local_apply / rls_cg_local_start / rls_cg_local_update, one launch each (cg_start_kernel, cg_update_kernel), and
         rls_cg_solve (maxiter 1 and 3, warm start) bit for bit against the same launches made one by one.
  ADMM   rls_admm_pre, rls_admm_post (admm_pre_kernel, admm_post_kernel) on their own; one rls_admm_step(a, 1) with L1 at N = 1025 and
         4097: the fused start's beta and xold, x byte for byte against rls_cg_solve on that beta, then admm_zu_kernel's z, u and norms
         from the x that came back.
  phases fista_update_kernel's phases 1 and 2 around the TV launch (iterationsTV = 0: the launch hands its input on, so the gradient step
         is read through x) and around the wavelet launch (first iteration: the bits of the gradient step are known, x must be the
         library's own wavelet prox of them).
  batch  the K = 3 plan with a padded ldv (rls_cg_create_batched, rls_admm_step, rls_admm_set_bregman): the dim3(K) launches of
         cg_start_kernel, cg_update_kernel and admm_zu_kernel, and cg_start_bregman_kernel.  A CHANGE OF SHAPE against the other cases:
         batched plans take M, N multiples of 16 only (at M = 8, N = 1025 the refusal is asserted), so this one runs at the nearest
         accepted shape, M = 16, N = 1040 = 1024 + 16 (still a ragged second pass of the 1024-stride loops), ldv = 1048.  No call
         isolates a batched launch and the products live in plan scratch, so with iterations_cg = 1 every column is judged from the
         matrices the test owns: AHA x and AHA u in float64 with upd_ref.product_gate, everything behind them as the single-column cases.
"""
import ctypes as C
import os
import sys
from contextlib import contextmanager

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pgm_ref as P  # noqa: E402
import upd_ref as R  # noqa: E402
from test_gpu_f64_plan_products import GUARD, Guarded, _report, held  # noqa: E402,F401

pytestmark = pytest.mark.gpu
DT = [np.float32, np.complex64]
DT_IDS = ["float32", "complex64"]
INVALID = -1
UNFUSED = dict(resident=0, small=0, cgnr_pipeline=0, gram_pipeline=0)
# what comes back afterwards: the library has no getter for these keys (rls_tune_get answers RLS_E_INVALID for every key but the one a
# binding reads), so, as every test that moves a switch does, the defaults the header documents are set again
DEFAULTS = dict(resident=1, small=1, cgnr_pipeline=1, gram_pipeline=1)
M = 8


@contextmanager
def unfused(ctx):
    """one launch per product and per update; the defaults come back whatever happens"""
    try:
        ctx.tune(**UNFUSED)
        yield
    finally:
        ctx.tune(**DEFAULTS)


def name(dt):
    return np.dtype(dt).name


def f(x):
    return float(np.float32(x))


def err(a, b):
    return np.abs(np.asarray(a).astype(np.complex128) - np.asarray(b).astype(np.complex128))


class Case:
    """A (8 x n) and its operator, b, and guarded vectors by name"""

    def __init__(self, rls, ctx, dt, n, names, seed=0):
        self.rls, self.ctx, self.lib, self.dt, self.n = rls, ctx, ctx.lib, np.dtype(dt), n
        self.A, self.b = R.problem(dt, n, seed, M)
        self.Ad = rls.DeviceMatrix.from_host(self.A, ctx)
        self.op = rls.OperatorHandle(self.Ad)
        self.bd = rls.DeviceVector.from_host(self.b, ctx)
        self.code = self.bd.code
        self.g = {k: Guarded(rls, ctx, dt, n, body=P.vector(dt, n, 31 * n + i), lead=GUARD) for i, k in enumerate(names)}
        self.plan = C.c_void_p()

    def ptr(self, k):
        return self.g[k].ptr

    def put(self, k, v):
        self.g[k] = Guarded(self.rls, self.ctx, self.dt, self.n, body=np.asarray(v, self.dt), lead=GUARD)

    def read(self):
        self.ctx.sync()
        return {k: g.read().copy() for k, g in self.g.items()}

    def path(self, fn):
        out = C.c_int32(-1)
        assert fn(self.plan, C.byref(out)) == 0
        return out.value


def fields(st):
    return {k: getattr(st, k) for k, _ in st._fields_}


# ---- CGNR ----------------------------------------------------------------------------------------------------------------------------------
def cgnr_plan(rls, ctx, dt, n, seed=0):
    c = Case(rls, ctx, dt, n, ("x", "r", "p", "v"), seed)
    assert c.lib.rls_cgnr_create(c.op.handle, c.ptr("x"), c.ptr("r"), c.ptr("p"), c.ptr("v"), C.byref(c.plan)) == 0
    return c


def cgnr_init(c, lam, rel_tol, iterations):
    from rls_amd import _lib
    st = _lib.CgnrStatus()
    assert c.lib.rls_cgnr_init(c.plan, c.bd.ptr, f(lam), f(rel_tol), iterations) == 0
    assert c.path(c.lib.rls_cgnr_path) == 0, "not the two-product path"
    assert c.lib.rls_cgnr_get_status(c.plan, C.byref(st)) == 0
    return c.read(), fields(st)


def cgnr_step(c, k=1):
    from rls_amd import _lib
    st = _lib.CgnrStatus()
    assert c.lib.rls_cgnr_step_status(c.plan, k, C.byref(st)) == 0
    return c.read(), fields(st)


def judge_cgnr_init(group, case, got, st, lam, rel_tol, max_iter):
    want = R.cgnr_init(got["r"], rel_tol, max_iter)
    for k in ("x", "v", "p"):
        assert got[k].tobytes() == want[k].tobytes(), (case, k)
    w_, b_ = P.norm_gate(got["r"])
    held(f"{group} z0", case, [abs(st["z0"] - w_)], [b_])
    held(f"{group} ||r||", case, [abs(st["residual"] - w_)], [b_])
    assert (st["iteration"], st["done"]) == (0, want["done"]), (case, st)
    return want


def judge_cgnr_update(group, case, before, after, st, lam, rel_tol, iteration, max_iter):
    rr = float(R.sumsq(before["r"]))
    z0 = float(np.sqrt(R.L(R.sumsq(before["r0"]))))
    v = after["v"]                                   # the device's own AHA p of this step
    w = R.cgnr_update(before["x"], before["r"], before["p"], v, rr, z0, lam, rel_tol, iteration, max_iter, r_dev=after["r"])
    gates = R.cgnr_gates(before["x"], before["r"], before["p"], v, lam, w, after["r"])
    R.check(held, group, case, after, w, gates)
    ma = abs(w["alpha"])
    held(f"{group} alpha", case, [abs(complex(st["alpha_re"], st["alpha_im"]) - w["alpha"])], [w["ds_alpha"] * ma])
    held(f"{group} beta", case, [abs(st["beta_re"] - w["beta"])], [w["ds_beta"] * abs(w["beta"])])
    held(f"{group} zeta", case, [abs(st["zeta"] - rr)], [P.sum_gate(rr, before["r"].size, rr)])
    w_, b_ = P.norm_gate(after["r"])
    held(f"{group} ||r||", case, [abs(st["residual"] - w_)], [b_])
    assert st["beta_im"] == 0 and st["iteration"] == w["iteration"], (case, st)
    return w


def cgnr_group(dt, n):
    form = "cgnr_update_kernel" if n > 8192 else f"cgnr_update_reg_kernel<{1 if n <= 1024 else 2 if n <= 2048 else 4 if n <= 4096 else 8}>"
    return f"{form} {name(dt)}"


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("lam", [0.0, 0.05], ids=["lambda0", "lambda>0"])
@pytest.mark.parametrize("n", R.LENGTHS)
def test_cgnr_init_and_three_updates(rls, ctx, dt, n, lam):
    with unfused(ctx):
        c = cgnr_plan(rls, ctx, dt, n)
        try:
            iters = 5
            cur, st = cgnr_init(c, lam, 0.0, iters)
            judge_cgnr_init(f"cgnr_init_kernel {name(dt)}", f"n={n}", cur, st, lam, 0.0, min(iters, n))
            r0 = cur["r"].copy()
            for k in range(min(3, n)):
                nxt, st = cgnr_step(c)
                assert nxt["v"].tobytes() != cur["v"].tobytes() or not np.any(cur["p"])
                w = judge_cgnr_update(cgnr_group(dt, n), f"n={n} lambda={lam} iteration {k + 1}", dict(cur, r0=r0), nxt, st, lam, 0.0, k,
                                      min(iters, n))
                assert st["done"] == w["done"] == int(k + 1 >= min(iters, n)), st
                cur = nxt
            assert c.path(c.lib.rls_cgnr_path) == 0
        finally:
            assert c.lib.rls_cgnr_destroy(c.plan) == 0


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("n", [1, 65, 1025, 2049, 4097, 8193])
def test_cgnr_done_rules(rls, ctx, dt, n):
    """max_iter and rel_tol each stop at the iteration the restatement says; iterations > N stops at N; a step call after `done` moves
    nothing (the early return behind the loads of the register forms); max_iter = 0 is done at entry; the same case twice: same bytes"""
    with unfused(ctx):
        c = cgnr_plan(rls, ctx, dt, n)
        try:
            # max_iter = 0: done at entry, a step changes nothing
            cur, st = cgnr_init(c, 0.0, 0.0, 0)
            assert (st["iteration"], st["done"]) == (0, 1)
            nxt, st2 = cgnr_step(c)
            assert all(nxt[k].tobytes() == cur[k].tobytes() for k in cur) and st2 == st
            # max_iter = 2 (or N when smaller: iterations > N stops at N)
            stop = min(2, n)
            cur, st = cgnr_init(c, 0.0, 0.0, 2 if n > 1 else 7)
            runs = [cur]
            for k in range(stop):
                assert st["done"] == 0, (k, st)
                cur, st = cgnr_step(c)
                runs.append(cur)
            assert (st["iteration"], st["done"]) == (stop, 1), st
            nxt, st2 = cgnr_step(c)
            assert all(nxt[k].tobytes() == cur[k].tobytes() for k in cur) and st2 == st, "a step after done moved something"
            # the same again: the same bytes
            cur, st = cgnr_init(c, 0.0, 0.0, 2 if n > 1 else 7)
            for k in range(stop):
                cur, st = cgnr_step(c)
                assert all(cur[q].tobytes() == runs[k + 1][q].tobytes() for q in cur), (k, "run to run")
            if n == 1:
                return
            # rel_tol on either side of ||r_1|| / z0, 2e-3 relative away
            q = float(np.sqrt(R.sumsq(runs[1]["r"]) / R.sumsq(runs[0]["r"])))
            for rel_tol, done in ((np.float32(q * (1 + 2e-3)), 1), (np.float32(q * (1 - 2e-3)), 0)):
                cur, st = cgnr_init(c, 0.0, rel_tol, 5)
                cur, st = cgnr_step(c)
                w = R.cgnr_update(runs[0]["x"], runs[0]["r"], runs[0]["p"], cur["v"], float(R.sumsq(runs[0]["r"])),
                                  float(np.sqrt(R.sumsq(runs[0]["r"]))), 0.0, rel_tol, 0, min(5, n), r_dev=cur["r"])
                assert st["done"] == w["done"] == done, (rel_tol, q, st)
                assert all(cur[k].tobytes() == runs[1][k].tobytes() for k in ("x", "r", "p"))
                nxt, st2 = cgnr_step(c)
                if done:
                    assert all(nxt[k].tobytes() == cur[k].tobytes() for k in cur) and st2 == st
                else:
                    assert st2["iteration"] == 2 and nxt["x"].tobytes() != cur["x"].tobytes()
        finally:
            assert c.lib.rls_cgnr_destroy(c.plan) == 0


def test_cgnr_refusals(rls, ctx):
    c = Case(rls, ctx, np.float32, 65, ("x", "r", "p", "v"))
    before = c.read()
    out = C.c_void_p()
    lib = c.lib
    assert lib.rls_cgnr_create(None, c.ptr("x"), c.ptr("r"), c.ptr("p"), c.ptr("v"), C.byref(out)) == INVALID
    for miss in range(4):
        a = [c.ptr(k) if i != miss else None for i, k in enumerate(("x", "r", "p", "v"))]
        assert lib.rls_cgnr_create(c.op.handle, *a, C.byref(out)) == INVALID
    assert lib.rls_cgnr_create(c.op.handle, c.ptr("x"), c.ptr("r"), c.ptr("p"), c.ptr("v"), None) == INVALID
    assert lib.rls_cgnr_path(None, C.byref(C.c_int32())) == INVALID
    after = c.read()
    assert all(after[k].tobytes() == before[k].tobytes() for k in before)


# ---- FISTA ---------------------------------------------------------------------------------------------------------------------------------
def fista_plan(rls, ctx, dt, n, reg, proj, lam, slices=1):
    c = Case(rls, ctx, dt, n, ("x", "x0", "xold", "res"))
    assert c.lib.rls_fista_create(c.op.handle, c.ptr("x"), c.ptr("x0"), c.ptr("xold"), c.ptr("res"), C.byref(c.plan)) == 0
    assert c.lib.rls_fista_set_reg(c.plan, reg, f(lam), slices, proj) == 0
    return c


def fista_status(c):
    from rls_amd import _lib
    st = _lib.FistaStatus()
    assert c.lib.rls_fista_get_status(c.plan, C.byref(st)) == 0
    return fields(st)


def fista_group(dt, n, reg):
    form = "fista_update_kernel" if (n > 4096 or reg == R.REG_L21) else f"fista_update_reg_kernel<{1 if n <= 1024 else 2 if n <= 2048 else 4}>"
    return f"{form} {name(dt)}"


def fista_three_updates(rls, ctx, dt, n, reg, proj, slices=1, iters=5):
    lam = np.float32(0.02)
    with unfused(ctx):
        c = fista_plan(rls, ctx, dt, n, reg, proj, lam, slices)
        try:
            hi_ = np.complex128 if np.dtype(dt).kind == "c" else np.float64
            rho = np.float32(0.9 / np.linalg.norm(c.A.astype(hi_), 2) ** 2)
            assert c.lib.rls_fista_init(c.plan, c.bd.ptr, f(rho), 1.0, 0.0, iters, 0) == 0
            assert c.path(c.lib.rls_fista_path) == 0, "not the two-product path"
            cur, st = c.read(), fista_status(c)
            case = f"n={n} reg={reg} proj={proj} slices={slices}"
            want = R.fista_init(cur["x0"], 1.0, iters)
            for k in ("x", "xold", "res"):
                assert cur[k].tobytes() == want[k].tobytes(), (case, k)
            w_, b_ = P.norm_gate(cur["x0"])
            held(f"fista_init_kernel {name(dt)} ||x0||", case, [abs(st["norm_x0"] - w_)], [b_])
            assert (st["iteration"], st["done"], st["theta"], st["theta_old"]) == (0, 0, 1.0, 1.0) and np.isinf(st["rel_res_norm"]), st
            norm_x0 = w_
            group = fista_group(dt, n, reg)
            theta, theta_old = np.float32(1), np.float32(1)
            for k in range(3):
                new, old = ("xold", "x") if k % 2 == 0 else ("x", "xold")       # state.x after the swap: buf[(it & 1) ^ 1]
                y, yb = R.fista_y(cur[new], cur[old], theta_old, theta)         # (x_{k-1}, x_k)
                assert c.lib.rls_fista_step_local_a(c.plan) == 0
                raw = c.read()["res"]
                assert c.lib.rls_fista_step_local_b(c.plan) == 0
                nxt, st = c.read(), fista_status(c)
                w, gates = R.fista_update(cur[old], y, raw, cur["x0"], rho, lam, reg, proj, slices, theta, k, iters, 0.0, norm_x0,
                                          res_dev=nxt["res"], y_bound=yb)
                kc = f"{case} iteration {k + 1}"
                held(f"{group} res", kc, err(nxt["res"], w["res"]), gates["res"])
                held(f"{group} x", kc, err(nxt[new], w["x"]), gates["x"])
                assert nxt[old].tobytes() == cur[old].tobytes() and nxt["x0"].tobytes() == cur["x0"].tobytes(), (kc, "x_k or x0 written")
                wn, bn = P.norm_gate(nxt["res"])
                held(f"{group} ||res||", kc, [abs(st["residual"] - wn)], [bn])
                held(f"{group} rel_res_norm", kc, [abs(st["rel_res_norm"] - wn / norm_x0)], [bn / norm_x0 + 2 * R.U * wn / norm_x0])
                # theta, theta_old: the Float32 recursion bit for bit (exactly representable in Float64)
                assert (np.float64(st["theta"]), np.float64(st["theta_old"])) == (np.float64(w["theta"]), np.float64(w["theta_old"])), (kc, st)
                assert (st["iteration"], st["done"]) == (k + 1, 0), (kc, st)
                theta_old, theta = w["theta_old"], w["theta"]
                cur = nxt
            assert c.path(c.lib.rls_fista_path) == 0
        finally:
            assert c.lib.rls_fista_destroy(c.plan) == 0


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("n", R.LENGTHS)
def test_fista_init_and_three_updates_l1(rls, ctx, dt, n):
    fista_three_updates(rls, ctx, dt, n, R.REG_L1, R.PROJ_NONE)


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("proj", [R.PROJ_NONE, R.PROJ_REAL, R.PROJ_POSITIVE], ids=["none", "real", "positive"])
@pytest.mark.parametrize("reg", [R.REG_NONE, R.REG_L1, R.REG_L2, R.REG_L21], ids=["none", "l1", "l2", "l21"])
def test_fista_every_regulariser_and_projection(rls, ctx, dt, reg, proj):
    fista_three_updates(rls, ctx, dt, 1025, reg, proj, slices=5 if reg == R.REG_L21 else 1)


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("slices", [1, 4])
@pytest.mark.parametrize("n", [1024, 2049])
def test_fista_l21_takes_the_loop_form_below_4096(rls, ctx, dt, n, slices):
    fista_three_updates(rls, ctx, dt, n, R.REG_L21, R.PROJ_NONE, slices=slices)


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("n", [65, 1025, 2049, 4097])
def test_fista_done_rules(rls, ctx, dt, n):
    """through rls_fista_step_status(s, 1) on path 0: max_iter and rel_tol stop where the restatement says, a step after `done` moves
    nothing, max_iter = 0 is done at entry, and the same case twice gives the same bytes"""
    from rls_amd import _lib
    lam = np.float32(0.02)
    with unfused(ctx):
        c = fista_plan(rls, ctx, dt, n, R.REG_L1, R.PROJ_NONE, lam)
        try:
            hi_ = np.complex128 if np.dtype(dt).kind == "c" else np.float64
            rho = np.float32(0.9 / np.linalg.norm(c.A.astype(hi_), 2) ** 2)

            def init(rel_tol, iters):
                assert c.lib.rls_fista_init(c.plan, c.bd.ptr, f(rho), 1.0, f(rel_tol), iters, 0) == 0
                assert c.path(c.lib.rls_fista_path) == 0
                return c.read(), fista_status(c)

            def step():
                st = _lib.FistaStatus()
                assert c.lib.rls_fista_step_status(c.plan, 1, C.byref(st)) == 0
                return c.read(), fields(st)

            cur, st = init(0.0, 0)
            assert (st["iteration"], st["done"]) == (0, 1)
            nxt, st2 = step()
            assert all(nxt[k].tobytes() == cur[k].tobytes() for k in cur) and st2 == st
            runs = []
            for _ in range(2):
                cur, st = init(0.0, 2)
                seq = [cur]
                for k in range(2):
                    assert st["done"] == 0
                    cur, st = step()
                    seq.append(cur)
                assert (st["iteration"], st["done"]) == (2, 1), st
                nxt, st2 = step()
                assert all(nxt[k].tobytes() == cur[k].tobytes() for k in cur) and st2 == st, "a step after done moved something"
                runs.append(seq)
            assert all(a[k].tobytes() == b[k].tobytes() for a, b in zip(*runs) for k in a), "run to run"
            # rel_tol on either side of ||res_1|| / ||x0||: done is `<`
            q = float(np.sqrt(R.sumsq(runs[0][1]["res"]) / R.sumsq(runs[0][0]["x0"])))
            for rel_tol, done in ((np.float32(q * (1 + 2e-3)), 1), (np.float32(q * (1 - 2e-3)), 0)):
                cur, st = init(rel_tol, 5)
                x0_ = cur["x0"]
                cur, st = step()
                zero = np.zeros_like(x0_)
                w, _ = R.fista_update(zero, zero, cur["res"] + x0_, x0_, rho, lam, R.REG_L1, R.PROJ_NONE, 1, 1.0, 0, 5, rel_tol,
                                      float(np.sqrt(R.L(R.sumsq(x0_)))), res_dev=cur["res"])
                assert (st["iteration"], st["done"]) == (w["iteration"], w["done"]) == (1, done), (rel_tol, q, st)
                assert all(cur[k].tobytes() == runs[0][1][k].tobytes() for k in cur)
                nxt, st2 = step()
                if done:
                    assert all(nxt[k].tobytes() == cur[k].tobytes() for k in cur) and st2 == st
                else:
                    assert st2["iteration"] == 2
        finally:
            assert c.lib.rls_fista_destroy(c.plan) == 0


def test_fista_refusals(rls, ctx):
    c = Case(rls, ctx, np.float32, 65, ("x", "x0", "xold", "res"))
    before = c.read()
    lib, out = c.lib, C.c_void_p()
    assert lib.rls_fista_create(None, c.ptr("x"), c.ptr("x0"), c.ptr("xold"), c.ptr("res"), C.byref(out)) == INVALID
    for miss in range(4):
        a = [c.ptr(k) if i != miss else None for i, k in enumerate(("x", "x0", "xold", "res"))]
        assert lib.rls_fista_create(c.op.handle, *a, C.byref(out)) == INVALID
    assert lib.rls_fista_create(c.op.handle, c.ptr("x"), c.ptr("x0"), c.ptr("xold"), c.ptr("res"), C.byref(c.plan)) == 0
    try:
        for reg, slices, proj in ((-1, 1, 0), (6, 1, 0), (R.REG_L1, 1, 3), (R.REG_L1, 1, -1), (R.REG_L21, 0, 0), (R.REG_L21, 66, 0), (5, 1, 0)):
            assert lib.rls_fista_set_reg(c.plan, reg, 0.1, slices, proj) == INVALID, (reg, slices, proj)
    finally:
        assert lib.rls_fista_destroy(c.plan) == 0
    after = c.read()
    assert all(after[k].tobytes() == before[k].tobytes() for k in before)


# ---- cg! -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("n", R.LENGTHS)
def test_cg_start_and_three_updates(rls, ctx, dt, n):
    """from a non-zero warm start: the launches one by one through rls_cg_local_*, every one judged; then rls_cg_solve with maxiter 1
    and 3 from the same start reproduces the bytes of the first and the third of them"""
    from rls_amd import _lib
    rho, reltol, maxiter = np.float32(0.3), 0.0, 3
    with unfused(ctx):
        c = Case(rls, ctx, dt, n, ("x", "b", "u", "r", "c"))
        assert c.lib.rls_cg_create(c.op.handle, c.ptr("u"), c.ptr("r"), c.ptr("c"), C.byref(c.plan)) == 0
        try:
            assert c.path(c.lib.rls_cg_path) == 0, "not the two-product path"
            start = c.read()
            st = _lib.CgStatus()
            assert c.lib.rls_cg_local_apply(c.plan, c.ptr("x")) == 0
            cur = c.read()
            assert c.lib.rls_cg_local_start(c.plan, c.ptr("x"), c.ptr("b"), f(rho), maxiter, reltol) == 0
            nxt = c.read()
            assert c.lib.rls_cg_get_status(c.plan, C.byref(st)) == 0
            case = f"n={n}"
            w = R.cg_start(cur["x"], cur["b"], cur["c"], rho, reltol, maxiter)
            R.check(held, f"cg_start_kernel {name(dt)}", case, nxt, w, R.cg_start_gates(cur["x"], cur["b"], cur["c"], rho))
            assert nxt["u"].tobytes() == nxt["r"].tobytes() and all(nxt[k].tobytes() == cur[k].tobytes() for k in ("x", "b", "c"))
            rec = R.cg_start_record(nxt["r"], reltol, maxiter)
            wn, bn = P.norm_gate(nxt["r"])
            held(f"cg_start_kernel {name(dt)} ||r||", case, [abs(st.residual - wn)], [bn])
            assert (st.iterations, st.tol) == (0, rec["tol"]), (st.iterations, st.tol)
            residual = wn
            stages = []
            cur = nxt
            for k in range(min(maxiter, n)):
                assert c.lib.rls_cg_local_apply(c.plan, None) == 0
                cv = c.read()["c"]
                assert c.lib.rls_cg_local_update(c.plan, c.ptr("x")) == 0
                nxt = c.read()
                assert c.lib.rls_cg_get_status(c.plan, C.byref(st)) == 0
                w = R.cg_update(cur["x"], cur["u"], cur["r"], cv, residual, rho, rec["tol"], k, maxiter, r_dev=nxt["r"], c_dev=nxt["c"])
                gates = R.cg_update_gates(cur["x"], cur["u"], cur["r"], cv, rho, w, nxt["r"], nxt["c"])
                kc = f"{case} iteration {k + 1}"
                R.check(held, f"cg_update_kernel {name(dt)}", kc, nxt, w, gates)
                if w["done"]:
                    assert nxt["u"].tobytes() == cur["u"].tobytes(), "u moved on the last iteration"
                wn, bn = P.norm_gate(nxt["r"])
                held(f"cg_update_kernel {name(dt)} ||r||", kc, [abs(st.residual - wn)], [bn])
                assert st.iterations == k + 1 and nxt["b"].tobytes() == cur["b"].tobytes()
                assert w["done"] == int(k + 1 >= maxiter) or n < maxiter
                residual = wn
                stages.append(nxt)
                cur = nxt
                if w["done"]:
                    break
            # a further update launch after done: nothing moves
            if w["done"]:
                assert c.lib.rls_cg_local_apply(c.plan, None) == 0
                held_c = c.read()
                assert c.lib.rls_cg_local_update(c.plan, c.ptr("x")) == 0
                again = c.read()
                assert all(again[k].tobytes() == held_c[k].tobytes() for k in again), "an update after done moved something"
            # rls_cg_solve, maxiter 3 (the whole sequence) and 1 (the first launch pair, u left as the start made it)
            if n >= maxiter:
                for k_, v_ in start.items():
                    c.put(k_, v_)
                plan2 = C.c_void_p()
                assert c.lib.rls_cg_create(c.op.handle, c.ptr("u"), c.ptr("r"), c.ptr("c"), C.byref(plan2)) == 0
                try:
                    assert c.lib.rls_cg_solve(plan2, c.ptr("x"), c.ptr("b"), f(rho), maxiter, reltol) == 0
                    got = c.read()
                    assert all(got[k].tobytes() == stages[-1][k].tobytes() for k in got), "rls_cg_solve(maxiter=3) != the launches one by one"
                    assert c.lib.rls_cg_get_status(plan2, C.byref(st)) == 0 and st.iterations == maxiter
                    for k_, v_ in start.items():
                        c.put(k_, v_)
                    assert c.lib.rls_cg_destroy(plan2) == 0
                    plan2 = C.c_void_p()
                    assert c.lib.rls_cg_create(c.op.handle, c.ptr("u"), c.ptr("r"), c.ptr("c"), C.byref(plan2)) == 0
                    assert c.lib.rls_cg_solve(plan2, c.ptr("x"), c.ptr("b"), f(rho), 1, reltol) == 0
                    got = c.read()
                    assert c.lib.rls_cg_get_status(plan2, C.byref(st)) == 0 and st.iterations == 1
                    for k_ in ("x", "r", "c"):
                        assert got[k_].tobytes() == stages[0][k_].tobytes(), ("rls_cg_solve(maxiter=1)", k_)
                finally:
                    assert c.lib.rls_cg_destroy(plan2) == 0
        finally:
            assert c.lib.rls_cg_destroy(c.plan) == 0


# ---- rls_admm_pre / rls_admm_post ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("n", R.LENGTHS)
def test_admm_pre_and_post(rls, ctx, dt, n):
    names = ("beta", "beta_y", "z", "u", "x", "xold", "zold")
    g = {k: Guarded(rls, ctx, dt, n, body=P.vector(dt, n, 17 * n + i), lead=GUARD) for i, k in enumerate(names)}
    code = rls.DeviceVector(1, dt, ctx).code
    rho = np.float32(0.37)

    def read():
        ctx.sync()
        return {k: v.read().copy() for k, v in g.items()}

    cur = read()
    for acc in (0, 1):
        assert ctx.lib.rls_admm_pre(ctx.handle, code, n, g["beta"].ptr, g["beta_y"].ptr, g["z"].ptr, g["u"].ptr, g["x"].ptr, g["xold"].ptr,
                                    f(rho), acc) == 0
        nxt = read()
        w = R.admm_pre(cur["beta"], cur["beta_y"], cur["z"], cur["u"], cur["x"], rho, acc)
        R.check(held, f"admm_pre_kernel {name(dt)}", f"n={n} accumulate={acc}", nxt, w,
                R.admm_pre_gates(cur["beta"], cur["beta_y"], cur["z"], cur["u"], rho, acc), exact=() if acc else ("xold",))
        untouched = ("beta_y", "z", "u", "x", "zold") + (("xold",) if acc else ())
        assert all(nxt[k].tobytes() == cur[k].tobytes() for k in untouched)
        cur = nxt
    out = (C.c_float * 6)()
    assert ctx.lib.rls_admm_post(ctx.handle, code, n, g["x"].ptr, g["xold"].ptr, g["z"].ptr, g["zold"].ptr, g["u"].ptr, out) == 0
    nxt = read()
    case = f"n={n}"
    R.check(held, f"admm_post_kernel {name(dt)}", case, nxt, R.admm_post(cur["x"], cur["xold"], cur["z"], cur["zold"], cur["u"]),
            R.admm_post_gates(cur["x"], cur["z"], cur["u"]))
    assert all(nxt[k].tobytes() == cur[k].tobytes() for k in names if k != "u")
    norms = R.admm_norms(cur["x"], cur["xold"], cur["z"], cur["zold"], cur["u"], nxt["u"])
    (dx, bdx), (dz, bdz), (du, bdu), (nx, bnx), (nz, bnz), (nxz, bnxz), (nu, bnu) = norms
    got = np.array(out[:], np.float64)
    group = f"admm_post_kernel {name(dt)} norms"
    held(group, case, [abs(got[0] - (dx + dz + du)), abs(got[1] - dz), abs(got[2] - max(nx, nz)), abs(got[3] - nxz), abs(got[4] - nu),
                       abs(got[5] - dx)],
         [bdx + bdz + bdu + 2 * R.U * (dx + dz + du), bdz, max(bnx, bnz), bnxz, bnu, bdx])
    # refusals: nothing is written
    cur = nxt
    lib, h = ctx.lib, ctx.handle
    a = [g[k].ptr for k in ("beta", "beta_y", "z", "u", "x", "xold")]
    assert lib.rls_admm_pre(h, code, -1, *a, f(rho), 0) == INVALID
    assert lib.rls_admm_pre(h, 99, n, *a, f(rho), 0) == INVALID
    assert lib.rls_admm_pre(h, code, n, None, *a[1:], f(rho), 0) == INVALID
    p = [g[k].ptr for k in ("x", "xold", "z", "zold", "u")]
    assert lib.rls_admm_post(h, code, 0, *p, out) == INVALID
    assert lib.rls_admm_post(h, 99, n, *p, out) == INVALID
    assert lib.rls_admm_post(h, code, n, *p[:4], None, out) == INVALID
    assert lib.rls_admm_post(h, code, n, *p, None) == INVALID
    nxt = read()
    assert all(nxt[k].tobytes() == cur[k].tobytes() for k in names)


# ---- one whole outer iteration of the ADMM plan: cg_start_kernel with the fused right-hand side, cg_update_kernel, admm_zu_kernel ----------------
@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("proj", [R.PROJ_NONE, R.PROJ_POSITIVE], ids=["none", "positive"])
@pytest.mark.parametrize("n", [1025, 4097])
def test_admm_step_l1(rls, ctx, dt, n, proj):
    """rls_admm_step(a, 1) with L1: xold and beta from the fused start, x against rls_cg_solve on the beta that came back (the kernels
    test_cg_start_and_three_updates judges) byte for byte, then admm_zu_kernel alone: z, u and the norms of the status from the x that
    came back; `done` at max_iter, and a further step moves nothing"""
    from rls_amd import _lib
    names = ("x", "xold", "beta", "beta_y", "z0", "z1", "u", "cu", "cr", "cc")
    rho, lam, icg = np.float32(0.3), np.float32(0.05), 2
    with unfused(ctx):
        c = Case(rls, ctx, dt, n, names)
        a = C.c_void_p()
        assert c.lib.rls_cg_create(c.op.handle, c.ptr("cu"), c.ptr("cr"), c.ptr("cc"), C.byref(c.plan)) == 0
        try:
            assert c.path(c.lib.rls_cg_path) == 0, "not the two-product path"
            assert c.lib.rls_admm_create(c.plan, C.byref(a)) == 0
            p = _lib.AdmmParams()
            for k in ("x", "xold", "beta", "beta_y", "z0", "z1", "u"):
                setattr(p, k, c.ptr(k))
            p.rho, p.sigma_abs, p.rel_tol, p.iterations, p.iterations_cg, p.tol_inner = f(rho), 0.0, 0.0, 1, icg, 0.0
            p.reg_kind, p.prox_lambda, p.proj_kind = R.REG_L1, f(lam), proj
            assert c.lib.rls_admm_init(a, C.byref(p)) == 0
            cur = c.read()
            st, log = _lib.AdmmStatus(), (C.c_float * 8)()
            assert c.lib.rls_admm_step_status(a, 1, C.byref(st), log, 1) == 0
            nxt = c.read()
            case, g = f"n={n} proj={proj}", name(dt)
            assert c.path(c.lib.rls_cg_path) == 0
            # the fused start: xold = x, beta = beta_y + rho (z - u)
            w = R.cg_start(cur["x"], None, cur["cc"], rho, 0.0, icg, fuse=(cur["beta_y"], cur["z0"], cur["u"], rho))
            assert nxt["xold"].tobytes() == cur["x"].tobytes()
            held(f"cg_start_kernel fused {g} beta", case, err(nxt["beta"], w["beta"]),
                 R.cg_start_gates(cur["x"], None, cur["cc"], rho, fuse=(cur["beta_y"], cur["z0"], cur["u"], rho))["beta"])
            assert all(nxt[k].tobytes() == cur[k].tobytes() for k in ("beta_y", "z0"))
            # x: the plain cg! from the same start on the beta that came back
            t = Case(rls, ctx, dt, n, ("x", "b", "u", "r", "c"))
            t.put("x", cur["x"])
            t.put("b", nxt["beta"])
            assert t.lib.rls_cg_create(c.op.handle, t.ptr("u"), t.ptr("r"), t.ptr("c"), C.byref(t.plan)) == 0
            try:
                assert t.lib.rls_cg_solve(t.plan, t.ptr("x"), t.ptr("b"), f(rho), icg, 0.0) == 0
                plain = t.read()
            finally:
                assert t.lib.rls_cg_destroy(t.plan) == 0
            assert nxt["x"].tobytes() == P.project(plain["x"], proj).tobytes(), "x is not proj(cg!(x, beta))"
            for k_, q_ in (("cu", "u"), ("cr", "r"), ("cc", "c")):
                assert nxt[k_].tobytes() == plain[q_].tobytes(), k_
            # admm_zu_kernel from the x that came back
            z = R.admm_zu(nxt["x"], None, cur["u"], R.REG_L1, lam, proj, z_dev=nxt["z1"])
            held(f"admm_zu_kernel {g} z", case, err(nxt["z1"], z["z"]), R.admm_zu_gates(nxt["x"], cur["u"], R.REG_L1)["z"])
            held(f"admm_zu_kernel {g} u", case, err(nxt["u"], z["u"]), R.admm_u_gate(nxt["x"], nxt["z1"], cur["u"])["u"])
            norms = R.admm_norms(nxt["x"], nxt["xold"], nxt["z1"], cur["z0"], cur["u"], nxt["u"])
            (dx, bdx), (dz, bdz), (du, bdu), (nx, bnx), (nz, bnz), (nxz, bnxz), (nu, bnu) = norms
            r_ = float(rho)
            held(f"admm_zu_kernel {g} norms", case,
                 [abs(st.delta - (dx + dz + du)), abs(st.sk - r_ * dz), abs(st.eps_pri - max(nx, nz)), abs(st.rk - nxz), abs(st.eps_dua - r_ * nu)],
                 [bdx + bdz + bdu + 2 * R.U * (dx + dz + du), r_ * bdz + R.U * r_ * dz, max(bnx, bnz), bnxz, r_ * bnu + R.U * r_ * nu])
            # the record as the kernel forms it from ITS Float32 norms: sqrt(dx) comes back as log[0] - ..., so rebuild from the status
            assert (st.iteration, st.done, st.cg_iterations) == (1, 1, icg), (st.iteration, st.done, st.cg_iterations)
            assert [log[i] for i in range(5)] == [st.delta, st.sk, st.eps_pri, st.rk, st.eps_dua] and log[5] == icg
            # done: a further step moves nothing
            assert c.lib.rls_admm_step_status(a, 1, C.byref(st), log, 1) == 0
            again = c.read()
            assert all(again[k].tobytes() == nxt[k].tobytes() for k in names) and (st.iteration, st.done) == (1, 1)
        finally:
            if a:
                assert c.lib.rls_admm_destroy(a) == 0
            assert c.lib.rls_cg_destroy(c.plan) == 0


def test_batched_cg_plan_is_refused_at_these_shapes(rls, ctx):
    """rls_cg_create_batched runs on the matrix cores and takes M, N multiples of 16 only (include/rls_mi355x.h): at M = 8, N = 1025,
    K = 3 with a padded ldv it answers RLS_E_UNSUPPORTED, creates nothing and writes nothing"""
    n, K, ldv = 1025, 3, 1032
    c = Case(rls, ctx, np.complex64, n, ())
    U_, R_, C_ = (Guarded(rls, ctx, np.complex64, ldv * K, body=P.vector(np.complex64, ldv * K, 5 + i), lead=GUARD) for i in range(3))
    out = C.c_void_p()
    assert c.lib.rls_cg_create_batched(c.op.handle, K, U_.ptr, R_.ptr, C_.ptr, ldv, C.byref(out)) == -2 and not out
    ctx.sync()
    for g_ in (U_, R_, C_):
        assert g_.read().tobytes() == g_.host0[GUARD:GUARD + ldv * K].tobytes()


# ---- phases 1 and 2 of fista_update_kernel around a prox that is a launch of its own ------------------------------------------------------------
@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("proj", [R.PROJ_NONE, R.PROJ_POSITIVE], ids=["none", "positive"])
def test_fista_phases_around_the_tv_launch(rls, ctx, dt, proj):
    """TV with iterationsTV = 0: the FGP launch hands its input on unchanged (x - lam grad^T(0)), so phase 1's gradient step, which lives in
    plan scratch, is read through phase 2's x = proj(tv_out); res, ||res|| (phase 1), x, theta, theta_old, done (phase 2) as the one-launch
    form.  n = 1025 = 25 x 41"""
    n, iters, lam = 1025, 5, np.float32(0.02)
    with unfused(ctx):
        c = Case(rls, ctx, dt, n, ("x", "x0", "xold", "res"))
        assert c.lib.rls_fista_create(c.op.handle, c.ptr("x"), c.ptr("x0"), c.ptr("xold"), c.ptr("res"), C.byref(c.plan)) == 0
        try:
            shape, dims = (C.c_int64 * 2)(25, 41), (C.c_int32 * 2)(0, 1)
            assert c.lib.rls_fista_set_reg_tv(c.plan, f(lam), 2, shape, 2, dims, 0, proj) == 0
            hi_ = np.complex128 if np.dtype(dt).kind == "c" else np.float64
            rho = np.float32(0.9 / np.linalg.norm(c.A.astype(hi_), 2) ** 2)
            assert c.lib.rls_fista_init(c.plan, c.bd.ptr, f(rho), 1.0, 0.0, iters, 0) == 0
            assert c.path(c.lib.rls_fista_path) == 0
            cur = c.read()
            norm_x0 = P.norm_gate(cur["x0"])[0]
            theta, theta_old = np.float32(1), np.float32(1)
            group = f"fista_update_kernel phases 1+2 (TV) {name(dt)}"
            for k in range(3):
                new, old = ("xold", "x") if k % 2 == 0 else ("x", "xold")
                y, yb = R.fista_y(cur[new], cur[old], theta_old, theta)
                assert c.lib.rls_fista_step_local_a(c.plan) == 0
                raw = c.read()["res"]
                assert c.lib.rls_fista_step_local_b(c.plan) == 0
                nxt, st = c.read(), fista_status(c)
                a_ = (cur[old], y, raw, cur["x0"], rho, lam, R.REG_NONE, proj, 1, theta, k, iters, 0.0, norm_x0)
                w1, g1 = R.fista_update(*a_, res_dev=nxt["res"], y_bound=yb, phase=1)
                w2, g2 = R.fista_update(*a_, phase=2, tv_out=w1["tv_in"], res_norm_in=w1["res_norm"])
                kc = f"proj={proj} iteration {k + 1}"
                held(f"{group} res", kc, err(nxt["res"], w1["res"]), g1["res"])
                held(f"{group} x", kc, err(nxt[new], w2["x"]), g1["tv_in"] + g2["x"])
                wn, bn = P.norm_gate(nxt["res"])
                held(f"{group} ||res||", kc, [abs(st["residual"] - wn)], [bn])
                assert nxt[old].tobytes() == cur[old].tobytes() and nxt["x0"].tobytes() == cur["x0"].tobytes()
                assert (np.float64(st["theta"]), np.float64(st["theta_old"])) == (np.float64(w2["theta"]), np.float64(w2["theta_old"])), (kc, st)
                assert (st["iteration"], st["done"]) == (w2["iteration"], w2["done"]) == (k + 1, 0), (kc, st)
                theta_old, theta = w2["theta_old"], w2["theta"]
                cur = nxt
        finally:
            assert c.lib.rls_fista_destroy(c.plan) == 0


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
def test_fista_phases_around_the_wavelet_launch(rls, ctx, dt):
    """wavelet L1 (Haar, 32 x 32), first iteration: y = 0, so phase 1's gradient step is -(rho res) with ONE rounding however it is
    contracted -- its bits are known; phase 2's x must be the bytes the library's own wavelet prox gives for them (the plan makes that
    very launch), projected; res, ||res||, theta, theta_old, done as the one-launch form"""
    n, iters, lam = 1024, 5, np.float32(0.02)
    with unfused(ctx):
        c = Case(rls, ctx, dt, n, ("x", "x0", "xold", "res"))
        wv = C.c_void_p()
        assert c.lib.rls_wavelet_create(ctx.handle, c.code, 2, (C.c_int64 * 2)(32, 32), 0, -1, C.byref(wv)) == 0
        assert c.lib.rls_fista_create(c.op.handle, c.ptr("x"), c.ptr("x0"), c.ptr("xold"), c.ptr("res"), C.byref(c.plan)) == 0
        try:
            assert c.lib.rls_fista_set_reg_wavelet(c.plan, wv, f(lam), R.PROJ_POSITIVE) == 0
            hi_ = np.complex128 if np.dtype(dt).kind == "c" else np.float64
            rho = np.float32(0.9 / np.linalg.norm(c.A.astype(hi_), 2) ** 2)
            assert c.lib.rls_fista_init(c.plan, c.bd.ptr, f(rho), 1.0, 0.0, iters, 0) == 0
            assert c.path(c.lib.rls_fista_path) == 0
            cur = c.read()
            norm_x0 = P.norm_gate(cur["x0"])[0]
            assert c.lib.rls_fista_step_local_a(c.plan) == 0
            raw = c.read()["res"]
            assert not raw.any(), "AHA 0 is not 0"
            assert c.lib.rls_fista_step_local_b(c.plan) == 0
            nxt, st = c.read(), fista_status(c)
            zero = np.zeros_like(raw)
            a_ = (zero, zero, raw, cur["x0"], rho, lam, R.REG_NONE, R.PROJ_POSITIVE, 1, 1.0, 0, iters, 0.0, norm_x0)
            w1, g1 = R.fista_update(*a_, res_dev=nxt["res"], phase=1)
            group = f"fista_update_kernel phases 1+2 (wavelet) {name(dt)}"
            held(f"{group} res", "iteration 1", err(nxt["res"], w1["res"]), g1["res"])
            tv_in = (-(np.float32(rho) * nxt["res"].view(np.float32))).view(nxt["res"].dtype)
            held(f"{group} tv_in", "iteration 1", err(tv_in, w1["tv_in"]), g1["tv_in"])
            t = rls.DeviceVector.from_host(tv_in, ctx)
            assert c.lib.rls_prox_wavelet_l1(wv, t.ptr, float(np.float32(rho) * np.float32(lam))) == 0
            w2, _ = R.fista_update(*a_, phase=2, tv_out=t.to_host(), res_norm_in=w1["res_norm"])
            assert nxt["xold"].tobytes() == w2["x"].astype(dt).tobytes(), "x is not proj(prox(the gradient step))"
            assert nxt["x"].tobytes() == cur["x"].tobytes()
            wn, bn = P.norm_gate(nxt["res"])
            held(f"{group} ||res||", "iteration 1", [abs(st["residual"] - wn)], [bn])
            assert (np.float64(st["theta"]), np.float64(st["theta_old"])) == (np.float64(w2["theta"]), np.float64(w2["theta_old"]))
            assert (st["iteration"], st["done"]) == (w2["iteration"], w2["done"]) == (1, 0)
        finally:
            assert c.lib.rls_fista_destroy(c.plan) == 0
            assert c.lib.rls_wavelet_destroy(wv) == 0


# ---- the convergence branch of admm_zu_kernel --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
def test_admm_step_converged_on_either_side_of_rel_tol(rls, ctx, dt):
    """iterations = 3, so that `done` after one step can only come from `converged`: rel_tol 2e-3 relative above and below the larger of
    rk / eps_pri and sk / eps_dua of the first step; the decision is upd_ref.admm_converged fed the Float32 record that came back"""
    from rls_amd import _lib
    names = ("x", "xold", "beta", "beta_y", "z0", "z1", "u", "cu", "cr", "cc")
    n, rho, lam = 1025, np.float32(0.3), np.float32(0.05)

    def run(rel_tol):
        c = Case(rls, ctx, dt, n, names)
        a = C.c_void_p()
        assert c.lib.rls_cg_create(c.op.handle, c.ptr("cu"), c.ptr("cr"), c.ptr("cc"), C.byref(c.plan)) == 0
        try:
            assert c.path(c.lib.rls_cg_path) == 0
            assert c.lib.rls_admm_create(c.plan, C.byref(a)) == 0
            p = _lib.AdmmParams()
            for k in ("x", "xold", "beta", "beta_y", "z0", "z1", "u"):
                setattr(p, k, c.ptr(k))
            p.rho, p.sigma_abs, p.rel_tol, p.iterations, p.iterations_cg, p.tol_inner = f(rho), 0.0, f(rel_tol), 3, 2, 0.0
            p.reg_kind, p.prox_lambda, p.proj_kind = R.REG_L1, f(lam), R.PROJ_NONE
            assert c.lib.rls_admm_init(a, C.byref(p)) == 0
            st, log = _lib.AdmmStatus(), (C.c_float * 8)()
            assert c.lib.rls_admm_step_status(a, 1, C.byref(st), log, 1) == 0
            first, rec = c.read(), fields(st)
            assert c.lib.rls_admm_step_status(a, 1, C.byref(st), log, 1) == 0
            return first, rec, c.read(), fields(st)
        finally:
            if a:
                assert c.lib.rls_admm_destroy(a) == 0
            assert c.lib.rls_cg_destroy(c.plan) == 0

    with unfused(ctx):
        v0, r0, _, s0 = run(0.0)
        assert (r0["iteration"], r0["done"], s0["iteration"]) == (1, 0, 2)
        q = max(r0["rk"] / r0["eps_pri"], r0["sk"] / r0["eps_dua"])
        for rel_tol, done in ((np.float32(q * (1 + 2e-3)), 1), (np.float32(q * (1 - 2e-3)), 0)):
            v1, r1, v2, s1 = run(rel_tol)
            assert all(v1[k].tobytes() == v0[k].tobytes() for k in v0), "run to run"
            want = R.admm_converged(r1["rk"], r1["sk"], r1["eps_pri"], r1["eps_dua"], 0.0, rel_tol)
            assert (r1["iteration"], r1["done"]) == (1, int(want)) == (1, done), (rel_tol, q, r1)
            if done:   # the step behind it moved nothing
                assert all(v2[k].tobytes() == v1[k].tobytes() for k in v1) and s1 == r1
            else:
                assert s1["iteration"] == 2


# ---- refusals of the cg! entry points -----------------------------------------------------------------------------------------------------------
def test_cg_refusals(rls, ctx):
    c = Case(rls, ctx, np.complex64, 65, ("x", "b", "u", "r", "c"))
    before, lib, out = c.read(), c.lib, C.c_void_p()
    assert lib.rls_cg_create(None, c.ptr("u"), c.ptr("r"), c.ptr("c"), C.byref(out)) == INVALID
    for miss in range(3):
        a = [c.ptr(k) if i != miss else None for i, k in enumerate(("u", "r", "c"))]
        assert lib.rls_cg_create(c.op.handle, *a, C.byref(out)) == INVALID
    assert lib.rls_cg_create(c.op.handle, c.ptr("u"), c.ptr("r"), c.ptr("c"), None) == INVALID
    assert lib.rls_cg_create_batched(c.op.handle, 0, c.ptr("u"), c.ptr("r"), c.ptr("c"), 65, C.byref(out)) == INVALID
    assert lib.rls_cg_create_batched(c.op.handle, 1, c.ptr("u"), c.ptr("r"), c.ptr("c"), 64, C.byref(out)) == INVALID   # ldv < N
    assert lib.rls_cg_create(c.op.handle, c.ptr("u"), c.ptr("r"), c.ptr("c"), C.byref(c.plan)) == 0
    try:
        assert lib.rls_cg_solve(None, c.ptr("x"), c.ptr("b"), 0.3, 1, 0.0) == INVALID
        assert lib.rls_cg_solve(c.plan, None, c.ptr("b"), 0.3, 1, 0.0) == INVALID
        assert lib.rls_cg_solve(c.plan, c.ptr("x"), None, 0.3, 1, 0.0) == INVALID
        assert lib.rls_cg_solve(c.plan, c.ptr("x"), c.ptr("b"), 0.3, -1, 0.0) == INVALID
        assert lib.rls_cg_local_start(c.plan, c.ptr("x"), c.ptr("b"), 0.3, -1, 0.0) == INVALID
        assert lib.rls_cg_local_update(c.plan, None) == INVALID
        assert lib.rls_cg_path(None, C.byref(C.c_int32())) == INVALID and lib.rls_cg_path(c.plan, None) == INVALID
    finally:
        assert lib.rls_cg_destroy(c.plan) == 0
    after = c.read()
    assert all(after[k].tobytes() == before[k].tobytes() for k in before)


# ---- the K-column plan: dim3(K) launches and the Bregman start --------------------------------------------------------------------------------
MB, NB, KB, LDV, LEAD_B = 16, 1040, 3, 1048, 8


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
def test_batched_admm_and_bregman_columns(rls, ctx, dt):
    """two rls_admm_step(a, 1) of a K = 3 plan in Bregman mode with blocks of one inner iteration: the first starts with cg_start_kernel,
    the second with cg_start_bregman_kernel; iterations_cg = 1, so CU still holds the start's r (= u) and CC the update's c afterwards.
    Every column against its own restatement, the rows between N and ldv byte for byte"""
    from rls_amd import _lib
    names = ("X", "XOLD", "BETA", "BETA_Y", "Z0", "Z1", "U", "CU", "CR", "CC", "Y")
    rho, plam = np.float32(0.3), np.float32(0.05)
    A, _ = R.problem(dt, NB, 0, MB)
    Ad = rls.DeviceMatrix.from_host(A, ctx)
    op = rls.OperatorHandle(Ad)
    g = {k: Guarded(rls, ctx, dt, LDV * KB, body=P.vector(dt, LDV * KB, 400 + i), lead=LEAD_B) for i, k in enumerate(names)}
    lib, cg, a = ctx.lib, C.c_void_p(), C.c_void_p()

    def read():
        ctx.sync()
        return {k: v.read().copy() for k, v in g.items()}

    def col(h, k, j):
        return h[k][j * LDV: j * LDV + NB]

    def pads(h):
        return b"".join(h[k][j * LDV + NB: (j + 1) * LDV].tobytes() for k in names for j in range(KB))

    assert lib.rls_cg_create_batched(op.handle, KB, g["CU"].ptr, g["CR"].ptr, g["CC"].ptr, LDV, C.byref(cg)) == 0
    try:
        path = C.c_int32(-1)
        assert lib.rls_cg_path(cg, C.byref(path)) == 0 and path.value == 3, "not the batched matrix-core path"
        assert lib.rls_admm_create(cg, C.byref(a)) == 0
        p = _lib.AdmmParams()
        for k, q in (("x", "X"), ("xold", "XOLD"), ("beta", "BETA"), ("beta_y", "BETA_Y"), ("z0", "Z0"), ("z1", "Z1"), ("u", "U")):
            setattr(p, k, g[q].ptr)
        p.rho, p.sigma_abs, p.rel_tol, p.iterations, p.iterations_cg, p.tol_inner = f(rho), 0.0, 0.0, 3, 1, 0.0
        p.reg_kind, p.prox_lambda, p.proj_kind = R.REG_L1, f(plam), R.PROJ_NONE
        assert lib.rls_admm_init(a, C.byref(p)) == 0
        assert lib.rls_admm_set_bregman(a, 1, g["Y"].ptr, LDV) == 0
        cur = read()
        pad0 = pads(cur)
        for step, (zc_, zn_) in enumerate((("Z0", "Z1"), ("Z1", "Z0"))):
            bregman = step == 1
            assert lib.rls_admm_step(a, 1) == 0
            st = (_lib.AdmmStatus * KB)()
            assert lib.rls_admm_get_status_batched(a, st, None, 0) == 0
            nxt = read()
            assert pads(nxt) == pad0, "rows between N and ldv were written"
            assert nxt["Y"].tobytes() == cur["Y"].tobytes()
            for j in range(KB):
                case, gname = f"step {step + 1} column {j}", name(dt)
                start = ("cg_start_bregman_kernel" if bregman else "cg_start_kernel dim3(K)") + " " + gname
                x0 = col(cur, "X", j)
                cvx, Gx = R.product_gate(A, x0)
                assert col(nxt, "XOLD", j).tobytes() == x0.tobytes(), (case, "xold")
                beta_dev, r0 = col(nxt, "BETA", j), col(nxt, "CU", j)
                if bregman:
                    by, y = col(cur, "BETA_Y", j), col(cur, "Y", j)
                    w = R.cg_start_bregman(x0, y, cvx, by, rho)
                    gb = R.cg_start_bregman_gates(x0, y, cvx, by, rho)
                    by_dev = col(nxt, "BETA_Y", j)
                    held(f"{start} beta_y", case, err(by_dev, w["beta_y"]), gb["beta_y"] + Gx)
                    assert col(nxt, zc_, j).tobytes() == x0.tobytes(), (case, "z = x")
                    held(f"{start} beta", case, err(beta_dev, R.c64(by_dev) + float(rho) * R.c64(x0)),
                         R.gam(2) * (R._mag(by_dev) + float(rho) * R._mag(x0)))
                    zc, u_in = x0, np.zeros_like(x0)
                else:
                    fuse = (col(cur, "BETA_Y", j), col(cur, zc_, j), col(cur, "U", j), rho)
                    w = R.cg_start(x0, None, cvx, rho, 0.0, 1, fuse=fuse)
                    held(f"{start} beta", case, err(beta_dev, w["beta"]), R.cg_start_gates(x0, None, cvx, rho, fuse=fuse)["beta"])
                    assert col(nxt, "BETA_Y", j).tobytes() == col(cur, "BETA_Y", j).tobytes()
                    assert col(nxt, zc_, j).tobytes() == col(cur, zc_, j).tobytes()
                    zc, u_in = col(cur, zc_, j), col(cur, "U", j)
                # r = beta - (AHA x + rho x) from the beta that came back; still in CU: the one update was the last, u stayed
                r_want = R.c64(beta_dev) - (cvx + float(rho) * R.c64(x0))
                held(f"{start} r", case, err(r0, r_want), R.gam(3) * (R._mag(beta_dev) + np.abs(cvx) + float(rho) * R._mag(x0)) + Gx)
                # the update: c = AHA u + rho u, then alpha, x, r from the c and r that came back
                cvu, Gu = R.product_gate(A, r0)
                c_dev, r1, x1 = col(nxt, "CC", j), col(nxt, "CR", j), col(nxt, "X", j)
                upd = f"cg_update_kernel dim3(K) {gname}"
                held(f"{upd} c", case, err(c_dev, cvu + float(rho) * R.c64(r0)), R.gam(2) * (np.abs(cvu) + float(rho) * R._mag(r0)) + Gu)
                residual = P.norm_gate(r0)[0]
                wu = R.cg_update(x0, r0, r0, cvu, residual, rho, 0.0, 0, 1, r_dev=r1, c_dev=c_dev)
                gu = R.cg_update_gates(x0, r0, r0, cvu, rho, wu, r1, c_dev)
                held(f"{upd} x", case, err(x1, wu["x"]), gu["x"])
                held(f"{upd} r", case, err(r1, wu["r"]), gu["r"])
                assert wu["done"] == 1
                # admm_zu_kernel from the x that came back
                zn, un = col(nxt, zn_, j), col(nxt, "U", j)
                z = R.admm_zu(x1, None, u_in, R.REG_L1, plam, R.PROJ_NONE, z_dev=zn)
                zu = f"admm_zu_kernel dim3(K) {gname}"
                held(f"{zu} z", case, err(zn, z["z"]), R.admm_zu_gates(x1, u_in, R.REG_L1)["z"])
                held(f"{zu} u", case, err(un, z["u"]), R.admm_u_gate(x1, zn, u_in)["u"])
                norms = R.admm_norms(x1, col(nxt, "XOLD", j), zn, zc, u_in, un)
                (dx, bdx), (dz, bdz), (du, bdu), (nx, bnx), (nz, bnz), (nxz, bnxz), (nu, bnu) = norms
                r_, s_ = float(rho), st[j]
                held(f"{zu} norms", case,
                     [abs(s_.delta - (dx + dz + du)), abs(s_.sk - r_ * dz), abs(s_.eps_pri - max(nx, nz)), abs(s_.rk - nxz),
                      abs(s_.eps_dua - r_ * nu)],
                     [bdx + bdz + bdu + 2 * R.U * (dx + dz + du), r_ * bdz + R.U * r_ * dz, max(bnx, bnz), bnxz, r_ * bnu + R.U * r_ * nu])
                want_done = int(R.admm_converged(s_.rk, s_.sk, s_.eps_pri, s_.eps_dua, 0.0, 0.0) or step + 1 >= 3)
                assert (s_.iteration, s_.done, s_.cg_iterations) == (step + 1, want_done, 1) and want_done == 0, (case, s_.iteration, s_.done)
            cur = nxt
    finally:
        if a:
            assert lib.rls_admm_destroy(a) == 0
        if cg:
            assert lib.rls_cg_destroy(cg) == 0
