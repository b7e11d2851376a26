"""The OptISTA / POGM update kernels of csrc/pgm.hip one launch at a time, against tests/pgm_ref.py (anchored to the oracle and
held to its own gates in tests/test_pgm_ref.py; the gates and their derivation: the docstring of pgm_ref.py).

Part A  the 1024-thread single-workgroup kernels through the C ABI -- rls_optista_update, rls_pogm_update (restart 0 / 1), their
        _async forms and rls_pogm_update_auto -- on guarded device vectors: Float32 and ComplexF32, n on either side of a wave, of
        one pass of the loop and at five passes, every reg_kind x proj_kind at n = 1025, every output vector and scalar, the
        device record (iteration, done, ||res||, theta, theta_old, sigma, gamma), the no-op-once-done rule, the last-iteration
        theta rule, the restart decision, and the refusals.
Part B  pgmb_update_kernel<E, KIND, EPT> through solve_(S, B, scheduler=BatchedState): N walks the dispatch of
        pgmb_launch_update_typed (EPT = 1 / 2 / 4, full tiles and clamped tails, the strided loop past 4096), every column against
        its float64 oracle column, and the register form against the strided form (pgm_batched_reg = 0) bit for bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pgm_ref as P  # noqa: E402
import rls_oracle as O  # noqa: E402
from conftest import parity_check  # noqa: E402
from test_gpu_f64_plan_products import GUARD, Guarded, _report, held  # noqa: E402,F401
from test_gpu_pgm_batched import VARIANTS, batched, hi, make, oracle_column, problem, reg_kind_of, regs  # noqa: E402

pytestmark = pytest.mark.gpu
DT = [np.float32, np.complex64]
DT_IDS = ["float32", "complex64"]
INVALID = -1
OPT_IN, OPT_OUT = ("res", "x0", "x", "y", "z"), ("res", "x", "y", "z", "zold")
POGM_IN, POGM_OUT = ("res", "x0", "xbuf", "ybuf", "z", "w"), ("res", "xbuf", "ybuf", "z", "xold", "w")


def f(x):
    return float(np.float32(x))


def kinds_at(n, pogm):
    """the full cross at n = 1025, L1 (+ Positive for POGM) elsewhere"""
    if n != P.FULL_CROSS_N:
        return [(P.REG_L1, P.PROJ_POSITIVE)] if pogm else [(P.REG_L1, None)]
    kinds = (P.REG_NONE, P.REG_L1, P.REG_L2)
    return [(r, p) for r in kinds for p in (P.PROJ_NONE, P.PROJ_REAL, P.PROJ_POSITIVE)] if pogm else [(r, None) for r in kinds]


class Vectors:
    """guarded device copies (a sentinel zone in front of and behind each) of the vectors of one case; `old`: the copy target
    (zold / xold), prefilled with other numbers"""

    def __init__(self, rls, ctx, dt, v, old):
        self.n = len(v["res"])
        self.host = dict(v)
        self.host[old] = P.vector(dt, self.n, 991)
        self.dev = {k: Guarded(rls, ctx, dt, self.n, body=a, lead=GUARD) for k, a in self.host.items() if a is not None}

    def ptr(self, name):
        return self.dev[name].ptr if name in self.dev else None

    def read(self):
        return {k: g.read() for k, g in self.dev.items()}

    def untouched(self, got, names):
        for k in names:
            assert got[k].tobytes() == self.host[k].tobytes(), f"{k} was written"


def record(rls, ctx, words, init=()):
    h0 = np.zeros(words, np.float32)
    h0[4:4 + len(init)] = init
    return Guarded(rls, ctx, np.float32, words, body=h0, lead=GUARD)


def read_record(rec):
    raw = rec.read()
    return {"iteration": int(raw[:1].view(np.int32)[0]), "done": int(raw[1:2].view(np.int32)[0]), "res_norm": raw[2], "raw": raw.copy()}


def optista_launch(ctx, V, c, state=None, norm_x0=1.0, rel_tol=0.0, n=None, code=None):
    a = (ctx.handle, V.code if code is None else code, V.n if n is None else n, V.ptr("res"), V.ptr("x0"), V.ptr("x"), V.ptr("y"),
         V.ptr("z"), V.ptr("zold"), f(c["step"]), int(c["reg_kind"]), f(c["thr"]), f(c["c_z"]), f(c["c_y"]), f(c["c_x"]), f(c["c_zn"]),
         f(c["c_zo"]))
    if state is None:
        out = (C.c_float * 1)()
        return ctx.lib.rls_optista_update(*a, out), np.float32(out[0])
    return ctx.lib.rls_optista_update_async(*a, f(norm_x0), f(rel_tol), state), None


def pogm_launch(ctx, V, c, state=None, norm_x0=1.0, rel_tol=0.0, n=None, w="w"):
    a = (ctx.handle, V.code, V.n if n is None else n, V.ptr("res"), V.ptr("x0"), V.ptr("xbuf"), V.ptr("ybuf"), V.ptr("xold"), V.ptr("z"))
    s = (f(c["rho"]), f(c["c_y"]), f(c["c_x1"]), f(c["c_xo"]), f(c["c_z"]), int(c["reg_kind"]), f(c["thr"]), int(c["proj_kind"]))
    if state is None:
        out = (C.c_float * 4)()
        rc = ctx.lib.rls_pogm_update(*a, V.ptr(w) if w else None, *s, int(c["restart"]), f(c["rg"]), out)
        return rc, np.array(out[:], np.float32)
    return ctx.lib.rls_pogm_update_async(*a, *s, f(norm_x0), f(rel_tol), state), None


def upload(rls, ctx, dt, v, old):
    V = Vectors(rls, ctx, dt, v, old)
    V.code = rls.DeviceVector(1, dt, ctx).code
    return V


def judge_optista(case, v, c, got, res_norm):
    a = [v[k] for k in OPT_IN]
    want = P.optista_step(*a, *P.optista_args(c))
    P.check_vectors(held, "optista_update_kernel " + np.dtype(got["x"].dtype).name, case, got, want, P.optista_gates(*a, *P.optista_args(c)),
                    exact=("zold",))
    w_, b_ = P.norm_gate(got["res"])
    held(f"optista_update_kernel {np.dtype(got['x'].dtype).name} ||res||", case, [abs(float(res_norm) - w_)], [b_])


def judge_pogm(group, case, v, c, got, sums):
    a = [v[k] for k in POGM_IN]
    want = P.pogm_step(*a, *P.pogm_args(c))
    gates = P.pogm_gates(*a[:5], c["rho"], c["c_y"], c["c_x1"], c["c_xo"], c["c_z"], c["reg_kind"], c["thr"], c["proj_kind"], c["rg"])
    group = f"{group} {np.dtype(got['z'].dtype).name}"
    P.check_vectors(held, group, case, got, want, gates, exact=("xold",))
    w_, b_ = P.norm_gate(got["res"])
    held(f"{group} ||res||", case, [abs(float(sums[0]) - w_)], [b_])
    if c["restart"] and len(sums) > 1:
        for i, (name, (w_, b_)) in enumerate(P.dot_gates(v["w"], got, c["rg"]).items()):
            held(f"{group} {name}", case, [abs(float(sums[1 + i]) - w_)], [b_])


# ---- part A: rls_optista_update, rls_pogm_update -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("n", P.LENGTHS)
def test_optista_update(rls, ctx, dt, n):
    for reg, _ in kinds_at(n, False):
        v, c = P.optista_case(dt, n, reg)
        V = upload(rls, ctx, dt, v, "zold")
        rc, rn = optista_launch(ctx, V, c)
        assert rc == 0
        got = V.read()
        V.untouched(got, ("x0",))
        judge_optista(f"n={n} reg={reg}", v, c, got, rn)


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("restart", [0, 1], ids=["restart0", "restart1"])
@pytest.mark.parametrize("n", P.LENGTHS)
def test_pogm_update(rls, ctx, dt, n, restart):
    for reg, proj in kinds_at(n, True):
        v, c = P.pogm_case(dt, n, reg, proj, bool(restart))
        V = upload(rls, ctx, dt, v, "xold")
        rc, out = pogm_launch(ctx, V, c)
        assert rc == 0
        got = V.read()
        V.untouched(got, ("x0",) if restart else ("x0", "w"))
        if not restart:
            got["w"] = None
        judge_pogm(f"pogm_update_kernel<{restart}>", f"n={n} reg={reg} proj={proj}", v, c, got, out)


# ---- part A: the deferred forms and their record ------------------------------------------------------------------------------------------
def tolerances(res_norm, norm_x0):
    """rel_tol on either side of ||res|| / norm_x0, 2e-3 relative away: (rel_tol, done)"""
    q = float(res_norm) / float(np.float32(norm_x0))
    out = [(np.float32(q * (1 + 2e-3)), 1), (np.float32(q * (1 - 2e-3)), 0)]
    for t, done in out:
        assert abs(float(t) - q) >= 1e-3 * q and (q < float(t)) == bool(done)
    return out


def same_bits(a, b, names):
    for k in names:
        if a.get(k) is not None:
            assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("n", P.LENGTHS)
def test_optista_update_async_and_its_record(rls, ctx, dt, n):
    for reg, _ in kinds_at(n, False):
        v, c = P.optista_case(dt, n, reg)
        S = upload(rls, ctx, dt, v, "zold")
        rc, rn = optista_launch(ctx, S, c)          # the launch test_optista_update gates: out[0] and every vector
        assert rc == 0
        sync = S.read()
        judge_optista(f"async n={n} reg={reg}", v, c, sync, rn)
        norm_x0 = np.float32(np.linalg.norm(v["x0"].astype(hi(dt))))
        other = dict(c, c_zn=c["c_zo"], c_zo=c["c_zn"], step=c["c_y"])
        for rel_tol, done in tolerances(rn, norm_x0):
            V = upload(rls, ctx, dt, v, "zold")
            rec = record(rls, ctx, 4)
            assert optista_launch(ctx, V, c, rec.ptr, norm_x0, rel_tol)[0] == 0
            got, r1 = V.read(), read_record(rec)
            same_bits(got, sync, OPT_OUT + ("x0",))
            assert (r1["iteration"], r1["done"]) == (1, done), (r1, rel_tol)
            assert r1["res_norm"].tobytes() == rn.tobytes()
            assert optista_launch(ctx, V, other, rec.ptr, norm_x0, rel_tol)[0] == 0   # other coefficients
            again, r2 = V.read(), read_record(rec)
            if done:   # a no-op: nothing moves
                same_bits(again, got, OPT_OUT + ("x0",))
                assert r2["raw"].tobytes() == r1["raw"].tobytes()
            else:
                assert r2["iteration"] == 2 and again["x"].tobytes() != got["x"].tobytes()


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("n", P.LENGTHS)
def test_pogm_update_async_and_its_record(rls, ctx, dt, n):
    names = tuple(k for k in POGM_OUT if k != "w") + ("x0",)
    for reg, proj in kinds_at(n, True):
        v, c = P.pogm_case(dt, n, reg, proj, False, solver="POGM")
        v = dict(v, w=None)
        S = upload(rls, ctx, dt, v, "xold")
        rc, out = pogm_launch(ctx, S, c, w=None)
        assert rc == 0
        sync = S.read()
        judge_pogm("pogm_update_kernel<0>", f"async n={n} reg={reg} proj={proj}", dict(v, w=np.zeros(n, dt)), c, dict(sync, w=None), out)
        norm_x0 = np.float32(np.linalg.norm(v["x0"].astype(hi(dt))))
        other = dict(c, c_y=c["c_x1"], c_x1=c["c_y"], rho=c["c_z"])
        for rel_tol, done in tolerances(out[0], norm_x0):
            V = upload(rls, ctx, dt, v, "xold")
            rec = record(rls, ctx, 4)
            assert pogm_launch(ctx, V, c, rec.ptr, norm_x0, rel_tol)[0] == 0
            got, r1 = V.read(), read_record(rec)
            same_bits(got, sync, names)
            assert (r1["iteration"], r1["done"]) == (1, done), (r1, rel_tol)
            assert r1["res_norm"].tobytes() == out[:1].tobytes()
            assert pogm_launch(ctx, V, other, rec.ptr, norm_x0, rel_tol)[0] == 0
            again, r2 = V.read(), read_record(rec)
            if done:
                same_bits(again, got, names)
                assert r2["raw"].tobytes() == r1["raw"].tobytes()
            else:
                assert r2["iteration"] == 2 and again["ybuf"].tobytes() != got["ybuf"].tobytes()


# ---- part A: rls_pogm_update_auto -----------------------------------------------------------------------------------------------------------
def auto_launch(ctx, V, s, sigma_fac, iterations, reg, proj, norm_x0, rel_tol, state, xb="xbuf", yb="ybuf", n=None, w="w"):
    return ctx.lib.rls_pogm_update_auto(ctx.handle, V.code, V.n if n is None else n, V.ptr("res"), V.ptr("x0"), V.ptr(xb), V.ptr(yb),
                                        V.ptr("xold"), V.ptr("z"), V.ptr(w) if w else None, f(s["rho"]), f(s["lam"]), f(sigma_fac),
                                        int(iterations), int(reg), int(proj), f(norm_x0), f(rel_tol), state)


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("force", ["restart", "no-restart"])
@pytest.mark.parametrize("n", P.LENGTHS)
def test_pogm_update_auto_three_launches(rls, ctx, dt, n, force):
    """iterations = 3: the third launch takes the 8 theta^2 rule.  Before every launch res (a fresh AHA x) and w are written by the
    test; w = -/+ alpha d with d = (x - z) / gamma - res from the float64 step, alpha large enough that the float64 criterion
    <w', d> is negative / positive by at least 1e-3 of |<w', x>| / gamma + |<w', z>| / gamma + |<w', res>|."""
    sigma_fac = np.float32(0.96)
    for reg, proj in kinds_at(n, True):
        s = P.iteration3("POGM-restart", dt)
        v, _ = P.pogm_case(dt, n, reg, proj, True)
        V = upload(rls, ctx, dt, v, "xold")
        rec = record(rls, ctx, 8, init=[s["theta"], s["theta"], s["sigma"], s["gamma"]])
        th, sg, gm = s["theta"], s["sigma"], s["gamma"]
        xb, yb = "xbuf", "ybuf"
        cur = {k: v[k].copy() for k in POGM_IN}
        for k in range(3):
            c = P.pogm_auto_coefs(th, sg, gm, k == 2, s["rho"], s["lam"])
            c = dict({q: np.float32(c[q]) for q in ("theta", "gamma", "rho", "c_y", "c_x1", "c_xo", "c_z", "thr", "rg")},
                     reg_kind=reg, proj_kind=proj, restart=1)
            if k:   # a fresh product in res; on the first launch the case's own
                cur["res"] = P.vector(dt, n, 5000 * n + k)
            # w for the decision
            a = [cur[q] for q in POGM_IN]
            w64 = P.pogm_step(*a, *P.pogm_args(c))
            d = (w64["ybuf"] - w64["z"]) / float(c["gamma"]) - w64["res"]
            rest = w64["xbuf"] + float(c["rg"]) * (w64["ybuf"] - w64["z"])
            dd = float(P.redot(d, d))
            assert dd > 0
            alpha = 4.0 * abs(float(P.redot(rest, d))) / dd + 1.0
            cur["w"] = ((-alpha if force == "restart" else alpha) * d).astype(dt)
            a = [cur[q] for q in POGM_IN]
            w64 = P.pogm_step(*a, *P.pogm_args(c))
            crit = (float(w64["dwx"]) - float(w64["dwz"])) / float(c["gamma"]) - float(w64["dwr"])
            scale = (abs(float(w64["dwx"])) + abs(float(w64["dwz"]))) / float(c["gamma"]) + abs(float(w64["dwr"]))
            assert (crit < 0) == (force == "restart") and abs(crit) >= 1e-3 * scale, (k, crit, scale)
            V.dev["res"] = Guarded(rls, ctx, dt, n, body=cur["res"], lead=GUARD)
            V.dev["w"] = Guarded(rls, ctx, dt, n, body=cur["w"], lead=GUARD)
            norm_x0, rel_tol = np.float32(1.0), np.float32(0.0)
            assert auto_launch(ctx, V, s, sigma_fac, 3, reg, proj, norm_x0, rel_tol, rec.ptr, xb, yb) == 0
            raw = V.read()
            got = {"res": raw["res"], "xbuf": raw[xb], "ybuf": raw[yb], "z": raw["z"], "xold": raw["xold"], "w": raw["w"]}
            assert raw["x0"].tobytes() == v["x0"].tobytes()
            r = read_record(rec)
            case = f"launch {k} n={n} reg={reg} proj={proj} {force}"
            judge_pogm("pogm_auto_kernel", case, cur, c, got, [r["res_norm"]])
            # the record: one rounding per operation, as NumPy's Float32 scalars
            want = P.pogm_auto_record(th, sg, sigma_fac, c, force == "restart")
            assert r["iteration"] == k + 1 and r["done"] == 0, r
            assert r["raw"][4:8].tobytes() == np.array(want, np.float32).tobytes(), (case, r["raw"][4:8], want)
            if force == "restart":
                assert r["raw"][4] == 1 and r["raw"][6] == 1
            # the same data and coefficients through rls_pogm_update, which returns the three dot products the decision was taken
            # from.  (Its vectors are in the same gates, not the same bits: the two kernels inline the body apart and the compiler
            # contracts c_y = -alpha differently -- last-bit differences in z and x.)
            T = upload(rls, ctx, dt, cur, "xold")
            rc, out = pogm_launch(ctx, T, c)
            assert rc == 0
            judge_pogm("pogm_update_kernel<1>", "twin of " + case, cur, c, T.read(), out)
            assert P.pogm_restart(c["gamma"], *out[1:])[0] == (force == "restart")
            # the next launch: the buffers swap roles (the new x is in the old y buffer)
            th, _, sg, gm = want
            cur.update(xbuf=got["ybuf"], ybuf=got["xbuf"], z=got["z"])
            xb, yb = yb, xb
        # done: rel_tol above ||res|| / norm_x0 on a fourth launch stops the sequence; a fifth is a no-op
        V.dev["res"] = Guarded(rls, ctx, dt, n, body=P.vector(dt, n, 77), lead=GUARD)
        assert auto_launch(ctx, V, s, sigma_fac, 8, reg, proj, 1.0, 1e30, rec.ptr, xb, yb) == 0
        r4, v4 = read_record(rec), V.read()
        assert (r4["iteration"], r4["done"]) == (4, 1), r4
        assert auto_launch(ctx, V, dict(s, rho=np.float32(0.5)), sigma_fac, 8, reg, proj, 1.0, 1e30, rec.ptr, yb, xb) == 0
        r5, v5 = read_record(rec), V.read()
        assert r5["raw"].tobytes() == r4["raw"].tobytes()
        same_bits(v5, v4, tuple(v4))


# ---- part A: refusals -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
def test_bad_arguments_launch_nothing(rls, ctx, dt):
    n = 65
    vo, co = P.optista_case(dt, n)
    vp, cp = P.pogm_case(dt, n)
    s = P.iteration3("POGM-restart", dt)
    Vo, Vp = upload(rls, ctx, dt, vo, "zold"), upload(rls, ctx, dt, vp, "xold")
    rec4, rec8 = record(rls, ctx, 4), record(rls, ctx, 8, init=[1, 1, 1, 1])
    calls = [
        lambda: optista_launch(ctx, Vo, co, n=0)[0],
        lambda: optista_launch(ctx, Vo, dict(co, reg_kind=3))[0],
        lambda: optista_launch(ctx, Vo, dict(co, reg_kind=-1))[0],
        lambda: optista_launch(ctx, Vo, co, rec4.ptr, n=0)[0],
        lambda: optista_launch(ctx, Vo, dict(co, reg_kind=3), rec4.ptr)[0],
        lambda: ctx.lib.rls_optista_update_async(ctx.handle, Vo.code, n, Vo.ptr("res"), Vo.ptr("x0"), Vo.ptr("x"), Vo.ptr("y"), Vo.ptr("z"),
                                                 Vo.ptr("zold"), *[f(x) if i != 1 else int(x) for i, x in enumerate(P.optista_args(co))],
                                                 1.0, 0.0, None),
        lambda: pogm_launch(ctx, Vp, cp, n=0)[0],
        lambda: pogm_launch(ctx, Vp, dict(cp, reg_kind=3))[0],
        lambda: pogm_launch(ctx, Vp, dict(cp, reg_kind=-1))[0],
        lambda: pogm_launch(ctx, Vp, dict(cp, proj_kind=3))[0],
        lambda: pogm_launch(ctx, Vp, dict(cp, restart=1), w=None)[0],
        lambda: pogm_launch(ctx, Vp, dict(cp, restart=0), rec4.ptr, n=0)[0],
        lambda: pogm_launch(ctx, Vp, dict(cp, restart=0, proj_kind=3), rec4.ptr)[0],
        lambda: ctx.lib.rls_pogm_update_async(ctx.handle, Vp.code, n, Vp.ptr("res"), Vp.ptr("x0"), Vp.ptr("xbuf"), Vp.ptr("ybuf"), Vp.ptr("xold"),
                                              Vp.ptr("z"), f(cp["rho"]), f(cp["c_y"]), f(cp["c_x1"]), f(cp["c_xo"]), f(cp["c_z"]), P.REG_L1,
                                              f(cp["thr"]), P.PROJ_NONE, 1.0, 0.0, None),
        lambda: auto_launch(ctx, Vp, s, 0.96, 3, P.REG_L1, P.PROJ_NONE, 1.0, 0.0, rec8.ptr, n=0),
        lambda: auto_launch(ctx, Vp, s, 0.96, 3, 3, P.PROJ_NONE, 1.0, 0.0, rec8.ptr),
        lambda: auto_launch(ctx, Vp, s, 0.96, 3, -1, P.PROJ_NONE, 1.0, 0.0, rec8.ptr),
        lambda: auto_launch(ctx, Vp, s, 0.96, 3, P.REG_L1, 3, 1.0, 0.0, rec8.ptr),
        lambda: auto_launch(ctx, Vp, s, 0.96, 3, P.REG_L1, P.PROJ_NONE, 1.0, 0.0, rec8.ptr, w=None),
        lambda: auto_launch(ctx, Vp, s, 0.96, 3, P.REG_L1, P.PROJ_NONE, 1.0, 0.0, None),
    ]
    for i, call in enumerate(calls):
        assert call() == INVALID, i
    ctx.sync()
    for V in (Vo, Vp):
        got = V.read()
        for k, a in V.host.items():
            assert got[k].tobytes() == a.tobytes(), k
    assert not rec4.read().any() and rec8.read().tobytes() == rec8.host0[GUARD:GUARD + 8].tobytes()


# ---- part B: the batched kernel at every EPT and tail ------------------------------------------------------------------------------------------
M_B, K_B, ITERS_B = 32, 3, 6
# N -> the instantiation pgmb_launch_update_typed takes with pgm_batched_reg = 1 (16-aligned: the matrix-core products)
N_B = [(1008, "EPT1-idle-threads"), (1024, "last-EPT1"), (1040, "EPT2-clamped"), (2064, "EPT4-tail-in-third-slot"), (4096, "last-EPT4"),
       (4112, "EPT1-five-passes-tail")]
BITS = {}   # (variant, dtype, N) -> "equal"


def record_of(s_):
    return (s_.iteration, s_.done, s_.res_norm, s_.rel_res_norm, s_.norm_x0, s_.theta, s_.theta_old, s_.sigma, s_.gamma)


def solve_both_forms(rls, ctx, name, kw, Ad, Bd, reg, rho, relTol):
    """(X, status) with the strided loop, then with the register tiles: the tune value restored whatever happens"""
    out = []
    try:
        for form in (0, 1):
            ctx.tune(pgm_batched_reg=form)
            S = make(rls, name, kw, Ad, reg(), rho, relTol, iters=ITERS_B)
            X = batched(rls, S, Bd)
            out.append((X, S.state.status()))
    finally:
        ctx.tune(pgm_batched_reg=1)
    return out


def against_oracle(tag, name, kw, dt, A, B, kind, lam, rho, relTol, X, stat):
    its = []
    for j in range(B.shape[1]):
        H = hi(dt)
        ref, _ = oracle_column(name, kw, A.astype(H), B[:, j].astype(H), regs(O, kind, lam, name), rho, relTol, iters=ITERS_B)
        memo = {}

        def f32():
            if "s" not in memo:
                memo["s"] = oracle_column(name, kw, A, np.ascontiguousarray(B[:, j]), regs(O, kind, lam, name), rho, 0.0, iters=ref.iteration)[0]
            return memo["s"]

        assert stat[j].iteration == ref.iteration and stat[j].done, (j, stat[j].iteration, ref.iteration)
        parity_check(f"{tag}_col{j}", X[:, j], ref.x, lambda: f32().x, record=(j == 0))
        # res = AHA x - x0 is the difference of two vectors of the size of x0 (here 0.2 .. 6 % of it is left after six iterations):
        # its error is that of AHA x, so ||res|| is judged on the scale of ||x0|| -- the scale of the stopping test, which compares
        # ||res|| / ||x0|| -- as conftest's `scale` is there for
        parity_check(f"{tag}_col{j}_res_norm", np.array([stat[j].res_norm]), np.array([float(ref.rel_res_norm) * float(ref.norm_x0)]),
                     lambda: np.array([float(f32().rel_res_norm) * float(f32().norm_x0)]), record=False, scale=float(ref.norm_x0))
        if kw:
            parity_check(f"{tag}_col{j}_theta_sigma_gamma", np.array([stat[j].theta, stat[j].sigma, stat[j].gamma]),
                         np.array([ref.theta, ref.sigma, ref.gamma], dtype=np.float64),
                         lambda: np.array([f32().theta, f32().sigma, f32().gamma], dtype=np.float64), record=False)
        its.append(ref.iteration)
    return its


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("name,kw", VARIANTS, ids=["OptISTA", "POGM", "POGM-restart"])
@pytest.mark.parametrize("N,regime", N_B, ids=[r for _, r in N_B])
def test_batched_update_at_every_tile_form(rls, ctx, name, kw, dt, N, regime):
    A, B, lam, rho = problem(dt, M_B, N, K_B)
    kind = reg_kind_of(dt, "l1", name)
    Ad, Bd = rls.DeviceMatrix.from_host(A), rls.DeviceMatrix.from_host(B)
    (X0, st0), (X1, st1) = solve_both_forms(rls, ctx, name, kw, Ad, Bd, lambda: regs(rls, kind, lam, name), rho, 0.0)
    tag = f"pgm_edges_{name}_{'restart' if kw else 'none'}_{np.dtype(dt).name}_{M_B}x{N}_{regime}"
    assert against_oracle(tag, name, kw, dt, A, B, kind, lam, rho, 0.0, X0, st0) == [ITERS_B] * K_B
    # the per-thread summation order is the element order in both forms: not one bit differs
    assert X1.tobytes() == X0.tobytes(), float(np.abs(X1 - X0).max())
    assert [record_of(s_) for s_ in st1] == [record_of(s_) for s_ in st0]
    BITS[f"{name}{'-restart' if kw else ''} {np.dtype(dt).name} N={N}"] = "equal"
    print(f"pgm_batched_reg 1 against 0, {tag}: X and the status records bit-identical")


@pytest.mark.parametrize("name,kw", VARIANTS, ids=["OptISTA", "POGM", "POGM-restart"])
def test_batched_columns_retire_inside_the_two_element_tile(rls, ctx, name, kw):
    """N = 1040 (EPT = 2, clamped loads), relTol between the columns' residuals so that they retire at different iterations; as in
    test_equals_column_solves no rel_res_norm of the float64 oracle is within 1e-3 relTol of relTol"""
    dt, N = np.complex64, 1040
    A, B, lam, rho = problem(dt, M_B, N, K_B)
    H = hi(dt)
    hist = [oracle_column(name, kw, A.astype(H), B[:, j].astype(H), regs(O, "l1", lam, name), rho, 0.0, iters=ITERS_B)[1] for j in range(K_B)]
    relTol = None
    for k in range(1, ITERS_B - 1):   # between two columns' residuals after iteration k + 1
        vals = sorted(h[k] for h in hist)
        for lo, up in zip(vals, vals[1:]):
            t = float(np.sqrt(lo * up))
            stops = [next((i + 1 for i, r_ in enumerate(h) if r_ < t), ITERS_B) for h in hist]
            if len(set(stops)) > 1 and all(abs(r_ - t) >= 1e-3 * t for h in hist for r_ in h):
                relTol = t
                break
        if relTol is not None:
            break
    assert relTol is not None, hist
    Ad, Bd = rls.DeviceMatrix.from_host(A), rls.DeviceMatrix.from_host(B)
    (X0, st0), (X1, st1) = solve_both_forms(rls, ctx, name, kw, Ad, Bd, lambda: regs(rls, "l1", lam, name), rho, relTol)
    its = against_oracle(f"pgm_edges_retire_{name}_{'restart' if kw else 'none'}", name, kw, dt, A, B, "l1", lam, rho, relTol, X1, st1)
    assert len(set(its)) > 1, its
    assert X1.tobytes() == X0.tobytes() and [record_of(s_) for s_ in st1] == [record_of(s_) for s_ in st0]
