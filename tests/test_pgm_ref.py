"""tests/pgm_ref.py, the checker of the OptISTA / POGM update kernels (csrc/pgm.hip), held to the oracle and to its own gates -- no GPU.

  anchor   O.OptISTA, O.POGM and O.POGM(restart="gradient") on a 24 x 16 problem, five iterations, the state snapshotted after
           each: pgm_ref's step maps every snapshot (res := AHA x) to the next to 1e-13 relative, the scalars (theta, sigma, gamma,
           hence the restart decisions) included; and the Float32 recurrences equal the Float32 oracle's bit for bit.
  gates    on the very inputs of tests/test_gpu_pgm_edges.py, part A: the float32 evaluation of pgm_ref is inside every gate
           against the float64 evaluation (the gates admit a correct Float32 implementation), and each of five planted
           mistakes breaks at least one gate at every length, n = 1 included (the gates would see a wrong kernel)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pgm_ref as P  # noqa: E402
import rls_oracle as O  # noqa: E402

ITERS = 5
F64_L1 = functools.partial(P.prox_l1, eps=np.finfo(np.float64).eps)   # the float64 oracle's prox carries eps(Float64)
VARIANTS = [("OptISTA", {}), ("POGM", {}), ("POGM", {"restart": "gradient", "sigma_fac": 0.96})]
IDS = ["OptISTA", "POGM", "POGM-restart"]


def rel(a, b):
    a, b = np.asarray(a, dtype=np.complex128), np.asarray(b, dtype=np.complex128)
    d = np.linalg.norm(np.atleast_1d(a - b))
    n = np.linalg.norm(np.atleast_1d(b))
    return d / n if n > 0 else d


def run(name, kw, dt, seed=39, lam_rel=0.05):
    """(seed 39: POGM with the gradient restart takes both branches of :224-230 within five iterations, in all four types)"""
    A, _, b = O.make_problem(24, 16, dt, seed)
    hi = np.complex128 if np.dtype(dt).kind == "c" else np.float64
    rho = 0.9 / np.linalg.norm(A.astype(hi), 2) ** 2
    lam = lam_rel * float(np.abs(A.astype(hi).conj().T @ b.astype(hi)).max())
    S = getattr(O, name)(A, reg=O.L1Regularization(lam), rho=rho, iterations=ITERS, relTol=0.0, **kw)
    vecs = ("x", "y", "z", "zold", "res") if name == "OptISTA" else ("x", "y", "z", "xold", "w", "res")
    scal = ("theta", "theta_old", "rel_res_norm") + (() if name == "OptISTA" else ("sigma", "gamma"))
    snaps = []

    def snap(s, it):
        d = {k: getattr(s, k).copy() for k in vecs}
        d.update({k: getattr(s, k) for k in scal})
        snaps.append(d)

    O.solve(S, b, callbacks=snap)
    assert len(snaps) == ITERS + 1
    return S, snaps, lam


@pytest.mark.parametrize("dt", [np.float64, np.complex128], ids=["float64", "complex128"])
@pytest.mark.parametrize("name,kw", VARIANTS, ids=IDS)
def test_step_maps_every_oracle_snapshot_to_the_next(name, kw, dt):
    S, snaps, lam = run(name, kw, dt)
    T = np.float64
    restart = bool(kw)
    restarts = []
    for k in range(ITERS):
        a, b = snaps[k], snaps[k + 1]
        aha = S.AHA.mul(a["x"])
        last = k == ITERS - 1
        if name == "OptISTA":
            c = P.optista_coefs(a["theta"], S.theta_n, last, S.rho, lam, T)
            out = P.optista_step(aha, S.x0, a["x"], a["y"], a["z"], c["step"], P.REG_L1, c["thr"], c["c_z"], c["c_y"], c["c_x"],
                                 c["c_zn"], c["c_zo"], prec=T, l1=F64_L1)
            pairs = [(out[v], b[v]) for v in ("x", "y", "z", "zold", "res")]
            pairs += [(c["theta"], b["theta"]), (T(a["theta"]), b["theta_old"])]
            if last:
                assert rel(c["gamma"], S.gamma) <= 1e-13
        else:
            c = P.pogm_coefs(a["theta"], a["sigma"], a["gamma"], last, S.rho, lam, restart, T)
            out = P.pogm_step(aha, S.x0, a["x"], a["y"], a["z"], a["w"], c["rho"], c["c_y"], c["c_x1"], c["c_xo"], c["c_z"], P.REG_L1,
                              c["thr"], P.PROJ_NONE, restart, c["rg"], prec=T, l1=F64_L1)
            # the reference swaps x and y (:206-208): the new x is in the buffer that held y
            pairs = [(out["ybuf"], b["x"]), (out["xbuf"], b["y"]), (out["z"], b["z"]), (out["xold"], b["xold"]), (out["res"], b["res"])]
            if restart:
                pairs.append((out["w"], b["w"]))
                hit, crit = P.pogm_restart(c["gamma"], out["dwx"], out["dwz"], out["dwr"], T)
                scale = (abs(out["dwx"]) + abs(out["dwz"])) / c["gamma"] + abs(out["dwr"])
                assert abs(crit) > 1e-9 * scale, (k, crit, scale)   # a decision float64 rounding cannot turn
                restarts.append(hit)
                th, tho, sg, gm = P.pogm_auto_record(a["theta"], a["sigma"], S.sigma_fac, c, hit, T)
            else:
                th, tho, sg, gm = c["theta"], T(a["theta"]), T(a["sigma"]), c["gamma"]
            pairs += [(th, b["theta"]), (tho, b["theta_old"]), (sg, b["sigma"]), (gm, b["gamma"])]
        pairs.append((out["res_norm"] / S.norm_x0, b["rel_res_norm"]))
        for i, (got, want) in enumerate(pairs):
            assert rel(got, want) <= 1e-13, (name, k, i, rel(got, want))
    if restart:
        assert any(restarts) and not all(restarts), restarts   # both branches of :224-230 were compared


@pytest.mark.parametrize("dt", [np.float32, np.complex64], ids=["float32", "complex64"])
@pytest.mark.parametrize("name,kw", VARIANTS, ids=IDS)
def test_float32_recurrences_equal_the_float32_oracle_bit_for_bit(name, kw, dt):
    """theta, gamma and (restart) sigma of every iteration, from the oracle's own state before it"""
    S, snaps, lam = run(name, kw, dt)
    f = np.float32
    for k in range(ITERS):
        a, b = snaps[k], snaps[k + 1]
        last = k == ITERS - 1
        if name == "OptISTA":
            c = P.optista_coefs(a["theta"], S.theta_n, last, S.rho, lam)
            assert c["theta"].dtype == f and c["theta"] == b["theta"]
            continue
        c = P.pogm_coefs(a["theta"], a["sigma"], a["gamma"], last, S.rho, lam, bool(kw))
        assert c["gamma"].dtype == f and c["gamma"] == b["gamma"], (k, c["gamma"], b["gamma"])
        if not kw:
            assert c["theta"] == b["theta"]
            continue
        hit = bool(b["theta"] == 1 and b["sigma"] == 1)   # (theta = 1 without a restart: theta_old = 0, which does not occur)
        got = P.pogm_auto_record(a["theta"], a["sigma"], S.sigma_fac, c, hit)
        assert [np.float32(v) for v in got] == [b["theta"], b["theta_old"], b["sigma"], b["gamma"]], (k, got)


# ---- the CPU half of the gates ---------------------------------------------------------------------------------------------------------
DT = [np.float32, np.complex64]
DT_IDS = ["float32", "complex64"]
WORST = {}


def broken(got, want, gates, exact, sums):
    """the names of the outputs of `got` outside their gate (`sums`: name -> (want, bound))"""
    bad = []
    for name, bound in gates.items():
        if want.get(name) is None:
            continue
        err = np.abs(np.asarray(got[name]).astype(np.complex128) - np.asarray(want[name]).astype(np.complex128))
        ratio = float(np.max(err / np.maximum(bound, 1e-300)))
        if not np.all(err <= bound):
            bad.append(name)
        elif got.get("_ref"):
            WORST[got["_ref"], name] = max(WORST.get((got["_ref"], name), 0.0), ratio)
    for name in exact:
        if np.asarray(got[name]).tobytes() != np.asarray(want[name]).astype(np.asarray(got[name]).dtype).tobytes():
            bad.append(name)
    for name, (w_, bound) in sums.items():
        if not abs(float(got[name]) - w_) <= bound:
            bad.append(name)
    return bad


def unwritten_tail(got, entry):
    """the last element of every output as it was on entry"""
    out = dict(got)
    for name, before in entry.items():
        if out.get(name) is not None:
            out[name] = out[name].copy()
            out[name][-1] = before[-1]
    return out


def optista_judge(v, c, got):
    want = P.optista_step(*[v[k] for k in ("res", "x0", "x", "y", "z")], *P.optista_args(c))
    gates = P.optista_gates(*[v[k] for k in ("res", "x0", "x", "y", "z")], *P.optista_args(c))
    return broken(got, want, gates, ("zold",), {"res_norm": P.norm_gate(got["res"])})


def pogm_judge(v, c, got):
    a = [v[k] for k in ("res", "x0", "xbuf", "ybuf", "z", "w")]
    want = P.pogm_step(*a, *P.pogm_args(c))
    gates = P.pogm_gates(*a[:5], c["rho"], c["c_y"], c["c_x1"], c["c_xo"], c["c_z"], c["reg_kind"], c["thr"], c["proj_kind"], c["rg"])
    sums = {"res_norm": P.norm_gate(got["res"])}
    if c["restart"]:
        sums.update(P.dot_gates(v["w"], got, c["rg"]))
    return broken(got, want, gates, ("xold",), sums)


def kinds_at(n, pogm):
    if n != P.FULL_CROSS_N:
        return [(P.REG_L1, P.PROJ_POSITIVE)] if pogm else [(P.REG_L1, None)]
    regs = (P.REG_NONE, P.REG_L1, P.REG_L2)
    return [(r, p) for r in regs for p in (P.PROJ_NONE, P.PROJ_REAL, P.PROJ_POSITIVE)] if pogm else [(r, None) for r in regs]


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("n", P.LENGTHS)
def test_optista_gates_admit_float32_and_see_every_planted_mistake(dt, n):
    cplx = np.dtype(dt).kind == "c"
    for reg, _ in kinds_at(n, False):
        v, c = P.optista_case(dt, n, reg)
        a = [v[k] for k in ("res", "x0", "x", "y", "z")]
        got = P.optista_step(*a, *P.optista_args(c), prec=np.float32)
        assert got["x"].dtype == np.dtype(dt) and got["res_norm"].dtype == np.float32
        assert optista_judge(v, c, dict(got, _ref=f"optista {np.dtype(dt).name}")) == [], (reg, n)
        # c_zn and c_zo exchanged
        c2 = dict(c, c_zn=c["c_zo"], c_zo=c["c_zn"])
        assert "x" in optista_judge(v, c, P.optista_step(*a, *P.optista_args(c2), prec=np.float32)), (reg, n)
        # zold taken after the update of z
        assert "zold" in optista_judge(v, c, dict(got, zold=got["z"])), (reg, n)
        # the last element left unwritten (zold's held something else before)
        entry = dict(v, zold=v["x"])
        assert optista_judge(v, c, unwritten_tail(got, entry)) != [], (reg, n)
        # the L1 eps added to the imaginary part too (complex data: real data has no imaginary part to add it to)
        if cplx and reg == P.REG_L1:
            wrong = P.optista_step(*a, *P.optista_args(c), prec=np.float32, l1=functools.partial(P.prox_l1, eps_imag=True))
            assert "y" in optista_judge(v, c, wrong), n


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("n", P.LENGTHS)
def test_pogm_gates_admit_float32_and_see_every_planted_mistake(dt, n):
    cplx = np.dtype(dt).kind == "c"
    for reg, proj in kinds_at(n, True):
        for restart in (True, False):
            v, c = P.pogm_case(dt, n, reg, proj, restart)
            a = [v[k] for k in ("res", "x0", "xbuf", "ybuf", "z", "w")]
            got = P.pogm_step(*a, *P.pogm_args(c), prec=np.float32)
            assert pogm_judge(v, c, dict(got, _ref=f"pogm {np.dtype(dt).name}")) == [], (reg, proj, restart, n)
            entry = dict(v, xold=v["z"])
            assert pogm_judge(v, c, unwritten_tail(got, entry)) != [], (reg, proj, restart, n)
            # rg applied with one sign flipped (:223, the z term)
            if restart:
                wrong = P.pogm_step(*a, *P.pogm_args(c), prec=np.float32, rg_flip=True)
                assert set(pogm_judge(v, c, wrong)) & {"dwx", "dwz", "dwr"}, (reg, proj, n)
            # the projections drop the imaginary part: the eps shows where there is none
            if cplx and reg == P.REG_L1 and proj == P.PROJ_NONE:
                wrong = P.pogm_step(*a, *P.pogm_args(c), prec=np.float32, l1=functools.partial(P.prox_l1, eps_imag=True))
                assert "ybuf" in pogm_judge(v, c, wrong), n


def test_report_largest_ratio_of_the_float32_reference():
    """(runs last in this file) error / bound of the float32 evaluation: how much room a correct implementation leaves"""
    for (group, name), r in sorted(WORST.items()):
        print(f"float32 pgm_ref, {group} {name}: largest error / bound {r:.3e}")
        assert r <= 1.0
