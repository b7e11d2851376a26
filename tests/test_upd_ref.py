"""The CPU half of the update-kernel tests: tests/upd_ref.py held to the oracle, and its gates shown to reject planted mistakes.

Anchors (float64 / complex128, scalars kept in double: the oracle's own arithmetic): N steps of upd_ref.cgnr_update from cgnr_init
reproduce O.CGNR's iterates; fista_init / fista_update reproduce O.FISTA's for every regulariser; cg_start / cg_update reproduce
O.cg_inplace on AHA + rho I, the cg! that O.ADMM and O.SplitBregman call.  Tolerance: both sides are float64 evaluations of the same
formulas in different summation orders; one iteration is two products of length M and N and a handful of vector operations, so an
iterate moves by at most (M + N + 16) 2^-53 times the size of its terms per iteration, amplified by no more than the step itself
(||alpha AHA|| <= 1 on CG's Krylov space, rho ||AHA|| < 1 for FISTA): k iterations stay within 8 k (M + N + 16) 2^-53 max |terms|.

Planted mistakes: for every restatement the correct float64 result, rounded to Float32 (what a correct kernel returns at best), is
within the elementwise gate, and the result of the mistaken formula is not -- at the small shapes of tests/test_gpu_update_edges.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pgm_ref as P  # noqa: E402
import rls_oracle as O  # noqa: E402
import upd_ref as R  # noqa: E402

DT = [np.float32, np.complex64]
DT_IDS = ["float32", "complex64"]
HI = {np.dtype(np.float32): np.float64, np.dtype(np.complex64): np.complex128}
MM, NN, STEPS = 24, 16, 6


def tol64(k, scale):
    return 8 * k * (MM + NN + 16) * 2.0 ** -53 * scale


def problem64(dt, seed=3):
    A, _, b = O.make_problem(MM, NN, dt, seed)
    H = HI[np.dtype(dt)]
    return A.astype(H), b.astype(H)


def aha(A, v):
    return A.conj().T @ (A @ v)


# ---- anchors -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("lam", [0.0, 0.0625])
def test_cgnr_restatement_reproduces_the_oracle(dt, lam):
    A, b = problem64(dt)
    S = O.CGNR(A, reg=O.L2Regularization(lam), iterations=STEPS, relTol=0.0)
    S.init(b)
    r0 = A.conj().T @ b
    w = R.cgnr_init(r0, 0.0, STEPS)
    assert np.array_equal(w["p"], r0) and not w["x"].any() and not w["v"].any() and w["done"] == 0
    x, r, p, rr, z0 = w["x"], r0, w["p"], w["rr"], w["z0"]
    assert abs(z0 - float(S.z0)) <= tol64(1, z0)
    for k in range(STEPS):
        S.iterate()
        v = aha(A, p)
        w = R.cgnr_update(x, r, p, v, rr, z0, lam, 0.0, k, STEPS, f32=False)
        x, r, p, rr = w["x"], w["r"], w["p"], w["rr"]
        scale = max(np.abs(S.x).max(), np.abs(S.p).max(), np.abs(r0).max())
        for got, want in ((x, S.x), (r, S.r), (p, S.p)):
            assert np.abs(got - want).max() <= tol64(k + 1, scale), (k, np.abs(got - want).max(), tol64(k + 1, scale))
        assert abs(w["alpha"] - complex(S.alpha)) <= tol64(k + 1, abs(w["alpha"])) and abs(w["beta"] - complex(S.beta).real) <= tol64(k + 1, w["beta"])
        assert (w["iteration"], bool(w["done"])) == (S.iteration, S.done())


def test_cgnr_init_keeps_the_nan_ratio():
    w = R.cgnr_init(np.zeros(5, np.float32), 0.5, 3)
    assert w["done"] == 0 and w["z0"] == 0          # NaN <= relTol is false, as in the reference
    assert R.cgnr_init(np.zeros(5, np.float32), 0.5, 0)["done"] == 1


REGS = [("none", R.REG_NONE, R.PROJ_NONE, 1), ("l1", R.REG_L1, R.PROJ_NONE, 1), ("l2", R.REG_L2, R.PROJ_NONE, 1), ("l21", R.REG_L21, R.PROJ_NONE, 4),
        ("l1+positive", R.REG_L1, R.PROJ_POSITIVE, 1), ("l21+real", R.REG_L21, R.PROJ_REAL, 2)]


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("tag,reg,proj,slices", REGS, ids=[r[0] for r in REGS])
def test_fista_restatement_reproduces_the_oracle(dt, tag, reg, proj, slices):
    A, b = problem64(dt)
    lam = 0.0625
    rho = 0.9 / np.linalg.norm(A, 2) ** 2
    oreg = {R.REG_NONE: O.L1Regularization(0.0), R.REG_L1: O.L1Regularization(lam), R.REG_L2: O.L2Regularization(lam),
            R.REG_L21: O.L21Regularization(lam, slices)}[reg]
    regs = [oreg] + ([O.PositiveRegularization()] if proj == R.PROJ_POSITIVE else [O.RealRegularization()] if proj == R.PROJ_REAL else [])
    S = O.FISTA(A, reg=regs, rho=rho, iterations=STEPS, relTol=0.0)
    S.init(b)
    x0 = A.conj().T @ b
    w = R.fista_init(x0, 1.0, STEPS)
    assert abs(w["norm_x0"] - float(S.norm_x0)) <= tol64(1, w["norm_x0"]) and np.isinf(w["res"]).all() and w["done"] == 0
    T = np.float64
    xk, xkm1, theta, theta_old, norm_x0 = w["x"], w["xold"], T(1), T(1), w["norm_x0"]
    l1 = lambda v, t: P.prox_l1(v, t, eps=np.finfo(np.float64).eps)   # noqa: E731  (the float64 oracle's eps)
    for k in range(STEPS):
        S.iterate()
        y, _ = R.fista_y(xkm1, xk, theta_old, theta, T)
        out, _ = R.fista_update(xk, y, aha(A, y), x0, rho, lam if reg != R.REG_NONE else 0.0, reg, proj, slices, theta, k, STEPS, 0.0, norm_x0,
                                T=T, l1=l1)
        xkm1, xk, theta_old, theta = xk, out["x"], out["theta_old"], out["theta"]
        scale = max(np.abs(x0).max() * rho, np.abs(S.x).max())
        assert np.abs(xk - S.x).max() <= tol64(k + 1, scale), (k, np.abs(xk - S.x).max())
        assert np.abs(out["res"] - S.res).max() <= tol64(k + 1, np.abs(x0).max())
        assert abs(out["theta"] - S.theta) <= 4 * 2.0 ** -53 * float(S.theta), (k, out["theta"], S.theta)
        assert abs(out["theta_old"] - S.theta_old) <= 4 * 2.0 ** -53 * float(S.theta_old), (k, out["theta_old"], S.theta_old)
        assert abs(float(out["rel_res_norm"]) - float(S.rel_res_norm)) <= tol64(k + 1, 1.0)
        assert (out["iteration"], bool(out["done"])) == (S.iteration, S.done())


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("maxiter", [1, 3, 5])
def test_cg_restatement_reproduces_the_cg_of_admm_and_splitbregman(dt, maxiter):
    """O.ADMM and O.SplitBregman call cg_inplace(x, AHA + rho I, beta, iterationsCG, tolInner) from the previous x; beta is the fused
    right-hand side beta_y + rho (z - u)"""
    A, b = problem64(dt)
    rho = 0.25
    rng = np.random.default_rng(5)
    H = A.dtype
    x, z, u = (rng.standard_normal(NN).astype(H) for _ in range(3))
    by = A.conj().T @ b
    xo = x.copy()
    beta = by + rho * (z - u)
    its = O.cg_inplace(xo, lambda q: aha(A, q) + rho * q, beta, maxiter, 0.0)
    w = R.cg_start(x, None, aha(A, x), rho, 0.0, maxiter, fuse=(by, z, u, rho))
    assert np.abs(w["beta"] - beta).max() <= tol64(1, np.abs(beta).max()) and np.array_equal(w["xold"], x)
    rec = R.cg_start_record(w["r"], 0.0, maxiter)
    xs, us, rs, residual = x, w["u"], w["r"], rec["residual"]
    k, done, tol = 0, rec["done"], rec["tol"]
    while not done:
        s = R.cg_update(xs, us, rs, aha(A, us), residual, rho, tol, k, maxiter, f32=False)
        xs, us, rs, residual, done = s["x"], s["u"], s["r"], s["residual"], s["done"]
        k += 1
    assert k == its
    assert np.abs(xs - xo).max() <= tol64(k, max(np.abs(xo).max(), np.abs(x).max()))


L1_64 = lambda v, t: P.prox_l1(v, t, eps=np.finfo(np.float64).eps)   # noqa: E731  (the float64 oracle's eps)


def cg_run(A, x, u, r, rho, tol_inner, icg):
    """the inner cg! from a start kernel's (u, r): (x, iterations)"""
    rec = R.cg_start_record(r, tol_inner, icg)
    residual, done, tol, k = rec["residual"], rec["done"], rec["tol"], 0
    while not done:
        s_ = R.cg_update(x, u, r, aha(A, u), residual, rho, tol, k, icg, f32=False)
        x, u, r, residual, done = s_["x"], s_["u"], s_["r"], s_["residual"], s_["done"]
        k += 1
    return x, k


def nrm(v):
    return float(np.linalg.norm(v))


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
def test_admm_restatements_reproduce_whole_outer_iterations(dt):
    """O.ADMM with L1: the fused start (beta = beta_y + rho (z - u), xold = x), its cg!, z = prox(x + u), u += x - z, the norms and
    `done`, outer iteration by outer iteration"""
    A, b = problem64(dt)
    rho, lam, icg, outer = 0.25, 0.0625, 3, 3
    S = O.ADMM(A, reg=O.L1Regularization(lam), rho=rho, iterations=outer, iterationsCG=icg, absTol=0.0, relTol=0.0, tolInner=0.0)
    S.init(b)
    x, z, u, by = S.x.copy(), S.z[0].copy(), S.u[0].copy(), S.beta_y.copy()
    for k in range(outer):
        S.iterate()
        w = R.cg_start(x, None, aha(A, x), rho, 0.0, icg, fuse=(by, z, u, rho))
        pre = R.admm_pre(None, by, z, u, x, rho, 0)
        assert np.array_equal(pre["beta"], w["beta"]) and np.array_equal(pre["xold"], x)     # the two forms of the right-hand side agree
        xn, its = cg_run(A, x, w["u"], w["r"], rho, 0.0, icg)
        assert its == S.cg_iters[-1]
        zu = R.admm_zu(xn, None, u, R.REG_L1, lam / (2 * rho), R.PROJ_NONE, l1=L1_64)
        assert np.array_equal(zu["u"], R.admm_post(xn, None, zu["z"], None, u)["u"])
        scale = max(np.abs(S.x).max(), np.abs(S.beta).max(), np.abs(S.u[0]).max())
        for got, want in ((w["beta"], S.beta), (xn, S.x), (zu["z"], S.z[0]), (zu["u"], S.u[0])):
            assert np.abs(got - want).max() <= tol64((k + 1) * (icg + 1), scale), (k, np.abs(got - want).max())
        norms = [nrm(xn - x), nrm(zu["z"] - z), nrm(zu["u"] - u), nrm(xn), nrm(zu["z"]), nrm(xn - zu["z"]), nrm(zu["u"])]
        d = R.admm_decision(norms, rho, 0.0, 0.0, k, outer, T=np.float64)
        for name_, want in (("delta", S.Delta[0]), ("sk", S.sk[0]), ("eps_pri", S.eps_pri[0]), ("rk", S.rk[0]), ("eps_dua", S.eps_dua[0])):
            assert abs(float(d[name_]) - float(want)) <= tol64((k + 1) * (icg + 1), scale * np.sqrt(NN)), (k, name_)
        assert (d["iteration"], bool(d["done"])) == (S.iteration, S.done())
        x, z, u = xn, zu["z"], zu["u"]


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
def test_bregman_start_reproduces_the_splitbregman_update(dt):
    """O.SplitBregman, two inner iterations per block: the Bregman update at the end of a block (beta_y += y - AHA x, z = x, u = 0) as
    cg_start_bregman applies it on the start of the next inner iteration, and that iteration's cg! from its (u, r)"""
    A, b = problem64(dt)
    rho, lam, icg, inner = 0.25, 0.0625, 3, 2
    S = O.SplitBregman(A, reg=O.L1Regularization(lam), rho=rho, iterations=2, iterationsInner=inner, iterationsCG=icg, absTol=0.0,
                       relTol=0.0, tolInner=0.0)
    S.init(b)
    y = S.beta_y.copy()
    x, z, u, by = S.x.copy(), S.z[0].copy(), S.u[0].copy(), S.beta_y.copy()
    for k in range(inner):
        S.iterate()
        w = R.cg_start(x, None, aha(A, x), rho, 0.0, icg, fuse=(by, z, u, rho))
        x, _ = cg_run(A, x, w["u"], w["r"], rho, 0.0, icg)
        zu = R.admm_zu(x, None, u, R.REG_L1, lam / rho, R.PROJ_NONE, l1=L1_64)
        z, u = zu["z"], zu["u"]
    scale = max(np.abs(S.x).max(), np.abs(S.beta_y).max())
    t_ = tol64(inner * (icg + 1), scale)
    assert np.abs(x - S.x).max() <= t_
    w = R.cg_start_bregman(x, y, aha(A, x), by, rho)
    assert np.abs(w["beta_y"] - S.beta_y).max() <= t_ and np.abs(w["z"] - S.z[0]).max() <= t_ and not w["zu"].any() and not S.u[0].any()
    assert np.array_equal(w["xold"], x)
    S.iterate()
    assert np.abs(w["beta"] - S.beta).max() <= 2 * t_
    xn, its = cg_run(A, x, w["u"], w["r"], rho, 0.0, icg)
    assert its == S.cg_iters[-1] and np.abs(xn - S.x).max() <= 2 * t_


# ---- planted mistakes ---------------------------------------------------------------------------------------------------------------------
def as_device(want, dt, names):
    """the correct float64 result rounded to the working type: the best a correct kernel can return"""
    return {k: np.asarray(want[k]).astype(dt) for k in names}


def rejects(got, want, gates, names=None):
    """does the elementwise gate turn `got` down?"""
    try:
        R.check(R.held_cpu, "planted", "", got, {k: want[k] for k in gates}, gates if names is None else {k: gates[k] for k in names})
    except AssertionError:
        return True
    return False


def cgnr_inputs(dt, n, lam):
    A, b = R.problem(dt, n)
    H = HI[np.dtype(dt)]
    r = (A.astype(H).conj().T @ b.astype(H)).astype(dt)
    x, p = P.vector(dt, n, 3), (r + 0.3 * P.vector(dt, n, 4)).astype(dt)
    v = aha(A.astype(H), p.astype(H)).astype(dt)
    return x, r, p, v


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("n", R.SMALL)
@pytest.mark.parametrize("mistake", ["conj", "drop_reg", "beta_flip", "keep_last"])
def test_cgnr_gate_rejects(dt, n, mistake):
    lam = np.float32(0.5)
    x, r, p, v = cgnr_inputs(dt, n, lam)
    rr, z0 = float(R.sumsq(r)), float(np.sqrt(R.sumsq(r)))
    good = R.cgnr_update(x, r, p, v, rr, z0, lam, 0.0, 0, 5)
    dev = as_device(good, dt, ("x", "r", "p"))
    good = R.cgnr_update(x, r, p, v, rr, z0, lam, 0.0, 0, 5, r_dev=dev["r"])
    dev["p"] = good["p"].astype(dt)
    gates = R.cgnr_gates(x, r, p, v, lam, good, dev["r"])
    assert not rejects(dev, good, gates)
    kw = {"conj": dict(conj=False), "drop_reg": dict(drop_reg=True), "beta_flip": dict(beta_flip=True), "keep_last": dict(keep_last=True)}[mistake]
    bad = R.cgnr_update(x, r, p, v, rr, z0, lam, 0.0, 0, 5, **kw)
    if mistake == "conj" and np.dtype(dt).kind != "c":   # a real inner product has no conjugate: nothing to tell apart
        assert np.allclose(bad["x"], good["x"], rtol=1e-12, atol=0)
        return
    bad_dev = as_device(bad, dt, ("x", "r", "p"))
    judged = R.cgnr_update(x, r, p, v, rr, z0, lam, 0.0, 0, 5, r_dev=bad_dev["r"])   # as the device test judges: p from the r that came back
    assert rejects(bad_dev, judged, R.cgnr_gates(x, r, p, v, lam, judged, bad_dev["r"]))


def test_cgnr_done_with_gt_is_caught():
    x, r, p, v = cgnr_inputs(np.float32, 65, 0.0)
    rr, z0 = float(R.sumsq(r)), float(np.sqrt(R.sumsq(r)))
    assert R.cgnr_update(x, r, p, v, rr, z0, 0.0, 0.0, 1, 2)["done"] == 1
    assert R.cgnr_update(x, r, p, v, rr, z0, 0.0, 0.0, 1, 2, done_gt=True)["done"] == 0   # the device test asserts `done` exactly


def cg_inputs(dt, n):
    A, _ = R.problem(dt, n)
    H = HI[np.dtype(dt)]
    x, u, r = (P.vector(dt, n, 10 + i) for i in range(3))
    cv = aha(A.astype(H), u.astype(H)).astype(dt)
    return x, u, r, cv, float(np.sqrt(R.sumsq(r)))


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("n", R.SMALL)
@pytest.mark.parametrize("mistake", ["conj", "drop_rho", "beta_flip", "keep_last"])
def test_cg_update_gate_rejects(dt, n, mistake):
    rho = np.float32(0.75)
    x, u, r, cv, residual = cg_inputs(dt, n)

    def judged(dev):
        w = R.cg_update(x, u, r, cv, residual, rho, 0.0, 0, 5, r_dev=dev["r"], c_dev=dev["c"])
        return w, R.cg_update_gates(x, u, r, cv, rho, w, dev["r"], dev["c"])

    good = R.cg_update(x, u, r, cv, residual, rho, 0.0, 0, 5)
    dev = as_device(good, dt, ("c", "x", "r", "u"))
    w, gates = judged(dev)
    dev["u"] = w["u"].astype(dt)
    assert not rejects(dev, w, gates)
    kw = {"conj": dict(conj=False), "drop_rho": dict(drop_rho=True), "beta_flip": dict(beta_flip=True), "keep_last": dict(keep_last=True)}[mistake]
    bad = as_device(R.cg_update(x, u, r, cv, residual, rho, 0.0, 0, 5, **kw), dt, ("c", "x", "r", "u"))
    if mistake == "conj" and np.dtype(dt).kind != "c":   # a real inner product has no conjugate: nothing to tell apart
        assert np.allclose(bad["x"], dev["x"], rtol=1e-6, atol=0)
        return
    w, gates = judged(bad)
    assert rejects(bad, w, gates)


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("n", R.SMALL)
def test_cg_start_and_bregman_gates_reject(dt, n):
    x, b, c, by, z, u, y = (P.vector(dt, n, 20 + i) for i in range(7))
    rho = np.float32(0.75)
    for fuse in (None, (by, z, u, rho)):
        good = R.cg_start(x, b, c, rho, 0.0, 3, fuse=fuse)
        gates = R.cg_start_gates(x, b, c, rho, fuse=fuse)
        assert not rejects(as_device(good, dt, gates), good, gates)
        assert rejects(as_device(R.cg_start(x, b, c, rho, 0.0, 3, fuse=fuse, drop_rho=True), dt, gates), good, gates)
    good = R.cg_start_bregman(x, y, c, by, rho)
    gates = R.cg_start_bregman_gates(x, y, c, by, rho)
    assert not rejects(as_device(good, dt, gates), good, gates)
    bad = R.cg_start_bregman(x, y, -c, by, rho)       # beta_y += y + AHA x
    assert rejects(as_device(bad, dt, gates), good, gates)
    assert R.cg_start_bregman(x, y, c, by, rho, keep_z=True)["z"].tobytes() != good["z"].tobytes()   # the copies are compared by bytes


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("n", R.SMALL)
def test_admm_gates_reject(dt, n):
    beta, by, z, u, x, xold, zold = (P.vector(dt, n, 40 + i) for i in range(7))
    rho = np.float32(0.37)
    for acc in (0, 1):
        good = R.admm_pre(beta, by, z, u, x, rho, acc)
        gates = R.admm_pre_gates(beta, by, z, u, rho, acc)
        assert not rejects(as_device(good, dt, gates), good, gates)
        assert rejects(as_device(R.admm_pre(beta, by, z, u, x, rho, acc, plus_u=True), dt, gates), good, gates)
        assert rejects(as_device(R.admm_pre(beta, by, z, u, x, rho, 1 - acc), dt, gates), good, gates)    # the wrong base vector
    good = R.admm_post(x, xold, z, zold, u)
    gates = R.admm_post_gates(x, z, u)
    assert not rejects(as_device(good, dt, gates), good, gates)
    assert rejects(as_device(R.admm_post(x, xold, z, zold, u, minus_x=True), dt, gates), good, gates)
    # z = prox(x + u): the L1 prox with eps on the imaginary part too is caught on complex data (pgm_ref plants the same)
    good = R.admm_zu(x, None, u, R.REG_L1, 0.3, R.PROJ_NONE)
    gates = R.admm_zu_gates(x, u, R.REG_L1)
    dev = as_device(good, dt, ("z", "u"))
    assert not rejects(dev, good, gates)
    assert not rejects(dev, R.admm_zu(x, None, u, R.REG_L1, 0.3, R.PROJ_NONE, z_dev=dev["z"]), R.admm_u_gate(x, dev["z"], u))
    bad = as_device(R.admm_zu(x, None, u, R.REG_L1, 0.6, R.PROJ_NONE), dt, ("z", "u"))     # lambda / rho in place of lambda / (2 rho)
    assert rejects(bad, good, gates)
    bad["u"] = (R.c64(u) - R.c64(x) - R.c64(bad["z"])).astype(dt)                          # u -= x
    assert rejects(bad, R.admm_zu(x, None, u, R.REG_L1, 0.3, R.PROJ_NONE, z_dev=bad["z"]), R.admm_u_gate(x, bad["z"], u))
    # the decision: rk against the dual limit and sk against the primal one
    norms = [0.5, 0.1, 0.2, 3.0, 2.0, 0.5, 40.0]
    a, b_ = R.admm_decision(norms, 0.5, 0.0, 0.1, 0, 9), R.admm_decision(norms, 0.5, 0.0, 0.1, 0, 9, swap=True)
    assert a["done"] != b_["done"]


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("n", [65, 1025])
@pytest.mark.parametrize("reg,slices", [(R.REG_L1, 1), (R.REG_L21, 5), (R.REG_NONE, 1)])
@pytest.mark.parametrize("mistake", ["keep_last", "plus_grad"])
def test_fista_gate_rejects(dt, n, reg, slices, mistake):
    A, b = R.problem(dt, n)
    H = HI[np.dtype(dt)]
    x0 = (A.astype(H).conj().T @ b.astype(H)).astype(dt)
    xold, y = P.vector(dt, n, 50), P.vector(dt, n, 51)
    raw = aha(A.astype(H), y.astype(H)).astype(dt)
    rho, lam = np.float32(0.4), np.float32(0.05)
    norm_x0 = float(np.sqrt(R.sumsq(x0)))
    a = (xold, y, raw, x0, rho, lam, reg, R.PROJ_NONE, slices, np.float32(1.7), 2, 9, 0.0, norm_x0)
    good, _ = R.fista_update(*a)
    dev = as_device(good, dt, ("res", "x"))
    judged, gates = R.fista_update(*a, res_dev=dev["res"])
    dev["x"] = judged["x"].astype(dt)
    assert not rejects(dev, judged, {k: gates[k] for k in ("res", "x")})
    bad, _ = R.fista_update(*a, **{mistake: True})
    bad_dev = as_device(bad, dt, ("res", "x"))
    judged, gates = R.fista_update(*a, res_dev=bad_dev["res"])
    assert rejects(bad_dev, judged, {k: gates[k] for k in ("res", "x")})


def test_fista_record_mistakes_are_caught():
    """theta and theta_old swapped; `done` with <= in place of <: the device test compares these fields exactly"""
    x0 = P.vector(np.float32, 65, 1)
    a = (x0, x0, x0, x0, 0.4, 0.05, R.REG_L1, R.PROJ_NONE, 1, np.float32(1.7), 2, 9)
    norm_x0 = float(np.sqrt(R.sumsq(x0)))
    good, _ = R.fista_update(*a, 0.0, norm_x0)
    swapped, _ = R.fista_update(*a, 0.0, norm_x0, swap_theta=True)
    assert (good["theta"], good["theta_old"]) == (swapped["theta_old"], swapped["theta"]) and good["theta"] != good["theta_old"]
    assert good["theta_old"] == np.float32(1.7) and good["theta"] == R.theta_next(np.float32(1.7))
    assert (good["rel_res_norm"], good["done"]) == (0, 0)        # res = x0 - x0: 0 < 0 is false
    le, _ = R.fista_update(*a, 0.0, norm_x0, done_le=True)
    assert le["done"] == 1
    assert R.fista_init(x0, 1.0, 0)["done"] == 1 and R.fista_init(x0, 1.0, 1)["done"] == 0


# ---- the records: what the device file compares them with turns the mistakes down -----------------------------------------------------------
def norm_rejects(got, vec):
    want, bound = P.norm_gate(vec)
    return not abs(float(np.float32(got)) - want) <= bound


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("n", R.SMALL)
def test_init_and_record_gates_reject(dt, n):
    r = (3.0 * P.vector(dt, n, 60)).astype(dt)
    # cgnr_init: z0 and ||r|| by norm_gate on the r that came back, p by bytes, done exactly
    good = R.cgnr_init(r, 0.0, 3)
    assert not norm_rejects(good["z0"], r)
    assert norm_rejects(R.cgnr_init(r, 0.0, 3, "z0_is_rr")["z0"], r)
    assert R.cgnr_init(r, 0.0, 3, "p_zero")["p"].tobytes() != good["p"].tobytes()
    assert R.cgnr_init(r, 0.0, 0)["done"] == 1 and R.cgnr_init(r, 0.0, 0, "done_gt")["done"] == 0
    assert R.cgnr_init(r, 1.0, 3)["done"] == 1                       # ratio 1 <= relTol 1
    # fista_init: ||x0|| by norm_gate, res = Inf and x = xold = 0 by bytes, theta_old = theta exactly
    good = R.fista_init(r, 1.5, 3)
    assert not norm_rejects(good["norm_x0"], r) and norm_rejects(R.fista_init(r, 1.5, 3, "norm_squared")["norm_x0"], r)
    assert R.fista_init(r, 1.5, 3, "res_zero")["res"].tobytes() != good["res"].tobytes()
    assert R.fista_init(r, 1.5, 3, "theta_old_one")["theta_old"] != good["theta_old"] == np.float32(1.5)
    # cg_start_record: ||r|| by norm_gate, tol exactly
    good = R.cg_start_record(r, 0.5, 3)
    assert not norm_rejects(good["residual"], r) and norm_rejects(R.cg_start_record(r, 0.5, 3, "residual_squared")["residual"], r)
    assert good["tol"] == float(np.float32(0.5) * np.float32(good["residual"])) != R.cg_start_record(r, 0.5, 3, "tol_is_reltol")["tol"]
    assert R.cg_start_record(r, 1.0, 3)["done"] == 1 and R.cg_start_record(r, 0.5, 3)["done"] == 0 and R.cg_start_record(r, 0.5, 0)["done"] == 1
    # admm_norms: each of the seven by its own (want, bound)
    x, xold, z, zold, u0, u1 = (P.vector(dt, n, 70 + i) for i in range(6))
    good = R.admm_norms(x, xold, z, zold, u0, u1)
    for name, idx in (("u_old_norm", 6), ("x_minus_zold", 5)):
        bad = R.admm_norms(x, xold, z, zold, u0, u1, name)
        want, bound = good[idx]
        assert abs(float(np.float32(want)) - want) <= bound and not abs(float(np.float32(bad[idx][0])) - want) <= bound
    # admm_decision: the record is compared field by field; the swapped limits flip `done` on a record that the correct rule keeps going
    w_ = [g[0] for g in good]
    w_[5], w_[1], w_[6] = 0.5, 0.1, 40.0
    a, b_ = R.admm_decision(w_, 0.5, 0.0, 0.1, 0, 9), R.admm_decision(w_, 0.5, 0.0, 0.1, 0, 9, swap=True)
    assert a["rk"] == b_["rk"] and (a["done"], b_["done"]) == (int(not a["rk"] >= np.float32(0.1) * a["eps_pri"]), 1)


# ---- the two-launch form of the FISTA update -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("proj", [R.PROJ_NONE, R.PROJ_POSITIVE])
def test_fista_phases_compose_to_the_one_launch_form(dt, proj):
    """phase 1, an identity prox, phase 2 is phase 0 with no regulariser -- every output and every record field; and O.FISTA through the
    two phases with the oracle's L1 prox in between reproduces O.FISTA"""
    n = 65
    A, b = R.problem(dt, n)
    H = HI[np.dtype(dt)]
    x0 = (A.astype(H).conj().T @ b.astype(H)).astype(dt)
    xold, y = P.vector(dt, n, 50), P.vector(dt, n, 51)
    raw = aha(A.astype(H), y.astype(H)).astype(dt)
    norm_x0 = float(np.sqrt(R.sumsq(x0)))
    a = (xold, y, raw, x0, np.float32(0.4), np.float32(0.05), R.REG_NONE, proj, 1, np.float32(1.7), 2, 9, 0.0, norm_x0)
    one, g0 = R.fista_update(*a)
    p1, g1 = R.fista_update(*a, phase=1)
    p2, g2 = R.fista_update(*a, phase=2, tv_out=p1["tv_in"], res_norm_in=p1["res_norm"])
    assert np.array_equal(p1["res"], one["res"]) and np.array_equal(p2["x"], one["x"]) and np.array_equal(g1["res"], g0["res"])
    assert np.array_equal(g1["tv_in"] + g2["x"], g0["x"])
    for k in ("res_norm", "rel_res_norm", "theta", "theta_old", "iteration", "done"):
        assert p2[k] == one[k], k
    # planted: phase 2 that forgets the projection, phase 1 with the wrong sign of the gradient step, phase 2 with another ||res||
    dev = {"x": p2["x"].astype(dt)}
    assert not rejects(dev, p2, {"x": g1["tv_in"] + g2["x"]})
    bad1, _ = R.fista_update(*a, phase=1, plus_grad=True)
    bad2, _ = R.fista_update(*a, phase=2, tv_out=bad1["tv_in"], res_norm_in=p1["res_norm"])
    assert rejects({"x": bad2["x"].astype(dt)}, p2, {"x": g1["tv_in"] + g2["x"]})
    if proj != R.PROJ_NONE:
        noproj, _ = R.fista_update(*a[:7], R.PROJ_NONE, *a[8:], phase=2, tv_out=p1["tv_in"], res_norm_in=p1["res_norm"])
        assert rejects({"x": noproj["x"].astype(dt)}, p2, {"x": g1["tv_in"] + g2["x"]})
    other, _ = R.fista_update(*a, phase=2, tv_out=p1["tv_in"], res_norm_in=2 * p1["res_norm"])
    assert other["rel_res_norm"] != p2["rel_res_norm"]            # the device cases compare rel_res_norm with the phase-1 norm


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
def test_fista_phases_reproduce_the_oracle_around_its_prox(dt):
    A, b = problem64(dt)
    lam = 0.0625
    rho = 0.9 / np.linalg.norm(A, 2) ** 2
    S = O.FISTA(A, reg=[O.L1Regularization(lam), O.PositiveRegularization()], rho=rho, iterations=STEPS, relTol=0.0)
    S.init(b)
    x0 = A.conj().T @ b
    w = R.fista_init(x0, 1.0, STEPS)
    T = np.float64
    xk, xkm1, theta, theta_old = w["x"], w["xold"], T(1), T(1)
    for k in range(STEPS):
        S.iterate()
        y, _ = R.fista_y(xkm1, xk, theta_old, theta, T)
        a = (xk, y, aha(A, y), x0, rho, lam, R.REG_NONE, R.PROJ_POSITIVE, 1, theta, k, STEPS, 0.0, w["norm_x0"])
        p1, _ = R.fista_update(*a, T=T, phase=1)
        mid = p1["tv_in"].copy()
        O.L1Regularization(lam).prox(mid, T(rho) * T(lam))          # the launch between the two phases
        p2, _ = R.fista_update(*a, T=T, phase=2, tv_out=mid, res_norm_in=p1["res_norm"])
        xkm1, xk, theta_old, theta = xk, p2["x"], p2["theta_old"], p2["theta"]
        assert np.abs(xk - S.x).max() <= tol64(k + 1, max(np.abs(x0).max() * rho, np.abs(S.x).max()))
        assert np.abs(p1["res"] - S.res).max() <= tol64(k + 1, np.abs(x0).max())
        assert abs(float(p2["rel_res_norm"]) - float(S.rel_res_norm)) <= tol64(k + 1, 1.0)
        assert abs(p2["theta"] - S.theta) <= 4 * 2.0 ** -53 * float(S.theta) and (p2["iteration"], bool(p2["done"])) == (S.iteration, S.done())


def test_admm_converged_holds_each_residual_to_its_own_limit():
    """what the device cases feed the Float32 record through: rk to the primal limit, sk to the dual one"""
    assert R.admm_converged(0.5, 0.05, 3.0, 20.0, 0.0, 0.1) is False and R.admm_converged(0.5, 0.05, 3.0, 20.0, 0.0, 0.1, swap=True) is True
    assert R.admm_converged(0.2, 0.05, 3.0, 20.0, 0.0, 0.1) is True and R.admm_converged(0.3, 0.05, 3.0, 20.0, 0.0, 0.1) is False   # `<`
    assert R.admm_converged(0.0, 0.0, 3.0, 20.0, 0.0, 0.0) is False


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
def test_product_gate_holds_a_float32_product_and_rejects_a_wrong_one(dt):
    n = 1040
    A, _ = R.problem(dt, n, 0, 16)
    v = P.vector(dt, n, 9)
    want, bound = R.product_gate(A, v)
    got = (A.conj().T @ (A @ v).astype(dt)).astype(dt)            # a Float32 evaluation
    assert (np.abs(got - want) <= bound).all() and np.abs(got - want).max() > 0
    assert not (np.abs(got * np.float32(1.01) - want) <= bound).all()
    assert not (np.abs((A.T @ (A @ v)).astype(dt) - want) <= bound).all() or np.dtype(dt).kind != "c"   # A^T for A^H
