"""Batched OptISTA / POGM (solve_(S, B, scheduler=BatchedState), csrc/pgm.hip pgmb_update_kernel + rls_pgm_*_batched):
the K columns share one pass over A per product, and each column must come out as its own solve would."""
import numpy as np
import pytest

import rls_oracle as O
from conftest import parity_check

pytestmark = pytest.mark.gpu

ITERS = 25
VARIANTS = [("OptISTA", {}), ("POGM", {}), ("POGM", {"restart": "gradient", "sigma_fac": 0.96})]
CASES = [(np.complex64, 256, 128, 5, "l1"), (np.float32, 320, 96, 20, "l1"), (np.float32, 128, 64, 3, "l2"),
         (np.complex64, 4096, 2048, 16, "l1")]


def hi(dt):
    return np.complex128 if np.dtype(dt).kind == "c" else np.float64


def problem(dt, M, N, K, seed=41):
    """A, B with the columns of B scaled by 4 ** (j % 6), one fixed lambda, rho below 1 / sigma_max(A)^2"""
    A, _, B = O.make_problem(M, N, dt, seed, n_rhs=K)
    B = np.asfortranarray(B * (4.0 ** (np.arange(K) % 6)).astype(B.real.dtype)[None, :])
    A64 = A.astype(hi(dt))
    lam = 0.02 * float(np.abs(A64.conj().T @ B[:, 0].astype(hi(dt))).max())
    if M * N >= 1 << 22:
        rho = 0.9 / (np.sqrt(M) + np.sqrt(N)) ** 2  # sigma_max of a Gaussian matrix is below sqrt M + sqrt N
    else:
        rho = 0.9 / np.linalg.norm(A64, 2) ** 2
    return A, B, lam, float(rho)


def regs(R, kind, lam, name):
    if kind == "l2":
        return R.L2Regularization(lam)
    if kind == "l1+pos":
        return [R.L1Regularization(lam), R.PositiveRegularization()]
    return R.L1Regularization(lam)


def reg_kind_of(dt, kind, name):
    # the Float32 L1 case carries the Positive projection for POGM (OptISTA applies no projections)
    return "l1+pos" if (kind == "l1" and np.dtype(dt) == np.float32 and name == "POGM") else kind


def oracle_column(name, kw, A, b, reg, rho, relTol, iters=ITERS, **okw):
    """a fresh oracle solver (POGM's gamma starts at 1) on one column: (solver, rel_res_norm after every iteration)"""
    ref = getattr(O, name)(A, reg=reg, rho=rho, iterations=iters, relTol=relTol, **kw, **okw)
    hist = []
    O.solve(ref, b, callbacks=lambda s, it: hist.append(float(s.rel_res_norm)) if it > 0 else None)
    return ref, hist


def make(rls, name, kw, Ad, reg, rho, relTol, iters=ITERS, **skw):
    return rls.createLinearSolver(getattr(rls, name), Ad, reg=reg, rho=rho, iterations=iters, relTol=relTol, **kw, **skw)


def batched(rls, S, Bd, **kw):
    xs = rls.solve_(S, Bd, scheduler=rls.BatchedState, **kw)
    assert type(S.state).__name__ == "PgmBatchedState"
    return np.stack([x.to_host() for x in xs], axis=1)


@pytest.mark.parametrize("name,kw", VARIANTS)
@pytest.mark.parametrize("dt,M,N,K,kind", CASES)
def test_equals_column_solves(rls, ctx, name, kw, dt, M, N, K, kind):
    """per column: the iteration count of the float64 oracle, x inside the parity gate, and the MultiThreadingState solve of
    a second fresh solver inside the same gate.  relTol is chosen (checked below, with the oracle) so that no column's
    rel_res_norm ever comes within 1e-3 relTol of it: the Float32 stopping test cannot then differ for a harmless reason."""
    large = M * N >= 1 << 22
    relTol = 0.0 if large else 0.02
    A, B, lam, rho = problem(dt, M, N, K)
    kind = reg_kind_of(dt, kind, name)
    A64 = A.astype(hi(dt))
    cols = (0, 7, K - 1) if large else tuple(range(K))
    refs = {}
    for j in cols:
        refs[j] = oracle_column(name, kw, A64, B[:, j].astype(hi(dt)), regs(O, kind, lam, name), rho, relTol)
        for r_ in refs[j][1]:
            assert abs(r_ - relTol) >= 1e-3 * relTol, (j, r_, relTol)
    Ad, Bd = rls.DeviceMatrix.from_host(A), rls.DeviceMatrix.from_host(B)
    S = make(rls, name, kw, Ad, regs(rls, kind, lam, name), rho, relTol)
    X = batched(rls, S, Bd)
    stat = S.state.status()
    its = [s_.iteration for s_ in stat]
    S2 = make(rls, name, kw, Ad, regs(rls, kind, lam, name), rho, relTol)
    X2 = [x.to_host() for x in rls.solve_(S2, Bd, scheduler=rls.MultiThreadingState)]
    assert type(S2.state).__name__ == "MultiThreadingState"
    tag = f"pgm_batched_{name}_{'restart' if kw else 'none'}_{np.dtype(dt).name}_{M}x{N}_K{K}_{kind}"
    print(tag, "iterations", its)
    for j in cols:
        ref, _ = refs[j]
        assert stat[j].iteration == ref.iteration, (j, stat[j].iteration, ref.iteration)
        assert stat[j].done
        x32 = lambda: oracle_column(name, kw, A, np.ascontiguousarray(B[:, j]), regs(O, kind, lam, name), rho, 0.0,
                                    iters=ref.iteration)[0].x
        parity_check(f"{tag}_col{j}", X[:, j], ref.x, x32, record=(j == cols[0]))
        assert S2.state.states[j].iteration == ref.iteration
        parity_check(f"{tag}_col{j}_multithreading", X2[j], ref.x, x32, record=False)
    if (np.dtype(dt), M, N, kind) == (np.dtype(np.complex64), 256, 128, "l1"):
        assert len(set(its)) > 1, its  # the columns really retire at different iterations


@pytest.mark.parametrize("name,kw", VARIANTS)
def test_callbacks_and_reuse(rls, ctx, name, kw):
    dt, M, N, K = np.complex64, 256, 128, 5
    A, B, lam, rho = problem(dt, M, N, K)
    Ad, Bd = rls.DeviceMatrix.from_host(A), rls.DeviceMatrix.from_host(B)
    S = make(rls, name, kw, Ad, rls.L1Regularization(lam), rho, 0.02)
    X = batched(rls, S, Bd)
    n_max = max(s_.iteration for s_ in S.state.status())
    # callbacks fire at 0 .. n and the result has the bits of the no-callback solve
    fired = []
    Sc = make(rls, name, kw, Ad, rls.L1Regularization(lam), rho, 0.02)
    Xc = batched(rls, Sc, Bd, callbacks=lambda s, it: fired.append(it))
    assert fired == list(range(n_max + 1)), (fired, n_max)
    assert np.array_equal(X, Xc)
    # a second matrix solve on the same solver.  POGM's gamma is not reset by init! in the reference, and the solver hands on
    # the gamma column 0 ended with (as the per-column schedulers do): its second solve starts elsewhere, so for POGM the
    # comparison is with a second fresh solver
    if name == "OptISTA":
        assert np.array_equal(batched(rls, S, Bd), X)
    else:
        assert np.array_equal(batched(rls, make(rls, name, kw, Ad, rls.L1Regularization(lam), rho, 0.02), Bd), X)
        batched(rls, S, Bd)
    # back to a vector right-hand side: a plain state with the solver's scalars, the gate against the oracle.  POGM: the oracle
    # starts from the gamma the solver carried over, as the reference would
    b = np.ascontiguousarray(B[:, 1])
    bd = rls.DeviceVector.from_host(b)
    rls.init_(Sc, bd)
    assert type(Sc.state).__name__ == "_ProxGradState"
    assert Sc.state.rho == rho and Sc.state.relTol == 0.02
    gamma = None
    if name == "POGM":
        assert Sc.state.sigma_fac == kw.get("sigma_fac", 1)
        gamma = Sc.state.gamma
        assert np.isfinite(gamma) and gamma > 0
    x = rls.solve_(Sc, bd).to_host()
    assert type(Sc.state).__name__ == "_ProxGradState"

    def oracle(A_, b_, relTol, iters):
        ref = getattr(O, name)(A_, reg=O.L1Regularization(lam), rho=rho, iterations=iters, relTol=relTol, **kw)
        if gamma is not None:
            ref.gamma = ref.T(gamma)
        O.solve(ref, b_)
        return ref

    ref = oracle(A.astype(np.complex128), b.astype(np.complex128), 0.02, ITERS)
    assert Sc.state.iteration == ref.iteration
    parity_check(f"pgm_batched_then_vector_{name}_{'restart' if kw else 'none'}", x, ref.x,
                 lambda: oracle(A, b, 0.0, ref.iteration).x, record=False)


@pytest.mark.parametrize("name,kw", VARIANTS)
def test_padding_and_panels(rls, ctx, name, kw):
    """K = 1 is not batched; K in {7, 8, 9, 17} give the same bits for the columns they share (a column's arithmetic does not
    depend on its neighbours); across the half / full operand layouts the products are pinned equal with skinny_half, as
    test_batched_half_operand_panels_change_no_bit does for the other plans."""
    dt, M, N = np.complex64, 256, 128
    A, B, lam, rho = problem(dt, M, N, 17)
    Ad = rls.DeviceMatrix.from_host(A)
    S1 = make(rls, name, kw, Ad, rls.L1Regularization(lam), rho, 0.0, iters=9)
    rls.solve_(S1, rls.DeviceMatrix.from_host(np.asfortranarray(B[:, :1])), scheduler=rls.BatchedState)
    assert type(S1.state).__name__ != "PgmBatchedState"
    got = {}
    for half in (1, 0):
        ctx.tune(skinny_half=half)
        try:
            for K in (7, 8, 9, 17):
                S = make(rls, name, kw, Ad, rls.L1Regularization(lam), rho, 0.0, iters=9)
                got[half, K] = batched(rls, S, rls.DeviceMatrix.from_host(np.asfortranarray(B[:, :K])))
        finally:
            ctx.tune(skinny_half=1)
    base = got[1, 17]
    assert np.isfinite(base).all() and np.abs(base).max() > 0
    for (half, K), X in got.items():
        assert np.array_equal(X, base[:, :K]), (half, K, np.abs(X - base[:, :K]).max())


@pytest.mark.parametrize("name,kw", VARIANTS)
def test_explicit_gram(rls, ctx, name, kw):
    dt, M, N, K = np.complex64, 256, 128, 5
    A, B, lam, rho = problem(dt, M, N, K)
    A64 = A.astype(np.complex128)
    G64 = A64.conj().T @ A64
    Ad, Bd = rls.DeviceMatrix.from_host(A), rls.DeviceMatrix.from_host(B)
    S = make(rls, name, kw, Ad, rls.L1Regularization(lam), rho, 0.0, AHA=Ad.gram())
    X = batched(rls, S, Bd)
    G32 = (A.conj().T @ A).astype(np.complex64)
    for j in range(K):
        ref, _ = oracle_column(name, kw, A64, B[:, j].astype(np.complex128), O.L1Regularization(lam), rho, 0.0, AHA=G64)
        x32 = lambda: oracle_column(name, kw, A, np.ascontiguousarray(B[:, j]), O.L1Regularization(lam), rho, 0.0, AHA=G32)[0].x
        parity_check(f"pgm_batched_gram_{name}_{'restart' if kw else 'none'}_col{j}", X[:, j], ref.x, x32, record=False)


@pytest.mark.parametrize("name", ["OptISTA", "POGM"])
@pytest.mark.parametrize("why", ["shape", "tv", "double", "measurement"])
def test_fallbacks_keep_working(rls, ctx, name, why):
    dt = np.float64 if why == "double" else np.float32
    M, N, K = (250, 64, 3) if why == "shape" else (256, 64, 3)
    A, B, lam, rho = problem(dt, M, N, K)
    A64 = A.astype(np.float64)
    reg = (lambda R: R.TVRegularization(lam, shape=(8, 8))) if why == "tv" else (lambda R: R.L1Regularization(lam))
    skw = {"normalizeReg": rls.MeasurementBasedNormalization()} if why == "measurement" else {}
    okw = {"normalizeReg": "measurement"} if why == "measurement" else {}
    S = make(rls, name, {}, rls.DeviceMatrix.from_host(A), reg(rls), rho, 0.0, iters=12, **skw)
    xs = rls.solve_(S, rls.DeviceMatrix.from_host(B), scheduler=rls.BatchedState)
    assert type(S.state).__name__ == "MultiThreadingState"
    for j in range(K):
        ref, _ = oracle_column(name, {}, A64, B[:, j].astype(np.float64), reg(O), rho, 0.0, iters=12, **okw)
        x32 = lambda: oracle_column(name, {}, A, np.ascontiguousarray(B[:, j]), reg(O), rho, 0.0, iters=12, **okw)[0].x
        parity_check(f"pgm_batched_fallback_{why}_{name}_col{j}", xs[j].to_host(), ref.x, x32, record=False)


@pytest.mark.parametrize("name,kw", VARIANTS)
def test_reproducible(rls, ctx, name, kw):
    dt, M, N, K, _ = CASES[0]
    A, B, lam, rho = problem(dt, M, N, K)
    Ad, Bd = rls.DeviceMatrix.from_host(A), rls.DeviceMatrix.from_host(B)
    runs = [batched(rls, make(rls, name, kw, Ad, rls.L1Regularization(lam), rho, 0.02), Bd) for _ in range(2)]
    assert np.array_equal(runs[0], runs[1])
