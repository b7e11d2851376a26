"""PseudoInverse on the device (csrc/pinv.hip): x = V diag(s / (s^2 + lambda)) U'b from a one-sided Jacobi SVD A = W V'.

Truth: the SVD formula in float64 / complex128 (numpy.linalg.svd; singular values below 1e-12 s_max count as zero, which only
the rank-deficient cases meet).  Yardstick: the same formula from numpy.linalg.svd in the element type.

* Full rank: relative l2 error against the truth <= max(1e-5, 4 x the yardstick's error), the DirectSolver gate; the 1e-5
  floor is what binds (yardstick 1e-7 to 3e-7).
* Rank deficient (wide A, a repeated column, a zero column): <= 4 x e_J, the error of `_jacobi` + `_jacobi_solve` below, a
  Float32 NumPy restatement of the tournament Jacobi and of the drop rule (s_j <= 1e-6 ||A||_F).  DirectSolver refuses each
  of these at lambda = 0 (the pivot of the dependent column is zero to rounding); the zero-column case asserts it, where the
  pivot is exactly 0.
* The factorisation itself: ||W V' - A|| / ||A||, ||V'V - I|| and max |s - s64| / s_max, each <= 4 x the restatement's value;
  without the Newton step on (c, s) the restatement is 10 x worse on each, so the gate sees a kernel that forgets it.

Every case prints its errors (`pytest -s`).  Observed on an MI355X over the cases below: full rank, device 3.2e-08 to 2.0e-06
against a yardstick of 1.1e-08 to 1.8e-06 -- for N >= 63 the device sits at 1.2e-06 to 2.0e-06, 4 to 10 x LAPACK's error (Jacobi
rotates every column up to 9 N times), so the 1e-5 floor is what holds, with 5 x headroom; rank deficient, device / e_J: wide
1.44e-05 / 1.45e-05 (Float32) and 5.3e-06 / 5.4e-06 (ComplexF32), repeated column 2.0e-06 / 2.1e-06 and 1.5e-06 / 1.3e-06, zero
column 1.2e-06 / 1.4e-06 and 1.1e-06 / 1.5e-06 (ratio 0.76 to 1.19); factorisation at 200 x 130 ComplexF32: 1.96e-06, 2.29e-05,
8.4e-07 (restatement 2.11e-06, 2.52e-05, 8.7e-07), largest ratio to the restatement 1.65 (sigma, 100 x 65 ComplexF32); 9 to 10
sweeps, within one of the restatement's count."""
import numpy as np
import pytest

import rls_oracle as O

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.complex64]
KMAX = 17
# (N, M, lambda).  M = "lds+1": one row past the longest column pair that stays in LDS during a round (rls_pinv_lds_rows).
SHAPES = [(1, 3, 0.0), (2, 3, 0.0), (3, 5, 1e-2), (5, 8, 1e-2), (63, 100, 0.0), (64, 96, 1e-2), (65, 100, 0.0), (130, 200, 0.0),
          (4, "lds+1", 0.0), (3, 3, 1e-2)]
LDS_ROWS = {np.dtype(np.float32): 8192, np.dtype(np.complex64): 4096}   # 64 KiB for the two columns


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.complex128) - np.asarray(b, np.complex128)) / np.linalg.norm(b))


def _svd_solve(A, B, lam):
    """the formula of src/Direct.jl:158 in A's precision"""
    U, s, Vh = np.linalg.svd(A, full_matrices=False)
    s = s.astype(U.real.dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(s > 1e-12 * s.max(), s / (s * s + s.dtype.type(lam)), 0).astype(s.dtype)
    B2 = B.reshape(B.shape[0], -1)
    return (Vh.conj().T @ (f[:, None] * (U.conj().T @ B2))).reshape((A.shape[1],) + B.shape[1:])


def _truth(A, B, lam):
    dt = np.complex128 if A.dtype.kind == "c" else np.float64
    return _svd_solve(A.astype(dt), B.astype(dt), lam)


def _yardstick(A, B, lam):
    x = _svd_solve(A, B, lam)
    assert x.dtype == A.dtype
    return x


def _jacobi(A, renorm=True, max_sweeps=40):
    """csrc/pinv.hip in Float32 NumPy: the tournament, the rotation test, the rotation.  Returns (W, V, sweeps)."""
    f = np.float32
    W, N = A.copy(), A.shape[1]
    V = np.eye(N, dtype=A.dtype)
    null, tol = f(1e-6) * np.sqrt((np.abs(W) ** 2).sum(dtype=f)), f(2e-7)
    m = N + (N & 1)
    i = np.arange(m // 2)
    for sweep in range(1, max_sweeps + 1):
        rotated = False
        for r in range(m - 1):
            p, q = np.where(i == 0, m - 1, (r + i) % (m - 1)), np.where(i == 0, r, (r - i + m - 1) % (m - 1))
            p, q = np.minimum(p, q), np.maximum(p, q)
            p, q = p[q < N], q[q < N]          # the dummy player
            wp, wq = W[:, p], W[:, q]
            a, b, g = (np.abs(wp) ** 2).sum(0, dtype=f), (np.abs(wq) ** 2).sum(0, dtype=f), (wp.conj() * wq).sum(0)
            gabs, na, nb = np.abs(g).astype(f), np.sqrt(a), np.sqrt(b)
            act = (gabs > tol * na * nb) & (na > null) & (nb > null)
            if not act.any():
                continue
            rotated = True
            p, q, a, b, g, gabs = p[act], q[act], a[act], b[act], g[act], gabs[act]
            ph = (g / gabs).astype(A.dtype)
            zeta = (b - a) / (f(2) * gabs)
            t = np.where(zeta >= 0, f(1), f(-1)) / (np.abs(zeta) + np.sqrt(f(1) + zeta * zeta))
            c = f(1) / np.sqrt(f(1) + t * t)
            s = c * t
            if renorm:   # one Newton step on c^2 + s^2 = 1 and on |ph| = 1, the residual exact (the kernel's fma)
                h = (-0.5 * (c.astype(np.float64) ** 2 + s.astype(np.float64) ** 2 - 1)).astype(f)
                c, s = c + h * c, s + h * s
                hp = (-0.5 * (ph.real.astype(np.float64) ** 2 + ph.imag.astype(np.float64) ** 2 - 1)).astype(f)
                ph = (ph + hp * ph).astype(A.dtype)
            for X in (W, V):
                xp, qt = X[:, p], ph.conj() * X[:, q]
                X[:, p], X[:, q] = c * xp - s * qt, s * xp + c * qt
        if not rotated:
            return W, V, sweep
    raise AssertionError("the restatement hit the sweep cap")


def _jacobi_solve(W, V, B, lam):
    """t_j = w_j'b / (s_j^2 + lambda), dropped where s_j <= 1e-6 ||A||_F; x = V t"""
    f = np.float32
    s2 = (np.abs(W) ** 2).sum(0, dtype=f)
    keep = s2 > f(1e-6) * f(1e-6) * s2.sum(dtype=f)
    fac = np.where(keep, f(1) / np.where(keep, s2 + f(lam), f(1)), f(0)).astype(f)
    x = V @ (fac[:, None] * (W.conj().T @ B.reshape(B.shape[0], -1)))
    assert x.dtype == W.dtype
    return x.reshape((W.shape[1],) + B.shape[1:])


def _factor_metrics(A, W, V):
    A64 = A.astype(np.complex128)
    s64 = np.linalg.svd(A64, compute_uv=False)
    s = np.sort(np.sqrt((np.abs(W.astype(np.complex128)) ** 2).sum(0)))[::-1]
    V = V.astype(np.complex128)
    return (float(np.linalg.norm(W.astype(np.complex128) @ V.conj().T - A64) / np.linalg.norm(A64)),
            float(np.linalg.norm(V.conj().T @ V - np.eye(V.shape[1]))), float(np.abs(s - s64).max() / s64.max()))


def _gate(tag, got, truth, yard):
    e, ey = _rel(got, truth), _rel(yard, truth)
    print(f"{tag}: device {e:.3e}  yardstick {ey:.3e}  ratio {e / ey if ey > 0 else float('inf'):.2f}")
    assert np.all(np.isfinite(got))
    assert e <= max(1e-5, 4 * ey), f"{tag}: device {e:.3e} > max(1e-5, 4 x yardstick {ey:.3e})"
    return e


def _matrix(rls, ctx, B, pad=0, junk=7):
    """B (M x K) on the device, columns M + pad apart (the padding rows hold junk: nothing may read them)"""
    if not pad:
        return rls.DeviceMatrix.from_host(B, ctx)
    M, K = B.shape
    Bd = rls.DeviceMatrix(M, K, B.dtype, ctx, lda=M + pad)
    host = np.full((M + pad, K), junk, dtype=B.dtype, order="F")
    host[:M] = B
    rls._lib.check(ctx.handle, ctx.lib.rls_memcpy_h2d(ctx.handle, Bd.ptr, host.ctypes.data, host.nbytes), "rls_memcpy_h2d")
    return Bd


def _solve_cols(rls, solver, Bd, scheduler):
    return np.stack([x.to_host() for x in rls.solve_(solver, Bd, scheduler=scheduler)], axis=1)


def _rows(shape, dt):
    return LDS_ROWS[np.dtype(dt)] + 1 if shape[1] == "lds+1" else shape[1]


@pytest.fixture(scope="module")
def problems():
    """(A, B with KMAX columns, truth, yardstick) per (shape, dtype): built once, never written to"""
    cache = {}

    def get(shape, dt):
        key = (shape, np.dtype(dt))
        if key not in cache:
            N, M, lam = shape[0], _rows(shape, dt), shape[2]
            A, _, B = O.make_problem(M, N, dt, 300 + N + M, n_rhs=KMAX)
            cache[key] = (A, B, _truth(A, B, lam), _yardstick(A, B, lam))
            for a in cache[key]:
                a.setflags(write=False)
        return cache[key]

    return get


@pytest.fixture(scope="module")
def restated():
    """the restatement's factor (W, V, sweeps) per matrix, keyed by the caller: built once"""
    cache = {}

    def get(key, A):
        if key not in cache:
            cache[key] = _jacobi(A)
        return cache[key]

    return get


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "c64"])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{M}x{N}" for N, M, _ in SHAPES])
def test_full_rank_solution_within_the_direct_solver_gate(rls, ctx, problems, shape, dt):
    N, M, lam = shape[0], _rows(shape, dt), shape[2]
    A, B, truth, yard = problems(shape, dt)
    solver = rls.createLinearSolver(rls.PseudoInverse, rls.DeviceMatrix.from_host(A, ctx), reg=[rls.L2Regularization(lam)])
    tag = f"pinv {M}x{N} {np.dtype(dt).name} lam={lam}"
    x = rls.solve_(solver, rls.DeviceVector.from_host(B[:, 0].copy(), ctx)).to_host()           # K = 1: a vector
    _gate(tag + " K=1", x, truth[:, 0], yard[:, 0])
    for K in (3, KMAX):
        X = _solve_cols(rls, solver, _matrix(rls, ctx, np.asfortranarray(B[:, :K])), rls.BatchedState)
        _gate(tag + f" K={K}", X, truth[:, :K], yard[:, :K])
        assert isinstance(solver.state, rls.PseudoInverseBatchedState)
    conv = rls.solverconvergence(solver)[0]
    assert (conv["info"], conv["lambda"], conv["factorizations"]) == (0, float(np.float32(lam)), 1) and 1 <= conv["sweeps"] <= 12
    sv = solver.singular_values()
    assert sv.shape == (N,) and np.all(np.diff(sv) <= 0)
    assert np.abs(sv - np.linalg.svd(A.astype(np.complex128), compute_uv=False)).max() <= 1e-5 * sv[0]


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "c64"])
def test_padded_leading_dimension_of_a_with_junk_in_the_padding(rls, ctx, problems, dt):
    A, B, truth, yard = problems((65, 100, 0.0), dt)
    plain = rls.PseudoInverse(rls.DeviceMatrix.from_host(A, ctx))
    solver = rls.PseudoInverse(_matrix(rls, ctx, A, pad=5, junk=1e6))
    bd = rls.DeviceVector.from_host(B[:, 0].copy(), ctx)
    x = rls.solve_(solver, bd).to_host()
    _gate(f"pinv 100x65 {np.dtype(dt).name} lda=105", x, truth[:, 0], yard[:, 0])
    assert x.tobytes() == rls.solve_(plain, bd).to_host().tobytes()    # the plan's copy of A has the plan's own layout


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "c64"])
def test_padded_leading_dimension_of_b(rls, ctx, problems, dt):
    A, B, truth, yard = problems((65, 100, 0.0), dt)
    solver = rls.PseudoInverse(rls.DeviceMatrix.from_host(A, ctx))
    X = _solve_cols(rls, solver, _matrix(rls, ctx, np.asfortranarray(B[:, :3]), pad=5), rls.BatchedState)
    _gate(f"pinv 100x65 {np.dtype(dt).name} ldb=105", X, truth[:, :3], yard[:, :3])
    # columns that are not 16-byte aligned are read element by element, in the same order: the bits of aligned ones
    X0 = _solve_cols(rls, solver, _matrix(rls, ctx, np.asfortranarray(B[:, :3])), rls.BatchedState)
    assert X.tobytes() == X0.tobytes()


def _deficient(case, dt):
    """(A, b, lambda) of the three rank-deficient cases"""
    if case == "wide":
        A, _, B = O.make_problem(40, 63, dt, 511)
        return A, B, 0.5
    A, _, B = O.make_problem(96, 64, dt, 512)
    A = A.copy(order="F")
    if case == "repeated":
        A[:, 5] = A[:, 20]
        return A, B, 0.5
    A[:, 10] = 0
    return A, B, 0.0


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "c64"])
@pytest.mark.parametrize("case", ["wide", "repeated", "zero"])
def test_rank_deficient_systems_are_solved(rls, ctx, restated, case, dt):
    A, b, lam = _deficient(case, dt)
    Wj, Vj, sweeps_j = restated((case, np.dtype(dt)), A)
    truth = _truth(A, b, lam)
    e_j = _rel(_jacobi_solve(Wj, Vj, b, lam), truth)
    Ad, bd = rls.DeviceMatrix.from_host(A, ctx), rls.DeviceVector.from_host(b, ctx)
    solver = rls.PseudoInverse(Ad, reg=[rls.L2Regularization(lam)])
    x = rls.solve_(solver, bd).to_host()
    e = _rel(x, truth)
    conv = rls.solverconvergence(solver)
    print(f"pinv {case} {np.dtype(dt).name} lam={lam}: device {e:.3e}  restatement {e_j:.3e}  ratio {e / e_j:.2f}  "
          f"sweeps {conv['sweeps']} (restatement {sweeps_j})")
    assert np.all(np.isfinite(x)) and conv["info"] == 0
    assert e <= 4 * e_j, f"{case}: device {e:.3e} > 4 x restatement {e_j:.3e}"
    if case == "zero":
        assert x[10] == 0                      # exactly: the column is dropped, not divided by
        with pytest.raises(rls.RLSError, match="column 11"):     # what DirectSolver does with the same system
            rls.solve_(rls.DirectSolver(Ad), bd)


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "c64"])
@pytest.mark.parametrize("shape", [(65, 100, 0.0), (130, 200, 0.0)], ids=["100x65", "200x130"])
def test_the_factorisation_itself(rls, ctx, problems, restated, shape, dt):
    A = problems(shape, dt)[0]
    Wj, Vj, sweeps_j = restated((shape, np.dtype(dt)), A)
    want = _factor_metrics(A, Wj, Vj)
    solver = rls.PseudoInverse(rls.DeviceMatrix.from_host(A, ctx))
    W, V = solver._the_plan().factor_to_host()
    got = _factor_metrics(A, W, V)
    st = solver._the_plan().status()
    print(f"pinv factor {shape[1]}x{shape[0]} {np.dtype(dt).name}: |WV'-A|/|A| {got[0]:.2e} ({want[0]:.2e})  |V'V-I| {got[1]:.2e} "
          f"({want[1]:.2e})  sigma {got[2]:.2e} ({want[2]:.2e})  sweeps {st.sweeps} ({sweeps_j})")
    assert W.shape == A.shape and V.shape == (shape[0], shape[0])
    for name, g, w in zip(("W V' - A", "V'V - I", "sigma"), got, want):
        assert g <= 4 * w, f"{name}: device {g:.3e} > 4 x restatement {w:.3e}"
    assert st.info == 0 and st.factorizations == 1 and st.sweeps <= sweeps_j + 2
    sv = solver.singular_values()
    assert np.all(np.diff(sv) <= 0)
    assert np.abs(sv - np.sort(np.sqrt((np.abs(W.astype(np.complex128)) ** 2).sum(0)))[::-1]).max() <= 1e-6 * sv[0]   # the norms of W's columns


def test_the_gate_sees_a_missing_newton_step(problems, restated):
    """the restatement without the renormalisation of (c, s) misses 4 x the renormalised one on every metric (no device needed)"""
    shape = (130, 200, 0.0)
    A = problems(shape, np.complex64)[0]
    good, bad = _factor_metrics(A, *restated((shape, np.dtype(np.complex64)), A)[:2]), _factor_metrics(A, *_jacobi(A, renorm=False)[:2])
    print(f"restatement 200x130 c64: renormalised {good}, not renormalised {bad}")
    assert all(b > 4 * g for b, g in zip(bad, good))


def test_lambda_is_free(rls, ctx, problems):
    shape = (64, 96, 1e-2)
    A, B, _, _ = problems(shape, np.complex64)
    solver = rls.PseudoInverse(rls.DeviceMatrix.from_host(A, ctx))
    bd = rls.DeviceVector.from_host(B[:, 0].copy(), ctx)
    for lam in (0.01, 0.1, 1.0):
        solver.l2 = rls.L2Regularization(lam)
        x = rls.solve_(solver, bd).to_host()
        conv = rls.solverconvergence(solver)
        assert conv["factorizations"] == 1 and conv["lambda"] == float(np.float32(lam)) and conv["info"] == 0
        _gate(f"pinv lam={lam}", x, _truth(A, B[:, 0], lam), _yardstick(A, B[:, 0], lam))


def test_measurement_based_normalization_never_refactors(rls, ctx, problems):
    A, B, _, _ = problems((64, 96, 1e-2), np.float32)
    solver = rls.PseudoInverse(rls.DeviceMatrix.from_host(A, ctx), reg=[rls.L2Regularization(0.2)],
                               normalizeReg=rls.MeasurementBasedNormalization())
    for k in (0, 1):                                         # a new b: a new lambda, the same factor
        b = B[:, k].copy()
        x = rls.solve_(solver, rls.DeviceVector.from_host(b, ctx)).to_host()
        lam = 0.2 * float(np.abs(b.astype(np.float64)).sum()) / b.size
        conv = rls.solverconvergence(solver)
        assert abs(conv["lambda"] - lam) <= 1e-5 * lam and conv["factorizations"] == 1
        _gate(f"pinv MeasurementBasedNormalization b{k}", x, _truth(A, b, conv["lambda"]), _yardstick(A, b, conv["lambda"]))
    # a matrix right-hand side: per-column lambda on the one factor, and the state stays the batched one
    X = _solve_cols(rls, solver, _matrix(rls, ctx, np.asfortranarray(B[:, :2])), rls.BatchedState)
    assert isinstance(solver.state, rls.PseudoInverseBatchedState)
    conv = rls.solverconvergence(solver)
    lams = [c["lambda"] for c in conv]
    want = [0.2 * float(np.abs(B[:, k].astype(np.float64)).sum()) / B.shape[0] for k in range(2)]
    assert np.allclose(lams, want, rtol=1e-5) and lams[0] != lams[1]
    assert [c["factorizations"] for c in conv] == [1, 1]
    for k in range(2):
        _gate(f"pinv MeasurementBasedNormalization column {k}", X[:, k], _truth(A, B[:, k], lams[k]), _yardstick(A, B[:, k], lams[k]))


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "c64"])
def test_same_bits(rls, ctx, problems, dt):
    A, B, _, _ = problems((65, 100, 0.0), dt)
    out = []
    for _ in range(2):      # two fresh solvers: two factorisations of the same A
        solver = rls.PseudoInverse(rls.DeviceMatrix.from_host(A, ctx), reg=[rls.L2Regularization(0.1), rls.PositiveRegularization()])
        X = _solve_cols(rls, solver, _matrix(rls, ctx, B), rls.BatchedState)
        cols = [rls.solve_(solver, rls.DeviceVector.from_host(B[:, k].copy(), ctx)).to_host() for k in range(KMAX)]
        W, V = solver._plan.factor_to_host()
        out.append(X.tobytes() + W.tobytes() + V.tobytes() + solver.singular_values().tobytes())
        for k in range(KMAX):   # column k of a K = 17 solve is the vector solve
            assert X[:, k].tobytes() == cols[k].tobytes(), k
    assert out[0] == out[1]
    Bd = _matrix(rls, ctx, np.asfortranarray(B[:, :3]))
    for sched, state in ((rls.BatchedState, rls.PseudoInverseBatchedState), (rls.MultiThreadingState, rls.MultiThreadingState),
                         (rls.SequentialState, rls.SequentialState)):
        Xs = _solve_cols(rls, solver, Bd, sched)
        assert type(solver.state) is state
        assert Xs.tobytes() == X[:, :3].tobytes(), sched.__name__
    assert solver._plan.status().factorizations == 1


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "c64"])
def test_same_answer_as_direct_solver_and_cgnr(rls, ctx, dt):
    lam = 0.5
    A, _, b = O.make_problem(96, 64, dt, 7)
    Ad, bd = rls.DeviceMatrix.from_host(A, ctx), rls.DeviceVector.from_host(b, ctx)
    reg = [rls.L2Regularization(lam)]
    xp = rls.solve_(rls.createLinearSolver(rls.PseudoInverse, Ad, reg=reg), bd).to_host()
    xd = rls.solve_(rls.createLinearSolver(rls.DirectSolver, Ad, reg=reg), bd).to_host()
    xc = rls.solve_(rls.createLinearSolver(rls.CGNR, Ad, reg=reg, iterations=64), bd).to_host()
    print(f"pinv vs direct {np.dtype(dt).name}: {_rel(xp, xd):.3e}   vs CGNR: {_rel(xp, xc):.3e}")
    assert _rel(xp, xd) <= 1e-4 and _rel(xp, xc) <= 1e-4


def test_projections_and_the_extra_term(rls, ctx, problems):
    """A projection is 1-Lipschitz: the projected device solution is within the unprojected gate's absolute bound of the
    projected truth."""
    A, B, truth, yard = problems((65, 100, 0.0), np.complex64)
    Ad, b, xt, xy = rls.DeviceMatrix.from_host(A, ctx), B[:, 0].copy(), truth[:, 0], yard[:, 0]
    bound = max(1e-5, 4 * _rel(xy, xt)) * np.linalg.norm(xt)
    bd = rls.DeviceVector.from_host(b, ctx)
    for reg, want in ((rls.PositiveRegularization(), np.maximum(xt.real, 0)), (rls.RealRegularization(), xt.real)):
        x = rls.solve_(rls.PseudoInverse(Ad, reg=[reg]), bd).to_host()
        assert np.all(x.imag == 0) and (not isinstance(reg, rls.PositiveRegularization) or np.all(x.real >= 0))
        assert np.linalg.norm(x - want) <= bound, type(reg).__name__
    # one L1 term as the additional term: prox! applied to the solution, the same bits
    plain = rls.solve_(rls.PseudoInverse(Ad), bd)
    want = rls.prox_(rls.L1Regularization(0.05), plain).to_host()
    got = rls.solve_(rls.PseudoInverse(Ad, reg=[rls.L2Regularization(0.0), rls.L1Regularization(0.05)]), bd).to_host()
    assert got.tobytes() == want.tobytes() and np.count_nonzero(got) > 0
    # ... and on every column of a matrix right-hand side
    solver = rls.PseudoInverse(Ad, reg=[rls.L1Regularization(0.05), rls.PositiveRegularization()])
    X = _solve_cols(rls, solver, _matrix(rls, ctx, np.asfortranarray(B[:, :3])), rls.BatchedState)
    x0 = rls.solve_(solver, bd).to_host()
    assert X[:, 0].tobytes() == x0.tobytes() and np.all(X.imag == 0) and np.all(X.real >= 0)


def test_callbacks_fire_at_iterations_0_and_1(rls, ctx, problems):
    A, B, _, _ = problems((65, 100, 0.0), np.float32)
    solver = rls.PseudoInverse(rls.DeviceMatrix.from_host(A, ctx))
    seen, store = [], rls.StoreSolutionCallback()
    x = rls.solve_(solver, rls.DeviceVector.from_host(B[:, 0].copy(), ctx), callbacks=[lambda s, it: seen.append(it), store], x0=3.0)
    assert seen == [0, 1]
    assert np.all(store.solutions[0] == 3.0)                       # x0 is stored and plays no part in the result
    assert store.solutions[-1].tobytes() == x.to_host().tobytes()
    assert rls.iterate(solver) is None
    seen.clear()
    rls.solve_(solver, _matrix(rls, ctx, np.asfortranarray(B[:, :3])), callbacks=lambda s, it: seen.append(it), scheduler=rls.BatchedState)
    assert seen == [0, 1]


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "c64"])
def test_orthogonal_columns_need_one_sweep_and_no_rotation(rls, ctx, dt):
    M, N = 12, 7
    A = np.zeros((M, N), dtype=dt, order="F")
    A[np.arange(N), np.arange(N)] = np.arange(1, N + 1) * (1 + (1j if np.dtype(dt).kind == "c" else 0))   # scaled identity columns
    solver = rls.PseudoInverse(rls.DeviceMatrix.from_host(A, ctx))
    W, V = solver._the_plan().factor_to_host()
    st = solver._plan.status()
    assert (st.sweeps, st.info, st.factorizations) == (1, 0, 1)
    assert W.tobytes() == np.ascontiguousarray(A).tobytes() and np.array_equal(V, np.eye(N, dtype=dt))
    assert np.allclose(solver.singular_values(), np.abs(np.diag(A[:N]))[::-1], rtol=1e-6)


def test_refusals_on_the_device(rls, ctx):
    for dt in (np.float64, np.complex128):
        A, _, _ = O.make_problem(12, 8, dt, 3)
        with pytest.raises(NotImplementedError, match="Float32 / ComplexF32"):
            rls.createLinearSolver(rls.PseudoInverse, rls.DeviceMatrix.from_host(A, ctx), reg=[rls.L2Regularization(0.1)])
    A, _, _ = O.make_problem(12, 8, np.float32, 3)
    Ad = rls.DeviceMatrix.from_host(A, ctx)
    with pytest.raises(ValueError, match="needs the matrix A"):
        rls.PseudoInverse(AHA=Ad.gram())
    # ... and the C entry point says the same of a Gram-only operator
    import ctypes as C
    op, h = rls.OperatorHandle(None, Ad.gram()), C.c_void_p()
    assert ctx.lib.rls_pinv_create(op.handle, C.byref(h)) == -1 and not h.value
    assert b"no explicit A" in ctx.lib.rls_last_error_string(ctx.handle)
