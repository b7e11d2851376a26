"""DirectSolver on the device (csrc/direct.hip): x = (A'A + lambda I) \\ A'b by a blocked Cholesky factorisation.

Truth: numpy.linalg.solve(A'A + lambda I, A'B) in float64 / complex128.  Yardstick: the reference's own arithmetic in the
element type -- Gram matrix and right-hand side formed in Float32 / ComplexF32, then LAPACK's LU (numpy.linalg.solve).
Gate: relative l2 error against the truth <= max(1e-5, 4 x the yardstick's error on the same inputs); the factor 4 covers the
different error constants of unpivoted Cholesky and pivoted LU and the summation order of the matrix cores.

Observed on an MI355X over the shapes below (profiles/direct_solver.txt; every case prints its two errors, `pytest -s`
shows them): for N >= 63 the device's error is 0.8 - 2.5 x the yardstick's, largest ratio 2.54 (256 x 128
ComplexF32, K = 1: 1.41e-06 against 5.55e-07), largest error 1.87e-05 (40 x 63, lambda = 0.5; yardstick 1.45e-05).  At N = 1 and 2
both errors are single Float32 roundings (device <= 1.9e-07, yardstick down to 1.2e-08), the ratio is noise there (largest 5.18,
3 x 2 Float32 K = 3: 1.28e-07 against 2.47e-08) and the gate's floor of 1e-5 is what holds."""
import numpy as np
import pytest

import rls_oracle as O

pytestmark = pytest.mark.gpu

# (N, M, lambda): the edges of the 64-block; each tall by >= 1.5 x or with lambda > 0, so that cond(G + lambda I) <= 1e3
SHAPES = [(1, 3, 0.0), (2, 3, 0.0), (63, 100, 0.0), (64, 96, 1e-2), (65, 100, 0.0), (128, 256, 1e-2), (130, 200, 0.0), (200, 300, 0.0),
          (63, 40, 0.5)]
DTYPES = [np.float32, np.complex64]
KMAX = 17


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.complex128) - np.asarray(b, np.complex128)) / np.linalg.norm(b))


def _truth(A, B, lam):
    A64 = A.astype(np.complex128 if A.dtype.kind == "c" else np.float64)
    B64 = B.astype(A64.dtype)
    return np.linalg.solve(A64.conj().T @ A64 + lam * np.eye(A.shape[1]), A64.conj().T @ B64)


def _yardstick(A, B, lam):
    G = A.conj().T @ A                      # in the element type, as `A'*A` is in the reference
    G = G + (np.eye(A.shape[1]) * lam).astype(A.dtype)
    x = np.linalg.solve(G, A.conj().T @ B)
    assert x.dtype == A.dtype
    return x


def _gate(tag, got, truth, yard):
    e, ey = _rel(got, truth), _rel(yard, truth)
    print(f"{tag}: device {e:.3e}  yardstick {ey:.3e}  ratio {e / ey if ey > 0 else float('inf'):.2f}")
    assert e <= max(1e-5, 4 * ey), f"{tag}: device {e:.3e} > max(1e-5, 4 x yardstick {ey:.3e})"
    return e


def _matrix(rls, ctx, B, pad=0):
    """B (M x K) on the device, columns M + pad apart"""
    if not pad:
        return rls.DeviceMatrix.from_host(B, ctx)
    M, K = B.shape
    Bd = rls.DeviceMatrix(M, K, B.dtype, ctx, lda=M + pad)
    host = np.full((M + pad, K), 7, dtype=B.dtype, order="F")   # (the padding rows hold junk: nothing may read them)
    host[:M] = B
    rls._lib.check(ctx.handle, ctx.lib.rls_memcpy_h2d(ctx.handle, Bd.ptr, host.ctypes.data, host.nbytes), "rls_memcpy_h2d")
    return Bd


def _solve_cols(rls, solver, Bd, scheduler):
    return np.stack([x.to_host() for x in rls.solve_(solver, Bd, scheduler=scheduler)], axis=1)


@pytest.fixture(scope="module")
def problems():
    """(A, B with KMAX columns, truth, yardstick) per (shape, dtype): built once, never written to"""
    cache = {}

    def get(shape, dt):
        key = (shape, np.dtype(dt))
        if key not in cache:
            N, M, lam = shape
            A, _, B = O.make_problem(M, N, dt, 100 + N + M, n_rhs=KMAX)
            cache[key] = (A, B, _truth(A, B, lam), _yardstick(A, B, lam))
            for a in cache[key]:
                a.setflags(write=False)
        return cache[key]

    return get


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "c64"])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{M}x{N}" for N, M, _ in SHAPES])
def test_solution_within_four_times_lapack(rls, ctx, problems, shape, dt):
    N, M, lam = shape
    A, B, truth, yard = problems(shape, dt)
    solver = rls.createLinearSolver(rls.DirectSolver, rls.DeviceMatrix.from_host(A, ctx), reg=[rls.L2Regularization(lam)])
    tag = f"direct {M}x{N} {np.dtype(dt).name} lam={lam}"
    x = rls.solve_(solver, rls.DeviceVector.from_host(B[:, 0].copy(), ctx)).to_host()           # K = 1: a vector
    _gate(tag + " K=1", x, truth[:, 0], yard[:, 0])
    for K in (3, KMAX):
        X = _solve_cols(rls, solver, _matrix(rls, ctx, np.asfortranarray(B[:, :K])), rls.BatchedState)
        _gate(tag + f" K={K}", X, truth[:, :K], yard[:, :K])
        assert isinstance(solver.state, rls.DirectBatchedState)
    assert rls.solverconvergence(solver)[0] == {"info": 0, "lambda": float(np.float32(lam)), "factorizations": 1}


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "c64"])
def test_padded_leading_dimension_of_b(rls, ctx, problems, dt):
    shape = (65, 100, 0.0)
    A, B, truth, yard = problems(shape, dt)
    solver = rls.DirectSolver(rls.DeviceMatrix.from_host(A, ctx))
    X = _solve_cols(rls, solver, _matrix(rls, ctx, np.asfortranarray(B[:, :3]), pad=5), rls.BatchedState)
    _gate(f"direct 100x65 {np.dtype(dt).name} ldb=105", X, truth[:, :3], yard[:, :3])
    # (not necessarily the bits of ldb = 100: columns that are not 16-byte aligned take the element-wise A'b kernel, which sums
    # in another order -- the gate is the check)


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "c64"])
def test_same_answer_as_cgnr_pins_lambda_on_the_diagonal(rls, ctx, dt):
    lam = 0.5
    A, _, b = O.make_problem(96, 64, dt, 7)
    Ad, bd = rls.DeviceMatrix.from_host(A, ctx), rls.DeviceVector.from_host(b, ctx)
    xd = rls.solve_(rls.createLinearSolver(rls.DirectSolver, Ad, reg=[rls.L2Regularization(lam)]), bd).to_host()
    xc = rls.solve_(rls.createLinearSolver(rls.CGNR, Ad, reg=[rls.L2Regularization(lam)], iterations=64), bd).to_host()
    e = _rel(xd, xc)
    print(f"direct vs CGNR {np.dtype(dt).name}: {e:.3e}")
    assert e <= 1e-4
    # what src/Direct.jl:59 writes (lambda on EVERY entry) is another system
    A64 = A.astype(np.complex128)
    xb = np.linalg.solve(A64.conj().T @ A64 + lam, A64.conj().T @ b.astype(np.complex128))
    assert _rel(xd, xb) > 1e-2


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "c64"])
def test_schedulers_give_the_bits_of_vector_solves(rls, ctx, problems, dt):
    A, B, _, _ = problems((65, 100, 0.0), dt)
    Ad = rls.DeviceMatrix.from_host(A, ctx)
    solver = rls.DirectSolver(Ad, reg=[rls.L2Regularization(0.1), rls.PositiveRegularization()])
    cols = [rls.solve_(solver, rls.DeviceVector.from_host(B[:, k].copy(), ctx)).to_host() for k in range(3)]
    Bd = _matrix(rls, ctx, np.asfortranarray(B[:, :3]))
    for sched, state in ((rls.BatchedState, rls.DirectBatchedState), (rls.MultiThreadingState, rls.MultiThreadingState),
                         (rls.SequentialState, rls.SequentialState)):
        X = _solve_cols(rls, solver, Bd, sched)
        assert type(solver.state) is state
        for k in range(3):
            assert X[:, k].tobytes() == cols[k].tobytes(), (sched.__name__, k)
    assert solver._plan.status().factorizations == 1


def test_factor_is_reused_until_lambda_changes(rls, ctx, problems):
    shape = (130, 200, 0.0)
    A, B, _, _ = problems(shape, np.complex64)
    Ad = rls.DeviceMatrix.from_host(A, ctx)
    solver = rls.DirectSolver(Ad, reg=[rls.L2Regularization(0.05)])
    b = [rls.DeviceVector.from_host(B[:, k].copy(), ctx) for k in range(3)]
    rls.solve_(solver, b[0])
    rls.solve_(solver, b[1])
    assert rls.solverconvergence(solver)["factorizations"] == 1
    solver.l2 = rls.L2Regularization(0.3)
    x = rls.solve_(solver, b[2]).to_host()
    conv = rls.solverconvergence(solver)
    assert conv["factorizations"] == 2 and conv["lambda"] == float(np.float32(0.3)) and conv["info"] == 0
    _gate("direct refactor lam=0.3", x, _truth(A, B[:, 2], 0.3), _yardstick(A, B[:, 2], 0.3))
    # an explicit Gram matrix on the operator is the one that is factored (A.gram(): the same kernel the plan runs itself)
    sg = rls.DirectSolver(Ad, AHA=Ad.gram(), reg=[rls.L2Regularization(0.3)])
    assert rls.solve_(sg, b[2]).to_host().tobytes() == x.tobytes()


def test_measurement_based_normalization_sets_the_factored_lambda(rls, ctx, problems):
    A, B, _, _ = problems((64, 96, 1e-2), np.float32)
    b = B[:, 0].copy()
    solver = rls.DirectSolver(rls.DeviceMatrix.from_host(A, ctx), reg=[rls.L2Regularization(0.2)],
                              normalizeReg=rls.MeasurementBasedNormalization())
    x = rls.solve_(solver, rls.DeviceVector.from_host(b, ctx)).to_host()
    lam = 0.2 * float(np.abs(b.astype(np.float64)).sum()) / b.size
    got = rls.solverconvergence(solver)["lambda"]
    assert abs(got - lam) <= 1e-5 * lam, (got, lam)
    _gate("direct MeasurementBasedNormalization", x, _truth(A, b, got), _yardstick(A, b, got))
    # per-column lambda: the batched scheduler hands over to per-column states, one factor per column
    rls.solve_(solver, _matrix(rls, ctx, np.asfortranarray(B[:, :2])), scheduler=rls.BatchedState)
    assert isinstance(solver.state, rls.MultiThreadingState)
    lams = [c["lambda"] for c in rls.solverconvergence(solver)]
    want = [0.2 * float(np.abs(B[:, k].astype(np.float64)).sum()) / B.shape[0] for k in range(2)]
    assert np.allclose(lams, want, rtol=1e-5)


def test_projections_and_the_extra_term(rls, ctx, problems):
    """A projection is 1-Lipschitz, so the projected device solution is as close to the projected truth as the unprojected ones
    are to each other: the same absolute bound, max(1e-5, 4 x yardstick) x ||truth||."""
    shape = (65, 100, 0.0)
    A, B, truth, yard = problems(shape, np.complex64)
    Ad, b, xt, xy = rls.DeviceMatrix.from_host(A, ctx), B[:, 0].copy(), truth[:, 0], yard[:, 0]
    bound = max(1e-5, 4 * _rel(xy, xt)) * np.linalg.norm(xt)
    bd = rls.DeviceVector.from_host(b, ctx)
    for reg, want in ((rls.PositiveRegularization(), np.maximum(xt.real, 0)), (rls.RealRegularization(), xt.real)):
        x = rls.solve_(rls.DirectSolver(Ad, reg=[reg]), bd).to_host()
        assert np.all(x.imag == 0) and (not isinstance(reg, rls.PositiveRegularization) or np.all(x.real >= 0))
        assert np.linalg.norm(x - want) <= bound, type(reg).__name__
    # both, in the order given: Real then Positive is Positive
    x = rls.solve_(rls.DirectSolver(Ad, reg=[rls.RealRegularization(), rls.PositiveRegularization()]), bd).to_host()
    assert np.linalg.norm(x - np.maximum(xt.real, 0)) <= bound
    # one L1 term as the additional term: prox! applied to the solution, the same bits
    plain = rls.solve_(rls.DirectSolver(Ad), bd)
    want = rls.prox_(rls.L1Regularization(0.05), plain).to_host()
    got = rls.solve_(rls.DirectSolver(Ad, reg=[rls.L2Regularization(0.0), rls.L1Regularization(0.05)]), bd).to_host()
    assert got.tobytes() == want.tobytes() and np.count_nonzero(got) > 0
    # ... and on every column of a matrix right-hand side
    solver = rls.DirectSolver(Ad, reg=[rls.L1Regularization(0.05), rls.PositiveRegularization()])
    X = _solve_cols(rls, solver, _matrix(rls, ctx, np.asfortranarray(B[:, :3])), rls.BatchedState)
    x0 = rls.solve_(solver, bd).to_host()
    assert X[:, 0].tobytes() == x0.tobytes() and np.all(X.imag == 0) and np.all(X.real >= 0)


def test_callbacks_fire_at_iterations_0_and_1(rls, ctx, problems):
    A, B, _, _ = problems((65, 100, 0.0), np.float32)
    solver = rls.DirectSolver(rls.DeviceMatrix.from_host(A, ctx))
    seen, store = [], rls.StoreSolutionCallback()
    x = rls.solve_(solver, rls.DeviceVector.from_host(B[:, 0].copy(), ctx), callbacks=[lambda s, it: seen.append(it), store], x0=3.0)
    assert seen == [0, 1]
    assert np.all(store.solutions[0] == 3.0)                       # x0 is stored and plays no part in the result
    assert store.solutions[-1].tobytes() == x.to_host().tobytes()
    x2 = rls.solve_(solver, rls.DeviceVector.from_host(B[:, 0].copy(), ctx))
    assert x2.to_host().tobytes() == x.to_host().tobytes()
    assert rls.iterate(solver) is None
    # the batched state counts the same way
    seen.clear()
    rls.solve_(solver, _matrix(rls, ctx, np.asfortranarray(B[:, :3])), callbacks=lambda s, it: seen.append(it), scheduler=rls.BatchedState)
    assert seen == [0, 1]


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "c64"])
def test_two_runs_give_the_same_bits(rls, ctx, problems, dt):
    A, B, _, _ = problems((200, 300, 0.0), dt)
    out = []
    for _ in range(2):
        solver = rls.DirectSolver(rls.DeviceMatrix.from_host(A, ctx), reg=[rls.L2Regularization(1e-3)])
        X = _solve_cols(rls, solver, _matrix(rls, ctx, B), rls.BatchedState)
        x = rls.solve_(solver, rls.DeviceVector.from_host(B[:, 0].copy(), ctx)).to_host()
        out.append(X.tobytes() + x.tobytes())
        assert X[:, 0].tobytes() == x.tobytes()
    assert out[0] == out[1]


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "c64"])
def test_not_positive_definite_is_an_error_naming_the_column(rls, ctx, dt):
    A, _, b = O.make_problem(96, 64, dt, 11)
    A = A.copy(order="F")
    A[:, 10] = 0        # column 11 (1-based): its pivot is exactly 0
    solver = rls.DirectSolver(rls.DeviceMatrix.from_host(A, ctx))
    bd = rls.DeviceVector.from_host(b, ctx)
    with pytest.raises(rls.RLSError, match=r"column 11 .*lambda > 0"):
        rls.solve_(solver, bd)
    assert solver._plan.status().info == 11
    with pytest.raises(rls.RLSError, match="column 11"):     # a failed factor is not taken for a factor
        rls.solve_(solver, bd)
    solver.l2 = rls.L2Regularization(0.1)
    x = rls.solve_(solver, bd).to_host()
    assert rls.solverconvergence(solver)["info"] == 0
    _gate(f"direct after a failed pivot {np.dtype(dt).name}", x, _truth(A, b, 0.1), _yardstick(A, b, 0.1))


def test_double_precision_operators_are_refused_at_construction(rls, ctx):
    for dt in (np.float64, np.complex128):
        A, _, _ = O.make_problem(12, 8, dt, 3)
        Ad = rls.DeviceMatrix.from_host(A, ctx)
        with pytest.raises(NotImplementedError, match="Float32 / ComplexF32"):
            rls.DirectSolver(Ad)
        with pytest.raises(NotImplementedError, match="Float64"):
            rls.createLinearSolver(rls.DirectSolver, Ad, reg=[rls.L2Regularization(0.1)])
