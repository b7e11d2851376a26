"""PseudoInverse's blocked sweeps on the device (csrc/pinv.hip): phase 1 on the matrix cores, forced with
ctx.tune(pinv_block=...), ahead of the plain sweeps that decide convergence.

Truth and yardstick are those of tests/test_gpu_pinv.py (the SVD formula in float64, and in the element type).  "The restatement"
is tests/test_pinv_blocked_restatement.py: phase 1 in Float32 NumPy followed by the plain `_jacobi`.

* the factor: ||W V' - A|| / ||A||, ||V'V - I|| and max |s - s64| / s_max each <= 4 x the restatement's;
* solutions at K = 1, 3, 17: <= max(1e-5, 4 x LAPACK's error) for full rank, <= 4 x the restatement's error for rank
  deficient, dropped components exactly 0;
* phase 1 does the work (block, block_sweeps, fewer plain sweeps than with pinv_block=0 on the same A), pinv_block=0 has the
  bits of a factorisation made before the key was touched, two blocked factorisations have the same bits.

Every case prints its figures (`pytest -s`)."""
import numpy as np
import pytest

import rls_oracle as O
from test_gpu_pinv import KMAX, _factor_metrics, _gate, _jacobi_solve, _matrix, _rel, _solve_cols, _truth, _yardstick
from test_pinv_blocked_restatement import blocked_jacobi, deficient, factor_metrics2

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.complex64]
# (M, N): even block count; ragged last block + odd count (dummy block); two blocks, the second nearly empty; M no multiple of the
# Gram row split
SHAPES = [(96, 64), (200, 130), (70, 33), (520, 48)]
WIDTHS = [16, 32]


@pytest.fixture
def bctx(rls, ctx):
    """the context, handed back with the key at its default"""
    yield ctx
    ctx.tune(pinv_block=-1)


@pytest.fixture(scope="module")
def problems():
    cache = {}

    def get(shape, dt):
        key = (shape, np.dtype(dt))
        if key not in cache:
            M, N = shape
            A, _, B = O.make_problem(M, N, dt, 300 + N + M, n_rhs=KMAX)
            cache[key] = (A, B, _truth(A, B, 0.0), _yardstick(A, B, 0.0))
            for a in cache[key]:
                a.setflags(write=False)
        return cache[key]

    return get


@pytest.fixture(scope="module")
def restated():
    """the blocked restatement's (W, V, plain sweeps, blocked sweeps) per (key, width): built once"""
    cache = {}

    def get(key, A, b):
        if (key, b) not in cache:
            cache[(key, b)] = blocked_jacobi(A, b)
        return cache[(key, b)]

    return get


def _factor(rls, ctx, A, reg=None):
    solver = rls.PseudoInverse(rls.DeviceMatrix.from_host(A, ctx), reg=reg)
    plan = solver._the_plan()
    W, V = plan.factor_to_host()
    return solver, W, V, plan.status(), plan.block_status()


def _bits(solver, W, V):
    return W.tobytes() + V.tobytes() + solver.singular_values().tobytes()


def test_the_key_takes_its_four_values_and_nothing_else(rls, bctx):
    for v in (-1, 0, 16, 32):
        bctx.tune(pinv_block=v)
    for v in (8, 64, 1, -2):
        with pytest.raises(rls.RLSError):
            bctx.tune(pinv_block=v)


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "c64"])
@pytest.mark.parametrize("b", WIDTHS)
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{m}x{n}" for m, n in SHAPES])
def test_blocked_factor_and_solutions(rls, bctx, problems, restated, shape, b, dt):
    M, N = shape
    A, B, truth, yard = problems(shape, dt)
    tag = f"pinv blocked b={b} {M}x{N} {np.dtype(dt).name}"
    solver0, W0, V0, st0, bs0 = _factor(rls, bctx, A)           # before the key is touched: the plain path
    assert bs0.block == 0 and bs0.block_sweeps == 0
    bctx.tune(pinv_block=b)
    solver, W, V, st, bs = _factor(rls, bctx, A)
    two_blocks = N > b
    assert st.info == 0 and st.factorizations == 1
    assert bs.block == (b if two_blocks else 0)
    if two_blocks:
        Wj, Vj, sweeps_j, bs_j = restated(shape, A, b)
        got, want = _factor_metrics(A, W, V), _factor_metrics(A, Wj, Vj)
        print(f"{tag}: |WV'-A|/|A| {got[0]:.2e} ({want[0]:.2e})  |V'V-I| {got[1]:.2e} ({want[1]:.2e})  sigma {got[2]:.2e} ({want[2]:.2e})  "
              f"blocked sweeps {bs.block_sweeps} ({bs_j}), rounds {bs.block_rounds}, plain sweeps {st.sweeps} ({sweeps_j}; without phase 1 {st0.sweeps})")
        assert W.shape == A.shape and V.shape == (N, N)
        for name, g, w in zip(("W V' - A", "V'V - I", "sigma"), got, want):
            assert g <= 4 * w, f"{name}: device {g:.3e} > 4 x restatement {w:.3e}"
        nb = -(-N // b)
        assert bs.block_sweeps >= 1 and bs.block_rounds == bs.block_sweeps * (nb + (nb & 1) - 1)
        assert st.sweeps < st0.sweeps, "phase 1 saved no plain sweep"
    # solutions on the blocked factor
    x = rls.solve_(solver, rls.DeviceVector.from_host(B[:, 0].copy(), bctx)).to_host()
    _gate(tag + " K=1", x, truth[:, 0], yard[:, 0])
    for K in (3, KMAX):
        X = _solve_cols(rls, solver, _matrix(rls, bctx, np.asfortranarray(B[:, :K])), rls.BatchedState)
        _gate(tag + f" K={K}", X, truth[:, :K], yard[:, :K])
    conv = rls.solverconvergence(solver)[0]
    assert conv["block"] == bs.block and conv["block_sweeps"] == bs.block_sweeps and conv["factorizations"] == 1
    # a second blocked factorisation: the same bits
    solver2, W2, V2, _, _ = _factor(rls, bctx, A)
    assert _bits(solver2, W2, V2) == _bits(solver, W, V)
    x2 = rls.solve_(solver2, rls.DeviceVector.from_host(B[:, 0].copy(), bctx)).to_host()
    assert x2.tobytes() == x.tobytes()
    # pinv_block = 0: the plain path, bit for bit what it was before the key was touched
    bctx.tune(pinv_block=0)
    solver3, W3, V3, st3, bs3 = _factor(rls, bctx, A)
    assert bs3.block == 0 and st3.sweeps == st0.sweeps and _bits(solver3, W3, V3) == _bits(solver0, W0, V0)
    bd = rls.DeviceVector.from_host(B[:, 0].copy(), bctx)
    assert rls.solve_(solver3, bd).to_host().tobytes() == rls.solve_(solver0, bd).to_host().tobytes()


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "c64"])
@pytest.mark.parametrize("b", WIDTHS)
@pytest.mark.parametrize("case", ["wide3", "wide40", "repeated+zero"])
def test_rank_deficient_systems_on_blocks(rls, bctx, restated, case, b, dt):
    A, B1, lam = deficient(case, dt)
    M, N = A.shape
    rng = np.random.default_rng(77)
    B = np.asfortranarray(np.concatenate([B1[:, None], rng.standard_normal((M, KMAX - 1)).astype(dt)], axis=1))
    Wj, Vj, sweeps_j, bs_j = restated((case, np.dtype(dt).name), A, b)
    truth = _truth(A, B, lam)
    bctx.tune(pinv_block=0)
    st0 = _factor(rls, bctx, A)[3]
    bctx.tune(pinv_block=b)
    solver, W, V, st, bs = _factor(rls, bctx, A, reg=[rls.L2Regularization(lam)])
    got, want = factor_metrics2(A, W, V), factor_metrics2(A, Wj, Vj)
    print(f"pinv blocked b={b} {case} {np.dtype(dt).name}: |WV'-A|/|A| {got[0]:.2e} ({want[0]:.2e})  |V'V-I| {got[1]:.2e} ({want[1]:.2e})  "
          f"blocked sweeps {bs.block_sweeps} ({bs_j}), plain sweeps {st.sweeps} ({sweeps_j}; without phase 1 {st0.sweeps})")
    assert st.info == 0 and bs.block == b and bs.block_sweeps >= 1 and st.sweeps < st0.sweeps
    assert got[0] <= 4 * want[0] and got[1] <= 4 * want[1]
    for K in (1, 3, KMAX):
        X = _solve_cols(rls, solver, _matrix(rls, bctx, np.asfortranarray(B[:, :K])), rls.BatchedState)
        e, e_j = _rel(X, truth[:, :K]), _rel(_jacobi_solve(Wj, Vj, B[:, :K], lam), truth[:, :K])
        print(f"   K={K}: device {e:.3e}  restatement {e_j:.3e}  ratio {e / e_j:.2f}")
        assert np.all(np.isfinite(X)) and e <= 4 * e_j
    if case == "repeated+zero":        # lambda = 0: the zero column's component is dropped, not divided by
        solver.l2 = rls.L2Regularization(0.0)
        x = rls.solve_(solver, rls.DeviceVector.from_host(B[:, 0].copy(), bctx)).to_host()
        assert x[10] == 0 and np.all(np.isfinite(x)) and rls.solverconvergence(solver)["factorizations"] == 1
        assert np.all(W[:, 10] == 0) and np.all(np.delete(V[:, 10], 10) == 0) and V[10, 10] == 1      # the zero column was never rotated


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "c64"])
@pytest.mark.parametrize("b", WIDTHS)
def test_orthogonal_columns_one_blocked_sweep_one_plain_sweep_no_rotation(rls, bctx, b, dt):
    M, N = 80, 70
    A = np.zeros((M, N), dtype=dt, order="F")
    A[np.arange(N), np.arange(N)] = np.arange(1, N + 1) * (1 + (1j if np.dtype(dt).kind == "c" else 0))
    bctx.tune(pinv_block=b)
    solver, W, V, st, bs = _factor(rls, bctx, A)
    assert (bs.block, bs.block_sweeps) == (b, 1) and (st.sweeps, st.info, st.factorizations) == (1, 0, 1)
    assert W.tobytes() == np.ascontiguousarray(A).tobytes() and np.array_equal(V, np.eye(N, dtype=dt))


def test_automatic_mode_below_the_threshold_and_one_block(rls, bctx, problems):
    A, B, truth, yard = problems((200, 130), np.complex64)
    bctx.tune(pinv_block=-1)
    assert _factor(rls, bctx, A)[4].block == 0           # N = 130 < 256: never blocked
    A12, _, b12 = O.make_problem(20, 12, np.float32, 9)
    bctx.tune(pinv_block=16)
    solver, W, V, st, bs = _factor(rls, bctx, A12)       # one block: phase 1 is skipped
    assert bs.block == 0 and bs.block_sweeps == 0 and st.info == 0
    x = rls.solve_(solver, rls.DeviceVector.from_host(b12, bctx)).to_host()
    _gate("pinv 20x12 forced width, one block", x, _truth(A12, b12, 0.0), _yardstick(A12, b12, 0.0))


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "c64"])
def test_automatic_mode_at_300_by_256(rls, bctx, dt):
    A, _, B = O.make_problem(300, 256, dt, 856, n_rhs=3)
    bctx.tune(pinv_block=-1)
    solver = rls.PseudoInverse(rls.DeviceMatrix.from_host(A, bctx))
    X = _solve_cols(rls, solver, _matrix(rls, bctx, B), rls.BatchedState)
    conv = rls.solverconvergence(solver)[0]
    print(f"pinv automatic 300x256 {np.dtype(dt).name}: block {conv['block']} blocked sweeps {conv['block_sweeps']} plain sweeps {conv['sweeps']}")
    assert conv["info"] == 0 and conv["block"] in (0, 16, 32)
    _gate(f"pinv automatic 300x256 {np.dtype(dt).name}", X, _truth(A, B, 0.0), _yardstick(A, B, 0.0))


def test_automatic_mode_switches_blocks_on_from_2048_columns(rls, bctx):
    """RLS_PINV_BLOCK_AUTO_N (csrc/rls_common.hpp): one column short of it the plain path, at it blocks of RLS_PINV_BLOCK = 16;
    the wide A keeps the columns short.  This test is about the switch (the accuracy gates are the tests above, whose restatement
    would take minutes at 2048 columns): the factorisation converges and the solution is finite; its error is printed."""
    A, _, b = O.make_problem(24, 2048, np.float32, 2048)
    bctx.tune(pinv_block=-1)
    assert _factor(rls, bctx, np.asfortranarray(A[:, :2047]))[4].block == 0
    solver, W, V, st, bs = _factor(rls, bctx, A, reg=[rls.L2Regularization(0.5)])
    assert (bs.block, st.info) == (16, 0) and 1 <= bs.block_sweeps
    x = rls.solve_(solver, rls.DeviceVector.from_host(b, bctx)).to_host()
    e = _rel(x, _truth(A, b, 0.5))
    print(f"pinv automatic 24x2048 float32: blocked sweeps {bs.block_sweeps}, plain sweeps {st.sweeps}, error vs float64 {e:.2e}")
    assert np.all(np.isfinite(x))


def test_lambda_stays_free_on_a_blocked_factor(rls, bctx, problems):
    A, B, _, _ = problems((96, 64), np.complex64)
    bctx.tune(pinv_block=16)
    solver = rls.PseudoInverse(rls.DeviceMatrix.from_host(A, bctx))
    bd = rls.DeviceVector.from_host(B[:, 0].copy(), bctx)
    for lam in (0.01, 0.1, 1.0):
        solver.l2 = rls.L2Regularization(lam)
        x = rls.solve_(solver, bd).to_host()
        conv = rls.solverconvergence(solver)
        assert conv["factorizations"] == 1 and conv["block"] == 16 and conv["lambda"] == float(np.float32(lam)) and conv["info"] == 0
        _gate(f"pinv blocked lam={lam}", x, _truth(A, B[:, 0], lam), _yardstick(A, B[:, 0], lam))
    X = _solve_cols(rls, solver, _matrix(rls, bctx, np.asfortranarray(B[:, :3])), rls.BatchedState)
    _gate("pinv blocked lam=1.0 K=3", X, _truth(A, B[:, :3], 1.0), _yardstick(A, B[:, :3], 1.0))
    assert [c["factorizations"] for c in rls.solverconvergence(solver)] == [1, 1, 1]
    # MeasurementBasedNormalization: a new b is a new lambda on the same factor
    A, B, _, _ = problems((96, 64), np.float32)
    solver = rls.PseudoInverse(rls.DeviceMatrix.from_host(A, bctx), reg=[rls.L2Regularization(0.2)], normalizeReg=rls.MeasurementBasedNormalization())
    for k in (0, 1):
        b = B[:, k].copy()
        x = rls.solve_(solver, rls.DeviceVector.from_host(b, bctx)).to_host()
        conv = rls.solverconvergence(solver)
        lam = 0.2 * float(np.abs(b.astype(np.float64)).sum()) / b.size
        assert abs(conv["lambda"] - lam) <= 1e-5 * lam and conv["factorizations"] == 1 and conv["block"] == 16
        _gate(f"pinv blocked MeasurementBasedNormalization b{k}", x, _truth(A, b, conv["lambda"]), _yardstick(A, b, conv["lambda"]))
