"""CPU checks of tests/direct_ref.py, the restatement tests/test_gpu_direct_edges.py holds the Cholesky kernels to:
  * on every integer system the GPU tests use, the Float32 restatement returns L and X bit for bit and never forms a sum of absolute
    values at or above 2^24 -- the condition under which bit equality is a fair gate for ANY order of summation;
  * in float64 it agrees with numpy.linalg.cholesky / solve on random positive definite systems;
  * the inputs of the bounded GPU cases pass the derived bounds when the float64 restatement is rounded to Float32, and when the
    restatement itself runs in Float32;
  * every planted mistake is caught by the gate meant for it: by integer inequality, and by exceeding the componentwise bound."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import direct_ref as R  # noqa: E402

DT = pytest.mark.parametrize("dt", R.DTYPES, ids=["f32", "c64"])


def _f32(v, dt):
    return np.asarray(v).astype(dt)


@DT
@pytest.mark.parametrize("N", sorted(set(R.FACTOR_N + R.SOLVE_N)))
def test_integer_systems_are_exact_in_float32(N, dt):
    L, G, X, B = R.integer_case(N, dt)
    assert np.all(np.isin(L.diagonal().real, (1, 2, 4))) and np.all(np.abs(L.real) <= 4) and np.all(np.abs(L.imag) <= 1)
    assert np.array_equal(np.triu(L, 1), np.zeros_like(L))
    for lam, Gin in ((0.0, G), (R.SHIFT, G - R.SHIFT * np.eye(N))):
        out = R.blocked_cholesky(_f32(Gin, dt), lam, np.float32)
        assert out["info"] == 0 and out["peak"] < R.EXACT, (out["info"], out["peak"])
        assert R.first_difference(out["L"], _f32(L, dt)) is None, R.first_difference(out["L"], _f32(L, dt))
    # the padding carries the identity, W's diagonal blocks are left unfactored
    ld = R.padded(N)
    Lp = np.tril(out["W"], -1)
    assert np.array_equal(Lp[N:, :], np.zeros_like(Lp[N:, :]))
    assert np.array_equal(out["tiles"][-1][N - (ld - R.DB):, :][:, N - (ld - R.DB):], np.eye(ld - N, dtype=out["tiles"].dtype))
    for proj in (0, 1, 2):
        got, peak = R.blocked_solve(_f32(L, dt), _f32(B, dt), np.float32, proj)
        assert peak < R.EXACT
        assert R.first_difference(got, R.project(_f32(X, dt), proj)) is None, (proj, R.first_difference(got, R.project(_f32(X, dt), proj)))
    # every chunk of 16 columns has something for each projection to do
    if N >= 64:
        for c0 in range(0, R.KMAX, 16):
            assert (X[:, c0:c0 + 16].real < 0).any() and (np.dtype(dt).kind != "c" or (X[:, c0:c0 + 16].imag != 0).any())


def test_integer_factor_is_not_banded():
    """dense rows and columns cross every 64-block boundary: every lower-triangle tile of L has entries"""
    for dt in R.DTYPES:
        L = R.integer_case(321, dt)[0]
        for p in range(6):
            for q in range(p):
                assert np.count_nonzero(L[64 * p:64 * (p + 1), 64 * q:64 * (q + 1)]) > 0, (p, q)


@DT
@pytest.mark.parametrize("kind", R.PIVOT_KINDS)
def test_planted_pivots_fail_exactly_at_their_column(kind, dt):
    N = R.PIVOT_N
    for col in R.PIVOT_COLS:
        G, L = R.planted_pivot(N, dt, col, kind)
        with np.errstate(invalid="ignore", over="ignore"):
            out = R.blocked_cholesky(G.astype(dt), 0.0, np.float32)
        assert out["info"] == col and out["peak"] < R.EXACT, (col, out["info"], out["peak"])
        # the leading columns are an exact integer factor: block columns in front of the failing one hold L
        jf = (col - 1) // R.DB
        got = np.tril(out["W"], -1)[:N, : jf * R.DB]
        want = _f32(np.tril(L, -1)[:, : jf * R.DB], dt)
        for j in range(jf):
            got[j * 64:(j + 1) * 64, j * 64:(j + 1) * 64] = out["tiles"][j]
            want[j * 64:(j + 1) * 64, j * 64:(j + 1) * 64] = _f32(L[j * 64:(j + 1) * 64, j * 64:(j + 1) * 64], dt)
        assert R.first_difference(got, want) is None
        if kind in ("zero", "negative"):
            lam = R.repairing_lambda(G)
            ok = R.blocked_cholesky(G.astype(dt), lam, np.float32)
            assert ok["info"] == 0 and R.factor_ratio(G.astype(dt), lam, ok["L"]) <= 1.0


@DT
@pytest.mark.parametrize("N", [1, 5, 64, 65, 130, 200])
def test_float64_restatement_against_numpy(N, dt):
    G, X, B = R.random_hpd(N, dt, 100.0, seed=N)
    for lam in (0.0, 0.5):
        A = R.hermitian(G) + lam * np.eye(N)
        out = R.blocked_cholesky(G.astype(R.wide(dt)), lam, np.float64)
        want = np.linalg.cholesky(A)
        assert out["info"] == 0
        assert np.max(np.abs(out["L"] - want)) <= 1e-12 * np.max(np.abs(want))
        got, _ = R.blocked_solve(out["L"], B.astype(R.wide(dt)), np.float64)
        ref = np.linalg.solve(A, B.astype(R.wide(dt)))
        assert np.max(np.abs(got - ref)) <= 1e-10 * np.max(np.abs(ref))


@DT
@pytest.mark.parametrize("cond", R.BOUND_COND)
@pytest.mark.parametrize("N", R.BOUND_N)
def test_bounded_inputs_pass_their_bounds_on_the_cpu(N, cond, dt):
    G, _, B = R.bound_case(N, dt, cond)
    for lam in R.BOUND_LAM:
        lam32 = float(np.float32(lam))
        o64 = R.blocked_cholesky(G.astype(R.wide(dt)), lam32, np.float64)
        assert o64["info"] == 0
        L = o64["L"].astype(dt)                               # the float64 restatement rounded to Float32
        X = R.blocked_solve(o64["L"], B.astype(R.wide(dt)), np.float64)[0].astype(dt)
        rf, rs = R.factor_ratio(G, lam, L), R.solve_ratio(G, lam, L, B, X)
        o32 = R.blocked_cholesky(G, lam, np.float32)          # ... and the restatement run in Float32
        assert o32["info"] == 0
        X32 = R.blocked_solve(o32["L"], B, np.float32)[0]
        rf32, rs32 = R.factor_ratio(G, lam, o32["L"]), R.solve_ratio(G, lam, o32["L"], B, X32)
        print(f"N={N} cond={cond:g} lam={lam} {np.dtype(dt).name}: rounded float64 {rf:.3f} / {rs:.3f}, Float32 {rf32:.3f} / {rs32:.3f}")
        assert max(rf, rs, rf32, rs32) <= 1.0


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_planted_mistakes_are_caught(mistake):
    """by integer inequality on the exact gate, and by the componentwise bound on a random system (ComplexF32: a dropped conjugate is
    invisible on real data)"""
    dt, N = np.complex64, 192   # three full blocks: the skipped sub-tile lies in tile (2, 1)
    L, G, X, B = R.integer_case(N, dt)
    G32, B32, L32, X32 = (_f32(v, dt) for v in (G, B, L, X))
    Gr, _, Br = R.bound_case(257, dt, 10.0)
    if mistake == "back_uses_L":
        got, _ = R.blocked_solve(L32, B32, np.float32, mistake=mistake)
        assert R.first_difference(got, X32) is not None
        Lr = R.blocked_cholesky(Gr, 0.0, np.float32)["L"]
        assert R.solve_ratio(Gr, 0.0, Lr, Br, R.blocked_solve(Lr, Br, np.float32)[0]) <= 1.0
        ratio = R.solve_ratio(Gr, 0.0, Lr, Br, R.blocked_solve(Lr, Br, np.float32, mistake=mistake)[0])
    else:
        out = R.blocked_cholesky(G32, 0.0, np.float32, mistake=mistake)
        assert out["info"] != 0 or R.first_difference(out["L"], L32) is not None
        bad = R.blocked_cholesky(Gr, 0.0, np.float32, mistake=mistake)
        ratio = float("inf") if bad["info"] != 0 else R.factor_ratio(Gr, 0.0, bad["L"])
    print(f"{mistake}: caught, observed / bound {ratio:.3g}")
    assert ratio > 1.0


def test_assemble_reads_the_layout_of_the_plan():
    """the flat allocation (padded square, then NB tiles, column-major) back into L"""
    for dt in R.DTYPES:
        L = R.integer_case(129, dt)[0]
        out = R.blocked_cholesky(_f32(R.integer_case(129, dt)[1], dt), 0.0, np.float32)
        ld = R.padded(129)
        flat = np.concatenate([out["W"].ravel(order="F"), np.concatenate([t.ravel(order="F") for t in out["tiles"]])])
        assert R.first_difference(R.assemble(flat, ld, 129), _f32(L, dt)) is None
        W, tiles = R.split(flat, ld)
        assert np.array_equal(W, out["W"]) and np.array_equal(tiles, out["tiles"])
