"""The blocked Cholesky of DirectSolver (csrc/direct.hip: chol_load, chol_panel, chol_trail, chol_trsm forward and backward) held to its
factor entry by entry, through the C ABI on a Gram-only operator (rls_operator_create with A = NULL, rls_operator_set_gram), the one route
on which the test chooses G itself.  The factor is read through rls_direct_get_factor.

Integer systems (tests/direct_ref.py): G = L L^H with L of small Gaussian integers and a diagonal in {1, 2, 4}.  Every pivot, reciprocal
root, product and partial sum is then an exact Float32 integer in any order of summation, so the device must return L, and X for
B = G X, BIT FOR BIT; tests/test_direct_ref.py asserts on the CPU, for every system used here, that no sum reaches 2^24.  No tolerance.
Non-integer systems are held entrywise to the bounds derived in direct_ref's docstring (Higham Thm 10.3 / 10.4), never to a measured
figure; each case prints observed / bound.

Every G is uploaded with a padded ldg and NaN in all that the load kernel must not read: the strict upper triangle, the imaginary part
of the diagonal, the padding rows.  The factor allocation is prefilled with a sentinel through the returned pointer, so the tiles nothing
may write (the upper-triangle tiles of W, the diagonal tiles behind a failed pivot) are checked too, and the whole allocation can be
compared between two runs on fresh buffers."""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import direct_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DT = pytest.mark.parametrize("dt", R.DTYPES, ids=["f32", "c64"])
GUARD = 5
SENTINEL = {np.dtype(np.float32): np.float32(-1.2345e30), np.dtype(np.complex64): np.complex64(-1.2345e30 + 9.875e29j)}
WORST = {}     # group -> (largest observed / bound, case)
DROPPED = []   # bounded cases given up for conditioning: none may be


@pytest.fixture(autouse=True)
def _wall(request):
    t0 = time.perf_counter()
    yield
    print(f"\n[{request.node.name}: {time.perf_counter() - t0:.2f} s]")


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for g, (r, c) in sorted(WORST.items()):
        print(f"\nlargest observed / bound, {g}: {r:.3e}  ({c})")


def note(group, ratio, case):
    if ratio > WORST.get(group, (-1.0, ""))[0]:
        WORST[group] = (ratio, case)
    print(f"{group}: {case}: observed / bound {ratio:.3e}")


def poisoned(G, dt, poison=True, pad=3):
    """G in the element type with ldg = N + pad; NaN wherever chol_load_kernel must not read (poison) or zeros / the mirror (clean)"""
    dt = np.dtype(dt)
    N = G.shape[0]
    nan = np.nan + 1j * np.nan if dt.kind == "c" else np.nan
    with np.errstate(invalid="ignore", over="ignore"):
        Gh = np.asarray(G).astype(dt)
    host = np.full((N + pad, N), nan if poison else 0, dtype=dt, order="F")
    host[:N] = Gh
    if poison:
        host[:N][np.triu_indices(N, 1)] = nan
        if dt.kind == "c":
            d = np.full(N, nan, dtype=dt)      # (not re + 1j * nan: that product has a NaN real part)
            d.real = Gh.diagonal().real
            host[np.arange(N), np.arange(N)] = d
    return host


class Buf:
    """a flat device buffer with `lead` elements in front and GUARD behind, both holding the sentinel"""

    def __init__(self, rls, ctx, dt, body, lead=3):
        self.dt, self.lead, self.n = np.dtype(dt), lead, body.size
        self.host0 = np.full(lead + body.size + GUARD, SENTINEL[self.dt], dtype=self.dt)
        self.host0[lead: lead + self.n] = body.ravel(order="F")
        self.dev = rls.DeviceVector.from_host(self.host0, ctx)
        self.ptr = self.dev.ptr + lead * self.dt.itemsize

    def read(self):
        h = self.dev.to_host()
        assert h[: self.lead].tobytes() == self.host0[: self.lead].tobytes(), "elements in front of the buffer were written"
        assert h[self.lead + self.n:].tobytes() == self.host0[self.lead + self.n:].tobytes(), "elements past the end of the buffer were written"
        return h[self.lead: self.lead + self.n]

    def unchanged(self):
        return self.dev.to_host().tobytes() == self.host0.tobytes()


def columns(dt, V, ld, fill_body=True):
    """V (N x K) as an ld x K block whose padding rows (and, for fill_body = False, all rows) hold the sentinel"""
    N, K = V.shape
    host = np.full((ld, K), SENTINEL[np.dtype(dt)], dtype=dt, order="F")
    if fill_body:
        host[:N] = V
    return host


class Plan:
    """rls_direct on a Gram-only operator; the factor allocation starts out as the sentinel"""

    def __init__(self, rls, ctx, G, dt, poison=True):
        self.rls, self.ctx, self.lib, self.dt = rls, ctx, ctx.lib, np.dtype(dt)
        self.N = N = G.shape[0]
        host = poisoned(G, dt, poison)
        self.Gd = rls.DeviceMatrix(N, N, self.dt, ctx, lda=host.shape[0])
        assert self.lib.rls_memcpy_h2d(ctx.handle, self.Gd.ptr, host.ctypes.data, host.nbytes) == 0
        self.op = rls.OperatorHandle(None, self.Gd)
        self.plan = C.c_void_p()
        assert self.lib.rls_direct_create(self.op.handle, C.byref(self.plan)) == 0, self.lib.rls_last_error_string(ctx.handle)
        W, ld, Ld = C.c_void_p(), C.c_int64(), C.c_void_p()
        assert self.lib.rls_direct_get_factor(self.plan, C.byref(W), C.byref(ld), C.byref(Ld)) == 0
        self.W, self.ld = W.value, ld.value
        assert self.ld == R.padded(N) and Ld.value == self.W + self.ld * self.ld * self.dt.itemsize
        self.elems = self.ld * self.ld + self.ld * R.DB
        self.fill()

    def fill(self):
        host = np.full(self.elems, SENTINEL[self.dt], dtype=self.dt)
        assert self.lib.rls_memcpy_h2d(self.ctx.handle, self.W, host.ctypes.data, host.nbytes) == 0

    def status(self):
        st = self.rls._lib.DirectStatus()
        assert self.lib.rls_direct_get_status(self.plan, C.byref(st)) == 0
        return st

    def factor(self, lam):
        assert self.lib.rls_direct_factor(self.plan, float(lam)) == 0, self.lib.rls_last_error_string(self.ctx.handle)
        return self.status()

    def read(self):
        host = np.empty(self.elems, dtype=self.dt)
        assert self.lib.rls_memcpy_d2h(self.ctx.handle, host.ctypes.data, self.W, host.nbytes) == 0
        return host

    def solve(self, K, B, ldb, X, ldx, proj=0):
        return self.lib.rls_direct_solve(self.plan, K, B, ldb, X, ldx, proj)

    def close(self):
        assert self.lib.rls_direct_destroy(self.plan) == 0
        self.plan = None


def expected_allocation(out, dt, tiles_from=None):
    """the whole factor allocation after a factorisation the restatement `out` describes: the lower-triangle tiles of W as the kernels
    leave them, the sentinel in the upper-triangle tiles, the diagonal tiles (sentinel from tile `tiles_from` on: a failed pivot)"""
    ld = out["W"].shape[0]
    nb = ld // R.DB
    W = out["W"].astype(dt).copy(order="F")
    for p in range(nb):
        W[p * R.DB:(p + 1) * R.DB, (p + 1) * R.DB:] = SENTINEL[np.dtype(dt)]
    tiles = out["tiles"].astype(dt).copy()
    if tiles_from is not None:
        tiles[tiles_from:] = SENTINEL[np.dtype(dt)]
    return np.concatenate([W.ravel(order="F")] + [t.ravel(order="F") for t in tiles])


def same(got, want, nan_ok=False):
    """None, or where the two flat allocations differ (as a position in W or in the tile buffer)"""
    if got.tobytes() == want.tobytes() or (nan_ok and np.array_equal(got, want, equal_nan=True)):
        return None
    ld = int(round((-R.DB + (R.DB * R.DB + 4 * got.size) ** 0.5) / 2))
    Wg, Tg = R.split(got, ld)
    Ww, Tw = R.split(want, ld)
    neq = (lambda a, b: ~((a == b) | (np.isnan(a) & np.isnan(b)))) if nan_ok else None
    if nan_ok:
        bw, bt = neq(Wg, Ww), neq(Tg, Tw)
        return f"W differs at {np.argwhere(bw)[:1].tolist()}, tiles at {np.argwhere(bt)[:1].tolist()} ({int(bw.sum())} + {int(bt.sum())} entries)"
    return f"W: {R.first_difference(Wg, Ww)}; tiles: {[(j, R.first_difference(Tg[j], Tw[j])) for j in range(len(Tg)) if R.first_difference(Tg[j], Tw[j])][:1]}"


# ---- the exact factor ---------------------------------------------------------------------------------------------------------------
@DT
@pytest.mark.parametrize("N", R.FACTOR_N)
def test_factor_of_an_integer_system_is_exact(rls, ctx, N, dt):
    L, G, _, _ = R.integer_case(N, dt)
    L32, ld = L.astype(dt), R.padded(N)
    runs = []
    for lam, Gin in ((0.0, G), (R.SHIFT, G - R.SHIFT * np.eye(N))):
        want = R.blocked_cholesky(Gin.astype(dt), lam, np.float32)
        assert want["info"] == 0 and want["peak"] < R.EXACT
        for poison in (True, True, False):          # twice on fresh buffers, then once with a clean G: the same bytes
            p = Plan(rls, ctx, Gin, dt, poison)
            st = p.factor(lam)
            flat = p.read()
            p.close()
            assert (st.info, st.factorizations, st.lambda_) == (0, 1, lam)
            diff = R.first_difference(R.assemble(flat, ld, N), L32)
            assert diff is None, f"N={N} lambda={lam} poison={poison}: L: {diff}"
            Lp = R.assemble_padded(flat, ld)
            pad = np.zeros((ld, ld), dtype=dt)
            pad[np.arange(N, ld), np.arange(N, ld)] = 1
            assert R.first_difference(Lp[N:, :], pad[N:, :]) is None, f"padding rows: {R.first_difference(Lp[N:, :], pad[N:, :])}"
            # everything else: W's diagonal blocks still hold the unfactored Schur complements, nothing wrote an upper-triangle tile
            diff = same(flat, expected_allocation(want, dt))
            assert diff is None, f"N={N} lambda={lam} poison={poison}: {diff}"
            runs.append(flat.tobytes())
    assert runs[0] == runs[1] == runs[2] and runs[3] == runs[4] == runs[5]


# ---- the exact solves ---------------------------------------------------------------------------------------------------------------
def _solve_run(rls, ctx, N, dt):
    L, G, X, B = R.integer_case(N, dt)
    X32, B32 = X.astype(dt), B.astype(dt)
    p = Plan(rls, ctx, G, dt)
    assert p.factor(0.0).info == 0
    got = []
    cases = [(K, ldx, inplace, 0) for K in R.SOLVE_K for ldx in (N, N + 3) for inplace in (True, False)]
    cases += [(R.KMAX, N + 3, inplace, proj) for proj in (1, 2) for inplace in (True, False)]
    for K, ldx, inplace, proj in cases:
        tag = f"N={N} K={K} ldx={ldx} {'in place' if inplace else 'out of place'} proj={proj}"
        xb = Buf(rls, ctx, dt, columns(dt, B32[:, :K], ldx, fill_body=inplace))
        bb = xb if inplace else Buf(rls, ctx, dt, columns(dt, B32[:, :K], N + 1), lead=1)
        assert p.solve(K, bb.ptr, ldx if inplace else N + 1, xb.ptr, ldx, proj) == 0, tag
        out = xb.read().reshape((ldx, K), order="F")
        if not inplace:
            assert bb.unchanged(), f"{tag}: B was written"
        assert out[N:].tobytes() == columns(dt, B32[:, :K], ldx)[N:].tobytes(), f"{tag}: the padding rows of X were written"
        want = R.project(X32[:, :K], proj)
        diff = R.first_difference(np.ascontiguousarray(out[:N]), np.ascontiguousarray(want))
        assert diff is None, f"{tag}: X (columns go 16 per workgroup: chunk = column // 16): {diff}"
        if proj and np.dtype(dt).kind == "c":
            assert not np.signbit(out[:N].imag).any() and (out[:N].imag == 0).all(), f"{tag}: imaginary parts are not +0"
        got.append(out[:N].tobytes())
    assert p.status().factorizations == 1
    p.close()
    return b"".join(got)


@DT
@pytest.mark.parametrize("N", R.SOLVE_N)
def test_solves_of_an_integer_system_are_exact(rls, ctx, N, dt):
    assert _solve_run(rls, ctx, N, dt) == _solve_run(rls, ctx, N, dt)


# ---- planted pivots -----------------------------------------------------------------------------------------------------------------
def _pivot_run(rls, ctx, dt, kind, col):
    N = R.PIVOT_N
    G, L = R.planted_pivot(N, dt, col, kind)
    with np.errstate(invalid="ignore", over="ignore"):
        want = R.blocked_cholesky(G.astype(dt), 0.0, np.float32)
    assert want["info"] == col
    tag = f"{kind} pivot at column {col}"
    p = Plan(rls, ctx, G, dt)
    st = p.factor(0.0)
    assert (st.info, st.factorizations) == (col, 1), f"{tag}: info = {st.info}"
    # block columns in front of the failing one are factored, the failing panel and everything behind it wrote nothing: its strip and
    # the later ones hold the Schur complement the trailing updates left, the later diagonal tiles the sentinel
    flat = p.read()
    diff = same(flat, expected_allocation(want, dt, tiles_from=(col - 1) // R.DB), nan_ok=kind in ("inf", "nan"))
    assert diff is None, f"{tag}: {diff}"
    # the solves are no-ops: X is not written
    K = 17
    xb = Buf(rls, ctx, dt, columns(dt, np.zeros((N, K), dtype=dt), N + 3, fill_body=False))
    bb = Buf(rls, ctx, dt, np.ones((N, K), dtype=dt))
    assert p.solve(K, bb.ptr, N, xb.ptr, N + 3) == 0
    assert xb.unchanged(), f"{tag}: X was written after a failed factorisation"
    assert p.solve(K, bb.ptr, N, bb.ptr, N) == 0 and bb.unchanged(), f"{tag}: X (in place) was written after a failed factorisation"
    assert p.status().info == col
    # a failed factor is never reused
    st = p.factor(0.0)
    assert (st.info, st.factorizations) == (col, 2), tag
    assert same(p.read(), flat, nan_ok=True) is None
    if kind in ("zero", "negative"):
        lam = R.repairing_lambda(G)
        st = p.factor(lam)
        assert (st.info, st.factorizations, st.lambda_) == (0, 3, lam), tag
        G32 = G.astype(dt)
        Lg = R.assemble(p.read(), R.padded(N), N)
        note("repaired factor", R.factor_ratio(G32, lam, Lg), f"{tag} {np.dtype(dt).name} lambda={lam:g}")
        Xi = np.random.default_rng(col).integers(-3, 4, (N, K)).astype(R.wide(dt))
        B32 = ((R.hermitian(G32) + lam * np.eye(N)) @ Xi).astype(dt)
        xs = Buf(rls, ctx, dt, columns(dt, B32, N))
        assert p.solve(K, xs.ptr, N, xs.ptr, N) == 0
        Xg = xs.read().reshape((N, K), order="F")
        rs = R.solve_ratio(G32, lam, Lg, B32, Xg)
        note("repaired solve", rs, f"{tag} {np.dtype(dt).name} lambda={lam:g}")
        assert R.factor_ratio(G32, lam, Lg) <= 1.0 and rs <= 1.0, tag
    p.close()
    return flat.tobytes()


@DT
@pytest.mark.parametrize("kind", R.PIVOT_KINDS)
def test_planted_pivot_is_reported_at_its_column_and_stops_everything(rls, ctx, kind, dt):
    for col in R.PIVOT_COLS:
        a, b = _pivot_run(rls, ctx, dt, kind, col), _pivot_run(rls, ctx, dt, kind, col)
        assert a == b, f"{kind} pivot at column {col}: two runs differ"


# ---- non-integer data against the derived bounds --------------------------------------------------------------------------------------
@DT
@pytest.mark.parametrize("cond", R.BOUND_COND, ids=["cond10", "cond1e3"])
@pytest.mark.parametrize("N", R.BOUND_N)
def test_random_positive_definite_systems_within_the_derived_bounds(rls, ctx, N, cond, dt):
    G, _, B = R.bound_case(N, dt, cond)
    K, ldx = R.BOUND_K, N + 3
    runs = []
    for lam in R.BOUND_LAM:
        case = f"N={N} cond={cond:g} lambda={lam} {np.dtype(dt).name}"
        for _ in range(2):
            p = Plan(rls, ctx, G, dt)
            st = p.factor(lam)
            if st.info != 0:
                DROPPED.append(case)
            assert st.info == 0, f"{case}: pivot {st.info} failed on a system of condition {cond:g}"
            flat = p.read()
            xb = Buf(rls, ctx, dt, columns(dt, B, ldx, fill_body=False))
            bb = Buf(rls, ctx, dt, columns(dt, B, N + 1), lead=1)
            assert p.solve(K, bb.ptr, N + 1, xb.ptr, ldx) == 0
            out = xb.read().reshape((ldx, K), order="F")
            p.close()
            assert bb.unchanged() and out[N:].tobytes() == columns(dt, B, ldx)[N:].tobytes()
            runs.append(flat.tobytes() + out.tobytes())
        Lg = R.assemble(flat, R.padded(N), N)
        rf, rs = R.factor_ratio(G, lam, Lg), R.solve_ratio(G, lam, Lg, B, out[:N])
        note("factor", rf, case)
        note("solve", rs, case)
        assert rf <= 1.0, f"{case}: |G + lambda I - L L^H| is {rf:.3f} x the bound"
        assert rs <= 1.0, f"{case}: |B - (G + lambda I) X| is {rs:.3f} x the bound"
    assert runs[0] == runs[1] and runs[2] == runs[3]
    assert len(DROPPED) <= 0, DROPPED


# ---- the same bits through Python ---------------------------------------------------------------------------------------------------
@DT
def test_python_solver_with_an_explicit_gram_matrix_gives_the_bits_of_the_abi(rls, ctx, dt):
    N, K = 129, R.KMAX
    L, G, X, B = R.integer_case(N, dt)
    X32, B32 = X.astype(dt), B.astype(dt)
    p = Plan(rls, ctx, G, dt)
    assert p.factor(0.0).info == 0
    xb = Buf(rls, ctx, dt, B32)
    assert p.solve(K, xb.ptr, N, xb.ptr, N) == 0
    abi = xb.read().reshape((N, K), order="F")
    p.close()
    assert R.first_difference(np.ascontiguousarray(abi), np.ascontiguousarray(X32)) is None
    # A = L^H: A^H A = G and A^H (A X) = B, both exact in any order
    Ad = rls.DeviceMatrix.from_host(np.asfortranarray(L.conj().T.astype(dt)), ctx)
    Gd = rls.DeviceMatrix.from_host(np.asfortranarray(R.hermitian(G.astype(dt)).astype(dt)), ctx)
    b = np.asfortranarray((L.conj().T @ X).astype(dt))
    solver = rls.DirectSolver(Ad, AHA=Gd)
    x = rls.solve_(solver, rls.DeviceVector.from_host(b[:, 0].copy(), ctx)).to_host()
    assert x.tobytes() == abi[:, 0].tobytes()
    cols = rls.solve_(solver, rls.DeviceMatrix.from_host(b, ctx), scheduler=rls.BatchedState)
    assert np.stack([c.to_host() for c in cols], axis=1).tobytes() == np.ascontiguousarray(abi).tobytes()
    assert solver._plan.status().factorizations == 1
    # the Gram matrix alone: b is taken as A^H b
    alone = rls.DirectSolver(None, AHA=Gd)
    x = rls.solve_(alone, rls.DeviceVector.from_host(B32[:, 0].copy(), ctx)).to_host()
    assert x.tobytes() == abi[:, 0].tobytes()


@DT
def test_overlapping_b_and_x_are_refused_on_a_gram_only_operator(rls, ctx, dt):
    """the copy X = B runs all columns at once: B and X are the same block (solved in place) or apart, anything else RLS_E_INVALID"""
    N, K = 65, 3
    L, G, X, B = R.integer_case(N, dt)
    p = Plan(rls, ctx, G, dt)
    assert p.factor(0.0).info == 0
    buf = Buf(rls, ctx, dt, columns(dt, B.astype(dt)[:, :K], 2 * N + 8))
    es = np.dtype(dt).itemsize
    assert p.solve(K, buf.ptr, N, buf.ptr, N + 3) == -1                    # the same start, other strides
    assert p.solve(K, buf.ptr, N + 3, buf.ptr + 5 * es, N + 3) == -1       # shifted into each other
    assert p.solve(K, buf.ptr + (K * N - 1) * es, N, buf.ptr, N) == -1     # the last element of X is the first of B
    assert buf.unchanged()
    assert p.solve(1, buf.ptr + N * es, N, buf.ptr, N) == 0                # adjacent, not overlapping
    p.close()
