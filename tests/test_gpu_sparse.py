"""GPU tests of the sparse operator (csrc/sparse.hip) and of the solvers that accept it.  Every input comes from tests/sparse_ref.py
(checked on the CPU by tests/test_sparse_abi.py); every comparison is against the dense float64 twin: 1e-5 relative for Float32 /
ComplexF32 (the parity gate), 1e-12 for Float64 / ComplexF64.

The products' shapes have N = 129, so "one row of 200 non-zeros" does not fit them: at those shapes the long row has N - 3 = 126
non-zeros, and one more matrix (65 x 257) carries the row of exactly 200."""
import numpy as np
import pytest

import rls_oracle as O
import sparse_ref as SR

pytestmark = pytest.mark.gpu

TOL = {np.dtype(np.float32): 1e-5, np.dtype(np.complex64): 1e-5, np.dtype(np.float64): 1e-12, np.dtype(np.complex128): 1e-12}
LANES = (1, 4, 16, 64)
OP_N, OP_T, OP_C = 0, 1, 2


def _rel(got, ref):
    ref = np.asarray(ref)
    n = np.linalg.norm(ref)
    d = np.linalg.norm(np.asarray(got).astype(ref.dtype) - ref)
    return d / n if n > 0 else d


def _vec(rng, n, dtype):
    v = rng.standard_normal(n)
    if np.dtype(dtype).kind == "c":
        v = v + 1j * rng.standard_normal(n)
    return v.astype(dtype)


def _matrices(dtype):
    """name -> (csc, dense twin): every shape and structure the products are held to"""
    out = {"1x1": SR.from_pattern(np.ones((1, 1), bool), dtype, 1), "7x5 nnz=0": SR.from_pattern(np.zeros((7, 5), bool), dtype, 2)}
    for M in (63, 65, 257):
        out[f"{M}x129 holes"] = SR.with_holes(M, 129, dtype, 10 + M)
        out[f"{M}x129 holes + long row"] = SR.with_holes(M, 129, dtype, 20 + M, long_row=M // 3)
    out["65x257 row of 200"] = SR.with_holes(65, 257, dtype, 31, long_row=40)
    lens = sorted({n for L in LANES for n in (L - 1, L, L + 1, 2 * L + 1)})   # 0 .. 129 = N: a full row
    out["rows of L-1, L, L+1, 2L+1"] = SR.row_lengths(lens, 129, dtype, 41)
    return out


@pytest.fixture(scope="module")
def matrices():
    """built once, shared, never modified"""
    return {np.dtype(dt): _matrices(dt) for dt in SR.DTYPES}


@pytest.fixture()
def auto_lanes(ctx):
    ctx.tune(sparse_lanes=0, sparse_kaczmarz_lds=1)
    yield ctx
    ctx.tune(sparse_lanes=0, sparse_kaczmarz_lds=1)


def _opmat(D, op):
    return D if op == OP_N else (D.T if op == OP_T else D.conj().T)


def _mul(A, op, x, y0, alpha, beta, rls, ctx):
    xd, yd = rls.DeviceVector.from_host(x, ctx), rls.DeviceVector.from_host(y0, ctx)
    A.spmv_(op, xd, yd, alpha, beta)
    return yd.to_host()


@pytest.mark.parametrize("dtype", SR.DTYPES)
def test_mul_every_shape_direction_and_instantiation(rls, auto_lanes, matrices, dtype):
    ctx, dt = auto_lanes, np.dtype(dtype)
    cplx, tol = dt.kind == "c", TOL[dt]
    pairs = [(1, 0, False), (0, 0.5, False), (1, 0, True)] + ([(2 - 0.5j, 1, False)] if cplx else [])
    rng = np.random.default_rng(7)
    for name, (csc, D) in matrices[dt].items():
        A = rls.DeviceSparseMatrix.from_host(csc, ctx)
        assert (A.M, A.N, A.nnz, A.shape, A.size(1), A.size(2)) == (*D.shape, csc[2].size, D.shape, *D.shape) and A.dtype == dt
        if cplx and csc[2].size:
            assert not np.array_equal(D.T, D.conj().T)   # T and C are different operators on these values
        for op in (OP_N, OP_T, OP_C):
            B = _opmat(D, op)
            x = _vec(rng, B.shape[1], dt)
            y0 = _vec(rng, B.shape[0], dt)
            for alpha, beta, nan in pairs:
                ystart = np.full_like(y0, np.nan) if nan else y0
                ref = alpha * (B @ x.astype(D.dtype)) + (beta * y0.astype(D.dtype) if beta != 0 else 0)
                tag = (name, op, alpha, beta, nan)
                ctx.tune(sparse_lanes=0)
                auto = _mul(A, op, x, ystart, alpha, beta, rls, ctx)
                assert np.all(np.isfinite(auto)), tag
                assert _rel(auto, ref) <= tol, (tag, _rel(auto, ref))
                assert _mul(A, op, x, ystart, alpha, beta, rls, ctx).tobytes() == auto.tobytes(), tag   # run to run: the same bits
                assert A.variant(op) in LANES
                for L in LANES:
                    ctx.tune(sparse_lanes=L)
                    assert A.variant(op) == L
                    got = _mul(A, op, x, ystart, alpha, beta, rls, ctx)
                    assert _rel(got, ref) <= tol, (tag, L, _rel(got, ref))
                    assert np.linalg.norm(got.astype(D.dtype) - auto.astype(D.dtype)) <= tol * np.linalg.norm(ref), (tag, L)
                    assert _mul(A, op, x, ystart, alpha, beta, rls, ctx).tobytes() == got.tobytes(), (tag, L)
    with pytest.raises(rls.RLSError):
        ctx.tune(sparse_lanes=8)   # not an instantiation


def test_mul_more_rows_than_one_grid_pass(rls, auto_lanes):
    """33000 rows of three non-zeros: at 16 lanes per row one pass of the grid covers 2048 x 16 = 32768 rows, at 64 lanes 8192 --
    the forced instantiations take the grid stride, the automatic one (4 lanes: 131072 rows a pass) does not"""
    ctx, M, N = auto_lanes, 33000, 64
    mask = np.zeros((M, N), bool)
    m = np.arange(M)
    for off in (0, 11, 23):
        mask[m, (7 * m + off) % N] = True
    csc, D = SR.from_pattern(mask, np.complex64, 51)
    A = rls.DeviceSparseMatrix.from_host(csc, ctx)
    rng = np.random.default_rng(8)
    for op in (OP_N, OP_C):
        B = _opmat(D, op)
        x, y0 = _vec(rng, B.shape[1], np.complex64), _vec(rng, B.shape[0], np.complex64)
        ref = B @ x.astype(np.complex128) + 0.5 * y0
        for L in (0, 16, 64):
            ctx.tune(sparse_lanes=L)
            got = _mul(A, op, x, y0, 1, 0.5, rls, ctx)
            assert _rel(got, ref) <= 1e-5, (op, L, _rel(got, ref))
            assert _mul(A, op, x, y0, 1, 0.5, rls, ctx).tobytes() == got.tobytes()


@pytest.mark.parametrize("dtype", SR.DTYPES)
def test_adjoint_identity_rownorm2_to_dense_and_round_trip(rls, auto_lanes, matrices, dtype):
    ctx, dt = auto_lanes, np.dtype(dtype)
    rng = np.random.default_rng(9)
    for name, (csc, D) in matrices[dt].items():
        A = rls.DeviceSparseMatrix.from_host(csc, ctx)
        M, N = D.shape
        x, y = _vec(rng, N, dt), _vec(rng, M, dt)
        xd, yd = rls.DeviceVector.from_host(x, ctx), rls.DeviceVector.from_host(y, ctx)
        Ax = (A @ xd).to_host().astype(D.dtype)
        AHy = A.mul_adj_(xd.similar(), yd).to_host().astype(D.dtype)
        lhs, rhs = np.vdot(y.astype(D.dtype), Ax), np.vdot(AHy, x.astype(D.dtype))   # <y, A x> = <A^H y, x>
        scale = np.linalg.norm(D) * np.linalg.norm(x) * np.linalg.norm(y)
        assert abs(lhs - rhs) <= TOL[dt] * max(scale, 1e-300), (name, lhs, rhs)
        At = A.mul_transpose_(xd.similar(), yd).to_host()
        assert _rel(At, D.T @ y.astype(D.dtype)) <= TOL[dt], name
        s2 = A.rownorm2()
        assert s2.dtype == (np.float64 if dt in (np.float64, np.complex128) else np.float32) and s2.n == M
        assert _rel(s2.to_host(), SR.rownorm2(csc)) <= TOL[dt], name
        dense = A.to_dense()
        assert isinstance(dense, rls.DeviceMatrix) and np.array_equal(dense.to_host(), D.astype(dt)), name   # exact
        back = A.to_host()
        assert all(np.array_equal(a, b) for a, b in zip(back[:3], csc[:3])) and back[3] == csc[3]
        # the lazy normal operator: two sparse products
        v = A.normal_operator().mul_(xd.similar(), xd).to_host()
        assert _rel(v, D.conj().T @ (D @ x.astype(D.dtype))) <= TOL[dt], name


# ---- the sparse row sweep through the C ABI ----------------------------------------------------------------------------------
def _banded(M, N, dtype, seed, width=9):
    """row m holds columns m .. m + width - 1 (mod N): consecutive rows share all but one of their columns"""
    mask = np.zeros((M, N), bool)
    for m in range(M):
        mask[m, (m + np.arange(width)) % N] = True
    return SR.from_pattern(mask, dtype, seed)


def _system(kind, M, N, dtype):
    if kind == "banded":
        return _banded(M, N, dtype, 61)
    csc, D = SR.random_csc(M, N, 0.3 if M < 100 else 0.05, dtype, 62)
    mask = D != 0
    mask[3, :] = False   # an empty row
    return SR.from_pattern(mask, dtype, 63)


@pytest.fixture(scope="module")
def systems():
    return {(k, M, N, np.dtype(dt)): _system(k, M, N, dt) for k in ("random", "banded") for M, N in ((40, 24), (300, 520))
            for dt in (np.complex64, np.float64)}


def _device_sweep(rls, ctx, A, X0, U, VL0, rows, denom, eps_w, n_sweeps, lds=(0, 0, 0)):
    """X0: N x nrhs, U, VL0: M x nrhs host arrays; lds = (ldx - N, ldu - M, ldvl - M) of padding, filled with a sentinel.
    Returns (X, VL, the three padded buffers as they came back)."""
    dt = A.dtype
    rt = np.float64 if A.double else np.float32
    nrhs = X0.shape[1]
    sent = dt.type(-77.25)
    bufs, devs = [], []
    for a, pad in zip((X0, U, VL0), lds):
        h = np.full((a.shape[0] + pad, nrhs), sent, dt, order="F")
        h[:a.shape[0], :] = a
        bufs.append(h)
        devs.append(rls.DeviceVector.from_host(h.reshape(-1, order="F"), ctx))
    rows_d = rls.DeviceVector.from_host(np.ascontiguousarray(rows, np.int32).view(np.float32), ctx)
    den_d = rls.DeviceVector.from_host(np.ascontiguousarray(denom, rt), ctx)
    st = ctx.lib.rls_sparse_kaczmarz_sweep(A.handle, nrhs, devs[0].ptr, bufs[0].shape[0], devs[1].ptr, bufs[1].shape[0], devs[2].ptr,
                                           bufs[2].shape[0], rows_d.ptr, den_d.ptr, len(rows), float(eps_w), int(n_sweeps))
    assert st == 0, st
    back = [d.to_host().reshape(b.shape, order="F") for d, b in zip(devs, bufs)]
    return back[0][:X0.shape[0]], back[2][:VL0.shape[0]], back


ORDERS = ("natural", "reversed", "subset", "one row x3", "empty row")


@pytest.mark.parametrize("dtype", (np.complex64, np.float64))
@pytest.mark.parametrize("M,N", ((40, 24), (300, 520)))
def test_kaczmarz_sweep_against_the_float64_restatement(rls, auto_lanes, systems, M, N, dtype):
    ctx, dt = auto_lanes, np.dtype(dtype)
    rng = np.random.default_rng(12)
    lam = 0.05
    for kind, orders in (("random", ORDERS), ("banded", ("natural",))):   # banded, natural: consecutive rows share their columns
        csc, D = systems[(kind, M, N, dt)]
        A = rls.DeviceSparseMatrix.from_host(csc, ctx)
        s2 = SR.rownorm2(csc)
        live = np.flatnonzero(s2 > 0)
        b = (D @ _vec(rng, N, dt).astype(D.dtype)).astype(dt)
        if kind == "random":
            b[3] = 1.5   # (row 3 is empty: A x is zero there, and only a non-zero u[3] makes its step move vl[3])
        x0 = (0.1 * _vec(rng, N, dt)).astype(dt)
        for order in orders:
            rows, sweeps = live, 2
            if order == "reversed":
                rows = live[::-1]
            elif order == "subset":
                rows = rng.permutation(live)[:len(live) // 2]
            elif order == "one row x3":
                rows, sweeps = live[7:8], 3
            elif order == "empty row":
                rows = np.concatenate([live[:5], [3], live[5:11]])   # row 3 has no non-zeros: tau = 0, x untouched, vl updated
                assert s2[3] == 0
            denom = 1.0 / (s2[rows] + lam)
            eps_w = np.sqrt(lam)
            xr, vr = SR.sparse_sweep(csc, x0, b, np.zeros(M), rows, denom, eps_w, sweeps)
            if order == "empty row":
                assert vr[3] != 0
            res = {}
            for lds in (1, 0):
                ctx.tune(sparse_kaczmarz_lds=lds)
                x, vl, _ = _device_sweep(rls, ctx, A, x0[:, None], b[:, None], np.zeros((M, 1), dt), rows, denom, eps_w, sweeps)
                tag = (kind, order, lds)
                assert _rel(x[:, 0], xr) <= TOL[dt], (tag, _rel(x[:, 0], xr))
                assert _rel(vl[:, 0], vr) <= TOL[dt], (tag, _rel(vl[:, 0], vr))
                x2, vl2, _ = _device_sweep(rls, ctx, A, x0[:, None], b[:, None], np.zeros((M, 1), dt), rows, denom, eps_w, sweeps)
                assert x2.tobytes() == x.tobytes() and vl2.tobytes() == vl.tobytes(), tag   # run to run: the same bits
                res[lds] = x[:, 0]
            assert _rel(res[0], res[1].astype(D.dtype)) <= TOL[dt]   # x in LDS and x in global memory


def _long_row_system(kind, dtype):
    """the systems that reach the rest of the sweep kernel (rls_sparse_kaczmarz_sweep runs 256 threads when nnz > 64 M, else 64):
    "wide": 40 x 300 at 60 % -- about 180 per row: the 256-thread form, cross-wave reduction, one pass;
    "wide, two passes": 24 x 600 at 60 % -- about 360 per row: the 256-thread form takes a second pass;
    "one long row": 60 x 300, about five per row and row 17 with 150 -- the 64-thread form takes a second and a third pass"""
    if kind == "wide":
        return SR.random_csc(40, 300, 0.6, dtype, 91)
    if kind == "wide, two passes":
        return SR.random_csc(24, 600, 0.6, dtype, 92)
    rng = np.random.default_rng(93)
    mask = rng.random((60, 300)) < 5 / 300
    mask[np.arange(60), rng.integers(0, 300, 60)] = True   # no empty row
    mask[17, :] = False
    mask[17, rng.choice(300, size=150, replace=False)] = True
    return SR.from_pattern(mask, dtype, 94)


@pytest.mark.parametrize("dtype", (np.complex64, np.float64))
@pytest.mark.parametrize("kind", ("wide", "wide, two passes", "one long row"))
def test_kaczmarz_sweep_long_rows_and_the_four_wave_form(rls, auto_lanes, kind, dtype):
    ctx, dt = auto_lanes, np.dtype(dtype)
    csc, D = _long_row_system(kind, dt)
    M, N = D.shape
    per_row = (D != 0).sum(axis=1)
    nnz = int(per_row.sum())
    if kind == "wide":
        assert nnz > 64 * M and per_row.max() <= 256
    elif kind == "wide, two passes":
        assert nnz > 64 * M and per_row.min() > 256
    else:
        assert nnz <= 64 * M and per_row[17] == 150 and np.sort(per_row)[-2] <= 64
    A = rls.DeviceSparseMatrix.from_host(csc, ctx)
    rng = np.random.default_rng(15)
    lam = 0.05
    s2 = SR.rownorm2(csc)
    b = (D @ _vec(rng, N, dt).astype(D.dtype)).astype(dt)
    x0 = (0.1 * _vec(rng, N, dt)).astype(dt)
    for order in ("natural", "reversed", "one row x3"):
        rows, sweeps = np.arange(M), 2
        if order == "reversed":
            rows = rows[::-1]
        elif order == "one row x3":
            rows, sweeps = np.array([17]), 3
        denom = 1.0 / (s2[rows] + lam)
        xr, vr = SR.sparse_sweep(csc, x0, b, np.zeros(M), rows, denom, np.sqrt(lam), sweeps)
        res = {}
        for lds in (1, 0):
            ctx.tune(sparse_kaczmarz_lds=lds)
            x, vl, _ = _device_sweep(rls, ctx, A, x0[:, None], b[:, None], np.zeros((M, 1), dt), rows, denom, np.sqrt(lam), sweeps)
            tag = (kind, order, lds)
            assert _rel(x[:, 0], xr) <= TOL[dt], (tag, _rel(x[:, 0], xr))
            assert _rel(vl[:, 0], vr) <= TOL[dt], (tag, _rel(vl[:, 0], vr))
            x2, vl2, _ = _device_sweep(rls, ctx, A, x0[:, None], b[:, None], np.zeros((M, 1), dt), rows, denom, np.sqrt(lam), sweeps)
            assert x2.tobytes() == x.tobytes() and vl2.tobytes() == vl.tobytes(), tag   # run to run: the same bits
            res[lds] = x[:, 0]
        assert _rel(res[0], res[1].astype(D.dtype)) <= TOL[dt]
    # three columns at once, padded leading dimensions
    rows = np.arange(M)
    denom = 1.0 / (s2 + lam)
    B = np.stack([b, 0.5 * b, (D @ _vec(rng, N, dt).astype(D.dtype)).astype(dt)], axis=1)
    X0 = np.stack([x0, 0 * x0, -x0], axis=1)
    X, VL, back = _device_sweep(rls, ctx, A, X0, B, np.zeros((M, 3), dt), rows, denom, np.sqrt(lam), 2, lds=(3, 2, 1))
    for j in range(3):
        xr, vr = SR.sparse_sweep(csc, X0[:, j], B[:, j], np.zeros(M), rows, denom, np.sqrt(lam), 2)
        assert _rel(X[:, j], xr) <= TOL[dt] and _rel(VL[:, j], vr) <= TOL[dt], (kind, j)
    assert np.all(back[0][N:, :] == dt.type(-77.25)) and np.all(back[2][M:, :] == dt.type(-77.25))


@pytest.mark.parametrize("dtype", (np.complex64, np.float64))
def test_kaczmarz_sweep_three_columns_with_padded_leading_dimensions(rls, auto_lanes, systems, dtype):
    ctx, dt = auto_lanes, np.dtype(dtype)
    M, N, lam = 40, 24, 0.05
    csc, D = systems[("random", M, N, dt)]
    A = rls.DeviceSparseMatrix.from_host(csc, ctx)
    rng = np.random.default_rng(13)
    s2 = SR.rownorm2(csc)
    rows = np.flatnonzero(s2 > 0)
    denom = 1.0 / (s2[rows] + lam)
    B = np.stack([(D @ _vec(rng, N, dt).astype(D.dtype)).astype(dt) for _ in range(3)], axis=1)
    X0 = np.stack([(0.1 * _vec(rng, N, dt)).astype(dt) for _ in range(3)], axis=1)
    for lds in (1, 0):
        ctx.tune(sparse_kaczmarz_lds=lds)
        X, VL, back = _device_sweep(rls, ctx, A, X0, B, np.zeros((M, 3), dt), rows, denom, np.sqrt(lam), 2, lds=(5, 3, 2))
        for j in range(3):
            xr, vr = SR.sparse_sweep(csc, X0[:, j], B[:, j], np.zeros(M), rows, denom, np.sqrt(lam), 2)
            assert _rel(X[:, j], xr) <= TOL[dt] and _rel(VL[:, j], vr) <= TOL[dt], (lds, j)
        assert np.all(back[0][N:, :] == dt.type(-77.25)) and np.all(back[1][M:, :] == dt.type(-77.25)) and \
            np.all(back[2][M:, :] == dt.type(-77.25))   # the padding came back untouched
        assert np.array_equal(back[1][:M], B)          # u is read only


# ---- solvers through createLinearSolver ---------------------------------------------------------------------------------------
SOLVER_CASES = (((64, 32), np.complex64), ((96, 40), np.float64))


@pytest.fixture(scope="module")
def problems():
    out = {}
    for (M, N), dt in SOLVER_CASES + (((64, 32), np.float64),):
        csc, D = SR.random_csc(M, N, 0.3, dt, 71)
        rng = np.random.default_rng(72)
        b = (D @ _vec(rng, N, dt).astype(D.dtype) + 0.01 * _vec(rng, M, dt)).astype(dt)
        out[((M, N), np.dtype(dt))] = (csc, D, b)
    return out


def _narrow(dt):
    """the working-precision twin for the parity gate's second bound (Float32 / ComplexF32 only)"""
    return dt if np.dtype(dt) in (np.dtype(np.float32), np.dtype(np.complex64)) else None


def _gate(parity, tag, got, ref64, dt, ref32=None):
    if _narrow(dt) is None:
        e = _rel(got, ref64)
        assert e <= 1e-12, (tag, e)
    else:
        parity(tag, got, ref64, ref32)


@pytest.mark.parametrize("shape,dtype", SOLVER_CASES)
@pytest.mark.parametrize("lam", (0.0, 1e-2))
def test_cgnr(rls, auto_lanes, problems, parity, shape, dtype, lam):
    ctx, dt = auto_lanes, np.dtype(dtype)
    csc, D, b = problems[(shape, dt)]
    A = rls.DeviceSparseMatrix.from_host(csc, ctx)
    bd = rls.DeviceVector.from_host(b, ctx)
    kw = dict(iterations=20, relTol=0.0)
    ref = O.CGNR(D, reg=O.L2Regularization(lam), **kw)
    O.solve(ref, b.astype(D.dtype))

    def ref32():
        r = O.CGNR(D.astype(dt), reg=O.L2Regularization(lam), **kw)
        return O.solve(r, b)

    S = rls.createLinearSolver(rls.CGNR, A, reg=rls.L2Regularization(lam), **kw)
    x = rls.solve_(S, bd).to_host()
    assert S.state.iteration == ref.iteration == 20 and not S.state._plan
    _gate(parity, f"sparse CGNR {shape} {dt} lam={lam}", x, ref.x, dt, ref32)
    Sd = rls.createLinearSolver(rls.CGNR, A.to_dense(), reg=rls.L2Regularization(lam), **kw)
    xd = rls.solve_(Sd, bd).to_host()
    _gate(parity, f"dense CGNR on to_dense() {shape} {dt} lam={lam}", xd, ref.x, dt, ref32)
    assert _rel(x, xd.astype(D.dtype)) <= TOL[dt], _rel(x, xd.astype(D.dtype))   # sparse against the same solver on to_dense(), directly
    # the same solve with A's own lazy normal operator named explicitly
    S2 = rls.createLinearSolver(rls.CGNR, A, AHA=A.normal_operator(), reg=rls.L2Regularization(lam), **kw)
    assert np.array_equal(rls.solve_(S2, bd).to_host(), x)


@pytest.mark.parametrize("shape,dtype", SOLVER_CASES)
def test_fista_l1_with_explicit_rho(rls, auto_lanes, problems, parity, shape, dtype):
    ctx, dt = auto_lanes, np.dtype(dtype)
    csc, D, b = problems[(shape, dt)]
    A = rls.DeviceSparseMatrix.from_host(csc, ctx)
    bd = rls.DeviceVector.from_host(b, ctx)
    kw = dict(rho=0.9 / np.linalg.norm(D, 2) ** 2, iterations=20, relTol=0.0)
    ref = O.FISTA(D, reg=O.L1Regularization(0.05), **kw)
    O.solve(ref, b.astype(D.dtype))

    def ref32():
        r = O.FISTA(D.astype(dt), reg=O.L1Regularization(0.05), **kw)
        return O.solve(r, b)

    S = rls.createLinearSolver(rls.FISTA, A, reg=rls.L1Regularization(0.05), **kw)
    x = rls.solve_(S, bd).to_host()
    assert S.state.iteration == 20 and not S.state._plan
    _gate(parity, f"sparse FISTA+L1 {shape} {dt}", x, ref.x, dt, ref32)
    Sd = rls.createLinearSolver(rls.FISTA, A.to_dense(), reg=rls.L1Regularization(0.05), **kw)
    xd = rls.solve_(Sd, bd).to_host()
    _gate(parity, f"dense FISTA+L1 on to_dense() {shape} {dt}", xd, ref.x, dt, ref32)
    assert _rel(x, xd.astype(D.dtype)) <= TOL[dt], _rel(x, xd.astype(D.dtype))   # sparse against the same solver on to_dense(), directly


@pytest.mark.parametrize("dtype", (np.complex64, np.float64))
@pytest.mark.parametrize("shuffle", (False, True))
def test_kaczmarz_l2_positive(rls, auto_lanes, problems, parity, dtype, shuffle):
    ctx, dt = auto_lanes, np.dtype(dtype)
    csc, D, b = problems[((64, 32), dt)]
    A = rls.DeviceSparseMatrix.from_host(csc, ctx)
    bd = rls.DeviceVector.from_host(b, ctx)
    mk = lambda mod: [mod.L2Regularization(0.05), mod.PositiveRegularization()]
    kw = dict(iterations=10, shuffleRows=shuffle, seed=4321)
    Sd = rls.createLinearSolver(rls.Kaczmarz, A.to_dense(), reg=mk(rls), **kw)
    xd = rls.solve_(Sd, bd).to_host()
    order = np.array(Sd.state.usedIndices)   # the order the seed gives (natural without shuffleRows)
    assert shuffle == (not np.array_equal(order, np.arange(len(order))))
    ref = O.Kaczmarz(D, reg=mk(O), iterations=10, order_fn=lambda it: order)
    O.solve(ref, b.astype(D.dtype))

    def ref32():
        r = O.Kaczmarz(D.astype(dt), reg=mk(O), iterations=10, order_fn=lambda it: order)
        return O.solve(r, b)

    S = rls.createLinearSolver(rls.Kaczmarz, A, reg=mk(rls), **kw)
    x = rls.solve_(S, bd).to_host()
    assert np.array_equal(S.state.usedIndices, order) and S.state.iteration == 10
    _gate(parity, f"sparse Kaczmarz L2+Positive {dt} shuffle={shuffle}", x, ref.x, dt, ref32)
    _gate(parity, f"dense Kaczmarz on to_dense() {dt} shuffle={shuffle}", xd, ref.x, dt, ref32)
    assert _rel(x, xd.astype(D.dtype)) <= TOL[dt], _rel(x, xd.astype(D.dtype))   # sparse against the same solver on to_dense(), directly
    conv = rls.solverconvergence(S)["residual"]
    assert abs(conv - np.linalg.norm(D @ x.astype(D.dtype) - b)) <= 1e-4 * np.linalg.norm(b)
    # L2 only and no callbacks: every sweep in one launch, the same sweeps
    S1 = rls.createLinearSolver(rls.Kaczmarz, A, reg=rls.L2Regularization(0.05), iterations=4)
    x1 = rls.solve_(S1, bd).to_host()
    r1 = O.Kaczmarz(D, reg=O.L2Regularization(0.05), iterations=4)
    O.solve(r1, b.astype(D.dtype))
    _gate(parity, f"sparse Kaczmarz L2 {dt}", x1, r1.x, dt, lambda: O.solve(O.Kaczmarz(D.astype(dt), reg=O.L2Regularization(0.05), iterations=4), b))


def test_system_matrix_normalization_callbacks_and_matrix_right_hand_sides(rls, auto_lanes, problems):
    ctx = auto_lanes
    csc, D, b = problems[((64, 32), np.dtype(np.complex64))]
    A = rls.DeviceSparseMatrix.from_host(csc, ctx)
    Ad = A.to_dense()
    bd = rls.DeviceVector.from_host(b, ctx)
    norm = rls.SystemMatrixBasedNormalization()
    want = 0.02 * (np.abs(D) ** 2).sum() / 32
    for T in (rls.CGNR, rls.Kaczmarz):
        S = rls.createLinearSolver(T, A, reg=rls.L2Regularization(0.02), normalizeReg=norm, iterations=3)
        Sd = rls.createLinearSolver(T, Ad, reg=rls.L2Regularization(0.02), normalizeReg=norm, iterations=3)
        assert abs(S.L2.lam - Sd.L2.lam) <= 1e-5 * Sd.L2.lam and abs(S.L2.lam - want) <= 1e-5 * want
    Sf = rls.createLinearSolver(rls.FISTA, A, reg=rls.L1Regularization(0.02), normalizeReg=norm, rho=0.01, iterations=3)
    assert abs(Sf.reg.lam - want) <= 1e-5 * want

    # callbacks fire at iterations 0 .. n, and the last stored solution is the returned one
    for T, kw, n in ((rls.CGNR, dict(relTol=0.0), 5), (rls.FISTA, dict(rho=0.01, relTol=0.0, reg=rls.L1Regularization(0.01)), 5),
                     (rls.Kaczmarz, dict(reg=[rls.L2Regularization(0.05), rls.PositiveRegularization()]), 5)):
        S = rls.createLinearSolver(T, A, iterations=n, **kw)
        seen, store = [], rls.StoreSolutionCallback()
        x = rls.solve_(S, bd, callbacks=[lambda s, it: seen.append(it), store]).to_host()
        assert seen == list(range(n + 1)), (T.__name__, seen)
        assert np.array_equal(store.solutions[-1], x), T.__name__
        S0 = rls.createLinearSolver(T, A, iterations=n, **kw)
        assert np.array_equal(rls.solve_(S0, bd).to_host(), x), T.__name__   # with and without callbacks: the same solve

    # a matrix right-hand side: per column, bit for bit; BatchedState falls back to per-column plans
    rng = np.random.default_rng(14)
    B = np.asfortranarray(np.stack([b, (D @ _vec(rng, 32, np.complex64)).astype(np.complex64), 0.5 * b], axis=1))
    Bd = rls.DeviceMatrix.from_host(B, ctx)
    for T, kw in ((rls.CGNR, dict(iterations=6, relTol=0.0)), (rls.FISTA, dict(iterations=6, rho=0.01, reg=rls.L1Regularization(0.01))),
                  (rls.Kaczmarz, dict(iterations=3, reg=rls.L2Regularization(0.05)))):
        cols = [rls.solve_(rls.createLinearSolver(T, A, **kw), rls.DeviceVector.from_host(np.ascontiguousarray(B[:, j]), ctx)).to_host()
                for j in range(3)]
        for sched in (rls.SequentialState, rls.MultiThreadingState, rls.BatchedState):
            S = rls.createLinearSolver(T, A, **kw)
            xs = rls.solve_(S, Bd, scheduler=sched)
            assert not isinstance(S.state, rls.BatchedState)
            for j in range(3):
                assert np.array_equal(xs[j].to_host(), cols[j]), (T.__name__, sched.__name__, j)


def test_fista_default_rho_from_power_iterations(rls, auto_lanes):
    """The default rho is 0.95 / power_iterations(A^H A), whose stopping rule (src/Utils.jl:262-287, rtol 1e-3) bounds the CHANGE of
    the estimate between two iterations, not its error, and whose start vector is random.  The bound of 1e-3 against the dense
    twin therefore needs a matrix whose iteration contracts fast: all values in the first quadrant give A^H A a dominant
    eigenvalue far above the rest (checked below: r = lambda_2 / lambda_1 < 0.5).  The Rayleigh quotients approach lambda_1 like
    r^(2k), so what is left after a step that moved the estimate by less than 1e-3 is at most r^2 / (1 - r^2) < 1/3 of that:
    each of the two estimates is within 3.4e-4 of lambda_1, and they are within 1e-3 of each other."""
    ctx = auto_lanes
    csc, _ = SR.random_csc(64, 32, 0.3, np.complex64, 81)
    nz = (np.abs(csc[2].real) + 1j * np.abs(csc[2].imag)).astype(np.complex64)
    csc = (csc[0], csc[1], nz, csc[3])
    D = SR.dense(csc)
    s = np.linalg.svd(D, compute_uv=False)
    assert (s[1] / s[0]) ** 2 < 0.5
    A = rls.DeviceSparseMatrix.from_host(csc, ctx)
    rho = rls.createLinearSolver(rls.FISTA, A, reg=rls.L1Regularization(0.01)).state.rho
    rho_dense = rls.createLinearSolver(rls.FISTA, A.to_dense(), reg=rls.L1Regularization(0.01)).state.rho
    exact = 0.95 / s[0] ** 2
    assert abs(rho - rho_dense) <= 1e-3 * rho_dense, (rho, rho_dense)
    assert abs(rho - exact) <= 1e-3 * exact, (rho, exact)


def test_gram_mode_and_refusals(rls, auto_lanes, problems, parity):
    ctx = auto_lanes
    csc, D, b = problems[((64, 32), np.dtype(np.complex64))]
    A = rls.DeviceSparseMatrix.from_host(csc, ctx)
    bd = rls.DeviceVector.from_host(b, ctx)
    # AHA = a dense Gram matrix: the existing Gram path, on A^H b formed by the sparse product
    G = A.to_dense().gram()
    ref = O.CGNR(D, reg=O.L2Regularization(1e-2), iterations=20, relTol=0.0)
    O.solve(ref, b.astype(D.dtype))
    S = rls.createLinearSolver(rls.CGNR, A, AHA=G, reg=rls.L2Regularization(1e-2), iterations=20, relTol=0.0)
    parity("sparse CGNR, dense Gram", rls.solve_(S, bd).to_host(), ref.x,
           lambda: O.solve(O.CGNR(D.astype(np.complex64), reg=O.L2Regularization(1e-2), iterations=20, relTol=0.0), b))
    for T in (rls.ADMM, rls.SplitBregman, rls.OptISTA, rls.POGM, rls.DirectSolver, rls.PseudoInverse):
        with pytest.raises(TypeError, match="sparse"):
            rls.createLinearSolver(T, A, reg=rls.L2Regularization(0.01))
    with pytest.raises(ValueError, match="sparse"):
        rls.createLinearSolver(rls.Kaczmarz, A, reg=rls.L2Regularization(np.full(32, 0.1, np.float32)))
    for bad in (np.eye(32, dtype=np.complex64), "AHA", A, rls.DeviceSparseMatrix.from_host(csc, ctx).normal_operator(),
                A.to_dense().normal_operator()):
        for T in (rls.CGNR, rls.FISTA):
            with pytest.raises(TypeError):
                rls.createLinearSolver(T, A, AHA=bad, rho=0.01) if T is rls.FISTA else rls.createLinearSolver(T, A, AHA=bad)
    mg = rls.multigpu
    for make in (lambda: mg.HipLocalOps(rls, A, 0), lambda: mg.HipFistaOps(rls, A, 0), lambda: mg.HipAdmmOps(rls, A, 0),
                 lambda: mg.CommRowShardedCGNR(rls, [A]), lambda: mg.CommRowShardedFISTA(rls, [A]),
                 lambda: mg.ConcurrentSolves(rls, n_streams=1).upload([A])):
        with pytest.raises(TypeError, match="sparse"):
            make()
    with pytest.raises(TypeError, match="sparse"):
        rls.ProdOp(rls.WeightingOp(bd), A)
