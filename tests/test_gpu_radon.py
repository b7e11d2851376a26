"""GPU tests of RadonOp (csrc/radon.hip) and of CGNR and FISTA on it.  Every comparison is against
tests/radon_ref.py (checked on the CPU by tests/test_radon_abi.py) through the `parity` gate on the scale of the result: 1e-5 relative
to the float64 restatement for Float32 / ComplexF32, 1e-12 for Float64 / ComplexF64, the Float32 restatement as the own-error
yardstick.  "Bit for bit" compares the bytes.

Every test angle is either snapped onto an axis or has min(|cos|, |sin|) >= 0.05: the weight has slope 1 / (mn mx), and a Float32
near-axis angle that is not snapped loses accuracy like eps extent / mn (the documented property; not tested away here).

Matrix entries are held one by one.  At a snapped angle every operand is a half-integer, 0 or +-1: equality.  Elsewhere the bound is
rounding analysis of w = clamp((hi - |t - (xr c + yr s)|) / mn, 0, 1) / mx with unit roundoff u = eps / 2: the table entries and the
products perturb xr c + yr s by at most 3 u (|xr c| + |yr s|), the difference by u (|t| + |xr c| + |yr s|), hi and hi - d by
2 u hi, and the two scalings add 5 u to a value of at most 1 / mx; all of it doubled:
    |w - w_ref| <= 4 eps (|t| + |xr c| + |yr s| + hi) / (mn mx) + 4 eps / mx."""
import functools

import numpy as np
import pytest

import radon_ref as RR
import rls_oracle as O

pytestmark = pytest.mark.gpu

TOL = {np.dtype(np.float32): 1e-5, np.dtype(np.complex64): 1e-5, np.dtype(np.float64): 1e-12, np.dtype(np.complex128): 1e-12}
DTYPES = (np.float32, np.complex64, np.float64, np.complex128)
SHAPES = ((1, 1), (2, 2), (3, 5), (8, 8), (16, 12), (31, 33), (64, 64))
# snapped axes and their exact ties, |c| = |s|, near-axis angles, a negative angle, angles above pi
ANGLES = (0.0, np.pi / 2, np.pi, np.pi / 4, 3 * np.pi / 4, 0.05, np.pi / 2 - 0.05, -0.4, 3.5, 1.0, 2.0, 0.3, 2.9)
LANES = (1, 4, 16, 64)


def _detectors(shape):
    """the default; 1 and 5 crop; 63, 64, 65 sit at a wave's edge; default + 6 has rays that see nothing"""
    d = RR.default_detectors(shape)
    return (d, 1, 5, 63, 64, 65, d + 6)


def _real(dt):
    return np.dtype(np.float64 if np.dtype(dt) in (np.dtype(np.float64), np.dtype(np.complex128)) else np.float32)


@functools.lru_cache(maxsize=16)
def _ref(shape, angles, D, prec):
    """the restatement's matrix, built once per (shape, angles, D, precision) and shared; never modified"""
    A = RR.dense(shape, angles, D, prec)
    A.setflags(write=False)
    return A


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _vec(rng, n, dtype):
    v = rng.standard_normal(n)
    if np.dtype(dtype).kind == "c":
        v = v + 1j * rng.standard_normal(n)
    return v.astype(dtype)


def _own(dt, fn):
    """the Float32 restatement is the own-error yardstick of a Float32 / ComplexF32 result; the double types are held to 1e-12 alone"""
    return fn if _real(dt) == np.dtype(np.float32) else None


def _apply(rls, ctx, fn, x, n_out):
    """fn(out, in) on device vectors, out filled with NaN (beta = 0 must not read it), twice: the two runs give the same bits"""
    xd = rls.DeviceVector.from_host(x, ctx)
    y1 = fn(rls.DeviceVector(n_out, x.dtype, ctx).fill_(np.nan), xd).to_host()
    y2 = fn(rls.DeviceVector(n_out, x.dtype, ctx).fill_(np.nan), xd).to_host()
    assert _bits(y1, y2)
    return y1


@pytest.fixture()
def auto_lanes(ctx):
    ctx.tune(radon_lanes=0)
    yield ctx
    ctx.tune(radon_lanes=0)


def _entry_bound(shape, D, dt):
    """the bound of the module docstring for every entry (M x N); 0 in the rows of the snapped angles"""
    eps = float(np.finfo(_real(dt)).eps)
    n1, n2 = shape
    c, s, mx, mn, hi = RR.table(ANGLES)
    xr = np.repeat(np.arange(n1)[None, :], n2, axis=0).ravel() - (n1 - 1) / 2   # column-major pixel order: i fastest
    yr = np.repeat(np.arange(n2)[:, None], n1, axis=1).ravel() - (n2 - 1) / 2
    t = np.abs(np.arange(D) - (D - 1) / 2)
    out = np.zeros((D * len(ANGLES), n1 * n2))
    for q in range(len(ANGLES)):
        if mn[q] > 0:
            mag = t[:, None] + (np.abs(xr * c[q]) + np.abs(yr * s[q]))[None, :] + hi[q]
            out[q * D:(q + 1) * D] = 4 * eps * mag / (mn[q] * mx[q]) + 4 * eps / mx[q]
    return out


# ---- the operator grid -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dtype", [(s_, d_) for s_ in SHAPES for d_ in DTYPES])
def test_operator_grid(rls, auto_lanes, parity, shape, dtype):
    ctx, dt = auto_lanes, np.dtype(dtype)
    prec = _real(dt)
    n = shape[0] * shape[1]
    rng = np.random.default_rng(41)
    for D in _detectors(shape):
        A64, A32 = _ref(shape, ANGLES, D, np.dtype(np.float64)), _ref(shape, ANGLES, D, np.dtype(np.float32))
        m = A64.shape[0]
        A = rls.RadonOp(dt, ANGLES, shape, detectors=None if D == RR.default_detectors(shape) else D, ctx=ctx)
        assert (A.M, A.N, A.size(1), A.size(2), A.shape, A.detectors, A.image_shape) == (m, n, m, n, (m, n), D, shape)
        assert np.array_equal(A.angles, np.asarray(ANGLES))
        tag = f"RadonOp {dt} {shape} D={D}"
        x, y = _vec(rng, n, dt), _vec(rng, m, dt)
        c32 = np.complex64 if dt.kind == "c" else np.float32
        # forward and adjoint against the restatement
        Ax = _apply(rls, ctx, A.mul_, x, m)
        parity(tag + " forward", Ax, A64 @ x.astype(np.complex128 if dt.kind == "c" else np.float64),
               _own(dt, lambda: A32 @ x.astype(c32)), tol=TOL[dt])
        if D == RR.default_detectors(shape) + 6:   # three bins on either side lie more than 1 > hi beyond every pixel: exact zeros
            dark = np.tile((np.arange(D) < 3) | (np.arange(D) >= D - 3), len(ANGLES))
            assert not A64[dark].any() and not np.any(Ax[dark]) and not np.any(np.signbit(Ax[dark].real))
        ATy = _apply(rls, ctx, A.mul_adj_, y, n)
        parity(tag + " adjoint", ATy, A64.T @ y.astype(np.complex128 if dt.kind == "c" else np.float64),
               _own(dt, lambda: A32.T @ y.astype(c32)), tol=TOL[dt])
        assert _bits(_apply(rls, ctx, A.mul_transpose_, y, n), ATy)   # the weights are real: A^T = A^H
        # the dot test, the difference on the scale ||x|| ||y||
        lhs, rhs = np.vdot(y.astype(np.complex128), Ax.astype(np.complex128)), np.vdot(ATy.astype(np.complex128), x.astype(np.complex128))
        parity(tag + " dot test", np.array([lhs]), np.array([rhs]), tol=TOL[dt], scale=np.linalg.norm(x) * np.linalg.norm(y))
        # the alpha / beta forms
        for alpha, beta in ((2.0, 0.5), (-1.5, 0.0)) + (((2 - 1j), (1 + 2j)),) * (dt.kind == "c"):
            y0, x0 = _vec(rng, m, dt), _vec(rng, n, dt)
            wide = np.complex128 if dt.kind == "c" else np.float64
            got = A.mul_(rls.DeviceVector.from_host(y0, ctx), rls.DeviceVector.from_host(x, ctx), alpha, beta).to_host()
            parity(tag + f" forward alpha={alpha} beta={beta}", got, alpha * (A64 @ x.astype(wide)) + beta * y0.astype(wide),
                   _own(dt, lambda: (alpha * (A32 @ x.astype(c32)) + beta * y0).astype(c32)), tol=TOL[dt])
            for adj in (A.mul_adj_, A.mul_transpose_):
                got = adj(rls.DeviceVector.from_host(x0, ctx), rls.DeviceVector.from_host(y, ctx), alpha, beta).to_host()
                parity(tag + f" adjoint alpha={alpha} beta={beta}", got, alpha * (A64.T @ y.astype(wide)) + beta * x0.astype(wide),
                       _own(dt, lambda: (alpha * (A32.T @ y.astype(c32)) + beta * x0).astype(c32)), tol=TOL[dt])
        # the matrix, entry by entry
        Ad = A.to_dense()
        assert (Ad.M, Ad.N) == (m, n)
        got = Ad.to_host()
        assert got.dtype == dt and (dt.kind != "c" or not np.any(got.imag))
        got = got.real.astype(np.float64)
        bound = _entry_bound(shape, D, dt)
        snapped = np.repeat(RR.table(ANGLES)[3] == 0, D)
        assert np.array_equal(got[snapped], _ref(shape, ANGLES, D, prec)[snapped].astype(np.float64)), tag
        excess = np.abs(got - A64) - bound
        assert excess.max() <= 0, (tag, np.unravel_index(excess.argmax(), excess.shape), excess.max())
        # the normal product is the two calls, bit for bit
        v = _apply(rls, ctx, A.mul_normal_, x, n)
        t = A.mul_(rls.DeviceVector(m, dt, ctx), rls.DeviceVector.from_host(x, ctx))
        two = A.mul_adj_(rls.DeviceVector(n, dt, ctx), t).to_host()
        assert _bits(v, two), tag
        assert _bits(_apply(rls, ctx, A.normal_operator().mul_, x, n), v), tag
        xd = rls.DeviceVector.from_host(x, ctx)   # in place
        assert _bits(A.mul_normal_(xd, xd).to_host(), v), tag
    with pytest.raises(ValueError):
        A.mul_(rls.DeviceVector(3, dt, ctx), rls.DeviceVector(n + 1, dt, ctx))
    with pytest.raises(TypeError):
        A.mul_(rls.DeviceVector(A.M, np.complex64 if dt != np.complex64 else np.float32, ctx), rls.DeviceVector(n, dt, ctx))


def _many_angles(count):
    """1, 5 or 70 angles, every one snapped or with mn >= 0.05"""
    if count <= len(ANGLES):
        return tuple(ANGLES[:count])
    first = np.linspace(0.06, np.pi / 2 - 0.06, count // 2)
    return tuple(np.concatenate([first, first + np.pi / 2]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("count", [1, 5, 70])
def test_adjoint_at_every_lane_count(rls, auto_lanes, parity, dtype, count):
    ctx, dt = auto_lanes, np.dtype(dtype)
    shape = (16, 12)
    angles = _many_angles(count)
    assert len(angles) == count
    D = RR.default_detectors(shape)
    A64, A32 = _ref(shape, angles, D, np.dtype(np.float64)), _ref(shape, angles, D, np.dtype(np.float32))
    A = rls.RadonOp(dt, angles, shape, ctx=ctx)
    rng = np.random.default_rng(43)
    y = _vec(rng, A.M, dt)
    x0 = _vec(rng, A.N, dt)
    wide, c32 = (np.complex128, np.complex64) if dt.kind == "c" else (np.float64, np.float32)
    for L in LANES:
        ctx.tune(radon_lanes=L)
        assert A.lanes() == L
        got = _apply(rls, ctx, A.mul_adj_, y, A.N)
        parity(f"RadonOp adjoint {dt} {count} angles L={L}", got, A64.T @ y.astype(wide), _own(dt, lambda: A32.T @ y.astype(c32)), tol=TOL[dt])
        acc = A.mul_adj_(rls.DeviceVector.from_host(x0, ctx), rls.DeviceVector.from_host(y, ctx), 0.5, -2.0).to_host()
        parity(f"RadonOp adjoint {dt} {count} angles L={L} alpha beta", acc, 0.5 * (A64.T @ y.astype(wide)) - 2.0 * x0.astype(wide),
               _own(dt, lambda: (0.5 * (A32.T @ y.astype(c32)) - 2.0 * x0).astype(c32)), tol=TOL[dt])
        x = _vec(rng, A.N, dt)
        v = _apply(rls, ctx, A.mul_normal_, x, A.N)
        t = A.mul_(rls.DeviceVector(A.M, dt, ctx), rls.DeviceVector.from_host(x, ctx))
        assert _bits(A.mul_adj_(rls.DeviceVector(A.N, dt, ctx), t).to_host(), v)


def test_lanes_forced_and_automatic(rls, auto_lanes):
    """rls_tune_set("radon_lanes", L) forces L; 0 is the rule on the pixel count (rd_pick_lanes, from profiles/radon.txt); anything
    else is refused"""
    ctx = auto_lanes
    for shape, want in (((8, 8), 64), ((64, 64), 64), ((65, 64), 16), ((128, 128), 16), ((129, 128), 4), ((256, 256), 4), ((257, 256), 1)):
        A = rls.RadonOp(np.float32, [0.3], shape, detectors=3, ctx=ctx)
        assert A.lanes() == want, (shape, A.lanes())
        for L in LANES:
            ctx.tune(radon_lanes=L)
            assert A.lanes() == L
        ctx.tune(radon_lanes=0)
    for bad in (2, 3, 8, 32, 128, -1):
        with pytest.raises(rls.RLSError):
            ctx.tune(radon_lanes=bad)
    assert A.lanes() == 1


# ---- solvers -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ct_problem():
    """a 16 x 12 phantom of two rectangles under 7 angles in [0, pi).  Built once, shared, never modified."""
    shape = (16, 12)
    angles = tuple(np.linspace(0.0, np.pi, 7, endpoint=False))
    img = np.zeros(shape)
    img[4:10, 2:6] = 1.0
    img[8:14, 7:10] = 0.5
    D = RR.default_detectors(shape)
    A = RR.dense(shape, angles, D)
    A.setflags(write=False)
    return shape, angles, A, A @ img.ravel(order="F")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_cgnr_l2(rls, auto_lanes, parity, ct_problem, dtype):
    """3 iterations: Float32 CGNR drifts from Float64 by 4e-7 after 3 iterations of this problem and by 4e-3 after 20 (the restatement on
    the CPU), so the oracle comparison is the short run and the long run gets the residual check"""
    ctx, dt = auto_lanes, np.dtype(dtype)
    shape, angles, D, b = ct_problem
    A = rls.RadonOp(dt, angles, shape, ctx=ctx)
    bd = rls.DeviceVector.from_host(b.astype(dt), ctx)
    kw = dict(iterations=3, relTol=0.0)
    S = rls.createLinearSolver(rls.CGNR, A, reg=rls.L2Regularization(0.05), **kw)
    x = rls.solve_(S, bd).to_host()
    assert not S.state._plan
    ref = O.CGNR(D, reg=O.L2Regularization(0.05), **kw)
    O.solve(ref, b)
    assert S.state.iteration == ref.iteration == 3
    parity(f"CGNR+L2 on RadonOp {dt}", x, ref.x,
           _own(dt, lambda: O.solve(O.CGNR(D.astype(np.float32), reg=O.L2Regularization(0.05), **kw), b.astype(np.float32))), tol=TOL[dt])
    S2 = rls.createLinearSolver(rls.CGNR, A, AHA=A.normal_operator(), reg=rls.L2Regularization(0.05), **kw)
    assert _bits(rls.solve_(S2, bd).to_host(), x) and not S2.state._plan
    S3 = rls.createLinearSolver(rls.CGNR, A, reg=rls.L2Regularization(0.05), iterations=20, relTol=0.0)
    x20 = rls.solve_(S3, bd)
    r = A.mul_(rls.DeviceVector(A.M, dt, ctx), x20).to_host() - b
    assert np.all(np.isfinite(x20.to_host())) and np.linalg.norm(r) < np.linalg.norm(b), (np.linalg.norm(r), np.linalg.norm(b))


def test_fista_tv_positive(rls, auto_lanes, parity, ct_problem):
    ctx = auto_lanes
    shape, angles, D, b = ct_problem
    A = rls.RadonOp(np.float32, angles, shape, ctx=ctx)
    kw = dict(iterations=20, rho=0.95 / np.linalg.norm(D, 2) ** 2, relTol=0.0)
    S = rls.createLinearSolver(rls.FISTA, A, reg=[rls.TVRegularization(0.01, shape=shape), rls.PositiveRegularization()], **kw)
    x = rls.solve_(S, rls.DeviceVector.from_host(b.astype(np.float32), ctx)).to_host()
    assert S.state.iteration == 20 and not S.state._plan
    mk = lambda: [O.TVRegularization(0.01, shape=shape), O.PositiveRegularization()]
    ref = O.FISTA(D, reg=mk(), **kw)
    O.solve(ref, b)
    parity("FISTA+TV+Positive on RadonOp Float32", x, ref.x,
           lambda: O.solve(O.FISTA(D.astype(np.float32), reg=mk(), **kw), b.astype(np.float32)))


def test_callbacks_and_matrix_right_hand_sides(rls, auto_lanes, ct_problem):
    ctx, dt = auto_lanes, np.dtype(np.float32)
    shape, angles, D, b = ct_problem
    A = rls.RadonOp(dt, angles, shape, ctx=ctx)
    bd = rls.DeviceVector.from_host(b.astype(dt), ctx)
    rho = 0.95 / np.linalg.norm(D, 2) ** 2
    for T, kw in ((rls.CGNR, dict(relTol=0.0, reg=rls.L2Regularization(0.05))), (rls.FISTA, dict(rho=rho, relTol=0.0, reg=rls.L1Regularization(0.01)))):
        S = rls.createLinearSolver(T, A, iterations=5, **kw)
        seen, store = [], rls.StoreSolutionCallback()
        x = rls.solve_(S, bd, callbacks=[lambda s, it: seen.append(it), store]).to_host()
        assert seen == list(range(6)), (T.__name__, seen)   # iterations + 1 calls
        assert _bits(store.solutions[-1], x) and not S.state._plan
        assert _bits(rls.solve_(rls.createLinearSolver(T, A, iterations=5, **kw), bd).to_host(), x)
        B = np.asfortranarray(np.stack([b, 0.5 * b[::-1]], axis=1).astype(dt))
        cols = [rls.solve_(rls.createLinearSolver(T, A, iterations=5, **kw),
                           rls.DeviceVector.from_host(np.ascontiguousarray(B[:, j]), ctx)).to_host() for j in range(2)]
        for sched in (rls.SequentialState, rls.MultiThreadingState, rls.BatchedState):
            S = rls.createLinearSolver(T, A, iterations=5, **kw)
            xs = rls.solve_(S, rls.DeviceMatrix.from_host(B, ctx), scheduler=sched)
            assert not isinstance(S.state, rls.BatchedState)
            for j in range(2):
                assert _bits(xs[j].to_host(), cols[j]), (T.__name__, sched.__name__, j)


def test_reference_example_at_its_own_size(rls, auto_lanes):
    """docs/src/literate/examples/computed_tomography.jl: 256 x 256 Float32, 256 angles in [0, pi), CGNR + L2(0.001), 20 iterations.
    No oracle at this size: it finishes, is finite and lowers ||A x - b|| below ||b||."""
    ctx = auto_lanes
    shape = (256, 256)
    yy, xx = np.mgrid[-1:1:256j, -1:1:256j]
    img = ((xx ** 2 + (yy / 1.3) ** 2 < 0.6).astype(np.float32) + 0.5 * ((xx - 0.2) ** 2 + (yy + 0.1) ** 2 < 0.05)).astype(np.float32)
    angles = np.linspace(0.0, np.pi, 256, endpoint=False)
    A = rls.RadonOp(np.float32, angles, shape, ctx=ctx)
    assert A.shape == (256 * RR.default_detectors(shape), 65536)
    b = A.mul_(rls.DeviceVector(A.M, np.float32, ctx), rls.DeviceVector.from_host(img.ravel(order="F"), ctx))
    S = rls.createLinearSolver(rls.CGNR, A, reg=rls.L2Regularization(0.001), iterations=20)
    x = rls.solve_(S, b)
    assert not S.state._plan
    bh = b.to_host()
    r = A.mul_(rls.DeviceVector(A.M, np.float32, ctx), x).to_host() - bh
    assert np.all(np.isfinite(x.to_host())) and np.linalg.norm(r) < np.linalg.norm(bh), (np.linalg.norm(r), np.linalg.norm(bh))
