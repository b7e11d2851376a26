"""WaveletOp on the device against the float64 matrix of tests/wavelet_ref.py (checked on its own in tests/test_wavelet_abi.py).

Bars: relative l2 error <= 1e-5 for Float32 / ComplexF32 and <= 1e-12 for Float64 / ComplexF64, the project's parity bars.
The single-workgroup path (the image in one workgroup's LDS) and the general path (one launch per level and dimension) are held
against each other BIT FOR BIT: both form every coefficient with the same chain of one multiply and L - 1 (analysis) or L - 1
(synthesis) explicit fused multiply-adds in the same order (csrc/wavelet.hip, wv_ana / wv_syn), the threshold is one shared
expression, and no sum is reordered by the tiling -- equality holds by construction, so it is asserted."""
import numpy as np
import pytest

import rls_oracle as O
import wavelet_ref as WR

pytestmark = pytest.mark.gpu

FILTERS = ("haar", "db2")
DTYPES = (np.float32, np.complex64, np.float64, np.complex128)
# shapes at which a mechanism can break: n = 2 (the db2 taps wrap twice), 4, full depth, a ragged wave, non-square with J limited
# by the short side, a level limit, not a power of two, a dropped unit dimension
SMALL = [((2,), None), ((4,), None), ((64,), None), ((24,), None), ((2, 2), None), ((8, 4), None), ((16, 16), None),
         ((32, 8), 1), ((96, 40), None), ((1, 16), None)]
LARGE = [((256, 256), np.float32), ((128, 256), np.complex64)]   # 2 N elements do not fit one workgroup's LDS: general path only


def tol(dt):
    return 1e-5 if np.dtype(dt) in (np.dtype(np.float32), np.dtype(np.complex64)) else 1e-12


def rel(a, b, scale=None):
    a, b = np.asarray(a).astype(np.complex128), np.asarray(b).astype(np.complex128)
    n = np.linalg.norm(b) if scale is None else float(scale)
    return float(np.linalg.norm(a - b) / n) if n > 0 else float(np.linalg.norm(a - b))


def data(n, dt, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n)
    if np.dtype(dt).kind == "c":
        x = x + 1j * rng.standard_normal(n)
    return x.astype(dt)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


class paths:
    """runs a block once per path: wavelet_fused = 1 (single workgroup where the image fits) and 0 (general)"""

    def __init__(self, ctx):
        self.ctx = ctx

    def __iter__(self):
        try:
            for fused in (1, 0):
                self.ctx.tune(wavelet_fused=fused)
                yield fused
        finally:
            self.ctx.tune(wavelet_fused=1)


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("wt", FILTERS)
@pytest.mark.parametrize("shape,levels", SMALL, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"J{v}")
def test_forward_adjoint_roundtrip_aliasing_and_path_agreement(rls, ctx, shape, levels, wt, dt):
    W = WR.dense(shape, wt, levels)
    N = W.shape[0]
    x = data(N, dt, N + len(wt))
    op = rls.WaveletOp(shape, wt=wt, levels=levels)
    assert op.levels == (WR.default_levels(shape) if levels is None else levels)
    seen = {}
    for fused in paths(ctx):
        xd = rls.DeviceVector.from_host(x, ctx)
        y = op.mul(xd)
        yh = y.to_host()
        assert rel(yh, W @ x.astype(np.complex128)) <= tol(dt), ("forward", fused)
        assert bits(xd.to_host()) == bits(x)                       # the input of an out-of-place call is left alone
        z = rls.DeviceVector(N, dt, ctx)
        op.mul_adj_(z, xd)
        zh = z.to_host()
        assert rel(zh, W.T @ x.astype(np.complex128)) <= tol(dt), ("adjoint", fused)
        back = rls.DeviceVector(N, dt, ctx)
        op.mul_adj_(back, y)
        assert rel(back.to_host(), x) <= tol(dt), ("round trip", fused)
        a = rls.DeviceVector.from_host(x, ctx)                     # y = x: the same bits as out of place
        op.mul_(a, a)
        assert bits(a.to_host()) == bits(yh), ("aliased forward", fused)
        a = rls.DeviceVector.from_host(x, ctx)
        op.mul_adj_(a, a)
        assert bits(a.to_host()) == bits(zh), ("aliased adjoint", fused)
        seen[fused] = (yh, zh)
    # by construction (module docstring): the two paths give the same bits
    assert bits(seen[1][0]) == bits(seen[0][0]) and bits(seen[1][1]) == bits(seen[0][1])


@pytest.mark.parametrize("wt", FILTERS)
@pytest.mark.parametrize("shape,dt", LARGE, ids=["256x256-f32", "128x256-c64"])
def test_forward_adjoint_past_the_lds_limit(rls, ctx, shape, dt, wt):
    N = int(np.prod(shape))
    x = data(N, dt, 5)
    op = rls.WaveletOp(shape, wt=wt)
    xd = rls.DeviceVector.from_host(x, ctx)
    y = op.mul(xd)
    assert rel(y.to_host(), WR.apply(x, shape, wt)) <= tol(dt)
    z = rls.DeviceVector(N, dt, ctx)
    op.mul_adj_(z, xd)
    assert rel(z.to_host(), WR.apply(x, shape, wt, adjoint=True)) <= tol(dt)
    op.mul_adj_(y, y)                                              # in place, and the round trip
    assert rel(y.to_host(), x) <= tol(dt)
    lam = 0.8
    want = WR.apply(O.prox_l1(WR.apply(x, shape, wt), lam), shape, wt, adjoint=True)
    got = rls.prox_(rls.TransformedRegularization(rls.L1Regularization(lam), op), xd)
    assert got is xd and rel(xd.to_host(), want) <= tol(dt)


def _lams(c):
    a = np.abs(c)
    return {"zero": 0.0, "above": float(2.0 * a.max() + 1.0), "median": float(np.median(a))}


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("wt", FILTERS)
@pytest.mark.parametrize("shape,levels", SMALL, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"J{v}")
def test_prox_wavelet_l1_against_the_oracle_and_the_dense_route(rls, ctx, shape, levels, wt, dt):
    """W' prox_l1(W x, lambda) from the oracle's prox_l1 in float64; lambda = 0 (identity up to rounding), above every coefficient
    (exactly zero) and at the median coefficient magnitude.  The same call with the matrix W itself as a DeviceMatrix trafo (the
    dense route that existed before) is held to the same bar and to the wavelet route, at every shape and element type.
    Errors are relative to the result.  The one exception: n = 2 in Float32 / ComplexF32 at the median lambda, where the median is
    the mean of the two magnitudes and the whole result is the single coefficient (|c_0| - |c_1|) / 2 -- small by cancellation,
    while its absolute error is the one c carries (eps |c|); measured there, Float32 Haar: 1.08e-5 of the result.  That case alone
    is measured on the scale of ||x|| (||result|| <= ||x|| always: the prox shrinks)."""
    W = WR.dense(shape, wt, levels)
    N = W.shape[0]
    x = data(N, dt, 3 * N + 1)
    x64 = x.astype(np.complex128 if np.dtype(dt).kind == "c" else np.float64)
    op = rls.WaveletOp(shape, wt=wt, levels=levels)
    Wd = rls.DeviceMatrix.from_host(np.asfortranarray(W.astype(dt)), ctx)
    for name, lam in _lams(W @ x64).items():
        want = W.T @ O.prox_l1(W @ x64, lam)
        nx = np.linalg.norm(x64) if (N == 2 and name == "median" and tol(dt) == 1e-5) else None
        got = {}
        for fused in paths(ctx):
            xd = rls.DeviceVector.from_host(x, ctx)
            rls.prox_(rls.TransformedRegularization(rls.L1Regularization(lam), op), xd)
            got[fused] = xd.to_host()
            if name == "above":
                assert not got[fused].any(), (name, fused)
            else:
                print(f"prox {shape} {wt} {np.dtype(dt).name} {name} fused={fused}: {rel(got[fused], want):.3e} of the result")
                assert rel(got[fused], want, nx) <= tol(dt), (name, fused)
        assert bits(got[1]) == bits(got[0]), name                 # the two paths: the same bits (module docstring)
        xd = rls.DeviceVector.from_host(x, ctx)
        rls.prox_(rls.TransformedRegularization(rls.L1Regularization(lam), Wd), xd)
        if name == "above":
            assert not xd.to_host().any()
        else:
            print(f"prox {shape} {wt} {np.dtype(dt).name} {name} dense: {rel(xd.to_host(), want):.3e}, to the wavelet route {rel(xd.to_host(), got[1]):.3e}")
            assert rel(xd.to_host(), want, nx) <= tol(dt) and rel(xd.to_host(), got[1], nx) <= tol(dt), name


def test_other_inner_terms_keep_the_three_steps_on_the_device_transform(rls, ctx):
    shape, lam = (16, 16), 0.4
    W = WR.dense(shape, "db2")
    x = data(256, np.complex64, 11)
    want = W.T @ O.prox_l21((W @ x.astype(np.complex128)).copy(), lam, 4)
    xd = rls.DeviceVector.from_host(x, ctx)
    rls.prox_(rls.TransformedRegularization(rls.L21Regularization(lam, slices=4), rls.WaveletOp(shape)), xd)
    assert rel(xd.to_host(), want) <= 1e-5
    n = rls.norm(rls.TransformedRegularization(rls.L1Regularization(lam), rls.WaveletOp(shape)), rls.DeviceVector.from_host(x, ctx))
    assert abs(n - lam * np.abs(W @ x.astype(np.complex128)).sum()) <= 1e-5 * n


def test_prox_is_reproducible_bit_for_bit(rls, ctx):
    x = data(96 * 40, np.complex64, 2)
    reg = rls.TransformedRegularization(rls.L1Regularization(0.7), rls.WaveletOp((96, 40)))
    for fused in paths(ctx):
        runs = []
        for _ in range(2):
            xd = rls.DeviceVector.from_host(x, ctx)
            rls.prox_(reg, xd)
            runs.append(bits(xd.to_host()))
        assert runs[0] == runs[1], fused


def test_refusals_leave_the_vector_untouched(rls, ctx):
    for bad in (dict(shape=(3,), levels=1), dict(shape=(6,), levels=2), dict(shape=(4, 4, 4)), dict(shape=(8,), levels=-1),
                dict(shape=(8,), wt="coif2"), dict(shape=(8, 8), levels=4)):
        with pytest.raises(ValueError):
            rls.WaveletOp(**bad)
    op = rls.WaveletOp((8, 8))
    x = data(48, np.float32, 1)
    xd = rls.DeviceVector.from_host(x, ctx)
    with pytest.raises(ValueError):
        op.mul(xd)
    with pytest.raises(ValueError):
        op.mul_adj_(xd, rls.DeviceVector(64, np.float32, ctx))
    with pytest.raises(ValueError):
        rls.prox_(rls.TransformedRegularization(rls.L1Regularization(0.1), op), xd)
    with pytest.raises(ValueError):
        rls.prox_(rls.TransformedRegularization(rls.L2Regularization(0.1), op), xd)
    assert bits(xd.to_host()) == bits(x)
    # the library refuses bad geometry as well (RLS_E_INVALID), for callers of the C ABI
    import ctypes as C
    w = C.c_void_p()
    for shp, lv, kind in (((6,), 2, 1), ((4, 4, 4), -1, 1), ((8,), -1, 7), ((0,), -1, 1)):
        assert ctx.lib.rls_wavelet_create(ctx.handle, 0, len(shp), (C.c_int64 * len(shp))(*shp), kind, lv, C.byref(w)) == -1
        assert not w.value


# ---- solvers ---------------------------------------------------------------------------------------------------------------------

def _problem(M, shape, wt, dt, seed, sparse=8):
    """b = A x_true with x_true = W' c, c `sparse`-sparse"""
    rng = np.random.default_rng(seed)
    N = int(np.prod(shape))
    A = rng.standard_normal((M, N))
    c = np.zeros(N)
    c[rng.choice(N, sparse, replace=False)] = rng.uniform(1.0, 2.0, sparse) * rng.choice([-1.0, 1.0], sparse)
    if np.dtype(dt).kind == "c":
        A = A + 1j * rng.standard_normal((M, N))
        c = c * np.exp(2j * np.pi * rng.uniform(size=N))
    A = np.asfortranarray((A / np.sqrt(M)).astype(dt))
    xt = WR.apply(c, shape, wt, adjoint=True)
    A64 = A.astype(np.complex128 if np.dtype(dt).kind == "c" else np.float64)
    b = (A64 @ xt).astype(dt)
    rho = 0.95 / np.linalg.norm(A64, 2) ** 2
    return A, A64, b, rho


def _run(rls, ctx, solver, A, b, plan=None, **kw):
    sol = rls.createLinearSolver(solver, rls.DeviceMatrix.from_host(A, ctx), **kw)
    if plan is not None:
        sol.use_device_plan = plan
    x = rls.solve_(sol, rls.DeviceVector.from_host(b, ctx)).to_host()
    return x, sol


def _oracle32(A, b, lam, shape, wt, kw):
    """the oracle's run in the working precision (Float32 A, b, transform and scalars), computed once: the second half of the
    parity gate.  These wide systems (M = 64 or 16 rows for 4096 or 65536 unknowns) lose digits in any Float32 run: the Float32
    oracle itself is 3.8e-5 (64 x 4096) and 1.5e-3 (16 x 65536) from its float64 run after 3 iterations."""
    r = O.FISTA(A, reg=O.TransformedRegularization(O.L1Regularization(lam), WR.SeparableOp(shape, wt, native=True)), **kw)
    O.solve(r, b)
    return r.x


@pytest.mark.parametrize("wt", FILTERS)
def test_fista_wavelet_l1_on_the_device_plan(rls, ctx, parity, wt):
    """128 x 256 ComplexF32 (a 16 x 16 image, underdetermined), 8-sparse in the wavelet basis: iterates 1, 5 and 30 against the
    float64 oracle with the dense W as its trafo, on the plan; the primitive loop (plan switched off on the solver, and refused by
    the library under wavelet_fused = 0) gives the same iterates at the bar"""
    shape, lam = (16, 16), 0.05
    A, A64, b, rho = _problem(128, shape, wt, np.complex64, 21)
    W = WR.dense(shape, wt)
    for it in (1, 5, 30):
        kw = dict(rho=rho, iterations=it, relTol=0.0)
        ref = O.FISTA(A64, reg=O.TransformedRegularization(O.L1Regularization(lam), W), **kw)
        O.solve(ref, b.astype(np.complex128))

        def ref32():
            r = O.FISTA(A, reg=O.TransformedRegularization(O.L1Regularization(lam), W.astype(np.float32)), **kw)
            O.solve(r, b)
            return r.x

        mk = lambda: rls.TransformedRegularization(rls.L1Regularization(lam), rls.WaveletOp(shape, wt=wt))  # noqa: E731
        x, sol = _run(rls, ctx, rls.FISTA, A, b, reg=mk(), **kw)
        assert sol.state._plan, "the device plan was not taken"
        assert sol.state.iteration == it
        parity(f"fista_wavelet_{wt}_it{it}_plan", x, ref.x, ref32)
        xp, solp = _run(rls, ctx, rls.FISTA, A, b, plan=False, reg=mk(), **kw)
        assert not solp.state._plan
        parity(f"fista_wavelet_{wt}_it{it}_primitives", xp, ref.x, ref32)
        assert rel(xp, x) <= 1e-5
        if it == 5:
            ctx.tune(wavelet_fused=0)
            try:
                xg, solg = _run(rls, ctx, rls.FISTA, A, b, reg=mk(), **kw)
            finally:
                ctx.tune(wavelet_fused=1)
            assert not solg.state._plan, "wavelet_fused = 0: the plan must refuse the term"
            parity(f"fista_wavelet_{wt}_it{it}_general", xg, ref.x, ref32)
            assert rel(xg, x) <= 1e-5


def test_swapping_the_wavelet_on_one_solver_between_two_solves(rls, ctx, parity):
    """One solver, one plan, two solves of more than one iteration each (so the step graph is cached and replayed): the regulariser
    is replaced between them by one with ANOTHER filter, then by one with fewer levels -- same lambda, rho and projection.  The old
    operator's handle is freed, the new one may come back at its address; the cached launch carries the old filter and depth as
    arguments and has to go.  Each solve is held to the oracle with ITS operator."""
    shape, lam = (16, 16), 0.05
    A, A64, b, rho = _problem(128, shape, "db2", np.complex64, 28)
    kw = dict(rho=rho, iterations=6, relTol=0.0)
    sol = rls.createLinearSolver(rls.FISTA, rls.DeviceMatrix.from_host(A, ctx),
                                 reg=rls.TransformedRegularization(rls.L1Regularization(lam), rls.WaveletOp(shape, wt="db2")), **kw)
    bd = rls.DeviceVector.from_host(b, ctx)
    seen = []
    for wt, levels in (("db2", None), ("haar", None), ("haar", 1), ("db2", 1), ("db2", None)):
        sol.reg = rls.TransformedRegularization(rls.L1Regularization(lam), rls.WaveletOp(shape, wt=wt, levels=levels))
        x = rls.solve_(sol, bd).to_host()
        assert sol.state._plan and sol.state.iteration == 6
        ref = O.FISTA(A64, reg=O.TransformedRegularization(O.L1Regularization(lam), WR.dense(shape, wt, levels)), **kw)
        O.solve(ref, b.astype(np.complex128))

        def ref32():
            r = O.FISTA(A, reg=O.TransformedRegularization(O.L1Regularization(lam), WR.dense(shape, wt, levels).astype(np.float32)), **kw)
            O.solve(r, b)
            return r.x

        parity(f"fista_wavelet_swap_{wt}_J{levels}", x, ref.x, ref32)
        seen.append(x)
    assert rel(seen[1], seen[0]) > 1e-3 and rel(seen[2], seen[1]) > 1e-3    # (the operators do differ: the check can see a stale one)
    assert bits(seen[4]) == bits(seen[0])


def test_fista_wavelet_l1_with_positive_projection_float32(rls, ctx, parity):
    shape, lam, wt = (16, 16), 0.03, "db2"
    A, A64, b, rho = _problem(128, shape, wt, np.float32, 22)
    W = WR.dense(shape, wt)
    for it in (1, 5, 30):
        kw = dict(rho=rho, iterations=it, relTol=0.0)
        ref = O.FISTA(A64, reg=[O.TransformedRegularization(O.L1Regularization(lam), W), O.PositiveRegularization()], **kw)
        O.solve(ref, b.astype(np.float64))

        def ref32():
            r = O.FISTA(A, reg=[O.TransformedRegularization(O.L1Regularization(lam), W.astype(np.float32)), O.PositiveRegularization()], **kw)
            O.solve(r, b)
            return r.x

        reg = [rls.TransformedRegularization(rls.L1Regularization(lam), rls.WaveletOp(shape)), rls.PositiveRegularization()]
        x, sol = _run(rls, ctx, rls.FISTA, A, b, reg=reg, **kw)
        assert sol.state._plan
        parity(f"fista_wavelet_positive_it{it}", x, ref.x, ref32)


def test_fista_wavelet_l1_under_measurement_normalisation_takes_the_plan(rls, ctx, parity):
    shape, lam = (16, 16), 0.05
    A, A64, b, rho = _problem(128, shape, "db2", np.complex64, 23)
    kw = dict(rho=rho, iterations=5, relTol=0.0)
    ref = O.FISTA(A64, reg=O.TransformedRegularization(O.L1Regularization(lam), WR.dense(shape, "db2")), normalizeReg="measurement", **kw)
    O.solve(ref, b.astype(np.complex128))
    x, sol = _run(rls, ctx, rls.FISTA, A, b, reg=rls.TransformedRegularization(rls.L1Regularization(lam), rls.WaveletOp(shape)),
                  normalizeReg=rls.MeasurementBasedNormalization(), **kw)
    assert sol.state._plan
    parity("fista_wavelet_normalised", x, ref.x)


def test_fista_64x64_image_plan_and_primitives(rls, ctx, parity):
    """64 x 4096 Float32 (a 64 x 64 image), 3 iterations: this image takes the single-workgroup launch (32 KiB of LDS), so the plan
    runs it; the primitive loop -- on the fused prox and, under wavelet_fused = 0, on the general path -- gives the same iterates"""
    shape, lam, wt = (64, 64), 0.02, "db2"
    A, A64, b, rho = _problem(64, shape, wt, np.float32, 24)
    kw = dict(rho=rho, iterations=3, relTol=0.0)
    ref = O.FISTA(A64, reg=O.TransformedRegularization(O.L1Regularization(lam), WR.SeparableOp(shape, wt)), **kw)
    O.solve(ref, b.astype(np.float64))
    ref32 = _oracle32(A, b, lam, shape, wt, kw)
    mk = lambda: rls.TransformedRegularization(rls.L1Regularization(lam), rls.WaveletOp(shape, wt=wt))  # noqa: E731
    x, sol = _run(rls, ctx, rls.FISTA, A, b, reg=mk(), **kw)
    assert sol.state._plan
    parity("fista_wavelet_64x64_plan", x, ref.x, ref32)
    for fused in paths(ctx):
        xp, solp = _run(rls, ctx, rls.FISTA, A, b, plan=False if fused else None, reg=mk(), **kw)
        assert not solp.state._plan
        parity(f"fista_wavelet_64x64_primitives_fused{fused}", xp, ref.x, ref32)
        assert rel(xp, x) <= 1e-5


def test_fista_image_past_the_lds_limit_falls_back_to_the_primitives(rls, ctx, parity):
    """16 x 65536 Float32 (a 256 x 256 image: 512 KiB for its two copies), 3 iterations: rls_fista_set_reg_wavelet answers
    RLS_E_UNSUPPORTED and the solver drives the primitives, the prox on the general path"""
    shape, lam, wt = (256, 256), 0.02, "db2"
    A, A64, b, rho = _problem(16, shape, wt, np.float32, 25)
    kw = dict(rho=rho, iterations=3, relTol=0.0)
    ref = O.FISTA(A64, reg=O.TransformedRegularization(O.L1Regularization(lam), WR.SeparableOp(shape, wt)), **kw)
    O.solve(ref, b.astype(np.float64))
    x, sol = _run(rls, ctx, rls.FISTA, A, b, reg=rls.TransformedRegularization(rls.L1Regularization(lam), rls.WaveletOp(shape, wt=wt)), **kw)
    assert not sol.state._plan and sol.state.iteration == 3
    x32 = _oracle32(A, b, lam, shape, wt, kw)
    parity("fista_wavelet_256x256_primitives", x, ref.x, x32)
    # there is no plan to hold these iterates to: they are held to the working-precision oracle at the bar instead (the two runs
    # round differently but lose the same digits to the conditioning of the system)
    print(f"fista 256x256: device vs Float32 oracle {rel(x, x32):.3e}")
    assert rel(x, x32) <= 1e-5


def test_fista_float64_runs_on_the_primitives(rls, ctx):
    shape, lam = (16, 16), 0.05
    A, A64, b, rho = _problem(128, shape, "db2", np.complex128, 26)
    kw = dict(rho=rho, iterations=30, relTol=0.0)
    ref = O.FISTA(A64, reg=O.TransformedRegularization(O.L1Regularization(lam), WR.dense(shape, "db2")), **kw)
    O.solve(ref, b)
    x, sol = _run(rls, ctx, rls.FISTA, A, b, reg=rls.TransformedRegularization(rls.L1Regularization(lam), rls.WaveletOp(shape)), **kw)
    assert not sol.state._plan
    assert rel(x, ref.x) <= 1e-12


def test_optista_and_admm_reach_the_nested_prox(rls, ctx, parity):
    shape, lam = (16, 16), 0.05
    A, A64, b, rho = _problem(128, shape, "db2", np.complex64, 27)
    W = WR.dense(shape, "db2")
    mk = lambda: rls.TransformedRegularization(rls.L1Regularization(lam), rls.WaveletOp(shape))  # noqa: E731
    mko = lambda Wm: O.TransformedRegularization(O.L1Regularization(lam), Wm)  # noqa: E731
    kw = dict(rho=rho, iterations=3, relTol=0.0)
    ref = O.OptISTA(A64, reg=mko(W), **kw)
    O.solve(ref, b.astype(np.complex128))

    def ref32():
        r = O.OptISTA(A, reg=mko(W.astype(np.float32)), **kw)
        O.solve(r, b)
        return r.x

    x, _ = _run(rls, ctx, rls.OptISTA, A, b, reg=mk(), **kw)
    parity("optista_wavelet", x, ref.x, ref32)
    kwa = dict(rho=0.1, iterations=3, iterationsCG=5, tolInner=1e-5)
    refa = O.ADMM(A64, reg=mko(W), **kwa)
    O.solve(refa, b.astype(np.complex128))

    def refa32():
        r = O.ADMM(A, reg=mko(W.astype(np.float32)), **kwa)
        O.solve(r, b)
        return r.x

    xa, _ = _run(rls, ctx, rls.ADMM, A, b, reg=mk(), **kwa)
    parity("admm_wavelet", xa, refa.x, refa32)
