"""GPU tests of the matrix-free operators (csrc/fft.hip) and of CGNR and FISTA on them.  Every comparison is
against tests/matfree_ref.py (checked on the CPU by tests/test_matfree_abi.py) through the `parity` gate: 1e-5 relative to the
float64 restatement for Float32 / ComplexF32, 1e-12 for Float64 / ComplexF64 (as tests/test_gpu_float64.py holds them).  Sampling is
copies and exact 0 / 1 products: exact equality.  "Bit for bit" compares the bytes."""
import numpy as np
import pytest

import matfree_ref as MR
import rls_oracle as O

pytestmark = pytest.mark.gpu

TOL = {np.dtype(np.float32): 1e-5, np.dtype(np.complex64): 1e-5, np.dtype(np.float64): 1e-12, np.dtype(np.complex128): 1e-12}
DTYPES = (np.float32, np.complex64, np.float64, np.complex128)
CPLX = (np.complex64, np.complex128)
# the longest line: 64 KiB of LDS per workgroup on the general path (csrc/fft.hip, FFT_LINE_LDS)
MAX_LINE = {np.dtype(np.complex64): 8192, np.dtype(np.complex128): 4096}
# the sampling kernels are grid-stride loops of at most 2048 workgroups of 256 threads (MF_MAX_GRID, MF_THREADS): from 524288
# elements on a thread takes a second pass
GRID_SPAN = 2048 * 256
FLAGS = [(True, True), (True, False), (False, True), (False, False)]


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _vec(rng, n, dtype):
    v = rng.standard_normal(n)
    if np.dtype(dtype).kind == "c":
        v = v + 1j * rng.standard_normal(n)
    return v.astype(dtype)


def _ints(rng, n, dtype):
    """small integers: every product and sum of the alpha / beta form is exact in every element type"""
    v = rng.integers(-8, 9, n).astype(np.float64)
    if np.dtype(dtype).kind == "c":
        v = v + 1j * rng.integers(-8, 9, n)
    return v.astype(dtype)


@pytest.fixture()
def fused(ctx):
    """fft_fused = 2: the single-workgroup path for every image that fits (the default, 1, sends only small images there)"""
    ctx.tune(fft_fused=2)
    yield ctx
    ctx.tune(fft_fused=1)


def _apply(rls, ctx, fn, x, n_out):
    """fn(out, in) on device vectors, twice: the two runs must give the same bits"""
    xd = rls.DeviceVector.from_host(x, ctx)
    y1 = fn(rls.DeviceVector(n_out, x.dtype, ctx).fill_(np.nan), xd).to_host()
    y2 = fn(rls.DeviceVector(n_out, x.dtype, ctx).fill_(np.nan), xd).to_host()
    assert _bits(y1, y2)
    return y1


# ---- sampling ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_sampling_forward_adjoint_normal_and_alpha_beta_are_exact(rls, ctx, dtype):
    dt = np.dtype(dtype)
    rng = np.random.default_rng(5)
    n = 48
    big = GRID_SPAN + 1000   # a second pass of every grid-stride loop, over m as over N
    cases = [((6, 8), np.array([5], np.int32)), ((6, 8), rng.permutation(n).astype(np.int32)), ((6, 8), MR.pattern(n, n // 3, 1)),
             ((big,), rng.permutation(big).astype(np.int32))]
    assert {0, n - 1} <= set(cases[2][1].tolist())
    for shape, pat in cases:
        N, m = int(np.prod(shape)), pat.size
        S = rls.SamplingOp(dt, pat, shape, ctx)
        assert (S.M, S.N, S.size(1), S.size(2), S.shape) == (m, N, m, N, (m, N))
        x, y = _ints(rng, N, dt), _ints(rng, m, dt)
        assert np.array_equal(_apply(rls, ctx, S.mul_, x, m), MR.sampling(x, pat))
        assert _bits(_apply(rls, ctx, S.mul_adj_, y, N), MR.sampling_adj(y, pat, N))
        assert np.array_equal(_apply(rls, ctx, S.mul_normal_, x, N), (MR.sampling_mask(pat, N) * x).astype(dt))
        assert np.array_equal(_apply(rls, ctx, S.normal_operator().mul_, x, N), (MR.sampling_mask(pat, N) * x).astype(dt))
        for alpha, beta in ((2.0, 0.5), (-1.0, 0.0)) + (((2 - 1j), (1 + 2j)),) * (dt.kind == "c"):
            y0, x0 = _ints(rng, m, dt), _ints(rng, N, dt)
            got = S.mul_(rls.DeviceVector.from_host(y0, ctx), rls.DeviceVector.from_host(x, ctx), alpha, beta).to_host()
            assert np.array_equal(got, (alpha * MR.sampling(x, pat) + beta * y0).astype(dt)), (shape, alpha, beta)
            for adj in (S.mul_adj_, S.mul_transpose_):
                got = adj(rls.DeviceVector.from_host(x0, ctx), rls.DeviceVector.from_host(y, ctx), alpha, beta).to_host()
                assert np.array_equal(got, (alpha * MR.sampling_adj(y, pat, N) + beta * x0).astype(dt)), (shape, alpha, beta)
    with pytest.raises(ValueError):
        S.mul_(rls.DeviceVector(3, dt, ctx), rls.DeviceVector(big, dt, ctx))


# ---- FFT ---------------------------------------------------------------------------------------------------------------------------
def _fft_case(rls, ctx, parity, dt, shape, shift, unitary, rng, expect_variant=None):
    """forward and adjoint on the path the shape takes and, where that is the single-workgroup one, again on the general path:
    the same bits.  Returns the operator."""
    n = int(np.prod(shape))
    x = _vec(rng, n, dt)
    ctx.tune(fft_fused=2)
    F = rls.FFTOp(dt, shape, shift, unitary, ctx)
    if expect_variant is not None:
        assert F.variant() == expect_variant, (shape, F.variant())
    tag = f"FFTOp {dt} {shape} shift={shift} unitary={unitary}"
    y = _apply(rls, ctx, F.mul_, x, n)
    parity(tag + " forward", y, MR.fft(x, shape, shift, unitary), tol=TOL[dt])
    z = _apply(rls, ctx, F.mul_adj_, x, n)
    parity(tag + " adjoint", z, MR.fft_adj(x, shape, shift, unitary), tol=TOL[dt])
    xd = rls.DeviceVector.from_host(x, ctx)   # in place
    assert _bits(F.mul_(xd, xd).to_host(), y)
    if F.variant() == 1:
        ctx.tune(fft_fused=0)
        assert F.variant() == 0
        assert _bits(_apply(rls, ctx, F.mul_, x, n), y), tag
        assert _bits(_apply(rls, ctx, F.mul_adj_, x, n), z), tag
        xd = rls.DeviceVector.from_host(x, ctx)
        assert _bits(F.mul_adj_(xd, xd).to_host(), z)
        ctx.tune(fft_fused=2)
    return F


@pytest.mark.parametrize("dtype", CPLX)
def test_fft_lines_every_length_and_flag(rls, fused, parity, dtype):
    dt = np.dtype(dtype)
    rng = np.random.default_rng(11)
    for n in (2, 4, 8, 32, 64, 128, 256, 2048, MAX_LINE[dt]):
        for shift, unitary in FLAGS:
            _fft_case(rls, fused, parity, dt, (n,), shift, unitary, rng)
    with pytest.raises((rls.RLSError, ValueError)):
        rls.FFTOp(dt, (2 * MAX_LINE[dt],), ctx=fused)
    with pytest.raises((rls.RLSError, ValueError)):
        rls.FFTOp(dt, (2 * MAX_LINE[dt], 2), ctx=fused)


@pytest.mark.parametrize("dtype", CPLX)
def test_fft_images_on_both_paths(rls, fused, parity, dtype):
    dt = np.dtype(dtype)
    rng = np.random.default_rng(12)
    for shape in ((2, 2), (4, 2), (8, 32), (32, 8), (1, 16), (64, 64)):
        for shift, unitary in FLAGS:
            _fft_case(rls, fused, parity, dt, shape, shift, unitary, rng, expect_variant=1)
    # the largest shapes one workgroup's LDS holds (159.5 KiB: 16384 ComplexF32, 8192 ComplexF64 points) and the first ones beyond
    last, beyond = (((128, 128),), ((256, 128), (128, 256))) if dt == np.complex64 else (((64, 128), (128, 64)), ((128, 128),))
    for shape in last:
        _fft_case(rls, fused, parity, dt, shape, True, True, rng, expect_variant=1)
    for shape in beyond + ((256, 256),):
        _fft_case(rls, fused, parity, dt, shape, True, True, rng, expect_variant=0)


def test_default_choice_of_path(rls, ctx):
    """fft_fused = 1, the default: the single-workgroup launch up to 1024 points (FFT_FUSED_AUTO_N, chosen from profiles/matfree.txt),
    the general path beyond; 2: whatever fits one workgroup's LDS; 0: never"""
    for shape, want in (((16, 16), (1, 1, 0)), ((32, 32), (1, 1, 0)), ((1024,), (1, 1, 0)), ((64, 32), (0, 1, 0)), ((128, 128), (0, 1, 0)),
                        ((256, 128), (0, 0, 0))):
        F = rls.FFTOp(np.complex64, shape, ctx=ctx)
        got = []
        for level in (1, 2, 0):
            ctx.tune(fft_fused=level)
            got.append(F.variant())
        ctx.tune(fft_fused=1)
        assert tuple(got) == want, (shape, got)


def _dot_test(rls, ctx, parity, A, dt, rng, tag):
    """<A x, y> = <x, A^H y>, the difference on the scale ||x|| ||y||"""
    x, y = _vec(rng, A.N, dt), _vec(rng, A.M, dt)
    Ax = _apply(rls, ctx, A.mul_, x, A.M).astype(np.complex128)
    AHy = _apply(rls, ctx, A.mul_adj_, y, A.N).astype(np.complex128)
    lhs, rhs = np.vdot(y, Ax), np.vdot(AHy, x.astype(np.complex128))
    parity(tag + " dot test", np.array([lhs]), np.array([rhs]), tol=TOL[dt], scale=np.linalg.norm(x) * np.linalg.norm(y))


@pytest.mark.parametrize("dtype", CPLX)
@pytest.mark.parametrize("shape", [(64,), (16, 16), (32, 8), (256, 128)])
def test_structure_inverse_dot_test_and_fused_normal(rls, fused, parity, dtype, shape):
    ctx, dt = fused, np.dtype(dtype)
    rng = np.random.default_rng(13)
    n = int(np.prod(shape))
    pat = MR.pattern(n, n // 3, 2)
    S, F = rls.SamplingOp(dt, pat, shape, ctx), rls.FFTOp(dt, shape, ctx=ctx)
    P = rls.ProdOp(S, F)
    assert isinstance(P, rls.SampledFFTOp) and (P.M, P.N) == (pat.size, n)
    x = _vec(rng, n, dt)
    normal = {}
    for path in ((2, 0) if F.variant() == 1 else (0,)):
        ctx.tune(fft_fused=path)
        assert F.variant() == (1 if path else 0)
        tag = f"{dt} {shape} fused={path}"
        parity(tag + " F^H F x = x", _apply(rls, ctx, F.mul_normal_, x, n), x.astype(np.complex128), tol=TOL[dt])
        for A, name in ((S, "SamplingOp"), (F, "FFTOp"), (P, "ProdOp")):
            _dot_test(rls, ctx, parity, A, dt, rng, f"{name} {tag}")
        parity(tag + " S F x", _apply(rls, ctx, P.mul_, x, P.M), MR.sampled_fft(x, pat, shape), tol=TOL[dt])
        y = _vec(rng, P.M, dt)
        parity(tag + " (S F)^H y", _apply(rls, ctx, P.mul_adj_, y, n), MR.sampled_fft_adj(y, pat, shape), tol=TOL[dt])
        # the fused normal apply against adjoint(mask(forward)) as three calls: bit for bit
        v = _apply(rls, ctx, P.mul_normal_, x, n)
        t = F.mul_(rls.DeviceVector(n, dt, ctx), rls.DeviceVector.from_host(x, ctx))
        S.mul_normal_(t, t)
        three = F.mul_adj_(rls.DeviceVector(n, dt, ctx), t).to_host()
        assert _bits(v, three), tag
        assert _bits(_apply(rls, ctx, P.normal_operator().mul_, x, n), v)
        parity(tag + " normal", v, MR.fft_adj(MR.sampling_mask(pat, n) * MR.fft(x, shape), shape), tol=TOL[dt])
        normal[path] = v
    assert len(normal) == 1 or _bits(normal[0], normal[2])   # the two paths: the same bits


# ---- solvers -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cs_problem():
    """the reference suite's L1 case in two dimensions: a 16 x 16 image with three planted spikes, half of the unitary DFT's rows.
    Built once, shared, never modified."""
    shape, n = (16, 16), 256
    pat = MR.pattern(n, n // 2, 21)
    x = np.zeros(n, np.complex128)
    x[[37, 120, 201]] = [1.0, -0.7 + 0.4j, 0.5j]
    D = MR.sampled_fft_dense(pat, shape)
    return shape, pat, D, D @ x


@pytest.mark.parametrize("dtype", CPLX)
@pytest.mark.parametrize("rho", [0.95, None])
def test_fista_l1_on_the_sampled_fft(rls, fused, parity, cs_problem, dtype, rho):
    ctx, dt = fused, np.dtype(dtype)
    shape, pat, D, b = cs_problem
    A = rls.ProdOp(rls.SamplingOp(dt, pat, shape, ctx), rls.FFTOp(dt, shape, ctx=ctx))
    kw = dict(iterations=30, relTol=0.0)
    S = rls.createLinearSolver(rls.FISTA, A, reg=rls.L1Regularization(0.01), rho=rho, **kw)
    if rho is None:   # 0.95 / power_iterations: the largest eigenvalue of F^H diag(mask) F is 1, the estimate's stopping rule 1e-3
        assert abs(S.state.rho - 0.95) <= 2e-3 * 0.95, S.state.rho
    x = rls.solve_(S, rls.DeviceVector.from_host(b.astype(dt), ctx)).to_host()
    assert S.state.iteration == 30 and not S.state._plan
    ref = O.FISTA(D, reg=O.L1Regularization(0.01), rho=S.state.rho, **kw)
    O.solve(ref, b)
    parity(f"FISTA+L1 on ProdOp(S, F) {dt} rho={rho}", x, ref.x,
           lambda: O.solve(O.FISTA(D.astype(np.complex64), reg=O.L1Regularization(0.01), rho=S.state.rho, **kw), b.astype(np.complex64)),
           tol=TOL[dt])


def test_fista_tv_positive_on_a_float32_sampling_op(rls, ctx, parity):
    shape, n = (16, 16), 256
    pat = MR.pattern(n, n // 3, 22)
    rng = np.random.default_rng(23)
    img = np.zeros(shape)
    img[4:11, 3:9] = 1.0
    img[9:14, 10:15] = 0.5
    xt = img.ravel(order="F")
    D = MR.sampling_dense(pat, n)
    b = D @ xt + 0.01 * rng.standard_normal(pat.size)
    A = rls.SamplingOp(np.float32, pat, shape, ctx)
    kw = dict(iterations=20, rho=0.95, relTol=0.0)
    S = rls.createLinearSolver(rls.FISTA, A, reg=[rls.TVRegularization(0.01, shape=shape), rls.PositiveRegularization()], **kw)
    x = rls.solve_(S, rls.DeviceVector.from_host(b.astype(np.float32), ctx)).to_host()
    assert S.state.iteration == 20 and not S.state._plan
    mk = lambda: [O.TVRegularization(0.01, shape=shape), O.PositiveRegularization()]
    ref = O.FISTA(D, reg=mk(), **kw)
    O.solve(ref, b)
    parity("FISTA+TV+Positive on SamplingOp Float32", x, ref.x,
           lambda: O.solve(O.FISTA(D.astype(np.float32), reg=mk(), **kw), b.astype(np.float32)))


@pytest.mark.parametrize("which", ["sampling", "fft", "product"])
def test_cgnr_l2(rls, fused, parity, cs_problem, which):
    ctx, dt = fused, np.dtype(np.complex64)
    shape, pat, D, b = cs_problem
    S_, F_ = rls.SamplingOp(dt, pat, shape, ctx), rls.FFTOp(dt, shape, ctx=ctx)
    if which == "sampling":
        A, D = S_, MR.sampling_dense(pat, 256, np.complex128)
    elif which == "fft":
        A, D = F_, MR.fft_dense(shape)
        b = D @ np.concatenate([b, b])
    else:
        A = rls.ProdOp(S_, F_)
    kw = dict(iterations=3, relTol=0.0)
    S = rls.createLinearSolver(rls.CGNR, A, reg=rls.L2Regularization(0.05), **kw)
    x = rls.solve_(S, rls.DeviceVector.from_host(b.astype(dt), ctx)).to_host()
    assert not S.state._plan
    ref = O.CGNR(D, reg=O.L2Regularization(0.05), **kw)
    O.solve(ref, b)
    assert S.state.iteration == ref.iteration
    parity(f"CGNR+L2 on {which}", x, ref.x,
           lambda: O.solve(O.CGNR(D.astype(dt), reg=O.L2Regularization(0.05), **kw), b.astype(dt)))
    S2 = rls.createLinearSolver(rls.CGNR, A, AHA=A.normal_operator(), reg=rls.L2Regularization(0.05), **kw)
    assert _bits(rls.solve_(S2, rls.DeviceVector.from_host(b.astype(dt), ctx)).to_host(), x)


def test_callbacks_and_matrix_right_hand_sides(rls, fused, cs_problem):
    ctx, dt = fused, np.dtype(np.complex64)
    shape, pat, D, b = cs_problem
    A = rls.ProdOp(rls.SamplingOp(dt, pat, shape, ctx), rls.FFTOp(dt, shape, ctx=ctx))
    bd = rls.DeviceVector.from_host(b.astype(dt), ctx)
    for T, kw in ((rls.CGNR, dict(relTol=0.0)), (rls.FISTA, dict(rho=0.95, relTol=0.0, reg=rls.L1Regularization(0.01)))):
        S = rls.createLinearSolver(T, A, iterations=5, **kw)
        seen, store = [], rls.StoreSolutionCallback()
        x = rls.solve_(S, bd, callbacks=[lambda s, it: seen.append(it), store]).to_host()
        assert seen == list(range(6)), (T.__name__, seen)   # iterations + 1 calls
        assert _bits(store.solutions[-1], x)
        assert _bits(rls.solve_(rls.createLinearSolver(T, A, iterations=5, **kw), bd).to_host(), x)
        B = np.asfortranarray(np.stack([b, 0.5j * b[::-1]], axis=1).astype(dt))
        cols = [rls.solve_(rls.createLinearSolver(T, A, iterations=5, **kw),
                           rls.DeviceVector.from_host(np.ascontiguousarray(B[:, j]), ctx)).to_host() for j in range(2)]
        for sched in (rls.SequentialState, rls.MultiThreadingState, rls.BatchedState):
            S = rls.createLinearSolver(T, A, iterations=5, **kw)
            xs = rls.solve_(S, rls.DeviceMatrix.from_host(B, ctx), scheduler=sched)
            assert not isinstance(S.state, rls.BatchedState)
            for j in range(2):
                assert _bits(xs[j].to_host(), cols[j]), (T.__name__, sched.__name__, j)


def test_reference_example_at_its_own_size(rls, ctx):
    """docs/src/literate/examples/compressed_sensing.jl: 256 x 256 Float32, a third of the pixels, FISTA + TV, 20 iterations.  No oracle
    at this size: it finishes and lowers ||A x - b|| below ||b||."""
    shape, n = (256, 256), 65536
    rng = np.random.default_rng(31)
    yy, xx = np.mgrid[-1:1:256j, -1:1:256j]
    img = ((xx ** 2 + (yy / 1.3) ** 2 < 0.6).astype(np.float32) + 0.5 * ((xx - 0.2) ** 2 + (yy + 0.1) ** 2 < 0.05)).astype(np.float32)
    pat = np.sort(rng.choice(n, n // 3, replace=False)).astype(np.int32)
    A = rls.SamplingOp(np.float32, pat, shape, ctx)
    b = img.ravel(order="F")[pat]
    bd = rls.DeviceVector.from_host(b, ctx)
    S = rls.createLinearSolver(rls.FISTA, A, reg=rls.TVRegularization(0.01, shape=shape), iterations=20)
    x = rls.solve_(S, bd)
    assert S.state.iteration == 20
    r = A.mul_(rls.DeviceVector(pat.size, np.float32, ctx), x).to_host() - b
    assert np.all(np.isfinite(x.to_host())) and np.linalg.norm(r) < np.linalg.norm(b), (np.linalg.norm(r), np.linalg.norm(b))
