"""GPU tests of NFFTOp (csrc/nfft.hip) and of CGNR and FISTA on it, both element types throughout.  The
device is held element by element to tests/nfft_ref.py (checked on the CPU by tests/test_nfft_ref.py): to the restatement in
complex128 within the derived rounding gate, and to the dense non-uniform DFT within the published truncation bound plus that gate.
"Bit for bit" compares the bytes.

m = 4 (and 8) on N = 1 and N = 2 has n = 2 or 4 < 2 m: the footprint wraps onto itself.  The operator is CORRECT there, not refused --
a grid point is visited by several taps of one node, which is the periodic window -- and the cases below hold it to the same gates.
No kernel of nfft.hip has a grid-stride loop (every launch covers its items exactly), so no case needs a second trip."""
import ctypes as C
import functools

import numpy as np
import pytest

import nfft_ref as NR
import rls_oracle as O

pytestmark = pytest.mark.gpu

CASES = [(s_, m_, d_) for d_ in NR.DT for s_ in NR.SHAPES for m_ in NR.ms_of(d_)]
IDS = [f"{np.dtype(d_).name}-" + "x".join(map(str, s_)) + f"-m{m_}" for s_, m_, d_ in CASES]


@functools.lru_cache(maxsize=None)
def _sets(shape, m):
    """per node set of one (shape, m): the nodes, the restatement in complex128 and the exact matrix.  Built once, shared by the element
    types, never modified"""
    out = []
    for name, nodes in NR.node_sets(shape, m):
        nodes.setflags(write=False)
        E = NR.exact(nodes, shape)
        E.setflags(write=False)
        out.append((name, nodes, NR.restated(nodes, shape, m), E))
    return out


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _apply(rls, ctx, fn, x, n_out):
    """fn(out, in) on device vectors, out filled with NaN (none may survive), twice: the same bits, and the input unwritten"""
    xd = rls.DeviceVector.from_host(x, ctx)
    y1 = fn(rls.DeviceVector(n_out, x.dtype, ctx).fill_(np.nan), xd).to_host()
    y2 = fn(rls.DeviceVector(n_out, x.dtype, ctx).fill_(np.nan), xd).to_host()
    assert not np.any(np.isnan(y1.real) | np.isnan(y1.imag))
    assert _bits(y1, y2) and _bits(xd.to_host(), x)
    return y1


@pytest.mark.parametrize("shape,m,dtype", CASES, ids=IDS)
def test_operator(rls, ctx, shape, m, dtype):
    dt = np.dtype(dtype)
    d, N = len(NR.extents(shape)), int(np.prod(shape))
    f, trunc = NR.ref_factor(dt), NR.truncation(m, d)
    for name, nodes, P, E in _sets(shape, m):
        tag = f"NFFTOp {dt} {shape} m={m} {name}"
        J = nodes.shape[1]
        A = rls.NFFTOp(dt, nodes if d == 2 else nodes[0], shape, m=m, ctx=ctx)
        n = [NR.grid_extent(N_) for N_ in NR.extents(shape)]
        assert (A.M, A.N, A.size(1), A.size(2), A.shape, A.m, A.image_shape, A.grid_points) == (J, N, J, N, (J, N), m, tuple(shape), int(np.prod(n)))
        x, y = NR.gauss(N, 21).astype(dt), NR.gauss(J, 22).astype(dt)
        # forward and adjoint: against the restatement within the rounding gate, against the definition within truncation + gate
        Ax = _apply(rls, ctx, A.mul_, x, J)
        want, bf = NR.forward_bound(dt, P, x)
        NR.check(tag + " forward", Ax, want, f * bf)
        NR.check(tag + " forward / exact", Ax, E @ x.astype(np.complex128), trunc * np.abs(x).sum() + f * bf)
        AHy = _apply(rls, ctx, A.mul_adj_, y, N)
        want, ba = NR.adjoint_bound(dt, P, y)
        NR.check(tag + " adjoint", AHy, want, f * ba)
        NR.check(tag + " adjoint / exact", AHy, E.conj().T @ y.astype(np.complex128), trunc * np.abs(y).sum() + f * ba)
        # <A x, y> = <x, A^H y> within what the two gates allow
        lhs, rhs = np.vdot(y.astype(np.complex128), Ax.astype(np.complex128)), np.vdot(AHy.astype(np.complex128), x.astype(np.complex128))
        assert abs(lhs - rhs) <= 2 * (np.abs(y) @ bf + np.abs(x) @ ba), (tag, abs(lhs - rhs))
        # the matrix by both routes: A applied to the unit vectors of length N, A^H to those of length J
        Fd = A.to_dense()
        assert (Fd.M, Fd.N) == (J, N)
        Fd = Fd.to_host()
        Ad = np.stack([_apply(rls, ctx, A.mul_adj_, e, N) for e in np.eye(J, dtype=dt)], axis=1)
        wantF, bF = NR.forward_bound(dt, P, np.eye(N))
        wantA, bA = NR.adjoint_bound(dt, P, np.eye(J))
        NR.check(tag + " dense", Fd, wantF, f * bF)
        NR.check(tag + " dense / exact", Fd, E, trunc + f * bF)
        NR.check(tag + " dense adjoint", Ad, wantA, f * bA)
        # (the restatement's own two routes differ by its complex128 roundings: their gates join the device's)
        own = NR.forward_bound(np.complex128, P, np.eye(N))[1].T + NR.adjoint_bound(np.complex128, P, np.eye(J))[1]
        NR.check(tag + " adjoint route = conjugate transpose", Ad, Fd.conj().T, bA + bF.T + own)
        # the normal product: one call, two calls, the lazy operator and in place are the same bits
        v = _apply(rls, ctx, A.mul_normal_, x, N)
        t = A.mul_(rls.DeviceVector(J, dt, ctx), rls.DeviceVector.from_host(x, ctx))
        assert _bits(A.mul_adj_(rls.DeviceVector(N, dt, ctx), t).to_host(), v), tag
        assert _bits(_apply(rls, ctx, A.normal_operator().mul_, x, N), v), tag
        xd = rls.DeviceVector.from_host(x, ctx)
        assert _bits(A.mul_normal_(xd, xd).to_host(), v), tag
    # mismatches, as RadonOp's
    with pytest.raises(ValueError):
        A.mul_(rls.DeviceVector(J + 1, dt, ctx), rls.DeviceVector(N, dt, ctx))
    with pytest.raises(ValueError):
        A.mul_adj_(rls.DeviceVector(N, dt, ctx), rls.DeviceVector(J + 2, dt, ctx))
    with pytest.raises(ValueError):
        A.mul_normal_(rls.DeviceVector(N + 1, dt, ctx), rls.DeviceVector(N, dt, ctx))
    other = np.complex64 if dt != np.complex64 else np.complex128
    with pytest.raises(TypeError):
        A.mul_(rls.DeviceVector(J, other, ctx), rls.DeviceVector(N, dt, ctx))
    with pytest.raises(TypeError):
        A.mul_(rls.DeviceVector(J, dt, ctx), rls.DeviceVector(N, np.float32, ctx))


@pytest.mark.parametrize("dtype", NR.DT, ids=NR.DT_IDS)
def test_transpose_is_unsupported_and_writes_nothing(rls, ctx, dtype):
    dt = np.dtype(dtype)
    nodes = NR.node_sets((8, 6), 2)[5][1]
    A = rls.NFFTOp(dt, nodes, (8, 6), m=2, ctx=ctx)
    y = rls.DeviceVector.from_host(NR.gauss(A.M, 3).astype(dt), ctx)
    x = rls.DeviceVector(A.N, dt, ctx).fill_(np.nan)
    before = y.to_host()
    assert ctx.lib.rls_nfft_mul(A._h, 1, y.ptr, x.ptr) == -2   # RLS_OP_T: RLS_E_UNSUPPORTED
    with pytest.raises(rls.RLSError):
        A.mul_transpose_(x, y)
    out = x.to_host()
    assert np.all(np.isnan(out.real)) and _bits(y.to_host(), before)
    assert ctx.lib.rls_nfft_mul(A._h, 7, y.ptr, x.ptr) == -1 and ctx.lib.rls_nfft_mul(A._h, 0, y.ptr, y.ptr) == -1
    n = C.c_int64()
    assert ctx.lib.rls_nfft_info(A._h, C.byref(n), None, None) == 0 and n.value == A.M


def test_create_refusals_of_the_library(rls, ctx):
    """what the Python class screens ahead of the context, asked of rls_nfft_create itself: nothing is created"""
    lib, h = ctx.lib, C.c_void_p()
    ok = np.zeros(4, np.float64)

    def create(code, shape, J, nodes, m):
        cs = (C.c_int64 * len(shape))(*shape)
        return lib.rls_nfft_create(ctx.handle, code, len(shape), cs, J, nodes.ctypes.data, m, C.byref(h))

    for code in (0, 2, 7):   # Float32, Float64, no type at all
        assert create(code, (8,), 4, ok, 4) == -1 and not h.value
    for J in (0, -1, 2 ** 31):
        assert create(1, (8,), J, ok, 4) == -1 and not h.value
    for bad in (0.5, -0.51, np.nan, np.inf):
        nodes = ok.copy()
        nodes[3] = bad
        assert create(1, (8,), 4, nodes, 4) == -1 and not h.value
        assert create(1, (4, 4), 2, nodes, 4) == -1 and not h.value
    assert create(1, (0,), 4, ok, 4) == -1 and not h.value
    for m in (0, 9, -2):
        assert create(1, (8,), 4, ok, m) == -2 and not h.value
    assert create(1, (4, 4, 4), 1, ok, 4) == -2 and create(1, (4097,), 4, ok, 4) == -2 and create(3, (8, 2049), 2, ok, 4) == -2 and not h.value
    assert create(1, (1, 1, 1), 4, ok, 8) == 0 and h.value   # every extent dropped: a signal of one point
    assert lib.rls_nfft_destroy(h) == 0


# ---- solvers -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mri_problem():
    """8 x 6, J = 70 nodes, m = 4: the restatement's dense matrix in complex128 (the window error is in it, so it cancels and only the
    device arithmetic is judged), a sparse image and its samples.  Built once, shared, never modified.

    The nodes are a 10 x 7 lattice over [-0.5, 0.5)^2, each moved by up to 0.02: the matrix has condition number 1.8, CGNR contracts by
    0.28 per iteration and 20 iterations CONVERGE, so x_20 is a property of the operator.  At 70 uniformly random nodes (condition
    number 22, contraction 0.913: x_20 is an iterate on the way) the comparison measures how a Float32 Krylov recurrence amplifies its
    own rounding instead: the Float32 ORACLE on the dense matrix is itself 5.8e-6 from the Float64 one there, and the device, whose
    product carries the roundings of a transform and a 64-term sum on top of a dense product's, was 1.9e-5."""
    shape = (8, 6)
    g1, g2 = np.meshgrid((np.arange(10) + 0.5) / 10 - 0.5, (np.arange(7) + 0.5) / 7 - 0.5, indexing="ij")
    nodes = np.stack([g1.ravel(), g2.ravel()]) + np.random.default_rng(5).uniform(-0.02, 0.02, (2, 70))
    D = NR.restated(nodes, shape, 4).dense()
    xt = np.zeros(48, np.complex128)
    xt[[3, 11, 20, 29, 41]] = [1.0, -0.5 + 0.5j, 2.0j, 0.75, -1.0 - 1.0j]
    for a in (nodes, D, xt):
        a.setflags(write=False)
    return shape, nodes, D, D @ xt


@pytest.mark.parametrize("dtype", NR.DT, ids=NR.DT_IDS)
def test_cgnr_l2(rls, ctx, parity, mri_problem, dtype):
    dt = np.dtype(dtype)
    shape, nodes, D, b = mri_problem
    A = rls.NFFTOp(dt, nodes, shape, ctx=ctx)
    bd = rls.DeviceVector.from_host(b.astype(dt), ctx)
    kw = dict(iterations=20, relTol=0.0)
    S = rls.createLinearSolver(rls.CGNR, A, reg=rls.L2Regularization(1e-2), **kw)
    seen = []
    x = rls.solve_(S, bd, callbacks=[lambda s, it: seen.append(it)]).to_host()
    assert seen == list(range(21)) and S.state.iteration == 20 and not S.state._plan
    ref = O.CGNR(D, reg=O.L2Regularization(1e-2), **kw)
    O.solve(ref, b)
    parity(f"CGNR+L2 on NFFTOp {dt}", x, ref.x,
           (lambda: O.solve(O.CGNR(D.astype(np.complex64), reg=O.L2Regularization(1e-2), **kw), b.astype(np.complex64))) if dt == NR.C64 else None)
    S2 = rls.createLinearSolver(rls.CGNR, A, AHA=A.normal_operator(), reg=rls.L2Regularization(1e-2), **kw)
    assert _bits(rls.solve_(S2, bd).to_host(), x) and not S2.state._plan


@pytest.mark.parametrize("dtype", NR.DT, ids=NR.DT_IDS)
def test_fista_l1(rls, ctx, parity, mri_problem, dtype):
    dt = np.dtype(dtype)
    shape, nodes, D, b = mri_problem
    A = rls.NFFTOp(dt, nodes, shape, ctx=ctx)
    bd = rls.DeviceVector.from_host(b.astype(dt), ctx)
    kw = dict(iterations=20, rho=0.95 / np.linalg.norm(D, 2) ** 2, relTol=0.0)
    S = rls.createLinearSolver(rls.FISTA, A, reg=rls.L1Regularization(0.05), **kw)
    seen = []
    x = rls.solve_(S, bd, callbacks=[lambda s, it: seen.append(it)]).to_host()
    assert seen == list(range(21)) and S.state.iteration == 20 and not S.state._plan
    ref = O.FISTA(D, reg=O.L1Regularization(0.05), **kw)
    O.solve(ref, b)
    parity(f"FISTA+L1 on NFFTOp {dt}", x, ref.x,
           (lambda: O.solve(O.FISTA(D.astype(np.complex64), reg=O.L1Regularization(0.05), **kw), b.astype(np.complex64))) if dt == NR.C64 else None)
