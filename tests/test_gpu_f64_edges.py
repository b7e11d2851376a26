"""The double-precision primitives of csrc/f64.hip at their tile, stride and geometry edges: rls_gemv_d at the 64-row and
4-column-split edges, the reductions on either side of every launch geometry, the elementwise kernels up to the first size that
takes a second grid-stride pass, L21 with degenerate groups, the TV prox with extents 1 and 2, Kaczmarz with N on either side of
its 1024-thread stride, and transpose / row norms / row scaling at the 32 x 32 tile edges.

References as in test_gpu_f64_plan_products.py: longdouble, and per entry the forward bound c (n_terms + 4) 2^-53 sum |a||x| of
any summation order (gamma() there; complex: n_terms = 2n, c = sqrt 2).  Where the kernel does one rounding per element and NumPy
the same operation, the comparison is exact.  A complex product is not such a case: the kernel's a.x b.x - a.y b.y may be
contracted into one fused multiply-add, so it gets the bound of a complex multiplication, sqrt 2 gamma_2 (Higham, Accuracy and
Stability of Numerical Algorithms, 2nd ed., (3.13)); sums of two such products get it twice.  Leading dimensions are padded with
NaN in the padding, outputs are longer than needed and the excess must come back bit-identical."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rls_oracle as O  # noqa: E402  (the checker)
from test_gpu_f64_plans import upload_padded  # noqa: E402
from test_gpu_f64_plan_products import GUARD, LD, SENTINEL, U, Guarded, _report, gamma, held, is_cplx, vector  # noqa: E402,F401
from test_gpu_kaczmarz_solve import L2LAM, problem as kz_problem, regs as kz_regs, run_oracle  # noqa: E402

pytestmark = pytest.mark.gpu
DT = [np.float64, np.complex128]
DT_IDS = ["float64", "complex128"]
OP_N, OP_T, OP_C = 0, 1, 2
CMUL = 2.0 * math.sqrt(2.0) * U   # sqrt 2 gamma_2: one complex multiplication


def code_of(rls, ctx, dt):
    return rls.DeviceVector(1, dt, ctx).code


def scalars(dt):
    return (0.7 - 0.2j, -0.3 + 0.5j) if is_cplx(dt) else (0.7 + 0j, -0.3 + 0j)


def up_full(rls, ctx, full, M):
    """a column-major host array with its padding rows, as a DeviceMatrix of M rows and lda = full.shape[0]"""
    Ad = rls.DeviceMatrix(M, full.shape[1], full.dtype, ctx, lda=full.shape[0])
    assert ctx.lib.rls_memcpy_h2d(ctx.handle, Ad.ptr, full.ctypes.data, full.nbytes) == 0
    return Ad


def down_full(ctx, Ad):
    out = np.empty((Ad.lda, Ad.N), dtype=Ad.dtype, order="F")
    assert ctx.lib.rls_memcpy_d2h(ctx.handle, out.ctypes.data, Ad.ptr, out.nbytes) == 0
    return out


def padded(dt, rows, cols, pad, fill):
    return np.full((rows + pad, cols), fill, dtype=dt, order="F")


# ---- rls_gemv_d ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("op", [OP_N, OP_T, OP_C], ids=["opN", "opT", "opC"])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 129], ids=lambda m: f"M{m}")
def test_gemv_at_the_row_tile_and_column_split_edges(rls, ctx, dt, op, M):
    """N = 1, 3 leave waves of d_gemv_n_kernel without a column (w N / 4 .. (w + 1) N / 4 is empty); 4, 5, 9 split evenly, with one
    and with a ragged remainder.  beta = 0 (the host then passes beta_zero = 1): y is not read, NaN in it does not reach the result."""
    L, code, lib, h = LD[np.dtype(dt)], code_of(rls, ctx, dt), ctx.lib, ctx.handle
    al, be = scalars(dt)
    for N in (1, 3, 4, 5, 9):
        A = vector(dt, M * N, 1000 * M + N).reshape((M, N), order="F")
        Ad = upload_padded(rls, ctx, A, 3)
        opA = A if op == OP_N else A.T if op == OP_T else A.conj().T
        nout, nin = opA.shape
        x, y0 = vector(dt, nin, 5), vector(dt, nout, 6)
        xd = Guarded(rls, ctx, dt, nin, body=x)
        prod = opA.astype(L) @ x.astype(L)
        sabs = np.abs(opA) @ np.abs(x)
        for beta, pre in ((be, y0), (0j, np.full(nout, np.nan, dtype=dt))):
            yd = Guarded(rls, ctx, dt, nout, body=pre)
            assert lib.rls_gemv_d(h, code, op, M, N, al.real, al.imag, Ad.ptr, Ad.lda, xd.ptr, beta.real, beta.imag, yd.ptr) == 0
            got = yd.read()
            ref = L(al if is_cplx(dt) else al.real) * prod
            bound = abs(al) * sabs
            if beta != 0:
                ref = ref + L(beta if is_cplx(dt) else beta.real) * y0.astype(L)
                bound = bound + abs(beta) * np.abs(y0)
            assert not np.isnan(got).any(), (M, N, beta)
            # sum: gamma; alpha s, beta y, the final add: (2 sqrt 2 + 1) u at the most on each part, inside the + 4
            held("rls_gemv_d", f"{np.dtype(dt).name} op={op} {M}x{N} beta={beta}", np.abs(got.astype(L) - ref), gamma(dt, nin) * bound)
        xd.read()


# ---- reductions -----------------------------------------------------------------------------------------------------------------------
RED_PER_WG = 8192                  # d_reduce_launch: nwg = ceil(n / 8192) workgroups of 1024 threads ...
RED_CAP = 4096 // 2 - 2            # ... at most RLS_RED_SLOTS / 2 - 2 = 2046 of them (two doubles per partial, two for the result)
RED_N = [(1, "n=1"), (RED_PER_WG - 1, "one-workgroup-below-edge"), (RED_PER_WG, "one-workgroup-finalises-directly"),
         (RED_PER_WG + 1, "two-stage-first-n"), (RED_CAP * RED_PER_WG - 1, "below-partials-cap"), (RED_CAP * RED_PER_WG, "at-partials-cap"),
         (RED_CAP * RED_PER_WG + 1, "above-partials-cap-second-pass")]
_big = {}


def ld_sums(x, y):
    """(sum |x|^2, sum |x|, conj(x).y, sum |x||y|) in longdouble, a million elements at a time"""
    L = LD[x.dtype]
    s2 = s1 = sxy = np.longdouble(0)
    dot = L(0)
    for i in range(0, x.size, 1 << 20):
        xl, yl = x[i: i + (1 << 20)].astype(L), y[i: i + (1 << 20)].astype(L)
        ax = np.abs(xl)
        s2, s1, dot, sxy = s2 + np.sum(ax * ax), s1 + np.sum(ax), dot + np.sum(np.conj(xl) * yl), sxy + np.sum(ax * np.abs(yl))
    return s2, s1, dot, sxy


def cancelling(x, y0):
    """y = y0 - c x with c such that conj(x).y is about 1e-10 of sum |x||y|"""
    target = 1e-10 * float(np.abs(x) @ np.abs(y0))
    return (y0 - ((np.vdot(x, y0) - target) / np.vdot(x, x)) * x).astype(x.dtype)


def big_vectors(rls, ctx, dt):
    """one pair of vectors for the three sizes around the cap, uploaded once; the sums of the first cap * 8192 - 1 elements once"""
    key = np.dtype(dt)
    if key not in _big:
        n = RED_CAP * RED_PER_WG + 1
        x, y = vector(dt, n, 41), vector(dt, n, 42)
        y[: n - 1] = cancelling(x[: n - 1], y[: n - 1])
        _big[key] = (x, y, rls.DeviceVector.from_host(x, ctx), rls.DeviceVector.from_host(y, ctx), ld_sums(x[: n - 2], y[: n - 2]))
    return _big[key]


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("n,name", RED_N, ids=[r[1] for r in RED_N])
def test_reductions_on_either_side_of_every_launch_geometry(rls, ctx, dt, n, name):
    """nrm2, asum, dotc: bounds on the sums of moduli, never on the result (dotc's inputs cancel to about 1e-10)"""
    L, code, lib, h = LD[np.dtype(dt)], code_of(rls, ctx, dt), ctx.lib, ctx.handle
    if n > 4 * RED_PER_WG:
        x, y, xd, yd, base = big_vectors(rls, ctx, dt)
        m = RED_CAP * RED_PER_WG - 1
        s2, s1, dot, sxy = (a + b for a, b in zip(base, ld_sums(x[m: n], y[m: n])))
        xp, yp = xd.ptr, yd.ptr
    else:
        x = vector(dt, n, 43)
        y = cancelling(x, vector(dt, n, 44)) if n > 1 else vector(dt, n, 44)
        xg, yg = Guarded(rls, ctx, dt, n, body=x), Guarded(rls, ctx, dt, n, body=y)
        s2, s1, dot, sxy = ld_sums(x, y)
        xp, yp = xg.ptr, yg.ptr
    case = f"{np.dtype(dt).name} n={n}"
    r = (C.c_double * 2)()
    # sum of n squares (complex: 2n), positive terms: relative (terms + 4) u; the square root halves it and adds one rounding
    assert lib.rls_nrm2_d(h, code, n, xp, r) == 0
    held("rls_nrm2_d", case, [abs(float(np.longdouble(r[0]) - np.sqrt(s2)))], [gamma(dt, n) / math.sqrt(2.0 if is_cplx(dt) else 1.0) * float(np.sqrt(s2))])
    assert r[1] == 0.0
    # sum of n moduli (complex: hypot, within an ulp each)
    assert lib.rls_asum_d(h, code, n, xp, r) == 0
    held("rls_asum_d", case, [abs(float(np.longdouble(r[0]) - s1))], [(n + 4) * U * float(s1)])
    assert lib.rls_dotc_d(h, code, n, xp, yp, r) == 0
    got = L(r[0]) + (1j * L(r[1]) if is_cplx(dt) else 0)
    if n > 1:
        assert abs(complex(dot)) < 1e-6 * float(sxy)   # (the inputs do cancel)
    held("rls_dotc_d", case, [abs(complex(got - dot))], [gamma(dt, n) * float(sxy)])
    if not is_cplx(dt):
        assert r[1] == 0.0
    again = (C.c_double * 2)()
    assert lib.rls_dotc_d(h, code, n, xp, yp, again) == 0 and bytes(again) == bytes(r)   # fixed order: the same bits


# ---- elementwise kernels ---------------------------------------------------------------------------------------------------------------
GRID_CAP = 2048 * 256   # dgrid: at most 2048 workgroups of 256 threads; element GRID_CAP is the first of a second pass
EW_N = [1, 255, 256, 257, GRID_CAP + 1]


def watch(n):
    """indices asserted one by one on top of the whole-array comparison: the last element, the two sides of the second pass"""
    return sorted({n - 1, min(n - 1, GRID_CAP - 1), min(n - 1, GRID_CAP)})


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("n", EW_N, ids=lambda n: f"n{n}")
def test_elementwise_kernels_up_to_a_second_grid_pass(rls, ctx, dt, n):
    code, lib, h, cplx = code_of(rls, ctx, dt), ctx.lib, ctx.handle, is_cplx(dt)
    a, b = scalars(dt)
    av, bv = (a, b) if cplx else (a.real, b.real)
    x, y = vector(dt, n, 51), vector(dt, n, 52)
    ax, ay = np.abs(x), np.abs(y)
    case = f"{np.dtype(dt).name} n={n}"

    def run(fn, *vecs):
        """fn(ptrs...) on fresh guarded copies; returns what the last vector holds afterwards"""
        g = [Guarded(rls, ctx, dt, n, body=v) for v in vecs]
        assert fn(*[q.ptr for q in g]) == 0
        out = [q.read() for q in g]
        for v, o in zip(vecs[:-1], out[:-1]):
            assert o.tobytes() == v.tobytes()   # inputs untouched
        return out[-1]

    def exact(name, got, want):
        for i in watch(n):
            assert got[i] == want[i], (name, case, i)
        assert np.array_equal(got, want), (name, case)

    def within(name, got, want, bound):
        for i in watch(n):
            assert abs(got[i] - want[i]) <= bound[i], (name, case, i)
        held(name, case, np.abs(got - want), bound)

    exact("fill", run(lambda p: lib.rls_fill_d(h, code, n, p, a.real, a.imag), x), np.full(n, av, dtype=dt))
    got = run(lambda p: lib.rls_scal_d(h, code, n, a.real, a.imag, p), x)
    within("rls_scal_d", got, av * x, CMUL * abs(a) * ax) if cplx else exact("scal", got, av * x)
    # a x + y, a x + b y: one or two products and one sum; real: one fused multiply-add at the least, two roundings at the most
    within("rls_axpy_d", run(lambda px, py: lib.rls_axpy_d(h, code, n, a.real, a.imag, px, py), x, y), av * x + y,
           (CMUL + 2 * U) * (abs(a) * ax + ay))
    z0 = vector(dt, n, 53)
    within("rls_lincomb_d", run(lambda px, py, pz: lib.rls_lincomb_d(h, code, n, a.real, a.imag, px, b.real, b.imag, py, pz), x, y, z0),
           av * x + bv * y, (CMUL + 2 * U) * (abs(a) * ax + abs(b) * ay))
    got = run(lambda px, pz: lib.rls_lincomb_d(h, code, n, a.real, a.imag, px, 0.0, 0.0, None, pz), x, z0)   # b = 0: y is not read
    within("rls_lincomb_d, no y", got, av * x, CMUL * abs(a) * ax) if cplx else exact("lincomb, no y", got, av * x)
    lam = 0.37
    f = 1.0 / (1.0 + 2.0 * lam)
    exact("prox_l2", run(lambda p: lib.rls_prox_l2_d(h, code, n, p, lam), x), (x.real * f + 1j * (x.imag * f)).astype(dt) if cplx else x * f)
    exact("positive", run(lambda p: lib.rls_prox_positive_d(h, code, n, p), x), np.maximum(x.real, 0.0).astype(dt))
    exact("real", run(lambda p: lib.rls_prox_real_d(h, code, n, p), x), x.real.astype(dt))
    # prox_l1 with its edge entries in front and at the very end: |x| = lambda exactly (0.625 = |0.375 + 0.5i|), exact zeros, and
    # complex entries with a zero real part above and below the threshold
    lam_c = 0.625
    edge = [lam_c, -lam_c, 0.0] + ([0.375 + 0.5j, 2.0j, -0.25j] if cplx else [])
    xs = x.copy()
    xs[: min(len(edge), n)] = edge[: min(len(edge), n)]
    if n > 1:
        xs[n - 1] = -lam_c
    got = run(lambda p: lib.rls_prox_l1_d(h, code, n, p, lam_c), xs)
    want = O.prox_l1(xs.copy(), lam_c)
    # hypot, a subtraction, a sum, a product and a quotient: each within an ulp of a quantity no larger than |x| + eps
    within("rls_prox_l1_d", got, want, 8.0 * U * (np.abs(xs) + U))
    zero = np.nonzero(xs == 0)[0]
    assert not got[zero].any() and not want[zero].any()
    if cplx:   # eps is on the real part alone: a zero real part comes out as sh eps / (|x| + eps) > 0, to a few ulps of that
        zr = np.nonzero((xs.real == 0) & (np.abs(xs.imag) > lam_c))[0]
        assert zr.size or n < 6
        assert np.all(got.real[zr] > 0) and np.allclose(got.real[zr], want.real[zr], rtol=1e-14, atol=0.0)


# ---- rls_prox_l21_d ----------------------------------------------------------------------------------------------------------------------
L21_CASES = [("slen=1-one-group", 8, 8, None), ("ragged-n-tail-joins-first-groups", 23, 4, None), ("two-workgroups-of-groups", 1031, 4, None),
             ("all-zero-group-lambda>0-stays-0", 12, 3, 0.37), ("all-zero-group-lambda=0-is-NaN", 12, 3, 0.0)]


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("name,n,slices,zero_lam", L21_CASES, ids=[c[0] for c in L21_CASES])
def test_prox_l21_with_degenerate_groups(rls, ctx, dt, name, n, slices, zero_lam):
    """(g - lambda) / g of an all-zero group is -Inf (clamped to 0) for lambda > 0 and NaN for lambda = 0, which max() propagates in
    the reference (ProxL21.jl:30-35) as in the kernel and in the oracle"""
    slen = n // slices
    x = vector(dt, n, 61)
    lam = 0.37 if zero_lam is None else zero_lam
    if zero_lam is not None:
        x[2::slen] = 0
    xd = Guarded(rls, ctx, dt, n, body=x)
    assert ctx.lib.rls_prox_l21_d(ctx.handle, code_of(rls, ctx, dt), n, slices, xd.ptr, lam) == 0
    got, want = xd.read(), O.prox_l21(x.copy(), lam, slices)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    if zero_lam is not None:
        grp = np.arange(n) % slen == 2
        assert np.array_equal(nan, grp) if zero_lam == 0.0 else (not nan.any() and not got[grp].any())
    # the group norm: a sum of <= slices + 1 squares, a root, a difference, a quotient, a product
    held("rls_prox_l21_d", f"{np.dtype(dt).name} {name}", np.abs(got[~nan] - want[~nan]), (n // slen + 10) * U * np.abs(x[~nan]))


# ---- rls_prox_tv_fgp_d --------------------------------------------------------------------------------------------------------------------
TV_SHAPES = [((1, 7), None), ((7, 1), None), ((2, 2), None), ((1,), None), ((2,), None), ((3, 1, 5), (1, 3)), ((3, 1, 5), None),
             ((2, 1, 3, 2), None), ((1, 4, 1, 3), (1, 2, 3))]


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("shape,dims", TV_SHAPES, ids=[f"shape{'x'.join(map(str, s))}-dims{d}" for s, d in TV_SHAPES])
def test_prox_tv_with_extents_one_and_two(rls, ctx, dt, shape, dims):
    """a TV dimension of extent 1 has no gradient rows: its block is empty, wherever it stands among the blocks, and nothing of
    d_tv_dual_kernel divides by that extent minus one; (1,) has no rows at all and the prox is the identity"""
    n = int(np.prod(shape))
    x = vector(dt, n, 71)
    want = O.prox_tv_fgp(x.copy(), 0.3, shape, dims, 10)
    xd = Guarded(rls, ctx, dt, n, body=x)
    rls.prox_(rls.TVRegularization, rls.DeviceVector.borrow(xd.ptr, n, dt, ctx, keep=xd), 0.3, shape=shape, dims=dims)
    got = xd.read()
    assert np.isfinite(got).all()
    err = float(np.linalg.norm(got - want) / np.linalg.norm(want))
    print(f"tv {np.dtype(dt).name} {shape} dims={dims}: {err:.3e}")
    assert err < 1e-12, err
    if shape == (1,):
        assert got.tobytes() == x.tobytes()


# ---- rls_kaczmarz_solve_d -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("maps", ["none", "posl1"], ids=["no-maps", "positive+l1-after-every-sweep"])
@pytest.mark.parametrize("N", [1, 1023, 1024, 1025, 2050], ids=lambda n: f"N{n}")
def test_kaczmarz_on_either_side_of_the_thread_stride(rls, ctx, dt, maps, N):
    """M = 12 with one zero row, 3 sweeps, 3 right-hand sides with ldx = N + 3: a thread owns no, one, two or three entries of x"""
    M, K, SW = 12, 3, 3
    A, b, lam1 = kz_problem(dt, M, N)
    B = np.stack([b, 2 * b - 1, b[::-1]], axis=1).astype(dt)
    denom, rowindex = O.init_kaczmarz(np.asarray(A), np.float64(L2LAM))
    assert len(rowindex) == M - 1
    at = padded(dt, N, M, 2, np.nan)
    at[:N, :] = np.asarray(A).T
    xs = padded(dt, N, K, 3, SENTINEL[np.dtype(dt)])
    xs[:N, :] = 0
    us = padded(dt, M, K, 1, np.nan)
    us[:M, :] = B
    vls = padded(dt, M, K, 1, SENTINEL[np.dtype(dt)])
    vls[:M, :] = 0
    Atd, Xd, Ud, Vd = up_full(rls, ctx, at, N), up_full(rls, ctx, xs, N), up_full(rls, ctx, us, M), up_full(rls, ctx, vls, M)
    rows = rls.DeviceVector.from_host(np.ascontiguousarray(rowindex, dtype=np.int32).view(np.float32), ctx)
    den = rls.DeviceVector.from_host(denom.astype(np.float64), ctx)
    pk, rk, lam = (2, 1, lam1) if maps == "posl1" else (0, 0, 0.0)   # RLS_PROJ_POSITIVE, RLS_REG_L1
    st = ctx.lib.rls_kaczmarz_solve_d(ctx.handle, code_of(rls, ctx, dt), M, N, Atd.ptr, Atd.lda, K, Xd.ptr, Xd.lda, Ud.ptr, Ud.lda, Vd.ptr,
                                      Vd.lda, rows.ptr, den.ptr, len(rowindex), 0, math.sqrt(L2LAM), SW, pk, rk, lam)
    assert st == 0, ctx.lib.rls_last_error_string(ctx.handle)
    X, V = down_full(ctx, Xd), down_full(ctx, Vd)
    assert X[N:, :].tobytes() == xs[N:, :].tobytes() and V[M:, :].tobytes() == vls[M:, :].tobytes()
    for j in range(K):
        xr, vl = run_oracle(np.asarray(A), B[:, j].copy(), kz_regs(O, maps, lam1), SW)
        ex = float(np.linalg.norm(X[:N, j] - xr[-1]) / max(np.linalg.norm(xr[-1]), 1e-300))
        ev = float(np.linalg.norm(V[:M, j] - vl) / np.linalg.norm(vl))
        print(f"kaczmarz {np.dtype(dt).name} N={N} {maps} rhs {j}: x {ex:.3e} vl {ev:.3e}")
        assert ex <= 1e-12 and ev <= 1e-12, (j, ex, ev)


# ---- rls_transpose_d, rls_rownorm2_d, rls_scale_rows_d ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("M", [1, 31, 32, 33, 65], ids=lambda m: f"M{m}")
def test_transpose_rownorms_and_row_scaling_at_the_tile_edges(rls, ctx, dt, M):
    code, lib, h, cplx = code_of(rls, ctx, dt), ctx.lib, ctx.handle, is_cplx(dt)
    for N in (1, 31, 32, 33, 65):
        case = f"{np.dtype(dt).name} {M}x{N}"
        A = vector(dt, M * N, 100 * M + N).reshape((M, N), order="F")
        Ad = upload_padded(rls, ctx, A, 3)
        t0 = padded(dt, N, M, 2, SENTINEL[np.dtype(dt)])
        Td = up_full(rls, ctx, t0, N)
        assert lib.rls_transpose_d(h, code, M, N, Ad.ptr, Ad.lda, Td.ptr, Td.lda) == 0
        T = down_full(ctx, Td)
        assert np.array_equal(T[:N, :], A.T) and T[N:, :].tobytes() == t0[N:, :].tobytes(), case
        out = Guarded(rls, ctx, np.float64, M)
        assert lib.rls_rownorm2_d(h, code, M, N, Ad.ptr, Ad.lda, out.ptr) == 0
        a2 = np.abs(A.astype(LD[np.dtype(dt)])) ** 2
        s = np.sum(a2, axis=1)
        held("rls_rownorm2_d", case, np.abs(out.read().astype(np.longdouble) - s), ((2 if cplx else 1) * N + 4) * U * s.astype(np.float64))
        w = vector(dt, M, 9)
        wd = Guarded(rls, ctx, dt, M, body=w)
        b0 = padded(dt, M, N, 1, SENTINEL[np.dtype(dt)])
        Bd = up_full(rls, ctx, b0, M)
        assert lib.rls_scale_rows_d(h, code, M, N, wd.ptr, Ad.ptr, Ad.lda, Bd.ptr, Bd.lda) == 0
        Bh = down_full(ctx, Bd)
        assert Bh[M:, :].tobytes() == b0[M:, :].tobytes(), case
        want = w[:, None] * A
        if cplx:
            held("rls_scale_rows_d", case, np.abs(Bh[:M, :] - want), CMUL * np.abs(want) + U * np.abs(want))
        else:
            assert np.array_equal(Bh[:M, :], want), case
        wd.read()
