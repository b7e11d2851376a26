"""The FFT and sampling kernels of csrc/fft.hip through the C ABI, at every bundle regime of the general path (fft_pass: base value,
floor of 3 along dimension 1, clamp to the other extent, shrink loop against the 64 KiB, exact fit, 64 / 512 / 1024 threads, 1 / 2 / 4
trips of a stage's thread loop, a second trip of the bundle loop), at both thread counts and at the LDS limit of the single-workgroup
kernel, with unit extents in every place, and at the edges of the sampling kernels' grid-stride loops.  tests/test_fft_ref.py proves
on the CPU that the shape table of tests/fft_ref.py reaches every one of those regimes.  NOT reached: a second trip of the bundle loop
along dimension 1 -- its smallest shape is 8192 x 8192, 512 MiB -- and extents that are no powers of two, which are refused.

References, shapes, inputs and gates are those of tests/fft_ref.py (derived in its docstring from the radix-2 error bound, never
measured; held to numpy.fft and to planted mistakes by tests/test_fft_ref.py).  Every output vector is prefilled with NaN between two
guards of sentinel elements that must come back bit-identical, every input must come back bit-identical, every launch is made twice
and must return the same bytes, in place must give the bytes of out of place, and where an image fits one workgroup the two paths
must give the same bytes -- the signs of the exact zeros that unit impulses and the constant vector produce included, which is how
this file found the general path signing its shifts in another place than the single-workgroup kernel (profiles/fft_edges.txt)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fft_ref as R  # noqa: E402
import matfree_ref as MR  # noqa: E402
from test_gpu_f64_plan_products import GUARD, Guarded, _report, note  # noqa: E402,F401
from test_gpu_vec_edges import code_of, guarded, same  # noqa: E402

pytestmark = pytest.mark.gpu
E_INVALID, E_UNSUPPORTED = -1, -2
OP_N, OP_T, OP_C = 0, 1, 2
FFT_SHIFT, FFT_UNITARY = 1, 2
DTYPES = (np.float32, np.complex64, np.float64, np.complex128)
NAN = {np.dtype(d): (np.dtype(d).type(complex(np.nan, np.nan)) if np.dtype(d).kind == "c" else np.dtype(d).type(np.nan)) for d in DTYPES}


@pytest.fixture()
def paths(ctx):
    """the context for a test that switches fft_fused; the default comes back afterwards"""
    yield ctx
    ctx.tune(fft_fused=1)


def nan_out(rls, ctx, dt, n):
    """n NaN elements between two guards"""
    return Guarded(rls, ctx, dt, n, body=NAN[np.dtype(dt)], lead=GUARD)


def fft_create(rls, ctx, dt, shape, shift, unitary, flags=None):
    """(status, handle) of rls_fft_create with ndims = len(shape)"""
    h = C.c_void_p()
    flags = ((FFT_SHIFT if shift else 0) | (FFT_UNITARY if unitary else 0)) if flags is None else flags
    st = ctx.lib.rls_fft_create(ctx.handle, code_of(rls, ctx, dt), len(shape), (C.c_int64 * max(len(shape), 1))(*shape), flags, C.byref(h))
    return st, h


def fft_op(rls, ctx, dt, shape, shift=True, unitary=True):
    st, h = fft_create(rls, ctx, dt, shape, shift, unitary)
    assert st == 0 and h.value, (shape, ctx.lib.rls_last_error_string(ctx.handle))
    return h


def samp_create(rls, ctx, dt, N, pat, m=None):
    pat = np.ascontiguousarray(pat, dtype=np.int32)
    h = C.c_void_p()
    st = ctx.lib.rls_sampling_create(ctx.handle, code_of(rls, ctx, dt), N, pat.size if m is None else m, pat.ctypes.data, C.byref(h))
    return st, h


def samp_op(rls, ctx, dt, N, pat):
    st, h = samp_create(rls, ctx, dt, N, pat)
    assert st == 0 and h.value, ctx.lib.rls_last_error_string(ctx.handle)
    return h


def variant(ctx, F):
    v = C.c_int32(-1)
    assert ctx.lib.rls_fft_variant(F, C.byref(v)) == 0
    return v.value


def twice(rls, ctx, dt, n_out, ins, call):
    """call(out pointer) twice on NaN-filled guarded outputs: the same bytes, the inputs `ins` [(guarded, host)] and the guards intact"""
    outs = []
    for _ in range(2):
        yg = nan_out(rls, ctx, dt, n_out)
        assert call(yg.ptr) == 0, ctx.lib.rls_last_error_string(ctx.handle)
        outs.append(yg.read().copy())
    assert outs[0].tobytes() == outs[1].tobytes(), "two launches differ"
    for g, a in ins:
        assert same(g, a), "an input was written"
    return outs[0]


def apply(rls, ctx, F, adjoint, x):
    """rls_fft_apply out of place (twice) and in place: the same bytes"""
    lib = ctx.lib
    xg = guarded(rls, ctx, x)
    y = twice(rls, ctx, x.dtype, x.size, [(xg, x)], lambda p: lib.rls_fft_apply(F, adjoint, xg.ptr, p))
    zg = guarded(rls, ctx, x)
    assert lib.rls_fft_apply(F, adjoint, zg.ptr, zg.ptr) == 0
    assert zg.read().tobytes() == y.tobytes(), "in place differs from out of place"
    return y


def shape_class(dt, shape):
    if len(shape) == 1:
        return "lines"
    return "general-path images" if shape in R.GENERAL[np.dtype(dt)] or shape == R.BIG else "single-workgroup images"


def check(group, case, triples):
    """fft_ref.judge's triples: every error within its bound; the largest ratio goes to the report"""
    worst = 0.0
    for label, e, b in triples:
        e, b = np.asarray(e, np.float64).ravel(), np.asarray(b, np.float64).ravel()
        bad = np.nonzero(~(e <= b))[0]
        assert bad.size == 0, f"{group} {case} {label}: {bad.size} entries beyond the bound, first {bad[0]}: {e[bad[0]]:.3e} > {b[bad[0]]:.3e}"
        if e.size:
            worst = max(worst, float(np.max(e / np.maximum(b, 1e-300))))
    note(group, worst, case)


def transform_case(rls, ctx, dt, shape, flags, kinds=None):
    """every input of the shape under `flags`, forward and adjoint: the general path against the gates, the single-workgroup path
    (where the image fits) against the general path's bytes; rls_fft_variant at all three levels"""
    dt = np.dtype(dt)
    lg1, lg2 = R.extents(shape)
    fits = R.fused_fits(dt, lg1, lg2)
    kw = {} if kinds is None else {"kinds": kinds}
    for shift, unitary in flags:
        F = fft_op(rls, ctx, dt, shape, shift, unitary)
        for adjoint in (0, 1):
            names, X = R.inputs(dt, shape, shift, unitary, bool(adjoint), **kw)
            want = R.reference(X, shape, shift, unitary, bool(adjoint), dt)
            ctx.tune(fft_fused=0)
            assert variant(ctx, F) == 0
            got = np.stack([apply(rls, ctx, F, adjoint, np.ascontiguousarray(X[:, c])) for c in range(len(names))], axis=1)
            assert not np.isnan(got).any()
            case = f"{shape} shift={shift} unitary={unitary} adjoint={adjoint}"
            check(f"fft {dt.name} {shape_class(dt, shape)}", case, R.judge(dt, shape, shift, unitary, names, X, got, want, R.ref_factor(dt, shape)))
            ctx.tune(fft_fused=2)
            assert variant(ctx, F) == (1 if fits else 0), case
            if fits:
                for c, name in enumerate(names):
                    y = apply(rls, ctx, F, adjoint, np.ascontiguousarray(X[:, c]))
                    assert y.tobytes() == got[:, c].tobytes(), f"{case} {name}: the two paths differ"
            ctx.tune(fft_fused=1)
            assert variant(ctx, F) == (1 if R.use_fused(dt, lg1, lg2, 1) else 0), case
        assert ctx.lib.rls_fft_destroy(F) == 0


# ---- transforms --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", R.DT, ids=R.DT_IDS)
@pytest.mark.parametrize("k", range(14), ids=lambda k: f"n{1 << k}")
def test_lines_of_every_length(rls, paths, dt, k):
    """1, 2, ... 8192 (ComplexF64: 4096): 1 returns from fft_lines at once on a table of one entry, up to 64 the workgroup has idle
    threads, 1024 is where lgb reaches 0, 4096 and 8192 take 2 and 4 trips of a stage's thread loop; the single-workgroup kernel
    switches from 256 to 1024 threads behind 2048"""
    shape = (1 << k,)
    if shape not in R.line_lengths(dt):
        assert shape == (8192,) and np.dtype(dt) == R.C128
        st, h = fft_create(rls, paths, dt, shape, True, True)   # the longest ComplexF64 line is 4096: refused
        assert st == E_UNSUPPORTED and not h.value
        return
    transform_case(rls, paths, dt, shape, R.flags_of(shape))


def _images():
    return [(dt, s) for dt in R.DT for s in R.GENERAL[np.dtype(dt)] + R.FUSED[np.dtype(dt)]]


@pytest.mark.parametrize("dt,shape", _images(), ids=lambda v: str(v).replace(" ", "") if isinstance(v, tuple) else np.dtype(v).name)
def test_images_in_every_bundle_regime_and_on_one_workgroup(rls, paths, dt, shape):
    """fft_ref.GENERAL: an extent of 2 beside the longest line both ways, the floor of 3 with an exact fit / a shrink to 2, shrinks to
    2, 1 and 0 (one strided element per line), the longest contiguous lines in several workgroups, lgb = 0 on dimension 0 inside
    an image.  fft_ref.FUSED: both thread counts, the most points the LDS admits with an extent of 2 either way, unit extents in every
    place and (4, 1, 8) through ndims = 3, which acts as (4, 8)."""
    transform_case(rls, paths, dt, shape, R.flags_of(shape))
    if shape == (4, 1, 8):   # the same bytes as (4, 8)
        x = R.gauss(dt, 32, 3)
        a, b = fft_op(rls, paths, dt, (4, 1, 8)), fft_op(rls, paths, dt, (4, 8))
        for level in (0, 2):
            paths.tune(fft_fused=level)
            for adjoint in (0, 1):
                assert apply(rls, paths, a, adjoint, x).tobytes() == apply(rls, paths, b, adjoint, x).tobytes()
        assert paths.lib.rls_fft_destroy(a) == 0 and paths.lib.rls_fft_destroy(b) == 0


def test_second_trip_of_the_bundle_loop(rls, paths):
    """1024 x 8192 ComplexF32 (64 MiB) under (True, True): 8192 bundles of one line on 4096 workgroups along dimension 0, the smallest
    shape at which `bundle += gridDim.x` runs.  One random input and one impulse (in the second half of the bundles), forward and
    adjoint.  Along dimension 1 the same needs 8192 x 8192 and is not tested."""
    p = R.pass_plan(np.complex64, 10, 13, False)
    assert (p.bundles, p.grid, p.bundle_trips) == (8192, 4096, 2)
    N = R.points(R.BIG)
    transform_case(rls, paths, np.complex64, R.BIG, [(True, True)], kinds=("random", ("impulse", N // 2 + 5 * 1024 + 3)))


# ---- the normal operator and the product ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", R.DT, ids=R.DT_IDS)
@pytest.mark.parametrize("shape", R.NORMAL_SHAPES, ids=lambda s: str(s).replace(" ", ""))
def test_normal_operator_and_product_with_structured_masks(rls, paths, dt, shape):
    """rls_fft_sampled_mul_normal on both paths with masks of all ones, of one sample (at 0, at N - 1, at an index whose bit reversal
    differs) and of a random third: within (2 gate + gate^2) N scale^2 ||x|| of the reference, bit for bit the three separate calls,
    the two paths bit for bit, in place allowed.  rls_fft_sampled_mul forward and adjoint with m = 1, m = N and the third."""
    ctx, lib, dt = paths, paths.lib, np.dtype(dt)
    lg1, lg2 = R.extents(shape)
    N = R.points(shape)
    fits = R.fused_fits(dt, lg1, lg2)
    x = R.gauss(dt, N, 40 + N)
    nx = float(np.linalg.norm(x.astype(np.complex128)))
    fac = R.ref_factor(dt, shape)
    for shift, unitary in R.flags_of(shape):
        F = fft_op(rls, ctx, dt, shape, shift, unitary)
        s2 = 1.0 if unitary else float(N)
        for name, pat in R.masks(shape):
            S = samp_op(rls, ctx, dt, N, pat)
            mask = MR.sampling_mask(pat, N)
            case = f"{shape} shift={shift} unitary={unitary} mask {name}"
            want = R.reference_normal(x, mask, shape, shift, unitary, dt)
            bound = R.gate_normal(dt, shape) * fac * s2 * nx
            got = {}
            for level in ((0, 2) if fits else (0,)):
                ctx.tune(fft_fused=level)
                assert variant(ctx, F) == (1 if level else 0)
                xg = guarded(rls, ctx, x)
                v = twice(rls, ctx, dt, N, [(xg, x)], lambda p: lib.rls_fft_sampled_mul_normal(F, S, xg.ptr, p))
                assert not np.isnan(v).any()
                zg = guarded(rls, ctx, x)
                assert lib.rls_fft_sampled_mul_normal(F, S, zg.ptr, zg.ptr) == 0
                assert zg.read().tobytes() == v.tobytes(), f"{case} fused={level}: in place differs"
                tg, wg = nan_out(rls, ctx, dt, N), nan_out(rls, ctx, dt, N)   # forward, mask, adjoint as three calls
                assert lib.rls_fft_apply(F, 0, xg.ptr, tg.ptr) == 0 and lib.rls_sampling_mul_normal(S, tg.ptr, tg.ptr) == 0
                assert lib.rls_fft_apply(F, 1, tg.ptr, wg.ptr) == 0
                assert wg.read().tobytes() == v.tobytes(), f"{case} fused={level}: the three calls differ"
                err = np.abs(v.astype(want.dtype) - want).astype(np.float64)
                check(f"normal operator {dt.name}", f"{case} fused={level}", [("norm", [float(np.linalg.norm(err))], [bound]), ("elements", err, np.full(N, bound))])
                if name == "ones":   # the identity, N x when not unitary
                    e1 = np.abs(v.astype(want.dtype) - s2 * x.astype(want.dtype)).astype(np.float64)
                    check(f"normal operator {dt.name}", f"{case} fused={level} = x", [("norm", [float(np.linalg.norm(e1))], [bound])])
                got[level] = v
            assert len(got) == 1 or got[0].tobytes() == got[2].tobytes(), f"{case}: the two paths differ"
            if name in ("ones", "third") or name == R.masks(shape)[-2][0]:   # the product: m = N, the third, m = 1
                m = pat.size
                fx = R.reference(x, shape, shift, unitary, False, dt)
                y = R.gauss(dt, m, 50 + m)
                fhy = R.reference(MR.sampling_adj(y, pat, N), shape, shift, unitary, True, dt)
                g = R.gate(dt, shape) * fac
                nfx, nfy = float(np.linalg.norm(fx.astype(np.complex128))), float(np.linalg.norm(fhy.astype(np.complex128)))
                for level in ((0, 2) if fits else (0,)):
                    ctx.tune(fft_fused=level)
                    xg, yg = guarded(rls, ctx, x), guarded(rls, ctx, y)
                    sf = twice(rls, ctx, dt, m, [(xg, x)], lambda p: lib.rls_fft_sampled_mul(F, S, OP_N, xg.ptr, p))
                    e = np.abs(sf.astype(fx.dtype) - fx[pat]).astype(np.float64)
                    check(f"product {dt.name}", f"{case} fused={level} S F x", [("elements", e, np.full(m, g * nfx))])
                    tg, og = nan_out(rls, ctx, dt, N), nan_out(rls, ctx, dt, m)
                    assert lib.rls_fft_apply(F, 0, xg.ptr, tg.ptr) == 0 and lib.rls_sampling_mul(S, OP_N, 1.0, 0.0, tg.ptr, 0.0, 0.0, og.ptr) == 0
                    assert og.read().tobytes() == sf.tobytes(), f"{case}: S F x differs from its two calls"
                    ah = twice(rls, ctx, dt, N, [(yg, y)], lambda p: lib.rls_fft_sampled_mul(F, S, OP_C, yg.ptr, p))
                    e = np.abs(ah.astype(fhy.dtype) - fhy).astype(np.float64)
                    check(f"product {dt.name}", f"{case} fused={level} (S F)^H y", [("norm", [float(np.linalg.norm(e))], [g * nfy]), ("elements", e, np.full(N, g * nfy))])
                    tg, og = nan_out(rls, ctx, dt, N), nan_out(rls, ctx, dt, N)
                    assert lib.rls_sampling_mul(S, OP_C, 1.0, 0.0, yg.ptr, 0.0, 0.0, tg.ptr) == 0 and lib.rls_fft_apply(F, 1, tg.ptr, og.ptr) == 0
                    assert og.read().tobytes() == ah.tobytes(), f"{case}: (S F)^H y differs from its two calls"
            assert lib.rls_sampling_destroy(S) == 0
        assert lib.rls_fft_destroy(F) == 0


# ---- sampling ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def sampling_cases():
    """(name, N, pattern): m = N in order and reversed, m = 1 at N - 1, and m and N on either side of one grid pass (524288 elements);
    the largest index of every pattern is N - 1"""
    n, span = 48, R.GRID_SPAN
    out = [("identity", n, np.arange(n)), ("reversed", n, np.arange(n)[::-1]), ("one@N-1", n, np.array([n - 1]))]
    for m, N in ((span, span), (span, span + 1), (span + 1, span + 1)):
        pat = np.random.default_rng(m + N).permutation(N)[:m]
        if N - 1 not in pat:
            pat[-1] = N - 1
        out.append((f"m{m}-N{N}", N, pat))
    return [(name, N, np.ascontiguousarray(p, dtype=np.int32)) for name, N, p in out]


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("case", range(6), ids=[c[0] for c in sampling_cases()])
def test_sampling_at_the_edges_of_its_grid_passes(rls, ctx, dt, case):
    """gather, both spellings of the adjoint and the mask: beta = 0 on NaN-filled destinations (they are not read: no NaN comes out),
    beta != 0 (complex for the complex types) on small integers, all exact; guards intact behind index N - 1"""
    lib, dt = ctx.lib, np.dtype(dt)
    name, N, pat = sampling_cases()[case]
    m = pat.size
    assert pat.max() == N - 1
    S = samp_op(rls, ctx, dt, N, pat)
    x, y = R.ints(dt, N, 1), R.ints(dt, m, 2)
    xg, yg = guarded(rls, ctx, x), guarded(rls, ctx, y)
    scalars = [(1.0, 0.0), (-2.0, 0.0), (2.0, 0.5)] + ([(2 - 1j, 1 + 2j), (1j, 0.0)] if dt.kind == "c" else [])
    for alpha, beta in scalars:
        a, b = complex(alpha), complex(beta)
        if beta == 0.0:   # NaN-filled destinations
            got = twice(rls, ctx, dt, m, [(xg, x)], lambda p: lib.rls_sampling_mul(S, OP_N, a.real, a.imag, xg.ptr, 0.0, 0.0, p))
            assert np.array_equal(got, (alpha * MR.sampling(x, pat)).astype(dt)), (name, alpha)   # (NaN equals nothing)
            for op in (OP_T, OP_C):
                got = twice(rls, ctx, dt, N, [(yg, y)], lambda p: lib.rls_sampling_mul(S, op, a.real, a.imag, yg.ptr, 0.0, 0.0, p))
                assert not np.isnan(got).any()
                assert np.array_equal(got, (alpha * MR.sampling_adj(y, pat, N)).astype(dt)), (name, alpha, op)
        else:
            y0, x0 = R.ints(dt, m, 3), R.ints(dt, N, 4)
            og = guarded(rls, ctx, y0)
            assert lib.rls_sampling_mul(S, OP_N, a.real, a.imag, xg.ptr, b.real, b.imag, og.ptr) == 0
            assert np.array_equal(og.read(), (alpha * MR.sampling(x, pat) + beta * y0).astype(dt)), (name, alpha, beta)
            for op in (OP_T, OP_C):
                og = guarded(rls, ctx, x0)
                assert lib.rls_sampling_mul(S, op, a.real, a.imag, yg.ptr, b.real, b.imag, og.ptr) == 0
                assert np.array_equal(og.read(), (alpha * MR.sampling_adj(y, pat, N) + beta * x0).astype(dt)), (name, alpha, beta, op)
    want = (MR.sampling_mask(pat, N) * x).astype(dt)
    got = twice(rls, ctx, dt, N, [(xg, x)], lambda p: lib.rls_sampling_mul_normal(S, xg.ptr, p))
    assert np.array_equal(got, want)
    zg = guarded(rls, ctx, x)
    assert lib.rls_sampling_mul_normal(S, zg.ptr, zg.ptr) == 0 and np.array_equal(zg.read(), want)
    assert same(xg, x) and same(yg, y)
    assert lib.rls_sampling_destroy(S) == 0


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", R.DT, ids=R.DT_IDS)
def test_refusals_on_a_live_context(rls, paths, dt):
    """every refusal returns its status code, writes nothing, and leaves the same handles able to complete a valid call with the
    results they gave before"""
    ctx, lib, dt = paths, paths.lib, np.dtype(dt)
    other = np.dtype(np.complex128 if dt == R.C64 else np.complex64)
    shape, N = (8, 4), 32
    pat = MR.pattern(N, 8, 4)
    F, S = fft_op(rls, ctx, dt, shape), samp_op(rls, ctx, dt, N, pat)
    S_type, S_size = samp_op(rls, ctx, other, N, pat), samp_op(rls, ctx, dt, 16, pat[pat < 16])
    x, y = R.gauss(dt, N, 1), R.gauss(dt, pat.size, 2)
    xg, yg = guarded(rls, ctx, x), guarded(rls, ctx, y)
    og, pg = nan_out(rls, ctx, dt, N), nan_out(rls, ctx, dt, pat.size)
    nan_n, nan_m = np.full(N, NAN[dt]), np.full(pat.size, NAN[dt])

    def valid():
        """one call of each entry point on the same handles"""
        a = twice(rls, ctx, dt, pat.size, [(xg, x)], lambda p: lib.rls_sampling_mul(S, OP_N, 1.0, 0.0, xg.ptr, 0.0, 0.0, p))
        b = twice(rls, ctx, dt, N, [(xg, x)], lambda p: lib.rls_fft_apply(F, 0, xg.ptr, p))
        c = twice(rls, ctx, dt, pat.size, [(xg, x)], lambda p: lib.rls_fft_sampled_mul(F, S, OP_N, xg.ptr, p))
        d = twice(rls, ctx, dt, N, [(yg, y)], lambda p: lib.rls_fft_sampled_mul(F, S, OP_C, yg.ptr, p))
        e = twice(rls, ctx, dt, N, [(xg, x)], lambda p: lib.rls_fft_sampled_mul_normal(F, S, xg.ptr, p))
        return b"".join(v.tobytes() for v in (a, b, c, d, e)), (a, b, c, d, e)

    first, (a, b, c, d, e) = valid()
    g = R.gate(dt, shape) * R.ref_factor(dt, shape)
    fx = R.reference(x, shape, True, True, False, dt)
    assert np.array_equal(a, x[pat]) and np.array_equal(c, b[pat])
    assert np.max(np.abs(b.astype(fx.dtype) - fx)) <= g * float(np.linalg.norm(fx.astype(np.complex128)))
    refusals = [
        ("sampling_mul x == y", lambda: lib.rls_sampling_mul(S, OP_N, 1.0, 0.0, og.ptr, 0.0, 0.0, og.ptr), E_INVALID),
        ("sampling_mul op 3", lambda: lib.rls_sampling_mul(S, 3, 1.0, 0.0, xg.ptr, 0.0, 0.0, pg.ptr), E_INVALID),
        ("sampling_mul op -1", lambda: lib.rls_sampling_mul(S, -1, 1.0, 0.0, xg.ptr, 0.0, 0.0, pg.ptr), E_INVALID),
        ("sampling_mul null x", lambda: lib.rls_sampling_mul(S, OP_N, 1.0, 0.0, None, 0.0, 0.0, pg.ptr), E_INVALID),
        ("fft_sampled_mul RLS_OP_T", lambda: lib.rls_fft_sampled_mul(F, S, OP_T, xg.ptr, pg.ptr), E_UNSUPPORTED),
        ("fft_sampled_mul op 3", lambda: lib.rls_fft_sampled_mul(F, S, 3, xg.ptr, pg.ptr), E_INVALID),
        ("fft_sampled_mul x == y", lambda: lib.rls_fft_sampled_mul(F, S, OP_C, og.ptr, og.ptr), E_INVALID),
        ("fft_sampled_mul other element type", lambda: lib.rls_fft_sampled_mul(F, S_type, OP_N, xg.ptr, pg.ptr), E_INVALID),
        ("fft_sampled_mul other size", lambda: lib.rls_fft_sampled_mul(F, S_size, OP_N, xg.ptr, pg.ptr), E_INVALID),
        ("fft_sampled_mul_normal other element type", lambda: lib.rls_fft_sampled_mul_normal(F, S_type, xg.ptr, og.ptr), E_INVALID),
        ("fft_sampled_mul_normal other size", lambda: lib.rls_fft_sampled_mul_normal(F, S_size, xg.ptr, og.ptr), E_INVALID),
        ("fft_apply adjoint = 2", lambda: lib.rls_fft_apply(F, 2, xg.ptr, og.ptr), E_INVALID),
        ("fft_apply adjoint = -1", lambda: lib.rls_fft_apply(F, -1, xg.ptr, og.ptr), E_INVALID),
        ("fft_apply null y", lambda: lib.rls_fft_apply(F, 0, xg.ptr, None), E_INVALID),
    ]
    line = R.MAX_LINE[dt]
    creates = [("flags 4", (8, 4), 4, E_INVALID), ("flags 7", (8, 4), 7, E_INVALID), ("ndims 0", (), 3, E_INVALID), ("an extent of 0", (8, 0), 3, E_INVALID),
               ("a negative extent", (-8, 4), 3, E_INVALID), ("three extents", (2, 2, 2), 3, E_UNSUPPORTED), ("three extents around a unit one", (2, 1, 2, 2), 3, E_UNSUPPORTED),
               ("no power of two", (12,), 3, E_UNSUPPORTED), ("no power of two in an image", (8, 6), 3, E_UNSUPPORTED),
               ("a line of twice the maximum", (2 * line,), 3, E_UNSUPPORTED), ("a line of twice the maximum in an image", (2, 2 * line), 3, E_UNSUPPORTED)]
    for name, call, want in refusals:
        assert call() == want, name
        ctx.sync()
        assert og.read().tobytes() == nan_n.tobytes() and pg.read().tobytes() == nan_m.tobytes(), f"{name}: an output was written"
        assert valid()[0] == first, f"after {name}"
    for name, shp, flags, want in creates:
        st, h = fft_create(rls, ctx, dt, shp, True, True, flags=flags)
        assert st == want and not h.value, name
    idx = lambda *v: np.array(v, dtype=np.int32)
    for name, n, p, m, want in (("m > N", 4, idx(0, 1, 2, 3, 3), 5, E_INVALID), ("a repeated index", 8, idx(0, 5, 5), None, E_INVALID),
                                ("an index equal to N", 8, idx(0, 8), None, E_INVALID), ("a negative index", 8, idx(-1, 2), None, E_INVALID),
                                ("m = 0", 8, idx(0), 0, E_INVALID)):
        st, h = samp_create(rls, ctx, dt, n, p, m)
        assert st == want and not h.value, name
    assert valid()[0] == first
    assert same(xg, x) and same(yg, y)
    for h in (S, S_type, S_size):
        assert lib.rls_sampling_destroy(h) == 0
    assert lib.rls_fft_destroy(F) == 0
