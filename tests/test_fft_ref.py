"""tests/fft_ref.py, the checker of the FFT kernels (csrc/fft.hip), held to tests/matfree_ref.py, to its own gates and to planted
mistakes -- no GPU.

  anchor    the complex128 restatement of the kernels' order of operations equals matfree_ref.fft / fft_adj / fft_adj(mask fft) to 1e-13
            of the norm, and the long-double references agree with each other.
  gates     on the very shapes and inputs of tests/test_gpu_fft_edges.py the working-precision restatement is inside every gate (a
            correct kernel passes) ...
  plants    ... and each planted mistake breaks one at the smallest shape where it can show (a wrong kernel does not).
  regimes   over that shape table pass_plan reports every launch regime of fft_pass that the element type can reach, the bundle
            loop along dimension 1 (8192 x 8192) excepted."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fft_ref as R  # noqa: E402
import matfree_ref as MR  # noqa: E402

WORST = {}
OLD_GATE = {R.C64: 1e-5, R.C128: 1e-12}   # tests/test_gpu_matfree.py, relative to the norm


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.complex128) - np.asarray(b, np.complex128)) / max(np.linalg.norm(np.asarray(b, np.complex128)), 1e-300))


def worst_ratio(triples):
    """(largest error / bound, its label) of fft_ref.judge's triples"""
    best = (0.0, "")
    for label, e, b in triples:
        e, b = np.asarray(e, np.float64), np.asarray(b, np.float64)
        bad = ~(e <= b)
        r = float("inf") if bad.any() and not np.all(b[bad] > 0) else float(np.max(e / np.maximum(b, 1e-300)))
        if r > best[0]:
            best = (r, label)
    return best


def judged(dt, shape, shift, unitary, adjoint, plant=None, kinds=None):
    kw = {} if kinds is None else {"kinds": kinds}
    names, X = R.inputs(dt, shape, shift, unitary, adjoint, **kw)
    got = R.transform(X, shape, shift, unitary, adjoint, dt, plant)
    assert got.dtype == np.dtype(dt)
    want = R.reference(X, shape, shift, unitary, adjoint, dt)
    return worst_ratio(R.judge(dt, shape, shift, unitary, names, X, got, want, R.ref_factor(dt, shape)))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for g, (r, c) in sorted(WORST.items()):
        print(f"\nworking-precision restatement, largest error / gate, {g}: {r:.3e}  ({c})")


def shape_class(dt, shape):
    if len(shape) == 1:
        return "lines"
    return "general-path images" if shape in R.GENERAL[np.dtype(dt)] or shape == R.BIG else "single-workgroup images"


# ---- anchors -------------------------------------------------------------------------------------------------------------------------
def test_gates_are_the_derived_numbers():
    assert abs(R.gate(np.complex64, (2,)) / 5.8e-7 - 1) < 0.02 and abs(R.gate(np.complex64, (8192,)) / 6.1e-6 - 1) < 0.02
    assert abs(R.gate(np.complex128, (2,)) / 1.1e-15 - 1) < 0.05 and abs(R.gate(np.complex128, (4096,)) / 1.1e-14 - 1) < 0.06
    assert R.gate(np.complex64, (64, 128)) == R.gate(np.complex64, (8192,)) and R.gate(np.complex64, (4, 1, 8)) == R.gate(np.complex64, (32,))
    assert R.gate(np.complex64, (1,)) == 2 * R.U[R.C64]


@pytest.mark.parametrize("dt", R.DT, ids=R.DT_IDS)
def test_restatement_in_complex128_is_numpy_fft(dt):
    """every shape of the device table of up to 4096 points under all four flag pairs, the larger ones under (True, True): forward,
    adjoint and the normal operator with a random third of the samples"""
    for shape in R.shapes(dt):
        N = R.points(shape)
        x = R.gauss(np.complex128, N, 7 + N)
        mask = MR.sampling_mask(R.masks(shape)[-1][1], N) if N >= 3 else np.ones(N)
        for shift, unitary in (R.FLAGS if N <= R.ALL_FLAGS_UP_TO else R.FLAGS[:1]):
            case = (shape, shift, unitary)
            assert rel(R.transform(x, shape, shift, unitary), MR.fft(x, shape, shift, unitary)) <= 1e-13, case
            assert rel(R.transform(x, shape, shift, unitary, adjoint=True), MR.fft_adj(x, shape, shift, unitary)) <= 1e-13, case
            want = MR.fft_adj(mask * MR.fft(x, shape, shift, unitary), shape, shift, unitary)
            assert rel(R.normal(x, mask, shape, shift, unitary), want) <= 1e-13, case
            assert rel(R.reference(x, shape, shift, unitary, False, dt), MR.fft(x, shape, shift, unitary)) <= 1e-13, case
            assert rel(R.reference(x, shape, shift, unitary, True, dt), MR.fft_adj(x, shape, shift, unitary)) <= 1e-13, case


def test_long_double_references_agree():
    """the DFT matrix in long double against numpy.fft in long double and the long-double restatement: three routes to one number"""
    if not R.LONG:   # long double is double here: nothing to compare, the ComplexF64 gates are doubled instead (fft_ref.ref_factor)
        return
    tol = 64 * float(np.finfo(np.longdouble).eps)
    for shape in ((1,), (2,), (64,), (2, 2), (8, 32), (64, 64), (4, 1, 8)):
        x = R.gauss(np.complex128, R.points(shape), 5)
        for shift, unitary in R.FLAGS:
            for adjoint in (False, True):
                a = R.by_dft_matrix(x, shape, shift, unitary, adjoint)
                b = R.transform(x, shape, shift, unitary, adjoint, dtype=np.clongdouble)
                assert a.dtype == b.dtype == R.CLD
                assert float(np.linalg.norm(a - b) / np.linalg.norm(a)) <= tol, (shape, shift, unitary, adjoint)
                if R.LONG_FFT:
                    X = x.astype(R.CLD).reshape(tuple(1 << e for e in R.extents(shape)), order="F")
                    c = np.fft.fftshift(np.fft.fftn(np.fft.ifftshift(X))) if shift else np.fft.fftn(X)
                    if not adjoint and unitary:
                        assert float(np.linalg.norm(a - c.ravel(order="F") / np.sqrt(np.longdouble(x.size))) / np.linalg.norm(a)) <= tol


# ---- gates -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", R.DT, ids=R.DT_IDS)
def test_working_precision_restatement_is_inside_every_gate(dt):
    """every shape, flag pair, direction and input of the device tier (the 1024 x 8192 case is left to the device and numpy.fft)"""
    for shape in R.shapes(dt):
        for shift, unitary in R.flags_of(shape):
            for adjoint in (False, True):
                r, label = judged(dt, shape, shift, unitary, adjoint)
                case = f"{shape} shift={shift} unitary={unitary} adjoint={adjoint} {label}"
                assert r <= 1.0, (case, r)
                key = f"{np.dtype(dt).name} {shape_class(dt, shape)}"
                if r > WORST.get(key, (-1.0, ""))[0]:
                    WORST[key] = (r, case)


@pytest.mark.parametrize("dt", R.DT, ids=R.DT_IDS)
@pytest.mark.parametrize("shape", R.NORMAL_SHAPES, ids=str)
def test_working_precision_normal_operator_is_inside_its_gate(dt, shape):
    N = R.points(shape)
    x = R.gauss(dt, N, 40 + N)
    for shift, unitary in R.flags_of(shape):
        s2 = 1.0 if unitary else float(N)
        for name, pat in R.masks(shape):
            mask = MR.sampling_mask(pat, N)
            got = R.normal(x, mask, shape, shift, unitary, dt)
            want = R.reference_normal(x, mask, shape, shift, unitary, dt)
            bound = R.gate_normal(dt, shape) * R.ref_factor(dt, shape) * s2 * float(np.linalg.norm(x))
            err = np.abs(got.astype(want.dtype) - want).astype(np.float64)
            assert float(np.linalg.norm(err)) <= bound, (shape, shift, unitary, name)
            key = f"{np.dtype(dt).name} normal operator"
            r = float(np.linalg.norm(err)) / bound
            if r > WORST.get(key, (-1.0, ""))[0]:
                WORST[key] = (r, f"{shape} shift={shift} unitary={unitary} mask {name}")
            # bit for bit adjoint(mask(forward)): the same operations in the same order
            three = R.transform(R.transform(x, shape, shift, unitary, False, dt) * mask.astype(R.real_of(dt)), shape, shift, unitary, True, dt)
            assert got.tobytes() == three.tobytes(), (shape, shift, unitary, name)


# ---- planted mistakes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", R.DT, ids=R.DT_IDS)
def test_table_stride_ignored(dt):
    """lgtw: shows only where the extents differ (the shorter one reads the longer one's table); the first stride-dependent twiddle is
    -i of an extent of 4 beside an extent of 8"""
    for shape in ((4, 8), (8, 4)):
        for adjoint in (False, True):
            assert judged(dt, shape, True, True, adjoint, "lgtw")[0] > 1.0, (shape, adjoint)
    assert judged(dt, (8, 8), True, True, False, "lgtw")[0] <= 1.0 and judged(dt, (2, 8), True, True, False, "lgtw")[0] <= 1.0


@pytest.mark.parametrize("dt", R.DT, ids=R.DT_IDS)
def test_global_sign_of_an_extent_of_two_dropped(dt):
    for shape in ((2,), (2, 4), (4, 2)):
        for adjoint in (False, True):
            assert judged(dt, shape, True, True, adjoint, "sign2")[0] > 1.0, (shape, adjoint)
    assert judged(dt, (2,), False, True, False, "sign2")[0] <= 1.0 and judged(dt, (2, 2), True, True, False, "sign2")[0] <= 1.0   # (two minus signs)


@pytest.mark.parametrize("dt", R.DT, ids=R.DT_IDS)
def test_shift_sign_on_the_input_side_only(dt):
    for shape in ((2,), (4,), (2, 2)):
        for adjoint in (False, True):
            assert judged(dt, shape, True, True, adjoint, "shift_in_only")[0] > 1.0, (shape, adjoint)
    assert judged(dt, (4,), False, True, False, "shift_in_only")[0] <= 1.0


@pytest.mark.parametrize("dt", R.DT, ids=R.DT_IDS)
def test_mask_at_natural_positions(dt):
    """caught by ONE sample at an index whose reversal differs, on a rectangular image -- and by no sample at a self-reversed index"""
    shape = (8, 32)
    N = R.points(shape)
    x = R.gauss(dt, N, 77)
    bound = R.gate_normal(dt, shape) * R.ref_factor(dt, shape) * float(np.linalg.norm(x))
    for name, pat in R.masks(shape):
        mask = MR.sampling_mask(pat, N)
        err = float(np.linalg.norm((R.normal(x, mask, shape, True, True, dt, "mask_natural").astype(R.ref_type(dt))
                                    - R.reference_normal(x, mask, shape, True, True, dt)).astype(np.complex128)))
        selfrev = name in ("ones", "one@0", f"one@{N - 1}")
        assert (err <= bound) == selfrev, (name, err, bound)
    assert R.nonself(shape, (0, N - 1)) not in (None, 0, N - 1)


@pytest.mark.parametrize("dt", R.DT, ids=R.DT_IDS)
def test_adjoint_twiddles_not_conjugated(dt):
    """an extent of 2 has the twiddle 1 alone; -i of an extent of 4 is the first to tell"""
    for shape in ((4,), (2, 4)):
        assert judged(dt, shape, True, True, True, "noconj")[0] > 1.0, shape
    assert judged(dt, (2,), True, True, True, "noconj")[0] <= 1.0 and judged(dt, (4,), True, True, False, "noconj")[0] <= 1.0


@pytest.mark.parametrize("dt", R.DT, ids=R.DT_IDS)
def test_scale_in_both_passes(dt):
    for adjoint in (False, True):
        assert judged(dt, (2, 2), True, True, adjoint, "scale_twice")[0] > 1.0
    assert judged(dt, (2, 2), True, False, False, "scale_twice")[0] <= 1.0 and judged(dt, (4,), True, True, False, "scale_twice")[0] <= 1.0


def _old_and_new(plant, shape):
    """a ComplexF64 transform with a planted table: its error on dense random input relative to the norm, as tests/test_gpu_matfree.py
    measures it, and error / gate of the new checks"""
    x = R.gauss(np.complex128, R.points(shape), 9)
    old = rel(R.transform(x, shape, True, True, False, np.complex128, plant), MR.fft(x, shape))
    return old, judged(np.complex128, shape, True, True, False, plant)[0]


def test_float32_table_on_the_complex_f64_path():
    """np.cos / np.sin on float32 angles: eps(Float32) in every twiddle but 1 and -i, so an extent of 8 is the first to show it.  It
    breaks the new gate by seven orders of magnitude.  It does NOT pass the old 1e-12 gate either, as had been expected of it: the
    error is about 1e-8 of the norm at every extent from 8 on (printed).  The table mistake that the old gate cannot see is the
    next test's."""
    for shape in ((8,), (4096,), (8, 32)):
        old, new = _old_and_new("table32", shape)
        print(f"float32 table, ComplexF64 {shape}: {old:.3e} of the norm, {new:.3e} of the new gate")
        assert new > 1.0 and old > OLD_GATE[R.C128], shape
    assert _old_and_new("table32", (4,))[1] <= 1.0   # (1 and -i alone)


def test_table_by_recurrence_passes_the_old_gate_and_fails_the_new():
    """w_j = w_(j-1) w_1 in double: the rounding of w_1 grows with j to about n u / 2 at the end of the table.  At the longest
    ComplexF64 line that is within the old 1e-12 of the norm and beyond the new gate (1.1e-14): the gap this file closes"""
    old, new = _old_and_new("recurrence", (4096,))
    print(f"table by recurrence, ComplexF64 (4096,): {old:.3e} of the norm, {new:.3e} of the new gate")
    assert old <= OLD_GATE[R.C128] and new > 1.0, (old, new)


# ---- regimes -----------------------------------------------------------------------------------------------------------------------------
def regimes(dt, shape):
    out = set()
    for dim1, p in enumerate(R.passes(dt, shape)):
        if p.how == ("base",):
            out.add(("lgb", "base"))
        out |= {("lgb", h) for h in p.how if h in ("floor", "clamp")}
        if "shrink" in p.how:
            out.add(("shrink to", p.lgb))
        if p.lgb == 0 and not dim1 and R.extents(shape)[1] > 0:
            out.add(("lgb 0 on dimension 0 inside an image",))
        if p.exact_fit:
            out.add(("exact fit",))
        if p.idle:
            out.add(("idle threads",))
        out |= {("threads", p.threads), ("stage trips", p.stage_trips), ("bundle trips dim1" if dim1 else "bundle trips", p.bundle_trips)}
    return out


@pytest.mark.parametrize("dt", R.DT, ids=R.DT_IDS)
def test_the_device_table_reaches_every_regime(dt):
    """whatever ANY supported shape of the element type reaches (all extent pairs up to the longest line, enumerated), the table reaches
    -- but for a second trip of the bundle loop along dimension 1, whose smallest shape is 8192 x 8192 (512 MiB)"""
    L = R.lg(R.MAX_LINE[np.dtype(dt)])
    reachable = set()
    for lg1 in range(L + 1):
        for lg2 in range(L + 1):
            reachable |= regimes(dt, (1 << lg1, 1 << lg2))
    table = set()
    for shape in R.shapes(dt) + ([R.BIG] if np.dtype(dt) == R.C64 else []):
        table |= regimes(dt, shape)
    exempt = {("bundle trips dim1", 2)}
    assert reachable - table <= exempt, sorted(reachable - table, key=str)
    assert (exempt <= reachable) == (np.dtype(dt) == R.C64)
    want = {("lgb", "base"), ("lgb", "floor"), ("lgb", "clamp"), ("shrink to", 2), ("shrink to", 1), ("shrink to", 0), ("exact fit",),
            ("idle threads",), ("threads", 64), ("threads", 512), ("threads", 1024), ("stage trips", 1), ("stage trips", 2),
            ("bundle trips", 1), ("lgb 0 on dimension 0 inside an image",)}
    if np.dtype(dt) == R.C64:   # ComplexF64: 4096 points a workgroup and 4096 bundles at the most
        want |= {("stage trips", 4), ("bundle trips", 2)}
    else:
        assert ("stage trips", 4) not in reachable and ("bundle trips", 2) not in reachable
    assert want <= table, sorted(want - table, key=str)


def test_named_shapes_take_the_regimes_they_are_named_for():
    c64, c128 = np.complex64, np.complex128
    assert R.pass_plan(c64, 1, 12, True)[:2] == (1, ("base", "floor", "clamp")) and R.pass_plan(c64, 1, 12, True).exact_fit
    assert R.pass_plan(c128, 1, 12, True)[:2] == (0, ("base", "floor", "clamp", "shrink"))
    assert R.pass_plan(c64, 3, 10, True)[:2] == (3, ("base", "floor")) and R.pass_plan(c64, 3, 10, True).exact_fit
    assert R.pass_plan(c128, 3, 10, True).lgb == 2 and R.pass_plan(c64, 4, 11, True).lgb == 2 and R.pass_plan(c128, 4, 11, True).lgb == 1
    assert R.pass_plan(c64, 2, 12, True)[:2] == (1, ("base", "floor", "clamp", "shrink"))
    assert R.pass_plan(c64, 3, 13, True).lgb == 0 and R.pass_plan(c128, 3, 12, True).lgb == 0
    p = R.pass_plan(c64, 10, 13, False)
    assert (p.lgb, p.bundles, p.grid, p.bundle_trips) == (0, 8192, 4096, 2)
    assert [R.pass_plan(c64, k, 0, False).stage_trips for k in (0, 1, 11, 12, 13)] == [0, 1, 1, 2, 4]
    assert R.pass_plan(c64, 10, 0, False)[:2] == (0, ("base",)) and R.pass_plan(c64, 9, 0, False)[:2] == (0, ("base", "clamp"))
    # the single-workgroup launch: 256 threads up to 2048 points, 16384 ComplexF32 / 8192 ComplexF64 points the most that fit
    assert R.fused_threads(5, 6) == R.fused_threads(11, 0) == 256 and R.fused_threads(6, 6) == R.fused_threads(12, 0) == 1024
    assert R.fused_fits(c64, 13, 1) and not R.fused_fits(c64, 13, 2) and R.fused_fits(c128, 12, 1) and not R.fused_fits(c128, 12, 2)
    assert [R.use_fused(c64, 5, 5, lv) for lv in (0, 1, 2)] == [False, True, True] and [R.use_fused(c64, 6, 5, lv) for lv in (0, 1, 2)] == [False, False, True]
