"""tests/vec_ref.py, the checker of the Float32 / ComplexF32 vector kernels (csrc/blas1.hip, prox.hip, nested.hip, the ADMM bookkeeping
of solvers.hip), held to the oracle and to its own gates -- no GPU.

  anchor   prox_l1's scaled call of O.prox_l1 equals the map written out with eps(Float32) at float64, and O.prox_l1 itself at
           float32; the serial L21 restatement equals O.prox_l21 / O.norm_l21 at float64; clamp + shift_scale and shift_scale +
           restore_outside equal O.ClampedScalingTransform's transform / inverse_transform bit for bit.
  gates    on the very inputs and lengths of tests/test_gpu_vec_edges.py: the float32 evaluation is inside every gate against the
           float64 evaluation (a correct Float32 implementation passes), and each planted mistake breaks a gate at every length
           where it applies (a wrong kernel does not)."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pgm_ref as P  # noqa: E402
import rls_oracle as O  # noqa: E402
import vec_ref as V  # noqa: E402

WORST = {}


def inside(group, case, got, want, gate):
    """got within gate of want (gate None: the same bytes as the float32 evaluation, which `want` then is)"""
    if gate is None:
        return np.asarray(got).tobytes() == np.asarray(want).tobytes()
    r, ok = V.ratio(V.err(got, want), gate)
    if ok and r > WORST.get(group, (-1.0, ""))[0]:
        WORST[group] = (r, case)
    return ok


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for g, (r, c) in sorted(WORST.items()):
        print(f"\nfloat32 evaluation, largest error / bound, {g}: {r:.3e}  ({c})")


# ---- anchors -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", V.DT, ids=V.DT_IDS)
def test_prox_l1_is_the_oracles_map_with_the_float32_eps(dt):
    x = V.l1_input(dt, 257)
    want = P.prox_l1(V.cast(x, 64), np.float64(V.L1_LAM), eps=V.EPS32)
    got = V.prox_l1(x, V.L1_LAM, 64)
    assert np.max(V.err(got, want)) <= 4 * 2.0 ** -53 * float(np.max(V.mag(x)))
    f32 = O.prox_l1(x.copy(), V.L1_LAM)
    if V.is_cplx(dt):   # (NumPy's complex64 modulus is up to 1.9 ulp off; vec_ref rounds it once)
        assert np.max(V.err(V.prox_l1(x, V.L1_LAM, 32), f32)) <= 8 * V.U * float(np.max(V.mag(x)))
    else:
        assert V.prox_l1(x, V.L1_LAM, 32).tobytes() == f32.tobytes()
    if not V.is_cplx(dt):   # (it matters: with ITS eps the float64 oracle is further from the Float32 operation than the real gate is wide)
        other = O.prox_l1(V.cast(x, 64), np.float64(V.L1_LAM))
        assert not V.ratio(V.err(other, got), V.gate_l1(x, V.L1_LAM))[1]


@pytest.mark.parametrize("dt", V.DT, ids=V.DT_IDS)
@pytest.mark.parametrize("name,n,slices", V.L21_CASES[:8], ids=[c[0] for c in V.L21_CASES[:8]])
def test_serial_l21_lines_are_the_oracles_at_float64(dt, name, n, slices):
    lam = np.float32(0.4)
    x = V.l21_input(dt, n, slices, lam)
    want, wnorm, _ = V.l21_ref(x, lam, slices)
    got, gnorm = V.l21_lines(x, lam, slices, 64)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and not np.isnan(want).any()
    assert np.max(V.err(got, want)) <= 1e-13 * float(np.max(V.mag(x))) and abs(gnorm - wnorm) <= 1e-13 * wnorm


def test_transforms_are_the_oracles_bit_for_bit():
    x = V.clamp_input(257)
    lo, hi = V.CLAMP_LO, V.CLAMP_HI
    t = O.ClampedScalingTransform(x, lo, hi)
    fwd = V.shift_scale(V.clamp(x, lo, hi), lo, hi - lo, 0, 32)
    assert fwd.dtype == np.float32 and fwd.tobytes() == t.transform(x).tobytes()
    back = V.restore_outside(V.shift_scale(fwd, lo, hi - lo, 1, 32), x, lo, hi)
    assert back.tobytes() == t.inverse_transform(fwd).tobytes()
    assert back[0] == x[0] == lo and back[1] == x[1] == hi       # lo is inside (rescaled to itself), hi is outside (restored)
    z = O.ZTransform(x)
    assert V.shift_scale(x, z.mean, z.std, 0, 32).tobytes() == z.transform(x).tobytes()


# ---- elementwise ---------------------------------------------------------------------------------------------------------------------
def _unwritten(o, got, i):
    """the output with element i left as it was before the launch (a fresh output holds the sentinel)"""
    from test_gpu_f64_plan_products import SENTINEL

    bad = np.array(got, copy=True)
    bad[i] = SENTINEL[bad.dtype] if o["out0"] is None else o["out0"][i]
    return bad


@pytest.mark.parametrize("dt", V.DT, ids=V.DT_IDS)
@pytest.mark.parametrize("n", V.EW_N, ids=lambda n: f"n{n}")
def test_elementwise_gates_admit_float32_and_see_an_unwritten_element(dt, n):
    for name, (args, outs) in V.ew_cases(dt, n).items():
        for o in outs:
            case = f"{np.dtype(dt).name} n={n} {name}"
            want = o["got32"] if o["gate"] is None else o["want"]
            assert inside(f"{name} {o['name']}", case, o["got32"], want, o["gate"]), case
            if name == "prox_real" and np.dtype(dt) == np.float32 or name == "admm_pre-accumulate1" and o["name"] == "xold":
                assert np.asarray(o["got32"]).tobytes() == o["out0"].tobytes()    # nothing to write: every byte stays
                continue
            for k, i in zip(V.watch(n), o["watch"]):
                if k in (n - 1, V.GRID_CAP):                                          # the last element, the first of a second pass
                    assert not inside("", "", _unwritten(o, o["got32"], i), want, o["gate"]), (case, o["name"], i)


@pytest.mark.parametrize("n", V.EW_N, ids=lambda n: f"n{n}")
def test_l1_eps_on_the_imaginary_part_and_strict_upper_limit_are_seen(n):
    (args, (o,)) = V.ew_cases(np.complex64, n)["prox_l1-small"]
    wrong = V.prox_l1(o["out0"], args["lam"], 32, eps_imag=True)
    assert not V.ratio(V.err(wrong, o["want"]), o["gate"])[1]
    orig, out0 = V.restore_input(n), V.vector(np.float32, n, 52)
    good = V.restore_outside(out0, orig, V.CLAMP_LO, V.CLAMP_HI)
    assert V.restore_outside(out0, orig, V.CLAMP_LO, V.CLAMP_HI, strict_upper=True).tobytes() != good.tobytes()


# ---- reductions ----------------------------------------------------------------------------------------------------------------------
def _red_errs(dt, res, s64):
    nrm, asum, dot = res
    return abs(float(nrm) - math.sqrt(s64[0])), abs(float(asum) - s64[1]), abs(complex(dot) - s64[2])


@pytest.mark.parametrize("dt", V.DT, ids=V.DT_IDS)
@pytest.mark.parametrize("n", V.RED_N, ids=lambda n: f"n{n}")
def test_reduction_gates_admit_double_sums_and_see_every_planted_mistake(dt, n):
    x, y, s64, s32 = V.red_case(dt, n)
    gates = V.gates_red(dt, n, s64)
    case = f"{np.dtype(dt).name} n={n}"
    for name, e, g in zip(("nrm2", "asum", "dotc"), _red_errs(dt, V.results32(s32), s64), gates):
        assert inside(name, case, e, 0.0, [g]), (case, name, e, g)
    if n == 1:
        return
    assert abs(s64[2]) <= 4e-6 * s64[3], (case, abs(s64[2]) / s64[3])           # the dotc inputs do cancel
    # leaving out one element of modulus 4: the last one; the last one under the cap and the first one past it where n reaches them
    drop = {n - 1} | {i for i in (V.RED_CAP * V.RED_PER_WG - 1, V.RED_CAP * V.RED_PER_WG) if i < n}
    for i in drop:
        assert abs(abs(complex(x[i])) - 4.0) < 1e-2 and abs(abs(complex(y[i])) - 4.0) < 0.1, (case, i)
        t = V.sums(x, y, 32, i, i + 1)
        short = tuple(a - b for a, b in zip(s32, t))
        for name, e, g in zip(("nrm2", "asum", "dotc"), _red_errs(dt, V.results32(short), s64), gates):
            assert e > g, (case, name, i, e, g)
    if n >= V.RED_PER_WG - 1:
        # sums held in Float32 (serially, as one thread would): nrm2 and the cancelling dotc both leave their gates, dotc by far
        s2_f32 = float(np.cumsum((x.real * x.real + x.imag * x.imag) if V.is_cplx(dt) else x * x, dtype=np.float32)[-1])
        assert abs(float(np.float32(math.sqrt(s2_f32))) - math.sqrt(s64[0])) > gates[0], case
        pr = np.conj(x) * y
        d_f32 = complex(np.cumsum(pr.real, dtype=np.float32)[-1], np.cumsum(pr.imag, dtype=np.float32)[-1] if V.is_cplx(dt) else 0.0)
        print(f"{case}: Float32-accumulated dotc misses its gate by a factor {abs(d_f32 - s64[2]) / gates[2]:.3g}")
        # (around 2048 * 8192 the worst-case bound of a double sum, n 2^-53 sum |x||y|, is as wide as the typical error of a Float32
        # accumulator, 1e-9 sum |x||y|: the factor printed there is about 1, and it is the sizes up to 8193 that tell the two apart)
        if n <= 4 * V.RED_PER_WG:
            assert abs(d_f32 - s64[2]) > 1000.0 * gates[2], (case, abs(d_f32 - s64[2]) / gates[2])


@pytest.mark.parametrize("dt", V.DT, ids=V.DT_IDS)
@pytest.mark.parametrize("n", V.STAT_N, ids=lambda n: f"n{n}")
def test_stats_gates_admit_double_sums_and_see_a_dropped_element(dt, n):
    for where in ("first", "last", "cap"):
        x, pos = V.stats_input(dt, n, where)
        want, got, gate = V.stats(x, 64), V.stats(x, 32), V.gate_stats(x)
        case = f"{np.dtype(dt).name} n={n} {where}"
        assert want[1] == (24 if V.is_cplx(dt) else 40) and want[4] == 40 and (n == 1 or want[0] == -33), case
        assert inside("stats", case, np.abs(got - want), 0.0, gate), (case, got - want, gate)
        if n > 1:
            short = V.stats(np.delete(x, pos), 32)                # the element at `pos` left out: the maxima and both sums show it
            assert np.all(np.abs(short - want)[[1, 2, 3, 4]] > gate[[1, 2, 3, 4]]), case


# ---- admm_post -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", V.DT, ids=V.DT_IDS)
@pytest.mark.parametrize("kind", ["generic", "x=z", "xold=x"])
@pytest.mark.parametrize("n", V.POST_N, ids=lambda n: f"n{n}")
def test_admm_post_gates_admit_float32_and_see_a_late_du(dt, kind, n):
    x, xold, z, zold, u = V.admm_input(dt, n, kind)[:5]
    case = f"{np.dtype(dt).name} n={n} {kind}"
    un = V.admm_post_u(x, z, u, 32)
    assert inside("admm_post u", case, un, V.admm_post_u(x, z, u, 64), V.gate_admm_post_u(x, z, u)), case
    want = V.admm_post_out(x, xold, z, zold, u, un, 64)
    gate = V.gate_admm_post_out(want, n, dt)
    assert inside("admm_post out", case, np.abs(V.admm_post_out(x, xold, z, zold, u, un, 32) - want), 0.0, gate), case
    assert (want[3] == 0) == (kind == "x=z") and (want[5] == 0) == (kind == "xold=x")
    if kind != "x=z":                                             # (x = z: u_new = u, there is no ||u_new - u|| to lose)
        late = V.admm_post_out(x, xold, z, zold, u, un, 32, late_du=True)
        assert abs(late[0] - want[0]) > gate[0], case


# ---- L21 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", V.DT, ids=V.DT_IDS)
@pytest.mark.parametrize("name,n,slices", V.L21_CASES, ids=[c[0] for c in V.L21_CASES])
def test_l21_gates_admit_a_serial_float32_sum_and_see_a_lost_tail(dt, name, n, slices):
    lam = np.float32(0.4)
    x = V.l21_input(dt, n, slices, lam)
    want, wnorm, g = V.l21_ref(x, lam, slices)
    gate, ngate = V.gate_l21(x, lam, slices, g)
    got, gnorm = V.l21_lines(x, lam, slices, 32)
    case = f"{np.dtype(dt).name} {name}"
    assert inside("prox_l21", case, got, want, gate), case
    assert inside("norm_l21", case, abs(float(gnorm) - wnorm), 0.0, [ngate]), case
    slen = n // slices
    if slen >= 4:
        assert not got[1::slen].any() and not got[2::slen].any() and got[3::slen].all(), case   # zero group, g = lambda / 2, g = 2 lambda
    if n % slices:
        bad, bnorm = V.l21_lines(x, lam, slices, 32, ragged=False)
        assert not V.ratio(V.err(bad, want), gate)[1] and abs(float(bnorm) - wnorm) > ngate, case
