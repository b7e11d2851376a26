"""The Float32 / ComplexF32 vector kernels of csrc/blas1.hip, csrc/prox.hip, csrc/nested.hip and rls_admm_pre / rls_admm_post of
csrc/solvers.hip, through the C ABI, at every launch geometry: the 256-thread grid-stride kernels up to the first length of a second
pass, the two-stage reductions on either side of one workgroup and of the partials cap, rls_stats around its 818 records, the
single-workgroup admm_post around its 1024-thread stride, L21 with one thread per group.

References, inputs, lengths and gates are those of tests/vec_ref.py (derived in its docstring, u = 2^-24; held to the oracle and to
planted mistakes by tests/test_vec_ref.py on the CPU).  Every output vector has GUARD sentinel elements in front and behind that
must come back bit-identical, every input vector must come back bit-identical, and every launch is made twice on fresh copies and
must return the same bytes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rls_oracle as O  # noqa: E402  (the checker)
import vec_ref as V  # noqa: E402
from test_gpu_f64_plan_products import GUARD, SENTINEL, Guarded, _report, held, vector  # noqa: E402,F401

pytestmark = pytest.mark.gpu
E_INVALID = -1


def code_of(rls, ctx, dt):
    return rls.DeviceVector(1, dt, ctx).code


def guarded(rls, ctx, a=None, dt=None, n=None):
    """a device copy of `a` (int32: its bytes) between two guards; a is None: n sentinel elements of type dt"""
    if a is None:
        return Guarded(rls, ctx, dt, n, lead=GUARD)
    a = np.ascontiguousarray(a)
    body = a.view(np.float32) if a.dtype == np.int32 else a
    return Guarded(rls, ctx, body.dtype, body.size, body=body, lead=GUARD)


def same(g, a):
    """the vector behind g holds a's bytes (and its guards are intact)"""
    return g.read().tobytes() == np.ascontiguousarray(a).tobytes()


def fl(v):
    return float(np.float32(v))


# ---- elementwise -----------------------------------------------------------------------------------------------------------------------
def launch(lib, h, code, n, name, a, p):
    """the entry point of case `name`: scalars from a, device pointers from p"""
    base = name.split("-")[0]
    ca, cb = complex(a.get("a", 0)), complex(a.get("b", 0))
    if base == "fill":
        return lib.rls_fill(h, code, n, p["x"], ca.real, ca.imag)
    if base == "scal":
        return lib.rls_scal(h, code, n, ca.real, ca.imag, p["x"])
    if base == "axpy":
        return lib.rls_axpy(h, code, n, ca.real, ca.imag, p["x"], p["y"])
    if base == "lincomb":
        return lib.rls_lincomb(h, code, n, ca.real, ca.imag, p["x"], cb.real, cb.imag, p["y"], p["z"])
    if base == "axpby":
        return lib.rls_axpby(h, code, n, ca.real, ca.imag, p["x"], cb.real, cb.imag, p["y"])
    if base in ("prox_l1", "prox_l2"):
        return getattr(lib, "rls_" + base)(h, code, n, p["x"], fl(a["lam"]))
    if base in ("prox_positive", "prox_real"):
        return getattr(lib, "rls_" + base)(h, code, n, p["x"])
    if base == "gather":
        return lib.rls_gather(h, code, n, p["idx"], p["x"], p["out"])
    if base == "scatter":
        return lib.rls_scatter(h, code, n, p["idx"], p["in"], p["x"])
    if base == "shift_scale":
        return lib.rls_shift_scale(h, n, p["x"], fl(a["shift"]), fl(a["scale"]), a["inverse"])
    if base == "clamp":
        return lib.rls_clamp(h, n, p["x"], fl(a["lo"]), fl(a["hi"]))
    if base == "restore_outside":
        return lib.rls_restore_outside(h, n, p["out"], p["orig"], fl(a["lo"]), fl(a["hi"]))
    if base == "complex_split":
        return lib.rls_complex_split(h, n, p["z"], p["re"], p["im"])
    if base == "complex_merge":
        return lib.rls_complex_merge(h, n, p["re"], p["im"], p["z"])
    if base == "admm_pre":
        return lib.rls_admm_pre(h, code, n, p["beta"], p["beta_y"], p["z"], p["u"], p["x"], p["xold"], fl(a["rho"]), a["accumulate"])
    raise AssertionError(name)


def run_once(rls, ctx, dt, n, name, args, outs):
    """one launch on fresh guarded copies: the outputs, after the inputs and the guards have been checked"""
    ins = {k: guarded(rls, ctx, v) for k, v in args.items() if isinstance(v, np.ndarray)}
    og = {o["name"]: guarded(rls, ctx, o["out0"], o["got32"].dtype, len(o["got32"])) for o in outs}
    p = {k: g.ptr for k, g in ins.items()}
    p.update({k: g.ptr for k, g in og.items()})
    p.setdefault("y", None)
    st = launch(ctx.lib, ctx.handle, code_of(rls, ctx, dt), n, name, args, p)
    assert st == 0, (name, ctx.lib.rls_last_error_string(ctx.handle))
    got = [og[o["name"]].read().copy() for o in outs]
    for k, g in ins.items():
        assert same(g, args[k]), f"{name}: input {k} was written"
    return got


@pytest.mark.parametrize("dt", V.DT, ids=V.DT_IDS)
@pytest.mark.parametrize("n", V.EW_N, ids=lambda n: f"n{n}")
def test_elementwise_kernels_up_to_a_second_grid_pass(rls, ctx, dt, n):
    """every entry point of vec_ref.ew_cases: rls_fill, rls_scal, rls_axpy, rls_lincomb (b != 0; b = 0 with y = NULL and with a NaN y),
    rls_axpby in place, rls_prox_l1 (at O(1) and at 1e-3, where eps(Float32) shows), rls_prox_l2, rls_prox_positive, rls_prox_real,
    rls_gather / rls_scatter (a permutation, a sparse sorted subset), rls_shift_scale (both modes), rls_clamp, rls_restore_outside,
    rls_complex_split / rls_complex_merge, rls_admm_pre (accumulate 0 and 1)"""
    for name, (args, outs) in V.ew_cases(dt, n).items():
        case = f"{np.dtype(dt).name} n={n}"
        got, again = run_once(rls, ctx, dt, n, name, args, outs), run_once(rls, ctx, dt, n, name, args, outs)
        for o, g, g2 in zip(outs, got, again):
            what = f"{name} {o['name']} {case}"
            assert g.tobytes() == g2.tobytes(), f"{what}: two launches differ"
            if o["gate"] is None:
                for i in o["watch"]:
                    assert g[i].tobytes() == o["got32"][i].tobytes(), (what, i, g[i], o["got32"][i])
                assert g.tobytes() == np.ascontiguousarray(o["got32"]).tobytes(), what
            else:
                e = V.err(g, o["want"])
                for i in o["watch"]:
                    assert e[i] <= o["gate"][i], (what, i, g[i], o["want"][i])
                held(f"rls_{name} {o['name']} {np.dtype(dt).name}", f"n={n}", e, o["gate"])
        if name.startswith("prox_l1"):
            x = outs[0]["out0"]
            # exact zeros, |x| < lambda, |x| = lambda: exact zeros out (complex: hypotf may land an ulp above a modulus of lambda, so
            # only moduli four roundings below it are held to an exact zero; the gate covers the rest)
            zero = np.nonzero(V.mag(x) <= float(args["lam"]) * (1.0 - 4.0 * V.U * V.is_cplx(dt)))[0]
            assert (zero.size or n == 1) and not got[0][zero].any(), (name, case)


# ---- two-stage reductions ------------------------------------------------------------------------------------------------------------------
_dev_big = {}


def big_on_device(rls, ctx, dt):
    key = np.dtype(dt)
    if key not in _dev_big:
        x, y = V.red_big(dt)[:2]
        _dev_big[key] = (rls.DeviceVector.from_host(x, ctx), rls.DeviceVector.from_host(y, ctx))
    return _dev_big[key]


@pytest.mark.parametrize("dt", V.DT, ids=V.DT_IDS)
@pytest.mark.parametrize("n", V.RED_N, ids=lambda n: f"n{n}")
def test_reductions_on_either_side_of_every_launch_geometry(rls, ctx, dt, n):
    """rls_nrm2, rls_asum, rls_dotc, and rls_nrm2_dev / rls_dotc_dev into a guarded device result: 8192 is the last n that one
    workgroup finalises directly, 2048 * 8192 the last n below the partials cap (2048 partials: the whole scratch block)"""
    lib, h, code = ctx.lib, ctx.handle, code_of(rls, ctx, dt)
    x, y, s64, _ = V.red_case(dt, n)
    big = n > 4 * V.RED_PER_WG
    if big:
        xd, yd = big_on_device(rls, ctx, dt)
        xp, yp = xd.ptr, yd.ptr
    else:
        xg, yg = guarded(rls, ctx, x), guarded(rls, ctx, y)
        xp, yp = xg.ptr, yg.ptr
    gates = V.gates_red(dt, n, s64)
    want = (np.sqrt(s64[0]), s64[1], s64[2])
    case = f"n={n}"
    if n > 1:
        assert abs(s64[2]) <= 4e-6 * s64[3]                              # the dotc inputs cancel
    runs = []
    for _ in range(2):
        r1, r2, r3 = (C.c_float * 2)(), (C.c_float * 2)(), (C.c_float * 2)()
        assert lib.rls_nrm2(h, code, n, xp, r1) == 0 and lib.rls_asum(h, code, n, xp, r2) == 0 and lib.rls_dotc(h, code, n, xp, yp, r3) == 0
        d1, d3 = guarded(rls, ctx, None, np.float32, 2), guarded(rls, ctx, None, np.float32, 2)
        assert lib.rls_nrm2_dev(h, code, n, xp, d1.ptr) == 0 and lib.rls_dotc_dev(h, code, n, xp, yp, d3.ptr) == 0
        runs.append(bytes(r1)[:4] + bytes(r2)[:4] + bytes(r3) + d1.read().tobytes() + d3.read().tobytes())
    assert runs[0] == runs[1], f"{case}: two launches differ"
    d1, d3 = d1.read(), d3.read()
    assert bytes(r1)[:4] == d1[:1].tobytes() and d1[1] == 0 and bytes(r3) == d3.tobytes()   # the _dev forms: the same numbers, im = 0
    name = np.dtype(dt).name
    held(f"rls_nrm2 {name}", case, [abs(float(r1[0]) - want[0])], [gates[0]])
    held(f"rls_asum {name}", case, [abs(float(r2[0]) - want[1])], [gates[1]])
    held(f"rls_dotc {name}", case, [abs(complex(r3[0], r3[1]) - want[2])], [gates[2]])
    if not V.is_cplx(dt):
        assert r3[1] == 0.0
    if big:
        assert xd.to_host()[:n].tobytes() == x.tobytes() and yd.to_host()[:n].tobytes() == y.tobytes()
    else:
        assert same(xg, x) and same(yg, y)


# ---- rls_stats ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", V.DT, ids=V.DT_IDS)
@pytest.mark.parametrize("n", V.STAT_N, ids=lambda n: f"n{n}")
def test_stats_around_its_partial_records(rls, ctx, dt, n):
    """min, max of the real parts and max |x| exact, sum and sum of squares of the real parts to the double bound; the extrema in the
    first element, in the last, and in element 818 * 8192 (the first of a second pass of workgroup 0)"""
    lib, h, code = ctx.lib, ctx.handle, code_of(rls, ctx, dt)
    for where in ("first", "last", "cap"):
        x, pos = V.stats_input(dt, n, where)
        xg = guarded(rls, ctx, x)
        out, again = (C.c_double * 5)(), (C.c_double * 5)()
        assert lib.rls_stats(h, code, n, xg.ptr, out) == 0 and lib.rls_stats(h, code, n, xg.ptr, again) == 0
        assert bytes(out) == bytes(again)
        want, gate = V.stats(x, 64), V.gate_stats(x)
        got = np.array(out[:])
        assert got[0] == want[0] and got[1] == want[1] and got[4] == want[4] == 40, (n, where, got, want)
        held(f"rls_stats sums {np.dtype(dt).name}", f"n={n} extrema {where}", np.abs(got - want)[2:4], gate[2:4])
        assert same(xg, x)


# ---- rls_admm_post -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", V.DT, ids=V.DT_IDS)
@pytest.mark.parametrize("n,kind", [(n, "generic") for n in V.POST_N] + [(1025, "x=z"), (1025, "xold=x")], ids=lambda v: str(v))
def test_admm_post_around_its_thread_stride(rls, ctx, dt, n, kind):
    lib, h, code = ctx.lib, ctx.handle, code_of(rls, ctx, dt)
    x, xold, z, zold, u = V.admm_input(dt, n, kind)[:5]
    runs = []
    for _ in range(2):
        ins = [guarded(rls, ctx, v) for v in (x, xold, z, zold)]
        ug, out = guarded(rls, ctx, u), (C.c_float * 6)()
        assert lib.rls_admm_post(h, code, n, ins[0].ptr, ins[1].ptr, ins[2].ptr, ins[3].ptr, ug.ptr, out) == 0
        un = ug.read().copy()
        assert all(same(g, v) for g, v in zip(ins, (x, xold, z, zold)))
        runs.append(un.tobytes() + bytes(out))
    assert runs[0] == runs[1]
    name, case = np.dtype(dt).name, f"n={n} {kind}"
    held(f"rls_admm_post u {name}", case, V.err(un, V.admm_post_u(x, z, u, 64)), V.gate_admm_post_u(x, z, u))
    want = V.admm_post_out(x, xold, z, zold, u, un, 64)
    got = np.array(out[:], dtype=np.float64)
    held(f"rls_admm_post out {name}", case, np.abs(got - want), V.gate_admm_post_out(want, n, dt))
    if kind == "x=z":
        assert got[3] == 0.0                                            # r = 0 exactly (u_new = (u + x) - x need not be u: two roundings)
    if kind == "xold=x":
        assert got[5] == 0.0


# ---- L21 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", V.DT, ids=V.DT_IDS)
@pytest.mark.parametrize("name,n,slices", V.L21_CASES, ids=[c[0] for c in V.L21_CASES])
def test_l21_with_one_thread_per_group(rls, ctx, dt, name, n, slices):
    """rls_prox_l21 and rls_norm_l21 at lambda = 0.4, and rls_prox_l21 at lambda = 0.  Where there are at least four groups, group 1
    is all zero (exact zeros for lambda > 0; NaN in that group and nowhere else for lambda = 0), group 2 has g = lambda / 2 (exact
    zeros) and group 3 g = 2 lambda"""
    lib, h, code = ctx.lib, ctx.handle, code_of(rls, ctx, dt)
    lam, slen, case, tname = np.float32(0.4), n // slices, f"{name} n={n} slices={slices}", np.dtype(dt).name
    x = V.l21_input(dt, n, slices, lam)
    want, wnorm, g = V.l21_ref(x, lam, slices)
    gate, ngate = V.gate_l21(x, lam, slices, g)
    runs = []
    for _ in range(2):
        xg, xin, res = guarded(rls, ctx, x), guarded(rls, ctx, x), (C.c_float * 1)()
        assert lib.rls_prox_l21(h, code, n, slices, xg.ptr, fl(lam)) == 0 and lib.rls_norm_l21(h, code, n, slices, xin.ptr, fl(lam), res) == 0
        got = xg.read().copy()
        assert same(xin, x)
        runs.append(got.tobytes() + bytes(res))
    assert runs[0] == runs[1]
    assert not np.isnan(got).any()
    held(f"rls_prox_l21 {tname}", case, V.err(got, want), gate)
    held(f"rls_norm_l21 {tname}", case, [abs(float(res[0]) - wnorm)], [ngate])
    if slen >= 4:
        assert not got[1::slen].any() and not got[2::slen].any() and got[3::slen].all(), case
    # lambda = 0: the factor is g / g = 1 (three roundings allowed for: gam(3) |x|), NaN in an all-zero group
    x0 = V.l21_input(dt, n, slices, np.float32(0.0))
    xg = guarded(rls, ctx, x0)
    assert lib.rls_prox_l21(h, code, n, slices, xg.ptr, 0.0) == 0
    got0 = xg.read()
    nan = (np.arange(n) % slen == 1) if slen >= 4 else np.zeros(n, dtype=bool)
    assert np.array_equal(np.isnan(got0), nan), case
    held(f"rls_prox_l21 lambda=0 {tname}", case, V.err(got0[~nan], x0[~nan]), V.gam(3) * V.mag(x0[~nan]))


@pytest.mark.parametrize("dt", V.DT, ids=V.DT_IDS)
def test_l21_one_long_group_summed_in_float32(rls, ctx, parity, dt):
    """slices = n = 65536: one thread sums 65536 squares serially in Float32, where every other reduction of these files accumulates
    in double.  lambda is half the group norm: the factor is q = 1/2 and its conditioning (lambda / g) / q = 1, so the relative
    error of the result is the relative error of the group norm itself.  Gate: the project's parity gate (1e-5 relative to the
    float64 oracle, or twice the Float32 oracle's own error) -- and the derived gate of vec_ref, which is far wider here."""
    n = V.LONG_GROUP
    x = vector(dt, n, 65)
    lam = np.float32(0.5 * np.sqrt(np.sum(V.mag(x) ** 2)))
    want, _, g = V.l21_ref(x, lam, n)
    ref32 = O.prox_l21(x.copy(), lam, n)
    xg = guarded(rls, ctx, x)
    assert ctx.lib.rls_prox_l21(ctx.handle, code_of(rls, ctx, dt), n, n, xg.ptr, fl(lam)) == 0
    got = xg.read()
    held(f"rls_prox_l21 {np.dtype(dt).name}", f"one long group n={n}", V.err(got, want), V.gate_l21(x, lam, n, g)[0])
    e = float(np.linalg.norm(V.err(got, want)) / np.linalg.norm(want))
    e32 = float(np.linalg.norm(V.err(ref32, want)) / np.linalg.norm(want))
    print(f"L21 one long group n={n} {np.dtype(dt).name}: device vs float64 oracle {e:.3e}, Float32 oracle vs float64 oracle {e32:.3e}")
    parity(f"l21_long_group_{np.dtype(dt).name}", got, want, ref32)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", V.DT, ids=V.DT_IDS)
def test_refusals_leave_everything_alone(rls, ctx, dt):
    """null pointers, n < 0, slices of 0 and above n, rls_admm_post with n = 0: RLS_E_INVALID, and no vector is touched"""
    lib, h, code, n = ctx.lib, ctx.handle, code_of(rls, ctx, dt), 8
    v = [vector(dt, n, 200 + i) for i in range(6)]
    g = [guarded(rls, ctx, a) for a in v]
    a, b, c, d, e, f = (q.ptr for q in g)
    fr, fi = vector(np.float32, n, 210), vector(np.float32, n, 211)
    rg, ig = guarded(rls, ctx, fr), guarded(rls, ctx, fi)
    idx = guarded(rls, ctx, np.arange(n, dtype=np.int32))
    res, dres, six = (C.c_float * 2)(), (C.c_double * 5)(), (C.c_float * 6)()
    dev = guarded(rls, ctx, None, np.float32, 2)
    calls = []
    for m, px in ((n, None), (-1, a)):                                   # a null vector; a negative length
        calls += [lambda m=m, px=px: lib.rls_fill(h, code, m, px, 1.0, 0.0), lambda m=m, px=px: lib.rls_scal(h, code, m, 2.0, 0.0, px),
                  lambda m=m, px=px: lib.rls_axpy(h, code, m, 2.0, 0.0, px, b), lambda m=m, px=px: lib.rls_axpy(h, code, m, 2.0, 0.0, b, px),
                  lambda m=m, px=px: lib.rls_lincomb(h, code, m, 2.0, 0.0, px, 1.0, 0.0, b, c),
                  lambda m=m, px=px: lib.rls_lincomb(h, code, m, 2.0, 0.0, b, 1.0, 0.0, c, px),
                  lambda m=m, px=px: lib.rls_axpby(h, code, m, 2.0, 0.0, b, 1.0, 0.0, px),
                  lambda m=m, px=px: lib.rls_prox_l1(h, code, m, px, 0.1), lambda m=m, px=px: lib.rls_prox_l2(h, code, m, px, 0.1),
                  lambda m=m, px=px: lib.rls_prox_positive(h, code, m, px), lambda m=m, px=px: lib.rls_prox_real(h, code, m, px),
                  lambda m=m, px=px: lib.rls_prox_l21(h, code, m, 2, px, 0.1), lambda m=m, px=px: lib.rls_norm_l21(h, code, m, 2, px, 0.1, res),
                  lambda m=m, px=px: lib.rls_gather(h, code, m, idx.ptr, px, b), lambda m=m, px=px: lib.rls_gather(h, code, m, idx.ptr, b, px),
                  lambda m=m, px=px: lib.rls_scatter(h, code, m, idx.ptr, px, b), lambda m=m, px=px: lib.rls_scatter(h, code, m, idx.ptr, b, px),
                  lambda m=m, px=px: lib.rls_stats(h, code, m, px, dres),
                  lambda m=m, px=px: lib.rls_nrm2(h, code, m, px, res), lambda m=m, px=px: lib.rls_asum(h, code, m, px, res),
                  lambda m=m, px=px: lib.rls_dotc(h, code, m, px, b, res), lambda m=m, px=px: lib.rls_dotc(h, code, m, b, px, res),
                  lambda m=m, px=px: lib.rls_nrm2_dev(h, code, m, px, dev.ptr), lambda m=m, px=px: lib.rls_dotc_dev(h, code, m, b, px, dev.ptr),
                  lambda m=m, px=px: lib.rls_admm_post(h, code, m, px, b, c, d, e, six), lambda m=m, px=px: lib.rls_admm_post(h, code, m, b, c, d, e, px, six)]
        calls += [lambda m=m, px=px, k=k: lib.rls_admm_pre(h, code, m, *[px if j == k else q for j, q in enumerate((a, b, c, d, e, f))], 0.5, 0)
                  for k in range(6)]
        pr = None if px is None else rg.ptr
        calls += [lambda m=m, pr=pr: lib.rls_shift_scale(h, m, pr, 0.1, 2.0, 0), lambda m=m, pr=pr: lib.rls_clamp(h, m, pr, 0.0, 1.0),
                  lambda m=m, pr=pr: lib.rls_restore_outside(h, m, pr, ig.ptr, 0.0, 1.0), lambda m=m, pr=pr: lib.rls_restore_outside(h, m, ig.ptr, pr, 0.0, 1.0),
                  lambda m=m, pr=pr: lib.rls_complex_split(h, m, a, pr, ig.ptr), lambda m=m, pr=pr: lib.rls_complex_split(h, m, a, ig.ptr, pr),
                  lambda m=m, pr=pr: lib.rls_complex_merge(h, m, pr, ig.ptr, a), lambda m=m, pr=pr: lib.rls_complex_merge(h, m, ig.ptr, pr, a)]
    calls += [lambda: lib.rls_gather(h, code, n, None, a, b), lambda: lib.rls_scatter(h, code, n, None, a, b),
              lambda: lib.rls_complex_split(h, n, None, rg.ptr, ig.ptr), lambda: lib.rls_complex_merge(h, n, rg.ptr, ig.ptr, None),
              lambda: lib.rls_nrm2(h, code, n, a, None), lambda: lib.rls_asum(h, code, n, a, None), lambda: lib.rls_dotc(h, code, n, a, b, None),
              lambda: lib.rls_nrm2_dev(h, code, n, a, None), lambda: lib.rls_dotc_dev(h, code, n, a, b, None),
              lambda: lib.rls_stats(h, code, n, a, None), lambda: lib.rls_norm_l21(h, code, n, 2, a, 0.1, None),
              lambda: lib.rls_admm_post(h, code, n, a, b, c, d, e, None), lambda: lib.rls_admm_post(h, code, 0, a, b, c, d, e, six)]
    for slices in (0, n + 1):
        calls += [lambda s=slices: lib.rls_prox_l21(h, code, n, s, a, 0.1), lambda s=slices: lib.rls_norm_l21(h, code, n, s, a, 0.1, res)]
    for i, call in enumerate(calls):
        assert call() == E_INVALID, f"refusal {i}"
    ctx.sync()
    assert all(same(q, w) for q, w in zip(g, v)) and same(rg, fr) and same(ig, fi) and same(idx, np.arange(n, dtype=np.int32))
    assert dev.read().tobytes() == np.full(2, SENTINEL[np.dtype(np.float32)]).tobytes()
