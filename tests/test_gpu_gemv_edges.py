"""The Float32 / ComplexF32 GEMV of csrc/gemv.hip, y = alpha op(A) x + beta y, in every loop regime, kernel variant and load path,
through the C ABI as it is: rls_gemv, rls_operator_* and the tune switches gemvn_g, gemvn_waves, gemvt_cols, gemvt_reverse.

Two kinds of data, two acceptance criteria; every case runs both, with beta != 0 and with beta = 0 over a NaN-filled y.
  integers  A, x, y0 uniform in [-7, 7] (complex: both parts), alpha, beta = 2, -1 (complex: 1 - 2j, 2j).  Every product and every
            partial sum is an integer below 2^24 in magnitude (asserted on the host before each launch), so Float32 holds it exactly
            in any order of summation, fused or not: the result must EQUAL the integer reference.  A dropped, doubled or misplaced
            term fails this however long the contraction.  (The reference has no negative zero, and neither has the kernel: its sums
            start from +0, and x + (-x) is +0 in round-to-nearest.  The comparison is by value.)
  Gaussian  reference: the Float32 inputs promoted to float64 / complex128.  Bound, per output entry and for any summation order,
            with u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., (3.5)):
                |got - ref|_i <= c g(k) (|alpha| (|op(A)| |x|)_i + |beta| |y0|_i),   g(k) = k u / (1 - k u)
            real: k = n + 4, c = 1; complex: k = 2 n + 4, c = sqrt 2 (n the contraction length; a component of a complex dot product
            is a real sum of 2 n products; + 4 covers alpha s, beta y and the final add).  This is gamma() of
            test_gpu_f64_plan_products.py with the denominator kept: n u is not negligible at n = 9000.  Derived, never measured;
            tests/test_gemv_edges_host.py shows that a plain Float32 evaluation in NumPy stays inside it.

Guards in every case: y and x are Guarded (elements in front of y and behind both must come back bit-identical; x's excess is NaN), A
has lda > M with NaN in the padding rows (and in front, where A is offset), so a clamped or masked load that leaks shows as NaN.

The case generators and the restatement of the host's choices (t_plan, n_plan) need no device: tests/test_gemv_edges_host.py imports
them and checks that every case lands in the regime its id names and that every regime and instantiation is named."""
import ctypes as C
import math
import os
import sys
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_f64_plans import upload_padded  # noqa: E402
from test_gpu_f64_plan_products import GUARD, LD, Guarded, _report, held, is_cplx, note, vector  # noqa: E402,F401

pytestmark = pytest.mark.gpu
F32, C64 = np.dtype(np.float32), np.dtype(np.complex64)
DTS = [("f32", F32), ("c64", C64)]
OP_N, OP_T, OP_C = 0, 1, 2
OP_NAME = {OP_N: "N", OP_T: "T", OP_C: "C"}
U24 = 2.0 ** -24
VEC = {F32: 4, C64: 2}            # elem<E>::vec: elements per 16-byte load
TILE = {F32: 4096, C64: 2048}     # gemv_n_kernel: x staged through LDS 16 KiB at a time
T_THREADS, UNROLL = 256, 8        # launch_t: WAVES = 4, U = 8; launch_n: U = 8
SPAN = T_THREADS * UNROLL         # chunks of one unpredicated trip of gemv_t_kernel
POOL = {F32: 2_400_000, C64: 700_000}   # the largest operand of each type, in elements (under 10 MB)
TUNE_DEFAULT = dict(gemvn_g=0, gemvn_waves=0, gemvt_cols=0, gemvt_reverse=-1)
Y_LEAD = 3
EXACT = {"launches": 0}


def scalars(dt, beta_zero=False):
    al, be = (1 - 2j, 2j) if is_cplx(dt) else (2 + 0j, -1 + 0j)
    return al, (0j if beta_zero else be)


def g(k):
    """k u / (1 - k u), u = 2^-24"""
    return k * U24 / (1.0 - k * U24)


def bound_factor(dt, n):
    """c g(k) of the module docstring for a contraction of n elements of type dt"""
    return math.sqrt(2.0) * g(2 * n + 4) if is_cplx(dt) else g(n + 4)


# ---- the host's choices, restated (gemv.hip: gemv_typed, dispatch_t, launch_t, dispatch_n, launch_n and the kernels' trip counts) ---
def t_plan(dt, M, N, lda, a_off=0, x_off=0, cols=0):
    """a_off, x_off: byte offsets of A and x from a 16-byte boundary.  Every operand here is far below the 256 MiB switch."""
    V = VEC[np.dtype(dt)]
    NV = V if (a_off % 16 == 0 and lda % V == 0 and M % V == 0 and x_off % 16 == 0) else 1
    Mc = M // NV
    if cols == 0:
        cols = 8 if N >= 4096 else 4 if N >= 2048 else 2 if N >= 1024 else 1
    grid = -(-N // cols)
    return SimpleNamespace(NV=NV, Mc=Mc, COLS=cols, spans=Mc // SPAN, tail=Mc % SPAN, grid=grid, dup=grid * cols - N)


def n_plan(dt, M, N, lda, a_off=0, G=0, waves=0):
    """tiles: (nt, main_rounds, rounds) of every x tile; live: chunks of the last workgroup that are not clamped"""
    dt = np.dtype(dt)
    V = VEC[dt]
    NV = V if (a_off % 16 == 0 and lda % V == 0 and M % V == 0) else 1
    Mc = -(-M // NV)
    if G == 0:
        G = next((c for c in (64, 32, 16) if -(-Mc // c) >= 256), 8)
    rb = -(-Mc // G)
    if waves == 0:
        waves = 16 if rb <= 256 else 8 if rb <= 512 else 4
    if NV == 1:
        G = 64
    CPR = waves * (64 // G)
    grid = -(-Mc // G)
    tiles = []
    for t0 in range(0, N, TILE[dt]):
        nt = min(N - t0, TILE[dt])
        tiles.append((nt, nt // CPR // UNROLL * UNROLL, -(-nt // CPR)))
    return SimpleNamespace(NV=NV, Mc=Mc, G=G, WAVES=waves, CPR=CPR, grid=grid, live=Mc - (grid - 1) * G, tiles=tiles)


def pad_for(dt, M, lda_vec, odd=False):
    """the smallest padding >= 1 whose lda = M + pad is (lda_vec) or is not a multiple of V; `odd`: an odd lda"""
    V = VEC[np.dtype(dt)]
    for pad in range(1, V + 2):
        if ((M + pad) % V == 0) == lda_vec and (not odd or (M + pad) % 2 == 1):
            return pad
    raise AssertionError((dt, M, lda_vec, odd))


# ---- cases --------------------------------------------------------------------------------------------------------------------------
# claims: what the id names -- NV, COLS or G / WAVES, and the regimes of rows and columns; checked against t_plan / n_plan on the host
Case = namedtuple("Case", "kernel name dt M N pad a_lead x_lead tune claims")


def case(kernel, name, dt, M, N, pad, a_lead=0, x_lead=0, tune=None, **claims):
    return Case(kernel, name, np.dtype(dt), M, N, pad, a_lead, x_lead, dict(tune or {}), claims)


def plan_of(c):
    """the restated launch of a case"""
    item = c.dt.itemsize
    if c.kernel == "t":
        return t_plan(c.dt, c.M, c.N, c.M + c.pad, c.a_lead * item, c.x_lead * item, c.tune.get("gemvt_cols", 0))
    return n_plan(c.dt, c.M, c.N, c.M + c.pad, c.a_lead * item, c.tune.get("gemvn_g", 0), c.tune.get("gemvn_waves", 0))


def params(cases):
    return [pytest.param(c, id=c.name) for c in cases]


def layout(dt, Mc, nv, way=None):
    """(M, pad, a_lead) of an operand of Mc chunks: NV = V (nv == "V": M = Mc V, everything aligned) or NV = 1 (M = Mc) by one `way`
    -- 'M' (M % V != 0, lda % V == 0, needs Mc % V != 0), 'lda' (an odd lda), 'A' (A one element off a 16-byte boundary, lda % V == 0).
    Without a way: 'M' where it can be, else 'lda'."""
    V = VEC[np.dtype(dt)]
    if nv == "V":
        return Mc * V, V, 0
    if way is None or (way == "M" and Mc % V == 0):
        way = "M" if Mc % V else "lda"
    if way == "lda":
        return Mc, pad_for(dt, Mc, False, odd=True), 0
    return Mc, pad_for(dt, Mc, True), (1 if way == "A" else 0)


T_ROWS = [(1, "one-live-lane"), (255, "below-one-slice"), (256, "one-slice"), (257, "one-slice+1"), (2047, "tail-only"),
          (2048, "full-only"), (2049, "full+one-chunk-tail"), (4353, "two-spans+tail")]
T_COLS = (1, 2, 4, 8)
NVS = ("V", "1")


def t_col_regime(COLS, N):
    return ("one-column" if N == 1 else "short-workgroup" if N == COLS - 1 else "exact-workgroup" if N == COLS
            else "second-workgroup-one-live" if N == COLS + 1 else "three-workgroups")


def t_row_cases():
    out = []
    for kind, dt in DTS:
        for nv in NVS:
            for COLS in (1, 8):
                for Mc, regime in T_ROWS:
                    M, pad, _ = layout(dt, Mc, nv)
                    out.append(case("t", f"gemv_t-{kind}-NV{nv}-COLS{COLS}-Mc{Mc}-{regime}", dt, M, COLS + 1, pad,
                                    tune=dict(gemvt_cols=COLS), NV=nv, COLS=COLS, rows=regime, cols="second-workgroup-one-live"))
    return out


def t_way_cases():
    """the four conditions of the vector path, broken one at a time at 2049 chunks (x offset: ops T / C fall back, op N does not)"""
    out = []
    for kind, dt in DTS:
        V = VEC[dt]
        for way, (M, pad, a_lead, x_lead) in (("M%V", (2049, pad_for(dt, 2049, True), 0, 0)), ("lda%V", (2049 * V, 1, 0, 0)),
                                              ("A-offset", (2049 * V, V, 1, 0)), ("x-offset", (2049 * V, V, 0, 1))):
            out.append(case("t", f"gemv_t-{kind}-NV1-by-{way}-M{M}", dt, M, 3, pad, a_lead, x_lead, NV="1", COLS=1, rows="full+tail",
                            way=way))
    return out


def t_col_cases():
    out = []
    for kind, dt in DTS:
        for nv in NVS:
            for COLS in T_COLS:
                for Mc in (257, 2049):
                    for N in sorted({n for n in (1, COLS - 1, COLS, COLS + 1, 2 * COLS + 1) if n > 0}):
                        M, pad, _ = layout(dt, Mc, nv)
                        out.append(case("t", f"gemv_t-{kind}-NV{nv}-COLS{COLS}-N{N}-{t_col_regime(COLS, N)}-Mc{Mc}", dt, M, N, pad,
                                        tune=dict(gemvt_cols=COLS), NV=nv, COLS=COLS, cols=t_col_regime(COLS, N),
                                        rows="one-slice+1" if Mc == 257 else "full+one-chunk-tail"))
    return out


def t_auto_cases():
    out = []
    for kind, dt in DTS:
        for N in (1023, 1024, 2047, 2048, 4095, 4096, 4099):
            COLS = 8 if N >= 4096 else 4 if N >= 2048 else 2 if N >= 1024 else 1
            out.append(case("t", f"gemv_t-{kind}-auto-N{N}-COLS{COLS}", dt, 2 * VEC[dt], N, VEC[dt], NV="V", COLS=COLS))
    return out


# gemv_n: the 12 G x WAVES instantiations at NV = V, the 3 WAVES at NV = 1 (G = 64 whatever is forced; G = 8 is forced to show it)
N_INST = [("V", G, W, None) for G in (8, 16, 32, 64) for W in (4, 8, 16)] + [("1", 64, 4, "M"), ("1", 64, 8, "lda"), ("1", 64, 16, "A")]


def n_inst_name(nv, G, W):
    return f"NV{nv}-G{G}-W{W}"


def n_case(kind, dt, inst, Mc, N, tag, **claims):
    nv, G, W, way = inst
    M, pad, a_lead = layout(dt, Mc, nv, way)          # ('M' where M % V != 0 cannot hold at this row count: an odd lda)
    return case("n", f"gemv_n-{kind}-{n_inst_name(nv, G, W)}-{tag}", dt, M, N, pad, a_lead,
                tune=dict(gemvn_g=G if nv == "V" else 8, gemvn_waves=W), NV=nv, G=G, WAVES=W, **claims)


def n_col_list(dt, CPR):
    last = "steady+remainder" if 17 * CPR + 1 <= TILE[dt] else "steady-tile-then-remainder-tile"   # (CPR = 128 at TILE = 2048)
    return [(1, "one-column"), (CPR - 1, "remainder-only-short-round"), (CPR, "remainder-only-one-full-round"),
            (CPR + 1, "remainder-only-two-rounds"), (8 * CPR - 1, "remainder-only-eight-rounds"), (8 * CPR, "prologue-only"),
            (8 * CPR + 1, "prologue+remainder"), (16 * CPR, "one-steady-trip"), (17 * CPR + 1, last)]


def n_col_cases():
    out = []
    for kind, dt in DTS:
        for inst in N_INST:
            G, W = inst[1], inst[2]
            for N, regime in n_col_list(dt, W * (64 // G)):
                out.append(n_case(kind, dt, inst, G + 1, N, f"N{N}-{regime}", cols=regime, rows="second-workgroup-one-live"))
    return out


N_TILE_INST = [N_INST[2], N_INST[9], N_INST[13]]   # CPR = 128, CPR = 4, NV = 1 with 8 waves


def n_tile_cases():
    out = []
    for kind, dt in DTS:
        for inst in N_TILE_INST:
            G, W = inst[1], inst[2]
            CPR, T = W * (64 // G), TILE[dt]
            for N, regime in ((T - 1, "one-ragged-tile"), (T, "one-whole-tile"), (T + 1, "tile+one-column-tile"),
                              (2 * T + 8 * CPR + 3, "two-tiles+prologue-remainder-tile")):
                out.append(n_case(kind, dt, inst, G + 1, N, f"N{N}-{regime}", cols=regime, rows="second-workgroup-one-live"))
    return out


def n_row_cases():
    out = []
    for kind, dt in DTS:
        for inst in N_INST:
            G, W = inst[1], inst[2]
            for Mc, regime in ((1, "one-chunk"), (G - 1, "last-lane-clamped"), (G, "one-full-workgroup"),
                               (G + 1, "second-workgroup-one-live"), (2 * G + 1, "three-workgroups")):
                out.append(n_case(kind, dt, inst, Mc, 8 * W * (64 // G) + 1, f"Mc{Mc}-{regime}", rows=regime, cols="prologue+remainder"))
    return out


def n_auto_cases():
    """either side of every switch of dispatch_n: G by the workgroup count, the waves by the row-block count"""
    out = []
    for kind, dt in DTS:
        V = VEC[dt]
        for Mc, G, W in ((2048, 8, 16), (2049, 8, 8), (255 * 16, 8, 8), (255 * 16 + 1, 16, 16), (255 * 32, 16, 8), (255 * 32 + 1, 32, 16),
                         (255 * 64, 32, 8), (255 * 64 + 1, 64, 16), (256 * 64, 64, 16), (256 * 64 + 1, 64, 8), (512 * 64, 64, 8),
                         (512 * 64 + 1, 64, 4)):
            out.append(case("n", f"gemv_n-{kind}-auto-Mc{Mc}-G{G}-W{W}", dt, Mc * V, 9, V, NV="V", G=G, WAVES=W))
        out.append(case("n", f"gemv_n-{kind}-x-offset-stays-on-the-vector-path", dt, 2049 * V, 3, V, x_lead=1, NV="V", G=8, WAVES=8))
    return out


T_CASES = t_row_cases() + t_way_cases() + t_col_cases() + t_auto_cases()
N_CASES = n_col_cases() + n_tile_cases() + n_row_cases() + n_auto_cases()


# ---- data: one pool of numbers per kind and element type, every A a view of it --------------------------------------------------------
_pool = {}


def draw(kind, dt, n, seed):
    """n integers in [-7, 7] (kind 'int') or standard Gaussian numbers (kind 'gauss') of type dt"""
    if kind == "gauss":
        return vector(dt, n, seed)
    rng = np.random.default_rng(seed)
    v = rng.integers(-7, 8, n).astype(np.float64)
    if is_cplx(dt):
        v = v + 1j * rng.integers(-7, 8, n)
    return v.astype(dt)


def matrix(kind, dt, M, N):
    key = (kind, np.dtype(dt))
    if key not in _pool:
        v = draw(kind, dt, POOL[np.dtype(dt)], 20261)
        v.setflags(write=False)
        _pool[key] = v
    assert M * N <= POOL[np.dtype(dt)], (M, N)
    return _pool[key][: M * N].reshape((M, N), order="F")


def op_of(A, op):
    return A if op == OP_N else A.T if op == OP_T else A.conj().T


def abs1(v):
    """|Re| + |Im|"""
    return np.abs(v.real).astype(np.float64) + np.abs(v.imag).astype(np.float64)


def operands(kind, dt, op, M, N):
    """(op(A), x, y0) of a case"""
    opA = op_of(matrix(kind, dt, M, N), op)
    return opA, draw(kind, dt, opA.shape[1], 11 + 3 * M + N), draw(kind, dt, opA.shape[0], 12 + M + 5 * N)


def reference(dt, opA, x, y0, al, be):
    """(alpha op(A) x + beta y0 in float64 / complex128, the factor the bound multiplies: |alpha| |op(A)| |x| + |beta| |y0|)"""
    H = LD[np.dtype(dt)]
    cast = (lambda s: H(s)) if is_cplx(dt) else (lambda s: H(s.real))
    ref = cast(al) * (opA.astype(H) @ x.astype(H))
    mag = abs(al) * (np.abs(opA).astype(np.float64) @ np.abs(x).astype(np.float64))
    if be != 0:
        ref, mag = ref + cast(be) * y0.astype(H), mag + abs(be) * np.abs(y0)
    return ref, mag


def integers_are_exact(opA, x, y0, al, be):
    """the precondition of the integer criterion: every partial sum of every output entry stays below 2^24"""
    top = (abs(al.real) + abs(al.imag)) * (abs1(opA) @ abs1(x)) + (abs(be.real) + abs(be.imag)) * abs1(y0)
    return bool(np.all(top < 2.0 ** 24))


# ---- the device side ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def _tune_restored(ctx):
    yield
    ctx.tune(**TUNE_DEFAULT)


@pytest.fixture(scope="module", autouse=True)
def _exact_report():
    yield
    print(f"\ninteger data: {EXACT['launches']} launches, every one equal to the integer reference")


class Operand:
    """A on the device: lda = M + pad, NaN in the padding rows; with a_lead, that many (NaN) elements in front of it"""

    def __init__(self, rls, ctx, A, pad, a_lead=0):
        M, N = A.shape
        self.lda = M + pad
        if a_lead == 0:
            self.keep = upload_padded(rls, ctx, A, pad)
            self.ptr = self.keep.ptr
        else:
            host = np.full(a_lead + self.lda * N, np.nan, dtype=A.dtype)
            host[a_lead:].reshape((self.lda, N), order="F")[:M, :] = A
            self.keep = rls.DeviceVector.from_host(host, ctx)
            self.ptr = self.keep.ptr + a_lead * A.dtype.itemsize
        assert (self.ptr - a_lead * A.dtype.itemsize) % 16 == 0


def code_of(rls, ctx, dt):
    return rls.DeviceVector(1, dt, ctx).code


def gemv(ctx, code, op, M, N, al, A_ptr, lda, x_ptr, be, y_ptr):
    return ctx.lib.rls_gemv(ctx.handle, code, op, M, N, al.real, al.imag, A_ptr, lda, x_ptr, be.real, be.imag, y_ptr)


def check_products(rls, ctx, group, label, dt, M, N, pad, ops, a_lead=0, x_lead=0, betas=(False, True)):
    """every op of `ops` on both kinds of data and with both betas; returns the outputs' bytes, in order"""
    dt = np.dtype(dt)
    code, out = code_of(rls, ctx, dt), []
    for kind in ("int", "gauss"):
        Ad = Operand(rls, ctx, matrix(kind, dt, M, N), pad, a_lead)
        for op in ops:
            opA, x, y0 = operands(kind, dt, op, M, N)
            xd = Guarded(rls, ctx, dt, x.size, body=x, lead=x_lead, fill=np.nan)
            assert xd.ptr % 16 == (x_lead * dt.itemsize) % 16
            for beta_zero in betas:
                al, be = scalars(dt, beta_zero)
                ref, mag = reference(dt, opA, x, y0, al, be)
                if kind == "int":
                    assert integers_are_exact(opA, x, y0, al, be), label
                yd = Guarded(rls, ctx, dt, y0.size, body=np.full(y0.size, np.nan, dtype=dt) if beta_zero else y0, lead=Y_LEAD)
                assert gemv(ctx, code, op, M, N, al, Ad.ptr, Ad.lda, xd.ptr, be, yd.ptr) == 0, ctx.lib.rls_last_error_string(ctx.handle)
                got = yd.read()
                what = f"{label} op {OP_NAME[op]} beta={be} {kind}"
                assert not np.isnan(got).any(), what
                if kind == "int":
                    bad = np.nonzero(got != ref.astype(dt))[0]
                    assert bad.size == 0, f"{what}: {bad.size} entries differ from the integer reference, first {bad[0]}: {got[bad[0]]} != {ref[bad[0]]}"
                    EXACT["launches"] += 1
                else:
                    held(group, what, np.abs(got.astype(LD[dt]) - ref), bound_factor(dt, x.size) * mag)
                out.append(got.tobytes())
            xd.read()
    return out


def group_of(c, p):
    if c.kernel == "t":
        return "gemv_t NV = V" if p.NV > 1 else "gemv_t NV = 1"
    return f"gemv_n G = {p.G}" if p.NV > 1 else "gemv_n NV = 1"


def run_case(rls, ctx, c, ops, **kw):
    p = plan_of(c)
    ctx.tune(**c.tune)
    return check_products(rls, ctx, group_of(c, p), f"{c.name} {c.M}x{c.N} lda={c.M + c.pad}", c.dt, c.M, c.N, c.pad, ops,
                          a_lead=c.a_lead, x_lead=c.x_lead, **kw)


@pytest.mark.parametrize("c", params(T_CASES))
def test_gemv_t(rls, ctx, c):
    run_case(rls, ctx, c, (OP_T, OP_C))


@pytest.mark.parametrize("c", params(N_CASES))
def test_gemv_n(rls, ctx, c):
    run_case(rls, ctx, c, (OP_N,))


REVERSE_CASES = [case("t", f"gemv_t-{kind}-NV{nv}-COLS{COLS}-reverse", dt, layout(dt, 2049, nv)[0], 2 * COLS + 1, layout(dt, 2049, nv)[1],
                      tune=dict(gemvt_cols=COLS), NV=nv, COLS=COLS, rows="full+one-chunk-tail", cols="three-workgroups")
                 for kind, dt in DTS for nv in NVS for COLS in T_COLS]


@pytest.mark.parametrize("c", params(REVERSE_CASES))
def test_gemv_t_reverse_changes_no_bit(rls, ctx, c):
    """gemvt_reverse = 0 and 1: the first workgroups take the first or the last columns; beta != 0"""
    runs = []
    for reverse in (0, 1):
        ctx.tune(gemvt_reverse=reverse)
        runs.append(run_case(rls, ctx, c, (OP_T, OP_C), betas=(False,)))
    assert runs[0] == runs[1]


# ---- around the kernels -------------------------------------------------------------------------------------------------------------------
def cmul_bound(dt):
    """one multiplication: a rounding (real), sqrt 2 gamma_2 (complex; Higham (3.13))"""
    return math.sqrt(2.0) * g(2) if is_cplx(dt) else U24


@pytest.mark.parametrize("kind,dt", DTS, ids=[k for k, _ in DTS])
def test_empty_contraction(rls, ctx, kind, dt):
    """M = 0 under T / C and N = 0 under N: y = beta y0; beta = 0 writes exact zeros over NaN.  An output of length 0: a no-op."""
    code, n = code_of(rls, ctx, dt), 37
    Ad = Operand(rls, ctx, matrix("gauss", dt, 5, 5), 3)        # (never read; the pointer must not be null)
    xd = Guarded(rls, ctx, dt, 0, fill=np.nan)
    for data in ("int", "gauss"):
        y0 = draw(data, dt, n, 77)
        for op, M, N in ((OP_T, 0, n), (OP_C, 0, n), (OP_N, n, 0)):
            lda = max(M, 1) + 3
            for beta_zero in (False, True):
                al, be = scalars(dt, beta_zero)
                yd = Guarded(rls, ctx, dt, n, body=np.full(n, np.nan, dtype=dt) if beta_zero else y0, lead=Y_LEAD)
                assert gemv(ctx, code, op, M, N, al, Ad.ptr, lda, xd.ptr, be, yd.ptr) == 0
                got = yd.read()
                what = f"{kind} op {OP_NAME[op]} {M}x{N} beta={be} {data}"
                if beta_zero:
                    assert got.tobytes() == np.zeros(n, dtype=dt).tobytes(), what
                    continue
                ref = (be if is_cplx(dt) else be.real) * y0.astype(LD[np.dtype(dt)])
                if data == "int":
                    assert np.array_equal(got, ref.astype(dt)), what
                    EXACT["launches"] += 1
                else:
                    held("empty", what, np.abs(got.astype(LD[np.dtype(dt)]) - ref), cmul_bound(dt) * abs(be) * np.abs(y0))
    for op, M, N in ((OP_N, 0, 5), (OP_T, 5, 0), (OP_C, 5, 0), (OP_N, 0, 0), (OP_T, 0, 0)):
        al, be = scalars(dt)
        yd = Guarded(rls, ctx, dt, 0, lead=Y_LEAD)
        assert gemv(ctx, code, op, M, N, al, Ad.ptr, 8, xd.ptr, be, yd.ptr) == 0
        yd.read()
    xd.read()


@pytest.mark.parametrize("kind,dt", DTS, ids=[k for k, _ in DTS])
def test_bad_arguments_are_errors_and_write_nothing(rls, ctx, kind, dt):
    code, M, N = code_of(rls, ctx, dt), 8, 5
    Ad = Operand(rls, ctx, matrix("int", dt, M, N), 4)
    al, be = scalars(dt)
    for op in (OP_N, OP_T, OP_C):
        nout, nin = (M, N) if op == OP_N else (N, M)
        y0 = draw("int", dt, nout, 5)
        xd = Guarded(rls, ctx, dt, nin, body=draw("int", dt, nin, 6), fill=np.nan)
        yd = Guarded(rls, ctx, dt, nout, body=y0, lead=Y_LEAD)
        assert gemv(ctx, code, op, M, N, al, Ad.ptr, M - 1, xd.ptr, be, yd.ptr) != 0            # lda < M
        assert gemv(ctx, code, op, 0, N, al, Ad.ptr, 0, xd.ptr, be, yd.ptr) != 0                # lda < 1 at M = 0
        assert gemv(ctx, code, op, M, N, al, None, Ad.lda, xd.ptr, be, yd.ptr) != 0
        assert gemv(ctx, code, op, M, N, al, Ad.ptr, Ad.lda, None, be, yd.ptr) != 0
        assert gemv(ctx, code, op, M, N, al, Ad.ptr, Ad.lda, xd.ptr, be, None) != 0
        for bad_op in (-1, 3):
            assert gemv(ctx, code, bad_op, M, N, al, Ad.ptr, Ad.lda, xd.ptr, be, yd.ptr) != 0
        assert yd.read().tobytes() == y0.tobytes()
        xd.read()


def device_flag(rls, ctx, value):
    return rls.DeviceVector.from_host(np.array([value], dtype=np.int32).view(np.float32), ctx)


SKIP_SHAPES = [("vector-path", lambda V: (130 * V, 33 * V)), ("NV1", lambda V: (130 * V + 1, 33 * V + 1))]


@pytest.mark.parametrize("kind,dt", DTS, ids=[k for k, _ in DTS])
@pytest.mark.parametrize("path,shape", SKIP_SHAPES, ids=[s[0] for s in SKIP_SHAPES])
@pytest.mark.parametrize("gram", [False, True], ids=["A", "gram-only"])
def test_skip_flag(rls, ctx, kind, dt, path, shape, gram):
    """rls_operator_mul_normal_skip on the two-product path (fused_normal = 0) and on a Gram-only operator (one square N-product):
    flag 1 leaves v as it was, flag 0 gives the bits of the same rls_gemv calls.  Those are held to the bound on the way."""
    dt = np.dtype(dt)
    lib, h, code, H = ctx.lib, ctx.handle, code_of(rls, ctx, dt), LD[dt]
    M, N = shape(VEC[dt])
    if gram:
        M = N
    lda = M + (VEC[dt] if path == "vector-path" else pad_for(dt, M, True))
    assert n_plan(dt, M, N, lda).NV == (VEC[dt] if path == "vector-path" else 1)
    A, p = matrix("gauss", dt, M, N), draw("gauss", dt, N, 31)
    Ad = Operand(rls, ctx, A, lda - M)
    pd = Guarded(rls, ctx, dt, N, body=p, fill=np.nan)
    one, zero = 1 + 0j, 0j
    # the plain calls: t = A p, and v = A^H t on the device's own t
    td = Guarded(rls, ctx, dt, M, fill=np.nan)
    assert gemv(ctx, code, OP_N, M, N, one, Ad.ptr, lda, pd.ptr, zero, td.ptr) == 0
    t = td.read().copy()
    held("skip", f"{kind} {path} {'gram' if gram else 'A'} {M}x{N} t = A p", np.abs(t.astype(H) - A.astype(H) @ p.astype(H)),
         bound_factor(dt, N) * (np.abs(A).astype(np.float64) @ np.abs(p)))
    if gram:
        want = t
    else:
        wd = Guarded(rls, ctx, dt, N, fill=np.nan)
        assert gemv(ctx, code, OP_C, M, N, one, Ad.ptr, lda, td.ptr, zero, wd.ptr) == 0
        want = wd.read().copy()
        held("skip", f"{kind} {path} A {M}x{N} v = A^H t", np.abs(want.astype(H) - A.conj().T.astype(H) @ t.astype(H)),
             bound_factor(dt, M) * (np.abs(A.T).astype(np.float64) @ np.abs(t)))
    op = C.c_void_p()
    try:
        ctx.tune(fused_normal=0)
        if gram:
            assert lib.rls_operator_create(h, code, 0, N, None, 0, C.byref(op)) == 0
            assert lib.rls_operator_set_gram(op, Ad.ptr, lda) == 0
        else:
            assert lib.rls_operator_create(h, code, M, N, Ad.ptr, lda, C.byref(op)) == 0
        v0 = draw("gauss", dt, N, 32)
        for flag, expect in ((1, v0), (0, want)):
            vd = Guarded(rls, ctx, dt, N, body=v0, lead=Y_LEAD)
            fd = device_flag(rls, ctx, flag)
            assert lib.rls_operator_mul_normal_skip(op, pd.ptr, vd.ptr, fd.ptr) == 0
            assert vd.read().tobytes() == expect.tobytes(), flag
        if not gram:   # the unflagged calls give the same bits as rls_gemv
            yd, xd = Guarded(rls, ctx, dt, M, fill=np.nan), Guarded(rls, ctx, dt, N, fill=np.nan)
            assert lib.rls_operator_mul(op, pd.ptr, yd.ptr) == 0
            assert yd.read().tobytes() == t.tobytes()
            assert lib.rls_operator_mul_adj(op, td.ptr, xd.ptr) == 0
            assert xd.read().tobytes() == want.tobytes()
        vd = Guarded(rls, ctx, dt, N, fill=np.nan)
        assert lib.rls_operator_mul_normal(op, pd.ptr, vd.ptr) == 0
        assert vd.read().tobytes() == want.tobytes()
        pd.read()
    finally:
        ctx.tune(fused_normal=1)
        if op:
            assert lib.rls_operator_destroy(op) == 0


RUN_TO_RUN = [c for c in T_CASES if c.claims.get("rows") == "full+one-chunk-tail" and c.claims.get("COLS") == 8 and c.N == 9][:4] + \
             [c for c in N_CASES if c.claims.get("cols") == "two-tiles+prologue-remainder-tile" and c.claims["G"] == 8]


@pytest.mark.parametrize("c", params(RUN_TO_RUN))
def test_same_bits_run_to_run(rls, ctx, c):
    ops = (OP_T, OP_C) if c.kernel == "t" else (OP_N,)
    assert run_case(rls, ctx, c, ops) == run_case(rls, ctx, c, ops)
