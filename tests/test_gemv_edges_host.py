"""The device-free half of tests/test_gpu_gemv_edges.py: its cases are what their ids say, every regime and instantiation of the two
GEMV kernels is named by a case, the integer data stays exact in Float32, and the rounding bound is not tighter than honest Float32
arithmetic.

The regimes are decided here from the trip counts that t_plan / n_plan restate from csrc/gemv.hip:
  gemv_t_kernel  span = 256 x 8 chunks; spans = Mc / span full trips, then a tail of Mc % span chunks in 8 slices of 256 lanes;
                 grid = ceil(N / COLS) workgroups, the last with `dup` clamped duplicate columns
  gemv_n_kernel  per x tile of nt columns: main_rounds = (nt / CPR) / 8 * 8 unpredicated rounds, the first 8 of them the prologue
                 (loaded ahead of the LDS staging), the others steady trips of 8; then rounds - main_rounds clamped remainder rounds;
                 grid = ceil(Mc / G) workgroups, the last with `live` chunks that are not clamped"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_gemv_edges as E  # noqa: E402

ALL = E.T_CASES + E.N_CASES + E.REVERSE_CASES

T_ROW = {
    "one-live-lane": lambda p: p.spans == 0 and p.tail == 1,
    "below-one-slice": lambda p: p.spans == 0 and p.tail == E.T_THREADS - 1,
    "one-slice": lambda p: p.spans == 0 and p.tail == E.T_THREADS,
    "one-slice+1": lambda p: p.spans == 0 and p.tail == E.T_THREADS + 1,
    "tail-only": lambda p: p.spans == 0 and p.tail == E.SPAN - 1,
    "full-only": lambda p: p.spans == 1 and p.tail == 0,
    "full+one-chunk-tail": lambda p: p.spans == 1 and p.tail == 1,
    "two-spans+tail": lambda p: p.spans == 2 and p.tail > E.T_THREADS,
    "full+tail": lambda p: p.spans >= 1 and p.tail >= 1,
}
T_COL = {
    "one-column": lambda p, N: N == 1 and p.grid == 1 and p.dup == p.COLS - 1,
    "short-workgroup": lambda p, N: N > 1 and p.grid == 1 and p.dup == 1,
    "exact-workgroup": lambda p, N: p.grid == 1 and p.dup == 0,
    "second-workgroup-one-live": lambda p, N: p.grid == 2 and p.dup == p.COLS - 1,
    "three-workgroups": lambda p, N: p.grid == 3 and p.dup == p.COLS - 1,
}


def one_tile(f):
    return lambda p, dt: len(p.tiles) == 1 and f(p, *p.tiles[0])


N_COL = {
    "one-column": one_tile(lambda p, nt, main, rounds: nt == 1 and main == 0 and rounds == 1 and p.CPR > 1),
    "remainder-only-short-round": one_tile(lambda p, nt, main, rounds: 1 < nt < p.CPR and main == 0 and rounds == 1),
    "remainder-only-one-full-round": one_tile(lambda p, nt, main, rounds: nt == p.CPR and main == 0 and rounds == 1),
    "remainder-only-two-rounds": one_tile(lambda p, nt, main, rounds: main == 0 and rounds == 2 and nt % p.CPR == 1),
    "remainder-only-eight-rounds": one_tile(lambda p, nt, main, rounds: main == 0 and rounds == 8 and nt % p.CPR),
    "prologue-only": one_tile(lambda p, nt, main, rounds: main == 8 and rounds == 8),
    "prologue+remainder": one_tile(lambda p, nt, main, rounds: main == 8 and rounds == 9),
    "one-steady-trip": one_tile(lambda p, nt, main, rounds: main == 16 and rounds == 16),
    "steady+remainder": one_tile(lambda p, nt, main, rounds: main == 16 and rounds == 18),
    # (CPR = 128 at TILE = 2048: 16 rounds fill the tile, a steady trip can have no remainder behind it in the same tile)
    "steady-tile-then-remainder-tile": lambda p, dt: p.tiles == [(E.TILE[dt], 16, 16), (p.CPR + 1, 0, 2)] and 16 * p.CPR == E.TILE[dt],
    "one-ragged-tile": one_tile(lambda p, nt, main, rounds: main >= 8 and rounds > main and nt % p.CPR),
    "one-whole-tile": lambda p, dt: len(p.tiles) == 1 and p.tiles[0][0] == E.TILE[dt] and p.tiles[0][1] == p.tiles[0][2] >= 16,
    "tile+one-column-tile": lambda p, dt: len(p.tiles) == 2 and p.tiles[0][0] == E.TILE[dt] and p.tiles[1] == (1, 0, 1),
    "two-tiles+prologue-remainder-tile": lambda p, dt: len(p.tiles) == 3 and p.tiles[0][0] == p.tiles[1][0] == E.TILE[dt]
    and p.tiles[2][1:] == (8, 9),
}
N_ROW = {
    "one-chunk": lambda p: p.grid == 1 and p.live == 1,
    "last-lane-clamped": lambda p: p.grid == 1 and p.live == p.G - 1,
    "one-full-workgroup": lambda p: p.grid == 1 and p.live == p.G,
    "second-workgroup-one-live": lambda p: p.grid == 2 and p.live == 1,
    "three-workgroups": lambda p: p.grid == 3 and p.live == 1,
}
ONE_TILE_COLS = ["one-column", "remainder-only-short-round", "remainder-only-one-full-round", "remainder-only-two-rounds",
                 "remainder-only-eight-rounds", "prologue-only", "prologue+remainder", "one-steady-trip"]
TILE_COLS = ["one-ragged-tile", "one-whole-tile", "tile+one-column-tile", "two-tiles+prologue-remainder-tile"]


def broken(c):
    """which of the vector path's conditions a case breaks"""
    V, item = E.VEC[c.dt], c.dt.itemsize
    out = set()
    if c.M % V:
        out.add("M%V")
    if (c.M + c.pad) % V:
        out.add("lda%V")
    if (c.a_lead * item) % 16:
        out.add("A-offset")
    if c.kernel == "t" and (c.x_lead * item) % 16:
        out.add("x-offset")
    return out


@pytest.mark.parametrize("c", E.params(ALL))
def test_case_is_what_its_id_says(c):
    p, V, k = E.plan_of(c), E.VEC[c.dt], c.claims
    assert c.pad >= 1 and c.M * c.N <= E.POOL[c.dt] and c.M * c.N * c.dt.itemsize <= 10e6
    assert p.NV == (V if k["NV"] == "V" else 1) and (p.NV == V) == (not broken(c))
    assert f"NV{k['NV']}" in c.name or "auto" in c.name or "x-offset" in c.name
    if c.kernel == "t":
        assert p.COLS == k["COLS"] and (f"COLS{p.COLS}" in c.name or "way" in k)
        assert p.Mc == c.M // p.NV and p.Mc >= 1
        if "rows" in k:
            assert T_ROW[k["rows"]](p), (k["rows"], vars(p))
            assert k["rows"] in c.name or "cols" in k or "way" in k
        if "cols" in k:
            assert T_COL[k["cols"]](p, c.N), (k["cols"], vars(p))
        if "way" in k:
            assert broken(c) == {k["way"]} and k["way"] in c.name
    else:
        assert (p.G, p.WAVES) == (k["G"], k["WAVES"]) and p.CPR == p.WAVES * 64 // p.G
        assert f"G{p.G}-W{p.WAVES}" in c.name or "x-offset" in c.name
        if "rows" in k:
            assert N_ROW[k["rows"]](p), (k["rows"], vars(p))
        if "cols" in k:
            assert N_COL[k["cols"]](p, c.dt), (k["cols"], vars(p))
            assert k["cols"] in c.name or k["rows"] in c.name


def named(cases, **want):
    return [c for c in cases if all(c.claims.get(k) == v for k, v in want.items())]


@pytest.mark.parametrize("kind,dt", E.DTS, ids=[k for k, _ in E.DTS])
def test_every_gemv_t_regime_and_instantiation_is_named(kind, dt):
    cases = [c for c in E.T_CASES if c.dt == dt]
    for nv in E.NVS:
        for COLS in E.T_COLS:   # (the GPU test runs ops T and C on every case: CONJ false and true of each COLS x NV)
            assert named(cases, NV=nv, COLS=COLS)
            cols = {"one-column", "second-workgroup-one-live", "three-workgroups"} | ({"exact-workgroup"} if COLS > 1 else set()) | \
                   ({"short-workgroup"} if COLS > 2 else set())
            for regime in cols:
                for rows in ("one-slice+1", "full+one-chunk-tail"):
                    assert named(cases, NV=nv, COLS=COLS, cols=regime, rows=rows), (nv, COLS, regime, rows)
            assert named(E.REVERSE_CASES, NV=nv, COLS=COLS, rows="full+one-chunk-tail", cols="three-workgroups")
        for COLS in (1, 8):
            for regime in T_ROW:
                if regime != "full+tail":
                    assert named(cases, NV=nv, COLS=COLS, rows=regime), (nv, COLS, regime)
    for way in ("M%V", "lda%V", "A-offset", "x-offset"):
        assert named(cases, NV="1", way=way, rows="full+tail")
    for N, COLS in ((1023, 1), (1024, 2), (2047, 2), (2048, 4), (4095, 4), (4096, 8), (4099, 8)):
        assert [c for c in cases if "auto" in c.name and c.N == N and c.claims["COLS"] == COLS and not c.tune]
    # the x offset with everything else aligned leaves op N on the vector path
    assert [c for c in E.N_CASES if c.dt == dt and c.x_lead == 1 and c.claims["NV"] == "V" and not broken(c)]


@pytest.mark.parametrize("kind,dt", E.DTS, ids=[k for k, _ in E.DTS])
def test_every_gemv_n_regime_and_instantiation_is_named(kind, dt):
    cases = [c for c in E.N_CASES if c.dt == dt and c.tune]
    insts = [("V", G, W) for G in (8, 16, 32, 64) for W in (4, 8, 16)] + [("1", 64, W) for W in (4, 8, 16)]
    assert len(insts) == 15
    for nv, G, W in insts:
        CPR = W * 64 // G
        last = "steady+remainder" if 17 * CPR + 1 <= E.TILE[dt] else "steady-tile-then-remainder-tile"
        for regime in ONE_TILE_COLS + [last]:
            assert named(cases, NV=nv, G=G, WAVES=W, cols=regime, rows="second-workgroup-one-live"), (nv, G, W, regime)
        for regime in N_ROW:
            assert named(cases, NV=nv, G=G, WAVES=W, rows=regime, cols="prologue+remainder"), (nv, G, W, regime)
    for nv, G, W in (("V", 8, 16), ("V", 64, 4), ("1", 64, 8)):   # CPR = 128, CPR = 4, and an element-granular one
        for regime in TILE_COLS:
            assert named(cases, NV=nv, G=G, WAVES=W, cols=regime), (nv, G, W, regime)
    # each way into NV = 1 on its own
    for way in ("M%V", "lda%V", "A-offset"):
        assert [c for c in cases if c.claims["NV"] == "1" and broken(c) == {way}], way
    auto = {(c.claims["G"], c.claims["WAVES"]): c for c in E.N_CASES if c.dt == dt and not c.tune}
    assert {g for g, _ in auto} == {8, 16, 32, 64} and {w for _, w in auto} == {4, 8, 16}
    V = E.VEC[dt]
    for Mc in (2048, 255 * 16, 255 * 32, 255 * 64, 256 * 64, 512 * 64):   # the two sides of every switch choose differently
        a, b = (E.n_plan(dt, m * V, 9, m * V + V) for m in (Mc, Mc + 1))
        assert (a.G, a.WAVES) != (b.G, b.WAVES)
        assert [c for c in E.N_CASES if c.dt == dt and not c.tune and c.M == Mc * V] and \
               [c for c in E.N_CASES if c.dt == dt and not c.tune and c.M == (Mc + 1) * V]


def ops_of(c):
    return (E.OP_T, E.OP_C) if c.kernel == "t" else (E.OP_N,)


def test_integer_data_is_exact_in_float32():
    """the precondition each GPU case asserts again before its launch, here for all of them; beta != 0 is the larger side"""
    top = 0.0
    for c in ALL:
        for op in ops_of(c):
            opA, x, y0 = E.operands("int", c.dt, op, c.M, c.N)
            al, be = E.scalars(c.dt)
            assert np.abs(opA.real).max() <= 7 and np.abs(x.imag).max() <= 7 and np.all(opA == np.round(opA))
            assert E.integers_are_exact(opA, x, y0, al, be), c.name
            top = max(top, float(((abs(al.real) + abs(al.imag)) * (E.abs1(opA) @ E.abs1(x))).max()))
    print(f"largest sum of magnitudes: {top:.3e} (2^24 = {2.0 ** 24:.3e})")
    assert top < 2.0 ** 24


def plain_float32(opA, x, y0, al, be, rows):
    """alpha op(A) x + beta y0 with inputs and accumulation in float32 / complex64: the products rounded one by one and summed in
    sequence (cumsum), and the library's matrix-vector product"""
    dt = opA.dtype
    sc = (lambda s: dt.type(s)) if E.is_cplx(dt) else (lambda s: dt.type(s.real))
    sums = [np.cumsum(opA[:rows] * x[None, :], axis=1, dtype=dt)[:, -1], opA[:rows] @ x]
    outs = [sc(al) * s + (sc(be) * y0[:rows] if be != 0 else dt.type(0)) for s in sums]
    assert all(o.dtype == dt for o in outs)
    return outs


def test_plain_float32_arithmetic_stays_inside_the_bound():
    """at every contraction length of every case (the first case of each length and type, 64 output entries of it at the most)"""
    seen, worst = set(), (0.0, "")
    for c in ALL:
        for op in ops_of(c):
            n = c.N if op == E.OP_N else c.M
            if (c.dt, n) in seen:
                continue
            seen.add((c.dt, n))
            opA, x, y0 = E.operands("gauss", c.dt, op, c.M, c.N)
            rows = min(opA.shape[0], 64)
            for beta_zero in (False, True):
                al, be = E.scalars(c.dt, beta_zero)
                ref, mag = E.reference(c.dt, opA[:rows], x, y0[:rows], al, be)
                bound = E.bound_factor(c.dt, n) * mag
                for got in plain_float32(opA, x, y0, al, be, rows):
                    err = np.abs(got.astype(ref.dtype) - ref)
                    assert np.all(err <= bound), (c.name, n, float((err / bound).max()))
                    if (err / bound).max() > worst[0]:
                        worst = (float((err / bound).max()), f"{c.dt.name} n={n}")
    lengths = sorted({n for _, n in seen})
    print(f"{len(seen)} (type, length) pairs, lengths {lengths[0]} .. {lengths[-1]}; largest error / bound {worst[0]:.3e} ({worst[1]})")
    assert lengths[-1] >= 9219 and 0 < worst[0] <= 1


def test_the_bound_is_the_one_derived():
    u = 2.0 ** -24
    assert E.bound_factor(np.float32, 100) == (104 * u) / (1 - 104 * u)
    assert E.bound_factor(np.complex64, 100) == np.sqrt(2.0) * (204 * u) / (1 - 204 * u)
    assert E.scalars(np.float32) == (2, -1) and E.scalars(np.complex64) == (1 - 2j, 2j) and E.scalars(np.complex64, True)[1] == 0
