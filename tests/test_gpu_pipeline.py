"""The single-column streaming slab pipeline of csrc/normal.hip (rls_cgnr_path / rls_fista_path 1 and 2 and the plain
normal_operator().mul_), product by product, on every layout and at every clamp of the loads.

Layouts.  kCfgs (normal.hip) lists (G, K, WV); slab_cfg gives S = 64 / G column slots per wave, CPR = WV * S columns per round
and NMAX = K * CPR; elem<E>::vec is V = 4 (Float32) / 2 (ComplexF32) rows per 16-byte row chunk, so a row block is G * V rows.
pick_cfg takes the first entry with N <= NMAX (and, with the switch slab_g set, G == slab_g) whose LDS image fits 160 KiB:
  (G, K, WV)   S   CPR   NMAX   takes N       rows per block f32 / c64   exchange planes f32 / c64 (slab_planes)
  (8,  8, 8)   8    64    512   1 .. 512        32 / 16                  4 / 4   (DPP-paired: lanes g, g ^ 1 share a plane)
  (8, 16, 8)   8    64   1024   513 .. 1024     32 / 16                  4 / 4
  (8, 32, 8)   8    64   2048   1025 .. 2048    32 / 16                  4 / 4
  (4, 32, 8)  16   128   4096   2049 .. 4096    16 /  8                  4 / 2   (f32: the plain G-plane form; c64: paired)
  slab_g = 4: (4, 32, 8) takes every N <= 4096;  slab_g = 8: N > 2048 is refused.
`LAYOUTS` and `pick` below restate that table; test_layout_table_matches_source reads kCfgs from the source the library was
built from, so a drift shows.  The slab refuses (fused_ok) M % V != 0, lda % V != 0 and N above the table: rls_cgnr_path reports 0
there (the two-GEMV path), which the refused cases assert.  The instantiation of a launch follows from its shape: FULL where
N == NMAX and the row blocks cover M exactly (slab_full), the walking (MULTI) form where a K = 32 layout has more row blocks than
the device has compute units, the hinted forms as pipe_cur_hint says.  slab_g is set before any operator of a case is created
and stays until the case is over: the operator's workspace is sized by it.

The Gram pipeline (path 2: cgnr_gram_kernel, fista_gram_kernel and their finish kernels) always runs G = 4, WV = 8 and picks
K = 8, 16, 32 for N <= 1024, 2048, 4096 (gram_pick); FULL at N = 1024, 2048, 4096.  rls_gram_pipe_ok refuses N % V != 0, so the
nearest ragged sizes are NMAX - V and the previous NMAX + V; N = NMAX - 1 is a refused shape (path 0), asserted as such.

What is read.  Every step call of path 1 is K_A (which applies the PREVIOUS update in its prologue, then one pass over A) + K_R
per iteration and one finish kernel (cgnr_pipe_f_kernel / fista_pipe_f_kernel) that applies the last update and brings r, p
back into the caller's vectors; path 2 is one launch per iteration and cgnr_gram_f_kernel / fista_gram_f_kernel.  So the
plan's vectors are read through the Python state after a step call, i.e. behind the finish kernel:
  after init_      r = p = A^H b, x = v = 0, z0 = residual = |r|
  after a step     v = A^H (A p0) (Gram mode: v = AHA p0) of the DEVICE's own p0, and x, r, p, alpha, beta, zeta, residual as an
                   elementwise function of the device's own p0, r0, v, lambda (src/CGNR.jl:153-176), rebuilt in float64 with
                   alpha and beta applied as Float32 scalars
A single-step call takes the update through the finish kernel, the second iteration of a two-step call through K_A's
prologue: both must give the same bits (split steps), as must the hint modes 0 / 1 / 2 of pipe_hint_mode, use_graph = 0 (which
makes the first launch of a call a hinted one: pipe_cur_hint) and slab_order 0 / 1.  red_threads (256, 512, 1024: multiples of
the 64-lane wave up to the 16 waves slab_group_combine has room for, the values tools/pipe_variants.py sweeps) changes the
order of the reduce kernels' sums: each value is held to float64, not to the others' bits.

Bounds (relative l2), the project's own: one product 2e-6 (test_gemv_all_ops), two chained products 3e-6
(test_normal_operator_one_pass_vs_two_pass), both through conftest.parity_check with NumPy's product in the working precision
as the Float32 yardstick; rebuilt vectors 4 x 2e-7 (test_blas1), alpha / beta / zeta / residual 1e-6 (test_gpu_skinny.py);
iterates of FISTA through parity_check against the float64 oracle from init on.  alpha and beta are compared as float64
numbers; where they multiply a vector they are Float32 scalars, and x and r are rebuilt with the Float32 value of the DEVICE's
alpha: a float64 alpha rebuilt here can round to the neighbouring Float32, and where CG converges fast (M << N) r - alpha v
cancels and shows that one unit several times over (32 x 4096 Float32, step 2: 2.6e-8 with the device's alpha, 1.4e-6 with
this file's; the log prints both).  As in test_gpu_small.py the new r of a step is also allowed 2 x the error of the same update
done by NumPy in the working precision; no case needs it (profiles/pipeline_edges.txt lists every case with its measured
error).  The structured cases use an A of
small integers that encode (row, column): A^H A p is exact in Float32 in any summation order, and is compared with array_equal.

The plain operator's partial-row workspace belongs to the operator and is not reachable through the binding, so the NaN fill
of the plain-operator cases covers v (every element must be overwritten) and the padding rows of A (none may be read)."""
import contextlib
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import rls_oracle as O
from conftest import parity_check

pytestmark = pytest.mark.gpu

TOL_ONE, TOL_TWO = 2e-6, 3e-6            # one product, two chained products
TOL_ELEM, TOL_SCALAR = 4 * 2e-7, 1e-6    # rebuilt vectors, alpha / beta / zeta / residual
F32, C64 = np.float32, np.complex64
DTYPES = [F32, C64]
LAYOUTS = [(8, 8, 8), (8, 16, 8), (8, 32, 8), (4, 32, 8)]   # kCfgs (csrc/normal.hip), in its order
LDS_LIMIT = 160 * 1024
DEFAULTS = dict(resident=1, slab_g=0, slab_order=1, red_threads=1024, slab_multi=1, pipe_hint_mode=0, fused_normal=1, use_graph=1)


def cplx(dt):
    return np.dtype(dt).kind == "c"


def hi(dt):
    return np.complex128 if cplx(dt) else np.float64


def dname(dt):
    return np.dtype(dt).name


def vec(dt):
    """elem<E>::vec: elements of a 16-byte row chunk"""
    return 16 // np.dtype(dt).itemsize


def cpr(l):
    return l[2] * (64 // l[0])


def nmax(l):
    return l[1] * cpr(l)


def prev_nmax(l):
    i = LAYOUTS.index(l)
    return nmax(LAYOUTS[i - 1]) if i else 0


def rows(dt, l):
    """rows of a row block"""
    return l[0] * vec(dt)


def pick(dt, N, g=0):
    """pick_cfg: the first layout that holds N columns (None: refused)"""
    size = np.dtype(dt).itemsize
    for l in LAYOUTS:
        if g and l[0] != g:
            continue
        planes = 4 if l[0] == 8 else (2 if cplx(dt) and l[0] == 4 else l[0])
        lds = (planes * (nmax(l) + 64 // size) + nmax(l)) * size + 4096
        if N <= nmax(l) and lds <= LDS_LIMIT:
            return l
    return None


def slab_takes(dt, M, N, lda=None, g=0):
    """fused_ok, for an aligned allocation"""
    return M % vec(dt) == 0 and (lda or M) % vec(dt) == 0 and pick(dt, N, g) is not None


def pairing(G, nwg):
    """slab_pairing: 0 none, 1 every block, n the first n blocks"""
    return 0 if G != 4 else (1 if nwg % 16 == 0 else (nwg // 16) * 16)


def gram_k(N):
    """gram_pick: K of the Gram pipeline (G = 4, WV = 8: 128 columns per round)"""
    return next((k for k in (8, 16, 32) if N <= k * 128), None)


def rel(a, b, scale=None):
    d = np.linalg.norm(np.asarray(a).astype(np.complex128) - np.asarray(b).astype(np.complex128))
    n = np.linalg.norm(np.asarray(b).astype(np.complex128)) if scale is None else float(scale)
    return float(d / n) if n > 0 else float(d)


@contextlib.contextmanager
def tuned(ctx, **kw):
    """the context's switches set for one case, every one of this file's back at its default afterwards.  Device objects of a
    case are created inside (slab_g sizes an operator's workspace)."""
    try:
        ctx.tune(**kw)
        yield
    finally:
        ctx.tune(**DEFAULTS)


def gauss(rng, shape, dt):
    v = rng.standard_normal(shape)
    if cplx(dt):
        v = (v + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)
    return np.asfortranarray(v.astype(dt))


@functools.lru_cache(maxsize=24)
def problem(M, N, dtn):
    """Gaussian A, b, p with A^H b and A^H (A p) in float64 and in the working precision: computed once per shape, shared, never
    written to"""
    dt = np.dtype(dtn)
    rng = np.random.default_rng(1000003 * M + 1009 * N + (7 if cplx(dt) else 0))
    A, b, p = gauss(rng, (M, N), dt), gauss(rng, M, dt), gauss(rng, N, dt)
    A64 = A.astype(hi(dt))
    out = dict(A=A, b=b, p=p, A64=A64, r64=A64.conj().T @ b.astype(hi(dt)), r32=A.conj().T @ b,
               v64=A64.conj().T @ (A64 @ p.astype(hi(dt))), v32=A.conj().T @ (A @ p))
    for a in out.values():
        a.setflags(write=False)
    return out


def upload(rls, ctx, A, lda=None):
    """A on the device; with `lda` the rows M .. lda - 1 of every column hold NaN (nothing may use them)"""
    M, N = A.shape
    if lda is None or lda == M:
        return rls.DeviceMatrix.from_host(A, ctx)
    Ad = rls.DeviceMatrix(M, N, A.dtype, ctx, lda=lda)
    host = np.full((lda, N), np.nan, dtype=A.dtype, order="F")
    host[:M, :] = A
    assert ctx.lib.rls_memcpy_h2d(ctx.handle, Ad.ptr, host.ctypes.data, host.nbytes) == 0
    return Ad


def cgnr_path(ctx, S):
    out = C.c_int32(-1)
    assert ctx.lib.rls_cgnr_path(S.state._plan, C.byref(out)) == 0
    return out.value


def fista_path(ctx, S):
    out = C.c_int32(-1)
    assert ctx.lib.rls_fista_path(S.state._plan, C.byref(out)) == 0
    return out.value


def new_cgnr(rls, Ad, lam, iters=12, gram=None):
    return rls.createLinearSolver(rls.CGNR, Ad, AHA=gram, reg=rls.L2Regularization(lam), iterations=iters, relTol=0.0)


def slab_path(rls, ctx, Ad):
    """1 where the register slab takes this matrix (the operator has a partial-row workspace), 0 where it refuses: the path of a
    CGNR plan on it, resident = 0 (rls_normal_fused_workspace decides both)"""
    S = new_cgnr(rls, Ad, 0.0)
    S._prepare(S.state, rls.DeviceVector(Ad.M, Ad.dtype, ctx))
    return cgnr_path(ctx, S)


def apply_normal(rls, ctx, Ad, p):
    """v = A^H (A p) through normal_operator().mul_, twice into NaN-filled vectors: the result, which must be the same bits"""
    op = Ad.normal_operator()
    pd = rls.DeviceVector.from_host(p, ctx)
    out = []
    for _ in range(2):
        v = rls.DeviceVector(Ad.N, Ad.dtype, ctx).fill_(np.nan)
        op.mul_(v, pd)
        out.append(v.to_host())
    assert np.array_equal(out[0], out[1], equal_nan=True), "the same call repeated: other bits"
    return out[0]


def test_layout_table_matches_source(rls):
    src = os.path.join(os.path.dirname(os.path.abspath(rls.__file__)), "csrc", "normal.hip")
    with open(src) as f:
        text = f.read()
    m = re.search(r"kCfgs\[\]\s*=\s*\{(.*?)\};", text)
    assert m, "kCfgs not found in normal.hip"
    assert [tuple(int(x) for x in t) for t in re.findall(r"\{(\d+),\s*(\d+),\s*(\d+)\}", m.group(1))] == LAYOUTS
    assert [nmax(l) for l in LAYOUTS] == [512, 1024, 2048, 4096] and [cpr(l) for l in LAYOUTS] == [64, 64, 64, 128]
    for dt in DTYPES:
        for l in LAYOUTS:
            assert pick(dt, nmax(l)) == l and pick(dt, prev_nmax(l) + 1) == l and pick(dt, nmax(l), 4) == LAYOUTS[3]
        assert pick(dt, 4097) is None and pick(dt, 2049, 8) is None and pick(dt, 2048, 8) == LAYOUTS[2] and pick(dt, 1, 4) == LAYOUTS[3]
    assert [pairing(4, n) for n in (5, 16, 19, 32, 35)] == [0, 1, 16, 1, 32] and pairing(8, 16) == 0
    assert [gram_k(n) for n in (1, 1024, 1025, 2048, 2049, 4096, 4097)] == [8, 8, 16, 16, 32, 32, None]


# ---- 1. the plain normal operator on every layout -------------------------------------------------------------------------------
def operator_cases(dt):
    """(layout, kind, M, N, lda, slab_g): the smallest shape of every branch of slab_load / slab_finish on every layout"""
    v, out = vec(dt), []
    for l in LAYOUTS:
        rb, nm, pv = rows(dt, l), nmax(l), prev_nmax(l)
        out += [(l, "full-1-block", rb, nm, None, 0), (l, "full-2-blocks", 2 * rb, nm, None, 0),
                (l, "nmax-ragged-last-block", 2 * rb - v, nm, 2 * rb, 0),          # FULL's N, one dead row chunk; NaN padding rows
                (l, "nmax-minus-1", rb, nm - 1, None, 0),                          # the last round's `last` clamp
                (l, "one-row-chunk", v, pv + 5, 2 * v, 0),                         # M = V: G - 1 dead chunks; NaN padding rows
                (l, "tall-last-half-dead", 3 * rb + rb // 2, pv + (nm - pv) // 2 + 1, 3 * rb + rb // 2 + v, 0)]
        if pv:   # all rounds but one slot of the second dead (on the first layout this is N = 1 below)
            out.append((l, "prev-nmax-plus-1", rb + v, pv + 1, None, 0))
    # N < CPR (`last0`, rounds past N re-reading round 0): the first layout, and (4, 32, 8) -- CPR = 128 -- through slab_g = 4
    # ((8, 16, 8) and (8, 32, 8) start at N = 513 and 1025: above their CPR = 64)
    for l, g in ((LAYOUTS[0], 0), (LAYOUTS[3], 4)):
        for N in (1, 3, cpr(l) - 1):
            out.append((l, f"n-below-cpr-{N}", 2 * rows(dt, l) - v, N, 2 * rows(dt, l), g))
    out += [(LAYOUTS[3], "slab_g4-two-rounds", 3 * rows(dt, LAYOUTS[3]) - v, 130, None, 4),
            (LAYOUTS[3], "slab_g4-mid", rows(dt, LAYOUTS[3]), 1500, None, 4),
            (LAYOUTS[2], "slab_g8", rows(dt, LAYOUTS[2]) + v, 1500, None, 8)]
    for l, kind, M, N, lda, g in out:
        assert pick(dt, N, g) == l and slab_takes(dt, M, N, lda, g), (dname(dt), l, kind, M, N)
        assert kind.startswith("full") == (N == nmax(l) and M % rows(dt, l) == 0)   # slab_full
    return [(dt,) + c for c in out]


OP_CASES = [c for dt in DTYPES for c in operator_cases(dt)]
OP_IDS = [f"{dname(c[0])}-G{c[1][0]}K{c[1][1]}-{c[2]}-{c[3]}x{c[4]}" for c in OP_CASES]


@pytest.mark.parametrize("dt,l,kind,M,N,lda,g", OP_CASES, ids=OP_IDS)
def test_normal_operator_on_every_layout(rls, ctx, dt, l, kind, M, N, lda, g):
    pb = problem(M, N, dname(dt))
    with tuned(ctx, resident=0, slab_g=g):
        Ad = upload(rls, ctx, pb["A"], lda)
        assert slab_path(rls, ctx, Ad) == 1, "the register slab must take this shape"
        got = apply_normal(rls, ctx, Ad, pb["p"])
    assert np.isfinite(got).all(), "NaN: an element of v not written, or the padding of A used"
    e = parity_check(f"pipeline_op_{kind}_{M}x{N}_{dname(dt)}", got, pb["v64"], pb["v32"], tol=TOL_TWO)
    print(f"[pipeline] op G{l[0]}K{l[1]} {kind} {M}x{N} lda{lda or M} {dname(dt)}: device {e:.3e}  numpy-f32 {rel(pb['v32'], pb['v64']):.3e}")


REFUSED = [(F32, 34, 40, None, 0, "M % V"), (C64, 17, 40, None, 0, "M % V"), (F32, 32, 40, 34, 0, "lda % V"), (C64, 16, 40, 17, 0, "lda % V"),
           (F32, 32, 4097, None, 0, "N above the table"), (C64, 16, 4097, None, 0, "N above the table"),
           (F32, 32, 2049, None, 8, "slab_g = 8 and N > 2048"), (C64, 16, 2049, None, 8, "slab_g = 8 and N > 2048")]


@pytest.mark.parametrize("dt,M,N,lda,g,why", REFUSED, ids=[f"{dname(c[0])}-{c[1]}x{c[2]}-lda{c[3] or c[1]}-g{c[4]}" for c in REFUSED])
def test_refused_shapes_report_path_0(rls, ctx, dt, M, N, lda, g, why):
    """a shape the slab refuses: path 0, and the product (two GEMVs) is still right"""
    assert not slab_takes(dt, M, N, lda, g), why
    pb = problem(M, N, dname(dt))
    with tuned(ctx, resident=0, slab_g=g):
        Ad = upload(rls, ctx, pb["A"], lda)
        assert slab_path(rls, ctx, Ad) == 0, why
        got = apply_normal(rls, ctx, Ad, pb["p"])
    parity_check(f"pipeline_refused_{M}x{N}_{dname(dt)}", got, pb["v64"], pb["v32"], tol=TOL_TWO)


# ---- 2. pairing of the G = 4 row blocks -------------------------------------------------------------------------------------------
PAIR_CASES = [(dt, nwg, N, g, ragged) for dt in DTYPES for nwg in (5, 16, 19) for N, g in ((2049, 0), (40, 4)) for ragged in (0, 1)]


@pytest.mark.parametrize("dt,nwg,N,g,ragged", PAIR_CASES, ids=[f"{dname(c[0])}-nwg{c[1]}-N{c[2]}-{'ragged' if c[4] else 'even'}" for c in PAIR_CASES])
def test_pairing_regimes(rls, ctx, dt, nwg, N, g, ragged):
    """slab_pairing: no pairing (5 row blocks), every block (16), the first 16 of 19; `ragged`: the last block loses a row chunk.
    Against float64 and against the two-GEMV path: a row block used twice or skipped shows in both."""
    l = LAYOUTS[3]
    M = nwg * rows(dt, l) - (vec(dt) if ragged else 0)
    assert pick(dt, N, g) == l and -(-M // rows(dt, l)) == nwg and pairing(4, nwg) == {5: 0, 16: 1, 19: 16}[nwg]
    pb = problem(M, N, dname(dt))
    with tuned(ctx, resident=0, slab_g=g):
        Ad = upload(rls, ctx, pb["A"])
        assert slab_path(rls, ctx, Ad) == 1
        one = apply_normal(rls, ctx, Ad, pb["p"])
        ctx.tune(fused_normal=0)
        two = apply_normal(rls, ctx, Ad, pb["p"])
    tag = f"pipeline_pair_nwg{nwg}_{M}x{N}_{dname(dt)}"
    e1 = parity_check(tag, one, pb["v64"], pb["v32"], tol=TOL_TWO)
    e2 = parity_check(tag + "_two_gemv", two, pb["v64"], pb["v32"], tol=TOL_TWO, record=False)
    e12 = rel(one, two)
    print(f"[pipeline] pair nwg{nwg} {M}x{N} {dname(dt)}: one-pass {e1:.3e}  two-GEMV {e2:.3e}  one against the other {e12:.3e}")
    assert e12 <= TOL_TWO, (tag, e12)


# ---- 3. CGNR on the pipeline, product by product ----------------------------------------------------------------------------------
def snap(ctx, S):
    """the plan's vectors and scalars as they stand in memory behind the finish kernel of the last call"""
    st = S.state
    s = st._refresh(ctx.lib)
    return dict(x=st.x.to_host(), r=st.x0.to_host(), p=st.pl.to_host(), v=st.vl.to_host(), it=s.iteration, done=s.done,
                alpha=complex(s.alpha_re, s.alpha_im), beta=complex(s.beta_re, s.beta_im), zeta=s.zeta, residual=s.residual, z0=s.z0)


def same_bits(a, b, what):
    for k in "xrpv":
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k, float(np.nanmax(np.abs(a[k] - b[k]))))


def finite(tag, s):
    for k in "xrpv":
        assert np.isfinite(s[k]).all(), (tag, k, "not finite: the padding of A was used, or a product broke down")


def check_init(tag, pb, s0):
    """r = p = A^H b, x = v = 0, the scalars of init!"""
    finite(tag, s0)
    e = parity_check(f"pipeline_{tag}_AhB", s0["r"], pb["r64"], pb["r32"], tol=TOL_ONE)
    print(f"[pipeline] {tag}_AhB: device {e:.3e}  numpy-f32 {rel(pb['r32'], pb['r64']):.3e}")
    assert np.array_equal(s0["r"], s0["p"]), tag
    assert not s0["x"].any() and not s0["v"].any(), tag
    z0 = float(np.linalg.norm(s0["r"].astype(hi(s0["r"].dtype))))
    assert s0["it"] == 0 and s0["done"] == 0, (tag, s0["it"], s0["done"])
    assert abs(s0["z0"] - z0) <= TOL_SCALAR * z0 and abs(s0["residual"] - z0) <= TOL_SCALAR * z0, (tag, s0["z0"], s0["residual"], z0)
    assert s0["alpha"] == 0 and s0["beta"] == 0 and s0["zeta"] == 0, tag


def check_step(tag, pb, prev, cur, lam, it, max_iter, G=None):
    """one iteration: v against the float64 product of the device's own p (two products of A, or one of the Gram matrix `G`), then
    src/CGNR.jl:153-176 in float64 on the device's own p, r, v"""
    finite(tag, cur)
    dt = prev["p"].dtype
    h = hi(dt)
    p0 = prev["p"].astype(h)
    if G is None:
        v64, v32, tol, name = pb["A64"].conj().T @ (pb["A64"] @ p0), pb["A"].conj().T @ (pb["A"] @ prev["p"]), TOL_TWO, "AhAP"
    else:
        v64, v32, tol, name = np.matmul(G, p0), G @ prev["p"], TOL_ONE, "GP"
    ev, e32 = parity_check(f"pipeline_{tag}_{name}{it}", cur["v"], v64, v32, tol=tol), rel(v32, v64)
    lam32 = float(np.float32(lam))
    x, r, v = prev["x"].astype(h), prev["r"].astype(h), cur["v"].astype(h)
    zeta = float(np.sum(np.abs(r) ** 2))
    den = np.vdot(p0, v) + (lam32 * float(np.sum(np.abs(p0) ** 2)) if lam32 > 0 else 0.0)
    alpha = zeta / den
    # alpha is applied as a working-precision scalar: the device's own (its float64 value is held to `alpha` below), since the
    # rounding of a float64 alpha of this file's may land on the neighbouring Float32, and r1 = r - alpha v amplifies that one
    # unit by |r| / |r1| where CG converges fast (M << N: 32 x 4096, step 2: 1.4e-6 of |r1| with this file's alpha, `own` in the log)
    a32 = np.dtype(dt).type(cur["alpha"] if cplx(dt) else cur["alpha"].real)
    a = h(a32)
    x1 = x + a * p0
    r1 = r - a * v - ((a * lam32) * p0 if lam32 > 0 else 0.0)
    ex, er = rel(cur["x"], x1), rel(cur["r"], r1)
    a_own = h(np.dtype(dt).type(alpha))
    er_own = rel(cur["r"], r - a_own * v - ((a_own * lam32) * p0 if lam32 > 0 else 0.0))
    # the Float32 yardstick of r: the same update in NumPy's working precision from the same p0, r0, v (no fused multiply-add)
    l32 = np.float32(lam32)
    r_np = prev["r"] - a32 * cur["v"]
    if lam32 > 0:
        r_np = r_np - (l32 * prev["p"]) * a32
    er32 = rel(r_np, r1)
    rr = float(np.sum(np.abs(cur["r"].astype(h)) ** 2))   # beta, the residual and p follow the device's own new r
    beta = rr / zeta
    p1 = float(np.float32(beta)) * p0 + cur["r"].astype(h)
    ep = rel(cur["p"], p1)
    ea = abs(cur["alpha"] - alpha) / abs(alpha)
    eb = abs(cur["beta"].real - beta) / beta if beta > 0 else abs(cur["beta"].real)
    ez = abs(cur["zeta"] - zeta) / zeta
    es = abs(cur["residual"] - np.sqrt(rr)) / np.sqrt(rr) if rr > 0 else abs(cur["residual"])
    print(f"[pipeline] {tag}_step{it}: {name} device {ev:.3e}  numpy-f32 {e32:.3e}  x {ex:.3e}  r {er:.3e}  (numpy-f32 {er32:.3e}, own {er_own:.3e})  "
          f"p {ep:.3e}  scalars {max(ea, eb, ez, es):.3e}")
    assert ex <= TOL_ELEM and ep <= TOL_ELEM, (tag, it, ex, ep)
    assert er <= max(TOL_ELEM, 2 * er32), (tag, it, "r", er, "NumPy Float32", er32)
    assert max(ea, eb, ez, es) <= TOL_SCALAR, (tag, it, ea, eb, ez, es)
    assert cur["beta"].imag == 0.0 and (cplx(dt) or cur["alpha"].imag == 0.0), tag
    assert cur["it"] == it and cur["done"] == int(it >= max_iter) and cur["z0"] == prev["z0"], (tag, cur["it"], cur["done"])


def start_cgnr(rls, ctx, tag, pb, Ad, lam, path, Gd=None):
    S = new_cgnr(rls, Ad, lam, gram=Gd)
    rls.init_(S, rls.DeviceVector.from_host(pb["b"], ctx))
    assert cgnr_path(ctx, S) == path, (tag, "path", cgnr_path(ctx, S), "wanted", path)
    return S


def run_cgnr(rls, ctx, tag, pb, Ad, lam, path=1, Gd=None, G=None, calls=(1, 1), check=True):
    """init! and one step call per entry of `calls` (iterations per call) on `path`; with `check` every product and every update of
    the single-iteration calls is held to float64.  Returns the snapshots after init and after every call."""
    S = start_cgnr(rls, ctx, tag, pb, Ad, lam, path, Gd)
    snaps = [snap(ctx, S)]
    if check:
        check_init(tag, pb, snaps[0])
    it = 0
    for n in calls:
        S.state._step_status(ctx.lib, n)
        it += n
        cur = snap(ctx, S)
        assert cur["it"] == it, (tag, cur["it"], it)
        if check and n == 1:
            check_step(tag, pb, snaps[-1], cur, lam, it, min(12, pb["A"].shape[1]), G)
        snaps.append(cur)
    return snaps


def pipe_shapes(dt):
    """(layout, kind, M, N, slab_g, lambda) of the CGNR / FISTA pipeline cases: every layout at a FULL shape of two row blocks
    (workgroup 1 is not the one that stores x, r, p) and at a both-ragged one, the finish kernels' edges N = 1024 | 1025 (1 | 2
    elements per thread) and 2048 | 2049 (2 | 4), and (4, 32, 8) at a small N through slab_g = 4 (ComplexF32: ALWAYS_HINTED)"""
    v, out = vec(dt), []
    for i, l in enumerate(LAYOUTS):
        out += [(l, "full", 2 * rows(dt, l), nmax(l), 0, 0.0), (l, "ragged", 3 * rows(dt, l) - v, nmax(l) - 3, 0, 1e-2)]
    for N in (1024, 1025, 2048, 2049):
        l = pick(dt, N)
        out.append((l, f"ept-edge-{N}", rows(dt, l) + v, N, 0, 1e-2 if N % 2 else 0.0))
    out.append((LAYOUTS[3], "slab_g4-small", 2 * rows(dt, LAYOUTS[3]) + v, 40, 4, 1e-2))
    for l, kind, M, N, g, lam in out:
        assert pick(dt, N, g) == l and slab_takes(dt, M, N, None, g)
    return [(dt,) + c for c in out]


PIPE_CASES = [c for dt in DTYPES for c in pipe_shapes(dt)]
PIPE_IDS = [f"{dname(c[0])}-G{c[1][0]}K{c[1][1]}-{c[2]}-{c[3]}x{c[4]}" for c in PIPE_CASES]


@pytest.mark.parametrize("dt,l,kind,M,N,g,lam", PIPE_CASES, ids=PIPE_IDS)
def test_cgnr_pipeline_products_and_updates(rls, ctx, dt, l, kind, M, N, g, lam):
    pb = problem(M, N, dname(dt))
    with tuned(ctx, resident=0, slab_g=g):
        run_cgnr(rls, ctx, f"cgnr_G{l[0]}K{l[1]}_{kind}_{M}x{N}_{dname(dt)}_lam{lam}", pb, upload(rls, ctx, pb["A"]), lam)


VARIANTS = [("two-step call", dict(), (2,)), ("hint withheld", dict(pipe_hint_mode=1), (2,)), ("hint wrong", dict(pipe_hint_mode=2), (2,)),
            ("hint wrong, single steps", dict(pipe_hint_mode=2), (1, 1)), ("no graph: first launch hinted", dict(use_graph=0), (1, 1)),
            ("no graph, two-step call", dict(use_graph=0), (2,)), ("slab_order 0", dict(slab_order=0), (1, 1))]


@pytest.mark.parametrize("dt,l,kind,M,N,g,lam", PIPE_CASES, ids=PIPE_IDS)
def test_cgnr_pipeline_variants_give_the_same_bits(rls, ctx, dt, l, kind, M, N, g, lam):
    """1 + 1 steps == one two-step call, whatever the (r, p) pair hint says (known, withheld, wrong), with and without graph
    capture and in both orders of the small loads: x, r, p, v bit for bit"""
    pb = problem(M, N, dname(dt))
    tag = f"cgnr_variants_{M}x{N}_{dname(dt)}"
    with tuned(ctx, resident=0, slab_g=g):
        Ad = upload(rls, ctx, pb["A"])
        want = run_cgnr(rls, ctx, tag, pb, Ad, lam, check=False)[-1]
        for name, switches, calls in VARIANTS:
            ctx.tune(**switches)
            got = run_cgnr(rls, ctx, tag, pb, Ad, lam, calls=calls, check=False)[-1]
            ctx.tune(**{k: DEFAULTS[k] for k in switches})
            same_bits(want, got, (tag, name))
            assert got["it"] == want["it"] == 2


RED_CASES = [c for c in PIPE_CASES if c[2] in ("ragged", "slab_g4-small")]


@pytest.mark.parametrize("threads", [256, 512])
@pytest.mark.parametrize("dt,l,kind,M,N,g,lam", RED_CASES, ids=[i for c, i in zip(PIPE_CASES, PIPE_IDS) if c in RED_CASES])
def test_cgnr_pipeline_reduce_widths(rls, ctx, dt, l, kind, M, N, g, lam, threads):
    """red_threads: 16 or 32 row groups per column in cgnr_pipe_r_kernel instead of 64 (the default runs above)"""
    pb = problem(M, N, dname(dt))
    with tuned(ctx, resident=0, slab_g=g, red_threads=threads):
        run_cgnr(rls, ctx, f"cgnr_red{threads}_{kind}_{M}x{N}_{dname(dt)}", pb, upload(rls, ctx, pb["A"]), lam)
        got = apply_normal(rls, ctx, upload(rls, ctx, pb["A"]), pb["p"])   # slab_reduce_kernel at the same width
    parity_check(f"pipeline_op_red{threads}_{M}x{N}_{dname(dt)}", got, pb["v64"], pb["v32"], tol=TOL_TWO)


@pytest.mark.parametrize("threads", [256, 512, 1024])
@pytest.mark.parametrize("nwg", [17, 65, 70, 130])
@pytest.mark.parametrize("dt", DTYPES, ids=dname)
def test_more_partial_rows_than_row_groups(rls, ctx, dt, nwg, threads):
    """slab_column_sum: a thread of the reduce kernels sums the partial rows wy, wy + ny, ... (ny = red_threads / 16 row groups) in
    batches of four loads whose last batch is clamped and masked: one row more than ny, than 4 ny, and counts in between, on 40
    columns ((8, 8, 8) for even counts, (4, 32, 8) through slab_g = 4 for odd ones); the last row block loses a row chunk"""
    g = 4 if nwg % 2 else 0
    l = pick(dt, 40, g)
    M = nwg * rows(dt, l) - vec(dt)
    pb = problem(M, 40, dname(dt))
    with tuned(ctx, resident=0, slab_g=g, red_threads=threads):
        Ad = upload(rls, ctx, pb["A"])
        got = apply_normal(rls, ctx, Ad, pb["p"])
        run_cgnr(rls, ctx, f"cgnr_rows{nwg}_red{threads}_{M}x40_{dname(dt)}", pb, Ad, 0.0, calls=(1,))
    parity_check(f"pipeline_op_rows{nwg}_red{threads}_{dname(dt)}", got, pb["v64"], pb["v32"], tol=TOL_TWO)


# ---- 4. FISTA on the pipeline -------------------------------------------------------------------------------------------------------
FISTA_STEPS = 3


def fista_regs(R, kind, lam):
    return {"l1": R.L1Regularization(lam), "none": None}[kind]


@functools.lru_cache(maxsize=8)
def fista_problem(M, N, dtn):
    dt = np.dtype(dtn)
    A, _, b = O.make_problem(M, N, dt, 67)
    A64, b64 = A.astype(hi(dt)), b.astype(hi(dt))
    rho = 0.9 / np.linalg.norm(A64, 2) ** 2
    lam = 2e-2 * float(np.max(np.abs(A64.conj().T @ b64)))
    for a in (A, b, A64, b64):
        a.setflags(write=False)
    return dict(A=A, b=b, A64=A64, b64=b64, rho=rho, lam=lam)


@functools.lru_cache(maxsize=16)
def fista_oracle(M, N, dtn, kind, restart, normal):
    """the float64 oracle and the Float32 one after init and after every iteration: (x, xold, res, rel_res_norm) per precision"""
    fp = fista_problem(M, N, dtn)
    out = []
    for A, b in ((fp["A64"], fp["b64"]), (fp["A"], fp["b"])):
        ref = O.FISTA(A, reg=fista_regs(O, kind, fp["lam"]), rho=fp["rho"], iterations=FISTA_STEPS, relTol=0.0, restart=restart, normal=normal)
        ref.init(b)
        states = [(ref.x.copy(), ref.xold.copy(), ref.res.copy(), float(ref.rel_res_norm))]
        while ref.iterate() is not None:
            states.append((ref.x.copy(), ref.xold.copy(), ref.res.copy(), float(ref.rel_res_norm)))
        out.append((states, float(np.linalg.norm(ref.x0)), ref.x0.copy()))
    return out


def fista_state(ctx, S):
    st = S.state
    st._refresh(ctx.lib)
    return dict(x=st.x.to_host(), xold=st.xold.to_host(), res=st.res.to_host(), x0=st.x0.to_host(), rel=st.rel_res_norm, it=st.iteration)


FISTA_VARIANTS = [("one call", dict(), True), ("hint wrong", dict(pipe_hint_mode=2), False), ("hint wrong, one call", dict(pipe_hint_mode=2), True),
                  ("no graph: first launch hinted", dict(use_graph=0), False), ("hint withheld, one call", dict(pipe_hint_mode=1), True)]


def run_fista(rls, ctx, tag, M, N, dt, kind, restart, Ad, path, Gd=None, variants=FISTA_VARIANTS):
    """init! and 3 one-iteration calls held to the oracles from init on (with graph capture on, the first launch of a call does not
    know the parity of the iteration count: the unhinted instantiation).  Then the same solve under `variants` -- as ONE 3-iteration
    call (launches 2 and 3 are hinted), with the parity known, wrong (the kernel re-loads) and withheld: the same bits."""
    fp = fista_problem(M, N, dname(dt))
    (ref, nx0, x0_64), (ref32, _, x0_32) = fista_oracle(M, N, dname(dt), kind, restart, "gram" if Gd is not None else "matrixfree")
    make = lambda: rls.createLinearSolver(rls.FISTA, Ad, AHA=Gd, reg=fista_regs(rls, kind, fp["lam"]), rho=fp["rho"], iterations=FISTA_STEPS,
                                          relTol=0.0, restart=restart)
    bd = rls.DeviceVector.from_host(fp["b"], ctx)
    S = make()
    rls.init_(S, bd)
    assert fista_path(ctx, S) == path, (tag, "path", fista_path(ctx, S), "wanted", path)
    got = fista_state(ctx, S)
    # after init!: x = xold = 0, x0 = A^H b, res = Inf and an infinite residual norm (src/FISTA.jl:110-129), as the oracle
    assert got["it"] == 0 and np.isinf(ref[0][3]) and got["rel"] == ref[0][3], (tag, got["it"], got["rel"])
    assert not got["x"].any() and not got["xold"].any(), tag
    assert np.array_equal(got["res"], ref[0][2].astype(dt)), (tag, "res after init!")
    parity_check(f"pipeline_{tag}_x0", got["x0"], x0_64, x0_32, tol=TOL_ONE, record=False)
    for it in range(1, FISTA_STEPS + 1):
        assert rls.iterate(S) is not None
        got = fista_state(ctx, S)
        assert got["it"] == it and all(np.isfinite(got[k]).all() for k in ("x", "xold", "res")), (tag, it)
        ex = parity_check(f"pipeline_{tag}_x_it{it}", got["x"], ref[it][0], ref32[it][0], record=it == FISTA_STEPS)
        parity_check(f"pipeline_{tag}_xold_it{it}", got["xold"], ref[it][1], ref32[it][1], record=False)
        er = parity_check(f"pipeline_{tag}_res_it{it}", got["res"], ref[it][2], ref32[it][2], scale=nx0, record=False)
        assert abs(got["rel"] - ref[it][3]) < 1e-4 * ref[it][3] + 2e-6, (tag, it, got["rel"], ref[it][3])
        print(f"[pipeline] {tag}_it{it}: x device {ex:.3e}  f32-oracle {rel(ref32[it][0], ref[it][0]):.3e}  res {er:.3e}")
    assert rls.iterate(S) is None
    for name, switches, once in variants:
        ctx.tune(**switches)
        try:
            V = make()
            rls.init_(V, bd)
            assert fista_path(ctx, V) == path
            if once:
                assert ctx.lib.rls_fista_step(V.state._plan, FISTA_STEPS) == 0
            else:
                for _ in range(FISTA_STEPS):
                    assert rls.iterate(V) is not None
            other = fista_state(ctx, V)
        finally:
            ctx.tune(**{k: DEFAULTS[k] for k in switches})
        for k in ("x", "xold", "res"):
            assert np.array_equal(other[k], got[k]), (tag, name, k, rel(other[k], got[k]))
        assert other["it"] == FISTA_STEPS
    return got


FISTA_CASES = [c[:6] + (kind, restart) for c in PIPE_CASES for kind in ("l1", "none") for restart in ("none", "gradient")]


@pytest.mark.parametrize("dt,l,shape,M,N,g,kind,restart", FISTA_CASES,
                         ids=[f"{dname(c[0])}-G{c[1][0]}K{c[1][1]}-{c[2]}-{c[3]}x{c[4]}-{c[6]}-{c[7]}" for c in FISTA_CASES])
def test_fista_pipeline_against_the_oracle(rls, ctx, dt, l, shape, M, N, g, kind, restart):
    fp = fista_problem(M, N, dname(dt))
    with tuned(ctx, resident=0, slab_g=g):
        run_fista(rls, ctx, f"fista_G{l[0]}K{l[1]}_{shape}_{M}x{N}_{dname(dt)}_{kind}_{restart}", M, N, dt, kind, restart,
                  upload(rls, ctx, fp["A"]), 1)


# ---- 5. the Gram pipeline, CGNR and FISTA ---------------------------------------------------------------------------------------
def gram_sizes(dt):
    """(N, kind): per K of gram_pick the FULL size, the nearest ragged sizes the pipeline takes (N % V == 0: NMAX - V with a short
    last row block, previous NMAX + V with all rounds but one dead), and N < 128 = CPR with a row-chunk count that is no multiple of
    the 4 chunks of a row block"""
    v, out = vec(dt), [(25 * vec(dt), "below-cpr")]
    for k, prev in ((8, 0), (16, 1024), (32, 2048)):
        out += [(k * 128, "full"), (k * 128 - v, "nmax-minus-v")]
        if prev:
            out.append((prev + v, "prev-nmax-plus-v"))
    for N, kind in out:
        assert N % v == 0 and gram_k(N) is not None and (kind == "full") == (N == gram_k(N) * 128 and (N // v) % 4 == 0)
    return [(dt, N, kind) for N, kind in out]


@functools.lru_cache(maxsize=2)
def gram_matrix(N, dtn):
    """A (48 x N, Gaussian) from fista_problem and AHA built on the host in float64, rounded ONCE to the working precision: the
    device's product is measured against the float64 product of exactly the matrix it was given"""
    fp = fista_problem(48, N, dtn)
    G = np.asfortranarray((fp["A64"].conj().T @ fp["A64"]).astype(np.dtype(dtn)))
    G.setflags(write=False)
    return G


GRAM_CASES = [c for dt in DTYPES for c in gram_sizes(dt)]


@pytest.mark.parametrize("dt,N,kind", GRAM_CASES, ids=[f"{dname(c[0])}-K{gram_k(c[1])}-{c[2]}-N{c[1]}" for c in GRAM_CASES])
def test_gram_pipeline_cgnr_and_fista(rls, ctx, dt, N, kind):
    """path 2: v = AHA p0 of the device's own p0 (one product) and the rebuilt update over two single steps, the split-step and
    hint variants bit for bit, then FISTA (L1, gradient restart where N is even in units of V) against the oracle from init on"""
    M = 48
    fp, G = fista_problem(M, N, dname(dt)), gram_matrix(N, dname(dt))
    pb = dict(A=fp["A"], b=fp["b"], r64=fp["A64"].conj().T @ fp["b64"], r32=fp["A"].conj().T @ fp["b"])
    tag = f"gram_K{gram_k(N)}_{kind}_N{N}_{dname(dt)}"
    nwg = -(-(N // vec(dt)) // 4)
    with tuned(ctx, resident=0):
        Ad, Gd = upload(rls, ctx, fp["A"]), rls.DeviceMatrix.from_host(G, ctx)
        lam = 1e-2 * float(np.real(G[0, 0]))
        want = run_cgnr(rls, ctx, f"cgnr_{tag}_pair{pairing(4, nwg)}", pb, Ad, lam, path=2, Gd=Gd, G=G)[-1]
        for name, switches, calls in (("two-step call", dict(), (2,)), ("no graph", dict(use_graph=0), (1, 1)), ("slab_order 0", dict(slab_order=0), (2,))):
            ctx.tune(**switches)
            got = run_cgnr(rls, ctx, tag, pb, Ad, lam, path=2, Gd=Gd, calls=calls, check=False)[-1]
            ctx.tune(**{k: DEFAULTS[k] for k in switches})
            same_bits(want, got, (tag, name))
        run_fista(rls, ctx, f"fista_{tag}", M, N, dt, "l1", "gradient" if (N // vec(dt)) % 2 == 0 else "none", Ad, 2, Gd=Gd)
        if cplx(dt) and kind == "full" and gram_k(N) == 32:
            # 512 row blocks of AHA: the launches above walk them; one workgroup per block is the FULL form that does not walk
            ctx.tune(slab_multi=0)
            run_cgnr(rls, ctx, f"cgnr_{tag}_slab_multi0", pb, Ad, lam, path=2, Gd=Gd, G=G)
            run_fista(rls, ctx, f"fista_{tag}_slab_multi0", M, N, dt, "l1", "none", Ad, 2, Gd=Gd, variants=FISTA_VARIANTS[:1])


@pytest.mark.parametrize("dt", DTYPES, ids=dname)
def test_gram_pipeline_refuses_odd_n(rls, ctx, dt):
    """N = NMAX - 1 is no multiple of V: rls_gram_pipe_ok refuses it (path 0, one GEMV over AHA per iteration), and the steps are
    still right"""
    M, N = 48, 1023
    fp, G = fista_problem(M, N, dname(dt)), gram_matrix(N, dname(dt))
    pb = dict(A=fp["A"], b=fp["b"], r64=fp["A64"].conj().T @ fp["b64"], r32=fp["A"].conj().T @ fp["b"])
    with tuned(ctx, resident=0):
        run_cgnr(rls, ctx, f"gram_refused_N{N}_{dname(dt)}", pb, upload(rls, ctx, fp["A"]), 0.0, path=0, Gd=rls.DeviceMatrix.from_host(G, ctx), G=G)


# ---- 6. the walking form at its smallest shapes -----------------------------------------------------------------------------------
def compute_units():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


WALK_CASES = [(dt, l, N, g) for dt in DTYPES for l, N, g in ((LAYOUTS[2], 1025, 0), (LAYOUTS[3], 130, 4), (LAYOUTS[2], 2048, 0), (LAYOUTS[3], 4096, 0))]


@pytest.mark.parametrize("dt,l,N,g", WALK_CASES, ids=[f"{dname(c[0])}-G{c[1][0]}K{c[1][1]}-N{c[2]}" for c in WALK_CASES])
def test_walking_form_smallest_shapes(rls, ctx, dt, l, N, g):
    """one row block more than the device has compute units, the last one half dead: workgroup 0 walks two blocks
    (normal_slab_multi_kernel, cgnr_pipe_a_kernel and fista_pipe_a_kernel <..., MULTI>); against float64 and against the same launch
    as one workgroup per block (slab_multi = 0) within the bound of two products.  N: the narrowest of (8, 32, 8); (4, 32, 8) at
    two rounds of columns through slab_g = 4; and N = NMAX with every row block whole, the only shapes of the FULL walking forms."""
    cus = compute_units()
    M = (cus + 1) * rows(dt, l) if N == nmax(l) else cus * rows(dt, l) + rows(dt, l) // 2
    assert pick(dt, N, g) == l and l[1] == 32 and -(-M // rows(dt, l)) == cus + 1
    pb = problem(M, N, dname(dt))
    tag = f"walk_G{l[0]}K{l[1]}_{M}x{N}_{dname(dt)}"
    out = {}
    with tuned(ctx, resident=0, slab_g=g):
        Ad = upload(rls, ctx, pb["A"])
        assert slab_path(rls, ctx, Ad) == 1
        for multi in (1, 0):
            ctx.tune(slab_multi=multi)
            v = apply_normal(rls, ctx, Ad, pb["p"])
            parity_check(f"pipeline_{tag}_op_multi{multi}", v, pb["v64"], pb["v32"], tol=TOL_TWO)
            cg = run_cgnr(rls, ctx, f"{tag}_multi{multi}", pb, Ad, 1e-2)[-1]
            # as ONE two-step call: the second launch knows its (r, p) pair (the hinted walking form): the same bits
            same_bits(cg, run_cgnr(rls, ctx, tag, pb, Ad, 1e-2, calls=(2,), check=False)[-1], (tag, multi, "two-step call"))
            S = rls.createLinearSolver(rls.FISTA, Ad, reg=rls.L1Regularization(0.05 * float(np.max(np.abs(pb["r32"])))),
                                       rho=0.9 / (np.sqrt(M) + np.sqrt(N)) ** 2, iterations=FISTA_STEPS, relTol=0.0)
            rls.init_(S, rls.DeviceVector.from_host(pb["b"], ctx))
            assert fista_path(ctx, S) == 1
            assert ctx.lib.rls_fista_step(S.state._plan, FISTA_STEPS) == 0
            out[multi] = dict(v=v, cg=cg, fx=fista_state(ctx, S))
    e = dict(op=rel(out[1]["v"], out[0]["v"]), fista=rel(out[1]["fx"]["x"], out[0]["fx"]["x"]), **{k: rel(out[1]["cg"][k], out[0]["cg"][k]) for k in "xrpv"})
    print(f"[pipeline] {tag}: walking against one workgroup per block: " + "  ".join(f"{k} {x:.3e}" for k, x in e.items()))
    assert np.isfinite(out[1]["fx"]["x"]).all() and out[1]["fx"]["x"].any() and max(e.values()) <= TOL_TWO, (tag, e)


def test_walking_form_gram_complex(rls, ctx):
    """cgnr_gram_kernel / fista_gram_kernel <float2, 4, 32, 8, false, ., MULTI>: ComplexF32 with one 8-row block of AHA more than the
    device has compute units (the last block: one live row chunk)"""
    dt, cus, M = C64, compute_units(), 48
    N = 2 * (4 * cus + 1)
    if gram_k(N) != 32:
        pytest.fail(f"{cus} compute units: {N} columns are not on the K = 32 Gram layout, the walking form has no smallest shape here")
    fp, G = fista_problem(M, N, dname(dt)), gram_matrix(N, dname(dt))
    pb = dict(A=fp["A"], b=fp["b"], r64=fp["A64"].conj().T @ fp["b64"], r32=fp["A"].conj().T @ fp["b"])
    tag = f"walk_gram_N{N}_{dname(dt)}"
    out = {}
    with tuned(ctx, resident=0):
        Ad, Gd = upload(rls, ctx, fp["A"]), rls.DeviceMatrix.from_host(G, ctx)
        for multi in (1, 0):
            ctx.tune(slab_multi=multi)
            cg = run_cgnr(rls, ctx, f"{tag}_multi{multi}", pb, Ad, 1e-2 * float(np.real(G[0, 0])), path=2, Gd=Gd, G=G)[-1]
            fx = run_fista(rls, ctx, f"fista_{tag}_multi{multi}", M, N, dt, "l1", "none", Ad, 2, Gd=Gd, variants=FISTA_VARIANTS[:1])
            out[multi] = dict(cg=cg, fx=fx)
    e = dict(fista=rel(out[1]["fx"]["x"], out[0]["fx"]["x"]), **{k: rel(out[1]["cg"][k], out[0]["cg"][k]) for k in "xrpv"})
    print(f"[pipeline] {tag}: walking against one workgroup per block: " + "  ".join(f"{k} {x:.3e}" for k, x in e.items()))
    assert max(e.values()) <= TOL_ONE, (tag, e)


# ---- 7. structured data: exact in Float32 -------------------------------------------------------------------------------------------
def indexed_matrix(M, N, dt):
    """entries in -3 .. 3 that encode (row, column): every partial sum of A p and of A^H (A p), p of zeros and ones, is an integer
    below 2^24 for the shapes here (|t| <= 2 * 3 N, |v| <= M * 2 * 3 * 6 N < 2^24 for M <= 112 at N = 4096), so Float32
    arithmetic is exact in any order and a swapped slot, row chunk or plane changes the result"""
    i, j = np.arange(M, dtype=np.int64)[:, None], np.arange(N, dtype=np.int64)[None, :]
    re = (3 * i + 5 * j + (i // 4) * (j % 11)) % 7 - 3
    if not cplx(dt):
        return re, np.asfortranarray(re.astype(dt))
    z = re + 1j * ((5 * i + 2 * j + (i % 3) * (j // 8)) % 7 - 3)
    return z, np.asfortranarray(z.astype(dt))


def exact_cases(dt):
    v, out = vec(dt), []
    for l in LAYOUTS:
        out += [(l, 2 * rows(dt, l), nmax(l), 0), (l, 3 * rows(dt, l) - v, nmax(l) - 1, 0)]
    out += [(LAYOUTS[3], 19 * rows(dt, LAYOUTS[3]) - v, 130, 4), (LAYOUTS[0], 2 * rows(dt, LAYOUTS[0]) - v, 3, 0)]
    for l, M, N, g in out:
        assert pick(dt, N, g) == l and M * 36 * N < 2 ** 24
    return [(dt,) + c for c in out]


EXACT_CASES = [c for dt in DTYPES for c in exact_cases(dt)]


@pytest.mark.parametrize("dt,l,M,N,g", EXACT_CASES, ids=[f"{dname(c[0])}-G{c[1][0]}K{c[1][1]}-{c[2]}x{c[3]}" for c in EXACT_CASES])
def test_indexed_matrix_is_exact(rls, ctx, dt, l, M, N, g):
    Z, A = indexed_matrix(M, N, dt)
    with tuned(ctx, resident=0, slab_g=g):
        Ad = upload(rls, ctx, A, M + vec(dt))
        assert slab_path(rls, ctx, Ad) == 1
        for name, idx in (("ones", None), ("first", 0), ("last", N - 1), ("middle", N // 2 + 1)):
            p = np.ones(N, dtype=np.int64) if idx is None else np.eye(1, N, min(idx, N - 1), dtype=np.int64)[0]
            want = Z.conj().T @ (Z @ p)
            got = apply_normal(rls, ctx, Ad, p.astype(dt))
            assert np.array_equal(got, want.astype(dt)), (name, M, N, int(np.count_nonzero(got != want.astype(dt))), "elements differ")
