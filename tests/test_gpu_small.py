"""The single-workgroup small-system kernels of csrc/small.hip (rls_cgnr_path / rls_fista_path 8), product by product, on every
tile and on both ways of loading A.

Tiles.  small_pick takes the first tile (R, C) with M <= 32 R and N <= 16 C; `pick` below is a copy of that table and chooses
every parametrised shape, so a drift between the two shows as a path-8 refusal or a wrong expectation.  The library has no tile
query; the tile of a case follows from its shape:
  type        R   C   takes M     and N          but not (an earlier tile does)     smallest shapes here      NVE | R
  Float32     1   1   1 .. 32     1 .. 16                                           1 x 1                     -
  Float32     2   2   1 .. 64     1 .. 32        M <= 32 and N <= 16                33 x 3, 32 x 17           -
  Float32     4   2   65 .. 128   1 .. 32                                           65 x 3                    yes
  Float32     4   4   1 .. 128    33 .. 64                                          67 x 33                   yes
  Float32     8   4   129 .. 256  1 .. 64                                           129 x 3                   yes
  Float32     8   8   1 .. 256    65 .. 128                                         131 x 65                  yes
  Float32     16  4   257 .. 512  1 .. 64                                           257 x 3                   yes
  ComplexF32  1   1 / 2   2 / 4   2 / 4   4 / 8   4: the same five rows (NVE = 2: vector loads from R = 2 on)
Every tile also runs its largest shape 32 R x 16 C and one ragged in both directions, (32 R - 3) x (16 C - 3).

What is read.  A CGNR plan on path 8 owns x, r (state.x0), p (state.pl), v (state.vl) and the status scalars:
  after init_     r = p = A^H b (the kernel's init branch: small_adjoint_partials alone), x = v = 0, z0 = residual = |r|
  after a step    v = A^H (A p0) of the DEVICE's own p0, and x, r, p, alpha, beta, zeta, residual as an elementwise function of
                  the device's own p0, r0, v, lambda (src/CGNR.jl:153-176), rebuilt in float64 with alpha and beta applied as
                  Float32 scalars (al, na, bf in the kernel); beta, the residual and p from the device's own new r
Every step is a launch of its own (the status read in between ends a listening kernel), so the second step enters through the
branch that reloads x, r, p, v and the scalars from memory.

Bounds (relative l2), the project's own: one product 2e-6 (test_gemv_all_ops), two chained products 3e-6
(test_normal_operator_one_pass_vs_two_pass), both through conftest.parity_check with NumPy's product in the working precision
as the Float32 yardstick; rebuilt vectors 4 x 2e-7 (test_blas1), alpha / beta / zeta / residual 1e-6 (as test_gpu_skinny.py).
Every rebuilt vector is measured on its own norm.  Where the new r = r0 - alpha v (- alpha lambda p0) cancels to rounding noise
-- the step that ends CG in exact arithmetic: N = 1, 1 x 64 -- no Float32 update can hold 8e-7 of the result, and the bar is 2 x
the error of the same update done by NumPy in the working precision on the same p0, r0, v (the rule for a bar that has to move).
Measured on an MI355X (profiles/small_edges.txt has every case; the maxima stand at MEASURED below): apart from r in those
steps every bar sits more than 2 x above the largest device error, so none was moved, and NumPy's Float32 products on the same
inputs stay under the bars too: the fixed bars gate every product, never the 2 x yardstick.

FISTA: the largest shape of every tile runs the four regularisers with both restarts; the both-ragged shape and the padded-lda
cases run both restarts resp. one, with the regulariser rotated over the cases, not crossed with them.

small.hip:67-71 (a 16-byte piece that sticks out of the matrix is re-read element by element) runs only with a ragged M AND a
leading dimension that is a multiple of NVE: test_load_paths and test_fista_load_paths, every case whose M is not a multiple
of NVE (Float32 250, 251, 253, 501, 97, 5, 3; ComplexF32 251, 65, 33, 3) in its `aligned` upload.  The `unaligned` upload of the
same matrix (odd lda) runs the element path on the same tile; both put the same values into the same registers, so r after init
and v after a step are the same bits.  The padding rows hold NaN: nothing may read them.
"""
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
# MEASURED: largest device error per quantity over this file on an MI355X (NumPy Float32 on the same inputs, its own largest):
#   A^H b 1.3e-7 (1.9e-7)   A^H (A p) 1.0e-7 (1.5e-7)   x 5.0e-8   p 4.1e-8   scalars 5.7e-8
#   r, on its own norm: 2.6e-7 (3.3e-7) over the 262 ordinary steps; in the 10 steps that end CG the new r is noise and the
#   device stands at 1.6e-5 .. 2.4 against NumPy's 4.7e-2 .. 3.4 (closest: 1.04 against 1.00, 160 x 1 ComplexF32, lambda = 0)
#   FISTA after 7 iterations: x 9.7e-7 (the Float32 oracle 9.9e-7), res 5.8e-7, against the 1e-5 gate
F32, C64 = np.float32, np.complex64
DTYPES = [F32, C64]
REAL_TILES = [(1, 1), (2, 2), (4, 2), (4, 4), (8, 4), (8, 8), (16, 4)]   # small_pick (csrc/small.hip), in its order
CPLX_TILES = REAL_TILES[:5]
ROW_BLOCKS, COL_BLOCKS = 32, 16                                          # SM_RB, the 16 lanes of a DPP row


def cplx(dt):
    return np.dtype(dt).kind == "c"


def hi(dt):
    return np.complex128 if cplx(dt) else np.float64


def tiles(dt):
    return CPLX_TILES if cplx(dt) else REAL_TILES


def nve(dt):
    return 16 // np.dtype(dt).itemsize


def pick(dt, M, N):
    """small_pick: the first tile that holds M x N, None where the small path refuses"""
    for R, Cc in tiles(dt):
        if M <= ROW_BLOCKS * R and N <= COL_BLOCKS * Cc:
            return (R, Cc)
    return None


def tile_shapes(dt, t):
    """(kind, M, N) of one tile: its largest shape, the smallest that no earlier tile takes -- one more row than the previous tile
    holds forces the next R, one more column the next C --, and one ragged in both directions"""
    ts = tiles(dt)
    i = ts.index(t)
    R, Cc = t
    out = [("full", ROW_BLOCKS * R, COL_BLOCKS * Cc), ("ragged", ROW_BLOCKS * R - 3, COL_BLOCKS * Cc - 3)]
    if i == 0:
        out.append(("min", 1, 1))
    else:
        Rp, Cp = ts[i - 1]
        if R > Rp:
            out.append(("minrow", ROW_BLOCKS * Rp + 1, 3))
        if Cc > Cp:
            N = COL_BLOCKS * Cp + 1
            out.append(("mincol", min(2 * N + 1, ROW_BLOCKS * Rp), N))
    for kind, M, N in out:
        assert pick(dt, M, N) == t, (dt, t, kind, M, N)
        if kind == "minrow":
            assert pick(dt, M - 1, N) != t
        if kind == "mincol":
            assert pick(dt, M, N - 1) != t
    return out


def dname(dt):
    return np.dtype(dt).name


def rel(a, b, scale=None):
    d = np.linalg.norm(np.asarray(a).astype(np.complex128) - np.asarray(b).astype(np.complex128))
    n = np.linalg.norm(np.asarray(b).astype(np.complex128)) if scale is None else float(scale)
    return float(d / n) if n > 0 else float(d)


@functools.lru_cache(maxsize=None)
def problem(M, N, dtn):
    """Gaussian A and b with A^H b in float64 and in the working precision: computed once per shape, shared, never written to"""
    dt = np.dtype(dtn)
    rng = np.random.default_rng(1000003 * M + 1009 * N + (7 if cplx(dt) else 0))

    def gauss(*shape):
        v = rng.standard_normal(shape)
        if cplx(dt):
            v = (v + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)
        return np.asfortranarray(v.astype(dt))

    A, b = gauss(M, N), gauss(M)
    A64 = A.astype(hi(dt))
    out = dict(A=A, b=b, A64=A64, r64=A64.conj().T @ b.astype(hi(dt)), r32=A.conj().T @ b)
    for a in out.values():
        a.setflags(write=False)
    return out


def upload(rls, ctx, A, lda=None):
    """A on the device; with `lda` the rows M .. lda - 1 of every column hold NaN (nothing may read them)"""
    M, N = A.shape
    if lda is None:
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


def new_cgnr(rls, Ad, lam, iters, relTol=0.0):
    return rls.createLinearSolver(rls.CGNR, Ad, reg=rls.L2Regularization(lam), iterations=iters, relTol=relTol)


def snap(ctx, S):
    """the plan's vectors and scalars as they stand in memory"""
    st = S.state
    s = st._refresh(ctx.lib)
    return dict(x=st.x.to_host(), r=st.x0.to_host(), p=st.pl.to_host(), v=st.vl.to_host(), it=s.iteration, done=s.done,
                alpha=complex(s.alpha_re, s.alpha_im), beta=complex(s.beta_re, s.beta_im), zeta=s.zeta, residual=s.residual, z0=s.z0)


def same_bits(a, b, what):
    for k in "xrpv":
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k, float(np.nanmax(np.abs(a[k] - b[k]))))


def finite(tag, s):
    for k in "xrpv":
        assert np.isfinite(s[k]).all(), (tag, k, "not finite: the padding of A was read, or a product broke down")


def check_init(tag, pb, s0):
    """r = p = A^H b, x = v = 0, the scalars of init!"""
    finite(tag, s0)
    e = parity_check(f"small_{tag}_AhB", s0["r"], pb["r64"], pb["r32"], tol=TOL_ONE)
    print(f"[small] {tag}_AhB: device {e:.3e}  numpy-f32 {rel(pb['r32'], pb['r64']):.3e}")
    assert np.array_equal(s0["r"], s0["p"]), tag
    assert not s0["x"].any() and not s0["v"].any(), tag
    z0 = float(np.linalg.norm(s0["r"].astype(hi(s0["r"].dtype))))
    assert s0["it"] == 0 and s0["done"] == 0, (tag, s0["it"], s0["done"])
    assert abs(s0["z0"] - z0) <= TOL_SCALAR * z0 and abs(s0["residual"] - z0) <= TOL_SCALAR * z0, (tag, s0["z0"], s0["residual"], z0)
    z64 = float(np.linalg.norm(pb["r64"]))   # rr = |A^H b|^2 against float64: the product's bound and the reduction's
    assert abs(s0["residual"] - z64) <= (TOL_ONE + TOL_SCALAR) * z64, (tag, s0["residual"], z64)
    assert s0["alpha"] == 0 and s0["beta"] == 0 and s0["zeta"] == 0, tag


def check_step(tag, pb, prev, cur, lam, it, max_iter, rel_tol=0.0):
    """one iteration: v against the float64 product of the device's own p, then src/CGNR.jl:153-176 in float64 on the device's own
    p, r, v"""
    finite(tag, cur)
    dt = prev["p"].dtype
    h = hi(dt)
    M, N = pb["A"].shape
    p0 = prev["p"].astype(h)
    v64, v32 = pb["A64"].conj().T @ (pb["A64"] @ p0), pb["A"].conj().T @ (pb["A"] @ prev["p"])
    ev, e32 = parity_check(f"small_{tag}_AhAP{it}", cur["v"], v64, v32, tol=TOL_TWO), rel(v32, v64)
    lam32 = float(np.float32(lam))
    x, r, v = prev["x"].astype(h), prev["r"].astype(h), cur["v"].astype(h)
    zeta = float(np.sum(np.abs(r) ** 2))
    den = np.vdot(p0, v) + (lam32 * float(np.sum(np.abs(p0) ** 2)) if lam32 > 0 else 0.0)
    alpha = zeta / den
    a = h(np.dtype(dt).type(alpha))   # applied as a working-precision scalar
    x1 = x + a * p0
    r1 = r - a * v - ((a * lam32) * p0 if lam32 > 0 else 0.0)
    ex = rel(cur["x"], x1)
    er = rel(cur["r"], r1)
    # the Float32 yardstick of r: the same update in NumPy's working precision from the same p0, r0, v (no fused multiply-add)
    a32, l32 = np.dtype(dt).type(alpha), np.float32(lam32)
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
    print(f"[small] {tag}_step{it}: AhAP device {ev:.3e}  numpy-f32 {e32:.3e}  x {ex:.3e}  r {er:.3e}  (numpy-f32 {er32:.3e})  "
          f"p {ep:.3e}  scalars {max(ea, eb, ez, es):.3e}")
    assert ex <= TOL_ELEM and ep <= TOL_ELEM, (tag, it, ex, ep)
    assert er <= max(TOL_ELEM, 2 * er32), (tag, it, "r", er, "NumPy Float32", er32)
    assert max(ea, eb, ez, es) <= TOL_SCALAR, (tag, it, ea, eb, ez, es)
    assert cur["beta"].imag == 0.0 and (cplx(dt) or cur["alpha"].imag == 0.0), tag
    # done(): src/CGNR.jl:181-185 -- converged, or iteration >= min(iterations, N); the plan's count is cgnr_effective_iterations
    # (solvers.hip), of which `max_iter` here is the test's own statement
    with np.errstate(all="ignore"):
        done = bool(np.float32(np.sqrt(rr) / prev["z0"]) <= np.float32(rel_tol)) or it >= max_iter
    assert cur["it"] == it and cur["done"] == int(done) and cur["z0"] == prev["z0"], (tag, cur["it"], cur["done"], done)


def run_cgnr(rls, ctx, tag, pb, Ad, lam, steps=2, iters=12):
    """init! and `steps` one-iteration calls on path 8, every product and every update checked (a call on a plan that is done must
    change nothing); returns the snapshots"""
    S = new_cgnr(rls, Ad, lam, iters)
    rls.init_(S, rls.DeviceVector.from_host(pb["b"], ctx))
    assert cgnr_path(ctx, S) == 8, (tag, "not on the small-system path")
    snaps = [snap(ctx, S)]
    check_init(tag, pb, snaps[0])
    max_iter = min(iters, pb["A"].shape[1])
    for k in range(1, steps + 1):
        S.state._step_status(ctx.lib, 1)
        cur = snap(ctx, S)
        if snaps[-1]["done"]:
            same_bits(snaps[-1], cur, (tag, "a step on a plan that is done"))
            assert cur["it"] == snaps[-1]["it"] and cur["done"] == 1
        else:
            check_step(tag, pb, snaps[-1], cur, lam, k, max_iter)
        snaps.append(cur)
    return snaps


# ---- 1. each product on its own, on every tile ----------------------------------------------------------------------------------
TILE_CASES = [(dt, t, kind, M, N) for dt in DTYPES for t in tiles(dt) for kind, M, N in tile_shapes(dt, t)]


@pytest.mark.parametrize("lam", [0.0, 1e-2])   # lambda > 0: the pp reduction and the extra fma
@pytest.mark.parametrize("dt,t,kind,M,N", TILE_CASES, ids=[f"{dname(c[0])}-R{c[1][0]}C{c[1][1]}-{c[2]}-{c[3]}x{c[4]}" for c in TILE_CASES])
def test_products_on_every_tile(rls, ctx, dt, t, kind, M, N, lam):
    pb = problem(M, N, dname(dt))
    run_cgnr(rls, ctx, f"tile{t[0]}x{t[1]}_{kind}_{M}x{N}_{dname(dt)}_lam{lam}", pb, upload(rls, ctx, pb["A"]), lam)


# Most of the tile dead: 512 x 1 and 512 x 2 keep 63 / 62 of the 64 padded columns of tile (16, 4) zero; 1 x 64 and 3 x 128 have one
# live row block; M < N ends CG after min(M, N) steps in exact arithmetic.
ASPECT = [(F32, 512, 1, (16, 4)), (F32, 512, 2, (16, 4)), (F32, 1, 64, (4, 4)), (F32, 3, 128, (8, 8)), (F32, 5, 7, (1, 1)),
          (C64, 160, 1, (8, 4)), (C64, 1, 64, (4, 4)), (C64, 20, 40, (4, 4))]


@pytest.mark.parametrize("lam", [0.0, 1e-2])
@pytest.mark.parametrize("dt,M,N,t", ASPECT, ids=[f"{dname(c[0])}-{c[1]}x{c[2]}" for c in ASPECT])
def test_extreme_aspect_ratios(rls, ctx, dt, M, N, t, lam):
    assert pick(dt, M, N) == t
    pb = problem(M, N, dname(dt))
    run_cgnr(rls, ctx, f"aspect_{M}x{N}_{dname(dt)}_lam{lam}", pb, upload(rls, ctx, pb["A"]), lam)


def oracle_cgnr(A, b, lam, iters):
    h = hi(A.dtype)
    ref = O.CGNR(A.astype(h), reg=O.L2Regularization(lam), iterations=iters, relTol=0.0)
    O.solve(ref, b.astype(h))
    return ref, (lambda: O.solve(O.CGNR(A, reg=O.L2Regularization(lam), iterations=iters, relTol=0.0), b))


@pytest.mark.parametrize("dt,M,N", [(F32, 40, 6), (F32, 6, 9), (C64, 37, 5)])
def test_more_iterations_than_columns(rls, ctx, dt, M, N):
    """iterations > N: the plan itself stops at N (src/CGNR.jl:185), in one launch and call by call.  lambda = 1: with M < N the
    normal matrix A^H A + lambda I has the eigenvalue lambda on the null space of A against (sqrt M + sqrt N)^2 = 30 at the top,
    and the last steps of a Float32 CG act on rounding noise that the solve amplifies by that ratio: 30 x 6e-8 stays within the
    1e-5 gate, the 3000 of lambda = 1e-2 would not (nor does it for the Float32 oracle on other draws)."""
    A, _, b = O.make_problem(M, N, dt, 71)
    lam, iters = 1.0, 12
    ref, ref32 = oracle_cgnr(A, b, lam, iters)
    Ad, bd = rls.DeviceMatrix.from_host(A, ctx), rls.DeviceVector.from_host(b, ctx)
    S = new_cgnr(rls, Ad, lam, iters)
    x = rls.solve_(S, bd).to_host()
    assert cgnr_path(ctx, S) == 8 and S.state.iteration == ref.iteration == N
    parity_check(f"small_iters_gt_N_{M}x{N}_{dname(dt)}", x, ref.x, ref32)
    S2 = new_cgnr(rls, Ad, lam, iters)
    rls.init_(S2, bd)
    n = 0
    while rls.iterate(S2) is not None:
        n += 1
    assert n == N and S2.state.iteration == N and np.array_equal(S2.state.x.to_host(), x)


@pytest.mark.parametrize("dt,M,N,iters", [(F32, 513, 16, 8), (F32, 32, 129, 8), (C64, 257, 8, 8), (C64, 8, 65, 6), (C64, 161, 8, 8)])
def test_refused_shapes_still_solve(rls, ctx, dt, M, N, iters):
    """one row or one column more than the largest tile: not path 8, and the solve matches the oracle.  (ComplexF32 goes up to
    256 x 64 on the (8, 4) tile -- 64 registers of A per lane, as 256 x 128 Float32 --, so 161 x 8 is inside: it is held to the
    table like every other shape.)"""
    small = pick(dt, M, N) is not None
    assert small == ((dt, M, N) == (C64, 161, 8)) and (small or pick(dt, M - 1, N) or pick(dt, M, N - 1))
    A, _, b = O.make_problem(M, N, dt, 73)
    lam = 1e-2
    ref, ref32 = oracle_cgnr(A, b, lam, iters)
    S = new_cgnr(rls, rls.DeviceMatrix.from_host(A, ctx), lam, iters)
    x = rls.solve_(S, rls.DeviceVector.from_host(b, ctx)).to_host()
    assert (cgnr_path(ctx, S) == 8) == small and S.state.iteration == ref.iteration
    parity_check(f"small_refused_{M}x{N}_{dname(dt)}", x, ref.x, ref32)


# ---- 2. both load paths and the ragged pieces -----------------------------------------------------------------------------------
# (dt, M, N, lda of the aligned upload, tile, what the shape is there for).  Float32 NVE = 4, ComplexF32 NVE = 2.
LDA_CASES = [
    (F32, 250, 40, 252, (8, 4), "last piece of row block 31: 2 live rows; its second piece wholly outside"),
    (F32, 250, 70, 252, (8, 8), "the same on the 8 x 8 tile"),
    (F32, 253, 40, 256, (8, 4), "last piece: exactly 1 live row"),
    (F32, 253, 70, 256, (8, 8), "last piece: exactly 1 live row"),
    (F32, 251, 40, 252, (8, 4), "last piece: NVE - 1 = 3 live rows"),
    (F32, 501, 40, 504, (16, 4), "NQ = 4: piece 0 full, piece 1 one live row, pieces 2 and 3 outside"),
    (F32, 97, 20, 100, (4, 2), "NQ = 1: 1 live row"),
    (F32, 97, 40, 100, (4, 4), "NQ = 1: 1 live row"),
    (F32, 5, 70, 8, (8, 8), "row block 0: piece 0 full, piece 1 one live row; every other row block outside"),
    (F32, 3, 40, 4, (4, 4), "row block 0: 3 live rows; every other row block outside"),
    (F32, 128, 32, None, (4, 2), "aligned shape: vector path against the element path"),
    (F32, 128, 64, None, (4, 4), "aligned shape"),
    (F32, 256, 64, None, (8, 4), "aligned shape"),
    (F32, 256, 128, None, (8, 8), "aligned shape"),
    (F32, 512, 64, None, (16, 4), "aligned shape"),
    (C64, 251, 40, 252, (8, 4), "NQ = 4: last piece 1 live row = NVE - 1"),
    (C64, 65, 20, 66, (4, 2), "NQ = 2: row block 16: piece 0 one live row, piece 1 outside"),
    (C64, 65, 40, 66, (4, 4), "the same on the 4 x 4 tile"),
    (C64, 33, 20, 34, (2, 2), "NQ = 1: 1 live row"),
    (C64, 3, 40, 4, (4, 4), "row block 0: piece 0 full, piece 1 one live row; every other row block outside"),
    (C64, 64, 32, None, (2, 2), "aligned shape"),
    (C64, 128, 32, None, (4, 2), "aligned shape"),
    (C64, 128, 64, None, (4, 4), "aligned shape"),
    (C64, 256, 64, None, (8, 4), "aligned shape"),
]
LDA_IDS = [f"{dname(c[0])}-{c[1]}x{c[2]}-lda{c[3] or c[1]}" for c in LDA_CASES]


def odd_lda(M):
    """a leading dimension whose columns are not 16-byte aligned in either type"""
    return M + 1 if M % 2 == 0 else M + 2


def check_lda_case(dt, M, N, lda, t):
    assert pick(dt, M, N) == t and t[0] % nve(dt) == 0, "a tile with vector loads"
    assert (lda or M) % nve(dt) == 0 and (lda or M) >= M and (odd_lda(M) * np.dtype(dt).itemsize) % 16 != 0


@pytest.mark.parametrize("dt,M,N,lda,t,why", LDA_CASES, ids=LDA_IDS)
def test_load_paths(rls, ctx, dt, M, N, lda, t, why):
    """16-byte pieces (ragged ones re-read element by element) against element loads of the same matrix: each held to float64, and
    the same bits in r after init and in every vector after two steps"""
    check_lda_case(dt, M, N, lda, t)
    pb = problem(M, N, dname(dt))
    tag = f"lda_{M}x{N}_{dname(dt)}"
    al = run_cgnr(rls, ctx, f"{tag}_aligned{lda or M}", pb, upload(rls, ctx, pb["A"], lda), 1e-2)
    un = run_cgnr(rls, ctx, f"{tag}_unaligned{odd_lda(M)}", pb, upload(rls, ctx, pb["A"], odd_lda(M)), 1e-2)
    for k, (a, u) in enumerate(zip(al, un)):
        same_bits(a, u, (tag, "aligned against unaligned upload, after step", k))


# ---- 3. FISTA on the same tiles ---------------------------------------------------------------------------------------------------
KINDS = ["l1", "l2", "none", "l1pos"]
FISTA_STEPS = 7


def fista_regs(R, kind, lam):
    return {"l1": R.L1Regularization(lam), "l2": R.L2Regularization(lam), "none": None,
            "l1pos": [R.L1Regularization(lam), R.PositiveRegularization()], "l21": R.L21Regularization(lam, 4)}[kind]


@functools.lru_cache(maxsize=None)
def fista_problem(M, N, dtn):
    dt = np.dtype(dtn)
    A, _, b = O.make_problem(M, N, dt, 67)
    A64, b64 = A.astype(hi(dt)), b.astype(hi(dt))
    rho = 0.9 / np.linalg.norm(A64, 2) ** 2
    lam = 2e-2 * float(np.max(np.abs(A64.conj().T @ b64)))
    for a in (A, b, A64, b64):
        a.setflags(write=False)
    return dict(A=A, b=b, A64=A64, b64=b64, rho=rho, lam=lam)


@functools.lru_cache(maxsize=None)
def fista_oracle(M, N, dtn, kind, restart):
    """the float64 oracle and the Float32 one after init and after every iteration: (x, xold, res, rel_res_norm) per precision"""
    fp = fista_problem(M, N, dtn)
    out = []
    for A, b in ((fp["A64"], fp["b64"]), (fp["A"], fp["b"])):
        ref = O.FISTA(A, reg=fista_regs(O, kind, fp["lam"]), rho=fp["rho"], iterations=FISTA_STEPS, relTol=0.0, restart=restart)
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


def run_fista(rls, ctx, tag, M, N, dt, kind, restart, Ad, want_path8=True, x0=None):
    """init! and 7 one-iteration calls against the oracles, then init! and ONE 7-iteration call: the same bits.  Returns the final
    state.  `x0`: once init! has been checked, the plan's x0 = A^H b is replaced by this one (init! computes it with the GEMV
    kernel, whose variant depends on the alignment of A: two uploads of one matrix then iterate on the same input)."""
    fp = fista_problem(M, N, dname(dt))
    (ref, nx0, x0_64), (ref32, _, x0_32) = fista_oracle(M, N, dname(dt), kind, restart)
    make = lambda: rls.createLinearSolver(rls.FISTA, Ad, reg=fista_regs(rls, kind, fp["lam"]), rho=fp["rho"], iterations=FISTA_STEPS,
                                          relTol=0.0, restart=restart)
    bd = rls.DeviceVector.from_host(fp["b"], ctx)
    S = make()
    rls.init_(S, bd)
    assert (fista_path(ctx, S) == 8) == want_path8, (tag, fista_path(ctx, S))
    got = fista_state(ctx, S)
    # after init!: x = xold = 0, x0 = A^H b, res = Inf and an infinite residual norm (src/FISTA.jl:110-129), as the oracle
    assert got["it"] == 0 and np.isinf(ref[0][3]) and got["rel"] == ref[0][3], (tag, got["it"], got["rel"])
    parity_check(f"small_{tag}_x_it0", got["x"], ref[0][0], ref32[0][0], record=False)
    parity_check(f"small_{tag}_xold_it0", got["xold"], ref[0][1], ref32[0][1], record=False)
    assert np.array_equal(got["res"], ref[0][2].astype(dt)), (tag, "res after init!")
    parity_check(f"small_{tag}_x0", got["x0"], x0_64, x0_32, tol=TOL_ONE, record=False)
    if x0 is not None:
        S.state.x0.copy_from_host(x0)
    for it in range(1, FISTA_STEPS + 1):
        assert rls.iterate(S) is not None
        if it in (1, 2, FISTA_STEPS):
            got = fista_state(ctx, S)
            assert got["it"] == it and all(np.isfinite(got[k]).all() for k in ("x", "xold", "res")), (tag, it)
            ex = parity_check(f"small_{tag}_x_it{it}", got["x"], ref[it][0], ref32[it][0], record=it == FISTA_STEPS)
            parity_check(f"small_{tag}_xold_it{it}", got["xold"], ref[it][1], ref32[it][1], record=False)
            er = parity_check(f"small_{tag}_res_it{it}", got["res"], ref[it][2], ref32[it][2], scale=nx0, record=False)
            assert abs(got["rel"] - ref[it][3]) < 1e-4 * ref[it][3] + 2e-6, (tag, it, got["rel"], ref[it][3])
            if it == FISTA_STEPS:
                print(f"[small] {tag}_it{it}: x device {ex:.3e}  f32-oracle {rel(ref32[it][0], ref[it][0]):.3e}  res {er:.3e}")
    assert rls.iterate(S) is None
    if not want_path8:
        return got
    S1 = make()
    rls.init_(S1, bd)
    if x0 is not None:
        S1.state.x0.copy_from_host(x0)
    assert ctx.lib.rls_fista_step(S1.state._plan, FISTA_STEPS) == 0
    once = fista_state(ctx, S1)
    for k in ("x", "xold", "res"):
        assert np.array_equal(once[k], got[k]), (tag, k, "one 7-step call against 7 one-step calls")
    assert once["rel"] == got["rel"] and once["it"] == FISTA_STEPS
    return got


FISTA_CASES = [(dt, t, "full", 32 * t[0], 16 * t[1], kind, restart) for dt in DTYPES for t in tiles(dt) for kind in KINDS
               for restart in ("none", "gradient")]
FISTA_CASES += [(dt, t, "ragged", 32 * t[0] - 3, 16 * t[1] - 3, KINDS[(i + (2 if cplx(dt) else 0)) % 4], restart)
                for dt in DTYPES for i, t in enumerate(tiles(dt)) for restart in ("none", "gradient")]


@pytest.mark.parametrize("dt,t,shape,M,N,kind,restart", FISTA_CASES,
                         ids=[f"{dname(c[0])}-R{c[1][0]}C{c[1][1]}-{c[2]}-{c[5]}-{c[6]}" for c in FISTA_CASES])
def test_fista_on_every_tile(rls, ctx, dt, t, shape, M, N, kind, restart):
    assert pick(dt, M, N) == t
    fp = fista_problem(M, N, dname(dt))
    run_fista(rls, ctx, f"fista_tile{t[0]}x{t[1]}_{M}x{N}_{dname(dt)}_{kind}_{restart}", M, N, dt, kind, restart, upload(rls, ctx, fp["A"]))


@pytest.mark.parametrize("dt,M,N,lda,t,why", LDA_CASES, ids=LDA_IDS)
def test_fista_load_paths(rls, ctx, dt, M, N, lda, t, why):
    check_lda_case(dt, M, N, lda, t)
    fp = fista_problem(M, N, dname(dt))
    kind, restart = KINDS[(M + N) % 4], ("gradient" if M % 2 else "none")
    tag = f"fista_lda_{M}x{N}_{dname(dt)}_{kind}_{restart}"
    al = run_fista(rls, ctx, f"{tag}_aligned{lda or M}", M, N, dt, kind, restart, upload(rls, ctx, fp["A"], lda))
    un = run_fista(rls, ctx, f"{tag}_unaligned{odd_lda(M)}", M, N, dt, kind, restart, upload(rls, ctx, fp["A"], odd_lda(M)), x0=al["x0"])
    for k in ("x", "xold", "res", "x0"):   # the same x0 in, the same registers of A: the same bits out
        assert np.array_equal(al[k], un[k]), (tag, k)


@pytest.mark.parametrize("dt", DTYPES)
def test_fista_refused_regulariser_still_solves(rls, ctx, dt):
    """L21 couples the elements of a group: not an elementwise update of one wave, so the small path refuses it"""
    M, N = 64, 32
    assert pick(dt, M, N) is not None
    fp = fista_problem(M, N, dname(dt))
    run_fista(rls, ctx, f"fista_l21_{M}x{N}_{dname(dt)}", M, N, dt, "l21", "none", upload(rls, ctx, fp["A"]), want_path8=False)


# ---- 4. groups and step splitting -------------------------------------------------------------------------------------------------
def group_max(rls):
    """RLS_SMALL_GROUP_MAX, from the header the library is built from"""
    hdr = os.path.join(os.path.dirname(os.path.abspath(rls.__file__)), "csrc", "rls_common.hpp")
    with open(hdr) as f:
        m = re.search(r"constexpr\s+int\s+RLS_SMALL_GROUP_MAX\s*=\s*(\d+)\s*;", f.read())
    assert m, "RLS_SMALL_GROUP_MAX not found in rls_common.hpp"
    return int(m.group(1))


@pytest.mark.parametrize("dt,big,t", [(F32, (100, 50), (4, 4)), (F32, (200, 30), (8, 4)), (C64, (100, 50), (4, 4)), (C64, (200, 30), (8, 4))])
def test_mixed_group_runs_on_the_largest_members_tile(rls, ctx, dt, big, t):
    """one launch: the largest member picks the tile, the others leave most of it dead"""
    shapes = [(1, 1), (5, 3), big, (33, 2), (2, 17)]
    assert pick(dt, max(s[0] for s in shapes), max(s[1] for s in shapes)) == t
    assert all(pick(dt, *s) != t for s in shapes if s != big)
    lam, iters = 1e-2, 2   # (no member goes past its rank: the iterates stay determined)
    probs = [O.make_problem(M, N, dt, 300 + k) for k, (M, N) in enumerate(shapes)]
    mats = [rls.DeviceMatrix.from_host(A, ctx) for A, _, _ in probs]
    rhs = [rls.DeviceVector.from_host(b, ctx) for _, _, b in probs]
    K = len(shapes)
    # init! alone as one group launch: every member's r = A^H b on the shared tile
    group = [new_cgnr(rls, Ad, lam, iters) for Ad in mats]
    plans = (C.c_void_p * K)()
    for k, (s_, b) in enumerate(zip(group, rhs)):
        s_._prepare(s_.state, b)
        plans[k] = s_.state._plan
        assert cgnr_path(ctx, s_) == 8
    bptr = (C.c_void_p * K)(*[b.ptr for b in rhs])
    rls._lib.check(ctx.handle, ctx.lib.rls_cgnr_init_step_group(plans, bptr, K, lam, 0.0, iters, 0), "init_step_group")
    for k, (A, _, b) in enumerate(probs):
        r = group[k].state.x0.to_host()
        h = hi(dt)
        e = parity_check(f"small_group_{dname(dt)}_tile{t[0]}x{t[1]}_member{k}_AhB", r, A.astype(h).conj().T @ b.astype(h), A.conj().T @ b, tol=TOL_ONE)
        print(f"[small] group_{dname(dt)}_tile{t[0]}x{t[1]}_member{shapes[k][0]}x{shapes[k][1]}_AhB: device {e:.3e}")
        solo = new_cgnr(rls, mats[k], lam, iters)
        rls.init_(solo, rhs[k])
        if shapes[k] in ((1, 1), big):   # the solo plan of the largest member runs the same tile; 1 x 1: one product and zeros
            assert np.array_equal(r, solo.state.x0.to_host()), (k, "r after init, group member against solo plan")
        else:   # (the group runs on the tile of its largest member: another summation order)
            assert rel(r, solo.state.x0.to_host()) < 1e-4
    xs = rls.solve_group_([new_cgnr(rls, Ad, lam, iters) for Ad in mats], rhs)
    for k, ((A, _, b), x) in enumerate(zip(probs, xs)):
        ref, ref32 = oracle_cgnr(A, b, lam, iters)
        parity_check(f"small_group_{dname(dt)}_tile{t[0]}x{t[1]}_member{k}_x", x.to_host(), ref.x, ref32)
        solo = rls.solve_(new_cgnr(rls, mats[k], lam, iters), rhs[k]).to_host()
        if shapes[k] == big:
            assert np.array_equal(x.to_host(), solo), (k, "x, group member against solo solve on the same tile")
        else:
            assert rel(x.to_host(), solo) < 1e-4   # (the group runs on the tile of its largest member: another summation order)


@pytest.mark.parametrize("dt", DTYPES)
def test_group_size_edges(rls, ctx, dt):
    """RLS_SMALL_GROUP_MAX members are one launch; one more makes a second launch of one, which is a solo solve"""
    G = group_max(rls)
    rng = np.random.default_rng(11)
    shapes = [(lambda N: (int(rng.integers(2 * N + 4, 60)), N))(int(rng.integers(3, 13))) for _ in range(G + 1)]
    shapes[G] = (90, 20)   # the member left over has a tile of its own
    lam, iters = 1e-2, 4
    probs = [O.make_problem(M, N, dt, 400 + k) for k, (M, N) in enumerate(shapes)]
    mats = [rls.DeviceMatrix.from_host(A, ctx) for A, _, _ in probs]
    rhs = [rls.DeviceVector.from_host(b, ctx) for _, _, b in probs]
    solve = lambda n: [x.to_host() for x in rls.solve_group_([new_cgnr(rls, Ad, lam, iters) for Ad in mats[:n]], rhs[:n])]
    full, over = solve(G), solve(G + 1)
    for k, ((A, _, b), x) in enumerate(zip(probs, over)):
        ref, ref32 = oracle_cgnr(A, b, lam, iters)
        parity_check(f"small_group_edges_{dname(dt)}_{k}", x, ref.x, ref32, record=k in (0, G))
    for k in range(G):
        assert np.array_equal(full[k], over[k]), k   # the first launch is the same launch
    assert np.array_equal(over[G], rls.solve_(new_cgnr(rls, mats[G], lam, iters), rhs[G]).to_host())


SPLIT_CASES = [(dt, t) for dt in DTYPES for t in tiles(dt)]


@pytest.mark.parametrize("dt,t", SPLIT_CASES, ids=[f"{dname(c[0])}-R{c[1][0]}C{c[1][1]}" for c in SPLIT_CASES])
def test_step_splitting_and_server_mode(rls, ctx, dt, t):
    """init + n steps in one launch == init + k + (n - k) steps, as plain launches, as commands to a workgroup that stays and runs
    one iteration ahead, and with that mode off -- bit for bit; a call on a plan that is done changes no bit"""
    M, N = ROW_BLOCKS * t[0], COL_BLOCKS * t[1]
    pb = problem(M, N, dname(dt))
    Ad, bd = upload(rls, ctx, pb["A"]), rls.DeviceVector.from_host(pb["b"], ctx)
    lam, n, k = 1e-2, 6, 2
    lib, check = ctx.lib, rls._lib.check

    def started(iters=n, relTol=0.0):
        S = new_cgnr(rls, Ad, lam, iters, relTol)
        rls.init_(S, bd)
        assert cgnr_path(ctx, S) == 8
        return S

    one = started()
    check(ctx.handle, lib.rls_cgnr_step(one.state._plan, n), "cgnr_step")
    want = snap(ctx, one)
    assert want["it"] == n and want["done"] == 1
    two = started()
    check(ctx.handle, lib.rls_cgnr_step(two.state._plan, k), "cgnr_step")
    check(ctx.handle, lib.rls_cgnr_step(two.state._plan, n - k), "cgnr_step")
    same_bits(want, snap(ctx, two), "k + (n - k) steps, plain launches")
    srv = started()
    srv.state._step_status(lib, k)       # no other call in between: the second command goes to the workgroup left listening,
    srv.state._step_status(lib, n - k)   # which has its first iteration done ahead
    same_bits(want, snap(ctx, srv), "k + (n - k) steps, server mode")
    ctx.tune(resident_server=0)
    try:
        off = started()
        off.state._step_status(lib, k)
        off.state._step_status(lib, n - k)
        got = snap(ctx, off)
    finally:
        ctx.tune(resident_server=1)
    same_bits(want, got, "k + (n - k) steps, server mode off")
    # done on max_iter: further calls, of either kind, change nothing
    check(ctx.handle, lib.rls_cgnr_step(one.state._plan, 3), "cgnr_step")
    one.state._step_status(lib, 1)
    after = snap(ctx, one)
    same_bits(want, after, "steps after done (max_iter)")
    assert after["it"] == n and after["done"] == 1
    # done on relTol, inside a launch
    tol = started(iters=12, relTol=0.2)
    check(ctx.handle, lib.rls_cgnr_step(tol.state._plan, 12), "cgnr_step")
    stop = snap(ctx, tol)
    assert 0 < stop["it"] < 12 and stop["done"] == 1 and stop["residual"] <= 0.2 * stop["z0"] * (1 + 1e-6)
    check(ctx.handle, lib.rls_cgnr_step(tol.state._plan, 2), "cgnr_step")
    tol.state._step_status(lib, 1)
    again = snap(ctx, tol)
    same_bits(stop, again, "steps after done (relTol)")
    assert again["it"] == stop["it"] and again["done"] == 1
