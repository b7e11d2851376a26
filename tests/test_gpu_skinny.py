"""The shared-A matrix-core kernels of csrc/skinny.hip, product by product, at every loop regime and shipped variant.

What is read.  `CgnrBatchedState` owns X, R, P, V as N x K device matrices, and the batched CGNR plan (rls_cgnr_*_batched,
path 3; path 6 with an explicit AHA) is nothing but these kernels:
  after init       R = P = A^H B         skinny_pack_rows_kernel -> skinny_v_kernel -> skinny_u_kernel<E, INIT> (sums the splits)
  after one step   V = A^H (A P0)        skinny_t_kernel -> skinny_v_kernel; the step's skinny_u_kernel stores the summed V
                   V = AHA P0            Gram mode: skinny_t_kernel<..., VOUT> over the N x N matrix (launch_g)
                   X, R, P, status()     skinny_u_kernel<E, false, EPT, NT>
so R after init is ONE product of known inputs, V after a step is the product(s) of the DEVICE's own P0, and X1, R1, P1 and the
scalars are an elementwise function of the device's own P0, R0, V.  Each is compared on its own, per column:
  one product            2e-6 relative l2 (as test_gemv_all_ops)                      R0; V in Gram mode; rls_gram
  two chained products   3e-6             (as test_normal_operator_one_pass_vs_two_pass)   V = A^H (A P0)
both through conftest.parity_check with the same product done by NumPy in the working precision as the Float32 yardstick;
  update outputs         4 x 2e-7 relative l2 per column (as test_blas1), alpha and beta 1e-6 relative.
The update is rebuilt in float64 from the device's P0, R0, V (src/CGNR.jl:153-176): alpha = |r|^2 / (<p, v> + lambda |p|^2),
x1 = x + alpha p, r1 = r - alpha v - alpha lambda p, beta = |r1|^2 / |r|^2, p1 = beta p + r1.  alpha and beta are compared as
float64 numbers; where they multiply a vector they are working-precision scalars (as in the reference, whose scalars have
the element type), i.e. rounded to Float32 first.  On NumPy's Float32 products of these Gaussian inputs: the largest error
on the CPU is 1.7e-6 (A^H (A P), float32, contraction 8192), so the fixed bounds and not the 2 x yardstick gate every case.

skinny_u_kernel<E, INIT, EPT, NT> by N (launch_u); INIT always runs <E, true, 0, 1024>:
  N <= 1024                    <E, false, 2, 512>     16 and 1008: clamped tail (i >= N), 1024: exact
  1024 < N <= 2048             <E, false, 4, 512>     1040, 2048
  2048 < N <= 4096             <E, false, 8, 512>     2064, 4096
  4096 < N <= 8192, float32    <float, false, 8, 1024>     4112, 8192
  4096 < N, complex64          <float2, false, 0, 1024>    4112      (vectors re-read between the reductions)
  8192 < N                     <E, false, 0, 1024>    8208 (float32)

Tuning values that select no instantiation of their own (launch_t / launch_v / launch_g), so no case claims them:
  float32                      skinny_t_roll / _v_roll / _g_roll are ignored (the rolling window is a complex-only form)
  skinny_t_roll = 32, full     no such instantiation: the (t_waves, t_u) two-set pipeline runs
  a roll depth and waves != 8  four waves (skinny_t_waves = 2 with a roll depth launches four)
  a roll depth                 t_u = 4 / v_u = 1 whatever skinny_t_u / skinny_v_u say
  a (waves, u) pair not listed the default <4, 4> (T) / <4, 1> (V);  skinny_g_roll other than 0 and 16: 8
The variants are run with the other switch at 0 so that each listed value reaches its own kernel."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

import rls_oracle as O
from conftest import parity_check

pytestmark = pytest.mark.gpu

TOL_ONE, TOL_TWO = 2e-6, 3e-6   # one product (test_gemv_all_ops), two chained products (test_normal_operator_one_pass_vs_two_pass)
TOL_ELEM, TOL_SCALAR = 4 * 2e-7, 1e-6   # elementwise kernels (test_blas1), alpha / beta
DTYPES = [np.float32, np.complex64]
DEFAULTS = dict(skinny_t_waves=4, skinny_t_u=4, skinny_v_waves=4, skinny_v_u=1, skinny_v_splits=0, skinny_t_roll=8,
                skinny_v_roll=2, skinny_g_roll=8, skinny_half=1, resident=1)


def hi(dt):
    return np.complex128 if np.dtype(dt).kind == "c" else np.float64


def cplx(dt):
    return np.dtype(dt).kind == "c"


def rel(a, b):
    d = np.linalg.norm(np.asarray(a).astype(np.complex128) - np.asarray(b).astype(np.complex128))
    n = np.linalg.norm(np.asarray(b).astype(np.complex128))
    return float(d / n) if n > 0 else float(d)


def gauss(rng, shape, dt):
    v = rng.standard_normal(shape)
    if cplx(dt):
        v = (v + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)
    return np.asfortranarray(v.astype(dt))


@contextlib.contextmanager
def tuned(ctx, **kw):
    """the context's switches set for one case, every one of this file's back at its default afterwards"""
    try:
        ctx.tune(**kw)
        yield
    finally:
        ctx.tune(**DEFAULTS)


@functools.lru_cache(maxsize=8)
def problem(M, N, K, dtname):
    """Gaussian A (M x N) and B (M x K, column 0 scaled by 1e-3) with A^H B in float64 and in the working precision:
    computed once per shape, shared by every case on it, never written to"""
    dt = np.dtype(dtname)
    rng = np.random.default_rng(1000003 * M + 1009 * N + 31 * K + (7 if cplx(dt) else 0))
    A, B = gauss(rng, (M, N), dt), gauss(rng, (M, K), dt)
    B[:, 0] *= 1e-3
    A64 = A.astype(hi(dt))
    out = dict(A=A, B=B, A64=A64, R64=A64.conj().T @ B.astype(hi(dt)), R32=A.conj().T @ B)
    for a in out.values():
        a.setflags(write=False)
    return out


def gate(tag, got, ref64, ref32, tol):
    """every column through the project's gate; the worst column is the one that goes into the log and the table"""
    assert got.shape == ref64.shape and np.isfinite(got).all(), tag
    errs = [rel(got[:, j], ref64[:, j]) for j in range(got.shape[1])]
    worst = int(np.argmax(errs))
    print(f"[skinny] {tag}: device {errs[worst]:.3e}  numpy-f32 {rel(ref32[:, worst], ref64[:, worst]):.3e}  (column {worst})")
    for j in range(got.shape[1]):
        parity_check(f"skinny_{tag}_col{j}", got[:, j], ref64[:, j], ref32[:, j], tol=tol, record=(j == worst))
    return errs[worst]


def cgnr_path(rls, S):
    out = C.c_int32(-1)
    assert rls.load().rls_cgnr_path(S.state._plan, C.byref(out)) == 0
    return out.value


def snapshot(st):
    return dict(X=st.X.to_host().copy(), R=st.R.to_host().copy(), P=st.P.to_host().copy(), V=st.V.to_host().copy(),
                status=st.status())


def run_cgnr(rls, Ad, Bd, lam=0.0, steps=1, gram=None):
    """init! and `steps` single steps of the batched plan; the state after init and after every step"""
    S = rls.createLinearSolver(rls.CGNR, Ad, AHA=gram, reg=rls.L2Regularization(lam) if lam else None, iterations=64, relTol=0.0)
    rls.init_(S, Bd, scheduler=rls.BatchedState)
    st = S.state
    assert isinstance(st, rls.CgnrBatchedState), "the shape must take the shared-A plan"
    assert cgnr_path(rls, S) == (6 if gram is not None else 3)
    snaps = [snapshot(st)]
    for _ in range(steps):
        st._step(1)
        snaps.append(snapshot(st))
    return snaps


def check_init(tag, pb, s0):
    """R = P = A^H B, x = v = 0, scalars of init!"""
    gate(f"{tag}_AhB", s0["R"], pb["R64"], pb["R32"], TOL_ONE)
    assert np.array_equal(s0["R"], s0["P"]), tag
    assert not s0["X"].any() and not s0["V"].any(), tag
    for j, s_ in enumerate(s0["status"]):
        z0 = np.linalg.norm(s0["R"][:, j].astype(hi(s0["R"].dtype)))
        assert s_.iteration == 0 and s_.done == 0 and abs(s_.z0 - z0) <= TOL_SCALAR * z0, (tag, j)


def check_product(tag, pb, prev, cur, G=None):
    """V against the float64 product of the device's own P"""
    dt = prev["P"].dtype
    P64 = prev["P"].astype(hi(dt))
    if G is None:
        ref64 = pb["A64"].conj().T @ (pb["A64"] @ P64)
        ref32 = pb["A"].conj().T @ (pb["A"] @ prev["P"])
        return gate(f"{tag}_AhAP", cur["V"], ref64, ref32, TOL_TWO)
    return gate(f"{tag}_GP", cur["V"], G.astype(hi(dt)) @ P64, G @ prev["P"], TOL_ONE)


def check_update(tag, prev, cur, lam, it):
    """X, R, P and the scalars after a step against src/CGNR.jl:153-176 in float64 on the device's own p, r, v"""
    dt = prev["P"].dtype
    h = hi(dt)
    lam32 = float(np.float32(lam))
    x, r, p, v = prev["X"].astype(h), prev["R"].astype(h), prev["P"].astype(h), cur["V"].astype(h)
    zeta = np.sum(np.abs(r) ** 2, axis=0)
    pp = np.sum(np.abs(p) ** 2, axis=0)
    alpha = zeta / (np.sum(p.conj() * v, axis=0) + lam32 * pp)
    a = alpha.astype(dt).astype(h)  # applied as a working-precision scalar
    x1 = x + a * p
    r1 = r - a * v - (a * lam32) * p
    rr = np.sum(np.abs(r1) ** 2, axis=0)
    beta = rr / zeta
    p1 = beta.astype(np.float32).astype(np.float64) * p + r1
    worst = {}
    for name, got, want in (("x", cur["X"], x1), ("r", cur["R"], r1), ("p", cur["P"], p1)):
        assert np.isfinite(got).all(), (tag, name)
        errs = [rel(got[:, j], want[:, j]) for j in range(got.shape[1])]
        worst[name] = max(errs)
        assert worst[name] <= TOL_ELEM, (tag, name, int(np.argmax(errs)), worst[name])
    sc = 0.0
    for j, s_ in enumerate(cur["status"]):
        assert s_.iteration == it and s_.done == 0, (tag, j, s_.iteration, s_.done)
        ea = abs(complex(s_.alpha_re, s_.alpha_im) - alpha[j]) / abs(alpha[j])
        eb = abs(complex(s_.beta_re, s_.beta_im) - beta[j]) / beta[j]
        ez = abs(s_.zeta - zeta[j]) / zeta[j]
        er = abs(s_.residual - np.sqrt(rr[j])) / np.sqrt(rr[j])
        sc = max(sc, ea, eb, ez, er)
        assert max(ea, eb, ez, er) <= TOL_SCALAR, (tag, j, ea, eb, ez, er)
        assert s_.beta_im == 0.0 and (cplx(dt) or s_.alpha_im == 0.0), (tag, j)
    print(f"[skinny] {tag}_update{it}: x {worst['x']:.3e}  r {worst['r']:.3e}  p {worst['p']:.3e}  scalars {sc:.3e}")


def full_case(rls, ctx, tag, dt, M, N, K, lam=0.0, steps=1, gram=False):
    """init, `steps` steps, every product and every update checked; returns the snapshots"""
    pb = problem(M, N, K, np.dtype(dt).name)
    Ad, Bd = rls.DeviceMatrix.from_host(pb["A"], ctx), rls.DeviceMatrix.from_host(pb["B"], ctx)
    Gd = Ad.gram() if gram else None
    G = Gd.to_host() if gram else None
    snaps = run_cgnr(rls, Ad, Bd, lam, steps, Gd)
    check_init(tag, pb, snaps[0])
    for k in range(1, steps + 1):
        check_product(f"{tag}_step{k}", pb, snaps[k - 1], snaps[k], G)
        check_update(tag, snaps[k - 1], snaps[k], lam, k)
    return snaps


def name(dt, M, N, K):
    return f"{M}x{N}_{np.dtype(dt).name}_K{K}"


# ---- 1. T-kernel loop regimes: ns = N / 16 steps per wave -----------------------------------------------------------------------
# 16, 48: no full batch; 64, 80: one; 128: two (the tail pair); 208: three and a remainder; 256: ns == 2 D for the complex rolling
# window; 272: ns >= 2 D, not a multiple of D; 384: rolled, three rounds.  M = 32: two row blocks over four V waves, so two of
# them get no step.  Complex K = 3: the (8 re | 8 im) half layout, K = 9: the full layout.
@pytest.mark.parametrize("K", [3, 9])
@pytest.mark.parametrize("N", [16, 48, 64, 80, 128, 208, 256, 272, 384])
@pytest.mark.parametrize("dt", DTYPES)
def test_t_kernel_loop_regimes(rls, ctx, dt, N, K):
    with tuned(ctx):
        full_case(rls, ctx, "t_" + name(dt, 32, N, K), dt, 32, N, K)


# ---- 2. V-kernel loop regimes ---------------------------------------------------------------------------------------------------
# N = 32 at the natural split count: M = 16, 32, 48: fewer row blocks than waves; 64, 80: one step each, one wave two; 272: 17 row
# blocks, S = 1; 1040: S = 4 over 65 row blocks.  N = 16 with M = 4096 / 4112: S = 16 over 256 / 257 row blocks.
@pytest.mark.parametrize("K", [3, 9])
@pytest.mark.parametrize("M,N", [(16, 32), (32, 32), (48, 32), (64, 32), (80, 32), (272, 32), (1040, 32), (4096, 16), (4112, 16)])
@pytest.mark.parametrize("dt", DTYPES)
def test_v_kernel_loop_regimes(rls, ctx, dt, M, N, K):
    with tuned(ctx):
        full_case(rls, ctx, "v_" + name(dt, M, N, K), dt, M, N, K)


# 17 row blocks over 3, 5, 7 splits (lo = s MB / S uneven; the update kernels sum S in batches of four: 3, 4 + 1, 4 + 3) and over
# 20 (three splits own no row block and must write zeros; 4 x 5 batches)
@pytest.mark.parametrize("S", [3, 5, 7, 20])
@pytest.mark.parametrize("dt", DTYPES)
def test_v_kernel_row_splits(rls, ctx, dt, S):
    with tuned(ctx, skinny_v_splits=S):  # read when the plan is created
        full_case(rls, ctx, f"v_{name(dt, 272, 32, 3)}_S{S}", dt, 272, 32, 3, lam=1e-2)


# ---- 3. right-hand-side counts: every column asserted, the last one next to the padding columns of its group -------------------
@pytest.mark.parametrize("K", [2, 8, 9, 16, 17, 33])
@pytest.mark.parametrize("dt", DTYPES)
def test_rhs_counts(rls, ctx, dt, K):
    with tuned(ctx):
        got = full_case(rls, ctx, "k_" + name(dt, 64, 64, K), dt, 64, 64, K, lam=1e-2)
        if cplx(dt) and K <= 8:
            # the (8 re | 8 im) operand layout runs the same four FMA chains per element as the 16-column one
            ctx.tune(skinny_half=0)
            full = full_case(rls, ctx, "k_" + name(dt, 64, 64, K) + "_full", dt, 64, 64, K, lam=1e-2)
            assert np.array_equal(got[0]["R"], full[0]["R"]) and np.array_equal(got[1]["V"], full[1]["V"])


# ---- 4. update-kernel dispatch on N (table in the module docstring); two steps, so that the second product reads the operand
# panel the first update wrote ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", [0.0, 1e-2])
@pytest.mark.parametrize("dt,N", [(dt, N) for dt in DTYPES for N in (16, 1008, 1024, 1040, 2048, 2064, 4096, 4112)] +
                         [(np.float32, 8192), (np.float32, 8208)])
def test_update_kernel_dispatch(rls, ctx, dt, N, lam):
    with tuned(ctx):
        full_case(rls, ctx, f"u_{name(dt, 16, N, 3)}_lam{lam}", dt, 16, N, 3, lam=lam, steps=2)


# ---- 5. tuning variants ----------------------------------------------------------------------------------------------------------
T_PAIRS = [(4, 4), (8, 4), (8, 8), (4, 8), (4, 2), (4, 16), (2, 4)]   # launch_t, full layout (and the default)
T_PAIRS_HALF = T_PAIRS + [(8, 2), (8, 16)]
V_PAIRS = [(4, 1), (8, 1), (8, 2), (4, 2), (4, 4), (2, 1), (2, 2)]    # launch_v, both layouts (and the default)


def variant_products(rls, ctx, tag, pb, Ad, Bd, refs, Gd=None, G=None):
    """R0 and V1 of one variant, both held to float64; the reference of V is shared by the variants that start from the same P0"""
    s0, s1 = run_cgnr(rls, Ad, Bd, gram=Gd)
    gate(f"{tag}_AhB", s0["R"], pb["R64"], pb["R32"], TOL_ONE)
    key = s0["P"].tobytes()
    if key not in refs:
        h = hi(s0["P"].dtype)
        if G is None:
            refs[key] = (pb["A64"].conj().T @ (pb["A64"] @ s0["P"].astype(h)), pb["A"].conj().T @ (pb["A"] @ s0["P"]))
        else:
            refs[key] = (G.astype(h) @ s0["P"].astype(h), G @ s0["P"])
    gate(f"{tag}_{'GP' if G is not None else 'AhAP'}", s1["V"], refs[key][0], refs[key][1], TOL_TWO if G is None else TOL_ONE)
    return s0["R"], s1["V"]


def assert_same_bits(group, what):
    """variants that run the same FMA chains (same wave count and splits; prefetch depth and operand layout differ)"""
    tags = sorted(group)
    for t in tags[1:]:
        assert np.array_equal(group[tags[0]], group[t]), (what, tags[0], t, float(np.abs(group[tags[0]] - group[t]).max()))


def layouts(dt):
    return [("half", 1), ("full", 0)] if cplx(dt) else [("full", 0)]


@pytest.mark.parametrize("N", [2048, 2064])
@pytest.mark.parametrize("dt", DTYPES)
def test_t_variants(rls, ctx, dt, N):
    """every (t_waves, t_u) pair of launch_t with the rolling window off, and every rolling-window depth, on 32 x 2048 (every
    per-wave step count a multiple of every depth) and 32 x 2064 (129 steps per wave at four waves; 65 | 64 at eight: half the
    waves roll).  Same bits at equal wave count: for complex data the chains do not depend on the batching at all; for float32
    the two chains alternate within a batch and the one-at-a-time remainder goes to chain 0, which at 128, 129, 64 and 65
    steps is the same assignment for every even batch size."""
    K = 3
    pb = problem(32, N, K, np.dtype(dt).name)
    Ad, Bd = rls.DeviceMatrix.from_host(pb["A"], ctx), rls.DeviceMatrix.from_host(pb["B"], ctx)
    refs, bits = {}, {2: {}, 4: {}, 8: {}}
    for lname, half in layouts(dt):
        for w, u in (T_PAIRS_HALF if half else T_PAIRS):
            with tuned(ctx, skinny_half=half, skinny_t_waves=w, skinny_t_u=u, skinny_t_roll=0):
                tag = f"tvar_{name(dt, 32, N, K)}_{lname}_w{w}_u{u}"
                bits[w][tag] = variant_products(rls, ctx, tag, pb, Ad, Bd, refs)[1]
        for d in ((8, 16, 32) if half else (8, 16)) if cplx(dt) else ():
            for w in (4, 8):
                with tuned(ctx, skinny_half=half, skinny_t_waves=w, skinny_t_roll=d):
                    tag = f"tvar_{name(dt, 32, N, K)}_{lname}_w{w}_roll{d}"
                    bits[w][tag] = variant_products(rls, ctx, tag, pb, Ad, Bd, refs)[1]
    for w, group in bits.items():
        assert_same_bits(group, f"T kernel, {w} waves")


@pytest.mark.parametrize("splits", [1, 0])
@pytest.mark.parametrize("M", [2048, 2064])
@pytest.mark.parametrize("dt", DTYPES)
def test_v_variants(rls, ctx, dt, M, splits):
    """every (v_waves, v_u) pair of launch_v with the rolling window off, and every rolling-window depth, on 2048 x 32 and
    2064 x 32 as one split (32 | 33 steps per wave at four waves) and at the natural count (8 splits of 16 | 17 row blocks).
    Both the init product and the step run the variant.  Same bits at equal wave count and split count: no chain of the V
    kernel depends on the batching (float32: chain t & 1 by row within a step)."""
    K = 3
    pb = problem(M, 32, K, np.dtype(dt).name)
    Ad, Bd = rls.DeviceMatrix.from_host(pb["A"], ctx), rls.DeviceMatrix.from_host(pb["B"], ctx)
    refs, bits_r, bits_v = {}, {2: {}, 4: {}, 8: {}}, {2: {}, 4: {}, 8: {}}
    for lname, half in layouts(dt):
        for w, u in V_PAIRS:
            with tuned(ctx, skinny_half=half, skinny_v_splits=splits, skinny_v_waves=w, skinny_v_u=u, skinny_v_roll=0):
                tag = f"vvar_{name(dt, M, 32, K)}_S{splits}_{lname}_w{w}_u{u}"
                bits_r[w][tag], bits_v[w][tag] = variant_products(rls, ctx, tag, pb, Ad, Bd, refs)
        for d in (2, 4, 8) if cplx(dt) else ():
            for w in (4, 8):
                with tuned(ctx, skinny_half=half, skinny_v_splits=splits, skinny_v_waves=w, skinny_v_roll=d):
                    tag = f"vvar_{name(dt, M, 32, K)}_S{splits}_{lname}_w{w}_roll{d}"
                    bits_r[w][tag], bits_v[w][tag] = variant_products(rls, ctx, tag, pb, Ad, Bd, refs)
    for w in bits_r:
        assert_same_bits(bits_r[w], f"V kernel (init), {w} waves")
        assert_same_bits(bits_v[w], f"V kernel (step), {w} waves")


@pytest.mark.parametrize("N", [2048, 2064])
def test_gram_mode_variants(rls, ctx, N):
    """V = AHA P0 as one skinny_t_kernel<..., VOUT> product (path 6) at skinny_g_roll 0, 8, 16 in both layouts: 128 steps per wave
    (rolled) and 129 (two-set pipeline and a remainder).  Four waves throughout, so every variant gives the same bits."""
    dt, K = np.complex64, 3
    pb = problem(16, N, K, np.dtype(dt).name)
    Ad, Bd = rls.DeviceMatrix.from_host(pb["A"], ctx), rls.DeviceMatrix.from_host(pb["B"], ctx)
    Gd = Ad.gram()
    G = Gd.to_host()
    refs, bits = {}, {}
    for lname, half in layouts(dt):
        for d in (0, 8, 16):
            with tuned(ctx, resident=0, skinny_half=half, skinny_g_roll=d):
                tag = f"gvar_{name(dt, 16, N, K)}_{lname}_roll{d}"
                bits[tag] = variant_products(rls, ctx, tag, pb, Ad, Bd, refs, Gd, G)[1]
    assert_same_bits(bits, "Gram mode")


# ---- 6. Gram mode, S = 16 column splits (from M = 4096) over 4 and 12 four-column blocks: splits that own none write zeros ------
@pytest.mark.parametrize("N", [16, 48])
@pytest.mark.parametrize("dt", DTYPES)
def test_gram_mode_empty_column_splits(rls, ctx, dt, N):
    with tuned(ctx, resident=0):
        full_case(rls, ctx, "g_" + name(dt, 4096, N, 3), dt, 4096, N, 3, lam=1e-2, steps=2, gram=True)


# ---- 7. the setup GEMM, rls_gram -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,tiles", [(16, 64, True), (32, 64, True), (64, 128, True), (48, 192, True),   # 1, 2, 4, 3 row blocks
                                       (16, 16, False), (16, 48, False), (272, 80, False), (32, 1040, False)])
@pytest.mark.parametrize("dt", DTYPES)
def test_gram_setup(rls, ctx, dt, M, N, tiles):
    """gram_mfma_kernel (N a multiple of 64) and the A^H T form with T = A (skinny_pack_rows_kernel + skinny_v_kernel)"""
    A = problem(M, N, 3, np.dtype(dt).name)["A"]
    with tuned(ctx):
        G = rls.DeviceMatrix.from_host(A, ctx).gram().to_host()
    A64 = A.astype(hi(dt))
    gate(f"gram_{'tiles' if tiles else 'panels'}_{name(dt, M, N, 0)}", G, A64.conj().T @ A64, A.conj().T @ A, TOL_ONE)
    if tiles:  # entry (i, j) and entry (j, i) run the same products in the same order
        assert np.array_equal(G, G.conj().T)
        assert not np.iscomplexobj(G) or not np.diagonal(G).imag.any()


# ---- 8. padded leading dimensions: the padding rows of A and of B hold NaN ------------------------------------------------------
def padded(rls, ctx, a, ld):
    d = rls.DeviceMatrix(a.shape[0], a.shape[1], a.dtype, ctx, lda=ld)
    buf = np.full((ld, a.shape[1]), np.nan, dtype=a.dtype, order="F")
    buf[: a.shape[0]] = a
    rls._lib.check(ctx.handle, ctx.lib.rls_memcpy_h2d(ctx.handle, d.ptr, buf.ctypes.data, buf.nbytes), "h2d")
    return d


@pytest.mark.parametrize("dt", DTYPES)
def test_padded_leading_dimension(rls, ctx, dt):
    M, N, K = 64, 48, 3
    pb = problem(M, N, K, np.dtype(dt).name)
    Ad = padded(rls, ctx, pb["A"], M + (2 if cplx(dt) else 4))  # columns stay 16-byte aligned: rls_skinny_ok accepts
    Bd = padded(rls, ctx, pb["B"], M + 3)
    tag = "lda_" + name(dt, M, N, K)
    with tuned(ctx):
        snaps = run_cgnr(rls, Ad, Bd, lam=1e-2, steps=2)
    check_init(tag, pb, snaps[0])
    for k in (1, 2):
        check_product(f"{tag}_step{k}", pb, snaps[k - 1], snaps[k])
        check_update(tag, snaps[k - 1], snaps[k], 1e-2, k)
    assert all(np.isfinite(s[k]).all() for s in snaps for k in "XRPV")


# ---- 9. shapes the matrix-core path refuses still solve, column by column --------------------------------------------------------
def test_refused_shape_falls_back_to_per_column_plans(rls, ctx):
    M, N, K, dt = 72, 40, 3, np.complex64
    A, _, B = O.make_problem(M, N, dt, 53, n_rhs=K)
    B = np.asfortranarray(B)
    B[:, 0] *= 1e-3
    S = rls.createLinearSolver(rls.CGNR, rls.DeviceMatrix.from_host(A, ctx), reg=rls.L2Regularization(1e-3), iterations=12, relTol=0.0)
    xs = rls.solve_(S, rls.DeviceMatrix.from_host(B, ctx), scheduler=rls.BatchedState)
    assert not isinstance(S.state, rls.BatchedState)
    for j in range(K):
        ref = O.CGNR(A.astype(np.complex128), reg=O.L2Regularization(1e-3), iterations=12, relTol=0.0)
        O.solve(ref, B[:, j].astype(np.complex128))
        parity_check(f"skinny_refused_{M}x{N}_col{j}", xs[j].to_host(), ref.x,
                     lambda: O.solve(O.CGNR(A, reg=O.L2Regularization(1e-3), iterations=12, relTol=0.0), np.ascontiguousarray(B[:, j])))


# ---- 10. every shared-A plan sums forced row splits -----------------------------------------------------------------------------
# The per-column kernels of all four batched plans (CGNR; FISTA; cg! under ADMM and SplitBregman; OptISTA / POGM) take AHA u as S
# partial rows per column and add them in one fixed order; the loop of that sum runs only when S > 1, which no shape this small
# reaches on its own.  272 x 32 with S = 3 as in test_v_kernel_row_splits.  K = 3: complex the (8 re | 8 im) half layout (rows 8
# columns apart), real one full group; K = 17: two groups (rows 32 columns apart), the second all padding but one column.
# Gaussian A (condition number about 2), b = A x_true: on the CPU the Float32 oracle of every case below is within 6e-7 of the
# float64 oracle, so the 1e-5 gate holds on its own and the Float32 fallback is not what a case passes by.
SPLIT_FAMILIES = {
    "CGNR": ("CGNR", "CgnrBatchedState", lambda R, lam, rho: dict(reg=R.L2Regularization(1e-2), iterations=5, relTol=0.0)),
    "FISTA": ("FISTA", "FistaBatchedState", lambda R, lam, rho: dict(reg=R.L1Regularization(lam), rho=rho, iterations=5, relTol=0.0)),
    "ADMM": ("ADMM", "AdmmBatchedState", lambda R, lam, rho: dict(reg=R.L1Regularization(0.05), rho=0.3, iterations=3, iterationsCG=4,
                                                                  tolInner=1e-6, absTol=0.0, relTol=0.0)),
    "SplitBregman": ("SplitBregman", "SplitBregmanBatchedState",
                     lambda R, lam, rho: dict(reg=R.L1Regularization(0.05), rho=0.3, iterations=2, iterationsInner=2, iterationsCG=4,
                                              tolInner=1e-6, absTol=0.0, relTol=0.0)),
    "OptISTA": ("OptISTA", "PgmBatchedState", lambda R, lam, rho: dict(reg=R.L1Regularization(lam), rho=rho, iterations=5, relTol=0.0)),
    "POGM": ("POGM", "PgmBatchedState", lambda R, lam, rho: dict(reg=R.L1Regularization(lam), rho=rho, iterations=5, relTol=0.0)),
}


@functools.lru_cache(maxsize=None)
def split_case(family, dtname, K):
    """the problem, the solver's keywords (as a function of the module the regulariser comes from) and per column the float64 and
    the working-precision oracle solutions: computed once per case, never written to"""
    dt = np.dtype(dtname)
    A, _, B = O.make_problem(272, 32, dt, 71, n_rhs=K)
    B = np.asfortranarray(B)
    A64 = A.astype(hi(dt))
    lam = 0.02 * float(np.abs(A64.conj().T @ B[:, 0].astype(hi(dt))).max())
    rho = float(0.9 / np.linalg.norm(A64, 2) ** 2)
    cls, _, kw = SPLIT_FAMILIES[family]
    x64 = [np.array(O.solve(getattr(O, cls)(A64, **kw(O, lam, rho)), B[:, j].astype(hi(dt)))) for j in range(K)]
    x32 = [np.array(O.solve(getattr(O, cls)(A, **kw(O, lam, rho)), np.ascontiguousarray(B[:, j]))) for j in range(K)]
    for a in [A, B] + x64 + x32:
        a.setflags(write=False)
    return A, B, (lambda R: kw(R, lam, rho)), x64, x32


@pytest.mark.parametrize("K", [3, 17])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("family", list(SPLIT_FAMILIES))
def test_every_plan_sums_forced_row_splits(rls, ctx, family, dt, K):
    A, B, kw, x64, x32 = split_case(family, np.dtype(dt).name, K)
    cls, state, _ = SPLIT_FAMILIES[family]
    with tuned(ctx, skinny_v_splits=3):  # read when the plan is created
        S = rls.createLinearSolver(getattr(rls, cls), rls.DeviceMatrix.from_host(A, ctx), **kw(rls))
        xs = rls.solve_(S, rls.DeviceMatrix.from_host(B, ctx), scheduler=rls.BatchedState)
        assert type(S.state).__name__ == state, "the shape must take the shared-A plan"
        got = [x.to_host() for x in xs]
    tag = f"splits_{family}_{name(dt, 272, 32, K)}_S3"
    errs = [rel(got[j], x64[j]) for j in range(K)]
    worst = int(np.argmax(errs))
    print(f"[skinny] {tag}: device {errs[worst]:.3e}  oracle-f32 {rel(x32[worst], x64[worst]):.3e}  (column {worst})")
    for j in range(K):
        parity_check(f"skinny_{tag}_col{j}", got[j], x64[j], x32[j], record=(j == worst))
