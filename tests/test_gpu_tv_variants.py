"""Every code path of the TV proximal map (FGP, csrc/tv.hip; the double-precision kernels of csrc/f64.hip) against the float64
oracle at the edges of its selection rules.  The launcher picks one of six variants from the geometry and two tuning switches
(rls_tv_variant: 0 = two launches per FGP iteration, replayed from a captured graph; 1 = fgp_fused_kernel; 21 / 22 / 24 / 28 =
fgp2d_kernel at 1 / 2 / 4 / 8 pixels per thread); every case asserts the variant it means to test before it compares anything.

Bars (the ones the suite already holds these operations to): gradient and adjoint 1e-6 relative, prox and solver columns
`parity` (1e-5 against the float64 oracle, or twice the Float32 oracle's own error), double precision 1e-12.  The oracle is a
restatement, so every geometry is also held to <G x, g> == <x, G^T g>, evaluated on the host in float64 from the two device
outputs.  Every prox comparison is preceded by two checks on the oracle alone (`oracle_prox`): its output lies more than 100 bars
from its input and from its own output after one FGP iteration fewer, so that neither a no-op nor a dropped or doubled
iteration could pass."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import rls_oracle as O  # noqa: E402  (the checker)
from conftest import parity_check  # noqa: E402  (<= 1e-5 vs float64, or <= 2 x the Float32 oracle's own error)

pytestmark = pytest.mark.gpu
F32, C64 = np.float32, np.complex64
DT = [F32, C64]
DTD = [np.float64, np.complex128]
LAM, ITERS = 0.3, 10
# csrc/tv.hip, struct fgp_graph_cache: `entry entries[8];` -- the captured launch sequences one context keeps
GRAPH_CACHE_ENTRIES = 8


def hi(dt):
    return np.complex128 if np.dtype(dt).kind == "c" else np.float64


def bar(dt):
    return 1e-12 if np.dtype(dt).itemsize // (2 if np.dtype(dt).kind == "c" else 1) == 8 else 1e-5


def rel(a, b):
    a, b = np.asarray(a).astype(np.complex128), np.asarray(b).astype(np.complex128)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def draw(rng, dt, n):
    v = rng.standard_normal(n)
    if np.dtype(dt).kind == "c":
        v = (v + 1j * rng.standard_normal(n)) / math.sqrt(2)
    return v.astype(dt)


def image(dt, shape, seed=0):
    """standard normal, one fixed seed per shape (and `seed` for a second image of the same shape)"""
    n = int(np.prod(shape))
    return draw(np.random.default_rng([n, len(shape), int(shape[0]), seed]), dt, n)


_ORACLE = {}


def oracle_prox(x, lam, shape, dims, iters=ITERS):
    """float64 FGP of x (computed once per input and shared), after the two preconditions of the module docstring"""
    dims = None if dims is None else tuple(dims)
    key = (x.dtype.str, x.tobytes(), float(lam), tuple(shape), dims, iters)
    if key not in _ORACLE:
        x64 = x.astype(hi(x.dtype))
        want = O.prox_tv_fgp(x64.copy(), lam, shape, dims, iters)
        short = O.prox_tv_fgp(x64.copy(), lam, shape, dims, iters - 1)
        _ORACLE[key] = (want, rel(want, x64), rel(short, want))
    want, moved, last_step = _ORACLE[key]
    assert moved > 100 * bar(x.dtype), f"the prox barely moves this input ({moved:.2e}): pick another seed or lambda"
    assert last_step > 100 * bar(x.dtype), f"the last FGP iteration changes too little ({last_step:.2e}): pick another seed or lambda"
    return want


def oracle32(x, lam, shape, dims, iters=ITERS):
    return lambda: O.prox_tv_fgp(x.copy(), lam, shape, dims, iters)


@pytest.fixture(scope="module")
def rls():
    import rls_amd
    return rls_amd


@pytest.fixture(scope="module")
def ctx(rls):
    return rls.default_context(0)


def variant(rls, ctx, dt, shape, dims):
    """the launcher's own selector, under the context's current tuning"""
    from rls_amd.arrays import dtype_code
    from rls_amd.regularization import _tv_geometry
    shape, d0, cs, cd = _tv_geometry(shape, dims)
    return ctx.lib.rls_tv_variant(ctx.handle, dtype_code(dt), len(shape), cs, len(d0), cd)


def check_prox(rls, ctx, dt, shape, dims, expect, tag, lam=LAM):
    """variant, then prox against the float64 oracle; returns the error"""
    got_variant = variant(rls, ctx, dt, shape, dims)
    assert got_variant == expect, f"{tag}: the launcher takes variant {got_variant}, this case is about {expect}"
    x = image(dt, shape)
    want = oracle_prox(x, lam, shape, dims)
    got = rls.prox_(rls.TVRegularization, rls.DeviceVector.from_host(x, ctx), lam, shape=shape, dims=dims).to_host()
    e = parity_check(tag, got, want, oracle32(x, lam, shape, dims), record=False)
    print(f"{tag}: variant {got_variant} prox error {e:.3e}")
    return e


def check_gradient(rls, ctx, dt, shape, dims, tag):
    """G x and G^T g against the oracle at 1e-6, and <G x, g> == <x, G^T g> from the device outputs alone.
    The identity is held to 1e-6 of the inner product itself; g is redrawn (on the host, before any device call) until the exact
    inner product is at least a quarter of its typical size ||(G x) .* g||, so that the relative bar is not met by cancellation."""
    n = int(np.prod(shape))
    d0 = O._as_dims(shape, dims)
    x = image(dt, shape)
    u64 = O.grad_apply(x.astype(hi(dt)), shape, d0)
    G = rls.GradientOp(shape, dims)
    assert G.n_out == O.grad_len(shape, d0) == u64.size
    g = a64 = None
    for seed in range(1, 9):
        g = image(dt, (G.n_out,), seed)
        a64 = np.vdot(u64, g.astype(hi(dt)))
        if abs(a64) >= 0.25 * np.linalg.norm(u64 * g):
            break
    assert abs(a64) >= 0.25 * np.linalg.norm(u64 * g), "no draw of g gives an inner product of typical size"
    gx = G.mul(rls.DeviceVector.from_host(x, ctx)).to_host()
    e_g = rel(gx, u64)
    back = rls.DeviceVector(n, dt, ctx)
    G.mul_adj_(back, rls.DeviceVector.from_host(g, ctx))
    gtg = back.to_host()
    e_t = rel(gtg, O.grad_apply_t(g.astype(hi(dt)), shape, d0))
    lhs = np.vdot(gx.astype(hi(dt)), g.astype(hi(dt)))
    rhs = np.vdot(x.astype(hi(dt)), gtg.astype(hi(dt)))
    e_a = abs(lhs - rhs) / max(abs(lhs), abs(rhs))
    print(f"{tag}: gradient {e_g:.3e} adjoint {e_t:.3e} <Gx,g> vs <x,G'g> {e_a:.3e}")
    assert e_g < 1e-6 and e_t < 1e-6, (tag, e_g, e_t)
    assert e_a < 1e-6, (tag, lhs, rhs, e_a)


# ---- 1. fgp2d_kernel at every boundary of its pixel-count ladder -------------------------------------------------------------
# (shape, dims, variant for Float32, variant for ComplexF32)
CASES_2D = [((32, 32), None, 21, 21),      # 1024: the last image at one pixel per thread
            ((25, 41), None, 22, 22),      # 1025: 576 threads, 127 of them own one pixel only
            ((64, 32), None, 22, 22),      # 2048
            ((3, 683), None, 24, 24),      # 2049: 576 threads, the last 255 own three pixels
            ((17, 241), None, 28, 0),      # 4097: Float32 moves to 8 pixels per thread, ComplexF32 leaves the kernel
            ((3, 2731), None, 0, 0),       # 8193
            ((25, 41), (1,), 22, 22), ((25, 41), (2,), 22, 22),
            ((1, 1500), None, 22, 22), ((1500, 1), None, 22, 22), ((2, 700), None, 22, 22)]  # an empty / a one-row gradient block


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("shape,dims,v32,v64", CASES_2D)
def test_register_resident_kernel_at_its_boundaries(rls, ctx, dt, shape, dims, v32, v64):
    tag = f"tv2d_{np.dtype(dt).name}_{shape}_{dims}"
    check_prox(rls, ctx, dt, shape, dims, v32 if dt is F32 else v64, tag)
    check_gradient(rls, ctx, dt, shape, dims, tag)


# ---- 2. fgp_fused_kernel above one pixel per thread ----------------------------------------------------------------------------
CASES_FUSED = [((12, 12, 12), None, 1),       # 1728 pixels: 704 threads own two
               ((16, 16, 8), None, 1),        # 2048 == tv_fused_max_n
               ((6, 6, 6, 6), None, 1), ((6, 6, 6, 6), (1, 3), 1),
               ((40, 50), (2, 1), 1),         # not the natural order: the 2-D kernel refuses
               ((1, 40, 40), None, 1), ((40, 1, 40), None, 1),
               ((13, 13, 13), None, 0)]       # 2197 > tv_fused_max_n


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("shape,dims,expect", CASES_FUSED)
def test_lds_resident_kernel_above_one_pixel_per_thread(rls, ctx, dt, shape, dims, expect):
    tag = f"tvfused_{np.dtype(dt).name}_{shape}_{dims}"
    check_prox(rls, ctx, dt, shape, dims, expect, tag)
    check_gradient(rls, ctx, dt, shape, dims, tag)


# ---- 3. three routes, one image (includes case 2's (64, 32) with tv_fused_2d = 0) ---------------------------------------------
@pytest.mark.parametrize("dt", DT)
def test_three_routes_one_image(rls, ctx, dt):
    shape = (64, 32)
    seen = []
    try:
        for tune, expect in (({}, 22), ({"tv_fused_2d": 0}, 1), ({"tv_fused_2d": 0, "tv_fused_max_n": 16}, 0)):
            ctx.tune(**tune)
            check_prox(rls, ctx, dt, shape, None, expect, f"tvroutes_{np.dtype(dt).name}_{expect}")
            seen.append(variant(rls, ctx, dt, shape, None))
    finally:
        ctx.tune(tv_fused_2d=1, tv_fused_max_n=2048)
    assert len(set(seen)) == 3, seen
    assert variant(rls, ctx, dt, shape, None) == 22


# ---- 4. the multi-launch path: graph replay, recapture, eviction, and the eager launches ---------------------------------------
def _multi_launch_sequence(rls, ctx, dt, shape, use_graph):
    """one device buffer, one workspace (the regulariser instance keeps it): [(image, lambda, result), ...]"""
    first, second = image(dt, shape), image(dt, shape, seed=1)
    lams = [LAM + 0.02 * k for k in range(GRAPH_CACHE_ENTRIES + 1)]   # more keys than the cache holds; lams[0] == LAM
    plan = [(first, LAM),        # captured (use_graph = 1)
            (second, LAM),       # replayed: must read the buffer's new contents
            (second, 0.2)]       # a new key
    plan += [(first, l) for l in lams]   # fills the cache and evicts
    plan += [(first, LAM)]               # the first key again: evicted by now, captured afresh
    out = []
    ctx.tune(use_graph=use_graph)
    try:
        reg = rls.TVRegularization(LAM, shape=shape, iterationsTV=ITERS)
        xd = rls.DeviceVector(first.size, dt, ctx)
        ws = None
        for img, lam in plan:
            xd.copy_from_host(img)
            reg.prox_(xd, lam)
            assert ws is None or reg._ws is ws, "the workspace must stay the same buffer"
            ws = reg._ws
            out.append((img, lam, xd.to_host()))
    finally:
        ctx.tune(use_graph=1)
    return out


@pytest.mark.parametrize("dt,shape", [(F32, (13, 13, 13)), (C64, (17, 241))])
def test_multi_launch_replay_recapture_and_eviction(rls, ctx, dt, shape):
    assert variant(rls, ctx, dt, shape, None) == 0
    runs = {g: _multi_launch_sequence(rls, ctx, dt, shape, g) for g in (1, 0)}
    worst = 0.0
    for g, seq in runs.items():
        for k, (img, lam, got) in enumerate(seq):
            want = oracle_prox(img, lam, shape, None)
            worst = max(worst, parity_check(f"tvmulti_{np.dtype(dt).name}_{shape}_graph{g}_call{k}", got, want,
                                            oracle32(img, lam, shape, None), record=False))
    print(f"tvmulti_{np.dtype(dt).name}_{shape}: variant 0, worst prox error over {len(runs[1])} calls x 2 modes {worst:.3e}")
    # the same kernels with the same arguments in the same order, replayed or launched one by one
    for k, ((_, _, a), (_, _, b)) in enumerate(zip(runs[1], runs[0])):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"call {k}: the replayed graph and the eager launches differ"


def test_grid_stride_loops_wrap(rls, ctx):
    """(1024, 513) = 525,312 pixels, 1,049,087 gradient entries: the first size past the 2048 x 256 threads of tv_grid"""
    shape = (1024, 513)
    assert int(np.prod(shape)) > 2048 * 256
    check_prox(rls, ctx, F32, shape, None, 0, "tvwrap_float32")
    check_gradient(rls, ctx, F32, shape, None, "tvwrap_float32")


# ---- 5. iterationsTV = 0 returns the input ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("shape,v32,v64", [((32, 32), 21, 21), ((25, 41), 22, 22), ((3, 683), 24, 24), ((17, 241), 28, 0),
                                           ((12, 12, 12), 1, 1), ((13, 13, 13), 0, 0)])
def test_zero_iterations_return_the_input_bit_for_bit(rls, ctx, dt, shape, v32, v64):
    assert variant(rls, ctx, dt, shape, None) == (v32 if dt is F32 else v64)
    x = image(dt, shape)
    x[:2] = [0.0, -0.0]   # (x - lambda * grad^T 0 keeps the sign of a zero)
    got = rls.prox_(rls.TVRegularization, rls.DeviceVector.from_host(x, ctx), LAM, shape=shape, iterationsTV=0).to_host()
    assert np.array_equal(got.view(np.uint32), x.view(np.uint32))


# ---- 6. the double-precision kernels at the degenerate geometries and past the grid cap -------------------------------------------
@pytest.mark.parametrize("dt", DTD)
@pytest.mark.parametrize("shape", [(1, 1500), (2, 700), (1, 40, 40), (1024, 513)])
def test_double_precision_kernels(rls, ctx, dt, shape):
    assert variant(rls, ctx, dt, shape, None) == -1   # RLS_E_INVALID: the selector is about the Float32 / ComplexF32 kernels
    x = image(dt, shape)
    want = oracle_prox(x, LAM, shape, None)
    got = rls.prox_(rls.TVRegularization, rls.DeviceVector.from_host(x, ctx), LAM, shape=shape).to_host()
    e = rel(got, want)
    print(f"tvdouble_{np.dtype(dt).name}_{shape}: prox error {e:.3e}")
    assert got.dtype == np.dtype(dt) and e < 1e-12, e


# ---- 7. several columns per launch --------------------------------------------------------------------------------------------------
# The one caller of the single-workgroup kernels with count > 1 is the batched ADMM plan (csrc/solvers.hip, admm_step_impl:
# rls_tv_single_launch(..., K, ldv, skip_stride)); it needs M and N to be multiples of 16.  Batched FISTA keeps TV regularisers out of
# its shared-A plan and SplitBregman has none, so both solve matrix right-hand sides column by column -- asserted below.
K_RHS, OUTER = 3, 6


def _problem(dt, shape):
    N = int(np.prod(shape))
    M = N + 64
    A, _, B = O.make_problem(M, N, dt, 1000 + N, n_rhs=K_RHS)
    B = np.asfortranarray(B)
    B[:, 1] *= 1e-3
    return A, B.astype(dt), M, N


def _columns_against_oracle(tag, xs, make_oracle, A, B, dt, iterations=None):
    worst = 0.0
    for j in range(K_RHS):
        kw = {} if iterations is None else dict(iterations=iterations[j])
        x64 = np.array(O.solve(make_oracle(A.astype(hi(dt)), **kw), B[:, j].astype(hi(dt))))
        x32 = (lambda j=j, kw=kw: np.array(O.solve(make_oracle(A, **kw), np.ascontiguousarray(B[:, j]))))
        worst = max(worst, parity_check(f"{tag}_col{j}", xs[j].to_host(), x64, x32, record=False))
    print(f"{tag}: worst column error {worst:.3e}")


@pytest.mark.parametrize("dt,shape,batched,expect", [(F32, (25, 41), False, 22), (C64, (25, 41), False, 22), (F32, (12, 12, 12), True, 1),
                                                     (C64, (12, 12, 12), True, 1), (F32, (32, 33), True, 22), (C64, (32, 33), True, 22)])
def test_admm_tv_columns(rls, ctx, dt, shape, batched, expect):
    """ADMM + TV on K = 3 right-hand sides through the shared-A scheduler.  M = N + 64; (25, 41) has N = 1025, not a multiple of
    16, so the batched plan refuses and the columns run one by one; (12, 12, 12) and (32, 33) (N = 1056: two pixels per thread)
    run the FGP kernels with one workgroup per column.  Column 1 is a thousand times smaller: absTol is chosen from the oracle's
    own history so that it alone stops early (after its first iteration) -- its skip flag is set while the other two workgroups go on."""
    assert variant(rls, ctx, dt, shape, None) == expect
    A, B, M, N = _problem(dt, shape)
    kw = dict(rho=0.3, iterations=OUTER, iterationsCG=5, tolInner=1e-5, relTol=0.0)
    regs = lambda R: R.TVRegularization(2e-2, shape=shape)
    # history of max(rk, sk) per column with the stopping rule off (float64 oracle), then a threshold sigma_abs = sqrt(M) absTol
    # that column 1 meets and the other columns never meet while it matters
    hist = []
    for j in range(K_RHS):
        o = O.ADMM(A.astype(hi(dt)), reg=regs(O), absTol=0.0, **kw)
        o.init(B[:, j].astype(hi(dt)))
        h = []
        while o.iterate() is not None:
            h.append(max(float(o.rk[0]), float(o.sk[0])))
        hist.append(h)
    # (the small column is dominated by the TV term: its residuals start a factor of ten below anything the others reach and stay
    #  there, so it meets the threshold after its first iteration; a value of the last iteration is never tested)
    below, above = hist[1][0], min(hist[0][:OUTER - 1] + hist[2][:OUTER - 1])
    assert below < 0.5 * above, (hist, "column 1 must cross a threshold that nothing else crosses")
    absTol = math.sqrt(below * above) / math.sqrt(M)
    S = rls.createLinearSolver(rls.ADMM, rls.DeviceMatrix.from_host(A, ctx), reg=regs(rls), absTol=absTol, **kw)
    xs = rls.solve_(S, rls.DeviceMatrix.from_host(B, ctx), scheduler=rls.BatchedState)
    assert type(S.state).__name__ == ("AdmmBatchedState" if batched else "MultiThreadingState")
    its = [s.iteration for s in (S.state.status() if batched else S.state.states)]
    assert its == [OUTER, 1, OUTER], its   # exactly one column retired early
    _columns_against_oracle(f"tvcols_admm_{np.dtype(dt).name}_{shape}", xs, lambda A_, **o: O.ADMM(A_, reg=regs(O), **dict(kw, absTol=0.0, **o)),
                            A, B, dt, iterations=its)


@pytest.mark.parametrize("dt,shape,expect", [(F32, (25, 41), 22), (C64, (25, 41), 22), (F32, (12, 12, 12), 1), (C64, (12, 12, 12), 1)])
def test_fista_tv_columns_run_one_by_one(rls, ctx, dt, shape, expect):
    """FISTA + TV on a matrix right-hand side: the shared-A plan does not take TV, every column runs its own plan with the FGP
    launch inside (count = 1).  relTol from the oracle's own residual history: one column alone stops early, the launches behind
    its `done` flag are skipped."""
    assert variant(rls, ctx, dt, shape, None) == expect
    A, B, M, N = _problem(dt, shape)
    rho = 0.9 / (math.sqrt(M) + math.sqrt(N)) ** 2 / 1.05   # (sigma_max of a Gaussian matrix is sqrt(M) + sqrt(N) to a per cent)
    lam = 0.02 * float(np.max(np.abs(A.astype(hi(dt)).conj().T @ B[:, 0].astype(hi(dt)))))
    regs = lambda R: R.TVRegularization(lam, shape=shape)
    kw = dict(rho=rho, iterations=OUTER)
    hist = []
    for j in range(K_RHS):
        o = O.FISTA(A.astype(hi(dt)), reg=regs(O), relTol=0.0, **kw)
        o.init(B[:, j].astype(hi(dt)))
        h = []
        while o.iterate() is not None:
            h.append(float(o.rel_res_norm))
        hist.append(h)
    # rel_res_norm of iteration k + 1 (hist[j][k]) is tested before iteration k + 2.  The small column is dominated by the TV term and
    # stalls; the other two fall at nearly the same rate, so the one column that can stop alone is the one that is lowest before
    # the last iteration: it is spared that iteration, the other two run all of them.  0.99: the device's Float32 rel_res_norm is
    # within 1e-4 of the oracle's
    k = OUTER - 2
    j = int(np.argmin([h[k] for h in hist]))
    below = hist[j][k]
    above = min(hist[j][:k] + [v for i in range(K_RHS) if i != j for v in hist[i][:OUTER - 1]])
    assert below < 0.99 * above, (hist, "one column must cross a threshold that nothing else crosses")
    tol = math.sqrt(below * above)
    want_its = [OUTER - 1 if i == j else OUTER for i in range(K_RHS)]
    S = rls.createLinearSolver(rls.FISTA, rls.DeviceMatrix.from_host(A, ctx), reg=regs(rls), relTol=tol, **kw)
    xs = rls.solve_(S, rls.DeviceMatrix.from_host(B, ctx), scheduler=rls.BatchedState)
    assert type(S.state).__name__ == "MultiThreadingState" and all(s._plan for s in S.state.states)
    its = [s.iteration for s in S.state.states]
    assert its == want_its, (its, want_its)
    _columns_against_oracle(f"tvcols_fista_{np.dtype(dt).name}_{shape}", xs, lambda A_, **o: O.FISTA(A_, reg=regs(O), relTol=0.0, **dict(kw, **o)),
                            A, B, dt, iterations=its)


@pytest.mark.parametrize("dt,shape,expect", [(F32, (25, 41), 22), (C64, (25, 41), 22), (F32, (12, 12, 12), 1), (C64, (12, 12, 12), 1)])
def test_split_bregman_tv_columns_run_one_by_one(rls, ctx, dt, shape, expect):
    """SplitBregman + TV on a matrix right-hand side: no shared-A plan, every column runs its own ADMM-style device plan with the
    FGP launch inside (count = 1); 6 outer iterations of 2 inner ones, the stopping rule off (SplitBregman's `converged` starts a
    Bregman update instead of retiring the column)."""
    assert variant(rls, ctx, dt, shape, None) == expect
    A, B, M, N = _problem(dt, shape)
    kw = dict(rho=0.3, iterations=OUTER, iterationsInner=2, iterationsCG=5, tolInner=1e-5, absTol=0.0, relTol=0.0)
    regs = lambda R: R.TVRegularization(2e-2, shape=shape)
    S = rls.createLinearSolver(rls.SplitBregman, rls.DeviceMatrix.from_host(A, ctx), reg=regs(rls), **kw)
    xs = rls.solve_(S, rls.DeviceMatrix.from_host(B, ctx), scheduler=rls.BatchedState)
    assert type(S.state).__name__ == "MultiThreadingState"
    _columns_against_oracle(f"tvcols_splitbregman_{np.dtype(dt).name}_{shape}", xs, lambda A_: O.SplitBregman(A_, reg=regs(O), **kw), A, B, dt)
