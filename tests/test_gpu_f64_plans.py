"""Float64 / ComplexF64 CGNR and FISTA as device plans (rls_cgnr_*_d, rls_fista_*_d; csrc/plans_f64.hip): the plan is taken and the
host is out of the loop, iterates and status scalars against the float64 oracle (1e-12 relative, 1e-11 in Gram mode: the bars of
test_gpu_float64.py; status scalars at that file's 1e-10), the same semantics as the primitive loops (use_device_plan_f64 = False),
bit reproducibility, and the fallbacks."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import rls_oracle as O  # noqa: E402  (the checker)

pytestmark = pytest.mark.gpu
DT = [np.float64, np.complex128]
PRIMS = ("rls_nrm2_d", "rls_dotc_d", "rls_asum_d", "rls_gemv_d", "rls_axpy_d")
SCALAR_TOL = 1e-10   # alpha, beta, zeta, residual, theta, rel_res_norm: the bar test_gpu_float64.py holds alphal to
ITER_TOL = 1e-12     # iterates against the float64 oracle ...
GRAM_TOL = 1e-11     # ... and in Gram mode (the bars of test_gpu_float64.py; test_gpu_warm_start.py imports the three)


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300))


def close(a, b, tol=SCALAR_TOL):
    return abs(complex(a) - complex(b)) <= tol * max(abs(complex(b)), 1e-300)


def upload_padded(rls, ctx, A, pad):
    """A on the device with leading dimension M + pad (the padding rows hold NaN: nothing may read them)"""
    M, N = A.shape
    Ad = rls.DeviceMatrix(M, N, A.dtype, ctx, lda=M + pad)
    host = np.full((M + pad, N), np.nan, dtype=A.dtype, order="F")
    host[:M, :] = A
    st = ctx.lib.rls_memcpy_h2d(ctx.handle, Ad.ptr, host.ctypes.data, host.nbytes)
    assert st == 0
    return Ad


class Counter:
    """counting proxies on the context's double-precision primitives, armed once init_ has returned"""

    def __init__(self, lib):
        self.lib, self.armed, self.calls = lib, False, {}
        self.orig = {n: getattr(lib, n) for n in PRIMS}

    def __enter__(self):
        for n, f in self.orig.items():
            def proxy(*a, _n=n, _f=f):
                if self.armed:
                    self.calls[_n] = self.calls.get(_n, 0) + 1
                return _f(*a)
            setattr(self.lib, n, proxy)
        return self

    def __exit__(self, *exc):
        for n, f in self.orig.items():
            setattr(self.lib, n, f)

    def arm_after_init(self, solver):
        orig = solver.init_

        def init_then_arm(*a, **k):
            r = orig(*a, **k)
            self.armed = True
            return r
        solver.init_ = init_then_arm

    @property
    def total(self):
        return sum(self.calls.values())


def plan_path(rls, ctx, S):
    st = S.state
    assert st._plan, "no device plan was created"
    path = C.c_int32(-1)
    fn = ctx.lib.rls_cgnr_path_d if isinstance(S, rls.CGNR) else ctx.lib.rls_fista_path_d
    assert fn(st._plan, C.byref(path)) == 0
    return path.value


def problem(dt, M, N, seed):
    A, xt, b = O.make_problem(M, N, dt, seed)
    rho = 0.9 / np.linalg.norm(A, 2) ** 2
    lam1 = 0.02 * float(np.max(np.abs(A.conj().T @ b)))
    return A, b, rho, lam1


def fista_cases(R, lam1):
    """(name, regulariser list) -- L1 / L2 / L21 / none, with and without a projection"""
    return [("l1", [R.L1Regularization(lam1)]), ("l2", [R.L2Regularization(0.3)]), ("l21", [R.L21Regularization(lam1, slices=4)]),
            ("none", [R.L1Regularization(0.0)]), ("l1+pos", [R.L1Regularization(lam1), R.PositiveRegularization()]),
            ("l2+real", [R.L2Regularization(0.3), R.RealRegularization()]), ("l21+pos", [R.L21Regularization(lam1, slices=4), R.PositiveRegularization()])]


@pytest.mark.parametrize("dt", DT)
def test_plan_is_taken_and_host_is_out_of_the_loop(rls, ctx, dt):
    """solve_ without callbacks: no rls_nrm2_d / dotc_d / asum_d / gemv_d / axpy_d between init_ returning and the solution"""
    A, b, rho, lam1 = problem(dt, 96, 40, 3)
    Ad, bd = rls.DeviceMatrix.from_host(A, ctx), rls.DeviceVector.from_host(b, ctx)
    G = np.asfortranarray(A.conj().T @ A)
    Gd = rls.DeviceMatrix.from_host(G, ctx)
    solvers = []
    for lam in (0.0, 1e-2):
        solvers.append((f"cgnr lam={lam}", lambda lam=lam: rls.createLinearSolver(rls.CGNR, Ad, reg=rls.L2Regularization(lam), iterations=12, relTol=0.0),
                        lambda lam=lam: O.CGNR(A, reg=O.L2Regularization(lam), iterations=12, relTol=0.0), 0))
    solvers.append(("cgnr gram", lambda: rls.createLinearSolver(rls.CGNR, Ad, AHA=Gd, iterations=12, relTol=0.0),
                    lambda: O.CGNR(A, AHA=G, iterations=12, relTol=0.0), 2))
    for restart in ("none", "gradient"):
        for (name, regs), (_, oregs) in zip(fista_cases(rls, lam1), fista_cases(O, lam1)):
            kw = dict(rho=rho, iterations=15, relTol=0.0, restart=restart)
            solvers.append((f"fista {name} {restart}", lambda regs=regs, kw=kw: rls.createLinearSolver(rls.FISTA, Ad, reg=regs, **kw),
                            lambda oregs=oregs, kw=kw: O.FISTA(A, reg=oregs, **kw), 0))
    solvers.append(("fista gram l1", lambda: rls.createLinearSolver(rls.FISTA, Ad, AHA=Gd, reg=rls.L1Regularization(lam1), rho=rho, iterations=15, relTol=0.0),
                    lambda: O.FISTA(A, AHA=G, reg=O.L1Regularization(lam1), rho=rho, iterations=15, relTol=0.0), 2))
    for name, mk, mk_ref, want_path in solvers:
        S, ref = mk(), mk_ref()
        O.solve(ref, b)
        with Counter(ctx.lib) as cnt:
            cnt.arm_after_init(S)
            x = rls.solve_(S, bd).to_host()
        assert cnt.total == 0, (name, cnt.calls)
        assert plan_path(rls, ctx, S) in ((0, 1) if want_path == 0 else (2,)), name
        assert S.state.iteration == ref.iteration, name
        assert rel(x, ref.x) < (1e-11 if want_path == 2 else 1e-12), (name, rel(x, ref.x))


SHAPES = [("64x32", 64, 32, 0, False), ("96x40", 96, 40, 0, False), ("257x130 lda=M+3", 257, 130, 3, False), ("gram only", 96, 40, 0, True)]


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_parity_of_iterates_and_status_scalars(rls, ctx, dt, shape):
    """iterates at iterations 1, 5, 10 and at the end, and alpha / beta / zeta / residual / theta / rel_res_norm there"""
    _, M, N, pad, gram_only = shape
    A, b, rho, lam1 = problem(dt, M, N, 21)
    tol = GRAM_TOL if gram_only else ITER_TOL
    if gram_only:
        G = np.asfortranarray(A.conj().T @ A)
        rhs = A.conj().T @ b
        Ad, Gd = None, rls.DeviceMatrix.from_host(G, ctx)
        o_kw, d_kw, oA = dict(AHA=G), dict(AHA=Gd), None
    else:
        rhs = b
        Ad = upload_padded(rls, ctx, A, pad) if pad else rls.DeviceMatrix.from_host(A, ctx)
        o_kw, d_kw, oA = {}, {}, A
    bd = rls.DeviceVector.from_host(rhs, ctx)
    watch = (1, 5, 10)

    def run(S, ref, scalars):
        seen_ref, seen = {}, {}
        O.solve(ref, rhs, callbacks=lambda sv, i: seen_ref.__setitem__(i, (sv.x.copy(), scalars(sv, True))))
        x = rls.solve_(S, bd, callbacks=lambda sv, i: seen.__setitem__(i, (rls.solversolution(sv).to_host(), scalars(sv, False)))).to_host()
        assert sorted(seen) == sorted(seen_ref)
        last = max(seen_ref)
        for i in watch + (last,):
            assert rel(seen[i][0], seen_ref[i][0]) < tol, (i, rel(seen[i][0], seen_ref[i][0]))
            for name, got, want in zip(scalars.names, seen[i][1], seen_ref[i][1]):
                assert close(got, want), (i, name, got, want)
        assert rel(x, ref.x) < tol
        assert S.state._plan and plan_path(rls, ctx, S) == (2 if gram_only else 0)

    def cg_scalars(s, is_ref):
        if is_ref:
            return (s.alpha, s.beta, s.zeta, s.convergence()["residual"])
        res = rls.solverconvergence(s)["residual"]   # (reads the plan's record)
        return (s.state.alphal, s.state.betal, s.state.zetal, res)
    cg_scalars.names = ("alpha", "beta", "zeta", "residual")

    def fi_scalars(s, is_ref):
        if is_ref:
            return (s.theta, s.rel_res_norm, s.convergence()["residual"])
        res = rls.solverconvergence(s)["residual"]
        return (s.state.theta, s.state.rel_res_norm, res)
    fi_scalars.names = ("theta", "rel_res_norm", "residual")

    for lam in (0.0, 1e-2):
        run(rls.createLinearSolver(rls.CGNR, Ad, reg=rls.L2Regularization(lam), iterations=14, relTol=0.0, **d_kw),
            O.CGNR(oA, reg=O.L2Regularization(lam), iterations=14, relTol=0.0, **o_kw), cg_scalars)
    for restart in ("none", "gradient"):
        for (name, regs), (_, oregs) in zip(fista_cases(rls, lam1), fista_cases(O, lam1)):
            kw = dict(rho=rho, iterations=14, relTol=0.0, restart=restart)
            run(rls.createLinearSolver(rls.FISTA, Ad, reg=regs, **kw, **d_kw), O.FISTA(oA, reg=oregs, **kw, **o_kw), fi_scalars)


def _early_tols(A, b, rho, lam1):
    """a relTol that stops CGNR at iteration 3 of 10, and one that stops FISTA + L1 at the first iteration k >= 3 whose
    rel_res_norm is a new minimum -- both taken from the oracle's own sequences"""
    ratios = {}
    ref = O.CGNR(A, iterations=10, relTol=0.0)
    O.solve(ref, b, callbacks=lambda sv, i: ratios.__setitem__(i, float(sv.convergence()["residual"] / sv.z0)))
    cg_tol = math.sqrt(ratios[3] * ratios[2])
    assert ratios[3] < cg_tol < min(ratios[i] for i in range(3))
    rels = {}
    ref = O.FISTA(A, reg=O.L1Regularization(lam1), rho=rho, iterations=30, relTol=0.0)
    O.solve(ref, b, callbacks=lambda sv, i: rels.__setitem__(i, float(sv.rel_res_norm)))
    k = next(i for i in range(3, 30) if rels[i] < min(rels[j] for j in range(1, i)))
    fi_tol = math.sqrt(rels[k] * min(rels[j] for j in range(1, k)))
    return cg_tol, fi_tol, k


@pytest.mark.parametrize("dt", DT)
def test_same_semantics_as_the_primitive_path(rls, ctx, dt):
    """plan and use_device_plan_f64 = False agree on iteration count, done, callback cadence and convergence values; solutions
    to 1e-12; early stop by relTol; steps after done are no-ops; iterations > N stops CGNR at N"""
    M, N = 96, 40
    A, b, rho, lam1 = problem(dt, M, N, 8)
    Ad, bd = rls.DeviceMatrix.from_host(A, ctx), rls.DeviceVector.from_host(b, ctx)
    cg_tol, fi_tol, k_fista = _early_tols(A, b, rho, lam1)
    cases = [("cgnr", lambda: rls.createLinearSolver(rls.CGNR, Ad, reg=rls.L2Regularization(1e-2), iterations=12, relTol=0.0), None),
             ("cgnr early", lambda: rls.createLinearSolver(rls.CGNR, Ad, iterations=10, relTol=cg_tol), 3),
             ("cgnr iterations > N", lambda: rls.createLinearSolver(rls.CGNR, Ad, iterations=3 * N, relTol=0.0), N),
             ("fista early", lambda: rls.createLinearSolver(rls.FISTA, Ad, reg=rls.L1Regularization(lam1), rho=rho, iterations=30, relTol=fi_tol), k_fista)]
    for restart in ("none", "gradient"):
        for name, regs in fista_cases(rls, lam1):
            cases.append((f"fista {name} {restart}", lambda regs=regs, restart=restart: rls.createLinearSolver(
                rls.FISTA, Ad, reg=regs, rho=rho, iterations=12, relTol=0.0, restart=restart), None))
    for name, mk, stop_at in cases:
        out = {}
        for plan in (True, False):
            S = mk()
            S.use_device_plan_f64 = plan
            seen = []
            x = rls.solve_(S, bd, callbacks=lambda sv, i: seen.append((i, float(rls.solverconvergence(sv)["residual"])))).to_host()
            assert bool(S.state._plan) == plan, name
            again = rls.iterate(S)   # done: a further iterate returns None and changes nothing
            out[plan] = (x, S.state.iteration, seen, again, S.state._done, S)
        (xp, itp, seenp, againp, donep, Sp), (xq, itq, seenq, againq, doneq, _) = out[True], out[False]
        assert itp == itq and againp is None and againq is None and donep, (name, itp, itq)
        assert [i for i, _ in seenp] == [i for i, _ in seenq] == list(range(itp + 1)), name
        if stop_at is not None:
            assert itp == stop_at, (name, itp, stop_at)
        if name != "cgnr iterations > N":   # (iterates past convergence are rounding noise over rounding noise)
            for (i, rp), (_, rq) in zip(seenp, seenq):
                assert rp == rq or close(rp, rq), (name, i, rp, rq)
            assert rel(xp, xq) < 1e-12, (name, rel(xp, xq))
        # further step calls after done leave x bit-identical
        step = ctx.lib.rls_cgnr_step_d if name.startswith("cgnr") else ctx.lib.rls_fista_step_d
        assert step(Sp.state._plan, 3) == 0
        ctx.sync()
        assert rls.solversolution(Sp).to_host().tobytes() == xp.tobytes(), name
        # and without callbacks (one step_status_d for the whole solve) the same iteration count and bits as under callbacks
        S2 = mk()
        x2 = rls.solve_(S2, bd).to_host()
        assert S2.state.iteration == itp and x2.tobytes() == xp.tobytes(), name


@pytest.mark.parametrize("dt", DT)
def test_bit_reproducibility(rls, ctx, dt):
    A, b, rho, lam1 = problem(dt, 257, 130, 5)
    Ad, bd = upload_padded(rls, ctx, A, 3), rls.DeviceVector.from_host(b, ctx)
    for mk in (lambda: rls.createLinearSolver(rls.CGNR, Ad, reg=rls.L2Regularization(1e-3), iterations=20, relTol=0.0),
               lambda: rls.createLinearSolver(rls.FISTA, Ad, reg=rls.L1Regularization(lam1), rho=rho, iterations=20, relTol=0.0, restart="gradient")):
        runs = [rls.solve_(mk(), bd).to_host().tobytes() for _ in range(2)]
        assert runs[0] == runs[1]
        S = mk()   # and the same solver object solved twice
        assert rls.solve_(S, bd).to_host().tobytes() == runs[0] and rls.solve_(S, bd).to_host().tobytes() == runs[0]


# the primitive path's own error against the complex128 oracle at 4096 x 2048, 32 iterations, measured once on an MI355X
# (tools/bench_f64_plans.py writes the figures into profiles/f64_plans.txt)
PRIMITIVE_ERROR_FULL = {"cgnr": 2.700e-15, "fista": 1.856e-15}


def test_full_size_complexf64(rls, ctx):
    """4096 x 2048 ComplexF64, CGNR and FISTA + L1, 32 iterations, against the complex128 oracle.  Gate: max(1e-12, 4 x the
    primitive path's own error at this shape) -- both paths sum in double and differ only in summation order.
    Measured on an MI355X: primitives 2.700e-15 (CGNR) and 1.856e-15 (FISTA + L1), the plans 2.768e-15 and 1.903e-15; four times
    the yardstick is below 1e-12, so the gate is 1e-12 for both (profiles/f64_plans.txt)."""
    M, N = 4096, 2048
    A, xt, b = O.make_problem(M, N, np.complex128, 4)
    Ad, bd = rls.DeviceMatrix.from_host(A, ctx), rls.DeviceVector.from_host(b, ctx)
    rho = 0.9 / np.linalg.norm(A, 2) ** 2
    lam1 = 0.02 * float(np.max(np.abs(A.conj().T @ b)))
    refs = {"cgnr": O.CGNR(A, reg=O.L2Regularization(1e-3), iterations=32, relTol=0.0),
            "fista": O.FISTA(A, reg=O.L1Regularization(lam1), rho=rho, iterations=32, relTol=0.0)}
    mks = {"cgnr": lambda: rls.createLinearSolver(rls.CGNR, Ad, reg=rls.L2Regularization(1e-3), iterations=32, relTol=0.0),
           "fista": lambda: rls.createLinearSolver(rls.FISTA, Ad, reg=rls.L1Regularization(lam1), rho=rho, iterations=32, relTol=0.0)}
    errs = {}
    for name in ("cgnr", "fista"):
        O.solve(refs[name], b)
        for plan in (False, True):
            S = mks[name]()
            S.use_device_plan_f64 = plan
            x = rls.solve_(S, bd).to_host()
            assert S.state.iteration == 32 and bool(S.state._plan) == plan
            errs[name, plan] = rel(x, refs[name].x)
        print(f"full size {name}: primitives {errs[name, False]:.3e}  plan {errs[name, True]:.3e}")
    for name in ("cgnr", "fista"):
        gate = max(1e-12, 4.0 * PRIMITIVE_ERROR_FULL[name])
        assert errs[name, True] <= gate, (name, errs[name, True], gate)


@pytest.mark.parametrize("dt", DT)
def test_fallbacks(rls, ctx, dt):
    """FISTA + TV in double precision still solves through the primitives; set_reg_d(RLS_REG_TV) is RLS_E_UNSUPPORTED;
    create_d with a Float32 code is RLS_E_INVALID with a message"""
    A, b, rho, lam1 = problem(dt, 384, 160, 77)
    Ad, bd = rls.DeviceMatrix.from_host(A, ctx), rls.DeviceVector.from_host(b, ctx)
    regs = lambda R: [R.TVRegularization(lam1, shape=(16, 10)), R.PositiveRegularization()]
    ref = O.FISTA(A, reg=regs(O), rho=rho, iterations=30, relTol=0.0)
    O.solve(ref, b)
    S = rls.createLinearSolver(rls.FISTA, Ad, reg=regs(rls), rho=rho, iterations=30, relTol=0.0)
    with Counter(ctx.lib) as cnt:
        cnt.arm_after_init(S)
        x = rls.solve_(S, bd).to_host()
    assert not S.state._plan and cnt.total > 0
    assert rel(x, ref.x) < 1e-12, rel(x, ref.x)
    # the C ABI directly
    lib, h = ctx.lib, ctx.handle
    N = Ad.N
    v = [rls.DeviceVector(N, dt, ctx) for _ in range(4)]
    plan = C.c_void_p()
    assert lib.rls_fista_create_d(h, Ad.code, Ad.M, N, Ad.ptr, Ad.lda, None, 0, v[0].ptr, v[1].ptr, v[2].ptr, v[3].ptr, C.byref(plan)) == 0
    assert lib.rls_fista_set_reg_d(plan, 4, 0.1, 1, 0) == -2      # RLS_REG_TV
    assert lib.rls_fista_set_reg_d(plan, 17, 0.1, 1, 0) == -2     # an unknown kind
    assert lib.rls_fista_set_reg_d(plan, 1, 0.1, 1, 0) == 0
    assert lib.rls_fista_destroy_d(plan) == 0
    for create in (lib.rls_cgnr_create_d, lib.rls_fista_create_d):
        for code in (0, 1):   # RLS_F32, RLS_C32
            plan = C.c_void_p()
            assert create(h, code, Ad.M, N, Ad.ptr, Ad.lda, None, 0, v[0].ptr, v[1].ptr, v[2].ptr, v[3].ptr, C.byref(plan)) == -1
            assert not plan.value and b"dtype must be RLS_F64 or RLS_C64" in lib.rls_last_error_string(h)
            assert lib.rls_nrm2_d(h, Ad.code, -1, None, (C.c_double * 2)()) == -1   # (another message in between)
            assert b"dtype must be" not in lib.rls_last_error_string(h)
        plan = C.c_void_p()
        assert create(h, Ad.code, Ad.M, N, None, 0, None, 0, v[0].ptr, v[1].ptr, v[2].ptr, v[3].ptr, C.byref(plan)) == -1   # neither A nor AHA


# shapes that select every instantiation of the two product kernels (plans_f64.hip: dp_gn_lanes, the CB choice of dp_gemv_t_v).
# t = A p: G lanes along the rows, V elements per lane (V = 2: Float64 with even M and lda); G = 64 / 32 need >= 256 workgroups of
# G V rows.  v = A^H t: CB columns per wave, 4 from N >= 8192, 2 from N >= 2048.  These shapes select the wide instantiations but
# stay inside their tails (N = 8, M = 64): their unrolled main loops are reached in test_gpu_f64_plan_products.py, not here.
VARIANTS = [("M=8192 (c128: G=32)", 8192, 8), ("M=16384 (c128: G=64; f64: V=2, G=32)", 16384, 8), ("M=32768 (f64: V=2, G=64)", 32768, 8),
            ("M=8193 (f64: V=1, G=32)", 8193, 8), ("M=16385 (f64: V=1, G=64)", 16385, 8), ("N=8192 (CB=4)", 64, 8192),
            ("N=8192, odd M (f64: V=1, CB=4)", 63, 8192), ("N=2048 (CB=2)", 64, 2048), ("N=2048, odd M (f64: V=1, CB=2)", 63, 2048)]


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("shape", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_every_product_kernel_variant(rls, ctx, dt, shape):
    """CGNR (lambda > 0) and FISTA + L1, 4 iterations, against the float64 oracle at 1e-12 on shapes that reach the wide-row
    (G = 32 / 64) and many-column (CB = 2 / 4) instantiations, in both element types and both load widths"""
    _, M, N = shape
    A, b, rho, lam1 = problem(dt, M, N, 13)
    Ad, bd = rls.DeviceMatrix.from_host(A, ctx), rls.DeviceVector.from_host(b, ctx)
    ref = O.CGNR(A, reg=O.L2Regularization(1e-2), iterations=4, relTol=0.0)
    O.solve(ref, b)
    S = rls.createLinearSolver(rls.CGNR, Ad, reg=rls.L2Regularization(1e-2), iterations=4, relTol=0.0)
    x = rls.solve_(S, bd).to_host()
    assert S.state._plan and S.state.iteration == ref.iteration == 4
    assert rel(x, ref.x) < 1e-12, rel(x, ref.x)
    assert close(S.state.alphal, ref.alpha) and close(S.state._residual, ref.convergence()["residual"])
    ref = O.FISTA(A, reg=O.L1Regularization(lam1), rho=rho, iterations=4, relTol=0.0)
    O.solve(ref, b)
    S = rls.createLinearSolver(rls.FISTA, Ad, reg=rls.L1Regularization(lam1), rho=rho, iterations=4, relTol=0.0)
    x = rls.solve_(S, bd).to_host()
    assert S.state._plan and rel(x, ref.x) < 1e-12, rel(x, ref.x)
    assert close(S.state.rel_res_norm, ref.rel_res_norm)


@pytest.mark.parametrize("dt", DT)
def test_reg_none_and_solution_pointer_through_the_abi(rls, ctx, dt):
    """RLS_REG_NONE through rls_fista_set_reg_d (the Python solver never passes it: its default term is L1 with lambda = 0) and
    rls_fista_solution_d: x for an even iteration count, xold for an odd one, from the status just read or from a read of its own"""
    A, b, rho, _ = problem(dt, 96, 40, 9)
    Ad, bd = rls.DeviceMatrix.from_host(A, ctx), rls.DeviceVector.from_host(b, ctx)
    lib, h = ctx.lib, ctx.handle
    from rls_amd import _lib
    x, x0, xold, res = (rls.DeviceVector(Ad.N, dt, ctx) for _ in range(4))
    plan = C.c_void_p()
    assert lib.rls_fista_create_d(h, Ad.code, Ad.M, Ad.N, Ad.ptr, Ad.lda, None, 0, x.ptr, x0.ptr, xold.ptr, res.ptr, C.byref(plan)) == 0
    assert lib.rls_fista_set_reg_d(plan, 0, 123.0, 1, 0) == 0   # RLS_REG_NONE: lambda is ignored
    assert lib.rls_fista_init_d(plan, bd.ptr, rho, 1.0, 0.0, 50, 0) == 0
    st, sol = _lib.FistaStatusD(), C.c_void_p()
    ref = O.FISTA(A, reg=O.L1Regularization(0.0), rho=rho, iterations=50, relTol=0.0)   # prox with threshold 0: the identity to 1e-16
    ref.init(b)
    for n, total in ((7, 7), (4, 11)):
        assert lib.rls_fista_step_status_d(plan, n, C.byref(st)) == 0 and st.iteration == total and not st.done
        assert lib.rls_fista_solution_d(plan, C.byref(sol)) == 0      # (answered from the status just read)
        for _ in range(n):
            ref.iterate()
        cur = xold if total & 1 else x
        assert sol.value == cur.ptr
        assert rel(cur.to_host(), ref.x) < 1e-12, (total, rel(cur.to_host(), ref.x))
        assert close(st.rel_res_norm, ref.rel_res_norm) and close(st.theta, ref.theta)
    assert lib.rls_fista_step_d(plan, 1) == 0                         # nothing read since: solution_d reads the record itself
    assert lib.rls_fista_solution_d(plan, C.byref(sol)) == 0 and sol.value == x.ptr
    ref.iterate()
    assert rel(x.to_host(), ref.x) < 1e-12
    assert lib.rls_fista_destroy_d(plan) == 0


@pytest.mark.parametrize("dt", DT)
def test_matrix_right_hand_side_runs_one_plan_per_column(rls, ctx, dt):
    """solve!(solver, B) in double precision keeps the per-column scheduler (the shared-A batched plans are Float32 / ComplexF32);
    each column's state now carries its own device plan, and the columns are those of independent solves"""
    M, N, K = 200, 96, 3
    A, b, rho, lam1 = problem(dt, M, N, 31)
    rng = np.random.default_rng(32)
    B = np.asfortranarray(np.stack([b, 2 * b - 1, (A @ rng.standard_normal(N)).astype(dt)], axis=1))
    Ad, Bd = rls.DeviceMatrix.from_host(A, ctx), rls.DeviceMatrix.from_host(B, ctx)
    for mk_ref, mk in ((lambda: O.CGNR(A, reg=O.L2Regularization(1e-3), iterations=20, relTol=0.0),
                        lambda: rls.createLinearSolver(rls.CGNR, Ad, reg=rls.L2Regularization(1e-3), iterations=20, relTol=0.0)),
                       (lambda: O.FISTA(A, reg=O.L1Regularization(lam1), rho=rho, iterations=20, relTol=0.0),
                        lambda: rls.createLinearSolver(rls.FISTA, Ad, reg=rls.L1Regularization(lam1), rho=rho, iterations=20, relTol=0.0))):
        S = mk()
        X = rls.solve_(S, Bd)
        X = X.to_host() if hasattr(X, "to_host") else np.stack([c.to_host() for c in X], axis=1)
        assert len(S.state.states) == K and all(st._plan and st._plan_d for st in S.state.states)
        for j in range(K):
            assert rel(X[:, j], O.solve(mk_ref(), B[:, j].copy())) < 1e-12, j
