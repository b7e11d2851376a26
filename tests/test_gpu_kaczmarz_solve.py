"""A whole regularised or randomised Kaczmarz solve as one launch (rls_kaczmarz_solve / _d): the projection and the prox run
on the registers that hold x at the end of every sweep, `randomized` walks one table of per-sweep row orders.

Gate: x and vl against the float64 oracle within 1e-5 relative (or twice the Float32 oracle's own error), 1e-12 for
Float64 / ComplexF64.  Shapes: M = 24 rows (23 used: one zero row) or M = 12 (sweeps of <= 16 rows: one launch per sweep); N picks
the instantiation (kz_launch): 40 = 1 x 256 masked vectorised, 41 / 43 = not vectorised, 512 = 1 x 256 full, 1100 = 2 x 512 masked,
2048 = 2 x 512 full, 4100 = 4 x 1024, 8200 = 8 x 1024 with a pipeline depth of 1."""
import ctypes as C

import numpy as np
import pytest

import rls_oracle as O

pytestmark = pytest.mark.gpu

ITS = 5
L2LAM = 0.05
REGSETS = ("pos", "real", "realpos", "l1", "posl1")
SHAPES = ([(np.complex64, n) for n in (40, 41, 512, 1100, 2048, 4100, 8200)] + [(np.float32, n) for n in (40, 43, 1024)] +
          [(np.float64, n) for n in (40, 1100)] + [(np.complex128, n) for n in (40, 1100)])
SEED = 11


def is_double(dt):
    return np.dtype(dt) in (np.dtype(np.float64), np.dtype(np.complex128))


def wide(dt):
    return np.complex128 if np.dtype(dt).kind == "c" else np.float64


def rel(a, b):
    n = np.linalg.norm(b)
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / (n if n > 0 else 1.0))


_problems = {}


def problem(dt, M, N):
    """A (row 3 zero: initkaczmarz skips it), b and lambda_1 = 0.3 x the median of |x| after one unregularised float64 sweep"""
    key = (np.dtype(dt).name, M, N)
    if key not in _problems:
        A, _, b = O.make_problem(M, N, dt, SEED)
        A = np.array(A)
        A[3, :] = 0
        first = run_oracle(A.astype(wide(dt)), b.astype(wide(dt)), [O.L2Regularization(L2LAM)], 1)
        lam1 = float(0.3 * np.median(np.abs(first[0][-1])))
        for a in (A, b):
            a.setflags(write=False)
        _problems[key] = (A, b, lam1)
    return _problems[key]


def regs(R, name, lam1):
    l2 = R.L2Regularization(L2LAM)
    return {"none": [l2], "pos": [l2, R.PositiveRegularization()], "real": [l2, R.RealRegularization()],
            "realpos": [l2, R.RealRegularization(), R.PositiveRegularization()], "l1": [l2, R.L1Regularization(lam1)],
            "posl1": [l2, R.PositiveRegularization(), R.L1Regularization(lam1)]}[name]


def run_oracle(A, b, reg, its, order_fn=None):
    """([x after init, x after sweep 1, ...], vl)"""
    ref = O.Kaczmarz(A, reg=reg, iterations=its, order_fn=order_fn)
    ref.init(b)
    xs = [ref.x.copy()]
    while ref.iterate() is not None:
        xs.append(ref.x.copy())
    return xs, ref.vl.copy()


_refs = {}


def reference(dt, M, N, name, its=ITS):
    """the float64 oracle and the oracle in the working precision, computed once per case"""
    key = (np.dtype(dt).name, M, N, name, its)
    if key not in _refs:
        A, b, lam1 = problem(dt, M, N)
        r64 = run_oracle(A.astype(wide(dt)), b.astype(wide(dt)), regs(O, name, lam1), its)
        r32 = r64 if is_double(dt) else run_oracle(A, b, regs(O, name, lam1), its)
        _refs[key] = (r64, r32)
    return _refs[key]


def gate(parity, tag, dt, got, want64, want32):
    if is_double(dt):
        e = rel(got, want64)
        assert e <= 1e-12, f"{tag}: {e:.3e} > 1e-12"
    else:
        parity(tag, got, want64, want32, record=False)


def device_solver(rls, ctx, dt, M, N, name, its=ITS, **kw):
    A, b, lam1 = problem(dt, M, N)
    Ad = rls.DeviceMatrix.from_host(np.asfortranarray(A), ctx)
    return rls.createLinearSolver(rls.Kaczmarz, Ad, reg=regs(rls, name, lam1), iterations=its, **kw), rls.DeviceVector.from_host(np.array(b), ctx)


class Counters:
    """counting proxies on the sweep / solve entries and on every rls_prox_* of the binding"""

    def __init__(self, rls, ctx):
        from rls_amd import _lib
        self.lib = ctx.lib
        self.names = [n for n in _lib.PROTOTYPES if n.startswith(("rls_kaczmarz_", "rls_prox_"))]
        self.calls = {n: 0 for n in self.names}

    def __enter__(self):
        self.orig = {n: getattr(self.lib, n) for n in self.names}
        for n in self.names:
            setattr(self.lib, n, self._proxy(n))
        return self

    def _proxy(self, n):
        def f(*a):
            self.calls[n] += 1
            return self.orig[n](*a)
        return f

    def __exit__(self, *exc):
        for n in self.names:
            setattr(self.lib, n, self.orig[n])

    def prox(self):
        return sum(v for n, v in self.calls.items() if n.startswith("rls_prox_"))

    def solve(self):
        return self.calls["rls_kaczmarz_solve"] + self.calls["rls_kaczmarz_solve_d"]

    def sweep(self):
        return self.calls["rls_kaczmarz_sweep"] + self.calls["rls_kaczmarz_sweep_d"]


# 1 / 2: parity of every regulariser set on every instantiation, M = 24 (one launch) and M = 12 (one launch per sweep)
@pytest.mark.parametrize("M", [24, 12])
@pytest.mark.parametrize("dt,N", SHAPES, ids=[f"{np.dtype(d).name}-{n}" for d, n in SHAPES])
def test_parity_of_the_fused_maps(rls, ctx, parity, dt, N, M):
    for name in REGSETS:
        (xs64, vl64), (xs32, vl32) = reference(dt, M, N, name)
        S, bd = device_solver(rls, ctx, dt, M, N, name)
        assert len(S.rowindex) == M - 1 and S._fused() is not None
        with Counters(rls, ctx) as cnt:
            x = rls.solve_(S, bd).to_host()
        assert cnt.prox() == 0 and cnt.sweep() == 0 and cnt.solve() == (1 if M == 24 else ITS), cnt.calls
        assert S.state.iteration == ITS
        tag = f"kaczmarz_solve_{np.dtype(dt).name}_{M}x{N}_{name}"
        print(f"{tag}: x {rel(x, xs64[-1]):.3e} (oracle32 {rel(xs32[-1], xs64[-1]):.3e})  vl {rel(S.state.vl.to_host(), vl64):.3e}")
        gate(parity, tag + "_x", dt, x, xs64[-1], xs32[-1])
        gate(parity, tag + "_vl", dt, S.state.vl.to_host(), vl64, vl32)
        if name in ("l1", "posl1"):   # the threshold bites, and not everywhere
            nz = np.count_nonzero(xs64[-1])
            assert 0 < nz < N, (tag, nz)
        if name != "l1":
            assert np.all(np.imag(x) == 0) and (name == "real" or np.all(np.real(x) >= 0))


# 1 / 3: launch counts and the columns of a matrix right-hand side
@pytest.mark.parametrize("M", [24, 12])
@pytest.mark.parametrize("dt,N", [(np.complex64, 1100), (np.float32, 43), (np.complex128, 40)])
def test_one_launch_and_matrix_columns(rls, ctx, dt, N, M):
    A, b, lam1 = problem(dt, M, N)
    rng = np.random.default_rng(11)
    B = np.stack([b, (A @ rng.standard_normal(N)).astype(dt), (0.5 * b + (A @ rng.standard_normal(N))).astype(dt)], axis=1)
    for name in ("posl1", "real"):
        cols = []
        for j in range(3):
            S, _ = device_solver(rls, ctx, dt, M, N, name)
            with Counters(rls, ctx) as cnt:
                cols.append(rls.solve_(S, rls.DeviceVector.from_host(np.ascontiguousarray(B[:, j]), ctx)).to_host())
            assert cnt.solve() == (1 if M == 24 else ITS) and cnt.sweep() == 0 and cnt.prox() == 0, cnt.calls
        S, _ = device_solver(rls, ctx, dt, M, N, name)
        with Counters(rls, ctx) as cnt:
            xs = rls.solve_(S, rls.DeviceMatrix.from_host(np.asfortranarray(B), ctx), scheduler=rls.BatchedState)
        assert cnt.solve() == (1 if M == 24 else ITS) and cnt.sweep() == 0 and cnt.prox() == 0, cnt.calls
        for j in range(3):
            assert np.array_equal(xs[j].to_host(), cols[j]), (name, j)
        assert np.array_equal(cols[0], rls.solve_(device_solver(rls, ctx, dt, M, N, name)[0], rls.DeviceVector.from_host(np.array(b), ctx)).to_host())


# 4: callbacks take one sweep per call with the maps inside it
@pytest.mark.parametrize("dt,N", [(np.complex64, 1100), (np.float32, 40), (np.float64, 40)])
def test_callbacks_step_through_the_same_iterates(rls, ctx, parity, dt, N):
    M, name = 24, "posl1"
    (xs64, _), (xs32, _) = reference(dt, M, N, name)
    S, bd = device_solver(rls, ctx, dt, M, N, name)
    whole = rls.solve_(S, bd).to_host()
    S2, bd2 = device_solver(rls, ctx, dt, M, N, name)
    cb = rls.StoreSolutionCallback()
    with Counters(rls, ctx) as cnt:
        last = rls.solve_(S2, bd2, callbacks=cb).to_host()
    assert cnt.solve() == ITS and cnt.prox() == 0 and cnt.sweep() == 0, cnt.calls
    assert len(cb.solutions) == ITS + 1
    assert np.array_equal(cb.solutions[-1], whole) and np.array_equal(last, whole)
    assert np.count_nonzero(cb.solutions[0]) == 0
    for k in range(1, ITS + 1):
        gate(parity, f"kaczmarz_solve_cb_{np.dtype(dt).name}_{k}", dt, cb.solutions[k], xs64[k], xs32[k])


# 5: randomized: one table of per-sweep orders
@pytest.mark.parametrize("name", ["none", "pos"])
@pytest.mark.parametrize("dt,N", [(np.complex64, 1100), (np.complex64, 41), (np.float32, 1024), (np.complex128, 40)])
def test_randomized_from_one_table(rls, ctx, parity, dt, N, name):
    M, its = 24, 6
    A, b, lam1 = problem(dt, M, N)
    kw = dict(randomized=True, subMatrixFraction=0.75, seed=4321)
    S, bd = device_solver(rls, ctx, dt, M, N, name, its=its, **kw)
    assert S.subMatrixSize == 18
    # the solver's orders, drawn again on the host: same seed, same Generator.choice calls, same p
    rng = np.random.default_rng(4321)
    p = S.probabilities / S.probabilities.sum()
    orders = [rng.choice(len(S.rowindex), size=18, replace=False, p=p) for _ in range(its)]
    table = S.rowindex[np.concatenate(orders)]
    from rls_amd import solvers
    pieces = solvers._kaczmarz_launch_splits(table, 18, its)
    with Counters(rls, ctx) as cnt:
        x = rls.solve_(S, bd).to_host()
    assert cnt.solve() == len(pieces) and cnt.sweep() == 0 and cnt.prox() == 0, (cnt.calls, pieces)
    assert np.array_equal(S.state.usedIndices, orders[-1]) and S.state.iteration == its
    order_fn = lambda k: orders[k]
    xs64, vl64 = run_oracle(A.astype(wide(dt)), b.astype(wide(dt)), regs(O, name, lam1), its, order_fn)
    xs32, vl32 = (xs64, vl64) if is_double(dt) else run_oracle(A, b, regs(O, name, lam1), its, order_fn)
    tag = f"kaczmarz_solve_rand_{np.dtype(dt).name}_{N}_{name}"
    print(f"{tag}: pieces {pieces}  x {rel(x, xs64[-1]):.3e} (oracle32 {rel(xs32[-1], xs64[-1]):.3e})  vl {rel(S.state.vl.to_host(), vl64):.3e}")
    gate(parity, tag + "_x", dt, x, xs64[-1], xs32[-1])
    gate(parity, tag + "_vl", dt, S.state.vl.to_host(), vl64, vl32)
    # the same solver driven sweep by sweep: the same bits, and the same generator stream when the two are mixed
    S2, bd2 = device_solver(rls, ctx, dt, M, N, name, its=its, **kw)
    rls.init_(S2, bd2)
    while rls.iterate(S2) is not None:
        pass
    assert np.array_equal(rls.solversolution(S2).to_host(), x) and np.array_equal(S2.state.vl.to_host(), S.state.vl.to_host())
    S3, bd3 = device_solver(rls, ctx, dt, M, N, name, its=its, **kw)
    rls.init_(S3, bd3)
    rls.iterate(S3)
    rls.iterate(S3)
    S3._run(S3.state)
    assert np.array_equal(rls.solversolution(S3).to_host(), x) and np.array_equal(S3.state.usedIndices, orders[-1])


def _abi_state(rls, ctx, dt, M, N):
    A, b, _ = problem(dt, M, N)
    S = rls.createLinearSolver(rls.Kaczmarz, rls.DeviceMatrix.from_host(np.asfortranarray(A), ctx), reg=rls.L2Regularization(L2LAM))
    x = rls.DeviceVector.from_host(np.zeros(N, dt), ctx)
    u = rls.DeviceVector.from_host(np.array(b), ctx)
    vl = rls.DeviceVector.from_host(np.zeros(M, dt), ctx)
    return S, x, u, vl


def _abi_call(ctx, S, x, u, vl, rows, den, first, nused, stride, n_sweeps, pk=0, rk=0, lam=0.0, eps_w=None):
    A = S.A_in
    dbl = is_double(x.dtype)
    f = ctx.lib.rls_kaczmarz_solve_d if dbl else ctx.lib.rls_kaczmarz_solve
    eps_w = float(np.sqrt(np.float32(L2LAM))) if eps_w is None else eps_w
    return f(ctx.handle, A.code, A.M, A.N, S.At.ptr, S.At.lda, 1, x.ptr, A.N, u.ptr, A.M, vl.ptr, A.M, rows.ptr + 4 * first * stride,
             den.ptr + (8 if dbl else 4) * first * stride, nused, stride, eps_w, n_sweeps, pk, rk, lam)


# 6: the vl hazard: rows that come back right behind a sweep boundary
@pytest.mark.parametrize("dt,N", [(np.complex64, 1100), (np.complex64, 8200), (np.float32, 43)])
def test_rows_recurring_across_a_sweep_boundary(rls, ctx, parity, dt, N):
    from rls_amd import solvers
    M, nused = 24, 18
    A, b, _ = problem(dt, M, N)
    S, x, u, vl = _abi_state(rls, ctx, dt, M, N)
    rng = np.random.default_rng(5)
    orders = [rng.permutation(len(S.rowindex))[:nused]]
    for _ in range(2):   # the last row comes back first, the second to last third (1 and 4 steps later)
        prev = orders[-1]
        others = [i for i in rng.permutation(len(S.rowindex)) if i not in (prev[-1], prev[-2])]
        orders.append(np.array([prev[-1], others[0], prev[-2]] + others[1:nused - 2]))
    assert all(len(set(o)) == nused for o in orders)
    clean = [np.roll(orders[0], -6 * s) for s in range(3)]   # nothing comes back within 4 steps: one launch
    for which, tab, want_pieces in (("hazard", orders, [(0, 1), (1, 1), (2, 1)]), ("clean", clean, [(0, 3)])):
        pos = np.concatenate(tab)
        rows = rls.DeviceVector.from_host(S.rowindex[pos].astype(np.int32).view(np.float32), ctx)
        den = rls.DeviceVector.from_host(S.denom[pos], ctx)
        pieces = solvers._kaczmarz_launch_splits(S.rowindex[pos], nused, 3)
        assert pieces == want_pieces
        x.fill_(0)
        vl.fill_(0)
        for first, n in pieces:
            assert _abi_call(ctx, S, x, u, vl, rows, den, first, nused, nused, n) == 0
        order_fn = lambda k: tab[k]
        xs64, vl64 = run_oracle(A.astype(wide(dt)), b.astype(wide(dt)), [O.L2Regularization(L2LAM)], 3, order_fn)
        xs32, vl32 = run_oracle(A, b, [O.L2Regularization(L2LAM)], 3, order_fn)
        tag = f"kaczmarz_solve_{which}_{np.dtype(dt).name}_{N}"
        print(f"{tag}: x {rel(x.to_host(), xs64[-1]):.3e} (oracle32 {rel(xs32[-1], xs64[-1]):.3e})  vl {rel(vl.to_host(), vl64):.3e}")
        gate(parity, tag + "_x", dt, x.to_host(), xs64[-1], xs32[-1])
        gate(parity, tag + "_vl", dt, vl.to_host(), vl64, vl32)


# 7: ctx.tune(kaczmarz_fused=0): the host loop
@pytest.mark.parametrize("dt,N", [(np.complex64, 1100), (np.float64, 40)])
def test_escape_hatch_takes_the_host_loop(rls, ctx, parity, dt, N):
    M, name = 24, "posl1"
    (xs64, vl64), (xs32, vl32) = reference(dt, M, N, name)
    S, bd = device_solver(rls, ctx, dt, M, N, name)
    fused = rls.solve_(S, bd).to_host()
    ctx.tune(kaczmarz_fused=0)
    try:
        S2, bd2 = device_solver(rls, ctx, dt, M, N, name)
        assert S2._fused() is None
        with Counters(rls, ctx) as cnt:
            loop = rls.solve_(S2, bd2).to_host()
        assert cnt.prox() == 2 * ITS and cnt.sweep() == ITS and cnt.solve() == 0, cnt.calls
        x0 = rls.DeviceVector.from_host(np.ones(N, dt), ctx)
        Sx, xx, uu, vv = _abi_state(rls, ctx, dt, M, N)
        rows = rls.DeviceVector.from_host(Sx.rowindex.astype(np.int32).view(np.float32), ctx)
        den = rls.DeviceVector.from_host(Sx.denom, ctx)
        assert _abi_call(ctx, Sx, x0, uu, vv, rows, den, 0, len(Sx.rowindex), 0, 1, pk=2) == -2   # RLS_E_UNSUPPORTED while switched off
        assert np.array_equal(x0.to_host(), np.ones(N, dt))
    finally:
        ctx.tune(kaczmarz_fused=1)
    gate(parity, f"kaczmarz_solve_hostloop_{np.dtype(dt).name}", dt, loop, xs64[-1], xs32[-1])
    gate(parity, f"kaczmarz_solve_hostloop_vs_fused_{np.dtype(dt).name}", dt, fused, xs64[-1], xs32[-1])
    assert rel(loop, fused) <= (1e-12 if is_double(dt) else 1e-5)


# 8: invalid arguments
@pytest.mark.parametrize("dt", [np.complex64, np.float64])
def test_invalid_arguments(rls, ctx, dt):
    M, N = 24, 40
    S, x, u, vl = _abi_state(rls, ctx, dt, M, N)
    nused = len(S.rowindex)
    rows = rls.DeviceVector.from_host(np.tile(S.rowindex, 2).astype(np.int32).view(np.float32), ctx)
    den = rls.DeviceVector.from_host(np.tile(S.denom, 2), ctx)
    start = (np.arange(N) + 1).astype(dt)
    x.copy_from(rls.DeviceVector.from_host(start, ctx))
    bad = [dict(stride=5), dict(stride=-1), dict(stride=nused + 1), dict(pk=3), dict(pk=-1), dict(rk=3), dict(rk=4), dict(rk=-1),
           dict(rk=1, lam=-0.5), dict(lam=-1e-3), dict(rk=2, lam=float("nan"))]
    for kw in bad:
        st = _abi_call(ctx, S, x, u, vl, rows, den, 0, nused, kw.pop("stride", 0), 2, **kw)
        assert st == -1, (kw, st)
    assert np.array_equal(x.to_host(), start) and np.count_nonzero(vl.to_host()) == 0
    # and the valid neighbours go through
    assert _abi_call(ctx, S, x, u, vl, rows, den, 0, nused, nused, 2, pk=2, rk=1, lam=0.0) == 0
    assert not np.array_equal(x.to_host(), start)
