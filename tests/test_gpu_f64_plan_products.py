"""The two product kernels of the Float64 / ComplexF64 plans (csrc/plans_f64.hip) one by one, in every loop regime, and the
single-workgroup update kernels past one stride.

Products, through the C ABI as it is:
  dp_gemv_t alone   rls_cgnr_create_d on caller-owned vectors, rls_cgnr_init_d(b): p = r = A^H b, z0 = ||A^H b||
  dp_gemv_n         one rls_cgnr_step_status_d(plan, 1): v = A^H (A p0) stays in the caller's buffer, and alpha = zeta / ||A p0||^2
                    gives back the sum of the per-workgroup partials (zeta is the old <r, r>, published unchanged); both are judged
                    on the device's own p0, read back after init
  dp_gemv_n alone   a Gram-only plan (A = NULL): v = AHA p0 is one product over a square operand (small N only)

Reference: the same product in numpy.longdouble / clongdouble from the float64 inputs.  Bound, per output entry and for any order
of summation (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., (3.5): |fl(x.y) - x.y| <= gamma_n sum |x_k||y_k|):
    |got_i - ref_i| <= c (n_terms + 4) 2^-53 sum_k |a_ik| |x_k|
real: n_terms = n, c = 1.  Complex: each component of a complex dot product of n terms is a real sum of 2n products whose absolute
values add up to no more than sum |a||x| (|a_r x_r| + |a_i x_i| <= |a||x|, Cauchy-Schwarz), so n_terms = 2n for the component and
c = sqrt 2 for the modulus of the two components' errors.  Fused multiply-adds only remove roundings.  The bound is derived, never
measured: an entry beyond it is a finding, not a reason to widen it.
Composite quantities carry the bounds of their parts (see bound_npp, bound_v below).

Guards: A is uploaded with lda = M + pad and NaN in the padding rows; every caller-owned vector is GUARD elements longer than N,
prefilled with a sentinel that must come back bit-identical (a V = 2 lane or a duplicate column that stores past the end).

The solver-level half runs CGNR and FISTA through the Python solvers at the N where a thread of the 1024-thread update kernels
owns one element, two, or a ragged count, at the bars of test_gpu_f64_plans.py."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rls_oracle as O  # noqa: E402  (the checker)
from test_gpu_f64_plans import GRAM_TOL, ITER_TOL, SCALAR_TOL, _early_tols, close, plan_path, rel, upload_padded  # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
GUARD = 5
SENTINEL = {np.dtype(np.float64): np.float64(-1.2345e300), np.dtype(np.complex128): np.complex128(-1.2345e300 + 9.875e299j),
            np.dtype(np.float32): np.float32(-1.2345e30), np.dtype(np.complex64): np.complex64(-1.2345e30 + 9.875e29j)}
# (the reference type of each element type; the 4-byte types are judged in float64 / complex128: test_gpu_gemv_edges.py)
LD = {np.dtype(np.float64): np.longdouble, np.dtype(np.complex128): np.clongdouble,
      np.dtype(np.float32): np.float64, np.dtype(np.complex64): np.complex128}
POOL = {np.dtype(np.float64): 5_400_000, np.dtype(np.complex128): 2_700_000}   # the largest operand of each type, in elements
KINDS = [("f64-V1", np.float64, 1), ("f64-V2", np.float64, 2), ("c128-V1", np.complex128, 1)]
WORST = {}   # group -> (largest error / bound, case)


def is_cplx(dt):
    return np.dtype(dt).kind == "c"


def gamma(dt, n):
    """c (n_terms + 4) 2^-53 of the module docstring for a dot product of n elements of type dt"""
    return (math.sqrt(2.0) * (2 * n + 4) if is_cplx(dt) else (n + 4)) * U


# ---- the host's choices, restated (plans_f64.hip: dp_gn_lanes, dp_vec, the CB choice of dp_gemv_t_v) --------------------------
def gn_lanes(M, V):
    for G in (64, 32):
        if -(-M // (G * V)) >= 256:
            return G
    return 16


def load_width(dt, M, lda):
    return 2 if (not is_cplx(dt) and M % 2 == 0 and lda % 2 == 0) else 1


def gt_cb(N):
    return 4 if N // 16 >= 512 else 2 if N // 8 >= 256 else 1


def pad_for(dt, M, V):
    """a padding of 2 or 3 rows that makes the host choose load width V: Float64 sees an even and an odd lda"""
    for pad in ((2, 3) if V == 2 else (3, 2)):
        if load_width(dt, M, M + pad) == V:
            return pad
    raise AssertionError((dt, M, V))


# ---- data: one pool of Gaussian numbers per element type, every A a view of it -------------------------------------------------
_pool = {}


def matrix(dt, M, N):
    key = np.dtype(dt)
    if key not in _pool:
        rng = np.random.default_rng(20260)
        v = rng.standard_normal(POOL[key])
        if is_cplx(key):
            v = (v + 1j * rng.standard_normal(POOL[key])) / math.sqrt(2.0)
        v = v.astype(key)
        v.setflags(write=False)
        _pool[key] = v
    assert M * N <= POOL[key], (M, N)
    return _pool[key][: M * N].reshape((M, N), order="F")


def vector(dt, n, seed):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(n)
    if is_cplx(dt):
        v = (v + 1j * rng.standard_normal(n)) / math.sqrt(2.0)
    return v.astype(dt)


def note(group, ratio, case):
    if ratio > WORST.get(group, (-1.0, ""))[0]:
        WORST[group] = (ratio, case)
    print(f"{group}: {case}: error / bound {ratio:.3e}")


def held(group, case, err, bound):
    """per entry: err <= bound; records the largest ratio"""
    err, bound = np.asarray(err, dtype=np.float64).ravel(), np.asarray(bound, dtype=np.float64).ravel()
    ratio = float(np.max(err / np.maximum(bound, 1e-300))) if err.size else 0.0
    note(group, ratio, case)
    bad = np.nonzero(~(err <= bound))[0]
    assert bad.size == 0, f"{group} {case}: {bad.size} entries beyond the bound, first {bad[0]}: {err[bad[0]]:.3e} > {bound[bad[0]]:.3e}"


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for g, (r, c) in sorted(WORST.items()):
        print(f"\nlargest error / bound, {g}: {r:.3e}  ({c})")


class Guarded:
    """a device vector of n + GUARD elements (+ `lead` in front), the excess prefilled with the sentinel (or with `fill`)"""

    def __init__(self, rls, ctx, dt, n, body=None, lead=0, fill=None):
        self.n, self.lead, self.dt = n, lead, np.dtype(dt)
        self.host0 = np.full(lead + n + GUARD, SENTINEL[self.dt] if fill is None else fill, dtype=self.dt)
        if body is not None:
            self.host0[lead: lead + n] = body
        self.dev = rls.DeviceVector.from_host(self.host0, ctx)
        self.ptr = self.dev.ptr + lead * self.dt.itemsize

    def read(self):
        """the n elements; asserts that the excess is bit-unchanged"""
        h = self.dev.to_host()
        assert h[: self.lead].tobytes() == self.host0[: self.lead].tobytes(), "elements in front of the vector were written"
        assert h[self.lead + self.n:].tobytes() == self.host0[self.lead + self.n:].tobytes(), "elements past the end of the vector were written"
        return h[self.lead: self.lead + self.n]


class Plan:
    """rls_cgnr_create_d on guarded caller-owned x, r, p, v"""

    def __init__(self, rls, ctx, dt, M, N, A=None, pad=0, gram=None, gpad=0):
        from rls_amd import _lib
        self.lib, self.h, self.dt, self.M, self.N = ctx.lib, ctx.handle, np.dtype(dt), M, N
        self.Ad = upload_padded(rls, ctx, A, pad) if A is not None else None
        self.Gd = upload_padded(rls, ctx, gram, gpad) if gram is not None else None
        self.x, self.r, self.p, self.v = (Guarded(rls, ctx, dt, N) for _ in range(4))
        self.plan = C.c_void_p()
        code = rls.DeviceVector(1, dt, ctx).code
        st = self.lib.rls_cgnr_create_d(self.h, code, M, N, self.Ad.ptr if self.Ad else None, self.Ad.lda if self.Ad else 0,
                                        self.Gd.ptr if self.Gd else None, self.Gd.lda if self.Gd else 0,
                                        self.x.ptr, self.r.ptr, self.p.ptr, self.v.ptr, C.byref(self.plan))
        assert st == 0, self.lib.rls_last_error_string(self.h)
        self.status = _lib.CgnrStatusD()

    def init(self, b_ptr, iterations=2):
        assert self.lib.rls_cgnr_init_d(self.plan, b_ptr, 0.0, 0.0, iterations) == 0
        assert self.lib.rls_cgnr_get_status_d(self.plan, C.byref(self.status)) == 0
        return self.status

    def step(self):
        assert self.lib.rls_cgnr_step_status_d(self.plan, 1, C.byref(self.status)) == 0
        return self.status

    def close(self):
        if self.plan:
            assert self.lib.rls_cgnr_destroy_d(self.plan) == 0
            self.plan = None


def ld_norm2(v):
    w = v.astype(LD[v.dtype])
    return np.sum(w.real * w.real + w.imag * w.imag) if is_cplx(v.dtype) else np.sum(w * w)


def adjoint_case(rls, ctx, case, dt, M, N, pad, lead=0):
    """init on (A, b): p = r = A^H b against the longdouble product entry by entry, x = v = 0, z0 = ||p||.  Returns p's bytes."""
    A, b = matrix(dt, M, N), vector(dt, M, 7 * M + N)
    plan = Plan(rls, ctx, dt, M, N, A=A, pad=pad)
    bd = Guarded(rls, ctx, dt, M, body=b, lead=lead)
    try:
        st = plan.init(bd.ptr)
        p, r, x, v = plan.p.read(), plan.r.read(), plan.x.read(), plan.v.read()
        bd.read()
    finally:
        plan.close()
    ref = np.conj(np.conj(b).astype(LD[np.dtype(dt)]) @ A.astype(LD[np.dtype(dt)]))   # (b^H A)^H: one product, columns contiguous
    bound = gamma(dt, M) * (np.abs(b) @ np.abs(A))
    held("dp_gemv_t", case, np.abs(p.astype(LD[np.dtype(dt)]) - ref), bound)
    assert r.tobytes() == p.tobytes() and not x.any() and not v.any(), case
    # z0 = sqrt(sum |p_j|^2) of the device's own p: N positive terms (complex: fma(x, x, y y), two roundings) and one square root
    nrm = float(np.sqrt(ld_norm2(p)))
    held("init z0", case, [abs(st.z0 - nrm)], [(N + 4) * U * nrm])
    assert st.iteration == 0
    return p.tobytes()


def forward_case(rls, ctx, case, dt, M, N, pad):
    """init, read the device's p0, one step: ||A p0||^2 = zeta / alpha and v = A^H (A p0) against longdouble on that p0"""
    A, b = matrix(dt, M, N), vector(dt, M, 3 * M + N)
    plan = Plan(rls, ctx, dt, M, N, A=A, pad=pad)
    bd = Guarded(rls, ctx, dt, M, body=b)
    try:
        plan.init(bd.ptr)
        p0 = plan.p.read().copy()
        st = plan.step()
        v, x = plan.v.read(), plan.x.read()
        plan.p.read(), plan.r.read()
    finally:
        plan.close()
    L = LD[np.dtype(dt)]
    Al, absA = A.astype(L), np.abs(A)
    t = Al @ p0.astype(L)                                     # reference product 1: t = A p0
    e_t = gamma(dt, N) * (absA @ np.abs(p0))                  # |t^_i - t_i| <= e_t[i], t^ the device's (unseen) product
    abs_t = np.abs(t).astype(np.float64)
    # bound_npp.  | sum |t^_i|^2 - sum |t_i|^2 | <= sum e_i (2 |t_i| + e_i); the device then sums M squares (two roundings each for
    # complex, any order: (M + 4) u relative, the terms being positive), divides zeta by it and the test divides back: 4 u more.
    npp = float(np.sum((t.real * t.real + t.imag * t.imag) if is_cplx(dt) else t * t))
    d1 = float(np.sum(e_t * (2.0 * abs_t + e_t)))
    bound_npp = d1 + (M + 8) * U * (npp + d1)
    assert st.alpha_im == 0.0 and st.iteration == 1
    got_npp = np.longdouble(st.zeta) / np.longdouble(st.alpha_re)
    held("dp_gemv_n  ||A p||^2", case, [abs(float(got_npp - np.longdouble(npp)))], [bound_npp])
    # bound_v.  v^_j = fl(sum_i conj(a_ij) t^_i): gamma_M sum_i |a_ij| |t^_i| with |t^_i| <= |t_i| + e_i, and the product's own
    # propagation of t^ - t: sum_i |a_ij| e_i.
    vref = np.conj(np.conj(t) @ Al)                           # reference product 2: v = A^H t
    bound_v = gamma(dt, M) * ((abs_t + e_t) @ absA) + e_t @ absA
    held("dp_gemv_t after dp_gemv_n", case, np.abs(v.astype(L) - vref), bound_v)
    # x = alpha p0 from x = 0: one fused multiply-add per component pair
    held("update x", case, np.abs(x - st.alpha_re * p0), 4.0 * math.sqrt(2.0) * U * abs(st.alpha_re) * np.abs(p0))
    return v.tobytes() + bytes(st)


# ---- dp_gemv_n: every G x V, every trip count of the unrolled loop and the tail ---------------------------------------------------
RAGGED_M = {1: {16: 85, 32: 8203, 64: 16405}, 2: {16: 106, 32: 16406, 64: 32810}}   # last workgroup: fewer than half its rows live
RANGE_M = {1: [(8160, 16), (8161, 32), (16320, 32), (16321, 64)], 2: [(16320, 16), (16322, 32), (32640, 32), (32642, 64)]}


def gn_columns(G):
    step = 8 * (64 // G)   # GN_WAVES * (64 / G) column slots
    return [(1, "one-column"), (step - 1, "tail-only-short"), (7 * step, "tail-only-7-trips"), (7 * step + 1, "one-slot-unrolled"),
            (8 * step, "all-unrolled-no-tail"), (8 * step + 1, "unrolled+1-column-tail"), (16 * step + 3, "two-trips+tail")]


def gn_cases():
    out = []
    for kind, dt, V in KINDS:
        for G in (16, 32, 64):
            M = RAGGED_M[V][G]
            assert gn_lanes(M, V) == G and M % (G * V) and 2 * (M % (G * V)) < G * V
            for N, regime in gn_columns(G):
                out.append(pytest.param(dt, V, G, M, N, id=f"gemv_n-{kind}-G{G}-M{M}-ragged-last-workgroup-N{N}-{regime}"))
        for M, G in RANGE_M[V]:
            assert gn_lanes(M, V) == G
            edge = "first-M" if gn_lanes(M - V, V) != G else "last-M"
            out.append(pytest.param(dt, V, G, M, 8 * 8 * (64 // G) + 1, id=f"gemv_n-{kind}-G{G}-{edge}-of-range-M{M}"))
    return out


@pytest.mark.parametrize("dt,V,G,M,N", gn_cases())
def test_forward_product(rls, ctx, dt, V, G, M, N):
    pad = pad_for(dt, M, V)
    assert load_width(dt, M, M + pad) == V and gn_lanes(M, V) == G
    forward_case(rls, ctx, f"{np.dtype(dt).name} V={V} G={G} {M}x{N} lda={M + pad}", dt, M, N, pad)


# ---- dp_gemv_t: every CB x V, the unrolled loop's hand-over to the tail, the column-block edges -----------------------------------
def gt_rows(CB, V):
    T = (8 // CB) * 64 * V   # rows of one unrolled trip
    if V == 2:
        return [(T - 2, "tail-only"), (T, "one-trip-no-tail"), (T + 2, "one-trip+one-lane-tail"), (T + 136, "one-trip+two-chunk-tail")]
    return [(T - 1, "tail-only"), (T, "one-trip-no-tail"), (T + 1, "one-trip+one-lane-tail"), (T + 64 + 7, "one-trip+two-chunk-tail")]


GT_N_FOR_ROWS = {1: 5, 2: 2049, 4: 8195}
GT_COLUMNS = {1: [(1, "N=1-waves-return-early"), (2047, "last-N-of-CB1")], 2: [(2048, "first-N-of-CB2"), (8191, "last-N-of-CB2")],
              4: [(8192, "first-N-of-CB4"), (8193, "one-real-column+3-duplicates")]}
GT_N_NAME = {5: "N=5-waves-return-early", 2049: "one-real-column+1-duplicate", 8195: "three-real-columns+1-duplicate"}


def gt_cases():
    out = []
    for kind, dt, V in KINDS:
        for CB in (1, 2, 4):
            N = GT_N_FOR_ROWS[CB]
            for M, regime in gt_rows(CB, V):
                out.append(pytest.param(dt, V, CB, M, N, id=f"gemv_t-{kind}-CB{CB}-M{M}-{regime}-N{N}-{GT_N_NAME[N]}"))
            M = gt_rows(CB, V)[-1][0]
            for N, regime in GT_COLUMNS[CB]:
                out.append(pytest.param(dt, V, CB, M, N, id=f"gemv_t-{kind}-CB{CB}-N{N}-{regime}-M{M}"))
    return out


@pytest.mark.parametrize("dt,V,CB,M,N", gt_cases())
def test_adjoint_product(rls, ctx, dt, V, CB, M, N):
    pad = pad_for(dt, M, V)
    assert load_width(dt, M, M + pad) == V and gt_cb(N) == CB
    adjoint_case(rls, ctx, f"{np.dtype(dt).name} V={V} CB={CB} {M}x{N} lda={M + pad}", dt, M, N, pad)


@pytest.mark.parametrize("CB", [1, 2, 4], ids=lambda cb: f"unaligned-b-CB{cb}")
def test_adjoint_product_with_unaligned_b(rls, ctx, CB):
    """Float64, even M and lda (V = 2 for a 16-byte aligned b): b at the buffer's base, then 8 bytes in (dp_vec drops to V = 1).
    Both hold the bound; they need not agree to the bit (two summation orders)."""
    M, N = gt_rows(CB, 2)[-1][0], GT_N_FOR_ROWS[CB]
    assert load_width(np.float64, M, M + 2) == 2
    for lead in (0, 1):
        adjoint_case(rls, ctx, f"float64 CB={CB} {M}x{N} b at base + {8 * lead} bytes", np.float64, M, N, 2, lead=lead)


# ---- dp_gemv_n alone: a Gram-only plan, v = AHA p0 over a square operand ------------------------------------------------------------
GRAM_N = [(2, "two-columns")] + [(n, r) for n, r in gn_columns(16) if n > 1]


@pytest.mark.parametrize("kind,dt,V", KINDS, ids=[k[0] for k in KINDS])
@pytest.mark.parametrize("N,regime", GRAM_N, ids=[f"gram-{r}" for _, r in GRAM_N])
def test_forward_product_alone_on_a_gram_operand(rls, ctx, kind, dt, V, N, regime):
    """G = 16 (N < 8161).  p0 = b (a copy), v = G p0 entry by entry, alpha = zeta / <p0, v> on the device's own v."""
    N += N % 2 if V == 2 else 0   # (V = 2 needs an even N: the next one up keeps the regime, bar one more unrolled slot)
    pad = pad_for(dt, N, V)
    case = f"{kind} gram {N}x{N} ldg={N + pad} {regime}"
    Gm, b = matrix(dt, N, N), vector(dt, N, N)
    plan = Plan(rls, ctx, dt, 0, N, gram=Gm, gpad=pad)
    bd = Guarded(rls, ctx, dt, N, body=b)
    try:
        plan.init(bd.ptr)
        p0 = plan.p.read().copy()
        assert p0.tobytes() == b.tobytes()
        st = plan.step()
        v = plan.v.read()
        plan.x.read(), plan.r.read(), plan.p.read()
    finally:
        plan.close()
    L = LD[np.dtype(dt)]
    held("dp_gemv_n alone", case, np.abs(v.astype(L) - Gm.astype(L) @ p0.astype(L)), gamma(dt, N) * (np.abs(Gm) @ np.abs(p0)))
    # alpha = zeta / conj(p0).v on the device's own v: an N-term dot product, one (complex) division, and the division back
    dot = np.sum(np.conj(p0).astype(L) * v.astype(L))
    got = np.longdouble(st.zeta) / (np.longdouble(st.alpha_re) + (1j * np.longdouble(st.alpha_im) if is_cplx(dt) else 0))
    sabs = float(np.abs(p0) @ np.abs(v))
    held("gram <p, v>", case, [abs(complex(got - dot))], [gamma(dt, N) * sabs + 8.0 * U * abs(complex(dot))])


# ---- fixed-order sums: the same bits run to run --------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["gemv_t", "gemv_n"], ids=lambda w: f"determinism-{w}")
def test_products_are_bit_reproducible(rls, ctx, which):
    for kind, dt, V in KINDS:
        if which == "gemv_t":
            M, N = gt_rows(2, V)[-1][0], 2049
            runs = [adjoint_case(rls, ctx, f"{kind} {M}x{N} run {i}", dt, M, N, pad_for(dt, M, V)) for i in range(2)]
        else:
            M, N = RAGGED_M[V][32], 8 * 16 + 1
            runs = [forward_case(rls, ctx, f"{kind} {M}x{N} run {i}", dt, M, N, pad_for(dt, M, V)) for i in range(2)]
        assert runs[0] == runs[1], kind


# ---- the same regimes through the whole plans -------------------------------------------------------------------------------------
DT = [np.float64, np.complex128]
DT_IDS = ["float64", "complex128"]
OPERAND_BYTES = 64 << 20
_problems = {}


def rows_for(dt, N):
    """M about 1.5 N, cut down where the operand would pass 64 MiB (the update kernels see N alone)"""
    if N == 1:
        return 3
    return min(3 * N // 2, OPERAND_BYTES // (N * np.dtype(dt).itemsize))


def problem(dt, N, M=None):
    """A, b, rho, lambda_1, computed once.  rho = 0.9 / L with L = (sqrt M + sqrt N)^2, the limit of ||A||_2^2 for Gaussian entries
    (an SVD of every A would be most of this module's time); small operands take the norm itself."""
    M = rows_for(dt, N) if M is None else M
    key = (np.dtype(dt).name, M, N)
    if key not in _problems:
        A, _, b = O.make_problem(M, N, dt, 100 + N)
        L = np.linalg.norm(A, 2) ** 2 if M * N <= 1 << 16 else (math.sqrt(M) + math.sqrt(N)) ** 2
        g = A.conj().T @ b
        for a in (A, b, g):
            a.setflags(write=False)
        _problems[key] = (A, b, 0.9 / L, 0.02 * float(np.max(np.abs(g))), g)
    return _problems[key]


def solve_both(rls, ctx, dt, N, gram):
    """CGNR (lambda = 1e-2) and FISTA + L1, 4 iterations, against the float64 oracle: test_every_product_kernel_variant's checks"""
    A, b, rho, lam1, g = problem(dt, N)
    if gram:
        Gh = np.asfortranarray(A.conj().T @ A)
        Ad, rhs, oA = None, np.array(g), None
        d_kw, o_kw, tol = dict(AHA=rls.DeviceMatrix.from_host(Gh, ctx)), dict(AHA=Gh), GRAM_TOL
    else:
        Ad, rhs, oA, d_kw, o_kw, tol = upload_padded(rls, ctx, A, 2), np.array(b), A, {}, {}, ITER_TOL
    bd = rls.DeviceVector.from_host(rhs, ctx)
    ref = O.CGNR(oA, reg=O.L2Regularization(1e-2), iterations=4, relTol=0.0, **o_kw)
    O.solve(ref, rhs)
    S = rls.createLinearSolver(rls.CGNR, Ad, reg=rls.L2Regularization(1e-2), iterations=4, relTol=0.0, **d_kw)
    x = rls.solve_(S, bd).to_host()
    assert S.state._plan and plan_path(rls, ctx, S) == (2 if gram else 0)
    assert S.state.iteration == ref.iteration == min(4, N)
    print(f"N={N} {np.dtype(dt).name} gram={gram}: cgnr {rel(x, ref.x):.3e}")
    assert rel(x, ref.x) < tol, rel(x, ref.x)
    assert close(S.state.alphal, ref.alpha)
    if N > 1:   # (N = 1: one step solves the system, what is left of r is rounding noise of r0 - alpha v)
        assert close(S.state._residual, ref.convergence()["residual"])
    ref = O.FISTA(oA, reg=O.L1Regularization(lam1), rho=rho, iterations=4, relTol=0.0, **o_kw)
    O.solve(ref, rhs)
    S = rls.createLinearSolver(rls.FISTA, Ad, reg=rls.L1Regularization(lam1), rho=rho, iterations=4, relTol=0.0, **d_kw)
    x = rls.solve_(S, bd).to_host()
    print(f"N={N} {np.dtype(dt).name} gram={gram}: fista {rel(x, ref.x):.3e}")
    assert S.state._plan and rel(x, ref.x) < tol, rel(x, ref.x)
    assert close(S.state.rel_res_norm, ref.rel_res_norm)


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("N", [1, 1023, 1024, 1025, 2049, 3000], ids=lambda n: f"update-kernels-N{n}")
def test_update_kernels_past_one_stride(rls, ctx, dt, N):
    """N below, at and above UPD_T = 1024, two full strides and one element, and a ragged third stride; matrix-free"""
    solve_both(rls, ctx, dt, N, gram=False)


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("N", [1025, 2049], ids=lambda n: f"update-kernels-gram-N{n}")
def test_update_kernels_past_one_stride_in_gram_mode(rls, ctx, dt, N):
    """the GRAM instantiation of the CGNR update (<p, v> strided over N) and the square dp_gemv_n"""
    solve_both(rls, ctx, dt, N, gram=True)


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
@pytest.mark.parametrize("pos", [False, True], ids=["l21", "l21+positive"])
@pytest.mark.parametrize("N", [4100, 4102], ids=["L21-N4100-slen1025-two-groups-per-thread", "L21-N4102-ragged-tail-joins-first-groups"])
def test_l21_groups_crossing_threads(rls, ctx, dt, pos, N):
    """FISTA + L21 (slices = 4), gradient restart: slen = 1025 > UPD_T, so thread 0 owns groups 0 and 1024, and every group's
    elements belong to four (five) different threads of the passes around it.  lambda = the median group norm of A^H b: the
    threshold bites on some groups and not on all."""
    A, b, rho, _, g = problem(dt, N)
    slen = N // 4
    idx = np.arange(N) % slen
    lam = float(np.median(np.sqrt(np.bincount(idx, weights=np.abs(g) ** 2, minlength=slen))))
    regs = lambda R: [R.L21Regularization(lam, slices=4)] + ([R.PositiveRegularization()] if pos else [])
    kw = dict(rho=rho, iterations=4, relTol=0.0, restart="gradient")
    ref = O.FISTA(A, reg=regs(O), **kw)
    O.solve(ref, np.array(b))
    S = rls.createLinearSolver(rls.FISTA, upload_padded(rls, ctx, A, 2), reg=regs(rls), **kw)
    x = rls.solve_(S, rls.DeviceVector.from_host(np.array(b), ctx)).to_host()
    assert S.state._plan and S.state.iteration == ref.iteration == 4
    zero_ref = np.bincount(idx, weights=np.abs(ref.x), minlength=slen) == 0
    zero_dev = np.bincount(idx, weights=np.abs(x), minlength=slen) == 0
    nz = int(zero_ref.sum())
    print(f"N={N} {np.dtype(dt).name} pos={pos}: {nz} of {slen} groups zero, x {rel(x, ref.x):.3e}")
    assert 0 < nz < slen and np.array_equal(zero_ref, zero_dev)
    assert rel(x, ref.x) < ITER_TOL, rel(x, ref.x)
    assert close(S.state.rel_res_norm, ref.rel_res_norm) and close(S.state.theta, ref.theta)


@pytest.mark.parametrize("dt", DT, ids=DT_IDS)
def test_early_stop_where_a_thread_owns_two_elements(rls, ctx, dt):
    """N = 1025: relTol stops CGNR at iteration 3 of 10 and FISTA + L1 at its iteration k; the launches behind `done` are no-ops"""
    N = 1025
    A, b, rho, lam1, _ = problem(dt, N)
    cg_tol, fi_tol, k = _early_tols(A, np.array(b), rho, lam1)
    Ad, bd = upload_padded(rls, ctx, A, 2), rls.DeviceVector.from_host(np.array(b), ctx)
    for name, mk, mk_ref, stop, step in (
            ("cgnr", lambda: rls.createLinearSolver(rls.CGNR, Ad, iterations=10, relTol=cg_tol), lambda: O.CGNR(A, iterations=10, relTol=cg_tol),
             3, ctx.lib.rls_cgnr_step_d),
            ("fista", lambda: rls.createLinearSolver(rls.FISTA, Ad, reg=rls.L1Regularization(lam1), rho=rho, iterations=30, relTol=fi_tol),
             lambda: O.FISTA(A, reg=O.L1Regularization(lam1), rho=rho, iterations=30, relTol=fi_tol), k, ctx.lib.rls_fista_step_d)):
        ref, S = mk_ref(), mk()
        O.solve(ref, np.array(b))
        x = rls.solve_(S, bd).to_host()
        assert S.state._plan and S.state.iteration == ref.iteration == stop and S.state._done, (name, S.state.iteration, stop)
        assert rel(x, ref.x) < ITER_TOL, (name, rel(x, ref.x))
        assert step(S.state._plan, 3) == 0
        ctx.sync()
        assert rls.solversolution(S).to_host().tobytes() == x.tobytes(), name
