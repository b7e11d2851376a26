"""The blocked Cholesky of csrc/direct.hip restated on the CPU, the integer systems on which it is exact, and the componentwise
bounds it is held to on everything else.  No device is needed here; tests/test_direct_ref.py checks this module against itself and
numpy, tests/test_gpu_direct_edges.py holds the kernels to it.

Integer systems
    G = L L^H with L of small (Gaussian) integers whose diagonal is 1, 2 or 4.  Every pivot is then 1, 4 or 16, `sqrtf` and
    `1.0f / sqrtf` of those are exact, a strip entry is an integer multiple of the pivot root before it is scaled, and every product,
    Schur complement and partial sum of the matrix cores is an integer.  Integers below 2^24 are Float32 numbers and their sums and
    products are exact whatever the order (and whether or not a product is fused into the sum), so the Float32 factorisation returns
    L bit for bit and the solve of B = G X for an integer X returns X bit for bit.  `blocked_cholesky(..., np.float32)` records the
    largest sum of absolute values any entry's update could have formed (`peak`): while it stays below 2^24, bit equality is a
    fair gate.  Exact cancellation gives +0 in round-to-nearest and nothing here produces -0 (G is normalised to +0), so "bit for bit"
    includes the sign of zero.

Bounds on non-integer data (u = 2^-24, gamma_k = k u / (1 - k u); Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed.)
    factor    |G + lambda I - L L^H| <= gamma_{n+4} |L| |L^H|                     (Thm 10.3: gamma_{n+1})
    solve     |B - (G + lambda I) X| <= gamma_{3n+6} |L| |L^H| |X|                (Thm 10.4: gamma_{3n+1})
    entrywise, with the COMPUTED L and X, and n = 64 ceil(N / 64): the contraction length of the padded system the kernels run on (the
    padding contributes exact zeros; n >= N only loosens the bound by the padding).  Both theorems rest on Lemma 8.4: if
    y = (c - sum_{i<k} a_i b_i) / b_k is evaluated in ANY order, then b_k y (1 + theta_k) = c - sum a_i b_i (1 + theta_i) with
    |theta_i| <= gamma_i; a fused multiply-add only removes roundings, so the order in which the matrix cores sum and the
    -ffp-contract=fast build do not matter.  What the constants pay for beyond the textbook algorithm:
      factor, c = 4:  1  lambda is added to the diagonal in Float32 by the load kernel;
                      1  an entry is multiplied with the rounded reciprocal root rs = fl(1 / fl(sqrt d)) instead of divided by the
                         root: l = s rs (1 + d1) = s (1 + d1)(1 + d2) / fl(sqrt d), one rounding more than one division;
                      2  the stored diagonal is fl(sqrt d), so l_jj^2 = d (1 + d3)^2 (this is the theorem's own "+1", counted twice
                         because no division absorbs it here).
      solve,  c = 6:  (n + 4) for the factor and (n + 1) for each substitution, which multiplies with fl(1 / l_kk) (one rounding
                      more than Lemma 8.4's division): (L + dL1)(L^H + dL2) y = b, and gamma_a + 2 gamma_b + gamma_b^2 <=
                      gamma_{a + 2b} (Lemma 3.3), a = n + 4, b = n + 1.
    ComplexF32: a complex product is four real products and two sums, and the kernels scale with REAL reciprocals.  Each component of
    sum_k l_ik conj(l_jk) is a real sum of 2n products whose absolute values add up to no more than sum_k |l_ik| |l_jk| (Cauchy-Schwarz:
    |a_r b_r| + |a_i b_i| <= |a| |b|), so n becomes 2n per component and the modulus of the two components' errors is at most sqrt 2
    times the component bound:
      factor  sqrt 2 gamma_{2n+4} |L| |L^H|,   solve  sqrt 2 gamma_{6n+6} |L| |L^H| |X|     (|.|: the complex modulus).
    These complex constants are deliberately generous, not tight: counting every component as a worst-case real sum of 2n products
    and then taking sqrt 2 is about 2.8 times looser than Higham's constant for a complex inner product (Lemma 3.5), and all the
    bounds here are worst-case ones that rounding errors rarely approach.  They are a gate against a wrong algorithm (a planted
    mistake exceeds them by 10^2 .. 10^4), not a measure of accuracy; the integer systems are the sharp gate.
    Division and square root: csrc/Makefile builds with -O3 -ffp-contract=fast and neither -ffast-math nor
    -fno-hip-fp32-correctly-rounded-divide-sqrt, so `1.0f / x` and `sqrtf` are the correctly rounded ones (the HIP default); nothing
    is added to c for an approximation.
    The checks evaluate the residuals in float64 from the Float32 data; that evaluation's own error, (n + 2) 2^-53 |G| |X|, is added to
    the solve bound (it is nine orders of magnitude below it).  None of these numbers is fitted to a device's output."""
import math

import numpy as np

DB = 64                 # block size of direct.hip
U = 2.0 ** -24
EXACT = 2.0 ** 24       # integers below this are Float32 numbers
MISTAKES = ("conj_dropped", "previous_pivot", "subtile_skipped", "back_uses_L")


def padded(N):
    return -(-N // DB) * DB


def is_cplx(dt):
    return np.dtype(dt).kind == "c"


def wide(dt):
    return np.complex128 if is_cplx(dt) else np.float64


def _ctype(like, real_type):
    real_type = np.dtype(real_type)
    if not np.iscomplexobj(like):
        return real_type
    return np.dtype(np.complex64 if real_type == np.float32 else np.complex128)


# ---- reading a factor back ----------------------------------------------------------------------------------------------------------
def split(Wbuf, ld):
    """(the padded square, the NB diagonal tiles [j, row, column]) of the plan's factor allocation read back as one flat array"""
    Wbuf = np.asarray(Wbuf)
    nb = ld // DB
    assert Wbuf.size == ld * ld + ld * DB, (Wbuf.size, ld)
    return Wbuf[: ld * ld].reshape((ld, ld), order="F"), Wbuf[ld * ld:].reshape((nb, DB, DB)).transpose(0, 2, 1)


def assemble_padded(Wbuf, ld):
    W, tiles = split(Wbuf, ld)
    L = np.tril(W, -1)
    for j in range(ld // DB):
        L[j * DB:(j + 1) * DB, j * DB:(j + 1) * DB] = tiles[j]
    return L


def assemble(Wbuf, ld, N):
    """the N x N lower-triangular L: strict lower-triangle tiles from W, diagonal blocks from the tile buffer"""
    return assemble_padded(Wbuf, ld)[:N, :N]


def first_difference(got, want):
    """None, or '(row, column, block)' text of the first entry (column-major) whose BITS differ"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    if got.tobytes() == want.tobytes():
        return None
    it = np.dtype(f"u{got.dtype.itemsize}")
    diff = np.asfortranarray(got).view(it) != np.asfortranarray(want).view(it)
    if got.ndim == 1:
        r = int(np.nonzero(diff)[0][0])
        return f"first difference at {r}: got {got[r]!r}, want {want[r]!r}; {int(diff.sum())} entries differ"
    c = int(np.nonzero(diff.any(axis=0))[0][0])
    r = int(np.nonzero(diff[:, c])[0][0])
    return (f"first difference at (row {r}, column {c}), block ({r // DB}, {c // DB}): got {got[r, c]!r}, want {want[r, c]!r}; "
            f"{int(diff.sum())} entries differ")


# ---- integer systems ----------------------------------------------------------------------------------------------------------------
def _small(rng, shape, cplx, density):
    v = rng.integers(-1, 2, shape).astype(np.float64) * (rng.random(shape) < density)
    if cplx:
        v = v + 1j * (rng.integers(-1, 2, shape) * (rng.random(shape) < density))
    return v


def integer_factor(N, dtype, seed, density=0.7, K=1, band=6):
    """(L, G = L L^H, X, B = G X) in float64 / complex128: L has its diagonal in {1, 2, 4} and off-diagonal parts in {-1, 0, 1}: a
    band, plus three dense rows and every sixteenth column dense, which cross every 64-block boundary.  X: N x K integers with parts in -3 .. 3."""
    cplx = is_cplx(dtype)
    rng = np.random.default_rng(seed)
    dense = _small(rng, (N, N), cplx, density)
    i, j = np.indices((N, N))
    keep = (i - j <= band)
    for r in sorted({N - 1, N // 2, (2 * N) // 3}):      # dense rows (to the left of the diagonal) ...
        keep[r, :] = True
    keep[:, ::16] = True                                 # ... and dense columns (below it), one per 16: every 16 x 16 sub-tile of
    #                                                      every trailing update then has something to subtract
    L = np.tril(dense * keep, -1) + np.diag(rng.choice([1.0, 2.0, 4.0], N))
    L = L.astype(wide(dtype))
    G = L @ L.conj().T + 0.0                                # (+ 0.0: no -0 anywhere)
    X = rng.integers(-3, 4, (N, K)).astype(np.float64)
    if cplx:
        X = X + 1j * rng.integers(-3, 4, (N, K))
    X = X.astype(wide(dtype))
    B = G @ X + 0.0
    return L, G, X, B


def planted_pivot(N, dtype, col, kind, seed=5):
    """(G, L): an integer system whose first pivot that is not strictly positive and finite is exactly the one of 1-based column `col`.
    kind 'zero' / 'negative': G = L D L^H with D = I but D[col] = 0 / -4, so the first col - 1 columns of its factor are L's and the
    pivot is 0 / -4 L[col, col]^2.  'inf' / 'nan': G = L L^H with the value planted in G[col, col] (it survives every update)."""
    L, G, _, _ = integer_factor(N, dtype, seed)
    c = col - 1
    if kind in ("zero", "negative"):
        D = np.ones(N)
        D[c] = 0.0 if kind == "zero" else -4.0
        G = (L * D) @ L.conj().T + 0.0
    else:
        G = G.copy()
        G[c, c] = {"inf": np.inf, "nan": np.nan}[kind]
    return G, L


def random_hpd(N, dtype, cond, seed, K=1):
    """(G, X, B) in the ELEMENT type: G = Q diag(s) Q^H rounded (s from 1 down to 1 / cond, logarithmically), Hermitian with a
    real diagonal after the rounding; X Gaussian; B = G X rounded."""
    rng = np.random.default_rng(seed)
    Z = rng.standard_normal((N, N))
    if is_cplx(dtype):
        Z = Z + 1j * rng.standard_normal((N, N))
    Q, _ = np.linalg.qr(Z)
    s = np.logspace(0.0, -math.log10(cond), N) if N > 1 else np.ones(1)
    G = ((Q * s) @ Q.conj().T).astype(dtype)
    G = np.tril(G, -1) + np.tril(G, -1).conj().T + np.diag(G.diagonal().real).astype(dtype)
    X = rng.standard_normal((N, K))
    if is_cplx(dtype):
        X = (X + 1j * rng.standard_normal((N, K))) / math.sqrt(2.0)
    X = X.astype(dtype)
    B = (G.astype(wide(dtype)) @ X.astype(wide(dtype))).astype(dtype)
    return G, X, B


# ---- the algorithm of direct.hip ------------------------------------------------------------------------------------------------------
def _absparts(v):
    return np.abs(v.real) + np.abs(v.imag) if np.iscomplexobj(v) else np.abs(v)


def blocked_cholesky(G, lam, real_type, mistake=None):
    """direct.hip restated in `real_type` arithmetic: W = [G + lambda I, 0; 0, I] from G's lower triangle and the real part of its
    diagonal; right-looking over 64-blocks; inside a panel the pivots stay in place, a column is scaled with rs = 1 / sqrt(d) (the
    reciprocal root, then a product), and the diagonal tile gets sqrt of the pivots at the end; W's own diagonal blocks are never
    written.  Returns a dict: info (0, or the 1-based column of the first pivot that is not > 0 and finite), W (padded square as the
    kernels leave it), tiles [j, row, column], L (N x N; None when info != 0), peak (see the module docstring).
    `mistake`: one of MISTAKES, planted for tests/test_direct_ref.py; 'back_uses_L' belongs to blocked_solve."""
    rt = np.dtype(real_type).type
    G = np.asarray(G)
    N = G.shape[0]
    ct = _ctype(G, real_type)
    ld, nb = padded(N), padded(N) // DB
    fmax = rt(np.finfo(rt).max)
    W = np.zeros((ld, ld), dtype=ct)
    W[:N, :N] = np.tril(G, -1).astype(ct)
    with np.errstate(invalid="ignore", over="ignore"):
        diag = G.diagonal().real.astype(rt) + rt(lam)
    W[np.arange(N), np.arange(N)] = diag
    W[np.arange(N, ld), np.arange(N, ld)] = 1
    tiles = np.zeros((nb, DB, DB), dtype=ct)
    out = {"info": 0, "W": W, "tiles": tiles, "L": None, "peak": float(np.nanmax(_absparts(W[np.isfinite(W)]), initial=0.0))}

    def peak(v):
        v = v[np.isfinite(v)]
        if v.size:
            out["peak"] = max(out["peak"], float(v.max()))

    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(nb):
            d0 = j * DB
            D = W[d0:d0 + DB, d0:d0 + DB].copy()
            S = W[d0 + DB:, d0:d0 + DB].copy()
            rs_prev = None
            for k in range(DB):
                d = rt(D[k, k].real)
                if not (d > 0 and d <= fmax):
                    out["info"] = d0 + k + 1
                    return out
                rs = rt(1) / np.sqrt(d)
                D[k + 1:, k] *= rs
                S[:, k] *= rs_prev if (mistake == "previous_pivot" and rs_prev is not None) else rs
                rs_prev = rs
                lc = D[k + 1:, k].conj()
                peak(_absparts(D[k + 1:, k + 1:]) + np.outer(_absparts(D[k + 1:, k]), _absparts(lc)))
                peak(_absparts(S[:, k + 1:]) + np.outer(_absparts(S[:, k]), _absparts(lc)))
                D[k + 1:, k + 1:] -= np.tril(np.outer(D[k + 1:, k], lc))
                S[:, k + 1:] -= np.outer(S[:, k], lc)
            tiles[j] = np.tril(D, -1)
            tiles[j][np.arange(DB), np.arange(DB)] = np.sqrt(D.diagonal().real)
            W[d0 + DB:, d0:d0 + DB] = S
            # the trailing update, tile by tile on the lower triangle: C -= P Q^H
            for p in range(nb - 1 - j):
                r0 = d0 + DB * (1 + p)
                P = W[r0:r0 + DB, d0:d0 + DB]
                for q in range(p + 1):
                    c0 = d0 + DB * (1 + q)
                    Q = W[c0:c0 + DB, d0:d0 + DB]
                    QH = Q.T if mistake == "conj_dropped" else Q.conj().T
                    peak(_absparts(W[r0:r0 + DB, c0:c0 + DB]) + _absparts(P).astype(np.float64) @ _absparts(QH).astype(np.float64))
                    upd = P @ QH
                    if mistake == "subtile_skipped" and j == 0 and p == min(1, nb - 2) and q == 0:
                        upd[16:32, 32:48] = 0          # tile (2, 1) where there is one: wave 1, sub-tile 2
                    W[r0:r0 + DB, c0:c0 + DB] -= upd
    L = np.tril(W, -1)
    for j in range(nb):
        L[j * DB:(j + 1) * DB, j * DB:(j + 1) * DB] = tiles[j]
    out["L"] = L[:N, :N]
    return out


def project(X, proj):
    """RLS_PROJ_NONE / REAL / POSITIVE (0 / 1 / 2) as the backward pass's store applies it: imaginary part +0"""
    if proj == 0:
        return X
    re = X.real.copy()
    if proj == 2:
        re[re < 0] = 0
    return re.astype(X.dtype)


def blocked_solve(L, B, real_type, proj=0, mistake=None):
    """chol_trsm_kernel restated: L Y = B forward, L^H X = Y backward, one 64-block after the other on the padded system; inside a
    block a substitution that multiplies with rd = 1 / l_kk; the other row blocks get the block's contribution subtracted.
    Returns (X, peak)."""
    rt = np.dtype(real_type).type
    N, K = B.shape
    ct = _ctype(L, real_type)
    ld, nb = padded(N), padded(N) // DB
    Lp = np.eye(ld, dtype=ct)
    Lp[:N, :N] = L
    Y = np.zeros((ld, K), dtype=ct)
    Y[:N] = B
    pk = [float(_absparts(Y).max(initial=0.0))]

    def sub(dst, T, v):
        pk[0] = max(pk[0], float((_absparts(dst) + _absparts(T).astype(np.float64) @ _absparts(v).astype(np.float64)).max(initial=0.0)))
        dst -= T @ v

    for back in (False, True):
        for j in (range(nb - 1, -1, -1) if back else range(nb)):
            d0 = j * DB
            T = Lp[d0:d0 + DB, d0:d0 + DB]
            if back:
                T = T if (mistake == "back_uses_L" and j == 0) else T.conj().T
            y = Y[d0:d0 + DB]
            for k in (range(DB - 1, -1, -1) if back else range(DB)):
                y[k] = (rt(1) / rt(T[k, k].real)) * y[k]
                rows = slice(0, k) if back else slice(k + 1, DB)
                sub(y[rows], T[rows, k:k + 1], y[k:k + 1])
            for r in (range(j) if back else range(j + 1, nb)):
                b0 = r * DB
                C = Lp[d0:d0 + DB, b0:b0 + DB].conj().T if back else Lp[b0:b0 + DB, d0:d0 + DB]
                sub(Y[b0:b0 + DB], C, y)
    return project(Y[:N], proj), pk[0]


# ---- the bounds -----------------------------------------------------------------------------------------------------------------------
def gamma(k):
    assert k * U < 1
    return k * U / (1 - k * U)


def factor_gamma(N, dtype):
    n = padded(N)
    return math.sqrt(2.0) * gamma(2 * n + 4) if is_cplx(dtype) else gamma(n + 4)


def solve_gamma(N, dtype):
    n = padded(N)
    return math.sqrt(2.0) * gamma(6 * n + 6) if is_cplx(dtype) else gamma(3 * n + 6)


def hermitian(G):
    """the matrix the kernels factor: G's lower triangle mirrored, the real part of its diagonal (float64 / complex128)"""
    G = np.asarray(G).astype(wide(G.dtype))
    return np.tril(G, -1) + np.tril(G, -1).conj().T + np.diag(G.diagonal().real)


def factor_ratio(G, lam, L):
    """max over entries of |G + lambda I - L L^H| / (factor_gamma |L| |L^H|); <= 1 is the gate.  lambda as the Float32 it crosses as."""
    N = G.shape[0]
    A = hermitian(G) + float(np.float32(lam)) * np.eye(N)
    L = np.asarray(L).astype(A.dtype)
    res = np.abs(A - L @ L.conj().T)
    bound = factor_gamma(N, G.dtype) * (np.abs(L) @ np.abs(L).T)
    return _worst(res, bound)


def solve_ratio(G, lam, L, B, X):
    """max over entries of |B - (G + lambda I) X| / (solve_gamma |L| |L^H| |X| + the float64 evaluation's own error)"""
    N = G.shape[0]
    A = hermitian(G) + float(np.float32(lam)) * np.eye(N)
    L, B, X = (np.asarray(v).astype(A.dtype) for v in (L, B, X))
    res = np.abs(B - A @ X)
    bound = solve_gamma(N, G.dtype) * (np.abs(L) @ (np.abs(L).T @ np.abs(X))) + (N + 2) * 2.0 ** -53 * (np.abs(A) @ np.abs(X) + np.abs(B))
    return _worst(res, bound)


def _worst(res, bound):
    if not (np.all(np.isfinite(res)) and np.all(np.isfinite(bound))):
        return math.inf
    return float(np.max(res / np.maximum(bound, 1e-300))) if res.size else 0.0


# ---- the cases of tests/test_gpu_direct_edges.py (asserted exact on the CPU by tests/test_direct_ref.py) -------------------------------
DTYPES = [np.float32, np.complex64]
FACTOR_N = [1, 2, 63, 64, 65, 127, 128, 129, 192, 257, 321]
SOLVE_N = [1, 64, 65, 129, 257]
SOLVE_K = [1, 15, 16, 17, 32, 33]
KMAX = 33
PIVOT_N = 130
PIVOT_COLS = [1, 2, 63, 64, 65, 128, 129, PIVOT_N]
PIVOT_KINDS = ["zero", "negative", "inf", "nan"]
BOUND_N = [63, 65, 200, 257]
BOUND_COND = [10.0, 1e3]
BOUND_LAM = [0.0, 0.5]
BOUND_K = 17
SHIFT = 3.0   # the lambda of the shifted exact-factor case: G - 3 I is factored with lambda = 3

_cache = {}


def integer_case(N, dtype):
    """the one integer system per (N, element type) every GPU test shares: (L, G, X with KMAX columns, B), read-only"""
    key = ("int", N, np.dtype(dtype))
    if key not in _cache:
        _cache[key] = integer_factor(N, dtype, seed=1000 + N, K=KMAX)
        for a in _cache[key]:
            a.setflags(write=False)
    return _cache[key]


def bound_case(N, dtype, cond):
    key = ("hpd", N, np.dtype(dtype), cond)
    if key not in _cache:
        _cache[key] = random_hpd(N, dtype, cond, seed=2000 + N + int(cond), K=BOUND_K)
        for a in _cache[key]:
            a.setflags(write=False)
    return _cache[key]


def repairing_lambda(G):
    """a lambda (a small integer, exact in Float32) that makes a 'zero' / 'negative' planted system positive definite with room:
    8 more than the magnitude of the most negative eigenvalue, rounded up"""
    w = np.linalg.eigvalsh(hermitian(G))
    return float(math.ceil(max(0.0, -w.min())) + 8)
