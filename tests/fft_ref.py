"""The checker of the FFT and sampling kernels (csrc/fft.hip): NumPy only.  tests/test_fft_ref.py holds it to
tests/matfree_ref.py and to planted mistakes on the CPU, tests/test_gpu_fft_edges.py holds the device to it.

  launch geometry   pass_plan restates fft_pass's choice of the bundle size (base value, floor of 3 along dimension 1, clamp to the
                    other extent, shrink loop against FFT_LINE_LDS) and what follows from it; fused_fits / fused_threads / use_fused
                    the single-workgroup launch.  The constants carry the C++ names.
  restatement       transform / normal: the kernels' own order of operations -- decimation in frequency with half-spans n/2 ... 1 and
                    the result at the bit-reversed positions; decimation in time from the bit-reversed placement with conjugated
                    twiddles; the shifts as (-1)^k on load and store plus one global minus for an extent of 2 on the forward's way
                    out and the adjoint's way in; one twiddle table of the longer extent read with stride 2^(lgmax - lgn); the scale
                    in the last store; the mask at the bit-reversed positions between the two halves of the normal operator --
                    evaluated in any complex type.  NumPy has no fma: it is NOT the device bit for bit, and nothing asks that.
  references        numpy.fft in complex128 for ComplexF32; for ComplexF64 numpy.fft in long double where NumPy transforms long doubles
                    (LONG_FFT), and for extents <= 64 a DFT matrix formed in long double.  Where neither is better than double the
                    reference makes the same error as the device may, and REF_FACTOR doubles the gate.

The gates (derived, not measured; u = 2^-24 for ComplexF32, 2^-53 for ComplexF64).  A radix-2 transform of 2^t points whose twiddles
carry a relative error mu satisfies (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Theorem 24.2)

    ||y^ - y||_2 / ||y||_2  <=  t eta / (1 - t eta),     eta = mu + gamma_4 (sqrt(2) + mu),     gamma_4 = 4 u / (1 - 4 u).

The table is cos / sin in double rounded once to the working type: mu = 2 u.  A 2-D transform is the same statement with
t = lg1 + lg2 (each dimension is a transform of lines; the factors multiply).  The scale 1 / sqrt(N) is rounded once and multiplies
once: 2 u more.  The sign patterns and permutations are exact.  So

    gate = t eta / (1 - t eta) + 2 u        5.8e-7 (n = 2) ... 6.1e-6 (n = 8192) ComplexF32,  1.1e-15 ... 1.1e-14 (n = 4096) ComplexF64,

relative to ||y||_2 for the whole vector, and |y^_k - y_k| <= gate ||y||_2 for every element of any input.  For a UNIT IMPULSE every
butterfly adds an exact zero, so an output is the input times at most t rounded twiddles (and the scale): the same bound holds
relative to EACH element, |y^_k - y_k| <= gate |y_k|, and | |y^_k| - scale | <= gate scale.  The normal operator F^H diag(mask) F is
two transforms with a contraction between them: with ||F||^2 = N scale^2 its error is within (2 gate + gate^2) N scale^2 ||x||_2
-- relative to ||x||, not to the result, which a mask of one sample makes small.  An input that was itself rounded to the working
type (the pure frequency) is judged against the reference of the ROUNDED input.
"""
import math
from collections import namedtuple

import numpy as np

# ---- csrc/fft.hip ----------------------------------------------------------------------------------------------------------------------
MF_THREADS = 256
MF_MAX_GRID = 2048
GRID_SPAN = MF_THREADS * MF_MAX_GRID   # from this many elements on a thread of a sampling kernel takes a second pass
FFT_LINE_LDS = 64 * 1024
FFT_FUSED_LDS = 160 * 1024 - 512
FFT_FUSED_AUTO_N = 1024
FFT_THREADS = 1024
FFT_LG_BUNDLE = 10
FFT_PASS_MAX_GRID = 4096               # (a literal in fft_pass)

C64, C128 = np.dtype(np.complex64), np.dtype(np.complex128)
DT = [np.complex64, np.complex128]
DT_IDS = ["complex64", "complex128"]
U = {C64: 2.0 ** -24, C128: 2.0 ** -53}
MAX_LINE = {C64: 8192, C128: 4096}
FLAGS = [(True, True), (True, False), (False, True), (False, False)]
ALL_FLAGS_UP_TO = 4096                 # points; beyond: (True, True) and (False, False)

Plan = namedtuple("Plan", "lgb how points threads idle bundles grid bundle_trips stage_trips lds exact_fit")


def lg(n):
    n = int(n)
    if n < 1 or n & (n - 1):
        raise ValueError(f"{n} is no power of two")
    return n.bit_length() - 1


def extents(shape):
    """(lg1, lg2) as rls_fft_create has them: unit extents dropped, a signal has lg2 = 0"""
    ext = [int(s) for s in np.atleast_1d(shape) if int(s) != 1]
    if len(ext) > 2:
        raise ValueError("1-D and 2-D shapes only")
    ext += [1] * (2 - len(ext))
    return lg(ext[0]), lg(ext[1])


def points(shape):
    return int(np.prod(np.atleast_1d(shape)))


def pass_plan(dtype, lg1, lg2, dim1):
    """fft_pass's launch of one dimension.  `how`: the steps that set lgb, in order ("base", then "floor", "clamp", "shrink" where they
    changed it)"""
    es = np.dtype(dtype).itemsize
    lgn, lgo = (lg2, lg1) if dim1 else (lg1, lg2)
    lgb, how = max(FFT_LG_BUNDLE - lgn, 0), ["base"]
    if dim1 and lgb < 3:
        lgb = 3
        how.append("floor")
    if lgb > lgo:
        lgb = lgo
        how.append("clamp")
    while lgb > 0 and (es << (lgn + lgb)) > FFT_LINE_LDS:
        lgb -= 1
        if how[-1] != "shrink":
            how.append("shrink")
    cnt = 1 << (lgn + lgb)
    nt = 64 if cnt // 2 < 64 else min(cnt // 2, FFT_THREADS)
    nb = 1 << (lgo - lgb)
    grid = min(nb, FFT_PASS_MAX_GRID)
    return Plan(lgb, tuple(how), cnt, nt, cnt // 2 < nt, nb, grid, -(-nb // grid), -(-(cnt // 2) // nt) if lgn else 0, cnt * es,
                cnt * es == FFT_LINE_LDS)


def passes(dtype, shape):
    """the launches of a transform of `shape` on the general path"""
    lg1, lg2 = extents(shape)
    return [pass_plan(dtype, lg1, lg2, False)] + ([pass_plan(dtype, lg1, lg2, True)] if lg2 else [])


def fused_fits(dtype, lg1, lg2):
    return (1 << (lg1 + lg2)) * np.dtype(dtype).itemsize <= FFT_FUSED_LDS


def fused_threads(lg1, lg2):
    return 256 if (1 << (lg1 + lg2)) <= 2048 else FFT_THREADS


def use_fused(dtype, lg1, lg2, level):
    """fft_use_fused at ctx.tune(fft_fused=level): what rls_fft_variant reports"""
    if level == 0 or not fused_fits(dtype, lg1, lg2):
        return False
    return level >= 2 or (1 << (lg1 + lg2)) <= FFT_FUSED_AUTO_N


# ---- the shapes of the device tier ------------------------------------------------------------------------------------------------------
def line_lengths(dtype):
    return [(1 << k,) for k in range(lg(MAX_LINE[np.dtype(dtype)]) + 1)]


# images for the general path's regimes (each runs on the single-workgroup path as well where it fits)
GENERAL = {C64: [(4096, 2), (2, 4096), (8, 1024), (16, 2048), (4, 4096), (8, 8192), (8192, 8), (1024, 16)],
           C128: [(4096, 2), (2, 4096), (8, 1024), (16, 2048), (8, 4096), (4096, 8), (1024, 16)]}
# the single-workgroup kernel: both thread counts, an extent of 2 beside the longest line the LDS admits (16384 ComplexF32 /
# 8192 ComplexF64 points are the most that fit), unit extents in every place ((4, 1, 8) acts as (4, 8))
FUSED = {C64: [(32, 64), (64, 64), (8192, 2), (2, 8192), (1, 1), (16, 1), (1, 16), (2, 2), (4, 1, 8)],
         C128: [(32, 64), (64, 64), (1, 1), (16, 1), (1, 16), (2, 2), (4, 1, 8)]}
BIG = (1024, 8192)   # ComplexF32, (True, True) only: the smallest shape whose bundle loop takes a second trip (dimension 0)
NORMAL_SHAPES = [(8, 32), (2, 4096), (64,), (1024, 16)]


def shapes(dtype):
    return line_lengths(dtype) + GENERAL[np.dtype(dtype)] + FUSED[np.dtype(dtype)]


def flags_of(shape):
    return FLAGS if points(shape) <= ALL_FLAGS_UP_TO else [FLAGS[0], FLAGS[3]]


# ---- the gates ---------------------------------------------------------------------------------------------------------------------------
def eta(dtype):
    u = U[np.dtype(dtype)]
    mu, g4 = 2.0 * u, 4.0 * u / (1.0 - 4.0 * u)
    return mu + g4 * (math.sqrt(2.0) + mu)

def gate(dtype, shape):
    t = sum(extents(shape)) * eta(dtype)
    return t / (1.0 - t) + 2.0 * U[np.dtype(dtype)]


def gate_normal(dtype, shape):
    g = gate(dtype, shape)
    return 2.0 * g + g * g


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
PLANTS = ("lgtw", "sign2", "shift_in_only", "mask_natural", "noconj", "scale_twice", "table32", "recurrence")


def real_of(dtype):
    return np.zeros(1, dtype).real.dtype


def bitrev(lgn):
    k = np.arange(1 << lgn)
    r = np.zeros_like(k)
    for b in range(lgn):
        r |= ((k >> b) & 1) << (lgn - 1 - b)
    return r


def _pi(R):
    return 4 * np.arctan(R.type(1)) if R == np.dtype(np.longdouble) else R.type(math.pi)


def twiddles(lgmax, dtype, plant=None):
    """tw[j] = exp(-2 pi i j / 2^lgmax), j < max(2^lgmax / 2, 1): cos / sin in double (long double for a long-double type), rounded
    once, entries 0 and n / 4 exact -- rls_fft_create's table"""
    nt = max((1 << lgmax) // 2, 1)
    R = real_of(dtype)
    H = np.dtype(np.longdouble) if R == np.dtype(np.longdouble) else np.dtype(np.float64)
    a = -2 * _pi(H) * np.arange(nt).astype(H) / H.type(1 << lgmax)
    if plant == "table32":
        a = a.astype(np.float32)
    c, s = np.cos(a), np.sin(a)
    if plant == "recurrence":   # w_j = w_(j-1) w_1 in double
        w = np.ones(nt, np.complex128)
        for j in range(1, nt):
            w[j] = w[j - 1] * complex(c[1], s[1])
        c, s = w.real.copy(), w.imag.copy()
    c[0], s[0] = 1, 0
    if nt >= 2:
        c[nt // 2], s[nt // 2] = 0, -1
    tw = np.empty(nt, dtype)
    tw.real, tw.imag = c.astype(R), s.astype(R)
    return tw


def _stages(S, axis, lgn, tw, lgtw, inv, conj=True):
    """fft_lines along `axis` of S (n1, n2, batch): every stage of half-span h a butterfly (a, u) -> (a + u, (a - u) w) forward,
    (a + u conj(w), a - u conj(w)) adjoint, w = tw[(p 2^(lgn - 1 - lgh)) 2^lgtw]"""
    if lgn == 0:
        return S
    S = np.moveaxis(S, axis, 0)
    shp, n = S.shape, 1 << lgn
    S = S.reshape(n, -1)
    for lgh in (range(lgn) if inv else range(lgn - 1, -1, -1)):
        h = 1 << lgh
        V = S.reshape(n // (2 * h), 2, h, -1)
        w = tw[(np.arange(h) << (lgn - 1 - lgh)) << lgtw][None, :, None]
        a, u = V[:, 0], V[:, 1]
        if not inv:
            lo, hi = a + u, (a - u) * w
        else:
            t = u * (np.conj(w) if conj else w)
            lo, hi = a + t, a - t
        S = np.stack([lo, hi], axis=1).reshape(n, -1)
    return np.moveaxis(S.reshape(shp), 0, axis)


def _signs(S, axis, lgn, global_side, plant):
    """fft_neg: a minus at odd k, and at every k once more for an extent of 2 on the global side"""
    k = np.arange(1 << lgn)
    neg = ((k & 1) != 0) != (global_side and lgn == 1 and plant != "sign2")
    sgn = np.where(neg, -1, 1).astype(real_of(S.dtype))
    return S * (sgn[:, None, None] if axis == 0 else sgn[None, :, None])


def _setup(x, shape, unitary, dtype, plant):
    lg1, lg2 = extents(shape)
    N = 1 << (lg1 + lg2)
    x = np.asarray(x)
    S = np.reshape(x.astype(dtype), (1 << lg1, 1 << lg2, -1), order="F")
    R = real_of(dtype)
    one = R.type(1)
    scale = (one / np.sqrt(R.type(N)) if R == np.dtype(np.longdouble) else R.type(1.0 / math.sqrt(N))) if unitary else one
    lgmax = max(lg1, lg2)
    return lg1, lg2, N, S, scale, lgmax, twiddles(lgmax, dtype, plant), x.ndim == 2


def _result(S, N, batch):
    y = np.reshape(S, (N, -1), order="F")
    return y if batch else y[:, 0]


def transform(x, shape, shift=True, unitary=True, adjoint=False, dtype=np.complex128, plant=None):
    """F x (adjoint: F^H x) of a column-major image x (or of the columns of an (N, batch) array) in the kernels' order of operations,
    every operation in `dtype`.  `plant`: one of PLANTS, a mistake made on purpose"""
    lg1, lg2, N, S, scale, lgmax, tw, batch = _setup(x, shape, unitary, dtype, plant)
    dims = [(0, lg1)] + ([(1, lg2)] if lg2 else [])
    if adjoint:
        dims.reverse()
    for i, (axis, lgn) in enumerate(dims):
        lgtw = 0 if plant == "lgtw" else lgmax - lgn
        rev = bitrev(lgn)
        if shift:
            S = _signs(S, axis, lgn, adjoint, plant)
        if adjoint:   # s[rev(k)] = x[k]
            S = np.take(S, rev, axis=axis)
        S = _stages(S, axis, lgn, tw, lgtw, adjoint, conj=plant != "noconj")
        if not adjoint:   # y[k] = s[rev(k)]
            S = np.take(S, rev, axis=axis)
        if shift and plant != "shift_in_only":
            S = _signs(S, axis, lgn, not adjoint, plant)
        if i == len(dims) - 1 or plant == "scale_twice":
            S = S * scale
    return _result(S, N, batch)


def normal(x, mask, shape, shift=True, unitary=True, dtype=np.complex128, plant=None):
    """F^H diag(mask) F x as the single-workgroup kernel runs it: no permutation, the mask (behind the scale) at the bit-reversed
    positions, neither global sign"""
    lg1, lg2, N, S, scale, lgmax, tw, batch = _setup(x, shape, unitary, dtype, plant)
    l1, l2 = (0, 0) if plant == "lgtw" else (lgmax - lg1, lgmax - lg2)
    if shift:
        S = _signs(_signs(S, 0, lg1, False, plant), 1, lg2, False, plant)
    S = _stages(_stages(S, 0, lg1, tw, l1, False), 1, lg2, tw, l2, False)
    M = np.reshape(np.asarray(mask), (1 << lg1, 1 << lg2), order="F").astype(real_of(dtype))
    if plant != "mask_natural":
        M = M[bitrev(lg1)][:, bitrev(lg2)]
    S = (S * scale) * M[:, :, None]
    S = _stages(_stages(S, 1, lg2, tw, l2, True, plant != "noconj"), 0, lg1, tw, l1, True, plant != "noconj")
    if shift:
        S = _signs(_signs(S, 0, lg1, False, plant), 1, lg2, False, plant)
    return _result(S * scale, N, batch)


# ---- references --------------------------------------------------------------------------------------------------------------------------
LD, CLD = np.dtype(np.longdouble), np.dtype(np.clongdouble)
LONG = bool(np.finfo(np.longdouble).eps < 2.0 ** -60)
LONG_FFT = LONG and np.fft.fft(np.zeros(2, np.clongdouble)).dtype == CLD
DFT_MAX = 64


def dft_matrix(n, shift, adjoint):
    """the n x n matrix of one dimension, formed in long double: exp(-+ 2 pi i (j k mod n) / n), rolled by n / 2 both ways for the shifts"""
    k = np.arange(n)
    a = 2 * _pi(LD) * ((np.outer(k, k) % n).astype(LD)) / LD.type(n)
    W = np.empty((n, n), CLD)
    W.real, W.imag = np.cos(a), (np.sin(a) if adjoint else -np.sin(a))
    if shift:
        W = np.roll(np.roll(W, n // 2, axis=0), n // 2, axis=1)
    return W


def by_dft_matrix(x, shape, shift=True, unitary=True, adjoint=False):
    lg1, lg2 = extents(shape)
    N = 1 << (lg1 + lg2)
    x = np.asarray(x)
    X = np.reshape(x.astype(CLD), (1 << lg1, 1 << lg2, -1), order="F")
    Y = np.einsum("kj,jlb->klb", dft_matrix(1 << lg1, shift, adjoint), X)
    Y = np.einsum("lj,kjb->klb", dft_matrix(1 << lg2, shift, adjoint), Y)
    if unitary:
        Y = Y / np.sqrt(LD.type(N))
    return _result(Y, N, x.ndim == 2)


def ref_type(dtype):
    return np.dtype(np.complex128) if np.dtype(dtype) == C64 else (CLD if LONG else np.dtype(np.complex128))


def ref_factor(dtype, shape):
    """what the gate is multiplied by: 2 where the reference is no better than the working type (it may err as much as the device)"""
    if np.dtype(dtype) == C64 or LONG_FFT or (LONG and max(1 << e for e in extents(shape)) <= DFT_MAX):
        return 1.0
    return 2.0


def reference(x, shape, shift=True, unitary=True, adjoint=False, dtype=np.complex128):
    """F x / F^H x of x (or its columns) for judging a result of element type `dtype`: see the module docstring"""
    lg1, lg2 = extents(shape)
    N = 1 << (lg1 + lg2)
    H = ref_type(dtype)
    if np.dtype(dtype) == C128 and LONG and max(1 << lg1, 1 << lg2) <= DFT_MAX:
        return by_dft_matrix(x, shape, shift, unitary, adjoint)
    if H == CLD and not LONG_FFT:
        H = np.dtype(np.complex128)
    x = np.asarray(x)
    X = np.reshape(x.astype(H), (1 << lg1, 1 << lg2, -1), order="F")
    if shift:
        X = np.fft.ifftshift(X, axes=(0, 1))
    X = np.fft.ifftn(X, axes=(0, 1), norm="forward") if adjoint else np.fft.fftn(X, axes=(0, 1))
    if shift:
        X = np.fft.fftshift(X, axes=(0, 1))
    if unitary:
        X = X / np.sqrt(real_of(H).type(N))
    return _result(X, N, x.ndim == 2)


def reference_normal(x, mask, shape, shift=True, unitary=True, dtype=np.complex128):
    y = reference(x, shape, shift, unitary, False, dtype)
    m = np.asarray(mask).astype(real_of(y.dtype))
    return reference(y * (m[:, None] if y.ndim == 2 else m), shape, shift, unitary, True, dtype)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def nonself(shape, exclude=()):
    """the first index whose per-dimension bit reversal is not itself (not among `exclude` where there is a choice); None: there is none"""
    lg1, lg2 = extents(shape)
    r1, r2 = bitrev(lg1), bitrev(lg2)
    first = None
    for i in range(min(1 << (lg1 + lg2), 4096)):
        k1, k2 = i & ((1 << lg1) - 1), i >> lg1
        if (r1[k1], r2[k2]) != (k1, k2):
            if i not in exclude:
                return i
            first = i if first is None else first
    return first


def impulse_positions(shape):
    """0, 1, n1 - 1, n1, N / 2, N - 1 and one index whose bit reversal is not itself"""
    lg1, lg2 = extents(shape)
    n1, N = 1 << lg1, 1 << (lg1 + lg2)
    pos = sorted({p for p in (0, 1, n1 - 1, n1, N // 2, N - 1) if 0 <= p < N})
    ns = nonself(shape, pos)
    return sorted(set(pos) | ({ns} if ns is not None else set()))


def gauss(dtype, n, seed):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) / math.sqrt(2.0)).astype(dtype)


def inputs(dtype, shape, shift, unitary, adjoint, kinds=("random", "impulse", "constant", "frequency")):
    """(names, X): the columns of X (N, len(names)) are one dense random vector, the unit impulses, the constant vector and one pure
    frequency -- the OTHER transform's image of a unit impulse, rounded to `dtype`, which this transform turns back into an impulse"""
    N = points(shape)
    names, cols = [], []
    if "random" in kinds:
        names.append("random")
        cols.append(gauss(dtype, N, 1000 + sum(extents(shape)) * 7 + extents(shape)[0]))
    if "impulse" in kinds:
        for p in (impulse_positions(shape) if kinds.count("impulse") == 1 else []):
            names.append(f"impulse@{p}")
            e = np.zeros(N, dtype)
            e[p] = 1
            cols.append(e)
    for k in kinds:
        if isinstance(k, tuple) and k[0] == "impulse":
            names.append(f"impulse@{k[1]}")
            e = np.zeros(N, dtype)
            e[k[1]] = 1
            cols.append(e)
    if "constant" in kinds:
        names.append("constant")
        cols.append(np.ones(N, dtype))
    if "frequency" in kinds:
        j = nonself(shape)
        j = N - 1 if j is None else j
        e = np.zeros(N, dtype)
        e[j] = 1
        names.append(f"frequency@{j}")
        cols.append(reference(e, shape, shift, unitary, not adjoint, dtype).astype(dtype))
    return names, np.stack(cols, axis=1)


def peak_of_constant(shape, shift):
    lg1, lg2 = extents(shape)
    n1, n2 = 1 << lg1, 1 << lg2
    return ((n1 // 2) if shift else 0) + n1 * ((n2 // 2) if shift else 0)


def judge(dtype, shape, shift, unitary, names, X, got, want, factor=1.0):
    """the checks of one batch as (label, error, bound) triples, error <= bound entry by entry: got (N, batch) is the result under
    test, want the reference of the same columns.  Module docstring for the bounds."""
    N, u = points(shape), U[np.dtype(dtype)]
    g = gate(dtype, shape) * factor
    s = 1.0 / math.sqrt(N) if unitary else 1.0
    H = want.dtype
    out = []
    for c, name in enumerate(names):
        y, w = got[:, c].astype(H), want[:, c]
        err = np.abs(y - w).astype(np.float64)
        nw = float(np.sqrt(np.sum(np.abs(w).astype(np.float64) ** 2)))
        out.append((f"{name} norm", [float(np.sqrt(np.sum(err ** 2)))], [g * nw]))
        out.append((f"{name} elements", err, np.full(N, g * nw)))
        if name.startswith("impulse"):
            out.append((f"{name} element-relative", err, g * np.abs(w).astype(np.float64)))
            out.append((f"{name} modulus", np.abs(np.abs(y).astype(np.float64) - s), np.full(N, g * s)))
        elif name == "constant":
            p = peak_of_constant(shape, shift)
            rest = np.abs(y).astype(np.float64)
            out.append((f"{name} peak", [abs(complex(y[p]) - N * s)], [g * N * s]))
            rest[p] = 0.0
            out.append((f"{name} zeros", rest, np.full(N, g * N * s)))
        elif name.startswith("frequency"):
            j = int(name.split("@")[1])
            rest = np.abs(y).astype(np.float64)
            out.append((f"{name} peak", [abs(complex(y[j]) - N * s * s)], [(g + u) * N * s * s]))
            rest[j] = 0.0
            out.append((f"{name} zeros", rest, np.full(N, (g + u) * N * s * s)))
    return out


# ---- sampling ----------------------------------------------------------------------------------------------------------------------------
def ints(dtype, n, seed):
    """small integers: every product and sum of the alpha / beta form is exact in every element type"""
    rng = np.random.default_rng(seed)
    v = rng.integers(-8, 9, n).astype(np.float64)
    if np.dtype(dtype).kind == "c":
        v = v + 1j * rng.integers(-8, 9, n)
    return v.astype(dtype)


def masks(shape, seed=3):
    """(name, pattern) for the normal operator: all ones, one sample at 0, at N - 1 and at an index whose reversal differs, a random third"""
    N = points(shape)
    rng = np.random.default_rng(seed + N)
    ns = nonself(shape, (0, N - 1))
    out = [("ones", np.arange(N)), ("one@0", np.array([0])), (f"one@{N - 1}", np.array([N - 1]))]
    if ns is not None:
        out.append((f"one@{ns}", np.array([ns])))
    out.append(("third", np.sort(rng.choice(N, N // 3, replace=False))))
    return [(n, p.astype(np.int32)) for n, p in out]
