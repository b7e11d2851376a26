"""The Float32 / ComplexF32 vector kernels of csrc/blas1.hip, csrc/prox.hip, csrc/nested.hip and the two ADMM bookkeeping kernels of
csrc/solvers.hip (admm_pre_kernel, admm_post_kernel), restated in NumPy: the checker of tests/test_vec_ref.py (CPU) and of
tests/test_gpu_vec_edges.py (device), which share the inputs, the lengths and the gates below.

Every operation is ONE set of lines run at `prec` = 64 (float64 / complex128: the reference value) or 32 (float32 / complex64, one
rounding per operation, nothing fused: what a correct Float32 implementation may return).  The prox maps, L21 and the transforms
call oracle/rls_oracle.py at either precision, so their semantics are the oracle's reading of the reference: the L1 eps on the real
part alone, the ragged tail of an L21 group, the `>=` of restore_outside.  Two of them need a word:
  prox_l1   the Float32 path carries eps(Float32); O.prox_l1 takes the eps of its argument's type.  The map is homogeneous in
            (x, lambda, eps), so O.prox_l1(s x, s lambda) / s with s = eps(Float64) / eps(Float32) = 2^-29 IS the float64 value of
            the Float32 operation, and s is a power of two: the scaling rounds nothing.  (At float32 s = 1.)
  prox_l21  the kernel sums a group's squares serially in Float32; the oracle sums them in float64 whatever the type.  The reference
            value is O.prox_l21 / O.norm_l21 on the float64 data; the float32 evaluation is the serial restatement l21_lines()
            below, whose float64 run test_vec_ref.py holds to the oracle.

Gates.  u = 2^-24.  gam(k) = k u / (1 - k u).  Per element |got - want| <= gam(k) S, S = sum |coef| |operand| over the output's
terms and k the roundings on the longest path of the kernel's own arithmetic.  The library is built with -ffp-contract=fast: every
a * b + c the source does not pin may or may not become one fused multiply-add, so k is counted for whichever evaluation has more
roundings (the products of one sum count once together: their errors add up to u sum |term| <= u S; every addition once: u |partial
sum| <= u S), and a chain of fused multiply-adds counts each of its links.
  bit for bit   one correctly rounded operation per element, or none: fill, real scal, real lincomb without y, the positive / real
                projections, gather / scatter, split / merge, clamp, restore_outside, xold = x of admm_pre, shift_scale mode 1
                (f32_mul, f32_add: single instructions) and mode 0 (f32_sub, then a division that the build leaves correctly
                rounded: no extra ulp to count).
  complex a x   Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., (3.13): sqrt 2 gam(2) |a| |x|, contracted or not.
  axpy          real   fmaf(a, x, y) on the device, a x then + y here:                                       gam(2) (|a||x| + |y|)
                complex  two chained fmaf per part on the device (2), products / subtraction / sum here (3); the modulus of the
                         two parts' sums is at most sqrt 2 |a||x| + |y| (Cauchy-Schwarz, Minkowski):  gam(3) (sqrt 2 |a||x| + |y|)
  lincomb       real   a x, then fmaf(b, y, .), or three roundings of which the two products count once:   gam(2) (|a||x| + |b||y|)
                complex  the product's own two roundings, then two chained fmaf per part:         gam(4) sqrt 2 (|a||x| + |b||y|)
  prox_l1       out = sh (v + eps) / (a + eps), a = |v|, sh = max(a - lambda, 0) <= a (nothing here is of the form a b + c)
                real     a exact; sh, v + eps, the product, a + eps, the quotient: five relative roundings:                gam(5) sh
                complex  a = hypotf = sqrt(fmaf(re, re, im im)) of the scaled parts: 2 u on the sum, u of it and the root's own
                         rounding on a: 2 u.  sh is off by 2 u a + u sh; a + eps by 3 u, v.re + eps, the product and
                         the quotient by u each, on a value of modulus <= sh:                                gam(2) a + gam(7) sh
  prox_l2       the factor and the product in double, one rounding on store (and the double's own, inside gam(1) - u): gam(1) |x| f
  admm_pre      b + rho z - rho u with a real rho: two products (once), two additions; the same real operation on both parts of a
                complex element, so the modulus obeys the same k without a sqrt 2:                   gam(3) (|b| + |rho| (|z| + |u|))
  admm_post u   (u + x) - z: two roundings:                                                                  gam(2) (|u| + |x| + |z|)
Sums.  blas1, admm_post and stats accumulate in double.  Any order of summation of n terms in double is within
dsum(dt, n) = c (terms + 4) 2^-53 of sum |term| (gamma() of tests/test_gpu_f64_plan_products.py: complex data doubles the terms and
c = sqrt 2), and the bound is taken against the sum of moduli, never against the result.  Stored as a float: + u |want|.
  nrm2          the square root halves the relative error of the sum; not halved here, which covers its own rounding:
                                                                                                       (dsum + u (1 + dsum)) sqrt(s2)
  asum          real: |x| is exact.  complex: hypotf, 2 u each, as terms of a sum of moduli:           (dsum + u) s1 (+ gam(2) s1)
  dotc          dsum sxy + u |dot|, sxy = sum |x||y|
  stats         min, max, max |x| exact (real parts are converted, not rounded; the complex extremum is planted with modulus
                40 = |24 + 32i|, whose squares add up exactly, so that every hypotf that takes the root of that sum returns 40);
                the two sums are doubles: dsum(n) sum |re|, dsum(n) sum re^2
  admm_post     each norm is the root of a double sum of squares of Float32 numbers that carry r = 0 or 1 roundings (x - xold,
                z - zold, x - z, u_new - u are rounded differences; x, z, u_new are data) -- 2 r u on the sum, r u on the root --
                then one Float32 rounding:  (gam(r + 1) + dsum) want, `want` formed from the u_new that came back (a gated output
                itself).  out[0] adds three such floats: + 2 u out[0].  The maximum of two floats rounds nothing.
L21.  One thread sums a group of m elements serially in Float32: m terms of one (real: a a) or two (complex: fmaf(re, re, im im))
roundings and m - 1 additions, (m + 2) u on the squared norm at the most, half of it plus the root's rounding on g:
e_g = gam((m + 2) / 2 + 1).  q = (g - lambda) / g = 1 - lambda / g moves by (lambda / g) e_g / (1 - e_g) with g, and the subtraction,
the quotient and the product with x add three roundings of |q|:  |x| dq, dq = (lambda / g) e_g / (1 - e_g) + gam(3) |q|.  Where
q < -dq the factor is max(q, 0) = 0 on the device too and the bound is 0: exact zeros.  The bound is absolute, so it also holds for
groups near g = lambda, where q itself is ill-conditioned; the planted groups keep a margin of a factor L21_MARGIN = 2 from it
(g = lambda / 2 and g >= 2 lambda) so that what is asserted about them (zeros, a known factor) does not hang on rounding.
  norm_l21      lambda sum g over slen groups in double, stored as a float:    (e_g + dsum(slen) + u) lambda sum g
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rls_oracle as O  # noqa: E402
from test_gpu_f64_plan_products import gamma as dsum, is_cplx, vector  # noqa: E402

U = 2.0 ** -24
EPS32 = 2.0 ** -23
SQRT2 = math.sqrt(2.0)
HI = {np.dtype(np.float32): np.float64, np.dtype(np.complex64): np.complex128}
DT = [np.float32, np.complex64]
DT_IDS = ["float32", "complex64"]

GRID_CAP = 2048 * 256              # 256-thread grid-stride kernels: at most 2048 workgroups; element GRID_CAP opens the second pass
EW_N = [1, 255, 256, 257, GRID_CAP + 1]
RED_PER_WG = 8192                  # reduce_launch: ceil(n / 8192) workgroups of 1024 threads ...
RED_CAP = 4096 // 2                # ... at most RLS_RED_SLOTS / 2 = 2048: the partials then fill the whole scratch block
RED_N = [1, RED_PER_WG - 1, RED_PER_WG, RED_PER_WG + 1, RED_CAP * RED_PER_WG - 1, RED_CAP * RED_PER_WG, RED_CAP * RED_PER_WG + 1]
STAT_CAP = 4096 // 5 - 1           # rls_stats: at most 818 partial records, the result in the last record
STAT_N = [1, RED_PER_WG, RED_PER_WG + 1, STAT_CAP * RED_PER_WG, STAT_CAP * RED_PER_WG + 1]
POST_N = [1, 63, 64, 1023, 1024, 1025, 5000]
L21_MARGIN = 2.0
# (name, n, slices): slen = n // slices groups, one thread each, 256 threads a workgroup, at most 2048 workgroups
L21_CASES = [("one-group-of-everything", 4096, 4096), ("groups-of-one-n257", 257, 1), ("groups-of-one-second-pass", GRID_CAP + 1, 1),
             ("ragged-n1000-slices7", 1000, 7), ("ragged-tail-reaches-3-of-255-groups", 1023, 4), ("slen255", 1020, 4),
             ("slen256", 1024, 4), ("slen257", 1028, 4), ("slen-second-pass-2048-partials", 2 * (GRID_CAP + 1), 2)]
LONG_GROUP = 65536                 # the one long group of the issue's finding: slices = n = 65536


def gam(k):
    return k * U / (1.0 - k * U)


def cast(v, prec):
    v = np.asarray(v)
    return v.astype(HI[v.dtype]) if prec == 64 else v.copy()


def _T(v):
    return v.real.dtype.type


def _rscale(s, v):
    """real scalar times vector: one rounding per part"""
    T = _T(v)
    return (T(s) * v.view(T)).view(v.dtype)


def scalar(a, v):
    """the coefficient a (a complex number whose parts are Float32 values) as an element of v's type"""
    return v.dtype.type(a) if np.iscomplexobj(v) else v.dtype.type(complex(a).real)


def mag(v):
    return np.abs(np.asarray(v).astype(np.complex128))


def err(got, want):
    return np.abs(np.asarray(got).astype(np.complex128) - np.asarray(want).astype(np.complex128))


def ratio(e, bound):
    """(largest error / bound, all inside); 0 / 0 counts as inside"""
    e, bound = np.atleast_1d(np.asarray(e, dtype=np.float64)), np.atleast_1d(np.asarray(bound, dtype=np.float64))
    ok = bool(np.all(e <= bound))
    return (float(np.max(e / np.maximum(bound, 1e-300))) if e.size else 0.0), ok


# ---- blas1.hip: elementwise ---------------------------------------------------------------------------------------------------------
def coefs(dt):
    """(a, b): Float32 parts, mixed signs"""
    f = np.float32
    return (complex(f(0.7), f(-0.2)), complex(f(-0.3), f(0.5))) if is_cplx(dt) else (complex(f(0.7)), complex(f(-0.3)))


def fill(n, dt, a):
    return np.full(n, scalar(a, np.zeros(1, dt)), dtype=dt)


def scal(a, x, prec):
    x = cast(x, prec)
    return scalar(a, x) * x


def axpy(a, x, y, prec):
    x, y = cast(x, prec), cast(y, prec)
    return scalar(a, x) * x + y


def lincomb(a, x, b, y, prec):
    """z = a x + b y; b = 0: y is not read"""
    x = cast(x, prec)
    if b == 0:
        return scalar(a, x) * x
    return scalar(a, x) * x + scalar(b, x) * cast(y, prec)


def gate_scal(a, x):
    return SQRT2 * gam(2) * abs(a) * mag(x) if is_cplx(x.dtype) else np.zeros(x.size)


def gate_axpy(a, x, y):
    return gam(3) * (SQRT2 * abs(a) * mag(x) + mag(y)) if is_cplx(x.dtype) else gam(2) * (abs(a) * mag(x) + mag(y))


def gate_lincomb(a, x, b, y):
    if b == 0:
        return gate_scal(a, x)
    S = abs(a) * mag(x) + abs(b) * mag(y)
    return gam(4) * SQRT2 * S if is_cplx(x.dtype) else gam(2) * S


# ---- prox.hip: elementwise ----------------------------------------------------------------------------------------------------------
L1_LAM = np.float32(0.625)         # = |0.375 + 0.5i|: a complex entry of modulus lambda exactly


def l1_input(dt, n):
    """planted in front (and the last element, n > 1): |x| = lambda exactly, a negative real of that modulus, an exact zero, |x| <
    lambda, a negative real above the threshold; complex: a modulus of exactly lambda off the axes, purely imaginary values above and
    below the threshold"""
    x = vector(dt, n, 53)
    edge = ([2.0j] if is_cplx(dt) else []) + [L1_LAM, -L1_LAM, 0.0, 0.25, -1.75] + ([0.375 + 0.5j, -0.25j] if is_cplx(dt) else [])
    k = min(len(edge), n)
    x[:k] = np.array(edge[:k], dtype=dt)
    if n > 1:
        x[n - 1] = -L1_LAM
    return x


def _pow2(v, s):
    return _rscale(s, v)


def modulus32(v):
    """|v| of Float32 / ComplexF32 data rounded once to Float32 (NumPy's own complex64 modulus is up to 1.9 ulp off)"""
    w = np.asarray(v)
    return np.sqrt(w.real.astype(np.float64) ** 2 + w.imag.astype(np.float64) ** 2).astype(np.float32)


def prox_l1(x, lam, prec, eps_imag=False):
    """prec = 64: O.prox_l1 under the exact scaling of the module docstring.  prec = 32: real data O.prox_l1 itself; complex data
    the same map written out (ProxL1.jl:18-22) on modulus32, one rounding per operation.  `eps_imag`: the mistake of adding eps to
    the imaginary part too (prec = 32, complex)"""
    v = cast(x, prec)
    T = _T(v)
    if prec == 64 or not np.iscomplexobj(v):
        s = T(np.finfo(T).eps / EPS32)
        return _pow2(O.prox_l1(_pow2(v, s), T(lam) * s), T(1) / s)
    a, eps = modulus32(v), T(EPS32)
    sh, den = np.maximum(a - T(lam), T(0)), a + eps
    out = np.empty_like(v)
    out.real = (sh * (v.real + eps)) / den
    out.imag = (sh * (v.imag + eps if eps_imag else v.imag)) / den
    return out


def gate_l1(x, lam):
    a = mag(x)
    sh = np.maximum(a - float(lam), 0.0)
    return gam(2) * a + gam(7) * sh if is_cplx(x.dtype) else gam(5) * sh


def prox_l2(x, lam, prec):
    return O.prox_l2(cast(x, prec), np.float32(lam))


def gate_l2(x, lam):
    return gam(1) * mag(x) / (1.0 + 2.0 * float(np.float32(lam)))


def prox_positive(x):
    return O.prox_positive(np.asarray(x).copy())


def prox_real(x):
    return O.prox_real(np.asarray(x).copy())


# ---- prox.hip: L21 ------------------------------------------------------------------------------------------------------------------
def l21_group_sums(x, slen, ragged=True):
    """sum of |x_k|^2 over k = i, i + slen, ... < n for every group i, accumulated serially in x's own precision (l21_kernel's loop).
    `ragged` False: the mistake of stopping at slices * slen"""
    T, n = _T(x), x.size
    s2 = np.zeros(slen, dtype=T)
    end = n if ragged else (n // slen) * slen
    for lo in range(0, end, slen):
        blk = x[lo: min(lo + slen, end)]
        a2 = (blk.real * blk.real + blk.imag * blk.imag) if np.iscomplexobj(x) else blk * blk
        s2[: blk.size] += a2
    return s2


def l21_lines(x, lam, slices, prec, ragged=True):
    """(prox, norm) of ProxL21.jl:30-46 line by line as l21_kernel does them"""
    v = cast(x, prec)
    T, n = _T(v), v.size
    slen = n // slices
    g = np.sqrt(l21_group_sums(v, slen, ragged))
    with np.errstate(divide="ignore", invalid="ignore"):
        fac = np.maximum((g - T(lam)) / g, T(0))     # (NaN propagates, as fmaxf does not: the kernel tests q != q)
    out = v.copy()
    w = out.view(T).reshape(n, -1)
    w *= fac[np.arange(n) % slen][:, None]
    return out, T(np.float64(np.float32(lam)) * np.sum(g.astype(np.float64)))


def l21_ref(x, lam, slices):
    """the float64 oracle on the float64 data: (prox, norm, group norms)"""
    v = cast(x, 64)
    slen = v.size // slices
    g = O._l21_group_norms(v, slen, np.arange(v.size) % slen)
    return O.prox_l21(v.copy(), np.float32(lam), slices), float(O.norm_l21(v, np.float32(lam), slices)), g


def gate_l21(x, lam, slices, g):
    """(per-element bound, bound of the norm); g: the float64 group norms"""
    n, lam = x.size, float(np.float32(lam))
    slen = n // slices
    m = -(-n // slen)                                # the longest group
    e_g = gam((m + 2) / 2.0 + 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = (g - lam) / g
        dq = (lam / g) * e_g / (1.0 - e_g) + gam(3) * np.abs(q)
    dq = np.where(q < -dq, 0.0, dq)
    dq = np.where(np.isfinite(dq), dq, 0.0)          # all-zero groups: exact zeros (lambda > 0) or NaN (lambda = 0: compared as NaN)
    return mag(x) * dq[np.arange(n) % slen], (e_g + dsum(np.float32, slen) + U) * lam * float(np.sum(g))


def l21_input(dt, n, slices, lam, zero_group=True):
    """Gaussian, scaled so that a typical group norm is 3 lambda; planted (where there are at least 4 groups): group 1 all zero,
    group 2 at g = lambda / L21_MARGIN, group 3 at g = L21_MARGIN lambda"""
    slen = n // slices
    m = -(-n // slen)
    x = (vector(dt, n, 61 + n + slices) * np.float32(3.0 * lam / math.sqrt(m) if lam > 0 else 1.0 / math.sqrt(m))).astype(dt)
    if slen >= 4:
        if zero_group:
            x[1::slen] = 0
        ref = max(float(lam), 0.5)
        for grp, target in ((2, ref / L21_MARGIN), (3, ref * L21_MARGIN)):
            gn = math.sqrt(float(np.sum(mag(x[grp::slen]) ** 2)))
            x[grp::slen] = (x[grp::slen] * np.float32(target / gn)).astype(dt)
    return x


# ---- nested.hip ---------------------------------------------------------------------------------------------------------------------
def _ztransform(shift, scale, T):
    t = O.ZTransform.__new__(O.ZTransform)           # (x - mean) / std and x std + mean with given numbers
    t.mean, t.std = T(shift), T(scale)
    return t


def shift_scale(x, shift, scale, inverse, prec):
    """mode 0: (x - shift) / scale, mode 1: x scale + shift (Transforms.jl:11,15,41,45), through the oracle's ZTransform"""
    v = cast(x, prec)
    t = _ztransform(shift, scale, _T(v))
    return t.inverse_transform(v) if inverse else t.transform(v)


def clamp(x, lo, hi):
    return np.clip(x, np.float32(lo), np.float32(hi))


def restore_outside(out, orig, lo, hi, strict_upper=False):
    """out[mask] = orig[mask], mask = (orig < lo) | (orig >= hi), the oracle's (Transforms.jl:62-66).  `strict_upper`: the mistake
    of `>` for the upper limit"""
    out = np.asarray(out).copy()
    mask = ((orig < lo) | (orig > hi)) if strict_upper else O.ClampedScalingTransform(orig, np.float32(lo), np.float32(hi)).mask
    out[mask] = orig[mask]
    return out


CLAMP_LO, CLAMP_HI = np.float32(-0.5), np.float32(0.75)


def clamp_input(n):
    """Float32 Gaussian with values exactly at lo and at hi, just inside and just outside, in front (and hi in the last element)"""
    x = vector(np.float32, n, 71)
    f = np.float32
    edge = [CLAMP_LO, CLAMP_HI, np.nextafter(CLAMP_LO, f(-9)), np.nextafter(CLAMP_LO, f(9)), np.nextafter(CLAMP_HI, f(-9)),
            np.nextafter(CLAMP_HI, f(9)), f(-3), f(3)]
    k = min(len(edge), n)
    x[:k] = edge[:k]
    if n > 1:
        x[n - 1] = CLAMP_HI
    return x


def stats(x, prec):
    """(min re, max re, sum re, sum re^2, max |x|) as rls_stats forms them: the modulus in x's precision, the rest in double"""
    v = cast(x, prec)
    re = v.real.astype(np.float64)
    s = ss = 0.0
    for i in range(0, re.size, 1 << 20):
        c = re[i: i + (1 << 20)]
        s, ss = s + float(np.sum(c)), ss + float(np.sum(c * c))
    return np.array([re.min(), re.max(), s, ss, float((modulus32(v) if prec == 32 else np.abs(v)).max())])


def gate_stats(x):
    re = np.asarray(x).real.astype(np.float64)
    d = dsum(np.float32, x.size)
    return np.array([0.0, 0.0, d * float(np.sum(np.abs(re))), d * float(np.sum(re * re)), 0.0])


def stats_input(dt, n, where):
    """Gaussian; the maximum of the real parts and of the moduli (40, complex: 24 + 32i) at `where` ("first", "last", "cap": element
    STAT_CAP * 8192), the minimum (-33) at the mirrored position"""
    x = vector(dt, n, 81)
    pos = {"first": 0, "last": n - 1, "cap": min(n - 1, STAT_CAP * RED_PER_WG)}[where]
    if n - 1 - pos != pos:
        x[n - 1 - pos] = -33
    x[pos] = (24 + 32j) if is_cplx(dt) else 40
    return x, pos


# ---- solvers.hip: ADMM bookkeeping --------------------------------------------------------------------------------------------------
def admm_pre(beta, beta_y, z, u, rho, accumulate, prec):
    """beta = (accumulate ? beta : beta_y) + rho z - rho u   (src/ADMM.jl:236-243, identity regTrafo)"""
    b = cast(beta if accumulate else beta_y, prec)
    b = b + _rscale(np.float32(rho), cast(z, prec))
    return b + _rscale(-np.float32(rho), cast(u, prec))


def gate_admm_pre(beta, beta_y, z, u, rho, accumulate):
    return gam(3) * (mag(beta if accumulate else beta_y) + abs(float(np.float32(rho))) * (mag(z) + mag(u)))


def _ssq(v):
    w = np.asarray(v)
    return float(np.sum(w.real.astype(np.float64) ** 2) + (np.sum(w.imag.astype(np.float64) ** 2) if np.iscomplexobj(w) else 0.0))


def admm_post_u(x, z, u, prec):
    """u += x ; u -= z   (src/ADMM.jl:266-267)"""
    return (cast(u, prec) + cast(x, prec)) - cast(z, prec)


def gate_admm_post_u(x, z, u):
    return gam(2) * (mag(u) + mag(x) + mag(z))


def admm_post_out(x, xold, z, zold, u, u_new, prec, late_du=False):
    """the six outputs of admm_post_kernel (src/ADMM.jl:265-299 with Phi = I) from the data and the u_new that was stored: differences
    in the element precision, sums of squares in double, roots and out[0]'s two additions in the real precision.  `late_du`: the
    mistake of forming ||u_new - u|| after u has been overwritten"""
    x, xold, z, zold, u, un = (cast(v, prec) for v in (x, xold, z, zold, u, u_new))
    T = _T(x)
    rt = lambda v: T(math.sqrt(_ssq(v)))   # noqa: E731
    dx, dz, du = rt(x - xold), rt(z - zold), rt(un - (un if late_du else u))
    return np.array([dx + dz + du, dz, max(rt(x), rt(z)), rt(x - z), rt(un), dx], dtype=T)


def gate_admm_post_out(want, n, dt):
    """bounds of the six outputs from their float64 values `want` (module docstring)"""
    d = dsum(dt, n)
    one, none = gam(2) + d, gam(1) + d                 # a norm of rounded differences, a norm of data
    w = np.abs(np.asarray(want, dtype=np.float64))
    return np.array([one * w[0] + 2.0 * U * w[0] * (1.0 + one), one * w[1], none * w[2], one * w[3], none * w[4], one * w[5]])


def admm_input(dt, n, kind="generic"):
    """(x, xold, z, zold, u, beta, beta_y); kind "x=z": r = 0 exactly, "xold=x": ||x - xold|| = 0"""
    v = [vector(dt, n, 90 + i + 7 * n) for i in range(7)]
    if kind == "x=z":
        v[2] = v[0].copy()
    if kind == "xold=x":
        v[1] = v[0].copy()
    return v


# ---- blas1.hip: reductions ----------------------------------------------------------------------------------------------------------
def sums(x, y, prec, lo=0, hi=None):
    """(sum |x|^2, sum |x|, conj(x) . y, sum |x||y|) over [lo, hi) as doubles, a million elements at a time; the moduli of asum in
    x's precision at prec = 32 (the kernel's hypotf), the products and every sum in double at either precision"""
    hi = x.size if hi is None else hi
    s2 = s1 = sxy = 0.0
    dot = 0j
    for i in range(lo, hi, 1 << 20):
        xs, ys = x[i: min(i + (1 << 20), hi)], y[i: min(i + (1 << 20), hi)]
        xl, yl = xs.astype(np.complex128), ys.astype(np.complex128)
        ax = np.abs(xl)
        a1 = modulus32(xs).astype(np.float64) if prec == 32 else ax
        s2 += float(np.sum(xl.real * xl.real + xl.imag * xl.imag))
        s1 += float(np.sum(a1))
        dot += complex(np.sum(xl.real * yl.real + xl.imag * yl.imag), np.sum(xl.real * yl.imag - xl.imag * yl.real))
        sxy += float(np.sum(ax * np.abs(yl)))
    return s2, s1, dot, sxy


def add_sums(a, b):
    return tuple(p + q for p, q in zip(a, b))


def results32(s):
    """what the entry points store from the double sums: nrm2, asum, (dot re, dot im) as floats"""
    f = np.float32
    return f(math.sqrt(s[0])), f(s[1]), complex(f(s[2].real), f(s[2].imag))


def gates_red(dt, n, s):
    """bounds of nrm2, asum, dotc from the float64 sums s (module docstring)"""
    d = dsum(dt, n)
    nrm = math.sqrt(s[0])
    return ((d + U * (1.0 + d)) * nrm, (d + U + (gam(2) if is_cplx(dt) else 0.0)) * s[1], d * s[3] + U * (abs(s[2]) + d * s[3]))


def cancelling(x, y0, target=1e-6):
    """y = y0 - c x, formed in float64 and rounded to x's type, with conj(x) . y about `target` of sum |x||y|"""
    xl, yl = x.astype(HI[x.dtype]), y0.astype(HI[x.dtype])
    t = target * float(np.abs(xl) @ np.abs(yl))
    return (yl - ((np.vdot(xl, yl) - t) / np.vdot(xl, xl)) * xl).astype(x.dtype)


def _four(dt, k):
    """modulus 4 (complex: off both axes)"""
    return np.dtype(dt).type(4 * np.exp(1j * (0.7 + k))) if is_cplx(dt) else np.dtype(dt).type(4 if k % 2 else -4)


def plant_fours(x, idx):
    for k, i in enumerate(idx):
        if 0 <= i < x.size:
            x[i] = _four(x.dtype, k)


def red_small(dt, n):
    """(x, y) of one of the four small sizes: modulus 4 in the last element (n > 1), y cancelling"""
    x, y = vector(dt, n, 43), vector(dt, n, 44)
    if n > 1:
        plant_fours(x, [n - 1])
        plant_fours(y, [n - 1])
        y = cancelling(x, y)
    return x, y


_big = {}


def red_big(dt):
    """ONE pair for the three sizes around the cap (a view of it each): modulus 4 at cap 8192 - 2, cap 8192 - 1 and cap 8192 -- the
    last element of each of the three sizes, and the first one past the cap -- and y cancelling over the first cap 8192 elements.
    Read-only, with the float64 sums of the first cap 8192 - 1 elements computed once."""
    key = np.dtype(dt)
    if key not in _big:
        n = RED_CAP * RED_PER_WG + 1
        x, y = vector(dt, n, 41), vector(dt, n, 42)
        for v in (x, y):
            plant_fours(v, [n - 3, n - 2, n - 1])
        y[: n - 1] = cancelling(x[: n - 1], y[: n - 1])
        x.setflags(write=False)
        y.setflags(write=False)
        _big[key] = (x, y, sums(x, y, 64, 0, n - 2), sums(x, y, 32, 0, n - 2))
    return _big[key]


def red_case(dt, n):
    """(x, y, float64 sums, the sums as the kernel's arithmetic forms them) of a reduction size"""
    if n > 4 * RED_PER_WG:
        x, y, base64, base32 = red_big(dt)
        m = RED_CAP * RED_PER_WG - 1
        return x[:n], y[:n], add_sums(base64, sums(x, y, 64, m, n)), add_sums(base32, sums(x, y, 32, m, n))
    x, y = red_small(dt, n)
    return x, y, sums(x, y, 64), sums(x, y, 32)


# ---- the elementwise cases, shared by both tiers --------------------------------------------------------------------------------------
def watch(n):
    """asserted one by one on top of the whole-array check: the last element, the two sides of the second grid pass"""
    return sorted({n - 1, min(n - 1, GRID_CAP - 1), min(n - 1, GRID_CAP)})


def _visible(x):
    """negative real parts (and non-zero imaginary ones) at the watched elements: a projection that skips one shows"""
    x = x.copy()
    for i in watch(x.size):
        x[i] = (-1.5 + 0.5j) if np.iscomplexobj(x) else -1.5
    return x


def restore_input(n):
    """orig with hi, lo and their four neighbours in front, and hi again at the watched elements (restored by `>=`, not by `>`)"""
    x = clamp_input(n)
    if n > 1:
        x[0], x[1] = x[1], x[0]
    for i in watch(n):
        x[i] = CLAMP_HI
    return x


def _out(name, out0, want64, got32, gate, watched=None):
    """one output vector: its content before the launch (None: fresh), its float64 value, its float32 evaluation, its gate (None:
    the bytes of the float32 evaluation), and the elements that the threads of watch(n) write"""
    return {"name": name, "out0": out0, "want": want64, "got32": got32, "gate": gate,
            "watch": watch(len(got32)) if watched is None else [int(i) for i in watched]}


def _both(f):
    return f(64), f(32)


L2_LAM = np.float32(0.37)
SHIFT, SCALE = np.float32(0.3125), np.float32(1.7)
RHO = np.float32(0.83)


def ew_cases(dt, n):
    """{case name: (arguments for the launch, [outputs])} of every elementwise entry point at length n.  Inputs that the kernel only
    reads are among the arguments; they must come back bit-identical."""
    dt = np.dtype(dt)
    cplx = is_cplx(dt)
    a, b = coefs(dt)
    x, y, z0 = vector(dt, n, 51), vector(dt, n, 52), vector(dt, n, 53)
    nan = np.full(n, np.nan, dtype=dt)
    c = {}
    c["fill"] = ({"a": a}, [_out("x", x, fill(n, dt, a), fill(n, dt, a), None)])
    c["scal"] = ({"a": a}, [_out("x", x, *_both(lambda p: scal(a, x, p)), gate_scal(a, x) if cplx else None)])
    c["axpy"] = ({"a": a, "x": x}, [_out("y", y, *_both(lambda p: axpy(a, x, y, p)), gate_axpy(a, x, y))])
    c["lincomb"] = ({"a": a, "b": b, "x": x, "y": y}, [_out("z", z0, *_both(lambda p: lincomb(a, x, b, y, p)), gate_lincomb(a, x, b, y))])
    for name, yy in (("lincomb-b0-null-y", None), ("lincomb-b0-nan-y", nan)):
        c[name] = ({"a": a, "b": 0j, "x": x, "y": yy}, [_out("z", z0, *_both(lambda p: lincomb(a, x, 0, None, p)), gate_scal(a, x) if cplx else None)])
    c["axpby"] = ({"a": a, "b": b, "x": x}, [_out("y", y, *_both(lambda p: lincomb(a, x, b, y, p)), gate_lincomb(a, x, b, y))])
    xl = l1_input(dt, n)
    c["prox_l1"] = ({"lam": L1_LAM}, [_out("x", xl, *_both(lambda p: prox_l1(xl, L1_LAM, p)), gate_l1(xl, L1_LAM))])
    xs, lam_s = _pow2(xl, 2.0 ** -10), np.float32(L1_LAM * 2.0 ** -10)   # the same entries at 1e-3: eps(Float32) is no longer small beside them
    c["prox_l1-small"] = ({"lam": lam_s}, [_out("x", xs, *_both(lambda p: prox_l1(xs, lam_s, p)), gate_l1(xs, lam_s))])
    xp = _visible(x)
    c["prox_l2"] = ({"lam": L2_LAM}, [_out("x", xp, *_both(lambda p: prox_l2(xp, L2_LAM, p)), gate_l2(xp, L2_LAM))])
    c["prox_positive"] = ({}, [_out("x", xp, prox_positive(xp), prox_positive(xp), None)])
    c["prox_real"] = ({}, [_out("x", xp, prox_real(xp), prox_real(xp), None)])
    rng = np.random.default_rng(n)
    for kind, N, idx in (("perm", n, rng.permutation(n)), ("sparse", 3 * n, np.arange(n) * 3 + (np.arange(n) % 3 == 1))):
        idx = idx.astype(np.int32)
        src, vals = vector(dt, N, 54), vector(dt, n, 55)
        c[f"gather-{kind}"] = ({"idx": idx, "x": src}, [_out("out", None, src[idx], src[idx], None)])
        sc = src.copy()
        sc[idx] = vals
        c[f"scatter-{kind}"] = ({"idx": idx, "in": vals}, [_out("x", src, sc, sc, None, idx[watch(n)])])
    xo, bt, by, z, u = (vector(dt, n, 56 + i) for i in range(5))
    for acc in (0, 1):
        outs = [_out("beta", bt, *_both(lambda p: admm_pre(bt, by, z, u, RHO, acc, p)), gate_admm_pre(bt, by, z, u, RHO, acc)),
                _out("xold", xo, xo if acc else x, xo if acc else x, None)]
        c[f"admm_pre-accumulate{acc}"] = ({"beta_y": by, "z": z, "u": u, "x": x, "rho": RHO, "accumulate": acc}, outs)
    if not cplx:
        for inv in (0, 1):
            c[f"shift_scale-mode{inv}"] = ({"shift": SHIFT, "scale": SCALE, "inverse": inv},
                                           [_out("x", x, *_both(lambda p: shift_scale(x, SHIFT, SCALE, inv, p)), None)])
        xc = _visible(clamp_input(n)) if n > 8 else np.array([3.0], np.float32)[:n]
        c["clamp"] = ({"lo": CLAMP_LO, "hi": CLAMP_HI}, [_out("x", xc, clamp(xc, CLAMP_LO, CLAMP_HI), clamp(xc, CLAMP_LO, CLAMP_HI), None)])
        orig = restore_input(n)
        r = restore_outside(y, orig, CLAMP_LO, CLAMP_HI)
        c["restore_outside"] = ({"orig": orig, "lo": CLAMP_LO, "hi": CLAMP_HI}, [_out("out", y, r, r, None)])
    else:
        re, im = np.ascontiguousarray(x.real), np.ascontiguousarray(x.imag)
        c["complex_split"] = ({"z": x}, [_out("re", None, re, re, None), _out("im", None, im, im, None)])
        c["complex_merge"] = ({"re": re, "im": im}, [_out("z", None, x, x, None)])
    return c
