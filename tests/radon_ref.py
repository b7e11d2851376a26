"""NumPy restatement of RadonOp, written from the operator's definition, not from the kernels.

The exact parallel-beam line integral of a piecewise-constant image:
  image n1 x n2, column-major: pixel (i, j) is element i + n1 j, its centre at xr = i - (n1 - 1) / 2, yr = j - (n2 - 1) / 2;
  D detector bins per angle, centred at t_k = k - (D - 1) / 2, unit spacing; the sinogram is D x nA, detector fastest: row k + D q;
  per angle (Float64): c = cos, s = sin; min(|c|, |s|) <= 2^-40 snaps the angle onto the axis (the small one 0, the large one +-1);
  mx = max(|c|, |s|), mn = min(|c|, |s|), hi = (|c| + |s|) / 2;
  A[k + D q, i + n1 j] = w(|t_k - (xr c + yr s)|),  w(d) = clamp((hi - d) / mn, 0, 1) / mx for mn > 0,
                                                   w(d) = 1 / mx (d < hi), 0.5 / mx (d == hi), 0 otherwise for mn = 0.
`dtype` is the precision everything behind the Float64 table is evaluated in: float64 is the reference, float32 the yardstick for a
Float32 result's own rounding."""
import numpy as np


def default_detectors(shape) -> int:
    return 2 * int(np.ceil(np.hypot(shape[0], shape[1]) / 2)) + 1


def table(angles):
    """(c, s, mx, mn, hi) per angle, Float64"""
    th = np.atleast_1d(np.asarray(angles, np.float64))
    c, s = np.cos(th), np.sin(th)
    snap = np.minimum(np.abs(c), np.abs(s)) <= 2.0 ** -40
    cx = np.abs(c) > np.abs(s)
    c = np.where(snap, np.where(cx, np.sign(c), 0.0), c)
    s = np.where(snap, np.where(cx, 0.0, np.sign(s)), s)
    a, b = np.abs(c), np.abs(s)
    return c, s, np.maximum(a, b), np.minimum(a, b), (a + b) / 2


def weight(d, mx, mn, hi, dtype=np.float64):
    dt = np.dtype(dtype).type
    d, mx, mn, hi = np.abs(d).astype(dt), dt(mx), dt(mn), dt(hi)
    if mn == 0:
        return np.where(d < hi, dt(1), np.where(d == hi, dt(0.5), dt(0))) / mx
    return np.clip((hi - d) / mn, dt(0), dt(1)) / mx


def dense(shape, angles, D=None, dtype=np.float64):
    """the M x N matrix, M = D len(angles), N = n1 n2"""
    dt = np.dtype(dtype).type
    n1, n2 = shape
    D = default_detectors(shape) if D is None else int(D)
    c, s, mx, mn, hi = table(angles)
    xr = np.arange(n1).astype(dt) - dt((n1 - 1) / 2)
    yr = np.arange(n2).astype(dt) - dt((n2 - 1) / 2)
    t = np.arange(D).astype(dt) - dt((D - 1) / 2)
    A = np.zeros((D * c.size, n1 * n2), dt)
    for q in range(c.size):
        p = (xr[:, None] * dt(c[q]) + yr[None, :] * dt(s[q])).astype(dt).ravel(order="F")
        A[q * D:(q + 1) * D] = weight(t[:, None] - p[None, :], mx[q], mn[q], hi[q], dt)
    return A


def forward(x, shape, angles, D=None, dtype=np.float64):
    """the sinogram A x (length D len(angles)); a complex x keeps its kind in the matching precision"""
    A = dense(shape, angles, D, dtype)
    x = np.asarray(x)
    return A @ x.astype(np.result_type(A.dtype, np.complex64 if x.dtype.kind == "c" else A.dtype))


def adjoint(y, shape, angles, D=None, dtype=np.float64):
    """the back-projection A^T y (length n1 n2); the weights are real, so this is A^H y as well"""
    A = dense(shape, angles, D, dtype)
    y = np.asarray(y)
    return A.T @ y.astype(np.result_type(A.dtype, np.complex64 if y.dtype.kind == "c" else A.dtype))
