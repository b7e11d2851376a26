"""Float64 reference of WaveletOp, built from the definition AS MATRICES (not by looping the algorithm):

    h: "haar" [1, 1]/sqrt 2, "db2" [1+sqrt 3, 3+sqrt 3, 3-sqrt 3, 1-sqrt 3]/(4 sqrt 2);  g[k] = (-1)^k h[L-1-k]
    one level on a line of even length n, output [a | d]:  a[i] = sum_k h[k] s[(2i+k) mod n],  d[i] = sum_k g[k] s[(2i+k) mod n]

`level_matrix` is that n x n matrix; levels compose as blockdiag(level, I); a column-major image n1 x n2 takes
kron(level(m2), level(m1)) on its leading (m1 x m2) block per level (Mallat form).  `dense` is the whole operator, `apply` the same
operator through kron(B, A) vec(X) = vec(A X B^T) for images whose dense matrix would not fit in memory."""
import functools

import numpy as np


def taps(wt):
    if wt == "haar":
        h = np.array([1.0, 1.0]) / np.sqrt(2.0)
    elif wt == "db2":
        s3 = np.sqrt(3.0)
        h = np.array([1 + s3, 3 + s3, 3 - s3, 1 - s3]) / (4 * np.sqrt(2.0))
    else:
        raise ValueError(wt)
    L = len(h)
    g = np.array([(-1.0) ** k * h[L - 1 - k] for k in range(L)])
    return h, g


@functools.lru_cache(maxsize=None)
def level_matrix(n, wt):
    h, g = taps(wt)
    M = np.zeros((n, n))
    for i in range(n // 2):
        for k in range(len(h)):
            M[i, (2 * i + k) % n] += h[k]          # (+=: for n < L the taps wrap more than once)
            M[n // 2 + i, (2 * i + k) % n] += g[k]
    return M


def extents(shape):
    """the transformed extents: dimensions of extent 1 are dropped"""
    shape = (shape,) if np.isscalar(shape) else tuple(shape)
    return tuple(int(s) for s in shape if s != 1)


def default_levels(shape):
    ext, J = extents(shape), 0
    while ext and all(s % (2 << J) == 0 for s in ext):
        J += 1
    return J


def _levels(shape, levels):
    return default_levels(shape) if levels is None else levels


@functools.lru_cache(maxsize=None)
def dense(shape, wt="db2", levels=None):
    """the N x N float64 matrix of the operator"""
    ext, J = extents(shape), _levels(shape, levels)
    if len(ext) == 0:
        return np.eye(1)
    n1, n2 = (ext + (1,))[:2]
    N = n1 * n2
    W = np.eye(N)
    for j in range(J):
        m1, m2 = n1 >> j, (n2 >> j if n2 > 1 else 1)
        K = level_matrix(m1, wt) if n2 == 1 else np.kron(level_matrix(m2, wt), level_matrix(m1, wt))
        idx = np.array([r + c * n1 for c in range(m2) for r in range(m1)])   # the leading block inside vec(image)
        W[idx, :] = K @ W[idx, :]                                          # blockdiag(level, I) @ W
    W.setflags(write=False)
    return W


def apply(x, shape, wt="db2", levels=None, adjoint=False, native=False):
    """dense(shape, wt, levels) @ x (or its transpose) without forming it: per level A X B^T on the leading block.
    In float64 / complex128 whatever x is; native=True: in the precision of x (the working-precision run of an oracle)."""
    ext, J = extents(shape), _levels(shape, levels)
    x = np.asarray(x)
    work = x.dtype if native else np.dtype(np.complex128 if x.dtype.kind == "c" else np.float64)
    real = np.dtype(np.float32 if work in (np.dtype(np.float32), np.dtype(np.complex64)) else np.float64)
    X = x.astype(work).reshape((ext + (1, 1))[:2], order="F").copy()
    n1, n2 = X.shape
    for j in (range(J - 1, -1, -1) if adjoint else range(J)):
        m1, m2 = n1 >> j, (n2 >> j if n2 > 1 else 1)
        A = level_matrix(m1, wt).astype(real)
        B = (level_matrix(m2, wt) if n2 > 1 else np.eye(1)).astype(real)
        X[:m1, :m2] = (A.T @ X[:m1, :m2] @ B) if adjoint else (A @ X[:m1, :m2] @ B.T)
    return X.reshape(-1, order="F")


class SeparableOp:
    """mul / mul_adj of the operator for the oracle's TransformedRegularization, through `apply`"""

    def __init__(self, shape, wt="db2", levels=None, native=False):
        self.shape, self.wt, self.levels, self.native = shape, wt, levels, native

    def mul(self, x):
        return apply(x, self.shape, self.wt, self.levels, native=self.native)

    def mul_adj(self, z):
        return apply(z, self.shape, self.wt, self.levels, adjoint=True, native=self.native)
