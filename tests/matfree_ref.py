"""A numpy restatement, in float64 / complex128, of the matrix-free operators (csrc/fft.hip): SamplingOp, FFTOp and their product,
as functions (numpy.fft and fancy indexing) and, for small shapes, as dense matrices built column by column from those functions.
Vectors are column-major images, like every vector of the project.  tests/test_matfree_abi.py checks this file on the CPU."""
import numpy as np


def _n(shape):
    return int(np.prod(np.atleast_1d(shape)))


def _img(x, shape):
    return np.asarray(x, np.complex128).reshape(tuple(np.atleast_1d(shape)), order="F")


def sampling(x, pattern):
    """y = x[pattern]"""
    return np.asarray(x)[np.asarray(pattern)]


def sampling_adj(y, pattern, n):
    """x = 0; x[pattern] = y"""
    y = np.asarray(y)
    x = np.zeros(n, y.dtype)
    x[np.asarray(pattern)] = y
    return x


def sampling_mask(pattern, n):
    m = np.zeros(n)
    m[np.asarray(pattern)] = 1.0
    return m


def fft(x, shape, shift=True, unitary=True):
    """F x = fftshift(fftn(ifftshift(x))) / sqrt(n); shift=False: no shifts, unitary=False: no scale"""
    X = _img(x, shape)
    if shift:
        X = np.fft.ifftshift(X)
    X = np.fft.fftn(X)
    if shift:
        X = np.fft.fftshift(X)
    if unitary:
        X = X / np.sqrt(_n(shape))
    return X.ravel(order="F")


def fft_adj(y, shape, shift=True, unitary=True):
    """F^H y, the conjugate transpose: fftshift(ifftn(ifftshift(y))) sqrt(n) when unitary, n ifftn (unscaled) otherwise"""
    Y = _img(y, shape)
    if shift:
        Y = np.fft.ifftshift(Y)
    Y = np.fft.ifftn(Y) * _n(shape)
    if shift:
        Y = np.fft.fftshift(Y)
    if unitary:
        Y = Y / np.sqrt(_n(shape))
    return Y.ravel(order="F")


def sampled_fft(x, pattern, shape, shift=True, unitary=True):
    return sampling(fft(x, shape, shift, unitary), pattern)


def sampled_fft_adj(y, pattern, shape, shift=True, unitary=True):
    return fft_adj(sampling_adj(np.asarray(y, np.complex128), pattern, _n(shape)), shape, shift, unitary)


def dense(fun, n_in, dtype=np.complex128):
    """the matrix of a linear function, column by column from the unit vectors"""
    cols = []
    for j in range(n_in):
        e = np.zeros(n_in, dtype)
        e[j] = 1
        cols.append(np.asarray(fun(e), dtype))
    return np.stack(cols, axis=1)


def sampling_dense(pattern, n, dtype=np.float64):
    return dense(lambda e: sampling(e, pattern), n, dtype)


def fft_dense(shape, shift=True, unitary=True):
    return dense(lambda e: fft(e, shape, shift, unitary), _n(shape))


def sampled_fft_dense(pattern, shape, shift=True, unitary=True):
    return dense(lambda e: sampled_fft(e, pattern, shape, shift, unitary), _n(shape))


def pattern(n, m, seed, ends=True):
    """m distinct sorted indices of [0, n); with `ends`, 0 and n - 1 among them (m >= 2)"""
    rng = np.random.default_rng(seed)
    if ends and m >= 2 and n >= 2:
        inner = rng.choice(np.arange(1, n - 1), size=m - 2, replace=False) if m > 2 else np.zeros(0, np.int64)
        idx = np.concatenate([[0, n - 1], inner])
    else:
        idx = rng.choice(n, size=m, replace=False)
    return np.sort(idx).astype(np.int32)
