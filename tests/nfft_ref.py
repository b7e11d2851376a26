"""The checker of NFFTOp (csrc/nfft.hip): NumPy only.  tests/test_nfft_ref.py holds it to the dense non-uniform
DFT and to planted mistakes on the CPU, tests/test_gpu_nfft.py holds the device to it.

  exact         the dense matrix E[j, k] = exp(-2 pi i k . nu_j), k_d in {-floor(N_d / 2), ..., ceil(N_d / 2) - 1}, first extent
                fastest, in complex128 (the phase k . nu reduced in double: |k . nu| <= N_1 / 4 + N_2 / 4, error <= 2^-53 of that).
  restated      Plan: the algorithm step by step in any complex type.  Grid n_d = the smallest power of two >= 2 N_d; the window
                phi(t) = sinh(b sqrt(m^2 - t^2)) / (pi sqrt(m^2 - t^2)), b = pi (2 - N_d / n_d), phi(+-m) = b / pi, at the taps
                u0 - m + 1 ... u0 + m, u0 = floor(n nu), periodic in u; the deapodisation 1 / phihat(k),
                phihat(k) = I0(m sqrt(b^2 - (2 pi k / n)^2)); numpy.fft for the grid transform between two shifts.  m^2 - t^2 and
                b^2 - w^2 are formed as (m - t)(m + t) and (b - w)(b + w) and I0 by its power series, as rls_nfft_create forms them:
                no expression a compiler could contract into an fma, so the two tables agree to the last bits of libm's sinh.
                The window and phihat are computed in double and rounded once to the real type of `dtype`.
  the scale     phihat above is the transform of phi in GRID units t.  The Fourier coefficient of the n-periodic window is
                c_k = phihat(k) / n, and the unscaled transform of the grid supplies the n: the factor is 1 / phihat(k) and no 1 / n
                is left over (NFFT3's g^_k = f^_k / (n c_k) is the same statement).  The plant "scale_n" puts one in.

The gates (derived, not measured; u = 2^-24 for ComplexF32, 2^-53 for ComplexF64, v = 2^-53 always).
Tables.  A table entry is a double evaluation rounded once: relative error mu = u + 16 v for ComplexF32 and 16 v for ComplexF64
(nothing is rounded there), 16 v being two implementations of sinh or of the series each within 4 ulp of the truth.
Forward.  g = (x d_1) d_2: d table roundings and d products, ||g^ - g||_2 <= 2 d u ||g||_2.  The transform of 2^t points,
t = lg n_1 + lg n_2, errs by at most fft_ref.gate ||G||_2 in every element (tests/fft_ref.py, Higham Theorem 24.2), and carries the
input's error at most at its 2-norm, so every |G^_q - G_q| <= eG ||G||_2, eG = gate + 2 d u.  A node's value is an fma chain over
T = (2 m)^d products w_1 w_2 G: gamma_T = T u / (1 - T u) from the chain, d mu + (d - 1) u from the weight, so

    |y^_j - y_j|  <=  (gamma_T + d mu + (d - 1) u) sum_T |w| |G|  +  eG ||G||_2 sum_T |w|.

Adjoint.  A grid point sums c_q products (c_q counted by the plan): e_q = (gamma_c + d mu + (d - 1) u) sum |w| |y|.  The transform
has entries of modulus one, so it carries e at most at ||e||_1 into every element, and adds gate ||h||_2 of its own,
||h||_2 = sqrt(n_1 n_2) ||G||_2; the crop is exact and the deapodisation 2 d u relative:

    |x^_k - x_k|  <=  d_k (gate sqrt(n_1 n_2) ||G||_2 + ||e||_1)  +  2 d u |x_k|.

Both are multiplied by SECOND = 1.05 for the second-order terms dropped above.
Truncation.  Potts & Steidl's estimate for the Kaiser-Bessel window at sigma = 2, the worst case of [2, 4), times d:
C(m, sigma) = 4 pi (sqrt(m) + m) (1 - 1 / sigma)^(1/4) exp(-2 pi m sqrt(1 - 1 / sigma)), relative to ||x||_1.  An entry of the
restated matrix is the response to a unit vector, so it is within d C of E's, and the adjoint within d C ||y||_1.
"""
import math

import numpy as np

import fft_ref as FR

C64, C128 = FR.C64, FR.C128
DT, DT_IDS, U = FR.DT, FR.DT_IDS, FR.U
MAX_N = {C64: 4096, C128: 2048}   # n_d = 2 N_d must not exceed the FFT's line limit (fft_ref.MAX_LINE)
M_MAX = 8
SECOND = 1.05
PLANTS = ("taps_off_by_one", "no_wrap", "scale_n", "phihat_swapped", "centre_off_by_one")


def real_of(dtype):
    return np.zeros(1, dtype).real.dtype


def extents(shape):
    """the one or two extents the operator works on: unit extents dropped, (1,) when nothing is left"""
    ext = [int(s) for s in np.atleast_1d(shape) if int(s) != 1]
    if len(np.atleast_1d(shape)) == 0 or len(ext) > 2 or any(s < 1 for s in ext):
        raise ValueError("one or two positive extents")
    return tuple(ext) if ext else (1,)


def grid_extent(N):
    n = 2
    while n < 2 * N:
        n *= 2
    return n


def centred(N):
    return np.arange(N) - N // 2


def as_nodes(nodes, d):
    nu = np.asarray(nodes, dtype=np.float64)
    if nu.ndim == 1 and d == 1:
        nu = nu[None, :]
    if nu.ndim != 2 or nu.shape[0] != d or nu.shape[1] < 1:
        raise ValueError("nodes is d x J")
    if not np.all((nu >= -0.5) & (nu < 0.5)):   # (NaN fails both)
        raise ValueError("a node lies outside [-0.5, 0.5)")
    return nu


def exact(nodes, shape):
    """the dense non-uniform DFT matrix (J x prod(shape)), complex128"""
    ext = extents(shape)
    nu = as_nodes(nodes, len(ext))
    ph = np.zeros((nu.shape[1], 1))
    for d, N in enumerate(ext):
        p = np.outer(nu[d], centred(N))
        ph = (ph[:, :, None] + p[:, None, :]).reshape(nu.shape[1], -1, order="F") if d else p
    return np.exp(-2j * np.pi * ph)


def i0(z):
    """I0 by its power series, all terms positive: sum_k (z^2 / 4)^k / (k!)^2, the loop of rls_nfft_create (z <= 8 b < 45: the terms
    fall below 2^-53 of the sum well inside 128 of them)"""
    z = np.asarray(z, dtype=np.float64)
    q = z * z / 4.0
    term, s = np.ones_like(z), np.ones_like(z)
    for k in range(1, 129):
        term = term * q / float(k * k)
        s = s + term
    return s


def window(t, m, b):
    s = (m - t) * (m + t)
    r = np.sqrt(np.maximum(s, 0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.sinh(b * r) / (np.pi * r)
    return np.where(s > 0.0, w, b / np.pi)


def phihat(N, n, m):
    b = np.pi * (2.0 - N / n)
    w = 2.0 * np.pi * centred(N) / n
    return i0(m * np.sqrt((b - w) * (b + w)))


class Plan:
    """what rls_nfft_create computes: per dimension (a signal has a second dimension of one point, one tap of weight 1 and a
    deapodisation of 1: exact factors) the deapodisation table, and per node the grid indices and weights of its taps"""

    def __init__(self, nodes, shape, m=4, dtype=np.complex128, plant=None):
        self.ext = extents(shape)
        self.d = len(self.ext)
        self.nu = as_nodes(nodes, self.d)
        self.J = self.nu.shape[1]
        if int(m) != m or not 1 <= m <= M_MAX:
            raise ValueError("m is an integer in 1 ... 8")
        self.m, self.dtype, self.plant = int(m), np.dtype(dtype), plant
        R = real_of(dtype)
        self.N = tuple(self.ext) + (1,) * (2 - self.d)
        self.n = tuple(grid_extent(N) for N in self.ext) + (1,) * (2 - self.d)
        self.size = int(np.prod(self.ext))
        self.dtab, self.q, self.w, self.u0 = [], [], [], []
        for d in range(2):
            N, n = self.N[d], self.n[d]
            if d >= self.d:
                self.dtab.append(np.ones(1, R))
                self.q.append(np.zeros((self.J, 1), np.int64))
                self.w.append(np.ones((self.J, 1), R))
                self.u0.append(np.zeros(self.J, np.int64))
                continue
            other = self.N[1 - d], self.n[1 - d]
            ph = phihat(*other, self.m) if plant == "phihat_swapped" and self.d == 2 else phihat(N, n, self.m)
            if ph.size != N:   # (the swapped table, brought to this dimension's length)
                ph = np.resize(ph, N)
            dt = 1.0 / ph
            if plant == "scale_n":
                dt = dt / n
            self.dtab.append(dt.astype(R))
            b = np.pi * (2.0 - N / n)
            v = n * self.nu[d]
            u0 = np.floor(v)
            first = u0 - self.m + (2 if plant == "taps_off_by_one" else 1)
            u = first[:, None] + np.arange(2 * self.m)[None, :]
            self.w.append(window(v[:, None] - u, self.m, b).astype(R))
            ui = u.astype(np.int64) + n // 2
            self.q.append(np.clip(ui, 0, n - 1) if plant == "no_wrap" else ui % n)
            self.u0.append(u0.astype(np.int64))
        # where the centred image sits in the centred grid
        self.lo = tuple(self.n[d] // 2 - self.N[d] // 2 + (1 if plant == "centre_off_by_one" and self.N[d] % 2 and d < self.d else 0)
                        for d in range(2))
        if self.d == 1:
            self.lo = (self.lo[0], 0)

    # ---- the two chains -------------------------------------------------------------------------------------------------------------
    def _taps(self):
        return [(t1, t2) for t2 in range(self.w[1].shape[1]) for t1 in range(self.w[0].shape[1])]

    def grid_of(self, x):
        """steps 1 and 2 of the forward: the transformed grid (n1, n2, batch)"""
        x = np.asarray(x)
        X = np.reshape(x.astype(self.dtype), self.N + (-1,), order="F")
        g = np.zeros(self.n + (X.shape[2],), self.dtype)
        g[self.lo[0]:self.lo[0] + self.N[0], self.lo[1]:self.lo[1] + self.N[1]] = (X * self.dtab[0][:, None, None]) * self.dtab[1][None, :, None]
        ax = (0, 1)
        return np.fft.fftshift(np.fft.fftn(np.fft.ifftshift(g, axes=ax), axes=ax), axes=ax).astype(self.dtype)

    def forward(self, x, parts=False):
        """A x of x (N,) or of the columns of (N, batch).  parts: also sum |w| |G| and sum |w| per output, and ||G||_2 per column"""
        x = np.asarray(x)
        G = self.grid_of(x)
        y = np.zeros((self.J, G.shape[2]), self.dtype)
        aw, a1 = np.zeros((self.J, G.shape[2])), np.zeros(self.J)
        for t1, t2 in self._taps():
            w = self.w[0][:, t1] * self.w[1][:, t2]
            v = G[self.q[0][:, t1], self.q[1][:, t2]]
            y = y + w[:, None] * v
            if parts:
                aw += np.abs(w.astype(np.float64))[:, None] * np.abs(v)
                a1 += np.abs(w.astype(np.float64))
        y = y if x.ndim == 2 else y[:, 0]
        if parts:
            return y, aw, a1, np.sqrt(np.sum(np.abs(G.astype(np.complex128)) ** 2, axis=(0, 1)))
        return y

    def spread(self, y, parts=False):
        y = np.asarray(y)
        Y = np.reshape(y.astype(self.dtype), (self.J, -1))
        G = np.zeros(self.n + (Y.shape[1],), self.dtype)
        aw, cnt = np.zeros(self.n + (Y.shape[1],)), np.zeros(self.n, np.int64)
        for t1, t2 in self._taps():
            w = self.w[0][:, t1] * self.w[1][:, t2]
            idx = (self.q[0][:, t1], self.q[1][:, t2])
            np.add.at(G, idx, w[:, None] * Y)
            if parts:
                np.add.at(aw, idx, np.abs(w.astype(np.float64))[:, None] * np.abs(Y))
                np.add.at(cnt, idx, 1)
        return (G, aw, cnt) if parts else G

    def adjoint(self, y, parts=False):
        """A^H y: the transpose chain.  parts: also the per-element pieces of the adjoint gate"""
        y = np.asarray(y)
        sp = self.spread(y, parts)
        G = sp[0] if parts else sp
        ax = (0, 1)
        h = np.fft.fftshift(np.fft.ifftn(np.fft.ifftshift(G, axes=ax), axes=ax, norm="forward"), axes=ax).astype(self.dtype)
        h = h[self.lo[0]:self.lo[0] + self.N[0], self.lo[1]:self.lo[1] + self.N[1]]
        X = (h * self.dtab[0][:, None, None]) * self.dtab[1][None, :, None]
        x = np.reshape(X, (self.size, -1), order="F")
        x = x if y.ndim == 2 else x[:, 0]
        if parts:
            nG = np.sqrt(np.sum(np.abs(G.astype(np.complex128)) ** 2, axis=(0, 1)))
            dk = np.reshape(np.abs(self.dtab[0].astype(np.float64))[:, None] * np.abs(self.dtab[1].astype(np.float64))[None, :], -1, order="F")
            return x, sp[1], sp[2], nG, dk
        return x

    def dense(self):
        return self.forward(np.eye(self.size, dtype=self.dtype))

    def dense_adjoint(self):
        return self.adjoint(np.eye(self.J, dtype=self.dtype))


def restated(nodes, shape, m=4, dtype=np.complex128, plant=None):
    return Plan(nodes, shape, m, dtype, plant)


# ---- the gates ---------------------------------------------------------------------------------------------------------------------------
V = 2.0 ** -53


def _mu(dtype):
    return (U[np.dtype(dtype)] if np.dtype(dtype) == C64 else 0.0) + 16 * V


def _gamma(T, u):
    return T * u / (1.0 - T * u)


def fft_gate(dtype, plan):
    return FR.gate(dtype, plan.n[:plan.d])


def forward_bound(dtype, plan, x):
    """(y, bound): plan (complex128) applied to x (N,) or (N, batch), and the rounding gate of a device of element type `dtype`,
    element by element"""
    u, d = U[np.dtype(dtype)], plan.d
    y, aw, a1, nG = plan.forward(x, parts=True)
    T = (2 * plan.m) ** d
    bound = (_gamma(T, u) + d * _mu(dtype) + (d - 1) * u) * aw + (fft_gate(dtype, plan) + 2 * d * u) * a1[:, None] * nG[None, :]
    bound = SECOND * bound
    return y, (bound if np.ndim(x) == 2 else bound[:, 0])


def adjoint_bound(dtype, plan, y):
    u, d = U[np.dtype(dtype)], plan.d
    x, aw, cnt, nG, dk = plan.adjoint(y, parts=True)
    e = (_gamma(np.maximum(cnt, 1), u)[:, :, None] + d * _mu(dtype) + (d - 1) * u) * aw
    e1 = np.sum(e, axis=(0, 1))
    X = np.reshape(x, (plan.size, -1))
    bound = dk[:, None] * (fft_gate(dtype, plan) * math.sqrt(plan.n[0] * plan.n[1]) * nG + e1)[None, :] + 2 * d * u * np.abs(X)
    bound = SECOND * bound
    return x, (bound if np.ndim(y) == 2 else bound[:, 0])


def ref_factor(dtype):
    """what a gate is multiplied by when the restatement in complex128 is the reference: 2 for a ComplexF64 device (the reference is no
    better than the working type and may err as much as the device), as fft_ref.ref_factor has it"""
    return 2.0 if np.dtype(dtype) == C128 else 1.0


def truncation(m, d, sigma=2.0):
    """Potts & Steidl's Kaiser-Bessel estimate, relative to ||x||_1, times the dimension"""
    return d * 4.0 * math.pi * (math.sqrt(m) + m) * (1.0 - 1.0 / sigma) ** 0.25 * math.exp(-2.0 * math.pi * m * math.sqrt(1.0 - 1.0 / sigma))


def check(label, got, want, bound):
    """error against a per-element bound, as fft_ref's judge has it"""
    err = np.abs(np.asarray(got).astype(np.complex128) - np.asarray(want).astype(np.complex128))
    excess = err - bound
    k = int(np.argmax(excess))
    assert excess.max() <= 0, (label, np.unravel_index(k, excess.shape), float(err.ravel()[k]), float(np.ravel(bound)[k]))
    return float(np.max(err / np.maximum(bound, np.finfo(np.float64).tiny)))


# ---- the cases of the device tier ----------------------------------------------------------------------------------------------------------
SHAPES = [(1,), (2,), (8,), (12,), (7,), (8, 6), (12, 20), (16, 16)]
MS = (1, 2, 4)


def ms_of(dtype):
    return MS + ((8,) if np.dtype(dtype) == C128 else ())


BELOW_HALF = float(np.nextafter(0.5, 0.0))


def node_sets(shape, m):
    """(name, nodes d x J) for one shape: the single nodes, nodes on grid points (the first of them has its last tap at t = -m: the
    limit), footprints that wrap at either end and at the corners, J = 1, 5, 70, one long cell list, one radial spoke (most cells
    empty) and repeated nodes"""
    ext = extents(shape)
    d = len(ext)
    n = [grid_extent(N) for N in ext]
    rng = np.random.default_rng(100 * sum(ext) + m)
    col = lambda *v: np.array(v, dtype=np.float64).reshape(d, -1)
    out = [("zero", col(*[0.0] * d)), ("minus half", col(*[-0.5] * d)), ("below half", col(*[BELOW_HALF] * d))]
    on = np.stack([((np.array([0, 1, -n[k] // 2, n[k] // 2 - 1, 3]) + n[k] // 2) % n[k] - n[k] // 2) / n[k] for k in range(d)])
    out.append(("on grid points", on))
    edge = [np.array([-0.5 + 0.3 / n[k], 0.5 - 0.3 / n[k], -0.5 + 0.3 / n[k], 0.5 - 0.3 / n[k], 0.1 / n[k]]) for k in range(d)]
    if d == 2:
        edge[1] = np.array([-0.5 + 0.6 / n[1], 0.5 - 0.6 / n[1], 0.5 - 0.6 / n[1], -0.5 + 0.6 / n[1], -0.5 + 0.6 / n[1]])
    out.append(("wrapping footprints", np.stack(edge)))
    for J in (1, 5, 70):
        out.append((f"random J={J}", rng.uniform(-0.5, 0.5, (d, J))))
    out.append(("one cell", np.stack([(min(1, n[k] // 2 - 1) + rng.uniform(0.0, 1.0, 70)) / n[k] for k in range(d)])))
    r = np.linspace(-0.5, 0.5, 33, endpoint=False)
    out.append(("one spoke", np.stack([r * c for c in ((1.0,) if d == 1 else (math.cos(0.3), math.sin(0.3)))])))
    rep = rng.uniform(-0.5, 0.5, (d, 4))
    out.append(("repeated", np.concatenate([rep, rep[:, ::-1], rep[:, :2]], axis=1)))
    return out


def gauss(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / math.sqrt(2.0)
