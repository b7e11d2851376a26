"""The blocked phase of PseudoInverse's factorisation (csrc/pinv.hip) restated in Float32 NumPy, followed by the
plain restatement `_jacobi` of tests/test_gpu_pinv.py -- no device needed.

Phase 1: the columns in blocks of b, the blocks in the round-robin tournament (a dummy block for an odd count); per block pair
G = X'X of the 2b columns (columns past N are zero columns), a cyclic two-sided Jacobi on G with the rotation of the plain
kernel (Newton-renormalised (c, s), null-level columns left alone, |g_pq| > tau_b sqrt(g_pp g_qq)) accumulating Q, then
X <- X Q on W and on V.  tau_b and the cap of blocked sweeps are read from csrc/rls_common.hpp, so the restatement follows them.

What it shows before any GPU run, on the matrices the GPU tests use: the blocked method stays inside the gates the plain
restatement sets (factor metrics within 4 x the plain restatement's, solutions within the solution gate), and the plain sweeps
behind phase 1 are fewer than without it."""
import os
import re

import numpy as np
import pytest

import rls_oracle as O
from test_gpu_pinv import _factor_metrics, _jacobi, _jacobi_solve, _rel, _truth, _yardstick

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_COMMON = open(os.path.join(ROOT, "regularizedleastsquares.jl_amd", "csrc", "rls_common.hpp")).read()
TOL = float(re.search(r"RLS_PINV_BLOCK_TOL = ([0-9.e-]+)f;", _COMMON).group(1))
CAP = int(re.search(r"RLS_PINV_BLOCK_CAP = (\d+);", _COMMON).group(1))
INNER = 10      # PINV_BLOCK_INNER, csrc/pinv.hip


def _players(m, r):
    i = np.arange(m // 2)
    p, q = np.where(i == 0, m - 1, (r + i) % (m - 1)), np.where(i == 0, r, (r - i + m - 1) % (m - 1))
    return np.minimum(p, q), np.maximum(p, q)


def _diag(G, tol, null):
    """cyclic two-sided Jacobi on the Hermitian G (n x n, n even): returns (Q, rotated) with Q'GQ diagonal to tol"""
    f = np.float32
    n = G.shape[0]
    G, Q = G.copy(), np.eye(n, dtype=G.dtype)
    did = False
    for _ in range(INNER):
        rotated = False
        for r in range(n - 1):
            p, q = _players(n, r)
            a, b, g = G[p, p].real.astype(f), G[q, q].real.astype(f), G[p, q]
            with np.errstate(invalid="ignore"):
                gabs, na, nb = np.abs(g).astype(f), np.sqrt(a), np.sqrt(b)
                act = (gabs > f(tol) * na * nb) & (na > null) & (nb > null)
            if not act.any():
                continue
            rotated = did = True
            p, q, a, b, g, gabs = p[act], q[act], a[act], b[act], g[act], gabs[act]
            ph = (g / gabs).astype(G.dtype)
            zeta = (b - a) / (f(2) * gabs)
            t = np.where(zeta >= 0, f(1), f(-1)) / (np.abs(zeta) + np.sqrt(f(1) + zeta * zeta))
            c = f(1) / np.sqrt(f(1) + t * t)
            s = c * t
            h = (-0.5 * (c.astype(np.float64) ** 2 + s.astype(np.float64) ** 2 - 1)).astype(f)
            c, s = c + h * c, s + h * s
            hp = (-0.5 * (ph.real.astype(np.float64) ** 2 + ph.imag.astype(np.float64) ** 2 - 1)).astype(f)
            ph = (ph + hp * ph).astype(G.dtype)
            for X in (G, Q):                               # columns: X <- X J
                xp, qt = X[:, p], ph.conj() * X[:, q]
                X[:, p], X[:, q] = c * xp - s * qt, s * xp + c * qt
            gp, qt = G[p, :], ph[:, None] * G[q, :]        # rows: G <- J' G
            G[p, :], G[q, :] = c[:, None] * gp - s[:, None] * qt, s[:, None] * gp + c[:, None] * qt
        if not rotated:
            break
    return Q, did


def _blocked_phase(A, b, tol=TOL, cap=CAP):
    """phase 1 alone: (W, V, blocked sweeps)"""
    f = np.float32
    M, N = A.shape
    W, V = A.copy(), np.eye(N, dtype=A.dtype)
    null = f(1e-6) * np.sqrt((np.abs(W) ** 2).sum(dtype=f))
    nb = -(-N // b)
    mb = nb + (nb & 1)
    sweeps = 0
    if nb < 2:
        return W, V, 0
    while sweeps < cap:
        sweeps += 1
        rotated = False
        for r in range(mb - 1):
            for P, Q in zip(*_players(mb, r)):
                if Q >= nb:
                    continue
                cols = np.concatenate([np.arange(P * b, P * b + b), np.arange(Q * b, Q * b + b)])
                ok = cols < N
                X = np.zeros((M, 2 * b), dtype=A.dtype)
                X[:, ok] = W[:, cols[ok]]
                Qm, did = _diag(X.conj().T @ X, tol, null)
                if not did:
                    continue
                rotated = True
                W[:, cols[ok]] = (X @ Qm)[:, ok]
                Y = np.zeros((N, 2 * b), dtype=A.dtype)
                Y[:, ok] = V[:, cols[ok]]
                V[:, cols[ok]] = (Y @ Qm)[:, ok]
        if not rotated:
            break
    return W, V, sweeps


def blocked_jacobi(A, b, tol=TOL, cap=CAP):
    """phase 1, then the plain sweeps on its result: (W, V, plain sweeps, blocked sweeps)"""
    W1, V1, bs = _blocked_phase(A, b, tol, cap)
    W, R, sweeps = _jacobi(W1)            # W1 = W R': the plain restatement starts from V = I
    return W, (V1 @ R).astype(A.dtype), sweeps, bs


def deficient(case, dt):
    """the rank-deficient matrices of the blocked tests: (A, b, lambda)"""
    if case == "wide3":
        A, _, B = O.make_problem(3, 40, dt, 521)
        return A, B, 0.5
    if case == "wide40":
        A, _, B = O.make_problem(40, 63, dt, 511)
        return A, B, 0.5
    A, _, B = O.make_problem(96, 64, dt, 512)
    A = A.copy(order="F")
    A[:, 5] = A[:, 20]       # a repeated column, both inside one block pair ...
    A[:, 10] = 0             # ... and a zero column
    return A, B, 0.5


def factor_metrics2(A, W, V):
    """(||W V' - A|| / ||A||, ||V'V - I||): the two factor metrics that also exist for a wide A"""
    A64, W, V = A.astype(np.complex128), W.astype(np.complex128), V.astype(np.complex128)
    return float(np.linalg.norm(W @ V.conj().T - A64) / np.linalg.norm(A64)), float(np.linalg.norm(V.conj().T @ V - np.eye(V.shape[1])))


FULL = [(96, 64), (200, 130), (70, 33), (520, 48)]
DTYPES = [np.float32, np.complex64]


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "c64"])
@pytest.mark.parametrize("shape", FULL, ids=[f"{m}x{n}" for m, n in FULL])
def test_blocked_restatement_stays_inside_the_gates_and_saves_plain_sweeps(shape, dt):
    M, N = shape
    A, _, B = O.make_problem(M, N, dt, 300 + N + M, n_rhs=3)
    Wp, Vp, sweeps_plain = _jacobi(A)
    want = _factor_metrics(A, Wp, Vp)
    W, V, sweeps, bs = blocked_jacobi(A, 16)
    got = _factor_metrics(A, W, V)
    truth, yard = _truth(A, B, 0.0), _yardstick(A, B, 0.0)
    e, ey = _rel(_jacobi_solve(W, V, B, 0.0), truth), _rel(yard, truth)
    print(f"{M}x{N} {np.dtype(dt).name}: blocked {got} plain {want}; plain sweeps {sweeps} (without phase 1: {sweeps_plain}), "
          f"blocked sweeps {bs}; solution {e:.2e} (LAPACK {ey:.2e})")
    for g, w in zip(got, want):
        assert g <= 4 * w
    assert e <= max(1e-5, 4 * ey)
    assert 1 <= bs <= CAP and sweeps < sweeps_plain


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "c64"])
@pytest.mark.parametrize("case", ["wide3", "wide40", "repeated+zero"])
def test_blocked_restatement_on_rank_deficient_matrices(case, dt):
    A, b, lam = deficient(case, dt)
    Wp, Vp, sweeps_plain = _jacobi(A)
    W, V, sweeps, bs = blocked_jacobi(A, 16)
    truth = _truth(A, b, lam)
    e, e_plain = _rel(_jacobi_solve(W, V, b, lam), truth), _rel(_jacobi_solve(Wp, Vp, b, lam), truth)
    print(f"{case} {np.dtype(dt).name}: blocked {e:.2e} plain {e_plain:.2e}; plain sweeps {sweeps} (without phase 1: {sweeps_plain}), blocked {bs}")
    assert e <= 4 * e_plain and sweeps < sweeps_plain
    got, want = factor_metrics2(A, W, V), factor_metrics2(A, Wp, Vp)
    assert got[0] <= 4 * want[0] and got[1] <= 4 * want[1]


def test_orthogonal_columns_are_left_alone():
    A = np.zeros((40, 33), dtype=np.complex64)
    A[np.arange(33), np.arange(33)] = np.arange(1, 34) * (1 + 1j)
    W, V, bs = _blocked_phase(A, 16)
    assert bs == 1 and W.tobytes() == A.tobytes() and np.array_equal(V, np.eye(33, dtype=np.complex64))
