"""CPU tests of tests/nfft_ref.py, the checker of NFFTOp (csrc/nfft.hip): the restatement in complex128
against the dense non-uniform DFT within the published truncation bound for every case of tests/test_gpu_nfft.py, the restated
adjoint against the conjugate transpose of the restated forward, and planted mistakes that the gates must catch."""
import numpy as np
import pytest

import nfft_ref as NR

CASES = [(s_, m_) for s_ in NR.SHAPES for m_ in NR.ms_of(np.complex128)]
IDS = ["x".join(map(str, s_)) + f"-m{m_}" for s_, m_ in CASES]


def _worst(shape, m, plant=None, sets=None):
    """the largest truncation error of the restated forward and adjoint over the node sets, relative to ||x||_1 / ||y||_1"""
    worst = 0.0
    N = int(np.prod(shape))
    for name, nodes in NR.node_sets(shape, m):
        if sets is not None and name not in sets:
            continue
        E = NR.exact(nodes, shape)
        P = NR.restated(nodes, shape, m, np.complex128, plant)
        x, y = NR.gauss(N, 5), NR.gauss(P.J, 6)
        worst = max(worst, np.abs(P.forward(x) - E @ x).max() / np.abs(x).sum(), np.abs(P.adjoint(y) - E.conj().T @ y).max() / np.abs(y).sum(),
                    np.abs(P.dense() - E).max())
    return worst


@pytest.mark.parametrize("shape,m", CASES, ids=IDS)
def test_restated_meets_the_published_truncation_bound(shape, m):
    d = len(NR.extents(shape))
    got, bound = _worst(shape, m), NR.truncation(m, d)
    print(f"truncation {shape} m={m}: {got:.3e} (bound {bound:.3e})")
    assert got <= bound, (shape, m, got, bound)


def test_exact_is_the_definition():
    """entry by entry against exp(-2 pi i k . nu) written out, odd and even extents, first extent fastest"""
    nodes = np.array([[-0.5, 0.1, 0.25], [0.3, -0.2, NR.BELOW_HALF]])
    E = NR.exact(nodes, (3, 4))
    assert E.shape == (3, 12) and E.dtype == np.complex128
    for j in range(3):
        for i2, k2 in enumerate(range(-2, 2)):
            for i1, k1 in enumerate(range(-1, 2)):
                assert abs(E[j, i1 + 3 * i2] - np.exp(-2j * np.pi * (k1 * nodes[0, j] + k2 * nodes[1, j]))) <= 1e-15
    assert np.array_equal(NR.exact(nodes[0], (3,)), NR.exact(nodes[:1], (1, 3, 1)))
    assert np.array_equal(NR.exact([0.2], (1,)), np.ones((1, 1)))
    assert [NR.grid_extent(N) for N in (1, 2, 7, 8, 12, 16, 20)] == [2, 4, 16, 16, 32, 32, 64]


@pytest.mark.parametrize("shape,m", CASES, ids=IDS)
def test_restated_adjoint_is_the_conjugate_transpose(shape, m):
    for name, nodes in NR.node_sets(shape, m):
        P = NR.restated(nodes, shape, m)
        F, T = P.dense(), P.dense_adjoint()
        assert np.abs(T - F.conj().T).max() <= 1e-13 * max(1.0, np.abs(F).max()), (name, np.abs(T - F.conj().T).max())
        x, y = NR.gauss(P.size, 7), NR.gauss(P.J, 8)
        assert abs(np.vdot(y, P.forward(x)) - np.vdot(P.adjoint(y), x)) <= 1e-13 * np.linalg.norm(x) * np.linalg.norm(y) * np.sqrt(P.J * P.size)


def test_restated_in_single_precision_is_within_its_own_gate():
    """the complex64 restatement is a device of element type ComplexF32 as far as the gate knows: it must pass, and does not pass the
    ComplexF64 gate"""
    for shape, m in (((12,), 4), ((8, 6), 2), ((16, 16), 4)):
        for name, nodes in NR.node_sets(shape, m):
            P, S = NR.restated(nodes, shape, m), NR.restated(nodes, shape, m, np.complex64)
            x, y = NR.gauss(P.size, 9).astype(np.complex64), NR.gauss(P.J, 10).astype(np.complex64)
            want, bound = NR.forward_bound(np.complex64, P, x)
            NR.check(f"{shape} {name} forward", S.forward(x), want, bound)
            want, bound = NR.adjoint_bound(np.complex64, P, y)
            NR.check(f"{shape} {name} adjoint", S.adjoint(y), want, bound)
    P, S = NR.restated(nodes, shape, m), NR.restated(nodes, shape, m, np.complex64)
    want, bound = NR.forward_bound(np.complex128, P, x)
    with pytest.raises(AssertionError):
        NR.check("single against the double gate", S.forward(x), want, bound)


@pytest.mark.parametrize("plant", NR.PLANTS)
def test_planted_mistakes_are_caught(plant):
    """every plant breaks the truncation bound against `exact` AND the ComplexF32 rounding gate against the sound restatement, on a
    shape where it can show: 8 x 6 for the swapped tables (the extents differ), 7 for the odd centring, m = 4 throughout"""
    shape = {"phihat_swapped": (8, 6), "centre_off_by_one": (7,)}.get(plant, (12,))
    sets = ("wrapping footprints",) if plant == "no_wrap" else None
    d = len(NR.extents(shape))
    assert _worst(shape, 4, None, sets) <= NR.truncation(4, d)
    assert _worst(shape, 4, plant, sets) > NR.truncation(4, d), plant
    name, nodes = [s_ for s_ in NR.node_sets(shape, 4) if s_[0] == (sets[0] if sets else "random J=70")][0]
    P, B = NR.restated(nodes, shape, 4), NR.restated(nodes, shape, 4, np.complex128, plant)
    x = NR.gauss(P.size, 11)
    want, bound = NR.forward_bound(np.complex64, P, x)
    with pytest.raises(AssertionError):
        NR.check(plant, B.forward(x), want, bound)
    want, bound = NR.adjoint_bound(np.complex64, P, NR.gauss(P.J, 12))
    with pytest.raises(AssertionError):
        NR.check(plant, B.adjoint(NR.gauss(P.J, 12)), want, bound)


def test_the_gates_are_of_the_size_the_derivation_gives():
    """ComplexF32, 16 x 16, m = 4: 64 taps, a 32 x 32 grid -- the transform's share is eG sqrt(n_1 n_2) ||x||_2 up to the
    window's spread, about 32 x 5e-6, the chain's a few 1e-6; the ComplexF64 gate is 2^-29 of it up to the 16 v evaluation term"""
    nodes = NR.node_sets((16, 16), 4)[7][1]
    P = NR.restated(nodes, (16, 16), 4)
    x = NR.gauss(256, 13)
    y, b32 = NR.forward_bound(np.complex64, P, x)
    _, b64 = NR.forward_bound(np.complex128, P, x)
    assert 1e-6 * np.linalg.norm(x) < b32.max() < 1e-3 * np.linalg.norm(x)
    assert np.all(b64 < b32 * 2.0 ** -24) and np.all(b64 > b32 * 2.0 ** -31)
