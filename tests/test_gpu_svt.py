"""The singular-value-thresholding kernel (csrc/svt.hip, svt_blocks_kernel<E, NW>: the whole device side of NuclearRegularization and
LLRRegularization) on structured spectra, at every wave count and at the edges of its launcher.

Truth: O.prox_nuclear / O.prox_llr (LAPACK svd) in float64 / complex128 on the input AFTER it was rounded to the element type.
Gate: conftest.parity_check, unchanged -- relative l2 <= 1e-5 against the truth, or <= 2 x the error the same oracle makes when it
runs in the element type (LAPACK in Float32) on the same input.  Every case prints both errors (`pytest -s`); the table of one
MI355X run is profiles/svt_prox_edges.txt.

The launcher picks NW, the waves per matrix, from the geometry alone (svt_launch; nv = min(rows, K) vectors are orthogonalised,
a wave rotates four pairs at a time, so one pass of the pair loop covers 4 NW pairs of a round):

    pairs = (nv + 1) // 2
    cap   = smallest power of two with 4 * cap >= pairs, at most 16
            nv 1..8 -> 1, 9..16 -> 2, 17..32 -> 4, 33..64 -> 8, >= 65 -> 16
    want  = 16 for nb <= 256 blocks, else max(1, 16 // ceil(nb / 256))
    NW    = largest power of two <= min(want, cap)
    passes of the pair loop = ceil(pairs / (4 NW))

The tests cannot observe NW; they choose their shapes from this table (`waves`, `passes` below restate it and every group asserts
the values it is aimed at, so a case that no longer restates the launcher is found by reading the two side by side).  `tr` is the
kernel's orientation flag: K > rows, the rows of X are orthogonalised instead of its columns.

  group                                   element types   NW (passes of the pair loop)
  NUCLEAR_SHAPES  5x3                     both            1 (1)
                  9x40 (tr), 40x9         both            2 (1), odd nv with a dummy player
                  17x17                   both            4 (1 .. 9 pairs of 16), odd nv
                  33x48 (tr), 64x33       both            8 (1), odd nv
                  64x64                   both            8 (1), all 32 slots of a round taken
                  65x70 (tr)              both            16 (1), odd nv
  largest accepted 97x97                  ComplexF32      16 (1)
                   138x138                Float32         16 (2: 69 pairs, 64 per pass)
  LLR ladder nb = 200, 272                Float32         8 (1)   nv = 33, 17 pairs
             nb = 600                     Float32         4 (2)
             nb = 1100                    Float32         2 (3)
             nb = 2100                    Float32         1 (5)
  LLR 9 blocks of 72 x 66                 ComplexF32      16 (1 .. 33 pairs of 64)
  LLR geometry edges                      both            1 (1), or 2 (1) for the 3-D case (nv = 12)
so all ten instantiations (Float32 / ComplexF32 x NW 1, 2, 4, 8, 16) are launched by a case that says so, and the pair loop takes
two or more passes at NW = 16 (138x138) and at NW = 1 (nb = 2100).

The structured families run on every NUCLEAR_SHAPES entry.  Each is built in float64 as (U * s) V^H with U, V from numpy.linalg.qr of
seeded Gaussian draws, rounded to the element type; before the device is compared, `case` checks on the float64 oracle alone that
the prox moves the input by more than ten gates (a kernel that does nothing could not pass) and, where a family is aimed at one
of the kernel's two reconstructions (`subtract`: X - removed part when the removed part is the smaller one; direct: the kept part),
that the exact singular values put it there.

Observed on an MI355X (profiles/svt_prox_edges.txt): largest device error 4.5e-6 (duplicated columns, 64 x 64 ComplexF32; the exact null
vectors end under the kernel's null_tol still correlated with the rest), largest device / LAPACK ratio 55 (rank 2, 64 x 64 ComplexF32:
3.3e-6 against 5.9e-8).  graded_direct found the drift of c^2 + s^2 in the rotations (2.3e-5 at 65 x 70 ComplexF32 before the
rotation was renormalised, 1.0e-6 since)."""
import functools
import math

import numpy as np
import pytest

import rls_oracle as O
from conftest import parity_check  # noqa: E402  (the gate: <= 1e-5 vs float64, or <= 2 x the Float32 oracle's own error)

pytestmark = pytest.mark.gpu
F32, C64 = np.float32, np.complex64
DT = [F32, C64]
GATE = 1e-5  # (the first arm of parity_check, for the preconditions on the oracle)
LDS_LIMIT = 150 * 1024  # csrc/svt.hip, svt_launch


def hi(dt):
    return np.complex128 if np.dtype(dt).kind == "c" else np.float64


def name(dt):
    return np.dtype(dt).name


def rel(a, b):
    """conftest._rel: relative l2, absolute where the reference is zero"""
    a, b = np.asarray(a).astype(np.complex128), np.asarray(b).astype(np.complex128)
    n, d = np.linalg.norm(b), np.linalg.norm(a - b)
    return float(d / n) if n > 0 else float(d)


# ---- the launcher's table ----------------------------------------------------------------------------------------------------------
def waves(nv, nb=1):
    pairs = (nv + 1) // 2
    cap = 1
    while cap * 4 < pairs and cap < 16:
        cap *= 2
    want = 16 if nb <= 256 else max(1, 16 // -(-nb // 256))
    nw = 1
    while nw * 2 <= min(want, cap):
        nw *= 2
    return nw


def passes(nv, nb=1):
    return -(-((nv + 1) // 2) // (4 * waves(nv, nb)))


def lds_bytes(dt, nv, length):
    return (nv * length + nv * nv) * np.dtype(dt).itemsize + (2 * nv + 16) * 4


def test_the_table_of_the_module_docstring():
    assert [waves(nv) for nv in (1, 8, 9, 16, 17, 32, 33, 64, 65, 138)] == [1, 1, 2, 2, 4, 4, 8, 8, 16, 16]
    assert [waves(33, nb) for nb in (200, 256, 257, 272, 600, 1100, 2100)] == [8, 8, 8, 8, 4, 2, 1]
    assert [passes(33, nb) for nb in (200, 272, 600, 1100, 2100)] == [1, 1, 2, 3, 5]
    assert (passes(97), passes(138), passes(66)) == (1, 2, 1)


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def gauss(rng, shape, dt):
    v = rng.standard_normal(shape)
    if np.dtype(dt).kind == "c":
        v = v + 1j * rng.standard_normal(shape)
    return v


def from_spectrum(rng, m, n, s, dt):
    nv = min(m, n)
    U = np.linalg.qr(gauss(rng, (m, nv), dt))[0]
    V = np.linalg.qr(gauss(rng, (n, nv), dt))[0]
    return (U * np.asarray(s, np.float64)) @ V.conj().T


def _first(nv, *head):
    s = np.zeros(nv)
    s[:len(head)] = head
    return s


def _dupcols(rng, m, n, dt):
    X = gauss(rng, (m, n), dt)
    h = n // 2
    X[:, h:2 * h] = X[:, :h]
    return X


def _zero_rowcol(rng, m, n, dt):
    X = gauss(rng, (m, n), dt)
    X[0, :] = 0
    X[:, 0] = 0
    return X


def _single(rng, m, n, dt):
    X = np.zeros((m, n), hi(dt))
    X[m // 2, n // 3] = 3.0 * (0.6 - 0.8j) if np.dtype(dt).kind == "c" else 3.0
    return X


# family -> (matrix in float64 from (rng, m, n, dt), lambda, the reconstruction it is aimed at or None)
FAMILIES = {
    "rank1": (lambda r, m, n, dt: from_spectrum(r, m, n, _first(min(m, n), 3.0), dt), 1.0, "subtract"),
    "rank2": (lambda r, m, n, dt: from_spectrum(r, m, n, _first(min(m, n), 3.0, 1.5), dt), 0.5, "subtract"),
    "equal": (lambda r, m, n, dt: from_spectrum(r, m, n, np.full(min(m, n), 2.0), dt), 0.5, "subtract"),
    "cluster": (lambda r, m, n, dt: from_spectrum(r, m, n, np.where(np.arange(min(m, n)) < min(m, n) // 2, 1.0, 1.0 + 1e-4), dt), 0.3,
                "subtract"),
    "graded_subtract": (lambda r, m, n, dt: from_spectrum(r, m, n, np.logspace(0, -6, min(m, n)), dt), 1e-3, "subtract"),
    "graded_direct": (lambda r, m, n, dt: from_spectrum(r, m, n, np.logspace(0, -6, min(m, n)), dt), 0.5, "direct"),
    "dupcols": (_dupcols, 0.7, None),
    "zero_rowcol": (_zero_rowcol, 0.7, None),
    "single": (_single, 1.5, None),   # 0.5 x |the entry|: kept and removed parts are equal, either reconstruction may run
}
#                 m   n  NW
NUCLEAR_SHAPES = [(5, 3, 1), (9, 40, 2), (40, 9, 2), (17, 17, 4), (33, 48, 8), (64, 33, 8), (64, 64, 8), (65, 70, 16)]
SHAPE_IDS = [f"{m}x{n}" for m, n, _ in NUCLEAR_SHAPES]


def _gaussian_case(m, n, dt, spread=True):
    """the recipe of test_prox_nuclear_matches_svd: Gaussian, column 0 ten times larger, lambda = 0.3 x the middle singular value"""
    X = gauss(np.random.default_rng([61, m, n, np.dtype(dt).kind == "c"]), (m, n), dt)
    if spread:
        X[:, 0] *= 10
    return X, 0.3 * float(np.linalg.svd(X, compute_uv=False)[min(m, n) // 2])


@functools.lru_cache(maxsize=None)
def case(family, m, n, dtname, scale=1.0):
    """(x in the element type, lambda, float64 truth, the Float32 oracle's result), computed once and read-only.
    `scale` multiplies the rounded input and lambda (a power of two: exact)."""
    dt = np.dtype(dtname).type
    if family == "gaussian":
        X, lam, aim = *_gaussian_case(m, n, dt), None
    elif family == "gaussian_plain":
        X, lam, aim = *_gaussian_case(m, n, dt, spread=False), None
    else:
        make, lam, aim = FAMILIES[family]
        X = make(np.random.default_rng([sorted(FAMILIES).index(family), m, n, np.dtype(dt).kind == "c"]), m, n, dt)
    x = X.reshape(-1, order="F").astype(dt) * dt(scale)
    lam = lam * scale
    x64, nv = x.astype(hi(dt)), min(m, n)
    s = np.linalg.svd(x64.reshape(m, n, order="F"), compute_uv=False)
    kept2, gone2 = float(np.sum(np.maximum(s - lam, 0) ** 2)), float(np.sum(np.minimum(s, lam) ** 2))
    if aim is not None:  # the kernel's `gone2 < kept2`.  graded_direct at nv = 3 keeps 0.5 of 1.0 and is on the direct side by 4e-6 only:
        # there either form may run and either must be right; from nv = 9 on the removed part is the larger one by 13 % (nv = 9) or more
        assert (2 * gone2 < kept2) if aim == "subtract" else (kept2 < gone2 and (nv < 9 or 1.1 * kept2 < gone2)), (family, m, n, kept2, gone2)
    ref64 = O.prox_nuclear(x64.copy(), lam, (m, n))
    assert np.linalg.norm(ref64) > 0 and rel(x64, ref64) > 10 * GATE, (family, m, n, "the prox barely moves this input")
    ref32 = O.prox_nuclear(x.copy(), lam, (m, n))
    assert ref32.dtype == x.dtype
    for a in (x, ref64, ref32):
        a.setflags(write=False)
    return x, lam, ref64, ref32


def device_nuclear(rls, ctx, x, lam, m, n):
    xd = rls.DeviceVector.from_host(np.array(x), ctx)
    rls.prox_(rls.NuclearRegularization(lam, svtShape=(m, n)), xd)
    return xd.to_host()


def gate(tag, got, ref64, ref32):
    e, e32 = rel(got, ref64), rel(ref32, ref64)
    print(f"{tag}: device {e:.3e}  LAPACK-Float32 {e32:.3e}  ratio {e / e32 if e32 > 0 else float('inf'):.2f}")
    parity_check(tag, got, ref64, ref32, record=False)
    return e


# ---- 2. nuclear prox: every instantiation in both orientations, and the largest matrices the launcher accepts -----------------------
@pytest.mark.parametrize("dt", DT, ids=name)
@pytest.mark.parametrize("m,n,nw", NUCLEAR_SHAPES, ids=SHAPE_IDS)
def test_nuclear_every_wave_count(rls, ctx, dt, m, n, nw):
    assert waves(min(m, n)) == nw and passes(min(m, n)) == 1
    x, lam, ref64, ref32 = case("gaussian", m, n, name(dt))
    gate(f"nuclear_gaussian_{m}x{n}_{name(dt)}_NW{nw}", device_nuclear(rls, ctx, x, lam, m, n), ref64, ref32)


@pytest.mark.parametrize("dt,m,npasses", [(C64, 97, 1), (F32, 138, 2)], ids=["97x97-complex64", "138x138-float32"])
def test_nuclear_largest_accepted(rls, ctx, dt, m, npasses):
    """one more row and column do not fit (test_refusal_above_the_lds_limit); 138 x 138: 69 pairs, the pair loop's second pass at NW = 16"""
    assert lds_bytes(dt, m, m) <= LDS_LIMIT < lds_bytes(dt, m + 1, m + 1)
    assert waves(m) == 16 and passes(m) == npasses
    x, lam, ref64, ref32 = case("gaussian", m, m, name(dt))
    gate(f"nuclear_gaussian_{m}x{m}_{name(dt)}_NW16_passes{npasses}", device_nuclear(rls, ctx, x, lam, m, m), ref64, ref32)


# ---- 3. structured spectra ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT, ids=name)
@pytest.mark.parametrize("m,n,nw", NUCLEAR_SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_nuclear_structured(rls, ctx, family, dt, m, n, nw):
    assert waves(min(m, n)) == nw
    x, lam, ref64, ref32 = case(family, m, n, name(dt))
    gate(f"nuclear_{family}_{m}x{n}_{name(dt)}_NW{nw}", device_nuclear(rls, ctx, x, lam, m, n), ref64, ref32)


@pytest.mark.parametrize("dt", DT, ids=name)
@pytest.mark.parametrize("m,n", [(9, 40), (40, 9), (17, 17), (64, 33)])
def test_nuclear_zero_matrix_stays_zero(rls, ctx, dt, m, n):
    got = device_nuclear(rls, ctx, np.zeros(m * n, dt), 0.5, m, n)
    assert got.dtype == np.dtype(dt) and np.array_equal(got, np.zeros(m * n, dt))


# ---- 4. what the kernel's design promises exactly --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT, ids=name)
@pytest.mark.parametrize("family,m,n", [("gaussian", 40, 9), ("gaussian", 9, 40), ("rank2", 40, 9), ("dupcols", 64, 33)])
def test_lambda_zero_returns_the_input(rls, ctx, dt, family, m, n):
    """fac = sigma / sigma = 1 for every vector; the subtract form then removes exactly zero from the input it reads again"""
    x = case(family, m, n, name(dt))[0]
    assert np.array_equal(device_nuclear(rls, ctx, x, 0.0, m, n), x)


@pytest.mark.parametrize("dt", DT, ids=name)
@pytest.mark.parametrize("family,m,n", [("rank1", 33, 48), ("rank1", 40, 9), ("dupcols", 64, 33), ("dupcols", 9, 40)])
def test_lambda_above_the_spectrum_gives_exact_zeros(rls, ctx, dt, family, m, n):
    """every fac is 0: nothing is kept, the direct form sums zeros"""
    x = case(family, m, n, name(dt))[0]
    smax = float(np.linalg.svd(x.astype(hi(dt)).reshape(m, n, order="F"), compute_uv=False)[0])
    assert np.array_equal(device_nuclear(rls, ctx, x, 1.01 * smax, m, n), np.zeros(m * n, dt))


@pytest.mark.parametrize("dt", DT, ids=name)
@pytest.mark.parametrize("m,n", [(65, 70), (33, 48)])
def test_two_runs_give_the_same_bits(rls, ctx, dt, m, n):
    """the pairs of a round are disjoint and every sum has a fixed order: no result may depend on which wave arrives first"""
    x, lam = case("gaussian", m, n, name(dt))[:2]
    assert np.array_equal(device_nuclear(rls, ctx, x, lam, m, n), device_nuclear(rls, ctx, x, lam, m, n))


# ---- 5. data far from unit scale ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT, ids=name)
@pytest.mark.parametrize("k", [-40, -20, 20, 40])
@pytest.mark.parametrize("family,m,n", [("gaussian_plain", 33, 48), ("rank2", 40, 9)])
def test_nuclear_far_from_unit_scale(rls, ctx, dt, family, m, n, k):
    """input and lambda times 2^k: squared norms stay normal Float32 numbers (2^-80 .. 2^93) and every threshold of the kernel is relative,
    so the gate, relative to the scaled truth, holds as at k = 0 (bit-for-bit homogeneity is not asked: hypotf need not have it)"""
    x, lam, ref64, ref32 = case(family, m, n, name(dt), scale=2.0 ** k)
    x1 = case(family, m, n, name(dt))[0]
    assert np.array_equal(x, x1 * dt(2.0 ** k)) and np.all(np.isfinite(x))
    gate(f"nuclear_{family}_{m}x{n}_{name(dt)}_2^{k}", device_nuclear(rls, ctx, x, lam, m, n), ref64, ref32)


# ---- 6. / 7. LLR --------------------------------------------------------------------------------------------------------------------------------
def llr_blocks(shape, bs):
    nblk = [-(-s // b) for s, b in zip(shape, bs)]
    for start in np.ndindex(*nblk):
        yield tuple(slice(st * b, min((st + 1) * b, s)) for st, b, s in zip(start, bs, shape))


def low_rank_series(seed, dt, shape, bs, K, shift, rank=3, noise=1e-3, zero_every=10):
    """an image series whose blocks, on the grid shifted by `shift`, are rank `rank` plus noise; every `zero_every`-th block is zero
    altogether (the oracle skips such a block, the kernel runs on it).  Returns x (element type) and the mask of the zeroed entries."""
    rng = np.random.default_rng(seed)
    mb = int(np.prod(bs))
    xs = np.zeros(tuple(shape) + (K,), hi(dt))
    zero = np.ones(xs.shape, bool)
    for j, sl in enumerate(llr_blocks(shape, bs)):
        if j % zero_every == 0:
            continue
        M = gauss(rng, (mb, rank), dt) @ gauss(rng, (rank, K), dt) + noise * gauss(rng, (mb, K), dt)
        cut = tuple(slice(0, s.stop - s.start) for s in sl)
        xs[sl] = M.reshape(tuple(bs) + (K,), order="F")[cut]
        zero[sl] = False
    axes = tuple(range(len(shape)))
    back = tuple(-s for s in shift)
    x = np.roll(xs, back, axis=axes).reshape(-1, order="F").astype(dt)
    return x, np.roll(zero, back, axis=axes).reshape(-1, order="F")


def check_llr(rls, ctx, tag, x, lam, shape, bs, shift):
    dt = x.dtype
    x64 = x.astype(hi(dt))
    ref64 = O.prox_llr(x64.copy(), lam, shape, bs, shift)
    assert np.linalg.norm(ref64) > 0 and rel(x64, ref64) > 10 * GATE, (tag, "the prox barely moves this input")
    ref32 = O.prox_llr(x.copy(), lam, shape, bs, shift)
    assert ref32.dtype == dt
    xd = rls.DeviceVector.from_host(x, ctx)
    rls.LLRRegularization(lam, shape=shape, blockSize=bs, randshift=False)._call(xd, lam, list(shift))
    got = xd.to_host()
    gate(tag, got, ref64, ref32)
    return got


@pytest.mark.parametrize("nb,nw,npasses", [(200, 8, 1), (272, 8, 1), (600, 4, 2), (1100, 2, 3), (2100, 1, 5)])
def test_llr_block_count_ladder(rls, ctx, nb, nw, npasses):
    """36-voxel blocks of 33 frames (nv = 33, 17 pairs a round) on a 1-D image whose last block is cut: the launcher gives a matrix fewer
    waves as the blocks multiply, down to one wave that takes the pairs of a round in five passes"""
    shape, bs, K, shift = (36 * nb - 5,), (36,), 33, (7,)
    assert (waves(33, nb), passes(33, nb)) == (nw, npasses)
    x, zero = low_rank_series([6, nb], F32, shape, bs, K, shift)
    got = check_llr(rls, ctx, f"llr_ladder_nb{nb}_float32_NW{nw}_passes{npasses}", x, 0.05, shape, bs, shift)
    assert zero.sum() == -(-nb // 10) * 36 * K and np.array_equal(got[zero], np.zeros(int(zero.sum()), F32))


def test_llr_sixteen_waves_complex(rls, ctx):
    """9 blocks of 72 voxels x 66 frames, ComplexF32: nv = 66, NW = 16"""
    shape, bs, K, shift = (27, 24), (9, 8), 66, (4, 3)
    assert (waves(66, 9), passes(66, 9)) == (16, 1)
    x, zero = low_rank_series([6, 66], C64, shape, bs, K, shift)
    got = check_llr(rls, ctx, "llr_72x66_nb9_complex64_NW16", x, 0.05, shape, bs, shift)
    assert zero.sum() == 72 * K and np.array_equal(got[zero], np.zeros(72 * K, C64))


#            shape      blockSize  K   shift       nv
LLR_EDGES = [((5,), (8,), 6, (0,), 6),                     # the block is larger than the image
             ((4, 3), (1, 1), 5, (0, 0), 1),               # one voxel a block: every frame vector is shrunk by its norm
             ((12,), (5,), 1, (2,), 1),                    # one frame
             ((10, 9), (4, 3), 5, (4, 3), 5),              # a shift of one whole block
             ((12,), (5,), 4, (29,), 4),                   # a shift beyond the image: taken modulo the shape
             ((5, 4, 3), (2, 3, 2), 14, (1, 2, 1), 12)]    # 3-D, cut in every dimension, more frames than voxels in a block


@pytest.mark.parametrize("dt", DT, ids=name)
@pytest.mark.parametrize("shape,bs,K,shift,nv", LLR_EDGES, ids=[f"{c[0]}-{c[1]}-K{c[2]}-shift{c[3]}" for c in LLR_EDGES])
def test_llr_geometry_edges(rls, ctx, dt, shape, bs, K, shift, nv):
    assert nv == min(int(np.prod(bs)), K)
    n = int(np.prod(shape)) * K
    x = gauss(np.random.default_rng([7, n, len(shape), K]), n, dt).astype(dt)
    check_llr(rls, ctx, f"llr_edge_{shape}_{bs}_K{K}_shift{shift}_{name(dt)}_NW{waves(nv, 1)}", x, 1.5, shape, bs, shift)


# ---- 8. above the LDS limit -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,m", [(C64, 98), (F32, 139)], ids=["98x98-complex64", "139x139-float32"])
def test_refusal_above_the_lds_limit(rls, ctx, dt, m):
    assert lds_bytes(dt, m, m) > LDS_LIMIT >= lds_bytes(dt, m - 1, m - 1)
    x = gauss(np.random.default_rng(m), m * m, dt).astype(dt)
    xd = rls.DeviceVector.from_host(x, ctx)
    with pytest.raises(rls.RLSError, match="LDS"):
        rls.prox_(rls.NuclearRegularization(0.5, svtShape=(m, m)), xd)
    assert np.array_equal(xd.to_host(), x)
