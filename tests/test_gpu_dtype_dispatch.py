"""Element-type dispatch of the C ABI (rls_with_elem, csrc/rls_common.hpp): the (entry point, element type) pairs that no other
test reaches, each against a float64 NumPy evaluation.  n = 1000 is no multiple of a workgroup size, so a swapped cast or grid
shows.  Every other exported function is reached with both of its element types by the tests of its own module."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 1000
TOL = 2e-6  # the bound tests/test_gpu_parity.py::test_tv_pieces_match_fused holds the same two entry points to (Float32)


def _rel(a, b):
    return np.linalg.norm(a.astype(np.complex128) - b.astype(np.complex128)) / np.linalg.norm(b.astype(np.complex128))


def _cvec(seed, scale):
    rng = np.random.default_rng(seed)
    return (scale * (rng.standard_normal(N) + 1j * rng.standard_normal(N)) / math.sqrt(2)).astype(np.complex64)


def test_tv_restrict_complex(rls, ctx):
    """q / max(1, |q|) (ProxTV.jl:135-139) on ComplexF32: magnitudes on both sides of 1"""
    q = _cvec(11, 1.5)
    assert (np.abs(q) > 1).any() and (np.abs(q) < 1).any()
    qd = rls.DeviceVector.from_host(q, ctx)
    rls._lib.check(ctx.handle, ctx.lib.rls_tv_restrict(ctx.handle, rls._lib.C32, N, qd.ptr), "tv_restrict")
    q64 = q.astype(np.complex128)
    assert _rel(qd.to_host(), q64 / np.maximum(1.0, np.abs(q64))) < TOL


def test_tv_lincomb_complex(rls, ctx):
    """rs = t3 * pq - t2 * pqOld on ComplexF32"""
    pq, pqo = _cvec(12, 1.0), _cvec(13, 1.0)
    t2, t3 = 0.625, 1.625
    rs = rls.DeviceVector(N, np.complex64).fill_(0)
    pqd, pqod = rls.DeviceVector.from_host(pq, ctx), rls.DeviceVector.from_host(pqo, ctx)
    rls._lib.check(ctx.handle, ctx.lib.rls_tv_lincomb(ctx.handle, rls._lib.C32, N, rs.ptr, t3, pqd.ptr, t2, pqod.ptr), "tv_lincomb")
    assert _rel(rs.to_host(), t3 * pq.astype(np.complex128) - t2 * pqo.astype(np.complex128)) < TOL
