"""Queue mode of the resident CGNR kernel (solvers.hip cgnr_queue_*, normal.hip cgnr_resident_kernel SPEC, resident_sync.hpp
resident_listen_q): back-to-back rls_cgnr_init + rls_cgnr_step calls post commands to one launch that keeps A in its registers.
The results must be those of the same calls with rls_tune_set("resident_queue", 0) (one launch per solve), within rounding."""
import ctypes as C
import os
import re
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

M, N, ITS = 4096, 2048, 32


def _problem(M, N, seed):
    rng = np.random.default_rng(seed)
    A = np.asfortranarray(((rng.standard_normal((M, N)) + 1j * rng.standard_normal((M, N))) / np.sqrt(2 * M)).astype(np.complex64))
    return A, rng


def _cgnr64(A, b, n):
    A = A.astype(np.complex128)
    x = np.zeros(A.shape[1], np.complex128)
    r = A.conj().T @ b.astype(np.complex128)
    p = r.copy()
    rr = np.vdot(r, r).real
    for _ in range(n):
        t = A @ p
        alpha = rr / np.vdot(t, t).real
        x += alpha * p
        r -= alpha * (A.conj().T @ t)
        rr_new = np.vdot(r, r).real
        p = r + (rr_new / rr) * p
        rr = rr_new
    return x


class _Run:
    """one solver on one operator; `solve(b)` = rls_cgnr_init + rls_cgnr_step(ITS) with no host wait"""

    def __init__(self, rls, ctx, A, its=ITS, rel_tol=0.0):
        self.rls, self.ctx, self.its = rls, ctx, its
        self.Ad = rls.DeviceMatrix.from_host(A, ctx)
        self.S = rls.createLinearSolver(rls.CGNR, self.Ad, iterations=its, relTol=rel_tol)
        self.lib, self.h = ctx.lib, ctx.handle

    def solve(self, bd):
        self.rls.init_(self.S, bd)
        self.rls._lib.check(self.h, self.lib.rls_cgnr_step(self.S.state._plan, self.its), "rls_cgnr_step")

    def status(self):
        st = self.rls._lib.CgnrStatus()
        self.rls._lib.check(self.h, self.lib.rls_cgnr_get_status(self.S.state._plan, C.byref(st)), "rls_cgnr_get_status")
        return st

    def x(self):
        return self.S.state.x.to_host()


def _bs(rls, ctx, A, rng, k):
    xs = [((rng.standard_normal(A.shape[1]) + 1j * rng.standard_normal(A.shape[1])) / np.sqrt(2)).astype(np.complex64) for _ in range(k)]
    bh = [(A @ x).astype(np.complex64) for x in xs]
    return bh, [rls.DeviceVector.from_host(b, ctx) for b in bh]


def _sequence(rls, ctx, A, bds, queue, checkpoints=(), **kw):
    """solves bds in order; returns {index: x} at the checkpoints (a read-back there ends the kernel) and the last x"""
    ctx.tune(resident_queue=queue)
    try:
        R = _Run(rls, ctx, A, **kw)
        out = {}
        for k, bd in enumerate(bds):
            R.solve(bd)
            if k in checkpoints:
                out[k] = R.x()
        out[len(bds) - 1] = R.x()
        return out, R
    finally:
        ctx.tune(resident_queue=1)


def _rel(a, b):
    return float(np.linalg.norm(a.astype(np.complex128) - b) / np.linalg.norm(b))


@pytest.mark.gpu
def test_back_to_back_solves_match_oracle_and_reproduce(rls, ctx):
    A, rng = _problem(M, N, 11)
    bh, bds = _bs(rls, ctx, A, rng, 100)
    R0 = _Run(rls, ctx, A)
    path = C.c_int32(-1)
    rls.init_(R0.S, bds[0])
    ctx.lib.rls_cgnr_path(R0.S.state._plan, C.byref(path))
    if path.value != 4:
        pytest.skip(f"not on the resident path ({path.value})")
    checks = (0, 1, 2, 17, 50)
    got, _ = _sequence(rls, ctx, A, bds, 1, checks)
    ref, _ = _sequence(rls, ctx, A, bds, 0, checks)
    for k in got:
        e = _rel(got[k], _cgnr64(A, bh[k], ITS))
        assert e < 1e-5, (k, e)
        assert _rel(got[k], ref[k].astype(np.complex128)) < 1e-5, k
    # uninterrupted: 100 solves, only the last one read back
    got2, _ = _sequence(rls, ctx, A, bds, 1)
    assert _rel(got2[99], _cgnr64(A, bh[99], ITS)) < 1e-5
    got3, _ = _sequence(rls, ctx, A, bds, 1)
    assert np.array_equal(got2[99], got3[99]), "queue mode is not bit-reproducible"


@pytest.mark.gpu
def test_reltol_stop_inside_a_queued_solve(rls, ctx):
    A, rng = _problem(M, N, 12)
    bh, bds = _bs(rls, ctx, A, rng, 6)
    res = {}
    for q in (1, 0):
        got, R = _sequence(rls, ctx, A, bds, q, rel_tol=0.2)
        st = R.status()
        res[q] = (got[5], st.iteration, st.done)
    assert res[1][2] and res[1][1] < ITS, res[1][1:]
    assert res[1][1] == res[0][1]
    assert _rel(res[1][0], res[0][0].astype(np.complex128)) < 1e-5


@pytest.mark.gpu
def test_status_idle_exit_and_relaunch(rls, ctx):
    A, rng = _problem(M, N, 13)
    bh, bds = _bs(rls, ctx, A, rng, 8)
    R = _Run(rls, ctx, A)
    for k in range(3):
        R.solve(bds[k])
    st = R.status()  # ends the kernel and sees solve 2's state
    assert st.iteration == ITS and st.fallbacks == 0
    assert _rel(R.x(), _cgnr64(A, bh[2], ITS)) < 1e-5
    for k in range(3, 6):
        R.solve(bds[k])
    time.sleep(0.02)  # beyond the idle time: the kernel has left on its own
    for k in range(6, 8):
        R.solve(bds[k])  # posted to a kernel that is gone: re-issued by a fresh launch
    assert _rel(R.x(), _cgnr64(A, bh[7], ITS)) < 1e-5
    assert R.status().fallbacks == 0


@pytest.mark.gpu
def test_life_cap_reissues_the_rest(rls, ctx):
    """~250 us per solve and a life of 20 ms: 160 solves span several lives; what a life left in the ring runs in the next"""
    A, rng = _problem(M, N, 14)
    bh, bds = _bs(rls, ctx, A, rng, 8)
    seq = [bds[k % 8] for k in range(160)]
    got, _ = _sequence(rls, ctx, A, seq, 1, checkpoints=(120,))
    ref, _ = _sequence(rls, ctx, A, seq, 0, checkpoints=(120,))
    for k in got:
        assert _rel(got[k], _cgnr64(A, bh[k % 8], ITS)) < 1e-5
        assert _rel(got[k], ref[k].astype(np.complex128)) < 1e-5


@pytest.mark.gpu
def test_destroy_and_other_plan_while_listening(rls, ctx):
    A, rng = _problem(M, N, 15)
    bh, bds = _bs(rls, ctx, A, rng, 4)
    R1, R2 = _Run(rls, ctx, A), _Run(rls, ctx, A)
    for k in range(3):
        R1.solve(bds[k])
    R2.solve(bds[3])  # another plan: the listening kernel of R1 is told to leave first
    assert _rel(R1.x(), _cgnr64(A, bh[2], ITS)) < 1e-5
    assert _rel(R2.x(), _cgnr64(A, bh[3], ITS)) < 1e-5
    for k in range(3):
        R1.solve(bds[k])
    ctx.lib.rls_cgnr_destroy(R1.S.state._plan)  # while listening
    R1.S.state._plan = None
    for k in range(3):
        R2.solve(bds[k])
    ctx.sync()
    assert _rel(R2.x(), _cgnr64(A, bh[2], ITS)) < 1e-5


@pytest.mark.gpu
def test_ragged_shape_back_to_back(rls, ctx):
    A, rng = _problem(4000, 2000, 16)
    bh, bds = _bs(rls, ctx, A, rng, 5)
    got, _ = _sequence(rls, ctx, A, bds, 1)
    ref, _ = _sequence(rls, ctx, A, bds, 0)
    assert _rel(got[4], _cgnr64(A, bh[4], ITS)) < 1e-5
    assert np.array_equal(got[4], ref[4])  # (no queue mode for ragged shapes: the same launches)


def test_queue_instantiations_use_no_scratch():
    """the listening (SPEC) instantiations carry queue mode's init!; none of them may spill"""
    import kernel_metadata

    if not os.path.exists(kernel_metadata.LIB):
        pytest.skip("library not built")
    ks = kernel_metadata.kernels()
    spec = [k for k in ks if re.fullmatch(r"cgnr_resident_kernel<(c32|float), \d, \d+, 8, \d, true, true>", k)]
    assert len(spec) >= 4, spec
    assert all(ks[k]["scratch"] == 0 and ks[k]["vgprs"] <= 256 for k in spec), {k: ks[k] for k in spec}
