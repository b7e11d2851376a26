"""The state machine of init_(): one solver object walks batched -> vector -> batched (same K) -> batched (other K) ->
per-column -> vector, and after every step its state has the expected type, still carries the scalars the solver was created
with, and the result has the bits of a fresh solver that performs only that one solve.

Shapes: 128 x 48 for every solver (ADMM Float32, the others ComplexF32) -- batched CGNR and FISTA take this shape, as
batched ADMM and OptISTA / POGM do in test_gpu_plan_lifecycle.  Every path here is fixed-order, so equal means equal bits.

POGM's init! does not reset gamma (test_gpu_pgm_batched.test_callbacks_and_reuse): only its first step can equal a fresh
solver's.  From the second step on the gamma it starts from must be the one column 0 ended the previous step with."""
import numpy as np
import pytest

import rls_oracle as O

pytestmark = pytest.mark.gpu

M, N, ITERS = 128, 48, 6
SOLVERS = ["CGNR", "FISTA", "ADMM", "OptISTA", "POGM"]
ADMM_TOLS = {"absTol": 1e-12, "relTol": 0.0, "tolInner": 1e-6}

# (right-hand side, scheduler) of every step: columns of B[:, :k] for a matrix, the column index for a vector
STEPS = [(("cols", 3), "BatchedState"), (("col", 1), None), (("cols", 3), "BatchedState"), (("cols", 2), "BatchedState"),
         (("cols", 4), "MultiThreadingState"), (("col", 0), None)]
BATCHED = {"CGNR": None, "FISTA": "FistaBatchedState", "ADMM": "AdmmBatchedState", "OptISTA": "PgmBatchedState",
           "POGM": "PgmBatchedState"}
PLAIN = {"CGNR": "CGNRState", "FISTA": "FISTAState", "ADMM": "ADMMState", "OptISTA": "_ProxGradState", "POGM": "_ProxGradState"}


class Problem:
    def __init__(self, rls, ctx, name):
        self.rls, self.ctx, self.name = rls, ctx, name
        dt = np.float32 if name == "ADMM" else np.complex64
        A, _, B = O.make_problem(M, N, dt, 29, n_rhs=4)
        self.B = np.asfortranarray(B * np.array([1.0, 3.0, 0.5, 2.0], dtype=B.real.dtype)[None, :])
        self.rho = 0.3 if name == "ADMM" else float(0.9 / np.linalg.norm(A.astype(np.complex128), 2) ** 2)
        self.Ad = rls.DeviceMatrix.from_host(A, ctx)

    def solver(self):
        rls, name = self.rls, self.name
        if name == "CGNR":
            return rls.createLinearSolver(rls.CGNR, self.Ad, reg=rls.L2Regularization(1e-3), iterations=ITERS, relTol=0.0)
        if name == "ADMM":
            return rls.createLinearSolver(rls.ADMM, self.Ad, reg=rls.L1Regularization(0.05), rho=self.rho, iterations=ITERS,
                                          iterationsCG=4, **ADMM_TOLS)
        return rls.createLinearSolver(getattr(rls, name), self.Ad, reg=rls.L1Regularization(1e-2), rho=self.rho,
                                      iterations=ITERS, relTol=0.0)

    def rhs(self, what):
        kind, k = what
        if kind == "col":
            return self.rls.DeviceVector.from_host(np.ascontiguousarray(self.B[:, k]), self.ctx)
        return self.rls.DeviceMatrix.from_host(np.asfortranarray(self.B[:, :k]), self.ctx)

    def solve(self, S, what, scheduler, **kw):
        if scheduler is not None:
            kw["scheduler"] = getattr(self.rls, scheduler)
        out = self.rls.solve_(S, self.rhs(what), **kw)
        return np.stack([x.to_host() for x in out], axis=1) if isinstance(out, list) else out.to_host()


def check_state(rls, name, S, scheduler, prob):
    """the type of S.state and the scalars it (or each of its per-column states) carries"""
    st = S.state
    tname = type(st).__name__
    if scheduler == "BatchedState":
        assert isinstance(st, rls.BatchedState)
        if BATCHED[name] is None:  # CGNR's own plan: the scheduler token or a subclass of its own, none of the siblings'
            assert tname.endswith("BatchedState")
            assert not isinstance(st, (rls.FistaBatchedState, rls.PgmBatchedState, rls.AdmmBatchedState))
        else:
            assert tname == BATCHED[name]
        holders = [st]
    elif scheduler == "MultiThreadingState":
        assert tname == "MultiThreadingState"
        assert len(st.states) == 4 and all(type(s).__name__ == PLAIN[name] for s in st.states)
        holders = st.states
    else:
        assert tname == PLAIN[name]
        holders = [st]
    for h in holders:
        if name == "ADMM":
            for k, v in ADMM_TOLS.items():
                assert getattr(h, k) == np.float32(v), (k, getattr(h, k))
            assert np.all(np.asarray(h.rho) == np.float32(prob.rho))
        else:
            assert h.relTol == 0.0
            if name != "CGNR":
                assert h.rho == prob.rho


def gamma_of_column0(st):
    if hasattr(st, "status"):
        return float(st.status()[0].gamma)
    return float((st.states[0] if hasattr(st, "states") else st).gamma)


@pytest.mark.parametrize("name", SOLVERS)
def test_one_solver_through_every_scheduler(rls, ctx, name):
    prob = Problem(rls, ctx, name)
    fresh = {}
    for what, scheduler in STEPS[:1] if name == "POGM" else STEPS:
        if (what, scheduler) not in fresh:
            fresh[what, scheduler] = prob.solve(prob.solver(), what, scheduler)
    S = prob.solver()
    seen = []
    for step, (what, scheduler) in enumerate(STEPS, 1):
        if name == "POGM" and step > 1:
            want_gamma = gamma_of_column0(S.state)
            at_init = []
            x = prob.solve(S, what, scheduler, callbacks=lambda s, it: at_init.append(gamma_of_column0(s.state)) if it == 0 else None)
            assert at_init == [want_gamma], (step, at_init, want_gamma)
            assert np.all(np.isfinite(x))
        else:
            x = prob.solve(S, what, scheduler)
            assert np.array_equal(x, fresh[what, scheduler]), (step, float(np.max(np.abs(x - fresh[what, scheduler]))))
        check_state(rls, name, S, scheduler, prob)
        seen.append(S.state)
    # every init_ that ends on a shared-A plan here builds a new batched state: the vector solve in between has put a plain
    # state in its place, and the last one changes K
    assert seen[2] is not seen[0]
    assert seen[3] is not seen[2] and seen[3] is not seen[0]
    assert seen[3].K == 2


def test_admm_keeps_its_batched_state_while_k_stays(rls, ctx):
    """two matrix solves in a row: ADMM takes its batched state (plan and state matrices) over when K is the same"""
    prob = Problem(rls, ctx, "ADMM")
    want = prob.solve(prob.solver(), ("cols", 3), "BatchedState")
    S = prob.solver()
    prob.solve(S, ("cols", 3), "BatchedState")
    first = S.state
    assert np.array_equal(prob.solve(S, ("cols", 3), "BatchedState"), want)
    assert S.state is first
    prob.solve(S, ("cols", 2), "BatchedState")
    assert S.state is not first and S.state.K == 2
    check_state(rls, "ADMM", S, "BatchedState", prob)


@pytest.mark.parametrize("name", ["FISTA", "ADMM", "OptISTA", "POGM"])
def test_device_start_vector_takes_the_per_column_path(rls, ctx, name):
    """a warm start is outside the shared-A plans: BatchedState falls back to MultiThreadingState (the values:
    test_gpu_warm_start)"""
    prob = Problem(rls, ctx, name)
    g = np.linspace(0.5, 1.5, N).astype(prob.B.dtype)
    S = prob.solver()
    x = prob.solve(S, ("cols", 3), "BatchedState", x0=rls.DeviceVector.from_host(g, ctx))
    assert type(S.state).__name__ == "MultiThreadingState"
    assert len(S.state.states) == 3
    assert np.all(np.isfinite(x))
