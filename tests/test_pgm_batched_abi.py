"""CPU tests of the batched OptISTA / POGM surface: the C entry points are declared and exported under the same names, the
scheduler state is public, and the host-side coefficient table equals the per-iteration recurrences row for row."""
import os
import re
import subprocess
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rls_mi355x.h")
ENTRY_POINTS = ("rls_pgm_create_batched", "rls_pgm_destroy_batched", "rls_pgm_set_reg_batched", "rls_pgm_init_batched",
                "rls_pgm_step_batched", "rls_pgm_get_status_batched")


def test_entry_points_declared_and_exported(rls):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(rls_[a-z0-9_]+)\s*\(", text))
    out = subprocess.run(["nm", "-D", "--defined-only", rls.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (rls_[a-z0-9_]+)", out))
    from rls_amd import _lib

    for name in ENTRY_POINTS:
        assert name in declared, name
        assert name in exported, name
        assert name in _lib.PROTOTYPES, name
    # the status struct of the binding has the header's fields in the header's order
    m = re.search(r"typedef struct rls_pgm_status \{(.*?)\} rls_pgm_status;", text, flags=re.S)
    fields = [f.strip() for decl in re.findall(r"(?:int32_t|float)\s+([^;]+);", m.group(1)) for f in decl.split(",")]
    assert fields == [f for f, _ in _lib.PgmStatus._fields_]


def test_state_is_public_and_a_batched_state(rls):
    assert issubclass(rls.PgmBatchedState, rls.BatchedState)
    assert rls.PgmBatchedState is not rls.BatchedState


def _stub(rls, cls, iterations, rho, lam, **attrs):
    """a solver object without an operator: what the coefficient recurrences read"""
    from rls_amd import solvers

    s = cls.__new__(cls)
    s._op = types.SimpleNamespace(double=False)
    s.iterations = iterations
    s.reg = types.SimpleNamespace(lam=lam)
    names = ("x", "x0", "y", "z", "zold", "res") if cls is rls.OptISTA else ("x", "x0", "xold", "y", "z", "w", "res")
    s.state = solvers._ProxGradState(rho, 1, 1e-6, names)
    for k, v in attrs.items():
        setattr(s.state, k, v)
    return s


@pytest.mark.parametrize("iterations,theta", [(1, 1), (7, 1), (25, 1), (25, 2.5)])
def test_optista_table_equals_the_stepped_coefficients(rls, iterations, theta):
    from rls_amd import solvers

    f32 = np.float32
    rho, lam = 0.0123, 0.37
    S = _stub(rls, rls.OptISTA, iterations, rho, lam)
    table, hist = solvers._pgm_batched_table(S, theta)
    assert table.dtype == np.float32 and table.shape == (iterations, 8) and len(hist) == iterations + 1
    st = S._new_state()
    S._set_theta(st, theta)
    st.iteration = 0
    assert hist[0] == (st.theta, st.thetaold)
    for k in range(iterations):
        r, gamma, alpha, beta = S._coefficients(st)   # the iteration's scalars, as OptISTA.iterate forms them
        st.iteration += 1
        want = [r * gamma, r * gamma * f32(lam), f32(-1) / gamma, f32(1) / gamma, -beta, f32(1) + alpha + beta, -alpha, f32(0)]
        assert all(type(w) is np.float32 for w in want)
        assert np.array_equal(table[k], np.array(want, np.float32)), (k, table[k], want)
        assert hist[k + 1] == (st.theta, st.thetaold)


@pytest.mark.parametrize("iterations,theta,gamma0", [(1, 1, 1.0), (25, 1, 1.0), (25, 1, 0.0173), (9, 3.0, 1.0)])
def test_pogm_table_equals_the_stepped_coefficients(rls, iterations, theta, gamma0):
    from rls_amd import solvers

    rho, lam = 0.0123, 0.37
    S = _stub(rls, rls.POGM, iterations, rho, lam, gamma=gamma0, sigma=1.0, sigma_fac=1.0)
    S.restart = "none"
    table, hist = solvers._pgm_batched_table(S, theta)
    assert table.dtype == np.float32 and table.shape == (iterations, 8) and len(hist) == iterations + 1
    st = S._new_state()
    st.theta = st.thetaold = float(theta)
    st.iteration = 0
    assert st.gamma == gamma0 and hist[0] == (st.theta, st.thetaold, gamma0)
    for k in range(iterations):
        c_rho, c_y, c_x1, c_xo, c_z, thr = S._coefficients(st)   # the arguments of rls_pogm_update_async
        st.iteration += 1
        want = np.array([c_rho, thr, c_y, c_x1, c_xo, c_z, 0, 0], np.float32)
        assert np.array_equal(table[k], want), (k, table[k], want)
        assert hist[k + 1] == (st.theta, st.thetaold, st.gamma)
    assert S.state.gamma == gamma0  # building the table leaves the solver's own state alone
