"""CPU tests of the one-launch Kaczmarz surface: rls_kaczmarz_solve[_d] are declared, exported and bound with the header's
argument lists; the classifier that decides which regularisers run inside the sweep kernel; the rule that splits a table of
per-sweep row orders into launches (the vl hazard of include/rls_mi355x.h)."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rls_mi355x.h")
ENTRY_POINTS = ("rls_kaczmarz_solve", "rls_kaczmarz_solve_d")


def test_entry_points_declared_exported_and_bound(rls):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", rls.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (rls_[a-z0-9_]+)", out))
    from rls_amd import _lib

    for name in ENTRY_POINTS:
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, text)
        assert m, f"{name} is not declared"
        assert name in exported, name
        assert name in _lib.PROTOTYPES, name
        nargs = len(m.group(1).split(","))
        assert nargs == 22 and len(_lib.PROTOTYPES[name][1]) == nargs, (name, nargs)
    # the sweep entries keep their 18 arguments
    for name in ("rls_kaczmarz_sweep", "rls_kaczmarz_sweep_d"):
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, text)
        assert len(m.group(1).split(",")) == 18 == len(_lib.PROTOTYPES[name][1]), name
    assert rls.load().rls_abi_version() == 2


def test_null_context_is_invalid(rls):
    lib = rls.load()
    z = [None, 1, 4, 4, None, 4, 1, None, 4, None, 4, None, 4, None, None, 1, 0, 0.0, 1, 0, 0, 0.0]
    assert lib.rls_kaczmarz_solve(*z) == -1
    assert lib.rls_kaczmarz_solve_d(*z) == -1


def test_classifier(rls):
    from rls_amd import solvers
    from rls_amd._lib import PROJ_NONE, PROJ_POSITIVE, PROJ_REAL, REG_L1, REG_L2, REG_NONE

    f = solvers._kaczmarz_fused_kinds
    Real, Pos, L1, L2 = rls.RealRegularization, rls.PositiveRegularization, rls.L1Regularization, rls.L2Regularization
    assert f([]) == (PROJ_NONE, REG_NONE, 0.0)
    assert f([Real()]) == (PROJ_REAL, REG_NONE, 0.0)
    assert f([Real(), Pos()]) == (PROJ_POSITIVE, REG_NONE, 0.0)
    assert f([Pos(), Real()]) == (PROJ_POSITIVE, REG_NONE, 0.0)
    assert f([Pos(), L1(0.25)]) == (PROJ_POSITIVE, REG_L1, 0.25)
    assert f([L2(0.5)]) == (PROJ_NONE, REG_L2, 0.5)
    assert f([rls.MaskedRegularization(L1(0.25), np.array([True, False]))]) is None
    assert f([rls.L21Regularization(0.25, slices=2)]) is None
    assert f([Pos(), rls.L21Regularization(0.25, slices=2)]) is None
    assert f([L1(0.25), L1(0.5)]) is None                 # one parameterised term
    assert f([L1(-1.0)]) is None
    assert f([L2(np.array([1.0, 2.0], np.float32))]) is None   # a vector lambda


def test_launch_splits(rls):
    from rls_amd import solvers

    split = solvers._kaczmarz_launch_splits
    nused, n = 18, 4
    clean = np.stack([np.arange(nused) + 100 * s for s in range(n)])        # no row comes back at all
    assert split(clean.reshape(-1), nused, n) == [(0, n)]
    t = clean.copy()
    t[2, 0] = t[1, -1]                                                         # sweep 1 ends in the row sweep 2 starts with
    assert split(t.reshape(-1), nused, n) == [(0, 2), (2, 2)]
    t = clean.copy()
    t[1, 2] = t[0, -2]                                                         # second to last -> third: 4 steps apart
    assert split(t.reshape(-1), nused, n) == [(0, 1), (1, 3)]
    t = clean.copy()
    t[1, 3] = t[0, -2]                                                         # 5 steps apart: beyond the pipeline
    t[3, 4] = t[2, -1]
    assert split(t.reshape(-1), nused, n) == [(0, n)]
    t = clean.copy()
    t[1, 0], t[2, 1], t[3, 3] = t[0, -1], t[1, -3], t[2, -1]                   # every boundary
    assert split(t.reshape(-1), nused, n) == [(0, 1), (1, 1), (2, 1), (3, 1)]
    # a real sample without replacement per sweep recurs across boundaries sooner or later: the pieces cover every sweep once
    rng = np.random.default_rng(3)
    t = np.stack([rng.choice(24, size=nused, replace=False) for _ in range(40)])
    parts = split(t.reshape(-1), nused, 40)
    assert [p[0] for p in parts] == list(np.cumsum([0] + [p[1] for p in parts[:-1]])) and sum(p[1] for p in parts) == 40
    assert 1 < len(parts) < 40
    for first, cnt in parts:       # inside a piece no row recurs within 4 steps
        flat = t[first:first + cnt].reshape(-1)
        assert all(flat[i] not in flat[i + 1:i + 5] for i in range(len(flat)))
    # sweeps of at most 16 rows: one launch each, whatever the table (None: one repeated order)
    small = np.stack([np.arange(16) + 100 * s for s in range(3)])
    assert split(small.reshape(-1), 16, 3) == [(0, 1), (1, 1), (2, 1)]
    assert split(None, 11, 3) == [(0, 1), (1, 1), (2, 1)]
    assert split(None, 17, 3) == [(0, 3)]
    assert split(clean.reshape(-1), nused, 0) == []
