"""The case table and the inputs of tests/test_gpu_graph_chunks.py (tests/graph_chunks_cases.py): no GPU needed."""
import importlib
import re

import numpy as np
import pytest

import graph_chunks_cases as gc
from graph_chunks_cases import NT

SWEEP_NAME = re.compile(r"_(forward|adjoint)")


def test_table_covers_every_sweep_entry_point():
    """Every femfct_*_(forward|adjoint)* name of the binding has a case: a sweep entry point added later without one
    fails here.  26 names today, femfct_solidbody_forward .. femfct_chtxs_adjoint_g."""
    _lib = importlib.import_module("fem-fct-pdeco_amd._lib")
    names = sorted(k for k in _lib.SIGNATURES if SWEEP_NAME.search(k))
    assert len(names) >= 26 and "femfct_solidbody_forward" in names and "femfct_chtxs_adjoint_g" in names
    covered = {c.entry for c in gc.CASES}
    assert sorted(covered - set(names)) == []
    assert sorted(set(names) - covered) == []
    for c in gc.CASES:
        assert ("_forward" in c.entry) == (c.sweep == "forward"), c.id
    assert len({c.id for c in gc.CASES}) == len(gc.CASES)


def test_table_has_the_modes_of_every_family():
    has = lambda fam, sweep, **kw: any(c.family == fam and c.sweep == sweep and all(c.opts.get(k) == v for k, v in kw.items())
                                       for c in gc.CASES)
    for eps in (0.0, 1e-3):
        assert has("solidbody", "forward", eps=eps) and has("solidbody", "forward", eps=eps, src=True)
        assert has("solidbody", "adjoint", eps=eps, mode="finaltime") and has("solidbody", "adjoint", eps=eps, mode="alltime")
    assert has("solidbody", "forward", c_shared=True)
    assert has("solidbody", "adjoint", mode="snapshots", window=True) and has("solidbody", "adjoint", mode="snapshots", window=None)
    assert has("solidbody", "adjoint", mode="bounds")
    for g in (False, True):
        assert has("linear", "forward", g=g)
        for mode in ("finaltime", "alltime", "snapshots", "bounds"):
            assert has("linear", "adjoint", g=g, mode=mode)
    assert has("nonlinear", "forward", ct=None) and has("nonlinear", "forward", ct=True)
    for mode in ("finaltime", "alltime", "snapshots"):
        assert has("nonlinear", "adjoint", mode=mode)
        for wind in (None, True):
            assert has("schnak", "adjoint", mode=mode, wind=wind)
        for growth in (None, True):
            assert has("chtxs", "adjoint", mode=mode, growth=growth)
    assert has("schnak", "forward", wind=None, ct=None) and has("schnak", "forward", wind=True) and has("schnak", "forward", ct=True)
    for growth in (None, True):
        assert has("chtxs", "forward", growth=growth, ct=None) and has("chtxs", "forward", growth=growth, ct=True)
    # both weight patterns reach theta and sigma
    for key in ("theta", "sigma"):
        assert {c.opts[key] for c in gc.CASES if key in c.opts} == {"A", "B"}


def test_weight_patterns_sit_on_the_graph_boundaries():
    A, B = gc.WEIGHTS["A"], gc.WEIGHTS["B"]
    assert A.size == B.size == NT + 1
    on = np.zeros(NT + 1, dtype=bool)
    on[list(gc.BOUNDARY_LEVELS)] = True
    assert gc.BOUNDARY_LEVELS == (0, 3, 4, NT)
    assert np.array_equal(A != 0, on) and np.array_equal(B != 0, ~on)
    for w in (A, B):                                    # no two weights equal
        nz = w[w != 0]
        assert len(set(nz)) == nz.size and np.all(nz > 0)
    assert gc.CHUNKINGS == {50: (7,), 3: (3, 3, 1), 4: (4, 3), 1: (1,) * 7}
    for per_graph, chunks in gc.CHUNKINGS.items():
        assert sum(chunks) == NT and all(c == min(per_graph, NT - k) for c, k in zip(chunks, np.cumsum((0,) + chunks)))
        for sweep in ("forward", "adjoint"):
            pairs = gc.graph_boundaries(chunks, sweep)
            assert len(pairs) == len(chunks) - 1
            if per_graph in (3, 4):
                # one side of every boundary is loaded with A and skipped with B, or the other way round
                assert all(on[a] or on[b] for a, b in pairs), (per_graph, sweep, pairs)
    assert gc.graph_boundaries((3, 3, 1), "forward") == [(3, 4), (6, 7)]
    assert gc.graph_boundaries((4, 3), "forward") == [(4, 5)]
    assert gc.graph_boundaries((3, 3, 1), "adjoint") == [(4, 3), (1, 0)]
    assert gc.graph_boundaries((4, 3), "adjoint") == [(3, 2)]
    dt = 2.5e-3
    for name in "AB":
        w, tau = gc.weights(name, dt)
        assert np.array_equal(w[:NT], gc.WEIGHTS[name][:NT] * dt) and tau == gc.WEIGHTS[name][NT] == w[NT]


def _levels(a, lead):
    """the NT + 1 levels of a level-indexed array, one row each (members kept apart: (lead, NT + 1, ...) -> rows)"""
    a = np.asarray(a)
    if a.shape[0] == NT + 1 and a.ndim <= 2:
        return [a.reshape(NT + 1, -1)]
    assert a.shape[:2] == (lead, NT + 1) or a.shape[:2] == (1, NT + 1), a.shape
    return [m.reshape(NT + 1, -1) for m in a]


@pytest.mark.parametrize("case", gc.CASES, ids=[c.id for c in gc.CASES])
def test_inputs_differ_at_every_level_and_member(case):
    N, B = 9, 3
    n = N * N
    d = gc.inputs(case, N, B)
    again = gc.inputs(case, N, B)
    for k, v in d.items():                              # deterministic per (case, member)
        if isinstance(v, np.ndarray):
            assert np.array_equal(v, again[k], equal_nan=True), k
    one = gc.inputs(case, N, 1)
    for k, v in d.items():
        if isinstance(v, np.ndarray) and v.ndim >= 2 and v.shape[0] == B:
            assert np.array_equal(v[:1], one[k], equal_nan=True), k
    assert d["dt"] == gc.time_step(case.family, N) > 0
    assert d["level_indexed"], case.id
    for name in d["level_indexed"]:
        for rows in _levels(d[name], B):
            seen = [r for r in rows if not np.isnan(r).all()]
            assert all(np.isfinite(r).all() for r in seen), name
            for i in range(len(seen)):
                for j in range(i + 1, len(seen)):
                    assert not np.array_equal(seen[i], seen[j]), (name, i, j)
    per_member = [k for k, v in d.items() if isinstance(v, np.ndarray) and v.ndim >= 2 and v.shape[0] == B and k != "g"]
    assert per_member
    for k in per_member:
        for a in range(B):
            for b in range(a + 1, B):
                assert not np.array_equal(d[k][a], d[k][b], equal_nan=True), (k, a, b)
    if case.sweep == "forward":
        assert all(d[k + "0"].shape == (B, n) for k in d["outputs"])
        return
    mode = case.opts["mode"]
    if mode in ("snapshots", "bounds"):
        for var in ("u", "v")[:len(d["outputs"])]:
            w, tau, hat = d["theta_" + var], d["tau_" + var], d[var + "hat"]
            name = case.opts["theta"] if var == "u" else case.opts["theta_v"]
            assert np.array_equal(w, gc.weights(name, d["dt"])[0]) and tau == w[NT]
            assert (w == 0).any() and (w != 0).any()
            for lv in range(NT + 1):                    # NaN exactly at the unobserved levels
                assert np.isnan(hat[:, lv]).all() == (w[lv] == 0), (var, lv)
                assert np.isnan(hat[:, lv]).any() == (w[lv] == 0), (var, lv)
    if mode == "bounds":
        s = d["sigma"]
        assert np.array_equal(s, gc.weights(case.opts["sigma"], d["dt"])[0]) and (s == 0).any() and (s != 0).any()
        u = d["u"]
        assert (u < d["lower"]).any() and (u > d["upper"]).any() and np.all(d["lower"] < d["upper"])
        for lv in np.flatnonzero(s):                    # every penalised level has violated nodes, in every member
            assert all(((u[m, lv] < d["lower"]) | (u[m, lv] > d["upper"])).any() for m in range(B))
    assert set(d["terminal"]) == set(d["outputs"])


def test_wind_factors_differ_at_every_level():
    for N in (21, 46):
        s = gc.wind_factors(gc.time_step("schnak", N))
        assert s.size == NT + 1 and (s > 0).any() and (s < 0).any() and np.all(np.abs(s) > 1e-2)
        assert np.abs(s[:, None] - s[None, :])[~np.eye(NT + 1, dtype=bool)].min() > 1e-2
