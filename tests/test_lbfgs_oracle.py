"""CPU checks of the projected L-BFGS reference loop (lbfgs_oracle.py), no GPU needed: the coefficient-space two-loop
recursion against the textbook one on vectors, and the condition the loop was added for -- on the drift problem at
13 x 13 nodes and 20 steps, seven iterations with a memory of 5 end below half the cost of plain projected gradient at
the same number of sweeps, with and without active bounds."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lbfgs_oracle as lo


@pytest.mark.parametrize("masked", [False, True])
def test_coefficient_two_loop_equals_vector_two_loop(masked):
    """random fields on 5 x 5 cells and 4 levels, four pairs of which two fail G[s, y] > 0 (one the newest), and four
    pairs that all pass; 1e-12 relative in the Q norm"""
    from oracle.mesh import SquareMesh
    from oracle.assembly import P1Assembler
    M = P1Assembler(SquareMesh(-1, 1, 5)).mass()
    Nt, dt, k = 3, 0.1, 4
    tl = (Nt + 1) * M.shape[0]
    rng = np.random.default_rng(11)
    mask = rng.random(tl) > 0.3 if masked else None
    chi = (lambda f: np.where(mask, f, 0.0)) if masked else (lambda f: f)
    inner = lambda a, b: lo.q_inner(chi(a), chi(b), Nt, dt, M)
    for fail in ((1, 3), ()):
        S = [rng.standard_normal(tl) for _ in range(k)]
        Y = [s + 0.5 * rng.standard_normal(tl) for s in S]
        for i in range(k):
            if (inner(S[i], Y[i]) > 0) == (i in fail):
                Y[i] = -Y[i]
        g = rng.standard_normal(tl)
        G = lo.q_gram(S + Y + [g], mask, Nt, dt, M)
        assert [G[i, k + i] > 0 for i in range(k)] == [i not in fail for i in range(k)]
        r, took = lo.two_loop_coefficients(G, k)
        assert took == k - len(fail)
        Hg = lo.combine([chi(f) for f in S + Y + [g]], r, None, None, 0.0)
        ref = lo.two_loop_vectors([chi(s) for s in S], [chi(y) for y in Y], chi(g), inner)
        err = Hg - ref
        assert lo.q_inner(err, err, Nt, dt, M) <= 1e-24 * lo.q_inner(ref, ref, Nt, dt, M)
        if not fail:                        # every pair took part: H is positive definite on the free set
            assert r @ G[:, -1] > 0


def _runs(name):
    cs = lo.solidbody_case(*lo.CONFIGS[name])
    return lo.run_solidbody(cs, 7, 0)[3], lo.run_solidbody(cs, 7, 5)[3]


def test_memory_5_halves_the_cost_of_projected_gradient_on_configuration_A():
    """beta = 1e-3, bounds [0, 5], all-time (measured: 1.417e-3 against 3.856e-4, ratio 0.27)"""
    h0, h5 = _runs("A")
    assert len(h0["cost"]) == len(h5["cost"]) == 7 and h0["sweeps"][-1] == h5["sweeps"][-1] == 15
    assert h5["cost"][-1] < 0.5 * h0["cost"][-1], (h5["cost"], h0["cost"])
    assert h5["used"][0] == "g" and set(h5["used"][1:]) == {"qn"} and set(h0["used"]) == {"g"}
    assert not h0["stalled"] and not h5["stalled"]


def test_memory_5_halves_the_cost_with_active_bounds_on_configuration_B():
    """beta = 1e-4, bounds [0, 2.5] (measured: 1.034e-3 against 8.52e-5, ratio 0.08; 3-6 % of the control bound from
    iteration 2 on, iterations counted from 0)"""
    h0, h5 = _runs("B")
    assert len(h0["cost"]) == len(h5["cost"]) == 7 and h0["sweeps"][-1] == h5["sweeps"][-1] == 15
    assert h5["cost"][-1] < 0.5 * h0["cost"][-1], (h5["cost"], h0["cost"])
    assert all(1.0 - f > 0 for f in h5["free_fraction"][2:]), h5["free_fraction"]


def test_costs_never_increase_and_rejections_are_searched():
    """the final-time variant of A: its sixth iteration accepts the third trial"""
    h = lo.run_solidbody(lo.solidbody_case(*lo.CONFIGS["A-finaltime"]), 6, 5)[3]
    assert h["armijo_k"] == [1, 1, 1, 1, 1, 3] and [len(m) for m in h["armijo_margin"]] == h["armijo_k"]
    costs = [h["cost0"]] + h["cost"]
    assert all(b <= a for a, b in zip(costs, costs[1:]))
    assert h["sweeps"] == [3, 5, 7, 9, 11, 15]


def test_source_control_memory_5_is_below_projected_gradient_after_5_iterations():
    cs = lo.source_case()
    h0, h5 = lo.run_source(cs, 5, 0)[3], lo.run_source(cs, 5, 5)[3]
    assert len(h0["cost"]) == len(h5["cost"]) == 5
    assert h5["cost"][-1] < h0["cost"][-1], (h5["cost"], h0["cost"])
    assert h5["armijo_margin_min"] > 1e-7 and h0["armijo_margin_min"] > 1e-7
