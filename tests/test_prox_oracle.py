"""CPU checks of the proximal-gradient reference loop for L1-sparse controls (prox_oracle.py), no GPU needed: with
alpha = 0 it is the projected-gradient loop of lbfgs_oracle.py exactly, accepted costs never increase and iterates stay in
the box, a larger alpha gives a sparser control, and the scalar prox is the minimiser it claims to be."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lbfgs_oracle as lo
import prox_oracle as po


def test_alpha_zero_is_projected_gradient_exactly():
    """configuration B (active bounds), four iterations: the iterates, costs and armijo_k of lbfgs_loop(memory=0)"""
    cs = lo.solidbody_case(*lo.CONFIGS["B"])
    u, p, c, h = po.run_solidbody(cs, 4, 0.0)
    uo, po_, co, ho = lo.run_solidbody(cs, 4, 0)
    assert h["armijo_k"] == ho["armijo_k"] and h["sweeps"] == ho["sweeps"] and len(h["cost"]) == 4
    assert np.array_equal(np.array(h["cost"]), np.array(ho["cost"])) and h["cost0"] == ho["cost0"]
    assert np.array_equal(c, co) and np.array_equal(u, uo) and np.array_equal(p, po_)
    assert h["l1"][-1] > 0 and h["cost_smooth"] == h["cost"]


@functools.lru_cache(maxsize=None)
def _drift_run(alpha):
    cs = po.drift_case()
    return cs, po.run_solidbody(cs, po.DRIFT_ITERS, alpha, s0=po.DRIFT_S0)


@pytest.mark.parametrize("alpha", [1e-4, 5e-4])
def test_drift_case_descends_inside_the_box_with_the_recorded_decisions(alpha):
    """13 x 13 nodes, 20 steps, s0 = 256, 8 iterations: Armijo halvings are taken, both bounds and both signs occur, and
    every Armijo decision is at least 9.0e-3 (alpha = 1e-4) / 1.4e-2 (5e-4) relative from its threshold"""
    cs, (u, p, c, h) = _drift_run(alpha)
    assert h["armijo_k"] == po.DRIFT_ARMIJO_K[alpha] and not h["stalled"]
    assert [len(m) for m in h["armijo_margin"]] == h["armijo_k"] and h["armijo_margin_min"] > 5e-3
    costs = [h["cost0"]] + h["cost"]
    assert all(b <= a for a, b in zip(costs, costs[1:]))
    assert c.min() >= cs["lo"] and c.max() <= cs["hi"]
    assert np.any(c == cs["lo"]) and np.any(c == cs["hi"]) and np.any((c < 0) & (c > cs["lo"])) and np.any(c > 0)
    assert np.allclose(h["cost"], np.array(h["cost_smooth"]) + alpha * np.array(h["l1"]), rtol=1e-15, atol=0)
    assert h["nonzero_fraction"][-1] == np.mean(c != 0)
    assert h["sweeps"] == list(1 + np.cumsum(1 + np.array(h["armijo_k"])))
    assert all(r > 0 for r in h["residual"])


def test_larger_alpha_gives_a_sparser_drift_control():
    """final nonzero fraction 0.952 (alpha = 0), 0.320 (1e-4), 0.194 (5e-4)"""
    cs = po.drift_case()
    f0 = po.run_solidbody(cs, po.DRIFT_ITERS, 0.0, s0=po.DRIFT_S0)[3]["nonzero_fraction"][-1]
    f1, f2 = (_drift_run(a)[1][3]["nonzero_fraction"][-1] for a in (1e-4, 5e-4))
    print(f0, f1, f2)
    assert f0 > f1 > f2 > 0
    assert abs(f1 - 0.320) < 1e-3 and abs(f2 - 0.194) < 1e-3


@pytest.mark.parametrize("run", sorted(po.SOURCE_RUNS))
def test_source_case_takes_the_recorded_decisions(run):
    """n = 49, 18 steps, box [-0.1, 0.5]: alpha = 1e-2 ends at F = 5.4184e-3 with 14 % of the values at -0.1, 34 % at 0.5
    and 52 % nonzero (min margin 1.1e-4); alpha = 3e-3 has min margin 5.2e-4"""
    alpha, s0, iters = run
    cs = po.source_case()
    assert (cs["n"], cs["Nt"]) == (49, 18) and abs(cs["dt"] - 1 / 36) < 1e-15
    u, p, c, h = po.run_source(cs, iters, alpha, s0)
    assert h["armijo_k"] == po.SOURCE_RUNS[run] and not h["stalled"]
    assert h["armijo_margin_min"] > 1e-4
    costs = [h["cost0"]] + h["cost"]
    assert all(b <= a for a, b in zip(costs, costs[1:]))
    assert c.min() >= cs["lo"] and c.max() <= cs["hi"]
    if alpha == 1e-2:
        assert abs(h["cost"][-1] - 5.4184e-3) < 1e-7
        assert abs(np.mean(c == -0.1) - 0.14) < 0.01 and abs(np.mean(c == 0.5) - 0.34) < 0.01
        assert abs(np.mean(c != 0) - 0.52) < 0.01


def test_a_search_without_an_acceptable_trial_stalls_and_keeps_the_control():
    """one trial of step 1e6 per iteration: the first jumps to a bang-bang control with a lower cost, the next finds
    nothing; started from that control the loop stalls at once and returns it unchanged"""
    cs = po.source_case()
    u, p, c, h = po.run_source(cs, 3, 1e-2, 1e6, max_armijo=1)
    assert h["stalled"] and h["iterations"] == 1 and h["cost"][0] < h["cost0"]
    u2, p2, c2, h2 = po.run_source(dict(cs, c0=c), 3, 1e-2, 1e6, max_armijo=1)
    assert h2["stalled"] and h2["iterations"] == 0 and h2["cost"] == [] and h2["armijo_margin_min"] is None
    assert np.array_equal(c2, c) and np.array_equal(u2, u) and h2["cost0"] == h["cost"][0]


def test_scalar_prox_is_the_minimiser_of_its_problem():
    """prox(x) against the brute-force minimiser of tau |z| + (z - x)^2 / 2 over [lo, hi]: the candidates are the bounds,
    zero (if inside) and the stationary points x -+ tau of the two smooth branches; x on a grid that includes +-tau; boxes
    around zero, with lo > 0 and with hi < 0"""
    for lo_, hi_ in ((-0.1, 0.5), (0.2, 1.0), (-1.0, -0.2), (0.0, 0.0), (-0.3, 0.0)):
        for tau in (0.0, 1e-3, 0.25, 0.7):
            x = np.concatenate([np.linspace(-2, 2, 81), [tau, -tau, lo_, hi_, lo_ + tau, hi_ + tau, lo_ - tau, hi_ - tau,
                                                        np.nextafter(tau, 1), np.nextafter(-tau, -1), 0.0, -0.0]])
            got = po.prox(x, tau, lo_, hi_)
            obj = lambda z, xx: tau * np.abs(z) + 0.5 * (z - xx) ** 2
            for xi, gi in zip(x, got):
                cand = np.clip(np.array([lo_, hi_, 0.0, xi - tau, xi + tau]), lo_, hi_)
                grid = np.linspace(lo_, hi_, 2001)
                best = min(obj(cand, xi).min(), obj(grid, xi).min())
                assert lo_ <= gi <= hi_
                assert obj(gi, xi) <= best + 1e-15, (lo_, hi_, tau, xi, gi)
            assert np.array_equal(po.prox(np.array([tau, -tau]), tau, -5.0, 5.0), np.zeros(2))
    assert np.array_equal(po.prox(np.array([0.3, -0.3, 2.0]), 0.0, -1.0, 1.0), np.array([0.3, -0.3, 1.0]))
