"""CPU checks of the control-budget reference (budget_oracle.py), no GPU needed: the exact projection is the projection it
claims to be (variational inequality, idempotence, prox_oracle's bits when the budget is slack, the budget met when it
binds), the reference loop takes the recorded decisions on the four runs the GPU tests repeat, and the entry point is
declared and bound."""
import functools
import importlib
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import budget_oracle as bo
import prox_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOXES = [(-0.1, 0.5), (0.0, 1.0), (-1.0, 0.0), (-1e9, 1e9)]


def _values(rng, N):
    """values spread over four decades, a seventh of them tied, with +-0.0 and values far outside the three small boxes.
    (How far is limited by what a double can resolve: at the root theta the norm moves by W ulp(theta) per step of the
    threshold, W the weight of the values still linear, so |phi - B| / B cannot be asked below W theta eps / B.  With
    outliers of 1e12 that is 13 % at a budget of 1e-3 of phi(0); with 40 it is 3e-12 there and below 5e-15 at the larger
    shares -- figures of this file's cases.)"""
    x = rng.standard_normal(N) * 10.0 ** rng.uniform(-3, 1, N)
    x[::7] = 0.25 * np.sign(x[::7] + 1e-300)
    x[:4] = [0.0, -0.0, 40.0, -40.0]
    return x, rng.uniform(0.5, 2.0, N) / N


@pytest.mark.parametrize("box", BOXES)
def test_projection_properties(box):
    lo_, hi_ = box
    rng = np.random.default_rng(11)
    for N in (36, 1000, 20000):
        x, om = _values(rng, N)
        for tau in (0.0, 1e-3):
            phi0 = bo.phi(x, om, tau, lo_, hi_)
            for share in (0.9, 0.3, 1e-3):
                B = share * phi0
                P, lam = bo.project(x, om, tau, B, lo_, hi_)
                assert lam > 0 and P.min() >= lo_ and P.max() <= hi_
                got = float(om @ np.abs(P))
                assert abs(got - B) <= (1e-11 if share == 1e-3 else 1e-12) * B, (N, tau, share, got / B - 1)
                assert np.array_equal(P, po.prox(x, tau + lam, lo_, hi_))
                # idempotent: P lies in the set of its own norm, and a point of the set is its own projection
                P2, lam2 = bo.project(P, om, 0.0, max(B, got), lo_, hi_)
                assert lam2 == 0.0 and np.array_equal(P2, P)
                # and against the budget itself, which P meets to rounding: the second multiplier is of that size
                P3, lam3 = bo.project(P, om, 0.0, B, lo_, hi_)
                assert lam3 <= 1e-11 * (tau + lam) and np.abs(P3 - P).max() <= 1e-11 * (tau + lam)
                if tau == 0.0:
                    # the projection of x onto C_B in the omega inner product: <x - P, y - P> <= 0 for every feasible y
                    bar = 1e-12 * float(om @ (x * x))
                    for _ in range(20):
                        y = np.clip(rng.standard_normal(N) * 10.0 ** rng.uniform(-3, 1, N), lo_, hi_)
                        y[rng.random(N) < 0.5] = 0.0
                        ny = float(om @ np.abs(y))
                        if ny > B:
                            y *= B / ny * (1 - 1e-15)
                        assert float(om @ ((x - P) * (y - P))) <= bar
            # slack: lam = 0 and the plain prox's bits
            P, lam = bo.project(x, om, tau, phi0 * (1 + 1e-12), lo_, hi_)
            assert lam == 0.0 and np.array_equal(P, po.prox(x, tau, lo_, hi_))


def test_trial_is_prox_trial_when_slack():
    rng = np.random.default_rng(3)
    c, d = rng.uniform(-0.3, 0.6, 500), rng.standard_normal(500)
    om = rng.uniform(0.5, 2.0, 500)
    P, lam, phi0 = bo.trial(c, 0.5, d, 1e-3, 1e300, -0.1, 0.5, om)
    assert lam == 0.0 and np.array_equal(P, po.prox_trial(c, 0.5, d, 1e-3, -0.1, 0.5)) and phi0 == float(om @ np.abs(P))


@functools.lru_cache(maxsize=None)
def _drift(alpha, B):
    cs = po.drift_case()
    return cs, bo.run_solidbody(cs, po.DRIFT_ITERS, alpha, B, s0=po.DRIFT_S0)


@pytest.mark.parametrize("run", sorted(bo.DRIFT_RUNS))
def test_drift_runs_take_the_recorded_decisions(run):
    """B = 0.2, alpha = 0: the budget binds in iterations 1, 3, 5, 7, 8 and is slack (l1 0.194 .. 0.197) in 2, 4, 6, final
    nonzero fraction 0.367, smallest Armijo margin 2.3e-2; B = 0.1: always binding, 2.7e-3 (alpha = 0), 2.6e-3 (1e-4)"""
    alpha, B = run
    cs, (u, p, c, h) = _drift(alpha, B)
    print(h["armijo_k"], h["armijo_margin_min"], h["multiplier"], h["l1"], h["nonzero_fraction"][-1])
    assert h["armijo_k"] == bo.DRIFT_RUNS[run] and not h["stalled"]
    assert h["armijo_margin_min"] > {(0.0, 0.2): 2e-2, (0.0, 0.1): 2.5e-3, (1e-4, 0.1): 2.5e-3}[run]
    binding = [m > 0 for m in h["multiplier"]]
    if B == 0.2:
        assert binding == [True, False, True, False, True, False, True, True]
        assert all(0.1935 <= l <= 0.1975 for l, b in zip(h["l1"], binding) if not b)
        assert abs(h["nonzero_fraction"][-1] - 0.367) < 1e-3
    else:
        assert all(binding)
    assert all(abs(l - B) <= 1e-12 * B for l, b in zip(h["l1"], binding) if b)
    assert all(l <= B * (1 + 1e-12) for l in h["l1"])
    costs = [h["cost0"]] + h["cost"]
    assert all(b <= a for a, b in zip(costs, costs[1:]))
    assert c.min() >= cs["lo"] and c.max() <= cs["hi"]


def test_source_run_takes_the_recorded_decisions():
    """alpha = 0, B = 0.05, s0 = 1024: always binding, smallest Armijo margin 1.5e-5, final nonzero fraction 0.158"""
    cs = po.source_case()
    u, p, c, h = bo.run_source(cs, 8, 0.0, bo.SOURCE_S0, 0.05)
    print(h["armijo_k"], h["armijo_margin_min"], h["multiplier"], h["nonzero_fraction"][-1])
    assert h["armijo_k"] == bo.SOURCE_RUNS[(0.0, 0.05)] and not h["stalled"]
    assert h["armijo_margin_min"] > 1e-5 and all(m > 0 for m in h["multiplier"])
    assert all(abs(l - 0.05) <= 1e-12 * 0.05 for l in h["l1"])
    assert abs(h["nonzero_fraction"][-1] - 0.158) < 1e-3
    assert c.min() >= cs["lo"] and c.max() <= cs["hi"]


def test_a_huge_budget_is_the_plain_loop():
    cs = po.drift_case()
    a = po.run_solidbody(cs, 3, 1e-4, s0=po.DRIFT_S0)
    b = bo.run_solidbody(cs, 3, 1e-4, 1e300, s0=po.DRIFT_S0)
    assert np.array_equal(a[2], b[2]) and a[3]["cost"] == b[3]["cost"] and b[3]["multiplier"] == [0.0] * 3


def test_entry_point_is_declared_and_bound():
    _lib = importlib.import_module("fem-fct-pdeco_amd._lib")
    assert "femfct_budget_trials" in _lib.SIGNATURES
    restype, args = _lib.SIGNATURES["femfct_budget_trials"]
    assert len(args) == 17
    hdr = open(os.path.join(ROOT, "include", "femfct.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"int\s+femfct_budget_trials\s*\(([^)]*)\)", hdr)
    assert m and len(m.group(1).split(",")) == 17
    assert not re.search(r"_(forward|adjoint)", "femfct_budget_trials")
