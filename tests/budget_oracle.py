"""CPU reference of the control budget ||c||_{1,h} <= B in the proximal-gradient loops (``solvers.prox_solidbody`` and
``solvers.prox_source_control`` with ``budget=``), beside prox_oracle.py, whose loop, cases and prox it reuses.

With the weights omega_{l,i} = dt w_l ml_i of the nodal-quadrature norm, phi(theta) = sum omega |prox(x, theta, lo, hi)|
is continuous, piecewise linear and non-increasing in the total threshold theta, for lo <= 0 <= hi.  Its breakpoints are
|x| (the value leaves zero) and |x| - bound (the value leaves its bound; bound = hi for x > 0, -lo for x < 0).
``project`` finds the segment between neighbouring breakpoints on which phi crosses B by bisection over the sorted
breakpoints, and solves the affine piece there: exact up to rounding, no iteration on the threshold.

``budget_loop`` runs prox_oracle's loop with its trial replaced by the budget trial."""
import contextlib

import numpy as np

import lbfgs_oracle as lo
import prox_oracle as po


def omega(num_steps, dt, ml):
    """the weights dt w_l ml_i of ||.||_{1,h}, flat, level-major"""
    return (dt * lo.q_weights(num_steps)[:, None] * np.asarray(ml)[None, :]).ravel()


def phi(x, om, theta, lo_, hi_):
    return float(om @ np.abs(po.prox(x, theta, lo_, hi_)))


def project(x, om, tau, B, lo_, hi_):
    """(clip(soft_threshold(x, tau + lam)), lam): lam = 0.0 if phi(tau) <= B, else the root of phi(tau + lam) = B"""
    assert lo_ <= 0 <= hi_ and B > 0 and tau >= 0
    x = np.asarray(x, dtype=np.float64)
    if phi(x, om, tau, lo_, hi_) <= B:
        return po.prox(x, tau, lo_, hi_), 0.0
    z = np.abs(x)
    bound = np.where(x > 0, hi_, -lo_)
    live = bound > 0
    bp = np.concatenate([z[live], (z - bound)[live]])
    bp = np.unique(np.concatenate([[tau], bp[bp > tau]]))          # sorted; phi(bp[0]) > B >= phi(bp[-1]) = 0
    i, j = 0, len(bp) - 1
    while j - i > 1:
        m = (i + j) // 2
        if phi(x, om, bp[m], lo_, hi_) > B:
            i = m
        else:
            j = m
    a, b = bp[i], bp[j]
    mid = 0.5 * (a + b)                                            # no breakpoint inside (a, b): classes are those at mid
    fixed = live & (z - bound >= mid)
    linear = live & (z > mid) & ~fixed
    W = float(om[linear].sum())
    theta = (float(om[fixed] @ bound[fixed]) + float(om[linear] @ z[linear]) - B) / W
    theta = min(max(theta, a), b)
    lam = theta - tau
    return po.prox(x, tau + lam, lo_, hi_), lam


def trial(c, s, d, alpha, B, lo_, hi_, om):
    """the budget trial for step s and direction d: (c_t, lam_t, phi_t(tau_t))"""
    x, tau = c + s * d, s * alpha
    P, lam = project(x, om, tau, B, lo_, hi_)
    return P, lam, phi(x, om, tau, lo_, hi_)


@contextlib.contextmanager
def _budget_trial(om, B, log):
    """prox_oracle.prox_loop with its trial replaced: every call of prox_trial inside is the budget trial"""
    plain = po.prox_trial

    def prox_trial(c, s, d, alpha, lo_, hi_):
        P, lam = project(c + s * d, om, s * alpha, B, lo_, hi_)
        log.append(lam)
        return P

    po.prox_trial = prox_trial
    try:
        yield
    finally:
        po.prox_trial = plain


def _with_multipliers(result, log, B):
    """an iteration calls the trial once for the residual and armijo_k times for the search: the accepted trial is the last"""
    h, k, mult = result[3], 0, []
    for ak in h["armijo_k"]:
        k += 1 + ak
        mult.append(log[k - 1])
    h["multiplier"] = mult
    h["budget_used"] = [v / B for v in h["l1"]]
    return result


def run_solidbody(cs, iters, alpha, B, **kw):
    om, log = omega(cs["Nt"], cs["dt"], po.lumped_mass(cs["sb"].cm.M)), []
    with _budget_trial(om, B, log):
        return _with_multipliers(po.run_solidbody(cs, iters, alpha, **kw), log, B)


def run_source(cs, iters, alpha, s0, B, **kw):
    om, log = omega(cs["Nt"], cs["dt"], po.lumped_mass(cs["ls"].cm.M)), []
    with _budget_trial(om, B, log):
        return _with_multipliers(po.run_source(cs, iters, alpha, s0, **kw), log, B)


# (case, alpha, B) -> armijo_k of eight iterations (drift: s0 = 256; source: s0 = 1024)
DRIFT_RUNS = {(0.0, 0.2): [1, 3, 2, 3, 3, 3, 3, 4], (0.0, 0.1): [1, 1, 3, 3, 3, 4, 1, 2], (1e-4, 0.1): [1, 1, 3, 3, 3, 4, 1, 2]}
SOURCE_RUNS = {(0.0, 0.05): [1, 6, 4, 6, 3, 5, 5, 5]}
SOURCE_S0 = 1024.0
