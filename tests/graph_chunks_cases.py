"""The sweeps of tests/test_gpu_graph_chunks.py and their inputs (NumPy only: checked by tests/test_graph_chunks_cases.py).

A trajectory sweep is enqueued as captured graphs of FEMFCT_STEPS_PER_GRAPH time steps (femfct_run_sweep, traj_common.h):
a graph is replayed at successive starting levels and a shorter one finishes the ragged tail.  That is right only if every
level-dependent operand is resolved on the device from the level counter, nothing level-dependent is decided on the host
while a graph is captured, and the fused step ends log at the ordinal the counters give.  The GPU test runs every sweep
below, NT = 7 steps, cut into graphs in every way of CHUNKINGS, and asks for the bits and the solver logs of eager
stepping.

CASES: one entry per sweep variant with the C entry point it calls; together they cover every ``femfct_*_(forward|adjoint)*``
name of ``_lib.SIGNATURES`` (the CPU test fails for an entry point added later without a case).  ``entry_call`` = "raw":
the Python wrapper of this entry point goes through a more general one (solidbody_forward -> _src, schnak_forward /
schnak_adjoint -> _tw), so the GPU test calls the C function itself.

``inputs(case, N, B)``: the host arrays of a case in VERTEX order, deterministic per (case, member):

  * every level-indexed input differs at every level: controls, sources, the reaction coefficient g, states, targets, wind
    factors, and the non-zero entries of theta and sigma (no sweep entry point takes interval starts: the control intervals
    act on whole trajectories outside the sweeps, femfct_time_restrict / femfct_time_prolong)
  * the members of a batch differ from each other
  * theta and sigma are WEIGHTS["A"] (non-zero exactly at the levels 0, 3, 4 and NT) or WEIGHTS["B"] (zero exactly
    there), scaled by dt below NT.  Every pair of levels that a graph boundary of CHUNKINGS separates, forward or backward,
    holds one of those four levels: with A the step next to the boundary loads a misfit / penalty, with B it skips the load
  * a target holds NaN at every level its weights do not observe (tests/test_gpu_snapshots.py: _member)
"""
import zlib
from collections import namedtuple

import numpy as np

NT = 7
# FEMFCT_STEPS_PER_GRAPH -> the graphs of a 7-step sweep
CHUNKINGS = {50: (7,), 3: (3, 3, 1), 4: (4, 3), 1: (1,) * 7}
BOUNDARY_LEVELS = (0, 3, 4, NT)
WEIGHTS = {"A": np.array([0.6, 0.0, 0.0, 1.1, 0.8, 0.0, 0.0, 1.3]),
           "B": np.array([0.0, 0.9, 0.5, 0.0, 0.0, 1.2, 0.7, 0.0])}
OM = np.pi / 40
GROWTH = (0.3, 1.0, -1.0)
GAMMA = 50.0                        # penalty weight of the state bounds
BOUNDS = (0.1, 0.6)                 # lower, upper: the solid-body / linear states leave them on both sides

Case = namedtuple("Case", "id entry family sweep opts entry_call")


def _case(id, entry, family, sweep, entry_call="wrapper", **opts):
    return Case(id, "femfct_" + entry, family, sweep, opts, entry_call)


def _solidbody():
    out = []
    for eps, tag in ((0.0, "eps0"), (1e-3, "eps1e-3")):
        out += [
            _case(f"sb-fwd-{tag}", "solidbody_forward", "solidbody", "forward", "raw", eps=eps),
            _case(f"sb-fwd-src-{tag}", "solidbody_forward_src", "solidbody", "forward", eps=eps, src=True),
            _case(f"sb-adj-finaltime-{tag}", "solidbody_adjoint", "solidbody", "adjoint", eps=eps, mode="finaltime"),
            _case(f"sb-adj-alltime-{tag}", "solidbody_adjoint", "solidbody", "adjoint", eps=eps, mode="alltime"),
        ]
    out += [
        _case("sb-fwd-c-shared", "solidbody_forward_src", "solidbody", "forward", eps=0.0, c_shared=True),
        _case("sb-adj-snapshots", "solidbody_adjoint_obs", "solidbody", "adjoint", eps=0.0, mode="snapshots", theta="A"),
        _case("sb-adj-snapshots-window", "solidbody_adjoint_obs", "solidbody", "adjoint", eps=1e-3, mode="snapshots",
              theta="B", window=True),
        _case("sb-adj-bounds", "solidbody_adjoint_bounds", "solidbody", "adjoint", eps=0.0, mode="bounds", theta="B",
              sigma="A"),
        _case("sb-adj-bounds-windows", "solidbody_adjoint_bounds", "solidbody", "adjoint", eps=1e-3, mode="bounds",
              theta="A", sigma="B", window=True, window_s=True, c_shared=True),
    ]
    return out


def _linear():
    out = []
    # without g: the solid-body entry points with the shared zero drift control and a source (LinearSourceControl)
    for g, tag, fwd, adj in ((False, "lin", "solidbody_forward_src", "solidbody_adjoint"),
                             (True, "linreact", "linear_forward_react", "linear_adjoint_react")):
        out += [
            _case(f"{tag}-fwd", fwd, "linear", "forward", g=g, src=True),
            _case(f"{tag}-adj-finaltime", adj, "linear", "adjoint", g=g, mode="finaltime"),
            _case(f"{tag}-adj-alltime", adj, "linear", "adjoint", g=g, mode="alltime"),
            _case(f"{tag}-adj-snapshots", adj + "_obs", "linear", "adjoint", g=g, mode="snapshots", theta="A" if g else "B"),
            _case(f"{tag}-adj-bounds", adj + "_bounds", "linear", "adjoint", g=g, mode="bounds", theta="A", sigma="B",
                  window_s=g),
        ]
    return out


def _nonlinear():
    return [
        _case("nl-fwd", "nonlinear_forward", "nonlinear", "forward"),
        _case("nl-fwd-ct", "nonlinear_forward_ct", "nonlinear", "forward", ct=True),
        _case("nl-adj-finaltime", "nonlinear_adjoint", "nonlinear", "adjoint", mode="finaltime"),
        _case("nl-adj-alltime", "nonlinear_adjoint_alltime", "nonlinear", "adjoint", mode="alltime"),
        _case("nl-adj-snapshots", "nonlinear_adjoint_obs", "nonlinear", "adjoint", mode="snapshots", theta="B"),
        _case("nl-adj-snapshots-window", "nonlinear_adjoint_obs", "nonlinear", "adjoint", mode="snapshots", theta="A",
              window=True),
    ]


def _schnak():
    return [
        _case("sk-fwd", "schnak_forward", "schnak", "forward", "raw"),
        _case("sk-fwd-wind", "schnak_forward_tw", "schnak", "forward", wind=True),
        _case("sk-fwd-ct", "schnak_forward_ct", "schnak", "forward", ct=True),
        _case("sk-fwd-ct-wind", "schnak_forward_ct", "schnak", "forward", ct=True, wind=True),
        _case("sk-adj-finaltime", "schnak_adjoint", "schnak", "adjoint", "raw", mode="finaltime"),
        _case("sk-adj-alltime", "schnak_adjoint", "schnak", "adjoint", "raw", mode="alltime"),
        _case("sk-adj-finaltime-wind", "schnak_adjoint_tw", "schnak", "adjoint", mode="finaltime", wind=True),
        _case("sk-adj-alltime-wind", "schnak_adjoint_tw", "schnak", "adjoint", mode="alltime", wind=True),
        _case("sk-adj-snapshots", "schnak_adjoint_obs", "schnak", "adjoint", mode="snapshots", theta="A", theta_v="B"),
        _case("sk-adj-snapshots-wind", "schnak_adjoint_obs", "schnak", "adjoint", mode="snapshots", theta="B", theta_v="A",
              wind=True, window=True),
    ]


def _chtxs():
    return [
        _case("cx-fwd", "chtxs_forward", "chtxs", "forward"),
        _case("cx-fwd-growth", "chtxs_forward_g", "chtxs", "forward", growth=True),
        _case("cx-fwd-ct", "chtxs_forward_ct", "chtxs", "forward", ct=True),
        _case("cx-fwd-ct-growth", "chtxs_forward_g", "chtxs", "forward", ct=True, growth=True),
        _case("cx-adj-finaltime", "chtxs_adjoint", "chtxs", "adjoint", mode="finaltime"),
        _case("cx-adj-alltime", "chtxs_adjoint", "chtxs", "adjoint", mode="alltime"),
        _case("cx-adj-finaltime-growth", "chtxs_adjoint_g", "chtxs", "adjoint", mode="finaltime", growth=True),
        _case("cx-adj-alltime-growth", "chtxs_adjoint_g", "chtxs", "adjoint", mode="alltime", growth=True),
        _case("cx-adj-snapshots", "chtxs_adjoint_obs", "chtxs", "adjoint", mode="snapshots", theta="A", theta_v="B"),
        _case("cx-adj-snapshots-growth", "chtxs_adjoint_obs", "chtxs", "adjoint", mode="snapshots", theta="B", theta_v="A",
              growth=True, window=True, misfit="nodal"),
    ]


CASES = _solidbody() + _linear() + _nonlinear() + _schnak() + _chtxs()
BY_ID = {c.id: c for c in CASES}
SPECIES = ("schnak", "chtxs")       # families whose step has a species (non-FCT) solve with a log of its own

# the domain and the time step of a family on a mesh of N nodes per side
DOMAIN = {"solidbody": (-1.0, 1.0), "linear": (0.0, 1.0), "nonlinear": (0.0, 1.0), "schnak": (0.0, 1.0), "chtxs": (0.0, 1.0)}


def time_step(family, N):
    return {"solidbody": 1e-3 * 80 / (N - 1), "linear": (1.0 / (N - 1)) ** 2, "nonlinear": 1e-3, "schnak": 5e-4,
            "chtxs": 5e-4}[family]


def linear_wind(x, y, gamma=0.1):
    """solvers.finaltime_exact_wind() (kept here: this module needs no built library)"""
    return gamma * np.sin(np.pi * x) * np.cos(np.pi * x), gamma * np.sin(np.pi * y) * np.cos(np.pi * y)


def wind_factors(dt):
    """s(t_0) .. s(t_NT) of the separable Schnakenberg wind: different at every level, both signs"""
    return 1.5 * np.cos(0.9 * np.arange(NT + 1) + 0.4 + 40.0 * dt) - 0.25


def weights(name, dt):
    """(level weights as the sweeps take them, terminal weight): WEIGHTS[name] * dt below NT, the terminal one as it is"""
    w = WEIGHTS[name] * dt
    w[NT] = WEIGHTS[name][NT]
    return w, float(w[NT])


def graph_boundaries(chunks, sweep):
    """the pairs (last level one graph produces, first level the next one produces) of a sweep of sum(chunks) steps"""
    Nt = sum(chunks)
    produced = list(range(1, Nt + 1)) if sweep == "forward" else list(range(Nt - 1, -1, -1))
    ends = np.cumsum(chunks)[:-1]
    return [(produced[e - 1], produced[e]) for e in ends]


def _coords(family, N):
    a1, a2 = DOMAIN[family]
    iy, ix = np.divmod(np.arange(N * N), N)
    h = (a2 - a1) / (N - 1)
    return a1 + ix * h, a1 + iy * h


def _rng(case, member, N):
    return np.random.default_rng([zlib.crc32(case.id.encode()), member, N])


def _traj(x, y, rng, m, base, amp, noise, move=0.0):
    """(NT + 1, n): a smooth field that changes with the level (and the member) + per-level noise"""
    lv = np.arange(NT + 1)[:, None]
    k = rng.uniform(1.0, 3.0, 2)
    smooth = np.sin(k[0] * np.pi * (x - move * lv) + 0.3 + 0.37 * lv + 0.5 * m) * np.cos(k[1] * np.pi * y - 0.2 * lv)
    return base + amp * smooth + noise * rng.random((NT + 1, x.size))


def _target(u, rng, w, tau, scale, noise):
    """a target trajectory next to the state ``u`` (NT + 1, n), NaN at the levels that (w, tau) do not observe"""
    t = scale * u + noise * rng.random(u.shape)
    seen = w != 0
    seen[NT] = tau != 0
    t[~seen] = np.nan
    return t


def _window(x, y, family):
    mid = 0.5 * sum(DOMAIN[family])
    return np.where(x > mid, 0.5 + (x - mid) * (1 + 0.5 * np.sin(3 * y)), 0.0)


def inputs(case, N, B):
    """dict of the host arrays of ``case`` on an N x N mesh for B members, vertex order; per-member arrays are (B, ...),
    trajectories (B, NT + 1, n).  Keys: see the families below; "level_indexed": the names of the per-level arrays,
    "dt", "outputs": the names of the trajectories the sweep writes."""
    fam, o, n = case.family, case.opts, N * N
    x, y = _coords(fam, N)
    dt = time_step(fam, N)
    rngs = [_rng(case, m, N) for m in range(B)]
    d = dict(dt=dt, level_indexed=[])
    stack = lambda f: np.stack([f(m, rngs[m]) for m in range(B)])

    def put(name, arr, per_level=True):
        d[name] = arr
        if per_level:
            d["level_indexed"].append(name)

    # ---- states: the level-0 field of a forward sweep, a whole trajectory for an adjoint sweep (it takes any)
    if fam in ("solidbody", "linear"):
        cx, cy = (-0.3, 0.2) if fam == "solidbody" else (0.4, 0.6)
        wd = 10.0 if fam == "solidbody" else 40.0

        def state(m, r):
            t = np.arange(NT + 1)[:, None] * dt
            return (np.exp(-wd * ((x - cx - 3 * t) ** 2 + (y - cy + 0.1 * (m + 1) * t) ** 2)) * (1 + 0.1 * m)
                    + 0.05 * r.random((NT + 1, n)))
        states = {"u": stack(state)}
    elif fam == "nonlinear":
        states = {"u": stack(lambda m, r: _traj(x, y, r, m, 0.0, 0.3, 0.05) * (16 * x * (1 - x) * y * (1 - y)))}
    elif fam == "schnak":
        states = {"u": stack(lambda m, r: _traj(x, y, r, m, 1.0, 0.1, 0.02)),
                  "v": stack(lambda m, r: _traj(x, y, r, m + 3, 0.9, 0.1, 0.02))}
    else:
        states = {"u": stack(lambda m, r: _traj(x, y, r, m, 1.5, 0.04, 0.02)),
                  "v": stack(lambda m, r: _traj(x, y, r, m + 3, 1.5, 0.04, 0.02))}

    # ---- controls and coefficients
    if fam == "solidbody":
        if o.get("c_shared"):
            put("c", 2.0 * _rng(case, 99, N).random((1, NT + 1, n)))
        else:
            put("c", stack(lambda m, r: 2.0 * r.random((NT + 1, n))))
    elif fam == "linear":
        if o.get("g"):
            lv = np.arange(NT + 1)[:, None]
            put("g", -55.0 + 45.0 * np.sin(3 * x + 0.7 * lv) * np.cos(2 * y - 0.3 * lv))
    elif fam == "nonlinear":
        put("c", stack(lambda m, r: r.random((NT + 1, n))))
    elif fam == "schnak":
        put("c", stack(lambda m, r: 0.1 + 0.05 * r.random((NT + 1, n))))
        if o.get("wind"):
            put("wind_scale", wind_factors(dt))
    else:
        put("c", stack(lambda m, r: 20.0 * r.random((NT + 1, n))))
    if o.get("src"):
        put("src", stack(lambda m, r: _traj(x, y, r, m + 7, 0.5, 1.0, 0.1)))

    if case.sweep == "forward":
        for k, s in states.items():
            put(k + "0", s[:, 0].copy(), per_level=False)
        d["outputs"] = sorted(states)
        return d

    # ---- adjoint sweeps: states, targets, weights
    for k, s in states.items():
        put(k, s)
    mode = o["mode"]
    if mode == "finaltime":
        for j, (k, s) in enumerate(states.items()):
            put(k + "hat", stack(lambda m, r: (0.9 + 0.15 * j) * s[m, NT] + 0.02 * r.random(n)), per_level=False)
    elif mode == "alltime":
        for j, (k, s) in enumerate(states.items()):
            put(k + "hat", stack(lambda m, r: (0.9 + 0.15 * j) * s[m] + 0.02 * r.random((NT + 1, n))))
    else:
        for j, (k, s) in enumerate(states.items()):
            w, tau = weights(o["theta"] if k == "u" else o["theta_v"], dt)
            put("theta_" + k, w, per_level=False)
            d["tau_" + k] = tau
            put(k + "hat", stack(lambda m, r: _target(s[m], r, w, tau, 0.8 + 0.3 * j, 0.02)))
        if o.get("window"):
            put("window", _window(x, y, fam), per_level=False)
    if mode == "bounds":
        put("sigma", weights(o["sigma"], dt)[0], per_level=False)
        put("lower", np.full(n, BOUNDS[0]), per_level=False)
        put("upper", BOUNDS[1] + 0.05 * np.sin(3 * x), per_level=False)
        if o.get("window_s"):
            put("window_s", 1.0 + 0.5 * np.cos(2 * x + y), per_level=False)
    d["outputs"] = ["p", "q"][:len(states)]
    # the terminal level of an output is non-zero where its own terminal condition is (final-time misfit, tau, sigma_NT)
    if mode == "finaltime":
        d["terminal"] = {k: True for k in d["outputs"]}
    elif mode == "alltime":
        d["terminal"] = {k: False for k in d["outputs"]}
    else:
        d["terminal"] = {"p": d["tau_u"] != 0 or (mode == "bounds" and d["sigma"][NT] != 0)}
        if "v" in states:
            d["terminal"]["q"] = d["tau_v"] != 0
    return d
