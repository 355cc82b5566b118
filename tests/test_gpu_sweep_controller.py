"""The sweep controller (femfct_run_sweep, csrc/traj_common.h) on its healthy path (-m gpu): budgets that grow, shrink and
recover, in every kernel regime, always against the CPU oracle and its direct spsolve.

Every trajectory sweep is enqueued whole with a remembered Jacobi budget per kind of sweep (48 sweeps to start with, a
fixed cap of 96 that doubles in the one-workgroup step, 40 iterations for the species solves); a step that ran out of
budget makes the controller grow the budget and repeat the whole sweep.  The inputs here need more than those budgets
(tests/jacobi_count.py counts the plain Jacobi sweeps of the oracle's own operator; tests/test_jacobi_count.py holds
every input to its window), so that every case goes through at least one repeat:

  A  the first sweep of a fresh context needs more than the starting budget; three runs, the last two identical bits
  B  the control ramps inside one sweep: early steps are cheap, late ones dear
  C  easy, hard, easy, hard controls on one context, forward and adjoint kinds interleaved
  D  one batch whose members need very different sweep counts, and one where only some members raise MMATRIX_ROWSUM
  E  a sweep cap between the easy and the hard count: NotConverged or a correct result, and the context recovers
  F  the species budget of the Schnakenberg and chemotaxis systems: every sweep at a base dt, then at 10 x dt

Regimes (asserted through ctx.kernel_regime unless a regime-moving tuning knob is set):

  rows      41 x 41, FEniCS order, set_fusion(False, False)      REGIME_ROWS
  strips    41 x 41, FEniCS order                                REGIME_STRIPS
  tile32    81 x 81, vertex order, B = 1                         REGIME_TILE32
  patch64   81 x 81, vertex order, B = 16                        REGIME_PATCH64
  mesh2x2   41 x 41, vertex order, B = 1 and B = 8               REGIME_MESH (2 x 2 blocks)
  mesh3x3   81 x 81, vertex order, B = 64                        REGIME_MESH (3 x 3 blocks)

The one-workgroup step sweeps Gauss-Seidel inside a thread's block and needs about as many sweeps as plain Jacobi or
fewer (0.7 x by DESIGN 4 (iii); 0.73 to 1.01 x on these inputs), so its easy inputs have a plain-Jacobi count under its
cap of 96 and its hard ones a count above 96 / 0.7 = 138: amplitudes 0 / 50 at 41 x 41 and dt = 1e-2 (89 and 150 / 202 plain sweeps), 0 / 40 at 81 x 81 and
dt = 4e-3 (84 and 153 / 154).  Its cap only doubles and never shrinks: in case C the first hard sweep of a kind doubles
it (two attempts), and every later sweep of that kind takes one attempt.

Tolerances are those of tests/test_gpu_systems_regimes.py: states < 1e-10, adjoints < 1e-9 relative l2 against the
oracle, every residual <= 1e-13, no SOLVER_BUDGET flag; a member against itself run alone < 1e-12 (bitwise where both
run the one-workgroup step); a sweep against the same sweep on a fresh context < 1e-11 (budgets differ).  "This path was
taken" is asserted on the device log, with the CPU count in the message.  The number of attempts a sweep took is read
off the FEMFCT_DEBUG lines on stderr and printed, never asserted; the same lines show a kind of sweep being handed to
BiCGStab, which no solid-body case but E may do: every input contracts under plain Jacobi within the cap of 400, so
BiCGStab would mean a budget that never took effect (a replayed graph with a stale budget ends there)."""
import importlib
import os

import numpy as np
import pytest

import jacobi_count as jc
from test_gpu_systems_regimes import REGIME_KNOBS

pytestmark = pytest.mark.gpu

STATE_TOL, ADJ_TOL, MEMBER_TOL, FRESH_TOL = 1e-10, 1e-9, 1e-12, 1e-11

# inputs per regime: mesh, order, batch, dt, the easy and the hard control amplitude and the starting budget they straddle
REGIMES = {
    "rows": dict(N=41, vertex=False, B=1, fusion=(False, False), regime="ROWS", dt=5e-3, win="N41", easy=0.0, hard=30.0,
                 start=jc.START_BUDGET),
    "strips": dict(N=41, vertex=False, B=1, fusion=None, regime="STRIPS", dt=5e-3, win="N41", easy=0.0, hard=30.0,
                   start=jc.START_BUDGET),
    "tile32": dict(N=81, vertex=True, B=1, fusion=None, regime="TILE32", dt=2.5e-3, win="N81", easy=0.0, hard=30.0,
                   start=jc.START_BUDGET),
    "patch64": dict(N=81, vertex=True, B=16, fusion=None, regime="PATCH64", dt=2.5e-3, win="N81", easy=0.0, hard=30.0,
                    start=jc.START_BUDGET),
    "mesh2x2-B1": dict(N=41, vertex=True, B=1, fusion=None, regime="MESH", dt=1e-2, win="N41-mesh", easy=0.0, hard=50.0,
                       start=jc.START_BUDGET_MESH),
    "mesh2x2-B8": dict(N=41, vertex=True, B=8, fusion=None, regime="MESH", dt=1e-2, win="N41-mesh", easy=0.0, hard=50.0,
                       start=jc.START_BUDGET_MESH),
    "mesh3x3": dict(N=81, vertex=True, B=64, fusion=None, regime="MESH", dt=4e-3, win="N81-mesh", easy=0.0, hard=40.0,
                    start=jc.START_BUDGET_MESH),
}
ALL = list(REGIMES)


@pytest.fixture(scope="module")
def hp():
    mod = importlib.import_module("fem-fct-pdeco_amd")
    mod.fct_helpers.VERBOSE = False
    return mod


@pytest.fixture(scope="module")
def solvers():
    return importlib.import_module("fem-fct-pdeco_amd.solvers")


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


_BUILD = []


def _report(hp, name, **figs):
    if not _BUILD:
        _BUILD.append(hp._lib.lib.femfct_build_id().decode())
        print(f"[controller] build {_BUILD[0]}")
    print(f"[controller] {name}: " + ", ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}"
                                               for k, v in figs.items()))


def _knobs_default():
    return not any(k in os.environ for k in REGIME_KNOBS)


class _Attempts:
    """Counts the attempts of the sweeps since the last take(): one FEMFCT_DEBUG line of femfct_run_sweep per attempt."""

    def __init__(self, monkeypatch, capfd):
        monkeypatch.setenv("FEMFCT_DEBUG", "1")
        self.capfd = capfd
        self.to_bicgstab = 0             # sweeps handed to BiCGStab so far ("... -> BiCGStab")

    def take(self):
        out, err = self.capfd.readouterr()
        print(out, end="")                                   # (the reports printed so far stay in the test's output)
        lines = [ln for ln in err.splitlines() if ln.startswith("[femfct] sweep kind")]
        self.to_bicgstab += sum(1 for ln in lines if ln.endswith("-> BiCGStab"))
        # an attempt ends in the budget line, or in the switch from pair-compact to full-row launches
        return sum(1 for ln in lines if " budget " in ln or "full-row Jacobi launches" in ln)

    def assert_jacobi_throughout(self):
        assert self.to_bicgstab == 0, f"{self.to_bicgstab} sweep(s) of contracting inputs were handed to BiCGStab"


# ----------------------------------------------------------------------------- the oracle, cached for the module
_ORACLE = {}


def _cached(key, fn):
    if key not in _ORACLE:
        _ORACLE[key] = fn()
    return _ORACLE[key]


def _o_forward(N, dt, amps, seed):
    """the oracle's forward trajectory (DoF order) of member ``seed`` under the control levels amps[k] * control_shape"""
    def f():
        mesh, _, sb = jc.solid_body(N)
        n, Nt = mesh.nodes, len(amps) - 1
        uo = np.zeros((Nt + 1) * n)
        uo[:n] = jc.state(mesh, seed)
        return otraj().solidbody_forward(sb, jc.control_traj(mesh, amps), uo, n, Nt, dt)
    return _cached((N, dt, tuple(amps), seed, "fwd"), f)


def _target(uo, seed):
    return 0.8 * uo + 0.01 * np.random.default_rng(1000 + seed).random(uo.size)


def _o_adjoint(N, dt, amps, seed):
    """the oracle's all-time adjoint of the oracle's own forward trajectory (the device gets that trajectory too)"""
    def f():
        mesh, _, sb = jc.solid_body(N)
        n, Nt = mesh.nodes, len(amps) - 1
        uo = _o_forward(N, dt, amps, seed)
        return otraj().solidbody_adjoint(sb, jc.control_traj(mesh, amps), uo, _target(uo, seed), np.zeros_like(uo), n, Nt,
                                         dt, optim="alltime")
    return _cached((N, dt, tuple(amps), seed, "adj"), f)


def otraj():
    from oracle import traj
    return traj


# ----------------------------------------------------------------------------- the device side
class _Run:
    """One SolidBodyDrift of a regime; host data in the oracle's DoF order, permuted at the boundary in vertex order."""

    def __init__(self, hp, solvers, cfg, Nt, dt=None, B=None):
        self.hp, self.cfg, self.Nt = hp, cfg, Nt
        self.N, self.dt, self.B = cfg["N"], cfg["dt"] if dt is None else dt, cfg["B"] if B is None else B
        self.mesh = jc.solid_body(self.N)[0]
        self.n = self.mesh.nodes
        self.tl = (Nt + 1) * self.n
        self.v2d = self.mesh.vertex_to_dof if cfg["vertex"] else np.arange(self.n)
        self.prob = solvers.SolidBodyDrift(hp.SquareMeshP1(-1.0, 1.0, self.N - 1), Nt, self.dt, batch=self.B,
                                           order=hp.ORDER_VERTEX if cfg["vertex"] else hp.ORDER_FENICS)
        self.ctx = self.prob.ctx
        if cfg["fusion"] is not None:
            self.ctx.set_fusion(*cfg["fusion"])

    def close(self):
        self.prob.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def assert_regime(self):
        if _knobs_default():
            assert self.ctx.kernel_regime(self.B) == getattr(self.hp._lib, "REGIME_" + self.cfg["regime"]), \
                (self.ctx.kernel_regime(self.B), self.cfg["regime"])

    def to_dev(self, a):
        return np.ascontiguousarray(np.asarray(a).reshape(-1, self.n)[:, self.v2d]).ravel()

    def from_dev(self, a, B):
        out = np.empty((a.size // self.n, self.n))
        out[:, self.v2d] = a.reshape(-1, self.n)
        return out.reshape(B, -1)

    def control(self, amps_per_member):
        return np.stack([jc.control_traj(self.mesh, a) for a in amps_per_member])

    def forward(self, c, seeds):
        """forward sweep of the members ``seeds`` with the controls c (B x tl, DoF order) -> (u (B x tl), log)"""
        B = len(seeds)
        init = np.zeros((B, self.tl))
        init[:, :self.n] = [jc.state(self.mesh, s) for s in seeds]
        d = [self.ctx.array(self.to_dev(c)), self.ctx.array(self.to_dev(init))]
        try:
            self.prob.forward(d[0], d[1], batch=B)
            return self.from_dev(d[1].download(), B), self.prob.solver_log(B)
        finally:
            for a in d:
                a.free()

    def adjoint(self, c, u, uhat):
        """all-time adjoint sweep -> (p (B x tl), log)"""
        B = len(u)
        d = [self.ctx.array(self.to_dev(x)) for x in (c, u, uhat)] + [self.ctx.zeros(B * self.tl)]
        try:
            self.prob.adjoint(d[0], d[1], d[2], d[3], "alltime", batch=B)
            return self.from_dev(d[3].download(), B), self.prob.solver_log(B)
        finally:
            for a in d:
                a.free()

    # -- a sweep of B members with their own control amplitudes, against the oracle
    def checked(self, kind, amps_per_member, seeds):
        """Runs the forward ("fwd") or adjoint ("adj") sweep; clean log; the members 0, B/2, B-1 (all for B <= 8) against
        the oracle.  Returns (result, log, worst error)."""
        N, dt, B = self.N, self.dt, len(seeds)
        c = self.control(amps_per_member)
        if kind == "fwd":
            got, log = self.forward(c, seeds)
        else:
            uo = np.stack([_o_forward(N, dt, a, s) for a, s in zip(amps_per_member, seeds)])
            got, log = self.adjoint(c, uo, np.stack([_target(u, s) for u, s in zip(uo, seeds)]))
        _clean(self.hp, log)
        err = 0.0
        for m in (range(B) if B <= 8 else sorted({0, B // 2, B - 1})):
            ref = (_o_forward if kind == "fwd" else _o_adjoint)(N, dt, amps_per_member[m], seeds[m])
            err = max(err, rel(got[m], ref))
        assert err < (STATE_TOL if kind == "fwd" else ADJ_TOL), (kind, err)
        return got, log, err


def _clean(hp, log):
    assert not np.any(log["flags"] & hp.FLAG_SOLVER_BUDGET), log["flags"]
    assert log["solver_resid"].max() <= 1e-13, log["solver_resid"].max()


def _cpu_counts(cfg, amp):
    N, dt, a, _ = jc.WINDOWS[(cfg["win"], amp)]
    r = jc.solid_body_counts(N, dt, a)
    return r["forward"][0], r["adjoint"][0]


def _took_a_repeat(cfg, log, amp, what):
    """precondition: some step needed more than the budget the first attempt had (relaxed under a regime-moving knob)"""
    worst = int(log["solver_iters"].max())
    if _knobs_default():
        assert worst > cfg["start"], (f"{what}: the device needed {worst} sweeps, not more than the starting budget "
                                      f"{cfg['start']}; plain Jacobi on the CPU needs {_cpu_counts(cfg, amp)} "
                                      f"(forward, adjoint) for amplitude {amp}")
    return worst


# ----------------------------------------------------------------------------- A
@pytest.mark.parametrize("rid", ALL)
def test_first_sweep_beyond_the_starting_budget_is_repeated(hp, solvers, monkeypatch, capfd, rid):
    """Case A.  A fresh context, a forward and an all-time adjoint sweep whose every step needs more Jacobi sweeps than
    the starting budget: the trajectory meets the oracle, the log is clean and shows more sweeps than the first attempt
    had.  Two more runs on the same context: the budget has settled, the third run has the bits of the second."""
    cfg = REGIMES[rid]
    B = cfg["B"]
    Nt = 3 if B >= 16 else 4
    amps, seeds = [(cfg["hard"],) * (Nt + 1)] * B, list(range(B))
    att = _Attempts(monkeypatch, capfd)
    with _Run(hp, solvers, cfg, Nt) as R:
        R.assert_regime()
        runs, figs = [], {}
        for rep in range(3):
            att.take()
            u, logf, eu = R.checked("fwd", amps, seeds)
            nf = att.take()
            p, loga, ep = R.checked("adj", amps, seeds)
            na = att.take()
            runs.append((u, p))
            figs.update({f"u{rep}": eu, f"p{rep}": ep, f"iters{rep}": (int(logf["solver_iters"].max()),
                                                                      int(loga["solver_iters"].max())),
                         f"attempts{rep}": (nf, na)})
            if rep == 0:
                _report(hp, f"A {rid} first run", **figs)
                _took_a_repeat(cfg, logf, cfg["hard"], "forward")
                _took_a_repeat(cfg, loga, cfg["hard"], "adjoint")
        _report(hp, f"A {rid}", cpu=_cpu_counts(cfg, cfg["hard"]), **figs)
        assert np.array_equal(runs[2][0], runs[1][0]) and np.array_equal(runs[2][1], runs[1][1])
        att.assert_jacobi_throughout()


# ----------------------------------------------------------------------------- B
@pytest.mark.parametrize("rid", ALL)
def test_load_that_varies_inside_one_sweep(hp, solvers, monkeypatch, capfd, rid):
    """Case B.  The control ramps from the easy amplitude at level 0 to the hard one at level Nt = 6 (81 x 81, dt = 2.5e-3:
    about 60 plain Jacobi sweeps for the first steps, 117 for the last): every level meets the oracle, and the log shows
    different sweep counts across the steps -- a budget sized from the first step alone would leave the last unconverged."""
    cfg = REGIMES[rid]
    B, Nt = cfg["B"], 6
    ramp = tuple(cfg["easy"] + (cfg["hard"] - cfg["easy"]) * k / Nt for k in range(Nt + 1))
    amps, seeds = [ramp] * B, list(range(B))
    att = _Attempts(monkeypatch, capfd)
    with _Run(hp, solvers, cfg, Nt) as R:
        R.assert_regime()
        att.take()
        u, logf, eu = R.checked("fwd", amps, seeds)
        nf = att.take()
        p, loga, ep = R.checked("adj", amps, seeds)
        na = att.take()
        itf, ita = logf["solver_iters"].max(axis=1), loga["solver_iters"].max(axis=1)
        _report(hp, f"B {rid}", u=eu, p=ep, iters_fwd=itf.tolist(), iters_adj=ita.tolist(), attempts=(nf, na),
                cpu_easy=_cpu_counts(cfg, cfg["easy"]), cpu_hard=_cpu_counts(cfg, cfg["hard"]))
        att.assert_jacobi_throughout()
        if _knobs_default():
            for it, what in ((itf, "forward"), (ita, "adjoint")):
                assert it.max() > it.min(), (what, it.tolist(), _cpu_counts(cfg, cfg["easy"]), _cpu_counts(cfg, cfg["hard"]))
                assert it.max() > cfg["start"], (what, it.tolist(), cfg["start"], _cpu_counts(cfg, cfg["hard"]))


# ----------------------------------------------------------------------------- C
@pytest.mark.parametrize("rid", ALL)
def test_easy_and_hard_controls_in_turn_on_one_context(hp, solvers, monkeypatch, capfd, rid):
    """Case C.  forward(easy), adjoint(easy), forward(hard), adjoint(hard), forward(easy), forward(hard), adjoint(easy) on
    one context: the budgets of the two kinds grow, shrink, try one launch fewer and fall back, and the graph cache
    holds several budgets per kind.  Every result meets the oracle with a clean log, and equals the same sweep on a
    fresh context to 1e-11 (not to the bit: the budgets differ).  No sweep ends on BiCGStab: a graph replayed with the
    budget of an earlier capture stays short whatever budget the controller asks for, until the controller gives the
    kind to BiCGStab -- which also meets the oracle, so only the solver that ran shows it."""
    cfg = REGIMES[rid]
    B = cfg["B"]
    Nt = 3 if B >= 16 else 4
    seeds = list(range(B))
    e, h = cfg["easy"], cfg["hard"]
    seq = [("fwd", e), ("adj", e), ("fwd", h), ("adj", h), ("fwd", e), ("fwd", h), ("adj", e)]
    att = _Attempts(monkeypatch, capfd)
    fresh = {}
    for kind, amp in dict.fromkeys(seq):
        with _Run(hp, solvers, cfg, Nt) as F:
            fresh[kind, amp] = F.checked(kind, [(amp,) * (Nt + 1)] * B, seeds)[0]
    with _Run(hp, solvers, cfg, Nt) as R:
        R.assert_regime()
        figs, hard_iters = {}, {}
        for i, (kind, amp) in enumerate(seq):
            att.take()
            got, log, err = R.checked(kind, [(amp,) * (Nt + 1)] * B, seeds)
            n_att = att.take()
            e_fresh = rel(got, fresh[kind, amp])
            figs[f"{i}:{kind}({amp:g})"] = f"err {err:.2e} fresh {e_fresh:.2e} iters {int(log['solver_iters'].max())} attempts {n_att}"
            if amp == h:
                hard_iters[kind] = log
            assert e_fresh < FRESH_TOL, (i, kind, amp, e_fresh)
        _report(hp, f"C {rid}", cpu_easy=_cpu_counts(cfg, e), cpu_hard=_cpu_counts(cfg, h), **figs)
        for kind, log in hard_iters.items():
            _took_a_repeat(cfg, log, h, kind)
        att.assert_jacobi_throughout()


# ----------------------------------------------------------------------------- D
D_CASES = [
    # regime, amplitudes, dt (None: the regime's), input window, precondition on the log:
    #   "repeat": the stiffest members needed more than the starting budget and more than the mildest ones
    #   "repeat-some": ... and the mildest members stayed under it (some members ran out of budget, others did not)
    pytest.param("patch64", (0.0, 3.0, 10.0, 30.0), None, "N81", "repeat", id="patch64"),
    pytest.param("patch64", (0.0, 3.0, 10.0), 1e-3, "N81-easy", None, id="patch64-mixed-flags"),
    pytest.param("mesh2x2-B8", (0.0, 50.0), None, "N41-mesh", "repeat-some", id="mesh2x2-B8-repeat"),
    pytest.param("mesh2x2-B8", (0.0, 3.0, 10.0, 30.0), 5e-3, "N41", None, id="mesh2x2-B8-under-cap"),
    pytest.param("mesh2x2-B8", (0.0, 3.0, 10.0), 2e-3, "N41-easy", None, id="mesh2x2-B8-mixed-flags"),
    pytest.param("mesh3x3", (0.0, 40.0), None, "N81-mesh", "repeat-some", id="mesh3x3-repeat"),
    pytest.param("mesh3x3", (0.0, 3.0, 10.0, 30.0), 2.5e-3, "N81", None, id="mesh3x3-under-cap"),
    pytest.param("mesh3x3", (0.0, 3.0, 10.0), 1e-3, "N81-easy", None, id="mesh3x3-mixed-flags"),
]


@pytest.mark.parametrize("rid, amp_set, dt, win, pre", D_CASES)
def test_batch_of_members_of_different_stiffness(hp, solvers, monkeypatch, capfd, rid, amp_set, dt, win, pre):
    """Case D.  One launch whose members carry the controls of amp_set in turn, each with its own initial noise (81 x 81,
    dt = 2.5e-3: 60 to 117 plain Jacobi sweeps): the members 0, B/2, B-1 (all for B <= 8) against the oracle, every
    member against itself run alone (1e-12; bitwise where both runs take the one-workgroup step, whose members share
    nothing), the stiffest members' sweep counts not below the mildest ones', and MMATRIX_ROWSUM on exactly the members
    whose operator has a row sum <= 0 on the CPU.  The mixed-flags batches (dt = 1e-3 at 81 x 81, 2e-3 at 41 x 41: only
    amplitude 0 passes the diagnostic) carry the flag on some members only.  In the "repeat" rows the sweep is repeated
    for the stiff members' sake; in the one-workgroup rows of that kind (amplitudes 0 and 50 / 40 in turn) the mild
    members converge under the cap of 96 in the very attempt in which the stiff ones run out of it.  The "under-cap"
    rows are the issue's inputs, which the one-workgroup step solves within its cap."""
    cfg = REGIMES[rid]
    B, N = cfg["B"], cfg["N"]
    dt = cfg["dt"] if dt is None else dt
    Nt = 3 if B >= 16 else 4
    seeds = list(range(B))
    member_amp = [amp_set[m % len(amp_set)] for m in range(B)]
    amps = [(a,) * (Nt + 1) for a in member_amp]
    cpu = {a: jc.solid_body_counts(*jc.WINDOWS[(win, a)][:3]) for a in amp_set}
    att = _Attempts(monkeypatch, capfd)
    figs = {}
    with _Run(hp, solvers, cfg, Nt, dt=dt) as R:
        R.assert_regime()
        knobs = _knobs_default()     # (before the run alone below sets a knob of its own)
        mesh_regime = R.ctx.kernel_regime(B) == hp._lib.REGIME_MESH
        att.take()
        u, logf, figs["u"] = R.checked("fwd", amps, seeds)
        nf = att.take()
        p, loga, figs["p"] = R.checked("adj", amps, seeds)
        figs["attempts"] = (nf, att.take())
    if N == 81:                      # the 3 x 3 one-workgroup step is chosen from 64 members on: have it run one alone
        monkeypatch.setenv("FEMFCT_MESH_STEP_BATCH_LARGE", "1" if mesh_regime else "1000000")
    with _Run(hp, solvers, cfg, Nt, dt=dt, B=1) as S:
        bitwise = mesh_regime and S.ctx.kernel_regime(1) == hp._lib.REGIME_MESH
        e_u = e_p = 0.0
        for m in range(B):
            u1, log0 = S.forward(S.control(amps[m:m + 1]), seeds[m:m + 1])
            _clean(hp, log0)
            uo = _o_forward(N, dt, amps[m], seeds[m])[None]
            p1, log1 = S.adjoint(S.control(amps[m:m + 1]), uo, _target(uo[0], seeds[m])[None])
            _clean(hp, log1)
            e_u, e_p = max(e_u, rel(u[m], u1[0])), max(e_p, rel(p[m], p1[0]))
            if bitwise:
                assert np.array_equal(u[m], u1[0]) and np.array_equal(p[m], p1[0]), m
        figs.update(u_vs_alone=e_u, p_vs_alone=e_p, bitwise=bitwise)
    for name, log, k in (("fwd", logf, "forward"), ("adj", loga, "adjoint")):
        it = log["solver_iters"].max(axis=0)                       # per member
        by_amp = {a: [int(it[m]) for m in range(B) if member_amp[m] == a] for a in amp_set}
        figs[f"iters_{name}"] = {a: (min(v), max(v)) for a, v in by_amp.items()}
        figs[f"cpu_{name}"] = {a: cpu[a][k][0] for a in amp_set}
        assert min(by_amp[amp_set[-1]]) >= max(by_amp[amp_set[0]]), (name, by_amp)
        if pre and knobs:
            msg = (f"{name}: device sweeps per amplitude {by_amp}, starting budget {cfg['start']}, plain Jacobi on the "
                   f"CPU {figs[f'cpu_{name}']}")
            assert min(by_amp[amp_set[-1]]) > cfg["start"] and min(by_amp[amp_set[-1]]) > max(by_amp[amp_set[0]]), msg
            if pre == "repeat-some":
                assert max(by_amp[amp_set[0]]) < cfg["start"], msg
        flagged = (log["flags"] & hp.FLAG_MMATRIX_ROWSUM) != 0     # steps x members
        want = np.array([not cpu[a][k][1] for a in member_amp])
        assert np.array_equal(flagged, np.broadcast_to(want, flagged.shape)), (name, flagged, want)
    figs["flagged_members"] = int(sum(not cpu[a]["forward"][1] for a in member_amp))
    att.take()                                                     # (the debug lines of the runs alone)
    att.assert_jacobi_throughout()
    _report(hp, f"D {rid} dt={dt:g}", **figs)
    assert e_u < MEMBER_TOL and e_p < MEMBER_TOL, (e_u, e_p)
    if "mixed" in win or win.endswith("easy"):
        assert 0 < figs["flagged_members"] < B


# ----------------------------------------------------------------------------- E
@pytest.mark.parametrize("rid", ["tile32", "patch64", "mesh2x2-B1"])
def test_sweep_cap_is_honoured_and_the_context_recovers(hp, solvers, monkeypatch, capfd, rid):
    """Case E.  set_solver(SOLVER_JACOBI, 1e-13, cap) with the cap halfway between the CPU counts of the easy and the hard
    control: the easy sweep meets the oracle; the hard one raises NotConverged or returns a trajectory that meets the
    oracle with a clean log (the permanent move to BiCGStab; the one-workgroup step, which needs fewer sweeps than plain
    Jacobi, may also just fit) -- never a result that misses the oracle, and no log entry beyond the cap.  The cap is
    lowered on a context that has already run the hard sweep, so the budgets remembered from before it (the doubled cap
    of the one-workgroup step among them) lie above it.  With the cap back at 400 both sweeps meet the oracle on the same
    context."""
    cfg = REGIMES[rid]
    B, Nt = cfg["B"], 3
    seeds = list(range(B))
    e, h = cfg["easy"], cfg["hard"]
    ce, ch = _cpu_counts(cfg, e)[0], _cpu_counts(cfg, h)[0]
    cap = (ce + ch) // 2
    assert ce < cap < ch, (ce, cap, ch)
    att = _Attempts(monkeypatch, capfd)
    figs = dict(cap=cap, cpu_easy=ce, cpu_hard=ch)
    with _Run(hp, solvers, cfg, Nt) as R:
        R.assert_regime()
        _, log, _ = R.checked("fwd", [(h,) * (Nt + 1)] * B, seeds)
        figs["iters_hard_before"] = _took_a_repeat(cfg, log, h, "forward, before the cap")
        R.ctx.set_solver(hp.SOLVER_JACOBI, 1e-13, cap)
        att.take()
        _, log, figs["u_easy_capped"] = R.checked("fwd", [(e,) * (Nt + 1)] * B, seeds)
        figs["iters_easy_capped"] = int(log["solver_iters"].max())
        assert log["solver_iters"].max() <= cap, (log["solver_iters"].max(), cap)
        try:
            _, log, figs["u_hard_capped"] = R.checked("fwd", [(h,) * (Nt + 1)] * B, seeds)     # asserts oracle + clean log
            figs["hard_capped"] = f"returned, iters {int(log['solver_iters'].max())}"
            assert log["solver_iters"].max() <= cap, (log["solver_iters"].max(), cap)
        except hp.NotConverged:
            figs["hard_capped"] = "NotConverged"
        figs["attempts_capped"] = att.take()
        R.ctx.set_solver(hp.SOLVER_JACOBI, 1e-13, 400)
        for kind in ("fwd", "adj"):
            for name, amp in (("easy", e), ("hard", h)):
                _, log, figs[f"{kind}_{name}"] = R.checked(kind, [(amp,) * (Nt + 1)] * B, seeds)
                figs[f"iters_{kind}_{name}"] = int(log["solver_iters"].max())
        figs["attempts_after"] = att.take()
    _report(hp, f"E {rid}", **figs)


# ----------------------------------------------------------------------------- F
# Base time steps of case F; the second PDESystems runs at ten times these.  Chemotaxis: the systems' 5e-4.  Schnakenberg:
# 1e-4, because its adjoint operator M_L + dt (A - D) + dt gamma (M - 2 M_uv) loses definiteness where
# dt gamma (2 u v - 1) reaches 1 -- dt = 5.4e-3 for gamma = 230.82 and u v = 0.9, the data of these sweeps.  At ten times
# the systems' 5e-4 the operator is next to singular (Jacobi diverges, BiCGStab breaks down, the sweep ends in
# NotConverged); 1e-3 keeps a factor of five to that bound.
F_DT = {"schnak": 1e-4, "chtxs": 5e-4}
MESH_CHEB_CHECK = 16         # k_mesh_cheb_solve: residual test every 16 iterations, logged count = that of the test + 16


class _SpeciesLog:
    """The checks of tests/test_gpu_systems_regimes.py's _Device, the worst iteration counts of the sweeps, and whether
    every / no species solve ran on Chebyshev"""

    def __init__(self, reg, hp, ctx, Nt, cheb):
        self.D = reg._Device(hp, ctx, Nt, species=True, cheb=cheb)
        self.hp, self.ctx, self.Nt, self.kiters, self.iters, self.cheb = hp, ctx, Nt, 0, 0, set()

    def run(self, sweep, outs, ins, B):
        got = self.D.run(sweep, outs, ins, B)
        klog = self.ctx.traj_krylov_info(self.Nt, B)
        self.kiters = max(self.kiters, int(klog["solver_iters"].max()))
        self.cheb |= set(((klog["flags"] & self.hp.FLAG_CHEBYSHEV) != 0).ravel().tolist())
        self.iters = max(self.iters, int(self.ctx.traj_info(self.Nt, B)["solver_iters"].max()))
        return got


def _species_case(hp, monkeypatch, capfd, system, N, dt, solver, tag):
    """every sweep of ``system`` on a fresh PDESystems (vertex order, unit square, one member) through the comparisons of
    tests/test_gpu_systems_regimes.py -> the _SpeciesLog of the run"""
    import test_gpu_systems_regimes as reg
    systems = importlib.import_module("fem-fct-pdeco_amd.systems")
    monkeypatch.setattr(reg, "_ORACLE", {})             # that module keys its oracle cache without dt: a cache of our own
    att = _Attempts(monkeypatch, capfd)
    Nt, B = 4, 1
    S = systems.PDESystems(hp.SquareMeshP1(0.0, 1.0, N - 1), order=hp.ORDER_VERTEX)
    try:
        knobs = _knobs_default()
        if knobs:       # N = 41: one-workgroup FCT step and species solve; N = 61: 32-tiles and the tile Chebyshev solve
            assert S.ctx.kernel_regime(B) == (hp._lib.REGIME_MESH if N == 41 else hp._lib.REGIME_TILE32)
        S.ctx.set_krylov(1e-13, 2000)
        S.ctx.set_species_solver(solver)
        mem = reg._Members(system, N, B, Nt)
        D = _SpeciesLog(reg, hp, S.ctx, Nt, cheb=knobs and solver == "auto" and tag == "base")
        att.take()
        errs = reg.SYSTEMS[system](hp, systems, S, D, mem, N, dt)
        _report(hp, f"F {tag} {system} N={N} dt={dt:g} {solver}", species_iters=D.kiters, jacobi_iters=D.iters,
                chebyshev=sorted(D.cheb), attempts=att.take(), **errs)
        if solver == "bicgstab":
            assert D.cheb == {False}, D.cheb
        return D
    finally:
        S.close()


@pytest.mark.parametrize("system", ["schnak", "chtxs"])
@pytest.mark.parametrize("N", [41, 61])
def test_species_budget_chebyshev_then_ten_times_the_step(hp, monkeypatch, capfd, N, system):
    """Case F (ii).  Every sweep of the system (forward with the frozen and the per-step control, adjoint with the
    final-time and the all-time misfit) in vertex order on the unit square, N = 41 (one-workgroup species solve) and
    N = 61 (tile Chebyshev), at the base dt (F_DT), where every species solve must carry FLAG_CHEBYSHEV, and then at ten
    times that on a second PDESystems: against the oracle (states < 1e-10, adjoints < 1e-9), both logs clean.  At ten
    times the step some species solve must need more than the 40 iterations a kind starts with (the message carries
    the count; relaxed under a regime-moving knob).  The one-workgroup species solve (N = 41) tests its residual every 16
    iterations and logs the count of the test that passed plus 16, an upper bound, so there the log must exceed 40 + 16.
    Its chemotaxis sweeps (64 logged: stopped at 48) pass that by being resized from one sweep to the next, not by a
    repeat: each of the four sweeps took one attempt; the Schnakenberg sweeps (224 / 351 iterations, more attempts than sweeps) are
    repeated.  Which solver ended up running there is reported, not asserted:
    the controller may give a kind whose Chebyshev iteration runs out to BiCGStab for good."""
    _species_case(hp, monkeypatch, capfd, system, N, F_DT[system], "auto", "base")
    D = _species_case(hp, monkeypatch, capfd, system, N, 10 * F_DT[system], "auto", "10x")
    if _knobs_default():
        least = jc.START_KBUDGET + (MESH_CHEB_CHECK if N == 41 else 0)
        assert D.kiters > least, (f"{system} N={N}: the species solves at dt = {10 * F_DT[system]:g} logged {D.kiters} "
                                  f"iterations, not more than {least} (the starting {jc.START_KBUDGET}; at N = 41 plus the "
                                  f"{MESH_CHEB_CHECK} of the one-workgroup solve's test interval)")


# Jacobi-preconditioned scipy.sparse.linalg.bicgstab on the species matrix of the forward sweep, to 1e-13 (a guide):
#   Schnakenberg  M + dt (Dv Ad + gamma M), Dv = 8.6676:  dt = 5e-4: 52 (N = 41) / 80 (N = 61); dt = 1e-3: 72 / 115
#   chemotaxis    M + dt (Df Ad + delta M), Df = 0.05, delta = 100:  dt = 5e-3: 11 / 18; 2.5e-2: 18 / 29; 5e-2: 20 / 29;
#                 0.2: 20 / 31 -- the count saturates, because the matrix tends to dt (Df Ad + delta M), whose condition
#                 number does not depend on dt; on the device 13 / 22 iterations at dt = 5e-3
# so the Schnakenberg sweeps reach case F (i) at dt = 1e-3 and no time step brings the chemotaxis ones there.
@pytest.mark.parametrize("N", [41, 61])
def test_species_budget_bicgstab_beyond_its_first_budget(hp, monkeypatch, capfd, N):
    """Case F (i).  The Schnakenberg species solves on BiCGStab (set_species_solver("bicgstab"), set_krylov(1e-13, 2000))
    at dt = 1e-3: the first sweep of a kind needs more than the 40 iterations it starts with and is repeated.  Against
    the oracle, both logs clean, no solve on Chebyshev, and some species solve beyond 40 iterations.  The chemotaxis
    system has no such input (see the guide counts above)."""
    D = _species_case(hp, monkeypatch, capfd, "schnak", N, 1e-3, "bicgstab", "bicgstab")
    if _knobs_default():
        assert D.kiters > jc.START_KBUDGET, (f"N={N}: BiCGStab needed {D.kiters} iterations, not more than the starting "
                                             f"{jc.START_KBUDGET}; the CPU guide needs {72 if N == 41 else 115}")
