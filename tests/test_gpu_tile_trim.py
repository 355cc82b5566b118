"""GPU tests of the trimmed prologues and epilogues of the latency-regime tile launches (FEMFCT_TILE_TRIM, -m gpu).

FEMFCT_TILE_TRIM is a bit mask read once per context.  Bit 1: the Jacobi launches of a solve whose residual test is
deferred (2 to 4 launches) end with the waves that hold owned rows -- one partial slot per (workgroup, owning wave)
instead of a block reduction -- and the du/dt launch reduces that many slots.  Bit 8: the output stores of the four
launches are write-through stores.  0 is the code as it was.  Maxima and minima are exact in any order and a store
stores what it is given: every bit of the trajectories, of the descent direction and of the per-step solver records
must be the same."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DT, OM = 1e-3, np.pi / 40
NT = 12                                 # steps per sweep: 12 forward + 12 adjoint
MASKS = ("1", "8", "9")                 # each kept bit alone, and all kept bits (the default)
# time steps at which the C2 operator on the 81 x 81 mesh needs 3, 4 and 5 launches in the forward sweep at rel_tol = 1e-13
# (the Jacobi contraction is about dt a / (m + dt a): two launches at 1e-3); the tests assert the counts they rely on
DT_THREE, DT_FOUR, DT_FIVE = 2e-3, 2.5e-3, 4e-3


@pytest.fixture(scope="module")
def hp():
    mod = importlib.import_module("fem-fct-pdeco_amd")
    mod.fct_helpers.VERBOSE = False
    return mod


@pytest.fixture(scope="module")
def solvers():
    return importlib.import_module("fem-fct-pdeco_amd.solvers")


def inputs(hp, N, Nt, c5, batch):
    """(u0, controls, target) in vertex order: slotted disc and a smooth space-time control (C2), or a Gaussian and
    c = 1 (C5), as bench.py sets them up; member m of a batch gets its own phase and amplitude."""
    mesh = hp.SquareMeshP1(-1, 1, N - 1)
    x, y = mesh.coordinates()
    if c5:
        u0 = np.exp(-20 * ((x + 2 / 3) ** 2 + 5 * (y + 5 / 6) ** 2))
    else:
        R = np.sqrt(x ** 2 + (y - 1 / 3) ** 2)
        u0 = ((R < 1 / 3) & ((np.abs(x) > 0.05) | (y > 0.5))).astype(np.float64)
    t = np.linspace(0.0, 1.0, Nt + 1)[:, None]
    cs = []
    for m in range(batch):
        if c5 and batch == 1:
            cs.append(np.ones((Nt + 1) * mesh.nodes))
        else:
            cs.append(np.clip(1.5 + (1.0 - 0.1 * m) * np.sin(2 * np.pi * (x[None, :] + t + 0.3 * m)) * np.cos(np.pi * y[None, :])
                              + 0.5 * t, 0.0, 5.0).reshape(-1))
    return mesh, u0, np.stack(cs), np.roll(u0, 7)


class Sweeper:
    """One context (created after the environment is set) and the device arrays of run()."""

    def __init__(self, hp, solvers, monkeypatch, trim, N=81, Nt=NT, c5=False, batch=1, graphs=True, eps=0.0, dt=DT, env=None,
                 u0_poison=None, max_iters=None, control=None):
        monkeypatch.setenv("FEMFCT_TILE_TRIM", trim)
        for k, v in (env or {}).items():
            monkeypatch.setenv(k, v)
        mesh, u0, c, uhat = inputs(hp, N, Nt, c5, batch)
        if control is not None:
            c = control(mesh, Nt)
        self.hp, self.n, self.Nt, self.batch = hp, mesh.nodes, Nt, batch
        self.alltime = c5 or batch > 1
        self.prob = solvers.SolidBodyDrift(mesh, Nt, dt, om=OM, eps=eps, rot_scale=0.0 if c5 else 1.0, batch=batch,
                                           order=hp.ORDER_VERTEX)
        try:
            ctx = self.prob.ctx
            ctx.set_graphs(graphs)
            if max_iters is not None:
                ctx.set_solver(max_iters=max_iters)
            assert ctx.kernel_regime(batch) == hp._lib.REGIME_TILE32
            tl = (Nt + 1) * self.n
            init = np.zeros((batch, tl))
            init[:, :self.n] = u0
            if u0_poison is not None:
                init[0, u0_poison] = np.nan
            self.d_c, self.d_u = ctx.array(c.ravel()), ctx.array(init.ravel())
            self.d_uhat = ctx.array(np.tile(uhat, batch * (Nt + 1)) if self.alltime else uhat)
            self.d_p, self.d_d = ctx.zeros(batch * tl), ctx.zeros(tl)
        except Exception:
            self.prob.close()
            raise
        self.logf = self.loga = None

    def forward(self):
        try:
            self.prob.forward(self.d_c, self.d_u, batch=self.batch)
        finally:
            self.logf = {k: v.copy() for k, v in self.prob.solver_log(self.batch).items()}

    def adjoint(self):
        self.prob.adjoint(self.d_c, self.d_u, self.d_uhat, self.d_p, "alltime" if self.alltime else "finaltime", batch=self.batch)
        self.loga = {k: v.copy() for k, v in self.prob.solver_log(self.batch).items()}

    def result(self):
        if self.batch == 1:                 # (the direction is a single-trajectory call)
            self.prob.descent_direction(self.d_c, self.d_u, self.d_p, 1.0, self.d_d)
        return dict(u=self.d_u.download(), p=self.d_p.download(), d=self.d_d.download(), logf=self.logf, loga=self.loga)

    def close(self):
        self.prob.close()


def run(hp, solvers, monkeypatch, trim, **kw):
    s = Sweeper(hp, solvers, monkeypatch, trim, **kw)
    try:
        for _ in range(2):                  # the second sweep of each kind runs at the settled budget
            s.forward()
        for _ in range(2):
            s.adjoint()
        return dict(s.result(), info=s.prob.ctx.tile_trim_info())
    finally:
        s.close()


def assert_same_bits(a, b):
    for k in ("u", "p", "d"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    for la, lb in ((a["logf"], b["logf"]), (a["loga"], b["loga"])):
        assert (la is None) == (lb is None)
        for k in (la or {}):
            assert np.array_equal(la[k], lb[k], equal_nan=True), k


def assert_trim_is_neutral(hp, solvers, monkeypatch, expect_waves=True, **kw):
    """Each bit alone and all kept bits against 0; returns the run with 0."""
    off = run(hp, solvers, monkeypatch, "0", **kw)
    assert np.abs(off["u"]).max() > 0 and np.abs(off["p"]).max() > 0
    assert np.isfinite(off["u"]).all() and np.isfinite(off["p"]).all()
    assert off["info"]["mask"] == 0 and off["info"]["wave_launches"] == 0 and off["info"]["wt_launches"] == 0
    for mask in MASKS:
        on = run(hp, solvers, monkeypatch, mask, **kw)
        assert_same_bits(on, off)
        # the knob was read and its kernels were enqueued (expect_waves: whether the solves of this case defer their test
        # and their slots fit an array)
        assert on["info"]["mask"] == int(mask)
        assert (on["info"]["wt_launches"] > 0) == bool(int(mask) & 8)
        if expect_waves is not None:
            assert (on["info"]["wave_launches"] > 0) == (expect_waves and bool(int(mask) & 1))
            assert (on["info"]["wave_slots"] > 0) == (expect_waves and bool(int(mask) & 1))
    return off


@pytest.mark.parametrize("c5", [False, True], ids=["c2-finaltime", "c5-alltime"])
def test_flagship_kernels(hp, solvers, monkeypatch, c5):
    """N = 81, one trajectory: 2 x 13 sweeps on 6 x 6 tiles (C2), and without rotation 2 x 12 on 8 x 8 tiles (C5): four
    owning waves of sixteen either way."""
    off = assert_trim_is_neutral(hp, solvers, monkeypatch, c5=c5)
    assert 0 < off["logf"]["solver_iters"].max() <= 26 and 0 < off["loga"]["solver_iters"].max() <= 26      # two launches


@pytest.mark.parametrize("N", [45, 53])
def test_ragged_tile_grid(hp, solvers, monkeypatch, N):
    """The last row and column of tiles hang over the mesh edge: border tiles have owned rows in fewer waves (the others
    publish the identity)."""
    assert_trim_is_neutral(hp, solvers, monkeypatch, N=N, env={"FEMFCT_MESH_STEP": "0"})


@pytest.mark.parametrize("batch", [2, 8])
def test_batch_with_different_controls(hp, solvers, monkeypatch, batch):
    """Per-member partial slots and level use (blockIdx.z)."""
    assert_trim_is_neutral(hp, solvers, monkeypatch, batch=batch)


def test_full_rows_three_launches(hp, solvers, monkeypatch):
    """eps = 1e-3: diffusion fills every off-diagonal; at dt = 2e-3 the forward solve takes three launches (one partk slot
    row per launch), the adjoint's three or four."""
    off = assert_trim_is_neutral(hp, solvers, monkeypatch, eps=1e-3, dt=DT_THREE)
    assert 26 < off["logf"]["solver_iters"].max() <= 39 and 26 < off["loga"]["solver_iters"].max() <= 52


def test_four_launches(hp, solvers, monkeypatch):
    """The longest solve whose test is still deferred."""
    off = assert_trim_is_neutral(hp, solvers, monkeypatch, dt=DT_FOUR)
    assert 39 < off["logf"]["solver_iters"].max() <= 52


def test_five_launches_run_the_in_launch_test(hp, solvers, monkeypatch):
    """Five launches: every launch tests the residual of the one before (block reductions, per-workgroup partials) --
    the path as it was, with the same sweep counts."""
    off = assert_trim_is_neutral(hp, solvers, monkeypatch, dt=DT_FIVE, expect_waves=None)    # (the sweeps on the way to the settled budget may defer)
    assert 52 < off["logf"]["solver_iters"].max() <= 65
    assert off["loga"]["solver_iters"].max() > 52


def test_more_slots_than_an_array_holds_fall_back(hp, solvers, monkeypatch):
    """N = 257 with room for 1024 workgroups: whichever halo the plan takes (8 .. 11: 17 .. 26 tiles per side, 8 or 6 owning
    waves), tiles^2 x owning waves > FEMFCT_MAX_PARTIALS = 2048, so the Jacobi launches (dt scaled with the mesh width,
    as many sweeps as at N = 81) keep their block reduction; bit 8 still applies."""
    assert min(17 * 17 * 8, 19 * 19 * 8, 22 * 22 * 6, 26 * 26 * 6) > 2048 and 33 * 33 > 1024
    assert_trim_is_neutral(hp, solvers, monkeypatch, N=257, Nt=4, dt=3e-4, env={"FEMFCT_WG_SLOTS": "1024"}, expect_waves=False)


def test_graphs_off(hp, solvers, monkeypatch):
    assert_trim_is_neutral(hp, solvers, monkeypatch, graphs=False)


# The issue's case "more contexts alive than the level table has slots" is not covered: the level table (bit 4) was built,
# measured slower and removed, so there are no slots.  What is left of it:
def test_five_plain_contexts_alive_two_sweeping_alternately(hp, solvers, monkeypatch):
    """What a context keeps for the trimmed launches (the knob, its partial slots) is its own: five contexts alive, two
    of them -- on different meshes -- sweeping in turns."""
    kws = (dict(N=81), dict(N=53, env={"FEMFCT_MESH_STEP": "0"}))
    off = [run(hp, solvers, monkeypatch, "0", **kw) for kw in kws]
    for mask in MASKS:
        idle = [Sweeper(hp, solvers, monkeypatch, mask, N=45, Nt=2, env={"FEMFCT_MESH_STEP": "0"}) for _ in range(3)]
        pair = [Sweeper(hp, solvers, monkeypatch, mask, **kw) for kw in kws]
        try:
            idle[0].forward()
            for _ in range(2):
                for s in pair:
                    s.forward()
            for _ in range(2):
                for s in pair:
                    s.adjoint()
            for s, o in zip(pair, off):
                assert_same_bits(s.result(), o)
        finally:
            for s in idle + pair:
                s.close()


# (gx, gy) on the 81 x 81 mesh with 6 x 6 tiles: row 6 b + 5 is the tile's last owned row -- alone in the last owning
# wave (patch rows 18 and 19); a tile's corner node (6 a, 6 b) lies in the first halo ring of its W, S and SW neighbours
@pytest.mark.parametrize("node", [(40, 41), (36, 36)], ids=["last-owning-wave", "first-ring-of-three-tiles"])
def test_nan_in_u0_fails_as_before(hp, solvers, monkeypatch, node):
    def outcome(trim):
        s = Sweeper(hp, solvers, monkeypatch, trim, Nt=4, u0_poison=node[1] * 81 + node[0])
        try:
            try:
                s.forward()
                raised = None
            except hp._lib.FemFctError as e:
                raised = type(e)
            return raised, s.logf, s.d_u.download()
        finally:
            s.close()

    r0, log0, u0 = outcome("0")
    assert r0 is not None or (log0["flags"] != 0).any()
    for mask in MASKS:
        r, log, u = outcome(mask)
        assert r is r0
        assert np.array_equal(u, u0, equal_nan=True)
        for k in log0:
            assert np.array_equal(log[k], log0[k], equal_nan=True), k


def test_rowsum_flag_on_the_same_steps(hp, solvers, monkeypatch):
    """A time step far beyond the scheme's restriction (as tests/test_gpu_mesh_step.py sets it up): some row sum of L is
    not positive.  The budget is held at three launches, so the deferred test -- which reduces the row sums from the
    per-wave slots -- writes the record."""
    def control(mesh, Nt):
        x, y = mesh.coordinates()
        return np.tile(5.0 * np.sin(3 * x) * np.cos(2 * y), Nt + 1)[None, :]

    def outcome(trim):
        s = Sweeper(hp, solvers, monkeypatch, trim, Nt=2, dt=0.5, max_iters=39, control=control)
        try:
            try:
                s.forward()
            except hp._lib.FemFctError:
                pass                        # (the solve itself may refuse such a step)
            return s.logf
        finally:
            s.close()

    log0 = outcome("0")
    assert log0["flags"][0, 0] & hp.FLAG_MMATRIX_ROWSUM and log0["min_rowsum"][0, 0] <= 0.0
    for mask in MASKS:
        log = outcome(mask)
        for k in log0:
            assert np.array_equal(log[k], log0[k], equal_nan=True), k
