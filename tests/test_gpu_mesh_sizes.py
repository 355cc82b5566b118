"""The one-workgroup FEM-FCT step (k_mesh_step, csrc/kernels_mesh.hip) at every mesh size where its control flow changes
(-m gpu): the sizes and inputs of tests/mesh_sizes_cases.py, pinned on the CPU by tests/test_mesh_sizes_cases.py.  One
test and one context per size, and the 81 x 81 dispatch with a non-flux matrix at 64 members.

Every call of ctx.fct_step holds ("one-workgroup kernels by size"):
  per node        |u_i - ref_i| <= TOL_STEP max_j |ref_j| per member and node, ref = oracle.fct.fct_step: the project's
                  step bar 1e-9 in max norm per node instead of relative l2, so that no corner or side node hides in the
                  norm of the interior; the worst error of every node class is printed
  solver info     check_infos of test_gpu_generic_patterns.py: no FLAG_SOLVER_BUDGET, solver_resid <= 1e-13, min_rowsum
                  to rtol 1e-9, FLAG_MMATRIX_ROWSUM by its sign
  bits            member 0 of the batch == member 0 alone; graphs on == off; N shared == N per member (the same N)
  no stray write  u_out, u_n, rhs, A and N lie in larger device buffers between 64 sentinel doubles each; u_out is
                  pre-filled with NaN: afterwards every output is finite, every sentinel has its bits and no input
                  has changed a bit
"""
import importlib

import numpy as np
import pytest

import generic_patterns as gp
import mesh_sizes_cases as ms
from regime_helpers import regime_knobs_default
from test_gpu_generic_patterns import check_infos, oracle

pytestmark = pytest.mark.gpu

TOL_STEP = 1e-9
GUARD = 64


@pytest.fixture(scope="module")
def hp():
    mod = importlib.import_module("fem-fct-pdeco_amd")
    mod.fct_helpers.VERBOSE = False
    return mod


def _nans(count, tag):
    """`count` quiet NaNs that differ in their payload (tag and index): a sentinel's bits say where it was written"""
    bits = np.uint64(0x7FF8000000000000) | (np.uint64(tag) << np.uint64(32)) | np.arange(1, count + 1, dtype=np.uint64)
    return bits.view(np.float64)


class Guarded:
    """`count` doubles on the device between GUARD sentinel doubles on either side"""

    def __init__(self, ctx, count, tag):
        self.count = int(count)
        self.fill = _nans(self.count + 2 * GUARD, tag)
        self.buf = ctx.array(self.fill)
        self.ptr = self.buf.ptr + 8 * GUARD
        self.bits = None

    def refill(self):
        self.buf.upload(self.fill)

    def put(self, host):
        """the payload from a host array; the buffer's bits from now on are the ones it may not lose"""
        whole = self.fill.copy()
        whole[GUARD:GUARD + self.count] = np.asarray(host, dtype=np.float64).ravel()
        self.buf.upload(whole)
        return self.freeze()

    def freeze(self):
        self.bits = self.buf.download().view(np.uint64).copy()
        return self

    def check_unchanged(self, what):
        got = self.buf.download().view(np.uint64)
        bad = np.flatnonzero(got != self.bits)
        assert bad.size == 0, (what, "changed at", (bad[:8] - GUARD).tolist(), bad.size)

    def payload_and_check_sentinels(self, what):
        got = self.buf.download()
        g, want = got.view(np.uint64), self.fill.view(np.uint64)
        for side, sl in (("before", slice(0, GUARD)), ("after", slice(GUARD + self.count, None))):
            bad = np.flatnonzero(g[sl] != want[sl])
            assert bad.size == 0, (what, "sentinel", side, bad.tolist())
        return got[GUARD:GUARD + self.count].copy()

    def free(self):
        self.buf.free()


class StepRunner:
    """ctx.fct_step on device ELL operands as run_step of test_gpu_generic_patterns.py does, every operand guarded"""

    def __init__(self, hp, ctx, P, members):
        self.hp, self.ctx, self.P, self.members = hp, ctx, P, list(members)
        B, n, wn = len(self.members), ctx.n, ctx.W * ctx.n
        self.B = B
        self.A = Guarded(ctx, B * wn, 1)
        self.Nm = Guarded(ctx, B * wn, 2)
        for b, m in enumerate(self.members):
            ctx.csr_to_ell(P.A[m].data, out=self.A.ptr + 8 * b * wn)
            ctx.csr_to_ell(P.N.data, out=self.Nm.ptr + 8 * b * wn)
        self.A.payload_and_check_sentinels("A after csr_to_ell")
        self.Nm.payload_and_check_sentinels("N after csr_to_ell")
        self.A.freeze()
        self.Nm.freeze()
        self.u_n = Guarded(ctx, B * n, 3).put(np.concatenate([P.u_n[m] for m in self.members]))
        self.rhs = Guarded(ctx, B * n, 4).put(np.concatenate([P.rhs[m] for m in self.members]))
        self.out = Guarded(ctx, B * n, 5)

    def run(self, what, rhs=False, N=False, N_shared=False, graphs=True):
        """-> (u[B, n], infos); asserts that nothing but u_out was written"""
        ctx, hp, B = self.ctx, self.hp, self.B
        try:
            ctx.set_graphs(graphs)
            for _ in range(8):      # a step that the adapted sweep budget did not suffice for is repeated (femfct.h)
                self.out.refill()
                ctx.fct_step(self.A.ptr, self.u_n.ptr, self.P.dt, self.out.ptr, rhs=self.rhs.ptr if rhs else None,
                             N_ell=self.Nm.ptr if N else None, N_shared=N_shared, batch=B)
                infos = ctx.last_step_info(B)
                if not any(i["flags"] & hp.FLAG_SOLVER_BUDGET for i in infos):
                    break
        finally:
            ctx.set_graphs(True)
        u = self.out.payload_and_check_sentinels(what + ": u_out").reshape(B, ctx.n)
        assert np.all(np.isfinite(u)), (what, "outputs not written or not finite:", np.flatnonzero(~np.isfinite(u))[:8].tolist())
        for name in ("A", "Nm", "u_n", "rhs"):
            getattr(self, name).check_unchanged(f"{what}: {name}")
        return u, infos

    def free(self):
        for g in (self.A, self.Nm, self.u_n, self.rhs, self.out):
            g.free()


def node_errors(P, members, u, **okw):
    """[B, n]: |u_i - ref_i| / max_j |ref_j| per member against the oracle's step"""
    out = np.empty_like(u)
    for b, m in enumerate(members):
        ref = oracle(P, m, **okw)[0]
        out[b] = np.abs(u[b] - ref) / np.abs(ref).max()
    return out


def check_member_infos(hp, infos, P, members, what, **okw):
    """check_infos for the members `members` of P (entry b of infos is member members[b])"""
    if list(members) == list(range(len(infos))):
        return check_infos(hp, infos, P, what, **okw)
    for inf, m in zip(infos, members):
        assert not (inf["flags"] & hp.FLAG_SOLVER_BUDGET), (what, m, inf)
        assert inf["solver_resid"] <= 1e-13, (what, m, inf)
        rowsum = oracle(P, m, **okw)[1]["l_rowsum"].min()
        assert abs(inf["min_rowsum"] - rowsum) <= 1e-9 * abs(rowsum), (what, m, inf, rowsum)
        assert bool(inf["flags"] & hp.FLAG_MMATRIX_ROWSUM) == (not rowsum > 0), (what, m, inf, rowsum)


def _fmt(errs):
    return ", ".join(f"{k}={v:.2e}" for k, v in errs.items())


@pytest.mark.parametrize("size", ms.SIZES, ids=[f"N{s.N}" for s in ms.SIZES])
def test_step_at_size(hp, size):
    """(a) no rhs, no N; (b) rhs; (c) rhs and N per member; (d) rhs and N shared on three members, (a) and (c) for member 0
    alone, (c) with graphs off -- every call against the oracle per node, its infos, the bits and the stray writes."""
    N = size.N
    P = ms.problem(N)
    ctx = hp.Context(0)
    worst = {k: 0.0 for k in ms.CLASSES}
    runners = []
    try:
        ctx.set_mesh_square(0.0, 1.0, N - 1, hp.ORDER_VERTEX)
        assert ctx.n == N * N and ctx.W == 7
        if regime_knobs_default():
            assert ctx.kernel_regime(ms.MEMBERS) == hp._lib.REGIME_MESH and ctx.kernel_regime(1) == hp._lib.REGIME_MESH
        batch, alone = StepRunner(hp, ctx, P, range(ms.MEMBERS)), StepRunner(hp, ctx, P, [0])
        runners += [batch, alone]
        calls = (
            # name, runner, arguments of the step, the oracle's variant
            ("a", batch, dict(), dict(rhs=False, N=False)),
            ("b", batch, dict(rhs=True), dict(rhs=True, N=False)),
            ("c", batch, dict(rhs=True, N=True), dict(rhs=True, N=True)),
            ("d", batch, dict(rhs=True, N=True, N_shared=True), dict(rhs=True, N=True)),
            ("a alone", alone, dict(), dict(rhs=False, N=False)),
            ("c alone", alone, dict(rhs=True, N=True), dict(rhs=True, N=True)),
            ("c eager", batch, dict(rhs=True, N=True, graphs=False), dict(rhs=True, N=True)),
        )
        got = {}
        for name, runner, args, okw in calls:
            what = f"N={N} ({name})"
            u, infos = runner.run(what, **args)
            got[name] = u
            err = node_errors(P, runner.members, u, **okw)
            by_class = ms.class_errors(N, err)
            print(f"[mesh sizes] {what}: {_fmt(by_class)}, bar={TOL_STEP:.0e}")
            for k, v in by_class.items():
                worst[k] = max(worst[k], v)
            b, i = np.unravel_index(np.argmax(err), err.shape)
            assert err.max() <= TOL_STEP, (what, "member", runner.members[b], "node (ix, iy)", (i % N, i // N), err.max())
            check_member_infos(hp, infos, P, runner.members, what, **okw)
        bits = lambda x: x.view(np.uint64)
        assert np.array_equal(bits(got["a"][0]), bits(got["a alone"][0])), "batched member 0 vs alone, no rhs, no N"
        assert np.array_equal(bits(got["c"][0]), bits(got["c alone"][0])), "batched member 0 vs alone, rhs and N"
        assert np.array_equal(bits(got["c"]), bits(got["c eager"])), "graphs on vs off"
        assert np.array_equal(bits(got["c"]), bits(got["d"])), "N per member vs shared"
        # the variants are different problems (a step that ignored rhs or N would not show in the bits above)
        for x, y in (("a", "b"), ("b", "c")):
            assert np.abs(got[x] - got[y]).max() > 1e-6 * np.abs(got[y]).max(), (x, y)
    finally:
        for r in runners:
            r.free()
        ctx.close()
    print(f"[mesh sizes] N={N} TX={size.TX} worst per class: {_fmt(worst)}, bar={TOL_STEP:.0e}  ({size.reason})")


def test_step_81x81_with_a_non_flux_matrix_leaves_the_one_workgroup_kernel(hp):
    """The 3 x 3-block instantiation has no variant with a non-flux matrix: at 81 x 81 and 64 members a step without N
    runs in one workgroup per member, the same members with a shared N go to the tiles.  Both runs: members 0, 31 and
    63 against the oracle per node, all 64 without FLAG_SOLVER_BUDGET and with solver_resid <= 1e-13."""
    N, B, held = 81, 64, (0, 31, 63)
    P = ms.problem(N, B)
    for m in range(B):
        for Nmat in (None, P.N):
            assert gp.jacobi_norm(P.M, P.A[m], P.ml, P.dt, Nmat) <= 0.5
    ctx = hp.Context(0)
    runner = None
    try:
        ctx.set_mesh_square(0.0, 1.0, N - 1, hp.ORDER_VERTEX)
        if regime_knobs_default():
            assert ctx.kernel_regime(B) == hp._lib.REGIME_MESH and ctx.kernel_regime(B - 1) != hp._lib.REGIME_MESH
        runner = StepRunner(hp, ctx, P, range(B))
        got = {}
        for name, args, okw in (("no N", dict(rhs=True), dict(rhs=True, N=False)),
                                ("N shared", dict(rhs=True, N=True, N_shared=True), dict(rhs=True, N=True))):
            what = f"N=81 B=64 ({name})"
            u, infos = runner.run(what, **args)
            got[name] = u
            for m, inf in enumerate(infos):
                assert not (inf["flags"] & hp.FLAG_SOLVER_BUDGET), (what, m, inf)
                assert inf["solver_resid"] <= 1e-13, (what, m, inf)
            err = node_errors(P, held, u[list(held)], **okw)
            by_class = ms.class_errors(N, err, block=3)
            print(f"[mesh sizes] {what}, members {held}: {_fmt(by_class)}, bar={TOL_STEP:.0e}")
            b, i = np.unravel_index(np.argmax(err), err.shape)
            assert err.max() <= TOL_STEP, (what, "member", held[b], "node (ix, iy)", (i % N, i // N), err.max())
            check_member_infos(hp, [infos[m] for m in held], P, held, what, **okw)
        assert np.abs(got["no N"] - got["N shared"]).max() > 1e-6 * np.abs(got["no N"]).max()
    finally:
        if runner is not None:
            runner.free()
        ctx.close()
