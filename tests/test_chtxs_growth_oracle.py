"""The CPU reference of the chemotaxis sweeps with a growth term (tests/chtxs_growth_oracle.py), checked by itself."""
import numpy as np
import pytest

import chtxs_growth_oracle as go
import per_step_oracle as pso
from oracle import traj as otraj
from oracle.assembly import P1Assembler
from oracle.fct import cost_functional
from oracle.mesh import SquareMesh

N = 11
MIMURA, LOGISTIC = (0.0, 1.0, -1.0), (4.0, -1.0, 0.0)


@pytest.fixture(scope="module")
def fem():
    mesh = SquareMesh(0.0, 1.0, N - 1)
    return mesh, P1Assembler(mesh)


def _traj(x0, Nt):
    return np.concatenate([x0, np.zeros(Nt * x0.size)])


def test_zero_growth_is_the_oracle_bit_for_bit(fem):
    """growth=None and growth=(0, 0, 0) give the bits of the unmodified oracle sweeps: forward with the frozen and the
    per-step control, adjoint with the final-time and the all-time misfit (11 x 11, 4 steps)."""
    mesh, asm = fem
    n, Nt, dt = mesh.nodes, 4, 5e-4
    tl = (Nt + 1) * n
    rng = np.random.default_rng(11)
    u0, v0 = 1.5 + 0.1 * (0.5 - rng.random(n)), 1.5 + 0.1 * (0.5 - rng.random(n))
    c = 20 * rng.random(tl)
    for per_step, ref_fn in ((False, otraj.solve_chtxs_system), (True, pso.solve_chtxs_system)):
        ur, vr = ref_fn(c, _traj(u0, Nt), _traj(v0, Nt), asm, n, Nt, dt)
        for growth in (None, (0.0, 0.0, 0.0)):
            u, v = go.solve_chtxs_system(c, _traj(u0, Nt), _traj(v0, Nt), asm, n, Nt, dt, growth=growth, per_step=per_step)
            assert np.array_equal(u, ur) and np.array_equal(v, vr), (per_step, growth)
    uhat, vhat = 0.9 * ur + 0.02 * rng.random(tl), 1.05 * vr + 0.02 * rng.random(tl)
    for optim, tu, tv in (("finaltime", uhat[Nt * n:], vhat[Nt * n:]), ("alltime", uhat, vhat)):
        pr, qr = otraj.solve_adjoint_chtxs_system(ur, vr, tu, tv, np.zeros(tl), np.zeros(tl), c, Nt * dt, asm, n, Nt, dt,
                                                  None, optim)
        assert np.abs(pr[:n]).max() > 0 and np.abs(qr[:n]).max() > 0
        for growth in (None, (0.0, 0.0, 0.0)):
            p, q = go.solve_adjoint_chtxs_system(ur, vr, tu, tv, np.zeros(tl), np.zeros(tl), c, Nt * dt, asm, n, Nt, dt,
                                                 None, optim, growth=growth)
            assert np.array_equal(p, pr) and np.array_equal(q, qr), (optim, growth)


def closed_form(growth, a0, b0, c, pT, qT, Nt, dt, delta, rescaling):
    """The scalar recursions constant states obey: gradients vanish, Ad 1 = 0 and the antidiffusive fluxes of a constant
    are zero, so the step is  a_{n+1} = a_n + dt r(a_n),  (1 + dt delta) b_{n+1} = b_n + dt c a_n / rescaling  and,
    backwards,  p_n = p_{n+1} + dt (c q_{n+1} / rescaling + r'(a_n) p_{n+1}),  q_n = q_{n+1} / (1 + dt delta)."""
    a, b = [a0], [b0]
    for _ in range(Nt):
        b.append((b[-1] + dt * c * a[-1] / rescaling) / (1 + dt * delta))
        a.append(a[-1] + dt * go.r(a[-1], growth))
    p, q = [pT], [qT]
    for k in range(Nt - 1, -1, -1):
        p.insert(0, p[0] + dt * (c * q[0] / rescaling + go.dr(a[k], growth) * p[0]))
        q.insert(0, q[0] / (1 + dt * delta))
    return np.array(a), np.array(b), np.array(p), np.array(q)


@pytest.mark.parametrize("growth", [MIMURA, LOGISTIC], ids=["m2(1-m)", "m(4-m)"])
def test_constant_states_follow_the_scalar_recursions(fem, growth):
    """u = a, v = b, a constant control and constant terminal values on the 11 x 11 mesh: every level of the forward and
    of the final-time adjoint sweep equals the scalar recursion (closed_form) to 1e-13 relative, the project's bound for
    closed-form answers.  Without the adjoint growth load (drop_adjoint_load) the p recursion is missed by orders of
    magnitude more, |r'| dt per step: the check that notices a dropped or mis-signed r'(u) p term."""
    mesh, asm = fem
    n, Nt, dt, resc = mesh.nodes, 6, 5e-3, 0.1
    tl = (Nt + 1) * n
    a0, b0, c, delta = 1.5, 1.2, 7.0, otraj.chtxs_params()["delta"]
    u, v = go.solve_chtxs_system(np.full(tl, c), _traj(np.full(n, a0), Nt), _traj(np.full(n, b0), Nt), asm, n, Nt, dt,
                                 rescaling=resc, growth=growth, per_step=True)
    uT, vT = u[Nt * n], v[Nt * n]
    pT, qT = 0.3, -0.2
    a, b, p, q = closed_form(growth, a0, b0, c, pT, qT, Nt, dt, delta, resc)
    one = np.ones(n)
    err = lambda x, s: np.abs(x.reshape(Nt + 1, n) - s[:, None]).max() / np.abs(s).max()
    assert err(u, a) < 1e-13 and err(v, b) < 1e-13, (err(u, a), err(v, b))
    assert abs(a[-1] - a0) > 1e-3          # growth acted
    args = (u, v, (uT + pT) * one, (vT + qT) * one)
    pk, qk = go.solve_adjoint_chtxs_system(*args, np.zeros(tl), np.zeros(tl), np.full(tl, c), Nt * dt, asm, n, Nt, dt, None,
                                           "finaltime", rescaling=resc, growth=growth)
    print(f"[growth oracle] closed form {growth}: u {err(u, a):.2e} v {err(v, b):.2e} p {err(pk, p):.2e} q {err(qk, q):.2e}")
    assert err(pk, p) < 1e-13 and err(qk, q) < 1e-13, (err(pk, p), err(qk, q))
    pd, _ = go.solve_adjoint_chtxs_system(*args, np.zeros(tl), np.zeros(tl), np.full(tl, c), Nt * dt, asm, n, Nt, dt, None,
                                          "finaltime", rescaling=resc, growth=growth, drop_adjoint_load=True)
    assert err(pd, p) > 1e-3, err(pd, p)


def _gradient_mismatch(asm, M, mesh, growth, drop=False):
    """|<beta c - q u / rescaling, dc>_Q - central difference of J| / |central difference|, all-time reduced cost"""
    n, Nt, dt, beta, resc, eps = mesh.nodes, 20, 5e-3, 1e-3, 0.1, 1e-3
    tl = (Nt + 1) * n
    x, y = mesh.x[mesh.dof_to_vertex], mesh.y[mesh.dof_to_vertex]
    u0 = 1.5 + 0.05 * np.cos(3 * np.pi * x) * np.cos(2 * np.pi * y)
    k = np.arange(Nt + 1)[:, None]
    c = (8 * (1 + 0.3 * np.sin(2 * np.pi * x) * np.cos(np.pi * y))[None, :] * (1 + 0.2 * np.sin(2 * np.pi * k / Nt))).ravel()
    dc = ((np.cos(np.pi * x) * np.sin(2 * np.pi * y) + 0.5)[None, :] * (1 + 0.5 * np.cos(np.pi * k / Nt))).ravel()

    def state(cc):
        u, v = go.solve_chtxs_system(cc, _traj(u0, Nt), _traj(u0, Nt), asm, n, Nt, dt, rescaling=resc, growth=growth,
                                     per_step=True)
        return u.copy(), v.copy()
    ut, vt = state(np.full(tl, 12.0))

    def J(cc):
        uu, vv = state(cc)
        return cost_functional(uu, ut, cc, Nt, dt, M, beta, "alltime", var2=vv, var2_target=vt)
    u, v = state(c)
    _, q = go.solve_adjoint_chtxs_system(u, v, ut, vt, np.zeros(tl), np.zeros(tl), c, Nt * dt, asm, n, Nt, dt, None,
                                         "alltime", rescaling=resc, growth=growth, drop_adjoint_load=drop)
    g = (beta * c - q * u / resc).reshape(Nt + 1, n)
    w = np.ones(Nt + 1)
    w[0] = w[-1] = 0.5
    dd = dt * sum(w[i] * g[i] @ (M @ dc.reshape(Nt + 1, n)[i]) for i in range(Nt + 1))
    fd = (J(c + eps * dc) - J(c - eps * dc)) / (2 * eps)
    return abs(dd - fd) / abs(fd), dd, fd


def test_gradient_mismatch_no_worse_than_twice_the_growth_free_one(fem):
    """Directional derivative <beta c - q u / rescaling, dc>_Q of the all-time reduced cost with growth (0, 1, -1) against
    a central finite difference (11 x 11, dt = 5e-3, 20 steps, u about 1.5 where r' = -3.75, so |r'| T = 0.375).  The
    bound is twice the mismatch the growth-free oracle shows on the same inputs: the added term has the same first-order
    explicit treatment as the terms already there.

    Measured: growth-free mismatch 1.16e+02 (dd -0.2442, fd -0.00209), with growth 1.21e+02 (dd -0.2410, fd -0.00198).
    The growth-free mismatch is this large because the all-time adjoint adds the raw nodal misfits uhat_n - u_n to
    assembled loads (helpers.py:1506-1507, 1533-1534, reproduced on purpose): the expression is about 1 / (lumped mass)
    times the derivative of the mass-weighted cost.  Leaving the r'(u) p load out moves the directional derivative by
    1 % (-0.2410 -> -0.2385), far inside the bound, so THIS test does not notice a missing adjoint load at any horizon;
    test_constant_states_follow_the_scalar_recursions does (1e-13 against |r'| dt per step)."""
    mesh, asm = fem
    M = asm.mass()
    base, dd0, fd0 = _gradient_mismatch(asm, M, mesh, None)
    grow, dd1, fd1 = _gradient_mismatch(asm, M, mesh, MIMURA)
    drop, dd2, _ = _gradient_mismatch(asm, M, mesh, MIMURA, drop=True)
    print(f"[growth oracle] gradient mismatch: growth-free {base:.3e} (dd {dd0:.6g}, fd {fd0:.6g}), growth {grow:.3e} "
          f"(dd {dd1:.6g}, fd {fd1:.6g}), adjoint load dropped {drop:.3e} (dd {dd2:.6g})")
    assert dd1 != dd2
    assert grow <= 2 * base, (grow, base)
