"""Snapshot tracking on the CPU: ``solvers.Observations`` and the reference loop of snapshots_oracle.py against the
unchanged oracle (no GPU)."""
import importlib

import numpy as np
import pytest

import snapshots_oracle as so
from oracle import traj as otraj
from oracle.assembly import P1Assembler
from oracle.fct import cost_functional
from oracle.mesh import SquareMesh


@pytest.fixture(scope="module")
def Observations():
    return importlib.import_module("fem-fct-pdeco_amd.solvers").Observations


@pytest.fixture(scope="module")
def case():
    """N = 11 nodes per side, eps > 0, 20 steps: a smooth state driven by a smooth control, and a target next to it.  The
    direction dk and the target's offset vanish on the boundary (the reference's gradient drops the boundary term of its
    integration by parts), and the diffusion is strong enough for the limiter to stay nearly inactive on so coarse a mesh."""
    nc, Nt, dt = 10, 20, 5e-3
    mesh = SquareMesh(-1.0, 1.0, nc)
    asm = P1Assembler(mesh)
    n = mesh.nodes
    sb = otraj.SolidBody(asm, om=np.pi / 40, eps=0.2)
    x, y = mesh.x[mesh.dof_to_vertex], mesh.y[mesh.dof_to_vertex]
    t = np.arange(Nt + 1)[:, None] * dt
    ck = (0.8 * np.sin(2 * x)[None] * np.cos(1.5 * y + 3 * t)).ravel()
    bump = (1 - x ** 2) * (1 - y ** 2)
    dk = (bump * np.cos(1.3 * x + 0.4)[None] * np.sin(0.9 * y - 2 * t + 0.3)).ravel()
    u0 = np.exp(-4 * ((x + 0.2) ** 2 + (y - 0.1) ** 2))
    uk = np.zeros((Nt + 1) * n)
    uk[:n] = u0
    otraj.solidbody_forward(sb, ck, uk, n, Nt, dt)
    uhat = 0.85 * uk + 0.05 * np.tile(bump * np.cos(x) * np.cos(y), Nt + 1)
    return dict(mesh=mesh, asm=asm, sb=sb, n=n, Nt=Nt, dt=dt, ck=ck, dk=dk, u0=u0, uk=uk, uhat=uhat, x=x, y=y)


def test_finaltime_corner_has_the_oracles_bits(case, Observations):
    c = case
    n, Nt, dt = c["n"], c["Nt"], c["dt"]
    obs = Observations.finaltime(Nt)
    assert obs.tau == 1.0 and not obs.theta.any()
    uhat = np.full_like(c["uhat"], np.nan)                  # only the last level is read
    uhat[Nt * n:] = c["uhat"][Nt * n:]
    p = so.adjoint(c["sb"], c["ck"], c["uk"], uhat, obs, n, Nt, dt)
    po = otraj.solidbody_adjoint(c["sb"], c["ck"], c["uk"], c["uhat"][Nt * n:], np.zeros_like(p), n, Nt, dt, optim="finaltime")
    assert np.array_equal(p, po)
    J = so.cost(c["sb"], c["uk"], uhat, c["ck"], obs, n, Nt, dt, 0.1)
    Jo = cost_functional(c["uk"], c["uhat"][Nt * n:], c["ck"], Nt, dt, c["sb"].cm.M, 0.1, "finaltime")
    assert abs(J - Jo) <= 4 * np.spacing(Jo)


def test_alltime_corner_has_the_oracles_bits(case, Observations):
    c = case
    n, Nt, dt = c["n"], c["Nt"], c["dt"]
    obs = Observations.alltime(Nt, dt)
    assert obs.tau == 0.0 and np.all(obs.theta[:Nt] == dt) and obs.theta[Nt] == 0.0
    p = so.adjoint(c["sb"], c["ck"], c["uk"], c["uhat"], obs, n, Nt, dt)
    po = otraj.solidbody_adjoint(c["sb"], c["ck"], c["uk"], c["uhat"], np.zeros_like(p), n, Nt, dt, optim="alltime")
    assert np.array_equal(p, po)
    J = so.cost(c["sb"], c["uk"], c["uhat"], c["ck"], obs, n, Nt, dt, 0.1)
    Jo = cost_functional(c["uk"], c["uhat"], c["ck"], Nt, dt, c["sb"].cm.M, 0.1, "alltime")
    assert abs(J - Jo) <= 4 * np.spacing(Jo)


def test_superposition_on_the_low_order_path(case, Observations):
    """For a fixed state and control the low-order adjoint is linear in the misfit: p{k1, k2} = p{k1} + p{k2}.  The bound:
    each p is the result of <= 20 linear solves on O(1) data, the sum of two differs from the joint solve by rounding
    alone -- 1e-12 of the largest entry leaves three orders over what 20 well-conditioned solves lose."""
    c = case
    n, Nt, dt = c["n"], c["Nt"], c["dt"]
    run = lambda lv, w: so.adjoint(c["sb"], c["ck"], c["uk"], c["uhat"], Observations(Nt, lv, w), n, Nt, dt, step="low")
    p12, p1, p2 = run([7, 20], [0.5, 2.0]), run([7], [0.5]), run([20], [2.0])
    assert np.abs(p1).max() > 0 and np.abs(p2).max() > 0
    assert not p1[8 * n:].any()                             # nothing above an interior snapshot
    err = np.abs(p12 - (p1 + p2)).max() / np.abs(p12).max()
    print(f"[snapshots] superposition: {err:.3e}")
    assert err <= 1e-12


def test_window(case, Observations):
    c = case
    n, Nt, dt, asm = c["n"], c["Nt"], c["dt"], c["asm"]
    run = lambda w: so.adjoint(c["sb"], c["ck"], c["uk"], c["uhat"], Observations(Nt, [7, 14, 20], window=w), n, Nt, dt)
    assert np.array_equal(run(np.ones(n)), run(None))       # omega = 1: the bits of no window
    omega = np.where(c["x"] > 0, 1.0, 0.0)
    d = c["uhat"][7 * n:8 * n] - c["uk"][7 * n:8 * n]
    load = so.misfit_load(asm, d, omega)
    M = c["sb"].cm.M
    dark = np.array([not omega[M.indices[M.indptr[i]:M.indptr[i + 1]]].any() for i in range(n)])
    assert dark.any() and not load[dark].any()              # rows whose whole stencil lies where omega = 0
    assert np.abs(load[~dark]).min() >= 0 and np.abs(load).max() > 0
    # the quadrature load is the triple-product matrix applied to the misfit, to rounding (both are exact integrals)
    Mw = so.weighted_mass(asm, omega)
    assert np.abs(Mw @ d - load).max() <= 64 * np.finfo(float).eps * np.abs(load).max()
    assert not (Mw @ d)[dark].any()
    smooth = 0.5 + 0.4 * np.sin(2 * c["x"]) * np.cos(c["y"])
    assert np.abs(so.weighted_mass(asm, smooth) @ d - so.misfit_load(asm, d, smooth)).max() <= 64 * np.finfo(float).eps * np.abs(d).max()
    assert abs(so.weighted_mass(asm, np.ones(n)) - M).max() <= 4 * np.finfo(float).eps * abs(M).max()


def _slope_mismatch(c, obs, h=1e-4):
    """|finite-difference slope of the misfit along dk - <gradient, dk>| / |slope|, the gradient from the adjoint:
    dt sum_n G(p_n, u_n) . d_n with G = assemble(p (b.grad u) v dx), the reference's descent vector without its control
    term (beta = 0: the regularisation is a quadratic whose derivative needs no adjoint)."""
    sb, n, Nt, dt = c["sb"], c["n"], c["Nt"], c["dt"]

    def J(ck):
        uk = np.zeros((Nt + 1) * n)
        uk[:n] = c["u0"]
        otraj.solidbody_forward(sb, ck, uk, n, Nt, dt)
        return so.cost(sb, uk, c["uhat"], ck, obs, n, Nt, dt, 0.0)

    fd = (J(c["ck"] + h * c["dk"]) - J(c["ck"] - h * c["dk"])) / (2 * h)
    p = so.adjoint(sb, c["ck"], c["uk"], c["uhat"], obs, n, Nt, dt)
    g = sum(-otraj.solidbody_descent_rhs(sb, c["ck"], c["uk"], p, 0.0, n, lv) @ c["dk"][lv * n:(lv + 1) * n] for lv in range(Nt + 1))
    return abs(fd - dt * g) / abs(fd), fd, dt * g


def test_directional_derivative(case, Observations):
    """The snapshot gradient is as good as the final-time one on the same case (the limiter and the reference's nodal
    terminal condition make neither exact): mismatch <= 2 x the final-time mismatch.  Without the interior loads
    (theta zeroed, tau kept) the mismatch leaves that bound by far (asked: twice the bound): the test sees a missing load.
    Measured on this case: final-time 6.7e-2, snapshots 5.0e-3, interior loads dropped 5.6e-1."""
    c = case
    Nt = c["Nt"]
    m_fin, *_ = _slope_mismatch(c, Observations.finaltime(Nt))
    obs = Observations(Nt, [7, 14, 20])
    m_snap, fd, g = _slope_mismatch(c, obs)

    class NoLoad:
        theta, tau, window, cost_w, levels = np.zeros(Nt + 1), obs.tau, None, obs.cost_w, obs.levels
    sb, n, dt = c["sb"], c["n"], c["dt"]
    p0 = so.adjoint(sb, c["ck"], c["uk"], c["uhat"], NoLoad, n, Nt, dt)
    g0 = dt * sum(-otraj.solidbody_descent_rhs(sb, c["ck"], c["uk"], p0, 0.0, n, lv) @ c["dk"][lv * n:(lv + 1) * n]
                  for lv in range(Nt + 1))
    m_drop = abs(fd - g0) / abs(fd)
    print(f"[snapshots] slope mismatch: final-time {m_fin:.3e}, snapshots {m_snap:.3e}, interior loads dropped {m_drop:.3e}")
    assert m_snap <= 2 * m_fin
    assert m_drop > 2 * (2 * m_fin)


def test_observations_validation(Observations):
    ok = Observations(10, [2, 5, 10], [1.0, 0.5, 2.0])
    assert ok.tau == 2.0 and ok.theta[2] == 1.0 and ok.theta[5] == 0.5 and ok.theta[10] == 0.0 and ok.theta[0] == 0.0
    assert ok.cost_w[10] == 2.0 and ok.theta.size == 11 and ok.cost_w.sum() == 3.5
    assert Observations(10, [3]).tau == 0.0
    for bad in (dict(levels=[5, 2]), dict(levels=[2, 2]), dict(levels=[0, 3]), dict(levels=[3, 11]), dict(levels=[]),
                dict(levels=[2, 5], weights=[1.0, -1.0]), dict(levels=[2, 5], weights=[1.0]), dict(levels=[2.5]),
                dict(levels=[2], window=[1.0, -0.5, 1.0])):
        with pytest.raises(ValueError):
            Observations(10, **bad)
    with pytest.raises(ValueError):
        Observations(10, [2], window=np.ones(7)).check(10, 9)       # a window of the wrong length
    with pytest.raises(ValueError):
        ok.check(12, 9)
    Observations(10, [2], window=np.ones(9)).check(10, 9)
    a = Observations.alltime(4, 0.1)
    assert np.array_equal(a.cost_w, [0.05, 0.1, 0.1, 0.1, 0.05]) and a.theta[0] == 0.1
