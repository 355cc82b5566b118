"""Projected gradient descent of the reference's refactored PDECO drivers, device resident.

  nonlinear_FCT_PDECO_refactored.py:105-232        "nonlinear"  (one state, final-time misfit)
  Schnak_FCT_PDECO_refactored.py:122-259           "schnak"     (two states, final-time misfit)
  chemotaxis_FCT_PDECO_AT_refactored.py:112-290    "chtxs"      (two states, all-time misfit)

Each problem also runs with the other misfit (``optim=``); "nonlinear" with ``optim="alltime"`` and
``control_per_step=True`` is nonlinear_FCT_PDECO_alltime.py (p(T) = 0, misfit load in every adjoint step).
``optim="snapshots"`` with ``obs=solvers.Observations(...)`` (extension) tracks each state at a few time levels,
optionally on part of the domain: J = 1/2 sum_n w_n ||u_n - uhat_n||^2_Mw [+ the same for v] + beta/2 ||c||^2_Q.

The loop, its constants, the line-search bookkeeping (fail counters, restarts, the control backup)
and the order of the floating-point operations of the pointwise gradient follow the scripts; states,
adjoints, controls and targets stay in HBM and only scalars (costs, norms) reach the host.
``speculative=True`` evaluates all Armijo trial steps s0/2^k of an iteration as one batch of
independent trajectories (helpers.py:1681-1708 picks the first accepted k: same iterate, the states
agree to the solver tolerance) -- the lever that fills the GPU on these small meshes.
``control_per_step=True`` steps the state with the control of the level being computed (the step to
level n+1 reads level n+1), as the reference's all-time scripts do; by default the state solvers
freeze the control at level 1 like helpers.py (see systems.py).
``control_time=solvers.ControlIntervals(...)`` (extension) holds the control constant in time on K intervals: the
pointwise direction is projected onto these controls.  With the default frozen sweep the state depends on one spatial
field only, so the problem posed is a stationary control and K = 1 (``ControlIntervals.stationary``) is its consistent
pairing: the projected direction is the time average of the pointwise expression, the gradient with respect to that one
field, where the free loop moves level 1 by its own slice and every other level by the regularisation alone.
"""
from __future__ import annotations

import time

import numpy as np

from . import _lib
from .mesh import SquareMeshP1
from .systems import (PDESystems, _chtxs_par, _schnak_par, get_nonlinear_eqns_params, split_observations,
                      upload_observations)

DEFAULTS = {
    # nonlinear_FCT_PDECO_refactored.py:49-65
    "nonlinear": dict(optim="finaltime", beta=1e-1, c_lower=-1.0, c_upper=1.0, tol=1e-4, max_iter_armijo=5,
                      max_iter_GD=50, gam=1e-4, s0=1.0, rescaling=1.0, fail_count_max=3, restart_max=5, min_iters=0),
    # Schnak_FCT_PDECO_refactored.py:54-72
    "schnak": dict(optim="finaltime", beta=1e-1, c_lower=0.0, c_upper=10.0, tol=1e-3, max_iter_armijo=10,
                   max_iter_GD=50, gam=1e-4, s0=1.0, rescaling=1.0, fail_count_max=3, restart_max=5, min_iters=0),
    # chemotaxis_FCT_PDECO_AT_refactored.py:55-75, 136-141, 150
    "chtxs": dict(optim="alltime", beta=1e-3, c_lower=0.0, c_upper=20.0, tol=1e-4, max_iter_armijo=20,
                  max_iter_GD=50, gam=1e-5, s0=2.0, rescaling=0.1, fail_count_max=5, restart_max=5, min_iters=2),
}


def rel_err(new, old):
    """helpers.py:69-85"""
    return abs(new - old) / abs(old)


class SystemPDECO:
    """One optimisation problem on one GPU.  ``V``: mesh descriptor (stands in for the dolfin
    FunctionSpace); host vectors are in FEniCS DoF order like the reference's."""

    def __init__(self, problem: str, V: SquareMeshP1, num_steps: int, dt: float, device_id: int = 0, wind=None,
                 wind_scale=None, control_per_step=False, growth=None, obs=None, misfit="mass", par=None,
                 control_time=None, **overrides):
        """``wind`` / ``wind_scale`` (problem "schnak" only): the separable time-dependent wind ``s(t) w0(x)`` of the
        script BASELINE config 3 names (Schnak_FCT_PDECO_alltime.py:55,174-175), see systems.solve_schnak_system.
        ``control_per_step``: the state step to level n+1 reads control level n+1 (the all-time scripts, e.g.
        Schnak_FCT_PDECO_alltime.py:182-191) instead of level 1 for every step (helpers.py:577-578 etc.).
        ``growth=(r0, r1, r2)`` (problem "chtxs" only): cell growth r(u) = u (r0 + r1 u + r2 u^2) in the state and the
        adjoint sweeps (systems.solve_chtxs_system); the gradient expression does not change.
        ``optim="snapshots"`` with ``obs=`` one ``solvers.Observations`` for every state variable, or for the two-variable
        problems a pair ``(obs_u, obs_v)`` one of which may be None (that variable is not observed, its target may be
        None): the targets are trajectories read at the observed levels only.  ``misfit`` (problem "chtxs" only):
        ``"mass"`` (default) loads the adjoint with Mw (hat_n - state_n), the discrete adjoint of the cost, ``"nodal"``
        with the raw nodal misfits of the reference's all-time sweep (systems.solve_adjoint_chtxs_system).
        ``par`` (problem "chtxs" only): ``(delta, Dm, Df, chi, eta)`` in the place of helpers.py:1197-1211's values, e.g.
        those of chemotaxis_mimura_FCT_PGD.py.
        ``control_time`` (a ``solvers.ControlIntervals``): the control is constant in time on its K intervals (see the
        module docstring).  K > 1 needs ``control_per_step=True``: the frozen sweep reads one level only."""
        if problem not in DEFAULTS:
            raise ValueError(f"unknown problem '{problem}' (one of {sorted(DEFAULTS)})")
        if (wind is not None or wind_scale is not None) and problem != "schnak":
            raise ValueError("wind / wind_scale: only the Schnakenberg driver has a time-dependent wind")
        if growth is not None and problem != "chtxs":
            raise ValueError("growth: only the chemotaxis driver has a growth term")
        if par is not None and (problem != "chtxs" or len(par) != 5 or not np.all(np.isfinite(np.asarray(par, dtype=np.float64)))):
            raise ValueError("par: the five finite chemotaxis parameters (delta, Dm, Df, chi, eta), problem 'chtxs' only")
        self.growth = growth
        self.problem, self.V, self.Nt, self.dt = problem, V, int(num_steps), float(dt)
        self.per_step = bool(control_per_step)
        if control_time is not None:
            control_time.check(num_steps)
            if control_time.K > 1 and not self.per_step:
                raise ValueError(f"control_time with K = {control_time.K} intervals needs control_per_step=True: the default "
                                 "state sweep freezes the control at level 1 and reads one level only (K = 1 fits it)")
        self.control_time = control_time
        self.P = dict(DEFAULTS[problem])
        unknown = set(overrides) - set(self.P)
        if unknown:
            raise TypeError(f"unknown option(s) {sorted(unknown)}")
        self.P.update(overrides)
        if self.P["optim"] not in ("alltime", "finaltime", "snapshots"):
            raise ValueError(f"Invalid value for 'optim': '{self.P['optim']}'. Must be one of ['alltime', 'finaltime'].")
        self.snap = self.P["optim"] == "snapshots"
        if misfit not in ("mass", "nodal"):
            raise ValueError(f"Invalid value for 'misfit': '{misfit}'. Must be one of ['mass', 'nodal'].")
        if misfit != "mass" and (problem != "chtxs" or not self.snap):
            raise ValueError("misfit: only the chemotaxis driver with optim='snapshots' has a choice of load")
        if obs is not None and not self.snap:
            raise ValueError("obs: only optim='snapshots' takes observations")
        self.misfit = misfit
        self.obs_pair = split_observations(obs, problem != "nonlinear", num_steps, V.nodes) if self.snap else None
        self.obs_dev, self._obs_arrays = None, []
        self.S = PDESystems(V, device_id=device_id, order=_lib.ORDER_VERTEX)
        self.ctx, self.n = self.S.ctx, self.S.n
        self.tl = (self.Nt + 1) * self.n
        self.v2d = np.asarray(V.vertex_to_dof, dtype=np.int64)
        self.two = problem != "nonlinear"
        if problem == "nonlinear":
            self.eps, _, wind = get_nonlinear_eqns_params()
            self.Aw, self.AwT = self.S.convection(wind, "nonlinear")
        elif problem == "schnak":
            from .systems import _wind_factors
            self.par, wind0 = _schnak_par()
            self.Aw, self.AwT = self.S.convection(wind or wind0, None if wind is not None else "schnak")
            self.wscale = _wind_factors(wind_scale, self.Nt, self.dt)                               # forward: t += dt
            self.wscale_adj = _wind_factors(wind_scale, self.Nt, self.dt, T=self.Nt * self.dt)      # adjoint: t = T; t -= dt
        else:
            self.par = _chtxs_par() if par is None else [float(x) for x in par]
        self._arrays = []
        self._ct_fields = None      # the K fields of a projected direction (control_time)

    # ------------------------------------------------------------------ staging
    def _up(self, x, count=None):
        x = np.asarray(x, dtype=np.float64).ravel()
        d = self.ctx.array(np.ascontiguousarray(x.reshape(-1, self.n)[:, self.v2d]).ravel())
        self._arrays.append(d)
        return d

    def _zeros(self, count):
        d = self.ctx.zeros(count)
        self._arrays.append(d)
        return d

    def _down(self, d, count=None, off=0):
        count = d.count if count is None else count
        tmp = self.ctx.empty(count)
        try:
            tmp.copy_from(d, count, src_off=off)
            h = tmp.download().reshape(-1, self.n)
        finally:
            tmp.free()
        out = np.empty_like(h)
        out[:, self.v2d] = h
        return out.ravel()

    def close(self):
        for a in self._arrays + self._obs_arrays:
            a.free()
        self._arrays, self._obs_arrays, self.obs_dev = [], [], None
        self.S.close()

    def _obs(self):
        """the observations on the device, uploaded once (window in the device's DoF order, cost weights per variable)"""
        if self.obs_dev is None:
            up = lambda w: self.ctx.array(np.ascontiguousarray(np.asarray(w, dtype=np.float64)[self.v2d]))
            self.obs_dev, self._obs_arrays = upload_observations(self.ctx, self.obs_pair, up)
            self.cost_w = [None if o is None else self.ctx.array(o.cost_w) for o in self.obs_pair[:2]]
            self._obs_arrays += [a for a in self.cost_w if a is not None]
        return self.obs_dev

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ------------------------------------------------------------------ solves (batch of B trajectories)
    def _state(self, c, u, v, clev, B):
        """solve_<problem>(c, u, v): the control is frozen at time level 1 (helpers.py:577-578 etc.), or with
        ``control_per_step`` the B control trajectories (stride tl) are read level by level (clev unused)"""
        n, tl = self.n, self.tl
        if self.per_step:
            if self.problem == "nonlinear":
                self.ctx.nonlinear_forward_ct(self.Aw, c, u, self.Nt, self.dt, self.eps, batch=B)
            elif self.problem == "schnak":
                self.ctx.schnak_forward_ct(self.Aw, c, u, v, self.Nt, self.dt, self.par, 1.0, batch=B,
                                           wind_scale=self.wscale)
            else:
                self.ctx.chtxs_forward_ct(c, u, v, self.Nt, self.dt, self.par, 0.1, batch=B, growth=self.growth)
            return
        for b in range(B):
            clev.copy_from(c, n, dst_off=b * n, src_off=b * tl + n)
        if self.problem == "nonlinear":
            self.ctx.nonlinear_forward(self.Aw, clev, u, self.Nt, self.dt, self.eps, batch=B)
        elif self.problem == "schnak":
            # the drivers and armijo_line_search_ref call the state solver without `rescaling`
            # (helpers.py:1685): its defaults apply, 1 (helpers.py:512) and 1/10 (helpers.py:1252)
            self.ctx.schnak_forward(self.Aw, clev, u, v, self.Nt, self.dt, self.par, 1.0, batch=B, wind_scale=self.wscale)
        else:
            self.ctx.chtxs_forward(clev, u, v, self.Nt, self.dt, self.par, 0.1, batch=B, growth=self.growth)

    def _adjoint(self, u, v, p, q, c, tg):
        obs = self._obs() if self.snap else None
        if self.problem == "nonlinear":
            self.ctx.nonlinear_adjoint(self.Aw, u, tg[0], p, self.Nt, self.dt, self.eps,
                                       alltime=self.P["optim"] == "alltime", obs=obs)
        elif self.problem == "schnak":
            self.ctx.schnak_adjoint(self.AwT, u, v, tg[0], tg[1], p, q, self.Nt, self.dt, self.par,
                                    alltime=self.P["optim"] == "alltime", wind_scale=self.wscale_adj, obs=obs)
        else:
            self.ctx.chtxs_adjoint(u, v, tg[0], tg[1], p, q, c, self.Nt, self.dt, self.par, self.P["rescaling"],
                                   self.P["optim"] == "alltime", growth=self.growth, obs=obs, misfit=self.misfit)

    def _cost(self, u, v, c, tg, B=1):
        if self.snap:       # the tracking term per observed variable, then the control term, every member in one call each
            obs = self._obs()
            J = 0.0
            for x, t, w in ((u, tg[0], self.cost_w[0]), (v, tg[1] if self.two else None, self.cost_w[1])):
                if w is not None:
                    J = J + self.ctx.obs_cost(x, t, w, self.Nt, obs.window, batch=B)
            return J + self.P["beta"] / 2 * self.ctx.l2_norm_sq_Q(c, None, self.Nt, self.dt, batch=B)
        return self.ctx.cost_functional(u, tg[0], c, self.Nt, self.dt, self.P["beta"], self.P["optim"],
                                        var2=v if self.two else None, var2_target=tg[1] if self.two else None, batch=B)

    def _descent(self, c, u, p, q, d):
        beta, r = self.P["beta"], self.P["rescaling"]
        if self.problem == "nonlinear":
            self.ctx.descent_pointwise(self.tl, beta, c, p, d)                       # -(beta*ck - pk)
        elif self.problem == "schnak":
            self.ctx.descent_pointwise(self.tl, beta, c, p, d, scale=self.par[3] / r)   # -(beta*ck - gamma/r*pk)
        else:
            self.ctx.descent_pointwise(self.tl, beta, c, q, d, y=u, divisor=r)       # -(beta*ck - qk*uk/r)
        ct = self.control_time
        if ct is not None:      # the start control is 0, so every iterate clip(c + s P d) is constant on the intervals
            if self._ct_fields is None:
                self._ct_fields = self.ctx.empty(ct.K * self.n)
            self.ctx.time_project(d, ct.starts, self.Nt, self._ct_fields)

    # ------------------------------------------------------------------ the loop
    def run(self, ic, targets, speculative=True, callback=None):
        """ic = (u0,) / (u0, v0); targets = (uhat,) / (uhat, vhat): final-time vectors (n) or trajectories
        ((Nt+1)*n) according to ``optim`` (``"snapshots"``: trajectories, read at the observed levels only -- the rest
        may hold anything, NaN included; None for a variable that is not observed).  Returns a dict: final u, v, p, q, c (NumPy, FEniCS order),
        ``cost`` (initial value first), ``armijo_its``, ``stop_crit``, ``it``, ``restored``."""
        P, ctx, n, tl, Nt, dt = self.P, self.ctx, self.n, self.tl, self.Nt, self.dt
        K = int(P["max_iter_armijo"])
        B = K if speculative else 1
        tsz = tl if P["optim"] != "finaltime" else n
        if len(ic) != (2 if self.two else 1) or len(targets) != len(ic):
            raise ValueError("ic / targets: one entry per state variable")
        if self.snap:       # a variable that is not observed has no target
            targets = [t if o is not None else None for t, o in zip(targets, self.obs_pair[:2])]
        for t in targets:
            if self.snap and t is None:
                continue
            if t is None or np.asarray(t).size != tsz:
                raise ValueError(f"target of {0 if t is None else np.asarray(t).size} values, expected {tsz} for optim='{P['optim']}'")

        def replicate(one, count, reps):
            """reps copies of a device vector, made on the device"""
            d = self._zeros(reps * count)
            for b in range(reps):
                d.copy_from(one, count, dst_off=b * count)
            return d

        def traj0(x0, reps=1):
            a = np.zeros(tl)
            a[:n] = np.asarray(x0, dtype=np.float64)
            one = self._up(a)
            return one if reps == 1 else replicate(one, tl, reps)

        u = traj0(ic[0])
        v = traj0(ic[1]) if self.two else None
        p = self._zeros(tl)
        q = self._zeros(tl) if self.two else None
        c, d, cbak = self._zeros(tl), self._zeros(tl), self._zeros(tl)
        tg = [None if t is None else self._up(t) for t in targets]
        clev = None if self.per_step else self._zeros(B * n)
        uB = traj0(ic[0], B)
        vB = traj0(ic[1], B) if self.two else None
        cB = self._zeros(B * tl)
        if speculative:
            ckB = self._zeros(B * tl)
            tgB = [None if t is None else replicate(t, tsz, B) for t in tg]
        else:
            ckB, tgB = c, tg

        self._state(c, u, v, clev, 1)
        self._adjoint(u, v, p, q, c, tg)
        cost_old = float(self._cost(u, v, c, tg)[0])
        cost_new = (2 + P["tol"]) * cost_old
        stop_crit = rel_err(cost_new, cost_old)
        it = fail_count = fail_restart_count = 0
        fail_pass = False
        it_backup = 0
        # armijo_margin[it][k]: distance of trial k's Armijo test from its threshold relative to the cost,
        # (J_trial - J_k + gam/s ||c_inc - c||^2_Q) / |J_k| (> 0: rejected), for the trials the sequential search looks at
        # wall[it]: host clock after iteration it's cost evaluation (a read-back: the device has finished the iteration);
        # wall0: after the initial state + adjoint + cost -- so (wall[-1] - wall0) / it is the time of an iteration proper
        hist = dict(cost=[cost_old], armijo_its=[], stop_crit=[], armijo_margin=[], wall=[], wall0=time.perf_counter())
        svals = [P["s0"] / 2 ** k for k in range(K)]
        while (stop_crit >= P["tol"] or fail_pass or it < P["min_iters"]) and it < P["max_iter_GD"]:
            self._descent(c, u, p, q, d)
            # armijo_line_search_ref, helpers.py:1681-1713
            if speculative:
                for k, s in enumerate(svals):
                    ctx.project_control(c, s, d, P["c_lower"], P["c_upper"], cB.ptr + 8 * k * tl, tl)
                    ckB.copy_from(c, tl, dst_off=k * tl)
                self._state(cB, uB, vB, clev, B)
                J = self._cost(uB, vB, cB, tgB, B)
                dif = ctx.l2_norm_sq_Q(cB, ckB, Nt, dt, batch=B)
                acc = K - 1
                margins = []
                for k, s in enumerate(svals):
                    margins.append((float(J[k]) - cost_old + P["gam"] / s * float(dif[k])) / abs(cost_old))
                    if J[k] - cost_old <= -P["gam"] / s * dif[k]:
                        acc = k
                        break
            else:
                acc = K - 1
                margins = []
                for k, s in enumerate(svals):
                    ctx.project_control(c, s, d, P["c_lower"], P["c_upper"], cB, tl)
                    self._state(cB, uB, vB, clev, 1)
                    Jk = float(self._cost(uB, vB, cB, tg)[0])
                    dif = float(ctx.l2_norm_sq_Q(cB, c, Nt, dt)[0])
                    margins.append((Jk - cost_old + P["gam"] / s * dif) / abs(cost_old))
                    if Jk - cost_old <= -P["gam"] / s * dif:
                        acc = k
                        break
            hist["armijo_margin"].append(margins)
            slot = acc if speculative else 0
            c.copy_from(cB, tl, src_off=slot * tl)
            u.copy_from(uB, tl, src_off=slot * tl)
            if self.two:
                v.copy_from(vB, tl, src_off=slot * tl)
            iters = acc + 1
            self._adjoint(u, v, p, q, c, tg)
            # line-search bookkeeping (e.g. Schnak_FCT_PDECO_refactored.py:180-215)
            if iters == K:
                fail_count += 1
                fail_pass = True
                if it == 0:
                    cbak.copy_from(c, tl)
                    it_backup = it
                if fail_count == P["fail_count_max"]:
                    break
            else:
                if fail_count > 0:
                    fail_count = 0
                    fail_restart_count += 1
                    fail_pass = False
                if fail_restart_count < P["restart_max"]:
                    cbak.copy_from(c, tl)
                    it_backup = it
                elif fail_restart_count == P["restart_max"]:
                    break
            cost_new = float(self._cost(u, v, c, tg)[0])
            stop_crit = rel_err(cost_new, cost_old)
            hist["cost"].append(cost_new)
            hist["armijo_its"].append(iters)
            hist["stop_crit"].append(stop_crit)
            hist["wall"].append(time.perf_counter())
            if callback is not None:
                callback(it, cost_new, iters, stop_crit)
            it += 1
            cost_old = cost_new
        restored = False
        if fail_count == P["fail_count_max"] or fail_restart_count == P["restart_max"] or \
                (it == P["max_iter_GD"] and fail_count > 0):
            # the scripts' state/adjoint "backups" alias the live arrays: only the control is restored
            c.copy_from(cbak, tl)
            restored = True
        out = dict(u=self._down(u), v=self._down(v) if self.two else None, p=self._down(p),
                   q=self._down(q) if self.two else None, c=self._down(c), it=it, it_backup=it_backup,
                   restored=restored, **hist)
        for a in self._arrays:
            a.free()
        self._arrays = []
        return out


def projected_gradient_descent(problem, V, ic, targets, num_steps, dt, speculative=True, device_id=0, wind=None,
                               wind_scale=None, control_per_step=False, growth=None, obs=None, misfit="mass", par=None,
                               control_time=None, **overrides):
    """One call = one run of the refactored driver ``problem`` (see module docstring)."""
    with SystemPDECO(problem, V, num_steps, dt, device_id=device_id, wind=wind, wind_scale=wind_scale,
                     control_per_step=control_per_step, growth=growth, obs=obs, misfit=misfit, par=par,
                     control_time=control_time, **overrides) as prob:
        return prob.run(ic, targets, speculative=speculative)
