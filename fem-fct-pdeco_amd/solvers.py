"""Trajectory solvers: forward and adjoint sweeps resident on the GPU.

Mirrors the time loops the reference writes in Python around ``FCT_alg[_ref]``
(one host<->device crossing per sweep instead of ~10 per time step):

  solid-body rotation + drift control (inline loops of the advection scripts)
      forward   advection_solidbody_FCT_PDECO_finaltime.py:175-193
      adjoint   advection_solidbody_FCT_PDECO_finaltime.py:200-221,
                advection_solidbody_FCT_PDECO_alltime.py:232-259
      gradient  advection_solidbody_FCT_PDECO_finaltime.py:228-238
      Armijo    advection_solidbody_FCT_PDECO_finaltime_Garvie.py:259-317

  linear advection-diffusion + distributed source control (pgd_source_control)
      loop      advection_FCT_PDECO_alltime_exact.py:212-330, advection_FCT_PDECO_finaltime.py:170-280
      errors    advection_FCT_PDECO_alltime_exact.py:333-440
      reaction  advection_FCT_PDECO_finaltime_exact.py (LinearReactionSourceControl, finaltime_exact_fields)

NumPy-facing methods take/return ``(num_steps+1)*nodes`` float64 arrays in FEniCS
DoF order, mutate the state array in place *and* return it, like the reference.
"""
from __future__ import annotations

import time

import numpy as np

from . import _lib
from .device import Context, DeviceArray, dptr
from .mesh import SquareMeshP1


def rotation_wind(om):
    """``1/om * Expression(('-x[1]','x[0]'))`` (advection_solidbody_FCT_PDECO_finaltime.py:91-93)."""
    return lambda x, y: (-(1.0 / om) * y, (1.0 / om) * x)


OPTIMS = ("alltime", "finaltime", "snapshots")


class Observations:
    """Observations of a state at chosen time levels, the tracking term

        J = 1/2 sum_n w_n (u_n - uhat_n)^T Mw (u_n - uhat_n),      Mw = assemble(omega_h*u*v*dx)  (M without a window)

    ``levels``: strictly increasing integer time levels in 1..num_steps; ``weights``: one w_n >= 0 per level (default 1);
    ``window``: nodal values omega >= 0 of a P1 field in the problem's DoF order that restricts or weights the observed
    part of the domain (None: omega = 1).  Derived, as the adjoint sweep and the cost take them:

        theta[n]   weight of level n < num_steps, 0 elsewhere (num_steps + 1 values): the step to level n is loaded with
                   (theta[n]/dt) Mw (uhat_n - u_n), the discrete adjoint of the backward-Euler step for J
        tau        weight of level num_steps (0 if not observed): p_Nt = tau * omega .* (uhat_Nt - u_Nt), nodal as the
                   reference's terminal condition
        cost_w[n]  the weights including level num_steps

    The reference's two modes are :meth:`finaltime` and :meth:`alltime`."""

    def __init__(self, num_steps, levels, weights=None, window=None):
        Nt = int(num_steps)
        if Nt < 1:
            raise ValueError(f"num_steps = {num_steps}: must be >= 1")
        lv = np.asarray(levels)
        if lv.ndim != 1 or lv.size == 0:
            raise ValueError("no observed levels")
        if not np.all(lv == np.floor(lv)):
            raise ValueError("levels must be integers")
        lv = lv.astype(np.int64)
        if lv.min() < 1 or lv.max() > Nt:
            raise ValueError(f"levels must lie in 1..num_steps = {Nt}")
        if np.any(np.diff(lv) <= 0):
            raise ValueError("levels must be strictly increasing (sorted, no duplicates)")
        w = np.ones(lv.size) if weights is None else np.asarray(weights, dtype=np.float64).ravel()
        if w.size != lv.size:
            raise ValueError(f"{w.size} weights for {lv.size} levels")
        if not np.all(w >= 0):
            raise ValueError("weights must be >= 0")
        cost_w = np.zeros(Nt + 1)
        cost_w[lv] = w
        theta = cost_w.copy()
        theta[Nt] = 0.0
        self._set(Nt, lv, theta, float(cost_w[Nt]), cost_w, window)

    def _set(self, Nt, levels, theta, tau, cost_w, window):
        if window is not None:
            window = np.array(window, dtype=np.float64).ravel()
            if not np.all(window >= 0):
                raise ValueError("window must be >= 0 everywhere")
            window.setflags(write=False)
        self.num_steps, self.levels, self.theta, self.tau, self.cost_w, self.window = Nt, levels, theta, tau, cost_w, window
        for a in (levels, theta, cost_w):
            a.setflags(write=False)

    @classmethod
    def finaltime(cls, num_steps, window=None):
        """The final-time mode: tau = 1, theta = 0."""
        return cls(num_steps, [int(num_steps)], window=window)

    @classmethod
    def alltime(cls, num_steps, dt, window=None):
        """The all-time mode: tau = 0 and theta[n] = dt at every level n < num_steps, level 0 included (the reference's
        sweep loads it); the cost weights are the trapezoid of L2_norm_sq_Q (helpers.py:330-360)."""
        Nt = int(num_steps)
        if Nt < 1 or not dt > 0:
            raise ValueError("num_steps >= 1 and dt > 0 are required")
        theta = np.full(Nt + 1, float(dt))
        theta[Nt] = 0.0
        cost_w = np.full(Nt + 1, float(dt))
        cost_w[0] = cost_w[Nt] = 0.5 * dt
        self = cls.__new__(cls)
        self._set(Nt, np.arange(0, Nt + 1), theta, 0.0, cost_w, window)
        return self

    def check(self, num_steps, nodes):
        """Raises ValueError unless these observations fit a problem of ``num_steps`` steps and ``nodes`` DoFs."""
        if self.num_steps != int(num_steps):
            raise ValueError(f"observations of {self.num_steps} steps for a problem of {num_steps}")
        if self.window is not None and self.window.size != int(nodes):
            raise ValueError(f"window of {self.window.size} values, expected {nodes}")
        return self


class StateBounds:
    """Bounds lower <= u_n <= upper on the state as a Moreau-Yosida penalty (an extension: the reference has none),

        v_n = u_n - clip(u_n, lower, upper)              the nodal violation, signed
        P(u) = gamma/2 sum_n sigma_n sum_i ml_i omega_i v_{n,i}^2,      J_gamma = J + P

    with the lumped mass ml (the max acts node by node; the choice of the sparse controls' ||c||_{1,h}).  ``lower`` /
    ``upper``: a scalar or n nodal values in the problem's DoF order, +-inf allowed, None: no bound on that side;
    ``gamma`` >= 0; ``levels``: strictly increasing time levels in 1..num_steps (default: all of them; level 0 is the
    fixed initial condition); ``weights``: one sigma_n >= 0 per level (default: the problem's dt); ``window``: nodal
    omega >= 0 (None: 1).  Derived for a problem with time step dt, as the sweep and the cost take them:

        sigma(dt)   num_steps + 1 level weights, sigma[0] = 0: the step to level n < num_steps is loaded with
                    -(sigma[n]/dt) gamma ml .* omega .* v_n on top of the tracking load
        tau_s(dt)   sigma[num_steps]: p_Nt gets -tau_s gamma omega .* v_Nt, nodal as the tracking terminal condition
        cost_w(dt)  the weights of P, = sigma

    :meth:`with_gamma` gives the same bounds with another gamma (continuation)."""

    def __init__(self, num_steps, lower=None, upper=None, gamma=1.0, levels=None, weights=None, window=None):
        Nt = int(num_steps)
        if Nt < 1:
            raise ValueError(f"num_steps = {num_steps}: must be >= 1")
        if lower is None and upper is None:
            raise ValueError("no bound: lower and upper are both None")
        lo = None if lower is None else np.array(lower, dtype=np.float64).ravel()
        hi = None if upper is None else np.array(upper, dtype=np.float64).ravel()
        for name, b in (("lower", lo), ("upper", hi)):
            if b is not None and (b.size == 0 or np.isnan(b).any()):
                raise ValueError(f"{name} is empty or holds NaN")
        if lo is not None and hi is not None:
            if lo.size != hi.size and 1 not in (lo.size, hi.size):
                raise ValueError(f"lower of {lo.size} values, upper of {hi.size}")
            if np.any(lo > hi):
                raise ValueError("lower > upper")
        lv = np.arange(1, Nt + 1) if levels is None else np.asarray(levels)
        if lv.ndim != 1 or lv.size == 0:
            raise ValueError("no penalised levels")
        if not np.all(lv == np.floor(lv)):
            raise ValueError("levels must be integers")
        lv = lv.astype(np.int64)
        if lv.min() < 1 or lv.max() > Nt:
            raise ValueError(f"levels must lie in 1..num_steps = {Nt}")
        if np.any(np.diff(lv) <= 0):
            raise ValueError("levels must be strictly increasing (sorted, no duplicates)")
        w = np.ones(lv.size) if weights is None else np.asarray(weights, dtype=np.float64).ravel()
        if w.size != lv.size:
            raise ValueError(f"{w.size} weights for {lv.size} levels")
        if not np.all(w >= 0):
            raise ValueError("weights must be >= 0")
        if window is not None:
            window = np.array(window, dtype=np.float64).ravel()
            if not np.all(window >= 0):
                raise ValueError("window must be >= 0 everywhere")
        level_w = np.zeros(Nt + 1)
        level_w[lv] = w
        self.num_steps, self.levels, self.lower, self.upper, self.window = Nt, lv, lo, hi, window
        self._level_w, self._per_dt = level_w, weights is None
        for a in (lv, lo, hi, window, level_w):
            if a is not None:
                a.setflags(write=False)
        self._fields = object()         # what the device copies hang on: shared by the with_gamma() variants
        self._set_gamma(gamma)

    def _set_gamma(self, gamma):
        g = float(gamma)
        if not (g >= 0 and np.isfinite(g)):
            raise ValueError(f"gamma = {gamma}: must be finite and >= 0")
        self.gamma = g

    def with_gamma(self, gamma):
        """The same bounds, levels, weights and window with another penalty weight."""
        other = StateBounds.__new__(StateBounds)
        other.__dict__.update(self.__dict__)
        other._set_gamma(gamma)
        return other

    def sigma(self, dt):
        return self._level_w * float(dt) if self._per_dt else self._level_w

    def tau_s(self, dt):
        return float(self.sigma(dt)[self.num_steps])

    def cost_w(self, dt):
        return self.sigma(dt)

    def nodal(self, nodes):
        """``(lower, upper, window)`` as ``nodes`` values each (scalars spread out), None where absent."""
        spread = lambda b: None if b is None else (np.full(int(nodes), b[0]) if b.size == 1 else b)
        return spread(self.lower), spread(self.upper), self.window

    def pairs(self, nodes, dt):
        """the number of penalised (level, node) pairs: sigma_n != 0 and omega_i != 0"""
        return int(np.count_nonzero(self.sigma(dt))) * (int(nodes) if self.window is None else int(np.count_nonzero(self.window)))

    def check(self, num_steps, nodes):
        """Raises ValueError unless these bounds fit a problem of ``num_steps`` steps and ``nodes`` DoFs."""
        if self.num_steps != int(num_steps):
            raise ValueError(f"state bounds of {self.num_steps} steps for a problem of {num_steps}")
        for name, b in (("lower", self.lower), ("upper", self.upper)):
            if b is not None and b.size not in (1, int(nodes)):
                raise ValueError(f"{name} of {b.size} values, expected 1 or {nodes}")
        if self.window is not None and self.window.size != int(nodes):
            raise ValueError(f"window of {self.window.size} values, expected {nodes}")
        return self


class Smoothness:
    """H1 regularisation of a control trajectory c = (c_0 .. c_Nt) in space and time, on top of beta/2 ||c||^2_Q:

        R(c) = beta_x/2 R_x + beta_t/2 R_t
        R_x  = dt sum_{l=0..Nt} w_l c_l^T Ad c_l                          (the trapezoid's w, Ad = assemble(grad u . grad v dx))
        R_t  = 1/dt sum_{l<Nt} (c_{l+1} - c_l)^T M (c_{l+1} - c_l)        (M the consistent mass of ``l2_norm_sq_Q``)

    the discrete beta_x/2 int int |grad c|^2 + beta_t/2 int int (dc/dt)^2.  Its gradient in the inner product of
    ``l2_norm_sq_Q`` has the per-level form of beta M c_l, M g_l = beta_x Ad c_l + beta_t M tau_l with the three-point
    time stencil tau (``femfct_smooth_rhs``), so a direction stays one mass solve per level.  Both coefficients finite
    and >= 0; ``Smoothness(0, 0)`` leaves every iterate as it is and only records the roughness."""

    def __init__(self, beta_x=0.0, beta_t=0.0):
        self.beta_x, self.beta_t = float(beta_x), float(beta_t)
        for name, b in (("beta_x", self.beta_x), ("beta_t", self.beta_t)):
            if not (np.isfinite(b) and b >= 0.0):
                raise ValueError(f"{name} = {b}: must be finite and >= 0")

    @property
    def active(self):
        return self.beta_x != 0.0 or self.beta_t != 0.0

    def value(self, Rx, Rt):
        """R = beta_x/2 Rx + beta_t/2 Rt"""
        return self.beta_x / 2 * Rx + self.beta_t / 2 * Rt


def _need_obs(optim, obs):
    if optim not in OPTIMS:
        raise ValueError(f"Invalid value for 'optim': '{optim}'. Must be one of {list(OPTIMS)}.")
    if optim == "snapshots" and not isinstance(obs, Observations):
        raise ValueError("optim='snapshots' needs obs=Observations(...)")
    return optim == "snapshots"


class ControlIntervals:
    """Controls that are piecewise constant in time: K intervals of time levels, interval k = the levels
    ``starts[k] <= l < starts[k+1]`` (K + 1 increasing integers, ``starts[0] = 0``, ``starts[K] = num_steps + 1``).

    Passed as ``control_time=`` to a projected-gradient loop, the descent direction is projected onto these controls,
    d <- P d with P = prolong o restrict,

        restrict(x)[k] = (sum_{l in k} w_l x_l) / W_k,   W_k = sum_{l in k} w_l,      prolong(y)[l] = y[k(l)]

    and the trapezoid's level weights w_l = 1, w_0 = w_Nt = 1/2 (dt cancels).  P is the orthogonal projection in the
    discrete L2(Q) inner product of the cost and the Armijo distance (L2_norm_sq_Q), so P d is the steepest descent
    direction among the piecewise-constant controls; and with a start control in that subspace every iterate
    clip(c + s P d) stays in it bit for bit, so the sweeps, costs and trial kernels are the free loop's.  K = 1
    (:meth:`stationary`) is a time-independent control: parameter identification, and the problem the default forward
    sweeps of the PDE systems pose, which freeze the control at level 1.  K = num_steps + 1 (:meth:`identity`) is the
    free space-time control.  The loops return the control as a full trajectory; :meth:`compact` gives its K fields."""

    def __init__(self, num_steps, starts):
        Nt = int(num_steps)
        if Nt < 1:
            raise ValueError(f"num_steps = {num_steps}: must be >= 1")
        st = np.asarray(starts)
        if st.ndim != 1 or st.size < 2:
            raise ValueError("starts: K + 1 >= 2 interval boundaries are needed")
        if not np.all(st == np.floor(st)):
            raise ValueError("starts must be integers")
        st = st.astype(np.int64)
        if st[0] != 0 or st[-1] != Nt + 1:
            raise ValueError(f"starts must begin at 0 and end at num_steps + 1 = {Nt + 1}")
        if np.any(np.diff(st) <= 0):
            raise ValueError("starts must be strictly increasing")
        w = np.ones(Nt + 1)
        w[0] = w[Nt] = 0.5
        self.num_steps, self.K = Nt, st.size - 1
        self.starts = st.astype(np.int32)
        self.level_weights = w
        self.interval_weights = np.add.reduceat(w, st[:-1])
        self.interval_of_level = np.repeat(np.arange(self.K), np.diff(st))
        for a in (self.starts, self.level_weights, self.interval_weights, self.interval_of_level):
            a.setflags(write=False)

    @classmethod
    def stationary(cls, num_steps):
        """One interval: a control that does not depend on time."""
        return cls(num_steps, [0, int(num_steps) + 1])

    @classmethod
    def every(cls, num_steps, stride):
        """Intervals of ``stride`` levels from level 0 on (the last one takes what is left)."""
        stride = int(stride)
        if stride < 1:
            raise ValueError(f"stride = {stride}: must be >= 1")
        return cls(num_steps, list(range(0, int(num_steps) + 1, stride)) + [int(num_steps) + 1])

    @classmethod
    def identity(cls, num_steps):
        """One interval per level: the free space-time control (the projection returns its input bit for bit)."""
        return cls(num_steps, np.arange(int(num_steps) + 2))

    def check(self, num_steps):
        """Raises ValueError unless these intervals partition the levels of a problem of ``num_steps`` steps."""
        if self.num_steps != int(num_steps):
            raise ValueError(f"control intervals of {self.num_steps} steps for a problem of {num_steps}")
        return self

    def _levels(self, c, n):
        c = np.asarray(c, dtype=np.float64)
        if c.size != (self.num_steps + 1) * int(n):
            raise ValueError(f"control of {c.size} values, expected (num_steps + 1) * n = {(self.num_steps + 1) * int(n)}")
        return c.reshape(self.num_steps + 1, int(n))

    def compact(self, c, n):
        """The K fields of a control trajectory, a (K, n) array: ``restrict`` (for a control that is constant on the
        intervals, its values there up to rounding; exactly so on an interval of one level)."""
        x = self._levels(c, n) * self.level_weights[:, None]
        return np.add.reduceat(x, self.starts[:-1].astype(np.int64), axis=0) / self.interval_weights[:, None]

    def expand(self, ck):
        """The (num_steps + 1) * n trajectory that holds the K fields ``ck`` (K, n) over their intervals."""
        ck = np.asarray(ck, dtype=np.float64)
        if ck.ndim != 2 or ck.shape[0] != self.K:
            raise ValueError(f"fields of shape {ck.shape}, expected ({self.K}, n)")
        return np.ascontiguousarray(ck[self.interval_of_level]).ravel()

    def contains(self, c, n):
        """True when the control trajectory ``c`` is constant on every interval, exactly."""
        x = self._levels(c, n)
        return bool(np.array_equal(x, x[self.starts[:-1].astype(np.int64)][self.interval_of_level]))

    def need(self, c, n, num_steps):
        """The loops' entry check: the intervals fit the problem and the start control ``c`` lies in the subspace."""
        self.check(num_steps)
        if not self.contains(c, n):
            raise ValueError("c0 is not constant in time on the control intervals (control_time): project it first, e.g. "
                             "control_time.expand(control_time.compact(c0, n))")
        return self


class ControlZones:
    """Controls that are piecewise constant in space: ``labels`` holds one integer per mesh node in the problem's DoF
    order, ``-1`` where no control acts and ``0 .. m-1`` for the node's zone (every zone non-empty, 1 <= m <= 256).

    Passed as ``control_space=`` to a descent loop, the direction of every time level lies in span{chi_j}, chi_j the P1
    function that is 1 on the nodes of zone j and 0 on all others: it is the steepest-descent direction among these
    controls in the mass inner product,

        d = chi G^-1 chi^T r      (drift control: r the dual right-hand side -(beta M c + G_l); no mass solve)
        d = chi G^-1 chi^T M d    (source control: the orthogonal projection P of the primal direction)

    with G = chi^T M chi (m x m, SPD).  d is exactly 0.0 where the label is -1, so the control keeps clip(c0) there, and
    every node of a zone receives the same stored value: with scalar bounds and a start control that is constant on every
    zone each iterate clip(c + s d) stays so bit for bit, and the sweeps, costs and trial kernels are the free loop's.
    The loops return the control as a full trajectory; :meth:`compact` gives its ``(levels, m)`` amplitudes."""

    def __init__(self, labels):
        lab = np.asarray(labels)
        if lab.ndim != 1 or lab.size < 1:
            raise ValueError("labels: one integer per node is needed")
        if not np.issubdtype(lab.dtype, np.number) or not np.all(lab == np.floor(lab)):
            raise ValueError("labels must be integers")
        lab = lab.astype(np.int64)
        if lab.min() < -1:
            raise ValueError(f"labels must be -1 (no control) or a zone 0 .. m-1, got {int(lab.min())}")
        m = int(lab.max()) + 1
        if not 1 <= m <= _lib.MAX_ZONES:
            raise ValueError(f"m = {m} zones: must be in 1..{_lib.MAX_ZONES}")
        sizes = np.bincount(lab[lab >= 0], minlength=m)
        if np.any(sizes == 0):
            raise ValueError(f"zone {int(np.argmin(sizes))} is empty: the labels must use every zone 0 .. {m - 1}")
        self.n, self.m = lab.size, m
        self.labels = lab.astype(np.int32)
        self.sizes = sizes
        self.active = lab >= 0
        self.first = np.array([int(np.argmax(lab == j)) for j in range(m)])       # first node of every zone
        for a in (self.labels, self.sizes, self.active, self.first):
            a.setflags(write=False)

    @classmethod
    def single(cls, n):
        """One zone of all ``n`` nodes: a control that depends on time only."""
        return cls(np.zeros(int(n), dtype=np.int32))

    @classmethod
    def blocks(cls, mesh: SquareMeshP1, bx, by, margin=0, order=_lib.ORDER_FENICS):
        """A ``bx`` x ``by`` grid of rectangles over the square (zone ``jy * bx + jx``); the nodes within ``margin`` node
        rows of the boundary get -1.  The labels are in the DoF order ``order`` of the problem they are meant for."""
        bx, by, margin, N = int(bx), int(by), int(margin), mesh.N
        inner = N - 2 * margin
        if margin < 0 or bx < 1 or by < 1 or max(bx, by) > inner:
            raise ValueError(f"blocks: {bx} x {by} blocks do not fit the {inner} x {inner} nodes inside margin = {margin}")
        iy, ix = np.divmod(np.arange(mesh.nodes), N)
        inside = (ix >= margin) & (ix < N - margin) & (iy >= margin) & (iy < N - margin)
        lab = np.where(inside, ((iy - margin) * by // inner) * bx + (ix - margin) * bx // inner, -1)
        if order != _lib.ORDER_VERTEX:
            dof = np.empty_like(lab)
            dof[mesh.vertex_to_dof] = lab
            lab = dof
        return cls(lab)

    def check(self, n):
        """Raises ValueError unless the labels are those of a problem of ``n`` nodes."""
        if self.n != int(n):
            raise ValueError(f"control zones of {self.n} nodes for a problem of {n}")
        return self

    def _levels(self, c, n):
        self.check(n)
        c = np.asarray(c, dtype=np.float64)
        if c.size == 0 or c.size % self.n:
            raise ValueError(f"control of {c.size} values, expected a multiple of n = {self.n}")
        return c.reshape(-1, self.n)

    def compact(self, c, n):
        """The amplitudes of a control trajectory, a ``(levels, m)`` array: its value at the first node of every zone."""
        return np.ascontiguousarray(self._levels(c, n)[:, self.first])

    def expand(self, a, base=None):
        """The levels * n trajectory with the amplitudes ``a`` (levels, m) on the zones; where no control acts it holds
        ``base`` (a trajectory, one level or a number; None: 0)."""
        a = np.asarray(a, dtype=np.float64)
        if a.ndim != 2 or a.shape[1] != self.m:
            raise ValueError(f"amplitudes of shape {a.shape}, expected (levels, {self.m})")
        out = np.zeros((a.shape[0], self.n))
        if base is not None:
            b = np.asarray(base, dtype=np.float64)
            out[:] = b if b.ndim == 0 else b.reshape(-1, self.n)
        out[:, self.active] = a[:, self.labels[self.active]]
        return out.ravel()

    def contains(self, c, n):
        """True when every level of the control trajectory ``c`` is constant on every zone, exactly."""
        x = self._levels(c, n)
        return bool(np.array_equal(x[:, self.active], x[:, self.first][:, self.labels[self.active]]))

    def need(self, c, n):
        """The loops' entry check: the labels fit the problem and the start control ``c`` lies in the subspace."""
        self.check(n)
        if not self.contains(c, n):
            raise ValueError("c0 is not constant on the control zones (control_space): project it first, e.g. "
                             "control_space.expand(control_space.compact(c0, n), base=c0), which gives every zone the "
                             "value at its first node and keeps c0 where no control acts")
        return self


def _direction_kw(prob, c0, control_time, control_space):
    """The entry checks of ``control_time=`` / ``control_space=`` and the keyword arguments they add to the
    ``descent_direction`` calls of a loop (neither given: none, today's call exactly)."""
    kw = {}
    if control_time is not None:
        kw["control_time"] = control_time.need(c0, prob.n, prob.num_steps)
    if control_space is not None:
        kw["control_space"] = control_space.need(c0, prob.n)
    return kw


class SolidBodyDrift:
    """Drift-control advection problem on one GPU; ``batch`` independent trajectories advance
    together in every kernel launch (Armijo trial steps, regularisation sweeps)."""

    def __init__(self, mesh: SquareMeshP1, num_steps: int, dt: float, om=np.pi / 40, eps=0.0,
                 drift=(1.0, 1.0), rot_scale=1.0, batch=1, device_id=0, order=_lib.ORDER_FENICS,
                 wind=None):
        self.mesh, self.num_steps, self.dt = mesh, int(num_steps), float(dt)
        self.eps, self.drift, self.rot_scale, self.batch = float(eps), tuple(map(float, drift)), float(rot_scale), int(batch)
        self.order = order
        self.ctx = Context(device_id)
        self.ctx.set_mesh_square(mesh.a1, mesh.a2, mesh.n_cells, order)
        self.n = self.ctx.n
        self.tlen = (self.num_steps + 1) * self.n
        if wind is None:        # 1/om * (-x[1], x[0]) (finaltime.py:91-93): linear, assembled in closed form
            self.Arot = self.ctx.assemble_rotation(1.0 / om)
        else:
            xq, yq = self.ctx.quad_points(mesh.n_cells)
            wx, wy = wind(xq, yq)
            self.Arot = self.ctx.assemble_convection(np.stack([wx, wy], axis=1).reshape(-1))

    # -- device-resident API ---------------------------------------------------
    def new_traj(self, batch=None) -> DeviceArray:
        return self.ctx.zeros(self.tlen * (self.batch if batch is None else batch))

    def forward(self, c: DeviceArray, u: DeviceArray, batch=None, c_shared=False, src=None):
        """u level 0 holds the IC; fills levels 1..Nt.  ``src``: optional source trajectory, the step to
        level n+1 gets rhs = assemble(src_{n+1}*v*dx) (advection_FCT_PDECO_alltime_exact.py:249-253)."""
        self.ctx.solidbody_forward(self.Arot, c, u, self.num_steps, self.dt, self.eps, self.rot_scale,
                                   self.drift, self.batch if batch is None else batch, c_shared, src_traj=src)

    def obs_device(self, obs: Observations):
        """``(theta, cost_w, window)`` of ``obs`` on the device (uploaded once per Observations object)."""
        cache = self.__dict__.setdefault("_obs_cache", {})
        hit = cache.get(id(obs))
        if hit is None or hit[0] is not obs:
            obs.check(self.num_steps, self.n)
            hit = (obs, self.ctx.array(obs.theta), self.ctx.array(obs.cost_w),
                   None if obs.window is None else self.ctx.array(obs.window))
            cache[id(obs)] = hit
        return hit[1:]

    def bounds_device(self, bounds: StateBounds):
        """``(sigma, lower, upper, window)`` of ``bounds`` on the device (uploaded once per set of bounds: the
        :meth:`StateBounds.with_gamma` variants share them)."""
        cache = self.__dict__.setdefault("_bounds_cache", {})
        hit = cache.get(id(bounds._fields))
        if hit is None or hit[0] is not bounds._fields:
            bounds.check(self.num_steps, self.n)
            lo, hi, win = bounds.nodal(self.n)
            up = lambda a: None if a is None else self.ctx.array(np.ascontiguousarray(a))
            hit = (bounds._fields, self.ctx.array(np.ascontiguousarray(bounds.sigma(self.dt))), up(lo), up(hi), up(win))
            cache[id(bounds._fields)] = hit
        return hit[1:]

    def zones_device(self, zones: ControlZones):
        """``Ginv`` of ``zones`` on the device, with the zone table registered on the context.  Once per ControlZones
        object: G = chi^T M chi is formed on the device as the mass restriction of the m indicator fields, symmetrised
        and inverted on the host in float64, and uploaded; another ControlZones on the same context registers its table
        again."""
        cache = self.__dict__.setdefault("_zones_cache", {})
        hit = cache.get(id(zones))
        if hit is None or hit[0] is not zones or self.__dict__.get("_zones_current") is not zones:
            zones.check(self.n)
            self.ctx.set_control_zones(zones.labels, zones.m)
            self.__dict__["_zones_current"] = zones
        if hit is None or hit[0] is not zones:
            m = zones.m
            chi = np.zeros((m, self.n))
            chi[zones.labels[zones.active], np.flatnonzero(zones.active)] = 1.0
            x, g = self.ctx.array(chi), self.ctx.empty(m * m)
            try:
                self.ctx.zone_restrict(x, m, g, apply_mass=True)
                G = g.download().reshape(m, m)
            finally:
                x.free()
                g.free()
            G = 0.5 * (G + G.T)
            hit = (zones, self.ctx.array(np.linalg.inv(G)), G)
            cache[id(zones)] = hit
        return hit[1]

    def _zone_direction(self, zones, x, fields, out, apply_mass):
        """out = chi G^-1 chi^T (M) x for ``fields`` one-level fields (``out`` may be ``x``): two to three launches"""
        Ginv = self.zones_device(zones)
        buf = self.__dict__.get("_zone_buf")
        if buf is None or buf.count < fields * zones.m:
            if buf is not None:
                buf.free()
            buf = self.__dict__["_zone_buf"] = self.ctx.empty(fields * zones.m)
        self.ctx.zone_restrict(x, fields, buf, apply_mass=apply_mass)
        self.ctx.zone_prolong(buf, fields, out, Ginv=Ginv)

    def _corner(self, optim, obs, uhat, batch):
        """The observations and the target trajectory of a mode, for the sweeps with state bounds (which are snapshot
        sweeps): final-time and all-time are their :class:`Observations` corners, the final-time target copied to level
        num_steps of a trajectory-sized buffer that is kept."""
        if _need_obs(optim, obs):
            return obs, uhat
        corners = self.__dict__.setdefault("_corner_obs", {})
        if optim not in corners:
            corners[optim] = (Observations.finaltime(self.num_steps) if optim == "finaltime"
                              else Observations.alltime(self.num_steps, self.dt))
        if optim == "alltime":
            return corners[optim], uhat
        buf = self.__dict__.get("_corner_target")
        if buf is None or buf.count < batch * self.tlen:
            if buf is not None:
                buf.free()
            buf = self.__dict__["_corner_target"] = self.ctx.zeros(batch * self.tlen)
        for b in range(batch):
            buf.copy_from(uhat, self.n, dst_off=b * self.tlen + self.num_steps * self.n, src_off=b * self.n)
        return corners[optim], buf

    def bound_stats(self, u, bounds: StateBounds, batch=None):
        """``(penalty, max_violation, violated_fraction)`` of the trajectories ``u``, one value per batch member each: P,
        the largest |v| and the share of v != 0 among the penalised (level, node) pairs, from one fused pass."""
        B = self.batch if batch is None else batch
        sigma, lo, hi, win = self.bounds_device(bounds)
        out = self.ctx.bound_cost(u, sigma, lo, hi, bounds.gamma, self.num_steps, win, batch=B)
        out[:, 2] /= max(1, bounds.pairs(self.n, self.dt))
        self.last_bound_stats = out
        return out[:, 0], out[:, 1], out[:, 2]

    def adjoint(self, c, u, uhat, p, optim="finaltime", batch=None, c_shared=False, obs=None, state_bounds=None):
        """optim="snapshots": ``uhat`` is a trajectory read at the levels ``obs`` observes only.  ``state_bounds`` (a
        :class:`StateBounds`): the adjoint of J + P, the penalty load in the load launch of every step."""
        if state_bounds is not None:
            B = self.batch if batch is None else batch
            obs, uhat = self._corner(optim, obs, uhat, B)
            theta, _, window = self.obs_device(obs)
            sigma, lo, hi, win = self.bounds_device(state_bounds)
            self.ctx.solidbody_adjoint_bounds(self.Arot, c, u, uhat, theta, obs.tau, window, lo, hi, state_bounds.gamma,
                                              sigma, win, p, self.num_steps, self.dt, self.eps, self.rot_scale, self.drift,
                                              B, c_shared)
            return
        if _need_obs(optim, obs):
            theta, _, window = self.obs_device(obs)
            self.ctx.solidbody_adjoint_obs(self.Arot, c, u, uhat, theta, obs.tau, window, p, self.num_steps, self.dt,
                                           self.eps, self.rot_scale, self.drift, self.batch if batch is None else batch,
                                           c_shared)
            return
        self.ctx.solidbody_adjoint(self.Arot, c, u, uhat, p, self.num_steps, self.dt, self.eps, self.rot_scale,
                                   self.drift, optim == "alltime", self.batch if batch is None else batch, c_shared)

    def descent_direction(self, c, u, p, beta, d, scratch=None, control_time=None, smoothness=None, control_space=None):
        """d_k = ChebSI(-(beta*M*c_k + int p_k (b.grad u_k) v)) for every level k (finaltime.py:228-238);
        all levels are one batched launch sequence.  ``control_time`` (a :class:`ControlIntervals`): the direction
        projected onto the controls constant on its K intervals.  The projection commutes with the per-level mass solve,
        so the right-hand sides are restricted first and K systems are solved in place of num_steps + 1.
        ``smoothness`` (a :class:`Smoothness`): the right-hand side gains -(beta_x Ad c_k + beta_t M tau_k) in the same
        launch; the restriction acts on the right-hand side, so it composes with ``control_time`` unchanged.
        ``control_space`` (a :class:`ControlZones`): d_k = chi G^-1 chi^T rhs_k, the steepest-descent direction among the
        zone-constant controls; the right-hand side is a dual vector, so no mass solve runs at all.  With
        ``control_time``: time restriction, the zone direction of the K fields, time prolongation."""
        levels = self.num_steps + 1
        own = scratch is None
        rhs = self.ctx.empty(self.tlen) if own else scratch
        try:
            if smoothness is None:
                self.ctx.drift_gradient_rhs(c, u, p, beta, rhs, levels, self.drift)
            else:
                self.ctx.drift_gradient_rhs_smooth(c, u, p, beta, smoothness.beta_x, smoothness.beta_t, self.dt, rhs,
                                                   levels, self.drift)
            if control_space is not None:
                self._zone_solve(control_space, control_time, rhs, d, False)
            elif control_time is None:
                self.ctx.chebsi(rhs, d, 20, 0.5, 2.0, batch=levels)
            else:
                self._projected_solve(control_time, rhs, d, 1)
        finally:
            if own:
                rhs.free()

    def _zone_solve(self, zones, ct, x, d, apply_mass):
        """d = chi G^-1 chi^T (M) x level by level (``d`` may be ``x``); with the intervals ``ct``: time restriction, the
        zone operation on the K fields, time prolongation."""
        if ct is None:
            self._zone_direction(zones, x, self.num_steps + 1, d, apply_mass)
            return
        K = ct.check(self.num_steps).K
        rk = self._interval_fields(2 * K * self.n)[0]
        self.ctx.time_restrict(x, ct.starts, self.num_steps, rk, 1)
        self._zone_direction(zones, rk, K, rk, apply_mass)
        self.ctx.time_prolong(rk, ct.starts, self.num_steps, d, 1)

    def _projected_solve(self, ct, rhs, d, batch):
        """d[b] = prolong(ChebSI(restrict(rhs[b]))) for ``batch`` trajectories: batch * K mass solves in one sequence."""
        K, n = ct.check(self.num_steps).K, self.n
        rk, dk = self._interval_fields(2 * batch * K * n)
        self.ctx.time_restrict(rhs, ct.starts, self.num_steps, rk, batch)
        self.ctx.chebsi(rk, dk, 20, 0.5, 2.0, batch=batch * K)
        self.ctx.time_prolong(dk, ct.starts, self.num_steps, d, batch)

    def _interval_fields(self, count):
        """two device buffers of count / 2 doubles each for the K fields of a projection (kept, grown on demand)"""
        buf = self.__dict__.get("_ivl_buf")
        if buf is None or buf.count < count:
            if buf is not None:
                buf.free()
            buf = self.__dict__["_ivl_buf"] = self.ctx.empty(count)
        return buf.ptr, buf.ptr + 8 * (count // 2)

    def cost(self, u, target, c, beta, optim, batch=None, obs=None, state_bounds=None, smoothness=None):
        """J per batch member.  ``state_bounds``: J + P, the statistics of the pass kept in ``last_bound_stats``.
        ``smoothness``: J + R, ``(R_x, R_t)`` of every member from one fused pass kept in ``last_smooth_stats``."""
        if smoothness is not None:
            J = self.cost(u, target, c, beta, optim, batch=batch, obs=obs, state_bounds=state_bounds)
            st = self.ctx.smooth_cost(c, self.num_steps, self.dt, batch=self.batch if batch is None else batch)
            self.last_smooth_stats = st
            return J + smoothness.value(st[:, 0], st[:, 1])
        if state_bounds is not None:
            return self.cost(u, target, c, beta, optim, batch=batch, obs=obs) + self.bound_stats(u, state_bounds, batch)[0]
        if _need_obs(optim, obs):       # every member (all Armijo trials of a batched sweep) in one call
            B = self.batch if batch is None else batch
            _, cost_w, window = self.obs_device(obs)
            return (self.ctx.obs_cost(u, target, cost_w, self.num_steps, window, batch=B)
                    + beta / 2 * self.ctx.l2_norm_sq_Q(c, None, self.num_steps, self.dt, batch=B))
        return self.ctx.cost_functional(u, target, c, self.num_steps, self.dt, beta, optim,
                                        batch=self.batch if batch is None else batch)

    # -- NumPy-facing mirrors of the inline reference loops --------------------------
    def solve_state(self, ck, uk):
        """finaltime.py:175-193: mutates ``uk[nodes:]`` in place and returns ``uk``."""
        c = self.ctx.array(ck)
        u = self.ctx.array(uk)
        try:
            self.forward(c, u, batch=1)
            u.download(uk)
        finally:
            c.free()
            u.free()
        return uk

    def solve_adjoint(self, ck, uk, uhat, pk, optim="finaltime", obs=None, state_bounds=None):
        """finaltime.py:200-221 / alltime.py:232-259: fills and returns ``pk``."""
        c = self.ctx.array(ck)
        u = self.ctx.array(uk)
        uh = self.ctx.array(uhat)
        p = self.ctx.zeros(self.tlen)
        try:
            self.adjoint(c, u, uh, p, optim, batch=1, obs=obs, state_bounds=state_bounds)
            p.download(pk)
        finally:
            for a in (c, u, uh, p):
                a.free()
        return pk

    def solve_descent_direction(self, ck, uk, pk, beta):
        c, u, p = self.ctx.array(ck), self.ctx.array(uk), self.ctx.array(pk)
        d = self.ctx.empty(self.tlen)
        try:
            self.descent_direction(c, u, p, beta, d)
            return d.download()
        finally:
            for a in (c, u, p, d):
                a.free()

    def solver_log(self, batch=None):
        return self.ctx.traj_info(self.num_steps, self.batch if batch is None else batch)

    def close(self):
        self.ctx.close()


class LinearSourceControl(SolidBodyDrift):
    """Linear advection-diffusion with a distributed source control, the problem family of
    advection_FCT_PDECO_{alltime,finaltime}[_exact].py:  A_u = A - eps*Ad (state), A_p = -A - eps*Ad (adjoint),
    state rhs assemble((g + c)*v*dx), adjoint rhs assemble((uhat - u)*v*dx) (all-time) or terminal condition
    uhat_T - u(T) (final-time).  ``wind(x, y) -> (wx, wy)`` as in the scripts' ``velocity``."""

    def __init__(self, mesh, num_steps, dt, wind, eps=1e-3, batch=1, device_id=0, order=_lib.ORDER_FENICS):
        super().__init__(mesh, num_steps, dt, eps=eps, drift=(0.0, 0.0), rot_scale=1.0, batch=batch,
                         device_id=device_id, order=order, wind=wind)
        self._zero_c = self.ctx.zeros(self.tlen)     # no drift control: the control enters through the source

    def state(self, src: DeviceArray, u: DeviceArray, batch=None):
        """advection_FCT_PDECO_alltime_exact.py:236-253 (src = g + c, both trajectories)"""
        self.forward(self._zero_c, u, batch=batch, c_shared=True, src=src)

    def adjoint_state(self, u, uhat, p, optim="alltime", batch=None, obs=None, state_bounds=None):
        """:259-274 (all-time) / advection_FCT_PDECO_finaltime.py (final-time)"""
        self.adjoint(self._zero_c, u, uhat, p, optim, batch=batch, c_shared=True, obs=obs, state_bounds=state_bounds)

    def descent_direction(self, c, p, beta, d, control_time=None, smoothness=None, control_space=None):
        """advection_FCT_PDECO_alltime_exact.py:278: d = -(beta*c - p), every level, the script's operation order.
        ``control_time`` (a :class:`ControlIntervals`): then projected onto the controls constant on its intervals.
        ``smoothness`` (a :class:`Smoothness` with a non-zero coefficient): d = -(beta*c - p) + ChebSI(smooth_rhs), one
        mass solve per level for the term's gradient, before the projection.
        ``control_space`` (a :class:`ControlZones`): then d_k <- chi G^-1 chi^T M d_k, the orthogonal projection in the
        mass inner product onto the zone-constant controls (with ``control_time``: on its K fields)."""
        if smoothness is not None and smoothness.active:
            buf = self.__dict__.get("_smooth_buf")
            if buf is None:
                buf = self.__dict__["_smooth_buf"] = self.ctx.empty(2 * self.tlen)
            rhs, sm = buf.ptr, buf.ptr + 8 * self.tlen
            self.ctx.smooth_rhs(c, smoothness.beta_x, smoothness.beta_t, self.num_steps, self.dt, rhs, batch=1)
            self.ctx.chebsi(rhs, sm, 20, 0.5, 2.0, batch=self.num_steps + 1)
            self.ctx.descent_pointwise(self.tlen, beta, c, p, rhs)
            self.ctx.axpby(self.tlen, 1.0, rhs, 1.0, sm, d)
        else:
            self.ctx.descent_pointwise(self.tlen, beta, c, p, d)
        if control_space is not None:
            self._zone_solve(control_space, control_time, d, d, True)
        elif control_time is not None:
            K = control_time.check(self.num_steps).K
            self.ctx.time_project(d, control_time.starts, self.num_steps, self._interval_fields(2 * K * self.n)[0])

    def sensitivity(self, d, w):
        """:282-297: w = S(d), the state sweep with source d and a zero initial condition (level 0 of ``w`` is zeroed)."""
        _lib.check(self.ctx.handle, _lib.lib.femfct_memset0(self.ctx.handle, dptr(w), 8 * self.n))
        self.forward(self._zero_c, w, batch=1, c_shared=True, src=d)

    def solve_state(self, src, uk):
        s, u = self.ctx.array(src), self.ctx.array(uk)
        try:
            self.state(s, u, batch=1)
            u.download(uk)
        finally:
            s.free()
            u.free()
        return uk

    def solve_adjoint_state(self, uk, uhat, pk, optim="alltime", obs=None, state_bounds=None):
        u, uh, p = self.ctx.array(uk), self.ctx.array(uhat), self.ctx.zeros(self.tlen)
        try:
            self.adjoint_state(u, uh, p, optim, batch=1, obs=obs, state_bounds=state_bounds)
            p.download(pk)
        finally:
            for a in (u, uh, p):
                a.free()
        return pk


class LinearReactionSourceControl(LinearSourceControl):
    """The same problem family with a reaction term, du/dt - eps*lap(u) + div(w u) + g u = c + f, the final-time
    manufactured-solution study advection_FCT_PDECO_finaltime_exact.py.  The reaction term is explicit (IMEX), as the
    script runs it:

        state / sensitivity (:252-279, :344-370)   rhs_i = M src_i - Mg(g_{i-1}) u_{i-1},  A_u = Aa1 - eps*Ad
        adjoint (:293-322)                         rhs_i = -Mg(g_i) p_{i+1} [+ M (uhat_i - u_i) all-time],
                                                   A_p = -(Aa1 + Aa2) - eps*Ad

    with Mg(g) = assemble(g_h*u*v*dx) applied matrix-free in the step's load kernel.  ``react``: the coefficient
    trajectory, (num_steps + 1) * nodes nodal values in the problem's DoF order, shared by every batch member.
    ``adjoint_mass``: nodal values of a P1 field sigma ~ div(w), Aa2 = assemble(sigma_h*u*v*dx) (None: Aa2 = 0).  The
    script builds Aa2 from a cellwise-constant L2 projection of div(w) instead; INTEGRATION.md states the difference.
    ``solve_state`` / ``solve_adjoint_state`` are the parent's and run the sweeps below."""

    def __init__(self, mesh, num_steps, dt, wind, react, eps=1e-4, adjoint_mass=None, batch=1, device_id=0,
                 order=_lib.ORDER_FENICS):
        react = np.asarray(react, dtype=np.float64).ravel()
        tlen = (int(num_steps) + 1) * mesh.nodes
        if react.size != tlen:
            raise ValueError(f"react of {react.size} values, expected (num_steps + 1) * nodes = {tlen}")
        if adjoint_mass is not None:
            adjoint_mass = np.asarray(adjoint_mass, dtype=np.float64).ravel()
            if adjoint_mass.size != mesh.nodes:
                raise ValueError(f"adjoint_mass of {adjoint_mass.size} values, expected {mesh.nodes}")
        super().__init__(mesh, num_steps, dt, wind, eps=eps, batch=batch, device_id=device_id, order=order)
        self._react = self.ctx.array(react)
        if adjoint_mass is None:
            self.Aadj = self.Arot
        else:
            sig = self.ctx.array(adjoint_mass)
            Aa2 = self.ctx.assemble_weighted_mass(sig)
            self.Aadj = self.ctx.empty(self.ctx.W * self.n)
            self.ctx.axpby(self.ctx.W * self.n, 1.0, self.Arot, 1.0, Aa2, self.Aadj)
            sig.free()
            Aa2.free()

    def state(self, src: DeviceArray, u: DeviceArray, batch=None):
        self.ctx.linear_forward_react(self.Arot, src, self._react, u, self.num_steps, self.dt, self.eps,
                                      self.batch if batch is None else batch)

    def adjoint_state(self, u, uhat, p, optim="finaltime", batch=None, obs=None, state_bounds=None):
        if state_bounds is not None:
            B = self.batch if batch is None else batch
            obs, uhat = self._corner(optim, obs, uhat, B)
            theta, _, window = self.obs_device(obs)
            sigma, lo, hi, win = self.bounds_device(state_bounds)
            self.ctx.linear_adjoint_react_bounds(self.Aadj, self._react, u, uhat, theta, obs.tau, window, lo, hi,
                                                 state_bounds.gamma, sigma, win, p, self.num_steps, self.dt, self.eps, B)
            return
        if _need_obs(optim, obs):
            theta, _, window = self.obs_device(obs)
            self.ctx.linear_adjoint_react_obs(self.Aadj, self._react, u, uhat, theta, obs.tau, window, p, self.num_steps,
                                              self.dt, self.eps, self.batch if batch is None else batch)
            return
        self.ctx.linear_adjoint_react(self.Aadj, self._react, u, uhat, p, self.num_steps, self.dt, self.eps,
                                      optim == "alltime", self.batch if batch is None else batch)

    def sensitivity(self, d, w):
        _lib.check(self.ctx.handle, _lib.lib.femfct_memset0(self.ctx.handle, dptr(w), 8 * self.n))
        self.state(d, w, batch=1)


def finaltime_exact_wind(gamma=0.1, k3=1, k4=1):
    """The wind of the final-time manufactured study on the unit square, w = gamma/2 * (sin 2 k3 pi x, sin 2 k4 pi y)
    (advection_FCT_PDECO_finaltime_exact.py:140-151), as a ``wind(x, y) -> (wx, wy)`` callable."""
    return lambda x, y: (gamma * np.sin(k3 * np.pi * x) * np.cos(k3 * np.pi * x),
                         gamma * np.sin(k4 * np.pi * y) * np.cos(k4 * np.pi * y))


def finaltime_exact_fields(t, X, Y, T=0.1, beta=0.1, c_lower=0.0, c_upper=1.0, e1=1.0, e2=1.0, k1=1, k2=1, k3=1, k4=1,
                           eps=1e-4, gamma=0.1, delta_ex=0.1):
    """Inputs of the manufactured problem of advection_FCT_PDECO_finaltime_exact.py:76-138 at time t on the grid X, Y
    (unit square), with the script's defaults: state u = e^{e1 t} (cos k1 pi x cos k2 pi y + 1), adjoint
    p = (e^{e2 T} - e^{e2 t}) cos k3 pi x cos k4 pi y, control c = clip(p / beta), reaction coefficient g, source f and
    target uhat = u.  "div" is the analytic divergence of the wind, gamma pi (k3 cos 2 k3 pi x + k4 cos 2 k4 pi y)."""
    pi = np.pi
    et = np.exp(e1 * t)
    cx1, sx1, cy2, sy2 = np.cos(k1 * pi * X), np.sin(k1 * pi * X), np.cos(k2 * pi * Y), np.sin(k2 * pi * Y)
    u = et * (cx1 * cy2 + 1)
    p = (np.exp(e2 * T) - np.exp(e2 * t)) * np.cos(k3 * pi * X) * np.cos(k4 * pi * Y)
    c = np.clip(1 / beta * p, c_lower, c_upper)
    g = (-e2 * np.exp(e2 * t) / (np.exp(e2 * T) - np.exp(e2 * t * (1 - delta_ex))) - eps * (k3 ** 2 + k4 ** 2) * pi ** 2
         - gamma * pi * (k3 * np.sin(k3 * pi * X) ** 2 + k4 * np.sin(k4 * pi * Y) ** 2))
    wx, wy = finaltime_exact_wind(gamma, k3, k4)(X, Y)
    div = gamma * pi * (k3 * np.cos(2 * k3 * pi * X) + k4 * np.cos(2 * k4 * pi * Y))
    f = (e1 * u                                                     # du/dt
         + eps * (k1 ** 2 + k2 ** 2) * pi ** 2 * (u - et)           # -eps lap u
         + div * u - et * pi * (k1 * wx * sx1 * cy2 + k2 * wy * cx1 * sy2)      # div(w u) = div(w) u + w . grad u
         + g * u - c)
    return dict(u=u, p=p, c=c, g=g, f=f, uhat=u.copy(), div=div)


def _bounds_kw(prob, state_bounds):
    """the keyword the loops pass on to ``prob.adjoint`` / ``prob.cost`` (none without state bounds: today's calls)"""
    if state_bounds is None:
        return {}
    if not isinstance(state_bounds, StateBounds):
        raise ValueError("state_bounds must be a StateBounds")
    state_bounds.check(prob.num_steps, prob.n)
    return dict(state_bounds=state_bounds)


def _record_bounds(prob, hist, member):
    """the statistics of batch member ``member`` of the last cost pass, the accepted iterate's, into the history"""
    P, vmax, frac = prob.last_bound_stats[member]
    hist.setdefault("penalty", []).append(float(P))
    hist.setdefault("max_violation", []).append(float(vmax))
    hist.setdefault("violated_fraction", []).append(float(frac))


def _smooth_kw(smoothness):
    """the keyword the loops pass on to ``prob.descent_direction`` / ``prob.cost`` (none without the term: today's calls)"""
    if smoothness is None:
        return {}
    if not isinstance(smoothness, Smoothness):
        raise ValueError("smoothness must be a Smoothness")
    return dict(smoothness=smoothness)


def _record_smooth(prob, hist, member):
    """``(R_x, R_t)`` of batch member ``member`` of the last cost pass, the accepted iterate's, into the history"""
    Rx, Rt = prob.last_smooth_stats[member]
    hist.setdefault("roughness_x", []).append(float(Rx))
    hist.setdefault("roughness_t", []).append(float(Rt))


def pgd_solidbody_finaltime(prob: SolidBodyDrift, u0, uhat_T, c0, beta, c_lower, c_upper, iters,
                            gam=1e-4, s0=1.0, max_armijo=10, speculative=True, tol=None, control_time=None,
                            state_bounds=None, smoothness=None, control_space=None):
    """Final-time variant of :func:`pgd_solidbody` (advection_solidbody_FCT_PDECO_finaltime_Garvie.py)."""
    return pgd_solidbody(prob, u0, uhat_T, c0, beta, c_lower, c_upper, iters, gam, s0, max_armijo, speculative, tol,
                         optim="finaltime", control_time=control_time, state_bounds=state_bounds, smoothness=smoothness,
                         control_space=control_space)


def pgd_solidbody_alltime(prob: SolidBodyDrift, u0, uhat_all, c0, beta, c_lower, c_upper, iters,
                          gam=1e-4, s0=1.0, max_armijo=10, speculative=True, tol=None, control_time=None,
                          state_bounds=None, smoothness=None, control_space=None):
    """All-time variant (advection_solidbody_FCT_PDECO_alltime_Garvie.py, config C5's loop): ``uhat_all``
    is the target trajectory ((Nt+1)*n, level 0 = u0)."""
    return pgd_solidbody(prob, u0, uhat_all, c0, beta, c_lower, c_upper, iters, gam, s0, max_armijo, speculative, tol,
                         optim="alltime", control_time=control_time, state_bounds=state_bounds, smoothness=smoothness,
                         control_space=control_space)


def pgd_solidbody_snapshots(prob: SolidBodyDrift, u0, uhat, obs: Observations, c0, beta, c_lower, c_upper, iters,
                            gam=1e-4, s0=1.0, max_armijo=10, speculative=True, tol=None, control_time=None,
                            state_bounds=None, smoothness=None, control_space=None):
    """Snapshot variant of :func:`pgd_solidbody`: ``uhat`` is a (num_steps+1)*n trajectory of which only the levels that
    ``obs`` observes are read (the others may hold anything, NaN included)."""
    return pgd_solidbody(prob, u0, uhat, c0, beta, c_lower, c_upper, iters, gam, s0, max_armijo, speculative, tol,
                         optim="snapshots", obs=obs, control_time=control_time, state_bounds=state_bounds,
                         smoothness=smoothness, control_space=control_space)


def pgd_solidbody(prob: SolidBodyDrift, u0, uhat, c0, beta, c_lower, c_upper, iters,
                  gam=1e-4, s0=1.0, max_armijo=10, speculative=True, tol=None, optim="finaltime", obs=None,
                  control_time=None, state_bounds=None, smoothness=None, control_space=None):
    """Projected gradient descent for the drift-control problem, following the loop of
    advection_solidbody_FCT_PDECO_finaltime_Garvie.py:164-330 / ..._alltime_Garvie.py:164-340 step for step:

        adjoint(c_prev, u) -> d = ChebSI(-(beta M c_prev + int p (b.grad u) v)) -> c = clip(c_prev + s0 d)
        -> state(c) -> J_k -> Armijo: trials c_inc = clip(c + s d), s = s0/2^k, accept the first with
        J(c_inc) - J_k <= -gam/s ||c_inc - c||^2_Q  (else the last) -> c_prev = c_inc

    optim="finaltime": target uhat(T) (n values), p(T) = uhat_T - u(T), u(T) seeded with the target before
    the first adjoint solve; optim="alltime": target trajectory, p(T) = 0, misfit load at every level,
    u seeded with the whole target trajectory (alltime_Garvie.py: ``uk = np.copy(uhat_all)``).
    Everything stays in HBM; the host sees scalars only.  ``speculative=True`` evaluates all
    ``max_armijo`` trial steps as one batch of independent trajectories (same launches, B = max_armijo)
    and picks the first accepted one -- the iterate of the sequential search (each trial trajectory is
    the same computation; the states agree to the low-order solver tolerance, 1e-13).
    optim="snapshots": target trajectory read at the levels of ``obs`` only, the adjoint and cost of
    :class:`Observations`; u is seeded with the target at the observed levels (both modes above, seen as observations).
    ``control_time`` (a :class:`ControlIntervals`): the control is constant in time on its intervals; d is projected onto
    these controls and ``c0`` must be one of them (ValueError otherwise).  None: the free space-time control.
    ``control_space`` (a :class:`ControlZones`): the control is constant in space on its zones and untouched where no
    zone lies; d is the steepest-descent direction among these controls and ``c0`` must be one of them.
    ``state_bounds`` (a :class:`StateBounds`): the loop descends J + P, and the history gains ``penalty``,
    ``max_violation`` and ``violated_fraction`` of the accepted iterate, from the pass that costs the trials.
    ``smoothness`` (a :class:`Smoothness`): the loop descends J + R (+ P), the direction's right-hand side gains the
    term's in the same launch, and the history gains ``roughness_x`` and ``roughness_t``, R_x and R_t of the accepted
    iterate, from the pass that costs the trials.
    Returns ``(u, p, c, history)`` as NumPy arrays + a dict of per-iteration scalars."""
    snap = _need_obs(optim, obs)
    sbk = _bounds_kw(prob, state_bounds)
    smk = _smooth_kw(smoothness)
    alltime = optim == "alltime" or snap         # (the target is a trajectory)
    ctx, n, Nt, dt, tl = prob.ctx, prob.n, prob.num_steps, prob.dt, prob.tlen
    dkw = _direction_kw(prob, c0, control_time, control_space)
    B = int(max_armijo) if speculative else 1
    u = ctx.zeros(tl)
    u.upload(np.concatenate([np.asarray(u0, dtype=np.float64), np.zeros(tl - n)]))
    # the reference seeds u(T) with the target before the first adjoint solve (finaltime.py:146)
    p, d, c, rhs = ctx.zeros(tl), ctx.zeros(tl), ctx.zeros(tl), ctx.empty(tl)
    c_prev = ctx.array(np.asarray(c0, dtype=np.float64))
    uhat = np.asarray(uhat, dtype=np.float64).ravel()
    if uhat.size != (tl if alltime else n):
        raise ValueError(f"target of {uhat.size} values, expected {tl if alltime else n} for optim='{optim}'")
    uh = ctx.array(uhat)
    uhB = ctx.zeros(B * uhat.size)                      # B copies of the target, replicated on the device
    for k in range(B):
        uhB.copy_from(uh, uhat.size, dst_off=k * uhat.size)
    cB, uB, ckB = ctx.zeros(B * tl), ctx.zeros(B * tl), ctx.zeros(B * tl)
    for k in range(B):                                  # level 0 of every trial trajectory = the initial condition
        uB.copy_from(u, n, dst_off=k * tl)
    # armijo_margin: per iteration, for every trial the sequential search looks at, the distance of the Armijo test from
    # its threshold relative to the cost, (J_trial - J_k + gam/s ||c_inc - c||^2_Q) / |J_k|  (> 0: rejected).  A margin of
    # the size of the solver tolerance would mean that two faithful implementations may decide differently.
    hist = dict(cost=[], armijo_k=[], step=[], rel_change=[], armijo_margin=[], wall=[], wall0=time.perf_counter())
    if snap:
        for lv in obs.levels[obs.levels > 0]:
            u.copy_from(uh, n, dst_off=int(lv) * n, src_off=int(lv) * n)
    elif alltime:
        u.copy_from(uh, tl - n, dst_off=n, src_off=n)      # uk = np.copy(uhat_all), level 0 = u0
    else:
        u.copy_from(uh, n, dst_off=Nt * n)                 # uk[num_steps*nodes:] = uhat_T
    try:
        for it in range(iters):
            prob.adjoint(c_prev, u, uh, p, optim, batch=1, obs=obs, **sbk)
            prob.descent_direction(c_prev, u, p, beta, d, scratch=rhs, **dkw, **smk)
            ctx.project_control(c_prev, s0, d, c_lower, c_upper, c, tl)
            prob.forward(c, u, batch=1)
            J_k = float(prob.cost(u, uh, c, beta, optim, batch=1, obs=obs, **sbk, **smk)[0])
            svals = [s0 * (1 / 2 ** k) for k in range(max_armijo)]
            accepted = None
            if speculative:
                for k, s in enumerate(svals):
                    ctx.project_control(c, s, d, c_lower, c_upper, cB.ptr + 8 * k * tl, tl)
                    ckB.copy_from(c, tl, dst_off=k * tl)
                prob.forward(cB, uB, batch=B)
                J = prob.cost(uB, uhB, cB, beta, optim, batch=B, obs=obs, **sbk, **smk)
                stat = ctx.l2_norm_sq_Q(cB, ckB, Nt, dt, batch=B)
                margins = []
                for k, s in enumerate(svals):
                    accepted = k
                    margins.append((float(J[k]) - J_k + gam / s * float(stat[k])) / abs(J_k))
                    if not (J[k] - J_k > -gam / s * stat[k]):
                        break
                J_acc = float(J[accepted])
                c_prev.copy_from(cB, tl, src_off=accepted * tl)
                u.copy_from(uB, tl, src_off=accepted * tl)
            else:
                margins = []
                for k, s in enumerate(svals):
                    accepted = k
                    ctx.project_control(c, s, d, c_lower, c_upper, cB, tl)
                    prob.forward(cB, uB, batch=1)
                    J_acc = float(prob.cost(uB, uh, cB, beta, optim, batch=1, obs=obs, **sbk, **smk)[0])
                    stat = float(ctx.l2_norm_sq_Q(cB, c, Nt, dt)[0])
                    margins.append((J_acc - J_k + gam / s * stat) / abs(J_k))
                    if not (J_acc - J_k > -gam / s * stat):
                        break
                c_prev.copy_from(cB, tl)
                u.copy_from(uB, tl)
            if sbk:
                _record_bounds(prob, hist, accepted if speculative else 0)
            if smk:
                _record_smooth(prob, hist, accepted if speculative else 0)
            hist["cost"].append(J_acc)
            hist["wall"].append(time.perf_counter())          # (J_acc is a read-back: the iteration's device work is done)
            hist["armijo_margin"].append(margins)
            hist["armijo_k"].append(accepted + 1)
            hist["step"].append(svals[accepted])
            hist["rel_change"].append(abs(J_k - J_acc) / abs(J_k))
            if tol is not None and hist["rel_change"][-1] < tol:
                break
        hist["armijo_margin_min"] = min((abs(m) for ms in hist["armijo_margin"] for m in ms), default=None)
        return u.download(), p.download(), c_prev.download(), hist
    finally:
        for a in (u, p, d, c, rhs, c_prev, uh, uhB, cB, uB, ckB):
            a.free()


class LockstepResult(list):
    """What :func:`pgd_solidbody_lockstep` returns: the list of ``(u, p, c, hist)``, one per problem, with ``record``, the
    launches of the run: per iteration ``problems`` (active problems = batch of the adjoint and first state sweep),
    ``trials`` (members of the trial sweep) and the ``ctx.kernel_regime`` of both batches."""
    record: dict


def pgd_solidbody_lockstep(prob: SolidBodyDrift, u0, uhat, c0, betas, c_lower, c_upper, iters,
                           gam=1e-4, s0=1.0, max_armijo=10, tol=None, optim="finaltime", control_time=None):
    """P projected-gradient loops of :func:`pgd_solidbody` (speculative form) carried in lockstep: problem p has the
    regularisation ``betas[p]`` and, optionally, its own start control (``c0`` of shape (P, tlen); one (tlen,) control is
    shared), first step length (``s0``: a scalar or P values) and target (``uhat``: one target or P).  The regularisation
    sweep of advection_solidbody_FCT_PDECO_alltime.py:43-74 (one edited script copy per beta) as one loop.

    Each iteration is pgd_solidbody's, statement for statement, for all active problems at once: one adjoint sweep and
    one state sweep of P_active trajectories, one sweep of the P_active * max_armijo trial trajectories, the trial
    controls and all costs / distances in one launch each (femfct_trial_controls, femfct_member_costs); the host makes
    the Armijo decisions from the 2 * P_active * max_armijo scalars.  A batch member computes what it would compute alone,
    so every problem follows its own pgd_solidbody run (to the low-order solver tolerance; P = 1 is that run, bit for bit).
    A problem whose rel_change < ``tol`` is finished: its results are kept and it leaves all later launches.
    ``control_time`` (a :class:`ControlIntervals`): as in pgd_solidbody, for every problem; the directions of the active
    problems are K * P_active mass solves in one sequence.
    Returns a :class:`LockstepResult`; each ``hist`` has pgd_solidbody's keys."""
    if optim == "snapshots":
        raise ValueError("optim='snapshots' is not yet carried by the lockstep loop (the snapshot cost takes one target per "
                         "member); use pgd_solidbody_snapshots per problem")
    if optim not in ("alltime", "finaltime"):
        raise ValueError(f"Invalid value for 'optim': '{optim}'. Must be one of ['alltime', 'finaltime'].")
    alltime = optim == "alltime"
    ctx, n, Nt, dt, tl = prob.ctx, prob.n, prob.num_steps, prob.dt, prob.tlen
    betas = np.asarray(betas, dtype=np.float64).ravel()
    P, K = betas.size, int(max_armijo)
    if P < 1:
        raise ValueError("betas is empty: no problem to solve")
    if K < 1 or P * K > _lib.MAX_MEMBERS:
        raise ValueError(f"{P} problems x max_armijo = {K}: the product must be in 1..{_lib.MAX_MEMBERS}")
    u0 = np.asarray(u0, dtype=np.float64).ravel()
    if u0.size != n:
        raise ValueError(f"u0 of {u0.size} values, expected {n}")
    c0 = np.asarray(c0, dtype=np.float64)
    if c0.shape == (tl,):
        c0 = np.broadcast_to(c0, (P, tl))
    elif c0.shape != (P, tl):
        raise ValueError(f"c0 of shape {c0.shape}, expected ({tl},) or ({P}, {tl})")
    if control_time is not None:
        for c0p in c0:
            control_time.need(c0p, n, Nt)
    s0 = np.asarray(s0, dtype=np.float64)
    if s0.ndim == 0:
        s0 = np.full(P, float(s0))
    elif s0.shape != (P,):
        raise ValueError(f"s0 of shape {s0.shape}, expected a scalar or ({P},)")
    usz = tl if alltime else n
    uhat = np.asarray(uhat, dtype=np.float64)
    if uhat.shape == (P, usz) and P > 1:
        per_problem = True
    elif uhat.size == usz:
        per_problem, uhat = False, uhat.reshape(usz)
    else:
        raise ValueError(f"target of shape {uhat.shape}, expected {usz} values or ({P}, {usz}) for optim='{optim}'")
    bufs = []

    def alloc(count, zero=True):
        a = ctx.zeros(count) if zero else ctx.empty(count)
        bufs.append(a)
        return a

    at = lambda a, off: a.ptr + 8 * off          # device address of element ``off``
    try:
        u, p, d, c, rhs = alloc(P * tl), alloc(P * tl), alloc(P * tl), alloc(P * tl), alloc(P * tl, False)
        c_prev = alloc(P * tl, False).upload(np.ascontiguousarray(c0))
        uhP = alloc(P * usz, False)                 # a target per problem: what the adjoint sweep of P members reads
        uhP.upload(np.ascontiguousarray(uhat if per_problem else np.broadcast_to(uhat, (P, usz))))
        # (a shared target: the costs read the first copy; never a copy per trial)
        cB, uB = alloc(P * K * tl), alloc(P * K * tl)
        u0d = alloc(n, False).upload(u0)
        for j in range(P):                          # level 0 of every trajectory = the initial condition
            u.copy_from(u0d, n, dst_off=j * tl)
        for m in range(P * K):
            uB.copy_from(u0d, n, dst_off=m * tl)
        for j in range(P):                          # the reference seeds u with the target before the first adjoint solve
            if alltime:
                u.copy_from(uhP, tl - n, dst_off=j * tl + n, src_off=j * tl + n)
            else:
                u.copy_from(uhP, n, dst_off=j * tl + Nt * n, src_off=j * n)
        wall0 = time.perf_counter()
        hists = [dict(cost=[], armijo_k=[], step=[], rel_change=[], armijo_margin=[], wall=[], wall0=wall0)
                 for _ in range(P)]
        results = [None] * P
        record = dict(problems=[], trials=[], regime_problems=[], regime_trials=[])
        act = list(range(P))                        # slot j of every buffer holds problem act[j]

        def finish(j):
            h = hists[act[j]]
            h["armijo_margin_min"] = min((abs(m) for ms in h["armijo_margin"] for m in ms), default=None)
            out = []
            for a in (u, p, c_prev):
                host = np.empty(tl)
                _lib.check(ctx.handle, _lib.lib.femfct_memcpy_d2h(ctx.handle, host.ctypes.data, at(a, j * tl), 8 * tl))
                out.append(host)
            results[act[j]] = (*out, h)

        for it in range(iters):
            Pa = len(act)
            if Pa == 0:
                break
            b_act, s_act = betas[act], s0[act]
            record["problems"].append(Pa)
            record["trials"].append(Pa * K)
            record["regime_problems"].append(ctx.kernel_regime(Pa))
            record["regime_trials"].append(ctx.kernel_regime(Pa * K))
            prob.adjoint(c_prev, u, uhP, p, optim, batch=Pa)
            for j in range(Pa):
                ctx.drift_gradient_rhs(at(c_prev, j * tl), at(u, j * tl), at(p, j * tl), b_act[j], at(rhs, j * tl), Nt + 1,
                                       prob.drift)
            if control_time is None:
                ctx.chebsi(rhs, d, 20, 0.5, 2.0, batch=(Nt + 1) * Pa)
            else:
                prob._projected_solve(control_time, rhs, d, Pa)
            ctx.trial_controls(c_prev, d, s_act, Pa, 1, c_lower, c_upper, tl, c)
            prob.forward(c, u, batch=Pa)
            J_k, _ = ctx.member_costs(u, uhP, c, b_act, Pa, 1, Nt, dt, optim,
                                      uhat_per_problem=per_problem)
            svals = [[float(s) * (1 / 2 ** k) for k in range(K)] for s in s_act]
            ctx.trial_controls(c, d, np.array(svals), Pa, K, c_lower, c_upper, tl, cB)
            prob.forward(cB, uB, batch=Pa * K)
            J, stat = ctx.member_costs(uB, uhP, cB, b_act, Pa, K, Nt, dt, optim, cref=c,
                                       uhat_per_problem=per_problem)
            now = time.perf_counter()               # (J is a read-back: the iteration's device work is done)
            done = []
            for j in range(Pa):
                Jk, h, margins, accepted = float(J_k[j]), hists[act[j]], [], None
                for k, s in enumerate(svals[j]):
                    accepted, m = k, j * K + k
                    margins.append((float(J[m]) - Jk + gam / s * float(stat[m])) / abs(Jk))
                    if not (J[m] - Jk > -gam / s * stat[m]):
                        break
                m = j * K + accepted
                J_acc = float(J[m])
                c_prev.copy_from(cB, tl, dst_off=j * tl, src_off=m * tl)
                u.copy_from(uB, tl, dst_off=j * tl, src_off=m * tl)
                h["cost"].append(J_acc)
                h["wall"].append(now)
                h["armijo_margin"].append(margins)
                h["armijo_k"].append(accepted + 1)
                h["step"].append(svals[j][accepted])
                h["rel_change"].append(abs(Jk - J_acc) / abs(Jk))
                if tol is not None and h["rel_change"][-1] < tol:
                    done.append(j)
            if done:                                # keep the finished problems' results, close the ranks of the others
                for j in done:
                    finish(j)
                keep = [j for j in range(Pa) if j not in done]
                for jn, jo in enumerate(keep):
                    if jn != jo:                    # (jn < jo: slots are disjoint blocks)
                        for a, sz in ((u, tl), (p, tl), (c_prev, tl)) + (((uhP, usz),) if per_problem else ()):
                            a.copy_from(a, sz, dst_off=jn * sz, src_off=jo * sz)
                act = [act[j] for j in keep]
        for j in range(len(act)):
            finish(j)
        out = LockstepResult(results)
        out.record = record
        return out
    finally:
        for a in bufs:
            a.free()


def pgd_source_control(prob: LinearSourceControl, u0, uhat, c0, beta, c_lower, c_upper, g=None, optim="alltime",
                       increment="linear", gam=1e-4, s0=1.0, max_armijo=10, tol=1e-4, max_iters=1000, stop="both", obs=None,
                       control_time=None, state_bounds=None, smoothness=None, control_space=None):
    """Projected gradient descent for the linear source-control problem, the loop of
    advection_FCT_PDECO_alltime_exact.py:212-330 (optim="alltime", stop="both") and advection_FCT_PDECO_finaltime.py:
    170-280 (optim="finaltime", stop="cost"):

        u = S(g + c_k) -> p (all-time: p(T) = 0, load M (uhat_n - u_n); final-time: p(T) = uhat_T - u(T))
        -> d = -(beta c_k - p) -> Armijo over s_j = s0 / 2^j, c_j = clip(c_k + s_j d): accept the first trial with
        J_j - J_ref <= -gam / s_j ||c_j - c_k||^2_Q (else the last) -> c_{k+1} = c_j

    increment="linear" (the scripts): J_j = J(u + s_j w, c_j) with the sensitivity w = S(d) (zero IC), all trials in one
    fused pass (femfct_linear_trial_costs).  increment="resolve" (HEAD's nonlinear_solver branch): J_j = J(S(g + c_j), c_j),
    the ``max_armijo`` trial states as one batched sweep.  J_ref starts at 10 J(u with level 0 only, c_0), then is the
    cost the previous iteration accepted.  Stop test: stop_crit = ||c_{k+1} - c_k||^2_Q / ||c_k||^2_Q (infinite while
    ||c_k|| = 0) and stop_crit2 = |J_ref - J_acc| / |J_ref|; the loop runs while stop_crit2 >= tol, or (stop="both")
    stop_crit >= tol, and fewer than ``max_iters`` iterations have run.

    optim="snapshots" (increment="resolve" only): the adjoint and cost of ``obs``, an :class:`Observations`; ``uhat`` is
    a trajectory read at the observed levels only.
    ``control_time`` (a :class:`ControlIntervals`): the control is constant in time on its intervals; d is projected onto
    these controls (both increments: in linear mode the sensitivity is S(P d)) and ``c0`` must be one of them.
    ``control_space`` (a :class:`ControlZones`): the control is constant in space on its zones; d is projected onto these
    controls in the mass inner product (both increments) and ``c0`` must be one of them.
    ``uhat``: target trajectory (all-time) or uhat_T (final-time, n values); ``g``: fixed source trajectory or None.
    Everything stays in HBM; the host sees scalars only.  Returns ``(u, p, c, hist)`` like the scripts: u and p are the
    last iteration's state and adjoint (at the control that iteration started from), c the last accepted control.
    hist["cost"][k] is the accepted J_acc (the linear estimate in linear mode); hist["cost_state"][k] the cost
    J(S(g + c_k), c_k) of the re-solved state at the control iteration k started from, so hist["cost_state"][k + 1]
    re-solves hist["cost"][k].
    ``state_bounds`` (a :class:`StateBounds`; increment="resolve" only): the loop descends J + P, and the history gains
    ``penalty``, ``max_violation`` and ``violated_fraction`` of the accepted iterate.
    ``smoothness`` (a :class:`Smoothness`; increment="resolve" only): the loop descends J + R (+ P) with
    d = -(beta c_k - p) + ChebSI(smooth_rhs), and the history gains ``roughness_x`` and ``roughness_t`` of the accepted
    iterate."""
    snap = _need_obs(optim, obs)
    if increment not in ("linear", "resolve"):
        raise ValueError(f"Invalid value for 'increment': '{increment}'. Must be one of ['linear', 'resolve'].")
    if smoothness is not None and increment == "linear":
        raise ValueError("smoothness needs increment='resolve': the fused linear-increment trial costs do not know the "
                         "term")
    smk = _smooth_kw(smoothness)
    if state_bounds is not None and increment == "linear":
        raise ValueError("state_bounds needs increment='resolve': the fused linear-increment trial costs know the "
                         "all-time and final-time modes only")
    sbk = _bounds_kw(prob, state_bounds)
    if snap and increment == "linear":
        raise ValueError("optim='snapshots' needs increment='resolve': the fused linear-increment trial costs know the "
                         "all-time and final-time modes only")
    if stop not in ("both", "cost"):
        raise ValueError(f"Invalid value for 'stop': '{stop}'. Must be one of ['both', 'cost'].")
    K = int(max_armijo)
    if not 1 <= K <= _lib.MAX_TRIALS:
        raise ValueError(f"max_armijo = {K}: must be in 1..{_lib.MAX_TRIALS}")
    alltime, linear = optim == "alltime" or snap, increment == "linear"
    ctx, n, Nt, dt, tl = prob.ctx, prob.n, prob.num_steps, prob.dt, prob.tlen
    uhat = np.asarray(uhat, dtype=np.float64).ravel()
    if uhat.size != (tl if alltime else n):
        raise ValueError(f"target of {uhat.size} values, expected {tl if alltime else n} for optim='{optim}'")
    c0 = np.asarray(c0, dtype=np.float64).ravel()
    if c0.size != tl:
        raise ValueError(f"c0 of {c0.size} values, expected {tl}")
    if g is not None and np.asarray(g).size != tl:
        raise ValueError(f"g of {np.asarray(g).size} values, expected {tl}")
    u0 = np.asarray(u0, dtype=np.float64).ravel()
    if u0.size != n:
        raise ValueError(f"u0 of {u0.size} values, expected {n}")
    dkw = _direction_kw(prob, c0, control_time, control_space)
    bufs = []

    def alloc(count, zero=True):
        a = ctx.zeros(count) if zero else ctx.empty(count)
        bufs.append(a)
        return a

    try:
        u, p, d, c = alloc(tl), alloc(tl), alloc(tl), alloc(tl, False).upload(c0)
        u.upload(np.concatenate([u0, np.zeros(tl - n)]))
        uh = alloc(uhat.size, False).upload(uhat)
        gd = None if g is None else alloc(tl, False).upload(g)
        src = c if gd is None else alloc(tl, False)
        if linear:
            w = alloc(tl)
        else:
            cB, uB, ckB, uhB = alloc(K * tl, False), alloc(K * tl), alloc(K * tl, False), alloc(K * uhat.size, False)
            srcB = cB if gd is None else alloc(K * tl, False)
            for k in range(K):
                uB.copy_from(u, n, dst_off=k * tl)              # level 0 of every trial state = u0
                uhB.copy_from(uh, uhat.size, dst_off=k * uhat.size)
        cost = lambda uu, cc: float(prob.cost(uu, uh, cc, beta, optim, batch=1, obs=obs, **sbk, **smk)[0])
        J_ref = 10 * cost(u, c)                                 # alltime_exact.py:212 / finaltime.py:170
        hist = dict(cost=[], cost_state=[], armijo_k=[], step=[], stop_crit=[], stop_crit2=[], armijo_margin=[],
                    wall=[], wall0=time.perf_counter())
        svals = [s0 * (1 / 2 ** k) for k in range(K)]
        stop1 = stop2 = np.inf
        while ((stop2 >= tol) or (stop == "both" and stop1 >= tol)) and len(hist["cost"]) < max_iters:
            if gd is not None:
                ctx.axpby(tl, 1.0, gd, 1.0, c, src)
            prob.state(src, u, batch=1)
            hist["cost_state"].append(cost(u, c))
            if snap or sbk:
                prob.adjoint_state(u, uh, p, optim, batch=1, obs=obs, **sbk)
            else:
                prob.adjoint_state(u, uh, p, optim, batch=1)
            prob.descent_direction(c, p, beta, d, **dkw, **smk)
            if linear:
                prob.sensitivity(d, w)
                J, dist = ctx.linear_trial_costs(u, w, uh, c, d, s0, K, c_lower, c_upper, beta, Nt, dt, optim)
            else:
                ctx.source_trials(c, d, s0, K, c_lower, c_upper, tl, cB, None if gd is None else srcB, g=gd)
                prob.state(srcB, uB, batch=K)
                J = prob.cost(uB, uhB, cB, beta, optim, batch=K, obs=obs, **sbk, **smk)
                for k in range(K):
                    ckB.copy_from(c, tl, dst_off=k * tl)
                dist = ctx.l2_norm_sq_Q(cB, ckB, Nt, dt, batch=K)
            margins = []
            for k, s in enumerate(svals):
                acc = k
                margins.append((float(J[k]) - J_ref + gam / s * float(dist[k])) / abs(J_ref))
                if J[k] - J_ref <= -gam / s * dist[k]:
                    break
            J_acc, dist_acc = float(J[acc]), float(dist[acc])
            if sbk:
                _record_bounds(prob, hist, acc)
            if smk:
                _record_smooth(prob, hist, acc)
            nc = float(ctx.l2_norm_sq_Q(c, None, Nt, dt)[0])
            stop1 = dist_acc / nc if nc > 0 else np.inf
            stop2 = abs(J_ref - J_acc) / abs(J_ref)
            if linear:
                ctx.project_control(c, svals[acc], d, c_lower, c_upper, c, tl)     # = the fused kernel's c_acc, bitwise
            else:
                c.copy_from(cB, tl, src_off=acc * tl)
            for key, v in (("cost", J_acc), ("armijo_k", acc + 1), ("step", svals[acc]), ("stop_crit", stop1),
                           ("stop_crit2", stop2), ("armijo_margin", margins), ("wall", time.perf_counter())):
                hist[key].append(v)
            J_ref = J_acc
        hist["iterations"] = len(hist["cost"])
        hist["armijo_margin_min"] = min((abs(m) for ms in hist["armijo_margin"] for m in ms), default=None)
        return u.download(), p.download(), c.download(), hist
    finally:
        for a in bufs:
            a.free()


def source_control_errors(mesh: SquareMeshP1, u, c, p, exact, dx, dt, iterations=0):
    """The error table of advection_FCT_PDECO_alltime_exact.py:333-440 (host NumPy).  ``exact(t)`` returns a dict with
    the manufactured fields "u", "c", "p" at time t in vertex order.  Per level i < num_steps, u is compared at level
    i + 1 and c, p at level i (the adjoint and control are one step behind), each in vertex order: the Euclidean error,
    relative to the exact field and weighted by dx.  Returns the maxima over the levels, ``iterations`` and the script's
    CSV line (:440)."""
    v2d = mesh.vertex_to_dof
    n = v2d.size
    lv = lambda a, i: np.asarray(a, dtype=np.float64)[i * n:(i + 1) * n][v2d]      # level i, vertex order
    num_steps = np.asarray(u).size // n - 1
    E = {k: [] for k in ("u", "c", "p")}
    R = {k: [] for k in ("u", "c", "p")}
    for i in range(num_steps):
        exU, exP = exact((i + 1) * dt), exact(i * dt)
        for key, comp, ex in (("u", lv(u, i + 1), exU["u"]), ("c", lv(c, i), exP["c"]), ("p", lv(p, i), exP["p"])):
            ex = np.asarray(ex, dtype=np.float64).reshape(n)
            e = np.linalg.norm(ex - comp)
            E[key].append(e)
            R[key].append(e / np.linalg.norm(ex))
    out = {f"rel_{k}": max(R[k]) for k in R}
    out.update({f"werr_{k}": dx * max(E[k]) for k in E})
    out["iterations"] = int(iterations)
    vals = [out["rel_u"], out["rel_c"], out["rel_p"], out["werr_u"], out["werr_c"], out["werr_p"]]
    out["csv"] = " , ".join(str(float(v)) for v in vals) + f" , {int(iterations)}"
    return out


# ---------------------------------------------------------------------------------------------- projected L-BFGS
# An extension (no reference call): the loops above are steepest descent in the L2(Q) metric; these keep their sweeps,
# costs and Armijo test and replace the direction by a limited-memory quasi-Newton one on the free set of the box.
def two_loop_coefficients(G, k):
    """The L-BFGS two-loop recursion on coefficient vectors over F = [s_1..s_k, y_1..y_k, g] (oldest pair first), every
    inner product read from the Gram matrix ``G`` of F: pair i takes part iff G[s_i, y_i] > 0, rho_i = 1 / G[s_i, y_i],
    and the initial scaling is gamma = G[s, y] / G[y, y] of the newest pair that takes part (1 if none does).  Returns
    ``(r, pairs that took part)`` with H g = F r."""
    J = 2 * k + 1
    q = np.zeros(J)
    q[2 * k] = 1.0
    part = [i for i in range(k) if G[i, k + i] > 0]
    alpha = {}
    for i in reversed(part):
        alpha[i] = (G[i] @ q) / G[i, k + i]
        q[k + i] -= alpha[i]
    gamma = G[part[-1], k + part[-1]] / G[k + part[-1], k + part[-1]] if part else 1.0
    r = gamma * q
    for i in part:
        b = (G[k + i] @ r) / G[i, k + i]
        r[i] += alpha[i] - b
    return r, len(part)


class LimitedMemory:
    """A ring of up to ``memory`` pairs of device trajectories s_i = c_{k+1} - c_k, y_i = g_{k+1} - g_k (``tl`` doubles
    each; g the L2(Q) Riesz representative of the gradient) and the quasi-Newton direction they give for a control with
    box constraints.  A pair is stored only if, unmasked, <s, y>_Q > 1e-10 sqrt(<s, s>_Q <y, y>_Q).

    :meth:`direction` is three launches and one read-back of J*J doubles, J = 2 pairs + 1, whatever the memory: the free
    set (``Context.free_set``), the Gram matrix of F = [s.., y.., g] masked to it (``Context.q_gram``), the two-loop
    recursion on the host in coefficient space (:func:`two_loop_coefficients`) and one combination of F
    (``Context.q_combine``): -H g on the free set, -g on the bound set.  The mask's bytes are read back as well, for
    ``free_fraction``.  ``dt`` scales the inner product (the direction does not depend on it).  :meth:`close` frees the
    ring."""
    PAIR_TOL = 1e-10

    def __init__(self, ctx: Context, tl: int, memory: int, dt: float = 1.0):
        self.ctx, self.tl, self.memory, self.dt = ctx, int(tl), int(memory), float(dt)
        if not 0 <= self.memory <= (_lib.MAX_GRAM_FIELDS - 1) // 2:
            raise ValueError(f"memory = {memory}: must be in 0..{(_lib.MAX_GRAM_FIELDS - 1) // 2}")
        if ctx.n < 1 or self.tl % ctx.n:
            raise ValueError(f"tl = {tl}: must be (num_steps + 1) * n with n = {ctx.n}")
        self.num_steps = self.tl // ctx.n - 1
        # memory + 1 slots: a candidate pair is formed in the spare one and takes the oldest pair's place only if stored
        self._slots = [(ctx.empty(self.tl), ctx.empty(self.tl)) for _ in range(self.memory + 1 if self.memory else 0)]
        self._ring = []                 # slot indices, oldest first
        self._mask = ctx.empty((self.tl + 7) // 8)      # tl bytes
        self.free_fraction = 1.0

    @property
    def pairs(self):
        return len(self._ring)

    def drop(self):
        self._ring = []

    def _gram(self, fields, mask=None):
        """the Gram matrix of ``fields`` in the memory's inner product (here L2(Q))"""
        return self.ctx.q_gram(fields, self.num_steps, self.dt, mask=mask)

    def _free_set(self, c, g, c_lower, c_upper):
        self.ctx.free_set(c, g, c_lower, c_upper, self.tl, self._mask)

    def push(self, c, c_old, g, g_old) -> bool:
        """Forms s = c - c_old, y = g - g_old and stores the pair if it passes the curvature test."""
        if not self.memory:
            return False
        spare = next(i for i in range(self.memory + 1) if i not in self._ring)
        s, y = self._slots[spare]
        self.ctx.axpby(self.tl, 1.0, c, -1.0, c_old, s)
        self.ctx.axpby(self.tl, 1.0, g, -1.0, g_old, y)
        G = self._gram([s, y])
        if not G[0, 1] > self.PAIR_TOL * np.sqrt(G[0, 0] * G[1, 1]):
            return False
        self._ring.append(spare)
        if len(self._ring) > self.memory:
            del self._ring[0]
        return True

    def direction(self, c, g, c_lower, c_upper, out) -> str:
        """out = the direction at the control ``c`` with gradient ``g``; returns "qn" when pairs took part, else "g"
        (out = -g).  If the quasi-Newton direction is not a descent direction on the free set the ring is dropped and
        out = -g.  ``free_fraction`` is then the share of free values."""
        ctx, tl, k = self.ctx, self.tl, len(self._ring)
        self._free_set(c, g, c_lower, c_upper)
        F = [self._slots[i][0] for i in self._ring] + [self._slots[i][1] for i in self._ring] + [g]
        G = self._gram(F, mask=self._mask)
        r, took = two_loop_coefficients(G, k)
        m = np.empty(tl, dtype=np.uint8)
        _lib.check(ctx.handle, _lib.lib.femfct_memcpy_d2h(ctx.handle, m.ctypes.data, dptr(self._mask), tl))
        self.free_fraction = float(m.mean())
        if not r @ G[:, -1] > 0:
            self.drop()
            ctx.q_combine([g], [-1.0], tl, out)
            return "g"
        ctx.q_combine(F, -r, tl, out, mask=self._mask, fallback=g, fallback_scale=-1.0)
        return "qn" if took else "g"

    def close(self):
        for s, y in self._slots:
            s.free()
            y.free()
        self._slots, self._ring = [], []
        self._mask.free()


class OmegaLimitedMemory(LimitedMemory):
    """:class:`LimitedMemory` for one-level fields of n values in the inner product a^T M b of ``l2_norm_sq_Omega`` (the
    initial state of :func:`initial_state_solidbody`): the Gram matrices come from ``Context.omega_gram`` (L2(Q)'s
    trapezoid weights are not defined for one level), the two-loop recursion and the combination are unchanged.  A caller
    that has filled :attr:`mask` for the (v, g) it is about to pass (``Context.initial_gradient`` writes it with g) sets
    ``mask_ready``; :meth:`direction` then launches no free-set kernel."""

    def __init__(self, ctx: Context, memory: int):
        super().__init__(ctx, ctx.n, memory, 1.0)
        self.mask_ready = False

    @property
    def mask(self):
        return self._mask

    def _gram(self, fields, mask=None):
        return self.ctx.omega_gram(fields, mask=mask)

    def _free_set(self, c, g, c_lower, c_upper):
        if not self.mask_ready:
            super()._free_set(c, g, c_lower, c_upper)
        self.mask_ready = False


def _lbfgs_iterate(ctx, lm, tl, c, g, bufs, J0, gradient, search, take, c_lower, c_upper, max_iters, gam, s0, K, stop):
    """The iteration both L-BFGS loops share.  ``gradient()`` fills g at the current (c, u); ``search(dir, J, svals,
    margins)`` looks at the trials c_t = clip(c + s_t dir) in order and returns ``(t, J_t, ||c_t - c||^2_Q, trials
    looked at)`` of the first that passes the Armijo test (t None: none did); ``take(t)`` makes trial t the iterate;
    ``stop(J, J_t, dist)`` ends the loop after an accepted step."""
    dirv, c_old, g_old = bufs
    hist = dict(cost=[], armijo_k=[], step=[], rel_change=[], armijo_margin=[], used=[], pairs=[], free_fraction=[],
                sweeps=[], wall=[], wall0=time.perf_counter(), cost0=J0, stalled=False)
    svals = [s0 * (1 / 2 ** k) for k in range(K)]
    J, sweeps, have_old = J0, 1, False
    for _ in range(max_iters):
        gradient()
        sweeps += 1
        if have_old:
            lm.push(c, c_old, g, g_old)
        used = lm.direction(c, g, c_lower, c_upper, dirv)
        pairs, free = lm.pairs, lm.free_fraction
        margins = []
        while True:
            t, Jt, dist, looked = search(dirv, J, svals, margins)
            sweeps += looked
            if t is not None or used != "qn":
                break
            lm.drop()                               # no quasi-Newton trial passed: -g within the same iteration
            ctx.q_combine([g], [-1.0], tl, dirv)
            used = "g"
        if t is None:
            hist["stalled"] = True
            break
        c_old.copy_from(c, tl)
        g_old.copy_from(g, tl)
        have_old = True
        take(t)
        for key, v in (("cost", Jt), ("armijo_k", t + 1), ("step", svals[t]), ("rel_change", abs(J - Jt) / abs(J)),
                       ("armijo_margin", margins), ("used", used), ("pairs", pairs), ("free_fraction", free),
                       ("sweeps", sweeps), ("wall", time.perf_counter())):
            hist[key].append(v)
        ended = stop(J, Jt, dist)
        J = Jt
        if ended:
            break
    hist["iterations"] = len(hist["cost"])
    hist["armijo_margin_min"] = min((abs(m) for ms in hist["armijo_margin"] for m in ms), default=None)
    return hist


def _first_accepted(J, dist, J_k, svals, gam, margins):
    """the first trial with J_t - J_k <= -gam/s_t dist_t among the evaluated ones: (t or None, trials looked at)"""
    for t, s in enumerate(svals[:len(J)]):
        margins.append((float(J[t]) - J_k + gam / s * float(dist[t])) / abs(J_k))
        if J[t] - J_k <= -gam / s * dist[t]:
            return t, t + 1
    return None, len(J)


def lbfgs_solidbody(prob: SolidBodyDrift, u0, uhat, c0, beta, c_lower, c_upper, iters, memory=5, gam=1e-4, s0=1.0,
                    max_armijo=10, speculative=True, tol=None, optim="finaltime", obs=None, control_time=None,
                    state_bounds=None, smoothness=None, control_space=None):
    """Projected L-BFGS descent for the drift-control problem: the sweeps, cost, direction kernels and Armijo test of
    :func:`pgd_solidbody` with the direction of a :class:`LimitedMemory` of ``memory`` pairs.  Per iteration, at the
    control c with u = S(c) and J = J(u, c):

        adjoint(c, u) -> g = -descent_direction (projected with ``control_time``) -> push the pair of the previous
        accepted step -> dir -> trials c_t = clip(c + s0/2^t dir): accept the first with
        J(c_t) - J <= -gam/s_t ||c_t - c||^2_Q

    If no quasi-Newton trial is accepted the ring is dropped and -g is searched within the same iteration; if that
    fails too the loop stops with ``history["stalled"] = True``.  There is no unconditional first step (this is a new
    loop, not a restatement of a script), so an accepted cost never exceeds the previous one.  ``memory=0`` is plain
    projected gradient with this search.  ``speculative=True`` evaluates the ``max_armijo`` trials as one batch, as
    pgd_solidbody does.  With ``control_time`` s, y, g and the free set are constant on every interval, so the iterates
    stay piecewise constant bit for bit; with ``control_space`` they are constant on every zone and zero where no zone
    lies, likewise.  ``optim``, ``obs``, ``tol``, ``state_bounds``, ``smoothness``: as in pgd_solidbody.

    Returns ``(u, p, c, history)``; history: ``cost``, ``armijo_k``, ``armijo_margin`` (every trial looked at, the
    quasi-Newton ones first), ``used`` ("qn" / "g"), ``pairs``, ``free_fraction``, ``sweeps`` (state and adjoint sweeps so
    far, counting the trials a sequential search looks at), ``step``, ``rel_change``, ``wall``, ``cost0``, ``stalled``."""
    snap = _need_obs(optim, obs)
    sbk = _bounds_kw(prob, state_bounds)
    smk = _smooth_kw(smoothness)
    alltime = optim == "alltime" or snap
    ctx, n, Nt, dt, tl = prob.ctx, prob.n, prob.num_steps, prob.dt, prob.tlen
    K = int(max_armijo)
    if K < 1:
        raise ValueError(f"max_armijo = {max_armijo}: must be >= 1")
    u0 = np.asarray(u0, dtype=np.float64).ravel()
    if u0.size != n:
        raise ValueError(f"u0 of {u0.size} values, expected {n}")
    c0 = np.asarray(c0, dtype=np.float64).ravel()
    if c0.size != tl:
        raise ValueError(f"c0 of {c0.size} values, expected {tl}")
    uhat = np.asarray(uhat, dtype=np.float64).ravel()
    if uhat.size != (tl if alltime else n):
        raise ValueError(f"target of {uhat.size} values, expected {tl if alltime else n} for optim='{optim}'")
    dkw = _direction_kw(prob, c0, control_time, control_space)
    B = K if speculative else 1
    lm = LimitedMemory(ctx, tl, memory, dt)
    bufs = []

    def alloc(count, zero=True):
        a = ctx.zeros(count) if zero else ctx.empty(count)
        bufs.append(a)
        return a

    try:
        u, p, d, g, rhs = alloc(tl), alloc(tl), alloc(tl), alloc(tl), alloc(tl, False)
        c = alloc(tl, False).upload(c0)
        qn_bufs = (alloc(tl, False), alloc(tl, False), alloc(tl, False))
        uh = alloc(uhat.size, False).upload(uhat)
        uhB = alloc(B * uhat.size, False)
        cB, uB, ckB = alloc(B * tl), alloc(B * tl), alloc(B * tl, False)
        u0d = alloc(n, False).upload(u0)
        u.copy_from(u0d, n)
        for k in range(B):
            uhB.copy_from(uh, uhat.size, dst_off=k * uhat.size)
            uB.copy_from(u0d, n, dst_off=k * tl)          # level 0 of every trial trajectory = the initial condition
        cost = lambda uu, hh, cc, b: prob.cost(uu, hh, cc, beta, optim, batch=b, obs=obs, **sbk, **smk)
        prob.forward(c, u, batch=1)
        J0 = float(cost(u, uh, c, 1)[0])
        bstat = {}

        def gradient():
            prob.adjoint(c, u, uh, p, optim, batch=1, obs=obs, **sbk)
            prob.descent_direction(c, u, p, beta, d, scratch=rhs, **dkw, **smk)
            ctx.axpby(tl, -1.0, d, 0.0, None, g)

        def search(dirv, J_k, svals, margins):
            if speculative:
                for k, s in enumerate(svals):
                    ctx.project_control(c, s, dirv, c_lower, c_upper, cB.ptr + 8 * k * tl, tl)
                    ckB.copy_from(c, tl, dst_off=k * tl)
                prob.forward(cB, uB, batch=B)
                J = cost(uB, uhB, cB, B)
                dist = ctx.l2_norm_sq_Q(cB, ckB, Nt, dt, batch=B)
                t, looked = _first_accepted(J, dist, J_k, svals, gam, margins)
                return t, (None if t is None else float(J[t])), (None if t is None else float(dist[t])), looked
            for k, s in enumerate(svals):
                ctx.project_control(c, s, dirv, c_lower, c_upper, cB, tl)
                prob.forward(cB, uB, batch=1)
                J = cost(uB, uh, cB, 1)
                dist = ctx.l2_norm_sq_Q(cB, c, Nt, dt)
                t, _ = _first_accepted(J, dist, J_k, [s], gam, margins)
                if t is not None:
                    return k, float(J[0]), float(dist[0]), k + 1
            return None, None, None, len(svals)

        def take(t):
            off = t * tl if speculative else 0
            c.copy_from(cB, tl, src_off=off)
            u.copy_from(uB, tl, src_off=off)
            if sbk:         # (the last cost pass is that of the search that found t)
                _record_bounds(prob, bstat, t if speculative else 0)
            if smk:
                _record_smooth(prob, bstat, t if speculative else 0)

        stop = lambda J, Jt, dist: tol is not None and abs(J - Jt) / abs(J) < tol
        hist = _lbfgs_iterate(ctx, lm, tl, c, g, qn_bufs, J0, gradient, search, take, c_lower, c_upper, int(iters), gam,
                              s0, K, stop)
        hist.update(bstat)
        return u.download(), p.download(), c.download(), hist
    finally:
        lm.close()
        for a in bufs:
            a.free()


def lbfgs_source_control(prob: LinearSourceControl, u0, uhat, c0, beta, c_lower, c_upper, g=None, optim="alltime",
                         memory=5, gam=1e-4, s0=1.0, max_armijo=10, tol=1e-4, max_iters=1000, stop="both", obs=None,
                         control_time=None, state_bounds=None, smoothness=None, control_space=None):
    """Projected L-BFGS descent for the linear source-control problem (:class:`LinearSourceControl`,
    :class:`LinearReactionSourceControl`): the iteration of :func:`lbfgs_solidbody` with the gradient
    -descent_direction = beta c - p, the trial controls and sources of ``femfct_source_trials`` and the ``max_armijo``
    trial states as one batched sweep, as ``pgd_source_control(increment="resolve")`` runs them.  The Armijo test
    compares with the cost of the current iterate, J(S(g + c_k), c_k) (no unconditional first step and no 10 J start
    value).  The loop runs while stop_crit2 = |J_k - J_acc| / |J_k| >= tol, or (stop="both")
    stop_crit = ||c_{k+1} - c_k||^2_Q / ||c_k||^2_Q >= tol, and fewer than ``max_iters`` iterations have run.
    Arguments (``smoothness`` and ``control_space`` included) and return value as pgd_source_control; the history is lbfgs_solidbody's with
    ``stop_crit``, ``stop_crit2``."""
    snap = _need_obs(optim, obs)
    sbk = _bounds_kw(prob, state_bounds)
    smk = _smooth_kw(smoothness)
    if stop not in ("both", "cost"):
        raise ValueError(f"Invalid value for 'stop': '{stop}'. Must be one of ['both', 'cost'].")
    K = int(max_armijo)
    if not 1 <= K <= _lib.MAX_TRIALS:
        raise ValueError(f"max_armijo = {K}: must be in 1..{_lib.MAX_TRIALS}")
    alltime = optim == "alltime" or snap
    ctx, n, Nt, dt, tl = prob.ctx, prob.n, prob.num_steps, prob.dt, prob.tlen
    uhat = np.asarray(uhat, dtype=np.float64).ravel()
    if uhat.size != (tl if alltime else n):
        raise ValueError(f"target of {uhat.size} values, expected {tl if alltime else n} for optim='{optim}'")
    c0 = np.asarray(c0, dtype=np.float64).ravel()
    if c0.size != tl:
        raise ValueError(f"c0 of {c0.size} values, expected {tl}")
    if g is not None and np.asarray(g).size != tl:
        raise ValueError(f"g of {np.asarray(g).size} values, expected {tl}")
    u0 = np.asarray(u0, dtype=np.float64).ravel()
    if u0.size != n:
        raise ValueError(f"u0 of {u0.size} values, expected {n}")
    dkw = _direction_kw(prob, c0, control_time, control_space)
    lm = LimitedMemory(ctx, tl, memory, dt)
    bufs = []

    def alloc(count, zero=True):
        a = ctx.zeros(count) if zero else ctx.empty(count)
        bufs.append(a)
        return a

    try:
        u, p, d, gr, c = alloc(tl), alloc(tl), alloc(tl), alloc(tl), alloc(tl, False).upload(c0)
        u.upload(np.concatenate([u0, np.zeros(tl - n)]))
        qn_bufs = (alloc(tl, False), alloc(tl, False), alloc(tl, False))
        uh = alloc(uhat.size, False).upload(uhat)
        gd = None if g is None else alloc(tl, False).upload(g)
        src = c if gd is None else alloc(tl, False)
        cB, uB, ckB, uhB = alloc(K * tl, False), alloc(K * tl), alloc(K * tl, False), alloc(K * uhat.size, False)
        srcB = cB if gd is None else alloc(K * tl, False)
        for k in range(K):
            uB.copy_from(u, n, dst_off=k * tl)              # level 0 of every trial state = u0
            uhB.copy_from(uh, uhat.size, dst_off=k * uhat.size)
        if gd is not None:
            ctx.axpby(tl, 1.0, gd, 1.0, c, src)
        prob.state(src, u, batch=1)
        J0 = float(prob.cost(u, uh, c, beta, optim, batch=1, obs=obs, **sbk, **smk)[0])
        crit = dict(stop_crit=[], stop_crit2=[])

        def gradient():
            if snap or sbk:
                prob.adjoint_state(u, uh, p, optim, batch=1, obs=obs, **sbk)
            else:
                prob.adjoint_state(u, uh, p, optim, batch=1)
            prob.descent_direction(c, p, beta, d, **dkw, **smk)
            ctx.axpby(tl, -1.0, d, 0.0, None, gr)

        def search(dirv, J_k, svals, margins):
            ctx.source_trials(c, dirv, s0, K, c_lower, c_upper, tl, cB, None if gd is None else srcB, g=gd)
            prob.state(srcB, uB, batch=K)
            J = prob.cost(uB, uhB, cB, beta, optim, batch=K, obs=obs, **sbk, **smk)
            for k in range(K):
                ckB.copy_from(c, tl, dst_off=k * tl)
            dist = ctx.l2_norm_sq_Q(cB, ckB, Nt, dt, batch=K)
            t, looked = _first_accepted(J, dist, J_k, svals, gam, margins)
            return t, (None if t is None else float(J[t])), (None if t is None else float(dist[t])), looked

        def take(t):
            c.copy_from(cB, tl, src_off=t * tl)
            u.copy_from(uB, tl, src_off=t * tl)
            if sbk:
                _record_bounds(prob, crit, t)
            if smk:
                _record_smooth(prob, crit, t)

        def stop_test(J, Jt, dist):
            nc = float(ctx.l2_norm_sq_Q(qn_bufs[1], None, Nt, dt)[0])      # (c_old: the control the step started from)
            crit["stop_crit"].append(dist / nc if nc > 0 else np.inf)
            crit["stop_crit2"].append(abs(J - Jt) / abs(J))
            return not (crit["stop_crit2"][-1] >= tol or (stop == "both" and crit["stop_crit"][-1] >= tol))

        hist = _lbfgs_iterate(ctx, lm, tl, c, gr, qn_bufs, J0, gradient, search, take, c_lower, c_upper, int(max_iters),
                              gam, s0, K, stop_test)
        hist.update(crit)
        return u.download(), p.download(), c.download(), hist
    finally:
        lm.close()
        for a in bufs:
            a.free()


# ---------------------------------------------------------------------------------------------- L1-sparse controls
# An extension (no reference call): the cost gains alpha ||c||_{1,h}, the nodal-quadrature L1(Q) norm
# dt sum_l w_l sum_i ml_i |c_{l,i}| (trapezoid level weights, lumped mass), and the loops above's projected step
# becomes a proximal one, c_t = clip(soft_threshold(c - s_t g, s_t alpha)): value by value the exact prox of
# s_t alpha |.| + the box indicator.  It is the nodal discretisation of the continuous proximal-gradient step, the same
# approximation the loops above make when they clip value by value under the consistent-mass metric.
def _prox_iterate(ctx, tl, Nt, dt, c, cB, J0, gradient, trial_costs, take, alpha, c_lower, c_upper, max_iters, gam, s0, K,
                  tol, budget=None, proj=None):
    """The iteration both proximal-gradient loops share.  ``gradient()`` runs the adjoint at the current (c, u) and returns
    the device direction d = -g; ``trial_costs(d)`` writes the K trial controls into ``cB``, runs their states as one
    batch and returns the K smooth costs J(S(c_t), c_t); ``take(t)`` makes trial t the iterate.  With a ``budget`` the
    residual trial is ``budget_trials``' and ``trial_costs`` leaves its trials' multipliers and search rounds in
    ``proj["lam"]``, ``proj["rounds"]``; everything else is the same code."""
    hist = dict(cost=[], cost_smooth=[], l1=[], nonzero_fraction=[], residual=[], armijo_k=[], step=[], armijo_margin=[],
                rel_change=[], sweeps=[], wall=[], wall0=time.perf_counter(), stalled=False)
    if budget is not None:
        hist.update(multiplier=[], budget_used=[], projection_rounds=[])
    svals = [s0 * (1 / 2 ** k) for k in range(K)]
    F = J0 + alpha * float(ctx.l1_norm_Q(c, Nt, dt)[0])
    hist["cost0"] = F
    sweeps = 1
    for _ in range(max_iters):
        d = gradient()
        sweeps += 1
        if budget is None:
            ctx.prox_trials(c, d, 1.0, 1, alpha, c_lower, c_upper, tl, cB)   # prox(c - g; tau = alpha), in trial 0's place
        else:
            ctx.budget_trials(c, d, 1.0, 1, alpha, budget, c_lower, c_upper, Nt, dt, cB)
        residual = float(ctx.l2_norm_sq_Q(cB, c, Nt, dt)[0])
        J = trial_costs(d)
        l1, dist, nnz = ctx.sparse_trial_stats(cB, c, K, Nt, dt)
        margins, found = [], None
        for t, s in enumerate(svals):
            Ft = float(J[t]) + alpha * float(l1[t])
            margins.append((Ft - F + gam / s * float(dist[t])) / abs(F))
            if Ft - F <= -gam / s * float(dist[t]):
                found = t
                break
        sweeps += len(margins)
        if found is None:
            hist["stalled"] = True
            break
        take(found)
        for key, v in (("cost", Ft), ("cost_smooth", float(J[found])), ("l1", float(l1[found])),
                       ("nonzero_fraction", int(nnz[found]) / tl), ("residual", residual), ("armijo_k", found + 1),
                       ("step", svals[found]), ("armijo_margin", margins), ("rel_change", abs(F - Ft) / abs(F)),
                       ("sweeps", sweeps), ("wall", time.perf_counter())):
            hist[key].append(v)
        if budget is not None:
            hist["multiplier"].append(float(proj["lam"][found]))
            hist["budget_used"].append(float(l1[found]) / budget)
            hist["projection_rounds"].append(int(proj["rounds"][found]))
        F = Ft
        if tol is not None and hist["rel_change"][-1] < tol:
            break
    hist["iterations"] = len(hist["cost"])
    hist["armijo_margin_min"] = min((abs(m) for ms in hist["armijo_margin"] for m in ms), default=None)
    return hist


def _need_budget(budget, c_lower, c_upper):
    if not (np.isfinite(budget) and budget > 0):
        raise ValueError(f"budget = {budget}: must be finite and > 0 (None: no budget; for 'unbounded' pass a large number)")
    if not c_lower <= 0 <= c_upper:
        raise ValueError(f"a budget needs a box that contains 0, got [{c_lower}, {c_upper}]")


def _need_within_budget(ctx, c, Nt, dt, budget):
    """the loops start from a control inside the budget (they never project the start themselves)"""
    l1 = float(ctx.l1_norm_Q(c, Nt, dt)[0])
    if not l1 <= budget * (1 + 1e-12):
        raise ValueError(f"c0 has ||c0||_(1,h) = {l1} > budget = {budget}: start from project_onto_budget(prob, c0, budget, "
                         f"c_lower, c_upper)[0]")


def project_onto_budget(prob, c, budget, c_lower, c_upper):
    """The projection of the control trajectory ``c`` (host array, (num_steps + 1) * n values) onto
    {c_lower <= c <= c_upper, ||c||_{1,h} <= budget}, c_lower <= 0 <= c_upper, in the nodal-quadrature inner product
    sum dt w_l ml_i a_{l,i} b_{l,i} -- the metric in which the prox of the L1 loops is taken, not the consistent-mass Q
    metric of their Armijo distance.  Returns ``(P, lam)``: P = clip(soft_threshold(c, lam)) as a host array and the
    multiplier, 0.0 where clip(c) is within the budget.  ``Context.budget_trials`` with d = None, K = 1."""
    c = np.asarray(c, dtype=np.float64).ravel()
    if c.size != prob.tlen:
        raise ValueError(f"c of {c.size} values, expected {prob.tlen}")
    _need_budget(budget, c_lower, c_upper)
    ctx = prob.ctx
    cd, out = ctx.array(c), ctx.empty(prob.tlen)
    try:
        lam, _, _ = ctx.budget_trials(cd, None, 1.0, 1, 0.0, budget, c_lower, c_upper, prob.num_steps, prob.dt, out)
        return out.download(), float(lam[0])
    finally:
        cd.free()
        out.free()


def _prox_arguments(prob, u0, uhat, c0, g, alpha, c_lower, c_upper, max_armijo, optim, obs, control_time, budget=None):
    """the argument validation of the L-BFGS loops, alpha >= 0 and the budget's; returns (K, u0, uhat, c0) as flat float64
    arrays"""
    snap = _need_obs(optim, obs)
    alltime = optim == "alltime" or snap
    n, Nt, tl = prob.n, prob.num_steps, prob.tlen
    K = int(max_armijo)
    if not 1 <= K <= _lib.MAX_TRIALS:
        raise ValueError(f"max_armijo = {K}: must be in 1..{_lib.MAX_TRIALS}")
    if not alpha >= 0:
        raise ValueError(f"alpha = {alpha}: must be >= 0")
    if not c_lower <= c_upper:
        raise ValueError(f"c_lower = {c_lower} > c_upper = {c_upper}")
    if budget is not None:
        _need_budget(budget, c_lower, c_upper)
    uhat = np.asarray(uhat, dtype=np.float64).ravel()
    if uhat.size != (tl if alltime else n):
        raise ValueError(f"target of {uhat.size} values, expected {tl if alltime else n} for optim='{optim}'")
    c0 = np.asarray(c0, dtype=np.float64).ravel()
    if c0.size != tl:
        raise ValueError(f"c0 of {c0.size} values, expected {tl}")
    if g is not None and np.asarray(g).size != tl:
        raise ValueError(f"g of {np.asarray(g).size} values, expected {tl}")
    u0 = np.asarray(u0, dtype=np.float64).ravel()
    if u0.size != n:
        raise ValueError(f"u0 of {u0.size} values, expected {n}")
    if control_time is not None:
        control_time.need(c0, n, Nt)
    return K, u0, uhat, c0


def prox_solidbody(prob: SolidBodyDrift, u0, uhat, c0, beta, alpha, c_lower, c_upper, iters, gam=1e-4, s0=1.0,
                   max_armijo=10, tol=None, optim="finaltime", obs=None, control_time=None, budget=None):
    """Proximal gradient descent for the drift-control problem with an L1 term: minimises
    F(c) = J(S(c), c) + alpha ||c||_{1,h} over the box, J the cost of :func:`lbfgs_solidbody` and
    ||c||_{1,h} = dt sum_l w_l sum_i ml_i |c_{l,i}| (``Context.l1_norm_Q``).  Per iteration, at the control c with
    u = S(c) and F:

        adjoint(c, u) -> g = -descent_direction (projected with ``control_time``) -> residual
        ||prox(c - g; alpha) - c||^2_Q -> trials c_t = clip(soft_threshold(c - s_t g, s_t alpha)), s_t = s0/2^t, their
        ``max_armijo`` states as one batched sweep: accept the first with F(c_t) - F <= -gam/s_t ||c_t - c||^2_Q

    If no trial is accepted the loop stops with ``history["stalled"] = True`` and c unchanged; there is no unconditional
    first step, so an accepted cost never exceeds the previous one.  ``alpha = 0`` is ``lbfgs_solidbody(memory=0)``.
    ``tol`` stops on rel_change = |F - F_t| / |F|.  With ``control_time`` c and g are constant on every interval and the
    prox acts value by value, so the iterates stay piecewise constant bit for bit.  ``optim``, ``obs``: as in
    pgd_solidbody.

    Returns ``(u, p, c, history)``; history: ``cost`` (F), ``cost_smooth`` (J), ``l1``, ``nonzero_fraction``, ``residual``
    (at the control the iteration started from), ``armijo_k``, ``step``, ``armijo_margin`` (every trial looked at,
    (F_t - F + gam/s_t dist_t) / |F|), ``armijo_margin_min``, ``rel_change``, ``sweeps`` (as the L-BFGS loops count
    them), ``wall``, ``wall0``, ``cost0``, ``stalled``, ``iterations``.  Every list has one entry per accepted step: an
    iteration that stalls, as in the L-BFGS loops, leaves no entry (its residual and the margins of its ``max_armijo``
    rejected trials are not kept, so a run that stalls at once has ``armijo_margin_min`` None).

    ``budget`` B (None: none; else finite and > 0, with c_lower <= 0 <= c_upper) adds the hard constraint
    ||c||_{1,h} <= B: the residual trial and the K trials become ``Context.budget_trials``',
    c_t = clip(soft_threshold(c - s_t g, s_t alpha + lam_t)) with lam_t >= 0 the smallest value that meets the budget --
    the prox of s_t alpha ||.||_{1,h} + the indicator of {box, ||.||_{1,h} <= B} in the nodal-quadrature metric (weights
    dt w_l ml_i), the metric the prox above is already taken in.  The Armijo test, its consistent-mass distance
    ||c_t - c||^2_Q, the statistics and the batched sweep are unchanged; ``alpha = 0`` is projected gradient onto the
    budget set.  One lam per trial and a value-by-value map: with ``control_time`` the iterates stay piecewise constant
    bit for bit.  c0 must satisfy ||c0||_{1,h} <= B (1 + 1e-12) (ValueError; see :func:`project_onto_budget`).  The
    history gains ``multiplier`` (lam of the accepted trial; 0.0: the budget was slack), ``budget_used`` (l1 / B) and
    ``projection_rounds``.  Not combined with zones, the L-BFGS, ensemble, lockstep or initial-state loops."""
    K, u0, uhat, c0 = _prox_arguments(prob, u0, uhat, c0, None, alpha, c_lower, c_upper, max_armijo, optim, obs, control_time,
                                      budget)
    ctx, n, Nt, dt, tl = prob.ctx, prob.n, prob.num_steps, prob.dt, prob.tlen
    bufs = []

    def alloc(count, zero=True):
        a = ctx.zeros(count) if zero else ctx.empty(count)
        bufs.append(a)
        return a

    try:
        u, p, d, rhs = alloc(tl), alloc(tl), alloc(tl), alloc(tl, False)
        c = alloc(tl, False).upload(c0)
        if budget is not None:
            _need_within_budget(ctx, c, Nt, dt, budget)
        uh = alloc(uhat.size, False).upload(uhat)
        uhB = alloc(K * uhat.size, False)
        cB, uB = alloc(K * tl), alloc(K * tl)
        u0d = alloc(n, False).upload(u0)
        u.copy_from(u0d, n)
        for k in range(K):
            uhB.copy_from(uh, uhat.size, dst_off=k * uhat.size)
            uB.copy_from(u0d, n, dst_off=k * tl)          # level 0 of every trial trajectory = the initial condition
        cost = lambda uu, hh, cc, b: prob.cost(uu, hh, cc, beta, optim, batch=b, obs=obs)
        prob.forward(c, u, batch=1)
        J0 = float(cost(u, uh, c, 1)[0])
        proj = {}

        def gradient():
            prob.adjoint(c, u, uh, p, optim, batch=1, obs=obs)
            if control_time is None:
                prob.descent_direction(c, u, p, beta, d, scratch=rhs)
            else:
                prob.descent_direction(c, u, p, beta, d, scratch=rhs, control_time=control_time)
            return d

        def trial_costs(dirv):
            if budget is None:
                ctx.prox_trials(c, dirv, s0, K, alpha, c_lower, c_upper, tl, cB)
            else:
                proj["lam"], _, proj["rounds"] = ctx.budget_trials(c, dirv, s0, K, alpha, budget, c_lower, c_upper, Nt, dt, cB)
            prob.forward(cB, uB, batch=K)
            return cost(uB, uhB, cB, K)

        def take(t):
            c.copy_from(cB, tl, src_off=t * tl)
            u.copy_from(uB, tl, src_off=t * tl)

        hist = _prox_iterate(ctx, tl, Nt, dt, c, cB, J0, gradient, trial_costs, take, alpha, c_lower, c_upper, int(iters),
                             gam, s0, K, tol, budget, proj)
        return u.download(), p.download(), c.download(), hist
    finally:
        for a in bufs:
            a.free()


def prox_source_control(prob: LinearSourceControl, u0, uhat, c0, beta, alpha, c_lower, c_upper, g=None, optim="alltime",
                        gam=1e-4, s0=1.0, max_armijo=10, tol=None, max_iters=1000, obs=None, control_time=None, budget=None):
    """Proximal gradient descent for the linear source-control problem (:class:`LinearSourceControl`,
    :class:`LinearReactionSourceControl`) with an L1 term: the iteration of :func:`prox_solidbody` with the gradient
    -descent_direction = beta c - p, the trial controls and sources g + c_t of ``femfct_prox_trials`` in one launch and the
    ``max_armijo`` trial states as one batched sweep, as :func:`lbfgs_source_control` runs them.  ``alpha = 0`` is
    ``lbfgs_source_control(memory=0)``'s iteration.  Runs ``max_iters`` iterations, or until rel_change < ``tol``.
    Arguments as lbfgs_source_control; return value, history and ``budget`` (the control budget ||c||_{1,h} <= B: projection
    in the nodal-quadrature metric, Armijo distance in the consistent-mass Q norm) as prox_solidbody."""
    K, u0, uhat, c0 = _prox_arguments(prob, u0, uhat, c0, g, alpha, c_lower, c_upper, max_armijo, optim, obs, control_time,
                                      budget)
    snap = _need_obs(optim, obs)
    ctx, n, Nt, dt, tl = prob.ctx, prob.n, prob.num_steps, prob.dt, prob.tlen
    bufs = []

    def alloc(count, zero=True):
        a = ctx.zeros(count) if zero else ctx.empty(count)
        bufs.append(a)
        return a

    try:
        u, p, d, c = alloc(tl), alloc(tl), alloc(tl), alloc(tl, False).upload(c0)
        u.upload(np.concatenate([u0, np.zeros(tl - n)]))
        uh = alloc(uhat.size, False).upload(uhat)
        gd = None if g is None else alloc(tl, False).upload(g)
        src = c if gd is None else alloc(tl, False)
        cB, uB, uhB = alloc(K * tl, False), alloc(K * tl), alloc(K * uhat.size, False)
        srcB = cB if gd is None else alloc(K * tl, False)
        for k in range(K):
            uB.copy_from(u, n, dst_off=k * tl)              # level 0 of every trial state = u0
            uhB.copy_from(uh, uhat.size, dst_off=k * uhat.size)
        if gd is not None:
            ctx.axpby(tl, 1.0, gd, 1.0, c, src)
        if budget is not None:
            _need_within_budget(ctx, c, Nt, dt, budget)
        prob.state(src, u, batch=1)
        J0 = float(prob.cost(u, uh, c, beta, optim, batch=1, obs=obs)[0])
        proj = {}

        def gradient():
            prob.adjoint_state(u, uh, p, optim, batch=1, obs=obs) if snap else prob.adjoint_state(u, uh, p, optim, batch=1)
            if control_time is None:
                prob.descent_direction(c, p, beta, d)
            else:
                prob.descent_direction(c, p, beta, d, control_time=control_time)
            return d

        def trial_costs(dirv):
            if budget is None:
                ctx.prox_trials(c, dirv, s0, K, alpha, c_lower, c_upper, tl, cB, None if gd is None else srcB, g=gd)
            else:
                proj["lam"], _, proj["rounds"] = ctx.budget_trials(c, dirv, s0, K, alpha, budget, c_lower, c_upper, Nt, dt, cB,
                                                                   None if gd is None else srcB, g=gd)
            prob.state(srcB, uB, batch=K)
            return prob.cost(uB, uhB, cB, beta, optim, batch=K, obs=obs)

        def take(t):
            c.copy_from(cB, tl, src_off=t * tl)
            u.copy_from(uB, tl, src_off=t * tl)

        hist = _prox_iterate(ctx, tl, Nt, dt, c, cB, J0, gradient, trial_costs, take, alpha, c_lower, c_upper,
                             int(max_iters), gam, s0, K, tol, budget, proj)
        return u.download(), p.download(), c.download(), hist
    finally:
        for a in bufs:
            a.free()


# ---------------------------------------------------------------------------------------------- ensemble drift control
# An extension (no reference call): one control for many scenarios, the sample-average form of control under uncertain
# data.  The scenarios are the batch of every sweep.
class Ensemble:
    """S scenarios of a drift-control problem that share one control: initial conditions ``u0`` (S, n), targets ``uhat``
    (S, n) for final-time tracking, else (S, (num_steps + 1) * n), and ``weights`` pi_s >= 0 (default uniform), finite
    with a positive sum, stored normalised to sum 1.  A scenario of weight 0 is carried along (its state, adjoint and
    cost are computed) and does not enter the cost or the gradient."""

    def __init__(self, u0, uhat, weights=None):
        u0 = np.array(u0, dtype=np.float64)
        uhat = np.array(uhat, dtype=np.float64)
        if u0.ndim != 2 or u0.shape[0] < 1:
            raise ValueError(f"u0 of shape {u0.shape}, expected (S, n)")
        if uhat.ndim != 2 or uhat.shape[0] != u0.shape[0]:
            raise ValueError(f"uhat of shape {uhat.shape} for {u0.shape[0]} scenarios, expected (S, n) or (S, tlen)")
        S = u0.shape[0]
        w = np.full(S, 1.0 / S) if weights is None else np.array(weights, dtype=np.float64).ravel()
        if w.size != S:
            raise ValueError(f"{w.size} weights for {S} scenarios")
        if not (np.all(np.isfinite(w)) and np.all(w >= 0) and w.sum() > 0):
            raise ValueError("weights must be finite and >= 0 with a positive sum")
        if weights is not None:
            w = w / w.sum()
        self.u0, self.uhat, self.weights = u0, uhat, w
        for a in (u0, uhat, w):
            a.setflags(write=False)

    @property
    def S(self):
        return self.u0.shape[0]


def ensemble_solidbody(prob: SolidBodyDrift, scenarios: Ensemble, c0, beta, c_lower, c_upper, iters, memory=0, gam=1e-4,
                       s0=1.0, max_armijo=10, tol=None, optim="finaltime", obs=None, control_time=None, state_bounds=None):
    """Projected gradient (``memory=0``) or projected L-BFGS (``memory>0``) descent for one drift control that serves the
    S ``scenarios`` (an :class:`Ensemble`),

        J(c) = sum_s pi_s T_s(u_s(c)) + beta/2 ||c||^2_Q,      T_s = 1/2 sum_n cost_w[n] (u_{s,n} - uhat_{s,n})^T Mw (..)

    with the tracking term of :class:`Observations` (``optim`` "finaltime" / "alltime" are its corners, "snapshots" takes
    ``obs``).  It is the iteration of :func:`lbfgs_solidbody` (``_lbfgs_iterate``, :class:`LimitedMemory`) with three
    callbacks of its own.  Every scenario has its own FCT state and FCT adjoint; the limiter is nonlinear, so the weights
    are not folded into the adjoint loads and enter where the gradient is formed:

        gradient   one adjoint sweep of S members with the shared control, rhs_l = -(beta M c_l + sum_s pi_s
                   assemble(p_{s,l} (b.grad u_{s,l}) v dx)) in one launch, d = ChebSI(rhs) -- num_steps + 1 mass solves
                   whatever S is (K with ``control_time``) -- and g = -d
        search     sequential: trial t is clip(c + s_t dir), one forward sweep of S members with the shared control, and
                   one fused cost pass; it stops at the first accepted trial
        take       the S accepted trajectories become the iterate

    There is no speculative mode: the scenarios are the batch, and a trial sweep is already S members wide.  State bounds
    are not carried by this loop (``state_bounds`` raises).  S is at most ``_lib.MAX_MEMBERS``.

    Returns ``(u, p, c, history)`` with u, p of shape (S, tlen); history holds the keys of lbfgs_solidbody (``sweeps``
    counts batched sweeps) and, per accepted iterate, ``scenario_costs`` (the S values T_s), ``worst`` (their maximum over
    the scenarios of non-zero weight) and ``control_cost`` (beta/2 ||c||^2_Q); ``scenario_costs0`` holds the T_s at ``c0``."""
    if state_bounds is not None:
        raise ValueError("state_bounds: state bounds are not carried by the ensemble loop (use lbfgs_solidbody per scenario)")
    if not isinstance(scenarios, Ensemble):
        raise ValueError("scenarios must be an Ensemble")
    _need_obs(optim, obs)
    ctx, n, Nt, dt, tl = prob.ctx, prob.n, prob.num_steps, prob.dt, prob.tlen
    levels = Nt + 1
    S, w = scenarios.S, scenarios.weights
    if S * 1 > _lib.MAX_MEMBERS:
        raise ValueError(f"{S} scenarios: at most {_lib.MAX_MEMBERS} per ensemble")
    K = int(max_armijo)
    if K < 1:
        raise ValueError(f"max_armijo = {max_armijo}: must be >= 1")
    if scenarios.u0.shape[1] != n:
        raise ValueError(f"u0 of {scenarios.u0.shape[1]} values per scenario, expected {n}")
    hsize = n if optim == "finaltime" else tl
    if scenarios.uhat.shape[1] != hsize:
        raise ValueError(f"targets of {scenarios.uhat.shape[1]} values per scenario, expected {hsize} for optim='{optim}'")
    c0 = np.asarray(c0, dtype=np.float64).ravel()
    if c0.size != tl:
        raise ValueError(f"c0 of {c0.size} values, expected {tl}")
    if control_time is not None:
        control_time.need(c0, n, Nt)
    lm = LimitedMemory(ctx, tl, memory, dt)
    bufs = []

    def alloc(count, zero=True):
        a = ctx.zeros(count) if zero else ctx.empty(count)
        bufs.append(a)
        return a

    try:
        u, p, uB = alloc(S * tl), alloc(S * tl), alloc(S * tl)
        d, g, rhs, cB = alloc(tl), alloc(tl), alloc(tl, False), alloc(tl)
        c = alloc(tl, False).upload(c0)
        qn_bufs = (alloc(tl, False), alloc(tl, False), alloc(tl, False))
        u0d = alloc(S * n, False).upload(scenarios.u0.ravel())
        uh = alloc(S * hsize, False).upload(scenarios.uhat.ravel())
        for s in range(S):      # level 0 of every scenario's trajectories = its initial condition
            u.copy_from(u0d, n, dst_off=s * tl, src_off=s * n)
            uB.copy_from(u0d, n, dst_off=s * tl, src_off=s * n)
        # the sweeps and the cost are the snapshot ones: final-time and all-time through their Observations corners
        # (the final-time targets copied once to level num_steps of a trajectory-sized buffer the problem keeps)
        ob, target = prob._corner(optim, obs, uh, S)
        theta, cost_w, window = prob.obs_device(ob)
        cur = dict(u=u, uB=uB)
        stats = {}

        def costs(uu, cc, cref=None):
            return ctx.ensemble_costs(uu, target, cost_w, cc, w, beta, Nt, dt, window=window, cref=cref)

        prob.forward(c, u, batch=S, c_shared=True)
        last = costs(u, c)
        J0 = last[1]

        def gradient():
            ctx.solidbody_adjoint_obs(prob.Arot, c, cur["u"], target, theta, ob.tau, window, p, Nt, dt, prob.eps,
                                      prob.rot_scale, prob.drift, S, True)
            ctx.ensemble_drift_gradient_rhs(c, cur["u"], p, w, beta, rhs, levels, prob.drift)
            if control_time is None:
                ctx.chebsi(rhs, d, 20, 0.5, 2.0, batch=levels)
            else:
                prob._projected_solve(control_time, rhs, d, 1)
            ctx.axpby(tl, -1.0, d, 0.0, None, g)

        def search(dirv, J_k, svals, margins):
            for k, s in enumerate(svals):
                ctx.project_control(c, s, dirv, c_lower, c_upper, cB, tl)
                prob.forward(cB, cur["uB"], batch=S, c_shared=True)
                T, J, dist = costs(cur["uB"], cB, cref=c)
                t, _ = _first_accepted([J], [dist], J_k, [s], gam, margins)
                if t is not None:
                    stats["last"] = (T, J)
                    return k, J, dist, k + 1
            return None, None, None, len(svals)

        def take(t):
            c.copy_from(cB, tl)
            cur["u"], cur["uB"] = cur["uB"], cur["u"]       # the S accepted trajectories: a swap (level 0 is the same)
            T, J = stats["last"]
            track = 0.0
            for ws, Ts in zip(w[w != 0], T[w != 0]):
                track = track + float(ws * Ts)
            stats.setdefault("scenario_costs", []).append(T.copy())
            stats.setdefault("worst", []).append(float(T[w != 0].max()))
            stats.setdefault("control_cost", []).append(J - track)       # (beta/2 ||c||^2_Q up to the rounding of J)

        stop = lambda J, Jt, dist: tol is not None and abs(J - Jt) / abs(J) < tol
        hist = _lbfgs_iterate(ctx, lm, tl, c, g, qn_bufs, J0, gradient, search, take, c_lower, c_upper, int(iters), gam,
                              s0, K, stop)
        for key in ("scenario_costs", "worst", "control_cost"):
            hist[key] = stats.get(key, [])
        hist["scenario_costs0"] = last[0]
        return (cur["u"].download().reshape(S, tl), p.download().reshape(S, tl), c.download(), hist)
    finally:
        lm.close()
        for a in bufs:
            a.free()


# ---------------------------------------------------------------------------------------------- initial-state recovery
# An extension (no reference call): every loop above recovers a control under a fixed initial condition; this one keeps the
# control fixed and recovers the initial condition from later observations of the transported field (4D-Var).
def initial_state_solidbody(prob: SolidBodyDrift, c, uhat, v0, beta0, v_lower, v_upper, iters, background=None, memory=5,
                            gam=1e-4, s0=1.0, max_armijo=10, tol=None, optim="finaltime", obs=None, speculative=True):
    """Projected gradient (``memory=0``) or projected L-BFGS descent on the initial state v of the solid-body problem
    under the fixed control trajectory ``c``,

        J(v) = T(u(v)) + beta0/2 (v - v_b)^T M (v - v_b),      u(v) = the forward sweep from u_0 = v under c,

    T the tracking term of ``optim`` ("finaltime" / "alltime", or "snapshots" with ``obs``; ``uhat`` shaped as for
    :func:`lbfgs_solidbody`), ``background`` v_b (None: 0), box ``[v_lower, v_upper]``.  It is the iteration of
    :func:`lbfgs_solidbody` (``_lbfgs_iterate``) on one level of n values with the inner product a^T M b
    (:class:`OmegaLimitedMemory`) and three callbacks of its own:

        gradient   the adjoint sweep p of u(v) (the drift loops' call for the mode) and g = beta0 (v - v_b) - p_0 with the
                   free set, one launch: p(T) = uhat - u(T), so -p_0 is the L2(Omega) representative of the tracking
                   term's gradient and no mass solve is needed.  p is an FCT discretisation of the continuous adjoint:
                   g is inexact, as every gradient of this project is
        search     trials v_t = clip(v + s0/2^t dir), the first with J(v_t) - J <= -gam/s_t ||v_t - v||^2_M accepted.
                   ``speculative``: the ``max_armijo`` trials are one ``initial_trials`` launch into level 0 of a batch,
                   one batched forward sweep under the shared control, one tracking-cost call and one
                   ``initial_trial_stats`` read-back, whatever ``max_armijo`` is; else one trial at a time
        take       the accepted member's trajectory becomes u (a copy, no second sweep)

    ``max_armijo`` may not exceed ``prob.batch`` when ``speculative``.  Argument errors raise ValueError before any launch.

    Returns ``(u, p, v, history)``; history has the keys of lbfgs_solidbody's plus ``tracking`` and ``background``, the two
    terms of J at every accepted iterate (``tracking0`` / ``background0`` at ``v0``)."""
    snap = _need_obs(optim, obs)
    ctx, n, Nt, dt, tl = prob.ctx, prob.n, prob.num_steps, prob.dt, prob.tlen
    K = int(max_armijo)
    if K < 1:
        raise ValueError(f"max_armijo = {max_armijo}: must be >= 1")
    if speculative and K > min(prob.batch, _lib.MAX_MEMBERS):
        raise ValueError(f"max_armijo = {K}: a speculative search needs a problem of batch >= max_armijo "
                         f"(prob.batch = {prob.batch}, at most {_lib.MAX_MEMBERS})")
    beta0 = float(beta0)
    if not (np.isfinite(beta0) and beta0 >= 0):
        raise ValueError(f"beta0 = {beta0}: must be finite and >= 0")
    v_lower, v_upper = float(v_lower), float(v_upper)
    if not v_lower <= v_upper:
        raise ValueError(f"v_lower = {v_lower} > v_upper = {v_upper}")
    c = np.asarray(c, dtype=np.float64).ravel()
    if c.size != tl:
        raise ValueError(f"c of {c.size} values, expected {tl}")
    v0 = np.asarray(v0, dtype=np.float64).ravel()
    if v0.size != n:
        raise ValueError(f"v0 of {v0.size} values, expected {n}")
    if background is not None:
        background = np.asarray(background, dtype=np.float64).ravel()
        if background.size != n:
            raise ValueError(f"background of {background.size} values, expected {n}")
    uhat = np.asarray(uhat, dtype=np.float64).ravel()
    hsize = n if optim == "finaltime" else tl
    if uhat.size != hsize:
        raise ValueError(f"target of {uhat.size} values, expected {hsize} for optim='{optim}'")
    if snap:
        obs.check(Nt, n)
    B = K if speculative else 1
    lm = OmegaLimitedMemory(ctx, memory)
    bufs = []

    def alloc(count, zero=True):
        a = ctx.zeros(count) if zero else ctx.empty(count)
        bufs.append(a)
        return a

    try:
        u, p, uB = alloc(tl), alloc(tl), alloc(B * tl)
        cd = alloc(tl, False).upload(c)
        v = alloc(n, False).upload(v0)
        g = alloc(n)
        qn_bufs = (alloc(n, False), alloc(n, False), alloc(n, False))
        vb = None if background is None else alloc(n, False).upload(background)
        uh = alloc(hsize, False).upload(uhat)
        uhB = alloc(B * hsize, False)
        for k in range(B):
            uhB.copy_from(uh, hsize, dst_off=k * hsize)
        # the tracking term of every mode is the snapshot cost: final-time and all-time through their Observations corners
        ob, target = prob._corner(optim, obs, uhB, B)
        _, cost_w, window = prob.obs_device(ob)
        tracking = lambda uu, b: ctx.obs_cost(uu, target, cost_w, Nt, window, batch=b)
        u.copy_from(v, n)
        prob.forward(cd, u, batch=1)
        T0 = float(tracking(u, 1)[0])
        B0 = (0.5 * beta0) * float(ctx.l2_norm_sq_Omega(v, vb)[0])
        last, terms = {}, dict(tracking=[], background=[])

        def gradient():
            prob.adjoint(cd, u, uh, p, optim, batch=1, obs=obs)
            ctx.initial_gradient(p, v, beta0, g, vb=vb, v_lower=v_lower, v_upper=v_upper, mask=lm.mask)
            lm.mask_ready = True

        def evaluate(dirv, steps):
            """(J, dist, T, background term) of the trials v + steps[k] dir, one batched sweep"""
            b = len(steps)
            ctx.initial_trials(v, dirv, steps, v_lower, v_upper, uB, Nt)
            prob.forward(cd, uB, batch=b, c_shared=True)
            T = tracking(uB, b)
            st = ctx.initial_trial_stats(uB, v, b, Nt, vb=vb)
            Bg = (0.5 * beta0) * st[:, 0]
            return T + Bg, st[:, 1], T, Bg

        def search(dirv, J_k, svals, margins):
            if speculative:
                J, dist, T, Bg = evaluate(dirv, svals)
                t, looked = _first_accepted(J, dist, J_k, svals, gam, margins)
                if t is None:
                    return None, None, None, looked
                last["terms"] = (float(T[t]), float(Bg[t]))
                return t, float(J[t]), float(dist[t]), looked
            for k, s in enumerate(svals):
                J, dist, T, Bg = evaluate(dirv, [s])
                t, _ = _first_accepted(J, dist, J_k, [s], gam, margins)
                if t is not None:
                    last["terms"] = (float(T[0]), float(Bg[0]))
                    return k, float(J[0]), float(dist[0]), k + 1
            return None, None, None, len(svals)

        def take(t):
            off = t * tl if speculative else 0
            u.copy_from(uB, tl, src_off=off)
            v.copy_from(uB, n, src_off=off)
            terms["tracking"].append(last["terms"][0])
            terms["background"].append(last["terms"][1])

        stop = lambda J, Jt, dist: tol is not None and abs(J - Jt) / abs(J) < tol
        hist = _lbfgs_iterate(ctx, lm, n, v, g, qn_bufs, T0 + B0, gradient, search, take, v_lower, v_upper, int(iters), gam,
                              s0, K, stop)
        hist.update(terms, tracking0=T0, background0=B0)
        return u.download(), p.download(), v.download(), hist
    finally:
        lm.close()
        for a in bufs:
            a.free()
