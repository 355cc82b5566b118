"""Thin object layer over the C ABI: one ``Context`` = one femfct_ctx (one GPU,
one HIP stream), ``DeviceArray`` = a float64 device buffer.

Any object exposing ``data_ptr()`` (e.g. a CUDA/ROCm ``torch.Tensor`` of dtype
float64) is accepted wherever a device array is expected, so callers that
already hold HBM-resident tensors hand them over without a copy.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import lib, check, StepInfo


def _host_ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def _as_f64(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64)


class DeviceArray:
    """float64 buffer in HBM owned by a Context."""

    def __init__(self, ctx: "Context", count: int):
        self.ctx = ctx
        self.count = int(count)
        ptr = C.c_void_p()
        check(ctx.handle, lib.femfct_malloc(ctx.handle, C.byref(ptr), self.count * 8))
        self.ptr = ptr.value
        ctx._arrays.add(self)

    def data_ptr(self) -> int:
        return self.ptr

    def upload(self, host) -> "DeviceArray":
        h = _as_f64(host).reshape(-1)
        if h.size != self.count:
            raise ValueError(f"upload: host array has {h.size} elements, device array {self.count}")
        check(self.ctx.handle, lib.femfct_memcpy_h2d(self.ctx.handle, self.ptr, _host_ptr(h), h.nbytes))
        return self

    def download(self, out: np.ndarray | None = None) -> np.ndarray:
        if out is None:
            out = np.empty(self.count, dtype=np.float64)
        if out.size != self.count or out.dtype != np.float64 or not out.flags.c_contiguous:
            raise ValueError("download: need a C-contiguous float64 array of matching size")
        check(self.ctx.handle, lib.femfct_memcpy_d2h(self.ctx.handle, _host_ptr(out), self.ptr, out.nbytes))
        return out

    def zero(self) -> "DeviceArray":
        check(self.ctx.handle, lib.femfct_memset0(self.ctx.handle, self.ptr, self.count * 8))
        return self

    def copy_from(self, other, count=None, dst_off=0, src_off=0) -> "DeviceArray":
        count = self.count if count is None else int(count)
        check(self.ctx.handle, lib.femfct_memcpy_d2d(self.ctx.handle, self.ptr + 8 * dst_off,
                                                      dptr(other) + 8 * src_off, count * 8))
        return self

    def free(self):
        if self.ptr:
            lib.femfct_free(self.ctx.handle, self.ptr)
            self.ptr = 0
            self.ctx._arrays.discard(self)


def _wind_scale(wind_scale, num_steps) -> np.ndarray:
    ws = _as_f64(wind_scale).reshape(-1)
    if ws.size != num_steps + 1:
        raise ValueError(f"wind_scale: {ws.size} values, expected num_steps + 1 = {num_steps + 1} (s(t_0) .. s(t_Nt))")
    return ws


def _growth(growth) -> np.ndarray:
    g = _as_f64(growth).reshape(-1)
    if g.size != 3:
        raise ValueError(f"growth: {g.size} values, expected the three coefficients (r0, r1, r2) of u (r0 + r1 u + r2 u^2)")
    return g


MISFITS = {"nodal": 0, "mass": 1}


class DeviceObs:
    """Snapshot observations of the state variables of a PDE-system sweep, on the device: ``theta_u`` / ``theta_v``
    (num_steps + 1 doubles; None: the variable is not observed and its target may be None), the terminal weights
    ``tau_u`` / ``tau_v`` and one ``window`` (n doubles or None) for both.  See solvers.Observations."""

    def __init__(self, theta_u=None, tau_u=0.0, theta_v=None, tau_v=0.0, window=None):
        self.theta_u, self.tau_u, self.theta_v, self.tau_v, self.window = theta_u, float(tau_u), theta_v, float(tau_v), window


def _misfit(misfit) -> int:
    if misfit not in MISFITS:
        raise ValueError(f"Invalid value for 'misfit': '{misfit}'. Must be one of {sorted(MISFITS)}.")
    return MISFITS[misfit]


def dptr(x) -> int:
    """device address of a DeviceArray / torch tensor / raw int (None -> 0)."""
    if x is None:
        return 0
    if isinstance(x, int):
        return x
    return int(x.data_ptr())


class Context:
    """femfct_ctx wrapper.  ``Context.n`` / ``.W`` describe the registered pattern."""

    def __init__(self, device_id: int = 0):
        h = C.c_void_p()
        code = lib.femfct_create(C.byref(h), int(device_id))
        if code != _lib.OK:
            raise _lib.FemFctError(code, f"femfct_create(device {device_id}) failed: no usable HIP device")
        self.handle = h
        self.device_id = int(device_id)
        self._arrays = set()
        self.mesh = None

    # -- lifetime ----------------------------------------------------------
    def close(self):
        if getattr(self, "handle", None):
            for a in list(self._arrays):
                a.free()
            lib.femfct_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- settings ----------------------------------------------------------
    def set_solver(self, solver=_lib.SOLVER_JACOBI, rel_tol=1e-13, max_iters=400):
        check(self.handle, lib.femfct_set_solver(self.handle, solver, rel_tol, max_iters))

    def set_graphs(self, enable: bool):
        check(self.handle, lib.femfct_set_graphs(self.handle, int(bool(enable))))

    def launch_info(self) -> dict:
        """Bandwidth-regime kernels of the most recent step / sweep (diagnostic): Jacobi launch kind, its walkers, interior
        patches per side of the split Chebyshev launch, halo depth."""
        out = (C.c_int32 * 4)()
        check(self.handle, lib.femfct_launch_info(self.handle, out))
        kinds = {0: "other", 1: "k_strip4_jacobi", 2: "k_strip4_jacobi_walk", 3: "k_strip_jacobi_pair_walk"}
        return {"jacobi_kernel": kinds.get(out[0], "?"), "jacobi_walkers": int(out[1]), "cheb_interior_patches": int(out[2]),
                "halo": int(out[3])}

    def tile_trim_info(self) -> dict:
        """What the latency-regime tile launchers made of FEMFCT_TILE_TRIM (diagnostic): the bits in effect, launches enqueued
        with the owning-wave epilogue and with write-through stores, partial slots per array of the last deferred-test solve
        (0: one per workgroup)."""
        out = (C.c_int32 * 4)()
        check(self.handle, lib.femfct_tile_trim_info(self.handle, out))
        return {"mask": int(out[0]), "wave_launches": int(out[1]), "wt_launches": int(out[2]), "wave_slots": int(out[3])}

    def graph_replay_active(self) -> bool:
        """False while sweeps are enqueued kernel by kernel: graphs off, per-class profiling, or rocprofv3 attached."""
        v = C.c_int(0)
        check(self.handle, lib.femfct_graph_replay_active(self.handle, C.byref(v)))
        return bool(v.value)

    def rotation_derived(self) -> bool:
        """True when the most recent solid-body sweep evaluated the rotation operator from the node positions."""
        v = C.c_int(0)
        check(self.handle, lib.femfct_rotation_derived(self.handle, C.byref(v)))
        return bool(v.value)

    KERNEL_CLASSES = ("build_low", "jacobi", "dudt_rhs", "cheb", "flux", "limit", "assemble", "other")

    def set_profiling(self, enable: bool):
        check(self.handle, lib.femfct_set_profiling(self.handle, int(bool(enable))))

    def profile_report(self):
        """{class: (total_ms, launches)} of the kernels run since profiling was enabled / last report."""
        ms = np.zeros(8)
        cnt = np.zeros(8, dtype=np.int32)
        check(self.handle, lib.femfct_profile_report(self.handle, _host_ptr(ms), _host_ptr(cnt), 8))
        return {k: (float(ms[i]), int(cnt[i])) for i, k in enumerate(self.KERNEL_CLASSES)}

    def set_fusion(self, strips=True, tiles=True):
        check(self.handle, lib.femfct_set_fusion(self.handle, int(bool(strips)), int(bool(tiles))))

    def patch_walkers(self, batch=1, sweeps=36) -> int:
        """Persistent workgroups per batch member of the bandwidth-regime Jacobi / Chebyshev launches (0: one
        workgroup per patch)."""
        return lib.femfct_patch_walkers(self.handle, int(batch), int(sweeps))

    def kernel_regime(self, batch=1) -> int:
        """_lib.REGIME_*: the Jacobi / Chebyshev kernel family a step with ``batch`` members runs."""
        return lib.femfct_kernel_regime(self.handle, int(batch))

    def lowop_nonzero_fraction(self) -> float:
        """share of the low-order operator's off-diagonals the bandwidth-regime Jacobi launches load (1.0: all)"""
        out = C.c_double(1.0)
        check(self.handle, lib.femfct_lowop_nonzero_fraction(self.handle, C.byref(out)))
        return float(out.value)

    def uses_bandwidth_tiles(self, batch=1) -> bool:
        return self.kernel_regime(batch) == _lib.REGIME_PATCH64

    def synchronize(self):
        check(self.handle, lib.femfct_synchronize(self.handle))

    @property
    def stream(self) -> int:
        return lib.femfct_stream(self.handle) or 0

    # -- memory --------------------------------------------------------------
    def empty(self, count) -> DeviceArray:
        return DeviceArray(self, count)

    def zeros(self, count) -> DeviceArray:
        return DeviceArray(self, count).zero()

    def array(self, host) -> DeviceArray:
        h = _as_f64(host).reshape(-1)
        return DeviceArray(self, h.size).upload(h)

    # -- pattern / constant operators -----------------------------------------
    @property
    def n(self) -> int:
        return lib.femfct_n(self.handle)

    @property
    def W(self) -> int:
        return lib.femfct_ell_width(self.handle)

    def set_pattern_csr(self, indptr, indices):
        ip = np.ascontiguousarray(indptr, dtype=np.int32)
        ix = np.ascontiguousarray(indices, dtype=np.int32)
        check(self.handle, lib.femfct_set_pattern_csr(self.handle, ip.size - 1, _host_ptr(ip), _host_ptr(ix)))
        self.mesh = None

    def set_mesh_square(self, a1, a2, n_cells, order=_lib.ORDER_FENICS):
        check(self.handle, lib.femfct_set_mesh_square(self.handle, float(a1), float(a2), int(n_cells), int(order)))

    def ell_cols(self) -> np.ndarray:
        out = np.empty(self.W * self.n, dtype=np.int32)
        check(self.handle, lib.femfct_get_ell_cols(self.handle, _host_ptr(out)))
        return out.reshape(self.W, self.n)

    def set_mass(self, M_csr_vals, ml):
        m = _as_f64(M_csr_vals)
        l = _as_f64(ml)
        check(self.handle, lib.femfct_set_mass(self.handle, _host_ptr(m), _host_ptr(l)))

    def csr_to_ell(self, csr_vals, out: DeviceArray | None = None) -> DeviceArray:
        v = _as_f64(csr_vals)
        if out is None:
            out = self.empty(self.W * self.n)
        check(self.handle, lib.femfct_csr_to_ell(self.handle, _host_ptr(v), dptr(out)))
        return out

    def ell_to_csr(self, ell, nnz: int) -> np.ndarray:
        out = np.empty(int(nnz), dtype=np.float64)
        check(self.handle, lib.femfct_ell_to_csr(self.handle, dptr(ell), _host_ptr(out)))
        return out

    @property
    def mass_ell(self) -> int:
        return lib.femfct_mass_ell(self.handle) or 0

    @property
    def stiffness_ell(self) -> int:
        return lib.femfct_stiffness_ell(self.handle) or 0

    @property
    def lumped_mass(self) -> int:
        return lib.femfct_lumped_mass(self.handle) or 0

    # -- step operator -----------------------------------------------------------
    def fct_step(self, A_ell, u_n, dt, u_out, rhs=None, N_ell=None, N_shared=False, batch=1):
        check(self.handle, lib.femfct_fct_step(self.handle, dptr(A_ell), dptr(N_ell), int(bool(N_shared)),
                                               dptr(rhs), dptr(u_n), float(dt), dptr(u_out), int(batch)))

    def last_step_info(self, batch=1):
        arr = (StepInfo * batch)()
        check(self.handle, lib.femfct_last_step_info(self.handle, arr, int(batch)))
        return [dict(flags=a.flags, solver_iters=a.solver_iters, solver_resid=a.solver_resid,
                     min_rowsum=a.min_rowsum) for a in arr]

    def fct_step_host(self, A_csr_vals, rhs, u_n, dt, N_csr_vals=None):
        a = _as_f64(A_csr_vals)
        u = _as_f64(u_n)
        r = None if rhs is None else _as_f64(rhs)
        nn = None if N_csr_vals is None else _as_f64(N_csr_vals)
        out = np.empty(self.n, dtype=np.float64)
        info = StepInfo()
        check(self.handle, lib.femfct_fct_step_host(
            self.handle, _host_ptr(a), None if nn is None else _host_ptr(nn),
            None if r is None else _host_ptr(r), _host_ptr(u), float(dt), _host_ptr(out), C.byref(info)))
        return out, dict(flags=info.flags, solver_iters=info.solver_iters, solver_resid=info.solver_resid,
                         min_rowsum=info.min_rowsum)

    def chebsi(self, b, y, cheb_iter=20, lmin=0.5, lmax=2.0, batch=1):
        check(self.handle, lib.femfct_chebsi(self.handle, dptr(b), dptr(y), int(cheb_iter), float(lmin),
                                             float(lmax), int(batch)))

    def chebsi_md(self, b, y, md, cheb_iter=20, lmin=0.5, lmax=2.0, batch=1):
        """ChebSI with a preconditioner diagonal of the caller's (not diag(M)); one system (any other batch: ValueError)."""
        check(self.handle, lib.femfct_chebsi_md(self.handle, dptr(b), dptr(y), dptr(md), int(cheb_iter), float(lmin),
                                                float(lmax), int(batch)))

    def artificial_diffusion(self, K_ell, D_ell, batch=1):
        check(self.handle, lib.femfct_artificial_diffusion(self.handle, dptr(K_ell), dptr(D_ell), int(batch)))

    def spmv(self, mat_ell, x, y, alpha=1.0, beta=0.0, batch=1):
        check(self.handle, lib.femfct_spmv(self.handle, dptr(mat_ell), dptr(x), float(alpha), float(beta),
                                           dptr(y), int(batch)))

    # -- structured assembly --------------------------------------------------------
    def quad_points(self, n_cells):
        cnt = n_cells * n_cells * 2 * 6
        xq = np.empty(cnt)
        yq = np.empty(cnt)
        check(self.handle, lib.femfct_mesh_quad_points(self.handle, _host_ptr(xq), _host_ptr(yq)))
        return xq, yq

    def assemble_convection(self, wind_q, scale=1.0, out: DeviceArray | None = None) -> DeviceArray:
        w = _as_f64(wind_q)
        if out is None:
            out = self.empty(self.W * self.n)
        check(self.handle, lib.femfct_assemble_convection(self.handle, _host_ptr(w), float(scale), dptr(out)))
        return out

    def assemble_rotation(self, omega, out: DeviceArray | None = None) -> DeviceArray:
        """``assemble_sparse(dot(wind, grad(v))*u*dx)`` for ``wind = omega * (-x[1], x[0])`` in closed form (equal to
        :meth:`assemble_convection` of that wind up to rounding); the large-mesh step kernels recognise it and derive
        its rows instead of loading them."""
        if out is None:
            out = self.empty(self.W * self.n)
        check(self.handle, lib.femfct_assemble_rotation(self.handle, float(omega), dptr(out)))
        return out

    def drift_gradient_rhs(self, c, u, p, beta, out, levels, drift=(1.0, 1.0)):
        check(self.handle, lib.femfct_drift_gradient_rhs(self.handle, dptr(c), dptr(u), dptr(p), float(beta),
                                                         float(drift[0]), float(drift[1]), dptr(out), int(levels)))

    # -- trajectories ------------------------------------------------------------------
    def solidbody_forward(self, Arot, c_traj, u_traj, num_steps, dt, eps=0.0, rot_scale=1.0,
                          drift=(1.0, 1.0), batch=1, c_shared=False, src_traj=None):
        check(self.handle, lib.femfct_solidbody_forward_src(
            self.handle, dptr(Arot), dptr(c_traj), int(bool(c_shared)), dptr(src_traj), dptr(u_traj), int(num_steps),
            float(dt), float(eps), float(rot_scale), float(drift[0]), float(drift[1]), int(batch)))

    def solidbody_adjoint(self, Arot, c_traj, u_traj, uhat, p_traj, num_steps, dt, eps=0.0, rot_scale=1.0,
                          drift=(1.0, 1.0), alltime=False, batch=1, c_shared=False):
        check(self.handle, lib.femfct_solidbody_adjoint(
            self.handle, dptr(Arot), dptr(c_traj), int(bool(c_shared)), dptr(u_traj), dptr(uhat), dptr(p_traj),
            int(num_steps), float(dt), float(eps), float(rot_scale), float(drift[0]), float(drift[1]),
            int(bool(alltime)), int(batch)))

    def linear_forward_react(self, A, src_traj, g_traj, u_traj, num_steps, dt, eps, batch=1):
        """State / sensitivity sweep with the explicit reaction term: rhs_{n+1} = M src_{n+1} - Mg(g_n) u_n
        (``src_traj`` may be None); ``g_traj`` is one coefficient trajectory for the whole batch."""
        check(self.handle, lib.femfct_linear_forward_react(self.handle, dptr(A), dptr(src_traj), dptr(g_traj), dptr(u_traj),
                                                           int(num_steps), float(dt), float(eps), int(batch)))

    def linear_adjoint_react(self, Aadj, g_traj, u_traj, uhat, p_traj, num_steps, dt, eps, alltime=False, batch=1):
        """Adjoint sweep with the explicit reaction term: rhs_n = -Mg(g_n) p_{n+1} (+ M (uhat_n - u_n) all-time) and the
        operator -Aadj - eps*Ad, ``Aadj = Aa1 + Aa2``."""
        check(self.handle, lib.femfct_linear_adjoint_react(self.handle, dptr(Aadj), dptr(g_traj), dptr(u_traj), dptr(uhat),
                                                           dptr(p_traj), int(num_steps), float(dt), float(eps),
                                                           int(bool(alltime)), int(batch)))

    def react_load(self, src, g, x, out, batch=1):
        """out = M src - Mg(g) x for one level, matrix-free (``src`` may be None); ``g`` is shared by the batch."""
        check(self.handle, lib.femfct_react_load(self.handle, dptr(src), dptr(g), dptr(x), dptr(out), int(batch)))

    # -- snapshot observations: J = 1/2 sum_n w_n (u_n - uhat_n)^T Mw (u_n - uhat_n), Mw = assemble(omega_h*u*v*dx) -------
    def solidbody_adjoint_obs(self, Arot, c_traj, u_traj, uhat_traj, theta, tau, window, p_traj, num_steps, dt, eps=0.0,
                              rot_scale=1.0, drift=(1.0, 1.0), batch=1, c_shared=False):
        """Adjoint sweep tracking the state at chosen levels: p_Nt = tau * omega .* (uhat_Nt - u_Nt), load
        (theta[n]/dt) Mw (uhat_n - u_n).  ``theta``: num_steps + 1 device doubles; ``window``: n device doubles or None."""
        check(self.handle, lib.femfct_solidbody_adjoint_obs(
            self.handle, dptr(Arot), dptr(c_traj), int(bool(c_shared)), dptr(u_traj), dptr(uhat_traj), dptr(theta),
            float(tau), dptr(window), dptr(p_traj), int(num_steps), float(dt), float(eps), float(rot_scale),
            float(drift[0]), float(drift[1]), int(batch)))

    def linear_adjoint_react_obs(self, Aadj, g_traj, u_traj, uhat_traj, theta, tau, window, p_traj, num_steps, dt, eps,
                                 batch=1):
        """The same for the sweep with the explicit reaction term (load ... - Mg(g_n) p_{n+1})."""
        check(self.handle, lib.femfct_linear_adjoint_react_obs(
            self.handle, dptr(Aadj), dptr(g_traj), dptr(u_traj), dptr(uhat_traj), dptr(theta), float(tau), dptr(window),
            dptr(p_traj), int(num_steps), float(dt), float(eps), int(batch)))

    def obs_load(self, a, b, theta, level, dt, out, window=None, batch=1):
        """out = (theta[level]/dt) Mw (a - b) for one level (zeros, a and b unread, where theta[level] == 0)."""
        check(self.handle, lib.femfct_obs_load(self.handle, dptr(a), dptr(b), dptr(theta), int(level), float(dt),
                                               dptr(window), dptr(out), int(batch)))

    def obs_cost(self, u_traj, uhat_traj, cost_w, num_steps, window=None, batch=1) -> np.ndarray:
        """1/2 sum_n cost_w[n] (u_n - uhat_n)^T Mw (u_n - uhat_n) per batch member (``cost_w``: device doubles)."""
        out = np.empty(batch)
        check(self.handle, lib.femfct_obs_cost(self.handle, dptr(u_traj), dptr(uhat_traj), dptr(cost_w), dptr(window),
                                               int(num_steps), int(batch), _host_ptr(out)))
        return out

    # -- state bounds: P = gamma/2 sum_n sigma_n sum_i ml_i ws_i v_{n,i}^2, v = u - clip(u, lower, upper) ----------------
    def solidbody_adjoint_bounds(self, Arot, c_traj, u_traj, uhat_traj, theta, tau, window, lower, upper, gamma, sigma,
                                 window_s, p_traj, num_steps, dt, eps=0.0, rot_scale=1.0, drift=(1.0, 1.0), batch=1,
                                 c_shared=False):
        """:meth:`solidbody_adjoint_obs` with the penalty of the state bounds: p_Nt loses sigma[Nt] gamma ws .* v_Nt, the
        load of level n loses (sigma[n]/dt) gamma ml .* ws .* v_n.  ``lower`` / ``upper`` / ``window_s``: n device doubles
        or None (not both bounds); ``sigma``: num_steps + 1 device doubles."""
        check(self.handle, lib.femfct_solidbody_adjoint_bounds(
            self.handle, dptr(Arot), dptr(c_traj), int(bool(c_shared)), dptr(u_traj), dptr(uhat_traj), dptr(theta),
            float(tau), dptr(window), dptr(lower), dptr(upper), float(gamma), dptr(sigma), dptr(window_s), dptr(p_traj),
            int(num_steps), float(dt), float(eps), float(rot_scale), float(drift[0]), float(drift[1]), int(batch)))

    def linear_adjoint_react_bounds(self, Aadj, g_traj, u_traj, uhat_traj, theta, tau, window, lower, upper, gamma, sigma,
                                    window_s, p_traj, num_steps, dt, eps, batch=1):
        """The same for the sweep with the explicit reaction term."""
        check(self.handle, lib.femfct_linear_adjoint_react_bounds(
            self.handle, dptr(Aadj), dptr(g_traj), dptr(u_traj), dptr(uhat_traj), dptr(theta), float(tau), dptr(window),
            dptr(lower), dptr(upper), float(gamma), dptr(sigma), dptr(window_s), dptr(p_traj), int(num_steps), float(dt),
            float(eps), int(batch)))

    def bound_load(self, uhat, u, theta, sigma, level, dt, lower, upper, gamma, out, window=None, g=None, x=None,
                   window_s=None, batch=1):
        """out = (theta[level]/dt) Mw (uhat - u) [- Mg(g) x] - (sigma[level]/dt) gamma ml .* ws .* v(u) for one level."""
        check(self.handle, lib.femfct_bound_load(self.handle, dptr(uhat), dptr(u), dptr(theta), dptr(sigma), int(level),
                                                 float(dt), dptr(window), dptr(g), dptr(x), dptr(lower), dptr(upper),
                                                 float(gamma), dptr(window_s), dptr(out), int(batch)))

    def bound_cost(self, u_traj, sigma, lower, upper, gamma, num_steps, window_s=None, batch=1) -> np.ndarray:
        """``(batch, 3)``: the penalty P, the largest |v| and the number of v != 0 over the penalised (level, node) pairs
        per batch member (``sigma``: device doubles)."""
        out = np.empty((batch, 3))
        check(self.handle, lib.femfct_bound_cost(self.handle, dptr(u_traj), dptr(sigma), dptr(lower), dptr(upper),
                                                 float(gamma), dptr(window_s), int(num_steps), int(batch), _host_ptr(out)))
        return out

    def assemble_weighted_mass(self, f, out: DeviceArray | None = None) -> DeviceArray:
        """``assemble_sparse(f_h*u*v*dx)`` for the P1 function with the nodal values ``f`` (ELL)."""
        if out is None:
            out = self.empty(self.W * self.n)
        check(self.handle, lib.femfct_assemble_weighted_mass(self.handle, dptr(f), dptr(out)))
        return out

    def traj_info(self, num_steps, batch=1):
        arr = (StepInfo * (num_steps * batch))()
        check(self.handle, lib.femfct_traj_info(self.handle, arr, int(num_steps), int(batch)))
        return dict(flags=np.array([a.flags for a in arr]).reshape(num_steps, batch),
                    solver_iters=np.array([a.solver_iters for a in arr]).reshape(num_steps, batch),
                    solver_resid=np.array([a.solver_resid for a in arr]).reshape(num_steps, batch),
                    min_rowsum=np.array([a.min_rowsum for a in arr]).reshape(num_steps, batch))

    # -- optimisation layer ------------------------------------------------------------
    def l2_norm_sq_Q(self, a, b, num_steps, dt, batch=1) -> np.ndarray:
        out = np.empty(batch)
        check(self.handle, lib.femfct_l2_norm_sq_Q(self.handle, dptr(a), dptr(b), int(num_steps), float(dt),
                                                   _host_ptr(out), int(batch)))
        return out

    def l2_norm_sq_Omega(self, a, b, batch=1) -> np.ndarray:
        out = np.empty(batch)
        check(self.handle, lib.femfct_l2_norm_sq_Omega(self.handle, dptr(a), dptr(b), _host_ptr(out), int(batch)))
        return out

    def cost_functional(self, var1, var1_target, control, num_steps, dt, beta, optim, var2=None,
                        var2_target=None, batch=1) -> np.ndarray:
        if optim not in ("alltime", "finaltime"):
            raise ValueError(f"Invalid value for 'optim': '{optim}'. Must be one of ['alltime', 'finaltime'].")
        out = np.empty(batch)
        check(self.handle, lib.femfct_cost_functional(
            self.handle, dptr(var1), dptr(var1_target), dptr(control), 0, int(num_steps), float(dt), float(beta),
            int(optim == "finaltime"), dptr(var2), dptr(var2_target), _host_ptr(out), int(batch)))
        return out

    def project_control(self, c, s, d, c_lower, c_upper, out, count):
        check(self.handle, lib.femfct_project_control(self.handle, dptr(c), float(s), dptr(d), float(c_lower),
                                                      float(c_upper), dptr(out), int(count)))

    def linear_trial_costs(self, u, w, uhat, c, d, s0, K, c_lower, c_upper, beta, num_steps, dt, optim):
        """Costs J[t] = cost_functional(u + s_t w, uhat, c_t) and distances dist[t] = L2_norm_sq_Q(c_t - c) of the K
        trials s_t = s0 / 2^t, c_t = clip(c + s_t d) of a linear-increment Armijo search, in one fused pass (bitwise the
        materialised trials).  Returns ``(J, dist)``, two host arrays of K values."""
        if optim not in ("alltime", "finaltime"):
            raise ValueError(f"Invalid value for 'optim': '{optim}'. Must be one of ['alltime', 'finaltime'].")
        J, dist = np.empty(max(int(K), 1)), np.empty(max(int(K), 1))
        check(self.handle, lib.femfct_linear_trial_costs(
            self.handle, dptr(u), dptr(w), dptr(uhat), dptr(c), dptr(d), float(s0), int(K), float(c_lower),
            float(c_upper), float(beta), int(num_steps), float(dt), int(optim == "finaltime"), _host_ptr(J),
            _host_ptr(dist)))
        return J, dist

    def source_trials(self, c, d, s0, K, c_lower, c_upper, count, c_out, src_out=None, g=None):
        """c_out[t] = clip(c + s_t d) and src_out[t] = g + c_out[t] (c_out[t] without g) for t < K, one launch; member t
        starts at t*count."""
        check(self.handle, lib.femfct_source_trials(self.handle, dptr(c), dptr(d), dptr(g), float(s0), int(K),
                                                    float(c_lower), float(c_upper), int(count), dptr(c_out),
                                                    dptr(src_out)))

    def trial_controls(self, c, d, steps, P, K, c_lower, c_upper, count, c_out):
        """Lockstep trial controls: c_out[p*K + t] = clip(c[p] + steps[p*K + t] * d[p]) for P problems x K trials (bitwise
        P*K project_control calls), one launch; ``c``, ``d``: P blocks of ``count`` doubles, ``steps``: P*K host values."""
        s = _as_f64(steps).reshape(-1)
        if s.size != int(P) * int(K):
            raise ValueError(f"trial_controls: {s.size} steps for P*K = {int(P) * int(K)} members")
        check(self.handle, lib.femfct_trial_controls(self.handle, dptr(c), dptr(d), _host_ptr(s), int(P), int(K),
                                                     float(c_lower), float(c_upper), int(count), dptr(c_out)))

    def member_costs(self, u, uhat, c, betas, P, K, num_steps, dt, optim, cref=None, uhat_per_problem=False):
        """J[m] = cost_functional(u_m, uhat_p, c_m, beta_p) and dist[m] = L2_norm_sq_Q(c_m - cref_p) of the P*K members
        m = p*K + t of a lockstep batch, one fused pass (bitwise the two calls on each member alone).  ``uhat``: one target
        or, with ``uhat_per_problem``, P; ``cref``: P reference controls or None.  Returns ``(J, dist)``, dist None
        without ``cref``."""
        if optim not in ("alltime", "finaltime"):
            raise ValueError(f"Invalid value for 'optim': '{optim}'. Must be one of ['alltime', 'finaltime'].")
        b = _as_f64(betas).reshape(-1)
        if b.size != int(P):
            raise ValueError(f"member_costs: {b.size} betas for P = {int(P)} problems")
        members = max(int(P) * int(K), 1)
        J = np.empty(members)
        dist = None if cref is None else np.empty(members)
        check(self.handle, lib.femfct_member_costs(
            self.handle, dptr(u), dptr(uhat), int(bool(uhat_per_problem)), dptr(c), dptr(cref), _host_ptr(b), int(P), int(K),
            int(num_steps), float(dt), int(optim == "finaltime"), _host_ptr(J), None if dist is None else _host_ptr(dist)))
        return J, dist

    # -- controls piecewise constant in time (solvers.ControlIntervals) --------------------
    @staticmethod
    def _starts(starts, num_steps):
        s = np.ascontiguousarray(np.asarray(starts).reshape(-1), dtype=np.int32)
        if s.size < 2:
            raise ValueError("starts: K + 1 >= 2 interval boundaries are needed")
        return s, s.size - 1

    def time_restrict(self, x, starts, num_steps, out, batch=1):
        """out[b][k] = the trapezoid-weighted time mean of x[b] over the levels starts[k] <= l < starts[k+1], for the
        ``batch`` trajectories x ((num_steps+1)*n doubles each); ``out``: batch*K*n doubles.  Does not synchronise."""
        s, K = self._starts(starts, num_steps)
        check(self.handle, lib.femfct_time_restrict(self.handle, dptr(x), _host_ptr(s), K, int(num_steps), int(batch),
                                                    dptr(out)))

    def time_prolong(self, y, starts, num_steps, out, batch=1):
        """out[b][l] = y[b][k(l)]: the K fields of every member held over their intervals (``out`` must not be ``y``)."""
        s, K = self._starts(starts, num_steps)
        check(self.handle, lib.femfct_time_prolong(self.handle, dptr(y), _host_ptr(s), K, int(num_steps), int(batch),
                                                   dptr(out)))

    def time_project(self, x, starts, num_steps, scratch, batch=1):
        """x <- prolong(restrict(x)) in place, the L2(Q)-orthogonal projection onto the trajectories constant on every
        interval; ``scratch``: batch*K*n doubles."""
        self.time_restrict(x, starts, num_steps, scratch, batch)
        self.time_prolong(scratch, starts, num_steps, x, batch)

    # -- controls piecewise constant in space (solvers.ControlZones) -----------------------------
    def set_control_zones(self, labels, m=None):
        """Registers the zone table: ``labels`` (n integers in the pattern's row order; -1: no control at the node,
        0 .. m-1: its zone; ``m`` default max + 1), or None to clear it.  A bad table raises ValueError and the previous
        one stays in place."""
        if labels is None:
            check(self.handle, lib.femfct_set_control_zones(self.handle, None, 0))
            return
        lab = np.asarray(labels).reshape(-1)
        if lab.size != self.n:
            raise ValueError(f"set_control_zones: {lab.size} labels for n = {self.n} nodes")
        if not np.all(lab == np.floor(lab)):
            raise ValueError("set_control_zones: labels must be integers")
        lab = np.ascontiguousarray(lab, dtype=np.int32)
        check(self.handle, lib.femfct_set_control_zones(self.handle, _host_ptr(lab),
                                                        int(lab.max()) + 1 if m is None else int(m)))

    def zone_restrict(self, x, fields, out, apply_mass=False):
        """out[f*m + j] = sum over the nodes i of zone j of x_f[i] (``apply_mass``: of (M x_f)[i]) for the ``fields`` fields
        of n doubles in ``x``; ``out``: fields*m doubles.  Fixed-order sums; does not synchronise."""
        check(self.handle, lib.femfct_zone_restrict(self.handle, dptr(x), int(fields), int(bool(apply_mass)), dptr(out)))

    def zone_prolong(self, s, fields, out, Ginv=None):
        """out[f*n + i] = (Ginv s_f)[label_i], 0.0 where no control acts; ``s``: fields*m doubles, ``Ginv``: m*m doubles on
        the device, row-major (None: the identity, s itself is scattered).  Does not synchronise."""
        check(self.handle, lib.femfct_zone_prolong(self.handle, dptr(s), dptr(Ginv), int(fields), dptr(out)))

    # -- limited-memory quasi-Newton primitives (solvers.LimitedMemory) -----------------------
    @staticmethod
    def _fields(fields):
        J = len(fields)
        if not 1 <= J <= _lib.MAX_GRAM_FIELDS:
            raise ValueError(f"{J} fields: must be in 1..{_lib.MAX_GRAM_FIELDS}")
        return (C.c_void_p * J)(*[dptr(f) for f in fields]), J

    def free_set(self, c, g, c_lower, c_upper, count, mask):
        """mask[k] = 0 where the value is bound ((c <= c_lower and g > 0) or (c >= c_upper and g < 0)), else 1: ``count``
        bytes on the device (any device buffer of at least that size).  One launch, does not synchronise."""
        check(self.handle, lib.femfct_free_set(self.handle, dptr(c), dptr(g), float(c_lower), float(c_upper), int(count),
                                               dptr(mask)))

    def q_gram(self, fields, num_steps, dt, mask=None) -> np.ndarray:
        """The (J, J) Gram matrix of the trajectories ``fields`` in the L2(Q) inner product of ``l2_norm_sq_Q``, each
        masked to the free set ``mask`` (bytes as ``free_set`` writes them; None: all free).  Exactly symmetric, the same
        bits on every call; without a mask the diagonal is ``l2_norm_sq_Q`` bit for bit."""
        ptrs, J = self._fields(fields)
        G = np.empty((J, J))
        check(self.handle, lib.femfct_q_gram(self.handle, ptrs, J, dptr(mask), int(num_steps), float(dt), _host_ptr(G)))
        return G

    def q_combine(self, fields, coef, count, out, mask=None, fallback=None, fallback_scale=0.0):
        """out = ((coef[0]*fields[0] + coef[1]*fields[1]) + ...) where ``mask`` is set (None: everywhere), and
        fallback_scale * fallback elsewhere; bitwise the NumPy expression.  ``out`` must not be an input."""
        ptrs, J = self._fields(fields)
        cf = _as_f64(coef).reshape(-1)
        if cf.size != J:
            raise ValueError(f"q_combine: {cf.size} coefficients for {J} fields")
        check(self.handle, lib.femfct_q_combine(self.handle, ptrs, _host_ptr(cf), J, dptr(mask), dptr(fallback),
                                                float(fallback_scale), int(count), dptr(out)))

    # -- L1-sparse controls (solvers.prox_solidbody, solvers.prox_source_control) ------------------
    def prox_trials(self, c, d, s0, K, alpha, c_lower, c_upper, count, c_out, src_out=None, g=None):
        """c_out[t] = clip(soft_threshold(c + s_t d, s_t alpha)) with s_t = s0 / 2^t, the exact prox of
        s_t alpha |.| + the box indicator value by value, and src_out[t] = g + c_out[t] (c_out[t] without g) for t < K,
        one launch; member t starts at t*count.  alpha = 0 gives ``source_trials``' values."""
        check(self.handle, lib.femfct_prox_trials(self.handle, dptr(c), dptr(d), dptr(g), float(s0), int(K), float(alpha),
                                                  float(c_lower), float(c_upper), int(count), dptr(c_out), dptr(src_out)))

    def budget_trials(self, c, d, s0, K, alpha, budget, c_lower, c_upper, num_steps, dt, c_out, src_out=None, g=None):
        """``prox_trials`` under the control budget ||c_t||_{1,h} <= ``budget``: c_out[t] = clip(soft_threshold(c + s_t d,
        s_t alpha + lam[t])), lam[t] = 0.0 exactly (and ``prox_trials``' bits) where that trial is within the budget, else
        the root of ||c_out[t]||_{1,h} = budget -- value by value the projection onto {box, ||.||_{1,h} <= budget} in the
        nodal-quadrature inner product (weights dt w_l ml_i), the metric of the prox.  ``d`` None (K = 1): the projection of
        ``c`` itself.  The box must contain 0.  Returns ``(lam, l1, rounds)``: the multipliers, ``l1_norm_Q`` of the
        written trials bit for bit, the search rounds used (int32, <= 16).  The same bits on every call; a NaN or Inf in
        ``c`` or ``d`` raises.  Synchronises."""
        k = max(int(K), 1)
        lam, l1, rounds = np.empty(k), np.empty(k), np.empty(k, dtype=np.int32)
        check(self.handle, lib.femfct_budget_trials(self.handle, dptr(c), dptr(d), dptr(g), float(s0), int(K), float(alpha),
                                                    float(budget), float(c_lower), float(c_upper), int(num_steps), float(dt),
                                                    dptr(c_out), dptr(src_out), _host_ptr(lam), _host_ptr(l1),
                                                    _host_ptr(rounds)))
        return lam, l1, rounds

    def l1_norm_Q(self, a, num_steps, dt, batch=1) -> np.ndarray:
        """dt sum_l w_l sum_i ml_i |a_{l,i}| of every batch member: the nodal-quadrature L1(Q) norm (the trapezoid weights
        of ``l2_norm_sq_Q``, the lumped mass).  The same bits on every call."""
        out = np.empty(max(int(batch), 1))
        check(self.handle, lib.femfct_l1_norm_Q(self.handle, dptr(a), int(num_steps), float(dt), _host_ptr(out), int(batch)))
        return out

    def sparse_trial_stats(self, c_trials, c_ref, K, num_steps, dt):
        """``(l1, dist, nnz)`` of the K trial controls ``c_trials`` against the one control ``c_ref``, one fused pass:
        l1[t] = l1_norm_Q(c_t) and dist[t] = l2_norm_sq_Q(c_t - c_ref) bit for bit, nnz[t] = the count of values != 0
        (int64)."""
        k = max(int(K), 1)
        l1, dist, nnz = np.empty(k), np.empty(k), np.empty(k, dtype=np.int64)
        check(self.handle, lib.femfct_sparse_trial_stats(self.handle, dptr(c_trials), dptr(c_ref), int(K), int(num_steps),
                                                         float(dt), _host_ptr(l1), _host_ptr(dist), _host_ptr(nnz)))
        return l1, dist, nnz

    # -- ensemble drift control (solvers.ensemble_solidbody): one control, S weighted scenarios ------------------
    def ensemble_drift_gradient_rhs(self, c, u, p, weights, beta, out, levels, drift=(1.0, 1.0)):
        """out = -(beta M c + sum_s weights[s] * assemble(p_s (b.grad u_s) v dx)) for every level, one launch; ``u``, ``p``:
        S trajectories of ``levels * n`` doubles, ``c``, ``out``: one; the sum in index order over the non-zero weights (a
        scenario of weight 0 is not read).  S = 1 with weight 1 is ``drift_gradient_rhs`` bit for bit."""
        w = _as_f64(weights).reshape(-1)
        check(self.handle, lib.femfct_ensemble_drift_gradient_rhs(
            self.handle, dptr(c), dptr(u), dptr(p), _host_ptr(w), int(w.size), float(beta), float(drift[0]), float(drift[1]),
            dptr(out), int(levels)))

    def ensemble_costs(self, u, uhat, cost_w, c, weights, beta, num_steps, dt, window=None, cref=None):
        """``(T, J, dist)``: T[s] = ``obs_cost`` of scenario s, J = sum_s weights[s] T[s] + (0.5 beta) ``l2_norm_sq_Q(c)``,
        dist = ``l2_norm_sq_Q(c - cref)`` (None without ``cref``), each bit for bit those calls' values, with one
        read-back; ``u``, ``uhat``: S trajectories, ``c``, ``cref``: one each."""
        w = _as_f64(weights).reshape(-1)
        T, J = np.empty(max(w.size, 1)), np.empty(1)
        dist = None if cref is None else np.empty(1)
        check(self.handle, lib.femfct_ensemble_costs(
            self.handle, dptr(u), dptr(uhat), dptr(cost_w), dptr(window), dptr(c), dptr(cref), _host_ptr(w), int(w.size),
            float(beta), int(num_steps), float(dt), _host_ptr(T), _host_ptr(J), None if dist is None else _host_ptr(dist)))
        return T, float(J[0]), (None if dist is None else float(dist[0]))

    # -- initial-state recovery (solvers.initial_state_solidbody): one-level fields of n values ------------------
    def initial_trials(self, v, direction, steps, v_lower, v_upper, u_traj, num_steps):
        """Level 0 of member k of the batch ``u_traj`` (K = len(steps) trajectories of ``(num_steps + 1) * n`` doubles)
        = clip(v + steps[k] * direction, v_lower, v_upper), bitwise the NumPy expression; no other level is touched.  One
        launch, does not synchronise."""
        s = _as_f64(steps).reshape(-1)
        check(self.handle, lib.femfct_initial_trials(self.handle, dptr(v), dptr(direction), _host_ptr(s), int(s.size),
                                                     float(v_lower), float(v_upper), dptr(u_traj), int(num_steps)))

    def initial_trial_stats(self, u_traj, v, K, num_steps, vb=None) -> np.ndarray:
        """``(K, 2)``: ||v_k - vb||^2_M and ||v_k - v||^2_M for v_k = level 0 of member k of ``u_traj`` (``vb`` None: a
        zero background), each ``l2_norm_sq_Omega`` bit for bit, from one pass with one read-back."""
        out = np.empty((max(int(K), 1), 2))
        check(self.handle, lib.femfct_initial_trial_stats(self.handle, dptr(u_traj), dptr(v), dptr(vb), int(K),
                                                          int(num_steps), _host_ptr(out)))
        return out

    def initial_gradient(self, p_traj, v, beta0, g, vb=None, v_lower=0.0, v_upper=0.0, mask=None):
        """g = beta0 * (v - vb) - p_0 (``vb`` None: 0), p_0 = level 0 of ``p_traj``; bitwise the NumPy expression.
        ``mask`` (n bytes on the device): the free set of ``free_set(v, g, v_lower, v_upper)`` from the same launch."""
        check(self.handle, lib.femfct_initial_gradient(self.handle, dptr(p_traj), dptr(v), dptr(vb), float(beta0), dptr(g),
                                                       float(v_lower), float(v_upper), dptr(mask)))

    def omega_gram(self, fields, mask=None) -> np.ndarray:
        """The (J, J) Gram matrix of the one-level ``fields`` in the inner product a^T M b of ``l2_norm_sq_Omega``, each
        masked to the free set ``mask`` (n bytes as ``free_set`` writes them; None: all free).  Exactly symmetric, the
        same bits on every call; without a mask the diagonal is ``l2_norm_sq_Omega`` bit for bit."""
        ptrs, J = self._fields(fields)
        G = np.empty((J, J))
        check(self.handle, lib.femfct_omega_gram(self.handle, ptrs, J, dptr(mask), _host_ptr(G)))
        return G

    # -- smooth controls (solvers.Smoothness): the H1 seminorm in space and time ------------------------------
    def smooth_cost(self, c, num_steps, dt, batch=1) -> np.ndarray:
        """``(batch, 2)``: R_x = dt sum_l w_l c_l^T Ad c_l and R_t = 1/dt sum_l (c_{l+1} - c_l)^T M (c_{l+1} - c_l) per
        batch member, from one pass over ``c`` with one read-back."""
        out = np.empty((max(int(batch), 1), 2))
        check(self.handle, lib.femfct_smooth_cost(self.handle, dptr(c), int(num_steps), float(dt), _host_ptr(out),
                                                  int(batch)))
        return out

    def smooth_rhs(self, c, beta_x, beta_t, num_steps, dt, out, batch=1):
        """out_l = -(beta_x Ad c_l + beta_t M tau_l) for every level and batch member, one launch."""
        check(self.handle, lib.femfct_smooth_rhs(self.handle, dptr(c), float(beta_x), float(beta_t), int(num_steps),
                                                 float(dt), dptr(out), int(batch)))

    def drift_gradient_rhs_smooth(self, c, u, p, beta, beta_x, beta_t, dt, out, levels, drift=(1.0, 1.0)):
        """``drift_gradient_rhs`` + ``smooth_rhs`` in one launch, bit for bit their sum."""
        check(self.handle, lib.femfct_drift_gradient_rhs_smooth(
            self.handle, dptr(c), dptr(u), dptr(p), float(beta), float(beta_x), float(beta_t), float(dt), dptr(out),
            int(levels), float(drift[0]), float(drift[1])))

    # -- non-FCT species / PDE systems ---------------------------------------------------
    def descent_pointwise(self, count, beta, c, x, out, y=None, scale=1.0, divisor=1.0):
        """out = -(beta*c - t), t = x*y/divisor (y given) or scale*x"""
        check(self.handle, lib.femfct_descent_pointwise(self.handle, int(count), float(beta), dptr(c), float(scale), dptr(x),
                                                       dptr(y), float(divisor), dptr(out)))

    def ell_transpose(self, src, out=None) -> DeviceArray:
        if out is None:
            out = self.empty(self.W * self.n)
        check(self.handle, lib.femfct_ell_transpose(self.handle, dptr(src), dptr(out)))
        return out

    def axpby(self, count, alpha, a, beta, b, out):
        check(self.handle, lib.femfct_axpby(self.handle, int(count), float(alpha), dptr(a), float(beta), dptr(b), dptr(out)))

    def set_krylov(self, rel_tol=1e-13, max_iters=2000):
        check(self.handle, lib.femfct_set_krylov(self.handle, float(rel_tol), int(max_iters)))

    def set_species_solver(self, mode="auto"):
        """'auto': tile-fused Chebyshev for the non-FCT solves of the sweeps where it applies; 'bicgstab'."""
        check(self.handle, lib.femfct_set_species_solver(self.handle, {"auto": 0, "bicgstab": 1}[mode]))

    def bicgstab(self, mat_ell, b, x0, x, batch=1, mat_shared=False):
        arr = (StepInfo * batch)()
        check(self.handle, lib.femfct_bicgstab(self.handle, dptr(mat_ell), int(bool(mat_shared)), dptr(b), dptr(x0),
                                               dptr(x), int(batch), arr))
        return [dict(flags=a.flags, solver_iters=a.solver_iters, solver_resid=a.solver_resid) for a in arr]

    def nonlinear_forward(self, Aw, c_level, u, num_steps, dt, eps, batch=1):
        check(self.handle, lib.femfct_nonlinear_forward(self.handle, dptr(Aw), dptr(c_level), dptr(u), int(num_steps),
                                                        float(dt), float(eps), int(batch)))

    def nonlinear_forward_ct(self, Aw, c_traj, u, num_steps, dt, eps, batch=1, c_shared=False):
        """Per-step control: the step to level n+1 reads level n+1 of c_traj ((num_steps+1)*n per member)."""
        check(self.handle, lib.femfct_nonlinear_forward_ct(self.handle, dptr(Aw), dptr(c_traj), int(bool(c_shared)), dptr(u),
                                                           int(num_steps), float(dt), float(eps), int(batch)))

    def nonlinear_adjoint(self, Aw, u, uhat_T, p, num_steps, dt, eps, batch=1, alltime=False, uhat_shared=False, obs=None):
        """alltime=False: final-time misfit, uhat_T n values per member.  alltime=True: all-time misfit
        (nonlinear_FCT_PDECO_alltime.py:198-216), uhat_T a target trajectory per member ((num_steps+1)*n values, or one
        for the whole batch with uhat_shared), p(T) = 0.  ``obs`` (a :class:`DeviceObs`; ``alltime`` is unused with it):
        snapshot observations, uhat_T a trajectory per member read at observed levels only,
        p_Nt = tau_u omega .* (uhat_Nt - u_Nt), load (theta_u[n]/dt) Mw (uhat_n - u_n)."""
        if obs is not None:
            if uhat_shared:
                raise ValueError("uhat_shared: only the all-time sweep takes a shared target")
            check(self.handle, lib.femfct_nonlinear_adjoint_obs(self.handle, dptr(Aw), dptr(u), dptr(uhat_T), dptr(obs.theta_u),
                                                                obs.tau_u, dptr(obs.window), dptr(p), int(num_steps),
                                                                float(dt), float(eps), int(batch)))
            return
        if alltime:
            check(self.handle, lib.femfct_nonlinear_adjoint_alltime(self.handle, dptr(Aw), dptr(u), dptr(uhat_T),
                                                                    int(bool(uhat_shared)), dptr(p), int(num_steps),
                                                                    float(dt), float(eps), int(batch)))
            return
        if uhat_shared:
            raise ValueError("uhat_shared: only the all-time sweep takes a shared target")
        check(self.handle, lib.femfct_nonlinear_adjoint(self.handle, dptr(Aw), dptr(u), dptr(uhat_T), dptr(p),
                                                        int(num_steps), float(dt), float(eps), int(batch)))

    def schnak_forward(self, Aw, c_level, u, v, num_steps, dt, par, rescaling=1.0, batch=1, wind_scale=None):
        """wind_scale: None (stationary wind) or the num_steps+1 factors s(t_k) of a separable wind s(t) w0(x)."""
        par = _as_f64(par)
        ws = None if wind_scale is None else _wind_scale(wind_scale, num_steps)
        check(self.handle, lib.femfct_schnak_forward_tw(self.handle, dptr(Aw), None if ws is None else _host_ptr(ws),
                                                        dptr(c_level), dptr(u), dptr(v), int(num_steps), float(dt),
                                                        _host_ptr(par), float(rescaling), int(batch)))

    def schnak_forward_ct(self, Aw, c_traj, u, v, num_steps, dt, par, rescaling=1.0, batch=1, wind_scale=None,
                          c_shared=False):
        """schnak_forward with a per-step control: the step to level n+1 reads level n+1 of c_traj."""
        par = _as_f64(par)
        ws = None if wind_scale is None else _wind_scale(wind_scale, num_steps)
        check(self.handle, lib.femfct_schnak_forward_ct(self.handle, dptr(Aw), None if ws is None else _host_ptr(ws),
                                                        dptr(c_traj), int(bool(c_shared)), dptr(u), dptr(v), int(num_steps),
                                                        float(dt), _host_ptr(par), float(rescaling), int(batch)))

    def schnak_adjoint(self, AwT, u, v, uhat_T, vhat_T, p, q, num_steps, dt, par, batch=1, alltime=False, wind_scale=None,
                       obs=None):
        """``obs`` (a :class:`DeviceObs`; ``alltime`` is unused with it): snapshot observations of u and v, the targets
        trajectories read at observed levels only (None for a variable that is not observed)."""
        par = _as_f64(par)
        ws = None if wind_scale is None else _wind_scale(wind_scale, num_steps)
        if obs is not None:
            check(self.handle, lib.femfct_schnak_adjoint_obs(
                self.handle, dptr(AwT), None if ws is None else _host_ptr(ws), dptr(u), dptr(v), dptr(uhat_T), dptr(vhat_T),
                dptr(obs.theta_u), obs.tau_u, dptr(obs.theta_v), obs.tau_v, dptr(obs.window), dptr(p), dptr(q),
                int(num_steps), float(dt), _host_ptr(par), int(batch)))
            return
        check(self.handle, lib.femfct_schnak_adjoint_tw(self.handle, dptr(AwT), None if ws is None else _host_ptr(ws),
                                                        dptr(u), dptr(v), dptr(uhat_T), dptr(vhat_T), dptr(p), dptr(q),
                                                        int(num_steps), float(dt), _host_ptr(par), int(bool(alltime)),
                                                        int(batch)))

    def chtxs_forward(self, c_level, u, v, num_steps, dt, par, rescaling=0.1, batch=1, growth=None):
        """``growth=(r0, r1, r2)``: the cell equation gains the source r(u) = u (r0 + r1 u + r2 u^2), explicit in time
        (None: no growth, the reference's solve_chtxs_system)."""
        par = _as_f64(par)
        if growth is not None:
            g = _growth(growth)
            check(self.handle, lib.femfct_chtxs_forward_g(self.handle, dptr(c_level), 0, 0, dptr(u), dptr(v), int(num_steps),
                                                          float(dt), _host_ptr(par), float(rescaling), _host_ptr(g),
                                                          int(batch)))
            return
        check(self.handle, lib.femfct_chtxs_forward(self.handle, dptr(c_level), dptr(u), dptr(v), int(num_steps),
                                                    float(dt), _host_ptr(par), float(rescaling), int(batch)))

    def chtxs_forward_ct(self, c_traj, u, v, num_steps, dt, par, rescaling=0.1, batch=1, c_shared=False, growth=None):
        """chtxs_forward with a per-step control: the step to level n+1 reads level n+1 of c_traj."""
        par = _as_f64(par)
        if growth is not None:
            g = _growth(growth)
            check(self.handle, lib.femfct_chtxs_forward_g(self.handle, dptr(c_traj), 1, int(bool(c_shared)), dptr(u), dptr(v),
                                                          int(num_steps), float(dt), _host_ptr(par), float(rescaling),
                                                          _host_ptr(g), int(batch)))
            return
        check(self.handle, lib.femfct_chtxs_forward_ct(self.handle, dptr(c_traj), int(bool(c_shared)), dptr(u), dptr(v),
                                                       int(num_steps), float(dt), _host_ptr(par), float(rescaling),
                                                       int(batch)))

    def chtxs_adjoint(self, u, v, uhat, vhat, p, q, c, num_steps, dt, par, rescaling=0.1, alltime=True, batch=1,
                      growth=None, obs=None, misfit="mass"):
        """``growth``: as in :meth:`chtxs_forward`; the p step gains the explicit load of r'(u_n) p_{n+1}.
        ``obs`` (a :class:`DeviceObs`; ``alltime`` is unused with it): snapshot observations; ``misfit="mass"`` loads
        (theta[n]/dt) Mw (hat_n - state_n), the discrete adjoint of the tracking cost, ``"nodal"`` the raw nodal misfits
        (theta[n]/dt) omega .* (hat_n - state_n) of the reference's all-time sweep."""
        par = _as_f64(par)
        if obs is not None:
            g = None if growth is None else _growth(growth)
            check(self.handle, lib.femfct_chtxs_adjoint_obs(
                self.handle, dptr(u), dptr(v), dptr(uhat), dptr(vhat), dptr(obs.theta_u), obs.tau_u, dptr(obs.theta_v),
                obs.tau_v, dptr(obs.window), dptr(p), dptr(q), dptr(c), int(num_steps), float(dt), _host_ptr(par),
                float(rescaling), None if g is None else _host_ptr(g), _misfit(misfit), int(batch)))
            return
        if growth is not None:
            g = _growth(growth)
            check(self.handle, lib.femfct_chtxs_adjoint_g(self.handle, dptr(u), dptr(v), dptr(uhat), dptr(vhat), dptr(p),
                                                          dptr(q), dptr(c), int(num_steps), float(dt), _host_ptr(par),
                                                          float(rescaling), int(bool(alltime)), _host_ptr(g), int(batch)))
            return
        check(self.handle, lib.femfct_chtxs_adjoint(self.handle, dptr(u), dptr(v), dptr(uhat), dptr(vhat), dptr(p), dptr(q),
                                                    dptr(c), int(num_steps), float(dt), _host_ptr(par), float(rescaling),
                                                    int(bool(alltime)), int(batch)))

    def traj_krylov_info(self, num_steps, batch=1):
        arr = (StepInfo * (num_steps * batch))()
        check(self.handle, lib.femfct_traj_krylov_info(self.handle, arr, int(num_steps), int(batch)))
        return dict(flags=np.array([a.flags for a in arr]).reshape(num_steps, batch),
                    solver_iters=np.array([a.solver_iters for a in arr]).reshape(num_steps, batch),
                    solver_resid=np.array([a.solver_resid for a in arr]).reshape(num_steps, batch))
