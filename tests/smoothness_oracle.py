"""CPU reference of smooth controls (``solvers.Smoothness``): H1 regularisation of a control trajectory in space and time,
in NumPy on ``oracle.assembly.P1Assembler.mass() / stiffness()``.  For c = (c_0 .. c_Nt), n values per level in FEniCS DoF
order, and the trapezoid's level weights w (1/2 at the end levels):

    R(c) = beta_x/2 R_x + beta_t/2 R_t
    R_x  = dt sum_{l=0..Nt} w_l c_l^T Ad c_l
    R_t  = 1/dt sum_{l<Nt} (c_{l+1} - c_l)^T M (c_{l+1} - c_l)
    M g_l = beta_x Ad c_l + beta_t M tau_l          the gradient in the inner product of l2_norm_sq_Q
    tau_l = (2 c_l - c_{l-1} - c_{l+1}) / dt^2  (0 < l < Nt),   tau_0 = 2 (c_0 - c_1) / dt^2,   tau_Nt = 2 (c_Nt - c_{Nt-1}) / dt^2

``smooth_rhs`` is -(M g_l), the vector the per-level mass solve is applied to.  The loops are the unchanged oracle's
(``oracle.traj.solidbody_pgd_loop``, the resolve loop of ``state_bounds_oracle.pgd_source_loop``) with R added to every
cost and ``smooth_rhs`` to every level's right-hand side before ``chebsi``."""
import numpy as np

from oracle import traj as otraj
from oracle.fct import chebsi, cost_functional, l2_norm_sq_Q


def _levels(c, Nt):
    return np.asarray(c, dtype=np.float64).reshape(Nt + 1, -1)


def roughness(M, Ad, c, Nt, dt):
    """``(R_x, R_t)``"""
    cl = _levels(c, Nt)
    w = np.ones(Nt + 1)
    w[0] = w[-1] = 0.5
    Rx = dt * sum(w[l] * (cl[l] @ (Ad @ cl[l])) for l in range(Nt + 1))
    Rt = sum((cl[l + 1] - cl[l]) @ (M @ (cl[l + 1] - cl[l])) for l in range(Nt)) / dt
    return Rx, Rt


def value(M, Ad, c, Nt, dt, beta_x, beta_t):
    Rx, Rt = roughness(M, Ad, c, Nt, dt)
    return beta_x / 2 * Rx + beta_t / 2 * Rt


def _neighbours(l, Nt):
    """the two levels tau_l reads besides l; at an end level the one neighbour twice"""
    return (l - 1 if l > 0 else 1), (l + 1 if l < Nt else Nt - 1)


def tau(c, Nt, dt):
    cl = _levels(c, Nt)
    out = np.empty_like(cl)
    for l in range(Nt + 1):
        lo, hi = _neighbours(l, Nt)
        out[l] = (2 * cl[l] - cl[lo] - cl[hi]) / dt ** 2
    return out.ravel()


def smooth_rhs(M, Ad, c, Nt, dt, beta_x, beta_t):
    """-(beta_x Ad c_l + beta_t M tau_l), every level"""
    cl, tl = _levels(c, Nt), _levels(tau(c, Nt, dt), Nt)
    return np.concatenate([-(beta_x * (Ad @ cl[l]) + beta_t * (M @ tl[l])) for l in range(Nt + 1)])


def rhs_magnitude(M, Ad, c, Nt, dt, beta_x, beta_t):
    """per row the sum of the magnitudes of smooth_rhs's terms,
    beta_x |Ad| |c_l| + beta_t |M| (2 |c_l| + |c_{l-1}| + |c_{l+1}|) / dt^2"""
    cl = np.abs(_levels(c, Nt))
    aM, aA = abs(M), abs(Ad)
    out = []
    for l in range(Nt + 1):
        lo, hi = _neighbours(l, Nt)
        out.append(beta_x * (aA @ cl[l]) + beta_t * (aM @ (2 * cl[l] + cl[lo] + cl[hi])) / dt ** 2)
    return np.concatenate(out)


def cost_magnitude(M, Ad, c, Nt, dt):
    """``(S_x, S_t, m_x, m_t)``: the sums of the magnitudes of the products R_x and R_t add up, and their numbers"""
    cl = np.abs(_levels(c, Nt))
    d = np.abs(np.diff(_levels(c, Nt), axis=0))
    aM, aA = abs(M), abs(Ad)
    w = np.ones(Nt + 1)
    w[0] = w[-1] = 0.5
    Sx = dt * sum(w[l] * (cl[l] @ (aA @ cl[l])) for l in range(Nt + 1))
    St = sum(d[l] @ (aM @ d[l]) for l in range(Nt)) / dt
    return Sx, St, (Nt + 1) * Ad.nnz, Nt * M.nnz


def pgd_loop(sb, u0, uhat, c0, beta, beta_x, beta_t, c_lower, c_upper, iters, nodes, num_steps, dt, gam=1e-4, s0=1.0,
             max_armijo=10, optim="finaltime"):
    """``oracle.traj.solidbody_pgd_loop`` for J + R; the history gains ``roughness_x`` / ``roughness_t`` of the accepted
    iterate."""
    n, Nt = nodes, num_steps
    tl = (Nt + 1) * n
    M, Ad = sb.cm.M, sb.cm.Ad
    Md = M.diagonal()
    uhat = np.asarray(uhat, dtype=np.float64)
    J_of = lambda u, c: cost_functional(u, uhat, c, Nt, dt, M, beta, optim) + value(M, Ad, c, Nt, dt, beta_x, beta_t)
    uk = np.zeros(tl)
    uk[:n] = u0
    if optim == "alltime":
        uk[n:] = uhat[n:]
    else:
        uk[Nt * n:] = uhat
    c_prev = np.array(c0, dtype=np.float64)
    pk = np.zeros(tl)
    hist = dict(cost=[], armijo_k=[], armijo_margin=[], roughness_x=[], roughness_t=[])
    for _ in range(iters):
        pk = otraj.solidbody_adjoint(sb, c_prev, uk, uhat, np.zeros(tl), n, Nt, dt, optim=optim)
        sm = smooth_rhs(M, Ad, c_prev, Nt, dt, beta_x, beta_t)
        dk = np.zeros(tl)
        for l in range(Nt + 1):
            rhs = otraj.solidbody_descent_rhs(sb, c_prev, uk, pk, beta, n, l) + sm[l * n:(l + 1) * n]
            dk[l * n:(l + 1) * n] = chebsi(rhs, M, Md, 20, 0.5, 2)
        ck = np.clip(c_prev + s0 * dk, c_lower, c_upper)
        otraj.solidbody_forward(sb, ck, uk, n, Nt, dt)
        J_k = J_of(uk, ck)
        margins = []
        for k in range(max_armijo):
            s = s0 * (1 / 2 ** k)
            c_inc = np.clip(ck + s * dk, c_lower, c_upper)
            otraj.solidbody_forward(sb, c_inc, uk, n, Nt, dt)
            J = J_of(uk, c_inc)
            stat = l2_norm_sq_Q(c_inc - ck, Nt, dt, M)
            margins.append((J - J_k + gam / s * stat) / abs(J_k))
            if not (J - J_k > -gam / s * stat):
                break
        Rx, Rt = roughness(M, Ad, c_inc, Nt, dt)
        for key, v in (("cost", J), ("armijo_k", k + 1), ("armijo_margin", margins), ("roughness_x", Rx),
                       ("roughness_t", Rt)):
            hist[key].append(v)
        c_prev = c_inc
    hist["armijo_margin_min"] = min(abs(m) for ms in hist["armijo_margin"] for m in ms)
    return uk, pk, c_prev, hist


def pgd_source_loop(ls, u0, uhat, c0, beta, beta_x, beta_t, c_lower, c_upper, nodes, num_steps, dt, max_iters, gam=1e-4,
                    s0=1.0, max_armijo=10):
    """The resolve loop of ``state_bounds_oracle.pgd_source_loop`` for all-time tracking and J + R in place of J + P:
    d = -(beta c - p) + chebsi(smooth_rhs) level by level, ``max_iters`` iterations (no stop test)."""
    n, Nt = nodes, num_steps
    tl = (Nt + 1) * n
    M, Ad = ls.cm.M, ls.cm.Ad
    Md = M.diagonal()
    uhat = np.asarray(uhat, dtype=np.float64)
    J_of = lambda u, c: cost_functional(u, uhat, c, Nt, dt, M, beta, "alltime") + value(M, Ad, c, Nt, dt, beta_x, beta_t)
    u = np.zeros(tl)
    u[:n] = u0
    c = np.array(c0, dtype=np.float64)
    J_ref = 10 * J_of(u, c)
    hist = dict(cost=[], cost_state=[], armijo_k=[], armijo_margin=[], roughness_x=[], roughness_t=[])
    p = np.zeros(tl)
    for _ in range(max_iters):
        otraj.linear_forward(ls, c, u, n, Nt, dt)
        hist["cost_state"].append(J_of(u, c))
        p = otraj.linear_adjoint(ls, u, uhat, np.zeros(tl), n, Nt, dt)
        sm = smooth_rhs(M, Ad, c, Nt, dt, beta_x, beta_t)
        d = -(beta * c - p) + np.concatenate([chebsi(sm[l * n:(l + 1) * n], M, Md, 20, 0.5, 2) for l in range(Nt + 1)])
        margins = []
        for k in range(max_armijo):
            s = s0 * (1 / 2 ** k)
            cj = np.clip(c + s * d, c_lower, c_upper)
            uj = np.zeros(tl)
            uj[:n] = u0
            otraj.linear_forward(ls, cj, uj, n, Nt, dt)
            Jj = J_of(uj, cj)
            dist = l2_norm_sq_Q(cj - c, Nt, dt, M)
            margins.append((Jj - J_ref + gam / s * dist) / abs(J_ref))
            if Jj - J_ref <= -gam / s * dist:
                break
        Rx, Rt = roughness(M, Ad, cj, Nt, dt)
        for key, v in (("cost", Jj), ("armijo_k", k + 1), ("armijo_margin", margins), ("roughness_x", Rx),
                       ("roughness_t", Rt)):
            hist[key].append(v)
        J_ref, c = Jj, cj
    hist["armijo_margin_min"] = min(abs(m) for ms in hist["armijo_margin"] for m in ms)
    return u, p, c, hist
