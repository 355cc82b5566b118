"""tests/jacobi_count.py against the oracle, and the sweep counts of every input of tests/test_gpu_sweep_controller.py
(no GPU): an input that is retuned out of the window its case needs fails here, not silently on the device."""
import numpy as np
import pytest

import jacobi_count as jc
from helpers_golden import load, fct_case


def test_converged_iterate_is_the_oracles_low_order_solution():
    """Golden step rot_N41: the Jacobi iterate that meets the device's criterion equals the oracle's spsolve u_low to
    1e-12, the count is that of a contracting iteration, and the row-sum diagnostic is the golden file's."""
    from oracle.fct import Pattern, fct_step
    c = fct_case(load("fct_cases.npz"), "rot_N41")
    info = {}
    fct_step(c["A"], c["rhs"], c["u_n"], c["dt"], c["n"], c["M"], c["ML"], None, info=info)
    L = Pattern(c["M"]).csr(info["l_vals"])
    b = c["ml"] * c["u_n"] + c["dt"] * c["rhs"]
    k, x = jc.sweeps(L, b)
    assert 0 < k < jc.MAX_ITERS, k
    assert np.abs(b - L @ x).max() <= jc.REL_TOL * np.abs(b).max()
    assert np.abs(x - info["u_low"]).max() <= 1e-12 * max(1.0, np.abs(info["u_low"]).max())
    assert bool(np.asarray(L.sum(axis=1)).min() > 0) == (not c["mmatrix_failed"])
    # one sweep fewer does not meet the criterion: the count is the first that does
    k1, x1 = jc.sweeps(L, b, max_sweeps=k - 1)
    assert k1 == k and np.abs(b - L @ x1).max() > jc.REL_TOL * np.abs(b).max()


def test_count_step_goes_through_the_oracles_own_step():
    """count_step on a solid-body step: L and b are the oracle step's (u_low solves them), the iterate meets u_low."""
    mesh, asm, sb = jc.solid_body(21)
    u = jc.state(mesh, 3)
    k, ok, x, info = jc.count_step(sb.cm, -sb.A_u(3.0 * jc.control_shape(mesh)), np.zeros(mesh.nodes), u, 4e-3)
    assert 0 < k < jc.MAX_ITERS
    assert np.abs(x - info["u_low"]).max() <= 1e-12
    assert ok == bool(info["l_rowsum"].min() > 0)


@pytest.mark.parametrize("key", list(jc.WINDOWS), ids=lambda k: f"{k[0]}-amp{k[1]:g}")
def test_inputs_of_the_controller_tests_lie_in_their_windows(key):
    N, dt, amp, (lo, hi) = jc.WINDOWS[key]
    r = jc.solid_body_counts(N, dt, amp)
    print(f"[jacobi count] {key}: N={N} dt={dt:g} amp={amp:g} forward {r['forward']} adjoint {r['adjoint']}")
    for kind in ("forward", "adjoint"):
        assert lo < r[kind][0] < hi, (key, kind, r[kind][0], lo, hi)


def test_row_sum_diagnostic_of_the_mixed_flag_batches():
    """The batches with MMATRIX_ROWSUM on some members only: amplitude 0 passes the diagnostic, amplitudes 3 and 10 fail it,
    forward and adjoint; at the hard time steps every amplitude fails it."""
    for win in ("N81-easy", "N41-easy"):
        for amp in (0.0, 3.0, 10.0):
            r = jc.solid_body_counts(*jc.WINDOWS[(win, amp)][:3])
            assert r["forward"][1] == r["adjoint"][1] == (amp == 0.0), (win, amp, r)
    for win in ("N81", "N41"):
        for amp in (0.0, 3.0, 10.0, 30.0):
            r = jc.solid_body_counts(*jc.WINDOWS[(win, amp)][:3])
            assert not r["forward"][1] and not r["adjoint"][1], (win, amp, r)


def test_cap_of_the_cap_case_separates_easy_from_hard():
    """Case E: the midpoint of the easy and the hard count lies strictly between them, with room on both sides."""
    for win, easy, hard in (("N81", 0.0, 30.0), ("N41-mesh", 0.0, 50.0)):
        ce = jc.solid_body_counts(*jc.WINDOWS[(win, easy)][:3])["forward"][0]
        ch = jc.solid_body_counts(*jc.WINDOWS[(win, hard)][:3])["forward"][0]
        cap = (ce + ch) // 2
        assert ce + 10 < cap < ch - 10, (win, ce, cap, ch)
