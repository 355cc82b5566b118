"""The CPU reference of the per-step control mode (tests/per_step_oracle.py) against the oracle itself: with a control
that is constant in time the chained one-step calls ARE the Nt-step call (bitwise, also with a time-dependent
Schnakenberg wind, which checks the time shift), and with the time-varying control of the GPU tests
(tests/test_gpu_control_per_step.py) the per-step trajectory is far from the frozen one -- so those tests discriminate."""
import numpy as np
import pytest

import per_step_oracle as po

NC, NT, DT = 40, 50, 5e-4
CASES = [("nonlinear", None), ("schnak", None), ("schnak", "sin"), ("chtxs", None)]


@pytest.fixture(scope="module")
def asm():
    from oracle.assembly import P1Assembler
    from oracle.mesh import SquareMesh
    return P1Assembler(SquareMesh(0.0, 1.0, NC))


def _run(solver_mod, problem, wind, control, asm, num_steps=NT):
    mesh, n = asm.mesh, asm.mesh.nodes
    ic = po.initial_conditions(problem, mesh)
    z = [np.concatenate([x, np.zeros(num_steps * n)]) for x in ic]
    if problem == "nonlinear":
        solver_mod.solve_nonlinear_equation(control, z[0], None, asm, n, num_steps, DT)
    elif problem == "schnak":
        solver_mod.solve_schnak_system(control, z[0], z[1], asm, n, num_steps, DT,
                                       wind_scale=po.sin_wind if wind else None)
    else:
        solver_mod.solve_chtxs_system(control, z[0], z[1], asm, n, num_steps, DT)
    return z


@pytest.mark.parametrize("problem,wind", CASES)
def test_chained_oracle_is_the_oracle_for_a_constant_control(asm, problem, wind):
    from oracle import traj
    c = po.constant_control(po.SCALE[problem] * po.bump(asm.mesh), NT)
    chained = _run(po, problem, wind, c, asm)
    single = _run(traj, problem, wind, c, asm)
    for a, b in zip(chained, single):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("problem,wind", CASES)
def test_time_varying_control_separates_the_modes(asm, problem, wind):
    from oracle import traj
    c = po.varying_control(po.SCALE[problem] * po.bump(asm.mesh), NT)
    per_step = _run(po, problem, wind, c, asm)
    frozen = _run(traj, problem, wind, c, asm)
    gaps = [np.max(np.abs(a - b)) / np.max(np.abs(b)) for a, b in zip(per_step, frozen)]
    assert max(gaps) > 1e-3, gaps


def test_chained_step_reads_level_k_plus_1(asm):
    """one step of the chain reads control level 1 and nothing else (level 0 never), two steps level 2 next"""
    from oracle import traj
    n = asm.mesh.nodes
    cbar = po.bump(asm.mesh)
    c = po.varying_control(cbar, 2)
    poisoned = c.copy()
    poisoned[:n] = np.nan                   # level 0
    a = _run(po, "nonlinear", None, poisoned, asm, num_steps=2)[0]
    assert np.all(np.isfinite(a))
    one = _run(traj, "nonlinear", None, c, asm, num_steps=1)[0]
    assert np.array_equal(a[:2 * n], one)
    # level 2 enters only the second step
    c2 = c.copy()
    c2[2 * n:] *= 3.0
    b = _run(po, "nonlinear", None, c2, asm, num_steps=2)[0]
    assert np.array_equal(b[:2 * n], a[:2 * n]) and not np.array_equal(b[2 * n:], a[2 * n:])
