"""The sweep controller (csrc/sweep_ctl.hip, femfct_run_sweep in csrc/traj_common.h) on the CPU: tools/asan/sweep_ctl_driver.cpp
calls femfct_run_sweep on top of the fake HIP runtime with `step` lambdas that launch nothing and write scripted step logs
("this step needs X sweeps / Y iterations", ROW_PAIRS, NaN / Inf residuals), and prints what every attempt received (budgets,
solver, pair_rows, Chebyshev or not, graphs dropped) between the library's own FEMFCT_DEBUG lines.  The trace must equal
tests/golden/sweep_ctl_trace.txt line for line; that file was recorded from the commit BEFORE the controller was split into
plan / run / verdict (its first line names the commit and the command), so the test pins that commit's budgets, hand-overs,
error texts and reset semantics -- the stale one-workgroup cap after femfct_set_solver included.

Scenarios: budgets growing, accepted and shrinking in the tile32, strip, row and patch64 regimes; one launch fewer tried and
failed / succeeded; max_iters between easy and hard (BiCGStab hand-over and recovery); NaN and Inf residuals; ROW_PAIRS and
kinds that start on full rows; the one-workgroup cap; Chebyshev budget growth, Chebyshev off, BiCGStab doubling and its cap,
femfct_set_species_solver; interleaved kinds; what survives each of the three setters; the single-patch margin.

Not scripted here (covered by the GPU suite only): FEMFCT_DEBUG_TIMES reporting (wall-clock figures), errors returned by
`begin` / `step` or by the HIP runtime in the middle of an attempt, and the kernels' side of the logs (the counts are the
driver's model of what the device reports)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="hipcc not available")
def test_sweep_controller_trace_equals_the_recorded_one():
    d = os.path.join(ROOT, "tools", "asan")
    b = subprocess.run(["make", "-C", d, "-j8", "_build/sweep_ctl_driver"], capture_output=True, text=True, timeout=900)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    r = subprocess.run([os.path.join(d, "_build", "sweep_ctl_driver")], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1"))
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert "AddressSanitizer" not in out and "LeakSanitizer" not in out and "bad launch geometry" not in out, out[-3000:]
    with open(os.path.join(ROOT, "tests", "golden", "sweep_ctl_trace.txt")) as f:
        want = [line.rstrip("\n") for line in f if not line.startswith("#")]
    got = r.stdout.splitlines()
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"trace line {k + 1}: got {g!r}, recorded {w!r}"
    assert len(got) == len(want)
    assert got[-1] == "sweep_ctl_driver: 0 unexpected results"
