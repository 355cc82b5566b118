"""The HOST code of femfct_budget_trials under AddressSanitizer, no GPU needed: tools/asan/budget_asan_driver.cpp, a
stand-alone program on tools/asan/fake_hip.cpp (kernels are not executed), built by tools/asan/Makefile like the other
drivers and run directly -- K = 1 and 16, g / src_out / d present and NULL, every rejected argument, a NULL context,
repeated calls whose scratch grows and then fits, and the search's verdict on a round's read-back driven with arbitrary
values (NaN, infinities, random bits): it ends within the round cap with a threshold inside the bracket."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="hipcc not available")
def test_budget_host_code_is_clean_under_address_sanitizer():
    d = os.path.join(ROOT, "tools", "asan")
    b = subprocess.run(["make", "-C", d, "-j8", "_build/budget_asan_driver"], capture_output=True, text=True, timeout=900)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    r = subprocess.run([os.path.join(d, "_build", "budget_asan_driver")], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1"))
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert "budget_asan_driver: 0 unexpected results" in out
    assert "AddressSanitizer" not in out and "LeakSanitizer" not in out and "bad launch geometry" not in out, out[-3000:]
