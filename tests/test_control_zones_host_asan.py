"""The HOST code of femfct_set_control_zones / femfct_zone_restrict / femfct_zone_prolong under AddressSanitizer, no GPU
needed: tools/asan/zones_asan_driver.cpp, a stand-alone program on tools/asan/fake_hip.cpp (kernels are not executed),
built by tools/asan/Makefile like the other drivers and run directly -- the argument checks, m = 1 and m = 256, a table
replaced by a larger and then a smaller one, restrict and prolong with fields = 1 and 3 x 251, and calls with no table
registered."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="hipcc not available")
def test_control_zones_host_code_is_clean_under_address_sanitizer():
    d = os.path.join(ROOT, "tools", "asan")
    b = subprocess.run(["make", "-C", d, "-j8", "_build/zones_asan_driver"], capture_output=True, text=True, timeout=900)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    r = subprocess.run([os.path.join(d, "_build", "zones_asan_driver")], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1"))
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert "zones_asan_driver: 0 unexpected return codes" in out
    assert "AddressSanitizer" not in out and "LeakSanitizer" not in out and "bad launch geometry" not in out, out[-3000:]
