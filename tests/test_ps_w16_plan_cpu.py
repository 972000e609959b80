"""The PS planner's plans for the 16-bit-window kernel (csrc/psplan.cpp, kern 3), walked on the host over n, s and the
knobs by tests/host_sanitize/w16_plan_driver.cpp: which calls get the kernel, the LDS word budget with the padding row and
the over-read slack, the register-staging caps, pinned plans and the refusal paths.  A stand-alone program built with
AddressSanitizer and UndefinedBehaviorSanitizer; no GPU."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_w16_plans_on_the_host(tmp_path):
    exe = tmp_path / "w16_plan_driver"
    csrc = os.path.join(REPO, "splicedice_amd", "csrc")
    subprocess.run(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-g", "-std=c++17", "-Wall",
                    "-I", os.path.join(REPO, "include"), "-I", csrc, os.path.join(REPO, "tests", "host_sanitize", "w16_plan_driver.cpp"),
                    os.path.join(csrc, "psplan.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and "w16 plan driver: ok" in run.stdout, run.stdout[-3000:] + run.stderr[-3000:]
