"""vp8oclenc_amd/csrc/intake_settings.h: the intake's settings in one struct -- the one validity rule against the verdicts the GPU suites
assert of the setters, the equality field by field, the canonical form, needs_device_planes and the size helpers.  The header is pure
host code, so all of it is a program of its own (scripts/native/intake_settings_check.cpp), built under the host sanitizers with
vp8_host.cpp and run as a program."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_the_settings_header_is_right_and_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "intake_settings_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "scripts", "native", "intake_settings_check.cpp"), os.path.join(ROOT, "vp8oclenc_amd", "csrc", "vp8_host.cpp"), "-o", exe], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("clean"), r.stdout + r.stderr

