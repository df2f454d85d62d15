"""libfsm_amd/csrc/image.cpp (a Plan's device image, the end-id, resume and trace tables) as a stand-alone program:
tests/c/test_image.cpp plans automata of its own under every layout and checks each member of the image against the Plan.  It
links plan.cpp and image.cpp and nothing of HIP, and runs without a GPU under AddressSanitizer and
UndefinedBehaviorSanitizer."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libfsm_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "c", "test_image.cpp"), os.path.join(CSRC, "plan.cpp"), os.path.join(CSRC, "image.cpp")]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_image_builder(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([gxx, *SAN, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("no sanitizer runtimes for g++")
    exe = str(tmp_path / "test_image")
    cc = subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-g", "-O1", *SAN, *SOURCES, "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "test_image: ok" in run.stdout
