"""libfsm_amd/csrc/front.h (the skeleton the host fronts of the tokens, the matches, the replaced and the extracted text and the
distinct records share: run_new / run_free / run_host / run_ms, copy_out, grid_of) as a stand-alone program:
tests/c/test_front.cpp defines stand-ins for the HIP entry points the header calls that record the order of the calls, so it
links without libamdhip64 and runs without a GPU, under AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "test_front.cpp")
ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_front_header(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    if not os.path.exists(os.path.join(ROCM_INCLUDE, "hip", "hip_runtime_api.h")):
        pytest.skip("no HIP headers")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([gxx, *SAN, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("no sanitizer runtimes for g++")
    exe = str(tmp_path / "test_front")
    cc = subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-g", "-O1", *SAN, "-D__HIP_PLATFORM_AMD__", "-I" + ROCM_INCLUDE, SRC, "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "test_front: ok" in run.stdout
