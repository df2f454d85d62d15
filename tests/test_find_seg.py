"""libfsm_amd/csrc/find_seg.h (the arithmetic of the lookup: the walk of a probe's chain over a finished table without a claim, the
bitmap's word and bit, the pick positions of the present and the absent records) as a stand-alone program with its own main,
tests/c/test_find_seg.cpp: the table built by sequential insertion in three record orders, under the plain and the weak hash, the
lookup of present and absent probes -- absent behind a full run of equal-tag slots, absent across the table's wrap -- against
std::map, under AddressSanitizer and UndefinedBehaviorSanitizer.  The header needs no device compiler and the program links nothing
of HIP."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "test_find_seg.cpp")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_find_seg_header(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([gxx, *SAN, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("no sanitizer runtimes for g++")
    exe = str(tmp_path / "test_find_seg")
    cc = subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-g", "-O1", *SAN, SRC, "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    assert "warning" not in cc.stderr, cc.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "test_find_seg: ok" in run.stdout
