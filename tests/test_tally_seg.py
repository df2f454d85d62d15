"""libfsm_amd/csrc/tally_seg.h (the arithmetic of the tally: the column of an id, the clamp of an offset to the total, the group of
an input with its empty groups and its two "counted nowhere" edges, the 64-ary search a wavefront makes, the rule "first of its
column in its input" over windows with a carried bitmap) as a stand-alone program with its own main, tests/c/test_tally_seg.cpp,
against a brute-force count, under AddressSanitizer and UndefinedBehaviorSanitizer.  The header needs no device compiler and the program links nothing of HIP."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "test_tally_seg.cpp")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_tally_seg_header(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([gxx, *SAN, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("no sanitizer runtimes for g++")
    exe = str(tmp_path / "test_tally_seg")
    cc = subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-g", "-O1", *SAN, SRC, "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    assert "warning" not in cc.stderr, cc.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "test_tally_seg: ok" in run.stdout
