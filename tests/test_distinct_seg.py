"""libfsm_amd/csrc/distinct_seg.h (the arithmetic of the distinct records: the trimmed length, the hash over 16-byte chunks with a
masked tail whose sum does not depend on how the chunks are split, the table size, the slot word, the probe sequence with its wrap,
the chunk comparison, the weak hash of the test flag) as a stand-alone program with its own main, tests/c/test_distinct_seg.cpp: the
insert simulated sequentially in several record orders against std::map, under AddressSanitizer and UndefinedBehaviorSanitizer.  The
header needs no device compiler and the program links nothing of HIP."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "test_distinct_seg.cpp")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_distinct_seg_header(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([gxx, *SAN, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("no sanitizer runtimes for g++")
    exe = str(tmp_path / "test_distinct_seg")
    cc = subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-g", "-O1", *SAN, SRC, "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    assert "warning" not in cc.stderr, cc.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "test_distinct_seg: ok" in run.stdout
