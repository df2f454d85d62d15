"""CPU: the template lookup of one line (libfsm_amd/csrc/replace_seg.h: the repl_at() that takes a rule's inserts, repl_xlen,
repl_inserts_of) as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer: tests/c/test_replace_tmpl.cpp."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_replace_tmpl(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([gxx, *san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("no sanitizer runtimes for g++")
    exe = str(tmp_path / "test_replace_tmpl")
    cc = subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-g", "-O1", *san, os.path.join(ROOT, "tests", "c", "test_replace_tmpl.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    assert "warning" not in cc.stderr, cc.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "test_replace_tmpl: ok" in run.stdout
