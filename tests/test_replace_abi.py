"""CPU: the replacement (include/fsm_hip.h, "replace").  The judge of tests/replace_ref.py against Python's re.sub on
Aho-Corasick pairs, with empty matches kept, with an empty table and with a trimmed delimiter; the lookup of one line
(libfsm_amd/csrc/replace_seg.h) as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer; and the entry
points: exported, in the binding's table, failing LOUDLY without a device."""
import ctypes as C
import errno
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import matches_ref
import replace_ref
import span_ref
import tokens_ref
from replace_ref import MASK
from span_ref import rows_of
from test_matches_abi import WORDS, word_lines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ("fsm_hip_repl_create", "fsm_hip_repl_free", "fsm_hip_repl_in_lds", "fsm_hip_repl_lds_bytes", "fsm_hip_repl_lds_rules",
           "fsm_hip_matches_replace", "fsm_hip_matches_replace_device", "fsm_hip_text_replace", "fsm_hip_replaced_count",
           "fsm_hip_replaced_nbytes", "fsm_hip_replaced_off_device", "fsm_hip_replaced_bytes_device", "fsm_hip_replaced_copy",
           "fsm_hip_replaced_ms", "fsm_hip_replaced_pass_ms", "fsm_hip_replaced_block_lines", "fsm_hip_replaced_block_bytes",
           "fsm_hip_replaced_free")
# the alternation ordered longest-first: leftmost-longest for literals
PATTERN = re.compile(b"|".join(re.escape(w) for w in sorted(WORDS, key=len, reverse=True)))


def keyword_matches(lines):
    """(rows, lens, (off, start, end, id)) of the keywords' pair, the id of a match the index of its word"""
    rows, lens = rows_of(lines)
    ends, sets = tokens_ref.trie_lexer(WORDS)
    ids = tokens_ref.state_ids(ends, tokens_ref.EARLIEST, sets)
    res = matches_ref.matches(span_ref.starts_of(WORDS), ends, rows, lens, ids=ids)
    return rows, lens, (res["off"], res["start"], res["end"], res["id"])


def sub(table, flags, line):
    def one(mo):
        own = mo.group()
        k = WORDS.index(own)
        if k >= len(table) or (flags & MASK and not table[k]):
            return own
        return (table[k] * len(own))[:len(own)] if flags & MASK else table[k]
    return PATTERN.sub(one, line)


@pytest.mark.parametrize("table,flags", [
    ([b"<AB>", b"", b"c", b"a much longer replacement than any word", b"bdb"], 0),     # grows, vanishes, shrinks, the same
    ([b"-", b"", b"xyz"], 0),                                                         # rules 3 and 4 beyond nrepl: left alone
    ([b"*", b"#@!", b"", b"xy"], MASK),                                               # |R| 1 and 3, |R| = 0 stays, rule 4 beyond
])
def test_judge_is_re_sub_on_the_keywords(table, flags):
    lines = word_lines()
    rows, lens, mt = keyword_matches(lines)
    assert len(mt[1]) >= 5000 and set(mt[3].tolist()) == set(range(len(WORDS)))
    off, data = replace_ref.replace(rows, lens, lens, mt, table, flags)
    got = replace_ref.lines_of(off, data)
    want = [sub(table, flags, x) for x in lines]
    assert got == want
    assert sum(g != x for g, x in zip(got, lines)) >= 1000
    if flags & MASK:
        assert [len(g) for g in got] == [len(x) for x in lines]                      # lengths never change under MASK
    else:
        shrink, grow = sum(len(g) < len(x) for g, x in zip(got, lines)), sum(len(g) > len(x) for g, x in zip(got, lines))
        assert grow + shrink >= 500 and grow >= 20 and shrink >= 20


def test_judge_inserts_at_empty_matches():
    """x* with every position a start: the replacement goes into every gap and over every run of x.  This is re.sub's answer;
    the cursor rule of the matches emits the empty match right behind a run, as re.sub does (GNU sed leaves that one out)."""
    lines = [b"", b"x", b"abxd", b"xxaxx", b"abc"] + [bytes(np.frombuffer(b"axb", np.uint8)[np.random.RandomState(31).randint(0, 3, k)]) for k in range(40)]
    rows, lens = rows_of(lines)
    dense = np.full((1, 256), -1, np.int64)
    dense[0, ord("x")] = 0
    ends = span_ref._auto(dense, [True])
    starts = span_ref.everywhere_of(span_ref.starts_of([b"x"]))
    res = matches_ref.matches(starts, ends, rows, lens, ids=np.zeros(1, np.int64))
    mt = (res["off"], res["start"], res["end"], res["id"])
    assert (res["end"] == res["start"]).sum() >= 100 and (res["end"] > res["start"]).sum() >= 50
    off, data = replace_ref.replace(rows, lens, lens, mt, [b"-"])
    got = replace_ref.lines_of(off, data)
    assert got == [re.sub(b"x*", b"-", x) for x in lines]
    assert got[:3] == [b"-", b"--", b"-a-b--d-"]
    # ... and the keywords' `ends` that accepts the empty string as well: an insert wherever no word begins
    lines = word_lines(300, 32)
    rows, lens = rows_of(lines)
    res = matches_ref.matches(span_ref.everywhere_of(span_ref.starts_of(WORDS)), span_ref.ends_of(WORDS, empty=True), rows, lens,
                              ids=np.zeros(64, np.int64))
    mt = (res["off"], res["start"], res["end"], res["id"])
    off, data = replace_ref.replace(rows, lens, lens, mt, [b"|"])
    pat = re.compile(b"|".join(re.escape(w) for w in sorted(WORDS, key=len, reverse=True)) + b"|")
    # (re.sub would try the empty alternative behind a word too; the definition's cursor does as well: the same)
    assert replace_ref.lines_of(off, data) == [pat.sub(b"|", x) for x in lines]


def test_judge_identity_with_an_empty_table_and_the_trimmed_delimiter():
    lines = word_lines(400, 33)
    rows, lens, mt = keyword_matches(lines)
    off, data = replace_ref.replace(rows, lens, lens, mt, [])
    assert replace_ref.lines_of(off, data) == lines and np.array_equal(off[1:], np.cumsum(lens).astype(np.uint64))
    # every line with its newline, trimmed for the matches and copied by the replacement; the last line has none
    with_nl = [x + b"\n" for x in lines[:-1]] + [lines[-1]]
    rows2, raws = rows_of(with_nl)
    assert np.array_equal(raws - lens, np.r_[np.ones(len(lines) - 1, np.int64), 0])
    table = [b"", b"", b"", b"", b""]                      # every word deleted: lines of words alone keep their newline only
    off, data = replace_ref.replace(rows2, lens, raws, mt, table)
    got = replace_ref.lines_of(off, data)
    assert got == [sub(table, 0, x) + (b"\n" if i + 1 < len(lines) else b"") for i, x in enumerate(lines)]
    assert sum(g == b"\n" for g in got) >= 3 and bytes(data).count(b"\n") == len(lines) - 1
    # an empty match at len stands before the delimiter
    assert replace_ref.line(b"ab\n", 2, [(2, 2, 0)], [b"!"]) == b"ab!\n"
    with pytest.raises(AssertionError):
        replace_ref.line(b"ab\n", 2, [(1, 3, 0)], [b"!"])   # a match over the delimiter is no match of the trimmed line


def test_replace_seg(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([gxx, *san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("no sanitizer runtimes for g++")
    exe = str(tmp_path / "test_replace_seg")
    cc = subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-g", "-O1", *san, os.path.join(ROOT, "tests", "c", "test_replace_seg.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "test_replace_seg: ok" in run.stdout


def test_every_new_symbol_is_exported_and_in_the_table(built):
    import libfsm_amd
    from libfsm_amd import capi
    lib = libfsm_amd.load_library()
    assert [s for s in SYMBOLS if not hasattr(lib, s)] == []
    assert [s for s in SYMBOLS if s not in capi.PROTOTYPES] == []
    header = open(os.path.join(ROOT, "include", "fsm_hip.h")).read()
    assert [s for s in SYMBOLS if s + "(" not in header] == []
    assert libfsm_amd.REPL_MASK == MASK == 1
    for name in ("HipRepl", "HipReplaced"):
        assert hasattr(libfsm_amd, name)
    for name in ("replace", "replace_device", "text_replace"):
        assert callable(getattr(libfsm_amd.HipMatches, name))
    # the constants need no device
    assert libfsm_amd.replaced_block_lines() == 256 and libfsm_amd.replaced_block_bytes() == 16384
    assert libfsm_amd.repl_lds_bytes() == 16384 and libfsm_amd.repl_lds_rules() == 1023


def test_no_replacement_without_a_device(built):
    """no CPU path: ENODEV from every entry point that would launch or upload, whatever the arguments (with a device, these
    arguments are EINVAL)"""
    import torch
    import libfsm_amd
    want = errno.EINVAL if torch.cuda.is_available() else errno.ENODEV
    lib = libfsm_amd.load_library()
    b = libfsm_amd.MatchBatch()
    roff = np.zeros(2, np.uint64)
    for fn, args in ((lib.fsm_hip_repl_create, (None, roff.ctypes.data_as(C.c_void_p), 1, 2)), (lib.fsm_hip_repl_create, (None, None, 1, 0)),
                     (lib.fsm_hip_matches_replace, (None, C.byref(b), None)), (lib.fsm_hip_matches_replace, (None, None, None)),
                     (lib.fsm_hip_matches_replace_device, (None, C.byref(b), None, None)), (lib.fsm_hip_text_replace, (None, None, None, None, None))):
        C.set_errno(0)
        assert fn(*args) is None and C.get_errno() == want
    if not torch.cuda.is_available():
        with pytest.raises(OSError) as ei:
            libfsm_amd.HipRepl([b"x"])
        assert ei.value.errno == errno.ENODEV


def test_accessors_take_null(built):
    import libfsm_amd
    lib = libfsm_amd.load_library()
    out = np.zeros(2, np.uint64)
    assert lib.fsm_hip_replaced_count(None) == 0 and lib.fsm_hip_replaced_nbytes(None) == 0 and lib.fsm_hip_repl_in_lds(None) == 0
    for fn in (lib.fsm_hip_replaced_off_device, lib.fsm_hip_replaced_bytes_device):
        assert fn(None) is None
    C.set_errno(0)
    assert lib.fsm_hip_replaced_copy(None, out.ctypes.data_as(C.c_void_p), None) == -1 and C.get_errno() == errno.EINVAL
    C.set_errno(0)
    assert lib.fsm_hip_replaced_ms(None) == -1.0 and C.get_errno() == errno.EINVAL
    C.set_errno(0)
    assert lib.fsm_hip_replaced_pass_ms(None, 0) == -1.0 and C.get_errno() == errno.EINVAL
    lib.fsm_hip_replaced_free(None)     # as free(NULL)
    lib.fsm_hip_repl_free(None)
