"""CPU: the matches (include/fsm_hip.h, "matches").  The judge of tests/matches_ref.py against an independent brute force on
Aho-Corasick pairs, against the rounds of span_ref.spans_rounds on pairs that do not belong together, and its ids against
tokens_ref.state_ids; the marks layout (libfsm_amd/csrc/match_marks.h) as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer; and the entry points: exported, in the binding's table, failing LOUDLY without a device."""
import ctypes as C
import errno
import os
import shutil
import subprocess

import numpy as np
import pytest

import matches_ref
import span_ref
import tokens_ref
from global_ref import affine
from matches_ref import DROP_EMPTY
from span_ref import NO_POS, rows_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libfsm_amd", "csrc")
WORDS = [b"ab", b"abc", b"ca", b"d", b"bdb"]

SYMBOLS = ("fsm_hip_matches_run", "fsm_hip_matches_run_device", "fsm_hip_text_matches", "fsm_hip_matches_count", "fsm_hip_matches_total",
           "fsm_hip_matches_off_device", "fsm_hip_matches_start_device", "fsm_hip_matches_end_device", "fsm_hip_matches_id_device",
           "fsm_hip_matches_copy", "fsm_hip_matches_ms", "fsm_hip_matches_pass_ms", "fsm_hip_matches_free")


def word_lines(n=2000, seed=21):
    """n lines over abcdxy, 0-40 bytes"""
    rng = np.random.RandomState(seed)
    return [bytes(np.frombuffer(b"abcdxy", np.uint8)[rng.randint(0, 6, rng.randint(0, 41))]) for _ in range(n)]


def per_line(res):
    off = res["off"].astype(np.int64)
    return [list(zip(res["start"][off[i]:off[i + 1]].tolist(), res["end"][off[i]:off[i + 1]].tolist())) for i in range(len(off) - 1)]


def test_judge_is_leftmost_longest_on_aho_corasick_pairs():
    lines = word_lines()
    assert len(lines) >= 2000
    rows, lens = rows_of(lines)
    res = matches_ref.matches(span_ref.starts_of(WORDS), span_ref.ends_of(WORDS), rows, lens)
    want = [span_ref.leftmost_longest(WORDS, x) for x in lines]
    assert per_line(res) == want
    assert sum(len(w) >= 4 for w in want) >= 500 and sum(len(w) == 0 for w in want) >= 50
    assert (res["end"] > res["start"]).all()
    # DROP_EMPTY changes nothing where no match is empty
    again = matches_ref.matches(span_ref.starts_of(WORDS), span_ref.ends_of(WORDS), rows, lens, DROP_EMPTY)
    assert all(np.array_equal(res[k], again[k]) for k in ("off", "start", "end", "state"))


def brute_with_empty(line, drop):
    """every position is a start, the longest word there or the empty string: [(start, end)]"""
    out, p = [], 0
    while p <= len(line):
        e = p + max([len(w) for w in WORDS if line[p:p + len(w)] == w], default=0)
        if not (drop and e == p):
            out.append((p, e))
        p = e if e > p else e + 1
    return out


def test_judge_on_empty_matches_with_and_without_drop_empty():
    lines = [b""] + word_lines(600, 22)
    rows, lens = rows_of(lines)
    starts, ends = span_ref.everywhere_of(span_ref.starts_of(WORDS)), span_ref.ends_of(WORDS, empty=True)
    kept = matches_ref.matches(starts, ends, rows, lens)
    dropped = matches_ref.matches(starts, ends, rows, lens, DROP_EMPTY)
    assert per_line(kept) == [brute_with_empty(x, False) for x in lines]
    assert per_line(dropped) == [brute_with_empty(x, True) for x in lines]
    empty = kept["end"] == kept["start"]
    assert empty.sum() >= 1000 and (~empty).sum() >= 1000 and int((~empty).sum()) == len(dropped["start"])
    assert lines[0] == b"" and per_line(kept)[0] == [(0, 0)] and per_line(dropped)[0] == []
    # ... and the matches that are left are those of the words alone, where a word begins
    assert per_line(dropped) == [span_ref.leftmost_longest(WORDS, x) for x in lines]


def flat_rounds(rounds, n):
    """spans_rounds flattened per input up to the first NO_POS"""
    out = [[] for _ in range(n)]
    alive = np.ones(n, bool)
    for st, en in rounds:
        alive &= st != NO_POS
        for i in np.flatnonzero(alive):
            out[i].append((int(st[i]), int(en[i])))
    return out


@pytest.mark.parametrize("pair", ["s15_s200", "dying_start"])
def test_judge_is_the_rounds_flattened_on_pairs_that_do_not_belong_together(pair):
    rng = np.random.RandomState(23)
    n = 300
    rows = rng.randint(0, 256, (n, 60)).astype(np.uint8)
    lens = rng.randint(0, 61, n).astype(np.int64)
    lens[:6] = [0, 1, 15, 16, 17, 60]
    if pair == "s15_s200":
        starts, ends = affine(15, 4), affine(200, 4, holes=16, sinks=3)
    else:
        starts, ends = affine(200, 4, holes=16, sinks=3), span_ref.start_accepting_of(affine(15, 4))
    want = flat_rounds(span_ref.spans_rounds(starts, ends, rows, lens), n)
    res = matches_ref.matches(starts, ends, rows, lens)
    assert per_line(res) == want
    cnt = np.diff(res["off"].astype(np.int64))
    assert (cnt >= 2).sum() >= 20 and (cnt == 0).sum() >= 10      # of 300 lines: the inputs are not trivial
    if pair == "dying_start":
        assert (res["end"] == res["start"]).sum() >= 30          # empty matches and the end + 1 step
        kept = per_line(res)
        dropped = per_line(matches_ref.matches(starts, ends, rows, lens, DROP_EMPTY))
        assert dropped == [[x for x in ms if x[1] > x[0]] for ms in kept]


def test_ids_are_those_of_the_state_at_end():
    words = [w.encode() for w in "a ab abcda b bc bcdab c ca cab d dd ddabc".split()]
    lines = word_lines(500, 24)
    rows, lens = rows_of(lines)
    ends, sets = tokens_ref.trie_lexer(words)
    starts = span_ref.starts_of(words)
    for mode in (tokens_ref.EARLIEST, tokens_ref.RET):
        ids = tokens_ref.state_ids(ends, mode, sets)
        res = matches_ref.matches(starts, ends, rows, lens, ids=ids)
        assert len(res["id"]) >= 2000 and np.array_equal(res["id"], ids[res["state"]].astype(np.uint32))
        if mode == tokens_ref.EARLIEST:     # the id is the index of the word that lies there
            off = res["off"].astype(np.int64)
            for i in range(0, len(lines), 7):
                for k in range(off[i], off[i + 1]):
                    assert words[int(res["id"][k])] == lines[i][int(res["start"][k]):int(res["end"][k])]
    # one state with two ids: EARLIEST the lower, RET the index of its set
    two = {s: ([3, 9] if v == [0] else [v[0] + 10]) for s, v in sets.items()}
    e_ids, r_ids = tokens_ref.state_ids(ends, tokens_ref.EARLIEST, two), tokens_ref.state_ids(ends, tokens_ref.RET, two)
    s_a = [s for s, v in sets.items() if v == [0]][0]
    assert e_ids[s_a] == 3 and r_ids[s_a] == len(words) - 1
    # select: a pick beyond the lines has no match, a repeated one has its matches again
    res = matches_ref.matches(starts, ends, rows, lens, ids=e_ids)
    off = res["off"].astype(np.int64)
    o, st, en, idv = matches_ref.select(res, [5, 10 ** 9, 5], len(lines))
    c5 = int(off[6] - off[5])
    assert o.tolist() == [0, c5, c5, 2 * c5] and st.tolist() == 2 * res["start"][off[5]:off[6]].tolist() and len(en) == len(idv) == 2 * c5


def test_marks_layout(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([gxx, *san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("no sanitizer runtimes for g++")
    exe = str(tmp_path / "test_match_marks")
    cc = subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-g", "-O1", *san, os.path.join(ROOT, "tests", "c", "test_match_marks.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "test_match_marks: ok" in run.stdout


def test_every_new_symbol_is_exported_and_in_the_table(built):
    import libfsm_amd
    from libfsm_amd import capi
    lib = libfsm_amd.load_library()
    assert [s for s in SYMBOLS if not hasattr(lib, s)] == []
    assert [s for s in SYMBOLS if s not in capi.PROTOTYPES] == []
    header = open(os.path.join(ROOT, "include", "fsm_hip.h")).read()
    assert [s for s in SYMBOLS if s + "(" not in header] == []
    assert libfsm_amd.MATCHES_DROP_EMPTY == DROP_EMPTY == 1
    mb = libfsm_amd.MatchBatch
    assert C.sizeof(mb) == 7 * 8 and [f for f, _ in mb._fields_] == ["base", "off", "n", "pick", "m", "trim_byte", "flags", "limit"]
    assert (mb.trim_byte.offset, mb.flags.offset, mb.limit.offset) == (40, 44, 48)


def test_struct_mirror_is_the_header(tmp_path):
    """struct fsm_hip_match_batch as the compiler reads it against the binding's mirror"""
    import libfsm_amd
    mb = libfsm_amd.MatchBatch
    names = [f for f, _ in mb._fields_]
    src = tmp_path / "mb.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fsm_hip.h"\nint main(void)\n{\n\tprintf("%zu", sizeof(struct fsm_hip_match_batch));\n'
                   + "".join('\tprintf(" %%zu", offsetof(struct fsm_hip_match_batch, %s));\n' % f for f in names) + "\treturn 0;\n}\n")
    exe = str(tmp_path / "mb")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    assert got == [C.sizeof(mb)] + [getattr(mb, f).offset for f in names]


def test_no_matches_without_a_device(built):
    """no CPU path: ENODEV from every entry point that would launch, whatever the arguments (with a device, NULL is EINVAL)"""
    import torch
    import libfsm_amd
    want = errno.EINVAL if torch.cuda.is_available() else errno.ENODEV
    lib = libfsm_amd.load_library()
    b = libfsm_amd.MatchBatch()
    for fn, args in ((lib.fsm_hip_matches_run, (None, None, C.byref(b))), (lib.fsm_hip_matches_run, (None, None, None)),
                     (lib.fsm_hip_matches_run_device, (None, None, C.byref(b), None)), (lib.fsm_hip_text_matches, (None, None, None, None, 0, None))):
        C.set_errno(0)
        assert fn(*args) is None and C.get_errno() == want


def test_accessors_take_null(built):
    import libfsm_amd
    lib = libfsm_amd.load_library()
    out = np.zeros(2, np.uint64)
    assert lib.fsm_hip_matches_count(None) == 0 and lib.fsm_hip_matches_total(None) == 0
    for fn in (lib.fsm_hip_matches_off_device, lib.fsm_hip_matches_start_device, lib.fsm_hip_matches_end_device, lib.fsm_hip_matches_id_device):
        assert fn(None) is None
    C.set_errno(0)
    assert lib.fsm_hip_matches_copy(None, out.ctypes.data_as(C.c_void_p), None, None, None) == -1 and C.get_errno() == errno.EINVAL
    C.set_errno(0)
    assert lib.fsm_hip_matches_ms(None) == -1.0 and C.get_errno() == errno.EINVAL
    C.set_errno(0)
    assert lib.fsm_hip_matches_pass_ms(None, 0) == -1.0 and C.get_errno() == errno.EINVAL
    lib.fsm_hip_matches_free(None)      # as free(NULL)
