"""CPU: the tokeniser (include/fsm_hip.h, "tokens").  The judge of tests/tokens_ref.py against an independent brute force on a
word lexer; the image builder (libfsm_amd/csrc/image.cpp build_tok_image) as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer; and the entry points: exported, refusing misuse, failing LOUDLY without a device."""
import ctypes as C
import errno
import os
import shutil
import subprocess

import numpy as np
import pytest

import tokens_ref
from span_ref import rows_of
from tokens_ref import NO_BACKTRACK, NO_MATCH, NO_POS, SKIP_BAD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libfsm_amd", "csrc")
WORDS = [w.encode() for w in "a ab abcda b bc bcdab c ca cab d dd ddabc".split()]

SYMBOLS = ("fsm_hip_tok_dfa_create", "fsm_hip_tok_dfa_free", "fsm_hip_tok_dfa_in_lds", "fsm_hip_tokens_run", "fsm_hip_tokens_run_device",
           "fsm_hip_text_tokens", "fsm_hip_tokens_count", "fsm_hip_tokens_total", "fsm_hip_tokens_off_device", "fsm_hip_tokens_end_device",
           "fsm_hip_tokens_id_device", "fsm_hip_tokens_err_device", "fsm_hip_tokens_copy", "fsm_hip_tokens_ms", "fsm_hip_tokens_pass_ms",
           "fsm_hip_tokens_free")


def word_lines():
    """2 000 lines over abcdx, 0-40 bytes, x rare: the recipe of the issue, draw by draw"""
    rng = np.random.RandomState(7)
    lines = []
    for _ in range(2000):
        length = rng.randint(0, 41)
        lines.append(bytes(np.frombuffer(b"abcdx", np.uint8)[rng.choice(5, length, p=[.24, .24, .24, .24, .04])]))
    return lines


def brute(line, flags):
    """the tokens of one line from the words alone: [(end, word index or -1)], err, [overrun of every real token]"""
    p, toks, err, over = 0, [], NO_POS, []
    while p < len(line):
        rest = line[p:]
        fit = [w for w in WORDS if rest.startswith(w)]
        # how far a walk of the trie gets: the longest prefix of the rest that begins some word; the next byte dies, if there is one
        reach = max(max(k for k in range(min(len(w), len(rest)) + 1) if w[:k] == rest[:k]) for w in WORDS)
        looked = reach + (1 if reach < len(rest) else 0)
        if flags & NO_BACKTRACK:
            fit = [w for w in fit if len(w) == reach]
        if fit:
            w = max(fit, key=len)
            toks.append((p + len(w), WORDS.index(w)))
            over.append(looked - len(w))
            p += len(w)
            continue
        if err == NO_POS:
            err = p
        if not flags & SKIP_BAD:
            break
        toks.append((p + 1, -1))
        p += 1
    return toks, err, over


def test_judge_is_the_brute_force_on_the_word_lexer():
    lines = word_lines()
    rows, lens = rows_of(lines)
    auto, sets = tokens_ref.trie_lexer(WORDS)
    ids = tokens_ref.state_ids(auto, tokens_ref.EARLIEST, sets)
    judge = tokens_ref.Judge(auto, rows, lens)
    n = len(lines)
    per = {}
    for flags in (0, NO_BACKTRACK, SKIP_BAD, NO_BACKTRACK | SKIP_BAD):
        res = judge.run(flags, ids)
        off = res["off"].astype(np.int64)
        want = [brute(x, flags) for x in lines]
        for i, (toks, err, over) in enumerate(want):
            got = list(zip(res["end"][off[i]:off[i + 1]].tolist(), res["id"][off[i]:off[i + 1]].tolist()))
            assert got == [(e, NO_MATCH if w < 0 else w) for e, w in toks], (flags, i, lines[i])
            assert int(res["err"][i]) == err, (flags, i)
            # the tokens tile [0, err), or the whole line
            ends = [e for e, _ in toks]
            assert ends == sorted(set(ends)) and (not ends or ends[-1] == (len(lines[i]) if flags & SKIP_BAD or err == NO_POS else err))
        assert res["overrun"].tolist() == [o for _, _, over in want for o in over], flags
        per[flags] = (want, res)
    share = lambda xs: sum(bool(x) for x in xs) / n      # noqa: E731
    stop, stop_nb = per[0][0], per[NO_BACKTRACK][0]
    assert share(len(t) >= 4 for t, _, _ in stop) >= 0.6
    assert share(any(o >= 2 for o in over) for _, _, over in stop) >= 0.05
    assert share(a[:2] != b[:2] for a, b in zip(stop, stop_nb)) >= 0.2
    assert 0.4 <= share(err != NO_POS for _, err, _ in stop) <= 0.6
    nonempty = [k for k, x in enumerate(lines) if x]
    assert sum(stop[k][1] == NO_POS for k in nonempty) / len(nonempty) >= 0.4
    assert {w for t, _, _ in stop for _, w in t} == set(range(12))
    skip, skip_nb = per[SKIP_BAD][0], per[NO_BACKTRACK | SKIP_BAD][0]
    assert share(len(t) >= 4 for t, _, _ in skip) >= 0.8
    assert share(a[:2] != b[:2] for a, b in zip(skip, skip_nb)) >= 0.3
    assert max(len(t) for t, _, _ in skip) >= 30


def test_judge_by_eye():
    auto, sets = tokens_ref.trie_lexer([b"ab", b"abc", b"c"])
    ids = tokens_ref.state_ids(auto, tokens_ref.EARLIEST, sets)
    rows, lens = rows_of([b"abcab", b"abx", b"", b"xab", b"abcc"])
    j = tokens_ref.Judge(auto, rows, lens)
    r = j.run(0, ids)
    assert r["off"].tolist() == [0, 2, 3, 3, 3, 5] and r["end"].tolist() == [3, 5, 2, 3, 4] and r["id"].tolist() == [1, 0, 0, 1, 2]
    assert r["err"].tolist() == [NO_POS, 2, NO_POS, 0, NO_POS]
    r = j.run(SKIP_BAD, ids)
    assert r["off"].tolist() == [0, 2, 4, 4, 6, 8] and r["end"].tolist() == [3, 5, 2, 3, 1, 3, 3, 4]
    assert r["id"].tolist() == [1, 0, 0, NO_MATCH, NO_MATCH, 0, 1, 2] and r["err"].tolist() == [NO_POS, 2, NO_POS, 0, NO_POS]
    r = j.run(NO_BACKTRACK, ids)          # "abx": the walk stops behind ab, an end state; "abca": behind abc
    assert r["off"].tolist() == [0, 2, 3, 3, 3, 5] and r["end"].tolist() == [3, 5, 2, 3, 4]
    auto2, sets2 = tokens_ref.trie_lexer([b"a", b"abc"])
    j2 = tokens_ref.Judge(auto2, *rows_of([b"abx", b"aba"]))
    ids2 = tokens_ref.state_ids(auto2, tokens_ref.EARLIEST, sets2)
    assert j2.run(0, ids2)["end"].tolist() == [1, 1] and j2.run(0, ids2)["err"].tolist() == [1, 1]
    assert j2.run(NO_BACKTRACK, ids2)["end"].tolist() == [] and j2.run(NO_BACKTRACK, ids2)["err"].tolist() == [0, 0]
    # RET: the index of the id set among the distinct sets, by count, then bytes
    assert tokens_ref.state_ids(auto, tokens_ref.RET, {2: [7], 3: [1, 2], 4: [256]}).tolist() == [NO_MATCH, NO_MATCH, 1, 2, 0]


def test_image_builder(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([gxx, *san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("no sanitizer runtimes for g++")
    exe = str(tmp_path / "test_tok_image")
    sources = [os.path.join(ROOT, "tests", "c", "test_tok_image.cpp"), os.path.join(CSRC, "plan.cpp"), os.path.join(CSRC, "image.cpp")]
    cc = subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-g", "-O1", *san, *sources, "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "test_tok_image: ok" in run.stdout


def test_every_new_symbol_is_exported(built):
    import libfsm_amd
    lib = libfsm_amd.load_library()
    assert [s for s in SYMBOLS if not hasattr(lib, s)] == []
    assert (libfsm_amd.TOKENS_NO_BACKTRACK, libfsm_amd.TOKENS_SKIP_BAD) == (NO_BACKTRACK, SKIP_BAD) == (1, 2)
    assert (libfsm_amd.IDS_EARLIEST, libfsm_amd.IDS_RET, libfsm_amd.IDS_ERROR) == (1, 2, 3)
    # the struct of the header: three pointers, two sizes, two ints in one word, a u64
    tb = libfsm_amd.TokBatch
    assert C.sizeof(tb) == 7 * 8 and [f for f, _ in tb._fields_] == ["base", "off", "n", "pick", "m", "trim_byte", "flags", "limit"]
    assert (tb.trim_byte.offset, tb.flags.offset, tb.limit.offset) == (40, 44, 48)


def test_struct_mirror_is_the_header(tmp_path):
    """struct fsm_hip_tok_batch as the compiler reads it against the binding's mirror"""
    import libfsm_amd
    tb = libfsm_amd.TokBatch
    names = [f for f, _ in tb._fields_]
    src = tmp_path / "tb.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fsm_hip.h"\nint main(void)\n{\n\tprintf("%zu", sizeof(struct fsm_hip_tok_batch));\n'
                   + "".join('\tprintf(" %%zu", offsetof(struct fsm_hip_tok_batch, %s));\n' % f for f in names) + "\treturn 0;\n}\n")
    exe = str(tmp_path / "tb")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    assert got == [C.sizeof(tb)] + [getattr(tb, f).offset for f in names]


def test_no_tokens_without_a_device(built):
    """no CPU path: ENODEV from every entry point that would launch, whatever the arguments (with a device, NULL is EINVAL)"""
    import torch
    import libfsm_amd
    want = errno.EINVAL if torch.cuda.is_available() else errno.ENODEV
    lib = libfsm_amd.load_library()
    b = libfsm_amd.TokBatch()
    for fn, args in ((lib.fsm_hip_tok_dfa_create, (None, 1)), (lib.fsm_hip_tokens_run, (None, C.byref(b))), (lib.fsm_hip_tokens_run, (None, None)),
                     (lib.fsm_hip_tokens_run_device, (None, C.byref(b), None)), (lib.fsm_hip_text_tokens, (None, None, None, 0, None))):
        C.set_errno(0)
        assert fn(*args) is None and C.get_errno() == want
    if not torch.cuda.is_available():
        with pytest.raises(OSError) as ei:
            libfsm_amd.TokDfa.from_flat(tokens_ref.trie_lexer(WORDS)[0][0])
        assert ei.value.errno == errno.ENODEV


def test_accessors_take_null(built):
    import libfsm_amd
    lib = libfsm_amd.load_library()
    out = np.zeros(2, np.uint64)
    assert lib.fsm_hip_tok_dfa_in_lds(None) == 0
    assert lib.fsm_hip_tokens_count(None) == 0 and lib.fsm_hip_tokens_total(None) == 0
    for fn in (lib.fsm_hip_tokens_off_device, lib.fsm_hip_tokens_end_device, lib.fsm_hip_tokens_id_device, lib.fsm_hip_tokens_err_device):
        assert fn(None) is None
    C.set_errno(0)
    assert lib.fsm_hip_tokens_copy(None, out.ctypes.data_as(C.c_void_p), None, None, None) == -1 and C.get_errno() == errno.EINVAL
    C.set_errno(0)
    assert lib.fsm_hip_tokens_ms(None) == -1.0 and C.get_errno() == errno.EINVAL
    C.set_errno(0)
    assert lib.fsm_hip_tokens_pass_ms(None, 0) == -1.0 and C.get_errno() == errno.EINVAL
    lib.fsm_hip_tokens_free(None)      # as free(NULL)
    lib.fsm_hip_tok_dfa_free(None)
