"""CPU: the match-position entry points (include/fsm_hip.h, "match positions") are exported, refuse misuse and fail LOUDLY
without a device; the span rule of the header, composed from the accept-position definition in numpy (tests/span_ref.py), is
what grep -o prints for literal sets; and what FlatDfa.from_strings does today with a word that ends inside another word's
prefix."""
import ctypes as C
import errno

import numpy as np
import pytest

import span_ref
from span_ref import NO_POS

SYMBOLS = ("fsm_hip_pos_dfa_create", "fsm_hip_pos_dfa_free", "fsm_hip_pos_dfa_in_lds", "fsm_hip_exec_accept_pos", "fsm_hip_exec_accept_pos_device",
           "fsm_hip_text_hits_spans", "fsm_hip_text_spans_next", "fsm_hip_text_spans_count", "fsm_hip_text_spans_start_device",
           "fsm_hip_text_spans_end_device", "fsm_hip_text_spans_copy", "fsm_hip_text_spans_ms", "fsm_hip_text_spans_free")


def lib_of():
    from libfsm_amd import load_library
    lib = load_library()
    return lib


def test_every_new_symbol_is_exported(built):
    import libfsm_amd
    lib = lib_of()
    assert [s for s in SYMBOLS if not hasattr(lib, s)] == []
    assert libfsm_amd.NO_POS == NO_POS == 2 ** 64 - 1 and libfsm_amd.POS_BACKWARD == 1
    assert C.sizeof(libfsm_amd.PosBatch) == 11 * 8       # the struct of the header: nine pointers, two sizes, two ints in one word, a u64


def test_no_positions_without_a_device(built):
    """no CPU path: ENODEV from every entry point that would launch, whatever the arguments (with a device, NULL is EINVAL)"""
    import torch
    from libfsm_amd import PosBatch
    want = errno.EINVAL if torch.cuda.is_available() else errno.ENODEV
    lib = lib_of()
    b = PosBatch()
    C.set_errno(0)
    assert lib.fsm_hip_pos_dfa_create(None) is None and C.get_errno() == want
    for fn, args in ((lib.fsm_hip_exec_accept_pos, (None, C.byref(b))), (lib.fsm_hip_exec_accept_pos_device, (None, C.byref(b), None)),
                     (lib.fsm_hip_exec_accept_pos, (None, None)), (lib.fsm_hip_exec_accept_pos_device, (None, None, None))):
        C.set_errno(0)
        assert fn(*args) == -1 and C.get_errno() == want
    C.set_errno(0)
    assert lib.fsm_hip_text_hits_spans(None, None, None, None, None) is None and C.get_errno() == want


def test_python_front_raises_without_a_device(built):
    import torch
    import libfsm_amd
    if not torch.cuda.is_available():
        with pytest.raises(OSError) as ei:
            libfsm_amd.PosDfa.from_flat(span_ref.ends_of([b"ab"])[0])
        assert ei.value.errno == errno.ENODEV


def test_accessors_take_null(built):
    lib = lib_of()
    out = np.zeros(2, np.uint64)
    assert lib.fsm_hip_pos_dfa_in_lds(None) == 0
    assert lib.fsm_hip_text_spans_count(None) == 0
    assert lib.fsm_hip_text_spans_start_device(None) is None and lib.fsm_hip_text_spans_end_device(None) is None
    C.set_errno(0)
    assert lib.fsm_hip_text_spans_copy(None, out.ctypes.data_as(C.c_void_p), None) == -1 and C.get_errno() == errno.EINVAL
    C.set_errno(0)
    assert lib.fsm_hip_text_spans_next(None) == -1 and C.get_errno() == errno.EINVAL
    C.set_errno(0)
    assert lib.fsm_hip_text_spans_ms(None) == -1.0 and C.get_errno() == errno.EINVAL
    lib.fsm_hip_text_spans_free(None)      # as free(NULL)
    lib.fsm_hip_pos_dfa_free(None)


def test_accept_positions_by_eye():
    """the definition on inputs small enough to check by eye: ends = exactly {ab, abc}, starts = anything then ba or cba"""
    ends, starts = span_ref.ends_of([b"ab", b"abc"]), span_ref.starts_of([b"ab", b"abc"])
    rows, lens = span_ref.rows_of([b"abcab", b"xab", b"", b"abx"])
    first, last = span_ref.accept_pos(ends, rows, lens)
    assert first.tolist() == [2, NO_POS, NO_POS, 2] and last.tolist() == [3, NO_POS, NO_POS, 2]
    first, last = span_ref.accept_pos(ends, rows, lens, frm=[3, 1, 0, 4])           # 4 > len 3: not walked
    assert first.tolist() == [5, 3, NO_POS, NO_POS] and last.tolist() == [5, 3, NO_POS, NO_POS]
    first, last = span_ref.accept_pos(starts, rows, lens, back=True)                 # walking order: first is the largest position
    assert first.tolist() == [3, 1, NO_POS, 0] and last.tolist() == [0, 1, NO_POS, 0]
    first, last = span_ref.accept_pos(starts, rows, lens, frm=[1, 0, 0, 0], to=[4, 9, 0, NO_POS], back=True)
    assert first.tolist() == [NO_POS, 1, NO_POS, 0]                                  # "abcab"[1:4] = "bca": no word begins inside it
    first, last = span_ref.accept_pos(span_ref.start_accepting_of(ends), rows, lens)      # k = 0: the start state accepts before any byte
    assert first.tolist() == [0, 0, 0, 0] and last.tolist() == [3, 0, 0, 2]
    sink = span_ref.line_matcher_of([b"ab"])                                         # an absorbing end state: last = len
    first, last = span_ref.accept_pos(sink, rows, lens)
    assert first.tolist() == [2, 3, NO_POS, 2] and last.tolist() == [5, 3, NO_POS, 3]
    first, last = span_ref.accept_pos(sink, rows, lens, back=True)                   # ... backward: the range's low end
    assert first.tolist() == [NO_POS, NO_POS, NO_POS, NO_POS]                        # ("ba" read backward never shows "ab")
    rows, lens = span_ref.rows_of([b"xbay"])
    first, last = span_ref.accept_pos(sink, rows, lens, frm=[1], back=True)
    assert first.tolist() == [1] and last.tolist() == [1]
    first, last = span_ref.accept_pos(sink, rows, lens, back=True)
    assert first.tolist() == [1] and last.tolist() == [0]


def test_span_rule_is_leftmost_longest_for_literal_sets():
    """8 sets of 6 random words of 1-4 bytes over abcd, 700 lines of 0-40 bytes over abcdxyzw each: the rounds of the header's
    rule, composed from the accept-position definition alone, are the brute force's matches on every line"""
    rng = np.random.RandomState(5)
    many = none = most = 0
    for _ in range(8):
        words = list({bytes(rng.choice(list(b"abcd"), rng.randint(1, 5)).astype(np.uint8)) for _ in range(6)})
        lines = [bytes(rng.choice(list(b"abcdxyzw"), rng.randint(0, 41)).astype(np.uint8)) for _ in range(700)]
        rows, lens = span_ref.rows_of(lines)
        rounds = span_ref.spans_rounds(span_ref.starts_of(words), span_ref.ends_of(words), rows, lens)
        want = [span_ref.leftmost_longest(words, x) for x in lines]
        got = [[] for _ in lines]
        for st, en in rounds:
            for i in np.flatnonzero(st != NO_POS):
                got[i].append((int(st[i]), int(en[i])))
        assert got == want
        assert len(rounds) == max(len(w) for w in want) + 1
        many += sum(len(w) > 1 for w in want)
        none += sum(len(w) == 0 for w in want)
        most = max(most, max(len(w) for w in want))
    assert many >= 1000 and none >= 500 and most >= 10      # lines with more than one match, with none, and a long run of rounds


def test_empty_matches_advance_by_one():
    """an `ends` that matches the empty string and a `starts` that accepts everywhere: the span at p is the longest word there or
    (p, p); an empty span moves p one byte on, and p = len still has one"""
    words = [b"ab", b"abc", b"c"]
    starts, ends = span_ref.everywhere_of(span_ref.starts_of(words)), span_ref.ends_of(words, empty=True)
    lines = [b"abcab", b"", b"xx", b"cab"]
    rows, lens = span_ref.rows_of(lines)
    rounds = span_ref.spans_rounds(starts, ends, rows, lens)
    got = [[(int(st[i]), int(en[i])) for st, en in rounds if st[i] != NO_POS] for i in range(len(lines))]
    assert got == [[(0, 3), (3, 5), (5, 5)], [(0, 0)], [(0, 0), (1, 1), (2, 2)], [(0, 1), (1, 3), (3, 3)]]


def test_from_strings_rejects_a_word_that_ends_inside_another_words_prefix(built):
    """A recorded observation, not a demand: the builder that equals the reference's re_strings state for state (tests/test_strings.py)
    does not accept `dbc` for the words a, dbda, cb, c, ad, dbcd under flags 0, 2, 4 and 6, although `dbc` ends in the word c.  The
    Python Aho-Corasick of span_ref, with outputs propagated along failure links, does -- which is why the span tests build their
    automata there.  (NOTES.md, "from_strings and words inside prefixes".)"""
    from libfsm_amd import FlatDfa
    from global_ref import walk
    words = [b"a", b"dbda", b"cb", b"c", b"ad", b"dbcd"]
    line = np.frombuffer(b"dbc", np.uint8)[None, :]
    ident = np.arange(256, dtype=np.int64)
    for flags in (0, 2, 4, 6):
        flat = FlatDfa.from_strings(words, flags)
        dense = flat.dense().astype(np.int64)
        dense[dense == 0xFFFFFFFF] = -1
        end = int(walk(dense, ident, flat.start, line)[0])
        assert end < 0 or not flat.is_end[end], flags
    flat, dense, cls = span_ref.starts_of([w[::-1] for w in words])      # anything, then a word
    end = int(walk(dense, cls, flat.start, line)[0])
    assert end >= 0 and flat.is_end[end]
