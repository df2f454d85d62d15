"""The inputs, the automata and the matches' judge that the GPU tests of the line fronts share (spans, tokens, matches, replace,
extract, templates): built once a process, returned read-only, never changed.

The inputs are 1 500 rows of at most 300 bytes with lengths 0, 1, 15, 16, 17, 31, 32, 33, ... -- random bytes (make_inputs) or
lines made of the KEYWORDS (keyword_inputs: line 8 = 300 times d) -- packed behind LEAD bytes that belong to no line.  The
automata are global_ref.affine's, span_ref's variants of them and its Python Aho-Corasick; the judge is tests/matches_ref.py.
tests/test_line_inputs.py holds the inputs to digests of what the test files built for themselves before this module."""
import functools

import numpy as np

import matches_ref
import span_ref
import tokens_ref
from global_ref import affine, packed
from tokens_ref import EARLIEST

FILL = 0xA5A5A5A5A5A5A5A5
LEAD = 5                                     # off[0]: the text does not begin at base
SIZES = (1, 63, 64, 65, 255, 256, 257, 1500)
KEYWORDS = [b"ab", b"abc", b"ca", b"d", b"bdb"]
EMPTY_RULE = len(KEYWORDS)                   # the id of the empty string in kw_ends_empty_ids
# name -> (S, K, keyword arguments, the start state is an end state too, walked from LDS)
AUTOMATA = {
    "s15_start": (15, 4, {}, True, True),
    "s200_dying": (200, 4, dict(holes=16, sinks=3), False, True),
    "lds_full": (1023, 16, {}, False, True),                        # 1024 * 16 = 16 384 entries: the largest LDS image
    "glob_first": (1024, 16, {}, False, False),                     # 1025 * 16 = 16 400 entries: the first global image
    "dying1023": (1023, 16, dict(holes=8, sinks=4), False, True),
}


def device_u64(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64).copy()).cuda()


def device_u8(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint8).copy()).cuda()


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def make_inputs():
    """1 500 rows of 300 random bytes; lengths 0, 1, 15, 16, 17, 31, 32, 33, then odd rows 0-12 and even rows 0-300"""
    rng = np.random.RandomState(11)
    rows = rng.randint(0, 256, (1500, 300)).astype(np.uint8)
    lens = np.where(np.arange(1500) % 2 == 1, rng.randint(0, 13, 1500), rng.randint(0, 301, 1500)).astype(np.int64)
    lens[:8] = [0, 1, 15, 16, 17, 31, 32, 33]
    return _frozen(rows, lens)


@functools.lru_cache(maxsize=None)
def keyword_inputs():
    """the same 1 500 lengths, the lines built from the keywords and a filler letter now and then; line 8: 300 times d"""
    rng = np.random.RandomState(19)
    pieces = KEYWORDS + [b"x", b"a", b"b"]
    rows = np.zeros((1500, 300), np.uint8)
    for i in range(1500):
        line = b"".join(pieces[k] for k in rng.randint(0, len(pieces), 300))[:300]
        rows[i] = np.frombuffer(line, np.uint8)
    lens = make_inputs()[1].copy()
    lens[8] = 300
    rows[8] = ord("d")
    return _frozen(rows, lens)


def lead_packed(rows, lens, lead=LEAD):
    """the lines packed behind `lead` bytes that belong to no line: (bytes of exactly off[n], off with off[0] = lead)"""
    data, off = packed(rows, lens)
    return np.concatenate([np.full(lead, 0x5A, np.uint8), data]), off + np.uint64(lead)


def inputs_of(name):
    """the 1 500 inputs an automaton is judged on: the keyword lines for kw_*, the random rows for every other"""
    return keyword_inputs() if name.startswith("kw") else make_inputs()


def _with_sets(auto, sets, is_end=None):
    """a copy of a trie_lexer automaton whose states carry `sets` (and, with is_end, are end states by it)"""
    from libfsm_amd import FlatDfa
    is_end = np.asarray(auto[0].is_end, np.uint8) if is_end is None else is_end
    return (FlatDfa.from_dense(auto[1], 0, is_end, endids=sets), auto[1], auto[2]), sets, None


def _make_auto(name):
    if name in AUTOMATA:
        S, K, kw, start_ends, in_lds = AUTOMATA[name]
        auto = affine(S, K, endids=True, **kw)
        if start_ends:     # (with_is_end drops the ids: such an `ends` gives FSM_HIP_NO_ID everywhere)
            auto = span_ref.start_accepting_of(auto)
        from libfsm_amd import Plan
        plan = Plan(auto[0])
        assert (plan.S1, plan.C) == (S + 1, K) and (plan.S1 * plan.C <= 16384) == in_lds
        return auto, None, in_lds
    if name == "kw_starts":
        return span_ref.starts_of(KEYWORDS), None, None
    if name == "kw_starts_everywhere":
        return span_ref.everywhere_of(span_ref.starts_of(KEYWORDS)), None, None
    if name == "kw_ends":
        return tokens_ref.trie_lexer(KEYWORDS) + (None,)
    if name == "kw_ends_two":               # a union where the state of "ab" carries two ids
        auto, sets = tokens_ref.trie_lexer(KEYWORDS)
        return _with_sets(auto, {s: ([3, 9] if v == [0] else [v[0] + 10]) for s, v in sets.items()})
    if name == "kw_ends_empty":
        return span_ref.ends_of(KEYWORDS, empty=True), None, None
    if name == "kw_ends_empty_ids":         # the keywords and, as rule EMPTY_RULE, the empty string
        auto, sets = tokens_ref.trie_lexer(KEYWORDS)
        is_end = np.asarray(auto[0].is_end, np.uint8).copy()
        is_end[0] = 1
        return _with_sets(auto, {**sets, 0: [EMPTY_RULE]}, is_end)
    if name == "sink_one":                  # one accepting state, every byte leads back to it: an absorbing START state
        return span_ref._auto(np.zeros((1, 256), np.int64), [True]), None, None
    if name == "d_starts":                  # a match begins wherever a d stands ...
        return span_ref.starts_of([b"d"]), None, None
    assert name == "d_plus"                 # ... and ends behind the last d of its run (d+): a run of d is ONE match, rule 0
    from libfsm_amd import FlatDfa
    dense = np.full((2, 256), -1, np.int64)
    dense[:, ord("d")] = 1
    sets = {1: [0]}
    return (FlatDfa.from_dense(dense, 0, np.array([0, 1], np.uint8), endids=sets), dense, np.arange(256, dtype=np.int64)), sets, None


@functools.lru_cache(maxsize=None)
def auto_of(name):
    """name -> (auto, {state: ids} or None, walked from LDS or None: not asserted); the form is asserted from the Plan"""
    made = _make_auto(name)
    assert made[0][0].start == 0
    return made


@functools.lru_cache(maxsize=None)
def starts_image(name):
    from libfsm_amd import PosDfa
    auto, _, in_lds = auto_of(name)
    pd = PosDfa.from_flat(auto[0])
    assert in_lds is None or pd.in_lds == in_lds       # the form, before any launch
    return pd


def ends_image(name, mode=EARLIEST):
    return _ends_image(name, mode)


@functools.lru_cache(maxsize=None)
def _ends_image(name, mode):
    from libfsm_amd import TokDfa
    auto, _, in_lds = auto_of(name)
    td = TokDfa.from_flat(auto[0], mode)
    assert in_lds is None or td.in_lds == in_lds
    return td


def state_ids(name, mode=EARLIEST):
    """the id of every state of an `ends` (an automaton without ids: NO_ID under EARLIEST, the one empty set under RET)"""
    auto, sets, _ = auto_of(name)
    return tokens_ref.state_ids(auto, mode, sets)


@functools.lru_cache(maxsize=None)
def marks_of(starts):
    """matches_ref.marks of a `starts` over its 1 500 inputs, shared by the pairs it is part of"""
    return matches_ref.marks(auto_of(starts)[0], *inputs_of(starts))


@functools.lru_cache(maxsize=None)
def longest_of(ends):
    """matches_ref.longest_from of an `ends` over its 1 500 inputs, shared by the pairs it is part of"""
    return matches_ref.longest_from(auto_of(ends)[0], *inputs_of(ends))


def reference(starts, ends, flags=0, mode=EARLIEST):
    """the judge's answer for all 1 500 inputs of a pair, computed once a process and left unchanged"""
    return _reference(starts, ends, flags, mode)


@functools.lru_cache(maxsize=None)
def _reference(starts, ends, flags, mode):
    rows, lens = inputs_of(ends)
    assert inputs_of(starts) is inputs_of(ends)
    res = matches_ref.matches(None, None, rows, lens, flags, ids=state_ids(ends, mode), tables=(marks_of(starts),) + longest_of(ends))
    _frozen(*res.values())
    return res


def judged(starts, ends, rows, lens, flags=0, mode=EARLIEST):
    """the judge on other lines than the 1 500: (off, start, end, id)"""
    r = matches_ref.matches(auto_of(starts)[0], auto_of(ends)[0], rows, lens, flags, ids=state_ids(ends, mode))
    return r["off"], r["start"], r["end"], r["id"]
