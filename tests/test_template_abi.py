"""CPU: the replacement templates (include/fsm_hip.h, "replace", the template table).  The entry points: exported, in the header, in
the binding's table, failing LOUDLY without a device; the constants; the binding's sed parser; and the judge of
tests/template_ref.py against tests/replace_ref.py where no rule has an insert, and against Python's re.sub where some have."""
import ctypes as C
import errno
import os
import re

import numpy as np
import pytest

import replace_ref
import template_ref
from span_ref import rows_of
from test_matches_abi import WORDS, word_lines
from test_replace_abi import PATTERN, keyword_matches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("fsm_hip_repl_create_template", "fsm_hip_repl_inserts", "fsm_hip_repl_max_inserts")


def test_every_new_symbol_is_exported_and_in_the_table(built):
    import libfsm_amd
    from libfsm_amd import capi
    lib = libfsm_amd.load_library()
    assert [s for s in SYMBOLS if not hasattr(lib, s)] == []
    assert [s for s in SYMBOLS if s not in capi.PROTOTYPES] == []
    header = open(os.path.join(ROOT, "include", "fsm_hip.h")).read()
    assert [s for s in SYMBOLS if s + "(" not in header] == []
    for name in ("template", "from_sed", "parse_sed", "max_inserts"):
        assert callable(getattr(libfsm_amd.HipRepl, name))
    assert isinstance(libfsm_amd.HipRepl.inserts, property)
    # the constants need no device; the cap is an interface condition
    assert lib.fsm_hip_repl_max_inserts() == 255 and libfsm_amd.HipRepl.max_inserts() == 255 and libfsm_amd.repl_max_inserts() == 255
    assert lib.fsm_hip_repl_inserts(None) == 0


def test_no_template_without_a_device(built):
    """no CPU path: ENODEV first, whatever the arguments (with a device, these arguments are EINVAL)"""
    import torch
    import libfsm_amd
    want = errno.EINVAL if torch.cuda.is_available() else errno.ENODEV
    lib = libfsm_amd.load_library()
    roff = np.zeros(2, np.uint64)
    ioff = np.array([1, 1], np.uint64)
    for args in ((None, None, 1, None, None, 0), (None, roff.ctypes.data_as(C.c_void_p), 1, None, None, 1),
                 (None, roff.ctypes.data_as(C.c_void_p), 1, None, ioff.ctypes.data_as(C.c_void_p), 0)):
        C.set_errno(0)
        assert lib.fsm_hip_repl_create_template(*args) is None and C.get_errno() == want, args
    if not torch.cuda.is_available():
        for make in (lambda: libfsm_amd.HipRepl.template([b"<>"], [[1]]), lambda: libfsm_amd.HipRepl.from_sed([b"<&>"])):
            with pytest.raises(OSError) as ei:
                make()
            assert ei.value.errno == errno.ENODEV


@pytest.mark.parametrize("parse", ["binding", "judge"])
def test_sed_replacements_are_parsed(parse):
    if parse == "binding":
        from libfsm_amd import HipRepl
        fn = HipRepl.parse_sed
    else:
        fn = template_ref.parse_sed
    assert fn(b"a&b") == (b"ab", [1])
    assert fn(b"\\&") == (b"&", [])
    assert fn(b"&&") == (b"", [0, 0])
    assert fn(b"") == (b"", [])
    assert fn(b"&") == (b"", [0])
    assert fn(b"<b>&</b>") == (b"<b></b>", [3])
    assert fn(b"\\\\&") == (b"\\", [1])                       # an escaped backslash, then the match
    assert fn(b"\\\\\\&&x&") == (b"\\&x", [2, 3])
    assert fn(b"a\\nb") == (b"a\\nb", [])                    # nothing else is read
    for bad in (b"\\", b"ab\\", b"&\\\\\\"):
        with pytest.raises(ValueError):
            fn(bad)


def test_judge_is_the_plain_judge_where_no_rule_has_an_insert():
    lines = word_lines()
    rows, lens, mt = keyword_matches(lines)
    with_nl = [x + b"\n" for x in lines[:-1]] + [lines[-1]]
    rows2, raws = rows_of(with_nl)
    for table in ([b"<AB>", b"", b"c", b"a much longer replacement than any word", b"bdb"], [b"-", b"", b"xyz"], []):
        want = replace_ref.replace(rows, lens, lens, mt, table)
        for inserts in (None, [[] for _ in table]):
            got = template_ref.replace(rows, lens, lens, mt, table, inserts)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        want = replace_ref.replace(rows2, lens, raws, mt, table)
        got = template_ref.replace(rows2, lens, raws, mt, table, None)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_judge_is_re_sub_with_the_match_in_the_replacement():
    """the sed strings through the judge's parser and the judge, against re.sub with a function that splices by hand"""
    lines = word_lines()
    rows, lens, mt = keyword_matches(lines)
    seds = [b"<&>", b"&&", b"", b"[\\&=&]"]                   # rule 4 beyond the table: stays
    parsed = [template_ref.parse_sed(x) for x in seds]
    table, inserts = [p[0] for p in parsed], [p[1] for p in parsed]
    assert (table, inserts) == ([b"<>", b"", b"", b"[&=]"], [[1], [0, 0], [], [3]])

    def one(mo):
        own = mo.group()
        k = WORDS.index(own)
        return [b"<" + own + b">", own + own, b"", b"[&=" + own + b"]", own][k]

    off, data = template_ref.replace(rows, lens, lens, mt, table, inserts)
    got = template_ref.lines_of(off, data)
    assert got == [PATTERN.sub(one, x) for x in lines]
    assert sum(len(g) > len(x) for g, x in zip(got, lines)) >= 500
    # the identity: an empty R with one insert at 0, for every rule
    off, data = template_ref.replace(rows, lens, lens, mt, [b""] * 5, [[0]] * 5)
    assert template_ref.lines_of(off, data) == lines
    # an empty match gives R[i]
    assert template_ref.line(b"ab\n", 2, [(1, 1, 0)], [b"<>"], [[1]]) == b"a<>b\n"
    assert template_ref.line(b"abc", 3, [(0, 2, 0)], [b"xy"], [[0, 2]]) == b"abxyabc"
    with pytest.raises(AssertionError):
        template_ref.x_of(b"a", 0, [b"xy"], [[3]])             # a position beyond |R|
    with pytest.raises(AssertionError):
        template_ref.x_of(b"a", 0, [b"xy"], [[2, 1]])          # positions that descend
    assert re.sub(b"ab", b"<\\g<0>>", b"xabx") == template_ref.line(b"xabx", 4, [(1, 3, 0)], [b"<>"], [[1]])
