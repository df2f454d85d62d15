"""The judge of the replacement templates (include/fsm_hip.h, "replace", the template table): the definition restated in plain
Python.  A template table is a list of literal strings R[i] and, per rule, a list of insert positions into R[i]; a match of rule i
with own bytes M and inserts a_0 <= ... <= a_{c-1} becomes

    X = R[i][0:a_0]  M  R[i][a_0:a_1]  M ... M  R[i][a_{c-1}:]

Everything around X is tests/replace_ref.py's: the text between the matches, the trimmed delimiter, a match without a rule stays.
The matches come from tests/matches_ref.py, never from the device, and nothing here goes through the library."""
import numpy as np

import replace_ref


def parse_sed(text: bytes):
    """a sed replacement -> (literal, inserts): & is an insert, \\& and \\\\ are the literals & and \\; a backslash before anything
    else stands for itself; a trailing backslash is a ValueError.  Written apart from the binding's parser, on purpose."""
    lit, ins = b"", []
    rest = bytes(text)
    while rest:
        if rest[:2] in (b"\\&", b"\\\\"):
            lit, rest = lit + rest[1:2], rest[2:]
        elif rest == b"\\":
            raise ValueError("trailing backslash")
        elif rest[:1] == b"&":
            ins, rest = ins + [len(lit)], rest[1:]
        else:
            lit, rest = lit + rest[:1], rest[1:]
    return lit, ins


def x_of(own: bytes, idv: int, table, inserts) -> bytes:
    """what stands for a match whose own bytes are `own` and whose id is idv"""
    if idv >= len(table):
        return own
    r, at = table[idv], list(inserts[idv])
    assert all(0 <= a <= len(r) for a in at) and at == sorted(at), "the judge takes well-formed templates only"
    out, last = [], 0
    for a in at:
        out += [r[last:a], own]
        last = a
    out.append(r[last:])
    return b"".join(out)


def line(raw: bytes, length: int, spans, table, inserts) -> bytes:
    """one line: raw = its bytes with the trimmed delimiter, length = its trimmed length, spans = [(start, end, id)] in order"""
    out, at = [], 0
    for s, e, idv in spans:
        assert at <= s <= e <= length, "the judge takes well-formed matches only"
        out.append(raw[at:s])
        out.append(x_of(raw[s:e], idv, table, inserts))
        at = e
    out.append(raw[at:])
    return b"".join(out)


def replace(rows, lens, raws, matches, table, inserts):
    """-> (out_off u64 [n + 1], bytes u8 [out_off[n]]); inserts[i]: the positions of rule i, or None: no rule has one"""
    if inserts is None:
        inserts = [[] for _ in table]
    assert len(inserts) == len(table)
    off, start, end, ids = matches
    off = np.asarray(off).astype(np.int64)
    n = len(off) - 1
    assert len(lens) == n and len(raws) == n
    outs, o = [], [0]
    for i in range(n):
        raw = bytes(np.asarray(rows[i], np.uint8)[:int(raws[i])]) if int(raws[i]) else b""
        spans = [(int(start[k]), int(end[k]), int(ids[k])) for k in range(off[i], off[i + 1])]
        outs.append(line(raw, int(lens[i]), spans, table, inserts))
        o.append(o[-1] + len(outs[-1]))
    return np.array(o, np.uint64), np.frombuffer(b"".join(outs), np.uint8)


lines_of = replace_ref.lines_of
