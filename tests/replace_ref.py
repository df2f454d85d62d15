"""The judge of the replacement (include/fsm_hip.h, "replace"): the definition restated in plain Python over
(rows, lens, raw lens, matches, table, flags).  The matches come from tests/matches_ref.py, never from the device, and nothing
here goes through the library.

rows[n][L] uint8; lens[i] the trimmed length and raws[i] the byte count of line i (raws[i] - lens[i] is 0 or 1: the trimmed
delimiter, which is copied); matches = (off[n + 1], start, end, id) as matches_ref.head / select give them; table = a list of
byte strings, R[i]; flags: MASK."""
import numpy as np

MASK = 1


def x_of(own: bytes, idv: int, table, flags: int) -> bytes:
    """what stands for a match whose own bytes are `own` and whose id is idv"""
    if idv >= len(table):
        return own                                   # a rule without a replacement, NO_ID, NO_MATCH: the text stays
    r = table[idv]
    if flags & MASK:
        if len(r) == 0:
            return own
        return bytes(r[t % len(r)] for t in range(len(own)))
    return r


def line(raw: bytes, length: int, spans, table, flags: int = 0) -> bytes:
    """one line: raw = its bytes with the trimmed delimiter, length = its trimmed length, spans = [(start, end, id)] in order"""
    out, at = [], 0
    for s, e, idv in spans:
        assert at <= s <= e <= length, "the judge takes well-formed matches only"
        out.append(raw[at:s])
        out.append(x_of(raw[s:e], idv, table, flags))
        at = e
    out.append(raw[at:length])
    out.append(raw[length:])
    return b"".join(out)


def replace(rows, lens, raws, matches, table, flags: int = 0):
    """-> (out_off u64 [n + 1], bytes u8 [out_off[n]])"""
    off, start, end, ids = matches
    off = np.asarray(off).astype(np.int64)
    n = len(off) - 1
    assert len(lens) == n and len(raws) == n
    outs, o = [], [0]
    for i in range(n):
        raw = bytes(np.asarray(rows[i], np.uint8)[:int(raws[i])]) if int(raws[i]) else b""
        spans = [(int(start[k]), int(end[k]), int(ids[k])) for k in range(off[i], off[i + 1])]
        outs.append(line(raw, int(lens[i]), spans, table, flags))
        o.append(o[-1] + len(outs[-1]))
    return np.array(o, np.uint64), np.frombuffer(b"".join(outs), np.uint8)


def lines_of(out_off, data):
    """the packed result as a list of byte strings"""
    o = np.asarray(out_off).astype(np.int64)
    b = bytes(np.asarray(data, np.uint8))
    return [b[o[i]:o[i + 1]] for i in range(len(o) - 1)]


def pack_table(table):
    """-> (bytes u8, roff u64 [nrepl + 1]) as fsm_hip_repl_create takes them"""
    roff = np.zeros(len(table) + 1, np.uint64)
    roff[1:] = np.cumsum([len(r) for r in table]) if table else []
    return np.frombuffer(b"".join(table), np.uint8), roff
