"""The judge of the extraction (include/fsm_hip.h, "extract"): the definition restated in plain Python over
(rows, lens, raw lens, matches, keep, keep_other, sep).  The matches come from tests/matches_ref.py, never from the device, and
nothing here goes through the library.

rows[n][L] uint8; lens[i] the trimmed length and raws[i] the (clipped) byte count of line i; matches = (off[n + 1], start, end,
id) as matches_ref.head / select give them; keep = None (every match) or (nrules, the set of kept ids below nrules); keep_other:
matches with id >= nrules are kept too; sep: -1 or the byte that follows every record."""
import numpy as np

KEEP_OTHER = 1


def kept(idv: int, keep, keep_other: bool) -> bool:
    if keep is None:
        return True
    nrules, ids = keep
    if idv >= nrules:
        return bool(keep_other)
    return idv in ids


def extract(rows, lens, raws, matches, keep=None, keep_other=False, sep=-1):
    """-> (off u64 [R + 1], bytes u8 [off[R]], line u64 [R], match u64 [R])"""
    moff, start, end, ids = matches
    moff = np.asarray(moff).astype(np.int64)
    n = len(moff) - 1
    assert len(lens) == n and len(raws) == n and -1 <= sep <= 255
    tail = bytes([sep]) if sep >= 0 else b""
    recs, off, line, match = [], [0], [], []
    for j in range(n):
        raw = int(raws[j])
        text = bytes(np.asarray(rows[j], np.uint8)[:raw]) if raw else b""
        for k in range(moff[j], moff[j + 1]):
            if not kept(int(ids[k]), keep, keep_other):
                continue
            en = min(int(end[k]), raw)                # every match clamped on its own
            st = min(int(start[k]), en)
            recs.append(text[st:en] + tail)
            off.append(off[-1] + len(recs[-1]))
            line.append(j)
            match.append(k)
    return np.array(off, np.uint64), np.frombuffer(b"".join(recs), np.uint8), np.array(line, np.uint64), np.array(match, np.uint64)


def records_of(off, data):
    """the packed result as a list of byte strings"""
    o = np.asarray(off).astype(np.int64)
    b = bytes(np.asarray(data, np.uint8))
    return [b[o[i]:o[i + 1]] for i in range(len(o) - 1)]


def pack_rules(ids, nrules):
    """-> the bitmap u8 [(nrules + 7) / 8] as fsm_hip_rules_create takes it"""
    bits = np.zeros((nrules + 7) // 8, np.uint8)
    for i in ids:
        assert 0 <= i < nrules
        bits[i >> 3] |= 1 << (i & 7)
    return bits
