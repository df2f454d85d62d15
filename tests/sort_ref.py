"""The judge of the sort of a packed text (include/fsm_hip.h, "sort"): the definition restated in plain Python, sorted() over the
trimmed keys of tests/distinct_ref.keys_of.  Nothing here goes through the library, and nothing that came from the device is ever
handed to it.

Keys order as memcmp does -- Python's bytes order: unsigned bytes, a proper prefix before the longer key.  With major, records
order by major[r] first.  REVERSE turns the order of the keys round (the longer key before its prefix), MAJOR_DESC that of major;
records equal in both keep ascending r under every flag."""
import numpy as np

from distinct_ref import keys_of

NO_TEXT, REVERSE, MAJOR_DESC, BY_COUNT = 1, 2, 4, 8
MAX_RECORDS = 2 ** 32 - 2


def sort_keys(keys, major=None, sep=-1, flags=0):
    """the judge over the trimmed keys themselves -> (order u64 [R], rank u32 [R], groups, soff u64 [R + 1], sbytes u8)"""
    assert -1 <= sep <= 255 and flags & ~(NO_TEXT | REVERSE | MAJOR_DESC) == 0 and (major is not None or not flags & MAJOR_DESC)
    R = len(keys)
    assert R <= MAX_RECORDS and (major is None or len(major) == R)
    mj = [0] * R if major is None else [int(x) for x in major]
    msign = -1 if flags & MAJOR_DESC else 1
    # descending keys as ascending ones: every byte complemented and an end mark above every byte, so the longer key comes first
    kk = [tuple(255 - x for x in k) + (256,) for k in keys] if flags & REVERSE else keys
    order = sorted(range(R), key=lambda r: (msign * mj[r], kk[r], r))
    rank, g = [], -1
    for p, r in enumerate(order):
        if p == 0 or (mj[r], keys[r]) != (mj[order[p - 1]], keys[order[p - 1]]):
            g += 1
        rank.append(g)
    tail = bytes([sep]) if sep >= 0 else b""
    out = [keys[r] + tail for r in order]
    soff = np.concatenate([[0], np.cumsum([len(x) for x in out])]).astype(np.uint64)
    return np.array(order, np.uint64), np.array(rank, np.uint32), g + 1, soff, np.frombuffer(b"".join(out), np.uint8)


def sort(off, data, trim=-1, major=None, sep=-1, flags=0, nbytes=None):
    """the judge over a packed text; FSM_HIP_SORT_NO_TEXT changes nothing here: the caller leaves soff / sbytes unread"""
    assert -1 <= trim <= 255
    return sort_keys(keys_of(off, data, trim, nbytes), major, sep, flags & ~NO_TEXT)
