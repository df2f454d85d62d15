"""The judge of the distinct records (include/fsm_hip.h, "distinct"): the definition restated in plain Python, a dict over the
trimmed keys (and tags) in record order.  Nothing here goes through the library, and nothing that came from the device is ever
handed to it.

A packed text is (off[R + 1], bytes); entries of off are clamped to the bytes that may be read and to their predecessor, as the
extraction clamps; with trim >= 0 a non-empty record whose last byte is the trim byte is one byte shorter."""
import numpy as np

NO_TEXT = 1
WEAK_HASH = 2
MAX_RECORDS = 2 ** 32 - 2


def keys_of(off, data, trim=-1, nbytes=None):
    """the trimmed bytes of every record"""
    o = [int(x) for x in np.asarray(off).astype(np.uint64)]
    b = bytes(np.asarray(data, np.uint8)) if not isinstance(data, (bytes, bytearray)) else bytes(data)
    R = len(o) - 1
    limit = min(o[R], len(b) if nbytes is None else nbytes) if R else 0
    keys = []
    for r in range(R):
        o0, o1 = o[r], o[r + 1]
        n = max(o1 - o0, 0)
        n = 0 if o0 > limit else min(n, limit - o0)
        k = b[o0:o0 + n]
        if trim >= 0 and k and k[-1] == trim:
            k = k[:-1]
        keys.append(k)
    return keys


def distinct(off, data, trim=-1, tag=None, sep=-1, nbytes=None):
    """-> (first u64 [D], count u64 [D], class u32 [R], doff u64 [D + 1], dbytes u8 [doff[D]])"""
    assert -1 <= trim <= 255 and -1 <= sep <= 255
    keys = keys_of(off, data, trim, nbytes)
    assert len(keys) <= MAX_RECORDS and (tag is None or len(tag) == len(keys))
    tail = bytes([sep]) if sep >= 0 else b""
    number, first, count, cls = {}, [], [], []
    for r, k in enumerate(keys):
        key = (k, None if tag is None else int(tag[r]))
        d = number.setdefault(key, len(first))
        if d == len(first):
            first.append(r)
            count.append(0)
        count[d] += 1
        cls.append(d)
    out = [keys[r] + tail for r in first]
    doff = np.concatenate([[0], np.cumsum([len(x) for x in out])]).astype(np.uint64)
    return (np.array(first, np.uint64), np.array(count, np.uint64), np.array(cls, np.uint32), doff, np.frombuffer(b"".join(out), np.uint8))


def pack(records):
    """a list of byte strings -> (off u64 [R + 1], bytes u8)"""
    off = np.concatenate([[0], np.cumsum([len(x) for x in records])]).astype(np.uint64)
    return off, np.frombuffer(b"".join(records), np.uint8)


def table_slots(R):
    s = 16
    while s < 2 * R:
        s *= 2
    return s
