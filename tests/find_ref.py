"""The judge of the lookup (include/fsm_hip.h, "find"): the definition restated in plain Python, a dict over distinct_ref.keys_of.
Nothing here goes through the library, and nothing that came from the device is ever handed to it.

The dictionary is a packed text with its trim byte and, optionally, tags: its keys are numbered by first occurrence, as "distinct"
numbers them.  The probe is a second packed text with its own trim byte and tags.  A NULL tag array is tag 0 on either side."""
import numpy as np

import distinct_ref

NO_PICK = 1
NONE = 0xFFFFFFFF


def numbers_of(off, data, trim=-1, tag=None, nbytes=None):
    """the dictionary: {(key bytes, tag): d}, d by first occurrence"""
    number = {}
    for r, k in enumerate(distinct_ref.keys_of(off, data, trim, nbytes)):
        number.setdefault((k, 0 if tag is None else int(tag[r])), len(number))
    return number


def find(number, off, data, trim=-1, tag=None, nbytes=None):
    """the probe (off, data, trim, tag) among the keys of numbers_of(...)
    -> (class u32 [R], bitmap u64 [ceil(R / 64)], pick u64 [R], present)"""
    assert -1 <= trim <= 255
    keys = distinct_ref.keys_of(off, data, trim, nbytes)
    R = len(keys)
    assert R <= distinct_ref.MAX_RECORDS and (tag is None or len(tag) == R)
    cls = np.array([number.get((k, 0 if tag is None else int(tag[r])), NONE) for r, k in enumerate(keys)], np.uint32).reshape(R)
    bits = np.zeros((R + 63) // 64 * 64, bool)              # the bits at and above R stay 0
    bits[:R] = cls != NONE
    bitmap = np.packbits(bits, bitorder="little").view(np.uint64) if R else np.zeros(0, np.uint64)
    there, gone = np.flatnonzero(bits[:R]), np.flatnonzero(~bits[:R])
    return cls, bitmap, np.concatenate([there, gone]).astype(np.uint64), len(there)
