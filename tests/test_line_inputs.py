"""CPU: the shared inputs of tests/line_inputs.py are what the GPU test files of the line fronts used to build for themselves.

The digests below were taken from those files' own make_inputs / keyword_inputs / lead_packed at the commit before
line_inputs.py (spans, tokens, matches, replace, extract, template: every copy gave the same bytes), not from this module:
SHA-256 over the arrays' bytes in the order given, dtypes and shapes as asserted."""
import hashlib

import numpy as np

import line_inputs

MAKE_INPUTS = "c7c85c8b3d95952bac7bb018cbc0cc32c2b772ba4ed8ad61b6d62bef56afed41"        # rows u8 [1500][300], lens i64 [1500]
KEYWORD_INPUTS = "370817659debf68ef4b51ccc0a15a3c66c18c544c413a77d510e82589dc310c2"     # rows u8 [1500][300], lens i64 [1500]
LEAD_PACKED = "2df16bcd011bfce8ec1e83dede26225e6d6455d72de36be9d969dfbfb7015724"        # data u8, off u64 [1501] of make_inputs()


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def is_rows_and_lens(rows, lens):
    return rows.dtype == np.uint8 and rows.shape == (1500, 300) and lens.dtype == np.int64 and lens.shape == (1500,)


def test_random_rows():
    rows, lens = line_inputs.make_inputs()
    assert is_rows_and_lens(rows, lens) and sha(rows, lens) == MAKE_INPUTS
    assert lens[:8].tolist() == [0, 1, 15, 16, 17, 31, 32, 33]


def test_keyword_lines():
    rows, lens = line_inputs.keyword_inputs()
    assert is_rows_and_lens(rows, lens) and sha(rows, lens) == KEYWORD_INPUTS
    assert int(lens[8]) == 300 and (rows[8] == ord("d")).all()
    other = np.arange(1500) != 8
    assert np.array_equal(lens[other], line_inputs.make_inputs()[1][other])             # the same 1 500 lengths but line 8's


def test_lines_packed_behind_a_lead():
    rows, lens = line_inputs.make_inputs()
    data, off = line_inputs.lead_packed(rows, lens)
    assert data.dtype == np.uint8 and off.dtype == np.uint64 and off.shape == (1501,) and sha(data, off) == LEAD_PACKED
    assert int(off[0]) == line_inputs.LEAD == 5 and len(data) == int(off[-1]) and (data[:5] == 0x5A).all()
    short, off3 = line_inputs.lead_packed(rows[:4], lens[:4], 3)
    assert off3.tolist() == [3, 3, 4, 19, 35] and bytes(short[4:19]) == bytes(rows[2, :15])


def test_inputs_are_built_once_and_read_only():
    for make in (line_inputs.make_inputs, line_inputs.keyword_inputs):
        first, again = make(), make()
        assert all(a is b for a, b in zip(first, again)) and not any(a.flags.writeable for a in first)
    assert line_inputs.inputs_of("kw_ends") is line_inputs.keyword_inputs() is line_inputs.inputs_of("kw_starts_everywhere")
    assert line_inputs.inputs_of("glob_first") is line_inputs.make_inputs() is line_inputs.inputs_of("sink_one")


def test_constants():
    assert line_inputs.KEYWORDS == [b"ab", b"abc", b"ca", b"d", b"bdb"] and line_inputs.EMPTY_RULE == 5
    assert line_inputs.SIZES == (1, 63, 64, 65, 255, 256, 257, 1500) and line_inputs.FILL == 0xA5A5A5A5A5A5A5A5
