"""CPU: the host half of the text front (libfsm_amd/csrc/lines.cpp, include/fsm_hip.h "text front").

fsm_hip_desc_identity_byte(desc, b) makes byte b a self-loop of every state.  The claim the whole front rests on: walking x
with copies of b put anywhere into it under the twin gives what walking x without any b gives under the ORIGINAL -- accept,
end state, end-ids, eager id set.  Checked with the oracle over every golden automaton the layout tests use and over one
whose original has a real transition on '\\n'; then the structure of the result, the planner's exactness on twins in every
layout, the no-device behaviour of the entry points that need one, and the reference splitter the GPU tests compare with."""
import ctypes
import errno
import os

import numpy as np
import pytest

from common import Golden, all_golden_paths, golden_id
from libfsm_amd import ALL_LAYOUTS, LAYOUT_COMB256, FlatDfa, Plan
from test_plan import check_plan
from text_ref import lines_of, newline_dfa, oracle_answers, split_ref, squeeze_ref

NSTR = 48      # golden inputs walked per automaton (+ the empty string)


def bytes_for(flat):
    """0x0A, 0x00, 0xFF and one byte on which the automaton has real edges (if it has any edge beside those three)"""
    out = [0x0A, 0x00, 0xFF]
    for r in flat.ranges:
        c = next((c for c in range(int(r["lo"]), int(r["hi"]) + 1) if c not in out), None)
        if c is not None:
            out.append(c)
            break
    return out


def cases():
    return [(golden_id(p), p) for p in all_golden_paths()] + [("newline_dfa", None)]


def load(path):
    if path is None:
        return newline_dfa(), [b"a\nb", b"ab", b"a", b"aa\n", b"a\n\na", b"\n", b"a\nba", b"b", b"aaa\nb"]
    g = Golden(path)
    return g.flat, g.strings()[:NSTR]


def with_byte(rng, x, b):
    """x with copies of b at the front, at the back and at random inner positions"""
    y = bytearray(x)
    for _ in range(int(rng.randint(0, 4))):
        y.insert(int(rng.randint(0, len(y) + 1)), b)
    return bytes([b]) * int(rng.randint(0, 3)) + bytes(y) + bytes([b]) * int(rng.randint(0, 3))


@pytest.mark.parametrize("name,path", cases(), ids=[c[0] for c in cases()])
def test_identity_byte_equivalence(name, path, built):
    from libfsm_amd import identity_byte
    flat, strings = load(path)
    strings = list(strings) + [b""]
    rng = np.random.RandomState(len(strings) + flat.nstates)
    bytes_ = bytes_for(flat)
    if path is None:
        assert 0x0A in bytes_ and (flat.dense()[:, 0x0A] != 0xFFFFFFFF).any()
    for b in bytes_:
        twin = identity_byte(flat, b)
        ys = [with_byte(rng, x, b) for x in strings]
        ys[0] = bytes([b]) + ys[0] + bytes([b])            # front and back at least once
        zs = [x.replace(bytes([b]), b"") for x in strings]
        ret_t, end_t, ids_t, sets_t = oracle_answers(twin, ys)
        ret_o, end_o, ids_o, sets_o = oracle_answers(flat, zs)
        assert np.array_equal(ret_t, ret_o), (name, b)
        assert np.array_equal(end_t, end_o), (name, b)
        assert ids_t == ids_o, (name, b)
        assert sets_t == sets_o, (name, b)


@pytest.mark.parametrize("name,path", cases(), ids=[c[0] for c in cases()])
def test_identity_byte_structure(name, path, built):
    from libfsm_amd import identity_byte
    flat, _ = load(path)
    for b in bytes_for(flat):
        twin = identity_byte(flat, b)
        assert (twin.nstates, twin.start) == (flat.nstates, flat.start)
        for f in ("is_end", "endid_off", "endids"):
            assert np.array_equal(getattr(twin, f), getattr(flat, f)), f
        assert (twin.eager_off is None) == (flat.eager_off is None)
        if flat.eager_off is not None:
            assert np.array_equal(twin.eager_off, flat.eager_off) and np.array_equal(twin.eager_ids, flat.eager_ids)
        for s in range(twin.nstates):      # sorted, disjoint
            r = twin.ranges[int(twin.edge_off[s]):int(twin.edge_off[s + 1])]
            lo, hi = r["lo"].astype(int), r["hi"].astype(int)
            assert (lo <= hi).all() and (lo[1:] > hi[:-1]).all(), (name, b, s)
        # the table: column b is the identity, every other column is the original's
        want = flat.dense()
        want[:, b] = np.arange(flat.nstates)
        assert np.array_equal(twin.dense(), want)
        assert np.array_equal(identity_byte(twin, b).dense(), want)      # applying it twice = applying it once


def test_identity_byte_rejects_bad_arguments(built):
    from libfsm_amd import identity_byte
    flat = newline_dfa()
    for b in (-1, 256):
        with pytest.raises(OSError) as ei:
            identity_byte(flat, b)
        assert ei.value.errno == errno.EINVAL
    bad = newline_dfa()
    bad.ranges["to"][0] = 99                # a target that is no state
    with pytest.raises(OSError) as ei:
        identity_byte(bad, 10)
    assert ei.value.errno == errno.EINVAL


@pytest.mark.parametrize("name,path", cases(), ids=[c[0] for c in cases()])
def test_planner_exact_on_twins(name, path, built):
    """every layout the original gets, plus AUTO: the per-(state, byte) decode of tests/test_plan.py on the twin.  The twin has
    the original's states and at most ONE byte class more (the delimiter's column, now the identity, may differ from every other
    byte's), so a layout that holds the original may refuse the twin only where that one class crosses a bound of the layout
    (<= 32 classes for the self-loop masks, the pair table's size) -- and COMB256, which the twin loses by that layout's own
    rule: it wants ONE default target for all 256 byte columns (plan.cpp build_comb), in a regex automaton DEAD, and the
    identity column has no majority target at all.  With an unchanged class count nothing else may be lost."""
    from libfsm_amd import identity_byte
    flat, _ = load(path)
    twin = identity_byte(flat, 0x0A)
    c_orig, c_twin = Plan(flat, 4).C, Plan(twin, 4).C
    assert c_orig <= c_twin <= c_orig + 1
    lost = []
    for L in ALL_LAYOUTS:
        try:
            Plan(flat, L)
        except OSError:
            continue
        if not check_plan(twin, L):
            lost.append(L)
    print(name, "classes", c_orig, "->", c_twin, "layouts the twin loses:", lost)
    if c_twin == c_orig:
        assert set(lost) <= {LAYOUT_COMB256}, lost
    assert check_plan(twin, 0)
    assert Plan(twin, 4).layout == 4, "the global layout must hold any DFA"


def test_no_device_means_enodev(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from libfsm_amd import HipText, LinesDfa
    for make in (lambda: HipText(b"a\nb\n"), lambda: HipText(d_text=4096, nbytes=16), lambda: LinesDfa(newline_dfa())):
        with pytest.raises(OSError) as ei:
            make()
        assert ei.value.errno == errno.ENODEV


def test_reference_splitter():
    """split_ref states the line rule of the header; squeeze_ref is hipgrep.c's squeezed copy; lines_of cuts by bytes.split"""
    def offs(t, d=0x0A):
        return split_ref(t, d).tolist()
    assert offs(b"") == [0]
    assert offs(b"\n") == [0, 1]
    assert offs(b"a") == [0, 1]
    assert offs(b"a\n") == [0, 2]
    assert offs(b"a\nb") == [0, 2, 3]
    assert offs(b"\n\na\n\n") == [0, 1, 2, 4, 5]
    assert offs(b"a\r\nb\r\n") == [0, 3, 6]               # no CRLF handling: the '\r' stays in its line
    assert offs(b"a\0b\0", 0) == [0, 2, 4] and offs(b"\xffa\xff\xff", 0xFF) == [0, 1, 3, 4]
    rng = np.random.RandomState(4)
    for d in (0x0A, 0x00, 0x80, 0xFF):
        for n in (0, 1, 2, 17, 300):
            t = rng.choice(np.array([d, d ^ 0x80, (d + 1) & 0xFF, 0x41], np.uint8), n)
            off = split_ref(t, d)
            lines = lines_of(t, d)
            assert len(lines) == len(off) - 1
            sq, so, k = squeeze_ref(t, d)
            assert k == len(lines) and [bytes(sq[int(so[i]):int(so[i + 1])]) for i in range(k)] == lines
            for i, ln in enumerate(lines):                  # [off[i], off[i + 1]) = the line + at most its one delimiter
                piece = bytes(t[int(off[i]):int(off[i + 1])])
                assert piece in (ln, ln + bytes([d])) and bytes([d]) not in ln
