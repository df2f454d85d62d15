"""libfsm_amd/csrc/pack_queue.h (the bookkeeping of walk_ldsdma_pack's pending queue: the in-place rule, a survivor's queue
position, the count, when a packed walk fires) as a stand-alone g++ program that links no HIP, held against the model in
tests/ldsdma_pack_ref.py over the tile sequences the GPU test (tests/test_gpu_ldsdma_pack.py) builds its rows from."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import ldsdma_pack_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "test_pack_queue.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    out = str(tmp_path_factory.mktemp("packq") / "test_pack_queue")
    cc = subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", SRC, "-o", out], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    return out


def run(exe, tiles):
    text = "".join("%x %x\n" % (sum(1 << k for k in range(64) if a[k]), sum(1 << k for k in range(64) if b[k])) for a, b in tiles)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    lines = r.stdout.split("\n")
    assert lines[0] == "M %d" % P.PACK_MAX_LIVE
    out = []
    for ln in lines[1:]:
        f = ln.split()
        if f and f[0] == "I":
            out.append(("I",))
        elif f and f[0] == "Q":
            out.append(("Q", int(f[1]), f[2] == "1", int(f[3]), [int(x) for x in f[4:]]))
        elif f and f[0] == "F":
            return out, int(f[1])
    raise AssertionError(r.stdout[-500:])


def seq_tiles(kinds, late=None):
    """a wavefront's tiles from tile kinds; late: rows that outlive 16 bytes but not the first segment"""
    tiles = []
    for j, k in enumerate(kinds):
        a = ~P.KINDS[k]
        b = a.copy()
        if late is not None:
            b &= (np.arange(64) + j) % late != 0
        tiles.append((a, b))
    return tiles


@pytest.mark.parametrize("s", range(len(P.SEQUENCES)))
def test_sequences_of_the_gpu_test(exe, s):
    kinds, left = P.SEQUENCES[s]
    tiles = seq_tiles(kinds)
    want = P.model(tiles)
    assert want[1] == left                      # the sequence does what its comment says
    assert run(exe, tiles) == want
    for late in (2, 3, 7):                      # rows that die between byte 16 and the first segment's end never queue
        tiles = seq_tiles(kinds, late)
        assert run(exe, tiles) == P.model(tiles)


def test_events_the_sequences_are_for():
    ev = [P.model(seq_tiles(k))[0] for k, _ in P.SEQUENCES]
    pushed = [[t[1] for t in e if t[0] == "Q"] for e in ev]
    assert 64 in pushed[0]                                          # exactly 64
    assert pushed[1][:3] == [48, 63, 111]                           # 63 pending + 48 new: the second set fills to position 110
    assert [P.model(seq_tiles(k))[1] for k, _ in P.SEQUENCES][:4] == [0, 32, 1, 63]
    for e in (ev[2], ev[3], ev[5]):                                 # an in-place tile while entries are pending
        kinds_seen = [t[0] for t in e]
        assert "I" in kinds_seen[kinds_seen.index("Q"):]


def test_either_side_of_the_in_place_bound(exe):
    for dead in range(0, 65):
        a = np.arange(64) >= dead
        got, left = run(exe, [(a, a)])
        if 64 - dead > P.PACK_MAX_LIVE:
            assert got == [("I",)] and left == 0
        else:
            assert got == [("Q", 64 - dead, False, 64 - dead, list(range(64 - dead)))] and left == 64 - dead


def test_long_random_runs(exe):
    rng = np.random.RandomState(5)
    for p in (0.1, 0.3, 0.5, 0.9):
        tiles = []
        for _ in range(400):
            a = rng.rand(64) >= p
            tiles.append((a, a & (rng.rand(64) >= 0.2)))
        want = P.model(tiles)
        assert run(exe, tiles) == want
        assert all(t[3] < 64 and t[1] < 128 for t in want[0] if t[0] == "Q")
