"""CPU: the plain-C oracle (oracle/dfa_oracle.c) is pinned against
 (a) every committed golden vector -- answers of the REAL reference fsm_exec on the
     reference's own fixtures (tests/retest/*.tst, endids, re_strings) and on the
     BASELINE config DFAs, frozen by tests/golden/make_golden.py;
 (b) live, the real reference (oracle/_ref) on seeded random inputs, when present."""
import numpy as np
import pytest

from common import Golden, all_golden_paths, golden_id
from oracle.pyoracle import Oracle, RefFsm, have_ref

NO = 0xFFFFFFFF


@pytest.mark.parametrize("path", all_golden_paths(), ids=golden_id)
def test_oracle_matches_golden(path):
    g = Golden(path)
    o = Oracle(g.flat)
    base, off = g.packed()
    ret, end = o.exec_offsets(base, off)
    assert np.array_equal(ret, g.ret), g.meta
    assert np.array_equal(end, g.end), g.meta
    if g.expect is not None:  # the fixture's own +/- lines
        assert np.array_equal(ret, g.expect)
    if g.ids_off is not None:
        for i, e in enumerate(end):
            want = g.ids_of(i)
            got = o.endids(int(e)) if e != NO else np.zeros(0, np.uint32)
            assert np.array_equal(got, want)


def test_golden_counts():
    paths = [p for p in all_golden_paths() if "/retest/" in p]
    assert len(paths) == 37  # 37 regexes ...
    assert sum(len(Golden(p).ret) for p in paths) == 115  # ... 115 cases


@pytest.mark.parametrize("name", ["c1.npz", "c3.npz", "c3u.npz", "endids_union_det.npz", "re_strings_1.npz"])
def test_table_walker_equals_group_scan(name):
    import os
    from common import GOLDEN
    g = Golden(os.path.join(GOLDEN, name))
    o = Oracle(g.flat)
    rng = np.random.RandomState(7)
    alpha = np.frombuffer(b"abcdefLlibfsm0123456789xyz_. \0", np.uint8)
    data = alpha[rng.randint(0, len(alpha), (300, 96))]
    lens = rng.randint(0, 97, 300).astype(np.uint32)
    ret, end = o.exec_stride(data, lens)
    end2 = o.table_walk(data, lens)
    assert np.array_equal(end, end2)
    assert np.array_equal(ret == 1, end != NO)
    # the threaded walker of bench.py's full-parity legs: whole rows and the first lens[i] bytes of each row
    for nt in (1, 3, 16):
        assert np.array_equal(o.table_walk_mt(data, nt, lens), end2)
        assert np.array_equal(o.table_walk_mt(data, nt), o.table_walk(data))


def test_oracle_semantics_edge_cases():
    """Appendix B of SURVEY.md: empty input, no start, *end only on match, NUL is data."""
    from libfsm_amd import FlatDfa
    nt = np.full((2, 256), -1, np.int64)
    nt[0, ord("a")] = 1
    nt[1, 0] = 1          # NUL byte is an ordinary symbol for a (ptr,len) stream
    flat = FlatDfa.from_dense(nt, 0, [0, 1])
    o = Oracle(flat)
    assert o.exec_one(b"") == (0, NO)              # start is not an end state
    assert o.exec_one(b"a") == (1, 1)
    assert o.exec_one(b"a\0\0") == (1, 1)
    assert o.exec_one(b"ab") == (0, NO)            # missing edge
    assert o.exec_one(b"b") == (0, NO)
    flat2 = FlatDfa.from_dense(nt, 0, [1, 1])
    assert Oracle(flat2).exec_one(b"") == (1, 0)   # empty input accepts iff start is an end state
    assert Oracle(flat, hasstart=False).exec_one(b"a")[0] == -1  # exec.c:111-114


@pytest.mark.skipif(not have_ref(), reason="oracle/_ref not built")
@pytest.mark.parametrize("dialect,regex,flags", [
    ("pcre", b"[Ll]ibf+(sm)*", 0), ("pcre", b"^ab+c?(de|fg)*$", 0), ("pcre", b"a.c", 16), ("glob", b"foo*bar?", 0),
    ("native", b"(abc|abd)+x", 0), ("pcre", b"^[0-9a-f]{2,4}(:[0-9a-f]{2})*$", 1), ("like", b"a%b_c", 0),
])
def test_oracle_vs_live_reference(dialect, regex, flags):
    f = RefFsm.re_comp(dialect, regex, flags, True, True, endid=3)
    flat = f.flatten()
    o = Oracle(flat)
    rng = np.random.RandomState(11)
    alpha = np.frombuffer(b"abcdefgxLlibsm0123456789:? \0\xff", np.uint8)
    strings = [bytes(alpha[rng.randint(0, len(alpha), rng.randint(0, 24))]) for _ in range(2000)]
    strings += [regex, b"", b"libfsm", b"abbbcdefg", b"foobar", b"fooXXbarz", b"ab:cd:ef", b"abcabdx"]
    r1, e1 = f.exec_strings(strings)
    r2, e2 = o.exec_strings(strings)
    assert np.array_equal(r1, r2) and np.array_equal(e1, e2)
    for e in set(int(x) for x in e1 if x != NO):
        assert np.array_equal(f.endids(e), o.endids(e))


@pytest.mark.skipif(not have_ref(), reason="oracle/_ref not built")
def test_reference_vm_agrees_with_fsm_exec():
    """The reference never tests VM == fsm_exec directly; we do, on accept/reject."""
    f = RefFsm.re_comp("pcre", b"[Ll]ibf+(sm)*", 0, True, True)
    rng = np.random.RandomState(3)
    data = rng.randint(0, 256, (2000, 64)).astype(np.uint8)
    data[::5, 10:16] = np.frombuffer(b"Libfsm", np.uint8)
    ret, _ = f.exec_stride(data)
    for v in (1, 2):
        assert np.array_equal(f.vm_match_stride(data, v), ret)


@pytest.mark.skipif(not have_ref(), reason="oracle/_ref not built")
def test_reference_vm_on_a_literal_set_automaton():
    """Found by bench.py's C5 reference leg (round 3): on re_strings automata of a few thousand states the reference's
    VM v2 stops agreeing with fsm_exec -- its encoder keeps the index into the far-branch address table in the
    instruction's 16-bit dest field (src/libfsm/vm/v2.c:71, :129-131), which wraps beyond 65 535 far branches --
    while v1 and the oracle agree.  v1 is therefore the VM baseline for configs[4]; v2's verdict is recorded, not
    asserted (a fixed reference would agree)."""
    import threading
    out = {}

    def work():
        rng = np.random.RandomState(5)
        alpha = np.frombuffer(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789_-", np.uint8)
        words = sorted(set(bytes(alpha[rng.randint(0, 64, rng.randint(4, 9))]) for _ in range(1000)))
        f = RefFsm.re_strings(words, 0, True)
        rows = alpha[rng.randint(0, 64, (1200, 128))].astype(np.uint8)
        for i in range(0, len(rows), 4):
            w = words[i % len(words)]
            rows[i, -len(w):] = np.frombuffer(w, np.uint8)
        ret, end = f.exec_hoisted_stride(rows)
        o_ret, o_end = Oracle(f.flatten()).exec_stride(rows)
        out.update(ret=ret, end=end, o_ret=o_ret, o_end=o_end, v1=f.vm_match_stride(rows, 1), v2=f.vm_match_stride(rows, 2))

    threading.stack_size(1 << 29)
    t = threading.Thread(target=work)
    t.start()
    t.join()
    threading.stack_size(0)
    assert int((out["ret"] == 1).sum()) >= 300
    assert np.array_equal(out["o_ret"], out["ret"]) and np.array_equal(out["o_end"], out["end"])
    assert np.array_equal(out["v1"] == 1, out["ret"] == 1)
    print("reference VM v2 vs fsm_exec on this automaton:", "agree" if np.array_equal(out["v2"] == 1, out["ret"] == 1) else "MISMATCH")


def test_oracle_eager_outputs_match_golden():
    """tests/eager_output/*.c (22 programs, 89 inputs): the oracle's restatement of exec.c:126-144
    emits exactly the ids the reference's callback received, and the union with the end state's
    end-ids equals each program's own expected_ids (the check run_test() makes, utils.c:170-251)."""
    from common import eager_golden_paths
    paths = eager_golden_paths()
    assert len(paths) == 22
    total = 0
    for path in paths:
        g = Golden(path)
        rows, lens = g.padded_rows()
        o = Oracle(g.flat)
        ret, end, sets = o.exec_eager(rows, lens)
        assert np.array_equal(ret, g.ret) and np.array_equal(end, g.end)
        for i in range(len(rows)):
            assert np.array_equal(sets[i], np.sort(g.eager_of(i))), (g.meta["source"], i)
            want, fail = g.meta["expected"][i], g.meta["expect_fail"][i]
            got = sorted(set(sets[i].tolist()) | set(o.endids(int(end[i])).tolist())) if ret[i] == 1 else []
            if fail or not want:
                assert ret[i] == 0 or not got
            else:
                assert got == want
        total += len(rows)
    assert total == 89


def test_oracle_on_reference_fsm_corpus():
    """319 automata checked into the reference as out*.fsm (pcre, pcre-anchor, pcre-repeat, native, glob,
    like, literal, sql, determinise, minimise, reverse, ...), 8 843 inputs incl. the reference's own
    fsm_generate_matches output: the oracle reproduces fsm_exec on all of them."""
    from common import Corpus
    c = Corpus()
    assert len(c) >= 300
    total = acc = 0
    for k in range(len(c)):
        flat, base, off, ret, end = c.get(k)
        r, e = Oracle(flat).exec_offsets(base, off)
        assert np.array_equal(r, ret) and np.array_equal(e, end), c.names[k]
        total += len(ret)
        acc += int((ret == 1).sum())
    assert total > 8000 and acc > 2500


def test_packed_table_walker_equals_the_goldens(built):
    """oracle_table_walk_packed_mt (the full-parity checker of bench.py's packed-lines legs) on every golden vector: the
    reference's own answers, on 1 and on 3 threads"""
    from common import Golden, all_golden_paths
    from oracle.pyoracle import Oracle
    for p in all_golden_paths():
        g = Golden(p)
        base, off = g.packed()
        want = np.where(g.ret == 1, g.end, 0xFFFFFFFF).astype(np.uint32)
        o = Oracle(g.flat)
        for nt in (1, 3):
            assert np.array_equal(o.table_walk_packed_mt(base, off, nt), want), g.name


@pytest.mark.parametrize("name", ["last16", "first32", "odd_rows", "bytewise_reordered", "dying", "eager40", "eager100"])
def test_affine_family_reference_agrees_with_the_oracle(name, built):
    """tests/global_ref.py judges the GPU walks of tests/test_gpu_global_table.py by the automaton's formula; here the two
    references meet: the formula's walk and the oracle's (fsm_exec restated, on the flat description) on a few hundred rows --
    whole rows, prefixes, resumed from a carried state, and with eager outputs."""
    import global_ref as G
    from oracle.pyoracle import Oracle
    flat, dense, cls = G.family(name)
    kw = G.FAMILY[name][2]
    o = Oracle(flat)
    rng = np.random.RandomState(11)
    n, L = 300, 256
    rows = rng.randint(0, 256, (n, L)).astype(np.uint8)
    lens = G.varlens(n, L, rng)
    st = G.walk(dense, cls, 0, rows)
    assert np.array_equal(o.table_walk(rows), G.ends(flat, st))
    st_len = G.walk(dense, cls, 0, rows, lens)
    assert np.array_equal(o.table_walk(rows, lens), G.ends(flat, st_len))
    start = np.full(n, 0xFFFFFFFD, np.uint32)
    assert np.array_equal(o.state_walk(rows, start, lens), G.carried(st_len))
    assert np.array_equal(o.state_walk(rows, G.carried(st_len), None), G.carried(G.walk(dense, cls, 0, rows, state_in=st_len)))
    if kw.get("holes"):
        assert (st < 0).sum() > 50 and (st >= flat.nstates - kw["sinks"]).sum() > 0
    if kw.get("endids"):
        slots = G.endid_slots(flat.nstates, flat.is_end.astype(bool))
        for s in set(G.ends(flat, st).tolist()) - {0xFFFFFFFF}:
            assert np.array_equal(o.endids(s), slots[s][slots[s] >= 0]) and np.array_equal(flat.endids_of(s), G.endids_of(flat, s))
    if kw.get("eager"):
        E = kw["eager"]
        for ln in (None, lens):
            ret, end, sets = o.exec_eager(rows, ln, cap=E + 8)
            ws, em = G.walk_eager(dense, cls, 0, rows, E, ln)
            assert np.array_equal(end, G.ends(flat, ws))
            assert all(np.array_equal(a, b) for a, b in zip(sets, G.eager_sets(em)))
