"""CPU: the case table of tests/test_gpu_lazy_front.py, checked before anything is launched -- that the planner gives every
automaton of tests/lazy_front_ref.py a lazy image of the kind it was made for (absorbing states reachable or not, clones,
states served by the all-sentinel record, own records that send hits the exact way), and that the lines reach what they are
for: from the reference walk (where a line turns absorbing, which lines end DEAD) and from tests/test_plan.py's Python model
of walk_lazy.h's lazy_step (sentinel steps, clone ids, cuts that fall in a clone or beyond the LDS set).  The planner's image
and the model are used HERE only; no expected answer of the GPU file comes from them.  Nothing here needs a GPU."""
import functools

import numpy as np
import pytest

import global_ref as G
import lazy_front_ref as R
from test_plan import decode_want, lazy_decode, lazy_step

LAZY_QBYTES = 16 * 112 * 16         # walk_lazy.h FSMHIP_LAZY_QBYTES
MODEL_LINES = 400                   # the model is a Python loop per byte


@pytest.fixture(scope="module")
def hip(built):
    import libfsm_amd
    libfsm_amd.load_library()
    return libfsm_amd


@pytest.fixture(scope="module", autouse=True)
def library(built):
    """the automata come from the library's own literal-set builder: every test here needs it built"""


@functools.lru_cache(maxsize=None)
def planned(name):
    import libfsm_amd as hip
    c = R.case(name)
    p = hip.Plan(c.flat, hip.LAYOUT_SPARSE)
    z = lazy_decode(p)
    want = decode_want(c.flat, p) if z is not None else None
    new2old = p.get("new2old").astype(np.int64)
    new2old[p.S1 - 1] = -1                                   # DEAD
    old2new = np.empty(p.S1, np.int64)
    old2new[new2old] = np.arange(p.S1)                       # (old2new[-1]: DEAD's)
    return c, p, z, want, new2old, old2new


def model_walk(name, line, sid=None):
    """the fast path's (id, sentinel step?) after every byte of one line, by the model: lazy_step, and on a sentinel the exact
    step, after which a state beyond the LDS set carries what car[] says -- as walk_lazy.h's lazy_careful does it"""
    c, p, z, want, new2old, old2new = planned(name)
    H, use_abs = z["H"], bool(z["abs_reach"])
    real = lambda x: int(z["cloneof"][x - p.S1]) if x >= p.S1 else x
    sid = p.start if sid is None else sid
    E = sid if sid < H else int(z["car"][sid])
    out = []
    for by in line:
        if real(sid) >= p.abs_min:
            out.append((sid, False))
            continue
        m, rep, sent = lazy_step(z, p.abs_min, sid, E, int(z["sh"][by]), use_abs)
        if sent:
            m = int(want[real(sid)][by])
            rep = m if m < H else int(z["car"][m])
        sid, E = m, rep
        out.append((sid, sent))
    return out


@functools.lru_cache(maxsize=None)
def modelled(name):
    """the model on MODEL_LINES lines of the random block: per line (pool index, [(id, sentinel)] per byte)"""
    c = R.case(name)
    lo, hi = c.random
    return [(i, model_walk(name, c.lines[i])) for i in range(lo, min(hi, lo + MODEL_LINES))]


@pytest.mark.parametrize("name", R.NAMES)
def test_the_planner_makes_the_image_each_automaton_is_for(hip, name):
    c, p, z, want, new2old, old2new = planned(name)
    sp = R.SPEC[name]
    assert c.S < 20000
    assert z is not None, "no lazy image at the default LDS limit"
    img = p.get("lazy")
    assert ((int(img[6]) + 15) & ~15) + LAZY_QBYTES <= 160 * 1024
    assert z["abs_reach"] == sp["abs_reach"]
    assert z["ncl"] > 0
    if name in R.REWIRED:
        assert z["nz"] > 0 and z["nsent"] > 0
    deep = max(p.abs_min - z["H"], 0)
    assert ((z["nz"] + z["nsent"]) * 10 <= deep) == sp["auto"]          # fsm_hip.hip dfa_upload's auto-lazy rule
    print(f"{name}: {c.S} states, H = {z['H']}, F = {z['F']}, {z['ncl']} clones, nz = {z['nz']}, nsent = {z['nsent']}, abs_reach = {z['abs_reach']}, "
          f"auto-lazy {sp['auto']}, image {int(img[6])} bytes of LDS")
    # the absorbing states of the reference are the planner's
    assert int(c.absorbing.sum()) + 1 == p.nabsorbing
    if name in ("abs_accept16", "abs_accept64"):
        assert int(c.absorbing.sum()) == 1 and c.is_end[c.absorbing].all()       # one absorbing accept state


@pytest.mark.parametrize("name", R.ABSORBING)
def test_hand_made_lines_turn_absorbing_where_they_say(name):
    c = R.case(name)
    seen = set()
    for i, ln, k in c.hand:
        assert c.lens[i] == ln and c.kind[i] == "hand"
        gone = (c.tr[i, :ln + 1] < 0) | c.absorbing[np.maximum(c.tr[i, :ln + 1], 0)]       # column t: the state before byte t
        if k is None:
            assert not gone.any(), (name, ln)
        else:
            assert not gone[:k + 1].any() and gone[k + 1:].all(), (name, ln, k)          # not absorbing before byte k, absorbing after it
            rest = c.lines[i][k + 1:]
            if name in R.REWIRED:
                dead = c.tr[i, k + 1] < 0
                assert dead and c.end[i] == R.NO                                           # a byte with no edge from the state reached
                assert len(rest) < 10 or c.accepts_from_start(rest)                        # ... and behind it a text a live state accepts
            else:
                assert c.end[i] != R.NO and c.lines[i][:k + 1].endswith(tuple(c.words))    # the last byte of a word
                assert not c.accepts_from_start(rest)                                      # ... and behind it nothing a live state accepts
        seen.add((ln, k))
    short = min(len(w) for w in c.words) - 1        # a whole line cannot end a word before this index (a resumed piece can: group 4)
    for ln in R.HAND_LENS:
        for k in set(R.HAND_AT + (ln - 1,) + ((ln - ln % 16,) if ln % 16 else ())):
            if k < ln and (name in R.REWIRED or k >= short):
                assert (ln, k) in seen, (name, ln, k)
        assert (ln, None) in seen, (name, ln)


@pytest.mark.parametrize("name", R.NAMES)
def test_shape_block_and_batches(name):
    c = R.case(name)
    lo, hi = c.shape
    ls = c.lens[lo:hi]
    assert hi - lo == 812 and (ls[:400] < 16).all() and set(ls[:400].tolist()) == set(range(16))
    assert (ls[400:800] % 16 == 0).all() and set(ls[400:800].tolist()) == set(range(0, 161, 16))
    assert ls[800:].tolist() == [16 * k + d for k in (1, 2, 3, 4) for d in (-1, 0, 1)]
    assert c.lens[c.EMPTY] == 0 and [int(c.lens[c.tail_idx[t]]) % 16 for t in R.TAILS] == list(R.TAILS)
    for n in R.SIZES + (c.FULL,):
        for tail in R.TAILS:
            idx = c.batch(n, tail)
            assert len(idx) == n
            assert all(c.lens[idx[i]] == 0 for i in R.EMPTY_AT if i < n - 1)
            assert c.lens[idx[-1]] % 16 == tail and (tail == 0) == (c.lens[idx[-1]] == 0)
            base, off = c.packed(idx)
            assert int(off[-1]) == len(base) and int(off[-1]) % 16 == (int(c.lens[idx].sum()) % 16)
    full = c.batch(c.FULL, 7)
    assert sorted(full[full < c.nfull].tolist()) == list(range(c.nfull))                   # every line of the three blocks, once
    assert c.FULL >= 2500
    # the reference on the batch is the reference on its lines: a second, direct walk of the packed text says the same
    idx = c.batch(257, 15)
    base, off = c.packed(idx)
    for i in (1, 100, 255, 256):
        st = R.walk1(c.dense, c.start, bytes(base[int(off[i]):int(off[i + 1])]))
        assert (st[-1] if st else c.start) == c.st[idx[i]]


@pytest.mark.parametrize("name", R.ABSORBING)
def test_random_lines_turn_absorbing_in_chunks_and_in_tails(name):
    """reference only: where a line of the random block first holds an absorbing state (DEAD included) -- inside its whole 16-byte
    chunks (the turn-end test and the unmasked ABS step of walk_lazy_lines) or inside its tail (the masked ABS step of flush())"""
    c = R.case(name)
    lo, hi = c.random
    tr, ls = c.tr[lo:hi], c.lens[lo:hi].astype(np.int64)
    gone = (tr < 0) | c.absorbing[np.maximum(tr, 0)]
    first = np.where(gone.any(axis=1), gone.argmax(axis=1) - 1, -1)         # the index of the byte that did it
    in_chunks = (first >= 0) & (first < ls - ls % 16)
    in_tail = (first >= 0) & (first >= ls - ls % 16)
    print(f"{name}: random lines turning absorbing inside their whole chunks {in_chunks.mean():.3f}, inside their tail {in_tail.mean():.3f}; "
          f"ending DEAD {(c.st[lo:hi] < 0).mean():.3f}")
    assert in_chunks.mean() >= 0.1 and in_tail.mean() >= 0.03
    if name in R.REWIRED:
        assert (c.st[lo:hi] < 0).mean() >= 0.1


@functools.lru_cache(maxsize=None)
def reach(name):
    """tests/test_plan.py's model of the fast path on 400 random lines: it ends where the reference ends (so the model may speak
    for the kernel's path), takes sentinel steps on the rewired pair, ends in clone ids, and the resumed group's random cuts fall
    where the fast path holds a clone id, and a state beyond the LDS set"""
    c, p, z, want, new2old, old2new = planned(name)
    real = lambda x: int(z["cloneof"][x - p.S1]) if x >= p.S1 else x
    runs = modelled(name)
    sent = clone_end = cut_clone = cut_deep = 0
    for i, steps in runs:
        last = steps[-1][0] if steps else p.start
        assert new2old[real(last)] == c.st[i], (name, i)
        sent += any(s for _, s in steps)
        clone_end += last >= p.S1
        cut = int(c.cut["random"][i])
        at = steps[cut - 1][0] if cut else p.start
        cut_clone += at >= p.S1
        cut_deep += at >= z["H"]
    n = len(runs)
    print(f"{name}: of {n} random lines {sent / n:.3f} take a sentinel step, {clone_end / n:.3f} end in a clone id; "
          f"random cuts in a clone id {cut_clone / n:.3f}, in a state >= H {cut_deep / n:.3f}")
    return dict(sent=sent / n, clone_end=clone_end / n, cut_clone=cut_clone / n, cut_deep=cut_deep / n)


@pytest.mark.parametrize("name", R.NAMES)
def test_the_model_says_what_the_lines_reach(hip, name):
    r = reach(name)
    if name in R.REWIRED:
        assert r["sent"] >= 0.5
    if name in R.REWIRED or name == "trie_ids":
        assert r["clone_end"] >= 0.1
    assert r["cut_deep"] >= 0.1
    if name in R.REWIRED or name == "trie_ids":          # (the accept families enter few clones: 0.000 and 0.013 of the cuts)
        assert r["cut_clone"] >= 0.1


def test_a_tenth_of_all_random_cuts_fall_in_a_clone(hip):
    """... over the five automata together, as the resumed group walks them"""
    share = [reach(name)["cut_clone"] for name in R.NAMES]
    assert sum(share) / len(share) >= 0.1, share


@pytest.mark.parametrize("name", R.WITH_IDS)
def test_end_ids_are_what_defines_them(name):
    """trie_ids: word i carries id i and an end state holds the ids of the words that end IN it -- the state the word itself
    leads to from the start state (a longer word that ends the same text has its own state and does not inherit);
    rewired_b: the description holds rewired_ids() for every end state"""
    c = R.case(name)
    low = c.lowest_id(c.st)
    assert ((low != R.NO) == (c.end != R.NO)).all() and ((low != R.NO) & (low != R.NO_ID)).sum() > 200
    if name == "trie_ids":
        owner = {}
        for k, w in enumerate(c.words):
            owner.setdefault(R.walk1(c.dense, c.start, w)[-1], []).append(k)
        for s in np.nonzero(c.is_end)[0].tolist():
            assert c.ids_of(s) == owner.get(s, []), s
    else:
        for s in np.nonzero(c.is_end)[0].tolist():
            assert c.flat.endids_of(s).tolist() == sorted(R.rewired_ids(s)) == c.ids_of(s)


@pytest.mark.parametrize("name", R.NAMES)
def test_cuts_and_pieces_add_up(name):
    """reference only: the second piece walked from the state the first one reached ends where the whole line ends"""
    c = R.case(name)
    idx = c.batch(513, 7)
    for kind in R.CUTS:
        cut = c.cut[kind][idx]
        assert (cut <= c.lens[idx]).all()
        rows, lens = c.rest(idx, cut)
        st = G.walk(c.dense, R.IDENT, c.start, rows, lens, c.state_at(idx, cut))
        assert np.array_equal(st, c.st[idx]), (name, kind)
    assert (c.cut[0] == 0).all() and (c.cut[16][c.lens >= 16] == 16).all()
    if c.has_abs:
        dead_first = (c.state_at(idx, c.cut["random"][idx]) < 0).mean()
        print(f"{name}: first pieces (random cut) that end DEAD {dead_first:.3f}")
