"""What tests/test_ldsdma_pack_cases.py (CPU) and tests/test_gpu_ldsdma_pack.py share: a model of walk_ldsdma_pack's pending
queue, the tile kinds and tile sequences that drive it to its edges, and the row builder of the GPU test.

The model is the kernel's rule restated (libfsm_amd/csrc/walk_kernels.h, pack_queue.h): per wavefront, a tile whose live rows
after 16 bytes number more than PACK_MAX_LIVE is walked in place; of any other tile the rows alive after the first segment
(128 bytes) go behind the pending entries in row order, and whenever 64 are pending the first 64 are walked and leave."""
import numpy as np

PACK_MAX_LIVE = 48


def model(tiles):
    """tiles: (alive after 16 bytes, alive after the first segment) bool[64] pairs of ONE wavefront, in its order.
    -> per tile ("I",) or ("Q", count after the push, fired, count after the pop, positions of the survivors), and the flush count"""
    count, out = 0, []
    for live16, live in tiles:
        if int(np.sum(live16)) > PACK_MAX_LIVE:
            out.append(("I",))
            continue
        pos = [count + k for k in range(int(np.sum(live)))]
        pushed = count + len(pos)
        fired = pushed >= 64
        count = pushed - 64 if fired else pushed
        out.append(("Q", pushed, fired, count, pos))
    return out, count


# ---- tile kinds: which of the 64 rows die EARLY (within the first 16 bytes) ------------------------------------------------
_k = np.arange(64)
KINDS = {
    "d0": _k < 0, "d1": _k == 37, "d15": _k < 15, "d16": _k < 16, "alt": _k % 2 == 1, "alt0": _k % 2 == 0, "d63": _k != 5, "d64": _k >= 0,
    "f20": _k < 20, "b20": _k >= 44,
    "d49": (_k % 4 != 0) | (_k == 0),      # 15 live rows: 48 + 15 = 63 pending, which the listed kinds cannot make in five tiles
}
assert int(KINDS["d49"].sum()) == 49 and int(KINDS["d15"].sum()) == 15 and int(KINDS["d63"].sum()) == 63

# five tiles a wavefront; what each is for, and the pending count it ends with when only early deaths occur
SEQUENCES = [
    (("alt", "alt0", "d64", "d0", "d1"), 0),        # exactly 64 -> fires, nothing left; a tile without survivors; in-place tiles; ends empty
    (("d16", "d49", "d16", "d63", "d16"), 32),      # 48, 63, 63 + 48 = 111: into the second set, fires -> 47, 48, 96 -> fires -> 32
    (("alt", "alt0", "d63", "d0", "d15"), 1),       # fires at 64, then ONE entry waits behind two in-place tiles for the flush
    (("d16", "d49", "d0", "d1", "d15"), 63),        # 63 entries wait behind three in-place tiles
    (("f20", "b20", "alt", "d64", "f20"), 36),      # bunched at either end: 44, 88 -> 24, 56, 56, 100 -> 36
    (("alt", "d15", "alt0", "d0", "d16"), 48),      # in-place tiles between queued ones while entries are pending
]
DIE_EARLY = (0, 15)
DIE_MID = (16, 17, 127)             # alive after 16 bytes, dead within the first segment
DIE_LATE = (128, 129, 0)            # in the first packed round, and at the row's last byte (0 stands for stride - 1)


def plan_rows(n, ncu, mixed, stride):
    """die[n]: the byte at which row i turns absorbing, -1 never.  Tile t belongs to wavefront t % ncu (one wavefront per
    workgroup, one workgroup per CU) as its (t // ncu)-th tile: wavefront w runs SEQUENCES[w % len].  mixed: the rows a kind
    leaves alive also die, a third of them in the first segment, a third later."""
    die = np.full(n, -1, np.int64)
    i = np.arange(n)
    t = i // 64
    w, step = t % ncu, (t // ncu) % 5
    for s, (kinds, _) in enumerate(SEQUENCES):
        for k in range(5):
            sel = (w % len(SEQUENCES) == s) & (step == k)
            early = sel & KINDS[kinds[k]][i % 64]
            die[early] = np.take(DIE_EARLY, i[early] % 2)
    if mixed:
        rest = die < 0
        mid, late = rest & (i % 3 == 0), rest & (i % 3 == 1)
        die[mid] = np.take(DIE_MID, (i[mid] // 3) % 3)
        die[late] = np.take(DIE_LATE, (i[late] // 3) % 3)
        die[late & (die == 0)] = stride - 1
    return die


def shares(die):
    """of all rows: dead after 16 bytes, dead after 128 bytes (not before), dead later, never dead"""
    never = die < 0
    return ((die < 16) & ~never).mean(), ((die >= 16) & (die < 128)).mean(), (die >= 128).mean(), never.mean()


def wave_tiles(alive16, alive128, ncu, wave):
    """the (alive after 16, alive after 128) pairs of wavefront `wave`'s tiles, the last one padded with dead rows"""
    n = len(alive16)
    out = []
    for t in range(wave, (n + 63) // 64, ncu):
        a, b = np.zeros(64, bool), np.zeros(64, bool)
        m = min(64, n - t * 64)
        a[:m], b[:m] = alive16[t * 64:t * 64 + m], alive128[t * 64:t * 64 + m]
        out.append((a, b))
    return out
