"""The tally (include/fsm_hip.h, "tally") restated in numpy: the judge of tests/test_gpu_tally.py and of tests/tools/tally_probe.py.

count is np.bincount over (group, col(id)) of every entry; lines is the same over the DISTINCT (input, col) pairs."""
import numpy as np

NO_MATCH = 0xFFFFFFFF
NO_ID = 0xFFFFFFFE
ADD = 1


def col(ids, nrules):
    """the column of every id: itself below nrules, else nrules ("other")"""
    ids = np.asarray(ids, np.uint32).astype(np.int64)
    return np.where(ids < nrules, ids, nrules)


def groups_of(m, group_off):
    """(G, the group of every input, or -1 for an input that is counted nowhere): the LAST g in [0, G) with group_off[g] <= j,
    provided j < group_off[G]"""
    if group_off is None:
        return 1, np.zeros(m, np.int64)
    goff = np.asarray(group_off, np.uint64).astype(np.int64)
    G = len(goff) - 1
    j = np.arange(m, dtype=np.int64)
    g = np.searchsorted(goff[:G], j, "right") - 1
    return G, np.where((g >= 0) & (j < goff[G]), g, -1)


def tally(off, ids, nrules, group_off=None):
    """-> (count, lines), each (G, nrules + 1) u64.  off[m + 1] ascending, an entry above len(ids) is len(ids)"""
    ids = np.asarray(ids, np.uint32)
    total = len(ids)
    off = np.minimum(np.asarray(off, np.uint64), np.uint64(total)).astype(np.int64)
    m = len(off) - 1
    C = nrules + 1
    G, group = groups_of(m, group_off)
    owner = np.repeat(np.arange(m, dtype=np.int64), np.diff(off))          # the input of every entry from off[0] on
    c = col(ids[off[0]:off[m]], nrules)
    g = group[owner]
    keep = g >= 0
    count = np.bincount(g[keep] * C + c[keep], minlength=G * C)
    pairs = np.unique(owner[keep] * C + c[keep])                            # distinct (input, col)
    lines = np.bincount(group[pairs // C] * C + pairs % C, minlength=G * C)
    return count.astype(np.uint64).reshape(G, C), lines.astype(np.uint64).reshape(G, C)
