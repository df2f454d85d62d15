"""Test helper of the text front's context (tests/test_text_context_abi.py, tests/test_gpu_text_context.py,
tests/tools/context_probe.py): the rule of include/fsm_hip.h ("Context") stated twice in numpy, independent of the code under
test -- the literal definition and the nearest-witness form --, the marks, and what grep -H -n prints from them."""
import numpy as np

from hits_ref import pack_bits


def file_of(n, file_lines=None):
    """file(i) of every line: 0 for a plain text, else the j with file_lines[j] <= i < file_lines[j + 1]"""
    if file_lines is None:
        return np.zeros(n, np.int64)
    return np.searchsorted(np.asarray(file_lines).astype(np.int64), np.arange(n), side="right") - 1


def context_literal(sel, before, after, file_lines=None):
    """W by the definition: every selected line marks [p - before, p + after] clipped to its file (Python integers: nothing wraps)"""
    sel = np.asarray(sel, bool)
    n = len(sel)
    fl = [0, n] if file_lines is None else [int(x) for x in file_lines]
    fo = file_of(n, file_lines)
    W = np.zeros(n, bool)
    for p in np.flatnonzero(sel).tolist():
        j = int(fo[p])
        W[max(p - int(before), fl[j]):min(p + int(after), fl[j + 1] - 1) + 1] = True
    return W


def context_witness(sel, before, after, file_lines=None):
    """W by the nearest selected line on either side: prevS / nextS / prevF / nextF as running maxima and minima.  A distance
    between two lines is below n, so a context beyond n is n: the clamp changes no comparison."""
    sel = np.asarray(sel, bool)
    n = len(sel)
    if n == 0:
        return np.zeros(0, bool)
    i = np.arange(n, dtype=np.int64)
    before, after = min(int(before), n), min(int(after), n)
    start = np.zeros(n, bool)
    if file_lines is not None:
        fl = np.asarray(file_lines).astype(np.int64)
        start[fl[(fl > 0) & (fl < n)]] = True
    prev_s = np.maximum.accumulate(np.where(sel, i, -1))
    next_s = np.minimum.accumulate(np.where(sel, i, n)[::-1])[::-1]
    prev_f = np.maximum.accumulate(np.where(start, i, 0))                     # the last file start <= i, 0 if none
    first_at = np.minimum.accumulate(np.where(start, i, n)[::-1])[::-1]       # the first file start >= i
    next_f = np.concatenate([first_at[1:], [n]])                              # ... > i
    return ((prev_s >= 0) & (i - prev_s <= after) & (prev_f <= prev_s)) | ((next_s < n) & (next_s - i <= before) & (next_s < next_f))


def marks_ref(sel, W, file_lines=None):
    """(lines, core, group) of the hits of W: core[k] = the hit is selected, group[k] = grep prints -- before it (or it is the first)"""
    sel, W = np.asarray(sel, bool), np.asarray(W, bool)
    lines = np.flatnonzero(W)
    fo = file_of(len(sel), file_lines)
    group = np.ones(len(lines), bool)
    group[1:] = (lines[1:] != lines[:-1] + 1) | (fo[lines[1:]] != fo[lines[:-1]])
    return lines.astype(np.uint64), sel[lines], group


def pack_marks(bits):
    """ceil(m / 64) words, bit k = hit k, the spare bits 0"""
    return pack_bits(bits, 0)


def unpack_marks(words, m):
    return np.unpackbits(np.asarray(words, np.uint64).view(np.uint8), bitorder="little")[:m].astype(bool)


def compose(names, per_file, sels, before, after, number=True, with_name=True):
    """what grep [-H] [-n] -B before -A after prints: per_file[j] = the lines of file j without their newlines, sels[j] = one
    bool per line.  NAME and NUMBER are followed by ':' on a selected line and by '-' on a context line; -- before every group but
    the first."""
    counts = [len(ls) for ls in per_file]
    file_lines = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    sel = np.concatenate([np.asarray(s, bool) for s in sels] + [np.zeros(0, bool)])
    flat = [l for ls in per_file for l in ls]
    lines, core, group = marks_ref(sel, context_literal(sel, before, after, file_lines), file_lines)
    fo = file_of(len(sel), file_lines)
    out = []
    for k, i in enumerate(lines.tolist()):
        j = int(fo[i])
        sep = b":" if core[k] else b"-"
        if group[k] and k != 0:
            out.append(b"--\n")
        out.append((names[j] + sep if with_name else b"") + (b"%d" % (i - int(file_lines[j]) + 1) + sep if number else b"") + flat[i] + b"\n")
    return b"".join(out)
