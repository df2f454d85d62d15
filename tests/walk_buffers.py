"""Device and host buffers, calls and knob settings shared by the GPU suites that drive one table layout over every input path
(tests/test_gpu_pair_table.py, tests/test_gpu_column_table.py).  A plain helper module: no test lives here.

Every output buffer (Out) is two entries longer than the batch and pre-filled with junk; nothing behind the batch may be
written.  The packed batches (Packed) start OFF0 bytes into their text, in every metadata form, and the device text is exactly
off[n] bytes long."""
from collections import namedtuple

import numpy as np

import global_ref as G
from pair_table_ref import OFF0, packed_from

NO = G.NO
JUNK32, JUNK64 = 0x5A5A5A5A, 0xA5A5A5A5A5A5A5A5
IN_DIRECT, IN_LDSDMA, IN_GENERIC, IN_RAGGED = 0, 1, 2, 3
NO_LINES32 = 32                                          # FSM_HIP_KNOB_EARLY_RETIRE bit 5: a packed batch takes walk_generic's own body

Knobs = namedtuple("Knobs", "label mode seg nb pre nt pack")
DEFAULT = Knobs("default", -1, 0, 0, -1, -1, -1)
SETTINGS = (DEFAULT,
            Knobs("lds-dma 64", IN_LDSDMA, 64, 0, -1, -1, 0),
            Knobs("lds-dma 128, nontemporal", IN_LDSDMA, 128, 0, -1, 1, 0),
            Knobs("lds-dma 128, temporal", IN_LDSDMA, 128, 0, -1, 0, 0),
            Knobs("packing, nontemporal", IN_LDSDMA, 128, 0, -1, 1, 1),
            Knobs("packing, temporal", IN_LDSDMA, 128, 0, -1, 0, 1),
            Knobs("direct 4", IN_DIRECT, 0, 4, 1, -1, -1),
            Knobs("direct 8", IN_DIRECT, 0, 8, 1, -1, -1),
            Knobs("direct, no prefetch", IN_DIRECT, 0, 4, 0, -1, -1),
            Knobs("generic", IN_GENERIC, 0, 0, -1, -1, -1),
            Knobs("ragged", IN_RAGGED, 0, 0, -1, -1, -1))


def set_knobs(dfa, hip, k):
    for knob, v in ((hip.KNOB_INPUT_MODE, k.mode), (hip.KNOB_SEG, k.seg), (hip.KNOB_NB, k.nb), (hip.KNOB_PREFETCH, k.pre), (hip.KNOB_NT, k.nt),
                    (hip.KNOB_PACK, k.pack)):
        dfa.tune(knob, v)


def to_dev(a, pad=0):
    """the array's bytes on the device, in a buffer of exactly that size + pad (one byte where there are none)"""
    import torch
    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    if pad or not len(b):
        b = np.concatenate([b, np.zeros(max(pad, 0 if len(b) else 1), np.uint8)])
    return torch.from_numpy(b.copy()).cuda()


class Buf:
    """an input array on the host and, made once, on the device"""

    def __init__(self, a, pad=0):
        self.a = np.ascontiguousarray(a)
        self.pad, self.t = pad, None

    def p(self, dev):
        if not dev:
            return self.a.ctypes.data if self.a.size else None
        if self.t is None:
            self.t = to_dev(self.a, self.pad)
        return self.t.data_ptr()


class Out:
    """end states, bitmap, ids and carried states of one call, on the host or the device: two entries longer than the batch,
    pre-filled with junk (the carried states: the states handed in, then junk)"""

    def __init__(self, n, dev, state=None, ids=False):
        self.n, self.dev, self.w = n, dev, (n + 63) // 64
        self.a = {"end": np.full(n + 2, JUNK32, np.uint32), "bm": np.full(self.w + 2, JUNK64, np.uint64)}
        if ids:
            self.a["ids"] = np.full(n + 2, JUNK32, np.uint32)
        if state is not None:
            self.a["st"] = np.concatenate([np.asarray(state, np.uint32)[:n], np.full(2, JUNK32, np.uint32)])
        self.t = {k: to_dev(v) for k, v in self.a.items()} if dev else None

    def p(self, k):
        return self.t[k].data_ptr() if self.dev else self.a[k].ctypes.data

    def check(self, want_end, *tag, carried=None, ids=None, bitmap=True):
        if self.dev:
            import torch
            torch.cuda.synchronize()
            self.a = {k: t.cpu().numpy().view(self.a[k].dtype) for k, t in self.t.items()}
        n, a = self.n, self.a
        end = a["end"]
        bad = np.nonzero(end[:n] != want_end)[0]
        assert len(bad) == 0, (tag, f"{len(bad)} of {n} end states differ", bad[:8].tolist(), end[bad[:8]].tolist(), np.asarray(want_end)[bad[:8]].tolist())
        assert (end[n:] == JUNK32).all(), (tag, "end states behind the batch written")
        if bitmap:
            got = np.unpackbits(a["bm"][:self.w].view(np.uint8), bitorder="little")[:n].astype(bool)
            assert np.array_equal(got, want_end != NO), (tag, "bitmap")
        else:
            assert (a["bm"][:self.w] == JUNK64).all(), (tag, "a bitmap nobody asked for")
        assert (a["bm"][self.w:] == JUNK64).all(), (tag, "bitmap words behind the batch written")
        if carried is not None:
            st = a["st"]
            bad = np.nonzero(st[:n] != carried)[0]
            assert len(bad) == 0, (tag, f"{len(bad)} of {n} carried states differ", bad[:8].tolist(), st[bad[:8]].tolist(), np.asarray(carried)[bad[:8]].tolist())
            assert (st[n:] == JUNK32).all(), (tag, "carried states behind the batch written")
        if ids is not None:
            assert (a["ids"][n:] == JUNK32).all(), (tag, "ids behind the batch written")
            return a["ids"][:n]
        return None


def call(name, dev, dfa, *args):
    """the host entry point, or its _device twin with the stream (none) behind the same arguments"""
    from libfsm_amd.capi import _call
    _call(name + "_device", dfa.handle, *args, None) if dev else _call(name, dfa.handle, *args)


def walk_rows(dfa, dev, base, stride, lens, n, o):
    call("fsm_hip_exec_batch", dev, dfa, base.p(dev), stride, lens.p(dev) if lens is not None else None, n, o.p("end"), o.p("bm"))


PACKED_FORMS = ("u64 offsets", "u32 offsets", "lengths", "packed_all u64", "packed_all u32", "packed_all lengths")


class Packed:
    """lines packed behind OFF0 bytes that belong to no line, in every metadata form; the device text is exactly off[n] bytes"""

    def __init__(self, rows, lens, n):
        lens = np.asarray(lens[:n], np.uint32)
        base, off = packed_from(rows[:n], lens)
        assert int(off[0]) == OFF0 and len(base) == int(off[n])
        self.n, self.lens_np, self.total = n, lens, int(off[n])
        self.base, self.off, self.off32, self.lens = Buf(base), Buf(off), Buf(off.astype(np.uint32)), Buf(lens)
        # the lengths-only form has no offset to start from: its text begins at the first line (the address is odd all the same)
        self.base_l = Buf(base[OFF0:])

    def mean(self, dev, form):
        """what the front holds against the pick threshold: a host front its last offset over n, the device the batch's bytes over n"""
        return (self.total - (OFF0 if dev or "lengths" in form else 0)) // self.n

    def walk(self, dfa, dev, form, o):
        meta = self.lens if "lengths" in form else self.off if "u64" in form else self.off32
        base = self.base_l if "lengths" in form else self.base
        if form.startswith("packed_all"):
            k = {"u64": 0, "u32": 1, "lengths": 2}[form.split()[-1]]
            call("fsm_hip_exec_batch_packed_all", dev, dfa, base.p(dev), k, meta.p(dev), self.n, o.p("end"), o.p("bm"), 0, None, None)
        else:
            fn = {"u64 offsets": "offsets", "u32 offsets": "offsets32", "lengths": "lengths"}[form]
            call("fsm_hip_exec_batch_" + fn, dev, dfa, base.p(dev), meta.p(dev), self.n, o.p("end"), o.p("bm"))
