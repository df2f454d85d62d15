"""ctypes binding of libfsm_hip.so -- the C ABI declared in include/fsm_hip.h.

Python is only the harness language here (tests, bench.py); the product is the
shared library.  Nothing in this module matches inputs on the CPU: every
exec_* call goes through the HIP kernels and raises if the library or a GPU is
missing.

The ABI is stated once, in PROTOTYPES and the struct mirrors below; load_library() applies the table to the library it
returns, and tests/test_capi_prototypes.py holds table, mirrors and constants to the headers as the compiler reads them.
"""
from __future__ import annotations

import ctypes as C
import os
from contextlib import contextmanager
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

NO_MATCH = 0xFFFFFFFF
NO_ID = 0xFFFFFFFE
STATE_START = 0xFFFFFFFD
STATE_DEAD = 0xFFFFFFFC

LAYOUT_AUTO, LAYOUT_TINY, LAYOUT_LDS, LAYOUT_COMB, LAYOUT_GLOBAL, LAYOUT_COMB256, LAYOUT_COMBSELF, LAYOUT_SPARSE, LAYOUT_LDSSELF, LAYOUT_LDS2 = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9
META_OFF64, META_OFF32, META_LENGTHS = 0, 1, 2   # fsm_hip_exec_batch_packed_all: what the metadata array is
LAYOUT_NAMES = {1: "tiny", 2: "lds", 3: "comb", 4: "global", 5: "comb256", 6: "combself", 7: "sparse", 8: "ldsself", 9: "lds2"}
ALL_LAYOUTS = (LAYOUT_TINY, LAYOUT_COMBSELF, LAYOUT_LDS2, LAYOUT_COMB256, LAYOUT_LDSSELF, LAYOUT_LDS, LAYOUT_COMB, LAYOUT_SPARSE, LAYOUT_GLOBAL)
NO_EARLY_RETIRE = 0x10
DEFER_UPLOAD = 0x20      # plan now, upload the layout's device image at the first call that needs it (fsm_hip_exec_multi never does)

KNOB_INPUT_MODE, KNOB_NB, KNOB_ROWS, KNOB_WAVES, KNOB_BLOCKS_PER_CU, KNOB_EARLY_RETIRE, KNOB_MASK, KNOB_HOT_BYTES, KNOB_SEG, KNOB_PREFETCH, KNOB_NT = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11
KNOB_NOSKIP = 13
KNOB_RAGGED_ALIGN = 14
KNOB_DMA_BUFS = 15
KNOB_PICK_MEAN, KNOB_SPARSE_FAST, KNOB_LAZY_DYN, KNOB_LAZY_LINES, KNOB_PACK = 18, 20, 21, 22, 23
IN_DIRECT, IN_LDSDMA, IN_GENERIC, IN_RAGGED = 0, 1, 2, 3
HITS_INVERT, HITS_NO_BYTES = 1, 2
NO_POS = 0xFFFFFFFFFFFFFFFF
POS_BACKWARD = 1
TOKENS_NO_BACKTRACK, TOKENS_SKIP_BAD = 1, 2
MATCHES_DROP_EMPTY = 1
REPL_MASK = 1
RULES_KEEP_OTHER = 1
TALLY_ADD = 1
DISTINCT_NO_TEXT = 1
DISTINCT_WEAK_HASH = 2
FIND_NO_PICK = 1
FOUND_NONE = 0xFFFFFFFF
SORT_NO_TEXT, SORT_REVERSE, SORT_MAJOR_DESC, SORT_BY_COUNT = 1, 2, 4, 8
IDS_EARLIEST, IDS_RET, IDS_ERROR = 1, 2, 3

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfsm_hip.so")

# ---- the ABI: structs -------------------------------------------------------------------------------------------------------
P, S, I, U, U32, U64, D, STR = C.c_void_p, C.c_size_t, C.c_int, C.c_uint, C.c_uint32, C.c_uint64, C.c_double, C.c_char_p
PP = C.POINTER(C.c_void_p)

RANGE_DTYPE = np.dtype([("lo", "u1"), ("hi", "u1"), ("reserved", "<u2"), ("to", "<u4")])


class _Desc(C.Structure):
    """struct fsm_hip_dfa_desc"""
    _fields_ = [("nstates", U32), ("start", U32), ("edge_off", P), ("ranges", P), ("is_end", P), ("endid_off", P), ("endids", P),
                ("eager_off", P), ("eager_ids", P)]


class _Info(C.Structure):
    """struct fsm_hip_dfa_info"""
    _fields_ = [("nstates", U32), ("nclasses", U32), ("layout", U32), ("nabsorbing", U32), ("table_bytes", U64), ("lds_bytes", U32),
                ("waves_per_block", U32), ("device", U32), ("reserved", U32)]


class MultiBatch(C.Structure):
    """struct fsm_hip_multi_batch"""
    _fields_ = [("base", P), ("off", P), ("n", S), ("end_out", P), ("accept_bitmap", P)]


class MultiBatchIds(C.Structure):
    """struct fsm_hip_multi_batch_ids"""
    _fields_ = MultiBatch._fields_ + [("id_out", P)]


class MultiBatchEager(C.Structure):
    """struct fsm_hip_multi_batch_eager"""
    _fields_ = MultiBatchIds._fields_ + [("eager_out", P)]


class NodeBatch(C.Structure):
    """struct fsm_hip_node_batch: per-device lists of device pointers"""
    _fields_ = [("d_base", PP), ("stride", S), ("d_len", PP), ("d_off", PP), ("d_end_out", PP), ("d_id_out", PP), ("ids_mode", I),
                ("d_eager_out", PP), ("d_bitmap_all", PP), ("want_count", I)]


class PosBatch(C.Structure):
    """struct fsm_hip_pos_batch"""
    _fields_ = [("base", P), ("off", P), ("n", S), ("pick", P), ("m", S), ("from_", P), ("to", P), ("trim_byte", I), ("flags", U),
                ("first_out", P), ("last_out", P), ("limit", U64)]


class TokBatch(C.Structure):
    """struct fsm_hip_tok_batch"""
    _fields_ = [("base", P), ("off", P), ("n", S), ("pick", P), ("m", S), ("trim_byte", I), ("flags", U), ("limit", U64)]


class MatchBatch(C.Structure):
    """struct fsm_hip_match_batch"""
    _fields_ = [("base", P), ("off", P), ("n", S), ("pick", P), ("m", S), ("trim_byte", I), ("flags", U), ("limit", U64)]


# ---- the ABI: every function the two headers declare, fsm_hip_<name>: (restype, argtypes) ------------------------------------
# P: any pointer (handles, FILE *, struct fsm *, host and device arrays, structs by address); STR: a const char * that is
# decoded; DESC: a returned description, read through .contents; S size_t, U unsigned, U32 / U64 uintN_t, I int, D double.
# One line per family of like-signed functions; the parameter names are in the headers.
DESC = C.POINTER(_Desc)
PROTOTYPES = {"fsm_hip_" + name: (restype, args) for restype, names, *args in (
    # a DFA on the device and its batch walks: rows (data, stride, len, n), packed (base, u64 off | u32 off | len, n); _device: + stream
    (P, "dfa_create", P, U),
    (None, "dfa_free", P),
    (I, "dfa_info", P, P),
    (I, "reserve", P, S),
    (I, "exec_batch exec_batch_resume exec_batch_eager", P, P, S, P, S, P, P),
    (I, "exec_batch_device exec_batch_eager_device", P, P, S, P, S, P, P, P),
    (I, "exec_batch_offsets exec_batch_offsets32 exec_batch_lengths exec_batch_resume_offsets exec_batch_eager_offsets", P, P, P, S, P, P),
    (I, "exec_batch_offsets_device exec_batch_offsets32_device exec_batch_lengths_device exec_batch_eager_offsets_device", P, P, P, S, P, P, P),
    (I, "exec_batch_all_device", P, P, S, P, P, S, P, P, I, P, P, P),
    (I, "exec_batch_packed_all", P, P, I, P, S, P, P, I, P, P),
    (I, "exec_batch_packed_all_device", P, P, I, P, S, P, P, I, P, P, P),
    (I, "exec_batch_resume_device", P, P, S, P, S, P, P, P, P),
    (I, "exec_batch_resume_offsets_device", P, P, P, S, P, P, P, P),
    (I, "exec_batch_resume_packed", P, P, I, P, S, P, P),
    (I, "exec_batch_resume_packed_device", P, P, I, P, S, P, P, P, P),
    (I, "exec_batch_ids", P, P, S, P, S, I, P),
    (I, "exec_batch_ids_device", P, P, S, P, S, I, P, P),
    (I, "exec_batch_ids_offsets", P, P, P, S, I, P),
    (I, "exec_batch_ids_offsets_device", P, P, P, S, I, P, P),
    (I, "exec_batch_eager_resume", P, P, S, P, P, S, P, P, P),
    (I, "exec_batch_eager_resume_device", P, P, S, P, P, S, P, P, P, P),
    (I, "exec_batch_eager_trace", P, P, S, P, P, S, S, P, P, P, P),
    (I, "exec_batch_eager_trace_device", P, P, S, P, P, S, S, P, P, P, P, P),
    (D, "last_kernel_ms", P),
    (STR, "last_kernel_name", P),
    (S, "endid_count", P, U32),
    (I, "endid_get", P, U32, S, P),
    (S, "ret_count eager_id_count eager_words", P),
    (I, "ret_get", P, U32, P, P),
    (U32, "eager_id", P, U),
    (I, "ids_conflict", P, P),
    (I, "state_is_absorbing", P, U32),
    # libfsm's side: struct fsm * in, fsm_exec's and fsm_print's shapes, one input by the whole device, descriptions on disk
    (P, "compile", P, U),
    (I, "exec", P, P, P, P, P),
    (I, "match_buffer", P, P, S),
    (I, "match_file", P, P),
    (I, "match_buffer_big", P, P, S, P),
    (I, "match_buffer_big_eager", P, P, S, P, P),
    (I, "match_file_eager", P, P, P, P),
    (None, "match_last_passes", P, P),
    (DESC, "flatten desc_read", P),
    (None, "desc_free", P),
    (I, "desc_write print", P, P),
    (DESC, "desc_identity_byte", P, I),
    # many DFAs in one submission: (dfas, batches, k[, ids_mode][, stream | out])
    (I, "exec_multi node_exec_multi", P, P, S),
    (I, "exec_multi_device", P, P, S, P),
    (I, "exec_multi_ids exec_multi_eager", P, P, S, I),
    (I, "exec_multi_ids_device exec_multi_eager_device multi_prepare multi_prepare_eager", P, P, S, I, P),
    (I, "multi_launch", P, P),
    (None, "multi_prepared_free", P),
    (U, "multi_last_launches multi_last_fused_jobs"),
    (I, "multi_assign", P, S, I, P),
    # one replica per device
    (P, "node_create node_compile", P, U, P, I),
    (None, "node_free", P),
    (I, "node_ndev node_uses_rccl", P),
    (P, "node_dfa", P, I),
    (None, "node_shard", P, S, I, P, P),
    (STR, "node_rccl_path"),
    (I, "node_exec_batch node_exec_batch_eager", P, P, S, P, S, P, P),
    (I, "node_exec_batch_offsets node_exec_batch_offsets32 node_exec_batch_lengths", P, P, P, S, P, P),
    (S, "node_bitmap_words", P, S),
    (I, "node_exec_batch_device", P, P, S, S, P, P, P),
    (I, "node_exec_device", P, P, S, P, I),
    (I, "node_wait", P, P),
    (I, "node_exec_batch_ids", P, P, S, P, S, I, P),
    # the text front: lines, hits, files, context
    (P, "lines_dfa_create lines_compile", P, I, U),
    (P, "lines_dfa_inner", P),
    (I, "lines_dfa_delim", P),
    (None, "lines_dfa_free text_free text_hits_free", P),
    (P, "text_open", P, S, I),
    (P, "text_open_device", P, S, I, P),
    (P, "text_open_files", P, S, I, P, S),
    (P, "text_open_files_device", P, S, I, P, S, P),
    (S, "text_lines text_files text_hits_count text_hits_nbytes text_hits_core_count text_hits_groups", P),
    (P, "text_offsets_device text_file_lines_device text_hits_lines_device text_hits_offsets_device text_hits_bytes_device "
        "text_hits_file_first_device text_hits_core_device text_hits_group_device", P),
    (I, "text_offsets text_file_lines text_hits_file_first", P, P),
    (D, "text_scan_ms text_files_ms text_hits_ms text_hits_gather_ms text_hits_file_first_ms text_hits_context_ms", P),
    (S, "text_block_bytes text_max_workgroups text_hits_block_lines text_hits_block_bytes text_files_block text_context_scan_block"),
    (I, "text_exec", P, P, P, P, I, P, P),
    (I, "text_exec_device", P, P, P, P, I, P, P, P),
    (P, "text_hits", P, P, U),
    (P, "text_hits_device", P, P, U, P),
    (P, "text_hits_context", P, P, U, U64, U64),
    (P, "text_hits_context_device", P, P, U, U64, U64, P),
    (I, "text_hits_copy", P, P, P, P),
    (I, "text_hits_marks", P, P, P),
    # match positions and spans
    (P, "pos_dfa_create", P),
    (None, "pos_dfa_free text_spans_free", P),
    (I, "pos_dfa_in_lds text_spans_next", P),
    (I, "exec_accept_pos", P, P),
    (I, "exec_accept_pos_device", P, P, P),
    (P, "text_hits_spans", P, P, P, P, P),
    (S, "text_spans_count", P),
    (P, "text_spans_start_device text_spans_end_device", P),
    (I, "text_spans_copy", P, P, P),
    (D, "text_spans_ms", P),
    # tokens
    (P, "tok_dfa_create", P, I),
    (None, "tok_dfa_free tokens_free", P),
    (I, "tok_dfa_in_lds", P),
    (P, "tokens_run", P, P),
    (P, "tokens_run_device", P, P, P),
    (P, "text_tokens", P, P, P, U, P),
    (S, "tokens_count tokens_total", P),
    (P, "tokens_off_device tokens_end_device tokens_id_device tokens_err_device", P),
    (I, "tokens_copy", P, P, P, P, P),
    (D, "tokens_ms", P),
    (D, "tokens_pass_ms", P, I),
    # matches
    (P, "matches_run", P, P, P),
    (P, "matches_run_device", P, P, P, P),
    (P, "text_matches", P, P, P, P, U, P),
    (None, "matches_free", P),
    (S, "matches_count matches_total", P),
    (P, "matches_off_device matches_start_device matches_end_device matches_id_device", P),
    (I, "matches_copy", P, P, P, P, P),
    (D, "matches_ms", P),
    (D, "matches_pass_ms", P, I),
    # replace
    (P, "repl_create", P, P, S, U),
    (P, "repl_create_template", P, P, S, P, P, U),
    (S, "repl_inserts", P),
    (S, "repl_max_inserts"),
    (None, "repl_free replaced_free", P),
    (I, "repl_in_lds", P),
    (S, "repl_lds_bytes repl_lds_rules replaced_block_lines replaced_block_bytes"),
    (P, "matches_replace", P, P, P),
    (P, "matches_replace_device", P, P, P, P),
    (P, "text_replace", P, P, P, P, P),
    (S, "replaced_count", P),
    (U64, "replaced_nbytes", P),
    (P, "replaced_off_device replaced_bytes_device", P),
    (I, "replaced_copy", P, P, P),
    (D, "replaced_ms", P),
    (D, "replaced_pass_ms", P, I),
    # extract
    (P, "rules_create", P, S, U),
    (None, "rules_free extracted_free", P),
    (S, "extracted_block_matches extracted_block_bytes"),
    (P, "matches_extract", P, P, P, I),
    (P, "matches_extract_device", P, P, P, I, P),
    (P, "text_extract", P, P, P, P, I, P),
    (S, "extracted_count", P),
    (U64, "extracted_nbytes", P),
    (P, "extracted_off_device extracted_bytes_device extracted_line_device extracted_match_device", P),
    (I, "extracted_copy", P, P, P, P, P),
    (D, "extracted_ms", P),
    (D, "extracted_pass_ms", P, I),
    # tally: (object | off, id, m, total), (group_off, ngroups | text, hits), nrules, flags, count, lines[, stream]
    (I, "tally_ids_device", P, P, S, S, P, S, S, U, P, P, P),
    (I, "matches_tally_device tokens_tally_device", P, P, S, S, U, P, P, P),
    (I, "matches_tally tokens_tally", P, P, S, S, U, P, P),
    (I, "text_matches_tally text_tokens_tally", P, P, P, S, U, P, P, P),
    (S, "tally_span_inputs tally_window tally_lds_columns tally_max_line_columns"),
    # distinct: (off, bytes, R[, nbytes], trim, tag | object), sep, flags[, stream]
    (P, "distinct_device", P, P, S, U64, I, P, I, U, P),
    (P, "distinct", P, P, S, I, P, I, U),
    (P, "extracted_distinct text_hits_distinct", P, I, U, P),
    (S, "distinct_count distinct_records", P),
    (U64, "distinct_nbytes", P),
    (P, "distinct_first_device distinct_count_device distinct_class_device distinct_off_device distinct_bytes_device", P),
    (I, "distinct_copy", P, P, P, P, P, P),
    (D, "distinct_ms", P),
    (D, "distinct_pass_ms", P, I),
    (S, "distinct_long_bytes"),
    (S, "distinct_table_slots", S),
    (None, "distinct_free", P),
    # sort: (off, bytes, R[, nbytes], trim, major | object), sep, flags[, stream]
    (P, "sort_device", P, P, S, U64, I, P, I, U, P),
    (P, "sort", P, P, S, I, P, I, U),
    (P, "extracted_sort text_hits_sort keys_sort", P, I, U, P),
    (S, "sorted_records sorted_groups sorted_rounds", P),
    (S, "sorted_radix_passes", P, I),
    (U64, "sorted_nbytes", P),
    (P, "sorted_order_device sorted_rank_device sorted_off_device sorted_bytes_device", P),
    (I, "sorted_copy", P, P, P, P, P),
    (D, "sorted_ms", P),
    (D, "sorted_pass_ms", P, I),
    (S, "sort_tile_records"),
    (None, "sorted_free", P),
    # find: keys, (off, bytes, R[, nbytes], trim, tag | object), flags[, stream]
    (P, "keys_find_device", P, P, P, S, U64, I, P, U, P),
    (P, "keys_find", P, P, P, S, I, P, U),
    (P, "keys_find_extracted keys_find_hits keys_find_text", P, P, U, P),
    (S, "found_records found_present", P),
    (P, "found_class_device found_bitmap_device found_pick_device", P),
    (I, "found_copy", P, P, P, P),
    (D, "found_ms", P),
    (D, "found_pass_ms", P, I),
    (None, "found_free", P),
    # input generators: (out, stride, n, first_index, seed, {bytes, count}..., every[, stream])
    (I, "gen_inputs_device", P, S, S, U64, U64, P, U, P, U, U, P),
    (None, "gen_inputs_host", P, S, S, U64, U64, P, U, P, U, U),
    (I, "gen_pack_rows_device", P, S, P, P, S, S, P, P),
    (I, "gen_affix_inputs_device", P, S, S, U64, U64, P, U, P, U, P, U, P, U, U, P),
    (None, "gen_affix_inputs_host", P, S, S, U64, U64, P, U, P, U, P, U, P, U, U),
    (I, "gen_affix2_inputs_device", P, S, S, U64, U64, P, U, P, U, P, U, P, U, P, U, U, P),
    (None, "gen_affix2_inputs_host", P, S, S, U64, U64, P, U, P, U, P, U, P, U, P, U, U),
    # literal sets
    (P, "strings_new"),
    (None, "strings_free", P),
    (I, "strings_add_raw", P, P, S, P),
    (I, "strings_add_str", P, P, P),
    (DESC, "strings_build", P, U),
    (DESC, "strings", P, S, U),
    # include/fsm_hip_plan.h: version, knobs, the host-side plan, probes
    (I, "version"),
    (I, "dfa_tune", P, I, I),
    (P, "plan_create", P, U, U32),
    (None, "plan_free", P),
    (I, "plan_get", P, I, P, P),
    (D, "stream_read_probe_ms", P, S, P, I, P),
    (D, "gather_probe_ms", P, S, S, I, P, P),
    (D, "lds_chain_probe_gbps", S, I, I, S, P, P),
    (I, "waves_by_occupancy", I, I, I),
) for name in names.split()}

_lib = None
_libc = C.CDLL(None, use_errno=True)
_libc.fopen.restype, _libc.fopen.argtypes, _libc.fclose.argtypes = P, [STR, STR], [P]


def load_library(path: Optional[str] = None) -> C.CDLL:
    """Load libfsm_hip.so (built in-tree by __graft_entry__.build()) with PROTOTYPES applied."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise RuntimeError(f"libfsm_hip.so not built at {p}: run `python __graft_entry__.py` (no CPU fallback exists)")
    lib = C.CDLL(p, mode=C.RTLD_GLOBAL, use_errno=True)
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    if path is None:
        _lib = lib
    return lib


def _line_arrays(base, off, pick):
    """the host arrays of a batch of lines as the library takes them -> (base u8, off u64 [n + 1], pick u64 [m] or None, n, m)"""
    base = np.ascontiguousarray(base, np.uint8)
    off = np.ascontiguousarray(off, np.uint64)
    pick = None if pick is None else np.ascontiguousarray(pick, np.uint64)
    n = len(off) - 1
    m = n if pick is None else len(pick)
    if pick is not None and m == 0:
        pick = np.zeros(1, np.uint64)   # an empty pick is still a pick: a non-NULL address
    return base, off, pick, n, m


def _oserr(what: str):
    e = C.get_errno()
    return OSError(e, f"{what}: {os.strerror(e)}")


def _call(name: str, *args, negative_only: bool = False):
    """Clear errno, call the library's `name`, raise its errno as OSError(name) on failure: a non-zero int (negative_only: a
    negative one, for the functions that answer 0 / 1), or NULL from a function that returns a pointer.  Returns the result."""
    C.set_errno(0)
    r = getattr(load_library(), name)(*args)
    if (not r) if PROTOTYPES[name][0] is not I else (r < 0 if negative_only else r != 0):
        raise _oserr(name)
    return r


def _ptr(a: Optional[np.ndarray]):
    """the array's address as a pointer object that keeps the array alive (_affix_args hands such pointers on without the arrays)"""
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _ptr0(a: Optional[np.ndarray]):
    """NULL for an empty array too"""
    return _ptr(a) if a is not None and a.size else None


def _host_batch(struct, base, off, pick, *tail):
    """a line batch (TokBatch, MatchBatch) over host arrays -> (the struct, the arrays it points into: held until the call is
    over); tail: the fields behind m"""
    base, off, pick, n, m = _line_arrays(base, off, pick)
    return struct(_ptr0(base), _ptr(off), n, _ptr(pick), m, *tail), (base, off, pick)


def _device_batch(struct, d_base: int, d_off: int, n: int, d_pick: int, m: int, *tail):
    """a line batch (PosBatch, TokBatch, MatchBatch) over device addresses, 0: NULL; tail: the fields behind m"""
    return struct(d_base or None, d_off or None, n, d_pick or None, m, *tail)


class _Owned:
    """One handle of the library and what has to outlive it.  _FREE names the function that frees the handle; close() calls
    it once, on a half-built object and on a second call it does nothing; dropping the last reference closes."""

    _FREE = None

    def __init__(self, handle, keep=()):
        self._lib = load_library()
        self._h, self._keep = handle, keep

    def close(self):
        if getattr(self, "_h", None):
            getattr(self._lib, self._FREE)(self._h)
        self._h = self._keep = None

    def __del__(self):
        self.close()      # (not an alias: a subclass's close is the one that runs)

    @property
    def handle(self):
        return self._h


class _Freed(_Owned):
    """an _Owned whose close() is spelt free() as well, as the library spells it: the objects the matches family hands out.  (Not
    in _Owned: tests/test_gpu_round5.py lists every public method of HipNode.)"""

    def free(self):
        self.close()


def _dev(fn: str):
    """a property of an _Owned: the device address the library's `fn` answers for the handle, 0 for NULL"""
    return property(lambda self: int(getattr(self._lib, fn)(self._h) or 0))


def _size(fn: str, doc: Optional[str] = None):
    """a property of an _Owned: the size_t (or uint64_t) the library's `fn` answers for the handle"""
    return property(lambda self: int(getattr(self._lib, fn)(self._h)), doc=doc)


@contextmanager
def _fopen(path: str, mode: bytes):
    """a FILE * of the C library, closed on the way out"""
    f = _libc.fopen(path.encode(), mode)
    if not f:
        raise OSError(C.get_errno(), "fopen")
    try:
        yield f
    finally:
        _libc.fclose(f)


def _pack_strings(strings: Sequence[bytes], pad: bytes = b""):
    """strings -> (base u8, off u64 [n + 1]); pad: what an empty base holds instead, for the callers that pass its address"""
    off = np.zeros(len(strings) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in strings])
    return np.frombuffer(b"".join(strings) or pad, dtype=np.uint8), off


def _outputs(n: int, want_end: bool = True, want_bitmap: bool = True, fill: Optional[int] = None):
    """(end u32 [n], accept bitmap u64 [ceil(n / 64)], zeroed), None for the one not asked for; fill: what end holds before the call"""
    end = None if not want_end else np.empty(n, np.uint32) if fill is None else np.full(n, fill, np.uint32)
    return end, np.zeros((n + 63) // 64, np.uint64) if want_bitmap else None


def _inputs(data, lens=None, off=None):
    """a batch as the fronts take it -> (data u8, lens u32 or None, off u64 or None, n, stride): [n][stride] rows (+ lens), or
    with off (n + 1 offsets) the packed bytes, stride 0"""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    if lens is not None:
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
    if off is None:
        return (data, lens, None) + data.shape
    off = np.ascontiguousarray(off, dtype=np.uint64)
    return data, lens, off, len(off) - 1, 0


# ---- the host fronts HipDfa and HipNode share: fn names the entry point, h is the handle ------------------------------------

def _exec_rows(fn, h, data, lens, want_bitmap=True):
    """(end u32 [n], bitmap u64 [ceil(n / 64)] or None) of [n][stride] rows"""
    data, lens, _, n, stride = _inputs(data, lens)
    end, bm = _outputs(n, True, want_bitmap)
    _call(fn, h, _ptr(data), stride, _ptr(lens), n, _ptr(end), _ptr(bm))
    return end, bm


def _exec_packed(fn, h, base, meta, dtype, want_bitmap=True, want_end=True):
    """(end or None, bitmap or None) of packed inputs; meta: n + 1 offsets, or (u32, a *_lengths front) n lengths"""
    base = np.ascontiguousarray(base, dtype=np.uint8)
    meta = np.ascontiguousarray(meta, dtype=dtype)
    n = len(meta) - (0 if fn.endswith("_lengths") else 1)
    end, bm = _outputs(n, want_end, want_bitmap)
    _call(fn, h, _ptr0(base), _ptr0(meta), n, _ptr(end), _ptr(bm))
    return end, bm


def _exec_rows_ids(fn, h, data, mode, lens):
    data, lens, _, n, stride = _inputs(data, lens)
    out = np.empty(n, dtype=np.uint32)
    _call(fn, h, _ptr(data), stride, _ptr(lens), n, mode, _ptr(out))
    return out


@dataclass
class FlatDfa:
    """Flat DFA description = struct fsm_hip_dfa_desc (include/fsm_hip.h)."""

    nstates: int
    start: int
    edge_off: np.ndarray  # u32 [nstates+1]
    ranges: np.ndarray  # RANGE_DTYPE [nranges]
    is_end: np.ndarray  # u8 [nstates]
    endid_off: np.ndarray  # u32 [nstates+1]
    endids: np.ndarray  # u32 []
    eager_off: Optional[np.ndarray] = None  # u32 [nstates+1] or None (no eager outputs)
    eager_ids: Optional[np.ndarray] = None  # u32 []

    def __post_init__(self):
        if self.eager_off is not None:
            self.eager_off = np.ascontiguousarray(self.eager_off, dtype=np.uint32)
            self.eager_ids = np.ascontiguousarray(self.eager_ids if self.eager_ids is not None else [], dtype=np.uint32)
            if int(self.eager_off[-1]) == 0:
                self.eager_off = self.eager_ids = None
        self.edge_off = np.ascontiguousarray(self.edge_off, dtype=np.uint32)
        self.ranges = np.ascontiguousarray(self.ranges, dtype=RANGE_DTYPE)
        self.is_end = np.ascontiguousarray(self.is_end, dtype=np.uint8)
        self.endid_off = np.ascontiguousarray(self.endid_off, dtype=np.uint32)
        self.endids = np.ascontiguousarray(self.endids, dtype=np.uint32)

    def desc(self) -> _Desc:
        d = _Desc()
        d.nstates, d.start = self.nstates, self.start
        d.edge_off = self.edge_off.ctypes.data
        d.ranges = self.ranges.ctypes.data if len(self.ranges) else None
        d.is_end = self.is_end.ctypes.data
        d.endid_off = self.endid_off.ctypes.data
        d.endids = self.endids.ctypes.data if len(self.endids) else None
        d.eager_off = self.eager_off.ctypes.data if self.eager_off is not None else None
        d.eager_ids = self.eager_ids.ctypes.data if self.eager_off is not None and len(self.eager_ids) else None
        return d

    @classmethod
    def from_desc(cls, d: _Desc) -> "FlatDfa":
        n = d.nstates

        def arr(addr, count, dt):
            if count == 0 or not addr:
                return np.zeros(0, dtype=dt)
            buf = (C.c_char * (count * np.dtype(dt).itemsize)).from_address(addr)
            return np.frombuffer(buf, dtype=dt).copy()

        edge_off = arr(d.edge_off, n + 1, np.uint32)
        endid_off = arr(d.endid_off, n + 1, np.uint32) if d.endid_off else np.zeros(n + 1, np.uint32)
        eo = arr(d.eager_off, n + 1, np.uint32) if d.eager_off else None
        return cls(n, d.start, edge_off, arr(d.ranges, int(edge_off[n]), RANGE_DTYPE), arr(d.is_end, n, np.uint8),
                   endid_off, arr(d.endids, int(endid_off[n]), np.uint32),
                   eo, arr(d.eager_ids, int(eo[n]), np.uint32) if eo is not None else None)

    @classmethod
    def from_dense(cls, next_tab: np.ndarray, start: int, is_end: Sequence[int], endids=None, eager_off=None, eager_ids=None) -> "FlatDfa":
        """next_tab: [S][256] int64/uint32, negative or 0xFFFFFFFF = no edge.  eager_off (u32 [S + 1], CSR) / eager_ids: the
        eager outputs of every state (the ids of state s are eager_ids[eager_off[s]:eager_off[s + 1]]), or None."""
        nt = np.asarray(next_tab, dtype=np.int64)
        S = nt.shape[0]
        rng, off = [], [0]
        for s in range(S):
            c = 0
            row = nt[s]
            while c < 256:
                t = row[c]
                if t < 0 or t == NO_MATCH:
                    c += 1
                    continue
                lo = c
                while c + 1 < 256 and row[c + 1] == t:
                    c += 1
                rng.append((lo, c, 0, int(t)))
                c += 1
            off.append(len(rng))
        eo, ei = [0], []
        for s in range(S):
            if endids is not None and s in endids:
                ei.extend(sorted(set(endids[s])))
            eo.append(len(ei))
        if eager_off is not None and len(eager_off) != S + 1:
            raise ValueError("eager_off needs nstates + 1 entries")
        return cls(S, start, np.array(off, np.uint32), np.array(rng, dtype=RANGE_DTYPE) if rng else np.zeros(0, RANGE_DTYPE),
                   np.asarray(is_end, np.uint8), np.array(eo, np.uint32), np.array(ei, np.uint32), eager_off, eager_ids)

    def dense(self) -> np.ndarray:
        """[S][256] uint32 next table, NO_MATCH = no edge."""
        t = np.full((self.nstates, 256), NO_MATCH, dtype=np.uint32)
        for s in range(self.nstates):
            for k in range(int(self.edge_off[s]), int(self.edge_off[s + 1])):
                r = self.ranges[k]
                t[s, int(r["lo"]):int(r["hi"]) + 1] = r["to"]
        return t

    def endids_of(self, state: int) -> np.ndarray:
        return self.endids[int(self.endid_off[state]):int(self.endid_off[state + 1])]

    def write_c(self, path: str):
        """fsm_hip_desc_write(): the library's own on-disk form ("FSMHIP01")."""
        d = self.desc()
        with _fopen(path, b"wb") as f:
            _call("fsm_hip_desc_write", C.byref(d), f)

    @classmethod
    def _take(cls, d) -> "FlatDfa":
        """a copy of a description the library returned, which is freed"""
        try:
            return cls.from_desc(d.contents)
        finally:
            load_library().fsm_hip_desc_free(d)

    @classmethod
    def read_c(cls, path: str) -> "FlatDfa":
        with _fopen(path, b"rb") as f:
            return cls._take(_call("fsm_hip_desc_read", f))

    @classmethod
    def from_strings(cls, words: Sequence[bytes], flags: int = 0, endids: Optional[Sequence[int]] = None) -> "FlatDfa":
        """fsm_hip_strings_*(): literal set -> DFA, the automaton libre's re_strings builds
        (flags: 1 anchor left, 2 anchor right, 4 AC automaton; endids: one per word or None)."""
        lib = load_library()
        g = _call("fsm_hip_strings_new")
        try:
            for i, w in enumerate(words):
                if not lib.fsm_hip_strings_add_raw(g, w, len(w), C.byref(C.c_uint32(int(endids[i]))) if endids is not None else None):
                    raise _oserr("fsm_hip_strings_add_raw")
            return cls._take(_call("fsm_hip_strings_build", g, flags))
        finally:
            lib.fsm_hip_strings_free(g)

    def canonical(self):
        """(nstates, start, dense [S][256] next table with 0xFFFFFFFF = no edge, is_end, end-id lists): order-free form."""
        nt = np.full((self.nstates, 256), NO_MATCH, np.uint32)
        for s_ in range(self.nstates):
            for r in self.ranges[int(self.edge_off[s_]):int(self.edge_off[s_ + 1])]:
                nt[s_, int(r["lo"]):int(r["hi"]) + 1] = r["to"]
        return self.nstates, self.start, nt, self.is_end.copy(), self.endid_off.copy(), self.endids.copy()

    def save(self, path: str, **extra):
        np.savez_compressed(path, nstates=np.uint32(self.nstates), start=np.uint32(self.start), edge_off=self.edge_off,
                            r_lo=self.ranges["lo"], r_hi=self.ranges["hi"], r_to=self.ranges["to"], is_end=self.is_end,
                            endid_off=self.endid_off, endids=self.endids,
                            **({"eager_off": self.eager_off, "eager_ids": self.eager_ids} if self.eager_off is not None else {}), **extra)

    @classmethod
    def load(cls, path_or_npz) -> "FlatDfa":
        z = np.load(path_or_npz) if isinstance(path_or_npz, (str, os.PathLike)) else path_or_npz
        r = np.zeros(len(z["r_lo"]), dtype=RANGE_DTYPE)
        r["lo"], r["hi"], r["to"] = z["r_lo"], z["r_hi"], z["r_to"]
        return cls(int(z["nstates"]), int(z["start"]), z["edge_off"], r, z["is_end"], z["endid_off"], z["endids"],
                   z["eager_off"] if "eager_off" in z else None, z["eager_ids"] if "eager_ids" in z else None)

    def eager_of(self, state: int) -> np.ndarray:
        if self.eager_off is None:
            return np.zeros(0, np.uint32)
        return self.eager_ids[int(self.eager_off[state]):int(self.eager_off[state + 1])]


class Plan(_Owned):
    """Host-side table plan (fsm_hip_plan_*): inspection only, never executes inputs."""

    _FREE = "fsm_hip_plan_free"

    _WHAT = dict(scalars=(0, np.uint32), cls=(1, np.uint8), new2old=(2, np.uint32), fin=(3, np.uint32),
                 dense=(4, np.uint32), tiny_col=(5, np.uint64), lds_tab=(6, np.uint16), comb=(7, np.uint32),
                 comb_dflt=(8, np.uint32), comb_off=(9, np.uint32), comb_fin=(10, np.uint32), glob_tab=(11, np.uint32),
                 comb256=(12, np.uint32), comb256_off=(13, np.uint32), comb256_fin=(14, np.uint32), comb_smask=(15, np.uint32),
                 emask=(16, np.uint64), eager_ids=(17, np.uint32), sparse=(18, np.uint32),
                 ew_off=(19, np.uint32), ew_word=(20, np.uint32), ew_mask=(21, np.uint64), tiny5_col=(22, np.uint32),
                 comb_rng=(23, np.uint16), lazy=(24, np.uint32), glob_tab16=(25, np.uint16), glob16_rank=(26, np.uint32), glob16_fin=(27, np.uint32))

    def __init__(self, flat: FlatDfa, flags: int = 0, lds_limit: int = 0):
        d = flat.desc()
        super().__init__(_call("fsm_hip_plan_create", C.byref(d), flags, lds_limit))
        s = self.get("scalars")
        (self.nstates, self.S1, self.start, self.C, self.abs_min, self.nabsorbing, self.layout, self.row_bytes,
         self.comb_abs_min_off, self.comb256_abs_min_off, self.comb256_dflt, self.eager_lo_end,
         self.eager_hi_begin, self.comb_eager_lo_off, self.comb_eager_hi_off, self.comb256_eager_lo_off,
         self.comb256_eager_hi_off) = (int(x) for x in s)

    def get(self, what: str) -> np.ndarray:
        w, dt = self._WHAT[what]
        p, n = C.c_void_p(), C.c_size_t()
        _call("fsm_hip_plan_get", self._h, w, C.byref(p), C.byref(n))
        if n.value == 0:
            return np.zeros(0, dt)
        buf = (C.c_char * (n.value * np.dtype(dt).itemsize)).from_address(p.value)
        return np.frombuffer(buf, dtype=dt).copy()


class HipDfa(_Owned):
    """struct fsm_hip_dfa *: a DFA resident on the GPU."""

    _FREE = "fsm_hip_dfa_free"

    def __init__(self, flat: Optional[FlatDfa] = None, flags: int = 0, *, handle=None, borrowed: bool = False):
        self._borrowed = borrowed      # a replica owned by a HipNode: never freed from here
        if handle is None:
            d = flat.desc()
            handle = _call("fsm_hip_dfa_create", C.byref(d), flags)
        super().__init__(handle)

    @classmethod
    def compile_fsm(cls, fsm_ptr: int, flags: int = 0) -> "HipDfa":
        """fsm_hip_compile(const struct fsm *): libfsm must already be loaded RTLD_GLOBAL."""
        return cls(handle=_call("fsm_hip_compile", fsm_ptr, flags))

    def close(self):
        if getattr(self, "_borrowed", False):
            self._h = None
        super().close()

    def info(self) -> dict:
        i = _Info()
        _call("fsm_hip_dfa_info", self._h, C.byref(i))
        d = {k: getattr(i, k) for k, _ in _Info._fields_ if k != "reserved"}
        d["layout_name"] = LAYOUT_NAMES.get(i.layout, "?")
        return d

    def tune(self, knob: int, value: int):
        _call("fsm_hip_dfa_tune", self._h, knob, value)

    # ---- host-buffer fronts -------------------------------------------------
    def exec_batch(self, data: np.ndarray, lens: Optional[np.ndarray] = None, want_bitmap: bool = True):
        """data: uint8 [n, stride]; returns (end u32[n], bitmap u64[ceil(n/64)])."""
        return _exec_rows("fsm_hip_exec_batch", self._h, data, lens, want_bitmap)

    def exec_batch_offsets(self, base: np.ndarray, off: np.ndarray, want_bitmap: bool = True):
        return _exec_packed("fsm_hip_exec_batch_offsets", self._h, base, off, np.uint64, want_bitmap)

    def exec_batch_offsets32(self, base: np.ndarray, off32: np.ndarray, want_bitmap: bool = True, want_end: bool = True):
        """fsm_hip_exec_batch_offsets32: u32 offsets (batches below 4 GiB)."""
        return _exec_packed("fsm_hip_exec_batch_offsets32", self._h, base, off32, np.uint32, want_bitmap, want_end)

    def exec_batch_lengths(self, base: np.ndarray, lens: np.ndarray, want_bitmap: bool = True, want_end: bool = True):
        """fsm_hip_exec_batch_lengths: inputs packed back to back, their lengths and nothing else."""
        return _exec_packed("fsm_hip_exec_batch_lengths", self._h, base, lens, np.uint32, want_bitmap, want_end)

    def exec_batch_offsets32_device(self, d_base: int, d_off32: int, n: int, d_end: int = 0, d_bitmap: int = 0, stream: int = 0):
        _call("fsm_hip_exec_batch_offsets32_device", self._h, d_base, d_off32, n, d_end or None, d_bitmap or None, stream or None)

    def exec_batch_lengths_device(self, d_base: int, d_len: int, n: int, d_end: int = 0, d_bitmap: int = 0, stream: int = 0):
        _call("fsm_hip_exec_batch_lengths_device", self._h, d_base, d_len, n, d_end or None, d_bitmap or None, stream or None)

    def exec_strings(self, strings: Sequence[bytes]):
        return self.exec_batch_offsets(*_pack_strings(strings))

    def match_buffer(self, s: bytes) -> int:
        return _call("fsm_hip_match_buffer", self._h, s, len(s), negative_only=True)

    # ---- device-pointer front (raw addresses, e.g. torch tensors' data_ptr()) ----
    def exec_batch_device(self, d_base: int, stride: int, n: int, d_end: int = 0, d_bitmap: int = 0, d_len: int = 0, stream: int = 0):
        _call("fsm_hip_exec_batch_device", self._h, d_base, stride, d_len or None, n, d_end or None, d_bitmap or None, stream or None)

    def last_kernel_name(self) -> str:
        return (self._lib.fsm_hip_last_kernel_name(self._h) or b"").decode()

    def exec_batch_eager_device(self, d_base: int, stride: int, n: int, d_end: int, d_sets: int, d_len: int = 0, stream: int = 0):
        """d_sets: n * eager_words() u64 on the device."""
        _call("fsm_hip_exec_batch_eager_device", self._h, d_base, stride, d_len or None, n, d_end or None, d_sets, stream or None)

    def eager_words(self) -> int:
        return int(self._lib.fsm_hip_eager_words(self._h))

    def exec_batch_offsets_device(self, d_base: int, d_off: int, n: int, d_end: int = 0, d_bitmap: int = 0, stream: int = 0):
        _call("fsm_hip_exec_batch_offsets_device", self._h, d_base, d_off, n, d_end or None, d_bitmap or None, stream or None)

    def exec_batch_ids(self, data: np.ndarray, mode: int, lens: Optional[np.ndarray] = None) -> np.ndarray:
        """Device-side end-id delivery: mode 1 = lowest id (AMBIG_EARLIEST), 2 = index into ret sets, 3 = AMBIG_ERROR."""
        return _exec_rows_ids("fsm_hip_exec_batch_ids", self._h, data, mode, lens)

    def exec_batch_resume(self, data: np.ndarray, state_io: np.ndarray, lens: Optional[np.ndarray] = None):
        """Streaming: start row i from state_io[i] (START/DEAD/state id); returns (state_out, end)."""
        data, lens, _, n, stride = _inputs(data, lens)
        st = np.ascontiguousarray(state_io, dtype=np.uint32).copy()
        end = np.empty(n, dtype=np.uint32)
        _call("fsm_hip_exec_batch_resume", self._h, _ptr(data), stride, _ptr(lens), n, _ptr(st), _ptr(end))
        return st, end

    def exec_batch_eager(self, data: np.ndarray, lens: Optional[np.ndarray] = None):
        """Walk + eager outputs: returns (end u32[n], list of emitted-id arrays per input)."""
        data, lens, _, n, stride = _inputs(data, lens)
        end, eo = np.empty(n, dtype=np.uint32), np.zeros((n, self.eager_words()), dtype=np.uint64)
        _call("fsm_hip_exec_batch_eager", self._h, _ptr(data), stride, _ptr(lens), n, _ptr(end), _ptr(eo))
        return end, self._decode(eo)

    def exec_eager_words(self, data: np.ndarray, lens: Optional[np.ndarray] = None, off: Optional[np.ndarray] = None, want_end: bool = True,
                         eager_out: Optional[np.ndarray] = None, null_sets: bool = False):
        """fsm_hip_exec_batch_eager (data: [n][stride] rows, + lens) or, with off (n + 1 u64 offsets), fsm_hip_exec_batch_eager_offsets
        (data: the packed bytes), with the sets as the library writes them: returns (end or None, u64 [n][eager_words()]).
        eager_out: the caller's own array, written in place; null_sets: NULL is passed for the sets (the fronts refuse it)."""
        data, lens, off, n, stride = _inputs(data, lens, off)
        end = np.empty(n, dtype=np.uint32) if want_end else None
        eo = None if null_sets else eager_out if eager_out is not None else np.zeros((n, self.eager_words()), dtype=np.uint64)
        if off is not None:
            _call("fsm_hip_exec_batch_eager_offsets", self._h, _ptr0(data), _ptr(off), n, _ptr(end), _ptr(eo))
        else:
            _call("fsm_hip_exec_batch_eager", self._h, _ptr0(data), stride, _ptr(lens), n, _ptr(end), _ptr(eo))
        return end, eo

    def exec_batch_eager_offsets_device(self, d_base: int, d_off: int, n: int, d_end: int, d_sets: int, stream: int = 0):
        """fsm_hip_exec_batch_eager_offsets_device; d_sets: n * eager_words() u64 on the device"""
        _call("fsm_hip_exec_batch_eager_offsets_device", self._h, d_base or None, d_off or None, n, d_end or None, d_sets or None, stream or None)

    def exec_batch_eager_trace(self, data: np.ndarray, lens: Optional[np.ndarray] = None, off: Optional[np.ndarray] = None, cap: int = 64):
        """fsm_exec's eager-output callback stream per input, order and repeats kept: (end u32[n], count u32[n],
        [(ids, positions) of the first min(count, cap) emissions]).  data: (n, stride) rows (+ lens), or a flat byte
        array with off[n + 1]."""
        data, lens, off, n, stride = _inputs(data, lens, off)
        end, cnt = np.empty(n, np.uint32), np.zeros(n, np.uint32)
        ids, pos = np.zeros((n, max(cap, 1)), np.uint32), np.zeros((n, max(cap, 1)), np.uint32)
        _call("fsm_hip_exec_batch_eager_trace", self._h, _ptr0(data), stride, _ptr(lens), _ptr(off), n, cap, _ptr(end), _ptr(cnt), _ptr(ids), _ptr(pos))
        k = np.minimum(cnt, cap)
        return end, cnt, [(ids[i, :k[i]].copy(), pos[i, :k[i]].copy()) for i in range(n)]

    def exec_batch_eager_trace_device(self, d_base: int, stride: int, n: int, cap: int, d_count: int, d_ids: int, d_pos: int = 0, d_end: int = 0,
                                      d_len: int = 0, d_off: int = 0, stream: int = 0):
        _call("fsm_hip_exec_batch_eager_trace_device", self._h, d_base or None, stride, d_len or None, d_off or None, n, cap, d_end or None,
              d_count, d_ids or None, d_pos or None, stream or None)

    def exec_packed_all_form(self, base: np.ndarray, meta_form: int, meta: np.ndarray, n: int, ids_mode: int = 0, want_end=True, want_bitmap=False,
                             want_eager=False):
        """fsm_hip_exec_batch_packed_all: returns dict(end=, bitmap=, ids=, eager=) with the outputs asked for."""
        base = np.ascontiguousarray(base, dtype=np.uint8)
        meta = np.ascontiguousarray(meta, dtype=np.uint64 if meta_form == 0 else np.uint32)
        end, bm = _outputs(n, want_end, want_bitmap)
        ids = np.empty(n, np.uint32) if ids_mode else None
        eo = np.zeros((n, self.eager_words()), np.uint64) if want_eager else None
        _call("fsm_hip_exec_batch_packed_all", self._h, _ptr0(base), meta_form, _ptr(meta), n, _ptr(end), _ptr(bm), ids_mode, _ptr(ids), _ptr(eo))
        return {"end": end, "bitmap": bm, "ids": ids, "eager": eo}

    def exec_packed_all_device(self, d_base: int, meta_form: int, d_meta: int, n: int, d_end: int = 0, d_bitmap: int = 0, ids_mode: int = 0, d_ids: int = 0,
                               d_eager: int = 0, stream: int = 0):
        _call("fsm_hip_exec_batch_packed_all_device", self._h, d_base or None, meta_form, d_meta or None, n, d_end or None, d_bitmap or None, ids_mode,
              d_ids or None, d_eager or None, stream or None)

    # ---- the same three fronts over packed inputs (base + off[n + 1]) -----------
    def exec_offsets_ids(self, base: np.ndarray, off: np.ndarray, mode: int) -> np.ndarray:
        base, _, off, n, _ = _inputs(base, None, off)
        out = np.empty(n, dtype=np.uint32)
        _call("fsm_hip_exec_batch_ids_offsets", self._h, _ptr0(base), _ptr(off), n, mode, _ptr(out))
        return out

    def _eager_ids(self) -> np.ndarray:
        """the id of every bit of a set, in bit order"""
        return np.array([self._lib.fsm_hip_eager_id(self._h, b) for b in range(self._lib.fsm_hip_eager_id_count(self._h))], np.uint32)

    def _decode(self, eo: np.ndarray) -> list:
        """u64 [n][W] sets -> per input the ids emitted, ascending"""
        ids = self._eager_ids()
        bits = np.unpackbits(eo.view(np.uint8), axis=1, bitorder="little")[:, :len(ids)].astype(bool)
        return [ids[row] for row in bits]

    def _eager_ids_of(self, words: np.ndarray) -> np.ndarray:
        """a W-word set -> the sorted ids it holds"""
        return np.sort(self._decode(np.ascontiguousarray(words, np.uint64).reshape(1, -1))[0])

    def decode_eager(self, words: np.ndarray) -> list:
        """n * eager_words() u64 as the eager fronts write them -> per input the ids emitted, ascending (what exec_batch_eager returns)"""
        return self._decode(np.ascontiguousarray(words, np.uint64).reshape(-1, self.eager_words()))

    def exec_batch_eager_resume(self, data: np.ndarray, state_io: np.ndarray, eager_io: Optional[np.ndarray], lens: Optional[np.ndarray] = None,
                                off: Optional[np.ndarray] = None, want_end: bool = True):
        """fsm_hip_exec_batch_eager_resume: one more piece of every input.  data: [n][stride] rows (+ lens), or with off (n + 1
        u64 offsets) the packed bytes.  eager_io: n * eager_words() u64 (zeroed before a stream's first piece), OR-ed into.
        Returns (state_out, end, eager_io) -- new arrays; the arguments are left as they are."""
        data, lens, off, n, stride = _inputs(data, lens, off)
        st = np.ascontiguousarray(state_io, dtype=np.uint32).copy() if state_io is not None else None
        eo = np.ascontiguousarray(eager_io, dtype=np.uint64).copy() if eager_io is not None else None   # (None: NULL, which the front refuses)
        if eo is not None and eo.size != n * self.eager_words():
            raise ValueError("eager_io needs n * eager_words() words")
        end = np.empty(n, dtype=np.uint32) if want_end else None
        _call("fsm_hip_exec_batch_eager_resume", self._h, _ptr0(data), stride, _ptr(lens), _ptr(off), n, _ptr(st), _ptr(end), _ptr(eo))
        return st, end, eo

    def exec_batch_eager_resume_device(self, d_base: int, stride: int, n: int, d_state_io: int, d_eager_io: int, d_len: int = 0, d_off: int = 0,
                                       d_end: int = 0, stream: int = 0):
        _call("fsm_hip_exec_batch_eager_resume_device", self._h, d_base or None, stride, d_len or None, d_off or None, n, d_state_io or None,
              d_end or None, d_eager_io or None, stream or None)

    def exec_offsets_resume(self, base: np.ndarray, off: np.ndarray, state_io: np.ndarray):
        base, _, off, n, _ = _inputs(base, None, off)
        st = np.ascontiguousarray(state_io, dtype=np.uint32).copy()
        end = np.empty(n, dtype=np.uint32)
        _call("fsm_hip_exec_batch_resume_offsets", self._h, _ptr0(base), _ptr(off), n, _ptr(st), _ptr(end))
        return st, end

    def exec_packed_resume(self, base: np.ndarray, meta_form: int, meta: np.ndarray, n: int, state_io: np.ndarray):
        """fsm_hip_exec_batch_resume_packed: resume over u64 offsets / u32 offsets / lengths alone; returns (state_out, end)."""
        base = np.ascontiguousarray(base, dtype=np.uint8)
        meta = np.ascontiguousarray(meta)
        st = np.ascontiguousarray(state_io, dtype=np.uint32).copy()
        end = np.empty(n, dtype=np.uint32)
        _call("fsm_hip_exec_batch_resume_packed", self._h, _ptr0(base), meta_form, _ptr0(meta), n, _ptr(st), _ptr(end))
        return st, end

    def exec_packed_resume_device(self, d_base: int, meta_form: int, d_meta: int, n: int, d_state_io: int, d_end: int = 0, d_bitmap: int = 0, stream: int = 0):
        _call("fsm_hip_exec_batch_resume_packed_device", self._h, d_base or None, meta_form, d_meta or None, n, d_state_io, d_end or None,
              d_bitmap or None, stream or None)

    def reserve(self, n: int):
        """fsm_hip_reserve: allocate now what batches of up to n inputs would allocate later (graph capture from the first launch)."""
        _call("fsm_hip_reserve", self._h, n)

    def exec_offsets_eager(self, base: np.ndarray, off: np.ndarray):
        end, eo = self.exec_eager_words(base, off=off)
        return end, self._decode(eo)

    def exec_offsets_device_front(self, what: str, d_base: int, d_off: int, n: int, d_out: int, d_aux: int = 0, mode: int = 1, stream: int = 0):
        """The *_offsets_device entry points: what = 'ids' (d_out = ids), 'resume' (d_out = state_io, d_aux = end), 'eager' (d_out = end, d_aux = sets)."""
        args = {"ids": (mode, d_out), "resume": (d_out, d_aux or None, None), "eager": (d_out or None, d_aux)}[what]
        _call("fsm_hip_exec_batch_%s_offsets_device" % what, self._h, d_base, d_off, n, *args, stream or None)

    def eager_id_count(self) -> int:
        return int(self._lib.fsm_hip_eager_id_count(self._h))

    def eager_id(self, bit: int) -> int:
        return int(self._lib.fsm_hip_eager_id(self._h, bit))

    def ret_sets(self):
        """The de-duplicated end-id sets, in retlist order."""
        out = []
        for k in range(self._lib.fsm_hip_ret_count(self._h)):
            p, n = C.c_void_p(), C.c_size_t()
            assert self._lib.fsm_hip_ret_get(self._h, k, C.byref(p), C.byref(n)) == 0
            out.append(np.frombuffer((C.c_char * (n.value * 4)).from_address(p.value), dtype=np.uint32).copy() if n.value else np.zeros(0, np.uint32))
        return out

    def ids_conflict(self):
        """AMBIG_ERROR's check: None, or the lowest end state that carries more than one end-id."""
        st = C.c_uint(0)
        r = _call("fsm_hip_ids_conflict", self._h, C.byref(st), negative_only=True)
        return int(st.value) if r == 1 else None

    def state_is_absorbing(self, state: int) -> bool:
        return bool(_call("fsm_hip_state_is_absorbing", self._h, state, negative_only=True))

    def match_file(self, path: str) -> int:
        """fsm_hip_match_file(dfa, FILE *) on a file opened with the C library."""
        with _fopen(path, b"rb") as f:
            return _call("fsm_hip_match_file", self._h, f, negative_only=True)

    def match_buffer_big(self, data: bytes):
        """fsm_hip_match_buffer_big: (1 / 0, caller's end state or NO_MATCH) of ONE input walked by the whole device."""
        e = C.c_uint32(NO_MATCH)
        buf = (C.c_char * max(len(data), 1)).from_buffer_copy(data if len(data) else b"\0")
        r = _call("fsm_hip_match_buffer_big", self._h, buf, len(data), C.byref(e), negative_only=True)
        return r, e.value

    def match_buffer_big_eager(self, data: bytes):
        """fsm_hip_match_buffer_big_eager: (1 / 0, caller's end state or NO_MATCH, sorted u32 ids of the eager outputs emitted
        over the whole input) of ONE input walked by the whole device."""
        e = C.c_uint32(NO_MATCH)
        eo = np.zeros(self.eager_words(), np.uint64)
        buf = (C.c_char * max(len(data), 1)).from_buffer_copy(data if len(data) else b"\0")
        r = _call("fsm_hip_match_buffer_big_eager", self._h, buf, len(data), C.byref(e), _ptr(eo), negative_only=True)
        return r, e.value, self._eager_ids_of(eo)

    def match_file_eager(self, path: str):
        """fsm_hip_match_file_eager on a file opened with the C library: (1 / 0, end state or NO_MATCH, sorted u32 ids)."""
        e = C.c_uint32(NO_MATCH)
        eo = np.zeros(self.eager_words(), np.uint64)
        with _fopen(path, b"rb") as f:
            r = _call("fsm_hip_match_file_eager", self._h, f, C.byref(e), _ptr(eo), negative_only=True)
        return r, e.value, self._eager_ids_of(eo)

    def match_last_passes(self):
        """(windows, passes) of the last match_file / match_buffer_big call of this process"""
        w, p_ = C.c_uint(0), C.c_uint(0)
        self._lib.fsm_hip_match_last_passes(C.byref(w), C.byref(p_))
        return w.value, p_.value

    def last_kernel_ms(self) -> float:
        return float(self._lib.fsm_hip_last_kernel_ms(self._h))

    # ---- end-ids --------------------------------------------------------------
    def endids(self, end_state: int) -> np.ndarray:
        n = self._lib.fsm_hip_endid_count(self._h, end_state)
        buf = np.zeros(max(n, 1), dtype=np.uint32)
        if self._lib.fsm_hip_endid_get(self._h, end_state, n, _ptr(buf)) != 1:
            raise RuntimeError("fsm_hip_endid_get")
        return buf[:n]


class HipNode(_Owned):
    """struct fsm_hip_node *: one table replica per device, a batch sharded over them (include/fsm_hip.h)."""

    _FREE = "fsm_hip_node_free"

    def __init__(self, flat: FlatDfa, devices: Optional[Sequence[int]] = None, flags: int = 0):
        d = flat.desc()
        devs = (C.c_int * len(devices))(*devices) if devices else None
        super().__init__(_call("fsm_hip_node_create", C.byref(d), flags, devs, len(devices) if devices else 0))
        self.ndev = int(self._lib.fsm_hip_node_ndev(self._h))

    def uses_rccl(self) -> bool:
        return bool(self._lib.fsm_hip_node_uses_rccl(self._h))

    def rccl_path(self) -> str:
        return (self._lib.fsm_hip_node_rccl_path() or b"").decode()

    def replica(self, k: int) -> "HipDfa":
        """Borrowed view of the k-th replica (do not close it)."""
        h = self._lib.fsm_hip_node_dfa(self._h, k)
        if not h:
            raise _oserr("fsm_hip_node_dfa")
        return HipDfa(handle=h, borrowed=True)

    def shard(self, n: int, k: int):
        f, c = C.c_size_t(), C.c_size_t()
        self._lib.fsm_hip_node_shard(self._h, n, k, C.byref(f), C.byref(c))
        return int(f.value), int(c.value)

    def bitmap_words(self, n: int) -> int:
        return int(self._lib.fsm_hip_node_bitmap_words(self._h, n))

    # ---- host-buffer fronts: HipDfa's, sharded over the devices ----
    def exec_batch(self, data: np.ndarray, lens: Optional[np.ndarray] = None):
        return _exec_rows("fsm_hip_node_exec_batch", self._h, data, lens)

    def exec_batch_offsets32(self, base: np.ndarray, off32: np.ndarray, want_bitmap: bool = True, want_end: bool = True):
        """fsm_hip_node_exec_batch_offsets32: u32 offsets (batches below 4 GiB)."""
        return _exec_packed("fsm_hip_node_exec_batch_offsets32", self._h, base, off32, np.uint32, want_bitmap, want_end)

    def exec_batch_lengths(self, base: np.ndarray, lens: np.ndarray, want_bitmap: bool = True, want_end: bool = True):
        """fsm_hip_node_exec_batch_lengths: inputs packed back to back, their lengths and nothing else."""
        return _exec_packed("fsm_hip_node_exec_batch_lengths", self._h, base, lens, np.uint32, want_bitmap, want_end)

    def exec_batch_offsets(self, base: np.ndarray, off: np.ndarray, want_bitmap: bool = True, want_end: bool = True):
        """fsm_hip_node_exec_batch_offsets: u64 offsets."""
        return _exec_packed("fsm_hip_node_exec_batch_offsets", self._h, base, off, np.uint64, want_bitmap, want_end)

    def exec_strings(self, strings: Sequence[bytes]):
        return self.exec_batch_offsets(*_pack_strings(strings, pad=b"\0"))

    def exec_batch_ids(self, data: np.ndarray, mode: int, lens: Optional[np.ndarray] = None) -> np.ndarray:
        return _exec_rows_ids("fsm_hip_node_exec_batch_ids", self._h, data, mode, lens)

    def exec_batch_eager(self, data: np.ndarray, lens: Optional[np.ndarray] = None, want_end: bool = True, eager_out: Optional[np.ndarray] = None):
        """fsm_hip_node_exec_batch_eager: (end u32[n] or None, the raw sets u64[n, W]); decode with replica(0).decode_eager.
        eager_out: the caller's own n * W words to write into (returned reshaped) instead of fresh zeros."""
        data, lens, _, n, stride = _inputs(data, lens)
        W = self.replica(0).eager_words()
        end = np.empty(n, dtype=np.uint32) if want_end else None
        if eager_out is None:
            eager_out = np.zeros((n, W), dtype=np.uint64)
        if eager_out.dtype != np.uint64 or eager_out.size != n * W or not eager_out.flags.c_contiguous:
            raise ValueError("eager_out: n * W contiguous u64 words")
        _call("fsm_hip_node_exec_batch_eager", self._h, _ptr(data), stride, _ptr(lens), n, _ptr(end), _ptr(eager_out))
        return end, eager_out.reshape(n, W)

    # ---- device-pointer fronts: per-device lists of device pointers ----
    def _ptrs(self, xs):
        """a list of ndev addresses (0 / None: NULL) as a C array, None as NULL"""
        return None if xs is None else (C.c_void_p * self.ndev)(*[x or None for x in xs])

    def exec_batch_device(self, d_base: Sequence[int], stride: int, n: int, d_end: Optional[Sequence[int]] = None,
                          d_bitmap_all: Optional[Sequence[int]] = None, want_count: bool = False):
        cnt = C.c_uint64(0)
        _call("fsm_hip_node_exec_batch_device", self._h, self._ptrs(d_base), stride, n, self._ptrs(d_end), self._ptrs(d_bitmap_all),
              C.byref(cnt) if want_count else None)
        return int(cnt.value) if want_count else None

    def exec_device(self, n: int, d_base, stride: int = 0, d_len=None, d_off=None, d_end=None, d_ids=None, ids_mode: int = 1,
                    d_eager=None, d_bitmap_all=None, want_count: bool = False, async_: bool = False):
        """fsm_hip_node_exec_device: per-device lists of device pointers (None entries allowed where the header allows them)."""
        keep = [self._ptrs(xs) for xs in (d_base, d_len, d_off, d_end, d_ids, d_eager, d_bitmap_all)]
        base, lens, off, end, ids, eager, bms = (a if a is None else C.cast(a, PP) for a in keep)
        b = NodeBatch(base, stride, lens, off, end, ids, ids_mode, eager, bms, 1 if want_count else 0)
        cnt = C.c_uint64(0)
        count_now = want_count and not async_
        _call("fsm_hip_node_exec_device", self._h, C.byref(b), n, C.byref(cnt) if count_now else None, 1 if async_ else 0)
        return int(cnt.value) if count_now else None

    def wait(self, want_count: bool = False):
        cnt = C.c_uint64(0)
        _call("fsm_hip_node_wait", self._h, C.byref(cnt) if want_count else None)
        return int(cnt.value) if want_count else None


# ---- many DFAs in one submission: MultiBatch (end, bitmap), MultiBatchIds (+ ids), MultiBatchEager (+ eager sets) --------------

_MULTI = {5: (MultiBatch, ""), 6: (MultiBatchIds, "_ids"), 7: (MultiBatchEager, "_eager")}    # by the number of fields


def _multi_args(struct, owners, jobs):
    """(handles, batches, k) of a submission: jobs[q] = the addresses of struct's fields, in order (0 / None: NULL; n: a count)"""
    k = len(jobs)
    if any(len(j) != len(struct._fields_) for j in jobs):
        raise ValueError("a job of %s is a %d-tuple" % (struct.__name__, len(struct._fields_)))
    arr = (struct * max(k, 1))()
    for q, j in enumerate(jobs):
        for (name, _), v in zip(struct._fields_, j):
            setattr(arr[q], name, v if name == "n" else (v or None))
    return (C.c_void_p * max(k, 1))(*[o._h if o is not None else None for o in owners]), arr, k


def _multi_host(width, fn, owners, jobs, *tail, want_bitmap=True, eager_words=None):
    """One submission of strings: job q = jobs[q] packed, with fresh outputs (end and ids poisoned, so that a job the library
    passes over shows) -> per job [end, bitmap, ids, sets][:width - 3].  eager_words[q]: the words of a set of job q, None: no sets."""
    struct, outs, rows, keep = _MULTI[width][0], [], [], []
    for q, strs in enumerate(jobs):
        n = len(strs)
        base, off = _pack_strings(strs, pad=b"\0")
        out = list(_outputs(n, True, want_bitmap, fill=0xDEADBEEF))
        if width >= 6:
            out.append(np.full(n, 0xDEADBEEF, dtype=np.uint32))
        if width == 7:
            out.append(np.full((n, eager_words[q]), 0xDEADBEEFDEADBEEF, dtype=np.uint64) if eager_words[q] is not None else None)
        keep.append((base, off))
        rows.append((base.ctypes.data, off.ctypes.data, n) + tuple(a.ctypes.data if (a is not None and n) else None for a in out))
        outs.append(out)
    _call(fn, *_multi_args(struct, owners, rows), *tail)
    return outs


def exec_multi(dfas: Sequence["HipDfa"], jobs: Sequence[Sequence[bytes]], want_bitmap: bool = True, nodes: Optional[Sequence["HipNode"]] = None):
    """fsm_hip_exec_multi: job q = the strings jobs[q] through dfas[q]; ONE submission.  Returns [(end, bitmap), ...].
    nodes: fsm_hip_node_exec_multi instead (the list sharded by DFA over the nodes' devices)."""
    if nodes is not None:
        return [tuple(o) for o in _multi_host(5, "fsm_hip_node_exec_multi", nodes, jobs, want_bitmap=want_bitmap)]
    return [tuple(o) for o in _multi_host(5, "fsm_hip_exec_multi", dfas, jobs, want_bitmap=want_bitmap)]


def exec_multi_ids(dfas: Sequence["HipDfa"], jobs: Sequence[Sequence[bytes]], ids_mode: int):
    """fsm_hip_exec_multi_ids: job q = the strings jobs[q] through dfas[q], ONE submission, end-ids by the device.
    Returns [(end, bitmap, ids), ...]."""
    return [tuple(o) for o in _multi_host(6, "fsm_hip_exec_multi_ids", dfas, jobs, ids_mode)]


def exec_multi_eager(dfas: Sequence["HipDfa"], jobs: Sequence[Sequence[bytes]], ids_mode: int = 1, want_eager: Optional[Sequence[bool]] = None):
    """fsm_hip_exec_multi_eager: job q = the strings jobs[q] through dfas[q], ONE submission, end-ids and eager-output sets by
    the device.  Returns [(end, bitmap, ids, sets), ...], sets decoded like exec_batch_eager (one array of emitted ids per
    string); want_eager[q] = False leaves job q's eager_out NULL (its sets: None)."""
    words = [dfas[q].eager_words() if (want_eager is None or want_eager[q]) else None for q in range(len(jobs))]
    outs = _multi_host(7, "fsm_hip_exec_multi_eager", dfas, jobs, ids_mode, eager_words=words)
    return [(e, m, i, None if eo is None else dfas[q].decode_eager(eo)) for q, (e, m, i, eo) in enumerate(outs)]


def exec_multi_device(dfas: Sequence["HipDfa"], jobs: Sequence[tuple], stream: int = 0):
    """fsm_hip_exec_multi_device: jobs[q] = (d_base, d_off, n, d_end, d_bitmap) device pointers (0 = NULL)."""
    _call("fsm_hip_exec_multi_device", *_multi_args(MultiBatch, dfas, jobs), stream or None)


def exec_multi_ids_device(dfas: Sequence["HipDfa"], jobs: Sequence[tuple], ids_mode: int, stream: int = 0):
    """fsm_hip_exec_multi_ids_device: jobs[q] = (d_base, d_off, n, d_end, d_bitmap, d_ids) device pointers (0 = NULL)."""
    _call("fsm_hip_exec_multi_ids_device", *_multi_args(MultiBatchIds, dfas, jobs), ids_mode, stream or None)


def exec_multi_eager_device(dfas: Sequence["HipDfa"], jobs: Sequence[tuple], ids_mode: int = 1, stream: int = 0):
    """fsm_hip_exec_multi_eager_device: jobs[q] = (d_base, d_off, n, d_end, d_bitmap, d_ids, d_eager) device pointers (0 = NULL);
    d_eager: n * dfas[q].eager_words() u64."""
    _call("fsm_hip_exec_multi_eager_device", *_multi_args(MultiBatchEager, dfas, jobs), ids_mode, stream or None)


def exec_multi_ptrs(dfas: Sequence[Optional["HipDfa"]], jobs: Sequence[tuple], ids_mode: int = 0, device: bool = False, stream: int = 0) -> None:
    """A many-DFA submission given as addresses, host memory (device=False) or device memory: jobs[q] = (base, off, n, end,
    bitmap) -> fsm_hip_exec_multi[_device], with a sixth (ids) -> fsm_hip_exec_multi_ids[_device], with a seventh (eager) ->
    fsm_hip_exec_multi_eager[_device]; every job of a submission has the same length.  0 = NULL: an output left out; dfas[q]
    None: a NULL handle.  The caller keeps the memory alive and reads the outputs where it put them."""
    width = len(jobs[0]) if len(jobs) else 5
    if width not in _MULTI or any(len(j) != width for j in jobs):
        raise ValueError("every job is a 5-tuple, a 6-tuple or a 7-tuple")
    struct, suffix = _MULTI[width]
    _call("fsm_hip_exec_multi" + suffix + ("_device" if device else ""), *_multi_args(struct, dfas, jobs),
          *([ids_mode] if width != 5 else []), *([stream or None] if device else []))


class MultiPrepared(_Owned):
    """fsm_hip_multi_prepare / _launch / _prepared_free: a device-pointer submission put on the device once; launch() is
    one kernel launch on the stream (capturable into a HIP graph).  jobs[q] = (d_base, d_off, n, d_end, d_bitmap, d_ids), or
    -- every job of the submission -- (d_base, d_off, n, d_end, d_bitmap, d_ids, d_eager): fsm_hip_multi_prepare_eager."""

    _FREE = "fsm_hip_multi_prepared_free"

    def __init__(self, dfas: Sequence["HipDfa"], jobs: Sequence[tuple], ids_mode: int = 0):
        eager = len(jobs) != 0 and len(jobs[0]) == 7
        if any(len(j) != (7 if eager else 6) for j in jobs):
            raise ValueError("every job is a 6-tuple, or every job is a 7-tuple")
        p = C.c_void_p()
        _call("fsm_hip_multi_prepare_eager" if eager else "fsm_hip_multi_prepare", *_multi_args(MultiBatchEager if eager else MultiBatchIds, dfas, jobs),
              ids_mode, C.byref(p))
        super().__init__(p.value, list(dfas))

    def launch(self, stream: int = 0) -> None:
        _call("fsm_hip_multi_launch", self._h, stream or None)


def multi_last_launches() -> int:
    return int(load_library().fsm_hip_multi_last_launches())


def multi_last_fused_jobs() -> int:
    return int(load_library().fsm_hip_multi_last_fused_jobs())


def multi_assign(cost: Sequence[int], ndev: int) -> np.ndarray:
    """fsm_hip_multi_assign: which device takes which job of a many-DFA submission (largest first, least loaded device).  Host arithmetic only."""
    c = np.ascontiguousarray(cost, dtype=np.uint64)
    out = np.zeros(len(c), dtype=np.int32)
    _call("fsm_hip_multi_assign", _ptr0(c), len(c), ndev, _ptr(out) if len(c) else None)
    return out


# ---- input generators and probes ----

def _bytes_arg(b):
    """bytes -> (its u8 copy or None, its length) as the generators take a byte set"""
    a = np.frombuffer(bytes(b), dtype=np.uint8).copy() if b else None
    return a, (len(a) if a is not None else 0)


def gen_inputs_host(n: int, stride: int, first_index: int = 0, seed: int = 0x5EEDF5A1, alphabet: Optional[bytes] = None,
                    plant: Optional[bytes] = None, plant_every: int = 0) -> np.ndarray:
    out = np.empty((n, stride), dtype=np.uint8)
    (a, na), (p, np_) = _bytes_arg(alphabet), _bytes_arg(plant)
    load_library().fsm_hip_gen_inputs_host(_ptr(out), stride, n, first_index, seed, _ptr(a), na, _ptr(p), np_, plant_every)
    return out


def gen_inputs_device(d_base: int, n: int, stride: int, first_index: int = 0, seed: int = 0x5EEDF5A1,
                      alphabet: Optional[bytes] = None, plant: Optional[bytes] = None, plant_every: int = 0, stream: int = 0):
    (a, na), (p, np_) = _bytes_arg(alphabet), _bytes_arg(plant)
    _call("fsm_hip_gen_inputs_device", d_base, stride, n, first_index, seed, _ptr(a), na, _ptr(p), np_, plant_every, stream or None)


def gen_pack_rows_device(d_rows: int, stride: int, d_len: int, d_off: int, n: int, max_len: int, d_out: int, stream: int = 0):
    """fsm_hip_gen_pack_rows_device: input i = the first len[i] bytes of row i, packed at d_out + off[i]."""
    _call("fsm_hip_gen_pack_rows_device", d_rows, stride, d_len, d_off, n, max_len, d_out, stream or None)


def gather_probe_ms(d_base: int, nbytes: int, ngathers: int, vec_bytes: int, d_scratch4: int, stream: int = 0) -> float:
    """fsm_hip_gather_probe_ms: one launch of `ngathers` independent vec_bytes-byte loads at pseudo-random offsets of the buffer."""
    ms = load_library().fsm_hip_gather_probe_ms(d_base, nbytes, ngathers, vec_bytes, d_scratch4, stream or None)
    if ms < 0:
        raise _oserr("fsm_hip_gather_probe_ms")
    return float(ms)


def lds_chain_probe_gbps(table_bytes: int, waves: int, blocks_per_cu: int, steps: int, d_scratch4: int, stream: int = 0) -> float:
    """fsm_hip_lds_chain_probe_gbps: what a dependent chain of random LDS reads sustains (the lookup layouts' ceiling)."""
    C.set_errno(0)
    r = load_library().fsm_hip_lds_chain_probe_gbps(table_bytes, waves, blocks_per_cu, steps, d_scratch4, stream or None)
    if r < 0:
        raise _oserr("fsm_hip_lds_chain_probe_gbps")
    return float(r)


def waves_by_occupancy(vgprs: int, workgroups_by_lds: int, max_waves: int = 16) -> int:
    """fsm_hip_waves_by_occupancy: the workgroup size (wavefronts) a latency-bound per-lane kernel gets (pure arithmetic)."""
    return int(load_library().fsm_hip_waves_by_occupancy(vgprs, workgroups_by_lds, max_waves))


def pack_affixes(items: Sequence[bytes]) -> np.ndarray:
    """[len<=7, b0..b6] entries for the affix generator."""
    t = np.zeros((len(items), 8), dtype=np.uint8)
    for i, s in enumerate(items):
        assert len(s) <= 7
        t[i, 0] = len(s)
        t[i, 1:1 + len(s)] = np.frombuffer(s, dtype=np.uint8)
    return t


def _affix_args(alphabet, body, body2, prefixes, suffixes, every):
    """the generators' arguments between the seed and the stream: {bytes, count} of alphabet, body, body2, prefixes, suffixes; every"""
    (a, na), (b, nb), (b2, nb2) = _bytes_arg(alphabet), _bytes_arg(body), _bytes_arg(body2)
    p, s = pack_affixes(prefixes), pack_affixes(suffixes)
    return _ptr(a), na, _ptr(b), nb, _ptr(b2), nb2, _ptr(p), len(p), _ptr(s), len(s), every


def gen_affix_inputs_host(n: int, stride: int, first_index: int, seed: int, alphabet: bytes, body: bytes,
                          prefixes: Sequence[bytes], suffixes: Sequence[bytes], every: int = 2, body2: Optional[bytes] = None) -> np.ndarray:
    """body2: alternate body / body2 byte by byte after the prefix (fsm_hip_gen_affix2_inputs_host)."""
    out = np.empty((n, stride), dtype=np.uint8)
    load_library().fsm_hip_gen_affix2_inputs_host(_ptr(out), stride, n, first_index, seed, *_affix_args(alphabet, body, body2, prefixes, suffixes, every))
    return out


def gen_affix_inputs_device(d_base: int, n: int, stride: int, first_index: int, seed: int, alphabet: bytes, body: bytes,
                            prefixes: Sequence[bytes], suffixes: Sequence[bytes], every: int = 2, stream: int = 0, body2: Optional[bytes] = None):
    _call("fsm_hip_gen_affix2_inputs_device", d_base, stride, n, first_index, seed, *_affix_args(alphabet, body, body2, prefixes, suffixes, every),
          stream or None)


def stream_read_probe_gbps(d_base: int, nbytes: int, d_scratch4: int, reps: int = 3, stream: int = 0) -> float:
    """GB/s of a trivially coalesced read-only kernel over the same buffer (measured HBM ceiling)."""
    ms = load_library().fsm_hip_stream_read_probe_ms(d_base, nbytes, d_scratch4, reps, stream or None)
    if ms <= 0:
        raise _oserr("fsm_hip_stream_read_probe_ms")
    return nbytes / (ms * 1e-3) / 1e9


# ---- the text front: one buffer with a delimiter between records (include/fsm_hip.h) ----

def identity_byte(flat: FlatDfa, byte: int) -> FlatDfa:
    """fsm_hip_desc_identity_byte: a copy of the description in which `byte` is a self-loop of every state (host arithmetic)."""
    d = flat.desc()
    return FlatDfa._take(_call("fsm_hip_desc_identity_byte", C.byref(d), int(byte)))


class LinesDfa(_Owned):
    """struct fsm_hip_lines_dfa *: the twin automaton in which the delimiter is a self-loop of every state, and that delimiter.
    .inner is the HipDfa to ask for end-ids, ret sets, eager ids, info, the last kernel and tuning (borrowed)."""

    _FREE = "fsm_hip_lines_dfa_free"

    def __init__(self, flat: FlatDfa, delim: int = 0x0A, flags: int = 0):
        d = flat.desc()
        super().__init__(_call("fsm_hip_lines_dfa_create", C.byref(d), delim, flags))
        self.inner = HipDfa(handle=self._lib.fsm_hip_lines_dfa_inner(self._h), borrowed=True)

    @property
    def delim(self) -> int:
        return int(self._lib.fsm_hip_lines_dfa_delim(self._h))

    def close(self):
        if getattr(self, "inner", None) is not None:
            self.inner._h = None      # it dies with the twin
        super().close()


class HipText(_Owned):
    """struct fsm_hip_text *: bytes on the device plus the offsets of their lines.  data: host bytes (copied once), or
    d_text = a device address with nbytes (borrowed: it must outlive the text; the scan is enqueued on `stream`).
    file_off: the text is files back to back (fsm_hip_text_open_files*): nfiles + 1 byte positions, a host array with `data`, with
    d_text either a device address (borrowed, with nfiles=) or an array-like that is copied to the device and kept."""

    _FREE = "fsm_hip_text_free"

    def __init__(self, data=None, delim: int = 0x0A, *, d_text: int = 0, nbytes: int = 0, stream: int = 0, file_off=None, nfiles: int = 0):
        if data is not None:
            buf = np.ascontiguousarray(np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray)) else data, dtype=np.uint8)
        if data is not None and file_off is not None:
            fo = np.ascontiguousarray(file_off, dtype=np.uint64)
            h = _call("fsm_hip_text_open_files", _ptr0(buf), buf.size, delim, _ptr0(fo), max(fo.size, 1) - 1)
        elif data is not None:
            h = _call("fsm_hip_text_open", _ptr0(buf), buf.size, delim)
        elif file_off is not None:
            if not isinstance(file_off, (int, np.integer)):   # a host array: its device copy lives as long as the text
                import torch
                fo = np.ascontiguousarray(file_off, dtype=np.uint64)
                self._file_off = torch.from_numpy(fo.view(np.int64).copy()).cuda() if fo.size else None
                file_off, nfiles = (self._file_off.data_ptr() if fo.size else 0), max(fo.size, 1) - 1
            h = _call("fsm_hip_text_open_files_device", d_text or None, nbytes, delim, int(file_off) or None, nfiles, stream or None)
        else:
            h = _call("fsm_hip_text_open_device", d_text or None, nbytes, delim, stream or None)
        super().__init__(h)

    lines = _size("fsm_hip_text_lines")
    d_off = _dev("fsm_hip_text_offsets_device")

    def offsets(self) -> np.ndarray:
        off = np.empty(self.lines + 1, np.uint64)
        _call("fsm_hip_text_offsets", self._h, _ptr(off))
        return off

    def scan_ms(self) -> float:
        return float(self._lib.fsm_hip_text_scan_ms(self._h))

    files = _size("fsm_hip_text_files", "fsm_hip_text_files: 0 for a plain text")
    file_lines_ptr = _dev("fsm_hip_text_file_lines_device")

    def file_lines(self) -> np.ndarray:
        """fsm_hip_text_file_lines: the files + 1 line indices at which the files begin (raises EINVAL on a plain text)"""
        out = np.empty(self.files + 1, np.uint64)
        _call("fsm_hip_text_file_lines", self._h, _ptr(out))
        return out

    def files_ms(self) -> float:
        return float(self._lib.fsm_hip_text_files_ms(self._h))

    def exec(self, ld: LinesDfa, ids_mode: int = 0, want_end=True, want_bitmap=False, want_eager=False, out: Optional[dict] = None):
        """fsm_hip_text_exec: dict(end=, bitmap=, ids=, eager=) with the outputs asked for (out: arrays to write into instead)."""
        n = self.lines
        if out is None:
            end, bm = _outputs(n, want_end, want_bitmap)
            out = {"end": end, "bitmap": bm, "ids": np.empty(n, np.uint32) if ids_mode else None,
                   "eager": np.zeros((n, ld.inner.eager_words()), np.uint64) if want_eager else None}
        _call("fsm_hip_text_exec", ld.handle, self._h, _ptr(out.get("end")), _ptr(out.get("bitmap")), ids_mode, _ptr(out.get("ids")), _ptr(out.get("eager")))
        return out

    def exec_device(self, ld: LinesDfa, d_end: int = 0, d_bitmap: int = 0, ids_mode: int = 0, d_ids: int = 0, d_eager: int = 0, stream: int = 0):
        _call("fsm_hip_text_exec_device", ld.handle, self._h, d_end or None, d_bitmap or None, ids_mode, d_ids or None, d_eager or None, stream or None)

    def hits(self, ld: LinesDfa, invert: bool = False, want_bytes: bool = True) -> "HipHits":
        """fsm_hip_text_hits: walk the text with ld and select the accepted lines (invert: the others)."""
        return HipHits(_call("fsm_hip_text_hits", ld.handle, self._h, hits_flags(invert, want_bytes)), self)

    def hits_device(self, d_bitmap: int, invert: bool = False, want_bytes: bool = True, stream: int = 0, flags: Optional[int] = None) -> "HipHits":
        """fsm_hip_text_hits_device: select by a caller-made bitmap on the device (ceil(n / 64) words, bit i = line i), enqueued on
        `stream`.  flags: the raw flag word instead of invert / want_bytes."""
        flags = hits_flags(invert, want_bytes) if flags is None else flags
        return HipHits(_call("fsm_hip_text_hits_device", self._h, d_bitmap or None, flags, stream or None), self)

    def hits_context(self, ld: LinesDfa, before: int, after: int, invert: bool = False, want_bytes: bool = True) -> "HipHits":
        """fsm_hip_text_hits_context: the hits of the lines within `before` / `after` lines of an accepted line of the same file
        (grep -B / -A; any value below 2 ** 64), with the core and group marks."""
        return HipHits(_call("fsm_hip_text_hits_context", ld.handle, self._h, hits_flags(invert, want_bytes), before, after), self)

    def hits_context_device(self, d_bitmap: int, before: int, after: int, invert: bool = False, want_bytes: bool = True, stream: int = 0,
                            flags: Optional[int] = None) -> "HipHits":
        """fsm_hip_text_hits_context_device: as hits_device, widened by the context."""
        flags = hits_flags(invert, want_bytes) if flags is None else flags
        return HipHits(_call("fsm_hip_text_hits_context_device", self._h, d_bitmap or None, flags, before, after, stream or None), self)


def hits_flags(invert: bool, want_bytes: bool) -> int:
    return (HITS_INVERT if invert else 0) | (0 if want_bytes else HITS_NO_BYTES)


class HipHits(_Owned):
    """struct fsm_hip_text_hits *: the selected lines' numbers, output offsets and bytes, packed on the device.  Keeps its text
    alive: the hits must be freed first."""

    _FREE = "fsm_hip_text_hits_free"

    def __init__(self, handle, text: HipText):
        super().__init__(handle)
        self._text = text

    def close(self):
        super().close()
        self._text = None

    count = _size("fsm_hip_text_hits_count")
    nbytes = _size("fsm_hip_text_hits_nbytes")
    lines_device = _dev("fsm_hip_text_hits_lines_device")
    offsets_device = _dev("fsm_hip_text_hits_offsets_device")
    bytes_device = _dev("fsm_hip_text_hits_bytes_device")

    def _copy(self, lines=None, off=None, data=None):
        _call("fsm_hip_text_hits_copy", self._h, _ptr(lines), _ptr(off), _ptr(data))

    def lines(self) -> np.ndarray:
        out = np.empty(self.count, np.uint64)
        self._copy(lines=out)
        return out

    def offsets(self) -> np.ndarray:
        out = np.empty(self.count + 1, np.uint64)
        self._copy(off=out)
        return out

    def bytes(self) -> np.ndarray:
        out = np.empty(self.nbytes, np.uint8)
        self._copy(data=out)
        return out

    def ms(self) -> float:
        return float(self._lib.fsm_hip_text_hits_ms(self._h))

    def gather_ms(self) -> float:
        return float(self._lib.fsm_hip_text_hits_gather_ms(self._h))

    file_first_ptr = _dev("fsm_hip_text_hits_file_first_device")

    def file_first(self) -> np.ndarray:
        """fsm_hip_text_hits_file_first: files + 1 entries, the hits of file j are [file_first[j], file_first[j + 1])"""
        out = np.empty(self._text.files + 1, np.uint64)
        _call("fsm_hip_text_hits_file_first", self._h, _ptr(out))
        return out

    def file_first_ms(self) -> float:
        return float(self._lib.fsm_hip_text_hits_file_first_ms(self._h))

    # hits with context (HipText.hits_context*); on plain hits: 0 from the pointers and the counts, EINVAL from the copies
    core_ptr = _dev("fsm_hip_text_hits_core_device")
    group_ptr = _dev("fsm_hip_text_hits_group_device")
    core_count = _size("fsm_hip_text_hits_core_count", "fsm_hip_text_hits_core_count: the selected lines, context left out (grep -c)")
    groups = _size("fsm_hip_text_hits_groups")

    def _marks(self, which: int) -> np.ndarray:
        m = self.count
        words = _outputs(m, False)[1]
        _call("fsm_hip_text_hits_marks", self._h, _ptr(words) if which == 0 else None, _ptr(words) if which == 1 else None)
        return np.unpackbits(words.view(np.uint8), bitorder="little")[:m].astype(bool)

    def core(self) -> np.ndarray:
        """one bool per hit: the hit is a selected line, not context"""
        return self._marks(0)

    def group(self) -> np.ndarray:
        """one bool per hit: the hit begins a group (grep prints -- before every group but the first)"""
        return self._marks(1)

    def marks_words(self):
        """fsm_hip_text_hits_marks as it is: (core, group), ceil(m / 64) words each"""
        core, group = _outputs(self.count, False)[1], _outputs(self.count, False)[1]
        _call("fsm_hip_text_hits_marks", self._h, _ptr(core), _ptr(group))
        return core, group

    def context_ms(self) -> float:
        return float(self._lib.fsm_hip_text_hits_context_ms(self._h))

    def distinct(self, sep_byte: int = -1, flags: int = 0, stream: int = 0) -> "HipDistinct":
        """fsm_hip_text_hits_distinct: the distinct lines of these hits, trimmed by the text's delimiter"""
        return HipDistinct(_call("fsm_hip_text_hits_distinct", self._h, sep_byte, flags, stream or None), (self,))

    def sort(self, sep_byte: int = -1, flags: int = 0, stream: int = 0) -> "HipSorted":
        """fsm_hip_text_hits_sort: the lines of these hits in byte order, trimmed by the text's delimiter"""
        return HipSorted(_call("fsm_hip_text_hits_sort", self._h, sep_byte, flags, stream or None), (self,))


def text_block_bytes() -> int:
    """fsm_hip_text_block_bytes: bytes one workgroup of the delimiter scan covers per step."""
    return int(load_library().fsm_hip_text_block_bytes())


def text_max_workgroups() -> int:
    """fsm_hip_text_max_workgroups: the most workgroups a scan launches on the current device."""
    return int(load_library().fsm_hip_text_max_workgroups())


def text_hits_block_lines() -> int:
    """fsm_hip_text_hits_block_lines: lines one workgroup of the select covers per step."""
    return int(load_library().fsm_hip_text_hits_block_lines())


def text_hits_block_bytes() -> int:
    """fsm_hip_text_hits_block_bytes: output bytes one workgroup of the gather covers per step."""
    return int(load_library().fsm_hip_text_hits_block_bytes())


def text_files_block() -> int:
    """fsm_hip_text_files_block: file ends one round of the files scan takes."""
    return int(load_library().fsm_hip_text_files_block())


def text_context_scan_block() -> int:
    """fsm_hip_text_context_scan_block: blocks of lines one round of the context scan takes."""
    return int(load_library().fsm_hip_text_context_scan_block())


# ---- match positions: first / last accepting offset, spans of a text's hits (include/fsm_hip.h, "match positions") ----

class PosDfa(_Owned):
    """struct fsm_hip_pos_dfa *: the device image of a HipDfa for the accept-position walk (the dfa may be closed afterwards)."""

    _FREE = "fsm_hip_pos_dfa_free"

    def __init__(self, dfa: "HipDfa"):
        super().__init__(_call("fsm_hip_pos_dfa_create", dfa.handle if dfa is not None else None))

    @classmethod
    def from_flat(cls, flat: FlatDfa) -> "PosDfa":
        """the image of a description: planned with DEFER_UPLOAD, so no other table goes to the device"""
        dfa = HipDfa(flat, DEFER_UPLOAD)
        try:
            return cls(dfa)
        finally:
            dfa.close()

    @property
    def in_lds(self) -> bool:
        return bool(self._lib.fsm_hip_pos_dfa_in_lds(self._h))

    def accept_pos(self, base: np.ndarray, off: np.ndarray, pick=None, frm=None, to=None, trim_byte: int = -1, backward: bool = False,
                   want_first: bool = True, want_last: bool = True, out: Optional[tuple] = None):
        """fsm_hip_exec_accept_pos on host arrays -> (first, last), u64 [m] each (None for the one not asked for).  out: the
        (first, last) arrays to write into instead."""
        base, off, pick, n, m = _line_arrays(base, off, pick)
        u64 = lambda a: None if a is None else np.ascontiguousarray(a, np.uint64)   # noqa: E731
        frm, to = u64(frm), u64(to)
        first, last = out if out is not None else (np.empty(m, np.uint64) if want_first else None, np.empty(m, np.uint64) if want_last else None)
        b = PosBatch(_ptr0(base), _ptr(off), n, _ptr(pick), m, _ptr(frm), _ptr(to), trim_byte, POS_BACKWARD if backward else 0, _ptr(first), _ptr(last), 0)
        _call("fsm_hip_exec_accept_pos", self._h, C.byref(b))
        return first, last

    def accept_pos_device(self, d_base: int, d_off: int, n: int, d_first: int = 0, d_last: int = 0, d_pick: int = 0, m: int = 0, d_from: int = 0,
                          d_to: int = 0, trim_byte: int = -1, backward: bool = False, limit: int = 0, stream: int = 0):
        """fsm_hip_exec_accept_pos_device: device addresses, asynchronous on `stream`"""
        b = _device_batch(PosBatch, d_base, d_off, n, d_pick, m, d_from or None, d_to or None, trim_byte, POS_BACKWARD if backward else 0,
                          d_first or None, d_last or None, limit)
        _call("fsm_hip_exec_accept_pos_device", self._h, C.byref(b), stream or None)


class HipSpans(_Owned):
    """struct fsm_hip_text_spans *: the leftmost-longest span of every hit, one match per round.  Keeps its hits, its text and
    the two images alive: the spans must be freed first."""

    _FREE = "fsm_hip_text_spans_free"

    def __init__(self, hits: "HipHits", starts: PosDfa, ends: PosDfa, stream: int = 0):
        self._m = hits.count
        super().__init__(_call("fsm_hip_text_hits_spans", hits.handle, hits._text.handle, starts.handle, ends.handle, stream or None),
                         (hits, hits._text, starts, ends))

    def next(self) -> None:
        """fsm_hip_text_spans_next: every hit's search position moves behind its match; the two walks run again"""
        _call("fsm_hip_text_spans_next", self._h)

    count = _size("fsm_hip_text_spans_count", "the hits with a span in the current round (one wait)")
    start_ptr = _dev("fsm_hip_text_spans_start_device")
    end_ptr = _dev("fsm_hip_text_spans_end_device")

    def copy(self):
        """-> (start, end), u64 [m] each, NO_POS where the hit has no span in this round"""
        start, end = np.empty(self._m, np.uint64), np.empty(self._m, np.uint64)
        _call("fsm_hip_text_spans_copy", self._h, _ptr(start), _ptr(end))
        return start, end

    def ms(self) -> float:
        return float(self._lib.fsm_hip_text_spans_ms(self._h))


# ---- tokens: every line cut into longest-match tokens with end-ids (include/fsm_hip.h, "tokens") ----

class TokDfa(_Owned):
    """struct fsm_hip_tok_dfa *: the device image of a HipDfa for the tokeniser's walk, one id per state under ids_mode (the dfa
    may be closed afterwards)."""

    _FREE = "fsm_hip_tok_dfa_free"

    def __init__(self, dfa: "HipDfa", ids_mode: int = IDS_EARLIEST):
        super().__init__(_call("fsm_hip_tok_dfa_create", dfa.handle if dfa is not None else None, ids_mode))

    @classmethod
    def from_flat(cls, flat: FlatDfa, ids_mode: int = IDS_EARLIEST) -> "TokDfa":
        """the image of a description: planned with DEFER_UPLOAD, so no other table goes to the device"""
        dfa = HipDfa(flat, DEFER_UPLOAD)
        try:
            return cls(dfa, ids_mode)
        finally:
            dfa.close()

    @property
    def in_lds(self) -> bool:
        return bool(self._lib.fsm_hip_tok_dfa_in_lds(self._h))

    def tokens(self, base: np.ndarray, off: np.ndarray, pick=None, trim_byte: int = -1, flags: int = 0) -> "HipTokens":
        """fsm_hip_tokens_run on host arrays"""
        b, _held = _host_batch(TokBatch, base, off, pick, trim_byte, flags, 0)
        return HipTokens(_call("fsm_hip_tokens_run", self._h, C.byref(b)), (self,))

    def tokens_device(self, d_base: int, d_off: int, n: int, d_pick: int = 0, m: int = 0, trim_byte: int = -1, flags: int = 0, limit: int = 0,
                      stream: int = 0) -> "HipTokens":
        """fsm_hip_tokens_run_device: device addresses; the emit pass is in flight on `stream` at return"""
        b = _device_batch(TokBatch, d_base, d_off, n, d_pick, m, trim_byte, flags, limit)
        return HipTokens(_call("fsm_hip_tokens_run_device", self._h, C.byref(b), stream or None), (self,))

    def text_tokens(self, text: "HipText", hits: Optional["HipHits"] = None, flags: int = 0, stream: int = 0) -> "HipTokens":
        """fsm_hip_text_tokens: every line of a text, or the lines of its hits"""
        return HipTokens(_call("fsm_hip_text_tokens", self._h, text.handle, hits.handle if hits is not None else None, flags, stream or None),
                         (self, text, hits))

    def text_matches(self, starts: PosDfa, text: "HipText", hits: Optional["HipHits"] = None, flags: int = 0, stream: int = 0) -> "HipMatches":
        """fsm_hip_text_matches with this image as `ends`: every match of every line of a text, or of the lines of its hits"""
        return HipMatches(_call("fsm_hip_text_matches", starts.handle, self._h, text.handle, hits.handle if hits is not None else None, flags,
                                stream or None), (starts, self, text, hits))


class _Tally:
    """the three forms of the tally (include/fsm_hip.h, "tally") over the off and id arrays an object owns; _TALLY: its name in
    the library's functions"""

    _TALLY = None

    def tally(self, group_off=None, nrules: int = 0, lines: bool = True, add_to=None):
        """fsm_hip_<object>_tally on host arrays -> (count, lines), each (G, nrules + 1) u64, lines None when not asked for;
        add_to: a (count, lines) pair of such arrays, or of None, that the new counts are added to"""
        goff = None if group_off is None else np.ascontiguousarray(group_off, np.uint64)
        G = 1 if goff is None else len(goff) - 1
        shape = (max(G, 0), nrules + 1)
        if add_to is not None:
            count, lin = (None if a is None else np.ascontiguousarray(a, np.uint64).reshape(shape).copy() for a in add_to)
        else:
            count, lin = np.zeros(shape, np.uint64), np.zeros(shape, np.uint64) if lines else None
        _call("fsm_hip_%s_tally" % self._TALLY, self._h, _ptr(goff), max(G, 0), nrules, TALLY_ADD if add_to is not None else 0, _ptr(count), _ptr(lin))
        return count, lin

    def tally_device(self, d_group_off: int, ngroups: int, nrules: int, d_count: int, d_lines: int, flags: int = 0, stream: int = 0) -> None:
        """fsm_hip_<object>_tally_device: device addresses, 0: NULL; in flight on `stream` at return"""
        _call("fsm_hip_%s_tally_device" % self._TALLY, self._h, d_group_off or None, ngroups, nrules, flags, d_count or None, d_lines or None,
              stream or None)

    def text_tally(self, text: "HipText", hits: Optional["HipHits"] = None, nrules: int = 0, d_count: int = 0, d_lines: int = 0, flags: int = 0,
                   stream: int = 0) -> None:
        """fsm_hip_text_<object>_tally: the groups are the files of the text (of its hits); tables of max(files, 1) rows on the device"""
        _call("fsm_hip_text_%s_tally" % self._TALLY, self._h, text.handle if text is not None else None, hits.handle if hits is not None else None,
              nrules, flags, d_count or None, d_lines or None, stream or None)


def tally_ids_device(d_off: int, d_id: int, m: int, total: int, d_group_off: int, ngroups: int, nrules: int, d_count: int, d_lines: int,
                     flags: int = 0, stream: int = 0) -> None:
    """fsm_hip_tally_ids_device: the reduction over any off[m + 1] / id[total] on the current device"""
    _call("fsm_hip_tally_ids_device", d_off or None, d_id or None, m, total, d_group_off or None, ngroups, nrules, flags, d_count or None,
          d_lines or None, stream or None)


def tally_span_inputs() -> int:
    return int(load_library().fsm_hip_tally_span_inputs())


def tally_window() -> int:
    return int(load_library().fsm_hip_tally_window())


def tally_lds_columns() -> int:
    return int(load_library().fsm_hip_tally_lds_columns())


def tally_max_line_columns() -> int:
    return int(load_library().fsm_hip_tally_max_line_columns())


class HipTokens(_Owned, _Tally):
    """struct fsm_hip_tokens *: off[m + 1], end[total], id[total], err[m] on the device.  Keeps its image (and its text and
    hits) alive: the tokens must be freed first."""

    _FREE = "fsm_hip_tokens_free"
    _TALLY = "tokens"
    count = _size("fsm_hip_tokens_count")
    total = _size("fsm_hip_tokens_total")
    off_ptr = _dev("fsm_hip_tokens_off_device")
    end_ptr = _dev("fsm_hip_tokens_end_device")
    id_ptr = _dev("fsm_hip_tokens_id_device")
    err_ptr = _dev("fsm_hip_tokens_err_device")

    def copy(self, extra: int = 0, fill: int = 0):
        """-> (off u64 [m + 1], end u64 [total], id u32 [total], err u64 [m]); extra: that many more entries in each array,
        pre-filled with `fill` and left alone by the library"""
        m, total = self.count, self.total
        off, end = np.full(m + 1 + extra, fill, np.uint64), np.full(total + extra, fill, np.uint64)
        ids, err = np.full(total + extra, fill & 0xFFFFFFFF, np.uint32), np.full(m + extra, fill, np.uint64)
        _call("fsm_hip_tokens_copy", self._h, _ptr(off), _ptr(end), _ptr(ids), _ptr(err))
        return off, end, ids, err

    def ms(self) -> float:
        return float(self._lib.fsm_hip_tokens_ms(self._h))

    def pass_ms(self, which: int) -> float:
        """0: the count pass, 1: the scan, 2: the emit pass"""
        return float(self._lib.fsm_hip_tokens_pass_ms(self._h, which))


# ---- matches: every match of every line, start / end / end-id, in one call (include/fsm_hip.h, "matches") ----

class HipMatches(_Freed, _Tally):
    """struct fsm_hip_matches *: off[m + 1], start[total], end[total], id[total] on the device.  Keeps its two images (and its
    text and hits) alive: the matches must be freed first."""

    _FREE = "fsm_hip_matches_free"
    _TALLY = "matches"

    @classmethod
    def run(cls, starts: PosDfa, ends: TokDfa, base: np.ndarray, off: np.ndarray, pick=None, trim_byte: int = -1, flags: int = 0) -> "HipMatches":
        """fsm_hip_matches_run on host arrays"""
        b, _held = _host_batch(MatchBatch, base, off, pick, trim_byte, flags, 0)
        return cls(_call("fsm_hip_matches_run", starts.handle, ends.handle, C.byref(b)), (starts, ends))

    @classmethod
    def run_device(cls, starts: PosDfa, ends: TokDfa, d_base: int, d_off: int, n: int, d_pick: int = 0, m: int = 0, trim_byte: int = -1,
                   flags: int = 0, limit: int = 0, stream: int = 0) -> "HipMatches":
        """fsm_hip_matches_run_device: device addresses; the emit pass is in flight on `stream` at return"""
        b = _device_batch(MatchBatch, d_base, d_off, n, d_pick, m, trim_byte, flags, limit)
        return cls(_call("fsm_hip_matches_run_device", starts.handle, ends.handle, C.byref(b), stream or None), (starts, ends))

    count = _size("fsm_hip_matches_count")
    total = _size("fsm_hip_matches_total")
    off_ptr = _dev("fsm_hip_matches_off_device")
    start_ptr = _dev("fsm_hip_matches_start_device")
    end_ptr = _dev("fsm_hip_matches_end_device")
    id_ptr = _dev("fsm_hip_matches_id_device")

    def copy(self, extra: int = 0, fill: int = 0):
        """-> (off u64 [m + 1], start u64 [total], end u64 [total], id u32 [total]); extra: that many more entries in each array,
        pre-filled with `fill` and left alone by the library"""
        m, total = self.count, self.total
        off, start = np.full(m + 1 + extra, fill, np.uint64), np.full(total + extra, fill, np.uint64)
        end, ids = np.full(total + extra, fill, np.uint64), np.full(total + extra, fill & 0xFFFFFFFF, np.uint32)
        _call("fsm_hip_matches_copy", self._h, _ptr(off), _ptr(start), _ptr(end), _ptr(ids))
        return off, start, end, ids

    def replace(self, repl: "HipRepl", base: np.ndarray, off: np.ndarray, pick=None, trim_byte: int = -1) -> "HipReplaced":
        """fsm_hip_matches_replace on host arrays: the batch these matches were made from"""
        b, _held = _host_batch(MatchBatch, base, off, pick, trim_byte, 0, 0)
        return HipReplaced(_call("fsm_hip_matches_replace", self._h, C.byref(b), repl.handle), (self, repl))

    def replace_device(self, repl: "HipRepl", d_base: int, d_off: int, n: int, d_pick: int = 0, m: int = 0, trim_byte: int = -1, limit: int = 0,
                       stream: int = 0) -> "HipReplaced":
        """fsm_hip_matches_replace_device: device addresses; the offsets and the write pass are in flight on `stream` at return"""
        b = _device_batch(MatchBatch, d_base, d_off, n, d_pick, m, trim_byte, 0, limit)
        return HipReplaced(_call("fsm_hip_matches_replace_device", self._h, C.byref(b), repl.handle, stream or None), (self, repl))

    def text_replace(self, repl: "HipRepl", text: "HipText", hits: Optional["HipHits"] = None, stream: int = 0) -> "HipReplaced":
        """fsm_hip_text_replace: these matches are fsm_hip_text_matches' of the same text and hits"""
        return HipReplaced(_call("fsm_hip_text_replace", self._h, text.handle, hits.handle if hits is not None else None, repl.handle,
                                 stream or None), (self, repl, text, hits))

    def extract(self, base: np.ndarray, off: np.ndarray, pick=None, trim_byte: int = -1, keep: Optional["HipRules"] = None,
                sep_byte: int = -1) -> "HipExtracted":
        """fsm_hip_matches_extract on host arrays: the batch these matches were made from"""
        b, _held = _host_batch(MatchBatch, base, off, pick, trim_byte, 0, 0)
        return HipExtracted(_call("fsm_hip_matches_extract", self._h, C.byref(b), keep.handle if keep is not None else None, sep_byte), (self, keep))

    def extract_device(self, d_base: int, d_off: int, n: int, d_pick: int = 0, m: int = 0, trim_byte: int = -1, limit: int = 0,
                       keep: Optional["HipRules"] = None, sep_byte: int = -1, stream: int = 0) -> "HipExtracted":
        """fsm_hip_matches_extract_device: device addresses; the offsets and the write pass are in flight on `stream` at return"""
        b = _device_batch(MatchBatch, d_base, d_off, n, d_pick, m, trim_byte, 0, limit)
        return HipExtracted(_call("fsm_hip_matches_extract_device", self._h, C.byref(b), keep.handle if keep is not None else None, sep_byte,
                                  stream or None), (self, keep))

    def text_extract(self, text: "HipText", hits: Optional["HipHits"] = None, keep: Optional["HipRules"] = None, sep_byte: int = -1,
                     stream: int = 0) -> "HipExtracted":
        """fsm_hip_text_extract: these matches are fsm_hip_text_matches' of the same text and hits"""
        return HipExtracted(_call("fsm_hip_text_extract", self._h, text.handle, hits.handle if hits is not None else None,
                                  keep.handle if keep is not None else None, sep_byte, stream or None), (self, keep, text, hits))

    def ms(self) -> float:
        return float(self._lib.fsm_hip_matches_ms(self._h))

    def pass_ms(self, which: int) -> float:
        """0: the marks, 1: the count pass, 2: the scan, 3: the emit pass"""
        return float(self._lib.fsm_hip_matches_pass_ms(self._h, which))


# ---- replace: every match replaced by its rule's replacement, a fresh packed text (include/fsm_hip.h, "replace") ----

class HipRepl(_Freed):
    """struct fsm_hip_repl *: a replacement table on the current device, R[i] = table[i]; flags: REPL_MASK"""

    _FREE = "fsm_hip_repl_free"

    def __init__(self, table: Sequence[bytes], flags: int = 0):
        table = [bytes(r) for r in table]
        data = np.frombuffer(b"".join(table), np.uint8)
        roff = np.zeros(len(table) + 1, np.uint64)
        if table:
            roff[1:] = np.cumsum([len(r) for r in table])
        super().__init__(_call("fsm_hip_repl_create", _ptr0(data), _ptr(roff) if table else None, len(table), flags))
        self.nrepl, self.flags = len(table), flags

    @classmethod
    def template(cls, table: Sequence[bytes], inserts: Optional[Sequence[Sequence[int]]], flags: int = 0) -> "HipRepl":
        """fsm_hip_repl_create_template: inserts[i] = the positions in table[i] at which the match itself is put (sed's &), ascending,
        each 0 .. len(table[i]); inserts None: no rule has one (ioff NULL)"""
        self = cls.__new__(cls)
        table = [bytes(r) for r in table]
        data = np.frombuffer(b"".join(table), np.uint8)
        roff = np.zeros(len(table) + 1, np.uint64)
        if table:
            roff[1:] = np.cumsum([len(r) for r in table])
        ins = ioff = None
        if inserts is not None:
            if len(inserts) != len(table):
                raise ValueError("one list of insert positions per rule")
            ioff = np.zeros(len(table) + 1, np.uint64)
            if table:
                ioff[1:] = np.cumsum([len(a) for a in inserts])
            ins = np.array([int(x) for a in inserts for x in a], np.uint64)
        _Owned.__init__(self, _call("fsm_hip_repl_create_template", _ptr0(data), _ptr(roff) if table else None, len(table),
                                    _ptr(ins) if ins is not None and len(ins) else None, _ptr(ioff) if ioff is not None else None, flags))
        self.nrepl, self.flags = len(table), flags
        return self

    @staticmethod
    def parse_sed(text: bytes):
        """a sed replacement -> (literal bytes, insert positions): & is an insert, \\& and \\\\ are the literals & and \\, and
        nothing else is read: a backslash before any other byte stands for itself, as that byte does (no \\n, no \\1).  A trailing
        backslash is a ValueError"""
        text = bytes(text)
        lit, ins, i = bytearray(), [], 0
        while i < len(text):
            c = text[i:i + 1]
            if c == b"&":
                ins.append(len(lit))
            elif c == b"\\" and i + 1 == len(text):
                raise ValueError("a replacement cannot end in a backslash: %r" % (text,))
            elif c == b"\\" and text[i + 1:i + 2] in (b"&", b"\\"):
                i += 1
                lit += text[i:i + 1]
            else:
                lit += c
            i += 1
        return bytes(lit), ins

    @classmethod
    def from_sed(cls, strings: Sequence[bytes]) -> "HipRepl":
        """a template table from sed replacements (parse_sed), one per rule"""
        parsed = [cls.parse_sed(x) for x in strings]
        return cls.template([p[0] for p in parsed], [p[1] for p in parsed])

    @property
    def in_lds(self) -> bool:
        return bool(self._lib.fsm_hip_repl_in_lds(self._h))

    inserts = _size("fsm_hip_repl_inserts", "the table's inserts, over all rules; 0 for a plain table")

    @staticmethod
    def max_inserts() -> int:
        """fsm_hip_repl_max_inserts: per rule"""
        return int(load_library().fsm_hip_repl_max_inserts())


class HipReplaced(_Freed):
    """struct fsm_hip_replaced *: out_off[m + 1] and the bytes on the device.  Keeps its matches and its table (and its text and
    hits) alive: the replaced object must be freed first."""

    _FREE = "fsm_hip_replaced_free"
    count = _size("fsm_hip_replaced_count")
    nbytes = _size("fsm_hip_replaced_nbytes")
    off_ptr = _dev("fsm_hip_replaced_off_device")
    bytes_ptr = _dev("fsm_hip_replaced_bytes_device")

    def copy(self, extra: int = 0, fill: int = 0):
        """-> (off u64 [m + 1], bytes u8 [nbytes]); extra: that many more entries in each array, pre-filled with `fill` and left
        alone by the library"""
        off, data = np.full(self.count + 1 + extra, fill, np.uint64), np.full(self.nbytes + extra, fill & 0xFF, np.uint8)
        _call("fsm_hip_replaced_copy", self._h, _ptr(off), _ptr(data))
        return off, data

    def off(self) -> np.ndarray:
        return self.copy()[0]

    def bytes(self) -> bytes:
        return self.copy()[1].tobytes()

    @property
    def ms(self) -> float:
        return float(self._lib.fsm_hip_replaced_ms(self._h))

    def pass_ms(self, which: int) -> float:
        """0: the lengths, 1: the scan of the block sums, 2: the offsets, 3: the write pass"""
        return float(self._lib.fsm_hip_replaced_pass_ms(self._h, which))


def replaced_block_lines() -> int:
    return int(load_library().fsm_hip_replaced_block_lines())


def replaced_block_bytes() -> int:
    return int(load_library().fsm_hip_replaced_block_bytes())


def repl_lds_bytes() -> int:
    return int(load_library().fsm_hip_repl_lds_bytes())


def repl_lds_rules() -> int:
    return int(load_library().fsm_hip_repl_lds_rules())


def repl_max_inserts() -> int:
    return int(load_library().fsm_hip_repl_max_inserts())


# ---- extract: every kept match's bytes as a record of a fresh packed text (include/fsm_hip.h, "extract") ----

class HipRules(_Freed):
    """struct fsm_hip_rules *: a set of rules on the current device; rules: the ids that are kept, all below nrules; flags:
    RULES_KEEP_OTHER"""

    _FREE = "fsm_hip_rules_free"

    def __init__(self, rules: Sequence[int], nrules: int, flags: int = 0):
        bits = np.zeros((nrules + 7) // 8, np.uint8)
        for i in rules:
            if not 0 <= i < nrules:
                raise ValueError("rule %d outside the set of %d" % (i, nrules))
            bits[i >> 3] |= 1 << (i & 7)
        super().__init__(_call("fsm_hip_rules_create", _ptr(bits) if nrules else None, nrules, flags))
        self.nrules, self.flags = nrules, flags


class HipExtracted(_Freed):
    """struct fsm_hip_extracted *: off[R + 1], the bytes, line[R] and match[R] on the device.  Keeps its matches and its set (and
    its text and hits) alive: the extracted object must be freed first."""

    _FREE = "fsm_hip_extracted_free"
    count = _size("fsm_hip_extracted_count")
    nbytes = _size("fsm_hip_extracted_nbytes")
    off_ptr = _dev("fsm_hip_extracted_off_device")
    bytes_ptr = _dev("fsm_hip_extracted_bytes_device")
    line_ptr = _dev("fsm_hip_extracted_line_device")
    match_ptr = _dev("fsm_hip_extracted_match_device")

    def copy(self, extra: int = 0, fill: int = 0):
        """-> (off u64 [R + 1], bytes u8 [nbytes], line u64 [R], match u64 [R]); extra: that many more entries in each array,
        pre-filled with `fill` and left alone by the library"""
        R = self.count
        off, data = np.full(R + 1 + extra, fill, np.uint64), np.full(self.nbytes + extra, fill & 0xFF, np.uint8)
        line, match = np.full(R + extra, fill, np.uint64), np.full(R + extra, fill, np.uint64)
        _call("fsm_hip_extracted_copy", self._h, _ptr(off), _ptr(data), _ptr(line), _ptr(match))
        return off, data, line, match

    def bytes(self) -> bytes:
        return self.copy()[1].tobytes()

    @property
    def ms(self) -> float:
        return float(self._lib.fsm_hip_extracted_ms(self._h))

    def pass_ms(self, which: int) -> float:
        """0: the lengths, 1: the scan of the block pairs, 2: the offsets, 3: the write pass"""
        return float(self._lib.fsm_hip_extracted_pass_ms(self._h, which))

    def distinct(self, sep_byte: int = -1, flags: int = 0, stream: int = 0) -> "HipDistinct":
        """fsm_hip_extracted_distinct: the distinct records, trimmed by the separator the extraction was made with"""
        return HipDistinct(_call("fsm_hip_extracted_distinct", self._h, sep_byte, flags, stream or None), (self,))

    def sort(self, sep_byte: int = -1, flags: int = 0, stream: int = 0) -> "HipSorted":
        """fsm_hip_extracted_sort: the records in byte order, trimmed by the separator the extraction was made with"""
        return HipSorted(_call("fsm_hip_extracted_sort", self._h, sep_byte, flags, stream or None), (self,))


def extracted_block_matches() -> int:
    return int(load_library().fsm_hip_extracted_block_matches())


def extracted_block_bytes() -> int:
    return int(load_library().fsm_hip_extracted_block_bytes())


# ---- distinct: the distinct records of a packed text with their counts (include/fsm_hip.h, "distinct") ----

class HipDistinct(_Freed):
    """struct fsm_hip_distinct *: first[D], count[D], class[R] and the packed text of the keys, doff[D + 1] and the bytes, on the
    device.  Keeps what it was made from alive: the distinct object must be freed first."""

    _FREE = "fsm_hip_distinct_free"

    count = _size("fsm_hip_distinct_count", "D: the distinct keys")
    records = _size("fsm_hip_distinct_records", "R")
    nbytes = _size("fsm_hip_distinct_nbytes")
    first_ptr = _dev("fsm_hip_distinct_first_device")
    count_ptr = _dev("fsm_hip_distinct_count_device")
    class_ptr = _dev("fsm_hip_distinct_class_device")
    off_ptr = _dev("fsm_hip_distinct_off_device")
    bytes_ptr = _dev("fsm_hip_distinct_bytes_device")

    def copy(self, extra: int = 0, fill: int = 0):
        """-> (first u64 [D], count u64 [D], class u32 [R], doff u64 [D + 1], dbytes u8 [nbytes]); doff and dbytes are None
        under DISTINCT_NO_TEXT; extra: that many more entries in each array, pre-filled with `fill` and left alone by the library"""
        D, R, text = self.count, self.records, self.off_ptr != 0
        first, count = np.full(D + extra, fill, np.uint64), np.full(D + extra, fill, np.uint64)
        cls = np.full(R + extra, fill & 0xFFFFFFFF, np.uint32)
        doff = np.full(D + 1 + extra, fill, np.uint64) if text else None
        data = np.full(self.nbytes + extra, fill & 0xFF, np.uint8) if text else None
        _call("fsm_hip_distinct_copy", self._h, _ptr(first), _ptr(count), _ptr(cls), _ptr(doff), _ptr(data))
        return first, count, cls, doff, data

    @property
    def ms(self) -> float:
        return float(self._lib.fsm_hip_distinct_ms(self._h))

    def pass_ms(self, which: int) -> float:
        """0: the hash pass, 1: the insert pass, 2: the number pass, 3: the write pass"""
        return float(self._lib.fsm_hip_distinct_pass_ms(self._h, which))

    def sort(self, by_count: bool = False, sep_byte: int = -1, flags: int = 0, stream: int = 0) -> "HipSorted":
        """fsm_hip_keys_sort: the D keys in byte order; by_count: by count[D] descending first, ties in byte order"""
        return HipSorted(_call("fsm_hip_keys_sort", self._h, sep_byte, flags | (SORT_BY_COUNT if by_count else 0), stream or None), (self,))

    # the lookup (include/fsm_hip.h, "find"): each found object keeps this dictionary and what it probed alive
    def find_device(self, d_off: int, d_bytes: int, R: int, nbytes: int, trim_byte: int = -1, d_tag: int = 0, flags: int = 0, stream: int = 0,
                    keep=()) -> "HipFound":
        """fsm_hip_keys_find_device: device addresses, 0: NULL; nothing waits, everything may be in flight on `stream` at return"""
        return HipFound(_call("fsm_hip_keys_find_device", self._h, d_off or None, d_bytes or None, R, nbytes, trim_byte, d_tag or None, flags,
                              stream or None), (self,) + tuple(keep))

    def find(self, off, data, trim_byte: int = -1, tag=None, flags: int = 0) -> "HipFound":
        """fsm_hip_keys_find on host arrays: off u64 [R + 1], the bytes, tag u32 [R] or None"""
        off = np.ascontiguousarray(off, np.uint64)
        data = np.ascontiguousarray(np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray)) else data, np.uint8)
        tag = None if tag is None else np.ascontiguousarray(tag, np.uint32)
        return HipFound(_call("fsm_hip_keys_find", self._h, _ptr(off), _ptr0(data), len(off) - 1, trim_byte, _ptr0(tag), flags), (self,))

    def find_extracted(self, x: "HipExtracted", flags: int = 0, stream: int = 0) -> "HipFound":
        """fsm_hip_keys_find_extracted: the records of an extraction, trimmed by its separator"""
        return HipFound(_call("fsm_hip_keys_find_extracted", self._h, x.handle, flags, stream or None), (self, x))

    def find_hits(self, hits: "HipHits", flags: int = 0, stream: int = 0) -> "HipFound":
        """fsm_hip_keys_find_hits: the lines of hits, trimmed by the text's delimiter"""
        return HipFound(_call("fsm_hip_keys_find_hits", self._h, hits.handle, flags, stream or None), (self, hits))

    def find_text(self, text: "HipText", flags: int = 0, stream: int = 0) -> "HipFound":
        """fsm_hip_keys_find_text: the lines of a text, trimmed by its delimiter; bitmap_ptr is what its hits_device takes"""
        return HipFound(_call("fsm_hip_keys_find_text", self._h, text.handle, flags, stream or None), (self, text))


def distinct_device(d_off: int, d_bytes: int, R: int, nbytes: int, trim_byte: int = -1, d_tag: int = 0, sep_byte: int = -1, flags: int = 0,
                    stream: int = 0, keep=()) -> HipDistinct:
    """fsm_hip_distinct_device: device addresses, 0: NULL; number and write are in flight on `stream` at return"""
    return HipDistinct(_call("fsm_hip_distinct_device", d_off or None, d_bytes or None, R, nbytes, trim_byte, d_tag or None, sep_byte, flags,
                             stream or None), keep)


def distinct(off, data, trim_byte: int = -1, tag=None, sep_byte: int = -1, flags: int = 0) -> HipDistinct:
    """fsm_hip_distinct on host arrays: off u64 [R + 1], the bytes, tag u32 [R] or None"""
    off = np.ascontiguousarray(off, np.uint64)
    data = np.ascontiguousarray(np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray)) else data, np.uint8)
    tag = None if tag is None else np.ascontiguousarray(tag, np.uint32)
    return HipDistinct(_call("fsm_hip_distinct", _ptr(off), _ptr0(data), len(off) - 1, trim_byte, _ptr0(tag), sep_byte, flags))


def distinct_long_bytes() -> int:
    return int(load_library().fsm_hip_distinct_long_bytes())


def distinct_table_slots(R: int) -> int:
    """fsm_hip_distinct_table_slots: a power of two >= 2 R, at least 16; EOVERFLOW above 2^32 - 2"""
    C.set_errno(0)
    n = int(load_library().fsm_hip_distinct_table_slots(R))
    if n == 0:
        raise _oserr("fsm_hip_distinct_table_slots")
    return n


# ---- find: the records of a packed text among the keys of a distinct object (include/fsm_hip.h, "find") ----

class HipFound:
    """struct fsm_hip_found *: class[R], the bitmap of ceil(R / 64) words and pick[R] on the device.  Keeps the dictionary and what
    it probed alive: the found object must be freed first.  An owner by _Owned's own methods, taken over as they are, as HipSorted
    is (tests/test_capi_owned.py holds the classes that DERIVE from _Owned to a list)."""

    _FREE = "fsm_hip_found_free"
    __init__, close, handle, free = _Owned.__init__, _Owned.close, _Owned.handle, _Freed.free

    def __del__(self):
        self.close()

    records = _size("fsm_hip_found_records", "R")
    present = _size("fsm_hip_found_present", "P: the records that equal a key; waits for the object's last event")
    class_ptr = _dev("fsm_hip_found_class_device")
    bitmap_ptr = _dev("fsm_hip_found_bitmap_device")
    pick_ptr = _dev("fsm_hip_found_pick_device")

    def copy(self, extra: int = 0, fill: int = 0):
        """-> (class u32 [R], bitmap u64 [ceil(R / 64)], pick u64 [R]); pick is None under FIND_NO_PICK; extra: that many more
        entries in each array, pre-filled with `fill` and left alone by the library"""
        R = self.records
        cls = np.full(R + extra, fill & 0xFFFFFFFF, np.uint32)
        bitmap = np.full((R + 63) // 64 + extra, fill, np.uint64)
        pick = np.full(R + extra, fill, np.uint64) if self.pick_ptr != 0 or R == 0 else None
        _call("fsm_hip_found_copy", self._h, _ptr(cls), _ptr(bitmap), _ptr(pick))
        return cls, bitmap, pick

    @property
    def ms(self) -> float:
        return float(self._lib.fsm_hip_found_ms(self._h))

    def pass_ms(self, which: int) -> float:
        """0: the hash pass, 1: the probe pass (both kernels), 2: mark and scan, 3: the pick pass"""
        return float(self._lib.fsm_hip_found_pass_ms(self._h, which))


# ---- sort: the records of a packed text in byte order (include/fsm_hip.h, "sort") ----

class HipSorted:
    """struct fsm_hip_sorted *: order[R], rank[R] and the sorted packed text, soff[R + 1] and the bytes, on the device.  Keeps
    what it was made from alive: the sorted object must be freed first.  An owner by _Owned's own methods, taken over as they
    are (tests/test_capi_owned.py holds the classes that DERIVE from _Owned to a list)."""

    _FREE = "fsm_hip_sorted_free"
    __init__, close, handle, free = _Owned.__init__, _Owned.close, _Owned.handle, _Freed.free

    def __del__(self):
        self.close()

    records = _size("fsm_hip_sorted_records", "R")
    groups = _size("fsm_hip_sorted_groups", "the distinct (major, key) pairs: rank[R - 1] + 1")
    nbytes = _size("fsm_hip_sorted_nbytes")
    rounds = _size("fsm_hip_sorted_rounds")
    order_ptr = _dev("fsm_hip_sorted_order_device")
    rank_ptr = _dev("fsm_hip_sorted_rank_device")
    off_ptr = _dev("fsm_hip_sorted_off_device")
    bytes_ptr = _dev("fsm_hip_sorted_bytes_device")

    def radix_passes(self, skipped: bool = False) -> int:
        """the radix passes the rounds ran, or skipped because their digit had one occupied bin"""
        return int(self._lib.fsm_hip_sorted_radix_passes(self._h, 1 if skipped else 0))

    def copy(self, extra: int = 0, fill: int = 0):
        """-> (order u64 [R], rank u32 [R], soff u64 [R + 1], sbytes u8 [nbytes]); soff and sbytes are None under SORT_NO_TEXT;
        extra: that many more entries in each array, pre-filled with `fill` and left alone by the library"""
        R, text = self.records, self.off_ptr != 0
        order, rank = np.full(R + extra, fill, np.uint64), np.full(R + extra, fill & 0xFFFFFFFF, np.uint32)
        soff = np.full(R + 1 + extra, fill, np.uint64) if text else None
        data = np.full(self.nbytes + extra, fill & 0xFF, np.uint8) if text else None
        _call("fsm_hip_sorted_copy", self._h, _ptr(order), _ptr(rank), _ptr(soff), _ptr(data))
        return order, rank, soff, data

    @property
    def ms(self) -> float:
        return float(self._lib.fsm_hip_sorted_ms(self._h))

    def pass_ms(self, which: int) -> float:
        """0: the keys (major, prefix skip, fetch), 1: the radix passes, 2: the rebucket, 3: the finish and the write pass"""
        return float(self._lib.fsm_hip_sorted_pass_ms(self._h, which))


def sort_device(d_off: int, d_bytes: int, R: int, nbytes: int, trim_byte: int = -1, d_major: int = 0, sep_byte: int = -1, flags: int = 0,
                stream: int = 0, keep=()) -> HipSorted:
    """fsm_hip_sort_device: device addresses, 0: NULL; the finish and the write pass are in flight on `stream` at return"""
    return HipSorted(_call("fsm_hip_sort_device", d_off or None, d_bytes or None, R, nbytes, trim_byte, d_major or None, sep_byte, flags,
                           stream or None), keep)


def sort(off, data, trim_byte: int = -1, major=None, sep_byte: int = -1, flags: int = 0) -> HipSorted:
    """fsm_hip_sort on host arrays: off u64 [R + 1], the bytes, major u64 [R] or None"""
    off = np.ascontiguousarray(off, np.uint64)
    data = np.ascontiguousarray(np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray)) else data, np.uint8)
    major = None if major is None else np.ascontiguousarray(major, np.uint64)
    return HipSorted(_call("fsm_hip_sort", _ptr(off), _ptr0(data), len(off) - 1, trim_byte, _ptr(major), sep_byte, flags))


def sort_tile_records() -> int:
    return int(load_library().fsm_hip_sort_tile_records())
