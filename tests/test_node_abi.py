"""CPU: the multi-device front (libfsm_amd/csrc/node.hip) is exported by libfsm_hip.so, wrapped by HipNode, refuses bad
arguments before touching a device, and answers the shard queries for a NULL node as include/fsm_hip.h says.  The shard
rule of the header is restated here in plain Python (shard_rule); tests/test_gpu_node_front.py holds fsm_hip_node_shard
equal to it for every batch size and replica count it runs."""
import ctypes as C
import errno as _errno

import pytest

SYMBOLS = ("fsm_hip_node_create", "fsm_hip_node_free", "fsm_hip_node_ndev", "fsm_hip_node_dfa", "fsm_hip_node_shard", "fsm_hip_node_uses_rccl",
           "fsm_hip_node_rccl_path", "fsm_hip_node_bitmap_words", "fsm_hip_node_exec_batch", "fsm_hip_node_exec_batch_offsets",
           "fsm_hip_node_exec_batch_offsets32", "fsm_hip_node_exec_batch_lengths", "fsm_hip_node_exec_batch_device", "fsm_hip_node_exec_device",
           "fsm_hip_node_wait", "fsm_hip_node_exec_batch_ids", "fsm_hip_node_exec_batch_eager", "fsm_hip_node_exec_multi")
WRAPPERS = ("close", "uses_rccl", "rccl_path", "replica", "shard", "bitmap_words", "exec_batch", "exec_batch_offsets", "exec_batch_offsets32",
            "exec_batch_lengths", "exec_strings", "exec_batch_device", "exec_device", "wait", "exec_batch_ids", "exec_batch_eager")


def shard_rule(n: int, G: int, k: int):
    """include/fsm_hip.h: shard k = inputs [k * per, min(n, (k + 1) * per)) with per = 64 * ceil(ceil(n / 64) / G); an
    empty shard starts at n.  -> (first, count)"""
    per = 64 * -(-(-(-n // 64)) // G)
    first = min(k * per, n)
    return first, min(per, n - first)


def bitmap_words_rule(n: int, G: int) -> int:
    """words of the whole-batch bitmap every replica holds: G slices of per / 64 words"""
    return G * -(-(-(-n // 64)) // G)


@pytest.fixture(scope="module")
def lib(built):
    import libfsm_amd
    return libfsm_amd.load_library()


def test_symbols_and_wrappers_exist(lib):
    import libfsm_amd
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing
    missing = [m for m in WRAPPERS if not callable(getattr(libfsm_amd.HipNode, m, None))]
    assert not missing, missing


def test_shard_rule_partitions_in_whole_words():
    for G in (1, 2, 3, 5, 8):
        for n in (0, 1, 63, 64, 65, 64 * (G - 1), 64 * (G - 1) + 1, 64 * G - 1, 64 * G, 64 * G + 1, 128 * G + 1, 10_007):
            cover = 0
            for k in range(G):
                f, c = shard_rule(n, G, k)
                assert f == cover and (f % 64 == 0 or c == 0) and (c % 64 == 0 or f + c == n), (G, n, k)
                cover += c
            assert cover == n and bitmap_words_rule(n, G) * 64 >= n and bitmap_words_rule(n, G) % G == 0
    assert [shard_rule(65, 3, k) for k in range(3)] == [(0, 64), (64, 1), (65, 0)]
    assert [shard_rule(129, 2, k) for k in range(2)] == [(0, 128), (128, 1)]


def test_null_arguments_are_einval_without_a_device(lib):
    sz, vp = C.c_size_t, C.c_void_p
    buf = C.create_string_buffer(64)
    u32 = (C.c_uint32 * 4)(0, 1, 2, 3)
    u64 = (C.c_uint64 * 4)(0, 1, 2, 3)
    out32 = (C.c_uint32 * 4)()
    out64 = (C.c_uint64 * 4)()
    ptrs = (vp * 1)(C.addressof(buf))
    batch = C.create_string_buffer(128)          # a zeroed struct fsm_hip_node_batch
    # never dereferenced: node.hip tests `eager_out == nullptr` / `id_out == nullptr` in the same condition as `nd == nullptr`,
    # before the node is touched (the first line of fsm_hip_node_exec_batch_eager / _ids)
    fake = C.create_string_buffer(4096)
    calls = {
        "exec_batch": lambda: lib.fsm_hip_node_exec_batch(None, buf, sz(16), None, sz(1), out32, out64),
        "exec_batch_offsets": lambda: lib.fsm_hip_node_exec_batch_offsets(None, buf, u64, sz(1), out32, out64),
        "exec_batch_offsets32": lambda: lib.fsm_hip_node_exec_batch_offsets32(None, buf, u32, sz(1), out32, out64),
        "exec_batch_lengths": lambda: lib.fsm_hip_node_exec_batch_lengths(None, buf, u32, sz(1), out32, out64),
        "exec_batch_device": lambda: lib.fsm_hip_node_exec_batch_device(None, ptrs, sz(16), sz(1), None, None, None),
        "exec_device": lambda: lib.fsm_hip_node_exec_device(None, batch, sz(1), None, C.c_int(0)),
        "exec_batch_ids": lambda: lib.fsm_hip_node_exec_batch_ids(None, buf, sz(16), None, sz(1), C.c_int(1), out32),
        "exec_batch_eager": lambda: lib.fsm_hip_node_exec_batch_eager(None, buf, sz(16), None, sz(1), out32, out64),
        "exec_multi (NULL nodes)": lambda: lib.fsm_hip_node_exec_multi(None, batch, sz(1)),
        "exec_batch_eager (NULL eager_out)": lambda: lib.fsm_hip_node_exec_batch_eager(fake, buf, sz(16), None, sz(1), out32, None),
        "exec_batch_ids (NULL id_out)": lambda: lib.fsm_hip_node_exec_batch_ids(fake, buf, sz(16), None, sz(1), C.c_int(1), None),
        "wait": lambda: lib.fsm_hip_node_wait(None, None),
    }
    for name, call in calls.items():
        C.set_errno(0)
        assert call() == -1, name
        assert C.get_errno() == _errno.EINVAL, name
    assert list(out32) == [0] * 4 and list(out64) == [0] * 4


def test_null_node_shard_queries(lib):
    f, c = C.c_size_t(7), C.c_size_t(7)
    lib.fsm_hip_node_shard(None, C.c_size_t(1000), C.c_int(0), C.byref(f), C.byref(c))
    assert (f.value, c.value) == (0, 0)
    assert lib.fsm_hip_node_bitmap_words(None, C.c_size_t(1000)) == 0
    assert lib.fsm_hip_node_ndev(None) == 0
