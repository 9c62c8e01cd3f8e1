"""CPU: the upper bounds mm_ba_index_build's callers allocate the segment and chunk tables at (no compute calls)."""
import ctypes as C


def bounds(F, span, n_pairs, chunk):
    from meatmodeler_amd import _lib      # (inside the tests, as in test_abi.py: not while the suite is being collected)
    seg, chunks = C.c_int64(-1), C.c_int64(-1)
    assert _lib.lib.mm_ba_index_bounds(F, span, n_pairs, chunk, C.byref(seg), C.byref(chunks)) == 0
    return seg.value, chunks.value


def test_segment_and_chunk_bounds():
    # bench shape: 500 cameras, span 87 -> 44000 keys, far fewer than pairs
    assert bounds(500, 87, 7040014, 512) == (44000, 44000 + 7040014 // 512)
    # fewer pairs than keys: a segment per pair at most
    assert bounds(500, 87, 100, 64) == (100, 101)
    assert bounds(2, 1, 1800, 64) == (4, 4 + 28)
    assert bounds(1, 0, 0, 64) == (0, 0)
    # the key count does not wrap in 32 bits
    assert bounds(2 ** 30, 3, 2 ** 40, 512)[0] == 2 ** 32


def test_chunk_bound_covers_the_worst_split():
    # n_seg segments of c_i pairs need sum ceil(c_i / chunk) chunks: at most n_seg + floor(sum c_i / chunk)
    for counts in ([600, 600, 600], [1] * 7, [64, 63, 65], [511, 513, 1]):
        for chunk in (64, 512):
            need = sum(-(-c // chunk) for c in counts)
            seg_cap, chunk_cap = bounds(len(counts), 0, sum(counts), chunk)
            assert seg_cap == len(counts) and need <= chunk_cap


def test_bad_arguments_and_no_device():
    from meatmodeler_amd import _lib
    seg, chunks = C.c_int64(0), C.c_int64(0)
    assert _lib.lib.mm_ba_index_bounds(0, 0, 1, 64, C.byref(seg), C.byref(chunks)) != 0
    assert _lib.lib.mm_ba_index_bounds(4, 0, 1, 0, C.byref(seg), C.byref(chunks)) != 0
    ix = _lib.BAIndex()
    assert _lib.lib.mm_ba_index_workspace_bytes(None, C.byref(ix), 0) == 0      # (no context: no size)
