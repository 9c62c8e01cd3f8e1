"""CPU: how the Schur build carves its workspace (no compute calls)."""
import ctypes as C

import pytest


def up(x):
    return (x + 255) // 256 * 256


def size(F, n_seg, n_chunks):
    from meatmodeler_amd import _lib      # (inside the tests, as in test_abi.py: not while the suite is being collected)
    pb = _lib.BAProblem()
    pb.F, pb.n_seg, pb.n_chunks = F, n_seg, n_chunks
    return _lib.lib.mm_ba_schur_workspace_bytes(C.byref(pb))


@pytest.mark.parametrize("F,n_seg,n_chunks,total", [(160, 7, 9, 35072), (1, 1, 1, None), (500, 2500, 3000, None)])
def test_workspace_is_five_regions_each_rounded_up_to_256(F, n_seg, n_chunks, total):
    layout = (up(n_chunks * 42 * 8)      # partial sums of multi-chunk segments: 42 doubles per chunk
              + up(n_seg * 4)            # finished-chunk counters
              + up(2 * 64 * 4)           # slab flags, slab counters
              + up(F * 24 * 8)           # per-camera table: 24 doubles per camera
              + up(n_chunks * 32))       # per-chunk descriptors: 8 int32 per chunk
    assert total is None or layout == total
    assert size(F, n_seg, n_chunks) == layout


def test_no_chunks_or_no_problem_no_workspace():
    from meatmodeler_amd import _lib
    assert size(160, 7, 0) == 0
    assert _lib.lib.mm_ba_schur_workspace_bytes(None) == 0
