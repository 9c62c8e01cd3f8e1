"""CPU: host-side logic of the fixed-camera bundle adjustment (no GPU needed): the anchored window selection, the
fixed-frame renumbering and the C-ABI declarations."""
import os
import re

import numpy as np
import torch

from meatmodeler_amd import _lib
from meatmodeler_amd.bundleAdjuster import fixed_frame_order
from meatmodeler_amd.pipeline import ClipPipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_anchored(first, last, lo, hi, F):
    return np.array([lo <= last[t] < hi and (hi >= F or last[t] <= hi - 2) for t in range(len(first))], bool)


def test_window_selection_anchored_equals_a_plain_loop():
    rng = np.random.default_rng(0)
    for trial in range(40):
        F = int(rng.integers(2, 40))
        T = int(rng.integers(0, 200))
        first = rng.integers(0, F, T)
        last = np.minimum(first + rng.integers(1, 8, T), F - 1)
        W = int(rng.integers(2, F + 1))
        for hi in sorted({W, F, int(rng.integers(W, F + 1))}):
            lo = max(0, hi - W)
            want = _plain_anchored(first, last, lo, hi, F)
            got = ClipPipeline.window_selection_anchored(first, last, lo, hi, F)
            assert np.array_equal(np.asarray(got, bool), want)
            got_t = ClipPipeline.window_selection_anchored(torch.as_tensor(first), torch.as_tensor(last), lo, hi, F)
            assert np.array_equal(got_t.numpy(), want)
            if lo == 0:      # the first window selects what boundary="inside" selects
                assert np.array_equal(ClipPipeline.window_selection(first, last, lo, hi, F), want)


def test_fixed_frame_order_round_trip():
    rng = np.random.default_rng(1)
    for trial in range(50):
        F = int(rng.integers(1, 60))
        mask = rng.random(F) < rng.random()
        order, new_index, F_free = fixed_frame_order(mask, F)
        assert F_free == int((~mask).sum())
        assert np.array_equal(np.sort(order), np.arange(F))
        assert np.array_equal(new_index[order], np.arange(F)) and np.array_equal(order[new_index], np.arange(F))
        # free frames first in their own order, fixed frames after them, also in order
        assert np.array_equal(order[:F_free], np.flatnonzero(~mask))
        assert np.array_equal(order[F_free:], np.flatnonzero(mask))
        o2, n2, f2 = fixed_frame_order(np.flatnonzero(mask).tolist(), F)
        assert np.array_equal(o2, order) and np.array_equal(n2, new_index) and f2 == F_free


def test_fixed_camera_entry_points_are_declared():
    src = open(os.path.join(ROOT, "include", "meatmodeler.h")).read()
    assert re.search(r"typedef struct mm_ba_fixed \{", src)
    for name in ("mm_ba_residual_fixed", "mm_ba_normal_eq_fixed", "mm_ba_trf_fixed_workspace_bytes", "mm_ba_trf_fixed"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert [f[0] for f in _lib.BAFixed._fields_] == ["F_fixed", "reserved", "cams"]
    assert _lib.lib.mm_abi_version() == 3
