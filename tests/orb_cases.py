"""Designed frames for the ORB detect tests (tests/test_orb_detect_cpu.py, tests/test_orb_detect_gpu.py): pure NumPy, seeded.

Rendered frames are corner-rich and free of ties; these are built so that a named edge of csrc/orb.hip is in the input.
The CPU file asserts from the oracle alone that each edge is there; the GPU file compares the kernels with the oracle on the
same bytes.  Nothing here touches a device.
"""
import functools

import numpy as np

from meatmodeler_amd.orb_pattern import brief_pattern
from oracle import orb_oracle as oo

EDGE = 31           # key points keep 31 pixels from the border of their level
H0, W0 = 259, 331   # the common frame: W % 4 == 3, a lattice dot exactly at x = W0 - 32 and at y = H0 - 32
SEED = 7


def dots(H=H0, W=W0):
    """Black frame with a white pixel every 4 pixels from (31, 31): every dot is a FAST corner with one and the same score,
    and all dots away from the border share one Harris value."""
    img = np.zeros((H, W), np.uint8)
    img[EDGE::4, EDGE::4] = 255
    return img


def dots_admissible(H=H0, W=W0):
    """(x, y) of the lattice dots that lie inside the 31-pixel border, counted from the construction alone."""
    xs = [x for x in range(EDGE, W, 4) if x <= W - EDGE - 1]
    ys = [y for y in range(EDGE, H, 4) if y <= H - EDGE - 1]
    return xs, ys


def noise(H=H0, W=W0, seed=SEED):
    """Uniform random bytes: about one pixel in ten survives the NMS, on every tile seam and border line."""
    return np.random.default_rng(seed).integers(0, 256, (H, W), dtype=np.uint8)


def periodic(H=H0, W=W0, seed=SEED):
    """A 32 x 32 random tile repeated: equal scores AND equal Harris values at distinct positions, one per period, with
    descriptors that are not trivial."""
    tile = np.random.default_rng(seed + 1000).integers(0, 256, (32, 32), dtype=np.uint8)
    return np.ascontiguousarray(np.tile(tile, ((H + 31) // 32, (W + 31) // 32))[:H, :W])


def flat(H=H0, W=W0, value=90):
    return np.full((H, W), value, np.uint8)


BUILDERS = dict(dots=dots, noise=noise, periodic=periodic, flat=flat)


@functools.lru_cache(maxsize=None)
def frame(kind, H=H0, W=W0):
    img = BUILDERS[kind](H, W)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def reference(kind, H, W, nfeatures, nlevels=8, scale_factor=1.2, fast_threshold=20):
    """The oracle's result for a case: computed once per process, shared by every test that needs it, never written to."""
    r = oo.detect_compute(frame(kind, H, W), nfeatures, brief_pattern(), nlevels, scale_factor, fast_threshold)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def level_counts(r, nlevels=8):
    return np.bincount(r["meta"][:, 0], minlength=nlevels)
