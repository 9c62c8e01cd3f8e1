"""CPU: the designed ORB frames of tests/orb_cases.py contain the edges they were built for.

tests/test_orb_detect_gpu.py compares csrc/orb.hip with oracle/orb_oracle.c bit for bit on these frames.  That comparison
says nothing if, say, no two key points of a frame tie, so every property a GPU test relies on is asserted here from the
oracle alone (tests/test_oracle_definitions.py ties the oracle stage by stage to DESIGN.md's mm-ORB definition): ties across
the select cut and the rank cut, key points on the last admissible column and row and none beyond, complete survivor sets,
levels without a valid area, and the per-level budgets at tiny feature counts.  No device is needed.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import orb_cases as oc  # noqa: E402
from oracle import orb_oracle as oo  # noqa: E402

H, W = oc.H0, oc.W0
RK_MAX = 4096       # capacity of the sorting rank kernel (csrc/orb.hip): 2 * max(nfeat) + 8 above it -> the counting kernel


def level0(r):
    m = r["meta"]
    return m[m[:, 0] == 0]


def lattice_in_select_order():
    """The admissible dots as the select stage orders equal scores: (y asc, x asc)."""
    xs, ys = oc.dots_admissible()
    return [(x, y) for y in ys for x in xs]


def test_dots_lattice_by_construction():
    xs, ys = oc.dots_admissible()
    assert len(xs) * len(ys) == 3400
    assert xs[-1] == W - 32 == 299 and ys[-1] == H - 32 == 227          # the last admissible column and row carry dots
    img = oc.frame("dots")
    assert img[227, 303] == 255 and img[231, 299] == 255 and img[231, 303] == 255      # and the next ones must be rejected
    # every dot is a corner with one and the same FAST score, the image border included
    sc = oo.fast_score_map(img)
    assert len({int(sc[y, x]) for x, y in lattice_in_select_order()}) == 1 and sc[31, 31] > 0


def test_dots_500_select_cut_and_rank_cut_pass_through_ties():
    nf = oo.level_sizes(H, W, 500)[2]
    assert nf[0] == 109
    r = oc.reference("dots", H, W, 500)
    l0 = level0(r)
    assert len(l0) == nf[0]
    lat = lattice_in_select_order()
    assert len(lat) > 2 * nf[0]                                        # more planted than the select stage keeps ...
    sel = lat[:2 * nf[0]]                                              # ... all of one score: the cut is decided on (y, x)
    assert sel[-1][1] == lat[2 * nf[0]][1], "the select cut lies inside one row: it is decided on the x bits"
    # kept: one FAST score (all dots have one), one Harris value, and more candidates with that value than are kept
    assert np.unique(l0[:, 3]).size == 1 and np.unique(r["resp"][r["meta"][:, 0] == 0]).size == 1
    img = oc.frame("dots")
    hv = [oo.harris25_at(img, x, y) for x, y in sel]
    top = max(hv)
    tied = [p for p, v in zip(sel, hv) if v == top]
    assert (top & 0xFFFFFFFF) == (int(l0[0, 3]) & 0xFFFFFFFF)
    assert len(tied) > nf[0], "the rank cut must pass through equal Harris values"
    assert [tuple(p) for p in l0[:, 1:3]] == tied[:nf[0]]              # (H desc, y asc, x asc) among the tied


def test_dots_300_keeps_the_last_selected_candidate():
    """The 2n-th candidate in select order is itself selected (`key <= threshold`), and here it is among the kept."""
    nf = oo.level_sizes(H, W, 300)[2]
    lat = lattice_in_select_order()
    last = lat[2 * nf[0] - 1]
    l0 = level0(oc.reference("dots", H, W, 300))
    assert len(l0) == nf[0] == 65
    assert last in [tuple(p) for p in l0[:, 1:3]]
    assert lat[2 * nf[0]] not in [tuple(p) for p in l0[:, 1:3]]


def test_dots_30000_keeps_every_admissible_dot_and_nothing_beyond():
    nf = oo.level_sizes(H, W, 30000)[2]
    assert 2 * nf.max() + 8 > RK_MAX
    r = oc.reference("dots", H, W, 30000)
    l0 = level0(r)
    assert len(l0) == 3400 < nf[0]
    assert sorted(tuple(p) for p in l0[:, 1:3]) == sorted(lattice_in_select_order())
    assert l0[:, 1].max() == 299 and l0[:, 2].max() == 227 and l0[:, 1].min() == 31 and l0[:, 2].min() == 31
    assert not (l0[:, 1] > W - 32).any() and not (l0[:, 2] > H - 32).any()
    zero = (r["mom"] == 0).all(axis=1)
    assert zero.any() and (~zero).any()                                 # both branches of the steering (|m| == 0 and > 0)


def test_noise_30000_is_the_complete_survivor_set_on_borders_and_seams():
    nf = oo.level_sizes(H, W, 30000)[2]
    assert 2 * nf.max() + 8 > RK_MAX
    r = oc.reference("noise", H, W, 30000)
    cnt = oc.level_counts(r)
    assert (cnt < nf).all() and (cnt > 0).all()
    assert cnt[0] > RK_MAX                                              # the counting kernel's early-return blocks and > 16 that work
    l0 = level0(r)
    for x in (31, W - 32, 94, 95):                                      # 94 | 95: the seam between FAST tiles 0 and 1
        assert (l0[:, 1] == x).any(), x
    for y in (31, H - 32, 94, 95):
        assert (l0[:, 2] == y).any(), y
    assert 0.08 < cnt[0] / ((W - 62) * (H - 62)) < 0.12


def test_noise_150x200_9000_complete_on_the_sort_path_with_empty_levels():
    w, h, nf, _ = oo.level_sizes(150, 200, 9000)
    assert 2 * nf.max() + 8 <= RK_MAX
    r = oc.reference("noise", 150, 200, 9000)
    cnt = oc.level_counts(r)
    assert (cnt < nf).all()
    assert (h[5:] <= 62).all() and (h[:5] > 62).all() and (w[:5] > 62).all()
    assert (cnt[5:] == 0).all() and (cnt[:5] > 0).all()


def test_noise_and_periodic_fill_their_budgets_at_500_and_300():
    """C > 2n at level 0 (the radix select runs) while small levels have C <= 2n (its early exit)."""
    for nfeatures in (500, 300):
        nf = oo.level_sizes(H, W, nfeatures)[2]
        full = oc.level_counts(oc.reference("noise", H, W, 30000))     # all survivors per level
        assert full[0] > 2 * nf[0] and full[7] <= 2 * nf[7]
        for kind in ("noise", "periodic"):
            cnt = oc.level_counts(oc.reference(kind, H, W, nfeatures))
            assert (cnt[:6] == nf[:6]).all()


def test_periodic_has_equal_harris_values_at_distinct_positions():
    l0 = level0(oc.reference("periodic", H, W, 500))
    vals, counts = np.unique(l0[:, 3], return_counts=True)
    assert (counts > 1).any()
    v = vals[np.argmax(counts)]
    grp = l0[l0[:, 3] == v]
    assert len({tuple(p) for p in grp[:, 1:3]}) == len(grp) >= 2
    # the tied points are one period apart and their descriptors are not trivial
    assert ((grp[:, 1] - grp[0, 1]) % 32 == 0).all() and ((grp[:, 2] - grp[0, 2]) % 32 == 0).all()
    d = oc.reference("periodic", H, W, 500)["desc"]
    assert 64 < np.unpackbits(d, axis=1).sum(axis=1).mean() < 192


def test_small_feature_counts_leave_levels_without_budget():
    assert oo.level_sizes(H, W, 1)[2].tolist() == [0, 0, 0, 0, 0, 0, 0, 1]
    assert oo.level_sizes(H, W, 3)[2].tolist() == [1, 1, 0, 0, 0, 0, 0, 1]
    assert oc.level_counts(oc.reference("noise", H, W, 1)).tolist() == [0, 0, 0, 0, 0, 0, 0, 1]
    assert oc.level_counts(oc.reference("noise", H, W, 3)).tolist() == [1, 1, 0, 0, 0, 0, 0, 1]


def test_frames_without_a_valid_area():
    w, h, _, _ = oo.level_sizes(62, 64, 500)
    assert ((w <= 62) | (h <= 62)).all()
    assert oc.reference("dots", 62, 64, 500)["n"] == 0 and oc.reference("noise", 62, 64, 500)["n"] == 0
    r = oc.reference("dots", 63, 63, 500)
    assert r["n"] == 1 and r["meta"][0, :3].tolist() == [0, 31, 31]


def test_parameter_cases_reach_what_they_are_for():
    for nl in (1, 2, 5):
        r = oc.reference("noise", H, W, 400, nlevels=nl)
        assert r["n"] == 400 and set(r["meta"][:, 0]) == set(range(nl))
    r15 = oc.reference("noise", H, W, 400, scale_factor=1.5)
    w, h, nf, _ = oo.level_sizes(H, W, 400, 8, 1.5)
    assert oc.level_counts(r15)[:3].tolist() == nf[:3].tolist() and (oc.level_counts(r15)[4:] == 0).all() and h[4] <= 62
    r105 = oc.reference("noise", H, W, 400, scale_factor=1.05)
    assert oc.level_counts(r105).tolist() == oo.level_sizes(H, W, 400, 8, 1.05)[2].tolist()
    lo = oc.reference("noise", H, W, 400, fast_threshold=5)
    hi = oc.reference("noise", H, W, 400, fast_threshold=60)
    ref = oc.reference("noise", H, W, 400)
    assert hi["n"] < ref["n"] and oc.level_counts(hi)[0] == oc.level_counts(ref)[0]
    # the threshold matters to the output: it changes which pixels compete in the NMS
    assert not np.array_equal(lo["meta"][:50], ref["meta"][:50]) or lo["n"] != ref["n"]


def test_padded_width_cases_are_complete_and_reach_the_last_column():
    """Widths 331, 330, 329 (W % 4 = 3, 2, 1) at 30000 features: every survivor is kept, some on the last admissible column,
    and the periodic frame brings equal Harris values."""
    for width in (331, 330, 329):
        nf = oo.level_sizes(H, width, 30000)[2]
        for kind in ("noise", "periodic"):
            r = oc.reference(kind, H, width, 30000)
            assert (oc.level_counts(r) < nf).all()
            l0 = level0(r)
            assert (l0[:, 1] == width - 32).any() and not (l0[:, 1] > width - 32).any()
        assert (np.unique(l0[:, 3], return_counts=True)[1] > 1).any()


def test_flat_frame_has_no_key_points():
    assert oc.reference("flat", H, W, 500)["n"] == 0
