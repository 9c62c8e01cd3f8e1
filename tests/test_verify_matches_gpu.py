"""GPU: mm_verify_matches through ops.verify_matches, processor.verifyMatches and ClipPipeline.run(verify=...) against the
NumPy restatement of tests/test_verify_matches_cpu.py.

Shapes: n_pairs <= 5, cap = 320.  The five-pair call holds 160 + 96, 64 + 0, 40 + 24 and 17 + 0 (inliers + outliers) and a pair
of 15 matches (too few); the boundaries vary one thing at a time: m in {0, 15, 16, 17, 63, 64, 65, 257, cap}, n_hyp in
{1, 63, 64, 65, 256}, n_pairs in {0, 1, 3}, refit_iters in {0, 2}, threshold_px = +inf.

Exact: best_h, flags, n_inliers, the number of valid hypotheses, the mask and the kept rows.  The fixtures have no match
within 0.02 px of the threshold (asserted in the CPU file), so a mask or best_h mismatch is not rounding: it means F is off.
F (up to sign) and the cost (relative) against the restatement: started at 1e-9; the first run on the MI355X measured, over
every comparison of this file, 2.0e-14 on F (m = 17, after the refit) and 7.9e-13 on the cost (the 17-match pair of the
five-pair call) -- the two NumPy routes differ by 1.7e-14 among themselves.  The bounds are the measured gaps with a margin
of ten: 2.0e-13 and 7.9e-12.
"""
import functools
import math
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_verify_matches_cpu as ref  # noqa: E402
from meatmodeler_amd import ops, processor, synth  # noqa: E402
from meatmodeler_amd.pipeline import ClipPipeline  # noqa: E402

DEV = torch.device("cuda", 0)
CAP = ref.CAP
KW = ref.FIVE_KW
# Gap to the restatement (the kernel's fused multiply-adds, its Gram-Schmidt null vector and its Jacobi eigenvectors are a third
# route beside NumPy's two): measured 1.998e-14 on F up to sign and 7.837e-13 relative on the cost, x 10 (module docstring)
F_TOL = 2.0e-13
COST_TOL = 7.9e-12


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def run(kp, pairs, m, **kw):
    """-> (pairs_out, m_out, F, cost, info) as NumPy arrays."""
    return tuple(t.cpu().numpy() for t in ops.verify_matches(dev(kp), dev(pairs), dev(m), **kw))


WORST = dict(F=0.0, cost=0.0)


def check(got, want, pairs, m, what=""):
    """One call against the restatement's list of per-pair results."""
    po, mo, F, cost, info = got
    for p, r in enumerate(want):
        mm = int(m[p])
        assert tuple(info[p]) == (r["flags"], r["n_inliers"], r["best_h"], r["n_valid"]), (what, p, info[p], r)
        assert mo[p] == len(r["kept"]) and np.array_equal(po[p, :mo[p]], r["kept"]), (what, p)
        assert (po[p, mo[p]:] == -1).all(), (what, p)      # the sentinel ops.verify_matches fills the output with
        if not r["flags"] & (ref.TOO_FEW | ref.NO_MODEL | ref.WEAK):
            assert np.array_equal(po[p, :mo[p]], pairs[p, :mm][r["mask"]])      # the input rows under the mask, in order
        if r["best_h"] < 0:
            assert np.isnan(F[p]).all() and np.isnan(cost[p])
            continue
        assert abs(np.linalg.norm(F[p]) - 1.0) < 1e-12
        gF = ref.sign_gap(F[p], r["F"])
        gc = abs(cost[p] - r["cost"]) / r["cost"]
        WORST["F"], WORST["cost"] = max(WORST["F"], gF), max(WORST["cost"], gc)
        print(f"{what} pair {p}: |F - F_numpy| = {gF:.3e}, cost gap {gc:.3e} (worst so far {WORST['F']:.3e}, {WORST['cost']:.3e})")
        assert gF <= F_TOL and gc <= COST_TOL, (what, p, gF, gc)


@functools.lru_cache(maxsize=None)
def five():
    """The five-pair call: (kp, pairs, m), the restatement's results and the kernel's outputs (computed once, never changed)."""
    _, kp, pairs, m = ref.five_pairs()
    return kp, pairs, m, ref.five_pairs_result(), run(kp, pairs, m, **KW)


# ------------------------------------------------------------------------------------------------ against the restatement

def test_five_pairs_against_the_restatement():
    kp, pairs, m, want, got = five()
    check(got, want, pairs, m, "five")
    info = got[4]
    assert list(info[:, 0]) == [0, 0, 0, 0, ref.TOO_FEW] and info[3, 3] < 256      # (one hypothesis of pair 3 ran out of tries)


@pytest.mark.parametrize("m", ref.BOUNDARY_M)
def test_match_count_boundaries(m):
    kp, pairs, mm = ref.pack([ref.boundary_scene(m)])
    for refit in (0, 2):
        kw = dict(KW, refit_iters=refit)
        check(run(kp, pairs, mm, **kw), ref.verify_numpy(kp, pairs, mm, **kw), pairs, mm, f"m={m} refit={refit}")


@pytest.mark.parametrize("n_hyp", ref.BOUNDARY_HYP)
def test_hypothesis_count_boundaries(n_hyp):
    kp, pairs, m = five()[:3]
    kw = dict(KW, n_hyp=n_hyp, pair_base=1)
    check(run(kp[1:3], pairs[1:2], m[1:2], **kw), ref.verify_numpy(kp[1:3], pairs[1:2], m[1:2], **kw), pairs[1:2], m[1:2],
          f"n_hyp={n_hyp}")


def test_pair_count_boundaries_and_infinite_threshold():
    kp, pairs, m, want, _ = five()
    for n in (1, 3):
        check(run(kp[:n + 1], pairs[:n], m[:n], **KW), want[:n], pairs, m, f"n_pairs={n}")
    po, mo, F, cost, info = run(kp[:1], pairs[:0], m[:0], **KW)
    assert po.shape == (0, CAP, 2) and mo.shape == (0,) and F.shape == (0, 9) and cost.shape == (0,) and info.shape == (0, 4)
    # and at the ABI: no pair, no launch, no pointer needed
    from meatmodeler_amd import _lib
    import ctypes as C
    prm = _lib.VerifyParams(256, 16, 16, 2, 0, 0, 0, 0, 2.0)
    assert _lib.lib.mm_verify_matches(_lib.default_context().h, None, None, None, 0, CAP, C.byref(prm), None, None, None, None,
                                      None, None, 0) == 0
    # tau = +inf: every well-formed match is an inlier of every hypothesis
    kw = dict(KW, threshold_px=math.inf)
    got = run(kp[:4], pairs[:3], m[:3], **kw)
    check(got, ref.verify_numpy(kp[:4], pairs[:3], m[:3], **kw), pairs, m, "tau=inf")
    assert np.array_equal(got[1], m[:3]) and np.array_equal(got[0], pairs[:3]) and np.isfinite(got[3]).all()


# ------------------------------------------------------------------------------------------------ determinism

def same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def rows(out, lo, hi):
    return tuple(t[lo:hi] for t in out)


def test_repeats_bit_for_bit_and_a_pair_does_not_see_its_neighbours():
    kp, pairs, m, _, whole = five()
    assert same(run(kp, pairs, m, **KW), whole)
    for p in range(5):
        one = run(kp[p:p + 2], pairs[p:p + 1], m[p:p + 1], pair_base=p, **KW)
        assert same(one, rows(whole, p, p + 1)), p
    assert same(run(kp[2:], pairs[2:], m[2:], pair_base=2, **KW), rows(whole, 2, 5))
    # the pairs laid out in reverse order in memory (each with its two frames), verified one by one with their own pair_base
    kp_r = np.concatenate([kp[p:p + 2] for p in reversed(range(5))])
    pairs_r, m_r = pairs[::-1].copy(), m[::-1].copy()
    for k, p in enumerate(reversed(range(5))):
        one = run(kp_r[2 * k:2 * k + 2], pairs_r[k:k + 1], m_r[k:k + 1], pair_base=p, **KW)
        assert same(one, rows(whole, p, p + 1)), p
    # a different pair_base or seed is a different draw
    assert not same(run(kp[:2], pairs[:1], m[:1], pair_base=1, **KW)[4:], rows(whole, 0, 1)[4:])


# ------------------------------------------------------------------------------------------------ failure paths

def test_all_matches_on_one_pixel_is_no_model():
    kp = np.zeros((2, CAP, 2), np.float32)
    kp[0], kp[1] = (100.0, 200.0), (130.0, 210.0)
    pairs = np.full((1, CAP, 2), -1, np.int32)
    pairs[0, :64] = np.stack([np.arange(64), np.arange(64)[::-1]], axis=1)
    m = np.array([64], np.int32)
    for on_fail, n_kept in (("keep", 64), ("drop", 0)):
        po, mo, F, cost, info = run(kp, pairs, m, on_fail=on_fail, **KW)
        assert tuple(info[0]) == (ref.NO_MODEL, 0, -1, 0) and np.isnan(F).all() and np.isnan(cost).all()
        assert mo[0] == n_kept and np.array_equal(po[0, :n_kept], pairs[0, :n_kept]) and (po[0, n_kept:] == -1).all()
    assert ref.verify_numpy(kp, pairs, m, **KW)[0]["flags"] == ref.NO_MODEL


def test_pure_outliers_are_weak():
    kp, pairs, m = ref.weak_fixture()
    for on_fail in ("keep", "drop"):
        kw = dict(KW, min_inliers=32)
        got = run(kp, pairs, m, on_fail=on_fail, **kw)
        check(got, ref.verify_numpy(kp, pairs, m, on_fail=on_fail == "drop", **kw), pairs, m, f"weak {on_fail}")
        assert got[4][0, 0] == ref.WEAK and got[1][0] == (64 if on_fail == "keep" else 0)
    # the same pair is not weak when eight inliers are enough
    assert run(kp, pairs, m, **dict(KW, min_inliers=8))[4][0, 0] == 0


def test_malformed_matches_are_dropped_and_flagged():
    kp, pairs, m = ref.malformed_fixture()
    got = run(kp, pairs, m, pair_base=2, **KW)
    check(got, ref.verify_numpy(kp, pairs, m, pair_base=2, **KW), pairs, m, "malformed")
    po, mo = got[0], got[1]
    assert got[4][0, 0] == ref.MALFORMED and (po[0, :mo[0]] >= 0).all() and (po[0, :mo[0]] < CAP).all()
    # too few matches AND a malformed one: both flags, and on_fail decides
    few = pairs.copy()
    few[0, 15:] = -1
    got = run(kp, few, np.array([15], np.int32), pair_base=2, **KW)
    assert tuple(got[4][0]) == (ref.TOO_FEW | ref.MALFORMED, 0, -1, 0) and got[1][0] == 15
    assert run(kp, few, np.array([15], np.int32), pair_base=2, on_fail="drop", **KW)[1][0] == 0


def test_bad_arguments_raise():
    kp, pairs, m = (dev(a) for a in five()[:3])
    for kw in (dict(n_hyp=0), dict(n_hyp=4097), dict(threshold_px=-1.0), dict(threshold_px=math.nan), dict(on_fail="ignore"),
               dict(refit_iters=-1)):
        with pytest.raises(ValueError):
            ops.verify_matches(kp, pairs, m, **kw)
    with pytest.raises(ValueError):
        ops.verify_matches(kp[:-1], pairs, m)


# ------------------------------------------------------------------------------------------------ surface

def test_processor_verify_matches_equals_the_op():
    x, xp, truth = ref.five_pairs()[0][0]
    mask, F = processor.verifyMatches(x.astype(np.float64), xp.astype(np.float64), **KW)
    # the same matches through the op: key point j of both frames is match j
    n = len(x)
    kp2 = np.stack([x, xp])
    idx = np.arange(n, dtype=np.int32)
    po, mo, Fo, _, info = run(kp2, np.stack([idx, idx], axis=1)[None], np.array([n], np.int32), **KW)
    assert mask.dtype == bool and mask.shape == (n,) and F.shape == (3, 3)
    assert np.array_equal(np.nonzero(mask)[0], po[0, :mo[0], 0]) and np.array_equal(F.ravel(), Fo[0])
    assert (mask & truth).sum() >= 0.95 * truth.sum() and (mask & ~truth).sum() <= 6
    e = np.einsum("ni,ij,nj->n", np.c_[xp, np.ones(n)], F, np.c_[x, np.ones(n)])
    assert np.abs(e[mask]).max() < np.abs(e[~mask]).max()
    mask0, F0 = processor.verifyMatches(np.array([]), np.array([]))
    assert mask0.shape == (0,) and np.isnan(F0).all()
    mask15, F15 = processor.verifyMatches(x[:15], xp[:15])      # too few: passed through
    assert mask15.all() and np.isnan(F15).all()
    assert not processor.verifyMatches(x[:15], xp[:15], on_fail="drop")[0].any()


@functools.lru_cache(maxsize=None)
def clip():
    frames, ext, K = synth.render_orbit_frames(6, 640, 480, arc_deg=6.0)
    return dev(frames), ext, K


def test_run_without_verify_is_unchanged_and_with_verify_links_only_inliers():
    frames, ext, K = clip()
    pipe = ClipPipeline(480, 640, 600, batch=6)
    plain = pipe.run(frames, K, ext, ba=False)
    none = pipe.run(frames, K, ext, ba=False, verify=None)
    assert "verify" not in none
    for k in ("track_ptr_dev", "obs_frame_dev", "obs_kp_dev", "points0"):
        assert torch.equal(plain[k], none[k])
    timers = {}
    out = pipe.run(frames, K, ext, ba=False, verify={}, timers=timers)
    assert timers["verify"] > 0.0
    no_timer = {}
    pipe.run(frames, K, ext, ba=False, timers=no_timer)
    assert "verify" not in no_timer and "match" in no_timer
    v = out["verify"]
    assert v["info"].shape == (5, 4) and v["cost"].shape == (5,) and v["F"].shape == (5, 9) and v["matches_in"].shape == (5,)
    assert v["info"].dtype == torch.int32 and v["F"].dtype == torch.float64
    assert np.array_equal(v["matches_in"].cpu().numpy(), plain["match_count"])
    # the stages by hand: every pair's kept matches are an ordered subset of the unverified ones
    det = pipe.detect(frames)
    pairs, m = pipe.match(det)
    po, mo, F, cost, info = pipe.verify(det, pairs, m)
    assert torch.equal(info, v["info"]) and torch.equal(F.nan_to_num(-7.0), v["F"].nan_to_num(-7.0))
    assert np.array_equal(mo.cpu().numpy(), out["match_count"])
    pairs, m, po, mo = (t.cpu().numpy() for t in (pairs, m, po, mo))
    for p in range(5):
        before = [tuple(r) for r in pairs[p, :m[p]]]
        at = -1
        for r in po[p, :mo[p]]:
            at = before.index(tuple(r), at + 1)      # (ValueError: not a subsequence)
        print(f"pair {p}: {mo[p]} of {m[p]} matches kept, info {info[p].tolist()}")
        assert 0 < mo[p] <= m[p]
    assert out["n_tracks"] <= plain["n_tracks"] and out["n_obs"] <= plain["n_obs"]
    print(f"tracks {plain['n_tracks']} -> {out['n_tracks']}, observations {plain['n_obs']} -> {out['n_obs']}")
    for bad in (dict(nhyp=64), dict(pair_base=1)):
        with pytest.raises(ValueError):
            pipe.run(frames, K, ext, ba=False, verify=bad)
