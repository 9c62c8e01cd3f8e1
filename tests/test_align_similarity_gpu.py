"""GPU: mm_align_similarity, mm_apply_similarity, mm_camera_centres, their wrappers and ClipPipeline.run(align=...) against the
NumPy restatement of tests/test_align_similarity_cpu.py, at the shapes where the kernels can go wrong: the rows of a problem
around the score kernel's tile of 256 and the chunk of 4096, the hypotheses around the 64 lanes of a workgroup, zero, one and
four problems, and one call whose problems have 4097, 0, 3 and 300 rows.

Flags, best_h, the valid count, n_inliers and the mask are compared exactly: the CPU module asserts the margins that make that
sound (no distance within 1e-6 tau of tau, the runner-up 1e-9 above the winner, lambda2 / lambda1 a factor 2 from the tolerance)
for every fixture used here.  sim and cost are compared with the bounds below: the first run on the MI355X was made with 1e-9
(relative on s and cost, absolute on R, d relative to the spread of dst), the measured worst gaps are in the constants' comments
and the bounds are those gaps times 10.
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
import test_align_similarity_cpu as ref  # noqa: E402
from meatmodeler_amd import ops, processor, synth  # noqa: E402
from meatmodeler_amd.bundleAdjuster import frameParameters  # noqa: E402
from meatmodeler_amd.pipeline import ClipPipeline  # noqa: E402

DEV = torch.device("cuda", 0)
TAU = ref.TAU
# measured worst gap to the restatement x 10 (test_zz_report_the_worst_gaps prints the gaps): the file is built without FMA
# contraction and the restatement follows the header's order, sqrt and division are correctly rounded on both sides -- the
# MI355X gave the restatement's bits on every fixture, so the bounds on sim and cost are 0, as in tests/test_recover_poses_gpu.py
S_TOL = 0.0          # relative, on s (measured 0)
R_TOL = 0.0          # absolute, on R (measured 0)
D_TOL = 0.0          # on d, relative to the spread of dst (measured 0)
COST_TOL = 0.0       # relative, on cost (measured 0)
BA_TOL = 1.2e-12     # relative, on the adjustment's cost before and after a transform (measured 1.135e-13)
WORST = dict(s=0.0, R=0.0, d=0.0, cost=0.0, ba=0.0)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def run(src, dst, ptr=None, tau=TAU, **kw):
    """-> (sim, cost, inlier, info) as NumPy arrays."""
    return tuple(t.cpu().numpy() for t in ops.align_similarity(dev(src), dev(dst), ptr=ptr, tau=tau, **kw))


def check(got, results, dst, ptr):
    """One call against the restatement's per-problem results."""
    sim, cost, inlier, info = got
    assert sim.shape == (len(results), 13) and cost.shape == (len(results),) and info.shape == (len(results), 4)
    for q, r in enumerate(results):
        assert info[q].tolist() == r["info"].tolist(), (q, info[q], r["info"])
        assert np.array_equal(inlier[ptr[q]:ptr[q + 1]], r["inlier"]), q
        assert np.array_equal(np.isnan(sim[q]), np.isnan(r["sim"])) and math.isnan(cost[q]) == math.isnan(r["cost"]), q
        if np.isnan(r["sim"]).any():
            assert np.isnan(sim[q]).all() and info[q, 2] == -1
            continue
        gs, gR, gd = ref.sim_gap(sim[q], r["sim"], ref.spread_of(dst[ptr[q]:ptr[q + 1]]))
        gc = ref.rel_gap(cost[q], r["cost"])
        for k, g in zip(("s", "R", "d", "cost"), (gs, gR, gd, gc)):
            WORST[k] = max(WORST[k], g)
        assert gs <= S_TOL and gR <= R_TOL and gd <= D_TOL and gc <= COST_TOL, (q, gs, gR, gd, gc)


@pytest.mark.parametrize("n", ref.SHAPE_N)
def test_row_count_boundaries(n):
    src, dst = ref.shape_problem(n)
    got = run(src, dst)
    check(got, [ref.shape_result(n)], dst, [0, n])
    assert got[3][0, 0] == (ref.TOO_FEW if n < 3 else 0)


@pytest.mark.parametrize("n_hyp", ref.SHAPE_HYP)
def test_hypothesis_count_boundaries(n_hyp):
    src, dst = ref.shape_problem(300)
    got = run(src, dst, n_hyp=n_hyp)
    check(got, [ref.shape_result(300, n_hyp)], dst, [0, 300])
    assert got[3][0, 3] == n_hyp


def mixed():
    parts = [ref.shape_problem(n) for n in ref.MIXED]
    ptr = np.concatenate([[0], np.cumsum(ref.MIXED)])
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), ptr


def test_problem_count_boundaries():
    src, dst = ref.shape_problem(300)
    sim, cost, inlier, info = run(src, dst, ptr=[0])      # no problem: no launch
    assert sim.shape == (0, 13) and cost.shape == (0,) and info.shape == (0, 4) and inlier.shape == (300,) and not inlier.any()
    sim, cost, inlier, info = run(src[:0], dst[:0], ptr=[0, 0, 0])      # problems without rows
    assert info.tolist() == [[ref.TOO_FEW, 0, -1, 0]] * 2 and np.isnan(sim).all() and np.isnan(cost).all()
    src, dst, ptr = mixed()
    check(run(src, dst, ptr=ptr), [ref.shape_result(n, 256, 0, True, q) for q, n in enumerate(ref.MIXED)], dst, ptr)


def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_repeats_bit_for_bit_and_a_problem_does_not_see_its_neighbours():
    src, dst, ptr = mixed()
    whole = run(src, dst, ptr=ptr)
    assert same(whole, run(src, dst, ptr=ptr))
    for q in range(len(ref.MIXED)):
        lo, hi = int(ptr[q]), int(ptr[q + 1])
        alone = run(src[lo:hi], dst[lo:hi], prob_base=q)
        assert same(alone, (whole[0][q:q + 1], whole[1][q:q + 1], whole[2][lo:hi], whole[3][q:q + 1])), q
    # rows [a, b) of a call equal a call on that block with prob_base + a; a shifted base gives another sampling
    lo = int(ptr[1])
    block = run(src[lo:], dst[lo:], ptr=ptr[1:] - lo, prob_base=1)
    assert same(block, (whole[0][1:], whole[1][1:], whole[2][lo:], whole[3][1:]))
    shifted = run(src[lo:], dst[lo:], ptr=ptr[1:] - lo, prob_base=0)
    assert shifted[3][2, 2] != whole[3][3, 2] or shifted[0][2].tobytes() != whole[0][3].tobytes()
    # problems that own only the tail of the rows: the rows before ptr[0] belong to nobody and stay 0
    tail = run(src, dst, ptr=ptr[2:], prob_base=2)
    assert same(tail, (whole[0][2:], whole[1][2:], np.concatenate([np.zeros(lo, np.uint8), whole[2][lo:]]), whole[3][2:]))


def test_nan_rows_set_nonfinite_and_are_never_inliers():
    src, dst = ref.shape_problem(300)
    src, dst = src.copy(), dst.copy()
    dst[::7, 1] = math.nan
    src[5, 0] = math.inf
    want = ref.align_problem(src, dst, 0, TAU)
    ref.check_margins(want)
    got = run(src, dst)
    check(got, [want], dst, [0, 300])
    assert got[3][0, 0] == ref.NONFINITE and not got[2][::7].any() and not got[2][5]
    few = run(src[:2], np.full((2, 3), math.nan))
    assert few[3][0].tolist() == [ref.TOO_FEW | ref.NONFINITE, 0, -1, 0]
    # every row non-finite: no hypothesis is valid
    none = run(src[:40], np.full((40, 3), math.nan))
    assert none[3][0].tolist() == [ref.NO_MODEL | ref.NONFINITE, 0, -1, 0] and np.isnan(none[0]).all() and not none[2].any()


def test_rigid_weak_and_collinear():
    src, dst = ref.shape_problem(300, 0, False)
    got = run(src, dst, with_scale=False)
    check(got, [ref.shape_result(300, 256, 0, False)], dst, [0, 300])
    assert got[0][0, 0] == 1.0
    src, dst = ref.shape_problem(300)
    want = ref.align_problem(src, dst, 0, TAU, min_inliers=299)
    got = run(src, dst, min_inliers=299)
    check(got, [want], dst, [0, 300])
    assert got[3][0, 0] == ref.WEAK
    assert run(src[:5], dst[:5], min_points=6)[3][0].tolist() == [ref.TOO_FEW, 0, -1, 0]
    line = np.linspace(-1.0, 1.0, 50)[:, None] * np.array([0.3, -0.2, 0.9]) + np.array([1.0, 2.0, 3.0])
    got = run(line, 2.0 * line + 1.0)      # a straight dolly
    assert got[3][0].tolist() == [ref.NO_MODEL, 0, -1, 0] and np.isnan(got[0]).all() and not got[2].any()


@pytest.mark.parametrize("name", ["orbit", "small", "random"])
def test_fixtures_recover_the_truth(name):
    fx = ref.fixture(name)
    got = run(fx["src"], fx["dst"])
    check(got, [ref.fixture_result(name)], fx["dst"], [0, len(fx["src"])])
    assert np.array_equal(got[2].astype(bool), fx["truth"]) and got[3][0, 3] == 256


def test_tau_rel_and_the_host_wrappers():
    fx = ref.fixture("orbit")
    spread = ref.spread_of(fx["dst"])
    a = run(fx["src"], fx["dst"], tau=None, tau_rel=TAU / spread)
    b = run(fx["src"], fx["dst"], tau=(TAU / spread) * float(torch.sqrt(((dev(fx["dst"]) - dev(fx["dst"]).mean(dim=0)) ** 2)
                                                                       .sum(dim=1).mean())))
    assert same(a, b) and a[3][0, 1] == fx["truth"].sum()
    sim, mask, info = processor.alignSimilarity(fx["src"], fx["dst"], tau=TAU)
    want = run(fx["src"], fx["dst"])
    assert sim.tobytes() == want[0][0].tobytes() and np.array_equal(mask, want[2].astype(bool)) and info.tolist() == want[3][0].tolist()
    ext = scene()["ext"]
    P, E = processor.applySimilarity(sim, fx["src"], np.concatenate([ext, np.tile([[[0.0, 0.0, 0.0, 1.0]]], (6, 1, 1))], 1))
    Pn, En = ref.apply_numpy(sim, fx["src"], ext)
    assert P.shape == (80, 3) and E.shape == (6, 3, 4)
    eps, s_, d_ = np.finfo(float).eps, abs(sim[0]), np.abs(sim[10:]).max()
    assert np.abs(P - Pn).max() <= 8.0 * eps * (3.0 * s_ * np.abs(fx["src"]).max() + d_)      # (the magnitude of the terms summed)
    assert np.abs(E - En).max() <= 8.0 * eps * (3.0 + 6.1 * s_ + 3.0 * d_)
    assert ref.sim_gap(sim, fx["sim_true"], spread)[0] < 5.0 * ref.NOISE


# ------------------------------------------------------------------------------------------------ the two maps

@functools.lru_cache(maxsize=None)
def scene():
    """Six cameras on an arc looking at 40 points: every point is seen by every camera (F = 6, P = 40, 240 observations)."""
    rng = np.random.default_rng(21)
    K = np.array([[800.0, 0.0, 320.0], [0.0, 800.0, 240.0], [0.0, 0.0, 1.0]])
    X = rng.uniform(-1.0, 1.0, (40, 3))
    ext = []
    for a in np.deg2rad(np.linspace(-20.0, 20.0, 6)):
        R = np.array([[math.cos(a), 0.0, -math.sin(a)], [0.0, 1.0, 0.0], [math.sin(a), 0.0, math.cos(a)]])
        ext.append(np.concatenate([R, np.array([[0.05 * a], [0.02], [6.0]])], 1))
    ext = np.stack(ext)
    fi, pi = np.repeat(np.arange(6), 40).astype(np.int32), np.tile(np.arange(40), 6).astype(np.int32)
    order = np.lexsort((fi, pi))      # point-major
    fi, pi = fi[order], pi[order]
    y = np.einsum("ij,ojk,ok->oi", K, ext[fi], np.concatenate([X[pi], np.ones((240, 1))], 1))
    obs = y[:, :2] / y[:, 2:] + rng.normal(size=(240, 2)) * 0.5
    return dict(K=K, X=X, ext=ext, fi=fi, pi=pi, obs=obs)


def test_camera_centres_and_apply_against_numpy():
    sc = scene()
    rng = np.random.default_rng(4)
    eps = np.finfo(float).eps
    C = ops.camera_centres(dev(sc["ext"])).cpu().numpy()
    assert np.abs(C - ref.centres_numpy(sc["ext"])).max() <= 8.0 * eps * 6.1      # (three products of entries below 6.1)
    assert ops.camera_centres(dev(sc["ext"][:0])).shape == (0, 3)
    for _ in range(4):
        sim = ref.random_similarity(rng)
        pts, ext = dev(sc["X"]), dev(sc["ext"])
        ops.apply_similarity(dev(sim), pts, ext)
        Pn, En = ref.apply_numpy(sim, sc["X"], sc["ext"])
        bound = 8.0 * eps * (3.0 * 3.0 + 4.0 + 3.0 * 6.1 + 3.0 * 4.0)      # (s <= 3, |d| <= 4, |X| <= 1, |tc| <= 6.1)
        assert np.abs(pts.cpu().numpy() - Pn).max() <= bound and np.abs(ext.cpu().numpy() - En).max() <= bound
        only_pts, only_ext = dev(sc["X"]), dev(sc["ext"])
        ops.apply_similarity(dev(sim), only_pts, None)
        ops.apply_similarity(dev(sim), None, only_ext)
        assert torch.equal(only_pts, pts) and torch.equal(only_ext, ext)
    pts, ext = dev(sc["X"]), dev(sc["ext"])
    bad = np.concatenate([[math.nan], np.eye(3).ravel(), np.zeros(3)])
    ops.apply_similarity(dev(bad), pts, ext)      # a non-finite sim changes nothing
    assert np.array_equal(pts.cpu().numpy(), sc["X"]) and np.array_equal(ext.cpu().numpy(), sc["ext"])


def test_the_adjustment_cost_survives_a_transform():
    sc = scene()
    rng = np.random.default_rng(8)
    pb = ops.BADevice(sc["K"], sc["fi"], sc["pi"], sc["obs"], 6, 40, DEV)

    def cost(ext, pts):
        with np.errstate(all="ignore"):
            cams = dev(frameParameters(ext.cpu().numpy()).reshape(6, 6))
        return float(pb.residual(cams, pts)[0].item())
    before = cost(dev(sc["ext"]), dev(sc["X"]))
    assert before > 0.0
    for _ in range(4):
        pts, ext = dev(sc["X"]), dev(sc["ext"])
        ops.apply_similarity(dev(ref.random_similarity(rng)), pts, ext)
        gap = ref.rel_gap(cost(ext, pts), before)
        WORST["ba"] = max(WORST["ba"], gap)
        assert gap <= BA_TOL, gap


# ------------------------------------------------------------------------------------------------ the pipeline

@functools.lru_cache(maxsize=None)
def clip():
    frames, ext, Kc = synth.render_orbit_frames(6, 640, 480, arc_deg=6.0)      # (the clip of tests/test_recover_poses_gpu.py)
    return dev(frames), ext, Kc


def test_run_with_align_registers_the_chain_to_the_targets():
    frames, _, Kc = clip()
    pipe = ClipPipeline(480, 640, 600, batch=6)
    plain = pipe.run(frames, Kc, None, verify={}, poses={}, ba=False)
    E0 = plain["poses"]["extrinsics"].cpu().numpy()
    # targets: the recovered centres under a known similarity, a little noise, frame 3 somewhere else entirely
    rng = np.random.default_rng(2)
    sim_true = ref.random_similarity(rng)
    c0 = ref.centres_numpy(E0)
    targets = ref.transformed(sim_true, c0)
    targets += rng.uniform(-1.0, 1.0, targets.shape) * 1e-3 * ref.spread_of(targets)
    targets[3] += np.array([0.4, -0.3, 0.5]) * ref.spread_of(targets) * 10.0
    opts = dict(frames=[0, 1, 2, 3, 4, 5], centres=targets, n_hyp=64, seed=3)
    timers = {}
    out = pipe.run(frames, Kc, None, verify={}, poses={}, max_nfev=8, align=opts, timers=timers)
    al = out["align"]
    assert set(al) == {"sim", "cost", "info", "inlier"} and timers["align"] > 0.0
    tau = 0.05 * ref.spread_of(targets)
    src_gpu = ops.camera_centres(plain["poses"]["extrinsics"]).cpu().numpy()
    want = ref.align_problem(src_gpu, targets, 0, tau, n_hyp=64, seed=3)
    ref.check_margins(want)
    sim = al["sim"].cpu().numpy()
    assert al["info"].cpu().numpy().tolist() == want["info"].tolist() and al["inlier"].cpu().numpy().tolist() == [1, 1, 1, 0, 1, 1]
    g = ref.sim_gap(sim, want["sim"], ref.spread_of(targets))
    assert max(g) <= 1e-9, g      # (tau here comes from torch's own sum over the targets: not one of the pinned bounds)
    assert ref.sim_gap(sim, sim_true, ref.spread_of(targets))[0] <= 0.02      # (the scale; a 6 degree arc is nearly a line)
    # the recovered extrinsics of the two runs differ by exactly that transform, and the tracks are the same tracks
    moved = plain["poses"]["extrinsics"].clone()
    ops.apply_similarity(al["sim"], None, moved)
    assert torch.equal(out["poses"]["extrinsics"], moved) and torch.equal(out["track_ptr_dev"], plain["track_ptr_dev"])
    pts_moved = ref.apply_numpy(sim, plain["points0"].cpu().numpy())[0]
    ok = np.isfinite(pts_moved).all(axis=1) & np.isfinite(out["points0"].cpu().numpy()).all(axis=1)
    assert ok.sum() > 10
    # the adjustment ran in the target frame, and its result is registered once more
    ba = out["ba_aligned"]
    assert set(ba) == {"extrinsics", "points", "sim", "info"} and ba["extrinsics"].shape == (6, 3, 4)
    assert ba["points"].shape == out["ba"].pts.reshape(-1, 3).shape and torch.isfinite(ba["sim"]).all()
    assert int(ba["info"][0]) & (ops.ALIGN_TOO_FEW | ops.ALIGN_NO_MODEL) == 0
    assert torch.isfinite(ba["extrinsics"]).all() and not torch.equal(ba["points"], out["ba"].pts.reshape(-1, 3))
    # a straight line of targets: no model, nothing is transformed, no exception
    line = np.linspace(0.0, 1.0, 6)[:, None] * np.array([1.0, 2.0, 3.0])
    flat = pipe.run(frames, Kc, None, verify={}, poses={}, ba=False, align=dict(frames=list(range(6)), centres=line, tau=1e-3))
    assert int(flat["align"]["info"][0]) & ops.ALIGN_NO_MODEL and torch.equal(flat["poses"]["extrinsics"], plain["poses"]["extrinsics"])
    assert torch.isnan(flat["align"]["sim"]).all() and "ba_aligned" not in flat


def test_run_without_align_is_unchanged():
    frames, ext, Kc = clip()
    pipe = ClipPipeline(480, 640, 600, batch=6)
    timers = {}
    plain = pipe.run(frames, Kc, ext, max_nfev=4, timers=timers)
    none = pipe.run(frames, Kc, ext, max_nfev=4, align=None)
    assert set(plain) == set(none) and "align" not in plain and "ba_aligned" not in plain and "align" not in timers
    assert torch.equal(plain["points0"], none["points0"]) and torch.equal(plain["ba"].cams, none["ba"].cams)
    assert torch.equal(plain["ba"].pts, none["ba"].pts)
    # given extrinsics are registered too: targets = the given cameras' own centres, the identity comes back
    own = pipe.run(frames, Kc, ext, ba=False, align=dict(frames=[0, 2, 3, 5], extrinsics=np.asarray(ext)[[0, 2, 3, 5]]))
    sim = own["align"]["sim"].cpu().numpy()
    assert max(ref.sim_gap(sim, np.concatenate([[1.0], np.eye(3).ravel(), np.zeros(3)]), 1.0)) <= 1e-9
    assert own["align"]["inlier"].cpu().numpy().all()
    for bad in (dict(frames=[0, 1], centres=np.zeros((2, 3))), dict(frames=[0, 1, 6], centres=np.zeros((3, 3))), dict(bogus=1)):
        with pytest.raises(ValueError):
            pipe.run(frames, Kc, ext, ba=False, align=bad)


def test_zz_report_the_worst_gaps():
    """Runs last in the file: the figures the bounds were taken from."""
    print("worst gaps over the file: " + ", ".join(f"{k} {v:.3e}" for k, v in WORST.items()))
