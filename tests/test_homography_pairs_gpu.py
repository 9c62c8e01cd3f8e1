"""GPU: mm_verify_homography and mm_recover_poses_homography through the ops, the processor wrappers and
ClipPipeline.run(degeneracy=...) against the NumPy restatements of tests/test_homography_pairs_cpu.py.

Shapes: n_pairs <= 6, cap = 320.  The six-pair call holds general 160 + 96, planar 160 + 96, rotation 160 + 96, planar 64 + 0,
mixed 120 + 40 and planar 17 + 0 (inliers + outliers) with the verify_info of a real ops.verify_matches call; the boundaries
vary one thing at a time: m in {0, 7, 8, 9, 63, 64, 65, 255, 256, 257, cap}, n_hyp in {1, 63, 64, 65, 256}, n_pairs in
{0, 1, 2}, threshold_px = +inf.

Exact: flags, n_inliers, best_h, the number of valid hypotheses, n_F, the kept rows and the rows left untouched; for the
poses flags, winner, the four vote counts, m and the NaN pattern of the depths.  The fixtures keep the margins asserted in the
CPU file, so a mismatch there is not rounding.
Float fields against the restatement -- H up to sign and R, t, sigma, normal (absolute), the cost and the finite depths
(relative): started at 1e-9; the first run on the MI355X measured 0 on every one of them over every comparison of this file,
the pan pair of the rendered clip included (no FMA contraction, the header's order followed: no operation differs).  The
bounds are the measured gaps with a margin of ten: 0, equality.
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
import test_homography_pairs_cpu as ref  # noqa: E402
from meatmodeler_amd import ops, processor, synth  # noqa: E402
from meatmodeler_amd.pipeline import ClipPipeline  # noqa: E402

DEV = torch.device("cuda", 0)
CAP = ref.CAP
KW = ref.SIX_KW
K = ref.K_SCENE
# Gaps to the restatement, measured on the MI355X over every comparison of this file (0 everywhere), x 10 (module docstring)
H_TOL = 0.0
COST_TOL = 0.0
POSE_TOL = 0.0
DEPTH_TOL = 0.0

WORST = dict(H=0.0, cost=0.0, pose=0.0, depth=0.0)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def run(kp, pairs, m, verify_info=None, **kw):
    """-> (pairs_out, m_out, H, cost, info) as NumPy arrays."""
    vi = None if verify_info is None else dev(verify_info)
    return tuple(t.cpu().numpy() for t in ops.verify_homography(dev(kp), dev(pairs), dev(m), verify_info=vi, **kw))


def want_of(kp, pairs, m, verify_info=None, **kw):
    return ref.homography_numpy(np.asarray(kp, np.float64), pairs, m, verify_info, **kw)


def check(got, want, pairs, m, what=""):
    """One call against the restatement's list of per-pair results."""
    po, mo, H, cost, info = got
    for p, r in enumerate(want):
        mm = int(m[p])
        assert tuple(info[p]) == tuple(r["info"]), (what, p, info[p], r["info"])
        assert mo[p] == len(r["kept"]) and np.array_equal(po[p, :mo[p]], r["kept"]), (what, p)
        assert (po[p, mo[p]:] == -1).all(), (what, p)      # the sentinel ops.verify_homography fills the output with
        if not r["flags"] & (ref.TOO_FEW | ref.NO_MODEL | ref.WEAK):
            assert np.array_equal(po[p, :mo[p]], pairs[p, :mm][r["mask"]])      # the input rows under the mask, in order
        if r["best_h"] < 0:
            assert np.isnan(H[p]).all() and np.isnan(cost[p])
            continue
        assert abs(np.linalg.norm(H[p]) - 1.0) < 1e-12
        gH = ref.sign_gap(H[p], r["H"])
        gc = abs(cost[p] - r["cost"]) / r["cost"] if r["cost"] > 0 else abs(cost[p])
        WORST["H"], WORST["cost"] = max(WORST["H"], gH), max(WORST["cost"], gc)
        print(f"{what} pair {p}: |H - H_numpy| = {gH:.3e}, cost gap {gc:.3e} (worst so far {WORST['H']:.3e}, {WORST['cost']:.3e})")
        assert gH <= H_TOL and gc <= COST_TOL, (what, p, gH, gc)


@functools.lru_cache(maxsize=None)
def six():
    """The six-pair call: (kp, pairs, m), the library's verify_info, the restatement's results and the kernel's outputs
    (computed once, never changed)."""
    kp, pairs, m, _ = ref.six_pairs()
    vi = ops.verify_matches(dev(kp), dev(pairs), dev(m), **ref.VERIFY_KW)[4].cpu().numpy()
    return kp, pairs, m, vi, want_of(kp, pairs, m, vi, **KW), run(kp, pairs, m, vi, **KW)


# ------------------------------------------------------------------------------------------------ against the restatement

def test_six_pairs_against_the_restatement():
    kp, pairs, m, vi, want, got = six()
    print("verify_info", vi.tolist())
    check(got, want, pairs, m, "six")
    info = got[4]
    assert np.array_equal(info[:, 4], vi[:, 1]) and (info[:, 5] == 0).all()
    D = ref.DEGENERATE
    assert [int(f) & D for f in info[:, 0]] == [0, D, D, D, 0, D]
    assert info[0, 0] & ref.WEAK and list(info[1:, 0] & ~D) == [0] * 5


@pytest.mark.parametrize("m", ref.BOUNDARY_M)
def test_match_count_boundaries(m):
    kp, pairs, mm, _ = ref.boundary_fixture(m)
    kw = ref.boundary_kw(m)
    check(run(kp, pairs, mm, **kw), [ref.boundary_reference(m)], pairs, mm, f"m={m}")


@pytest.mark.parametrize("n_hyp", ref.BOUNDARY_HYP)
def test_hypothesis_count_boundaries(n_hyp):
    kp, pairs, m, _ = ref.boundary_fixture(64)
    check(run(kp, pairs, m, **ref.hyp_kw(n_hyp)), [ref.hyp_reference(n_hyp)], pairs, m, f"n_hyp={n_hyp}")


def test_default_collinear_tolerance_on_the_grid():
    kp, pairs, m = ref.grid_fixture()
    got = run(kp, pairs, m, **ref.GRID_KW)
    check(got, [ref.grid_reference()], pairs, m, "grid")
    assert 0 < got[4][0, 3] < 64


def test_pair_count_boundaries_and_infinite_threshold():
    kp, pairs, m, vi, want, _ = six()
    for n in (1, 2):
        check(run(kp[:n + 1], pairs[:n], m[:n], vi[:n], **KW), want[:n], pairs, m, f"n_pairs={n}")
    po, mo, H, cost, info = run(kp[:1], pairs[:0], m[:0], **KW)
    assert po.shape == (0, CAP, 2) and mo.shape == (0,) and H.shape == (0, 9) and cost.shape == (0,) and info.shape == (0, 6)
    # and at the ABI: no pair, no launch, no pointer needed
    from meatmodeler_amd import _lib
    import ctypes as C
    prm = _lib.HomographyParams(256, 8, 16, 2, 0, 0, 2.0, 1e-3, 0.8)
    assert _lib.lib.mm_verify_homography(_lib.default_context().h, None, None, None, 0, CAP, C.byref(prm), None, None, None, None,
                                         None, None, None, 0) == 0
    pprm = _lib.HPoseParams(8, 0, 0.5, 0.9, 1e-2)
    Kc = (C.c_double * 9)(*K.ravel())
    assert _lib.lib.mm_recover_poses_homography(_lib.default_context().h, Kc, None, None, None, None, None, 0, CAP, C.byref(pprm),
                                                None, None, None, None, None, None) == 0
    # tau = +inf: every well-formed match is an inlier of every hypothesis
    got = run(kp[1:4], pairs[1:3], m[1:3], pair_base=1, **ref.INF_KW)
    check(got, ref.inf_reference(), pairs[1:3], m[1:3], "tau=inf")
    assert np.array_equal(got[1], m[1:3]) and np.array_equal(got[0], pairs[1:3]) and np.isfinite(got[3]).all()


# ------------------------------------------------------------------------------------------------ determinism

def same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def rows(out, lo, hi):
    return tuple(t[lo:hi] for t in out)


def test_repeats_bit_for_bit_and_a_pair_does_not_see_its_neighbours():
    kp, pairs, m, vi, _, whole = six()
    assert same(run(kp, pairs, m, vi, **KW), whole)
    for p in range(6):
        one = run(kp[p:p + 2], pairs[p:p + 1], m[p:p + 1], vi[p:p + 1], pair_base=p, **KW)
        assert same(one, rows(whole, p, p + 1)), p
    assert same(run(kp[2:6], pairs[2:5], m[2:5], vi[2:5], pair_base=2, **KW), rows(whole, 2, 5))
    # a different pair_base is a different draw
    assert not same(run(kp[1:3], pairs[1:2], m[1:2], vi[1:2], pair_base=2, **KW)[4:], rows(whole, 1, 2)[4:])


def test_without_verify_info_there_is_no_verdict_and_nothing_else_changes():
    kp, pairs, m, vi, _, whole = six()
    po, mo, H, cost, info = run(kp, pairs, m, None, **KW)
    assert same((po, mo, H, cost), whole[:4])
    assert np.array_equal(info[:, 0], whole[4][:, 0] & ~ref.DEGENERATE) and (info[:, 4] == -1).all()
    assert np.array_equal(info[:, [1, 2, 3, 5]], whole[4][:, [1, 2, 3, 5]])
    # the verdict follows verify_info alone: a failed fundamental matrix, or a large n_F
    fake = vi.copy()
    fake[1] = (ref.WEAK, 0, -1, 0)
    fake[2, 1] = 100000
    fake[0, 0] = ref.NO_MODEL      # (pair 0's homography is weak: no verdict whatever F did)
    info2 = run(kp, pairs, m, fake, **KW)[4]
    D = ref.DEGENERATE
    assert [int(f) & D for f in info2[:, 0]] == [0, D, 0, D, 0, D] and info2[2, 4] == 100000
    assert [int(f) & D for f in run(kp, pairs, m, vi, **dict(KW, degenerate_frac=1.0))[4][:, 0]] == [0, 0, 0, D, 0, D]


# ------------------------------------------------------------------------------------------------ failure paths

def test_all_matches_on_one_pixel_is_no_model():
    kp = np.zeros((2, CAP, 2), np.float32)
    kp[0], kp[1] = (100.0, 200.0), (130.0, 210.0)
    pairs = np.full((1, CAP, 2), -1, np.int32)
    pairs[0, :64] = np.stack([np.arange(64), np.arange(64)[::-1]], axis=1)
    m = np.array([64], np.int32)
    po, mo, H, cost, info = run(kp, pairs, m, **KW)
    assert tuple(info[0]) == (ref.NO_MODEL, 0, -1, 0, -1, 0) and np.isnan(H).all() and np.isnan(cost).all()
    assert mo[0] == 0 and (po == -1).all()
    assert want_of(kp, pairs, m, **KW)[0]["flags"] == ref.NO_MODEL


def test_all_points_on_one_image_line_is_no_model_without_a_valid_hypothesis():
    rng = np.random.default_rng(4)
    kp = rng.uniform(0, 400, (2, CAP, 2)).astype(np.float32)
    s = rng.uniform(0, 1, 64)
    kp[0, :64] = np.column_stack([50 + 500 * s, 80 + 250 * s])      # image 1: one line; image 2: anything
    pairs = np.full((1, CAP, 2), -1, np.int32)
    pairs[0, :64] = np.stack([np.arange(64), rng.permutation(64)], axis=1)
    m = np.array([64], np.int32)
    for tol in (1e-3, 1e-6):
        po, mo, H, cost, info = run(kp, pairs, m, **dict(KW, collinear_tol=tol))
        assert tuple(info[0]) == (ref.NO_MODEL, 0, -1, 0, -1, 0) and np.isnan(H).all() and mo[0] == 0, tol
    assert want_of(kp, pairs, m, **KW)[0]["info"][3] == 0


def test_independent_uniform_pixels_are_weak_and_never_degenerate():
    kp, pairs, m = ref.uniform_fixture()
    vi = ops.verify_matches(dev(kp), dev(pairs), dev(m), **ref.VERIFY_KW)[4].cpu().numpy()
    for fake in (vi, np.array([[ref.WEAK, 0, -1, 0]], np.int32)):      # (whatever the fundamental matrix made of them)
        got = run(kp, pairs, m, fake, **ref.UNIFORM_KW)
        want = ref.uniform_reference()
        want["info"][4] = want["n_F"] = fake[0, 1]
        check(got, [want], pairs, m, "uniform")
        assert got[4][0, 0] == ref.WEAK and got[1][0] == 0


def test_malformed_matches_are_dropped_flagged_and_never_read_through():
    kp, bad, m = ref.malformed_fixture()
    got = run(kp, bad, m, pair_base=3, **KW)
    check(got, [ref.malformed_reference()], bad, m, "malformed")
    po, mo = got[0], got[1]
    assert got[4][0, 0] == ref.MALFORMED and 48 <= mo[0] <= 61 and (po[0, :mo[0]] >= 0).all() and (po[0, :mo[0]] < CAP).all()
    # too few matches AND a malformed one: both flags
    few = bad.copy()
    few[0, 7:] = -1
    got = run(kp, few, np.array([7], np.int32), pair_base=3, **KW)
    assert tuple(got[4][0]) == (ref.TOO_FEW | ref.MALFORMED, 0, -1, 0, -1, 0) and got[1][0] == 0


def test_bad_arguments_raise():
    kp, pairs, m = (dev(a) for a in six()[:3])
    for kw in (dict(n_hyp=0), dict(n_hyp=4097), dict(threshold_px=-1.0), dict(threshold_px=math.nan), dict(collinear_tol=-1.0),
               dict(degenerate_frac=1.5), dict(degenerate_frac=math.nan), dict(refit_iters=-1), dict(verify_info=m)):
        with pytest.raises(ValueError):
            ops.verify_homography(kp, pairs, m, **kw)
    with pytest.raises(ValueError):
        ops.verify_homography(kp[:-1], pairs, m)
    H = torch.zeros((6, 9), dtype=torch.float64, device=DEV)
    for kw in (dict(min_front_frac=1.5), dict(ambiguous_frac=-0.1), dict(rotation_tol=-1.0), dict(rotation_tol=math.nan),
               dict(normal_hint=torch.zeros((5, 3), dtype=torch.float64, device=DEV))):
        with pytest.raises(ValueError):
            ops.recover_poses_homography(kp, pairs, m, H, K, **kw)
    with pytest.raises(ValueError):
        ops.recover_poses_homography(kp, pairs, m, H[:5], K)
    with pytest.raises(ValueError):
        ops.recover_poses_homography(kp, pairs, m, H, np.eye(3) * 2.0)


# ------------------------------------------------------------------------------------------------ poses

def run_pose(kp, pairs, m, H, hint=None, **kw):
    h = None if hint is None else dev(hint)
    return tuple(t.cpu().numpy() for t in ops.recover_poses_homography(dev(kp), dev(pairs), dev(m), dev(H), K, normal_hint=h, **kw))


def check_pose(got, want, what=""):
    R, t, sigma, normal, depth, info = got
    wR, wt, wsigma, wnormal, wdepth, winfo, res = want
    assert np.array_equal(info, winfo), (what, info, winfo)
    assert np.array_equal(np.isnan(depth), np.isnan(wdepth)), what
    for name, a, b in (("R", R, wR), ("t", t, wt), ("sigma", sigma, wsigma), ("normal", normal, wnormal)):
        assert np.array_equal(np.isnan(a), np.isnan(b)), (what, name)
        g = np.nanmax(np.abs(a - b), initial=0.0)
        WORST["pose"] = max(WORST["pose"], g)
        print(f"{what} {name}: gap {g:.3e} (worst so far {WORST['pose']:.3e})")
        assert g <= POSE_TOL, (what, name, g)
    fin = np.isfinite(wdepth)
    g = float(np.max(np.abs(depth[fin] - wdepth[fin]) / np.abs(wdepth[fin]), initial=0.0))
    WORST["depth"] = max(WORST["depth"], g)
    print(f"{what} depth: relative gap {g:.3e} over {int(fin.sum())} values (worst so far {WORST['depth']:.3e})")
    assert g <= DEPTH_TOL, (what, g)


@pytest.mark.parametrize("hinted", [False, True])
def test_poses_of_the_six_pairs_against_the_restatement(hinted):
    """The pose call on what the homography call returned -- the restatement's H, so that both sides decompose the same bits."""
    kp = ref.six_pairs()[0]
    po, mo, H, hint = ref.six_pose_reference(hinted)[:4]
    want = ref.six_pose_reference(hinted)[4:]
    got = run_pose(kp, po, mo, H, hint)
    check_pose(got, want, f"six hint={hinted}")
    info = got[5]
    assert info[0, 0] == ref.POSE_TOO_FEW and info[2, 0] == ref.ROTATION and info[2, 1] == -1
    assert (got[1][2] == 0).all() and np.isnan(got[4][2]).all() and np.isnan(got[3][2]).all()
    assert all(info[p, 0] == 0 and info[p, 1] >= 0 for p in (1, 3, 5))
    # and on the kernel's own homographies: the same integers
    gk = run_pose(kp, six()[5][0], six()[5][1], six()[5][2], hint)
    assert np.array_equal(gk[5], info)


@pytest.mark.parametrize("m", (0, 7, 8))
def test_pose_match_floor(m):
    kp, pairs, mm, _ = ref.boundary_fixture(m)
    H = ref.true_H("planar", 0)[None]
    got = run_pose(kp, pairs, mm, H)
    check_pose(got, ref.hpose_numpy(np.asarray(kp, np.float64), pairs, mm, H, K), f"pose m={m}")
    assert bool(got[5][0, 0] & ref.POSE_TOO_FEW) == (m < 8) and got[5][0, 6] == m
    if m < 8:
        assert np.isnan(got[0]).all() and np.isnan(got[4]).all()
    # a homography that is not finite, or zero (l3 <= 0), has no motion
    for Hbad in (np.full((1, 9), np.nan), np.zeros((1, 9)), np.array([[1.0, 0, 0, 0, 1.0, 0, 0, 0, math.inf]])):
        if m >= 8:
            bad = run_pose(kp, pairs, mm, Hbad)
            assert bad[5][0, 0] == ref.POSE_NO_MODEL and np.isnan(bad[0]).all() and np.isnan(bad[4]).all()


# ------------------------------------------------------------------------------------------------ surface

def test_processor_wrappers_equal_the_ops():
    kp, pairs, m, vi, _, whole = six()
    rows_, wf, x, xp = ref.unpack_pair(kp.astype(np.float64), pairs, m, 1)
    n = len(x)
    mask, H, flags = processor.verifyHomography(x, xp, **KW)
    kp2 = np.stack([x, xp]).astype(np.float32)
    idx = np.arange(n, dtype=np.int32)
    one = np.stack([idx, idx], axis=1)[None]
    po, mo, Ho, _, info = run(kp2, one, np.array([n], np.int32), **KW)
    assert mask.dtype == bool and mask.shape == (n,) and H.shape == (3, 3) and flags == info[0, 0] == 0
    assert np.array_equal(np.nonzero(mask)[0], po[0, :mo[0], 0]) and np.array_equal(H.ravel(), Ho[0])
    assert mask.sum() == 160
    viz = np.array([[0, 165, 0, 256]], np.int32)
    assert processor.verifyHomography(x, xp, verify_info=dev(viz), **KW)[2] == ref.DEGENERATE
    n_front, R, t, pmask, normal, pflags = processor.recoverPoseFromHomography(x[mask], xp[mask], K, H)
    k = int(mask.sum())
    idk = np.arange(k, dtype=np.int32)
    Ro, to, _, no, do, io = run_pose(kp2[:, mask], np.stack([idk, idk], axis=1)[None], np.array([k], np.int32), Ho)
    assert np.array_equal(R.ravel(), Ro[0]) and np.array_equal(t, to[0]) and np.array_equal(normal, no[0]) and pflags == io[0, 0]
    assert np.array_equal(pmask, np.isfinite(do[0, :, 0])) and n_front == pmask.sum() == io[0, 2 + io[0, 1]]
    hinted = processor.recoverPoseFromHomography(x[mask], xp[mask], K, H, normal_hint=ref.PLANE_N)
    Rp, tp = ref.pair_motion(1)
    assert ref.rot_gap(hinted[1], Rp) <= 5e-3 and not hinted[5] & ref.POSE_AMBIGUOUS
    e = processor.verifyHomography(np.array([]), np.array([]))
    assert e[0].shape == (0,) and np.isnan(e[1]).all() and e[2] == ref.TOO_FEW
    e = processor.recoverPoseFromHomography(np.array([]), np.array([]), K, np.eye(3))
    assert e[0] == 0 and np.isnan(e[1]).all() and e[5] == ref.POSE_TOO_FEW
    # the rotation pair through the wrappers
    _, _, x2, xp2 = ref.unpack_pair(kp.astype(np.float64), pairs, m, 2)
    mask2, H2, _ = processor.verifyHomography(x2, xp2, **KW)
    r2 = processor.recoverPoseFromHomography(x2[mask2], xp2[mask2], K, H2)
    assert r2[5] == ref.ROTATION and r2[0] == 0 and (r2[2] == 0).all() and ref.rot_gap(r2[1], ref.pair_motion(2)[0]) <= 2e-3


PAN = 0.05      # the turn of the pan pair about the camera's y axis: 26 px at f = 525


@functools.lru_cache(maxsize=None)
def pan_clip():
    """Six frames at 640 x 480: three on an orbit, then the third camera turned in place, then the orbit goes on (every later
    camera turned with it).  The middle pair, 2 -> 3, is a pure pan."""
    K_clip = synth.default_K(640, 480, f=525.0)
    tex = synth.make_texture(1024, n_shapes=2000, seed=7)
    orbit = synth.orbit_cameras(5, arc_deg=24.0, radius=7.0, height=-2.0)
    P = np.array([[math.cos(PAN), 0, math.sin(PAN)], [0, 1, 0], [-math.sin(PAN), 0, math.cos(PAN)]])
    ext = np.stack([orbit[0], orbit[1], orbit[2], P @ orbit[2], P @ orbit[3], P @ orbit[4]])
    frames = np.stack([synth.render_frame(tex, e, K_clip, 640, 480) for e in ext])
    return dev(frames), ext, K_clip, P


def test_run_without_degeneracy_is_unchanged_and_with_it_the_pan_is_repaired():
    frames, ext, Kc, P = pan_clip()
    pipe = ClipPipeline(480, 640, 600, batch=6)
    plain = pipe.run(frames, Kc, ba=False, verify={}, poses={})
    none = pipe.run(frames, Kc, ba=False, verify={}, poses={}, degeneracy=None)
    assert "degeneracy" not in none
    for k in ("track_ptr_dev", "obs_frame_dev", "obs_kp_dev", "points0"):
        assert torch.equal(plain[k], none[k])
    for k in ("extrinsics", "R", "t", "info", "scale"):
        assert torch.equal(plain["poses"][k].nan_to_num(-7.0), none["poses"][k].nan_to_num(-7.0)), k
    timers = {}
    out = pipe.run(frames, Kc, ba=False, verify={}, poses={}, degeneracy={}, timers=timers)
    assert timers["degeneracy"] > 0.0 and "degeneracy" not in pipe.run(frames, Kc, ba=False, verify={}, poses={}, timers={})
    d = out["degeneracy"]
    assert d["H"].shape == (5, 9) and d["cost"].shape == (5,) and d["info"].shape == (5, 6) and d["pose_info"].shape == (5, 8)
    assert d["sigma"].shape == (5, 3) and d["normal"].shape == (5, 3)
    info, pinfo = d["info"].cpu().numpy(), d["pose_info"].cpu().numpy()
    sg = d["sigma"].cpu().numpy()
    print("homography info", info.tolist(), "\npose info", pinfo.tolist(), "\nverify info", out["verify"]["info"].cpu().numpy().tolist())
    print("n_H / n_F", (info[:, 1] / np.maximum(info[:, 4], 1)).round(3).tolist(), "sigma1/sigma3 - 1", (sg[:, 0] / sg[:, 2] - 1).tolist())
    deg = (info[:, 0] & ref.DEGENERATE) != 0
    assert deg[2] and pinfo[2, 0] & ref.ROTATION and not deg[[0, 1, 3, 4]].any()
    # the stages by hand: the pan pair is linked by the homography's inliers
    det = pipe.detect(frames)
    pairs, m = pipe.match(det)
    pv, mv, Fv, _, iv = pipe.verify(det, pairs, m)
    ph, mh, Hh, _, ih = pipe.homography(det, pairs, m, verify_info=iv)
    assert torch.equal(ih, d["info"]) and torch.equal(Hh.nan_to_num(-7.0), d["H"].nan_to_num(-7.0))
    mc = out["match_count"]
    assert mc[2] == int(mh[2]) and [mc[p] for p in (0, 1, 3, 4)] == [int(mv[p]) for p in (0, 1, 3, 4)]
    assert list(plain["match_count"]) == [int(v) for v in mv]
    # the other pairs' rows are those of the run without degeneracy
    for k in ("R", "t", "info", "sigma"):
        a, b = out["poses"][k].cpu().numpy(), plain["poses"][k].cpu().numpy()
        assert np.array_equal(a[[0, 1, 3, 4]], b[[0, 1, 3, 4]], equal_nan=True), k
    # the pan pair: the restatement on the matches read back from the device, then the chain
    ph_h, mh_h, H_h = ph.cpu().numpy(), mh.cpu().numpy(), Hh.cpu().numpy()
    xy = det["xy"].cpu().numpy().astype(np.float64)
    _, wf, x, xp = ref.unpack_pair(xy[2:4], ph_h[2:3], mh_h[2:3], 0)
    r = ref.hpose_pair(x, xp, wf, H_h[2], Kc)
    got_R, got_t = out["poses"]["R"][2].cpu().numpy(), out["poses"]["t"][2].cpu().numpy()
    print(f"pan pair: {mh_h[2]} matches, rot measure {r['rot']:.2e}, |R - R_numpy| = {np.abs(got_R - r['R']).max():.2e}, "
          f"|R - R_true| = {ref.rot_gap(got_R, P):.2e}")
    assert r["flags"] == ref.ROTATION and np.abs(got_R - r["R"]).max() <= POSE_TOL and (got_t == 0).all()
    assert ref.rot_gap(got_R, P) <= 5e-3
    E = out["poses"]["extrinsics"].cpu().numpy()
    chained = np.array([[(got_R[3 * i] * E[2, 0, c] + got_R[3 * i + 1] * E[2, 1, c]) + got_R[3 * i + 2] * E[2, 2, c] for c in range(4)]
                        for i in range(3)])
    assert np.array_equal(E[3], chained)      # (t = 0: the chain adds s * 0)
    cinfo = out["poses"]["chain_info"].cpu().numpy()
    scale = out["poses"]["scale"].cpu().numpy()
    assert cinfo[2, 0] == ops.CHAIN_FEW_COMMON and cinfo[3, 0] == ops.CHAIN_FEW_COMMON and scale[2] == scale[1] == scale[3]
    # without the repair the pan pair is chained with whatever translation its arbitrary F implies
    Ep = plain["poses"]["extrinsics"].cpu().numpy()
    centre = lambda T: -T[:, :3].T @ T[:, 3]      # noqa: E731
    print(f"camera centre moved over the pan: {np.linalg.norm(centre(Ep[3]) - centre(Ep[2])):.3f} without, "
          f"{np.linalg.norm(centre(E[3]) - centre(E[2])):.2e} with degeneracy")
    assert np.linalg.norm(centre(E[3]) - centre(E[2])) <= 1e-12
    for bad in (dict(nhyp=64), dict(pair_base=1)):
        with pytest.raises(ValueError):
            pipe.run(frames, Kc, ba=False, verify={}, degeneracy=bad)
    with pytest.raises(ValueError):
        pipe.run(frames, Kc, ext, ba=False, degeneracy={})
    # without poses: only the linking changes
    lk = pipe.run(frames, Kc, ext, ba=False, verify={}, degeneracy={})
    assert "pose_info" not in lk["degeneracy"] and list(lk["match_count"]) == list(mc)
