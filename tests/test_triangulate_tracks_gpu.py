"""GPU: mm_triangulate_tracks through the C ABI wrappers (ops.triangulate_tracks, processor.triangulateTracks,
ClipPipeline.run(triangulation="multi_view", cull=...)) against the NumPy restatement and the independent references of
tests/test_triangulate_tracks_cpu.py.

Shapes: track lengths 2, 3, 4, 5 (one lane group full and one over), 63, 64, 65 and 200 (longer than a wave and than any
per-lane chunk; F = 200) mixed in one call, sorted long-first and short-first; T in {0, 1, 3, 257} (partial tail group and
tail workgroup); a track that visits its frames out of order.

Tolerances (RADIUS = 6, the orbit's): 1e-9 RADIUS against the SVD, 1e-6 RADIUS against least_squares, 1e-9 on the quality
columns, flags exact.  Against the restatement after 8 trial steps: 2.4e-8 RADIUS.  1e-9 proved tighter than contracted
multiply-adds allow: the first run on the MI355X measured 2.397e-9 RADIUS (all three orders), the size of the restatement's
own distance to the minimiser (2.4e-9 RADIUS) -- near convergence the strict "cost is lower" test of a trial step is decided
in the last bits of two sums, the kernel's (fused multiply-adds, four-lane order) and NumPy's fall on either side, and the two
then differ by that last, rounding-sized step.  The bound is the measured gap with a margin of ten.
"""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_triangulate_tracks_cpu as ref  # noqa: E402
from meatmodeler_amd import ops, processor, synth  # noqa: E402
from meatmodeler_amd.pipeline import ClipPipeline  # noqa: E402
from meatmodeler_amd.track import Track  # noqa: E402
from oracle import ba_oracle as bo  # noqa: E402

DEV = torch.device("cuda", 0)
RADIUS = ref.RADIUS
LENGTHS = (2, 3, 4, 5, 63, 64, 65, 200)
RESTATEMENT_TOL = 2.4e-8 * RADIUS      # (measured 2.397e-9 RADIUS, x 10: see the module docstring)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def run(proj, tp, fr, xy, **kw):
    X, q, fl = ops.triangulate_tracks(dev(proj), dev(tp), dev(fr), dev(xy), **kw)
    return X.cpu().numpy(), q.cpu().numpy(), fl.cpu().numpy()


def reorder(tp, fr, xy, order):
    """The CSR with its tracks in `order`."""
    lens = np.diff(tp)
    idx = np.concatenate([np.arange(tp[t], tp[t + 1]) for t in order]) if len(order) else np.zeros(0, np.int64)
    ptr = np.concatenate([[0], np.cumsum(lens[order])]).astype(np.int32)
    return ptr, fr[idx], xy[idx]


def numpy_quality(proj, tp, fr, xy, X):
    return np.stack([ref.quality_at(proj, fr[tp[t]:tp[t + 1]], xy[tp[t]:tp[t + 1]], X[t]) for t in range(len(tp) - 1)])


def costs(proj, tp, fr, xy, X):
    return np.array([(ref.residuals(proj, fr[tp[t]:tp[t + 1]], xy[tp[t]:tp[t + 1]], X[t])[0] ** 2).sum()
                     for t in range(len(tp) - 1)])


def close(a, b, tol=1e-9):
    """relative, or absolute where the value is below 1"""
    return np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b))


@functools.lru_cache(maxsize=None)
def mixed_scene():
    """257 tracks over F = 200, the lengths cycling through LENGTHS (the 200-frame one five times only), track 6 visiting
    its frames out of order; with the references computed once: SVD, restatement at 8 trial steps, least_squares."""
    proj = ref.orbit_projections(200)
    rng = np.random.default_rng(23)
    short = LENGTHS[:-1]      # 2 .. 65 in turn; the 200-frame track (slow in the NumPy references) at five places only
    lengths = [short[i % len(short)] for i in range(257)]
    for i in (7, 60, 130, 200, 256):
        lengths[i] = LENGTHS[-1]
    tp, fr, xy, _ = ref.make_tracks(proj, lengths, rng)
    s = slice(tp[6], tp[7])      # (length 65)
    perm = rng.permutation(tp[7] - tp[6])
    fr[s], xy[s] = fr[s][perm], xy[s][perm]
    T = len(tp) - 1
    svd = np.stack([ref.svd_point(proj, fr[tp[t]:tp[t + 1]], xy[tp[t]:tp[t + 1]]) for t in range(T)])
    np8 = ref.triangulate_tracks_numpy(proj, tp, fr, xy, 8)
    sci = np.stack([ref.scipy_point(proj, fr[tp[t]:tp[t + 1]], xy[tp[t]:tp[t + 1]], svd[t]) for t in range(T)])
    for a in (proj, tp, fr, xy, svd, np8, sci):
        a.setflags(write=False)
    return proj, tp, fr, xy, svd, np8, sci


def orders():
    tp = mixed_scene()[1]
    lens = np.diff(tp)
    T = len(lens)
    return dict(mixed=np.arange(T), long_first=np.argsort(-lens, kind="stable"), short_first=np.argsort(lens, kind="stable"))


# ------------------------------------------------------------------------------------------------ against the references

@pytest.mark.parametrize("order", ["mixed", "long_first", "short_first"])
def test_linear_stage_equals_the_svd(order):
    proj, tp, fr, xy, svd, _, _ = mixed_scene()
    o = orders()[order]
    X, _, _ = run(proj, *reorder(tp, fr, xy, o), refine_iters=0)
    gap = np.abs(X - svd[o]).max()
    print(f"{order}: linear stage against the SVD {gap / RADIUS:.3e} of the radius")
    assert gap <= 1e-9 * RADIUS


@pytest.mark.parametrize("order", ["mixed", "long_first", "short_first"])
def test_refined_points_equal_the_restatement_and_the_minimiser(order):
    proj, tp, fr, xy, _, np8, sci = mixed_scene()
    o = orders()[order]
    X, _, _ = run(proj, *reorder(tp, fr, xy, o), refine_iters=8)
    g_np, g_sci = np.abs(X - np8[o]).max(), np.abs(X - sci[o]).max()
    print(f"{order}: 8 trial steps against the restatement {g_np / RADIUS:.3e}, against least_squares {g_sci / RADIUS:.3e} "
          "of the radius")
    assert g_np <= RESTATEMENT_TOL
    assert g_sci <= 1e-6 * RADIUS


@pytest.mark.parametrize("iters", [0, 8])
def test_quality_and_flags_are_the_definitions_at_the_returned_point(iters):
    proj, tp, fr, xy = mixed_scene()[:4]
    # thresholds inside the spread of the data, so that every flag occurs on some track and not on others
    kw = dict(max_reproj_px=1.2, min_angle_deg=10.0, min_depth=5.5)
    X, q, fl = run(proj, tp, fr, xy, refine_iters=iters, **kw)
    qn = numpy_quality(proj, tp, fr, xy, X)
    assert close(q, qn).all(), np.abs(q - qn).max(axis=0)
    expect = ref.flags_of(q, np.diff(tp), X, 1.2, np.cos(np.radians(10.0)), 5.5)
    assert np.array_equal(fl, expect)
    for bit in (ref.BEHIND, ref.REPROJ, ref.PARALLAX):
        assert 0 < np.count_nonzero(fl & bit) < len(fl), bit
    # thresholds off: nothing flagged
    assert not run(proj, tp, fr, xy, refine_iters=iters)[2].any()


@pytest.mark.parametrize("T", [1, 3, 257])
def test_partial_groups_and_workgroups(T):
    proj, tp, fr, xy, svd, np8, _ = mixed_scene()
    o = np.arange(257)[::-1][:T]      # (from the end: the 200-frame track 256 is in every case)
    sub = reorder(tp, fr, xy, o)
    X0, _, _ = run(proj, *sub, refine_iters=0)
    X8, q, fl = run(proj, *sub, refine_iters=8)
    assert X0.shape == (T, 3) and q.shape == (T, 4) and fl.shape == (T,)
    assert np.abs(X0 - svd[o]).max() <= 1e-9 * RADIUS and np.abs(X8 - np8[o]).max() <= RESTATEMENT_TOL


def test_no_tracks():
    proj = mixed_scene()[0]
    X, q, fl = run(proj, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros((0, 2)))
    assert X.shape == (0, 3) and q.shape == (0, 4) and fl.shape == (0,)
    # the entry point itself: T = 0 is MM_OK without a launch, whatever the other pointers are
    from meatmodeler_amd._lib import default_context, lib, TriParams
    import ctypes as C
    prm = TriParams(8, 0, np.inf, 2.0, -np.inf)
    assert lib.mm_triangulate_tracks(default_context().h, None, 0, None, 0, None, None, C.byref(prm), None, None, None, None, 0) == 0
    assert lib.mm_triangulate_tracks(default_context().h, None, 4, None, 5, None, None, C.byref(prm), None, None, None, None, 0) != 0


def test_two_observation_tracks_equal_the_two_view_kernel():
    proj = ref.orbit_projections(40)
    tp, fr, xy, _ = ref.make_tracks(proj, [2] * 130, np.random.default_rng(5))
    X, _, _ = run(proj, tp, fr, xy, refine_iters=0)
    D = ops.triangulate_dlt(dev(proj), dev(fr[0::2]), dev(fr[1::2]), dev(xy[0::2]), dev(xy[1::2])).cpu().numpy()
    gap = (np.abs(X - D) / np.maximum(np.abs(D), 1e-300)).max()
    print(f"m = 2 against mm_triangulate_dlt: {gap:.3e} relative")
    assert np.allclose(X, D, rtol=1e-8, atol=0.0)


# ------------------------------------------------------------------------------------------------ isolation and determinism

def test_repeatable_isolated_and_permutation_invariant():
    proj, tp, fr, xy = mixed_scene()[:4]
    kw = dict(refine_iters=8, max_reproj_px=1.2, min_angle_deg=10.0, min_depth=5.5)
    a = run(proj, tp, fr, xy, **kw)
    b = run(proj, tp, fr, xy, **kw)
    for u, v in zip(a, b):
        assert np.array_equal(u, v, equal_nan=True)
    perm = np.random.default_rng(3).permutation(257)
    c = run(proj, *reorder(tp, fr, xy, perm), **kw)
    for u, v in zip(a, c):
        assert np.array_equal(u[perm], v, equal_nan=True)
    pd, tpd, frd, xyd = dev(proj), dev(tp), dev(fr), dev(xy)
    for t in range(257):      # every track alone: its row of the mixed call, bit for bit
        s = slice(int(tp[t]), int(tp[t + 1]))
        one = ops.triangulate_tracks(pd, tpd[t:t + 2] - tpd[t], frd[s], xyd[s], **kw)
        for u, v in zip(a, one):
            assert np.array_equal(u[t:t + 1], v.cpu().numpy(), equal_nan=True), t


# ------------------------------------------------------------------------------------------------ planted verdicts

@functools.lru_cache(maxsize=None)
def planted_scene():
    """200 clean tracks, 50 with one observation moved by 60-200 px, 20 far points seen from adjacent frames, 20 points
    behind their cameras (no noise), 10 single observations, 10 pairs through one projection matrix -- interleaved."""
    proj = ref.orbit_projections(40)
    C = ref.camera_centres(proj)
    rng = np.random.default_rng(41)
    kinds, frames, xys = [], [], []

    def track(kind, fr, X, sigma):
        kinds.append(kind)
        frames.append(np.asarray(fr))
        xys.append(ref.project(proj, np.asarray(fr), X) + rng.normal(0.0, sigma, (len(fr), 2)))

    for i in range(200):
        m = (3, 4, 5, 8)[i % 4]
        s = int(rng.integers(0, 40 - m + 1))
        track("clean", np.arange(s, s + m), rng.uniform(-1, 1, 3), 0.3)
    for i in range(50):
        m = (5, 8, 16)[i % 3]
        s = int(rng.integers(0, 40 - m + 1))
        track("outlier", np.arange(s, s + m), rng.uniform(-1, 1, 3), 0.3)
        ang = rng.uniform(0, 2 * np.pi)
        xys[-1][int(rng.integers(0, m))] += rng.uniform(60, 200) * np.array([np.cos(ang), np.sin(ang)])
    for i in range(20):
        s = int(rng.integers(0, 38))
        track("far", [s, s + 1], -1e4 * C[s] + rng.uniform(-1, 1, 3), 0.3)      # 1e4 radii away, beyond the origin
    for i in range(20):
        m = 3 + i % 3
        s = int(rng.integers(0, 40 - m + 1))
        track("behind", np.arange(s, s + m), 1.5 * C[s + m // 2] + rng.uniform(-0.3, 0.3, 3), 0.0)
    for i in range(10):
        track("single", [int(rng.integers(0, 40))], rng.uniform(-1, 1, 3), 0.3)
    for i in range(10):
        f = int(rng.integers(0, 40))
        track("same_frame", [f, f], rng.uniform(-1, 1, 3), 0.3)
    order = rng.permutation(len(kinds))
    kinds = np.array(kinds)[order]
    tp = np.concatenate([[0], np.cumsum([len(frames[i]) for i in order])]).astype(np.int32)
    fr = np.concatenate([frames[i] for i in order]).astype(np.int32)
    xy = np.concatenate([xys[i] for i in order])
    return proj, kinds, tp, fr, xy


THRESHOLDS = dict(max_reproj_px=4.0, min_angle_deg=1.0, min_depth=0.0)


def test_planted_tracks_get_their_verdict_and_no_clean_one_any():
    proj, kinds, tp, fr, xy = planted_scene()
    T = len(kinds)
    tr = [(fr[tp[t]:tp[t + 1]], xy[tp[t]:tp[t + 1]]) for t in range(T)]
    # the construction, in NumPy alone, with a factor of two to every threshold
    for t in range(T):
        f, x = tr[t]
        if kinds[t] in ("clean", "outlier", "far"):
            q = ref.quality_at(proj, f, x, ref.scipy_point(proj, f, x, ref.svd_point(proj, f, x)))
            if kinds[t] == "clean":
                assert q[1] < 2.0 and q[2] > 1.0 and q[3] < np.cos(np.radians(2.0)), (t, q)
            elif kinds[t] == "outlier":
                assert q[1] > 8.0, (t, q)
            else:
                assert q[3] > np.cos(np.radians(0.5)), (t, q)
        elif kinds[t] == "behind":
            q = ref.quality_at(proj, f, x, ref.svd_point(proj, f, x))
            assert q[2] < -1.0 and q[1] < 1e-6, (t, q)
    X8, q8, f8 = run(proj, tp, fr, xy, refine_iters=8, **THRESHOLDS)
    X0, q0, f0 = run(proj, tp, fr, xy, refine_iters=0, **THRESHOLDS)
    assert not f8[kinds == "clean"].any() and not f0[kinds == "clean"].any()
    assert (f8[kinds == "outlier"] & ref.REPROJ).all()
    assert (f8[kinds == "far"] & ref.PARALLAX).all()
    assert (f0[kinds == "behind"] & ref.BEHIND).all()
    for fl, X, q in ((f8, X8, q8), (f0, X0, q0)):
        assert (fl[kinds == "single"] == ref.DEGENERATE).all()
        bad = ~np.isfinite(X).all(axis=1)
        assert np.array_equal((fl & ref.DEGENERATE) != 0, bad | (np.diff(tp) < 2))
        assert np.isnan(q[(fl & ref.DEGENERATE) != 0]).all()
        assert np.isfinite(q[((fl & ref.DEGENERATE) == 0) & (kinds != "same_frame")]).all()
        assert np.array_equal(fl, ref.flags_of(q, np.diff(tp), X, 4.0, np.cos(np.radians(1.0)), 0.0))
    # the neighbours of the degenerate tracks: the same rows, bit for bit, as in a call without those tracks
    keep = np.nonzero((kinds != "single") & (kinds != "same_frame"))[0]
    Xk, qk, fk = run(proj, *reorder(tp, fr, xy, keep), refine_iters=8, **THRESHOLDS)
    assert np.array_equal(Xk, X8[keep]) and np.array_equal(qk, q8[keep], equal_nan=True) and np.array_equal(fk, f8[keep])


def test_refinement_never_raises_the_cost():
    """cost(8 trial steps) <= cost(linear) on every track that is refined, planted outliers included; both costs are
    evaluated in NumPy.  Only DEGENERATE tracks are left out: they are not refined, and X is asserted unchanged."""
    for name, (proj, tp, fr, xy) in (("mixed", mixed_scene()[:4]), ("planted", planted_scene()[:1] + planted_scene()[2:])):
        X0, _, f0 = run(proj, tp, fr, xy, refine_iters=0)
        X8, _, _ = run(proj, tp, fr, xy, refine_iters=8)
        deg = (f0 & ref.DEGENERATE) != 0
        assert np.array_equal(X0[deg], X8[deg], equal_nan=True)
        keep = np.nonzero(~deg)[0]
        tpk, frk, xyk = reorder(tp, fr, xy, keep)
        c0, c8 = costs(proj, tpk, frk, xyk, X0[keep]), costs(proj, tpk, frk, xyk, X8[keep])
        worst = int(np.argmax(c8 - c0))
        print(f"{name}: {len(keep)} refined tracks, largest cost(8) - cost(0) = {c8[worst] - c0[worst]:.3e} at track "
              f"{keep[worst]} (cost(0) {c0[worst]:.3e}, {tp[keep[worst] + 1] - tp[keep[worst]]} observations); "
              f"{np.count_nonzero(c8 > c0)} above")
        assert (c8 <= c0).all()


# ------------------------------------------------------------------------------------------------ surface

def test_processor_triangulate_tracks_equals_the_op():
    proj, tp, fr, xy = mixed_scene()[:4]
    tp, fr, xy = reorder(tp, fr, xy, np.arange(40))
    tracks = []
    for t in range(40):
        f, x = fr[tp[t]:tp[t + 1]], xy[tp[t]:tp[t + 1]]
        tr = Track(int(f[0]), tuple(x[0]), int(f[1]), tuple(x[1]))
        for k in range(2, len(f)):
            tr.update(int(f[k]), tuple(x[k]))
        tracks.append(tr)
    q, fl = processor.triangulateTracks(tracks, list(proj), **THRESHOLDS)
    X, qe, fe = run(proj, tp, fr, xy, **THRESHOLDS)
    assert isinstance(q, np.ndarray) and isinstance(fl, np.ndarray)
    assert np.array_equal(q, qe) and np.array_equal(fl, fe)
    for t, tr in enumerate(tracks):
        assert tr.getPoint().shape == (1, 3) and np.array_equal(tr.getPoint()[0], X[t])
    # a negative frame ID indexes from the end, one outside the list raises, as in triangulatePoints
    neg = [Track(-200 + int(fr[0]), tuple(xy[0]), int(fr[1]), tuple(xy[1]))]
    pos = [Track(int(fr[0]), tuple(xy[0]), int(fr[1]), tuple(xy[1]))]
    processor.triangulateTracks(neg, list(proj))
    processor.triangulateTracks(pos, list(proj))
    assert np.array_equal(neg[0].getPoint(), pos[0].getPoint())
    for bad in (200, -201):
        with pytest.raises(IndexError):
            processor.triangulateTracks([Track(0, (1.0, 2.0), bad, (3.0, 4.0))], list(proj))
    with pytest.raises(IndexError):
        run(proj, np.array([0, 2], np.int32), np.array([0, 200], np.int32), np.zeros((2, 2)))
    with pytest.raises(IndexError):
        run(proj, np.array([0, 2], np.int32), np.array([-1, 3], np.int32), np.zeros((2, 2)))
    assert processor.triangulateTracks([], list(proj))[1].shape == (0,)
    for kw in (dict(refine_iters=-1), dict(refine_iters=1001), dict(min_angle_deg=-1.0)):
        with pytest.raises(ValueError):
            run(proj, tp, fr, xy, **kw)
    with pytest.raises(ValueError):
        run(proj.reshape(-1, 4, 3), tp, fr, xy)


# ------------------------------------------------------------------------------------------------ ClipPipeline.run

@functools.lru_cache(maxsize=None)
def clip():
    frames, ext, K = synth.render_orbit_frames(6, 640, 480, arc_deg=6.0)
    return dev(frames), ext, K


def test_run_two_view_is_the_default_and_multi_view_is_the_op():
    frames, ext, K = clip()
    pipe = ClipPipeline(480, 640, 600, batch=6)
    default = pipe.run(frames, K, ext, ba=True)
    two = pipe.run(frames, K, ext, ba=True, triangulation="two_view")
    assert "track_flags" not in two and "kept_tracks" not in two
    assert torch.equal(default["points0"], two["points0"])
    assert torch.equal(default["ba"].pts, two["ba"].pts) and torch.equal(default["ba"].cams, two["ba"].cams)
    assert default["ba"].nfev == two["ba"].nfev and default["ba"].cost == two["ba"].cost
    multi = pipe.run(frames, K, ext, ba=False, triangulation="multi_view")
    for k in ("track_ptr_dev", "obs_frame_dev", "obs_kp_dev"):
        assert torch.equal(multi[k], default[k])
    coords, fi, _ = ops.flatten_tracks(multi["track_ptr_dev"], multi["obs_frame_dev"], multi["obs_kp_dev"], multi["xy_dev"])
    proj = dev(np.einsum("ij,fjk->fik", np.asarray(K, float), np.asarray(ext, float)[:, :3, :]))
    X, q, fl = ops.triangulate_tracks(proj, multi["track_ptr_dev"], fi, coords)
    assert multi["points0"].shape == (multi["n_tracks"], 3) and multi["n_tracks"] > 100
    assert torch.equal(multi["points0"], X) and torch.equal(multi["track_flags"], fl)
    assert torch.equal(multi["track_quality"].nan_to_num(-7.0), q.nan_to_num(-7.0))
    assert "kept_tracks" not in multi and not fl.any()
    assert not torch.equal(multi["points0"], default["points0"])


def test_run_with_cull_adjusts_exactly_the_kept_tracks():
    frames, ext, K = clip()
    pipe = ClipPipeline(480, 640, 600, batch=6)
    cull = dict(max_reproj_px=2.0, min_angle_deg=1.5, min_depth=0.0)
    # one evaluation: the adjustment returns its initial cost at its initial points (no evaluation left for a step)
    out = pipe.run(frames, K, ext, ba=True, triangulation="multi_view", cull=cull, max_nfev=1)
    fl = out["track_flags"].cpu().numpy()
    kept = out["kept_tracks"].cpu().numpy()
    assert np.array_equal(kept, np.nonzero(fl == 0)[0]) and (fl[kept] == 0).all()
    assert 0 < len(kept) < out["n_tracks"], (len(kept), out["n_tracks"])
    assert out["points0"].shape == (out["n_tracks"], 3)
    ClipPipeline.tracks_to_host(out)
    tp, of_, ok = out["track_ptr"], out["obs_frame"], out["obs_kp"]
    xy = out["xy_dev"].cpu().numpy()
    idx = np.concatenate([np.arange(tp[t], tp[t + 1]) for t in kept])
    obs = xy[of_[idx], ok[idx]].astype(np.float64)
    pi = np.repeat(np.arange(len(kept)), np.diff(tp)[kept])
    res = out["ba"]
    assert out["n_obs_local"] == len(idx)
    assert res.nfev == 1 and torch.equal(res.pts, out["points0"][out["kept_tracks"]])
    x0 = np.hstack([bo.frame_parameters(ext).ravel(), out["points0"].cpu().numpy()[kept].ravel()])
    c0 = 0.5 * np.sum(bo.point_fun(x0, K, 6, len(kept), of_[idx], pi, obs) ** 2)
    print(f"culled adjustment: {len(kept)} of {out['n_tracks']} tracks, initial cost {res.cost:.6e} (NumPy {c0:.6e})")
    assert abs(res.cost - c0) <= 1e-9 * c0
    # and a full adjustment of the kept tracks returns points aligned with kept_tracks
    full = pipe.run(frames, K, ext, ba=True, triangulation="multi_view", cull=cull)
    assert full["ba"].pts.shape == (len(kept), 3) and full["ba"].cost <= res.cost


def test_run_refuses_cull_without_multi_view_or_across_ranks():
    frames, ext, K = clip()
    pipe = ClipPipeline(480, 640, 600, batch=6)
    with pytest.raises(ValueError):
        pipe.run(frames, K, ext, cull=dict(max_reproj_px=4.0))
    with pytest.raises(ValueError):
        pipe.run(frames, K, ext, triangulation="two_view", cull=dict(max_reproj_px=4.0))
    with pytest.raises(ValueError):
        pipe.run(frames, K, ext, triangulation="three_view")
    for bad in (dict(max_reproj=4.0), dict(refine_iters=3), {}):      # a misspelt key; no threshold at all
        with pytest.raises(ValueError):
            pipe.run(frames, K, ext, triangulation="multi_view", cull=bad)

    class TwoRanks:
        @staticmethod
        def get_world_size():
            return 2

        @staticmethod
        def get_rank():
            return 0

    with pytest.raises(ValueError):
        pipe.run(frames, K, ext, triangulation="multi_view", cull=dict(max_reproj_px=4.0), dist=TwoRanks())
