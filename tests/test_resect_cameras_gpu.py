"""GPU: mm_resect_cameras through ops.resect_cameras, processor.resectCameras and ClipPipeline.run(resect=...) against the
NumPy restatement of tests/test_resect_cameras_cpu.py.

Shapes: n_cams in {0, 1, 3, 5}; usable rows per camera in {0, 5, 6, 11, 12, 13, 63, 64, 65, 255, 256, 257, 300} (each with three
rows that are not usable); n_hyp in {1, 63, 64, 65, 256} -- the wave, workgroup-stride and LDS-tile edges of a 256-thread camera
workgroup.  The five-camera call holds 192 + 64 and 40 + 24 (inliers + outliers), 64 + 0 with half the points masked by pt_ok, a
planar camera with and without a prior, and a camera with malformed rows, a NaN point and a NaN pixel.

Exact: flags, n_inliers, best_h, the valid-hypothesis count, n_use, accepted polish steps, the inlier bytes and which of them
were left untouched.  The fixtures keep every row 0.02 px from tau, every depth 1e-3 from zero, the two best hypotheses and every
accept / reject decision 1e-9 apart (asserted in the CPU file), so a count that differs is not rounding.  The g6 chessboard frames
run the polish to convergence, where the last trials decide on roundings: their accepted-step count is not compared.
With a tolerance: extrinsics (absolute) and cost (relative).  Started at 1e-9; the first run on the MI355X measured the worst gap
over every comparison of this file as 0 on both: resect.hip is compiled without FMA contraction, +, *, / and sqrt are correctly
rounded on both sides and the restatement follows the kernels' order of operations, so they compute the same bits.  The
committed bounds are the measured gaps with a margin of ten -- zero: equality.
"""
import ctypes as C
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
import test_resect_cameras_cpu as ref  # noqa: E402
from meatmodeler_amd import _lib, ops, processor, synth  # noqa: E402
from meatmodeler_amd.pipeline import ClipPipeline  # noqa: E402

DEV = torch.device("cuda", 0)
# measured gap to the restatement x 10 (module docstring)
EXT_TOL = 0.0
COST_TOL = 0.0
WORST = dict(ext=0.0, cost=0.0)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def run(K, X, obs, pi, cam_ptr, cam_obs, pt_ok=None, prior=None, **kw):
    """-> (extrinsics, cost, inlier, info) as NumPy arrays; the inlier bytes start as UNTOUCHED."""
    inl = torch.full((len(obs),), ref.UNTOUCHED, dtype=torch.uint8, device=DEV)
    out = ops.resect_cameras(K, dev(np.asarray(X, np.float64)), dev(np.asarray(obs, np.float64)), dev(np.asarray(pi, np.int32)),
                             dev(np.asarray(cam_ptr, np.int32)), dev(np.asarray(cam_obs, np.int32)),
                             pt_ok=None if pt_ok is None else dev(pt_ok), prior=None if prior is None else dev(prior),
                             inlier=inl, **kw)
    return tuple(t.cpu().numpy() for t in out)


def check(got, want, what="", polish_count=True):
    ext, cost, inlier, info = got
    wext, wcost, winlier, winfo = want[:4]
    cols = slice(0, 6) if polish_count else slice(0, 5)
    assert np.array_equal(info[:, cols], winfo[:, cols]), (what, info, winfo)
    assert np.array_equal(inlier, winlier), (what, np.flatnonzero(inlier != winlier))
    assert np.array_equal(np.isnan(ext), np.isnan(wext)) and np.array_equal(np.isnan(cost), np.isnan(wcost)), what
    for c in range(len(info)):
        if np.isnan(wcost[c]):
            continue
        g = dict(ext=float(np.abs(ext[c] - wext[c]).max()), cost=float(abs(cost[c] / wcost[c] - 1.0)) if wcost[c] != 0 else 0.0)
        for k, v in g.items():
            WORST[k] = max(WORST[k], v)
        print(f"{what} camera {c}: gaps ext {g['ext']:.2e}, cost {g['cost']:.2e} (worst so far ext {WORST['ext']:.2e}, "
              f"cost {WORST['cost']:.2e})")
        assert g["ext"] <= EXT_TOL and g["cost"] <= COST_TOL, (what, c, g)


def same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def five(with_prior):
    """The five-camera call: the fixture, the restatement's result and the kernel's outputs (computed once, never changed)."""
    fx = ref.five_cameras(with_prior)
    return fx, ref.five_reference(with_prior), run(*fx["args"], **fx["kw"])


# ------------------------------------------------------------------------------------------------ against the restatement

@pytest.mark.parametrize("with_prior", (False, True))
def test_five_cameras_against_the_restatement(with_prior):
    fx, want, got = five(with_prior)
    check(got, want, f"five prior={with_prior}")
    for c in (0, 1, 2, 4) + ((3,) if with_prior else ()):
        R = got[0][c][:, :3]
        assert abs(np.linalg.det(R) - 1.0) < 1e-9 and np.abs(R @ R.T - np.eye(3)).max() < 1e-9


@pytest.mark.parametrize("n", ref.BOUNDARY_ROWS)
def test_usable_row_boundaries(n):
    fx = ref.boundary_fixture(n)
    got = run(*fx["args"], n_hyp=64, **fx["kw"])
    check(got, ref.boundary_reference(n), f"rows={n}")
    assert got[3][0, 4] == n and bool(got[3][0, 0] & ref.TOO_FEW) == (n < 12)
    assert (got[2] == ref.UNTOUCHED).sum() == 3


@pytest.mark.parametrize("n_hyp", ref.BOUNDARY_HYP)
def test_hypothesis_count_boundaries(n_hyp):
    fx = ref.boundary_fixture(65)
    got = run(*fx["args"], n_hyp=n_hyp, seed=ref.HYP_SEED, **fx["kw"])
    check(got, ref.boundary_reference(65, n_hyp, ref.HYP_SEED), f"n_hyp={n_hyp}")
    assert got[3][0, 3] <= n_hyp


def test_camera_count_boundaries_and_cam_base():
    fx, want, whole = five(False)
    K, X, obs, pi, cam_ptr, cam_obs = fx["args"]
    # rows [a, b) of the call equal a call on that block with cam_base + a (the inlier bytes of the other cameras untouched)
    for a, b in ((0, 1), (1, 4), (2, 5)):
        part = run(K, X, obs, pi, cam_ptr[a:b + 1], cam_obs, cam_base=a, **fx["kw"])
        assert same((part[0], part[1], part[3]), (whole[0][a:b], whole[1][a:b], whole[3][a:b])), (a, b)
        touched = np.zeros(len(obs), bool)
        rows = cam_obs[cam_ptr[a]:cam_ptr[b]]
        touched[rows[(rows >= 0) & (rows < len(obs))]] = True
        assert np.array_equal(part[2][touched], whole[2][touched]) and (part[2][~touched] == ref.UNTOUCHED).all()
    # a camera alone equals its row of the call
    for c in range(5):
        one = run(K, X, obs, pi, cam_ptr[c:c + 2], cam_obs, cam_base=c, **fx["kw"])
        assert same((one[0], one[1], one[3]), (whole[0][c:c + 1], whole[1][c:c + 1], whole[3][c:c + 1])), c
    # no camera: shapes, and at the ABI no launch and no pointer needed
    ext, cost, inlier, info = run(K, X, obs, pi, cam_ptr[:1], cam_obs)
    assert ext.shape == (0, 3, 4) and cost.shape == (0,) and info.shape == (0, 6) and (inlier == ref.UNTOUCHED).all()
    prm = _lib.ResectParams(256, 12, 12, 2, 8, 0, 0, 0, 2.0)
    Kh = np.ascontiguousarray(K.ravel())
    assert _lib.lib.mm_resect_cameras(_lib.default_context().h, Kh.ctypes.data_as(_lib.c_f64p), None, 0, None, None, 0, None, None, 0, 0,
                                      None, None, C.byref(prm), None, None, None, None, None, 0) == 0


def test_repeats_bit_for_bit():
    fx, _, whole = five(True)
    assert same(run(*fx["args"], **fx["kw"]), whole)


def test_g6_chessboard_frames_through_the_kernel():
    fx = ref.g6_fixture()
    got = run(*fx["args"], prior=fx["ext0"], **fx["kw"])
    want = ref.g6_reference(True)
    ext, cost, inlier, info = got
    assert (info[:, 3] == 0).all() and (info[:, 2] == 64).all() and (info[:, 0] == 0).all() and (inlier == 1).all()
    gap = np.abs(ext - fx["result"]).max()
    print(f"g6: |polished - result| = {gap:.2e}, |polished - restatement| = {np.abs(ext - want[0]).max():.2e}, accepted steps "
          f"{info[:, 5].tolist()} (restatement {want[3][:, 5].tolist()}), half the summed cost {0.5 * cost.sum():.5f}")
    assert gap <= 1e-8
    assert np.array_equal(info[:, :5], want[3][:, :5]) and np.abs(ext - want[0]).max() <= 1e-9
    none = run(*fx["args"], **fx["kw"])
    check(none, ref.g6_reference(False), "g6 without a prior")
    assert (none[3][:, 0] == ref.NO_MODEL).all() and np.isnan(none[0]).all()


# ------------------------------------------------------------------------------------------------ surface

def test_argument_errors_come_back_before_the_device_is_touched():
    fx, _, _ = five(False)
    K, X, obs, pi, cam_ptr, cam_obs = fx["args"]
    Xd, od, pd, cpd, cod = dev(X), dev(obs), dev(pi), dev(cam_ptr), dev(cam_obs)
    n_cams, n_rows = len(cam_ptr) - 1, len(cam_obs)
    ext = torch.empty((n_cams, 12), dtype=torch.float64, device=DEV)
    cost = torch.empty(n_cams, dtype=torch.float64, device=DEV)
    inl = torch.zeros(len(obs), dtype=torch.uint8, device=DEV)
    info = torch.zeros((n_cams, 6), dtype=torch.int32, device=DEV)
    wsb = _lib.lib.mm_resect_workspace_bytes(n_cams, 256, n_rows)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    h = _lib.default_context().h
    p = _lib.ptr

    def call(prm=None, Kh=None, ws_bytes=wsb, null=None):
        prm = prm or _lib.ResectParams(256, 12, 12, 2, 8, 0, 0, 0, 2.0)
        Kh = np.ascontiguousarray(K.ravel() if Kh is None else np.asarray(Kh, float).ravel())
        a = dict(X=p(Xd), obs=p(od), pi=p(pd), cam_ptr=p(cpd), cam_obs=p(cod), ext=p(ext), cost=p(cost), inl=p(inl), info=p(info),
                 ws=p(ws))
        if null:
            a[null] = None
        return _lib.lib.mm_resect_cameras(h, Kh.ctypes.data_as(_lib.c_f64p), a["X"], len(X), a["obs"], a["pi"], len(obs),
                                          a["cam_ptr"], a["cam_obs"], n_rows, n_cams, None, None, C.byref(prm), a["ext"], a["cost"],
                                          a["inl"], a["info"], a["ws"], ws_bytes)

    assert call() == 0
    for n_hyp in (0, -1, 4097):
        assert call(_lib.ResectParams(n_hyp, 12, 12, 2, 8, 0, 0, 0, 2.0)) == -1
    for tau in (math.nan, -1.0):
        assert call(_lib.ResectParams(256, 12, 12, 2, 8, 0, 0, 0, tau)) == -1
    assert call(_lib.ResectParams(256, 12, 12, -1, 8, 0, 0, 0, 2.0)) == -1
    for name in ("X", "obs", "pi", "cam_ptr", "cam_obs", "ext", "cost", "inl", "info", "ws"):
        assert call(null=name) == -1, name
    for Kb in (np.diag([0.0, 1500.0, 1.0]), np.diag([1500.0, 1500.0, 2.0]), np.eye(3)[::-1], np.diag([math.nan, 1.0, 1.0])):
        assert call(Kh=Kb) == -1
    assert call(ws_bytes=wsb - 1) == -3
    # and the wrapper raises
    for kw in (dict(n_hyp=0), dict(n_hyp=5000), dict(threshold_px=math.nan), dict(polish_iters=-1)):
        with pytest.raises(ValueError):
            ops.resect_cameras(K, Xd, od, pd, cpd, cod, **kw)
    with pytest.raises(ValueError):
        ops.resect_cameras(np.eye(3)[::-1], Xd, od, pd, cpd, cod)
    with pytest.raises(ValueError):
        ops.resect_cameras(K, Xd, od, pd[:-1], cpd, cod)


def test_processor_resect_cameras_on_host_arrays():
    fx, _, whole = five(False)
    scs = fx["scenes"][:2]
    ext, masks, info = processor.resectCameras([s["X"] for s in scs], [s["obs"] for s in scs], ref.K_SCENE, seed=11)
    assert ext.shape == (2, 3, 4) and info.shape == (2, 6) and [m.shape for m in masks] == [(256,), (64,)] and masks[0].dtype == bool
    assert masks[0][:192].all() and not masks[0][192:].any() and masks[1][:40].all() and not masks[1][40:].any()
    for c in range(2):
        assert ref.rot_err_deg(ext[c][:, :3], scs[c]["R"]) < 0.05 and np.abs(ext[c][:, 3] - scs[c]["t"]).max() < 5e-3
    e0, m0, i0 = processor.resectCameras([], [], ref.K_SCENE)
    assert e0.shape == (0, 3, 4) and m0 == [] and i0.shape == (0, 6)
    few, mf, inf_ = processor.resectCameras([scs[0]["X"][:7]], [scs[0]["obs"][:7]], ref.K_SCENE)
    assert inf_[0, 0] == ref.TOO_FEW and np.isnan(few).all() and not mf[0].any()
    # a prior passes through a frame that cannot be estimated
    pr = np.hstack([scs[0]["R"], scs[0]["t"][:, None]])[None]
    kept, _, _ = processor.resectCameras([scs[0]["X"][:7]], [scs[0]["obs"][:7]], ref.K_SCENE, prior=pr)
    assert np.array_equal(kept, pr)
    with pytest.raises(ValueError):
        processor.resectCameras([scs[0]["X"]], [scs[0]["obs"][:-1]], ref.K_SCENE)


@functools.lru_cache(maxsize=None)
def clip():
    frames, ext, Kc = synth.render_orbit_frames(6, 640, 480, arc_deg=6.0)
    return dev(frames), ext, Kc


def test_run_with_resect_never_raises_a_cameras_cost():
    frames, ext, Kc = clip()
    pipe = ClipPipeline(480, 640, 600, batch=6)
    timers = {}
    out = pipe.run(frames, Kc, None, verify={}, poses={}, resect={}, max_nfev=8, timers=timers)
    rs = out["resect"]
    assert set(rs) == {"extrinsics", "cost", "info", "inliers_per_frame"} and timers["resect"] > 0.0
    E = rs["extrinsics"].cpu().numpy()
    info = rs["info"].cpu().numpy()
    assert E.shape == (6, 3, 4) and info.shape == (6, 6) and rs["inliers_per_frame"].shape == (6,) and np.isfinite(E).all()
    assert np.array_equal(rs["inliers_per_frame"].cpu().numpy(), info[:, 1])
    # per camera: the MSAC cost is not above the cost of the prior (the recovered pose) under the same score
    plain = pipe.run(frames, Kc, None, verify={}, poses={}, ba=False)
    prior = plain["poses"]["extrinsics"]
    by_hand = pipe.resect(Kc, plain["points0"], plain["track_ptr_dev"], plain["obs_frame_dev"], plain["obs_kp_dev"], plain["xy_dev"],
                          6, prior=prior)
    assert torch.equal(by_hand["extrinsics"], rs["extrinsics"]) and torch.equal(by_hand["info"], rs["info"])
    held = pipe.resect(Kc, plain["points0"], plain["track_ptr_dev"], plain["obs_frame_dev"], plain["obs_kp_dev"], plain["xy_dev"],
                       6, prior=prior, n_hyp=1, min_rows=10 ** 9)      # (every camera TOO_FEW: the prior passes through)
    assert torch.equal(held["extrinsics"], prior)
    cost = rs["cost"].cpu().numpy()
    coords, fi, pi = ops.flatten_tracks(plain["track_ptr_dev"], plain["obs_frame_dev"], plain["obs_kp_dev"], plain["xy_dev"])
    X, coords, fi, pi = (t.cpu().numpy() for t in (plain["points0"], coords, fi, pi))
    Pr = prior.cpu().numpy()
    for f in range(6):
        if info[f, 0] & (ref.TOO_FEW | ref.NO_MODEL):
            continue
        sel = (fi == f) & np.isfinite(X[pi]).all(axis=1)
        d2, inl, _ = ref.distance(ref.camera(Kc, Pr[f].reshape(1, 12)), X[pi[sel]], coords[sel], 4.0)
        c_prior = float(np.where(inl[0], d2[0], 4.0).sum())
        print(f"frame {f}: MSAC cost {cost[f]:.4f} (prior {c_prior:.4f}), info {info[f].tolist()}")
        assert info[f, 4] == sel.sum() and cost[f] <= c_prior * (1.0 + 1e-12)
    assert math.isfinite(out["ba"].cost) and out["n_tracks"] == plain["n_tracks"]
    for bad in (dict(nhyp=8), dict(ctx=None), dict(cam_base=1)):
        with pytest.raises(ValueError):
            pipe.run(frames, Kc, ext, resect=bad)


def test_run_without_resect_is_unchanged():
    frames, ext, Kc = clip()
    pipe = ClipPipeline(480, 640, 600, batch=6)
    timers = {}
    plain = pipe.run(frames, Kc, ext, max_nfev=6, timers=timers)
    none = pipe.run(frames, Kc, ext, max_nfev=6, resect=None)
    assert "resect" not in plain and "resect" not in none and "resect" not in timers
    assert torch.equal(plain["points0"], none["points0"]) and torch.equal(plain["ba"].cams, none["ba"].cams)
    assert torch.equal(plain["ba"].pts, none["ba"].pts)
    # with true extrinsics as the prior the resection runs and the tracks are the same tracks
    with_rs = pipe.run(frames, Kc, ext, ba=False, resect=dict(n_hyp=64))
    assert "resect" in with_rs and torch.equal(with_rs["track_ptr_dev"], plain["track_ptr_dev"])


def test_run_with_resect_under_multi_view_uses_the_unflagged_tracks():
    frames, ext, Kc = clip()
    pipe = ClipPipeline(480, 640, 600, batch=6)
    kw = dict(ba=False, triangulation="multi_view", cull=dict(max_reproj_px=2.0))
    plain = pipe.run(frames, Kc, ext, **kw)
    out = pipe.run(frames, Kc, ext, resect=dict(n_hyp=64), **kw)
    info = out["resect"]["info"].cpu().numpy()
    _, fi, pi = ops.flatten_tracks(plain["track_ptr_dev"], plain["obs_frame_dev"], plain["obs_kp_dev"], plain["xy_dev"])
    ok = (plain["track_flags"] == 0) & torch.isfinite(plain["points0"]).all(dim=1)
    want = torch.bincount(fi.long()[ok[pi.long()]], minlength=6).cpu().numpy()
    print(f"usable rows per frame {info[:, 4].tolist()} of {torch.bincount(fi.long(), minlength=6).tolist()}, flags {info[:, 0].tolist()}")
    assert 0 < ok.sum().item() < ok.numel() and np.array_equal(info[:, 4], want)
    assert out["track_flags"].shape == plain["track_flags"].shape and "kept_tracks" in out


def test_zz_report_the_worst_gaps():
    """Runs last in the file: the figures the bounds were taken from."""
    print("worst gaps over the file: " + ", ".join(f"{k} {v:.3e}" for k, v in WORST.items()))
