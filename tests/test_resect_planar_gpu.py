"""GPU: mm_resect_planar through ops.resect_planar, ops.resect_cameras(planar=...), processor.poseEstimationFromCorners and
ClipPipeline.run(resect=dict(planar=...)) against the NumPy restatement of tests/test_resect_planar_cpu.py.

Shapes: n_cams in {0, 1, 3, 4, 5}; usable rows per camera in {0, 3, 4, 7, 8, 9, 63, 64, 65, 255, 256, 257, 300} (each with
three rows that are not usable; 8 is the row floor); n_hyp in {1, 63, 64, 65, 256} -- the wave, workgroup-stride and LDS-tile
edges of a 256-thread camera workgroup.  The five-camera call holds a planar camera with outliers, a cube camera (refused), a
collinear one, one with 7 usable rows and a far, tilted planar one with malformed rows and a masked point, with and without priors.

Exact: flags, n_inliers, best_h, the valid-hypothesis count, n_use, accepted polish steps, the inlier bytes and which of them
were left untouched.  The fixtures keep every decision away from a rounding (the margins asserted in the CPU file), so a
count that differs is not rounding.  The g6 chessboard frames run the polish to convergence, where the last trials decide on
roundings: their accepted-step count is not compared.
With a tolerance: extrinsics and plane (absolute), cost (relative).  Started at 1e-9; the first run on the MI355X measured the
worst gap over every comparison of this file as 0 on all three: resect.hip is compiled without FMA contraction, +, *, / and
sqrt are correctly rounded on both sides and the restatement follows the kernels' order of operations, so they compute the
same bits.  The committed bounds are the measured gaps with a margin of ten -- zero: equality.
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
import test_resect_cameras_cpu as gen  # noqa: E402
import test_resect_planar_cpu as ref  # noqa: E402
from meatmodeler_amd import _lib, ops, processor, synth  # noqa: E402
from meatmodeler_amd.pipeline import ClipPipeline  # noqa: E402

DEV = torch.device("cuda", 0)
# measured gap to the restatement x 10 (module docstring)
EXT_TOL = 0.0
COST_TOL = 0.0
PLANE_TOL = 0.0
WORST = dict(ext=0.0, cost=0.0, plane=0.0)
UNTOUCHED = ref.UNTOUCHED


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def device_args(K, X, obs, pi, cam_ptr, cam_obs, pt_ok=None, prior=None):
    return (K, dev(np.asarray(X, np.float64)), dev(np.asarray(obs, np.float64)), dev(np.asarray(pi, np.int32)),
            dev(np.asarray(cam_ptr, np.int32)), dev(np.asarray(cam_obs, np.int32))), dict(
                pt_ok=None if pt_ok is None else dev(pt_ok), prior=None if prior is None else dev(prior))


def run(K, X, obs, pi, cam_ptr, cam_obs, pt_ok=None, prior=None, inlier=None, **kw):
    """-> (extrinsics, cost, inlier, info, plane) as NumPy arrays; the inlier bytes start as UNTOUCHED (or as `inlier`)."""
    inl = torch.full((len(obs),), UNTOUCHED, dtype=torch.uint8, device=DEV) if inlier is None else dev(inlier)
    a, k = device_args(K, X, obs, pi, cam_ptr, cam_obs, pt_ok, prior)
    return tuple(t.cpu().numpy() for t in ops.resect_planar(*a, inlier=inl, **k, **kw))


def check(got, want, what="", polish_count=True):
    ext, cost, inlier, info, plane = got
    wext, wcost, winlier, winfo, _, wplane = want
    cols = slice(0, 6) if polish_count else slice(0, 5)
    assert np.array_equal(info[:, cols], winfo[:, cols]), (what, info, winfo)
    assert np.array_equal(inlier, winlier), (what, np.flatnonzero(inlier != winlier))
    assert np.array_equal(np.isnan(ext), np.isnan(wext)) and np.array_equal(np.isnan(cost), np.isnan(wcost)), what
    assert np.array_equal(np.isnan(plane), np.isnan(wplane)), (what, plane, wplane)
    for c in range(len(info)):
        g = dict(ext=0.0, cost=0.0, plane=0.0)
        if np.isfinite(wplane[c]).all():
            g["plane"] = float(np.abs(plane[c] - wplane[c]).max())
        if not np.isnan(wext[c]).any():
            g["ext"] = float(np.abs(ext[c] - wext[c]).max())
        if not np.isnan(wcost[c]):
            g["cost"] = float(abs(cost[c] / wcost[c] - 1.0)) if wcost[c] != 0 else float(abs(cost[c]))
        for k, v in g.items():
            WORST[k] = max(WORST[k], v)
        print(f"{what} camera {c}: gaps ext {g['ext']:.2e}, cost {g['cost']:.2e}, plane {g['plane']:.2e}")
        assert g["ext"] <= EXT_TOL and g["cost"] <= COST_TOL and g["plane"] <= PLANE_TOL, (what, c, g)


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
    assert got[3][:, 0].tolist() == [ref.PLANAR, 0, ref.PLANAR | ref.NO_MODEL, ref.TOO_FEW, ref.PLANAR | ref.MALFORMED]
    for c in (0, 4):
        R = got[0][c][:, :3]
        assert abs(np.linalg.det(R) - 1.0) < 1e-9 and np.abs(R @ R.T - np.eye(3)).max() < 1e-9
        assert gen.rot_err_deg(R, fx["scenes"][c]["R"]) < 0.3


@pytest.mark.parametrize("n", ref.BOUNDARY_ROWS)
def test_usable_row_boundaries(n):
    fx = ref.boundary_fixture(n)
    got = run(*fx["args"], n_hyp=64, seed=ref.ROW_SEED.get(n, 0), **fx["kw"])
    check(got, ref.boundary_reference(n), f"rows={n}")
    assert got[3][0, 4] == n and bool(got[3][0, 0] & ref.TOO_FEW) == (n < 8) and bool(got[3][0, 0] & ref.PLANAR) == (n >= 8)
    assert (got[2] == UNTOUCHED).sum() == (3 if n >= 8 else n + 3)


def test_random_points_under_the_default_collinear_tol():
    fx = ref.boundary_fixture(64)
    got = run(*fx["args"], n_hyp=64, seed=ref.DEFAULT_TOL_SEED, **dict(fx["kw"], collinear_tol=ref.COLLINEAR_TOL))
    check(got, ref.default_tol_reference(), "default collinear_tol")
    same_default = run(*fx["args"], n_hyp=64, seed=ref.DEFAULT_TOL_SEED, pt_ok=fx["kw"]["pt_ok"], polish_iters=ref.POLISH)
    assert same(same_default, got)


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
        assert same((part[0], part[1], part[3], part[4]), (whole[0][a:b], whole[1][a:b], whole[3][a:b], whole[4][a:b])), (a, b)
        touched = np.zeros(len(obs), bool)
        rows = cam_obs[cam_ptr[a]:cam_ptr[b]]
        touched[rows[(rows >= 0) & (rows < len(obs))]] = True
        assert np.array_equal(part[2][touched], whole[2][touched]) and (part[2][~touched] == UNTOUCHED).all()
    # no camera: shapes, and at the ABI no launch and no pointer needed
    ext, cost, inlier, info, plane = run(K, X, obs, pi, cam_ptr[:1], cam_obs)
    assert ext.shape == (0, 3, 4) and cost.shape == (0,) and info.shape == (0, 6) and plane.shape == (0, 6)
    assert (inlier == UNTOUCHED).all()
    prm = _lib.ResectPlanarParams(256, 8, 12, 2, 8, 0, 0, 0, 2.0, 1e-2, 1e-3)
    Kh = np.ascontiguousarray(K.ravel())
    assert _lib.lib.mm_resect_planar(_lib.default_context().h, Kh.ctypes.data_as(_lib.c_f64p), None, 0, None, None, 0, None, None, 0, 0,
                                     None, None, C.byref(prm), None, None, None, None, None, None, 0) == 0


def test_repeats_bit_for_bit_and_leaves_refused_bytes_untouched():
    fx, _, whole = five(True)
    assert same(run(*fx["args"], **fx["kw"]), whole)
    before = (np.arange(len(fx["args"][2])) % 5 + 2).astype(np.uint8)
    got = run(*fx["args"], inlier=before, **fx["kw"])
    want = ref.resect_planar_numpy(*fx["args"], inlier=before, **fx["kw"])
    assert np.array_equal(got[2], want[2])
    cam_ptr = fx["args"][4]
    for c in (1, 3):
        lo, hi = int(cam_ptr[c]), int(cam_ptr[c + 1])
        assert np.array_equal(got[2][lo:hi], before[lo:hi])


def test_g6_chessboard_frames_without_a_prior_through_the_kernel():
    fx = gen.g6_fixture()
    got = run(*fx["args"], seed=ref.G6_SEED, **fx["kw"])
    want = ref.g6_reference()
    ext, cost, inlier, info, plane = got
    gap = np.abs(ext - fx["result"]).max()
    print(f"g6 without a prior: |polished - result| = {gap:.2e}, |polished - restatement| = {np.abs(ext - want[0]).max():.2e}, "
          f"accepted steps {info[:, 5].tolist()} (restatement {want[3][:, 5].tolist()}), half the summed cost {0.5 * cost.sum():.5f}")
    assert (info[:, 0] == ref.PLANAR).all() and (info[:, 1] == 12).all() and (inlier == 1).all()
    assert gap <= 1e-8 and abs(0.5 * cost.sum() - 2.0049) < 1e-4
    assert np.array_equal(info[:, :5], want[3][:, :5]) and np.abs(ext - want[0]).max() <= 1e-9
    assert np.array_equal(plane, want[5])
    # the default sampling key as well, and what the general resection makes of the same input
    plain = run(*fx["args"], **fx["kw"])
    assert (plain[3][:, 0] == ref.PLANAR).all() and np.abs(plain[0] - fx["result"]).max() <= 1e-8
    a, k = device_args(*fx["args"])
    general = ops.resect_cameras(*a, **fx["kw"])
    assert (general[3][:, 0] == ref.NO_MODEL).all() and torch.isnan(general[0]).all()


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
    plane = torch.zeros((n_cams, 6), dtype=torch.float64, device=DEV)
    wsb = _lib.lib.mm_resect_planar_workspace_bytes(n_cams, 256, n_rows)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    h = _lib.default_context().h
    p = _lib.ptr

    def params(n_hyp=256, refit=2, tau=2.0, ptol=1e-2, ctol=1e-3):
        return _lib.ResectPlanarParams(n_hyp, 8, 12, refit, 8, 0, 0, 0, tau, ptol, ctol)

    def call(prm=None, Kh=None, ws_bytes=wsb, null=None):
        prm = prm or params()
        Kh = np.ascontiguousarray(K.ravel() if Kh is None else np.asarray(Kh, float).ravel())
        a = dict(X=p(Xd), obs=p(od), pi=p(pd), cam_ptr=p(cpd), cam_obs=p(cod), ext=p(ext), cost=p(cost), inl=p(inl), info=p(info),
                 plane=p(plane), ws=p(ws))
        if null:
            a[null] = None
        return _lib.lib.mm_resect_planar(h, Kh.ctypes.data_as(_lib.c_f64p), a["X"], len(X), a["obs"], a["pi"], len(obs),
                                         a["cam_ptr"], a["cam_obs"], n_rows, n_cams, None, None, C.byref(prm), a["ext"], a["cost"],
                                         a["inl"], a["info"], a["plane"], a["ws"], ws_bytes)

    assert call() == 0
    for n_hyp in (0, -1, 4097):
        assert call(params(n_hyp=n_hyp)) == -1
    for tau in (math.nan, -1.0):
        assert call(params(tau=tau)) == -1
    assert call(params(refit=-1)) == -1
    for tol in (math.nan, -1e-3, math.inf):
        assert call(params(ptol=tol)) == -1 and call(params(ctol=tol)) == -1
    for name in ("X", "obs", "pi", "cam_ptr", "cam_obs", "ext", "cost", "inl", "info", "plane", "ws"):
        assert call(null=name) == -1, name
    for Kb in (np.diag([0.0, 1500.0, 1.0]), np.diag([1500.0, 1500.0, 2.0]), np.eye(3)[::-1], np.diag([math.nan, 1.0, 1.0])):
        assert call(Kh=Kb) == -1
    assert call(ws_bytes=wsb - 1) == -3
    # and the wrapper raises
    for kw in (dict(n_hyp=0), dict(n_hyp=5000), dict(threshold_px=math.nan), dict(polish_iters=-1), dict(planar_tol=-1.0),
               dict(planar_tol=math.nan), dict(collinear_tol=-1.0), dict(collinear_tol=math.nan)):
        with pytest.raises(ValueError):
            ops.resect_planar(K, Xd, od, pd, cpd, cod, **kw)
    with pytest.raises(ValueError):
        ops.resect_planar(np.eye(3)[::-1], Xd, od, pd, cpd, cod)
    with pytest.raises(ValueError):
        ops.resect_planar(K, Xd, od, pd[:-1], cpd, cod)
    with pytest.raises(ValueError):
        ops.resect_cameras(K, Xd, od, pd, cpd, cod, planar="yes")


def test_resect_cameras_planar_auto_on_a_mixed_call():
    fx, want, planar = five(True)
    a, k = device_args(*fx["args"], pt_ok=fx["kw"]["pt_ok"], prior=fx["kw"]["prior"])
    kw = dict(seed=fx["kw"]["seed"], polish_iters=fx["kw"]["polish_iters"], collinear_tol=fx["kw"]["collinear_tol"], min_rows=8)

    def fresh():
        return torch.full((len(fx["args"][2]),), UNTOUCHED, dtype=torch.uint8, device=DEV)

    today = [t.cpu().numpy() for t in ops.resect_cameras(*a, inlier=fresh(), **k, seed=kw["seed"], polish_iters=kw["polish_iters"],
                                                         min_rows=8)]
    none = [t.cpu().numpy() for t in ops.resect_cameras(*a, inlier=fresh(), planar=None, **k, **kw)]
    assert same(none, today)
    auto = [t.cpu().numpy() for t in ops.resect_cameras(*a, inlier=fresh(), planar="auto", **k, **kw)]
    only = [t.cpu().numpy() for t in ops.resect_cameras(*a, inlier=fresh(), planar="only", **k, **kw)]
    assert len(auto) == len(only) == 4 and same(only, planar[:4])
    cam_ptr, cam_obs = fx["args"][4], fx["args"][5]
    took = (planar[3][:, 0] & ref.PLANAR) != 0
    assert took.tolist() == [True, False, True, False, True]
    for c in range(5):
        src = planar if took[c] else today
        assert same((auto[0][c], auto[1][c], auto[3][c]), (src[0][c], src[1][c], src[3][c])), c
        rows = cam_obs[cam_ptr[c]:cam_ptr[c + 1]]
        rows = rows[(rows >= 0) & (rows < len(auto[2]))]
        assert np.array_equal(auto[2][rows], src[2][rows]), c
    assert (auto[2][-4:] == UNTOUCHED).all()
    # the general call alone has no valid hypothesis on the planar camera 0 (its prior carried it); "auto" has
    assert today[3][0, 3] == 0 and auto[3][0, 3] > 0 and auto[3][0, 0] == ref.PLANAR


def test_pose_estimation_from_corners_on_the_g6_frames():
    fx = gen.g6_fixture()
    K, obs = fx["args"][0], fx["args"][2]
    frames = [obs[12 * f:12 * f + 12].reshape(12, 1, 2) for f in range(5)]
    out = processor.poseEstimationFromCorners(frames, (4, 3), 2, K, threshold_px=50.0)
    assert isinstance(out, list) and len(out) == 5
    for f, (rvec, tvec, E, Pm) in enumerate(out):
        assert rvec.shape == (3, 1) and tvec.shape == (3, 1) and E.shape == (3, 4) and Pm.shape == (3, 4)
        assert np.abs(E - fx["result"][f]).max() <= 1e-8
        assert np.abs(gen.rodrigues(rvec.ravel()) - E[:, :3]).max() < 1e-12 and np.array_equal(tvec.ravel(), E[:, 3])
        assert np.array_equal(Pm, np.asarray(K, np.float64).reshape(3, 3) @ E)
    one = processor.poseEstimationFromCorners(frames[0], (4, 3), 2, K, threshold_px=50.0)
    assert isinstance(one, tuple) and np.array_equal(one[2], out[0][2])
    # a degenerate input: every corner at the same pixel fits no homography
    assert processor.poseEstimationFromCorners(np.full((12, 2), 300.0), (4, 3), 2, K) is None
    mixed = processor.poseEstimationFromCorners([frames[1], np.full((12, 2), 300.0)], (4, 3), 2, K, threshold_px=50.0)
    assert mixed[1] is None and np.array_equal(mixed[0][2], out[1][2])
    with pytest.raises(ValueError):
        processor.poseEstimationFromCorners(frames[0][:-1], (4, 3), 2, K)
    # resectCameras passes `planar` on
    X = fx["args"][1]
    ext, masks, info = processor.resectCameras([X] * 5, [obs[12 * f:12 * f + 12] for f in range(5)], K, planar="auto", threshold_px=50.0)
    assert (info[:, 0] == ref.PLANAR).all() and all(m.all() for m in masks) and np.abs(ext - fx["result"]).max() <= 1e-8


@functools.lru_cache(maxsize=None)
def clip():
    frames, ext, Kc = synth.render_orbit_frames(6, 640, 480, arc_deg=6.0)
    return dev(frames), ext, Kc


def test_run_with_planar_resect_and_run_without_it():
    frames, ext, Kc = clip()
    pipe = ClipPipeline(480, 640, 600, batch=6)
    plain = pipe.run(frames, Kc, ext, ba=False, resect=dict(n_hyp=64))
    auto = pipe.run(frames, Kc, ext, ba=False, resect=dict(n_hyp=64, planar="auto"))
    rs, ra = plain["resect"], auto["resect"]
    assert set(ra) == {"extrinsics", "cost", "info", "inliers_per_frame"}
    info, ainfo = rs["info"].cpu().numpy(), ra["info"].cpu().numpy()
    took = (ainfo[:, 0] & ref.PLANAR) != 0
    print(f"planar verdicts per frame {took.tolist()}, flags {ainfo[:, 0].tolist()} (general {info[:, 0].tolist()})")
    # a frame the planar call refused is the general call's, bit for bit
    keep = torch.as_tensor(~took).to(DEV)
    assert torch.equal(ra["extrinsics"][keep], rs["extrinsics"][keep]) and torch.equal(ra["info"][keep], rs["info"][keep])
    assert np.isfinite(ra["extrinsics"].cpu().numpy()).all()
    only = pipe.run(frames, Kc, ext, ba=False, resect=dict(n_hyp=64, planar="only", planar_tol=1e-3, collinear_tol=1e-4))
    assert only["resect"]["info"].shape == (6, 6)
    # without `planar` nothing changes: the default, {} and planar=None launch the same call
    none = pipe.run(frames, Kc, ext, ba=False, resect=dict(n_hyp=64, planar=None))
    assert torch.equal(none["resect"]["extrinsics"], rs["extrinsics"]) and torch.equal(none["resect"]["info"], rs["info"])
    bare, bare2 = pipe.run(frames, Kc, ext, max_nfev=6), pipe.run(frames, Kc, ext, max_nfev=6, resect=None)
    assert "resect" not in bare and torch.equal(bare["ba"].cams, bare2["ba"].cams) and torch.equal(bare["points0"], bare2["points0"])
    for bad in (dict(planar="both"), dict(planar_tolerance=1.0)):
        with pytest.raises(ValueError):
            pipe.run(frames, Kc, ext, resect=bad)


def test_zz_report_the_worst_gaps():
    """Runs last in the file: the figures the bounds were taken from."""
    print("worst gaps over the file: " + ", ".join(f"{k} {v:.3e}" for k, v in WORST.items()))
