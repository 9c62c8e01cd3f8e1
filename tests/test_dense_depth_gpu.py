"""GPU: mm_depth_sweep and mm_depth_fuse through ops.depth_sweep / ops.depth_fuse, ClipPipeline.run(dense=...) and
processor.densePointCloud against the NumPy restatement and the fixtures of tests/test_dense_depth_cpu.py.

The contract is equality: plane, keep, origin, n_consistent, grey and the counts exactly; cost, depth and points bit for bit
(NaN in the same places).  Only + - * / sqrt floor rint and conversions occur, each correctly rounded on both sides, so no
pixel is excluded and there is no tolerance.

Shapes at the sweep's edges, with T = ops.SWEEP_TILE: images whose valid interior is 1, T-1, T, T+1 and 2T+3 pixels wide and
high, r in {1, 3}, D in {1, 2, 3, 17}, S in {1, 2, 4 with -1 padding}, min_sources 1 and 2.  Fuse: V in {1, 3, 5}, cap below,
equal to and above the count and 0, kept pixels on both sides of the scan's chunk boundaries, more chunk sums than one step of
the second scan level takes, nothing kept, everything kept.
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
import test_dense_depth_cpu as ref  # noqa: E402
from meatmodeler_amd import ops, pipeline, processor, synth  # noqa: E402
from meatmodeler_amd.bundleAdjuster import _rodrigues_matrix  # noqa: E402
from meatmodeler_amd.pipeline import ClipPipeline  # noqa: E402

DEV = torch.device("cuda", 0)
T = ops.SWEEP_TILE


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def same_bits(got, want):
    """Float arrays equal bit for bit, NaN in the same places (a NaN's payload is not part of the contract)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    nan = np.isnan(want)
    word = np.uint32 if got.dtype == np.float32 else np.uint64
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(word)[~nan], want.view(word)[~nan])


def gpu_sweep(case):
    out = ops.depth_sweep(dev(case["frames"]), case["K"], case["ext"], case["ref"], case["src"], case["ranges"], planes=case["D"],
                          radius=case["r"], **case["kw"])
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() if torch.is_tensor(v) else v for k, v in out.items()}


def sweep_agrees(case):
    got = gpu_sweep(case)
    (depth, cost, plane), (AB, w0, dw) = ref.restate_sweep(case)
    assert got["AB"].tobytes() == AB.tobytes() and got["w0"].tobytes() == w0.tobytes() and got["dw"].tobytes() == dw.tobytes()
    assert np.array_equal(got["plane"], plane), (int((got["plane"] != plane).sum()), plane.size)
    assert same_bits(got["cost"], cost) and same_bits(got["depth"], depth)
    return got


# ------------------------------------------------------------------------------------------------ sweep: shapes at the edges

@functools.lru_cache(maxsize=None)
def tiny_clip(width, height):
    """Five frames of the scene at this size, on an arc short enough that the windows of a 3 x 3 image still land inside."""
    return synth.render_orbit_frames(5, width, height, arc_deg=1.0, tex_size=512)


# (interior width, interior height, r, D, source slots, min_sources)
EDGES = [(1, 1, 1, 1, [1], 1), (1, T + 1, 3, 2, [1, 3], 1), (T - 1, T, 1, 3, [1, -1, 3, 0], 2), (T, T - 1, 3, 17, [3], 1),
         (T, T, 1, 17, [-1, 1, 3, -1], 1), (T + 1, T + 1, 3, 3, [1, 3], 2), (T + 1, 1, 1, 2, [0, 1, 3, 4], 2),
         (2 * T + 3, T - 1, 3, 1, [-1, -1, 1, 3], 1), (2 * T + 3, 2 * T + 3, 1, 17, [1, 3], 1), (2 * T + 3, 2 * T + 3, 3, 17, [1, 3, 0, -1], 2)]


@pytest.mark.parametrize("iw, ih, r, D, src, min_sources", EDGES, ids=lambda v: "".join(str(v).split()))
def test_sweep_at_the_tile_edges(iw, ih, r, D, src, min_sources):
    W, H = iw + 2 * r, ih + 2 * r
    frames, ext, K = tiny_clip(W, H)
    case = dict(frames=frames, K=K, ext=ext, ref=np.array([2]), src=np.array([src]), ranges=np.array([[4.0, 14.0]]), D=D, r=r,
                kw=dict(min_sources=min_sources, var_min=1.0))
    got = sweep_agrees(case)
    assert np.isnan(got["depth"][0, :r]).all() and np.isnan(got["depth"][0, :, :r]).all() and (got["plane"][0, H - r:] == -1).all()
    if iw > 1 and ih > 1:
        assert (got["plane"][0, r:H - r, r:W - r] >= 0).any()          # (the case measures something)


def test_sweep_on_several_views_and_tiles():
    sm = ref.small_scene()
    case = dict(frames=sm["frames"], K=sm["K"], ext=sm["ext"], ref=sm["ref"], src=sm["src"], ranges=sm["ranges"], D=sm["planes"],
                r=sm["radius"], kw={})
    got = sweep_agrees(case)
    assert (got["plane"] >= 0).mean() > 0.3
    # the same call twice gives the same bits
    again = gpu_sweep(case)
    assert all(got[k].tobytes() == again[k].tobytes() for k in ("depth", "cost", "plane"))
    # V views in one call give the same bits as V calls of one view
    for v in range(len(sm["ref"])):
        one = gpu_sweep(dict(case, ref=sm["ref"][v:v + 1], src=sm["src"][v:v + 1], ranges=sm["ranges"][v:v + 1]))
        assert all(one[k][0].tobytes() == got[k][v].tobytes() for k in ("depth", "cost", "plane")), v


def test_sweep_with_the_widest_window_and_a_skewed_k():
    sm = ref.small_scene()
    K = sm["K"].copy()
    K[0, 1] = 0.75
    sweep_agrees(dict(frames=sm["frames"], K=K, ext=sm["ext"], ref=np.array([1, 3]), src=np.array([[0, 2, -1], [2, 4, 1]]),
                      ranges=np.array([[4.0, 14.0], [3.0, 30.0]]), D=5, r=ops.SWEEP_MAX_RADIUS, kw=dict(var_min=0.0)))


@pytest.mark.parametrize("name", ["twin", "turned_away", "behind_on_a_part", "constant", "one_source_is_enough", "both_sources_needed"])
def test_the_planted_sweeps(name):
    case = ref.planted_sweeps()[name]
    got = sweep_agrees(case)
    if name == "twin":
        seen = got["plane"][0] >= 0
        assert seen.mean() > 0.4 and (got["plane"][0][seen] == 0).all() and (got["depth"][0][seen] == np.float32(4.0)).all()
    if name in ("turned_away", "constant"):
        assert np.isnan(got["depth"]).all() and np.isnan(got["cost"]).all() and (got["plane"] == -1).all()


# ------------------------------------------------------------------------------------------------ fuse

def gpu_fuse(a):
    out = ops.depth_fuse(dev(a["depth"]), dev(a["cost"]), a["K"], a["ext"], a["nbr"], dev(a["grey"]),
                         **{k: v for k, v in a.items() if k in ("max_cost", "eps_depth", "tau_px", "min_consistent", "cap")})
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() if torch.is_tensor(v) else v for k, v in out.items()}


def fuse_agrees(got, want):
    assert tuple(got["counts"]) == tuple(want["counts"]) and got["n"] == want["n"]
    assert np.array_equal(got["keep"], want["keep"])
    for k in ("origin", "n_consistent", "grey"):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    assert same_bits(got["points"], want["points"])


@pytest.mark.parametrize("name", ["three_views", "cap_below", "cap_equal", "cap_above", "cap_zero", "five_views", "one_view_nothing_kept",
                                  "one_view_everything_kept", "nothing_is_a_candidate", "no_neighbour_table", "strict",
                                  "second_scan_level"])
def test_fuse_against_the_restatement(name):
    fx = ref.fuse_fixtures()[name]
    assert ref.margins_hold(fx["want"])
    got = gpu_fuse(fx["args"])
    fuse_agrees(got, fx["want"])
    if name == "three_views":
        again = gpu_fuse(fx["args"])                                   # the same call twice gives the same bits
        assert all(got[k].tobytes() == again[k].tobytes() for k in ("points", "grey", "origin", "n_consistent", "keep"))


def test_fuse_rows_beyond_cap_are_not_written():
    a = ref.fuse_fixtures()["three_views"]["args"]
    want = ref.fuse_fixtures()["three_views"]["want"]
    cap = want["n"] - 100
    V, H, W = a["depth"].shape
    # through the library, with buffers longer than cap and a pattern in them
    from meatmodeler_amd import _lib
    import ctypes as C
    ctx = _lib.default_context()
    rows = want["n"] + 8
    pts = torch.full((rows, 3), -7.0, dtype=torch.float64, device=DEV)
    grey = torch.full((rows,), 201, dtype=torch.uint8, device=DEV)
    org = torch.full((rows, 2), -7, dtype=torch.int32, device=DEV)
    ncs = torch.full((rows,), -7, dtype=torch.int32, device=DEV)
    keep = torch.zeros((V, H, W), dtype=torch.uint8, device=DEV)
    counts = torch.zeros(2, dtype=torch.int64, device=DEV)
    ws = torch.empty(_lib.lib.mm_depth_fuse_workspace_bytes(V, H, W), dtype=torch.uint8, device=DEV)
    d, c, g, e, nb = dev(a["depth"]), dev(a["cost"]), dev(a["grey"]), dev(np.asarray(a["ext"], np.float64)[:, :3, :]), dev(a["nbr"])
    Kh = np.ascontiguousarray(a["K"], np.float64).reshape(9)
    prm = _lib.FuseParams(a["min_consistent"], 0, 0.4, a["eps_depth"], a["tau_px"])
    ctx.check(_lib.lib.mm_depth_fuse(ctx.h, d.data_ptr(), c.data_ptr(), V, H, W, e.data_ptr(), Kh.ctypes.data_as(_lib.c_f64p), nb.data_ptr(),
                                     nb.shape[1], g.data_ptr(), C.byref(prm), cap, pts.data_ptr(), grey.data_ptr(), org.data_ptr(),
                                     ncs.data_ptr(), keep.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel()), "mm_depth_fuse")
    torch.cuda.synchronize()
    assert counts.tolist() == list(want["counts"])
    assert same_bits(pts[:cap].cpu().numpy(), want["points"][:cap]) and (pts[cap:] == -7.0).all()
    assert (grey[cap:] == 201).all() and (org[cap:] == -7).all() and (ncs[cap:] == -7).all()
    assert np.array_equal(org[:cap].cpu().numpy(), want["origin"][:cap])


def test_fuse_of_v_views_is_v_fuses_of_one_view_when_no_view_is_asked():
    fx = ref.fuse_fixtures()["five_views"]["args"]
    a = dict(fx, nbr=np.full((5, 2), -1, np.int32), min_consistent=0)
    whole = gpu_fuse(a)
    fuse_agrees(whole, ref.fuse(**a))
    at = 0
    for v in range(5):
        one = gpu_fuse(dict(a, depth=a["depth"][v:v + 1], cost=a["cost"][v:v + 1], ext=a["ext"][v:v + 1], grey=a["grey"][v:v + 1],
                            nbr=a["nbr"][v:v + 1]))
        n = one["n"]
        assert one["points"].tobytes() == whole["points"][at:at + n].tobytes() and np.array_equal(one["keep"][0], whole["keep"][v])
        assert np.array_equal(one["origin"][:, 1], whole["origin"][at:at + n, 1]) and (whole["origin"][at:at + n, 0] == v).all()
        at += n
    assert at == whole["n"]


# ------------------------------------------------------------------------------------------------ through the interface

DENSE = dict(every=1, sources=4, gap=1, neighbours=4, planes=16, radius=2, downscale=2, min_points=8, eps_depth=0.02, tau_px=1.5)


@functools.lru_cache(maxsize=None)
def clip_run():
    """The 7-frame clip of the issue (arc 35 degrees) at 320 x 240 -- the detector needs the room -- which the stage reduces to
    the fixture's 160 x 120; run with the adjustment, the filter behind it (a view's depth range is the min / max over its
    points: one outlier widens it) and the dense stage."""
    frames, ext, K = synth.render_orbit_frames(7, 320, 240, arc_deg=35.0)
    pipe = ClipPipeline(240, 320, 1500, batch=7, device=DEV)
    timers = {}
    out = pipe.run(dev(frames), K, ext, ba=True, refine={}, dense=DENSE, timers=timers)
    torch.cuda.synchronize()
    return frames, ext, K, pipe, out, timers


def test_run_with_dense_returns_the_restated_cloud():
    frames, ext, K, pipe, out, timers = clip_run()
    dn = out["dense"]
    assert "dense" in timers and timers["dense"] > 0
    assert dn["views"].tolist() == list(range(7)) and (dn["flags"] == 0).all()
    # the stage ran at the final cameras and points, the refined ones: its ranges are those of the points the filter kept, in
    # the cameras of the last solve, over the observations it kept
    res = out["refine"]["ba"]
    cams = res.cams.reshape(7, 6).cpu().numpy()
    E = np.stack([np.concatenate([_rodrigues_matrix(c[:3]), c[3:, None]], axis=1) for c in cams])
    pts = res.pts.reshape(-1, 3).cpu().numpy()
    ClipPipeline.tracks_to_host(out)
    point_map, obs_map = out["refine"]["point_map"].cpu().numpy(), out["refine"]["obs_map"].cpu().numpy()
    assert pts.shape[0] == point_map.size <= out["n_tracks"]
    new = np.full(out["n_tracks"], -1)
    new[point_map] = np.arange(point_map.size)
    fi = out["obs_frame"][obs_map]
    pi = new[np.repeat(np.arange(out["n_tracks"]), np.diff(out["track_ptr"]))[obs_map]]
    assert pi.min() >= 0
    z = np.einsum("oj,oj->o", E[fi, 2, :3], pts[pi]) + E[fi, 2, 3]
    print("tracks", out["n_tracks"], "kept points", point_map.size, "ranges", np.round(dn["range"], 3).tolist(), "counts", dn["counts"])
    for f in range(7):
        zf = z[(fi == f) & np.isfinite(z) & (z > 0)]
        assert zf.size >= DENSE["min_points"]
        assert np.allclose(dn["range"][f], [zf.min() / 1.1, zf.max() * 1.1], rtol=1e-12, atol=0)
    # the restatement on the reduced frames, the scaled K and those cameras and ranges
    f = frames.astype(np.int64)
    small = ((f[:, 0::2, 0::2] + f[:, 0::2, 1::2] + f[:, 1::2, 0::2] + f[:, 1::2, 1::2] + 2) >> 2).astype(np.uint8)
    Ks = dn["K"]
    assert np.array_equal(Ks, [[K[0, 0] / 2, 0.0, K[0, 2] / 2 - 0.25], [0.0, K[1, 1] / 2, K[1, 2] / 2 - 0.25], [0.0, 0.0, 1.0]])
    views, src, nbr = pipeline.dense_views(7, 1, 4, 1, 4)
    AB, w0, dw = ops.sweep_tables(Ks, E, views, src, dn["range"], DENSE["planes"])
    depth, cost, plane = ref.sweep(small, AB, w0, dw, views, src, DENSE["planes"], DENSE["radius"])
    assert np.array_equal(dn["plane"].cpu().numpy(), plane)
    assert same_bits(dn["depth"].cpu().numpy(), depth) and same_bits(dn["cost"].cpu().numpy(), cost)
    want = ref.fuse(depth, cost, Ks, E, nbr, small, eps_depth=DENSE["eps_depth"], tau_px=DENSE["tau_px"])
    assert ref.margins_hold(want) and want["n"] > 5000
    got = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in dn.items()}
    got["n"] = got["points"].shape[0]
    fuse_agrees(got, want)
    # and the cloud lies on the scene.  With every camera free the adjustment fixes no gauge: the reconstruction is the scene
    # up to a similarity, which leaves a pixel's depth in its own camera unchanged up to the one scale -- taken here as the
    # median ratio -- so most points are within 5 % of the analytic depth of their pixel, rescaled
    truth = np.stack([synth.render_depth(ext[v], Ks, 160, 120) for v in range(7)])
    o = got["origin"]
    d = depth[o[:, 0], o[:, 1] // 160, o[:, 1] % 160].astype(np.float64)
    t = truth[o[:, 0], o[:, 1] // 160, o[:, 1] % 160]
    scale = np.median((d / t)[np.isfinite(t)])
    share = (np.abs(d / scale - t) / t <= 0.05).mean()
    print("scale", scale, "within 5 %", share)
    assert share > 0.8
    # the facade returns the same points from the same cameras and ranges
    p, g = processor.densePointCloud(frames, K, E, dn["range"], **DENSE)
    assert p.tobytes() == got["points"].tobytes() and np.array_equal(g, got["grey"])


def test_run_without_dense_launches_nothing_of_it():
    frames, ext, K, pipe, _, _ = clip_run()
    ctx = pipe.ctx
    ctx.profile(1)
    try:
        timers = {}
        out = pipe.run(dev(frames), K, ext, ba=False, timers=timers)
        torch.cuda.synchronize()
        names = set(ctx.profile_report())
    finally:
        ctx.profile(0)
    assert "dense" not in out and "dense" not in timers
    assert names and not any(n.startswith(("ds_", "df_")) for n in names)
    # with ba=False the stage runs at the initial cameras and points
    out = pipe.run(dev(frames), K, ext, ba=False, dense=dict(DENSE, max_points=1000))
    dn = out["dense"]
    assert "ba" not in out and dn["points"].shape == (1000, 3) and dn["counts"][0] > 1000 and (dn["flags"] == 0).all()


def test_a_view_with_too_few_points_is_skipped_and_flagged():
    frames, ext, K, pipe, out, _ = clip_run()
    rng = np.array(out["dense"]["range"])
    rng[3] = np.nan
    dn = pipe.dense(dev(frames), K, ext, rng, **DENSE)
    assert dn["flags"].tolist() == [0, 0, 0, pipeline.DENSE_FEW_POINTS, 0, 0, 0] and np.isnan(dn["range"][3]).all()
    assert (dn["plane"][3] == -1).all() and torch.isnan(dn["depth"][3]).all() and (dn["plane"][2] >= 0).any()
    assert not (dn["origin"][:, 0] == 3).any() and dn["points"].shape[0] > 0
