"""Batched clip pipeline: the hot path of `processor.process` (reference processor.py:356-470) run over a whole
clip with device-resident state — detect all frames, match all consecutive pairs, link tracks, triangulate, bundle
adjust.  Same stages and semantics as the per-keyframe drop-in functions in `processor.py`, but frames, descriptors
and key points stay in HBM and each stage is a few large launches instead of one small launch per keyframe.

Keyframe gating, calibration and PnP are outside the scope: the caller provides K and one extrinsic
per frame (the reference gets them from calibrate / poseEstimation / adjustPose, processor.py:422-448) -- or, with
`run(verify={...}, poses={...})`, K alone.  Every stage the reference does not have is an option of `run` that is off by
default and is described by its `*_options` function below; `run_plan` judges all of them together before anything touches
the device, and `run` is then one call per phase: `_front`, `_link`, `_poses`, `_structure`, `_adjust`.
"""
import ctypes as C
import math
import queue
import time
from concurrent.futures import ThreadPoolExecutor
from collections import namedtuple
from contextlib import contextmanager

import numpy as np
import torch

from . import _lib, ops, parallel
from ._lib import lib, default_context, c_i32p, c_i64p, c_f32p, MMError
from .bundleAdjuster import SchurTRF, frameParameters, _rodrigues_matrix, refine_schedule, refine_rounds, REFINE_KEYS
from .orb_pattern import brief_pattern


VERIFY_KEYS = ("n_hyp", "threshold_px", "min_matches", "min_inliers", "refit_iters", "seed", "on_fail")
POSE_KEYS = ("min_matches", "min_front_frac", "ambiguous_frac", "min_common", "E0")
DEGENERACY_HOMOGRAPHY_KEYS = ("n_hyp", "threshold_px", "min_matches", "min_inliers", "refit_iters", "seed", "collinear_tol",
                              "degenerate_frac")
DEGENERACY_POSE_KEYS = ("min_front_frac", "ambiguous_frac", "rotation_tol")
DEGENERACY_KEYS = DEGENERACY_HOMOGRAPHY_KEYS + DEGENERACY_POSE_KEYS
GUIDED_KEYS = ("threshold_px", "ratio", "max_dist", "cross_check")
RESECT_KEYS = ("n_hyp", "threshold_px", "min_rows", "min_inliers", "refit_iters", "polish_iters", "seed", "planar", "planar_tol",
               "collinear_tol")
ALIGN_KEYS = ("frames", "extrinsics", "centres", "tau", "tau_rel", "n_hyp", "seed", "refit_iters", "with_scale", "min_inliers")
ALIGN_FRAMES = "align: frames must be at least 3 distinct indices in [0, F)"
DENSE_DEFAULTS = dict(every=4, sources=4, gap=2, neighbours=4, planes=64, radius=3, downscale=1, depth_margin=0.1, min_points=16,
                      var_min=4.0, min_sources=1, max_cost=0.4, eps_depth=0.01, tau_px=1.0, min_consistent=2, max_points=None)
DENSE_KEYS = tuple(DENSE_DEFAULTS)
DENSE_FEW_POINTS = 1      # flag of a reference view that observes fewer than min_points points: it is not swept


def _stage_options(stage, value, keys):
    """An option of `run` that is None (the stage is off) or a dict with keys out of `keys` ({} for the defaults).  Returns it
    as a dict of its own; anything else, or an unknown key, raises ValueError."""
    if value is None:
        return None
    if not isinstance(value, dict):
        raise ValueError(f"{stage} must be None or a dict of " + ", ".join(keys))
    unknown = set(value) - set(keys)
    if unknown:
        raise ValueError(f"{stage} takes {', '.join(keys)}; not {sorted(unknown)}")
    return dict(value)


def verify_options(verify):
    """`run(..., verify=)`: None (every Lowe-ratio survivor goes to the linker, as in the reference) or a dict of the parameters
    of ops.verify_matches (pair_base and ctx are the pipeline's own): each rank verifies its own pairs against a RANSAC
    fundamental matrix between `match` and the gather / `link`, and only the inliers are linked.  -> as `_stage_options`."""
    return _stage_options("verify", verify, VERIFY_KEYS)


def pose_options(poses):
    """`run(..., poses=)`: None (`extrinsics` holds one [3,4] per frame) or a dict of the parameters of ops.recover_poses and
    ops.chain_poses (needs `verify`, which supplies each pair's F): the extrinsics are recovered from the verified matches and
    K, and `extrinsics` may be None.  The first baseline is the unit of length.  -> as `_stage_options`."""
    return _stage_options("poses", poses, POSE_KEYS)


def degeneracy_options(degeneracy):
    """`run(..., degeneracy=)`: None (no homography stage) or a dict of the parameters of ops.verify_homography and of
    ops.recover_poses_homography (min_front_frac, ambiguous_frac, rotation_tol) -- verify_info, pair_base, the hint and ctx are
    the pipeline's own (needs `verify`): every rank fits a homography per pair on the matches `verify` read, and a pair it
    explains as well as the fundamental matrix (HOMOG_DEGENERATE: a planar scene or a camera that only turns) is
    linked by the homography's inliers; with `poses` its relative pose comes from the homography -- a pure rotation is chained
    with t = 0 and the scale carried -- before the one chain call.  The selection is a torch.where on the device, no host
    read.  -> as `_stage_options`."""
    return _stage_options("degeneracy", degeneracy, DEGENERACY_KEYS)


def guided_options(guided):
    """`run(..., guided=)`: None (no guided matching) or a dict of the parameters of ops.guided_match -- the seeds, the model,
    its kind and ctx are the pipeline's own (needs `verify`): after `verify` and `degeneracy` and before the gather / `link`,
    every rank matches the key points its pairs' matches leave unused once more, among the candidates within threshold_px of
    the pair's model: F of `verify`, no model where it flagged TOO_FEW, NO_MODEL or WEAK, and with `degeneracy`
    the homography where the pair is HOMOG_DEGENERATE (a torch.where on the device, no host read).  The enlarged set replaces
    the matches: the linker reads it, `poses` and the chain read the linked matches as before.  -> as `_stage_options`."""
    return _stage_options("guided", guided, GUIDED_KEYS)


def resect_options(resect):
    """`run(..., resect=)`: None (no resection) or a dict of the parameters of ops.resect_cameras -- the points, the prior,
    cam_base and ctx are the pipeline's own: after the triangulation every frame is resected against `points0` (under
    "multi_view" only against the tracks no test flagged), with the extrinsics in use -- given or recovered -- as the prior, so
    no frame ends with a higher MSAC cost than it came in with; the tracks are then triangulated again with the new poses and
    the adjustment starts from those.  `planar` ("auto" / "only", with planar_tol and collinear_tol) sends frames whose points
    are coplanar through the homography branch; without it exactly the one call of 6f is launched.
    -> as `_stage_options`."""
    return _stage_options("resect", resect, RESECT_KEYS)


def align_options(align, n_frames=None):
    """`run(..., align=)`: None (no registration) or a dict: `frames`, at least 3 distinct indices in [0, F); the targets of
    those frames as one of `extrinsics` [n, 3|4, 4] or `centres` [n, 3], in the frame the result is wanted in; and optionally
    tau or tau_rel (default tau_rel = 0.05: five percent of the targets' spread admits the drift DESIGN.md 6e measured on a
    recovered chain, 2.16 % at its worst, and not a broken link), n_hyp, seed, refit_iters, with_scale, min_inliers.  Once the
    extrinsics are settled -- given or recovered -- and before the first triangulation, the centres of the cameras `frames` are
    registered to the targets by a robust similarity and the extrinsics are replaced by their image, so
    triangulation, `resect` and the adjustment run in the target frame and scale; with `poses`, `poses["extrinsics"]` holds the
    image.  If the adjustment runs, its cameras are registered to the same targets once more (`ba_aligned`; `ba` itself is left
    as it is).  ALIGN_TOO_FEW or ALIGN_NO_MODEL: nothing is transformed, the flags say so.  Returns dict(frames [n] i64,
    centres [n, 3] f64, params for ops.align_similarity); anything else raises ValueError."""
    align = _stage_options("align", align, ALIGN_KEYS)
    if align is None:
        return None
    if "frames" not in align or ("extrinsics" in align) == ("centres" in align):
        raise ValueError("align needs frames and exactly one of extrinsics and centres")
    frames = np.asarray(align.pop("frames"))
    if frames.ndim != 1 or frames.size < 3 or not np.issubdtype(frames.dtype, np.integer) or np.unique(frames).size != frames.size \
            or frames.min() < 0 or (n_frames is not None and frames.max() >= n_frames):
        raise ValueError(ALIGN_FRAMES)
    if "centres" in align:
        centres = np.asarray(align.pop("centres"), np.float64)
    else:
        E = np.asarray(align.pop("extrinsics"), np.float64)
        if E.ndim != 3 or E.shape[1] not in (3, 4) or E.shape[2] != 4:
            raise ValueError("align: extrinsics [n, 3|4, 4] expected")
        centres = -np.einsum("nji,nj->ni", E[:, :3, :3], E[:, :3, 3])
    if centres.shape != (frames.size, 3):
        raise ValueError("align: one target per entry of frames expected (extrinsics [n, 3|4, 4] or centres [n, 3])")
    if "tau" in align and "tau_rel" in align:
        raise ValueError("align takes tau or tau_rel, not both")
    if "tau" not in align and "tau_rel" not in align:
        align["tau_rel"] = 0.05
    return dict(frames=frames.astype(np.int64), centres=np.ascontiguousarray(centres), params=align)


def refine_options(refine):
    """`run(..., refine=)`: None (no filtering after the adjustment) or a dict of the options of bundleAdjuster.refine_schedule
    ({} for the defaults): max_reproj_px, a number or one threshold per round with the last one repeated; min_angle_deg,
    min_depth, min_views; rounds (default 2); ftol / max_nfev of the re-solves.  After the adjustment every observation is
    judged at the adjusted cameras and points and every point by the observations it has left (ops.filter_observations,
    DESIGN.md 6k); if anything is flagged, what survives is adjusted again from the same cameras and the surviving points, up to
    `rounds` times.  `ba` itself is left as it is; with `align`, `ba_aligned` is computed from the refined result, so its points
    are those of `refine["point_map"]`.  Returns the schedule as a dict; anything else raises ValueError."""
    refine = _stage_options("refine", refine, REFINE_KEYS)
    return None if refine is None else refine_schedule(**refine)


def dense_options(dense):
    """`run(..., dense=)`: None (no dense stage) or a dict ({} for the defaults, DENSE_DEFAULTS): `every` (every every-th frame
    is a reference view), `sources` (source slots per view: the frames at -gap, +gap, -2 gap, +2 gap, ... that exist), `gap`,
    `neighbours` (the views before and after it in the view list a view is checked against, same pattern), `planes`, `radius`,
    `var_min`, `min_sources` (ops.depth_sweep), `downscale` (1, 2 or 4: the frames are reduced by integer 2 x 2 means and K
    scaled), `depth_margin` (a view's depth range is the min / max depth of the adjusted points it observes, divided /
    multiplied by 1 + depth_margin), `min_points` (a view that observes fewer is skipped and flagged DENSE_FEW_POINTS),
    `max_cost`, `eps_depth`, `tau_px`, `min_consistent` (ops.depth_fuse) and `max_points` (rows of the cloud; None: every
    pixel).  After the adjustment -- or, with ba=False, after the triangulation -- every reference view gets a depth map by
    plane sweep and the maps are fused into a point cloud.  Returns the options with the defaults filled in;
    anything else raises ValueError."""
    dense = _stage_options("dense", dense, DENSE_KEYS)
    if dense is None:
        return None
    d = dict(DENSE_DEFAULTS, **dense)

    def whole(key, lo, hi=None):
        v = d[key]
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo or (hi is not None and v > hi):
            raise ValueError(f"dense: {key} must be an integer of at least {lo}" + (f" and at most {hi}" if hi is not None else ""))
        d[key] = int(v)

    def number(key, lo):
        v = d[key]
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not (v >= lo) or v == np.inf:
            raise ValueError(f"dense: {key} must be a finite number of at least {lo}")
        d[key] = float(v)

    whole("every", 1), whole("gap", 1), whole("sources", 1, ops.SWEEP_MAX_SOURCES), whole("neighbours", 0, ops.FUSE_MAX_NEIGHBOURS)
    whole("planes", 1, ops.SWEEP_MAX_PLANES), whole("radius", 1, ops.SWEEP_MAX_RADIUS), whole("min_points", 1)
    whole("min_sources", 1, d["sources"]), whole("min_consistent", 0)
    if d["downscale"] not in (1, 2, 4) or isinstance(d["downscale"], bool):
        raise ValueError("dense: downscale must be 1, 2 or 4")
    d["downscale"] = int(d["downscale"])
    number("depth_margin", 0.0), number("var_min", 0.0), number("eps_depth", 0.0), number("tau_px", 0.0)
    if isinstance(d["max_cost"], bool) or not isinstance(d["max_cost"], (int, float, np.integer, np.floating)) or d["max_cost"] != d["max_cost"]:
        raise ValueError("dense: max_cost must be a number")
    d["max_cost"] = float(d["max_cost"])
    if d["max_points"] is not None:
        whole("max_points", 0)
    return d


def dense_views(n_frames, every, sources, gap, neighbours):
    """The view tables of the dense stage on the host -> (ref [V] i32: frames 0, every, 2 every, ...; src [V, sources] i32: the
    frames at -gap, +gap, -2 gap, +2 gap, ... of each, -1 where the clip has none; nbr [V, neighbours] i32: the views at -1, +1,
    -2, +2, ... in the view list, -1 where there is none)."""
    ref = np.arange(0, n_frames, every, dtype=np.int32)
    step = np.array([(j // 2 + 1) * (-1 if j % 2 == 0 else 1) for j in range(max(sources, neighbours))], np.int64)
    src = ref[:, None].astype(np.int64) + gap * step[None, :sources]
    src = np.where((src >= 0) & (src < n_frames), src, -1).astype(np.int32)
    nbr = np.arange(ref.size, dtype=np.int64)[:, None] + step[None, :neighbours]
    nbr = np.where((nbr >= 0) & (nbr < ref.size), nbr, -1).astype(np.int32)
    return ref, src, nbr


def downscale_frames(frames, K, factor):
    """frames [F, H, W] u8 reduced by `factor` (1, 2 or 4) with the integer 2 x 2 mean (a + b + c + d + 2) >> 2, once per
    halving (an odd last row or column is dropped), in torch, and K for the reduced grid: a reduced pixel's centre lies half an
    input pixel beyond the first of the two it covers, so fx, s, fy halve and c -> (c - 1/2) / 2.  -> (frames, K 3 x 3)."""
    K = np.array(np.asarray(K, np.float64).reshape(3, 3))
    while factor > 1:
        H2, W2 = frames.shape[1] // 2 * 2, frames.shape[2] // 2 * 2
        f = frames[:, :H2, :W2].to(torch.int32)
        frames = ((f[:, 0::2, 0::2] + f[:, 0::2, 1::2] + f[:, 1::2, 0::2] + f[:, 1::2, 1::2] + 2) >> 2).to(torch.uint8)
        K[0, :] = K[0, :] * 0.5
        K[1, :] = K[1, :] * 0.5
        K[0, 2], K[1, 2] = K[0, 2] - 0.25, K[1, 2] - 0.25
        factor //= 2
    return frames.contiguous(), K


def dense_cloud(frames, K, extrinsics, ranges, ctx=None, **options):
    """Depth maps and the fused cloud of a clip with known cameras (ops.depth_sweep, ops.depth_fuse; `options` as
    `dense_options` takes them): frames [F, H, W] u8 on the device, K 3 x 3, extrinsics [F, 3|4, 4] and ranges [F, 2] =
    (dmin, dmax) per frame on the host.  The reference views are every `every`-th frame; one whose range is not 0 < dmin
    <= dmax (NaN: how `run` marks a frame that observes fewer than min_points points) is flagged DENSE_FEW_POINTS and not
    swept: its maps hold no depth.  -> dict(views [V] the views' frames, range [V, 2] (NaN where flagged), flags [V] on the
    host; depth, cost [V, h, w] f32, plane [V, h, w] i32, keep [V, h, w] u8, points [n, 3] f64, grey [n] u8, origin [n, 2]
    i32 = (index into views, pixel v w + u of the reduced grid), n_consistent [n] i32 on the device; counts = (kept,
    candidates); K: the intrinsics of the reduced grid).  Duplicate surface points from neighbouring views are not merged."""
    opt = dense_options(options)
    E = np.ascontiguousarray(np.asarray(extrinsics, np.float64)[:, :3, :])
    F = frames.shape[0]
    rng = np.asarray(ranges, np.float64)
    if E.shape != (F, 3, 4) or rng.shape != (F, 2):
        raise ValueError("dense: one extrinsic [3|4, 4] and one range (dmin, dmax) per frame expected")
    ref, src, nbr = dense_views(F, opt["every"], opt["sources"], opt["gap"], opt["neighbours"])
    r = rng[ref]
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(r).all(1) & (r[:, 0] > 0) & (r[:, 1] >= r[:, 0])
    src = np.where(ok[:, None], src, -1).astype(np.int32)      # (a view without sources has no valid plane anywhere)
    small, Ks = downscale_frames(frames, K, opt["downscale"])
    sw = ops.depth_sweep(small, Ks, E, ref, src, np.where(ok[:, None], r, 1.0), planes=opt["planes"], radius=opt["radius"],
                         var_min=opt["var_min"], min_sources=opt["min_sources"], ctx=ctx)
    grey = small.index_select(0, torch.as_tensor(ref.astype(np.int64)).to(small.device))
    fu = ops.depth_fuse(sw["depth"], sw["cost"], Ks, E[ref], nbr, grey, max_cost=opt["max_cost"], eps_depth=opt["eps_depth"],
                        tau_px=opt["tau_px"], min_consistent=opt["min_consistent"], cap=opt["max_points"], ctx=ctx)
    return dict(views=ref, range=np.where(ok[:, None], r, np.nan), flags=np.where(ok, 0, DENSE_FEW_POINTS).astype(np.int32),
                depth=sw["depth"], cost=sw["cost"], plane=sw["plane"], keep=fu["keep"], points=fu["points"], grey=fu["grey"],
                origin=fu["origin"], n_consistent=fu["n_consistent"], counts=fu["counts"], K=Ks)


class RunPlan(namedtuple("RunPlan", "n_frames world sharded force_collectives triangulation cull verify poses resect degeneracy "
                                    "guided align refine dense", defaults=(None,))):
    """What `run_plan` makes of the options of `ClipPipeline.run`: every stage as its `*_options` function returns it (None: the
    stage is off), the clip's frame count, the ranks it is spread over, and whether the gather / all-reduce path is taken."""
    __slots__ = ()


def run_plan(n_frames, world=None, has_extrinsics=True, force_collectives=False, triangulation="two_view", cull=None,
             verify=None, poses=None, resect=None, degeneracy=None, guided=None, align=None, refine=None, dense=None):
    """Every check of `ClipPipeline.run` on its options, without a device -> RunPlan; a broken rule raises ValueError.  world:
    the ranks of the process group, None without one (one rank, and force_collectives has nothing to force).  n_frames and
    world may each be a function without arguments that gives the value: it is called only after the rules that need neither
    have passed -- the order the rules are reported in."""
    verify, poses, resect, degeneracy = verify_options(verify), pose_options(poses), resect_options(resect), degeneracy_options(degeneracy)
    guided, align, refine, dense = guided_options(guided), align_options(align), refine_options(refine), dense_options(dense)
    for stage, on, why in (("guided", guided, "it supplies each pair's fundamental matrix, the model the search is gated by"),
                           ("degeneracy", degeneracy, "the verdict compares the homography with each pair's fundamental matrix"),
                           ("poses", poses, "it supplies each pair's fundamental matrix")):
        if on is not None and verify is None:
            raise ValueError(f"{stage} needs verify ({why}): pass verify={{}} for the defaults")
    if poses is None and not has_extrinsics:
        raise ValueError("extrinsics is required unless poses is set")
    if triangulation not in ("two_view", "multi_view"):
        raise ValueError("triangulation must be 'two_view' or 'multi_view'")
    n_frames = n_frames() if callable(n_frames) else n_frames
    if align is not None and align["frames"].max() >= n_frames:
        raise ValueError(ALIGN_FRAMES)
    world = world() if callable(world) else world
    ranks = 1 if world is None else world
    if cull is not None and triangulation != "multi_view":
        raise ValueError("cull needs triangulation='multi_view' (the two-view path has no per-track verdict)")
    for stage, on, why in (("cull", cull, "the track partition takes contiguous ranges"),
                           ("poses", poses, "the chain needs the neighbouring pair's depths across every rank boundary"),
                           ("resect", resect, "every frame needs the whole point table"),
                           ("align", align, "the cameras of `frames` live on different ranks"),
                           ("refine", refine, "the compaction renumbers the points of one shard"),
                           ("dense", dense, "a view's depth range needs every point it observes and its sources' frames")):
        if on is not None and ranks > 1:
            raise ValueError(f"{stage} is not supported with more than one rank: {why}")
    if cull is not None:
        tests = {"max_reproj_px", "min_angle_deg", "min_depth"}
        unknown = set(cull) - tests - {"refine_iters"}
        if unknown or not tests & set(cull):
            raise ValueError("cull takes max_reproj_px, min_angle_deg, min_depth (at least one) and refine_iters"
                             + (f"; not {sorted(unknown)}" if unknown else ""))
    return RunPlan(n_frames, ranks, ranks > 1 or (world is not None and bool(force_collectives)), force_collectives, triangulation,
                   cull, verify, poses, resect, degeneracy, guided, align, refine, dense)


class StageClock:
    """The stage timers of `ClipPipeline.run`: `with clock("verify"):` adds the interval's milliseconds to ms["verify"], the
    context synchronised before the clock starts and before it stops.  `with clock.paused("poses"), clock("degeneracy"):`
    bills what it encloses to "degeneracy" and not to the open "poses" interval around it."""

    def __init__(self, ctx, ms, now=time.perf_counter):
        self.ctx, self.ms, self.now, self.since = ctx, ms, now, {}

    def _start(self, name):
        self.ctx.sync()
        self.since[name] = self.now()

    def _stop(self, name):
        self.ctx.sync()
        self.ms[name] = self.ms.get(name, 0.0) + (self.now() - self.since.pop(name)) * 1e3

    @contextmanager
    def __call__(self, name):
        self._start(name)
        yield
        self._stop(name)

    @contextmanager
    def paused(self, name):
        self._stop(name)
        yield
        self._start(name)


def _only(options, keys):
    return {k: v for k, v in options.items() if k in keys}


class _Front(namedtuple("_Front", "det xy n pairs m verify degeneracy guided is_deg pairs_local frames_local")):
    """What `ClipPipeline._front` hands on: this rank's `detect` result (None without frames) with its xy and n tables, the
    matches that go to the linker, the `verify` / `degeneracy` / `guided` entries of the result (None: stage off), the
    HOMOG_DEGENERATE mask of the pairs (with `degeneracy`), and how many pairs and frames the rank owns."""
    __slots__ = ()


class ClipPipeline:
    def __init__(self, height, width, nfeatures, batch=32, ratio=0.75, device=None, ctx=None, nlevels=8):
        self.ctx = ctx or default_context()
        self.device = device or self.ctx.device
        self.H, self.W = height, width
        self.prm = ops.orb_params(nfeatures, nlevels=nlevels)
        self.cap = nfeatures
        self.batch = batch
        self.ratio = ratio
        self.wsp = ops.OrbWorkspace(batch, height, width, self.prm, self.device, brief_pattern())
        self.scales = ops.orb_level_sizes(height, width, self.prm)[3]

    # ------------------------------------------------------------------------------------------- detect
    def detect(self, frames):
        """frames [F,H,W] u8 on the device -> dict of per-frame tables (xy [F,cap,2] f32, desc [F,cap,32] u8, n [F],
        meta, resp, mom), all device tensors."""
        F = frames.shape[0]
        d = self.device
        out = dict(xy=torch.zeros((F, self.cap, 2), dtype=torch.float32, device=d),
                   meta=torch.zeros((F, self.cap, 4), dtype=torch.int32, device=d),
                   resp=torch.zeros((F, self.cap), dtype=torch.float32, device=d),
                   mom=torch.zeros((F, self.cap, 2), dtype=torch.int32, device=d),
                   desc=torch.zeros((F, self.cap, 32), dtype=torch.uint8, device=d),
                   n=torch.zeros(F, dtype=torch.int32, device=d))
        for b0 in range(0, F, self.batch):
            b1 = min(F, b0 + self.batch)
            ops.orb_detect_compute(frames[b0:b1], self.wsp, self.ctx,
                                   out=(out["xy"][b0:b1], out["meta"][b0:b1], out["resp"][b0:b1], out["mom"][b0:b1],
                                        out["desc"][b0:b1], out["n"][b0:b1]))
        return out

    # ------------------------------------------------------------------------------------------- match
    def match(self, det, pair_lo=0, pair_hi=None):
        """Consecutive pairs (k, k+1), k in [pair_lo, pair_hi) relative to the frames in `det`:
        query = frame k, train = frame k+1 (processor.py:133).  -> pairs [n_pairs, cap, 2] i32, m [n_pairs] i32."""
        F = det["desc"].shape[0]
        if pair_hi is None:
            pair_hi = F - 1
        npairs = max(pair_hi - pair_lo, 0)
        desc, n = det["desc"], det["n"]
        if npairs == 0:
            return (torch.zeros((0, self.cap, 2), dtype=torch.int32, device=self.device),
                    torch.zeros(0, dtype=torch.int32, device=self.device))
        q = desc[pair_lo:pair_hi]
        t = desc[pair_lo + 1:pair_hi + 1]
        return ops.bf_match_ratio_batched(q, t, n[pair_lo:pair_hi].contiguous(), n[pair_lo + 1:pair_hi + 1].contiguous(),
                                          self.ratio, self.ctx)

    # ------------------------------------------------------------------------------------------- verify
    def verify(self, det, pairs, m, pair_lo=0, **params):
        """Epipolar verification of the matches `match` returned for the frames in `det` (ops.verify_matches): pair k of
        `pairs` joins frames k and k + 1 of `det`, and is pair pair_lo + k of the clip -- the key of its sampling, so a rank's
        block gives the rows the whole clip would.  -> (pairs_out, m_out, F [n,9], cost [n], info [n,4]), device tensors."""
        n = pairs.shape[0]
        return ops.verify_matches(det["xy"][:n + 1], pairs, m, pair_base=pair_lo, ctx=self.ctx, **params)

    # ------------------------------------------------------------------------------------------- homography
    def homography(self, det, pairs, m, verify_info=None, pair_lo=0, **params):
        """A RANSAC homography per pair on the matches `match` returned for the frames in `det` (ops.verify_homography) -- the
        same input `verify` takes, not its output; verify_info = the info `verify` returned for them, which the planar /
        rotation-only verdict needs; pair_lo as in `verify`.  -> (pairs_out, m_out, H [n,9], cost [n], info [n,6])."""
        n = pairs.shape[0]
        return ops.verify_homography(det["xy"][:n + 1], pairs, m, verify_info=verify_info, pair_base=pair_lo, ctx=self.ctx, **params)

    # ------------------------------------------------------------------------------------------- guided
    def guided(self, det, pairs, m, model, kind=None, **params):
        """Guided matching on what `verify` (or `homography`) returned for the frames in `det` (ops.guided_match): pairs, m the
        seeds, model [n,9] each pair's F (kind 0) or H (kind 1; anything else: no model, the pair passes through).
        -> (pairs_out, m_out, is_new [n,cap] u8, info [n,4]), device tensors."""
        n = pairs.shape[0]
        return ops.guided_match(det["xy"][:n + 1], det["desc"][:n + 1], det["n"][:n + 1], pairs, m, model, kind=kind, ctx=self.ctx,
                                **params)

    # ------------------------------------------------------------------------------------------- poses
    def recover_poses(self, det, pairs, m, F, K, E0=None, min_common=8, override=None, **params):
        """Camera poses from what `verify` returned for the frames in `det`: a relative pose per pair (ops.recover_poses,
        `params` as it takes them), chained into one scale and one frame (ops.chain_poses; E0 = the first frame's extrinsic,
        [I | 0] by default).  override: a function (R, t, depth, info) -> the same four, called between the two -- how `run`
        gives the degenerate pairs the homography's pose.  -> dict(extrinsics [n+1, 3, 4] f64, R, t, sigma, info, depth, scale,
        rho, chain_info), device tensors.  The first baseline is the unit of length."""
        n = pairs.shape[0]
        R, t, sigma, depth, info = ops.recover_poses(det["xy"][:n + 1], pairs, m, F, K, ctx=self.ctx, **params)
        if override is not None:
            R, t, depth, info = override(R, t, depth, info)
        ext, scale, rho, cinfo = ops.chain_poses(pairs, m, depth, R, t, info, E0=E0, min_common=min_common, ctx=self.ctx)
        return dict(extrinsics=ext, R=R, t=t, sigma=sigma, info=info, depth=depth, scale=scale, rho=rho, chain_info=cinfo)

    # ------------------------------------------------------------------------------------------- resect
    def resect(self, K, points, track_ptr, obs_frame, obs_kp, kp_xy_dev, n_frames, pt_ok=None, prior=None, **params):
        """Every frame registered against the 3-D points of the tracks it observes (ops.resect_cameras): points [T, 3] f64 (one
        per track, as `triangulate` returns them), the linked tracks as `run` keeps them, pt_ok [T] (0: the track's point is
        not used), prior [n_frames, 3, 4].  -> dict(extrinsics [n_frames, 3, 4] f64, cost [n_frames], info [n_frames, 6],
        inliers_per_frame [n_frames] i64, inlier [O] u8 over the observations in track order), device tensors."""
        d = self.device
        coords, fi, pi = ops.flatten_tracks(track_ptr, obs_frame, obs_kp, kp_xy_dev, ctx=self.ctx)
        # the camera CSR of the observations, stable (the order mm_ba_build_index gives)
        fl = fi.long()
        cam_obs = torch.argsort(fl, stable=True).to(torch.int32)
        cam_ptr = torch.zeros(n_frames + 1, dtype=torch.int32, device=d)
        cam_ptr[1:] = torch.cumsum(torch.bincount(fl, minlength=n_frames)[:n_frames], 0).to(torch.int32)
        pr = None if prior is None else (prior if torch.is_tensor(prior) else
                                         torch.as_tensor(np.ascontiguousarray(np.asarray(prior, np.float64)[:, :3, :]))).to(d)
        ext, cost, inlier, info = ops.resect_cameras(K, points.contiguous(), coords, pi, cam_ptr, cam_obs, pt_ok=pt_ok, prior=pr,
                                                     ctx=self.ctx, **params)
        per_frame = torch.zeros(n_frames, dtype=torch.int64, device=d).index_add_(0, fl, inlier.long())
        return dict(extrinsics=ext, cost=cost, info=info, inliers_per_frame=per_frame, inlier=inlier)

    # ------------------------------------------------------------------------------------------- link
    def link(self, kp_count, kp_xy, match_count, matches):
        """Host track linking over the clip (mm_link_tracks_clip).  numpy inputs:
        kp_count [F] i32, kp_xy [F,cap,2] f32, match_count [F-1] i32, matches [F-1,mcap,2] i32.
        -> (track_ptr [T+1] i64, obs_frame [O] i32, obs_kp [O] i32)."""
        kp_count = np.ascontiguousarray(kp_count, np.int32)
        kp_xy = np.ascontiguousarray(kp_xy, np.float32)
        match_count = np.ascontiguousarray(match_count, np.int32)
        matches = np.ascontiguousarray(matches, np.int32)
        F = len(kp_count)
        cap = kp_xy.shape[1] if kp_xy.ndim == 3 else 0
        mcap = matches.shape[1] if matches.ndim == 3 else 0
        total = int(match_count.sum())
        track_ptr = np.zeros(total + 2, np.int64)
        obs_frame = np.zeros(2 * total + 2, np.int32)
        obs_kp = np.zeros(2 * total + 2, np.int32)
        n_obs = C.c_int64(0)
        nt = lib.mm_link_tracks_clip(F, cap, kp_count.ctypes.data_as(c_i32p), kp_xy.ctypes.data_as(c_f32p), mcap,
                                     match_count.ctypes.data_as(c_i32p), matches.ctypes.data_as(c_i32p), total + 1,
                                     2 * total + 1, track_ptr.ctypes.data_as(c_i64p), obs_frame.ctypes.data_as(c_i32p),
                                     obs_kp.ctypes.data_as(c_i32p), C.byref(n_obs))
        if nt < 0:
            raise MMError(f"mm_link_tracks_clip failed ({nt})")
        return track_ptr[:nt + 1], obs_frame[:n_obs.value], obs_kp[:n_obs.value]

    # ------------------------------------------------------------------------------------------- triangulate
    def triangulate(self, track_ptr, obs_frame, obs_kp, kp_xy_dev, projections):
        """First/last observation of every track -> 3-D points [T,3] f64 on the device (processor.py:246-261).
        track_ptr / obs_frame / obs_kp: device tensors (or numpy arrays, uploaded here)."""
        d = self.device
        track_ptr, obs_frame, obs_kp = (t if torch.is_tensor(t) else torch.as_tensor(np.ascontiguousarray(t)).to(d)
                                        for t in (track_ptr, obs_frame, obs_kp))
        T = track_ptr.shape[0] - 1
        if T <= 0:
            return torch.zeros((0, 3), dtype=torch.float64, device=d)
        first = track_ptr[:-1].long()
        last = track_ptr[1:].long() - 1
        f0, f1 = obs_frame[first].int(), obs_frame[last].int()
        x0 = kp_xy_dev[f0.long(), obs_kp[first].long()].to(torch.float64)
        x1 = kp_xy_dev[f1.long(), obs_kp[last].long()].to(torch.float64)
        proj = torch.as_tensor(np.ascontiguousarray(projections, np.float64)).to(d)
        return ops.triangulate_dlt(proj, f0.contiguous(), f1.contiguous(), x0, x1, self.ctx)

    def triangulate_multi_view(self, track_ptr, obs_frame, obs_kp, kp_xy_dev, projections, **thresholds):
        """Every track from ALL its observations (ops.triangulate_tracks on the flattened CSR) -> (points [T,3] f64,
        quality [T,4] f64, flags [T] i32) on the device.  `thresholds` as ops.triangulate_tracks takes them."""
        coords, of_, _ = ops.flatten_tracks(track_ptr, obs_frame, obs_kp, kp_xy_dev, ctx=self.ctx)
        proj = torch.as_tensor(np.ascontiguousarray(projections, np.float64)).to(self.device)
        return ops.triangulate_tracks(proj, track_ptr, of_, coords, ctx=self.ctx, **thresholds)

    # ------------------------------------------------------------------------------------------- flatten (managePoints)
    @staticmethod
    def flatten(track_ptr, obs_frame, obs_kp, kp_xy_host):
        """(coordinates [O,2] f64, frame_indices [O] i32, point_indices [O] i32) in managePoints order
        (processor.py:264-291): point-major, insertion order inside a track."""
        lens = np.diff(track_ptr).astype(np.int64)
        pi = np.repeat(np.arange(len(lens), dtype=np.int32), lens)
        coords = kp_xy_host[obs_frame, obs_kp].astype(np.float64)
        return coords, obs_frame.astype(np.int32), pi

    # ------------------------------------------------------------------------------------------- sliding-window BA
    @staticmethod
    def window_selection(first_frame, last_frame, lo, hi, n_frames):
        """Tracks adjusted by the window of keyframes [lo, hi): every observation inside the window, and the track is
        finished ("popped", processor.py:233-238) by keyframe hi - 1 -- its last observation is at or before hi - 2 --
        or the clip ends with this window.  Works on numpy arrays and on tensors alike."""
        inside = (first_frame >= lo) & (last_frame < hi)
        if hi >= n_frames:
            return inside
        return inside & (last_frame <= hi - 2)

    @staticmethod
    def window_selection_anchored(first_frame, last_frame, lo, hi, n_frames):
        """Tracks adjusted by the ANCHORED window [lo, hi): finished by keyframe hi - 1 or the clip's end (as in
        `window_selection`) and last observed at or after keyframe lo -- a track may begin before the window (a boundary
        track); its older observations then pull against the fixed cameras.  For lo = 0 this is `window_selection`.
        (first_frame is not needed; it is taken for the same call shape.)  Works on numpy arrays and on tensors alike."""
        del first_frame
        sel = (last_frame >= lo) & (last_frame < hi)
        if hi >= n_frames:
            return sel
        return sel & (last_frame <= hi - 2)

    def adjust_windows(self, out, K, extrinsics, window=50, stride=25, ftol=1e-4, verbose=0, timers=None, dist=None,
                       order="sequential", streams=1, batched=False, max_nfev=None, boundary="inside"):
        """Incremental bundle adjustment over a sliding window of keyframes: the reference keeps this step as a
        commented hook (processor.py:395-408: after a keyframe whose tracks were popped, `managePoints(popped_tracks)`
        + `adjustPoints` over everything so far); bounding it to the last `window` keyframes is what makes the
        2000-frame clips tractable.  For hi = window, window + stride, ..., F the cameras
        lo = hi - window .. hi - 1 and the finished tracks that live entirely inside the window are adjusted with
        exactly the solver of `adjustPoints` (all window cameras and points free, ftol as given); camera parameters and
        points are written back and later windows start from them.

        With `dist` (torch.distributed, every rank holding the same linked tracks as `run(..., dist=dist)` leaves them)
        each window's points are split over the ranks by observation count, cameras are replicated, and the solver
        all-reduces the camera-side blocks exactly as the global adjustment does ("C5 sliding
        window: same, with F replaced by W"); the adjusted points of a window are re-assembled on every rank.

        order = "wavefront": the windows (`window_schedule`, which every schedule takes them from) are coloured so that
        windows of one colour share no camera (two colours for stride >= window / 2: the even windows, then the odd ones,
        which start from both neighbours' results; a last window that ends off the stride grid may take a third) and each
        colour is one pass in which every window is solved WHOLE by one rank (round robin), the results of a pass being
        exchanged with one all-reduce of the touched cameras / points.  Windows of a pass are independent, so this
        scales with the number of GPUs instead of paying a collective per trust-region iteration of a 300-unknown
        system, and the result does not depend on the world size at all (bit for bit: every window is solved by the
        same un-sharded code on the same inputs).  It is a different -- equally valid -- schedule than "sequential".
        streams > 1 (wavefront only): that many windows of a pass are in flight on this GPU at once, one HIP stream and
        one host thread each; the result does not depend on it either.
        max_nfev: evaluation budget PER WINDOW (None: SciPy's default of 100 n, as adjustPoints).  A window is adjusted again
        by its successor, so a budget is a reasonable guard against the occasional outlier-laden window that crawls
        (observed: one window of 79 taking 3466 evaluations where the others take 30 - 340); a window that exhausts it
        reports status 0 and its last accepted iterate is used.
        batched = True (wavefront only; supersedes `streams`): ALL windows of a pass that this rank owns advance in
        lock-step through mm_ba_trf_batched -- every kernel of the trust-region loop is launched once per round for all of
        them, so a pass costs about as many evaluations as its slowest window needs instead of the sum over its windows.
        Bit-identical to solving the windows one at a time.

        boundary = "inside" (default): the window adjusts the tracks that lie entirely inside it, with all its cameras free
        (above).  boundary = "anchored": the local bundle adjustment of SLAM / incremental SfM that SURVEY.md 8(f)-2
        specifies.  The points are the finished tracks (same rule) last observed at or after lo
        (`window_selection_anchored`), so a track that crosses the window's left edge is adjusted with ALL its
        observations; the cameras lo .. hi - 1 are free, the cameras 0 .. lo - 1 -- as earlier windows left them -- are
        fixed (mm_ba_trf_fixed: observed, not optimised, never written), so the gauge stays pinned to the settled
        trajectory instead of re-floating in every window.  The first window (lo = 0) is the same as with "inside".  Each
        window's stats gain `fixed_cameras`, the number of distinct fixed cameras its tracks observe.  Sequential, one rank,
        one stream only: windows solved side by side would read each other's free cameras as fixed (ValueError otherwise).

        `out` is the result of `run(..., ba=False)`.  -> dict(cams [F,6] device, points [T,3] device, windows=[...])."""
        d = self.device
        world = dist.get_world_size() if dist is not None else 1
        rank = dist.get_rank() if dist is not None else 0
        if order not in ("sequential", "wavefront"):
            raise ValueError("order must be 'sequential' or 'wavefront'")
        if boundary not in ("inside", "anchored"):
            raise ValueError("boundary must be 'inside' or 'anchored'")
        if boundary == "anchored" and (order != "sequential" or batched or int(streams) > 1 or dist is not None):
            raise ValueError("boundary='anchored' needs order='sequential' on one rank and one stream (no batched): "
                             "its windows read the cameras earlier windows settled")
        allreduce = parallel.AllReduce() if world > 1 else None
        F = int(np.asarray(extrinsics).shape[0])
        cams, pts, first_f, last_f, lens_all, T = self._windows_prologue(out, extrinsics, F)
        if T == 0:
            return dict(cams=cams, points=pts, windows=[])
        wins, colours = self.window_schedule(F, window, stride)
        t0 = time.perf_counter()
        if order == "wavefront":
            cams, pts, table = self._windows_wavefront(out, K, cams, pts, first_f, last_f, wins, colours, ftol, verbose,
                                                       allreduce, world, rank, streams, batched, max_nfev)
        else:
            stats = []
            for lo, hi in wins:
                sel = sel_all = self._window_tracks(first_f, last_f, lo, hi, F, boundary)
                P_all = int(sel.numel())
                if P_all == 0:
                    continue
                sharded = world > 1 and P_all >= 4 * world
                if sharded:
                    # this rank's contiguous share of the window's points (balanced by observations); tiny windows are
                    # solved redundantly on every rank (identical, deterministic) rather than with empty shards
                    cum = torch.cat([torch.zeros(1, dtype=torch.int64, device=d), torch.cumsum(lens_all[sel], 0)])
                    bounds = parallel.split_by_weight(cum, world)
                    p_lo, p_hi = bounds[rank], bounds[rank + 1]
                    sel = sel[p_lo:p_hi]
                pb, n_fixed = self._window_problem(out, K, cams, sel, lo, hi, boundary, self.ctx)
                O = pb.O
                res = SchurTRF(pb, allreduce=allreduce if sharded else None).solve(
                    cams[lo:hi].contiguous(), pts[sel].contiguous(), ftol=ftol, max_nfev=max_nfev,
                    verbose=verbose if rank == 0 else 0)
                cams[lo:hi] = res.cams
                if sharded:
                    buf = torch.zeros((P_all, 3), dtype=torch.float64, device=d)
                    buf[p_lo:p_hi] = res.pts
                    allreduce(buf)                                  # disjoint shards: the sum re-assembles the window
                    pts[sel_all] = buf
                    O_all = torch.tensor([float(O)], dtype=torch.float64, device=d)
                    allreduce(O_all)
                    O = int(O_all.item())
                else:
                    pts[sel] = res.pts
                st = dict(lo=lo, hi=hi, points=P_all, observations=O)
                if boundary == "anchored":
                    st["fixed_cameras"] = n_fixed
                stats.append(dict(st, nfev=res.nfev, cost=res.cost, status=res.status))
        self.ctx.sync()
        if timers is not None:
            timers["ba_windows"] = timers.get("ba_windows", 0.0) + (time.perf_counter() - t0) * 1e3
        if order == "wavefront":
            stats = [dict(lo=wins[k][0], hi=wins[k][1], points=int(r[0]), observations=int(r[1]), nfev=int(r[2]),
                          status=int(r[3]), cost=float(r[4]), colour=colours[k])
                     for k, r in enumerate(table.cpu().numpy()) if r[0] > 0]
        return dict(cams=cams, points=pts, windows=stats)

    @staticmethod
    def window_schedule(n_frames, window, stride):
        """The windows of `adjust_windows`, on the host -> (wins, colours).  wins: (lo, hi) for hi = window, window + stride,
        ..., n_frames with lo = max(0, hi - window); the window is clamped to 2 .. n_frames keyframes, the stride to at least
        1, and the last window ends at n_frames.  colours: greedy colouring in window order -- a window takes the first
        colour whose last window ended at or before its lo -- so a colour's windows share no camera (read by the wavefront
        schedule only)."""
        window = max(2, min(int(window), n_frames))
        wins = [(max(0, hi - window), hi) for hi in list(range(window, n_frames, max(1, int(stride)))) + [n_frames]]
        colour_end, colours = [], []
        for lo, hi in wins:
            c = next((k for k, e in enumerate(colour_end) if e <= lo), len(colour_end))
            colour_end[c:c + 1] = [hi]                # (a new colour when c == len(colour_end))
            colours.append(c)
        return wins, colours

    def _windows_prologue(self, out, extrinsics, F):
        """What every schedule starts from -> (cams [F,6], pts [T,3] (a copy of points0), first_f, last_f (first / last frame
        of every track), lens_all (observations per track), T); without tracks the last four are None, None, None, 0."""
        tp, of_ = out["track_ptr_dev"], out["obs_frame_dev"]
        with np.errstate(all="ignore"):
            cams = torch.as_tensor(frameParameters(np.asarray(extrinsics, float)[:, :3, :]).reshape(F, 6)).to(self.device)
        pts = out["points0"].clone()
        T = tp.shape[0] - 1
        if T == 0:
            return cams, pts, None, None, None, 0
        tp64 = tp.long()
        return cams, pts, of_[tp64[:-1]], of_[tp64[1:] - 1], tp64[1:] - tp64[:-1], T

    def _window_tracks(self, first_f, last_f, lo, hi, F, boundary="inside"):
        """Indices of the tracks the window [lo, hi) adjusts (`window_selection` / `window_selection_anchored`)."""
        select = self.window_selection_anchored if boundary == "anchored" else self.window_selection
        return torch.nonzero(select(first_f, last_f, lo, hi, F)).reshape(-1)

    def _window_flatten(self, out, sel, lo, hi, boundary="inside", ctx=None):
        """The observations of the tracks `sel`, point-major (managePoints order; mm_flatten_offsets + mm_flatten_tracks), frame
        indices relative to the window -> (fi, pi, coords, n_fixed).  Anchored: the cameras before the window (negative
        indices) become the fixed cameras W + f, and n_fixed counts the distinct ones observed."""
        coords, fi, pi = ops.flatten_tracks(out["track_ptr_dev"], out["obs_frame_dev"], out["obs_kp_dev"], out["xy_dev"], sel=sel,
                                            frame_offset=lo, ctx=ctx or self.ctx)
        n_fixed = 0
        if boundary == "anchored" and lo > 0:
            W = hi - lo
            fi = torch.where(fi < 0, fi + (lo + W), fi).contiguous()
            n_fixed = int(torch.unique(fi[fi >= W]).numel())
        return fi, pi, coords, n_fixed

    def _window_problem(self, out, K, cams, sel, lo, hi, boundary="inside", ctx=None):
        """The bundle adjustment problem of the tracks `sel` in the window [lo, hi) -> (BADevice, n_fixed): free
        cameras lo .. hi - 1 (indices f - lo); anchored, and lo > 0: fixed cameras 0 .. lo - 1 at their current values."""
        ctx = ctx or self.ctx
        fi, pi, coords, n_fixed = self._window_flatten(out, sel, lo, hi, boundary, ctx)
        fixed = dict(fixed_cams=cams[:lo].clone()) if boundary == "anchored" and lo > 0 else {}
        return ops.BADevice(K, fi, pi, coords, hi - lo, int(sel.numel()), self.device, ctx, **fixed), n_fixed

    def _windows_wavefront(self, out, K, cams, pts, first_f, last_f, wins, colours, ftol, verbose, allreduce, world, rank,
                           streams, batched, max_nfev):
        """adjust_windows(order="wavefront") between the prologue and the epilogue -> (cams, pts, table [windows, 5]: points,
        observations, nfev, status, cost of every window, all-reduced)."""
        d = self.device
        F, T = cams.shape[0], pts.shape[0]
        table = torch.zeros((len(wins), 5), dtype=torch.float64, device=d)
        # Windows of a pass are independent AND small (a 300-unknown reduced system keeps 16 workgroups busy): this rank
        # solves up to `streams` of them at once, each on its own HIP stream with its own library context, driven by its
        # own host thread (mm_ba_trf blocks in C with the GIL released).  Every window still runs the same code on the
        # same inputs, so the result does not depend on `streams`.
        n_streams = max(1, int(streams))
        slots = queue.SimpleQueue()
        if n_streams > 1:
            for _ in range(n_streams):
                st = torch.cuda.Stream(device=d)
                slots.put((st, _lib.Context(d, st)))

        def window_problem(k, ctx):         # -> (sel, BADevice; None for an empty window); the boundary is "inside"
            lo, hi = wins[k]
            sel = self._window_tracks(first_f, last_f, lo, hi, F)
            if int(sel.numel()) == 0:
                return sel, None
            return sel, self._window_problem(out, K, None, sel, lo, hi, ctx=ctx)[0]

        def solve_window(k, ctx, cams, pts, cams_upd, cam_mask, pts_upd, pt_mask):
            lo, hi = wins[k]
            sel, pb = window_problem(k, ctx)
            if pb is None:
                return
            res = SchurTRF(pb).solve(cams[lo:hi].contiguous(), pts[sel].contiguous(), ftol=ftol, max_nfev=max_nfev,
                                     verbose=verbose if rank == 0 and n_streams == 1 else 0)
            cams_upd[lo:hi] = res.cams
            cam_mask[lo:hi] = 1.0
            pts_upd[sel] = res.pts
            pt_mask[sel] = 1.0
            table[k] = torch.tensor([pb.P, pb.O, res.nfev, res.status, res.cost], dtype=torch.float64, device=d)

        def solve_window_on_slot(k, *state):
            slot = slots.get()
            try:
                with torch.cuda.stream(slot[0]):
                    solve_window(k, slot[1], *state)
                    slot[0].synchronize()       # results are in place before the pass's thread pool is joined
            finally:
                slots.put(slot)

        for c in range(max(colours) + 1):
            mine = [k for j, k in enumerate(k for k, cc in enumerate(colours) if cc == c) if j % world == rank]
            cams_upd, pts_upd = torch.zeros_like(cams), torch.zeros_like(pts)
            cam_mask = torch.zeros(F, dtype=torch.float64, device=d)
            pt_mask = torch.zeros(T, dtype=torch.float64, device=d)
            state = (cams, pts, cams_upd, cam_mask, pts_upd, pt_mask)
            if batched and len(mine) > 1:
                # every window of the pass through ONE lock-step solve (mm_ba_trf_batched)
                items = []
                for k in mine:
                    lo, hi = wins[k]
                    sel, pb = window_problem(k, self.ctx)
                    if pb is not None:
                        items.append((k, sel, pb, cams[lo:hi].contiguous(), pts[sel].contiguous()))
                reps, _ = ops.trf_solve_batched([it[2] for it in items], [it[3] for it in items], [it[4] for it in items],
                                                ftol, 1e-8, 1e-8, max_nfev=max_nfev, ctx=self.ctx)
                rows, ks = [], []
                for (k, sel, pb, cw, pw), rep in zip(items, reps):
                    lo, hi = wins[k]
                    cams_upd[lo:hi] = cw
                    cam_mask[lo:hi] = 1.0
                    pts_upd[sel] = pw
                    pt_mask[sel] = 1.0
                    rows.append([pb.P, pb.O, rep.nfev, rep.status, rep.cost])
                    ks.append(k)
                if ks:
                    table[torch.tensor(ks, device=d)] = torch.tensor(rows, dtype=torch.float64, device=d)
            elif n_streams > 1 and len(mine) > 1:
                torch.cuda.current_stream(d).synchronize()        # the pass's inputs are complete
                with ThreadPoolExecutor(max_workers=n_streams) as pool:
                    for f_ in [pool.submit(solve_window_on_slot, k, *state) for k in mine]:
                        f_.result()
            else:
                for k in mine:
                    solve_window(k, self.ctx, *state)
            if allreduce is not None:          # the windows of a pass touch disjoint cameras / points: the sums are copies
                for t_ in (cams_upd, cam_mask, pts_upd, pt_mask):
                    allreduce(t_)
            cams = torch.where(cam_mask[:, None] > 0, cams_upd, cams)
            pts = torch.where(pt_mask[:, None] > 0, pts_upd, pts)
        if allreduce is not None:
            allreduce(table)
        return cams, pts, table

    @staticmethod
    def tracks_to_host(out):
        """Copy the linked tracks of a `run` result to the host: adds numpy `track_ptr` [T+1] i64, `obs_frame`,
        `obs_kp` [O] i32 (the layout mm_link_tracks_clip returns) to `out`."""
        out["track_ptr"] = out["track_ptr_dev"].cpu().numpy().astype(np.int64)
        out["obs_frame"] = out["obs_frame_dev"].cpu().numpy()
        out["obs_kp"] = out["obs_kp_dev"].cpu().numpy()
        return out

    # ------------------------------------------------------------------------------------------- align
    def align(self, ext_d, align):
        """The cameras ext_d [F, 3, 4] (device) registered to the targets of `align` (align_options): the centres of
        ext_d[frames] against the target centres (ops.camera_centres, ops.align_similarity) -> dict(sim [13], cost, info [4],
        inlier [n]), device tensors.  Nothing is transformed here."""
        idx = torch.as_tensor(align["frames"]).to(self.device)
        src = ops.camera_centres(ext_d.index_select(0, idx).contiguous(), ctx=self.ctx)
        dst = torch.as_tensor(align["centres"]).to(self.device)
        sim, cost, inlier, info = ops.align_similarity(src, dst, ctx=self.ctx, **align["params"])
        return dict(sim=sim[0].contiguous(), cost=cost[0], info=info[0], inlier=inlier)

    # ------------------------------------------------------------------------------------------- dense
    def depth_ranges(self, extrinsics, points, fi, pi, depth_margin=0.1, min_points=16):
        """The depth range of every frame from the points it observes: extrinsics [F, 3, 4] on the host, points [P, 3] f64 and
        the observations' frame / point indices fi, pi [O] on the device.  z = R_2 . X + t_2 per observation; a frame's range is
        (min z / (1 + depth_margin), max z (1 + depth_margin)) over its finite, positive depths (torch scatter_reduce amin /
        amax: no float sum, so it does not depend on the order) -> ranges [F, 2] f64 on the host, NaN for a frame with fewer
        than min_points such observations."""
        d = self.device
        E = torch.as_tensor(np.ascontiguousarray(np.asarray(extrinsics, np.float64)[:, :3, :])).to(d)
        F = E.shape[0]
        fl, pl = fi.long(), pi.long()
        X = points.reshape(-1, 3)[pl]
        z = (E[fl, 2, 0] * X[:, 0] + E[fl, 2, 1] * X[:, 1]) + E[fl, 2, 2] * X[:, 2] + E[fl, 2, 3]
        ok = torch.isfinite(z) & (z > 0)
        inf = torch.full_like(z, math.inf)
        zmin = torch.full((F,), math.inf, dtype=torch.float64, device=d).scatter_reduce(0, fl, torch.where(ok, z, inf), "amin")
        zmax = torch.full((F,), -math.inf, dtype=torch.float64, device=d).scatter_reduce(0, fl, torch.where(ok, z, -inf), "amax")
        cnt = torch.zeros(F, dtype=torch.int64, device=d).index_add_(0, fl, ok.long())
        zmin, zmax, cnt = (t.cpu().numpy() for t in (zmin, zmax, cnt))      # (one synchronisation: the sweep's tables are the host's)
        rng = np.stack([zmin / (1.0 + depth_margin), zmax * (1.0 + depth_margin)], 1)
        rng[cnt < min_points] = np.nan
        return rng

    def dense(self, frames, K, extrinsics, ranges, **options):
        """`dense_cloud` on this pipeline's context."""
        return dense_cloud(frames, K, extrinsics, ranges, ctx=self.ctx, **options)

    def _dense(self, plan, frames, K, ext, X, kept, tracks, out, clock):
        """The dense stage of `run` at the final cameras and points: the refined ones if `refine` ran, the adjusted ones after
        the adjustment, the initial ones with ba=False -> the `dense` entry of the result."""
        with clock("dense"):
            F, T = plan.n_frames, tracks[0].shape[0] - 1
            if kept is not None:
                _, fi, pi = ops.flatten_tracks(*tracks, sel=kept, ctx=self.ctx)
                pts = X[kept]
            else:
                _, fi, pi = ops.flatten_tracks(*tracks, t_lo=0, n_sel=T, ctx=self.ctx)
                pts = X
            if "ba" in out:
                res = out["ba"]
                if "refine" in out:
                    # the refined points are rows point_map of the adjusted ones, their observations rows obs_map
                    res, pm, om = out["refine"]["ba"], out["refine"]["point_map"].long(), out["refine"]["obs_map"].long()
                    new = torch.full((pts.shape[0],), -1, dtype=torch.int64, device=self.device)
                    new[pm] = torch.arange(pm.shape[0], device=self.device)
                    fi, pi = fi[om], new[pi.long()[om]]
                pts = res.pts.reshape(-1, 3)
                if pi.numel() and int(pi.max()) >= pts.shape[0]:      # (a last round that kept nothing: no solve followed it)
                    fi, pi = fi[:0], pi[:0]
                cams_h = res.cams.reshape(F, 6).cpu().numpy()
                ext = np.stack([np.concatenate([_rodrigues_matrix(c[:3]), c[3:, None]], axis=1) for c in cams_h])
            opt = plan.dense
            ranges = self.depth_ranges(ext, pts, fi, pi, opt["depth_margin"], opt["min_points"])
            return self.dense(frames, K, ext, ranges, **opt)

    # ------------------------------------------------------------------------------------------- whole clip
    def run(self, frames, K, extrinsics=None, ba=True, ftol=1e-4, verbose=0, dist=None, timers=None, max_nfev=None,
            force_collectives=False, triangulation="two_view", cull=None, verify=None, poses=None, resect=None, degeneracy=None,
            guided=None, align=None, refine=None, dense=None):
        """frames [F,H,W] u8 (device), K [3,3], extrinsics [F, 3|4, 4] (None with `poses`).  With `dist` = torch.distributed
        (initialised), frames are the FULL clip on every rank (synthetic input is generated locally) and the work is sharded as
        described in parallel.py; `cull`, `poses`, `resect`, `align`, `refine` and `dense` need one rank (`run_plan` says why).
        `force_collectives`: take the gather / all-reduce path even in a one-rank group (the collectives are trivial but travel
        the real backend: how backend "nccl" is exercised on a single GPU).  `ba`, `ftol`, `max_nfev`: whether the adjustment
        runs, its tolerance and its evaluation budget (None = SciPy's default, as adjustPoints).  `timers`: a dict the stages'
        milliseconds are added to (detect, match, verify, degeneracy, guided, link, poses, align, triangulate, resect, ba,
        ba_solve, refine, dense).
        `triangulation`: "two_view" (default) triangulates a track from its first and last observation, as the reference
        does; "multi_view" from all its observations (`triangulate_multi_view`).  `points0` is [T,3] over all tracks either way.
        `cull` (needs "multi_view"): dict of the thresholds of ops.triangulate_tracks (max_reproj_px, min_angle_deg, min_depth,
        refine_iters).  The adjustment then takes only the tracks no test flagged, `kept_tracks` (indices in track order), and
        its points are aligned with that list.
        The stages that are off by default, each None or a dict ({} for the defaults) described where it is judged: `verify`
        (verify_options), `degeneracy` (degeneracy_options), `guided` (guided_options), `poses` (pose_options), `align`
        (align_options), `resect` (resect_options), `refine` (refine_options), `dense` (dense_options).  A stage that is None
        launches nothing.

        -> dict(det (`detect` of this rank's frames), n_tracks, n_obs, points0, track_ptr_dev, obs_frame_dev, obs_kp_dev, xy_dev,
        match_count, kp_count, pairs_local, frames_local); under "multi_view" also track_quality [T,4], track_flags [T] and with
        cull kept_tracks; after the adjustment ba (its result), n_obs_local, cam_span, n_pairs; and one entry per stage that is
        on, over this rank's n pairs: verify = dict(info [n,4], cost [n], F [n,9], matches_in [n]); degeneracy = dict(H [n,9],
        cost [n], info [n,6], and with poses pose_info [n,8], sigma [n,3], normal [n,3]); guided = dict(info [n,4], is_new
        [n,cap]); poses = what `recover_poses` returns, without depth; align = what `align` returns, and after the adjustment
        ba_aligned = dict(extrinsics [F,3,4], points, sim, info); resect = what `resect` returns, without inlier; refine = what
        bundleAdjuster.refine_rounds returns; dense = what `dense` returns (at the final cameras and points)."""
        plan = run_plan(lambda: frames.shape[0], lambda: None if dist is None else dist.get_world_size(), extrinsics is not None,
                        force_collectives, triangulation, cull, verify, poses, resect, degeneracy, guided, align, refine, dense)
        rank = dist.get_rank() if dist is not None else 0
        clock = StageClock(self.ctx, timers if timers is not None else {})
        front = self._front(frames, plan, rank, clock)
        tracks, m_h, n_h = self._link(front, plan, rank, dist, clock)
        ext, recovered = self._poses(front, plan, K, extrinsics, clock)
        ext, X, quality, flags, aligned, resected = self._structure(plan, K, ext, recovered, tracks, clock)
        track_ptr, obs_frame, obs_kp, xy_dev = tracks
        out = dict(det=front.det, n_tracks=track_ptr.shape[0] - 1, n_obs=obs_frame.shape[0], points0=X, track_ptr_dev=track_ptr,
                   obs_frame_dev=obs_frame, obs_kp_dev=obs_kp, xy_dev=xy_dev, match_count=m_h, kp_count=n_h,
                   pairs_local=front.pairs_local, frames_local=front.frames_local)
        for name, value in (("verify", front.verify), ("poses", recovered), ("degeneracy", front.degeneracy),
                            ("guided", front.guided), ("resect", resected), ("align", aligned)):
            if value is not None:
                out[name] = value
        kept = None
        if plan.triangulation == "multi_view":
            out.update(track_quality=quality, track_flags=flags)
            if plan.cull is not None:
                kept = torch.nonzero(flags == 0).reshape(-1)
                out["kept_tracks"] = kept
        if ba and out["n_obs"] > 0 and (kept is None or kept.numel() > 0):
            out.update(self._adjust(plan, K, ext, X, kept, tracks, rank, ftol, max_nfev, verbose, clock))
        if plan.dense is not None:
            out["dense"] = self._dense(plan, frames, K, ext, X, kept, tracks, out, clock)
        return out

    def _front(self, frames, plan, rank, clock):
        """This rank's frames and pairs: detect, match, and the pair stages that are on (verify, degeneracy, guided) -> _Front."""
        (p_lo, p_hi), (f_lo, f_hi) = parallel.pair_block(plan.n_frames, rank, plan.world)
        if f_hi <= f_lo:
            for name in ("detect", "match", "verify", "degeneracy", "guided"):      # (its timers still open and close)
                if getattr(plan, name, True) is not None:
                    with clock(name):
                        pass
            return self._empty_front(plan)
        with clock("detect"):
            det = self.detect(frames[f_lo:f_hi])
        with clock("match"):
            pairs, m = self.match(det)
        verified = degenerate = guided_out = is_deg = None
        if plan.verify is not None:
            with clock("verify"):
                pairs_in, matches_in = pairs, m
                pairs, m, F_v, cost_v, info_v = self.verify(det, pairs, m, pair_lo=p_lo, **plan.verify)
                verified = dict(info=info_v, cost=cost_v, F=F_v, matches_in=matches_in)
        if plan.degeneracy is not None:
            with clock("degeneracy"):
                pairs_h, m_hg, H_d, cost_d, info_d = self.homography(det, pairs_in, matches_in, verify_info=info_v, pair_lo=p_lo,
                                                                     **_only(plan.degeneracy, DEGENERACY_HOMOGRAPHY_KEYS))
                is_deg = (info_d[:, 0] & ops.HOMOG_DEGENERATE) != 0
                pairs = torch.where(is_deg[:, None, None], pairs_h, pairs)
                m = torch.where(is_deg, m_hg, m)
                degenerate = dict(H=H_d, cost=cost_d, info=info_d)
        if plan.guided is not None:
            with clock("guided"):
                failed = (info_v[:, 0] & (ops.VERIFY_TOO_FEW | ops.VERIFY_NO_MODEL | ops.VERIFY_WEAK)) != 0
                kind_g = torch.where(failed, -1, 0).to(torch.int32)
                model_g = F_v
                if degenerate is not None:
                    kind_g = torch.where(is_deg, 1, kind_g).to(torch.int32)
                    model_g = torch.where(is_deg[:, None], H_d, F_v)
                pairs, m, new_g, info_g = self.guided(det, pairs, m, model_g, kind=kind_g, **plan.guided)
                guided_out = dict(info=info_g, is_new=new_g)
        return _Front(det, det["xy"], det["n"], pairs, m, verified, degenerate, guided_out, is_deg, int(p_hi - p_lo), int(f_hi - f_lo))

    def _empty_front(self, plan):
        """The `_front` of a rank that owns no frames: det = None and zero rows of everything else, for the gather."""
        def rows(dtype, *shape):
            return torch.zeros((0,) + shape, dtype=dtype, device=self.device)

        f64, i32 = torch.float64, torch.int32
        m = rows(i32)
        verified = dict(info=rows(i32, 4), cost=rows(f64), F=rows(f64, 9), matches_in=m) if plan.verify is not None else None
        degenerate = dict(H=rows(f64, 9), cost=rows(f64), info=rows(i32, 6)) if plan.degeneracy is not None else None
        guided_out = dict(info=rows(i32, 4), is_new=rows(torch.uint8, self.cap)) if plan.guided is not None else None
        return _Front(None, rows(torch.float32, self.cap, 2), rows(i32), rows(i32, self.cap, 2), m, verified, degenerate, guided_out,
                      None, 0, 0)

    def _link(self, front, plan, rank, dist, clock):
        """Every rank's key points and matches (gathered when the run is sharded) linked into tracks
        -> ((track_ptr, obs_frame, obs_kp, xy_dev), device tensors in the order the track consumers take them, m_h, n_h: the
        match and key point counts of the whole clip on the host)."""
        with clock("link"):
            if plan.sharded:
                # every rank needs every frame's key points and every pair's matches to link identical tracks.  The block
                # partition is arithmetic on (F, world), so every rank knows every rank's row counts: fixed-shape device
                # all-gathers (RCCL over xGMI under "nccl"), nothing goes through host memory.
                blocks = [parallel.pair_block(plan.n_frames, r, plan.world) for r in range(plan.world)]
                pair_counts = [b[0][1] - b[0][0] for b in blocks]
                last_rank_with_pairs = max(r for r in range(plan.world) if pair_counts[r] > 0)
                # frames f_lo .. f_lo+own-1 are owned; the halo frame belongs to the next rank (the last one keeps it)
                frame_counts = [pair_counts[r] + (1 if r == last_rank_with_pairs else 0) for r in range(plan.world)]
                keep = frame_counts[rank]
                xy_dev = parallel.gather_blocks(front.xy[:keep].contiguous(), frame_counts, dist)
                n_d = parallel.gather_blocks(front.n[:keep].contiguous(), frame_counts, dist)
                m_d = parallel.gather_blocks(front.m.contiguous(), pair_counts, dist)
                pairs_d = parallel.gather_blocks(front.pairs.contiguous(), pair_counts, dist)
            else:
                xy_dev, n_d, m_d, pairs_d = front.xy, front.n, front.m, front.pairs
            m_h = m_d.cpu().numpy()
            n_h = n_d.cpu().numpy()
            track_ptr, obs_frame, obs_kp, bad = ops.link_tracks_device(n_d, xy_dev, m_d, pairs_d, self.ctx)
            if bad:
                raise MMError("link: match index outside the key point tables")
        return (track_ptr, obs_frame, obs_kp, xy_dev), m_h, n_h

    def _poses(self, front, plan, K, extrinsics, clock):
        """The extrinsics in use -> (ext [F,3,4] on the host, the `poses` entry of the result or None): the given ones, or the
        ones `recover_poses` chains from the linked matches -- with `degeneracy`, the homography's pose in the rows of the
        degenerate pairs, that call billed to "degeneracy"."""
        if plan.poses is None:
            return np.asarray(extrinsics, float)[:, :3, :], None
        det, pairs, m, is_deg = front.det, front.pairs, front.m, front.is_deg

        def homography_rows(R, t, depth, info):
            with clock.paused("poses"), clock("degeneracy"):
                hkw = _only(plan.degeneracy, DEGENERACY_POSE_KEYS)
                if "min_matches" in plan.poses:
                    hkw["min_matches"] = plan.poses["min_matches"]
                R_h, t_h, sigma_h, normal_h, depth_h, info_h = ops.recover_poses_homography(det["xy"], pairs, m, front.degeneracy["H"],
                                                                                            K, ctx=self.ctx, **hkw)
                R = torch.where(is_deg[:, None], R_h, R)
                t = torch.where(is_deg[:, None], t_h, t)
                depth = torch.where(is_deg[:, None, None], depth_h, depth)
                info = torch.where(is_deg[:, None], info_h, info)
                front.degeneracy.update(pose_info=info_h, sigma=sigma_h, normal=normal_h)
            return R, t, depth, info

        with clock("poses"):
            recovered = self.recover_poses(det, pairs, m, front.verify["F"], K,
                                           override=homography_rows if plan.degeneracy is not None else None, **plan.poses)
            recovered.pop("depth")
            ext = recovered["extrinsics"].cpu().numpy()
        return ext, recovered

    def _triangulated(self, plan, K, ext, tracks, clock):
        """(points, quality, flags) of the linked tracks under the extrinsics `ext`; two-view has no quality or flags."""
        proj = np.einsum("ij,fjk->fik", np.asarray(K, float), ext)   # K [R|t], processor.py:184,448
        with clock("triangulate"):
            if plan.triangulation == "multi_view":
                return self.triangulate_multi_view(*tracks, proj, **(plan.cull or {}))
            return self.triangulate(*tracks, proj), None, None

    def _structure(self, plan, K, ext, recovered, tracks, clock):
        """align, triangulate, and with `resect` every frame registered against the points and the tracks triangulated again
        -> (ext in use [F,3,4] on the host, X, quality, flags, the `align` and `resect` entries of the result or None)."""
        aligned = resected = None
        if plan.align is not None:
            with clock("align"):
                ext_d = torch.as_tensor(np.ascontiguousarray(ext, dtype=np.float64)).to(self.device)
                aligned = self.align(ext_d, plan.align)
                ops.apply_similarity(aligned["sim"], None, ext_d, ctx=self.ctx)      # (a NaN sim -- no model -- changes nothing)
                if recovered is not None:
                    recovered["extrinsics"] = ext_d
                ext = ext_d.cpu().numpy()
        X, quality, flags = self._triangulated(plan, K, ext, tracks, clock)
        if plan.resect is not None and tracks[0].shape[0] > 1:
            with clock("resect"):
                resected = self.resect(K, X, *tracks, plan.n_frames, pt_ok=(flags == 0) if plan.triangulation == "multi_view" else None,
                                       prior=ext, **plan.resect)
                resected.pop("inlier")
                ext = resected["extrinsics"].cpu().numpy()
            X, quality, flags = self._triangulated(plan, K, ext, tracks, clock)
        return ext, X, quality, flags, aligned, resected

    def _adjust(self, plan, K, ext, X, kept, tracks, rank, ftol, max_nfev, verbose, clock):
        """The global adjustment of the kept tracks (all of them without cull; this rank's share when sharded), then `refine`
        and the second registration of `align` -> what the result gains: ba, n_obs_local, cam_span, n_pairs, refine, ba_aligned."""
        F, d = plan.n_frames, self.device
        with clock("ba"):
            with np.errstate(all="ignore"):
                cams0 = frameParameters(ext).reshape(F, 6)
            # managePoints order (point-major, insertion order inside a track), assembled on the device
            if kept is not None:
                # (mm_flatten_offsets + mm_flatten_tracks: the kept tracks, in track order)
                coords_d, of_d, pi_d = ops.flatten_tracks(*tracks, sel=kept, ctx=self.ctx)
                pb = ops.BADevice(K, of_d, pi_d, coords_d, F, int(kept.numel()), d, self.ctx)
                pts0 = X[kept].contiguous()
            else:
                lo, hi = 0, tracks[0].shape[0] - 1
                if plan.world > 1:
                    lo, hi, _, _ = parallel.partition_tracks(tracks[0], rank, plan.world)
                # (mm_flatten_tracks: this rank's tracks lo .. hi - 1)
                coords_d, of_d, pi_d = ops.flatten_tracks(*tracks, t_lo=lo, n_sel=hi - lo, ctx=self.ctx)
                pb = ops.BADevice(K, of_d, pi_d, coords_d, F, hi - lo, d, self.ctx)
                pts0 = X[lo:hi].contiguous()
            solver = SchurTRF(pb, allreduce=parallel.AllReduce(force=plan.force_collectives) if plan.sharded else None)
            cams_d = torch.as_tensor(cams0).to(d)
            with clock("ba_solve"):
                res = solver.solve(cams_d, pts0, ftol=ftol, max_nfev=max_nfev, verbose=verbose if rank == 0 else 0)
        out = dict(ba=res, n_obs_local=pb.O, cam_span=pb.cam_span, n_pairs=pb.n_pairs)
        if plan.refine is not None:
            with clock("refine"):
                out["refine"] = refine_rounds(pb, res, K, plan.refine, verbose=verbose)
                res = out["refine"]["ba"]
        if plan.align is not None:
            with clock("align"):
                cams_h = res.cams.reshape(F, 6).cpu().numpy()
                ext_b = np.stack([np.concatenate([_rodrigues_matrix(c[:3]), c[3:, None]], axis=1) for c in cams_h])
                ext_b = torch.as_tensor(np.ascontiguousarray(ext_b)).to(d)
                again = self.align(ext_b, plan.align)
                pts_b = res.pts.reshape(-1, 3).clone().contiguous()
                ops.apply_similarity(again["sim"], pts_b, ext_b, ctx=self.ctx)
                out["ba_aligned"] = dict(extrinsics=ext_b, points=pts_b, sim=again["sim"], info=again["info"])
        return out
