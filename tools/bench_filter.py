"""The observation filter (ops.filter_observations) beside one residual sweep of the adjustment at the same
shape, and the global adjustment of a rendered clip with and without ClipPipeline.run(refine=...).

Reported: on synth.make_ba_problem(--ba-frames, --ba-points, track_len 8) with 2 % of the observations displaced by 40 to
120 px, warm, in HIP-event time (median and minimum of --reps): the whole filter call (its allocations and the one host read
of the counts included), its kernels one by one (per-launch events of the library), and one mm_ba_residual sweep; the bytes
the filter moves and the rate that makes.  Then, on the rendered clip of tools/bench_triangulate.py: the adjustment alone and
with refine -- evaluations, cost, RMS, observations and points kept, per round.

usage: python tools/bench_filter.py [--ba-frames 500] [--ba-points 250000] [--frames 200] [--width 1920] [--height 1080]
                                    [--nfeatures 4000] [--reps 20] [--max-nfev N] [--skip-clip] [--json OUT]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from meatmodeler_amd import _lib, ops, synth  # noqa: E402
from meatmodeler_amd._lib import default_context  # noqa: E402
from meatmodeler_amd.bundleAdjuster import frameParameters  # noqa: E402
from meatmodeler_amd.pipeline import ClipPipeline  # noqa: E402

TESTS = dict(max_reproj_px=4.0, min_angle_deg=1.0, min_depth=0.0)
REFINE = dict(max_reproj_px=(8.0, 4.0), min_angle_deg=1.0, min_depth=0.0, rounds=2)


def event_ms(ctx, fn, reps):
    """HIP-event time of fn() on the context's stream: (median, min) of `reps` after two warm calls."""
    tm = _lib.Timer(ctx)
    for _ in range(2):
        fn()
    ms = []
    for _ in range(reps):
        tm.start()
        fn()
        tm.stop()
        ms.append(tm.elapsed_ms())
    return round(float(np.median(ms)), 4), round(float(np.min(ms)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ba-frames", type=int, default=500)
    ap.add_argument("--ba-points", type=int, default=250000)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--nfeatures", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--max-nfev", type=int, default=0)
    ap.add_argument("--skip-clip", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    ctx = default_context()
    dev = ctx.device
    summary = dict(reps=a.reps, tests=TESTS)

    # ---- the filter beside one residual sweep
    pr = synth.make_ba_problem(a.ba_frames, a.ba_points, 8, seed=1)
    F, P, O = a.ba_frames, a.ba_points, len(pr["fi"])
    rng = np.random.default_rng(9)
    obs = pr["obs"].copy()
    hit = rng.choice(O, size=O // 50, replace=False)
    ang, mag = rng.uniform(0, 2 * np.pi, hit.size), rng.uniform(40.0, 120.0, hit.size)
    obs[hit] += np.stack([mag * np.cos(ang), mag * np.sin(ang)], axis=1)
    with np.errstate(all="ignore"):
        cams = torch.as_tensor(frameParameters(pr["ext"]).reshape(F, 6)).to(dev)
    pts = torch.as_tensor(pr["pts0"]).to(dev)
    pb = ops.BADevice(pr["K"], pr["fi"], pr["pi"], obs, F, P, dev, ctx, pairs=False)
    flt = ops.filter_observations(cams, pts, pr["K"], pb, ctx=ctx, **TESTS)
    call = event_ms(ctx, lambda: ops.filter_observations(cams, pts, pr["K"], pb, ctx=ctx, **TESTS), a.reps)
    sweep = event_ms(ctx, lambda: pb.residual(cams, pts), a.reps)
    sweep_res = event_ms(ctx, lambda: pb.residual(cams, pts, want_res=True), a.reps)
    ctx.profile(1)
    ops.filter_observations(cams, pts, pr["K"], pb, ctx=ctx, **TESTS)
    ctx.sync()
    kernels = {k: round(v[1], 4) for k, v in ctx.profile_report().items()}
    ctx.profile(0)
    kept = flt["n_obs"]
    # per observation: fi, pi, obs, the point, flags written, read twice and rewritten by the orphan pass; err, depth; the
    # compacted row (fi, pi, obs, map) of a kept one and the reads that feed it
    moved = O * (4 + 4 + 16 + 24 + 4 + 8 + 8) + O * (4 + 4 + 4) + O * (4 + 4) + kept * (4 + 4 + 16 + 4) + kept * (4 + 4 + 16 + 4) \
        + P * (24 + 8 + 4 + 4 + 4)
    kernel_ms = sum(kernels.values())
    part = dict(frames=F, points=P, observations=O, displaced=int(hit.size), kept_observations=kept, kept_points=flt["n_points"],
                removed_observations_own_test=flt["removed_obs"], removed_points=flt["removed_points"],
                filter_call_ms_median_min=call, filter_kernels_ms=kernels, filter_kernels_ms_sum=round(kernel_ms, 4),
                residual_sweep_ms_median_min=sweep, residual_sweep_with_residuals_ms_median_min=sweep_res,
                filter_bytes_moved=int(moved), filter_kernels_GBps=round(moved / (kernel_ms * 1e-3) / 1e9, 1))
    summary["filter_vs_residual_sweep"] = part
    print(json.dumps(part))

    # ---- the global adjustment of the rendered clip, with and without refine
    if not a.skip_clip:
        Fc, W, H = a.frames, a.width, a.height
        K = synth.default_K(W, H, f=525.0 * W / 640.0)
        frames, ext_gt, _ = synth.render_orbit_frames_torch(Fc, W, H, dev, arc_deg=min(360.0, 0.72 * Fc), seed=7, K=K)
        rng = np.random.default_rng(5)      # poses: ground truth + small noise, as bench.py
        ext = ext_gt.copy()
        for f in range(Fc):
            ext[f, :, :3] = synth.rodrigues(rng.normal(0, 5e-4, 3)) @ ext_gt[f, :, :3]
            ext[f, :, 3] += rng.normal(0, 2e-3, 3)
        pipe = ClipPipeline(H, W, a.nfeatures, batch=16, device=dev, ctx=ctx)
        runs = []
        for name, kw in (("ba", {}), ("ba_refine", dict(refine=REFINE))):
            timers = {}
            r = pipe.run(frames, K, ext, ba=True, ftol=1e-4, timers=timers, max_nfev=a.max_nfev or None, **kw)
            res = r["ba"]
            row = dict(run=name, tracks=int(r["n_tracks"]), observations=int(r["n_obs"]), nfev=int(res.nfev), status=int(res.status),
                       cost=float(res.cost), rms_px=round(math.sqrt(2 * res.cost / r["n_obs"]), 4),
                       ba_solve_ms=round(timers["ba_solve"], 2))
            if "refine" in r:
                rf = r["refine"]
                last = rf["ba"]
                n_o = int(rf["obs_map"].numel())
                row.update(refine_ms=round(timers["refine"], 2), rounds=rf["rounds"], kept_observations=n_o,
                           kept_points=int(rf["point_map"].numel()), refined_cost=float(last.cost),
                           refined_rms_px=round(math.sqrt(2 * last.cost / max(n_o, 1)), 4),
                           nfev_total=int(res.nfev) + sum(x["nfev"] for x in rf["rounds"]))
            runs.append(row)
            print(json.dumps(row))
        summary["clip"] = dict(frames=Fc, width=W, height=H, nfeatures=a.nfeatures, refine=REFINE, runs=runs)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(summary, fh, indent=1)


if __name__ == "__main__":
    main()
