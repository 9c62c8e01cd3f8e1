"""Sliding-window bundle adjustment, boundary="inside" against boundary="anchored" (ClipPipeline.adjust_windows), on the
same rendered clip and the same `run(..., ba=False)` output.  Per mode: windows, points, observations, fixed cameras per
window, total evaluations, wall time, time per evaluation, and the final reprojection cost over all finished tracks (one
mm_ba_residual over the whole clip at the written-back cameras and points).

usage: python tools/bench_anchored_windows.py [--frames 200] [--width 1920] [--height 1080] [--nfeatures 4000]
                                              [--window 50] [--stride 25] [--max-nfev N] [--json OUT]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from meatmodeler_amd import ops, synth  # noqa: E402
from meatmodeler_amd._lib import default_context  # noqa: E402
from meatmodeler_amd.pipeline import ClipPipeline  # noqa: E402


def total_cost(pipe, out, K, cams, pts, F):
    """0.5 |r|^2 over every finished track of the clip (the tracks either mode may adjust) at (cams, pts)."""
    tp, of_ = out["track_ptr_dev"], out["obs_frame_dev"]
    tp64 = tp.long()
    last = of_[tp64[1:] - 1]
    sel = torch.nonzero(ClipPipeline.window_selection_anchored(None, last, 0, F, F)).reshape(-1)
    coords, fi, pi = ops.flatten_tracks(tp, of_, out["obs_kp_dev"], out["xy_dev"], sel=sel, ctx=pipe.ctx)
    pb = ops.BADevice(K, fi, pi, coords, F, int(sel.numel()), pipe.device, pipe.ctx)
    c2, _ = pb.residual(cams.contiguous(), pts[sel].contiguous())
    return 0.5 * float(c2.item()), int(sel.numel()), int(fi.numel())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--nfeatures", type=int, default=4000)
    ap.add_argument("--window", type=int, default=50)
    ap.add_argument("--stride", type=int, default=25)
    ap.add_argument("--max-nfev", type=int, default=0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    ctx = default_context()
    dev = ctx.device
    F, W, H = a.frames, a.width, a.height
    K = synth.default_K(W, H, f=525.0 * W / 640.0)
    frames, ext_gt, _ = synth.render_orbit_frames_torch(F, W, H, dev, arc_deg=min(360.0, 0.72 * F), seed=7, K=K)
    rng = np.random.default_rng(5)      # poses: ground truth + small noise, as bench.py
    ext = ext_gt.copy()
    for f in range(F):
        ext[f, :, :3] = synth.rodrigues(rng.normal(0, 5e-4, 3)) @ ext_gt[f, :, :3]
        ext[f, :, 3] += rng.normal(0, 2e-3, 3)
    pipe = ClipPipeline(H, W, a.nfeatures, batch=16, device=dev, ctx=ctx)
    out = pipe.run(frames, K, ext, ba=False)
    torch.cuda.synchronize()
    results = {}
    for mode in ("inside", "anchored", "inside", "anchored"):      # (second round: warm, the one reported)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        w = pipe.adjust_windows(out, K, ext, window=a.window, stride=a.stride, ftol=1e-4, boundary=mode,
                                max_nfev=a.max_nfev or None)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        wins = w["windows"]
        nfev = sum(s["nfev"] for s in wins)
        cost, n_tracks, n_obs = total_cost(pipe, out, K, w["cams"], w["points"], F)
        results[mode] = dict(mode=mode, windows=len(wins), points=[s["points"] for s in wins],
                             observations=[s["observations"] for s in wins],
                             fixed_cameras=[s.get("fixed_cameras", 0) for s in wins], nfev_total=nfev, wall_ms=round(ms, 2),
                             ms_per_evaluation=round(ms / max(nfev, 1), 4),
                             obs_per_evaluation=round(sum(s["observations"] * s["nfev"] for s in wins) / max(nfev, 1), 1),
                             final_total_cost=cost, finished_tracks=n_tracks, finished_track_observations=n_obs)
    summary = dict(frames=F, width=W, height=H, nfeatures=a.nfeatures, window=a.window, stride=a.stride,
                   n_tracks=int(out["n_tracks"]), modes=[results["inside"], results["anchored"]])
    for r in summary["modes"]:
        print(json.dumps(r))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(summary, fh, indent=1)


if __name__ == "__main__":
    main()
