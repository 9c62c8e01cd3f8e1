"""Two-view against multi-view triangulation (ClipPipeline.run(triangulation=..., cull=...)) on the rendered clip of
tools/bench_anchored_windows.py (200 x 1080p, 4000 key points per frame).

Reported: the `triangulate` stage warm, in HIP-event time (median and minimum of --reps): two-view, multi-view with
refine_iters 0 and 8 -- each as the stage the pipeline runs (the multi-view one flattens all tracks first) and, for the
multi-view kernel, alone on observations that are already flat; the flag histogram under the cull thresholds; and the global
bundle adjustment of three runs (two-view; multi-view; multi-view with cull): initial cost, evaluations, solve time, time per
evaluation, final cost over the adjusted tracks, and final cost over the kept tracks and over all tracks (a culled track
keeps its triangulated point) so that the three can be compared.

usage: python tools/bench_triangulate.py [--frames 200] [--width 1920] [--height 1080] [--nfeatures 4000] [--reps 20]
                                         [--max-nfev N] [--json OUT]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from meatmodeler_amd import _lib, ops, synth  # noqa: E402
from meatmodeler_amd._lib import default_context  # noqa: E402
from meatmodeler_amd.bundleAdjuster import frameParameters  # noqa: E402
from meatmodeler_amd.pipeline import ClipPipeline  # noqa: E402

CULL = dict(max_reproj_px=4.0, min_angle_deg=1.0, min_depth=0.0)


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


def cost_over(pipe, out, K, F, cams, pts_all, sel=None):
    """0.5 |r|^2 of the tracks `sel` (None: all) at (cams, pts_all[sel])."""
    coords, fi, pi = ops.flatten_tracks(out["track_ptr_dev"], out["obs_frame_dev"], out["obs_kp_dev"], out["xy_dev"], sel=sel,
                                        ctx=pipe.ctx)
    pts = pts_all if sel is None else pts_all[sel]
    pb = ops.BADevice(K, fi, pi, coords, F, int(pts.shape[0]), pipe.device, pipe.ctx, pairs=False)
    c2, _ = pb.residual(cams.contiguous(), pts.contiguous())
    return 0.5 * float(c2.item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--nfeatures", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=20)
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
    tp, of_, ok, xy = out["track_ptr_dev"], out["obs_frame_dev"], out["obs_kp_dev"], out["xy_dev"]
    proj = np.einsum("ij,fjk->fik", np.asarray(K, float), np.asarray(ext, float)[:, :3, :])
    proj_d = torch.as_tensor(proj).to(dev)
    lens = (tp[1:] - tp[:-1]).cpu().numpy()
    summary = dict(frames=F, width=W, height=H, nfeatures=a.nfeatures, n_tracks=int(out["n_tracks"]), n_obs=int(out["n_obs"]),
                   track_length=dict(mean=round(float(lens.mean()), 3), max=int(lens.max()),
                                     histogram={str(k): int(v) for k, v in zip(*np.unique(np.minimum(lens, 16), return_counts=True))}),
                   reps=a.reps, cull=CULL)

    # ---- the triangulate stage, warm, HIP events
    coords, fi, _ = ops.flatten_tracks(tp, of_, ok, xy, ctx=ctx)
    stage = {}
    stage["two_view"] = event_ms(ctx, lambda: pipe.triangulate(tp, of_, ok, xy, proj), a.reps)
    for it in (0, 8):
        stage[f"multi_view_refine{it}"] = event_ms(ctx, lambda: pipe.triangulate_multi_view(tp, of_, ok, xy, proj, refine_iters=it), a.reps)
        stage[f"multi_view_refine{it}_op_on_flat_observations"] = event_ms(
            ctx, lambda: ops.triangulate_tracks(proj_d, tp, fi, coords, refine_iters=it, ctx=ctx), a.reps)
    stage["flatten_all_tracks"] = event_ms(ctx, lambda: ops.flatten_tracks(tp, of_, ok, xy, ctx=ctx), a.reps)
    # the kernels alone (per-launch events of the library, one warm call)
    ctx.profile(1)
    ops.triangulate_tracks(proj_d, tp, fi, coords, refine_iters=0, ctx=ctx)
    ctx.sync()
    k0 = ctx.profile_report()
    ctx.profile(0)
    ctx.profile(1)
    ops.triangulate_tracks(proj_d, tp, fi, coords, refine_iters=8, ctx=ctx)
    ctx.sync()
    k8 = ctx.profile_report()
    ctx.profile(0)
    summary["triangulate_stage_ms_median_min"] = stage
    summary["kernel_ms"] = dict(refine0={k: round(v[1], 4) for k, v in k0.items()}, refine8={k: round(v[1], 4) for k, v in k8.items()})
    print(json.dumps(dict(triangulate_stage_ms_median_min=stage, kernel_ms=summary["kernel_ms"])))

    # ---- verdicts
    X, quality, flags = ops.triangulate_tracks(proj_d, tp, fi, coords, ctx=ctx, **CULL)
    fl = flags.cpu().numpy()
    hist = dict(total=int(len(fl)), kept=int((fl == 0).sum()), behind=int(((fl & ops.TRI_BEHIND) != 0).sum()),
                reproj=int(((fl & ops.TRI_REPROJ) != 0).sum()), parallax=int(((fl & ops.TRI_PARALLAX) != 0).sum()),
                degenerate=int(((fl & ops.TRI_DEGENERATE) != 0).sum()),
                by_value={str(k): int(v) for k, v in zip(*np.unique(fl, return_counts=True))})
    summary["flags"] = hist
    print(json.dumps(dict(flags=hist)))
    kept = torch.nonzero(flags == 0).reshape(-1)

    # ---- the global adjustment, three ways
    with np.errstate(all="ignore"):
        cams0 = torch.as_tensor(frameParameters(np.asarray(ext, float)[:, :3, :]).reshape(F, 6)).to(dev)
    runs = []
    for name, kw in (("two_view", {}), ("multi_view", dict(triangulation="multi_view")),
                     ("multi_view_cull", dict(triangulation="multi_view", cull=CULL))):
        timers = {}
        r = pipe.run(frames, K, ext, ba=True, ftol=1e-4, timers=timers, max_nfev=a.max_nfev or None, **kw)
        res = r["ba"]
        pts0 = r["points0"]
        mine = r.get("kept_tracks")
        assert mine is None or torch.equal(mine, kept)
        pts1 = pts0.clone()
        if mine is None:
            pts1[:] = res.pts
        else:
            pts1[mine] = res.pts
        row = dict(run=name, adjusted_tracks=int(res.pts.shape[0]), observations=int(r["n_obs_local"]),
                   triangulate_ms_host_clock=round(timers["triangulate"], 3),
                   initial_cost=cost_over(pipe, out, K, F, cams0, pts0, mine),
                   initial_cost_kept_tracks=cost_over(pipe, out, K, F, cams0, pts0, kept),
                   initial_cost_all_tracks=cost_over(pipe, out, K, F, cams0, pts0),
                   nfev=int(res.nfev), status=int(res.status), ba_solve_ms=round(timers["ba_solve"], 2),
                   ms_per_evaluation=round(timers["ba_solve"] / max(int(res.nfev), 1), 4), final_cost=float(res.cost),
                   final_cost_kept_tracks=cost_over(pipe, out, K, F, res.cams, pts1, kept),
                   final_cost_all_tracks=cost_over(pipe, out, K, F, res.cams, pts1))
        runs.append(row)
        print(json.dumps(row))
    summary["global_ba"] = runs
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(summary, fh, indent=1)


if __name__ == "__main__":
    main()
