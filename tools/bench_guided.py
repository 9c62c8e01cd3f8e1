"""Guided matching (ClipPipeline.run(verify=..., guided=...)) on the rendered clip of tools/bench_verify.py (200 x 1080p, 4000
key points per frame).

Reported: the `guided` stage warm, in HIP-event time (median and minimum of --reps), beside the `match` and `verify` stages
measured the same way in the same run; the kernels of one guided call alone; the matches added per pair and the share of
unused key points that found one; of the added matches the share whose Sampson distance under the TRUE fundamental matrix
(from the clip's extrinsics and K) exceeds 4 px, beside the same share of the seeds; tracks, observations and mean track
length with and without the stage; and the global bundle adjustment of {no verify, verify, verify + guided} x {two-view,
multi-view + cull}: tracks, initial cost, evaluations, solve time, final cost.

usage: python tools/bench_guided.py [--frames 200] [--width 1920] [--height 1080] [--nfeatures 4000] [--reps 20]
                                    [--max-nfev N] [--no-ba] [--json OUT]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_verify import CULL, FAR_PX, event_ms, sampson_px, true_fundamental  # noqa: E402
from meatmodeler_amd import ops, synth  # noqa: E402
from meatmodeler_amd._lib import default_context  # noqa: E402
from meatmodeler_amd.bundleAdjuster import frameParameters  # noqa: E402
from meatmodeler_amd.pipeline import ClipPipeline  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--nfeatures", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--max-nfev", type=int, default=0)
    ap.add_argument("--no-ba", action="store_true", help="skip the six global adjustments")
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
    summary = dict(frames=F, width=W, height=H, nfeatures=a.nfeatures, reps=a.reps, cull=CULL, far_px=FAR_PX)

    def dump():
        if a.json:
            with open(a.json, "w") as fh:
                json.dump(summary, fh, indent=1)

    # ---- the stages, warm, HIP events
    det = pipe.detect(frames)
    pairs, m = pipe.match(det)
    pairs_v, m_v, F_v, _, info_v = pipe.verify(det, pairs, m)
    kind = torch.where((info_v[:, 0] & 7) != 0, -1, 0).to(torch.int32)
    stage = dict(match=event_ms(ctx, lambda: pipe.match(det), a.reps),
                 verify=event_ms(ctx, lambda: pipe.verify(det, pairs, m), a.reps),
                 guided=event_ms(ctx, lambda: pipe.guided(det, pairs_v, m_v, F_v, kind=kind), a.reps))
    ctx.profile(1)
    pairs_g, m_g, new_g, info_g = pipe.guided(det, pairs_v, m_v, F_v, kind=kind)
    ctx.sync()
    kernels = {k: round(v[1], 4) for k, v in ctx.profile_report().items()}
    ctx.profile(0)
    summary["stage_ms_median_min"] = stage
    summary["guided_kernel_ms"] = kernels
    print(json.dumps(dict(stage_ms_median_min=stage, guided_kernel_ms=kernels)), flush=True)

    # ---- what was added, judged by the true epipolar geometry
    xy = det["xy"].cpu().numpy()
    n_h = det["n"].cpu().numpy()
    pg, mg, ng, info, mv = (t.cpu().numpy() for t in (pairs_g, m_g, new_g, info_g, m_v))
    Ft = true_fundamental(K, ext_gt)
    far_new = far_seed = n_new = n_seed = 0
    for p in range(F - 1):
        rows, fresh = pg[p, :mg[p]], ng[p, :mg[p]] != 0
        far = sampson_px(Ft[p], xy[p, rows[:, 0]].astype(float), xy[p + 1, rows[:, 1]].astype(float)) > FAR_PX
        n_new += int(fresh.sum())
        n_seed += int((~fresh).sum())
        far_new += int((far & fresh).sum())
        far_seed += int((far & ~fresh).sum())
    unused = int((n_h[:-1] - mv).sum())
    fl = info[:, 0]
    added = dict(seeds=n_seed, added=n_new, share_added=round(n_new / max(n_seed, 1), 5),
                 added_per_pair=dict(mean=round(float(info[:, 2].mean()), 1), min=int(info[:, 2].min()), max=int(info[:, 2].max())),
                 proposals_per_pair=round(float(info[:, 3].mean()), 1), unused_queries=unused,
                 share_of_unused_queries_matched=round(n_new / max(unused, 1), 5),
                 added_beyond_far_px=far_new, share_of_added_beyond_far_px=round(far_new / max(n_new, 1), 5),
                 seeds_beyond_far_px=far_seed, share_of_seeds_beyond_far_px=round(far_seed / max(n_seed, 1), 5),
                 pairs=dict(total=int(len(fl)), ok=int((fl == 0).sum()), skipped=int(((fl & ops.GUIDED_SKIPPED) != 0).sum()),
                            unordered=int(((fl & ops.GUIDED_UNORDERED) != 0).sum()),
                            malformed=int(((fl & ops.GUIDED_MALFORMED) != 0).sum())))
    summary["matches"] = added
    print(json.dumps(dict(matches=added)), flush=True)

    # ---- tracks with and without the stage
    tracks = {}
    for name, kw in (("verify", dict(verify={})), ("verify_guided", dict(verify={}, guided={}))):
        r = pipe.run(frames, K, ext, ba=False, **kw)
        tracks[name] = dict(tracks=int(r["n_tracks"]), observations=int(r["n_obs"]),
                            mean_track_length=round(int(r["n_obs"]) / max(int(r["n_tracks"]), 1), 4))
    summary["tracks"] = tracks
    print(json.dumps(dict(tracks=tracks)), flush=True)
    dump()
    if a.no_ba:
        return

    # ---- the global adjustment, six ways
    runs = []
    for name, kw in (("two_view", {}), ("two_view_verify", dict(verify={})), ("two_view_verify_guided", dict(verify={}, guided={})),
                     ("multi_view_cull", dict(triangulation="multi_view", cull=CULL)),
                     ("multi_view_cull_verify", dict(triangulation="multi_view", cull=CULL, verify={})),
                     ("multi_view_cull_verify_guided", dict(triangulation="multi_view", cull=CULL, verify={}, guided={}))):
        timers = {}
        r = pipe.run(frames, K, ext, ba=True, ftol=1e-4, timers=timers, max_nfev=a.max_nfev or None, **kw)
        res = r["ba"]
        pts0 = r["points0"] if "kept_tracks" not in r else r["points0"][r["kept_tracks"]]
        coords, fi, pi = ops.flatten_tracks(r["track_ptr_dev"], r["obs_frame_dev"], r["obs_kp_dev"], r["xy_dev"],
                                            sel=r.get("kept_tracks"), ctx=ctx)
        pb = ops.BADevice(K, fi, pi, coords, F, int(pts0.shape[0]), dev, ctx, pairs=False)
        with np.errstate(all="ignore"):
            cams0 = torch.as_tensor(frameParameters(np.asarray(ext, float)[:, :3, :]).reshape(F, 6)).to(dev)
        c0 = 0.5 * float(pb.residual(cams0.contiguous(), pts0.contiguous())[0].item())
        row = dict(run=name, tracks=int(r["n_tracks"]), adjusted_tracks=int(res.pts.shape[0]), observations=int(r["n_obs_local"]),
                   match_ms_host_clock=round(timers["match"], 3), verify_ms_host_clock=round(timers.get("verify", 0.0), 3),
                   guided_ms_host_clock=round(timers.get("guided", 0.0), 3),
                   initial_cost=c0, nfev=int(res.nfev), status=int(res.status), ba_solve_ms=round(timers["ba_solve"], 2),
                   ms_per_evaluation=round(timers["ba_solve"] / max(int(res.nfev), 1), 4), final_cost=float(res.cost))
        runs.append(row)
        print(json.dumps(row), flush=True)
        summary["global_ba"] = runs
        dump()


if __name__ == "__main__":
    main()
