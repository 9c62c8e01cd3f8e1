"""Camera resection (ClipPipeline.run(resect=...)) on the rendered clip of tools/bench_verify.py (200 x 1080p, 4000 key points
per frame).

Reported: the `resect` stage (mm_resect_cameras, the four kernels of one call) warm, in HIP-event time (median and minimum of
--reps), beside the `verify` and `poses` stages measured the same way and the time of one evaluation of the global adjustment;
the kernels of one call alone; the flag histogram, rows and inliers per camera and how many cameras the prior, a sampled
hypothesis or the polish decided; the resected poses against the clip's TRUE extrinsics after the similarity alignment of the
camera centres tools/bench_poses.py uses (worst rotation error in degrees, worst camera-centre error as a fraction of the orbit
radius), beside the recovered poses they started from; and the global bundle adjustment from recovered poses with and without
`resect`: initial cost, evaluations, final cost.

usage: python tools/bench_resect.py [--frames 200] [--width 1920] [--height 1080] [--nfeatures 4000] [--reps 20]
                                    [--max-nfev N] [--json OUT]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_poses import centres, chain_error, event_ms  # noqa: E402
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
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    ctx = default_context()
    dev = ctx.device
    F, W, H = a.frames, a.width, a.height
    K = synth.default_K(W, H, f=525.0 * W / 640.0)
    frames, ext_gt, _ = synth.render_orbit_frames_torch(F, W, H, dev, arc_deg=min(360.0, 0.72 * F), seed=7, K=K)
    ext_gt = np.asarray(ext_gt, float)[:, :3, :]
    radius = float(np.linalg.norm(centres(ext_gt)[:, [0, 2]], axis=1).mean())
    pipe = ClipPipeline(H, W, a.nfeatures, batch=16, device=dev, ctx=ctx)
    summary = dict(frames=F, width=W, height=H, nfeatures=a.nfeatures, reps=a.reps, orbit_radius=radius)

    # ---- the run the stage is cut from: verified matches, recovered poses, two-view points
    base = pipe.run(frames, K, None, ba=False, verify={}, poses={})
    det = base["det"]
    pairs, m = pipe.match(det)
    pairs_v, m_v, F_v, _, _ = pipe.verify(det, pairs, m)
    prior = base["poses"]["extrinsics"]
    tracks = (base["track_ptr_dev"], base["obs_frame_dev"], base["obs_kp_dev"], base["xy_dev"])
    X = base["points0"]
    # the arguments of the one call, built once: the stage time is the call's, not the index build's
    coords, fi, pi = ops.flatten_tracks(*tracks, ctx=ctx)
    fl = fi.long()
    cam_obs = torch.argsort(fl, stable=True).to(torch.int32)
    cam_ptr = torch.zeros(F + 1, dtype=torch.int32, device=dev)
    cam_ptr[1:] = torch.cumsum(torch.bincount(fl, minlength=F)[:F], 0).to(torch.int32)
    pr = prior.reshape(F, 12).contiguous()

    def call():
        return ops.resect_cameras(K, X, coords, pi, cam_ptr, cam_obs, prior=pr, ctx=ctx)

    stage = dict(verify=event_ms(ctx, lambda: pipe.verify(det, pairs, m), a.reps),
                 poses=event_ms(ctx, lambda: pipe.recover_poses(det, pairs_v, m_v, F_v, K), a.reps),
                 resect=event_ms(ctx, call, a.reps),
                 resect_with_index_build=event_ms(ctx, lambda: pipe.resect(K, X, *tracks, F, prior=prior), a.reps))
    ctx.profile(1)
    ext_r, cost_r, inl_r, info_r = call()
    ctx.sync()
    kernels = {k: round(v[1], 4) for k, v in ctx.profile_report().items()}
    ctx.profile(0)
    summary["stage_ms_median_min"] = stage
    summary["resect_kernel_ms"] = kernels
    print(json.dumps(dict(stage_ms_median_min=stage, resect_kernel_ms=kernels)))

    # ---- flags, counts, and the poses against the truth
    info = info_r.cpu().numpy()
    fl_ = info[:, 0]
    rot0, cen0, _ = chain_error(prior.cpu().numpy(), ext_gt, radius)
    rot1, cen1, _ = chain_error(ext_r.cpu().numpy(), ext_gt, radius)
    cams = dict(cameras=int(F), observations=int(coords.shape[0]), tracks=int(X.shape[0]),
                usable_rows=dict(mean=round(float(info[:, 4].mean()), 1), min=int(info[:, 4].min()), max=int(info[:, 4].max())),
                inliers=dict(mean=round(float(info[:, 1].mean()), 1), min=int(info[:, 1].min()), max=int(info[:, 1].max())),
                valid_hypotheses=dict(mean=round(float(info[:, 3].mean()), 1), min=int(info[:, 3].min())),
                flags=dict(ok=int((fl_ == 0).sum()), too_few=int(((fl_ & ops.RESECT_TOO_FEW) != 0).sum()),
                           no_model=int(((fl_ & ops.RESECT_NO_MODEL) != 0).sum()), weak=int(((fl_ & ops.RESECT_WEAK) != 0).sum()),
                           malformed=int(((fl_ & ops.RESECT_MALFORMED) != 0).sum())),
                prior_won=int((info[:, 2] == 256).sum()), hypothesis_won=int(((info[:, 2] >= 0) & (info[:, 2] < 256)).sum()),
                polished=int((info[:, 5] > 0).sum()),
                msac_cost_sum=float(np.nansum(cost_r.cpu().numpy())),
                recovered=dict(worst_rotation_error_deg=rot0, worst_centre_error_over_radius=cen0),
                resected=dict(worst_rotation_error_deg=rot1, worst_centre_error_over_radius=cen1))
    summary["resect"] = cams
    print(json.dumps(dict(resect=cams)))

    # ---- the global adjustment with verification on, from recovered poses, without and with the resection
    runs = []
    for name, kw in (("recovered_poses", dict()), ("recovered_poses_resected", dict(resect={}))):
        timers = {}
        r = pipe.run(frames, K, None, ba=True, ftol=1e-4, timers=timers, max_nfev=a.max_nfev or None, verify={}, poses={}, **kw)
        res = r["ba"]
        ext0 = (r["resect"] if "resect" in r else r["poses"])["extrinsics"].cpu().numpy()
        c2, f2, p2 = ops.flatten_tracks(r["track_ptr_dev"], r["obs_frame_dev"], r["obs_kp_dev"], r["xy_dev"], ctx=ctx)
        pb = ops.BADevice(K, f2, p2, c2, F, int(r["points0"].shape[0]), dev, ctx, pairs=False)
        with np.errstate(all="ignore"):
            cams0 = torch.as_tensor(frameParameters(ext0).reshape(F, 6)).to(dev)
        c0 = 0.5 * float(pb.residual(cams0.contiguous(), r["points0"].contiguous())[0].item())
        row = dict(run=name, tracks=int(r["n_tracks"]), observations=int(r["n_obs_local"]),
                   resect_ms_host_clock=round(timers.get("resect", 0.0), 3), initial_cost=c0, nfev=int(res.nfev),
                   status=int(res.status), ba_solve_ms=round(timers["ba_solve"], 2),
                   ms_per_evaluation=round(timers["ba_solve"] / max(int(res.nfev), 1), 4), final_cost=float(res.cost))
        cams1 = res.cams.cpu().numpy().reshape(F, 6)
        ext1 = np.array([np.c_[synth.rodrigues(c[:3]), c[3:]] for c in cams1])
        rot, cen, _ = chain_error(ext1, ext_gt, radius)
        row.update(adjusted_worst_rotation_error_deg=rot, adjusted_worst_centre_error_over_radius=cen)
        runs.append(row)
        print(json.dumps(row))
    summary["global_ba"] = runs
    summary["one_ba_evaluation_ms"] = runs[0]["ms_per_evaluation"]
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(summary, fh, indent=1)


if __name__ == "__main__":
    main()
