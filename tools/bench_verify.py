"""Epipolar verification (ClipPipeline.run(verify=...)) on the rendered clip of tools/bench_triangulate.py (200 x 1080p, 4000
key points per frame).

Reported: the `verify` stage warm, in HIP-event time (median and minimum of --reps), beside the `match` stage measured the
same way and the time of one evaluation of the global adjustment of the same run; the kernels of one verify call alone; the
share of matches kept and the flag histogram; the share of kept and of rejected matches whose Sampson distance under the TRUE
fundamental matrix (from the clip's extrinsics and K) exceeds 4 px; and the global bundle adjustment of the four combinations
{no verify, verify} x {two-view, multi-view + cull}: tracks, initial cost, evaluations, solve time, final cost.

usage: python tools/bench_verify.py [--frames 200] [--width 1920] [--height 1080] [--nfeatures 4000] [--reps 20]
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
FAR_PX = 4.0


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


def true_fundamental(K, ext):
    """F [n-1, 3, 3] with x_{k+1}^T F x_k = 0 from the extrinsics [n, 3|4, 4] (x = K (R X + t))."""
    K = np.asarray(K, float)
    Ki = np.linalg.inv(K)
    ext = np.asarray(ext, float)[:, :3, :]
    out = []
    for a, b in zip(ext[:-1], ext[1:]):
        R = b[:, :3] @ a[:, :3].T
        t = b[:, 3] - R @ a[:, 3]
        tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
        out.append(Ki.T @ tx @ R @ Ki)
    return np.stack(out)


def sampson_px(F, x, xp):
    x1 = np.c_[x, np.ones(len(x))]
    x2 = np.c_[xp, np.ones(len(xp))]
    Fx, Ftx = x1 @ F.T, x2 @ F
    e = (x2 * Fx).sum(axis=1)
    with np.errstate(all="ignore"):
        return np.sqrt(e * e / (Fx[:, 0] ** 2 + Fx[:, 1] ** 2 + Ftx[:, 0] ** 2 + Ftx[:, 1] ** 2))


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
    summary = dict(frames=F, width=W, height=H, nfeatures=a.nfeatures, reps=a.reps, cull=CULL, far_px=FAR_PX)

    # ---- the stages, warm, HIP events
    det = pipe.detect(frames)
    pairs, m = pipe.match(det)
    stage = dict(match=event_ms(ctx, lambda: pipe.match(det), a.reps),
                 verify=event_ms(ctx, lambda: pipe.verify(det, pairs, m), a.reps))
    ctx.profile(1)
    pairs_v, m_v, F_v, cost_v, info_v = pipe.verify(det, pairs, m)
    ctx.sync()
    kernels = {k: round(v[1], 4) for k, v in ctx.profile_report().items()}
    ctx.profile(0)
    summary["stage_ms_median_min"] = stage
    summary["verify_kernel_ms"] = kernels
    print(json.dumps(dict(stage_ms_median_min=stage, verify_kernel_ms=kernels)))

    # ---- what was kept, judged by the true epipolar geometry
    xy = det["xy"].cpu().numpy()
    pairs_h, m_h, pv_h, mv_h, info = (t.cpu().numpy() for t in (pairs, m, pairs_v, m_v, info_v))
    Ft = true_fundamental(K, ext_gt)
    far_kept = far_rejected = n_kept = n_rejected = 0
    for p in range(F - 1):
        rows = pairs_h[p, :m_h[p]]
        keep = np.isin(rows[:, 0], pv_h[p, :mv_h[p], 0])      # (a query key point has at most one match)
        far = sampson_px(Ft[p], xy[p, rows[:, 0]].astype(float), xy[p + 1, rows[:, 1]].astype(float)) > FAR_PX
        n_kept += int(keep.sum())
        n_rejected += int((~keep).sum())
        far_kept += int((far & keep).sum())
        far_rejected += int((far & ~keep).sum())
    fl = info[:, 0]
    kept = dict(matches=int(m_h.sum()), kept=n_kept, share_kept=round(n_kept / max(int(m_h.sum()), 1), 5),
                matches_per_pair=dict(mean=round(float(m_h.mean()), 1), min=int(m_h.min()), max=int(m_h.max())),
                kept_beyond_far_px=far_kept, share_of_kept_beyond_far_px=round(far_kept / max(n_kept, 1), 5),
                rejected_beyond_far_px=far_rejected, share_of_rejected_beyond_far_px=round(far_rejected / max(n_rejected, 1), 5),
                pairs=dict(total=int(len(fl)), ok=int((fl == 0).sum()), too_few=int(((fl & ops.VERIFY_TOO_FEW) != 0).sum()),
                           no_model=int(((fl & ops.VERIFY_NO_MODEL) != 0).sum()), weak=int(((fl & ops.VERIFY_WEAK) != 0).sum()),
                           malformed=int(((fl & ops.VERIFY_MALFORMED) != 0).sum())),
                valid_hypotheses=dict(min=int(info[:, 3].min()), mean=round(float(info[:, 3].mean()), 1)))
    summary["matches"] = kept
    print(json.dumps(dict(matches=kept)))

    # ---- the global adjustment, four ways
    runs = []
    for name, kw in (("two_view", {}), ("two_view_verify", dict(verify={})),
                     ("multi_view_cull", dict(triangulation="multi_view", cull=CULL)),
                     ("multi_view_cull_verify", dict(triangulation="multi_view", cull=CULL, verify={}))):
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
                   initial_cost=c0, nfev=int(res.nfev), status=int(res.status), ba_solve_ms=round(timers["ba_solve"], 2),
                   ms_per_evaluation=round(timers["ba_solve"] / max(int(res.nfev), 1), 4), final_cost=float(res.cost))
        runs.append(row)
        print(json.dumps(row))
    summary["global_ba"] = runs
    summary["one_ba_evaluation_ms"] = runs[0]["ms_per_evaluation"]
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(summary, fh, indent=1)


if __name__ == "__main__":
    main()
