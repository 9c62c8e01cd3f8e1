"""Pose recovery (ClipPipeline.run(poses=...)) on the rendered clip of tools/bench_verify.py (200 x 1080p, 4000 key points
per frame).

Reported: the `poses` stage (mm_recover_poses + mm_chain_poses) warm, in HIP-event time (median and minimum of --reps), beside
the `verify` stage measured the same way and the time of one evaluation of the global adjustment of the same run; the kernels
of one call alone; the flag histograms; the recovered chain against the clip's TRUE extrinsics after a similarity alignment of
the camera centres (worst rotation error in degrees, worst camera-centre error as a fraction of the orbit radius); and the
global bundle adjustment with verification on, started from the recovered poses and from the true ones: initial cost,
evaluations, final cost, and the adjusted cameras against the truth after the same alignment.

usage: python tools/bench_poses.py [--frames 200] [--width 1920] [--height 1080] [--nfeatures 4000] [--reps 20]
                                   [--max-nfev N] [--json OUT]
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


def centres(ext):
    return np.array([-e[:, :3].T @ e[:, 3] for e in ext])


def similarity(src, dst):
    """(s, Q, d) of the least-squares dst ~ s Q src + d (Umeyama)."""
    ms, md = src.mean(axis=0), dst.mean(axis=0)
    a, b = src - ms, dst - md
    U, S, Vt = np.linalg.svd(b.T @ a / len(src))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    Q = U @ D @ Vt
    s = (S * np.diag(D)).sum() / (a * a).sum() * len(src)
    return s, Q, md - s * Q @ ms


def chain_error(ext, ext_true, radius):
    """Worst rotation error [deg] and worst camera-centre error / radius after aligning the recovered centres to the true ones."""
    c, ct = centres(ext), centres(ext_true)
    s, Q, d = similarity(c, ct)
    centre = np.linalg.norm(s * c @ Q.T + d - ct, axis=1).max() / radius
    rot = 0.0
    for e, et in zip(ext, ext_true):
        R = e[:, :3] @ Q.T @ et[:, :3].T
        rot = max(rot, math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(R) - 1.0) / 2.0)))))
    return rot, centre, s


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

    # ---- the stages, warm, HIP events
    det = pipe.detect(frames)
    pairs, m = pipe.match(det)
    pairs_v, m_v, F_v, _, info_v = pipe.verify(det, pairs, m)
    stage = dict(verify=event_ms(ctx, lambda: pipe.verify(det, pairs, m), a.reps),
                 poses=event_ms(ctx, lambda: pipe.recover_poses(det, pairs_v, m_v, F_v, K), a.reps))
    ctx.profile(1)
    po = pipe.recover_poses(det, pairs_v, m_v, F_v, K)
    ctx.sync()
    kernels = {k: round(v[1], 4) for k, v in ctx.profile_report().items()}
    ctx.profile(0)
    summary["stage_ms_median_min"] = stage
    summary["poses_kernel_ms"] = kernels
    print(json.dumps(dict(stage_ms_median_min=stage, poses_kernel_ms=kernels)))

    # ---- flags, votes, the chain against the truth
    info, cinfo, sigma, scale = (po[k].cpu().numpy() for k in ("info", "chain_info", "sigma", "scale"))
    m_h = m_v.cpu().numpy()
    fl, cf = info[:, 0], cinfo[:, 0]
    win = np.take_along_axis(info[:, 2:6], np.maximum(info[:, 1:2], 0), axis=1)[:, 0]
    ext_rec = po["extrinsics"].cpu().numpy()
    rot_deg, centre_frac, sim_scale = chain_error(ext_rec, ext_gt, radius)
    chain = dict(pairs=int(len(fl)), matches_per_pair=dict(mean=round(float(m_h.mean()), 1), min=int(m_h.min()), max=int(m_h.max())),
                 pose_flags=dict(ok=int((fl == 0).sum()), too_few=int(((fl & ops.POSE_TOO_FEW) != 0).sum()),
                                 no_model=int(((fl & ops.POSE_NO_MODEL) != 0).sum()),
                                 ambiguous=int(((fl & ops.POSE_AMBIGUOUS) != 0).sum()),
                                 malformed=int(((fl & ops.POSE_MALFORMED) != 0).sum())),
                 chain_flags=dict(ok=int((cf == 0).sum()), few_common=int(((cf & ops.CHAIN_FEW_COMMON) != 0).sum()),
                                  broken=int(((cf & ops.CHAIN_BROKEN) != 0).sum())),
                 front_share=dict(min=round(float((win / np.maximum(info[:, 6], 1)).min()), 4),
                                  mean=round(float((win / np.maximum(info[:, 6], 1)).mean()), 4)),
                 sigma_ratio_minus_1=dict(max=float(np.nanmax(np.abs(sigma[:, 0] / sigma[:, 1] - 1.0)))),
                 n_common=dict(min=int(cinfo[1:, 1].min()) if len(cf) > 1 else 0, mean=round(float(cinfo[1:, 1].mean()), 1) if len(cf) > 1 else 0),
                 scale=dict(min=float(scale.min()), max=float(scale.max()), last=float(scale[-1])),
                 worst_rotation_error_deg=rot_deg, worst_centre_error_over_radius=centre_frac, similarity_scale=float(sim_scale))
    summary["chain"] = chain
    print(json.dumps(dict(chain=chain)))

    # ---- the global adjustment with verification on, from the recovered and from the true poses
    runs = []
    for name, kw in (("true_poses", dict(extrinsics=ext_gt)), ("recovered_poses", dict(extrinsics=None, poses={}))):
        timers = {}
        r = pipe.run(frames, K, ba=True, ftol=1e-4, timers=timers, max_nfev=a.max_nfev or None, verify={}, **kw)
        res = r["ba"]
        ext0 = ext_gt if "poses" not in r else r["poses"]["extrinsics"].cpu().numpy()
        coords, fi, pi = ops.flatten_tracks(r["track_ptr_dev"], r["obs_frame_dev"], r["obs_kp_dev"], r["xy_dev"], ctx=ctx)
        pb = ops.BADevice(K, fi, pi, coords, F, int(r["points0"].shape[0]), dev, ctx, pairs=False)
        with np.errstate(all="ignore"):
            cams0 = torch.as_tensor(frameParameters(ext0).reshape(F, 6)).to(dev)
        c0 = 0.5 * float(pb.residual(cams0.contiguous(), r["points0"].contiguous())[0].item())
        row = dict(run=name, tracks=int(r["n_tracks"]), observations=int(r["n_obs_local"]),
                   verify_ms_host_clock=round(timers["verify"], 3), poses_ms_host_clock=round(timers.get("poses", 0.0), 3),
                   initial_cost=c0, nfev=int(res.nfev), status=int(res.status), ba_solve_ms=round(timers["ba_solve"], 2),
                   ms_per_evaluation=round(timers["ba_solve"] / max(int(res.nfev), 1), 4), final_cost=float(res.cost))
        # the adjusted cameras against the truth, aligned the same way (the adjustment has no gauge: both runs drift)
        cams = res.cams.cpu().numpy().reshape(F, 6)
        ext1 = np.array([np.c_[synth.rodrigues(c[:3]), c[3:]] for c in cams])
        rot1, cen1, _ = chain_error(ext1, ext_gt, radius)
        row.update(adjusted_worst_rotation_error_deg=rot1, adjusted_worst_centre_error_over_radius=cen1)
        runs.append(row)
        print(json.dumps(row))
    summary["global_ba"] = runs
    summary["one_ba_evaluation_ms"] = runs[0]["ms_per_evaluation"]
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(summary, fh, indent=1)


if __name__ == "__main__":
    main()
