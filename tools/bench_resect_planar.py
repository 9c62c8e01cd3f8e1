"""Planar resection (mm_resect_planar) on the rendered clip of tools/bench_resect.py (200 x 1080p, 4000 key points per frame)
with its scene flattened: the triangulated points of the clip are projected onto one plane -- parallel to the plane of the
camera centres, 0.35 orbit radii off it, so every camera sees it about 19 degrees above grazing -- and every observation is the
projection of its flattened point through the recovered pose of its frame plus 0.3 px of noise; one observation in ten keeps the
clip's own pixel and is an outlier.  Rows per camera, tracks and the index arrays are the clip's (about 3200 rows per camera).

Reported: the planar stage (the four kernels of one call, defaults, no prior) warm, in HIP-event time (median and minimum of
--reps), beside `resect` (mm_resect_cameras on the clip as it is, with the prior, as tools/bench_resect.py measures it), `verify`
and `poses` measured the same way in the same process; the kernels of one planar call alone; the flag histogram, inliers per
camera, and the worst rotation and camera-centre error against the poses the observations were made with.

usage: python tools/bench_resect_planar.py [--frames 200] [--width 1920] [--height 1080] [--nfeatures 4000] [--reps 20]
                                           [--json profiles/resect_planar_200.json]
Run it under a time limit (timeout -k 10 600 python tools/bench_resect_planar.py ...).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_poses import centres, event_ms  # noqa: E402
from meatmodeler_amd import ops, synth  # noqa: E402
from meatmodeler_amd._lib import default_context  # noqa: E402
from meatmodeler_amd.pipeline import ClipPipeline  # noqa: E402


def flatten_scene(K, X, coords, fi, pi, ext, seed=3, noise=0.3, outlier_every=10):
    """-> (X on the plane [T, 3], observations [O, 2], outlier mask [O]) as NumPy arrays (see the module docstring)."""
    rng = np.random.default_rng(seed)
    C = centres(ext)
    ok = np.isfinite(X).all(axis=1)
    p0 = X[ok].mean(axis=0)
    _, _, Vt = np.linalg.svd(C - C.mean(axis=0))
    n = Vt[2]
    radius = float(np.linalg.norm(C - p0, axis=1).mean())
    if (C.mean(axis=0) - p0) @ n > 0:
        n = -n
    q = p0 + 0.35 * radius * n
    Xp = X - ((X - q) @ n)[:, None] * n[None, :]
    Y = np.einsum("oij,oj->oi", ext[fi][:, :, :3], Xp[pi]) + ext[fi][:, :, 3]
    px = Y @ np.asarray(K, float).reshape(3, 3).T
    obs = px[:, :2] / px[:, 2:3] + noise * rng.standard_normal((len(fi), 2))
    out = (np.arange(len(fi)) % outlier_every) == 0
    obs[out] = coords[out]
    return Xp, obs, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--nfeatures", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    ctx = default_context()
    dev = ctx.device
    F, W, H = a.frames, a.width, a.height
    K = synth.default_K(W, H, f=525.0 * W / 640.0)
    frames, _, _ = synth.render_orbit_frames_torch(F, W, H, dev, arc_deg=min(360.0, 0.72 * F), seed=7, K=K)
    pipe = ClipPipeline(H, W, a.nfeatures, batch=16, device=dev, ctx=ctx)
    summary = dict(frames=F, width=W, height=H, nfeatures=a.nfeatures, reps=a.reps)

    base = pipe.run(frames, K, None, ba=False, verify={}, poses={})
    det = base["det"]
    pairs, m = pipe.match(det)
    pairs_v, m_v, F_v, _, _ = pipe.verify(det, pairs, m)
    prior = base["poses"]["extrinsics"]
    tracks = (base["track_ptr_dev"], base["obs_frame_dev"], base["obs_kp_dev"], base["xy_dev"])
    X = base["points0"]
    coords, fi, pi = ops.flatten_tracks(*tracks, ctx=ctx)
    fl = fi.long()
    cam_obs = torch.argsort(fl, stable=True).to(torch.int32)
    cam_ptr = torch.zeros(F + 1, dtype=torch.int32, device=dev)
    cam_ptr[1:] = torch.cumsum(torch.bincount(fl, minlength=F)[:F], 0).to(torch.int32)
    pr = prior.reshape(F, 12).contiguous()
    ext_true = prior.cpu().numpy().reshape(F, 3, 4)
    Xp, obs_p, outl = flatten_scene(K, X.cpu().numpy(), coords.cpu().numpy(), fl.cpu().numpy(), pi.long().cpu().numpy(), ext_true)
    Xp_d, obs_d = torch.as_tensor(Xp).to(dev).contiguous(), torch.as_tensor(obs_p).to(dev).contiguous()

    def planar():
        return ops.resect_planar(K, Xp_d, obs_d, pi, cam_ptr, cam_obs, ctx=ctx)

    def general():
        return ops.resect_cameras(K, X, coords, pi, cam_ptr, cam_obs, prior=pr, ctx=ctx)

    stage = dict(verify=event_ms(ctx, lambda: pipe.verify(det, pairs, m), a.reps),
                 poses=event_ms(ctx, lambda: pipe.recover_poses(det, pairs_v, m_v, F_v, K), a.reps),
                 resect=event_ms(ctx, general, a.reps),
                 resect_planar=event_ms(ctx, planar, a.reps),
                 resect_auto=event_ms(ctx, lambda: ops.resect_cameras(K, Xp_d, obs_d, pi, cam_ptr, cam_obs, prior=pr, planar="auto",
                                                                      ctx=ctx), a.reps))
    kernels = {}
    for name, fn in (("resect_planar", planar), ("resect", general)):
        ctx.profile(1)
        out = fn()
        ctx.sync()
        kernels[name] = {k: round(v[1], 4) for k, v in ctx.profile_report().items()}
        ctx.profile(0)
        if name == "resect_planar":
            ext_r, cost_r, inl_r, info_r, plane_r = out
    summary["stage_ms_median_min"] = stage
    summary["kernel_ms"] = kernels
    print(json.dumps(dict(stage_ms_median_min=stage, kernel_ms=kernels)))

    info = info_r.cpu().numpy()
    fl_ = info[:, 0]
    E = ext_r.cpu().numpy()
    rot, cen = [], []
    radius = float(np.linalg.norm(centres(ext_true) - Xp[np.isfinite(Xp).all(axis=1)].mean(axis=0), axis=1).mean())
    for f in range(F):
        if not np.isfinite(E[f]).all():
            continue
        c = (np.trace(E[f][:, :3] @ ext_true[f][:, :3].T) - 1.0) / 2.0
        rot.append(float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0)))))
        cen.append(float(np.linalg.norm(centres(E[f:f + 1]) - centres(ext_true[f:f + 1])) / radius))
    inl = inl_r.cpu().numpy().astype(bool)
    pl = plane_r.cpu().numpy()
    cams = dict(cameras=int(F), observations=int(coords.shape[0]), tracks=int(X.shape[0]), outlier_observations=int(outl.sum()),
                usable_rows=dict(mean=round(float(info[:, 4].mean()), 1), min=int(info[:, 4].min()), max=int(info[:, 4].max())),
                inliers=dict(mean=round(float(info[:, 1].mean()), 1), min=int(info[:, 1].min()), max=int(info[:, 1].max())),
                valid_hypotheses=dict(mean=round(float(info[:, 3].mean()), 1), min=int(info[:, 3].min())),
                flags=dict(planar=int(((fl_ & ops.RESECT_PLANAR) != 0).sum()), refused=int(((fl_ & ops.RESECT_PLANAR) == 0).sum()),
                           too_few=int(((fl_ & ops.RESECT_TOO_FEW) != 0).sum()), no_model=int(((fl_ & ops.RESECT_NO_MODEL) != 0).sum()),
                           weak=int(((fl_ & ops.RESECT_WEAK) != 0).sum()), malformed=int(((fl_ & ops.RESECT_MALFORMED) != 0).sum())),
                polished=int((info[:, 5] > 0).sum()), outliers_kept=int((inl & outl).sum()),
                thickness_max=float(np.nanmax(pl[:, 4])), aspect_min=float(np.nanmin(pl[:, 5])),
                worst_rotation_error_deg=max(rot) if rot else None, worst_centre_error_over_radius=max(cen) if cen else None)
    summary["resect_planar"] = cams
    print(json.dumps(dict(resect_planar=cams)))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(summary, fh, indent=1)


if __name__ == "__main__":
    main()
