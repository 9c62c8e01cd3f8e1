"""Similarity registration (ops.align_similarity) on the rendered clip of tools/bench_poses.py (200 x 1080p, 4000 key points
per frame).

Two cases, each warm, in HIP-event time (median and minimum of --reps):
  (a) centres: the camera centres of the recovered chain (run(verify={}, poses={})) against the clip's true centres, tau_rel 0.05;
  (b) cloud:   the clip's triangulated cloud against the same cloud under a known similarity with 30 % of the rows displaced.
Beside each: the kernels of one call alone, the host NumPy Umeyama of tools/bench_poses.py on the same rows (wall clock, median
of --reps) and one evaluation of the global adjustment of the same run.  For (a) also the chain against the truth after the
robust alignment and after the plain one; for (b) the recovered similarity against the known one and the mask against the truth.

usage: python tools/bench_align.py [--frames 200] [--width 1920] [--height 1080] [--nfeatures 4000] [--reps 20] [--json OUT]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_poses import centres, event_ms, similarity  # noqa: E402
from meatmodeler_amd import ops, synth  # noqa: E402
from meatmodeler_amd._lib import default_context  # noqa: E402
from meatmodeler_amd.pipeline import ClipPipeline  # noqa: E402


def host_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(ts)), 4), round(float(np.min(ts)), 4)


def measure(ctx, src, dst, reps, **kw):
    """Times and kernels of one align_similarity call on device rows; -> (dict, (sim, cost, inlier, info) on the host)."""
    out = ops.align_similarity(src, dst, ctx=ctx, **kw)
    stage = event_ms(ctx, lambda: ops.align_similarity(src, dst, ctx=ctx, **kw), reps)
    ctx.profile(1)
    ops.align_similarity(src, dst, ctx=ctx, **kw)
    ctx.sync()
    kernels = {k: (v[0], round(v[1], 4)) for k, v in ctx.profile_report().items()}
    ctx.profile(0)
    sh, dh = src.cpu().numpy(), dst.cpu().numpy()
    ok = np.isfinite(sh).all(axis=1) & np.isfinite(dh).all(axis=1)
    numpy_ms = host_ms(lambda: similarity(sh[ok], dh[ok]), reps)
    return dict(rows=int(src.shape[0]), align_ms_median_min=stage, kernels_launches_ms=kernels,
                numpy_umeyama_ms_median_min=numpy_ms), tuple(t.cpu().numpy() for t in out)


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
    frames, ext_gt, _ = synth.render_orbit_frames_torch(F, W, H, dev, arc_deg=min(360.0, 0.72 * F), seed=7, K=K)
    ext_gt = np.asarray(ext_gt, float)[:, :3, :]
    radius = float(np.linalg.norm(centres(ext_gt)[:, [0, 2]], axis=1).mean())
    pipe = ClipPipeline(H, W, a.nfeatures, batch=16, device=dev, ctx=ctx)
    timers = {}
    r = pipe.run(frames, K, None, ba=True, ftol=1e-4, timers=timers, verify={}, poses={})
    summary = dict(frames=F, width=W, height=H, nfeatures=a.nfeatures, reps=a.reps, orbit_radius=radius,
                   one_ba_evaluation_ms=round(timers["ba_solve"] / max(int(r["ba"].nfev), 1), 4), ba_nfev=int(r["ba"].nfev))

    # ---- (a) the recovered chain's centres against the true ones
    ext_rec = r["poses"]["extrinsics"]
    src = ops.camera_centres(ext_rec, ctx=ctx)
    ct = centres(ext_gt)
    dst = torch.as_tensor(np.ascontiguousarray(ct)).to(dev)
    case, (sim, cost, inlier, info) = measure(ctx, src, dst, a.reps, tau_rel=0.05)
    c = src.cpu().numpy()
    s, R, d = sim[0, 0], sim[0, 1:10].reshape(3, 3), sim[0, 10:]
    robust = np.linalg.norm(s * c @ R.T + d - ct, axis=1) / radius
    s2, Q2, d2 = similarity(c, ct)
    plain = np.linalg.norm(s2 * c @ Q2.T + d2 - ct, axis=1) / radius
    case.update(info=info[0].tolist(), scale=float(s), numpy_scale=float(s2),
                centre_error_over_radius=dict(robust_worst=float(robust.max()), robust_worst_inlier=float(robust[inlier == 1].max()),
                                              plain_worst=float(plain.max())))
    summary["centres"] = case
    print(json.dumps(dict(centres=case)))

    # ---- (b) the triangulated cloud against itself under a known similarity, 30 % of the rows displaced
    X = r["points0"]
    X = X[torch.isfinite(X).all(dim=1)].contiguous()
    rng = np.random.default_rng(5)
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    Rt = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                   [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                   [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    st, dt = 2.5, np.array([0.3, -1.2, 4.0])
    Xh = X.cpu().numpy()
    Y = st * Xh @ Rt.T + dt
    spread = float(np.sqrt(((Y - np.median(Y, axis=0)) ** 2).sum(axis=1).mean()))
    med = float(np.median(np.linalg.norm(Y - np.median(Y, axis=0), axis=1)))
    bad = rng.permutation(len(Y))[:int(0.3 * len(Y))]
    v = rng.normal(size=(len(bad), 3))
    Y[bad] += v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (len(bad), 1)) * med
    truth = np.ones(len(Y), bool)
    truth[bad] = False
    case, (sim, cost, inlier, info) = measure(ctx, X, torch.as_tensor(np.ascontiguousarray(Y)).to(dev), a.reps, tau=1e-3 * med)
    case.update(info=info[0].tolist(), rms_spread=spread, median_radius=med, scale_error=float(abs(sim[0, 0] - st) / st),
                rotation_error=float(np.abs(sim[0, 1:10].reshape(3, 3) - Rt).max()), translation_error=float(np.abs(sim[0, 10:] - dt).max()),
                mask_equals_truth=bool(np.array_equal(inlier.astype(bool), truth)))
    summary["cloud"] = case
    print(json.dumps(dict(cloud=case)))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(summary, fh, indent=1)


if __name__ == "__main__":
    main()
