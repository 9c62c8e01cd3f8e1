"""The dense stage (ops.depth_sweep, ops.depth_fuse) on the rendered clip of bench.py's shape (C3: 500 frames of
1920 x 1080, 4000 key points), behind `ClipPipeline.run(dense=...)` with downscale 2, 64 planes and 4 sources.

Reported: the stage timers of the run (`dense` beside `detect` per frame, for scale); then, on the cameras and ranges the run
ended with, warm, in HIP-event time per launch (the library's own events): the milliseconds of every kernel of the stage per
view, and the sweep's achieved share of its LDS-read bound -- the n window reads of 4 bytes every pixel makes per plane and
source, at the 128 B per clock and CU that `ds_read_b32` streams, on the device's CUs at --clock-ghz (2.4, the peak bench.py
takes its VALU rate at; a kernel that runs below it is further from the bound by that factor).  None of the numbers is a gate.

usage: python tools/bench_dense.py [--frames 500] [--width 1920] [--height 1080] [--nfeatures 4000] [--every 4] [--gap 2]
                                   [--planes 64] [--sources 4] [--radius 3] [--downscale 2] [--max-nfev N] [--reps 3] [--clock-ghz 2.4]
                                   [--json OUT]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch  # noqa: F401  (before the package: the library binds to the HIP runtime torch has loaded)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from meatmodeler_amd import _lib, synth  # noqa: E402
from meatmodeler_amd._lib import default_context  # noqa: E402
from meatmodeler_amd.bundleAdjuster import _rodrigues_matrix  # noqa: E402
from meatmodeler_amd.pipeline import ClipPipeline, dense_cloud, dense_views  # noqa: E402

LDS_READ_BYTES_PER_CLOCK_PER_CU = 128      # ds_read_b32: 64 lanes x 4 B in 2 LDS cycles


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=500)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--nfeatures", type=int, default=4000)
    ap.add_argument("--every", type=int, default=4)
    ap.add_argument("--gap", type=int, default=2)
    ap.add_argument("--planes", type=int, default=64)
    ap.add_argument("--sources", type=int, default=4)
    ap.add_argument("--radius", type=int, default=3)
    ap.add_argument("--downscale", type=int, default=2)
    ap.add_argument("--max-nfev", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--clock-ghz", type=float, default=2.4)
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
    opts = dict(every=a.every, gap=a.gap, planes=a.planes, sources=a.sources, radius=a.radius, downscale=a.downscale)
    pipe = ClipPipeline(H, W, a.nfeatures, batch=16, device=dev, ctx=ctx)
    timers = {}
    out = pipe.run(frames, K, ext, ba=True, ftol=1e-4, timers=timers, max_nfev=a.max_nfev or None, refine={}, dense=opts)
    dn = out["dense"]
    V = int(dn["views"].size)
    swept = int((dn["flags"] == 0).sum())
    h, w = dn["depth"].shape[1:]
    res = out["refine"]["ba"]
    E = np.stack([np.concatenate([_rodrigues_matrix(c[:3]), c[3:, None]], axis=1) for c in res.cams.reshape(F, 6).cpu().numpy()])
    ranges = np.full((F, 2), np.nan)
    ranges[dn["views"]] = dn["range"]

    def stage():
        return dense_cloud(frames, K, E, ranges, ctx=ctx, **opts)

    stage()
    ctx.sync()
    per_kernel = {}
    for _ in range(a.reps):
        ctx.profile(1)
        stage()
        ctx.sync()
        for name, (_, ms) in ctx.profile_report().items():
            if name.startswith(("ds_", "df_")):
                per_kernel.setdefault(name, []).append(ms)
        ctx.profile(0)
    kernels = {k: round(float(np.median(v)), 4) for k, v in per_kernel.items()}
    # the sweep's LDS-read bound: every pixel with a window reads its n samples once per plane and source that exists
    _, src, _ = dense_views(F, a.every, a.sources, a.gap, 0)
    slots = int((src[dn["flags"] == 0] >= 0).sum())
    n = (2 * a.radius + 1) ** 2
    interior = max(w - 2 * a.radius, 0) * max(h - 2 * a.radius, 0)
    lds_bytes = interior * slots * a.planes * n * 4
    cus = ctx.control(_lib.Context.CTL_CU_COUNT)
    clock_hz = a.clock_ghz * 1e9
    bound_ms = lds_bytes / (cus * LDS_READ_BYTES_PER_CLOCK_PER_CU * clock_hz) * 1e3
    sweep_ms = kernels.get("ds_sweep_kernel", float("nan"))
    summary = dict(frames=F, width=W, height=H, nfeatures=a.nfeatures, options=opts, views=V, views_swept=swept, map_size=[int(h), int(w)],
                   points=int(dn["counts"][0]), candidates=int(dn["counts"][1]), tracks=int(out["n_tracks"]),
                   run_timers_ms={k: round(v, 2) for k, v in timers.items()},
                   detect_ms_per_frame=round(timers["detect"] / F, 4), dense_ms_per_view=round(timers["dense"] / max(V, 1), 4),
                   kernels_ms=kernels, kernels_ms_per_view={k: round(v / max(swept, 1), 4) for k, v in kernels.items()},
                   sweep_lds_read_bytes=int(lds_bytes), compute_units=int(cus), clock_mhz=round(clock_hz / 1e6, 1),
                   sweep_lds_read_bound_ms=round(bound_ms, 4), sweep_share_of_lds_read_bound=round(bound_ms / sweep_ms, 4))
    print(json.dumps(summary))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(summary, fh, indent=1)


if __name__ == "__main__":
    main()
