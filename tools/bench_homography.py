"""The homography stage (ClipPipeline.run(degeneracy=...)) on a rendered clip.

clip = orbit: the clip of tools/bench_poses.py (200 x 1080p on an orbit, 4000 key points per frame): every pair is general.
clip = pan:   the same scene seen by a camera that stays where it is and turns about its y axis (synth.render_frame, numpy on
              the host, hence fewer frames by default): every pair is a pure rotation.

Reported per clip: the `degeneracy` stage (mm_verify_homography, and mm_recover_poses_homography on its output) warm, in
HIP-event time (median and minimum of --reps, one session) beside `verify` and `poses` measured the same way; the kernels of
one call alone; the verdict counts; the distributions of n_H / n_F and of sqrt(l1 / l3) - 1.

usage: python tools/bench_homography.py {orbit,pan} [--frames N] [--width 1920] [--height 1080] [--nfeatures 4000] [--reps 20]
                                        [--pan-deg 0.6] [--json OUT]
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


def quantiles(v):
    v = np.asarray(v, float)
    v = v[np.isfinite(v)]
    if v.size == 0:
        return None
    q = np.quantile(v, [0.0, 0.05, 0.5, 0.95, 1.0])
    return dict(n=int(v.size), min=float(q[0]), p05=float(q[1]), median=float(q[2]), p95=float(q[3]), max=float(q[4]))


def render_pan(n_frames, width, height, K, step_deg, device):
    """A camera on the orbit's first position that turns by step_deg per frame about its own y axis."""
    tex = synth.make_texture(2048, n_shapes=6500, seed=7)
    e0 = synth.orbit_cameras(2, arc_deg=1.0, radius=7.0, height=-2.0)[0]
    ext = []
    for i in range(n_frames):
        a = math.radians(step_deg * (i - (n_frames - 1) / 2.0))
        P = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
        ext.append(P @ e0)
    frames = np.stack([synth.render_frame(tex, e, K, width, height) for e in ext])
    return torch.as_tensor(frames).to(device), np.array(ext)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("clip", choices=("orbit", "pan"))
    ap.add_argument("--frames", type=int, default=0, help="default: 200 (orbit), 24 (pan)")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--nfeatures", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pan-deg", type=float, default=0.6, help="turn per frame of the pan clip")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    ctx = default_context()
    dev = ctx.device
    F, W, H = a.frames or (200 if a.clip == "orbit" else 24), a.width, a.height
    K = synth.default_K(W, H, f=525.0 * W / 640.0)
    if a.clip == "orbit":
        frames, ext_gt, _ = synth.render_orbit_frames_torch(F, W, H, dev, arc_deg=min(360.0, 0.72 * F), seed=7, K=K)
    else:
        frames, ext_gt = render_pan(F, W, H, K, a.pan_deg, dev)
    pipe = ClipPipeline(H, W, a.nfeatures, batch=16, device=dev, ctx=ctx)
    summary = dict(clip=a.clip, frames=F, width=W, height=H, nfeatures=a.nfeatures, reps=a.reps)

    # ---- the stages, warm, HIP events, one session
    det = pipe.detect(frames)
    pairs, m = pipe.match(det)
    pairs_v, m_v, F_v, _, info_v = pipe.verify(det, pairs, m)
    pairs_h, m_h, H_h, _, info_h = pipe.homography(det, pairs, m, verify_info=info_v)

    def hpose():
        return ops.recover_poses_homography(det["xy"], pairs_h, m_h, H_h, K, ctx=ctx)

    def degeneracy():
        ph, mh, Hh, _, _ = pipe.homography(det, pairs, m, verify_info=info_v)
        return ops.recover_poses_homography(det["xy"], ph, mh, Hh, K, ctx=ctx)

    stage = dict(verify=event_ms(ctx, lambda: pipe.verify(det, pairs, m), a.reps),
                 poses=event_ms(ctx, lambda: pipe.recover_poses(det, pairs_v, m_v, F_v, K), a.reps),
                 homography=event_ms(ctx, lambda: pipe.homography(det, pairs, m, verify_info=info_v), a.reps),
                 homography_poses=event_ms(ctx, hpose, a.reps),
                 degeneracy=event_ms(ctx, degeneracy, a.reps))
    ctx.profile(1)
    degeneracy()
    ctx.sync()
    kernels = {k: round(v[1], 4) for k, v in ctx.profile_report().items()}
    ctx.profile(0)
    ctx.profile(1)
    pipe.verify(det, pairs, m)
    ctx.sync()
    kernels.update({k: round(v[1], 4) for k, v in ctx.profile_report().items()})
    ctx.profile(0)
    summary["stage_ms_median_min"] = stage
    summary["kernel_ms"] = kernels
    print(json.dumps(dict(stage_ms_median_min=stage, kernel_ms=kernels)))

    # ---- verdicts and the two distributions
    R, t, sigma, normal, depth, pinfo = hpose()
    ih, iv, ip, sg = info_h.cpu().numpy(), info_v.cpu().numpy(), pinfo.cpu().numpy(), sigma.cpu().numpy()
    fl = ih[:, 0]
    ok = (fl & 7) == 0
    deg = (fl & ops.HOMOG_DEGENERATE) != 0
    rot = (ip[:, 0] & ops.HPOSE_ROTATION) != 0
    with np.errstate(all="ignore"):
        ratio = np.where(ok & (ih[:, 4] > 0), ih[:, 1] / np.maximum(ih[:, 4], 1), np.nan)
        spread = sg[:, 0] / sg[:, 2] - 1.0
    verdicts = dict(pairs=int(len(fl)), matches_per_pair=quantiles(m.cpu().numpy()),
                    homography_flags=dict(ok=int(ok.sum()), too_few=int(((fl & ops.HOMOG_TOO_FEW) != 0).sum()),
                                          no_model=int(((fl & ops.HOMOG_NO_MODEL) != 0).sum()),
                                          weak=int(((fl & ops.HOMOG_WEAK) != 0).sum()),
                                          malformed=int(((fl & ops.HOMOG_MALFORMED) != 0).sum())),
                    verify_failed=int(((iv[:, 0] & 7) != 0).sum()),
                    degenerate=int(deg.sum()), degenerate_and_rotation=int((deg & rot).sum()),
                    degenerate_and_planar=int((deg & ~rot & ((ip[:, 0] & 3) == 0)).sum()),
                    planar_ambiguous=int((deg & ~rot & ((ip[:, 0] & ops.POSE_AMBIGUOUS) != 0)).sum()),
                    n_H_over_n_F=quantiles(ratio), n_H=quantiles(ih[:, 1]), n_F=quantiles(iv[:, 1]),
                    sqrt_l1_over_l3_minus_1=quantiles(spread[ok]),
                    sqrt_l1_over_l3_minus_1_of_the_degenerate=quantiles(spread[deg]))
    if a.clip == "pan":      # the turn each pair recovered against the one it was rendered with
        err = []
        for p in np.nonzero(deg & rot)[0]:
            Rt = ext_gt[p + 1][:, :3] @ ext_gt[p][:, :3].T
            D = R[p].cpu().numpy().reshape(3, 3) @ Rt.T
            err.append(math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(D) - 1.0) / 2.0)))))
        verdicts["rotation_error_deg"] = quantiles(err)
    summary["verdicts"] = verdicts
    print(json.dumps(dict(verdicts=verdicts)))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(summary, fh, indent=1)


if __name__ == "__main__":
    main()
