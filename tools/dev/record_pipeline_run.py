#!/usr/bin/env python3
"""What `ClipPipeline.run` returns on the 6-frame clip the stage tests share, reduced to what a refactor of `run` must keep:

    python tools/dev/record_pipeline_run.py OUT.json [COMMIT]

For each case of `cases()` the file holds the sorted key set of the result and of every dict (and adjustment result) inside
it, the sorted keys of `timers`, the number of `ctx.sync()` calls `run` made, and a SHA-256 of dtype, shape and bytes of every
tensor and array in the result (scalars are kept as their repr).  Every case runs twice; a path whose digest differs between
the two runs is listed under "unstable" and is not compared.  Nothing before the adjustment may be unstable (every key but
`ba`, `refine`, `ba_aligned`): the script exits with an error if something is.

Only the public `ClipPipeline.run` is used, so the script runs unchanged beside any commit's tree.  The file recorded at the
parent of the refactor is tests/golden/pipeline_run_parent_e3d6e10.json; tests/test_pipeline_run_gpu.py recomputes it through
`observe` below and compares.
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

AFTER_ADJUSTMENT = ("ba", "refine", "ba_aligned")      # the only keys whose tensors may differ between two runs
BA_FIELDS = ("cams", "pts", "cost", "nfev", "status")  # what is digested of an adjustment result (the rest is timings)
# the similarity case D's targets are moved by: x -> S_SCALE * S_ROT x + S_SHIFT (30 degrees about z)
S_SCALE = 2.5
S_ROT = np.array([[np.sqrt(0.75), -0.5, 0.0], [0.5, np.sqrt(0.75), 0.0], [0.0, 0.0, 1.0]])
S_SHIFT = np.array([1.0, -2.0, 0.5])


def clip():
    """-> (frames [6,480,640] u8 on the device, extrinsics [6,3,4], K, pipeline)."""
    import torch
    from meatmodeler_amd import synth
    from meatmodeler_amd.pipeline import ClipPipeline
    frames, ext, K = synth.render_orbit_frames(6, 640, 480, arc_deg=6.0)
    return torch.as_tensor(frames).to("cuda"), ext, K, ClipPipeline(480, 640, 600, batch=6)


def cases(ext, recovered):
    """name -> (extrinsics, options of run).  `recovered` [6,3,4]: the extrinsics case B recovers (None: only A, B, C)."""
    out = dict(A=(ext, dict(ba=True, max_nfev=8)),
               B=(None, dict(verify={}, poses={}, ba=False)),
               C=(ext, dict(triangulation="multi_view", cull=dict(max_reproj_px=4.0), max_nfev=4)))
    if recovered is not None:
        E = np.asarray(recovered, np.float64)
        centres = -np.einsum("nji,nj->ni", E[:, :3, :3], E[:, :3, 3])
        out["D"] = (None, dict(verify={}, degeneracy={}, guided={}, poses={},
                               align=dict(frames=list(range(6)), centres=S_SCALE * centres @ S_ROT.T + S_SHIFT, n_hyp=64, seed=3),
                               triangulation="multi_view", cull=dict(max_reproj_px=4.0), resect=dict(planar="auto"), refine={},
                               max_nfev=8))
    return out


def _walk(value, path, keys, digests):
    import torch
    if isinstance(value, dict):
        keys[path] = sorted(value)
        for k in keys[path]:
            _walk(value[k], f"{path}.{k}" if path else k, keys, digests)
    elif isinstance(value, (list, tuple)):
        keys[path] = len(value)
        for i, v in enumerate(value):
            _walk(v, f"{path}[{i}]", keys, digests)
    elif isinstance(value, (torch.Tensor, np.ndarray)):
        a = value.detach().cpu().contiguous().numpy() if isinstance(value, torch.Tensor) else np.ascontiguousarray(value)
        digests[path] = hashlib.sha256(f"{a.dtype}{a.shape}".encode() + a.tobytes()).hexdigest()
    elif value is None or isinstance(value, (bool, int, float, str, np.generic)):
        digests[path] = "value:" + repr(value.item() if isinstance(value, np.generic) else value)
    elif not hasattr(value, "cams"):
        digests[path] = "object:" + type(value).__name__
    else:                                                     # an adjustment result
        keys[path] = sorted(vars(value))
        for k in BA_FIELDS:
            _walk(getattr(value, k), f"{path}.{k}", keys, digests)


def observe(pipe, frames, K, extrinsics, options):
    """One `run` -> (result, dict(keys, timer_keys, syncs, digests))."""
    timers, calls, sync = {}, [0], pipe.ctx.sync

    def counted():
        calls[0] += 1
        sync()

    pipe.ctx.sync = counted
    try:
        out = pipe.run(frames, K, extrinsics, timers=timers, **options)
    finally:
        del pipe.ctx.sync
    keys, digests = {}, {}
    _walk(out, "", keys, digests)
    return out, dict(keys=keys, timer_keys=sorted(timers), syncs=calls[0], digests=digests)


def after_adjustment(path):
    return path.split(".")[0].split("[")[0] in AFTER_ADJUSTMENT


def main():
    out_path, commit = sys.argv[1], (sys.argv[2] if len(sys.argv) > 2 else None)
    frames, ext, K, pipe = clip()
    recorded, recovered, bad = {}, None, []
    for name in "ABCD":
        extrinsics, options = cases(ext, recovered)[name]
        out, first = observe(pipe, frames, K, extrinsics, options)
        _, second = observe(pipe, frames, K, extrinsics, options)
        if name == "B":
            recovered = out["poses"]["extrinsics"].cpu().numpy()
        for k in ("keys", "timer_keys", "syncs"):
            if first[k] != second[k]:
                bad.append(f"{name}: {k} differ between two runs")
        first["unstable"] = sorted(p for p in first["digests"] if first["digests"][p] != second["digests"].get(p))
        bad += [f"{name}: {p} is unstable before the adjustment" for p in first["unstable"] if not after_adjustment(p)]
        recorded[name] = first
        print(f"case {name}: {len(first['digests'])} digests, {first['syncs']} syncs, timers {first['timer_keys']}, "
              f"unstable {first['unstable']}", flush=True)
    with open(out_path, "w") as fh:
        json.dump(dict(commit=commit, clip="synth.render_orbit_frames(6, 640, 480, arc_deg=6.0); ClipPipeline(480, 640, 600, batch=6)",
                       cases=recorded), fh, indent=1, sort_keys=True)
        fh.write("\n")
    if bad:
        raise SystemExit("\n".join(bad))


if __name__ == "__main__":
    main()
