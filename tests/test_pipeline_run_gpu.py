"""`ClipPipeline.run` against what commit e3d6e10 returned on an MI355X, where `run` was one method of 330 lines
(tests/golden/pipeline_run_parent_e3d6e10.json, written there by tools/dev/record_pipeline_run.py -- the same `observe` runs
here): result keys, timer keys, the number of context synchronisations and the digest of every tensor.  That commit gave the
same digests twice for every path of every case, the adjustment included, so every digest is compared."""
import functools
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from meatmodeler_amd import pipeline  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def recorder():
    spec = importlib.util.spec_from_file_location("record_pipeline_run", os.path.join(ROOT, "tools", "dev", "record_pipeline_run.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


@functools.lru_cache(maxsize=None)
def clip():
    return recorder().clip()


@functools.lru_cache(maxsize=None)
def observed(name):
    """(result, observation) of case `name`; D's targets come from the extrinsics case B recovers."""
    frames, ext, K, pipe = clip()
    recovered = observed("B")[0]["poses"]["extrinsics"].cpu().numpy() if name == "D" else None
    extrinsics, options = recorder().cases(ext, recovered)[name]
    return recorder().observe(pipe, frames, K, extrinsics, options)


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_run_is_what_the_parent_returned(name, golden_dir):
    with open(os.path.join(golden_dir, "pipeline_run_parent_e3d6e10.json")) as fh:
        want = json.load(fh)["cases"][name]
    got = observed(name)[1]
    unstable = set(want["unstable"])
    assert not [p for p in unstable if not recorder().after_adjustment(p)]
    print(f"case {name}: {got['syncs']} syncs (golden {want['syncs']}), timers {got['timer_keys']}, {len(got['digests'])} digests, "
          f"{len(unstable)} left out as unstable")
    assert got["keys"] == want["keys"]
    assert got["timer_keys"] == want["timer_keys"]
    assert got["syncs"] == want["syncs"]
    assert sorted(got["digests"]) == sorted(want["digests"])
    always = {p for p in want["digests"] if recorder().after_adjustment(p) and p.rsplit(".", 1)[-1] in ("nfev", "status")}
    differ = [p for p in want["digests"] if (p not in unstable or p in always) and got["digests"][p] != want["digests"][p]]
    assert not differ, differ


def test_a_rank_without_frames_gets_zero_rows_of_everything():
    """The second of two ranks on a two-frame clip owns no pair: det is None and every table has its shape with no rows."""
    _, _, _, pipe = clip()
    plan = pipeline.run_plan(2, 2, verify={}, degeneracy={}, guided={})
    ms = {}
    front = pipe._front(torch.zeros((2, 480, 640), dtype=torch.uint8, device=pipe.device), plan, 1, pipeline.StageClock(pipe.ctx, ms))
    cap, f64, i32 = pipe.cap, torch.float64, torch.int32
    assert front.det is None and front.is_deg is None and (front.pairs_local, front.frames_local) == (0, 0)
    assert sorted(ms) == ["degeneracy", "detect", "guided", "match", "verify"]
    assert sorted(front.verify) == ["F", "cost", "info", "matches_in"] and front.verify["matches_in"] is front.m
    assert sorted(front.degeneracy) == ["H", "cost", "info"] and sorted(front.guided) == ["info", "is_new"]
    want = [(front.pairs, (0, cap, 2), i32), (front.m, (0,), i32),
            (front.verify["F"], (0, 9), f64), (front.verify["cost"], (0,), f64), (front.verify["info"], (0, 4), i32),
            (front.degeneracy["H"], (0, 9), f64), (front.degeneracy["cost"], (0,), f64), (front.degeneracy["info"], (0, 6), i32),
            (front.guided["is_new"], (0, cap), torch.uint8), (front.guided["info"], (0, 4), i32),
            (front.xy, (0, cap, 2), torch.float32), (front.n, (0,), i32)]
    for k, (t, shape, dtype) in enumerate(want):
        assert tuple(t.shape) == shape and t.dtype == dtype and t.device == pipe.device, k
    off = pipe._front(None, pipeline.run_plan(2, 2), 1, pipeline.StageClock(pipe.ctx, {}))
    assert off.verify is None and off.degeneracy is None and off.guided is None and tuple(off.pairs.shape) == (0, cap, 2)
