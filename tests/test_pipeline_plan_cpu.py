"""`pipeline.run_plan`, the rules `ClipPipeline.run` judges its options by, and `pipeline.StageClock`, its stage timers --
both without a device.  The messages and, where a call breaks two rules, the rule that is reported are those of commit e3d6e10,
where the checks stood inside `run` (taken from that commit's `run` on an object made with `__new__`)."""
import numpy as np
import pytest

from meatmodeler_amd import pipeline
from meatmodeler_amd.pipeline import run_plan

F = 6
ALIGN = dict(frames=[0, 2, 4], centres=np.zeros((3, 3)))
MV = dict(triangulation="multi_view")
CULL = dict(cull=dict(max_reproj_px=4.0), **MV)

# one row per rule: (options beside n_frames = 6, message fragment)
RULES = [
    (dict(verify=dict(threshold=2.0)), "verify takes n_hyp"),
    (dict(verify={}, poses=dict(nope=1)), "poses takes min_matches"),
    (dict(resect=[("n_hyp", 8)]), "resect must be None or a dict of n_hyp"),
    (dict(verify={}, degeneracy=dict(on_fail="drop")), "degeneracy takes n_hyp"),
    (dict(verify={}, guided=dict(radius=3)), "guided takes threshold_px"),
    (dict(align=dict(frames=[0, 1, 2])), "align needs frames and exactly one of extrinsics and centres"),
    (dict(refine=dict(rounds=0)), "refine: rounds must be an integer of at least 1"),
    (dict(guided={}), "guided needs verify (it supplies each pair's fundamental matrix, the model the search is gated by)"),
    (dict(degeneracy={}), "degeneracy needs verify (the verdict compares the homography"),
    (dict(poses={}), "poses needs verify (it supplies each pair's fundamental matrix): pass verify={} for the defaults"),
    (dict(has_extrinsics=False), "extrinsics is required unless poses is set"),
    (dict(triangulation="three_view"), "triangulation must be 'two_view' or 'multi_view'"),
    (dict(align=dict(ALIGN, frames=[0, 2, 6])), "align: frames must be at least 3 distinct indices in [0, F)"),
    (dict(cull=dict(max_reproj_px=4.0)), "cull needs triangulation='multi_view' (the two-view path has no per-track verdict)"),
    (dict(world=2, **CULL), "cull is not supported with more than one rank: the track partition takes contiguous ranges"),
    (dict(world=2, verify={}, poses={}), "poses is not supported with more than one rank: the chain needs the neighbouring"),
    (dict(world=2, resect={}), "resect is not supported with more than one rank: every frame needs the whole point table"),
    (dict(world=2, align=ALIGN), "align is not supported with more than one rank: the cameras of `frames` live on different"),
    (dict(world=2, refine={}), "refine is not supported with more than one rank: the compaction renumbers the points"),
    (dict(cull=dict(refine_iters=4), **MV), "cull takes max_reproj_px, min_angle_deg, min_depth (at least one) and refine_iters"),
    (dict(cull=dict(max_reproj_px=4.0, max_px=4.0), **MV), "and refine_iters; not ['max_px']"),
]

# calls that break two rules: the one reported
FIRST_OF_TWO = [
    # a stage's own keys before any rule across stages, in the order verify, poses, resect, degeneracy, guided, align, refine
    (dict(verify=dict(threshold=2.0), guided={}, has_extrinsics=False), "verify takes"),
    (dict(resect=dict(nope=1), degeneracy=dict(nope=1)), "resect takes"),
    (dict(guided={}, degeneracy={}, poses={}), "guided needs verify"),
    (dict(degeneracy={}, poses={}), "degeneracy needs verify"),
    (dict(poses={}, has_extrinsics=False, triangulation="x"), "poses needs verify"),
    (dict(has_extrinsics=False, triangulation="x"), "extrinsics is required"),
    (dict(triangulation="x", cull={}), "triangulation must be"),
    (dict(align=dict(ALIGN, frames=[0, 2, 6]), cull=dict(max_reproj_px=4.0)), "align: frames must be"),   # the frame range before cull ...
    (dict(align=dict(ALIGN, frames=[0, 2, 6]), world=2), "align: frames must be"),                        # ... and before the world size
    (dict(cull=dict(nope=1), world=2), "cull needs triangulation='multi_view'"),
    (dict(world=2, verify={}, poses={}, **CULL), "cull is not supported"),
    (dict(world=2, verify={}, poses={}, resect={}, refine={}), "poses is not supported"),
    (dict(world=2, resect={}, align=ALIGN), "resect is not supported"),
    (dict(world=2, align=ALIGN, refine={}), "align is not supported"),
    (dict(world=2, refine={}, cull=dict(nope=1), **MV), "cull is not supported"),         # the world size before cull's own keys
    (dict(world=2, resect={}, cull=dict(nope=1), **MV), "cull is not supported"),
]


@pytest.mark.parametrize("options, message", RULES + FIRST_OF_TWO)
def test_a_broken_rule_is_reported_as_before(options, message):
    with pytest.raises(ValueError) as e:
        run_plan(F, **options)
    assert message in str(e.value)


def test_the_option_rules_come_before_the_frame_count_and_the_world_size():
    """`run` hands both over as functions: a call whose options are wrong never reads its frames or its process group."""
    def never():
        raise AssertionError("read before the option rules had passed")

    for options, message in RULES[:12]:
        with pytest.raises(ValueError) as e:
            run_plan(never, **dict(options, world=never))
        assert message in str(e.value)
    order = []
    plan = run_plan(lambda: order.append("frames") or 4, lambda: order.append("world") or 2)
    assert order == ["frames", "world"] and (plan.n_frames, plan.world, plan.sharded) == (4, 2, True)


def test_accepted_calls_give_the_normalised_options():
    plan = run_plan(F)
    assert plan == pipeline.RunPlan(n_frames=F, world=1, sharded=False, force_collectives=False, triangulation="two_view", cull=None,
                                    verify=None, poses=None, resect=None, degeneracy=None, guided=None, align=None, refine=None)
    with pytest.raises(AttributeError):
        plan.world = 2
    given = dict(verify=dict(n_hyp=64), poses=dict(min_common=4), resect=dict(planar="auto"), degeneracy={}, guided=dict(ratio=0.8))
    plan = run_plan(F, None, False, refine={}, align=dict(ALIGN, n_hyp=32), **given, **CULL)
    for name, value in given.items():
        assert getattr(plan, name) == value and getattr(plan, name) is not value          # (a copy: the caller's dict stays its own)
    assert plan.triangulation == "multi_view" and plan.cull == dict(max_reproj_px=4.0)
    assert plan.align["frames"].tolist() == [0, 2, 4] and plan.align["frames"].dtype == np.int64
    assert plan.align["centres"].shape == (3, 3) and plan.align["params"] == dict(n_hyp=32, tau_rel=0.05)
    assert plan.refine == pipeline.refine_options({}) and plan.refine["rounds"] == 2
    assert run_plan(F, align=dict(ALIGN, frames=[0, 2, 5])).align["frames"].max() == F - 1


@pytest.mark.parametrize("world, force, ranks, sharded", [(None, False, 1, False), (None, True, 1, False), (1, False, 1, False),
                                                          (1, True, 1, True), (2, False, 2, True), (2, True, 2, True)])
def test_sharded(world, force, ranks, sharded):
    """The gather / all-reduce path: more than one rank, or a one-rank group with force_collectives; never without a group."""
    plan = run_plan(F, world, force_collectives=force)
    assert (plan.world, plan.sharded, plan.force_collectives) == (ranks, sharded, force)


def test_run_plan_calls_nothing_in_the_shared_library(monkeypatch):
    """(The package loads the library when it is imported, so the check is that judging the options never calls into it, makes
    no context and no tensor.)"""
    import torch
    from meatmodeler_amd import _lib, bundleAdjuster, ops

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"run_plan reached for {name}")

    for module in (_lib, ops, bundleAdjuster, pipeline):
        if hasattr(module, "lib"):
            monkeypatch.setattr(module, "lib", Untouchable())
    monkeypatch.setattr(_lib, "default_context", Untouchable())
    monkeypatch.setattr(pipeline, "default_context", Untouchable())
    monkeypatch.setattr(pipeline, "torch", Untouchable())
    monkeypatch.setattr(torch, "zeros", Untouchable())
    plan = run_plan(F, 1, False, True, verify={}, poses={}, resect={}, degeneracy={}, guided={}, align=ALIGN, refine={}, **CULL)
    assert plan.sharded and plan.refine["max_reproj_px"] == [8.0, 4.0]


# ------------------------------------------------------------------------------------------------ the stage timers

class Stub:
    """A context whose sync counts its calls, and a clock that a test moves by hand (seconds)."""

    def __init__(self):
        self.syncs, self.t = 0, 100.0

    def sync(self):
        self.syncs += 1

    def now(self):
        return self.t


def test_stage_clock_syncs_twice_per_interval_and_accumulates():
    stub, ms = Stub(), dict(other=1.0)
    clock = pipeline.StageClock(stub, ms, now=stub.now)
    with clock("verify"):
        assert stub.syncs == 1 and "verify" not in ms
        stub.t += 0.25
    assert stub.syncs == 2 and ms == dict(other=1.0, verify=250.0)
    with clock("verify"):
        stub.t += 0.5
    with clock("link"):
        stub.t += 0.125
    assert stub.syncs == 6 and ms == dict(other=1.0, verify=750.0, link=125.0)
    with clock("ba"):                      # an interval inside an open one is billed to both
        stub.t += 1.0
        with clock("ba_solve"):
            stub.t += 2.0
    assert stub.syncs == 10 and ms["ba"] == 3000.0 and ms["ba_solve"] == 2000.0


def test_stage_clock_pauses_poses_around_degeneracy():
    stub, ms = Stub(), dict(degeneracy=500.0)
    clock = pipeline.StageClock(stub, ms, now=stub.now)
    with clock("poses"):
        stub.t += 1.0
        with clock.paused("poses"), clock("degeneracy"):
            assert stub.syncs == 3 and ms["poses"] == 1000.0
            stub.t += 4.0
        assert stub.syncs == 5 and ms["degeneracy"] == 4500.0
        stub.t += 2.0
    assert stub.syncs == 6 and ms == dict(degeneracy=4500.0, poses=3000.0)
    assert clock.since == {}
