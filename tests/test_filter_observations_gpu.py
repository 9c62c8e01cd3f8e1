"""GPU: mm_filter_observations through ops.filter_observations, bundleAdjuster.filterPoints / refinePoints and
ClipPipeline.run(refine=...) against the NumPy restatement and the fixtures of tests/test_filter_observations_cpu.py.

Discrete outputs (flags, counts, maps, fi_out / pi_out) are compared exactly -- every fixture keeps the margins the CPU file
states, asserted again here where a fixture is built in this file -- obs_out bit for bit, err / depth / cos_parallax to 1e-9
relative with NaN in the same places.

Shapes at the scans' edges, with C = ops.FILTER_CHUNK (rows per chunk) and S = 256 (chunk sums per step of the second level,
which one workgroup walks alone: the design has no second level of several workgroups): O and P each in {1, C-1, C, C+1, 2C+3,
S C + C + 3}, tracks straddling the chunk boundaries; O = 0, P = 0, everything kept, everything dropped.
"""
import functools
import math
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_filter_observations_cpu as ref  # noqa: E402
from meatmodeler_amd import bundleAdjuster, ops, synth  # noqa: E402
from meatmodeler_amd.pipeline import ClipPipeline  # noqa: E402
from oracle import ba_oracle as bo  # noqa: E402

DEV = torch.device("cuda", 0)
C = ops.FILTER_CHUNK
S = 256
DISCRETE = ("obs_flags", "pt_flags", "fi", "pi", "obs_map", "point_map")
COUNTS = ("n_obs", "n_points", "removed_obs", "removed_points")
CONTINUOUS = ("err", "depth", "cos_parallax")


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def run(fx, with_ptr=True, **tests):
    """ops.filter_observations on a fixture dict (cams, pts, K, fi, pi, obs, pt_ptr) -> its dict, tensors as NumPy arrays."""
    out = ops.filter_observations(dev(fx["cams"]), dev(fx["pts"]), fx["K"], dev(fx["fi"].astype(np.int32)), dev(fx["pi"].astype(np.int32)),
                                  dev(fx["obs"]), dev(fx["pt_ptr"].astype(np.int32)) if with_ptr else None, **tests)
    return {k: v.cpu().numpy() if torch.is_tensor(v) else v for k, v in out.items()}


def restated(fx, **tests):
    return ref.restate(fx["cams"], fx["pts"], fx["K"], fx["fi"], fx["pi"], fx["obs"], fx["pt_ptr"], **tests)


def agree(got, want):
    for k in COUNTS:
        assert got[k] == want[k], (k, got[k], want[k])
    for k in DISCRETE:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    assert got["obs"].tobytes() == np.ascontiguousarray(want["obs"]).tobytes()
    for k in CONTINUOUS:
        g, w = got[k], want[k]
        assert np.array_equal(np.isnan(g), np.isnan(w)), k
        inf = np.isinf(w)
        assert np.array_equal(g[inf], w[inf]), k
        fin = np.isfinite(w)
        worst = float(np.max(np.abs(g[fin] - w[fin]) / np.maximum(1.0, np.abs(w[fin])), initial=0.0))
        assert worst <= 1e-9, (k, worst)


def same_bits(a, b, keys=DISCRETE + CONTINUOUS + ("obs",)):
    return all(a[k].tobytes() == b[k].tobytes() for k in keys) and all(a[k] == b[k] for k in COUNTS)


# ------------------------------------------------------------------------------------------------ the planted fixtures

def test_planted_fixture_equals_the_restatement():
    fx = ref.planted_fixture()
    want = restated(fx, **ref.PLANTED_TESTS)
    assert ref.margins_hold(want, **ref.PLANTED_TESTS)
    got = run(fx, **ref.PLANTED_TESTS)
    agree(got, want)
    assert np.array_equal(got["obs"], fx["obs"][got["obs_map"]])
    # without pt_ptr the wrapper builds it; a BADevice supplies all four index arrays
    assert same_bits(run(fx, with_ptr=False, **ref.PLANTED_TESTS), got)
    pb = ops.BADevice(fx["K"], fx["fi"], fx["pi"], fx["obs"], len(fx["cams"]), len(fx["pts"]), DEV)
    via = ops.filter_observations(dev(fx["cams"]), dev(fx["pts"]), fx["K"], pb, **ref.PLANTED_TESTS)
    assert same_bits({k: v.cpu().numpy() if torch.is_tensor(v) else v for k, v in via.items()}, got)


def test_each_test_alone_and_the_known_answer():
    fx = ref.planted_fixture()
    for tests in (dict(max_reproj_px=8.0), dict(min_depth=0.1), dict(min_angle_deg=1.0), dict(min_views=4)):
        want = restated(fx, **tests)
        assert ref.margins_hold(want, **tests)
        agree(run(fx, **tests), want)
    pr, planted = ref.outlier_problem(10, 400, 5, 0.05, 2, at_truth=True)
    got = run(pr, max_reproj_px=4.0)
    agree(got, restated(pr, max_reproj_px=4.0))
    assert np.array_equal(got["obs_flags"] == ops.OBS_REPROJ, planted) and got["n_points"] == 400
    # the drop-in wrapper on the same problem: what adjustPoints returns and was given -> the next call's arguments
    pts, obs, fi, pi, pm = bundleAdjuster.filterPoints(pr["pts"], pr["ext_gt"], pr["K"], pr["obs"], pr["fi"], pr["pi"], max_reproj_px=4.0)
    assert np.array_equal(obs, pr["obs"][~planted]) and np.array_equal(fi, pr["fi"][~planted]) and np.array_equal(pi, pr["pi"][~planted])
    assert np.array_equal(pm, np.arange(400)) and np.array_equal(pts, pr["pts"])


# ------------------------------------------------------------------------------------------------ the scans' edges

EDGE_TESTS = dict(max_reproj_px=4.0, min_depth=0.0, min_views=2)
SIZES = (1, C - 1, C, C + 1, 2 * C + 3, S * C + C + 3)


@functools.lru_cache(maxsize=None)
def edge_problem(P, O, seed=0):
    """P points, O observations from 12 orbit cameras: point p owns O // P observations (+ 1 for the first O % P points, so
    with O < P the later points are empty), a quarter of the observations displaced by 30 px or more and the rest within a
    fraction of a pixel (no error near the threshold, however many rows), one point in nine behind the cameras."""
    rng = np.random.default_rng(seed + 7 * P + O)
    base = synth.make_ba_problem(12, 4, track_len=2, seed=1)
    cams = bo.frame_parameters(base["ext_gt"]).reshape(12, 6)
    pts = rng.uniform(-2.0, 2.0, (P, 3))
    counts = np.full(P, O // P, np.int64)
    counts[:O % P] += 1
    pi = np.repeat(np.arange(P), counts)
    fi = (rng.integers(0, 12, P)[pi] + np.arange(O) - np.concatenate([[0], np.cumsum(counts)])[pi]) % 12      # consecutive frames
    d, _ = ref.residuals(cams, pts, base["K"], fi, pi, np.zeros((O, 2)))
    obs = d + rng.normal(0.0, 0.2, (O, 2))
    hit = rng.random(O) < 0.25
    ang = rng.uniform(0, 2 * np.pi, O)
    obs[hit] += (rng.uniform(30.0, 60.0, O)[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=1))[hit]
    back = np.arange(P) % 9 == 4
    pts[back] *= 40.0      # far outside the orbit: behind some cameras, off by far in the others
    return dict(cams=cams, pts=pts, K=np.asarray(base["K"], np.float64), fi=fi.astype(np.int32), pi=pi.astype(np.int32),
                obs=np.ascontiguousarray(obs), pt_ptr=ref.csr(pi, P))


def check_edge(P, O):
    fx = edge_problem(P, O)
    want = restated(fx, **EDGE_TESTS)
    assert ref.margins_hold(want, **EDGE_TESTS)
    got = run(fx, **EDGE_TESTS)
    agree(got, want)
    return fx, got


@pytest.mark.parametrize("O", SIZES)
def test_observation_counts_at_the_scan_edges(O):
    P = max(1, O // 3)
    fx, got = check_edge(P, O)
    if O > C:      # a track straddles the first chunk boundary; with a whole second chunk both sides keep something
        ptr = fx["pt_ptr"]
        assert ((ptr[:-1] < C) & (ptr[1:] > C)).any()
        assert 0 < got["n_obs"] < O and (got["obs_map"] < C).any() and (O < 2 * C or (got["obs_map"] >= C).any())


@pytest.mark.parametrize("P", SIZES)
def test_point_counts_at_the_scan_edges(P):
    fx, got = check_edge(P, (5 * P) // 2)
    if P > C:
        assert 0 < got["n_points"] < P and (got["point_map"] < C).any() and (P < 2 * C or (got["point_map"] >= C).any())


def test_fewer_observations_than_points_leaves_empty_points():
    fx, got = check_edge(C + 1, C - 1)
    assert got["n_points"] == 0 and (got["pt_flags"] & ops.PT_SHORT).all() and np.isnan(got["cos_parallax"]).all()


def test_no_observations_no_points_everything_kept_everything_dropped():
    fx = edge_problem(C + 1, 3 * C + 5)
    none = dict(fx, fi=fx["fi"][:0], pi=fx["pi"][:0], obs=fx["obs"][:0], pt_ptr=np.zeros(C + 2, np.int32))
    got = run(none, **EDGE_TESTS)
    agree(got, restated(none, **EDGE_TESTS))
    assert got["n_obs"] == 0 and got["n_points"] == 0 and got["fi"].shape == (0,) and got["obs"].shape == (0, 2)
    empty = dict(none, pts=fx["pts"][:0], pt_ptr=np.zeros(1, np.int32))
    got = run(empty, **EDGE_TESTS)
    assert (got["n_obs"], got["n_points"], got["removed_obs"], got["removed_points"]) == (0, 0, 0, 0) and got["pt_flags"].shape == (0,)
    # everything kept: the clean observations of a problem at its ground truth
    pr, _ = ref.outlier_problem(10, 400, 5, 0.05, 2, at_truth=True)
    clean = dict(pr, obs=pr["obs_clean"])
    got = run(clean, max_reproj_px=6.0)
    agree(got, restated(clean, max_reproj_px=6.0))
    assert got["n_obs"] == 2000 and got["n_points"] == 400 and np.array_equal(got["obs_map"], np.arange(2000))
    assert np.array_equal(got["pi"], pr["pi"]) and got["obs"].tobytes() == clean["obs"].tobytes()
    # everything dropped, by the observations' own test and by the points'
    got = run(clean, max_reproj_px=0.0)
    agree(got, restated(clean, max_reproj_px=0.0))
    assert got["n_obs"] == 0 and got["n_points"] == 0 and got["removed_obs"] == 2000
    got = run(clean, min_views=6)
    agree(got, restated(clean, min_views=6))
    assert got["n_obs"] == 0 and got["removed_obs"] == 0 and (got["obs_flags"] == ops.OBS_ORPHAN).all()


# ------------------------------------------------------------------------------------------------ repeatability and isolation

def test_a_call_repeats_bit_for_bit():
    for fx, tests in ((ref.planted_fixture(), ref.PLANTED_TESTS), (edge_problem(2 * C + 3, 5 * C + 7), EDGE_TESTS)):
        first = run(fx, **tests)
        for _ in range(3):
            assert same_bits(run(fx, **tests), first)


def test_a_points_outputs_do_not_depend_on_the_other_points():
    fx = ref.planted_fixture()
    whole = run(fx, **ref.PLANTED_TESTS)
    P, ptr = len(fx["pts"]), fx["pt_ptr"]
    rng = np.random.default_rng(5)
    for order in (rng.permutation(P), rng.permutation(P)[: P // 3], np.arange(P)[::-1]):
        rows = np.concatenate([np.arange(ptr[p], ptr[p + 1]) for p in order])
        pi2 = np.repeat(np.arange(len(order)), np.diff(ptr)[order]).astype(np.int32)
        sub = dict(fx, pts=fx["pts"][order], fi=fx["fi"][rows], pi=pi2, obs=fx["obs"][rows], pt_ptr=ref.csr(pi2, len(order)))
        got = run(sub, **ref.PLANTED_TESTS)
        assert np.array_equal(got["pt_flags"], whole["pt_flags"][order]) and np.array_equal(got["obs_flags"], whole["obs_flags"][rows])
        assert got["cos_parallax"].tobytes() == whole["cos_parallax"][order].tobytes()
        assert got["err"].tobytes() == whole["err"][rows].tobytes() and got["depth"].tobytes() == whole["depth"][rows].tobytes()
        # and the compaction is the restatement's on the reordered problem
        agree(got, restated(sub, **ref.PLANTED_TESTS))


# ------------------------------------------------------------------------------------------------ the run() contract

@functools.lru_cache(maxsize=None)
def clip():
    frames, ext, K = synth.render_orbit_frames(6, 640, 480, arc_deg=6.0)
    return dev(frames), ext, K


def pipe():
    return ClipPipeline(480, 640, 600, batch=6)


def equal_values(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.shape == b.shape and torch.equal(a, b)
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    if isinstance(a, dict):
        return set(a) == set(b) and all(equal_values(a[k], b[k]) for k in a)
    if isinstance(a, bundleAdjuster.BAResult):
        return all(equal_values(getattr(a, k), getattr(b, k)) for k in ("cams", "pts", "cost", "nfev", "status", "optimality"))
    return a == b


def test_run_without_refine_is_what_it_was():
    frames, ext, K = clip()
    plain = pipe().run(frames, K, ext, ba=True)
    none = pipe().run(frames, K, ext, ba=True, refine=None)
    assert "refine" not in plain and "refine" not in none and set(plain) == set(none)
    for k in plain:
        assert equal_values(plain[k], none[k]), k
    # with refine every existing key keeps its value, `ba` included
    timers = {}
    refined = pipe().run(frames, K, ext, ba=True, refine=dict(max_reproj_px=(2.0, 1.0, 0.5), rounds=3), timers=timers)
    assert set(refined) == set(plain) | {"refine"} and "refine" in timers
    for k in plain:
        assert equal_values(plain[k], refined[k]), k


def round_inputs(out, K):
    """Per round of out["refine"]: (cams, pts, fi, pi, obs) it was given, as device tensors."""
    rf = out["refine"]
    coords, fi, pi = ops.flatten_tracks(out["track_ptr_dev"], out["obs_frame_dev"], out["obs_kp_dev"], out["xy_dev"])
    given = [(out["ba"], fi, pi, coords)]
    for flt, res in zip(rf["filters"], rf["results"]):
        given.append((res, flt["fi"], flt["pi"], flt["obs"]))
    return [(res.cams.reshape(6, 6), res.pts.reshape(-1, 3), fi, pi, obs) for res, fi, pi, obs in given[:len(rf["rounds"])]]


def test_run_with_refine_filters_and_adjusts_exactly_what_survives():
    frames, ext, K = clip()
    # one evaluation per re-solve: each returns its initial cost at its initial points (no evaluation left for a step)
    out = pipe().run(frames, K, ext, ba=True, refine=dict(max_reproj_px=(2.0, 1.0, 0.5), rounds=3, max_nfev=1))
    rf = out["refine"]
    rounds = rf["rounds"]
    assert 1 <= len(rounds) <= 3 and len(rf["filters"]) == len(rounds)
    assert any(r["cost_in"] is not None for r in rounds), "no round flagged anything: the test shows nothing"
    n_o, n_p = out["n_obs"], out["n_tracks"]
    pm, om = np.arange(n_p), np.arange(n_o)
    for r, (row, flt, (cams, pts, fi, pi, obs)) in enumerate(zip(rounds, rf["filters"], round_inputs(out, K))):
        assert row["max_reproj_px"] == (2.0, 1.0, 0.5)[r]
        direct = ops.filter_observations(cams, pts, K, fi, pi, obs, max_reproj_px=row["max_reproj_px"])
        for k in DISCRETE + CONTINUOUS + ("obs",):
            assert torch.equal(direct[k], flt[k]) or (k in CONTINUOUS and direct[k].cpu().numpy().tobytes() == flt[k].cpu().numpy().tobytes()), (r, k)
        assert (row["n_obs"], row["n_points"]) == (flt["n_obs"], flt["n_points"])
        assert (row["removed_obs"], row["removed_points"]) == (n_o - flt["n_obs"], n_p - flt["n_points"])
        n_o, n_p = flt["n_obs"], flt["n_points"]
        if row["cost_in"] is None:
            assert r == len(rounds) - 1 and row["removed_obs"] == 0 and row["removed_points"] == 0
            continue
        pm, om = pm[flt["point_map"].cpu().numpy()], om[flt["obs_map"].cpu().numpy()]
        res = rf["results"][r]
        kept_pts = pts[flt["point_map"].long()]
        assert res.nfev == 1 and torch.equal(res.pts.reshape(-1, 3), kept_pts) and torch.equal(res.cams.reshape(6, 6), cams)
        x0 = np.hstack([cams.cpu().numpy().ravel(), kept_pts.cpu().numpy().ravel()])
        c0 = 0.5 * np.sum(bo.point_fun(x0, K, 6, n_p, flt["fi"].cpu().numpy(), flt["pi"].cpu().numpy(), flt["obs"].cpu().numpy()) ** 2)
        print(f"round {r}: tau {row['max_reproj_px']}, {row['removed_obs']} observations and {row['removed_points']} points removed, "
              f"initial cost {row['cost_in']:.6e} (NumPy {c0:.6e})")
        assert abs(row["cost_in"] - c0) <= 1e-9 * c0 and abs(res.cost - c0) <= 1e-9 * c0
        assert row["cost_out"] <= row["cost_in"]
    assert np.array_equal(rf["point_map"].cpu().numpy(), pm) and np.array_equal(rf["obs_map"].cpu().numpy(), om)
    assert torch.equal(rf["obs_flags"], rf["filters"][0]["obs_flags"]) and torch.equal(rf["pt_flags"], rf["filters"][0]["pt_flags"])
    assert rf["ba"] is (rf["results"][-1] if rf["results"] else out["ba"])
    # full re-solves: the cost of every round falls, and the refined points are those of point_map
    full = pipe().run(frames, K, ext, ba=True, refine=dict(max_reproj_px=(2.0, 1.0, 0.5), rounds=3))
    for row in full["refine"]["rounds"]:
        assert row["cost_in"] is None or row["cost_out"] <= row["cost_in"]
    assert full["refine"]["ba"].pts.reshape(-1, 3).shape[0] == full["refine"]["point_map"].numel()


def test_run_refuses_refine_across_ranks_and_bad_options():
    frames, ext, K = clip()

    class TwoRanks:
        @staticmethod
        def get_world_size():
            return 2

        @staticmethod
        def get_rank():
            return 0

    with pytest.raises(ValueError):
        pipe().run(frames, K, ext, refine={}, dist=TwoRanks())
    for bad in (dict(max_reproj=4.0), dict(rounds=0), dict(max_reproj_px=math.inf), 4.0):
        with pytest.raises(ValueError):
            pipe().run(frames, K, ext, refine=bad)


# ------------------------------------------------------------------------------------------------ end to end, with a cap

def test_refined_adjustment_sheds_the_planted_outliers():
    """The fixture and the schedule are the ones the SciPy + NumPy loop of the CPU file meets the same caps with."""
    pr, planted = ref.outlier_problem(**ref.E2E)
    F, K = len(pr["ext"]), pr["K"]
    pts, ext, rep = bundleAdjuster.refinePoints(pr["ext"], K, pr["pts0"], pr["obs"], pr["fi"], pr["pi"], verbose=0, **ref.E2E_REFINE)
    om, pm = rep["obs_map"], rep["point_map"]
    assert len(pts) == pm.size and len(ext) == F
    fi, obs = pr["fi"][om], pr["obs"][om]
    pi = (np.cumsum(np.isin(np.arange(len(pr["pts0"])), pm)) - 1)[pr["pi"][om]]
    x = np.hstack([bo.frame_parameters(np.asarray(ext)).ravel(), np.asarray(pts).ravel()])
    cost = 0.5 * np.sum(bo.point_fun(x, K, F, len(pts), fi, pi, obs) ** 2)
    clean = bundleAdjuster.solvePoints(pr["ext"], K, pr["pts0"], pr["obs_clean"], pr["fi"], pr["pi"], verbose=0)
    left, lost = int(planted[om].sum()), int((~planted).sum() - (~planted[om]).sum())
    r_out, r_ref = ref.rms(cost, om.size), ref.rms(clean.cost, planted.size)
    print(f"refined: {len(rep['rounds'])} rounds {[(r['max_reproj_px'], r['removed_obs'], r['nfev']) for r in rep['rounds']]}, planted left "
          f"{left} of {planted.sum()}, clean lost {lost} of {(~planted).sum()}, rms {r_out:.4f} against {r_ref:.4f} outlier-free")
    assert left == 0
    assert lost <= 0.05 * (~planted).sum()
    assert r_out <= 1.5 * r_ref


def test_refine_points_keeps_fixed_frames_as_given():
    pr, planted = ref.outlier_problem(**ref.E2E)
    F, K = len(pr["ext"]), pr["K"]
    ext0 = np.concatenate([pr["ext"], np.tile([[[0.0, 0.0, 0.0, 1.0]]], (F, 1, 1))], axis=1)
    pts, ext, rep = bundleAdjuster.refinePoints(ext0, K, pr["pts0"], pr["obs"], pr["fi"], pr["pi"], fixed_frames=[0, F - 1], verbose=0,
                                                **ref.E2E_REFINE)
    cams_in, cams_out = bo.frame_parameters(ext0).reshape(F, 6), bo.frame_parameters(np.asarray(ext)).reshape(F, 6)
    assert np.abs(cams_out[[0, F - 1]] - cams_in[[0, F - 1]]).max() <= 1e-12 and np.abs(cams_out[1:F - 1] - cams_in[1:F - 1]).max() > 1e-6
    assert len(pts) == rep["point_map"].size and planted[rep["obs_map"]].sum() == 0
    assert rep["rounds"][0]["removed_obs"] >= planted.sum() and rep["rounds"][0]["cost_out"] <= rep["rounds"][0]["cost_in"]
