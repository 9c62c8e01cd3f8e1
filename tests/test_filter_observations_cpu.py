"""CPU: the definition of mm_filter_observations (include/meatmodeler.h, a-9b) restated in NumPy, its fixtures and the
filter-and-re-adjust loop in NumPy + SciPy.  tests/test_filter_observations_gpu.py compares the kernels with `restate` on the
fixtures of this file.

The restatement follows the header operation by operation (the library builds filter.hip without FMA contraction): the camera
table (R, t, C), step 1 per observation, step 2 per point over the survivors, the orphans, the order-preserving compaction.
Discrete outputs are compared exactly on the GPU, so every fixture keeps a margin, asserted here: every decided
|e - tau| >= 1e-6 tau, |depth - min_depth| >= 1e-9 and every cosine at least 1e-9 from its bound -- a thousand times what the
two sides' sin / cos / sqrt and division can differ by.
"""
import functools
import math

import numpy as np

from meatmodeler_amd import synth
from oracle import ba_oracle as bo

OBS_REPROJ, OBS_BEHIND, OBS_NONFINITE, OBS_ORPHAN = 1, 2, 4, 8
PT_SHORT, PT_PARALLAX, PT_NONFINITE = 1, 2, 4
CHUNK = 1024


# ------------------------------------------------------------------------------------------------ the restatement

def camera_table(cams):
    """cams [F, 6] -> (R [F, 9] row-major, t [F, 3], C [F, 3]), the header's expressions."""
    cams = np.asarray(cams, np.float64).reshape(-1, 6)
    rx, ry, rz = cams[:, 0], cams[:, 1], cams[:, 2]
    t = cams[:, 3:6]
    with np.errstate(all="ignore"):
        th2 = (rx * rx + ry * ry) + rz * rz
        small = th2 < 1e-4
        th = np.sqrt(th2)
        sh = np.sin(0.5 * th)
        c = np.cos(th)
        a = np.where(small, 1.0 + th2 * (-1.0 / 6 + th2 * (1.0 / 120 - th2 * (1.0 / 5040))), np.sin(th) / th)
        b = np.where(small, 0.5 + th2 * (-1.0 / 24 + th2 * (1.0 / 720 - th2 * (1.0 / 40320))), (2.0 * sh * sh) / th2)
        R = np.stack([c + b * rx * rx, -a * rz + b * rx * ry, a * ry + b * rx * rz,
                      a * rz + b * ry * rx, c + b * ry * ry, -a * rx + b * ry * rz,
                      -a * ry + b * rz * rx, a * rx + b * rz * ry, c + b * rz * rz], axis=1)
        C = np.stack([-((R[:, j] * t[:, 0] + R[:, 3 + j] * t[:, 1]) + R[:, 6 + j] * t[:, 2]) for j in range(3)], axis=1)
    return R, t, C


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def residuals(cams, pts, K, fi, pi, obs):
    """step 1's (dx, dy) [O, 2], depth [O]"""
    R, t, _ = camera_table(cams)
    K = np.asarray(K, np.float64).reshape(9)
    X, Rf, tf = np.asarray(pts, np.float64)[pi], R[fi], t[fi]
    with np.errstate(all="ignore"):
        Y = [((Rf[:, 3 * i] * X[:, 0] + Rf[:, 3 * i + 1] * X[:, 1]) + Rf[:, 3 * i + 2] * X[:, 2]) + tf[:, i] for i in range(3)]
        u = [(K[3 * i] * Y[0] + K[3 * i + 1] * Y[1]) + K[3 * i + 2] * Y[2] for i in range(3)]
        d = np.stack([u[0] / u[2] - obs[:, 0], u[1] / u[2] - obs[:, 1]], axis=1)
    return d, Y[2]


def restate(cams, pts, K, fi, pi, obs, pt_ptr, max_reproj_px=math.inf, min_angle_deg=0.0, min_depth=-math.inf, min_views=2):
    """Steps 1 to 4 -> dict of what ops.filter_observations returns (NumPy arrays)."""
    cams, pts, obs = (np.asarray(a, np.float64) for a in (cams, pts, obs))
    fi, pi, pt_ptr = (np.asarray(a, np.int64) for a in (fi, pi, pt_ptr))
    O, P = fi.size, pts.shape[0]
    max_cos = math.cos(math.radians(min_angle_deg)) if min_angle_deg > 0 else 2.0
    if O == 0 or P == 0:      # (counts = 0, nothing else is written: the wrapper's fills)
        z = np.zeros(0, np.int32)
        return dict(fi=z, pi=z, obs=np.zeros((0, 2)), obs_map=z, point_map=z, n_obs=0, n_points=0, removed_obs=0,
                    removed_points=P if not O else 0, obs_flags=np.zeros(O, np.int32), pt_flags=np.full(P, PT_SHORT if not O else 0, np.int32),
                    err=np.full(O, np.nan), depth=np.full(O, np.nan), cos_parallax=np.full(P, np.nan))
    # step 1
    d, depth = residuals(cams, pts, K, fi, pi, obs)
    with np.errstate(all="ignore"):
        err = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
        obs_flags = (OBS_NONFINITE * ~(np.isfinite(err) & np.isfinite(depth)) + OBS_BEHIND * (depth <= min_depth)
                     + OBS_REPROJ * (err > max_reproj_px)).astype(np.int32)
    # step 2: survivors in order; the first survivor of a point is the parallax reference
    assert (np.repeat(np.arange(P), np.diff(pt_ptr)) == pi).all(), "pt_ptr is not the CSR of pi"
    _, _, C = camera_table(cams)
    s = np.nonzero(obs_flags == 0)[0]
    n_ok = np.bincount(pi[s], minlength=P)
    first = np.full(P, -1, np.int64)
    up, ui = np.unique(pi[s], return_index=True)
    first[up] = s[ui]
    later = s[s != first[pi[s]]]
    cmin = np.full(P, np.inf)
    with np.errstate(all="ignore"):
        a = C[fi[first[pi[later]]]] - pts[pi[later]]
        b = C[fi[later]] - pts[pi[later]]
        cs = _dot(a, b) / np.sqrt(_dot(a, a) * _dot(b, b))
        np.minimum.at(cmin, pi[later], cs)      # (np.minimum keeps a NaN)
        cosp = np.where(n_ok < 2, np.nan, cmin)
        pt_flags = (PT_NONFINITE * ~np.isfinite(pts).all(axis=1) + PT_SHORT * (n_ok < min_views)
                    + PT_PARALLAX * (cosp > max_cos)).astype(np.int32)
    # step 3
    own = int((obs_flags != 0).sum())
    obs_flags = np.where((obs_flags == 0) & (pt_flags[pi] != 0), OBS_ORPHAN, obs_flags).astype(np.int32)
    # step 4
    obs_map = np.nonzero(obs_flags == 0)[0]
    point_map = np.nonzero(pt_flags == 0)[0]
    new = np.cumsum(pt_flags == 0) - 1
    return dict(fi=fi[obs_map].astype(np.int32), pi=new[pi[obs_map]].astype(np.int32), obs=obs[obs_map], obs_map=obs_map.astype(np.int32),
                point_map=point_map.astype(np.int32), n_obs=obs_map.size, n_points=point_map.size, removed_obs=own,
                removed_points=P - point_map.size, obs_flags=obs_flags, pt_flags=pt_flags, err=err, depth=depth, cos_parallax=cosp)


def margins_hold(ref, max_reproj_px=math.inf, min_angle_deg=0.0, min_depth=-math.inf, **_):
    """The margin condition of the module docstring on a restated result."""
    e, dep, cp = ref["err"], ref["depth"], ref["cos_parallax"]
    ok = True
    if math.isfinite(max_reproj_px):
        ok &= bool((np.abs(e[np.isfinite(e)] - max_reproj_px) >= 1e-6 * max_reproj_px).all())
    if math.isfinite(min_depth):
        ok &= bool((np.abs(dep[np.isfinite(dep)] - min_depth) >= 1e-9).all())
    if min_angle_deg > 0:
        ok &= bool((np.abs(cp[np.isfinite(cp)] - math.cos(math.radians(min_angle_deg))) >= 1e-9).all())
    return ok


def csr(pi, P):
    return np.concatenate([[0], np.cumsum(np.bincount(np.asarray(pi, np.int64), minlength=P))]).astype(np.int32)


# ------------------------------------------------------------------------------------------------ fixtures

PLANTED_TESTS = dict(max_reproj_px=8.0, min_angle_deg=1.0, min_depth=0.1, min_views=3)


@functools.lru_cache(maxsize=None)
def planted_fixture(seed=3):
    """A ragged problem (bo.ragged_ba_problem: track lengths 1 .. 30, an empty camera run, cameras at the series / closed-form
    boundaries of the rotation) at its noisy start, with planted points put in front of, between and behind its own:
    name -> point index in `planted`.  Judged under PLANTED_TESTS."""
    rng = np.random.default_rng(seed)
    pr = bo.ragged_ba_problem(seed, 40, 260, plant=False)
    K = np.asarray(pr["K"], np.float64)
    cams = pr["cams"].copy()
    F = cams.shape[0]
    s0 = int(pr["special"][0])
    cams[s0] = [0.0, 0.0, 0.0, 0.0, 0.0, 10.0]      # R = I exactly: a point with z = -10 has u[2] = 0 there
    lo_e, hi_e = pr["empty"]
    f_nan = lo_e + 1                                 # a camera of the empty run: only planted points see it
    orbit = [f for f in range(F) if f not in set(pr["special"].tolist()) and not lo_e <= f < hi_e]
    tracks = [(pr["pts0"][p], pr["fi"][pr["pi"] == p], pr["obs"][pr["pi"] == p]) for p in range(len(pr["pts0"]))]
    planted = {}

    def project(frames, X):
        frames = np.asarray(frames, np.int64)
        d, _ = residuals(cams, X[None], K, frames, np.zeros(frames.size, np.int64), np.zeros((frames.size, 2)))
        return d + rng.normal(0.0, 0.3, d.shape)

    def plant(name, X, frames, at=None, shift=None):
        X = np.asarray(X, np.float64)
        xy = project(frames, X) if len(frames) else np.zeros((0, 2))
        for k, dxy in (shift or {}).items():
            xy[k] += dxy
        planted[name] = (X, np.asarray(frames, np.int64), xy, at)

    def cube():
        return rng.uniform(-1.5, 1.5, 3)

    far = [orbit[0], orbit[4], orbit[9], orbit[14], orbit[-1]]      # cameras several degrees apart
    plant("displaced", cube(), far, shift={1: (50.0, -30.0)})
    R, t, C = camera_table(cams)
    s4 = int(pr["special"][4])
    plant("behind_one_camera", C[s4] - R[s4, 6:9], [s4] + far[:4])      # one unit behind camera s4, along its axis
    plant("nan_point", [np.nan, 0.0, 1.0], far[:3])
    plant("nan_camera", cube(), [f_nan] + far[:4])
    plant("u2_zero", [0.5, -0.25, -10.0], [s0] + far[:4])
    plant("first_flagged", cube(), far, shift={0: (-70.0, 40.0)})
    plant("exactly_min_views", cube(), far[:4], shift={2: (0.0, 90.0)})
    plant("one_short", cube(), far[:3], shift={1: (60.0, 60.0)})
    plant("all_flagged", cube(), far[:3], shift={0: (45.0, 0.0), 1: (0.0, -45.0), 2: (-45.0, 45.0)})
    plant("empty", cube(), [])
    plant("zero_baseline", C[orbit[5]] + 3.0e4 * R[orbit[5], 6:9], orbit[5:9])
    plant("special_cameras", cube(), [int(f) for f in pr["special"]])      # every rotation branch and boundary, clean
    cams[f_nan, 1] = np.nan
    # the planted points go in front, in the middle and at the end
    order = [("ragged", p) for p in range(len(tracks))]
    for k, n in enumerate(planted):
        order.insert((0, len(order) // 2, len(order))[k % 3], ("planted", n))
    pts, fi, pi, obs, index = [], [], [], [], {}
    for kind, key in order:
        X, fr, xy = tracks[key] if kind == "ragged" else planted[key][:3]
        if kind == "planted":
            index[key] = len(pts)
        fi.append(fr)
        pi.append(np.full(len(fr), len(pts), np.int64))
        obs.append(np.asarray(xy, np.float64).reshape(-1, 2))
        pts.append(X)
    pts = np.asarray(pts, np.float64)
    fi, pi, obs = np.concatenate(fi).astype(np.int32), np.concatenate(pi).astype(np.int32), np.concatenate(obs)
    return dict(cams=cams, pts=pts, K=K, fi=fi, pi=pi, obs=np.ascontiguousarray(obs), pt_ptr=csr(pi, len(pts)), planted=index,
                s0=s0, s4=s4, f_nan=f_nan)


@functools.lru_cache(maxsize=None)
def outlier_problem(n_frames, n_points, track_len, frac, seed, at_truth=False):
    """synth.make_ba_problem with `frac` of its observations displaced by 40 .. 120 px in a random direction, at most one per
    point -> (problem dict with obs replaced and cams / pts of the start (or of the ground truth), planted [O] bool)."""
    pr = dict(synth.make_ba_problem(n_frames, n_points, track_len=track_len, seed=seed))
    rng = np.random.default_rng(1000 + seed)
    O = pr["fi"].size
    n = int(round(frac * O))
    pts_hit = rng.choice(n_points, size=n, replace=False)      # (one observation each)
    ptr = csr(pr["pi"], n_points)
    rows = ptr[pts_hit] + rng.integers(0, np.diff(ptr)[pts_hit])
    ang, mag = rng.uniform(0, 2 * np.pi, n), rng.uniform(40.0, 120.0, n)
    pr["obs_clean"] = pr["obs"]
    pr["obs"] = pr["obs"].copy()
    pr["obs"][rows] += np.stack([mag * np.cos(ang), mag * np.sin(ang)], axis=1)
    planted = np.zeros(O, bool)
    planted[rows] = True
    ext = pr["ext_gt"] if at_truth else pr["ext"]
    pr["cams"] = bo.frame_parameters(ext).reshape(n_frames, 6)
    pr["pts"] = pr["pts_gt"] if at_truth else pr["pts0"]
    pr["pt_ptr"] = ptr
    return pr, planted


# the end-to-end fixture (the GPU file runs the same problem): chosen so that THIS file's SciPy + NumPy loop meets the caps --
# no planted observation left, at most 5 % of the clean ones removed, final RMS within 1.5 x of the outlier-free solve
E2E = dict(n_frames=16, n_points=240, track_len=8, frac=0.02, seed=5)
E2E_REFINE = dict(max_reproj_px=(16.0, 8.0, 4.0), rounds=4, min_views=3)


def cpu_refine(pr, max_reproj_px, rounds=2, ftol=1e-4, max_nfev=None, **tests):
    """The rounds of bundleAdjuster.refine_rounds with bo.adjust_points as the solver and `restate` as the filter."""
    taus = list(np.atleast_1d(max_reproj_px).astype(float))
    F, K = len(pr["ext"]), pr["K"]
    fi, pi, obs = pr["fi"].astype(np.int64), pr["pi"].astype(np.int64), pr["obs"]
    pts, ext, res = bo.adjust_points(pr["ext"], K, pr["pts0"], obs, fi, pi, ftol=ftol, max_nfev=max_nfev, return_result=True)
    first = res
    point_map, obs_map = np.arange(len(pts)), np.arange(fi.size)
    log, flags = [], None
    for r in range(rounds):
        tau = taus[min(r, len(taus) - 1)]
        cams = res.x[:6 * F].reshape(F, 6)
        flt = restate(cams, pts, K, fi, pi, obs, csr(pi, len(pts)), max_reproj_px=tau, **tests)
        flags = flags or (flt["obs_flags"], flt["pt_flags"])
        row = dict(max_reproj_px=tau, n_obs=flt["n_obs"], n_points=flt["n_points"], removed_obs=fi.size - flt["n_obs"],
                   removed_points=len(pts) - flt["n_points"], cost_in=None, cost_out=None, nfev=0, status=None,
                   inputs=(cams.copy(), pts.copy(), fi, pi, obs), filter=flt)
        log.append(row)
        if row["removed_obs"] == 0 and row["removed_points"] == 0:
            break
        point_map, obs_map = point_map[flt["point_map"]], obs_map[flt["obs_map"]]
        fi, pi, obs = flt["fi"].astype(np.int64), flt["pi"].astype(np.int64), flt["obs"]
        pts0 = pts[flt["point_map"]]
        x0 = np.hstack([cams.ravel(), pts0.ravel()])
        row["cost_in"] = 0.5 * float(np.sum(bo.point_fun(x0, K, F, len(pts0), fi, pi, obs) ** 2))
        ext_in = np.stack([np.hstack([bo.rodrigues_matrix(c[:3]), c[3:, None]]) for c in cams])
        pts, ext, res = bo.adjust_points(ext_in, K, pts0, obs, fi, pi, ftol=ftol, max_nfev=max_nfev, return_result=True)
        row.update(cost_out=float(res.cost), nfev=int(res.nfev), status=int(res.status))
    return dict(first=first, x=res.x, cost=float(res.cost), pts=pts, fi=fi, pi=pi, obs=obs, point_map=point_map, obs_map=obs_map,
                rounds=log, obs_flags=flags[0], pt_flags=flags[1])


def rms(cost, n_obs):
    return math.sqrt(2.0 * cost / n_obs)


# ------------------------------------------------------------------------------------------------ tests

def test_restated_residuals_equal_the_oracle_cost_function():
    fx = planted_fixture()
    ok = ~np.isnan(fx["cams"]).any(axis=1)[fx["fi"]] & np.isfinite(fx["pts"]).all(axis=1)[fx["pi"]]
    fi, pi, obs = fx["fi"][ok], fx["pi"][ok], fx["obs"][ok]
    cams = np.where(np.isnan(fx["cams"]), 0.0, fx["cams"])
    d, _ = residuals(cams, fx["pts"], fx["K"], fi, pi, obs)
    x = np.hstack([cams.ravel(), np.nan_to_num(fx["pts"]).ravel()])
    with np.errstate(all="ignore"):
        r = bo.point_fun(x, fx["K"], len(cams), len(fx["pts"]), fi, pi, obs).reshape(-1, 2)
    fin = np.isfinite(r).all(axis=1) & (np.abs(r).max(axis=1) < 1e4)      # (u[2] = 0 aside)
    assert fin.sum() > 0.95 * len(r)
    print("restatement against bo.point_fun: max |difference|", np.abs(d[fin] - r[fin]).max())
    assert np.abs(d[fin] - r[fin]).max() <= 1e-12
    # the cameras at the series / closed-form boundaries are among them
    assert set(bo.ragged_ba_problem(3, 40, 260, plant=False)["special"].tolist()) <= set(fi.tolist())


def test_planted_cases_get_the_flags_the_definition_gives_them():
    fx = planted_fixture()
    ref = restate(fx["cams"], fx["pts"], fx["K"], fx["fi"], fx["pi"], fx["obs"], fx["pt_ptr"], **PLANTED_TESTS)
    assert margins_hold(ref, **PLANTED_TESTS)
    ptr, of, pf, idx = fx["pt_ptr"], ref["obs_flags"], ref["pt_flags"], fx["planted"]

    def rows(name):
        return of[ptr[idx[name]]:ptr[idx[name] + 1]].tolist()

    assert rows("displaced") == [0, OBS_REPROJ, 0, 0, 0] and pf[idx["displaced"]] == 0
    assert ref["err"][ptr[idx["displaced"]] + 1] >= 40.0
    assert rows("behind_one_camera") == [OBS_BEHIND, 0, 0, 0, 0] and pf[idx["behind_one_camera"]] == 0
    assert ref["depth"][ptr[idx["behind_one_camera"]]] < -0.5
    assert rows("nan_point") == [OBS_NONFINITE] * 3 and pf[idx["nan_point"]] == PT_NONFINITE | PT_SHORT
    assert rows("nan_camera") == [OBS_NONFINITE, 0, 0, 0, 0] and pf[idx["nan_camera"]] == 0
    o = ptr[idx["u2_zero"]]
    assert ref["depth"][o] == 0.0 and not np.isfinite(ref["err"][o]) and of[o] & OBS_NONFINITE and of[o] & OBS_BEHIND
    assert rows("u2_zero")[1:] == [0, 0, 0, 0]
    assert rows("first_flagged") == [OBS_REPROJ, 0, 0, 0, 0] and pf[idx["first_flagged"]] == 0
    assert rows("exactly_min_views") == [0, 0, OBS_REPROJ, 0] and pf[idx["exactly_min_views"]] == 0
    assert rows("one_short") == [OBS_ORPHAN, OBS_REPROJ, OBS_ORPHAN] and pf[idx["one_short"]] == PT_SHORT
    assert rows("all_flagged") == [OBS_REPROJ] * 3 and pf[idx["all_flagged"]] == PT_SHORT
    assert np.isnan(ref["cos_parallax"][idx["all_flagged"]])
    assert rows("empty") == [] and pf[idx["empty"]] == PT_SHORT and np.isnan(ref["cos_parallax"][idx["empty"]])
    assert rows("special_cameras") == [0] * 7 and pf[idx["special_cameras"]] == 0
    assert rows("zero_baseline") == [OBS_ORPHAN] * 4 and pf[idx["zero_baseline"]] == PT_PARALLAX
    assert ref["cos_parallax"][idx["zero_baseline"]] > 1.0 - 1e-8
    # the parallax reference of first_flagged is its second observation: the cosine is the one of the point without the first
    p = idx["first_flagged"]
    sl = slice(ptr[p] + 1, ptr[p + 1])
    sub = restate(fx["cams"], fx["pts"][p:p + 1], fx["K"], fx["fi"][sl], np.zeros(4, np.int64), fx["obs"][sl], [0, 4], **PLANTED_TESTS)
    assert sub["cos_parallax"][0] == ref["cos_parallax"][p]
    # the ragged part brings every verdict too: short tracks, thin parallax, errors on either side of the threshold
    assert (pf == 0).sum() > 50 and (pf & PT_SHORT).sum() > 20 and (pf & PT_PARALLAX).sum() > 5 and (of == OBS_REPROJ).sum() > 10
    # compaction: order kept, points renumbered, point-major again
    assert (np.diff(ref["obs_map"]) > 0).all() and (np.diff(ref["point_map"]) > 0).all() and (np.diff(ref["pi"]) >= 0).all()
    assert np.array_equal(ref["point_map"][ref["pi"]], fx["pi"][ref["obs_map"]])
    assert np.array_equal(ref["obs"], fx["obs"][ref["obs_map"]]) and np.array_equal(ref["fi"], fx["fi"][ref["obs_map"]])
    assert ref["n_obs"] == (of == 0).sum() and ref["n_points"] == (pf == 0).sum()
    assert ref["removed_obs"] == ((of != 0) & (of != OBS_ORPHAN)).sum() and ref["removed_points"] == (pf != 0).sum()
    assert np.bincount(ref["pi"], minlength=ref["n_points"]).min() >= PLANTED_TESTS["min_views"]


def test_a_points_verdict_does_not_depend_on_the_other_points():
    fx = planted_fixture()
    ref = restate(fx["cams"], fx["pts"], fx["K"], fx["fi"], fx["pi"], fx["obs"], fx["pt_ptr"], **PLANTED_TESTS)
    P, ptr = len(fx["pts"]), fx["pt_ptr"]
    perm = np.random.default_rng(0).permutation(P)[: P // 2]
    rows = np.concatenate([np.arange(ptr[p], ptr[p + 1]) for p in perm])
    pi2 = np.repeat(np.arange(len(perm)), np.diff(ptr)[perm])
    sub = restate(fx["cams"], fx["pts"][perm], fx["K"], fx["fi"][rows], pi2, fx["obs"][rows], csr(pi2, len(perm)), **PLANTED_TESTS)
    assert np.array_equal(sub["pt_flags"], ref["pt_flags"][perm]) and np.array_equal(sub["obs_flags"], ref["obs_flags"][rows])
    assert np.array_equal(sub["cos_parallax"], ref["cos_parallax"][perm], equal_nan=True)
    assert np.array_equal(sub["err"], ref["err"][rows], equal_nan=True)


def test_known_answer_exactly_the_displaced_observations_are_flagged_at_the_truth():
    pr, planted = outlier_problem(10, 400, 5, 0.05, 2, at_truth=True)
    assert planted.sum() == 100 and np.bincount(pr["pi"][planted]).max() == 1
    tests = dict(max_reproj_px=4.0)
    ref = restate(pr["cams"], pr["pts"], pr["K"], pr["fi"], pr["pi"], pr["obs"], pr["pt_ptr"], **tests)
    assert margins_hold(ref, **tests)
    # a clean error above 4 px at sigma = 0.5 has probability exp(-32) per observation
    assert np.array_equal(ref["obs_flags"] == OBS_REPROJ, planted) and (ref["obs_flags"][~planted] == 0).all()
    assert (ref["pt_flags"] == 0).all() and ref["n_obs"] == planted.size - 100 and ref["n_points"] == 400
    assert ref["err"][planted].min() >= 40.0 - 4.0 and ref["err"][~planted].max() < 4.0


def test_degenerate_sizes_and_everything_kept_or_dropped():
    fx = planted_fixture()
    none = restate(fx["cams"], fx["pts"], fx["K"], fx["fi"][:0], fx["pi"][:0], fx["obs"][:0], np.zeros(len(fx["pts"]) + 1), **PLANTED_TESTS)
    assert none["n_obs"] == 0 and none["n_points"] == 0 and (none["pt_flags"] == PT_SHORT).all()
    pr, _ = outlier_problem(10, 400, 5, 0.05, 2, at_truth=True)
    a = (pr["cams"], pr["pts"], pr["K"], pr["fi"], pr["pi"], pr["obs_clean"], pr["pt_ptr"])
    kept = restate(*a, max_reproj_px=6.0)
    assert kept["n_obs"] == pr["fi"].size and kept["n_points"] == 400 and kept["removed_obs"] == 0
    dropped = restate(*a, max_reproj_px=0.0)
    assert dropped["n_obs"] == 0 and dropped["n_points"] == 0 and dropped["removed_obs"] == pr["fi"].size
    assert (dropped["pt_flags"] == PT_SHORT).all()
    lonely = restate(*a, min_views=6)      # every observation passes, every point is short: all orphans
    assert lonely["removed_obs"] == 0 and (lonely["obs_flags"] == OBS_ORPHAN).all() and lonely["n_obs"] == 0


def test_the_loop_keeps_its_books():
    pr, planted = outlier_problem(8, 60, 5, 0.05, 4)
    out = cpu_refine(pr, (12.0, 5.0), rounds=4, min_views=3)
    rounds = out["rounds"]
    assert len(rounds) >= 2 and rounds[0]["removed_obs"] > 0
    fi0, pi0, obs0 = pr["fi"], pr["pi"], pr["obs"]
    # the maps compose into the first problem's rows, and the outputs are point-major
    assert np.array_equal(out["obs"], obs0[out["obs_map"]]) and np.array_equal(out["fi"], fi0[out["obs_map"]])
    assert np.array_equal(out["point_map"][out["pi"]], pi0[out["obs_map"]])
    assert (np.diff(out["pi"]) >= 0).all() and (np.diff(out["obs_map"]) > 0).all() and (np.diff(out["point_map"]) > 0).all()
    n_o, n_p = fi0.size, 60
    for k, row in enumerate(rounds):
        assert row["n_obs"] == n_o - row["removed_obs"] and row["n_points"] == n_p - row["removed_points"]
        n_o, n_p = row["n_obs"], row["n_points"]
        solved = row["removed_obs"] > 0 or row["removed_points"] > 0
        assert solved == (row["cost_in"] is not None)
        if solved:
            # cost_in is the cost of the compacted problem at the previous cameras and the surviving points
            cams, pts, fi, pi, obs = row["inputs"]
            keep = row["filter"]["obs_flags"] == 0
            r = bo.point_fun(np.hstack([cams.ravel(), pts.ravel()]), pr["K"], 8, len(pts), fi, pi, obs).reshape(-1, 2)[keep]
            assert abs(row["cost_in"] - 0.5 * np.sum(r ** 2)) <= 1e-9 * row["cost_in"]
            assert row["cost_out"] <= row["cost_in"] and row["nfev"] >= 1
        else:
            assert k == len(rounds) - 1 and row["nfev"] == 0      # the loop stops when nothing is flagged
    assert len(rounds) == 4 or not (rounds[-1]["removed_obs"] or rounds[-1]["removed_points"])
    assert out["obs_map"].size == rounds[-1]["n_obs"] and out["point_map"].size == rounds[-1]["n_points"]
    assert np.array_equal(out["obs_flags"], rounds[0]["filter"]["obs_flags"])


def test_the_end_to_end_fixture_meets_its_caps_on_the_cpu():
    """What tests/test_filter_observations_gpu.py asks of the HIP path, asked of SciPy + NumPy first."""
    pr, planted = outlier_problem(**E2E)
    out = cpu_refine(pr, **E2E_REFINE)
    clean = dict(pr, obs=pr["obs_clean"])
    ref = bo.adjust_points(clean["ext"], pr["K"], pr["pts0"], clean["obs"], pr["fi"], pr["pi"], return_result=True)[2]
    left = planted[out["obs_map"]].sum()
    lost = (~planted).sum() - (~planted[out["obs_map"]]).sum()
    r_ref, r_out = rms(float(ref.cost), planted.size), rms(out["cost"], out["obs_map"].size)
    print(f"cpu loop: {len(out['rounds'])} rounds, planted left {left} of {planted.sum()}, clean lost {lost} of {(~planted).sum()}, "
          f"rms {r_out:.4f} against {r_ref:.4f} outlier-free")
    assert left == 0
    assert lost <= 0.05 * (~planted).sum()
    assert r_out <= 1.5 * r_ref
