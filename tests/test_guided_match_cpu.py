"""CPU: a NumPy restatement of mm_guided_match (include/meatmodeler.h), the fixtures of the GPU test and the conditions it
relies on.

The restatement follows the header step by step -- the two distances operation by operation, the order test on the seeds, the
used marks, the gated 2-NN with ties to the lower index, the proposal rule, both one-to-one rules, the merge by query -- on
dense [n_q, n_t] tables.  tests/test_guided_match_gpu.py imports it and asserts equality on every output.

Fixture A (realistic gate, tau = 2): two views of 200 scene points (f = 1400, 1920 x 1080, 0.3 px noise), train descriptors
20 bits off their query's; for 60 of the points a DECOY key point at a random place in the train image whose descriptor is 24
bits off the same query -- the global ratio test (20 < 0.75 * 24 fails) loses exactly those; 60 random clutter key points per
image; both tables shuffled; cap = 320.  Seeds: the ratio-0.75 matches that are inliers of the true F at 2 px.
Fixture B (dense gate, tau = 40): the same tables, every second ratio match as seed; with (ratio, max_dist) = (1, 256) the two
one-to-one rules give different sets.
Fixture P: the same construction over a planar scene with its true H (kind 1); its dense gate is a disc of 300 px.

A gate decision must not hinge on rounding: f64 rounding with coordinates below 2^11 px amplifies to about 1e-9 relative, the
fixtures keep every (query, train) combination more than 1e-6 relative from tau^2 (asserted below), so a gate disagreement
between the kernel and this file is a bug.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

SKIPPED, UNORDERED, MALFORMED = 1, 2, 8      # MM_GUIDED_*
CAP = 320
SHIFT = 22
BIG = np.int64(1) << 40
POP = np.array([bin(v).count("1") for v in range(256)], np.int64)
DEFAULTS = dict(threshold_px=2.0, ratio=0.8, max_dist=64, cross_check=1)


# ------------------------------------------------------------------------------------------------ the restatement

def sampson_all(F, xq, xt):
    """d^2 [n_q, n_t] of F [9] between every query xq [n_q, 2] and every train xt [n_t, 2] (f64)."""
    x, y = xq[:, 0][:, None], xq[:, 1][:, None]
    xp, yp = xt[:, 0][None, :], xt[:, 1][None, :]
    with np.errstate(all="ignore"):
        fx0 = F[0] * x + F[1] * y + F[2]
        fx1 = F[3] * x + F[4] * y + F[5]
        fx2 = F[6] * x + F[7] * y + F[8]
        ft0 = F[0] * xp + F[3] * yp + F[6]
        ft1 = F[1] * xp + F[4] * yp + F[7]
        e = xp * fx0 + yp * fx1 + fx2
        return e * e / (fx0 * fx0 + fx1 * fx1 + ft0 * ft0 + ft1 * ft1)


def adjugate(H):
    return np.array([H[4] * H[8] - H[5] * H[7], H[2] * H[7] - H[1] * H[8], H[1] * H[5] - H[2] * H[4],
                     H[5] * H[6] - H[3] * H[8], H[0] * H[8] - H[2] * H[6], H[2] * H[3] - H[0] * H[5],
                     H[3] * H[7] - H[4] * H[6], H[1] * H[6] - H[0] * H[7], H[0] * H[4] - H[1] * H[3]])


def transfer_all(H, xq, xt):
    """symmetric transfer d^2 [n_q, n_t] of H [9]."""
    A = adjugate(H)
    x, y = xq[:, 0][:, None], xq[:, 1][:, None]
    xp, yp = xt[:, 0][None, :], xt[:, 1][None, :]
    with np.errstate(all="ignore"):
        y0, y1, y2 = (H[0] * x + H[1] * y) + H[2], (H[3] * x + H[4] * y) + H[5], (H[6] * x + H[7] * y) + H[8]
        z0, z1, z2 = (A[0] * xp + A[1] * yp) + A[2], (A[3] * xp + A[4] * yp) + A[5], (A[6] * xp + A[7] * yp) + A[8]
        ex, ey, fx, fy = xp - y0 / y2, yp - y1 / y2, x - z0 / z2, y - z1 / z2
        return ((ex * ex + ey * ey) + (fx * fx + fy * fy)) * 0.5


def distance_all(model, kind, xq, xt):
    xq, xt = np.asarray(xq, np.float64), np.asarray(xt, np.float64)
    return (sampson_all if kind == 0 else transfer_all)(np.asarray(model, np.float64).reshape(9), xq, xt)


def gate_of(d2, tau2):
    with np.errstate(all="ignore"):
        return np.isfinite(d2) & (d2 <= tau2)


def hamming_all(dq, dt):
    return POP[dq[:, None, :] ^ dt[None, :, :]].sum(axis=2)


def two_nearest(keys):
    """(k0, k1) per row of an int64 key table in which BIG marks "no candidate"."""
    if keys.shape[1] == 0:
        return np.full(keys.shape[0], BIG), np.full(keys.shape[0], BIG)
    if keys.shape[1] == 1:
        return keys[:, 0].copy(), np.full(keys.shape[0], BIG)
    part = np.sort(keys, axis=1)[:, :2]
    return part[:, 0], part[:, 1]


def guided_pair(xq, xt, dq, dt, n_q, n_t, seeds, model, kind, cap=CAP, threshold_px=2.0, ratio=0.8, max_dist=64, cross_check=1):
    """One pair.  xq / xt [cap, 2], dq / dt [cap, 32] u8, seeds [m, 2] int -> dict(rows [k, 2], is_new [k], info (4,))."""
    seeds = np.asarray(seeds, np.int64).reshape(-1, 2)
    m = len(seeds)
    n_q, n_t = min(max(int(n_q), 0), cap), min(max(int(n_t), 0), cap)
    model = np.asarray(model, np.float64).reshape(9)
    flags = 0
    if kind not in (0, 1) or not np.isfinite(model).all():
        flags |= SKIPPED
    wf = (seeds >= 0).all(axis=1) & (seeds < cap).all(axis=1)
    if not wf.all():
        flags |= MALFORMED
    if m > 1 and not (seeds[:-1, 0] < seeds[1:, 0]).all():
        flags |= UNORDERED
    if flags & (SKIPPED | UNORDERED):
        return dict(rows=seeds.astype(np.int32), is_new=np.zeros(m, np.uint8), info=(flags, m, 0, 0))
    kept = seeds[wf]
    used_q, used_t = np.zeros(cap, bool), np.zeros(cap, bool)
    used_q[kept[:, 0]] = True
    used_t[kept[:, 1]] = True
    tau2 = float(threshold_px) * float(threshold_px)
    d2 = distance_all(model, kind, xq[:n_q], xt[:n_t])
    G = gate_of(d2, tau2) & ~used_q[:n_q, None] & ~used_t[None, :n_t]
    D = hamming_all(dq[:n_q], dt[:n_t])
    # forward: nearest and second nearest candidate per query, ties to the lower train
    k0, k1 = two_nearest(np.where(G, (D << SHIFT) + np.arange(n_t)[None, :], BIG))
    has = k0 < BIG
    d0, j0, d1 = k0 >> SHIFT, k0 & ((1 << SHIFT) - 1), k1 >> SHIFT
    proposed = has & (d0 <= max_dist) & ((k1 >= BIG) | (d0.astype(np.float64) < float(ratio) * d1.astype(np.float64)))
    prop_i = np.nonzero(proposed)[0]
    new = []
    if cross_check:
        # reverse: the nearest candidate query per train over the same gate, ties to the lower query
        r0, _ = two_nearest(np.where(G.T, (D.T << SHIFT) + np.arange(n_q)[None, :], BIG))
        for i in prop_i:
            if (r0[j0[i]] & ((1 << SHIFT) - 1)) == i:
                new.append((i, j0[i]))
    else:
        best = {}
        for i in prop_i:
            key = (int(d0[i]), int(i))
            if j0[i] not in best or key < best[j0[i]]:
                best[j0[i]] = key
        new = sorted((i, j) for j, (_, i) in best.items())
    rows = [(int(q), int(t), 0) for q, t in kept] + [(int(i), int(j), 1) for i, j in new]
    rows.sort()
    out = np.array(rows, np.int64).reshape(-1, 3)
    return dict(rows=out[:, :2].astype(np.int32), is_new=out[:, 2].astype(np.uint8), info=(flags, len(kept), len(new), len(prop_i)))


def guided_numpy(kp_xy, desc, n, pairs, m, model, kind=None, **kw):
    """The whole call -> (pairs_out [n_pairs, cap, 2] i32 with its -1 tail, m_out, is_new [n_pairs, cap] u8, info [n_pairs, 4])."""
    n_pairs, cap = pairs.shape[0], pairs.shape[1]
    po = np.full((n_pairs, cap, 2), -1, np.int32)
    mo, new, info = np.zeros(n_pairs, np.int32), np.zeros((n_pairs, cap), np.uint8), np.zeros((n_pairs, 4), np.int32)
    for p in range(n_pairs):
        mm = min(max(int(m[p]), 0), cap)
        r = guided_pair(kp_xy[p], kp_xy[p + 1], desc[p], desc[p + 1], n[p], n[p + 1], pairs[p, :mm], model[p],
                        0 if kind is None else int(kind[p]), cap=cap, **kw)
        k = len(r["rows"])
        po[p, :k], new[p, :k], mo[p], info[p] = r["rows"], r["is_new"], k, r["info"]
    return po, mo, new, info


def ratio_matches(dq, dt, ratio):
    """The match stage on its own: (q, t, d0) rows of the queries whose nearest train is under `ratio` times the second."""
    D = hamming_all(dq, dt)
    k0, k1 = two_nearest((D << SHIFT) + np.arange(D.shape[1])[None, :])
    ok = (k0 < BIG) & (k1 < BIG) & ((k0 >> SHIFT).astype(np.float64) < float(ratio) * (k1 >> SHIFT).astype(np.float64))
    q = np.nonzero(ok)[0]
    return np.stack([q, k0[q] & ((1 << SHIFT) - 1), k0[q] >> SHIFT], axis=1)


def lowest_per_train(rows):
    """Of (q, t, d) rows, per train the one with the lowest (d, q); (q, t) in query order."""
    best = {}
    for q, t, d in rows:
        if t not in best or (d, q) < best[t]:
            best[t] = (int(d), int(q))
    return np.array(sorted((q, t) for t, (_, q) in best.items()), np.int32).reshape(-1, 2)


# ------------------------------------------------------------------------------------------------ fixtures

K_SCENE = np.array([[1400.0, 0, 960.0], [0, 1400.0, 540.0], [0, 0, 1]])
W_IMG, H_IMG = 1920.0, 1080.0
N_SCENE, N_DECOY, N_CLUTTER = 200, 60, 60


def rot(yaw, pitch):
    cy, sy, cp, sp = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch)
    return np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])


R_SCENE, T_SCENE = rot(0.06, -0.02), np.array([-0.7, 0.05, 0.12])
PLANE_N, PLANE_D = np.array([0.15, -0.1, 1.0]) / np.linalg.norm([0.15, -0.1, 1.0]), 7.0


def unit(v):
    return v / np.sqrt((v * v).sum())


def true_F():
    tx = np.array([[0, -T_SCENE[2], T_SCENE[1]], [T_SCENE[2], 0, -T_SCENE[0]], [-T_SCENE[1], T_SCENE[0], 0]])
    Ki = np.linalg.inv(K_SCENE)
    return unit((Ki.T @ tx @ R_SCENE @ Ki).reshape(9))


def true_H():
    return unit((K_SCENE @ (R_SCENE + np.outer(T_SCENE, PLANE_N) / PLANE_D) @ np.linalg.inv(K_SCENE)).reshape(9))


def flip(rng, d, bits):
    """copies of the descriptors d [k, 32] with `bits` distinct random bits flipped in each."""
    out = np.unpackbits(d, axis=1)
    for r in range(len(out)):
        out[r, rng.choice(256, bits, replace=False)] ^= 1
    return np.packbits(out, axis=1)


@functools.lru_cache(maxsize=None)
def tables(seed, planar=False):
    """The two shuffled key point tables of one scene -> dict(kp [2, CAP, 2] f32, desc [2, CAP, 32] u8, n (2,), truth [N_SCENE, 2]
    = (query, train) index of every scene point, decoyed [N_DECOY] scene points with a decoy, model [9])."""
    rng = np.random.default_rng(1000 + seed)
    x1, x2 = np.zeros((0, 2)), np.zeros((0, 2))
    Ki = np.linalg.inv(K_SCENE)
    while len(x1) < N_SCENE:
        px = np.stack([rng.uniform(40, W_IMG - 40, 400), rng.uniform(40, H_IMG - 40, 400), np.ones(400)], axis=1)
        ray = px @ Ki.T
        depth = PLANE_D / (ray @ PLANE_N) if planar else rng.uniform(4.0, 12.0, 400)
        X2 = (ray * depth[:, None]) @ R_SCENE.T + T_SCENE
        q = X2 @ K_SCENE.T
        q = q[:, :2] / q[:, 2:]
        ok = (depth > 0) & (X2[:, 2] > 0) & (q[:, 0] > 40) & (q[:, 0] < W_IMG - 40) & (q[:, 1] > 40) & (q[:, 1] < H_IMG - 40)
        x1, x2 = np.concatenate([x1, px[ok, :2]]), np.concatenate([x2, q[ok]])
    x1, x2 = x1[:N_SCENE] + rng.normal(0, 0.3, (N_SCENE, 2)), x2[:N_SCENE] + rng.normal(0, 0.3, (N_SCENE, 2))
    d1 = rng.integers(0, 256, (N_SCENE, 32), dtype=np.uint8)
    d2 = flip(rng, d1, 20)
    decoy_xy = np.stack([rng.uniform(40, W_IMG - 40, N_DECOY), rng.uniform(40, H_IMG - 40, N_DECOY)], axis=1)
    decoy_d = flip(rng, d1[:N_DECOY], 24)
    cl = lambda: (np.stack([rng.uniform(40, W_IMG - 40, N_CLUTTER), rng.uniform(40, H_IMG - 40, N_CLUTTER)], axis=1),
                  rng.integers(0, 256, (N_CLUTTER, 32), dtype=np.uint8))
    (c1, cd1), (c2, cd2) = cl(), cl()
    q_xy, q_d = np.concatenate([x1, c1]), np.concatenate([d1, cd1])
    t_xy, t_d = np.concatenate([x2, decoy_xy, c2]), np.concatenate([d2, decoy_d, cd2])
    pq, pt = rng.permutation(len(q_xy)), rng.permutation(len(t_xy))      # row r of the shuffled table = old row p[r]
    iq, it = np.argsort(pq), np.argsort(pt)
    kp, desc = np.zeros((2, CAP, 2), np.float32), np.zeros((2, CAP, 32), np.uint8)
    kp[0, :len(pq)], desc[0, :len(pq)] = q_xy[pq], q_d[pq]
    kp[1, :len(pt)], desc[1, :len(pt)] = t_xy[pt], t_d[pt]
    truth = np.stack([iq[:N_SCENE], it[:N_SCENE]], axis=1)
    return dict(kp=kp, desc=desc, n=np.array([len(pq), len(pt)], np.int32), truth=truth, decoyed=np.arange(N_DECOY),
                model=true_H() if planar else true_F(), kind=1 if planar else 0)


def seeds_of(t, which):
    """Seeds of the fixtures: "A" the ratio-0.75 matches within 2 px of the true model, "B" every second ratio match,
    "none"; [m, 2] in query order."""
    if which == "none":
        return np.zeros((0, 2), np.int32)
    nq, nt = t["n"]
    r = ratio_matches(t["desc"][0, :nq], t["desc"][1, :nt], 0.75)
    if which == "B":
        return r[::2, :2].astype(np.int32)
    d2 = distance_all(t["model"], t["kind"], t["kp"][0], t["kp"][1])
    return r[gate_of(d2[r[:, 0], r[:, 1]], 4.0), :2].astype(np.int32)


def run_fixture(t, which, **kw):
    prm = dict(DEFAULTS)
    prm.update(kw)
    return guided_pair(t["kp"][0], t["kp"][1], t["desc"][0], t["desc"][1], t["n"][0], t["n"][1], seeds_of(t, which), t["model"],
                       t["kind"], **prm)


def relative_gap(t, tau):
    """the smallest |d^2 - tau^2| / tau^2 over every (query, train) combination of the two tables."""
    d2 = distance_all(t["model"], t["kind"], t["kp"][0, :t["n"][0]], t["kp"][1, :t["n"][1]])
    return float(np.nanmin(np.abs(d2 - tau * tau)) / (tau * tau))


def reversed_tables(t):
    """The same scene with the images exchanged: train becomes query; the model of that direction (F^T, adj(H))."""
    M = np.asarray(t["model"]).reshape(3, 3)
    back = M.T.reshape(9) if t["kind"] == 0 else unit(adjugate(M.reshape(9)))
    return dict(kp=t["kp"][::-1].copy(), desc=t["desc"][::-1].copy(), n=t["n"][::-1].copy(), truth=t["truth"][:, ::-1].copy(),
                decoyed=t["decoyed"], model=back, kind=t["kind"])


def reversed_seeds(seeds):
    s = np.asarray(seeds)[:, ::-1]
    return s[np.argsort(s[:, 0], kind="stable")].astype(np.int32)


# the scenes the GPU test runs: (seed, planar); every (fixture, tau) below keeps the margin
GPU_SEEDS = ((0, False), (1, False), (0, True))
TAUS = (2.0, 40.0, 300.0)
DENSE_TAU = {False: 40.0, True: 300.0}      # tens of candidates per query: a band of 40 px around a line, a disc of 300 px
MARGIN = 1e-6


# ------------------------------------------------------------------------------------------------ tests

@pytest.mark.parametrize("seed,planar", GPU_SEEDS)
def test_no_gate_decision_hinges_on_rounding(seed, planar):
    t = tables(seed, planar)
    for tt in (t, reversed_tables(t)):
        for tau in TAUS:
            gap = relative_gap(tt, tau)
            print(f"seed {seed} planar {planar} tau {tau}: smallest relative gap {gap:.3g}")
            assert gap > MARGIN


@pytest.mark.parametrize("seed,planar", GPU_SEEDS)
def test_fixture_A_recovers_the_decoyed_points(seed, planar):
    t = tables(seed, planar)
    seeds = seeds_of(t, "A")
    r = run_fixture(t, "A")
    new = r["rows"][r["is_new"] == 1]
    truth = {(int(q), int(j)) for q, j in t["truth"]}
    wrong = [tuple(row) for row in new.tolist() if tuple(row) not in truth]
    lost = {(int(q), int(j)) for q, j in t["truth"][t["decoyed"]]}
    recovered = sum(1 for row in new.tolist() if tuple(row) in lost)
    print(f"seed {seed} planar {planar}: {len(seeds)} seeds, {len(new)} new, {recovered} of {N_DECOY} decoyed recovered, "
          f"{len(wrong)} wrong")
    assert 100 <= len(seeds) <= N_SCENE - N_DECOY + 5
    assert recovered >= 58 and not wrong
    assert r["info"] == (0, len(seeds), len(new), r["info"][3]) and r["info"][3] >= len(new)


def properties(t, seeds, r, prm):
    rows, is_new = r["rows"], r["is_new"]
    old = rows[is_new == 0]
    assert np.array_equal(old, seeds)                                   # a superset of the seeds, each as it came
    assert (np.diff(rows[:, 0]) > 0).all()                              # strictly increasing query order
    new = rows[is_new == 1]
    assert len(set(new[:, 1].tolist())) == len(new)                     # no train gains two new rows
    assert not set(new[:, 0].tolist()) & set(seeds[:, 0].tolist()) and not set(new[:, 1].tolist()) & set(seeds[:, 1].tolist())
    d2 = distance_all(t["model"], t["kind"], t["kp"][0], t["kp"][1])
    D = hamming_all(t["desc"][0], t["desc"][1])
    assert gate_of(d2[new[:, 0], new[:, 1]], prm["threshold_px"] ** 2).all()
    assert (D[new[:, 0], new[:, 1]] <= prm["max_dist"]).all()
    assert (new[:, 0] < t["n"][0]).all() and (new[:, 1] < t["n"][1]).all()


@pytest.mark.parametrize("seed,planar", GPU_SEEDS)
def test_output_properties_on_every_fixture(seed, planar):
    t = tables(seed, planar)
    for which, tau in (("A", 2.0), ("B", 40.0), ("B", DENSE_TAU[planar])):
        for ratio, max_dist in ((0.8, 64), (1.0, 256)):
            for cc in (0, 1):
                prm = dict(threshold_px=tau, ratio=ratio, max_dist=max_dist, cross_check=cc)
                properties(t, seeds_of(t, which), run_fixture(t, which, **prm), prm)


@pytest.mark.parametrize("seed,planar", GPU_SEEDS)
def test_fixture_B_exercises_both_one_to_one_rules(seed, planar):
    t = tables(seed, planar)
    tau = DENSE_TAU[planar]
    a = run_fixture(t, "B", threshold_px=tau, ratio=1.0, max_dist=256, cross_check=0)
    b = run_fixture(t, "B", threshold_px=tau, ratio=1.0, max_dist=256, cross_check=1)
    d2 = distance_all(t["model"], t["kind"], t["kp"][0, :t["n"][0]], t["kp"][1, :t["n"][1]])
    print(f"seed {seed} planar {planar}: {gate_of(d2, tau * tau).sum() / t['n'][0]:.1f} candidates per query, "
          f"{a['info'][2]} / {b['info'][2]} new rows without / with the cross check, {a['info'][3]} proposals")
    assert a["info"][2] > b["info"][2] > 50
    assert a["info"][3] > a["info"][2]      # some train was proposed twice: the lowest (d, i) rule decided something
    assert not np.array_equal(a["rows"], b["rows"])


@pytest.mark.parametrize("seed,planar", GPU_SEEDS)
def test_without_gate_and_seeds_it_is_the_match_stage_resolved_per_train(seed, planar):
    t = tables(seed, planar)
    nq, nt = t["n"]
    for ratio in (0.75, 0.8, 1.0):
        r = run_fixture(t, "none", threshold_px=math.inf, ratio=ratio, max_dist=256, cross_check=0)
        want = lowest_per_train(ratio_matches(t["desc"][0, :nq], t["desc"][1, :nt], ratio))
        assert np.array_equal(r["rows"], want) and r["is_new"].all()


def test_pass_through_and_malformed_rows():
    t = tables(0)
    seeds = seeds_of(t, "A")
    args = (t["kp"][0], t["kp"][1], t["desc"][0], t["desc"][1], t["n"][0], t["n"][1])
    for model, kind in ((t["model"], -1), (t["model"], 2), (np.where(np.arange(9) == 4, np.nan, t["model"]), 0)):
        r = guided_pair(*args, seeds, model, kind)
        assert r["info"] == (SKIPPED, len(seeds), 0, 0) and np.array_equal(r["rows"], seeds) and not r["is_new"].any()
    swapped = seeds.copy()
    swapped[[3, 4]] = swapped[[4, 3]]
    r = guided_pair(*args, swapped, t["model"], 0)
    assert r["info"] == (UNORDERED, len(seeds), 0, 0) and np.array_equal(r["rows"], swapped)
    bad = seeds.copy()
    bad[5, 1] = CAP                              # a train index outside the table: dropped, its query is free again
    r = guided_pair(*args, bad, t["model"], 0)
    assert r["info"][0] == MALFORMED and r["info"][1] == len(seeds) - 1
    assert np.array_equal(r["rows"][r["is_new"] == 0], np.delete(seeds, 5, axis=0))
    row = r["rows"][r["rows"][:, 0] == seeds[5, 0]]
    assert len(row) == 1 and tuple(row[0]) == tuple(seeds[5])      # ... and the search finds the same match again


def test_all_used_adds_nothing():
    t = tables(0)
    n = int(t["n"][0])
    seeds = np.stack([np.arange(n), np.arange(n)], axis=1).astype(np.int32)
    r = guided_pair(t["kp"][0], t["kp"][1], t["desc"][0], t["desc"][1], t["n"][0], t["n"][1], seeds, t["model"], 0, threshold_px=math.inf,
                    ratio=1.0, max_dist=256)
    assert r["info"] == (0, n, 0, 0) and np.array_equal(r["rows"], seeds)


# ---- through the loaded library, without a GPU --------------------------------------------------------------------------

def test_library_table_has_the_guided_symbols():
    from meatmodeler_amd import _lib, ops
    assert {"mm_guided_workspace_bytes", "mm_guided_match"} <= set(_lib.SIGNATURES)
    assert C.sizeof(_lib.GuidedParams) == 24
    assert (ops.GUIDED_SKIPPED, ops.GUIDED_UNORDERED, ops.GUIDED_MALFORMED) == (SKIPPED, UNORDERED, MALFORMED)


def test_argument_errors_return_before_any_device_call():
    """No context and made-up addresses: a bad call must come back from the checks, not from the device."""
    from meatmodeler_amd import _lib
    lib = _lib.lib
    ERR_ARG, ERR_WORKSPACE = -1, -3
    need = lib.mm_guided_workspace_bytes(2, CAP)
    distinct = tuple(64 * (k + 1) for k in range(13))
    # kp_xy, desc, n, pairs, m, model, kind | pairs_out, m_out, is_new, info, ws

    def call(prm, ws_bytes=need, ptrs=distinct, n_pairs=2, cap=CAP):
        a = [C.c_void_p(v) if v else None for v in ptrs]
        return lib.mm_guided_match(None, a[0], a[1], a[2], a[3], a[4], a[5], a[6], n_pairs, cap,
                                   C.byref(prm) if prm is not None else None, a[7], a[8], a[9], a[10], a[11], ws_bytes)

    def prm(**kw):
        v = dict(DEFAULTS)
        v.update(kw)
        return _lib.GuidedParams(**v)

    for bad in (prm(threshold_px=-1.0), prm(threshold_px=math.nan), prm(ratio=math.nan), prm(ratio=-0.5), prm(max_dist=-1),
                prm(max_dist=257), prm(cross_check=2), prm(cross_check=-1)):
        assert call(bad) == ERR_ARG
    assert call(prm(), ws_bytes=need - 1) == ERR_WORKSPACE and call(prm(), ws_bytes=0) == ERR_WORKSPACE
    for k in range(12):      # each null pointer; kind alone may be null
        got = call(prm(), ptrs=tuple(0 if i == k else v for i, v in enumerate(distinct)))
        assert got == ERR_ARG, k      # (kind = NULL: a good call without a context, the same code)
    assert call(None) == ERR_ARG
    assert call(prm(), n_pairs=-1) == ERR_ARG and call(prm(), cap=0) == ERR_ARG and call(prm(), cap=(1 << 22) + 1) == ERR_ARG
    assert call(prm(), ptrs=distinct[:7] + (distinct[3],) + distinct[8:]) == ERR_ARG      # pairs_out aliases pairs
    assert call(prm(threshold_px=math.inf, ratio=math.inf, max_dist=256, cross_check=0)) == ERR_ARG      # good, but no context
    assert lib.mm_guided_match(None, *([None] * 7), 0, CAP, C.byref(prm()), *([None] * 5), 0) == ERR_ARG  # n_pairs 0, no context


def test_guided_option_validation():
    from meatmodeler_amd import pipeline
    assert pipeline.guided_options(None) is None and pipeline.guided_options({}) == {}
    assert pipeline.guided_options(dict(threshold_px=1.5, ratio=0.7, max_dist=48, cross_check=False))["max_dist"] == 48
    for bad in (dict(tau=2.0), dict(kind=None), dict(ctx=None), dict(model=None)):
        with pytest.raises(ValueError):
            pipeline.guided_options(bad)
    with pytest.raises(ValueError):
        pipeline.guided_options([("ratio", 0.8)])
