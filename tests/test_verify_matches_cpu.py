"""CPU: a NumPy restatement of mm_verify_matches (include/meatmodeler.h) and the conditions the GPU test relies on.

The restatement follows the header's definition step by step -- Hartley normalisation, the integer sampling, 8-point
hypotheses, MSAC score, refit rounds, flags -- and runs two numerically different ways: null vectors and the rank-2 step by
numpy.linalg.svd ("svd"), or by eigh of A^T A and the F - (F v3) v3^T form ("eigh").  Both must choose the same hypothesis,
the same mask and the same F to 1e-12.  tests/test_verify_matches_gpu.py imports the helpers of this module.

Measured here with the header's sampling, 160 inliers + 96 outliers, n_hyp = 256, tau = 2, seeds 0 .. 5: best_h and the masks
identical in both routes, |F0 - F1| <= 1.7e-14, 151 - 160 of 160 true inliers kept (160 for five of the seeds), 1 - 3 of 96
outliers kept (pixels that happen to lie near their epipolar line: no epipolar test can reject those).  Seed 5 is the odd one:
151 inliers and a match 0.002 px from the threshold -- which is why the fixtures of the GPU test are chosen by the conditions
asserted below (recall, kept outliers, no match within 0.02 px of tau) and not taken as they come.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from oracle.geom_oracle import pcg

TOO_FEW, NO_MODEL, WEAK, MALFORMED = 1, 2, 4, 8      # MM_VERIFY_*
CAP = 320
M32 = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------ sampling

def sample(seed, pair_index, n_hyp, m):
    """picks [n_hyp, 8] and ok [n_hyp] of the pair with global index pair_index."""
    h = np.arange(n_hyp, dtype=np.uint64)
    base = pcg((pcg((np.uint64(seed & M32) + pcg(np.uint64(pair_index & M32))) & np.uint64(M32)) + h) & np.uint64(M32))
    picks = np.zeros((n_hyp, 8), np.int64)
    ok = np.ones(n_hyp, bool)
    for k in range(8):
        chosen = np.full(n_hyp, -1, np.int64)
        for a in range(8):
            i = ((pcg((base + np.uint64(8 * k + a)) & np.uint64(M32)) * np.uint64(m)) >> np.uint64(32)).astype(np.int64)
            dup = (picks[:, :k] == i[:, None]).any(axis=1)
            chosen = np.where((chosen < 0) & ~dup, i, chosen)
        ok &= chosen >= 0
        picks[:, k] = np.maximum(chosen, 0)
    return picks, ok


def pcg_int(v):
    """The same function on Python integers (the independent restatement of the sampling uses this one)."""
    s = (v * 747796405 + 2891336453) & M32
    w = (((s >> ((s >> 28) + 4)) ^ s) * 277803737) & M32
    return ((w >> 22) ^ w) & M32


def sample_int(seed, pair_index, h, m):
    """Eight distinct indices of hypothesis h, or None after eight collisions in a row."""
    base = pcg_int((pcg_int((seed + pcg_int(pair_index & M32)) & M32) + h) & M32)
    picks = []
    for k in range(8):
        for a in range(8):
            i = (pcg_int((base + 8 * k + a) & M32) * m) >> 32
            if i not in picks:
                picks.append(i)
                break
        else:
            return None
    return picks


# ------------------------------------------------------------------------------------------------ the restatement

def sampson(F, x, xp):
    """d^2 [..., n] of F [..., 9] over matches x, xp [n, 2]."""
    F = np.asarray(F, float)[..., None, :]
    fx0 = F[..., 0] * x[:, 0] + F[..., 1] * x[:, 1] + F[..., 2]
    fx1 = F[..., 3] * x[:, 0] + F[..., 4] * x[:, 1] + F[..., 5]
    fx2 = F[..., 6] * x[:, 0] + F[..., 7] * x[:, 1] + F[..., 8]
    ft0 = F[..., 0] * xp[:, 0] + F[..., 3] * xp[:, 1] + F[..., 6]
    ft1 = F[..., 1] * xp[:, 0] + F[..., 4] * xp[:, 1] + F[..., 7]
    e = xp[:, 0] * fx0 + xp[:, 1] * fx1 + fx2
    with np.errstate(all="ignore"):
        return e * e / (fx0 * fx0 + fx1 * fx1 + ft0 * ft0 + ft1 * ft1)


def inliers(d2, tau2):
    with np.errstate(all="ignore"):
        return np.isfinite(d2) & (d2 <= tau2)


def msac(F, x, xp, tau2):
    d2 = sampson(F, x, xp)
    inl = inliers(d2, tau2)
    return np.where(inl, d2, tau2).sum(axis=-1), inl


def hartley(x):
    """(centroid, s) over the rows of x."""
    with np.errstate(all="ignore"):
        c = x.sum(axis=0) / len(x)
        return c, math.sqrt(2.0) / (np.sqrt(((x - c) ** 2).sum(axis=1)).sum() / len(x))


def rows_of(x, xp):
    one = np.ones(x.shape[:-1])
    return np.stack([xp[..., 0] * x[..., 0], xp[..., 0] * x[..., 1], xp[..., 0], xp[..., 1] * x[..., 0],
                     xp[..., 1] * x[..., 1], xp[..., 1], x[..., 0], x[..., 1], one], axis=-1)


def null_vector(A, route):
    """Unit right null vector(s) of A [..., n, 9]."""
    if route == "svd":
        return np.linalg.svd(A, full_matrices=True)[2][..., -1, :]
    return np.linalg.eigh(np.swapaxes(A, -1, -2) @ A)[1][..., :, 0]


def rank2(Fh, route):
    """Fh [..., 3, 3] -> its rank-2 neighbour."""
    if route == "svd":
        U, S, Vt = np.linalg.svd(Fh)
        S = S.copy()
        S[..., 2] = 0.0
        return (U * S[..., None, :]) @ Vt
    v3 = np.linalg.eigh(np.swapaxes(Fh, -1, -2) @ Fh)[1][..., :, 0]
    return Fh - (Fh @ v3[..., None]) * v3[..., None, :]


def finish(f, c, s, c2, s2, route):
    """f [..., 9] in normalised coordinates -> rank 2, F = T'^T F^ T, unit norm [..., 9]; valid [...]."""
    Fh = rank2(f.reshape(f.shape[:-1] + (3, 3)), route)
    T = np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1]])
    T2 = np.array([[s2, 0, -s2 * c2[0]], [0, s2, -s2 * c2[1]], [0, 0, 1]])
    with np.errstate(all="ignore"):
        F = (T2.T @ Fh @ T).reshape(f.shape)
        F = F / np.sqrt((F * F).sum(axis=-1, keepdims=True))
    return F, np.isfinite(F).all(axis=-1)


def verify_pair(x, xp, wf, pair_index, n_hyp=256, threshold_px=2.0, min_matches=16, min_inliers=16, refit_iters=2, seed=0,
                route="svd"):
    """One pair: x, xp [m, 2] f64 (rows of malformed matches NaN), wf [m] bool
    -> dict(flags, n_inliers, best_h, n_valid, F [9], cost, mask [m] -- the inliers of the final F)."""
    mm = len(x)
    tau2 = float(threshold_px) ** 2
    nan9 = np.full(9, np.nan)
    out = dict(flags=0 if wf.all() else MALFORMED, n_inliers=0, best_h=-1, n_valid=0, F=nan9, cost=np.nan,
               mask=np.zeros(mm, bool))
    if mm < max(int(min_matches), 16):
        out["flags"] |= TOO_FEW
        return out
    picks, ok = sample(seed, pair_index, n_hyp, mm)
    ok &= wf[picks].all(axis=1)
    if wf.any():
        (c, s), (c2, s2) = hartley(x[wf]), hartley(xp[wf])
        ok &= np.isfinite(s) and np.isfinite(s2)
    else:
        ok[:] = False
    cost_h = np.full(n_hyp, np.inf)
    Fh = np.full((n_hyp, 9), np.nan)
    if ok.any():
        hs = np.nonzero(ok)[0]
        A = rows_of(s * (x[picks[hs]] - c), s2 * (xp[picks[hs]] - c2))      # [H, 8, 9]
        F, valid = finish(null_vector(A, route), c, s, c2, s2, route)
        Fh[hs[valid]] = F[valid]
        cost_h[hs[valid]] = msac(F[valid], x, xp, tau2)[0]
    out["n_valid"] = int(np.isfinite(Fh[:, 0]).sum())
    if not np.isfinite(cost_h).any():
        out["flags"] |= NO_MODEL
        return out
    best = int(np.argmin(np.where(np.isfinite(cost_h), cost_h, np.inf)))      # (first minimum: ties to the lowest h)
    F = Fh[best]
    cost, mask = msac(F, x, xp, tau2)
    for _ in range(int(refit_iters)):
        if mask.sum() < 8:
            break
        (ci, si), (ci2, si2) = hartley(x[mask]), hartley(xp[mask])
        with np.errstate(all="ignore"):
            A = rows_of(si * (x[mask] - ci), si2 * (xp[mask] - ci2))
        if not np.isfinite(A).all():
            continue
        Fn, okF = finish(null_vector(A, route), ci, si, ci2, si2, route)
        cn, mn = msac(Fn, x, xp, tau2)
        if okF and np.isfinite(cn) and cn < cost:
            F, cost, mask = Fn, cn, mn
    out.update(best_h=best, F=F, cost=float(cost), mask=mask, n_inliers=int(mask.sum()))
    if out["n_inliers"] < int(min_inliers):
        out["flags"] |= WEAK
    return out


def verify_numpy(kp_xy, pairs, m, pair_base=0, on_fail=0, **kw):
    """The whole call -> (list of verify_pair dicts, each with `kept` [k, 2] = the rows mm_verify_matches writes)."""
    cap = kp_xy.shape[1]
    res = []
    for p in range(pairs.shape[0]):
        mm = int(np.clip(m[p], 0, cap))
        rows = pairs[p, :mm]
        wf = ((rows >= 0) & (rows < cap)).all(axis=1)
        x = np.full((mm, 2), np.nan)
        xp = np.full((mm, 2), np.nan)
        x[wf] = kp_xy[p, rows[wf, 0]]
        xp[wf] = kp_xy[p + 1, rows[wf, 1]]
        r = verify_pair(x, xp, wf, pair_base + p, **kw)
        if r["flags"] & (TOO_FEW | NO_MODEL | WEAK):
            r["kept"] = rows[:0] if on_fail else rows
        else:
            r["kept"] = rows[r["mask"]]
        res.append(r)
    return res


def sign_gap(Fa, Fb):
    """max |Fa -+ Fb|: F is defined up to sign."""
    return min(np.abs(Fa - Fb).max(), np.abs(Fa + Fb).max())


# ------------------------------------------------------------------------------------------------ fixtures

K_SCENE = np.array([[500.0, 0, 320.0], [0, 500.0, 240.0], [0, 0, 1]])


def scene_cameras():
    a = 0.12
    R = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    return R, np.array([-0.8, 0.05, 0.1])


def true_F():
    """x'^T F x = 0 of the scene's two cameras, unit norm."""
    R, t = scene_cameras()
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ki = np.linalg.inv(K_SCENE)
    F = Ki.T @ tx @ R @ Ki
    return (F / np.linalg.norm(F)).ravel()


def two_view_scene(seed, n_in, n_out):
    """(x [n, 2] f32, x' [n, 2] f32, truth [n] bool): n_in noisy projections of points seen by both cameras and n_out pairs
    of independent uniform pixels, shuffled."""
    rng = np.random.default_rng(seed)
    R, t = scene_cameras()
    xs, xps = np.zeros((0, 2)), np.zeros((0, 2))
    while len(xs) < n_in:
        X = rng.uniform([-2, -1.5, 4], [2, 1.5, 9], size=(2 * n_in + 8, 3))
        a = X @ K_SCENE.T
        b = (X @ R.T + t) @ K_SCENE.T
        a, b = a[:, :2] / a[:, 2:], b[:, :2] / b[:, 2:]
        vis = ((a >= 0) & (a < [640, 480]) & (b >= 0) & (b < [640, 480])).all(axis=1)
        xs, xps = np.vstack([xs, a[vis]]), np.vstack([xps, b[vis]])
    xs = xs[:n_in] + rng.normal(0, 0.25, (n_in, 2))
    xps = xps[:n_in] + rng.normal(0, 0.25, (n_in, 2))
    xs = np.vstack([xs, rng.uniform([0, 0], [640, 480], (n_out, 2))])
    xps = np.vstack([xps, rng.uniform([0, 0], [640, 480], (n_out, 2))])
    truth = np.arange(n_in + n_out) < n_in
    order = rng.permutation(n_in + n_out)
    return xs[order].astype(np.float32), xps[order].astype(np.float32), truth[order]


def pack(scenes, cap=CAP, seed=99):
    """Consecutive pairs out of two-view scenes: pair p's query points sit at the end of frame p's table, its train points at
    the start of frame p + 1's, both in a shuffled order (so a match's indices are not its position).
    -> kp_xy [n+1, cap, 2] f32, pairs [n, cap, 2] i32 (rows beyond m: -1), m [n] i32."""
    rng = np.random.default_rng(seed)
    n = len(scenes)
    kp = rng.uniform(0, 400, (n + 1, cap, 2)).astype(np.float32)
    pairs = np.full((n, cap, 2), -1, np.int32)
    m = np.zeros(n, np.int32)
    for p, (x, xp, _) in enumerate(scenes):
        k = len(x)
        assert k <= cap and (p + 1 == n or k + len(scenes[p + 1][0]) <= cap)
        pq, pt = rng.permutation(k), rng.permutation(k)
        kp[p, cap - k + pq] = x
        kp[p + 1, pt] = xp
        pairs[p, :k, 0] = cap - k + pq
        pairs[p, :k, 1] = pt
        m[p] = k
    return kp, pairs, m


FIVE = ((160, 96), (64, 0), (40, 24), (17, 0), (15, 0))      # the five-pair call of the GPU test
FIVE_SEEDS = (0, 1, 2, 3, 4)
FIVE_KW = dict(n_hyp=256, threshold_px=2.0, seed=7)


@functools.lru_cache(maxsize=None)
def five_pairs():
    scenes = [two_view_scene(s, a, b) for s, (a, b) in zip(FIVE_SEEDS, FIVE)]
    return (scenes,) + pack(scenes)


@functools.lru_cache(maxsize=None)
def five_pairs_result(route="svd"):
    _, kp, pairs, m = five_pairs()
    return verify_numpy(kp, pairs, m, route=route, **FIVE_KW)


def boundary_scene(m):
    """The single-pair fixture of the m-boundary tests: a quarter outliers from 63 matches on."""
    n_out = m // 4 if m >= 63 else 0
    return two_view_scene(100 + m, m - n_out, n_out)


BOUNDARY_M = (0, 15, 16, 17, 63, 64, 65, 257, CAP)
BOUNDARY_HYP = (1, 63, 64, 65, 256)


@functools.lru_cache(maxsize=None)
def weak_fixture():
    """64 pairs of independent uniform pixels: whatever F wins explains few of them."""
    return pack([two_view_scene(WEAK_SEED, 0, 64)])


@functools.lru_cache(maxsize=None)
def malformed_fixture():
    """Pair 2 of the five-pair call (pair_base = 2) with match 3's query index -1 and match 10's train index cap."""
    _, kp, pairs, m = five_pairs()
    bad = pairs[2:3].copy()
    bad[0, 3, 0] = -1
    bad[0, 10, 1] = CAP
    return kp[2:4], bad, m[2:3]


WEAK_SEED = 200


def margin(r, x, xp, tau):
    """min | d - tau | over the matches, d the Sampson distance under the result's F (inf without a model)."""
    if not np.isfinite(r["F"]).all() or not len(x):
        return np.inf
    d = np.sqrt(sampson(r["F"], x.astype(float), xp.astype(float)))
    return np.abs(d[np.isfinite(d)] - tau).min()


# ------------------------------------------------------------------------------------------------ tests

def test_pcg_is_pinned_and_both_statements_of_the_sampling_agree():
    assert [pcg_int(v) for v in (0, 1, 0xFFFFFFFF)] == PCG_PINNED
    assert [int(v) for v in pcg(np.array([0, 1, 0xFFFFFFFF], np.uint64))] == PCG_PINNED
    for m in (16, 17, 64, 1000, 4000):
        picks, ok = sample(5, 3, 300, m)
        assert ok.all() or m < 64      # (eight collisions in a row do happen at 16: (7/16)^8 per pick at the worst)
        for h in range(300):
            mine = sample_int(5, 3, h, m)
            assert (mine is not None) == bool(ok[h])
            if mine is not None:
                assert mine == list(picks[h]) and len(set(mine)) == 8 and 0 <= min(mine) and max(mine) < m


def test_sampling_gives_up_after_eight_collisions():
    picks, ok = sample(5, 3, 300, 7)      # eight distinct indices below 7 do not exist
    assert not ok.any() and all(sample_int(5, 3, h, 7) is None for h in range(300))
    picks, ok = sample(5, 3, 300, 9)      # below 9 they do, but eight tries often miss the last free index
    assert ok.any() and not ok.all()
    for h in range(300):
        mine = sample_int(5, 3, h, 9)
        assert (mine is not None) == bool(ok[h])
        if mine is not None:
            assert mine == list(picks[h]) and len(set(mine)) == 8


def test_true_F_annihilates_the_noise_free_scene():
    x, xp, truth = two_view_scene(11, 50, 10)
    d = np.sqrt(sampson(true_F(), x.astype(float), xp.astype(float)))
    assert d[truth].max() < 1.5 and np.median(d[~truth]) > 10


@pytest.mark.parametrize("seed", range(6))
def test_two_routes_agree(seed):
    x, xp, truth = two_view_scene(seed, 160, 96)
    wf = np.ones(len(x), bool)
    a = verify_pair(x.astype(float), xp.astype(float), wf, seed, seed=seed, route="svd")
    b = verify_pair(x.astype(float), xp.astype(float), wf, seed, seed=seed, route="eigh")
    gap = sign_gap(a["F"], b["F"])
    print(f"seed {seed}: best_h {a['best_h']} / {b['best_h']}, |F0 - F1| = {gap:.2e}, true inliers kept "
          f"{(a['mask'] & truth).sum()} of 160, outliers kept {(a['mask'] & ~truth).sum()} of 96, margin "
          f"{margin(a, x, xp, 2.0):.3f} px, valid {a['n_valid']}")
    assert a["best_h"] == b["best_h"] and a["n_valid"] == b["n_valid"] and a["flags"] == b["flags"] == 0
    assert np.array_equal(a["mask"], b["mask"])
    assert gap <= 1e-12 and abs(a["cost"] - b["cost"]) <= 1e-9 * a["cost"]


def test_conditions_on_the_five_pair_fixture():
    scenes, kp, pairs, m = five_pairs()
    res, other = five_pairs_result("svd"), five_pairs_result("eigh")
    for p, ((x, xp, truth), r, o) in enumerate(zip(scenes, res, other)):
        n_in, n_out = FIVE[p]
        assert r["best_h"] == o["best_h"] and np.array_equal(r["mask"], o["mask"]) and r["flags"] == o["flags"]
        if p == 4:
            assert r["flags"] == TOO_FEW and r["n_valid"] == 0 and np.array_equal(r["kept"], pairs[p, :15])
            continue
        assert sign_gap(r["F"], o["F"]) <= 1e-12
        kept_in, kept_out = (r["mask"] & truth).sum(), (r["mask"] & ~truth).sum()
        print(f"pair {p}: {kept_in} of {n_in} inliers, {kept_out} of {n_out} outliers kept, margin "
              f"{margin(r, x, xp, 2.0):.3f} px, best_h {r['best_h']}, valid {r['n_valid']}")
        assert r["flags"] == 0
        assert kept_in >= 0.95 * n_in and kept_out <= math.ceil(6 * n_out / 96)      # (6 of 96, in proportion)
        assert margin(r, x, xp, 2.0) >= 0.02
        assert sign_gap(r["F"], true_F()) < 0.05


@pytest.mark.parametrize("m", BOUNDARY_M)
def test_conditions_on_the_match_count_fixtures(m):
    x, xp, truth = boundary_scene(m)
    kp, pairs, mm = pack([(x, xp, truth)])
    for refit in (0, 2):
        r = verify_numpy(kp, pairs, mm, refit_iters=refit, **FIVE_KW)[0]
        assert bool(r["flags"] & TOO_FEW) == (m < 16)
        assert margin(r, x, xp, 2.0) >= 0.02
        if m >= 63:
            assert (r["mask"] & truth).sum() >= 0.95 * truth.sum()


@pytest.mark.parametrize("n_hyp", BOUNDARY_HYP)
def test_conditions_on_the_hypothesis_count_fixtures(n_hyp):
    scenes, kp, pairs, m = five_pairs()
    r = verify_numpy(kp[1:3], pairs[1:2], m[1:2], pair_base=1, **dict(FIVE_KW, n_hyp=n_hyp))[0]
    x, xp, _ = scenes[1]
    assert r["n_valid"] == n_hyp and margin(r, x, xp, 2.0) >= 0.02


def test_conditions_on_the_failure_fixtures():
    kp, pairs, m = weak_fixture()
    r = verify_numpy(kp, pairs, m, min_inliers=32, **FIVE_KW)[0]
    x, xp = kp[0, pairs[0, :64, 0]], kp[1, pairs[0, :64, 1]]
    print(f"pure outliers: {r['n_inliers']} inliers, margin {margin(r, x, xp, 2.0):.3f} px")
    assert r["flags"] == WEAK and 8 <= r["n_inliers"] < 32 and margin(r, x, xp, 2.0) >= 0.02
    assert np.array_equal(r["kept"], pairs[0, :64])
    kp, pairs, m = malformed_fixture()
    r = verify_numpy(kp, pairs, m, pair_base=2, **FIVE_KW)[0]
    clean = five_pairs_result()[2]
    keep = np.ones(64, bool)
    keep[[3, 10]] = False
    print(f"malformed: {r['n_valid']} valid hypotheses, {r['n_inliers']} inliers (clean: {clean['n_inliers']})")
    assert r["flags"] == MALFORMED and r["n_valid"] < 256 and not r["mask"][[3, 10]].any()
    assert np.array_equal(r["mask"][keep], clean["mask"][keep])      # the rest is judged as before
    ok = keep & (pairs[0, :64] >= 0).all(axis=1)
    assert margin(r, kp[0, pairs[0, :64, 0][ok]], kp[1, pairs[0, :64, 1][ok]], 2.0) >= 0.02


def test_sub_block_with_pair_base_gives_the_rows_of_the_whole_call():
    _, kp, pairs, m = five_pairs()
    whole = five_pairs_result()
    part = verify_numpy(kp[2:], pairs[2:], m[2:], pair_base=2, **FIVE_KW)
    for a, b in zip(whole[2:], part):
        assert a["best_h"] == b["best_h"] and np.array_equal(a["F"], b["F"], equal_nan=True)


# ---- through the loaded library, without a GPU --------------------------------------------------------------------------

def test_library_table_has_the_verify_symbols():
    from meatmodeler_amd import _lib
    assert {"mm_verify_workspace_bytes", "mm_verify_matches"} <= set(_lib.SIGNATURES)
    assert C.sizeof(_lib.VerifyParams) == 40


def test_workspace_bytes_is_monotone_and_aligned():
    from meatmodeler_amd._lib import lib
    f = lib.mm_verify_workspace_bytes
    sizes = [[f(n, h) for h in (1, 63, 64, 65, 256, 4096)] for n in (0, 1, 3, 199, 499)]
    for row in sizes:
        assert all(v % 16 == 0 for v in row) and all(a <= b for a, b in zip(row, row[1:]))
    for a, b in zip(sizes, sizes[1:]):
        assert all(u <= v for u, v in zip(a, b))
    assert f(199, 256) >= 199 * 256 * 10 * 8 and f(1, 1) > 0


def test_argument_errors_return_before_any_device_call():
    """No context and made-up addresses: a bad call must come back from the checks, not from the device."""
    from meatmodeler_amd import _lib
    lib = _lib.lib
    ERR_ARG, ERR_WORKSPACE = -1, -3
    need = lib.mm_verify_workspace_bytes(2, 256)

    def call(prm, ws_bytes=need, ptrs=(64,) * 9, n_pairs=2, cap=CAP):
        a = [C.c_void_p(v) for v in ptrs]
        return lib.mm_verify_matches(None, a[0], a[1], a[2], n_pairs, cap, C.byref(prm) if prm is not None else None, a[3], a[4],
                                     a[5], a[6], a[7], a[8], ws_bytes)

    def prm(**kw):
        v = dict(n_hyp=256, min_matches=16, min_inliers=16, refit_iters=2, seed=0, pair_base=0, on_fail=0, reserved=0,
                 threshold_px=2.0)
        v.update(kw)
        return _lib.VerifyParams(**v)

    distinct = (64, 128, 192, 256, 320, 384, 448, 512, 576)
    for bad in (prm(n_hyp=0), prm(n_hyp=4097), prm(n_hyp=-1), prm(threshold_px=-1.0), prm(threshold_px=math.nan),
                prm(on_fail=2), prm(refit_iters=-1)):
        assert call(bad, ptrs=distinct) == ERR_ARG
    # too small a workspace is told apart from a bad argument -- and is found although the context is missing
    assert call(prm(), ws_bytes=need - 1, ptrs=distinct) == ERR_WORKSPACE
    assert call(prm(n_hyp=4096), ws_bytes=need, ptrs=distinct) == ERR_WORKSPACE
    assert call(prm(), ws_bytes=0, ptrs=distinct) == ERR_WORKSPACE
    for k in range(9):      # each null pointer
        assert call(prm(), ptrs=tuple(0 if i == k else v for i, v in enumerate(distinct))) == ERR_ARG
    assert call(None, ptrs=distinct) == ERR_ARG
    assert call(prm(), ptrs=distinct, n_pairs=-1) == ERR_ARG and call(prm(), ptrs=distinct, cap=0) == ERR_ARG
    assert call(prm(), ptrs=(64, 128, 192, 128, 320, 384, 448, 512, 576)) == ERR_ARG      # pairs_out aliases pairs
    assert call(prm(), ptrs=distinct) == ERR_ARG      # a good call without a context


def test_verify_option_validation():
    from meatmodeler_amd import pipeline
    assert pipeline.verify_options(None) is None
    assert pipeline.verify_options({}) == {}
    assert pipeline.verify_options(dict(n_hyp=64, threshold_px=1.5, on_fail="drop"))["n_hyp"] == 64
    for bad in (dict(nhyp=64), dict(threshold=2.0), dict(pair_base=3), dict(ctx=None)):
        with pytest.raises(ValueError):
            pipeline.verify_options(bad)
    with pytest.raises(ValueError):
        pipeline.verify_options([("n_hyp", 64)])


PCG_PINNED = [129708002, 2831084092, 3861530882]
