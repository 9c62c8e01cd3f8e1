"""CPU: a NumPy restatement of mm_recover_poses and mm_chain_poses (include/meatmodeler.h) and the conditions the GPU test
relies on.  tests/test_recover_poses_gpu.py imports the helpers and fixtures of this module.

The restatement follows the header step by step, with the header's order of operations: E = K^T (F K), the 3 x 3 cyclic Jacobi
on E^T E in Python floats, the four candidates, the depth vote, the flags; the integer min-scatter, the lower median of the
depth ratios and the composition of the chain.  A second route builds the four candidates from numpy.linalg.svd(E): the two
must recover the same motion (R and t are compared, not the candidate index, which depends on the signs a factorisation
happens to return).

Measured here (restatement against the truth):
  noise-free two-view scenes (24 motions): |R - R_true| <= 4.4e-16, |t - t_true| <= 4.4e-16, sigma[0] / sigma[1] - 1 <= 4.4e-16,
  depth[:, 1] against true depth / baseline <= 2.1e-13 relative; candidates 0, 1, 2, 3 win 8, 8, 3 and 5 of the motions.
  chain fixture (six cameras, 120 points): extrinsics against the truth 3.4e-14 noise-free.  With 0.3 px noise (seed 5) the
  rotation blocks stay at 6.7e-16 (they come from the true F alone; the noise reaches only the scale ratios) and the
  translations are off by 8.06e-3 of the unit baseline -- asserted below as 1e-10 and, with a margin of two, 1.6e-2: the
  figure belongs to the fixed seed, the margin covers another NumPy's last bits, not another seed.
"""
import ctypes as C
import functools
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_verify_matches_cpu import K_SCENE, pack, scene_cameras, true_F, two_view_scene  # noqa: E402,F401
from meatmodeler_amd import synth  # noqa: E402
from oracle.geom_oracle import jacobi3, k_inverse  # noqa: E402,F401

POSE_TOO_FEW, POSE_NO_MODEL, POSE_AMBIGUOUS, POSE_MALFORMED = 1, 2, 4, 8      # MM_POSE_*
CHAIN_FEW_COMMON, CHAIN_BROKEN = 1, 2                                         # MM_CHAIN_*
CAP = 320


# ------------------------------------------------------------------------------------------------ the restatement: one pair

def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def cross3(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def mat3(M, v):
    """Row-major M [9] times v (components may be arrays), summed left to right."""
    return [(M[3 * r] * v[0] + M[3 * r + 1] * v[1]) + M[3 * r + 2] * v[2] for r in range(3)]


def essential(F, K):
    F, K = np.asarray(F, float).reshape(9), np.asarray(K, float).reshape(9)
    FK = [(F[3 * r] * K[c] + F[3 * r + 1] * K[3 + c]) + F[3 * r + 2] * K[6 + c] for r in range(3) for c in range(3)]
    return np.array([(K[r] * FK[c] + K[3 + r] * FK[3 + c]) + K[6 + r] * FK[6 + c] for r in range(3) for c in range(3)])


def rotation(u1, u2, u3, v1, v2, v3, transposed_w):
    sg = -1.0 if transposed_w else 1.0
    c1, c2 = sg * u2, -sg * u1
    return np.array([(c1[r] * v1[c] + c2[r] * v2[c]) + u3[r] * v3[c] for r in range(3) for c in range(3)])


def decompose(F, K):
    """-> dict(model, sigma [2], Ra [9], Rb [9], u3 [3]) by the header's construction."""
    with np.errstate(all="ignore"):
        E = essential(F, K)
        G = [[(E[r] * E[c] + E[3 + r] * E[3 + c]) + E[6 + r] * E[6 + c] for c in range(3)] for r in range(3)]
        lam, V = jacobi3(G)
        i3 = i1 = 0
        for c in (1, 2):
            if lam[c] < lam[i3]:
                i3 = c
            if lam[c] > lam[i1]:
                i1 = c
        v3, v1 = V[:, i3].copy(), V[:, i1].copy()
        v2 = cross3(v3, v1)
        e1, e2 = np.array(mat3(E, v1)), np.array(mat3(E, v2))
        s1 = math.sqrt(dot3(e1, e1)) if np.isfinite(dot3(e1, e1)) else math.nan
        u1 = e1 / s1 if s1 != 0 else e1 * math.nan
        w2 = e2 - dot3(u1, e2) * u1
        s2 = math.sqrt(dot3(w2, w2)) if np.isfinite(dot3(w2, w2)) else math.nan
        u2 = w2 / s2 if s2 != 0 else w2 * math.nan
        u3 = cross3(u1, u2)
    model = bool(np.isfinite(np.asarray(F, float)).all() and np.isfinite(s1) and np.isfinite(s2) and s1 > 0 and s2 > 0)
    return dict(model=model, sigma=np.array([s1, s2]), Ra=rotation(u1, u2, u3, v1, v2, v3, False),
                Rb=rotation(u1, u2, u3, v1, v2, v3, True), u3=u3, E=E)


def rays(K, x):
    ki = k_inverse(K)
    return [(ki[0] * x[:, 0] + ki[1] * x[:, 1]) + ki[2], ki[3] * x[:, 1] + ki[4], np.ones(len(x))]


def depths(R, t, a, b):
    """(l1 [n], l2 [n], det / ((r.r)(b.b)) [n]) of the header's formula; a, b lists of three component arrays."""
    r = mat3(R, a)
    with np.errstate(all="ignore"):
        rr, bb, rb, bt, rt = dot3(r, r), dot3(b, b), dot3(r, b), dot3(b, t), dot3(r, t)
        det = rr * bb - rb * rb
        return (rb * bt - rt * bb) / det, (rr * bt - rb * rt) / det, det / (rr * bb)


def front(l1, l2):
    with np.errstate(all="ignore"):
        return np.isfinite(l1) & np.isfinite(l2) & (l1 > 0) & (l2 > 0)


def candidates(dec):
    return [(dec["Ra"], dec["u3"]), (dec["Ra"], -dec["u3"]), (dec["Rb"], dec["u3"]), (dec["Rb"], -dec["u3"])]


def recover_pair(x, xp, wf, F, K, min_matches=8, min_front_frac=0.5, ambiguous_frac=0.5):
    """One pair: x, xp [m, 2] f64 (rows of malformed matches anything), wf [m] bool -> dict(flags, winner, votes [4], m, R [9],
    t [3], sigma [2], depth [m, 2], and for the margin condition cand [4, m, 2] and det_ratio [4, m] over the well-formed rows)."""
    mm = len(x)
    nan = math.nan
    out = dict(flags=0 if wf.all() else POSE_MALFORMED, winner=-1, votes=[0, 0, 0, 0], m=mm, R=np.full(9, nan), t=np.full(3, nan),
               sigma=np.full(2, nan), depth=np.full((mm, 2), nan), cand=np.full((4, mm, 2), nan), det_ratio=np.full((4, mm), nan))
    if mm < max(int(min_matches), 8):
        out["flags"] |= POSE_TOO_FEW
        return out
    dec = decompose(F, K)
    out["sigma"] = dec["sigma"]
    if not dec["model"]:
        out["flags"] |= POSE_NO_MODEL
        return out
    a, b = rays(K, x[wf]), rays(K, xp[wf])
    votes, per = [], []
    for c, (R, t) in enumerate(candidates(dec)):
        l1, l2, dr = depths(R, t, a, b)
        out["cand"][c, wf, 0], out["cand"][c, wf, 1], out["det_ratio"][c, wf] = l1, l2, dr
        ok = front(l1, l2)
        votes.append(int(ok.sum()))
        per.append((l1, l2, ok))
    w = max(range(4), key=lambda c: (votes[c], -c))      # the largest count, ties to the lowest c
    second = max(votes[c] for c in range(4) if c != w)
    if votes[w] < min_front_frac * mm or second >= ambiguous_frac * votes[w]:
        out["flags"] |= POSE_AMBIGUOUS
    l1, l2, ok = per[w]
    d = np.full((int(wf.sum()), 2), nan)
    d[ok, 0], d[ok, 1] = l1[ok], l2[ok]
    out["depth"][wf] = d
    out.update(winner=w, votes=votes, R=candidates(dec)[w][0], t=candidates(dec)[w][1])
    return out


def recover_numpy(kp_xy, pairs, m, F, K, **kw):
    """The whole call -> (R [n, 9], t [n, 3], sigma [n, 2], depth [n, cap, 2], info [n, 8], list of recover_pair dicts)."""
    n, cap = pairs.shape[0], pairs.shape[1]
    R, t, sigma = np.full((n, 9), np.nan), np.full((n, 3), np.nan), np.full((n, 2), np.nan)
    depth, info, res = np.full((n, cap, 2), np.nan), np.zeros((n, 8), np.int32), []
    for p in range(n):
        mm = int(np.clip(m[p], 0, cap))
        rows = pairs[p, :mm]
        wf = ((rows >= 0) & (rows < cap)).all(axis=1)
        x, xp = np.zeros((mm, 2)), np.zeros((mm, 2))
        x[wf] = kp_xy[p, rows[wf, 0]]
        xp[wf] = kp_xy[p + 1, rows[wf, 1]]
        r = recover_pair(x, xp, wf, F[p], K, **kw)
        R[p], t[p], sigma[p], depth[p, :mm] = r["R"], r["t"], r["sigma"], r["depth"]
        info[p] = [r["flags"], r["winner"]] + r["votes"] + [mm, 0]
        res.append(r)
    return R, t, sigma, depth, info, res


# ------------------------------------------------------------------------------------------------ the restatement: the chain

def positive(d):
    return bool(np.isfinite(d) and d > 0)


def chain_numpy(pairs, m, depth, R, t, info, E0=None, min_common=8):
    """-> (extrinsics [n+1, 3, 4], scale [n], rho [n], chain_info [n, 2]); every ratio one division, the composition summed
    left to right."""
    n, cap = pairs.shape[0], pairs.shape[1]
    T = np.eye(3, 4) if E0 is None else np.asarray(E0, float)[:3, :].copy()
    ext, scale, rho, cinfo = np.zeros((n + 1, 3, 4)), np.ones(n), np.ones(n), np.zeros((n, 2), np.int32)
    ext[0] = T
    broken = [(int(info[p, 0]) & (POSE_TOO_FEW | POSE_NO_MODEL)) != 0 for p in range(n)]
    s = 1.0
    for p in range(n):
        if broken[p]:
            cinfo[p] = (CHAIN_BROKEN, 0)
        elif p > 0 and broken[p - 1]:
            cinfo[p] = (CHAIN_FEW_COMMON, 0)
        elif p > 0:
            m0, m1 = int(np.clip(m[p - 1], 0, cap)), int(np.clip(m[p], 0, cap))
            prev = {}
            for i in range(m0):
                k = int(pairs[p - 1, i, 1])
                if 0 <= k < cap and positive(depth[p - 1, i, 1]) and k not in prev:
                    prev[k] = i
            ratios = []
            for j in range(m1):
                q = int(pairs[p, j, 0])
                if 0 <= q < cap and q in prev and positive(depth[p, j, 0]):
                    with np.errstate(all="ignore"):
                        ratios.append(np.float64(depth[p - 1, prev[q], 1]) / np.float64(depth[p, j, 0]))
            cinfo[p, 1] = len(ratios)
            if len(ratios) < min_common:
                cinfo[p, 0] = CHAIN_FEW_COMMON
            elif ratios:
                rho[p] = sorted(ratios)[(len(ratios) - 1) // 2]
        s = s * rho[p]
        scale[p] = s
        Rp = np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]) if broken[p] else np.asarray(R[p], float)
        tp = np.zeros(3) if broken[p] else np.asarray(t[p], float)
        N = np.zeros((3, 4))
        for r in range(3):
            for c in range(4):
                N[r, c] = (Rp[3 * r] * T[0, c] + Rp[3 * r + 1] * T[1, c]) + Rp[3 * r + 2] * T[2, c]
            N[r, 3] = N[r, 3] + s * tp[r]
        T = N
        ext[p + 1] = T
    return ext, scale, rho, cinfo


# ------------------------------------------------------------------------------------------------ the second route

def svd_route(x, xp, F, K):
    """The motion the depth vote picks among the four candidates built from numpy.linalg.svd(E) -> (R [3, 3], t [3], votes)."""
    K = np.asarray(K, float).reshape(3, 3)
    E = K.T @ np.asarray(F, float).reshape(3, 3) @ K
    U, _, Vt = np.linalg.svd(E)
    U = U * np.sign(np.linalg.det(U))
    Vt = Vt * np.sign(np.linalg.det(Vt))
    W = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    Ki = np.linalg.inv(K)
    a = np.c_[x, np.ones(len(x))] @ Ki.T
    b = np.c_[xp, np.ones(len(x))] @ Ki.T
    best = None
    for R in (U @ W @ Vt, U @ W.T @ Vt):
        for t in (U[:, 2], -U[:, 2]):
            r = a @ R.T
            lam = np.array([np.linalg.lstsq(np.c_[-r[i], b[i]], t, rcond=None)[0] for i in range(len(x))])      # l2 b - l1 r = t
            votes = int(((lam[:, 0] > 0) & (lam[:, 1] > 0)).sum())
            if best is None or votes > best[2]:
                best = (R, t, votes)
    return best


# ------------------------------------------------------------------------------------------------ fixtures

def skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


def fundamental(R, t, K=K_SCENE, sign=1.0):
    """x'^T F x = 0 of X2 = R X1 + t, unit norm [9]."""
    Ki = np.linalg.inv(K)
    F = Ki.T @ skew(t) @ R @ Ki
    return sign * (F / np.linalg.norm(F)).ravel()


def random_motion(seed):
    """(R, t): a rotation of 0.03 .. 0.25 rad about a random axis and a baseline of 0.4 .. 1.0, mostly sideways."""
    rng = np.random.default_rng(1000 + seed)
    axis = rng.normal(size=3)
    R = synth.rodrigues(axis / np.linalg.norm(axis) * rng.uniform(0.03, 0.25))
    t = rng.normal(size=3) * [1.0, 1.0, 0.3]
    return R, t / np.linalg.norm(t) * rng.uniform(0.4, 1.0)


def scene(seed, n_in, n_out, noise=0.25, motion=None):
    """A two-view scene under its own motion: dict(x, xp [n, 2] f64, truth [n] bool, R, t (unit), baseline, depth2 [n] -- the
    true camera-2 depth, NaN for an outlier --, F [9] the true fundamental matrix, its sign alternating with the seed)."""
    rng = np.random.default_rng(seed)
    R, t = random_motion(seed) if motion is None else motion
    xs, xps, d2 = np.zeros((0, 2)), np.zeros((0, 2)), np.zeros(0)
    while len(xs) < n_in:
        X = rng.uniform([-2, -1.5, 4], [2, 1.5, 9], size=(2 * n_in + 8, 3))
        X2 = X @ R.T + t
        a, b = X @ K_SCENE.T, X2 @ K_SCENE.T
        a, b = a[:, :2] / a[:, 2:], b[:, :2] / b[:, 2:]
        vis = ((a >= 0) & (a < [640, 480]) & (b >= 0) & (b < [640, 480])).all(axis=1) & (X2[:, 2] > 0.5)
        xs, xps, d2 = np.vstack([xs, a[vis]]), np.vstack([xps, b[vis]]), np.r_[d2, X2[vis, 2]]
    xs = xs[:n_in] + rng.normal(0, noise, (n_in, 2))
    xps = xps[:n_in] + rng.normal(0, noise, (n_in, 2))
    xs = np.vstack([xs, rng.uniform([0, 0], [640, 480], (n_out, 2))])
    xps = np.vstack([xps, rng.uniform([0, 0], [640, 480], (n_out, 2))])
    d2 = np.r_[d2[:n_in], np.full(n_out, np.nan)]
    truth = np.arange(n_in + n_out) < n_in
    order = rng.permutation(n_in + n_out)
    base = np.linalg.norm(t)
    return dict(x=xs[order], xp=xps[order], truth=truth[order], R=R, t=t / base, baseline=base, depth2=d2[order],
                F=fundamental(R, t, sign=1.0 if seed % 2 == 0 else -1.0))


def packed(scenes):
    """-> (kp_xy f32, pairs, m, F [n, 9]) of a list of scene dicts (the key point layout of test_verify_matches_cpu.pack)."""
    kp, pairs, m = pack([(s["x"], s["xp"], s["truth"]) for s in scenes], cap=CAP)
    return kp, pairs, m, np.array([s["F"] for s in scenes]).reshape(len(scenes), 9)


FIVE = ((192, 64), (64, 0), (40, 24), (17, 0), (9, 0))      # the five-pair call of the GPU test (inliers, outliers)
FIVE_SEEDS = (0, 1, 2, 3, 4)
BOUNDARY_M = (0, 7, 8, 9, 63, 64, 65, 255, 256, 257, CAP)


@functools.lru_cache(maxsize=None)
def five_pairs():
    scenes = [scene(s, a, b) for s, (a, b) in zip(FIVE_SEEDS, FIVE)]
    return (scenes,) + packed(scenes)


def boundary_scene(m):
    """The single-pair fixture of the m-boundary tests: a quarter outliers from 63 matches on."""
    n_out = m // 4 if m >= 63 else 0
    return scene(100 + m, m - n_out, n_out)


ROTATION_SEED = 300


@functools.lru_cache(maxsize=None)
def rotation_only_fixture():
    """64 matches of a camera that only rotates, each x' moved by exactly one pixel in a random direction (so that no two rays
    are parallel: det / ((r.r)(b.b)) stays near (1 px / f)^2 = 4e-6), with the F of that rotation and an arbitrary baseline
    direction -- what an epipolar fit of such a pair can return.  No candidate puts most of the points in front."""
    rng = np.random.default_rng(ROTATION_SEED)
    R, _ = random_motion(ROTATION_SEED)
    X = rng.uniform([-1.5, -1.0, 4], [1.5, 1.0, 9], size=(64, 3))
    a, b = X @ K_SCENE.T, (X @ R.T) @ K_SCENE.T
    phi = rng.uniform(0, 2 * np.pi, 64)
    x, xp = a[:, :2] / a[:, 2:], b[:, :2] / b[:, 2:] + np.c_[np.cos(phi), np.sin(phi)]
    s = dict(x=x, xp=xp, truth=np.ones(64, bool), F=fundamental(R, np.array([0.6, -0.3, 0.2])))
    return packed([s])


@functools.lru_cache(maxsize=None)
def malformed_fixture():
    """Pair 2 of the five-pair call with match 3's query index -1 and match 10's train index cap."""
    _, kp, pairs, m, F = five_pairs()
    bad = pairs[2:3].copy()
    bad[0, 3, 0] = -1
    bad[0, 10, 1] = CAP
    return kp[2:4], bad, m[2:3], F[2:3]


CHAIN_DEG = (0.0, 4.0, 9.0, 13.0, 20.0, 24.0)
CHAIN_POINTS = 120


@functools.lru_cache(maxsize=None)
def chain_fixture(noise=0.0, seed=5):
    """Six cameras on an orbit with unequal steps looking at 120 points; every frame's key point table in its own shuffled
    order, consecutive matches in shuffled row order, the true F per pair.
    -> dict(kp [6, cap, 2] f64, pairs [5, cap, 2], m [5], F [5, 9], ext [6, 3, 4] the true extrinsics with the first camera as
    origin and the first baseline as unit)."""
    rng = np.random.default_rng(seed)
    ext = np.array([synth.look_at_extrinsic((7.0 * math.cos(math.radians(d)), -2.0, 7.0 * math.sin(math.radians(d))))
                    for d in CHAIN_DEG])
    X = rng.uniform(-1.5, 1.5, size=(CHAIN_POINTS, 3))
    n = len(CHAIN_DEG)
    kp = rng.uniform(0, 400, (n, CAP, 2))
    slot = np.array([rng.permutation(CAP)[:CHAIN_POINTS] for _ in range(n)])
    for f in range(n):
        Xc = X @ ext[f, :, :3].T + ext[f, :, 3]
        px = Xc @ K_SCENE.T
        assert (Xc[:, 2] > 1).all()
        kp[f, slot[f]] = px[:, :2] / px[:, 2:] + (rng.normal(0, noise, (CHAIN_POINTS, 2)) if noise else 0.0)
    pairs = np.full((n - 1, CAP, 2), -1, np.int32)
    F = np.zeros((n - 1, 9))
    for p in range(n - 1):
        order = rng.permutation(CHAIN_POINTS)
        pairs[p, :CHAIN_POINTS] = np.c_[slot[p][order], slot[p + 1][order]]
        Rr = ext[p + 1, :, :3] @ ext[p, :, :3].T
        F[p] = fundamental(Rr, ext[p + 1, :, 3] - Rr @ ext[p, :, 3])
    R0, t0 = ext[0, :, :3], ext[0, :, 3]
    Rr1 = ext[1, :, :3] @ R0.T
    unit = np.linalg.norm(ext[1, :, 3] - Rr1 @ t0)
    rel = np.array([np.c_[e[:, :3] @ R0.T, (e[:, 3] - e[:, :3] @ R0.T @ t0) / unit] for e in ext])
    return dict(kp=kp, pairs=pairs, m=np.full(n - 1, CHAIN_POINTS, np.int32), F=F, ext=rel)


def run_chain(fx, **kw):
    R, t, sigma, depth, info, res = recover_numpy(fx["kp"], fx["pairs"], fx["m"], fx["F"], K_SCENE)
    return chain_numpy(fx["pairs"], fx["m"], depth, R, t, info, **kw) + (info, res)


def margin_of(res, min_front_frac=0.5, ambiguous_frac=0.5):
    """(min |l| over the finite depths of all candidates, min det ratio, distance of the vote fractions from their thresholds)
    of a list of recover_pair dicts."""
    lmin, dmin, fmin = np.inf, np.inf, np.inf
    for r in res:
        c = r["cand"][np.isfinite(r["cand"])]
        if c.size:
            lmin = min(lmin, np.abs(c).min())
        d = r["det_ratio"][np.isfinite(r["det_ratio"])]
        if d.size:
            dmin = min(dmin, d.min())
        if r["winner"] >= 0:
            v, w = r["votes"], r["winner"]
            fmin = min(fmin, abs(v[w] / r["m"] - min_front_frac))
            if v[w] > 0:
                fmin = min(fmin, abs(max(v[c] for c in range(4) if c != w) / v[w] - ambiguous_frac))
    return lmin, dmin, fmin


# ------------------------------------------------------------------------------------------------ tests

NOISE_FREE = tuple(range(24))


@functools.lru_cache(maxsize=None)
def noise_free(seed):
    s = scene(seed, 48, 0, noise=0.0)
    return s, recover_pair(s["x"], s["xp"], np.ones(48, bool), s["F"], K_SCENE)


@pytest.mark.parametrize("seed", NOISE_FREE)
def test_noise_free_scene_returns_the_true_motion(seed):
    s, r = noise_free(seed)
    gR, gt = np.abs(r["R"].reshape(3, 3) - s["R"]).max(), np.abs(r["t"] - s["t"]).max()
    gs = abs(r["sigma"][0] / r["sigma"][1] - 1.0)
    gd = np.abs(r["depth"][:, 1] * s["baseline"] / s["depth2"] - 1.0).max()
    print(f"seed {seed}: winner {r['winner']} votes {r['votes']}, |R - R*| {gR:.1e}, |t - t*| {gt:.1e}, sigma ratio - 1 {gs:.1e}, "
          f"depth gap {gd:.1e}")
    assert r["flags"] == 0 and r["votes"][r["winner"]] == 48
    assert gR <= 1e-9 and gt <= 1e-9 and gs < 1e-9 and gd <= 1e-8
    assert abs(np.linalg.det(r["R"].reshape(3, 3)) - 1.0) < 1e-12 and abs(np.linalg.norm(r["t"]) - 1.0) < 1e-12


def test_every_candidate_wins_somewhere():
    winners = {noise_free(seed)[1]["winner"] for seed in NOISE_FREE}
    winners |= {r["winner"] for r in recover_numpy(*five_pairs()[1:], K_SCENE)[5]}
    assert winners >= {0, 1, 2, 3}, winners


@pytest.mark.parametrize("seed", (0, 1, 2, 3, 5, 8))
def test_second_route_recovers_the_same_motion(seed):
    for s in (scene(seed, 48, 0, noise=0.0), scene(seed, 40, 16)):
        r = recover_pair(s["x"], s["xp"], np.ones(len(s["x"]), bool), s["F"], K_SCENE)
        R2, t2, votes2 = svd_route(s["x"], s["xp"], s["F"], K_SCENE)
        gR, gt = np.abs(r["R"].reshape(3, 3) - R2).max(), np.abs(r["t"] - t2).max()
        print(f"seed {seed}: |R - R_svd| {gR:.1e}, |t - t_svd| {gt:.1e}, votes {r['votes'][r['winner']]} / {votes2}")
        assert gR <= 1e-9 and gt <= 1e-9 and r["votes"][r["winner"]] == votes2


def test_margin_condition_on_the_gpu_fixtures():
    """What makes the exact comparison of counts and NaN patterns on the GPU legitimate: no depth of any candidate near zero,
    no pair of rays near parallel, no vote fraction near its threshold -- outlier rows included."""
    sets = {"five": recover_numpy(*five_pairs()[1:], K_SCENE)[5],
            "malformed": recover_numpy(*malformed_fixture(), K_SCENE)[5],
            "rotation": recover_numpy(*rotation_only_fixture(), K_SCENE)[5],
            "chain": run_chain(chain_fixture())[5], "chain noisy": run_chain(chain_fixture(0.3))[5]}
    for m in BOUNDARY_M:
        sets[f"m={m}"] = recover_numpy(*packed([boundary_scene(m)]), K_SCENE)[5]
    for name, res in sets.items():
        lmin, dmin, fmin = margin_of(res)
        print(f"{name}: min |l| {lmin:.2e}, min det ratio {dmin:.2e}, vote fractions {fmin:.3f} from the thresholds")
        assert lmin >= 1e-3 and dmin >= 1e-8 and fmin >= 0.02, name


def test_flag_fixtures():
    _, kp, pairs, m, F = five_pairs()
    info = recover_numpy(kp, pairs, m, F, K_SCENE)[4]
    assert list(info[:, 0]) == [0, 0, 0, 0, 0] and list(info[:, 6]) == [256, 64, 64, 17, 9]
    res = recover_numpy(*packed([boundary_scene(7)]), K_SCENE)
    assert res[4][0, 0] == POSE_TOO_FEW and res[4][0, 1] == -1 and np.isnan(res[0]).all() and np.isnan(res[3]).all()
    Fn = F.copy()
    Fn[1] = np.nan
    R, t, sigma, depth, info, _ = recover_numpy(kp, pairs, m, Fn, K_SCENE)
    assert info[1, 0] == POSE_NO_MODEL and np.isnan(R[1]).all() and np.isnan(t[1]).all() and np.isnan(depth[1]).all()
    assert info[0, 0] == 0 and info[2, 0] == 0
    r = recover_numpy(*rotation_only_fixture(), K_SCENE)[5][0]
    print(f"rotation only: votes {r['votes']} of {r['m']}")
    assert r["flags"] == POSE_AMBIGUOUS and np.isfinite(r["R"]).all()
    clean = recover_numpy(kp[2:4], pairs[2:3], m[2:3], F[2:3], K_SCENE)[5][0]
    bad = recover_numpy(*malformed_fixture(), K_SCENE)[5][0]
    assert bad["flags"] == POSE_MALFORMED and bad["winner"] == clean["winner"]
    # the counts lose exactly what the two rows voted before; nothing else changes
    lost = [int(front(clean["cand"][c, [3, 10], 0], clean["cand"][c, [3, 10], 1]).sum()) for c in range(4)]
    assert [a - b for a, b in zip(clean["votes"], bad["votes"])] == lost and sum(lost) > 0
    assert np.isnan(bad["depth"][[3, 10]]).all()


def test_chain_fixture_returns_the_true_extrinsics():
    """Noise-free to 1e-10; with 0.3 px noise (seed 5) the restatement's own error: measured 6.7e-16 on the rotation blocks (the
    true F fixes them; asserted at 1e-10) and 8.06e-3 of the unit baseline on the translations, asserted with a margin of
    two (1.6e-2)."""
    fx = chain_fixture()
    ext, scale, rho, cinfo, info, _ = run_chain(fx)
    gap = np.abs(ext - fx["ext"]).max()
    print(f"noise-free: |ext - truth| {gap:.1e}, scale {scale}, n_common {cinfo[:, 1]}")
    assert gap <= 1e-10 and (info[:, 0] == 0).all() and (cinfo[:, 0] == 0).all()
    assert list(cinfo[:, 1]) == [0] + [CHAIN_POINTS] * 4 and scale[0] == 1.0 and rho[0] == 1.0
    fx = chain_fixture(0.3)
    ext = run_chain(fx)[0]
    gR, gt = np.abs(ext[:, :, :3] - fx["ext"][:, :, :3]).max(), np.abs(ext[:, :, 3] - fx["ext"][:, :, 3]).max()
    print(f"0.3 px: rotation blocks {gR:.2e}, translations {gt:.2e} of the unit baseline")
    assert gR <= 1e-10 and gt <= 1.6e-2


def test_chain_edges_of_the_restatement():
    """Lower median, lowest finite row, few common, a broken pair: the cases the GPU test feeds the kernel."""
    for name, (args, want) in chain_edge_cases().items():
        ext, scale, rho, cinfo = chain_numpy(*args["inputs"], **args["kw"])
        assert list(cinfo[:, 0]) == want["flags"] and list(cinfo[:, 1]) == want["n_common"], name
        assert np.array_equal(rho, want["rho"]), name
        assert np.isfinite(ext).all(), name


def chain_inputs(n_pairs, common, cap=CAP, seed=0, depth_scale=None):
    """Hand-made chain inputs: every frame has `common[p]` key points shared by pair p - 1 and pair p (common[0] unused), 40
    matches per pair, random positive depths, random rotations.  -> [pairs, m, depth, R, t, info]."""
    rng = np.random.default_rng(seed)
    mm = 40
    pairs = np.full((n_pairs, cap, 2), -1, np.int32)
    depth = np.full((n_pairs, cap, 2), np.nan)
    for p in range(n_pairs):
        q = rng.permutation(cap // 2)[:mm]                    # queries of pair p: key points of frame p below cap / 2 ...
        if p > 0:
            q[:common[p]] = pairs[p - 1, rng.permutation(mm)[:common[p]], 1]      # ... except the shared ones
        pairs[p, :mm] = np.c_[q, cap // 2 + rng.permutation(cap // 2)[:mm]]       # trains of pair p: at or above cap / 2
        order = rng.permutation(mm)
        pairs[p, :mm] = pairs[p, :mm][order]
        depth[p, :mm] = rng.uniform(2.0, 9.0, (mm, 2)) * (1.0 if depth_scale is None else depth_scale[p])
    m = np.full(n_pairs, mm, np.int32)
    R = np.array([synth.rodrigues(rng.normal(size=3) * 0.1).ravel() for _ in range(n_pairs)])
    t = rng.normal(size=(n_pairs, 3))
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    info = np.zeros((n_pairs, 8), np.int32)
    info[:, 6] = mm
    return [pairs, m, depth, R, t, info]


@functools.lru_cache(maxsize=None)
def chain_edge_cases():
    """name -> (dict(inputs, kw), dict(flags, n_common, rho)): expected values worked out here by sorting, not by chain_numpy."""
    cases = {}

    def expect(inputs, p):
        pairs, m, depth = inputs[0], inputs[1], inputs[2]
        ratios = []
        for j in range(m[p]):
            rows = [i for i in range(m[p - 1]) if pairs[p - 1, i, 1] == pairs[p, j, 0] and depth[p - 1, i, 1] > 0]
            if rows and depth[p, j, 0] > 0:
                ratios.append(depth[p - 1, rows[0], 1] / depth[p, j, 0])
        return len(ratios), (sorted(ratios)[(len(ratios) - 1) // 2] if ratios else 1.0)

    one = chain_inputs(1, [0])
    cases["one pair"] = (dict(inputs=one, kw={}), dict(flags=[0], n_common=[0], rho=np.ones(1)))
    # n_common in {0, min_common - 1, min_common}, then an even (12) and an odd (13) count
    inp = chain_inputs(6, [0, 0, 7, 8, 12, 13], seed=1, depth_scale=[1, 1, 2, 0.5, 3, 1])
    rho = np.ones(6)
    for p in (3, 4, 5):
        n, rho[p] = expect(inp, p)
        assert n == [0, 0, 7, 8, 12, 13][p]
    cases["common counts"] = (dict(inputs=inp, kw={}), dict(flags=[0, CHAIN_FEW_COMMON, CHAIN_FEW_COMMON, 0, 0, 0],
                                                            n_common=[0, 0, 7, 8, 12, 13], rho=rho))
    # two rows of pair p - 1 with the same train, a finite and a NaN depth in either order: the lowest finite row wins
    for name, nan_first in (("duplicate train, NaN first", True), ("duplicate train, finite first", False)):
        inp = chain_inputs(2, [0, 9], seed=2)
        pairs, m, depth = inp[0], inp[1], inp[2]
        shared = pairs[1, [j for j in range(40) if pairs[1, j, 0] >= CAP // 2][0], 0]
        i0 = int(np.nonzero(pairs[0, :40, 1] == shared)[0][0])
        pairs[0, 40] = (CAP // 2 - 1, shared)      # a later row with the same train
        m[0] = 41
        depth[0, 40] = (3.0, 5.5)
        depth[0, i0 if nan_first else 40] = np.nan
        n, r = expect(inp, 1)
        assert n == 9
        cases[name] = (dict(inputs=inp, kw={}), dict(flags=[0, 0], n_common=[0, 9], rho=np.array([1.0, r])))
    # a broken pair in the middle of five, and a caller's E0
    inp = chain_inputs(5, [0, 10, 10, 10, 11], seed=3)
    inp[5][2, 0] = POSE_NO_MODEL
    inp[3][2], inp[4][2], inp[2][2] = np.nan, np.nan, np.nan
    rho = np.ones(5)
    rho[1], rho[4] = expect(inp, 1)[1], expect(inp, 4)[1]
    E0 = np.c_[synth.rodrigues([0.1, -0.2, 0.05]), [0.3, -1.0, 2.0]]
    cases["broken in the middle"] = (dict(inputs=inp, kw=dict(E0=E0)),
                                     dict(flags=[0, 0, CHAIN_BROKEN, CHAIN_FEW_COMMON, 0], n_common=[0, 10, 0, 0, 11], rho=rho))
    return cases


# ---- through the loaded library, without a GPU --------------------------------------------------------------------------

def test_library_table_has_the_pose_symbols():
    from meatmodeler_amd import _lib
    assert {"mm_recover_poses", "mm_chain_poses"} <= set(_lib.SIGNATURES)
    assert C.sizeof(_lib.PoseParams) == 24
    assert hasattr(_lib.lib, "mm_recover_poses") and hasattr(_lib.lib, "mm_chain_poses")


def test_argument_errors_return_before_any_device_call():
    """No context and made-up addresses: a bad call must come back from the checks, not from the device."""
    from meatmodeler_amd import _lib
    lib = _lib.lib
    ERR_ARG = -1
    K = np.ascontiguousarray(K_SCENE.ravel())

    def recover(prm, ptrs, K=K, n_pairs=2, cap=CAP):
        a = [C.c_void_p(v) for v in ptrs]
        kp = K.ctypes.data_as(_lib.c_f64p) if K is not None else None
        return lib.mm_recover_poses(None, kp, a[0], a[1], a[2], a[3], n_pairs, cap, C.byref(prm) if prm is not None else None,
                                    a[4], a[5], a[6], a[7], a[8])

    def prm(**kw):
        v = dict(min_matches=8, reserved=0, min_front_frac=0.5, ambiguous_frac=0.5)
        v.update(kw)
        return _lib.PoseParams(**v)

    distinct = tuple(64 * (i + 1) for i in range(9))
    for bad in (prm(min_front_frac=-0.1), prm(min_front_frac=1.5), prm(ambiguous_frac=math.nan), prm(ambiguous_frac=2.0)):
        assert recover(bad, distinct) == ERR_ARG
    for k in range(9):      # each null pointer
        assert recover(prm(), tuple(0 if i == k else v for i, v in enumerate(distinct))) == ERR_ARG
    assert recover(None, distinct) == ERR_ARG and recover(prm(), distinct, K=None) == ERR_ARG
    assert recover(prm(), distinct, cap=0) == ERR_ARG and recover(prm(), distinct, n_pairs=-1) == ERR_ARG
    for k, v in ((0, 0.0), (4, 0.0), (3, 1.0), (8, 2.0), (2, math.nan)):      # zero focal lengths, lower triangle, K[8], NaN
        Kb = K.copy()
        Kb[k] = v
        assert recover(prm(), distinct, K=Kb) == ERR_ARG
    assert recover(prm(), distinct) == ERR_ARG      # a good call without a context

    E0 = np.ascontiguousarray(np.eye(3, 4).ravel())

    def chain(ptrs, E0=E0, n_pairs=2, cap=CAP, min_common=8):
        a = [C.c_void_p(v) for v in ptrs]
        e = E0.ctypes.data_as(_lib.c_f64p) if E0 is not None else None
        return lib.mm_chain_poses(None, a[0], a[1], a[2], a[3], a[4], a[5], n_pairs, cap, e, min_common, a[6], a[7], a[8], a[9])

    ten = tuple(64 * (i + 1) for i in range(10))
    for k in range(10):
        assert chain(tuple(0 if i == k else v for i, v in enumerate(ten))) == ERR_ARG
    assert chain(ten, E0=None) == ERR_ARG and chain(ten, cap=0) == ERR_ARG and chain(ten, cap=8193) == ERR_ARG
    assert chain(ten, min_common=-1) == ERR_ARG and chain(ten, n_pairs=-1) == ERR_ARG
    assert chain(ten) == ERR_ARG      # a good call without a context


def test_pose_option_validation():
    from meatmodeler_amd import pipeline
    assert pipeline.pose_options(None) is None
    assert pipeline.pose_options({}) == {}
    assert pipeline.pose_options(dict(min_matches=12, min_common=4))["min_common"] == 4
    for bad in (dict(min_match=8), dict(ctx=None), dict(K=None), dict(front=0.5)):
        with pytest.raises(ValueError):
            pipeline.pose_options(bad)
    with pytest.raises(ValueError):
        pipeline.pose_options([("min_matches", 8)])


def test_run_rejects_poses_without_verify_and_missing_extrinsics():
    """The checks come before anything touches the device: a pipeline object without one is enough."""
    from meatmodeler_amd.pipeline import ClipPipeline
    pipe = ClipPipeline.__new__(ClipPipeline)
    frames = np.zeros((3, 8, 8), np.uint8)
    with pytest.raises(ValueError, match="verify"):
        pipe.run(frames, K_SCENE, None, poses={})
    with pytest.raises(ValueError, match="extrinsics"):
        pipe.run(frames, K_SCENE, None)
    with pytest.raises(ValueError):
        pipe.run(frames, K_SCENE, None, verify={}, poses=dict(nope=1))
