"""CPU: a NumPy restatement of mm_align_similarity, mm_apply_similarity and mm_camera_centres (include/meatmodeler.h) and the
conditions the GPU test relies on.  tests/test_align_similarity_gpu.py imports the helpers and fixtures of this module.

The restatement follows the header step by step, with the header's order of operations: the fit through the 3 x 3 cyclic Jacobi
of M^T M in Python floats (one routine for the three-point hypothesis and the refit), the integer sampling with three picks, the
MSAC score with A = s R, the ranking cost rows ascending inside a chunk of 4096 and chunks ascending, every other sum in the
workgroup's order inside a chunk, the winner, the refit rounds and the flags.  A second route, Umeyama's solution through
numpy.linalg.svd, must give the same similarity.

The discrete outputs (flags, best_h, the valid count, n_inliers, the mask) are compared exactly on the GPU; that is sound only
where no decision sits on a rounding error, so the margins of every fixture are conditions here: every |e - tau| >= 1e-6 tau for
every model that decides something, the runner-up hypothesis at least 1e-9 relative above the winner (hypotheses over the
winner's own three rows are the winner's bits: the rows enter the fit in ascending order, and the tie goes to the lowest h),
lambda2 / lambda1 a factor 2 from collinear_tol^2, and a refit's cost at least 1e-9 relative from the cost it is compared with unless it IS the current model
again (an unchanged inlier set gives the same moments, bit for bit, on either side).
"""
import functools
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_recover_poses_cpu import cross3, dot3, jacobi3, mat3  # noqa: E402
from oracle.geom_oracle import block_sum, factor_from, pcg  # noqa: E402

TOO_FEW, NO_MODEL, WEAK, NONFINITE = 1, 2, 4, 8      # MM_ALIGN_*
CHUNK = 4096                                         # MM_ALIGN_CHUNK
M32 = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------ the restatement: the fit

def fit(M, var, cs, cd, with_scale=True, collinear_tol=1e-6):
    """The fit from the moments about the centroids -> (sim [13], valid, lambda2 / lambda1)."""
    M = np.asarray(M, float).reshape(9)
    cs, cd = np.asarray(cs, float), np.asarray(cd, float)
    with np.errstate(all="ignore"):
        G = [[(M[r] * M[c] + M[3 + r] * M[3 + c]) + M[6 + r] * M[6 + c] for c in range(3)] for r in range(3)]
        lam, V = jacobi3(G)
        i1 = 0
        for c in (1, 2):
            if lam[c] > lam[i1]:
                i1 = c
        ia, ib = [c for c in range(3) if c != i1]
        i2 = ib if lam[ib] > lam[ia] else ia
        lam1, lam2 = np.float64(lam[i1]), np.float64(lam[i2])
        v1, v2 = V[:, i1].copy(), V[:, i2].copy()
        v3 = cross3(v1, v2)
        ok = bool(np.isfinite(lam1) and lam1 > 0 and np.isfinite(lam2) and not lam2 <= (collinear_tol * collinear_tol) * lam1
                  and np.isfinite(var) and var > 0)
        e1, e2 = np.array(mat3(M, v1)), np.array(mat3(M, v2))
        u1 = e1 / np.sqrt(np.float64(dot3(e1, e1)))
        w2 = e2 - dot3(u1, e2) * u1
        u2 = w2 / np.sqrt(np.float64(dot3(w2, w2)))
        u3 = cross3(u1, u2)
        R = np.array([(u1[r] * v1[c] + u2[r] * v2[c]) + u3[r] * v3[c] for r in range(3) for c in range(3)])
        tr = np.float64(0.0)
        for k in range(9):
            tr = tr + R[k] * M[k]
        s = tr / np.float64(var) if with_scale else np.float64(1.0)
        d = np.array([cd[r] - s * ((R[3 * r] * cs[0] + R[3 * r + 1] * cs[1]) + R[3 * r + 2] * cs[2]) for r in range(3)])
        sim = np.concatenate([[s], R, d])
        ratio = float(lam2 / lam1) if lam1 != 0 else math.nan
    return sim, ok and bool(np.isfinite(sim).all()), ratio


def moments_rows(src, dst):
    """Centroids and moments of a few rows, rows ascending (the hypothesis: three rows, centroids ((r0 + r1) + r2) / 3)."""
    n = len(src)
    cs, cd = np.zeros(3), np.zeros(3)
    for k in range(n):
        cs, cd = cs + src[k], cd + dst[k]
    cs, cd = cs / float(n), cd / float(n)
    M, var = np.zeros(9), 0.0
    for k in range(n):
        a, b = src[k] - cs, dst[k] - cd
        for r in range(3):
            for c in range(3):
                M[3 * r + c] += b[r] * a[c]
        var += (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
    return M, var, cs, cd


def fit_rows(src, dst, **kw):
    with np.errstate(all="ignore"):
        return fit(*moments_rows(np.asarray(src, float), np.asarray(dst, float)), **kw)


def chunk_sum(vals):
    """Sum of the rows of vals [n, N]: the workgroup's order inside a chunk, the chunks ascending from 0."""
    vals = np.asarray(vals, float)
    tot = np.zeros(vals.shape[1])
    for c0 in range(0, len(vals), CHUNK):
        tot = tot + block_sum(vals[c0:c0 + CHUNK])
    return tot


def distance(sims, src, dst, tau2):
    """sims [B, 13] -> (e2 [B, n], inlier [B, n])."""
    sims = np.asarray(sims, float).reshape(-1, 13)
    with np.errstate(all="ignore"):
        A = sims[:, 0:1] * sims[:, 1:10]
        x, y, z = src[None, :, 0], src[None, :, 1], src[None, :, 2]
        e = [dst[None, :, r] - (((A[:, 3 * r:3 * r + 1] * x + A[:, 3 * r + 1:3 * r + 2] * y) + A[:, 3 * r + 2:3 * r + 3] * z)
                                + sims[:, 10 + r:11 + r]) for r in range(3)]
        e2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        return e2, np.isfinite(e2) & (e2 <= tau2)


def model_cost(sim, src, dst, tau2):
    """(cost, n_inliers, inlier [n], e2 [n]) of one model, the sums in the workgroup order."""
    e2, inl = distance(sim, src, dst, tau2)
    e2, inl = e2[0], inl[0]
    tot = chunk_sum(np.stack([np.where(inl, e2, tau2), inl.astype(float)], 1)) if len(src) else np.zeros(2)
    return float(tot[0]), int(tot[1]), inl, e2


def refit(sim, src, dst, tau2, **kw):
    """The candidate of one round over the inliers of `sim` -> (sim, valid, ratio), or None with fewer than 3 inliers."""
    _, inl = distance(sim, src, dst, tau2)
    w = inl[0].astype(float)[:, None]
    if inl.sum() < 3:
        return None
    with np.errstate(all="ignore"):
        cen = chunk_sum(np.hstack([np.where(w > 0, src, 0.0), np.where(w > 0, dst, 0.0), w]))
        cs, cd = cen[:3] / cen[6], cen[3:6] / cen[6]
        a, b = src - cs, dst - cd
        terms = [b[:, r] * a[:, c] for r in range(3) for c in range(3)] + [(a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]]
        mom = chunk_sum(np.where(w > 0, np.stack(terms, 1), 0.0))
    return fit(mom[:9], mom[9], cs, cd, **kw)


# ------------------------------------------------------------------------------------------------ sampling

def sample3(seed, prob_index, n_hyp, n):
    """picks [n_hyp, 3] and ok [n_hyp] of the problem with global index prob_index."""
    h = np.arange(n_hyp, dtype=np.uint64)
    base = pcg((pcg((np.uint64(seed & 0xFFFFFFFF) + pcg(np.uint64(prob_index & 0xFFFFFFFF))) & M32) + h) & M32)
    picks = np.zeros((n_hyp, 3), np.int64)
    ok = np.ones(n_hyp, bool)
    for k in range(3):
        chosen = np.full(n_hyp, -1, np.int64)
        for t in range(8):
            i = ((pcg((base + np.uint64(8 * k + t)) & M32) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)
            dup = (picks[:, :k] == i[:, None]).any(axis=1)
            chosen = np.where((chosen < 0) & ~dup, i, chosen)
        ok &= chosen >= 0
        picks[:, k] = np.maximum(chosen, 0)
    return picks, ok


# ------------------------------------------------------------------------------------------------ the restatement: one problem

def rel_gap(a, b):
    return abs(a - b) / max(abs(a), abs(b), 1e-300)


def align_problem(src, dst, prob_index, tau, n_hyp=256, min_points=3, min_inliers=3, refit_iters=2, with_scale=True, seed=0,
                  collinear_tol=1e-6):
    """-> dict(sim [13], cost, inlier [n] u8, info [4], rank_cost [n_hyp], margins): margins holds the smallest |e - tau| / tau
    over the rows of every model that decided something (tau), the relative gap of the ranking cost of the best hypothesis over
    other rows than the winner's (runner_up; inf without one), the smallest factor of lambda2 / lambda1 from collinear_tol^2 (ratio) and the smallest relative
    gap of a refit's cost from the cost it was compared with, refits that reproduced the current model left out (accept)."""
    src, dst = np.asarray(src, float).reshape(-1, 3), np.asarray(dst, float).reshape(-1, 3)
    n, tau2 = len(src), tau * tau
    kw = dict(with_scale=with_scale, collinear_tol=collinear_tol)
    margins = dict(tau=math.inf, runner_up=math.inf, ratio=math.inf, accept=math.inf)
    nonfinite = NONFINITE if not (np.isfinite(src).all() and np.isfinite(dst).all()) else 0
    out = dict(sim=np.full(13, math.nan), cost=math.nan, inlier=np.zeros(n, np.uint8), rank_cost=np.full(n_hyp, math.inf),
               margins=margins)
    if n < max(min_points, 3):
        out["info"] = np.array([TOO_FEW | nonfinite, 0, -1, 0], np.int32)
        return out

    def seen(e2):
        e = np.sqrt(e2[np.isfinite(e2)])
        if e.size:
            margins["tau"] = min(margins["tau"], float(np.abs(e - tau).min() / tau))

    picks, ok = sample3(seed, prob_index, n_hyp, n)
    picks = np.sort(picks, axis=1)      # the rows enter the fit in ascending order
    sims = np.full((n_hyp, 13), math.nan)
    for h in range(n_hyp):
        S, D = src[picks[h]], dst[picks[h]]
        if not (ok[h] and np.isfinite(S).all() and np.isfinite(D).all()):
            continue
        sim, valid, ratio = fit_rows(S, D, **kw)
        margins["ratio"] = min(margins["ratio"], factor_from(ratio, collinear_tol * collinear_tol))
        if valid:
            sims[h] = sim
    valid = np.isfinite(sims[:, 0])
    # the ranking cost: rows ascending inside a chunk, chunks ascending
    e2, inl = distance(np.where(valid[:, None], sims, 0.0), src, dst, tau2)
    term = np.where(inl, e2, tau2)
    rank = np.zeros(n_hyp)
    for c0 in range(0, n, CHUNK):
        part = np.zeros(n_hyp)
        for j in range(c0, min(n, c0 + CHUNK)):
            part = part + term[:, j]
        rank = rank + part
    rank = np.where(valid, rank, math.inf)
    out["rank_cost"] = rank
    n_valid = int(valid.sum())
    if n_valid == 0:
        out["info"] = np.array([NO_MODEL | nonfinite, 0, -1, 0], np.int32)
        return out
    best_h = int(np.argmin(rank))      # (the first of equal minima)
    others = rank[np.isfinite(rank) & (picks != picks[best_h]).any(axis=1)]      # (the same three rows: the same bits, an exact tie)
    if others.size:
        margins["runner_up"] = (others.min() - rank[best_h]) / max(rank[best_h], 1e-300)
    sim = sims[best_h].copy()
    cost, n_in, inl, e2 = model_cost(sim, src, dst, tau2)
    seen(e2)
    for _ in range(refit_iters):
        cand = refit(sim, src, dst, tau2, **kw)
        if cand is None:
            continue
        csim, cvalid, ratio = cand
        margins["ratio"] = min(margins["ratio"], factor_from(ratio, collinear_tol * collinear_tol))
        if not cvalid:
            continue
        cn, cn_in, cinl, ce2 = model_cost(csim, src, dst, tau2)
        seen(ce2)
        if not np.allclose(csim, sim, rtol=1e-12, atol=1e-12):
            margins["accept"] = min(margins["accept"], rel_gap(cn, cost))
        if np.isfinite(cn) and cn < cost:
            sim, cost, n_in, inl = csim, cn, cn_in, cinl
    flags = nonfinite | (WEAK if n_in < min_inliers else 0)
    out.update(sim=sim, cost=cost, inlier=inl.astype(np.uint8), info=np.array([flags, n_in, best_h, n_valid], np.int32))
    return out


def align_numpy(src, dst, ptr, tau, prob_base=0, **kw):
    """-> (sim [n_prob, 13], cost [n_prob], inlier [N], info [n_prob, 4], per-problem results)."""
    src, dst = np.asarray(src, float).reshape(-1, 3), np.asarray(dst, float).reshape(-1, 3)
    ptr = np.asarray(ptr, np.int64)
    res = [align_problem(src[ptr[q]:ptr[q + 1]], dst[ptr[q]:ptr[q + 1]], prob_base + q, tau, **kw) for q in range(len(ptr) - 1)]
    inlier = np.zeros(len(src), np.uint8)
    for q, r in enumerate(res):
        inlier[ptr[q]:ptr[q + 1]] = r["inlier"]
    n_prob = len(res)
    return (np.array([r["sim"] for r in res]).reshape(n_prob, 13), np.array([r["cost"] for r in res]).reshape(n_prob), inlier,
            np.array([r["info"] for r in res], np.int32).reshape(n_prob, 4), res)


def apply_numpy(sim, points=None, extrinsics=None):
    """mm_apply_similarity on host arrays -> (points, extrinsics), new arrays; a non-finite sim returns copies."""
    sim = np.asarray(sim, float).reshape(13)
    P = None if points is None else np.array(points, float).reshape(-1, 3)
    E = None if extrinsics is None else np.array(extrinsics, float).reshape(-1, 3, 4)
    if not np.isfinite(sim).all():
        return P, E
    s, R, d = sim[0], sim[1:10].reshape(3, 3), sim[10:]
    if P is not None:
        A = s * R
        P = np.stack([((A[r, 0] * P[:, 0] + A[r, 1] * P[:, 1]) + A[r, 2] * P[:, 2]) + d[r] for r in range(3)], 1)
    if E is not None:
        Rc, tc = E[:, :, :3], E[:, :, 3]
        N = np.stack([np.stack([(Rc[:, i, 0] * R[j, 0] + Rc[:, i, 1] * R[j, 1]) + Rc[:, i, 2] * R[j, 2] for j in range(3)], 1)
                      for i in range(3)], 1)
        t = np.stack([s * tc[:, i] - ((N[:, i, 0] * d[0] + N[:, i, 1] * d[1]) + N[:, i, 2] * d[2]) for i in range(3)], 1)
        E = np.concatenate([N, t[:, :, None]], axis=2)
    return P, E


def centres_numpy(ext):
    E = np.asarray(ext, float).reshape(-1, 3, 4)
    return np.stack([-((E[:, 0, c] * E[:, 0, 3] + E[:, 1, c] * E[:, 1, 3]) + E[:, 2, c] * E[:, 2, 3]) for c in range(3)], 1)


# ------------------------------------------------------------------------------------------------ the second route

def umeyama_svd(src, dst, with_scale=True):
    """Umeyama 1991 through numpy.linalg.svd -> sim [13]."""
    src, dst = np.asarray(src, float), np.asarray(dst, float)
    cs, cd = src.mean(0), dst.mean(0)
    a, b = src - cs, dst - cd
    U, sg, Vt = np.linalg.svd(b.T @ a)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
    R = U @ D @ Vt
    s = float((sg * np.diag(D)).sum() / (a * a).sum()) if with_scale else 1.0
    return np.concatenate([[s], R.ravel(), cd - s * R @ cs])


def random_rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def random_similarity(rng, with_scale=True):
    s = float(rng.uniform(0.5, 3.0)) if with_scale else 1.0
    return np.concatenate([[s], random_rotation(rng).ravel(), rng.uniform(-4.0, 4.0, 3)])


def sim_gap(a, b, spread=1.0):
    """(relative gap on s, absolute on R, on d relative to `spread`)."""
    a, b = np.asarray(a, float).reshape(-1, 13), np.asarray(b, float).reshape(-1, 13)
    return (float(np.max(np.abs(a[:, 0] - b[:, 0]) / np.abs(b[:, 0]))), float(np.abs(a[:, 1:10] - b[:, 1:10]).max()),
            float(np.abs(a[:, 10:] - b[:, 10:]).max() / spread))


def spread_of(dst):
    dst = np.asarray(dst, float)
    dst = dst[np.isfinite(dst).all(axis=1)]
    return float(np.sqrt(((dst - dst.mean(0)) ** 2).sum(1).mean())) if len(dst) else 1.0


# ------------------------------------------------------------------------------------------------ fixtures

TAU = 0.01
NOISE = 1e-3


def corrupted(dst_true, n_out, rng):
    """dst with uniform noise of at most NOISE per coordinate and n_out rows displaced by 0.5 .. 2 -> (dst, truth mask)."""
    n = len(dst_true)
    dst = dst_true + rng.uniform(-NOISE, NOISE, (n, 3))
    bad = rng.permutation(n)[:n_out]
    v = rng.normal(size=(n_out, 3))
    dst[bad] += v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (n_out, 1))
    truth = np.ones(n, bool)
    truth[bad] = False
    return dst, truth


def transformed(sim, src):
    return sim[0] * src @ sim[1:10].reshape(3, 3).T + sim[10:]


@functools.lru_cache(maxsize=None)
def fixture(name):
    """-> dict(src, dst, truth, sim_true): 'orbit' 80 camera centres on a wobbling circle, 30 % outliers; 'small' 12 rows, 25 %;
    'random' 5000 rows, 50 %."""
    n, frac, seed = dict(orbit=(80, 0.30, 11), small=(12, 0.25, 12), random=(5000, 0.50, 13))[name]
    rng = np.random.default_rng(seed)
    if name == "orbit":
        a = np.linspace(0.0, 2.0 * np.pi, n, endpoint=False)
        src = np.stack([np.cos(a), 0.1 * np.sin(3.0 * a), np.sin(a)], 1)
    else:
        src = rng.uniform(-1.0, 1.0, (n, 3))
    sim = random_similarity(rng)
    dst, truth = corrupted(transformed(sim, src), int(round(frac * n)), rng)
    return dict(src=src, dst=dst, truth=truth, sim_true=sim)


@functools.lru_cache(maxsize=None)
def fixture_result(name):
    fx = fixture(name)
    return align_problem(fx["src"], fx["dst"], 0, TAU)


SHAPE_N = (0, 1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193)      # tile and chunk edges
SHAPE_HYP = (1, 63, 64, 65, 256)
MIXED = (4097, 0, 3, 300)


@functools.lru_cache(maxsize=None)
def shape_problem(n, seed=0, with_scale=True):
    """n rows under a random similarity, noise as above, 30 % outliers from 8 rows on -> (src, dst)."""
    rng = np.random.default_rng(1000 + 17 * n + seed)
    src = rng.uniform(-1.0, 1.0, (n, 3))
    dst, _ = corrupted(transformed(random_similarity(rng, with_scale), src), int(0.3 * n) if n >= 8 else 0, rng)
    return src, dst


@functools.lru_cache(maxsize=None)
def shape_result(n, n_hyp=256, seed=0, with_scale=True, prob_index=0):
    src, dst = shape_problem(n, seed, with_scale)
    return align_problem(src, dst, prob_index, TAU, n_hyp=n_hyp, with_scale=with_scale)


def check_margins(res):
    """The conditions under which the GPU's discrete outputs are compared exactly."""
    m = res["margins"]
    assert m["tau"] >= 1e-6 and m["ratio"] >= 2.0 and m["accept"] >= 1e-9 and m["runner_up"] >= 1e-9, m


# ------------------------------------------------------------------------------------------------ the fit

@pytest.mark.parametrize("seed", range(12))
def test_fit_equals_umeyama_through_svd(seed):
    rng = np.random.default_rng(seed)
    worst = [0.0, 0.0, 0.0]
    for case in range(16):
        n = int(rng.integers(3, 40))
        src = rng.uniform(-1.0, 1.0, (n, 3))
        if case % 3 == 0:
            src[:, 2] *= 1e-3      # nearly planar
        sim = random_similarity(rng)
        dst = transformed(sim, src) + (rng.normal(size=(n, 3)) * 1e-2 if case % 2 else 0.0)
        got, ok, _ = fit_rows(src, dst)
        assert ok
        R = got[1:10].reshape(3, 3)
        assert abs(np.linalg.det(R) - 1.0) < 1e-12 and np.abs(R @ R.T - np.eye(3)).max() < 1e-12
        worst = [max(w, g) for w, g in zip(worst, sim_gap(got, umeyama_svd(src, dst)))]
        rigid, ok, _ = fit_rows(src, dst, with_scale=False)
        assert ok and rigid[0] == 1.0 and np.abs(rigid[1:10] - got[1:10]).max() == 0.0
    assert max(worst) < 1e-11, worst      # (the issue's prototype measured 5.2e-14 on 200 such sets)


def test_fit_of_a_reflection_prone_set_is_a_rotation():
    # dst is a mirror image of src plus noise: det(sum b a^T) < 0, where Umeyama flips the last singular vector
    rng = np.random.default_rng(5)
    for n in (3, 4, 20):
        src = rng.uniform(-1, 1, (n, 3))
        dst = src * np.array([1.0, 1.0, -1.0]) + rng.normal(size=(n, 3)) * 0.05
        a, b = src - src.mean(0), dst - dst.mean(0)
        assert n == 3 or np.linalg.det(b.T @ a) < 0
        got, ok, _ = fit_rows(src, dst)
        assert ok and abs(np.linalg.det(got[1:10].reshape(3, 3)) - 1.0) < 1e-12
        assert max(sim_gap(got, umeyama_svd(src, dst))) < 1e-11


def test_collinear_rows_are_invalid_on_either_side():
    rng = np.random.default_rng(7)
    t = rng.uniform(-1, 1, (9, 1))
    line = np.array([0.3, -0.2, 0.9]) * t + np.array([1.0, 2.0, 3.0])
    cloud = rng.uniform(-1, 1, (9, 3))
    assert not fit_rows(line, cloud)[1] and not fit_rows(cloud, line)[1] and not fit_rows(line, line)[1]
    assert not fit_rows(line[:3], cloud[:3])[1] and not fit_rows(cloud[:3], line[:3])[1]
    assert fit_rows(cloud, transformed(random_similarity(rng), cloud))[1]
    # all rows equal: var = 0
    assert not fit_rows(np.ones((4, 3)), cloud[:4])[1]
    res = align_problem(line, line * 2.0 + 1.0, 0, TAU)
    assert res["info"][0] == NO_MODEL and res["info"][2] == -1 and res["info"][3] == 0 and np.isnan(res["sim"]).all()
    assert not res["inlier"].any() and np.isnan(res["cost"])


# ------------------------------------------------------------------------------------------------ RANSAC

@pytest.mark.parametrize("name", ["orbit", "small", "random"])
def test_fixture_is_recovered_with_every_hypothesis_valid(name):
    fx, res = fixture(name), fixture_result(name)
    flags, n_in, best_h, n_valid = res["info"]
    assert flags == 0 and n_valid == 256 and 0 <= best_h < 256
    assert np.array_equal(res["inlier"].astype(bool), fx["truth"]) and n_in == fx["truth"].sum()
    g = sim_gap(res["sim"], fx["sim_true"], spread_of(fx["dst"]))
    assert max(g) < 5.0 * NOISE, g      # (the noise is NOISE per coordinate)
    check_margins(res)


def test_flags():
    src, dst = shape_problem(300)
    assert align_problem(src[:2], dst[:2], 0, TAU)["info"].tolist() == [TOO_FEW, 0, -1, 0]
    assert align_problem(src[:5], dst[:5], 0, TAU, min_points=6)["info"][0] == TOO_FEW
    assert align_problem(src, dst, 0, TAU, min_inliers=299)["info"][0] == WEAK
    bad = dst.copy()
    bad[::7, 1] = math.nan
    res = align_problem(src, bad, 0, TAU)
    assert res["info"][0] == NONFINITE and not res["inlier"][::7].any() and res["info"][1] == res["inlier"].sum()
    assert align_problem(src[:2], bad[:2], 0, TAU)["info"][0] == TOO_FEW | NONFINITE
    rigid = align_problem(*shape_problem(300, 0, False), 0, TAU, with_scale=False)
    assert rigid["sim"][0] == 1.0 and rigid["info"][0] == 0 and rigid["info"][1] >= 200


def test_sampling_with_three_picks():
    picks, ok = sample3(0, 0, 4096, 5000)
    assert ok.all() and (picks >= 0).all() and (picks < 5000).all()
    assert (picks[:, 0] != picks[:, 1]).all() and (picks[:, 0] != picks[:, 2]).all() and (picks[:, 1] != picks[:, 2]).all()
    p3, ok3 = sample3(0, 0, 4096, 3)      # three rows: the last pick fails for (2 / 3)^8 = 3.9 % of the hypotheses
    assert 0.01 < 1.0 - ok3.mean() < 0.08 and (np.sort(p3[ok3], axis=1) == np.arange(3)).all()
    assert not np.array_equal(sample3(0, 1, 64, 5000)[0], picks[:64]) and not np.array_equal(sample3(1, 0, 64, 5000)[0], picks[:64])


def test_sub_block_with_prob_base_gives_the_rows_of_the_whole_call():
    parts = [shape_problem(n) for n in (65, 3, 300)]
    src, dst = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    ptr = np.array([0, 65, 68, 368])
    whole = align_numpy(src, dst, ptr, TAU, n_hyp=64)
    sub = align_numpy(src[65:], dst[65:], ptr[1:] - 65, TAU, prob_base=1, n_hyp=64)
    assert np.array_equal(whole[0][1:], sub[0]) and np.array_equal(whole[3][1:], sub[3]) and np.array_equal(whole[2][65:], sub[2])


@pytest.mark.parametrize("n", SHAPE_N)
def test_conditions_on_the_row_count_fixtures(n):
    res = shape_result(n)
    check_margins(res)
    if n < 3:
        assert res["info"][0] == TOO_FEW
    else:
        assert res["info"][0] == 0 and res["info"][1] >= n - int(0.3 * n) - 1


@pytest.mark.parametrize("n_hyp", SHAPE_HYP)
def test_conditions_on_the_hypothesis_count_fixtures(n_hyp):
    res = shape_result(300, n_hyp)
    check_margins(res)
    assert res["info"][3] == n_hyp


def test_conditions_on_the_mixed_call():
    for q, n in enumerate(MIXED):
        check_margins(shape_result(n, 256, 0, True, q))
    check_margins(shape_result(300, 256, 0, False))


# ------------------------------------------------------------------------------------------------ apply

def test_apply_and_centres_against_direct_numpy():
    rng = np.random.default_rng(3)
    sim = random_similarity(rng)
    s, R, d = sim[0], sim[1:10].reshape(3, 3), sim[10:]
    X = rng.uniform(-1, 1, (40, 3)) + np.array([0.0, 0.0, 6.0])
    ext = np.stack([np.concatenate([random_rotation(rng) @ np.eye(3), rng.uniform(-0.3, 0.3, (3, 1))], 1) for _ in range(6)])
    Xn, En = apply_numpy(sim, X, ext)
    assert np.abs(Xn - (s * X @ R.T + d)).max() < 1e-14
    assert np.abs(En[:, :, :3] - ext[:, :, :3] @ R.T).max() < 1e-15
    assert np.abs(En[:, :, 3] - (s * ext[:, :, 3] - (ext[:, :, :3] @ R.T) @ d)).max() < 1e-14
    # projections K [R|t] X are unchanged
    K = np.array([[800.0, 0.5, 320.0], [0.0, 790.0, 240.0], [0.0, 0.0, 1.0]])

    def project(E, P):
        y = np.einsum("ij,fjk,pk->fpi", K, E, np.concatenate([P, np.ones((len(P), 1))], 1))
        return y[..., :2] / y[..., 2:]
    assert np.abs(project(En, Xn) - project(ext, X)).max() < 1e-9
    # the centres move like points
    assert np.abs(centres_numpy(En) - apply_numpy(sim, centres_numpy(ext))[0]).max() < 1e-13
    assert np.abs(centres_numpy(ext) - np.stack([-E[:, :3].T @ E[:, 3] for E in ext])).max() < 1e-15
    Xs, Es = apply_numpy(np.full(13, math.nan), X, ext)
    assert np.array_equal(Xs, X) and np.array_equal(Es, ext)


# ------------------------------------------------------------------------------------------------ options (no device)

def test_align_option_validation():
    from meatmodeler_amd import pipeline
    assert pipeline.align_options(None) is None
    ext = np.tile(np.eye(4)[:3], (4, 1, 1))
    ext[:, :, 3] = np.arange(12).reshape(4, 3)
    o = pipeline.align_options(dict(frames=[0, 2, 3, 5], extrinsics=ext), 6)
    assert o["params"] == dict(tau_rel=0.05) and np.array_equal(o["centres"], -ext[:, :, 3]) and o["frames"].tolist() == [0, 2, 3, 5]
    assert pipeline.align_options(dict(frames=[0, 1, 2], centres=np.zeros((3, 3)), tau=0.1, n_hyp=8))["params"] == dict(tau=0.1, n_hyp=8)
    for bad in (dict(frames=[0, 1], centres=np.zeros((2, 3))), dict(frames=[0, 1, 1], centres=np.zeros((3, 3))),
                dict(frames=[0, 1, 9], centres=np.zeros((3, 3))), dict(frames=[0, 1, 2]), dict(centres=np.zeros((3, 3))),
                dict(frames=[0, 1, 2], centres=np.zeros((3, 3)), extrinsics=ext[:3]), dict(frames=[0, 1, 2], centres=np.zeros((4, 3))),
                dict(frames=[0, 1, 2], centres=np.zeros((3, 3)), tau=1.0, tau_rel=0.1), dict(frames=[0, 1, 2], centres=np.zeros((3, 3)), bogus=1),
                [0, 1, 2]):
        with pytest.raises(ValueError):
            pipeline.align_options(bad, 6)
