"""CPU: NumPy restatements of mm_verify_homography and mm_recover_poses_homography (include/meatmodeler.h), the fixtures of
tests/test_homography_pairs_gpu.py with the margin conditions that file relies on, and the library checks that need no GPU.

The restatements follow the header's order of operations: the workgroup's summation order (block_sum), the reduced DLT with
every product-sum bracketed as written there, the cyclic Jacobi, the adjugate written out.  Only the ranking cost of a
hypothesis is summed by numpy (the kernel sums it over j ascending): the margin on the two lowest costs covers that.  The
second route for the fit is the SVD of the 2n x 9 DLT under the same normalisation.

Recorded here (this file's fixtures, the restatement alone):
  noise-free planar / rotation-only matches: H against K (R + t n^T / d) K^-1 within 7.5e-15, the true (R, t / d, n) among the
  four candidates within 3.0e-15, the two routes of the fit within 1.7e-14 of each other; on the six-pair fixture (0.25 px of
  noise, final inlier sets) the two fits send no inlier more than 1.5e-3 px apart: they minimise the same algebraic residual
  under |h3| = 1 and under |h| = 1;
  six-pair fixture, n_H / n_F (n_F from the restatement of mm_verify_matches): planar 0.970, rotation 0.970, planar-64 1.000,
  mixed 0.744, planar-17 1.000; the general pair's best homography explains 12 of its 256 matches and is WEAK;
  sqrt(l1 / l3) - 1: planar 0.151 .. 0.159, rotation 3.3e-4;
  true inliers kept / outliers kept by the homography: SIX_COUNTS;
  closest margins over every fixture the GPU file compares exactly: 0.27 px from tau, best / second cost 1.2e-3, refit
  decision 1.8e-4, sampled triples a factor 15 from collinear_tol = 1e-6 (56 on the grid at the default 1e-3).
"""
import ctypes as C
import functools
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_verify_matches_cpu import CAP, K_SCENE, scene_cameras, verify_numpy  # noqa: E402
from test_recover_poses_cpu import (POSE_AMBIGUOUS, POSE_MALFORMED, POSE_NO_MODEL, POSE_TOO_FEW, CHAIN_FEW_COMMON,  # noqa: E402
                                    chain_numpy, cross3, dot3, fundamental, mat3, recover_pair)
from oracle.geom_oracle import (TRIPLES, block_sum, factor_from, jacobi, jacobi3, k_inverse, pcg, plane_dlt,  # noqa: E402
                                plane_terms, polar3, triple_measure)
from meatmodeler_amd import synth  # noqa: E402

TOO_FEW, NO_MODEL, WEAK, MALFORMED, DEGENERATE = 1, 2, 4, 8, 16      # MM_HOMOG_*
ROTATION = 16                                                        # MM_HPOSE_ROTATION
SQRT2 = 1.4142135623730951
M32 = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------ restatement: the homography

def sample4(seed, pair_index, n_hyp, m):
    """picks [n_hyp, 4] and ok [n_hyp] of the pair with global index pair_index (the integer scheme with four picks)."""
    h = np.arange(n_hyp, dtype=np.uint64)
    base = pcg(pcg(np.uint64(seed & M32) + pcg(np.uint64(pair_index & M32))) + h)
    picks = np.zeros((n_hyp, 4), np.int64)
    ok = np.ones(n_hyp, bool)
    for k in range(4):
        chosen = np.full(n_hyp, -1, np.int64)
        for a in range(8):
            i = ((pcg(base + np.uint64(8 * k + a)) * np.uint64(m)) >> np.uint64(32)).astype(np.int64)
            dup = (picks[:, :k] == i[:, None]).any(axis=1)
            chosen = np.where((chosen < 0) & ~dup, i, chosen)
        ok &= chosen >= 0
        picks[:, k] = np.maximum(chosen, 0)
    return picks, ok


def adjugate(H):
    H = np.asarray(H, float)
    h = [H[..., k] for k in range(9)]
    return np.stack([h[4] * h[8] - h[5] * h[7], h[2] * h[7] - h[1] * h[8], h[1] * h[5] - h[2] * h[4],
                     h[5] * h[6] - h[3] * h[8], h[0] * h[8] - h[2] * h[6], h[2] * h[3] - h[0] * h[5],
                     h[3] * h[7] - h[4] * h[6], h[1] * h[6] - h[0] * h[7], h[0] * h[4] - h[1] * h[3]], axis=-1)


def transfer(H, x, xp):
    """d^2 [..., n] of H [..., 9] over matches x, xp [n, 2]: the symmetric transfer distance of the header."""
    H = np.asarray(H, float)
    A = adjugate(H)[..., None, :]
    H = H[..., None, :]
    with np.errstate(all="ignore"):
        y0 = (H[..., 0] * x[:, 0] + H[..., 1] * x[:, 1]) + H[..., 2]
        y1 = (H[..., 3] * x[:, 0] + H[..., 4] * x[:, 1]) + H[..., 5]
        y2 = (H[..., 6] * x[:, 0] + H[..., 7] * x[:, 1]) + H[..., 8]
        z0 = (A[..., 0] * xp[:, 0] + A[..., 1] * xp[:, 1]) + A[..., 2]
        z1 = (A[..., 3] * xp[:, 0] + A[..., 4] * xp[:, 1]) + A[..., 5]
        z2 = (A[..., 6] * xp[:, 0] + A[..., 7] * xp[:, 1]) + A[..., 8]
        ex, ey, fx, fy = xp[:, 0] - y0 / y2, xp[:, 1] - y1 / y2, x[:, 0] - z0 / z2, x[:, 1] - z1 / z2
        return ((ex * ex + ey * ey) + (fx * fx + fy * fy)) * 0.5


def inliers(d2, tau2):
    with np.errstate(all="ignore"):
        return np.isfinite(d2) & (d2 <= tau2)


def block_cost(H, x, xp, tau2):
    """(cost, mask) of one H in the workgroup's summation order."""
    d2 = transfer(H, x, xp)
    inl = inliers(d2, tau2)
    v = block_sum(np.column_stack([np.where(inl, d2, tau2), inl.astype(float)]))
    return float(v[0]), inl


def hartley_block(x, xp, sel):
    """((c, s), (c', s')) over the rows sel, summed as the workgroup sums them."""
    with np.errstate(all="ignore"):
        one = np.ones(len(x))
        s5 = block_sum(np.where(sel[:, None], np.column_stack([one, x, xp]), 0.0))
        n = s5[0]
        c, c2 = s5[1:3] / n, s5[3:5] / n
        d = np.column_stack([np.sqrt((x[:, 0] - c[0]) * (x[:, 0] - c[0]) + (x[:, 1] - c[1]) * (x[:, 1] - c[1])),
                             np.sqrt((xp[:, 0] - c2[0]) * (xp[:, 0] - c2[0]) + (xp[:, 1] - c2[1]) * (xp[:, 1] - c2[1]))])
        dd = block_sum(np.where(sel[:, None], d, 0.0))
        return (c, SQRT2 / (dd[0] / n)), (c2, SQRT2 / (dd[1] / n))


def solve_h(acc, c, s, c2, s2):
    """The reduced DLT on a batch of sums acc [B, 24] under one normalisation -> (H [B, 9], ok [B])."""
    acc = np.asarray(acc, float)
    B = acc.shape[0]
    h1, h2, h3, ok = plane_dlt(acc)
    with np.errstate(all="ignore"):
        Hn = [h1[0], h1[1], h1[2], h2[0], h2[1], h2[2], h3[0], h3[1], h3[2]]
        G = [[(Hn[r] * Hn[cc] + Hn[3 + r] * Hn[3 + cc]) + Hn[6 + r] * Hn[6 + cc] for cc in range(3)] for r in range(3)]
        jacobi(G, 3)
        lo = np.where(G[0][0] < G[1][1], G[0][0], G[1][1])
        hi = np.where(G[0][0] > G[1][1], G[0][0], G[1][1])
        lo, hi = np.where(lo < G[2][2], lo, G[2][2]), np.where(hi > G[2][2], hi, G[2][2])
        ok &= lo > 1e-8 * hi
        A = [None] * 9
        for r in range(3):
            A[3 * r] = s * Hn[3 * r]
            A[3 * r + 1] = s * Hn[3 * r + 1]
            A[3 * r + 2] = (Hn[3 * r + 2] - (s * c[0]) * Hn[3 * r]) - (s * c[1]) * Hn[3 * r + 1]
        H = [None] * 9
        for cc in range(3):
            H[cc] = A[cc] / s2 + c2[0] * A[6 + cc]
            H[3 + cc] = A[3 + cc] / s2 + c2[1] * A[6 + cc]
            H[6 + cc] = A[6 + cc]
        nn = np.zeros(B)
        for k in range(9):
            nn = nn + H[k] * H[k]
        w = (H[6] * c[0] + H[7] * c[1]) + H[8]
        inv = np.where(w < 0.0, -1.0, 1.0) / np.sqrt(nn)
        H = np.stack([H[k] * inv for k in range(9)], axis=1)
    ok &= np.isfinite(H).all(axis=1)
    return H, ok


def svd_fit(x, xp, sel):
    """The second route: the 2n x 9 DLT by SVD over the rows sel under their Hartley normalisation -> H [9], unit norm, the
    header's sign."""
    (c, s), (c2, s2) = hartley_block(x, xp, sel)
    a, b = s * (x[sel] - c), s2 * (xp[sel] - c2)
    one, zero = np.ones(len(a)), np.zeros(len(a))
    rows = np.vstack([np.column_stack([a[:, 0], a[:, 1], one, zero, zero, zero, -b[:, 0] * a[:, 0], -b[:, 0] * a[:, 1], -b[:, 0]]),
                      np.column_stack([zero, zero, zero, a[:, 0], a[:, 1], one, -b[:, 1] * a[:, 0], -b[:, 1] * a[:, 1], -b[:, 1]])])
    Hn = np.linalg.svd(rows)[2][-1].reshape(3, 3)
    T = np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1]])
    T2i = np.array([[1 / s2, 0, c2[0]], [0, 1 / s2, c2[1]], [0, 0, 1]])
    H = (T2i @ Hn @ T).ravel()
    H = H / np.linalg.norm(H)
    return -H if (H[6] * c[0] + H[7] * c[1]) + H[8] < 0 else H


def homography_pair(x, xp, wf, pair_index, verify_row=None, n_hyp=256, threshold_px=2.0, min_matches=8, min_inliers=16,
                    refit_iters=2, seed=0, collinear_tol=1e-3, degenerate_frac=0.8):
    """One pair: x, xp [m, 2] f64 (rows of malformed matches NaN), wf [m] bool, verify_row = (flags, n_F, ..) or None
    -> dict(flags, n_inliers, best_h, n_valid, n_F, H [9], cost, mask, and for the margin conditions: tau_gap (px),
    cost_gap, refit_gaps, triple_factor, ratio)."""
    mm = len(x)
    tau2 = float(threshold_px) ** 2
    out = dict(flags=0 if wf.all() else MALFORMED, n_inliers=0, best_h=-1, n_valid=0, n_F=-1 if verify_row is None else int(verify_row[1]),
               H=np.full(9, np.nan), cost=np.nan, mask=np.zeros(mm, bool), tau_gap=np.inf, cost_gap=np.inf, refit_gaps=[],
               triple_factor=np.inf, ratio=np.nan)
    if mm < max(int(min_matches), 8):
        out["flags"] |= TOO_FEW
        return out
    picks, ok = sample4(seed, pair_index, n_hyp, mm)
    ok &= wf[picks].all(axis=1)
    (c, s), (c2, s2) = hartley_block(x, xp, wf)
    ok &= bool(np.isfinite(s) and np.isfinite(s2))
    Hh = np.full((n_hyp, 9), np.nan)
    cost_h = np.full(n_hyp, np.inf)
    if ok.any():
        hs = np.nonzero(ok)[0]
        with np.errstate(all="ignore"):
            xa, xb = s * (x[picks[hs]] - c), s2 * (xp[picks[hs]] - c2)      # [B, 4, 2]
        acc = np.zeros((len(hs), 24))
        for k in range(4):
            acc = acc + plane_terms(xa[:, k, 0], xa[:, k, 1], xb[:, k, 0], xb[:, k, 1])
        good = np.ones(len(hs), bool)
        for pts in (xa, xb):
            for (i, j, k) in TRIPLES:
                cr, lng = triple_measure(pts[:, i, 0], pts[:, i, 1], pts[:, j, 0], pts[:, j, 1], pts[:, k, 0], pts[:, k, 1])
                with np.errstate(all="ignore"):
                    good &= cr > collinear_tol * lng
                    meas = cr / lng
                for v in meas[np.isfinite(meas)]:
                    out["triple_factor"] = min(out["triple_factor"], factor_from(float(v), collinear_tol))
        H, valid = solve_h(acc, c, s, c2, s2)
        valid &= good
        Hh[hs[valid]] = H[valid]
        d2 = transfer(H[valid], x, xp)
        cost_h[hs[valid]] = np.where(inliers(d2, tau2), d2, tau2).sum(axis=-1)
    out["n_valid"] = int(np.isfinite(Hh[:, 0]).sum())
    fin = np.isfinite(cost_h)
    if not fin.any():
        out["flags"] |= NO_MODEL
        return out
    best = int(np.argmin(np.where(fin, cost_h, np.inf)))      # (first minimum: ties to the lowest h)
    two = np.sort(cost_h[fin])[:2]
    if len(two) == 2:
        out["cost_gap"] = (two[1] - two[0]) / two[1] if two[1] > 0 else 0.0
    H = Hh[best]
    cost, mask = block_cost(H, x, xp, tau2)
    for _ in range(int(refit_iters)):
        if mask.sum() < 4:
            break
        (ci, si), (ci2, si2) = hartley_block(x, xp, mask)
        with np.errstate(all="ignore"):
            terms = plane_terms(si * (x[:, 0] - ci[0]), si * (x[:, 1] - ci[1]), si2 * (xp[:, 0] - ci2[0]), si2 * (xp[:, 1] - ci2[1]))
        acc = block_sum(np.where(mask[:, None], terms, 0.0))
        Hn, okH = solve_h(acc[None, :], ci, si, ci2, si2)
        cn, mn = block_cost(Hn[0], x, xp, tau2)
        if np.isfinite(cn) and cost > 0 and not (Hn[0] == H).all():      # (the same inlier set gives the same bits: no decision)
            out["refit_gaps"].append(abs(cn - cost) / cost)
        if okH[0] and np.isfinite(cn) and cn < cost:
            H, cost, mask = Hn[0], cn, mn
    out.update(best_h=best, H=H, cost=float(cost), mask=mask, n_inliers=int(mask.sum()))
    d = np.sqrt(transfer(H, x, xp))
    d = d[np.isfinite(d)]
    if d.size and np.isfinite(threshold_px):
        out["tau_gap"] = float(np.abs(d - threshold_px).min())
    if out["n_inliers"] < int(min_inliers):
        out["flags"] |= WEAK
    if verify_row is not None and not out["flags"] & (TOO_FEW | NO_MODEL | WEAK):
        n_f = int(verify_row[1])
        out["ratio"] = out["n_inliers"] / n_f if n_f > 0 else np.inf
        if (int(verify_row[0]) & 7) != 0 or float(out["n_inliers"]) >= degenerate_frac * float(n_f):
            out["flags"] |= DEGENERATE
    return out


def unpack_pair(kp_xy, pairs, m, p):
    cap = kp_xy.shape[1]
    mm = int(np.clip(m[p], 0, cap))
    rows = pairs[p, :mm]
    wf = ((rows >= 0) & (rows < cap)).all(axis=1)
    x, xp = np.full((mm, 2), np.nan), np.full((mm, 2), np.nan)
    x[wf] = kp_xy[p, rows[wf, 0]]
    xp[wf] = kp_xy[p + 1, rows[wf, 1]]
    return rows, wf, x, xp


def homography_numpy(kp_xy, pairs, m, verify_info=None, pair_base=0, **kw):
    """The whole call -> list of homography_pair dicts, each with `kept` [k, 2] = the rows mm_verify_homography writes and
    `info` [6]."""
    res = []
    for p in range(pairs.shape[0]):
        rows, wf, x, xp = unpack_pair(kp_xy, pairs, m, p)
        r = homography_pair(x, xp, wf, pair_base + p, None if verify_info is None else verify_info[p], **kw)
        r["kept"] = rows[:0] if r["flags"] & (TOO_FEW | NO_MODEL | WEAK) else rows[r["mask"]]
        r["info"] = np.array([r["flags"], r["n_inliers"], r["best_h"], r["n_valid"], r["n_F"], 0], np.int32)
        res.append(r)
    return res


def sign_gap(Ha, Hb):
    return min(np.abs(Ha - Hb).max(), np.abs(Ha + Hb).max())


# ------------------------------------------------------------------------------------------------ restatement: the motion

def h_rays(K, x):
    ki = k_inverse(K)
    return [(ki[0] * x[:, 0] + ki[1] * x[:, 1]) + ki[2], ki[3] * x[:, 1] + ki[4], np.ones(len(x))]


def h_solution(G, v1, v2, v3, a1, a3, den):
    """One of the two plane solutions -> (R [9], t [3], n [3])."""
    with np.errstate(all="ignore"):
        u = (a1 * v1 + a3 * v3) / den
        n = cross3(v2, u)
        w0, w1 = np.array(mat3(G, v2)), np.array(mat3(G, u))
        w2 = cross3(w0, w1)
        R = np.array([(w0[r] * v2[c] + w1[r] * u[c]) + w2[r] * n[c] for r in range(3) for c in range(3)])
        t = np.array([((G[3 * r] - R[3 * r]) * n[0] + (G[3 * r + 1] - R[3 * r + 1]) * n[1]) + (G[3 * r + 2] - R[3 * r + 2]) * n[2]
                      for r in range(3)])
    return R, t, n


def h_depths(R, t, n, a):
    with np.errstate(all="ignore"):
        l1 = 1.0 / dot3(n, a)
        l2 = l1 * ((R[6] * a[0] + R[7] * a[1]) + R[8] * a[2]) + t[2]
        return l1, l2, np.isfinite(l1) & np.isfinite(l2) & (l1 > 0) & (l2 > 0)


def hpose_pair(x, xp, wf, H, K, hint=None, min_matches=8, min_front_frac=0.5, ambiguous_frac=0.9, rotation_tol=1e-2):
    """One pair -> dict(flags, winner, votes [4], m, R [9], t [3], sigma [3], normal [3], depth [m, 2], and for the margins
    rot (sqrt(l1 / l3) - 1), cand [4] of (R, t, n) before the division by |t|, cand_depth [4, m, 2])."""
    mm = len(x)
    nan = math.nan
    out = dict(flags=0 if wf.all() else POSE_MALFORMED, winner=-1, votes=[0, 0, 0, 0], m=mm, R=np.full(9, nan), t=np.full(3, nan),
               sigma=np.full(3, nan), normal=np.full(3, nan), depth=np.full((mm, 2), nan), rot=nan, cand=[],
               cand_depth=np.full((4, mm, 2), nan), sign_counts=(0, 0))
    if mm < max(int(min_matches), 8):
        out["flags"] |= POSE_TOO_FEW
        return out
    H = np.asarray(H, float).reshape(9)
    Kf = np.asarray(K, float).reshape(9)
    ki = k_inverse(K)
    with np.errstate(all="ignore"):
        HK = [(H[3 * r] * Kf[c] + H[3 * r + 1] * Kf[3 + c]) + H[3 * r + 2] * Kf[6 + c] for r in range(3) for c in range(3)]
        G = np.array([(ki[0] * HK[c] + ki[1] * HK[3 + c]) + ki[2] * HK[6 + c] for c in range(3)]
                     + [ki[3] * HK[3 + c] + ki[4] * HK[6 + c] for c in range(3)] + [HK[6 + c] for c in range(3)])
        M = [[(G[r] * G[c] + G[3 + r] * G[3 + c]) + G[6 + r] * G[6 + c] for c in range(3)] for r in range(3)]
        lam, V = jacobi3(M)
    lam = list(lam)
    cols = [V[:, k].copy() for k in range(3)]
    for i, j in ((0, 1), (1, 2), (0, 1)):      # descending, stable
        if lam[j] > lam[i]:
            lam[i], lam[j] = lam[j], lam[i]
            cols[i], cols[j] = cols[j], cols[i]
    model = bool(np.isfinite(H).all() and np.isfinite(lam).all() and lam[2] > 0.0)
    if not model:
        out["flags"] |= POSE_NO_MODEL
        return out
    sg = [math.sqrt(v) for v in lam]
    out["sigma"] = np.array(sg)
    G = G / sg[1]
    v1, v3 = cols[0], cols[2]
    v2 = cross3(v3, v1)
    out["rot"] = math.sqrt(lam[0] / lam[2]) - 1.0
    n1, n3 = lam[0] / lam[1], lam[2] / lam[1]
    a1, a3, den = math.sqrt(1.0 - n3), math.sqrt(n1 - 1.0), math.sqrt(n1 - n3)
    a, b = h_rays(K, x[wf]), h_rays(K, xp[wf])
    d = dot3(b, mat3(G, a))
    neg, pos = int((d < 0).sum()), int((d > 0).sum())
    out["sign_counts"] = (neg, pos)
    if neg > pos:
        G = -G
    if out["rot"] <= rotation_tol:
        R, okR = polar3(G.reshape(3, 3))
        if not (okR and np.isfinite(R).all()):
            out["flags"] |= POSE_NO_MODEL
            return out
        out["flags"] |= ROTATION
        out.update(R=R.ravel(), t=np.zeros(3))
        return out
    Rp, tp, npl = h_solution(G, v1, v2, v3, a1, a3, den)
    Rm, tm, nmi = h_solution(G, v1, v2, v3, a1, -a3, den)
    with np.errstate(all="ignore"):
        norms = [math.sqrt(dot3(tp, tp)), math.sqrt(dot3(tm, tm))]
    if not (all(np.isfinite(v) and v > 0 for v in norms) and np.isfinite(Rp).all() and np.isfinite(Rm).all()):
        out["flags"] |= POSE_NO_MODEL
        return out
    cand = [(Rp, tp, npl), (Rp, -tp, -npl), (Rm, tm, nmi), (Rm, -tm, -nmi)]
    votes, per = [], []
    for c, (R, t, n) in enumerate(cand):
        l1, l2, okc = h_depths(R, t, n, a)
        out["cand_depth"][c, wf, 0], out["cand_depth"][c, wf, 1] = l1, l2
        votes.append(int(okc.sum()))
        per.append((l1, l2, okc))
    vmax = max(votes)
    cont = [float(v) >= ambiguous_frac * float(vmax) for v in votes]
    hinted = hint is not None and bool(np.isfinite(np.asarray(hint, float)).all())
    if hinted:
        hv = np.asarray(hint, float)
        dp, dm = dot3(npl, hv), dot3(nmi, hv)
        score = [dp, -dp, dm, -dm]
        w = -1
        for c in range(4):
            if cont[c] and (w < 0 or score[c] > score[w]):
                w = c
    else:
        w = max(range(4), key=lambda c: (votes[c], -c))
    if votes[w] < min_front_frac * mm or (sum(cont) > 1 and not hinted):
        out["flags"] |= POSE_AMBIGUOUS
    R, t, n = cand[w]
    tn = math.sqrt(dot3(t, t))
    l1, l2, okc = per[w]
    dd = np.full((int(wf.sum()), 2), nan)
    dd[okc, 0], dd[okc, 1] = l1[okc] / tn, l2[okc] / tn
    out["depth"][wf] = dd
    out.update(winner=w, votes=votes, R=R, t=t / tn, normal=n, cand=cand)
    return out


def hpose_numpy(kp_xy, pairs, m, H, K, hint=None, **kw):
    """The whole call -> (R [n, 9], t [n, 3], sigma [n, 3], normal [n, 3], depth [n, cap, 2], info [n, 8], list of dicts)."""
    n, cap = pairs.shape[0], pairs.shape[1]
    R, t, sigma, normal = (np.full((n, k), np.nan) for k in (9, 3, 3, 3))
    depth, info, res = np.full((n, cap, 2), np.nan), np.zeros((n, 8), np.int32), []
    for p in range(n):
        rows, wf, x, xp = unpack_pair(kp_xy, pairs, m, p)
        r = hpose_pair(x, xp, wf, H[p], K, None if hint is None else hint[p], **kw)
        R[p], t[p], sigma[p], normal[p], depth[p, :len(x)] = r["R"], r["t"], r["sigma"], r["normal"], r["depth"]
        info[p] = [r["flags"], r["winner"]] + r["votes"] + [len(x), 0]
        res.append(r)
    return R, t, sigma, normal, depth, info, res


# ------------------------------------------------------------------------------------------------ fixtures

PLANE_N, PLANE_D = np.array([-0.3, -0.2, 1.0]), 6.0      # the plane z = 6 + 0.3 x + 0.2 y as n . X = d (n not normalised)
UNIT_N, UNIT_D = PLANE_N / np.linalg.norm(PLANE_N), PLANE_D / np.linalg.norm(PLANE_N)      # the same plane, |n| = 1
KINDS = ("general", "planar", "rotation", "mixed")


def pair_motion(p):
    """The motion of pair p of a packed call: two_view_scene's cameras, run backwards on odd pairs (so that a chain of pairs
    does not walk out of the image)."""
    R, t = scene_cameras()
    return (R, t) if p % 2 == 0 else (R.T, -R.T @ t)


def true_H(kind, p):
    """x' ~ H x of the pair's plane (or of its rotation), unit norm."""
    R, t = pair_motion(p)
    Hc = R if kind == "rotation" else R + np.outer(t, PLANE_N) / PLANE_D
    H = K_SCENE @ Hc @ np.linalg.inv(K_SCENE)
    return (H / np.linalg.norm(H)).ravel()


def move(kind, x, p, rng):
    """x [n, 2] pixels in camera 1 of pair p -> their matches in camera 2: the points sit on the plane (planar), anywhere in
    the box of depths 4 .. 9 (general; rotation, where the depth does not matter), or -- mixed -- on the plane for the first
    three quarters of the rows and in the box for the rest."""
    R, t = pair_motion(p)
    a = np.column_stack([x, np.ones(len(x))]) @ np.linalg.inv(K_SCENE).T
    on_plane = PLANE_D / (a @ PLANE_N)
    box = rng.uniform(4.0, 9.0, len(x))
    if kind == "planar":
        d = on_plane
    elif kind == "mixed":
        d = np.where(np.arange(len(x)) < (3 * len(x)) // 4, on_plane, box)
    else:
        d = box
    X2 = (a * d[:, None]) @ R.T + (0.0 if kind == "rotation" else t)
    b = X2 @ K_SCENE.T
    return b[:, :2] / b[:, 2:]


def chain_pack(specs, seed=99, noise=0.25, cap=CAP):
    """Consecutive pairs (kind, n_in, n_out) over shared key point tables: every frame holds cap key points, uniform in the
    image unless a pair wrote them; pair p takes k random slots of frame p as its query points -- whatever they hold, so the
    train points of pair p - 1 are among them -- and writes their matches into k random slots of frame p + 1: the first n_in
    (before the shuffle) under the pair's motion with `noise` px on either side, the others uniform.
    -> kp_xy [n+1, cap, 2] f32, pairs [n, cap, 2] i32 (rows beyond m: -1), m [n] i32, truth: list of [m] bool."""
    rng = np.random.default_rng(seed)
    n = len(specs)
    kp = rng.uniform([0, 0], [640, 480], (n + 1, cap, 2)).astype(np.float32)
    pairs = np.full((n, cap, 2), -1, np.int32)
    m = np.zeros(n, np.int32)
    truth = []
    for p, (kind, n_in, n_out) in enumerate(specs):
        k = n_in + n_out
        assert k <= cap and kind in KINDS
        q, t = rng.permutation(cap)[:k], rng.permutation(cap)[:k]
        x = kp[p, q].astype(np.float64)
        xp = rng.uniform([0, 0], [640, 480], (k, 2))
        xp[:n_in] = move(kind, x[:n_in] + rng.normal(0, noise, (n_in, 2)), p, rng) + rng.normal(0, noise, (n_in, 2))
        kp[p + 1, t] = xp
        order = rng.permutation(k)
        pairs[p, :k, 0], pairs[p, :k, 1] = q[order], t[order]
        m[p] = k
        truth.append((np.arange(k) < n_in)[order])
    return kp, pairs, m, truth


SIX = (("general", 160, 96), ("planar", 160, 96), ("rotation", 160, 96), ("planar", 64, 0), ("mixed", 120, 40), ("planar", 17, 0))
SIX_SEED = 3
SIX_KW = dict(n_hyp=256, threshold_px=2.0, seed=11, collinear_tol=1e-6)      # (1e-6: the sampled triples' margin, see below)
VERIFY_KW = dict(n_hyp=256, threshold_px=2.0, seed=7)
# (true inliers kept, outliers kept) by the homography of the restatement on the committed seeds; the mixed pair's plane
# holds 90 of its 120 true matches
SIX_COUNTS = ((0, 0), (160, 0), (160, 0), (64, 0), (90, 0), (17, 0))


@functools.lru_cache(maxsize=None)
def six_pairs():
    return chain_pack(SIX, seed=SIX_SEED)


@functools.lru_cache(maxsize=None)
def six_verify_info():
    """info [6, 4] of the restatement of mm_verify_matches on the six pairs (the GPU test takes the library's)."""
    kp, pairs, m, _ = six_pairs()
    res = verify_numpy(kp.astype(np.float64), pairs, m, **VERIFY_KW)
    return np.array([[r["flags"], r["n_inliers"], r["best_h"], r["n_valid"]] for r in res], np.int32)


@functools.lru_cache(maxsize=None)
def six_reference(with_info=True):
    kp, pairs, m, _ = six_pairs()
    return homography_numpy(kp.astype(np.float64), pairs, m, six_verify_info() if with_info else None, **SIX_KW)


@functools.lru_cache(maxsize=None)
def malformed_fixture():
    """Pair 3 of the six-pair call (pair_base = 3) with match 3's query index -1, match 10's train index cap and match 20's
    indices at the ends of int32."""
    kp, pairs, m, _ = six_pairs()
    bad = pairs[3:4].copy()
    bad[0, 3, 0] = -1
    bad[0, 10, 1] = CAP
    bad[0, 20] = (2 ** 31 - 1, -2 ** 31)
    return kp[3:5], bad, m[3:4]


@functools.lru_cache(maxsize=None)
def malformed_reference():
    kp, bad, m = malformed_fixture()
    return homography_numpy(kp.astype(np.float64), bad, m, pair_base=3, **SIX_KW)[0]


@functools.lru_cache(maxsize=None)
def uniform_fixture():
    """64 pairs of independent uniform pixels: whatever H wins explains few of them."""
    return chain_pack([("general", 0, 64)], seed=200)[:3]


UNIFORM_KW = dict(SIX_KW, seed=2)      # (under most keys the two best hypotheses explain their own four matches and tie at 60 tau^2)


def uniform_reference():
    kp, pairs, m = uniform_fixture()
    return homography_numpy(kp.astype(np.float64), pairs, m, np.array([[WEAK, 0, -1, 0]], np.int32), **UNIFORM_KW)[0]


INF_KW = dict(SIX_KW, threshold_px=math.inf)


@functools.lru_cache(maxsize=None)
def inf_reference():
    """Pairs 1 and 2 of the six-pair call under tau = +inf: every well-formed match is an inlier of every hypothesis."""
    kp, pairs, m, _ = six_pairs()
    return homography_numpy(kp[1:4].astype(np.float64), pairs[1:3], m[1:3], pair_base=1, **INF_KW)


BOUNDARY_M = (0, 7, 8, 9, 63, 64, 65, 255, 256, 257, CAP)
BOUNDARY_HYP = (1, 63, 64, 65, 256)
M_SEED = {9: 1}       # by m; 0 where not listed (m = 9, key 0: the two best hypotheses drew the same four matches -- a tie)
HYP_SEED = 0


def boundary_fixture(mm):
    """The single planar pair of the m-boundary tests: a quarter outliers from 63 matches on."""
    n_out = mm // 4 if mm >= 63 else 0
    return chain_pack([("planar", mm - n_out, n_out)], seed=500 + mm)


def boundary_kw(mm):
    return dict(n_hyp=64, threshold_px=2.0, seed=M_SEED.get(mm, 0), collinear_tol=1e-6)


@functools.lru_cache(maxsize=None)
def boundary_reference(mm):
    kp, pairs, m, _ = boundary_fixture(mm)
    return homography_numpy(kp.astype(np.float64), pairs, m, **boundary_kw(mm))[0]


def hyp_kw(n_hyp):
    return dict(n_hyp=n_hyp, threshold_px=2.0, seed=HYP_SEED, collinear_tol=1e-6)


@functools.lru_cache(maxsize=None)
def hyp_reference(n_hyp):
    kp, pairs, m, _ = boundary_fixture(64)
    return homography_numpy(kp.astype(np.float64), pairs, m, **hyp_kw(n_hyp))[0]


@functools.lru_cache(maxsize=None)
def grid_fixture():
    """The default collinear_tol where its margin holds by construction: a 5 x 4 grid of pixels 60 apart and its exact image
    under the plane's homography.  A triple of grid points is collinear -- |cross| / longest side^2 at rounding level, a
    factor 1e9 under 1e-3 -- or has |cross| >= one cell and sides of at most 4 x 3 cells: 1 / 25 = 0.04, a factor 40 above; a
    homography maps lines to lines, so image 2 keeps the first kind and the second stays a factor 10 away (asserted)."""
    gx, gy = np.meshgrid(np.arange(5) * 60.0 + 200.0, np.arange(4) * 60.0 + 150.0)
    x = np.column_stack([gx.ravel(), gy.ravel()])
    xp = move("planar", x, 0, np.random.default_rng(0))
    kp = np.zeros((2, CAP, 2), np.float32)
    kp[0, :20], kp[1, :20] = x, xp
    pairs = np.full((1, CAP, 2), -1, np.int32)
    pairs[0, :20] = np.arange(20)[:, None]
    return kp, pairs, np.array([20], np.int32)


GRID_KW = dict(n_hyp=64, threshold_px=2.0, seed=0, min_inliers=16)      # collinear_tol: the default


@functools.lru_cache(maxsize=None)
def grid_reference():
    kp, pairs, m = grid_fixture()
    return homography_numpy(kp.astype(np.float64), pairs, m, **GRID_KW)[0]


def exact_scene(kind, seed, n=64):
    """Noise-free matches in f64 (not through a key point table) -> (x, xp)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform([40, 40], [600, 440], (n, 2))
    return x, move(kind, x, 0, rng)


def pose_margins(r, min_front_frac=0.5, ambiguous_frac=0.9, rotation_tol=1e-2):
    """(factor of sqrt(l1 / l3) - 1 from rotation_tol, the smallest |finite candidate depth|, the distance of the vote fractions
    from the two fractions) of an hpose_pair dict."""
    rot = factor_from(r["rot"], rotation_tol) if np.isfinite(r["rot"]) else np.inf
    c = r["cand_depth"][np.isfinite(r["cand_depth"])]
    lmin = np.abs(c).min() if c.size else np.inf
    fmin = np.inf
    if r["winner"] >= 0:
        v = r["votes"]
        fmin = abs(v[r["winner"]] / r["m"] - min_front_frac)
        if max(v) > 0:
            fmin = min([fmin] + [abs(vc / max(v) - ambiguous_frac) for vc in v])
    return rot, lmin, fmin


@functools.lru_cache(maxsize=None)
def six_pose_reference(hinted=False):
    """The pose call on the homography's own output for the six pairs (NaN H where there is none)."""
    kp, pairs, m, _ = six_pairs()
    ref = six_reference()
    cap = pairs.shape[1]
    po = np.full_like(pairs, -1)
    mo = np.zeros_like(m)
    for p, r in enumerate(ref):
        mo[p] = len(r["kept"])
        po[p, :mo[p]] = r["kept"]
    H = np.array([r["H"] for r in ref])
    hint = None
    if hinted:
        hint = np.full((len(ref), 3), np.nan)
        for p in (1, 3, 5):
            hint[p] = PLANE_N
    assert cap == CAP
    return (po, mo, H, hint) + hpose_numpy(kp.astype(np.float64), po, mo, H, K_SCENE, hint)


# ------------------------------------------------------------------------------------------------ tests: truth

def rot_gap(Ra, Rb):
    return np.abs(np.asarray(Ra).reshape(3, 3) - np.asarray(Rb).reshape(3, 3)).max()


@pytest.mark.parametrize("kind", ["planar", "rotation"])
@pytest.mark.parametrize("seed", range(6))
def test_noise_free_matches_return_the_true_homography_and_motion(kind, seed):
    x, xp = exact_scene(kind, seed)
    wf = np.ones(len(x), bool)
    r = homography_pair(x, xp, wf, 0, n_hyp=32, seed=seed, collinear_tol=1e-6)
    assert r["flags"] == 0 and r["n_inliers"] == len(x)
    gap = sign_gap(r["H"], true_H(kind, 0))
    print(f"{kind} seed {seed}: |H - H_true| = {gap:.2e}, against the SVD route {sign_gap(r['H'], svd_fit(x, xp, wf)):.2e}")
    assert gap <= 1e-9
    assert sign_gap(r["H"], svd_fit(x, xp, wf)) <= 1e-9
    R, t = pair_motion(0)
    q = hpose_pair(x, xp, wf, r["H"], K_SCENE)
    if kind == "rotation":
        assert q["flags"] == ROTATION and q["winner"] == -1 and rot_gap(q["R"], R) <= 1e-9 and (q["t"] == 0).all()
        assert np.isnan(q["depth"]).all() and np.isnan(q["normal"]).all()
        return
    # the true (R, t / d, n) is among the four candidates, n the unit normal and d the distance of the plane n . X = d
    best = min(max(rot_gap(Rc, R), np.abs(tc - t / UNIT_D).max(), np.abs(nc - UNIT_N).max()) for Rc, tc, nc in q["cand"])
    print(f"planar seed {seed}: the true motion among the candidates within {best:.2e}; votes {q['votes']}")
    assert best <= 1e-9
    truth = [c for c, (Rc, tc, nc) in enumerate(q["cand"]) if max(rot_gap(Rc, R), np.abs(tc - t / UNIT_D).max()) <= 1e-9]
    assert len(truth) == 1 and q["votes"][truth[0]] == max(q["votes"]) == len(x)
    # here the vote alone decides: the twin solution puts half of the points behind a camera
    assert sorted(q["votes"])[-2] < 0.9 * len(x) and q["winner"] == truth[0] and not q["flags"] & POSE_AMBIGUOUS
    assert rot_gap(q["R"], R) <= 1e-9 and np.abs(q["t"] - t / np.linalg.norm(t)).max() <= 1e-9
    a = np.column_stack([x, np.ones(len(x))]) @ np.linalg.inv(K_SCENE).T      # depths in units of the baseline
    assert np.abs(q["depth"][:, 0] * np.linalg.norm(t) - PLANE_D / (a @ PLANE_N)).max() <= 1e-8


@pytest.mark.parametrize("seed", range(4))
def test_the_twofold_ambiguity_is_flagged_and_the_hint_resolves_it(seed):
    """A plane seen nearly head-on by a camera that moves towards it: both solutions put every point in front of both cameras."""
    n, d, t = np.array([0.05, -0.03, 1.0]), 6.0, np.array([0.05, 0.02, 0.5])
    R, _ = scene_cameras()
    Hs = K_SCENE @ (R + np.outer(t, n) / d) @ np.linalg.inv(K_SCENE)
    x = np.random.default_rng(seed).uniform([40, 40], [600, 440], (64, 2))
    b = np.column_stack([x, np.ones(64)]) @ Hs.T
    xp, wf, Hu = b[:, :2] / b[:, 2:], np.ones(64, bool), (Hs / np.linalg.norm(Hs)).ravel()
    q = hpose_pair(x, xp, wf, Hu, K_SCENE)
    print("head-on plane: votes", q["votes"], "winner", q["winner"], "flags", q["flags"])
    assert sorted(q["votes"])[-2:] == [64, 64] and q["flags"] == POSE_AMBIGUOUS
    h = hpose_pair(x, xp, wf, Hu, K_SCENE, hint=n)
    nn = np.linalg.norm(n)
    assert h["flags"] == 0 and rot_gap(h["R"], R) <= 1e-9 and np.abs(h["t"] - t / np.linalg.norm(t)).max() <= 1e-9
    assert np.abs(h["normal"] - n / nn).max() <= 1e-9
    # the other contender under the opposite hint: a different motion that explains the same matches
    o = hpose_pair(x, xp, wf, Hu, K_SCENE, hint=h["cand"][[c for c in range(4) if c != h["winner"] and h["votes"][c] == 64][0]][2])
    assert o["winner"] != h["winner"] and rot_gap(o["R"], R) > 1e-3


def test_six_pair_fixture_verdicts_and_counts():
    kp, pairs, m, truth = six_pairs()
    ref, vi = six_reference(), six_verify_info()
    for p, (r, (kind, n_in, n_out)) in enumerate(zip(ref, SIX)):
        kept_true = int((r["mask"] & truth[p]).sum())
        kept_out = int((r["mask"] & ~truth[p]).sum())
        print(f"pair {p} {kind}: flags {r['flags']}, n_H {r['n_inliers']}, n_F {vi[p, 1]} (flags {vi[p, 0]}), ratio {r['ratio']:.3f}, "
              f"true kept {kept_true}/{n_in}, outliers kept {kept_out}/{n_out}, cost gap {r['cost_gap']:.1e}, "
              f"refit gaps {['%.1e' % g for g in r['refit_gaps']]}, tau gap {r['tau_gap']:.3f}, triples {r['triple_factor']:.1f}")
        if kind == "general":
            assert not r["flags"] & DEGENERATE
        else:
            assert (r["flags"] & ~DEGENERATE) == 0
            assert bool(r["flags"] & DEGENERATE) == (kind != "mixed")
            assert (kept_true, kept_out) == SIX_COUNTS[p]
    # without verify_info: no verdict, n_F = -1, everything else the same
    for r, q in zip(ref, six_reference(False)):
        assert q["flags"] == r["flags"] & ~DEGENERATE and q["n_F"] == -1
        assert (q["H"] == r["H"]).all() or np.isnan(r["H"]).all()
        assert (q["mask"] == r["mask"]).all() and q["best_h"] == r["best_h"]


def test_six_pair_poses():
    po, mo, H, hint, R, t, sigma, normal, depth, info, res = six_pose_reference()
    for p, (kind, _, _) in enumerate(SIX):
        r = res[p]
        Rp, tp = pair_motion(p)
        print(f"pair {p} {kind}: pose flags {r['flags']}, winner {r['winner']}, votes {r['votes']}, rot {r['rot']:.2e}")
        if kind == "rotation":
            assert r["flags"] == ROTATION
            assert rot_gap(r["R"], Rp) <= 2e-3      # (0.25 px of noise at f = 500 over 160 matches)
        elif kind == "planar":
            assert not r["flags"] & ROTATION and r["winner"] >= 0
    # with the plane's normal as a hint the planar pairs return the true motion
    res_h = six_pose_reference(True)[-1]
    for p in (1, 3, 5):
        Rp, tp = pair_motion(p)
        r = res_h[p]
        assert not r["flags"] & POSE_AMBIGUOUS
        assert rot_gap(r["R"], Rp) <= (2e-2 if p == 5 else 5e-3) and np.abs(r["t"] - tp / np.linalg.norm(tp)).max() <= (0.2 if p == 5 else 5e-2)


# ------------------------------------------------------------------------------------------------ tests: margins

def check_margins(name, r, kw):
    tol = kw.get("collinear_tol", 1e-3)
    print(f"{name}: flags {r['flags']}, n {r['n_inliers']}, best_h {r['best_h']}, valid {r['n_valid']}, tau gap {r['tau_gap']:.3f}, "
          f"cost gap {r['cost_gap']:.1e}, refit gaps {['%.1e' % g for g in r['refit_gaps']]}, triples {r['triple_factor']:.1f} (tol {tol})")
    assert r["tau_gap"] >= 0.02, name
    assert r["cost_gap"] >= 1e-9, name
    assert all(g >= 1e-9 for g in r["refit_gaps"]), name
    assert r["triple_factor"] >= 10.0, name


def test_margins_of_the_six_pair_fixture():
    for p, r in enumerate(six_reference()):
        check_margins(f"six[{p}]", r, SIX_KW)
        if np.isfinite(r["ratio"]):
            assert abs(r["ratio"] - 0.8) >= 0.05, p
    for hinted in (False, True):
        for p, r in enumerate(six_pose_reference(hinted)[-1]):
            rot, lmin, fmin = pose_margins(r)
            print(f"six[{p}] pose (hint {hinted}): rot factor {rot:.1f}, min |depth| {lmin:.3g}, vote margin {fmin:.3f}")
            assert rot >= 3.0 and lmin >= 1e-3 and fmin >= 0.02, p


@pytest.mark.parametrize("mm", BOUNDARY_M)
def test_margins_of_the_match_count_fixtures(mm):
    r = boundary_reference(mm)
    check_margins(f"m = {mm}", r, boundary_kw(mm))
    assert bool(r["flags"] & TOO_FEW) == (mm < 8)
    if mm >= 8:
        assert r["flags"] == (WEAK if mm < 16 else 0)


@pytest.mark.parametrize("n_hyp", BOUNDARY_HYP)
def test_margins_of_the_hypothesis_count_fixtures(n_hyp):
    r = hyp_reference(n_hyp)
    check_margins(f"n_hyp = {n_hyp}", r, hyp_kw(n_hyp))
    assert r["flags"] == 0


def test_margins_of_the_malformed_and_the_uniform_fixture():
    r = malformed_reference()
    check_margins("malformed", r, SIX_KW)
    assert r["flags"] == MALFORMED and r["n_inliers"] == 61
    r = uniform_reference()
    check_margins("uniform", r, UNIFORM_KW)
    assert r["flags"] == WEAK and r["n_F"] == 0


def test_margins_of_the_infinite_threshold_call():
    for p, r in enumerate(inf_reference()):
        check_margins(f"tau = inf [{p}]", r, INF_KW)
        assert r["flags"] == 0 and r["n_inliers"] == 256 and r["mask"].all()


def test_margins_of_the_default_tolerance_fixture():
    r = grid_reference()
    check_margins("grid", r, GRID_KW)
    assert r["flags"] == 0 and r["n_inliers"] == 20 and 0 < r["n_valid"] < 64      # (samples with a collinear triple are refused)
    assert sign_gap(r["H"], true_H("planar", 0)) <= 1e-6                            # (the pixels went through f32)


# ------------------------------------------------------------------------------------------------ tests: the two routes

def test_second_route_on_the_six_pair_fixture():
    kp, pairs, m, _ = six_pairs()
    for p, r in enumerate(six_reference()):
        if r["n_inliers"] < 16 or not r["refit_gaps"]:
            continue
        rows, wf, x, xp = unpack_pair(kp.astype(np.float64), pairs, m, p)
        # the restatement's last accepted fit ran over the inliers of the model before it; refit once more over the final
        # set by both routes and compare where the two send the inliers
        sel = r["mask"]
        (c, s), (c2, s2) = hartley_block(x, xp, sel)
        terms = plane_terms(s * (x[:, 0] - c[0]), s * (x[:, 1] - c[1]), s2 * (xp[:, 0] - c2[0]), s2 * (xp[:, 1] - c2[1]))
        Ha = solve_h(block_sum(np.where(sel[:, None], terms, 0.0))[None, :], c, s, c2, s2)[0][0]
        Hb = svd_fit(x, xp, sel)
        pa = np.column_stack([x[sel], np.ones(sel.sum())]) @ Ha.reshape(3, 3).T
        pb = np.column_stack([x[sel], np.ones(sel.sum())]) @ Hb.reshape(3, 3).T
        gap = np.abs(pa[:, :2] / pa[:, 2:] - pb[:, :2] / pb[:, 2:]).max()
        print(f"pair {p}: |H_dlt - H_svd| = {sign_gap(Ha, Hb):.2e}, largest difference of a transferred inlier {gap:.2e} px")
        # both minimise the algebraic residual of the same rows, under |h3| = 1 and under |h| = 1: with 0.25 px of noise the
        # minimisers differ by a fraction of what the noise moves either of them; a tenth of the noise is the bound
        assert gap <= 0.025, p


# ------------------------------------------------------------------------------------------------ tests: the chain

PAN_DEG = (0.0, 5.0, 11.0, 11.0, 17.0, 24.0)      # the orbit angle per frame: frames 2 and 3 share their centre
PAN_ANGLE = 0.09                                  # and differ by this rotation about the camera's y axis


@functools.lru_cache(maxsize=None)
def pan_chain_fixture(seed=5, n_pts=120):
    """Six cameras: orbit, orbit, pan, orbit, orbit.  -> dict(kp f64, pairs, m, ext [6, 3, 4] true, in the first camera's frame
    with the first baseline as unit)."""
    rng = np.random.default_rng(seed)
    ext = np.array([synth.look_at_extrinsic((7.0 * math.cos(math.radians(d)), -2.0, 7.0 * math.sin(math.radians(d)))) for d in PAN_DEG])
    Rpan = np.array([[math.cos(PAN_ANGLE), 0, math.sin(PAN_ANGLE)], [0, 1, 0], [-math.sin(PAN_ANGLE), 0, math.cos(PAN_ANGLE)]])
    for f in range(3, 6):      # every camera after the pan is turned with it: the relative motions of the orbit pairs stay
        ext[f] = Rpan @ ext[f]
    X = rng.uniform(-1.2, 1.2, size=(n_pts, 3))
    n = len(PAN_DEG)
    kp = rng.uniform(0, 400, (n, CAP, 2))
    slot = np.array([rng.permutation(CAP)[:n_pts] for _ in range(n)])
    for f in range(n):
        Xc = X @ ext[f, :, :3].T + ext[f, :, 3]
        assert (Xc[:, 2] > 1).all()
        px = Xc @ K_SCENE.T
        kp[f, slot[f]] = px[:, :2] / px[:, 2:]
    pairs = np.full((n - 1, CAP, 2), -1, np.int32)
    for p in range(n - 1):
        order = rng.permutation(n_pts)
        pairs[p, :n_pts] = np.c_[slot[p][order], slot[p + 1][order]]
    R0, t0 = ext[0, :, :3], ext[0, :, 3]
    unit = np.linalg.norm(ext[1, :, 3] - ext[1, :, :3] @ R0.T @ t0)
    rel = np.array([np.c_[e[:, :3] @ R0.T, (e[:, 3] - e[:, :3] @ R0.T @ t0) / unit] for e in ext])
    return dict(kp=kp, pairs=pairs, m=np.full(n - 1, n_pts, np.int32), ext=rel)


def test_a_pan_inside_an_orbit_is_repaired_and_the_scale_carried():
    fx = pan_chain_fixture()
    kp, pairs, m, ext = fx["kp"], fx["pairs"], fx["m"], fx["ext"]
    n = len(m)
    R, t, depth, info = np.zeros((n, 9)), np.zeros((n, 3)), np.full((n, CAP, 2), np.nan), np.zeros((n, 8), np.int32)
    for p in range(n):
        rows, wf, x, xp = unpack_pair(kp, pairs, m, p)
        Rr = ext[p + 1, :, :3] @ ext[p, :, :3].T
        tr = ext[p + 1, :, 3] - Rr @ ext[p, :, 3]
        if p == 2:      # the pan: F is not determined; the homography is K R K^-1 and the verdict sends the pair here
            assert np.abs(tr).max() <= 1e-12
            Hh = K_SCENE @ Rr @ np.linalg.inv(K_SCENE)
            fit = homography_pair(x, xp, wf, p, n_hyp=32, collinear_tol=1e-6)
            assert fit["flags"] == 0 and fit["n_inliers"] == len(x) and sign_gap(fit["H"], (Hh / np.linalg.norm(Hh)).ravel()) <= 1e-9
            r = hpose_pair(x, xp, wf, fit["H"], K_SCENE)
            assert r["flags"] == ROTATION and rot_gap(r["R"], Rr) <= 1e-9
            info[p] = [r["flags"], r["winner"]] + r["votes"] + [len(x), 0]
        else:
            r = recover_pair(x, xp, wf, fundamental(Rr, tr), K_SCENE)
            assert r["flags"] == 0
            info[p] = [r["flags"], r["winner"]] + r["votes"] + [len(x), 0]
        R[p], t[p], depth[p, :len(x)] = r["R"], r["t"], r["depth"]
    got, scale, rho, cinfo = chain_numpy(pairs, m, depth, R, t, info)
    print("scale", scale, "chain flags", cinfo[:, 0], "common", cinfo[:, 1])
    assert list(cinfo[:, 0]) == [0, 0, CHAIN_FEW_COMMON, CHAIN_FEW_COMMON, 0]
    assert scale[2] == scale[1] and scale[3] == scale[1]      # carried across the pan and into the pair after it
    assert np.abs(got[:4, :, :3] - ext[:4, :, :3]).max() <= 1e-9 and np.abs(got[:4, :, 3] - ext[:4, :, 3]).max() <= 1e-8
    centre = lambda E: -E[:, :3].T @ E[:, 3]      # noqa: E731
    assert np.abs(centre(got[3]) - centre(got[2])).max() <= 1e-12      # the pan moved nothing
    # after the pan the rotations are right; the translations carry the scale of the pair before it, not the true one
    assert np.abs(got[4:, :, :3] - ext[4:, :, :3]).max() <= 1e-9
    step = lambda E, f: np.linalg.norm(centre(E[f + 1]) - centre(E[f]))      # noqa: E731
    assert abs(step(got, 4) / step(got, 3) - step(ext, 4) / step(ext, 3)) <= 1e-8      # (pair 4 is scaled against pair 3 again)


# ------------------------------------------------------------------------------------------------ tests: the library

def test_library_table_has_the_homography_symbols():
    from meatmodeler_amd import _lib
    for name in ("mm_homography_workspace_bytes", "mm_verify_homography", "mm_recover_poses_homography"):
        assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES
    assert C.sizeof(_lib.HomographyParams) == 6 * 4 + 3 * 8 and C.sizeof(_lib.HPoseParams) == 2 * 4 + 3 * 8
    assert _lib.lib.mm_abi_version() == 3


def test_workspace_is_monotone_and_aligned():
    from meatmodeler_amd import _lib
    f = _lib.lib.mm_homography_workspace_bytes
    assert f(0, 256) == 0 and f(-3, 256) == 0
    prev = 0
    for n_pairs in (1, 2, 7, 199):
        for n_hyp in (1, 64, 65, 256, 4096):
            b = f(n_pairs, n_hyp)
            assert b % 256 == 0 and b >= n_pairs * (8 + 10 * n_hyp) * 8
            assert f(n_pairs + 1, n_hyp) >= b and f(n_pairs, n_hyp + 1) >= b
        assert f(n_pairs, 256) > prev
        prev = f(n_pairs, 256)


def test_argument_errors_return_before_any_device_call():
    """Every bad call is refused with ctx = NULL: nothing below the argument block can have run."""
    from meatmodeler_amd import _lib
    lib = _lib.lib
    buf = (C.c_double * 4096)()
    p = C.addressof(buf)
    out = C.addressof(buf) + 16384

    def verify(prm, n_pairs=1, cap=8, ws_bytes=1 << 20, **null):
        a = dict(kp_xy=p, pairs=p, m=p, vi=None, pairs_out=out, m_out=p, H=p, cost=p, info=p, ws=p)
        a.update(null)
        return lib.mm_verify_homography(None, a["kp_xy"], a["pairs"], a["m"], n_pairs, cap, prm, a["vi"], a["pairs_out"], a["m_out"],
                                        a["H"], a["cost"], a["info"], a["ws"], ws_bytes)

    def hp(**kw):
        v = dict(n_hyp=256, min_matches=8, min_inliers=16, refit_iters=2, seed=0, pair_base=0, threshold_px=2.0, collinear_tol=1e-3,
                 degenerate_frac=0.8)
        v.update(kw)
        return C.byref(_lib.HomographyParams(*[v[k] for k, _ in _lib.HomographyParams._fields_]))

    ERR_ARG, ERR_WS = -1, -3
    assert verify(None) == ERR_ARG
    assert verify(hp(), n_pairs=-1) == ERR_ARG
    for bad in (dict(n_hyp=0), dict(n_hyp=4097), dict(threshold_px=-1.0), dict(threshold_px=math.nan), dict(collinear_tol=-1e-3),
                dict(collinear_tol=math.nan), dict(degenerate_frac=-0.1), dict(degenerate_frac=1.5), dict(degenerate_frac=math.nan),
                dict(refit_iters=-1), dict(min_inliers=-1)):
        assert verify(hp(**bad)) == ERR_ARG, bad
    for name in ("kp_xy", "pairs", "m", "pairs_out", "m_out", "H", "cost", "info", "ws"):
        assert verify(hp(), **{name: None}) == ERR_ARG, name
    assert verify(hp(), pairs_out=p) == ERR_ARG               # (aliases pairs)
    assert verify(hp(), cap=0) == ERR_ARG
    assert verify(hp(), ws_bytes=lib.mm_homography_workspace_bytes(1, 256) - 1) == ERR_WS
    # a good call gets as far as the context (NULL here): the same code, but only after every check above passed
    assert verify(hp()) == ERR_ARG and verify(hp(), n_pairs=0) == ERR_ARG

    K = (C.c_double * 9)(500, 0, 320, 0, 500, 240, 0, 0, 1)

    def pose(prm, K=K, n_pairs=1, cap=8, **null):
        a = dict(kp_xy=p, pairs=p, m=p, H=p, hint=None, R=p, t=p, sigma=p, normal=p, depth=p, info=p)
        a.update(null)
        return lib.mm_recover_poses_homography(None, K, a["kp_xy"], a["pairs"], a["m"], a["H"], a["hint"], n_pairs, cap, prm, a["R"],
                                               a["t"], a["sigma"], a["normal"], a["depth"], a["info"])

    def pp(min_matches=8, min_front_frac=0.5, ambiguous_frac=0.9, rotation_tol=1e-2):
        return C.byref(_lib.HPoseParams(min_matches, 0, min_front_frac, ambiguous_frac, rotation_tol))

    assert pose(None) == ERR_ARG and pose(pp(), K=None) == ERR_ARG and pose(pp(), n_pairs=-1) == ERR_ARG and pose(pp(), cap=0) == ERR_ARG
    for bad in (dict(min_front_frac=-0.1), dict(min_front_frac=1.1), dict(ambiguous_frac=math.nan), dict(ambiguous_frac=2.0),
                dict(rotation_tol=-1e-2), dict(rotation_tol=math.nan)):
        assert pose(pp(**bad)) == ERR_ARG, bad
    for k, v in ((3, 1.0), (8, 2.0), (0, 0.0), (4, math.inf)):
        Kb = (C.c_double * 9)(*K)
        Kb[k] = v
        assert pose(pp(), K=Kb) == ERR_ARG, k
    for name in ("kp_xy", "pairs", "m", "H", "R", "t", "sigma", "normal", "depth", "info"):
        assert pose(pp(), **{name: None}) == ERR_ARG, name
    assert pose(pp()) == ERR_ARG


def test_degeneracy_option_validation():
    from meatmodeler_amd import pipeline
    assert pipeline.degeneracy_options(None) is None and pipeline.degeneracy_options({}) == {}
    assert pipeline.degeneracy_options(dict(degenerate_frac=0.7, rotation_tol=0.02)) == dict(degenerate_frac=0.7, rotation_tol=0.02)
    with pytest.raises(ValueError, match="degeneracy"):
        pipeline.degeneracy_options(dict(on_fail="drop"))
    with pytest.raises(ValueError, match="degeneracy"):
        pipeline.degeneracy_options(True)
    # run() judges its options before it touches its frames or the device
    with pytest.raises(ValueError, match="degeneracy needs verify"):
        pipeline.ClipPipeline.run(None, None, None, extrinsics=np.zeros((2, 3, 4)), degeneracy={})
    with pytest.raises(ValueError, match="degeneracy takes"):
        pipeline.ClipPipeline.run(None, None, None, extrinsics=np.zeros((2, 3, 4)), verify={}, degeneracy=dict(threshold=2.0))
