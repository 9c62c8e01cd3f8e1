"""Thin tensor-level wrappers over the C ABI (include/meatmodeler.h).

torch is used for device memory and streams only; every computation below is a HIP kernel launched through
`libmeatmodeler_hip.so`.  All functions take/return torch tensors on the context's device.
"""
import ctypes as C
import math
import os

import numpy as np
import torch

from . import _lib
from ._lib import lib, ptr, vp, OrbParams, BAProblem, default_context

ptr_ = ptr      # (align_similarity has an argument of that name)


def _i32(t):
    assert t.dtype == torch.int32 and t.is_contiguous()
    return t


# ------------------------------------------------------------------------------------------------ matching

def bf_knn2_batched(q, t, nq=None, nt=None, ctx=None):
    """q [n_pairs, nq_cap, 32] u8, t [n_pairs, nt_cap, 32] u8 (may be strided views over a descriptor table
    as long as rows are contiguous); nq / nt optional int32 [n_pairs] valid counts.
    Returns idx, dist int32 [n_pairs, nq_cap, 2]."""
    ctx = ctx or default_context()
    assert q.dtype == torch.uint8 and t.dtype == torch.uint8 and q.shape[-1] == 32 and t.shape[-1] == 32
    assert q.stride(-1) == 1 and q.stride(-2) == 32 and t.stride(-1) == 1 and t.stride(-2) == 32
    n_pairs, nq_cap, nt_cap = q.shape[0], q.shape[1], t.shape[1]
    assert t.shape[0] == n_pairs
    both = torch.full((2, n_pairs, nq_cap, 2), -1, dtype=torch.int32, device=q.device)      # (one fill, two views)
    idx, dist = both[0], both[1]
    if n_pairs == 0 or nq_cap == 0:
        return idx, dist
    wsb = lib.mm_bf_workspace_bytes(n_pairs, nq_cap, nt_cap)
    ws = torch.empty(wsb, dtype=torch.uint8, device=q.device)
    qs = q.stride(0) if n_pairs > 1 else 0
    ts = t.stride(0) if n_pairs > 1 else 0
    ctx.check(lib.mm_bf_knn2_batched(ctx.h, ptr(q), ptr(nq), nq_cap, qs, ptr(t), ptr(nt), nt_cap, ts, n_pairs,
                                     ptr(idx), ptr(dist), ptr(ws), wsb), "mm_bf_knn2_batched")
    return idx, dist


def bf_knn2(q, t, ctx=None):
    """Single pair: q [nq,32], t [nt,32] -> idx, dist int32 [nq,2] (mm_bf_knn2_hamming)."""
    ctx = ctx or default_context()
    assert q.dtype == torch.uint8 and t.dtype == torch.uint8 and q.is_contiguous() and t.is_contiguous()
    nq, nt = q.shape[0], t.shape[0]
    idx = torch.full((nq, 2), -1, dtype=torch.int32, device=q.device)
    dist = torch.full((nq, 2), -1, dtype=torch.int32, device=q.device)
    if nq == 0:
        return idx, dist
    wsb = lib.mm_bf_workspace_bytes(1, nq, nt)
    ws = torch.empty(wsb, dtype=torch.uint8, device=q.device)
    ctx.check(lib.mm_bf_knn2_hamming(ctx.h, ptr(q), nq, ptr(t), nt, ptr(idx), ptr(dist), ptr(ws), wsb),
              "mm_bf_knn2_hamming")
    return idx, dist


def ratio_filter_batched(idx, dist, threshold=0.75, nq=None, ctx=None):
    """idx/dist [n_pairs, nq_cap, 2] -> pairs int32 [n_pairs, nq_cap, 2] (queryIdx, trainIdx), m int32 [n_pairs]."""
    ctx = ctx or default_context()
    n_pairs, nq_cap = idx.shape[0], idx.shape[1]
    pairs = torch.full((n_pairs, nq_cap, 2), -1, dtype=torch.int32, device=idx.device)
    m = torch.zeros(n_pairs, dtype=torch.int32, device=idx.device)
    if n_pairs == 0:
        return pairs, m
    ctx.check(lib.mm_ratio_filter_batched(ctx.h, ptr(_i32(idx)), ptr(_i32(dist)), ptr(nq), nq_cap, n_pairs,
                                          float(threshold), ptr(pairs), ptr(m)), "mm_ratio_filter_batched")
    return pairs, m


def bf_match_ratio_batched(q, t, nq=None, nt=None, threshold=0.75, ctx=None):
    """The match stage in one call (mm_bf_match_ratio_batched): what bf_knn2_batched + ratio_filter_batched return for the
    same arguments -- pairs int32 [n_pairs, nq_cap, 2] (queryIdx, trainIdx; -1 beyond m), m int32 [n_pairs] -- with every
    element written by the kernels (no fills) and without idx / dist in memory."""
    ctx = ctx or default_context()
    assert q.dtype == torch.uint8 and t.dtype == torch.uint8 and q.shape[-1] == 32 and t.shape[-1] == 32
    assert q.stride(-1) == 1 and q.stride(-2) == 32 and t.stride(-1) == 1 and t.stride(-2) == 32
    n_pairs, nq_cap, nt_cap = q.shape[0], q.shape[1], t.shape[1]
    assert t.shape[0] == n_pairs
    pairs = torch.empty((n_pairs, nq_cap, 2), dtype=torch.int32, device=q.device)
    m = torch.empty(n_pairs, dtype=torch.int32, device=q.device)
    if n_pairs == 0:
        return pairs, m
    wsb = lib.mm_bf_match_ratio_workspace_bytes(n_pairs, nq_cap, nt_cap)
    ws = torch.empty(wsb, dtype=torch.uint8, device=q.device)
    qs = q.stride(0) if n_pairs > 1 else 0
    ts = t.stride(0) if n_pairs > 1 else 0
    ctx.check(lib.mm_bf_match_ratio_batched(ctx.h, ptr(q), ptr(nq), nq_cap, qs, ptr(t), ptr(nt), nt_cap, ts, n_pairs,
                                            float(threshold), ptr(pairs), ptr(m), ptr(ws), wsb),
              "mm_bf_match_ratio_batched")
    return pairs, m


VERIFY_TOO_FEW, VERIFY_NO_MODEL, VERIFY_WEAK, VERIFY_MALFORMED = 1, 2, 4, 8      # MM_VERIFY_* of include/meatmodeler.h


def verify_matches(kp_xy, pairs, m, n_hyp=256, threshold_px=2.0, min_matches=16, min_inliers=16, refit_iters=2, seed=0,
                   pair_base=0, on_fail="keep", ctx=None):
    """Epipolar verification of consecutive frame pairs (mm_verify_matches): kp_xy [n_pairs+1, cap, 2] f32, pairs
    [n_pairs, cap, 2] i32, m [n_pairs] i32 (device tensors; what ratio_filter_batched returns)
    -> (pairs_out [n_pairs, cap, 2] i32 -- the inliers of each pair's fundamental matrix in input order, -1 beyond m_out --,
    m_out [n_pairs] i32, F [n_pairs, 9] f64 (x'^T F x = 0, unit norm, NaN without a model), cost [n_pairs] f64,
    info [n_pairs, 4] i32 = (VERIFY_* flags, n_inliers, best_h, valid hypotheses)).
    on_fail: "keep" passes the matches of a failed pair (too few, no model, weak) through, "drop" removes them."""
    if on_fail not in ("keep", "drop"):
        raise ValueError("verify_matches: on_fail must be 'keep' or 'drop'")
    if not 1 <= int(n_hyp) <= 4096:
        raise ValueError("verify_matches: n_hyp must be in 1 .. 4096")
    if not float(threshold_px) >= 0:
        raise ValueError("verify_matches: threshold_px must not be negative")
    if not 0 <= int(refit_iters) <= 1000 or int(min_inliers) < 0:
        raise ValueError("verify_matches: refit_iters must be in 0 .. 1000 and min_inliers not negative")
    if pairs.dim() != 3 or pairs.shape[2] != 2 or kp_xy.dim() != 3 or tuple(kp_xy.shape) != (pairs.shape[0] + 1, pairs.shape[1], 2) \
            or tuple(m.shape) != (pairs.shape[0],):
        raise ValueError("verify_matches: kp_xy [n_pairs+1, cap, 2], pairs [n_pairs, cap, 2] and m [n_pairs] expected")
    ctx = ctx or default_context()
    d = pairs.device
    n_pairs, cap = pairs.shape[0], pairs.shape[1]
    pairs_out = torch.full((n_pairs, cap, 2), -1, dtype=torch.int32, device=d)
    m_out = torch.zeros(n_pairs, dtype=torch.int32, device=d)
    F = torch.full((n_pairs, 9), math.nan, dtype=torch.float64, device=d)
    cost = torch.full((n_pairs,), math.nan, dtype=torch.float64, device=d)
    info = torch.zeros((n_pairs, 4), dtype=torch.int32, device=d)
    if n_pairs == 0 or cap == 0:
        return pairs_out, m_out, F, cost, info
    prm = _lib.VerifyParams(int(n_hyp), int(min_matches), int(min_inliers), int(refit_iters), int(seed) & 0xFFFFFFFF,
                            int(pair_base) & 0xFFFFFFFF, 1 if on_fail == "drop" else 0, 0, float(threshold_px))
    wsb = lib.mm_verify_workspace_bytes(n_pairs, int(n_hyp))
    ws = torch.empty(wsb, dtype=torch.uint8, device=d)
    assert kp_xy.dtype == torch.float32
    ctx.check(lib.mm_verify_matches(ctx.h, ptr(kp_xy.contiguous()), ptr(_i32(pairs.contiguous())), ptr(_i32(m.contiguous())),
                                    n_pairs, cap, C.byref(prm), ptr(pairs_out), ptr(m_out), ptr(F), ptr(cost), ptr(info),
                                    ptr(ws), wsb), "mm_verify_matches")
    return pairs_out, m_out, F, cost, info


POSE_TOO_FEW, POSE_NO_MODEL, POSE_AMBIGUOUS, POSE_MALFORMED = 1, 2, 4, 8      # MM_POSE_* of include/meatmodeler.h
CHAIN_FEW_COMMON, CHAIN_BROKEN = 1, 2                                         # MM_CHAIN_*
CHAIN_MAX_CAP = 8192


def _host_f64(a, n, what):
    a = np.ascontiguousarray(np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, dtype=np.float64)).reshape(-1)
    if a.size != n:
        raise ValueError(f"{what}: {n} numbers expected")
    return a


def recover_poses(kp_xy, pairs, m, F, K, min_matches=8, min_front_frac=0.5, ambiguous_frac=0.5, ctx=None):
    """Relative pose of every consecutive frame pair (mm_recover_poses): kp_xy [n_pairs+1, cap, 2] f32, pairs [n_pairs, cap, 2]
    i32, m [n_pairs] i32 and F [n_pairs, 9] f64 as verify_matches returns them (device tensors), K 3 x 3 on the host
    -> (R [n_pairs, 9] f64, t [n_pairs, 3] f64 with X2 = R X1 + t and |t| = 1, NaN without a model; sigma [n_pairs, 2] f64;
    depth [n_pairs, cap, 2] f64 -- the winner's depths of the rows that voted for it, NaN elsewhere;
    info [n_pairs, 8] i32 = (POSE_* flags, winner or -1, votes[0..3], m used, 0))."""
    Kh = _host_f64(K, 9, "recover_poses: K")
    if not np.isfinite(Kh).all() or Kh[3] != 0 or Kh[6] != 0 or Kh[7] != 0 or Kh[8] != 1 or Kh[0] == 0 or Kh[4] == 0:
        raise ValueError("recover_poses: K must be finite, upper triangular with K[2, 2] = 1 and non-zero focal lengths")
    if not (0.0 <= float(min_front_frac) <= 1.0 and 0.0 <= float(ambiguous_frac) <= 1.0):
        raise ValueError("recover_poses: min_front_frac and ambiguous_frac must be in [0, 1]")
    if pairs.dim() != 3 or pairs.shape[2] != 2 or kp_xy.dim() != 3 or tuple(kp_xy.shape) != (pairs.shape[0] + 1, pairs.shape[1], 2) \
            or tuple(m.shape) != (pairs.shape[0],) or tuple(F.shape) != (pairs.shape[0], 9):
        raise ValueError("recover_poses: kp_xy [n_pairs+1, cap, 2], pairs [n_pairs, cap, 2], m [n_pairs] and F [n_pairs, 9] expected")
    ctx = ctx or default_context()
    d = pairs.device
    n_pairs, cap = pairs.shape[0], pairs.shape[1]
    R = torch.full((n_pairs, 9), math.nan, dtype=torch.float64, device=d)
    t = torch.full((n_pairs, 3), math.nan, dtype=torch.float64, device=d)
    sigma = torch.full((n_pairs, 2), math.nan, dtype=torch.float64, device=d)
    depth = torch.empty((n_pairs, cap, 2), dtype=torch.float64, device=d)      # (every element is written by the kernel)
    info = torch.zeros((n_pairs, 8), dtype=torch.int32, device=d)
    if n_pairs == 0 or cap == 0:
        return R, t, sigma, depth, info
    assert kp_xy.dtype == torch.float32 and F.dtype == torch.float64
    prm = _lib.PoseParams(int(min_matches), 0, float(min_front_frac), float(ambiguous_frac))
    ctx.check(lib.mm_recover_poses(ctx.h, Kh.ctypes.data_as(_lib.c_f64p), ptr(kp_xy.contiguous()), ptr(_i32(pairs.contiguous())),
                                   ptr(_i32(m.contiguous())), ptr(F.contiguous()), n_pairs, cap, C.byref(prm), ptr(R), ptr(t),
                                   ptr(sigma), ptr(depth), ptr(info)), "mm_recover_poses")
    return R, t, sigma, depth, info


def chain_poses(pairs, m, depth, R, t, info, E0=None, min_common=8, ctx=None):
    """The pairs of recover_poses in one scale and one coordinate frame (mm_chain_poses); every argument is an input (device
    tensors), E0 the first frame's extrinsic [3, 4] on the host ([I | 0] by default)
    -> (extrinsics [n_pairs+1, 3, 4] f64, scale [n_pairs] f64, rho [n_pairs] f64, chain_info [n_pairs, 2] i32 =
    (CHAIN_* flags, n_common))."""
    E0h = _host_f64(np.eye(3, 4) if E0 is None else np.asarray(E0, float)[:3, :], 12, "chain_poses: E0")
    if int(min_common) < 0:
        raise ValueError("chain_poses: min_common must not be negative")
    n_pairs = pairs.shape[0]
    if pairs.dim() != 3 or pairs.shape[2] != 2 or tuple(m.shape) != (n_pairs,) or tuple(depth.shape) != tuple(pairs.shape) \
            or tuple(R.shape) != (n_pairs, 9) or tuple(t.shape) != (n_pairs, 3) or tuple(info.shape) != (n_pairs, 8):
        raise ValueError("chain_poses: pairs / depth [n_pairs, cap, 2], m [n_pairs], R [n_pairs, 9], t [n_pairs, 3], info [n_pairs, 8] expected")
    cap = pairs.shape[1]
    if cap > CHAIN_MAX_CAP:
        raise ValueError(f"chain_poses: cap must not exceed {CHAIN_MAX_CAP}")
    ctx = ctx or default_context()
    d = pairs.device
    ext = torch.empty((n_pairs + 1, 3, 4), dtype=torch.float64, device=d)
    scale = torch.ones(n_pairs, dtype=torch.float64, device=d)
    rho = torch.ones(n_pairs, dtype=torch.float64, device=d)
    cinfo = torch.zeros((n_pairs, 2), dtype=torch.int32, device=d)
    if n_pairs == 0 or cap == 0:
        ext[:] = torch.as_tensor(E0h.reshape(3, 4)).to(d)
        return ext, scale, rho, cinfo
    assert depth.dtype == torch.float64 and R.dtype == torch.float64 and t.dtype == torch.float64
    ctx.check(lib.mm_chain_poses(ctx.h, ptr(_i32(pairs.contiguous())), ptr(_i32(m.contiguous())), ptr(depth.contiguous()),
                                 ptr(R.contiguous()), ptr(t.contiguous()), ptr(_i32(info.contiguous())), n_pairs, cap,
                                 E0h.ctypes.data_as(_lib.c_f64p), int(min_common), ptr(ext), ptr(scale), ptr(rho), ptr(cinfo)),
              "mm_chain_poses")
    return ext, scale, rho, cinfo


HOMOG_TOO_FEW, HOMOG_NO_MODEL, HOMOG_WEAK, HOMOG_MALFORMED, HOMOG_DEGENERATE = 1, 2, 4, 8, 16      # MM_HOMOG_*
HPOSE_ROTATION = 16                                                                             # MM_HPOSE_ROTATION


def _pair_shapes(name, kp_xy, pairs, m):
    if pairs.dim() != 3 or pairs.shape[2] != 2 or kp_xy.dim() != 3 or tuple(kp_xy.shape) != (pairs.shape[0] + 1, pairs.shape[1], 2) \
            or tuple(m.shape) != (pairs.shape[0],):
        raise ValueError(f"{name}: kp_xy [n_pairs+1, cap, 2], pairs [n_pairs, cap, 2] and m [n_pairs] expected")


def verify_homography(kp_xy, pairs, m, verify_info=None, n_hyp=256, threshold_px=2.0, min_matches=8, min_inliers=16, refit_iters=2,
                      seed=0, pair_base=0, collinear_tol=1e-3, degenerate_frac=0.8, ctx=None):
    """A RANSAC homography per consecutive frame pair (mm_verify_homography) on the matches verify_matches reads: kp_xy
    [n_pairs+1, cap, 2] f32, pairs [n_pairs, cap, 2] i32, m [n_pairs] i32 (device tensors); verify_info [n_pairs, 4] i32 the
    info of verify_matches on the same matches, or None (no verdict)
    -> (pairs_out [n_pairs, cap, 2] i32 -- the inliers of each pair's homography in input order, -1 beyond m_out; nothing for
    a failed pair --, m_out [n_pairs] i32, H [n_pairs, 9] f64 (x' ~ H x, unit norm, NaN without a model), cost [n_pairs] f64,
    info [n_pairs, 6] i32 = (HOMOG_* flags, n_inliers, best_h, valid hypotheses, n_F or -1, 0)).  HOMOG_DEGENERATE: the pair
    is planar or rotation-only, its fundamental matrix one of a pencil."""
    if not 1 <= int(n_hyp) <= 4096:
        raise ValueError("verify_homography: n_hyp must be in 1 .. 4096")
    if not float(threshold_px) >= 0 or not float(collinear_tol) >= 0:
        raise ValueError("verify_homography: threshold_px and collinear_tol must not be negative")
    if not 0.0 <= float(degenerate_frac) <= 1.0:
        raise ValueError("verify_homography: degenerate_frac must be in [0, 1]")
    if not 0 <= int(refit_iters) <= 1000 or int(min_inliers) < 0:
        raise ValueError("verify_homography: refit_iters must be in 0 .. 1000 and min_inliers not negative")
    _pair_shapes("verify_homography", kp_xy, pairs, m)
    if verify_info is not None and tuple(verify_info.shape) != (pairs.shape[0], 4):
        raise ValueError("verify_homography: verify_info [n_pairs, 4] expected")
    ctx = ctx or default_context()
    d = pairs.device
    n_pairs, cap = pairs.shape[0], pairs.shape[1]
    pairs_out = torch.full((n_pairs, cap, 2), -1, dtype=torch.int32, device=d)
    m_out = torch.zeros(n_pairs, dtype=torch.int32, device=d)
    H = torch.full((n_pairs, 9), math.nan, dtype=torch.float64, device=d)
    cost = torch.full((n_pairs,), math.nan, dtype=torch.float64, device=d)
    info = torch.zeros((n_pairs, 6), dtype=torch.int32, device=d)
    if n_pairs == 0 or cap == 0:
        return pairs_out, m_out, H, cost, info
    prm = _lib.HomographyParams(int(n_hyp), int(min_matches), int(min_inliers), int(refit_iters), int(seed) & 0xFFFFFFFF,
                                int(pair_base) & 0xFFFFFFFF, float(threshold_px), float(collinear_tol), float(degenerate_frac))
    wsb = lib.mm_homography_workspace_bytes(n_pairs, int(n_hyp))
    ws = torch.empty(wsb, dtype=torch.uint8, device=d)
    assert kp_xy.dtype == torch.float32
    vi = None if verify_info is None else _i32(verify_info.contiguous())
    ctx.check(lib.mm_verify_homography(ctx.h, ptr(kp_xy.contiguous()), ptr(_i32(pairs.contiguous())), ptr(_i32(m.contiguous())),
                                       n_pairs, cap, C.byref(prm), ptr(vi), ptr(pairs_out), ptr(m_out), ptr(H), ptr(cost),
                                       ptr(info), ptr(ws), wsb), "mm_verify_homography")
    return pairs_out, m_out, H, cost, info


GUIDED_SKIPPED, GUIDED_UNORDERED, GUIDED_MALFORMED = 1, 2, 8      # MM_GUIDED_*


def guided_match(kp_xy, desc, n, pairs, m, model, kind=None, threshold_px=2.0, ratio=0.8, max_dist=64, cross_check=True, ctx=None):
    """Guided matching of consecutive frame pairs (mm_guided_match): the key points no seed match uses are matched again among
    the candidates each pair's model admits.  kp_xy [n_pairs+1, cap, 2] f32, desc [n_pairs+1, cap, 32] u8, n [n_pairs+1] i32 key
    points per frame; pairs [n_pairs, cap, 2] i32 and m [n_pairs] i32 the seeds, in strictly increasing query order (what
    verify_matches / verify_homography return); model [n_pairs, 9] f64 and kind [n_pairs] i32 (0: model is F with
    x'^T F x = 0, 1: H with x' ~ H x, anything else: no model; None: all 0) -- device tensors
    -> (pairs_out [n_pairs, cap, 2] i32 -- seeds and new rows merged in query order, -1 beyond m_out --, m_out [n_pairs] i32,
    is_new [n_pairs, cap] u8 parallel to pairs_out, info [n_pairs, 4] i32 = (GUIDED_* flags, input rows kept, rows added,
    proposals before the one-to-one step)).  A new row is within threshold_px of the model (the inlier rule of the verify
    stages), at most max_dist bits from its query, the only candidate or under `ratio` times the second, and one-to-one:
    cross_check=True keeps it when the query is also the train's nearest candidate, False the lowest distance per train."""
    if not float(threshold_px) >= 0:
        raise ValueError("guided_match: threshold_px must not be negative")
    if not float(ratio) >= 0:
        raise ValueError("guided_match: ratio must not be negative")
    if not 0 <= int(max_dist) <= 256:
        raise ValueError("guided_match: max_dist must be in 0 .. 256")
    _pair_shapes("guided_match", kp_xy, pairs, m)
    n_pairs, cap = pairs.shape[0], pairs.shape[1]
    if tuple(desc.shape) != (n_pairs + 1, cap, 32) or tuple(n.shape) != (n_pairs + 1,) or tuple(model.shape) != (n_pairs, 9) \
            or (kind is not None and tuple(kind.shape) != (n_pairs,)):
        raise ValueError("guided_match: desc [n_pairs+1, cap, 32], n [n_pairs+1], model [n_pairs, 9] and kind [n_pairs] expected")
    ctx = ctx or default_context()
    d = pairs.device
    pairs_out = torch.empty((n_pairs, cap, 2), dtype=torch.int32, device=d)      # (every element is written by the kernels)
    m_out = torch.zeros(n_pairs, dtype=torch.int32, device=d)
    is_new = torch.zeros((n_pairs, cap), dtype=torch.uint8, device=d)
    info = torch.zeros((n_pairs, 4), dtype=torch.int32, device=d)
    if n_pairs == 0 or cap == 0:
        return pairs_out, m_out, is_new, info
    assert kp_xy.dtype == torch.float32 and desc.dtype == torch.uint8 and model.dtype == torch.float64
    prm = _lib.GuidedParams(float(threshold_px), float(ratio), int(max_dist), 1 if cross_check else 0)
    wsb = lib.mm_guided_workspace_bytes(n_pairs, cap)
    ws = torch.empty(wsb, dtype=torch.uint8, device=d)
    kd = None if kind is None else _i32(kind.contiguous())
    ctx.check(lib.mm_guided_match(ctx.h, ptr(kp_xy.contiguous()), ptr(desc.contiguous()), ptr(_i32(n.contiguous())),
                                  ptr(_i32(pairs.contiguous())), ptr(_i32(m.contiguous())), ptr(model.contiguous()), ptr(kd),
                                  n_pairs, cap, C.byref(prm), ptr(pairs_out), ptr(m_out), ptr(is_new), ptr(info), ptr(ws), wsb),
              "mm_guided_match")
    return pairs_out, m_out, is_new, info


def recover_poses_homography(kp_xy, pairs, m, H, K, normal_hint=None, min_matches=8, min_front_frac=0.5, ambiguous_frac=0.9,
                             rotation_tol=1e-2, ctx=None):
    """The motion each pair's homography implies (mm_recover_poses_homography): kp_xy, pairs, m and H [n_pairs, 9] f64 as
    verify_homography returns them (device tensors), K 3 x 3 on the host, normal_hint [n_pairs, 3] f64 or None
    -> (R [n_pairs, 9], t [n_pairs, 3] with X2 = R X1 + t -- |t| = 1 for a plane, t = 0 with HPOSE_ROTATION --, sigma
    [n_pairs, 3], normal [n_pairs, 3] (the plane n . X = d in camera 1; NaN for a rotation), depth [n_pairs, cap, 2], info
    [n_pairs, 8] i32 = (POSE_* flags | HPOSE_ROTATION, winner or -1, votes[0..3], m used, 0)): the rows chain_poses reads."""
    Kh = _host_f64(K, 9, "recover_poses_homography: K")
    if not np.isfinite(Kh).all() or Kh[3] != 0 or Kh[6] != 0 or Kh[7] != 0 or Kh[8] != 1 or Kh[0] == 0 or Kh[4] == 0:
        raise ValueError("recover_poses_homography: K must be finite, upper triangular with K[2, 2] = 1 and non-zero focal lengths")
    if not (0.0 <= float(min_front_frac) <= 1.0 and 0.0 <= float(ambiguous_frac) <= 1.0):
        raise ValueError("recover_poses_homography: min_front_frac and ambiguous_frac must be in [0, 1]")
    if not float(rotation_tol) >= 0:
        raise ValueError("recover_poses_homography: rotation_tol must not be negative")
    _pair_shapes("recover_poses_homography", kp_xy, pairs, m)
    if tuple(H.shape) != (pairs.shape[0], 9) or (normal_hint is not None and tuple(normal_hint.shape) != (pairs.shape[0], 3)):
        raise ValueError("recover_poses_homography: H [n_pairs, 9] and normal_hint [n_pairs, 3] expected")
    ctx = ctx or default_context()
    d = pairs.device
    n_pairs, cap = pairs.shape[0], pairs.shape[1]
    R = torch.full((n_pairs, 9), math.nan, dtype=torch.float64, device=d)
    t = torch.full((n_pairs, 3), math.nan, dtype=torch.float64, device=d)
    sigma = torch.full((n_pairs, 3), math.nan, dtype=torch.float64, device=d)
    normal = torch.full((n_pairs, 3), math.nan, dtype=torch.float64, device=d)
    depth = torch.empty((n_pairs, cap, 2), dtype=torch.float64, device=d)      # (every element is written by the kernel)
    info = torch.zeros((n_pairs, 8), dtype=torch.int32, device=d)
    if n_pairs == 0 or cap == 0:
        return R, t, sigma, normal, depth, info
    assert kp_xy.dtype == torch.float32 and H.dtype == torch.float64
    hint = None
    if normal_hint is not None:
        assert normal_hint.dtype == torch.float64
        hint = normal_hint.contiguous()
    prm = _lib.HPoseParams(int(min_matches), 0, float(min_front_frac), float(ambiguous_frac), float(rotation_tol))
    ctx.check(lib.mm_recover_poses_homography(ctx.h, Kh.ctypes.data_as(_lib.c_f64p), ptr(kp_xy.contiguous()),
                                              ptr(_i32(pairs.contiguous())), ptr(_i32(m.contiguous())), ptr(H.contiguous()),
                                              ptr(hint), n_pairs, cap, C.byref(prm), ptr(R), ptr(t), ptr(sigma), ptr(normal),
                                              ptr(depth), ptr(info)), "mm_recover_poses_homography")
    return R, t, sigma, normal, depth, info


RESECT_TOO_FEW, RESECT_NO_MODEL, RESECT_WEAK, RESECT_MALFORMED = 1, 2, 4, 8      # MM_RESECT_* of include/meatmodeler.h
RESECT_PLANAR = 16


def _resect_args(name, K, X, obs, pi, cam_ptr, cam_obs, pt_ok, prior, n_hyp, threshold_px, min_inliers, refit_iters, polish_iters,
                 inlier):
    """The argument checks and output buffers that resect_cameras and resect_planar share
    -> (Kh, pt_ok, prior, ext, cost, inlier, info, (n_cams, P, O, n_rows))."""
    Kh = _host_f64(K, 9, f"{name}: K")
    if not np.isfinite(Kh).all() or Kh[3] != 0 or Kh[6] != 0 or Kh[7] != 0 or Kh[8] != 1 or Kh[0] == 0 or Kh[4] == 0:
        raise ValueError(f"{name}: K must be finite, upper triangular with K[2, 2] = 1 and non-zero focal lengths")
    if not 1 <= int(n_hyp) <= 4096:
        raise ValueError(f"{name}: n_hyp must be in 1 .. 4096")
    if not float(threshold_px) >= 0:
        raise ValueError(f"{name}: threshold_px must not be negative")
    if not 0 <= int(refit_iters) <= 1000 or not 0 <= int(polish_iters) <= 1000 or int(min_inliers) < 0:
        raise ValueError(f"{name}: refit_iters and polish_iters must be in 0 .. 1000 and min_inliers not negative")
    if X.dim() != 2 or X.shape[1] != 3 or obs.dim() != 2 or obs.shape[1] != 2 or tuple(pi.shape) != (obs.shape[0],) \
            or cam_ptr.dim() != 1 or cam_ptr.shape[0] < 1 or cam_obs.dim() != 1:
        raise ValueError(f"{name}: X [P, 3], obs [O, 2], pi [O], cam_ptr [n_cams+1] and cam_obs [n_rows] expected")
    n_cams, P, O, n_rows = cam_ptr.shape[0] - 1, X.shape[0], obs.shape[0], cam_obs.shape[0]
    if pt_ok is not None:
        if tuple(pt_ok.shape) != (P,):
            raise ValueError(f"{name}: pt_ok [P] expected")
        pt_ok = pt_ok.to(torch.uint8).contiguous()
    if prior is not None:
        if prior.numel() != 12 * n_cams:
            raise ValueError(f"{name}: prior [n_cams, 3, 4] expected")
        prior = prior.to(torch.float64).contiguous()
    d = X.device
    ext = torch.full((n_cams, 3, 4), math.nan, dtype=torch.float64, device=d)
    cost = torch.full((n_cams,), math.nan, dtype=torch.float64, device=d)
    info = torch.zeros((n_cams, 6), dtype=torch.int32, device=d)
    if inlier is None:
        inlier = torch.zeros(O, dtype=torch.uint8, device=d)
    elif inlier.dtype != torch.uint8 or tuple(inlier.shape) != (O,) or not inlier.is_contiguous():
        raise ValueError(f"{name}: inlier must be a contiguous u8 tensor [O]")
    return Kh, pt_ok, prior, ext, cost, inlier, info, (n_cams, P, O, n_rows)


def resect_cameras(K, X, obs, pi, cam_ptr, cam_obs, pt_ok=None, prior=None, n_hyp=256, threshold_px=2.0, min_rows=12,
                   min_inliers=12, refit_iters=2, polish_iters=8, seed=0, cam_base=0, inlier=None, ctx=None, planar=None,
                   planar_tol=1e-2, collinear_tol=1e-3):
    """Every camera registered against the 3-D points it observes (mm_resect_cameras): K 3 x 3 on the host; X [P, 3] f64, obs
    [O, 2] f64 pixels, pi [O] i32, the camera CSR cam_ptr [n_cams+1] / cam_obs [n_rows] i32 (what a BADevice carries), optional
    pt_ok [P] u8 / bool (0: the point is not used) and prior [n_cams, 3, 4] or [n_cams, 12] f64 (a non-finite one counts as
    absent) -- device tensors
    -> (extrinsics [n_cams, 3, 4] f64, cost [n_cams] f64, inlier [O] u8 -- written for every usable or malformed row of a camera,
    zero (or what `inlier` held) elsewhere --, info [n_cams, 6] i32 = (RESECT_* flags, n_inliers, best_h (n_hyp: the prior, -1:
    none), valid hypotheses, usable rows, accepted polish steps)).
    `planar`: None (default) -- that call alone; "auto" -- that call, then resect_planar on the same inlier buffer: a camera
    whose points are coplanar (RESECT_PLANAR in the planar call's flags) takes the planar call's extrinsic, cost and info row,
    every other camera keeps its own (selected on the device, nothing is read back); "only" -- the planar call alone, its
    `plane` dropped.  planar_tol and collinear_tol go to resect_planar; min_rows goes to both calls, each with its own floor."""
    if planar not in (None, "auto", "only"):
        raise ValueError('resect_cameras: planar must be None, "auto" or "only"')
    common = dict(pt_ok=pt_ok, prior=prior, n_hyp=n_hyp, threshold_px=threshold_px, min_rows=min_rows, min_inliers=min_inliers,
                  refit_iters=refit_iters, polish_iters=polish_iters, seed=seed, cam_base=cam_base, ctx=ctx)
    if planar == "only":
        return resect_planar(K, X, obs, pi, cam_ptr, cam_obs, planar_tol=planar_tol, collinear_tol=collinear_tol, inlier=inlier,
                             **common)[:4]
    Kh, pt_ok, prior, ext, cost, inlier, info, (n_cams, P, O, n_rows) = _resect_args(
        "resect_cameras", K, X, obs, pi, cam_ptr, cam_obs, pt_ok, prior, n_hyp, threshold_px, min_inliers, refit_iters, polish_iters,
        inlier)
    ctx = ctx or default_context()
    if n_cams == 0:
        return ext, cost, inlier, info
    assert X.dtype == torch.float64 and obs.dtype == torch.float64
    prm = _lib.ResectParams(int(n_hyp), int(min_rows), int(min_inliers), int(refit_iters), int(polish_iters), 0,
                            int(seed) & 0xFFFFFFFF, int(cam_base) & 0xFFFFFFFF, float(threshold_px))
    wsb = lib.mm_resect_workspace_bytes(n_cams, int(n_hyp), n_rows)
    ws = torch.empty(wsb, dtype=torch.uint8, device=X.device)
    ctx.check(lib.mm_resect_cameras(ctx.h, Kh.ctypes.data_as(_lib.c_f64p), ptr(X.contiguous()), P, ptr(obs.contiguous()),
                                    ptr(_i32(pi.contiguous())), O, ptr(_i32(cam_ptr.contiguous())), ptr(_i32(cam_obs.contiguous())),
                                    n_rows, n_cams, ptr(pt_ok), ptr(prior), C.byref(prm), ptr(ext), ptr(cost), ptr(inlier),
                                    ptr(info), ptr(ws), wsb), "mm_resect_cameras")
    if planar == "auto":
        common["ctx"] = ctx
        pext, pcost, _, pinfo, _ = resect_planar(K, X, obs, pi, cam_ptr, cam_obs, planar_tol=planar_tol, collinear_tol=collinear_tol,
                                                 inlier=inlier, **common)
        took = (pinfo[:, 0] & RESECT_PLANAR) != 0
        ext = torch.where(took[:, None, None], pext, ext)
        cost = torch.where(took, pcost, cost)
        info = torch.where(took[:, None], pinfo, info)
    return ext, cost, inlier, info


def resect_planar(K, X, obs, pi, cam_ptr, cam_obs, pt_ok=None, prior=None, n_hyp=256, threshold_px=2.0, min_rows=8,
                  min_inliers=12, refit_iters=2, polish_iters=8, seed=0, cam_base=0, planar_tol=1e-2, collinear_tol=1e-3,
                  inlier=None, ctx=None):
    """Every camera whose usable points are coplanar registered by a RANSAC homography between their plane and the calibrated
    image (mm_resect_planar); arguments as resect_cameras takes them, planar_tol the largest thickness sqrt(l0 / l1) of a point
    set that counts as a plane, collinear_tol the near-collinearity bound of a sampled triple
    -> (extrinsics, cost, inlier, info, plane [n_cams, 6] f64 = (unit normal, normal . centroid, thickness, aspect)).  A camera
    without RESECT_PLANAR in its flags was refused: extrinsic = the prior or NaN, cost NaN, and its bytes of `inlier` are left
    as they were -- so a buffer that resect_cameras has filled can be handed on."""
    Kh, pt_ok, prior, ext, cost, inlier, info, (n_cams, P, O, n_rows) = _resect_args(
        "resect_planar", K, X, obs, pi, cam_ptr, cam_obs, pt_ok, prior, n_hyp, threshold_px, min_inliers, refit_iters, polish_iters,
        inlier)
    if not (float(planar_tol) >= 0 and math.isfinite(float(planar_tol)) and float(collinear_tol) >= 0
            and math.isfinite(float(collinear_tol))):
        raise ValueError("resect_planar: planar_tol and collinear_tol must be finite and not negative")
    ctx = ctx or default_context()
    plane = torch.full((n_cams, 6), math.nan, dtype=torch.float64, device=X.device)
    if n_cams == 0:
        return ext, cost, inlier, info, plane
    assert X.dtype == torch.float64 and obs.dtype == torch.float64
    prm = _lib.ResectPlanarParams(int(n_hyp), int(min_rows), int(min_inliers), int(refit_iters), int(polish_iters), 0,
                                  int(seed) & 0xFFFFFFFF, int(cam_base) & 0xFFFFFFFF, float(threshold_px), float(planar_tol),
                                  float(collinear_tol))
    wsb = lib.mm_resect_planar_workspace_bytes(n_cams, int(n_hyp), n_rows)
    ws = torch.empty(wsb, dtype=torch.uint8, device=X.device)
    ctx.check(lib.mm_resect_planar(ctx.h, Kh.ctypes.data_as(_lib.c_f64p), ptr(X.contiguous()), P, ptr(obs.contiguous()),
                                   ptr(_i32(pi.contiguous())), O, ptr(_i32(cam_ptr.contiguous())), ptr(_i32(cam_obs.contiguous())),
                                   n_rows, n_cams, ptr(pt_ok), ptr(prior), C.byref(prm), ptr(ext), ptr(cost), ptr(inlier),
                                   ptr(info), ptr(plane), ptr(ws), wsb), "mm_resect_planar")
    return ext, cost, inlier, info, plane


ALIGN_TOO_FEW, ALIGN_NO_MODEL, ALIGN_WEAK, ALIGN_NONFINITE = 1, 2, 4, 8      # MM_ALIGN_* of include/meatmodeler.h


def align_similarity(src, dst, ptr=None, tau=None, tau_rel=None, n_hyp=256, min_points=3, min_inliers=3, refit_iters=2,
                     with_scale=True, seed=0, prob_base=0, collinear_tol=1e-6, ctx=None):
    """A robust similarity per problem, dst ~ s R src + d (mm_align_similarity): src, dst [N, 3] f64 device tensors; ptr
    [n_prob+1] integers on the HOST (a sequence or array; None: one problem over all rows)
    -> (sim [n_prob, 13] f64 = (s, R row-major, d), NaN without a model; cost [n_prob] f64; inlier [N] u8; info [n_prob, 4] i32 =
    (ALIGN_* flags, n_inliers, best_h or -1, valid hypotheses)).
    Exactly one of `tau` (the inlier distance in dst units) and `tau_rel` must be given; tau_rel multiplies the root-mean-square
    distance of the finite rows of dst from their centroid (one problem only: tau is one number per call).  with_scale False:
    rigid, s = 1."""
    if (tau is None) == (tau_rel is None):
        raise ValueError("align_similarity: exactly one of tau and tau_rel must be given")
    if src.dim() != 2 or src.shape[1] != 3 or tuple(dst.shape) != tuple(src.shape):
        raise ValueError("align_similarity: src [N, 3] and dst [N, 3] expected")
    if src.dtype != torch.float64 or dst.dtype != torch.float64:
        raise ValueError("align_similarity: src and dst must be f64")
    N = src.shape[0]
    ph = np.array([0, N], np.int64) if ptr is None else np.ascontiguousarray(np.asarray(ptr, dtype=np.int64).ravel())
    if ph.size < 1 or ph[0] < 0 or (np.diff(ph) < 0).any() or ph[-1] > N:
        raise ValueError("align_similarity: ptr must start at or above 0, not decrease and end at or below N")
    n_prob = ph.size - 1
    if not 1 <= int(n_hyp) <= 4096:
        raise ValueError("align_similarity: n_hyp must be in 1 .. 4096")
    if not 0 <= int(refit_iters) <= 1000 or int(min_inliers) < 0:
        raise ValueError("align_similarity: refit_iters must be in 0 .. 1000 and min_inliers not negative")
    if not (float(collinear_tol) >= 0 and math.isfinite(float(collinear_tol))):
        raise ValueError("align_similarity: collinear_tol must be finite and not negative")
    src, dst = src.contiguous(), dst.contiguous()
    if tau_rel is not None:
        if n_prob > 1:
            raise ValueError("align_similarity: tau_rel needs a single problem (tau is one number per call)")
        if not (float(tau_rel) > 0 and math.isfinite(float(tau_rel))):
            raise ValueError("align_similarity: tau_rel must be finite and positive")
        rows = dst[int(ph[0]):int(ph[-1])]
        rows = rows[torch.isfinite(rows).all(dim=1)]
        spread = float(torch.sqrt(((rows - rows.mean(dim=0)) ** 2).sum(dim=1).mean())) if rows.shape[0] else math.nan
        tau = float(tau_rel) * spread if spread > 0 and math.isfinite(spread) else float(tau_rel)      # (no spread: nothing to scale by)
    if not (float(tau) > 0 and math.isfinite(float(tau))):
        raise ValueError("align_similarity: tau must be finite and positive")
    d = src.device
    sim = torch.full((n_prob, 13), math.nan, dtype=torch.float64, device=d)
    cost = torch.full((n_prob,), math.nan, dtype=torch.float64, device=d)
    inlier = torch.zeros(N, dtype=torch.uint8, device=d)
    info = torch.zeros((n_prob, 4), dtype=torch.int32, device=d)
    ctx = ctx or default_context()
    if n_prob == 0:
        return sim, cost, inlier, info
    prm = _lib.AlignParams(int(n_hyp), int(min_points), int(min_inliers), int(refit_iters), 1 if with_scale else 0, 0,
                           int(seed) & 0xFFFFFFFF, int(prob_base) & 0xFFFFFFFF, float(tau), float(collinear_tol))
    wsb = lib.mm_align_workspace_bytes(n_prob, int(n_hyp), int(ph[-1]))
    ws = torch.empty(wsb, dtype=torch.uint8, device=d)
    ctx.check(lib.mm_align_similarity(ctx.h, ptr_(src), ptr_(dst), ph.ctypes.data_as(_lib.c_i64p), n_prob, C.byref(prm), ptr_(sim),
                                      ptr_(cost), ptr_(inlier), ptr_(info), ptr_(ws), wsb), "mm_align_similarity")
    return sim, cost, inlier, info


def apply_similarity(sim, points=None, extrinsics=None, ctx=None):
    """A similarity applied in place (mm_apply_similarity): sim [13] f64 device tensor as align_similarity returns a row; points
    [P, 3] -> s R X + d; extrinsics [F, 3, 4] -> [Rc R^T | s tc - Rc R^T d], so that every projection is unchanged.  Both are
    contiguous f64 device tensors or None and are returned.  A non-finite sim changes nothing."""
    if sim.numel() != 13 or sim.dtype != torch.float64 or not sim.is_contiguous():
        raise ValueError("apply_similarity: sim must be a contiguous f64 tensor of 13 numbers")
    for name, t, tail in (("points", points, (3,)), ("extrinsics", extrinsics, (3, 4))):
        if t is not None and (t.dtype != torch.float64 or not t.is_contiguous() or tuple(t.shape[1:]) != tail):
            raise ValueError(f"apply_similarity: {name} must be a contiguous f64 tensor [n, {', '.join(map(str, tail))}]")
    ctx = ctx or default_context()
    P = 0 if points is None else points.shape[0]
    F = 0 if extrinsics is None else extrinsics.shape[0]
    ctx.check(lib.mm_apply_similarity(ctx.h, ptr_(sim), ptr_(points), P, ptr_(extrinsics), F), "mm_apply_similarity")
    return points, extrinsics


def camera_centres(extrinsics, ctx=None):
    """extrinsics [F, 3, 4] f64 device tensor -> the camera centres -Rc^T tc, [F, 3] f64 (mm_camera_centres)."""
    if extrinsics.dim() != 3 or tuple(extrinsics.shape[1:]) != (3, 4) or extrinsics.dtype != torch.float64:
        raise ValueError("camera_centres: extrinsics [F, 3, 4] f64 expected")
    ctx = ctx or default_context()
    ext = extrinsics.contiguous()
    Cn = torch.empty((ext.shape[0], 3), dtype=torch.float64, device=ext.device)
    ctx.check(lib.mm_camera_centres(ctx.h, ptr_(ext), ext.shape[0], ptr_(Cn)), "mm_camera_centres")
    return Cn


# ------------------------------------------------------------------------------------------------ ORB

def orb_params(nfeatures, nlevels=8, scale_factor=1.2, edge_threshold=31, fast_threshold=20):
    return OrbParams(int(nfeatures), int(nlevels), int(edge_threshold), int(fast_threshold), float(scale_factor), 0)


def orb_level_sizes(H, W, prm):
    L = prm.nlevels
    w = (C.c_int32 * L)()
    h = (C.c_int32 * L)()
    n = (C.c_int32 * L)()
    s = (C.c_float * L)()
    rc = lib.mm_orb_level_sizes(H, W, C.byref(prm), w, h, n, s)
    if rc != 0:
        raise _lib.MMError(f"mm_orb_level_sizes failed ({rc})")
    return np.array(w), np.array(h), np.array(n), np.array(s, np.float32)


class OrbWorkspace:
    """Reusable device workspace + output buffers for a fixed (batch, H, W, params)."""

    def __init__(self, batch, H, W, prm, device, pattern):
        self.batch, self.H, self.W, self.prm = batch, H, W, prm
        nb = lib.mm_orb_workspace_bytes(batch, H, W, C.byref(prm))
        if nb == 0:
            raise _lib.MMError("mm_orb_workspace_bytes: unsupported geometry")
        self.nbytes = nb
        self.ws = torch.empty(nb, dtype=torch.uint8, device=device)
        self.pattern = torch.as_tensor(np.ascontiguousarray(pattern, np.int8)).to(device)
        cap = prm.nfeatures
        self.xy = torch.zeros((batch, cap, 2), dtype=torch.float32, device=device)
        self.meta = torch.zeros((batch, cap, 4), dtype=torch.int32, device=device)
        self.resp = torch.zeros((batch, cap), dtype=torch.float32, device=device)
        self.mom = torch.zeros((batch, cap, 2), dtype=torch.int32, device=device)
        self.desc = torch.zeros((batch, cap, 32), dtype=torch.uint8, device=device)
        self.n = torch.zeros(batch, dtype=torch.int32, device=device)


def orb_detect_compute(imgs, wsp, ctx=None, out=None):
    """imgs [B,H,W] u8 (B <= wsp.batch).  Fills (and returns) wsp.xy/meta/resp/mom/desc/n for the first B frames,
    or the tensors in `out` = (xy, meta, resp, mom, desc, n) if given (each with leading dim >= B)."""
    ctx = ctx or default_context()
    assert imgs.dtype == torch.uint8 and imgs.dim() == 3 and imgs.stride(2) == 1
    B, H, W = imgs.shape
    assert B <= wsp.batch and H == wsp.H and W == wsp.W and imgs.stride(0) == H * imgs.stride(1)
    xy, meta, resp, mom, desc, n = out if out is not None else (wsp.xy, wsp.meta, wsp.resp, wsp.mom, wsp.desc, wsp.n)
    ctx.check(lib.mm_orb_detect_compute(ctx.h, ptr(imgs), B, H, W, imgs.stride(1), C.byref(wsp.prm), ptr(wsp.pattern),
                                        ptr(wsp.ws), wsp.nbytes, ptr(xy), ptr(meta), ptr(resp), ptr(mom), ptr(desc),
                                        ptr(n)), "mm_orb_detect_compute")
    return xy, meta, resp, mom, desc, n


# ------------------------------------------------------------------------------------------------ triangulation

def triangulate_dlt(proj, f0, f1, x0, x1, ctx=None):
    """proj [F,3,4] f64, f0/f1 int32 [n], x0/x1 f64 [n,2] -> X f64 [n,3]."""
    ctx = ctx or default_context()
    n = f0.shape[0]
    X = torch.empty((n, 3), dtype=torch.float64, device=proj.device)
    if n:
        lim = torch.stack([f0.min(), f1.min(), f0.max(), f1.max()]).tolist()
        if min(lim[:2]) < 0 or max(lim[2:]) >= proj.shape[0]:
            raise IndexError("triangulate_dlt: frame index outside the projection table")
        ctx.check(lib.mm_triangulate_dlt(ctx.h, ptr(proj.contiguous()), ptr(_i32(f0)), ptr(_i32(f1)),
                                         ptr(x0.contiguous()), ptr(x1.contiguous()), n, ptr(X)), "mm_triangulate_dlt")
    return X


TRI_BEHIND, TRI_REPROJ, TRI_PARALLAX, TRI_DEGENERATE = 1, 2, 4, 8      # MM_TRI_* of include/meatmodeler.h


def triangulate_tracks(proj, track_ptr, obs_frame, obs_xy, refine_iters=8, max_reproj_px=math.inf, min_angle_deg=0,
                       min_depth=-math.inf, ctx=None):
    """Multi-view triangulation of whole tracks (mm_triangulate_tracks): proj [F,3,4] f64, track_ptr [T+1] i32, obs_frame [O]
    i32, obs_xy [O,2] f64 in CSR order (device tensors; what flatten_tracks over all tracks gives)
    -> (X [T,3] f64, quality [T,4] f64 = (rms_px, max_px, min_depth, cos_parallax), flags [T] i32 of TRI_* bits).
    A track is flagged when max_px > max_reproj_px, its parallax angle is below min_angle_deg (0: test off) or
    min_depth <= min_depth; refine_iters Levenberg-Marquardt trial steps follow the linear solution."""
    if proj.dim() != 3 or tuple(proj.shape[1:]) != (3, 4):
        raise ValueError("triangulate_tracks: proj must be [F,3,4]")
    if not 0 <= int(refine_iters) <= 1000:
        raise ValueError("triangulate_tracks: refine_iters must be in 0 .. 1000")
    if not min_angle_deg >= 0:
        raise ValueError("triangulate_tracks: min_angle_deg must not be negative")
    ctx = ctx or default_context()
    d = proj.device
    F = proj.shape[0]
    tp = _i32(track_ptr.to(torch.int32).contiguous())
    of_ = _i32(obs_frame.to(torch.int32).contiguous())
    xy = obs_xy.to(torch.float64).contiguous()
    T, O = tp.numel() - 1, of_.numel()
    if T < 0 or xy.shape != (O, 2):
        raise ValueError("triangulate_tracks: track_ptr [T+1], obs_frame [O] and obs_xy [O,2] expected")
    X = torch.empty((T, 3), dtype=torch.float64, device=d)
    quality = torch.empty((T, 4), dtype=torch.float64, device=d)
    flags = torch.empty(T, dtype=torch.int32, device=d)
    if T == 0:
        return X, quality, flags
    lim = [tp[0], tp[-1], (tp[1:] - tp[:-1]).min()] + ([of_.min(), of_.max()] if O else [])
    lim = torch.stack([v.long() for v in lim]).tolist()      # (one read-back)
    if lim[0] < 0 or lim[1] > O or lim[2] < 0:
        raise ValueError("triangulate_tracks: track_ptr is not a CSR over the observations")
    if O and (lim[3] < 0 or lim[4] >= F):
        raise IndexError("triangulate_tracks: frame index outside the projection table")
    max_cos = math.cos(math.radians(min_angle_deg)) if min_angle_deg > 0 else 2.0
    prm = _lib.TriParams(int(refine_iters), 0, float(max_reproj_px), max_cos, float(min_depth))
    ws = torch.empty(max(lib.mm_triangulate_tracks_workspace_bytes(F), 256), dtype=torch.uint8, device=d)
    if O == 0:      # (no observation at all: a valid pointer for the kernel's never-read arrays)
        of_ = torch.zeros(1, dtype=torch.int32, device=d)
        xy = torch.zeros((1, 2), dtype=torch.float64, device=d)
    ctx.check(lib.mm_triangulate_tracks(ctx.h, ptr(proj.to(torch.float64).contiguous()), F, ptr(tp), T, ptr(of_), ptr(xy),
                                        C.byref(prm), ptr(X), ptr(quality), ptr(flags), ptr(ws), ws.numel()),
              "mm_triangulate_tracks")
    return X, quality, flags


# ------------------------------------------------------------------------------------------------ track linking

def link_tracks_device(kp_count, kp_xy, match_count, matches, ctx=None):
    """pointTracking over a whole clip on the device (mm_link_tracks_device; reference processor.py:190-243,418).
    kp_count [F] i32, kp_xy [F,cap,2] f32, match_count [F-1] i32, matches [F-1,cap,2] i32 (device tensors)
    -> (track_ptr [T+1] i32, obs_frame [O] i32, obs_kp [O] i32, bad) device tensors in the reference's final track
    order.  One host read-back (the two counts) sizes the views."""
    ctx = ctx or default_context()
    F, cap = kp_xy.shape[0], kp_xy.shape[1]
    d = kp_xy.device
    npairs = max(F - 1, 0)
    if matches.shape[0] != npairs or (npairs and matches.shape[1] != cap) or match_count.shape[0] != npairs:
        raise ValueError("link_tracks_device: matches must be [F-1, cap, 2] with match_count [F-1]")
    track_ptr = torch.empty(npairs * cap + 1, dtype=torch.int32, device=d)
    obs_frame = torch.empty(max(2 * npairs * cap, 1), dtype=torch.int32, device=d)
    obs_kp = torch.empty_like(obs_frame)
    counts = torch.zeros(3, dtype=torch.int64, device=d)
    wsb = lib.mm_link_workspace_bytes(F, cap)
    ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device=d)
    ctx.check(lib.mm_link_tracks_device(ctx.h, F, cap, ptr(_i32(kp_count)), ptr(kp_xy.contiguous()),
                                        ptr(_i32(match_count)), ptr(_i32(matches)), ptr(ws), ws.numel(), ptr(track_ptr),
                                        ptr(obs_frame), ptr(obs_kp), ptr(counts)), "mm_link_tracks_device")
    nt, no, bad = (int(v) for v in counts.cpu())
    return track_ptr[:nt + 1], obs_frame[:no], obs_kp[:no], bool(bad)


def flatten_tracks(track_ptr, obs_frame, obs_kp, kp_xy, sel=None, t_lo=0, n_sel=None, frame_offset=0, ctx=None):
    """managePoints on the device (mm_flatten_tracks; reference processor.py:264-291): the flat observation arrays of a
    selection of tracks.  track_ptr [T+1] i32, obs_frame / obs_kp [O] i32, kp_xy [F,cap,2] f32 (device tensors).
    sel = None: the tracks t_lo .. t_lo + n_sel - 1 (default: all); sel [n] integer tensor: these tracks, in this order.
    -> (coords [n_obs,2] f64, frame_indices [n_obs] i32 (minus frame_offset), point_indices [n_obs] i32) device tensors."""
    ctx = ctx or default_context()
    d = kp_xy.device
    cap = kp_xy.shape[1]
    tp = track_ptr.to(torch.int32).contiguous()
    T = tp.numel() - 1
    out_ptr = None
    if sel is None:
        n_sel = T - t_lo if n_sel is None else int(n_sel)
        if n_sel < 0 or t_lo < 0 or t_lo + n_sel > T:
            raise ValueError("flatten_tracks: range outside the track list")
        n_obs = int((tp[t_lo + n_sel] - tp[t_lo]).item()) if n_sel else 0      # (one read-back sizes the outputs)
        sel_t = None
    else:
        sel_t = sel.to(torch.int32).contiguous()
        n_sel = sel_t.numel()
        out_ptr = torch.empty(n_sel + 1, dtype=torch.int64, device=d)
        ctx.check(lib.mm_flatten_offsets(ctx.h, ptr(tp), ptr(sel_t) if n_sel else None, n_sel, ptr(out_ptr)), "mm_flatten_offsets")
        n_obs = int(out_ptr[n_sel].item())
    coords = torch.empty((n_obs, 2), dtype=torch.float64, device=d)
    fi = torch.empty(n_obs, dtype=torch.int32, device=d)
    pi = torch.empty(n_obs, dtype=torch.int32, device=d)
    if n_obs:
        ctx.check(lib.mm_flatten_tracks(ctx.h, ptr(tp), ptr(obs_frame.to(torch.int32).contiguous()), ptr(obs_kp.to(torch.int32).contiguous()),
                                        ptr(kp_xy.contiguous()), cap,
                                        ptr(sel_t) if sel_t is not None else None, int(t_lo), n_sel,
                                        ptr(out_ptr) if out_ptr is not None else None, n_obs, int(frame_offset), ptr(coords),
                                        ptr(fi), ptr(pi)), "mm_flatten_tracks")
    return coords, fi, pi


# ------------------------------------------------------------------------------------------------ bundle adjustment

def ba_build_index(F, P, fi, pi):
    """Host CSR build (mm_ba_build_index).  fi, pi: int32 numpy [O]."""
    fi = np.ascontiguousarray(fi, np.int32)
    pi = np.ascontiguousarray(pi, np.int32)
    O = fi.size
    pt_ptr = np.zeros(P + 1, np.int32)
    cam_ptr = np.zeros(F + 1, np.int32)
    pt_obs = np.zeros(max(O, 1), np.int32)
    cam_obs = np.zeros(max(O, 1), np.int32)
    i32p = _lib.c_i32p
    rc = lib.mm_ba_build_index(F, P, O, fi.ctypes.data_as(i32p), pi.ctypes.data_as(i32p), pt_ptr.ctypes.data_as(i32p),
                               pt_obs.ctypes.data_as(i32p), cam_ptr.ctypes.data_as(i32p), cam_obs.ctypes.data_as(i32p))
    if rc != 0:
        raise ValueError(f"mm_ba_build_index failed ({rc}): frame/point index out of range")
    return pt_ptr, pt_obs[:O], cam_ptr, cam_obs[:O]


class BADevice:
    """Device-resident BA problem: observation arrays, CSR indices and the mm_ba_problem descriptor."""

    def __init__(self, K, fi, pi, obs, F, P, device, ctx=None, pairs=True, max_band_span=192, fixed_cams=None):
        """fi, pi: int [O] (numpy or device tensors), obs [O,2] f64 (numpy or device tensor).  All index structures
        (CSR by point, CSR by camera, co-observation pair list and its chunk table) are built on the device by
        mm_ba_index_build: two native calls with a host read-back each, and one more of each for observations that are
        not point-major (self.point_major says whether they are).

        fixed_cams: [F_fixed, 6] f64 device tensor of cameras that are observed but not optimised (mm_ba_fixed):
        fi in [F, F + F_fixed) is fixed camera fi - F.  The CSR by camera and the pair list then cover the F free
        cameras only, and residual / normal_eq / trf_solve run the *_fixed entry points; the other sweeps have no
        fixed-camera form and raise NotImplementedError."""
        self.ctx = ctx or default_context()
        self._mdot = None
        dev = device
        self.device = dev
        self.F, self.P, self.O = int(F), int(P), int(len(fi))
        F, P, O = self.F, self.P, self.O

        def to_dev(a, dtype):
            if isinstance(a, torch.Tensor):
                return a.to(device=dev, dtype=dtype).contiguous()
            return torch.as_tensor(np.ascontiguousarray(a)).to(device=dev, dtype=dtype).contiguous()

        self.K = to_dev(np.asarray(K, np.float64).reshape(9), torch.float64)
        self.fi = to_dev(fi, torch.int32).reshape(-1)
        self.pi = to_dev(pi, torch.int32).reshape(-1)
        self.obs = to_dev(obs, torch.float64).reshape(-1, 2)
        self.fixed_cams, self.F_fixed, self.fx = None, 0, None
        if fixed_cams is not None:
            assert (isinstance(fixed_cams, torch.Tensor) and fixed_cams.dtype == torch.float64 and fixed_cams.device == dev
                    and fixed_cams.dim() == 2 and fixed_cams.shape[1] == 6), "fixed_cams: [F_fixed, 6] f64 device tensor"
            self.F_fixed = int(fixed_cams.shape[0])
            if self.F_fixed:
                self.fixed_cams = fixed_cams.contiguous()
                self.fx = _lib.BAFixed(self.F_fixed, 0, ptr(self.fixed_cams))
        self.cam_span = 0
        self.max_band_span = int(max_band_span)
        self._slabs = None
        self.n_pairs = 0
        # build + solve overlapped on two streams (mm_ba_schur_solve).  Needs concurrent kernel execution: tools that
        # serialise kernels (rocprofv3 --pmc, launch-blocking debug modes) make the consumer wait for a producer that
        # cannot start; its bounded spins then give up (info = -1) and the driver falls back to one after the other.
        # Off by default since the factorisation became two-ended: its 137 workgroups use the whole register file of
        # their CUs (one wave per SIMD), the build slows down by 1.6x beside them and build-then-solve (0.32 + 0.59 ms at
        # 500 cameras) beats the overlapped pair (0.93 ms).  MM_SCHUR_OVERLAP=1 selects the overlapped path.
        self.overlap = os.environ.get("MM_SCHUR_OVERLAP", "0") != "0"
        if O and F + self.F_fixed > 0 and P > 0:
            self._build_index(pairs)
        elif O:
            raise ValueError("frame / point index out of range")
        else:      # no observations: empty CSRs, no pair list
            i32 = dict(dtype=torch.int32, device=dev)
            self.point_major = True
            self.pt_ptr, self.pt_obs = torch.zeros(P + 1, **i32), torch.zeros(0, **i32)
            self.cam_ptr, self.cam_obs = torch.zeros(F + 1, **i32), torch.zeros(0, **i32)
            self._set_problem()
        self._ws = torch.empty(2048 * 8, dtype=torch.uint8, device=dev)
        self._cost2 = torch.zeros(1, dtype=torch.float64, device=dev)
        self._S = None  # reduced camera system, allocated once (6F x 6F doubles)
        self._schur_ws = None
        self._chol_ws = None

    @staticmethod
    def _chunk_pairs():
        # pairs per chunk = per wave of the pair kernel (a multiple of 64: whole lane strides).  512 since the second
        # half of round 4: 230 us per build at the bench shape against 249 with 256 (384: 230; 1024: slower)
        return max(64, int(os.environ.get("MM_SCHUR_CHUNK", "512")) // 64 * 64)

    @property
    def slabs(self):
        """Camera slabs for the overlapped build + solve (mm_ba_schur_solve): first segment / chunk of each slab, or
        None.  Left to the first reader (two more host read-backs; the path that wants them, MM_SCHUR_OVERLAP=1, is off
        by default)."""
        n_slabs = 8
        cps = -(-self.F // n_slabs)
        if self._slabs is None and self.n_pairs and cps >= 16:
            seg_cam = self.seg_ids.to(torch.int64) // (self.cam_span + 1)
            bounds = torch.arange(n_slabs + 1, dtype=torch.int64, device=self.device) * cps
            sseg = torch.searchsorted(seg_cam, bounds)
            schunk = self.seg_chunk_ptr.to(torch.int64)[sseg]
            self._slabs = (n_slabs, cps, np.ascontiguousarray(sseg.cpu().numpy(), np.int64),
                           np.ascontiguousarray(schunk.cpu().numpy(), np.int64))
        return self._slabs

    def _set_problem(self):
        """The problem descriptor over the observation arrays and the two CSRs, without a pair list."""
        self.pb = BAProblem(self.F, self.P, self.O, ptr(self.K), ptr(self.fi), ptr(self.pi), ptr(self.obs),
                            ptr(self.pt_ptr), ptr(self.pt_obs), ptr(self.cam_ptr), ptr(self.cam_obs),
                            self.cam_span, 0, 0, None, None, 0, None, None, None, None, None, None)

    def _set_pair_list(self, pair_o, pair_o2, pair_p, seg_ids, seg_chunk_ptr, chunk_seg, chunk_begin, chunk_end):
        """Keeps the co-observation pair list (int32 device tensors) and points the problem descriptor at it."""
        self.pair_o, self.pair_o2, self.pair_p = pair_o, pair_o2, pair_p
        self.seg_ids, self.seg_chunk_ptr = seg_ids, seg_chunk_ptr
        self.chunk_seg, self.chunk_begin, self.chunk_end = chunk_seg, chunk_begin, chunk_end
        self.n_pairs = int(pair_o.numel())
        self.pb.n_seg = int(seg_ids.numel())
        self.pb.n_chunks = int(chunk_seg.numel())
        self.pb.seg_ids, self.pb.seg_chunk_ptr = ptr(seg_ids), ptr(seg_chunk_ptr)
        self.pb.chunk_seg, self.pb.chunk_begin, self.pb.chunk_end = ptr(chunk_seg), ptr(chunk_begin), ptr(chunk_end)
        self.pb.pair_o, self.pb.pair_o2, self.pb.pair_p = ptr(pair_o), ptr(pair_o2), ptr(pair_p)

    def _build_index(self, pairs):
        """mm_ba_index_build: stage 0 (again with the sort by point when the observations are not point-major), and for a
        banded problem stage 1."""
        F, P, O, dev = self.F, self.P, self.O, self.device
        i32 = dict(dtype=torch.int32, device=dev)
        pt_ptr, pt_obs = torch.empty(P + 1, **i32), torch.empty(O, **i32)
        cam_ptr, cam_obs = torch.empty(F + 1, **i32), torch.empty(O, **i32)
        head = torch.empty(8, dtype=torch.int64, device=dev)
        ix = _lib.BAIndex(F, P, O, self.F_fixed, 0, ptr(self.fi), ptr(self.pi), ptr(pt_ptr), ptr(pt_obs), ptr(cam_ptr), ptr(cam_obs),
                          ptr(head), 0, self._chunk_pairs(), 0, None, None, None, None, None, None, None, None)

        def stage0():
            ws0b = lib.mm_ba_index_workspace_bytes(self.ctx.h, C.byref(ix), 0)
            if not ws0b:
                raise _lib.MMError("mm_ba_index_workspace_bytes: no workspace size for stage 0")
            ws0 = torch.empty(ws0b, dtype=torch.uint8, device=dev)
            self.ctx.check(lib.mm_ba_index_build(self.ctx.h, C.byref(ix), 0, ptr(ws0), ws0b, None, 0), "mm_ba_index_build")
            return ws0, ws0b, head[:7].tolist()      # read-back 1 of 2

        ws0, ws0b, (span, n, bad_range, not_point_major, _, _, n_free) = stage0()
        if bad_range:
            raise ValueError("frame / point index out of range")
        self.point_major = not not_point_major
        if not_point_major:      # (one more read-back, for input that flatten_tracks did not make)
            ix.sort_by_point = 1
            ws0, ws0b, (span, n, _, _, _, _, n_free) = stage0()
        self.pt_ptr, self.pt_obs, self.cam_ptr, self.cam_obs = pt_ptr, pt_obs, cam_ptr, cam_obs[:n_free]
        self.cam_span = int(span)
        self._set_problem()
        # banded problems: co-observation pair list for the atomic-free, bitwise reproducible Schur kernel;
        # wide spans keep the general kernel
        if pairs and n and self.cam_span <= self.max_band_span and self.cam_span < F and F * (self.cam_span + 1) < 2 ** 31:
            seg_cap, chunk_cap = C.c_int64(0), C.c_int64(0)
            lib.mm_ba_index_bounds(F, self.cam_span, n, ix.chunk, C.byref(seg_cap), C.byref(chunk_cap))
            seg_cap, chunk_cap = seg_cap.value, chunk_cap.value
            pair_o, pair_o2, pair_p = torch.empty(n, **i32), torch.empty(n, **i32), torch.empty(n, **i32)
            seg_ids, seg_chunk_ptr = torch.empty(seg_cap, **i32), torch.empty(seg_cap + 1, **i32)
            chunk_seg, chunk_begin, chunk_end = (torch.empty(chunk_cap, **i32) for _ in range(3))
            ix.cam_span, ix.n_pairs = self.cam_span, n
            ix.pair_o, ix.pair_o2, ix.pair_p = ptr(pair_o), ptr(pair_o2), ptr(pair_p)
            ix.seg_ids, ix.seg_chunk_ptr = ptr(seg_ids), ptr(seg_chunk_ptr)
            ix.chunk_seg, ix.chunk_begin, ix.chunk_end = ptr(chunk_seg), ptr(chunk_begin), ptr(chunk_end)
            ws1b = lib.mm_ba_index_workspace_bytes(self.ctx.h, C.byref(ix), 1)
            if not ws1b:
                raise _lib.MMError("mm_ba_index_workspace_bytes: no workspace size for stage 1")
            ws1 = torch.empty(ws1b, dtype=torch.uint8, device=dev)
            self.ctx.check(lib.mm_ba_index_build(self.ctx.h, C.byref(ix), 1, ptr(ws0), ws0b, ptr(ws1), ws1b), "mm_ba_index_build")
            n_seg, n_chunks = head[4:6].tolist()      # read-back 2 of 2 (the workspaces are free to go after it)
            self._set_pair_list(pair_o, pair_o2, pair_p, seg_ids[:n_seg], seg_chunk_ptr[:n_seg + 1], chunk_seg[:n_chunks],
                                chunk_begin[:n_chunks], chunk_end[:n_chunks])

    def residual(self, cams, pts, want_res=False, cost_out=None):
        """-> (sum of squared residuals as a 1-element device tensor, res [O,2] or None).  cost_out: where to put the
        sum (a 1-element f64 device tensor, e.g. a slot of the trust-region driver's scalar board)."""
        res = torch.empty((self.O, 2), dtype=torch.float64, device=self.device) if want_res else None
        cost2 = cost_out if cost_out is not None else torch.empty(1, dtype=torch.float64, device=self.device)
        if self.fx is not None:
            self.ctx.check(lib.mm_ba_residual_fixed(self.ctx.h, C.byref(self.pb), C.byref(self.fx), ptr(cams), ptr(pts),
                                                    ptr(res), ptr(cost2), ptr(self._ws), self._ws.numel()),
                           "mm_ba_residual_fixed")
            return cost2, res
        self.ctx.check(lib.mm_ba_residual(self.ctx.h, C.byref(self.pb), ptr(cams), ptr(pts), ptr(res), ptr(cost2),
                                          ptr(self._ws), self._ws.numel()), "mm_ba_residual")
        return cost2, res

    def _no_fixed(self, what):
        if self.fx is not None:
            raise NotImplementedError(f"BADevice.{what}: no fixed-camera form (residual, normal_eq and trf_solve have one)")

    def jacobian(self, cams, pts):
        self._no_fixed("jacobian")
        Jc = torch.empty((self.O, 2, 6), dtype=torch.float64, device=self.device)
        Jp = torch.empty((self.O, 2, 3), dtype=torch.float64, device=self.device)
        self.ctx.check(lib.mm_ba_jacobian(self.ctx.h, C.byref(self.pb), ptr(cams), ptr(pts), ptr(Jc), ptr(Jp)),
                       "mm_ba_jacobian")
        return Jc, Jp

    def normal_eq(self, cams, pts, want_cams=True, want_pts=True, out=None):
        """-> (B [F,6,6], gc [F,6], C [P,6], gp [P,3]); `out` = the four tensors to fill (any contiguous storage of
        the right size, e.g. the two halves of the flat gradient vector for gc / gp)."""
        d = self.device
        if out is not None:
            B, gc, Cb, gp = out
            for t_ in out:
                assert t_ is None or (t_.dtype == torch.float64 and t_.is_contiguous())
        else:
            B = torch.empty((self.F, 6, 6), dtype=torch.float64, device=d) if want_cams else None
            gc = torch.empty((self.F, 6), dtype=torch.float64, device=d) if want_cams else None
            Cb = torch.empty((self.P, 6), dtype=torch.float64, device=d) if want_pts else None
            gp = torch.empty((self.P, 3), dtype=torch.float64, device=d) if want_pts else None
        if self.fx is not None:
            self.ctx.check(lib.mm_ba_normal_eq_fixed(self.ctx.h, C.byref(self.pb), C.byref(self.fx), ptr(cams), ptr(pts),
                                                     ptr(B), ptr(gc), ptr(Cb), ptr(gp)), "mm_ba_normal_eq_fixed")
            return B, gc, Cb, gp
        self.ctx.check(lib.mm_ba_normal_eq(self.ctx.h, C.byref(self.pb), ptr(cams), ptr(pts), ptr(B), ptr(gc), ptr(Cb),
                                           ptr(gp)), "mm_ba_normal_eq")
        return B, gc, Cb, gp

    def jvp(self, cams, pts, wc, wp):
        self._no_fixed("jvp")
        out = torch.empty((self.O, 2), dtype=torch.float64, device=self.device)
        self.ctx.check(lib.mm_ba_jvp(self.ctx.h, C.byref(self.pb), ptr(cams), ptr(pts), ptr(wc), ptr(wp), ptr(out)),
                       "mm_ba_jvp")
        return out

    def jvp_dots(self, cams, pts, wc, wp, other=None):
        """jvp with its inner products fused in (mm_ba_jvp_dots): -> (out [O,2], rows [2,3]) with rows[0] = <out, other>
        (other None: <out, out>) and rows[1] = <out, out>, each as {0, total, total}."""
        self._no_fixed("jvp_dots")
        out = torch.empty((self.O, 2), dtype=torch.float64, device=self.device)
        rows = torch.empty((2, 3), dtype=torch.float64, device=self.device)
        if getattr(self, "_jvp_ws", None) is None:
            self._jvp_ws = torch.zeros(lib.mm_ba_jvp_dots_workspace_bytes(C.byref(self.pb)), dtype=torch.uint8,
                                       device=self.device)
        self.ctx.check(lib.mm_ba_jvp_dots(self.ctx.h, C.byref(self.pb), ptr(cams), ptr(pts), ptr(wc), ptr(wp), ptr(out),
                                          ptr(other), ptr(rows), ptr(self._jvp_ws), self._jvp_ws.numel()), "mm_ba_jvp_dots")
        return out, rows

    def schur(self, cams, pts, Bd, Cd, gc, gp):
        """Reduced camera system.  With a pair list (banded problems) only the LOWER block band of S is produced
        (deterministically) and the rest of S is zero; otherwise all of S is filled."""
        self._no_fixed("schur")
        n = 6 * self.F
        S = self._schur_buffers(n)
        v = torch.empty(n, dtype=torch.float64, device=self.device)
        Cinv = torch.empty((self.P, 6), dtype=torch.float64, device=self.device)
        self.ctx.check(lib.mm_ba_schur(self.ctx.h, C.byref(self.pb), ptr(cams), ptr(pts), ptr(Bd), ptr(Cd), ptr(gc),
                                       ptr(gp), ptr(S), ptr(v), ptr(Cinv), ptr(self._schur_ws),
                                       self._schur_ws.numel()), "mm_ba_schur")
        return S, v, Cinv

    def _alloc_S(self, n):
        # n extra (zeroed) rows behind the matrix: band_view's diagonal-major strides run past row n - 1
        self._S_storage = torch.zeros(2 * n * n, dtype=torch.float64, device=self.device)
        self._S = self._S_storage[:n * n].view(n, n)

    def _schur_buffers(self, n):
        """S and the workspace of the Schur build, allocated on first use.  -> S"""
        if self._S is None:
            self._alloc_S(n)
        if self._schur_ws is None:
            nb = lib.mm_ba_schur_workspace_bytes(C.byref(self.pb))
            self._schur_ws = torch.empty(max(nb, 256), dtype=torch.uint8, device=self.device)
        return self._S

    def band_view(self, half_bandwidth):
        """The lower band of the reduced camera system as a strided [n, hb + 1] view of its storage: entry [j, k] is
        S[j + k, j] (rows past n - 1 fall into the zero padding).  What ranks exchange instead of the dense matrix."""
        n = 6 * self.F
        hb = int(min(half_bandwidth, n - 1))
        return torch.as_strided(self._S_storage, (n, hb + 1), (n + 1, n))

    def schur_solve(self, cams, pts, Bd, Cd, gc, gp, half_bandwidth):
        """Reduced camera system built and solved in one overlapped call (mm_ba_schur_solve): -> (info, dc [6F], Cinv).
        dc is the solution of S dc = v (the camera part of the damped Gauss-Newton step)."""
        self._no_fixed("schur_solve")
        n = 6 * self.F
        self._schur_buffers(n)
        v = torch.empty(n, dtype=torch.float64, device=self.device)
        Cinv = torch.empty((self.P, 6), dtype=torch.float64, device=self.device)
        info = torch.zeros(1, dtype=torch.int32, device=self.device)
        if self._chol_ws is None:
            self._chol_ws = torch.empty(lib.mm_chol_workspace_bytes(n), dtype=torch.uint8, device=self.device)
        hb = int(min(half_bandwidth, n))
        if self.overlap and self.slabs is not None:
            ns, cps, sseg, schunk = self.slabs
            a_seg, a_chunk = sseg.ctypes.data_as(_lib.c_i64p), schunk.ctypes.data_as(_lib.c_i64p)
        else:
            ns, cps, a_seg, a_chunk = 0, 0, None, None
        self.ctx.check(lib.mm_ba_schur_solve(self.ctx.h, C.byref(self.pb), ptr(cams), ptr(pts), ptr(Bd), ptr(Cd), ptr(gc),
                                             ptr(gp), ptr(self._S), ptr(v), ptr(Cinv), hb, ptr(info), ptr(self._schur_ws),
                                             self._schur_ws.numel(), ptr(self._chol_ws), self._chol_ws.numel(), ns, cps,
                                             a_seg, a_chunk), "mm_ba_schur_solve")
        return info, v, Cinv

    def multi_dot(self, pairs, split=0):
        """[k, 3] device tensor of inner products (camera part, point part, total); see ops.MultiDot."""
        if self._mdot is None:
            self._mdot = MultiDot(self.device, self.ctx)
        return self._mdot(pairs, split)

    _FUSED_ROWS = (2, 3, 2, 6, 0, 0)

    def trf_fused(self, op, ins, outs, scalars=(), h0=0.0, h1=0.0, split=0):
        """One fused element-wise pass of the trust-region step with its inner products (mm_trf_fused).
        -> device tensor [rows, 3] = (camera part, point part, total) per inner product, last row: maxima."""
        if self._mdot is None:
            self._mdot = MultiDot(self.device, self.ctx)
        ws = self._mdot.ws
        n = outs[0].numel()
        for t in list(ins) + list(outs) + list(scalars):
            assert t.dtype == torch.float64 and t.is_contiguous()
        pin = (C.c_void_p * len(ins))(*[t.data_ptr() for t in ins])
        pout = (C.c_void_p * len(outs))(*[t.data_ptr() for t in outs])
        psc = (C.c_void_p * max(len(scalars), 1))(*[t.data_ptr() for t in scalars]) if scalars else None
        rows = self._FUSED_ROWS[op]
        if n == 0:
            return torch.zeros((max(rows, 1), 3), dtype=torch.float64, device=self.device)
        res = torch.empty((max(rows, 1), 3), dtype=torch.float64, device=self.device)
        self.ctx.check(lib.mm_trf_fused(self.ctx.h, op, pin, pout, psc, float(h0), float(h1), n, int(split), ptr(res), ptr(ws),
                                        ws.numel()), "mm_trf_fused")
        return res

    def trf_step2d(self, r0, d11, r1, r2, r3, bs, reg, info, Delta, board):
        """2-D trust-region subproblem on the device from the fused passes' results (mm_trf_step2d) -> board[0:14]."""
        self.ctx.check(lib.mm_trf_step2d(self.ctx.h, ptr(r0), ptr(d11), ptr(r1), ptr(r2), ptr(r3), ptr(bs), ptr(reg),
                                         ptr(info), float(Delta), ptr(board)), "mm_trf_step2d")

    def trf_damping(self, gh2, d11, Delta, min_damping):
        """Device scalars -> tensor [reg, max(reg, min_damping)] (see ops.trf_damping)."""
        return trf_damping(gh2, d11, Delta, min_damping, self.ctx)

    def chol_solve(self, S, v, half_bandwidth=None):
        """In-place banded Cholesky solve of the reduced camera system (see ops.chol_solve)."""
        return chol_solve(S, v, self.ctx, half_bandwidth=half_bandwidth)

    def scale_update(self, B, Cb, si, first):
        """si <- sqrt(diag(J^T J)) (first: zeros -> 1) or max(si, sqrt(diag)) in one launch (mm_ba_scale_update)."""
        self.ctx.check(lib.mm_ba_scale_update(self.ctx.h, self.F, self.P, ptr(B), ptr(Cb), ptr(si), 1 if first else 0),
                       "mm_ba_scale_update")
        return si

    def damp(self, B, Cb, si, reg, Bd, Cd):
        """Bd = B + reg diag(si_c^2), Cd = C + reg diag(si_p^2); reg: 1-element device tensor (mm_ba_damp)."""
        assert reg.dtype == torch.float64 and reg.numel() == 1
        self.ctx.check(lib.mm_ba_damp(self.ctx.h, self.F, self.P, ptr(B), ptr(Cb), ptr(si), ptr(reg), ptr(Bd), ptr(Cd)),
                       "mm_ba_damp")
        return Bd, Cd

    def chol_solve_sym(self, S, v, half_bandwidth, both_triangles):
        """Solution only (S destroyed): lets a narrow band be eliminated from both ends (see ops.chol_solve_sym)."""
        return chol_solve_sym(S, v, self.ctx, half_bandwidth, both_triangles)

    def trf_solve(self, cams, pts, ftol, xtol, gtol, max_nfev=None, min_damping=1e-9, log_cap=0):
        """The whole trust-region solve in one library call (mm_ba_trf; one GPU).  cams [F,6] / pts [P,3] are updated in
        place.  -> (report, rows) with rows = the (iteration, nfev, cost, reduction, step_norm, optimality) lines of
        SciPy's verbose=2 table (the first `log_cap` of them)."""
        for t in (cams, pts):
            assert t.dtype == torch.float64 and t.is_contiguous() and t.device == self.device
        if getattr(self, "_trf_ws", None) is None:
            nb = (lib.mm_ba_trf_fixed_workspace_bytes(C.byref(self.pb), C.byref(self.fx)) if self.fx is not None
                  else lib.mm_ba_trf_workspace_bytes(C.byref(self.pb)))
            self._trf_ws = torch.empty(nb, dtype=torch.uint8, device=self.device)
        prm = _lib.TrfParams(ftol, xtol, gtol, min_damping, int(max_nfev) if max_nfev else 0)
        rep = _lib.TrfReport()
        log = (_lib.TrfRow * max(log_cap, 1))()
        if self.fx is not None:      # (fixed cameras: mm_ba_trf_fixed, the same loop over the free parameters)
            name = "mm_ba_trf_fixed"
            rc = lib.mm_ba_trf_fixed(self.ctx.h, C.byref(self.pb), C.byref(self.fx), ptr(cams), ptr(pts), C.byref(prm),
                                     C.byref(rep), log, int(log_cap), ptr(self._trf_ws), self._trf_ws.numel())
        else:
            name = "mm_ba_trf"
            rc = lib.mm_ba_trf(self.ctx.h, C.byref(self.pb), ptr(cams), ptr(pts), C.byref(prm), C.byref(rep), log,
                               int(log_cap), ptr(self._trf_ws), self._trf_ws.numel())
        if rc and rep.status == -2:
            raise ValueError("Residuals are not finite in the initial point.")      # (as scipy's least_squares does)
        self.ctx.check(rc, name)
        rows = [(r.iteration, r.nfev, r.cost, r.reduction, r.step_norm, r.optimality)
                for r in log[:min(rep.log_rows, log_cap)]]
        return rep, rows

    def trf_solve_dist(self, cams, pts, ftol, xtol, gtol, allreduce, half_bandwidth, band_exchange, max_nfev=None,
                       min_damping=1e-9, log_cap=0):
        """mm_ba_trf_dist: the same loop sharded over ranks (this problem = the rank's points).  `allreduce` is a callable
        summing a device tensor over the ranks in place (parallel.AllReduce); the library calls back with pointers into its
        workspace, which are wrapped as tensor views here.  -> (report, rows) like trf_solve.
        An exception raised by `allreduce` -- or any error on this rank -- is FATAL FOR THE WHOLE GROUP: this rank leaves
        the loop while its peers wait inside their next collective (include/meatmodeler.h); it is re-raised here and the
        caller is expected to tear the process group down (its timeout bounds the peers' wait otherwise)."""
        self._no_fixed("trf_solve_dist")
        for t in (cams, pts):
            assert t.dtype == torch.float64 and t.is_contiguous() and t.device == self.device
        need = lib.mm_ba_trf_dist_workspace_bytes(C.byref(self.pb), int(half_bandwidth))
        if getattr(self, "_trf_ws_dist", None) is None or self._trf_ws_dist.numel() < need:
            self._trf_ws_dist = torch.empty(need, dtype=torch.uint8, device=self.device)
        ws = self._trf_ws_dist
        base = ws.data_ptr()
        err = []

        def _cb(user, buf, count):
            try:
                off = int(buf) - base
                with torch.cuda.stream(self.ctx.stream):      # ordered on the stream the library launches on
                    allreduce(ws[off:off + 8 * int(count)].view(torch.float64))
                return 0
            except BaseException as e:      # (nothing may propagate through the C frames)
                err.append(e)
                return 1
        cb = _lib.ALLREDUCE_FN(_cb)
        d = _lib.Dist(int(getattr(allreduce, "rank", 0)), int(getattr(allreduce, "world_size", 1)), int(half_bandwidth),
                      1 if band_exchange else 0, cb, None)
        prm = _lib.TrfParams(ftol, xtol, gtol, min_damping, int(max_nfev) if max_nfev else 0)
        rep = _lib.TrfReport()
        log = (_lib.TrfRow * max(log_cap, 1))()
        rc = lib.mm_ba_trf_dist(self.ctx.h, C.byref(self.pb), ptr(cams), ptr(pts), C.byref(prm), C.byref(rep), log,
                                int(log_cap), ptr(ws), ws.numel(), C.byref(d))
        if err:
            raise err[0]
        if rc and rep.status == -2:
            raise ValueError("Residuals are not finite in the initial point.")
        self.ctx.check(rc, "mm_ba_trf_dist")
        rows = [(r.iteration, r.nfev, r.cost, r.reduction, r.step_norm, r.optimality)
                for r in log[:min(rep.log_rows, log_cap)]]
        return rep, rows

    def backsub(self, cams, pts, Cinv, gp, dc):
        self._no_fixed("backsub")
        dp = torch.empty((self.P, 3), dtype=torch.float64, device=self.device)
        if getattr(self, "_backsub_ws", None) is None:
            self._backsub_ws = torch.empty(lib.mm_ba_backsub_workspace_bytes(C.byref(self.pb)), dtype=torch.uint8,
                                           device=self.device)
        self.ctx.check(lib.mm_ba_backsub(self.ctx.h, C.byref(self.pb), ptr(cams), ptr(pts), ptr(Cinv), ptr(gp), ptr(dc),
                                         ptr(dp), ptr(self._backsub_ws), self._backsub_ws.numel()), "mm_ba_backsub")
        return dp


def trf_solve_batched(problems, cams_list, pts_list, ftol, xtol, gtol, max_nfev=None, min_damping=1e-9, ctx=None):
    """mm_ba_trf_batched: several independent problems (BADevice objects on one device) advanced in lock-step -- every
    kernel of the trust-region loop once per round for all of them.  cams_list[p] [F_p,6] / pts_list[p] [P_p,3] are
    updated in place; results are bit-identical to BADevice.trf_solve problem by problem.
    -> (list of reports, list of bool "was solved alone after the batch")."""
    n = len(problems)
    if n == 0:
        return [], []
    ctx = ctx or problems[0].ctx
    dev = problems[0].device
    pbs = (C.POINTER(_lib.BAProblem) * n)()
    cams_p, pts_p, ws_p = (C.c_void_p * n)(), (C.c_void_p * n)(), (C.c_void_p * n)()
    ws_b = (C.c_size_t * n)()
    keep = []
    for k, (pb, cm, pt) in enumerate(zip(problems, cams_list, pts_list)):
        for t in (cm, pt):
            assert t.dtype == torch.float64 and t.is_contiguous() and t.device == dev
        assert pb.device == dev
        need = lib.mm_ba_trf_batched_workspace_bytes(C.byref(pb.pb))
        if getattr(pb, "_trf_ws", None) is None or pb._trf_ws.numel() < need:
            pb._trf_ws = torch.empty(need, dtype=torch.uint8, device=dev)
        pbs[k] = C.pointer(pb.pb)
        cams_p[k], pts_p[k], ws_p[k], ws_b[k] = cm.data_ptr(), pt.data_ptr(), pb._trf_ws.data_ptr(), pb._trf_ws.numel()
        keep.append(pb._trf_ws)
    prm = _lib.TrfParams(ftol, xtol, gtol, min_damping, int(max_nfev) if max_nfev else 0)
    reps = (_lib.TrfReport * n)()
    alone = (C.c_int32 * n)()
    rc = lib.mm_ba_trf_batched(ctx.h, n, pbs, cams_p, pts_p, C.byref(prm), reps, ws_p, ws_b, alone)
    if rc and any(r.status == -2 for r in reps):
        raise ValueError("Residuals are not finite in the initial point.")
    ctx.check(rc, "mm_ba_trf_batched")
    return list(reps), [bool(a) for a in alone]


OBS_REPROJ, OBS_BEHIND, OBS_NONFINITE, OBS_ORPHAN = 1, 2, 4, 8      # MM_OBS_* of include/meatmodeler.h
PT_SHORT, PT_PARALLAX, PT_NONFINITE = 1, 2, 4                        # MM_PT_*
FILTER_CHUNK = 1024                                                  # MM_FILTER_CHUNK: rows per chunk of the compaction's scans


def filter_thresholds(max_reproj_px=math.inf, min_angle_deg=0, min_depth=-math.inf, min_views=2, what="filter_observations"):
    """The thresholds of filter_observations as mm_filter_params; a NaN, a negative angle, min_views < 2 or no active test at
    all (every threshold at its off value and min_views = 2) raises ValueError."""
    try:
        tau, ang, dep, mv = float(max_reproj_px), float(min_angle_deg), float(min_depth), int(min_views)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: max_reproj_px, min_angle_deg and min_depth must be numbers and min_views an integer") from None
    if math.isnan(tau) or math.isnan(dep) or not ang >= 0 or not ang <= 180:
        raise ValueError(f"{what}: thresholds must be numbers and min_angle_deg in 0 .. 180")
    if mv < 2 or mv != min_views:
        raise ValueError(f"{what}: min_views must be an integer of at least 2")
    if tau == math.inf and ang == 0 and dep == -math.inf and mv == 2:
        raise ValueError(f"{what}: no active test (give max_reproj_px, min_angle_deg, min_depth or min_views > 2)")
    return _lib.FilterParams(mv, 0, tau, dep, math.cos(math.radians(ang)) if ang > 0 else 2.0)


def filter_observations(cams, pts, K, fi, pi=None, obs=None, pt_ptr=None, max_reproj_px=math.inf, min_angle_deg=0,
                        min_depth=-math.inf, min_views=2, ctx=None):
    """Observations and points judged at an adjusted solution and the problem compacted (mm_filter_observations): cams [F, 6]
    f64 (one row for every value fi takes: fixed cameras behind the free ones), pts [P, 3] f64, K 3 x 3 on the host, fi / pi [O]
    i32 and obs [O, 2] f64 point-major (what flatten_tracks emits), optional pt_ptr [P+1] i32 -- device tensors; or a BADevice
    in place of fi, which supplies the four of them.
    An observation is flagged when its reprojection error exceeds max_reproj_px, its depth is <= min_depth or either is not
    finite; a point when fewer than min_views observations survive, its parallax over the survivors is below min_angle_deg
    (0: test off) or it is not finite; an unflagged observation of a flagged point is an orphan.
    -> dict(fi [O'], pi [O'] (renumbered), obs [O', 2], obs_map [O'], point_map [P'] -- views of worst-case buffers, sized after
    one host read of the counts --, n_obs, n_points, removed_obs (flagged by a test of their own), removed_points, obs_flags [O]
    of OBS_* bits, pt_flags [P] of PT_* bits, err [O], depth [O], cos_parallax [P]).
    Bad shapes or dtypes, indices out of range, observations that are not point-major and a call without an active test raise
    ValueError before the library is called."""
    name = "filter_observations"
    prm = filter_thresholds(max_reproj_px, min_angle_deg, min_depth, min_views, name)
    Kh = _host_f64(K, 9, f"{name}: K")
    if not np.isfinite(Kh).all() or Kh[3] != 0 or Kh[6] != 0 or Kh[7] != 0 or Kh[8] != 1 or Kh[0] == 0 or Kh[4] == 0:
        raise ValueError(f"{name}: K must be finite, upper triangular with K[2, 2] = 1 and non-zero focal lengths")
    checked = isinstance(fi, BADevice)      # (its ranges and point-major order were judged by mm_ba_index_build)
    if checked:
        pb = fi
        if pi is not None or obs is not None or pt_ptr is not None:
            raise ValueError(f"{name}: a BADevice supplies fi, pi, obs and pt_ptr")
        fi, pi, obs, pt_ptr = pb.fi, pb.pi, pb.obs, pb.pt_ptr
        if not pb.point_major:
            raise ValueError(f"{name}: the observations are not point-major")
        ctx = ctx or pb.ctx
    for what, t, dtype, tail in (("cams [F, 6] f64", cams, torch.float64, (6,)), ("pts [P, 3] f64", pts, torch.float64, (3,)),
                                 ("fi [O] i32", fi, torch.int32, ()), ("pi [O] i32", pi, torch.int32, ()),
                                 ("obs [O, 2] f64", obs, torch.float64, (2,))):
        if not torch.is_tensor(t) or t.dtype != dtype or t.dim() != 1 + len(tail) or tuple(t.shape[1:]) != tail:
            raise ValueError(f"{name}: {what} expected")
    F, P, O = cams.shape[0], pts.shape[0], fi.shape[0]
    if checked and (F != pb.F + pb.F_fixed or P != pb.P):
        raise ValueError(f"{name}: cams must have a row per camera of the BADevice (fixed ones included) and pts a row per point")
    if pi.shape[0] != O or obs.shape[0] != O:
        raise ValueError(f"{name}: fi, pi and obs must have one row per observation")
    if O > 2 ** 31 - 1 or P >= 2 ** 31 - 1:
        raise ValueError(f"{name}: more than 2^31 - 1 rows")
    d = pts.device
    if any(t.device != d for t in (cams, fi, pi, obs)) or (pt_ptr is not None and (not torch.is_tensor(pt_ptr) or pt_ptr.device != d)):
        raise ValueError(f"{name}: every tensor must live on one device")
    if pt_ptr is not None and (pt_ptr.dtype != torch.int32 or tuple(pt_ptr.shape) != (P + 1,)):
        raise ValueError(f"{name}: pt_ptr [P+1] i32 expected")
    if O and P and not checked:
        lim = [fi.min(), fi.max(), pi.min(), pi.max(), (pi[1:] >= pi[:-1]).all()]
        if pt_ptr is not None:
            lim += [pt_ptr[0], pt_ptr[-1], (pt_ptr[1:] >= pt_ptr[:-1]).all()]
        lim = torch.stack([v.long() for v in lim]).tolist()      # (one read-back)
        if lim[0] < 0 or lim[1] >= F or lim[2] < 0 or lim[3] >= P:
            raise ValueError(f"{name}: frame / point index out of range")
        if not lim[4]:
            raise ValueError(f"{name}: the observations are not point-major")
        if pt_ptr is not None and (lim[5] != 0 or lim[6] != O or not lim[7]):
            raise ValueError(f"{name}: pt_ptr is not a CSR over the observations")
    elif O and not P:
        raise ValueError(f"{name}: observations without points")
    if pt_ptr is None:
        pt_ptr = torch.searchsorted(pi, torch.arange(P + 1, dtype=torch.int32, device=d)).to(torch.int32)
    ctx = ctx or default_context()
    cams, pts, fi, pi, obs, pt_ptr = (t.contiguous() for t in (cams, pts, fi, pi, obs, pt_ptr))
    i32, f64 = dict(dtype=torch.int32, device=d), dict(dtype=torch.float64, device=d)
    obs_flags, err, depth = torch.zeros(O, **i32), torch.full((O,), math.nan, **f64), torch.full((O,), math.nan, **f64)
    # (a call without observations launches nothing per row: every point is then short, as step 2 would find it)
    pt_flags = torch.zeros(P, **i32) if O else torch.full((P,), PT_SHORT, **i32)
    cosp = torch.full((P,), math.nan, **f64)
    fi_out, pi_out, obs_map = torch.empty(O, **i32), torch.empty(O, **i32), torch.empty(O, **i32)
    obs_out, point_map = torch.empty((O, 2), **f64), torch.empty(P, **i32)
    counts = torch.zeros(4, dtype=torch.int64, device=d)
    wsb = lib.mm_filter_workspace_bytes(F, P, O)
    ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device=d)
    ctx.check(lib.mm_filter_observations(ctx.h, ptr(cams), F, ptr(pts), P, Kh.ctypes.data_as(_lib.c_f64p), ptr(fi), ptr(pi), ptr(obs),
                                         O, ptr(pt_ptr), C.byref(prm), ptr(obs_flags), ptr(err), ptr(depth), ptr(pt_flags), ptr(cosp),
                                         ptr(fi_out), ptr(pi_out), ptr(obs_out), ptr(obs_map), ptr(point_map), ptr(counts), ptr(ws),
                                         ws.numel()), "mm_filter_observations")
    n_obs, n_points, own, flagged = counts.tolist()      # (the one host read: it sizes the views)
    flagged = flagged if O else P
    return dict(fi=fi_out[:n_obs], pi=pi_out[:n_obs], obs=obs_out[:n_obs], obs_map=obs_map[:n_obs], point_map=point_map[:n_points],
                n_obs=n_obs, n_points=n_points, removed_obs=own, removed_points=flagged, obs_flags=obs_flags, pt_flags=pt_flags,
                err=err, depth=depth, cos_parallax=cosp)


SWEEP_TILE = 16                                         # MM_SWEEP_TILE: side of the tile of pixels one workgroup of the sweep owns
SWEEP_MAX_RADIUS, SWEEP_MAX_PLANES, SWEEP_MAX_SOURCES, FUSE_MAX_NEIGHBOURS = 4, 4096, 16, 64      # MM_SWEEP_MAX_*, MM_FUSE_MAX_*


def _dense_K(K, name):
    Kh = _host_f64(K, 9, f"{name}: K")
    if not np.isfinite(Kh).all() or Kh[3] != 0 or Kh[6] != 0 or Kh[7] != 0 or Kh[8] != 1 or Kh[0] == 0 or Kh[4] == 0:
        raise ValueError(f"{name}: K must be finite, upper triangular with K[2, 2] = 1 and non-zero focal lengths")
    return Kh


def _dense_ext(ext, name):
    e = np.asarray(ext, np.float64)
    if e.ndim != 3 or e.shape[1] not in (3, 4) or e.shape[2] != 4:
        raise ValueError(f"{name}: extrinsics [n, 3|4, 4] expected")
    return np.ascontiguousarray(e[:, :3, :])


def sweep_tables(K, extrinsics, ref, src, ranges, planes):
    """The host tables of depth_sweep, NumPy f64 with every product written out as include/meatmodeler.h states it (no BLAS, so
    the bits do not depend on the library NumPy was built with): K 3 x 3, extrinsics [F, 3|4, 4], ref [V] and src [V, S] frame
    indices (-1: no source; its row of AB is zero), ranges [V, 2] = (dmin, dmax) per view, planes = D
    -> (AB [V, S, 12] = (A row-major, b), w0 [V], dw [V])."""
    name = "sweep_tables"
    Kh = _dense_K(K, name)
    E = _dense_ext(extrinsics, name)
    ref, src = np.asarray(ref, np.int64).reshape(-1), np.asarray(src, np.int64)
    rng = np.asarray(ranges, np.float64)
    V = ref.size
    if src.ndim != 2 or src.shape[0] != V or rng.shape != (V, 2):
        raise ValueError(f"{name}: ref [V], src [V, S] and ranges [V, 2] expected")
    if V and (ref.min() < 0 or ref.max() >= len(E) or src.min() < -1 or src.max() >= len(E)):
        raise ValueError(f"{name}: frame index out of range")
    if not (np.isfinite(rng).all() and (rng[:, 0] > 0).all() and (rng[:, 1] >= rng[:, 0]).all()):
        raise ValueError(f"{name}: 0 < dmin <= dmax expected")
    D = int(planes)
    if D < 1:
        raise ValueError(f"{name}: planes must be at least 1")
    S = src.shape[1]
    Er = E[ref][:, None]                                         # [V, 1, 3, 4]
    Es = E[np.where(src < 0, 0, src)]                            # [V, S, 3, 4]
    Rr, tr, Rs, ts = Er[..., :3], Er[..., 3], Es[..., :3], Es[..., 3]
    R = np.empty((V, S, 3, 3))
    for i in range(3):
        for j in range(3):
            R[..., i, j] = (Rs[..., i, 0] * Rr[..., j, 0] + Rs[..., i, 1] * Rr[..., j, 1]) + Rs[..., i, 2] * Rr[..., j, 2]
    t = np.empty((V, S, 3))
    for i in range(3):
        t[..., i] = ts[..., i] - ((R[..., i, 0] * tr[..., 0] + R[..., i, 1] * tr[..., 1]) + R[..., i, 2] * tr[..., 2])
    fx, sk, cx, fy, cy = Kh[0], Kh[1], Kh[2], Kh[4], Kh[5]
    AB = np.empty((V, S, 12))
    for i in range(3):
        M = [(Kh[3 * i] * R[..., 0, j] + Kh[3 * i + 1] * R[..., 1, j]) + Kh[3 * i + 2] * R[..., 2, j] for j in range(3)]
        a0 = M[0] / fx
        a1 = (M[1] - sk * a0) / fy
        AB[..., 3 * i], AB[..., 3 * i + 1], AB[..., 3 * i + 2] = a0, a1, (M[2] - cx * a0) - cy * a1
        AB[..., 9 + i] = (Kh[3 * i] * t[..., 0] + Kh[3 * i + 1] * t[..., 1]) + Kh[3 * i + 2] * t[..., 2]
    AB[src < 0] = 0.0
    w0 = 1.0 / rng[:, 0]
    dw = (1.0 / rng[:, 1] - 1.0 / rng[:, 0]) / float(D - 1) if D > 1 else np.zeros(V)
    return AB, w0, dw


def depth_sweep(img, K, extrinsics, ref, src, ranges, planes=64, radius=3, var_min=4.0, min_sources=1, ctx=None):
    """A plane-sweep depth map per reference view (mm_depth_sweep): img [F, H, W] u8 on the device; K 3 x 3, extrinsics
    [F, 3|4, 4], ref [V] (the frame of each view), src [V, S] (its source frames, -1: none) and ranges [V, 2] = (dmin, dmax) on
    the host.  Every pixel with a (2 radius + 1)^2 window is scored on `planes` planes, evenly spaced in inverse depth, by
    zero-mean normalised cross-correlation against every source that sees the whole window and is textured there (variance
    above var_min in both images), the mean over at least min_sources of them; the lowest cost wins and is refined between its
    neighbouring planes.  -> dict(depth, cost [V, H, W] f32, NaN where there is none; plane [V, H, W] i32, -1 there; AB, w0, dw:
    the host tables of `sweep_tables`).  Bad shapes, dtypes, indices or parameters raise ValueError before the library is
    called."""
    name = "depth_sweep"
    if not torch.is_tensor(img) or img.dtype != torch.uint8 or img.dim() != 3:
        raise ValueError(f"{name}: img [F, H, W] u8 expected")
    F, H, W = img.shape
    try:
        D, r, ms, vm = int(planes), int(radius), int(min_sources), float(var_min)
    except (TypeError, ValueError):
        raise ValueError(f"{name}: planes, radius and min_sources must be integers and var_min a number") from None
    if D != planes or r != radius or ms != min_sources:
        raise ValueError(f"{name}: planes, radius and min_sources must be integers")
    E = _dense_ext(extrinsics, name)
    if len(E) != F:
        raise ValueError(f"{name}: one extrinsic per frame of img expected")
    src_h = np.asarray(src, np.int64)
    S = src_h.shape[1] if src_h.ndim == 2 else 0
    if not 1 <= D <= SWEEP_MAX_PLANES or not 1 <= r <= SWEEP_MAX_RADIUS or not 1 <= S <= SWEEP_MAX_SOURCES or not 1 <= ms <= S:
        raise ValueError(f"{name}: planes in 1 .. {SWEEP_MAX_PLANES}, radius in 1 .. {SWEEP_MAX_RADIUS}, 1 .. {SWEEP_MAX_SOURCES} "
                         "sources and min_sources in 1 .. S expected")
    if not (vm >= 0 and math.isfinite(vm)):
        raise ValueError(f"{name}: var_min must be finite and >= 0")
    AB, w0, dw = sweep_tables(K, E, ref, src_h, ranges, D)
    Kh = _dense_K(K, name)
    V = w0.size
    if F == 0 or H == 0 or W == 0 or max(F, V) * H * W > 2 ** 31 - 1 or V > 65535:
        raise ValueError(f"{name}: an empty image, more than 2^31 - 1 pixels or more than 65535 views")
    d = img.device
    ctx = ctx or default_context()
    f32 = dict(dtype=torch.float32, device=d)
    depth, cost = torch.empty((V, H, W), **f32), torch.empty((V, H, W), **f32)
    plane = torch.empty((V, H, W), dtype=torch.int32, device=d)
    out = dict(depth=depth, cost=cost, plane=plane, AB=AB, w0=w0, dw=dw)
    if V == 0:
        return out
    up = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dt)).to(d)
    ref_d, src_d = up(np.asarray(ref).reshape(-1), np.int32), up(src_h, np.int32)
    AB_d, w0_d, dw_d = up(AB, np.float64), up(w0, np.float64), up(dw, np.float64)
    prm = _lib.SweepParams(D, r, ms, 0, vm)
    ws = torch.empty(max(lib.mm_depth_sweep_workspace_bytes(V, S, D), 256), dtype=torch.uint8, device=d)
    img = img.contiguous()
    ctx.check(lib.mm_depth_sweep(ctx.h, ptr(img), F, H, W, Kh.ctypes.data_as(_lib.c_f64p), ptr(ref_d), ptr(src_d), ptr(AB_d), ptr(w0_d),
                                 ptr(dw_d), V, S, C.byref(prm), ptr(depth), ptr(cost), ptr(plane), ptr(ws), ws.numel()), "mm_depth_sweep")
    return out


def depth_fuse(depth, cost, K, extrinsics, nbr, grey, max_cost=0.4, eps_depth=0.01, tau_px=1.0, min_consistent=2, cap=None, ctx=None):
    """The depth maps of V views checked against each other and the consistent pixels compacted into a cloud (mm_depth_fuse):
    depth, cost [V, H, W] f32 as depth_sweep returns them and grey [V, H, W] u8, the views' images, on the device; K 3 x 3,
    extrinsics [V, 3|4, 4] (the views' own) and nbr [V, Q] (per view the other views it is checked against, -1: none) on the
    host.  A pixel with a finite depth and cost <= max_cost is a candidate; a neighbour agrees when the pixel's point falls on a
    candidate of it whose depth is within eps_depth (relative) and whose own point comes back within tau_px; a candidate at
    least min_consistent neighbours agree with is kept.  cap: rows of the outputs (default: every pixel).
    -> dict(points [n, 3] f64, grey [n] u8, origin [n, 2] i32 = (view, v W + u), n_consistent [n] i32 -- views of the buffers,
    sized after one host read of the counts, in (view, row, column) order --, keep [V, H, W] u8, counts = (kept, candidates), n =
    min(kept, cap)).  A surface point that several views keep appears once per view: duplicates are not merged."""
    name = "depth_fuse"
    for what, t, dt in (("depth [V, H, W] f32", depth, torch.float32), ("cost [V, H, W] f32", cost, torch.float32),
                        ("grey [V, H, W] u8", grey, torch.uint8)):
        if not torch.is_tensor(t) or t.dtype != dt or t.dim() != 3 or t.shape != depth.shape or t.device != depth.device:
            raise ValueError(f"{name}: {what} expected, all of one shape on one device")
    V, H, W = depth.shape
    Kh = _dense_K(K, name)
    E = _dense_ext(extrinsics, name)
    nb = np.asarray(nbr, np.int64)
    if len(E) != V or nb.ndim != 2 or nb.shape[0] != V or nb.shape[1] > FUSE_MAX_NEIGHBOURS:
        raise ValueError(f"{name}: one extrinsic per view and nbr [V, Q <= {FUSE_MAX_NEIGHBOURS}] expected")
    Q = nb.shape[1]
    if nb.size and (nb.min() < -1 or nb.max() >= V or (nb == np.arange(V)[:, None]).any()):
        raise ValueError(f"{name}: nbr must name other views of this call (or -1)")
    try:
        mc, ed, tp, mk = float(max_cost), float(eps_depth), float(tau_px), int(min_consistent)
    except (TypeError, ValueError):
        raise ValueError(f"{name}: max_cost, eps_depth and tau_px must be numbers and min_consistent an integer") from None
    if math.isnan(mc) or not ed >= 0 or not tp >= 0 or mk < 0 or mk != min_consistent:
        raise ValueError(f"{name}: max_cost must be a number, eps_depth and tau_px >= 0 and min_consistent an integer >= 0")
    N = V * H * W
    if H == 0 or W == 0 or N > 2 ** 31 - 1:
        raise ValueError(f"{name}: an empty image or more than 2^31 - 1 pixels")
    cap = N if cap is None else int(cap)
    if cap < 0:
        raise ValueError(f"{name}: cap must not be negative")
    d = depth.device
    ctx = ctx or default_context()
    rows = max(min(cap, N), 1)
    points = torch.empty((rows, 3), dtype=torch.float64, device=d)
    grey_out = torch.empty(rows, dtype=torch.uint8, device=d)
    origin = torch.empty((rows, 2), dtype=torch.int32, device=d)
    n_cons = torch.empty(rows, dtype=torch.int32, device=d)
    keep = torch.zeros((V, H, W), dtype=torch.uint8, device=d)
    counts = torch.zeros(2, dtype=torch.int64, device=d)
    up = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dt)).to(d)
    ext_d, nbr_d = up(E, np.float64), up(nb if Q else np.zeros((max(V, 1), 1)), np.int32)
    prm = _lib.FuseParams(mk, 0, mc, ed, tp)
    ws = torch.empty(max(lib.mm_depth_fuse_workspace_bytes(V, H, W), 256), dtype=torch.uint8, device=d)
    depth, cost, grey = depth.contiguous(), cost.contiguous(), grey.contiguous()
    ctx.check(lib.mm_depth_fuse(ctx.h, ptr(depth), ptr(cost), V, H, W, ptr(ext_d), Kh.ctypes.data_as(_lib.c_f64p), ptr(nbr_d), Q, ptr(grey),
                                C.byref(prm), min(cap, N), ptr(points), ptr(grey_out), ptr(origin), ptr(n_cons), ptr(keep), ptr(counts),
                                ptr(ws), ws.numel()), "mm_depth_fuse")
    kept, cand = counts.tolist()      # (the one host read: it sizes the views)
    n = min(kept, cap)
    return dict(points=points[:n], grey=grey_out[:n], origin=origin[:n], n_consistent=n_cons[:n], keep=keep, counts=(kept, cand), n=n)


class MultiDot:
    """[<a, b> for (a, b) in pairs] in one launch (mm_multi_dot): returns a device tensor [k, 3] =
    (sum over i < split, sum over i >= split, total).  Holds the zero-initialised workspace."""

    def __init__(self, device, ctx=None):
        self.ctx = ctx or default_context()
        self.ws = torch.zeros(lib.mm_multi_dot_workspace_bytes(), dtype=torch.uint8, device=device)

    def __call__(self, pairs, split=0):
        out_all = []
        for i0 in range(0, len(pairs), 8):
            chunk = pairs[i0:i0 + 8]
            k = len(chunk)
            n = chunk[0][0].numel()
            if n == 0:      # (empty tensors have no storage to point at)
                out_all.append(torch.zeros((k, 3), dtype=torch.float64, device=self.ws.device))
                continue
            for a, b in chunk:
                assert a.dtype == torch.float64 and b.dtype == torch.float64 and a.is_contiguous() and b.is_contiguous()
                assert a.numel() == n and b.numel() == n
            pa = (C.c_void_p * k)(*[a.data_ptr() for a, _ in chunk])
            pb_ = (C.c_void_p * k)(*[b.data_ptr() for _, b in chunk])
            out = torch.empty((k, 3), dtype=torch.float64, device=self.ws.device)
            self.ctx.check(lib.mm_multi_dot(self.ctx.h, k, pa, pb_, n, int(split), ptr(out), ptr(self.ws), self.ws.numel()),
                           "mm_multi_dot")
            out_all.append(out)
        return out_all[0] if len(out_all) == 1 else torch.cat(out_all)


def trf_damping(gh2, d11, Delta, min_damping, ctx=None):
    """Device scalars |g_h|^2 and |J_h g_h|^2 -> tensor [reg, max(reg, min_damping)] (mm_trf_damping)."""
    ctx = ctx or default_context()
    out = torch.empty(2, dtype=torch.float64, device=gh2.device)
    ctx.check(lib.mm_trf_damping(ctx.h, ptr(gh2), ptr(d11), float(Delta), float(min_damping), ptr(out)), "mm_trf_damping")
    return out


def chol_solve(A, b, ctx=None, half_bandwidth=None):
    """In place: A [n,n] f64 SPD (lower triangle used, overwritten by L), b [n] or [nrhs,n] overwritten by x.
    half_bandwidth: A[i][j] == 0 for i - j > half_bandwidth (None = dense).  Returns the device int32 info (0 = ok)."""
    ctx = ctx or default_context()
    n = A.shape[0]
    assert A.dtype == torch.float64 and A.is_contiguous() and b.is_contiguous() and b.shape[-1] == n
    nrhs = 1 if b.dim() == 1 else b.shape[0]
    info = torch.zeros(1, dtype=torch.int32, device=A.device)
    wsb = lib.mm_chol_workspace_bytes(n)
    ws = torch.empty(wsb, dtype=torch.uint8, device=A.device)
    hb = n if half_bandwidth is None else int(min(half_bandwidth, n))
    ctx.check(lib.mm_chol_solve(ctx.h, ptr(A), n, ptr(b), nrhs, hb, ptr(info), ptr(ws), wsb), "mm_chol_solve")
    return info


def chol_solve_sym(A, b, ctx=None, half_bandwidth=None, both_triangles=True):
    """In place, solution only: A [n,n] f64 SPD is destroyed, b [n] overwritten by x (mm_chol_solve_sym).
    both_triangles: both triangles of the band hold A (else only the lower one).  Returns the device int32 info."""
    ctx = ctx or default_context()
    n = A.shape[0]
    assert A.dtype == torch.float64 and A.is_contiguous() and b.is_contiguous() and b.dim() == 1 and b.shape[0] == n
    info = torch.zeros(1, dtype=torch.int32, device=A.device)
    wsb = lib.mm_chol_workspace_bytes(n)
    ws = torch.empty(wsb, dtype=torch.uint8, device=A.device)
    hb = n if half_bandwidth is None else int(min(half_bandwidth, n))
    ctx.check(lib.mm_chol_solve_sym(ctx.h, ptr(A), n, ptr(b), hb, 1 if both_triangles else 0, ptr(info), ptr(ws), wsb),
              "mm_chol_solve_sym")
    return info


# ------------------------------------------------------------------------------------------------ keyframe gating front end

def pyramid(img, max_level, ctx=None):
    """[H,W] u8 device tensor -> list of max_level + 1 device tensors (mm_pyr_down; level 0 is `img` itself)."""
    ctx = ctx or default_context()
    assert img.dtype == torch.uint8 and img.dim() == 2 and img.is_contiguous()
    levels = [img]
    for _ in range(int(max_level)):
        s = levels[-1]
        h, w = s.shape
        d = torch.empty(((h + 1) // 2, (w + 1) // 2), dtype=torch.uint8, device=s.device)
        ctx.check(lib.mm_pyr_down(ctx.h, ptr(s), w, h, s.stride(0), ptr(d), d.stride(0)), "mm_pyr_down")
        levels.append(d)
    return levels


def lk_track(prev_levels, next_levels, pts, win=(21, 21), max_count=30, epsilon=0.01, ctx=None):
    """Pyramidal Lucas-Kanade (mm_lk_track) on two pyramids from `pyramid`.  pts [n,2] f32 device.
    -> next [n,2] f32, status [n] u8, err [n] f32 (device)."""
    ctx = ctx or default_context()
    L = len(prev_levels)
    assert len(next_levels) == L and pts.dtype == torch.float32 and pts.is_contiguous() and pts.shape[-1] == 2
    n = pts.shape[0]
    d = pts.device
    out = torch.empty((n, 2), dtype=torch.float32, device=d)
    st = torch.empty(n, dtype=torch.uint8, device=d)
    err = torch.empty(n, dtype=torch.float32, device=d)
    if n == 0:
        return out, st, err
    arr_p = (C.c_void_p * L)(*[t.data_ptr() for t in prev_levels])
    arr_n = (C.c_void_p * L)(*[t.data_ptr() for t in next_levels])
    ws = (C.c_int * L)(*[t.shape[1] for t in prev_levels])
    hs = (C.c_int * L)(*[t.shape[0] for t in prev_levels])
    ps = (C.c_int * L)(*[t.stride(0) for t in prev_levels])
    for a, b in zip(prev_levels, next_levels):
        assert a.shape == b.shape and a.stride(0) == b.stride(0)
    eps = min(max(float(epsilon), 0.0), 10.0) ** 2
    ctx.check(lib.mm_lk_track(ctx.h, arr_p, arr_n, ws, hs, ps, L, ptr(pts), n, int(win[0]), int(win[1]),
                              min(max(int(max_count), 0), 100), eps, ptr(out), ptr(st), ptr(err)), "mm_lk_track")
    return out, st, err


def min_eig(img, block_size=3, ctx=None):
    """Shi-Tomasi minimum-eigenvalue map [H,W] f64 (mm_min_eig)."""
    ctx = ctx or default_context()
    assert img.dtype == torch.uint8 and img.dim() == 2 and img.stride(1) == 1
    h, w = img.shape
    eig = torch.empty((h, w), dtype=torch.float64, device=img.device)
    ctx.check(lib.mm_min_eig(ctx.h, ptr(img), w, h, img.stride(0), int(block_size), ptr(eig)), "mm_min_eig")
    return eig


def good_features(img, max_corners, quality, min_distance, block_size=3, ctx=None):
    """cv2.goodFeaturesToTrack on a device image: eigenvalue map, threshold + non-maximum suppression and compaction on
    the device, ordering by torch.sort (index plumbing), greedy minimum-distance selection on the host
    (mm_gftt_select).  -> numpy [n,2] f32 (x, y)."""
    ctx = ctx or default_context()
    h, w = img.shape
    if h < 3 or w < 3:                            # no interior pixel: no corner (the 3x3 suppression needs a neighbourhood)
        return np.zeros((0, 2), np.float32)
    eig = min_eig(img, block_size, ctx)
    cap = h * w                                  # (a plateau of equal values keeps every one of its pixels)
    d = img.device
    mx = torch.zeros(1, dtype=torch.int64, device=d)
    vb = torch.empty(cap, dtype=torch.int64, device=d)
    pos = torch.empty(cap, dtype=torch.int32, device=d)
    cnt = torch.zeros(1, dtype=torch.int32, device=d)
    ctx.check(lib.mm_corner_candidates(ctx.h, ptr(eig), w, h, float(quality), ptr(mx), ptr(vb), ptr(pos), cap, ptr(cnt)),
              "mm_corner_candidates")
    n = min(int(cnt.item()), cap)
    if n == 0:
        return np.zeros((0, 2), np.float32)
    pos_s, o1 = torch.sort(pos[:n], stable=True)                       # by position ...
    _, o2 = torch.sort(vb[:n][o1], descending=True, stable=True)       # ... then stably by strength (descending)
    pos_h = np.ascontiguousarray(pos_s[o2].cpu().numpy(), np.int32)
    out_cap = int(max_corners) if max_corners and max_corners > 0 else n
    out = np.zeros((max(out_cap, 1), 2), np.float32)
    m = lib.mm_gftt_select(pos_h.ctypes.data_as(C.c_void_p), n, w, h, int(max_corners or 0), float(min_distance),
                           out.ctypes.data_as(C.c_void_p), out_cap)
    if m < 0:
        raise _lib.MMError(f"mm_gftt_select failed ({m})")
    return out[:m]


_LAB_TABLES = {}


def increase_contrast(bgr, clip_limit=3.5, tiles=(8, 8), want_grey=False, ctx=None):
    """bgr [B,H,W,3] u8 device -> contrast-enhanced BGR (and the grey image of the result): mm_increase_contrast."""
    ctx = ctx or default_context()
    assert bgr.dtype == torch.uint8 and bgr.dim() == 4 and bgr.shape[-1] == 3 and bgr.is_contiguous()
    B, H, W, _ = bgr.shape
    d = bgr.device
    key = str(d)
    if key not in _LAB_TABLES:
        from .frame_tables import lab_tables
        _LAB_TABLES[key] = tuple(torch.as_tensor(t.view(np.int16) if t.dtype == np.uint16 else t).to(d) for t in lab_tables())
    g, cb, gi = _LAB_TABLES[key]
    out = torch.empty_like(bgr)
    grey = torch.empty((B, H, W), dtype=torch.uint8, device=d) if want_grey else None
    wsb = lib.mm_contrast_workspace_bytes(B, W, H, int(tiles[0]), int(tiles[1]))
    ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device=d)
    ctx.check(lib.mm_increase_contrast(ctx.h, ptr(bgr), B, W, H, ptr(g), ptr(cb), ptr(gi), float(clip_limit), int(tiles[0]),
                                       int(tiles[1]), ptr(out), ptr(grey), ptr(ws), ws.numel()), "mm_increase_contrast")
    return (out, grey) if want_grey else out


def bgr_to_grey(bgr, ctx=None):
    """[...,3] u8 device -> [...] u8: cv2.COLOR_BGR2GRAY's fixed-point weights (mm_bgr_to_grey)."""
    ctx = ctx or default_context()
    assert bgr.dtype == torch.uint8 and bgr.shape[-1] == 3 and bgr.is_contiguous()
    grey = torch.empty(bgr.shape[:-1], dtype=torch.uint8, device=bgr.device)
    ctx.check(lib.mm_bgr_to_grey(ctx.h, ptr(bgr), grey.numel(), ptr(grey)), "mm_bgr_to_grey")
    return grey
