"""CPU ORACLE (test infrastructure only) — NumPy/SciPy restatement of the reference's
bundle-adjustment, triangulation and track-bookkeeping path.

    *** This module is the CHECKER.  Only tests/, __graft_entry__.smoke() and bench.py's
    *** cpu_baseline leg may import it.  Nothing under meatmodeler_amd/ may.

Pinned against golden vectors G1-G8 (tests/golden/, captured by importing the reference's own
NumPy/SciPy code in the build container: tests/golden/make_golden.py) by tests/test_oracle_golden.py.
`triangulate_dlt` restates OpenCV's cv2.triangulatePoints (opencv-python~=4.5.2.54, absent offline,
no reference fixture) from its published algorithm: **parity unpinned** for that function.

Each function cites the reference lines it follows (paths relative to /root/reference).
"""
import math

import numpy as np
from scipy.optimize import least_squares
from scipy.sparse import csr_matrix


# ------------------------------------------------------------------ cost model (bundleAdjuster.py)

def rotate(points, rvecs):
    """Rodrigues rotation of points[n,3] by axis-angle rvecs[n,3] (bundleAdjuster.py:7-28).

    theta = |r|; unit axis k = r/theta with 0/0 -> 0 (the reference's nan_to_num), so theta == 0
    leaves the point unchanged.  X' = cos X + sin (k x X) + (1-cos)(k.X) k.
    """
    points = np.asarray(points, float)
    rvecs = np.asarray(rvecs, float)
    theta = np.sqrt((rvecs * rvecs).sum(axis=1, keepdims=True))
    safe = np.where(theta == 0.0, 1.0, theta)
    k = np.where(theta == 0.0, 0.0, rvecs / safe)
    c, s = np.cos(theta), np.sin(theta)
    kdotx = (k * points).sum(axis=1, keepdims=True)
    kxx = np.stack([k[:, 1] * points[:, 2] - k[:, 2] * points[:, 1],
                    k[:, 2] * points[:, 0] - k[:, 0] * points[:, 2],
                    k[:, 0] * points[:, 1] - k[:, 1] * points[:, 0]], axis=1)
    return c * points + s * kxx + kdotx * (1.0 - c) * k


def project(points, frame_params, K):
    """points[n,3], frame_params[n,6]=(r,t), full 3x3 K -> pixels[n,2] (bundleAdjuster.py:31-52)."""
    Xc = rotate(points, frame_params[:, :3]) + frame_params[:, 3:6]
    u = Xc @ np.asarray(K, float).T            # einsum("ij,...j") of the reference, :47
    return u[:, :2] / u[:, 2:3]


def point_fun(x, K, n_frames, n_points, fi, pi, obs):
    """Residual vector [2*O], interleaved x,y (bundleAdjuster.py:81-102).
    x = [cam0(r,t) .. cam_{F-1}, pt0 .. pt_{P-1}] (:96-97)."""
    cams = x[:6 * n_frames].reshape(n_frames, 6)
    pts = x[6 * n_frames:].reshape(n_points, 3)
    return (project(pts[pi], cams[fi], K) - obs).ravel()


def pose_fun(x, K, n_frames, fi, pi, pts3, obs):
    """Pose-only residuals, points fixed (bundleAdjuster.py:206-211)."""
    cams = x.reshape(n_frames, 6)
    return (project(pts3[pi], cams[fi], K) - obs).ravel()


def frame_parameters(ext):
    """[F,3|4,4] extrinsics -> [6F] (r,t) rows (bundleAdjuster.py:105-134).

    theta = arccos((tr R - 1)/2) with NO clipping (:117-119); axis from the skew part over
    2 sin(theta) (:124-126); 0/0 -> 0 via nan_to_num (:131); r = axis * theta.
    """
    ext = np.asarray(ext, float)
    R = ext[:, :3, :3]
    with np.errstate(invalid="ignore", divide="ignore"):
        theta = np.arccos((R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2] - 1.0) / 2.0)
        den = 2.0 * np.sin(theta)
        axis = np.stack([(R[:, 2, 1] - R[:, 1, 2]) / den,
                         (R[:, 0, 2] - R[:, 2, 0]) / den,
                         (R[:, 1, 0] - R[:, 0, 1]) / den], axis=1)
        rv = np.nan_to_num(axis) * theta[:, None]
    return np.hstack([rv, ext[:, :3, 3]]).reshape(-1)


def sparsity_pattern(n_frames, n_points, fi, pi):
    """CSR pattern of the Jacobian: rows 2i,2i+1 carry the 6 camera + 3 point columns
    (bundleAdjuster.py:55-78)."""
    fi = np.asarray(fi)
    pi = np.asarray(pi)
    O = fi.size
    cols = np.concatenate([6 * fi[:, None] + np.arange(6)[None, :],
                           6 * n_frames + 3 * pi[:, None] + np.arange(3)[None, :]], axis=1)  # [O,9]
    cols = np.repeat(cols, 2, axis=0)                                                          # [2O,9]
    indptr = np.arange(0, 18 * O + 1, 9)
    return csr_matrix((np.ones(cols.size, dtype=int), cols.ravel(), indptr),
                      shape=(2 * O, 6 * n_frames + 3 * n_points))


def rodrigues_matrix(rvec):
    """Closed-form axis-angle -> R (what cv2.Rodrigues computes at bundleAdjuster.py:153,201;
    OpenCV itself is absent: mathematical definition)."""
    r = np.asarray(rvec, float).reshape(3)
    th = float(np.sqrt(r @ r))
    if th == 0.0:
        return np.eye(3)
    k = r / th
    Kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(th) * Kx + (1.0 - np.cos(th)) * (Kx @ Kx)


def reformat_point_result(x, n_frames, n_points):
    """x -> (points[P,3], list of F 4x4) (bundleAdjuster.py:137-157)."""
    cams = x[:6 * n_frames].reshape(n_frames, 6)
    pts = x[6 * n_frames:].reshape(n_points, 3)
    ext = []
    for f in range(n_frames):
        E = np.eye(4)
        E[:3, :3] = rodrigues_matrix(cams[f, :3])
        E[:3, 3] = cams[f, 3:]
        ext.append(E)
    return pts, ext


def adjust_points(ext, K, points_3D, points_2D, fi, pi, ftol=1e-4, xtol=1e-8, gtol=1e-8, verbose=0,
                  max_nfev=None, return_result=False):
    """Full BA exactly as the reference drives SciPy (bundleAdjuster.py:160-194):
    TRF, jac_sparsity, x_scale='jac', ftol=1e-4, 2-point finite differences, LSMR."""
    F, P = len(ext), len(points_3D)
    fi = np.asarray(fi)
    pi = np.asarray(pi)
    x0 = np.hstack([frame_parameters(ext), np.asarray(points_3D, float).reshape(3 * P)])
    A = sparsity_pattern(F, P, fi, pi)
    res = least_squares(point_fun, x0, jac_sparsity=A, verbose=verbose, x_scale="jac", ftol=ftol, xtol=xtol,
                        gtol=gtol, method="trf", max_nfev=max_nfev,
                        args=(np.asarray(K, float), F, P, fi, pi, np.asarray(points_2D, float)))
    out = reformat_point_result(res.x, F, P)
    return (out + (res,)) if return_result else out


def chessboard_points(pattern_size=12):
    """The (4,3) chessboard of side 2 in the x-z plane (bundleAdjuster.py:220-223)."""
    pts = np.zeros((pattern_size, 3))
    g = np.mgrid[0:4, 0:3].T.reshape(-1, 2) * 2
    pts[:, 0] = g[:, 0]
    pts[:, 2] = g[:, 1]
    return pts


def adjust_pose(ext, K, points_2D, ftol=1e-4, verbose=0, return_result=False):
    """Pose-only refinement (bundleAdjuster.py:214-243): dense TRF (exact SVD solver), ftol=1e-4."""
    F = len(ext)
    n = int(len(points_2D) / F)
    pts3 = chessboard_points(n)
    fi = np.repeat(np.arange(F), n)
    pi = np.tile(np.arange(n), F)
    x0 = frame_parameters(ext)
    res = least_squares(pose_fun, x0, verbose=verbose, ftol=ftol,
                        args=(np.asarray(K, float), F, fi, pi, pts3, np.asarray(points_2D, float)))
    cams = res.x.reshape(F, 6)
    out = [np.hstack([rodrigues_matrix(c[:3]), c[3:6].reshape(3, 1)]) for c in cams]
    return (out, res) if return_result else out


def jacobian_fd(x, K, n_frames, n_points, fi, pi, obs, h=1e-6):
    """Central-difference blocks (Jc[O,2,6], Jp[O,2,3]) — the checker for the analytic Jacobian the
    HIP path uses in place of SciPy's 2-point scheme (scipy/optimize/_numdiff.py:628-705)."""
    O = len(fi)
    cams = x[:6 * n_frames].reshape(n_frames, 6)
    pts = x[6 * n_frames:].reshape(n_points, 3)
    Jc = np.empty((O, 2, 6))
    Jp = np.empty((O, 2, 3))
    c, p = cams[fi], pts[pi]
    for k in range(6):
        d = np.zeros(6)
        d[k] = h * np.maximum(1.0, 1.0)
        Jc[:, :, k] = (project(p, c + d, K) - project(p, c - d, K)) / (2 * d[k])
    for k in range(3):
        d = np.zeros(3)
        d[k] = h
        Jp[:, :, k] = (project(p + d, c, K) - project(p - d, c, K)) / (2 * h)
    return Jc, Jp


# ------------------------------------------------------------------ triangulation (processor.py:246-261)

def triangulate_dlt(P1, P2, x1, x2):
    """Homogeneous two-view DLT for n points — what cv2.triangulatePoints computes
    (processor.py:259; OpenCV calib3d `triangulate.cpp`: rows x*P[2]-P[0], y*P[2]-P[1] for both views,
    4x4, solution = right singular vector of the smallest singular value), then X[:3]/X[3] (:260).
    P1,P2: [n,3,4]; x1,x2: [n,2] -> [n,3].  PARITY UNPINNED (no OpenCV here, no reference fixture)."""
    n = len(x1)
    out = np.empty((n, 3))
    for i in range(n):
        A = np.stack([x1[i, 0] * P1[i, 2] - P1[i, 0], x1[i, 1] * P1[i, 2] - P1[i, 1],
                      x2[i, 0] * P2[i, 2] - P2[i, 0], x2[i, 1] * P2[i, 2] - P2[i, 1]])
        X = np.linalg.svd(A)[2][-1]
        out[i] = X[:3] / X[3]
    return out


# ------------------------------------------------------------------ track bookkeeping (track.py, processor.py)

class Track:
    """Insertion-ordered {frame_ID: (x, y)} with an `updated` flag and a 3-D point (track.py:1-41)."""

    def __init__(self, prev_frame_ID, feature, frame_ID, correspondent):
        self.coordinates = {prev_frame_ID: feature}
        self.coordinates[frame_ID] = correspondent
        self.point = None
        self.updated = False

    def update(self, frame_ID, correspondent):
        self.coordinates[frame_ID] = correspondent
        self.updated = True

    def reset(self):
        self.updated = False

    def wasUpdated(self):
        return self.updated

    def getCoordinate(self, frame_ID):
        return self.coordinates.get(frame_ID)

    def getTriangulationData(self):
        ids = list(self.coordinates)
        return ids[0], ids[-1], self.coordinates[ids[0]], self.coordinates[ids[-1]]

    def getCoordinates(self):
        return self.coordinates

    def setPoint(self, point):
        self.point = point

    def getPoint(self):
        return self.point


def point_tracking(tracks, prev_ID, feature_points, ID, correspondents):
    """Track linking (processor.py:190-243): for each match in order, the FIRST live track whose
    coordinate at prev_ID equals the match's previous-frame point exactly is updated (last writer
    wins on the new coordinate); otherwise a new track is made.  Returns (popped, updated+new)."""
    fresh = []
    for fp, co in zip(feature_points, correspondents):
        key = (fp[0], fp[1])
        val = (co[0], co[1])
        hit = next((t for t in tracks if t.getCoordinate(prev_ID) == key), None)
        if hit is None:
            fresh.append(Track(prev_ID, key, ID, val))
        else:
            hit.update(ID, val)
    kept, popped = [], []
    for t in tracks:
        if t.wasUpdated():
            t.reset()
            kept.append(t)
        else:
            popped.append(t)
    return popped, kept + fresh


def manage_points(tracks):
    """Flatten tracks to BA arrays (processor.py:264-291); return order
    (points, coordinates, frame_indices, point_indices) as at :291."""
    points, coords, fidx, pidx = [], [], [], []
    for i, t in enumerate(tracks):
        points.append(t.getPoint())
        for f, c in t.getCoordinates().items():
            coords.append(c)
            pidx.append(i)
            fidx.append(f)
    return points, coords, fidx, pidx


# ------------------------------------------------------------------ exact reference for the BA linear algebra
#
# Independent of the kernels' formulations: the Jacobian by complex-step differentiation of a complex-analytic
# restatement of point_fun, the sums in long double (64-bit mantissa where the platform has one).  Every function that
# feeds a bound also returns the sum of the magnitudes of the terms it added (the `abs` entries), so a test can bound
# a floating-point sum of k terms by k * eps * sum|terms|.

LD = np.longdouble if np.finfo(np.longdouble).nmant >= 63 else np.float64
CLD = np.clongdouble if LD is np.longdouble else np.complex128


def _series_or_closed(s, closed, denom):
    """f(s) for the entire functions A, B below: Taylor series sum_k (-s)^k / denom(k) for |s| < 1/2 (24 terms: the
    remainder is below 1e-40), the closed form elsewhere.  denom(k) is an exact integer; 1 / denom(k) is rounded once,
    in the working precision."""
    s = np.asarray(s)
    small = np.abs(s) < 0.5
    out = np.empty_like(s)
    if small.any():
        ss = s[small]
        rt = np.real(ss).dtype.type
        acc = np.zeros_like(ss)
        term = np.ones_like(ss)
        for k in range(24):
            acc = acc + (rt(1) / rt(str(denom(k)))) * term
            term = term * (-ss)
        out[small] = acc
    if (~small).any():
        out[~small] = closed(s[~small])
    return out


def _rot_A(s):      # sin(sqrt s) / sqrt s
    return _series_or_closed(s, lambda z: np.sin(np.sqrt(z)) / np.sqrt(z), lambda k: math.factorial(2 * k + 1))


def _rot_B(s):      # (1 - cos(sqrt s)) / s
    return _series_or_closed(s, lambda z: (1.0 - np.cos(np.sqrt(z))) / z, lambda k: math.factorial(2 * k + 2))


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1],
                     a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def project_analytic(c, X, K):
    """c [n,6] (r, t), X [n,3] (real or complex) -> pixels [n,2].  Rodrigues as R = I + A(s)[r]x + B(s)[r]x^2 with
    s = r.r (no norm, no division by theta: complex-analytic in r, so complex steps differentiate it)."""
    r, t = c[:, :3], c[:, 3:6]
    s = (r * r).sum(axis=1)
    A, B = _rot_A(s)[:, None], _rot_B(s)[:, None]
    rx = _cross(r, X)
    Xc = X + A * rx + B * _cross(r, rx) + t
    K = np.asarray(K)
    u = [K[m, 0] * Xc[:, 0] + K[m, 1] * Xc[:, 1] + K[m, 2] * Xc[:, 2] for m in range(3)]
    return np.stack([u[0] / u[2], u[1] / u[2]], axis=1)


def point_fun_exact(x, K, n_frames, n_points, fi, pi, obs):
    """point_fun in long double -> [O, 2]."""
    x = np.asarray(x, np.float64).astype(LD)
    cams = x[:6 * n_frames].reshape(n_frames, 6)
    pts = x[6 * n_frames:].reshape(n_points, 3)
    return project_analytic(cams[fi], pts[pi], np.asarray(K, np.float64).astype(LD)) - np.asarray(obs).astype(LD)


def jacobian_exact(x, K, n_frames, n_points, fi, pi, obs, dtype=None, block=1 << 18):
    """Complex-step Jacobian blocks Jc [O,2,6], Jp [O,2,3] (real dtype of `dtype`, default long double):
    J[:, k] = Im f(x + i h e_k) / h with h = 1e-30 -- no subtraction, so exact to the working precision."""
    ct = CLD if dtype is None else dtype
    rt = np.real(np.zeros(1, ct)).dtype
    h = 1e-30
    x = np.asarray(x, np.float64)
    cams = x[:6 * n_frames].reshape(n_frames, 6).astype(rt)
    pts = x[6 * n_frames:].reshape(n_points, 3).astype(rt)
    Kc = np.asarray(K, np.float64).astype(rt)
    fi, pi = np.asarray(fi), np.asarray(pi)
    O = fi.size
    Jc = np.empty((O, 2, 6), rt)
    Jp = np.empty((O, 2, 3), rt)
    for lo in range(0, O, block):
        c0 = cams[fi[lo:lo + block]].astype(ct)
        p0 = pts[pi[lo:lo + block]].astype(ct)
        for k in range(6):
            c = c0.copy()
            c[:, k] += 1j * h
            Jc[lo:lo + block, :, k] = project_analytic(c, p0, Kc).imag / rt.type(h)
        for k in range(3):
            p = p0.copy()
            p[:, k] += 1j * h
            Jp[lo:lo + block, :, k] = project_analytic(c0, p, Kc).imag / rt.type(h)
    return Jc, Jp


def _segment_sum(keys, vals, n_out):
    """out[k] = sum of vals[keys == k] (vals [m, ...]) -> [n_out, ...] (sorted reduceat, dtype kept)."""
    out = np.zeros((n_out,) + vals.shape[1:], vals.dtype)
    if keys.size == 0:
        return out
    order = np.argsort(keys, kind="stable")
    ks = keys[order]
    starts = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
    out[ks[starts]] = np.add.reduceat(vals[order], starts, axis=0)
    return out


def normal_blocks(Jc, Jp, res, fi, pi, n_frames, n_points):
    """J^T J and J^T r by blocks, summed in long double: B [F,6,6], gc [F,6], C [P,3,3], gp [P,3], each with the
    sum of |terms| (key + "_abs") and the number of terms per entry (key + "_k").  Observations of cameras fi >= F
    (fixed cameras) add to the point blocks only."""
    Jc, Jp, r = (np.asarray(a).astype(LD) for a in (Jc, Jp, res))
    fi, pi = np.asarray(fi), np.asarray(pi)
    r = r.reshape(-1, 2)
    free = fi < n_frames
    out = {}
    for name, J, idx, n, sel in (("B", Jc, fi, n_frames, free), ("C", Jp, pi, n_points, slice(None))):
        Js, rs, ix = J[sel], r[sel], idx[sel]
        out[name] = _segment_sum(ix, np.einsum("omi,omj->oij", Js, Js), n)
        out[name + "_abs"] = _segment_sum(ix, np.einsum("omi,omj->oij", np.abs(Js), np.abs(Js)), n)
        g = "gc" if name == "B" else "gp"
        out[g] = _segment_sum(ix, np.einsum("omi,om->oi", Js, rs), n)
        out[g + "_abs"] = _segment_sum(ix, np.einsum("omi,om->oi", np.abs(Js), np.abs(rs)), n)
        cnt = np.bincount(ix, minlength=n)
        out[name + "_k"] = 2 * cnt
        out[g + "_k"] = 2 * cnt
    return out


def _diag3(C):
    C = np.asarray(C)
    return C[:, [0, 3, 5]] if C.ndim == 2 else np.einsum("pii->pi", C)


def jac_scale(B, C, old=None):
    """SciPy's compute_jac_scale (scipy/optimize/_lsq/common.py) from the diagonal of J^T J: scale_inv =
    sqrt(diag); the first call sets zeros to 1, later calls keep the running maximum with `old`.
    B [F,6,6]; C [P,3,3] or packed [P,6] (xx,xy,xz,yy,yz,zz) -> [6F + 3P]."""
    d = np.concatenate([np.einsum("fii->fi", np.asarray(B)).ravel(), _diag3(C).ravel()])
    si = np.sqrt(d)
    if old is None:
        si[si == 0] = 1.0
        return si
    return np.maximum(si, old)


def damp(B, C, si, reg):
    """Bd = B + reg diag(si_c^2), Cd = C + reg diag(si_p^2), in long double (C packed [P,6] or [P,3,3])."""
    B = np.asarray(B).astype(LD)
    C = np.asarray(C).astype(LD)
    si = np.asarray(si).astype(LD)
    F = B.shape[0]
    reg = LD(reg)
    Bd = B.copy()
    Bd[:, np.arange(6), np.arange(6)] += reg * (si[:6 * F].reshape(F, 6) ** 2)
    Cd = C.copy()
    sp2 = si[6 * F:].reshape(-1, 3) ** 2
    if C.ndim == 2:
        Cd[:, [0, 3, 5]] += reg * sp2
    else:
        Cd[:, np.arange(3), np.arange(3)] += reg * sp2
    return Bd, Cd


def unpack_sym3(C6):
    """packed [P,6] (xx,xy,xz,yy,yz,zz) -> [P,3,3]."""
    C6 = np.asarray(C6)
    i = [[0, 1, 2], [1, 3, 4], [2, 4, 5]]
    return C6[:, i]


def inv3(C):
    """Inverse of symmetric 3x3 blocks [P,3,3] by cofactors, in the dtype given."""
    a, b, c = C[:, 0, 0], C[:, 0, 1], C[:, 0, 2]
    d, e, f = C[:, 1, 1], C[:, 1, 2], C[:, 2, 2]
    m00, m01, m02 = d * f - e * e, c * e - b * f, b * e - c * d
    m11, m12, m22 = a * f - c * c, b * c - a * e, a * d - b * b
    det = a * m00 + b * m01 + c * m02
    out = np.stack([m00, m01, m02, m01, m11, m12, m02, m12, m22], axis=1).reshape(-1, 3, 3)
    return out / det[:, None, None]


def _pairs_of_points(fi, pi, lower=True):
    """All (o, o2) with pi[o] == pi[o2] and (lower) fi[o] >= fi[o2]."""
    fi, pi = np.asarray(fi), np.asarray(pi)
    order = np.argsort(pi, kind="stable")
    ps = pi[order]
    starts = np.flatnonzero(np.r_[True, ps[1:] != ps[:-1]])
    lens = np.diff(np.r_[starts, ps.size])
    # every pair inside a point's run: (start + a, start + b), a, b < len
    rep = np.repeat(np.arange(starts.size), lens * lens)
    base = np.repeat(starts, lens * lens)
    ofs = np.arange(rep.size) - np.repeat(np.cumsum(lens * lens) - lens * lens, lens * lens)
    L = np.repeat(lens, lens * lens)
    o = order[base + ofs // L]
    o2 = order[base + ofs % L]
    if lower:
        keep = fi[o] >= fi[o2]
        o, o2 = o[keep], o2[keep]
    return o, o2


def index_reference(fi, pi, F, P, F_fixed=0, chunk=512, max_band_span=192, pairs=True):
    """The index structures of a BA problem as ops.BADevice holds them (int32 arrays): the CSR by point over all
    observations, the CSR by camera over the F free cameras (fi >= F is a fixed camera), cam_span, and -- if `pairs` and the
    span allows -- the co-observation pairs of the free observations sorted stably by camera(o) * (span + 1) + camera(o) -
    camera(o2), cut into segments and chunks of at most `chunk` pairs, with the camera slabs.  Small inputs only."""
    fi, pi = np.asarray(fi, np.int64).reshape(-1), np.asarray(pi, np.int64).reshape(-1)
    if fi.size and (fi.min() < 0 or fi.max() >= F + F_fixed or pi.min() < 0 or pi.max() >= P):
        raise ValueError("frame / point index out of range")
    i32 = lambda a: np.ascontiguousarray(a, np.int32)
    ptr_of = lambda counts: np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    pt_ptr, pt_obs = ptr_of(np.bincount(pi, minlength=P)), np.argsort(pi, kind="stable")
    cam_ptr = ptr_of(np.bincount(fi, minlength=F + F_fixed)[:F])
    cam_obs = np.argsort(fi, kind="stable")[:cam_ptr[F]]
    # pairs in emission order: o ascending, then the observations of o's point in pt_obs order
    o, o2 = [], []
    for i in np.flatnonzero(fi < F):
        others = pt_obs[pt_ptr[pi[i]]:pt_ptr[pi[i] + 1]]
        others = others[fi[others] <= fi[i]]
        o += [i] * others.size
        o2 += list(others)
    o, o2 = np.array(o, np.int64), np.array(o2, np.int64)
    d = fi[o] - fi[o2]
    span = int(d.max()) if d.size else 0
    out = dict(pt_ptr=i32(pt_ptr), pt_obs=i32(pt_obs), cam_ptr=i32(cam_ptr), cam_obs=i32(cam_obs), cam_span=span, n_pairs=0,
               slabs=None)
    if not (pairs and d.size and span <= max_band_span and span < F and F * (span + 1) < 2 ** 31):
        return out
    key = fi[o] * (span + 1) + d
    order = np.argsort(key, kind="stable")
    seg_ids, counts = np.unique(key, return_counts=True)
    seg_lo, n_chunks = ptr_of(counts), -(-counts // chunk)
    seg_chunk_ptr = ptr_of(n_chunks)
    chunk_seg = np.repeat(np.arange(seg_ids.size), n_chunks)
    chunk_begin = seg_lo[chunk_seg] + chunk * (np.arange(chunk_seg.size) - seg_chunk_ptr[chunk_seg])
    out.update(n_pairs=int(d.size), pair_o=i32(o[order]), pair_o2=i32(o2[order]), pair_p=i32(pi[o[order]]), seg_ids=i32(seg_ids),
               seg_chunk_ptr=i32(seg_chunk_ptr), chunk_seg=i32(chunk_seg), chunk_begin=i32(chunk_begin),
               chunk_end=i32(np.minimum(chunk_begin + chunk, seg_lo[chunk_seg + 1])))
    per_slab = -(-F // 8)      # 8 slabs of cameras: the first segment and the first chunk of each, and the ends
    if per_slab >= 16:
        first = np.searchsorted(seg_ids // (span + 1), np.arange(9) * per_slab)
        out["slabs"] = (8, per_slab, first.astype(np.int64), seg_chunk_ptr[first])
    return out


def reduced_system(Jc, Jp, fi, pi, n_frames, n_points, Bd, Cd, gc, gp, Cinv=None, chunk=1 << 19):
    """Reduced camera system S = blockdiag(Bd) - sum_p E_p Cd_p^-1 E_p^T (dense 6F x 6F) and v = gc - sum_p E_p Cd_p^-1 gp_p,
    E_o = Jc_o^T Jp_o, summed in long double over the co-observation pairs.  Cd packed [P,6] or [P,3,3]; Cinv (same
    layouts) is used instead of inverting Cd when given.  -> dict(S, v, Cinv [P,3,3], S_abs, v_abs, S_k, v_k): the sums
    of |terms| and the numbers of elementary terms per entry."""
    F, P = n_frames, n_points
    fi, pi = np.asarray(fi), np.asarray(pi)
    Jc, Jp = np.asarray(Jc).astype(LD), np.asarray(Jp).astype(LD)
    if Cinv is None:
        Cd = np.asarray(Cd).astype(LD)
        Q = inv3(unpack_sym3(Cd) if Cd.ndim == 2 else Cd)
    else:
        Cinv = np.asarray(Cinv).astype(LD)
        Q = unpack_sym3(Cinv) if Cinv.ndim == 2 else Cinv
    E = np.einsum("oma,omb->oab", Jc, Jp)
    Ea = np.einsum("oma,omb->oab", np.abs(Jc), np.abs(Jp))
    Y = np.einsum("oab,obc->oac", E, Q[pi])
    Ya = np.einsum("oab,obc->oac", Ea, np.abs(Q[pi]))
    gpl = np.asarray(gp).astype(LD).reshape(P, 3)
    nobs = np.bincount(fi, minlength=F)
    v = np.asarray(gc).astype(LD).reshape(F, 6) - _segment_sum(fi, np.einsum("oac,oc->oa", Y, gpl[pi]), F)
    v_abs = np.abs(np.asarray(gc).astype(LD).reshape(F, 6)) + _segment_sum(fi, np.einsum("oac,oc->oa", Ya, np.abs(gpl[pi])), F)
    v_k = 18 * nobs + 1
    blocks = np.zeros((F, F, 6, 6), LD)
    blocks_a = np.zeros((F, F, 6, 6), LD)
    npair = np.zeros((F, F), np.int64)
    o_all, o2_all = _pairs_of_points(fi, pi)
    for lo in range(0, o_all.size, chunk):
        o, o2 = o_all[lo:lo + chunk], o2_all[lo:lo + chunk]
        key = fi[o].astype(np.int64) * F + fi[o2]
        order = np.argsort(key, kind="stable")
        ks = key[order]
        starts = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
        oo, oo2 = o[order], o2[order]
        blk = np.add.reduceat(np.einsum("oac,odc->oad", Y[oo], E[oo2]), starts, axis=0)
        blka = np.add.reduceat(np.einsum("oac,odc->oad", Ya[oo], Ea[oo2]), starts, axis=0)
        ku = ks[starts]
        blocks.reshape(F * F, 6, 6)[ku] += blk
        blocks_a.reshape(F * F, 6, 6)[ku] += blka
        npair.reshape(-1)[ku] += np.diff(np.r_[starts, ks.size])
    # mirror the strictly lower blocks
    il = np.tril_indices(F, -1)
    blocks[il[1], il[0]] = np.swapaxes(blocks[il], 1, 2)
    blocks_a[il[1], il[0]] = np.swapaxes(blocks_a[il], 1, 2)
    npair[il[1], il[0]] = npair[il]
    Bd = np.asarray(Bd).astype(LD).reshape(F, 6, 6)
    S4 = -blocks
    S4[np.arange(F), np.arange(F)] += Bd
    Sa4 = blocks_a
    Sa4[np.arange(F), np.arange(F)] += np.abs(Bd)
    S = S4.transpose(0, 2, 1, 3).reshape(6 * F, 6 * F)
    S_abs = Sa4.transpose(0, 2, 1, 3).reshape(6 * F, 6 * F)
    S_k = np.repeat(np.repeat(36 * npair + 1, 6, axis=0), 6, axis=1)
    return dict(S=S, v=v.reshape(-1), Cinv=Q, S_abs=S_abs, v_abs=v_abs.reshape(-1), S_k=S_k, v_k=np.repeat(v_k, 6))


def backsub(Jc, Jp, fi, pi, n_points, Cinv, gp, dc):
    """Point step dp_p = Cinv_p (gp_p - sum_o E_o^T dc_fi[o]) in long double -> (dp [P,3], dp_abs, dp_k)."""
    P = n_points
    fi, pi = np.asarray(fi), np.asarray(pi)
    Jc, Jp = np.asarray(Jc).astype(LD), np.asarray(Jp).astype(LD)
    Q = np.asarray(Cinv).astype(LD)
    Q = unpack_sym3(Q) if Q.ndim == 2 else Q
    dc = np.asarray(dc).astype(LD).reshape(-1, 6)
    gp = np.asarray(gp).astype(LD).reshape(P, 3)
    E = np.einsum("oma,omb->oab", Jc, Jp)
    Ea = np.einsum("oma,omb->oab", np.abs(Jc), np.abs(Jp))
    t = gp - _segment_sum(pi, np.einsum("oab,oa->ob", E, dc[fi]), P)
    ta = np.abs(gp) + _segment_sum(pi, np.einsum("oab,oa->ob", Ea, np.abs(dc[fi])), P)
    dp = np.einsum("pbc,pc->pb", Q, t)
    dpa = np.einsum("pbc,pc->pb", np.abs(Q), ta)
    k = 3 * (12 * np.bincount(pi, minlength=P) + 1) + 2
    return dp, dpa, np.repeat(k[:, None], 3, axis=1)


# ------------------------------------------------------------------ ragged problems

SPECIAL_THETA2 = (0.0, 1e-4 * (1 - 1e-6), 1e-4 * (1 + 1e-6), 1e-2 * (1 - 1e-6), 1e-2 * (1 + 1e-6),
                  (np.pi - 1e-3) ** 2, 16.0)


def ragged_ba_problem(seed, n_frames, n_points, max_len=30, p_len=0.2, empty_run=True, shuffle=False, long_tracks=0,
                      long_span=0, plant=True, obs_sigma=0.5, point_sigma=0.02, pose_sigma=0.002):
    """A BA problem shaped like pipeline output rather than like make_ba_problem: track lengths 1..max_len,
    geometrically distributed (consecutive frames), hot cameras next to nearly empty ones, a run of ceil(F/8) + 2
    cameras with no observation (one camera slab of the Schur build holds no segment), and planted co-observation
    segments of exactly 512 and 513 pairs and of more than 1024 (a camera with itself and with its neighbour).
    Cameras 1..7 (or the first seven outside the empty run) have rotation angles at the series / closed-form
    boundaries: theta = 0, theta^2 = 1e-4 (1 -+ 1e-6), 1e-2 (1 -+ 1e-6), theta = pi - 1e-3 and theta = 4; each is
    placed at C = -10 R[2] so the scene lies in front of it.  long_tracks > 0 adds that many points seen from cameras
    spread over long_span + 1 cameras (a wide band: the general Schur kernel).  shuffle: observations in random order.
    plant = False leaves the planted segments out (small problems for dense checks; the same random tracks).

    Returns make_ba_problem's dict (ext, K, pts0, obs, fi, pi, pts_gt, ext_gt) plus cams [F,6] (the (r, t) the
    cameras were built from, exactly), special [7] camera indices, empty (lo, hi) and planted {(i, j): n_pairs}."""
    from meatmodeler_amd import synth
    rng = np.random.default_rng(seed)
    F = int(n_frames)
    K = synth.default_K()
    ext_gt = synth.orbit_cameras(F, arc_deg=min(360.0, 0.72 * F))
    cams_gt = frame_parameters(ext_gt).reshape(F, 6)
    # the empty run: one whole camera slab (ceil(F/8) cameras) plus a camera either side
    cps = -(-F // 8)
    lo_e = 3 * cps - 1 if empty_run else F
    hi_e = min(F, lo_e + cps + 2) if empty_run else F
    usable = np.ones(F, bool)
    usable[lo_e:hi_e] = False
    # special rotations (chosen first; the camera sits at C = -10 R[2], looking at the scene)
    cand = [f for f in range(1, F) if usable[f]]
    special = np.array(cand[:len(SPECIAL_THETA2)])
    for f, th2 in zip(special, SPECIAL_THETA2):
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        rv = ax * np.sqrt(th2)
        R = rodrigues_matrix(rv)
        cams_gt[f, :3] = rv
        cams_gt[f, 3:] = -R @ (-10.0 * R[2])
    # hot and cold cameras: track starts drawn from a heavy-tailed weight; cold cameras are barriers few tracks cross
    w = rng.lognormal(0.0, 1.5, F) * usable
    cold = rng.choice(np.flatnonzero(usable[2:F - 2]) + 2, size=max(2, F // 20), replace=False)
    w[cold] = 0.0
    barrier = np.zeros(F, bool)
    barrier[cold] = True
    starts = rng.choice(F, size=n_points, p=w / w.sum())
    lens = np.minimum(rng.geometric(p_len, size=n_points), max_len)
    tracks = []
    for s0, L in zip(starts, lens):
        fr = np.arange(s0, min(s0 + L, F))
        bad = ~usable[fr] | (barrier[fr] & (rng.random(fr.size) > 0.02))
        if bad.any():
            fr = fr[:np.argmax(bad)]
        tracks.append(fr)

    fi0 = np.concatenate(tracks).astype(np.int64)
    pi0 = np.repeat(np.arange(len(tracks)), [t.size for t in tracks])
    o, o2 = _pairs_of_points(fi0, pi0)
    cnt = {}
    for k, n in zip(*np.unique(fi0[o] * F + fi0[o2], return_counts=True)):
        cnt[(int(k) // F, int(k) % F)] = int(n)

    def add(frames, times):      # `times` copies of a track seen from `frames`
        assert times >= 0, (frames, times)
        for i in frames:
            for j in frames:
                if j <= i:
                    cnt[(i, j)] = cnt.get((i, j), 0) + times
        tracks.extend([np.array(frames)] * times)

    # planted segments: neighbour pairs first (they add to both cameras' own segments), then the own segments
    planted = {}
    cold_s = sorted(int(c) for c in cold if usable[c - 1] and c - 1 not in cold and c + 1 not in cold)
    for target in (512, 513) if plant else ():
        # the first cold camera not used yet whose segment with its neighbour is still below the target
        c = next(c for c in cold_s if (c, c - 1) not in planted and cnt.get((c, c - 1), 0) <= target)
        add([c - 1, c], target - cnt.get((c, c - 1), 0))
        planted[(c, c - 1)] = target
    if plant:
        own = np.array([cnt.get((f, f), 0) for f in range(F)])
        hot = int(np.argmax(own))
        add([hot], max(0, 1100 - own[hot]))
        nb = hot - 1 if hot > 0 and usable[hot - 1] else hot + 1
        key = (max(hot, nb), min(hot, nb))
        add(sorted((hot, nb)), max(0, 1030 - cnt.get(key, 0)))
        planted[(hot, hot)] = cnt[(hot, hot)]
        planted[key] = cnt[key]
        used = {c for k in planted for c in k}
        quiet = [f for f in range(F) if usable[f] and cnt.get((f, f), 0) < 512 and all(abs(f - u) > 1 for u in used)]
        for f, target in zip(quiet[:2], (512, 513)):
            add([f], target - cnt.get((f, f), 0))
            planted[(f, f)] = target
    for k in planted:
        planted[k] = cnt[k]
    # tracks over a wide band of cameras (skipping the empty run)
    for _ in range(long_tracks):
        s0 = int(rng.integers(0, max(1, F - long_span)))
        fr = np.unique(np.r_[s0, s0 + long_span, rng.integers(s0, s0 + long_span, 12)])
        tracks.append(fr[usable[fr]])
    tracks = [t for t in tracks if t.size]
    P = len(tracks)
    fi = np.concatenate(tracks).astype(np.int64)
    pi = np.repeat(np.arange(P, dtype=np.int64), [t.size for t in tracks])
    pts_gt = rng.uniform(-2.0, 2.0, size=(P, 3))
    obs = project(pts_gt[pi], cams_gt[fi], K) + rng.normal(0.0, obs_sigma, size=(fi.size, 2))
    pts0 = pts_gt + rng.normal(0.0, point_sigma, size=(P, 3))
    cams = cams_gt.copy()
    plain = np.setdiff1d(np.arange(F), special)
    cams[plain, :3] += rng.normal(0.0, pose_sigma, (plain.size, 3))     # the special angles stay as chosen
    cams[:, 3:] += rng.normal(0.0, pose_sigma * 5, (F, 3))
    if shuffle:
        perm = rng.permutation(fi.size)
        fi, pi, obs = fi[perm], pi[perm], obs[perm]

    def to_ext(c):
        return np.stack([np.hstack([rodrigues_matrix(r[:3]), r[3:, None]]) for r in c])
    return dict(ext=to_ext(cams), K=K, pts0=pts0, obs=obs, fi=fi, pi=pi, pts_gt=pts_gt, ext_gt=to_ext(cams_gt), cams=cams,
                special=special, empty=(lo_e, hi_e), planted=planted)
