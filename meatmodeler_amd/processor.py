"""Drop-in for the hot-path functions of the reference's ``processor.py`` — same names, argument order and
return order, HIP kernels underneath (no CPU fallback: a missing extension or GPU raises).

    reference                                      here
    ---------------------------------------------  ---------------------------------------------------------
    cv2.ORB_create(nfeatures=...)  processor.py:308  ORB_create(nfeatures=...) -> ORB (detectAndCompute on device)
    featureTracking                processor.py:113  featureTracking     (mm_orb_detect_compute + mm_bf_knn2_* + ratio)
    (no counterpart)                                 verifyMatches       (mm_verify_matches: RANSAC fundamental matrix, inlier mask)
    (no counterpart)                                 verifyHomography    (mm_verify_homography: RANSAC homography, planar / rotation-only verdict)
    pointTracking                  processor.py:190  pointTracking       (hash join; same list semantics)
    triangulatePoints              processor.py:246  triangulatePoints   (mm_triangulate_dlt, batched over tracks)
    (no counterpart)                                 triangulateTracks   (mm_triangulate_tracks: all views, quality, flags)
    managePoints                   processor.py:264  managePoints
    keyframeTracking               processor.py:61   keyframeTracking    (mm-LK + mm-GFTT: calcOpticalFlowPyrLK / goodFeaturesToTrack)
    increaseContrast               processor.py:12   increaseContrast    (fixed-point L*a*b* + CLAHE), cvtColorBGR2GRAY
    PLY tail                       processor.py:480  savePointCloud      (mm_write_ply)
    (no counterpart)                                 densePointCloud     (mm_depth_sweep + mm_depth_fuse: plane-sweep depth maps, fused)

Video decode, calibration (chessboard / calibrateCamera) and PnP stay outside (SURVEY.md §8 "out of scope").
"""
import math

import numpy as np
import torch

from . import ops
from ._lib import default_context
from .orb_pattern import brief_pattern
from .track import Track


# ----------------------------------------------------------------------------------------------- key points

class KeyPoint:
    """Minimal cv2.KeyPoint look-alike (`.pt`, `.size`, `.angle`, `.response`, `.octave`)."""
    __slots__ = ("pt", "size", "angle", "response", "octave", "class_id")

    def __init__(self, x, y, size, angle, response, octave):
        self.pt = (x, y)
        self.size = size
        self.angle = angle
        self.response = response
        self.octave = octave
        self.class_id = -1


class KeyPoints:
    """Sequence of the key points of one frame.  Holds the device tensors (coordinates, descriptors) so that
    featureTracking never re-uploads them; `kps[i]` builds a `KeyPoint` on demand (its `.pt` is a pair of Python
    floats converted from float32, as cv2.KeyPoint.pt is)."""

    def __init__(self, xy_dev, meta_dev, resp_dev, mom_dev, desc_dev, scales):
        self.xy_dev, self.meta_dev, self.resp_dev, self.mom_dev, self.desc_dev = xy_dev, meta_dev, resp_dev, mom_dev, desc_dev
        self._scales = scales
        self._host = None

    def _h(self):
        if self._host is None:
            self._host = (self.xy_dev.cpu().numpy(), self.meta_dev.cpu().numpy(), self.resp_dev.cpu().numpy(),
                          self.mom_dev.cpu().numpy())
        return self._host

    @property
    def xy(self):
        """[n,2] float32 numpy (level-0 coordinates)."""
        return self._h()[0]

    def __len__(self):
        return self.xy_dev.shape[0]

    def __getitem__(self, i):
        xy, meta, resp, mom = self._h()
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        lvl = int(meta[i, 0])
        ang = math.degrees(math.atan2(float(mom[i, 1]), float(mom[i, 0]))) % 360.0
        return KeyPoint(float(xy[i, 0]), float(xy[i, 1]), 31.0 * float(self._scales[lvl]), ang, float(resp[i]), lvl)

    def __iter__(self):
        return (self[i] for i in range(len(self)))


class ORB:
    """Device ORB with the cv2.ORB_create defaults the reference relies on (processor.py:308)."""

    def __init__(self, nfeatures=500, scaleFactor=1.2, nlevels=8, edgeThreshold=31, fastThreshold=20, device=None):
        self.prm = ops.orb_params(nfeatures, nlevels, scaleFactor, edgeThreshold, fastThreshold)
        self.device = device
        self._wsp = {}

    def workspace(self, batch, H, W, device):
        key = (batch, H, W, str(device))
        w = self._wsp.get(key)
        if w is None:
            w = self._wsp[key] = ops.OrbWorkspace(batch, H, W, self.prm, device, brief_pattern())
        return w

    def _as_device_image(self, image):
        if isinstance(image, torch.Tensor):
            img = image
        else:
            import warnings
            with warnings.catch_warnings():          # (a frozen host frame is only read)
                warnings.simplefilter("ignore", UserWarning)
                img = torch.as_tensor(np.ascontiguousarray(image))
        if img.dtype != torch.uint8 or img.dim() != 2:
            raise ValueError("detectAndCompute expects a single-channel uint8 image [H, W]")
        dev = self.device or torch.device("cuda", torch.cuda.current_device())
        img = img.to(dev)
        if img.stride(1) != 1 or img.stride(0) % 4 != 0:
            H, W = img.shape
            pad = torch.zeros((H, (W + 3) // 4 * 4), dtype=torch.uint8, device=dev)
            pad[:, :W] = img
            img = pad[:, :W]
        return img

    def detectAndCompute(self, image, mask=None):
        """-> (KeyPoints, descriptors ndarray [n,32] uint8), like cv2.ORB.detectAndCompute(img, None)."""
        if mask is not None:
            raise NotImplementedError("mask is not supported (the reference always passes None, processor.py:129)")
        img = self._as_device_image(image)
        H, W = img.shape
        wsp = self.workspace(1, H, W, img.device)
        ops.orb_detect_compute(img.as_strided((1, H, W), (H * img.stride(0), img.stride(0), 1)), wsp)
        n = int(wsp.n[0].item())
        kps = KeyPoints(wsp.xy[0, :n].clone(), wsp.meta[0, :n].clone(), wsp.resp[0, :n].clone(), wsp.mom[0, :n].clone(),
                        wsp.desc[0, :n].clone(), ops.orb_level_sizes(H, W, self.prm)[3])
        desc = DeviceBackedDescriptors(kps.desc_dev)
        return kps, desc


class DeviceBackedDescriptors(np.ndarray):
    """ndarray [n,32] uint8 (what cv2 returns) that remembers its device twin."""

    def __new__(cls, desc_dev):
        host = np.asarray(desc_dev.cpu().numpy())
        host.setflags(write=False)          # the device twin stays valid only while the host copy cannot change
        obj = host.view(cls)
        obj._dev = desc_dev
        return obj

    def __array_finalize__(self, obj):
        # views, slices, permutations and copies do NOT inherit the device twin (desc[::-1] or desc[perm] have the
        # same shape but other rows): only the object made in __new__ carries it
        self._dev = None


def ORB_create(nfeatures=500, scaleFactor=1.2, nlevels=8, edgeThreshold=31, fastThreshold=20, **_ignored):
    return ORB(nfeatures, scaleFactor, nlevels, edgeThreshold, fastThreshold)


def _device_descriptors(desc, device):
    dev = getattr(desc, "_dev", None)
    if dev is not None and dev.shape[0] == len(desc) and not desc.flags.writeable:
        return dev
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if isinstance(desc, torch.Tensor):
        return desc.to(device).contiguous()
    return torch.as_tensor(np.ascontiguousarray(desc, np.uint8)).to(device)


def _points_xy(points):
    if isinstance(points, KeyPoints):
        return points.xy
    return np.array([p.pt for p in points], np.float32).reshape(-1, 2)


# ----------------------------------------------------------------------------------------------- increaseContrast / grey

def increaseContrast(frame):
    """CLAHE (clip limit 3.5, 8 x 8 tiles) on the L channel of L*a*b* (processor.py:12-26).  frame [H,W,3] u8 BGR
    (ndarray or device tensor) -> ndarray [H,W,3] u8 BGR."""
    ctx = default_context()
    t = frame if isinstance(frame, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(frame, np.uint8))
    out = ops.increase_contrast(t.to(ctx.device).contiguous().unsqueeze(0), 3.5, (8, 8), ctx=ctx)[0]
    return out if isinstance(frame, torch.Tensor) else out.cpu().numpy()


def cvtColorBGR2GRAY(frame):
    """cv2.cvtColor(frame, cv2.COLOR_BGR2GRAY) (processor.py:357): [H,W,3] u8 -> [H,W] u8."""
    ctx = default_context()
    t = frame if isinstance(frame, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(frame, np.uint8))
    out = ops.bgr_to_grey(t.to(ctx.device).contiguous(), ctx)
    return out if isinstance(frame, torch.Tensor) else out.cpu().numpy()


# ----------------------------------------------------------------------------------------------- keyframeTracking

def _upload_u8(a, device):
    """host u8 array (possibly frozen: torch warns about wrapping read-only memory, which is only read here) -> device."""
    import warnings
    a = np.ascontiguousarray(a, np.uint8)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        t = torch.from_numpy(a)
    return t.to(device)


_PYR_CACHE = []          # [(weakref to the host frame, max_level, device pyramid)]: the frame of one call is `prev` of the next


def _frame_pyramid(frame_grey, max_level, ctx):
    import weakref
    if isinstance(frame_grey, torch.Tensor):
        return ops.pyramid(frame_grey.to(ctx.device).contiguous(), max_level, ctx)
    for ref, lv, pyr in _PYR_CACHE:
        if ref() is frame_grey and lv == max_level and not frame_grey.flags.writeable and frame_grey.base is None:
            return pyr
    img = _upload_u8(frame_grey, ctx.device)
    pyr = ops.pyramid(img, max_level, ctx)
    try:
        # (only frames that cannot change behind the cache's back are remembered: the caller opts in by freezing an array
        # that OWNS its data -- a read-only view of a writable base can still change through the base)
        if not frame_grey.flags.writeable and frame_grey.base is None:
            _PYR_CACHE.append((weakref.ref(frame_grey), max_level, pyr))
            del _PYR_CACHE[:-2]
    except TypeError:
        pass
    return pyr


def calcOpticalFlowPyrLK(prevImg, nextImg, prevPts, nextPts=None, winSize=(21, 21), maxLevel=3, criteria=(3, 30, 0.01),
                         **_ignored):
    """cv2.calcOpticalFlowPyrLK (processor.py:79) -> (nextPts [n,1,2] f32, status [n,1] u8, err [n,1] f32).
    prevPts = None raises, as the cv2 call does (the reference reaches it when goodFeaturesToTrack found no corner at the
    last keyframe, processor.py:104-110, and fails there -- it must not turn into "never a keyframe again" here);
    an EMPTY point array gives (None, None, None), cv2's empty outputs."""
    if prevPts is None:
        raise ValueError("calcOpticalFlowPyrLK: prevPts is None (no points to track; cv2 raises "
                         "'(npoints = prevPtsMat.checkVector(2, CV_32F, true)) >= 0' here)")
    if len(prevPts) == 0:
        return None, None, None
    ctx = default_context()
    pp = _frame_pyramid(prevImg, maxLevel, ctx)
    pn = _frame_pyramid(nextImg, maxLevel, ctx)
    pts = torch.as_tensor(np.ascontiguousarray(np.asarray(prevPts, np.float32).reshape(-1, 2))).to(ctx.device)
    max_count = criteria[1] if len(criteria) > 1 else 30
    eps = criteria[2] if len(criteria) > 2 else 0.01
    nx, st, err = ops.lk_track(pp, pn, pts, winSize, max_count, eps, ctx)
    return (nx.cpu().numpy().reshape(-1, 1, 2), st.cpu().numpy().reshape(-1, 1), err.cpu().numpy().reshape(-1, 1))


def goodFeaturesToTrack(image, maxCorners, qualityLevel, minDistance, mask=None, blockSize=3, useHarrisDetector=False,
                        k=0.04, **_ignored):
    """cv2.goodFeaturesToTrack (processor.py:104) -> [n,1,2] f32 or None without corners."""
    if mask is not None or useHarrisDetector:
        raise NotImplementedError("mask / Harris detector are not supported (the reference passes mask=None, processor.py:105)")
    ctx = default_context()
    img = image.to(ctx.device) if isinstance(image, torch.Tensor) else _upload_u8(image, ctx.device)
    c = ops.good_features(img.contiguous(), maxCorners, qualityLevel, minDistance, blockSize, ctx)
    return c.reshape(-1, 1, 2) if len(c) else None


def keyframeTracking(frame_grey, prev_frame_grey, prev_frame_points, accumulated_error, lk_params, feature_params,
                     threshold=0.2):
    """Is this frame a keyframe?  (processor.py:61-110.)  Tracks the previous frame's points into this frame with
    pyramidal LK, adds the mean tracking error to `accumulated_error`, and once that exceeds threshold * width declares
    a keyframe, resets the error and re-seeds the points with goodFeaturesToTrack.
    -> (is_keyframe, new prev_frame_grey, new prev_frame_points, new accumulated_error)."""
    p, st, err = calcOpticalFlowPyrLK(prev_frame_grey, frame_grey, prev_frame_points, None, **lk_params)
    if p is not None:
        good_new = p[st == 1]
        prev_frame_grey = frame_grey
        prev_frame_points = good_new.reshape(-1, 1, 2)
        if err is not None:
            new_err = np.nan_to_num(err)
            new_err[new_err < 0] = 0
            accumulated_error += np.average(new_err)
        if accumulated_error > threshold * frame_grey.shape[1]:
            accumulated_error = 0
            prev_frame_points = goodFeaturesToTrack(prev_frame_grey, mask=None, **feature_params)
            return True, prev_frame_grey, prev_frame_points, accumulated_error
    return False, prev_frame_grey, prev_frame_points, accumulated_error


# ----------------------------------------------------------------------------------------------- PLY export

def savePointCloud(points, path):
    """The reference's export (processor.py:480-485: PyntCloud(DataFrame(points, columns x, y, z)).to_file(path +
    "Cloud.ply")): binary little-endian PLY with double x, y, z.  -> the file name."""
    from ._lib import lib as _l, MMError as _E
    pts = np.ascontiguousarray(np.asarray(points, np.float64).reshape(-1, 3))
    filename = path + "Cloud.ply"
    rc = _l.mm_write_ply(filename.encode(), pts.ctypes.data_as(__import__("ctypes").c_void_p), len(pts))
    if rc != 0:
        raise _E(f"mm_write_ply({filename!r}) failed ({rc})")
    return filename


# ----------------------------------------------------------------------------------------------- featureTracking

def featureTracking(new_keyframe, prev_orb_points, prev_orb_descriptors, orb, flann_params, threshold=0.75):
    """Detect + describe the new keyframe and match the previous keyframe against it (processor.py:113-142).

    `flann_params` is accepted for signature compatibility and ignored: the matcher is the exact brute-force
    Hamming 2-NN that FLANN-LSH approximates (query = previous keyframe, train = new keyframe, processor.py:133);
    a match is kept iff it has two neighbours and d0 < threshold * d1 (processor.py:136-137).
    Returns (prev_matches [M,2] f64, curr_matches [M,2] f64, new_points, new_descriptors); M = 0 gives the
    reference's `np.array([])`.
    """
    new_points, new_descriptors = orb.detectAndCompute(new_keyframe, None)
    t_dev = _device_descriptors(new_descriptors, None)
    q_dev = _device_descriptors(prev_orb_descriptors, t_dev.device)
    idx, dist = ops.bf_knn2(q_dev, t_dev)
    pairs, m = ops.ratio_filter_batched(idx.unsqueeze(0), dist.unsqueeze(0), threshold)
    M = int(m[0].item())
    good = pairs[0, :M].cpu().numpy()
    if M == 0:
        return np.array([]), np.array([]), new_points, new_descriptors
    pxy = _points_xy(prev_orb_points)
    nxy = _points_xy(new_points)
    prev_matches = pxy[good[:, 0]].astype(np.float64)
    curr_matches = nxy[good[:, 1]].astype(np.float64)
    return prev_matches, curr_matches, new_points, new_descriptors


def verifyMatches(prev_matches, curr_matches, **params):
    """Epipolar verification of what `featureTracking` returns: prev_matches / curr_matches [n,2] pixel coordinates of the
    matched key points in the previous and the new keyframe -> (mask [n] bool, F [3,3] f64 with curr^T F prev = 0, NaN if
    no model was found).  `params` as ops.verify_matches takes them (n_hyp, threshold_px, min_matches, min_inliers,
    refit_iters, seed, pair_base, on_fail): with on_fail="keep" a pair that fails keeps all its matches."""
    prev = np.asarray(prev_matches, np.float32).reshape(-1, 2)
    curr = np.asarray(curr_matches, np.float32).reshape(-1, 2)
    if prev.shape != curr.shape:
        raise ValueError("verifyMatches: prev_matches and curr_matches must have the same length")
    n = prev.shape[0]
    if n == 0:
        return np.zeros(0, bool), np.full((3, 3), np.nan)
    dev = default_context().device
    kp = torch.as_tensor(np.stack([prev, curr])).to(dev)
    idx = torch.arange(n, dtype=torch.int32, device=dev)
    pairs = torch.stack([idx, idx], dim=1).unsqueeze(0).contiguous()
    m = torch.full((1,), n, dtype=torch.int32, device=dev)
    pairs_out, m_out, F, _, _ = ops.verify_matches(kp, pairs, m, **params)
    mask = np.zeros(n, bool)
    mask[pairs_out[0, :int(m_out[0].item()), 0].cpu().numpy()] = True
    return mask, F[0].cpu().numpy().reshape(3, 3)


def guidedMatching(prev_xy, prev_desc, curr_xy, curr_desc, matches, model, homography=False, **params):
    """Guided matching of one keyframe pair: prev_xy [n1,2] / curr_xy [n2,2] pixel coordinates and prev_desc [n1,32] /
    curr_desc [n2,32] u8 descriptors of ALL key points of the previous and the new keyframe, matches [k,2] int
    (index into prev, index into curr) in strictly increasing order of the first column -- the matches `verifyMatches` kept --
    and model [3,3]: the F it returned (curr^T F prev = 0), or with homography=True an H with curr ~ H prev
    -> (matches_out [k',2] int32: the given matches and the new ones merged in order of the first column, is_new [k'] bool).
    `params` as ops.guided_match takes them (threshold_px, ratio, max_dist, cross_check).  A model that is not finite, or
    matches that are not in order, return the matches as they came."""
    prev = np.asarray(prev_xy, np.float32).reshape(-1, 2)
    curr = np.asarray(curr_xy, np.float32).reshape(-1, 2)
    dp = np.asarray(prev_desc, np.uint8).reshape(-1, 32)
    dc = np.asarray(curr_desc, np.uint8).reshape(-1, 32)
    if dp.shape[0] != prev.shape[0] or dc.shape[0] != curr.shape[0]:
        raise ValueError("guidedMatching: one descriptor per key point expected")
    seeds = np.asarray(matches, np.int32).reshape(-1, 2)
    cap = max(prev.shape[0], curr.shape[0], seeds.shape[0], 1)
    kp = np.zeros((2, cap, 2), np.float32)
    ds = np.zeros((2, cap, 32), np.uint8)
    kp[0, :prev.shape[0]], kp[1, :curr.shape[0]] = prev, curr
    ds[0, :dp.shape[0]], ds[1, :dc.shape[0]] = dp, dc
    pr = np.full((1, cap, 2), -1, np.int32)
    pr[0, :seeds.shape[0]] = seeds
    dev = default_context().device
    to = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)
    out, m_out, new, _ = ops.guided_match(to(kp), to(ds), to(np.array([prev.shape[0], curr.shape[0]], np.int32)), to(pr),
                                          to(np.array([seeds.shape[0]], np.int32)),
                                          to(np.asarray(model, np.float64).reshape(1, 9)),
                                          kind=to(np.array([1 if homography else 0], np.int32)), **params)
    k = int(m_out[0].item())
    return out[0, :k].cpu().numpy(), new[0, :k].cpu().numpy().astype(bool)


def recoverPose(prev_matches, curr_matches, K, F, **params):
    """The relative pose of two keyframes from their matches, the calibration and the fundamental matrix `verifyMatches`
    returned (curr^T F prev = 0): -> (n_front, R [3,3], t [3], mask [n] bool) with X_curr = R X_prev + t, |t| = 1; mask marks
    the matches in front of both cameras (a finite depth), n_front their number.  R and t are NaN when there is no model.
    `params` as ops.recover_poses takes them (min_matches, min_front_frac, ambiguous_frac)."""
    prev = np.asarray(prev_matches, np.float32).reshape(-1, 2)
    curr = np.asarray(curr_matches, np.float32).reshape(-1, 2)
    if prev.shape != curr.shape:
        raise ValueError("recoverPose: prev_matches and curr_matches must have the same length")
    n = prev.shape[0]
    if n == 0:
        return 0, np.full((3, 3), np.nan), np.full(3, np.nan), np.zeros(0, bool)
    dev = default_context().device
    kp = torch.as_tensor(np.stack([prev, curr])).to(dev)
    idx = torch.arange(n, dtype=torch.int32, device=dev)
    pairs = torch.stack([idx, idx], dim=1).unsqueeze(0).contiguous()
    m = torch.full((1,), n, dtype=torch.int32, device=dev)
    Fd = torch.as_tensor(np.ascontiguousarray(np.asarray(F, np.float64).reshape(1, 9))).to(dev)
    R, t, _, depth, _ = ops.recover_poses(kp, pairs, m, Fd, K, **params)
    mask = torch.isfinite(depth[0, :, 0]).cpu().numpy()
    return int(mask.sum()), R[0].cpu().numpy().reshape(3, 3), t[0].cpu().numpy(), mask


def _one_pair(name, prev_matches, curr_matches):
    """The two coordinate lists of a wrapper as the one-pair call of the ops: (n, kp_xy [2,n,2], pairs [1,n,2], m [1])."""
    prev = np.asarray(prev_matches, np.float32).reshape(-1, 2)
    curr = np.asarray(curr_matches, np.float32).reshape(-1, 2)
    if prev.shape != curr.shape:
        raise ValueError(f"{name}: prev_matches and curr_matches must have the same length")
    n = prev.shape[0]
    if n == 0:
        return 0, None, None, None
    dev = default_context().device
    kp = torch.as_tensor(np.stack([prev, curr])).to(dev)
    idx = torch.arange(n, dtype=torch.int32, device=dev)
    pairs = torch.stack([idx, idx], dim=1).unsqueeze(0).contiguous()
    return n, kp, pairs, torch.full((1,), n, dtype=torch.int32, device=dev)


def verifyHomography(prev_matches, curr_matches, **params):
    """A RANSAC homography between two keyframes on what `featureTracking` returns (the input of `verifyMatches`, not its
    output): -> (mask [n] bool, H [3,3] f64 with curr ~ H prev, NaN if no model was found, flags -- the HOMOG_* bits of
    ops.verify_homography).  `params` as ops.verify_homography takes them; with verify_info = the [1,4] info row of
    ops.verify_matches on the same matches the flags carry the planar / rotation-only verdict HOMOG_DEGENERATE."""
    n, kp, pairs, m = _one_pair("verifyHomography", prev_matches, curr_matches)
    if n == 0:
        return np.zeros(0, bool), np.full((3, 3), np.nan), ops.HOMOG_TOO_FEW
    pairs_out, m_out, H, _, info = ops.verify_homography(kp, pairs, m, **params)
    mask = np.zeros(n, bool)
    mask[pairs_out[0, :int(m_out[0].item()), 0].cpu().numpy()] = True
    return mask, H[0].cpu().numpy().reshape(3, 3), int(info[0, 0].item())


def recoverPoseFromHomography(prev_matches, curr_matches, K, H, **params):
    """The motion a homography between two keyframes implies (curr ~ H prev, as `verifyHomography` returns it):
    -> (n_front, R [3,3], t [3], mask [n] bool, normal [3], flags) with X_curr = R X_prev + t.  A plane: |t| = 1, normal its
    unit-distance normal in the previous camera, mask the matches in front of both cameras; a camera that only turned
    (flags & HPOSE_ROTATION): t = 0, normal NaN, no depths.  `params` as ops.recover_poses_homography takes them
    (normal_hint [1,3], min_matches, min_front_frac, ambiguous_frac, rotation_tol)."""
    n, kp, pairs, m = _one_pair("recoverPoseFromHomography", prev_matches, curr_matches)
    if n == 0:
        return 0, np.full((3, 3), np.nan), np.full(3, np.nan), np.zeros(0, bool), np.full(3, np.nan), ops.POSE_TOO_FEW
    Hd = torch.as_tensor(np.ascontiguousarray(np.asarray(H, np.float64).reshape(1, 9))).to(kp.device)
    if params.get("normal_hint") is not None:
        params = dict(params, normal_hint=torch.as_tensor(np.asarray(params["normal_hint"], np.float64).reshape(1, 3)).to(kp.device))
    R, t, _, normal, depth, info = ops.recover_poses_homography(kp, pairs, m, Hd, K, **params)
    mask = torch.isfinite(depth[0, :, 0]).cpu().numpy()
    return (int(mask.sum()), R[0].cpu().numpy().reshape(3, 3), t[0].cpu().numpy(), mask, normal[0].cpu().numpy(),
            int(info[0, 0].item()))


def resectCameras(points_3D, points_2D, K, prior=None, **params):
    """Camera registration against known 3-D points, the robust counterpart of the reference's cv2.solvePnP call
    (processor.py:175): points_3D / points_2D are per-frame lists of [n_f, 3] object points and [n_f, 2] pixels (row i of one
    belongs to row i of the other); prior: optional [n, 3, 4] starting poses (a non-finite one counts as absent)
    -> (extrinsics [n, 3, 4] f64 -- [R|t] per frame, NaN where no pose was found --, masks: per frame the [n_f] bool inliers,
    info [n, 6] i32 as ops.resect_cameras returns it).  `params` as ops.resect_cameras takes them (n_hyp, threshold_px,
    min_rows, min_inliers, refit_iters, polish_iters, seed, cam_base, and planar = None / "auto" / "only" with planar_tol and
    collinear_tol: frames whose object points are coplanar, a chessboard's, need "auto" or "only")."""
    if len(points_3D) != len(points_2D):
        raise ValueError("resectCameras: points_3D and points_2D must have one entry per frame")
    X3 = [np.asarray(a, np.float64).reshape(-1, 3) for a in points_3D]
    x2 = [np.asarray(a, np.float64).reshape(-1, 2) for a in points_2D]
    if any(len(a) != len(b) for a, b in zip(X3, x2)):
        raise ValueError("resectCameras: a frame's points_3D and points_2D must have the same length")
    n = len(X3)
    if n == 0:
        return np.zeros((0, 3, 4)), [], np.zeros((0, 6), np.int32)
    dev = default_context().device
    counts = np.array([len(a) for a in X3], np.int64)
    cam_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    total = int(cam_ptr[-1])
    Xd = torch.as_tensor(np.ascontiguousarray(np.concatenate(X3).reshape(-1, 3))).to(dev)
    od = torch.as_tensor(np.ascontiguousarray(np.concatenate(x2).reshape(-1, 2))).to(dev)
    idx = torch.arange(total, dtype=torch.int32, device=dev)
    pr = None
    if prior is not None:
        pr = torch.as_tensor(np.ascontiguousarray(np.asarray(prior, np.float64)[:, :3, :].reshape(n, 12))).to(dev)
    ext, _, inlier, info = ops.resect_cameras(K, Xd, od, idx, torch.as_tensor(cam_ptr).to(dev), idx, prior=pr, **params)
    mask = inlier.cpu().numpy().astype(bool)
    return ext.cpu().numpy(), [mask[cam_ptr[f]:cam_ptr[f + 1]] for f in range(n)], info.cpu().numpy()


def alignSimilarity(points_src, points_dst, **params):
    """A robust similarity between two sets of corresponding 3-D points, points_dst ~ s R points_src + d (the reference has no
    counterpart: it is metric through its chessboard): [n, 3] host arrays, row i of one belongs to row i of the other
    -> (sim [13] f64 = (s, R row-major, d), NaN where no model was found; mask [n] bool, the inliers; info [4] i32 as
    ops.align_similarity returns it).  `params` as ops.align_similarity takes them (tau or tau_rel, n_hyp, min_points,
    min_inliers, refit_iters, with_scale, seed, collinear_tol)."""
    src = np.ascontiguousarray(np.asarray(points_src, np.float64).reshape(-1, 3))
    dst = np.ascontiguousarray(np.asarray(points_dst, np.float64).reshape(-1, 3))
    if src.shape != dst.shape:
        raise ValueError("alignSimilarity: points_src and points_dst must have the same length")
    dev = default_context().device
    sim, _, inlier, info = ops.align_similarity(torch.as_tensor(src).to(dev), torch.as_tensor(dst).to(dev), **params)
    return sim[0].cpu().numpy(), inlier.cpu().numpy().astype(bool), info[0].cpu().numpy()


def applySimilarity(sim, points=None, extrinsics=None):
    """The similarity `sim` [13] (alignSimilarity) applied to host arrays: points [P, 3] -> s R X + d, extrinsics [F, 3|4, 4] ->
    [Rc R^T | s tc - Rc R^T d] as [F, 3, 4] (every projection is unchanged).  -> (points, extrinsics), new arrays or None; a
    non-finite sim returns them as they were."""
    dev = default_context().device
    sd = torch.as_tensor(np.ascontiguousarray(np.asarray(sim, np.float64).reshape(13))).to(dev)
    pd = ed = None
    if points is not None:
        pd = torch.as_tensor(np.ascontiguousarray(np.asarray(points, np.float64).reshape(-1, 3))).to(dev)
    if extrinsics is not None:
        e = np.asarray(extrinsics, np.float64)
        ed = torch.as_tensor(np.ascontiguousarray(e.reshape(-1, e.shape[-2], 4)[:, :3, :])).to(dev)
    ops.apply_similarity(sd, pd, ed)
    return (None if pd is None else pd.cpu().numpy()), (None if ed is None else ed.cpu().numpy())


def densePointCloud(frames, K, extrinsics, ranges, **params):
    """A dense point cloud from grey frames with known cameras (the reference stops at the adjusted corner points, though it
    was written to model an item and estimate its volume): frames [F, H, W] u8 (host array or device tensor), K 3 x 3,
    extrinsics [F, 3|4, 4] and ranges [F, 2] = (dmin, dmax), the depth range each frame sees.  Every `every`-th frame gets a
    plane-sweep depth map against its neighbouring frames and the maps are checked against each other (pipeline.dense_cloud;
    `params` as pipeline.dense_options takes them) -> (points [n, 3] f64, grey [n] u8) as NumPy arrays, in (view, row, column)
    order, ready for savePointCloud.  Duplicate surface points from neighbouring views are not merged."""
    from .pipeline import dense_cloud
    ctx = default_context()
    f = frames if torch.is_tensor(frames) else torch.as_tensor(np.ascontiguousarray(frames, np.uint8))
    if f.dtype != torch.uint8 or f.dim() != 3:
        raise ValueError("densePointCloud: frames [F, H, W] u8 expected")
    out = dense_cloud(f.to(ctx.device), K, extrinsics, ranges, ctx=ctx, **params)
    return out["points"].cpu().numpy(), out["grey"].cpu().numpy()


def rotation_vector(R):
    """The rotation vector (axis times angle, what cv2.Rodrigues returns for a matrix) of a 3 x 3 rotation, on the host."""
    R = np.asarray(R, np.float64).reshape(3, 3)
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    sn, cs = 0.5 * np.linalg.norm(w), 0.5 * (np.trace(R) - 1.0)
    th = math.atan2(sn, cs)
    if sn > 1e-8:
        return w * (th / (2.0 * sn))
    if cs > 0.0:      # near the identity: R - R^T = 2 [w]x to first order
        return 0.5 * w
    # near a half turn: R + I = 2 a a^T; the largest column gives the axis, its sign does not matter at exactly pi
    B = 0.5 * (R + np.eye(3))
    k = int(np.argmax(np.diag(B)))
    ax = B[:, k] / math.sqrt(max(B[k, k], 1e-300))
    if w @ ax < 0.0:
        ax = -ax
    return ax * th


def poseEstimationFromCorners(corners, pattern_shape, side_length, camera_intrinsic_matrix, **params):
    """The part of the reference's poseEstimation (processor.py:145-187) that follows cv2.cornerSubPix: the pose of the camera
    over a flat chessboard from its refined corners [x * y, 2] (any shape cv2 returns them in), pattern_shape = (x, y) and the
    square's side_length, with the object points the reference builds (x along X, y along Z, Y = 0)
    -> (rvec [3, 1], tvec [3, 1], extrinsic_matrix [3, 4], projection_matrix [3, 4]) or None when no pose was found: no
    model at all, or one that fewer than min_inliers corners (default: half of them) agree with.  A list of corner arrays gives
    a list of such results from one call.  The pose is a RANSAC homography polished on the reprojection error
    (ops.resect_planar; `params` as it takes them).  It takes NO distortion coefficients: undistort the corners first
    (cv2.undistortPoints with P = K) when the lens needs it."""
    many = isinstance(corners, (list, tuple))
    frames = [np.asarray(c, np.float64).reshape(-1, 2) for c in (corners if many else [corners])]
    x, y = pattern_shape
    objp = np.zeros((x * y, 3), np.float32)
    grid = np.mgrid[0:x, 0:y].T.reshape(-1, 2) * side_length
    objp[:, 0] = grid[:, 0]
    objp[:, 2] = grid[:, 1]
    if any(len(f) != x * y for f in frames):
        raise ValueError("poseEstimationFromCorners: every frame needs pattern_shape[0] * pattern_shape[1] corners")
    K = np.asarray(camera_intrinsic_matrix, np.float64).reshape(3, 3)
    params.setdefault("min_inliers", (x * y + 1) // 2)
    ext, _, info = resectCameras([objp.astype(np.float64)] * len(frames), frames, K, planar="only", **params)
    refuse = ops.RESECT_TOO_FEW | ops.RESECT_NO_MODEL | ops.RESECT_WEAK
    out = []
    for E, row in zip(ext, info):
        if not np.isfinite(E).all() or (row[0] & refuse) or not (row[0] & ops.RESECT_PLANAR):
            out.append(None)
            continue
        out.append((rotation_vector(E[:, :3]).reshape(3, 1), E[:, 3].reshape(3, 1).copy(), E.copy(), K @ E))
    return out if many else out[0]


# ----------------------------------------------------------------------------------------------- pointTracking

def pointTracking(tracks, prev_keyframe_ID, feature_points, keyframe_ID, correspondents):
    """Track linking with the reference's list semantics (processor.py:190-243) as a hash join:
    the FIRST live track whose coordinate at `prev_keyframe_ID` equals the match's previous-frame point is
    updated (a later match on the same track overwrites its new coordinate); other matches start new tracks,
    appended after the surviving ones in match order; tracks not updated are popped in list order."""
    first = {}
    for pos, track in enumerate(tracks):
        c = track.getCoordinate(prev_keyframe_ID)
        if c is not None:
            first.setdefault((float(c[0]), float(c[1])), pos)
    new_tracks = []
    for fp, co in zip(feature_points, correspondents):
        feature_point = (fp[0], fp[1])
        correspondent = (co[0], co[1])
        pos = first.get((float(fp[0]), float(fp[1])))
        if pos is None:
            new_tracks.append(Track(prev_keyframe_ID, feature_point, keyframe_ID, correspondent))
        else:
            tracks[pos].update(keyframe_ID, correspondent)
    updated_tracks, popped_tracks = [], []
    for track in tracks:
        if track.wasUpdated():
            track.reset()
            updated_tracks.append(track)
        else:
            popped_tracks.append(track)
    updated_tracks += new_tracks
    return popped_tracks, updated_tracks


# ----------------------------------------------------------------------------------------------- triangulatePoints

def triangulatePoints(tracks, projections):
    """Two-view DLT of every track from its first and last observation (processor.py:246-261), one kernel launch
    for all tracks; each track receives a (1,3) float64 array via setPoint, as in the reference."""
    n = len(tracks)
    if n == 0:
        return
    f0 = np.empty(n, np.int32)
    f1 = np.empty(n, np.int32)
    x0 = np.empty((n, 2), np.float64)
    x1 = np.empty((n, 2), np.float64)
    for i, track in enumerate(tracks):
        a, b, pa, pb = track.getTriangulationData()
        f0[i], f1[i] = a, b
        x0[i] = (pa[0], pa[1])
        x1[i] = (pb[0], pb[1])
    n_proj = len(projections)
    if min(f0.min(), f1.min()) < -n_proj or max(f0.max(), f1.max()) >= n_proj:
        raise IndexError("list index out of range")          # what projections[frame_ID] raises, processor.py:257-258
    f0[f0 < 0] += n_proj                                       # (a negative ID indexes from the end, as in the reference)
    f1[f1 < 0] += n_proj
    ctx = default_context()
    dev = ctx.device
    proj = torch.as_tensor(np.ascontiguousarray(np.asarray(projections, np.float64).reshape(-1, 3, 4))).to(dev)
    X = ops.triangulate_dlt(proj, torch.as_tensor(f0).to(dev), torch.as_tensor(f1).to(dev),
                            torch.as_tensor(x0).to(dev), torch.as_tensor(x1).to(dev), ctx).cpu().numpy()
    for i, track in enumerate(tracks):
        track.setPoint(X[i:i + 1].copy())


def triangulateTracks(tracks, projections, **thresholds):
    """Multi-view sibling of triangulatePoints: every track is triangulated from ALL of track.getCoordinates(), in
    insertion order (ops.triangulate_tracks: linear least squares + a few Levenberg-Marquardt steps), and receives a (1,3)
    float64 array via setPoint.  `thresholds`: refine_iters, max_reproj_px, min_angle_deg, min_depth.
    -> (quality [n,4] f64 = (rms_px, max_px, min_depth, cos_parallax), flags [n] i32 of ops.TRI_* bits) as NumPy arrays.
    Frame IDs behave as in triangulatePoints: a negative ID indexes from the end, one outside the list raises IndexError."""
    n = len(tracks)
    if n == 0:
        return np.zeros((0, 4)), np.zeros(0, np.int32)
    lens = np.fromiter((len(t.getCoordinates()) for t in tracks), np.int64, n)
    track_ptr = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=track_ptr[1:])
    if track_ptr[-1] >= 2 ** 31:
        raise ValueError("triangulateTracks: more than 2^31 - 1 observations")
    frames = np.fromiter((f for t in tracks for f in t.getCoordinates().keys()), np.int64, int(track_ptr[-1]))
    xy = np.array([(c[0], c[1]) for t in tracks for c in t.getCoordinates().values()], np.float64).reshape(-1, 2)
    n_proj = len(projections)
    if len(frames) and (frames.min() < -n_proj or frames.max() >= n_proj):
        raise IndexError("list index out of range")          # what projections[frame_ID] raises, processor.py:257-258
    frames[frames < 0] += n_proj
    ctx = default_context()
    dev = ctx.device
    proj = torch.as_tensor(np.ascontiguousarray(np.asarray(projections, np.float64).reshape(-1, 3, 4))).to(dev)
    X, quality, flags = ops.triangulate_tracks(proj, torch.as_tensor(track_ptr.astype(np.int32)).to(dev),
                                               torch.as_tensor(frames.astype(np.int32)).to(dev), torch.as_tensor(xy).to(dev),
                                               ctx=ctx, **thresholds)
    X = X.cpu().numpy()
    for i, track in enumerate(tracks):
        track.setPoint(X[i:i + 1].copy())
    return quality.cpu().numpy(), flags.cpu().numpy()


# ----------------------------------------------------------------------------------------------- managePoints

def managePoints(tracks):
    """Flatten tracks into BA arrays (processor.py:264-291).  Return order is the reference's:
    (points, coordinates, frame_indices, point_indices)."""
    points, coordinates, frame_indices, point_indices = [], [], [], []
    for point_index, track in enumerate(tracks):
        points.append(track.getPoint())
        obs = track.getCoordinates()
        coordinates.extend(obs.values())
        frame_indices.extend(obs.keys())
        point_indices.extend([point_index] * len(obs))
    return points, coordinates, frame_indices, point_indices


# ----------------------------------------------------------------------------------------------- the driver loop

def processFrames(frames, camera_matrix, extrinsic_for_frame, path, lk_params, feature_params, flann_params=None,
                  threshold=0.1, nfeatures=20000, adjust=True):
    """The body of the reference's `process` (processor.py:294-489) on frames that are already decoded, in the
    reference's call order: contrast -> grey -> keyframe gate (:357-365) -> on a keyframe ORB + matching + track linking
    (:378-391) -> after the last frame triangulation, flattening, bundle adjustment and the PLY export (:418-485).
    What stays outside (video decode, chessboard detection, calibrate, poseEstimation, adjustPose)
    is supplied by the caller: `frames` = iterable of [H,W,3] u8 BGR images, `camera_matrix` = K, and
    `extrinsic_for_frame(i) -> 3x4` for the keyframes (every keyframe counts as "has a chessboard").
    -> dict(points [P,3], extrinsics (list of 4x4) | None, keyframes (frame indices), tracks, file)."""
    from . import bundleAdjuster
    orb = ORB_create(nfeatures=nfeatures)
    it = iter(frames)
    start_frame = next(it)
    prev_frame_grey = cvtColorBGR2GRAY(increaseContrast(start_frame))
    prev_frame_grey.setflags(write=False)          # (lets the LK pyramid of a frame be reused by the next call)
    prev_frame_points = goodFeaturesToTrack(prev_frame_grey, mask=None, **feature_params)
    accumulative_error = 0
    prev_orb_points, prev_orb_descriptors = orb.detectAndCompute(prev_frame_grey, None)
    keyframes = [0]
    tracks, popped_tracks = [], []
    prev_keyframe_ID, keyframe_ID = 0, 1
    for index, frame in enumerate(it, start=1):
        frame_grey = cvtColorBGR2GRAY(increaseContrast(frame))
        frame_grey.setflags(write=False)
        is_keyframe, prev_frame_grey, prev_frame_points, accumulative_error = keyframeTracking(
            frame_grey, prev_frame_grey, prev_frame_points, accumulative_error, lk_params, feature_params,
            threshold=threshold)
        if is_keyframe:
            keyframes.append(index)
            prev_matches, curr_matches, prev_orb_points, prev_orb_descriptors = featureTracking(
                frame_grey, prev_orb_points, prev_orb_descriptors, orb, flann_params)
            new_popped_tracks, tracks = pointTracking(tracks, prev_keyframe_ID, prev_matches, keyframe_ID, curr_matches)
            popped_tracks += new_popped_tracks
            prev_keyframe_ID = keyframe_ID
            keyframe_ID += 1
    popped_tracks += tracks
    out = dict(points=np.zeros((0, 3)), extrinsics=None, keyframes=keyframes, tracks=popped_tracks, file=None)
    if not popped_tracks:
        return out
    K = np.asarray(camera_matrix, float)
    extrinsic_matrices = [np.asarray(extrinsic_for_frame(i), float)[:3, :] for i in keyframes]
    projections = [K @ e for e in extrinsic_matrices]                     # processor.py:448
    triangulatePoints(popped_tracks, projections)
    points, points_2d, frame_indices, point_indices = managePoints(popped_tracks)
    if adjust:
        adjusted_points, adjusted_positions = bundleAdjuster.adjustPoints(
            np.array(extrinsic_matrices), K, np.array(points), np.array(points_2d), np.array(frame_indices),
            np.array(point_indices))
        out.update(points=adjusted_points, extrinsics=adjusted_positions)
    else:
        out.update(points=np.array(points).reshape(-1, 3))
    if path is not None:
        out["file"] = savePointCloud(out["points"], path)
    return out
