"""An independent restatement, in NumPy and Python integers, of the per-frame front end that oracle/frame_oracle.c defines
and meatmodeler_amd/csrc/flow.hip / contrast.hip implement: pyramid, pyramidal Lucas-Kanade, Shi-Tomasi corners, the
fixed-point L*a*b* conversion, CLAHE and the grey conversion.  TEST INFRASTRUCTURE ONLY (tests/ imports it, nothing else).

It is written from DESIGN.md section 3b and the published algorithms, not from the C file, and on purpose in another shape:
whole-image derivative maps that are sampled afterwards (as OpenCV does) where the C code evaluates taps per window pixel,
a modular reflect-101 index where it bounces in a loop, np.bincount / np.cumsum / integral images where it counts in loops,
a brute-force minimum-distance test where it walks a bucket grid, vectorised int64 where it is scalar.  What it shares with
the C file is the DEFINITION only: the constants of section 3b (tables of meatmodeler_amd/frame_tables.py, fixed-point
matrices, bit widths) and the order of the few floating-point operations, which the definition fixes.
tests/test_frame_reference_cpu.py requires the two to agree bit for bit; a disagreement is a question about the definition.

`lab_float` is a third statement of the colour conversion: CIELAB in float64 with no table, the yardstick of the
fixed-point conversion's accuracy.
"""
import math

import numpy as np

F32 = np.float32
I64 = np.int64


# ---- borders ------------------------------------------------------------------------------------------------------------
def reflect101(idx, n):
    """Index array -> reflect-101 position in [0, n): ... 2 1 | 0 1 2 .. n-1 | n-2 n-3 ...; any number of bounces."""
    idx = np.asarray(idx, I64)
    if n == 1:
        return np.zeros_like(idx)
    period = 2 * n - 2
    m = np.mod(idx, period)
    return np.where(m >= n, period - m, m)


def window(img, x0, y0, cw, ch):
    """The ch x cw window with top-left corner (x0, y0) of the reflect-101 continuation of `img`, int64."""
    h, w = img.shape
    rows = reflect101(np.arange(y0, y0 + ch), h)
    cols = reflect101(np.arange(x0, x0 + cw), w)
    return img[np.ix_(rows, cols)].astype(I64)


def window_zero(img, x0, y0, cw, ch):
    """The same window of the continuation of `img` by ZEROS."""
    h, w = img.shape
    out = np.zeros((ch, cw), I64)
    ya, yb, xa, xb = max(y0, 0), min(y0 + ch, h), max(x0, 0), min(x0 + cw, w)
    if ya < yb and xa < xb:
        out[ya - y0:yb - y0, xa - x0:xb - x0] = img[ya:yb, xa:xb]
    return out


def descale(x, n):
    return (x + (1 << (n - 1))) >> n


# ---- pyramid ------------------------------------------------------------------------------------------------------------
def pyr_down(img):
    """[1 4 6 4 1] / 16 in both directions on the reflected image, every second sample, (sum + 128) >> 8."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    hd, wd = (h + 1) // 2, (w + 1) // 2
    p = window(img, -2, -2, 2 * wd + 3, 2 * hd + 3)
    taps = (1, 4, 6, 4, 1)
    rows = sum(k * p[:, i:i + 2 * wd:2] for i, k in enumerate(taps))          # [2 hd + 3, wd]
    full = sum(k * rows[i:i + 2 * hd:2] for i, k in enumerate(taps))          # [hd, wd]
    return ((full + 128) >> 8).astype(np.uint8)


def pyramid(img, max_level):
    levels = [np.ascontiguousarray(img, np.uint8)]
    for _ in range(max_level):
        levels.append(pyr_down(levels[-1]))
    return levels


# ---- pyramidal Lucas-Kanade ---------------------------------------------------------------------------------------------
W_BITS = 14
LK_LABELS = ("start_outside", "rejected", "left_image", "eps", "half_step", "count", "zero_count", "final_outside")


def scharr_maps(img):
    """Scharr derivatives (3 10 3) of every pixel of the image, taps reflected at the edges -> (dx, dy) int64 [h, w]."""
    h, w = img.shape
    p = window(img, -1, -1, w + 2, h + 2)
    left, right, up, down = p[:, :-2], p[:, 2:], p[:-2, :], p[2:, :]
    gx, gy = right - left, down - up
    dx = 3 * gx[:-2] + 10 * gx[1:-1] + 3 * gx[2:]
    dy = 3 * gy[:, :-2] + 10 * gy[:, 1:-1] + 3 * gy[:, 2:]
    return dx, dy


def _weights(fx, fy):
    """14-bit bilinear weights of the fractional position (fx, fy), f32 products rounded half to even (cvRound)."""
    one, s = F32(1.0), F32(1 << W_BITS)
    w00 = int(np.rint((one - fx) * (one - fy) * s))
    w01 = int(np.rint(fx * (one - fy) * s))
    w10 = int(np.rint((one - fx) * fy * s))
    return w00, w01, w10, (1 << W_BITS) - w00 - w01 - w10


def _blend(g, wts, bits):
    """[ch + 1, cw + 1] samples -> [ch, cw] values interpolated with the integer weights, rounded to `bits` fewer bits."""
    w00, w01, w10, w11 = wts
    return descale(g[:-1, :-1] * w00 + g[:-1, 1:] * w01 + g[1:, :-1] * w10 + g[1:, 1:] * w11, bits)


def _isum(a):
    return sum(a.ravel().tolist())          # Python integers: no width to overflow


def _outside(ix, iy, W, H, ww, wh):
    """The window's corner is more than a window outside the level image."""
    return ix < -ww or ix >= W or iy < -wh or iy >= H


def lk_track_point(prev_levels, next_levels, pt, win=(21, 21), max_count=30, eps_sq=1e-4, maps=None):
    """One point of cv2.calcOpticalFlowPyrLK on two pyramids (lists of [h, w] u8, level 0 first).  pt (x, y) in level-0
    pixels, max_count and eps_sq (= epsilon squared) already clamped.  -> ((x, y) f32, status, err f32, path): path has one
    label of LK_LABELS per level, coarsest first; at level 0 '+final_outside' is appended when the position the level
    ended on is more than a window outside the image."""
    ww, wh = win
    nlev = len(prev_levels)
    half_x, half_y = F32(ww - 1) * F32(0.5), F32(wh - 1) * F32(0.5)
    x0, y0 = F32(pt[0]), F32(pt[1])
    status, err = 1, F32(0.0)
    nx = ny = F32(0.0)
    path = []
    for lev in range(nlev - 1, -1, -1):
        I, J = prev_levels[lev], next_levels[lev]
        H, W = I.shape
        scale = F32(1.0) / F32(1 << lev)
        px, py = x0 * scale, y0 * scale
        if lev == nlev - 1:
            nx, ny = px, py
        else:
            nx, ny = nx * F32(2.0), ny * F32(2.0)
        px, py = px - half_x, py - half_y
        ipx, ipy = math.floor(px), math.floor(py)
        if _outside(ipx, ipy, W, H, ww, wh):
            if lev == 0:
                status, err = 0, F32(0.0)
            path.append("start_outside")
            continue
        wts = _weights(px - F32(ipx), py - F32(ipy))
        dxm, dym = maps[lev] if maps is not None else scharr_maps(I)
        Ip = _blend(window(I, ipx, ipy, ww + 1, wh + 1), wts, W_BITS - 5)
        Ix = _blend(window_zero(dxm, ipx, ipy, ww + 1, wh + 1), wts, W_BITS)
        Iy = _blend(window_zero(dym, ipx, ipy, ww + 1, wh + 1), wts, W_BITS)
        scale20 = 1.0 / (1 << 20)
        A11, A12, A22 = _isum(Ix * Ix) * scale20, _isum(Ix * Iy) * scale20, _isum(Iy * Iy) * scale20
        det = A11 * A22 - A12 * A12
        diff = A11 - A22
        min_eig = (A22 + A11 - math.sqrt(diff * diff + 4.0 * (A12 * A12))) / float(2 * ww * wh)
        if min_eig < 1e-4 or det < 2.0 ** -23:
            if lev == 0:
                status = 0
            path.append("rejected")
            continue
        inv = 1.0 / det
        nx, ny = nx - half_x, ny - half_y
        label = "zero_count" if max_count == 0 else "count"
        pdx = pdy = F32(0.0)
        for it in range(max_count):
            inx, iny = math.floor(nx), math.floor(ny)
            if _outside(inx, iny, W, H, ww, wh):
                if lev == 0:
                    status = 0
                label = "left_image"
                break
            Jp = _blend(window(J, inx, iny, ww + 1, wh + 1), _weights(nx - F32(inx), ny - F32(iny)), W_BITS - 5)
            diffp = Jp - Ip
            b1, b2 = _isum(diffp * Ix) * scale20, _isum(diffp * Iy) * scale20
            ddx, ddy = F32((A12 * b2 - A22 * b1) * inv), F32((A12 * b1 - A11 * b2) * inv)
            nx, ny = nx + ddx, ny + ddy
            if float(ddx) * float(ddx) + float(ddy) * float(ddy) <= eps_sq:
                label = "eps"
                break
            if it > 0 and abs(ddx + pdx) < F32(0.01) and abs(ddy + pdy) < F32(0.01):
                nx, ny = nx - ddx * F32(0.5), ny - ddy * F32(0.5)
                label = "half_step"
                break
            pdx, pdy = ddx, ddy
        if lev == 0 and status:
            inx, iny = math.floor(nx), math.floor(ny)
            if _outside(inx, iny, W, H, ww, wh):
                status = 0
                label += "+final_outside"
            else:
                Jp = _blend(window(J, inx, iny, ww + 1, wh + 1), _weights(nx - F32(inx), ny - F32(iny)), W_BITS - 5)
                err = F32(_isum(np.abs(Jp - Ip)) / float(32 * ww * wh))
        path.append(label)
        nx, ny = nx + half_x, ny + half_y
    if not status:
        err = F32(0.0)
    return (nx, ny), status, err, tuple(path)


def lk_track(prev, nxt, pts, win=(21, 21), max_level=3, max_count=30, epsilon=0.01):
    """cv2.calcOpticalFlowPyrLK(prev, nxt, pts, None, winSize=win, maxLevel=max_level, criteria=(3, max_count, epsilon))
    -> (next [n, 2] f32, status [n] u8, err [n] f32, paths [n] tuples)."""
    pp, pn = pyramid(prev, max_level), pyramid(nxt, max_level)
    maps = [scharr_maps(a) for a in pp]
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    count = min(max(int(max_count), 0), 100)
    eps_sq = min(max(float(epsilon), 0.0), 10.0) ** 2
    out, st, err, paths = np.zeros((len(pts), 2), np.float32), np.zeros(len(pts), np.uint8), np.zeros(len(pts), np.float32), []
    for i, p in enumerate(pts):
        out[i], st[i], err[i], path = lk_track_point(pp, pn, p, win, count, eps_sq, maps)
        paths.append(path)
    return out, st, err, paths


# ---- Shi-Tomasi corners -------------------------------------------------------------------------------------------------
def sobel_maps(img):
    h, w = img.shape
    p = window(img, -1, -1, w + 2, h + 2)
    gx, gy = p[:, 2:] - p[:, :-2], p[2:, :] - p[:-2, :]
    return gx[:-2] + 2 * gx[1:-1] + gx[2:], gy[:, :-2] + 2 * gy[:, 1:-1] + gy[:, 2:]


def _box(a, bs, anchor):
    """Sum of `a` over the bs x bs box whose cell `anchor` (both axes) lies on the pixel; `a` continues by reflect-101."""
    h, w = a.shape
    p = window(a, -anchor, -anchor, w + bs - 1, h + bs - 1)
    ii = np.zeros((p.shape[0] + 1, p.shape[1] + 1), I64)
    ii[1:, 1:] = p.cumsum(0).cumsum(1)
    return ii[bs:, bs:] - ii[:-bs, bs:] - ii[bs:, :-bs] + ii[:-bs, :-bs]


def min_eig(img, bs=3):
    """cv2.cornerMinEigenVal(img, bs, 3) on 8-bit input, f64 [h, w]: the box filter's anchor is cell bs // 2, the products
    of the Sobel derivatives continue past the edge by reflection."""
    assert 1 <= bs <= 15
    img = np.asarray(img, np.uint8)
    dx, dy = sobel_maps(img)
    a, b, c = (_box(m, bs, bs // 2) for m in (dx * dx, dx * dy, dy * dy))
    scale = 1.0 / (4.0 * bs * 255.0)
    A, B, C = 0.5 * a.astype(np.float64), b.astype(np.float64), 0.5 * c.astype(np.float64)
    d = A - C
    return ((A + C) - np.sqrt(d * d + B * B)) * (scale * scale)


def corner_candidates(eig, quality):
    """-> (y, x, v) of the candidates in order (v descending, y, x)."""
    h, w = eig.shape
    if h < 3 or w < 3:
        z = np.zeros(0, I64)
        return z, z, np.zeros(0)
    thr = max(float(eig.max()), 0.0) * quality
    kept = np.where(eig > thr, eig, 0.0)
    neigh = np.max([kept[dy:h - 2 + dy, dx:w - 2 + dx] for dy in range(3) for dx in range(3)], axis=0)
    c = kept[1:-1, 1:-1]
    ys, xs = np.nonzero((c != 0.0) & (c == neigh))
    ys, xs = ys + 1, xs + 1
    v = eig[ys, xs]
    order = np.lexsort((xs, ys, -v))
    return ys[order], xs[order], v[order]


def good_features(img, max_corners, quality, min_distance, bs=3, stats=None):
    """cv2.goodFeaturesToTrack -> [n, 2] f32 (x, y).  `stats` (a dict) receives the number of candidates, the size of the
    largest group of exactly equal strength and how many candidates only the distance test rejected."""
    ys, xs, v = corner_candidates(min_eig(img, bs), quality)
    chosen = []
    rejected = 0
    md2 = float(min_distance) * float(min_distance)
    for y, x in zip(ys.tolist(), xs.tolist()):
        if min_distance >= 1 and any((x - cx) ** 2 + (y - cy) ** 2 < md2 for cx, cy in chosen):
            rejected += 1
            continue
        chosen.append((x, y))
        if max_corners > 0 and len(chosen) >= max_corners:
            break
    if stats is not None:
        stats["candidates"] = len(v)
        stats["largest_tie"] = int(np.unique(v, return_counts=True)[1].max()) if len(v) else 0
        stats["distance_rejected"] = rejected
    return np.array(chosen, np.float32).reshape(-1, 2)


# ---- L*a*b* -------------------------------------------------------------------------------------------------------------
# XYZ / white from 12-bit linear sRGB and back, 12-bit fixed point (rows of both sum to 4096: grey stays grey)
RGB_TO_XYZ = np.array([[1777, 1541, 778], [871, 2929, 296], [73, 448, 3575]], I64)
XYZ_TO_RGB = np.array([[12621, -6300, -2225], [-3775, 7686, 185], [215, -834, 4715]], I64)
Q15 = 1 << 15
F_KNEE = 6779                   # f(0.008856) = 6 / 29 in Q15, rounded down: above it f^-1 is the cube
F_ZERO = 4520                   # f(0) = 16 / 116 in Q15
F_SLOPE = 269254                # the linear branch of f^-1, 12-bit result per Q15 unit, in Q24: the definition's constant
#                                 (4095 / (7.787 * 32768) is 269248.7 in Q24; over the branch that is < 0.003 of a 12-bit step)


def _round_div(num, den):
    """num / den rounded to nearest, halves away from zero (den > 0), int64 arrays."""
    return np.sign(num) * ((np.abs(num) + den // 2) // den)


def lab_forward(bgr, tables):
    """[..., 3] u8 BGR -> [..., 3] u8 (L, a, b), integer arithmetic only."""
    gamma, cbrt_tab, _ = tables
    bgr = np.asarray(bgr, np.uint8)
    rgb = gamma.astype(I64)[bgr[..., ::-1]]                                    # 12-bit linear light, R G B
    xyz = np.minimum((rgb @ RGB_TO_XYZ.T + 2048) >> 12, 4095)
    f = cbrt_tab.astype(I64)[xyz]                                             # f(X), f(Y), f(Z) in Q15
    fx, fy, fz = f[..., 0], f[..., 1], f[..., 2]
    num = (116 * fy - 16 * Q15) * 255                                         # L* 255 / 100 over 100 Q15 (never negative)
    assert num.min() >= 0
    L = (num + 50 * Q15) // (100 * Q15)
    a = (500 * (fx - fy) + 128 * Q15 + Q15 // 2) >> 15
    b = (200 * (fy - fz) + 128 * Q15 + Q15 // 2) >> 15
    return np.clip(np.stack([L, a, b], -1), 0, 255).astype(np.uint8)


def lab_inverse(lab, tables):
    """[..., 3] u8 (L, a, b) -> ([..., 3] u8 BGR, counts): counts['finv_low' / 'finv_high'] values of f^-1 clamped to
    0 / 4095, counts['r_low'] ... ['b_high'] linear channel values clamped, counts['linear_pixels'] pixels with at least
    one of X, Y, Z on the linear branch of f^-1."""
    _, _, gamma_inv = tables
    lab = np.asarray(lab, np.uint8).astype(I64)
    L, a, b = lab[..., 0], lab[..., 1], lab[..., 2]
    fy = _round_div((L * 100 + 16 * 255) * Q15, 116 * 255)                    # (L* + 16) / 116
    fx = fy + _round_div((a - 128) * (2 * Q15), 1000)                         # + a* / 500
    fz = fy - _round_div((b - 128) * (Q15 // 2), 100)                         # - b* / 200
    f = np.stack([fx, fy, fz], -1)
    linear = f <= F_KNEE
    t = np.where(linear, ((f - F_ZERO) * F_SLOPE + (1 << 23)) >> 24, (f * f * f * 4095 + (1 << 44)) >> 45)
    counts = {"finv_low": int((t < 0).sum()), "finv_high": int((t > 4095).sum()), "linear_pixels": int(linear.any(-1).sum())}
    xyz = np.clip(t, 0, 4095)
    rgb = (xyz @ XYZ_TO_RGB.T + 2048) >> 12
    for k, name in enumerate("rgb"):
        counts[name + "_low"] = int((rgb[..., k] < 0).sum())
        counts[name + "_high"] = int((rgb[..., k] > 4095).sum())
    out = gamma_inv[np.clip(rgb, 0, 4095)]
    return np.ascontiguousarray(out[..., ::-1]), counts


def lab_float(bgr):
    """CIELAB of 8-bit sRGB in float64, no table: sRGB decode, linear RGB -> XYZ (D65), f(t), scaled like the 8-bit
    encoding (L* 255 / 100, a* + 128, b* + 128) but neither rounded nor clamped.  [..., 3] u8 BGR -> [..., 3] f64."""
    c = np.asarray(bgr, np.uint8)[..., ::-1] / 255.0
    lin = np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)
    m = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])
    xyz = lin @ (m / m.sum(1, keepdims=True)).T                                # / white point: the row sums
    f = np.where(xyz > 0.008856, np.cbrt(xyz), 7.787 * xyz + 16.0 / 116.0)
    fx, fy, fz = f[..., 0], f[..., 1], f[..., 2]
    return np.stack([(116.0 * fy - 16.0) * 2.55, 500.0 * (fx - fy) + 128.0, 200.0 * (fy - fz) + 128.0], -1)


# ---- CLAHE --------------------------------------------------------------------------------------------------------------
def clahe_luts(plane, clip, tiles):
    """-> (lut [ty, tx, 256] u8, tw, th)."""
    h, w = plane.shape
    tx, ty = tiles
    tw, th = -(-w // tx), -(-h // ty)
    area = tw * th
    padded = window(plane, 0, 0, tx * tw, ty * th)                            # reflected to a multiple of the grid
    limit = max(int(clip * area / 256.0), 1)
    scale = F32(255.0) / F32(area)
    lut = np.zeros((ty, tx, 256), np.uint8)
    for j in range(ty):
        for i in range(tx):
            hist = np.bincount(padded[j * th:(j + 1) * th, i * tw:(i + 1) * tw].ravel(), minlength=256)
            excess = int(np.maximum(hist - limit, 0).sum())
            hist = np.minimum(hist, limit) + excess // 256
            residual = excess % 256
            if residual:
                step = max(256 // residual, 1)
                hist[np.arange(0, 256, step)[:residual]] += 1                # bins 0, step, 2 step, ...: `residual` of them, below 256
            lut[j, i] = np.clip(np.rint(np.cumsum(hist).astype(F32) * scale), 0, 255).astype(np.uint8)
    return lut, tw, th


def _tile_blend(n, size, count):
    """Along one axis: for pixel 0..n-1 the two tile indices and the f32 weights of the blend."""
    t = np.arange(n).astype(F32) * (F32(1.0) / F32(size)) - F32(0.5)
    lo = np.floor(t)
    w_hi = t - lo
    w_lo = F32(1.0) - w_hi
    lo = lo.astype(I64)
    return np.maximum(lo, 0), np.minimum(lo + 1, count - 1), w_lo.astype(F32), w_hi.astype(F32)


def clahe(plane, clip=3.5, tiles=(8, 8)):
    """cv2.createCLAHE(clip, tiles).apply(plane) on an 8-bit plane."""
    plane = np.asarray(plane, np.uint8)
    h, w = plane.shape
    lut, tw, th = clahe_luts(plane, clip, tiles)
    x1, x2, xa1, xa = _tile_blend(w, tw, tiles[0])
    y1, y2, ya1, ya = _tile_blend(h, th, tiles[1])
    Y1, Y2, X1, X2 = y1[:, None], y2[:, None], x1[None, :], x2[None, :]
    xa1, xa, ya1, ya = xa1[None, :], xa[None, :], ya1[:, None], ya[:, None]
    top = lut[Y1, X1, plane].astype(F32) * xa1 + lut[Y1, X2, plane].astype(F32) * xa
    bottom = lut[Y2, X1, plane].astype(F32) * xa1 + lut[Y2, X2, plane].astype(F32) * xa
    return np.clip(np.rint(top * ya1 + bottom * ya), 0, 255).astype(np.uint8)


def increase_contrast(bgr, tables, clip=3.5, tiles=(8, 8), counts=None):
    """BGR -> L*a*b* -> CLAHE on L -> BGR.  `counts` (a dict) receives lab_inverse's counts."""
    lab = lab_forward(bgr, tables).copy()
    lab[..., 0] = clahe(lab[..., 0], clip, tiles)
    out, c = lab_inverse(lab, tables)
    if counts is not None:
        counts.update(c)
    return out


def grey(bgr):
    """cv2.COLOR_BGR2GRAY on 8-bit input: 14-bit weights, rounded."""
    v = np.asarray(bgr, np.uint8).astype(I64) @ np.array([1868, 9617, 4899], I64)
    return ((v + 8192) >> 14).astype(np.uint8)
