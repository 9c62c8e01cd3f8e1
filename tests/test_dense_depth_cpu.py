"""CPU: the NumPy restatement of mm_depth_sweep and mm_depth_fuse (include/meatmodeler.h, a-9c), its fixtures, its accuracy
against the analytic depth of the synthetic scene, and the plan rules of `run(dense=...)` -- no device.

The restatement follows the header operation by operation, f32 where it says f32, vectorised over pixels; `tables` is the host
table code with Python floats (IEEE doubles, one operation at a time) and must give the bits of ops.sweep_tables.  The sweep
keeps the whole cost volume and picks the winner with argmin -- not the running best the kernel keeps in registers.

Margins: a fuse fixture is usable by the GPU file only if no comparison of the fuse lies within 1e-9 (relative to its
threshold; absolute for the sign of a depth and for the distance of a projection from the next half pixel, where rint turns)
of flipping: `margins_hold`.  The GPU must then give the same bits anyway -- the arithmetic is the same -- but a fixture that
sits on a threshold would turn a one-ulp difference into a different cloud instead of a different bit.

Accuracy of the committed restatement on the 7-frame scene (160 x 120, arc 35 degrees, views 1 .. 5, range 4 .. 14, 64 planes,
r = 3, defaults otherwise), relative error of a depth against the ray-cast's: see ACCURACY below, measured values in the
comments beside the floors.
"""
import functools
import math

import numpy as np
import pytest

from meatmodeler_amd import synth

f32 = np.float32
CHUNK = 1024      # MM_FILTER_CHUNK: pixels per chunk of the compaction's scan


# ------------------------------------------------------------------------------------------------ host tables

def tables(K, ext, ref, src, ranges, D):
    """AB [V, S, 12], w0 [V], dw [V] as the header defines them, one Python float operation at a time."""
    K = [float(x) for x in np.asarray(K, np.float64).reshape(9)]
    fx, sk, cx, fy, cy = K[0], K[1], K[2], K[4], K[5]
    ext = np.asarray(ext, np.float64)
    V, S = len(ref), np.asarray(src).shape[1]
    AB, w0, dw = np.zeros((V, S, 12)), np.zeros(V), np.zeros(V)
    for v in range(V):
        Er = ext[int(ref[v])].tolist()
        dmin, dmax = float(ranges[v][0]), float(ranges[v][1])
        w0[v] = 1.0 / dmin
        dw[v] = (1.0 / dmax - 1.0 / dmin) / float(D - 1) if D > 1 else 0.0
        for s in range(S):
            if src[v][s] < 0:
                continue
            Es = ext[int(src[v][s])].tolist()
            R = [[(Es[i][0] * Er[j][0] + Es[i][1] * Er[j][1]) + Es[i][2] * Er[j][2] for j in range(3)] for i in range(3)]
            t = [Es[i][3] - ((R[i][0] * Er[0][3] + R[i][1] * Er[1][3]) + R[i][2] * Er[2][3]) for i in range(3)]
            for i in range(3):
                M = [(K[3 * i] * R[0][j] + K[3 * i + 1] * R[1][j]) + K[3 * i + 2] * R[2][j] for j in range(3)]
                a0 = M[0] / fx
                a1 = (M[1] - sk * a0) / fy
                AB[v, s, 3 * i:3 * i + 3] = a0, a1, (M[2] - cx * a0) - cy * a1
                AB[v, s, 9 + i] = (K[3 * i] * t[0] + K[3 * i + 1] * t[1]) + K[3 * i + 2] * t[2]
    return AB, w0, dw


# ------------------------------------------------------------------------------------------------ sweep

def window_sums(a, r):
    """Row-major sequential f32 sums over the (2r+1)^2 window of every interior pixel."""
    H, W = a.shape
    out = np.zeros((H - 2 * r, W - 2 * r), f32)
    for dv in range(2 * r + 1):
        for du in range(2 * r + 1):
            out = out + a[dv:dv + H - 2 * r, du:du + W - 2 * r]
    return out


def centred(a, mean, r):
    """[n] list of (window value - mean) per interior pixel, row-major."""
    H, W = a.shape
    return [a[dv:dv + H - 2 * r, du:du + W - 2 * r] - mean for dv in range(2 * r + 1) for du in range(2 * r + 1)]


def sums_of_products(xs, ys):
    out = np.zeros_like(xs[0])
    for x, y in zip(xs, ys):
        out = out + x * y
    return out


def warp_sample(img_s, ab, wk, H, W):
    """The warped image of one (source, plane): f32 [H, W], NaN where the warp is invalid."""
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    with np.errstate(all="ignore"):
        c = [ab[2] + wk * ab[9], ab[5] + wk * ab[10], ab[8] + wk * ab[11]]
        p = [(ab[3 * i] * u + ab[3 * i + 1] * v) + c[i] for i in range(3)]
        xs, ys = p[0] / p[2], p[1] / p[2]
        valid = (p[2] > 0) & (xs >= 0) & (xs <= W - 1) & (ys >= 0) & (ys <= H - 1)
        x0 = np.minimum(np.floor(xs), W - 2.0)
        y0 = np.minimum(np.floor(ys), H - 2.0)
        fx, fy = (xs - x0).astype(f32), (ys - y0).astype(f32)
    xi, yi = np.where(valid, x0, 0).astype(np.int64), np.where(valid, y0, 0).astype(np.int64)
    fx, fy = np.where(valid, fx, f32(0)), np.where(valid, fy, f32(0))
    g = img_s.astype(f32)
    s00, s01, s10, s11 = g[yi, xi], g[yi, xi + 1], g[yi + 1, xi], g[yi + 1, xi + 1]
    top = s00 + fx * (s01 - s00)
    bot = s10 + fx * (s11 - s10)
    val = top + fy * (bot - top)
    assert val.dtype == f32
    return np.where(valid, val, f32(np.nan))


def sweep_view(img, ab, w0, dw, ref, src, D, r, var_min, min_sources):
    """One view of `sweep`: ab [S, 12], w0, dw, ref scalars, src [S] -> (depth, cost [H, W] f32, plane [H, W] i32)."""
    _, H, W = img.shape
    n = (2 * r + 1) ** 2
    nf, thr = f32(n), f32(var_min) * f32(n)
    depth, cost, plane = np.full((H, W), np.nan, f32), np.full((H, W), np.nan, f32), np.full((H, W), -1, np.int32)
    if H <= 2 * r or W <= 2 * r:
        return depth, cost, plane
    a = img[ref].astype(f32)
    ca = centred(a, window_sums(a, r) / nf, r)
    saa = sums_of_products(ca, ca)
    ref_ok = saa > thr
    vol = np.full((D,) + saa.shape, np.nan, f32)
    for k in range(D):
        wk = w0 + float(k) * dw
        acc, cnt = np.zeros_like(saa), np.zeros(saa.shape, np.int32)
        for s in range(len(src)):
            if src[s] < 0:
                continue
            b = warp_sample(img[src[s]], ab[s], wk, H, W)
            with np.errstate(all="ignore"):
                cb = centred(b, window_sums(b, r) / nf, r)
                sbb = sums_of_products(cb, cb)
                sab = sums_of_products(ca, cb)
                counts = ref_ok & (sbb > thr)              # (NaN, a window with an invalid sample, compares false)
                cs = f32(1) - sab / np.sqrt(saa * sbb)
            assert cs.dtype == f32
            acc = acc + np.where(counts, cs, f32(0))
            cnt = cnt + counts
        with np.errstate(all="ignore"):
            vol[k] = np.where(cnt >= min_sources, acc / cnt.astype(f32), f32(np.nan))
    any_valid = ~np.isnan(vol).all(0)
    k0 = np.argmin(np.where(np.isnan(vol), f32(np.inf), vol), 0)          # (the first of equal minima)
    take = lambda kk: np.take_along_axis(vol, np.clip(kk, 0, D - 1)[None], 0)[0].astype(np.float64)
    c0, cm, cp = take(k0), take(k0 - 1), take(k0 + 1)
    with np.errstate(all="ignore"):
        den = (cm - 2.0 * c0) + cp
        step = (k0 > 0) & (k0 < D - 1) & ~np.isnan(cm) & ~np.isnan(cp) & (den > 0)
        delta = np.where(step, np.clip((cm - cp) / (2.0 * den), -0.5, 0.5), 0.0)
        d = (1.0 / (w0 + (k0.astype(np.float64) + delta) * dw)).astype(f32)
    inner = (slice(r, H - r), slice(r, W - r))
    depth[inner] = np.where(any_valid, d, f32(np.nan))
    cost[inner] = np.where(any_valid, c0.astype(f32), f32(np.nan))
    plane[inner] = np.where(any_valid, k0, -1)
    return depth, cost, plane


def sweep(img, AB, w0, dw, ref, src, D, r, var_min=4.0, min_sources=1):
    """mm_depth_sweep restated -> (depth, cost [V, H, W] f32, plane [V, H, W] i32)."""
    img, src = np.asarray(img), np.asarray(src)
    _, H, W = img.shape
    maps = [sweep_view(img, AB[v], float(w0[v]), float(dw[v]), int(ref[v]), src[v], D, r, var_min, min_sources) for v in range(len(ref))]
    return tuple(np.stack([m[i] for m in maps]) if maps else np.zeros((0, H, W), t) for i, t in enumerate((f32, f32, np.int32)))


# ------------------------------------------------------------------------------------------------ fuse

def lift(K, e, u, v, d):
    fx, sk, cx, fy, cy = K[0], K[1], K[2], K[4], K[5]
    yn = (v - cy) / fy
    xn = ((u - cx) - sk * yn) / fx
    a = [d * xn - e[0, 3], d * yn - e[1, 3], d - e[2, 3]]
    return [(e[0, j] * a[0] + e[1, j] * a[1]) + e[2, j] * a[2] for j in range(3)]


def project(K, e, X):
    Y = [((e[i, 0] * X[0] + e[i, 1] * X[1]) + e[i, 2] * X[2]) + e[i, 3] for i in range(3)]
    px = ((K[0] * Y[0] + K[1] * Y[1]) + K[2] * Y[2]) / Y[2]
    py = (K[4] * Y[1] + K[5] * Y[2]) / Y[2]
    return Y, px, py


def fuse(depth, cost, K, ext, nbr, grey, max_cost=0.4, eps_depth=0.01, tau_px=1.0, min_consistent=2, cap=None):
    """mm_depth_fuse restated -> dict(points, grey, origin, n_consistent, keep, counts, n, margin): margin = the smallest
    distance of any comparison from flipping, in the units of the module docstring."""
    K = np.asarray(K, np.float64).reshape(9)
    ext = np.asarray(ext, np.float64)[:, :3, :]
    nbr = np.asarray(nbr).reshape(len(ext), -1)
    V, H, W = depth.shape
    d64, c64 = depth.astype(np.float64), cost.astype(np.float64)
    with np.errstate(invalid="ignore"):
        cand = np.isfinite(d64) & (c64 <= max_cost)
    margin = [math.inf]

    def note(values, scale=1.0):
        values = np.asarray(values, np.float64)
        values = values[np.isfinite(values)]
        if values.size and scale > 0:
            margin[0] = min(margin[0], float(np.abs(values).min()) / scale)

    note(c64[np.isfinite(d64)] - max_cost, abs(max_cost) if max_cost else 1.0)
    keep = np.zeros((V, H, W), np.uint8)
    agree = np.zeros((V, H, W), np.int32)
    Xw_all = np.full((V, H, W, 3), np.nan)
    vv, uu = np.mgrid[0:H, 0:W].astype(np.float64)
    for i in range(V):
        m = cand[i]
        u, v, d = uu[m], vv[m], d64[i][m]
        Xw = lift(K, ext[i], u, v, d)
        n_ok = np.zeros(u.size, np.int32)
        for q in nbr[i]:
            if q < 0:
                continue
            with np.errstate(all="ignore"):
                Y, px, py = project(K, ext[q], Xw)
                ok = Y[2] > 0
                note(Y[2])
                xi, yi = np.rint(px), np.rint(py)
                note(np.abs(px[ok] - np.floor(px[ok]) - 0.5))
                note(np.abs(py[ok] - np.floor(py[ok]) - 0.5))
                ok &= (xi >= 0) & (xi <= W - 1) & (yi >= 0) & (yi <= H - 1)
                xq, yq = np.where(ok, xi, 0).astype(np.int64), np.where(ok, yi, 0).astype(np.int64)
                ok &= cand[q][yq, xq]
                dq = d64[q][yq, xq]
                note((np.abs(dq - Y[2]) - eps_depth * Y[2])[ok], 1.0)
                note(((np.abs(dq - Y[2]) - eps_depth * Y[2]) / (eps_depth * Y[2]))[ok] if eps_depth > 0 else [])
                ok &= np.abs(dq - Y[2]) <= eps_depth * Y[2]
                Z, bx, by = project(K, ext[i], lift(K, ext[q], xi, yi, dq))
                note(Z[2][ok])
                ok &= Z[2] > 0
                dx, dy = bx - u, by - v
                dist = np.sqrt(dx * dx + dy * dy)
                note((dist - tau_px)[ok], tau_px if tau_px > 0 else 1.0)
                ok &= dist <= tau_px
            n_ok += ok
        keep[i][m] = n_ok >= min_consistent
        agree[i][m] = n_ok
        Xw_all[i][m] = np.stack(Xw, -1)
    sel = keep.astype(bool)
    vi, yi, xi = np.nonzero(sel)                                    # (view, row, column) order
    kept = int(sel.sum())
    n = kept if cap is None else min(kept, int(cap))
    return dict(points=Xw_all[sel][:n], grey=np.asarray(grey)[sel][:n], origin=np.stack([vi, yi * W + xi], 1).astype(np.int32)[:n],
                n_consistent=agree[sel][:n], keep=keep, counts=(kept, int(cand.sum())), n=n, margin=margin[0])


def margins_hold(fused):
    """The margin condition of the module docstring on a restated fuse."""
    return fused["margin"] >= 1e-9


# ------------------------------------------------------------------------------------------------ fixtures

def view_tables(n_frames, every=1, sources=4, gap=1, neighbours=4, first=0, last=None):
    """ref, src, nbr of pipeline.dense_views restricted to the views first .. last of the view list (nbr renumbered)."""
    from meatmodeler_amd.pipeline import dense_views
    ref, src, nbr = dense_views(n_frames, every, sources, gap, neighbours)
    last = ref.size - 1 if last is None else last
    nbr = np.where((nbr >= first) & (nbr <= last), nbr - first, -1).astype(np.int32)
    return ref[first:last + 1], src[first:last + 1], nbr[first:last + 1]


SCENE = dict(n_frames=7, width=160, height=120, arc_deg=35.0, dmin=4.0, dmax=14.0, planes=64, radius=3)


@functools.lru_cache(maxsize=None)
def scene():
    """The 7-frame scene of the issue: frames, cameras, the tables of views 1 .. 5, the restated maps and the restated cloud
    under the defaults of ops.depth_fuse (max_cost 0.4, eps_depth 0.01, tau_px 1, min_consistent 2), the analytic depth."""
    from meatmodeler_amd import ops
    s = SCENE
    frames, ext, K = synth.render_orbit_frames(s["n_frames"], s["width"], s["height"], arc_deg=s["arc_deg"])
    ref, src, nbr = view_tables(s["n_frames"], first=1, last=5)
    ranges = np.tile([[s["dmin"], s["dmax"]]], (ref.size, 1))
    AB, w0, dw = ops.sweep_tables(K, ext, ref, src, ranges, s["planes"])
    depth, cost, plane = sweep(frames, AB, w0, dw, ref, src, s["planes"], s["radius"])
    fused = fuse(depth, cost, K, ext[ref], nbr, frames[ref])
    truth = np.stack([synth.render_depth(ext[f], K, s["width"], s["height"]) for f in ref])
    return dict(frames=frames, ext=ext, K=K, ref=ref, src=src, nbr=nbr, ranges=ranges, AB=AB, w0=w0, dw=dw, depth=depth, cost=cost,
                plane=plane, fused=fused, truth=truth)


@functools.lru_cache(maxsize=None)
def small_scene(width=57, height=44, n_frames=5, planes=17, radius=2, seed=7):
    """A scene small enough for many shapes: 5 frames, every frame a view, two source slots at +-1, two neighbours."""
    frames, ext, K = synth.render_orbit_frames(n_frames, width, height, arc_deg=20.0, seed=seed, tex_size=512)
    ref, src, nbr = view_tables(n_frames, sources=2, neighbours=2)
    ranges = np.tile([[4.0, 14.0]], (ref.size, 1))
    return dict(frames=frames, ext=ext, K=K, ref=ref, src=src, nbr=nbr, ranges=ranges, planes=planes, radius=radius)


def errors(depth, truth, mask):
    with np.errstate(all="ignore"):
        rel = np.abs(depth.astype(np.float64) - truth) / truth
    rel = rel[mask & np.isfinite(truth)]
    return dict(within5=float((rel <= 0.05).mean()), within2=float((rel <= 0.02).mean()), median=float(np.median(rel)), n=int(rel.size))


# measured on the committed restatement (test_accuracy_against_the_analytic_depth prints them): the floors are the measured
# shares rounded down to two decimals, the ceilings of the medians the measured values rounded up to three
ACCURACY = dict(raw=dict(within5=0.75, within2=0.51, median=0.020),          # measured 0.7582, 0.5161, 0.01921 (view 3, 12497 pixels)
                fused=dict(within5=0.98, within2=0.75, median=0.011),        # measured 0.9827, 0.7514, 0.01056 (26323 points)
                share=0.27)                                                  # measured 0.2747 of the pixels of views 1 .. 5


# ------------------------------------------------------------------------------------------------ tests

def test_ops_and_the_restatement_build_the_same_tables():
    from meatmodeler_amd import ops
    sc = scene()
    AB, w0, dw = tables(sc["K"], sc["ext"], sc["ref"], sc["src"], sc["ranges"], SCENE["planes"])
    assert AB.tobytes() == sc["AB"].tobytes() and w0.tobytes() == sc["w0"].tobytes() and dw.tobytes() == sc["dw"].tobytes()
    # a K with skew, one plane, a padded source row, a view list out of order
    K = np.array([[410.0, 1.5, 81.25], [0.0, 395.0, 58.5], [0.0, 0.0, 1.0]])
    ref, src = np.array([4, 0, 2]), np.array([[3, -1, 5], [-1, 1, 2], [6, 0, -1]])
    rng = np.array([[3.0, 9.0], [2.5, 2.5], [4.0, 40.0]])
    for D in (1, 2, 33):
        a = ops.sweep_tables(K, sc["ext"], ref, src, rng, D)
        b = tables(K, sc["ext"], ref, src, rng, D)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
        assert (a[0][src < 0] == 0).all() and (a[2] == 0).all() == (D == 1)
    # the homography of plane k maps a reference pixel where the point at that depth projects in the source
    AB, w0, dw = ops.sweep_tables(sc["K"], sc["ext"], [2], [[3]], [[5.0, 9.0]], 5)
    u, v, k = 70.0, 50.0, 3
    d = 1.0 / (w0[0] + k * dw[0])
    Er, Es = sc["ext"][2], sc["ext"][3]
    Xw = Er[:, :3].T @ (d * np.linalg.solve(sc["K"], [u, v, 1.0]) - Er[:, 3])
    want = sc["K"] @ (Es[:, :3] @ Xw + Es[:, 3])
    ab = AB[0, 0]
    p = [ab[3 * i] * u + ab[3 * i + 1] * v + ab[3 * i + 2] + (w0[0] + k * dw[0]) * ab[9 + i] for i in range(3)]
    assert np.allclose([p[0] / p[2], p[1] / p[2]], want[:2] / want[2], rtol=0, atol=1e-9)


def test_sweep_tables_refuse_bad_input():
    from meatmodeler_amd import ops
    sc = scene()
    good = dict(K=sc["K"], extrinsics=sc["ext"], ref=[1], src=[[0, 2]], ranges=[[4.0, 14.0]], planes=8)
    ops.sweep_tables(**good)
    for bad in (dict(K=np.eye(3) * 2), dict(ref=[7]), dict(ref=[-1]), dict(src=[[0, 7]]), dict(src=[[-2, 1]]), dict(src=[0, 2]),
                dict(ranges=[[0.0, 5.0]]), dict(ranges=[[5.0, 4.0]]), dict(ranges=[[4.0, math.inf]]), dict(ranges=[[4.0, math.nan]]),
                dict(ranges=[[4.0, 14.0], [4.0, 14.0]]), dict(planes=0), dict(extrinsics=sc["ext"][:, :, :3])):
        with pytest.raises(ValueError):
            ops.sweep_tables(**dict(good, **bad))


def test_render_depth_is_the_depth_of_the_rendered_surface():
    sc = scene()
    s = SCENE
    d = synth.render_depth(sc["ext"][3], sc["K"], s["width"], s["height"])
    assert d.shape == (s["height"], s["width"]) and np.isnan(d).any() and np.nanmin(d) > 4.0
    # the ellipsoid's nearest point is near the image centre, about radius - 2 away; the ground (the top rows: y points down
    # and the camera is below it) recedes towards the horizon, and beyond the horizon there is nothing
    assert 4.5 < d[s["height"] // 2, s["width"] // 2] < 5.5 and d[0, 5] < d[40, 5] < d[80, 5] and np.isnan(d[-1]).all()
    # a point lifted with this depth lies on the ellipsoid or on the ground
    E, K = sc["ext"][3], sc["K"]
    for (v, u) in ((60, 80), (10, 20), (75, 140)):
        X = E[:, :3].T @ (d[v, u] * np.linalg.solve(K, [u, v, 1.0]) - E[:, 3])
        on_e = abs((X[0] / 2.0) ** 2 + (X[1] / 1.4) ** 2 + (X[2] / 2.0) ** 2 - 1.0) < 1e-9
        assert on_e or abs(X[1] - 1.4) < 1e-9


@functools.lru_cache(maxsize=None)
def planted_sweeps():
    """name -> dict(frames, K, ext, ref, src, ranges, D, r, kw): the planted sweeps, which the GPU file repeats."""
    sm = small_scene()
    fr, ext, K = sm["frames"], sm["ext"], sm["K"]
    out = {}

    def add(name, frames, e, ref, src, **kw):
        out[name] = dict(frames=frames, K=K, ext=e, ref=np.asarray(ref), src=np.asarray(src), ranges=np.tile([[4.0, 14.0]], (len(ref), 1)),
                         D=sm["planes"], r=sm["radius"], kw=kw)

    # a source equal to the reference (same image, same pose, t = 0): every plane ties
    add("twin", np.stack([fr[2], fr[2]]), np.stack([ext[2], ext[2]]), [0], [[1]])
    # a source turned away (half a turn about its own y axis): nothing warps validly
    away = ext[3].copy()
    away[:, :3], away[:, 3] = np.diag([-1.0, 1.0, -1.0]) @ ext[3][:, :3], np.diag([-1.0, 1.0, -1.0]) @ ext[3][:, 3]
    add("turned_away", fr, np.stack([ext[0], ext[1], ext[2], away, ext[4]]), [2], [[3]])
    # a source turned 1.35 rad sideways: p_2 <= 0 on a part of the image
    c, s_ = math.cos(1.35), math.sin(1.35)
    Ry = np.array([[c, 0.0, s_], [0.0, 1.0, 0.0], [-s_, 0.0, c]])
    side = np.hstack([Ry @ ext[3][:, :3], (Ry @ ext[3][:, 3])[:, None]])
    add("behind_on_a_part", np.stack([fr[2], fr[3]]), np.stack([ext[2], side]), [0], [[1]])
    # a constant image: untextured
    add("constant", np.full_like(fr, 90), ext, [2], [[1, 3]])
    add("one_source_is_enough", fr, ext, [2], [[1, 3]])
    add("both_sources_needed", fr, ext, [2], [[1, 3]], min_sources=2)
    return out


def restate_sweep(case):
    from meatmodeler_amd import ops
    AB, w0, dw = ops.sweep_tables(case["K"], case["ext"], case["ref"], case["src"], case["ranges"], case["D"])
    return sweep(case["frames"], AB, w0, dw, case["ref"], case["src"], case["D"], case["r"], **case["kw"]), (AB, w0, dw)


def test_the_planted_cases_of_the_sweep():
    cases = planted_sweeps()
    r = cases["twin"]["r"]
    H, W = cases["twin"]["frames"].shape[1:]
    (depth, cost, plane), _ = restate_sweep(cases["twin"])
    inner = (0, slice(r, H - r), slice(r, W - r))
    textured = ~np.isnan(cost[inner])
    # every plane ties at cost 0 -> plane 0, delta 0, depth dmin
    assert textured.mean() > 0.5 and (plane[inner][textured] == 0).all() and (depth[inner][textured] == f32(4.0)).all()
    assert np.abs(cost[inner][textured]).max() < 1e-6
    assert np.isnan(depth[0, :r]).all() and np.isnan(depth[0, :, W - r:]).all() and (plane[0, H - r:] == -1).all()
    (depth, cost, plane), _ = restate_sweep(cases["turned_away"])
    assert np.isnan(depth).all() and np.isnan(cost).all() and (plane == -1).all()
    (depth, cost, plane), (AB, w0, dw) = restate_sweep(cases["behind_on_a_part"])
    vv, uu = np.mgrid[0:H, 0:W].astype(np.float64)
    p2 = (AB[0, 0, 6] * uu + AB[0, 0, 7] * vv) + (AB[0, 0, 8] + w0[0] * AB[0, 0, 11])
    assert (p2 <= 0).any() and (p2 > 0).any()
    (depth, cost, plane), _ = restate_sweep(cases["constant"])
    assert np.isnan(depth).all() and (plane == -1).all()
    # min_sources = 2 keeps no more pixels than min_sources = 1
    one, two = restate_sweep(cases["one_source_is_enough"])[0], restate_sweep(cases["both_sources_needed"])[0]
    assert 0 < (~np.isnan(two[0])).sum() <= (~np.isnan(one[0])).sum()


def test_a_views_map_does_not_depend_on_the_views_beside_it():
    sm = small_scene()
    from meatmodeler_amd import ops
    AB, w0, dw = ops.sweep_tables(sm["K"], sm["ext"], sm["ref"], sm["src"], sm["ranges"], sm["planes"])
    whole = sweep(sm["frames"], AB, w0, dw, sm["ref"], sm["src"], sm["planes"], sm["radius"])
    for v in (0, 3):
        alone = sweep(sm["frames"], AB[v:v + 1], w0[v:v + 1], dw[v:v + 1], sm["ref"][v:v + 1], sm["src"][v:v + 1], sm["planes"], sm["radius"])
        assert all(a[0].tobytes() == b[v].tobytes() for a, b in zip(alone, whole))


def test_accuracy_against_the_analytic_depth():
    sc = scene()
    fused, truth, depth = sc["fused"], sc["truth"], sc["depth"]
    raw = errors(depth[2], truth[2], ~np.isnan(depth[2]))                     # view 3 of the clip alone
    kept = fused["keep"].astype(bool)
    fu = errors(depth, truth, kept)
    share = kept.mean()
    print(f"raw winner, view 3: within 5 % {raw['within5']:.4f}, within 2 % {raw['within2']:.4f}, median {raw['median']:.4g} "
          f"({raw['n']} pixels); fused: within 5 % {fu['within5']:.4f}, within 2 % {fu['within2']:.4f}, median {fu['median']:.4g} "
          f"({fu['n']} points, {share:.4f} of the pixels); candidates {fused['counts'][1]}")
    a = ACCURACY
    assert raw["within5"] >= a["raw"]["within5"] and raw["within2"] >= a["raw"]["within2"] and raw["median"] <= a["raw"]["median"]
    assert fu["within5"] >= a["fused"]["within5"] and fu["within2"] >= a["fused"]["within2"] and fu["median"] <= a["fused"]["median"]
    assert share >= a["share"]
    assert fu["within5"] > raw["within5"]                                      # fusion raises the 5 % share over the raw winner
    assert fused["counts"][0] == fused["n"] == kept.sum() and fused["counts"][1] >= fused["n"]


def test_the_fuse_fixtures_keep_their_margins():
    assert margins_hold(scene()["fused"])
    for fx in fuse_fixtures().values():
        assert margins_hold(fx["want"]), fx["name"]


@functools.lru_cache(maxsize=None)
def fuse_fixtures():
    """The fuse calls the GPU file repeats, on the maps of small_scene: name -> dict(args of `fuse`, want = its result)."""
    from meatmodeler_amd import ops
    sm = small_scene()
    AB, w0, dw = ops.sweep_tables(sm["K"], sm["ext"], sm["ref"], sm["src"], sm["ranges"], sm["planes"])
    depth, cost, _ = sweep(sm["frames"], AB, w0, dw, sm["ref"], sm["src"], sm["planes"], sm["radius"])
    K, ext, grey = sm["K"], sm["ext"][sm["ref"]], sm["frames"][sm["ref"]]
    out = {}

    def add(name, views, nbr, **kw):
        v = list(views)
        a = dict(depth=depth[v], cost=cost[v], K=K, ext=ext[v], nbr=np.asarray(nbr, np.int32), grey=grey[v], **kw)
        out[name] = dict(name=name, args=a, want=fuse(**a))

    three = [[1, 2], [0, 2], [1, 0]]
    add("three_views", (0, 1, 2), three, eps_depth=0.02, tau_px=1.5, min_consistent=1)
    kept = out["three_views"]["want"]["counts"][0]
    chunks = np.unique(np.flatnonzero(out["three_views"]["want"]["keep"]) // CHUNK)
    assert chunks.size >= 6 and (np.diff(chunks) == 1).sum() >= 4     # (the kept pixels straddle the scan's chunk boundaries)
    for name, cap in (("cap_below", kept - 7), ("cap_equal", kept), ("cap_above", kept + 5), ("cap_zero", 0)):
        add(name, (0, 1, 2), three, eps_depth=0.02, tau_px=1.5, min_consistent=1, cap=cap)
    add("five_views", range(5), sm["nbr"], eps_depth=0.02, tau_px=1.5, min_consistent=2)
    add("one_view_nothing_kept", (2,), [[-1, -1]], min_consistent=1)
    add("one_view_everything_kept", (2,), [[-1, -1]], min_consistent=0, max_cost=2.5)
    add("nothing_is_a_candidate", (0, 1, 2), three, max_cost=-1.0, min_consistent=0)
    add("no_neighbour_table", (0, 1), np.zeros((2, 0)), min_consistent=0)
    add("strict", (0, 1, 2), three, eps_depth=0.0, tau_px=0.0, min_consistent=2)
    # more chunk sums than the one workgroup that scans them takes in a step (256): two views of 400 x 340 pixels with the
    # analytic depth of the scene as their maps (no sweep: the fuse takes any maps), the second one with a band of bad cost
    W, H = 400, 340
    K2, e2 = synth.default_K(W, H, f=525.0 * W / 640.0), synth.orbit_cameras(2, arc_deg=8.0, radius=7.0, height=-2.0)
    d2 = np.stack([synth.render_depth(e, K2, W, H) for e in e2]).astype(f32)
    c2 = np.zeros_like(d2)
    c2[1, 100:140] = 0.9
    g2 = (np.arange(2 * H * W, dtype=np.int64) % 251).astype(np.uint8).reshape(2, H, W)
    a = dict(depth=d2, cost=c2, K=K2, ext=e2, nbr=np.array([[1], [0]], np.int32), grey=g2, eps_depth=0.01, tau_px=1.0, min_consistent=1)
    out["second_scan_level"] = dict(name="second_scan_level", args=a, want=fuse(**a))
    assert 2 * H * W > 256 * CHUNK and out["second_scan_level"]["want"]["counts"][0] > 100000
    return out


def test_the_fuse_restatement_on_its_fixtures():
    fxs = fuse_fixtures()
    a = fxs["three_views"]["want"]
    assert 0 < a["counts"][0] < a["counts"][1] and a["n"] == a["counts"][0]
    o = a["origin"]
    order = o[:, 0].astype(np.int64) * (1 << 32) + o[:, 1]
    assert (np.diff(order) > 0).all()                                 # (view, row, column) order, no pixel twice
    assert a["n_consistent"].min() >= 1 and a["n_consistent"].max() <= 2
    for name in ("cap_below", "cap_equal", "cap_above"):
        w = fxs[name]["want"]
        assert w["counts"] == a["counts"] and w["n"] == min(a["n"], fxs[name]["args"]["cap"])
        assert w["points"].tobytes() == a["points"][:w["n"]].tobytes() and np.array_equal(w["keep"], a["keep"])
    assert fxs["cap_zero"]["want"]["n"] == 0 and fxs["cap_zero"]["want"]["counts"] == a["counts"]
    assert fxs["one_view_nothing_kept"]["want"]["counts"][0] == 0 and fxs["one_view_nothing_kept"]["want"]["counts"][1] > 0
    e = fxs["one_view_everything_kept"]["want"]
    assert e["counts"][0] == e["counts"][1] == int(np.isfinite(fxs["one_view_everything_kept"]["args"]["depth"]).sum()) > 0
    assert fxs["nothing_is_a_candidate"]["want"]["counts"] == (0, 0)
    assert fxs["strict"]["want"]["counts"][0] == 0
    # every kept point projects back onto its own pixel
    sm = small_scene()
    W = sm["frames"].shape[2]
    for row in range(0, a["n"], 97):
        E = sm["ext"][sm["ref"]][o[row, 0]]
        x = sm["K"] @ (E[:, :3] @ a["points"][row] + E[:, 3])
        assert np.allclose(x[:2] / x[2], [o[row, 1] % W, o[row, 1] // W], rtol=0, atol=1e-8)


# ------------------------------------------------------------------------------------------------ the plan

DENSE_RULES = [
    (dict(dense=dict(planes=64, plane=3)), "dense takes every, sources, gap, neighbours, planes, radius, downscale, depth_margin, "
                                           "min_points, var_min, min_sources, max_cost, eps_depth, tau_px, min_consistent, max_points; "
                                           "not ['plane']"),
    (dict(dense=[("planes", 8)]), "dense must be None or a dict of every"),
    (dict(dense=dict(every=0)), "dense: every must be an integer of at least 1"),
    (dict(dense=dict(planes=2.5)), "dense: planes must be an integer of at least 1"),
    (dict(dense=dict(planes=True)), "dense: planes must be an integer"),
    (dict(dense=dict(radius=5)), "dense: radius must be an integer of at least 1 and at most 4"),
    (dict(dense=dict(sources=2, min_sources=3)), "dense: min_sources must be an integer of at least 1 and at most 2"),
    (dict(dense=dict(downscale=3)), "dense: downscale must be 1, 2 or 4"),
    (dict(dense=dict(depth_margin=-0.1)), "dense: depth_margin must be a finite number of at least 0"),
    (dict(dense=dict(var_min=math.nan)), "dense: var_min must be a finite number"),
    (dict(dense=dict(tau_px=math.inf)), "dense: tau_px must be a finite number"),
    (dict(dense=dict(max_cost=math.nan)), "dense: max_cost must be a number"),
    (dict(dense=dict(max_points=-1)), "dense: max_points must be an integer of at least 0"),
    (dict(world=2, dense={}), "dense is not supported with more than one rank: a view's depth range needs every point it observes"),
    # a stage's own keys before any rule across stages; dense after refine; the world size after the frame rules
    (dict(dense=dict(nope=1), refine=dict(rounds=0)), "refine: rounds"),
    (dict(dense=dict(nope=1), poses={}), "dense takes every"),
    (dict(world=2, refine={}, dense={}), "refine is not supported"),
]


@pytest.mark.parametrize("options, message", DENSE_RULES)
def test_a_broken_dense_rule_is_reported(options, message):
    from meatmodeler_amd.pipeline import run_plan
    with pytest.raises(ValueError) as e:
        run_plan(6, **options)
    assert message in str(e.value)


def test_the_plan_carries_the_dense_options():
    from meatmodeler_amd import pipeline
    assert pipeline.run_plan(6).dense is None and pipeline.RunPlan._field_defaults == dict(dense=None)
    given = dict(planes=32, downscale=2)
    plan = pipeline.run_plan(6, dense=given)
    assert plan.dense == dict(pipeline.DENSE_DEFAULTS, **given) and given == dict(planes=32, downscale=2)
    assert pipeline.run_plan(6, 1, dense={}).dense == pipeline.DENSE_DEFAULTS and pipeline.DENSE_KEYS == tuple(pipeline.DENSE_DEFAULTS)
    assert pipeline.run_plan(6, dense=dict(max_points=0, max_cost=-math.inf, min_consistent=0, neighbours=0)).dense["max_points"] == 0


def test_the_view_tables_and_the_frame_reduction():
    import torch
    from meatmodeler_amd import pipeline
    ref, src, nbr = pipeline.dense_views(11, 3, 4, 2, 3)
    assert ref.tolist() == [0, 3, 6, 9]
    assert src.tolist() == [[-1, 2, -1, 4], [1, 5, -1, 7], [4, 8, 2, 10], [7, -1, 5, -1]]
    assert nbr.tolist() == [[-1, 1, -1], [0, 2, -1], [1, 3, 0], [2, -1, 1]]
    fr = torch.arange(2 * 5 * 6, dtype=torch.int32).reshape(2, 5, 6).to(torch.uint8)
    K = np.array([[400.0, 2.0, 81.0], [0.0, 380.0, 59.0], [0.0, 0.0, 1.0]])
    same, K1 = pipeline.downscale_frames(fr, K, 1)
    assert same.shape == fr.shape and np.array_equal(K1, K)
    half, K2 = pipeline.downscale_frames(fr, K, 2)
    f = fr.numpy().astype(np.int64)
    assert half.shape == (2, 2, 3) and np.array_equal(half.numpy(), (f[:, 0:4:2, 0::2] + f[:, 0:4:2, 1::2] + f[:, 1:4:2, 0::2]
                                                                     + f[:, 1:4:2, 1::2] + 2) >> 2)
    assert np.array_equal(K2, [[200.0, 1.0, 40.25], [0.0, 190.0, 29.25], [0.0, 0.0, 1.0]])
    # a point projects to the centre of the reduced pixel that covers its input pixels: x' = (x - 1/2) / 2
    X = np.array([0.3, -0.2, 2.0])
    x, x2 = K @ X, K2 @ X
    assert np.allclose(x2[:2] / x2[2], (x[:2] / x[2] - 0.5) / 2)
    quarter, K4 = pipeline.downscale_frames(torch.zeros((1, 9, 13), dtype=torch.uint8), K, 4)
    assert quarter.shape == (1, 2, 3) and K4[0, 0] == 100.0 and K4[0, 2] == (81.0 - 1.5) / 4
