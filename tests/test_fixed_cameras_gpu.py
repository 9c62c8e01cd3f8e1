"""GPU: bundle adjustment with fixed cameras (mm_ba_trf_fixed and its sweeps) and the anchored sliding window
(ClipPipeline.adjust_windows(boundary="anchored"); hook at reference processor.py:395-408).

Run on the MI355X box:  python -m pytest tests/test_fixed_cameras_gpu.py -q
"""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from scipy.optimize import least_squares  # noqa: E402
from scipy.sparse import csr_matrix  # noqa: E402

from meatmodeler_amd import _lib, ops, synth, bundleAdjuster  # noqa: E402
from meatmodeler_amd._lib import default_context, lib, ptr  # noqa: E402
from meatmodeler_amd.bundleAdjuster import SchurTRF, frameParameters  # noqa: E402
from meatmodeler_amd.pipeline import ClipPipeline  # noqa: E402
from oracle import ba_oracle as bo  # noqa: E402

DEV = torch.device("cuda", 0)
MM_CTL_CHOL_LAST_PATH = 2


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def remap(fi, fixed, F):
    """Free frames -> 0..F_free-1 in order, fixed frames -> F_free + k (restated here, not taken from the package)."""
    free = [f for f in range(F) if f not in set(fixed)]
    order = np.array(free + sorted(fixed))
    new = np.empty(F, np.int64)
    new[order] = np.arange(F)
    return order, new[np.asarray(fi)], len(free)


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


def test_residual_and_normal_equations_with_fixed_cameras():
    """mm_ba_residual_fixed against the oracle on [free | fixed | points]; the normal-equation blocks of the free cameras
    and of the points against the same problem with every camera free (mm_ba_normal_eq)."""
    pr = synth.make_ba_problem(48, 1500, 6)
    F, P = 48, len(pr["pts0"])
    fixed = list(range(6)) + [30]
    order, fi, Ff = remap(pr["fi"], fixed, F)
    cams = frameParameters(pr["ext"]).reshape(F, 6)[order]
    pb = ops.BADevice(pr["K"], fi, pr["pi"], pr["obs"], Ff, P, DEV, fixed_cams=dev(cams[Ff:]))
    assert pb.F_fixed == len(fixed) and int(pb.cam_ptr[-1]) == int((fi < Ff).sum())
    c2, res = pb.residual(dev(cams[:Ff]), dev(pr["pts0"]), want_res=True)
    ref = bo.point_fun(np.hstack([cams.ravel(), pr["pts0"].ravel()]), pr["K"], F, P, fi, pr["pi"], pr["obs"])
    assert rel(res.cpu().numpy().ravel(), ref) <= 1e-9
    assert abs(float(c2) - np.sum(ref ** 2)) <= 1e-9 * np.sum(ref ** 2)
    B, gc, Cb, gp = (t.cpu().numpy() for t in pb.normal_eq(dev(cams[:Ff]), dev(pr["pts0"])))
    pa = ops.BADevice(pr["K"], fi, pr["pi"], pr["obs"], F, P, DEV)
    Ba, gca, Ca, gpa = (t.cpu().numpy() for t in pa.normal_eq(dev(cams), dev(pr["pts0"])))
    for a, b in ((B, Ba[:Ff]), (gc, gca[:Ff]), (Cb, Ca), (gp, gpa)):
        assert rel(a, b) <= 1e-13
    bitwise = all(np.array_equal(a, b) for a, b in ((B, Ba[:Ff]), (gc, gca[:Ff]), (Cb, Ca), (gp, gpa)))
    print("normal equations with fixed cameras equal the all-free blocks bitwise:", bitwise)
    # the pair list holds free-free pairs only, cam_span is over the free cameras
    po, po2 = pb.pair_o.long().cpu().numpy(), pb.pair_o2.long().cpu().numpy()
    assert (fi[po] < Ff).all() and (fi[po2] < Ff).all()
    free_obs = np.flatnonzero(fi < Ff)
    assert pb.n_pairs == sum(int(((fi[free_obs] <= fi[o]) & (pr["pi"][free_obs] == pr["pi"][o])).sum()) for o in free_obs)


def _g5c(golden_dir):
    d = np.load(os.path.join(golden_dir, "g5_adjust_points_c.npz"))
    F, P, L, seed = (int(d[k]) for k in ("F", "P", "L", "seed"))
    pr = synth.make_ba_problem(F, P, L, seed=seed)
    return pr, F, P, frameParameters(pr["ext"]).reshape(F, 6)


def test_trf_fixed_with_no_fixed_camera_is_trf(golden_dir):
    """mm_ba_trf_fixed(fx = {0, NULL}) is mm_ba_trf, bit for bit (G5 case c)."""
    pr, F, P, cams0 = _g5c(golden_dir)
    pb = ops.BADevice(pr["K"], pr["fi"], pr["pi"], pr["obs"], F, P, DEV)
    c1, p1 = dev(cams0), dev(pr["pts0"])
    rep1, _ = pb.trf_solve(c1, p1, 1e-4, 1e-8, 1e-8)
    c2, p2 = dev(cams0), dev(pr["pts0"])
    fx = _lib.BAFixed(0, 0, None)
    ctx = default_context()
    ws = torch.empty(lib.mm_ba_trf_fixed_workspace_bytes(C.byref(pb.pb), C.byref(fx)), dtype=torch.uint8, device=DEV)
    prm = _lib.TrfParams(1e-4, 1e-8, 1e-8, 1e-9, 0)
    rep2 = _lib.TrfReport()
    log = (_lib.TrfRow * 1)()
    ctx.check(lib.mm_ba_trf_fixed(ctx.h, C.byref(pb.pb), C.byref(fx), ptr(c2), ptr(p2), C.byref(prm), C.byref(rep2), log, 0,
                                  ptr(ws), ws.numel()), "mm_ba_trf_fixed")
    assert torch.equal(c1, c2) and torch.equal(p1, p2)
    assert (rep1.nfev, rep1.njev, rep1.status, rep1.cost) == (rep2.nfev, rep2.njev, rep2.status, rep2.cost)


def test_unobserved_fixed_cameras_change_nothing(golden_dir):
    """G5 case c with frames 0 and 1 fixed, then the same with five more fixed cameras that no observation references:
    bit-identical cameras, points and report (they cost a row of the coefficient table and nothing else)."""
    pr, F, P, cams0 = _g5c(golden_dir)
    order, fi, Ff = remap(pr["fi"], [0, 1], F)
    cams = cams0[order]
    extra = np.random.default_rng(3).normal(0, 0.1, (5, 6))
    out = []
    for fixed in (cams[Ff:], np.vstack([cams[Ff:], extra])):
        pb = ops.BADevice(pr["K"], fi, pr["pi"], pr["obs"], Ff, P, DEV, fixed_cams=dev(fixed))
        c, p = dev(cams[:Ff]), dev(pr["pts0"])
        rep, _ = pb.trf_solve(c, p, 1e-4, 1e-8, 1e-8)
        out.append((c, p, (rep.nfev, rep.njev, rep.status, rep.cost)))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert out[0][2] == out[1][2]


def test_fixed_camera_solve_matches_scipy_on_the_reduced_problem():
    """SciPy's least_squares over the free parameters only (the oracle's residual with the fixed cameras inserted, the
    oracle's sparsity without the fixed columns) against solvePoints(fixed_frames=...).  The fixed cameras pin the gauge:
    no similarity alignment."""
    pr = synth.make_ba_problem(64, 1000, 6, seed=11)
    F, P = 64, len(pr["pts0"])
    fixed = list(range(8))
    order, fi, Ff = remap(pr["fi"], fixed, F)
    assert Ff == 56
    cams = frameParameters(pr["ext"]).reshape(F, 6)[order]
    fixed_rows = cams[Ff:].ravel()
    K, pi, obs = pr["K"], pr["pi"], pr["obs"]

    def fun(xr):
        return bo.point_fun(np.concatenate([xr[:6 * Ff], fixed_rows, xr[6 * Ff:]]), K, F, P, fi, pi, obs)

    A = csr_matrix(bo.sparsity_pattern(F, P, fi, pi))
    keep = np.r_[0:6 * Ff, 6 * F:6 * F + 3 * P]
    A = A[:, keep]
    x0 = np.concatenate([cams[:Ff].ravel(), pr["pts0"].ravel()])
    tight = least_squares(fun, x0, jac_sparsity=A, jac="3-point", x_scale="jac", ftol=1e-13, xtol=1e-13, gtol=1e-13,
                          method="trf", tr_solver="lsmr", tr_options=dict(atol=1e-14, btol=1e-14), max_nfev=3000)
    res = bundleAdjuster.solvePoints(pr["ext"], K, pr["pts0"], obs, pr["fi"], pi, ftol=1e-13, xtol=1e-13, gtol=1e-13,
                                     verbose=0, fixed_frames=fixed)
    assert default_context().control(MM_CTL_CHOL_LAST_PATH) == 1      # the single-launch two-ended factorisation
    assert tight.status > 0 and res.status > 0
    assert abs(res.cost - tight.cost) <= 1e-8 * tight.cost, (res.cost, tight.cost)
    scene = np.abs(tight.x[6 * Ff:]).max()
    pts_g = res.x[6 * F:]
    cams_g = res.x[:6 * F].reshape(F, 6)
    assert np.abs(pts_g - tight.x[6 * Ff:]).max() <= 1e-5 * scene
    assert np.abs(cams_g[order[:Ff]].ravel() - tight.x[:6 * Ff]).max() <= 1e-5 * scene
    assert np.array_equal(cams_g[fixed], frameParameters(pr["ext"]).reshape(F, 6)[fixed])
    # the reference's own settings (bundleAdjuster.py:180-192)
    ref = least_squares(fun, x0, jac_sparsity=A, verbose=0, x_scale="jac", ftol=1e-4, method="trf")
    res4 = bundleAdjuster.solvePoints(pr["ext"], K, pr["pts0"], obs, pr["fi"], pi, ftol=1e-4, verbose=0, fixed_frames=fixed)
    print(f"fixed-camera parity: tight nfev scipy {tight.nfev} gpu {res.nfev}; reference settings nfev scipy {ref.nfev} "
          f"gpu {res4.nfev}, status {ref.status} / {res4.status}, cost {ref.cost:.10e} / {res4.cost:.10e}")
    assert res4.status == ref.status
    # (at ftol = 1e-4 the two stop at different points of the descent: SciPy's inexact LSMR steps on 2-point differences
    # and the exact Schur steps take different paths -- measured: 5 vs 7 evaluations, 1.92133e3 vs 1.92093e3.  The GPU
    # solve must be no worse.)
    assert res4.cost <= ref.cost * (1 + 1e-5)


def test_solve_points_fixed_frames_api():
    pr = synth.make_ba_problem(24, 400, 5, seed=5)
    F, P = 24, len(pr["pts0"])
    args = (pr["ext"], pr["K"], pr["pts0"], pr["obs"], pr["fi"], pr["pi"])
    fixed = [0, 1, 17]
    res = bundleAdjuster.solvePoints(*args, verbose=0, fixed_frames=fixed)
    # the same problem remapped by hand
    order, fi, Ff = remap(pr["fi"], fixed, F)
    cams = frameParameters(pr["ext"]).reshape(F, 6)
    cr = cams[order]
    pb = ops.BADevice(pr["K"], fi, pr["pi"], pr["obs"], Ff, P, DEV, fixed_cams=dev(cr[Ff:]))
    r = SchurTRF(pb).solve(dev(cr[:Ff]), dev(pr["pts0"]))
    assert (res.nfev, res.cost, res.status) == (r.nfev, r.cost, r.status)
    x = res.x[:6 * F].reshape(F, 6)
    assert np.array_equal(x[order[:Ff]], r.cams.cpu().numpy())
    assert np.array_equal(res.x[6 * F:], r.pts.cpu().numpy().ravel())
    assert np.array_equal(x[fixed], cams[fixed])
    assert np.array_equal(res.cams.cpu().numpy(), x)
    # a boolean mask is the same request
    mask = np.zeros(F, bool)
    mask[fixed] = True
    assert np.array_equal(bundleAdjuster.solvePoints(*args, verbose=0, fixed_frames=mask).x, res.x)
    # fixed_frames=None is the call without it
    a = bundleAdjuster.solvePoints(*args, verbose=0)
    b = bundleAdjuster.solvePoints(*args, verbose=0, fixed_frames=None)
    assert np.array_equal(a.x, b.x) and (a.nfev, a.cost) == (b.nfev, b.cost)
    pts_a, _ = bundleAdjuster.adjustPoints(*args, fixed_frames=fixed)
    assert np.array_equal(pts_a, res.x[6 * F:].reshape(P, 3))
    with pytest.raises(ValueError):
        bundleAdjuster.solvePoints(*args, verbose=0, fixed_frames=list(range(F)))


@pytest.mark.parametrize("F,arc", [(9, 10.0), (16, 16.0)])
def test_anchored_windows_equal_window_by_window_adjustment(F, arc):
    """boundary="anchored": every window restated with NumPy (selection, remap, fixed set) and solved with
    BADevice(..., fixed_cams=...) gives the pipeline's stats and, at the end, its cameras and points bit for bit."""
    W, S = 5, 2
    frames, ext, K = synth.render_orbit_frames(F, 640, 480, arc_deg=arc)
    pipe = ClipPipeline(480, 640, 600, batch=F)
    out = pipe.run(dev(frames), K, ext, ba=False)
    res = pipe.adjust_windows(out, K, ext, window=W, stride=S, boundary="anchored")
    inside = pipe.adjust_windows(out, K, ext, window=W, stride=S)
    ClipPipeline.tracks_to_host(out)
    tp, of, ok = out["track_ptr"], out["obs_frame"], out["obs_kp"]
    xy = out["xy_dev"].cpu().numpy()
    cams = frameParameters(np.asarray(ext)[:, :3, :]).reshape(F, 6)
    pts = out["points0"].cpu().numpy().copy()
    first, last = of[tp[:-1]], of[tp[1:] - 1]
    wins = iter(res["windows"])
    n_checked, boundary_seen = 0, False
    for hi in list(range(W, F, S)) + [F]:
        lo = max(0, hi - W)
        Wn = hi - lo
        sel = [t for t in range(len(first)) if lo <= last[t] < hi and (hi >= F or last[t] <= hi - 2)]
        if not sel:
            continue
        fi, pi, coords = [], [], []
        for j, t in enumerate(sel):
            for o in range(tp[t], tp[t + 1]):
                fi.append(of[o] - lo if of[o] >= lo else Wn + of[o])
                pi.append(j)
                coords.append(xy[of[o], ok[o]])
        fi, pi, coords = np.array(fi), np.array(pi), np.array(coords, np.float64)
        n_fixed = len(set(fi[fi >= Wn].tolist()))
        fixed_cams = dev(cams[:lo]) if lo > 0 else None
        pb = ops.BADevice(K, fi, pi, coords, Wn, len(sel), DEV, fixed_cams=fixed_cams)
        before = cams[:lo].copy()
        r = SchurTRF(pb).solve(dev(cams[lo:hi]), dev(pts[sel]))
        st = next(wins)
        assert (st["lo"], st["hi"], st["points"], st["observations"], st["fixed_cameras"]) == (lo, hi, len(sel), len(fi), n_fixed)
        assert (st["nfev"], st["cost"]) == (r.nfev, r.cost)
        rc, rp = r.cams.cpu().numpy(), r.pts.cpu().numpy()
        x1 = np.hstack([rc.ravel(), cams[:lo].ravel(), rp.ravel()])
        c_oracle = 0.5 * np.sum(bo.point_fun(x1, K, Wn + lo, len(sel), fi, pi, coords) ** 2)
        assert abs(c_oracle - st["cost"]) <= 1e-7 * max(c_oracle, 1.0)
        if lo > 0 and n_fixed > 0 and any(first[t] < lo for t in sel):
            boundary_seen = True
        if lo == 0:      # the first window is the one boundary="inside" adjusts
            assert {k: v for k, v in st.items() if k != "fixed_cameras"} == inside["windows"][0]
        cams[lo:hi] = rc
        pts[sel] = rp
        assert np.array_equal(cams[:lo], before)
        n_checked += 1
    assert n_checked >= 2 and next(wins, None) is None
    assert boundary_seen, "no window held a boundary track observed by a fixed camera"
    assert np.array_equal(res["points"].cpu().numpy(), pts) and np.array_equal(res["cams"].cpu().numpy(), cams)


def test_anchored_windows_refuse_concurrent_schedules():
    F = 9
    frames, ext, K = synth.render_orbit_frames(F, 640, 480, arc_deg=10.0)
    pipe = ClipPipeline(480, 640, 600, batch=F)
    out = pipe.run(dev(frames), K, ext, ba=False)
    for kw in (dict(order="wavefront"), dict(batched=True), dict(streams=2), dict(boundary="outside")):
        kw.setdefault("boundary", "anchored")
        with pytest.raises(ValueError):
            pipe.adjust_windows(out, K, ext, window=5, stride=2, **kw)
