"""GPU: the BA linear algebra -- residual, Jacobian, normal equations, Jacobian scaling and damping, reduced camera system,
its banded solves and the back-substitution -- against the exact CPU reference of oracle/ba_oracle.py, on ragged
problems shaped like pipeline output and at the benchmark shape.

Every bound is a formula in eps = 2^-52, the number k of terms a kernel sums and, for the inverses and solves, a
condition number; the safety factor is at most 10.  Each test also asserts which kernel path it exercised.

Run on the MI355X box:  python -m pytest tests/test_ba_reference_gpu.py -q -s
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import scipy.linalg as sla  # noqa: E402

from meatmodeler_amd import ops, synth  # noqa: E402
from meatmodeler_amd._lib import default_context  # noqa: E402
from oracle import ba_oracle as bo  # noqa: E402

DEV = torch.device("cuda", 0)
EPS = 2.0 ** -52
LD = bo.LD


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def check(name, got, ref, bound):
    """|got - ref| <= bound entrywise (bound 0: exactly equal); prints the worst err / bound.  A NaN or an infinity
    anywhere -- in what the kernel wrote, in the reference or in the bound -- fails."""
    got = np.asarray(got).astype(LD)
    ref = np.asarray(ref).astype(LD)
    assert got.shape == ref.shape and np.ndim(bound) <= ref.ndim, (name, got.shape, ref.shape, np.shape(bound))
    for what, a in (("kernel output", got), ("reference", ref), ("bound", np.asarray(bound))):
        assert np.isfinite(a).all(), (name, what, "is not finite", int((~np.isfinite(a)).sum()))
    bound = np.broadcast_to(np.asarray(bound).astype(LD), ref.shape)
    err = np.abs(got - ref)
    pos = bound > 0
    worst = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    print(f"  {name:<28} worst err/bound {worst:.3g}")
    bad = ~(err <= bound)
    assert not bad.any(), (name, int(bad.sum()), float(err[bad].max()), float(bound[bad].min()), worst)


TRI = ([0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2])      # packed 3 x 3 (xx, xy, xz, yy, yz, zz)


def check_normal_eq(prefix, got, nb):
    """The kernels' (B, gc, C packed, gp) against normal_blocks: (k + 1) eps sum|terms| entrywise (k summed products,
    one rounding for the product)."""
    for name, g in zip(("B", "gc", "C", "gp"), got):
        ref, ab = nb[name], nb[name + "_abs"]
        if name == "C":
            ref, ab = ref[:, TRI[0], TRI[1]], ab[:, TRI[0], TRI[1]]
        k = nb[name + "_k"].reshape((-1,) + (1,) * (ref.ndim - 1)) + 1
        check(f"{prefix} {name}", g, ref, k * EPS * ab)


def ulp_check(name, got, ref, n_ulp=2):
    ref64 = np.asarray(ref).astype(np.float64)
    check(name, got, ref, n_ulp * np.spacing(np.abs(ref64)))


# ---------------------------------------------------------------------------------------------------- problems

def _problem(kind):
    if kind in ("R1", "R1s", "R1f"):
        pr = bo.ragged_ba_problem(1, 160, 40_000, shuffle=kind == "R1s")
    elif kind == "R2":
        pr = bo.ragged_ba_problem(2, 300, 20_000, empty_run=False, long_tracks=6, long_span=240)
    else:
        pr = synth.make_ba_problem(500, 300_000, 5, seed=9)
        pr["cams"] = bo.frame_parameters(pr["ext"]).reshape(500, 6)
    return pr


def _residual_bound(pr, x, F, P, fi, pi):
    """First-order magnitude of the projection's rounding: |K| (|R||X| + |t|) over u_z, for both rows."""
    cams = x[:6 * F].reshape(F, 6)
    pts = x[6 * F:].reshape(P, 3)
    R = np.abs(np.stack([bo.rodrigues_matrix(c[:3]) for c in cams]))
    Xa = np.einsum("oij,oj->oi", R[fi], np.abs(pts[pi])) + np.abs(cams[fi, 3:])
    Ka = np.abs(pr["K"])
    ua = Xa @ Ka.T
    X = bo.project(pts[pi], cams[fi], pr["K"])
    uz = (bo.rotate(pts[pi], cams[fi, :3]) + cams[fi, 3:]) @ pr["K"][2]
    mag = (ua[:, :2] + np.abs(X) * ua[:, 2:3]) / np.abs(uz)[:, None] + np.abs(pr["obs"])
    return 10 * EPS * mag


def _sweeps(pr, F, P, pb, cams, pts, fi, pi, jac_dtype=None):
    """Residual, Jacobian, normal equations: -> (Jc, Jp exact, Jc, Jp, res, B, gc, C6, gp of the kernels)."""
    x = np.hstack([cams.ravel(), pts.ravel()])
    cd, pd = dev(cams), dev(pts)
    c2, res = pb.residual(cd, pd, True)
    res = host(res)
    check("residual", res, bo.point_fun_exact(x, pr["K"], F, P, fi, pi, pr["obs"]), _residual_bound(pr, x, F, P, fi, pi))
    assert abs(float(c2) - float((res.astype(LD) ** 2).sum())) <= 2 * res.size * EPS * float(c2)
    Jc_x, Jp_x = bo.jacobian_exact(x, pr["K"], F, P, fi, pi, pr["obs"], dtype=jac_dtype)
    Jc_g, Jp_g = (host(t) for t in pb.jacobian(cd, pd))
    scale = np.maximum(np.abs(Jc_x).max(axis=(1, 2)), np.abs(Jp_x).max(axis=(1, 2)))[:, None, None]
    check("jacobian Jc", Jc_g, Jc_x, 1e-12 * scale)
    check("jacobian Jp", Jp_g, Jp_x, 1e-12 * scale)
    B, gc, C6, gp = (host(t) for t in pb.normal_eq(cd, pd))
    # the normal equations from the kernels' own Jacobian and residual: what is pinned here is the accumulation
    check_normal_eq("normal_eq", (B, gc, C6, gp), bo.normal_blocks(Jc_g, Jp_g, res, fi, pi, F, P))
    return Jc_x, Jp_x, Jc_g, Jp_g, res, B, gc, C6, gp


def _backward_error(S, v, x):
    """eta of the diagonally scaled system (long double): |S^ x^ - v^|inf / (|S^|inf |x^|inf + |v^|inf)."""
    S, v, x = (np.asarray(a).astype(LD) for a in (S, v, x))
    d = np.sqrt(np.diag(S))
    Sh = S / d[:, None] / d[None, :]
    vh, xh = v / d, x * d
    r = Sh @ xh - vh
    return float(np.abs(r).max() / (np.abs(Sh).sum(1).max() * np.abs(xh).max() + np.abs(vh).max())), Sh


def _solves(name, reg, pb, cams, pts, Bd, Cd, gc, gp, rs, hb, Sb, vb, expect_path):
    """dc from mm_chol_solve_sym / mm_chol_solve on the uploaded reference system and from schur_solve (both
    overlap settings) against S_ref, v_ref: backward errors of the scaled system."""
    ctx = default_context()
    S64, v64 = rs["S"].astype(np.float64), rs["v"].astype(np.float64)
    n = S64.shape[0]
    d = np.sqrt(np.diag(S64))
    Sh64 = S64 / d[:, None] / d[None, :]
    lam = float(np.linalg.eigvalsh(Sh64)[0])
    assert np.isfinite(lam), (name, lam)
    want_ok = lam >= 100 * n * EPS
    # kappa of the 64 x 64 diagonal blocks of LAPACK's factor of the scaled system (the one eta is measured on)
    Lf = None
    try:
        Lf = np.linalg.cholesky(Sh64)
    except np.linalg.LinAlgError:
        assert not want_ok, (name, "LAPACK cannot factor a system with lambda_min", lam)
    kap = max(np.linalg.cond(Lf[i:i + 64, i:i + 64]) for i in range(0, n, 64)) if Lf is not None else np.inf
    assert want_ok <= bool(np.isfinite(kap)), (name, kap)
    base = n * EPS * (1.0 if reg >= 1e-3 else kap)
    # the S / v bound of the build, in the norms of the scaled system
    Sh_b = (Sb / d[:, None] / d[None, :]).sum(1).max()
    Sh_n = np.abs(S64 / d[:, None] / d[None, :]).sum(1).max()
    build = float(Sh_b / Sh_n + np.abs(vb / d).max() / np.abs(v64 / d).max())
    eta_lapack = _backward_error(S64, v64, sla.cho_solve(sla.cho_factor(S64, lower=True), v64))[0] if Lf is not None \
        else float("nan")
    print(f"  {name}: n={n} kappa(L_kk)max={kap:.3g} lambda_min={lam:.3g} bound={base:.3g} (+build {build:.3g}) "
          f"LAPACK eta={eta_lapack:.3g}")
    runs = []
    for how in ("sym", "chol"):
        Sg, vg = dev(S64), dev(v64)
        info = ops.chol_solve_sym(Sg, vg, half_bandwidth=hb, both_triangles=True) if how == "sym" \
            else ops.chol_solve(Sg, vg, half_bandwidth=hb)
        ctx.sync()
        runs.append((how, int(info), host(vg), 0.0))
        if how == "chol":
            assert int(ctx.control(ctx.CTL_CHOL_LAST_PATH)) == expect_path
    for ov in (True, False):
        pb.overlap = ov
        info, dc, _ = pb.schur_solve(dev(cams), dev(pts), dev(Bd), dev(Cd), dev(gc), dev(gp), hb)
        runs.append((f"schur_solve overlap={ov}", int(info), host(dc), build))
    pb.overlap = False
    for how, info, x, extra in runs:
        if want_ok:
            assert info == 0, (name, how, info, lam)
        if info != 0:
            print(f"    {how}: info={info} (lambda_min {lam:.3g} < 100 n eps)")
            continue
        eta = _backward_error(rs["S"], rs["v"], x)[0]
        assert np.isfinite(eta) and np.isfinite(base + extra), (name, how, eta, base, extra)
        print(f"    {how}: eta={eta:.3g}  eta/bound={eta / (base + extra):.3g}  eta/LAPACK={eta / eta_lapack:.3g}")
        assert eta <= base + extra, (name, how, eta, base, extra)
    return runs[2][2] if runs[2][1] == 0 else None


def _chain(kind, pr, F, pb, jac_dtype=None, regs=(1e-3, 1e-9), s_from_kernel_jacobian=False):
    P = len(pr["pts0"])
    fi, pi = np.asarray(pr["fi"]), np.asarray(pr["pi"])
    cams, pts = pr["cams"], pr["pts0"]
    print(f"\n{kind}: F={F} P={P} O={fi.size} pairs={pb.n_pairs} span={pb.cam_span} slabs={pb.slabs is not None}")
    Jc, Jp, Jc_g, Jp_g, res, B, gc, C6, gp = _sweeps(pr, F, P, pb, cams, pts, fi, pi, jac_dtype)
    # x_scale='jac': the first call and a later one (running maximum)
    si_t = torch.empty(6 * F + 3 * P, dtype=torch.float64, device=DEV)
    si = host(pb.scale_update(dev(B), dev(C6), si_t, True))
    ulp_check("scale_update first", si, bo.jac_scale(B, C6))
    old = si * np.where(np.arange(si.size) % 3 == 0, 1.25, 0.75)
    si2 = host(pb.scale_update(dev(B), dev(C6), dev(old), False))
    ulp_check("scale_update later", si2, bo.jac_scale(B, C6, old))
    hb = 6 * pb.cam_span + 5
    Bt, Ct = dev(B), dev(C6)
    for reg in regs:
        Bd_t, Cd_t = torch.empty_like(Bt), torch.empty_like(Ct)
        pb.damp(Bt, Ct, dev(si), torch.tensor([reg], dtype=torch.float64, device=DEV), Bd_t, Cd_t)
        Bd, Cd = host(Bd_t), host(Cd_t)
        Bd_x, Cd_x = bo.damp(B, C6, si, reg)
        ulp_check(f"damp B reg {reg:g}", Bd, Bd_x)
        ulp_check(f"damp C reg {reg:g}", Cd, Cd_x)
        S, v, Cinv = (host(t) for t in pb.schur(dev(cams), dev(pts), Bd_t, Cd_t, dev(gc), dev(gp)))
        Cd3 = bo.unpack_sym3(Cd)
        Q = bo.inv3(Cd3.astype(LD))
        cond = np.linalg.cond(Cd3)
        qn = np.linalg.norm(bo.unpack_sym3(Cinv), 2, axis=(1, 2))
        check(f"Cinv reg {reg:g}", Cinv, Q[:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]],
              (10 * EPS * cond * qn)[:, None])
        # S from the exact Jacobian: that pins the pair kernel's lean camera table.  The general kernel evaluates the
        # closed form mm_ba_jacobian uses (pinned above); its S is compared with the sums of that Jacobian, since on
        # entries with a few pairs its rounding (1e-15 of the observation's largest entry) exceeds k eps sum|terms|
        Js = (Jc_g, Jp_g) if s_from_kernel_jacobian else (Jc, Jp)
        rs = bo.reduced_system(*Js, fi, pi, F, P, Bd, None, gc, gp, Cinv=Cinv)
        Sb = rs["S_k"] * EPS * rs["S_abs"]
        vb = rs["v_k"] * EPS * rs["v_abs"]
        check(f"S reg {reg:g}", S, rs["S"], Sb)
        check(f"v reg {reg:g}", v, rs["v"], vb)
        i, j = np.indices(S.shape)
        assert not S[np.abs(i // 6 - j // 6) > pb.cam_span].any()
        # the single-launch factorisation takes bands of up to FUSED_MAX_BWB = 15 blocks of 64 (csrc/chol.hip), the
        # launch-per-column one wider bands; nothing here sets the switches that avoid the former
        path = 1 if -(-hb // 64) <= 15 else 0
        dc = _solves(f"{kind} reg {reg:g}", reg, pb, cams, pts, Bd, Cd, gc, gp, rs, hb, Sb.astype(np.float64),
                     vb.astype(np.float64), path)
        if dc is not None:
            dp = host(pb.backsub(dev(cams), dev(pts), dev(Cinv), dev(gp), dev(dc.reshape(F, 6))))
            # from the kernels' own Jacobian: a point seen once has an ill-conditioned Cd, and Cinv amplifies the
            # Jacobian's own rounding beyond k eps sum|terms| -- what is pinned here is the accumulation
            dpx, dpa, dpk = bo.backsub(Jc_g, Jp_g, fi, pi, P, Cinv, gp, dc)
            check(f"backsub reg {reg:g}", dp, dpx, dpk * EPS * dpa)


def _segments(pb, F):
    """{(camera, other camera): pairs} from the device's segment / chunk tables."""
    seg = host(pb.seg_ids).astype(np.int64)
    ptr = host(pb.seg_chunk_ptr)
    cb, ce = host(pb.chunk_begin), host(pb.chunk_end)
    n = np.array([(ce[ptr[s]:ptr[s + 1]] - cb[ptr[s]:ptr[s + 1]]).sum() for s in range(len(seg))])
    span = pb.cam_span + 1
    return {(int(k // span), int(k // span - k % span)): int(c) for k, c in zip(seg, n)}, ptr


@pytest.mark.parametrize("kind", ["R1", "R1s"])
def test_ragged_pair_path_against_exact_reference(kind):
    pr = _problem(kind)
    F = 160
    pb = ops.BADevice(pr["K"], pr["fi"], pr["pi"], pr["obs"], F, len(pr["pts0"]), DEV)
    # the path: pair list, camera slabs (ceil(F/8) >= 16) with an empty one, multi-chunk segments
    assert pb.n_pairs > 0 and pb.slabs is not None
    ns, cps, sseg, _ = pb.slabs
    assert (np.diff(sseg) == 0).any(), "one camera slab holds no segment"
    segs, ptr = _segments(pb, F)
    for key, want in pr["planted"].items():
        assert segs[key] == want
    nch = {k: -(-c // 512) for k, c in segs.items()}
    assert max(nch.values()) >= 3 and nch[[k for k, c in pr["planted"].items() if c == 513][0]] == 2
    lo, hi = pr["empty"]
    assert int(pb.cam_ptr[hi]) == int(pb.cam_ptr[lo])          # cameras with no observation
    _chain(kind, pr, F, pb)


def test_ragged_fixed_cameras_residual_and_normal_equations():
    pr = _problem("R1f")
    F, P = 160, len(pr["pts0"])
    fixed = np.arange(5, F, 16)[:10]
    free = np.setdiff1d(np.arange(F), fixed)
    order = np.r_[free, fixed]
    new = np.empty(F, np.int64)
    new[order] = np.arange(F)
    fi = new[pr["fi"]]
    Ff = free.size
    cams = pr["cams"][order]
    pts = pr["pts0"]
    pb = ops.BADevice(pr["K"], fi, pr["pi"], pr["obs"], Ff, P, DEV, fixed_cams=dev(cams[Ff:]))
    assert pb.F_fixed == 10 and pb.n_pairs > 0
    x = np.hstack([cams.ravel(), pts.ravel()])
    cd, pd = dev(cams[:Ff]), dev(pts)
    c2, res = pb.residual(cd, pd, True)
    res = host(res)
    check("residual fixed", res, bo.point_fun_exact(x, pr["K"], F, P, fi, pr["pi"], pr["obs"]),
          _residual_bound(pr, x, F, P, fi, pr["pi"]))
    assert abs(float(c2) - float((res.astype(LD) ** 2).sum())) <= 2 * res.size * EPS * float(c2)
    # the kernels' Jacobian from the same problem with every camera free (no fixed form of mm_ba_jacobian)
    pb_all = ops.BADevice(pr["K"], fi, pr["pi"], pr["obs"], F, P, DEV)
    Jc_g, Jp_g = (host(t) for t in pb_all.jacobian(dev(cams), pd))
    Jc_x, Jp_x = bo.jacobian_exact(x, pr["K"], F, P, fi, pr["pi"], pr["obs"])
    scale = np.maximum(np.abs(Jc_x).max(axis=(1, 2)), np.abs(Jp_x).max(axis=(1, 2)))[:, None, None]
    check("jacobian (all free)", Jc_g, Jc_x, 1e-12 * scale)
    B, gc, C6, gp = (host(t) for t in pb.normal_eq(cd, pd))
    check_normal_eq("normal_eq_fixed", (B, gc, C6, gp), bo.normal_blocks(Jc_g, Jp_g, res, fi, pr["pi"], Ff, P))


def test_ragged_wide_band_general_kernel_against_exact_reference():
    pr = _problem("R2")
    F = 300
    pb = ops.BADevice(pr["K"], pr["fi"], pr["pi"], pr["obs"], F, len(pr["pts0"]), DEV)
    # the path: no pair list (span > 192), two 256-camera column windows of the LDS-atomic kernel
    assert pb.n_pairs == 0 and pb.cam_span > 192 and F > 256
    fi, pi = pr["fi"], pr["pi"]
    lo_cam = np.full(len(pr["pts0"]), F)
    hi_cam = np.zeros(len(pr["pts0"]), np.int64)
    np.minimum.at(lo_cam, pi, fi)
    np.maximum.at(hi_cam, pi, fi)
    assert ((lo_cam < 256) & (hi_cam >= 256)).any()          # couplings across the window boundary
    _chain("R2", pr, F, pb, s_from_kernel_jacobian=True)


def test_benchmark_shape_against_exact_reference():
    """R3, the benchmark's problem (500 cameras, 300 k points, n = 3000, camera span 4).  The Jacobian reference runs in complex128 here
    (complex steps are exact to the working precision, 2^-52 relative per entry, far inside the 1e-12 bound); the
    sums stay in long double."""
    pr = _problem("R3")
    F = 500
    pb = ops.BADevice(pr["K"], pr["fi"], pr["pi"], pr["obs"], F, len(pr["pts0"]), DEV)
    assert pb.n_pairs > 0 and pb.slabs is not None
    _chain("R3", pr, F, pb, jac_dtype=np.complex128)
