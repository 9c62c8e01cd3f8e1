"""CPU: the exact BA reference of oracle/ba_oracle.py (complex-step Jacobian, long-double normal equations, reduced
camera system, SciPy's Jacobian scaling) against independent formulations -- 50-digit mpmath derivatives, central
differences, dense np.linalg algebra and SciPy itself.  The GPU tests of tests/test_ba_reference_gpu.py lean on it."""
import numpy as np
import pytest

from meatmodeler_amd import synth
from oracle import ba_oracle as bo

mpmath = pytest.importorskip("mpmath")


def _x(pr):
    return np.hstack([pr["cams"].ravel(), pr["pts0"].ravel()])


def test_ragged_problem_has_the_planned_structure():
    pr = bo.ragged_ba_problem(3, 160, 6000)
    F, P = 160, len(pr["pts0"])
    fi, pi = pr["fi"], pr["pi"]
    lens = np.bincount(pi, minlength=P)
    assert lens.min() == 1 and lens.max() >= 20
    lo, hi = pr["empty"]
    assert hi - lo >= -(-F // 8) and not np.isin(fi, np.arange(lo, hi)).any()
    per_cam = np.bincount(fi, minlength=F)
    assert per_cam.max() > 1000 and ((per_cam > 0) & (per_cam < 50)).any()     # hot cameras and nearly empty ones
    o, o2 = bo._pairs_of_points(fi, pi)
    key, n = np.unique(fi[o] * F + fi[o2], return_counts=True)
    cnt = dict(zip(key.tolist(), n.tolist()))
    for (i, j), want in pr["planted"].items():
        assert cnt[i * F + j] == want
    got = sorted(pr["planted"].values())
    assert 512 in got and 513 in got and got[-1] > 1024
    assert any(i == j for i, j in pr["planted"]) and any(i != j for i, j in pr["planted"])
    th2 = (pr["cams"][pr["special"], :3] ** 2).sum(1)
    np.testing.assert_allclose(th2, bo.SPECIAL_THETA2, rtol=1e-14, atol=0)
    # every special camera sees the scene in front of it
    R = np.stack([bo.rodrigues_matrix(c[:3]) for c in pr["cams"][pr["special"]]])
    z = np.einsum("fj,fj->f", R[:, 2], np.zeros((len(R), 3))) + pr["cams"][pr["special"], 5]
    assert (z > 5).all()
    sh = bo.ragged_ba_problem(3, 160, 6000, shuffle=True)
    assert not (np.diff(sh["pi"]) >= 0).all()
    assert sorted(zip(sh["fi"], sh["pi"])) == sorted(zip(fi, pi))


def _mp_project(c, X, K):
    """Textbook Rodrigues (theta = |r|, unit axis) in mpmath."""
    r = [mpmath.mpf(v) for v in c[:3]]
    th = mpmath.sqrt(sum(v * v for v in r))
    X = [mpmath.mpf(v) for v in X]
    if th == 0:
        Xr = X
    else:
        k = [v / th for v in r]
        kx = [k[1] * X[2] - k[2] * X[1], k[2] * X[0] - k[0] * X[2], k[0] * X[1] - k[1] * X[0]]
        kd = sum(a * b for a, b in zip(k, X))
        Xr = [mpmath.cos(th) * X[i] + mpmath.sin(th) * kx[i] + (1 - mpmath.cos(th)) * kd * k[i] for i in range(3)]
    Xc = [Xr[i] + mpmath.mpf(c[3 + i]) for i in range(3)]
    u = [sum(mpmath.mpf(K[m][j]) * Xc[j] for j in range(3)) for m in range(3)]
    return u[0] / u[2], u[1] / u[2]


def test_jacobian_exact_against_mpmath_50_digits():
    pr = bo.ragged_ba_problem(5, 40, 800, empty_run=False)
    F, P = 40, len(pr["pts0"])
    fi, pi = pr["fi"], pr["pi"]
    rng = np.random.default_rng(0)
    sel = [int(rng.choice(np.flatnonzero(fi == f))) for f in pr["special"]]
    sel += rng.choice(fi.size, 8, replace=False).tolist()
    Jc, Jp = bo.jacobian_exact(_x(pr), pr["K"], F, P, fi[sel], pi[sel], pr["obs"][sel])
    with mpmath.workdps(50):
        for n, o in enumerate(sel):
            c, X = pr["cams"][fi[o]].copy(), pr["pts0"][pi[o]].copy()
            ref = np.zeros((2, 9))
            for k in range(9):
                def f(t, m, k=k):
                    cc, XX = [mpmath.mpf(v) for v in c], [mpmath.mpf(v) for v in X]
                    (cc if k < 6 else XX)[k if k < 6 else k - 6] += t
                    return _mp_project(cc, XX, pr["K"])[m]
                for m in range(2):
                    ref[m, k] = float(mpmath.diff(lambda t: f(t, m), 0))
            got = np.concatenate([Jc[n], Jp[n]], axis=1).astype(np.float64)
            err = np.abs(got - ref).max() / np.abs(ref).max()
            assert err <= 1e-14, (o, fi[o], err)


def test_jacobian_exact_against_central_differences():
    pr = bo.ragged_ba_problem(6, 40, 2000, empty_run=False)
    F, P = 40, len(pr["pts0"])
    x = _x(pr)
    Jc, Jp = bo.jacobian_exact(x, pr["K"], F, P, pr["fi"], pr["pi"], pr["obs"])
    Jco, Jpo = bo.jacobian_fd(x, pr["K"], F, P, pr["fi"], pr["pi"], pr["obs"])
    # the tolerances tests/test_gpu_parity.py applies to central differences with h = 1e-6
    np.testing.assert_allclose(Jc.astype(float), Jco, rtol=2e-6, atol=5e-4)
    np.testing.assert_allclose(Jp.astype(float), Jpo, rtol=2e-6, atol=5e-4)
    # and the long-double residual agrees with point_fun
    r = bo.point_fun_exact(x, pr["K"], F, P, pr["fi"], pr["pi"], pr["obs"])
    np.testing.assert_allclose(r.astype(float).ravel(), bo.point_fun(x, pr["K"], F, P, pr["fi"], pr["pi"], pr["obs"]),
                               rtol=0, atol=1e-9)


def _dense_J(Jc, Jp, fi, pi, F, P):
    O = len(fi)
    J = np.zeros((2 * O, 6 * F + 3 * P))
    for o in range(O):
        J[2 * o:2 * o + 2, 6 * fi[o]:6 * fi[o] + 6] = Jc[o]
        J[2 * o:2 * o + 2, 6 * F + 3 * pi[o]:6 * F + 3 * pi[o] + 3] = Jp[o]
    return J


@pytest.mark.parametrize("kind", ["uniform", "ragged"])
def test_reduced_system_equals_dense_schur_complement(kind):
    if kind == "uniform":
        pr = synth.make_ba_problem(10, 120, 4, seed=2)
        pr["cams"] = bo.frame_parameters(pr["ext"]).reshape(10, 6)
        F = 10
    else:
        pr = bo.ragged_ba_problem(7, 24, 150, max_len=8, empty_run=False, plant=False)     # (dense: small)
        F = 24
    P = len(pr["pts0"])
    fi, pi = pr["fi"], pr["pi"]
    x = _x(pr)
    Jc, Jp = bo.jacobian_exact(x, pr["K"], F, P, fi, pi, pr["obs"])
    res = bo.point_fun_exact(x, pr["K"], F, P, fi, pi, pr["obs"])
    nb = bo.normal_blocks(Jc, Jp, res, fi, pi, F, P)
    J = _dense_J(Jc.astype(float), Jp.astype(float), fi, pi, F, P)
    H = J.T @ J
    g = J.T @ res.astype(float).ravel()
    nc = 6 * F
    for f in range(F):
        np.testing.assert_allclose(nb["B"][f].astype(float), H[6 * f:6 * f + 6, 6 * f:6 * f + 6], rtol=1e-12,
                                   atol=1e-12 * np.abs(H).max())
    np.testing.assert_allclose(nb["gc"].astype(float).ravel(), g[:nc], rtol=1e-10, atol=1e-10 * np.abs(g).max())
    si = bo.jac_scale(nb["B"].astype(float), nb["C"].astype(float))
    reg = 1e-3
    Bd, Cd = bo.damp(nb["B"], nb["C"], si, reg)
    Hd = H + reg * np.diag(si ** 2)
    rs = bo.reduced_system(Jc, Jp, fi, pi, F, P, Bd, Cd, nb["gc"], nb["gp"])
    Hcc, Hcp, Hpp = Hd[:nc, :nc], Hd[:nc, nc:], Hd[nc:, nc:]
    So = Hcc - Hcp @ np.linalg.solve(Hpp, Hcp.T)
    vo = g[:nc] - Hcp @ np.linalg.solve(Hpp, g[nc:])
    np.testing.assert_allclose(rs["S"].astype(float), So, rtol=1e-9, atol=1e-11 * np.abs(So).max())
    np.testing.assert_allclose(rs["v"].astype(float), vo, rtol=1e-9, atol=1e-11 * np.abs(vo).max())
    assert (rs["S_abs"] >= np.abs(rs["S"])).all() and (rs["v_abs"] >= np.abs(rs["v"])).all()
    # the given-Cinv form uses it as is; back-substitution completes the dense solve
    rs2 = bo.reduced_system(Jc, Jp, fi, pi, F, P, Bd, None, nb["gc"], nb["gp"], Cinv=rs["Cinv"])
    assert np.array_equal(rs2["S"], rs["S"]) and np.array_equal(rs2["v"], rs["v"])
    dc = np.linalg.solve(rs["S"].astype(float), rs["v"].astype(float))
    dp, _, _ = bo.backsub(Jc, Jp, fi, pi, P, rs["Cinv"], nb["gp"], dc)
    sol = np.linalg.solve(Hd, g)
    np.testing.assert_allclose(np.concatenate([dc, dp.astype(float).ravel()]), sol, rtol=1e-7, atol=1e-9 * np.abs(sol).max())


def test_jac_scale_and_damp_equal_scipy():
    from scipy.optimize._lsq.common import compute_jac_scale
    pr = bo.ragged_ba_problem(8, 20, 100, max_len=6, empty_run=False, plant=False)
    F, P = 20, len(pr["pts0"])
    fi, pi = pr["fi"], pr["pi"]
    Jc, Jp = bo.jacobian_exact(_x(pr), pr["K"], F, P, fi, pi, pr["obs"], dtype=np.complex128)
    Jc[:, :, 5][fi == 3] = 0.0          # a column of zeros: the first call sets its scale to 1
    J = _dense_J(Jc, Jp, fi, pi, F, P)
    B = np.zeros((F, 6, 6))
    np.add.at(B, fi, np.einsum("omi,omj->oij", Jc, Jc))
    C = np.zeros((P, 3, 3))
    np.add.at(C, pi, np.einsum("omi,omj->oij", Jp, Jp))
    C6 = C[:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]]
    _, si_ref = compute_jac_scale(J)
    si = bo.jac_scale(B, C6)
    # the same sums of squares in another order: k eps relative, k = the most rows of any column
    k = max(np.bincount(fi).max(), np.bincount(pi).max()) * 2
    tol = k * np.finfo(float).eps
    np.testing.assert_allclose(si, si_ref, rtol=tol, atol=0)
    assert si[6 * 3 + 5] == 1.0
    assert np.array_equal(bo.jac_scale(B, C), si)
    old = si * np.where(np.arange(si.size) % 2 == 0, 1.5, 0.5)
    _, si2_ref = compute_jac_scale(J, old)
    np.testing.assert_allclose(bo.jac_scale(B, C6, old), si2_ref, rtol=tol, atol=0)
    Bd, Cd = bo.damp(B, C6, si, 1e-3)
    H = J.T @ J + 1e-3 * np.diag(si ** 2)
    for f in range(F):
        blk = H[6 * f:6 * f + 6, 6 * f:6 * f + 6]
        np.testing.assert_allclose(Bd[f].astype(float), blk, rtol=tol, atol=tol * np.abs(blk).max())
    Cd3 = bo.unpack_sym3(Cd).astype(float)
    for p in range(P):
        q = 6 * F + 3 * p
        np.testing.assert_allclose(Cd3[p], H[q:q + 3, q:q + 3], rtol=tol, atol=tol * np.abs(H[q:q + 3, q:q + 3]).max())
