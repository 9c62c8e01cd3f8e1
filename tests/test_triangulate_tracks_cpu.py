"""CPU: a NumPy restatement of mm_triangulate_tracks (include/meatmodeler.h) and the numbers the GPU test relies on.

The restatement follows the header's definition step by step -- A^T A of the unnormalised rows, cyclic Jacobi, a fixed number
of Levenberg-Marquardt trial steps, the four quality columns and the flags -- and is checked here against independent
references: the SVD of the stacked rows for the linear stage and scipy.optimize.least_squares driven to 1e-15 tolerances for
the refinement.  tests/test_triangulate_tracks_gpu.py imports the helpers of this module.
"""
import numpy as np
from scipy.optimize import least_squares

from meatmodeler_amd import synth

RADIUS = 6.0
BEHIND, REPROJ, PARALLAX, DEGENERATE = 1, 2, 4, 8      # MM_TRI_*


# ------------------------------------------------------------------------------------------------ the restatement

def rows_of(proj, frames, xy):
    """The stacked [2m, 4] system: x P[2] - P[0] and y P[2] - P[1] per observation (unnormalised)."""
    P = proj[frames]
    return np.concatenate([xy[:, :1] * P[:, 2] - P[:, 0], xy[:, 1:] * P[:, 2] - P[:, 1]], axis=1).reshape(-1, 4)


def jacobi_smallest(M):
    """Eigenvector of the smallest eigenvalue of a symmetric 4 x 4 by cyclic Jacobi; a rotation is skipped once
    |a_pq| <= eps sqrt(a_pp a_qq)."""
    A = np.array(M, float)
    V = np.eye(4)
    eps = np.finfo(float).eps
    for _ in range(30):
        rotated = False
        for p in range(3):
            for q in range(p + 1, 4):
                apq = A[p, q]
                if abs(apq) > eps * np.sqrt(abs(A[p, p] * A[q, q])) and apq != 0.0:
                    rotated = True
                    zeta = (A[q, q] - A[p, p]) / (2.0 * apq)
                    t = np.copysign(1.0, zeta) / (abs(zeta) + np.sqrt(1.0 + zeta * zeta))
                    c = 1.0 / np.sqrt(1.0 + t * t)
                    s = c * t
                    G = np.eye(4)
                    G[p, p] = G[q, q] = c
                    G[p, q], G[q, p] = s, -s
                    A = G.T @ A @ G
                    A[p, q] = A[q, p] = 0.0
                    V = V @ G
        if not rotated:
            break
    return V[:, int(np.argmin(np.diag(A)))]


def linear_point(proj, frames, xy):
    A = rows_of(proj, frames, xy)
    v = jacobi_smallest(A.T @ A)
    with np.errstate(all="ignore"):
        return v[:3] / v[3]


def residuals(proj, frames, xy, X):
    """r [m,2], w [m], u [m,2] at X."""
    P = proj[frames]
    h = P[:, :, :3] @ X + P[:, :, 3]
    with np.errstate(all="ignore"):
        u = h[:, :2] / h[:, 2:3]
    return u - xy, h[:, 2], u


def normal_equations(proj, frames, xy, X):
    """(cost, H, g): sum |r|^2, sum J^T J, sum J^T r with J = (P[:2, :3] - u P[2, :3]) / w."""
    P = proj[frames]
    r, w, u = residuals(proj, frames, xy, X)
    with np.errstate(all="ignore"):
        J = (P[:, :2, :3] - u[:, :, None] * P[:, 2:3, :3]) / w[:, None, None]
        return float((r * r).sum()), np.einsum("mki,mkj->ij", J, J), np.einsum("mki,mk->i", J, r)


def refine_point(proj, frames, xy, X, iters):
    """`iters` trial steps of Levenberg-Marquardt from X -> (X, [cost after every trial step, the start first])."""
    X = np.array(X, float)
    cost, H, g = normal_equations(proj, frames, xy, X)
    costs = [cost]
    lam = 1e-3
    for _ in range(iters):
        accept = False
        try:
            with np.errstate(all="ignore"):
                L = np.linalg.cholesky(H + lam * np.diag(np.diag(H)))      # raises on a pivot that is not positive
                d = np.linalg.solve(L.T, np.linalg.solve(L, -g))
            Xn = X + d
            cn, Hn, gn = normal_equations(proj, frames, xy, Xn)
            accept = bool(np.isfinite(cn) and cn < cost)
        except np.linalg.LinAlgError:
            pass
        if accept:
            X, cost, H, g = Xn, cn, Hn, gn
            lam = max(lam / 10.0, 1e-12)
        else:
            lam *= 10.0
        costs.append(cost)
    return X, costs


def camera_centres(proj):
    return np.stack([-np.linalg.solve(P[:, :3], P[:, 3]) for P in proj])


def quality_at(proj, frames, xy, X):
    """(rms_px, max_px, min_depth, cos_parallax) at X; NaN for a track of fewer than two observations or a non-finite X."""
    m = len(frames)
    if m < 2 or not np.all(np.isfinite(X)):
        return np.full(4, np.nan)
    r, w, _ = residuals(proj, frames, xy, X)
    rn = np.sqrt((r * r).sum(axis=1))
    C = camera_centres(proj[frames])
    a = C[0] - X
    b = C[1:] - X
    cosv = (b @ a) / np.sqrt((a @ a) * (b * b).sum(axis=1))
    depth = w / np.linalg.norm(proj[frames][:, 2, :3], axis=1)
    return np.array([np.sqrt((rn * rn).sum() / m), rn.max(), depth.min(), cosv.min()])


def flags_of(quality, lens, X, max_reproj_px=np.inf, max_cos_parallax=2.0, min_depth=-np.inf):
    """The thresholds applied to quality columns [T,4] (NaN compares false) + DEGENERATE from m < 2 / non-finite X."""
    with np.errstate(invalid="ignore"):
        fl = np.where(quality[:, 2] <= min_depth, BEHIND, 0)
        fl |= np.where(quality[:, 1] > max_reproj_px, REPROJ, 0)
        fl |= np.where(quality[:, 3] > max_cos_parallax, PARALLAX, 0)
    fl |= np.where((np.asarray(lens) < 2) | ~np.isfinite(X).all(axis=1), DEGENERATE, 0)
    return fl.astype(np.int32)


def triangulate_tracks_numpy(proj, track_ptr, obs_frame, obs_xy, refine_iters):
    """The whole definition over a CSR of tracks -> X [T,3] (a degenerate track is not refined)."""
    T = len(track_ptr) - 1
    X = np.empty((T, 3))
    for t in range(T):
        s = slice(track_ptr[t], track_ptr[t + 1])
        fr, xy = obs_frame[s], obs_xy[s]
        if len(fr) == 0:
            X[t] = np.nan
            continue
        x = linear_point(proj, fr, xy)
        if len(fr) >= 2 and np.all(np.isfinite(x)) and refine_iters:
            x, _ = refine_point(proj, fr, xy, x, refine_iters)
        X[t] = x
    return X


# ------------------------------------------------------------------------------------------------ independent references

def svd_point(proj, frames, xy):
    v = np.linalg.svd(rows_of(proj, frames, xy))[2][-1]
    return v[:3] / v[3]


def scipy_point(proj, frames, xy, X0):
    """The minimiser of sum |pi(P X) - x|^2 from X0, least_squares at 1e-15 tolerances."""
    P = proj[frames]

    def fun(X):
        return residuals(proj, frames, xy, X)[0].ravel()

    def jac(X):
        _, w, u = residuals(proj, frames, xy, X)
        return ((P[:, :2, :3] - u[:, :, None] * P[:, 2:3, :3]) / w[:, None, None]).reshape(-1, 3)

    return least_squares(fun, X0, jac=jac, method="lm", ftol=1e-15, xtol=1e-15, gtol=1e-15, max_nfev=2000).x


# ------------------------------------------------------------------------------------------------ scenes

def orbit_projections(n_frames, deg_per_frame=1.8, radius=RADIUS):
    K = synth.default_K()
    ext = synth.orbit_cameras(n_frames, arc_deg=deg_per_frame * n_frames, radius=radius)
    return np.einsum("ij,fjk->fik", K, ext)


def project(proj, frames, X):
    h = proj[frames][:, :, :3] @ X + proj[frames][:, :, 3]
    return h[:, :2] / h[:, 2:3]


def make_tracks(proj, lengths, rng, sigma=0.5, consecutive=True):
    """One track per entry of `lengths`: a true point in [-1, 1]^3 seen from `length` consecutive frames from a random
    start, pixel noise sigma -> CSR (track_ptr [T+1] i32, obs_frame [O] i32, obs_xy [O,2] f64) and the true points."""
    F = len(proj)
    ptr, frames, xy, truth = [0], [], [], []
    for m in lengths:
        start = int(rng.integers(0, F - m + 1))
        fr = np.arange(start, start + m)
        X = rng.uniform(-1.0, 1.0, 3)
        frames.append(fr)
        xy.append(project(proj, fr, X) + rng.normal(0.0, sigma, (m, 2)))
        truth.append(X)
        ptr.append(ptr[-1] + m)
    return (np.array(ptr, np.int32), np.concatenate(frames).astype(np.int32), np.concatenate(xy), np.array(truth))


def cpu_scene():
    proj = orbit_projections(40)
    rng = np.random.default_rng(11)
    lengths = [m for m in (2, 3, 4, 5, 8, 16, 33, 40) for _ in range(25)]
    return (proj,) + make_tracks(proj, lengths, rng)


# ------------------------------------------------------------------------------------------------ the tests

def test_linear_stage_equals_svd_of_the_stacked_rows():
    proj, tp, fr, xy, _ = cpu_scene()
    worst = 0.0
    for t in range(len(tp) - 1):
        s = slice(tp[t], tp[t + 1])
        worst = max(worst, np.abs(linear_point(proj, fr[s], xy[s]) - svd_point(proj, fr[s], xy[s])).max())
    print(f"linear stage against the SVD: {worst / RADIUS:.3e} of the radius")
    assert worst <= 1e-9 * RADIUS


def test_eight_trial_steps_reach_the_minimiser_and_never_raise_the_cost():
    proj, tp, fr, xy, _ = cpu_scene()
    worst = 0.0
    for t in range(len(tp) - 1):
        s = slice(tp[t], tp[t + 1])
        x0 = linear_point(proj, fr[s], xy[s])
        x8, costs = refine_point(proj, fr[s], xy[s], x0, 8)
        assert len(costs) == 9 and all(b <= a for a, b in zip(costs, costs[1:])), (t, costs)
        worst = max(worst, np.abs(x8 - scipy_point(proj, fr[s], xy[s], x0)).max())
    print(f"eight trial steps against least_squares: {worst / RADIUS:.3e} of the radius")
    assert worst <= 1e-6 * RADIUS


def test_whole_definition_and_flags_on_degenerate_input():
    proj, tp, fr, xy, _ = cpu_scene()
    # two tracks appended: one observation; two observations through one projection matrix
    tp2 = np.concatenate([tp, [tp[-1] + 1, tp[-1] + 3]]).astype(np.int32)
    fr2 = np.concatenate([fr, [3, 7, 7]]).astype(np.int32)
    xy2 = np.concatenate([xy, [[900.0, 500.0], [800.0, 400.0], [810.0, 420.0]]])
    X = triangulate_tracks_numpy(proj, tp2, fr2, xy2, 8)
    T = len(tp2) - 1
    lens = np.diff(tp2)
    q = np.stack([quality_at(proj, fr2[tp2[t]:tp2[t + 1]], xy2[tp2[t]:tp2[t + 1]], X[t]) for t in range(T)])
    fl = flags_of(q, lens, X, max_reproj_px=4.0, max_cos_parallax=np.cos(np.radians(1.0)), min_depth=0.0)
    assert fl[T - 2] & DEGENERATE and np.isnan(quality_at(proj, fr2[-3:-2], xy2[-3:-2], X[T - 2])).all()
    assert bool(fl[T - 1] & DEGENERATE) == (not np.isfinite(X[T - 1]).all())
    clean = fl[:T - 2]
    assert not (clean & (BEHIND | DEGENERATE)).any()
    assert (q[:T - 2, 2] > 3.0).all() and (q[:T - 2, 0] <= q[:T - 2, 1] + 1e-12).all()
