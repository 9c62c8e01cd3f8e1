"""Drop-in for the reference's ``bundleAdjuster.py`` — same public names, argument and return conventions.

The reference hands its cost function to ``scipy.optimize.least_squares`` (TRF, ``jac_sparsity``,
``x_scale='jac'``, ``ftol=1e-4``; bundleAdjuster.py:180-192).  SciPy then differentiates numerically and solves
each damped Gauss-Newton system with LSMR (scipy/optimize/_lsq/trf.py:401-560).  Here the same trust-region
iteration (`trf_no_bounds`: Jacobian column scaling with running max, Cauchy-derived regulariser, 2-D subspace
trust-region step, ratio test, ftol/xtol/gtol termination) runs with

  * the analytic Jacobian (never materialised) and block normal equations computed by HIP sweeps,
  * the regularised Gauss-Newton system  (J^T J + reg D^-2) q = J^T f  solved EXACTLY through the Schur complement
    onto the cameras (point blocks eliminated, dense 6F x 6F Cholesky on f64 MFMA) instead of iteratively by LSMR.

So the iterates follow SciPy's to within LSMR's own 1e-6 tolerance and the finite-difference error of the reference's
Jacobian; see DESIGN.md §BA for what "parity" means on this gauge-free problem.

The iteration of `adjustPoints` has two drivers, same kernels and bit-identical iterates: the loop inside the C-ABI
library (mm_ba_trf and its fixed-camera and sharded forms; the default) and the device-resident loop sequenced from
here (`SchurTRF._solve_device`).  Either way the 2x2 trust-region subproblem is solved on the device; host Python
only sequences launches and takes the accept / reject / terminate decisions (`_TrfDecide`) from one small board of
scalars per trial step.  torch is used for device buffers.
"""
import math
import os
import time
import warnings

import numpy as np
import torch
from numpy.linalg import norm as _norm
from scipy.sparse import csr_matrix

from . import ops
from ._lib import default_context, MMError

EPS = np.finfo(float).eps


# ----------------------------------------------------------------------------------------------- small helpers

def _rodrigues_matrix(rvec):
    """Axis-angle -> R, the closed form cv2.Rodrigues evaluates at bundleAdjuster.py:153,201."""
    r = np.asarray(rvec, float).reshape(3)
    th2 = float(r @ r)
    th = np.sqrt(th2)
    Kx = np.array([[0.0, -r[2], r[1]], [r[2], 0.0, -r[0]], [-r[1], r[0], 0.0]])
    if th < 1e-8:
        a, b = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0
    else:
        a, b = np.sin(th) / th, (1.0 - np.cos(th)) / th2
    return np.eye(3) + a * Kx + b * (Kx @ Kx)


def frameParameters(frame_extrinsic_matrices):
    """[F,3|4,4] -> [6F] rows (rvec, tvec) (bundleAdjuster.py:105-134): theta = arccos((tr R - 1)/2) without
    clipping, axis = skew part / (2 sin theta) with 0/0 -> 0, r = axis * theta.  O(F) host glue."""
    E = np.asarray(frame_extrinsic_matrices, float)
    R = E[:, :3, :3]
    with np.errstate(invalid="ignore", divide="ignore"):
        theta = np.arccos((np.trace(R, axis1=1, axis2=2) - 1.0) * 0.5)
        two_s = 2.0 * np.sin(theta)
        axis = np.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], 1) / two_s[:, None]
        rvec = np.nan_to_num(axis) * theta[:, None]
    return np.concatenate([rvec, E[:, :3, 3]], axis=1).reshape(-1)


def pointAdjustmentSparsity(n_frames, n_points, frame_indices, point_indices):
    """Jacobian sparsity structure (bundleAdjuster.py:55-78) as CSR: observation i owns rows 2i, 2i+1 with ones in its
    camera's 6 and its point's 3 columns.  The HIP path never needs it (the block layout is implicit); provided for
    callers that used it."""
    fi = np.asarray(frame_indices).astype(np.int64)
    pi = np.asarray(point_indices).astype(np.int64)
    O = fi.size
    cols = np.empty((O, 2, 9), np.int64)
    cols[:, :, :6] = (6 * fi)[:, None, None] + np.arange(6)
    cols[:, :, 6:] = (6 * n_frames + 3 * pi)[:, None, None] + np.arange(3)
    return csr_matrix((np.ones(18 * O, dtype=int), cols.reshape(-1), np.arange(0, 18 * O + 1, 9)),
                      shape=(2 * O, 6 * n_frames + 3 * n_points))


def _dev(x, device):
    return torch.as_tensor(np.ascontiguousarray(x, np.float64)).to(device)


def project(points, frame_params, camera_matrix):
    """points [n,3], frame_params [n,6] -> pixels [n,2] on the device (bundleAdjuster.py:31-52): the residual sweep
    with zero observations and identity index maps."""
    ctx = default_context()
    n = len(points)
    ar = np.arange(n, dtype=np.int32)
    pb = ops.BADevice(camera_matrix, ar, ar, np.zeros((n, 2)), n, n, ctx.device, ctx)
    _, res = pb.residual(_dev(np.asarray(frame_params, float)[:, :6], ctx.device), _dev(points, ctx.device), True)
    return res.cpu().numpy()


def rotate(points, rot_vecs):
    """Rodrigues rotation of points by per-row axis-angle vectors (bundleAdjuster.py:7-28).  Not on the hot path (the
    sweeps fuse it); evaluated through `project` with K = I after translating by +t0 to keep z away from zero is NOT
    possible in general, so this helper uses device tensor algebra."""
    ctx = default_context()
    X = _dev(points, ctx.device)
    r = _dev(rot_vecs, ctx.device)
    th = r.norm(dim=1, keepdim=True)
    k = torch.where(th > 0, r / torch.where(th > 0, th, torch.ones_like(th)), torch.zeros_like(r))
    c, s = torch.cos(th), torch.sin(th)
    out = c * X + s * torch.cross(k, X, dim=1) + (k * X).sum(1, keepdim=True) * (1 - c) * k
    return out.cpu().numpy()


def pointFun(parameters, camera_matrix, n_frames, n_points, frame_indices, point_indices, points_2D):
    """Residual vector [2*O] (bundleAdjuster.py:81-102) from the HIP residual sweep."""
    ctx = default_context()
    parameters = np.asarray(parameters, float)
    pb = ops.BADevice(camera_matrix, frame_indices, point_indices, points_2D, n_frames, n_points, ctx.device, ctx)
    cams = _dev(parameters[:6 * n_frames].reshape(n_frames, 6), ctx.device)
    pts = _dev(parameters[6 * n_frames:].reshape(n_points, 3), ctx.device)
    return pb.residual(cams, pts, True)[1].cpu().numpy().ravel()


def poseFun(parameters, camera_intrinsic_matrix, n_frames, frame_indices, point_indices, points_3D, points_2D):
    """Pose-only residuals (bundleAdjuster.py:206-211)."""
    ctx = default_context()
    pb = ops.BADevice(camera_intrinsic_matrix, frame_indices, point_indices, points_2D, n_frames, len(points_3D),
                      ctx.device, ctx)
    cams = _dev(np.asarray(parameters, float).reshape(n_frames, 6), ctx.device)
    return pb.residual(cams, _dev(points_3D, ctx.device), True)[1].cpu().numpy().ravel()


# ----------------------------------------------------------------------------------------------- trust region (host scalars)

def _update_tr_radius(Delta, actual, predicted, step_norm, bound_hit):
    if predicted > 0:
        ratio = actual / predicted
    elif predicted == actual == 0:
        ratio = 1
    else:
        ratio = 0
    if ratio < 0.25:
        Delta = 0.25 * step_norm
    elif ratio > 0.75 and bound_hit:
        Delta *= 2.0
    return Delta, ratio


def _check_termination(dF, F, dx_norm, x_norm, ratio, ftol, xtol):
    ftol_ok = dF < ftol * F and ratio > 0.25
    xtol_ok = dx_norm < xtol * (xtol + x_norm)
    if ftol_ok and xtol_ok:
        return 4
    if ftol_ok:
        return 2
    if xtol_ok:
        return 3
    return None


class _TrfDecide:
    """The host's decisions of the trust-region solve -- accept / reject / try again / terminate as SciPy's trf_no_bounds
    takes them, plus the rule for raising the damping when the reduced camera system is not positive definite -- stated
    once for the loop sequenced from Python.  The Python statement of csrc/trf_decide.h, method for method and field
    for field (tests/test_trf_decisions_cpu.py replays the same boards through both); see there for a driver's iteration.
    `log` (a list, optional) receives the rows of the verbose=2 table, NaN where SciPy prints nothing."""

    # what the machine answers (the numbers of csrc/trf_decide.h)
    BODY, TRIAL, FINAL, DONE, RETRY, USABLE, ABANDONED, INDEFINITE = range(8)

    def __init__(self, cost, xx_scaled, n, ftol, xtol, gtol, max_nfev=None, min_damping=0.0, log=None):
        self.Delta = math.sqrt(xx_scaled)      # Delta0 = |x * scale_inv|  (trf.py:428)
        if self.Delta == 0:
            self.Delta = 1.0
        self.cost = self.cost0 = cost
        self.x_norm = 0.0
        self.step_norm = self.actual = self.g_norm = float("nan")
        self.min_damping = min_damping if min_damping > 0 else 1e-9
        self.reg = 0.0
        self.nfev = self.njev = 1
        self.iteration = self.attempt = 0
        self.termination = None
        self.max_nfev = max_nfev if max_nfev is not None and max_nfev > 0 else 100 * n
        self.accepted = False
        self.ftol, self.xtol, self.gtol = ftol, xtol, gtol
        self.log, self.n_log = log, 0

    def begin(self):
        return self.FINAL if self.termination is not None or self.nfev == self.max_nfev else self.BODY

    def on_solve(self, info, reg_used, g_norm, xx):
        """The board of an iteration's first trial step: info of the factorisation, the damping it ran with, |g|_inf, |x|^2."""
        if info < 0:
            return self.ABANDONED      # (nothing noted: the driver may issue the same attempt again)
        if info > 0:
            if reg_used <= self.min_damping * (1.0 + 1e-12):      # failed AT the floor: the floor was too low
                self.min_damping *= 100.0
            self.reg = reg_used * 100.0
            self.attempt += 1
            return self.INDEFINITE if self.attempt >= 6 else self.RETRY
        self.attempt = 0
        self.g_norm = g_norm
        if g_norm < self.gtol:      # (checked before the step is used, as trf.py:443 does)
            self.termination = 1
        self._emit_row()
        if self.termination is not None:
            return self.DONE
        self.x_norm = math.sqrt(xx)
        self.actual = -1.0
        return self.USABLE

    def on_trial(self, predicted, step_h_norm, step_norm, cost2_new):
        """A trial step: predicted reduction, |p| in the scaled variables, the unscaled step norm, twice the cost there."""
        cost_new = 0.5 * cost2_new
        self.nfev += 1
        if not math.isfinite(cost_new):
            self.Delta = 0.25 * step_h_norm
        else:
            self.actual = self.cost - cost_new
            Delta_new, ratio = _update_tr_radius(self.Delta, self.actual, predicted, step_h_norm,
                                                 step_h_norm > 0.95 * self.Delta)
            self.step_norm = step_norm
            self.termination = _check_termination(self.actual, self.cost, step_norm, self.x_norm, ratio, self.ftol, self.xtol)
            if self.termination is None:
                self.Delta = Delta_new
        if self.termination is None and self.actual <= 0 and self.nfev < self.max_nfev:
            return self.TRIAL
        self.accepted = self.actual > 0
        if self.accepted:
            self.cost = cost_new
            self.njev += 1
        else:
            self.step_norm = 0.0
            self.actual = 0.0
        self.iteration += 1
        return self.begin()

    def on_final(self, g_norm):
        self.g_norm = g_norm
        self._emit_row()
        return self.DONE

    @property
    def status(self):
        return 0 if self.termination is None else self.termination

    def _emit_row(self):
        if self.log is not None:
            self.log.append((self.iteration, self.nfev, self.cost, self.actual, self.step_norm, self.g_norm))
        self.n_log += 1


_MESSAGES = {-1: "Improper input parameters status returned from `leastsq`",
             0: "The maximum number of function evaluations is exceeded.",
             1: "`gtol` termination condition is satisfied.", 2: "`ftol` termination condition is satisfied.",
             3: "`xtol` termination condition is satisfied.",
             4: "Both `ftol` and `xtol` termination conditions are satisfied."}


def _print_header():
    print("{:^15}{:^15}{:^15}{:^15}{:^15}{:^15}".format("Iteration", "Total nfev", "Cost", "Cost reduction",
                                                          "Step norm", "Optimality"))


def _print_iteration(it, nfev, cost, red, step, opt):
    """One row of the table; None (solvePose) or NaN (the rows of the decision machines) where SciPy prints nothing."""
    red = " " * 15 if red is None or np.isnan(red) else f"{red:^15.2e}"
    step = " " * 15 if step is None or np.isnan(step) else f"{step:^15.2e}"
    print(f"{it:^15}{nfev:^15}{cost:^15.4e}{red}{step}{opt:^15.2e}")


class BAResult:
    def __init__(self, **kw):
        self.__dict__.update(kw)


class SchurTRF:
    """SciPy's trf_no_bounds (tr_solver='lsmr', x_scale='jac', linear loss) with the Gauss-Newton system solved by
    the Schur complement.  `allreduce` (optional) sums partial block quantities across ranks for the sharded path
    (points partitioned over GPUs, cameras replicated): it is called on every tensor that is a sum over
    observations.

    `solve` hands the iteration to one of two drivers: `_solve_library` (the loop inside the C-ABI library) or
    `_solve_device` (the same loop sequenced from Python).  The parameter vector lives in ONE flat device buffer
    x = [cams (6F) | points (3P)] (views are handed to the sweeps), so every axpy / dot of the iteration is a single
    launch, and the host reads one board of device scalars per trial step."""

    def __init__(self, pb, allreduce=None, min_damping=1e-9, driver=None):
        self.pb = pb
        self.allreduce = allreduce
        self.min_damping = min_damping
        # "library": the loop itself runs inside the C-ABI library (mm_ba_trf, mm_ba_trf_fixed, mm_ba_trf_dist); "python":
        # sequenced from here (also what the overlapped build, more than 16 ranks and a problem object without the library
        # entry points -- the CPU stand-in of the tests -- get).  Same kernels, bit-identical iterates.
        self.driver = driver or os.environ.get("MM_TRF_DRIVER", "library")
        self._avoid_fused = False

    # -- reductions that need the cross-rank sum when sharded --
    def _ar(self, *tensors):
        if self.allreduce is not None:
            for t in tensors:
                self.allreduce(t)

    def _cost_dev(self, x):
        c2, _ = self.pb.residual(self._cams(x), self._pts(x))
        self._ar(c2)
        return c2

    def _cost(self, cams, pts):
        c2, _ = self.pb.residual(cams, pts)
        self._ar(c2)
        return 0.5 * float(c2.item())

    def _cams(self, v):
        return v[:self.nc].view(self.pb.F, 6)

    def _pts(self, v):
        return v[self.nc:].view(self.pb.P, 3)

    def _combine(self, rows):
        """rows [k, 3] of a fused pass -> [k] totals (the point part is summed across ranks when sharded)."""
        if self.allreduce is None:
            return rows[:, 2]
        # The camera part is replicated, but its reduction tree depends on the LOCAL vector length (shards differ), so
        # the ranks' copies differ in the last bit.  Rank 0's copy is the one that enters the sum: every rank then
        # holds the same scalars bit for bit, takes the same accept / reject / terminate decisions and stays inside the
        # same sequence of collectives.
        t = (rows[:, 0] + rows[:, 1]) if self.allreduce.rank == 0 else rows[:, 1].clone()
        t = t.contiguous()
        self.allreduce(t)
        return t

    def _fix_params(self, rows, k, max_row=None):
        """result rows of a pass over the PARAMETER vector: column 2 <- cross-rank total (camera part replicated)."""
        if self.allreduce is None:
            return rows
        rows[:k, 2] = self._combine(rows[:k])
        if max_row is not None:
            m = rows[max_row, 1:2].contiguous()
            self.allreduce(m, op="max")
            rows[max_row, 2:3] = torch.maximum(rows[max_row, 0:1], m)
        return rows

    def _fix_residual(self, rows):
        """result rows of inner products of RESIDUAL-space vectors (every rank holds its own observations)."""
        if self.allreduce is None:
            return rows
        t = rows[:, 2].contiguous()
        self.allreduce(t)
        rows[:, 2] = t
        return rows

    def _normal(self, x, g, B, C):
        """Block normal equations at x: the sweeps write into the persistent blocks B / C and put g_c / g_p straight into
        the two halves of the flat gradient g.  Camera blocks are sums over all observations; point blocks are local."""
        self.pb.normal_eq(self._cams(x), self._pts(x), out=(B, self._cams(g), C, self._pts(g)))
        self._ar(B, self._cams(g))

    def _reduced_solve(self, x, Bd, Cd, gc, gp, half_bw, band_exchange):
        """-> (info, v = solution of the reduced camera system, Cinv) at the current iterate x."""
        pb, ar = self.pb, self.allreduce
        if ar is None:      # one GPU: S is built and factored in one call (mm_ba_schur_solve)
            return pb.schur_solve(self._cams(x), self._pts(x), Bd, Cd, gc, gp, half_bw)
        S, v, Cinv = pb.schur(self._cams(x), self._pts(x), Bd, Cd, gc, gp)
        ws = ar.world_size
        if band_exchange:
            # only the lower band is exchanged: n x (hb + 1) doubles (12.7 MB at 500 cameras) instead of the dense 72 MB
            band = pb.band_view(half_bw)
            packed = band.contiguous()
            ar(packed)
            band.copy_(packed)
        else:
            ar(S)
        ar(v)
        if ws > 1:      # every rank added the full blockdiag(Bd) and gc: remove the duplicates after the sum
            blk = S.reshape(pb.F, 6, pb.F, 6)
            f = torch.arange(pb.F, device=pb.device)
            blk[f, :, f, :] -= (ws - 1) * Bd
            v -= (ws - 1) * gc.reshape(-1)
        # after a band exchange only the lower band is the sum; the dense exchange sums everything
        info = pb.chol_solve_sym(S, v, half_bw, both_triangles=not band_exchange)
        return info, v, Cinv

    def _serial_fallback(self):
        warnings.warn("mm_ba_schur_solve: kernels are being serialised; building and solving the reduced system one "
                      "after the other from here on")
        self.pb.overlap = False

    def solve(self, cams0, pts0, ftol=1e-4, xtol=1e-8, gtol=1e-8, max_nfev=None, verbose=0, local_points_norm=None):
        pb, ar = self.pb, self.allreduce
        self.nc = nc = 6 * pb.F
        f64 = dict(dtype=torch.float64, device=pb.device)
        x = torch.cat([cams0.reshape(-1), pts0.reshape(-1)]).to(**f64).contiguous()
        # the one thing a problem object may lack: the library's entry points (trf_solve and trf_solve_dist come together)
        library = self.driver == "library" and hasattr(pb, "trf_solve")
        if pb.F_fixed:      # fixed cameras: the library loop only (mm_ba_trf_fixed)
            if self.driver != "library" or ar is not None:
                raise NotImplementedError("fixed cameras: only the library driver on one GPU (mm_ba_trf_fixed)")
            return self._solve_library(x, ftol, xtol, gtol, max_nfev, verbose)
        if library and ar is None and not pb.overlap:      # (the overlapped build is sequenced from Python)
            return self._solve_library(x, ftol, xtol, gtol, max_nfev, verbose)
        cost = 0.5 * float(self._cost_dev(x).item())
        if not np.isfinite(cost):
            raise ValueError("Residuals are not finite in the initial point.")
        # band of the reduced camera system: |camera i - camera j| <= span  ->  |row - col| <= 6 span + 5
        span = torch.tensor([float(pb.cam_span)], **f64)
        if ar is not None:
            ar(span, op="max")
        span_all = int(span.item())
        half_bw = 6 * span_all + 5
        # Sharded: what is exchanged for the reduced camera system is decided from GLOBAL quantities only, so that every
        # rank enters the same collective with the same size whatever its own shard looks like (a rank whose points
        # include one very long track, or no observation at all, builds S with the general kernel; the others with the
        # pair-list kernel).  Every rank's S is zero outside the lower band |i - j| <= half_bw or symmetric inside it,
        # so the packed band [n, half_bw + 1] carries everything the factorisation reads.
        band_exchange = ar is not None and span_all <= pb.max_band_span and half_bw < nc
        if library and ar is not None and ar.world_size <= 16:
            # sharded: the same library loop, with this process group's all-reduce as its callback (mm_ba_trf_dist)
            return self._solve_library(x, ftol, xtol, gtol, max_nfev, verbose, dist=(half_bw, band_exchange))
        return self._solve_device(x, cost, half_bw, band_exchange, ftol, xtol, gtol, max_nfev, verbose)

    def _result(self, td, x, seg):
        return BAResult(cams=self._cams(x).clone(), pts=self._pts(x).clone(), cost=td.cost, optimality=td.g_norm,
                        nfev=td.nfev, njev=td.njev, status=td.status, message=_MESSAGES[td.status], success=td.status > 0,
                        iterations=td.iteration, host_segments_ms={k: 1e3 * v for k, v in seg.items()})

    def _solve_library(self, x, ftol, xtol, gtol, max_nfev, verbose, dist=None):
        """The whole loop of `_solve_device` inside the library: mm_ba_trf on one GPU, mm_ba_trf_dist (dist = (half
        bandwidth, band exchange), both decided from all-reduced quantities) when the points are sharded over ranks
        (csrc/trf.hip)."""
        nc = self.nc
        cams, pts = x[:nc], x[nc:]
        t0 = time.perf_counter()
        if dist is None:
            rep, rows = self.pb.trf_solve(cams, pts, ftol, xtol, gtol, max_nfev, self.min_damping,
                                          log_cap=4096 if verbose == 2 else 0)
        else:
            rep, rows = self.pb.trf_solve_dist(cams, pts, ftol, xtol, gtol, self.allreduce, dist[0], dist[1], max_nfev,
                                               self.min_damping, log_cap=4096 if verbose == 2 else 0)
        self.min_damping = rep.min_damping
        if verbose == 2:
            _print_header()
            for row in rows:
                _print_iteration(*row)
            if rep.log_rows > len(rows):
                print(f"... ({rep.log_rows - len(rows)} more iterations)")
        return BAResult(cams=self._cams(x).clone(), pts=self._pts(x).clone(), cost=rep.cost, optimality=rep.optimality,
                        nfev=rep.nfev, njev=rep.njev, status=rep.status, message=_MESSAGES[rep.status],
                        success=rep.status > 0, iterations=rep.iterations, chol_fallbacks=rep.chol_fallbacks,
                        collectives=rep.collectives,
                        host_segments_ms={"library": 1e3 * (time.perf_counter() - t0)})

    def _solve_device(self, x, cost, half_bw, band_exchange, ftol, xtol, gtol, max_nfev, verbose):
        """The iteration sequenced from Python, with everything device resident: block scaling and damping are single
        launches on persistent buffers, the 2-D trust-region subproblem is solved by a kernel from the fused passes'
        results (mm_trf_step2d), the trial point is formed from its output and the host reads one small board of scalars
        per trial step -- after the trial cost is known.  Sharded (points partitioned over ranks): every sum over
        observations / points is all-reduced on the device before the next kernel reads it (the "total" column of the
        fused passes' result rows is overwritten with the cross-rank total), so all ranks feed identical scalars to
        identical kernels and read identical boards."""
        pb, ar = self.pb, self.allreduce
        F, P, nc = pb.F, pb.P, self.nc
        n = nc + 3 * P
        f64 = dict(dtype=torch.float64, device=pb.device)
        cams, pts = self._cams, self._pts
        g, si = torch.empty(n, **f64), torch.empty(n, **f64)
        B, C = torch.empty((F, 6, 6), **f64), torch.empty((P, 6), **f64)
        Bd, Cd = torch.empty((F, 6, 6), **f64), torch.empty((P, 6), **f64)
        self._normal(x, g, B, C)
        pb.scale_update(B, C, si, True)      # si = sqrt of the block diagonals of J^T J, zeros -> 1
        xs = x * si
        # every decision from here on is the machine's; this loop does the device work its answers ask for
        td = _TrfDecide(cost, float(self._fix_params(pb.multi_dot([(xs, xs)], nc), 1)[0, 2].item()), n, ftol, xtol, gtol,
                        max_nfev, self.min_damping, log=[] if verbose == 2 else None)
        del xs
        gh, ghs, gn, q1, w, q2, s1, s2, x_new = (torch.empty_like(g) for _ in range(9))
        board = torch.zeros(16, **f64)
        cost_slot = board[14:15]
        if verbose == 2:
            _print_header()
        # wall time between the host synchronisation points of an iteration (the syncs drain the stream, so these are real
        # intervals): normal equations, damping, Schur, Cholesky, subspace, first trial step .. sync | further trial steps
        seg = {"to_syncA": 0.0, "syncA_to_accept": 0.0}
        t_mark = time.perf_counter()
        state = td.begin()
        # an abandoned single-launch factorisation switches THIS solve to the launch-per-column path; the context's setting
        # (normally the shared default context) and this object's flag are restored on the way out, as trf.hip's
        # FusedGuard does
        has_ctx = getattr(pb, "ctx", None) is not None
        self._avoid_fused = False
        prev_avoid = pb.ctx.control(pb.ctx.CTL_CHOL_AVOID_FUSED, -1) if has_ctx else None
        try:
            while True:
                # g_h = d * g (d = 1 / scale_inv) and d * g_h in one pass that also yields |g_h|^2 and max |g|
                r0 = self._fix_params(pb.trf_fused(0, [g, si], [gh, ghs], split=nc), 1, max_row=1)
                gh2_t = r0[0, 2:3]
                u1, d11 = pb.jvp_dots(cams(x), pts(x), cams(ghs), pts(ghs))      # J (d g_h) and |J d g_h|^2 in one sweep
                d11 = self._fix_residual(d11)
                if state == _TrfDecide.FINAL:
                    td.on_final(float(r0[1, 2].item()))
                    if verbose == 2:
                        _print_iteration(*td.log[-1])
                    break
                # Cauchy-derived regulariser (trf.py:473-477) computed on the device: the reduced system is built and
                # factored without the host having seen |g|, |g_h| or |J_h g_h| (they arrive with the board).
                # Damped blocks: J^T J + reg * D^-2  (D^-2 = scale_inv^2).  No gauge is fixed (as in the reference), so
                # J^T J has a 7-dimensional null space and only the damping makes the reduced system definite; SciPy's
                # LSMR copes with a singular system, a Cholesky factorisation needs `reg` to stay above rounding:
                # a floor of 1e-9 (relative to the unit diagonal of the scaled system), x100 on a bad pivot, and the
                # raised floor is kept for the rest of the solve (a system that needed it once needs it again).
                reg_eff = pb.trf_damping(gh2_t, d11[0, 2:3], td.Delta, td.min_damping)[1:2]
                gc, gp = cams(g), pts(g)
                while True:
                    pb.damp(B, C, si, reg_eff, Bd, Cd)      # Bd, Cd = B, C (packed 6) + reg diag(scale_inv^2)
                    info, v, Cinv = self._reduced_solve(x, Bd, Cd, gc, gp, half_bw, band_exchange)
                    # q = [v ; dp] = (J^T J + reg D^-2)^-1 g, the unscaled Gauss-Newton step
                    dp = pb.backsub(cams(x), pts(x), Cinv, gp, v.view(F, 6)).reshape(-1)
                    # orthonormal basis of span{g_h, gn_h} (trf.py:481-482) in three fused passes:
                    #   gn_h = q * scale_inv, q1 = g_h / |g_h|            (+ <q1, gn_h>, |gn_h|^2)
                    #   w = gn_h - <q1, gn_h> q1                            (+ |w|^2)
                    #   q2 = w / |w|, s1 = d q1, s2 = d q2 (unscaled steps) (+ the five step inner products)
                    r1 = self._fix_params(pb.trf_fused(1, [v, dp, si, gh], [gn, q1], [gh2_t], split=nc), 2)
                    r2 = self._fix_params(pb.trf_fused(2, [gn, q1], [w], [r1[0, 2:3]], split=nc), 1)
                    r3 = self._fix_params(pb.trf_fused(3, [w, q1, si, gh, x], [q2, s1, s2], [r2[0, 2:3]], split=nc), 5)
                    # J_h q1 = J (d q1) = u1 / |g_h|: <Jq1, Jq1> = d11 / |g_h|^2, <Jq1, Jq2> = <u1, J s2> / |g_h|
                    _, bs = pb.jvp_dots(cams(x), pts(x), cams(s2), pts(s2), other=u1)      # <J s2, u1>, |J s2|^2
                    bs = self._fix_residual(bs)

                    def trial(Delta_):
                        pb.trf_step2d(r0, d11, r1, r2, r3, bs, reg_eff, info, Delta_, board)
                        pb.trf_fused(5, [x, s1, s2], [x_new], [board], split=nc)
                        pb.residual(cams(x_new), pts(x_new), cost_out=cost_slot)
                        if ar is not None:
                            ar(cost_slot)
                        return board.tolist()                                 # ---- the host sync of a trial step ----

                    vals = trial(td.Delta)       # enqueued before the host knows whether the factorisation succeeded
                    solved = td.on_solve(int(vals[6]), vals[13], vals[10], vals[9])
                    self.min_damping = td.min_damping      # (a raised floor outlives the solve)
                    if solved == _TrfDecide.ABANDONED:
                        # the single-launch factorisation gave up waiting (its workgroups or the producer of S were not
                        # co-resident: another tenant, a profiler attaching mid-run).  Overlapped build: redo this attempt
                        # with the build and the solve one after the other and stay there.
                        if ar is None and pb.overlap:
                            self._serial_fallback()
                            continue
                        if not self._avoid_fused and has_ctx:
                            # otherwise repeat the attempt, same damping, on the launch-per-column factorisation and stay
                            # there for the rest of the solve.  (Sharded: every rank reads the same replicated board... but
                            # info is LOCAL -- a rank-local decision would desynchronise the collectives, so the switch is
                            # only taken on one GPU.)
                            if ar is None:
                                self._avoid_fused = True
                                pb.ctx.control(pb.ctx.CTL_CHOL_AVOID_FUSED, 1)
                                continue
                        raise MMError("mm_chol_solve: the fused banded factorisation was abandoned (info = -1)")
                    if solved != _TrfDecide.RETRY:
                        break
                    reg_eff = torch.full_like(reg_eff, td.reg)
                if solved == _TrfDecide.INDEFINITE:
                    raise MMError(f"reduced camera system is not positive definite (pivot {int(vals[6])})")
                t_now = time.perf_counter()
                seg["to_syncA"] += t_now - t_mark
                t_mark = t_now
                if verbose == 2:
                    _print_iteration(*td.log[-1])
                if solved == _TrfDecide.DONE:      # gtol: the trial point enqueued above is simply dropped
                    break
                state = td.on_trial(vals[2], vals[3], vals[4], vals[14])
                while state == _TrfDecide.TRIAL:      # (the machine says when this iteration needs another trial step)
                    vals = trial(td.Delta)
                    state = td.on_trial(vals[2], vals[3], vals[4], vals[14])
                t_now = time.perf_counter()
                seg["syncA_to_accept"] += t_now - t_mark
                t_mark = t_now
                if td.accepted:
                    x, x_new = x_new, x
                    self._normal(x, g, B, C)
                    pb.scale_update(B, C, si, False)      # running maximum
            return self._result(td, x, seg)
        finally:
            if prev_avoid is not None:
                pb.ctx.control(pb.ctx.CTL_CHOL_AVOID_FUSED, prev_avoid)
            self._avoid_fused = False


def _finish_verbose(res, cost0, verbose):
    if verbose >= 1:
        print(res.message)
        print(f"Function evaluations {res.nfev}, initial cost {cost0:.4e}, final cost {res.cost:.4e}, "
              f"first-order optimality {res.optimality:.2e}.")


def reformatPointResult(result, n_frames, n_points):
    """x -> (points [P,3], list of F 4x4 extrinsics) (bundleAdjuster.py:137-157)."""
    x = np.asarray(result.x, float)
    points = x[n_frames * 6:].reshape((n_points, 3))
    frames = x[:n_frames * 6].reshape((n_frames, 6))
    extrinsics = []
    for rvec, tvec in zip(frames[:, :3], frames[:, 3:]):
        E = np.eye(4)
        E[:3, :3] = _rodrigues_matrix(rvec)
        E[:3, 3] = tvec
        extrinsics.append(E)
    return points, extrinsics


def reformatPoseResult(result, n_frames):
    """x -> list of F 3x4 extrinsics (bundleAdjuster.py:197-203)."""
    fp = np.asarray(result.x, float).reshape((n_frames, 6))
    return [np.hstack((_rodrigues_matrix(r), t.reshape(3, 1))) for r, t in zip(fp[:, :3], fp[:, 3:6])]


def fixed_frame_order(fixed_frames, n_frames):
    """Mask or index list of fixed frames -> (order, new_index): the free frames in their original order, then the fixed
    ones (order [F] = original index of each new camera index); new_index [F] is its inverse.  The free frames become
    cameras 0..F_free-1, fixed frame order[F_free + k] becomes fixed camera k (mm_ba_fixed)."""
    fx = np.asarray(fixed_frames)
    if fx.dtype == bool:
        if fx.shape != (n_frames,):
            raise ValueError(f"fixed_frames: a boolean mask needs {n_frames} entries")
        mask = fx.copy()
    else:
        idx = fx.astype(np.int64).reshape(-1)
        if idx.size and (idx.min() < 0 or idx.max() >= n_frames):
            raise ValueError("fixed_frames: frame index out of range")
        mask = np.zeros(n_frames, bool)
        mask[idx] = True
    order = np.concatenate([np.flatnonzero(~mask), np.flatnonzero(mask)])
    new_index = np.empty(n_frames, np.int64)
    new_index[order] = np.arange(n_frames)
    return order, new_index, int((~mask).sum())


def solvePoints(frame_extrinsic_matrices, camera_intrinsic_matrix, points_3D, points_2D, frame_indices, point_indices,
                ftol=1e-4, xtol=1e-8, gtol=1e-8, max_nfev=None, verbose=2, *, fixed_frames=None):
    """adjustPoints with the optimiser settings exposed; returns the full result object (x, cost, nfev, ...).

    fixed_frames (keyword only): boolean mask or index list over the frames whose extrinsics are observed but not
    adjusted (mm_ba_trf_fixed).  The solve runs over the free frames and all points; res.x and
    res.cams come back in the caller's frame order, the rows of the fixed frames equal to their input parameters."""
    ctx = default_context()
    dev = ctx.device
    ext = np.asarray(frame_extrinsic_matrices, float)
    F = len(ext)
    pts0 = np.asarray(points_3D, float).reshape(-1, 3)
    P = len(pts0)
    with np.errstate(all="ignore"):
        cams0 = frameParameters(ext).reshape(F, 6)
    if fixed_frames is not None:
        return _solve_points_fixed(ctx, cams0, pts0, camera_intrinsic_matrix, points_2D, frame_indices, point_indices,
                                   fixed_frames, ftol, xtol, gtol, max_nfev, verbose)
    pb = ops.BADevice(camera_intrinsic_matrix, frame_indices, point_indices, points_2D, F, P, dev, ctx)
    solver = SchurTRF(pb)
    cams_d, pts_d = _dev(cams0, dev), _dev(pts0, dev)
    cost0 = None
    if verbose >= 1:
        cost0 = solver._cost(cams_d, pts_d)
    res = solver.solve(cams_d, pts_d, ftol=ftol, xtol=xtol, gtol=gtol, max_nfev=max_nfev, verbose=verbose)
    res.x = np.concatenate([res.cams.cpu().numpy().reshape(-1), res.pts.cpu().numpy().reshape(-1)])
    if verbose >= 1:
        _finish_verbose(res, cost0, verbose)
    return res


def _solve_points_fixed(ctx, cams0, pts0, K, points_2D, frame_indices, point_indices, fixed_frames, ftol, xtol, gtol,
                        max_nfev, verbose):
    dev = ctx.device
    F, P = len(cams0), len(pts0)
    order, new_index, F_free = fixed_frame_order(fixed_frames, F)
    if F_free == 0:
        raise ValueError("fixed_frames: every frame is fixed (points-only refinement is not supported)")
    fi = new_index[np.asarray(frame_indices, np.int64).reshape(-1)]
    if not (fi < F_free).any():
        raise ValueError("fixed_frames: no point is observed by a free frame")
    cams_r = cams0[order]
    fixed_d = _dev(np.ascontiguousarray(cams_r[F_free:]), dev)
    pb = ops.BADevice(K, fi.astype(np.int32), point_indices, points_2D, F_free, P, dev, ctx, fixed_cams=fixed_d)
    solver = SchurTRF(pb)
    cams_d, pts_d = _dev(np.ascontiguousarray(cams_r[:F_free]), dev), _dev(pts0, dev)
    cost0 = None
    if verbose >= 1:
        cost0 = solver._cost(cams_d, pts_d)
    res = solver.solve(cams_d, pts_d, ftol=ftol, xtol=xtol, gtol=gtol, max_nfev=max_nfev, verbose=verbose)
    cams = cams0.copy()
    cams[order[:F_free]] = res.cams.cpu().numpy()
    res.cams = torch.as_tensor(cams).to(dev)
    res.x = np.concatenate([cams.reshape(-1), res.pts.cpu().numpy().reshape(-1)])
    if verbose >= 1:
        _finish_verbose(res, cost0, verbose)
    return res


def adjustPoints(frame_extrinsic_matrices, camera_intrinsic_matrix, points_3D, points_2D, frame_indices, point_indices,
                 *, fixed_frames=None):
    """Full bundle adjustment over all cameras and points (bundleAdjuster.py:160-194) with the reference's settings
    (x_scale='jac', ftol=1e-4, verbose=2 progress table).  -> (points [P,3], list of F 4x4 extrinsics).
    fixed_frames: frames kept fixed (see solvePoints); their extrinsics come back as given."""
    res = solvePoints(frame_extrinsic_matrices, camera_intrinsic_matrix, points_3D, points_2D, frame_indices,
                      point_indices, ftol=1e-4, verbose=2, fixed_frames=fixed_frames)
    F = len(frame_extrinsic_matrices)
    return reformatPointResult(res, F, len(np.asarray(points_3D).reshape(-1, 3)))


# ----------------------------------------------------------------------------------------------- filter and re-adjust

REFINE_KEYS = ("max_reproj_px", "min_angle_deg", "min_depth", "min_views", "rounds", "ftol", "max_nfev")


def refine_schedule(**options):
    """The filter-and-re-adjust rounds from their options: max_reproj_px, a number or a sequence with one
    threshold per round, the last one repeated (default (8, 4): a least-squares solve smears each gross outlier over its
    camera's other observations, so the first round is wide and the next one tight); min_angle_deg, min_depth, min_views (the
    tests of ops.filter_observations); rounds (default 2); ftol (default 1e-4) and max_nfev (default None) of the re-solves.
    -> dict(max_reproj_px [rounds], min_angle_deg, min_depth, min_views, rounds, ftol, max_nfev); anything else raises
    ValueError."""
    unknown = set(options) - set(REFINE_KEYS)
    if unknown:
        raise ValueError(f"refine takes {', '.join(REFINE_KEYS)}; not {sorted(unknown)}")
    rounds = options.get("rounds", 2)
    if isinstance(rounds, bool) or not isinstance(rounds, (int, np.integer)) or rounds < 1:
        raise ValueError("refine: rounds must be an integer of at least 1")
    taus = options.get("max_reproj_px", (8.0, 4.0))
    try:
        taus = [float(t) for t in (taus if np.ndim(taus) else [taus])]
    except (TypeError, ValueError):
        raise ValueError("refine: max_reproj_px must be a number or a sequence of numbers") from None
    if not taus:
        raise ValueError("refine: max_reproj_px must not be empty")
    taus = [taus[min(r, len(taus) - 1)] for r in range(int(rounds))]
    tests = {k: options[k] for k in ("min_angle_deg", "min_depth", "min_views") if k in options}
    for tau in taus:      # (every round must have an active test; a NaN or a negative angle ends here too)
        ops.filter_thresholds(max_reproj_px=tau, what="refine", **tests)
    ftol, max_nfev = options.get("ftol", 1e-4), options.get("max_nfev")
    if not (isinstance(ftol, (int, float)) and ftol > 0):
        raise ValueError("refine: ftol must be positive")
    if max_nfev is not None and (isinstance(max_nfev, bool) or not isinstance(max_nfev, (int, np.integer)) or max_nfev < 1):
        raise ValueError("refine: max_nfev must be None or a positive integer")
    return dict(max_reproj_px=taus, rounds=int(rounds), ftol=float(ftol), max_nfev=None if max_nfev is None else int(max_nfev), **tests)


def refine_rounds(pb, res, K, schedule, verbose=0):
    """The rounds after an adjustment `res` of the problem `pb` (an ops.BADevice): filter at the returned cameras and points
    (ops.filter_observations); nothing flagged: stop; otherwise build a BADevice from the compacted arrays and solve again from
    the same cameras and pts[point_map]; up to schedule["rounds"] times (`refine_schedule`).  A round that would keep no
    observation ends the loop without a solve.
    -> dict(ba = the last result, point_map / obs_map into the rows of `pb`, composed across rounds, rounds = [dict(max_reproj_px,
    n_obs, n_points, removed_obs, removed_points, cost_in, cost_out, nfev, status)], obs_flags / pt_flags of the first round, and
    filters = each round's ops.filter_observations result, results = the result of each re-solve)."""
    dev = pb.device
    tests = {k: schedule[k] for k in ("min_angle_deg", "min_depth", "min_views") if k in schedule}
    point_map = torch.arange(pb.P, dtype=torch.int32, device=dev)
    obs_map = torch.arange(pb.O, dtype=torch.int32, device=dev)
    out = dict(ba=res, rounds=[], filters=[], results=[], obs_flags=None, pt_flags=None)
    for tau in schedule["max_reproj_px"]:
        cams, pts = res.cams.reshape(pb.F, 6), res.pts.reshape(pb.P, 3)
        cams_all = cams if pb.fixed_cams is None else torch.cat([cams, pb.fixed_cams])
        flt = ops.filter_observations(cams_all, pts, K, pb, max_reproj_px=tau, ctx=pb.ctx, **tests)
        out["filters"].append(flt)
        if out["obs_flags"] is None:
            out["obs_flags"], out["pt_flags"] = flt["obs_flags"], flt["pt_flags"]
        row = dict(max_reproj_px=tau, n_obs=flt["n_obs"], n_points=flt["n_points"], removed_obs=pb.O - flt["n_obs"],
                   removed_points=pb.P - flt["n_points"], cost_in=None, cost_out=None, nfev=0, status=None)
        out["rounds"].append(row)
        if row["removed_obs"] == 0 and row["removed_points"] == 0:
            break
        point_map, obs_map = point_map[flt["point_map"].long()], obs_map[flt["obs_map"].long()]
        if flt["n_obs"] == 0:
            break
        pb = ops.BADevice(K, flt["fi"], flt["pi"], flt["obs"], pb.F, flt["n_points"], dev, pb.ctx, fixed_cams=pb.fixed_cams)
        pts0 = pts[flt["point_map"].long()].contiguous()
        solver = SchurTRF(pb)
        row["cost_in"] = solver._cost(cams, pts0)
        res = solver.solve(cams, pts0, ftol=schedule["ftol"], max_nfev=schedule["max_nfev"], verbose=verbose)
        row.update(cost_out=res.cost, nfev=res.nfev, status=res.status)
        out["ba"] = res
        out["results"].append(res)
    out.update(point_map=point_map, obs_map=obs_map)
    return out


def filterPoints(points, extrinsics, K, points_2D, frame_indices, point_indices, **thresholds):
    """What adjustPoints returns (points [P,3], F extrinsics) and was given (K, points_2D [O,2], frame_indices, point_indices,
    point-major) judged by ops.filter_observations under `thresholds` (max_reproj_px, min_angle_deg, min_depth, min_views)
    -> (points [P',3], points_2D [O',2], frame_indices [O'], point_indices [O'] renumbered, point_map [P'] = the input index of
    each kept point), NumPy arrays ready for the next adjustPoints."""
    unknown = set(thresholds) - {"max_reproj_px", "min_angle_deg", "min_depth", "min_views"}
    if unknown:
        raise ValueError(f"filterPoints takes max_reproj_px, min_angle_deg, min_depth and min_views; not {sorted(unknown)}")
    ops.filter_thresholds(what="filterPoints", **thresholds)
    ext = np.asarray(extrinsics, float)
    pts = np.ascontiguousarray(np.asarray(points, float).reshape(-1, 3))
    fi = np.asarray(frame_indices).reshape(-1)
    pi = np.asarray(point_indices).reshape(-1)
    obs = np.asarray(points_2D, float).reshape(-1, 2)
    if fi.size != pi.size or obs.shape[0] != fi.size:
        raise ValueError("filterPoints: points_2D, frame_indices and point_indices must have one row per observation")
    if pi.size and (np.diff(pi) < 0).any():
        raise ValueError("filterPoints: the observations are not point-major")
    ctx = default_context()
    dev = ctx.device
    with np.errstate(all="ignore"):
        cams = frameParameters(ext).reshape(len(ext), 6)
    i32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.int32)).to(dev)
    flt = ops.filter_observations(_dev(cams, dev), _dev(pts, dev), K, i32(fi), i32(pi), _dev(obs, dev), ctx=ctx, **thresholds)
    pm = flt["point_map"].cpu().numpy()
    return pts[pm], flt["obs"].cpu().numpy(), flt["fi"].cpu().numpy(), flt["pi"].cpu().numpy(), pm


def refinePoints(frame_extrinsic_matrices, camera_intrinsic_matrix, points_3D, points_2D, frame_indices, point_indices,
                 *, fixed_frames=None, verbose=2, **refine):
    """adjustPoints, then the filter-and-re-adjust rounds of `refine_rounds` under the options of `refine_schedule`
    -> (points [P',3], list of F 4x4 extrinsics, report): adjustPoints' return shape for the points that survived, plus the
    report of refine_rounds with point_map, obs_map, obs_flags and pt_flags as NumPy arrays (the result objects and the
    per-round filter outputs dropped).  fixed_frames: as in adjustPoints; their extrinsics come back as given."""
    schedule = refine_schedule(**refine)
    ctx = default_context()
    dev = ctx.device
    ext = np.asarray(frame_extrinsic_matrices, float)
    F = len(ext)
    pts0 = np.asarray(points_3D, float).reshape(-1, 3)
    with np.errstate(all="ignore"):
        cams0 = frameParameters(ext).reshape(F, 6)
    fi = np.asarray(frame_indices, np.int64).reshape(-1)
    order, F_free, fixed_d = np.arange(F), F, None
    if fixed_frames is not None:
        order, new_index, F_free = fixed_frame_order(fixed_frames, F)
        if F_free == 0:
            raise ValueError("fixed_frames: every frame is fixed (points-only refinement is not supported)")
        fi = new_index[fi]
        fixed_d = _dev(np.ascontiguousarray(cams0[order][F_free:]), dev)
    pb = ops.BADevice(camera_intrinsic_matrix, fi.astype(np.int32), point_indices, points_2D, F_free, len(pts0), dev, ctx,
                      fixed_cams=fixed_d)
    res = SchurTRF(pb).solve(_dev(np.ascontiguousarray(cams0[order][:F_free]), dev), _dev(pts0, dev), ftol=1e-4, verbose=verbose)
    rep = refine_rounds(pb, res, camera_intrinsic_matrix, schedule, verbose=verbose)
    last = rep.pop("ba")
    rep.pop("filters")
    rep.pop("results")
    cams = cams0.copy()
    cams[order[:F_free]] = last.cams.cpu().numpy().reshape(F_free, 6)
    pts = last.pts.cpu().numpy().reshape(-1, 3)
    for k in ("point_map", "obs_map", "obs_flags", "pt_flags"):
        rep[k] = rep[k].cpu().numpy()
    x = np.concatenate([cams.reshape(-1), pts.reshape(-1)])
    return reformatPointResult(BAResult(x=x), F, len(pts)) + (rep,)


# ----------------------------------------------------------------------------------------------- pose-only refinement

def _solve_lsq_trust_region_eig(lam, vg, V, Delta, m, initial_alpha, rtol=0.01, max_iter=10):
    """scipy/optimize/_lsq/common.py:solve_lsq_trust_region expressed through the eigen-decomposition of J^T J.
    The pose-only Jacobian is block diagonal (one 2n x 6 block per camera), so its SVD is the union of the per-camera
    SVDs: singular values s = sqrt(eig(B_f)), right vectors V_f, and s*U^T f = V^T g.
    lam [F,6] eigenvalues, vg [F,6] = V^T g, V [F,6,6]."""
    s2 = np.maximum(lam, 0.0).ravel()
    s = np.sqrt(s2)
    suf = vg.ravel()
    n = s.size

    def phi_and_derivative(alpha):
        denom = s2 + alpha
        p_norm = _norm(suf / denom)
        return p_norm - Delta, -np.sum(suf ** 2 / denom ** 3) / p_norm

    def back(coef):
        return -np.einsum("fij,fj->fi", V, coef.reshape(V.shape[0], 6))

    full_rank = (m >= n) and (s.min() > EPS * m * s.max())
    if full_rank:
        p = back(suf / s2)
        if _norm(p) <= Delta:
            return p, 0.0, 0
    alpha_upper = _norm(suf) / Delta
    if full_rank:
        phi, phi_prime = phi_and_derivative(0.0)
        alpha_lower = -phi / phi_prime
    else:
        alpha_lower = 0.0
    if initial_alpha is None or (not full_rank and initial_alpha == 0):
        alpha = max(0.001 * alpha_upper, (alpha_lower * alpha_upper) ** 0.5)
    else:
        alpha = initial_alpha
    it = 0
    for it in range(max_iter):
        if alpha < alpha_lower or alpha > alpha_upper:
            alpha = max(0.001 * alpha_upper, (alpha_lower * alpha_upper) ** 0.5)
        phi, phi_prime = phi_and_derivative(alpha)
        if phi < 0:
            alpha_upper = alpha
        ratio = phi / phi_prime
        alpha_lower = max(alpha_lower, alpha - ratio)
        alpha -= (phi + Delta) * ratio / Delta
        if np.abs(phi) < rtol * Delta:
            break
    p = back(suf / (s2 + alpha))
    p *= Delta / _norm(p)
    return p, alpha, it + 1


def solvePose(frame_extrinsic_matrices, camera_intrinsic_matrix, points_2D, ftol=1e-4, xtol=1e-8, gtol=1e-8,
              max_nfev=None, verbose=2):
    """adjustPose with the optimiser exposed.  The reference calls least_squares(poseFun, ..., ftol=1e-4) with every
    other setting at its default (bundleAdjuster.py:232-241): TRF, dense 2-point Jacobian, tr_solver='exact' (SVD),
    x_scale=1.  Same iteration here; the camera blocks B_f = J_f^T J_f and g_f come from the HIP sweep with the
    points held fixed, and the 'exact' trust-region solve works on their 6x6 eigen-decompositions."""
    ctx = default_context()
    dev = ctx.device
    ext = np.asarray(frame_extrinsic_matrices, float)
    F = len(ext)
    pattern_size = int(len(points_2D) / F)
    pts3 = np.zeros((pattern_size, 3), np.float32)           # the (4,3) chessboard of side 2, bundleAdjuster.py:220-223
    grid = np.mgrid[0:4, 0:3].T.reshape(-1, 2) * 2
    pts3[:, 0] = grid[:, 0]
    pts3[:, 2] = grid[:, 1]
    fi = np.repeat(np.arange(F), pattern_size)
    pi = np.repeat([np.arange(pattern_size)], F, axis=0).reshape(pattern_size * F)
    with np.errstate(all="ignore"):
        x = frameParameters(ext).reshape(F, 6)
    pb = ops.BADevice(camera_intrinsic_matrix, fi, pi, points_2D, F, pattern_size, dev, ctx, pairs=False)
    pts_d = _dev(pts3.astype(np.float64), dev)
    m, n = 2 * len(fi), 6 * F

    def fun(xc):
        c2, _ = pb.residual(_dev(xc, dev), pts_d)
        return 0.5 * float(c2.item())

    def blocks(xc):
        B, g, _, _ = pb.normal_eq(_dev(xc, dev), pts_d, want_cams=True, want_pts=False)
        return B.cpu().numpy(), g.cpu().numpy()

    cost = fun(x)
    cost0 = cost
    if not np.isfinite(cost):
        raise ValueError("Residuals are not finite in the initial point.")
    nfev, njev = 1, 1
    B, g = blocks(x)
    Delta = _norm(x)          # x_scale = 1  (trf.py:427-430)
    if Delta == 0:
        Delta = 1.0
    if max_nfev is None:
        max_nfev = n * 100
    alpha = 0.0
    termination, iteration, step_norm, actual = None, 0, None, None
    if verbose == 2:
        _print_header()
    while True:
        g_norm = float(np.abs(g).max())
        if g_norm < gtol:
            termination = 1
        if verbose == 2:
            _print_iteration(iteration, nfev, cost, actual, step_norm, g_norm)
        if termination is not None or nfev == max_nfev:
            break
        lam, V = np.linalg.eigh(B)
        vg = np.einsum("fji,fj->fi", V, g)
        actual = -1.0
        while actual <= 0 and nfev < max_nfev:
            step, alpha, _ = _solve_lsq_trust_region_eig(lam, vg, V, Delta, m, alpha)
            predicted = -(0.5 * np.einsum("fi,fij,fj->", step, B, step) + np.sum(g * step))
            x_new = x + step
            cost_new = fun(x_new)
            nfev += 1
            step_h_norm = _norm(step)
            if not np.isfinite(cost_new):
                Delta = 0.25 * step_h_norm
                continue
            actual = cost - cost_new
            Delta_new, ratio = _update_tr_radius(Delta, actual, predicted, step_h_norm, step_h_norm > 0.95 * Delta)
            step_norm = step_h_norm
            termination = _check_termination(actual, cost, step_norm, _norm(x), ratio, ftol, xtol)
            if termination is not None:
                break
            alpha *= Delta / Delta_new
            Delta = Delta_new
        if actual > 0:
            x, cost = x_new, cost_new
            B, g = blocks(x)
            njev += 1
        else:
            step_norm = 0
            actual = 0
        iteration += 1
    if termination is None:
        termination = 0
    res = BAResult(x=x.reshape(-1), cost=cost, optimality=g_norm, nfev=nfev, njev=njev, status=termination,
                   message=_MESSAGES[termination], success=termination > 0)
    if verbose >= 1:
        _finish_verbose(res, cost0, verbose)
    return res


def adjustPose(frame_extrinsic_matrices, camera_intrinsic_matrix, points_2D):
    """Pose-only refinement against the fixed chessboard (bundleAdjuster.py:214-243) -> list of F 3x4 extrinsics."""
    res = solvePose(frame_extrinsic_matrices, camera_intrinsic_matrix, points_2D, ftol=1e-4, verbose=2)
    return reformatPoseResult(res, len(frame_extrinsic_matrices))
