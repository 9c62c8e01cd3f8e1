// Two-view homogeneous DLT triangulation, one thread per track (gfx950, f64).
//
// Replaces the per-track loop of processor.triangulatePoints (reference processor.py:254-261):
//   cv2.triangulatePoints(P_first, P_last, x_first, x_last) -> X[:3] / X[3].
// OpenCV builds the 4x4 system  x*P[2]-P[0], y*P[2]-P[1]  for both views and takes the right singular vector of
// the smallest singular value (calib3d triangulate.cpp, one-sided Jacobi SVD).  The same one-sided (Hestenes)
// Jacobi runs here entirely in registers: 16 + 16 doubles per thread, fully unrolled so every index is static.
// The work is tiny (64 B in, 24 B out, ~2 kflop per track): the kernel is latency-bound by construction.
#include "mm_common.h"
#include "mm_geom.h"

namespace {

__global__ __launch_bounds__(256) void dlt_kernel(const double *__restrict__ proj, const int32_t *__restrict__ f0,
                                                  const int32_t *__restrict__ f1, const double *__restrict__ x0,
                                                  const double *__restrict__ x1, int64_t n, double *__restrict__ X) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double *P0 = proj + (size_t)f0[i] * 12;
    const double *P1 = proj + (size_t)f1[i] * 12;
    const double ax = x0[2 * i], ay = x0[2 * i + 1], bx = x1[2 * i], by = x1[2 * i + 1];
    double A[4][4], V[4][4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        A[0][c] = ax * P0[8 + c] - P0[c];
        A[1][c] = ay * P0[8 + c] - P0[4 + c];
        A[2][c] = bx * P1[8 + c] - P1[c];
        A[3][c] = by * P1[8 + c] - P1[4 + c];
#pragma unroll
        for (int r = 0; r < 4; ++r) V[r][c] = (r == c) ? 1.0 : 0.0;
    }
    for (int sweep = 0; sweep < 30; ++sweep) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                double a = 0, b = 0, g = 0;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    a += A[r][p] * A[r][p];
                    b += A[r][q] * A[r][q];
                    g += A[r][p] * A[r][q];
                }
                if (fabs(g) > MM_F64_EPS * sqrt(a * b) && g != 0.0) {
                    rotated = true;
                    double zeta = (b - a) / (2.0 * g);
                    double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                    double c = 1.0 / sqrt(1.0 + t * t);
                    double s = c * t;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        double ap = A[r][p], aq = A[r][q];
                        A[r][p] = c * ap - s * aq;
                        A[r][q] = s * ap + c * aq;
                        double vp = V[r][p], vq = V[r][q];
                        V[r][p] = c * vp - s * vq;
                        V[r][q] = s * vp + c * vq;
                    }
                }
            }
        }
        if (!rotated) break;
    }
    // column with the smallest norm = smallest singular value
    double best = 1e300;
    double v0 = 0, v1 = 0, v2 = 0, v3 = 1;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        double nn = A[0][c] * A[0][c] + A[1][c] * A[1][c] + A[2][c] * A[2][c] + A[3][c] * A[3][c];
        if (nn < best) {
            best = nn;
            v0 = V[0][c];
            v1 = V[1][c];
            v2 = V[2][c];
            v3 = V[3][c];
        }
    }
    X[3 * i] = v0 / v3;
    X[3 * i + 1] = v1 / v3;
    X[3 * i + 2] = v2 / v3;
}

// ---- multi-view triangulation of whole tracks with per-track quality (mm_triangulate_tracks) ---------------------------------
// Four lanes per track (the point-block pattern of ba.hip): lane `sub` of a track's quad walks the observations
// begin + sub, begin + sub + 4, ... and the four partial sums meet in a fixed two-step butterfly.  Floating-point addition
// commutes, so all four lanes end up with the SAME bits and carry on redundantly -- no broadcast, and a track's result
// depends on the track alone (not on its position in the call: every track starts at sub = 0 of its own quad).
// No lane leaves early and no shuffle sits under a divergent branch: accept / reject of a trial step are selects.
constexpr int TRI_LANES = 4;
constexpr int TRI_THREADS = 256;

__device__ __forceinline__ double tri_quad_sum(double v) {
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    return v;
}
// max / min that keep a NaN (fmax / fmin would drop it): a residual or depth that is not a number makes its column NaN,
// as NumPy's max / min do
__device__ __forceinline__ double tri_nanmax(double a, double b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ double tri_nanmin(double a, double b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ double tri_quad_max(double v) {
    v = tri_nanmax(v, __shfl_xor(v, 1, 64));
    return tri_nanmax(v, __shfl_xor(v, 2, 64));
}
__device__ __forceinline__ double tri_quad_min(double v) {
    v = tri_nanmin(v, __shfl_xor(v, 1, 64));
    return tri_nanmin(v, __shfl_xor(v, 2, 64));
}

// per frame: camera centre C = -P[:, :3]^-1 P[:, 3] (adjugate / determinant) and |P[2, :3]| -> fr[f] = (Cx, Cy, Cz, norm)
__global__ __launch_bounds__(256) void tri_frame_kernel(const double *__restrict__ proj, int F, double *__restrict__ fr) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const double *P = proj + (size_t)f * 12;
    const double a = P[0], b = P[1], c = P[2], d = P[4], e = P[5], g = P[6], h = P[8], i = P[9], j = P[10];
    const double p0 = P[3], p1 = P[7], p2 = P[11];
    const double c00 = e * j - g * i, c01 = c * i - b * j, c02 = b * g - c * e;
    const double c10 = g * h - d * j, c11 = a * j - c * h, c12 = c * d - a * g;
    const double c20 = d * i - e * h, c21 = b * h - a * i, c22 = a * e - b * d;
    const double det = a * c00 + b * c10 + c * c20;
    fr[4 * (size_t)f] = -(c00 * p0 + c01 * p1 + c02 * p2) / det;
    fr[4 * (size_t)f + 1] = -(c10 * p0 + c11 * p1 + c12 * p2) / det;
    fr[4 * (size_t)f + 2] = -(c20 * p0 + c21 * p1 + c22 * p2) / det;
    fr[4 * (size_t)f + 3] = sqrt(h * h + i * i + j * j);
}

// this lane's share of cost = sum |pi(P X) - x|^2 and of H = sum J^T J (upper triangle, row-major), g = sum J^T r at X
__device__ __forceinline__ void tri_normal_pass(const double *__restrict__ proj, const int32_t *__restrict__ obs_frame,
                                                const double *__restrict__ obs_xy, int o_first, int o_end, double X0, double X1,
                                                double X2, double &cost, double (&H)[6], double (&g)[3]) {
    cost = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) H[k] = 0.0;
    g[0] = g[1] = g[2] = 0.0;
    for (int o = o_first; o < o_end; o += TRI_LANES) {
        const double *P = proj + (size_t)obs_frame[o] * 12;
        const double2 xy = reinterpret_cast<const double2 *>(obs_xy)[o];
        const double w = P[8] * X0 + P[9] * X1 + P[10] * X2 + P[11];
        const double iw = 1.0 / w;
        const double u = (P[0] * X0 + P[1] * X1 + P[2] * X2 + P[3]) * iw;
        const double v = (P[4] * X0 + P[5] * X1 + P[6] * X2 + P[7]) * iw;
        const double ru = u - xy.x, rv = v - xy.y;
        const double ju0 = (P[0] - u * P[8]) * iw, ju1 = (P[1] - u * P[9]) * iw, ju2 = (P[2] - u * P[10]) * iw;
        const double jv0 = (P[4] - v * P[8]) * iw, jv1 = (P[5] - v * P[9]) * iw, jv2 = (P[6] - v * P[10]) * iw;
        cost += ru * ru + rv * rv;
        H[0] += ju0 * ju0 + jv0 * jv0;
        H[1] += ju0 * ju1 + jv0 * jv1;
        H[2] += ju0 * ju2 + jv0 * jv2;
        H[3] += ju1 * ju1 + jv1 * jv1;
        H[4] += ju1 * ju2 + jv1 * jv2;
        H[5] += ju2 * ju2 + jv2 * jv2;
        g[0] += ju0 * ru + jv0 * rv;
        g[1] += ju1 * ru + jv1 * rv;
        g[2] += ju2 * ru + jv2 * rv;
    }
    cost = tri_quad_sum(cost);
#pragma unroll
    for (int k = 0; k < 6; ++k) H[k] = tri_quad_sum(H[k]);
#pragma unroll
    for (int k = 0; k < 3; ++k) g[k] = tri_quad_sum(g[k]);
}

__global__ __launch_bounds__(TRI_THREADS) void tri_tracks_kernel(const double *__restrict__ proj, const int32_t *__restrict__ track_ptr,
                                                                 const int32_t *__restrict__ obs_frame, const double *__restrict__ obs_xy,
                                                                 const double *__restrict__ fr, int64_t T, mm_tri_params prm,
                                                                 double *__restrict__ Xout, double *__restrict__ quality,
                                                                 int32_t *__restrict__ flags) {
    const int sub = threadIdx.x & (TRI_LANES - 1);
    const int64_t t = (int64_t)blockIdx.x * (TRI_THREADS / TRI_LANES) + threadIdx.x / TRI_LANES;
    const bool live = t < T;      // (no early return: whole waves execute the shuffles)
    int o_begin = 0, o_end = 0;
    if (live) {
        o_begin = track_ptr[t];
        o_end = track_ptr[t + 1];
    }
    const int m = o_end - o_begin;

    // ---- linear stage: M = A^T A (4 x 4 symmetric), rows x P[2] - P[0] and y P[2] - P[1] of every observation
    double A[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) A[r][c] = 0.0;
    for (int o = o_begin + sub; o < o_end; o += TRI_LANES) {
        const double *P = proj + (size_t)obs_frame[o] * 12;
        const double2 xy = reinterpret_cast<const double2 *>(obs_xy)[o];
        double a[4], b[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            a[c] = xy.x * P[8 + c] - P[c];
            b[c] = xy.y * P[8 + c] - P[4 + c];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = r; c < 4; ++c) A[r][c] += a[r] * a[c] + b[r] * b[c];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = r; c < 4; ++c) {
            A[r][c] = tri_quad_sum(A[r][c]);
            A[c][r] = A[r][c];
        }
    // mm_jacobi<4> of mm_geom.h, written out.  This file is built with FMA contraction; with the shared function called here
    // the kernel compiles to the same instruction mix in another arrangement and X differs (measured on the MI355X: up to
    // 3e-11 relative at refine_iters = 0, wherever V is initialised).  The loop stays so that the kernel keeps its bits: a
    // change to mm_jacobi is made here as well.
    double V[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) V[r][c] = (r == c) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 30; ++sweep) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                const double apq = A[p][q];
                if (fabs(apq) > MM_F64_EPS * sqrt(fabs(A[p][p] * A[q][q])) && apq != 0.0) {
                    rotated = true;
                    const double zeta = (A[q][q] - A[p][p]) / (2.0 * apq);
                    const double tn = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                    const double cs = 1.0 / sqrt(1.0 + tn * tn);
                    const double sn = cs * tn;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {      // columns p, q of A and of V
                        const double akp = A[k][p], akq = A[k][q];
                        A[k][p] = cs * akp - sn * akq;
                        A[k][q] = sn * akp + cs * akq;
                        const double vkp = V[k][p], vkq = V[k][q];
                        V[k][p] = cs * vkp - sn * vkq;
                        V[k][q] = sn * vkp + cs * vkq;
                    }
#pragma unroll
                    for (int k = 0; k < 4; ++k) {      // rows p, q of A
                        const double apk = A[p][k], aqk = A[q][k];
                        A[p][k] = cs * apk - sn * aqk;
                        A[q][k] = sn * apk + cs * aqk;
                    }
                    A[p][q] = A[q][p] = 0.0;
                }
            }
        }
        if (!rotated) break;
    }
    double best = A[0][0], v0 = V[0][0], v1 = V[1][0], v2 = V[2][0], v3 = V[3][0];
#pragma unroll
    for (int c = 1; c < 4; ++c) {
        if (A[c][c] < best) {
            best = A[c][c];
            v0 = V[0][c];
            v1 = V[1][c];
            v2 = V[2][c];
            v3 = V[3][c];
        }
    }
    double X0 = v0 / v3, X1 = v1 / v3, X2 = v2 / v3;
    const bool degenerate = m < 2 || !(isfinite(X0) && isfinite(X1) && isfinite(X2));
    // a degenerate track walks no observation from here on: its trial steps are all rejected, X stays the linear one
    const int o_first = degenerate ? o_end : o_begin + sub;

    // ---- refinement: a fixed number of Levenberg-Marquardt trial steps on the inhomogeneous point
    if (prm.refine_iters > 0) {
        double cost, H[6], g[3], lam = 1e-3;
        tri_normal_pass(proj, obs_frame, obs_xy, o_first, o_end, X0, X1, X2, cost, H, g);
        for (int it = 0; it < prm.refine_iters; ++it) {
            // (H + lam diag H) delta = -g by a 3 x 3 Cholesky; a pivot that is not positive fails the trial
            const double a00 = H[0] + lam * H[0], a11 = H[3] + lam * H[3], a22 = H[5] + lam * H[5];
            bool ok = a00 > 0.0;
            const double l00 = sqrt(a00);
            const double l10 = H[1] / l00, l20 = H[2] / l00;
            const double d1 = a11 - l10 * l10;
            ok = ok && d1 > 0.0;
            const double l11 = sqrt(d1);
            const double l21 = (H[4] - l20 * l10) / l11;
            const double d2 = a22 - l20 * l20 - l21 * l21;
            ok = ok && d2 > 0.0;
            const double l22 = sqrt(d2);
            const double y0 = -g[0] / l00;
            const double y1 = (-g[1] - l10 * y0) / l11;
            const double y2 = (-g[2] - l20 * y0 - l21 * y1) / l22;
            const double e2 = y2 / l22;
            const double e1 = (y1 - l21 * e2) / l11;
            const double e0 = (y0 - l10 * e1 - l20 * e2) / l00;
            const double N0 = X0 + e0, N1 = X1 + e1, N2 = X2 + e2;
            double cn, Hn[6], gn[3];
            tri_normal_pass(proj, obs_frame, obs_xy, o_first, o_end, N0, N1, N2, cn, Hn, gn);
            const bool accept = ok && isfinite(cn) && cn < cost;      // (anything else, a non-finite cost included, is a reject)
            X0 = accept ? N0 : X0;
            X1 = accept ? N1 : X1;
            X2 = accept ? N2 : X2;
            cost = accept ? cn : cost;
#pragma unroll
            for (int k = 0; k < 6; ++k) H[k] = accept ? Hn[k] : H[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) g[k] = accept ? gn[k] : g[k];
            lam = accept ? fmax(lam / 10.0, 1e-12) : lam * 10.0;
        }
    }

    // ---- quality at the returned X
    const double inf = __builtin_huge_val();
    double ss = 0.0, mx = 0.0, dmin = inf, cmin = inf;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    if (!degenerate) {      // the first observation's camera centre, minus X
        const double *Cf = fr + 4 * (size_t)obs_frame[o_begin];
        a0 = Cf[0] - X0;
        a1 = Cf[1] - X1;
        a2 = Cf[2] - X2;
    }
    const double aa = a0 * a0 + a1 * a1 + a2 * a2;
    for (int o = o_first; o < o_end; o += TRI_LANES) {
        const int f = obs_frame[o];
        const double *P = proj + (size_t)f * 12;
        const double2 xy = reinterpret_cast<const double2 *>(obs_xy)[o];
        const double w = P[8] * X0 + P[9] * X1 + P[10] * X2 + P[11];
        const double ru = (P[0] * X0 + P[1] * X1 + P[2] * X2 + P[3]) / w - xy.x;
        const double rv = (P[4] * X0 + P[5] * X1 + P[6] * X2 + P[7]) / w - xy.y;
        const double r2 = ru * ru + rv * rv;
        ss += r2;
        mx = tri_nanmax(mx, r2);
        const double *Cf = fr + 4 * (size_t)f;
        dmin = tri_nanmin(dmin, w / Cf[3]);
        if (o != o_begin) {
            const double b0 = Cf[0] - X0, b1 = Cf[1] - X1, b2 = Cf[2] - X2;
            cmin = tri_nanmin(cmin, (a0 * b0 + a1 * b1 + a2 * b2) / sqrt(aa * (b0 * b0 + b1 * b1 + b2 * b2)));
        }
    }
    ss = tri_quad_sum(ss);
    mx = tri_quad_max(mx);
    dmin = tri_quad_min(dmin);
    cmin = tri_quad_min(cmin);
    if (live && sub == 0) {
        const double nan = __builtin_nan("");
        const double q0 = degenerate ? nan : sqrt(ss / (double)m), q1 = degenerate ? nan : sqrt(mx);
        const double q2 = degenerate ? nan : dmin, q3 = degenerate ? nan : cmin;
        int fl = degenerate ? MM_TRI_DEGENERATE : 0;
        if (q2 <= prm.min_depth) fl |= MM_TRI_BEHIND;
        if (q1 > prm.max_reproj_px) fl |= MM_TRI_REPROJ;
        if (q3 > prm.max_cos_parallax) fl |= MM_TRI_PARALLAX;
        Xout[3 * t] = X0;
        Xout[3 * t + 1] = X1;
        Xout[3 * t + 2] = X2;
        quality[4 * t] = q0;
        quality[4 * t + 1] = q1;
        quality[4 * t + 2] = q2;
        quality[4 * t + 3] = q3;
        flags[t] = fl;
    }
}

}  // namespace

extern "C" int mm_triangulate_dlt(mm_ctx *ctx, const double *proj, const int32_t *f0, const int32_t *f1,
                                  const double *x0, const double *x1, int64_t n, double *X) {
    if (!ctx) return MM_ERR_ARG;
    if (n == 0) return MM_OK;
    if (!proj || !f0 || !f1 || !x0 || !x1 || !X || n < 0) return mm_fail(ctx, MM_ERR_ARG, "mm_triangulate_dlt: bad argument");
    int64_t blocks = (n + 255) / 256;
    MM_LAUNCH(ctx, "dlt_kernel", dlt_kernel, dim3((unsigned)blocks), dim3(256), 0, proj, f0, f1, x0, x1, n, X);
    return MM_OK;
}

extern "C" size_t mm_triangulate_tracks_workspace_bytes(int F) { return mm_align_up((size_t)(F > 0 ? F : 0) * 4 * sizeof(double), 256); }

extern "C" int mm_triangulate_tracks(mm_ctx *ctx, const double *proj, int F, const int32_t *track_ptr, int64_t T,
                                     const int32_t *obs_frame, const double *obs_xy, const mm_tri_params *prm, double *X,
                                     double *quality, int32_t *flags, void *ws, size_t ws_bytes) {
    if (!ctx) return MM_ERR_ARG;
    if (T == 0) return MM_OK;
    if (!proj || !track_ptr || !obs_frame || !obs_xy || !prm || !X || !quality || !flags || !ws || T < 0 || F <= 0 ||
        T > INT32_MAX || prm->refine_iters < 0 || prm->refine_iters > 1000)
        return mm_fail(ctx, MM_ERR_ARG, "mm_triangulate_tracks: bad argument");
    if ((uintptr_t)obs_xy & 15) return mm_fail(ctx, MM_ERR_ARG, "mm_triangulate_tracks: obs_xy must be 16-byte aligned");
    if (ws_bytes < mm_triangulate_tracks_workspace_bytes(F)) return mm_fail(ctx, MM_ERR_WORKSPACE, "mm_triangulate_tracks: workspace too small");
    double *fr = (double *)ws;
    MM_LAUNCH(ctx, "tri_frame_kernel", tri_frame_kernel, dim3((unsigned)((F + 255) / 256)), dim3(256), 0, proj, F, fr);
    const int per_wg = TRI_THREADS / TRI_LANES;
    MM_LAUNCH(ctx, "tri_tracks_kernel", tri_tracks_kernel, dim3((unsigned)((T + per_wg - 1) / per_wg)), dim3(TRI_THREADS), 0, proj,
              track_ptr, obs_frame, obs_xy, fr, T, *prm, X, quality, flags);
    return MM_OK;
}
