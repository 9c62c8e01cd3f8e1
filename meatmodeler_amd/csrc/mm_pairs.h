// What the stages over the matches of consecutive frame pairs share (verify.hip, pose.hip, homography.hip, guided.hip): how a
// match is read, the two distances, the Hartley normalisation, and the MSAC skeleton around a model.
//
// The rule of mm_geom.h holds here: shared means a definition or a skeleton.  A stage plugs in its model and keeps it in its
// own file: a type built from nine doubles (with whatever it prepares once, such as an adjugate) that has
//     double distance(double x, double y, double xp, double yp) const
// and the stage's solver, verdict and flags.  The distances themselves (vfy_sampson, hg_adjugate / hg_transfer) are here
// since guided.hip gates by them: one definition each.  Everything here is __forceinline__ and compiled under the including file's
// flags; sums run in an order that depends on the pair alone (per-thread strides, mm_block_sum), so a pair's row repeats bit
// for bit whatever else shares the call.
#pragma once
#include "mm_common.h"
#include "mm_geom.h"

constexpr int MM_PAIR_TILE = 256;      // matches per LDS tile of a score kernel

// the arguments every RANSAC stage over match pairs has; a stage derives its own from this
struct MmPairArgs {
    const float *kp_xy;
    const int32_t *pairs, *m;
    int n_pairs, cap, n_hyp, min_matches, min_inliers, refit_iters;
    uint32_t seed, pair_base;
    double tau2;
    double *norm;       // [n_pairs, 8]: cx, cy, s, cx', cy', s', number of malformed matches, -
    double *model_h;    // [n_pairs, n_hyp, 9] (NaN: invalid hypothesis)
    double *cost_h;     // [n_pairs, n_hyp] (+inf: invalid hypothesis)
};

// ---- access ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int mm_pair_count(const int32_t *m, int cap, int p) {
    const int mm = m[p];
    return mm < 0 ? 0 : (mm > cap ? cap : mm);
}

// match j of pair p, widened; false (and NaN coordinates) for a malformed match -- nothing is read through a bad index
__device__ __forceinline__ bool mm_pair_load(const float *kp_xy, const int32_t *pairs, int cap, int p, int j, double &x, double &y,
                                             double &xp, double &yp) {
    const int2 qt = reinterpret_cast<const int2 *>(pairs)[(size_t)p * cap + j];
    const bool wf = (unsigned)qt.x < (unsigned)cap && (unsigned)qt.y < (unsigned)cap;
    const double nan = __builtin_nan("");
    x = y = xp = yp = nan;
    if (wf) {
        const float2 u = reinterpret_cast<const float2 *>(kp_xy)[(size_t)p * cap + qt.x];
        const float2 v = reinterpret_cast<const float2 *>(kp_xy)[(size_t)(p + 1) * cap + qt.y];
        x = (double)u.x;
        y = (double)u.y;
        xp = (double)v.x;
        yp = (double)v.y;
    }
    return wf;
}
template <class Args>
__device__ __forceinline__ bool mm_pair_load(const Args &a, int p, int j, double &x, double &y, double &xp, double &yp) {
    return mm_pair_load(a.kp_xy, a.pairs, a.cap, p, j, x, y, xp, yp);
}

// calibrated rays K^-1 (x, y, 1) of match j of pair p (a.Ki: mm_k_inverse); (0, 0, 1) twice and false for a malformed match
template <class Args>
__device__ __forceinline__ bool mm_pair_rays(const Args &a, int p, int j, Vec3 &ra, Vec3 &rb) {
    double x, y, xp, yp;
    const bool wf = mm_pair_load(a, p, j, x, y, xp, yp);
    ra = rb = Vec3{0.0, 0.0, 1.0};
    if (wf) {
        ra = Vec3{(a.Ki[0] * x + a.Ki[1] * y) + a.Ki[2], a.Ki[3] * y + a.Ki[4], 1.0};
        rb = Vec3{(a.Ki[0] * xp + a.Ki[1] * yp) + a.Ki[2], a.Ki[3] * yp + a.Ki[4], 1.0};
    }
    return wf;
}

__device__ __forceinline__ bool mm_pair_inlier(double d2, double tau2) { return isfinite(d2) && d2 <= tau2; }

// ---- the two distances (verify.hip, homography.hip and guided.hip read these and nothing else) -------------------------------
// Sampson distance of x'^T F x = 0
__device__ __forceinline__ double vfy_sampson(const double (&F)[9], double x, double y, double xp, double yp) {
    const double fx0 = F[0] * x + F[1] * y + F[2], fx1 = F[3] * x + F[4] * y + F[5], fx2 = F[6] * x + F[7] * y + F[8];
    const double ft0 = F[0] * xp + F[3] * yp + F[6], ft1 = F[1] * xp + F[4] * yp + F[7];
    const double e = xp * fx0 + yp * fx1 + fx2;
    return e * e / (fx0 * fx0 + fx1 * fx1 + ft0 * ft0 + ft1 * ft1);
}

// adj(H), written out: every entry one difference of two products, no division by the determinant
__device__ __forceinline__ void hg_adjugate(const double (&H)[9], double (&A)[9]) {
    A[0] = H[4] * H[8] - H[5] * H[7];
    A[1] = H[2] * H[7] - H[1] * H[8];
    A[2] = H[1] * H[5] - H[2] * H[4];
    A[3] = H[5] * H[6] - H[3] * H[8];
    A[4] = H[0] * H[8] - H[2] * H[6];
    A[5] = H[2] * H[3] - H[0] * H[5];
    A[6] = H[3] * H[7] - H[4] * H[6];
    A[7] = H[1] * H[6] - H[0] * H[7];
    A[8] = H[0] * H[4] - H[1] * H[3];
}

// symmetric transfer distance d^2 = (|x' - pi(H x)|^2 + |x - pi(adj(H) x')|^2) / 2
__device__ __forceinline__ double hg_transfer(const double (&H)[9], const double (&A)[9], double x, double y, double xp, double yp) {
    const double y0 = (H[0] * x + H[1] * y) + H[2], y1 = (H[3] * x + H[4] * y) + H[5], y2 = (H[6] * x + H[7] * y) + H[8];
    const double z0 = (A[0] * xp + A[1] * yp) + A[2], z1 = (A[3] * xp + A[4] * yp) + A[5], z2 = (A[6] * xp + A[7] * yp) + A[8];
    const double ex = xp - y0 / y2, ey = yp - y1 / y2, fx = x - z0 / z2, fy = y - z1 / z2;
    return ((ex * ex + ey * ey) + (fx * fx + fy * fy)) * 0.5;
}

// is match j an inlier of the model (a malformed match has NaN coordinates, a NaN distance, and is none)
template <class Model, class Args>
__device__ __forceinline__ bool mm_pair_inlier_of(const Model &M, const Args &a, int p, int j) {
    double x, y, xp, yp;
    mm_pair_load(a, p, j, x, y, xp, yp);
    return mm_pair_inlier(M.distance(x, y, xp, yp), a.tau2);
}

// ---- Hartley normalisation ------------------------------------------------------------------------------------------------
// Over the matches j < mm of pair p for which use(well_formed, x, y, xp, yp) holds: their number n, the centroid of each
// image and the scale sqrt 2 / (mean distance from it).  One workgroup of MM_BLOCK_THREADS; sm holds MM_BLOCK_WAVES * 5
// doubles; every thread ends with the same bits.  The two predicates in use: "well-formed" and "inlier of the current model".
template <class Args, class Use>
__device__ __forceinline__ void mm_pairs_hartley(const Args &a, int p, int mm, Use use, double *sm, double &n, double &cx, double &cy,
                                                 double &s, double &cx2, double &cy2, double &s2) {
    double s5[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int j = threadIdx.x; j < mm; j += MM_BLOCK_THREADS) {
        double x, y, xp, yp;
        const bool wf = mm_pair_load(a, p, j, x, y, xp, yp);
        if (use(wf, x, y, xp, yp)) {
            s5[0] += 1.0;
            s5[1] += x;
            s5[2] += y;
            s5[3] += xp;
            s5[4] += yp;
        }
    }
    mm_block_sum<5>(s5, sm);
    n = s5[0];
    cx = s5[1] / n;
    cy = s5[2] / n;
    cx2 = s5[3] / n;
    cy2 = s5[4] / n;
    double dd[2] = {0.0, 0.0};
    for (int j = threadIdx.x; j < mm; j += MM_BLOCK_THREADS) {
        double x, y, xp, yp;
        const bool wf = mm_pair_load(a, p, j, x, y, xp, yp);
        if (use(wf, x, y, xp, yp)) {
            dd[0] += sqrt((x - cx) * (x - cx) + (y - cy) * (y - cy));
            dd[1] += sqrt((xp - cx2) * (xp - cx2) + (yp - cy2) * (yp - cy2));
        }
    }
    mm_block_sum<2>(dd, sm);
    s = 1.4142135623730951 / (dd[0] / n);
    s2 = 1.4142135623730951 / (dd[1] / n);
}

// body of a stage's normalise kernel: one workgroup per pair, over its well-formed matches, into a.norm
template <class Args>
__device__ __forceinline__ void mm_pairs_normalise(const Args &a) {
    __shared__ double sm[MM_BLOCK_WAVES * 5];
    const int p = blockIdx.x;
    const int mm = mm_pair_count(a.m, a.cap, p);
    double n, cx, cy, s, cx2, cy2, s2;
    mm_pairs_hartley(a, p, mm, [](bool wf, double, double, double, double) { return wf; }, sm, n, cx, cy, s, cx2, cy2, s2);
    if (threadIdx.x == 0) {
        double *o = a.norm + 8 * (size_t)p;
        o[0] = cx;
        o[1] = cy;
        o[2] = s;
        o[3] = cx2;
        o[4] = cy2;
        o[5] = s2;
        o[6] = (double)mm - n;
        o[7] = 0.0;
    }
}

// ---- MSAC -----------------------------------------------------------------------------------------------------------------
// body of a stage's score kernel: lane = hypothesis, its model in registers; the pair's matches go through LDS in tiles and
// every lane reads the same address (broadcast), summing min(d^2, tau^2) over j ascending: no cross-lane step.  Workgroups of
// 64, grid (pair, hypotheses / 64).
template <class Model, class Args>
__device__ __forceinline__ void mm_pairs_score(const Args &a) {
    __shared__ double tile[MM_PAIR_TILE * 4];
    const int p = blockIdx.x;
    const int h = blockIdx.y * 64 + threadIdx.x;
    const int mm = mm_pair_count(a.m, a.cap, p);
    if (mm < a.min_matches) return;      // (uniform over the workgroup)
    const bool live = h < a.n_hyp;
    double v[9];
    const double *src = a.model_h + ((size_t)p * a.n_hyp + (live ? h : 0)) * 9;
#pragma unroll
    for (int c = 0; c < 9; ++c) v[c] = src[c];
    const Model M(v);
    double cost = 0.0;
    for (int j0 = 0; j0 < mm; j0 += MM_PAIR_TILE) {
        const int nt = min(MM_PAIR_TILE, mm - j0);
        __syncthreads();
        for (int j = threadIdx.x; j < nt; j += 64) {
            double x, y, xp, yp;
            mm_pair_load(a, p, j0 + j, x, y, xp, yp);
            tile[4 * j] = x;
            tile[4 * j + 1] = y;
            tile[4 * j + 2] = xp;
            tile[4 * j + 3] = yp;
        }
        __syncthreads();
        for (int j = 0; j < nt; ++j) {
            const double d2 = M.distance(tile[4 * j], tile[4 * j + 1], tile[4 * j + 2], tile[4 * j + 3]);
            cost += mm_pair_inlier(d2, a.tau2) ? d2 : a.tau2;
        }
    }
    if (live) a.cost_h[(size_t)p * a.n_hyp + h] = isfinite(v[0]) ? cost : __builtin_huge_val();
}

// MSAC cost and inlier count of a model over all matches of the pair (one workgroup; every thread returns the same bits)
template <class Model, class Args>
__device__ __forceinline__ void mm_pairs_cost(const Model &M, const Args &a, int p, int mm, double *sm, double &cost, int &n_in) {
    double v[2] = {0.0, 0.0};
    for (int j = threadIdx.x; j < mm; j += MM_BLOCK_THREADS) {
        double x, y, xp, yp;
        mm_pair_load(a, p, j, x, y, xp, yp);
        const double d2 = M.distance(x, y, xp, yp);
        const bool in = mm_pair_inlier(d2, a.tau2);
        v[0] += in ? d2 : a.tau2;
        v[1] += in ? 1.0 : 0.0;
    }
    mm_block_sum<2>(v, sm);
    cost = v[0];
    n_in = (int)v[1];
}

// The winner of a pair and its refit rounds.  v (NaN), cost (NaN), n_in (0), best_h (-1), n_valid (0) come in preset.
// Returns 0 with the model in v, or the reason there is none: MM_PAIRS_TOO_FEW (fewer than min_matches matches) or
// MM_PAIRS_NO_MODEL (no hypothesis with a finite cost).  The winner is the lowest finite cost, ties to the lowest h.  A refit
// round -- while the model has at least min_sample inliers -- normalises over the inliers of the current model and calls
//     bool refit(const Model &current, double cx, cy, s, cx2, cy2, s2, double (&vn)[9])
// the stage's solver over those inliers; its result replaces the model when it is valid and its cost finite and lower.
// sm: as large as the refit's own sums need, at least MM_BLOCK_WAVES * 5 doubles; bc, bh: MM_BLOCK_WAVES entries.
constexpr int MM_PAIRS_TOO_FEW = 1, MM_PAIRS_NO_MODEL = 2;
template <class Model, class Args, class Refit>
__device__ __forceinline__ int mm_pairs_winner_refit(const Args &a, int p, int mm, int min_sample, double *sm, double *bc, int *bh,
                                                     Refit refit, double (&v)[9], double &cost, int &n_in, int &best_h, int &n_valid) {
    if (mm < a.min_matches) return MM_PAIRS_TOO_FEW;
    double c_best;
    int h_best;
    mm_block_argmin_finite(a.cost_h + (size_t)p * a.n_hyp, a.n_hyp, a.model_h + (size_t)p * a.n_hyp * 9, 9, bc, bh, sm, c_best, h_best,
                           n_valid);
    if (h_best == INT32_MAX) return MM_PAIRS_NO_MODEL;
    best_h = h_best;
#pragma unroll
    for (int c = 0; c < 9; ++c) v[c] = a.model_h[((size_t)p * a.n_hyp + h_best) * 9 + c];
    mm_pairs_cost(Model(v), a, p, mm, sm, cost, n_in);
    for (int it = 0; it < a.refit_iters; ++it) {
        if (n_in < min_sample) break;      // (uniform: nothing changes any more)
        const Model M(v);
        double n, cx, cy, s, cx2, cy2, s2;
        mm_pairs_hartley(
            a, p, mm, [&](bool, double x, double y, double xp, double yp) { return mm_pair_inlier(M.distance(x, y, xp, yp), a.tau2); }, sm,
            n, cx, cy, s, cx2, cy2, s2);
        double vn[9];
        const bool ok = refit(M, cx, cy, s, cx2, cy2, s2, vn);
        double cn;
        int nn_in;
        mm_pairs_cost(Model(vn), a, p, mm, sm, cn, nn_in);
        if (ok && isfinite(cn) && cn < cost) {
            cost = cn;
            n_in = nn_in;
#pragma unroll
            for (int c = 0; c < 9; ++c) v[c] = vn[c];
        }
    }
    return 0;
}

// The matches j < mm for which keep(j) holds, in their input order, into row p of pairs_out; returns their number.  One
// workgroup; wcount: MM_BLOCK_WAVES entries.
template <class Args, class Keep>
__device__ __forceinline__ int mm_pairs_compact(const Args &a, int p, int mm, Keep keep_of, int32_t *pairs_out, int *wcount) {
    int kept = 0;
    for (int j0 = 0; j0 < mm; j0 += MM_BLOCK_THREADS) {
        const int j = j0 + threadIdx.x;
        bool keep = false;
        int2 qt = make_int2(0, 0);
        if (j < mm) {
            qt = reinterpret_cast<const int2 *>(a.pairs)[(size_t)p * a.cap + j];
            keep = keep_of(j);
        }
        const int at = mm_block_compact_slot(keep, kept, wcount);
        if (keep) reinterpret_cast<int2 *>(pairs_out)[(size_t)p * a.cap + at] = qt;
    }
    return kept;
}

// ---- host: the [norm | models | costs] workspace --------------------------------------------------------------------------
inline size_t mm_pairs_workspace(int n_pairs, int n_hyp) {
    const size_t np = n_pairs > 0 ? (size_t)n_pairs : 0, nh = n_hyp > 0 ? (size_t)n_hyp : 0;
    return mm_align_up(np * 8 * sizeof(double), 256) + mm_align_up(np * nh * 9 * sizeof(double), 256) +
           mm_align_up(np * nh * sizeof(double), 256);
}
// points a.norm, a.model_h and a.cost_h into ws (a.n_pairs and a.n_hyp set)
inline void mm_pairs_carve(MmPairArgs &a, void *ws) {
    char *w = (char *)ws;
    a.norm = (double *)w;
    w += mm_align_up((size_t)a.n_pairs * 8 * sizeof(double), 256);
    a.model_h = (double *)w;
    w += mm_align_up((size_t)a.n_pairs * a.n_hyp * 9 * sizeof(double), 256);
    a.cost_h = (double *)w;
}
