// Epipolar verification of the matches of consecutive frame pairs: a RANSAC fundamental matrix per pair (gfx950, f64).
//
// No reference counterpart: the reference hands every Lowe-ratio survivor to pointTracking.  The definition -- sampling,
// 8-point hypotheses, MSAC score, refit, flags -- is in include/meatmodeler.h (mm_verify_matches); this file maps it:
//   vfy_normalise_kernel   one workgroup per pair: Hartley centroid / scale of both images over the well-formed matches
//   vfy_hypothesis_kernel  one lane per (pair, hypothesis): eight sampled rows orthonormalised in registers (every index
//                          static, nothing in scratch), null vector, rank 2, denormalise
//   vfy_score_kernel       lane = hypothesis, F in nine registers; the pair's matches go through LDS in tiles and every lane
//                          reads the same address (broadcast), summing min(d^2, tau^2) over j ascending: no cross-lane step
//   vfy_refit_kernel       one workgroup per pair: argmin, refit rounds (45 sums of A^T A, 9 x 9 Jacobi in LDS), inlier mask,
//                          order-preserving compaction, outputs
// How a match is read, the normalisation and the MSAC skeleton (score body, cost, winner / refit frame, compaction) are
// mm_pairs.h's; here is the model: vfy_sampson, the eight-point hypothesis, vfy_rank2 / vfy_finish and the refit's 45 sums.
// This file is built with FMA contraction (Makefile), where the arrangement of the code can change which products fuse: a
// shared piece is used here only while every output stays byte-equal to the written-out form on the MI355X.
// Plain f64 VALU work; sums in an order that depends on the pair alone (per-thread strides, xor butterflies, waves in order),
// no atomics: a pair's row repeats bit for bit whatever else shares the call.
#include "mm_pairs.h"

namespace {

constexpr int VFY_THREADS = 256;      // normalise / refit: one workgroup per pair
constexpr int VFY_WAVES = VFY_THREADS / 64;
static_assert(VFY_THREADS == MM_BLOCK_THREADS, "the mm_block_* helpers are written for this workgroup");

struct VfyArgs : MmPairArgs {      // (model_h: the hypotheses' F)
    int on_fail;
};

// the model of the MSAC skeleton (mm_pairs.h): F, nothing prepared; the distance is mm_pairs.h's vfy_sampson
struct VfyModel {
    double F[9];
    __device__ __forceinline__ explicit VfyModel(const double (&f)[9]) {
#pragma unroll
        for (int c = 0; c < 9; ++c) F[c] = f[c];
    }
    __device__ __forceinline__ double distance(double x, double y, double xp, double yp) const { return vfy_sampson(F, x, y, xp, yp); }
};

// F^ <- F^ - (F^ v3) v3^T, v3 the eigenvector of the smallest eigenvalue of F^^T F^ (3 x 3 cyclic Jacobi in registers)
__device__ __forceinline__ void vfy_rank2(double (&F)[9]) {
    double G[3][3], V[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            G[r][c] = F[r] * F[c] + F[3 + r] * F[3 + c] + F[6 + r] * F[6 + c];
            V[r][c] = (r == c) ? 1.0 : 0.0;      // (here, not by mm_identity: see mm_jacobi)
        }
    mm_jacobi<3>(G, V);
    double best = G[0][0], v0 = V[0][0], v1 = V[1][0], v2 = V[2][0];      // smallest eigenvalue, ties to the lowest column
#pragma unroll
    for (int c = 1; c < 3; ++c) {
        if (G[c][c] < best) {
            best = G[c][c];
            v0 = V[0][c];
            v1 = V[1][c];
            v2 = V[2][c];
        }
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double fv = F[3 * r] * v0 + F[3 * r + 1] * v1 + F[3 * r + 2] * v2;
        F[3 * r] -= fv * v0;
        F[3 * r + 1] -= fv * v1;
        F[3 * r + 2] -= fv * v2;
    }
}

// rank 2, F = T'^T F^ T with T = [[s, 0, -s cx], [0, s, -s cy], [0, 0, 1]], unit Frobenius norm; false: not finite
__device__ __forceinline__ bool vfy_finish(double (&F)[9], double cx, double cy, double s, double cx2, double cy2, double s2) {
    vfy_rank2(F);
    double G[9];
#pragma unroll
    for (int r = 0; r < 3; ++r) {      // G = F^ T
        G[3 * r] = s * F[3 * r];
        G[3 * r + 1] = s * F[3 * r + 1];
        G[3 * r + 2] = F[3 * r + 2] - s * cx * F[3 * r] - s * cy * F[3 * r + 1];
    }
    double nn = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {      // F = T'^T G
        F[c] = s2 * G[c];
        F[3 + c] = s2 * G[3 + c];
        F[6 + c] = G[6 + c] - s2 * cx2 * G[c] - s2 * cy2 * G[3 + c];
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) nn += F[k] * F[k];
    const double inv = 1.0 / sqrt(nn);
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        F[k] *= inv;
        ok = ok && isfinite(F[k]);
    }
    return ok;
}

// ---- normalisation over all well-formed matches of the pair -----------------------------------------------------------------
__global__ __launch_bounds__(VFY_THREADS) void vfy_normalise_kernel(VfyArgs a) { mm_pairs_normalise(a); }

// ---- one hypothesis per lane --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void vfy_hypothesis_kernel(VfyArgs a) {
    const int p = blockIdx.x;
    const int h = blockIdx.y * 64 + threadIdx.x;
    const int mm = mm_pair_count(a.m, a.cap, p);
    if (h >= a.n_hyp || mm < a.min_matches) return;      // (a pair with too few matches is never scored either)
    const double *nr = a.norm + 8 * (size_t)p;
    const double cx = nr[0], cy = nr[1], s = nr[2], cx2 = nr[3], cy2 = nr[4], s2 = nr[5];
    bool ok = isfinite(s) && isfinite(s2);
    // eight distinct match indices, integer arithmetic only
    const uint32_t base = mm_pcg(mm_pcg(a.seed + mm_pcg(a.pair_base + (uint32_t)p)) + (uint32_t)h);
    int pick[8];
    ok = mm_sample_distinct<8>(base, mm, pick) && ok;
    double A[8][9];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        double x, y, xp, yp;
        ok = mm_pair_load(a, p, pick[k], x, y, xp, yp) && ok;
        x = s * (x - cx);
        y = s * (y - cy);
        xp = s2 * (xp - cx2);
        yp = s2 * (yp - cy2);
        A[k][0] = xp * x;
        A[k][1] = xp * y;
        A[k][2] = xp;
        A[k][3] = yp * x;
        A[k][4] = yp * y;
        A[k][5] = yp;
        A[k][6] = x;
        A[k][7] = y;
        A[k][8] = 1.0;
    }
    // the rows orthonormalised in place (modified Gram-Schmidt, each row twice against its predecessors); the null vector
    // is then the normalised column of I - Q^T Q with the largest diagonal entry, cleaned once more against the rows
#pragma unroll
    for (int i = 0; i < 8; ++i) {
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
            for (int k = 0; k < i; ++k) {
                double d = 0.0;
#pragma unroll
                for (int c = 0; c < 9; ++c) d += A[i][c] * A[k][c];
#pragma unroll
                for (int c = 0; c < 9; ++c) A[i][c] -= d * A[k][c];
            }
        }
        double nn = 0.0;
#pragma unroll
        for (int c = 0; c < 9; ++c) nn += A[i][c] * A[i][c];
        const double inv = 1.0 / sqrt(nn);
#pragma unroll
        for (int c = 0; c < 9; ++c) A[i][c] *= inv;
    }
    double col[8];      // column kbest of Q (selected without a runtime index)
    {
        double best = -1.0;
        int kbest = 0;
#pragma unroll
        for (int c = 0; c < 9; ++c) {
            double dg = 1.0;
#pragma unroll
            for (int i = 0; i < 8; ++i) dg -= A[i][c] * A[i][c];
            if (dg > best) {
                best = dg;
                kbest = c;
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            double v = A[i][0];
#pragma unroll
            for (int c = 1; c < 9; ++c) v = (kbest == c) ? A[i][c] : v;
            col[i] = v;
        }
        double F[9];
#pragma unroll
        for (int c = 0; c < 9; ++c) {
            double v = (kbest == c) ? 1.0 : 0.0;
#pragma unroll
            for (int i = 0; i < 8; ++i) v -= A[i][c] * col[i];
            F[c] = v;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            double d = 0.0;
#pragma unroll
            for (int c = 0; c < 9; ++c) d += F[c] * A[i][c];
#pragma unroll
            for (int c = 0; c < 9; ++c) F[c] -= d * A[i][c];
        }
        double nn = 0.0;
#pragma unroll
        for (int c = 0; c < 9; ++c) nn += F[c] * F[c];
        const double inv = 1.0 / sqrt(nn);
#pragma unroll
        for (int c = 0; c < 9; ++c) F[c] *= inv;
        ok = vfy_finish(F, cx, cy, s, cx2, cy2, s2) && ok;
        double *o = a.model_h + ((size_t)p * a.n_hyp + h) * 9;
        const double nan = __builtin_nan("");
#pragma unroll
        for (int c = 0; c < 9; ++c) o[c] = ok ? F[c] : nan;
    }
}

// ---- MSAC cost of every hypothesis --------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void vfy_score_kernel(VfyArgs a) { mm_pairs_score<VfyModel>(a); }

// ---- winner, refit, compaction --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VFY_THREADS) void vfy_refit_kernel(VfyArgs a, int32_t *__restrict__ pairs_out, int32_t *__restrict__ m_out,
                                                                double *__restrict__ Fm, double *__restrict__ cost_out,
                                                                int32_t *__restrict__ info) {
    __shared__ double sm[VFY_WAVES * 45];
    __shared__ double M[9][9], V[9][9];
    __shared__ double bc[VFY_WAVES];
    __shared__ int bh[VFY_WAVES], wcount[VFY_WAVES];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int mm = mm_pair_count(a.m, a.cap, p);
    const double nan = __builtin_nan("");
    int flags = a.norm[8 * (size_t)p + 6] > 0.0 ? MM_VERIFY_MALFORMED : 0;
    double F[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) F[c] = nan;
    double cost = nan;
    int n_in = 0, best_h = -1, n_valid = 0;
    // a refit round: the null vector of A^T A over the inliers of the current F, rank 2, denormalised
    const auto refit = [&](const VfyModel &cur, double cx, double cy, double s, double cx2, double cy2, double s2, double (&Fn)[9]) {
        // M = A^T A over the inliers: 45 sums (upper triangle, row-major)
        double acc[45];
#pragma unroll
        for (int k = 0; k < 45; ++k) acc[k] = 0.0;
        for (int j = tid; j < mm; j += VFY_THREADS) {
            double x, y, xp, yp;
            mm_pair_load(a, p, j, x, y, xp, yp);
            if (mm_pair_inlier(cur.distance(x, y, xp, yp), a.tau2)) {
                x = s * (x - cx);
                y = s * (y - cy);
                xp = s2 * (xp - cx2);
                yp = s2 * (yp - cy2);
                const double r[9] = {xp * x, xp * y, xp, yp * x, yp * y, yp, x, y, 1.0};
                int k = 0;
#pragma unroll
                for (int i = 0; i < 9; ++i)
#pragma unroll
                    for (int c = i; c < 9; ++c) acc[k++] += r[i] * r[c];
            }
        }
        mm_block_sum<45>(acc, sm);
        __syncthreads();
        if (tid == 0) {
            int k = 0;
#pragma unroll
            for (int i = 0; i < 9; ++i)
#pragma unroll
                for (int c = i; c < 9; ++c) {
                    M[i][c] = acc[k];
                    M[c][i] = acc[k];
                    ++k;
                }
        }
        if (tid < 81) V[tid / 9][tid % 9] = (tid / 9 == tid % 9) ? 1.0 : 0.0;
        __syncthreads();
        // cyclic Jacobi on M with V in LDS: every thread takes the same decisions from the same LDS words, lane k < 9
        // rotates row / column k.  A rotation is skipped once |m_pq| <= eps sqrt(m_pp m_qq).
        for (int sweep = 0; sweep < 30; ++sweep) {
            bool rotated = false;
            for (int pp = 0; pp < 8; ++pp) {
                for (int q = pp + 1; q < 9; ++q) {
                    const double apq = M[pp][q], app = M[pp][pp], aqq = M[q][q];
                    if (fabs(apq) > MM_F64_EPS * sqrt(fabs(app * aqq)) && apq != 0.0) {      // (uniform)
                        rotated = true;
                        const double zeta = (aqq - app) / (2.0 * apq);
                        const double tn = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                        const double cs = 1.0 / sqrt(1.0 + tn * tn);
                        const double sn = cs * tn;
                        __syncthreads();
                        if (tid < 9) {
                            const double akp = M[tid][pp], akq = M[tid][q];
                            M[tid][pp] = cs * akp - sn * akq;
                            M[tid][q] = sn * akp + cs * akq;
                            const double vkp = V[tid][pp], vkq = V[tid][q];
                            V[tid][pp] = cs * vkp - sn * vkq;
                            V[tid][q] = sn * vkp + cs * vkq;
                        }
                        __syncthreads();
                        if (tid < 9) {
                            const double apk = M[pp][tid], aqk = M[q][tid];
                            M[pp][tid] = cs * apk - sn * aqk;
                            M[q][tid] = sn * apk + cs * aqk;
                        }
                        __syncthreads();
                        if (tid == 0) M[pp][q] = M[q][pp] = 0.0;
                        __syncthreads();
                    }
                }
            }
            if (!rotated) break;
        }
        int cbest = 0;
        double ev = M[0][0];
        for (int c = 1; c < 9; ++c) {
            if (M[c][c] < ev) {
                ev = M[c][c];
                cbest = c;
            }
        }
#pragma unroll
        for (int c = 0; c < 9; ++c) Fn[c] = V[c][cbest];
        __syncthreads();      // (M and V are rewritten by the next round)
        return vfy_finish(Fn, cx, cy, s, cx2, cy2, s2);
    };
    const int none = mm_pairs_winner_refit<VfyModel>(a, p, mm, 8, sm, bc, bh, refit, F, cost, n_in, best_h, n_valid);
    if (none == MM_PAIRS_TOO_FEW) flags |= MM_VERIFY_TOO_FEW;
    if (none == MM_PAIRS_NO_MODEL) flags |= MM_VERIFY_NO_MODEL;
    if (none == 0 && n_in < a.min_inliers) flags |= MM_VERIFY_WEAK;

    const bool failed = (flags & (MM_VERIFY_TOO_FEW | MM_VERIFY_NO_MODEL | MM_VERIFY_WEAK)) != 0;
    // the kept matches in their input order: the inliers of F, or -- a failed pair -- all of them (on_fail 0) / none (1)
    int kept = 0;
    if (!(failed && a.on_fail != 0)) {
        const VfyModel M_(F);
        kept = mm_pairs_compact(a, p, mm, [&](int j) { return failed || mm_pair_inlier_of(M_, a, p, j); }, pairs_out, wcount);
    }
    if (tid == 0) {
        m_out[p] = kept;
#pragma unroll
        for (int c = 0; c < 9; ++c) Fm[9 * (size_t)p + c] = F[c];
        cost_out[p] = cost;
        info[4 * (size_t)p] = flags;
        info[4 * (size_t)p + 1] = n_in;
        info[4 * (size_t)p + 2] = best_h;
        info[4 * (size_t)p + 3] = n_valid;
    }
}

}  // namespace

extern "C" size_t mm_verify_workspace_bytes(int n_pairs, int n_hyp) {
    return mm_pairs_workspace(n_pairs, n_hyp);
}

extern "C" int mm_verify_matches(mm_ctx *ctx, const float *kp_xy, const int32_t *pairs, const int32_t *m, int n_pairs, int cap,
                                 const mm_verify_params *prm, int32_t *pairs_out, int32_t *m_out, double *Fm, double *cost,
                                 int32_t *info, void *ws, size_t ws_bytes) {
    // every argument is judged before the context is looked at: nothing below this block runs on a bad call
    if (!prm || n_pairs < 0) return mm_fail(ctx, MM_ERR_ARG, "mm_verify_matches: bad argument");
    if (prm->n_hyp < 1 || prm->n_hyp > 4096) return mm_fail(ctx, MM_ERR_ARG, "mm_verify_matches: n_hyp must be in 1 .. 4096");
    if (!(prm->threshold_px >= 0.0))      // (negative or NaN; +inf keeps every well-formed match)
        return mm_fail(ctx, MM_ERR_ARG, "mm_verify_matches: threshold_px must not be negative");
    if (prm->refit_iters < 0 || prm->refit_iters > 1000 || prm->min_inliers < 0 || (prm->on_fail != 0 && prm->on_fail != 1))
        return mm_fail(ctx, MM_ERR_ARG, "mm_verify_matches: bad parameter");
    if (n_pairs > 0 && (!kp_xy || !pairs || !m || !pairs_out || !m_out || !Fm || !cost || !info || !ws || cap <= 0 || pairs == pairs_out))
        return mm_fail(ctx, MM_ERR_ARG, "mm_verify_matches: bad argument");
    if (n_pairs > 0 && ws_bytes < mm_verify_workspace_bytes(n_pairs, prm->n_hyp))
        return mm_fail(ctx, MM_ERR_WORKSPACE, "mm_verify_matches: workspace too small");
    if (!ctx) return MM_ERR_ARG;
    if (n_pairs == 0) return MM_OK;
    if (((uintptr_t)kp_xy | (uintptr_t)pairs | (uintptr_t)pairs_out) & 7)
        return mm_fail(ctx, MM_ERR_ARG, "mm_verify_matches: kp_xy, pairs and pairs_out must be 8-byte aligned");
    VfyArgs a;
    a.kp_xy = kp_xy;
    a.pairs = pairs;
    a.m = m;
    a.n_pairs = n_pairs;
    a.cap = cap;
    a.n_hyp = prm->n_hyp;
    a.min_matches = prm->min_matches < 16 ? 16 : prm->min_matches;
    a.min_inliers = prm->min_inliers;
    a.refit_iters = prm->refit_iters;
    a.on_fail = prm->on_fail;
    a.seed = prm->seed;
    a.pair_base = prm->pair_base;
    a.tau2 = prm->threshold_px * prm->threshold_px;
    mm_pairs_carve(a, ws);
    const dim3 per_hyp((unsigned)n_pairs, (unsigned)((a.n_hyp + 63) / 64));
    MM_LAUNCH(ctx, "vfy_normalise_kernel", vfy_normalise_kernel, dim3((unsigned)n_pairs), dim3(VFY_THREADS), 0, a);
    MM_LAUNCH(ctx, "vfy_hypothesis_kernel", vfy_hypothesis_kernel, per_hyp, dim3(64), 0, a);
    MM_LAUNCH(ctx, "vfy_score_kernel", vfy_score_kernel, per_hyp, dim3(64), 0, a);
    MM_LAUNCH(ctx, "vfy_refit_kernel", vfy_refit_kernel, dim3((unsigned)n_pairs), dim3(VFY_THREADS), 0, a, pairs_out, m_out, Fm, cost, info);
    return MM_OK;
}
