// Camera poses from verified matches: a relative pose per consecutive frame pair, and the pairs chained into one set of
// extrinsics (gfx950, f64).
//
// No reference counterpart: the reference takes every keyframe's pose from a chessboard (findChessboardCorners + solvePnP).
// The definition -- decomposition of E = K^T F K, the four candidates, the depth vote, flags, the median scale ratio and the
// composition -- is in include/meatmodeler.h (mm_recover_poses, mm_chain_poses); this file maps it:
//   pose_pair_kernel     one workgroup per pair: every thread forms the decomposition from the same nine doubles (3 x 3 cyclic
//                        Jacobi in registers, every index static), the threads stride over the pair's matches and count the
//                        votes of the four candidates in integers, a second pass writes the winner's depths
//   chain_ratio_kernel   one workgroup per pair: integer min-scatter of the previous pair's rows into an LDS table indexed by
//                        key point, then the lower median of the depth ratios by a radix select on their bit patterns (eight
//                        256-bin integer histograms; the ratios are recomputed per pass, one division each)
//   chain_compose_kernel one workgroup: the pairs' motions staged through LDS 256 at a time, composed in order by one lane
// Built without FMA contraction (Makefile): the vote pass and the depth pass evaluate the same expression and must agree on
// every bit, and a product-sum then has one value whatever the compiler makes of its surroundings.  All counts are integers,
// the only atomics are integer min / add in LDS: a pair's row does not depend on which other pairs share the call.
#include "mm_pairs.h"

namespace {

constexpr int POSE_THREADS = 256;
constexpr int POSE_WAVES = POSE_THREADS / 64;
constexpr int CHAIN_MAX_CAP = 8192;

struct PoseArgs {
    const float *kp_xy;
    const int32_t *pairs, *m;
    const double *Fm;
    int n_pairs, cap, min_matches;
    double min_front_frac, ambiguous_frac;
    double K[9];
    double Ki[5];      // K^-1 = [[Ki0, Ki1, Ki2], [0, Ki3, Ki4], [0, 0, 1]]
    double *R, *t, *sigma, *depth;
    int32_t *info;
};

// depths (l1, l2) of the least-squares solution of l2 b = l1 r + t; true: both finite and positive
__device__ __forceinline__ bool pose_depths(Vec3 r, Vec3 b, Vec3 t, double &l1, double &l2) {
    const double rr = dot3(r, r), bb = dot3(b, b), rb = dot3(r, b), bt = dot3(b, t), rt = dot3(r, t);
    const double det = rr * bb - rb * rb;
    l1 = (rb * bt - rt * bb) / det;
    l2 = (rr * bt - rb * rt) / det;
    return isfinite(l1) && isfinite(l2) && l1 > 0.0 && l2 > 0.0;
}

// R = U W V^T (transposed_w false) or U W^T V^T (true), row-major; U and V given by their columns
__device__ __forceinline__ void pose_rotation(Vec3 u1, Vec3 u2, Vec3 u3, Vec3 v1, Vec3 v2, Vec3 v3, bool transposed_w, double (&R)[9]) {
    // U W = [u2, -u1, u3], U W^T = [-u2, u1, u3]
    const double sg = transposed_w ? -1.0 : 1.0;
    const Vec3 c1 = Vec3{sg * u2.x, sg * u2.y, sg * u2.z}, c2 = Vec3{-sg * u1.x, -sg * u1.y, -sg * u1.z};
    R[0] = (c1.x * v1.x + c2.x * v2.x) + u3.x * v3.x;
    R[1] = (c1.x * v1.y + c2.x * v2.y) + u3.x * v3.y;
    R[2] = (c1.x * v1.z + c2.x * v2.z) + u3.x * v3.z;
    R[3] = (c1.y * v1.x + c2.y * v2.x) + u3.y * v3.x;
    R[4] = (c1.y * v1.y + c2.y * v2.y) + u3.y * v3.y;
    R[5] = (c1.y * v1.z + c2.y * v2.z) + u3.y * v3.z;
    R[6] = (c1.z * v1.x + c2.z * v2.x) + u3.z * v3.x;
    R[7] = (c1.z * v1.y + c2.z * v2.y) + u3.z * v3.y;
    R[8] = (c1.z * v1.z + c2.z * v2.z) + u3.z * v3.z;
}

__global__ __launch_bounds__(POSE_THREADS) void pose_pair_kernel(PoseArgs a) {
    __shared__ int cnt[POSE_WAVES][5];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mm = mm_pair_count(a.m, a.cap, p);
    const double nan = __builtin_nan("");
    int flags = 0;
    double Ra[9], Rb[9];
    Vec3 tp = Vec3{nan, nan, nan};
    double s1 = nan, s2 = nan;
    bool model = false;
#pragma unroll
    for (int k = 0; k < 9; ++k) Ra[k] = Rb[k] = nan;

    if (mm < a.min_matches) {
        flags |= MM_POSE_TOO_FEW;
    } else {
        double F[9];
        bool finite = true;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            F[k] = a.Fm[9 * (size_t)p + k];
            finite = finite && isfinite(F[k]);
        }
        // E = K^T (F K), G = E^T E
        double FK[9], E[9], G[3][3], V[3][3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) FK[3 * r + c] = (F[3 * r] * a.K[c] + F[3 * r + 1] * a.K[3 + c]) + F[3 * r + 2] * a.K[6 + c];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) E[3 * r + c] = (a.K[r] * FK[c] + a.K[3 + r] * FK[3 + c]) + a.K[6 + r] * FK[6 + c];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) G[r][c] = (E[r] * E[c] + E[3 + r] * E[3 + c]) + E[6 + r] * E[6 + c];
        mm_identity<3>(V);
        mm_jacobi<3>(G, V);
        // v3: smallest eigenvalue, v1: largest, ties to the lowest column (selected without a runtime index)
        double lo = G[0][0], hi = G[0][0];
        Vec3 v3 = Vec3{V[0][0], V[1][0], V[2][0]}, v1 = v3;
#pragma unroll
        for (int c = 1; c < 3; ++c) {
            if (G[c][c] < lo) {
                lo = G[c][c];
                v3 = Vec3{V[0][c], V[1][c], V[2][c]};
            }
            if (G[c][c] > hi) {
                hi = G[c][c];
                v1 = Vec3{V[0][c], V[1][c], V[2][c]};
            }
        }
        const Vec3 v2 = cross3(v3, v1);
        const Vec3 e1 = mat3(E, v1), e2 = mat3(E, v2);
        s1 = sqrt(dot3(e1, e1));
        const Vec3 u1 = Vec3{e1.x / s1, e1.y / s1, e1.z / s1};
        const double d12 = dot3(u1, e2);
        const Vec3 w2 = Vec3{e2.x - d12 * u1.x, e2.y - d12 * u1.y, e2.z - d12 * u1.z};
        s2 = sqrt(dot3(w2, w2));
        const Vec3 u2 = Vec3{w2.x / s2, w2.y / s2, w2.z / s2};
        const Vec3 u3 = cross3(u1, u2);
        model = finite && isfinite(s1) && isfinite(s2) && s1 > 0.0 && s2 > 0.0;
        if (model) {
            pose_rotation(u1, u2, u3, v1, v2, v3, false, Ra);
            pose_rotation(u1, u2, u3, v1, v2, v3, true, Rb);
            tp = u3;
        } else {
            flags |= MM_POSE_NO_MODEL;
        }
    }
    const Vec3 tn = Vec3{-tp.x, -tp.y, -tp.z};

    // votes of the four candidates and the malformed rows, in integers
    int v0 = 0, v1c = 0, v2c = 0, v3c = 0, bad = 0;
    for (int j = tid; j < mm; j += POSE_THREADS) {
        Vec3 ra, rb;
        const bool wf = mm_pair_rays(a, p, j, ra, rb);
        bad += wf ? 0 : 1;
        if (model && wf) {
            const Vec3 qa = mat3(Ra, ra), qb = mat3(Rb, ra);
            double l1, l2;
            v0 += pose_depths(qa, rb, tp, l1, l2) ? 1 : 0;
            v1c += pose_depths(qa, rb, tn, l1, l2) ? 1 : 0;
            v2c += pose_depths(qb, rb, tp, l1, l2) ? 1 : 0;
            v3c += pose_depths(qb, rb, tn, l1, l2) ? 1 : 0;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        v0 += __shfl_xor(v0, off, 64);
        v1c += __shfl_xor(v1c, off, 64);
        v2c += __shfl_xor(v2c, off, 64);
        v3c += __shfl_xor(v3c, off, 64);
        bad += __shfl_xor(bad, off, 64);
    }
    if (lane == 0) {
        cnt[wave][0] = v0;
        cnt[wave][1] = v1c;
        cnt[wave][2] = v2c;
        cnt[wave][3] = v3c;
        cnt[wave][4] = bad;
    }
    __syncthreads();
    v0 = cnt[0][0] + cnt[1][0] + cnt[2][0] + cnt[3][0];
    v1c = cnt[0][1] + cnt[1][1] + cnt[2][1] + cnt[3][1];
    v2c = cnt[0][2] + cnt[1][2] + cnt[2][2] + cnt[3][2];
    v3c = cnt[0][3] + cnt[1][3] + cnt[2][3] + cnt[3][3];
    bad = cnt[0][4] + cnt[1][4] + cnt[2][4] + cnt[3][4];
    if (bad > 0) flags |= MM_POSE_MALFORMED;

    int winner = -1;
    double Rw[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) Rw[k] = nan;
    Vec3 tw = Vec3{nan, nan, nan};
    if (model) {
        // largest count, ties to the lowest c; the runner-up is the largest of the other three
        int best = v0;
        winner = 0;
        if (v1c > best) {
            best = v1c;
            winner = 1;
        }
        if (v2c > best) {
            best = v2c;
            winner = 2;
        }
        if (v3c > best) {
            best = v3c;
            winner = 3;
        }
        int second = 0;
        second = (winner != 0 && v0 > second) ? v0 : second;
        second = (winner != 1 && v1c > second) ? v1c : second;
        second = (winner != 2 && v2c > second) ? v2c : second;
        second = (winner != 3 && v3c > second) ? v3c : second;
        if ((double)best < a.min_front_frac * (double)mm || (double)second >= a.ambiguous_frac * (double)best)
            flags |= MM_POSE_AMBIGUOUS;
#pragma unroll
        for (int k = 0; k < 9; ++k) Rw[k] = winner < 2 ? Ra[k] : Rb[k];
        tw = (winner & 1) ? tn : tp;
    }

    // the winner's depths of the rows that voted for it; NaN everywhere else, rows at or beyond m included
    for (int j = tid; j < a.cap; j += POSE_THREADS) {
        double l1 = nan, l2 = nan;
        if (model && j < mm) {
            Vec3 ra, rb;
            if (mm_pair_rays(a, p, j, ra, rb)) {
                double d1, d2;
                if (pose_depths(mat3(Rw, ra), rb, tw, d1, d2)) {
                    l1 = d1;
                    l2 = d2;
                }
            }
        }
        reinterpret_cast<double2 *>(a.depth)[(size_t)p * a.cap + j] = make_double2(l1, l2);
    }
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) a.R[9 * (size_t)p + k] = Rw[k];
        a.t[3 * (size_t)p] = tw.x;
        a.t[3 * (size_t)p + 1] = tw.y;
        a.t[3 * (size_t)p + 2] = tw.z;
        a.sigma[2 * (size_t)p] = s1;
        a.sigma[2 * (size_t)p + 1] = s2;
        int32_t *o = a.info + 8 * (size_t)p;
        o[0] = flags;
        o[1] = winner;
        o[2] = v0;
        o[3] = v1c;
        o[4] = v2c;
        o[5] = v3c;
        o[6] = mm;
        o[7] = 0;
    }
}

// ---- chain: scale ratio of pair p against pair p - 1 ---------------------------------------------------------------------------
struct ChainArgs {
    const int32_t *pairs, *m, *info;
    const double *depth, *R, *t;
    int n_pairs, cap, min_common;
    double E0[12];
    double *extrinsics, *scale, *rho;
    int32_t *chain_info;
};

__device__ __forceinline__ int chain_count(const ChainArgs &a, int p) {
    const int mm = a.m[p];
    return mm < 0 ? 0 : (mm > a.cap ? a.cap : mm);
}
__device__ __forceinline__ bool chain_broken(const ChainArgs &a, int p) {
    return (a.info[8 * (size_t)p] & (MM_POSE_TOO_FEW | MM_POSE_NO_MODEL)) != 0;
}
__device__ __forceinline__ bool chain_pos(double d) { return isfinite(d) && d > 0.0; }

// ratio of row j of pair p (true: the row has one): its query key point was a train of pair p - 1 with a positive depth
__device__ __forceinline__ bool chain_ratio(const ChainArgs &a, int p, int j, const int *tab, double &rho) {
    const int q = a.pairs[2 * ((size_t)p * a.cap + j)];
    if ((unsigned)q >= (unsigned)a.cap) return false;
    const int i = tab[q];
    const double d = a.depth[2 * ((size_t)p * a.cap + j)];
    if (i == INT32_MAX || !chain_pos(d)) return false;
    rho = a.depth[2 * ((size_t)(p - 1) * a.cap + i) + 1] / d;
    return true;
}

__global__ __launch_bounds__(POSE_THREADS) void chain_ratio_kernel(ChainArgs a) {
    extern __shared__ int tab[];      // [cap]: lowest row of pair p - 1 per train key point
    __shared__ int hist[256];
    __shared__ int total;
    const int p = blockIdx.x, tid = threadIdx.x;
    int flags = 0, n_common = 0;
    double rho = 1.0;
    if (chain_broken(a, p)) {
        flags = MM_CHAIN_BROKEN;
    } else if (p > 0 && chain_broken(a, p - 1)) {
        flags = MM_CHAIN_FEW_COMMON;
    } else if (p > 0) {      // (all three tests are uniform over the workgroup)
        const int m0 = chain_count(a, p - 1), m1 = chain_count(a, p);
        for (int k = tid; k < a.cap; k += POSE_THREADS) tab[k] = INT32_MAX;
        if (tid == 0) total = 0;
        __syncthreads();
        for (int i = tid; i < m0; i += POSE_THREADS) {
            const int tr = a.pairs[2 * ((size_t)(p - 1) * a.cap + i) + 1];
            if ((unsigned)tr < (unsigned)a.cap && chain_pos(a.depth[2 * ((size_t)(p - 1) * a.cap + i) + 1])) atomicMin(&tab[tr], i);
        }
        __syncthreads();
        int mine = 0;
        for (int j = tid; j < m1; j += POSE_THREADS) {
            double r;
            mine += chain_ratio(a, p, j, tab, r) ? 1 : 0;
        }
        if (mine) atomicAdd(&total, mine);
        __syncthreads();
        n_common = total;
        if (n_common < a.min_common) {
            flags = MM_CHAIN_FEW_COMMON;
        } else if (n_common > 0) {
            // the (n_common - 1) / 2-th smallest: positive doubles order like their bit patterns; one byte per pass, high first
            int k = (n_common - 1) / 2;
            unsigned long long prefix = 0ull;
            for (int shift = 56; shift >= 0; shift -= 8) {
                __syncthreads();
                hist[tid] = 0;      // (POSE_THREADS == 256 bins)
                __syncthreads();
                const unsigned long long himask = shift == 56 ? 0ull : (~0ull << (shift + 8));
                for (int j = tid; j < m1; j += POSE_THREADS) {
                    double r;
                    if (chain_ratio(a, p, j, tab, r)) {
                        const unsigned long long bits = (unsigned long long)__double_as_longlong(r);
                        if ((bits & himask) == prefix) atomicAdd(&hist[(int)((bits >> shift) & 255ull)], 1);
                    }
                }
                __syncthreads();
                int digit = 0, below = 0;
                for (int b = 0; b < 256; ++b) {      // (every thread reads the same words: same digit everywhere)
                    const int h = hist[b];
                    if (below + h > k) {
                        digit = b;
                        break;
                    }
                    below += h;
                }
                k -= below;
                prefix |= (unsigned long long)digit << shift;
            }
            rho = __longlong_as_double((long long)prefix);
        }
    }
    if (tid == 0) {
        a.rho[p] = rho;
        a.chain_info[2 * (size_t)p] = flags;
        a.chain_info[2 * (size_t)p + 1] = n_common;
    }
}

// ---- chain: composition in order ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(POSE_THREADS) void chain_compose_kernel(ChainArgs a) {
    __shared__ double mot[POSE_THREADS][13];      // in: R (9), t (3), rho; out: T_{p+1} (12), s_p
    const int tid = threadIdx.x;
    double T[12], s = 1.0;      // (lane 0's running state)
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = a.E0[k];
    if (tid < 12) a.extrinsics[tid] = a.E0[tid];
    for (int base = 0; base < a.n_pairs; base += POSE_THREADS) {
        const int n = min(POSE_THREADS, a.n_pairs - base), p = base + tid;
        __syncthreads();
        if (tid < n) {
            const bool broken = chain_broken(a, p);
#pragma unroll
            for (int k = 0; k < 9; ++k) mot[tid][k] = broken ? ((k % 4 == 0) ? 1.0 : 0.0) : a.R[9 * (size_t)p + k];
#pragma unroll
            for (int k = 0; k < 3; ++k) mot[tid][9 + k] = broken ? 0.0 : a.t[3 * (size_t)p + k];
            mot[tid][12] = a.rho[p];
        }
        __syncthreads();
        if (tid == 0) {
            for (int i = 0; i < n; ++i) {
                double R[9], N[12];
#pragma unroll
                for (int k = 0; k < 9; ++k) R[k] = mot[i][k];
                s = s * mot[i][12];
#pragma unroll
                for (int r = 0; r < 3; ++r) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) N[4 * r + c] = (R[3 * r] * T[c] + R[3 * r + 1] * T[4 + c]) + R[3 * r + 2] * T[8 + c];
                    N[4 * r + 3] = N[4 * r + 3] + s * mot[i][9 + r];
                }
#pragma unroll
                for (int k = 0; k < 12; ++k) {
                    T[k] = N[k];
                    mot[i][k] = N[k];
                }
                mot[i][12] = s;
            }
        }
        __syncthreads();
        if (tid < n) {
#pragma unroll
            for (int k = 0; k < 12; ++k) a.extrinsics[12 * ((size_t)p + 1) + k] = mot[tid][k];
            a.scale[p] = mot[tid][12];
        }
    }
}

}  // namespace

extern "C" int mm_recover_poses(mm_ctx *ctx, const double *K, const float *kp_xy, const int32_t *pairs, const int32_t *m,
                                const double *Fm, int n_pairs, int cap, const mm_pose_params *prm, double *R, double *t,
                                double *sigma, double *depth, int32_t *info) {
    // every argument is judged before the context is looked at: nothing below this block runs on a bad call
    if (!prm || !K || n_pairs < 0 || cap <= 0) return mm_fail(ctx, MM_ERR_ARG, "mm_recover_poses: bad argument");
    if (!(prm->min_front_frac >= 0.0 && prm->min_front_frac <= 1.0) || !(prm->ambiguous_frac >= 0.0 && prm->ambiguous_frac <= 1.0))
        return mm_fail(ctx, MM_ERR_ARG, "mm_recover_poses: min_front_frac and ambiguous_frac must be in [0, 1]");
    bool k_ok = K[3] == 0.0 && K[6] == 0.0 && K[7] == 0.0 && K[8] == 1.0 && K[0] != 0.0 && K[4] != 0.0;
    for (int k = 0; k < 9; ++k) k_ok = k_ok && std::isfinite(K[k]);
    if (!k_ok)
        return mm_fail(ctx, MM_ERR_ARG, "mm_recover_poses: K must be finite and upper triangular with K[8] = 1 and non-zero focal lengths");
    if (n_pairs > 0 && (!kp_xy || !pairs || !m || !Fm || !R || !t || !sigma || !depth || !info))
        return mm_fail(ctx, MM_ERR_ARG, "mm_recover_poses: bad argument");
    if (!ctx) return MM_ERR_ARG;
    if (n_pairs == 0) return MM_OK;
    if (((uintptr_t)kp_xy | (uintptr_t)pairs) & 7 || ((uintptr_t)depth & 15))
        return mm_fail(ctx, MM_ERR_ARG, "mm_recover_poses: kp_xy and pairs must be 8-byte aligned, depth 16-byte aligned");
    PoseArgs a;
    a.kp_xy = kp_xy;
    a.pairs = pairs;
    a.m = m;
    a.Fm = Fm;
    a.n_pairs = n_pairs;
    a.cap = cap;
    a.min_matches = prm->min_matches < 8 ? 8 : prm->min_matches;
    a.min_front_frac = prm->min_front_frac;
    a.ambiguous_frac = prm->ambiguous_frac;
    for (int k = 0; k < 9; ++k) a.K[k] = K[k];
    mm_k_inverse(K, a.Ki);
    a.R = R;
    a.t = t;
    a.sigma = sigma;
    a.depth = depth;
    a.info = info;
    MM_LAUNCH(ctx, "pose_pair_kernel", pose_pair_kernel, dim3((unsigned)n_pairs), dim3(POSE_THREADS), 0, a);
    return MM_OK;
}

extern "C" int mm_chain_poses(mm_ctx *ctx, const int32_t *pairs, const int32_t *m, const double *depth, const double *R,
                              const double *t, const int32_t *info, int n_pairs, int cap, const double *E0, int min_common,
                              double *extrinsics, double *scale, double *rho, int32_t *chain_info) {
    if (!E0 || n_pairs < 0 || cap <= 0 || cap > CHAIN_MAX_CAP || min_common < 0)
        return mm_fail(ctx, MM_ERR_ARG, "mm_chain_poses: bad argument (cap must be in 1 .. 8192)");
    if (n_pairs > 0 && (!pairs || !m || !depth || !R || !t || !info || !extrinsics || !scale || !rho || !chain_info))
        return mm_fail(ctx, MM_ERR_ARG, "mm_chain_poses: bad argument");
    if (!ctx) return MM_ERR_ARG;
    if (n_pairs == 0) return MM_OK;
    ChainArgs a;
    a.pairs = pairs;
    a.m = m;
    a.info = info;
    a.depth = depth;
    a.R = R;
    a.t = t;
    a.n_pairs = n_pairs;
    a.cap = cap;
    a.min_common = min_common;
    for (int k = 0; k < 12; ++k) a.E0[k] = E0[k];
    a.extrinsics = extrinsics;
    a.scale = scale;
    a.rho = rho;
    a.chain_info = chain_info;
    MM_LAUNCH(ctx, "chain_ratio_kernel", chain_ratio_kernel, dim3((unsigned)n_pairs), dim3(POSE_THREADS), (size_t)cap * sizeof(int), a);
    MM_LAUNCH(ctx, "chain_compose_kernel", chain_compose_kernel, dim3(1), dim3(POSE_THREADS), 0, a);
    return MM_OK;
}
