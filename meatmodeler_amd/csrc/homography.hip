// A homography per consecutive frame pair: the planar / rotation-only verdict beside mm_verify_matches, and the motion a
// homography implies beside mm_recover_poses (gfx950, f64).
//
// No reference counterpart: the reference takes its poses from a chessboard.  A fundamental matrix is not determined when the
// camera only turns or when the scene is a plane; a homography explains exactly those pairs.  The definition -- sampling,
// the reduced DLT, the symmetric transfer distance, MSAC, refit, the verdict, the decomposition into four motions, the depth
// vote -- is in include/meatmodeler.h (mm_verify_homography, mm_recover_poses_homography); this file maps it:
//   hg_normalise_kernel   one workgroup per pair: Hartley centroid / scale of both images over the well-formed matches
//   hg_hypothesis_kernel  one lane per (pair, hypothesis): four sampled matches, near-collinear triples rejected in both
//                         images, the 24 sums and the reduced DLT in registers (every index static), rank guard, denormalise
//   hg_score_kernel       lane = hypothesis, H and its adjugate in registers; the pair's matches go through LDS in tiles and
//                         every lane reads the same address (broadcast), summing min(d^2, tau^2) over j ascending
//   hg_finish_kernel      one workgroup per pair: argmin, refit rounds (24 sums over the inliers, the same solve), the verdict
//                         against the fundamental matrix's inlier count, order-preserving compaction, outputs
//   hp_pair_kernel        one workgroup per pair: G = K^-1 H K, its eigenpairs, the sign from the matches, then either the
//                         polar factor (rotation only) or the four plane motions, integer votes, the winner's depths
// The reduced DLT and the triple rule are mm_geom.h's (shared with resect.hip); how a match is read, the normalisation and the
// MSAC skeleton are mm_pairs.h's (shared with verify.hip); here is the model: HgModel, hg_solve's own tail, the verdict.
// Built without FMA contraction (Makefile): the inlier test is evaluated in several passes that must agree on every bit, the
// depth pass repeats the vote pass, and the NumPy restatement of the tests follows the header operation by operation.
// Plain f64 VALU work; sums in an order that depends on the pair alone (per-thread strides, xor butterflies, waves in order),
// no float atomics: a pair's row repeats bit for bit whatever else shares the call.
#include "mm_pairs.h"

namespace {

constexpr int HG_THREADS = 256;      // normalise / finish / pose: one workgroup per pair
constexpr int HG_WAVES = HG_THREADS / 64;
static_assert(HG_THREADS == MM_BLOCK_THREADS, "the mm_block_* helpers are written for this workgroup");

struct HgArgs : MmPairArgs {      // (model_h: the hypotheses' H)
    const int32_t *verify_info;
    double collinear_tol, degenerate_frac;
};

// the model of the MSAC skeleton (mm_pairs.h): H with its adjugate prepared once; hg_adjugate and hg_transfer are mm_pairs.h's
struct HgModel {
    double H[9], A[9];
    __device__ __forceinline__ explicit HgModel(const double (&h)[9]) {
#pragma unroll
        for (int c = 0; c < 9; ++c) H[c] = h[c];
        hg_adjugate(H, A);
    }
    __device__ __forceinline__ double distance(double x, double y, double xp, double yp) const { return hg_transfer(H, A, x, y, xp, yp); }
};

// H from the 24 sums: the reduced DLT (mm_plane_dlt), the rank guard on the normalised matrix, H = T'^-1 H^ T, unit Frobenius
// norm, (H c)_2 >= 0.
// false: a failed pivot, a rank below three or a non-finite entry.
__device__ __forceinline__ bool hg_solve(const double (&acc)[24], double cx, double cy, double s, double cx2, double cy2, double s2,
                                         double (&H)[9]) {
    double h1[3], h2[3], h3[3];
    bool ok = mm_plane_dlt(acc, h1, h2, h3);
    const double Hn[9] = {h1[0], h1[1], h1[2], h2[0], h2[1], h2[2], h3[0], h3[1], h3[2]};
    {   // rank guard: the smallest eigenvalue of H^^T H^ must be above 1e-8 of the largest (a NaN does not pass)
        double G[3][3], V[3][3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) G[r][c] = (Hn[r] * Hn[c] + Hn[3 + r] * Hn[3 + c]) + Hn[6 + r] * Hn[6 + c];
        mm_identity<3>(V);
        mm_jacobi<3>(G, V);
        double lo = G[0][0] < G[1][1] ? G[0][0] : G[1][1], hi = G[0][0] > G[1][1] ? G[0][0] : G[1][1];
        lo = lo < G[2][2] ? lo : G[2][2];
        hi = hi > G[2][2] ? hi : G[2][2];
        ok = ok && lo > 1e-8 * hi;
    }
    double A[9];      // A = H^ T with T = [[s, 0, -s cx], [0, s, -s cy], [0, 0, 1]]
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        A[3 * r] = s * Hn[3 * r];
        A[3 * r + 1] = s * Hn[3 * r + 1];
        A[3 * r + 2] = (Hn[3 * r + 2] - (s * cx) * Hn[3 * r]) - (s * cy) * Hn[3 * r + 1];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {      // H = T'^-1 A with T'^-1 = [[1/s', 0, cx'], [0, 1/s', cy'], [0, 0, 1]]
        H[c] = A[c] / s2 + cx2 * A[6 + c];
        H[3 + c] = A[3 + c] / s2 + cy2 * A[6 + c];
        H[6 + c] = A[6 + c];
    }
    double nn = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) nn += H[k] * H[k];
    const double w = (H[6] * cx + H[7] * cy) + H[8];
    const double inv = (w < 0.0 ? -1.0 : 1.0) / sqrt(nn);
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        H[k] *= inv;
        ok = ok && isfinite(H[k]);
    }
    return ok;
}

// ---- normalisation over all well-formed matches of the pair -----------------------------------------------------------------
__global__ __launch_bounds__(HG_THREADS) void hg_normalise_kernel(HgArgs a) { mm_pairs_normalise(a); }

// ---- one hypothesis per lane --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void hg_hypothesis_kernel(HgArgs a) {
    const int p = blockIdx.x;
    const int h = blockIdx.y * 64 + threadIdx.x;
    const int mm = mm_pair_count(a.m, a.cap, p);
    if (h >= a.n_hyp || mm < a.min_matches) return;      // (a pair with too few matches is never scored either)
    const double *nr = a.norm + 8 * (size_t)p;
    const double cx = nr[0], cy = nr[1], s = nr[2], cx2 = nr[3], cy2 = nr[4], s2 = nr[5];
    bool ok = isfinite(s) && isfinite(s2);
    const uint32_t base = mm_pcg(mm_pcg(a.seed + mm_pcg(a.pair_base + (uint32_t)p)) + (uint32_t)h);
    int pick[4];
    ok = mm_sample_distinct<4>(base, mm, pick) && ok;
    double xa[4], ya[4], xb[4], yb[4], acc[24];
#pragma unroll
    for (int k = 0; k < 24; ++k) acc[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        double x, y, xp, yp;
        ok = mm_pair_load(a, p, pick[k], x, y, xp, yp) && ok;
        xa[k] = s * (x - cx);
        ya[k] = s * (y - cy);
        xb[k] = s2 * (xp - cx2);
        yb[k] = s2 * (yp - cy2);
        mm_plane_accumulate(acc, xa[k], ya[k], xb[k], yb[k]);
    }
    ok = mm_triples_ok(xa, ya, a.collinear_tol) && ok;
    ok = mm_triples_ok(xb, yb, a.collinear_tol) && ok;
    double H[9];
    ok = hg_solve(acc, cx, cy, s, cx2, cy2, s2, H) && ok;
    double *o = a.model_h + ((size_t)p * a.n_hyp + h) * 9;
    const double nan = __builtin_nan("");
#pragma unroll
    for (int c = 0; c < 9; ++c) o[c] = ok ? H[c] : nan;
}

// ---- MSAC cost of every hypothesis --------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void hg_score_kernel(HgArgs a) { mm_pairs_score<HgModel>(a); }

// ---- winner, refit, verdict, compaction -----------------------------------------------------------------------------------
__global__ __launch_bounds__(HG_THREADS) void hg_finish_kernel(HgArgs a, int32_t *__restrict__ pairs_out, int32_t *__restrict__ m_out,
                                                               double *__restrict__ Hm, double *__restrict__ cost_out,
                                                               int32_t *__restrict__ info) {
    __shared__ double sm[HG_WAVES * 24];
    __shared__ double bc[HG_WAVES];
    __shared__ int bh[HG_WAVES], wcount[HG_WAVES];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int mm = mm_pair_count(a.m, a.cap, p);
    const double nan = __builtin_nan("");
    int flags = a.norm[8 * (size_t)p + 6] > 0.0 ? MM_HOMOG_MALFORMED : 0;
    double H[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) H[c] = nan;
    double cost = nan;
    int n_in = 0, best_h = -1, n_valid = 0;
    // a refit round: the 24 sums over the inliers of the current H, the same solve
    const auto refit = [&](const HgModel &M, double cx, double cy, double s, double cx2, double cy2, double s2, double (&Hn)[9]) {
        double acc[24];
#pragma unroll
        for (int k = 0; k < 24; ++k) acc[k] = 0.0;
        for (int j = tid; j < mm; j += HG_THREADS) {
            double x, y, xp, yp;
            mm_pair_load(a, p, j, x, y, xp, yp);
            if (mm_pair_inlier(M.distance(x, y, xp, yp), a.tau2))
                mm_plane_accumulate(acc, s * (x - cx), s * (y - cy), s2 * (xp - cx2), s2 * (yp - cy2));
        }
        mm_block_sum<24>(acc, sm);
        return hg_solve(acc, cx, cy, s, cx2, cy2, s2, Hn);
    };
    const int none = mm_pairs_winner_refit<HgModel>(a, p, mm, 4, sm, bc, bh, refit, H, cost, n_in, best_h, n_valid);
    if (none == MM_PAIRS_TOO_FEW) flags |= MM_HOMOG_TOO_FEW;
    if (none == MM_PAIRS_NO_MODEL) flags |= MM_HOMOG_NO_MODEL;
    if (none == 0 && n_in < a.min_inliers) flags |= MM_HOMOG_WEAK;

    const bool failed = (flags & (MM_HOMOG_TOO_FEW | MM_HOMOG_NO_MODEL | MM_HOMOG_WEAK)) != 0;
    int n_f = -1;
    if (a.verify_info != nullptr) {
        const int vflags = a.verify_info[4 * (size_t)p];
        n_f = a.verify_info[4 * (size_t)p + 1];
        if (!failed && ((vflags & 7) != 0 || (double)n_in >= a.degenerate_frac * (double)n_f)) flags |= MM_HOMOG_DEGENERATE;
    }
    // the inliers of H in their input order; a failed pair keeps none
    int kept = 0;
    if (!failed) {
        const HgModel M(H);
        kept = mm_pairs_compact(a, p, mm, [&](int j) { return mm_pair_inlier_of(M, a, p, j); }, pairs_out, wcount);
    }
    if (tid == 0) {
        m_out[p] = kept;
#pragma unroll
        for (int c = 0; c < 9; ++c) Hm[9 * (size_t)p + c] = H[c];
        cost_out[p] = cost;
        int32_t *o = info + 6 * (size_t)p;
        o[0] = flags;
        o[1] = n_in;
        o[2] = best_h;
        o[3] = n_valid;
        o[4] = n_f;
        o[5] = 0;
    }
}

// ---- the motion a homography implies --------------------------------------------------------------------------------------
struct HpArgs {
    const float *kp_xy;
    const int32_t *pairs, *m;
    const double *Hm, *hint;
    int n_pairs, cap, min_matches;
    double min_front_frac, ambiguous_frac, rotation_tol;
    double K[9];
    double Ki[5];      // K^-1 = [[Ki0, Ki1, Ki2], [0, Ki3, Ki4], [0, 0, 1]]
    double *R, *t, *sigma, *normal, *depth;
    int32_t *info;
};

// depths of a match on the plane n . X = 1 seen from camera 1: l1 = 1 / (n . a), l2 = (l1 R a + t)_z; true: both > 0
__device__ __forceinline__ bool hp_depths(const double (&R)[9], Vec3 t, Vec3 n, Vec3 ra, double &l1, double &l2) {
    l1 = 1.0 / dot3(n, ra);
    l2 = l1 * ((R[6] * ra.x + R[7] * ra.y) + R[8] * ra.z) + t.z;
    return isfinite(l1) && isfinite(l2) && l1 > 0.0 && l2 > 0.0;
}

// one of the two solutions: u = (a1 v1 + sg a3 v3) / den; U = [v2, u, v2 x u], W = [G v2, G u, G v2 x G u]; R = W U^T,
// n = v2 x u, t = (G - R) n
__device__ __forceinline__ void hp_solution(const double (&G)[9], Vec3 v1, Vec3 v2, Vec3 v3, double a1, double a3, double den,
                                            double (&R)[9], Vec3 &t, Vec3 &n) {
    const Vec3 u = Vec3{(a1 * v1.x + a3 * v3.x) / den, (a1 * v1.y + a3 * v3.y) / den, (a1 * v1.z + a3 * v3.z) / den};
    n = cross3(v2, u);
    const Vec3 w0 = mat3(G, v2), w1 = mat3(G, u);
    const Vec3 w2 = cross3(w0, w1);
    R[0] = (w0.x * v2.x + w1.x * u.x) + w2.x * n.x;
    R[1] = (w0.x * v2.y + w1.x * u.y) + w2.x * n.y;
    R[2] = (w0.x * v2.z + w1.x * u.z) + w2.x * n.z;
    R[3] = (w0.y * v2.x + w1.y * u.x) + w2.y * n.x;
    R[4] = (w0.y * v2.y + w1.y * u.y) + w2.y * n.y;
    R[5] = (w0.y * v2.z + w1.y * u.z) + w2.y * n.z;
    R[6] = (w0.z * v2.x + w1.z * u.x) + w2.z * n.x;
    R[7] = (w0.z * v2.y + w1.z * u.y) + w2.z * n.y;
    R[8] = (w0.z * v2.z + w1.z * u.z) + w2.z * n.z;
    t = Vec3{((G[0] - R[0]) * n.x + (G[1] - R[1]) * n.y) + (G[2] - R[2]) * n.z,
             ((G[3] - R[3]) * n.x + (G[4] - R[4]) * n.y) + (G[5] - R[5]) * n.z,
             ((G[6] - R[6]) * n.x + (G[7] - R[7]) * n.y) + (G[8] - R[8]) * n.z};
}

__device__ __forceinline__ int hp_block_count(int slot, int (*cnt)[5]) {      // (after the caller's barrier)
    return cnt[0][slot] + cnt[1][slot] + cnt[2][slot] + cnt[3][slot];
}

__global__ __launch_bounds__(HG_THREADS) void hp_pair_kernel(HpArgs a) {
    __shared__ int cnt[HG_WAVES][5];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mm = mm_pair_count(a.m, a.cap, p);
    const double nan = __builtin_nan("");
    int flags = 0;
    double G[9], Rp[9], Rm[9];
    Vec3 tpl = Vec3{nan, nan, nan}, tmi = tpl, npl = tpl, nmi = tpl;
    double sg1 = nan, sg2 = nan, sg3 = nan;
    bool model = false, rotation = false;
#pragma unroll
    for (int k = 0; k < 9; ++k) G[k] = Rp[k] = Rm[k] = nan;
    Vec3 v1 = tpl, v2 = tpl, v3 = tpl;
    double a1 = nan, a3 = nan, den = nan;

    if (mm < a.min_matches) {
        flags |= MM_POSE_TOO_FEW;
    } else {
        double H[9];
        bool finite = true;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            H[k] = a.Hm[9 * (size_t)p + k];
            finite = finite && isfinite(H[k]);
        }
        // G = K^-1 (H K), M = G^T G
        double HK[9], M[3][3], V[3][3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) HK[3 * r + c] = (H[3 * r] * a.K[c] + H[3 * r + 1] * a.K[3 + c]) + H[3 * r + 2] * a.K[6 + c];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            G[c] = (a.Ki[0] * HK[c] + a.Ki[1] * HK[3 + c]) + a.Ki[2] * HK[6 + c];
            G[3 + c] = a.Ki[3] * HK[3 + c] + a.Ki[4] * HK[6 + c];
            G[6 + c] = HK[6 + c];
        }
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) M[r][c] = (G[r] * G[c] + G[3 + r] * G[3 + c]) + G[6 + r] * G[6 + c];
        mm_identity<3>(V);
        mm_jacobi<3>(M, V);
        // l1 >= l2 >= l3 by a stable exchange sort of the columns -- (0,1), (1,2), (0,1), each exchanged only when the right
        // eigenvalue is strictly larger (every index static)
        double l[3] = {M[0][0], M[1][1], M[2][2]};
        Vec3 col[3] = {Vec3{V[0][0], V[1][0], V[2][0]}, Vec3{V[0][1], V[1][1], V[2][1]}, Vec3{V[0][2], V[1][2], V[2][2]}};
#define HP_EXCHANGE(i, j)            \
    if (l[j] > l[i]) {               \
        const double tl = l[i];      \
        l[i] = l[j];                 \
        l[j] = tl;                   \
        const Vec3 tc = col[i];      \
        col[i] = col[j];             \
        col[j] = tc;                 \
    }
        HP_EXCHANGE(0, 1)
        HP_EXCHANGE(1, 2)
        HP_EXCHANGE(0, 1)
#undef HP_EXCHANGE
        model = finite && isfinite(l[0]) && isfinite(l[1]) && isfinite(l[2]) && l[2] > 0.0;
        if (model) {
            sg1 = sqrt(l[0]);
            sg2 = sqrt(l[1]);
            sg3 = sqrt(l[2]);
#pragma unroll
            for (int k = 0; k < 9; ++k) G[k] = G[k] / sg2;
            v1 = col[0];
            v3 = col[2];
            v2 = cross3(v3, v1);
            rotation = sqrt(l[0] / l[2]) - 1.0 <= a.rotation_tol;
            const double n1 = l[0] / l[1], n3 = l[2] / l[1];      // the normalised eigenvalues (the middle one is 1)
            a1 = sqrt(1.0 - n3);
            a3 = sqrt(n1 - 1.0);
            den = sqrt(n1 - n3);
        }
    }

    // the sign of G from the well-formed matches: b . (G a) should be positive; and the malformed rows
    int neg = 0, pos = 0, bad = 0;
    for (int j = tid; j < mm; j += HG_THREADS) {
        Vec3 ra, rb;
        const bool wf = mm_pair_rays(a, p, j, ra, rb);
        bad += wf ? 0 : 1;
        if (model && wf) {
            const double d = dot3(rb, mat3(G, ra));
            neg += d < 0.0 ? 1 : 0;
            pos += d > 0.0 ? 1 : 0;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        neg += __shfl_xor(neg, off, 64);
        pos += __shfl_xor(pos, off, 64);
        bad += __shfl_xor(bad, off, 64);
    }
    if (lane == 0) {
        cnt[wave][0] = neg;
        cnt[wave][1] = pos;
        cnt[wave][2] = bad;
    }
    __syncthreads();
    neg = hp_block_count(0, cnt);
    pos = hp_block_count(1, cnt);
    bad = hp_block_count(2, cnt);
    __syncthreads();      // (cnt is rewritten by the vote)
    if (bad > 0) flags |= MM_POSE_MALFORMED;
    if (model && neg > pos) {
#pragma unroll
        for (int k = 0; k < 9; ++k) G[k] = -G[k];
    }

    double Rw[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) Rw[k] = nan;
    Vec3 tw = Vec3{nan, nan, nan}, nw = tw;
    double tnorm = nan;
    int winner = -1, v0 = 0, v1c = 0, v2c = 0, v3c = 0;

    if (model && rotation) {
        double Gm[3][3], Rr[3][3], rt[3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) Gm[r][c] = G[3 * r + c];
        bool okR = mm_polar3(Gm, Rr, rt);
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) okR = okR && isfinite(Rr[r][c]);
        if (okR) {
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) Rw[3 * r + c] = Rr[r][c];
            tw = Vec3{0.0, 0.0, 0.0};
            flags |= MM_HPOSE_ROTATION;
        } else {
            model = false;
        }
    } else if (model) {
        hp_solution(G, v1, v2, v3, a1, a3, den, Rp, tpl, npl);
        hp_solution(G, v1, v2, v3, a1, -a3, den, Rm, tmi, nmi);
        const double np_ = sqrt(dot3(tpl, tpl)), nm_ = sqrt(dot3(tmi, tmi));
        model = isfinite(np_) && isfinite(nm_) && np_ > 0.0 && nm_ > 0.0;
#pragma unroll
        for (int k = 0; k < 9; ++k) model = model && isfinite(Rp[k]) && isfinite(Rm[k]);
    }
    if (!model && !(flags & MM_POSE_TOO_FEW)) flags |= MM_POSE_NO_MODEL;
    const bool planar = model && !rotation;

    if (planar) {      // (uniform over the workgroup)
        const Vec3 tpn = Vec3{-tpl.x, -tpl.y, -tpl.z}, npn = Vec3{-npl.x, -npl.y, -npl.z};
        const Vec3 tmn = Vec3{-tmi.x, -tmi.y, -tmi.z}, nmn = Vec3{-nmi.x, -nmi.y, -nmi.z};
        for (int j = tid; j < mm; j += HG_THREADS) {
            Vec3 ra, rb;
            if (mm_pair_rays(a, p, j, ra, rb)) {
                double l1, l2;
                v0 += hp_depths(Rp, tpl, npl, ra, l1, l2) ? 1 : 0;
                v1c += hp_depths(Rp, tpn, npn, ra, l1, l2) ? 1 : 0;
                v2c += hp_depths(Rm, tmi, nmi, ra, l1, l2) ? 1 : 0;
                v3c += hp_depths(Rm, tmn, nmn, ra, l1, l2) ? 1 : 0;
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            v0 += __shfl_xor(v0, off, 64);
            v1c += __shfl_xor(v1c, off, 64);
            v2c += __shfl_xor(v2c, off, 64);
            v3c += __shfl_xor(v3c, off, 64);
        }
        if (lane == 0) {
            cnt[wave][0] = v0;
            cnt[wave][1] = v1c;
            cnt[wave][2] = v2c;
            cnt[wave][3] = v3c;
        }
        __syncthreads();
        v0 = hp_block_count(0, cnt);
        v1c = hp_block_count(1, cnt);
        v2c = hp_block_count(2, cnt);
        v3c = hp_block_count(3, cnt);

        int vmax = v0 > v1c ? v0 : v1c;
        vmax = vmax > v2c ? vmax : v2c;
        vmax = vmax > v3c ? vmax : v3c;
        const double bar = a.ambiguous_frac * (double)vmax;
        const bool c0 = (double)v0 >= bar, c1 = (double)v1c >= bar, c2 = (double)v2c >= bar, c3 = (double)v3c >= bar;
        const int n_cont = (c0 ? 1 : 0) + (c1 ? 1 : 0) + (c2 ? 1 : 0) + (c3 ? 1 : 0);
        bool hinted = false;
        Vec3 hv = Vec3{0.0, 0.0, 0.0};
        if (a.hint != nullptr) {
            hv = Vec3{a.hint[3 * (size_t)p], a.hint[3 * (size_t)p + 1], a.hint[3 * (size_t)p + 2]};
            hinted = isfinite(hv.x) && isfinite(hv.y) && isfinite(hv.z);
        }
        if (hinted) {      // the contender whose normal agrees best with the hint, ties to the lowest c
            const double dp = dot3(npl, hv), dm = dot3(nmi, hv);
            const double d0 = dp, d1 = -dp, d2 = dm, d3 = -dm;
            double best = 0.0;
            if (c0) {
                winner = 0;
                best = d0;
            }
            if (c1 && (winner < 0 || d1 > best)) {
                winner = 1;
                best = d1;
            }
            if (c2 && (winner < 0 || d2 > best)) {
                winner = 2;
                best = d2;
            }
            if (c3 && (winner < 0 || d3 > best)) {
                winner = 3;
                best = d3;
            }
        } else {           // the largest count, ties to the lowest c
            int wv = v0;
            winner = 0;
            if (v1c > wv) {
                wv = v1c;
                winner = 1;
            }
            if (v2c > wv) {
                wv = v2c;
                winner = 2;
            }
            if (v3c > wv) {
                wv = v3c;
                winner = 3;
            }
        }
        const int wv = winner == 0 ? v0 : (winner == 1 ? v1c : (winner == 2 ? v2c : v3c));
        if ((double)wv < a.min_front_frac * (double)mm || (n_cont > 1 && !hinted)) flags |= MM_POSE_AMBIGUOUS;
#pragma unroll
        for (int k = 0; k < 9; ++k) Rw[k] = winner < 2 ? Rp[k] : Rm[k];
        tw = winner == 0 ? tpl : (winner == 1 ? tpn : (winner == 2 ? tmi : tmn));
        nw = winner == 0 ? npl : (winner == 1 ? npn : (winner == 2 ? nmi : nmn));
        tnorm = sqrt(dot3(tw, tw));
    }

    // the winner's depths of the rows that voted for it, over |t|; NaN everywhere else, rows at or beyond m included
    for (int j = tid; j < a.cap; j += HG_THREADS) {
        double l1 = nan, l2 = nan;
        if (planar && j < mm) {
            Vec3 ra, rb;
            if (mm_pair_rays(a, p, j, ra, rb)) {
                double d1, d2;
                if (hp_depths(Rw, tw, nw, ra, d1, d2)) {
                    l1 = d1 / tnorm;
                    l2 = d2 / tnorm;
                }
            }
        }
        reinterpret_cast<double2 *>(a.depth)[(size_t)p * a.cap + j] = make_double2(l1, l2);
    }
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) a.R[9 * (size_t)p + k] = Rw[k];
        a.t[3 * (size_t)p] = planar ? tw.x / tnorm : tw.x;
        a.t[3 * (size_t)p + 1] = planar ? tw.y / tnorm : tw.y;
        a.t[3 * (size_t)p + 2] = planar ? tw.z / tnorm : tw.z;
        a.sigma[3 * (size_t)p] = sg1;
        a.sigma[3 * (size_t)p + 1] = sg2;
        a.sigma[3 * (size_t)p + 2] = sg3;
        a.normal[3 * (size_t)p] = nw.x;
        a.normal[3 * (size_t)p + 1] = nw.y;
        a.normal[3 * (size_t)p + 2] = nw.z;
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

}  // namespace

extern "C" size_t mm_homography_workspace_bytes(int n_pairs, int n_hyp) {
    return mm_pairs_workspace(n_pairs, n_hyp);
}

extern "C" int mm_verify_homography(mm_ctx *ctx, const float *kp_xy, const int32_t *pairs, const int32_t *m, int n_pairs, int cap,
                                    const mm_homography_params *prm, const int32_t *verify_info, int32_t *pairs_out, int32_t *m_out,
                                    double *Hm, double *cost, int32_t *info, void *ws, size_t ws_bytes) {
    // every argument is judged before the context is looked at: nothing below this block runs on a bad call
    if (!prm || n_pairs < 0) return mm_fail(ctx, MM_ERR_ARG, "mm_verify_homography: bad argument");
    if (prm->n_hyp < 1 || prm->n_hyp > 4096) return mm_fail(ctx, MM_ERR_ARG, "mm_verify_homography: n_hyp must be in 1 .. 4096");
    if (!(prm->threshold_px >= 0.0) || !(prm->collinear_tol >= 0.0))      // (negative or NaN; +inf keeps every well-formed match)
        return mm_fail(ctx, MM_ERR_ARG, "mm_verify_homography: threshold_px and collinear_tol must not be negative");
    if (!(prm->degenerate_frac >= 0.0 && prm->degenerate_frac <= 1.0))
        return mm_fail(ctx, MM_ERR_ARG, "mm_verify_homography: degenerate_frac must be in [0, 1]");
    if (prm->refit_iters < 0 || prm->refit_iters > 1000 || prm->min_inliers < 0)
        return mm_fail(ctx, MM_ERR_ARG, "mm_verify_homography: bad parameter");
    if (n_pairs > 0 && (!kp_xy || !pairs || !m || !pairs_out || !m_out || !Hm || !cost || !info || !ws || cap <= 0 || pairs == pairs_out))
        return mm_fail(ctx, MM_ERR_ARG, "mm_verify_homography: bad argument");
    if (n_pairs > 0 && ws_bytes < mm_homography_workspace_bytes(n_pairs, prm->n_hyp))
        return mm_fail(ctx, MM_ERR_WORKSPACE, "mm_verify_homography: workspace too small");
    if (!ctx) return MM_ERR_ARG;
    if (n_pairs == 0) return MM_OK;
    if (((uintptr_t)kp_xy | (uintptr_t)pairs | (uintptr_t)pairs_out) & 7)
        return mm_fail(ctx, MM_ERR_ARG, "mm_verify_homography: kp_xy, pairs and pairs_out must be 8-byte aligned");
    HgArgs a;
    a.kp_xy = kp_xy;
    a.pairs = pairs;
    a.m = m;
    a.verify_info = verify_info;
    a.n_pairs = n_pairs;
    a.cap = cap;
    a.n_hyp = prm->n_hyp;
    a.min_matches = prm->min_matches < 8 ? 8 : prm->min_matches;
    a.min_inliers = prm->min_inliers;
    a.refit_iters = prm->refit_iters;
    a.seed = prm->seed;
    a.pair_base = prm->pair_base;
    a.tau2 = prm->threshold_px * prm->threshold_px;
    a.collinear_tol = prm->collinear_tol;
    a.degenerate_frac = prm->degenerate_frac;
    mm_pairs_carve(a, ws);
    const dim3 per_hyp((unsigned)n_pairs, (unsigned)((a.n_hyp + 63) / 64));
    MM_LAUNCH(ctx, "hg_normalise_kernel", hg_normalise_kernel, dim3((unsigned)n_pairs), dim3(HG_THREADS), 0, a);
    MM_LAUNCH(ctx, "hg_hypothesis_kernel", hg_hypothesis_kernel, per_hyp, dim3(64), 0, a);
    MM_LAUNCH(ctx, "hg_score_kernel", hg_score_kernel, per_hyp, dim3(64), 0, a);
    MM_LAUNCH(ctx, "hg_finish_kernel", hg_finish_kernel, dim3((unsigned)n_pairs), dim3(HG_THREADS), 0, a, pairs_out, m_out, Hm, cost, info);
    return MM_OK;
}

extern "C" int mm_recover_poses_homography(mm_ctx *ctx, const double *K, const float *kp_xy, const int32_t *pairs, const int32_t *m,
                                           const double *Hm, const double *normal_hint, int n_pairs, int cap,
                                           const mm_hpose_params *prm, double *R, double *t, double *sigma, double *normal,
                                           double *depth, int32_t *info) {
    // every argument is judged before the context is looked at: nothing below this block runs on a bad call
    if (!prm || !K || n_pairs < 0 || cap <= 0) return mm_fail(ctx, MM_ERR_ARG, "mm_recover_poses_homography: bad argument");
    if (!(prm->min_front_frac >= 0.0 && prm->min_front_frac <= 1.0) || !(prm->ambiguous_frac >= 0.0 && prm->ambiguous_frac <= 1.0))
        return mm_fail(ctx, MM_ERR_ARG, "mm_recover_poses_homography: min_front_frac and ambiguous_frac must be in [0, 1]");
    if (!(prm->rotation_tol >= 0.0)) return mm_fail(ctx, MM_ERR_ARG, "mm_recover_poses_homography: rotation_tol must not be negative");
    bool k_ok = K[3] == 0.0 && K[6] == 0.0 && K[7] == 0.0 && K[8] == 1.0 && K[0] != 0.0 && K[4] != 0.0;
    for (int k = 0; k < 9; ++k) k_ok = k_ok && std::isfinite(K[k]);
    if (!k_ok)
        return mm_fail(ctx, MM_ERR_ARG,
                       "mm_recover_poses_homography: K must be finite and upper triangular with K[8] = 1 and non-zero focal lengths");
    if (n_pairs > 0 && (!kp_xy || !pairs || !m || !Hm || !R || !t || !sigma || !normal || !depth || !info))
        return mm_fail(ctx, MM_ERR_ARG, "mm_recover_poses_homography: bad argument");
    if (!ctx) return MM_ERR_ARG;
    if (n_pairs == 0) return MM_OK;
    if (((uintptr_t)kp_xy | (uintptr_t)pairs) & 7 || ((uintptr_t)depth & 15))
        return mm_fail(ctx, MM_ERR_ARG, "mm_recover_poses_homography: kp_xy and pairs must be 8-byte aligned, depth 16-byte aligned");
    HpArgs a;
    a.kp_xy = kp_xy;
    a.pairs = pairs;
    a.m = m;
    a.Hm = Hm;
    a.hint = normal_hint;
    a.n_pairs = n_pairs;
    a.cap = cap;
    a.min_matches = prm->min_matches < 8 ? 8 : prm->min_matches;
    a.min_front_frac = prm->min_front_frac;
    a.ambiguous_frac = prm->ambiguous_frac;
    a.rotation_tol = prm->rotation_tol;
    for (int k = 0; k < 9; ++k) a.K[k] = K[k];
    mm_k_inverse(K, a.Ki);
    a.R = R;
    a.t = t;
    a.sigma = sigma;
    a.normal = normal;
    a.depth = depth;
    a.info = info;
    MM_LAUNCH(ctx, "hp_pair_kernel", hp_pair_kernel, dim3((unsigned)n_pairs), dim3(HG_THREADS), 0, a);
    return MM_OK;
}
