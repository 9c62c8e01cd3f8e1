// Similarity registration: a robust 7-DoF alignment (s, R, d), dst ~ s R src + d, per problem of a call, and the two
// maps that put a reconstruction into the frame it gives (gfx950, f64).
//
// No reference counterpart: the reference is metric through its chessboard and never registers one frame to another.  The
// definition -- the fit through the 3 x 3 cyclic Jacobi of M^T M, the three-pick sampling, the MSAC score, the chunked order
// of every sum, the refit rounds, flags and outputs -- is in include/meatmodeler.h (mm_align_similarity,
// mm_apply_similarity, mm_camera_centres); this file maps it:
//   al_hypothesis_kernel  lane = hypothesis: three picks, the fit in registers (every index static)
//   al_score_kernel       grid (chunk, n_hyp / 64): the chunk's rows staged through LDS 256 at a time, every lane reads the
//                         same address (a broadcast), one partial cost per (chunk, hypothesis)
//   al_select_kernel      one workgroup per problem: the partial costs summed over the chunks ascending, the argmin
//   al_centroid_kernel, al_moment_kernel   per chunk, over the inliers of the current model: the sums of the centroids, then
//                         the nine sums of M and var about them
//   al_solve_kernel       per problem: the moments summed over the chunks ascending, the fit
//   al_cost_kernel, al_accept_kernel       per chunk the MSAC cost of the candidate; per problem the sum and the decision
//   al_finish_kernel, al_mask_kernel       the outputs of a problem; the inlier rows of a chunk
// A chunk is MM_ALIGN_CHUNK = 4096 rows of one problem: every sum is a workgroup's fixed order inside a chunk and the chunk
// index ascending across chunks, so the bits depend on the problem alone.  Built without FMA contraction (Makefile): the
// inlier test is evaluated by five kernels and must give one answer, and the NumPy restatement follows the header operation
// by operation.  No float atomics; the only atomic is an integer OR that raises a flag bit.
#include "mm_common.h"
#include "mm_geom.h"
#include <cmath>

namespace {

constexpr int AL_THREADS = MM_BLOCK_THREADS;
constexpr int AL_CHUNK = MM_ALIGN_CHUNK;      // rows per chunk: a constant of the definition
constexpr int AL_TILE = 256;        // rows of the score kernel's LDS tile
constexpr int AL_STATE = 40;        // doubles of a problem's state
constexpr int AL_CSUM = 20;         // doubles of a chunk's row of sums
// a problem's state: the current model, its cost and inlier count, the candidate of a round and the select kernel's verdict
constexpr int ST_SIM = 0, ST_COST = 13, ST_NIN = 14, ST_MODEL = 15, ST_CAND = 16, ST_CAND_OK = 29, ST_BEST_H = 30, ST_NVALID = 31,
              ST_FLAGS = 32, ST_CEN = 33;      // ST_CEN: cs (3), cd (3), count of the round's inliers

struct AlProb {
    int64_t lo;          // first row
    int32_t n, chunk0;   // rows; index of the problem's first chunk
};

struct AlArgs {
    const double *src, *dst;
    const AlProb *prob;          // [n_prob]
    const int32_t *chunk_prob;   // [n_chunks]
    int n_prob, n_chunks, n_hyp, min_points, min_inliers, with_scale;
    uint32_t seed, prob_base;
    double tau2, tol2;
    double *hyp;        // [n_prob, n_hyp, 13]
    double *partial;    // [n_chunks, n_hyp]
    double *cost_h;     // [n_prob, n_hyp]
    double *state;      // [n_prob, AL_STATE]
    double *csum;       // [n_chunks, AL_CSUM]: pass 1 of a refit in slots 0 .. 6, pass 2 in 7 .. 16; the cost pass in 0 .. 1
    double *sim, *cost;
    uint8_t *inlier;
    int32_t *info;
};

// The fit from the moments about the centroids cs, cd: M = sum b a^T (row-major), var = sum a . a.  sim = (s, R, d); false:
// invalid (every entry is still written).
__device__ __forceinline__ bool al_fit(const double (&M)[9], double var, const double (&cs)[3], const double (&cd)[3], int with_scale,
                                       double tol2, double (&sim)[13]) {
    double G[3][3], V[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) G[r][c] = (M[r] * M[c] + M[3 + r] * M[3 + c]) + M[6 + r] * M[6 + c];
    mm_identity<3>(V);
    mm_jacobi<3>(G, V);
    // v1: largest eigenvalue, v2: the larger of the other two; ties to the lowest column (selected without a runtime index)
    const double l0 = G[0][0], l1 = G[1][1], l2 = G[2][2];
    const int i1 = (l1 > l0) ? ((l2 > l1) ? 2 : 1) : ((l2 > l0) ? 2 : 0);
    const int ia = i1 == 0 ? 1 : 0, ib = i1 == 2 ? 1 : 2;      // the other two, ascending
    const double la = ia == 0 ? l0 : l1, lb = ib == 1 ? l1 : l2;
    const int i2 = (lb > la) ? ib : ia;
    const double lam1 = i1 == 0 ? l0 : (i1 == 1 ? l1 : l2), lam2 = (lb > la) ? lb : la;
    Vec3 v1, v2;
    v1 = i1 == 0 ? Vec3{V[0][0], V[1][0], V[2][0]} : (i1 == 1 ? Vec3{V[0][1], V[1][1], V[2][1]} : Vec3{V[0][2], V[1][2], V[2][2]});
    v2 = i2 == 0 ? Vec3{V[0][0], V[1][0], V[2][0]} : (i2 == 1 ? Vec3{V[0][1], V[1][1], V[2][1]} : Vec3{V[0][2], V[1][2], V[2][2]});
    const Vec3 v3 = cross3(v1, v2);
    bool ok = isfinite(lam1) && lam1 > 0.0 && isfinite(lam2) && !(lam2 <= tol2 * lam1) && isfinite(var) && var > 0.0;
    const Vec3 e1 = mat3(M, v1), e2 = mat3(M, v2);
    const double n1 = sqrt(dot3(e1, e1));
    const Vec3 u1 = Vec3{e1.x / n1, e1.y / n1, e1.z / n1};
    const double d12 = dot3(u1, e2);
    const Vec3 w2 = Vec3{e2.x - d12 * u1.x, e2.y - d12 * u1.y, e2.z - d12 * u1.z};
    const double n2 = sqrt(dot3(w2, w2));
    const Vec3 u2 = Vec3{w2.x / n2, w2.y / n2, w2.z / n2};
    const Vec3 u3 = cross3(u1, u2);
    double R[9];
    R[0] = (u1.x * v1.x + u2.x * v2.x) + u3.x * v3.x;
    R[1] = (u1.x * v1.y + u2.x * v2.y) + u3.x * v3.y;
    R[2] = (u1.x * v1.z + u2.x * v2.z) + u3.x * v3.z;
    R[3] = (u1.y * v1.x + u2.y * v2.x) + u3.y * v3.x;
    R[4] = (u1.y * v1.y + u2.y * v2.y) + u3.y * v3.y;
    R[5] = (u1.y * v1.z + u2.y * v2.z) + u3.y * v3.z;
    R[6] = (u1.z * v1.x + u2.z * v2.x) + u3.z * v3.x;
    R[7] = (u1.z * v1.y + u2.z * v2.y) + u3.z * v3.y;
    R[8] = (u1.z * v1.z + u2.z * v2.z) + u3.z * v3.z;
    double tr = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) tr += R[k] * M[k];
    const double s = with_scale ? tr / var : 1.0;
    sim[0] = s;
#pragma unroll
    for (int k = 0; k < 9; ++k) sim[1 + k] = R[k];
#pragma unroll
    for (int r = 0; r < 3; ++r) sim[10 + r] = cd[r] - s * ((R[3 * r] * cs[0] + R[3 * r + 1] * cs[1]) + R[3 * r + 2] * cs[2]);
#pragma unroll
    for (int k = 0; k < 13; ++k) ok = ok && isfinite(sim[k]);
    return ok;
}

// A = s R and d of a model: what the distance is evaluated with
struct AlMap {
    double A[9], d[3];
};
__device__ __forceinline__ AlMap al_map(const double *sim) {
    AlMap m;
    const double s = sim[0];
#pragma unroll
    for (int k = 0; k < 9; ++k) m.A[k] = s * sim[1 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) m.d[k] = sim[10 + k];
    return m;
}
// e^2 of one row; true: an inlier (e^2 finite and <= tau^2)
__device__ __forceinline__ bool al_distance(const AlMap &m, double sx, double sy, double sz, double dx, double dy, double dz, double tau2,
                                            double &e2) {
    const double ex = dx - (((m.A[0] * sx + m.A[1] * sy) + m.A[2] * sz) + m.d[0]);
    const double ey = dy - (((m.A[3] * sx + m.A[4] * sy) + m.A[5] * sz) + m.d[1]);
    const double ez = dz - (((m.A[6] * sx + m.A[7] * sy) + m.A[8] * sz) + m.d[2]);
    e2 = (ex * ex + ey * ey) + ez * ez;
    return isfinite(e2) && e2 <= tau2;
}

// the rows [r0, r0 + nr) of chunk g, all of problem q
__device__ __forceinline__ void al_chunk(const AlArgs &a, int g, int &q, int64_t &r0, int &nr) {
    q = a.chunk_prob[g];
    const AlProb pr = a.prob[q];
    const int k = g - pr.chunk0;
    r0 = pr.lo + (int64_t)k * AL_CHUNK;
    nr = min(AL_CHUNK, pr.n - k * AL_CHUNK);
}

// ---- one similarity per hypothesis -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void al_hypothesis_kernel(AlArgs a) {
    const int q = blockIdx.x;
    const int h = blockIdx.y * 64 + threadIdx.x;
    const AlProb pr = a.prob[q];
    if (pr.n < a.min_points || h >= a.n_hyp) return;
    const uint32_t base = mm_pcg(mm_pcg(a.seed + mm_pcg(a.prob_base + (uint32_t)q)) + (uint32_t)h);
    int pick[3];
    bool ok = mm_sample_distinct<3>(base, pr.n, pick);
    // the rows enter the fit in ascending order: two hypotheses over the same three rows are the same bits and tie exactly
    if (pick[0] > pick[1]) { const int t = pick[0]; pick[0] = pick[1]; pick[1] = t; }
    if (pick[1] > pick[2]) { const int t = pick[1]; pick[1] = pick[2]; pick[2] = t; }
    if (pick[0] > pick[1]) { const int t = pick[0]; pick[0] = pick[1]; pick[1] = t; }
    double S[3][3], D[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double *ps = a.src + 3 * (pr.lo + pick[k]), *pd = a.dst + 3 * (pr.lo + pick[k]);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            S[k][c] = ps[c];
            D[k][c] = pd[c];
            ok = ok && isfinite(S[k][c]) && isfinite(D[k][c]);
        }
    }
    double cs[3], cd[3], M[9], var = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        cs[c] = ((S[0][c] + S[1][c]) + S[2][c]) / 3.0;
        cd[c] = ((D[0][c] + D[1][c]) + D[2][c]) / 3.0;
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) M[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double ax = S[k][0] - cs[0], ay = S[k][1] - cs[1], az = S[k][2] - cs[2];
        const double b[3] = {D[k][0] - cd[0], D[k][1] - cd[1], D[k][2] - cd[2]};
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            M[3 * r] += b[r] * ax;
            M[3 * r + 1] += b[r] * ay;
            M[3 * r + 2] += b[r] * az;
        }
        var += (ax * ax + ay * ay) + az * az;
    }
    double sim[13];
    ok = al_fit(M, var, cs, cd, a.with_scale, a.tol2, sim) && ok;
    double *o = a.hyp + ((size_t)q * a.n_hyp + h) * 13;
    const double nan = __builtin_nan("");
#pragma unroll
    for (int k = 0; k < 13; ++k) o[k] = ok ? sim[k] : nan;
}

// ---- MSAC cost of every hypothesis over one chunk ------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void al_score_kernel(AlArgs a) {
    __shared__ double tile[AL_TILE * 6];
    int q, nr;
    int64_t r0;
    al_chunk(a, blockIdx.x, q, r0, nr);
    if (a.prob[q].n < a.min_points) return;      // (uniform over the workgroup)
    const int h = blockIdx.y * 64 + threadIdx.x;
    const bool live = h < a.n_hyp;
    const AlMap m = al_map(a.hyp + ((size_t)q * a.n_hyp + (live ? h : 0)) * 13);
    double cost = 0.0;
    for (int j0 = 0; j0 < nr; j0 += AL_TILE) {
        const int nt = min(AL_TILE, nr - j0);
        __syncthreads();
        for (int j = threadIdx.x; j < 3 * nt; j += 64) {      // (3 nt doubles of each side, contiguous)
            const int row = j / 3, c = j - 3 * row;
            tile[6 * row + c] = a.src[3 * (r0 + j0) + j];
            tile[6 * row + 3 + c] = a.dst[3 * (r0 + j0) + j];
        }
        __syncthreads();
        for (int j = 0; j < nt; ++j) {
            double e2;
            const bool in = al_distance(m, tile[6 * j], tile[6 * j + 1], tile[6 * j + 2], tile[6 * j + 3], tile[6 * j + 4], tile[6 * j + 5],
                                        a.tau2, e2);
            cost += in ? e2 : a.tau2;
        }
    }
    if (live) a.partial[(size_t)blockIdx.x * a.n_hyp + h] = cost;
}

// ---- winner of a problem ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AL_THREADS) void al_select_kernel(AlArgs a) {
    __shared__ double sm[MM_BLOCK_WAVES];
    __shared__ double bc[MM_BLOCK_WAVES];
    __shared__ int bh[MM_BLOCK_WAVES];
    const int q = blockIdx.x, tid = threadIdx.x;
    const AlProb pr = a.prob[q];
    double *st = a.state + (size_t)q * AL_STATE;
    const double nan = __builtin_nan("");
    int flags = 0, best_h = -1, n_valid = 0;
    if (pr.n < a.min_points) {
        flags = MM_ALIGN_TOO_FEW;
    } else {
        const int nch = (pr.n + AL_CHUNK - 1) / AL_CHUNK;
        const double *hy = a.hyp + (size_t)q * a.n_hyp * 13;
        double *ch = a.cost_h + (size_t)q * a.n_hyp;
        for (int h = tid; h < a.n_hyp; h += AL_THREADS) {      // (the argmin below reads cost[h] with the same stride)
            double c = 0.0;
            for (int k = 0; k < nch; ++k) c += a.partial[(size_t)(pr.chunk0 + k) * a.n_hyp + h];
            ch[h] = isfinite(hy[(size_t)h * 13]) ? c : __builtin_huge_val();
        }
        double c_best;
        int h_best;
        mm_block_argmin_finite(ch, a.n_hyp, hy, 13, bc, bh, sm, c_best, h_best, n_valid);
        if (h_best != INT32_MAX) best_h = h_best;
        else flags = MM_ALIGN_NO_MODEL;
    }
    if (tid < 13) {
        const double v = best_h >= 0 ? a.hyp[((size_t)q * a.n_hyp + best_h) * 13 + tid] : nan;
        st[ST_SIM + tid] = v;
        st[ST_CAND + tid] = v;      // the winner is the candidate of the first cost pass
    }
    if (tid == 0) {
        st[ST_COST] = nan;
        st[ST_NIN] = 0.0;
        st[ST_MODEL] = best_h >= 0 ? 1.0 : 0.0;
        st[ST_CAND_OK] = best_h >= 0 ? 1.0 : 0.0;
        st[ST_BEST_H] = (double)best_h;
        st[ST_NVALID] = (double)n_valid;
        st[ST_FLAGS] = (double)flags;
    }
}

// ---- refit, pass 1: a chunk's sums of the inliers' coordinates ---------------------------------------------------------------
__global__ __launch_bounds__(AL_THREADS) void al_centroid_kernel(AlArgs a) {
    __shared__ double sm[MM_BLOCK_WAVES * 7];
    int q, nr;
    int64_t r0;
    al_chunk(a, blockIdx.x, q, r0, nr);
    const double *st = a.state + (size_t)q * AL_STATE;
    if (st[ST_MODEL] == 0.0) return;      // (uniform)
    const AlMap m = al_map(st + ST_SIM);
    double v[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int j = threadIdx.x; j < nr; j += AL_THREADS) {
        const double *ps = a.src + 3 * (r0 + j), *pd = a.dst + 3 * (r0 + j);
        const double sx = ps[0], sy = ps[1], sz = ps[2], dx = pd[0], dy = pd[1], dz = pd[2];
        double e2;
        if (al_distance(m, sx, sy, sz, dx, dy, dz, a.tau2, e2)) {
            v[0] += sx;
            v[1] += sy;
            v[2] += sz;
            v[3] += dx;
            v[4] += dy;
            v[5] += dz;
            v[6] += 1.0;
        }
    }
    mm_block_sum<7>(v, sm);
    if (threadIdx.x < 7) a.csum[(size_t)blockIdx.x * AL_CSUM + threadIdx.x] = v[threadIdx.x];
}

// the centroids of the round from the chunks' sums, chunk index ascending: every workgroup of the problem forms the same bits
__device__ __forceinline__ void al_centroids(const AlArgs &a, const AlProb &pr, double *cen /*LDS [7]*/) {
    const int nch = (pr.n + AL_CHUNK - 1) / AL_CHUNK;
    if (threadIdx.x < 7) {
        double s = 0.0;
        for (int k = 0; k < nch; ++k) s += a.csum[(size_t)(pr.chunk0 + k) * AL_CSUM + threadIdx.x];
        cen[threadIdx.x] = s;
    }
    __syncthreads();
}

// ---- refit, pass 2: a chunk's centred sums (M row-major, var) ------------------------------------------------------------------
__global__ __launch_bounds__(AL_THREADS) void al_moment_kernel(AlArgs a) {
    __shared__ double sm[MM_BLOCK_WAVES * 10];
    __shared__ double cen[7];
    int q, nr;
    int64_t r0;
    al_chunk(a, blockIdx.x, q, r0, nr);
    double *st = a.state + (size_t)q * AL_STATE;
    if (st[ST_MODEL] == 0.0) return;      // (uniform)
    const AlProb pr = a.prob[q];
    al_centroids(a, pr, cen);
    const double cnt = cen[6];
    const double cs0 = cen[0] / cnt, cs1 = cen[1] / cnt, cs2 = cen[2] / cnt, cd0 = cen[3] / cnt, cd1 = cen[4] / cnt, cd2 = cen[5] / cnt;
    const AlMap m = al_map(st + ST_SIM);
    double v[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) v[k] = 0.0;
    for (int j = threadIdx.x; j < nr; j += AL_THREADS) {
        const double *ps = a.src + 3 * (r0 + j), *pd = a.dst + 3 * (r0 + j);
        const double sx = ps[0], sy = ps[1], sz = ps[2], dx = pd[0], dy = pd[1], dz = pd[2];
        double e2;
        if (al_distance(m, sx, sy, sz, dx, dy, dz, a.tau2, e2)) {
            const double ax = sx - cs0, ay = sy - cs1, az = sz - cs2;
            const double b[3] = {dx - cd0, dy - cd1, dz - cd2};
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                v[3 * r] += b[r] * ax;
                v[3 * r + 1] += b[r] * ay;
                v[3 * r + 2] += b[r] * az;
            }
            v[9] += (ax * ax + ay * ay) + az * az;
        }
    }
    mm_block_sum<10>(v, sm);
    // (slots 0 .. 6 hold pass 1, which other workgroups of the problem may still be reading: pass 2 has slots 7 .. 16)
    if (threadIdx.x < 10) a.csum[(size_t)blockIdx.x * AL_CSUM + 7 + threadIdx.x] = v[threadIdx.x];
    if (blockIdx.x == pr.chunk0 && threadIdx.x == 0) {
        st[ST_CEN] = cs0;
        st[ST_CEN + 1] = cs1;
        st[ST_CEN + 2] = cs2;
        st[ST_CEN + 3] = cd0;
        st[ST_CEN + 4] = cd1;
        st[ST_CEN + 5] = cd2;
        st[ST_CEN + 6] = cnt;
    }
}

// ---- refit: the candidate of the round ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void al_solve_kernel(AlArgs a) {
    const int q = blockIdx.x;
    double *st = a.state + (size_t)q * AL_STATE;
    if (threadIdx.x != 0) return;
    st[ST_CAND_OK] = 0.0;
    if (st[ST_MODEL] == 0.0 || st[ST_NIN] < 3.0) return;      // fewer than 3 inliers: the round changes nothing
    const AlProb pr = a.prob[q];
    const int nch = (pr.n + AL_CHUNK - 1) / AL_CHUNK;
    double M[9], var = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) M[k] = 0.0;
    for (int c = 0; c < nch; ++c) {
        const double *o = a.csum + (size_t)(pr.chunk0 + c) * AL_CSUM + 7;
#pragma unroll
        for (int k = 0; k < 9; ++k) M[k] += o[k];
        var += o[9];
    }
    const double cs[3] = {st[ST_CEN], st[ST_CEN + 1], st[ST_CEN + 2]}, cd[3] = {st[ST_CEN + 3], st[ST_CEN + 4], st[ST_CEN + 5]};
    double sim[13];
    const bool ok = al_fit(M, var, cs, cd, a.with_scale, a.tol2, sim);
#pragma unroll
    for (int k = 0; k < 13; ++k) st[ST_CAND + k] = sim[k];
    st[ST_CAND_OK] = ok ? 1.0 : 0.0;
}

// ---- MSAC cost of the candidate over one chunk: (cost, inliers) ---------------------------------------------
__global__ __launch_bounds__(AL_THREADS) void al_cost_kernel(AlArgs a) {
    __shared__ double sm[MM_BLOCK_WAVES * 2];
    int q, nr;
    int64_t r0;
    al_chunk(a, blockIdx.x, q, r0, nr);
    const double *st = a.state + (size_t)q * AL_STATE;
    if (st[ST_CAND_OK] == 0.0) return;      // (uniform)
    const AlMap m = al_map(st + ST_CAND);
    double v[2] = {0.0, 0.0};
    for (int j = threadIdx.x; j < nr; j += AL_THREADS) {
        const double *ps = a.src + 3 * (r0 + j), *pd = a.dst + 3 * (r0 + j);
        double e2;
        const bool in = al_distance(m, ps[0], ps[1], ps[2], pd[0], pd[1], pd[2], a.tau2, e2);
        v[0] += in ? e2 : a.tau2;
        v[1] += in ? 1.0 : 0.0;
    }
    mm_block_sum<2>(v, sm);
    if (threadIdx.x < 2) a.csum[(size_t)blockIdx.x * AL_CSUM + threadIdx.x] = v[threadIdx.x];
}

// first: the winner's own cost (taken as it is); else a refit's, accepted only when valid, finite and strictly lower
__global__ __launch_bounds__(64) void al_accept_kernel(AlArgs a, int first) {
    const int q = blockIdx.x;
    double *st = a.state + (size_t)q * AL_STATE;
    if (threadIdx.x != 0 || st[ST_CAND_OK] == 0.0) return;
    const AlProb pr = a.prob[q];
    const int nch = (pr.n + AL_CHUNK - 1) / AL_CHUNK;
    double cost = 0.0, n_in = 0.0;
    for (int c = 0; c < nch; ++c) {
        cost += a.csum[(size_t)(pr.chunk0 + c) * AL_CSUM];
        n_in += a.csum[(size_t)(pr.chunk0 + c) * AL_CSUM + 1];
    }
    if (first || (isfinite(cost) && cost < st[ST_COST])) {
#pragma unroll
        for (int k = 0; k < 13; ++k) st[ST_SIM + k] = st[ST_CAND + k];
        st[ST_COST] = cost;
        st[ST_NIN] = n_in;
    }
}

// ---- outputs ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void al_finish_kernel(AlArgs a) {
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q >= a.n_prob) return;
    const double *st = a.state + (size_t)q * AL_STATE;
    const bool model = st[ST_MODEL] != 0.0;
    const double nan = __builtin_nan("");
#pragma unroll
    for (int k = 0; k < 13; ++k) a.sim[13 * (size_t)q + k] = model ? st[ST_SIM + k] : nan;
    a.cost[q] = model ? st[ST_COST] : nan;
    int flags = (int)st[ST_FLAGS];
    const int n_in = model ? (int)st[ST_NIN] : 0;
    if (model && n_in < a.min_inliers) flags |= MM_ALIGN_WEAK;
    int32_t *o = a.info + 4 * (size_t)q;
    o[0] = flags;
    o[1] = n_in;
    o[2] = (int)st[ST_BEST_H];
    o[3] = (int)st[ST_NVALID];
}

// the inlier rows of the final model (0 without one), and MM_ALIGN_NONFINITE where a chunk holds a non-finite row
__global__ __launch_bounds__(AL_THREADS) void al_mask_kernel(AlArgs a) {
    int q, nr;
    int64_t r0;
    al_chunk(a, blockIdx.x, q, r0, nr);
    const double *st = a.state + (size_t)q * AL_STATE;
    const bool model = st[ST_MODEL] != 0.0;
    const AlMap m = al_map(st + ST_SIM);
    bool bad = false;
    for (int j = threadIdx.x; j < nr; j += AL_THREADS) {
        const double *ps = a.src + 3 * (r0 + j), *pd = a.dst + 3 * (r0 + j);
        const double sx = ps[0], sy = ps[1], sz = ps[2], dx = pd[0], dy = pd[1], dz = pd[2];
        bad = bad || !(isfinite(sx) && isfinite(sy) && isfinite(sz) && isfinite(dx) && isfinite(dy) && isfinite(dz));
        double e2;
        const bool in = al_distance(m, sx, sy, sz, dx, dy, dz, a.tau2, e2);
        a.inlier[r0 + j] = (model && in) ? 1 : 0;
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(a.info + 4 * (size_t)q, MM_ALIGN_NONFINITE);
}

// ---- the two maps --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AL_THREADS) void al_apply_kernel(const double *sim, double *pts, int64_t P, double *ext, int64_t F) {
    const int64_t i = (int64_t)blockIdx.x * AL_THREADS + threadIdx.x;
    if (i >= P + F) return;
    double sm[13];
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 13; ++k) {
        sm[k] = sim[k];
        fin = fin && isfinite(sm[k]);
    }
    if (!fin) return;
    const double s = sm[0];
    const double *R = sm + 1, *d = sm + 10;
    if (i < P) {
        double *x = pts + 3 * i;
        const double X = x[0], Y = x[1], Z = x[2];
#pragma unroll
        for (int r = 0; r < 3; ++r) x[r] = (((s * R[3 * r]) * X + (s * R[3 * r + 1]) * Y) + (s * R[3 * r + 2]) * Z) + d[r];
    } else {
        double *e = ext + 12 * (i - P);
        double E[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) E[k] = e[k];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            double N[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) N[c] = (E[4 * r] * R[3 * c] + E[4 * r + 1] * R[3 * c + 1]) + E[4 * r + 2] * R[3 * c + 2];
            e[4 * r] = N[0];
            e[4 * r + 1] = N[1];
            e[4 * r + 2] = N[2];
            e[4 * r + 3] = s * E[4 * r + 3] - ((N[0] * d[0] + N[1] * d[1]) + N[2] * d[2]);
        }
    }
}

__global__ __launch_bounds__(AL_THREADS) void al_centres_kernel(const double *ext, int64_t F, double *C) {
    const int64_t i = (int64_t)blockIdx.x * AL_THREADS + threadIdx.x;
    if (i >= F) return;
    const double *e = ext + 12 * i;
#pragma unroll
    for (int c = 0; c < 3; ++c) C[3 * i + c] = -((e[c] * e[3] + e[4 + c] * e[7]) + e[8 + c] * e[11]);
}

size_t al_region(size_t bytes) { return mm_align_up(bytes, 256); }

// chunks a call can have at most: every problem's last chunk may be partial
size_t al_max_chunks(size_t n_prob, size_t N) { return N / AL_CHUNK + n_prob; }

}  // namespace

extern "C" size_t mm_align_workspace_bytes(int n_prob, int n_hyp, int64_t N) {
    const size_t np = n_prob > 0 ? (size_t)n_prob : 0, nh = n_hyp > 0 ? (size_t)n_hyp : 0, nr = N > 0 ? (size_t)N : 0;
    const size_t nc = al_max_chunks(np, nr);
    return al_region(np * sizeof(AlProb)) + al_region(nc * sizeof(int32_t)) + al_region(np * nh * 13 * sizeof(double)) +
           al_region(nc * nh * sizeof(double)) + al_region(np * nh * sizeof(double)) + al_region(np * AL_STATE * sizeof(double)) +
           al_region(nc * AL_CSUM * sizeof(double));
}

extern "C" int mm_align_similarity(mm_ctx *ctx, const double *src, const double *dst, const int64_t *ptr, int n_prob,
                                   const mm_align_params *prm, double *sim, double *cost, uint8_t *inlier, int32_t *info, void *ws,
                                   size_t ws_bytes) {
    // every argument is judged before the context is looked at: nothing below this block runs on a bad call
    if (!prm || !ptr || n_prob < 0) return mm_fail(ctx, MM_ERR_ARG, "mm_align_similarity: bad argument");
    if (prm->n_hyp < 1 || prm->n_hyp > 4096) return mm_fail(ctx, MM_ERR_ARG, "mm_align_similarity: n_hyp must be in 1 .. 4096");
    if (!(prm->tau > 0.0) || !std::isfinite(prm->tau)) return mm_fail(ctx, MM_ERR_ARG, "mm_align_similarity: tau must be finite and positive");
    if (!(prm->collinear_tol >= 0.0) || !std::isfinite(prm->collinear_tol) || prm->refit_iters < 0 || prm->refit_iters > 1000 ||
        prm->min_inliers < 0 || (prm->with_scale != 0 && prm->with_scale != 1))
        return mm_fail(ctx, MM_ERR_ARG, "mm_align_similarity: bad parameter");
    if (ptr[0] < 0) return mm_fail(ctx, MM_ERR_ARG, "mm_align_similarity: ptr must not be negative");
    for (int q = 0; q < n_prob; ++q)
        if (ptr[q + 1] < ptr[q] || ptr[q + 1] - ptr[q] > INT32_MAX) return mm_fail(ctx, MM_ERR_ARG, "mm_align_similarity: ptr must not decrease");
    const int64_t N = ptr[n_prob];
    if (n_prob > 0 && (!sim || !cost || !info || !ws)) return mm_fail(ctx, MM_ERR_ARG, "mm_align_similarity: bad argument");
    if (n_prob > 0 && N > 0 && (!src || !dst || !inlier)) return mm_fail(ctx, MM_ERR_ARG, "mm_align_similarity: bad argument");
    if (n_prob > 0 && ws_bytes < mm_align_workspace_bytes(n_prob, prm->n_hyp, N))
        return mm_fail(ctx, MM_ERR_WORKSPACE, "mm_align_similarity: workspace too small");
    if (!ctx) return MM_ERR_ARG;
    if (n_prob == 0) return MM_OK;
    if (((uintptr_t)ws) & 7) return mm_fail(ctx, MM_ERR_ARG, "mm_align_similarity: the workspace must be 8-byte aligned");

    // the problems and their chunks, from the host's ptr: the grids are sized without a device read
    std::vector<AlProb> prob((size_t)n_prob);
    std::vector<int32_t> chunk_prob;
    for (int q = 0; q < n_prob; ++q) {
        const int n = (int)(ptr[q + 1] - ptr[q]);
        prob[q] = AlProb{ptr[q], n, (int32_t)chunk_prob.size()};
        for (int k = 0; k < (n + AL_CHUNK - 1) / AL_CHUNK; ++k) chunk_prob.push_back(q);
    }
    const size_t nc_max = al_max_chunks((size_t)n_prob, (size_t)N), nh = (size_t)prm->n_hyp;
    AlArgs a;
    a.src = src;
    a.dst = dst;
    a.n_prob = n_prob;
    a.n_chunks = (int)chunk_prob.size();
    a.n_hyp = prm->n_hyp;
    a.min_points = prm->min_points < 3 ? 3 : prm->min_points;
    a.min_inliers = prm->min_inliers;
    a.with_scale = prm->with_scale;
    a.seed = prm->seed;
    a.prob_base = prm->prob_base;
    a.tau2 = prm->tau * prm->tau;
    a.tol2 = prm->collinear_tol * prm->collinear_tol;
    char *w = (char *)ws;
    AlProb *d_prob = (AlProb *)w;
    w += al_region((size_t)n_prob * sizeof(AlProb));
    int32_t *d_chunk = (int32_t *)w;
    w += al_region(nc_max * sizeof(int32_t));
    a.hyp = (double *)w;
    w += al_region((size_t)n_prob * nh * 13 * sizeof(double));
    a.partial = (double *)w;
    w += al_region(nc_max * nh * sizeof(double));
    a.cost_h = (double *)w;
    w += al_region((size_t)n_prob * nh * sizeof(double));
    a.state = (double *)w;
    w += al_region((size_t)n_prob * AL_STATE * sizeof(double));
    a.csum = (double *)w;
    a.prob = d_prob;
    a.chunk_prob = d_chunk;
    a.sim = sim;
    a.cost = cost;
    a.inlier = inlier;
    a.info = info;
    // (pageable sources: the copies have left the vectors when the calls return)
    MM_HIP(ctx, hipMemcpyAsync(d_prob, prob.data(), prob.size() * sizeof(AlProb), hipMemcpyHostToDevice, ctx->stream));
    if (a.n_chunks > 0)
        MM_HIP(ctx, hipMemcpyAsync(d_chunk, chunk_prob.data(), chunk_prob.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));

    const unsigned hb = (unsigned)((a.n_hyp + 63) / 64), nch = (unsigned)a.n_chunks, np = (unsigned)n_prob;
    MM_LAUNCH(ctx, "al_hypothesis_kernel", al_hypothesis_kernel, dim3(np, hb), dim3(64), 0, a);
    if (nch) MM_LAUNCH(ctx, "al_score_kernel", al_score_kernel, dim3(nch, hb), dim3(64), 0, a);
    MM_LAUNCH(ctx, "al_select_kernel", al_select_kernel, dim3(np), dim3(AL_THREADS), 0, a);
    for (int it = 0; it <= prm->refit_iters; ++it) {      // round 0: the winner's own cost
        if (it > 0) {
            if (nch) MM_LAUNCH(ctx, "al_centroid_kernel", al_centroid_kernel, dim3(nch), dim3(AL_THREADS), 0, a);
            if (nch) MM_LAUNCH(ctx, "al_moment_kernel", al_moment_kernel, dim3(nch), dim3(AL_THREADS), 0, a);
            MM_LAUNCH(ctx, "al_solve_kernel", al_solve_kernel, dim3(np), dim3(64), 0, a);
        }
        if (nch) MM_LAUNCH(ctx, "al_cost_kernel", al_cost_kernel, dim3(nch), dim3(AL_THREADS), 0, a);
        MM_LAUNCH(ctx, "al_accept_kernel", al_accept_kernel, dim3(np), dim3(64), 0, a, it == 0 ? 1 : 0);
    }
    MM_LAUNCH(ctx, "al_finish_kernel", al_finish_kernel, dim3((np + 63) / 64), dim3(64), 0, a);
    if (nch) MM_LAUNCH(ctx, "al_mask_kernel", al_mask_kernel, dim3(nch), dim3(AL_THREADS), 0, a);
    return MM_OK;
}

extern "C" int mm_apply_similarity(mm_ctx *ctx, const double *sim, double *pts, int64_t P, double *ext, int64_t F) {
    if (!sim || P < 0 || F < 0) return mm_fail(ctx, MM_ERR_ARG, "mm_apply_similarity: bad argument");
    if (!ctx) return MM_ERR_ARG;
    const int64_t np = pts ? P : 0, nf = ext ? F : 0;
    if (np + nf == 0) return MM_OK;
    const int64_t nb = (np + nf + AL_THREADS - 1) / AL_THREADS;
    if (nb > INT32_MAX) return mm_fail(ctx, MM_ERR_ARG, "mm_apply_similarity: too many rows");
    MM_LAUNCH(ctx, "al_apply_kernel", al_apply_kernel, dim3((unsigned)nb), dim3(AL_THREADS), 0, sim, pts, np, ext, nf);
    return MM_OK;
}

extern "C" int mm_camera_centres(mm_ctx *ctx, const double *ext, int64_t F, double *C) {
    if (F < 0 || (F > 0 && (!ext || !C))) return mm_fail(ctx, MM_ERR_ARG, "mm_camera_centres: bad argument");
    if (!ctx) return MM_ERR_ARG;
    if (F == 0) return MM_OK;
    const int64_t nb = (F + AL_THREADS - 1) / AL_THREADS;
    if (nb > INT32_MAX) return mm_fail(ctx, MM_ERR_ARG, "mm_camera_centres: too many rows");
    MM_LAUNCH(ctx, "al_centres_kernel", al_centres_kernel, dim3((unsigned)nb), dim3(AL_THREADS), 0, ext, F, C);
    return MM_OK;
}
