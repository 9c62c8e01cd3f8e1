// Guided matching: the key points no match uses, matched again among the candidates each pair's model admits (gfx950).
//
// No reference counterpart: the reference links every Lowe-ratio survivor and never looks at a key point again.  The definition
// -- gate, seeds, search, the proposal rule, one-to-one, merge, flags -- is in include/meatmodeler.h (mm_guided_match); this
// file maps it:
//   gm_prepare_kernel  one workgroup per pair: the model and the order of the seeds judged, the used marks written, the unused
//                      queries and the unused trains listed in ascending order (ballot / popcount prefix), the result
//                      tables preset
//   gm_search_kernel   workgroup = (pair, 256 unused queries), lane = query: its descriptor in eight registers and the
//                      per-query part of the distance prepared once; the unused trains go through LDS in tiles of 256 with
//                      their per-train part and their descriptor.  Pass 1 over a tile has no branch: every lane reads the
//                      same address (broadcast) and puts every train to a NECESSARY test on the prepared terms (below) --
//                      four to seven f64 operations -- one bit of a 256-bit mask each.  Pass 2 walks the lane's own set bits
//                      (a band around the line, a disc around the transferred point: about one train per tile): the gate
//                      itself, which is mm_pairs.h's distance called as verify.hip and homography.hip call it, and for what
//                      passes it a xor / popcount.  Best and second are kept on a packed (distance << 22 | train) key; the
//                      reverse direction is an integer atomicMin of (distance << 22 | query) per train in the same pass:
//                      the gate is evaluated once per (query, train), so both directions see the same set
//   gm_finish_kernel   one workgroup per pair: the proposal rule, one-to-one (the reverse table, or an atomicMin per train over
//                      the proposals), the merge of seeds and new rows by query (ballot / popcount prefix), the -1 tail
// The necessary tests.  Built without FMA contraction (Makefile), so a term computed here has the bits the distance computes.
//   kind 0: e = x' fx0 + y' fx1 + fx2 is the distance's e; its denominator den sums the same four squares as nq + nt in another
//   order, each sum of non-negative terms within (1 + eps)^3 of the exact one.  An inlier has fl(e e) / den <= tau^2 up to one
//   rounding, hence fl(e e) <= tau^2 (nq + nt) (1 + 8 eps) in the normal range: "e e > tau^2 (1 + 1e-6) (nq + nt)" is false for it.
//   kind 1: the forward half fwd = (x' - y0/y2)^2 + (y' - y1/y2)^2 is the distance's own; an inlier has a finite, non-negative
//   backward half, so fl(fwd + bwd) >= fwd and fwd <= 2 tau^2 exactly: "fwd > 2 tau^2" is false for it.
// Either comparison is false on a NaN, which then reaches the gate and is judged there.
// Integer atomicMin is the only operation here whose order is not fixed, and its result does not depend on it.
#include "mm_pairs.h"

namespace {

constexpr int GM_THREADS = 256;      // every kernel: mm_block_compact_slot is written for this workgroup
constexpr int GM_TILE = 256;         // unused trains per LDS tile of the search
static_assert(GM_TILE == 256, "the search keeps one 64-bit mask per 64 trains of a tile in four register pairs");
static_assert(GM_THREADS == MM_BLOCK_THREADS, "the mm_block_* helpers are written for this workgroup");
constexpr uint32_t GM_NONE = 0xFFFFFFFFu;
constexpr int GM_SHIFT = 22;         // key = distance << 22 | index: cap <= 2^22, distance <= 256
constexpr uint32_t GM_INDEX = (1u << GM_SHIFT) - 1u;
constexpr int GM_PASS = MM_GUIDED_SKIPPED | MM_GUIDED_UNORDERED;

struct GmArgs {
    const float *kp_xy;
    const uint8_t *desc;
    const int32_t *n, *pairs, *m, *kind;
    const double *model;
    int n_pairs, cap, max_dist, cross_check;
    double tau2, tau2_slack, tau2_twice, ratio;      // tau^2, tau^2 (1 + 1e-6), 2 tau^2
    // workspace, [n_pairs, cap] each
    int32_t *seed_t;        // train of the kept seed whose query is i, or -1
    int32_t *q_list, *t_list;      // the unused queries / trains, ascending
    uint32_t *rev;          // per train: lowest (distance, query) key over the gate, GM_NONE: none
    uint32_t *prop;         // per train: lowest (distance, query) key over the proposals (cross_check 0)
    uint2 *fwd;             // per query: (best, second) key, GM_NONE: none
    uint8_t *used_q, *used_t;
    int32_t *cnt;           // [n_pairs, 4]: unused queries, unused trains, flags, -
};

__device__ __forceinline__ int gm_clamp(int v, int cap) { return v < 0 ? 0 : (v > cap ? cap : v); }

// ---- prepare ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GM_THREADS) void gm_prepare_kernel(GmArgs a) {
    __shared__ int wcount[MM_BLOCK_WAVES];
    const int p = blockIdx.x, tid = threadIdx.x;
    const size_t row = (size_t)p * a.cap;
    const int mm = mm_pair_count(a.m, a.cap, p);
    const int n_q = gm_clamp(a.n[p], a.cap), n_t = gm_clamp(a.n[p + 1], a.cap);
    const int kind = a.kind != nullptr ? a.kind[p] : 0;
    bool finite = true;
#pragma unroll
    for (int c = 0; c < 9; ++c) finite = finite && isfinite(a.model[9 * (size_t)p + c]);
    int flags = ((kind != 0 && kind != 1) || !finite) ? MM_GUIDED_SKIPPED : 0;
    int bad = 0, unordered = 0;
    for (int j = tid; j < mm; j += GM_THREADS) {
        const int2 qt = reinterpret_cast<const int2 *>(a.pairs)[row + j];
        if (!((unsigned)qt.x < (unsigned)a.cap && (unsigned)qt.y < (unsigned)a.cap)) bad = 1;
        if (j + 1 < mm && !(qt.x < a.pairs[2 * (row + j + 1)])) unordered = 1;
    }
    bad = __syncthreads_or(bad);
    unordered = __syncthreads_or(unordered);
    if (bad) flags |= MM_GUIDED_MALFORMED;
    if (unordered) flags |= MM_GUIDED_UNORDERED;
    const bool pass = (flags & GM_PASS) != 0;
    for (int i = tid; i < a.cap; i += GM_THREADS) {
        a.seed_t[row + i] = -1;
        a.rev[row + i] = GM_NONE;
        a.prop[row + i] = GM_NONE;
        a.fwd[row + i] = make_uint2(GM_NONE, GM_NONE);
        a.used_q[row + i] = 0;
        a.used_t[row + i] = 0;
    }
    __syncthreads();
    if (!pass) {
        for (int j = tid; j < mm; j += GM_THREADS) {
            const int2 qt = reinterpret_cast<const int2 *>(a.pairs)[row + j];
            if ((unsigned)qt.x < (unsigned)a.cap && (unsigned)qt.y < (unsigned)a.cap) {
                a.seed_t[row + qt.x] = qt.y;      // (queries strictly increase: one seed per query)
                a.used_q[row + qt.x] = 1;
                a.used_t[row + qt.y] = 1;
            }
        }
    }
    __syncthreads();
    int n_qu = 0, n_tu = 0;
    if (!pass) {      // (uniform over the workgroup)
        for (int i0 = 0; i0 < n_q; i0 += GM_THREADS) {
            const int i = i0 + tid;
            const bool keep = i < n_q && a.used_q[row + i] == 0;
            const int at = mm_block_compact_slot(keep, n_qu, wcount);
            if (keep) a.q_list[row + at] = i;
        }
        for (int j0 = 0; j0 < n_t; j0 += GM_THREADS) {
            const int j = j0 + tid;
            const bool keep = j < n_t && a.used_t[row + j] == 0;
            const int at = mm_block_compact_slot(keep, n_tu, wcount);
            if (keep) a.t_list[row + at] = j;
        }
    }
    if (tid == 0) {
        int32_t *c = a.cnt + 4 * (size_t)p;
        c[0] = n_qu;
        c[1] = n_tu;
        c[2] = flags;
        c[3] = 0;
    }
}

// ---- search -----------------------------------------------------------------------------------------------------------------
struct GmTrain {      // 32 bytes: two 16-byte LDS reads, the same address in every lane
    double xp, yp, nt;
    int j, pad;
};

// the per-query part of the necessary test and the gate of one kind
template <int KIND>
struct GmQuery;
template <>
struct GmQuery<0> {
    double F[9], x, y, fx0, fx1, fx2, nq;
    __device__ __forceinline__ GmQuery(const double (&v)[9], double x_, double y_) : x(x_), y(y_) {
#pragma unroll
        for (int c = 0; c < 9; ++c) F[c] = v[c];
        fx0 = F[0] * x + F[1] * y + F[2];
        fx1 = F[3] * x + F[4] * y + F[5];
        fx2 = F[6] * x + F[7] * y + F[8];
        nq = fx0 * fx0 + fx1 * fx1;
    }
    __device__ __forceinline__ static double train_term(const double (&v)[9], double xp, double yp) {
        const double ft0 = v[0] * xp + v[3] * yp + v[6], ft1 = v[1] * xp + v[4] * yp + v[7];
        return ft0 * ft0 + ft1 * ft1;
    }
    __device__ __forceinline__ bool may_pass(const GmTrain &t, const GmArgs &a) const {
        const double e = t.xp * fx0 + t.yp * fx1 + fx2;
        return !(e * e > a.tau2_slack * (nq + t.nt));
    }
    __device__ __forceinline__ double distance(double xp, double yp) const { return vfy_sampson(F, x, y, xp, yp); }
};
template <>
struct GmQuery<1> {
    double H[9], A[9], x, y, u, v;
    __device__ __forceinline__ GmQuery(const double (&h)[9], double x_, double y_) : x(x_), y(y_) {
#pragma unroll
        for (int c = 0; c < 9; ++c) H[c] = h[c];
        hg_adjugate(H, A);
        const double y0 = (H[0] * x + H[1] * y) + H[2], y1 = (H[3] * x + H[4] * y) + H[5], y2 = (H[6] * x + H[7] * y) + H[8];
        u = y0 / y2;
        v = y1 / y2;
    }
    __device__ __forceinline__ static double train_term(const double (&)[9], double, double) { return 0.0; }
    __device__ __forceinline__ bool may_pass(const GmTrain &t, const GmArgs &a) const {
        const double ex = t.xp - u, ey = t.yp - v;
        return !(ex * ex + ey * ey > a.tau2_twice);
    }
    __device__ __forceinline__ double distance(double xp, double yp) const { return hg_transfer(H, A, x, y, xp, yp); }
};

template <int KIND>
__device__ __forceinline__ void gm_search_body(const GmArgs &a, int p, int q0, int n_qu, int n_tu, GmTrain *tile, uint4 *tdesc) {
    const int tid = threadIdx.x;
    const size_t row = (size_t)p * a.cap;
    const bool live = q0 + tid < n_qu;
    const int i = live ? a.q_list[row + q0 + tid] : 0;
    double mv[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) mv[c] = a.model[9 * (size_t)p + c];
    const float2 xy = reinterpret_cast<const float2 *>(a.kp_xy)[row + i];
    const GmQuery<KIND> Q(mv, (double)xy.x, (double)xy.y);
    const uint4 *dq = reinterpret_cast<const uint4 *>(a.desc) + 2 * (row + i);
    const uint4 qa = dq[0], qb = dq[1];
    const float2 *txy = reinterpret_cast<const float2 *>(a.kp_xy) + (size_t)(p + 1) * a.cap;
    const uint4 *tds = reinterpret_cast<const uint4 *>(a.desc) + 2 * (size_t)(p + 1) * a.cap;
    uint32_t k0 = GM_NONE, k1 = GM_NONE;
    for (int t0 = 0; t0 < n_tu; t0 += GM_TILE) {
        const int nt = min(GM_TILE, n_tu - t0);
        __syncthreads();
        if (tid < nt) {
            const int j = a.t_list[row + t0 + tid];
            const float2 v = txy[j];
            GmTrain t;
            t.xp = (double)v.x;
            t.yp = (double)v.y;
            t.nt = GmQuery<KIND>::train_term(mv, t.xp, t.yp);
            t.j = j;
            t.pad = 0;
            tile[tid] = t;
            tdesc[2 * tid] = tds[2 * (size_t)j];
            tdesc[2 * tid + 1] = tds[2 * (size_t)j + 1];
        }
        __syncthreads();
        // pass 1, no branch: the necessary test of every train of the tile, one bit each (entries at or beyond nt hold stale
        // words; their bits are cleared below)
        uint64_t mask[GM_TILE / 64];
#pragma unroll
        for (int c = 0; c < GM_TILE / 64; ++c) {
            uint64_t mk = 0;
            if (c * 64 < nt) {      // (uniform)
#pragma unroll 4
                for (int b = 0; b < 64; ++b) mk |= (uint64_t)(Q.may_pass(tile[c * 64 + b], a) ? 1 : 0) << b;
                const int valid = nt - c * 64;
                if (valid < 64) mk &= (1ull << valid) - 1ull;
            }
            mask[c] = live ? mk : 0ull;
        }
        // pass 2: the lane's own survivors -- a handful per tile, so the wave runs this body for the longest list among its
        // lanes instead of once per train that any lane lets through.  The key carries the train: the order does not matter.
        for (;;) {
            int k;
            if (mask[0]) {
                k = __builtin_ctzll(mask[0]);
                mask[0] &= mask[0] - 1;
            } else if (mask[1]) {
                k = 64 + __builtin_ctzll(mask[1]);
                mask[1] &= mask[1] - 1;
            } else if (mask[2]) {
                k = 128 + __builtin_ctzll(mask[2]);
                mask[2] &= mask[2] - 1;
            } else if (mask[3]) {
                k = 192 + __builtin_ctzll(mask[3]);
                mask[3] &= mask[3] - 1;
            } else {
                break;
            }
            const GmTrain t = tile[k];
            if (mm_pair_inlier(Q.distance(t.xp, t.yp), a.tau2)) {
                const uint4 ta = tdesc[2 * k], tb = tdesc[2 * k + 1];
                const uint32_t d = __popc(qa.x ^ ta.x) + __popc(qa.y ^ ta.y) + __popc(qa.z ^ ta.z) + __popc(qa.w ^ ta.w) +
                                   __popc(qb.x ^ tb.x) + __popc(qb.y ^ tb.y) + __popc(qb.z ^ tb.z) + __popc(qb.w ^ tb.w);
                const uint32_t key = (d << GM_SHIFT) | (uint32_t)t.j;
                if (key < k0) {
                    k1 = k0;
                    k0 = key;
                } else if (key < k1) {
                    k1 = key;
                }
                atomicMin(a.rev + row + t.j, (d << GM_SHIFT) | (uint32_t)i);
            }
        }
    }
    if (live) a.fwd[row + i] = make_uint2(k0, k1);
}

__global__ __launch_bounds__(GM_THREADS) void gm_search_kernel(GmArgs a, int tiles_per_pair) {
    __shared__ GmTrain tile[GM_TILE];
    __shared__ uint4 tdesc[2 * GM_TILE];
    const int p = blockIdx.x / tiles_per_pair, q0 = (blockIdx.x % tiles_per_pair) * GM_THREADS;
    const int32_t *c = a.cnt + 4 * (size_t)p;
    const int n_qu = c[0], n_tu = c[1];
    if (q0 >= n_qu || n_tu == 0) return;      // (uniform over the workgroup; a pair that passes through has no list)
    const int kind = a.kind != nullptr ? a.kind[p] : 0;
    if (kind == 0)
        gm_search_body<0>(a, p, q0, n_qu, n_tu, tile, tdesc);
    else
        gm_search_body<1>(a, p, q0, n_qu, n_tu, tile, tdesc);
}

// ---- finish -----------------------------------------------------------------------------------------------------------------
// the proposal of query i, if it makes one: its nearest gated train and the distance
__device__ __forceinline__ bool gm_proposal(const GmArgs &a, size_t row, int i, int n_q, int &j0, int &d0) {
    if (i >= n_q) return false;
    const uint2 f = a.fwd[row + i];
    if (f.x == GM_NONE) return false;
    d0 = (int)(f.x >> GM_SHIFT);
    j0 = (int)(f.x & GM_INDEX);
    if (d0 > a.max_dist) return false;
    return f.y == GM_NONE || (double)d0 < a.ratio * (double)(int)(f.y >> GM_SHIFT);
}

__global__ __launch_bounds__(GM_THREADS) void gm_finish_kernel(GmArgs a, int32_t *__restrict__ pairs_out, int32_t *__restrict__ m_out,
                                                               uint8_t *__restrict__ is_new, int32_t *__restrict__ info) {
    __shared__ int wcount[MM_BLOCK_WAVES];
    __shared__ int n_prop, n_new;
    const int p = blockIdx.x, tid = threadIdx.x;
    const size_t row = (size_t)p * a.cap;
    const int mm = mm_pair_count(a.m, a.cap, p);
    const int n_q = gm_clamp(a.n[p], a.cap);
    const int flags = a.cnt[4 * (size_t)p + 2];
    int2 *out = reinterpret_cast<int2 *>(pairs_out) + row;
    if ((flags & GM_PASS) != 0) {      // (uniform) the input rows as they are
        for (int j = tid; j < a.cap; j += GM_THREADS) {
            out[j] = j < mm ? reinterpret_cast<const int2 *>(a.pairs)[row + j] : make_int2(-1, -1);
            is_new[row + j] = 0;
        }
        if (tid == 0) {
            m_out[p] = mm;
            info[4 * (size_t)p] = flags;
            info[4 * (size_t)p + 1] = mm;
            info[4 * (size_t)p + 2] = 0;
            info[4 * (size_t)p + 3] = 0;
        }
        return;
    }
    if (tid == 0) n_prop = n_new = 0;
    __syncthreads();
    {
        int mine = 0;
        for (int i = tid; i < n_q; i += GM_THREADS) {
            int j0, d0;
            if (gm_proposal(a, row, i, n_q, j0, d0)) {
                ++mine;
                if (a.cross_check == 0) atomicMin(a.prop + row + j0, ((uint32_t)d0 << GM_SHIFT) | (uint32_t)i);
            }
        }
        if (mine) atomicAdd(&n_prop, mine);
    }
    __syncthreads();      // (the reads of prop below are atomic loads: they are served where the atomicMin ran)
    int total = 0;
    for (int i0 = 0; i0 < a.cap; i0 += GM_THREADS) {
        const int i = i0 + tid;
        bool seed = false, fresh = false;
        int t = -1;
        if (i < a.cap) {
            const int st = a.seed_t[row + i];
            int j0, d0;
            if (st >= 0) {
                seed = true;
                t = st;
            } else if (gm_proposal(a, row, i, n_q, j0, d0)) {
                const uint32_t w = a.cross_check != 0 ? a.rev[row + j0]
                                                      : __hip_atomic_load(a.prop + row + j0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if ((int)(w & GM_INDEX) == i && w != GM_NONE) {
                    fresh = true;
                    t = j0;
                }
            }
        }
        const int at = mm_block_compact_slot(seed || fresh, total, wcount);
        if (seed || fresh) {
            out[at] = make_int2(i, t);
            is_new[row + at] = fresh ? 1 : 0;
        }
        if (fresh) atomicAdd(&n_new, 1);
    }
    for (int j = total + tid; j < a.cap; j += GM_THREADS) {
        out[j] = make_int2(-1, -1);
        is_new[row + j] = 0;
    }
    __syncthreads();
    if (tid == 0) {
        m_out[p] = total;
        info[4 * (size_t)p] = flags;
        info[4 * (size_t)p + 1] = total - n_new;
        info[4 * (size_t)p + 2] = n_new;
        info[4 * (size_t)p + 3] = n_prop;
    }
}

// ---- host: the workspace ----------------------------------------------------------------------------------------------------
inline size_t gm_region(size_t rows, size_t bytes) { return mm_align_up(rows * bytes, 256); }

}  // namespace

extern "C" size_t mm_guided_workspace_bytes(int n_pairs, int cap) {
    const size_t rows = (n_pairs > 0 && cap > 0) ? (size_t)n_pairs * (size_t)cap : 0;
    const size_t np = n_pairs > 0 ? (size_t)n_pairs : 0;
    // seed_t, q_list, t_list, rev, prop (4 bytes each), fwd (8), used_q, used_t (1 each), cnt [n_pairs, 4]; never 0
    return 5 * gm_region(rows, 4) + gm_region(rows, 8) + 2 * gm_region(rows, 1) + gm_region(np, 16) + 256;
}

extern "C" int mm_guided_match(mm_ctx *ctx, const float *kp_xy, const uint8_t *desc, const int32_t *n, const int32_t *pairs,
                               const int32_t *m, const double *model, const int32_t *kind, int n_pairs, int cap,
                               const mm_guided_params *prm, int32_t *pairs_out, int32_t *m_out, uint8_t *is_new, int32_t *info,
                               void *ws, size_t ws_bytes) {
    // every argument is judged before the context is looked at: nothing below this block runs on a bad call
    if (!prm || n_pairs < 0) return mm_fail(ctx, MM_ERR_ARG, "mm_guided_match: bad argument");
    if (!(prm->threshold_px >= 0.0))      // (negative or NaN; +inf admits every finite distance)
        return mm_fail(ctx, MM_ERR_ARG, "mm_guided_match: threshold_px must not be negative");
    if (!(prm->ratio >= 0.0)) return mm_fail(ctx, MM_ERR_ARG, "mm_guided_match: ratio must not be negative");
    if (prm->max_dist < 0 || prm->max_dist > 256) return mm_fail(ctx, MM_ERR_ARG, "mm_guided_match: max_dist must be in 0 .. 256");
    if (prm->cross_check != 0 && prm->cross_check != 1) return mm_fail(ctx, MM_ERR_ARG, "mm_guided_match: cross_check must be 0 or 1");
    if (n_pairs > 0 && (!kp_xy || !desc || !n || !pairs || !m || !model || !pairs_out || !m_out || !is_new || !info || !ws || cap <= 0 ||
                        cap > (1 << GM_SHIFT) || pairs == pairs_out))
        return mm_fail(ctx, MM_ERR_ARG, "mm_guided_match: bad argument");
    if (n_pairs > 0 && ws_bytes < mm_guided_workspace_bytes(n_pairs, cap))
        return mm_fail(ctx, MM_ERR_WORKSPACE, "mm_guided_match: workspace too small");
    if (!ctx) return MM_ERR_ARG;
    if (n_pairs == 0) return MM_OK;
    if ((((uintptr_t)kp_xy | (uintptr_t)pairs | (uintptr_t)pairs_out) & 7) || ((uintptr_t)desc & 15) || ((uintptr_t)ws & 15))
        return mm_fail(ctx, MM_ERR_ARG, "mm_guided_match: kp_xy, pairs and pairs_out must be 8-byte aligned, desc and ws 16-byte aligned");
    const int tiles = (cap + GM_THREADS - 1) / GM_THREADS;
    if ((long long)n_pairs * tiles > 0x7FFFFFFFll) return mm_fail(ctx, MM_ERR_ARG, "mm_guided_match: too many pairs for one call");
    GmArgs a;
    a.kp_xy = kp_xy;
    a.desc = desc;
    a.n = n;
    a.pairs = pairs;
    a.m = m;
    a.kind = kind;
    a.model = model;
    a.n_pairs = n_pairs;
    a.cap = cap;
    a.max_dist = prm->max_dist;
    a.cross_check = prm->cross_check;
    a.tau2 = prm->threshold_px * prm->threshold_px;
    a.tau2_slack = a.tau2 * (1.0 + 1e-6);
    a.tau2_twice = 2.0 * a.tau2;
    a.ratio = prm->ratio;
    const size_t rows = (size_t)n_pairs * (size_t)cap;
    char *w = (char *)ws;
    a.seed_t = (int32_t *)w;
    w += gm_region(rows, 4);
    a.q_list = (int32_t *)w;
    w += gm_region(rows, 4);
    a.t_list = (int32_t *)w;
    w += gm_region(rows, 4);
    a.rev = (uint32_t *)w;
    w += gm_region(rows, 4);
    a.prop = (uint32_t *)w;
    w += gm_region(rows, 4);
    a.fwd = (uint2 *)w;
    w += gm_region(rows, 8);
    a.used_q = (uint8_t *)w;
    w += gm_region(rows, 1);
    a.used_t = (uint8_t *)w;
    w += gm_region(rows, 1);
    a.cnt = (int32_t *)w;
    MM_LAUNCH(ctx, "gm_prepare_kernel", gm_prepare_kernel, dim3((unsigned)n_pairs), dim3(GM_THREADS), 0, a);
    MM_LAUNCH(ctx, "gm_search_kernel", gm_search_kernel, dim3((unsigned)(n_pairs * tiles)), dim3(GM_THREADS), 0, a, tiles);
    MM_LAUNCH(ctx, "gm_finish_kernel", gm_finish_kernel, dim3((unsigned)n_pairs), dim3(GM_THREADS), 0, a, pairs_out, m_out, is_new, info);
    return MM_OK;
}
