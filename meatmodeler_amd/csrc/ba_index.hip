// Index structures of a bundle-adjustment problem in two native calls (mm_ba_index_build, stage 0 and stage 1).
//
// The CSR by point, the CSR by camera (stable order), the camera span, and -- for banded problems -- the co-observation
// pair list in segment order with its segment and chunk tables:
//   * pairs in ascending key camera(o) * (span + 1) + camera(o) - camera(o2); inside a key in emission order (o ascending,
//     then the point's observations in pt_obs order) -- what a stable sort of the emitted keys gives;
//   * cam_obs = the stable order of the observations by camera.
// Cameras F .. F + F_fixed - 1 are fixed: their observations are in the CSR by point, but not in the CSR by camera (they
// sort behind the free ones; head[6] says where) and in no pair.
// Point-major observations (pi non-decreasing, as flatten_tracks emits them) make pt_obs the identity and pt_ptr the
// places where pi changes.  Stage 0 assumes them and reports in its head whether they are (and whether every index is in
// range); for other input the caller runs it again with sort_by_point set, which sorts (pi, identity) stably first.
//
// The two sorts are rocPRIM's radix sort (stable) over the bits that can be set only: the camera index (9 bits at 500
// cameras instead of 32) and the pair key (16 bits at the bench shape: 500 cameras x span 87).  The pair sort carries
// (o, o2) as one 64-bit value, so there is no permutation to gather through afterwards.  Segments are the runs of the
// sorted keys (rocPRIM run-length encode), their first pairs and first chunks two exclusive scans over the segment table.
//
// Host read-backs: the head after stage 0 (span, number of pairs, validity) sizes the pair arrays; the head after stage 1
// gives the number of segments and chunks, whose arrays are allocated at their upper bounds (mm_ba_index_bounds).
#include <cstring>
#include "mm_common.h"
#include <rocprim/rocprim.hpp>

namespace {

constexpr int HEAD_SPAN = 0, HEAD_PAIRS = 1, HEAD_BAD_RANGE = 2, HEAD_NOT_POINT_MAJOR = 3, HEAD_SEG = 4, HEAD_CHUNKS = 5, HEAD_FREE = 6;

__device__ __forceinline__ bool idx_ok(const int64_t *head) { return head[HEAD_BAD_RANGE] == 0 && head[HEAD_NOT_POINT_MAJOR] == 0; }

// validity of the input; nothing else runs on input that fails here (every later kernel looks at the head first).
// F_all counts the fixed cameras in.  identity (sort by point): receives 0 .. O - 1, and the order is not judged.
__global__ __launch_bounds__(256) void idx_validate_kernel(const int32_t *__restrict__ fi, const int32_t *__restrict__ pi,
                                                           int64_t O, int F_all, int P, int32_t *__restrict__ identity,
                                                           int64_t *__restrict__ head) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool bad = false, unsorted = false;
    if (o < O) {
        const int f = fi[o], p = pi[o];
        bad = f < 0 || f >= F_all || p < 0 || p >= P;
        unsorted = !identity && o > 0 && pi[o - 1] > p;
        if (identity) identity[o] = (int32_t)o;
    }
    if (__ballot(bad) != 0 && (threadIdx.x & 63) == 0) head[HEAD_BAD_RANGE] = 1;      // (any writer writes the same value)
    if (__ballot(unsorted) != 0 && (threadIdx.x & 63) == 0) head[HEAD_NOT_POINT_MAJOR] = 1;
}

// ptr [nbins + 1] of a CSR whose keys [n] are sorted: entry i opens the bins (keys[i - 1], keys[i]], the last one closes
// the rest.  Keys >= nbins (fixed cameras) open no bin past ptr[nbins], which is then the number of keys < nbins.
// identity (optional) receives 0 .. n - 1.
__global__ __launch_bounds__(256) void idx_ptr_kernel(const int32_t *__restrict__ keys, int64_t n, int nbins,
                                                      int32_t *__restrict__ ptr, int32_t *__restrict__ identity,
                                                      const int64_t *__restrict__ head) {
    if (!idx_ok(head)) return;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int k = keys[i];
    const int lo = i == 0 ? 0 : keys[i - 1] + 1;
    for (int b = lo; b <= min(k, nbins); ++b) ptr[b] = (int32_t)i;
    if (i == n - 1)
        for (int b = k + 1; b <= nbins; ++b) ptr[b] = (int32_t)n;
    if (identity) identity[i] = (int32_t)i;
}

// cnt[o] = number of observations o2 of the same point with camera(o2) <= camera(o); span = max camera distance.
// The observations of point p are pt_obs[pt_ptr[p] .. pt_ptr[p + 1]]; IDENT: pt_obs is the identity and is not read.
// An observation of a fixed camera (f >= F) has no pairs and no span; as o2 it drops out by d < 0.
template <bool IDENT>
__global__ __launch_bounds__(256) void idx_count_kernel(const int32_t *__restrict__ fi, const int32_t *__restrict__ pi,
                                                        const int32_t *__restrict__ pt_ptr, const int32_t *__restrict__ pt_obs,
                                                        int64_t O, int F, int32_t *__restrict__ cnt,
                                                        int32_t *__restrict__ span_out, const int64_t *__restrict__ head) {
    if (!idx_ok(head)) return;
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int dmax = 0;
    if (o < O) {
        const int f = fi[o], p = pi[o];
        int c = 0;
        if (f < F)
            for (int e = pt_ptr[p]; e < pt_ptr[p + 1]; ++e) {
                const int d = f - fi[IDENT ? e : pt_obs[e]];
                c += d >= 0;
                dmax = max(dmax, d);
            }
        cnt[o] = c;
    }
    for (int off = 32; off > 0; off >>= 1) dmax = max(dmax, __shfl_down(dmax, off, 64));
    if ((threadIdx.x & 63) == 0 && dmax > __hip_atomic_load(span_out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(span_out, dmax);
}

__global__ void idx_head0_kernel(const int32_t *__restrict__ cnt, const int64_t *__restrict__ offs, int64_t O,
                                 const int32_t *__restrict__ span, const int32_t *__restrict__ cam_ptr, int F,
                                 int64_t *__restrict__ head) {
    if (!idx_ok(head)) return;
    head[HEAD_SPAN] = *span;
    head[HEAD_PAIRS] = offs[O - 1] + cnt[O - 1];
    head[HEAD_FREE] = cam_ptr[F];
}

// the pairs of observation o at offs[o] ..: key = camera(o) * (span + 1) + camera(o) - camera(o2), value = o2 << 32 | o
// (IDENT and fixed cameras as in idx_count_kernel)
template <bool IDENT>
__global__ __launch_bounds__(256) void idx_emit_kernel(const int32_t *__restrict__ fi, const int32_t *__restrict__ pi,
                                                       const int32_t *__restrict__ pt_ptr, const int32_t *__restrict__ pt_obs,
                                                       int64_t O, int F, const int64_t *__restrict__ offs, int span,
                                                       int64_t n_pairs, int32_t *__restrict__ key, uint64_t *__restrict__ val,
                                                       const int64_t *__restrict__ head) {
    if (!idx_ok(head)) return;
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= O) return;
    const int f = fi[o], p = pi[o];
    if (f >= F) return;
    int64_t w = offs[o];
    for (int e = pt_ptr[p]; e < pt_ptr[p + 1]; ++e) {
        const int o2 = IDENT ? e : pt_obs[e];
        const int d = f - fi[o2];
        if (d < 0) continue;
        if (w >= n_pairs) return;      // (cannot happen with the n_pairs stage 0 reported; keeps a wrong one inside the arrays)
        key[w] = f * (span + 1) + min(d, span);      // (min: a span smaller than the truth cannot make a key past F (span + 1))
        val[w] = ((uint64_t)(uint32_t)o2 << 32) | (uint32_t)o;
        ++w;
    }
}

__global__ __launch_bounds__(256) void idx_unpack_kernel(const uint64_t *__restrict__ val, const int32_t *__restrict__ pi,
                                                         int64_t n_pairs, int64_t O, int32_t *__restrict__ pair_o,
                                                         int32_t *__restrict__ pair_o2, int32_t *__restrict__ pair_p) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pairs) return;
    const uint64_t v = val[i];
    const uint32_t o = (uint32_t)v, o2 = (uint32_t)(v >> 32);
    pair_o[i] = (int32_t)o;
    pair_o2[i] = (int32_t)o2;
    pair_p[i] = pi[min((int64_t)o, O - 1)];
}

// counts of the runs past the last one read as 0, so that scans over the whole (upper bound) table are scans over the runs
__global__ __launch_bounds__(256) void idx_segcount_kernel(const int32_t *__restrict__ counts, const int32_t *__restrict__ n_seg,
                                                           int64_t seg_cap, int chunk, int32_t *__restrict__ pairs_of,
                                                           int32_t *__restrict__ chunks_of) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s > seg_cap) return;
    const int c = s < *n_seg ? counts[s] : 0;
    pairs_of[s] = c;
    chunks_of[s] = (c + chunk - 1) / chunk;
}

// one wave per segment writes the segment's chunks; wave 0 also closes the head
__global__ __launch_bounds__(256) void idx_chunks_kernel(const int32_t *__restrict__ n_seg_dev, const int32_t *__restrict__ seg_lo,
                                                         const int32_t *__restrict__ pairs_of,
                                                         const int32_t *__restrict__ seg_chunk_ptr, int chunk, int64_t chunk_cap,
                                                         int32_t *__restrict__ chunk_seg, int32_t *__restrict__ chunk_begin,
                                                         int32_t *__restrict__ chunk_end, int64_t *__restrict__ head) {
    const int64_t s = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    const int n_seg = *n_seg_dev;
    if (s == 0 && lane == 0) {
        head[HEAD_SEG] = n_seg;
        head[HEAD_CHUNKS] = seg_chunk_ptr[n_seg];
    }
    if (s >= n_seg) return;
    const int lo = seg_lo[s], hi = lo + pairs_of[s];
    const int64_t c0 = seg_chunk_ptr[s], c1 = seg_chunk_ptr[s + 1];
    for (int64_t c = c0 + lane; c < c1 && c < chunk_cap; c += 64) {
        const int b = lo + chunk * (int)(c - c0);
        chunk_seg[c] = (int32_t)s;
        chunk_begin[c] = b;
        chunk_end[c] = min(b + chunk, hi);
    }
}

int bits_for(int64_t n_values) {      // bits that can be set in 0 .. n_values - 1 (at least one)
    int b = 1;
    while (b < 63 && ((int64_t)1 << b) < n_values) ++b;
    return b;
}

// workspace of one stage: a walk over its regions; tmp sizes come from rocPRIM (they need the device)
struct Carve {
    size_t at = 0;
    size_t take(size_t bytes) {
        const size_t o = at;
        at += mm_align_up(bytes ? bytes : 1, 256);
        return o;
    }
};
struct Ws0 {
    size_t keys, cnt, offs, span, tmp, tmp_bytes, total;
};
struct Ws1 {
    size_t key, val, key_s, val_s, counts, n_seg, pairs_of, chunks_of, seg_lo, tmp, tmp_bytes, total;
};

// keys holds the sorted point indices (sort by point) until pt_ptr is made of them, then the sorted camera indices; cnt
// holds the identity the two sorts carry (sort by point) until the count kernel writes it
hipError_t ws0_layout(const mm_ba_index *ix, hipStream_t st, Ws0 &w) {
    const int64_t O = ix->O;
    size_t t_sort = 0, t_sort_p = 0, t_scan = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, t_sort, (const int32_t *)nullptr, (int32_t *)nullptr, (const int32_t *)nullptr,
                                             (int32_t *)nullptr, (size_t)O, 0u, (unsigned)bits_for((int64_t)ix->F + ix->F_fixed), st);
    if (e != hipSuccess) return e;
    if (ix->sort_by_point) {
        e = rocprim::radix_sort_pairs(nullptr, t_sort_p, (const int32_t *)nullptr, (int32_t *)nullptr, (const int32_t *)nullptr,
                                      (int32_t *)nullptr, (size_t)O, 0u, (unsigned)bits_for(ix->P), st);
        if (e != hipSuccess) return e;
        if (t_sort_p > t_sort) t_sort = t_sort_p;
    }
    e = rocprim::exclusive_scan(nullptr, t_scan, (const int32_t *)nullptr, (int64_t *)nullptr, (int64_t)0, (size_t)O,
                                rocprim::plus<int64_t>(), st);
    if (e != hipSuccess) return e;
    Carve c;
    w.keys = c.take((size_t)O * 4);
    w.cnt = c.take((size_t)O * 4);
    w.offs = c.take((size_t)O * 8);
    w.span = c.take(4);
    w.tmp_bytes = t_sort > t_scan ? t_sort : t_scan;
    w.tmp = c.take(w.tmp_bytes);
    w.total = c.at;
    return hipSuccess;
}

hipError_t ws1_layout(int64_t n_pairs, int64_t seg_cap, int key_bits, hipStream_t st, Ws1 &w) {
    size_t t_sort = 0, t_rle = 0, t_scan = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, t_sort, (const int32_t *)nullptr, (int32_t *)nullptr, (const uint64_t *)nullptr,
                                             (uint64_t *)nullptr, (size_t)n_pairs, 0u, (unsigned)key_bits, st);
    if (e != hipSuccess) return e;
    e = rocprim::run_length_encode(nullptr, t_rle, (const int32_t *)nullptr, (size_t)n_pairs, (int32_t *)nullptr, (int32_t *)nullptr,
                                   (int32_t *)nullptr, st);
    if (e != hipSuccess) return e;
    e = rocprim::exclusive_scan(nullptr, t_scan, (const int32_t *)nullptr, (int32_t *)nullptr, (int32_t)0, (size_t)seg_cap + 1,
                                rocprim::plus<int32_t>(), st);
    if (e != hipSuccess) return e;
    Carve c;
    w.key = c.take((size_t)n_pairs * 4);
    w.val = c.take((size_t)n_pairs * 8);
    w.key_s = c.take((size_t)n_pairs * 4);
    w.val_s = c.take((size_t)n_pairs * 8);
    w.counts = c.take((size_t)seg_cap * 4);
    w.n_seg = c.take(4);
    w.pairs_of = c.take((size_t)(seg_cap + 1) * 4);
    w.chunks_of = c.take((size_t)(seg_cap + 1) * 4);
    w.seg_lo = c.take((size_t)(seg_cap + 1) * 4);
    w.tmp_bytes = t_sort > t_rle ? t_sort : t_rle;
    if (t_scan > w.tmp_bytes) w.tmp_bytes = t_scan;
    w.tmp = c.take(w.tmp_bytes);
    w.total = c.at;
    return hipSuccess;
}

bool index_args_ok(const mm_ba_index *ix) {
    return ix && ix->F >= 0 && ix->F_fixed >= 0 && (int64_t)ix->F + ix->F_fixed > 0 && (int64_t)ix->F + ix->F_fixed < 0x7fffffffLL &&
           ix->P > 0 && ix->O > 0 && ix->O < 0x7fffffffLL && ix->fi && ix->pi && ix->head;
}
bool band_ok(const mm_ba_index *ix) {      // the condition under which ops.BADevice builds a pair list
    return ix->cam_span >= 0 && ix->cam_span < ix->F && (int64_t)ix->F * (ix->cam_span + 1) < 0x80000000LL && ix->n_pairs > 0 &&
           ix->n_pairs < 0x7fffffffLL && ix->chunk >= 64 && ix->chunk % 64 == 0;
}

}  // namespace

extern "C" {

int mm_ba_index_bounds(int F, int cam_span, int64_t n_pairs, int chunk, int64_t *seg_cap, int64_t *chunk_cap) {
    if (F <= 0 || cam_span < 0 || n_pairs < 0 || chunk <= 0 || !seg_cap || !chunk_cap) return MM_ERR_ARG;
    const int64_t keys = (int64_t)F * ((int64_t)cam_span + 1);
    *seg_cap = n_pairs < keys ? n_pairs : keys;          // a segment per key that occurs
    *chunk_cap = *seg_cap + n_pairs / chunk;             // sum of ceil(c_i / chunk) <= n_seg + floor(sum c_i / chunk)
    return MM_OK;
}

size_t mm_ba_index_workspace_bytes(mm_ctx *ctx, const mm_ba_index *ix, int stage) {
    if (!ctx || !index_args_ok(ix)) return 0;
    if (stage == 0) {
        Ws0 w;
        return ws0_layout(ix, ctx->stream, w) == hipSuccess ? w.total : 0;
    }
    if (stage != 1 || !band_ok(ix)) return 0;
    int64_t seg_cap, chunk_cap;
    mm_ba_index_bounds(ix->F, ix->cam_span, ix->n_pairs, ix->chunk, &seg_cap, &chunk_cap);
    Ws1 w;
    return ws1_layout(ix->n_pairs, seg_cap, bits_for((int64_t)ix->F * (ix->cam_span + 1)), ctx->stream, w) == hipSuccess ? w.total : 0;
}

int mm_ba_index_build(mm_ctx *ctx, const mm_ba_index *ix, int stage, void *ws0, size_t ws0_bytes, void *ws1, size_t ws1_bytes) {
    if (!ctx) return MM_ERR_ARG;
    if (!index_args_ok(ix) || !ix->pt_ptr || !ix->pt_obs || !ix->cam_ptr || !ix->cam_obs || !ws0 || ((uintptr_t)ws0 & 15))
        return mm_fail(ctx, MM_ERR_ARG, "mm_ba_index_build: bad argument");
    const int64_t O = ix->O;
    const unsigned gO = (unsigned)((O + 255) / 256);
    const int F_all = ix->F + ix->F_fixed;
    const bool ident = !ix->sort_by_point;
    hipStream_t st = ctx->stream;
    Ws0 w0;
    MM_HIP(ctx, ws0_layout(ix, st, w0));
    if (ws0_bytes < w0.total) return mm_fail(ctx, MM_ERR_WORKSPACE, "mm_ba_index_build: stage 0 workspace too small");
    uint8_t *b0 = (uint8_t *)ws0;
    int32_t *keys = (int32_t *)(b0 + w0.keys), *cnt = (int32_t *)(b0 + w0.cnt), *span = (int32_t *)(b0 + w0.span);
    int64_t *offs = (int64_t *)(b0 + w0.offs);
    if (stage == 0) {
        MM_HIP(ctx, hipMemsetAsync(ix->head, 0, 8 * sizeof(int64_t), st));
        MM_HIP(ctx, hipMemsetAsync(span, 0, sizeof(int32_t), st));
        MM_LAUNCH(ctx, "idx_validate_kernel", idx_validate_kernel, dim3(gO), dim3(256), 0, ix->fi, ix->pi, O, F_all, ix->P,
                  ident ? (int32_t *)nullptr : cnt, ix->head);
        size_t tb = w0.tmp_bytes;
        if (ident) {
            MM_LAUNCH(ctx, "idx_ptr_kernel", idx_ptr_kernel, dim3(gO), dim3(256), 0, ix->pi, O, ix->P, ix->pt_ptr, ix->pt_obs,
                      (const int64_t *)ix->head);
        } else {      // pt_obs: the identity carried through a stable sort of the point indices
            MM_HIP(ctx, rocprim::radix_sort_pairs((void *)(b0 + w0.tmp), tb, ix->pi, keys, (const int32_t *)cnt, ix->pt_obs, (size_t)O, 0u,
                                                  (unsigned)bits_for(ix->P), st));
            MM_LAUNCH(ctx, "idx_ptr_kernel", idx_ptr_kernel, dim3(gO), dim3(256), 0, (const int32_t *)keys, O, ix->P, ix->pt_ptr,
                      (int32_t *)nullptr, (const int64_t *)ix->head);
            tb = w0.tmp_bytes;
        }
        // cam_obs: the same through a stable sort of the camera indices (garbage, but in bounds, on bad input)
        MM_HIP(ctx, rocprim::radix_sort_pairs((void *)(b0 + w0.tmp), tb, ix->fi, keys, (const int32_t *)(ident ? ix->pt_obs : cnt),
                                              ix->cam_obs, (size_t)O, 0u, (unsigned)bits_for(F_all), st));
        MM_LAUNCH(ctx, "idx_ptr_kernel", idx_ptr_kernel, dim3(gO), dim3(256), 0, (const int32_t *)keys, O, ix->F, ix->cam_ptr,
                  (int32_t *)nullptr, (const int64_t *)ix->head);
        MM_LAUNCH(ctx, "idx_count_kernel", (ident ? idx_count_kernel<true> : idx_count_kernel<false>), dim3(gO), dim3(256), 0, ix->fi,
                  ix->pi, (const int32_t *)ix->pt_ptr, (const int32_t *)ix->pt_obs, O, ix->F, cnt, span, (const int64_t *)ix->head);
        tb = w0.tmp_bytes;
        MM_HIP(ctx, rocprim::exclusive_scan((void *)(b0 + w0.tmp), tb, (const int32_t *)cnt, offs, (int64_t)0, (size_t)O,
                                            rocprim::plus<int64_t>(), st));
        MM_LAUNCH(ctx, "idx_head0_kernel", idx_head0_kernel, dim3(1), dim3(1), 0, (const int32_t *)cnt, (const int64_t *)offs, O,
                  (const int32_t *)span, (const int32_t *)ix->cam_ptr, ix->F, ix->head);
        return MM_OK;
    }
    if (stage != 1) return mm_fail(ctx, MM_ERR_ARG, "mm_ba_index_build: stage must be 0 or 1");
    if (!band_ok(ix) || !ix->pair_o || !ix->pair_o2 || !ix->pair_p || !ix->seg_ids || !ix->seg_chunk_ptr || !ix->chunk_seg ||
        !ix->chunk_begin || !ix->chunk_end || !ws1 || ((uintptr_t)ws1 & 15))
        return mm_fail(ctx, MM_ERR_ARG, "mm_ba_index_build: bad stage 1 argument");
    int64_t seg_cap, chunk_cap;
    mm_ba_index_bounds(ix->F, ix->cam_span, ix->n_pairs, ix->chunk, &seg_cap, &chunk_cap);
    const int key_bits = bits_for((int64_t)ix->F * (ix->cam_span + 1));
    Ws1 w1;
    MM_HIP(ctx, ws1_layout(ix->n_pairs, seg_cap, key_bits, st, w1));
    if (ws1_bytes < w1.total) return mm_fail(ctx, MM_ERR_WORKSPACE, "mm_ba_index_build: stage 1 workspace too small");
    uint8_t *b1 = (uint8_t *)ws1;
    int32_t *key = (int32_t *)(b1 + w1.key), *key_s = (int32_t *)(b1 + w1.key_s), *counts = (int32_t *)(b1 + w1.counts);
    int32_t *n_seg = (int32_t *)(b1 + w1.n_seg), *pairs_of = (int32_t *)(b1 + w1.pairs_of), *chunks_of = (int32_t *)(b1 + w1.chunks_of);
    int32_t *seg_lo = (int32_t *)(b1 + w1.seg_lo);
    uint64_t *val = (uint64_t *)(b1 + w1.val), *val_s = (uint64_t *)(b1 + w1.val_s);
    const int64_t n = ix->n_pairs;
    const unsigned gN = (unsigned)((n + 255) / 256);
    // (a pair the emit kernel did not reach -- n_pairs larger than the truth -- must still be an index inside the arrays)
    MM_HIP(ctx, hipMemsetAsync(key, 0, (size_t)n * 4, st));
    MM_HIP(ctx, hipMemsetAsync(val, 0, (size_t)n * 8, st));
    MM_LAUNCH(ctx, "idx_emit_kernel", (ident ? idx_emit_kernel<true> : idx_emit_kernel<false>), dim3(gO), dim3(256), 0, ix->fi, ix->pi,
              (const int32_t *)ix->pt_ptr, (const int32_t *)ix->pt_obs, O, ix->F, (const int64_t *)offs, ix->cam_span, n, key, val,
              (const int64_t *)ix->head);
    size_t tb = w1.tmp_bytes;
    MM_HIP(ctx, rocprim::radix_sort_pairs((void *)(b1 + w1.tmp), tb, (const int32_t *)key, key_s, (const uint64_t *)val, val_s, (size_t)n,
                                          0u, (unsigned)key_bits, st));
    MM_LAUNCH(ctx, "idx_unpack_kernel", idx_unpack_kernel, dim3(gN), dim3(256), 0, (const uint64_t *)val_s, ix->pi, n, O, ix->pair_o,
              ix->pair_o2, ix->pair_p);
    tb = w1.tmp_bytes;
    MM_HIP(ctx, rocprim::run_length_encode((void *)(b1 + w1.tmp), tb, (const int32_t *)key_s, (size_t)n, ix->seg_ids, counts, n_seg, st));
    MM_LAUNCH(ctx, "idx_segcount_kernel", idx_segcount_kernel, dim3((unsigned)((seg_cap + 1 + 255) / 256)), dim3(256), 0,
              (const int32_t *)counts, (const int32_t *)n_seg, seg_cap, ix->chunk, pairs_of, chunks_of);
    tb = w1.tmp_bytes;
    MM_HIP(ctx, rocprim::exclusive_scan((void *)(b1 + w1.tmp), tb, (const int32_t *)pairs_of, seg_lo, (int32_t)0, (size_t)seg_cap + 1,
                                        rocprim::plus<int32_t>(), st));
    tb = w1.tmp_bytes;
    MM_HIP(ctx, rocprim::exclusive_scan((void *)(b1 + w1.tmp), tb, (const int32_t *)chunks_of, ix->seg_chunk_ptr, (int32_t)0,
                                        (size_t)seg_cap + 1, rocprim::plus<int32_t>(), st));
    MM_LAUNCH(ctx, "idx_chunks_kernel", idx_chunks_kernel, dim3((unsigned)((seg_cap * 64 + 255) / 256)), dim3(256), 0,
              (const int32_t *)n_seg, (const int32_t *)seg_lo, (const int32_t *)pairs_of, (const int32_t *)ix->seg_chunk_ptr, ix->chunk,
              chunk_cap, ix->chunk_seg, ix->chunk_begin, ix->chunk_end, ix->head);
    return MM_OK;
}

}  // extern "C"
