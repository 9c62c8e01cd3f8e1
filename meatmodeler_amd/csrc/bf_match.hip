// Brute-force Hamming 2-NN + Lowe ratio test for 256-bit descriptors (gfx950).
//
// Replaces cv2.FlannBasedMatcher(...).knnMatch(prev_desc, new_desc, k=2) and the ratio filter of
// processor.featureTracking (reference processor.py:132-137) by the exact search FLANN-LSH approximates.
//
// Mapping to the hardware.  The search is compute bound (0.02 B of HBM per descriptor pair), and
// there are two formulations of the distance in this file, returning identical results (ties -> lowest train index);
// bf_plan() below chooses between them (times: tools/bench_bf.py, 499 pairs of 4000 x 4000):
//  314  matrix cores, FP4 operands, ONE candidate per lane and train tile (bf_knn2_fp4min_kernel: the vector unit only
//       takes a minimum over the lane's 16 accumulators; 4 waves per SIMD): 0.95 ms = 8.4 T pairs/s       <- default
//       It reads the PACKED train descriptors and expands each 32-row tile to FP4 on its way into LDS (no expand pass,
//       no expanded copy in memory), and has the ratio test in its epilogue for mm_bf_match_ratio_batched.
//  114  xor / popcount on the vector unit (bf_knn2_lds_kernel, below): 3.9-4.2 ms = 2.0 T pairs/s; what small train
//       sets (< 64) and train sets of 65536 or more descriptors take, and what MM_BF_VARIANT=114 puts on every shape
// The numbers are the values of MM_BF_VARIANT, which accepts these two only.  The formulations that each held the default
// for a round before -- train descriptor fed by scalar loads, other tilings of the LDS-fed kernel, int8 matrix cores
// (1.9 ms), FP4 matrix cores with packed per-accumulator streams (1.15-1.2 ms), and the default at three waves per SIMD
// with its A operand read a tile ahead (no faster) -- are measured in profiles/r01_bf_variants.txt,
// profiles/r02_bf_variants.txt and profiles/r02_bf_pmc.txt; their code is in the history of this file.
// The matrix-core kernel is described where it is defined; the vector-unit formulation:
//  * one lane owns one query descriptor (8 VGPRs); a wave covers 64 queries, a workgroup 256;
//  * the workgroup stages 128 train descriptors at a time in LDS (double buffered, the next chunk's global loads fly
//    during the current chunk's compute); every lane reads the same train with two same-address ds_read_b128 (LDS
//    broadcast) so that the eight v_xor_b32 take VGPR operands (2.6 cycles per wave instruction; 4.1 with an SGPR
//    operand, measured: profiles/r01_valu_issue_rates.txt); 8 v_bcnt_u32_b32 accumulate the popcounts;
//  * trains are handled in groups of four: a candidate can only enter the two smallest keys (key = dist << 20 | train
//    index, ties -> lowest train index) if its distance is below the current second-best distance, so the group's
//    minimum is tested and the min / med3 bookkeeping sits behind a wave-uniform, rarely taken branch:
//    18.8 VALU instructions per descriptor pair, 16 of them the xor / popcount floor;
//  * no cross-lane traffic: the bound is VALU integer issue.  Measured with the SQ counters
//    (profiles/r02_bf_pmc.txt): 3.84 cycles per VALU instruction at the 2.1 GHz the chip holds under this load = 91 %
//    of the issue roof of this instruction mix (v_bcnt / v_min issue at quarter rate) -- which is why the distances
//    moved to the matrix cores;
//  * small launches split the train range over blockIdx.y and merge partial top-2 keys in a second kernel.
#include "mm_common.h"
#include <cstdlib>
#include <type_traits>

namespace {

constexpr int BF_THREADS = 256;
constexpr uint32_t BF_NONE = 0xFFFFFFFFu;
constexpr int BF_IDX_BITS = 20;

// popcount(x) + acc in ONE instruction.  Written as asm because hipcc otherwise re-associates the eight adds
// into v_bcnt + v_add3 trees (+3 VALU per pair, measured in the .s).
__device__ __forceinline__ uint32_t bcnt_acc(uint32_t x, uint32_t acc) {
    uint32_t r;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
    return r;
}

__device__ __forceinline__ uint32_t ham256(const uint32_t (&a)[8], const uint4 &t0, const uint4 &t1) {
    uint32_t d = bcnt_acc(a[0] ^ t0.x, 0u);
    d = bcnt_acc(a[1] ^ t0.y, d);
    d = bcnt_acc(a[2] ^ t0.z, d);
    d = bcnt_acc(a[3] ^ t0.w, d);
    d = bcnt_acc(a[4] ^ t1.x, d);
    d = bcnt_acc(a[5] ^ t1.y, d);
    d = bcnt_acc(a[6] ^ t1.z, d);
    d = bcnt_acc(a[7] ^ t1.w, d);
    return d;
}

__device__ __forceinline__ void top2_insert(uint32_t key, uint32_t &b0, uint32_t &b1) {
    // (b0 <= b1) and key  ->  two smallest of the three
    uint32_t hi = max(b0, key);
    b0 = min(b0, key);
    b1 = min(b1, hi);
}

// The xor / popcount kernel, its train descriptors fed from LDS.  Measured on MI355X (profiles/r01_valu_issue_rates.txt): v_xor_b32 issues in 2 cycles per wave with
// VGPR operands but in 4 with an SGPR operand; v_bcnt_u32_b32 / v_min / v_med3 / v_lshl_or take 4.  Feeding the train
// descriptor from VGPRs (two same-address ds_read_b128 = LDS broadcast, on the LDS pipe, not the VALU) makes the eight
// xors half price: 8*2 + 8*4 + 3*4 = 60 cycles per descriptor pair instead of ~82.  The workgroup stages BF_TCHUNK train
// descriptors at a time (registers -> LDS, double buffered: the next chunk's global loads fly during the current
// chunk's compute); all four waves read the same chunk.
constexpr int BF_TCHUNK = 128;  // trains per LDS stage: 4 KB, one 16-byte piece per thread

__device__ __forceinline__ void top2_insert_med3(uint32_t key, uint32_t &b0, uint32_t &b1) {
    uint32_t m;
    asm("v_med3_u32 %0, %1, %2, %3" : "=v"(m) : "v"(b0), "v"(b1), "v"(key));  // middle of three = new second smallest
    b0 = min(b0, key);
    b1 = m;
}

__global__ __launch_bounds__(BF_THREADS) void bf_knn2_lds_kernel(
    const uint8_t *__restrict__ q, const int32_t *__restrict__ nq_dev, int nq_cap, size_t q_stride,
    const uint8_t *__restrict__ t, const int32_t *__restrict__ nt_dev, int nt_cap, size_t t_stride, int n_splits,
    uint32_t *__restrict__ part, int32_t *__restrict__ idx, int32_t *__restrict__ dist) {
    // One query per lane.  The loops over u below have one trip; they stay because the compiler lays out the blocks of
    // the distance loop and of the epilogue differently without them, and this kernel's machine code is the measured one.
    constexpr int BF_QPL = 1;
    __shared__ uint4 tl[2][BF_TCHUNK * 2];
    const int pair = blockIdx.z;
    const int split = blockIdx.y;
    int nq = nq_dev ? min(nq_dev[pair], nq_cap) : nq_cap;
    int nt = nt_dev ? min(nt_dev[pair], nt_cap) : nt_cap;
    constexpr int BF_QTILE = BF_THREADS * BF_QPL;
    const int qbase = blockIdx.x * BF_QTILE;
    if (qbase >= nq) return;  // workgroup-uniform

    uint32_t qa[BF_QPL][8];
    const uint8_t *qp = q + (size_t)pair * q_stride;
#pragma unroll
    for (int u = 0; u < BF_QPL; ++u) {
        int qi = qbase + u * BF_THREADS + threadIdx.x;
        uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
        if (qi < nq) {
            const uint4 *p = reinterpret_cast<const uint4 *>(qp + (size_t)qi * 32);
            lo = p[0];
            hi = p[1];
        }
        qa[u][0] = lo.x; qa[u][1] = lo.y; qa[u][2] = lo.z; qa[u][3] = lo.w;
        qa[u][4] = hi.x; qa[u][5] = hi.y; qa[u][6] = hi.z; qa[u][7] = hi.w;
    }
    int chunk = (nt + n_splits - 1) / n_splits;
    chunk = (chunk + 3) & ~3;
    const int j0 = split * chunk;
    const int j1 = min(nt, j0 + chunk);
    uint32_t b0[BF_QPL], b1[BF_QPL];
#pragma unroll
    for (int u = 0; u < BF_QPL; ++u) b0[u] = b1[u] = BF_NONE;

    const uint4 *__restrict__ tp = reinterpret_cast<const uint4 *>(t + (size_t)pair * t_stride);
    // stage 0
    uint4 stage;
    {
        const int e = 2 * j0 + (int)threadIdx.x;
        stage = e < 2 * j1 ? tp[e] : make_uint4(0, 0, 0, 0);
        tl[0][threadIdx.x] = stage;
    }
    __syncthreads();
    int buf = 0;
    for (int c0 = j0; c0 < j1; c0 += BF_TCHUNK) {
        const int cn = min(BF_TCHUNK, j1 - c0);
        const int nxt = c0 + BF_TCHUNK;
        if (nxt < j1) {  // prefetch the next chunk into registers (in flight during the compute below)
            const int e = 2 * nxt + (int)threadIdx.x;
            stage = e < 2 * j1 ? tp[e] : make_uint4(0, 0, 0, 0);
        }
        const uint4 *tb = tl[buf];
        int k = 0;
        for (; k + 4 <= cn; k += 4) {
            uint4 tv[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) tv[r] = tb[2 * k + r];  // same address in every lane: LDS broadcast
            uint32_t d[4][BF_QPL];
            bool hit = false;
#pragma unroll
            for (int u = 0; u < BF_QPL; ++u) {
#pragma unroll
                for (int r = 0; r < 4; ++r) d[r][u] = ham256(qa[u], tv[2 * r], tv[2 * r + 1]);
                // train indices only grow, so a candidate enters the two smallest keys iff its DISTANCE is strictly
                // below the current second-best distance; test the group's minimum and skip the bookkeeping otherwise
                const uint32_t m = min(min(d[0][u], d[1][u]), min(d[2][u], d[3][u]));
                hit |= m < (b1[u] >> BF_IDX_BITS);
            }
            if (__builtin_amdgcn_ballot_w64(hit) != 0) {  // wave-uniform branch, rarely taken after the first trains
#pragma unroll
                for (int r = 0; r < 4; ++r) {
#pragma unroll
                    for (int u = 0; u < BF_QPL; ++u)
                        top2_insert_med3((d[r][u] << BF_IDX_BITS) | (uint32_t)(c0 + k + r), b0[u], b1[u]);
                }
            }
        }
        for (; k < cn; ++k) {
            const uint4 t0 = tb[2 * k], t1 = tb[2 * k + 1];
#pragma unroll
            for (int u = 0; u < BF_QPL; ++u) {
                uint32_t d = ham256(qa[u], t0, t1);
                top2_insert_med3((d << BF_IDX_BITS) | (uint32_t)(c0 + k), b0[u], b1[u]);
            }
        }
        if (nxt < j1) {
            tl[buf ^ 1][threadIdx.x] = stage;
            __syncthreads();
            buf ^= 1;
        }
    }
#pragma unroll
    for (int u = 0; u < BF_QPL; ++u) {
        int qi = qbase + u * BF_THREADS + threadIdx.x;
        if (qi >= nq) continue;
        if (n_splits == 1) {
            size_t o = ((size_t)pair * nq_cap + qi) * 2;
            idx[o] = b0[u] == BF_NONE ? -1 : (int32_t)(b0[u] & ((1u << BF_IDX_BITS) - 1));
            idx[o + 1] = b1[u] == BF_NONE ? -1 : (int32_t)(b1[u] & ((1u << BF_IDX_BITS) - 1));
            dist[o] = b0[u] == BF_NONE ? -1 : (int32_t)(b0[u] >> BF_IDX_BITS);
            dist[o + 1] = b1[u] == BF_NONE ? -1 : (int32_t)(b1[u] >> BF_IDX_BITS);
        } else {
            size_t o = (((size_t)pair * n_splits + split) * nq_cap + qi) * 2;
            part[o] = b0[u];
            part[o + 1] = b1[u];
        }
    }
}

__global__ __launch_bounds__(256) void bf_merge_kernel(const uint32_t *__restrict__ part,
                                                       const int32_t *__restrict__ nq_dev, int nq_cap, int n_splits,
                                                       int32_t *__restrict__ idx, int32_t *__restrict__ dist) {
    const int pair = blockIdx.y;
    const int qi = blockIdx.x * blockDim.x + threadIdx.x;
    int nq = nq_dev ? min(nq_dev[pair], nq_cap) : nq_cap;
    if (qi >= nq) return;
    uint32_t b0 = BF_NONE, b1 = BF_NONE;
    for (int s = 0; s < n_splits; ++s) {
        size_t o = (((size_t)pair * n_splits + s) * nq_cap + qi) * 2;
        top2_insert(part[o], b0, b1);
        top2_insert(part[o + 1], b0, b1);
    }
    size_t o = ((size_t)pair * nq_cap + qi) * 2;
    idx[o] = b0 == BF_NONE ? -1 : (int32_t)(b0 & ((1u << BF_IDX_BITS) - 1));
    idx[o + 1] = b1 == BF_NONE ? -1 : (int32_t)(b1 & ((1u << BF_IDX_BITS) - 1));
    dist[o] = b0 == BF_NONE ? -1 : (int32_t)(b0 >> BF_IDX_BITS);
    dist[o + 1] = b1 == BF_NONE ? -1 : (int32_t)(b1 >> BF_IDX_BITS);
}

// Order-preserving compaction of the queries that pass the ratio test; one workgroup per pair.
__global__ __launch_bounds__(256) void ratio_filter_kernel(const int32_t *__restrict__ idx,
                                                           const int32_t *__restrict__ dist,
                                                           const int32_t *__restrict__ nq_dev, int nq_cap,
                                                           double threshold, int32_t *__restrict__ pairs,
                                                           int32_t *__restrict__ m_out) {
    __shared__ int wave_cnt[4];
    __shared__ int base_s;
    const int pair = blockIdx.x;
    int nq = nq_dev ? min(nq_dev[pair], nq_cap) : nq_cap;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) base_s = 0;
    __syncthreads();
    for (int q0 = 0; q0 < nq; q0 += 256) {
        int qi = q0 + threadIdx.x;
        bool keep = false;
        int ti = -1;
        if (qi < nq) {
            size_t o = ((size_t)pair * nq_cap + qi) * 2;
            int d0 = dist[o], d1 = dist[o + 1];
            ti = idx[o];
            keep = (d0 >= 0) && (d1 >= 0) && ((double)d0 < threshold * (double)d1);
        }
        unsigned long long m = __ballot(keep);
        int before = __builtin_popcountll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wave_cnt[wave] = __builtin_popcountll(m);
        __syncthreads();
        int off = base_s;
        for (int w = 0; w < wave; ++w) off += wave_cnt[w];
        if (keep) {
            size_t o = ((size_t)pair * nq_cap + (off + before)) * 2;
            pairs[o] = qi;
            pairs[o + 1] = ti;
        }
        __syncthreads();
        if (threadIdx.x == 0) base_s += wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
        __syncthreads();
    }
    if (threadIdx.x == 0) m_out[pair] = base_s;
}

// The same compaction for the whole match stage (mm_bf_match_ratio_batched), one workgroup per pair.  CODES: the matching
// kernel has applied the ratio test already and `idx` holds one int32 per query [n_pairs, nq_cap], the train index of a
// match or -1; otherwise idx / dist are what the 2-NN kernels write and the test is made here.  Writes m_out and the -1
// tail pairs[p, m:nq_cap] itself, so the outputs need no fill; rows from nq on are never read.
template <bool CODES>
__global__ __launch_bounds__(256) void match_compact_kernel(const int32_t *__restrict__ idx,
                                                            const int32_t *__restrict__ dist,
                                                            const int32_t *__restrict__ nq_dev, int nq_cap,
                                                            double threshold, int32_t *__restrict__ pairs,
                                                            int32_t *__restrict__ m_out) {
    __shared__ int wave_cnt[2][4];      // (two sets: one barrier per round)
    const int pair = blockIdx.x;
    const int nq = nq_dev ? max(min(nq_dev[pair], nq_cap), 0) : nq_cap;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int2 *__restrict__ out = reinterpret_cast<int2 *>(pairs) + (size_t)pair * nq_cap;
    int base = 0, par = 0;
    for (int q0 = 0; q0 < nq; q0 += 256, par ^= 1) {
        const int qi = q0 + threadIdx.x;
        int ti = -1;
        if (qi < nq) {
            if constexpr (CODES) {
                ti = idx[(size_t)pair * nq_cap + qi];
            } else {
                const size_t o = ((size_t)pair * nq_cap + qi) * 2;
                const int d0 = dist[o], d1 = dist[o + 1];
                if ((d0 >= 0) && (d1 >= 0) && ((double)d0 < threshold * (double)d1)) ti = idx[o];
            }
        }
        const bool keep = ti >= 0;
        const unsigned long long m = __ballot(keep);
        if (lane == 0) wave_cnt[par][wave] = __builtin_popcountll(m);
        __syncthreads();
        const int c0 = wave_cnt[par][0], c1 = wave_cnt[par][1], c2 = wave_cnt[par][2], c3 = wave_cnt[par][3];
        const int off = base + (wave > 0 ? c0 : 0) + (wave > 1 ? c1 : 0) + (wave > 2 ? c2 : 0);
        if (keep) out[off + __builtin_popcountll(m & ((1ull << lane) - 1ull))] = make_int2(qi, ti);
        base += c0 + c1 + c2 + c3;
    }
    for (int j = base + (int)threadIdx.x; j < nq_cap; j += 256) out[j] = make_int2(-1, -1);
    if (threadIdx.x == 0) m_out[pair] = base;
}

// ---- Hamming distances on the matrix cores ------------------------------------------------------------------------------
// With the bits of a descriptor written as 256 values +1 / -1, the dot product of two descriptors is
// (#equal bits) - (#different bits) = 256 - 2 dist: all-pairs matching is a [queries x 256] x [256 x trains] GEMM.  The
// matching IS compute bound (0.02 B/pair) and the xor / popcount formulation sits at 91 % of ITS roof, 19 VALU instructions
// per pair (see the header), so this is where it belongs.  +1 and -1 are exact in FP4 (E2M1: 0x2 / 0xA), their products
// and sums up to 256 exact in the f32 accumulators, and v_mfma_scale_f32_32x32x64_f8f6f4 with FP4 operands is the fastest
// matrix instruction of the chip: measured 16 ns per instruction and SIMD with every SIMD busy against 29 ns for
// v_mfma_i32_32x32x32_i8 at half the K (tools/dev/mfma_rate.hip) -- 3.6x the int8 rate per descriptor pair.
//   * a descriptor is 256 nibbles = 128 bytes, a K-step takes 64 bits, a tile four matrix instructions per query tile;
//   * a wave keeps 64 queries resident as the B operand (2 column tiles x 4 K-steps x 16 bytes per lane, expanded from
//     the packed descriptors at kernel start); the workgroup (4 waves, 256 queries) streams train tiles of 32 descriptors
//     through LDS (144-byte row pitch: conflict-free ds_read_b128) as the A operand;
//   * D[m][n]: lane l holds column (= query) l % 32 and 16 of the 32 rows (= trains), so the two-smallest search needs
//     no cross-lane traffic until the two lanes of a query are merged at the end;
//   * the accumulators start at 1.5 * 2^23: the sum lands in the low mantissa bits as an integer, so the vector unit
//     works on the float's bit pattern.
typedef int bf_v4i __attribute__((ext_vector_type(4)));
typedef int bf_v8i __attribute__((ext_vector_type(8)));
typedef float bf_v16f __attribute__((ext_vector_type(16)));
constexpr int MF_TT = 32;        // train descriptors per tile
constexpr int F4_PITCH = 144;    // bytes per expanded descriptor row in LDS (128 + 16: conflict-free ds_read_b128)

// 32 descriptor bits -> 32 FP4 values in four words: nibble i of word k is bit 4 i + k, set -> -1 (0xA), clear -> +1 (0x2).
// Three shifts, four ands and four ors.  The values are neither in bit order nor of the sign written above (set = +1); a
// dot product does not care about the order of its terms nor about a sign common to both factors, so a kernel that expands
// BOTH operands this way gets exactly the sums of the in-order expansion (bf_knn2_fp4min_kernel does: queries at its
// start, train tiles on their way into LDS).
__device__ __forceinline__ bf_v4i bf_fp4x32_planes(uint32_t bits) {
    bf_v4i r;
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = (int)(((bits << (3 - k)) & 0x88888888u) | 0x22222222u);
    return r;
}

// ---- one candidate per (lane, train tile) -----------------------------------------------------------------------------------
// A two-smallest update of every accumulator costs 2 vector instructions per descriptor pair, 64 per wave and train tile:
// ~400 cycles beside ~270 cycles of matrix instructions, and the two do not overlap well (measured on the kernel that
// did so: profiles/r02_bf_variants.txt).  Here the 16 accumulators of a lane (16 trains x 1 query) only feed a MINIMUM:
// the row of each accumulator rides in the low bits of the value itself
// (C operand = 1.5 * 2^23 + 2^18 + row, a per-lane constant in registers that is never rewritten; train block scale 2^10:
// acc = 1.5 * 2^23 + 2^11 * dist + row, exact), so the tile's best (dist, row) is an 8-instruction v_min3_u32 tree over
// the raw bit patterns, 3 instructions turn it into a key  dist << 22 | tile * 32 + row, 2 more (v_med3 / v_min) keep the
// lane's two smallest tile minima: 13 instructions per 16 pairs.  The exact two smallest of a query are then
//     best   = the smallest tile minimum (tile t0),
//     second = min(the smallest minimum of the other tiles, the SECOND smallest inside tile t0),
// and the second term is recomputed once per (lane, query) at the end of the kernel with xor / popcount on the 15 other
// rows of that one tile (packed descriptors from global memory): ~300 instructions per lane and query against ~6000 saved.
// Ties go to the lowest train index as everywhere (keys order by (dist, tile, row)).

// The 13 instructions per (query tile, train tile) in four chunks (5 + 3 + 3 + 2) so that each can be placed behind one
// matrix instruction of the OTHER query tile.
struct F4mState {
    uint32_t m[5], last, n0, n1, key;
};
template <bool PARTIAL>
__device__ __forceinline__ void f4m_chunk0(const bf_v16f &acc, F4mState &st, int h, int dead_from) {
    uint32_t v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const float f = acc[i];      // (value first: a bit cast of the element reference reads element 0)
        v[i] = __float_as_uint(f);
        if constexpr (PARTIAL) {
            const int m = 8 * (i >> 2) + 4 * h + (i & 3);
            if (m >= dead_from) v[i] = 0xFFFFFFFFu;
        }
    }
    // minimum of 16 as v_min3_u32 x 8 (all values share sign and exponent: unsigned order = numeric order)
#pragma unroll
    for (int g = 0; g < 5; ++g) st.m[g] = min(min(v[3 * g], v[3 * g + 1]), v[3 * g + 2]);
    st.last = v[15];
}
__device__ __forceinline__ void f4m_chunk1(F4mState &st) {
    st.n0 = min(min(st.m[0], st.m[1]), st.m[2]);
    st.n1 = min(min(st.m[3], st.m[4]), st.last);
    st.n0 = min(st.n0, st.n1);
}
template <bool PARTIAL>
__device__ __forceinline__ void f4m_chunk2(F4mState &st, uint32_t tile32) {
    // key = dist << 22 | tile * 32 + row   (mask: mantissa bits 5..21 = dist << 11; bit 22 is the 1.5)
    const uint32_t m = st.n0;
    uint32_t k = ((m & 0x003FFFE0u) << 11) + tile32;
    k = (m & 31u) | k;
    if constexpr (PARTIAL) k = m == 0xFFFFFFFFu ? BF_NONE : k;
    st.key = k;
}
__device__ __forceinline__ void f4m_update(uint32_t k, uint32_t &b0, uint32_t &b1) {      // b0 <= b1
    asm("v_med3_u32 %0, %1, %2, %3" : "=v"(b1) : "v"(b0), "v"(b1), "v"(k));      // = min(max(b0, k), b1) for b0 <= b1
    b0 = min(b0, k);
}

#ifdef MM_BF_CLOCK
// diagnostic build only (tools/dev/bf_inkernel_clock.sh): shader clock the kernel ran at = s_memtime ticks per 100 MHz
// s_memrealtime tick around each workgroup's life; the product build executes no stamp
__device__ long long g_bf_clock[2 * 4096];
#endif
// A wave reads the A operand of a train tile from LDS after the barrier that published it, four registers per K-step that
// the next tile overwrites: with the resident queries and the two accumulator sets, four waves per SIMD fit.  Train
// tiles rotate through THREE LDS buffers although a tile is only read after its barrier: the commit runs two tiles ahead
// of the compute (the schedule the kernel was tuned with; see the comment at tile_step).
// RATIO: the epilogue applies the ratio test of ratio_filter_kernel to the two neighbours it holds and writes ONE int32
// per query to idx [n_pairs, nq_cap] -- the train index of a match, or -1 -- instead of idx / dist (dist is not used).
template <bool RATIO>
__global__ __launch_bounds__(BF_THREADS, 4) void bf_knn2_fp4min_kernel(
    const uint8_t *__restrict__ q, const int32_t *__restrict__ nq_dev, int nq_cap, size_t q_stride,
    const uint8_t *__restrict__ tpk, size_t t_stride, const int32_t *__restrict__ nt_dev,
    int nt_cap, int32_t *__restrict__ idx, int32_t *__restrict__ dist, int qtiles, int n_pairs, double threshold) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[3][MF_TT][F4_PITCH];
    // XCD-aware order: workgroups are dealt round-robin to the 8 XCDs (each with its own L2), so the linear id is read as
    // (slot, xcd) and an XCD walks ITS pairs one after the other, all query tiles of a pair side by side: the train
    // set of a pair (128 KB packed at 4000 key points) is fetched into one L2 instead of into all eight.
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int grp = slot / qtiles;
    const int pair = grp * 8 + xcd;
    if (pair >= n_pairs) return;      // (padding of the last group of eight pairs)
    const int nq = nq_dev ? min(nq_dev[pair], nq_cap) : nq_cap;
    const int nt = nt_dev ? min(nt_dev[pair], nt_cap) : nt_cap;
    const int qbase = (slot - grp * qtiles) * BF_THREADS;
    if (qbase >= nq) return;  // workgroup-uniform
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int c = lane & 31, h = lane >> 5;
#ifdef MM_BF_CLOCK
    const long long clk_t0 = __builtin_readcyclecounter();
    const unsigned long long clk_r0 = __builtin_amdgcn_s_memrealtime();
#endif
    bf_v4i B4[2][4];
    const uint8_t *qp = q + (size_t)pair * q_stride;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int qi = qbase + 64 * wv + 32 * u + c;
        uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
        if (qi < nq) {
            const uint4 *p = reinterpret_cast<const uint4 *>(qp + (size_t)qi * 32);
            lo = p[0];
            hi = p[1];
        }
        const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bf_v4i e = bf_fp4x32_planes(~(h ? w[2 * j + 1] : w[2 * j]));      // queries enter NEGATED
            B4[u][j] = e;
        }
    }
    // C operand: 1.5 * 2^23 + 2^18 + row of accumulator i (rows 8 (i / 4) + 4 h + i % 4): never rewritten
    bf_v16f cinit;
#pragma unroll
    for (int i = 0; i < 16; ++i) cinit[i] = 12582912.0f + 262144.0f + (float)(8 * (i >> 2) + 4 * h + (i & 3));
    uint32_t b0[2] = {BF_NONE, BF_NONE}, b1[2] = {BF_NONE, BF_NONE};      // the two smallest tile minima per query
    const int ntiles = (nt + MF_TT - 1) / MF_TT;
    // Train tiles come straight from the PACKED descriptors: a tile is 1 KB, thread e0 takes word e0 & 7 of row e0 >> 3 (a
    // wave reads 256 contiguous bytes), keeps it in one register while it is in flight and expands it to its 16 bytes of
    // FP4 on the way into LDS (11 vector instructions per tile).  Rows from nt_cap on read as 0 bits.
    const uint8_t *tp = tpk + (size_t)pair * t_stride;
    const int e0 = threadIdx.x;
    uint32_t ra, rb, rc;
    auto fetch = [&](int tt, auto set) __attribute__((always_inline)) {
        constexpr int S = decltype(set)::value;
        if (tt < ntiles) {      // (workgroup-uniform)
            const uint32_t v = tt * MF_TT + (e0 >> 3) < nt_cap
                                   ? reinterpret_cast<const uint32_t *>(tp + (size_t)tt * MF_TT * 32)[e0] : 0u;
            if constexpr (S == 0) ra = v;
            if constexpr (S == 1) rb = v;
            if constexpr (S == 2) rc = v;
        }
    };
    auto commit = [&](int buf, auto set) __attribute__((always_inline)) {
        constexpr int S = decltype(set)::value;
        bf_v4i *d = reinterpret_cast<bf_v4i *>(&tile[buf][e0 >> 3][(e0 & 7) * 16]);
        if constexpr (S == 0) *d = bf_fp4x32_planes(ra);
        if constexpr (S == 1) *d = bf_fp4x32_planes(rb);
        if constexpr (S == 2) *d = bf_fp4x32_planes(rc);
    };
    // One train tile = two phases of 4 matrix instructions (query tile 0, query tile 1); the 13 vector instructions that
    // go with a phase's results run in the shadow of the NEXT phase's matrix instructions (query tile 1 of tile t-1 beside
    // query tile 0 of tile t: carried across the barrier).  cbsz = blgp = 4: FP4 operands; block scales (E8M0): train
    // operand 137 = 2^10, queries 127 = 1.0.
    // Tile t is computed from LDS buffer t % 3 while tile t + 2 is committed to buffer (t + 2) % 3, one barrier per tile.
    // Two buffers would be enough to keep a commit away from the tile being read; the third keeps the commit one barrier
    // further ahead of its readers, so a tile has five iterations from its request to its use (three in registers, two in
    // LDS).  That is the schedule this kernel was tuned and measured with, and 13.5 KB of LDS does not limit the four
    // workgroups of a CU.
    bf_v16f acc1_prev;
    bf_v4i A4[4];      // (four registers per K-step; the instruction's operand type is eight wide, the upper half unused for FP4)
    auto read_a = [&](int buf, int j) __attribute__((always_inline)) {
        A4[j] = *reinterpret_cast<const bf_v4i *>(&tile[buf][c][32 * j + 16 * h]);
    };
#define F4M_A(j) (bf_v8i{A4[j][0], A4[j][1], A4[j][2], A4[j][3], 0, 0, 0, 0})
#define F4M_B(u, j) (bf_v8i{B4[u][j][0], B4[u][j][1], B4[u][j][2], B4[u][j][3], 0, 0, 0, 0})
    // A wave whose 64 queries all lie past the pair's last one (the fourth wave of the 16th query tile at 4000 key points)
    // only helps to stage the train tiles: no matrix instructions, no bookkeeping -- 1/64 of the matrix work at that size.
    const bool wave_active = __builtin_amdgcn_readfirstlane(qbase + 64 * wv) < nq;
    auto tile_step = [&](int tt, auto cur_tag, auto first_tag) __attribute__((always_inline)) {
        constexpr bool HAVE_PREV = !decltype(first_tag)::value;
        if (!wave_active) return;
#pragma unroll
        for (int j = 0; j < 4; ++j) read_a(decltype(cur_tag)::value, j);      // buffer tt % 3
        // query tile 0 of this train tile beside the bookkeeping of query tile 1 of the previous one, then query tile 1
        // beside the bookkeeping of query tile 0: one matrix instruction, one chunk of vector work, and so on
        F4mState st;
        bf_v16f acc0 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(F4M_A(0), F4M_B(0, 0), cinit, 4, 4, 0, 137, 0, 127);
        if constexpr (HAVE_PREV) f4m_chunk0<false>(acc1_prev, st, h, 0);
        __builtin_amdgcn_sched_barrier(0);
        acc0 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(F4M_A(1), F4M_B(0, 1), acc0, 4, 4, 0, 137, 0, 127);
        if constexpr (HAVE_PREV) f4m_chunk1(st);
        __builtin_amdgcn_sched_barrier(0);
        acc0 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(F4M_A(2), F4M_B(0, 2), acc0, 4, 4, 0, 137, 0, 127);
        if constexpr (HAVE_PREV) f4m_chunk2<false>(st, (uint32_t)(tt - 1) * MF_TT);
        __builtin_amdgcn_sched_barrier(0);
        acc0 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(F4M_A(3), F4M_B(0, 3), acc0, 4, 4, 0, 137, 0, 127);
        if constexpr (HAVE_PREV) f4m_update(st.key, b0[1], b1[1]);
        __builtin_amdgcn_sched_barrier(0);
        bf_v16f acc1 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(F4M_A(0), F4M_B(1, 0), cinit, 4, 4, 0, 137, 0, 127);
        f4m_chunk0<false>(acc0, st, h, 0);
        __builtin_amdgcn_sched_barrier(0);
        acc1 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(F4M_A(1), F4M_B(1, 1), acc1, 4, 4, 0, 137, 0, 127);
        f4m_chunk1(st);
        __builtin_amdgcn_sched_barrier(0);
        acc1 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(F4M_A(2), F4M_B(1, 2), acc1, 4, 4, 0, 137, 0, 127);
        f4m_chunk2<false>(st, (uint32_t)tt * MF_TT);
        __builtin_amdgcn_sched_barrier(0);
        acc1 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(F4M_A(3), F4M_B(1, 3), acc1, 4, 4, 0, 137, 0, 127);
        f4m_update(st.key, b0[0], b1[0]);
        __builtin_amdgcn_sched_barrier(0);
        acc1_prev = acc1;
    };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    // tile t lives in register set / LDS buffer t % 3
    fetch(0, I0{});
    fetch(1, I1{});
    fetch(2, I2{});
    if (ntiles > 0) commit(0, I0{});
    fetch(3, I0{});
    if (ntiles > 1) commit(1, I1{});
    fetch(4, I1{});
    __syncthreads();
    const int nfull = nt / MF_TT;
    // iteration tt (tt % 3 == CUR): compute tile tt from LDS buffer CUR, commit tile tt + 2, request tile tt + 5
    auto iteration = [&](int tt, auto cur_tag, auto first_tag) __attribute__((always_inline)) {
        constexpr int C2 = (decltype(cur_tag)::value + 2) % 3;
        tile_step(tt, cur_tag, first_tag);
        if (tt + 2 < ntiles) commit(C2, std::integral_constant<int, C2>{});
        fetch(tt + 5, std::integral_constant<int, C2>{});
        __syncthreads();
    };
    int tt = 0;
    if (nfull > 0) {      // peeled: the first tile has no predecessor
        iteration(0, I0{}, std::true_type{});
        tt = 1;
        if (tt < nfull) { iteration(tt, I1{}, std::false_type{}); ++tt; }
        if (tt < nfull) { iteration(tt, I2{}, std::false_type{}); ++tt; }
    }
    for (; tt + 3 <= nfull; tt += 3) {      // (tt is a multiple of 3 here)
        iteration(tt, I0{}, std::false_type{});
        iteration(tt + 1, I1{}, std::false_type{});
        iteration(tt + 2, I2{}, std::false_type{});
    }
    if (tt < nfull) {
        iteration(tt, I0{}, std::false_type{});
        if (tt + 1 < nfull) iteration(tt + 1, I1{}, std::false_type{});
    }
    auto book = [&](const bf_v16f &acc, uint32_t tile32, int u, auto partial_tag, int dead_from) __attribute__((always_inline)) {
        constexpr bool PARTIAL = decltype(partial_tag)::value;
        F4mState st;
        f4m_chunk0<PARTIAL>(acc, st, h, dead_from);
        f4m_chunk1(st);
        f4m_chunk2<PARTIAL>(st, tile32);
        f4m_update(st.key, b0[u], b1[u]);
    };
    if (!wave_active) return;      // (no barrier follows)
    if (nfull > 0) book(acc1_prev, (uint32_t)(nfull - 1) * MF_TT, 1, std::false_type{}, 0);
    if (nfull < ntiles) {      // the partial last tile, unpipelined: rows past the last train never win
        bf_v16f acc0 = cinit, acc1 = cinit;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            read_a(nfull % 3, j);
            acc0 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(F4M_A(j), F4M_B(0, j), acc0, 4, 4, 0, 137, 0, 127);
            acc1 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(F4M_A(j), F4M_B(1, j), acc1, 4, 4, 0, 137, 0, 127);
        }
        const int dead_from = nt - nfull * MF_TT;
        book(acc0, (uint32_t)nfull * MF_TT, 0, std::true_type{}, dead_from);
        book(acc1, (uint32_t)nfull * MF_TT, 1, std::true_type{}, dead_from);
    }
    // the second smallest INSIDE the best tile, by xor / popcount on the lane's 15 other rows of that tile
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int qi = qbase + 64 * wv + 32 * u + c;
        {
            // (all loads unconditional on clamped rows and issued in four batches of four: a guarded load per row turns into
            // sixteen dependent trips to memory)
            const uint4 *p = reinterpret_cast<const uint4 *>(qp + (size_t)min(qi, nq - 1) * 32);
            const uint4 lo = p[0], hi = p[1];
            const uint32_t a[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
            const bool have = b0[u] != BF_NONE;
            const uint32_t best_idx = have ? (b0[u] & 0xFFFFu) : 0u, t0 = best_idx & ~31u;
            const uint32_t last = (uint32_t)max(nt - 1, 0);
            uint32_t c2 = BF_NONE;
#pragma unroll
            for (int part = 0; part < 4; ++part) {
                uint4 r0[4], r1[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int ii = 4 * part + i;
                    const uint32_t ti = t0 + (uint32_t)(8 * (ii >> 2) + 4 * h + (ii & 3));
                    const uint4 *r = reinterpret_cast<const uint4 *>(tp + (size_t)min(ti, last) * 32);
                    r0[i] = r[0];
                    r1[i] = r[1];
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int ii = 4 * part + i;
                    const uint32_t ti = t0 + (uint32_t)(8 * (ii >> 2) + 4 * h + (ii & 3));
                    const uint32_t key = (ham256(a, r0[i], r1[i]) << 22) | ti;
                    c2 = (have && ti != best_idx && ti < (uint32_t)nt) ? min(c2, key) : c2;
                }
            }
            b1[u] = min(b1[u], c2);
        }
        // the two lanes of a query (rows 4 h ..) -> one result
        const uint32_t o0 = __shfl_xor(b0[u], 32, 64), o1 = __shfl_xor(b1[u], 32, 64);
        top2_insert(o0, b0[u], b1[u]);
        top2_insert(o1, b0[u], b1[u]);
        if (h == 0 && qi < nq) {
            if constexpr (RATIO) {      // (the comparison of ratio_filter_kernel; fewer than two neighbours: never a match)
                const bool keep = b0[u] != BF_NONE && b1[u] != BF_NONE &&
                                  (double)(int32_t)(b0[u] >> 22) < threshold * (double)(int32_t)(b1[u] >> 22);
                idx[(size_t)pair * nq_cap + qi] = keep ? (int32_t)(b0[u] & 0xFFFFu) : -1;
            } else {
                const size_t o = ((size_t)pair * nq_cap + qi) * 2;
                idx[o] = b0[u] == BF_NONE ? -1 : (int32_t)(b0[u] & 0xFFFFu);
                idx[o + 1] = b1[u] == BF_NONE ? -1 : (int32_t)(b1[u] & 0xFFFFu);
                dist[o] = b0[u] == BF_NONE ? -1 : (int32_t)(b0[u] >> 22);
                dist[o + 1] = b1[u] == BF_NONE ? -1 : (int32_t)(b1[u] >> 22);
            }
        }
    }
#ifdef MM_BF_CLOCK
    if (threadIdx.x == 0) {
        const unsigned w = blockIdx.x & 4095u;
        g_bf_clock[2 * w] = __builtin_readcyclecounter() - clk_t0;
        g_bf_clock[2 * w + 1] = (long long)(__builtin_amdgcn_s_memrealtime() - clk_r0);
    }
#endif
}

#undef F4M_B
#undef F4M_A

// ---- the plan: which kernel, how many splits, how much workspace -----------------------------------------------------------
// Everything the entry points decide about a shape, computed once per call (one look at the environment).
struct BfPlan {
    bool matrix;         // bf_knn2_fp4min_kernel; otherwise bf_knn2_lds_kernel (+ bf_merge_kernel when splits > 1)
    int splits;          // train-range splits of the popcount kernel (1 with matrix)
    size_t knn_bytes;    // workspace of the search itself (never 0: the search wants a pointer)
    bool bad_variant;    // MM_BF_VARIANT names a removed kernel: the size functions plan as for the default, compute refuses
};

BfPlan bf_plan(int n_pairs, int nq_cap, int nt_cap) {
    // MM_BF_VARIANT: unset, 0 or 314 = the rule below; 114 = the popcount kernel on every shape (how the tests put it on
    // matrix-sized inputs)
    const char *e = getenv("MM_BF_VARIANT");
    const int forced = e ? atoi(e) : 0;
    BfPlan p;
    p.bad_variant = forced != 0 && forced != 314 && forced != 114;
    // the matrix-core kernel keeps train indices in 16 bits and pays off from two train tiles on
    const bool matrix_shape = forced != 114 && nt_cap >= 64 && nt_cap < 65536;
    p.matrix = matrix_shape && n_pairs > 0 && nq_cap > 0;
    p.splits = 1;
    if (!matrix_shape) {      // small launches of the popcount kernel split the train range to fill the chip
        const long waves = (long)n_pairs * ((nq_cap + BF_THREADS - 1) / BF_THREADS) * (BF_THREADS / 64);
        if (waves > 0) {
            long s = (2048 + waves - 1) / waves;  // aim for >= 2 waves per SIMD on 256 CUs
            long smax = (nt_cap + 127) / 128;     // keep >= 128 trains per split
            if (s > smax) s = smax;
            if (s > 64) s = 64;
            if (s < 1) s = 1;
            p.splits = (int)s;
        }
    }
    // partial top-2 keys of every split; with one split (and with the matrix kernel) nothing is held
    p.knn_bytes = p.splits == 1 ? 256 : mm_align_up((size_t)n_pairs * p.splits * nq_cap * 2 * sizeof(uint32_t), 256);
    return p;
}

}  // namespace

#ifdef MM_BF_CLOCK
extern "C" int mm_debug_bf_clock(long long *host /*[2*4096]*/) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_bf_clock), sizeof(g_bf_clock));
}
#endif

namespace {

// The 2-NN search of mm_bf_knn2_batched under `plan`.  ratio != nullptr (only with plan.matrix) asks for the fused form:
// idx then receives one int32 per query, the train index of a match under threshold *ratio or -1, and dist is not used.
int bf_knn2_run(mm_ctx *ctx, const BfPlan &plan, const uint8_t *q, const int32_t *nq, int nq_cap, size_t q_set_stride,
                const uint8_t *t, const int32_t *nt, int nt_cap, size_t t_set_stride, int n_pairs, int32_t *idx,
                int32_t *dist, void *ws, size_t ws_bytes, const double *ratio) {
    if (plan.bad_variant)
        return mm_fail(ctx, MM_ERR_ARG, "mm_bf_knn2_batched: MM_BF_VARIANT accepts 314 (matrix cores, the default) and 114 "
                                        "(xor / popcount) only; the other variants were removed");
    if (n_pairs == 0 || nq_cap == 0) return MM_OK;
    if (!q || (!t && nt_cap > 0) || !idx || (!dist && !ratio) || n_pairs < 0 || nq_cap < 0 || nt_cap < 0)
        return mm_fail(ctx, MM_ERR_ARG, "mm_bf_knn2_batched: bad argument");
    if (nt_cap >= (1 << BF_IDX_BITS)) return mm_fail(ctx, MM_ERR_ARG, "mm_bf_knn2_batched: nt_cap must be < 2^20");
    if (((uintptr_t)q | (uintptr_t)t | q_set_stride | t_set_stride) & 15)
        return mm_fail(ctx, MM_ERR_ARG, "mm_bf_knn2_batched: descriptors must be 16-byte aligned");
    if (n_pairs > 65535) return mm_fail(ctx, MM_ERR_ARG, "mm_bf_knn2_batched: at most 65535 pairs per call");
    const int s = plan.splits;
    if (s > 1 && (!ws || ws_bytes < plan.knn_bytes))
        return mm_fail(ctx, MM_ERR_WORKSPACE, "mm_bf_knn2_batched: workspace too small");
    const int qtiles = (nq_cap + BF_THREADS - 1) / BF_THREADS;
    if (plan.matrix) {      // no expand pass: the kernel reads the packed descriptors
        if (!ws || ws_bytes < plan.knn_bytes || ((uintptr_t)ws & 15))
            return mm_fail(ctx, MM_ERR_WORKSPACE, "mm_bf_knn2_batched: workspace too small or misaligned");
        const dim3 grid_x(8u * (unsigned)((n_pairs + 7) / 8) * (unsigned)qtiles);      // (slot, xcd): see the kernel
        const double thr = ratio ? *ratio : 0.0;
        if (ratio)
            MM_LAUNCH(ctx, "bf_knn2_fp4min_kernel", bf_knn2_fp4min_kernel<true>, grid_x, dim3(BF_THREADS), 0, q, nq, nq_cap,
                      q_set_stride, t, t_set_stride, nt, nt_cap, idx, dist, qtiles, n_pairs, thr);
        else
            MM_LAUNCH(ctx, "bf_knn2_fp4min_kernel", bf_knn2_fp4min_kernel<false>, grid_x, dim3(BF_THREADS), 0, q, nq, nq_cap,
                      q_set_stride, t, t_set_stride, nt, nt_cap, idx, dist, qtiles, n_pairs, thr);
        return MM_OK;
    }
    MM_LAUNCH(ctx, "bf_knn2_lds_kernel", bf_knn2_lds_kernel, dim3(qtiles, s, n_pairs), dim3(BF_THREADS), 0, q, nq, nq_cap,
              q_set_stride, t, nt, nt_cap, t_set_stride, s, (uint32_t *)ws, idx, dist);
    if (s > 1) {
        dim3 g2((nq_cap + 255) / 256, n_pairs);
        MM_LAUNCH(ctx, "bf_merge_kernel", bf_merge_kernel, g2, dim3(256), 0, (const uint32_t *)ws, nq, nq_cap, s, idx, dist);
    }
    return MM_OK;
}

// workspace of mm_bf_match_ratio_batched: the search's own, then what the search hands to the compaction
struct BfMatchWs {
    size_t knn, idx, dist, total;      // byte offsets of idx / dist behind the search's workspace of `knn` bytes
};
BfMatchWs bf_match_ws(const BfPlan &plan, int n_pairs, int nq_cap) {
    BfMatchWs w;
    w.knn = mm_align_up(plan.knn_bytes, 256);
    const size_t rows = (size_t)max(n_pairs, 0) * (size_t)max(nq_cap, 0);
    const bool fused = plan.matrix;      // one code per query instead of idx + dist
    const size_t one = mm_align_up(rows * (fused ? 1 : 2) * sizeof(int32_t), 256);
    w.idx = w.knn;
    w.dist = fused ? w.idx : w.idx + one;
    w.total = w.dist + one;
    return w;
}

}  // namespace

extern "C" {

int mm_bf_knn2_batched(mm_ctx *ctx, const uint8_t *q, const int32_t *nq, int nq_cap, size_t q_set_stride,
                       const uint8_t *t, const int32_t *nt, int nt_cap, size_t t_set_stride, int n_pairs,
                       int32_t *idx, int32_t *dist, void *ws, size_t ws_bytes) {
    if (!ctx) return MM_ERR_ARG;
    return bf_knn2_run(ctx, bf_plan(n_pairs, nq_cap, nt_cap), q, nq, nq_cap, q_set_stride, t, nt, nt_cap, t_set_stride, n_pairs,
                       idx, dist, ws, ws_bytes, nullptr);
}

size_t mm_bf_workspace_bytes(int n_pairs, int nq_cap, int nt_cap) { return bf_plan(n_pairs, nq_cap, nt_cap).knn_bytes; }

size_t mm_bf_match_ratio_workspace_bytes(int n_pairs, int nq_cap, int nt_cap) {
    return bf_match_ws(bf_plan(n_pairs, nq_cap, nt_cap), n_pairs, nq_cap).total;
}

int mm_bf_match_ratio_batched(mm_ctx *ctx, const uint8_t *q, const int32_t *nq, int nq_cap, size_t q_set_stride,
                              const uint8_t *t, const int32_t *nt, int nt_cap, size_t t_set_stride, int n_pairs,
                              double threshold, int32_t *pairs, int32_t *m_out, void *ws, size_t ws_bytes) {
    if (!ctx) return MM_ERR_ARG;
    if (n_pairs == 0) return MM_OK;
    if (n_pairs < 0 || nq_cap < 0 || nt_cap < 0 || !m_out || (!pairs && nq_cap > 0))
        return mm_fail(ctx, MM_ERR_ARG, "mm_bf_match_ratio_batched: bad argument");
    const BfPlan plan = bf_plan(n_pairs, nq_cap, nt_cap);
    const BfMatchWs w = bf_match_ws(plan, n_pairs, nq_cap);
    if (!ws || ws_bytes < w.total || ((uintptr_t)ws & 15))
        return mm_fail(ctx, MM_ERR_WORKSPACE, "mm_bf_match_ratio_batched: workspace too small or misaligned");
    int32_t *idx = (int32_t *)((uint8_t *)ws + w.idx), *dist = (int32_t *)((uint8_t *)ws + w.dist);
    const bool fused = plan.matrix;
    const int rc = bf_knn2_run(ctx, plan, q, nq, nq_cap, q_set_stride, t, nt, nt_cap, t_set_stride, n_pairs, idx, dist, ws,
                               w.knn, fused ? &threshold : nullptr);
    if (rc != MM_OK) return rc;
    if (fused)
        MM_LAUNCH(ctx, "match_compact_kernel", match_compact_kernel<true>, dim3(n_pairs), dim3(256), 0, idx, (const int32_t *)nullptr, nq, nq_cap,
                  threshold, pairs, m_out);
    else
        MM_LAUNCH(ctx, "match_compact_kernel", match_compact_kernel<false>, dim3(n_pairs), dim3(256), 0, idx, dist, nq, nq_cap,
                  threshold, pairs, m_out);
    return MM_OK;
}

int mm_bf_knn2_hamming(mm_ctx *ctx, const uint8_t *q, int nq, const uint8_t *t, int nt, int32_t *idx, int32_t *dist,
                       void *ws, size_t ws_bytes) {
    return mm_bf_knn2_batched(ctx, q, nullptr, nq, 0, t, nullptr, nt, 0, 1, idx, dist, ws, ws_bytes);
}

int mm_ratio_filter_batched(mm_ctx *ctx, const int32_t *idx, const int32_t *dist, const int32_t *nq, int nq_cap,
                            int n_pairs, double threshold, int32_t *pairs, int32_t *m_out) {
    if (!ctx) return MM_ERR_ARG;
    if (n_pairs == 0) return MM_OK;
    if (!idx || !dist || !pairs || !m_out || n_pairs < 0 || nq_cap < 0)
        return mm_fail(ctx, MM_ERR_ARG, "mm_ratio_filter_batched: bad argument");
    MM_LAUNCH(ctx, "ratio_filter_kernel", ratio_filter_kernel, dim3(n_pairs), dim3(256), 0, idx, dist, nq, nq_cap, threshold, pairs, m_out);
    return MM_OK;
}

}  // extern "C"
