// Dense depth (mm_depth_sweep, mm_depth_fuse; gfx950): a plane-sweep depth map per reference view from the adjusted cameras, and
// the maps of several views checked against each other and compacted into a point cloud.  include/meatmodeler.h has the
// definition, operation by operation; this file is built without FMA contraction (Makefile) and uses only + - * / sqrt floor
// rint and conversions, all correctly rounded, so the NumPy restatement of tests/test_dense_depth_cpu.py gives the same bits.
//
// Sweep.  ds_column_kernel writes, per (view, source, plane), the third column A_i2 + w_k b_i of the plane's homography (one
// thread each: 3 doubles).  ds_sweep_kernel: one workgroup of 256 threads per 16 x 16 tile of the valid interior, grid (tiles,
// V).  A thread keeps the n centred values of its reference window in registers (the window radius is a template parameter),
// filled once from the (16 + 2r)^2 patch in LDS.  Per (plane, source) the workgroup warps the (16 + 2r)^2 halo pixels -- one
// f64 warp and one bilinear sample (four u8 loads through L1 / L2) per halo pixel, not n per output pixel -- into one of two LDS
// tiles (rows padded to 48 floats, conflict-free; an invalid sample is a NaN, which no later comparison lets through), one barrier, and every thread reads its n samples
// from LDS once and sums in the defined order.  The best cost, its plane and the costs of the two neighbouring planes stay in
// registers.  What bounds it: n LDS reads and about 6 n f32 operations per pixel, plane and source; the VALU issues, not the
// LDS.  ds_border_kernel writes NaN / -1 outside the interior.
//
// Fuse.  df_test_kernel: one thread per pixel judges it against its view's neighbours; kept and candidate pixels are counted
// per chunk of MM_FILTER_CHUNK pixels.  df_scan_kernel: exclusive scan of the chunk sums (one workgroup walks an array alone).
// df_emit_kernel: every chunk places its kept pixels, (view, row, column) order, rows beyond cap not written.  Separate
// launches, no workgroup waits for another, no atomics, no float sum across threads: a call repeats bit for bit.
#include <cmath>
#include "mm_common.h"

namespace {

constexpr int DS_T = MM_SWEEP_TILE;
constexpr int DS_THREADS = DS_T * DS_T;
static_assert(DS_THREADS == 256, "one thread per tile pixel, four waves");

constexpr int DF_THREADS = 256;
constexpr int DF_WAVES = DF_THREADS / 64;
constexpr int DF_ROUNDS = MM_FILTER_CHUNK / DF_THREADS;
static_assert(MM_FILTER_CHUNK % DF_THREADS == 0, "a chunk is a whole number of rounds");

struct DfK {
    double k[9];
};

// ---------------------------------------------------------------------------------------------------------------- sweep

__global__ __launch_bounds__(256) void ds_column_kernel(const double *__restrict__ AB, const double *__restrict__ w0,
                                                        const double *__restrict__ dw, int V, int S, int D, double *__restrict__ col) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)V * S * D) return;
    const int k = (int)(i % D);
    const int64_t vs = i / D;
    const int v = (int)(vs / S);
    const double wk = w0[v] + (double)k * dw[v];
    const double *ab = AB + vs * 12;
    col[3 * i] = ab[2] + wk * ab[9];
    col[3 * i + 1] = ab[5] + wk * ab[10];
    col[3 * i + 2] = ab[8] + wk * ab[11];
}

__global__ __launch_bounds__(256) void ds_border_kernel(int64_t N, int H, int W, int r, float *__restrict__ depth, float *__restrict__ cost,
                                                        int32_t *__restrict__ plane) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int u = (int)(i % W), v = (int)((i / W) % H);
    if (u >= r && u < W - r && v >= r && v < H - r) return;
    depth[i] = __builtin_nanf("");
    cost[i] = __builtin_nanf("");
    plane[i] = -1;
}

template <int R>
__global__ __launch_bounds__(DS_THREADS) void ds_sweep_kernel(const uint8_t *__restrict__ img, int H, int W, const int32_t *__restrict__ ref,
                                                              const int32_t *__restrict__ src, const double *__restrict__ AB,
                                                              const double *__restrict__ col, const double *__restrict__ w0,
                                                              const double *__restrict__ dw, int S, int D, float var_min_n, int min_sources,
                                                              int tiles_x, float *__restrict__ depth, float *__restrict__ cost,
                                                              int32_t *__restrict__ plane) {
    constexpr int SIDE = DS_T + 2 * R;
    constexpr int NH = SIDE * SIDE;
    constexpr int N = (2 * R + 1) * (2 * R + 1);
    // rows 48 floats apart: the two tile rows a 32-lane group reads (16 lanes each) fall on disjoint halves of the 32 banks
    constexpr int STRIDE = 48;
    static_assert(SIDE <= STRIDE, "a halo row fits its LDS row");
    __shared__ float tile[2][SIDE * STRIDE];

    const int view = blockIdx.y;
    const int tx = threadIdx.x % DS_T, ty = threadIdx.x / DS_T;
    const int hu0 = (blockIdx.x % tiles_x) * DS_T, hv0 = (blockIdx.x / tiles_x) * DS_T;      // image pixel of halo pixel (0, 0)
    const int u = hu0 + R + tx, v = hv0 + R + ty;
    const bool mine = u < W - R && v < H - R;
    const size_t plane_px = (size_t)H * W;
    const float nan = __builtin_nanf("");
    const float nf = (float)N;

    // the reference patch, once; a thread's centred window and saa stay in registers
    const uint8_t *rimg = img + (size_t)ref[view] * plane_px;
    for (int h = threadIdx.x; h < NH; h += DS_THREADS) {
        const int x = hu0 + h % SIDE, y = hv0 + h / SIDE;
        tile[0][(h / SIDE) * STRIDE + h % SIDE] = (x < W && y < H) ? (float)rimg[(size_t)y * W + x] : nan;
    }
    __syncthreads();
    float ca[N];
    float saa = 0.0f;
    bool ref_ok = false;
    if (mine) {
        float sum = 0.0f;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            ca[i] = tile[0][(ty + i / (2 * R + 1)) * STRIDE + tx + i % (2 * R + 1)];
            sum += ca[i];
        }
        const float mean = sum / nf;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            ca[i] = ca[i] - mean;
            saa += ca[i] * ca[i];
        }
        ref_ok = saa > var_min_n;
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) ca[i] = 0.0f;
    }
    __syncthreads();      // (the patch is read: tile[0] is free for the first warped image)

    float best = nan, c_prev = nan, c_minus = nan, c_plus = nan;
    int best_k = -1;
    int buf = 0;
    for (int k = 0; k < D; ++k) {
        float acc = 0.0f;
        int cnt = 0;
        for (int s = 0; s < S; ++s) {
            const int sf = src[(size_t)view * S + s];      // (the same in every thread: all of them reach the barrier)
            if (sf < 0) continue;
            const uint8_t *simg = img + (size_t)sf * plane_px;
            const double *ab = AB + ((size_t)view * S + s) * 12;
            const double *c3 = col + (((size_t)view * S + s) * D + k) * 3;
            const double a00 = ab[0], a01 = ab[1], a10 = ab[3], a11 = ab[4], a20 = ab[6], a21 = ab[7];
            const double c0 = c3[0], c1 = c3[1], c2 = c3[2];
            for (int h = threadIdx.x; h < NH; h += DS_THREADS) {
                const int x = hu0 + h % SIDE, y = hv0 + h / SIDE;
                float val = nan;
                if (x < W && y < H) {
                    const double xd = (double)x, yd = (double)y;
                    const double p0 = (a00 * xd + a01 * yd) + c0;
                    const double p1 = (a10 * xd + a11 * yd) + c1;
                    const double p2 = (a20 * xd + a21 * yd) + c2;
                    const double xs = p0 / p2, ys = p1 / p2;
                    if (p2 > 0.0 && xs >= 0.0 && xs <= (double)(W - 1) && ys >= 0.0 && ys <= (double)(H - 1)) {
                        const double x0 = fmin(floor(xs), (double)(W - 2)), y0 = fmin(floor(ys), (double)(H - 2));
                        const float fx = (float)(xs - x0), fy = (float)(ys - y0);
                        const uint8_t *p = simg + (size_t)(int)y0 * W + (int)x0;
                        const float s00 = (float)p[0], s01 = (float)p[1], s10 = (float)p[W], s11 = (float)p[W + 1];
                        const float top = s00 + fx * (s01 - s00);
                        const float bot = s10 + fx * (s11 - s10);
                        val = top + fy * (bot - top);
                    }
                }
                tile[buf][(h / SIDE) * STRIDE + h % SIDE] = val;
            }
            __syncthreads();      // (one barrier per warped image: the next one goes to the other tile)
            if (ref_ok) {
                float b[N];
                float sum = 0.0f;
#pragma unroll
                for (int i = 0; i < N; ++i) {
                    b[i] = tile[buf][(ty + i / (2 * R + 1)) * STRIDE + tx + i % (2 * R + 1)];
                    sum += b[i];
                }
                const float mean = sum / nf;
                float sbb = 0.0f, sab = 0.0f;
#pragma unroll
                for (int i = 0; i < N; ++i) {
                    const float cb = b[i] - mean;
                    sbb += cb * cb;
                    sab += ca[i] * cb;
                }
                if (sbb > var_min_n) {      // (false for a window with an invalid sample: its sums are NaN)
                    acc += 1.0f - sab / sqrtf(saa * sbb);
                    ++cnt;
                }
            }
            buf ^= 1;
        }
        const float c = cnt >= min_sources ? acc / (float)cnt : nan;      // (cnt >= 1: min_sources is at least 1)
        if (best_k == k - 1 && k > 0) c_plus = c;
        if (c < best || (c == c && best_k < 0)) {
            best = c;
            best_k = k;
            c_minus = c_prev;
            c_plus = nan;
        }
        c_prev = c;
    }
    if (!mine) return;
    const size_t o = (size_t)view * plane_px + (size_t)v * W + u;
    if (best_k < 0) {
        depth[o] = nan;
        cost[o] = nan;
        plane[o] = -1;
        return;
    }
    double delta = 0.0;
    if (best_k > 0 && best_k < D - 1 && c_minus == c_minus && c_plus == c_plus) {
        const double cm = (double)c_minus, cz = (double)best, cp = (double)c_plus;
        const double den = (cm - 2.0 * cz) + cp;
        if (den > 0.0) {
            delta = (cm - cp) / (2.0 * den);
            delta = delta < -0.5 ? -0.5 : (delta > 0.5 ? 0.5 : delta);
        }
    }
    depth[o] = (float)(1.0 / (w0[view] + ((double)best_k + delta) * dw[view]));
    cost[o] = best;
    plane[o] = best_k;
}

inline size_t dd_region(size_t bytes) { return mm_align_up(bytes, 256); }

// ----------------------------------------------------------------------------------------------------------------- fuse

// exclusive prefix of v over the workgroup's threads, in thread order; total = the workgroup's sum (the scan of filter.hip)
__device__ __forceinline__ int df_block_scan(int v, int *sm /*[DF_WAVES]*/, int &total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(inc, off, 64);
        if (lane >= off) inc += t;
    }
    __syncthreads();      // (the previous call's readers are done with sm)
    if (lane == 63) sm[w] = inc;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < DF_WAVES; ++i) {
        const int s = sm[i];
        base += i < w ? s : 0;
        total += s;
    }
    return base + inc - v;
}

struct DfPoint {
    double x, y, z;
};

__device__ __forceinline__ bool df_candidate(const float *__restrict__ depth, const float *__restrict__ cost, size_t i, double max_cost,
                                             double &d) {
    d = (double)depth[i];
    return isfinite(d) && (double)cost[i] <= max_cost;
}

// d K^-1 (u, v, 1) of view `e` taken to the world: X_w = R^T (X_c - t)
__device__ __forceinline__ DfPoint df_lift(const DfK &K, const double *__restrict__ e, double u, double v, double d) {
    const double yn = (v - K.k[5]) / K.k[4];
    const double xn = ((u - K.k[2]) - K.k[1] * yn) / K.k[0];
    const double a = d * xn - e[3], b = d * yn - e[7], c = d - e[11];
    return DfPoint{(e[0] * a + e[4] * b) + e[8] * c, (e[1] * a + e[5] * b) + e[9] * c, (e[2] * a + e[6] * b) + e[10] * c};
}

// Y = R X + t of view `e`; px, py its projection
__device__ __forceinline__ DfPoint df_project(const DfK &K, const double *__restrict__ e, const DfPoint &X, double &px, double &py) {
    const DfPoint Y{((e[0] * X.x + e[1] * X.y) + e[2] * X.z) + e[3], ((e[4] * X.x + e[5] * X.y) + e[6] * X.z) + e[7],
                    ((e[8] * X.x + e[9] * X.y) + e[10] * X.z) + e[11]};
    px = ((K.k[0] * Y.x + K.k[1] * Y.y) + K.k[2] * Y.z) / Y.z;
    py = (K.k[4] * Y.y + K.k[5] * Y.z) / Y.z;
    return Y;
}

__global__ __launch_bounds__(DF_THREADS) void df_test_kernel(const float *__restrict__ depth, const float *__restrict__ cost, int V, int H, int W,
                                                             const double *__restrict__ ext, DfK K, const int32_t *__restrict__ nbr, int Q,
                                                             mm_fuse_params prm, uint8_t *__restrict__ keep, uint8_t *__restrict__ agree,
                                                             int32_t *__restrict__ sums_keep, int32_t *__restrict__ sums_cand) {
    __shared__ int sm[DF_WAVES];
    const int64_t N = (int64_t)V * H * W, npx = (int64_t)H * W;
    const int64_t base = (int64_t)blockIdx.x * MM_FILTER_CHUNK;
    int n_keep = 0, n_cand = 0;
    for (int r = 0; r < DF_ROUNDS; ++r) {
        const int64_t i = base + r * DF_THREADS + threadIdx.x;
        if (i >= N) continue;      // (no shuffle inside this loop)
        const int view = (int)(i / npx);
        const int64_t px = i - (int64_t)view * npx;
        const int v = (int)(px / W), u = (int)(px - (int64_t)v * W);
        double d;
        int n_ok = 0;
        bool kept = false;
        if (df_candidate(depth, cost, (size_t)i, prm.max_cost, d)) {
            ++n_cand;
            const double *ei = ext + (size_t)view * 12;
            const DfPoint Xw = df_lift(K, ei, (double)u, (double)v, d);
            for (int j = 0; j < Q; ++j) {
                const int q = nbr[(size_t)view * Q + j];
                if (q < 0) continue;
                const double *eq = ext + (size_t)q * 12;
                double qx, qy;
                const DfPoint Y = df_project(K, eq, Xw, qx, qy);
                if (!(Y.z > 0.0)) continue;
                const double xi = rint(qx), yi = rint(qy);
                if (!(xi >= 0.0 && xi <= (double)(W - 1) && yi >= 0.0 && yi <= (double)(H - 1))) continue;
                double dq;
                if (!df_candidate(depth, cost, (size_t)q * npx + (size_t)(int)yi * W + (int)xi, prm.max_cost, dq)) continue;
                if (!(fabs(dq - Y.z) <= prm.eps_depth * Y.z)) continue;
                const DfPoint Xq = df_lift(K, eq, xi, yi, dq);
                double bx, by;
                const DfPoint Z = df_project(K, ei, Xq, bx, by);
                if (!(Z.z > 0.0)) continue;
                const double dx = bx - (double)u, dy = by - (double)v;
                if (!(sqrt(dx * dx + dy * dy) <= prm.tau_px)) continue;
                ++n_ok;
            }
            kept = n_ok >= prm.min_consistent;
        }
        keep[i] = kept ? 1 : 0;
        agree[i] = (uint8_t)n_ok;
        n_keep += kept;
    }
    int total_keep, total_cand;
    df_block_scan(n_keep, sm, total_keep);
    df_block_scan(n_cand, sm, total_cand);
    if (threadIdx.x == 0) {
        sums_keep[blockIdx.x] = total_keep;
        sums_cand[blockIdx.x] = total_cand;
    }
}

// workgroup 0 turns sums_keep into exclusive offsets and writes counts[0], workgroup 1 adds up sums_cand into counts[1]
__global__ __launch_bounds__(DF_THREADS) void df_scan_kernel(int32_t *__restrict__ sums_keep, const int32_t *__restrict__ sums_cand, int n,
                                                             int64_t *__restrict__ counts) {
    __shared__ int sm[DF_WAVES];
    const int which = blockIdx.x;
    int64_t carry = 0;
    for (int b0 = 0; b0 < n; b0 += DF_THREADS) {      // (n is the same in every thread: all of them reach the scan)
        const int i = b0 + threadIdx.x;
        const int v = i < n ? (which == 0 ? sums_keep[i] : sums_cand[i]) : 0;
        int total;
        const int ex = df_block_scan(v, sm, total);
        if (which == 0 && i < n) sums_keep[i] = (int32_t)(carry + ex);
        carry += total;
    }
    if (threadIdx.x == 0) counts[which] = carry;
}

__global__ __launch_bounds__(DF_THREADS) void df_emit_kernel(const float *__restrict__ depth, int V, int H, int W, const double *__restrict__ ext,
                                                             DfK K, const uint8_t *__restrict__ grey, const uint8_t *__restrict__ keep,
                                                             const uint8_t *__restrict__ agree, const int32_t *__restrict__ offs, int64_t cap,
                                                             double *__restrict__ points, uint8_t *__restrict__ grey_out,
                                                             int32_t *__restrict__ origin, int32_t *__restrict__ n_consistent) {
    __shared__ int sm[DF_WAVES];
    const int64_t N = (int64_t)V * H * W, npx = (int64_t)H * W;
    const int64_t base = (int64_t)blockIdx.x * MM_FILTER_CHUNK;
    int64_t at = offs[blockIdx.x];
    for (int r = 0; r < DF_ROUNDS; ++r) {
        const int64_t i = base + r * DF_THREADS + threadIdx.x;
        const bool k = i < N && keep[i] != 0;
        int total;
        const int64_t dst = at + df_block_scan(k ? 1 : 0, sm, total);
        if (k && dst < cap) {
            const int view = (int)(i / npx);
            const int64_t px = i - (int64_t)view * npx;
            const int v = (int)(px / W), u = (int)(px - (int64_t)v * W);
            const DfPoint Xw = df_lift(K, ext + (size_t)view * 12, (double)u, (double)v, (double)depth[i]);
            points[3 * dst] = Xw.x;
            points[3 * dst + 1] = Xw.y;
            points[3 * dst + 2] = Xw.z;
            grey_out[dst] = grey[i];
            origin[2 * dst] = view;
            origin[2 * dst + 1] = (int32_t)px;
            n_consistent[dst] = agree[i];
        }
        at += total;
    }
}

__global__ void df_zero_counts_kernel(int64_t *__restrict__ counts) {
    if (threadIdx.x < 2) counts[threadIdx.x] = 0;
}

inline size_t df_chunks(int64_t n) { return n > 0 ? (size_t)((n + MM_FILTER_CHUNK - 1) / MM_FILTER_CHUNK) : 0; }

bool dd_k_ok(const double *K) {
    bool ok = K[3] == 0.0 && K[6] == 0.0 && K[7] == 0.0 && K[8] == 1.0 && K[0] != 0.0 && K[4] != 0.0;
    for (int k = 0; k < 9; ++k) ok = ok && std::isfinite(K[k]);
    return ok;
}

}  // namespace

// the third column of every plane's homography: 3 doubles per (view, source, plane)
extern "C" size_t mm_depth_sweep_workspace_bytes(int V, int S, int D) {
    const size_t nv = V > 0 ? (size_t)V : 0, ns = S > 0 ? (size_t)S : 0, nd = D > 0 ? (size_t)D : 0;
    return dd_region(nv * ns * nd * 3 * sizeof(double));
}

extern "C" int mm_depth_sweep(mm_ctx *ctx, const uint8_t *img, int F, int H, int W, const double *K, const int32_t *ref, const int32_t *src,
                              const double *AB, const double *w0, const double *dw, int V, int S, const mm_sweep_params *prm, float *depth,
                              float *cost, int32_t *plane, void *ws, size_t ws_bytes) {
    // every argument is judged before the context is looked at: nothing below this block runs on a bad call
    if (!prm || !K || F <= 0 || H <= 0 || W <= 0 || V < 0 || S <= 0 || S > MM_SWEEP_MAX_SOURCES)
        return mm_fail(ctx, MM_ERR_ARG, "mm_depth_sweep: bad argument");
    if (prm->planes < 1 || prm->planes > MM_SWEEP_MAX_PLANES || prm->radius < 1 || prm->radius > MM_SWEEP_MAX_RADIUS || prm->min_sources < 1 ||
        prm->min_sources > S)
        return mm_fail(ctx, MM_ERR_ARG, "mm_depth_sweep: planes in 1 .. %d, radius in 1 .. %d and min_sources in 1 .. S expected",
                       MM_SWEEP_MAX_PLANES, MM_SWEEP_MAX_RADIUS);
    if (!(prm->var_min >= 0.0) || !std::isfinite(prm->var_min)) return mm_fail(ctx, MM_ERR_ARG, "mm_depth_sweep: var_min must be finite and >= 0");
    if (!dd_k_ok(K))
        return mm_fail(ctx, MM_ERR_ARG, "mm_depth_sweep: K must be finite and upper triangular with K[8] = 1 and non-zero focal lengths");
    if ((int64_t)F * H * W > INT32_MAX || (int64_t)V * H * W > INT32_MAX) return mm_fail(ctx, MM_ERR_ARG, "mm_depth_sweep: more than 2^31 - 1 pixels");
    if (V > 65535) return mm_fail(ctx, MM_ERR_ARG, "mm_depth_sweep: more than 65535 views");
    if (V > 0 && (!img || !ref || !src || !AB || !w0 || !dw || !depth || !cost || !plane || !ws))
        return mm_fail(ctx, MM_ERR_ARG, "mm_depth_sweep: bad argument");
    if (V > 0 && ws_bytes < mm_depth_sweep_workspace_bytes(V, S, prm->planes))
        return mm_fail(ctx, MM_ERR_WORKSPACE, "mm_depth_sweep: workspace too small");
    if (!ctx) return MM_ERR_ARG;
    if (V == 0) return MM_OK;
    if ((uintptr_t)ws & 7) return mm_fail(ctx, MM_ERR_ARG, "mm_depth_sweep: the workspace must be 8-byte aligned");

    const int D = prm->planes, r = prm->radius;
    const int n = (2 * r + 1) * (2 * r + 1);
    double *col = (double *)ws;
    const int64_t n_col = (int64_t)V * S * D, N = (int64_t)V * H * W;
    MM_LAUNCH(ctx, "ds_column_kernel", ds_column_kernel, dim3((unsigned)((n_col + 255) / 256)), dim3(256), 0, AB, w0, dw, V, S, D, col);
    MM_LAUNCH(ctx, "ds_border_kernel", ds_border_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, N, H, W, r, depth, cost, plane);
    const int iw = W - 2 * r, ih = H - 2 * r;
    if (iw <= 0 || ih <= 0) return MM_OK;
    const int tiles_x = (iw + DS_T - 1) / DS_T, tiles_y = (ih + DS_T - 1) / DS_T;
    const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)V);
    const float var_min_n = (float)prm->var_min * (float)n;
#define DS_GO(R)                                                                                                                        \
    MM_LAUNCH(ctx, "ds_sweep_kernel", ds_sweep_kernel<R>, grid, dim3(DS_THREADS), 0, img, H, W, ref, src, AB, col, w0, dw, S, D, var_min_n, \
              prm->min_sources, tiles_x, depth, cost, plane)
    switch (r) {
        case 1: DS_GO(1); break;
        case 2: DS_GO(2); break;
        case 3: DS_GO(3); break;
        default: DS_GO(4); break;
    }
#undef DS_GO
    return MM_OK;
}

// the views' agreement counts (one byte a pixel) and two arrays of chunk sums
extern "C" size_t mm_depth_fuse_workspace_bytes(int V, int H, int W) {
    const int64_t N = (V > 0 && H > 0 && W > 0) ? (int64_t)V * H * W : 0;
    return dd_region((size_t)N) + 2 * dd_region(df_chunks(N) * sizeof(int32_t));
}

extern "C" int mm_depth_fuse(mm_ctx *ctx, const float *depth, const float *cost, int V, int H, int W, const double *ext, const double *K,
                             const int32_t *nbr, int Q, const uint8_t *grey, const mm_fuse_params *prm, int64_t cap, double *points,
                             uint8_t *grey_out, int32_t *origin, int32_t *n_consistent, uint8_t *keep, int64_t *counts, void *ws,
                             size_t ws_bytes) {
    if (!prm || !K || !counts || V < 0 || H <= 0 || W <= 0 || Q < 0 || Q > MM_FUSE_MAX_NEIGHBOURS || cap < 0)
        return mm_fail(ctx, MM_ERR_ARG, "mm_depth_fuse: bad argument");
    if (std::isnan(prm->max_cost) || !(prm->eps_depth >= 0.0) || !(prm->tau_px >= 0.0) || prm->min_consistent < 0)
        return mm_fail(ctx, MM_ERR_ARG, "mm_depth_fuse: max_cost must be a number, eps_depth and tau_px >= 0 and min_consistent >= 0");
    if (!dd_k_ok(K))
        return mm_fail(ctx, MM_ERR_ARG, "mm_depth_fuse: K must be finite and upper triangular with K[8] = 1 and non-zero focal lengths");
    if ((int64_t)V * H * W > INT32_MAX) return mm_fail(ctx, MM_ERR_ARG, "mm_depth_fuse: more than 2^31 - 1 pixels");
    if (V > 0 && (!depth || !cost || !ext || !grey || !keep || !ws || (Q > 0 && !nbr) ||
                  (cap > 0 && (!points || !grey_out || !origin || !n_consistent))))
        return mm_fail(ctx, MM_ERR_ARG, "mm_depth_fuse: bad argument");
    if (V > 0 && ws_bytes < mm_depth_fuse_workspace_bytes(V, H, W)) return mm_fail(ctx, MM_ERR_WORKSPACE, "mm_depth_fuse: workspace too small");
    if (!ctx) return MM_ERR_ARG;
    if (V == 0) {
        MM_LAUNCH(ctx, "df_zero_counts_kernel", df_zero_counts_kernel, dim3(1), dim3(64), 0, counts);
        return MM_OK;
    }
    if ((uintptr_t)ws & 7) return mm_fail(ctx, MM_ERR_ARG, "mm_depth_fuse: the workspace must be 8-byte aligned");

    const int64_t N = (int64_t)V * H * W;
    const size_t n_ch = df_chunks(N);
    char *w = (char *)ws;
    uint8_t *agree = (uint8_t *)w;
    w += dd_region((size_t)N);
    int32_t *sums_keep = (int32_t *)w;
    w += dd_region(n_ch * sizeof(int32_t));
    int32_t *sums_cand = (int32_t *)w;
    DfK Kv;
    for (int k = 0; k < 9; ++k) Kv.k[k] = K[k];

    MM_LAUNCH(ctx, "df_test_kernel", df_test_kernel, dim3((unsigned)n_ch), dim3(DF_THREADS), 0, depth, cost, V, H, W, ext, Kv, nbr, Q, *prm, keep,
              agree, sums_keep, sums_cand);
    MM_LAUNCH(ctx, "df_scan_kernel", df_scan_kernel, dim3(2), dim3(DF_THREADS), 0, sums_keep, sums_cand, (int)n_ch, counts);
    MM_LAUNCH(ctx, "df_emit_kernel", df_emit_kernel, dim3((unsigned)n_ch), dim3(DF_THREADS), 0, depth, V, H, W, ext, Kv, grey, keep, agree,
              sums_keep, cap, points, grey_out, origin, n_consistent);
    return MM_OK;
}
