// Observation filter at the adjusted solution (mm_filter_observations; gfx950, f64): judge every observation by its
// reprojection error and depth at the cameras and points an adjustment returned, every point by what it has left, and
// compact the problem, order preserved, for the next solve.  include/meatmodeler.h has the definition, operation by operation;
// this file is built without FMA contraction (Makefile), so the bits follow from the expression trees alone and the NumPy
// restatement of tests/test_filter_observations_cpu.py agrees on every comparison of a fixture that keeps its margins.
//
// The call is memory-bound: an observation costs ~56 B read (fi, pi, obs, its point -- shared with its neighbours -- and its
// flags twice more) and ~52 B written (err, depth, flags, the compacted row), the 120-byte camera rows stay in L2.  Seven
// short launches, none of which waits for another workgroup:
//   fl_cam_kernel     per camera   R, t, C = -R^T t                                    -> tab [F, 15]
//   fl_obs_kernel     per obs      err, depth, the observation's own flags
//   fl_pts_kernel     per point    n_ok, cos_parallax, pt_flags; kept points per chunk  -> sums_pt
//   fl_orphan_kernel  per obs      MM_OBS_ORPHAN; kept / own-flagged obs per chunk      -> sums_keep, sums_own
//   fl_scan_kernel    3 workgroups exclusive scan of each sums array in place (one workgroup walks one array), counts
//   fl_emit_pts_kernel, fl_emit_obs_kernel   per chunk: position = chunk offset + rank inside the chunk
// The counts are integers and every float is computed by one thread from its own inputs: there is no float sum across threads,
// no atomic, and a point's verdict depends on the point alone.
#include <cmath>
#include "mm_common.h"
#include "mm_geom.h"

namespace {

constexpr int FL_THREADS = 256;
constexpr int FL_WAVES = FL_THREADS / 64;
constexpr int FL_ROUNDS = MM_FILTER_CHUNK / FL_THREADS;      // a workgroup walks its chunk in rounds of one row per thread
constexpr int FL_CAM = 15;                                   // doubles per camera: R [9] row-major, t [3], C [3]
static_assert(MM_FILTER_CHUNK % FL_THREADS == 0, "a chunk is a whole number of rounds");

struct FlK {
    double k[9];
};

// exclusive prefix of v over the workgroup's threads, in thread order; total = the workgroup's sum.  Every thread calls it.
__device__ __forceinline__ int fl_block_scan(int v, int *sm /*[FL_WAVES]*/, int &total) {
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
    for (int i = 0; i < FL_WAVES; ++i) {
        const int s = sm[i];
        base += i < w ? s : 0;
        total += s;
    }
    return base + inc - v;
}

__global__ __launch_bounds__(FL_THREADS) void fl_cam_kernel(const double *__restrict__ cams, int F, double *__restrict__ tab) {
    const int f = blockIdx.x * FL_THREADS + threadIdx.x;
    if (f >= F) return;
    const double *cm = cams + (size_t)f * 6;
    const double rx = cm[0], ry = cm[1], rz = cm[2], tx = cm[3], ty = cm[4], tz = cm[5];
    const double th2 = (rx * rx + ry * ry) + rz * rz;
    double c, a, b;
    if (th2 < 1e-4) {      // the series of the adjustment's own sweeps (ba_eval.h); a NaN camera takes the other branch
        c = cos(sqrt(th2));
        a = 1.0 + th2 * (-1.0 / 6 + th2 * (1.0 / 120 - th2 * (1.0 / 5040)));
        b = 0.5 + th2 * (-1.0 / 24 + th2 * (1.0 / 720 - th2 * (1.0 / 40320)));
    } else {
        const double th = sqrt(th2);
        const double sh = sin(0.5 * th);
        c = cos(th);
        a = sin(th) / th;
        b = (2.0 * sh * sh) / th2;
    }
    // R = c I + a [r]x + b r r^T
    const double R[9] = {c + b * rx * rx,       -a * rz + b * rx * ry, a * ry + b * rx * rz,
                         a * rz + b * ry * rx,  c + b * ry * ry,       -a * rx + b * ry * rz,
                         -a * ry + b * rz * rx, a * rx + b * rz * ry,  c + b * rz * rz};
    double *t = tab + (size_t)f * FL_CAM;
#pragma unroll
    for (int k = 0; k < 9; ++k) t[k] = R[k];
    t[9] = tx;
    t[10] = ty;
    t[11] = tz;
#pragma unroll
    for (int j = 0; j < 3; ++j) t[12 + j] = -((R[j] * tx + R[3 + j] * ty) + R[6 + j] * tz);
}

// step 1: one thread per observation
__global__ __launch_bounds__(FL_THREADS) void fl_obs_kernel(const double *__restrict__ tab, const double *__restrict__ pts, FlK K,
                                                            const int32_t *__restrict__ fi, const int32_t *__restrict__ pi,
                                                            const double *__restrict__ obs, int64_t O, mm_filter_params prm,
                                                            int32_t *__restrict__ obs_flags, double *__restrict__ err,
                                                            double *__restrict__ depth) {
    const int64_t o = (int64_t)blockIdx.x * FL_THREADS + threadIdx.x;
    if (o >= O) return;
    const double *T = tab + (size_t)fi[o] * FL_CAM;
    const double *Xp = pts + (size_t)pi[o] * 3;
    const Vec3 X{Xp[0], Xp[1], Xp[2]};
    double R[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = T[k];
    const Vec3 RX = mat3(R, X);
    const Vec3 Y{RX.x + T[9], RX.y + T[10], RX.z + T[11]};
    const Vec3 u = mat3(K.k, Y);
    const double2 xy = reinterpret_cast<const double2 *>(obs)[o];
    const double dx = u.x / u.z - xy.x, dy = u.y / u.z - xy.y;
    const double e = sqrt(dx * dx + dy * dy);
    int fl = 0;
    if (!(isfinite(e) && isfinite(Y.z))) fl |= MM_OBS_NONFINITE;
    if (Y.z <= prm.min_depth) fl |= MM_OBS_BEHIND;
    if (e > prm.max_reproj_px) fl |= MM_OBS_REPROJ;
    err[o] = e;
    depth[o] = Y.z;
    obs_flags[o] = fl;
}

// step 2: one thread per point, a workgroup per chunk of points; sums_pt[chunk] = points of the chunk no test flagged
__global__ __launch_bounds__(FL_THREADS) void fl_pts_kernel(const double *__restrict__ tab, const double *__restrict__ pts, int64_t P,
                                                            const int32_t *__restrict__ pt_ptr, const int32_t *__restrict__ fi,
                                                            const int32_t *__restrict__ obs_flags, mm_filter_params prm,
                                                            int32_t *__restrict__ pt_flags, double *__restrict__ cos_parallax,
                                                            int32_t *__restrict__ sums_pt) {
    __shared__ int sm[FL_WAVES];
    const int64_t base = (int64_t)blockIdx.x * MM_FILTER_CHUNK;
    const double inf = __builtin_huge_val();
    int kept = 0;
    for (int r = 0; r < FL_ROUNDS; ++r) {
        const int64_t p = base + r * FL_THREADS + threadIdx.x;
        if (p >= P) continue;      // (no shuffle inside this loop)
        const Vec3 X{pts[3 * p], pts[3 * p + 1], pts[3 * p + 2]};
        const int o_end = pt_ptr[p + 1];
        int n_ok = 0;
        Vec3 a{0.0, 0.0, 0.0};
        double aa = 0.0, cmin = inf;
        for (int o = pt_ptr[p]; o < o_end; ++o) {
            if (obs_flags[o] != 0) continue;
            const double *C = tab + (size_t)fi[o] * FL_CAM + 12;
            const Vec3 b{C[0] - X.x, C[1] - X.y, C[2] - X.z};
            if (n_ok == 0) {
                a = b;
                aa = dot3(a, a);
            } else {
                const double cs = dot3(a, b) / sqrt(aa * dot3(b, b));
                cmin = (cs < cmin || cs != cs) ? cs : cmin;      // (a NaN stays, as in mm_triangulate_tracks)
            }
            ++n_ok;
        }
        const double cp = n_ok < 2 ? __builtin_nan("") : cmin;
        int fl = 0;
        if (!(isfinite(X.x) && isfinite(X.y) && isfinite(X.z))) fl |= MM_PT_NONFINITE;
        if (n_ok < prm.min_views) fl |= MM_PT_SHORT;
        if (cp > prm.max_cos_parallax) fl |= MM_PT_PARALLAX;
        pt_flags[p] = fl;
        cos_parallax[p] = cp;
        kept += fl == 0;
    }
    int total;
    fl_block_scan(kept, sm, total);
    if (threadIdx.x == 0) sums_pt[blockIdx.x] = total;
}

// step 3: an unflagged observation of a dropped point becomes an orphan; kept and own-flagged observations per chunk
__global__ __launch_bounds__(FL_THREADS) void fl_orphan_kernel(const int32_t *__restrict__ pi, const int32_t *__restrict__ pt_flags,
                                                               int64_t O, int32_t *__restrict__ obs_flags,
                                                               int32_t *__restrict__ sums_keep, int32_t *__restrict__ sums_own) {
    __shared__ int sm[FL_WAVES];
    const int64_t base = (int64_t)blockIdx.x * MM_FILTER_CHUNK;
    int keep = 0, own = 0;
    for (int r = 0; r < FL_ROUNDS; ++r) {
        const int64_t o = base + r * FL_THREADS + threadIdx.x;
        if (o >= O) continue;
        if (obs_flags[o] != 0) {
            ++own;
        } else if (pt_flags[pi[o]] != 0) {
            obs_flags[o] = MM_OBS_ORPHAN;
        } else {
            ++keep;
        }
    }
    int total_keep, total_own;
    fl_block_scan(keep, sm, total_keep);
    fl_block_scan(own, sm, total_own);
    if (threadIdx.x == 0) {
        sums_keep[blockIdx.x] = total_keep;
        sums_own[blockIdx.x] = total_own;
    }
}

// the second scan level: workgroup 0 turns sums_keep into exclusive offsets, workgroup 1 sums_pt, workgroup 2 adds up sums_own;
// each walks its array alone, FL_THREADS entries a step, and writes its share of counts
__global__ __launch_bounds__(FL_THREADS) void fl_scan_kernel(int32_t *__restrict__ sums_keep, int32_t *__restrict__ sums_pt,
                                                             const int32_t *__restrict__ sums_own, int n_o, int n_p, int64_t P,
                                                             int64_t *__restrict__ counts) {
    __shared__ int sm[FL_WAVES];
    const int which = blockIdx.x;
    int32_t *s = which == 0 ? sums_keep : sums_pt;
    const int n = which == 1 ? n_p : n_o;
    int carry = 0;
    for (int b0 = 0; b0 < n; b0 += FL_THREADS) {      // (n is the same in every thread: all of them reach the scan)
        const int i = b0 + threadIdx.x;
        const int v = i < n ? (which == 2 ? sums_own[i] : s[i]) : 0;
        int total;
        const int ex = fl_block_scan(v, sm, total);
        if (which != 2 && i < n) s[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) {
        if (which == 0) counts[0] = carry;
        if (which == 1) {
            counts[1] = carry;
            counts[3] = P - carry;
        }
        if (which == 2) counts[2] = carry;
    }
}

// step 4 for points: kept points in input order; pt_new[p] = the new index of point p (unset for a dropped point: no kept
// observation refers to one)
__global__ __launch_bounds__(FL_THREADS) void fl_emit_pts_kernel(const int32_t *__restrict__ pt_flags, int64_t P,
                                                                 const int32_t *__restrict__ offs_pt, int32_t *__restrict__ point_map,
                                                                 int32_t *__restrict__ pt_new) {
    __shared__ int sm[FL_WAVES];
    const int64_t base = (int64_t)blockIdx.x * MM_FILTER_CHUNK;
    int at = offs_pt[blockIdx.x];
    for (int r = 0; r < FL_ROUNDS; ++r) {
        const int64_t p = base + r * FL_THREADS + threadIdx.x;
        const bool keep = p < P && pt_flags[p] == 0;
        int total;
        const int dst = at + fl_block_scan(keep ? 1 : 0, sm, total);
        if (keep) {
            point_map[dst] = (int32_t)p;
            pt_new[p] = dst;
        }
        at += total;
    }
}

// step 4 for observations: kept observations in input order, their points renumbered
__global__ __launch_bounds__(FL_THREADS) void fl_emit_obs_kernel(const int32_t *__restrict__ obs_flags, const int32_t *__restrict__ fi,
                                                                 const int32_t *__restrict__ pi, const double *__restrict__ obs, int64_t O,
                                                                 const int32_t *__restrict__ offs_keep, const int32_t *__restrict__ pt_new,
                                                                 int32_t *__restrict__ fi_out, int32_t *__restrict__ pi_out,
                                                                 double *__restrict__ obs_out, int32_t *__restrict__ obs_map) {
    __shared__ int sm[FL_WAVES];
    const int64_t base = (int64_t)blockIdx.x * MM_FILTER_CHUNK;
    int at = offs_keep[blockIdx.x];
    for (int r = 0; r < FL_ROUNDS; ++r) {
        const int64_t o = base + r * FL_THREADS + threadIdx.x;
        const bool keep = o < O && obs_flags[o] == 0;
        int total;
        const int64_t dst = at + fl_block_scan(keep ? 1 : 0, sm, total);
        if (keep) {
            fi_out[dst] = fi[o];
            pi_out[dst] = pt_new[pi[o]];
            reinterpret_cast<double2 *>(obs_out)[dst] = reinterpret_cast<const double2 *>(obs)[o];
            obs_map[dst] = (int32_t)o;
        }
        at += total;
    }
}

__global__ void fl_zero_counts_kernel(int64_t *__restrict__ counts) {
    if (threadIdx.x < 4) counts[threadIdx.x] = 0;
}

inline size_t fl_chunks(int64_t n) { return n > 0 ? (size_t)((n + MM_FILTER_CHUNK - 1) / MM_FILTER_CHUNK) : 0; }
inline size_t fl_region(size_t bytes) { return mm_align_up(bytes, 256); }

}  // namespace

// the camera table, the new index of every point, three arrays of chunk sums
extern "C" size_t mm_filter_workspace_bytes(int F, int64_t P, int64_t O) {
    const size_t nf = F > 0 ? (size_t)F : 0, np = P > 0 ? (size_t)P : 0;
    return fl_region(nf * FL_CAM * sizeof(double)) + fl_region(np * sizeof(int32_t)) + 2 * fl_region(fl_chunks(O) * sizeof(int32_t)) +
           fl_region(fl_chunks(P) * sizeof(int32_t));
}

extern "C" int mm_filter_observations(mm_ctx *ctx, const double *cams, int F, const double *pts, int64_t P, const double *K,
                                      const int32_t *fi, const int32_t *pi, const double *obs, int64_t O, const int32_t *pt_ptr,
                                      const mm_filter_params *prm, int32_t *obs_flags, double *err, double *depth, int32_t *pt_flags,
                                      double *cos_parallax, int32_t *fi_out, int32_t *pi_out, double *obs_out, int32_t *obs_map,
                                      int32_t *point_map, int64_t *counts, void *ws, size_t ws_bytes) {
    // every argument is judged before the context is looked at: nothing below this block runs on a bad call
    if (!prm || !K || !counts || F < 0 || P < 0 || O < 0 || O > INT32_MAX || P >= INT32_MAX)
        return mm_fail(ctx, MM_ERR_ARG, "mm_filter_observations: bad argument");
    if (prm->min_views < 2) return mm_fail(ctx, MM_ERR_ARG, "mm_filter_observations: min_views must be at least 2");
    if (std::isnan(prm->max_reproj_px) || std::isnan(prm->min_depth) || std::isnan(prm->max_cos_parallax))
        return mm_fail(ctx, MM_ERR_ARG, "mm_filter_observations: a threshold is not a number");
    bool k_ok = K[3] == 0.0 && K[6] == 0.0 && K[7] == 0.0 && K[8] == 1.0 && K[0] != 0.0 && K[4] != 0.0;
    for (int k = 0; k < 9; ++k) k_ok = k_ok && std::isfinite(K[k]);
    if (!k_ok)
        return mm_fail(ctx, MM_ERR_ARG, "mm_filter_observations: K must be finite and upper triangular with K[8] = 1 and non-zero focal lengths");
    const bool work = O > 0 && P > 0;
    if (work && (F <= 0 || !cams || !pts || !fi || !pi || !obs || !pt_ptr || !obs_flags || !err || !depth || !pt_flags || !cos_parallax ||
                 !fi_out || !pi_out || !obs_out || !obs_map || !point_map || !ws))
        return mm_fail(ctx, MM_ERR_ARG, "mm_filter_observations: bad argument");
    if (work && ws_bytes < mm_filter_workspace_bytes(F, P, O))
        return mm_fail(ctx, MM_ERR_WORKSPACE, "mm_filter_observations: workspace too small");
    if (!ctx) return MM_ERR_ARG;
    if (!work) {
        MM_LAUNCH(ctx, "fl_zero_counts_kernel", fl_zero_counts_kernel, dim3(1), dim3(64), 0, counts);
        return MM_OK;
    }
    if (((uintptr_t)obs | (uintptr_t)obs_out) & 15) return mm_fail(ctx, MM_ERR_ARG, "mm_filter_observations: obs and obs_out must be 16-byte aligned");
    if ((uintptr_t)ws & 7) return mm_fail(ctx, MM_ERR_ARG, "mm_filter_observations: the workspace must be 8-byte aligned");

    const size_t n_o = fl_chunks(O), n_p = fl_chunks(P);
    char *w = (char *)ws;
    double *tab = (double *)w;
    w += fl_region((size_t)F * FL_CAM * sizeof(double));
    int32_t *pt_new = (int32_t *)w;
    w += fl_region((size_t)P * sizeof(int32_t));
    int32_t *sums_keep = (int32_t *)w;
    w += fl_region(n_o * sizeof(int32_t));
    int32_t *sums_own = (int32_t *)w;
    w += fl_region(n_o * sizeof(int32_t));
    int32_t *sums_pt = (int32_t *)w;
    FlK Kv;
    for (int k = 0; k < 9; ++k) Kv.k[k] = K[k];

    MM_LAUNCH(ctx, "fl_cam_kernel", fl_cam_kernel, dim3((unsigned)((F + FL_THREADS - 1) / FL_THREADS)), dim3(FL_THREADS), 0, cams, F, tab);
    MM_LAUNCH(ctx, "fl_obs_kernel", fl_obs_kernel, dim3((unsigned)((O + FL_THREADS - 1) / FL_THREADS)), dim3(FL_THREADS), 0, tab, pts, Kv,
              fi, pi, obs, O, *prm, obs_flags, err, depth);
    MM_LAUNCH(ctx, "fl_pts_kernel", fl_pts_kernel, dim3((unsigned)n_p), dim3(FL_THREADS), 0, tab, pts, P, pt_ptr, fi, obs_flags, *prm,
              pt_flags, cos_parallax, sums_pt);
    MM_LAUNCH(ctx, "fl_orphan_kernel", fl_orphan_kernel, dim3((unsigned)n_o), dim3(FL_THREADS), 0, pi, pt_flags, O, obs_flags, sums_keep,
              sums_own);
    MM_LAUNCH(ctx, "fl_scan_kernel", fl_scan_kernel, dim3(3), dim3(FL_THREADS), 0, sums_keep, sums_pt, sums_own, (int)n_o, (int)n_p, P,
              counts);
    MM_LAUNCH(ctx, "fl_emit_pts_kernel", fl_emit_pts_kernel, dim3((unsigned)n_p), dim3(FL_THREADS), 0, pt_flags, P, sums_pt, point_map,
              pt_new);
    MM_LAUNCH(ctx, "fl_emit_obs_kernel", fl_emit_obs_kernel, dim3((unsigned)n_o), dim3(FL_THREADS), 0, obs_flags, fi, pi, obs, O, sums_keep,
              pt_new, fi_out, pi_out, obs_out, obs_map);
    return MM_OK;
}
