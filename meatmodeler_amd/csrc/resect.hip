// Camera registration against existing 3-D points: a RANSAC resection (PnP) per camera (gfx950, f64).
//
// Reference counterpart: the pose source cv2.solvePnP(..., SOLVEPNP_ITERATIVE) at processor.py:175 -- there on a chessboard,
// here on whatever points the camera observes, robustly.  The definition -- usable rows, normalisation, sampling, the reduced
// DLT, MSAC score, refit, polish, flags -- is in include/meatmodeler.h (mm_resect_cameras); this file maps it:
//   rs_prepare_kernel     one workgroup per camera: the usable rows compacted in order (ballot / popcount prefix), centroid and
//                         scale of their points
//   rs_hypothesis_kernel  one lane per (camera, hypothesis): six sampled rows summed into the 40 numbers of the reduced DLT, both
//                         factorisations and both Jacobis in registers (every index static, nothing in scratch)
//   rs_score_kernel       lane = hypothesis, K [R|t] in twelve registers; the camera's rows go through LDS in tiles and every
//                         lane reads the same address (broadcast), summing min(d^2, tau^2) over the rows ascending
//   rs_finish_kernel      one workgroup per camera: argmin, the prior, refit rounds, Levenberg-Marquardt polish, mask, outputs
// and the planar branch (mm_resect_planar: coplanar points, where the reduced DLT above has no valid sample), which shares the
// score kernel, the workspace slots and the finish stage:
//   rp_prepare_kernel     one workgroup per camera: the same compaction, then the plane through the points (six sums, 3 x 3
//                         Jacobi), the verdict -- planar, collinear, refused -- and the camera's frame e1, e2, n
//   rp_hypothesis_kernel  one lane per (camera, hypothesis): four sampled rows in plane coordinates, near-collinear triples
//                         rejected, the 24 sums of the same DLT one dimension down, the pose from the homography
//   rs_finish_kernel<true>  the finish stage with the verdict in front and the homography refit in the place of the DLT's
// Built without FMA contraction (Makefile): a product-sum then has one value whatever the compiler makes of its surroundings,
// and the NumPy restatement of the tests can follow the header operation by operation.  Plain f64 VALU work; sums in an order
// that depends on the camera alone (per-thread strides, xor butterflies, waves in order), no atomics.
#include "mm_common.h"
#include "mm_geom.h"

namespace {

constexpr int RS_THREADS = 256;      // prepare / finish: one workgroup per camera
constexpr int RS_WAVES = RS_THREADS / 64;
constexpr int RS_TILE = 256;         // rows per LDS tile of the score kernel
static_assert(RS_THREADS == MM_BLOCK_THREADS, "the mm_block_* helpers are written for this workgroup");

struct RsArgs {
    const double *X, *obs;
    const int32_t *pi, *cam_ptr, *cam_obs;
    const uint8_t *pt_ok;
    const double *prior;
    long long P, O, n_rows;
    int n_cams, n_hyp, min_rows, min_inliers, refit_iters, polish_iters;
    uint32_t seed, cam_base;
    double tau2;
    double K[9];
    double Ki[5];      // K^-1 = [[Ki0, Ki1, Ki2], [0, Ki3, Ki4], [0, 0, 1]]
    double *norm;      // [n_cams, 8]: cx, cy, cz, s, n_use, number of malformed rows, -, -
                       // (mm_resect_planar: slot 4 is n_use where the homography branch runs, else 0; 6: n_use; 7: verdict flags)
    double *frame;     // mm_resect_planar only, [n_cams, 9]: e1, e2, n of the fitted plane
    double *plane;     // mm_resect_planar only, the output [n_cams, 6]
    double planar_tol2, collinear_tol;
    double *Eh;        // [n_cams, n_hyp, 12] (NaN: invalid hypothesis)
    double *cost_h;    // [n_cams, n_hyp] (+inf: invalid hypothesis)
    int32_t *rows;     // [n_rows]: the usable observations of camera c at cam_ptr[c] .. + n_use, in order
    uint8_t *mask;     // [n_rows]: the polish set, by compacted row
    double *ext, *cost;
    uint8_t *inlier;
    int32_t *info;
};

// rows of camera c in cam_obs, clamped to the array: nothing is read outside it whatever cam_ptr holds
__device__ __forceinline__ void rs_range(const RsArgs &a, int c, int &lo, int &hi) {
    long long l = a.cam_ptr[c], h = a.cam_ptr[c + 1];
    l = l < 0 ? 0 : (l > a.n_rows ? a.n_rows : l);
    h = h < l ? l : (h > a.n_rows ? a.n_rows : h);
    lo = (int)l;
    hi = (int)h;
}

// compacted row k of the camera whose rows start at lo (validated by the prepare kernel)
__device__ __forceinline__ void rs_load(const RsArgs &a, int lo, int k, double &X, double &Y, double &Z, double &ox, double &oy) {
    const int o = a.rows[lo + k];
    const int p = a.pi[o];
    X = a.X[3 * (size_t)p];
    Y = a.X[3 * (size_t)p + 1];
    Z = a.X[3 * (size_t)p + 2];
    ox = a.obs[2 * (size_t)o];
    oy = a.obs[2 * (size_t)o + 1];
}

// one row into the 40 sums: S, Bu, Bv, C, each the upper triangle of a 4 x 4, row-major
__device__ __forceinline__ void rs_accumulate(double (&acc)[40], const RsArgs &a, double cx, double cy, double cz, double s,
                                              double X, double Y, double Z, double ox, double oy) {
    const double x[4] = {s * (X - cx), s * (Y - cy), s * (Z - cz), 1.0};
    const double u = (a.Ki[0] * ox + a.Ki[1] * oy) + a.Ki[2], v = a.Ki[3] * oy + a.Ki[4];
    const double r2 = u * u + v * v;
    int k = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = i; j < 4; ++j) {
            const double w = x[i] * x[j];
            acc[k] += w;
            acc[10 + k] += u * w;
            acc[20 + k] += v * w;
            acc[30 + k] += r2 * w;
            ++k;
        }
}

// the reduced DLT: [R|t] from the 40 sums; false: a failed pivot, a non-positive eigenvalue or a non-finite result
__device__ __forceinline__ bool rs_solve(const double (&acc)[40], double cx, double cy, double cz, double s, double (&E)[12]) {
    double S[4][4], Bu[4][4], Bv[4][4], M[4][4];
    {
        int k = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = i; j < 4; ++j) {
                S[i][j] = S[j][i] = acc[k];
                Bu[i][j] = Bu[j][i] = acc[10 + k];
                Bv[i][j] = Bv[j][i] = acc[20 + k];
                M[i][j] = M[j][i] = acc[30 + k];
                ++k;
            }
    }
    bool ok = true;
    double L[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double d = S[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
        ok = ok && isfinite(d) && d > 1e-12 * S[j][j];
        const double ljj = sqrt(d);
        L[j][j] = ljj;
#pragma unroll
        for (int i = j + 1; i < 4; ++i) {
            double v = S[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
            L[i][j] = v / ljj;
        }
    }
    double Yu[4][4], Yv[4][4];      // L^-1 Bu, L^-1 Bv
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            double vu = Bu[i][c], vv = Bv[i][c];
#pragma unroll
            for (int k = 0; k < i; ++k) {
                vu -= L[i][k] * Yu[k][c];
                vv -= L[i][k] * Yv[k][c];
            }
            Yu[i][c] = vu / L[i][i];
            Yv[i][c] = vv / L[i][i];
        }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = i; j < 4; ++j) {
            const double tu = ((Yu[0][i] * Yu[0][j] + Yu[1][i] * Yu[1][j]) + Yu[2][i] * Yu[2][j]) + Yu[3][i] * Yu[3][j];
            const double tv = ((Yv[0][i] * Yv[0][j] + Yv[1][i] * Yv[1][j]) + Yv[2][i] * Yv[2][j]) + Yv[3][i] * Yv[3][j];
            M[i][j] = M[j][i] = (M[i][j] - tu) - tv;
        }
    double V4[4][4];
    mm_identity<4>(V4);
    mm_jacobi<4>(M, V4);
    double ev = M[0][0], p3[4] = {V4[0][0], V4[1][0], V4[2][0], V4[3][0]};      // smallest eigenvalue, ties to the lowest column
#pragma unroll
    for (int c = 1; c < 4; ++c) {
        if (M[c][c] < ev) {
            ev = M[c][c];
#pragma unroll
            for (int r = 0; r < 4; ++r) p3[r] = V4[r][c];
        }
    }
    double p1[4], p2[4];      // S^-1 Bu p3 = L^-T (Yu p3), S^-1 Bv p3
    {
        double wu[4], wv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            wu[i] = ((Yu[i][0] * p3[0] + Yu[i][1] * p3[1]) + Yu[i][2] * p3[2]) + Yu[i][3] * p3[3];
            wv[i] = ((Yv[i][0] * p3[0] + Yv[i][1] * p3[1]) + Yv[i][2] * p3[2]) + Yv[i][3] * p3[3];
        }
#pragma unroll
        for (int i = 3; i >= 0; --i) {
            double vu = wu[i], vv = wv[i];
#pragma unroll
            for (int k = i + 1; k < 4; ++k) {
                vu -= L[k][i] * p1[k];
                vv -= L[k][i] * p2[k];
            }
            p1[i] = vu / L[i][i];
            p2[i] = vv / L[i][i];
        }
    }
    // P = [p1; p2; p3] T, T = [[s I, -s c], [0, 1]]: A = P[:, :3]; the translation is taken about the centroid (below)
    double A[3][3], b[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        A[0][c] = s * p1[c];
        A[1][c] = s * p2[c];
        A[2][c] = s * p3[c];
    }
    b[0] = p1[3];
    b[1] = p2[3];
    b[2] = p3[3];
    const double det = (A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0])) +
                       A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]);
    if (det < 0.0) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            b[r] = -b[r];
#pragma unroll
            for (int c = 0; c < 3; ++c) A[r][c] = -A[r][c];
        }
    }
    double G[3][3], V[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) G[r][c] = (A[0][r] * A[0][c] + A[1][r] * A[1][c]) + A[2][r] * A[2][c];
    mm_identity<3>(V);
    mm_jacobi<3>(G, V);
    double dk[3], sig = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double lam = G[k][k];
        ok = ok && isfinite(lam) && lam > 0.0;
        const double rt = sqrt(lam);
        dk[k] = 1.0 / rt;
        sig = (k == 0) ? rt : sig + rt;
    }
    sig = sig / 3.0;
    double W[3][3];      // V diag(lambda^-1/2) V^T
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) W[i][j] = ((V[i][0] * dk[0]) * V[j][0] + (V[i][1] * dk[1]) * V[j][1]) + (V[i][2] * dk[2]) * V[j][2];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) E[4 * r + c] = (A[r][0] * W[0][c] + A[r][1] * W[1][c]) + A[r][2] * W[2][c];
        E[4 * r + 3] = b[r] / sig - ((E[4 * r] * cx + E[4 * r + 1] * cy) + E[4 * r + 2] * cz);
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) ok = ok && isfinite(E[k]);
    return ok;
}

// Q = K [R|t], every dot product summed left to right
__device__ __forceinline__ void rs_camera(const RsArgs &a, const double (&E)[12], double (&Q)[12]) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) Q[4 * r + c] = (a.K[3 * r] * E[c] + a.K[3 * r + 1] * E[4 + c]) + a.K[3 * r + 2] * E[8 + c];
}

// squared pixel distance of the projection to the observation; true: an inlier (in front, d^2 finite and <= tau^2)
__device__ __forceinline__ bool rs_distance(const double (&Q)[12], double X, double Y, double Z, double ox, double oy, double tau2,
                                            double &d2) {
    const double y0 = ((Q[0] * X + Q[1] * Y) + Q[2] * Z) + Q[3];
    const double y1 = ((Q[4] * X + Q[5] * Y) + Q[6] * Z) + Q[7];
    const double y2 = ((Q[8] * X + Q[9] * Y) + Q[10] * Z) + Q[11];
    const double ex = y0 / y2 - ox, ey = y1 / y2 - oy;
    d2 = ex * ex + ey * ey;
    return y2 > 0.0 && isfinite(d2) && d2 <= tau2;
}

// ---- the planar branch (mm_resect_planar): the reduced DLT one dimension down ----------------------------------------------
// plane coordinates (ma, mb) = s ((X - c) . e1, (X - c) . e2) of a point and the calibrated pixel (u, v); fr = e1, e2, n
__device__ __forceinline__ void rp_row(const RsArgs &a, const double (&fr)[9], double cx, double cy, double cz, double s, double X,
                                       double Y, double Z, double ox, double oy, double &ma, double &mb, double &u, double &v) {
    const double dx = X - cx, dy = Y - cy, dz = Z - cz;
    ma = s * ((dx * fr[0] + dy * fr[1]) + dz * fr[2]);
    mb = s * ((dx * fr[3] + dy * fr[4]) + dz * fr[5]);
    u = (a.Ki[0] * ox + a.Ki[1] * oy) + a.Ki[2];
    v = a.Ki[3] * oy + a.Ki[4];
}

// [R|t] from the 24 sums: the homography H = [h1; h2; h3] by the reduced DLT, then the pose of the plane's frame fr = e1, e2, n
// about the centroid.  false: a failed pivot, a non-positive eigenvalue or a non-finite result.
__device__ __forceinline__ bool rp_solve(const double (&acc)[24], const double (&fr)[9], double cx, double cy, double cz, double s,
                                         double (&E)[12]) {
    double h1[3], h2[3], h3[3];
    bool ok = mm_plane_dlt(acc, h1, h2, h3);
    const double sg = h3[2] < 0.0 ? -1.0 : 1.0;      // H[2][2] >= 0: the centroid in front
    const double g1[3] = {sg * h1[0], sg * h2[0], sg * h3[0]}, g2[3] = {sg * h1[1], sg * h2[1], sg * h3[1]};
    const double g3[3] = {sg * h1[2], sg * h2[2], sg * h3[2]};
    const double sigma = (sqrt((g1[0] * g1[0] + g1[1] * g1[1]) + g1[2] * g1[2]) + sqrt((g2[0] * g2[0] + g2[1] * g2[1]) + g2[2] * g2[2])) / 2.0;
    double g12[3];
    mm_cross3(g1, g2, g12);
    double A[3][3], Rp[3][3], rt[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        A[r][0] = g1[r];
        A[r][1] = g2[r];
        A[r][2] = g12[r] / sigma;
    }
    ok = mm_polar3(A, Rp, rt) && ok;
    {   // a homography of rank one or two (every pixel the same, or on a line) has no pose: its polar factor is no rotation
        double lo_ = rt[0] < rt[1] ? rt[0] : rt[1], hi_ = rt[0] > rt[1] ? rt[0] : rt[1];
        lo_ = lo_ < rt[2] ? lo_ : rt[2];
        hi_ = hi_ > rt[2] ? hi_ : rt[2];
        ok = ok && lo_ > 1e-4 * hi_;
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) E[4 * r + c] = (Rp[r][0] * fr[c] + Rp[r][1] * fr[3 + c]) + Rp[r][2] * fr[6 + c];
        E[4 * r + 3] = g3[r] / (sigma * s) - ((E[4 * r] * cx + E[4 * r + 1] * cy) + E[4 * r + 2] * cz);
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) ok = ok && isfinite(E[k]);
    return ok;
}

// ---- usable rows, centroid and scale ----------------------------------------------------------------------------------------
// row q of a camera: its observation o; mal: an index out of range or a non-finite pixel; use: a usable row; mark: o is in
// range and the row is usable or malformed (the rows whose inlier byte a call writes).  Nothing is read through a bad index.
__device__ __forceinline__ void rs_classify(const RsArgs &a, int q, int &o, bool &mal, bool &mark, bool &use) {
    o = a.cam_obs[q];
    mal = !(o >= 0 && (long long)o < a.O);
    use = false;
    mark = false;
    if (!mal) {
        const int p = a.pi[o];
        const double ox = a.obs[2 * (size_t)o], oy = a.obs[2 * (size_t)o + 1];
        mal = !(p >= 0 && (long long)p < a.P) || !(isfinite(ox) && isfinite(oy));
        if (!mal && (a.pt_ok == nullptr || a.pt_ok[p] != 0))
            use = isfinite(a.X[3 * (size_t)p]) && isfinite(a.X[3 * (size_t)p + 1]) && isfinite(a.X[3 * (size_t)p + 2]);
        mark = mal || use;
    }
}

// the usable rows of the camera compacted in order into a.rows[lo ..]; n_use: their number (uniform), bad: this thread's
// malformed rows.  MARK: the inlier byte of every usable or malformed row is zeroed on the way.
template <bool MARK>
__device__ __forceinline__ void rs_compact_rows(const RsArgs &a, int lo, int hi, int *wcount, int &n_use, int &bad) {
    const int tid = threadIdx.x;
    n_use = 0;
    bad = 0;
    for (int q0 = lo; q0 < hi; q0 += RS_THREADS) {
        const int q = q0 + tid;
        bool use = false;
        int o = 0;
        if (q < hi) {
            bool mal, mark;
            rs_classify(a, q, o, mal, mark, use);
            if (MARK && mark) a.inlier[o] = 0;
            bad += mal ? 1 : 0;
        }
        const int at = mm_block_compact_slot(use, n_use, wcount);
        if (use) a.rows[lo + at] = o;
    }
}

__global__ __launch_bounds__(RS_THREADS) void rs_prepare_kernel(RsArgs a) {
    __shared__ double sm[RS_WAVES * 3];
    __shared__ int wcount[RS_WAVES], wbad[RS_WAVES];
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int lo, hi;
    rs_range(a, c, lo, hi);
    int n_use, bad;
    rs_compact_rows<true>(a, lo, hi, wcount, n_use, bad);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) bad += __shfl_xor(bad, off, 64);
    if (lane == 0) wbad[wave] = bad;
    __syncthreads();      // (also publishes rows to the whole workgroup)
    bad = wbad[0] + wbad[1] + wbad[2] + wbad[3];
    double s3[3] = {0.0, 0.0, 0.0};
    for (int k = tid; k < n_use; k += RS_THREADS) {
        double X, Y, Z, ox, oy;
        rs_load(a, lo, k, X, Y, Z, ox, oy);
        s3[0] += X;
        s3[1] += Y;
        s3[2] += Z;
    }
    mm_block_sum<3>(s3, sm);
    const double n = (double)n_use, cx = s3[0] / n, cy = s3[1] / n, cz = s3[2] / n;
    double dd[1] = {0.0};
    for (int k = tid; k < n_use; k += RS_THREADS) {
        double X, Y, Z, ox, oy;
        rs_load(a, lo, k, X, Y, Z, ox, oy);
        dd[0] += sqrt(((X - cx) * (X - cx) + (Y - cy) * (Y - cy)) + (Z - cz) * (Z - cz));
    }
    mm_block_sum<1>(dd, sm);
    if (tid == 0) {
        double *o = a.norm + 8 * (size_t)c;
        o[0] = cx;
        o[1] = cy;
        o[2] = cz;
        o[3] = 1.7320508075688772 / (dd[0] / n);
        o[4] = n;
        o[5] = (double)bad;
        o[6] = 0.0;
        o[7] = 0.0;
    }
}

// mm_resect_planar: the usable rows, the plane through them, the verdict and the header (norm, frame) of the camera
__global__ __launch_bounds__(RS_THREADS) void rp_prepare_kernel(RsArgs a) {
    __shared__ double sm[RS_WAVES * 6];
    __shared__ int wcount[RS_WAVES], wbad[RS_WAVES];
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int lo, hi;
    rs_range(a, c, lo, hi);
    int n_use, bad;
    rs_compact_rows<false>(a, lo, hi, wcount, n_use, bad);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) bad += __shfl_xor(bad, off, 64);
    if (lane == 0) wbad[wave] = bad;
    __syncthreads();      // (also publishes rows to the whole workgroup)
    bad = wbad[0] + wbad[1] + wbad[2] + wbad[3];
    double s3[3] = {0.0, 0.0, 0.0};
    for (int k = tid; k < n_use; k += RS_THREADS) {
        double X, Y, Z, ox, oy;
        rs_load(a, lo, k, X, Y, Z, ox, oy);
        s3[0] += X;
        s3[1] += Y;
        s3[2] += Z;
    }
    mm_block_sum<3>(s3, sm);
    const double n = (double)n_use, cx = s3[0] / n, cy = s3[1] / n, cz = s3[2] / n;
    double cv[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};      // (X - c)(X - c)^T, upper triangle row-major
    for (int k = tid; k < n_use; k += RS_THREADS) {
        double X, Y, Z, ox, oy;
        rs_load(a, lo, k, X, Y, Z, ox, oy);
        const double dx = X - cx, dy = Y - cy, dz = Z - cz;
        cv[0] += dx * dx;
        cv[1] += dx * dy;
        cv[2] += dx * dz;
        cv[3] += dy * dy;
        cv[4] += dy * dz;
        cv[5] += dz * dz;
    }
    mm_block_sum<6>(cv, sm);
    double G[3][3] = {{cv[0], cv[1], cv[2]}, {cv[1], cv[3], cv[4]}, {cv[2], cv[4], cv[5]}}, V[3][3];
    mm_identity<3>(V);
    mm_jacobi<3>(G, V);
    // eigenpairs ascending by a stable exchange sort of the three columns: (0, 1), (1, 2), (0, 1), each only on a strictly
    // smaller right neighbour
    double l[3] = {G[0][0], G[1][1], G[2][2]};
#define RP_EXCHANGE(i, j)                     \
    if (l[j] < l[i]) {                        \
        const double t_ = l[i];               \
        l[i] = l[j];                          \
        l[j] = t_;                            \
        _Pragma("unroll") for (int r = 0; r < 3; ++r) { \
            const double w_ = V[r][i];        \
            V[r][i] = V[r][j];                \
            V[r][j] = w_;                     \
        }                                     \
    }
    RP_EXCHANGE(0, 1)
    RP_EXCHANGE(1, 2)
    RP_EXCHANGE(0, 1)
#undef RP_EXCHANGE
    const double nrm[3] = {V[0][0], V[1][0], V[2][0]}, e1[3] = {V[0][2], V[1][2], V[2][2]};
    double e2[3];
    mm_cross3(nrm, e1, e2);
    int verdict = 0;
    bool runs = false;
    if (n_use < a.min_rows) {
        verdict = MM_RESECT_TOO_FEW;
    } else if (!(isfinite(l[2]) && l[2] > 0.0) || !(l[1] > 1e-12 * l[2])) {
        verdict = MM_RESECT_PLANAR | MM_RESECT_NO_MODEL;      // collinear (or no finite extent at all)
    } else if (l[0] <= a.planar_tol2 * l[1]) {
        verdict = MM_RESECT_PLANAR;
        runs = true;
    }
    double dd[1] = {0.0};
    for (int k = tid; k < n_use; k += RS_THREADS) {
        double X, Y, Z, ox, oy;
        rs_load(a, lo, k, X, Y, Z, ox, oy);
        const double dx = X - cx, dy = Y - cy, dz = Z - cz;
        const double pa = (dx * e1[0] + dy * e1[1]) + dz * e1[2], pb = (dx * e2[0] + dy * e2[1]) + dz * e2[2];
        dd[0] += sqrt(pa * pa + pb * pb);
    }
    mm_block_sum<1>(dd, sm);
    if (verdict & MM_RESECT_PLANAR) {      // the rows this call writes: as rs_prepare_kernel does for every camera
        for (int q = lo + tid; q < hi; q += RS_THREADS) {
            int o;
            bool mal, mark, use;
            rs_classify(a, q, o, mal, mark, use);
            if (mark) a.inlier[o] = 0;
        }
    }
    if (tid == 0) {
        double *o = a.norm + 8 * (size_t)c;
        o[0] = cx;
        o[1] = cy;
        o[2] = cz;
        o[3] = 1.4142135623730951 / (dd[0] / n);
        o[4] = runs ? n : 0.0;
        o[5] = (double)bad;
        o[6] = n;
        o[7] = (double)verdict;
        double *f = a.frame + 9 * (size_t)c, *p = a.plane + 6 * (size_t)c;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            f[k] = e1[k];
            f[3 + k] = e2[k];
            f[6 + k] = nrm[k];
            p[k] = nrm[k];
        }
        p[3] = (nrm[0] * cx + nrm[1] * cy) + nrm[2] * cz;
        p[4] = sqrt((l[0] > 0.0 ? l[0] : 0.0) / l[1]);
        p[5] = sqrt(l[1] / l[2]);
    }
}

// ---- one hypothesis per lane --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void rs_hypothesis_kernel(RsArgs a) {
    const int c = blockIdx.x;
    const int h = blockIdx.y * 64 + threadIdx.x;
    const double *nr = a.norm + 8 * (size_t)c;
    const int n_use = (int)nr[4];
    if (h >= a.n_hyp || n_use < a.min_rows) return;      // (a camera with too few rows is never scored either)
    int lo, hi;
    rs_range(a, c, lo, hi);
    const double cx = nr[0], cy = nr[1], cz = nr[2], s = nr[3];
    bool ok = isfinite(s) && isfinite(cx) && isfinite(cy) && isfinite(cz);
    // six distinct rows, integer arithmetic only
    const uint32_t base = mm_pcg(mm_pcg(a.seed + mm_pcg(a.cam_base + (uint32_t)c)) + (uint32_t)h);
    int pick[6];
    ok = mm_sample_distinct<6>(base, n_use, pick) && ok;
    double acc[40];
#pragma unroll
    for (int k = 0; k < 40; ++k) acc[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        double X, Y, Z, ox, oy;
        rs_load(a, lo, pick[k], X, Y, Z, ox, oy);
        rs_accumulate(acc, a, cx, cy, cz, s, X, Y, Z, ox, oy);
    }
    double E[12];
    ok = rs_solve(acc, cx, cy, cz, s, E) && ok;
    double *o = a.Eh + ((size_t)c * a.n_hyp + h) * 12;
    const double nan = __builtin_nan("");
#pragma unroll
    for (int k = 0; k < 12; ++k) o[k] = ok ? E[k] : nan;
}

// mm_resect_planar: four sampled rows, the near-collinear triples rejected, the 24 sums and the pose from the homography
__global__ __launch_bounds__(64) void rp_hypothesis_kernel(RsArgs a) {
    const int c = blockIdx.x;
    const int h = blockIdx.y * 64 + threadIdx.x;
    const double *nr = a.norm + 8 * (size_t)c;
    const int n_use = (int)nr[4];
    if (h >= a.n_hyp || n_use < a.min_rows) return;      // (a refused camera is never scored either)
    int lo, hi;
    rs_range(a, c, lo, hi);
    const double cx = nr[0], cy = nr[1], cz = nr[2], s = nr[3];
    double fr[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) fr[k] = a.frame[9 * (size_t)c + k];
    bool ok = isfinite(s) && isfinite(cx) && isfinite(cy) && isfinite(cz);
    const uint32_t base = mm_pcg(mm_pcg(a.seed + mm_pcg(a.cam_base + (uint32_t)c)) + (uint32_t)h);
    int pick[4];
    ok = mm_sample_distinct<4>(base, n_use, pick) && ok;
    double ma[4], mb[4], acc[24];
#pragma unroll
    for (int k = 0; k < 24; ++k) acc[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        double X, Y, Z, ox, oy, u, v;
        rs_load(a, lo, pick[k], X, Y, Z, ox, oy);
        rp_row(a, fr, cx, cy, cz, s, X, Y, Z, ox, oy, ma[k], mb[k], u, v);
        mm_plane_accumulate(acc, ma[k], mb[k], u, v);
    }
    ok = mm_triples_ok(ma, mb, a.collinear_tol) && ok;
    double E[12];
    ok = rp_solve(acc, fr, cx, cy, cz, s, E) && ok;
    double *o = a.Eh + ((size_t)c * a.n_hyp + h) * 12;
    const double nan = __builtin_nan("");
#pragma unroll
    for (int k = 0; k < 12; ++k) o[k] = ok ? E[k] : nan;
}

// ---- MSAC cost of every hypothesis ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void rs_score_kernel(RsArgs a) {
    __shared__ double tile[RS_TILE * 5];
    const int c = blockIdx.x;
    const int h = blockIdx.y * 64 + threadIdx.x;
    const int n_use = (int)a.norm[8 * (size_t)c + 4];
    if (n_use < a.min_rows) return;      // (uniform over the workgroup)
    int lo, hi;
    rs_range(a, c, lo, hi);
    const bool live = h < a.n_hyp;
    double E[12], Q[12];
    const double *src = a.Eh + ((size_t)c * a.n_hyp + (live ? h : 0)) * 12;
#pragma unroll
    for (int k = 0; k < 12; ++k) E[k] = src[k];
    rs_camera(a, E, Q);
    double cost = 0.0;
    for (int j0 = 0; j0 < n_use; j0 += RS_TILE) {
        const int nt = min(RS_TILE, n_use - j0);
        __syncthreads();
        for (int j = threadIdx.x; j < nt; j += 64) {
            double X, Y, Z, ox, oy;
            rs_load(a, lo, j0 + j, X, Y, Z, ox, oy);
            tile[5 * j] = X;
            tile[5 * j + 1] = Y;
            tile[5 * j + 2] = Z;
            tile[5 * j + 3] = ox;
            tile[5 * j + 4] = oy;
        }
        __syncthreads();
        for (int j = 0; j < nt; ++j) {
            double d2;
            const bool in = rs_distance(Q, tile[5 * j], tile[5 * j + 1], tile[5 * j + 2], tile[5 * j + 3], tile[5 * j + 4], a.tau2, d2);
            cost += in ? d2 : a.tau2;
        }
    }
    if (live) a.cost_h[(size_t)c * a.n_hyp + h] = isfinite(E[0]) ? cost : __builtin_huge_val();
}

// ---- winner, prior, refit, polish, outputs ----------------------------------------------------------------------------------
// MSAC cost and inlier count of [R|t] over the usable rows of the camera (every thread returns the same bits)
__device__ __forceinline__ void rs_cost(const RsArgs &a, int lo, int n_use, const double (&E)[12], double *sm, double &cost, int &n_in) {
    double Q[12];
    rs_camera(a, E, Q);
    double v[2] = {0.0, 0.0};
    for (int k = threadIdx.x; k < n_use; k += RS_THREADS) {
        double X, Y, Z, ox, oy, d2;
        rs_load(a, lo, k, X, Y, Z, ox, oy);
        const bool in = rs_distance(Q, X, Y, Z, ox, oy, a.tau2, d2);
        v[0] += in ? d2 : a.tau2;
        v[1] += in ? 1.0 : 0.0;
    }
    mm_block_sum<2>(v, sm);
    cost = v[0];
    n_in = (int)v[1];
}

// one pass of the polish over the set in a.mask: v = (sum |r|^2, rows not in front, H upper triangle (21), g (6))
__device__ __forceinline__ void rs_polish_pass(const RsArgs &a, int lo, int n_use, const double (&E)[12], double *sm, double (&v)[29]) {
    const double fx = a.K[0], sk = a.K[1], pcx = a.K[2], fy = a.K[4], pcy = a.K[5];
#pragma unroll
    for (int k = 0; k < 29; ++k) v[k] = 0.0;
    for (int k = threadIdx.x; k < n_use; k += RS_THREADS) {
        if (a.mask[lo + k] == 0) continue;
        double X, Y, Z, ox, oy;
        rs_load(a, lo, k, X, Y, Z, ox, oy);
        const double D0 = (E[0] * X + E[1] * Y) + E[2] * Z, D1 = (E[4] * X + E[5] * Y) + E[6] * Z, D2 = (E[8] * X + E[9] * Y) + E[10] * Z;
        const double Y0 = D0 + E[3], Y1 = D1 + E[7], Y2 = D2 + E[11];
        const double nu = fx * Y0 + sk * Y1, nv = fy * Y1;
        const double ru = (nu / Y2 + pcx) - ox, rv = (nv / Y2 + pcy) - oy;
        const double a0 = fx / Y2, a1 = sk / Y2, a2 = -((nu / Y2) / Y2), b1 = fy / Y2, b2 = -((nv / Y2) / Y2);
        const double Ju[6] = {a2 * D1 - a1 * D2, a0 * D2 - a2 * D0, a1 * D0 - a0 * D1, a0, a1, a2};
        const double Jv[6] = {b2 * D1 - b1 * D2, -(b2 * D0), b1 * D0, 0.0, b1, b2};
        v[0] += ru * ru + rv * rv;
        v[1] += (Y2 > 0.0) ? 0.0 : 1.0;
        int idx = 2;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = i; j < 6; ++j) v[idx++] += Ju[i] * Ju[j] + Jv[i] * Jv[j];
#pragma unroll
        for (int i = 0; i < 6; ++i) v[23 + i] += Ju[i] * ru + Jv[i] * rv;
    }
    mm_block_sum<29>(v, sm);
}

// (H + lam diag H) delta = -g by a 6 x 6 Cholesky; false: a pivot that is not positive
__device__ __forceinline__ bool rs_lm_step(const double (&v)[29], double lam, double (&e)[6]) {
    double H[6][6], L[6][6], y[6];
    {
        int idx = 2;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = i; j < 6; ++j) {
                H[i][j] = H[j][i] = v[idx];
                ++idx;
            }
    }
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double d = H[j][j] + lam * H[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
        ok = ok && d > 0.0;
        const double ljj = sqrt(d);
        L[j][j] = ljj;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double w = H[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) w -= L[i][k] * L[j][k];
            L[i][j] = w / ljj;
        }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double w = -v[23 + i];
#pragma unroll
        for (int k = 0; k < i; ++k) w -= L[i][k] * y[k];
        y[i] = w / L[i][i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double w = y[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) w -= L[k][i] * e[k];
        e[i] = w / L[i][i];
    }
    return ok;
}

// R <- cay(w) R, t <- t + dt
__device__ __forceinline__ void rs_update(const double (&E)[12], const double (&e)[6], double (&N)[12]) {
    const double a0 = e[0] / 2.0, a1 = e[1] / 2.0, a2 = e[2] / 2.0;
    const double aa = (a0 * a0 + a1 * a1) + a2 * a2;
    const double den = 1.0 + aa, dg = 1.0 - aa;
    const double C[3][3] = {{(dg + 2.0 * (a0 * a0)) / den, (2.0 * (a0 * a1) - 2.0 * a2) / den, (2.0 * (a0 * a2) + 2.0 * a1) / den},
                            {(2.0 * (a1 * a0) + 2.0 * a2) / den, (dg + 2.0 * (a1 * a1)) / den, (2.0 * (a1 * a2) - 2.0 * a0) / den},
                            {(2.0 * (a2 * a0) - 2.0 * a1) / den, (2.0 * (a2 * a1) + 2.0 * a0) / den, (dg + 2.0 * (a2 * a2)) / den}};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) N[4 * r + c] = (C[r][0] * E[c] + C[r][1] * E[4 + c]) + C[r][2] * E[8 + c];
        N[4 * r + 3] = E[4 * r + 3] + e[3 + r];
    }
}

// PLANAR: the finish stage of mm_resect_planar -- the verdict of rp_prepare_kernel decides whether anything runs, and the refit
// is the homography's.  A separate instantiation: the general one compiles from the source it always had.
template <bool PLANAR>
__global__ __launch_bounds__(RS_THREADS) void rs_finish_kernel(RsArgs a) {
    __shared__ double sm[RS_WAVES * 40];
    __shared__ double bc[RS_WAVES];
    __shared__ int bh[RS_WAVES];
    const int c = blockIdx.x, tid = threadIdx.x;
    const double *nr = a.norm + 8 * (size_t)c;
    const int n_use = (int)nr[4];      // (PLANAR: 0 for a camera the homography branch does not run on)
    const double cx = nr[0], cy = nr[1], cz = nr[2], s = nr[3];
    int lo, hi;
    rs_range(a, c, lo, hi);
    const double nan = __builtin_nan("");
    int flags = nr[5] > 0.0 ? MM_RESECT_MALFORMED : 0;
    double E[12], Pr[12];
    bool prior = a.prior != nullptr;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        E[k] = nan;
        Pr[k] = prior ? a.prior[12 * (size_t)c + k] : nan;
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) prior = prior && isfinite(Pr[k]);
    double cost = nan;
    int n_in = 0, best_h = -1, n_valid = 0, n_polish = 0;
    bool model = false;

    if (n_use < a.min_rows) {
        if constexpr (PLANAR) {
            flags |= (int)nr[7];      // TOO_FEW, nothing (refused) or PLANAR | NO_MODEL (collinear)
        } else {
            flags |= MM_RESECT_TOO_FEW;
        }
    } else {
        if constexpr (PLANAR) flags |= MM_RESECT_PLANAR;
        // lowest finite cost, ties to the lowest h; and the number of valid hypotheses
        double c_best;
        int h_best;
        mm_block_argmin_finite(a.cost_h + (size_t)c * a.n_hyp, a.n_hyp, a.Eh + (size_t)c * a.n_hyp * 12, 12, bc, bh, sm, c_best, h_best,
                               n_valid);
        if (h_best != INT32_MAX) {
            model = true;
            best_h = h_best;
#pragma unroll
            for (int k = 0; k < 12; ++k) E[k] = a.Eh[((size_t)c * a.n_hyp + h_best) * 12 + k];
            rs_cost(a, lo, n_use, E, sm, cost, n_in);
        }
        if (prior) {      // hypothesis number n_hyp: it loses ties
            double cp;
            int np_in;
            rs_cost(a, lo, n_use, Pr, sm, cp, np_in);
            if (isfinite(cp) && (!model || cp < cost)) {
                model = true;
                best_h = a.n_hyp;
                cost = cp;
                n_in = np_in;
#pragma unroll
                for (int k = 0; k < 12; ++k) E[k] = Pr[k];
            }
        }
        if (!model) flags |= MM_RESECT_NO_MODEL;
    }

    if (model) {
        for (int it = 0; it < a.refit_iters; ++it) {
            if (n_in < (PLANAR ? 4 : 6)) break;      // (uniform: nothing changes any more)
            double Q[12], En[12];
            rs_camera(a, E, Q);
            bool okE;
            if constexpr (PLANAR) {
                // the plane's frame goes through LDS: read from there it lives in vector registers for this block only (as
                // nine uniform loads it sat in scalar registers over the whole kernel, which has none to spare)
                __shared__ double sfr[9];
                __syncthreads();
                if (tid < 9) sfr[tid] = a.frame[9 * (size_t)c + tid];
                __syncthreads();
                double fr[9], acc[24];
#pragma unroll
                for (int k = 0; k < 9; ++k) fr[k] = sfr[k];
#pragma unroll
                for (int k = 0; k < 24; ++k) acc[k] = 0.0;
                for (int k = tid; k < n_use; k += RS_THREADS) {
                    double X, Y, Z, ox, oy, d2;
                    rs_load(a, lo, k, X, Y, Z, ox, oy);
                    if (rs_distance(Q, X, Y, Z, ox, oy, a.tau2, d2)) {
                        double ma, mb, u, v;
                        rp_row(a, fr, cx, cy, cz, s, X, Y, Z, ox, oy, ma, mb, u, v);
                        mm_plane_accumulate(acc, ma, mb, u, v);
                    }
                }
                mm_block_sum<24>(acc, sm);
                okE = rp_solve(acc, fr, cx, cy, cz, s, En);
            } else {
                double acc[40];
#pragma unroll
                for (int k = 0; k < 40; ++k) acc[k] = 0.0;
                for (int k = tid; k < n_use; k += RS_THREADS) {
                    double X, Y, Z, ox, oy, d2;
                    rs_load(a, lo, k, X, Y, Z, ox, oy);
                    if (rs_distance(Q, X, Y, Z, ox, oy, a.tau2, d2)) rs_accumulate(acc, a, cx, cy, cz, s, X, Y, Z, ox, oy);
                }
                mm_block_sum<40>(acc, sm);
                okE = rs_solve(acc, cx, cy, cz, s, En);
            }
            double cn;
            int nn_in;
            rs_cost(a, lo, n_use, En, sm, cn, nn_in);
            if (okE && isfinite(cn) && cn < cost) {
                cost = cn;
                n_in = nn_in;
#pragma unroll
                for (int k = 0; k < 12; ++k) E[k] = En[k];
            }
        }
        if (a.polish_iters > 0) {
            // the set: the inliers of the model at entry (each thread writes and later reads its own rows)
            double Q[12];
            rs_camera(a, E, Q);
            for (int k = tid; k < n_use; k += RS_THREADS) {
                double X, Y, Z, ox, oy, d2;
                rs_load(a, lo, k, X, Y, Z, ox, oy);
                a.mask[lo + k] = rs_distance(Q, X, Y, Z, ox, oy, a.tau2, d2) ? 1 : 0;
            }
            double Ec[12], v[29], lam = 1e-3;
#pragma unroll
            for (int k = 0; k < 12; ++k) Ec[k] = E[k];
            rs_polish_pass(a, lo, n_use, Ec, sm, v);
            int accepted = 0;
            for (int it = 0; it < a.polish_iters; ++it) {
                double e[6], En[12], vn[29];
                const bool ok = rs_lm_step(v, lam, e);
                rs_update(Ec, e, En);
                rs_polish_pass(a, lo, n_use, En, sm, vn);
                const bool accept = ok && vn[1] == 0.0 && isfinite(vn[0]) && vn[0] < v[0];
                if (accept) {
                    ++accepted;
#pragma unroll
                    for (int k = 0; k < 12; ++k) Ec[k] = En[k];
#pragma unroll
                    for (int k = 0; k < 29; ++k) v[k] = vn[k];
                }
                lam = accept ? fmax(lam / 10.0, 1e-12) : lam * 10.0;
            }
            if (accepted > 0) {
                double cn;
                int nn_in;
                bool fin = true;
#pragma unroll
                for (int k = 0; k < 12; ++k) fin = fin && isfinite(Ec[k]);
                rs_cost(a, lo, n_use, Ec, sm, cn, nn_in);
                if (fin && isfinite(cn) && cn < cost) {
                    cost = cn;
                    n_in = nn_in;
                    n_polish = accepted;
#pragma unroll
                    for (int k = 0; k < 12; ++k) E[k] = Ec[k];
                }
            }
        }
        if (n_in < a.min_inliers) flags |= MM_RESECT_WEAK;
        // the inliers of the final model (the prepare kernel has zeroed every row the call writes)
        double Q[12];
        rs_camera(a, E, Q);
        for (int k = tid; k < n_use; k += RS_THREADS) {
            double X, Y, Z, ox, oy, d2;
            rs_load(a, lo, k, X, Y, Z, ox, oy);
            a.inlier[a.rows[lo + k]] = rs_distance(Q, X, Y, Z, ox, oy, a.tau2, d2) ? 1 : 0;
        }
    }
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < 12; ++k) a.ext[12 * (size_t)c + k] = model ? E[k] : Pr[k];      // (an absent prior is NaN)
        a.cost[c] = cost;
        int32_t *o = a.info + 6 * (size_t)c;
        o[0] = flags;
        o[1] = n_in;
        o[2] = best_h;
        o[3] = n_valid;
        o[4] = PLANAR ? (int)nr[6] : n_use;
        o[5] = n_polish;
    }
}

size_t rs_region(size_t bytes) { return mm_align_up(bytes, 256); }

}  // namespace

extern "C" size_t mm_resect_workspace_bytes(int n_cams, int n_hyp, int64_t n_rows) {
    const size_t nc = n_cams > 0 ? (size_t)n_cams : 0, nh = n_hyp > 0 ? (size_t)n_hyp : 0, nr = n_rows > 0 ? (size_t)n_rows : 0;
    return rs_region(nc * 8 * sizeof(double)) + rs_region(nc * nh * 12 * sizeof(double)) + rs_region(nc * nh * sizeof(double)) +
           rs_region(nr * sizeof(int32_t)) + rs_region(nr);
}

namespace {

// Every argument of the two entry points judged, then RsArgs filled and the general workspace carved (`extra` bytes may follow
// it).  MM_OK with launch = false: n_cams = 0.  Nothing here touches the device.
int rs_setup(mm_ctx *ctx, const char *fn, const double *K, const double *X, int64_t P, const double *obs, const int32_t *pi, int64_t O,
             const int32_t *cam_ptr, const int32_t *cam_obs, int64_t n_rows, int n_cams, const uint8_t *pt_ok, const double *prior,
             const mm_resect_params *prm, int row_floor, double *extrinsics, double *cost, uint8_t *inlier, int32_t *info, void *ws,
             size_t ws_bytes, size_t extra, bool extra_ok, RsArgs &a, char *&ws_end, bool &launch) {
    launch = false;
    // every argument is judged before the context is looked at: nothing below this block runs on a bad call
    if (!prm || !K || n_cams < 0 || P < 0 || O < 0 || n_rows < 0 || P > INT32_MAX || O > INT32_MAX || n_rows > INT32_MAX)
        return mm_fail(ctx, MM_ERR_ARG, "%s: bad argument", fn);
    if (prm->n_hyp < 1 || prm->n_hyp > 4096) return mm_fail(ctx, MM_ERR_ARG, "%s: n_hyp must be in 1 .. 4096", fn);
    if (!(prm->threshold_px >= 0.0))      // (negative or NaN)
        return mm_fail(ctx, MM_ERR_ARG, "%s: threshold_px must not be negative", fn);
    if (prm->refit_iters < 0 || prm->refit_iters > 1000 || prm->polish_iters < 0 || prm->polish_iters > 1000 || prm->min_inliers < 0)
        return mm_fail(ctx, MM_ERR_ARG, "%s: bad parameter", fn);
    if (!extra_ok) return mm_fail(ctx, MM_ERR_ARG, "%s: planar_tol and collinear_tol must not be negative", fn);
    bool k_ok = K[3] == 0.0 && K[6] == 0.0 && K[7] == 0.0 && K[8] == 1.0 && K[0] != 0.0 && K[4] != 0.0;
    for (int k = 0; k < 9; ++k) k_ok = k_ok && std::isfinite(K[k]);
    if (!k_ok)
        return mm_fail(ctx, MM_ERR_ARG, "%s: K must be finite and upper triangular with K[8] = 1 and non-zero focal lengths", fn);
    if (n_cams > 0 && (!cam_ptr || !extrinsics || !cost || !info || !ws)) return mm_fail(ctx, MM_ERR_ARG, "%s: bad argument", fn);
    if (n_cams > 0 && n_rows > 0 && (!cam_obs || !inlier || (O > 0 && (!obs || !pi)) || (P > 0 && !X)))
        return mm_fail(ctx, MM_ERR_ARG, "%s: bad argument", fn);
    if (n_cams > 0 && ws_bytes < mm_resect_workspace_bytes(n_cams, prm->n_hyp, n_rows) + extra)
        return mm_fail(ctx, MM_ERR_WORKSPACE, "%s: workspace too small", fn);
    if (!ctx) return MM_ERR_ARG;
    if (n_cams == 0) return MM_OK;
    if (((uintptr_t)ws) & 7) return mm_fail(ctx, MM_ERR_ARG, "%s: the workspace must be 8-byte aligned", fn);
    a.X = X;
    a.obs = obs;
    a.pi = pi;
    a.cam_ptr = cam_ptr;
    a.cam_obs = cam_obs;
    a.pt_ok = pt_ok;
    a.prior = prior;
    a.P = P;
    a.O = O;
    a.n_rows = n_rows;
    a.n_cams = n_cams;
    a.n_hyp = prm->n_hyp;
    a.min_rows = prm->min_rows < row_floor ? row_floor : prm->min_rows;
    a.min_inliers = prm->min_inliers;
    a.refit_iters = prm->refit_iters;
    a.polish_iters = prm->polish_iters;
    a.seed = prm->seed;
    a.cam_base = prm->cam_base;
    a.tau2 = prm->threshold_px * prm->threshold_px;
    for (int k = 0; k < 9; ++k) a.K[k] = K[k];
    mm_k_inverse(K, a.Ki);
    char *w = (char *)ws;
    a.norm = (double *)w;
    w += rs_region((size_t)n_cams * 8 * sizeof(double));
    a.Eh = (double *)w;
    w += rs_region((size_t)n_cams * a.n_hyp * 12 * sizeof(double));
    a.cost_h = (double *)w;
    w += rs_region((size_t)n_cams * a.n_hyp * sizeof(double));
    a.rows = (int32_t *)w;
    w += rs_region((size_t)n_rows * sizeof(int32_t));
    a.mask = (uint8_t *)w;
    w += rs_region((size_t)n_rows);
    ws_end = w;
    a.frame = nullptr;
    a.plane = nullptr;
    a.planar_tol2 = 0.0;
    a.collinear_tol = 0.0;
    a.ext = extrinsics;
    a.cost = cost;
    a.inlier = inlier;
    a.info = info;
    launch = true;
    return MM_OK;
}

}  // namespace

extern "C" int mm_resect_cameras(mm_ctx *ctx, const double *K, const double *X, int64_t P, const double *obs, const int32_t *pi,
                                 int64_t O, const int32_t *cam_ptr, const int32_t *cam_obs, int64_t n_rows, int n_cams,
                                 const uint8_t *pt_ok, const double *prior, const mm_resect_params *prm, double *extrinsics,
                                 double *cost, uint8_t *inlier, int32_t *info, void *ws, size_t ws_bytes) {
    RsArgs a;
    char *ws_end;
    bool launch;
    const int rc = rs_setup(ctx, "mm_resect_cameras", K, X, P, obs, pi, O, cam_ptr, cam_obs, n_rows, n_cams, pt_ok, prior, prm, 12,
                            extrinsics, cost, inlier, info, ws, ws_bytes, 0, true, a, ws_end, launch);
    if (rc != MM_OK || !launch) return rc;
    const dim3 per_hyp((unsigned)n_cams, (unsigned)((a.n_hyp + 63) / 64));
    MM_LAUNCH(ctx, "rs_prepare_kernel", rs_prepare_kernel, dim3((unsigned)n_cams), dim3(RS_THREADS), 0, a);
    MM_LAUNCH(ctx, "rs_hypothesis_kernel", rs_hypothesis_kernel, per_hyp, dim3(64), 0, a);
    MM_LAUNCH(ctx, "rs_score_kernel", rs_score_kernel, per_hyp, dim3(64), 0, a);
    MM_LAUNCH(ctx, "rs_finish_kernel", rs_finish_kernel<false>, dim3((unsigned)n_cams), dim3(RS_THREADS), 0, a);
    return MM_OK;
}

extern "C" size_t mm_resect_planar_workspace_bytes(int n_cams, int n_hyp, int64_t n_rows) {
    const size_t nc = n_cams > 0 ? (size_t)n_cams : 0;
    return mm_resect_workspace_bytes(n_cams, n_hyp, n_rows) + rs_region(nc * 9 * sizeof(double));
}

extern "C" int mm_resect_planar(mm_ctx *ctx, const double *K, const double *X, int64_t P, const double *obs, const int32_t *pi,
                                int64_t O, const int32_t *cam_ptr, const int32_t *cam_obs, int64_t n_rows, int n_cams,
                                const uint8_t *pt_ok, const double *prior, const mm_resect_planar_params *prm, double *extrinsics,
                                double *cost, uint8_t *inlier, int32_t *info, double *plane, void *ws, size_t ws_bytes) {
    mm_resect_params base;
    bool tol_ok = false;
    if (prm) {
        base.n_hyp = prm->n_hyp;
        base.min_rows = prm->min_rows;
        base.min_inliers = prm->min_inliers;
        base.refit_iters = prm->refit_iters;
        base.polish_iters = prm->polish_iters;
        base.reserved = 0;
        base.seed = prm->seed;
        base.cam_base = prm->cam_base;
        base.threshold_px = prm->threshold_px;
        tol_ok = prm->planar_tol >= 0.0 && prm->collinear_tol >= 0.0 && std::isfinite(prm->planar_tol) && std::isfinite(prm->collinear_tol);
    }
    if (n_cams > 0 && !plane) return mm_fail(ctx, MM_ERR_ARG, "mm_resect_planar: bad argument");
    RsArgs a;
    char *ws_end;
    bool launch;
    const size_t extra = rs_region((size_t)(n_cams > 0 ? n_cams : 0) * 9 * sizeof(double));
    const int rc = rs_setup(ctx, "mm_resect_planar", K, X, P, obs, pi, O, cam_ptr, cam_obs, n_rows, n_cams, pt_ok, prior,
                            prm ? &base : nullptr, 8, extrinsics, cost, inlier, info, ws, ws_bytes, extra, !prm || tol_ok, a, ws_end, launch);
    if (rc != MM_OK || !launch) return rc;
    a.frame = (double *)ws_end;
    a.plane = plane;
    a.planar_tol2 = prm->planar_tol * prm->planar_tol;
    a.collinear_tol = prm->collinear_tol;
    const dim3 per_hyp((unsigned)n_cams, (unsigned)((a.n_hyp + 63) / 64));
    MM_LAUNCH(ctx, "rp_prepare_kernel", rp_prepare_kernel, dim3((unsigned)n_cams), dim3(RS_THREADS), 0, a);
    MM_LAUNCH(ctx, "rp_hypothesis_kernel", rp_hypothesis_kernel, per_hyp, dim3(64), 0, a);
    MM_LAUNCH(ctx, "rs_score_kernel", rs_score_kernel, per_hyp, dim3(64), 0, a);
    MM_LAUNCH(ctx, "rp_finish_kernel", rs_finish_kernel<true>, dim3((unsigned)n_cams), dim3(RS_THREADS), 0, a);
    return MM_OK;
}
