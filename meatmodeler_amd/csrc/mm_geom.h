// What the geometry stages share (verify.hip, pose.hip, resect.hip, homography.hip, triangulate.hip); mm_pairs.h holds what
// only the stages over match pairs share.
//
// include/meatmodeler.h states each of these once and lets the later stages refer back ("the integer scheme of
// mm_verify_matches", "the reduced DLT of mm_resect_planar"); the stages promise results that repeat bit for bit, so every one
// of them is written once.  The rule: shared means a definition (a sampling scheme, a reduction order, a solve the C header
// gives once) or a skeleton (a loop that is the same around any model); a stage's model -- its distance, its solver's own
// tail, its verdict and flags -- stays in the stage's file and is plugged in.  Header only, __forceinline__ templates: each is
// compiled under the flags of the file that includes it (FMA contraction is off for pose.hip, resect.hip and homography.hip, on
// for verify.hip and triangulate.hip -- Makefile), so a stage's bits are those of its own build.  With contraction off the
// bits follow from the expression trees alone; with it on, where a piece stands can change which products fuse, and a file
// then keeps a written-out copy, marked as such (mm_jacobi below, tri_tracks_kernel, verify.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

constexpr double MM_F64_EPS = 2.220446049250313e-16;

// workgroup shape of the mm_block_* helpers: 256 threads, four waves of 64 (callers static_assert their thread count)
constexpr int MM_BLOCK_THREADS = 256;
constexpr int MM_BLOCK_WAVES = MM_BLOCK_THREADS / 64;

__host__ __device__ __forceinline__ uint32_t mm_pcg(uint32_t v) {
    const uint32_t s = v * 747796405u + 2891336453u;
    const uint32_t w = ((s >> ((s >> 28) + 4u)) ^ s) * 277803737u;
    return (w >> 22) ^ w;
}

// K distinct indices in [0, n), integer arithmetic only: pick k is the first of the eight tries pcg(base + 8 k + t) * n >> 32
// that is not an earlier pick.  false: some pick found all eight tries taken (that pick is 0).
template <int K>
__device__ __forceinline__ bool mm_sample_distinct(uint32_t base, int n, int (&pick)[K]) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        int chosen = -1;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const uint32_t r = mm_pcg(base + (uint32_t)(8 * k + t));
            const int i = (int)(((uint64_t)r * (uint64_t)n) >> 32);
            bool dup = false;
#pragma unroll
            for (int e = 0; e < k; ++e) dup = dup || pick[e] == i;
            if (chosen < 0 && !dup) chosen = i;
        }
        ok = ok && chosen >= 0;
        pick[k] = chosen < 0 ? 0 : chosen;
    }
    return ok;
}

// sum over the workgroup in a fixed order: xor butterfly inside a wave (addition commutes: every lane ends with the same
// bits), then the waves' sums in wave order.  sm holds MM_BLOCK_WAVES * N doubles.  Every thread of the workgroup calls
// it; it contains two barriers (the first also guards sm against the previous call's readers); every thread ends with the
// same bits.
template <int N>
__device__ __forceinline__ void mm_block_sum(double (&v)[N], double *sm) {
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v[i] += __shfl_xor(v[i], off, 64);
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    __syncthreads();
    if (l == 0) {
#pragma unroll
        for (int i = 0; i < N; ++i) sm[w * N + i] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = ((sm[i] + sm[N + i]) + sm[2 * N + i]) + sm[3 * N + i];
}

template <int N>
__device__ __forceinline__ void mm_identity(double (&V)[N][N]) {
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
        for (int c = 0; c < N; ++c) V[r][c] = (r == c) ? 1.0 : 0.0;
}

// Two-sided cyclic Jacobi in registers (every index static): the eigenvalues of the symmetric G end up on its diagonal, and
// V, which the caller sets to the identity, is rotated along: its columns end up as the eigenvectors.  Pairs (p, q)
// ascending, at most 30 sweeps; a rotation is skipped once |g_pq| <= eps sqrt(|g_pp g_qq|), the criterion that keeps the
// small eigenvalues of a positive semi-definite matrix accurate relative to themselves.
// Where V is set matters to the compiler, not to the mathematics: set inside a function (mm_identity) the sweeps are
// arranged one way, set by loops in the caller's own body another.  verify.hip (FMA contraction on) sets V in its own
// loop, where it always did; pose.hip and resect.hip (contraction off: one value either way) call mm_identity, and compile
// to what they compiled to.  tri_tracks_kernel keeps a written-out copy of this loop (see there).
// The callers then take the column of the smallest diagonal entry, ties to the lowest column; that selection is written
// out at each call site (as a function here it turned the callers' branches into selects).
template <int N>
__device__ __forceinline__ void mm_jacobi(double (&G)[N][N], double (&V)[N][N]) {
    for (int sweep = 0; sweep < 30; ++sweep) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < N - 1; ++p) {
#pragma unroll
            for (int q = p + 1; q < N; ++q) {
                const double apq = G[p][q];
                if (fabs(apq) > MM_F64_EPS * sqrt(fabs(G[p][p] * G[q][q])) && apq != 0.0) {
                    rotated = true;
                    const double zeta = (G[q][q] - G[p][p]) / (2.0 * apq);
                    const double tn = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                    const double cs = 1.0 / sqrt(1.0 + tn * tn);
                    const double sn = cs * tn;
#pragma unroll
                    for (int k = 0; k < N; ++k) {      // columns p, q of G and of V
                        const double akp = G[k][p], akq = G[k][q];
                        G[k][p] = cs * akp - sn * akq;
                        G[k][q] = sn * akp + cs * akq;
                        const double vkp = V[k][p], vkq = V[k][q];
                        V[k][p] = cs * vkp - sn * vkq;
                        V[k][q] = sn * vkp + cs * vkq;
                    }
#pragma unroll
                    for (int k = 0; k < N; ++k) {      // rows p, q of G
                        const double apk = G[p][k], aqk = G[q][k];
                        G[p][k] = cs * apk - sn * aqk;
                        G[q][k] = sn * apk + cs * aqk;
                    }
                    G[p][q] = G[q][p] = 0.0;
                }
            }
        }
        if (!rotated) break;
    }
}

// c = a x b, each component one difference of two products
__device__ __forceinline__ void mm_cross3(const double (&a)[3], const double (&b)[3], double (&c)[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// ---- 3-vectors held by value (pose.hip, homography.hip) -------------------------------------------------------------------
struct Vec3 {
    double x, y, z;
};
__device__ __forceinline__ double dot3(Vec3 a, Vec3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ Vec3 cross3(Vec3 a, Vec3 b) {
    return Vec3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
// row-major 3 x 3 times vector
__device__ __forceinline__ Vec3 mat3(const double (&M)[9], Vec3 v) {
    return Vec3{(M[0] * v.x + M[1] * v.y) + M[2] * v.z, (M[3] * v.x + M[4] * v.y) + M[5] * v.z, (M[6] * v.x + M[7] * v.y) + M[8] * v.z};
}

// Cholesky S = L L^T of a small symmetric matrix in registers, column by column, each entry reduced by its products left to
// right.  false: some pivot was not finite or <= 1e-12 times the diagonal entry it started from (the factor is then
// unusable; every entry is still written).  Only the lower triangle of L is set.
template <int N>
__device__ __forceinline__ bool mm_cholesky_pivot(const double (&S)[N][N], double (&L)[N][N]) {
    bool ok = true;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        double d = S[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
        ok = ok && isfinite(d) && d > 1e-12 * S[j][j];
        const double ljj = sqrt(d);
        L[j][j] = ljj;
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            double v = S[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
            L[i][j] = v / ljj;
        }
    }
    return ok;
}

// Polar factor of a 3 x 3 A: R = A (V diag(lambda^-1/2) V^T) with lambda, V from the cyclic Jacobi of A^T A; rt receives
// sqrt(lambda) in the Jacobi's order.  false: a lambda that is not finite and positive.  det R has the sign of det A.
__device__ __forceinline__ bool mm_polar3(const double (&A)[3][3], double (&R)[3][3], double (&rt)[3]) {
    double G[3][3], V[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) G[r][c] = (A[0][r] * A[0][c] + A[1][r] * A[1][c]) + A[2][r] * A[2][c];
    mm_identity<3>(V);
    mm_jacobi<3>(G, V);
    bool ok = true;
    double dk[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double lam = G[k][k];
        ok = ok && isfinite(lam) && lam > 0.0;
        rt[k] = sqrt(lam);
        dk[k] = 1.0 / rt[k];
    }
    double W[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) W[i][j] = ((V[i][0] * dk[0]) * V[j][0] + (V[i][1] * dk[1]) * V[j][1]) + (V[i][2] * dk[2]) * V[j][2];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) R[r][c] = (A[r][0] * W[0][c] + A[r][1] * W[1][c]) + A[r][2] * W[2][c];
    return ok;
}

// ---- the reduced DLT of a plane-to-image map (mm_resect_planar, mm_verify_homography) -------------------------------------
// one correspondence into the 24 sums: S, Bu, Bv, C, each the upper triangle of a 3 x 3, row-major, over m = (ma, mb, 1), the
// normalised plane point, with (u, v) its image
__device__ __forceinline__ void mm_plane_accumulate(double (&acc)[24], double ma, double mb, double u, double v) {
    const double m[3] = {ma, mb, 1.0};
    const double r2 = u * u + v * v;
    int k = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i; j < 3; ++j) {
            const double w = m[i] * m[j];
            acc[k] += w;
            acc[6 + k] += u * w;
            acc[12 + k] += v * w;
            acc[18 + k] += r2 * w;
            ++k;
        }
}

// true: the triangle (i, j, k) is not near-collinear: |cross| > tol x its longest squared side (NaN: false)
__device__ __forceinline__ bool mm_triple_ok(double ai, double bi, double aj, double bj, double ak, double bk, double tol) {
    const double pa = aj - ai, pb = bj - bi, qa = ak - ai, qb = bk - bi, ra = ak - aj, rb = bk - bj;
    const double cr = pa * qb - pb * qa;
    const double d0 = pa * pa + pb * pb, d1 = qa * qa + qb * qb, d2 = ra * ra + rb * rb;
    double lng = d0 > d1 ? d0 : d1;
    lng = lng > d2 ? lng : d2;
    return fabs(cr) > tol * lng;
}
// the rule over the four triples of four sampled points (a[k], b[k])
__device__ __forceinline__ bool mm_triples_ok(const double (&a)[4], const double (&b)[4], double tol) {
    bool ok = mm_triple_ok(a[0], b[0], a[1], b[1], a[2], b[2], tol);
    ok = mm_triple_ok(a[0], b[0], a[1], b[1], a[3], b[3], tol) && ok;
    ok = mm_triple_ok(a[0], b[0], a[2], b[2], a[3], b[3], tol) && ok;
    ok = mm_triple_ok(a[1], b[1], a[2], b[2], a[3], b[3], tol) && ok;
    return ok;
}

// The rows h1, h2, h3 of the map from the 24 sums: Cholesky of S, C - Bu S^-1 Bu - Bv S^-1 Bv through the two triangular
// solves, h3 = its eigenvector of the smallest eigenvalue (3 x 3 Jacobi, ties to the lowest column), h1 = S^-1 Bu h3 and
// h2 = S^-1 Bv h3 by back substitution.  Returns the pivot verdict of the Cholesky; every entry is written either way.
__device__ __forceinline__ bool mm_plane_dlt(const double (&acc)[24], double (&h1)[3], double (&h2)[3], double (&h3)[3]) {
    double S[3][3], Bu[3][3], Bv[3][3], M[3][3];
    {
        int k = 0;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = i; j < 3; ++j) {
                S[i][j] = S[j][i] = acc[k];
                Bu[i][j] = Bu[j][i] = acc[6 + k];
                Bv[i][j] = Bv[j][i] = acc[12 + k];
                M[i][j] = M[j][i] = acc[18 + k];
                ++k;
            }
    }
    double L[3][3];
    bool ok = mm_cholesky_pivot<3>(S, L);
    double Yu[3][3], Yv[3][3];      // L^-1 Bu, L^-1 Bv
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
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
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i; j < 3; ++j) {
            const double tu = (Yu[0][i] * Yu[0][j] + Yu[1][i] * Yu[1][j]) + Yu[2][i] * Yu[2][j];
            const double tv = (Yv[0][i] * Yv[0][j] + Yv[1][i] * Yv[1][j]) + Yv[2][i] * Yv[2][j];
            M[i][j] = M[j][i] = (M[i][j] - tu) - tv;
        }
    double V3[3][3];
    mm_identity<3>(V3);
    mm_jacobi<3>(M, V3);
    double ev = M[0][0];      // smallest eigenvalue, ties to the lowest column
    h3[0] = V3[0][0];
    h3[1] = V3[1][0];
    h3[2] = V3[2][0];
#pragma unroll
    for (int c = 1; c < 3; ++c) {
        if (M[c][c] < ev) {
            ev = M[c][c];
#pragma unroll
            for (int r = 0; r < 3; ++r) h3[r] = V3[r][c];
        }
    }
    {   // S^-1 Bu h3 = L^-T (Yu h3), S^-1 Bv h3
        double wu[3], wv[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            wu[i] = (Yu[i][0] * h3[0] + Yu[i][1] * h3[1]) + Yu[i][2] * h3[2];
            wv[i] = (Yv[i][0] * h3[0] + Yv[i][1] * h3[1]) + Yv[i][2] * h3[2];
        }
#pragma unroll
        for (int i = 2; i >= 0; --i) {
            double vu = wu[i], vv = wv[i];
#pragma unroll
            for (int k = i + 1; k < 3; ++k) {
                vu -= L[k][i] * h1[k];
                vv -= L[k][i] * h2[k];
            }
            h1[i] = vu / L[i][i];
            h2[i] = vv / L[i][i];
        }
    }
    return ok;
}

// Argmin over the n hypotheses of one workgroup's item: the lowest finite cost[h], ties to the lowest h (h_best stays
// INT32_MAX when no cost is finite), and n_valid = the number of h whose probe[h * probe_stride] is finite.  Butterfly
// inside a wave, then the waves in order through bc / bh (MM_BLOCK_WAVES entries each); sm as for mm_block_sum<1>.  Every
// thread of the workgroup calls it and ends with the same values.
__device__ __forceinline__ void mm_block_argmin_finite(const double *cost, int n, const double *probe, int probe_stride, double *bc,
                                                       int *bh, double *sm, double &c_best, int &h_best, int &n_valid) {
    c_best = __builtin_huge_val();
    h_best = INT32_MAX;
    double nv[1] = {0.0};
    for (int h = threadIdx.x; h < n; h += MM_BLOCK_THREADS) {
        const double ch = cost[h];
        nv[0] += isfinite(probe[(size_t)h * probe_stride]) ? 1.0 : 0.0;
        if (isfinite(ch) && ch < c_best) {
            c_best = ch;
            h_best = h;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double oc = __shfl_xor(c_best, off, 64);
        const int oh = __shfl_xor(h_best, off, 64);
        if (oc < c_best || (oc == c_best && oh < h_best)) {
            c_best = oc;
            h_best = oh;
        }
    }
    if ((threadIdx.x & 63) == 0) {
        bc[threadIdx.x >> 6] = c_best;
        bh[threadIdx.x >> 6] = h_best;
    }
    mm_block_sum<1>(nv, sm);      // (its barriers also publish bc / bh)
    n_valid = (int)nv[0];
    c_best = bc[0];
    h_best = bh[0];
#pragma unroll
    for (int w = 1; w < MM_BLOCK_WAVES; ++w) {
        if (bc[w] < c_best || (bc[w] == c_best && bh[w] < h_best)) {
            c_best = bc[w];
            h_best = bh[w];
        }
    }
}

// Order-preserving compaction, one round of MM_BLOCK_THREADS candidates: the slot of this thread's element among the kept
// ones (ballot, popcount prefix, the waves' counts in wcount[MM_BLOCK_WAVES]), counted from `running`, which advances by
// the round's total.  Contains two barriers: call it from loops whose trip count is uniform over the workgroup.
__device__ __forceinline__ int mm_block_compact_slot(bool keep, int &running, int *wcount) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(keep);
    __syncthreads();
    if (lane == 0) wcount[wave] = __popcll(bal);
    __syncthreads();
    int at = running;
    for (int w = 0; w < wave; ++w) at += wcount[w];
    at += __popcll(bal & ((1ull << lane) - 1ull));
    running += wcount[0] + wcount[1] + wcount[2] + wcount[3];
    return at;
}

// K^-1 = [[Ki0, Ki1, Ki2], [0, Ki3, Ki4], [0, 0, 1]] of the upper triangular K with K[8] = 1, in closed form (host)
inline void mm_k_inverse(const double K[9], double Ki[5]) {
    const double fx = K[0], sk = K[1], cx = K[2], fy = K[4], cy = K[5];
    Ki[0] = 1.0 / fx;
    Ki[1] = -sk / (fx * fy);
    Ki[2] = (sk * cy - cx * fy) / (fx * fy);
    Ki[3] = 1.0 / fy;
    Ki[4] = -cy / fy;
}
