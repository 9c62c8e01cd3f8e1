/*
 * meatmodeler.h — C ABI of libmeatmodeler_hip.so (MI355X / gfx950 only).
 *
 * The drop-in boundary for the structure-from-motion hot path of skyepurchase/MeatModeler.
 * The reference has no FFI of its own (it is pure Python calling cv2 / scipy); each entry point below
 * names the reference call site it replaces (paths relative to the reference checkout) — the Python
 * façade in meatmodeler_amd/{processor,bundleAdjuster,track}.py binds them with ctypes
 * (see INTEGRATION.md for the stub a maintainer would add).
 *
 * Conventions
 *  - extern "C", plain pointers and sizes; no torch / C++ types.
 *  - Pointers marked [dev] are HIP device pointers on the context's device; [host] are host pointers.
 *  - Every call is asynchronous on the context's stream unless marked (sync); no call allocates or
 *    frees device memory: the caller passes workspaces sized by the *_workspace_bytes functions.
 *  - Return value: 0 = ok, negative = error (text via mm_last_error).  Nothing throws across the ABI.
 */
#ifndef MEATMODELER_H
#define MEATMODELER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MM_OK 0
#define MM_ERR_ARG (-1)
#define MM_ERR_HIP (-2)
#define MM_ERR_WORKSPACE (-3)
#define MM_ERR_NUMERIC (-4)

typedef struct mm_ctx mm_ctx;

/* ---- context ------------------------------------------------------------------------------- */
/* 3 since round 4: mm_trf_report is 64 bytes (chol_fallbacks, collectives), mm_ctx_control / mm_flatten_* /
 * mm_ba_trf_dist / mm_ba_trf_batched exist.  A caller built against an older header must refuse to run. */
int mm_abi_version(void);
/* hip_stream: a hipStream_t (e.g. torch.cuda.current_stream().cuda_stream) or NULL for the default stream. */
int mm_ctx_create(int device, void *hip_stream, mm_ctx **out);
void mm_ctx_destroy(mm_ctx *ctx);
const char *mm_last_error(mm_ctx *ctx);
int mm_ctx_sync(mm_ctx *ctx); /* (sync) hipStreamSynchronize on the context stream */
/* Knobs and queries of a context (tests, diagnostics).  Returns the queried value, MM_OK, or a negative error.
 *   MM_CTL_CHOL_FORCE_ABANDON: the next `value` single-launch banded factorisations on this context give up as if one of
 *     their workgroups had not become resident (info = -1) -- exercises the fall-back to the launch-per-column path;
 *   MM_CTL_CHOL_LAST_PATH: path of the last mm_chol_solve* on this context: 1 single launch, 0 per column, -1 none yet;
 *   MM_CTL_CHOL_RESERVED: workgroups this context currently holds of the per-process budget of co-resident
 *     factorisation workgroups (one compute unit each; given back at the context's next synchronisation, at every
 *     read-back inside mm_ba_trf, or -- once the event recorded behind the solve has completed -- at this context's next
 *     reservation or when another context finds the budget spent);
 *   MM_CTL_CU_COUNT: compute units of the device;
 *   MM_CTL_CHOL_AVOID_FUSED: value != 0: this context takes the launch-per-column factorisation from now on (what a
 *     caller that sequences the solver itself does after it has seen info = -1); 0: back to the default; < 0: query.
 *     Returns the setting as it was BEFORE the call (0 / 1), so a caller can restore it. */
#define MM_CTL_CHOL_FORCE_ABANDON 1
#define MM_CTL_CHOL_LAST_PATH 2
#define MM_CTL_CHOL_RESERVED 3
#define MM_CTL_CU_COUNT 4
#define MM_CTL_CHOL_AVOID_FUSED 5
/*   MM_CTL_LINK_LAST_VARIANT: formulation the last mm_link_tracks_device on this context took: 1 parallel (pointer
 *     doubling), 0 serial (asked for with MM_LINK_VARIANT=serial, or the safety valve: the parallel formulation's
 *     fixed-point pass over key points with coincident coordinates exceeded its work budget), -1 none yet. */
#define MM_CTL_LINK_LAST_VARIANT 6
/*   MM_CTL_BATCH_LAST: problems the last mm_ba_trf_batched on this context advanced in lock-step (0: all were solved one by
 *     one), -1 none yet. */
#define MM_CTL_BATCH_LAST 7
long long mm_ctx_control(mm_ctx *ctx, int what, long long value);
/* HIP-event timing on the context stream (bench.py's roofline leg). */
int mm_timer_create(mm_ctx *ctx, void **timer_out);
int mm_timer_start(mm_ctx *ctx, void *timer);
int mm_timer_stop(mm_ctx *ctx, void *timer);
int mm_timer_elapsed_ms(mm_ctx *ctx, void *timer, float *ms_out); /* (sync) */
void mm_timer_destroy(mm_ctx *ctx, void *timer);
/* Per-launch profiling: on = 1 brackets every kernel launched through this context with two HIP events on the
 * context's stream (~2.5 us of device time and ~5 us of host time per launch); on = 2 only launches of >= 64
 * workgroups, leaving the micro-launch chains of the Cholesky untouched; on = 3 only launches of the kernel named by
 * mm_profile_select (the name mm_profile_report prints; what bench.py's timed steps use: every bracketed launch costs the
 * stream a bubble, ~10 % of a BA iteration with on = 2); on = 0 stops collecting.  mm_profile_report (sync) writes one line
 * per kernel name, "name launches total_ms\n", and returns the number of lines.  Enabling clears earlier records. */
int mm_profile_enable(mm_ctx *ctx, int on);
int mm_profile_select(mm_ctx *ctx, const char *name);
int mm_profile_report(mm_ctx *ctx, char *buf, size_t buf_len);

/* ---- a-2: brute-force Hamming 2-NN + ratio test ----------------------------------------------
 * Replaces cv2.FlannBasedMatcher(...).knnMatch(prev_desc, new_desc, k=2) and the Lowe filter,
 * processor.py:132-137 (exact form of the approximate FLANN search; ties -> lowest train index).
 *
 * Batched form: pair p matches query set  q + p*q_set_stride  (nq[p] rows, or nq_cap if nq == NULL)
 * against train set t + p*t_set_stride.  Descriptors are 32 bytes, rows contiguous, 16-byte aligned.
 *   idx  [n_pairs, nq_cap, 2] int32 : train index of the nearest / second nearest (-1 if absent)
 *   dist [n_pairs, nq_cap, 2] int32 : their Hamming distances (-1 if absent)
 * Rows >= nq[p] are left untouched.
 * The distances are computed on the matrix cores (descriptors expanded to +1 / -1 FP4 values: dot product = 256 - 2 dist,
 * exact).  The default kernel expands the train descriptors tile by tile on their way into LDS and needs a token
 * workspace only (mm_bf_workspace_bytes: 256 bytes, never 0; 16-byte aligned).  Train sets of fewer than 64 or of 65536
 * and more descriptors take the xor / popcount kernel instead, whose workspace holds the partial results when a small
 * launch splits its train range -- both return identical results.  MM_BF_VARIANT=114 in the environment puts the
 * xor / popcount kernel on every shape (tests, tools/bench_bf.py); 314, 0 or unset is the rule above; any other value
 * names a kernel that was removed: the compute calls return MM_ERR_ARG, the size functions answer as for the default.
 */
size_t mm_bf_workspace_bytes(int n_pairs, int nq_cap, int nt_cap);
int mm_bf_knn2_batched(mm_ctx *ctx, const uint8_t *q /*dev*/, const int32_t *nq /*dev|NULL*/, int nq_cap,
                       size_t q_set_stride, const uint8_t *t /*dev*/, const int32_t *nt /*dev|NULL*/, int nt_cap,
                       size_t t_set_stride, int n_pairs, int32_t *idx /*dev*/, int32_t *dist /*dev*/,
                       void *ws /*dev*/, size_t ws_bytes);
int mm_bf_knn2_hamming(mm_ctx *ctx, const uint8_t *q /*dev*/, int nq, const uint8_t *t /*dev*/, int nt,
                       int32_t *idx /*dev [nq,2]*/, int32_t *dist /*dev [nq,2]*/, void *ws, size_t ws_bytes);
/* Lowe ratio test, order preserving: keeps query i iff it has two neighbours and
 * (double)d0 < threshold * (double)d1  (processor.py:136-137).  pairs[p, j] = (queryIdx, trainIdx) of the
 * j-th kept match in query order; m_out[p] = number kept. */
int mm_ratio_filter_batched(mm_ctx *ctx, const int32_t *idx /*dev*/, const int32_t *dist /*dev*/,
                            const int32_t *nq /*dev|NULL*/, int nq_cap, int n_pairs, double threshold,
                            int32_t *pairs /*dev [n_pairs,nq_cap,2]*/, int32_t *m_out /*dev [n_pairs]*/);
/* The whole match stage in one call: exactly what mm_bf_knn2_batched followed by mm_ratio_filter_batched produce, without
 * idx / dist ever being stored where the kernel has the ratio test in its epilogue (the default, matrix-core kernel: one
 * int32 per query goes to the workspace instead; the xor / popcount kernel keeps idx / dist there).  Every element of pairs [n_pairs, nq_cap, 2]
 * and of m_out [n_pairs] is written: pairs[p, j] = (queryIdx, trainIdx) of the j-th kept match in query order for
 * j < m_out[p], -1 from there on -- the outputs need no initialisation.  Workspace: mm_bf_match_ratio_workspace_bytes,
 * 16-byte aligned. */
size_t mm_bf_match_ratio_workspace_bytes(int n_pairs, int nq_cap, int nt_cap);
int mm_bf_match_ratio_batched(mm_ctx *ctx, const uint8_t *q /*dev*/, const int32_t *nq /*dev|NULL*/, int nq_cap,
                              size_t q_set_stride, const uint8_t *t /*dev*/, const int32_t *nt /*dev|NULL*/, int nt_cap,
                              size_t t_set_stride, int n_pairs, double threshold,
                              int32_t *pairs /*dev [n_pairs,nq_cap,2]*/, int32_t *m_out /*dev [n_pairs]*/,
                              void *ws /*dev*/, size_t ws_bytes);

/* ---- a-1: ORB detect + describe ----------------------------------------------------------------
 * Replaces orb.detectAndCompute(img, None), processor.py:129,328 with cv2.ORB_create(nfeatures=...) defaults
 * (processor.py:308): 8 levels x1.2, FAST-9/16 t=20 + 3x3 NMS, border 31, 2n by FAST score then n by Harris,
 * intensity-centroid orientation, 7x7 sigma=2 blur, 256-bit steered BRIEF.  Integer-exact definition in DESIGN.md.
 */
typedef struct mm_orb_params {
    int32_t nfeatures;      /* processor.py:308 uses 20000; BASELINE configs 2000 / 4000 / 8000 */
    int32_t nlevels;        /* 8  */
    int32_t edge_threshold; /* 31 */
    int32_t fast_threshold; /* 20 */
    float scale_factor;     /* 1.2f */
    int32_t reserved;
} mm_orb_params;
size_t mm_orb_workspace_bytes(int batch, int height, int width, const mm_orb_params *prm);
/* imgs [batch, height, stride] u8 grey.  Outputs are per frame with capacity cap = nfeatures:
 *   kp_xy   [batch, cap, 2] f32 : level-0 coordinates (cv2.KeyPoint.pt)
 *   kp_meta [batch, cap, 4] i32 : level, x_level, y_level, harris25 (low 32 bits; debugging / parity)
 *   kp_resp [batch, cap]    f32 : Harris response (cv2.KeyPoint.response)
 *   kp_mom  [batch, cap, 2] i32 : intensity-centroid moments m10, m01 (angle = atan2(m01, m10))
 *   desc    [batch, cap, 32] u8
 *   n_out   [batch] i32
 * pattern [256*4] int8 (x0,y0,x1,y1 per bit) device pointer — the rBRIEF sampling pattern. */
int mm_orb_detect_compute(mm_ctx *ctx, const uint8_t *imgs /*dev*/, int batch, int height, int width, int stride,
                          const mm_orb_params *prm, const int8_t *pattern /*dev*/, void *ws /*dev*/, size_t ws_bytes,
                          float *kp_xy, int32_t *kp_meta, float *kp_resp, int32_t *kp_mom, uint8_t *desc,
                          int32_t *n_out);
/* Level geometry shared with the host side (and the oracle checks it): widths/heights of the nlevels levels. */
int mm_orb_level_sizes(int height, int width, const mm_orb_params *prm, int32_t *lvl_w /*host[nlevels]*/,
                       int32_t *lvl_h /*host*/, int32_t *lvl_n /*host: features per level*/,
                       float *lvl_scale /*host*/);

/* ---- a-3 / a-5: track linking and flattening (host logic, exact coordinate-equality semantics) -----
 * Replaces processor.pointTracking (processor.py:190-243) run over a whole clip plus
 * `popped_tracks += tracks` (processor.py:418) and managePoints (processor.py:264-291).
 * All pointers are HOST pointers.  kp_xy [n_frames, cap, 2] f32, matches [n_frames-1, mcap, 2] (queryIdx, trainIdx).
 * Output: CSR over tracks in the reference's final order; obs_frame / obs_kp give each observation.
 * Returns the number of tracks (>= 0) or a negative error; *n_obs_out receives the observation count.
 * If the output capacity is too small returns MM_ERR_WORKSPACE with the required sizes in *n_obs_out / return. */
int64_t mm_link_tracks_clip(int n_frames, int cap, const int32_t *kp_count, const float *kp_xy, int mcap,
                            const int32_t *match_count, const int32_t *matches, int64_t max_tracks,
                            int64_t max_obs, int64_t *track_ptr /*[max_tracks+1]*/, int32_t *obs_frame,
                            int32_t *obs_kp, int64_t *n_obs_out);
/* The same linking ON THE DEVICE (one resident workgroup walks the clip; scatter-min / scatter-max / prefix sums per
 * keyframe pair): all pointers are DEVICE pointers, nothing is copied to the host, no synchronisation.
 * kp_xy [n_frames, cap, 2] f32, matches [n_frames-1, cap, 2] i32 (queryIdx, trainIdx), cap <= 8192.
 * Outputs sized for the worst case: track_ptr [(n_frames-1)*cap + 1] i32, obs_frame / obs_kp [2*(n_frames-1)*cap] i32;
 * counts [3] i64 = (n_tracks, n_obs, 1 if a malformed match was skipped).  Same result as mm_link_tracks_clip. */
size_t mm_link_workspace_bytes(int n_frames, int cap);
int mm_link_tracks_device(mm_ctx *ctx, int n_frames, int cap, const int32_t *kp_count, const float *kp_xy,
                          const int32_t *match_count, const int32_t *matches, void *ws, size_t ws_bytes,
                          int32_t *track_ptr, int32_t *obs_frame, int32_t *obs_kp, int64_t *counts /*dev[3]*/);
/* managePoints ON THE DEVICE (processor.py:264-291): the flat observation arrays of a selection of tracks, point-major,
 * insertion order inside a track -- what adjustPoints takes (bundleAdjuster.py:160-166).  All pointers are DEVICE pointers.
 *   selection: sel == NULL: the n_sel tracks t_lo .. t_lo + n_sel - 1 (everything, or one rank's shard);
 *              sel [n_sel] i32: these tracks in this order (a sliding window), with out_ptr [n_sel + 1] i64 = the exclusive
 *              scan of their lengths from mm_flatten_offsets (out_ptr[n_sel] = number of observations: read it back to size
 *              the outputs);
 *   coords [n_obs, 2] f64 = kp_xy[obs_frame, obs_kp] (kp_xy [F, cap, 2] f32); frame_indices [n_obs] i32 = obs_frame -
 *   frame_offset; point_indices [n_obs] i32 = position of the observation's track in the selection. */
int mm_flatten_offsets(mm_ctx *ctx, const int32_t *track_ptr, const int32_t *sel, int64_t n_sel, int64_t *out_ptr);
int mm_flatten_tracks(mm_ctx *ctx, const int32_t *track_ptr, const int32_t *obs_frame, const int32_t *obs_kp, const float *kp_xy,
                      int cap, const int32_t *sel /*|NULL*/, int t_lo, int64_t n_sel, const int64_t *out_ptr /*|NULL*/, int64_t n_obs,
                      int frame_offset, double *coords, int32_t *frame_indices, int32_t *point_indices);
/* Host: co-observation pairs (o, o2) of one point with camera(o2) <= camera(o), grouped by block segment
 * camera(o) * (span + 1) + camera(o) - camera(o2) in a fixed canonical order.  seg_ptr [F*(span+1)+1].  Call with
 * pair_o == NULL to get the pair count.  Returns the count or a negative error (MM_ERR_ARG if span is too small). */
int64_t mm_ba_build_pairs(int F, int P, int64_t O, const int32_t *fi, const int32_t *pi, const int32_t *pt_ptr,
                          const int32_t *pt_obs, const int32_t *cam_ptr, const int32_t *cam_obs, int span,
                          int64_t *seg_ptr, int32_t *pair_o, int32_t *pair_o2, int64_t max_pairs);
/* Host index build for BA: CSR of observations by point and by camera (stable). */
int mm_ba_build_index(int F, int P, int64_t O, const int32_t *fi, const int32_t *pi, int32_t *pt_ptr /*[P+1]*/,
                      int32_t *pt_obs /*[O]*/, int32_t *cam_ptr /*[F+1]*/, int32_t *cam_obs /*[O]*/);

/* ---- a-2b: epipolar verification of the matches of consecutive frame pairs (no reference counterpart) -------------
 * A fundamental matrix per frame pair, estimated robustly (RANSAC with the MSAC score), and the matches that agree with it:
 * the stage between mm_ratio_filter_batched and mm_link_tracks_device.  It needs no poses and no calibration.
 *   Inputs.  Pair p joins frame p (query) and frame p + 1 (train) of a block of n_pairs + 1 frames: kp_xy [n_pairs+1, cap, 2]
 *   f32, pairs [n_pairs, cap, 2] i32 = (queryIdx, trainIdx), m [n_pairs] i32 (clamped to 0 .. cap) -- what
 *   mm_ratio_filter_batched writes.  Match j gives x = kp_xy[p, q_j], x' = kp_xy[p+1, t_j], widened to f64; the convention is
 *   x'^T F x = 0 on homogeneous pixels, F row-major.  A match with an index outside [0, cap) is MALFORMED: never an inlier, a
 *   hypothesis that samples it is invalid, the pair is flagged, nothing is read through the index.
 *   Distance.  Sampson: d^2 = (x'^T F x)^2 / ((F x)_0^2 + (F x)_1^2 + (F^T x')_0^2 + (F^T x')_1^2); a match is an inlier when
 *   d^2 is finite and d^2 <= tau^2, tau = threshold_px.
 *   Score.  MSAC: cost(F) = sum_j (inlier_j ? d_j^2 : tau^2) -- a malformed match contributes tau^2 -- continuous in F, so the
 *   winner does not hinge on a match on the threshold.  An invalid hypothesis costs +inf.  The lowest FINITE cost wins, ties go
 *   to the lowest h.
 *   Normalisation (Hartley), per image, over all well-formed matches of the pair: centroid c, mean distance dbar to c,
 *   s = sqrt(2) / dbar, T = [[s, 0, -s c_x], [0, s, -s c_y], [0, 0, 1]].  A non-finite s (all points equal, no well-formed
 *   match) leaves the pair without a valid hypothesis.
 *   Sampling, integers only (arithmetic mod 2^32):  pcg(v): s = v * 747796405 + 2891336453;
 *   w = ((s >> ((s >> 28) + 4)) ^ s) * 277803737;  return (w >> 22) ^ w.   Hypothesis h of pair p:
 *   base = pcg(pcg(seed + pcg(pair_base + p)) + h); pick k = 0 .. 7 tries a = 0 .. 7: i = (uint64(pcg(base + 8 k + a)) * m) >> 32
 *   and takes the first i that is not among the earlier picks; eight collisions make the hypothesis invalid (at most (7/16)^8
 *   per pick for m >= 16: why min_matches is floored at 16).  pair_base is the global index of pair 0 of the call, so a
 *   rank's block of pairs gives the rows the whole clip would give.
 *   Hypothesis.  The eight normalised matches give the rows [x'x, x'y, x', y'x, y'y, y', x, y, 1]; f is the unit right null
 *   vector of that 8 x 9 matrix (rows orthonormalised in registers, twice each; the null vector is the largest column of
 *   I - Q^T Q); rank 2: F^ <- F^ - (F^ v3) v3^T with v3 the eigenvector of the smallest eigenvalue of F^^T F^ (3 x 3 cyclic
 *   Jacobi); F = T'^T F^ T scaled to unit Frobenius norm; a non-finite F makes the hypothesis invalid.
 *   Refit.  refit_iters rounds (a fixed count): take the inliers of the current F -- fewer than 8: nothing changes any more --
 *   normalise over them, M = A^T A (9 x 9) over them, f = eigenvector of the smallest eigenvalue of M (cyclic Jacobi, a
 *   rotation skipped once |m_pq| <= eps sqrt(m_pp m_qq)), rank 2, denormalise, unit norm; the refit replaces F only if it is
 *   finite and its cost over ALL matches is finite and strictly lower.
 *   Outputs.  pairs_out [n_pairs, cap, 2] (must not alias pairs): the inliers of the final F in their input order, m_out
 *   [n_pairs] their number; rows at or beyond m_out[p] are left untouched.  Fm [n_pairs, 9] f64 unit norm (NaN: no model),
 *   cost [n_pairs] f64 of the final F (NaN: no model), info [n_pairs, 4] i32 = (flags, n_inliers, best_h or -1, number of valid
 *   hypotheses).
 *   Flags.  MM_VERIFY_TOO_FEW m < max(min_matches, 16): no RANSAC is run | MM_VERIFY_NO_MODEL no hypothesis with a finite
 *   cost | MM_VERIFY_WEAK n_inliers < min_inliers | MM_VERIFY_MALFORMED.  The first three are failures: on_fail = 0 passes all
 *   m matches of the pair through unchanged (a malformed one included -- the flag says so), on_fail = 1 drops them (m_out = 0).
 * Sums run in an order that depends on the pair alone (per-thread strides, fixed trees), no atomics: a call repeats bit for
 * bit, a pair's row does not depend on which other pairs share the call, and rows [a, b) of a call equal a call on that
 * sub-block with pair_base + a.  n_pairs = 0 returns MM_OK without a launch.  All pointers are DEVICE pointers except prm;
 * kp_xy, pairs and pairs_out 8-byte aligned; ws holds mm_verify_workspace_bytes(n_pairs, n_hyp) bytes (normalisations, every
 * hypothesis' F and cost).  Argument errors -- n_hyp outside 1 .. 4096, a negative or NaN threshold_px, null pointers:
 * MM_ERR_ARG; a workspace that is too small: MM_ERR_WORKSPACE -- are returned before the device is touched. */
#define MM_VERIFY_TOO_FEW 1
#define MM_VERIFY_NO_MODEL 2
#define MM_VERIFY_WEAK 4
#define MM_VERIFY_MALFORMED 8
typedef struct mm_verify_params {
    int32_t n_hyp, min_matches, min_inliers, refit_iters;
    uint32_t seed, pair_base;
    int32_t on_fail, reserved;
    double threshold_px;
} mm_verify_params;
size_t mm_verify_workspace_bytes(int n_pairs, int n_hyp);
int mm_verify_matches(mm_ctx *ctx, const float *kp_xy /*[n_pairs+1,cap,2]*/, const int32_t *pairs /*[n_pairs,cap,2]*/,
                      const int32_t *m /*[n_pairs]*/, int n_pairs, int cap, const mm_verify_params *prm,
                      int32_t *pairs_out /*[n_pairs,cap,2]*/, int32_t *m_out /*[n_pairs]*/, double *Fm /*[n_pairs,9]*/,
                      double *cost /*[n_pairs]*/, int32_t *info /*[n_pairs,4]*/, void *ws, size_t ws_bytes);

/* ---- a-2c: camera poses from the verified matches (no reference counterpart: the reference reads every keyframe's pose off
 * a chessboard) -------------------------------------------------------------------------------------------------------------
 * mm_recover_poses: the relative pose of every consecutive frame pair from that pair's fundamental matrix, the calibration and
 * the pair's inlier matches; mm_chain_poses: the pairs chained into one set of extrinsics [n_pairs+1, 3, 4] that goes into
 * mm_triangulate_tracks and the adjustment.
 *   Inputs.  K [9] f64 HOST, row-major, upper triangular with K[8] = 1; kp_xy [n_pairs+1, cap, 2] f32; pairs [n_pairs, cap, 2]
 *   i32 and m [n_pairs] (clamped to 0 .. cap): what mm_verify_matches wrote to pairs_out / m_out; Fm [n_pairs, 9] f64 with
 *   x'^T F x = 0.  Pair p joins frame p (query, camera 1) and frame p + 1 (train, camera 2).
 *   Convention.  A point X1 in camera-1 coordinates is X2 = R X1 + t in camera 2, |t| = 1.
 *   Decomposition (no SVD).  E = K^T (F K), G = E^T E; eigen-decomposition of G by the 3 x 3 cyclic Jacobi of
 *   mm_verify_matches' rank-2 step (pairs (0,1), (0,2), (1,2) per sweep, a rotation skipped once |g_pq| <= eps sqrt(|g_pp g_qq|),
 *   at most 30 sweeps, V starts as the identity).  v3 = eigenvector of the smallest eigenvalue, v1 of the largest, ties to the
 *   lowest column; v2 = v3 x v1; u1 = E v1 / s1, s1 = |E v1|; u2 = (E v2 - (u1 . E v2) u1) / s2, s2 that vector's norm;
 *   u3 = u1 x u2.  U = [u1 u2 u3] and V = [v1 v2 v3] have determinant +1 by construction.  W = [[0,-1,0],[1,0,0],[0,0,1]],
 *   Ra = U W V^T, Rb = U W^T V^T; candidates c = 0 .. 3 are (Ra, +u3), (Ra, -u3), (Rb, +u3), (Rb, -u3).
 *   Depths.  K^-1 is formed once on the host, in closed form: with K = [[fx, s, cx], [0, fy, cy], [0, 0, 1]],
 *   K^-1 = [[1/fx, -s/(fx fy), (s cy - cx fy)/(fx fy)], [0, 1/fy, -cy/fy], [0, 0, 1]].  A match has the rays
 *   a = K^-1 (x, y, 1) and b = K^-1 (x', y', 1); with r = R a: det = (r.r)(b.b) - (r.b)^2,
 *   l1 = ((r.b)(b.t) - (r.t)(b.b)) / det, l2 = ((r.r)(b.t) - (r.b)(r.t)) / det -- the least-squares solution of
 *   l2 b = l1 r + t, the depths along a and b.  A match votes for c when both depths are finite and > 0.  A match with an
 *   index outside [0, cap) is MALFORMED: it never votes and nothing is read through it.
 *   Winner.  The largest vote count, ties to the lowest c.
 *   Outputs.  R [n_pairs, 9] row-major and t [n_pairs, 3] f64 of the winner (NaN: no model); sigma [n_pairs, 2] = (s1, s2) --
 *   a true essential matrix has s1 = s2, so the caller sees how far F and K disagree (NaN for a pair with too few matches);
 *   depth [n_pairs, cap, 2] f64 = (l1, l2) under the winner for every row that voted for it, NaN in every other row, rows at
 *   or beyond m[p] included; info [n_pairs, 8] i32 = (flags, winner or -1, votes[0 .. 3], m used, 0).
 *   Flags.  MM_POSE_TOO_FEW m < max(min_matches, 8): nothing is decomposed | MM_POSE_NO_MODEL a non-finite F, or s1 or s2 not
 *   finite and positive | MM_POSE_AMBIGUOUS votes[winner] < min_front_frac m, or the runner-up has >= ambiguous_frac
 *   votes[winner] (rotation-only and planar pairs land here; R and t are still written) | MM_POSE_MALFORMED.
 * One 256-thread workgroup per pair, integer counts: a call repeats bit for bit and a pair's row does not depend on which
 * other pairs share the call.  n_pairs = 0 returns MM_OK without a launch.  kp_xy and pairs 8-byte aligned, depth 16-byte.
 * Null pointers, cap <= 0, a K that is not finite / upper triangular / K[8] = 1 or has a zero focal length, and fractions
 * outside [0, 1] return MM_ERR_ARG before the device is touched. */
#define MM_POSE_TOO_FEW 1
#define MM_POSE_NO_MODEL 2
#define MM_POSE_AMBIGUOUS 4
#define MM_POSE_MALFORMED 8
typedef struct mm_pose_params {
    int32_t min_matches, reserved;
    double min_front_frac, ambiguous_frac;      /* defaults 0.5, 0.5 */
} mm_pose_params;
int mm_recover_poses(mm_ctx *ctx, const double *K /*host [9]*/, const float *kp_xy /*[n_pairs+1,cap,2]*/,
                     const int32_t *pairs /*[n_pairs,cap,2]*/, const int32_t *m /*[n_pairs]*/, const double *Fm /*[n_pairs,9]*/,
                     int n_pairs, int cap, const mm_pose_params *prm, double *R /*[n_pairs,9]*/, double *t /*[n_pairs,3]*/,
                     double *sigma /*[n_pairs,2]*/, double *depth /*[n_pairs,cap,2]*/, int32_t *info /*[n_pairs,8]*/);
/* One scale and one coordinate frame for the pairs of mm_recover_poses.  pairs, m, depth, R, t, info as above -- all of them
 * inputs --, cap <= 8192; E0 [12] f64 HOST: the first frame's extrinsic; min_common >= 0.
 *   Scale ratio of pair p >= 1 against pair p - 1.  Key point k of frame p is a train of pair p - 1 and a query of pair p.
 *   prev(k) = the lowest row i < m[p-1] of pair p - 1 with train k and depth[p-1, i, 1] finite and > 0.  Every row j < m[p]
 *   of pair p whose query has a prev and whose depth[p, j, 0] is finite and > 0 gives rho_j = depth[p-1, prev, 1] /
 *   depth[p, j, 0] (one IEEE division); rho_p is the lower median of those n_common values, the (n_common - 1) / 2-th
 *   smallest.  An index outside [0, cap) has no prev and gives no ratio.
 *   Flags (chain_info [n_pairs, 2] i32 = (flags, n_common)).  MM_CHAIN_BROKEN: the pair has MM_POSE_TOO_FEW or
 *   MM_POSE_NO_MODEL; its motion is taken as identity rotation and zero translation, rho_p = 1, n_common = 0, and the next
 *   pair is MM_CHAIN_FEW_COMMON with n_common = 0.  MM_CHAIN_FEW_COMMON: n_common < min_common; rho_p = 1, the previous scale
 *   is carried.  Pair 0 has no ratio: rho_0 = 1, n_common = 0, no flag.  An AMBIGUOUS pair is chained as it is.
 *   Composition, in this order: s_0 = 1 (times rho_0), s_p = s_{p-1} rho_p; T_0 = E0;
 *   T_{p+1} = [R_p T_p[:, :3] | R_p T_p[:, 3] + s_p t_p], every dot product summed left to right.
 *   Outputs.  extrinsics [n_pairs+1, 3, 4], scale [n_pairs] = s_p, rho [n_pairs], chain_info.
 * The median is an element of the set (a radix select on the bit patterns), the only atomics are integer min / add: the
 * result repeats bit for bit.  n_pairs = 0 returns MM_OK without a launch (extrinsics is not written).  Null pointers, cap
 * outside 1 .. 8192 and a negative min_common return MM_ERR_ARG before the device is touched. */
#define MM_CHAIN_FEW_COMMON 1
#define MM_CHAIN_BROKEN 2
int mm_chain_poses(mm_ctx *ctx, const int32_t *pairs /*[n_pairs,cap,2]*/, const int32_t *m /*[n_pairs]*/,
                   const double *depth /*[n_pairs,cap,2]*/, const double *R /*[n_pairs,9]*/, const double *t /*[n_pairs,3]*/,
                   const int32_t *info /*[n_pairs,8]*/, int n_pairs, int cap, const double *E0 /*host [12]*/, int min_common,
                   double *extrinsics /*[n_pairs+1,3,4]*/, double *scale /*[n_pairs]*/, double *rho /*[n_pairs]*/,
                   int32_t *chain_info /*[n_pairs,2]*/);

/* ---- a-2d: camera registration against existing 3-D points, a RANSAC resection (PnP) per camera ---------------------------------
 * Reference counterpart: the pose source cv2.solvePnP(..., SOLVEPNP_ITERATIVE) at processor.py:175 (there on the chessboard; the
 * refinement that follows it, adjustPose, is the adjustment with fixed points).  Every camera of the call is estimated from the
 * 3-D points it observes; cameras do not see each other.
 *   Inputs.  K [9] f64 HOST, row-major, upper triangular with K[8] = 1; K^-1 in closed form as in mm_recover_poses.  X [P, 3] f64,
 *   obs [O, 2] f64 pixels, pi [O] i32: observation o sees point pi[o] at obs[o].  The camera CSR cam_ptr [n_cams+1], cam_obs
 *   [n_rows] i32 -- the arrays an mm_ba_problem carries: row q in cam_ptr[c] .. cam_ptr[c+1] - 1 (clamped to 0 .. n_rows) of
 *   camera c is observation o = cam_obs[q].  pt_ok [P] u8 or NULL (every point usable).  prior [n_cams, 12] f64 or NULL: one
 *   [R|t] per camera; a prior with a non-finite entry counts as absent.
 *   Usable rows.  A row is usable when o is in [0, O), pi[o] in [0, P), obs[o] and X[pi[o]] are finite and pt_ok is NULL or
 *   pt_ok[pi[o]] != 0.  An index out of range or a non-finite pixel also sets MALFORMED; nothing is read through a bad index.  A
 *   masked-out or non-finite point is skipped without a flag.  The usable rows of a camera are compacted once, order preserved;
 *   n_use is their number and everything below works on the compacted list only, so sampling never meets an unusable row.
 *   Normalisation, per camera over its usable rows: centroid c (each coordinate sum / n_use), dbar the mean of
 *   sqrt(((X-c)_0^2 + (X-c)_1^2) + (X-c)_2^2), s = sqrt(3) / dbar, X^ = (s (X - c), 1).  The image side is calibrated:
 *   u = (Ki0 x + Ki1 y) + Ki2, v = Ki3 y + Ki4.
 *   Sampling, the integer scheme of mm_verify_matches with six picks: base = pcg(pcg(seed + pcg(cam_base + c)) + h); pick
 *   k = 0 .. 5 tries a = 0 .. 7: i = (uint64(pcg(base + 8 k + a)) * n_use) >> 32 and takes the first i that is not an earlier
 *   pick; eight collisions make the hypothesis invalid (at most (5/12)^8 < 1e-3 per pick for n_use >= 12: why min_rows is floored
 *   at 12).  cam_base is the global index of camera 0 of the call.
 *   Hypothesis and refit -- one routine, a reduced DLT without SVD and without a 12 x 12 system.  Over the chosen rows, in their
 *   order, four symmetric 4 x 4 sums (upper triangles, 40 numbers): with w_ij = X^_i X^_j, S += w, Bu += u w, Bv += v w,
 *   C += (u u + v v) w.  Cholesky S = L L^T, column by column, each entry reduced by its products left to right; a pivot that is
 *   not finite or <= 1e-12 times the diagonal entry it started from makes the hypothesis invalid (planar and otherwise
 *   degenerate samples leave here).  Yu = L^-1 Bu, Yv = L^-1 Bv (forward substitution), M = (C - Yu^T Yu) - Yv^T Yv; p3 = the
 *   eigenvector of the smallest eigenvalue of M, ties to the lowest column (4 x 4 cyclic Jacobi, pairs (p, q) ascending, a
 *   rotation skipped once |m_pq| <= eps sqrt(|m_pp m_qq|), at most 30 sweeps); p1 = L^-T (Yu p3), p2 = L^-T (Yv p3).
 *   P = [p1; p2; p3] T with T = [[s I, -s c], [0, 1]]: A = P[:, :3] = s [p1; p2; p3][:, :3], b = [p1; p2; p3][:, 3]; both
 *   negated when det A < 0.  3 x 3 Jacobi on A^T A gives lambda and V; a lambda that is not finite and positive is invalid.
 *   R = A (V diag(lambda^-1/2) V^T), sigma = ((sqrt l0 + sqrt l1) + sqrt l2) / 3, t = b / sigma - R c; a non-finite entry is
 *   invalid.  (For an exact scaled rotation A that t is P[:, 3] / sigma = (b - A c) / sigma; taken about the centroid, what the
 *   polar step removes from a noisy A is not multiplied by the distance of the points from the world's origin.)
 *   Score.  Q = K [R|t], y = Q (X, 1), d^2 = (y0/y2 - x)^2 + (y1/y2 - y)^2; a row is an inlier iff y2 > 0 and d^2 is finite and
 *   <= tau^2, tau = threshold_px.  MSAC: cost = sum over the usable rows of (inlier ? d^2 : tau^2); an invalid hypothesis costs
 *   +inf.  The hypotheses are ranked by that sum taken over the rows ascending; the lowest finite cost wins, ties go to the
 *   lowest h.  Every cost from here on -- the winner's, the prior's, a refit's, the polished pose's -- is the same sum in the
 *   workgroup's fixed order.  A present prior competes as hypothesis number n_hyp: it replaces the winner only with a finite,
 *   strictly lower cost (or when there is none).
 *   Refit.  refit_iters rounds (a fixed count) of the reduced DLT over the inliers of the current model, with the camera's
 *   normalisation; fewer than 6 inliers: nothing changes any more.  A refit is accepted only when it is valid and its cost over
 *   ALL usable rows is finite and strictly lower.
 *   Polish.  polish_iters Levenberg-Marquardt TRIAL steps on sum |r|^2 over the inlier set fixed at entry, with Y = R X + t,
 *   r = ((fx Y0 + sk Y1) / Y2 + cx - x, fy Y1 / Y2 + cy - y).  The update is R <- cay(w) R, t <- t + dt with the Cayley map
 *   cay(w) = ((1 - a.a) I + 2 a a^T + 2 [a]x) / (1 + a.a), a = w / 2 -- rational, so the whole estimator uses + * / sqrt only.
 *   J = J_pi(Y) [ -[Y - t]x | I ], H = sum J^T J, g = sum J^T r, (H + lambda diag H) delta = -g by 6 x 6 Cholesky (a pivot
 *   that is not positive fails the trial); lambda = 1e-3 at the start, accept / reject and the lambda schedule as in
 *   mm_triangulate_tracks.  A trial is accepted only if every row of the set keeps Y2 > 0 and the cost is finite and strictly
 *   lower.  The polished pose replaces the model only if it is finite and its MSAC cost over all usable rows is strictly lower;
 *   info then carries the number of accepted trials, otherwise 0.
 *   Outputs.  extrinsics [n_cams, 3, 4] f64; cost [n_cams] f64 (NaN: no model); inlier [O] u8, written at o for every usable
 *   or malformed (o in range) row of a camera and left untouched elsewhere; info [n_cams, 6] i32 = (flags, n_inliers, best_h or
 *   -1 (n_hyp: the prior), valid hypotheses, n_use, accepted polish steps).
 *   Flags.  MM_RESECT_TOO_FEW n_use < max(min_rows, 12): no RANSAC is run | MM_RESECT_NO_MODEL no finite-cost hypothesis, the
 *   prior included | MM_RESECT_WEAK n_inliers < min_inliers | MM_RESECT_MALFORMED.  On TOO_FEW or NO_MODEL the camera's
 *   extrinsic is the prior when present, else NaN, and its inlier rows are 0.
 * Sums run in an order that depends on the camera alone (per-thread strides, fixed trees), no atomics: a call repeats bit for
 * bit, a camera's row does not depend on which other cameras share the call, and rows [a, b) of a call equal a call on that
 * block with cam_base + a.  n_cams = 0 returns MM_OK without a launch.  All pointers are DEVICE pointers except K and prm; ws
 * holds mm_resect_workspace_bytes(n_cams, n_hyp, n_rows) bytes.  Argument errors -- n_hyp outside 1 .. 4096, a negative or NaN
 * threshold_px, null pointers, a K that is not finite / upper triangular / K[8] = 1 or has a zero focal length: MM_ERR_ARG; a
 * workspace that is too small: MM_ERR_WORKSPACE -- are returned before the device is touched. */
#define MM_RESECT_TOO_FEW 1
#define MM_RESECT_NO_MODEL 2
#define MM_RESECT_WEAK 4
#define MM_RESECT_MALFORMED 8
typedef struct mm_resect_params {
    int32_t n_hyp, min_rows, min_inliers, refit_iters, polish_iters, reserved;      /* defaults 256, 12, 12, 2, 8 */
    uint32_t seed, cam_base;
    double threshold_px;                                                            /* default 2 */
} mm_resect_params;
size_t mm_resect_workspace_bytes(int n_cams, int n_hyp, int64_t n_rows);
int mm_resect_cameras(mm_ctx *ctx, const double *K /*host [9]*/, const double *X /*[P,3]*/, int64_t P, const double *obs /*[O,2]*/,
                      const int32_t *pi /*[O]*/, int64_t O, const int32_t *cam_ptr /*[n_cams+1]*/,
                      const int32_t *cam_obs /*[n_rows]*/, int64_t n_rows, int n_cams, const uint8_t *pt_ok /*[P] or NULL*/,
                      const double *prior /*[n_cams,12] or NULL*/, const mm_resect_params *prm, double *extrinsics /*[n_cams,3,4]*/,
                      double *cost /*[n_cams]*/, uint8_t *inlier /*[O]*/, int32_t *info /*[n_cams,6]*/, void *ws, size_t ws_bytes);

/* ---- a-2e: planar resection, the pose of a camera over coplanar points by a RANSAC homography ----------------------------------
 * Reference counterpart: the same cv2.solvePnP(..., SOLVEPNP_ITERATIVE) at processor.py:175, on the data it is actually given: the
 * corners of a flat chessboard, where the reduced DLT of mm_resect_cameras has no valid sample.  A camera whose usable points are
 * coplanar is estimated from the homography between their plane and the calibrated image; any other camera is refused and left
 * as it was, so that this call can be laid over a mm_resect_cameras call on the same buffers.
 *   Inputs, usable rows, compaction, the calibrated image side (u, v), cam_base, the prior as hypothesis n_hyp, score, MSAC
 *   ranking, polish and every argument check: exactly as in mm_resect_cameras.  min_rows is floored at 8 (four picks out of
 *   n_use >= 8 with eight tries collide with chance at most (3/8)^8 < 1e-3 per pick).
 *   Plane fit, per camera over its usable rows: centroid c (each coordinate sum / n_use); the six sums of (X - c)(X - c)^T (xx,
 *   xy, xz, yy, yz, zz) in the workgroup's fixed order; 3 x 3 cyclic Jacobi (the one of mm_resect_cameras); the three eigenpairs
 *   are ordered ascending, l0 <= l1 <= l2, by a stable exchange sort of the columns -- (0,1), (1,2), (0,1), each exchanged only
 *   when the right eigenvalue is strictly smaller.  n = the eigenvector of l0, e1 = that of l2, e2 = n x e1: (e1, e2, n) is a
 *   rotation whatever signs the Jacobi returns.
 *   Verdicts, in this order.  n_use < max(min_rows, 8): TOO_FEW, refused.  Collinear: l2 is not finite and positive, or l1 is not
 *   above 1e-12 l2: PLANAR | NO_MODEL.  Planar: l0 <= planar_tol^2 l1: PLANAR, the branch below runs.  Anything else is not
 *   planar and refused (no flag but MALFORMED where that applies).
 *   Plane coordinates: with d = X - c, a = (d0 e1_0 + d1 e1_1) + d2 e1_2, b likewise with e2; rbar the mean of sqrt(a a + b b),
 *   s = sqrt(2) / rbar, m = (s a, s b, 1).
 *   Sampling: the integer scheme of mm_resect_cameras with four picks (same base; pick k = 0 .. 3, tries 0 .. 7 on
 *   pcg(base + 8 k + try)).  A sample is also invalid when any of its four triples (0,1,2), (0,1,3), (0,2,3), (1,2,3) is
 *   near-collinear: with p = m_j - m_i, q = m_k - m_i, r = m_k - m_j the triple passes only if
 *   |p_a q_b - p_b q_a| > collinear_tol * max(|p|^2, |q|^2, |r|^2) (a NaN does not pass).  Refits skip this test.
 *   Hypothesis and refit -- one routine, the reduced DLT of mm_resect_cameras one dimension down.  Over the chosen rows, in
 *   their order, four symmetric 3 x 3 sums (upper triangles, 24 numbers): with w_ij = m_i m_j, S += w, Bu += u w, Bv += v w,
 *   C += (u u + v v) w.  Cholesky S = L L^T with the same pivot rule; Yu = L^-1 Bu, Yv = L^-1 Bv; M = (C - Yu^T Yu) - Yv^T Yv;
 *   h3 = the eigenvector of the smallest eigenvalue of M, ties to the lowest column (3 x 3 Jacobi); h1 = L^-T (Yu h3),
 *   h2 = L^-T (Yv h3).  H = [h1; h2; h3] (rows), negated when H[2][2] < 0 (the centroid in front).
 *   Pose from H: columns g1, g2, g3; sigma = (|g1| + |g2|) / 2 with |g| = sqrt((g0 g0 + g1 g1) + g2 g2);
 *   A = [g1, g2, (g1 x g2) / sigma] (columns); R' = A (V diag(lambda^-1/2) V^T) from the 3 x 3 Jacobi of A^T A (a lambda that is
 *   not finite and positive is invalid, and so is an A whose smallest sqrt(lambda) is not above 1e-4 times its largest: a
 *   homography of rank one or two, whose polar factor is no rotation); R = R' [e1 e2 n]^T; t = g3 / (sigma s) - R c, the about-the-centroid form of
 *   mm_resect_cameras.  A non-finite entry is invalid.  det A = |g1 x g2|^2 / sigma > 0: R is a rotation.
 *   Refit: over the inliers of the current model, at least 4 of them, accepted only when valid with a finite, strictly lower
 *   cost over ALL usable rows.  The second (flipped) pose of a plane seen nearly fronto-parallel is not searched for.
 *   Score, ranking, prior, polish: the code of mm_resect_cameras on Q = K [R|t] and the 3-D points; the polished pose is a
 *   pose, not a homography.
 *   Outputs.  extrinsics, cost, inlier, info as in mm_resect_cameras, and plane [n_cams, 6] f64 = (n, n . c,
 *   thickness sqrt(max(l0, 0) / l1), aspect sqrt(l1 / l2)), written for every camera from the fit over its usable rows (NaN where
 *   that has none).  Flags: the four of mm_resect_cameras and MM_RESECT_PLANAR: the camera's usable points passed the
 *   coplanarity test (or are collinear, then with NO_MODEL).  A camera without that bit was refused: its extrinsic is the prior
 *   when present, else NaN, its cost NaN, its info row (flags, 0, -1, 0, n_use, 0), and its inlier rows are left UNTOUCHED.  For
 *   a camera with the bit the inlier rows are written as mm_resect_cameras writes them.
 * The guarantees of mm_resect_cameras hold: a call repeats bit for bit, a camera's row does not depend on its neighbours, rows
 * [a, b) equal a call on that block with cam_base + a; n_cams = 0 returns MM_OK without a launch.  ws holds
 * mm_resect_planar_workspace_bytes(n_cams, n_hyp, n_rows) bytes.  Argument errors as in mm_resect_cameras, and a planar_tol or
 * collinear_tol that is negative or not finite: MM_ERR_ARG, before the device is touched. */
#define MM_RESECT_PLANAR 16
typedef struct mm_resect_planar_params {
    int32_t n_hyp, min_rows, min_inliers, refit_iters, polish_iters, reserved;      /* defaults 256, 8, 12, 2, 8 */
    uint32_t seed, cam_base;
    double threshold_px;                                                            /* default 2 */
    double planar_tol, collinear_tol;                                               /* defaults 1e-2, 1e-3 */
} mm_resect_planar_params;
size_t mm_resect_planar_workspace_bytes(int n_cams, int n_hyp, int64_t n_rows);
int mm_resect_planar(mm_ctx *ctx, const double *K /*host [9]*/, const double *X /*[P,3]*/, int64_t P, const double *obs /*[O,2]*/,
                     const int32_t *pi /*[O]*/, int64_t O, const int32_t *cam_ptr /*[n_cams+1]*/,
                     const int32_t *cam_obs /*[n_rows]*/, int64_t n_rows, int n_cams, const uint8_t *pt_ok /*[P] or NULL*/,
                     const double *prior /*[n_cams,12] or NULL*/, const mm_resect_planar_params *prm,
                     double *extrinsics /*[n_cams,3,4]*/, double *cost /*[n_cams]*/, uint8_t *inlier /*[O]*/,
                     int32_t *info /*[n_cams,6]*/, double *plane /*[n_cams,6]*/, void *ws, size_t ws_bytes);

/* ---- a-2f: a homography per consecutive frame pair -- the planar / rotation-only verdict and the motion (no reference
 * counterpart) ----------------------------------------------------------------------------------------------------------------
 * A fundamental matrix is not determined when the camera only turns or when the scene is a plane: mm_verify_matches then
 * returns WEAK or an arbitrary F of the pencil, and mm_recover_poses flags AMBIGUOUS.  A homography explains exactly those
 * pairs.  mm_verify_homography estimates one per pair on the same raw matches mm_verify_matches reads (not on its inliers)
 * and compares the two inlier counts; mm_recover_poses_homography turns H and the calibration into R, t, depths and an info
 * row in the layouts mm_chain_poses consumes.
 *   Inputs, malformed matches, Hartley normalisation per image over all well-formed matches, the MSAC score and its tie rule:
 *   exactly as in mm_verify_matches.
 *   Convention.  x' ~ H x on homogeneous pixels, H row-major with unit Frobenius norm, negated when (H c)_2 < 0 with
 *   (H c)_2 = (H6 c_x + H7 c_y) + H8 and c the image-1 centroid of the normalisation the fit ran under.
 *   Distance.  Symmetric transfer: y = H (x, 1) with y_i = (H_i0 x + H_i1 y) + H_i2, z = adj(H) (x', 1) likewise, adj the
 *   adjugate written out (A00 = H4 H8 - H5 H7, A01 = H2 H7 - H1 H8, A02 = H1 H5 - H2 H4, A10 = H5 H6 - H3 H8,
 *   A11 = H0 H8 - H2 H6, A12 = H2 H3 - H0 H5, A20 = H3 H7 - H4 H6, A21 = H1 H6 - H0 H7, A22 = H0 H4 - H1 H3: no division by
 *   the determinant); d^2 = (((x' - y0/y2)^2 + (y' - y1/y2)^2) + ((x - z0/z2)^2 + (y - z1/z2)^2)) * 0.5.  A match is an inlier
 *   iff d^2 is finite and <= tau^2, tau = threshold_px.
 *   Sampling: the integer scheme of mm_resect_planar with four picks: base = pcg(pcg(seed + pcg(pair_base + p)) + h); pick
 *   k = 0 .. 3 tries a = 0 .. 7: i = (uint64(pcg(base + 8 k + a)) * m) >> 32, the first i that is not an earlier pick; eight
 *   collisions make the hypothesis invalid (at most (3/8)^8 < 1e-3 per pick for m >= 8: why min_matches is floored at 8).
 *   A sample is also invalid when any of its four triples (0,1,2), (0,1,3), (0,2,3), (1,2,3) is near-collinear in either
 *   image's normalised coordinates -- the rule of mm_resect_planar with collinear_tol; a NaN does not pass.
 *   Hypothesis and refit -- one routine, the reduced DLT of mm_resect_planar with m = (s (x - c), 1) in the place of the plane
 *   coordinates and (u, v) = s' (x' - c'): the 24 sums over the chosen matches in their order, Cholesky S = L L^T with the same
 *   pivot rule, Yu, Yv, M = (C - Yu^T Yu) - Yv^T Yv, h3 = the eigenvector of the smallest eigenvalue of M (3 x 3 Jacobi, ties to
 *   the lowest column), h1 = L^-T (Yu h3), h2 = L^-T (Yv h3), H^ = [h1; h2; h3].  Rank guard: the hypothesis is invalid unless
 *   the smallest eigenvalue of H^^T H^ (3 x 3 Jacobi; entry (r, c) = (H^0r H^0c + H^1r H^1c) + H^2r H^2c) is above 1e-8 times
 *   the largest (the guard of mm_resect_planar, squared).  Denormalise: A = H^ T with A_r0 = s H^_r0, A_r1 = s H^_r1,
 *   A_r2 = (H^_r2 - (s c_x) H^_r0) - (s c_y) H^_r1; H = T'^-1 A with H_0c = A_0c / s' + c'_x A_2c, H_1c = A_1c / s' + c'_y A_2c,
 *   H_2c = A_2c; then unit norm (the nine squares summed in order) and the sign rule.  A non-finite H is invalid.
 *   Refit.  refit_iters rounds (a fixed count) over the inliers of the current H -- fewer than 4: nothing changes any more --
 *   renormalised over them; a refit skips the collinearity test and replaces H only when it is valid and its cost over ALL
 *   matches is finite and strictly lower.
 *   Outputs.  pairs_out [n_pairs, cap, 2] (must not alias pairs) / m_out [n_pairs]: the inliers of the final H in input order,
 *   rows at or beyond m_out[p] untouched; a failed pair (any of the first three flags) has m_out = 0.  Hm [n_pairs, 9] and
 *   cost [n_pairs] f64, NaN without a model.  info [n_pairs, 6] i32 = (flags, n_inliers, best_h or -1, valid hypotheses,
 *   n_F or -1, 0).
 *   Flags.  MM_HOMOG_TOO_FEW m < max(min_matches, 8) | MM_HOMOG_NO_MODEL no hypothesis with a finite cost | MM_HOMOG_WEAK
 *   n_inliers < min_inliers | MM_HOMOG_MALFORMED | MM_HOMOG_DEGENERATE: verify_info [n_pairs, 4] (the info of
 *   mm_verify_matches on the same matches) is given, the pair has none of the first three flags, and either
 *   verify_info[p, 0] & 7 is non-zero (the fundamental matrix failed where the homography did not) or
 *   double(n_inliers) >= degenerate_frac * double(n_F) with n_F = verify_info[p, 1]: the homography explains nearly everything
 *   the fundamental matrix does, so the pair is planar or rotation-only and its F is one of a pencil.  With verify_info NULL
 *   the bit is never set, info[4] = -1 and every other output is the same.
 * Four launches (normalise, hypothesis, score, finish) with the shapes of mm_verify_matches; the guarantees are the same: a
 * call repeats bit for bit, a pair's row does not depend on its neighbours, rows [a, b) equal a call on that block with
 * pair_base + a, n_pairs = 0 returns MM_OK without a launch.  All pointers are DEVICE pointers except prm; kp_xy, pairs and
 * pairs_out 8-byte aligned; ws holds mm_homography_workspace_bytes(n_pairs, n_hyp) bytes (normalisations, every hypothesis' H
 * and cost).  Argument errors -- n_hyp outside 1 .. 4096, a negative or NaN threshold_px or collinear_tol, degenerate_frac
 * outside [0, 1], null pointers other than verify_info: MM_ERR_ARG; a workspace that is too small: MM_ERR_WORKSPACE -- are
 * returned before the device is touched. */
#define MM_HOMOG_TOO_FEW 1
#define MM_HOMOG_NO_MODEL 2
#define MM_HOMOG_WEAK 4
#define MM_HOMOG_MALFORMED 8
#define MM_HOMOG_DEGENERATE 16
typedef struct mm_homography_params {
    int32_t n_hyp, min_matches, min_inliers, refit_iters;      /* defaults 256, 8, 16, 2 */
    uint32_t seed, pair_base;
    double threshold_px, collinear_tol, degenerate_frac;       /* defaults 2, 1e-3, 0.8 */
} mm_homography_params;
size_t mm_homography_workspace_bytes(int n_pairs, int n_hyp);
int mm_verify_homography(mm_ctx *ctx, const float *kp_xy /*[n_pairs+1,cap,2]*/, const int32_t *pairs /*[n_pairs,cap,2]*/,
                         const int32_t *m /*[n_pairs]*/, int n_pairs, int cap, const mm_homography_params *prm,
                         const int32_t *verify_info /*[n_pairs,4] or NULL*/, int32_t *pairs_out /*[n_pairs,cap,2]*/,
                         int32_t *m_out /*[n_pairs]*/, double *Hm /*[n_pairs,9]*/, double *cost /*[n_pairs]*/,
                         int32_t *info /*[n_pairs,6]*/, void *ws, size_t ws_bytes);
/* The motion a homography implies.  K, kp_xy, pairs, m, the rays a = K^-1 (x, y, 1), b = K^-1 (x', y', 1), the convention
 * X2 = R X1 + t with |t| = 1 and the layouts of R, t, depth [n_pairs, cap, 2] and info [n_pairs, 8] = (flags, winner or -1,
 * votes[0 .. 3], m used, 0) are those of mm_recover_poses; pairs and m are what mm_verify_homography wrote to pairs_out /
 * m_out, Hm its homographies; normal_hint [n_pairs, 3] f64 or NULL.  The flag values 1, 2, 4, 8 mean what MM_POSE_* mean, so
 * mm_chain_poses reads the rows unchanged; MM_HPOSE_ROTATION is new.
 *   Setup.  G = K^-1 (H K), every entry summed left to right; M = G^T G; eigenpairs by the 3 x 3 Jacobi, ordered
 *   l1 >= l2 >= l3 by a stable exchange sort of the columns -- (0,1), (1,2), (0,1), each exchanged only when the right
 *   eigenvalue is strictly larger.  NO_MODEL when H or an eigenvalue is not finite or l3 <= 0.  sigma = (sqrt l1, sqrt l2,
 *   sqrt l3); G <- G / sqrt l2 (every entry divided); v1, v3 the eigenvectors of l1, l3 and v2 = v3 x v1.  G is negated when
 *   more of the pair's well-formed matches have b . (G a) < 0 than > 0.
 *   Rotation only: sqrt(l1 / l3) - 1 <= rotation_tol.  R = the polar factor of G (A (V diag(lambda^-1/2) V^T) from the Jacobi
 *   of A^T A, as in mm_resect_cameras; NO_MODEL when a lambda is not finite and positive or R is not finite), t = 0, normal
 *   and every depth row NaN, winner -1, no votes, flag MM_HPOSE_ROTATION.  mm_chain_poses composes the rotation, finds no
 *   common depths and carries the previous scale (FEW_COMMON on this pair and the next).
 *   Planar otherwise (Ma, Soatto, Kosecka, Sastry, An Invitation to 3-D Vision, section 5.3).  With n1 = l1 / l2 and
 *   n3 = l3 / l2: u+- = (sqrt(1 - n3) v1 +- sqrt(n1 - 1) v3) / sqrt(n1 - n3), each component one sum and one division;
 *   U = [v2, u, v2 x u] and W = [G v2, G u, (G v2) x (G u)] by columns; R = W U^T, n = v2 x u, t = (G - R) n.  Candidates
 *   c = 0: (R+, t+, n+), 1: (R+, -t+, -n+), 2: (R-, t-, n-), 3: (R-, -t-, -n-).  NO_MODEL when |t+| or |t-| is not finite and
 *   positive or an entry of R+ or R- is not finite.  n is a unit vector; with the plane n . X = d in camera 1, t comes out
 *   as t / d and the depths below in units of d.
 *   Depths and votes.  l1 = 1 / (n . a), l2 = l1 (R a)_z + t_z; a well-formed match votes for c when both are finite and > 0.
 *   After the vote t and the depths of the winner are divided by |t|.
 *   Winner.  The contenders are the candidates with double(votes) >= ambiguous_frac * double(largest count).  With a finite
 *   normal_hint[p] the winner is the contender with the largest n . hint, ties to the lowest c; without one the largest
 *   count, ties to the lowest c.  MM_POSE_AMBIGUOUS: votes[winner] < min_front_frac m, or several contenders and no hint (the
 *   twofold ambiguity of a plane seen by two cameras: both solutions put every point in front).
 *   Outputs.  R, t of the winner (NaN: no model); sigma [n_pairs, 3]; normal [n_pairs, 3] the winner's n (NaN without one);
 *   depth = (l1, l2) / |t| for the rows that voted for the winner, NaN elsewhere, rows at or beyond m[p] included; info.
 * One 256-thread workgroup per pair, integer counts; the depth pass repeats the vote pass's expression bit for bit.  The
 * guarantees and the argument checks of mm_recover_poses apply; a rotation_tol that is negative or NaN is MM_ERR_ARG. */
#define MM_HPOSE_ROTATION 16
typedef struct mm_hpose_params {
    int32_t min_matches, reserved;                              /* default 8 */
    double min_front_frac, ambiguous_frac, rotation_tol;        /* defaults 0.5, 0.9, 1e-2 */
} mm_hpose_params;
int mm_recover_poses_homography(mm_ctx *ctx, const double *K /*host [9]*/, const float *kp_xy /*[n_pairs+1,cap,2]*/,
                                const int32_t *pairs /*[n_pairs,cap,2]*/, const int32_t *m /*[n_pairs]*/,
                                const double *Hm /*[n_pairs,9]*/, const double *normal_hint /*[n_pairs,3] or NULL*/, int n_pairs,
                                int cap, const mm_hpose_params *prm, double *R /*[n_pairs,9]*/, double *t /*[n_pairs,3]*/,
                                double *sigma /*[n_pairs,3]*/, double *normal /*[n_pairs,3]*/, double *depth /*[n_pairs,cap,2]*/,
                                int32_t *info /*[n_pairs,8]*/);

/* ---- a-2d: guided matching -- matches recovered along each pair's epipolar geometry (no reference counterpart) -------------
 * mm_verify_matches and mm_verify_homography only remove matches.  The Lowe ratio test of the match stage is global: a key point
 * with a look-alike anywhere in the next image fails it.  Once a pair has a model the look-alike is almost never near the
 * epipolar line (or the transferred point): mm_guided_match searches the key points no match uses again, among the
 * candidates the model admits only.
 *   Inputs, all DEVICE pointers except prm.  Pair p joins frame p (query) and frame p + 1 (train) of a block of n_pairs + 1
 *   frames: kp_xy [n_pairs+1, cap, 2] f32, desc [n_pairs+1, cap, 32] u8 (256-bit binary descriptors), n [n_pairs+1] i32 key points
 *   per frame (clamped to 0 .. cap): n_q = n[p], n_t = n[p+1].  pairs [n_pairs, cap, 2] i32 = (queryIdx, trainIdx) and m
 *   [n_pairs] i32 (clamped to 0 .. cap): the seed matches, as mm_verify_matches / mm_verify_homography write them.  model
 *   [n_pairs, 9] f64 row-major, kind [n_pairs] i32 or NULL (all 0).  kind 0: model is F with x'^T F x = 0; kind 1: model is H
 *   with x' ~ H x; anything else: the pair has no model.
 *   Gate.  g(i, j) holds when d^2(x_i, x'_j) is finite and <= tau^2, tau = threshold_px, x_i = kp_xy[p, i], x'_j =
 *   kp_xy[p+1, j] widened to f64.  kind 0: the Sampson distance of mm_verify_matches, evaluated as written here:
 *   fx_r = F_r0 x + F_r1 y + F_r2 (r = 0, 1, 2), ft0 = F_00 x' + F_10 y' + F_20, ft1 = F_01 x' + F_11 y' + F_21,
 *   e = x' fx0 + y' fx1 + fx2, d^2 = e e / (fx0 fx0 + fx1 fx1 + ft0 ft0 + ft1 ft1), every sum left to right, no fused
 *   multiply-add.  kind 1: the symmetric transfer distance of mm_verify_homography as written there, the adjugate computed once
 *   per pair.  These are the inlier rules of the two verify stages, so a guided match is an inlier of the model it came from.
 *   Both distances are symmetric in the two images: the gate is the same set in either search direction.
 *   Seeds.  The input rows j < m must be in strictly increasing query order, q_j < q_(j+1) on the raw values (what the ratio
 *   filter and the compactions of the verify stages emit); otherwise the pair is MM_GUIDED_UNORDERED and passes through.  A row
 *   with an index outside [0, cap) is MALFORMED: it is dropped, nothing is read through it, the flag is set.  Every other input
 *   row is kept as it is and marks its query and its train as used.
 *   Search.  For every unused query i < n_q: C_i = { j < n_t : train j unused, g(i, j) }; j0 and j1 the nearest and the second
 *   nearest of C_i by the Hamming distance of the descriptors, ties to the lower j, d0 and d1 their distances.  (i, j0) is
 *   PROPOSED when d0 <= max_dist and either C_i has a single member or (double)d0 < ratio * (double)d1 (the comparison of
 *   mm_ratio_filter_batched).
 *   One-to-one.  cross_check = 1: the proposal is kept iff i is the nearest of { i' < n_q unused : g(i', j0) } to train j0, ties
 *   to the lower i' (the search in the reverse direction over the same gate).  cross_check = 0: among the proposals with the
 *   same train the lowest (d0, i) is kept.  Either way no train gains two new matches.
 *   Outputs.  pairs_out [n_pairs, cap, 2] (must not alias pairs): the kept input rows and the new rows merged in query order,
 *   -1 from row m_out[p] on -- every element is written; m_out [n_pairs]; is_new [n_pairs, cap] u8 parallel to pairs_out (1: a
 *   new row; 0 elsewhere, the tail included); info [n_pairs, 4] i32 = (flags, input rows kept, rows added, proposals before the
 *   one-to-one step).  A pair that passes through (SKIPPED, UNORDERED) has its m input rows copied as they are -- malformed
 *   ones included, the flag says so -- and info = (flags, m, 0, 0).
 *   Flags.  MM_GUIDED_SKIPPED: kind names no model, or model has a non-finite entry | MM_GUIDED_UNORDERED |
 *   MM_GUIDED_MALFORMED.
 * Three launches: prepare (one workgroup per pair: the order test, the used marks, the unused queries and trains listed in
 * ascending order), search (workgroup = pair x 256 unused queries, lane = query; a train passes a cheap necessary test on
 * terms prepared once before the distance itself is evaluated; best and second on a packed (distance, index) key; the reverse
 * direction is an integer atomicMin of (distance, query) per train in the same pass, whose result does not depend on order)
 * and finish (one workgroup per pair: the proposal rule, one-to-one, the merge by ballot / popcount prefix).  Nothing else
 * depends on order and nothing is sampled: a call repeats bit for bit, a pair's row does not depend on which other pairs share
 * the call, rows [a, b) of a call equal a call on that sub-block.  n_pairs = 0 returns MM_OK without a launch.  kp_xy, pairs
 * and pairs_out 8-byte aligned, desc and ws 16-byte aligned; ws holds mm_guided_workspace_bytes(n_pairs, cap) bytes.  Argument
 * errors -- null pointers other than kind, cap < 1 or above 2^22, a negative or NaN threshold_px (+inf admits every finite
 * distance), a negative or NaN ratio, max_dist outside 0 .. 256, cross_check outside {0, 1}, pairs_out == pairs: MM_ERR_ARG; a
 * workspace that is too small: MM_ERR_WORKSPACE -- are returned before the device is touched. */
#define MM_GUIDED_SKIPPED 1
#define MM_GUIDED_UNORDERED 2
#define MM_GUIDED_MALFORMED 8
typedef struct mm_guided_params {
    double threshold_px, ratio;          /* defaults 2, 0.8 */
    int32_t max_dist, cross_check;       /* defaults 64, 1 */
} mm_guided_params;
size_t mm_guided_workspace_bytes(int n_pairs, int cap);
int mm_guided_match(mm_ctx *ctx, const float *kp_xy /*[n_pairs+1,cap,2]*/, const uint8_t *desc /*[n_pairs+1,cap,32]*/,
                    const int32_t *n /*[n_pairs+1]*/, const int32_t *pairs /*[n_pairs,cap,2]*/, const int32_t *m /*[n_pairs]*/,
                    const double *model /*[n_pairs,9]*/, const int32_t *kind /*[n_pairs] or NULL*/, int n_pairs, int cap,
                    const mm_guided_params *prm, int32_t *pairs_out /*[n_pairs,cap,2]*/, int32_t *m_out /*[n_pairs]*/,
                    uint8_t *is_new /*[n_pairs,cap]*/, int32_t *info /*[n_pairs,4]*/, void *ws, size_t ws_bytes);

/* ---- a-2h: similarity registration, a robust 7-DoF alignment to known geometry ---------------------------------------------------
 * No reference counterpart: the reference is metric through its chessboard.  A chain recovered by mm_chain_poses, a triangulated
 * cloud or an adjusted result lives in a frame nobody chose (first camera at the origin, first baseline the unit of length); this
 * call estimates, for each of n_prob independent problems, the similarity (s, R, d) with dst_j ~ s R src_j + d from correspondences
 * that may hold gross outliers.
 *   Inputs.  src, dst [N, 3] f64.  ptr [n_prob+1] i64 HOST (the grids are sized without a device read): problem q owns rows
 *   ptr[q] .. ptr[q+1] - 1, n = ptr[q+1] - ptr[q] of them (at most 2^31 - 1).
 *   Fit -- one routine for the three-point hypothesis and the refit over n rows.  Centroids cs, cd: each coordinate sum / n.
 *   a = src - cs, b = dst - cd; M = sum b a^T (nine sums, M_rc += b_r a_c) and var = sum ((a0 a0 + a1 a1) + a2 a2), rows ascending
 *   for a hypothesis, in the chunked order below for a refit.  G = M^T M, G_rc = (M_0r M_0c + M_1r M_1c) + M_2r M_2c; 3 x 3 cyclic
 *   Jacobi (the one of mm_resect_cameras) gives lambda and V.  v1 = the column of the largest lambda (lambda1), v2 = the column of
 *   the larger of the other two (lambda2), ties to the lowest column both times; v3 = v1 x v2.  Invalid: lambda1 not finite and
 *   positive, lambda2 not finite or <= collinear_tol^2 lambda1 (points collinear on either side: a three-point M has rank 2 at
 *   best, which is why the polar factor of mm_resect_cameras cannot serve here), var not finite and positive, or a non-finite
 *   entry of the result.  u1 = M v1 / |M v1|; w2 = M v2 - (u1 . M v2) u1, u2 = w2 / |w2|; u3 = u1 x u2 (norms as
 *   sqrt((x x + y y) + z z), products M v as (M_r0 v_0 + M_r1 v_1) + M_r2 v_2).  R_rc = (u1_r v1_c + u2_r v2_c) + u3_r v3_c:
 *   det R = +1 by construction, the Kabsch / Umeyama solution with its reflection case.  s = (sum_k R_k M_k, k = 0 .. 8 row-major,
 *   left to right) / var, or 1 when with_scale = 0.  d_r = cd_r - s ((R_r0 cs_0 + R_r1 cs_1) + R_r2 cs_2).
 *   Sampling, the integer scheme of mm_verify_matches with three picks: base = pcg(pcg(seed + pcg(prob_base + q)) + h); pick
 *   k = 0 .. 2 tries t = 0 .. 7: i = (uint64(pcg(base + 8 k + t)) * n) >> 32, the first i that is not an earlier pick; eight
 *   collisions, or a picked row with a non-finite coordinate, make the hypothesis invalid.  The three rows enter the fit in
 *   ascending row order: two hypotheses over the same rows are the same bits and tie exactly (with few rows that happens, and
 *   the tie then goes to the lowest h on any machine).  prob_base is the global index of problem 0 of the call.
 *   Score.  With A = s R (nine products) e_r = dst_r - (((A_r0 x + A_r1 y) + A_r2 z) + d_r), e^2 = (e0 e0 + e1 e1) + e2 e2.  A row
 *   is an inlier iff e^2 is finite and <= tau^2.  MSAC: cost = sum of (inlier ? e^2 : tau^2); an invalid hypothesis costs +inf.
 *   Order of every sum over rows.  Rows go in chunks of MM_ALIGN_CHUNK = 4096 rows of the problem, a constant of this definition;
 *   across chunks the partial sums are added chunk index ascending, starting from 0.  Inside a chunk the ranking cost of a
 *   hypothesis is taken rows ascending; every other sum (a model's cost and inlier count, the refit's moments) is the workgroup's
 *   fixed order of mm_resect_cameras (256 threads striding the chunk's rows, xor butterfly, waves in order).  The bits depend on
 *   the problem alone, not on the grid.
 *   Winner.  The lowest finite ranking cost, ties to the lowest h.  Its cost and inliers are then taken in the workgroup order,
 *   like every cost from here on.
 *   Refit.  refit_iters rounds (a fixed count) over the inliers of the current model, two passes: the sums of src and dst and the
 *   count give the centroids, then M and var about them.  Fewer than 3 inliers: the round changes nothing.  The candidate is
 *   accepted only when it is valid and its cost over ALL rows is finite and strictly lower.
 *   Outputs.  sim [n_prob, 13] f64 = (s, R row-major, d), NaN without a model; cost [n_prob] f64 (NaN without a model); inlier
 *   [N] u8, every row of every problem written (0 without a model); info [n_prob, 4] i32 = (flags, n_inliers, best_h or -1, valid
 *   hypotheses).
 *   Flags.  MM_ALIGN_TOO_FEW n < max(min_points, 3): no RANSAC is run | MM_ALIGN_NO_MODEL no finite-cost hypothesis (collinear
 *   data, a straight dolly, ends here) | MM_ALIGN_WEAK n_inliers < min_inliers | MM_ALIGN_NONFINITE some row of the problem has a
 *   non-finite coordinate (such a row is never an inlier and costs tau^2).
 * No float atomics: a call repeats bit for bit, a problem's row does not depend on which other problems share the call, and
 * rows [a, b) of a call equal a call on that block with prob_base + a.  n_prob = 0 returns MM_OK without a launch.  src, dst and
 * the outputs are DEVICE pointers, ptr and prm host; ws holds mm_align_workspace_bytes(n_prob, n_hyp, N) bytes, N = ptr[n_prob],
 * 8-byte aligned.  Argument errors -- n_hyp outside 1 .. 4096, tau not finite and positive, a collinear_tol that is negative or not
 * finite, refit_iters outside 0 .. 1000, a negative min_inliers, with_scale outside {0, 1}, a negative or decreasing ptr, null
 * pointers: MM_ERR_ARG; a workspace that is too small: MM_ERR_WORKSPACE -- are returned before the device is touched. */
#define MM_ALIGN_TOO_FEW 1
#define MM_ALIGN_NO_MODEL 2
#define MM_ALIGN_WEAK 4
#define MM_ALIGN_NONFINITE 8
#define MM_ALIGN_CHUNK 4096
typedef struct mm_align_params {
    int32_t n_hyp, min_points, min_inliers, refit_iters, with_scale, reserved;      /* defaults 256, 3, 3, 2, 1 */
    uint32_t seed, prob_base;
    double tau;                                                                     /* in dst units; required, > 0 */
    double collinear_tol;                                                           /* default 1e-6 */
} mm_align_params;
size_t mm_align_workspace_bytes(int n_prob, int n_hyp, int64_t N);
int mm_align_similarity(mm_ctx *ctx, const double *src /*[N,3]*/, const double *dst /*[N,3]*/, const int64_t *ptr /*host [n_prob+1]*/,
                        int n_prob, const mm_align_params *prm, double *sim /*[n_prob,13]*/, double *cost /*[n_prob]*/,
                        uint8_t *inlier /*[N]*/, int32_t *info /*[n_prob,4]*/, void *ws, size_t ws_bytes);

/* A similarity applied to a reconstruction, in place; sim [13] f64 = (s, R, d) as mm_align_similarity writes it (DEVICE).
 *   Points pts [P, 3] or NULL: X' = s R X + d, evaluated as the score above evaluates it (A = s R first).
 *   Extrinsics ext [F, 3, 4] or NULL: Rc' = Rc R^T, Rc'_ij = (Rc_i0 R_j0 + Rc_i1 R_j1) + Rc_i2 R_j2, and
 *   tc'_i = s tc_i - ((Rc'_i0 d_0 + Rc'_i1 d_1) + Rc'_i2 d_2): the camera frame is scaled by s, Rc' X' + tc' = s (Rc X + tc), so
 *   every projection is unchanged.
 * A sim with a non-finite entry leaves both untouched and returns MM_OK.  One thread per point / camera, plain stores. */
int mm_apply_similarity(mm_ctx *ctx, const double *sim /*dev [13]*/, double *pts /*[P,3] in/out or NULL*/, int64_t P,
                        double *ext /*[F,3,4] in/out or NULL*/, int64_t F);
/* Camera centres C [F, 3] of ext [F, 3, 4]: C_j = -((Rc_0j tc_0 + Rc_1j tc_1) + Rc_2j tc_2). */
int mm_camera_centres(mm_ctx *ctx, const double *ext /*[F,3,4]*/, int64_t F, double *C /*[F,3]*/);

/* ---- a-4: two-view DLT triangulation ------------------------------------------------------------
 * Replaces the per-track cv2.triangulatePoints + dehomogenise loop, processor.py:254-261.
 * proj [F,3,4] f64; track i uses views f0[i], f1[i] with pixels x0[i], x1[i]; X [n,3]. */
int mm_triangulate_dlt(mm_ctx *ctx, const double *proj /*dev*/, const int32_t *f0 /*dev*/, const int32_t *f1 /*dev*/,
                       const double *x0 /*dev [n,2]*/, const double *x1 /*dev [n,2]*/, int64_t n,
                       double *X /*dev [n,3]*/);
/* Multi-view triangulation of whole tracks, with a per-track verdict.  The tracks are a CSR over observations
 * (mm_link_tracks_device): track t owns observations track_ptr[t] .. track_ptr[t+1] - 1 (m of them), observation o was made
 * in frame obs_frame[o] (0 <= obs_frame[o] < F: the caller checks) at pixel obs_xy[o] -- what mm_flatten_tracks over all
 * tracks produces.  All pointers are DEVICE pointers; ws holds mm_triangulate_tracks_workspace_bytes(F) bytes (camera
 * centres C_f = -P[:, :3]^-1 P[:, 3] and |P[2, :3]| of every frame, written by a small pre-kernel).
 *   Linear stage: every observation contributes the rows x P[2] - P[0] and y P[2] - P[1] (unnormalised, the rows OpenCV
 *   builds); X is the de-homogenised eigenvector of the smallest eigenvalue of A^T A (cyclic Jacobi).  For m = 2 that is the
 *   vector mm_triangulate_dlt finds.
 *   Refinement: refine_iters Levenberg-Marquardt TRIAL steps on sum |pi(P X) - x|^2 with H = sum J^T J, g = sum J^T r,
 *   J = (P[:2, :3] - u P[2, :3]) / w, (H + lambda diag H) delta = -g by Cholesky, lambda = 1e-3 at the start; a trial whose
 *   cost is finite and strictly lower is accepted (lambda <- max(lambda / 10, 1e-12)), anything else -- a failed pivot, a
 *   non-finite cost -- is rejected (lambda <- 10 lambda).  The cost never rises; refine_iters = 0 returns the linear X.
 *   quality [T,4] at the returned X = (rms_px = sqrt(sum |r|^2 / m), max_px = max |r|, min_depth = min_i P_i[2].(X,1) /
 *   |P_i[2, :3]|, cos_parallax = min over i != first of cos angle(C_first - X, C_i - X)).  Every pairwise angle is at most
 *   the sum of two angles to the first ray, so acos(cos_parallax) is within a factor of two of the largest pairwise angle
 *   of the track, at O(m) instead of O(m^2) cost.
 *   A residual, depth or cosine that is not a number (w = 0 at X; X on the first camera's centre) makes its column NaN, as
 *   NumPy's max / min would; a comparison with NaN is false, so that test does not flag the track: a caller that culls on
 *   flags == 0 and can meet such input also asks for finite quality.
 *   flags [T]: MM_TRI_BEHIND min_depth <= prm.min_depth | MM_TRI_REPROJ max_px > prm.max_reproj_px | MM_TRI_PARALLAX
 *   cos_parallax > prm.max_cos_parallax (thresholds -inf, +inf, 2.0 switch a test off) | MM_TRI_DEGENERATE m < 2 or a
 *   non-finite component of X: such a track is not refined and its quality is NaN.
 * Four lanes per track, sums in a fixed order that depends on the track alone, no atomics: a call repeats bit for bit and a
 * track's result does not depend on which other tracks share the call.  T = 0 returns MM_OK without a launch. */
#define MM_TRI_BEHIND 1
#define MM_TRI_REPROJ 2
#define MM_TRI_PARALLAX 4
#define MM_TRI_DEGENERATE 8
typedef struct mm_tri_params {
    int32_t refine_iters, reserved;
    double max_reproj_px, max_cos_parallax, min_depth;
} mm_tri_params;
size_t mm_triangulate_tracks_workspace_bytes(int F);
int mm_triangulate_tracks(mm_ctx *ctx, const double *proj /*[F,3,4]*/, int F, const int32_t *track_ptr /*[T+1]*/, int64_t T,
                          const int32_t *obs_frame /*[O]*/, const double *obs_xy /*[O,2]*/, const mm_tri_params *prm,
                          double *X /*[T,3]*/, double *quality /*[T,4]*/, int32_t *flags /*[T]*/, void *ws, size_t ws_bytes);

/* ---- a-9b: observation filter at the adjusted solution ---------------------------------------------------------------------------
 * No reference counterpart: the reference adjusts whatever its matcher linked.  Every test in front of the solver judges a track
 * at its initial triangulation under the initial poses; this call judges every observation, and every point by what it has left,
 * at the cameras and points an adjustment returned, and compacts the problem for the next solve.
 *   Inputs, what the adjustment takes and returns.  cams [F, 6] f64 (Rodrigues vector, then t), one row for every value fi takes
 *   (a caller with fixed cameras concatenates them); pts [P, 3] f64; fi, pi [O] i32 and obs [O, 2] f64 point-major, as
 *   mm_flatten_tracks emits them; pt_ptr [P+1] i32: point p owns observations pt_ptr[p] .. pt_ptr[p+1] - 1 (what
 *   mm_ba_index_build writes).  The caller checks 0 <= fi < F, 0 <= pi < P and that pt_ptr is that CSR.  These and the outputs
 *   are DEVICE pointers; K [9] row-major and prm are HOST (K is judged before the device is touched and travels by value).
 *   Camera table, a small pre-kernel, 15 doubles per camera.  th2 = (rx rx + ry ry) + rz rz.  th2 < 1e-4 (the series of the
 *   adjustment's own sweeps): c = cos(sqrt(th2)), a = 1 + th2 (-1/6 + th2 (1/120 - th2 / 5040)), b = 1/2 + th2 (-1/24 + th2
 *   (1/720 - th2 / 40320)); otherwise th = sqrt(th2), c = cos th, a = sin th / th, b = (2 sin^2(th / 2)) / th2.
 *   R = c I + a [r]x + b r r^T, every entry as written here, products left to right: R00 = c + b rx rx, R01 = -a rz + b rx ry,
 *   R02 = a ry + b rx rz, R10 = a rz + b ry rx, R11 = c + b ry ry, R12 = -a rx + b ry rz, R20 = -a ry + b rz rx,
 *   R21 = a rx + b rz ry, R22 = c + b rz rz.  Centre C_j = -((R_0j t_0 + R_1j t_1) + R_2j t_2).
 *   Step 1, per observation o (camera f, point p).  Y_i = ((R_i0 X_0 + R_i1 X_1) + R_i2 X_2) + t_i; depth = Y_2;
 *   u_i = (K_i0 Y_0 + K_i1 Y_1) + K_i2 Y_2; dx = u_0 / u_2 - obs_x, dy = u_1 / u_2 - obs_y; e = sqrt(dx dx + dy dy).
 *   obs_flags[o] = MM_OBS_NONFINITE e or depth is not finite | MM_OBS_BEHIND depth <= min_depth | MM_OBS_REPROJ
 *   e > max_reproj_px.  A comparison with NaN is false, as in mm_triangulate_tracks; thresholds +inf, -inf and 2.0 switch a test
 *   off, as in mm_tri_params.  err [O] = e and depth [O] are outputs.
 *   Step 2, per point p, over its observations with obs_flags == 0 (the survivors), in order.  n_ok = their count.  With
 *   a = C_first - X of the first survivor and b = C_i - X of each later one, dots as (x x + y y) + z z,
 *   cos_parallax[p] = min over them of (a . b) / sqrt((a . a) (b . b)) -- a NaN stays, as NumPy's min keeps it -- and NaN when
 *   n_ok < 2: the cosine of mm_triangulate_tracks restricted to survivors.  pt_flags[p] = MM_PT_NONFINITE a component of X is
 *   not finite | MM_PT_SHORT n_ok < min_views | MM_PT_PARALLAX cos_parallax > max_cos_parallax.
 *   Step 3.  An observation is kept iff its flags are 0 and its point's flags are 0; an unflagged observation of a flagged point
 *   gains MM_OBS_ORPHAN.
 *   Step 4, compaction, order preserved.  Kept observations stay in input order and kept points are renumbered in input order, so
 *   the output is point-major again: fi_out, pi_out (renumbered), obs_out (the input's bits), obs_map [O'] (input row of each
 *   kept observation), point_map [P'] (input index of each kept point), each sized by the caller for O and P rows; counts [4]
 *   i64 = (O', P', observations flagged by a test of their own, points flagged).  The positions are two exclusive scans of 0 / 1
 *   flags in chunks of MM_FILTER_CHUNK = 1024 rows, a constant of this definition: sums per chunk, one scan of the sums, then
 *   each chunk places its rows -- separate launches, no workgroup waits for another.
 * Every number is computed by one thread from its own inputs, the counts are integers and there are no atomics: a call repeats
 * bit for bit and a point's verdict does not depend on which other points share the call.  O = 0 or P = 0 returns MM_OK with
 * counts = 0 and writes nothing else.  ws holds mm_filter_workspace_bytes(F, P, O) bytes, 8-byte aligned; obs and obs_out
 * 16-byte aligned.  Argument errors -- min_views < 2, a NaN threshold, a K that mm_resect_cameras would refuse, null pointers,
 * negative sizes, O or P beyond 2^31 - 1: MM_ERR_ARG; a workspace that is too small: MM_ERR_WORKSPACE -- are returned before the
 * device is touched. */
#define MM_OBS_REPROJ 1
#define MM_OBS_BEHIND 2
#define MM_OBS_NONFINITE 4
#define MM_OBS_ORPHAN 8
#define MM_PT_SHORT 1
#define MM_PT_PARALLAX 2
#define MM_PT_NONFINITE 4
#define MM_FILTER_CHUNK 1024
typedef struct mm_filter_params {
    int32_t min_views, reserved;
    double max_reproj_px, min_depth, max_cos_parallax;
} mm_filter_params;
size_t mm_filter_workspace_bytes(int F, int64_t P, int64_t O);
int mm_filter_observations(mm_ctx *ctx, const double *cams /*[F,6]*/, int F, const double *pts /*[P,3]*/, int64_t P,
                           const double *K /*host [9]*/, const int32_t *fi /*[O]*/, const int32_t *pi /*[O]*/,
                           const double *obs /*[O,2]*/, int64_t O, const int32_t *pt_ptr /*[P+1]*/, const mm_filter_params *prm,
                           int32_t *obs_flags /*[O]*/, double *err /*[O]*/, double *depth /*[O]*/, int32_t *pt_flags /*[P]*/,
                           double *cos_parallax /*[P]*/, int32_t *fi_out /*[O]*/, int32_t *pi_out /*[O]*/, double *obs_out /*[O,2]*/,
                           int32_t *obs_map /*[O]*/, int32_t *point_map /*[P]*/, int64_t *counts /*[4]*/, void *ws, size_t ws_bytes);

/* ---- a-9c: dense depth: a plane-sweep depth map per view, the maps fused into a cloud ---------------------------------------------
 * No reference counterpart: the reference ends with the adjusted corner points.  Every reference view gets a depth map by
 * sweeping D fronto-parallel planes through its depth range and scoring each against up to S source frames by zero-mean
 * normalised cross-correlation over a (2r+1)^2 window (mm_depth_sweep); the maps are then checked against each other and the
 * pixels enough other views agree with become a point cloud (mm_depth_fuse).  Only + - * / sqrt floor rint and conversions
 * occur, each correctly rounded and none contracted, so a restatement that follows this text gives the same bits.
 *
 * mm_depth_sweep.  img [F, H, W] u8; ref [V] i32, the frame of each view; src [V, S] i32, its source frames, -1: none (the
 * caller checks 0 <= ref < F and -1 <= src < F); AB [V, S, 12] f64, w0, dw [V] f64 -- DEVICE pointers, as are the outputs; K [9]
 * row-major and prm are HOST.
 *   Host tables (the caller's: ops.sweep_tables writes every product out).  With [R_r | t_r] the reference and [R_s | t_s] the
 *   source extrinsic: R = R_s R_r^T, R_ij = (Rs_i0 Rr_j0 + Rs_i1 Rr_j1) + Rs_i2 Rr_j2; t_i = ts_i - ((R_i0 tr_0 + R_i1 tr_1) +
 *   R_i2 tr_2); M = K R, M_ij = (K_i0 R_0j + K_i1 R_1j) + K_i2 R_2j; with K = (fx s cx; 0 fy cy; 0 0 1), A = M K^-1:
 *   A_i0 = M_i0 / fx, A_i1 = (M_i1 - s A_i0) / fy, A_i2 = (M_i2 - cx A_i0) - cy A_i1; b_i = (K_i0 t_0 + K_i1 t_1) + K_i2 t_2.
 *   AB = (A row-major, b).  The view's planes have inverse depths w_k = w0 + k dw, k = 0 .. D-1, with w0 = 1 / dmin and
 *   dw = (1 / dmax - 1 / dmin) / (D - 1) (0 for D = 1).  K^-1 has the last row (0, 0, 1), so the homography of plane k is A with
 *   w_k b added to its third column -- the premise K is judged for (the check of mm_resect_cameras); the kernels read AB alone.
 *   Warp, f64, per reference pixel (u, v), plane k, source s: c_i = A_i2 + w_k b_i; p_i = (A_i0 u + A_i1 v) + c_i; xs = p_0 /
 *   p_2, ys = p_1 / p_2.  Valid iff p_2 > 0, 0 <= xs <= W-1 and 0 <= ys <= H-1 (a comparison with NaN is false).
 *   x0 = min(floor(xs), W-2), fx = (float)(xs - x0); y0, fy likewise.
 *   Sample, f32, with s00 = img[src, y0, x0], s01 at x0+1, s10 at y0+1, s11 at both: top = s00 + fx (s01 - s00), bot = s10 +
 *   fx (s11 - s10), val = top + fy (bot - top).  The reference's value at a pixel is its u8 as f32.
 *   Cost, f32.  A pixel with r <= u < W-r and r <= v < H-r has a window, n = (2r+1)^2 pixels, walked row-major (dv outer, du
 *   inner); every sum below starts at 0 and adds its terms one by one in that order.  mean_a = (sum of the reference values) /
 *   (float)n, ca = value - mean_a, saa = sum ca ca.  For a source all of whose n window pixels warp validly: mean_b, cb and
 *   sbb = sum cb cb likewise from the samples, sab = sum ca cb.  The source counts iff those n are valid, saa > thr and sbb > thr,
 *   thr = (float)var_min (float)n; then cost_s = 1 - sab / sqrt(saa sbb).  Over the sources that count, in list order: acc +=
 *   cost_s, cnt += 1; cost_k = acc / (float)cnt, valid iff cnt >= min_sources.
 *   Winner: the lowest valid cost_k, the lowest k among equals.  Sub-plane step, f64 from the f32 costs: if 0 < k < D-1, both
 *   neighbouring planes are valid and den = (c- - 2 c0) + c+ > 0, delta = (c- - c+) / (2 den) clamped to [-1/2, 1/2]; otherwise 0.
 *   depth = (float)(1 / (w0 + (k + delta) dw)).
 *   depth, cost [V, H, W] f32 and plane [V, H, W] i32: NaN, NaN and -1 where a pixel has no window or no valid plane.
 * A view's map depends on that view's rows alone, one thread computes each number from its own inputs, and a call repeats bit
 * for bit.  ws holds mm_depth_sweep_workspace_bytes(V, S, D) bytes, 8-byte aligned (c_i per view, source and plane).
 * planes outside 1 .. MM_SWEEP_MAX_PLANES, radius outside 1 .. MM_SWEEP_MAX_RADIUS, S outside 1 .. MM_SWEEP_MAX_SOURCES,
 * min_sources outside 1 .. S, a var_min that is negative or not finite, a K that mm_resect_cameras would refuse, null pointers,
 * non-positive F, H, W, more than 2^31 - 1 pixels: MM_ERR_ARG; a workspace that is too small: MM_ERR_WORKSPACE -- returned before
 * the device is touched.  V = 0 returns MM_OK and writes nothing.  MM_SWEEP_TILE is the side of the tile of pixels a workgroup
 * owns (tiles start at (r, r)); no result depends on it.
 *
 * mm_depth_fuse.  depth, cost [V, H, W] f32 as the sweep wrote them; ext [V, 3, 4] f64, the views' [R | t]; nbr [V, Q] i32,
 * per view the other views of this call it is checked against, -1: none (the caller checks -1 <= nbr < V); grey [V, H, W] u8, the
 * views' images -- DEVICE pointers, as are the outputs; K [9] and prm are HOST.  f64 throughout, sums left to right.
 *   Candidate: pixel (u, v) of view i with d = (double)depth finite and (double)cost <= max_cost.
 *   Lift(e, u, v, d): yn = (v - cy) / fy, xn = ((u - cx) - s yn) / fx, a = (d xn - t_0, d yn - t_1, d - t_2),
 *   X_j = (R_0j a_0 + R_1j a_1) + R_2j a_2.  Project(e, X): Y_i = ((R_i0 X_0 + R_i1 X_1) + R_i2 X_2) + t_i,
 *   px = ((fx Y_0 + s Y_1) + cx Y_2) / Y_2, py = (fy Y_1 + cy Y_2) / Y_2.
 *   X_w = Lift(i, u, v, d).  View q of nbr[i] agrees iff: (Y, px, py) = Project(q, X_w) has Y_2 > 0; xi = rint(px), yi =
 *   rint(py) lie in 0 .. W-1, 0 .. H-1; pixel (xi, yi) of q is a candidate, with depth dq; |dq - Y_2| <= eps_depth Y_2;
 *   (Z, bx, by) = Project(i, Lift(q, xi, yi, dq)) has Z_2 > 0 and sqrt((bx - u)^2 + (by - v)^2) <= tau_px.
 *   The pixel is kept iff at least min_consistent views agree.
 *   Kept pixels are compacted in (view, row, column) order: points [cap, 3] f64 = X_w, grey_out [cap] u8, origin [cap, 2] i32 =
 *   (view, v W + u), n_consistent [cap] i32 = the views that agreed; keep [V, H, W] u8; counts [2] i64 = (kept, candidates).
 *   Rows beyond cap are not written; counts[0] still counts them.  The positions are an exclusive scan in chunks of
 *   MM_FILTER_CHUNK pixels -- sums per chunk, one scan of the sums, then each chunk places its rows: separate launches.
 *   A surface point seen by several views appears once per view that keeps it: duplicates are NOT merged.
 * No atomics, no float sum across threads: a call repeats bit for bit.  ws holds mm_depth_fuse_workspace_bytes(V, H, W) bytes,
 * 8-byte aligned.  A NaN max_cost, a negative or NaN eps_depth or tau_px, min_consistent < 0, Q outside 0 ..
 * MM_FUSE_MAX_NEIGHBOURS, cap < 0, a K as above, null pointers (nbr may be null with Q = 0, the four row outputs with cap = 0),
 * more than 2^31 - 1 pixels: MM_ERR_ARG; a workspace that is too small: MM_ERR_WORKSPACE -- before the device is touched.
 * V = 0 returns MM_OK with counts = 0. */
#define MM_SWEEP_TILE 16
#define MM_SWEEP_MAX_RADIUS 4
#define MM_SWEEP_MAX_PLANES 4096
#define MM_SWEEP_MAX_SOURCES 16
#define MM_FUSE_MAX_NEIGHBOURS 64
typedef struct mm_sweep_params {
    int32_t planes, radius, min_sources, reserved;
    double var_min;
} mm_sweep_params;
typedef struct mm_fuse_params {
    int32_t min_consistent, reserved;
    double max_cost, eps_depth, tau_px;
} mm_fuse_params;
size_t mm_depth_sweep_workspace_bytes(int V, int S, int D);
int mm_depth_sweep(mm_ctx *ctx, const uint8_t *img /*[F,H,W]*/, int F, int H, int W, const double *K /*host [9]*/,
                   const int32_t *ref /*[V]*/, const int32_t *src /*[V,S]*/, const double *AB /*[V,S,12]*/, const double *w0 /*[V]*/,
                   const double *dw /*[V]*/, int V, int S, const mm_sweep_params *prm, float *depth /*[V,H,W]*/,
                   float *cost /*[V,H,W]*/, int32_t *plane /*[V,H,W]*/, void *ws, size_t ws_bytes);
size_t mm_depth_fuse_workspace_bytes(int V, int H, int W);
int mm_depth_fuse(mm_ctx *ctx, const float *depth /*[V,H,W]*/, const float *cost /*[V,H,W]*/, int V, int H, int W,
                  const double *ext /*[V,3,4]*/, const double *K /*host [9]*/, const int32_t *nbr /*[V,Q]*/, int Q,
                  const uint8_t *grey /*[V,H,W]*/, const mm_fuse_params *prm, int64_t cap, double *points /*[cap,3]*/,
                  uint8_t *grey_out /*[cap]*/, int32_t *origin /*[cap,2]*/, int32_t *n_consistent /*[cap]*/, uint8_t *keep /*[V,H,W]*/,
                  int64_t *counts /*[2]*/, void *ws, size_t ws_bytes);

/* ---- a-7..a-9: bundle adjustment sweeps -----------------------------------------------------------
 * Cost model of bundleAdjuster.py:7-52,81-102 (Rodrigues rotate, translate, full 3x3 K, divide, minus obs),
 * f64 throughout.  The LM/trust-region driver (the reference's scipy least_squares TRF loop,
 * bundleAdjuster.py:180-192) lives in meatmodeler_amd/bundleAdjuster.py and calls these sweeps. */
typedef struct mm_ba_problem {
    int32_t F, P;
    int64_t O;
    const double *K;         /* dev [9] row-major 3x3 */
    const int32_t *fi, *pi;  /* dev [O] camera / point index of each observation */
    const double *obs;       /* dev [O,2] */
    const int32_t *pt_ptr, *pt_obs;   /* dev CSR by point  (mm_ba_build_index) */
    const int32_t *cam_ptr, *cam_obs; /* dev CSR by camera */
    /* optional co-observation pair list (mm_ba_build_pairs) for the banded, bitwise reproducible Schur kernel;
     * n_seg == 0 / NULL pointers select the general kernel.  Segments are cut into chunks of at most 256 pairs: one
     * wave sums a chunk, a second pass adds the chunks of a segment in order. */
    int32_t cam_span;                 /* max over points of (largest - smallest observing camera index) */
    int32_t reserved;
    int64_t n_seg;                    /* number of NON-EMPTY block segments */
    const int32_t *seg_ids;           /* dev [n_seg]   segment id = camera * (cam_span + 1) + (camera - camera2) */
    const int32_t *seg_chunk_ptr;     /* dev [n_seg+1] first chunk of each segment */
    int64_t n_chunks;
    const int32_t *chunk_seg;         /* dev [n_chunks] index into seg_ids */
    const int32_t *chunk_begin, *chunk_end; /* dev [n_chunks] pair range */
    const int32_t *pair_o, *pair_o2;  /* dev [n_pairs] */
    const int32_t *pair_p;            /* dev [n_pairs] point index of each pair (= pi[pair_o]); NULL: looked up */
} mm_ba_problem;

/* res [O,2] (may be NULL) ; cost2 [1] receives sum of squared residuals (caller halves it). */
int mm_ba_residual(mm_ctx *ctx, const mm_ba_problem *pb, const double *cams /*dev [F,6]*/,
                   const double *pts /*dev [P,3]*/, double *res /*dev|NULL*/, double *cost2 /*dev [1]*/,
                   void *ws, size_t ws_bytes);
/* Analytic Jacobian blocks per observation: Jc [O,2,6], Jp [O,2,3] (parity / debugging surface). */
int mm_ba_jacobian(mm_ctx *ctx, const mm_ba_problem *pb, const double *cams, const double *pts, double *Jc,
                   double *Jp);
/* Block normal equations: B [F,6,6] = sum Jc^T Jc, gc [F,6] = sum Jc^T r, C [P,6] = upper triangle of sum Jp^T Jp
 * (xx,xy,xz,yy,yz,zz), gp [P,3] = sum Jp^T r.  Deterministic (segmented, atomic-free).  gc/B may be NULL when
 * cameras are fixed; C/gp may be NULL when points are fixed (pose-only, bundleAdjuster.py:206-243). */
int mm_ba_normal_eq(mm_ctx *ctx, const mm_ba_problem *pb, const double *cams, const double *pts, double *B,
                    double *gc, double *C, double *gp);
/* out [O,2] = Jc * wc[fi] + Jp * wp[pi]  (either w may be NULL = zero). */
int mm_ba_jvp(mm_ctx *ctx, const mm_ba_problem *pb, const double *cams, const double *pts, const double *wc,
              const double *wp, double *out);
/* mm_ba_jvp with its inner products fused in: rows [2,3] dev receives {0, s, s} for s = <out, other> (other == NULL:
 * <out, out>) and for s = <out, out> (the layout of mm_multi_dot's rows for residual-space vectors).  Deterministic. */
size_t mm_ba_jvp_dots_workspace_bytes(const mm_ba_problem *pb);
int mm_ba_jvp_dots(mm_ctx *ctx, const mm_ba_problem *pb, const double *cams, const double *pts, const double *wc,
                   const double *wp, double *out, const double *other /*dev [O,2] | NULL*/, double *rows /*dev [2,3]*/,
                   void *ws, size_t ws_bytes);
/* Reduced camera system.  Cd [P,6] = damped point blocks (C + reg*diag), Bd [F,6,6] damped camera blocks.
 * S [6F,6F] (row-major) = blockdiag(Bd) - sum_p E_p Cd_p^-1 E_p^T ;  v [6F] = gc - E Cd^-1 gp.
 * Cinv [P,6] receives Cd^-1 (upper triangle).  S and v are overwritten.
 * If the problem carries a co-observation pair list (mm_ba_build_pairs) the LOWER block band |i - j| <= cam_span of S
 * is computed by an atomic-free, bitwise reproducible kernel and the rest of S is zero; otherwise a general kernel
 * fills all of S (LDS f64 atomics, last bits vary from run to run). */
int mm_ba_schur(mm_ctx *ctx, const mm_ba_problem *pb, const double *cams, const double *pts, const double *Bd,
                const double *Cd, const double *gc, const double *gp, double *S, double *v, double *Cinv, void *ws,
                size_t ws_bytes);
/* partial sums and a descriptor per chunk, a counter per segment, a table row per camera, the slab flags (0 without chunks) */
size_t mm_ba_schur_workspace_bytes(const mm_ba_problem *pb);
/* The index structures of a problem, built on the device in two calls: the CSR by point over all observations, the CSR
 * by camera (stable) over the F free cameras, cam_span = the widest camera distance inside a point, and the pair list:
 * every (o, o2) of one point with camera(o2) <= camera(o) < F, sorted STABLY by key = camera(o) * (cam_span + 1) +
 * camera(o) - camera(o2) from the order o ascending, then o2 in pt_obs order; a segment per key, cut into chunks.
 * Cameras F .. F + F_fixed - 1 are fixed (mm_ba_fixed): their observations count for the CSR by point only.
 *   stage 0: pt_ptr [P+1], pt_obs [O], cam_ptr [F+1], cam_obs [O] and head [8] (dev): head[0] = cam_span, head[1] =
 *            number of pairs (0: no free camera observes anything), head[2] != 0: an index outside 0 <= fi < F + F_fixed,
 *            0 <= pi < P, head[3] != 0: not point-major, head[6] = n_free, the number of observations of free cameras:
 *            cam_obs[:n_free] is the CSR's.  With head[2] or head[3] set nothing else is valid.
 *            sort_by_point == 0 assumes POINT-MAJOR observations (pi non-decreasing, as mm_flatten_tracks emits them;
 *            pt_obs is then the identity) and reports others in head[3]; the caller then runs stage 0 again with
 *            sort_by_point != 0, which sorts (pi, identity) stably first and never sets head[3].
 *   stage 1: (the caller read head, set cam_span and n_pairs and allocated the pair arrays [n_pairs], seg_ids [seg_cap],
 *            seg_chunk_ptr [seg_cap + 1] and the chunk arrays [chunk_cap]: mm_ba_index_bounds)  the pair list in
 *            segment order, its segment and chunk tables, head[4] = n_seg, head[5] = n_chunks.  chunk = pairs per
 *            chunk, a multiple of 64.  Needs n_pairs > 0, cam_span < F and F * (cam_span + 1) < 2^31.  ws0 is stage 0's
 *            workspace, untouched since, and sort_by_point what stage 0 last ran with.
 * Workspaces (16-byte aligned): mm_ba_index_workspace_bytes(ctx, ix, stage); it asks the sort / scan library, which
 * needs the context's device, and returns 0 when it cannot. */
typedef struct mm_ba_index {
    int32_t F, P;
    int64_t O;
    int32_t F_fixed;                                /* cameras F .. F + F_fixed - 1 are observed but not optimised */
    int32_t sort_by_point;                          /* != 0: the observations come in any order */
    const int32_t *fi, *pi;                         /* dev [O] */
    int32_t *pt_ptr, *pt_obs, *cam_ptr, *cam_obs;   /* dev, stage 0 */
    int64_t *head;                                  /* dev [8] */
    int32_t cam_span, chunk;                        /* stage 1 inputs */
    int64_t n_pairs;
    int32_t *pair_o, *pair_o2, *pair_p;             /* dev [n_pairs], stage 1 */
    int32_t *seg_ids, *seg_chunk_ptr;
    int32_t *chunk_seg, *chunk_begin, *chunk_end;
} mm_ba_index;
int mm_ba_index_bounds(int F, int cam_span, int64_t n_pairs, int chunk, int64_t *seg_cap, int64_t *chunk_cap);
size_t mm_ba_index_workspace_bytes(mm_ctx *ctx, const mm_ba_index *ix, int stage);
int mm_ba_index_build(mm_ctx *ctx, const mm_ba_index *ix, int stage, void *ws0 /*dev*/, size_t ws0_bytes,
                      void *ws1 /*dev, stage 1*/, size_t ws1_bytes);
/* k <= 8 inner products <a_q, b_q> over vectors of length n in one launch (the trust-region driver's reductions, SciPy
 * trf.py via bundleAdjuster.py:180-192).  a, b: HOST arrays of k device pointers.  out [k,3] dev = {sum over i < split,
 * sum over i >= split, total}; deterministic.  The workspace must be zero-filled once before its first use. */
size_t mm_multi_dot_workspace_bytes(void);
int mm_multi_dot(mm_ctx *ctx, int k, const double *const *a, const double *const *b, int64_t n, int64_t split,
                 double *out, void *ws, size_t ws_bytes);
/* Fused element-wise passes of the 2-D subspace trust-region step (SciPy trf.py:478-494 via bundleAdjuster.py:180-192),
 * each accumulating the inner products the next pass needs (deterministic, reported like mm_multi_dot as rows of
 * {i < split, i >= split, total}; one more row holds maxima).  in / outv / scalars: HOST arrays of device pointers.
 *   op 0: in {g, si}                 outv {gh = g/si, ghs = gh/si}            out rows: gh.gh | max |g|
 *   op 1: in {v[split], dp[n-split], si, gh}  scalars {gh2}  outv {gn = [v;dp]*si, q1 = gh/sqrt(gh2)}   rows: q1.gn, gn.gn | -
 *   op 2: in {gn, q1}  scalars {sc}   outv {w = gn - sc q1}                    rows: w.w | -
 *   op 3: in {w, q1, si, gh, x}  scalars {wn2}  outv {q2 = w/sqrt(wn2), s1 = q1/si, s2 = q2/si}
 *                                                                              rows: s1.s1, s1.s2, s2.s2, q2.gh, x.x | -
 *   op 4: in {x, s1, s2}  h0, h1      outv {x + h0 s1 + h1 s2}                 (no result rows)
 *   op 5: in {x, s1, s2}  scalars {p[2]}  outv {x + p[0] s1 + p[1] s2}  with p in device memory (mm_trf_step2d);
 *         p[1] == 0 skips s2 (one-dimensional subspace)                        (no result rows)
 * out [(K+1), 3] dev; workspace as for mm_multi_dot (zero-filled once). */
int mm_trf_fused(mm_ctx *ctx, int op, const double *const *in, double *const *outv, const double *const *scalars,
                 double h0, double h1, int64_t n, int64_t split, double *out, void *ws, size_t ws_bytes);
/* Regulariser of the trust-region sub-problem on the device (SciPy trf.py:473-477, reached through
 * bundleAdjuster.py:180-192): gh2 = |g_h|^2, d11 = |J_h g_h|^2 (device scalars), Delta the radius.
 * out [2] dev = {reg, max(reg, min_damping)}. */
int mm_trf_damping(mm_ctx *ctx, const double *gh2, const double *d11, double Delta, double min_damping, double *out);
/* dp [P,3] = Cinv (gp - E^T dc).  With a workspace (mm_ba_backsub_workspace_bytes: 24 bytes per observation) the work is
 * spread over the observations and added per point in a second pass -- a launch with one thread per point waits for the
 * longest tracks; ws == NULL keeps that one-launch form.  Both are deterministic. */
size_t mm_ba_backsub_workspace_bytes(const mm_ba_problem *pb);
int mm_ba_backsub(mm_ctx *ctx, const mm_ba_problem *pb, const double *cams, const double *pts, const double *Cinv,
                  const double *gp, const double *dc /*dev [F,6]*/, double *dp, void *ws /*dev|NULL*/, size_t ws_bytes);
/* mm_ba_schur followed by mm_chol_solve(S, 6F, v, 1, half_bandwidth), overlapped: S is built in n_slabs ascending camera
 * slabs (slab s = cameras [s, s+1) * cams_per_slab; slab_seg_ptr / slab_chunk_ptr: HOST arrays [n_slabs+1] with the first
 * segment / chunk of each slab) on the context's stream while the single-launch banded factorisation runs on a second
 * stream and consumes block rows as their slabs complete.  The build is what mm_ba_schur launches -- zero fill of S, one
 * prepare launch, the pair kernel -- with the pair kernel cut in two: its first half runs alone, its second half beside
 * the factorisation.  On return (stream-ordered) v holds the solution and info the factorisation status.  Without a pair
 * list / slabs (2 .. 64 of at least 16 cameras), without points, or for bands the single-launch factorisation does not
 * take, the two steps simply run one after the other. */
int mm_ba_schur_solve(mm_ctx *ctx, const mm_ba_problem *pb, const double *cams, const double *pts, const double *Bd,
                      const double *Cd, const double *gc, const double *gp, double *S, double *v, double *Cinv,
                      int half_bandwidth, int32_t *info, void *ws_schur, size_t ws_schur_bytes, void *ws_chol,
                      size_t ws_chol_bytes, int n_slabs, int cams_per_slab, const int64_t *slab_seg_ptr,
                      const int64_t *slab_chunk_ptr);
/* Block glue of the trust-region driver (one launch each instead of a handful of tensor-library kernels):
 * scale_update: scale_inv [6F+3P] = sqrt of the diagonal of J^T J taken from B [F,6,6] and C [P,6] (packed upper
 *   triangle); first != 0: zeros become 1 (SciPy compute_jac_scale), else the running maximum with the stored value;
 * damp: Bd = B + reg diag(scale_inv_c^2), Cd = C + reg diag(scale_inv_p^2), reg [1] in device memory. */
int mm_ba_scale_update(mm_ctx *ctx, int F, int P, const double *B, const double *C, double *scale_inv /*in/out*/, int first);
int mm_ba_damp(mm_ctx *ctx, int F, int P, const double *B, const double *C, const double *scale_inv, const double *reg /*dev [1]*/,
               double *Bd, double *Cd);
/* The 2-D trust-region subproblem of a TRF iteration solved on the device (SciPy trf.py:481-494, common.py:171-219) from
 * the results of the fused passes, all still in device memory: r0 [2,3] (op 0), d11 [1,3] = <J g_hs, J g_hs>, r1 [3,3]
 * (op 1), r2 [2,3] (op 2), r3 [6,3] (op 3), bs [2,3] = {<u1, J s2>, <J s2, J s2>} (the "total" column of each is used),
 * reg [1] the damping in use, info [1] the factorisation status.  board [14] receives p0, p1 (step in the orthonormal
 * basis; feed them to mm_trf_fused op 5), predicted reduction, |p|, unscaled step norm, degenerate flag, info, and the
 * scalars the host-side bookkeeping needs (wn2, gn2, |x|^2, |g|_inf, |g_h|^2, d11, reg): one read-back per trial step. */
int mm_trf_step2d(mm_ctx *ctx, const double *r0, const double *d11, const double *r1, const double *r2, const double *r3,
                  const double *bs, const double *reg, const int32_t *info, double Delta, double *board /*dev [14]*/);
/* The whole trust-region solve of adjustPoints in ONE call (single GPU; replaces the loop scipy.optimize.least_squares
 * runs for bundleAdjuster.py:180-192: method='trf', x_scale='jac', linear loss, exact Schur-complement step instead of
 * LSMR).  Sequences exactly the calls above the way meatmodeler_amd/bundleAdjuster.py does -- bit-identical iterates --
 * with the host side of an iteration in C++: one 16-double read-back per trial step, no allocation.
 * cams [F,6] / pts [P,3] dev: initial values in, solution out.  log (HOST, may be NULL with log_cap 0) receives one row
 * per line of SciPy's verbose=2 table; report->log_rows counts the rows produced (may exceed log_cap).
 * status: SciPy's (0 max_nfev, 1 gtol, 2 ftol, 3 xtol, 4 both).  Returns MM_ERR_NUMERIC if the residuals are not finite
 * at the start or the reduced system stays indefinite after six 100x increases of the damping. */
typedef struct mm_trf_params {
    double ftol, xtol, gtol;
    double min_damping;   /* floor of the damping relative to the unit diagonal of the scaled system (<= 0: 1e-9) */
    int64_t max_nfev;     /* <= 0: 100 * (6F + 3P) */
} mm_trf_params;
typedef struct mm_trf_row {
    int32_t iteration, nfev;
    double cost, reduction, step_norm, optimality;   /* reduction / step_norm are NaN on the first row */
} mm_trf_row;
typedef struct mm_trf_report {
    double cost0, cost, optimality, min_damping /* as raised during the solve */;
    int32_t nfev, njev, status, iterations, log_rows;
    int32_t chol_fallbacks;   /* times the solve switched to the launch-per-column factorisation (info = -1 seen): 0 or 1 */
    int32_t collectives;      /* mm_ba_trf_dist: all-reduce calls made (7 per trust-region iteration + 3 at the start) */
    int32_t reserved;
} mm_trf_report;
size_t mm_ba_trf_workspace_bytes(const mm_ba_problem *pb);
int mm_ba_trf(mm_ctx *ctx, const mm_ba_problem *pb, double *cams /*dev, in/out*/, double *pts /*dev, in/out*/,
              const mm_trf_params *prm, mm_trf_report *report /*host*/, mm_trf_row *log /*host|NULL*/, int log_cap,
              void *ws /*dev, 256-byte aligned*/, size_t ws_bytes);
/* The same loop SHARDED over the GPUs of a node (one process per GPU): `pb` holds this rank's points
 * with all their observations (point indices local), the cameras are replicated, `pts` is the rank's shard.  Every sum
 * over observations / points is completed by the caller's all-reduce -- the library does not link a communication
 * library: `allreduce(user, buf, count)` must sum `count` doubles at the DEVICE pointer `buf` (inside the workspace) over
 * the ranks, in place, ordered after the work already on the context's stream and before what follows (RCCL:
 * ncclAllReduce(buf, buf, count, ncclDouble, ncclSum, comm, stream); torch.distributed: all_reduce on a tensor view of the
 * workspace), and return 0.  Per trust-region iteration: {B, g_c} | {|g_h|^2, |g|_inf, |J d g_h|^2} | {band of S, v} |
 * {<q1, gn_h>, |gn_h|^2} | {|w|^2} | {the five step inner products, <u1, J s2>, |J s2|^2} | {trial cost, "a rank's
 * factorisation was abandoned"} -- seven collectives, six of them one 64-double vector (the chain of dependent scalars of
 * SciPy's 2-D subspace step does not get shorter than the four groups it has).
 *   half_bandwidth: of the reduced camera system, from the GLOBAL camera span (6 * max over ranks of cam_span + 5);
 *   band_exchange != 0: every rank's S is confined to that band (all shards have a pair list): n (hb + 1) + n doubles are
 *     exchanged instead of n^2 + n.  Both must be the same on every rank (decide them from all-reduced quantities).
 * All ranks see identical scalars and take identical decisions; the replicated cameras come out bit-identical: that
 * includes the choice between the two factorisation paths (a rank whose context is set to avoid the single launch, finds
 * no room in the co-residency budget, or sees its factorisation abandoned tells the others inside the exchanges above
 * and all switch together).
 * FATAL ERRORS ARE GROUP-WIDE: a non-zero return of the callback, or any error on one rank, makes THAT rank return; its
 * peers are then waiting inside their next all-reduce.  The caller must treat a failed mm_ba_trf_dist as fatal for the
 * whole group (abort / destroy the communicator, which releases the peers with an error, or rely on its timeout). */
typedef int (*mm_allreduce_fn)(void *user, double *buf /*dev*/, int64_t count);
typedef struct mm_dist {
    int32_t rank, world;   /* world <= 16 */
    int32_t half_bandwidth, band_exchange;
    mm_allreduce_fn allreduce;
    void *user;
} mm_dist;
size_t mm_ba_trf_dist_workspace_bytes(const mm_ba_problem *pb, int half_bandwidth);
int mm_ba_trf_dist(mm_ctx *ctx, const mm_ba_problem *pb, double *cams, double *pts, const mm_trf_params *prm,
                   mm_trf_report *report, mm_trf_row *log, int log_cap, void *ws, size_t ws_bytes, const mm_dist *dist);
/* SEVERAL INDEPENDENT PROBLEMS IN LOCK-STEP (the sliding-window adjustment; hook at reference
 * processor.py:395-408: the windows of one colour of the wavefront schedule share no camera).  Every kernel of mm_ba_trf's loop
 * is launched once per round for all problems (blockIdx.y = problem; per-problem grids and bodies identical to the
 * single-problem kernels), the host reads one 16-double mailbox per problem and round and takes each problem's accept /
 * reject / terminate decision exactly as mm_ba_trf does: cams[p] / pts[p] / reports[p] come out BIT-IDENTICAL to n_prob calls
 * of mm_ba_trf.  A reduced system that is not positive definite is retried with 100x the damping inside the batch, as
 * mm_ba_trf does; a problem whose factorisation was abandoned (info = -1) or that stays indefinite after six raises is
 * solved by mm_ba_trf itself after the batch, from its initial point (solved_alone[p] = 1; may be NULL);
 * if a problem cannot be batched at all (no co-observation pair list, reduced system outside the single-launch
 * factorisation, n_prob == 1) the call solves them one after the other.
 * pbs / cams / pts / ws / ws_bytes: HOST arrays of n_prob entries; ws[p] >= mm_ba_trf_batched_workspace_bytes(pbs[p]),
 * 256-byte aligned.  Problems must not share buffers.  (sync) */
size_t mm_ba_trf_batched_workspace_bytes(const mm_ba_problem *pb);
int mm_ba_trf_batched(mm_ctx *ctx, int n_prob, const mm_ba_problem *const *pbs, double *const *cams /*dev, in/out*/,
                      double *const *pts /*dev, in/out*/, const mm_trf_params *prm, mm_trf_report *reports /*host [n_prob]*/,
                      void *const *ws /*dev*/, const size_t *ws_bytes, int32_t *solved_alone /*host [n_prob] | NULL*/);
/* FIXED CAMERAS (the anchored sliding window; hook at reference processor.py:395-408: the cameras
 * older than the window are observed but not optimised).  A side descriptor to an unchanged mm_ba_problem: observations with
 * fi in [pb->F, pb->F + F_fixed) use fixed camera fi - pb->F, whose 6 parameters (rvec, t) are read-only inputs.  The
 * residual is bundleAdjuster.py:81-102 on [free cams | fixed cams | points]; the solve is the one of mm_ba_trf
 * (bundleAdjuster.py:180-192) over the FREE parameters [free cams | points] only: n = 6F + 3P, and every norm, scale and
 * termination test (|x| of the xtol test included) is over those n entries.  Fixed-camera observations enter the residual,
 * the cost, the point blocks C / g_p and the point half of J v -- not B, g_c, the pair list, S or cam_span.  So the CSR by
 * camera (cam_ptr / cam_obs) covers the F free cameras and the pair list holds free-free pairs only (mm_ba_index_build
 * with F_fixed makes both).  The caller guarantees fi < F + F_fixed.
 * fx == NULL or F_fixed == 0: exactly the call without _fixed. */
typedef struct mm_ba_fixed {
    int32_t F_fixed;        /* observations with fi in [pb->F, pb->F + F_fixed) use these cameras */
    int32_t reserved;
    const double *cams;     /* dev [F_fixed, 6], read only */
} mm_ba_fixed;
/* mm_ba_residual / mm_ba_normal_eq with fixed cameras (parity surface): B / gc cover the free cameras. */
int mm_ba_residual_fixed(mm_ctx *ctx, const mm_ba_problem *pb, const mm_ba_fixed *fx, const double *cams /*dev [F,6]*/,
                         const double *pts /*dev [P,3]*/, double *res /*dev|NULL*/, double *cost2 /*dev [1]*/, void *ws,
                         size_t ws_bytes);
int mm_ba_normal_eq_fixed(mm_ctx *ctx, const mm_ba_problem *pb, const mm_ba_fixed *fx, const double *cams, const double *pts,
                          double *B, double *gc, double *C, double *gp);
/* mm_ba_trf with fixed cameras: the same loop, the same launches per trust-region iteration (the fixed cameras' rotation
 * coefficients are computed once per solve), the same fall-back to the launch-per-column factorisation.  cams [F,6] are the
 * free cameras (in/out), fx->cams are never written.  Needs the co-observation pair list (MM_ERR_ARG without one). */
size_t mm_ba_trf_fixed_workspace_bytes(const mm_ba_problem *pb, const mm_ba_fixed *fx);
int mm_ba_trf_fixed(mm_ctx *ctx, const mm_ba_problem *pb, const mm_ba_fixed *fx, double *cams /*dev, in/out*/,
                    double *pts /*dev, in/out*/, const mm_trf_params *prm, mm_trf_report *report /*host*/,
                    mm_trf_row *log /*host|NULL*/, int log_cap, void *ws /*dev, 256-byte aligned*/, size_t ws_bytes);
/* SPD solve A x = b by blocked Cholesky (f64 MFMA trailing updates).  A [n,n] row-major, lower triangle is
 * overwritten by L; b [nrhs,n] is overwritten by x.  half_bandwidth: A[i][j] == 0 whenever i - j > half_bandwidth
 * (pass n for a dense matrix); the factorisation and the substitutions skip blocks outside the band.
 * info [1] dev int32: 0 ok, k>0 = non-positive pivot at column k, -1 = the single-launch banded factorisation gave up
 * waiting for a block (its spin loops are bounded so that a scheduling surprise cannot hang the GPU; mm_ba_trf then
 * repeats the solve on the launch-per-column path).
 * Narrow bands (<= 15 blocks of 64) are factored by ONE data-flow scheduled launch, everything else by three launches
 * per block column; MM_CHOL_FUSED=0 in the environment forces the latter.  The workgroups of the single launch wait for
 * each other, so all of them must be resident (one per compute unit): every launch reserves its grid out of a
 * per-process budget of the device's compute units, held until the context's next synchronisation (mm_ctx_sync, the
 * end of mm_ba_trf); a launch that does not fit -- several contexts solving at once -- takes the per-column path. */
size_t mm_chol_workspace_bytes(int n);
/* Solution only: A x = b for ONE right-hand side, A destroyed (the layout of the factor it is overwritten with is
 * unspecified).  both_triangles != 0: both triangles of the band hold A on input; 0: only the lower one (the band of the
 * upper triangle is then filled from it first).  This freedom lets a narrow band be eliminated from BOTH ends at once
 * (chain of ~(nblk + bwb) / 2 dependent block columns instead of nblk): what the bundle adjustment calls per
 * trust-region iteration.  MM_CHOL_TWISTED=0 in the environment forces the one-ended elimination.
 * info: as for mm_chol_solve while the elimination is one-ended.  The two-ended elimination runs in another order than
 * LAPACK's, and on the reversed side a failure spreads towards SMALLER columns: a matrix that is not positive definite (or
 * holds a NaN) then gives 1 <= info <= n, some column at which a pivot was not positive, not necessarily the first. */
int mm_chol_solve_sym(mm_ctx *ctx, double *A /*dev*/, int n, double *b /*dev [n]*/, int half_bandwidth, int both_triangles,
                      int32_t *info /*dev*/, void *ws, size_t ws_bytes);
int mm_chol_solve(mm_ctx *ctx, double *A /*dev*/, int n, double *b /*dev*/, int nrhs, int half_bandwidth,
                  int32_t *info /*dev*/, void *ws, size_t ws_bytes);

/* ---- keyframe gating front end (reference processor.py:61-110 keyframeTracking) ------------------------------------------
 * The arithmetic of the three calls is defined by oracle/frame_oracle.c (OpenCV's published algorithms made integer exact;
 * OpenCV itself is absent offline: parity unpinned) and reproduced bit for bit.
 * mm_pyr_down: one pyramid level, 5-tap [1 4 6 4 1]/16, reflect-101: dst [(h+1)/2, (w+1)/2].
 * mm_lk_track: cv2.calcOpticalFlowPyrLK(prev, next, pts, None, winSize, maxLevel, criteria) (processor.py:79) on pyramids
 *   built with mm_pyr_down.  prev_levels / next_levels / w / h / pitch: HOST arrays of `levels` (= maxLevel + 1) device
 *   pointers / sizes; pts [n,2] f32 dev.  next_pts [n,2] f32, status [n] u8, err [n] f32 (dev).  window 3..41, <= 8 levels.
 * mm_min_eig: Shi-Tomasi minimum eigenvalue map [h,w] f64 (cornerMinEigenVal scaling for 8-bit input), block size 1..15.
 * mm_corner_candidates: pixels above quality * max that survive the 3x3 non-maximum suppression -> value bit patterns
 *   [cap] i64 and flat positions [cap] i32 (unordered), count [1]; the caller sorts (value desc, position asc) and runs
 * mm_gftt_select (host): greedy minimum-distance selection of cv2.goodFeaturesToTrack (processor.py:104). */
int mm_pyr_down(mm_ctx *ctx, const uint8_t *src /*dev*/, int w, int h, int src_pitch, uint8_t *dst /*dev*/, int dst_pitch);
int mm_lk_track(mm_ctx *ctx, const uint8_t *const *prev_levels, const uint8_t *const *next_levels, const int *w, const int *h,
                const int *pitch, int levels, const float *pts, int n, int win_w, int win_h, int max_count,
                double epsilon_sq, float *next_pts, uint8_t *status, float *err);
int mm_min_eig(mm_ctx *ctx, const uint8_t *img /*dev*/, int w, int h, int pitch, int block_size, double *eig /*dev*/);
int mm_corner_candidates(mm_ctx *ctx, const double *eig, int w, int h, double quality, unsigned long long *max_bits /*dev [1]*/,
                         long long *val_bits /*dev [cap]*/, int32_t *pos /*dev [cap]*/, int cap, int32_t *count /*dev [1]*/);
int mm_gftt_select(const int32_t *pos /*host [n], sorted*/, int64_t n, int w, int h, int max_corners, double min_distance,
                   float *out /*host [cap,2]*/, int cap);
/* ---- increaseContrast + grey (reference processor.py:12-26, :357) and the PLY export (processor.py:480-485) ---------------
 * mm_increase_contrast: bgr [batch,h,w,3] u8 -> out (same shape), optionally grey [batch,h,w] of the result: fixed-point
 *   BGR <-> L*a*b* with the tables of meatmodeler_amd/frame_tables.py (gamma [256] u16, cbrt_tab [4096] u16, gamma_inv
 *   [4096] u8, device), CLAHE(clip_limit, tiles) on L.  mm_bgr_to_grey: (1868 B + 9617 G + 4899 R + 8192) >> 14.
 * mm_write_ply (host): binary little-endian PLY, double x / y / z per vertex. */
size_t mm_contrast_workspace_bytes(int batch, int w, int h, int tiles_x, int tiles_y);
int mm_increase_contrast(mm_ctx *ctx, const uint8_t *bgr, int batch, int w, int h, const uint16_t *gamma,
                         const uint16_t *cbrt_tab, const uint8_t *gamma_inv, double clip_limit, int tiles_x, int tiles_y,
                         uint8_t *out, uint8_t *grey /*dev|NULL*/, void *ws, size_t ws_bytes);
int mm_bgr_to_grey(mm_ctx *ctx, const uint8_t *bgr /*dev [n,3]*/, size_t n_pixels, uint8_t *grey /*dev [n]*/);
int mm_write_ply(const char *path, const double *xyz /*host [n,3]*/, int64_t n);

#ifdef __cplusplus
}
#endif
#endif /* MEATMODELER_H */
