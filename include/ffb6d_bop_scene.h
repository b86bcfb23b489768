/* include/ffb6d_bop_scene.h -- C ABI of the two steps between the BOP pose errors of include/ffb6d_bop.h and a BOP19 number of a
 * scene with several instances and several scored estimates: which ground-truth instances are targets (instance visibility in the
 * measured depth), and which estimate answers which instance (greedy matching by score, once per error function and threshold).
 * There is no BOP toolkit to port or to compare with: the rules are stated here in full and restated in numpy by
 * tests/bop_scene_ref.py, which the kernels are held against bit for bit.  Nothing here claims to reproduce the bytes of the
 * files the BOP datasets publish (scene_gt_info.json, mask_visib): their renderer differs, and see bbox_obj below.
 *
 * Every float operation below is rounded on its own, in the order written (the library is built with -ffp-contract=off).
 *
 * ffb6d_bop_visib_f32 -> info i32 [Q,12], visib_fract f64 [Q], mask_visib u8 [Q,H,W] (optional)
 *   depth_test f32 [B,H,W] metres, the measured depth;  depth_obj f32 [Q,H,W], row q's model rendered ALONE under its pose
 *   frame_of i32 [Q];  K f64 [B,3,3] (only fx = K[0], fy = K[4], cx = K[2], cy = K[5] are read);  delta (metres)
 *   Per pixel (r, c) of row q, b = frame_of[q], all in float:
 *     t, g    = the test and the object depth, taken as 0 unless > 0 && <= FLT_MAX (not finite or <= 0: no measurement / nothing
 *               drawn; the sanitising ffb6d_bop_vsd_f32 applies to the test image, applied here to both images)
 *     dt, dg  = dist(t), dist(g) with dist exactly as in ffb6d_bop.h (same operations, same order, correctly rounded division
 *               and square root, the intrinsics narrowed to float first)
 *     obj     = dg > 0
 *     valid   = obj && dt > 0
 *     visib   = obj && (dt == 0 || dg - dt <= delta)                     (vis_gt of the VSD rule)
 *     support = valid && dg - dt <= delta && dt - dg <= delta            (the measured depth agrees with the rendered one)
 *   info[q] = px_count_all (obj), px_count_valid, px_count_visib, px_count_support,
 *             bbox_obj = x, y, w, h over the obj pixels, bbox_visib = x, y, w, h over the visib pixels
 *     with x = min column, y = min row, w = max column - min column + 1, h likewise; -1, -1, -1, -1 when there is no such pixel.
 *     bbox_obj covers the part of the silhouette INSIDE the frame (it is taken from the rendered image); the published BOP files
 *     extend it beyond the frame.
 *   visib_fract[q] = (double)px_count_visib / (double)px_count_all, 0.0 when px_count_all == 0
 *   mask_visib[q,r,c] = 1 where visib, 0 elsewhere
 *   px_count_support / px_count_all of an ESTIMATED pose is the usual plausibility score of an estimate: how much of the rendered
 *   model the measured depth supports.
 *   A row whose frame id is outside [0, B) gives counts 0, boxes -1, visib_fract NaN and an all-zero mask; nothing is read through
 *   the bad index.  Integer sums, minima and maxima: exact whatever the reduction shape.
 *
 * ffb6d_bop_match_f64 -> est_gt i32 [Etot, n_col, n_thr], gt_est i32 [Gtot, n_col, n_thr]
 *   G groups; a group is one (frame, object) of a test set with E_g estimates and T_g ground-truth instances.
 *   est_begin i32 [G+1], gt_begin i32 [G+1]   prefix tables: group g owns the estimates est_begin[g] .. est_begin[g+1]-1 (E_g of
 *                                             them) and the instances gt_begin[g] .. gt_begin[g+1]-1 (T_g)
 *   pair_begin i64 [G+1]                      pair_begin[g+1] - pair_begin[g] = E_g * T_g
 *   err f64 [Npairs, n_col]                   the pair (e, t) of group g (local indices) is row pair_begin[g] + e * T_g + t: the
 *                                             rows ffb6d_bop_mssd_mspd_f64 and ffb6d_bop_vsd_f32 produce (n_col = 1, or n_tau)
 *   score f32 [Etot];  thr f64 [G, n_thr] (per-group thresholds such as theta * diameter);  max_ests i32 [G] or null
 *   Independently for every group g and every configuration (col, k):
 *     - estimates are ordered by score descending; a NaN score counts as -inf; ties go to the lower index;
 *     - only the first max_ests[g] of that order are considered when max_ests is given and max_ests[g] > 0 (0: all); the others
 *       get -1;
 *     - each considered estimate in turn takes, among the instances nobody has taken yet, the one with the smallest
 *       err[pair][col] that is < thr[g][k] (strict: a NaN never matches, an error equal to the threshold does not either); ties
 *       go to the lower instance index; if there is none it takes nothing;
 *     - est_gt = the LOCAL index of the instance the estimate took, or -1; gt_est = the local index of the estimate that took the
 *       instance, or -1.  Every entry of every group is written, so the outputs need no fill.
 *   Whether an instance is a valid target (visib_fract) plays no part in matching; it decides only what is counted afterwards.
 *   Caps: E_g, T_g <= FFB6D_BOP_MAX_GROUP, n_col <= 16, n_thr <= 16.  The tables live in device memory and nothing is read back:
 *   ffb6d_bop_match_check validates the HOST copies before the upload (the pattern of ffb6d_jitter_frames_check).  A group whose
 *   table entries break a cap, run past Etot / Gtot / Npairs or miss the pair_begin identity is not matched: the kernel writes -1
 *   into at most FFB6D_BOP_MAX_GROUP of the entries it names that lie inside the outputs, and never indexes out of range.
 *
 * All pointers are DEVICE pointers except those of ffb6d_bop_match_check; a call enqueues its work on `stream` and returns
 * without waiting for it or reading anything back.  Return value: 0 or an FFB6D_ERR_* code (text through ffb6d_last_error()); on
 * an error nothing is launched and no output is written.
 */
#ifndef FFB6D_BOP_SCENE_H
#define FFB6D_BOP_SCENE_H

#include <stddef.h>
#include <stdint.h>

#include "ffb6d_knn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FFB6D_BOP_MAX_GROUP 64
#define FFB6D_BOP_MAX_MATCH_COLS 16
#define FFB6D_BOP_MAX_MATCH_THRS 16
#define FFB6D_BOP_INFO_INTS 12

/* Bytes of workspace of ffb6d_bop_visib_f32 (0 for sizes the call refuses and for Q = 0): per row and per run of 4096 pixels one
 * record of 12 integers (4 counts, 4 minima, 4 maxima); rounded up to 256 bytes. */
size_t ffb6d_bop_visib_workspace_bytes(int Q, int H, int W);

/* 0 <= Q <= 65535 (Q = 0: nothing to do), B > 0, H, W > 0, H*W < 2^31 - 4096; info and visib_fract are both written, mask_visib
 * may be NULL (not written).  Two launches: a streaming pass over the two images (16-byte accesses and 4-byte mask stores where
 * H*W is a multiple of 4, the images are 16-byte and the mask is 4-byte aligned; single floats and bytes otherwise) writes one
 * partial record per (row, run) into the workspace, which may hold anything on entry; one wavefront per row combines them. */
int ffb6d_bop_visib_f32(const float* depth_test, const float* depth_obj, const int* frame_of, int Q, const double* K, int B, int H,
                        int W, float delta, int* info, double* visib_fract, uint8_t* mask_visib, void* workspace,
                        size_t workspace_bytes, ffb6d_stream_t stream);

/* HOST pointers, no GPU: 0 when the tables are ones ffb6d_bop_match_f64 matches every group of -- G >= 0, 1 <= n_col <= 16,
 * 1 <= n_thr <= 16, est_begin[0] = gt_begin[0] = pair_begin[0] = 0, the begins monotone and ending at Etot / Gtot / Npairs,
 * every E_g and T_g <= FFB6D_BOP_MAX_GROUP, pair_begin[g+1] - pair_begin[g] = E_g * T_g, max_ests (may be NULL) >= 0. */
int ffb6d_bop_match_check(const int* host_est_begin, const int* host_gt_begin, const int64_t* host_pair_begin,
                          const int* host_max_ests, int G, int64_t Etot, int64_t Gtot, int64_t Npairs, int n_col, int n_thr);

/* The matching needs no workspace: always 0.  Here so that every call of the library is sized the same way. */
size_t ffb6d_bop_match_workspace_bytes(int G, int n_col, int n_thr);

/* G >= 0 (G = 0: nothing to do), 0 <= Etot, Gtot <= INT_MAX, Npairs >= 0; err may be NULL when Npairs = 0, score / est_gt when
 * Etot = 0, gt_est when Gtot = 0; max_ests may be NULL; workspace is not used.  One launch, one workgroup of 256 lanes per group:
 * lanes e < E_g rank the estimates by counting, then lane = configuration walks them with a 64-bit taken mask. */
int ffb6d_bop_match_f64(const int* est_begin, const int* gt_begin, const int64_t* pair_begin, int G, int64_t Etot, int64_t Gtot,
                        int64_t Npairs, const double* err, int n_col, const float* score, const double* thr, int n_thr,
                        const int* max_ests, int* est_gt, int* gt_est, void* workspace, size_t workspace_bytes,
                        ffb6d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
