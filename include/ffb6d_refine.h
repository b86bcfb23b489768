/* include/ffb6d_refine.h -- C ABI of the gfx950 ICP pose refinement: the step that follows the keypoint fit
 * (ffb6d_best_fit_transform_f32, include/ffb6d_pose.h).  The reference repository has no ICP code; the algorithm is
 * stated here and restated in numpy by tests/icp_ref.py.
 *
 * Point-to-point ICP, scene -> model, for P problems at once.  Problem p = (frame frame_of[p], class class_of[p],
 * pose T[p] = [R|t], row-major double [3,4], model -> camera).  Its scene points are the points i of pcld[frame] with
 * mask[frame,i] == class (and keep[frame,i] != 0 when keep is given), in index order; its model cloud is the class's
 * rows of the prepared model set.  One iteration, R and t rounded once from double to float32:
 *   1. q_i = R^T (s_i - t) in float32: d = s_i - t, q_j = ((d0*R0j + d1*R1j) + d2*R2j), every product and sum rounded
 *   2. m(i) = the model point with the smallest ((dx*dx + dy*dy) + dz*dz) (float32, every operation rounded); equal
 *      distances resolve to the lowest model index
 *   3. the pair is kept when d2 <= max_dist * max_dist (float32; a NaN distance is never kept; max_dist = inf keeps all)
 *   4. [R|t] <- the reflection-corrected least-squares transform model[m(i)] -> s_i over the kept pairs, in double from
 *      the float inputs (the arithmetic of ffb6d_best_fit_transform_f32 after the sums; the sums are made per block of
 *      64 scene points and added in block order: no atomics, the same bits in every run).  H is formed in one pass,
 *      H = sum m s^T - n c_a c_b^T, so the accuracy stated for ffb6d_best_fit_transform_f32 holds with cond multiplied by
 *      (s1 + n |c_a| |c_b|) / s1: max |R - R_svd| <= 9.2e-14 * cond * (s1 + n |c_a| |c_b|) / s1 -- a model cloud given
 *      about its own centre loses nothing, one given far from its origin loses the cancellation
 *   5. the problem stops after max_iter iterations; earlier when fewer than min_pairs pairs were kept (the pose of
 *      that iteration is left as it is) or, with tol > 0, when the update moved no corner of the model's bounding
 *      box by more than tol metres.
 * A class without model points, a class id outside [0, n_cls), a frame index outside [0, B) or an empty scene set
 * give a problem without pairs: its pose comes back as the bits that went in.
 *
 * All pointers are DEVICE pointers unless stated; ffb6d_icp_correspond_f32 and ffb6d_icp_refine_f32 enqueue their work
 * on `stream` and return without waiting for it or reading anything back.  Return value: 0 or an FFB6D_ERR_* code
 * (text through ffb6d_last_error()); on an error nothing is launched and no output is written.
 */
#ifndef FFB6D_REFINE_H
#define FFB6D_REFINE_H

#include <stddef.h>
#include <stdint.h>

#include "ffb6d_knn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The model set prepared for the search, made once per model set:
 *   model_pts f32 [total,3], model_begin i64 [n_cls+1] (class c = rows model_begin[c] .. model_begin[c+1]-1, the
 *   buffers of the evaluation, include/ffb6d_eval.h)  ->  `prepared`, ffb6d_icp_prepared_bytes(total, n_cls) bytes:
 *   every class in Morton order in tiles of 64 points {x, y, z, bit-cast index within the class}, the bounding box of
 *   every tile and of every class, and the clouds in their own order.
 * ffb6d_icp_prepare copies the clouds to the host, orders them there and uploads the result: it WAITS for `stream`
 * (once per model set; the searches never wait).  total < 2^31. */
size_t ffb6d_icp_prepared_bytes(int64_t total, int n_cls);
int ffb6d_icp_prepare(const float* model_pts, const int64_t* model_begin, int n_cls, int64_t total, void* prepared,
                      size_t prepared_bytes, ffb6d_stream_t stream);

/* Bytes of workspace of ffb6d_icp_correspond_f32 / ffb6d_icp_refine_f32 for P problems (0 when P <= 0 or
 * set_stride <= 0): the scene sets [P, set_stride] float4 {x, y, z, bit-cast index of the cloud point} (the vote-set
 * layout of include/ffb6d_pose.h), 17 doubles per block of 64 scene points, and the state of every problem. */
size_t ffb6d_icp_workspace_bytes(int P, int64_t set_stride);

/* 0 (default) = scan: every scene point is compared with every model point of its class (the model streams through LDS);
 * 1 = pruned: a wavefront takes one scene point at a time against whole tiles (one model point per lane), nearest
 *     tile box first, and skips every tile whose box is farther than the best distance found so far;
 * -1 = automatic: pruned for the classes of at least 1024 model points, scan below.  Identical results. */
void ffb6d_icp_set_form(int form);

/* Counts the (scene point, model point) pairs whose distance is evaluated into *device_counter (one atomic per
 * wavefront, not on the result path); NULL (default) = off. */
int ffb6d_icp_set_pair_counter(unsigned long long* device_counter);

/* Steps 1-3 once, for P problems under the poses T f64 [P,3,4]:
 *   pcld f32 [B,N,3]; mask int32|int64 [B,N] (mask_bits = 32|64); keep u8 [B,N] or NULL; frame_of, class_of i32 [P];
 *   set_stride >= N;
 *   idx i32 [P,set_stride]: for the j-th scene point of the problem the index of its model point within the class,
 *       -1 where the pair is not kept or j is beyond the problem's count;   d2 f32 [P,set_stride]: the smallest
 *       squared distance, kept or not (NaN for a NaN scene point, +inf beyond the count or without model points);
 *   counts i32 [P]: scene points of the problem.  idx, d2, counts may each be NULL. */
int ffb6d_icp_correspond_f32(const void* prepared, int n_cls, int64_t total, const float* pcld, const void* mask,
                             int mask_bits, const unsigned char* keep, const int* frame_of, const int* class_of,
                             const double* T, int P, int B, int N, int64_t set_stride, float max_dist, int* idx,
                             float* d2, int* counts, void* workspace, size_t workspace_bytes, ffb6d_stream_t stream);

/* The whole loop from the poses T0 f64 [P,3,4]:
 *   T f64 [P,3,4] the refined poses (may be T0 itself); n_pairs i32 [P] and rms f32 [P]: pairs kept by the last
 *   iteration made and the root of their mean d2 (measured before that iteration's update; 0 without pairs);
 *   iters i32 [P]: updates made.  T, n_pairs, rms, iters may each be NULL.
 *   max_dist > 0 (inf allowed), max_iter >= 0, tol >= 0 (0 = no early stop), min_pairs >= 1.
 * One launch for the scene sets and two per iteration (P <= 65535); a finished problem costs an early exit per block. */
int ffb6d_icp_refine_f32(const void* prepared, int n_cls, int64_t total, const float* pcld, const void* mask,
                         int mask_bits, const unsigned char* keep, const int* frame_of, const int* class_of,
                         const double* T0, int P, int B, int N, int64_t set_stride, float max_dist, int max_iter,
                         double tol, int min_pairs, double* T, int* n_pairs, float* rms, int* iters, void* workspace,
                         size_t workspace_bytes, ffb6d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
