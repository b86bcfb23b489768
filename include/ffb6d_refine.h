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
 * Several instances of a class in a frame (ffb6d_icp_correspond_inst_f32, ffb6d_icp_refine_inst_f32).  Problem p becomes
 * (frame_of[p], class_of[p], inst_of[p], T[p]); inst is the u8 [B,N] map of ffb6d_set_clusters_to_points
 * (include/ffb6d_pose.h; 0 = no instance); tests/icp_inst_ref.py restates what follows.  Steps 1, 2, 4 and 5 are the
 * ones above; the scene set and step 3 depend on `mode`:
 *   mode 0, map.  The scene points are the points with mask == class && inst == inst_of[p] (and keep != 0 when given), in
 *     index order.  Step 3 is unchanged.  An inst_of outside 1 .. 255 gives a problem without pairs: its pose comes back as
 *     the bits that went in.
 *   mode 1, nearest.  The scene points are the points with mask == class (and keep), in index order, whatever their
 *     instance id (inst is not read and may be NULL; inst_of only names what is written to inst_out).
 *     The GROUP of p is the maximal run of adjacent problems with the same frame_of and class_of (pose.solve_instances orders
 *     its rows by (frame, class, instance), so its groups are the instances of a pair; equal pairs that are not adjacent form
 *     separate groups).  After steps 1-2 of every problem of the group, the OWNER of scene point i is the group member with
 *     the smallest d2: the comparison is in float32, a NaN distance never owns, equal distances go to the lowest problem
 *     index.  Step 3 becomes: the pair is kept for p when p owns i AND d2 <= max_dist * max_dist.  A problem that has stopped
 *     (step 5) keeps its pose and goes on competing under it until the loop ends.
 * The sums of step 4 are made as above, per block of 64 scene points of the problem's set and added in block order, without
 * atomics: a map-mode problem whose set equals a class problem's set gives that call's bits, and so does a nearest-mode
 * problem alone in its group.
 * inst_out u8 [B,N] (zeroed by the call, on the stream): inst_out[frame, i] = the low 8 bits of inst_of[p] where p keeps the
 * pair of point i, 0 elsewhere.  Mode 0: the pairs p kept in the last iteration it made (a problem that stopped early: in
 * that iteration, before its update).  Mode 1: the pairs kept in the loop's last iteration, iteration max_iter - 1, stopped
 * problems included, under the poses that went into it; max_iter = 0 leaves it zero.  Within a group a point has one owner,
 * and the sets of distinct map-mode problems are disjoint, so a point has one writer and no atomics are needed; problems that
 * repeat a (frame, class, instance) in mode 0, or a (frame, class) in separate groups in mode 1, may keep the same point:
 * it then carries the id of either.
 *
 * The point-to-plane metric (the *_plane calls; tests/icp_plane_ref.py restates what follows).  It minimises the distance of
 * every scene point to the tangent plane at its model point, so a scene point may slide along the surface.  It needs one unit
 * normal per model point, in a second buffer next to `prepared`, in the clouds' own order (ffb6d_icp_set_normals,
 * ffb6d_icp_estimate_normals_f32).
 *   Given normals: each is normalised once in double (n / sqrt(x*x + y*y + z*z)) and rounded to float32; a normal with a
 *     non-finite component or of zero length becomes the zero vector.
 *   Estimated normals: for model point j of class c take its k = min(16, n_c) nearest points of the class, itself included
 *     (the exact search and tie rule of include/ffb6d_knn.h, ffb6d_knn_batch_device on the class's rows).  With p_i those points
 *     in the order of the index row, in double from the float32 points: mean = (sum p_i) / k, C = sum (p_i - mean)(p_i - mean)^T.
 *     The normal is the singular vector of C's smallest singular value (the cyclic one-sided Jacobi of the rigid fit: rotate
 *     while |g_p . g_q| > 1.5 * 2^-52 |g_p| |g_q|; the first of equal values), normalised, with the sign that makes its
 *     component of largest magnitude positive (the lowest axis wins ties), rounded to float32.  It is the zero vector when
 *     n_c < 3 or the second singular value is zero (a point whose neighbours lie on a line or coincide).  The test is on
 *     the computed value: neighbours on an axis-aligned line give exact zeros, neighbours on an oblique line may leave a
 *     second value of rounding size (~2^-52 of the first), and the normal is then some unit vector across the line -- its
 *     pairs pull along a direction the data does not determine.  Callers with such models pass mesh normals instead.
 *   Class constants: c = the centre of the class's bounding box, rho = half its diagonal, in double from the float32 box
 *     (c_a = (lo_a + hi_a) / 2, rho = sqrt(ex*ex + ey*ey + ez*ez) / 2).  Scaling by rho makes the rotation and the
 *     translation columns of the system commensurate.
 *   Steps 1-3 are the ones above, with the same bits for idx and d2 (in the instance calls: the mode's step 3).
 *   4p. for every kept pair, in double from the float32 q (step 1), m = model[m(i)] and n = normal[m(i)]:
 *         u = (q - c) / rho,   a = [u x n, n] in R^6,   r = n . (q - m) / rho
 *       30 sums per block of 64 scene points, added in block order as in step 4 (no atomics): count, sum d2, sum r*r, the 21
 *       upper entries of sum a a^T row by row, the 6 of sum a r.  A zero normal gives a zero row and still counts as a pair.
 *   5p. M = sum a a^T, g = sum a r.  M is eigen-decomposed by cyclic two-sided Jacobi: the pair (p, q) is rotated while
 *       |M_pq| > 1.5 * 2^-52 sqrt(M_pp M_qq) (false for NaN), at most 30 sweeps.  With l_max the largest eigenvalue,
 *         x = - sum_k v_k (v_k . g) / l_k   over the k with l_k > 0 and l_k >= min_eig * l_max.
 *       The directions left out are not moved: a plane keeps its in-plane pose, a sphere its rotation, a can its spin.
 *       min_eig (0 <= min_eig < 1; 1e-6 in the Python calls) is a parameter of the method, not a tolerance of a test.
 *       w = x[0:3], v = x[3:6]; Rd = exp([w]x) = I + A [w]x + B [w]x^2 with A = sin(th)/th, B = (1 - cos(th))/th^2, th = |w|;
 *       below th = 1e-4, A = 1 - th^2/6 and B = 1/2 - th^2/24.  d = c - Rd c + rho v.   R <- R Rd^T, then t <- t - R_new d
 *       (the scene point in the model frame moves from q to Rd q + d).
 *       The problem ends with the pose it has when fewer than min_pairs pairs were kept, when rho = 0 (a class of one point or
 *       none) or when x is not finite.  The stop rule is step 5's: max_iter, min_pairs, tol on the box corners.
 *   Outputs as the point calls, and rms_plane f32 [P] = sqrt(rho^2 sum r*r / n) of the last iteration made, in metres, before
 *   that iteration's update (0 without pairs).  A *_plane call with max_iter = 0 returns the input bits.
 *   The point calls, their workspaces and their bits are what they were before the plane metric existed.
 *
 * All pointers are DEVICE pointers unless stated; the ffb6d_icp_correspond* and ffb6d_icp_refine* calls enqueue their work
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

/* The instance calls (the rule is stated at the top).  Arguments as the class calls, and:
 *   inst u8 [B,N] (NULL allowed in mode 1 only); inst_of i32 [P]; mode 0 = map, 1 = nearest;
 *   workspace of ffb6d_icp_inst_workspace_bytes(P, set_stride, mode) bytes (0 when P <= 0, set_stride <= 0 or mode is
 *   neither): the class calls' workspace, one i32 and one f32 row of set_stride per problem, and the groups.
 * ffb6d_icp_correspond_inst_f32, steps 1-3 once:
 *   idx as ffb6d_icp_correspond_f32 with the mode's step 3: -1 where the pair is not kept, in mode 1 also where p does not
 *   own the point;  d2 the problem's own smallest distance, owned or not;  counts the problem's scene points;
 *   owner i32 [P,set_stride]: the index of the owning problem, -1 when no member of the group has a non-NaN distance or j is
 *   beyond the count (all rows of a group agree; in mode 0 every problem is its own group).  Each may be NULL.
 * ffb6d_icp_refine_inst_f32, the loop: T, n_pairs, rms, iters as ffb6d_icp_refine_f32; inst_out u8 [B,N] or NULL.
 *   One launch for the scene sets, one for the groups, two per iteration in mode 0 and three in mode 1 (the distances of
 *   every problem, the owners and sums, the updates), one for inst_out.
 * Refused with their own messages: a mode outside {0, 1}, inst == NULL in mode 0, P > 65535. */
size_t ffb6d_icp_inst_workspace_bytes(int P, int64_t set_stride, int mode);
int ffb6d_icp_correspond_inst_f32(const void* prepared, int n_cls, int64_t total, const float* pcld, const void* mask,
                                  int mask_bits, const unsigned char* keep, const unsigned char* inst, const int* frame_of,
                                  const int* class_of, const int* inst_of, const double* T, int P, int B, int N,
                                  int64_t set_stride, float max_dist, int mode, int* idx, float* d2, int* counts, int* owner,
                                  void* workspace, size_t workspace_bytes, ffb6d_stream_t stream);
int ffb6d_icp_refine_inst_f32(const void* prepared, int n_cls, int64_t total, const float* pcld, const void* mask,
                              int mask_bits, const unsigned char* keep, const unsigned char* inst, const int* frame_of,
                              const int* class_of, const int* inst_of, const double* T0, int P, int B, int N,
                              int64_t set_stride, float max_dist, int max_iter, double tol, int min_pairs, int mode, double* T,
                              int* n_pairs, float* rms, int* iters, unsigned char* inst_out, void* workspace,
                              size_t workspace_bytes, ffb6d_stream_t stream);

/* ---- the point-to-plane metric (the rule is stated at the top) ----------------------------------------------------------
 * The normals buffer: ffb6d_icp_normals_bytes(total) bytes (0 when total < 0), float4 {nx, ny, nz, 0} per model point in
 * the clouds' own order (the rows of model_pts).  Made once per model set by one of:
 *   ffb6d_icp_set_normals: normals_in f32 [total,3] given by the caller (mesh vertex normals), validated, normalised and
 *     copied on `stream`; it does not wait.
 *   ffb6d_icp_estimate_normals_f32: estimated from the clouds alone (model_pts / model_begin as ffb6d_icp_prepare), one
 *     exact K = min(16, n_c) search and one launch of icp_normals_kernel per class.  It reads model_begin back, allocates
 *     its scratch and WAITS for `stream`, like ffb6d_icp_prepare.  total < 2^31. */
size_t ffb6d_icp_normals_bytes(int64_t total);
int ffb6d_icp_set_normals(const float* normals_in, int64_t total, void* normals, size_t normals_bytes, ffb6d_stream_t stream);
int ffb6d_icp_estimate_normals_f32(const float* model_pts, const int64_t* model_begin, int n_cls, int64_t total, void* normals,
                                   size_t normals_bytes, ffb6d_stream_t stream);

/* The loops under the plane metric: the arguments of ffb6d_icp_refine_f32 / ffb6d_icp_refine_inst_f32, and
 *   normals (the buffer above, after `prepared`), min_eig (after min_pairs), rms_plane f32 [P] or NULL (after rms);
 *   workspace of ffb6d_icp_plane_workspace_bytes(P, set_stride) / ffb6d_icp_plane_inst_workspace_bytes(P, set_stride, mode)
 *   bytes: the point calls' layout with 30 doubles per block of 64 scene points and one more row of state.
 * The same number of launches per iteration as the point calls; no wait, no read-back.
 * Refused with their own messages besides what the point calls refuse: normals == NULL, min_eig outside [0, 1). */
size_t ffb6d_icp_plane_workspace_bytes(int P, int64_t set_stride);
size_t ffb6d_icp_plane_inst_workspace_bytes(int P, int64_t set_stride, int mode);
int ffb6d_icp_refine_plane_f32(const void* prepared, const void* normals, int n_cls, int64_t total, const float* pcld,
                               const void* mask, int mask_bits, const unsigned char* keep, const int* frame_of,
                               const int* class_of, const double* T0, int P, int B, int N, int64_t set_stride, float max_dist,
                               int max_iter, double tol, int min_pairs, double min_eig, double* T, int* n_pairs, float* rms,
                               float* rms_plane, int* iters, void* workspace, size_t workspace_bytes, ffb6d_stream_t stream);
int ffb6d_icp_refine_plane_inst_f32(const void* prepared, const void* normals, int n_cls, int64_t total, const float* pcld,
                                    const void* mask, int mask_bits, const unsigned char* keep, const unsigned char* inst,
                                    const int* frame_of, const int* class_of, const int* inst_of, const double* T0, int P, int B,
                                    int N, int64_t set_stride, float max_dist, int max_iter, double tol, int min_pairs,
                                    double min_eig, int mode, double* T, int* n_pairs, float* rms, float* rms_plane, int* iters,
                                    unsigned char* inst_out, void* workspace, size_t workspace_bytes, ffb6d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
