/* include/ffb6d_eval.h -- C ABI of the gfx950 pose evaluation: the ADD / ADD-S distances that every
 * FFB6D accuracy number is built from.  Replaces, batched over every evaluated object of a batch:
 *
 *   Basic_Utils.cal_add_cuda / cal_adds_cuda   ffb6d/utils/basic_utils.py:651-669
 *   (called one object at a time by eval_metric / eval_metric_lm, pvn3d_eval_utils_kpls.py:162-196,287-305)
 *
 * All pointers are DEVICE pointers.  Return value: 0 or an FFB6D_ERR_* code (text through
 * ffb6d_last_error()); on an error nothing is written.
 */
#ifndef FFB6D_EVAL_H
#define FFB6D_EVAL_H

#include <stddef.h>
#include <stdint.h>

#include "ffb6d_knn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace for Q rows whose models have at most max_points points:
 *   36 * Q * max_points  (per point of a row: its ADD distance and the nearest squared distance found in each of the
 *   8 slices the predicted cloud is split into), 0 when Q <= 0 or max_points <= 0. */
size_t ffb6d_pose_add_adds_workspace_bytes(int Q, int64_t max_points);

/* ADD and ADD-S of Q (predicted pose, ground-truth pose) pairs.
 *   model_pts   f32 [total,3]   every class's model cloud, concatenated
 *   model_begin i64 [n_cls+1]   class c = rows model_begin[c] .. model_begin[c+1]-1
 *   class_of    i32 [Q]         class of each row, in [0, n_cls)
 *   pred_RT, gt_RT f32 [Q,3,4]  row-major [R|t]
 *   add, adds   f32 [Q]
 * For row q with model points p_0 .. p_{N-1}, in fp32 (the products and sums of R*p + t rounded one by one):
 *   pd_i = R_pred p_i + t_pred,  gt_i = R_gt p_i + t_gt
 *   add[q]  = mean_i |pd_i - gt_i|                 (basic_utils.py:651-657)
 *   adds[q] = mean_i min_j |pd_j - gt_i|           (:659-669: nearest predicted point of every ground-truth point)
 * Minima are taken over squared distances (one sqrtf per point at the end); each mean is summed in double in a fixed
 * order that depends on N alone and rounded once to f32, so a row's result does not depend on Q, on the other rows of
 * the call or on the run.  pd_i is computed identically for both, hence adds[q] <= add[q] exactly.  A class with
 * 0 points gives NaN (torch.mean of an empty tensor).
 * The call reads class_of and model_begin back to validate them and size the launch: it waits for the work queued
 * on `stream` before it (Q + n_cls + 1 words), then enqueues two kernels and returns without waiting for them. */
int ffb6d_pose_add_adds_f32(const float* model_pts, const int64_t* model_begin, int n_cls, const int* class_of,
                            const float* pred_RT, const float* gt_RT, int Q, float* add, float* adds,
                            void* workspace, size_t workspace_bytes, ffb6d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
