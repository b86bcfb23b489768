/* include/ffb6d_bop.h -- C ABI of the gfx950 BOP pose errors: MSSD and MSPD (maximum symmetry-aware surface / projection
 * distance) and VSD (visible surface discrepancy), the three error functions the 6D-pose field ranks methods by, next to the
 * ADD / ADD-S of include/ffb6d_eval.h.  The reference evaluates ADD(-S) only and there is no BOP toolkit to port: the
 * arithmetic is stated here in full and restated in numpy by tests/bop_ref.py, which the kernels are held against bit for bit.
 *
 * Every product, sum and quotient below is rounded on its own, in the order written (the library is built with
 * -ffp-contract=off); "double" is IEEE binary64, "float" binary32.
 *
 * Inputs shared by the calls
 *   model_pts f32 [total,3], model_begin i64 [n_cls+1]   the layout of ffb6d_eval.h (BOP scores the mesh vertices); class c owns
 *                                                        the rows model_begin[c] .. model_begin[c+1]-1
 *   sym_R f64 [Stot,3,3], sym_t f64 [Stot,3], sym_begin i64 [n_cls+1]   the symmetry transforms of every class, concatenated;
 *                                                        a class with no entries is scored with the identity alone (R = I, t = 0)
 *   class_of, frame_of i32 [Q];  est_T, gt_T f64 [Q,3,4]  model -> camera, row-major [R|t], the renderer's convention
 *   K f64 [B,3,3]                                         only fx = K[0], fy = K[4], cx = K[2], cy = K[5] are read
 * The tables are clamped to [0, total] / [0, Stot] and a class's counts to max_points / max_syms: no table content makes a kernel
 * read outside its arrays.  The host passes max_points and max_syms (the largest count of a class) to size the launches;
 * points and symmetries of a class beyond them are not scored.
 *
 * ffb6d_bop_mssd_mspd_f64 -> mssd2 f64 [Q], mspd2 f64 [Q]: the SQUARED errors (the kernels take no square root).
 *   For row q, point p = (x, y, z) of its class widened to double, symmetry s = (Rs, ts), est_T = [Re|te], gt_T = [Rg|tg]:
 *     Xe = ((Re00*x + Re01*y) + Re02*z) + te0, likewise Ye (row 1) and Ze (row 2)
 *     Rg'[i][j] = ((Rg[i][0]*Rs[0][j] + Rg[i][1]*Rs[1][j]) + Rg[i][2]*Rs[2][j])
 *     tg'[i]    = (((Rg[i][0]*ts[0] + Rg[i][1]*ts[1]) + Rg[i][2]*ts[2]) + tg[i])
 *     (Xg, Yg, Zg) from Rg', tg' in the order of the estimated point
 *   MSSD:  dx = Xe - Xg, dy = Ye - Yg, dz = Ze - Zg;  d2 = ((dx*dx + dy*dy) + dz*dz);  m_s = max_i d2;  mssd2[q] = min_s m_s
 *   MSPD:  u = (fx*X)/Z + cx, v = (fy*Y)/Z + cy (the renderer's formula) under both poses; du = ue - ug, dv = ve - vg;
 *          d2 = du*du + dv*dv; a point with !(Z > 0) under either pose makes d2 = +inf;  mspd2[q] = min_s max_i d2
 *   A d2 that is NaN (overflow, or a table that holds values that are not finite) counts as +inf.  Max and min are then
 *   order-independent: any reduction shape gives the same bits, and a row's result does not depend on Q or on the other rows.
 *   Rows that give NaN in both outputs, with nothing read through the bad index: a row whose class has 0 points, whose class id
 *   is outside [0, n_cls) or frame id outside [0, B), or whose 24 pose entries are not all finite.
 *
 * ffb6d_bop_vsd_f32 -> counts i32 [Q, 2+n_tau], vsd f64 [Q, n_tau]: the "bop19" visibility rule with the step cost, the
 * depth difference normalised by the object's diameter.
 *   depth_test f32 [B,H,W] metres; a value that is not finite or is <= 0 counts as 0 (no measurement)
 *   depth_est, depth_gt f32 [Q,H,W]  row q's model rendered ALONE under est_T[q] / gt_T[q]; 0 = nothing drawn
 *   diameter f32 [n_cls];  delta (metres);  taus f32 [n_tau], fractions of the diameter, 1 <= n_tau <= FFB6D_BOP_MAX_TAUS
 *   Per pixel (r, c) of row q, b = frame_of[q], all in float, fxf = (float)K[b][0], fyf = (float)K[b][4], cxf = (float)K[b][2],
 *   cyf = (float)K[b][5]:
 *     dist(z) = 0 if z == 0, else X = (((float)c - cxf) * z) / fxf, Y = (((float)r - cyf) * z) / fyf,
 *               dist = sqrt((X*X + Y*Y) + z*z)          (correctly rounded division and square root)
 *     dt, de, dg = dist of the test, est and gt pixel
 *     vis_gt  = dg > 0 && (dt == 0 || dg - dt <= delta)
 *     vis_est = de > 0 && (dt == 0 || de - dt <= delta || vis_gt)
 *     union = vis_gt || vis_est, inter = vis_gt && vis_est
 *     on inter pixels: e = fabsf(dg - de) / diameter[class], cost_k += (e >= taus[k])
 *   counts[q] = [n_union, n_inter, cost_0, ...]
 *   vsd[q,k] = 1.0 if n_union == 0, else (double)(cost_k + (n_union - n_inter)) / (double)n_union
 *   A row whose class id is outside [0, n_cls) or frame id outside [0, B) gives counts of 0 and a vsd of NaN; nothing is read
 *   through the bad index.  Integer sums: exact whatever the reduction shape.
 *
 * All pointers are DEVICE pointers; a call enqueues its work on `stream` and returns without waiting for it or reading anything
 * back.  Return value: 0 or an FFB6D_ERR_* code (text through ffb6d_last_error()); on an error nothing is launched and no output
 * is written.
 */
#ifndef FFB6D_BOP_H
#define FFB6D_BOP_H

#include <stddef.h>
#include <stdint.h>

#include "ffb6d_knn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FFB6D_BOP_MAX_TAUS 16

/* Bytes of workspace of ffb6d_bop_mssd_mspd_f64: per row, per symmetry (max(max_syms, 1) rounded up to the symmetry block of 8)
 * and per chunk of 1024 points, the two running maxima as doubles; rounded up to 256 bytes.  0 for sizes the call refuses, for
 * Q = 0 and for max_points = 0 (which the call takes: every row is NaN and no workspace is needed). */
size_t ffb6d_bop_mssd_mspd_workspace_bytes(int Q, int64_t max_points, int64_t max_syms);

/* mssd2, mspd2: either may be NULL but not both (K and frame_of are still needed: a bad frame id makes the row NaN).
 * 0 <= Q <= 65535 (Q = 0: nothing to do; a grid dimension: ffb6d_amd/bop.py splits larger batches), n_cls > 0, B > 0,
 * 0 <= max_points <= total, max_points < 2^31 - 1024, 0 <= max_syms <= Stot, max_syms <= 8 * 65535.
 * Two launches: (row, symmetry block, point chunk) workgroups write per-symmetry maxima into the workspace, which may hold
 * anything on entry; one wavefront per row takes the max over the chunks and the min over the symmetries. */
int ffb6d_bop_mssd_mspd_f64(const float* model_pts, const int64_t* model_begin, int n_cls, int64_t total, int64_t max_points,
                            const double* sym_R, const double* sym_t, const int64_t* sym_begin, int64_t Stot, int64_t max_syms,
                            const int* class_of, const int* frame_of, const double* est_T, const double* gt_T, int Q,
                            const double* K, int B, double* mssd2, double* mspd2, void* workspace, size_t workspace_bytes,
                            ffb6d_stream_t stream);

/* Bytes of workspace of ffb6d_bop_vsd_f32 (0 for sizes the call refuses): per row and per run of 4096 pixels, 2 + 16 integer
 * partial counts; rounded up to 256 bytes. */
size_t ffb6d_bop_vsd_workspace_bytes(int Q, int H, int W);

/* 0 <= Q <= 65535 (Q = 0: nothing to do), H, W > 0, H*W < 2^31 - 4096; counts and vsd are both written.
 * Two launches: a streaming pass over the three images (16-byte accesses where H*W is a multiple of 4 and the images are 16-byte
 * aligned, single floats otherwise and for the tail) writes per-workgroup partial counts into the workspace, which may hold
 * anything on entry; one wavefront per row adds them and writes counts and vsd. */
int ffb6d_bop_vsd_f32(const float* depth_test, const float* depth_est, const float* depth_gt, const int* class_of,
                      const int* frame_of, int Q, const double* K, int B, int H, int W, const float* diameter, int n_cls,
                      float delta, const float* taus, int n_tau, int* counts, double* vsd, void* workspace,
                      size_t workspace_bytes, ffb6d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
