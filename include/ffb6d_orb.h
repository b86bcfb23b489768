/* include/ffb6d_orb.h -- C ABI of the texture-aware object keypoints on gfx950: a 2-D corner detector on rendered frames, the
 * lift of its pixels through the rendered depth into the object frame, and the compaction of the lifted points into point
 * sets that ffb6d_fps_f32 samples.  This is the chain of the reference's offline tool (gen_obj_info.py:119-125,
 * rgbd_rnder_sift_kp3ds.py:38-166: render a few views, cv2.ORB_create().detectAndCompute, depth -> object frame, FPS) whose
 * result Basic_Utils.get_kps reads when use_orbfps is set (common.py:71-73,129-131), the reference's default.
 *
 * The detector is the published ORB *detector* -- FAST-9 corners on a 1.2x scale pyramid, ranked by a Harris response, with a
 * quota per level -- stated below in integers only.  It is NOT OpenCV's implementation and does not reproduce cv2.ORB's
 * keypoints bit for bit (OpenCV's pyramid interpolation, its FAST score threshold search and its float Harris response are
 * not restated); orientation and descriptors are not built, the reference uses kp.pt alone.  tests/orb_ref.py restates the
 * rule in numpy and every implementation is held to it bit for bit.
 *
 * THE RULE.  Input rgb u8 [F,3,H,W] (the layout ffb6d_render_f32 writes).  Parameters: n_levels L in 1 .. 8, the FAST
 * threshold t, edge >= 4, quota i32 [L] >= 0.  All arithmetic is integer; "//" is the floor quotient of non-negative integers.
 *   Gray.        g = (4899*R + 9617*G + 1868*B + 8192) >> 14.
 *   Level sizes. W_l = (2*W*5^l + 6^l) // (2*6^l), H_l likewise: W / 1.2^l rounded half up.  A level with W_l or H_l below
 *                2*edge + 1 holds no keypoints.
 *   Resize.      Level l is made from level l-1 (gray p), bilinear, centre-aligned, 11-bit weights.  For a destination x:
 *                  num = (2x+1)*W_{l-1} - W_l, den = 2*W_l, x0 = num // den, fx = ((num - x0*den)*2048) // den,
 *                  x1 = min(x0+1, W_{l-1}-1); the same in y.  With p00 = p(x0,y0), p01 = p(x1,y0), p10 = p(x0,y1), p11 = p(x1,y1):
 *                  v = ((2048-fy)*((2048-fx)*p00 + fx*p01) + fy*((2048-fx)*p10 + fx*p11) + 2^21) >> 22.
 *   FAST-9.      The 16 pixels c_i of the radius-3 circle, clockwise from c_0 = (0,-3) with y pointing down:
 *                  (0,-3) (1,-3) (2,-2) (3,-1) (3,0) (3,1) (2,2) (1,3) (0,3) (-1,3) (-2,2) (-3,1) (-3,0) (-3,-1) (-2,-2) (-1,-3).
 *                At a pixel p with d_i = g(p + c_i) - g(p), indices mod 16:
 *                  score = max(0, max_k min_{i=k..k+8} d_i, max_k min_{i=k..k+8} (-d_i)).
 *   Candidates.  A pixel with edge <= x < W_l - edge and edge <= y < H_l - edge whose score is > t and strictly greater than
 *                the score of each of its 8 neighbours.
 *   Harris.      With the 3x3 Sobel derivatives of the level's gray image,
 *                  Ix(x,y) = (g(x+1,y-1) + 2*g(x+1,y) + g(x+1,y+1)) - (g(x-1,y-1) + 2*g(x-1,y) + g(x-1,y+1)),
 *                  Iy(x,y) = (g(x-1,y+1) + 2*g(x,y+1) + g(x+1,y+1)) - (g(x-1,y-1) + 2*g(x,y-1) + g(x+1,y-1)),
 *                summed over the 7x7 block around the candidate: a = sum Ix^2, b = sum Iy^2, c = sum Ix*Iy, and
 *                  resp = 25*(a*b - c*c) - (a+b)^2   in int64 (k = 0.04 made exact; |resp| < 2^57).
 *   Selection.   Per (frame, level) the quota[l] candidates with the largest resp are kept; of equal responses the one with
 *                the smaller pixel index y*W_l + x comes first.  A frame's keypoints are listed by level, then by that rank.
 *   Level-0 pixel of a keypoint: X = ((2x+1)*W) // (2*W_l), Y = ((2y+1)*H) // (2*H_l): the identity at level 0.
 *   Quotas are made by the caller (ffb6d_amd/objinfo.py orb_quotas, in double as ORB does): f = 1/1.2,
 *                n = n_features*(1-f)/(1-f^L); quota[l] = round-half-even(n), n *= f, for l < L-1; the last level takes
 *                max(n_features - sum, 0).
 * Outputs, with Q = sum quota:  count i32 [F];  kps i32 [F,Q,5] rows (x_l, y_l, level, X, Y);  resp i64 [F,Q].  Rows past
 * count[f] hold -1 (kps) and 0 (resp).
 *
 * No capacity drops a candidate: strict 8-neighbour maxima are never adjacent, so a level holds at most
 * ceil(H_l/2)*ceil(W_l/2) of them, and the candidate lists in the workspace are sized by that bound.  Candidates are
 * appended in arbitrary order; the output order comes from the rank alone, so every run gives the same bytes.
 *
 * THE LIFT (rgbd_rnder_sift_kp3ds.py:80,112-128, dataset_tools/utils.py:143-167,194-204).  Row r < count[f] of a frame whose
 * instance owns at least min_pixels pixels (visible[f], from ffb6d_render_f32) reads z = depth[f,Y,X] and is dropped unless z
 * is finite and z > 1e-8f.  In float, each operation rounded on its own (the library is built with -ffp-contract=off):
 *     px = (((float)X - cx) * z) / fx,  py = (((float)Y - cy) * z) / fy,  pz = z.
 * In double, with the frame's pose T[f] = [R|t] (row-major [3,4], object -> camera) and d = (double)p - t:
 *     o_j = (d_0*R_0j + d_1*R_1j) + d_2*R_2j,   j = 0 .. 2,   rounded once to float:   (p - t) . R of the reference.
 * ffb6d_orb_lift_f32 writes slot_pts f32 [F,Q,3] and slot_ok i32 [F,Q] (zeros for a dropped row): frames can be lifted in
 * chunks while their depth is at hand.  ffb6d_orb_compact_f32 then packs the kept points of all frames, V frames per object
 * (object s owns the frames s*V .. s*V+V-1), in (frame, row) order: pts f32 [S*V*Q,3] (rows past the last point are zero),
 * begin i64 [S+1], n_found i32 [S] -- the layout ffb6d_fps_f32 takes, with max_n = V*Q known to the host.
 *
 * All pointers are DEVICE pointers but `quota`, which is read on the host when the call is made.  The calls enqueue their work
 * on `stream` and return without waiting for it or reading anything back.  Return value: 0 or an FFB6D_ERR_* code (text
 * through ffb6d_last_error()); on an error nothing is launched and no output is written.
 */
#ifndef FFB6D_ORB_H
#define FFB6D_ORB_H

#include <stddef.h>
#include <stdint.h>

#include "ffb6d_knn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FFB6D_ORB_MAX_LEVELS 8

/* Bytes of workspace of ffb6d_orb_detect_u8 (0 for sizes the call refuses): the gray pyramid u8 [F,H_l,W_l] per level, the
 * candidate counters i32 [F,L], and the candidate lists resp i64 / pixel i32 of ceil(H_l/2)*ceil(W_l/2) entries per
 * (frame, level); every part rounded up to 256 bytes. */
size_t ffb6d_orb_workspace_bytes(int F, int H, int W, int n_levels);

/* 1 <= F <= 65535, 4 <= H, W <= 16384, F*H*W < 2^31, 1 <= n_levels <= 8, 0 <= fast_threshold <= 255, 4 <= edge <= 4096,
 * quota (HOST) i32 [n_levels] >= 0 with 1 <= Q = sum quota and F*Q < 2^27. */
int ffb6d_orb_detect_u8(const unsigned char* rgb, int F, int H, int W, int n_levels, int fast_threshold, int edge,
                        const int* quota, int* count, int* kps, int64_t* resp, void* workspace, size_t workspace_bytes,
                        ffb6d_stream_t stream);

/* kps i32 [F,Q,5], count i32 [F] as ffb6d_orb_detect_u8 writes them; depth f32 [F,H,W]; visible i32 [F]; T f64 [F,3,4];
 * fx, fy, cx, cy: the intrinsics of every frame, in float.  A row whose (X, Y) lies outside the frame is dropped. */
int ffb6d_orb_lift_f32(const int* kps, const int* count, const float* depth, const int* visible, const double* T, int F, int Q,
                       int H, int W, float fx, float fy, float cx, float cy, int min_pixels, float* slot_pts, int* slot_ok,
                       ffb6d_stream_t stream);

/* slot_pts f32 [S*V,Q,3], slot_ok i32 [S*V,Q] -> pts f32 [S*V*Q,3], begin i64 [S+1], n_found i32 [S].  S, V, Q >= 1,
 * S*V*Q < 2^31. */
int ffb6d_orb_compact_f32(const float* slot_pts, const int* slot_ok, int S, int V, int Q, float* pts, int64_t* begin,
                          int* n_found, ffb6d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
