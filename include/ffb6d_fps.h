/* include/ffb6d_fps.h -- C ABI of batched farthest-point sampling (FPS) and per-set bounding-box statistics on gfx950: what
 * the reference's offline tool makes of a mesh (utils/dataset_tools/gen_obj_info.py:92-117 -- the FPS keypoints through
 * fps/src/farthest_point_sampling.cpp, the box corners, the centre and the radius, dataset_tools/utils.py:89-115) and what
 * pose.solve_poses, train_data.pose_targets, refine.PreparedModels and evaluate take as mesh_kps / mesh_ctr / r_lst / model
 * points.
 *
 * S point sets lie in the layout the library already uses (evaluate.ModelPoints pts / begin, render.PreparedMeshes verts /
 * vert_begin): pts f32 [total,3], begin i64 [S+1]; set s owns the rows begin[s] .. begin[s+1]-1, n_s of them.  The table is
 * clamped to [0, total] and a set is cut at max_n rows (the host sizes its launches by max_n and reads nothing back): no table
 * content makes a kernel read outside pts.  Coordinates must be FINITE: the kernels assume it (the host wrapper
 * ffb6d_amd/objinfo.py checks host data; a NaN never wins a comparison and gives unspecified but in-range indices).
 *
 * The rule is the reference's (farthest_point_sampling.cpp:41-160), quirks included; "float" is IEEE binary32 and every
 * product and sum is rounded on its own (the library is built with -ffp-contract=off, as the reference's is by default on
 * x86-64):
 *     d(i, c) = (dx*dx + dy*dy) + dz*dz   with dx = x_i - x_c, dy = y_i - y_c, dz = z_i - z_c
 *   min_dist[i] starts at FLT_MAX.  After a point c is picked it is masked, and every unmasked i takes
 *     min_dist[i] = min(min_dist[i], d(i, c)).
 *   The next pick is the unmasked point with the largest min_dist, the lowest index on ties, provided that value is > 0;
 *   otherwise the pick is index 0 -- even when 0 is masked already (find_max_dist_idx, :56-73: max_idx = 0, max_d = 0.f).
 *   That is what happens once only duplicates of picked points are left, or once m > n_s.
 *   (With finite coordinates d(c, c) = 0, so "masked" and "min_dist == 0" select the same points: the kernels keep no mask.)
 *   Two start modes:
 *     start i32 [S]: the first pick of set s is start[s], clamped to [0, n_s - 1] (sample_farthest_points, :77-105, with
 *       its clock-seeded `rand() % n` handed in by the caller); out_dist of that first pick is FLT_MAX.
 *     start == NULL: the reference's init_center mode (:122-160).  centre = (max + min) * 0.5f per axis over the set,
 *       min_dist[i] starts as min(d(i, centre), FLT_MAX), and the first pick comes from the rule above.
 *   An empty set gives idx = -1 and out_pts = out_dist = 0 in its row.
 * Outputs, each may be NULL but not all of them:
 *   idx i32 [S,m]: indices WITHIN the set;  out_pts f32 [S,m,3]: the picked points;
 *   out_dist f32 [S,m]: the value the pick was chosen by -- its minimum squared distance to the earlier picks (to the box
 *   centre for the first pick of the init_center mode) at the moment it is chosen; 0 when the pick is the index-0 fallback
 *   (the point then coincides with an earlier pick), FLT_MAX for a given first pick.
 *
 * Two forms, identical bits (ffb6d_fps_set_form):
 *   resident: one workgroup of 1024 threads per set; the set's coordinates and min_dist live in registers, up to 8 points
 *     per lane, so n_s <= ffb6d_fps_resident_capacity() = 8192.  No workspace.
 *   streaming: one workgroup per set; coordinates are read from pts in every step and min_dist lives in the workspace
 *     (f32 [S,max_n]).  Any n_s.
 *   A step is a distance update, a 64-bit arg-max key per lane (float bits of min_dist << 32 | ~index; zero distances give
 *   key 0, so the maximum is the largest distance at the lowest index), a reduction over the wave's lanes (DPP row rotations,
 *   then across rows), the winning lane's key and xyz written to a parity-double-buffered LDS slot per wave, ONE barrier, and
 *   a reduction of the 16 slots by every wave on its own: the next centre is known without a second barrier or a trip
 *   through global memory.
 *   A set is owned by one workgroup from start to end: no form waits on another workgroup (no grid-wide barrier, no flag,
 *   no cooperative launch).  One huge set with a small m therefore runs on a single compute unit; splitting a set over
 *   workgroups is out of scope.
 *
 * All pointers are DEVICE pointers; the calls enqueue their work on `stream` and return without waiting for it or reading
 * anything back.  Return value: 0 or an FFB6D_ERR_* code (text through ffb6d_last_error()); on an error nothing is launched
 * and no output is written.
 */
#ifndef FFB6D_FPS_H
#define FFB6D_FPS_H

#include <stddef.h>
#include <stdint.h>

#include "ffb6d_knn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Points of a set that the resident form holds (a compile-time constant of the library). */
int ffb6d_fps_resident_capacity(void);

/* 0 (default) = automatic: resident when max_n <= the capacity, streaming above it; 1 = resident (max_n above the capacity is
 * refused); 2 = streaming.  Identical results. */
void ffb6d_fps_set_form(int form);

/* Bytes of workspace of ffb6d_fps_f32 under the current form setting: 0 for the resident form and for sizes the call refuses,
 * min_dist f32 [S,max_n] rounded up to 256 bytes for the streaming form. */
size_t ffb6d_fps_workspace_bytes(int S, int64_t max_n, int m);

/* S >= 1 sets, m >= 1 samples per set; 0 <= max_n < 2^31: the largest n_s (larger sets are cut there); total >= 0 rows in pts
 * (pts may be NULL when total == 0).  workspace may be NULL when ffb6d_fps_workspace_bytes is 0. */
int ffb6d_fps_f32(const float* pts, const int64_t* begin, int S, int64_t total, int64_t max_n, int m, const int* start,
                  int* idx, float* out_pts, float* out_dist, void* workspace, size_t workspace_bytes, ffb6d_stream_t stream);

/* Box statistics of every set in one launch (dataset_tools/utils.py:89-115); each output may be NULL but not all of them:
 *   corners f32 [S,8,3]: corner k = (x: max if k & 4 else min, y: max if k & 2 else min, z: max if k & 1 else min), the order
 *     of get_3D_bbox (:93-102);
 *   ctr f32 [S,3] = (max + min) * 0.5f per axis (get_centers_3d, :113-115);
 *   radius f32 [S] = 0.5f * sqrtf((dx*dx + dy*dy) + dz*dz), d = max - min in float (get_r, :109-110).
 * An empty set gives zeros.  Sets are not cut: there is no max_n. */
int ffb6d_box_info_f32(const float* pts, const int64_t* begin, int S, int64_t total, float* corners, float* ctr, float* radius,
                       ffb6d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
