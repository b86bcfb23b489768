/* include/ffb6d_train.h -- C ABI of the gfx950 training-sample arithmetic: what the training half of the reference's
 * Dataset.get_item computes per frame on the CPU, batched on the device.
 *
 *   ffb6d_pose_targets        get_pose_gt_info + labels_pt   ycb_dataset.py:240,348-386, linemod_dataset.py:287,398-436
 *   ffb6d_pose_targets_inst   the same per instance: several instances of one class in a frame (no counterpart in the reference)
 *   ffb6d_rgb_hsv_jitter      rgb_add_noise, HSV stage      ycb_dataset.py:110-116, linemod_dataset.py:145-151
 *   ffb6d_rgb_stencil         rgb_add_noise, filter2D / GaussianBlur stages and the Gaussian noise
 *                                                             ycb_dataset.py:82-143, linemod_dataset.py:117-164
 *   ffb6d_add_real_back       add_real_back                  ycb_dataset.py:145-163, linemod_dataset.py:166-186
 *   ffb6d_color_jitter_u8     self.trancolor (ColorJitter)   ycb_dataset.py:34,190-193, linemod_dataset.py:35,221-223
 *
 * All pointers are DEVICE pointers.  Return value: 0 or an FFB6D_ERR_* code (text through ffb6d_last_error()); on an
 * error nothing is written.  No call reads anything back or waits: each enqueues one kernel on `stream` (ffb6d_color_jitter_u8: two).
 * OpenCV is not available where this library is built: the HSV and filter arithmetic below restates OpenCV's published
 * 8-bit algorithms (color_hsv.simd.hpp, filter.simd.hpp, drawing.cpp) and is pinned against those restatements only.
 */
#ifndef FFB6D_TRAIN_H
#define FFB6D_TRAIN_H

#include <stddef.h>
#include <stdint.h>

#include "ffb6d_knn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Pose targets of B frames with N sampled points, O object slots and K keypoints.
 *   cld        f32 [B,N,3]             sampled points (metres)
 *   choose     [B,N]  i32 or i64       (choose_i64 = 0 / 1) pixel indices into the HxW label image, HW = H*W
 *   label_img  [B,HW] u8 or i32        (label_u8 = 1 / 0)
 *   cls_ids    i32 [B,O]               class id per object slot; 0 = empty slot
 *   RTs        [B,O,3,4] f32 or f64    (rts_f64 = 0 / 1) row-major [R|t]
 *   mesh_kps   f32 [n_cls,K,3], mesh_ctr f32 [n_cls,3]   model-frame keypoints / centre indexed by class id
 * Outputs:
 *   labels     i32 [B,N]        = label_img[b, choose[b,n]]                               (ycb :240, linemod :287)
 *   kp_targ_ofst  f32 [B,N,K,3], ctr_targ_ofst f32 [B,N,3]
 *   kp_3ds     f32 [B,O,K,3], ctr_3ds f32 [B,O,3], RTs_out f32 [B,O,3,4], cls_ids_out i32 [B,O,1]
 * Formulas, in double as the reference computes them (float32 mesh points times float64 r.T; ycb :362,378, linemod :411,427):
 *   kp3d[o,k,j]  = ((m[k,0]*r[j,0] + m[k,1]*r[j,1]) + m[k,2]*r[j,2]) + t[j]      m = mesh_kps[cls], r, t of RTs[b,o]
 *   ctr3d[o,j]   = the same with m = mesh_ctr[cls]
 *   point n with label l >= 1 takes the LAST slot o whose class is l (later objects overwrite earlier ones, ycb :385);
 *   kp_targ_ofst[b,n,k,j] = (float)((double)cld[b,n,j] - kp3d[o,k,j])   POINT MINUS KEYPOINT (np.add(cld, -1.0*kp), :383)
 *   ctr_targ_ofst[b,n,j]  = (float)((double)cld[b,n,j] - ctr3d[o,j])      (:366)
 *   points whose label matches no slot, and label-0 points, get zeros.
 *   kp_3ds / ctr_3ds = (float)kp3d / (float)ctr3d, RTs_out = (float)RTs, cls_ids_out = cls_ids for the used slots.
 * A slot whose class id lies outside [1, n_cls) -- 0 included -- is empty: its rows are all zero and it matches no point.
 * Class ids are therefore never used to index out of bounds, whatever the device memory holds; the Python wrapper rejects
 * host-side ids outside [0, n_cls) before launching.  A choose index outside [0, HW) reads label 0.
 * Limits: 1 <= K <= 64, 1 <= O <= 64, O * (K + 1) <= 1024. */
int ffb6d_pose_targets(const float* cld, const void* choose, int choose_i64, const void* label_img, int label_u8,
                       const int* cls_ids, const void* RTs, int rts_f64, const float* mesh_kps, const float* mesh_ctr,
                       int n_cls, int B, int64_t N, int64_t HW, int O, int K, int* labels, float* kp_targ_ofst,
                       float* ctr_targ_ofst, float* kp_3ds, float* ctr_3ds, float* RTs_out, int* cls_ids_out,
                       ffb6d_stream_t stream);

/* Pose targets per INSTANCE: B frames with N sampled points, I instances over the whole batch (the renderer's own list:
 * ffb6d_render.h's frame_of / class_of / poses and its `inst` image) and K keypoints.  Where ffb6d_pose_targets finds a point's
 * object through its class label -- so that two instances of one class in a frame both get the LAST slot's keypoints -- this call
 * finds it through the instance image, and every instance keeps its own.
 *   cld        f32 [B,N,3]             sampled points (metres)
 *   choose     [B,N]  i32 or i64       (choose_i64 = 0 / 1) pixel indices into the HxW instance image, HW = H*W
 *   inst_img   i32 [B,HW]              global instance index per pixel, negative = none
 *   frame_of   i32 [I], class_of i32 [I]   frame and class of each instance
 *   poses      f64 [I,3,4]             row-major [R|t] of each instance
 *   mesh_kps   f32 [n_cls,K,3], mesh_ctr f32 [n_cls,3]   model-frame keypoints / centre indexed by class id
 * Outputs:
 *   labels     i32 [B,N], inst_of_point i32 [B,N]        class and global instance index per point (0 and -1 = none)
 *   kp_targ_ofst  f32 [B,N,K,3], ctr_targ_ofst f32 [B,N,3]
 *   kp_3ds     f32 [I,K,3], ctr_3ds f32 [I,3]            posed keypoints / centre per instance
 *   n_points   i32 [I]                                   sampled points owned by each instance
 * The rule:
 *   instance i EXISTS iff 0 <= frame_of[i] < B and 1 <= class_of[i] < n_cls;
 *   i = inst_img[b, choose[b,n]], none when the choose index lies outside [0, HW);
 *   point n of frame b BELONGS to instance i iff 0 <= i < I, i exists and frame_of[i] == b (an index painted into another
 *     frame's image than the instance's own owns nothing there);
 *   a point that belongs:  labels = class_of[i], inst_of_point = i,
 *     kp_targ_ofst[b,n,k,j] = (float)((double)cld[b,n,j] - kp3d[i,k,j])     POINT MINUS KEYPOINT, as ffb6d_pose_targets
 *     ctr_targ_ofst[b,n,j]  = (float)((double)cld[b,n,j] - ctr3d[i,j])
 *   any other point:  labels = 0, inst_of_point = -1, offsets all zero;
 *   kp3d[i,k,j]  = ((m[k,0]*r[j,0] + m[k,1]*r[j,1]) + m[k,2]*r[j,2]) + t[j]   in double, m = mesh_kps[class_of[i]], r, t of poses[i]:
 *   ctr3d[i,j]   = the same with m = mesh_ctr[class_of[i]]: exactly the formula of ffb6d_pose_targets, the same operations in the
 *     same order with no contraction, so that with at most one instance per class and frame both calls give the same bits;
 *   kp_3ds / ctr_3ds = (float)kp3d / (float)ctr3d; an instance that does not exist has zero rows and owns no point;
 *   n_points[i] = the number of points that belong to i: an integer count, exact in whatever order it is added up; the call
 *     zeroes it itself.
 * Frame, class, instance and choose values are compared before they index anything: nothing is ever read or written through a bad
 * id, whatever the device memory holds.  The Python wrapper rejects host-side ids out of range before launching.
 * Two launches on `stream` (the instances' rows, then the points; one when I = 0 or there are no points), no read-back, no wait.
 * The workspace (ffb6d_pose_targets_inst_workspace_bytes: the double rows of all instances, 0 for I = 0) may hold anything on entry.
 * Limits: 1 <= K <= 64, 0 <= I <= 1024.  FFB6D_ERR_ARG, with nothing launched or written: negative sizes, n_cls < 1, K or I outside
 * the limits, a null pointer that would be used, B > 65535; FFB6D_ERR_WORKSPACE: a workspace below the query, or not 8-byte aligned. */
size_t ffb6d_pose_targets_inst_workspace_bytes(int I, int K);
int ffb6d_pose_targets_inst(const float* cld, const void* choose, int choose_i64, const int* inst_img, const int* frame_of,
                            const int* class_of, const double* poses, const float* mesh_kps, const float* mesh_ctr, int n_cls,
                            int B, int64_t N, int64_t HW, int I, int K, int* labels, int* inst_of_point, float* kp_targ_ofst,
                            float* ctr_targ_ofst, float* kp_3ds, float* ctr_3ds, int* n_points, void* workspace,
                            size_t workspace_bytes, ffb6d_stream_t stream);

/* HSV jitter of B uint8 images [B,3,H,W] (plane 0 plays OpenCV's "B": the reference hands an RGB array to
 * COLOR_BGR2HSV / COLOR_HSV2BGR, ycb :111,116).  fs_fv f64 [B,2]; a frame with fs_fv[b,0] < 0 is copied unchanged.
 *   forward (8-bit RGB2HSV_b, hsv_shift = 12, hrange = 180):
 *     v = max(b,g,r), vmin = min(b,g,r), diff = v - vmin
 *     sdiv[x] = x ? cvRound((255 << 12) / (double)x) : 0,  hdiv[x] = x ? cvRound((180 << 12) / (6.0 x)) : 0
 *     s = (diff * sdiv[v] + (1 << 11)) >> 12
 *     h = v == r ? g - b : v == g ? b - r + 2 diff : r - g + 4 diff;  h = (h * hdiv[diff] + (1 << 11)) >> 12;  h += h < 0 ? 180 : 0
 *   jitter (ycb :112-115; the uint16 array is assigned a float64 product, which truncates):
 *     s' = min(255, floor(s * fs)), v' = min(255, floor(v * fv))
 *   back (8-bit HSV2RGB_b, float path, float32): H = h * (6.f/180) wrapped into [0,6), S = s' * (1.f/255), V = v' * (1.f/255)
 *     sector = floor(H), f = H - sector;  tab = {V, V(1-S), V(1-S f), V(1-S(1-f))}
 *     (b,g,r) = tab[{1,3,0},{1,0,2},{3,0,1},{0,2,1},{0,1,3},{2,1,0}][sector]  (S == 0: b = g = r = V)
 *     out = saturate(cvRound(x * 255.f))   (round half to even) */
int ffb6d_rgb_hsv_jitter(const uint8_t* in, const double* fs_fv, uint8_t* out, int B, int64_t H, int64_t W,
                         ffb6d_stream_t stream);

#define FFB6D_STENCIL_MAX_TAPS 32
#define FFB6D_STENCIL_MAX_HALO 15

/* One frame's stencil pass (host-built, uploaded as an array of B). */
typedef struct {
    int32_t n_taps;                       /* 0: no filter (copy); at most FFB6D_STENCIL_MAX_TAPS */
    int32_t halo;                         /* max |dy|, |dx| over the taps, at most FFB6D_STENCIL_MAX_HALO */
    float sigma;                          /* > 0: Gaussian noise sigma (0 = none) */
    float extra_sigma;                    /* > 0: a further N(0, extra_sigma^2) (YCB: 7) */
    int32_t dy[FFB6D_STENCIL_MAX_TAPS];   /* tap offsets relative to the output pixel (row, column) */
    int32_t dx[FFB6D_STENCIL_MAX_TAPS];
    float w[FFB6D_STENCIL_MAX_TAPS];      /* tap weights */
} ffb6d_stencil_frame_t;

/* One batched filter pass over uint8 [B,3,H,W] with per-frame taps, Gaussian noise fused after the filter.
 *   filter (filter2D / GaussianBlur on 8-bit, BORDER_REFLECT_101; correlation, anchor folded into dy / dx):
 *     acc = sum over taps in list order of w * in[reflect101(y + dy), reflect101(x + dx)]   (float32, no FMA)
 *     v = saturate(cvRound(acc))                                   (n_taps = 0: v = in[y,x])
 *   noise (gaussian_noise, ycb :82-86, then :140-143; both casts to uint8 truncate):
 *     sigma > 0:        v = (uint8) clamp(v + sigma * n1, 0, 255)
 *     extra_sigma > 0:  v = (uint8) clamp(v + extra_sigma * n2, 0, 255)
 *   n1, n2 ~ N(0,1) from a counter-based generator: the splitmix64 finaliser keyed on (seed, frame, stage 0 / 1, channel,
 *   pixel), Box-Muller on 24 + 24 bits of one 64-bit draw.  Replaces the reference's rng.randn / np.random.normal:
 *   distribution-equivalent, not draw-identical.
 * Taps are built on the host (ffb6d_amd/train_data.py): sharpen 3x3 (ycb :118-122), linear motion blur with the
 * cv2.line 8-connected rasterisation (:88-105), Gaussian 3x3 / 5x5 (:129-133).  `in` and `out` must not overlap.
 * A frame whose n_taps or halo lies outside the limits above is copied (plus its noise); tap offsets are clamped into
 * [-halo, halo], so no tap list can read outside the staged tile. */
int ffb6d_rgb_stencil(const uint8_t* in, const ffb6d_stencil_frame_t* frames, uint64_t seed, uint8_t* out, int B,
                      int64_t H, int64_t W, ffb6d_stream_t stream);

/* Background compositing of B frames (add_real_back, ycb :145-163, linemod :166-186), one elementwise pass.
 *   rgb u8 [B,3,H,W], label [B,HW] (u8 or i32: label_u8), depth f32 [B,HW]
 *   back_rgb u8 [B,3,H,W], back_depth f32 [B,HW], back_mask [B,HW] (u8 or i32: back_mask_u8)
 *   flavour 0 = YCB: keep_back = back_mask <= 0 (the real frame's label); 1 = LineMOD: keep_back = back_mask < 255 (mask[...,0])
 *   composite_rgb u8 [B] or NULL (= all 1): 0 leaves a frame's RGB as it is (LineMOD composites with probability 0.6, :179)
 *   rgb_out[c]  = label <= 0 ? back_rgb[c] * keep_back : rgb[c]                 (when composite_rgb[b])
 *   depth_out   = depth > 1e-6 ? depth : back_depth * keep_back                 (msk_dp = dpt > 1e-6, ycb :196) */
int ffb6d_add_real_back(const uint8_t* rgb, const void* label, int label_u8, const float* depth, const uint8_t* back_rgb,
                        const float* back_depth, const void* back_mask, int back_mask_u8, int flavour,
                        const uint8_t* composite_rgb, uint8_t* rgb_out, float* depth_out, int B, int64_t HW,
                        ffb6d_stream_t stream);

/* ColorJitter of B uint8 images [B,3,H,W]: torchvision's transforms.ColorJitter on its PIL backend, which the reference applies to
 * every decoded frame when add_noise is on (self.trancolor, linemod_dataset.py:35,221-223, ycb_dataset.py:34,190-193).  That
 * backend is a thin layer over Pillow (ImageEnhance.Brightness / Contrast / Color, an HSV round trip with a uint8 hue shift), and
 * Pillow is installed where this library is built: the rule below is held to Pillow's own bytes (tests/golden/color_jitter.npz,
 * tests/test_color_jitter_cpu.py), not to a restatement alone.
 * Layout: plane 0 = R, plane 1 = G, plane 2 = B.  NOT the convention of the OpenCV stages above, where plane 0 plays "B": the
 * reference jitters the PIL image (RGB) before it becomes the array that rgb_add_noise hands to OpenCV.
 * A frame carries a chain of at most four operations, applied in the frame's own order, each to the uint8 result of the one before.
 *   L(r,g,b) = (r 19595 + g 38470 + b 7471 + 0x8000) >> 16                                        (Pillow's RGB -> L)
 *   blend(d, x, alpha): t = (float)d + alpha * ((float)x - (float)d)    float32, product and sum rounded separately (no FMA)
 *                       out = t <= 0 ? 0 : t >= 255 ? 255 : (uint8)t    (truncation)
 *   FFB6D_JITTER_BRIGHTNESS  blend(0, x, alpha)
 *   FFB6D_JITTER_CONTRAST    blend(m, x, alpha) on every channel, m = (int)((double)sum L / (double)(H W) + 0.5); the sum runs over
 *                            the whole frame AS IT STANDS when the contrast is reached, i.e. after the operations before it
 *   FFB6D_JITTER_SATURATION  blend(L(pixel), x, alpha)
 *   FFB6D_JITTER_HUE         RGB -> HSV, h' = (h + hue_shift) & 255, HSV -> RGB; alpha is not used.  hue_shift = (int)(hue * 255.0)
 *                            truncated toward zero, modulo 256 (hue = -0.05 gives 244: np.uint8 wrap-around in torchvision)
 *   RGB -> HSV: V = max; max == min: H = S = 0; otherwise
 *     cr = (float)(max - min), s = cr / (float)max, rc, gc, bc = (float)(max - c) / cr                       (float32 quotients)
 *     h = r == max ? bc - gc : g == max ? 2.0 + rc - bc : 4.0 + gc - rc         in double from the float32 quotients, then (float)
 *     h = fmod(h / 6.0 + 1.0, 1.0)                                              in double, then (float)
 *     H = clip((int)(h * 255.0), 0, 255), S = clip((int)(s * 255.0), 0, 255)    products in double
 *   HSV -> RGB: S == 0: R = G = B = V; otherwise, all float32:
 *     hh = (float)H * 6 / 255, i = floor(hh), f = hh - i, fs = (float)S / 255
 *     p = round(V (1 - fs)), q = round(V (1 - fs f)), t = round(V (1 - fs (1 - f)))      C round, clipped to 0..255
 *     (R,G,B) = [(V,t,p), (q,V,p), (p,V,t), (p,q,V), (t,p,V), (V,p,q)][i mod 6] */
#define FFB6D_JITTER_BRIGHTNESS 0
#define FFB6D_JITTER_CONTRAST 1
#define FFB6D_JITTER_SATURATION 2
#define FFB6D_JITTER_HUE 3
#define FFB6D_JITTER_MAX_OPS 4

/* One frame's chain (host-built, uploaded as an array of B; every field 4 bytes wide: no padding). */
typedef struct {
    int32_t n_ops;                        /* 0: the frame is copied; at most FFB6D_JITTER_MAX_OPS */
    int32_t op[FFB6D_JITTER_MAX_OPS];     /* FFB6D_JITTER_* in the order of application, no operation twice */
    float alpha[FFB6D_JITTER_MAX_OPS];    /* factor of op[i], finite and >= 0 (not used for the hue) */
    int32_t hue_shift;                    /* 0..255 */
} ffb6d_jitter_frame_t;

/* Checks B records in HOST memory: FFB6D_ERR_ARG for n_ops outside [0, 4], an unknown or a repeated operation, a negative or
 * non-finite factor, a hue_shift outside [0, 255].  ffb6d_color_jitter_u8 takes its records in device memory and reads nothing
 * back, so it cannot refuse a bad record itself: callers check them here before the upload (ffb6d_amd.train_data does), and the
 * kernels, for which the same predicate holds, copy a frame whose record fails it. */
int ffb6d_jitter_frames_check(const ffb6d_jitter_frame_t* host_frames, int B);

/* Bytes of device workspace for ffb6d_color_jitter_u8 (per-workgroup luminance sums; 0 for an empty batch). */
size_t ffb6d_color_jitter_workspace_bytes(int B, int64_t H, int64_t W);

/* The whole batch in two launches, whatever the per-frame orders; no read-back, no host wait.
 *   sum pass    frames whose chain holds a contrast: every lane applies the operations BEFORE the contrast to its pixels in
 *               registers and adds their L; each workgroup writes one 64-bit integer partial sum into the workspace (integer sums
 *               are exact in any order; partial sums rather than an atomic into a slot, so that no third launch has to zero the
 *               slot and the workspace may hold anything on entry).  Workgroups of other frames exit at once.
 *   apply pass  every workgroup adds its frame's partial sums (at most 1024), takes the mean, applies the frame's whole chain to
 *               its pixels in registers and stores once.
 * Each lane takes 16 consecutive pixels of the three planes: one 16-byte load / store per plane when H W is a multiple of 16 and
 * `in` / `out` are 16-byte aligned (planes of another size do not keep the alignment from one plane to the next), 4-byte words
 * when H W is a multiple of 4 and the pointers are 4-byte aligned, single bytes otherwise and for the last, partial run.
 * FFB6D_ERR_ARG, with nothing launched or written: negative sizes, a null pointer, in == out, B > 65535;
 * FFB6D_ERR_WORKSPACE: a workspace below ffb6d_color_jitter_workspace_bytes (or not 8-byte aligned). */
int ffb6d_color_jitter_u8(const uint8_t* in, const ffb6d_jitter_frame_t* frames, uint8_t* out, int B, int64_t H, int64_t W,
                          void* workspace, size_t workspace_bytes, ffb6d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
