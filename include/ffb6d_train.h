/* include/ffb6d_train.h -- C ABI of the gfx950 training-sample arithmetic: what the training half of the reference's
 * Dataset.get_item computes per frame on the CPU, batched on the device.
 *
 *   ffb6d_pose_targets        get_pose_gt_info + labels_pt   ycb_dataset.py:240,348-386, linemod_dataset.py:287,398-436
 *   ffb6d_rgb_hsv_jitter      rgb_add_noise, HSV stage       ycb_dataset.py:110-116, linemod_dataset.py:145-151
 *   ffb6d_rgb_stencil         rgb_add_noise, filter2D / GaussianBlur stages and the Gaussian noise
 *                                                             ycb_dataset.py:82-143, linemod_dataset.py:117-164
 *   ffb6d_add_real_back       add_real_back                  ycb_dataset.py:145-163, linemod_dataset.py:166-186
 *
 * All pointers are DEVICE pointers.  Return value: 0 or an FFB6D_ERR_* code (text through ffb6d_last_error()); on an
 * error nothing is written.  No call reads anything back or waits: each enqueues one kernel on `stream`.
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

#ifdef __cplusplus
}
#endif
#endif
