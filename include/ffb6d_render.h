/* include/ffb6d_render.h -- C ABI of the gfx950 mesh rasteriser: posed, vertex-coloured triangle meshes -> rgb, depth and
 * label frames, the first link of the training-sample chain (include/ffb6d_train.h takes over from a rendered frame).
 * The reference reads such frames from disk (linemod_dataset.py:55-103,209-249: the .pkl files under renders/<cls>/ and
 * fuse/<cls>/) and has them made by an external z-buffer library whose source is not part of it
 * (rgbd_rnder_sift_kp3ds.py:38-105), so there is no code to port: the algorithm is stated here and restated in numpy by
 * tests/render_ref.py.
 *
 * I instances (frame frame_of[i], class class_of[i], pose T[i] = [R|t], row-major double [3,4], model -> camera) are drawn
 * into B frames of H x W pixels with the pinhole intrinsics K[frame] (row-major double [3,3]; only fx = K[0], fy = K[4],
 * cx = K[2], cy = K[5] are read).  Every product, sum and quotient below is rounded on its own, in the order written (the
 * library is built with -ffp-contract=off); "double" is IEEE binary64, "float" binary32.
 *
 * Per vertex (x, y, z) of an instance, in double:
 *     Xc = ((R00*x + R01*y) + R02*z) + t0, likewise Yc (row 1) and Zc (row 2);   zf = (float)Zc
 *     u = (fx*Xc)/Zc + cx,  v = (fy*Yc)/Zc + cy;   Xs = llrint(256*u), Ys = llrint(256*v)  (round half to even)
 *   The vertex is UNUSABLE when !(zf >= z_near) or !(|256*u| <= 2^23) or !(|256*v| <= 2^23), tested in double before the
 *   conversion (a NaN or infinite pose gives unusable vertices, never an undefined conversion).
 *
 * Per triangle (face f of the class, vertices 0, 1, 2):
 *   dropped when a vertex is unusable (there is no clipping) or names no vertex of the class;
 *   A2 = (X1-X0)*(Y2-Y0) - (X2-X0)*(Y1-Y0) in int64; dropped when A2 == 0; when A2 < 0, vertices 1 and 2 trade places
 *   (with their depths and colours) and A2 changes sign.
 *   Edge i runs a -> b over the other two vertices in cyclic order (edge 0: 1 -> 2, edge 1: 2 -> 0, edge 2: 0 -> 1);
 *     E_i(P) = (Xb-Xa)*(Py-Ya) - (Yb-Ya)*(Px-Xa), exact in int64.
 *   The sample of pixel (row, col) is P = (256*col, 256*row): the sample convention of ffb6d_depth_to_cloud_f32
 *   (x = (col - cx) d / fx), so a rendered depth back-projects onto the surface.
 *   The sample is COVERED iff for every i: E_i > 0, or E_i == 0 and (dy > 0 or (dy == 0 and dx < 0)) with (dx, dy) = b - a.
 *   An edge and its reverse get opposite ownership: a sample on an edge shared by two triangles belongs to exactly one of
 *   them, whatever their vertex orders.  Candidate pixels: the sub-pixel bounding box clamped to the frame.
 *
 * Per covered sample, in double:
 *     b_i = (double)E_i / (double)A2,  iz_i = 1.0 / (double)zf_i,  w = (b0*iz0 + b1*iz1) + b2*iz2,  z = (float)(1.0 / w)
 *     key = bits(z) << 32 | i << 22 | f         (i = the instance, f = the face within its class)
 *   A pixel keeps the SMALLEST key: nearest depth, then lowest instance, then lowest face -- independent of the order in
 *   which triangles are drawn, so every run gives the same bits.
 *
 * Resolve, per pixel with a key:  depth = z, label = class_of[i], inst = i, face = f, and per colour channel
 *     c = (((b0*iz0)*c0 + (b1*iz1)*c1) + (b2*iz2)*c2) / w,   u8 = min(255, floor(c + 0.5))
 *   (b, iz, w recomputed from the key's triangle; c0..c2 the vertices' colours after the swap).  A pixel without a key gets
 *   depth 0, label 0, inst -1, face -1, rgb 0.  visible[i] = the number of pixels instance i owns (the reference discards
 *   renders with fewer than 500 of them, rgbd_rnder_sift_kp3ds.py:80).
 *
 * A frame index outside [0, B), a class id outside [0, n_cls) or a class without faces gives an instance without triangles.
 *
 * All pointers are DEVICE pointers; ffb6d_render_f32 enqueues its work on `stream` and returns without waiting for it or
 * reading anything back.  Return value: 0 or an FFB6D_ERR_* code (text through ffb6d_last_error()); on an error nothing is
 * launched and no output is written.
 */
#ifndef FFB6D_RENDER_H
#define FFB6D_RENDER_H

#include <stddef.h>
#include <stdint.h>

#include "ffb6d_knn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FFB6D_RENDER_MAX_INSTANCES 1024          /* 10 bits of the key */
#define FFB6D_RENDER_MAX_FACES (1 << 22)         /* faces of one class: 22 bits of the key */

/* Bytes of workspace of ffb6d_render_f32 (0 for sizes the call refuses): the key image u64 [B,H,W] and the screen vertices
 * {Xs i32, Ys i32, zf f32, usable i32} [I, max_verts], each rounded up to 256 bytes.  max_verts = the largest vertex count of
 * a class. */
size_t ffb6d_render_workspace_bytes(int I, int64_t max_verts, int B, int H, int W);

/* How the raster pass walks a triangle's candidate pixels; identical results:
 *   0 (default) = one thread per triangle walks its bounding box (meshes seen from 0.5 - 1.5 m: a few pixels each);
 *   1 = a wavefront per triangle, the bounding box spread over the lanes in 8 x 8 pixel tiles;
 *  -1 = automatic: form 1 for the triangles whose clamped bounding box holds more than 256 pixels, form 0 for the rest. */
void ffb6d_render_set_form(int form);

/* The mesh set (made once per object set, see ffb6d_amd/render.py PreparedMeshes):
 *   verts f32 [Vtot,3], colors u8 [Vtot,3], faces i32 [Ftot,3] (vertex indices WITHIN the class),
 *   vert_begin, face_begin i64 [n_cls+1]: class c owns the rows vert_begin[c] .. vert_begin[c+1]-1 of verts / colors and
 *   face_begin[c] .. face_begin[c+1]-1 of faces; a class may be empty.  max_verts / max_faces: the largest count of a class
 *   (the host sizes its launches by them and reads nothing back; rows beyond them are not drawn); max_faces <= 2^22.
 *   The tables are clamped to [0, Vtot] / [0, Ftot] and a face that names no vertex of its class is dropped: no table
 *   content makes the kernels read outside the arrays.
 * The call:
 *   frame_of, class_of i32 [I]; T f64 [I,3,4]; K f64 [B,3,3]; 0 <= I <= 1024 (I = 0: empty frames); B*H*W < 2^31; z_near > 0.
 * Outputs, each may be NULL but not all of them:
 *   rgb u8 [B,3,H,W], depth f32 [B,H,W], label i32 [B,H,W], inst i32 [B,H,W], face i32 [B,H,W], visible i32 [I].
 * Three launches (vertices, raster, resolve) behind two fills; the key image is combined with 64-bit global minimum atomics. */
int ffb6d_render_f32(const float* verts, const unsigned char* colors, const int* faces, const int64_t* vert_begin,
                     const int64_t* face_begin, int n_cls, int64_t Vtot, int64_t Ftot, int64_t max_verts, int64_t max_faces,
                     const int* frame_of, const int* class_of, const double* T, int I, const double* K, int B, int H, int W,
                     float z_near, unsigned char* rgb, float* depth, int* label, int* inst, int* face, int* visible,
                     void* workspace, size_t workspace_bytes, ffb6d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
