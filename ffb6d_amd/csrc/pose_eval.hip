// ffb6d_amd/csrc/pose_eval.hip -- ADD / ADD-S of a batch of (predicted, ground-truth) poses in one call
// (include/ffb6d_eval.h; basic_utils.py:651-669).
//
// ADD-S is N^2 pair distances per row, brute force as in the reference (which builds two [N,N,3] tensors per object).
//   add_adds_pairs_kernel: one workgroup = (row, slice s of the predicted cloud, tile of kGtTile ground-truth points).
//     Every thread keeps kPer ground-truth points in registers; the slice's predicted points are transformed and staged
//     through LDS kPdTile at a time and read back as wave-wide broadcasts.  Minima over squared distances go to the
//     workspace per (row, slice, point); the slice-0 workgroups also store the point's ADD distance.
//   add_adds_reduce_kernel: one workgroup per row: min over the slices, one sqrtf per point, both means summed in double
//     in an order that depends on N only (thread-strided partial sums, then a fixed tree), rounded once to f32.
// Both kernels compute pd_i with the same inline code and the same squared-distance expression, so the j = i candidate of
// ADD-S is bit-identical to the ADD term and adds <= add holds exactly.
#include <climits>
#include <cmath>
#include <vector>

#include "common.h"
#include "ffb6d_eval.h"

namespace {

constexpr int kSlices = 8;                  // the predicted cloud of a row is split into this many slices (fills the chip)
constexpr int kThreads = 256;
constexpr int kPer = 4;                     // ground-truth points per thread
constexpr int kGtTile = kThreads * kPer;    // ground-truth points per workgroup
constexpr int kPdTile = kThreads;           // predicted points per LDS tile (one per thread to stage)

// R * p + t with every product and sum rounded on its own (the build has -ffp-contract=off)
__device__ __forceinline__ void xform(const float* T, float x, float y, float z, float& ox, float& oy, float& oz)
{
    ox = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
    oy = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
    oz = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
}

__device__ __forceinline__ float sq_dist(float px, float py, float pz, float gx, float gy, float gz)
{
    const float dx = px - gx, dy = py - gy, dz = pz - gz;
    return (dx * dx + dy * dy) + dz * dz;
}

__global__ __launch_bounds__(kThreads) void add_adds_pairs_kernel(const float* __restrict__ pts, const int64_t* __restrict__ begin,
                                                                  const int* __restrict__ class_of, const float* __restrict__ pred_RT,
                                                                  const float* __restrict__ gt_RT, int n_tiles, int64_t max_n,
                                                                  float* __restrict__ ws_add, float* __restrict__ ws_min)
{
    const int tile = blockIdx.x % n_tiles;
    const int s = (blockIdx.x / n_tiles) % kSlices;
    const int q = blockIdx.x / (n_tiles * kSlices);
    const int c = class_of[q];
    const int64_t b = begin[c];
    const int n = static_cast<int>(begin[c + 1] - b);
    const int i0 = tile * kGtTile;
    if (i0 >= n) return;                                      // uniform over the workgroup
    const int chunk = (n + kSlices - 1) / kSlices;
    const int j0 = min(n, s * chunk), j1 = min(n, j0 + chunk);
    const float* p = pts + 3 * b;
    const int tid = threadIdx.x;

    float Tp[12], Tg[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        Tp[k] = pred_RT[12 * q + k];
        Tg[k] = gt_RT[12 * q + k];
    }

    float gx[kPer], gy[kPer], gz[kPer], best[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const int i = i0 + k * kThreads + tid;
        gx[k] = gy[k] = gz[k] = 0.f;
        best[k] = INFINITY;
        if (i < n) {
            const float x = p[3 * i], y = p[3 * i + 1], z = p[3 * i + 2];
            xform(Tg, x, y, z, gx[k], gy[k], gz[k]);
            if (s == 0) {
                float dx, dy, dz;
                xform(Tp, x, y, z, dx, dy, dz);
                ws_add[q * max_n + i] = sqrtf(sq_dist(dx, dy, dz, gx[k], gy[k], gz[k]));
            }
        }
    }

    __shared__ float4 pd[kPdTile];
    for (int jt = j0; jt < j1; jt += kPdTile) {
        const int m = min(kPdTile, j1 - jt);
        __syncthreads();                                      // the previous tile has been read by every wave
        if (tid < m) {
            const int j = jt + tid;
            float x, y, z;
            xform(Tp, p[3 * j], p[3 * j + 1], p[3 * j + 2], x, y, z);
            pd[tid] = make_float4(x, y, z, 0.f);
        }
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < m; ++j) {
            const float4 d = pd[j];                           // same address in every lane: broadcast
#pragma unroll
            for (int k = 0; k < kPer; ++k) best[k] = fminf(best[k], sq_dist(d.x, d.y, d.z, gx[k], gy[k], gz[k]));
        }
    }

#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const int i = i0 + k * kThreads + tid;
        if (i < n) ws_min[(static_cast<int64_t>(q) * kSlices + s) * max_n + i] = best[k];
    }
}

__global__ __launch_bounds__(kThreads) void add_adds_reduce_kernel(const int64_t* __restrict__ begin, const int* __restrict__ class_of,
                                                                   int64_t max_n, const float* __restrict__ ws_add,
                                                                   const float* __restrict__ ws_min, float* __restrict__ add,
                                                                   float* __restrict__ adds)
{
    const int q = blockIdx.x;
    const int c = class_of[q];
    const int n = static_cast<int>(begin[c + 1] - begin[c]);
    const int tid = threadIdx.x;
    if (n == 0) {
        if (tid == 0) add[q] = adds[q] = NAN;
        return;
    }
    double sa = 0.0, ss = 0.0;
    for (int i = tid; i < n; i += kThreads) {
        float m = ws_min[static_cast<int64_t>(q) * kSlices * max_n + i];
#pragma unroll
        for (int s = 1; s < kSlices; ++s) m = fminf(m, ws_min[(static_cast<int64_t>(q) * kSlices + s) * max_n + i]);
        sa += static_cast<double>(ws_add[q * max_n + i]);
        ss += static_cast<double>(sqrtf(m));
    }
    __shared__ double red_a[kThreads], red_s[kThreads];
    red_a[tid] = sa;
    red_s[tid] = ss;
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        __syncthreads();
        if (tid < w) {
            red_a[tid] += red_a[tid + w];
            red_s[tid] += red_s[tid + w];
        }
    }
    if (tid == 0) {
        add[q] = static_cast<float>(red_a[0] / n);
        adds[q] = static_cast<float>(red_s[0] / n);
    }
}

}  // namespace

extern "C" {

size_t ffb6d_pose_add_adds_workspace_bytes(int Q, int64_t max_points)
{
    if (Q <= 0 || max_points <= 0) return 0;
    return static_cast<size_t>(Q) * static_cast<size_t>(max_points) * (kSlices + 1) * sizeof(float);
}

int ffb6d_pose_add_adds_f32(const float* model_pts, const int64_t* model_begin, int n_cls, const int* class_of,
                            const float* pred_RT, const float* gt_RT, int Q, float* add, float* adds,
                            void* workspace, size_t workspace_bytes, ffb6d_stream_t stream)
{
    FFB6D_REQUIRE(Q >= 0 && n_cls >= 0, "ffb6d_pose_add_adds_f32: Q = %d, n_cls = %d", Q, n_cls);
    if (Q == 0) return FFB6D_OK;
    FFB6D_REQUIRE(n_cls > 0 && model_begin && class_of && pred_RT && gt_RT && add && adds,
                  "ffb6d_pose_add_adds_f32: n_cls = %d or a null pointer", n_cls);
    hipStream_t st = ffb6d::as_stream(stream);
    std::vector<int> cls(Q);
    std::vector<int64_t> beg(static_cast<size_t>(n_cls) + 1);
    FFB6D_HIP_TRY(hipMemcpyAsync(cls.data(), class_of, sizeof(int) * cls.size(), hipMemcpyDeviceToHost, st));
    FFB6D_HIP_TRY(hipMemcpyAsync(beg.data(), model_begin, sizeof(int64_t) * beg.size(), hipMemcpyDeviceToHost, st));
    FFB6D_HIP_TRY(hipStreamSynchronize(st));
    FFB6D_REQUIRE(beg[0] >= 0, "ffb6d_pose_add_adds_f32: model_begin[0] = %lld", static_cast<long long>(beg[0]));
    for (int c = 0; c < n_cls; ++c)
        FFB6D_REQUIRE(beg[c + 1] >= beg[c] && beg[c + 1] - beg[c] <= INT_MAX / 3,
                      "ffb6d_pose_add_adds_f32: model_begin[%d..%d] = %lld..%lld", c, c + 1, static_cast<long long>(beg[c]),
                      static_cast<long long>(beg[c + 1]));
    FFB6D_REQUIRE(model_pts || beg[n_cls] == beg[0], "ffb6d_pose_add_adds_f32: model_pts is null");
    int64_t max_n = 0;
    for (int q = 0; q < Q; ++q) {
        FFB6D_REQUIRE(cls[q] >= 0 && cls[q] < n_cls, "ffb6d_pose_add_adds_f32: class_of[%d] = %d outside [0, %d)", q, cls[q], n_cls);
        max_n = std::max(max_n, beg[cls[q] + 1] - beg[cls[q]]);
    }
    const size_t need = ffb6d_pose_add_adds_workspace_bytes(Q, max_n);
    if (workspace_bytes < need || (need > 0 && workspace == nullptr))
        return ffb6d::set_error(FFB6D_ERR_WORKSPACE, "ffb6d_pose_add_adds_f32: workspace of %zu bytes, %zu needed (Q = %d, %lld points)",
                                workspace_bytes, need, Q, static_cast<long long>(max_n));
    float* ws_add = static_cast<float*>(workspace);
    float* ws_min = ws_add + static_cast<int64_t>(Q) * max_n;
    if (max_n > 0) {
        const int64_t n_tiles = ffb6d::ceil_div(max_n, kGtTile);
        const int64_t blocks = static_cast<int64_t>(Q) * kSlices * n_tiles;
        FFB6D_REQUIRE(blocks <= INT_MAX, "ffb6d_pose_add_adds_f32: %lld workgroups", static_cast<long long>(blocks));
        add_adds_pairs_kernel<<<dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, st>>>(
            model_pts, model_begin, class_of, pred_RT, gt_RT, static_cast<int>(n_tiles), max_n, ws_add, ws_min);
        FFB6D_LAUNCH_CHECK();
    }
    add_adds_reduce_kernel<<<dim3(Q), dim3(kThreads), 0, st>>>(model_begin, class_of, max_n, ws_add, ws_min, add, adds);
    FFB6D_LAUNCH_CHECK();
    return FFB6D_OK;
}

}  // extern "C"
