// ffb6d_amd/csrc/train_inst.hip -- pose targets per INSTANCE (include/ffb6d_train.h, ffb6d_pose_targets_inst): the arithmetic of
// pose_targets_kernel (train_data.hip), with a point's object found through the renderer's instance image instead of the class
// label image, so that several instances of one class in a frame keep their own keypoints.
//
//   inst_rows_kernel: one thread per (instance, keypoint-or-centre) row, I * (K + 1) rows.  Transforms the model point in double,
//     writes the double row into the workspace and its float copy into kp_3ds / ctr_3ds; an instance whose frame or class id is
//     bad gets zero rows.  The thread of an instance's centre row also zeroes n_points[i], so the count needs no launch of its own
//     and the workspace may hold anything on entry.
//   inst_points_kernel: one workgroup = (frame, 128 points), as pose_targets_kernel.  It stages its points' coordinates and owning
//     instance in LDS, then writes the flat [128, K, 3] offset rows: 4 consecutive floats per thread as one 16-byte store when the
//     rows keep that alignment, single floats otherwise.  The 4 keypoint coordinates a thread subtracts are 4 consecutive doubles
//     of its instance's workspace row ((i (K + 1) + k) 3 + j = i (K + 1) 3 + r for the r-th float of a point's row), a few KB per
//     instance that every workgroup of the frame re-reads from cache.
//     Counting: every owned point adds 1 to its instance's LDS counter; the point whose add returned 0 adds the counter's final
//     value to n_points[i] after the barrier -- one integer atomic per (workgroup, instance present in it), exact in any order.
#include <climits>

#include "common.h"
#include "ffb6d_train.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPts = 128;                   // points per workgroup
constexpr int kMaxK = 64;
constexpr int kMaxI = 1024;                 // render.MAX_INSTANCES

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// the frame and class of instance i as the rule reads them: class 0 = the instance does not exist
__device__ __forceinline__ int inst_class(const int* __restrict__ frame_of, const int* __restrict__ class_of, int i, int B,
                                          int n_cls, int& frame)
{
    frame = frame_of[i];
    const int c = class_of[i];
    return (frame >= 0 && frame < B && c >= 1 && c < n_cls) ? c : 0;
}

__global__ __launch_bounds__(kThreads) void inst_rows_kernel(
    const int* __restrict__ frame_of, const int* __restrict__ class_of, const double* __restrict__ poses,
    const float* __restrict__ mesh_kps, const float* __restrict__ mesh_ctr, int n_cls, int B, int I, int K,
    double* __restrict__ xf, float* __restrict__ kp_3ds, float* __restrict__ ctr_3ds, int* __restrict__ n_points)
{
    const int K1 = K + 1;
    const int row = blockIdx.x * kThreads + threadIdx.x;
    if (row >= I * K1) return;
    const int i = row / K1, k = row - i * K1;
    int frame;
    const int c = inst_class(frame_of, class_of, i, B, n_cls, frame);
    double p[3] = {0.0, 0.0, 0.0};
    if (c != 0) {
        const float* m = k < K ? mesh_kps + (static_cast<int64_t>(c) * K + k) * 3 : mesh_ctr + static_cast<int64_t>(c) * 3;
        const double m0 = m[0], m1 = m[1], m2 = m[2];
        const double* rt = poses + static_cast<int64_t>(i) * 12;
#pragma unroll
        for (int j = 0; j < 3; ++j) p[j] = ((m0 * rt[4 * j] + m1 * rt[4 * j + 1]) + m2 * rt[4 * j + 2]) + rt[4 * j + 3];
    }
    float* dst = k < K ? kp_3ds + (static_cast<int64_t>(i) * K + k) * 3 : ctr_3ds + static_cast<int64_t>(i) * 3;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        xf[static_cast<int64_t>(row) * 3 + j] = p[j];
        dst[j] = static_cast<float>(p[j]);
    }
    if (k == K) n_points[i] = 0;
}

template <bool kVec>
__global__ __launch_bounds__(kThreads) void inst_points_kernel(
    const float* __restrict__ cld, const void* __restrict__ choose, int choose_i64, const int* __restrict__ inst_img,
    const int* __restrict__ frame_of, const int* __restrict__ class_of, const double* __restrict__ xf, int n_cls, int B, int64_t N,
    int64_t HW, int I, int K, int* __restrict__ labels, int* __restrict__ inst_of_point, float* __restrict__ kp_ofst,
    float* __restrict__ ctr_ofst, int* __restrict__ n_points)
{
    __shared__ float cld_s[kPts * 3];
    __shared__ int match_s[kPts];
    __shared__ int cnt_s[kMaxI];
    const int b = blockIdx.y;
    const int tid = threadIdx.x;
    const int64_t n0 = static_cast<int64_t>(blockIdx.x) * kPts;
    const int np = N - n0 >= kPts ? kPts : N - n0 > 0 ? static_cast<int>(N - n0) : 0;
    const int K1 = K + 1;

    for (int i = tid; i < I; i += kThreads) cnt_s[i] = 0;
    __syncthreads();

    const int64_t row0 = static_cast<int64_t>(b) * N + n0;
    for (int i = tid; i < np * 3; i += kThreads) cld_s[i] = cld[row0 * 3 + i];
    bool leader = false;
    int mine = -1;
    if (tid < np) {
        const int64_t idx = choose_i64 ? static_cast<const int64_t*>(choose)[row0 + tid]
                                       : static_cast<int64_t>(static_cast<const int*>(choose)[row0 + tid]);
        int lab = 0;
        if (idx >= 0 && idx < HW) {
            const int i = inst_img[static_cast<int64_t>(b) * HW + idx];
            if (i >= 0 && i < I) {                              // only now is i an index
                int frame;
                const int c = inst_class(frame_of, class_of, i, B, n_cls, frame);
                if (c != 0 && frame == b) { lab = c; mine = i; }
            }
        }
        labels[row0 + tid] = lab;
        inst_of_point[row0 + tid] = mine;
        match_s[tid] = mine;
        if (mine >= 0) leader = atomicAdd(&cnt_s[mine], 1) == 0;
    }
    __syncthreads();
    if (leader) atomicAdd(&n_points[mine], cnt_s[mine]);

    const int row = K * 3;
    float* kp_dst = kp_ofst + row0 * row;
    if (kVec) {
        // the launcher checked that N * row is a multiple of 4 floats and the pointer 16-byte aligned; a tile starts a multiple of
        // 128 rows into its frame, so row0 * row and np * row = (N - n0) * row are multiples of 4 too: whole 16-byte stores only
        for (int i = tid * 4; i < np * row; i += kThreads * 4) {
            float v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int e = i + q;
                const int p = e / row, r = e - p * row, j = r % 3;
                const int m = match_s[p];
                v[q] = m >= 0 ? static_cast<float>(static_cast<double>(cld_s[p * 3 + j]) - xf[static_cast<int64_t>(m) * K1 * 3 + r]) : 0.f;
            }
            *reinterpret_cast<float4*>(kp_dst + i) = make_float4(v[0], v[1], v[2], v[3]);
        }
    } else {
        for (int i = tid; i < np * row; i += kThreads) {
            const int p = i / row, r = i - p * row, j = r % 3;
            const int m = match_s[p];
            kp_dst[i] = m >= 0 ? static_cast<float>(static_cast<double>(cld_s[p * 3 + j]) - xf[static_cast<int64_t>(m) * K1 * 3 + r]) : 0.f;
        }
    }
    float* ctr_dst = ctr_ofst + row0 * 3;
    for (int i = tid; i < np * 3; i += kThreads) {
        const int p = i / 3, j = i - p * 3;
        const int m = match_s[p];
        ctr_dst[i] = m >= 0 ? static_cast<float>(static_cast<double>(cld_s[i]) - xf[(static_cast<int64_t>(m) * K1 + K) * 3 + j]) : 0.f;
    }
}

}  // namespace

extern "C" {

size_t ffb6d_pose_targets_inst_workspace_bytes(int I, int K)
{
    if (I <= 0 || K <= 0) return 0;
    const size_t bytes = static_cast<size_t>(I) * static_cast<size_t>(K + 1) * 3 * sizeof(double);
    return (bytes + 255) / 256 * 256;
}

int ffb6d_pose_targets_inst(const float* cld, const void* choose, int choose_i64, const int* inst_img, const int* frame_of,
                            const int* class_of, const double* poses, const float* mesh_kps, const float* mesh_ctr, int n_cls,
                            int B, int64_t N, int64_t HW, int I, int K, int* labels, int* inst_of_point, float* kp_targ_ofst,
                            float* ctr_targ_ofst, float* kp_3ds, float* ctr_3ds, int* n_points, void* workspace,
                            size_t workspace_bytes, ffb6d_stream_t stream)
{
    FFB6D_REQUIRE(B >= 0 && N >= 0 && HW >= 0 && n_cls >= 1, "ffb6d_pose_targets_inst: B = %d, N = %lld, HW = %lld, n_cls = %d", B,
                  static_cast<long long>(N), static_cast<long long>(HW), n_cls);
    FFB6D_REQUIRE(K >= 1 && K <= kMaxK && I >= 0 && I <= kMaxI,
                  "ffb6d_pose_targets_inst: K = %d, I = %d outside the limits (1 <= K <= %d, 0 <= I <= %d)", K, I, kMaxK, kMaxI);
    const bool points = B > 0 && N > 0;
    if (I == 0 && !points) return FFB6D_OK;
    FFB6D_REQUIRE(I == 0 || (frame_of && class_of && poses && mesh_kps && mesh_ctr && kp_3ds && ctr_3ds && n_points),
                  "ffb6d_pose_targets_inst: a null instance pointer");
    FFB6D_REQUIRE(!points || (cld && choose && labels && inst_of_point && kp_targ_ofst && ctr_targ_ofst && (HW == 0 || inst_img)),
                  "ffb6d_pose_targets_inst: a null point pointer");
    const int64_t tiles = ffb6d::ceil_div(N, kPts);
    FFB6D_REQUIRE(tiles <= INT_MAX && B <= 65535, "ffb6d_pose_targets_inst: grid %lld x %d", static_cast<long long>(tiles), B);
    const size_t need = ffb6d_pose_targets_inst_workspace_bytes(I, K);
    if (need != 0 && (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 7u) != 0))
        return ffb6d::set_error(FFB6D_ERR_WORKSPACE, "ffb6d_pose_targets_inst: workspace %zu < %zu bytes (or null, or not 8-byte aligned)",
                                workspace_bytes, need);
    double* xf = static_cast<double*>(workspace);
    hipStream_t s = ffb6d::as_stream(stream);
    if (I > 0) {
        const int blocks = static_cast<int>(ffb6d::ceil_div(static_cast<int64_t>(I) * (K + 1), kThreads));
        inst_rows_kernel<<<dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, s>>>(
            frame_of, class_of, poses, mesh_kps, mesh_ctr, n_cls, B, I, K, xf, kp_3ds, ctr_3ds, n_points);
        FFB6D_LAUNCH_CHECK();
    }
    if (points) {
        const dim3 grid(static_cast<unsigned>(tiles), static_cast<unsigned>(B));
        if ((N * K * 3) % 4 == 0 && aligned16(kp_targ_ofst))
            inst_points_kernel<true><<<grid, dim3(kThreads), 0, s>>>(cld, choose, choose_i64, inst_img, frame_of, class_of, xf,
                                                                     n_cls, B, N, HW, I, K, labels, inst_of_point, kp_targ_ofst,
                                                                     ctr_targ_ofst, n_points);
        else
            inst_points_kernel<false><<<grid, dim3(kThreads), 0, s>>>(cld, choose, choose_i64, inst_img, frame_of, class_of, xf,
                                                                      n_cls, B, N, HW, I, K, labels, inst_of_point, kp_targ_ofst,
                                                                      ctr_targ_ofst, n_points);
        FFB6D_LAUNCH_CHECK();
    }
    return FFB6D_OK;
}

}  // extern "C"
