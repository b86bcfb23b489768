// ffb6d_amd/csrc/knn_common.h -- what the exact-KNN sources (knn.hip, knn_pruned.hip) state once: the padded K and its dispatch,
// the reference-order squared distance, the flattened-grid guard of the batched launches.
#pragma once
#include "common.h"

#include <climits>
#include <type_traits>

namespace ffb6d {

// the kernels are instantiated for K = 1, 2, 4, ..., 32; a search with another K runs the next one and stores its first K results
inline int pad_k(int K)
{
    int p = 1;
    while (p < K) p <<= 1;
    return p;
}

// f(std::integral_constant<int, kp>) for kp = pad_k(K) of a K in [1,32]: the one place that turns the padded K into a template argument
template <typename F>
int dispatch_padded_k(int kp, F&& f)
{
    switch (kp) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 8: return f(std::integral_constant<int, 8>{});
        case 16: return f(std::integral_constant<int, 16>{});
        case 32: return f(std::integral_constant<int, 32>{});
    }
    return set_error(FFB6D_ERR_ARG, "knn: unsupported padded K=%d", kp);
}

// A batched launch flattens (search, frame, query block) into blockIdx.x: `blocks` grows by gx * B per search, counted in 64 bits
// (a shape that overflows an int here could not be allocated, but it must fail as an argument error, not wrap around).
inline int add_blocks(int64_t& blocks, int64_t gx, int64_t B)
{
    blocks += gx * B;
    FFB6D_REQUIRE(blocks <= INT_MAX, "knn: a launch of %lld workgroups does not fit the grid", (long long)blocks);
    return FFB6D_OK;
}

// squared distance with the reference's operation order ((dx*dx+dy*dy)+dz*dz, nanoflann.hpp:323-348), each op rounded to f32
__device__ __forceinline__ float sqdist3(float qx, float qy, float qz, float px, float py, float pz)
{
    const float dx = __fsub_rn(qx, px), dy = __fsub_rn(qy, py), dz = __fsub_rn(qz, pz);
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

}  // namespace ffb6d
