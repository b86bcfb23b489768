// ffb6d_amd/csrc/bop_common.h -- what the streaming passes over depth images share (csrc/bop_eval.hip: VSD; csrc/bop_scene.hip:
// instance visibility): the shape of a run of pixels, the ray distance dist(z) of include/ffb6d_bop.h and the pixel loader.
// The library is built with -ffp-contract=off; float division and __fsqrt_rn are correctly rounded.
#pragma once
#include "common.h"

namespace ffb6d {
namespace bop {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPx = 4;                              // pixels per lane and step: 16 bytes of each image
constexpr int kSteps = 4;
constexpr int kRunPx = kThreads * kPx * kSteps;     // pixels per workgroup

struct Camera { float fx, fy, cx, cy; };

__device__ __forceinline__ float ray_dist(float z, int r, int c, const Camera& k)
{
    if (z == 0.f) return 0.f;
    const float X = ((static_cast<float>(c) - k.cx) * z) / k.fx;
    const float Y = ((static_cast<float>(r) - k.cy) * z) / k.fy;
    return __fsqrt_rn((X * X + Y * Y) + z * z);
}

// n floats from p (n == kPx and kVec == 4: one 16-byte access); entries past n read as 0
template <int kVec>
__device__ __forceinline__ void load_px(const float* __restrict__ p, int n, float (&v)[kPx])
{
    if (kVec == 4 && n == kPx) {
        const float4 x = *reinterpret_cast<const float4*>(p);
        v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
    } else {
#pragma unroll
        for (int j = 0; j < kPx; ++j) v[j] = j < n ? p[j] : 0.f;
    }
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace bop
}  // namespace ffb6d
