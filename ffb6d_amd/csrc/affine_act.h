// ffb6d_amd/csrc/affine_act.h -- the arithmetic of the colour branch's BatchNorm / residual / activation glue (extractors.py:49-63)
// on one 16-byte unit of a row, shared by affine_act_pm_kernel (csrc/ops_pm.hip) and the Winograd output transform
// (csrc/winograd.h) so that a residual block computes the same expression in the same order on either path:
//     v = act( scale*v + shift + (res ? (rscale ? rscale*res + rshift : res) : 0) ),   act(v) = v > 0 ? v : slope*v
// (the library is compiled with -ffp-contract=off: every product and sum rounds separately)
#pragma once
#include <hip/hip_runtime.h>

namespace ffb6d {

// fp32 per-channel parameters (BatchNorm scale / shift) of a unit's VL channels
template <int VL>
__device__ __forceinline__ void load_params(const float* p, int unit, float (&out)[VL])
{
#pragma unroll
    for (int i = 0; i < VL; i += 4) {
        const float4 f = *reinterpret_cast<const float4*>(p + (size_t)unit * VL + i);
        out[i] = f.x; out[i + 1] = f.y; out[i + 2] = f.z; out[i + 3] = f.w;
    }
}

// res: the unit of the residual row or null; rs / rb: the residual's own affine (the down-sample block), read only with has_raff
template <int VL>
__device__ __forceinline__ void affine_act_unit(float (&v)[VL], const float (&s)[VL], const float (&b)[VL], const float* res, bool has_raff,
                                                const float (&rs)[VL], const float (&rb)[VL], float slope)
{
#pragma unroll
    for (int e = 0; e < VL; ++e) v[e] = v[e] * s[e] + b[e];
    if (res) {
        if (has_raff) {
#pragma unroll
            for (int e = 0; e < VL; ++e) v[e] += res[e] * rs[e] + rb[e];
        } else {
#pragma unroll
            for (int e = 0; e < VL; ++e) v[e] += res[e];
        }
    }
#pragma unroll
    for (int e = 0; e < VL; ++e) v[e] = v[e] > 0.f ? v[e] : slope * v[e];     // exact PReLU for ANY learned slope (> 1, < 0)
}

}  // namespace ffb6d
