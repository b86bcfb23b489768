// ffb6d_amd/csrc/winograd.h -- the two data transforms of Winograd F(2x2,3x3) around the batched tile-sequence GEMM
// (csrc/mlp_pm.hip: ffb6d_mlp_pm_batched_f32), for the wide stride-1 3x3 convolutions of the colour trunk (extractors.py:49-63,
// BasicBlock: conv3x3 -> BN -> ReLU -> conv3x3 -> BN -> (+ residual) -> ReLU), fp32 inference.
//
//   Y = A^T [ (G g G^T) .* (B^T d B) ] A        (Lavin & Gray, "Fast Algorithms for Convolutional Neural Networks", 2015)
//
// per 4 x 4 input window d (stride 2) and 2 x 2 output tile Y, summed over the input channels: 16 multiplies per output tile and
// channel pair where the direct form needs 36.  The sum over channels of position xi = 4u + v of the transformed tiles is a GEMM
// of its own, M[xi] = V[xi] U[xi]^T -- 16 GEMMs with 16 weight matrices, one launch.  Layouts are pixel-major like everything else:
//     x [B,H,W,C]      V [16][Tp][C]      U [16][O][C]      M [16][Tp][O]      out [B,H,W,O]
// T = B * ceil(H/2) * ceil(W/2) tiles numbered (b, ty, tx), Tp = T rounded up to the GEMM's point tile of 128 rows.
//
// Both kernels are memory bound and built alike: one lane owns 4 channels (16 bytes) of one tile, lanes run along the channels, so
// each of a lane's 16 loads and 16 (or 4) stores is its piece of a contiguous row segment.  Every access goes through a
// range-checked buffer descriptor at an offset computed from the tile number alone (nothing is addressed through a loaded value);
// a pixel outside the map sits at an out-of-range offset: it loads as zero (= padding 1, and the odd last row / column of an odd
// map) and its store is dropped.
//
// Below the F(2x2) pair: the same two transforms for F(4x4,3x3) (6 x 6 windows at stride 4, 36 planes), taken where its GEMM has fewer
// rows (forward_pm.wino_variant).
//
// Kernels and their launchers; compiled in csrc/ops_pm.hip, the translation unit of the colour branch's glue kernels, whose C entry
// points ffb6d_wino_input_f32 / ffb6d_wino_output_f32 and ffb6d_wino4_input_f32 / ffb6d_wino4_output_f32 call them (one unit, so that
// every build of that unit carries all four).
#pragma once
#include "affine_act.h"
#include "common.h"
#include "ffb6d_ops.h"
#include "mfma_pm.h"

namespace ffb6d {
namespace wino {

using pm::make_rsrc;
using pm::u32x4;

constexpr int BLK = 256;
constexpr int OOB = 0x7ffffff0;                       // byte offset past every buffer (each is < 2 GiB: host check)

struct WinoGeom {
    int H, W, C;          // map, channels of the rows this kernel moves (input channels / output channels)
    int TH, TW, T, Tp;    // tiles per column / row, tiles, tiles padded to the GEMM's point tile
};

__device__ __forceinline__ float4 as_f4(u32x4 u)
{
    return make_float4(__uint_as_float(u[0]), __uint_as_float(u[1]), __uint_as_float(u[2]), __uint_as_float(u[3]));
}
__device__ __forceinline__ u32x4 as_u4(float4 f)
{
    u32x4 u = {__float_as_uint(f.x), __float_as_uint(f.y), __float_as_uint(f.z), __float_as_uint(f.w)};
    return u;
}
__device__ __forceinline__ float4 operator+(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 operator-(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }

// ------------------------------------------------------------------------------------------------
// V = B^T d B,  B^T = [[1,0,-1,0],[0,1,1,0],[0,-1,1,0],[0,1,0,-1]]: adds and subtracts only.  d = the 4 x 4 window whose top left
// pixel is (2 ty - 1, 2 tx - 1).  Rows T .. Tp - 1 of every plane of V are NEVER written: the rows of a GEMM are independent of
// each other, so whatever they hold reaches only rows T .. Tp - 1 of M, which the output transform never reads.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BLK)
wino_input_f32_kernel(const float* __restrict__ x, float* __restrict__ v, const WinoGeom g, unsigned x_bytes, unsigned v_bytes, int q,
                      unsigned total)
{
    const unsigned t = blockIdx.x * BLK + threadIdx.x;
    if (t >= total) return;
    const int tile = (int)(t / (unsigned)q), cq = (int)(t - (unsigned)tile * (unsigned)q);
    const int tx = tile % g.TW, ty = (tile / g.TW) % g.TH, b = tile / (g.TW * g.TH);
    const __amdgpu_buffer_rsrc_t rs_x = make_rsrc(x, x_bytes), rs_v = make_rsrc(v, v_bytes);

    float4 d[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int y = 2 * ty - 1 + i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int xx = 2 * tx - 1 + j;
            const bool in = y >= 0 && y < g.H && xx >= 0 && xx < g.W;
            const int off = in ? (((b * g.H + y) * g.W + xx) * g.C + cq * 4) * 4 : OOB;
            d[i][j] = as_f4(__builtin_amdgcn_raw_buffer_load_b128(rs_x, off, 0, 0));
        }
    }
    float4 r[4][4];                                   // B^T d
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        r[0][j] = d[0][j] - d[2][j];
        r[1][j] = d[1][j] + d[2][j];
        r[2][j] = d[2][j] - d[1][j];
        r[3][j] = d[1][j] - d[3][j];
    }
    const int row = (tile * g.C + cq * 4) * 4, plane = g.Tp * g.C * 4;      // bytes
#pragma unroll
    for (int i = 0; i < 4; ++i) {                     // (B^T d) B
        const float4 o[4] = {r[i][0] - r[i][2], r[i][1] + r[i][2], r[i][2] - r[i][1], r[i][1] - r[i][3]};
#pragma unroll
        for (int j = 0; j < 4; ++j) __builtin_amdgcn_raw_buffer_store_b128(as_u4(o[j]), rs_v, row + (4 * i + j) * plane, 0, 0);
    }
}

// ------------------------------------------------------------------------------------------------
// Y = A^T m A,  A^T = [[1,1,1,0],[0,1,-1,-1]], then the arithmetic of affine_act_pm on each of the tile's 2 x 2 output pixels
// (BatchNorm scale / shift, optional residual with its optional own affine, activation; csrc/affine_act.h), stored where the
// pixel is inside the map (odd H or W: the tile's second row / column is not).
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BLK)
wino_output_f32_kernel(const float* __restrict__ m, const float* __restrict__ scale, const float* __restrict__ shift,
                       const float* __restrict__ res, const float* __restrict__ rscale, const float* __restrict__ rshift,
                       float* __restrict__ out, const WinoGeom g, unsigned m_bytes, unsigned o_bytes, int q, unsigned total, float slope)
{
    const unsigned t = blockIdx.x * BLK + threadIdx.x;
    if (t >= total) return;
    const int tile = (int)(t / (unsigned)q), cq = (int)(t - (unsigned)tile * (unsigned)q);
    const int tx = tile % g.TW, ty = (tile / g.TW) % g.TH, b = tile / (g.TW * g.TH);
    const __amdgpu_buffer_rsrc_t rs_m = make_rsrc(m, m_bytes), rs_o = make_rsrc(out, o_bytes);
    const __amdgpu_buffer_rsrc_t rs_r = make_rsrc(res ? res : out, res ? o_bytes : 0u);

    int off[2][2];                                    // the tile's output pixels, OOB outside the map
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int y = 2 * ty + i, xx = 2 * tx + j;
            off[i][j] = (y < g.H && xx < g.W) ? (((b * g.H + y) * g.W + xx) * g.C + cq * 4) * 4 : OOB;
        }
    const int row = (tile * g.C + cq * 4) * 4, plane = g.Tp * g.C * 4;
    float4 mm[4][4], rr[2][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) mm[i][j] = as_f4(__builtin_amdgcn_raw_buffer_load_b128(rs_m, row + (4 * i + j) * plane, 0, 0));
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) rr[i][j] = as_f4(__builtin_amdgcn_raw_buffer_load_b128(rs_r, off[i][j], 0, 0));     // (no residual: zeros, unused)
    float s[4], sh[4], rs[4], rb[4];
    load_params<4>(scale, cq, s);
    load_params<4>(shift, cq, sh);
    if (rscale) {
        load_params<4>(rscale, cq, rs);
        load_params<4>(rshift, cq, rb);
    }

    float4 a[2][4];                                   // A^T m
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        a[0][j] = (mm[0][j] + mm[1][j]) + mm[2][j];
        a[1][j] = (mm[1][j] - mm[2][j]) - mm[3][j];
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const float4 y2[2] = {(a[i][0] + a[i][1]) + a[i][2], (a[i][1] - a[i][2]) - a[i][3]};      // (A^T m) A
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float v[4] = {y2[j].x, y2[j].y, y2[j].z, y2[j].w};
            const float r4[4] = {rr[i][j].x, rr[i][j].y, rr[i][j].z, rr[i][j].w};
            affine_act_unit<4>(v, s, sh, res ? r4 : nullptr, rscale != nullptr, rs, rb, slope);
            __builtin_amdgcn_raw_buffer_store_b128(as_u4(make_float4(v[0], v[1], v[2], v[3])), rs_o, off[i][j], 0, 0);
        }
    }
}

// ================================================================================================
// F(4x4,3x3) on the interpolation points 0, 1, -1, 2, -1/2: 6 x 6 windows at stride 4, 4 x 4 output tiles, 36 planes -- 2.25 multiplies
// per output where F(2x2) needs 4.  The rows of B^T are scaled to integers (their products are exact), the inverse scale sits in G
// (forward_pm.wino4_filter, applied once in float64).  Same layouts and conventions as above with
//     V [36][Tp][C]      U [36][O][C]      M [36][Tp][O]      T = B * ceil(H/4) * ceil(W/4),  plane 6u + v.
// A lane still owns 16 bytes of one tile: its 36 loads are all in flight before the first use (the transform runs in place, a column
// at a time, then a row at a time into the stores), which is what hides the latency at the two waves per SIMD the 36 float4 leave.
// ================================================================================================
__device__ __forceinline__ float4 operator*(float a, float4 b) { return make_float4(a * b.x, a * b.y, a * b.z, a * b.w); }

// t = B^T s,  B^T = [[2,3,-4,-3,2,0],[0,-2,-5,-1,2,0],[0,2,1,-5,2,0],[0,-1,-2,1,2,0],[0,2,-1,-2,1,0],[0,2,3,-4,-3,2]]
// (V: float4, or a narrower vector of channels -- the same expression per channel)
template <typename V>
__device__ __forceinline__ void wino4_bt(const V (&s)[6], V (&t)[6])
{
    t[0] = ((2.f * s[0] + 3.f * s[1]) - (4.f * s[2] + 3.f * s[3])) + 2.f * s[4];
    t[1] = (2.f * s[4] - s[3]) - (2.f * s[1] + 5.f * s[2]);
    t[2] = ((2.f * s[1] + s[2]) - 5.f * s[3]) + 2.f * s[4];
    t[3] = ((s[3] - s[1]) - 2.f * s[2]) + 2.f * s[4];
    t[4] = ((2.f * s[1] - s[2]) - 2.f * s[3]) + s[4];
    t[5] = ((2.f * s[1] + 3.f * s[2]) - (4.f * s[3] + 3.f * s[4])) + 2.f * s[5];
}

// t = A^T s,  A^T = [[1,1,1,1,1,0],[0,1,-1,2,-1/2,0],[0,1,1,4,1/4,0],[0,1,-1,8,-1/8,1]]
__device__ __forceinline__ void wino4_at(const float4 (&s)[6], float4 (&t)[4])
{
    const float4 p = s[1] + s[2], q = s[1] - s[2];
    t[0] = ((s[0] + p) + s[3]) + s[4];
    t[1] = (q + 2.f * s[3]) - .5f * s[4];
    t[2] = (p + 4.f * s[3]) + .25f * s[4];
    t[3] = ((q + 8.f * s[3]) - .125f * s[4]) + s[5];
}

// V = B^T d B of the 6 x 6 window whose top left pixel is (4 ty - 1, 4 tx - 1); rows T .. Tp - 1 of every plane are never written
__global__ void __launch_bounds__(BLK)
wino4_input_f32_kernel(const float* __restrict__ x, float* __restrict__ v, const WinoGeom g, unsigned x_bytes, unsigned v_bytes, int q,
                       unsigned total)
{
    const unsigned t = blockIdx.x * BLK + threadIdx.x;
    if (t >= total) return;
    const int tile = (int)(t / (unsigned)q), cq = (int)(t - (unsigned)tile * (unsigned)q);
    const int tx = tile % g.TW, ty = (tile / g.TW) % g.TH, b = tile / (g.TW * g.TH);
    const __amdgpu_buffer_rsrc_t rs_x = make_rsrc(x, x_bytes), rs_v = make_rsrc(v, v_bytes);

    float4 d[6][6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const int y = 4 * ty - 1 + i;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const int xx = 4 * tx - 1 + j;
            const bool in = y >= 0 && y < g.H && xx >= 0 && xx < g.W;
            const int off = in ? (((b * g.H + y) * g.W + xx) * g.C + cq * 4) * 4 : OOB;
            d[i][j] = as_f4(__builtin_amdgcn_raw_buffer_load_b128(rs_x, off, 0, 0));
        }
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) {                     // B^T d, in place
        const float4 s[6] = {d[0][j], d[1][j], d[2][j], d[3][j], d[4][j], d[5][j]};
        float4 r[6];
        wino4_bt(s, r);
#pragma unroll
        for (int i = 0; i < 6; ++i) d[i][j] = r[i];
    }
    const int row = (tile * g.C + cq * 4) * 4, plane = g.Tp * g.C * 4;      // bytes
#pragma unroll
    for (int i = 0; i < 6; ++i) {                     // (B^T d) B
        float4 o[6];
        wino4_bt(d[i], o);
#pragma unroll
        for (int j = 0; j < 6; ++j) __builtin_amdgcn_raw_buffer_store_b128(as_u4(o[j]), rs_v, row + (6 * i + j) * plane, 0, 0);
    }
}

// Y = A^T m A, then the arithmetic of affine_act_pm on each of the tile's 4 x 4 output pixels, stored where the pixel is inside the map
// (H or W no multiple of 4: the tile's last rows / columns are not)
__global__ void __launch_bounds__(BLK)
wino4_output_f32_kernel(const float* __restrict__ m, const float* __restrict__ scale, const float* __restrict__ shift,
                        const float* __restrict__ res, const float* __restrict__ rscale, const float* __restrict__ rshift,
                        float* __restrict__ out, const WinoGeom g, unsigned m_bytes, unsigned o_bytes, int q, unsigned total, float slope)
{
    const unsigned t = blockIdx.x * BLK + threadIdx.x;
    if (t >= total) return;
    const int tile = (int)(t / (unsigned)q), cq = (int)(t - (unsigned)tile * (unsigned)q);
    const int tx = tile % g.TW, ty = (tile / g.TW) % g.TH, b = tile / (g.TW * g.TH);
    const __amdgpu_buffer_rsrc_t rs_m = make_rsrc(m, m_bytes), rs_o = make_rsrc(out, o_bytes);
    const __amdgpu_buffer_rsrc_t rs_r = make_rsrc(res ? res : out, res ? o_bytes : 0u);

    const int row = (tile * g.C + cq * 4) * 4, plane = g.Tp * g.C * 4;
    float4 mm[6][6];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) mm[i][j] = as_f4(__builtin_amdgcn_raw_buffer_load_b128(rs_m, row + (6 * i + j) * plane, 0, 0));
    float s[4], sh[4], rs[4], rb[4];
    load_params<4>(scale, cq, s);
    load_params<4>(shift, cq, sh);
    if (rscale) {
        load_params<4>(rscale, cq, rs);
        load_params<4>(rshift, cq, rb);
    }

    float4 a[4][6];                                   // A^T m
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const float4 c[6] = {mm[0][j], mm[1][j], mm[2][j], mm[3][j], mm[4][j], mm[5][j]};
        float4 r[4];
        wino4_at(c, r);
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i][j] = r[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float4 y4[4];                                 // (A^T m) A
        wino4_at(a[i], y4);
        const int y = 4 * ty + i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int xx = 4 * tx + j;
            const int off = (y < g.H && xx < g.W) ? (((b * g.H + y) * g.W + xx) * g.C + cq * 4) * 4 : OOB;      // OOB: outside the map
            const float4 rr = as_f4(__builtin_amdgcn_raw_buffer_load_b128(rs_r, off, 0, 0));                    // (no residual: zeros, unused)
            float v[4] = {y4[j].x, y4[j].y, y4[j].z, y4[j].w};
            const float r4[4] = {rr.x, rr.y, rr.z, rr.w};
            affine_act_unit<4>(v, s, sh, res ? r4 : nullptr, rscale != nullptr, rs, rb, slope);
            __builtin_amdgcn_raw_buffer_store_b128(as_u4(make_float4(v[0], v[1], v[2], v[3])), rs_o, off, 0, 0);
        }
    }
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// geometry and the 2 GiB bound of every buffer a launch touches (offsets are 32-bit byte offsets into buffer descriptors);
// m = output tile edge: 2 (16 planes) or 4 (36 planes)
inline int geom(const char* who, int64_t B, int64_t H, int64_t W, int64_t C, int64_t Tp, WinoGeom& g, int m = 2)
{
    FFB6D_REQUIRE(B >= 0 && H >= 1 && W >= 1 && C >= 4 && C % 4 == 0, "%s: bad shape (channels must be a positive multiple of 4)", who);
    const int64_t TH = (H + m - 1) / m, TW = (W + m - 1) / m, T = B * TH * TW, planes = (m + 2) * (m + 2);
    FFB6D_REQUIRE(Tp >= T && Tp % 128 == 0, "%s: Tp must be the tile count %lld rounded up to a multiple of 128 or more (got %lld)", who,
                  (long long)T, (long long)Tp);
    FFB6D_REQUIRE(planes * Tp * C * 4 < (1LL << 31) - 16 && B * H * W * C * 4 < (1LL << 31) - 16 && T * (C / 4) < (1LL << 31),
                  "%s: a tensor of 2 GiB or more (the kernels address with 32-bit byte offsets)", who);
    g.H = (int)H; g.W = (int)W; g.C = (int)C; g.TH = (int)TH; g.TW = (int)TW; g.T = (int)T; g.Tp = (int)Tp;
    return FFB6D_OK;
}

inline int input_f32(const float* x, float* v, int64_t B, int64_t H, int64_t W, int64_t C, int64_t Tp, ffb6d_stream_t stream)
{
    WinoGeom g;
    if (const int rc = geom("wino_input", B, H, W, C, Tp, g)) return rc;
    if (g.T == 0) return FFB6D_OK;
    FFB6D_REQUIRE(x && v && al16(x) && al16(v), "wino_input: null or unaligned pointer");
    const unsigned total = (unsigned)g.T * (unsigned)(C / 4);
    hipLaunchKernelGGL(wino_input_f32_kernel, dim3((unsigned)ceil_div(total, BLK)), dim3(BLK), 0, as_stream(stream), x, v, g,
                       (unsigned)(B * H * W * C * 4), (unsigned)(16 * Tp * C * 4), (int)(C / 4), total);
    FFB6D_LAUNCH_CHECK();
    return FFB6D_OK;
}

inline int output_f32(const float* m, const float* scale, const float* shift, const float* res, const float* rscale,
                      const float* rshift, float* out, int64_t B, int64_t H, int64_t W, int64_t O, int64_t Tp, int act, float slope,
                      ffb6d_stream_t stream)
{
    WinoGeom g;
    if (const int rc = geom("wino_output", B, H, W, O, Tp, g)) return rc;
    FFB6D_REQUIRE(act >= 0 && act <= 2, "wino_output: act must be 0 (none), 1 (relu) or 2 (leaky/prelu with slope)");
    if (g.T == 0) return FFB6D_OK;
    FFB6D_REQUIRE(m && scale && shift && out && (rscale == nullptr) == (rshift == nullptr) && (!rscale || res), "wino_output: null pointer");
    FFB6D_REQUIRE(al16(m) && al16(out) && al16(res) && al16(scale) && al16(shift) && al16(rscale) && al16(rshift),
                  "wino_output: 16-byte aligned pointers expected");
    FFB6D_REQUIRE(out != res, "wino_output: the residual may not alias the output");
    const unsigned total = (unsigned)g.T * (unsigned)(O / 4);
    const float sl = act == 0 ? 1.f : (act == 1 ? 0.f : slope);
    hipLaunchKernelGGL(wino_output_f32_kernel, dim3((unsigned)ceil_div(total, BLK)), dim3(BLK), 0, as_stream(stream), m, scale, shift, res,
                       rscale, rshift, out, g, (unsigned)(16 * Tp * O * 4), (unsigned)(B * H * W * O * 4), (int)(O / 4), total, sl);
    FFB6D_LAUNCH_CHECK();
    return FFB6D_OK;
}

inline int input4_f32(const float* x, float* v, int64_t B, int64_t H, int64_t W, int64_t C, int64_t Tp, ffb6d_stream_t stream)
{
    WinoGeom g;
    if (const int rc = geom("wino4_input", B, H, W, C, Tp, g, 4)) return rc;
    if (g.T == 0) return FFB6D_OK;
    FFB6D_REQUIRE(x && v && al16(x) && al16(v), "wino4_input: null or unaligned pointer");
    const unsigned total = (unsigned)g.T * (unsigned)(C / 4);
    hipLaunchKernelGGL(wino4_input_f32_kernel, dim3((unsigned)ceil_div(total, BLK)), dim3(BLK), 0, as_stream(stream), x, v, g,
                       (unsigned)(B * H * W * C * 4), (unsigned)(36 * Tp * C * 4), (int)(C / 4), total);
    FFB6D_LAUNCH_CHECK();
    return FFB6D_OK;
}

inline int output4_f32(const float* m, const float* scale, const float* shift, const float* res, const float* rscale,
                       const float* rshift, float* out, int64_t B, int64_t H, int64_t W, int64_t O, int64_t Tp, int act, float slope,
                       ffb6d_stream_t stream)
{
    WinoGeom g;
    if (const int rc = geom("wino4_output", B, H, W, O, Tp, g, 4)) return rc;
    FFB6D_REQUIRE(act >= 0 && act <= 2, "wino4_output: act must be 0 (none), 1 (relu) or 2 (leaky/prelu with slope)");
    if (g.T == 0) return FFB6D_OK;
    FFB6D_REQUIRE(m && scale && shift && out && (rscale == nullptr) == (rshift == nullptr) && (!rscale || res), "wino4_output: null pointer");
    FFB6D_REQUIRE(al16(m) && al16(out) && al16(res) && al16(scale) && al16(shift) && al16(rscale) && al16(rshift),
                  "wino4_output: 16-byte aligned pointers expected");
    FFB6D_REQUIRE(out != res, "wino4_output: the residual may not alias the output");
    const unsigned total = (unsigned)g.T * (unsigned)(O / 4);
    const float sl = act == 0 ? 1.f : (act == 1 ? 0.f : slope);
    hipLaunchKernelGGL(wino4_output_f32_kernel, dim3((unsigned)ceil_div(total, BLK)), dim3(BLK), 0, as_stream(stream), m, scale, shift, res,
                       rscale, rshift, out, g, (unsigned)(36 * Tp * O * 4), (unsigned)(B * H * W * O * 4), (int)(O / 4), total, sl);
    FFB6D_LAUNCH_CHECK();
    return FFB6D_OK;
}

}  // namespace wino
}  // namespace ffb6d
