// ffb6d_amd/csrc/winograd_fused.h -- Winograd F(4x4,3x3) in ONE kernel for the narrow stride-1 3x3 convolutions of the colour trunk
// (64 and 128 input channels; fp32 inference): input transform -> 36 small GEMMs -> output transform -> BatchNorm / residual / activation,
//     out[B,H,W,O] = act(scale * conv3x3(x[B,H,W,C], pad 1) + shift + residual term),
// with the matrices, the plane order 6u + v and the filter U [36][O][C] of the three-kernel path (csrc/winograd.h, forward_pm.wino4_filter).
// On these maps that path is bound by the round trip of V and M through memory (2 x 2.25 maps each way); here V lives in LDS only and M
// in registers only, so a layer moves x, the residual and the output.
//
// A workgroup owns 16 consecutive tiles (b, ty, tx) and 16 * NW output channels, one wave per 16 channels:
//   * input transform, KC input channels at a time: a lane owns 16 bytes (4 channels) of one tile, 36 loads, B^T d B in registers as in
//     wino4_input_f32_kernel, 36 16-byte LDS stores to V[plane][tile][k].  The 16-byte units of a tile's row are XOR-swizzled with the
//     tile number so that the 16 tiles of a fragment read (same k, row stride a multiple of 128 bytes) fall into 16 different bank groups.
//   * multiply with v_mfma_f32_16x16x4_f32, channels on rows: per plane D[16 channels x 16 tiles] += U_plane[16 x k] V_plane[k x 16].  One
//     16-byte LDS read (B) and one 16-byte read of a row of U from L2 (A) feed 4 successive MFMAs: lane group g = l >> 4 holds k0 + 4g .. + 3
//     of both, MFMA t multiplies the four k = k0 + 4g + t (the order inside the sum is free as long as A and B agree).  The 36 x 4
//     accumulators persist across the K chunks.
//   * epilogue: in that instruction's C/D layout a lane holds the same (tile, 4 consecutive channels) in all 36 planes, so A^T m A is
//     lane-local: wino4_at twice, affine_act_unit, one 16-byte store per pixel.  The residual is requested before the arithmetic.
// Conventions of csrc/winograd.h: range-checked buffer descriptors, offsets from tile numbers only, pixels outside the map (and the
// tile slots past the last tile) at the out-of-range offset -- zero on load, dropped on store; any H, W.
#pragma once
#include "winograd.h"

namespace ffb6d {
namespace wino {

// SKIP: phases left out by the phase-removal builds of scripts/probes/wino4_phase_probe.hip (their results mean nothing; every launcher
// below instantiates SKIP = 0 only)
constexpr int SKIP_TRANSFORM = 1, SKIP_MFMA = 2, SKIP_U = 4, SKIP_EPILOGUE = 8;

// what a phase-removal build does with its accumulators instead of the epilogue: they stay live, nothing is stored (o_bytes is never 1)
__device__ __forceinline__ void keep_accumulators(const pm::f32x4 (&acc)[36], __amdgpu_buffer_rsrc_t rs_o, unsigned o_bytes)
{
    pm::f32x4 s = acc[0];
#pragma unroll
    for (int p = 1; p < 36; ++p) s += acc[p];
    if (o_bytes == 1u) __builtin_amdgcn_raw_buffer_store_b128(as_u4(make_float4(s[0], s[1], s[2], s[3])), rs_o, 0, 0, 0);
}

template <int NW, int KC, int SKIP = 0>
__global__ void __launch_bounds__(64 * NW)
wino4_conv_f32_kernel(const float* __restrict__ x, const float* __restrict__ u, const float* __restrict__ scale,
                      const float* __restrict__ shift, const float* __restrict__ res, const float* __restrict__ rscale,
                      const float* __restrict__ rshift, float* __restrict__ out, const WinoGeom g, int O, unsigned x_bytes, unsigned u_bytes,
                      unsigned o_bytes, float slope)
{
    __shared__ __attribute__((aligned(16))) float vlds[36 * 16 * KC];      // V [36][16 tiles][KC], 16-byte units swizzled
    constexpr int NT = 64 * NW, Q = KC / 4, TASKS = 16 * Q;
    static_assert(TASKS % NT == 0 && (Q == 8 || Q == 16), "a whole number of (tile, channel quad) tasks per thread");
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int jt = lane & 15, gq = lane >> 4;         // MFMA column (tile of the block) and k group / channel quad of the accumulators
    const int tile0 = (int)blockIdx.x * 16, o0 = ((int)blockIdx.y * NW + wave) * 16;
    const __amdgpu_buffer_rsrc_t rs_x = make_rsrc(x, x_bytes), rs_u = make_rsrc(u, u_bytes), rs_o = make_rsrc(out, o_bytes);
    const __amdgpu_buffer_rsrc_t rs_r = make_rsrc(res ? res : out, res ? o_bytes : 0u);
    float4* const v4 = reinterpret_cast<float4*>(vlds);

    pm::f32x4 acc[36];
#pragma unroll
    for (int p = 0; p < 36; ++p) acc[p] = pm::f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
    for (int kc0 = 0; kc0 < g.C; kc0 += KC) {
        if (kc0) __syncthreads();                     // the previous chunk's fragment reads are done
#pragma unroll 1
        for (int task = (SKIP & SKIP_TRANSFORM) ? TASKS : tid; task < TASKS; task += NT) {
            const int tl = task / Q, cq = task % Q, tile = tile0 + tl;
            const int tx = tile % g.TW, ty = (tile / g.TW) % g.TH, b = tile / (g.TW * g.TH);
            const bool live = tile < g.T;
            float4 d[6][6];
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                const int y = 4 * ty - 1 + i;
#pragma unroll
                for (int j = 0; j < 6; ++j) {
                    const int xx = 4 * tx - 1 + j;
                    const bool in = live && y >= 0 && y < g.H && xx >= 0 && xx < g.W;
                    const int off = in ? (((b * g.H + y) * g.W + xx) * g.C + kc0 + cq * 4) * 4 : OOB;
                    d[i][j] = as_f4(__builtin_amdgcn_raw_buffer_load_b128(rs_x, off, 0, 0));
                }
            }
#pragma unroll
            for (int j = 0; j < 6; ++j) {             // B^T d, in place
                const float4 s[6] = {d[0][j], d[1][j], d[2][j], d[3][j], d[4][j], d[5][j]};
                float4 r[6];
                wino4_bt(s, r);
#pragma unroll
                for (int i = 0; i < 6; ++i) d[i][j] = r[i];
            }
            float4* const dst = v4 + tl * Q + (cq ^ ((tl * Q) >> 4));
#pragma unroll
            for (int i = 0; i < 6; ++i) {             // (B^T d) B
                float4 o[6];
                wino4_bt(d[i], o);
#pragma unroll
                for (int j = 0; j < 6; ++j) dst[(6 * i + j) * 16 * Q] = o[j];
            }
        }
        __syncthreads();
        // 36 planes x KC / 16 k-steps in groups of 9 planes, double buffered: the fragment loads of group n + 1 (9 rows of U from L2, 9 LDS
        // reads) are issued before the 36 MFMAs of group n, which cover their latency (the scheduling barriers keep that order: left to
        // itself the compiler sinks every load to its use and waits for it with nothing else in flight -- measured 4x slower)
        constexpr int GP = 9, NG = (KC / 16) * (36 / GP);
        const int a_base = ((o0 + jt) * g.C + kc0 + 4 * gq) * 4, a_plane = O * g.C * 4;
        const int swz = (jt * Q) >> 4;
        u32x4 av[2][GP];
        float4 bv[2][GP];
        auto load_group = [&](int n, u32x4 (&a)[GP], float4 (&b)[GP]) {
            const int ks = n / (36 / GP), p0 = (n % (36 / GP)) * GP;
            const float4* const bsrc = v4 + jt * Q + ((4 * ks + gq) ^ swz);
#pragma unroll
            for (int i = 0; i < GP; ++i) {
                if (!(SKIP & SKIP_U) || n < 2) a[i] = __builtin_amdgcn_raw_buffer_load_b128(rs_u, a_base + 64 * ks + (p0 + i) * a_plane, 0, 0);
                b[i] = bsrc[(p0 + i) * 16 * Q];
            }
        };
        load_group(0, av[0], bv[0]);
#pragma unroll
        for (int n = 0; n < NG; ++n) {
            if (n + 1 < NG) load_group(n + 1, av[(n + 1) & 1], bv[(n + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
            const int p0 = (n % (36 / GP)) * GP;
#pragma unroll
            for (int i = 0; i < GP; ++i) {
                const u32x4 a = av[n & 1][i];
                const float4 b = bv[n & 1][i];
                if constexpr (SKIP & SKIP_MFMA) {
                    pm::use_here(a[0] ^ a[1] ^ a[2] ^ a[3]);
                    pm::use_here(__float_as_uint(b.x) ^ __float_as_uint(b.y) ^ __float_as_uint(b.z) ^ __float_as_uint(b.w));
                    continue;
                }
                acc[p0 + i] = pm::mfma_16x16x4(__uint_as_float(a[0]), b.x, acc[p0 + i]);
                acc[p0 + i] = pm::mfma_16x16x4(__uint_as_float(a[1]), b.y, acc[p0 + i]);
                acc[p0 + i] = pm::mfma_16x16x4(__uint_as_float(a[2]), b.z, acc[p0 + i]);
                acc[p0 + i] = pm::mfma_16x16x4(__uint_as_float(a[3]), b.w, acc[p0 + i]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    if constexpr (SKIP & SKIP_EPILOGUE) {
        keep_accumulators(acc, rs_o, o_bytes);
        return;
    }
    // epilogue: this lane's tile and its 4 output channels o0 + 4 gq .. + 3
    const int tile = tile0 + jt, cq = (o0 >> 2) + gq;
    const int tx = tile % g.TW, ty = (tile / g.TW) % g.TH, b = tile / (g.TW * g.TH);
    const bool live = tile < g.T;
    int off[4][4];
    float4 rr[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int y = 4 * ty + i, xx = 4 * tx + j;
            off[i][j] = (live && y < g.H && xx < g.W) ? (((b * g.H + y) * g.W + xx) * O + cq * 4) * 4 : OOB;       // OOB: outside the map
            rr[i][j] = as_f4(__builtin_amdgcn_raw_buffer_load_b128(rs_r, off[i][j], 0, 0));                        // (no residual: zeros, unused)
        }
    float sc[4], sh[4], rs[4], rb[4];
    load_params<4>(scale, cq, sc);
    load_params<4>(shift, cq, sh);
    if (rscale) {
        load_params<4>(rscale, cq, rs);
        load_params<4>(rshift, cq, rb);
    }
    float4 a[4][6];                                   // A^T m
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        float4 c[6], r[4];
#pragma unroll
        for (int i = 0; i < 6; ++i) c[i] = make_float4(acc[6 * i + j][0], acc[6 * i + j][1], acc[6 * i + j][2], acc[6 * i + j][3]);
        wino4_at(c, r);
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i][j] = r[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float4 y4[4];                                 // (A^T m) A
        wino4_at(a[i], y4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float v[4] = {y4[j].x, y4[j].y, y4[j].z, y4[j].w};
            const float r4[4] = {rr[i][j].x, rr[i][j].y, rr[i][j].z, rr[i][j].w};
            affine_act_unit<4>(v, sc, sh, res ? r4 : nullptr, rscale != nullptr, rs, rb, slope);
            __builtin_amdgcn_raw_buffer_store_b128(as_u4(make_float4(v[0], v[1], v[2], v[3])), rs_o, off[i][j], 0, 0);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// The same operator with TWO workgroups resident on a CU (two waves per SIMD), so that one workgroup's transform, barrier, epilogue
// and load waits run under the other's MFMAs: 4 waves x 16 tiles x 64 output channels as above, but within 256 registers per lane
// and half the LDS (KC = 32: 73728 bytes).  What that forces:
//   * input transform: a lane owns 8 bytes (2 channels) of one tile -- 256 (tile, channel pair) tasks, one per thread and chunk; 36
//     8-byte loads, 72 registers, wino4_bt on the pair (its unused half is dead code), 36 8-byte LDS stores.  Rows of V are 128 bytes; the
//     16-byte units keep the swizzle of the 2-wave shape (unit ^ (tile >> 1): two tiles span the 64 banks, 8 units each), so the 16
//     tiles of a fragment read still hit 16 bank groups and the 16 lanes of a tile's row write one whole row.
//   * multiply: groups of GP = 4 planes (2 x 4 x 8 fragment registers), the next group requested before the 16 MFMAs of the current one.
//     Every accumulator receives its k-steps in the order of the kernel above (chunk, then k-step, the four k of a lane group per
//     MFMA), so the two kernels agree bit for bit.
//   * epilogue: A^T m a column at a time (the accumulators die as it goes), then a row of pixels at a time with that row's residual
//     requested one row ahead.
// ------------------------------------------------------------------------------------------------
typedef float f32x2 __attribute__((ext_vector_type(2)));

template <int SKIP = 0>
__global__ void __launch_bounds__(256, 2)
wino4_conv2_f32_kernel(const float* __restrict__ x, const float* __restrict__ u, const float* __restrict__ scale,
                       const float* __restrict__ shift, const float* __restrict__ res, const float* __restrict__ rscale,
                       const float* __restrict__ rshift, float* __restrict__ out, const WinoGeom g, int O, unsigned x_bytes, unsigned u_bytes,
                       unsigned o_bytes, float slope)
{
    constexpr int KC = 32, Q = KC / 4, GP = 4, NGP = 36 / GP, NG = (KC / 16) * NGP;
    __shared__ __attribute__((aligned(16))) float vlds[36 * 16 * KC];      // V [36][16 tiles][KC], 16-byte units swizzled
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int jt = lane & 15, gq = lane >> 4;
    const int tile0 = (int)blockIdx.x * 16, o0 = ((int)blockIdx.y * 4 + wave) * 16;
    const __amdgpu_buffer_rsrc_t rs_x = make_rsrc(x, x_bytes), rs_u = make_rsrc(u, u_bytes), rs_o = make_rsrc(out, o_bytes);
    const __amdgpu_buffer_rsrc_t rs_r = make_rsrc(res ? res : out, res ? o_bytes : 0u);
    float4* const v4 = reinterpret_cast<float4*>(vlds);

    pm::f32x4 acc[36];
#pragma unroll
    for (int p = 0; p < 36; ++p) acc[p] = pm::f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
    for (int kc0 = 0; kc0 < g.C; kc0 += KC) {
        if (kc0) __syncthreads();                     // the previous chunk's fragment reads are done
        if constexpr (!(SKIP & SKIP_TRANSFORM)) {
            // this thread's tile slot and channel pair; opaque: the 36 window offsets are computed here, chunk by chunk, not kept across the loop
            const int tl = tid >> 4, cp = tid & 15, tile = pm::opaque(tile0 + tl);
            const int tx = tile % g.TW, ty = (tile / g.TW) % g.TH, b = tile / (g.TW * g.TH);
            const bool live = tile < g.T;
            f32x2 d[6][6];
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                const int y = 4 * ty - 1 + i;
#pragma unroll
                for (int j = 0; j < 6; ++j) {
                    const int xx = 4 * tx - 1 + j;
                    const bool in = live && y >= 0 && y < g.H && xx >= 0 && xx < g.W;
                    const int off = in ? (((b * g.H + y) * g.W + xx) * g.C + kc0 + cp * 2) * 4 : OOB;
                    d[i][j] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rs_x, off, 0, 0));
                }
                __builtin_amdgcn_sched_barrier(0);    // a row's 6 offsets at a time: 36 of them next to the window do not fit
            }
#pragma unroll
            for (int j = 0; j < 6; ++j) {             // B^T d, in place
                const f32x2 s[6] = {d[0][j], d[1][j], d[2][j], d[3][j], d[4][j], d[5][j]};
                f32x2 r[6];
                wino4_bt(s, r);
#pragma unroll
                for (int i = 0; i < 6; ++i) d[i][j] = r[i];
            }
            f32x2* const dst = reinterpret_cast<f32x2*>(v4 + tl * Q + ((cp >> 1) ^ (tl >> 1))) + (cp & 1);
#pragma unroll
            for (int i = 0; i < 6; ++i) {             // (B^T d) B
                f32x2 o[6];
                wino4_bt(d[i], o);
#pragma unroll
                for (int j = 0; j < 6; ++j) dst[(6 * i + j) * 16 * Q * 2] = o[j];
            }
        }
        __syncthreads();
        const int a_base = ((o0 + jt) * g.C + kc0 + 4 * gq) * 4, a_plane = O * g.C * 4;
        const int swz = jt >> 1;
        u32x4 av[2][GP];
        float4 bv[2][GP];
        auto load_group = [&](int n, u32x4 (&a)[GP], float4 (&b)[GP]) {
            const int ks = n / NGP, p0 = (n % NGP) * GP;
            const float4* const bsrc = v4 + jt * Q + ((4 * ks + gq) ^ swz);
#pragma unroll
            for (int i = 0; i < GP; ++i) {
                if (!(SKIP & SKIP_U) || n < 2) a[i] = __builtin_amdgcn_raw_buffer_load_b128(rs_u, a_base, 64 * ks + (p0 + i) * a_plane, 0);      // plane, k-step: scalar
                b[i] = bsrc[(p0 + i) * 16 * Q];
            }
        };
        load_group(0, av[0], bv[0]);
#pragma unroll
        for (int n = 0; n < NG; ++n) {
            if (n + 1 < NG) load_group(n + 1, av[(n + 1) & 1], bv[(n + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
            const int p0 = (n % NGP) * GP;
#pragma unroll
            for (int i = 0; i < GP; ++i) {
                const u32x4 a = av[n & 1][i];
                const float4 b = bv[n & 1][i];
                if constexpr (SKIP & SKIP_MFMA) {
                    pm::use_here(a[0] ^ a[1] ^ a[2] ^ a[3]);
                    pm::use_here(__float_as_uint(b.x) ^ __float_as_uint(b.y) ^ __float_as_uint(b.z) ^ __float_as_uint(b.w));
                    continue;
                }
                acc[p0 + i] = pm::mfma_16x16x4(__uint_as_float(a[0]), b.x, acc[p0 + i]);
                acc[p0 + i] = pm::mfma_16x16x4(__uint_as_float(a[1]), b.y, acc[p0 + i]);
                acc[p0 + i] = pm::mfma_16x16x4(__uint_as_float(a[2]), b.z, acc[p0 + i]);
                acc[p0 + i] = pm::mfma_16x16x4(__uint_as_float(a[3]), b.w, acc[p0 + i]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    if constexpr (SKIP & SKIP_EPILOGUE) {
        keep_accumulators(acc, rs_o, o_bytes);
        return;
    }
    // epilogue: this lane's tile and its 4 output channels o0 + 4 gq .. + 3
    const int tile = tile0 + jt, cq = (o0 >> 2) + gq;
    const int tx = tile % g.TW, ty = (tile / g.TW) % g.TH, b = tile / (g.TW * g.TH);
    const bool live = tile < g.T;
    auto pixel = [&](int i, int j) {                  // byte offset of output pixel (i, j) of the tile, OOB outside the map
        const int y = 4 * ty + i, xx = 4 * tx + j;
        return (live && y < g.H && xx < g.W) ? (((b * g.H + y) * g.W + xx) * O + cq * 4) * 4 : OOB;
    };
    float4 rr[2][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) rr[0][j] = as_f4(__builtin_amdgcn_raw_buffer_load_b128(rs_r, pixel(0, j), 0, 0));     // (no residual: zeros, unused)
    float sc[4], sh[4], rs[4], rb[4];
    load_params<4>(scale, cq, sc);
    load_params<4>(shift, cq, sh);
    if (rscale) {
        load_params<4>(rscale, cq, rs);
        load_params<4>(rshift, cq, rb);
    }
    float4 a[4][6];                                   // A^T m
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        float4 c[6], r[4];
#pragma unroll
        for (int i = 0; i < 6; ++i) c[i] = make_float4(acc[6 * i + j][0], acc[6 * i + j][1], acc[6 * i + j][2], acc[6 * i + j][3]);
        wino4_at(c, r);
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i][j] = r[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (i + 1 < 4) {
#pragma unroll
            for (int j = 0; j < 4; ++j) rr[(i + 1) & 1][j] = as_f4(__builtin_amdgcn_raw_buffer_load_b128(rs_r, pixel(i + 1, j), 0, 0));
        }
        float4 y4[4];                                 // (A^T m) A
        wino4_at(a[i], y4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float v[4] = {y4[j].x, y4[j].y, y4[j].z, y4[j].w};
            const float4 r = rr[i & 1][j];
            const float r4[4] = {r.x, r.y, r.z, r.w};
            affine_act_unit<4>(v, sc, sh, res ? r4 : nullptr, rscale != nullptr, rs, rb, slope);
            __builtin_amdgcn_raw_buffer_store_b128(as_u4(make_float4(v[0], v[1], v[2], v[3])), rs_o, pixel(i, j), 0, 0);
        }
    }
}

template <int NW, int KC>
inline int launch_conv4(const float* x, const float* u, const float* scale, const float* shift, const float* res, const float* rscale,
                        const float* rshift, float* out, const WinoGeom& g, int O, unsigned x_bytes, unsigned u_bytes, unsigned o_bytes,
                        float sl, hipStream_t st)
{
    hipLaunchKernelGGL((wino4_conv_f32_kernel<NW, KC>), dim3((unsigned)ceil_div(g.T, 16), (unsigned)(O / (16 * NW))), dim3(64 * NW), 0, st,
                       x, u, scale, shift, res, rscale, rshift, out, g, O, x_bytes, u_bytes, o_bytes, sl);
    FFB6D_LAUNCH_CHECK();
    return FFB6D_OK;
}

inline int launch_conv4_2(const float* x, const float* u, const float* scale, const float* shift, const float* res, const float* rscale,
                          const float* rshift, float* out, const WinoGeom& g, int O, unsigned x_bytes, unsigned u_bytes, unsigned o_bytes,
                          float sl, hipStream_t st)
{
    hipLaunchKernelGGL(wino4_conv2_f32_kernel<0>, dim3((unsigned)ceil_div(g.T, 16), (unsigned)(O / 64)), dim3(256), 0, st, x, u, scale, shift,
                       res, rscale, rshift, out, g, O, x_bytes, u_bytes, o_bytes, sl);
    FFB6D_LAUNCH_CHECK();
    return FFB6D_OK;
}

// the automatic form per (C, O).  Alone on the chip, median of five rounds of 50 launches [smallest, largest], microseconds
// (profiles/winograd_narrow2_layers.jsonl), form 1 against form 3:
//     64 ->  64 on 8 x 120 x 160:   86.4 [ 86.3,  90.2]    74.6 [ 74.5,  74.8]
//    128 -> 128 on 8 x  60 x  80:   97.9 [ 97.7,  99.0]    84.4 [ 84.3,  84.5]
//    128 -> 256 on 8 x  60 x  80:  148.5 [148.4, 148.6]   132.4 [132.3, 132.6]
// Form 3 wins by 12 - 16 us where the rounds spread by 0.2 - 3.9; the widths that were not measured (64 -> 128, 64 -> 256, 128 -> 64: no
// layer of the network has them) stay on form 1.
inline int conv4_form(int64_t C, int64_t O)
{
    return (C == 64 && O == 64) || (C == 128 && (O == 128 || O == 256)) ? 3 : 1;
}

// form: 0 = the measured choice, 1 = 4 waves x 64-channel chunks (one workgroup per CU), 2 = 2 waves x 32-channel chunks (two per CU,
// one wave per SIMD), 3 = 4 waves x 32-channel chunks within 256 registers (two per CU, two waves per SIMD)
inline int conv4_f32(const float* x, const float* u, const float* scale, const float* shift, const float* res, const float* rscale,
                     const float* rshift, float* out, int64_t B, int64_t H, int64_t W, int64_t C, int64_t O, int act, float slope, int form,
                     ffb6d_stream_t stream)
{
    FFB6D_REQUIRE(B >= 0 && H >= 1 && W >= 1, "wino4_conv: bad shape");
    FFB6D_REQUIRE((C == 64 || C == 128) && (O == 64 || O == 128 || O == 256),
                  "wino4_conv: built for 64 or 128 input channels and 64, 128 or 256 output channels (got %lld -> %lld)", (long long)C,
                  (long long)O);
    FFB6D_REQUIRE(act >= 0 && act <= 2, "wino4_conv: act must be 0 (none), 1 (relu) or 2 (leaky/prelu with slope)");
    FFB6D_REQUIRE(form >= 0 && form <= 3, "wino4_conv: form must be 0 (automatic), 1, 2 or 3");
    const int64_t TH = (H + 3) / 4, TW = (W + 3) / 4, T = B * TH * TW;
    FFB6D_REQUIRE(B * H * W * C * 4 < (1LL << 31) - 16 && B * H * W * O * 4 < (1LL << 31) - 16 && T + 16 < (1LL << 31),
                  "wino4_conv: a tensor of 2 GiB or more (the kernel addresses with 32-bit byte offsets)");
    if (T == 0) return FFB6D_OK;
    FFB6D_REQUIRE(x && u && scale && shift && out && (rscale == nullptr) == (rshift == nullptr) && (!rscale || res), "wino4_conv: null pointer");
    FFB6D_REQUIRE(al16(x) && al16(u) && al16(out) && al16(res) && al16(scale) && al16(shift) && al16(rscale) && al16(rshift),
                  "wino4_conv: 16-byte aligned pointers expected");
    FFB6D_REQUIRE(out != res && out != x, "wino4_conv: the output may alias neither the residual nor the input");
    WinoGeom g;
    g.H = (int)H; g.W = (int)W; g.C = (int)C; g.TH = (int)TH; g.TW = (int)TW; g.T = (int)T; g.Tp = 0;
    const float sl = act == 0 ? 1.f : (act == 1 ? 0.f : slope);
    const unsigned xb = (unsigned)(B * H * W * C * 4), ub = (unsigned)(36 * O * C * 4), ob = (unsigned)(B * H * W * O * 4);
    if (form == 0) form = conv4_form(C, O);
    if (form == 3)
        return launch_conv4_2(x, u, scale, shift, res, rscale, rshift, out, g, (int)O, xb, ub, ob, sl, as_stream(stream));
    if (form == 1)
        return launch_conv4<4, 64>(x, u, scale, shift, res, rscale, rshift, out, g, (int)O, xb, ub, ob, sl, as_stream(stream));
    return launch_conv4<2, 32>(x, u, scale, shift, res, rscale, rshift, out, g, (int)O, xb, ub, ob, sl, as_stream(stream));
}

}  // namespace wino
}  // namespace ffb6d
