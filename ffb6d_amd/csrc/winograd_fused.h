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

template <int NW, int KC>
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
        for (int task = tid; task < TASKS; task += NT) {
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
                a[i] = __builtin_amdgcn_raw_buffer_load_b128(rs_u, a_base + 64 * ks + (p0 + i) * a_plane, 0, 0);
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
                acc[p0 + i] = pm::mfma_16x16x4(__uint_as_float(a[0]), b.x, acc[p0 + i]);
                acc[p0 + i] = pm::mfma_16x16x4(__uint_as_float(a[1]), b.y, acc[p0 + i]);
                acc[p0 + i] = pm::mfma_16x16x4(__uint_as_float(a[2]), b.z, acc[p0 + i]);
                acc[p0 + i] = pm::mfma_16x16x4(__uint_as_float(a[3]), b.w, acc[p0 + i]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
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

// form: 0 = the measured choice, 1 = 4 waves x 64-channel chunks (one workgroup per CU), 2 = 2 waves x 32-channel chunks (two per CU)
inline int conv4_f32(const float* x, const float* u, const float* scale, const float* shift, const float* res, const float* rscale,
                     const float* rshift, float* out, int64_t B, int64_t H, int64_t W, int64_t C, int64_t O, int act, float slope, int form,
                     ffb6d_stream_t stream)
{
    FFB6D_REQUIRE(B >= 0 && H >= 1 && W >= 1, "wino4_conv: bad shape");
    FFB6D_REQUIRE((C == 64 || C == 128) && (O == 64 || O == 128 || O == 256),
                  "wino4_conv: built for 64 or 128 input channels and 64, 128 or 256 output channels (got %lld -> %lld)", (long long)C,
                  (long long)O);
    FFB6D_REQUIRE(act >= 0 && act <= 2, "wino4_conv: act must be 0 (none), 1 (relu) or 2 (leaky/prelu with slope)");
    FFB6D_REQUIRE(form >= 0 && form <= 2, "wino4_conv: form must be 0 (automatic), 1 or 2");
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
    if (form == 0) form = 1;
    if (form == 1)
        return launch_conv4<4, 64>(x, u, scale, shift, res, rscale, rshift, out, g, (int)O, xb, ub, ob, sl, as_stream(stream));
    return launch_conv4<2, 32>(x, u, scale, shift, res, rscale, rshift, out, g, (int)O, xb, ub, ob, sl, as_stream(stream));
}

}  // namespace wino
}  // namespace ffb6d
