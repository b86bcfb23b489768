// ffb6d_amd/csrc/train_data.hip -- the arithmetic of a training sample on the device (include/ffb6d_train.h).
//
//   pose_targets_kernel: one workgroup = (frame, 128 points).  Every workgroup transforms the frame's O * (K + 1) mesh
//     points in double into LDS (a few hundred 3-term dot products), stages its points' coordinates and matched slot in LDS,
//     then writes the flat [128, K, 3] offset rows with one thread per output float: consecutive lanes, consecutive
//     addresses.  The workgroups of point tile 0 also write the per-object rows.
//   hsv_kernel: elementwise, 4 pixels per thread (one 4-byte word per plane when H*W is a multiple of 4); the two
//     fixed-point division tables of OpenCV's RGB2HSV_b are built in LDS per workgroup.
//   stencil_kernel: one workgroup = (frame, 64 x 16 output tile), 4 horizontally adjacent pixels per thread.  The tile plus
//     the frame's halo (<= 15 px; columns staged 16 px either side so that every staged word is 4-byte aligned) is loaded
//     into LDS as 4-byte words (BORDER_REFLECT_101 resolved while loading: words that straddle the image edge are gathered
//     byte by byte), the per-frame tap list is applied, the noise of the pass added, and 4 pixels stored as one word.
//   add_real_back_kernel: elementwise, 4 pixels per thread.
#include <climits>
#include <cmath>

#include "common.h"
#include "ffb6d_train.h"

namespace {

constexpr int kThreads = 256;

// ---------------------------------------------------------------------------------------------------------------------
// pose targets
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kPts = 128;                   // points per workgroup
constexpr int kMaxK = 64, kMaxO = 64;
constexpr int kMaxXf = 1024;                // O * (K + 1) transformed points staged in LDS

__device__ __forceinline__ double rt_at(const void* RTs, int rts_f64, int64_t i)
{
    return rts_f64 ? static_cast<const double*>(RTs)[i] : static_cast<double>(static_cast<const float*>(RTs)[i]);
}

__global__ __launch_bounds__(kThreads) void pose_targets_kernel(
    const float* __restrict__ cld, const void* __restrict__ choose, int choose_i64, const void* __restrict__ label_img,
    int label_u8, const int* __restrict__ cls_ids, const void* __restrict__ RTs, int rts_f64,
    const float* __restrict__ mesh_kps, const float* __restrict__ mesh_ctr, int n_cls, int64_t N, int64_t HW, int O, int K,
    int* __restrict__ labels, float* __restrict__ kp_ofst, float* __restrict__ ctr_ofst, float* __restrict__ kp_3ds,
    float* __restrict__ ctr_3ds, float* __restrict__ RTs_out, int* __restrict__ cls_out)
{
    __shared__ double xf[kMaxXf * 3];       // [O][K+1][3]: keypoints, then the centre
    __shared__ int cls_s[kMaxO];
    __shared__ float cld_s[kPts * 3];
    __shared__ int match_s[kPts];
    const int b = blockIdx.y;
    const int tid = threadIdx.x;
    const int64_t n0 = static_cast<int64_t>(blockIdx.x) * kPts;
    const int np = N - n0 >= kPts ? kPts : N - n0 > 0 ? static_cast<int>(N - n0) : 0;
    const int K1 = K + 1;

    for (int o = tid; o < O; o += kThreads) {
        const int c = cls_ids[static_cast<int64_t>(b) * O + o];
        cls_s[o] = (c >= 1 && c < n_cls) ? c : 0;           // anything else is an empty slot: never an index
    }
    __syncthreads();

    for (int i = tid; i < O * K1; i += kThreads) {
        const int o = i / K1, k = i - o * K1;
        const int c = cls_s[o];
        double p[3] = {0.0, 0.0, 0.0};
        if (c != 0) {
            const float* m = k < K ? mesh_kps + (static_cast<int64_t>(c) * K + k) * 3 : mesh_ctr + static_cast<int64_t>(c) * 3;
            const double m0 = m[0], m1 = m[1], m2 = m[2];
            const int64_t rt = (static_cast<int64_t>(b) * O + o) * 12;
#pragma unroll
            for (int j = 0; j < 3; ++j)
                p[j] = ((m0 * rt_at(RTs, rts_f64, rt + 4 * j) + m1 * rt_at(RTs, rts_f64, rt + 4 * j + 1)) +
                        m2 * rt_at(RTs, rts_f64, rt + 4 * j + 2)) + rt_at(RTs, rts_f64, rt + 4 * j + 3);
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) xf[i * 3 + j] = p[j];
        if (blockIdx.x == 0) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                if (k < K) kp_3ds[((static_cast<int64_t>(b) * O + o) * K + k) * 3 + j] = static_cast<float>(p[j]);
                else ctr_3ds[(static_cast<int64_t>(b) * O + o) * 3 + j] = static_cast<float>(p[j]);
            }
        }
    }
    if (blockIdx.x == 0) {
        for (int i = tid; i < O * 12; i += kThreads) {
            const int64_t at = static_cast<int64_t>(b) * O * 12 + i;
            RTs_out[at] = cls_s[i / 12] != 0 ? static_cast<float>(rt_at(RTs, rts_f64, at)) : 0.f;
        }
        for (int o = tid; o < O; o += kThreads) cls_out[static_cast<int64_t>(b) * O + o] = cls_s[o];
    }

    const int64_t row0 = static_cast<int64_t>(b) * N + n0;
    for (int i = tid; i < np * 3; i += kThreads) cld_s[i] = cld[row0 * 3 + i];
    for (int p = tid; p < np; p += kThreads) {
        const int64_t idx = choose_i64 ? static_cast<const int64_t*>(choose)[row0 + p]
                                       : static_cast<int64_t>(static_cast<const int*>(choose)[row0 + p]);
        int lab = 0;
        if (idx >= 0 && idx < HW) {
            const int64_t at = static_cast<int64_t>(b) * HW + idx;
            lab = label_u8 ? static_cast<int>(static_cast<const uint8_t*>(label_img)[at]) : static_cast<const int*>(label_img)[at];
        }
        labels[row0 + p] = lab;
        int m = -1;
        if (lab >= 1)
            for (int o = 0; o < O; ++o)
                if (cls_s[o] == lab) m = o;                    // the last slot of the class wins (ycb_dataset.py:385)
        match_s[p] = m;
    }
    __syncthreads();

    const int row = K * 3;
    float* kp_dst = kp_ofst + row0 * row;
    for (int i = tid; i < np * row; i += kThreads) {
        const int p = i / row, r = i - p * row, k = r / 3, j = r - k * 3;
        const int m = match_s[p];
        kp_dst[i] = m >= 0 ? static_cast<float>(static_cast<double>(cld_s[p * 3 + j]) - xf[(m * K1 + k) * 3 + j]) : 0.f;
    }
    float* ctr_dst = ctr_ofst + row0 * 3;
    for (int i = tid; i < np * 3; i += kThreads) {
        const int p = i / 3, j = i - p * 3;
        const int m = match_s[p];
        ctr_dst[i] = m >= 0 ? static_cast<float>(static_cast<double>(cld_s[i]) - xf[(m * K1 + K) * 3 + j]) : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// HSV jitter
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int sat_u8(float x)          // saturate_cast<uchar>(float): cvRound (half to even), clamp
{
    const float r = rintf(x);
    return r < 0.f ? 0 : r > 255.f ? 255 : static_cast<int>(r);
}

__device__ __forceinline__ void hsv_px(int b, int g, int r, double fs, double fv, const int* sdiv, const int* hdiv,
                                       int& ob, int& og, int& orr)
{
    int v = max(max(b, g), r);
    const int vmin = min(min(b, g), r);
    const int diff = v - vmin;
    const int vr = v == r ? -1 : 0, vg = v == g ? -1 : 0;
    int s = (diff * sdiv[v] + (1 << 11)) >> 12;
    int h = (vr & (g - b)) + (~vr & ((vg & (b - r + 2 * diff)) + ((~vg) & (r - g + 4 * diff))));
    h = (h * hdiv[diff] + (1 << 11)) >> 12;
    h += h < 0 ? 180 : 0;
    s = min(255, static_cast<int>(floor(static_cast<double>(s) * fs)));
    v = min(255, static_cast<int>(floor(static_cast<double>(v) * fv)));

    const float S = static_cast<float>(s) * (1.f / 255.f), V = static_cast<float>(v) * (1.f / 255.f);
    float fb, fg, fr;
    if (S == 0.f) {
        fb = fg = fr = V;
    } else {
        float H = static_cast<float>(h) * (6.f / 180.f);
        if (H < 0.f) do H += 6.f; while (H < 0.f);
        else if (H >= 6.f) do H -= 6.f; while (H >= 6.f);
        int sector = static_cast<int>(floorf(H));
        H -= static_cast<float>(sector);
        if (sector < 0 || sector >= 6) { sector = 0; H = 0.f; }
        float tab[4];
        tab[0] = V;
        tab[1] = V * (1.f - S);
        tab[2] = V * (1.f - S * H);
        tab[3] = V * (1.f - S * (1.f - H));
        // sector_data of color_hsv: {1,3,0},{1,0,2},{3,0,1},{0,2,1},{0,1,3},{2,1,0} as (b, g, r), one nibble per sector
        const int sb = (0x200311 >> (4 * sector)) & 0xf;   // sectors 0..5: 1,1,3,0,0,2
        const int sg = (0x112003 >> (4 * sector)) & 0xf;   // 3,0,0,2,1,1
        const int sr = (0x031120 >> (4 * sector)) & 0xf;   // 0,2,1,1,3,0
        fb = tab[sb]; fg = tab[sg]; fr = tab[sr];
    }
    ob = sat_u8(fb * 255.f);
    og = sat_u8(fg * 255.f);
    orr = sat_u8(fr * 255.f);
}

template <bool kVec>
__global__ __launch_bounds__(kThreads) void hsv_kernel(const uint8_t* __restrict__ in, const double* __restrict__ fs_fv,
                                                       uint8_t* __restrict__ out, int64_t HW)
{
    __shared__ int sdiv[256], hdiv[256];
    const int tid = threadIdx.x;
    if (tid == 0) {
        sdiv[0] = hdiv[0] = 0;
    } else {
        sdiv[tid] = static_cast<int>(rint((255 << 12) / static_cast<double>(tid)));
        hdiv[tid] = static_cast<int>(rint((180 << 12) / (6.0 * tid)));
    }
    __syncthreads();
    const int b = blockIdx.y;
    const double fs = fs_fv[2 * b], fv = fs_fv[2 * b + 1];
    const int64_t p0 = (static_cast<int64_t>(blockIdx.x) * kThreads + tid) * 4;
    if (p0 >= HW) return;
    const uint8_t* src = in + static_cast<int64_t>(b) * 3 * HW;
    uint8_t* dst = out + static_cast<int64_t>(b) * 3 * HW;
    const bool on = fs >= 0.0;
    if (kVec) {
        uint32_t w[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) w[c] = *reinterpret_cast<const uint32_t*>(src + c * HW + p0);
        uint32_t o[3] = {0u, 0u, 0u};
        if (on) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                int ob, og, orr;
                hsv_px((w[0] >> (8 * q)) & 0xff, (w[1] >> (8 * q)) & 0xff, (w[2] >> (8 * q)) & 0xff, fs, fv, sdiv, hdiv, ob, og, orr);
                o[0] |= static_cast<uint32_t>(ob) << (8 * q);
                o[1] |= static_cast<uint32_t>(og) << (8 * q);
                o[2] |= static_cast<uint32_t>(orr) << (8 * q);
            }
        } else {
            o[0] = w[0]; o[1] = w[1]; o[2] = w[2];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<uint32_t*>(dst + c * HW + p0) = o[c];
    } else {
        for (int64_t p = p0; p < p0 + 4 && p < HW; ++p) {
            int ob = src[p], og = src[HW + p], orr = src[2 * HW + p];
            if (on) hsv_px(ob, og, orr, fs, fv, sdiv, hdiv, ob, og, orr);
            dst[p] = static_cast<uint8_t>(ob);
            dst[HW + p] = static_cast<uint8_t>(og);
            dst[2 * HW + p] = static_cast<uint8_t>(orr);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// stencil + noise
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kTileW = 64, kTileH = 16;
constexpr int kPadX = 16;                                   // staged columns either side (>= max halo, multiple of 4)
constexpr int kStageW = kTileW + 2 * kPadX;                 // 96 bytes = 24 words per staged row
constexpr int kStageWords = kStageW / 4;
constexpr int kStageH = kTileH + 2 * FFB6D_STENCIL_MAX_HALO;

__device__ __forceinline__ int64_t reflect101(int64_t p, int64_t len)
{
    if (len == 1) return 0;
    while (p < 0 || p >= len) p = p < 0 ? -p : 2 * len - 2 - p;
    return p;
}

__device__ __forceinline__ uint64_t mix64(uint64_t z)     // splitmix64 finaliser
{
    z ^= z >> 30; z *= 0xbf58476d1ce4e5b9ull;
    z ^= z >> 27; z *= 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ float normal01(uint64_t seed, int b, int stage, int c, int64_t pix)
{
    const uint64_t key = mix64(seed ^ (0x9e3779b97f4a7c15ull * static_cast<uint64_t>((static_cast<int64_t>(b) * 2 + stage) * 3 + c + 1)));
    const uint64_t r = mix64(key + static_cast<uint64_t>(pix));
    const float u1 = (static_cast<float>(r >> 40) + 1.f) * (1.f / 16777216.f);        // (0, 1]
    const float u2 = static_cast<float>((r >> 16) & 0xffffffu) * (1.f / 16777216.f);  // [0, 1)
    return sqrtf(-2.f * logf(u1)) * cosf(6.2831853071795865f * u2);
}

__device__ __forceinline__ int add_noise(int v, float sigma, float n)   // (uint8) clip(v + sigma n, 0, 255): truncates
{
    float x = static_cast<float>(v) + sigma * n;
    x = x < 0.f ? 0.f : x > 255.f ? 255.f : x;
    return static_cast<int>(x);
}

template <bool kVec>
__global__ __launch_bounds__(kThreads) void stencil_kernel(const uint8_t* __restrict__ in,
                                                           const ffb6d_stencil_frame_t* __restrict__ frames, uint64_t seed,
                                                           uint8_t* __restrict__ out, int64_t H, int64_t W)
{
    __shared__ uint32_t stage[3 * kStageH * kStageWords];
    __shared__ int tap_off[FFB6D_STENCIL_MAX_TAPS];
    __shared__ float tap_w[FFB6D_STENCIL_MAX_TAPS];
    const int b = blockIdx.z;
    const int tid = threadIdx.x;
    const ffb6d_stencil_frame_t& f = frames[b];
    int n_taps = f.n_taps, halo = f.halo;
    if (n_taps < 0 || n_taps > FFB6D_STENCIL_MAX_TAPS || halo < 0 || halo > FFB6D_STENCIL_MAX_HALO) n_taps = halo = 0;
    const float sigma = f.sigma, extra = f.extra_sigma;
    if (tid < n_taps) {
        const int dy = min(max(f.dy[tid], -halo), halo), dx = min(max(f.dx[tid], -halo), halo);
        tap_off[tid] = dy * kStageW + dx;
        tap_w[tid] = f.w[tid];
    }
    const int64_t HW = H * W;
    const uint8_t* src = in + static_cast<int64_t>(b) * 3 * HW;
    uint8_t* dst = out + static_cast<int64_t>(b) * 3 * HW;
    const int64_t x0 = static_cast<int64_t>(blockIdx.x) * kTileW, y0 = static_cast<int64_t>(blockIdx.y) * kTileH;

    // stage rows y0 - halo .. y0 + kTileH + halo - 1 and the words that cover columns x0 - halo .. x0 + kTileW + halo - 1
    const int rows = kTileH + 2 * halo;
    const int wlo = (kPadX - halo) >> 2, whi = (kPadX + kTileW + halo + 3) >> 2;
    const int nw = whi - wlo;
    for (int i = tid; i < 3 * rows * nw; i += kThreads) {
        const int c = i / (rows * nw), rem = i - c * rows * nw, rr = rem / nw, w = wlo + (rem - rr * nw);
        const int64_t gy = reflect101(y0 - halo + rr, H);
        const int64_t gx = x0 - kPadX + 4 * w;
        const uint8_t* line = src + c * HW + gy * W;
        uint32_t word;
        if (kVec && gx >= 0 && gx + 3 < W) {
            word = *reinterpret_cast<const uint32_t*>(line + gx);
        } else {
            word = 0u;
#pragma unroll
            for (int q = 0; q < 4; ++q) word |= static_cast<uint32_t>(line[reflect101(gx + q, W)]) << (8 * q);
        }
        stage[(c * kStageH + rr) * kStageWords + w] = word;
    }
    __syncthreads();

    const int tx = tid & 15, ty = tid >> 4;
    const int64_t y = y0 + ty, xs = x0 + 4 * tx;
    if (y >= H || xs >= W) return;
    const uint8_t* st = reinterpret_cast<const uint8_t*>(stage);
    for (int c = 0; c < 3; ++c) {
        const uint8_t* centre = st + (c * kStageH + ty + halo) * kStageW + kPadX + 4 * tx;
        int v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (n_taps == 0) {
                v[q] = centre[q];
            } else {
                float acc = 0.f;
                for (int t = 0; t < n_taps; ++t) acc = acc + tap_w[t] * static_cast<float>(centre[q + tap_off[t]]);
                v[q] = sat_u8(acc);
            }
            const int64_t pix = y * W + xs + q;
            if (sigma > 0.f) v[q] = add_noise(v[q], sigma, normal01(seed, b, 0, c, pix));
            if (extra > 0.f) v[q] = add_noise(v[q], extra, normal01(seed, b, 1, c, pix));
        }
        uint8_t* drow = dst + c * HW + y * W;
        if (kVec && xs + 3 < W) {
            *reinterpret_cast<uint32_t*>(drow + xs) = static_cast<uint32_t>(v[0]) | (static_cast<uint32_t>(v[1]) << 8) |
                                                      (static_cast<uint32_t>(v[2]) << 16) | (static_cast<uint32_t>(v[3]) << 24);
        } else {
            for (int q = 0; q < 4 && xs + q < W; ++q) drow[xs + q] = static_cast<uint8_t>(v[q]);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// background compositing
// ---------------------------------------------------------------------------------------------------------------------
template <bool kVec>
__global__ __launch_bounds__(kThreads) void add_real_back_kernel(
    const uint8_t* __restrict__ rgb, const void* __restrict__ label, int label_u8, const float* __restrict__ depth,
    const uint8_t* __restrict__ back_rgb, const float* __restrict__ back_depth, const void* __restrict__ back_mask,
    int back_mask_u8, int flavour, const uint8_t* __restrict__ composite_rgb, uint8_t* __restrict__ rgb_out,
    float* __restrict__ depth_out, int64_t HW)
{
    const int b = blockIdx.y;
    const int64_t p0 = (static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x) * 4;
    if (p0 >= HW) return;
    const bool do_rgb = composite_rgb == nullptr || composite_rgb[b] != 0;
    const int64_t base = static_cast<int64_t>(b) * HW;
    uint32_t fg = 0u, keep = 0u;                            // per pixel q: bit q = label <= 0, keep_back
    const int n = HW - p0 >= 4 ? 4 : static_cast<int>(HW - p0);
    for (int q = 0; q < n; ++q) {
        const int64_t at = base + p0 + q;
        const int lab = label_u8 ? static_cast<int>(static_cast<const uint8_t*>(label)[at]) : static_cast<const int*>(label)[at];
        const int bm = back_mask_u8 ? static_cast<int>(static_cast<const uint8_t*>(back_mask)[at]) : static_cast<const int*>(back_mask)[at];
        const bool kb = flavour == 0 ? bm <= 0 : bm < 255;
        fg |= static_cast<uint32_t>(lab <= 0) << q;
        keep |= static_cast<uint32_t>(kb) << q;
        const float d = depth[at];
        depth_out[at] = d > 1e-6f ? d : back_depth[at] * (kb ? 1.f : 0.f);
    }
    const uint8_t* s = rgb + 3 * base;
    const uint8_t* bk = back_rgb + 3 * base;
    uint8_t* o = rgb_out + 3 * base;
    for (int c = 0; c < 3; ++c) {
        if (kVec) {
            const uint32_t a = *reinterpret_cast<const uint32_t*>(s + c * HW + p0);
            const uint32_t k = *reinterpret_cast<const uint32_t*>(bk + c * HW + p0);
            uint32_t r = 0u;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t mask = 0xffu << (8 * q);
                const uint32_t pick = do_rgb && ((fg >> q) & 1u) ? (((keep >> q) & 1u) ? (k & mask) : 0u) : (a & mask);
                r |= pick;
            }
            *reinterpret_cast<uint32_t*>(o + c * HW + p0) = r;
        } else {
            for (int q = 0; q < n; ++q) {
                const int64_t at = c * HW + p0 + q;
                o[at] = do_rgb && ((fg >> q) & 1u) ? (((keep >> q) & 1u) ? bk[at] : static_cast<uint8_t>(0)) : s[at];
            }
        }
    }
}

bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

}  // namespace

extern "C" {

int ffb6d_pose_targets(const float* cld, const void* choose, int choose_i64, const void* label_img, int label_u8,
                       const int* cls_ids, const void* RTs, int rts_f64, const float* mesh_kps, const float* mesh_ctr,
                       int n_cls, int B, int64_t N, int64_t HW, int O, int K, int* labels, float* kp_targ_ofst,
                       float* ctr_targ_ofst, float* kp_3ds, float* ctr_3ds, float* RTs_out, int* cls_ids_out,
                       ffb6d_stream_t stream)
{
    FFB6D_REQUIRE(B >= 0 && N >= 0 && HW >= 0 && n_cls >= 1, "ffb6d_pose_targets: B = %d, N = %lld, HW = %lld, n_cls = %d", B,
                  static_cast<long long>(N), static_cast<long long>(HW), n_cls);
    FFB6D_REQUIRE(K >= 1 && K <= kMaxK && O >= 1 && O <= kMaxO && O * (K + 1) <= kMaxXf,
                  "ffb6d_pose_targets: K = %d, O = %d outside the limits (K <= %d, O <= %d, O * (K + 1) <= %d)", K, O, kMaxK,
                  kMaxO, kMaxXf);
    if (B == 0) return FFB6D_OK;
    FFB6D_REQUIRE(cls_ids && RTs && mesh_kps && mesh_ctr && kp_3ds && ctr_3ds && RTs_out && cls_ids_out,
                  "ffb6d_pose_targets: a null pointer");
    FFB6D_REQUIRE(N == 0 || (cld && choose && label_img && labels && kp_targ_ofst && ctr_targ_ofst),
                  "ffb6d_pose_targets: a null point pointer");
    const int64_t tiles = N > 0 ? ffb6d::ceil_div(N, kPts) : 1;
    FFB6D_REQUIRE(tiles <= INT_MAX && B <= 65535, "ffb6d_pose_targets: grid %lld x %d", static_cast<long long>(tiles), B);
    pose_targets_kernel<<<dim3(static_cast<unsigned>(tiles), static_cast<unsigned>(B)), dim3(kThreads), 0, ffb6d::as_stream(stream)>>>(
        cld, choose, choose_i64, label_img, label_u8, cls_ids, RTs, rts_f64, mesh_kps, mesh_ctr, n_cls, N, HW, O, K, labels,
        kp_targ_ofst, ctr_targ_ofst, kp_3ds, ctr_3ds, RTs_out, cls_ids_out);
    FFB6D_LAUNCH_CHECK();
    return FFB6D_OK;
}

int ffb6d_rgb_hsv_jitter(const uint8_t* in, const double* fs_fv, uint8_t* out, int B, int64_t H, int64_t W,
                         ffb6d_stream_t stream)
{
    FFB6D_REQUIRE(B >= 0 && H >= 0 && W >= 0, "ffb6d_rgb_hsv_jitter: B = %d, H = %lld, W = %lld", B, static_cast<long long>(H),
                  static_cast<long long>(W));
    const int64_t HW = H * W;
    if (B == 0 || HW == 0) return FFB6D_OK;
    FFB6D_REQUIRE(in && fs_fv && out, "ffb6d_rgb_hsv_jitter: a null pointer");
    FFB6D_REQUIRE(B <= 65535, "ffb6d_rgb_hsv_jitter: B = %d", B);
    const int64_t blocks = ffb6d::ceil_div(ffb6d::ceil_div(HW, 4), kThreads);
    FFB6D_REQUIRE(blocks <= INT_MAX, "ffb6d_rgb_hsv_jitter: %lld workgroups", static_cast<long long>(blocks));
    const dim3 grid(static_cast<unsigned>(blocks), static_cast<unsigned>(B));
    if (HW % 4 == 0 && aligned4(in) && aligned4(out))
        hsv_kernel<true><<<grid, dim3(kThreads), 0, ffb6d::as_stream(stream)>>>(in, fs_fv, out, HW);
    else
        hsv_kernel<false><<<grid, dim3(kThreads), 0, ffb6d::as_stream(stream)>>>(in, fs_fv, out, HW);
    FFB6D_LAUNCH_CHECK();
    return FFB6D_OK;
}

int ffb6d_rgb_stencil(const uint8_t* in, const ffb6d_stencil_frame_t* frames, uint64_t seed, uint8_t* out, int B,
                      int64_t H, int64_t W, ffb6d_stream_t stream)
{
    FFB6D_REQUIRE(B >= 0 && H >= 0 && W >= 0, "ffb6d_rgb_stencil: B = %d, H = %lld, W = %lld", B, static_cast<long long>(H),
                  static_cast<long long>(W));
    if (B == 0 || H == 0 || W == 0) return FFB6D_OK;
    FFB6D_REQUIRE(in && frames && out && in != out, "ffb6d_rgb_stencil: a null pointer, or in == out");
    const int64_t gx = ffb6d::ceil_div(W, kTileW), gy = ffb6d::ceil_div(H, kTileH);
    FFB6D_REQUIRE(gx <= INT_MAX && gy <= 65535 && B <= 65535, "ffb6d_rgb_stencil: grid %lld x %lld x %d",
                  static_cast<long long>(gx), static_cast<long long>(gy), B);
    const dim3 grid(static_cast<unsigned>(gx), static_cast<unsigned>(gy), static_cast<unsigned>(B));
    if (W % 4 == 0 && aligned4(in) && aligned4(out))
        stencil_kernel<true><<<grid, dim3(kThreads), 0, ffb6d::as_stream(stream)>>>(in, frames, seed, out, H, W);
    else
        stencil_kernel<false><<<grid, dim3(kThreads), 0, ffb6d::as_stream(stream)>>>(in, frames, seed, out, H, W);
    FFB6D_LAUNCH_CHECK();
    return FFB6D_OK;
}

int ffb6d_add_real_back(const uint8_t* rgb, const void* label, int label_u8, const float* depth, const uint8_t* back_rgb,
                        const float* back_depth, const void* back_mask, int back_mask_u8, int flavour,
                        const uint8_t* composite_rgb, uint8_t* rgb_out, float* depth_out, int B, int64_t HW,
                        ffb6d_stream_t stream)
{
    FFB6D_REQUIRE(B >= 0 && HW >= 0 && (flavour == 0 || flavour == 1), "ffb6d_add_real_back: B = %d, HW = %lld, flavour = %d", B,
                  static_cast<long long>(HW), flavour);
    if (B == 0 || HW == 0) return FFB6D_OK;
    FFB6D_REQUIRE(rgb && label && depth && back_rgb && back_depth && back_mask && rgb_out && depth_out,
                  "ffb6d_add_real_back: a null pointer");
    FFB6D_REQUIRE(B <= 65535, "ffb6d_add_real_back: B = %d", B);
    const int64_t blocks = ffb6d::ceil_div(ffb6d::ceil_div(HW, 4), kThreads);
    FFB6D_REQUIRE(blocks <= INT_MAX, "ffb6d_add_real_back: %lld workgroups", static_cast<long long>(blocks));
    const dim3 grid(static_cast<unsigned>(blocks), static_cast<unsigned>(B));
    if (HW % 4 == 0 && aligned4(rgb) && aligned4(back_rgb) && aligned4(rgb_out))
        add_real_back_kernel<true><<<grid, dim3(kThreads), 0, ffb6d::as_stream(stream)>>>(
            rgb, label, label_u8, depth, back_rgb, back_depth, back_mask, back_mask_u8, flavour, composite_rgb, rgb_out, depth_out, HW);
    else
        add_real_back_kernel<false><<<grid, dim3(kThreads), 0, ffb6d::as_stream(stream)>>>(
            rgb, label, label_u8, depth, back_rgb, back_depth, back_mask, back_mask_u8, flavour, composite_rgb, rgb_out, depth_out, HW);
    FFB6D_LAUNCH_CHECK();
    return FFB6D_OK;
}

}  // extern "C"
