// ffb6d_amd/csrc/fps.hip -- batched farthest-point sampling and per-set box statistics (include/ffb6d_fps.h states the rule
// and the two forms).  One workgroup of kBlock threads owns a set from start to end; a step is
//   distance update + per-lane arg-max key  ->  wave reduction (DPP inside a row, then across rows)  ->  the winning lane writes
//   key + xyz to its wave's LDS slot (double-buffered by step parity)  ->  ONE barrier  ->  every wave reduces the kWaves slots.
// Why one barrier is enough: step k writes slots[k & 1] and reads them behind barrier k.  The next writes to slots[k & 1] come in
// step k + 2, behind barrier k + 1, which no wave passes before every wave has arrived there -- with its reads of step k done.
#include <cfloat>

#include "common.h"
#include "ffb6d_fps.h"

namespace {

constexpr int kBlock = 1024;                 // 16 waves, 4 per SIMD: at most 128 VGPRs per lane
constexpr int kWaves = kBlock / 64;
constexpr int kMaxPerLane = 8;               // 8 x (x, y, z, min_dist) = 32 VGPRs; with 16 per lane hipcc spills to scratch
constexpr int kCapacity = kBlock * kMaxPerLane;
constexpr int kBoxBlock = 256;

static_assert(kWaves == 16, "the slot reduction below is one DPP row of 16 lanes");

size_t align256(size_t x) { return (x + 255) & ~static_cast<size_t>(255); }

int g_form = 0;

struct alignas(16) Slot { unsigned long long key; float x, y, z, pad; };

// the reference's squared_norm of a difference (farthest_point_sampling.cpp:18,25): every operation rounded on its own
__device__ __forceinline__ float dist2(float x, float y, float z, float cx, float cy, float cz) {
    const float dx = __fsub_rn(x, cx), dy = __fsub_rn(y, cy), dz = __fsub_rn(z, cz);
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

__device__ __forceinline__ unsigned long long pack(unsigned hi, unsigned lo) { return (static_cast<unsigned long long>(hi) << 32) | lo; }
__device__ __forceinline__ unsigned long long umax64(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

// lane i of a row of 16 receives lane (i - N) mod 16 of the same row (v_mov_b32_dpp row_ror:N), both halves of the key
template <int N>
__device__ __forceinline__ unsigned long long row_ror(unsigned long long v) {
    const int lo = static_cast<int>(static_cast<unsigned>(v)), hi = static_cast<int>(static_cast<unsigned>(v >> 32));
    const int rlo = __builtin_amdgcn_update_dpp(lo, lo, 0x120 + N, 0xf, 0xf, false);
    const int rhi = __builtin_amdgcn_update_dpp(hi, hi, 0x120 + N, 0xf, 0xf, false);
    return pack(static_cast<unsigned>(rhi), static_cast<unsigned>(rlo));
}

// maximum over the 16 lanes of a DPP row, in every lane of the row
__device__ __forceinline__ unsigned long long row_max_key(unsigned long long v) {
    v = umax64(v, row_ror<1>(v));
    v = umax64(v, row_ror<2>(v));
    v = umax64(v, row_ror<4>(v));
    v = umax64(v, row_ror<8>(v));
    return v;
}

// maximum over the 64 lanes of a wave, in every lane
__device__ __forceinline__ unsigned long long wave_max_key(unsigned long long v) {
    v = row_max_key(v);
    v = umax64(v, __shfl_xor(v, 16));
    // lanes l and l ^ 32 trade their keys (v_permlane32_swap: of the two results one is the lane's own value, one its partner's)
    const auto lo = __builtin_amdgcn_permlane32_swap(static_cast<unsigned>(v), static_cast<unsigned>(v), false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap(static_cast<unsigned>(v >> 32), static_cast<unsigned>(v >> 32), false, false);
    return umax64(pack(hi[0], lo[0]), pack(hi[1], lo[1]));
}

__device__ __forceinline__ float wave_min_f(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_max_f(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// rows of set s, clamped so that no table content leads outside pts
__device__ __forceinline__ int64_t set_rows(const int64_t* __restrict__ begin, int s, int64_t total, int64_t* first) {
    int64_t b0 = begin[s], b1 = begin[s + 1];
    b0 = b0 < 0 ? 0 : (b0 > total ? total : b0);
    b1 = b1 < 0 ? 0 : (b1 > total ? total : b1);
    *first = b0;
    return b1 > b0 ? b1 - b0 : 0;
}

// the pick of a step, the same in every thread of the workgroup
struct Pick { int idx; float x, y, z, d; };

// PPL > 0: the resident form, point j * kBlock + tid in register slot j of thread tid; PPL == 0: the streaming form, the same
// assignment of points to threads with the coordinates re-read from pts and min_dist in `md_ws` (f32 [S,max_n]).
template <int PPL>
__global__ __launch_bounds__(kBlock) void fps_kernel(const float* __restrict__ pts, const int64_t* __restrict__ begin, int64_t total,
                                                     int64_t max_n, int m, const int* __restrict__ start, int* __restrict__ idx,
                                                     float* __restrict__ out_pts, float* __restrict__ out_dist,
                                                     float* __restrict__ md_ws) {
    __shared__ Slot slots[2][kWaves];
    __shared__ float box_lo[kWaves][3], box_hi[kWaves][3];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t b0;
    int64_t rows = set_rows(begin, s, total, &b0);
    if (rows > max_n) rows = max_n;
    const int n = static_cast<int>(rows);                                      // max_n < 2^31
    const int64_t row0 = static_cast<int64_t>(s) * m;
    if (n == 0) {                                                              // the whole workgroup leaves: no barrier is skipped by some
        for (int k = tid; k < m; k += kBlock) {
            if (idx) idx[row0 + k] = -1;
            if (out_dist) out_dist[row0 + k] = 0.f;
            if (out_pts) out_pts[(row0 + k) * 3] = out_pts[(row0 + k) * 3 + 1] = out_pts[(row0 + k) * 3 + 2] = 0.f;
        }
        return;
    }
    const float* __restrict__ P = pts + b0 * 3;
    float* __restrict__ md_g = PPL == 0 ? md_ws + static_cast<int64_t>(s) * max_n : nullptr;
    const float p0x = P[0], p0y = P[1], p0z = P[2];                            // the index-0 fallback

    constexpr int R = PPL > 0 ? PPL : 1;
    float rx[R], ry[R], rz[R], rmd[R];
    if constexpr (PPL > 0) {
#pragma unroll
        for (int j = 0; j < PPL; ++j) {
            const int i = j * kBlock + tid;
            const bool live = i < n;
            const int64_t at = live ? static_cast<int64_t>(i) * 3 : 0;        // row 0 exists: the loads need no branch
            const float x = P[at], y = P[at + 1], z = P[at + 2];
            rx[j] = live ? x : 0.f;
            ry[j] = live ? y : 0.f;
            rz[j] = live ? z : 0.f;
            rmd[j] = live ? FLT_MAX : 0.f;                                     // a dead slot stays at 0: never a candidate
        }
    }

    int parity = 0;
    // one step: min_dist takes the distance to (cx, cy, cz), then the arg-max.  `first`: min_dist counts as FLT_MAX (streaming form:
    // the workspace holds nothing yet).
    auto step = [&](float cx, float cy, float cz, bool first) -> Pick {
        float bmd = 0.f, bx = 0.f, by = 0.f, bz = 0.f;
        int bi = 0;
        if constexpr (PPL > 0) {
#pragma unroll
            for (int j = 0; j < PPL; ++j) {
                const float v = fminf(rmd[j], dist2(rx[j], ry[j], rz[j], cx, cy, cz));
                rmd[j] = v;
                if (v > bmd) { bmd = v; bi = j * kBlock + tid; bx = rx[j]; by = ry[j]; bz = rz[j]; }      // ascending index: the lowest stays
            }
        } else {
#pragma unroll 4
            for (int i = tid; i < n; i += kBlock) {
                const float x = P[static_cast<int64_t>(i) * 3], y = P[static_cast<int64_t>(i) * 3 + 1], z = P[static_cast<int64_t>(i) * 3 + 2];
                const float old = first ? FLT_MAX : md_g[i];
                const float v = fminf(old, dist2(x, y, z, cx, cy, cz));
                md_g[i] = v;                                                   // read and written by this thread only
                if (v > bmd) { bmd = v; bi = i; bx = x; by = y; bz = z; }
            }
        }
        const unsigned long long key = bmd > 0.f ? pack(__float_as_uint(bmd), ~static_cast<unsigned>(bi)) : 0ull;
        const unsigned long long wmax = wave_max_key(key);
        if (wmax != 0ull ? key == wmax : lane == 0) {                          // keys above 0 are unique: they hold the index
            Slot& w = slots[parity][wave];
            w.key = wmax;
            w.x = bx;
            w.y = by;
            w.z = bz;
        }
        __syncthreads();
        const unsigned long long kmax = row_max_key(slots[parity][lane & (kWaves - 1)].key);
        Pick p;
        if (kmax == 0ull) {
            p = Pick{0, p0x, p0y, p0z, 0.f};
        } else {
            p.idx = static_cast<int>(~static_cast<unsigned>(kmax));
            p.d = __uint_as_float(static_cast<unsigned>(kmax >> 32));
            const Slot& w = slots[parity][(p.idx & (kBlock - 1)) >> 6];        // the wave that owns the point
            p.x = w.x;
            p.y = w.y;
            p.z = w.z;
        }
        parity ^= 1;
        return p;
    };

    Pick cur;
    if (start) {
        int c = start[s];
        c = c < 0 ? 0 : (c >= n ? n - 1 : c);
        cur = Pick{c, P[static_cast<int64_t>(c) * 3], P[static_cast<int64_t>(c) * 3 + 1], P[static_cast<int64_t>(c) * 3 + 2], FLT_MAX};
    } else {
        float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
        if constexpr (PPL > 0) {
#pragma unroll
            for (int j = 0; j < PPL; ++j)
                if (j * kBlock + tid < n) {
                    lo[0] = fminf(lo[0], rx[j]); hi[0] = fmaxf(hi[0], rx[j]);
                    lo[1] = fminf(lo[1], ry[j]); hi[1] = fmaxf(hi[1], ry[j]);
                    lo[2] = fminf(lo[2], rz[j]); hi[2] = fmaxf(hi[2], rz[j]);
                }
        } else {
            for (int i = tid; i < n; i += kBlock)
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const float v = P[static_cast<int64_t>(i) * 3 + a];
                    lo[a] = fminf(lo[a], v);
                    hi[a] = fmaxf(hi[a], v);
                }
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = wave_min_f(lo[a]);
            hi[a] = wave_max_f(hi[a]);
            if (lane == 0) { box_lo[wave][a] = lo[a]; box_hi[wave][a] = hi[a]; }
        }
        __syncthreads();
        float c[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            float l = box_lo[0][a], h = box_hi[0][a];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) { l = fminf(l, box_lo[w][a]); h = fmaxf(h, box_hi[w][a]); }
            c[a] = __fmul_rn(__fadd_rn(h, l), 0.5f);                           // (max + min) / 2.f = * (1.f / 2.f), :20,138
        }
        cur = step(c[0], c[1], c[2], true);
    }
    const bool fresh = start != nullptr;                                       // the first update finds no min_dist in the workspace
    for (int k = 0;; ++k) {
        if (tid == 0) {
            if (idx) idx[row0 + k] = cur.idx;
            if (out_dist) out_dist[row0 + k] = cur.d;
            if (out_pts) {
                out_pts[(row0 + k) * 3] = cur.x;
                out_pts[(row0 + k) * 3 + 1] = cur.y;
                out_pts[(row0 + k) * 3 + 2] = cur.z;
            }
        }
        if (k == m - 1) break;
        cur = step(cur.x, cur.y, cur.z, fresh && k == 0);
    }
}

__global__ __launch_bounds__(kBoxBlock) void box_info_kernel(const float* __restrict__ pts, const int64_t* __restrict__ begin,
                                                             int64_t total, float* __restrict__ corners, float* __restrict__ ctr,
                                                             float* __restrict__ radius) {
    __shared__ float box_lo[kBoxBlock / 64][3], box_hi[kBoxBlock / 64][3];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t b0;
    const int64_t n = set_rows(begin, s, total, &b0);
    float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (int64_t i = tid; i < n; i += kBoxBlock)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float v = pts[(b0 + i) * 3 + a];
            lo[a] = fminf(lo[a], v);
            hi[a] = fmaxf(hi[a], v);
        }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        lo[a] = wave_min_f(lo[a]);
        hi[a] = wave_max_f(hi[a]);
        if (lane == 0) { box_lo[wave][a] = lo[a]; box_hi[wave][a] = hi[a]; }
    }
    __syncthreads();
    if (tid != 0) return;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        lo[a] = box_lo[0][a];
        hi[a] = box_hi[0][a];
        for (int w = 1; w < kBoxBlock / 64; ++w) { lo[a] = fminf(lo[a], box_lo[w][a]); hi[a] = fmaxf(hi[a], box_hi[w][a]); }
        if (n == 0) lo[a] = hi[a] = 0.f;
    }
    if (corners)
        for (int k = 0; k < 8; ++k) {
            corners[(static_cast<int64_t>(s) * 8 + k) * 3] = (k & 4) ? hi[0] : lo[0];
            corners[(static_cast<int64_t>(s) * 8 + k) * 3 + 1] = (k & 2) ? hi[1] : lo[1];
            corners[(static_cast<int64_t>(s) * 8 + k) * 3 + 2] = (k & 1) ? hi[2] : lo[2];
        }
    if (ctr)
        for (int a = 0; a < 3; ++a) ctr[static_cast<int64_t>(s) * 3 + a] = __fmul_rn(__fadd_rn(hi[a], lo[a]), 0.5f);
    if (radius) {
        const float dx = __fsub_rn(hi[0], lo[0]), dy = __fsub_rn(hi[1], lo[1]), dz = __fsub_rn(hi[2], lo[2]);
        radius[s] = __fmul_rn(0.5f, __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz))));
    }
}

bool sizes_ok(int S, int64_t max_n, int m) { return S >= 1 && m >= 1 && max_n >= 0 && max_n < (static_cast<int64_t>(1) << 31); }

// 1 = resident, 2 = streaming, 0 = the forced resident form cannot hold max_n
int form_for(int64_t max_n) {
    if (g_form == 2) return 2;
    if (max_n <= kCapacity) return 1;
    return g_form == 1 ? 0 : 2;
}

}  // namespace

extern "C" {

int ffb6d_fps_resident_capacity(void) { return kCapacity; }

void ffb6d_fps_set_form(int form) { g_form = (form == 1 || form == 2) ? form : 0; }

size_t ffb6d_fps_workspace_bytes(int S, int64_t max_n, int m)
{
    if (!sizes_ok(S, max_n, m) || form_for(max_n) != 2) return 0;
    return align256(sizeof(float) * static_cast<size_t>(S) * static_cast<size_t>(max_n));
}

int ffb6d_fps_f32(const float* pts, const int64_t* begin, int S, int64_t total, int64_t max_n, int m, const int* start,
                  int* idx, float* out_pts, float* out_dist, void* workspace, size_t workspace_bytes, ffb6d_stream_t stream)
{
    FFB6D_REQUIRE(sizes_ok(S, max_n, m), "fps: bad sizes S=%d (>= 1) m=%d (>= 1) max_n=%lld (0 .. 2^31-1)", S, m, (long long)max_n);
    FFB6D_REQUIRE(total >= 0, "fps: bad sizes total=%lld", (long long)total);
    FFB6D_REQUIRE(idx || out_pts || out_dist, "fps: no output given");
    FFB6D_REQUIRE(begin && (pts || total == 0), "fps: null pointer in the point sets");
    const int form = form_for(max_n);
    FFB6D_REQUIRE(form != 0, "fps: max_n=%lld above the resident capacity %d with the resident form forced", (long long)max_n, kCapacity);
    const size_t need = ffb6d_fps_workspace_bytes(S, max_n, m);
    if (need && (!workspace || workspace_bytes < need))
        return ffb6d::set_error(FFB6D_ERR_WORKSPACE, "fps: workspace %zu < %zu bytes", workspace_bytes, need);
    hipStream_t st = ffb6d::as_stream(stream);
    float* md = static_cast<float*>(workspace);
    if (form == 2)
        fps_kernel<0><<<S, kBlock, 0, st>>>(pts, begin, total, max_n, m, start, idx, out_pts, out_dist, md);
    else if (max_n <= 2 * kBlock)
        fps_kernel<2><<<S, kBlock, 0, st>>>(pts, begin, total, max_n, m, start, idx, out_pts, out_dist, md);
    else
        fps_kernel<kMaxPerLane><<<S, kBlock, 0, st>>>(pts, begin, total, max_n, m, start, idx, out_pts, out_dist, md);
    FFB6D_LAUNCH_CHECK();
    return 0;
}

int ffb6d_box_info_f32(const float* pts, const int64_t* begin, int S, int64_t total, float* corners, float* ctr, float* radius,
                       ffb6d_stream_t stream)
{
    FFB6D_REQUIRE(S >= 1 && total >= 0, "box_info: bad sizes S=%d (>= 1) total=%lld", S, (long long)total);
    FFB6D_REQUIRE(corners || ctr || radius, "box_info: no output given");
    FFB6D_REQUIRE(begin && (pts || total == 0), "box_info: null pointer in the point sets");
    box_info_kernel<<<S, kBoxBlock, 0, ffb6d::as_stream(stream)>>>(pts, begin, total, corners, ctr, radius);
    FFB6D_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
