// ffb6d_amd/csrc/color_jitter.hip -- torchvision's PIL ColorJitter on the device, held to Pillow's bytes (include/ffb6d_train.h
// states the rule).  Two launches per batch, whatever the per-frame orders:
//
//   jitter_sum_kernel:   grid (partials per frame, B).  Only frames whose chain holds a contrast do anything.  A workgroup walks its
//     share of the frame in tiles of 256 lanes x 16 pixels, applies the operations that precede the contrast in registers, adds the
//     luminances into a per-lane integer, reduces over the wave (shuffles) and the workgroup (LDS) and writes ONE 64-bit partial sum
//     into the workspace.  Partial sums, not an atomic into a slot: integer sums are exact either way, but a slot would have to be
//     zeroed by a third launch, and partial sums leave the workspace free to hold anything on entry.
//   jitter_apply_kernel: grid (tiles of 4096 pixels, B).  A workgroup of a contrast frame first adds the frame's partial sums (at most
//     kMaxPartials) and takes the mean; then every lane runs the whole chain on its 16 pixels in registers and stores once.
//
// Both are byte-stream kernels (3 bytes read per pixel in the sum pass, 3 read + 3 written in the apply pass), so a lane moves its 16
// pixels of a plane with one 16-byte access where the planes keep that alignment (H W a multiple of 16), with four 4-byte words
// where they keep 4 bytes, with single bytes otherwise and for the last, partial run of a frame.  256 lanes x 16 pixels: a wave's
// access covers 1 KiB of each plane, the widest a wave-instruction moves.  The 48 pixel registers of a lane and the unrolled hue
// arithmetic come to 120 - 130 VGPRs (3 - 4 waves per SIMD, no scratch): enough waves to cover the loads of a kernel that spends
// most of its time in the VALU (the hue's float divisions and its double-precision division by 6 are the long pole, see DESIGN.md
// section 8).  The operation of a chain step is uniform over the workgroup: the switch below is a scalar branch.
// The library is built with -ffp-contract=off: blend() rounds its product and its sum separately, as Pillow's C does.
#include <climits>
#include <cmath>

#include "common.h"
#include "ffb6d_train.h"

namespace {

constexpr int kThreads = 256;
constexpr int kRun = 16;                          // pixels per lane
constexpr int kTile = kThreads * kRun;            // pixels per workgroup step
constexpr int kMaxPartials = 1024;                // partial sums per frame: what every apply workgroup re-adds

// the one predicate of a valid record: the host check refuses on it, the kernels copy the frame
__host__ __device__ inline bool frame_ok(const ffb6d_jitter_frame_t& f)
{
    if (f.n_ops < 0 || f.n_ops > FFB6D_JITTER_MAX_OPS || f.hue_shift < 0 || f.hue_shift > 255) return false;
    unsigned seen = 0u;
    for (int i = 0; i < FFB6D_JITTER_MAX_OPS; ++i) {
        if (i >= f.n_ops) break;
        const int op = f.op[i];
        if (op < FFB6D_JITTER_BRIGHTNESS || op > FFB6D_JITTER_HUE || ((seen >> op) & 1u)) return false;
        seen |= 1u << op;
        if (op != FFB6D_JITTER_HUE && !(f.alpha[i] >= 0.f && f.alpha[i] <= 3.4028234663852886e38f)) return false;   // NaN fails both
    }
    return true;
}

__device__ __forceinline__ int luminance(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

__device__ __forceinline__ int blend(int d, int x, float alpha)
{
    const float fd = static_cast<float>(d);
    const float t = fd + alpha * (static_cast<float>(x) - fd);
    return t <= 0.f ? 0 : t >= 255.f ? 255 : static_cast<int>(t);
}

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

__device__ __forceinline__ void hue_px(int& r, int& g, int& b, int shift)
{
    const int mx = max(r, max(g, b)), mn = min(r, min(g, b));
    int H = 0, S = 0;
    const int V = mx;
    if (mx != mn) {
        const float cr = static_cast<float>(mx - mn);
        const float s = cr / static_cast<float>(mx);
        // h = base + qa - qb in double from two float32 quotients: (bc, gc, 0), (rc, bc, 2), (gc, rc, 4)
        const int ca = r == mx ? b : g == mx ? r : g;
        const int cb = r == mx ? g : g == mx ? b : r;
        const double base = r == mx ? 0.0 : g == mx ? 2.0 : 4.0;
        const float qa = static_cast<float>(mx - ca) / cr, qb = static_cast<float>(mx - cb) / cr;
        float h = static_cast<float>(base + static_cast<double>(qa) - static_cast<double>(qb));
        const double x = static_cast<double>(h) / 6.0 + 1.0;             // in (0.8, 1.9): fmod(x, 1.0) is x or x - 1, both exact
        h = static_cast<float>(x >= 1.0 ? x - 1.0 : x);
        H = clip8(static_cast<int>(static_cast<double>(h) * 255.0));
        S = clip8(static_cast<int>(static_cast<double>(s) * 255.0));
    }
    H = (H + shift) & 255;
    if (S == 0) {
        r = g = b = V;
        return;
    }
    const float hh = static_cast<float>(H) * 6.f / 255.f;
    const float fl = floorf(hh);
    const int i = static_cast<int>(fl) % 6;
    const float f = hh - fl;
    const float fs = static_cast<float>(S) / 255.f;
    const float fv = static_cast<float>(V);
    const int p = clip8(static_cast<int>(roundf(fv * (1.f - fs))));
    const int q = clip8(static_cast<int>(roundf(fv * (1.f - fs * f))));
    const int t = clip8(static_cast<int>(roundf(fv * (1.f - fs * (1.f - f)))));
    r = i == 0 || i == 5 ? V : i == 1 ? q : i == 4 ? t : p;
    g = i == 1 || i == 2 ? V : i == 0 ? t : i == 3 ? q : p;
    b = i == 3 || i == 4 ? V : i == 2 ? t : i == 5 ? q : p;
}

// one chain step on a lane's run; `op` is uniform over the workgroup
__device__ __forceinline__ void apply_op(int op, float alpha, int shift, int mean, int (&r)[kRun], int (&g)[kRun], int (&b)[kRun])
{
    switch (op) {
    case FFB6D_JITTER_BRIGHTNESS:
#pragma unroll
        for (int q = 0; q < kRun; ++q) { r[q] = blend(0, r[q], alpha); g[q] = blend(0, g[q], alpha); b[q] = blend(0, b[q], alpha); }
        break;
    case FFB6D_JITTER_CONTRAST:
#pragma unroll
        for (int q = 0; q < kRun; ++q) { r[q] = blend(mean, r[q], alpha); g[q] = blend(mean, g[q], alpha); b[q] = blend(mean, b[q], alpha); }
        break;
    case FFB6D_JITTER_SATURATION:
#pragma unroll
        for (int q = 0; q < kRun; ++q) {
            const int l = luminance(r[q], g[q], b[q]);
            r[q] = blend(l, r[q], alpha); g[q] = blend(l, g[q], alpha); b[q] = blend(l, b[q], alpha);
        }
        break;
    default:
#pragma unroll
        for (int q = 0; q < kRun; ++q) hue_px(r[q], g[q], b[q], shift);
        break;
    }
}

// n pixels of one plane from p (n == kRun: with the widest access kVec allows; pixels past n read as 0)
template <int kVec>
__device__ __forceinline__ void load_run(const uint8_t* __restrict__ p, int n, int (&v)[kRun])
{
    if (kVec >= 4 && n == kRun) {
        uint32_t w[4];
        if (kVec == 16) {
            const uint4 x = *reinterpret_cast<const uint4*>(p);
            w[0] = x.x; w[1] = x.y; w[2] = x.z; w[3] = x.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) w[k] = reinterpret_cast<const uint32_t*>(p)[k];
        }
#pragma unroll
        for (int q = 0; q < kRun; ++q) v[q] = static_cast<int>((w[q >> 2] >> (8 * (q & 3))) & 0xffu);
    } else {
#pragma unroll
        for (int q = 0; q < kRun; ++q) v[q] = q < n ? static_cast<int>(p[q]) : 0;
    }
}

template <int kVec>
__device__ __forceinline__ void store_run(uint8_t* __restrict__ p, int n, const int (&v)[kRun])
{
    if (kVec >= 4 && n == kRun) {
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int q = 0; q < kRun; ++q) w[q >> 2] |= static_cast<uint32_t>(v[q]) << (8 * (q & 3));
        if (kVec == 16) {
            *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) reinterpret_cast<uint32_t*>(p)[k] = w[k];
        }
    } else {
#pragma unroll
        for (int q = 0; q < kRun; ++q)
            if (q < n) p[q] = static_cast<uint8_t>(v[q]);
    }
}

// sum over the workgroup, returned to every thread; all kThreads threads must call it
__device__ __forceinline__ unsigned long long block_sum(unsigned long long v, unsigned long long* lds)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    const int tid = threadIdx.x;
    __syncthreads();                                // lds may still be read from an earlier call
    if ((tid & 63) == 0) lds[tid >> 6] = v;
    __syncthreads();
    unsigned long long s = 0ull;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) s += lds[w];
    return s;
}

// pixels of one sum workgroup (a multiple of kTile) and partial sums per frame (<= kMaxPartials)
inline int64_t sum_chunk(int64_t HW) { return kTile * ffb6d::ceil_div(HW, static_cast<int64_t>(kTile) * kMaxPartials); }
inline int64_t partials(int64_t HW) { return HW > 0 ? ffb6d::ceil_div(HW, sum_chunk(HW)) : 0; }

// position of the contrast in a valid chain, or -1
__device__ __forceinline__ int contrast_at(const ffb6d_jitter_frame_t& f)
{
    int at = -1;
    for (int i = 0; i < FFB6D_JITTER_MAX_OPS; ++i)
        if (i < f.n_ops && f.op[i] == FFB6D_JITTER_CONTRAST) at = i;
    return at;
}

template <int kVec>
__global__ __launch_bounds__(kThreads) void jitter_sum_kernel(const uint8_t* __restrict__ in,
                                                              const ffb6d_jitter_frame_t* __restrict__ frames,
                                                              unsigned long long* __restrict__ partial, int64_t HW, int64_t chunk,
                                                              int n_partials)
{
    __shared__ unsigned long long lds[kThreads / 64];
    const int b = blockIdx.y;
    const ffb6d_jitter_frame_t& f = frames[b];
    if (!frame_ok(f)) return;
    const int pre = contrast_at(f);
    if (pre < 0) return;                                        // no contrast: nothing to sum
    const uint8_t* src = in + static_cast<int64_t>(b) * 3 * HW;
    const int64_t lo = static_cast<int64_t>(blockIdx.x) * chunk;
    const int64_t hi = lo + chunk < HW ? lo + chunk : HW;
    unsigned long long acc = 0ull;
    for (int64_t p0 = lo + static_cast<int64_t>(threadIdx.x) * kRun; p0 < hi; p0 += kTile) {
        const int n = hi - p0 >= kRun ? kRun : static_cast<int>(hi - p0);
        int r[kRun], g[kRun], bl[kRun];
        load_run<kVec>(src + p0, n, r);
        load_run<kVec>(src + HW + p0, n, g);
        load_run<kVec>(src + 2 * HW + p0, n, bl);
        for (int i = 0; i < pre; ++i) apply_op(f.op[i], f.alpha[i], f.hue_shift, 0, r, g, bl);
        unsigned s = 0u;
#pragma unroll
        for (int q = 0; q < kRun; ++q) s += q < n ? static_cast<unsigned>(luminance(r[q], g[q], bl[q])) : 0u;
        acc += s;
    }
    const unsigned long long total = block_sum(acc, lds);
    if (threadIdx.x == 0) partial[static_cast<int64_t>(b) * n_partials + blockIdx.x] = total;
}

template <int kVec>
__global__ __launch_bounds__(kThreads) void jitter_apply_kernel(const uint8_t* __restrict__ in,
                                                                const ffb6d_jitter_frame_t* __restrict__ frames,
                                                                const unsigned long long* __restrict__ partial,
                                                                uint8_t* __restrict__ out, int64_t HW, int n_partials)
{
    __shared__ unsigned long long lds[kThreads / 64];
    const int b = blockIdx.y;
    const ffb6d_jitter_frame_t& f = frames[b];
    const int n_ops = frame_ok(f) ? f.n_ops : 0;                // a record that fails the check: the frame is copied
    int mean = 0;
    if (n_ops > 0 && contrast_at(f) >= 0) {                     // uniform over the workgroup
        unsigned long long s = 0ull;
        for (int i = threadIdx.x; i < n_partials; i += kThreads) s += partial[static_cast<int64_t>(b) * n_partials + i];
        s = block_sum(s, lds);
        mean = static_cast<int>(static_cast<double>(s) / static_cast<double>(HW) + 0.5);
    }
    const int64_t p0 = (static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x) * kRun;
    if (p0 >= HW) return;
    const int n = HW - p0 >= kRun ? kRun : static_cast<int>(HW - p0);
    const uint8_t* src = in + static_cast<int64_t>(b) * 3 * HW + p0;
    uint8_t* dst = out + static_cast<int64_t>(b) * 3 * HW + p0;
    int r[kRun], g[kRun], bl[kRun];
    load_run<kVec>(src, n, r);
    load_run<kVec>(src + HW, n, g);
    load_run<kVec>(src + 2 * HW, n, bl);
    for (int i = 0; i < n_ops; ++i) apply_op(f.op[i], f.alpha[i], f.hue_shift, mean, r, g, bl);
    store_run<kVec>(dst, n, r);
    store_run<kVec>(dst + HW, n, g);
    store_run<kVec>(dst + 2 * HW, n, bl);
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

template <int kVec>
void launch(const uint8_t* in, const ffb6d_jitter_frame_t* frames, uint8_t* out, int B, int64_t HW, unsigned long long* partial,
            hipStream_t stream)
{
    const int np = static_cast<int>(partials(HW));
    jitter_sum_kernel<kVec><<<dim3(static_cast<unsigned>(np), static_cast<unsigned>(B)), dim3(kThreads), 0, stream>>>(
        in, frames, partial, HW, sum_chunk(HW), np);
    jitter_apply_kernel<kVec><<<dim3(static_cast<unsigned>(ffb6d::ceil_div(HW, kTile)), static_cast<unsigned>(B)), dim3(kThreads), 0, stream>>>(
        in, frames, partial, out, HW, np);
}

}  // namespace

extern "C" {

int ffb6d_jitter_frames_check(const ffb6d_jitter_frame_t* host_frames, int B)
{
    FFB6D_REQUIRE(B >= 0, "ffb6d_jitter_frames_check: B = %d", B);
    if (B == 0) return FFB6D_OK;
    FFB6D_REQUIRE(host_frames, "ffb6d_jitter_frames_check: a null pointer");
    for (int b = 0; b < B; ++b)
        FFB6D_REQUIRE(frame_ok(host_frames[b]),
                      "ffb6d_jitter_frames_check: frame %d: n_ops outside [0, %d], an unknown or repeated operation, a negative or "
                      "non-finite factor, or a hue_shift outside [0, 255]", b, FFB6D_JITTER_MAX_OPS);
    return FFB6D_OK;
}

size_t ffb6d_color_jitter_workspace_bytes(int B, int64_t H, int64_t W)
{
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    const size_t bytes = static_cast<size_t>(B) * static_cast<size_t>(partials(H * W)) * sizeof(unsigned long long);
    return (bytes + 255) / 256 * 256;
}

int ffb6d_color_jitter_u8(const uint8_t* in, const ffb6d_jitter_frame_t* frames, uint8_t* out, int B, int64_t H, int64_t W,
                          void* workspace, size_t workspace_bytes, ffb6d_stream_t stream)
{
    FFB6D_REQUIRE(B >= 0 && H >= 0 && W >= 0 && (W == 0 || H <= INT64_MAX / 4 / W),
                  "ffb6d_color_jitter_u8: B = %d, H = %lld, W = %lld", B, static_cast<long long>(H), static_cast<long long>(W));
    const int64_t HW = H * W;
    if (B == 0 || HW == 0) return FFB6D_OK;
    FFB6D_REQUIRE(in && frames && out && in != out, "ffb6d_color_jitter_u8: a null pointer, or in == out");
    FFB6D_REQUIRE(B <= 65535 && ffb6d::ceil_div(HW, kTile) <= INT_MAX, "ffb6d_color_jitter_u8: grid %lld x %d",
                  static_cast<long long>(ffb6d::ceil_div(HW, kTile)), B);
    const size_t need = ffb6d_color_jitter_workspace_bytes(B, H, W);
    if (!workspace || workspace_bytes < need || !aligned(workspace, 8))
        return ffb6d::set_error(FFB6D_ERR_WORKSPACE, "ffb6d_color_jitter_u8: workspace %zu < %zu bytes (or null, or not 8-byte aligned)",
                                workspace_bytes, need);
    unsigned long long* partial = static_cast<unsigned long long*>(workspace);
    hipStream_t s = ffb6d::as_stream(stream);
    if (HW % 16 == 0 && aligned(in, 16) && aligned(out, 16)) launch<16>(in, frames, out, B, HW, partial, s);
    else if (HW % 4 == 0 && aligned(in, 4) && aligned(out, 4)) launch<4>(in, frames, out, B, HW, partial, s);
    else launch<1>(in, frames, out, B, HW, partial, s);
    FFB6D_LAUNCH_CHECK();
    return FFB6D_OK;
}

}  // extern "C"
