// ffb6d_amd/csrc/orb.hip -- texture-aware object keypoints: FAST-9 / Harris corners on a 1.2x gray pyramid, their lift through
// the rendered depth into the object frame, and the compaction into point sets for fps.hip (include/ffb6d_orb.h states the rule,
// in integers; tests/orb_ref.py restates it).  Launches of one detect call, all on the caller's stream:
//   gray (level 0), resize (levels 1 .. L-1, a dependent chain), three fills, detect (one launch over the tiles of every
//   (frame, level)), select (one workgroup per (frame, level)).
// detect: a 32 x 32 tile of the candidate rectangle; the gray tile with a halo of 4 is staged once in LDS as bytes, FAST scores
// are computed for the tile plus a halo of 1 and kept in LDS, NMS runs there, and the Harris sums are formed only at the (rare)
// survivors from the same LDS tile.  Survivors are appended to the (frame, level) list with an atomicAdd: the order of the list
// is arbitrary, so select takes the output position of a candidate from its rank alone (counted against the list in LDS chunks,
// long lists cut by a radix select first).
#include <cfloat>

#include "common.h"
#include "ffb6d_orb.h"

namespace {

constexpr int kMaxL = FFB6D_ORB_MAX_LEVELS;
constexpr int kTile = 32;                    // candidate pixels per tile side
constexpr int kGray = kTile + 8;             // + halo of 4: 3 (circle) + 1 (scores of the neighbours); 4 = 3 (7x7 block) + 1 (Sobel)
constexpr int kScore = kTile + 2;            // + halo of 1
constexpr int kDetectBlock = 256;
constexpr int kSelectBlock = 1024;
constexpr int kChunk = 2048;                 // candidates of the list held in LDS at a time: 24 KB
constexpr int kPixBlock = 256;
constexpr int kCompactBlock = 256;

size_t align256(size_t x) { return (x + 255) & ~static_cast<size_t>(255); }

// everything the kernels need to know about the pyramid, by value
struct Plan {
    int L, t, edge, Q;
    int W[kMaxL], H[kMaxL];
    int tiles_x[kMaxL], tile0[kMaxL + 1];    // tiles of the candidate rectangle per level, and their first block
    int cap[kMaxL], quota[kMaxL];            // list capacity per (frame, level): ceil(H_l/2) * ceil(W_l/2)
    long long gray_off[kMaxL];               // bytes: level l of frame f starts at gray_off[l] + f * H_l * W_l
    long long cand_off[kMaxL];               // entries: the list of (f, l) starts at cand_off[l] + f * cap[l]
    size_t cnt_off, resp_off, pix_off, total;       // bytes: the gray pyramid comes first
};

long long level_size(long long n, int l)
{
    long long p5 = 1, p6 = 1;
    for (int i = 0; i < l; ++i) { p5 *= 5; p6 *= 6; }
    return (2 * n * p5 + p6) / (2 * p6);
}

bool sizes_ok(int F, int H, int W, int L)
{
    return F >= 1 && F <= 65535 && H >= 4 && W >= 4 && H <= 16384 && W <= 16384 && L >= 1 && L <= kMaxL &&
           static_cast<long long>(F) * H * W < (1ll << 31);
}

// sizes and workspace layout; edge and quota only shape the launches
Plan make_plan(int F, int H, int W, int L, int t, int edge, const int* quota)
{
    Plan p{};
    p.L = L; p.t = t; p.edge = edge;
    size_t gray = 0;
    long long cand = 0;
    for (int l = 0; l < L; ++l) {
        p.W[l] = static_cast<int>(level_size(W, l));
        p.H[l] = static_cast<int>(level_size(H, l));
        p.cap[l] = ((p.H[l] + 1) / 2) * ((p.W[l] + 1) / 2);
        p.quota[l] = quota ? quota[l] : 0;
        p.Q += p.quota[l];
        p.gray_off[l] = static_cast<long long>(gray);
        gray += align256(static_cast<size_t>(F) * p.H[l] * p.W[l]);
        p.cand_off[l] = cand;
        cand += static_cast<long long>(F) * p.cap[l];
        const int w = p.W[l] - 2 * edge, h = p.H[l] - 2 * edge;
        const bool live = w >= 1 && h >= 1;
        p.tiles_x[l] = live ? (w + kTile - 1) / kTile : 0;
        p.tile0[l + 1] = p.tile0[l] + (live ? p.tiles_x[l] * ((h + kTile - 1) / kTile) : 0);
    }
    p.cnt_off = gray;
    p.resp_off = p.cnt_off + align256(sizeof(int) * static_cast<size_t>(F) * L);
    p.pix_off = p.resp_off + align256(sizeof(long long) * static_cast<size_t>(cand));
    p.total = p.pix_off + align256(sizeof(int) * static_cast<size_t>(cand));
    return p;
}

__global__ __launch_bounds__(kPixBlock) void orb_gray_kernel(const unsigned char* __restrict__ rgb, unsigned char* __restrict__ gray,
                                                             int F, int HW)
{
    const long long i = static_cast<long long>(blockIdx.x) * kPixBlock + threadIdx.x;
    if (i >= static_cast<long long>(F) * HW) return;
    const long long f = i / HW, px = i - f * HW;
    const unsigned char* s = rgb + f * 3 * HW + px;
    gray[i] = static_cast<unsigned char>((4899 * s[0] + 9617 * s[HW] + 1868 * s[2 * static_cast<long long>(HW)] + 8192) >> 14);
}

// source index and 11-bit weight of destination index x: n_src / n_dst are the two level sizes along the axis
__device__ __forceinline__ void tap(int x, int n_src, int n_dst, int* x0, int* x1, int* fx)
{
    const int num = (2 * x + 1) * n_src - n_dst, den = 2 * n_dst;
    *x0 = num / den;
    *fx = ((num - *x0 * den) * 2048) / den;
    *x1 = min(*x0 + 1, n_src - 1);
}

__global__ __launch_bounds__(kPixBlock) void orb_resize_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                               int F, int Hs, int Ws, int Hd, int Wd)
{
    const long long i = static_cast<long long>(blockIdx.x) * kPixBlock + threadIdx.x;
    const int HWd = Hd * Wd;
    if (i >= static_cast<long long>(F) * HWd) return;
    const long long f = i / HWd;
    const int px = static_cast<int>(i - f * HWd), y = px / Wd, x = px - y * Wd;
    int x0, x1, fx, y0, y1, fy;
    tap(x, Ws, Wd, &x0, &x1, &fx);
    tap(y, Hs, Hd, &y0, &y1, &fy);
    const unsigned char* s = src + f * Hs * Ws;
    const int top = (2048 - fx) * s[y0 * Ws + x0] + fx * s[y0 * Ws + x1];
    const int bot = (2048 - fx) * s[y1 * Ws + x0] + fx * s[y1 * Ws + x1];
    dst[i] = static_cast<unsigned char>(((2048 - fy) * top + fy * bot + (1 << 21)) >> 22);
}

// the radius-3 circle, clockwise from (0,-3) with y down: X(i, dx, dy)
#define ORB_CIRCLE(X) \
    X(0, 0, -3) X(1, 1, -3) X(2, 2, -2) X(3, 3, -1) X(4, 3, 0) X(5, 3, 1) X(6, 2, 2) X(7, 1, 3) \
    X(8, 0, 3) X(9, -1, 3) X(10, -2, 2) X(11, -3, 1) X(12, -3, 0) X(13, -3, -1) X(14, -2, -2) X(15, -1, -3)

// 9 consecutive set bits somewhere on the 16-bit ring
__device__ __forceinline__ bool ring_run9(unsigned m)
{
    const unsigned m2 = m | (m << 16);
    unsigned r = m2 & (m2 >> 1);
    r &= r >> 2;
    r &= r >> 4;                             // bit i: bits i .. i+7 of m2
    r &= m2 >> 8;
    return (r & 0xffffu) != 0;
}

// the FAST-9 score where it is above t, 0 (which no candidate test tells from the true value) where it is not: a score above t
// needs an arc of 9 pixels all brighter than g + t or all darker than g - t
__device__ __forceinline__ int fast_score(const unsigned char* g, int t)
{
    const int c = g[0];
    int d[16];
    unsigned hi = 0, lo = 0;
#define ORB_LOAD(i, dx, dy)                              \
    d[i] = static_cast<int>(g[(dy) * kGray + (dx)]) - c; \
    hi |= static_cast<unsigned>(d[i] > t) << (i);        \
    lo |= static_cast<unsigned>(d[i] < -t) << (i);
    ORB_CIRCLE(ORB_LOAD)
#undef ORB_LOAD
    if (!ring_run9(hi) && !ring_run9(lo)) return 0;
    int best = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        int mn = d[k], mx = d[k];
#pragma unroll
        for (int j = 1; j < 9; ++j) {
            mn = min(mn, d[(k + j) & 15]);
            mx = max(mx, d[(k + j) & 15]);
        }
        best = max(best, max(mn, -mx));
    }
    return best;
}

// g points at the candidate in the LDS gray tile
__device__ __forceinline__ long long harris(const unsigned char* g)
{
    long long a = 0, b = 0, c = 0;
    for (int by = -3; by <= 3; ++by)
        for (int bx = -3; bx <= 3; ++bx) {
            const unsigned char* q = g + by * kGray + bx;
            const int nw = q[-kGray - 1], n = q[-kGray], ne = q[-kGray + 1], w = q[-1], e = q[1];
            const int sw = q[kGray - 1], s = q[kGray], se = q[kGray + 1];
            const int ix = (ne + 2 * e + se) - (nw + 2 * w + sw), iy = (sw + 2 * s + se) - (nw + 2 * n + ne);
            a += ix * ix;
            b += iy * iy;
            c += ix * iy;
        }
    return 25 * (a * b - c * c) - (a + b) * (a + b);
}

__global__ __launch_bounds__(kDetectBlock) void orb_detect_kernel(Plan p, const unsigned char* __restrict__ gray, int* __restrict__ cnt,
                                                                  long long* __restrict__ cresp, int* __restrict__ cpix)
{
    __shared__ unsigned char sg[kGray * kGray];
    __shared__ short ss[kScore * kScore];
    const int tid = threadIdx.x, f = blockIdx.y;
    int b = blockIdx.x, l = 0;
    while (l + 1 < p.L && b >= p.tile0[l + 1]) ++l;
    b -= p.tile0[l];
    const int Wl = p.W[l], Hl = p.H[l];
    const int x0 = p.edge + (b % p.tiles_x[l]) * kTile, y0 = p.edge + (b / p.tiles_x[l]) * kTile;
    const unsigned char* g = gray + p.gray_off[l] + static_cast<long long>(f) * Hl * Wl;
    // pixels outside the level are clamped into it: they only feed scores that no candidate looks at (edge >= 4)
    for (int i = tid; i < kGray * kGray; i += kDetectBlock) {
        const int yy = min(max(y0 - 4 + i / kGray, 0), Hl - 1), xx = min(max(x0 - 4 + i % kGray, 0), Wl - 1);
        sg[i] = g[yy * Wl + xx];
    }
    __syncthreads();
    for (int i = tid; i < kScore * kScore; i += kDetectBlock) {
        const int sy = i / kScore, sx = i % kScore;
        ss[i] = static_cast<short>(fast_score(sg + (sy + 3) * kGray + sx + 3, p.t));
    }
    __syncthreads();
    for (int i = tid; i < kTile * kTile; i += kDetectBlock) {
        const int ty = i / kTile, tx = i % kTile, x = x0 + tx, y = y0 + ty;
        if (x >= Wl - p.edge || y >= Hl - p.edge) continue;
        const short* s = ss + (ty + 1) * kScore + tx + 1;
        const int v = s[0];
        if (v <= p.t) continue;
        if (v <= s[-kScore - 1] || v <= s[-kScore] || v <= s[-kScore + 1] || v <= s[-1] || v <= s[1] || v <= s[kScore - 1] ||
            v <= s[kScore] || v <= s[kScore + 1])
            continue;
        const long long r = harris(sg + (ty + 4) * kGray + tx + 4);
        const int pos = atomicAdd(&cnt[f * p.L + l], 1);
        if (pos < p.cap[l]) {                // always: strict maxima are never adjacent
            const long long at = p.cand_off[l] + static_cast<long long>(f) * p.cap[l] + pos;
            cresp[at] = r;
            cpix[at] = y * Wl + x;
        }
    }
}

// a signed response as an unsigned key of the same order
__device__ __forceinline__ unsigned long long order_key(long long r) { return static_cast<unsigned long long>(r) ^ (1ull << 63); }

// the output row of the candidate of rank `rank` at pixel index pi of level l
__device__ __forceinline__ void write_row(const Plan& p, int H0, int W0, int f, int l, int row0, int rank, int pi, long long ri,
                                          int* __restrict__ kps, long long* __restrict__ resp)
{
    const int Wl = p.W[l], Hl = p.H[l], y = pi / Wl, x = pi - y * Wl;
    const long long row = static_cast<long long>(f) * p.Q + row0 + rank;
    int* o = kps + row * 5;
    o[0] = x;
    o[1] = y;
    o[2] = l;
    o[3] = static_cast<int>((static_cast<long long>(2 * x + 1) * W0) / (2 * Wl));
    o[4] = static_cast<int>((static_cast<long long>(2 * y + 1) * H0) / (2 * Hl));
    resp[row] = ri;
}

// One workgroup per (frame, level): the rank of a candidate is the number of candidates that come before it, counted against the
// list in LDS chunks -- quadratic in the list's length.  A list longer than one chunk with a quota below its length is cut first:
// the quota-th largest response T is found by a radix select (8 passes over the 64-bit key, a 256-bin LDS histogram each), and only
// the candidates with a response >= T, which hold every candidate of rank < quota, are collected in LDS and ranked among themselves.
// Should more than a chunk of them remain (thousands of equal responses), the whole list is ranked after all.
__global__ __launch_bounds__(kSelectBlock) void orb_select_kernel(Plan p, int H0, int W0, const int* __restrict__ cnt,
                                                                  const long long* __restrict__ cresp, const int* __restrict__ cpix,
                                                                  int* __restrict__ count, int* __restrict__ kps, long long* __restrict__ resp)
{
    __shared__ long long lr[kChunk];
    __shared__ int lp[kChunk];
    __shared__ int hist[256];
    __shared__ unsigned long long s_prefix;
    __shared__ int s_need, s_kept;
    const int tid = threadIdx.x, l = blockIdx.x, f = blockIdx.y;
    int row0 = 0, all = 0;
    for (int k = 0; k < p.L; ++k) {
        const int kept = min(min(cnt[f * p.L + k], p.cap[k]), p.quota[k]);
        if (k < l) row0 += kept;
        all += kept;
    }
    if (l == 0 && tid == 0) count[f] = all;
    const int n = min(cnt[f * p.L + l], p.cap[l]), q = p.quota[l];
    if (min(n, q) == 0) return;
    const long long base = p.cand_off[l] + static_cast<long long>(f) * p.cap[l];
    if (n > kChunk && q < n) {
        if (tid == 0) { s_prefix = 0; s_need = q; }
        for (int shift = 56; shift >= 0; shift -= 8) {
            for (int b = tid; b < 256; b += kSelectBlock) hist[b] = 0;
            __syncthreads();
            // at least `need` candidates carry `prefix` in the bits above shift + 8, and the wanted key is among them
            const unsigned long long prefix = s_prefix, above = shift == 56 ? 0ull : ~0ull << (shift + 8);
            const int need = s_need;
            for (int i = tid; i < n; i += kSelectBlock) {
                const unsigned long long u = order_key(cresp[base + i]);
                if ((u & above) == prefix) atomicAdd(&hist[static_cast<int>((u >> shift) & 255)], 1);
            }
            __syncthreads();
            if (tid == 0) {
                int acc = 0, d = 255;
                while (d > 0 && acc + hist[d] < need) acc += hist[d--];
                s_prefix = prefix | (static_cast<unsigned long long>(d) << shift);
                s_need = need - acc;
                s_kept = 0;
            }
            __syncthreads();
        }
        const unsigned long long T = s_prefix;
        for (int i = tid; i < n; i += kSelectBlock) {
            const long long r = cresp[base + i];
            if (order_key(r) >= T) {
                const int pos = atomicAdd(&s_kept, 1);
                if (pos < kChunk) { lr[pos] = r; lp[pos] = cpix[base + i]; }
            }
        }
        __syncthreads();
        const int m = s_kept;
        if (m <= kChunk) {
            for (int i = tid; i < m; i += kSelectBlock) {
                const long long ri = lr[i];
                const int pi = lp[i];
                int rank = 0;
                for (int j = 0; j < m; ++j) rank += (lr[j] > ri || (lr[j] == ri && lp[j] < pi)) ? 1 : 0;
                if (rank < q) write_row(p, H0, W0, f, l, row0, rank, pi, ri, kps, resp);
            }
            return;
        }
    }
    for (int i0 = 0; i0 < n; i0 += kSelectBlock) {
        const int i = i0 + tid;
        const bool mine = i < n;
        const long long ri = mine ? cresp[base + i] : 0;
        const int pi = mine ? cpix[base + i] : 0;
        int rank = 0;
        for (int c0 = 0; c0 < n; c0 += kChunk) {
            const int m = min(kChunk, n - c0);
            __syncthreads();
            for (int j = tid; j < m; j += kSelectBlock) { lr[j] = cresp[base + c0 + j]; lp[j] = cpix[base + c0 + j]; }
            __syncthreads();
            if (mine)
                for (int j = 0; j < m; ++j) rank += (lr[j] > ri || (lr[j] == ri && lp[j] < pi)) ? 1 : 0;
        }
        if (mine && rank < q) write_row(p, H0, W0, f, l, row0, rank, pi, ri, kps, resp);
    }
}

__global__ __launch_bounds__(kPixBlock) void orb_lift_kernel(const int* __restrict__ kps, const int* __restrict__ count,
                                                             const float* __restrict__ depth, const int* __restrict__ visible,
                                                             const double* __restrict__ T, int F, int Q, int H, int W, float fx, float fy,
                                                             float cx, float cy, int min_pixels, float* __restrict__ slot_pts,
                                                             int* __restrict__ slot_ok)
{
    const long long i = static_cast<long long>(blockIdx.x) * kPixBlock + threadIdx.x;
    if (i >= static_cast<long long>(F) * Q) return;
    const int f = static_cast<int>(i / Q), r = static_cast<int>(i - static_cast<long long>(f) * Q);
    float o[3] = {0.f, 0.f, 0.f};
    int ok = 0;
    if (r < count[f] && visible[f] >= min_pixels) {
        const int X = kps[i * 5 + 3], Y = kps[i * 5 + 4];
        if (X >= 0 && X < W && Y >= 0 && Y < H) {
            const float z = depth[(static_cast<long long>(f) * H + Y) * W + X];
            if (fabsf(z) <= FLT_MAX && z > 1e-8f) {
                // a float quotient formed in double and rounded once is the correctly rounded float quotient (53 >= 2*24 + 2)
                const float px = static_cast<float>(static_cast<double>(__fmul_rn(__fsub_rn(static_cast<float>(X), cx), z)) / fx);
                const float py = static_cast<float>(static_cast<double>(__fmul_rn(__fsub_rn(static_cast<float>(Y), cy), z)) / fy);
                const double* t = T + static_cast<long long>(f) * 12;
                const double d0 = static_cast<double>(px) - t[3], d1 = static_cast<double>(py) - t[7], d2 = static_cast<double>(z) - t[11];
#pragma unroll
                for (int j = 0; j < 3; ++j) o[j] = static_cast<float>((d0 * t[j] + d1 * t[4 + j]) + d2 * t[8 + j]);
                ok = 1;
            }
        }
    }
    slot_pts[i * 3] = o[0];
    slot_pts[i * 3 + 1] = o[1];
    slot_pts[i * 3 + 2] = o[2];
    slot_ok[i] = ok;
}

// sum over the workgroup, in every thread; `part` holds one int per wave
__device__ __forceinline__ int block_sum(int v, int* part)
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((tid & 63) == 0) part[tid >> 6] = v;
    __syncthreads();
    int s = 0;
    for (int w = 0; w < kCompactBlock / 64; ++w) s += part[w];
    return s;
}

__global__ __launch_bounds__(kCompactBlock) void orb_count_kernel(const int* __restrict__ slot_ok, int rows, int* __restrict__ n_found)
{
    __shared__ int part[kCompactBlock / 64];
    const int s = blockIdx.x;
    int v = 0;
    for (int i = threadIdx.x; i < rows; i += kCompactBlock) v += slot_ok[static_cast<long long>(s) * rows + i] != 0;
    v = block_sum(v, part);
    if (threadIdx.x == 0) n_found[s] = v;
}

// one workgroup per object: its first row is the number of points of the objects before it; its kept rows follow in order
__global__ __launch_bounds__(kCompactBlock) void orb_compact_kernel(const float* __restrict__ slot_pts, const int* __restrict__ slot_ok,
                                                                    const int* __restrict__ n_found, int S, int rows,
                                                                    float* __restrict__ pts, long long* __restrict__ begin)
{
    __shared__ int part[kCompactBlock / 64];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int v = 0;
    for (int i = tid; i < s; i += kCompactBlock) v += n_found[i];
    long long at = block_sum(v, part);
    if (tid == 0) {
        begin[s] = at;
        if (s == S - 1) begin[S] = at + n_found[s];
    }
    for (int i0 = 0; i0 < rows; i0 += kCompactBlock) {
        const int i = i0 + tid;
        const long long src = static_cast<long long>(s) * rows + i;
        const bool ok = i < rows && slot_ok[src] != 0;
        const unsigned long long mask = __ballot(ok);
        __syncthreads();
        if (lane == 0) part[wave] = __popcll(mask);
        __syncthreads();
        int before = __popcll(mask & ((1ull << lane) - 1)), total = 0;
        for (int w = 0; w < kCompactBlock / 64; ++w) {
            if (w < wave) before += part[w];
            total += part[w];
        }
        if (ok) {
            float* o = pts + (at + before) * 3;
            o[0] = slot_pts[src * 3];
            o[1] = slot_pts[src * 3 + 1];
            o[2] = slot_pts[src * 3 + 2];
        }
        at += total;
    }
}

}  // namespace

extern "C" {

size_t ffb6d_orb_workspace_bytes(int F, int H, int W, int n_levels)
{
    if (!sizes_ok(F, H, W, n_levels)) return 0;
    return make_plan(F, H, W, n_levels, 0, 4, nullptr).total;
}

int ffb6d_orb_detect_u8(const unsigned char* rgb, int F, int H, int W, int n_levels, int fast_threshold, int edge,
                        const int* quota, int* count, int* kps, int64_t* resp, void* workspace, size_t workspace_bytes,
                        ffb6d_stream_t stream)
{
    FFB6D_REQUIRE(sizes_ok(F, H, W, n_levels), "orb_detect: bad sizes F=%d (1 .. 65535) H=%d W=%d (4 .. 16384, F*H*W < 2^31) n_levels=%d (1 .. 8)",
                  F, H, W, n_levels);
    FFB6D_REQUIRE(fast_threshold >= 0 && fast_threshold <= 255 && edge >= 4 && edge <= 4096,
                  "orb_detect: bad parameters fast_threshold=%d (0 .. 255) edge=%d (4 .. 4096)", fast_threshold, edge);
    FFB6D_REQUIRE(rgb && quota && count && kps && resp, "orb_detect: null pointer");
    long long Q = 0;
    for (int l = 0; l < n_levels; ++l) {
        FFB6D_REQUIRE(quota[l] >= 0, "orb_detect: bad quota[%d]=%d", l, quota[l]);
        Q += quota[l];
    }
    FFB6D_REQUIRE(Q >= 1 && F * Q < (1ll << 27), "orb_detect: bad quota sum Q=%lld (>= 1, F*Q < 2^27)", Q);
    const Plan p = make_plan(F, H, W, n_levels, fast_threshold, edge, quota);
    if (!workspace || workspace_bytes < p.total)
        return ffb6d::set_error(FFB6D_ERR_WORKSPACE, "orb_detect: workspace %zu < %zu bytes", workspace_bytes, p.total);
    hipStream_t st = ffb6d::as_stream(stream);
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    unsigned char* gray = ws;
    int* cnt = reinterpret_cast<int*>(ws + p.cnt_off);
    long long* cresp = reinterpret_cast<long long*>(ws + p.resp_off);
    int* cpix = reinterpret_cast<int*>(ws + p.pix_off);
    const long long n0 = static_cast<long long>(F) * H * W;
    orb_gray_kernel<<<static_cast<unsigned>(ffb6d::ceil_div(n0, kPixBlock)), kPixBlock, 0, st>>>(rgb, gray, F, H * W);
    for (int l = 1; l < n_levels; ++l) {
        const long long n = static_cast<long long>(F) * p.H[l] * p.W[l];
        orb_resize_kernel<<<static_cast<unsigned>(ffb6d::ceil_div(n, kPixBlock)), kPixBlock, 0, st>>>(
            gray + p.gray_off[l - 1], gray + p.gray_off[l], F, p.H[l - 1], p.W[l - 1], p.H[l], p.W[l]);
    }
    FFB6D_HIP_TRY(hipMemsetAsync(cnt, 0, sizeof(int) * static_cast<size_t>(F) * n_levels, st));
    FFB6D_HIP_TRY(hipMemsetAsync(kps, 0xff, sizeof(int) * 5 * static_cast<size_t>(F) * static_cast<size_t>(Q), st));
    FFB6D_HIP_TRY(hipMemsetAsync(resp, 0, sizeof(int64_t) * static_cast<size_t>(F) * static_cast<size_t>(Q), st));
    if (p.tile0[n_levels] > 0)
        orb_detect_kernel<<<dim3(p.tile0[n_levels], F), kDetectBlock, 0, st>>>(p, gray, cnt, cresp, cpix);
    orb_select_kernel<<<dim3(n_levels, F), kSelectBlock, 0, st>>>(p, H, W, cnt, cresp, cpix, count, kps, reinterpret_cast<long long*>(resp));
    FFB6D_LAUNCH_CHECK();
    return 0;
}

int ffb6d_orb_lift_f32(const int* kps, const int* count, const float* depth, const int* visible, const double* T, int F, int Q,
                       int H, int W, float fx, float fy, float cx, float cy, int min_pixels, float* slot_pts, int* slot_ok,
                       ffb6d_stream_t stream)
{
    FFB6D_REQUIRE(F >= 1 && Q >= 1 && H >= 1 && W >= 1 && static_cast<long long>(F) * H * W < (1ll << 31) &&
                      static_cast<long long>(F) * Q < (1ll << 27),
                  "orb_lift: bad sizes F=%d Q=%d H=%d W=%d (>= 1, F*H*W < 2^31, F*Q < 2^27)", F, Q, H, W);
    FFB6D_REQUIRE(fx != 0.f && fy != 0.f && fx == fx && fy == fy && cx == cx && cy == cy, "orb_lift: bad intrinsics fx=%g fy=%g cx=%g cy=%g",
                  fx, fy, cx, cy);
    FFB6D_REQUIRE(kps && count && depth && visible && T && slot_pts && slot_ok, "orb_lift: null pointer");
    const long long n = static_cast<long long>(F) * Q;
    orb_lift_kernel<<<static_cast<unsigned>(ffb6d::ceil_div(n, kPixBlock)), kPixBlock, 0, ffb6d::as_stream(stream)>>>(
        kps, count, depth, visible, T, F, Q, H, W, fx, fy, cx, cy, min_pixels, slot_pts, slot_ok);
    FFB6D_LAUNCH_CHECK();
    return 0;
}

int ffb6d_orb_compact_f32(const float* slot_pts, const int* slot_ok, int S, int V, int Q, float* pts, int64_t* begin,
                          int* n_found, ffb6d_stream_t stream)
{
    FFB6D_REQUIRE(S >= 1 && V >= 1 && Q >= 1 && static_cast<long long>(S) * V * Q < (1ll << 31),
                  "orb_compact: bad sizes S=%d V=%d Q=%d (>= 1, S*V*Q < 2^31)", S, V, Q);
    FFB6D_REQUIRE(slot_pts && slot_ok && pts && begin && n_found, "orb_compact: null pointer");
    hipStream_t st = ffb6d::as_stream(stream);
    const int rows = V * Q;
    FFB6D_HIP_TRY(hipMemsetAsync(pts, 0, sizeof(float) * 3 * static_cast<size_t>(S) * rows, st));
    orb_count_kernel<<<S, kCompactBlock, 0, st>>>(slot_ok, rows, n_found);
    orb_compact_kernel<<<S, kCompactBlock, 0, st>>>(slot_pts, slot_ok, n_found, S, rows, pts, reinterpret_cast<long long*>(begin));
    FFB6D_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
