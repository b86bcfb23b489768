// ffb6d_amd/csrc/bop_scene.hip -- BOP scene evaluation: instance visibility in the measured depth and the greedy matching of scored
// estimates to ground-truth instances (include/ffb6d_bop_scene.h states both rules; tests/bop_scene_ref.py restates them in numpy).
//
// Visibility is a streaming pass over two float images, shaped like the VSD compare of bop_eval.hip (with which it shares the run of
// pixels, ray_dist and load_px through bop_common.h).
//   visib_count_kernel: grid (runs of kRunPx pixels, rows); a lane takes 4 consecutive pixels of each image per step (one 16-byte access
//     where the rows keep that alignment, single floats otherwise and for the tail) and keeps 4 counters, 4 running minima (from
//     INT_MAX) and 4 running maxima (from -1) in registers.  Most pixels of a single-instance render are empty: the distances are only
//     taken where something is drawn.  The workgroup writes ONE record of 12 integers per (row, run) (wave shuffles, then one LDS
//     slot set per wave): no atomics, and the workspace may hold anything on entry.  The mask, when asked for, leaves with the same
//     pass: 4 bytes per lane and step as one 32-bit store, single bytes where the vector path does not apply.
//   visib_finish_kernel: one wavefront per row adds the counts, combines the boxes and writes info and visib_fract.
// Matching is one workgroup of 256 lanes per group.
//   match_kernel: lanes e < E_g rank the estimates by counting (score descending, NaN as -inf, ties to the lower index) and write
//     order[rank] into LDS; after the barrier lane = configuration (col, k) walks the ordered estimates with a 64-bit taken mask in
//     registers, reading the group's error rows from global memory, and writes its entries of both output tables, -1 included.
//     All loops are bounded by the caps; no workgroup waits for another.
// The library is built with -ffp-contract=off; float division and __fsqrt_rn are correctly rounded.
#include <cfloat>
#include <climits>

#include "bop_common.h"
#include "ffb6d_bop_scene.h"

namespace {

using namespace ffb6d::bop;

constexpr int kRec = FFB6D_BOP_INFO_INTS;           // a partial record: 4 counts, 4 minima (column, row of obj; of visib), 4 maxima
constexpr int kMaxGroup = FFB6D_BOP_MAX_GROUP;

__device__ __forceinline__ float measured(float z) { return (z > 0.f && z <= FLT_MAX) ? z : 0.f; }      // not finite or <= 0: nothing

template <int kVec, bool kMask>
__global__ __launch_bounds__(kThreads) void visib_count_kernel(const float* __restrict__ depth_test, const float* __restrict__ depth_obj,
                                                               const int* __restrict__ frame_of, const double* __restrict__ K, int B, int HW,
                                                               int W, float delta, int* __restrict__ partial, int n_parts,
                                                               uint8_t* __restrict__ mask)
{
    __shared__ int red[kWaves][kRec];
    const int q = blockIdx.y, tid = threadIdx.x;
    const int b = frame_of[q];
    const int lo = blockIdx.x * kRunPx;                         // < HW <= INT_MAX - kRunPx: lo + kRunPx does not overflow
    const int hi = HW - lo > kRunPx ? lo + kRunPx : HW;
    uint8_t* mq = kMask ? mask + static_cast<int64_t>(q) * HW : nullptr;
    const bool ok = b >= 0 && b < B;                            // uniform; the finish kernel does not read a bad row's records
    Camera cam{1.f, 1.f, 0.f, 0.f};
    if (ok) {
        const double* Kb = K + 9 * static_cast<int64_t>(b);
        cam.fx = static_cast<float>(Kb[0]); cam.fy = static_cast<float>(Kb[4]);
        cam.cx = static_cast<float>(Kb[2]); cam.cy = static_cast<float>(Kb[5]);
    } else if (!kMask) {
        return;
    }
    const float* it = depth_test + static_cast<int64_t>(ok ? b : 0) * HW;
    const float* ig = depth_obj + static_cast<int64_t>(q) * HW;
    int cnt[4], mn[4], mx[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { cnt[k] = 0; mn[k] = INT_MAX; mx[k] = -1; }
    for (int step = 0; step < kSteps; ++step) {
        const int p0 = lo + (step * kThreads + tid) * kPx;
        if (p0 >= hi) break;
        const int n = hi - p0 >= kPx ? kPx : hi - p0;
        unsigned bytes = 0;
        if (ok) {
            float zt[kPx], zg[kPx];
            load_px<kVec>(it + p0, n, zt);
            load_px<kVec>(ig + p0, n, zg);
            const int r0 = p0 / W, c0 = p0 - r0 * W;
#pragma unroll
            for (int j = 0; j < kPx; ++j) {
                const float g = measured(zg[j]);                // entries past n read as 0
                if (g != 0.f) {
                    int r = r0, c = c0 + j;
                    if (c >= W) { r = (p0 + j) / W; c = (p0 + j) - r * W; }
                    const float dg = ray_dist(g, r, c, cam);
                    if (dg > 0.f) {                             // obj
                        const float dt = ray_dist(measured(zt[j]), r, c, cam);
                        const bool valid = dt > 0.f;
                        const bool visib = dt == 0.f || dg - dt <= delta;
                        const bool support = valid && dg - dt <= delta && dt - dg <= delta;
                        cnt[0] += 1;
                        cnt[1] += valid ? 1 : 0;
                        cnt[3] += support ? 1 : 0;
                        mn[0] = min(mn[0], c); mn[1] = min(mn[1], r); mx[0] = max(mx[0], c); mx[1] = max(mx[1], r);
                        if (visib) {
                            cnt[2] += 1;
                            mn[2] = min(mn[2], c); mn[3] = min(mn[3], r); mx[2] = max(mx[2], c); mx[3] = max(mx[3], r);
                            bytes |= 1u << (8 * j);
                        }
                    }
                }
            }
        }
        if (kMask) {
            if (kVec == 4 && n == kPx) {
                *reinterpret_cast<unsigned*>(mq + p0) = bytes;  // p0 and the row's offset are multiples of 4, the mask is 4-byte aligned
            } else {
#pragma unroll
                for (int j = 0; j < kPx; ++j)
                    if (j < n) mq[p0 + j] = static_cast<uint8_t>((bytes >> (8 * j)) & 1u);
            }
        }
    }
    if (!ok) return;                                            // uniform
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            cnt[k] += __shfl_xor(cnt[k], m, 64);
            mn[k] = min(mn[k], __shfl_xor(mn[k], m, 64));
            mx[k] = max(mx[k], __shfl_xor(mx[k], m, 64));
        }
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            red[tid >> 6][k] = cnt[k];
            red[tid >> 6][4 + k] = mn[k];
            red[tid >> 6][8 + k] = mx[k];
        }
    }
    __syncthreads();
    if (tid < kRec) {
        int v = red[0][tid];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) v = tid < 4 ? v + red[w][tid] : tid < 8 ? min(v, red[w][tid]) : max(v, red[w][tid]);
        partial[(static_cast<int64_t>(q) * n_parts + blockIdx.x) * kRec + tid] = v;
    }
}

__global__ __launch_bounds__(64) void visib_finish_kernel(const int* __restrict__ frame_of, int B, const int* __restrict__ partial,
                                                          int n_parts, int* __restrict__ info, double* __restrict__ visib_fract)
{
    const int q = blockIdx.x, tid = threadIdx.x;
    int* iq = info + static_cast<int64_t>(q) * kRec;
    const int b = frame_of[q];
    if (b < 0 || b >= B) {
        if (tid < kRec) iq[tid] = tid < 4 ? 0 : -1;
        if (tid == 0) visib_fract[q] = __builtin_nan("");
        return;
    }
    int cnt[4], mn[4], mx[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { cnt[k] = 0; mn[k] = INT_MAX; mx[k] = -1; }
    for (int i = tid; i < n_parts; i += 64) {
        const int* p = partial + (static_cast<int64_t>(q) * n_parts + i) * kRec;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            cnt[k] += p[k];
            mn[k] = min(mn[k], p[4 + k]);
            mx[k] = max(mx[k], p[8 + k]);
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            cnt[k] += __shfl_xor(cnt[k], m, 64);
            mn[k] = min(mn[k], __shfl_xor(mn[k], m, 64));
            mx[k] = max(mx[k], __shfl_xor(mx[k], m, 64));
        }
    }
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) iq[k] = cnt[k];
#pragma unroll
        for (int s = 0; s < 2; ++s) {                           // bbox_obj from the obj pixels, bbox_visib from the visib pixels
            const bool any = cnt[s == 0 ? 0 : 2] > 0;
            iq[4 + 4 * s] = any ? mn[2 * s] : -1;
            iq[5 + 4 * s] = any ? mn[2 * s + 1] : -1;
            iq[6 + 4 * s] = any ? mx[2 * s] - mn[2 * s] + 1 : -1;
            iq[7 + 4 * s] = any ? mx[2 * s + 1] - mn[2 * s + 1] + 1 : -1;
        }
        visib_fract[q] = cnt[0] == 0 ? 0.0 : static_cast<double>(cnt[2]) / static_cast<double>(cnt[0]);
    }
}

// ---- matching -----------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : v > hi ? hi : v; }

__global__ __launch_bounds__(kThreads) void match_kernel(const int* __restrict__ est_begin, const int* __restrict__ gt_begin,
                                                         const int64_t* __restrict__ pair_begin, int64_t Etot, int64_t Gtot, int64_t Npairs,
                                                         const double* __restrict__ err, int n_col, const float* __restrict__ score,
                                                         const double* __restrict__ thr, int n_thr, const int* __restrict__ max_ests,
                                                         int* __restrict__ est_gt, int* __restrict__ gt_est)
{
    __shared__ int order[kMaxGroup];
    const int g = blockIdx.x, tid = threadIdx.x;
    const int n_cfg = n_col * n_thr;                            // <= 256
    const int64_t e0 = est_begin[g], e1 = est_begin[g + 1], t0 = gt_begin[g], t1 = gt_begin[g + 1];
    const int64_t p0 = pair_begin[g], p1 = pair_begin[g + 1];
    const int64_t E64 = e1 - e0, T64 = t1 - t0;
    const bool good = e0 >= 0 && E64 >= 0 && E64 <= kMaxGroup && e1 <= Etot && t0 >= 0 && T64 >= 0 && T64 <= kMaxGroup && t1 <= Gtot &&
                      p0 >= 0 && p1 - p0 == E64 * T64 && p1 <= Npairs;
    if (!good) {                                                // uniform: -1 into at most kMaxGroup of the named entries inside the outputs
        const int64_t ea = clamp64(e0, 0, Etot), eb = clamp64(e1, ea, Etot), ta = clamp64(t0, 0, Gtot), tb = clamp64(t1, ta, Gtot);
        const int ne = static_cast<int>(eb - ea < kMaxGroup ? eb - ea : kMaxGroup), nt = static_cast<int>(tb - ta < kMaxGroup ? tb - ta : kMaxGroup);
        if (tid < n_cfg) {
            for (int e = 0; e < ne; ++e) est_gt[(ea + e) * n_cfg + tid] = -1;
            for (int t = 0; t < nt; ++t) gt_est[(ta + t) * n_cfg + tid] = -1;
        }
        return;
    }
    const int E = static_cast<int>(E64), T = static_cast<int>(T64);
    if (tid < E) {
        const float mine = score[e0 + tid];
        const float s = mine == mine ? mine : -__builtin_huge_valf();           // a NaN score counts as -inf
        int rank = 0;
        for (int o = 0; o < E; ++o) {
            const float theirs = score[e0 + o];
            const float so = theirs == theirs ? theirs : -__builtin_huge_valf();
            rank += (so > s || (so == s && o < tid)) ? 1 : 0;
        }
        order[rank] = tid;
    }
    __syncthreads();
    if (tid >= n_cfg) return;
    const int col = tid / n_thr, k = tid - col * n_thr;
    const double th = thr[static_cast<int64_t>(g) * n_thr + k];
    const int limit = max_ests ? max_ests[g] : 0;
    const int considered = (limit > 0 && limit < E) ? limit : E;
    unsigned long long taken = 0;
    for (int i = 0; i < E; ++i) {
        const int e = order[i];
        int best = -1;
        if (i < considered) {
            const double* row = err + (p0 + static_cast<int64_t>(e) * T) * n_col + col;
            double bv = 0.0;
            for (int t = 0; t < T; ++t) {
                if ((taken >> t) & 1ull) continue;
                const double v = row[static_cast<int64_t>(t) * n_col];
                if (v < th && (best < 0 || v < bv)) { best = t; bv = v; }       // strict: a NaN never matches; ties keep the lower index
            }
            if (best >= 0) {
                taken |= 1ull << best;
                gt_est[(t0 + best) * n_cfg + tid] = e;
            }
        }
        est_gt[(e0 + e) * n_cfg + tid] = best;
    }
    for (int t = 0; t < T; ++t)
        if (!((taken >> t) & 1ull)) gt_est[(t0 + t) * n_cfg + tid] = -1;
}

}  // namespace

extern "C" {

size_t ffb6d_bop_visib_workspace_bytes(int Q, int H, int W)
{
    if (Q <= 0 || Q > 65535 || H <= 0 || W <= 0 || static_cast<int64_t>(H) * W > INT_MAX - kRunPx) return 0;
    const size_t bytes = static_cast<size_t>(Q) * static_cast<size_t>(ffb6d::ceil_div(static_cast<int64_t>(H) * W, kRunPx)) * kRec * sizeof(int);
    return (bytes + 255) / 256 * 256;
}

int ffb6d_bop_visib_f32(const float* depth_test, const float* depth_obj, const int* frame_of, int Q, const double* K, int B, int H,
                        int W, float delta, int* info, double* visib_fract, uint8_t* mask_visib, void* workspace,
                        size_t workspace_bytes, ffb6d_stream_t stream)
{
    FFB6D_REQUIRE(Q >= 0 && Q <= 65535 && B > 0 && H > 0 && W > 0 && static_cast<int64_t>(H) * W <= INT_MAX - kRunPx,
                  "ffb6d_bop_visib_f32: bad sizes Q = %d (at most 65535), B = %d, H = %d, W = %d (H*W < 2^31 - 4096)", Q, B, H, W);
    if (Q == 0) return FFB6D_OK;
    FFB6D_REQUIRE(depth_test && depth_obj && frame_of && K && info && visib_fract, "ffb6d_bop_visib_f32: a null pointer");
    const size_t need = ffb6d_bop_visib_workspace_bytes(Q, H, W);
    if (workspace == nullptr || workspace_bytes < need || !aligned(workspace, 4))
        return ffb6d::set_error(FFB6D_ERR_WORKSPACE, "ffb6d_bop_visib_f32: workspace of %zu bytes, %zu needed (or null, or not 4-byte aligned)",
                                workspace_bytes, need);
    const int HW = H * W;
    const int n_parts = static_cast<int>(ffb6d::ceil_div(HW, kRunPx));
    int* partial = static_cast<int*>(workspace);
    hipStream_t st = ffb6d::as_stream(stream);
    const dim3 grid(static_cast<unsigned>(n_parts), static_cast<unsigned>(Q));
    const bool vec = HW % 4 == 0 && aligned(depth_test, 16) && aligned(depth_obj, 16) && (mask_visib == nullptr || aligned(mask_visib, 4));
    if (vec && mask_visib)
        visib_count_kernel<4, true><<<grid, dim3(kThreads), 0, st>>>(depth_test, depth_obj, frame_of, K, B, HW, W, delta, partial, n_parts, mask_visib);
    else if (vec)
        visib_count_kernel<4, false><<<grid, dim3(kThreads), 0, st>>>(depth_test, depth_obj, frame_of, K, B, HW, W, delta, partial, n_parts, mask_visib);
    else if (mask_visib)
        visib_count_kernel<1, true><<<grid, dim3(kThreads), 0, st>>>(depth_test, depth_obj, frame_of, K, B, HW, W, delta, partial, n_parts, mask_visib);
    else
        visib_count_kernel<1, false><<<grid, dim3(kThreads), 0, st>>>(depth_test, depth_obj, frame_of, K, B, HW, W, delta, partial, n_parts, mask_visib);
    FFB6D_LAUNCH_CHECK();
    visib_finish_kernel<<<dim3(static_cast<unsigned>(Q)), dim3(64), 0, st>>>(frame_of, B, partial, n_parts, info, visib_fract);
    FFB6D_LAUNCH_CHECK();
    return FFB6D_OK;
}

int ffb6d_bop_match_check(const int* host_est_begin, const int* host_gt_begin, const int64_t* host_pair_begin,
                          const int* host_max_ests, int G, int64_t Etot, int64_t Gtot, int64_t Npairs, int n_col, int n_thr)
{
    FFB6D_REQUIRE(G >= 0 && Etot >= 0 && Etot <= INT_MAX && Gtot >= 0 && Gtot <= INT_MAX && Npairs >= 0,
                  "ffb6d_bop_match_check: bad sizes G = %d, Etot = %lld, Gtot = %lld, Npairs = %lld", G, static_cast<long long>(Etot),
                  static_cast<long long>(Gtot), static_cast<long long>(Npairs));
    FFB6D_REQUIRE(n_col >= 1 && n_col <= FFB6D_BOP_MAX_MATCH_COLS && n_thr >= 1 && n_thr <= FFB6D_BOP_MAX_MATCH_THRS,
                  "ffb6d_bop_match_check: n_col = %d, n_thr = %d outside [1, 16]", n_col, n_thr);
    FFB6D_REQUIRE(host_est_begin && host_gt_begin && host_pair_begin, "ffb6d_bop_match_check: a null pointer");
    FFB6D_REQUIRE(host_est_begin[0] == 0 && host_gt_begin[0] == 0 && host_pair_begin[0] == 0 && host_est_begin[G] == Etot &&
                      host_gt_begin[G] == Gtot && host_pair_begin[G] == Npairs,
                  "ffb6d_bop_match_check: the tables do not begin at 0 or do not end at Etot = %lld, Gtot = %lld, Npairs = %lld",
                  static_cast<long long>(Etot), static_cast<long long>(Gtot), static_cast<long long>(Npairs));
    for (int g = 0; g < G; ++g)
        FFB6D_REQUIRE(host_est_begin[g + 1] >= host_est_begin[g] && host_gt_begin[g + 1] >= host_gt_begin[g] &&
                          host_pair_begin[g + 1] >= host_pair_begin[g],
                      "ffb6d_bop_match_check: group %d: the begin tables are not monotone", g);
    for (int g = 0; g < G; ++g) {
        const int64_t E = static_cast<int64_t>(host_est_begin[g + 1]) - host_est_begin[g];
        const int64_t T = static_cast<int64_t>(host_gt_begin[g + 1]) - host_gt_begin[g];
        FFB6D_REQUIRE(E <= kMaxGroup && T <= kMaxGroup, "ffb6d_bop_match_check: group %d has %lld estimates and %lld instances, at most %d of each",
                      g, static_cast<long long>(E), static_cast<long long>(T), kMaxGroup);
        FFB6D_REQUIRE(host_pair_begin[g + 1] - host_pair_begin[g] == E * T,
                      "ffb6d_bop_match_check: group %d: pair_begin advances by %lld for %lld x %lld pairs", g,
                      static_cast<long long>(host_pair_begin[g + 1] - host_pair_begin[g]), static_cast<long long>(E), static_cast<long long>(T));
        FFB6D_REQUIRE(host_max_ests == nullptr || host_max_ests[g] >= 0, "ffb6d_bop_match_check: group %d: max_ests = %d is negative", g,
                      host_max_ests ? host_max_ests[g] : 0);
    }
    return FFB6D_OK;
}

size_t ffb6d_bop_match_workspace_bytes(int, int, int) { return 0; }

int ffb6d_bop_match_f64(const int* est_begin, const int* gt_begin, const int64_t* pair_begin, int G, int64_t Etot, int64_t Gtot,
                        int64_t Npairs, const double* err, int n_col, const float* score, const double* thr, int n_thr,
                        const int* max_ests, int* est_gt, int* gt_est, void*, size_t, ffb6d_stream_t stream)
{
    FFB6D_REQUIRE(G >= 0 && Etot >= 0 && Etot <= INT_MAX && Gtot >= 0 && Gtot <= INT_MAX && Npairs >= 0,
                  "ffb6d_bop_match_f64: bad sizes G = %d, Etot = %lld, Gtot = %lld, Npairs = %lld", G, static_cast<long long>(Etot),
                  static_cast<long long>(Gtot), static_cast<long long>(Npairs));
    FFB6D_REQUIRE(n_col >= 1 && n_col <= FFB6D_BOP_MAX_MATCH_COLS && n_thr >= 1 && n_thr <= FFB6D_BOP_MAX_MATCH_THRS,
                  "ffb6d_bop_match_f64: n_col = %d, n_thr = %d outside [1, 16]", n_col, n_thr);
    if (G == 0) return FFB6D_OK;
    FFB6D_REQUIRE(est_begin && gt_begin && pair_begin && thr && (err || Npairs == 0) && ((score && est_gt) || Etot == 0) && (gt_est || Gtot == 0),
                  "ffb6d_bop_match_f64: a null pointer");
    match_kernel<<<dim3(static_cast<unsigned>(G)), dim3(kThreads), 0, ffb6d::as_stream(stream)>>>(est_begin, gt_begin, pair_begin, Etot, Gtot, Npairs, err,
                                                                                               n_col, score, thr, n_thr, max_ests, est_gt, gt_est);
    FFB6D_LAUNCH_CHECK();
    return FFB6D_OK;
}

}  // extern "C"
