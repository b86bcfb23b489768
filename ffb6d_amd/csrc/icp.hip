// ffb6d_amd/csrc/icp.hip -- gfx950 ICP pose refinement (include/ffb6d_refine.h): point-to-point, scene -> model, every
// (frame, object) pair of a batch in the same launches.  The reference repository has no ICP; the algorithm is stated in
// the header and restated in numpy by tests/icp_ref.py.
//
// The model stays in its own frame: an iteration moves the SCENE points into it (q = R^T (s - t), 3 x 3 floats per problem),
// so whatever is prepared on the model clouds -- Morton order, 64-point tiles, tile boxes -- serves every iteration, frame
// and object.  Per call:
//   icp_select_kernel      one workgroup per problem compacts its scene points (mask == class, keep) once, in index order
//   icp_correspond_kernel  one workgroup per 64 scene points of a problem: nearest model point of each (exact fp32 distance,
//                          ties to the lowest model index), the gate, and the block's 17 partial sums in double
//                          (count, sum m, sum s, sum m s^T, sum d2) -- a fixed butterfly over the 64 lanes
//   icp_solve_kernel       one workgroup per problem: the partial sums added in block order, Kabsch in double (csrc/kabsch.h,
//                          the body of the keypoint fit), the bounding-box convergence test, the problem's state
// A finished problem sets a flag that both kernels read first: no host polling, no read-back, the call never waits.
//
// Several instances of a class (the *_inst calls; the rule is in the header): problems are (frame, class, instance).
//   map      icp_select_kernel<.., kInst> also tests the instance map; the loop is the one above on those sets
//   nearest  the sets are the class's points; per iteration icp_correspond_kernel writes every problem's distances (stopped
//            problems too: they go on competing under their pose), icp_claim_kernel -- one wavefront per (problem, 64 scene
//            points), lane = scene point -- reads the rows of the problem's group (icp_groups_kernel: the run of adjacent
//            problems with its frame and class), keeps the pairs the problem owns and makes the block's sums with the same
//            butterfly; icp_solve_kernel is unchanged
//   icp_inst_out_kernel writes the refined instance map from the kept pairs the loop left.
//
// Two forms of the search, identical results (the comparison is on (d2 bits, model index) as one 64-bit key, and a tile is
// skipped only when its box is STRICTLY farther than the best distance; the box distance is rounded like the point distance,
// so it never exceeds the distance of a point inside the box):
//   scan    lane = scene point; the class's cloud streams through LDS in 1024-point chunks, the four wavefronts take the
//           chunk's tiles in turn (same-address LDS reads: broadcast) and meet in LDS
//   pruned  wavefront = one scene point at a time, lane = model point of a tile: the lanes first measure the tile boxes
//           (64 boxes per step), the nearest box is visited first, then only the boxes that are not farther than the best
//           distance so far.  The skip test is wave-uniform by construction, so it pays although neighbouring scene points
//           of a block lie anywhere on the object (they are in cloud order).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "common.h"
#include "ffb6d_refine.h"
#include "kabsch.h"

namespace {

using ffb6d::ceil_div;

constexpr int kBlock = 256;
constexpr int kTilePts = 64;                  // scene points per workgroup = model points per tile = lanes
constexpr int kChunk = 1024;                  // model points in LDS per step of the scan form (16 KB)
constexpr int kSums = 17;                     // count, sum m (3), sum s (3), sum m s^T (9), sum d2
constexpr int kPlaneSums = 30;                // count, sum d2, sum r^2, the 21 upper entries of sum a a^T (row by row), sum a r (6)
constexpr int kNormalK = 16;                  // neighbours of the estimated normals
constexpr int kPoint = 0, kPlane = 1;         // the metric the sums and the update are made for
constexpr int kPrunedMin = 1024;              // form -1 (automatic): classes of at least this many points take the pruned form
constexpr int kNoIndex = 0x7fffffff;
constexpr unsigned long long kNoKey = (0x7f800000ull << 32) | 0x7fffffffull;      // (+inf, no index): loses against every point

struct ClassInfo { int pt_begin, count, tile_begin, n_tiles; };

struct Prepared {
    const ClassInfo* cls;                     // [n_cls]
    const float4* cls_lo;                     // [n_cls] bounding box of the class
    const float4* cls_hi;
    const float4* orig;                       // [total] the clouds in their own order
    const float4* sorted;                     // [max_tiles * 64] {x, y, z, index within the class}, Morton order, NaN padding
    const float4* tile_lo;                    // [max_tiles]
    const float4* tile_hi;
};

size_t align256(size_t x) { return (x + 255) & ~static_cast<size_t>(255); }

struct Layout { size_t cls, cls_box, orig, sorted, tile_box, bytes; int64_t max_tiles; };

Layout prepared_layout(int64_t total, int n_cls) {
    Layout l;
    l.max_tiles = total / kTilePts + n_cls;   // >= sum over the classes of ceil(count / 64)
    l.cls = 0;
    l.cls_box = l.cls + align256(sizeof(ClassInfo) * n_cls);
    l.orig = l.cls_box + align256(2 * sizeof(float4) * n_cls);
    l.sorted = l.orig + align256(sizeof(float4) * static_cast<size_t>(total));
    l.tile_box = l.sorted + align256(sizeof(float4) * static_cast<size_t>(l.max_tiles) * kTilePts);
    l.bytes = l.tile_box + align256(2 * sizeof(float4) * static_cast<size_t>(l.max_tiles));
    return l;
}

Prepared prepared_view(const void* base, const Layout& l, int n_cls) {
    const char* b = static_cast<const char*>(base);
    Prepared m;
    m.cls = reinterpret_cast<const ClassInfo*>(b + l.cls);
    m.cls_lo = reinterpret_cast<const float4*>(b + l.cls_box);
    m.cls_hi = m.cls_lo + n_cls;
    m.orig = reinterpret_cast<const float4*>(b + l.orig);
    m.sorted = reinterpret_cast<const float4*>(b + l.sorted);
    m.tile_lo = reinterpret_cast<const float4*>(b + l.tile_box);
    m.tile_hi = m.tile_lo + l.max_tiles;
    return m;
}

// ---- the arithmetic the header states, every operation rounded on its own -----------------------------------------
__device__ __forceinline__ float dist2(float qx, float qy, float qz, float mx, float my, float mz) {
    const float dx = __fsub_rn(qx, mx), dy = __fsub_rn(qy, my), dz = __fsub_rn(qz, mz);
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

// lower bound of dist2 over the points of a box: per axis fl(lo - q) <= fl(p - q) for p >= lo (rounding is monotone), and
// squares and sums of non-negative terms keep the order.  A NaN coordinate gives 0 (the tile is visited).
__device__ __forceinline__ float box_dist2(float qx, float qy, float qz, const float4 lo, const float4 hi) {
    const float ex = fmaxf(fmaxf(__fsub_rn(lo.x, qx), __fsub_rn(qx, hi.x)), 0.f);
    const float ey = fmaxf(fmaxf(__fsub_rn(lo.y, qy), __fsub_rn(qy, hi.y)), 0.f);
    const float ez = fmaxf(fmaxf(__fsub_rn(lo.z, qz), __fsub_rn(qz, hi.z)), 0.f);
    return __fadd_rn(__fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey)), __fmul_rn(ez, ez));
}

// distances are >= +0 or NaN: their order is the order of their bits, NaN above +inf
__device__ __forceinline__ unsigned long long make_key(float d2, float index_bits) {
    return (static_cast<unsigned long long>(__float_as_uint(d2)) << 32) | static_cast<unsigned long long>(__float_as_uint(index_bits));
}

__device__ __forceinline__ unsigned long long wave_min_key(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(v, o);
        v = other < v ? other : v;
    }
    return v;
}

__device__ __forceinline__ double shfl_xor_f64(double v, int o) {
    return __builtin_bit_cast(double, __shfl_xor(__builtin_bit_cast(unsigned long long, v), o));
}

__device__ __forceinline__ unsigned long long visit_tile(const float4* __restrict__ sorted, int t, int lane, float qx, float qy, float qz) {
    const float4 m = sorted[static_cast<int64_t>(t) * kTilePts + lane];
    return wave_min_key(make_key(dist2(qx, qy, qz, m.x, m.y, m.z), m.w));
}

// q = R^T (s - t), step 1: every product and sum rounded
__device__ __forceinline__ void to_model_frame(const float* __restrict__ Rt, const float4 s, float& qx, float& qy, float& qz) {
    const float d0 = __fsub_rn(s.x, Rt[3]), d1 = __fsub_rn(s.y, Rt[7]), d2s = __fsub_rn(s.z, Rt[11]);
    qx = __fadd_rn(__fadd_rn(__fmul_rn(d0, Rt[0]), __fmul_rn(d1, Rt[4])), __fmul_rn(d2s, Rt[8]));
    qy = __fadd_rn(__fadd_rn(__fmul_rn(d0, Rt[1]), __fmul_rn(d1, Rt[5])), __fmul_rn(d2s, Rt[9]));
    qz = __fadd_rn(__fadd_rn(__fmul_rn(d0, Rt[2]), __fmul_rn(d1, Rt[6])), __fmul_rn(d2s, Rt[10]));
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += shfl_xor_f64(v, o);
    return v;
}

// centre c and half diagonal rho of a class's bounding box, in double from the float32 box
__device__ __forceinline__ double box_centre(const float4 lo, const float4 hi, double* c) {
    const double ex = static_cast<double>(hi.x) - lo.x, ey = static_cast<double>(hi.y) - lo.y, ez = static_cast<double>(hi.z) - lo.z;
    c[0] = 0.5 * (static_cast<double>(lo.x) + hi.x);
    c[1] = 0.5 * (static_cast<double>(lo.y) + hi.y);
    c[2] = 0.5 * (static_cast<double>(lo.z) + hi.z);
    return 0.5 * sqrt(ex * ex + ey * ey + ez * ez);
}

// what the plane metric adds to a pair: the model normals of the class (its own order), the scene point in the model frame
// (step 1) and the class constants
struct PlanePair {
    const float4* normals;
    float qx, qy, qz;
    double c[3], rho;
};

// The sums of step 4 / 4p over a block of 64 scene points (lane = scene point, the whole wavefront calls): a kept lane adds its
// pair (model point cloud[idx], scene point s, distance d2), the fixed butterfly adds the lanes, lane 0 stores.
//   kPoint  17 doubles, all held by the lane and reduced in turn
//   kPlane  30 doubles; the lane holds a (6) and r and reduces one product at a time, so the 30 are never live together
template <int kMetric>
__device__ __forceinline__ void block_sums(bool kept, const float4* __restrict__ cloud, int idx, const float4 s, float d2, int lane,
                                           double* __restrict__ out, const PlanePair& pp) {
    if constexpr (kMetric == kPoint) {
        double v[kSums];
#pragma unroll
        for (int k = 0; k < kSums; ++k) v[k] = 0.0;
        if (kept) {
            const float4 m = cloud[idx];
            const double mm[3] = {m.x, m.y, m.z}, ss[3] = {s.x, s.y, s.z};
            v[0] = 1.0;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                v[1 + r] = mm[r];
                v[4 + r] = ss[r];
#pragma unroll
                for (int c = 0; c < 3; ++c) v[7 + 3 * r + c] = mm[r] * ss[c];
            }
            v[16] = d2;
        }
#pragma unroll
        for (int k = 0; k < kSums; ++k) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v[k] += shfl_xor_f64(v[k], o);
        }
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < kSums; ++k) out[k] = v[k];
        }
    } else {
        double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, r = 0.0, one = 0.0, dd = 0.0;
        if (kept) {
            const float4 m = cloud[idx], nf = pp.normals[idx];
            const double n[3] = {nf.x, nf.y, nf.z};
            const double e[3] = {static_cast<double>(pp.qx) - m.x, static_cast<double>(pp.qy) - m.y, static_cast<double>(pp.qz) - m.z};
            const double u[3] = {(pp.qx - pp.c[0]) / pp.rho, (pp.qy - pp.c[1]) / pp.rho, (pp.qz - pp.c[2]) / pp.rho};
            a[0] = u[1] * n[2] - u[2] * n[1];
            a[1] = u[2] * n[0] - u[0] * n[2];
            a[2] = u[0] * n[1] - u[1] * n[0];
            a[3] = n[0];
            a[4] = n[1];
            a[5] = n[2];
            r = (n[0] * e[0] + n[1] * e[1] + n[2] * e[2]) / pp.rho;
            one = 1.0;
            dd = d2;
        }
        double t;
        t = wave_sum(one);
        if (lane == 0) out[0] = t;
        t = wave_sum(dd);
        if (lane == 0) out[1] = t;
        t = wave_sum(r * r);
        if (lane == 0) out[2] = t;
        int k = 3;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
#pragma unroll
            for (int j = i; j < 6; ++j) {
                t = wave_sum(a[i] * a[j]);
                if (lane == 0) out[k] = t;
                ++k;
            }
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            t = wave_sum(a[i] * r);
            if (lane == 0) out[24 + i] = t;
        }
    }
}

// ---- scene sets ------------------------------------------------------------------------------------------------------
// kInst: the map form of the instance calls -- a point is taken only when inst[frame, i] == inst_of[p] as well
template <typename MaskT, bool kInst>
__global__ __launch_bounds__(kBlock) void icp_select_kernel(
    const float* __restrict__ pcld, const MaskT* __restrict__ mask, const unsigned char* __restrict__ keep,
    const unsigned char* __restrict__ inst, const int* __restrict__ frame_of, const int* __restrict__ class_of,
    const int* __restrict__ inst_of, int B, int N, int64_t stride, float4* __restrict__ sets, int* __restrict__ counts) {
    __shared__ int wave_total[kBlock / 64];
    const int p = blockIdx.x;
    const int b = frame_of[p];
    int want = 0;
    if (kInst) want = inst_of[p];
    if (b < 0 || b >= B || (kInst && (want < 1 || want > 255))) {      // never an index / an id: a problem without scene points
        if (threadIdx.x == 0) counts[p] = 0;
        return;
    }
    const MaskT cls = static_cast<MaskT>(class_of[p]);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int base = 0;
    for (int i0 = 0; i0 < N; i0 += kBlock) {
        const int i = i0 + threadIdx.x;
        bool sel = false;
        if (i < N) sel = mask[static_cast<int64_t>(b) * N + i] == cls && (!keep || keep[static_cast<int64_t>(b) * N + i]);
        if (kInst && sel) sel = inst[static_cast<int64_t>(b) * N + i] == want;
        const unsigned long long bal = __ballot(sel);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        __syncthreads();
        if (lane == 0) wave_total[wave] = __popcll(bal);
        __syncthreads();
        int pos = base + before, total = 0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) {
            if (w < wave) pos += wave_total[w];
            total += wave_total[w];
        }
        if (sel) {
            const float* pt = pcld + (static_cast<int64_t>(b) * N + i) * 3;
            sets[static_cast<int64_t>(p) * stride + pos] = make_float4(pt[0], pt[1], pt[2], __int_as_float(i));
        }
        base += total;
    }
    if (threadIdx.x == 0) counts[p] = base;
}

__global__ __launch_bounds__(kBlock) void icp_fill_kernel(int* __restrict__ idx, float* __restrict__ d2, int64_t n) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= n) return;
    if (idx) idx[i] = -1;
    if (d2) d2[i] = __uint_as_float(0x7f800000u);
}

// ---- correspondences + partial sums -------------------------------------------------------------------------------
struct CorrArgs {
    const float4* sets;
    const int* counts;
    int64_t stride;
    const int* class_of;
    const double* T;
    const int* done;                          // or NULL
    Prepared m;
    int n_cls;
    float max_d2;
    int form;
    int* idx_out;                             // or NULL
    float* d2_out;                            // or NULL
    double* partials;                         // or NULL
    int tiles;                                // blocks per problem in `partials`
    unsigned long long* pairs;                // or NULL
    const float4* normals;                    // the plane metric: [total] {nx, ny, nz, 0} in the clouds' own order
};

template <int kMetric>
__global__ __launch_bounds__(kBlock) void icp_correspond_kernel(const CorrArgs a) {
    __shared__ float4 chunk[kChunk];
    __shared__ float4 qs[kTilePts];
    __shared__ unsigned long long wkey[kBlock / 64][kTilePts];
    const int p = blockIdx.y, tile = blockIdx.x;
    if (a.done && a.done[p]) return;
    const int cnt = a.counts[p];
    const int q0 = tile * kTilePts;
    if (q0 >= cnt) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cls = a.class_of[p];
    ClassInfo ci = {0, 0, 0, 0};
    if (cls >= 0 && cls < a.n_cls) ci = a.m.cls[cls];           // (a class id that is no index: no model points)
    float Rt[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) Rt[k] = static_cast<float>(a.T[static_cast<int64_t>(p) * 12 + k]);
    const float4 s = a.sets[static_cast<int64_t>(p) * a.stride + min(q0 + lane, cnt - 1)];
    float qx, qy, qz;
    to_model_frame(Rt, s, qx, qy, qz);
    const float4* __restrict__ sorted = a.m.sorted + static_cast<int64_t>(ci.tile_begin) * kTilePts;
    const int n_valid = min(kTilePts, cnt - q0);
    const bool pruned = a.form == 1 || (a.form < 0 && ci.count >= kPrunedMin);
    unsigned long long wave_pairs = 0;

    if (!pruned) {
        unsigned long long best = kNoKey;
        const int n_pad = ci.n_tiles * kTilePts;
        const float nanf_ = __uint_as_float(0x7fc00000u);
        for (int j0 = 0; j0 < n_pad; j0 += kChunk) {
            __syncthreads();
            for (int x = tid; x < kChunk; x += kBlock) {
                const int j = j0 + x;
                chunk[x] = j < n_pad ? sorted[j] : make_float4(nanf_, nanf_, nanf_, __int_as_float(kNoIndex));
            }
            __syncthreads();
            const int n = min(kChunk, n_pad - j0);
            for (int x0 = wave * kTilePts; x0 < n; x0 += kBlock) {
#pragma unroll 8
                for (int k = 0; k < kTilePts; ++k) {
                    const float4 m = chunk[x0 + k];
                    const unsigned long long key = make_key(dist2(qx, qy, qz, m.x, m.y, m.z), m.w);
                    best = key < best ? key : best;
                }
                wave_pairs += static_cast<unsigned long long>(kTilePts) * n_valid;
            }
        }
        wkey[wave][lane] = best;
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int w = 1; w < kBlock / 64; ++w) best = wkey[w][lane] < best ? wkey[w][lane] : best;
            wkey[0][lane] = best;
        }
    } else {
        if (wave == 0) qs[lane] = make_float4(qx, qy, qz, 0.f);
        __syncthreads();
        const int T = ci.n_tiles;
        const float4* __restrict__ tlo = a.m.tile_lo + ci.tile_begin;
        const float4* __restrict__ thi = a.m.tile_hi + ci.tile_begin;
        constexpr int kPer = kTilePts / (kBlock / 64);          // scene points per wavefront
        for (int i = 0; i < kPer; ++i) {
            const int pi = wave * kPer + i;
            if (pi >= n_valid) break;
            const float4 qq = qs[pi];
            unsigned long long bk = kNoKey;
            if (T > 0) {
                unsigned long long near = ~0ull;
                for (int g = 0; g < T; g += 64) {
                    const int t = g + lane;
                    if (t < T) {
                        const unsigned long long k = (static_cast<unsigned long long>(__float_as_uint(box_dist2(qq.x, qq.y, qq.z, tlo[t], thi[t]))) << 32) | static_cast<unsigned>(t);
                        near = k < near ? k : near;
                    }
                }
                near = wave_min_key(near);
                const int t_first = static_cast<int>(near & 0xffffffffull);
                bk = visit_tile(sorted, t_first, lane, qq.x, qq.y, qq.z);
                wave_pairs += kTilePts;
                for (int g = 0; g < T; g += 64) {
                    const int t = g + lane;
                    float bd = 0.f;
                    bool cand = false;
                    if (t < T && t != t_first) {
                        bd = box_dist2(qq.x, qq.y, qq.z, tlo[t], thi[t]);
                        cand = !(bd > __uint_as_float(static_cast<unsigned>(bk >> 32)));
                    }
                    unsigned long long todo = __ballot(cand);
                    while (todo) {
                        const int l = __ffsll(static_cast<long long>(todo)) - 1;
                        todo &= todo - 1;
                        if (__shfl(bd, l, 64) > __uint_as_float(static_cast<unsigned>(bk >> 32))) continue;      // the best has improved since
                        const unsigned long long k = visit_tile(sorted, g + l, lane, qq.x, qq.y, qq.z);
                        bk = k < bk ? k : bk;
                        wave_pairs += kTilePts;
                    }
                }
            }
            if (lane == 0) wkey[0][pi] = bk;
        }
        __syncthreads();
    }
    if (a.pairs && lane == 0 && wave_pairs) atomicAdd(a.pairs, wave_pairs);
    if (wave != 0) return;

    // the gate, the outputs of the single step, the block's sums
    const bool valid = lane < n_valid;
    const unsigned long long key = valid ? wkey[0][lane] : kNoKey;
    const int idx = static_cast<int>(key & 0xffffffffull);
    float d2 = __uint_as_float(static_cast<unsigned>(key >> 32));
    const bool matched = idx != kNoIndex;
    if (!matched) d2 = ci.count > 0 ? __uint_as_float(0x7fc00000u) : __uint_as_float(0x7f800000u);   // every distance NaN / no model
    if (d2 != d2) d2 = __uint_as_float(0x7fc00000u);
    const bool kept = valid && matched && d2 <= a.max_d2;       // (false for NaN)
    if (valid) {
        const int64_t at = static_cast<int64_t>(p) * a.stride + q0 + lane;
        if (a.idx_out) a.idx_out[at] = kept ? idx : -1;
        if (a.d2_out) a.d2_out[at] = d2;
    }
    if (!a.partials) return;
    constexpr int kN = kMetric == kPlane ? kPlaneSums : kSums;
    PlanePair pp;
    if constexpr (kMetric == kPlane) {
        pp.normals = a.normals + ci.pt_begin;
        pp.qx = qx; pp.qy = qy; pp.qz = qz;
        pp.rho = 0.0;
        pp.c[0] = pp.c[1] = pp.c[2] = 0.0;
        if (ci.count > 0) pp.rho = box_centre(a.m.cls_lo[cls], a.m.cls_hi[cls], pp.c);
    }
    block_sums<kMetric>(kept, a.m.orig + ci.pt_begin, idx, s, d2, lane, a.partials + (static_cast<int64_t>(p) * a.tiles + tile) * kN, pp);
}

// ---- nearest mode: the instances of a (frame, class) compete for every point ---------------------------------------------
// group of p = the maximal run of adjacent problems with its frame and class: {begin, end} per problem, once per call
__global__ __launch_bounds__(kBlock) void icp_groups_kernel(const int* __restrict__ frame_of, const int* __restrict__ class_of, int P, int nearest,
                                                            int2* __restrict__ groups) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= P) return;
    int lo = p, hi = p + 1;
    if (nearest) {
        const int f = frame_of[p], c = class_of[p];
        while (lo > 0 && frame_of[lo - 1] == f && class_of[lo - 1] == c) --lo;
        while (hi < P && frame_of[hi] == f && class_of[hi] == c) ++hi;
    }
    int2 g;
    g.x = lo;
    g.y = hi;
    groups[p] = g;
}

struct ClaimArgs {
    const float4* sets;
    const int* counts;
    int64_t stride;
    const int* class_of;
    const int2* groups;
    Prepared m;
    int n_cls;
    const float* d2_rows;                     // [P, stride] every problem's own smallest distance (icp_correspond_kernel)
    const int* idx_rows;                      // [P, stride] its model point, -1 where its own gate drops the pair
    int* idx_out;                             // or NULL; may be idx_rows
    float* d2_out;                            // or NULL
    int* owner_out;                           // or NULL
    double* partials;                         // or NULL
    int tiles;
    const float4* normals;                    // the plane metric (as CorrArgs), and the poses the rows were measured under
    const double* T;
};

// One wavefront per (problem, block of 64 scene points), lane = scene point: the rows of a group are aligned (its members have
// the same scene set), so every member's distance to the lane's point is one coalesced read.  The owner is the member with the
// smallest distance (float compare: a NaN never owns, the first of equals stays); the pair survives when p owns it.
template <int kMetric>
__global__ __launch_bounds__(64) void icp_claim_kernel(const ClaimArgs a) {
    const int p = blockIdx.y, tile = blockIdx.x, lane = threadIdx.x;
    const int cnt = a.counts[p];
    const int q0 = tile * kTilePts;
    if (q0 >= cnt) return;
    const bool valid = q0 + lane < cnt;
    const int64_t j = q0 + min(lane, cnt - 1 - q0);
    const int2 g = a.groups[p];
    int owner = -1;
    float best = 0.f;
    for (int q = g.x; q < g.y; ++q) {
        const float d = a.d2_rows[static_cast<int64_t>(q) * a.stride + j];
        if (d == d && (owner < 0 || d < best)) {
            owner = q;
            best = d;
        }
    }
    const int64_t at = static_cast<int64_t>(p) * a.stride + j;
    const int idx = a.idx_rows[at];
    const float d2 = a.d2_rows[at];
    const bool kept = valid && owner == p && idx >= 0;
    if (valid) {
        if (a.idx_out) a.idx_out[at] = kept ? idx : -1;
        if (a.d2_out) a.d2_out[at] = d2;
        if (a.owner_out) a.owner_out[at] = owner;
    }
    if (!a.partials) return;
    const int cls = a.class_of[p];
    int pt_begin = 0;
    if (cls >= 0 && cls < a.n_cls) pt_begin = a.m.cls[cls].pt_begin;
    constexpr int kN = kMetric == kPlane ? kPlaneSums : kSums;
    const float4 s = a.sets[at];
    PlanePair pp;
    if constexpr (kMetric == kPlane) {                          // step 1 again: the bits icp_correspond_kernel measured with
        float Rt[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) Rt[k] = static_cast<float>(a.T[static_cast<int64_t>(p) * 12 + k]);
        to_model_frame(Rt, s, pp.qx, pp.qy, pp.qz);
        pp.normals = a.normals + pt_begin;
        pp.rho = 0.0;
        pp.c[0] = pp.c[1] = pp.c[2] = 0.0;
        if (cls >= 0 && cls < a.n_cls && a.m.cls[cls].count > 0) pp.rho = box_centre(a.m.cls_lo[cls], a.m.cls_hi[cls], pp.c);
    }
    block_sums<kMetric>(kept, a.m.orig + pt_begin, idx, s, d2, lane, a.partials + (static_cast<int64_t>(p) * a.tiles + tile) * kN, pp);
}

// inst_out[frame, i] = inst_of[p] for the kept pairs of the idx rows as the loop left them (one writer per point)
__global__ __launch_bounds__(kBlock) void icp_inst_out_kernel(const float4* __restrict__ sets, const int* __restrict__ counts, int64_t stride,
                                                              const int* __restrict__ idx_rows, const int* __restrict__ frame_of,
                                                              const int* __restrict__ inst_of, int N, unsigned char* __restrict__ inst_out) {
    const int p = blockIdx.y;
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= counts[p]) return;                                 // (a frame that is no index has no scene points)
    const int64_t at = static_cast<int64_t>(p) * stride + j;
    if (idx_rows[at] < 0) return;
    inst_out[static_cast<int64_t>(frame_of[p]) * N + __float_as_int(sets[at].w)] = static_cast<unsigned char>(inst_of[p]);
}

// ---- the update -----------------------------------------------------------------------------------------------------
struct SolveArgs {
    const int* counts;
    const int* class_of;
    Prepared m;
    int n_cls;
    const double* partials;
    int tiles;
    double* T;
    int* done;
    int* iters;
    int* n_pairs;
    float* rms;
    int min_pairs;
    double tol;
    float* rms_plane;                         // the plane metric only
    double min_eig;
};

// the stop rule on the box corners: no corner of the class's bounding box moved by more than tol between the poses To and Tn
__device__ inline bool box_converged(const SolveArgs& a, int cls, const double* To, const double* Tn) {
    if (!(a.tol > 0 && cls >= 0 && cls < a.n_cls)) return false;
    const float4 lo = a.m.cls_lo[cls], hi = a.m.cls_hi[cls];
    double mv = 0.0;
    for (int c8 = 0; c8 < 8; ++c8) {
        const double x = (c8 & 1) ? hi.x : lo.x, y = (c8 & 2) ? hi.y : lo.y, z = (c8 & 4) ? hi.z : lo.z;
        double e2 = 0.0;
        for (int r = 0; r < 3; ++r) {
            const double dn = Tn[4 * r] * x + Tn[4 * r + 1] * y + Tn[4 * r + 2] * z + Tn[4 * r + 3];
            const double dp = To[4 * r] * x + To[4 * r + 1] * y + To[4 * r + 2] * z + To[4 * r + 3];
            e2 += (dn - dp) * (dn - dp);
        }
        mv = fmax(mv, sqrt(e2));
    }
    return mv <= a.tol;
}

__global__ __launch_bounds__(64) void icp_solve_kernel(const SolveArgs a) {
    __shared__ double sh[kSums];
    const int p = blockIdx.x;
    if (a.done[p]) return;
    const int nt = (a.counts[p] + kTilePts - 1) / kTilePts;
    const int k = threadIdx.x;
    if (k < kSums) {
        double s = 0.0;
        for (int t = 0; t < nt; ++t) s += a.partials[(static_cast<int64_t>(p) * a.tiles + t) * kSums + k];      // block order
        sh[k] = s;
    }
    __syncthreads();
    if (k != 0) return;
    const double n = sh[0];
    a.n_pairs[p] = static_cast<int>(n);
    a.rms[p] = n > 0 ? static_cast<float>(sqrt(sh[16] / n)) : 0.f;
    if (n < static_cast<double>(a.min_pairs)) {                 // too few pairs: the pose stays, the problem is over
        a.done[p] = 1;
        return;
    }
    double ca[3], cb[3], H[3][3];
    for (int r = 0; r < 3; ++r) {
        ca[r] = sh[1 + r] / n;
        cb[r] = sh[4 + r] / n;
    }
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) H[r][c] = sh[7 + 3 * r + c] - n * ca[r] * cb[c];      // sum (m - ca)(s - cb)^T
    double Tn[12];
    ffb6d::kabsch_from_covariance(H, ca, cb, Tn);
    double* To = a.T + static_cast<int64_t>(p) * 12;
    const bool conv = box_converged(a, a.class_of[p], To, Tn);
    for (int i = 0; i < 12; ++i) To[i] = Tn[i];
    a.iters[p] += 1;
    if (conv) a.done[p] = 1;
}

// Eigen-decomposition of a symmetric 6 x 6 matrix by cyclic two-sided Jacobi, the contract of jacobi_svd3 (csrc/kabsch.h): the pair
// (p, q) is rotated while |M_pq| > 1.5 * 2^-52 sqrt(M_pp M_qq) -- false for NaN, for a zero and for a negative diagonal entry -- and
// the number of sweeps is bounded.  On exit the diagonal of M holds the eigenvalues and the columns of V the eigenvectors.  Every
// index is a compile-time constant after unrolling (the matrices stay in registers); a zero row and column is never touched, so
// the directions a planar model leaves free come out as eigenvalues that are exactly zero.
__device__ inline void jacobi_eig6(double M[6][6], double V[6][6]) {
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) V[i][j] = i == j;
    for (int sweep = 0; sweep < 30; ++sweep) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < 5; ++p)
#pragma unroll
            for (int q = p + 1; q < 6; ++q) {
                const double apq = M[p][q];
                if (!(fabs(apq) > 0x1.8p-52 * sqrt(M[p][p] * M[q][q]))) continue;
                rotated = true;
                const double zeta = (M[q][q] - M[p][p]) / (2.0 * apq);
                const double tt = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(zeta * zeta + 1.0));
                const double cs = 1.0 / sqrt(tt * tt + 1.0), sn = tt * cs;
#pragma unroll
                for (int k = 0; k < 6; ++k) {      // M <- M J
                    const double mkp = M[k][p], mkq = M[k][q];
                    M[k][p] = cs * mkp - sn * mkq;
                    M[k][q] = sn * mkp + cs * mkq;
                }
#pragma unroll
                for (int k = 0; k < 6; ++k) {      // M <- J^T M
                    const double mpk = M[p][k], mqk = M[q][k];
                    M[p][k] = cs * mpk - sn * mqk;
                    M[q][k] = sn * mpk + cs * mqk;
                }
                M[p][q] = M[q][p] = 0.0;           // (what the rotation was chosen for)
#pragma unroll
                for (int k = 0; k < 6; ++k) {      // V <- V J
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = cs * vkp - sn * vkq;
                    V[k][q] = sn * vkp + cs * vkq;
                }
            }
        if (!rotated) break;
    }
}

// Step 5p: one lane per problem, in double.  The sums are added in block order by 30 lanes, as icp_solve_kernel adds its 17.
__global__ __launch_bounds__(64) void icp_solve_plane_kernel(const SolveArgs a) {
    __shared__ double sh[kPlaneSums];
    const int p = blockIdx.x;
    if (a.done[p]) return;
    const int nt = (a.counts[p] + kTilePts - 1) / kTilePts;
    const int k = threadIdx.x;
    if (k < kPlaneSums) {
        double s = 0.0;
        for (int t = 0; t < nt; ++t) s += a.partials[(static_cast<int64_t>(p) * a.tiles + t) * kPlaneSums + k];      // block order
        sh[k] = s;
    }
    __syncthreads();
    if (k != 0) return;
    const double n = sh[0];
    const int cls = a.class_of[p];
    double c[3] = {0.0, 0.0, 0.0}, rho = 0.0;
    if (cls >= 0 && cls < a.n_cls && a.m.cls[cls].count > 0) rho = box_centre(a.m.cls_lo[cls], a.m.cls_hi[cls], c);
    a.n_pairs[p] = static_cast<int>(n);
    a.rms[p] = n > 0 ? static_cast<float>(sqrt(sh[1] / n)) : 0.f;
    a.rms_plane[p] = n > 0 && rho > 0 ? static_cast<float>(sqrt(rho * rho * sh[2] / n)) : 0.f;
    if (n < static_cast<double>(a.min_pairs) || !(rho > 0)) {   // too few pairs, a class without extent: the pose stays
        a.done[p] = 1;
        return;
    }
    double M[6][6], V[6][6], g[6];
    {
        int at = 3;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = i; j < 6; ++j) {
                M[i][j] = M[j][i] = sh[at];
                ++at;
            }
#pragma unroll
        for (int i = 0; i < 6; ++i) g[i] = sh[24 + i];
    }
    jacobi_eig6(M, V);
    double lmax = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) lmax = fmax(lmax, M[i][i]);
    double x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int e = 0; e < 6; ++e) {
        const double lam = M[e][e];
        if (!(lam > 0 && lam >= a.min_eig * lmax)) continue;    // the direction is left where it is
        double vg = 0.0;
#pragma unroll
        for (int i = 0; i < 6; ++i) vg += V[i][e] * g[i];
        const double f = vg / lam;
#pragma unroll
        for (int i = 0; i < 6; ++i) x[i] -= V[i][e] * f;
    }
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 6; ++i) finite = finite && fabs(x[i]) <= 1.7976931348623157e308;      // (false for NaN and inf)
    if (!finite) {
        a.done[p] = 1;
        return;
    }
    // Rd = exp([w]x) by Rodrigues; below theta = 1e-4 the series of sin t / t and (1 - cos t) / t^2 (their next terms are < 1e-18)
    const double th2 = x[0] * x[0] + x[1] * x[1] + x[2] * x[2], th = sqrt(th2);
    double A, Bc;
    if (th < 1e-4) {
        A = 1.0 - th2 / 6.0;
        Bc = 0.5 - th2 / 24.0;
    } else {
        A = sin(th) / th;
        Bc = (1.0 - cos(th)) / th2;
    }
    const double K[3][3] = {{0.0, -x[2], x[1]}, {x[2], 0.0, -x[0]}, {-x[1], x[0], 0.0}};
    double Rd[3][3];
    for (int r = 0; r < 3; ++r)
        for (int q = 0; q < 3; ++q) {
            double kk = 0.0;
            for (int j = 0; j < 3; ++j) kk += K[r][j] * K[j][q];
            Rd[r][q] = (r == q ? 1.0 : 0.0) + A * K[r][q] + Bc * kk;
        }
    double d[3];
    for (int r = 0; r < 3; ++r) d[r] = c[r] - (Rd[r][0] * c[0] + Rd[r][1] * c[1] + Rd[r][2] * c[2]) + rho * x[3 + r];
    double* To = a.T + static_cast<int64_t>(p) * 12;
    double Tn[12];
    for (int r = 0; r < 3; ++r)                                 // R <- R Rd^T
        for (int q = 0; q < 3; ++q) Tn[4 * r + q] = To[4 * r] * Rd[q][0] + To[4 * r + 1] * Rd[q][1] + To[4 * r + 2] * Rd[q][2];
    for (int r = 0; r < 3; ++r) Tn[4 * r + 3] = To[4 * r + 3] - (Tn[4 * r] * d[0] + Tn[4 * r + 1] * d[1] + Tn[4 * r + 2] * d[2]);
    const bool conv = box_converged(a, cls, To, Tn);
    for (int i = 0; i < 12; ++i) To[i] = Tn[i];
    a.iters[p] += 1;
    if (conv) a.done[p] = 1;
}

// ---- model normals -----------------------------------------------------------------------------------------------------
// One lane per model point of a class: the covariance of its k nearest points of the class (rows of `knn`, itself included)
// about their own mean, in double from the float32 points; the normal is the singular vector of the smallest singular value
// (jacobi_svd3), normalised, its component of largest magnitude positive (the lowest axis on ties).  The zero vector when
// n < 3 or the second singular value is zero.
__global__ __launch_bounds__(kBlock) void icp_normals_kernel(const float* __restrict__ pts, const int* __restrict__ knn, int n, int k,
                                                            float4* __restrict__ normals) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    double nv[3] = {0.0, 0.0, 0.0};
    if (n >= 3 && k >= 1) {
        const int* row = knn + static_cast<int64_t>(j) * k;
        double mean[3] = {0.0, 0.0, 0.0};
        for (int i = 0; i < k; ++i) {
            const float* pt = pts + static_cast<int64_t>(min(max(row[i], 0), n - 1)) * 3;
            for (int a = 0; a < 3; ++a) mean[a] += pt[a];
        }
        for (int a = 0; a < 3; ++a) mean[a] /= k;
        double G[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}}, V[3][3];
        for (int i = 0; i < k; ++i) {
            const float* pt = pts + static_cast<int64_t>(min(max(row[i], 0), n - 1)) * 3;
            const double e[3] = {pt[0] - mean[0], pt[1] - mean[1], pt[2] - mean[2]};
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) G[a][b] += e[a] * e[b];
        }
        ffb6d::jacobi_svd3(G, V);
        double s2[3];
        for (int c = 0; c < 3; ++c) s2[c] = G[0][c] * G[0][c] + G[1][c] * G[1][c] + G[2][c] * G[2][c];
        int lo = 0;                                             // the smallest singular value (the first of equals)
        for (int c = 1; c < 3; ++c)
            if (s2[c] < s2[lo]) lo = c;
        double second = -1.0;                                   // the smaller of the other two
        for (int c = 0; c < 3; ++c)
            if (c != lo && (second < 0 || s2[c] < second)) second = s2[c];
        if (second > 0) {
            double v[3] = {V[0][lo], V[1][lo], V[2][lo]};
            if (ffb6d::normalize3(v) > 0) {
                int big = 0;
                for (int a = 1; a < 3; ++a)
                    if (fabs(v[a]) > fabs(v[big])) big = a;
                const double sg = v[big] < 0 ? -1.0 : 1.0;
                for (int a = 0; a < 3; ++a) nv[a] = sg * v[a];
            }
        }
    }
    normals[j] = make_float4(static_cast<float>(nv[0]), static_cast<float>(nv[1]), static_cast<float>(nv[2]), 0.f);
}

// given normals: each normalised once in double; a non-finite component or zero length gives the zero vector
__global__ __launch_bounds__(kBlock) void icp_set_normals_kernel(const float* __restrict__ in, int64_t total, float4* __restrict__ normals) {
    const int64_t j = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (j >= total) return;
    const double v[3] = {in[3 * j], in[3 * j + 1], in[3 * j + 2]};
    const double len = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (len > 0 && len <= 1.7976931348623157e308) o = make_float4(static_cast<float>(v[0] / len), static_cast<float>(v[1] / len), static_cast<float>(v[2] / len), 0.f);
    normals[j] = o;
}

// ---- host ------------------------------------------------------------------------------------------------------------
struct Workspace {
    float4* sets;
    int* counts;
    double* partials;
    double* T;
    int *done, *iters, *n_pairs;
    float* rms;
    float* rms_plane;                         // the plane metric only
    int tiles;
    size_t state_off, state_bytes, bytes;
};

// (the offsets are added as integers: the layouts are also made on a null base, for the sizes alone)
char* at_offset(void* base, size_t off) { return reinterpret_cast<char*>(reinterpret_cast<uintptr_t>(base) + off); }

// metric kPoint: the layout as it has always been; kPlane: 30 doubles per block and one more state row (rms_plane)
Workspace workspace_layout(void* base, int P, int64_t set_stride, int metric = kPoint) {
    Workspace w;
    w.tiles = static_cast<int>(ceil_div(set_stride, kTilePts));
    size_t off = 0;
    w.sets = reinterpret_cast<float4*>(at_offset(base, off));
    off += align256(sizeof(float4) * static_cast<size_t>(P) * set_stride);
    w.counts = reinterpret_cast<int*>(at_offset(base, off));
    off += align256(sizeof(int) * P);
    w.partials = reinterpret_cast<double*>(at_offset(base, off));
    off += align256(sizeof(double) * (metric == kPlane ? kPlaneSums : kSums) * static_cast<size_t>(P) * w.tiles);
    w.T = reinterpret_cast<double*>(at_offset(base, off));
    off += align256(sizeof(double) * 12 * P);
    w.state_off = off;
    w.done = reinterpret_cast<int*>(at_offset(base, off));
    w.iters = w.done + P;
    w.n_pairs = w.iters + P;
    w.rms = reinterpret_cast<float*>(w.n_pairs + P);
    w.rms_plane = metric == kPlane ? w.rms + P : nullptr;
    w.state_bytes = (metric == kPlane ? 5 : 4) * sizeof(int) * P;
    off += align256(w.state_bytes);
    w.bytes = off;
    return w;
}

int g_form = 0;                               // scan until the pruned form is measured faster at both model sizes
unsigned long long* g_pairs = nullptr;

unsigned morton10(unsigned x, unsigned y, unsigned z) {
    auto spread = [](unsigned v) {
        v &= 0x3ffu;
        v = (v | (v << 16)) & 0x030000ffu;
        v = (v | (v << 8)) & 0x0300f00fu;
        v = (v | (v << 4)) & 0x030c30c3u;
        v = (v | (v << 2)) & 0x09249249u;
        return v;
    };
    return spread(x) | (spread(y) << 1) | (spread(z) << 2);
}

int check_scene_args(const char* who, const void* prepared, int n_cls, int64_t total, const void* pcld, const void* mask, int mask_bits,
                     const int* frame_of, const int* class_of, const double* T, int P, int B, int N, int64_t set_stride, float max_dist,
                     void* workspace, size_t workspace_bytes, size_t need) {
    FFB6D_REQUIRE(P >= 0 && P <= 65535 && B > 0 && N > 0 && n_cls > 0 && total >= 0, "%s: bad sizes P=%d B=%d N=%d n_cls=%d total=%lld", who, P, B, N, n_cls,
                  (long long)total);
    FFB6D_REQUIRE(mask_bits == 32 || mask_bits == 64, "%s: mask_bits must be 32 or 64, got %d", who, mask_bits);
    FFB6D_REQUIRE(set_stride >= N, "%s: set_stride %lld < N %d", who, (long long)set_stride, N);
    FFB6D_REQUIRE(max_dist > 0.f, "%s: max_dist must be positive (inf allowed), got %g", who, (double)max_dist);
    if (P == 0) return 0;
    FFB6D_REQUIRE(prepared && pcld && mask && frame_of && class_of && T, "%s: null pointer", who);
    if (!workspace || workspace_bytes < need)
        return ffb6d::set_error(FFB6D_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", who, workspace_bytes, need);
    return 0;
}

// inst / inst_of != NULL: the map form (mask == class && inst == inst_of[p])
int launch_select(const float* pcld, const void* mask, int mask_bits, const unsigned char* keep, const unsigned char* inst, const int* frame_of,
                  const int* class_of, const int* inst_of, int P, int B, int N, int64_t set_stride, const Workspace& w, hipStream_t st) {
    const unsigned grid = static_cast<unsigned>(P);
    if (mask_bits == 64 && inst)
        icp_select_kernel<int64_t, true><<<grid, kBlock, 0, st>>>(pcld, static_cast<const int64_t*>(mask), keep, inst, frame_of, class_of, inst_of,
                                                                   B, N, set_stride, w.sets, w.counts);
    else if (mask_bits == 64)
        icp_select_kernel<int64_t, false><<<grid, kBlock, 0, st>>>(pcld, static_cast<const int64_t*>(mask), keep, inst, frame_of, class_of, inst_of,
                                                                    B, N, set_stride, w.sets, w.counts);
    else if (inst)
        icp_select_kernel<int32_t, true><<<grid, kBlock, 0, st>>>(pcld, static_cast<const int32_t*>(mask), keep, inst, frame_of, class_of, inst_of,
                                                                   B, N, set_stride, w.sets, w.counts);
    else
        icp_select_kernel<int32_t, false><<<grid, kBlock, 0, st>>>(pcld, static_cast<const int32_t*>(mask), keep, inst, frame_of, class_of, inst_of,
                                                                    B, N, set_stride, w.sets, w.counts);
    FFB6D_LAUNCH_CHECK();
    return 0;
}

// the instance calls: the workspace of the class calls, then the rows the owners are decided on and every problem's group
struct InstWorkspace {
    Workspace w;
    int* idx_rows;                            // [P, set_stride]
    float* d2_rows;                           // [P, set_stride]
    int2* groups;                             // [P]
    size_t bytes;
};

InstWorkspace inst_workspace_layout(void* base, int P, int64_t set_stride, int metric = kPoint) {
    InstWorkspace iw;
    iw.w = workspace_layout(base, P, set_stride, metric);
    size_t off = iw.w.bytes;
    iw.idx_rows = reinterpret_cast<int*>(at_offset(base, off));
    off += align256(sizeof(int) * static_cast<size_t>(P) * set_stride);
    iw.d2_rows = reinterpret_cast<float*>(at_offset(base, off));
    off += align256(sizeof(float) * static_cast<size_t>(P) * set_stride);
    iw.groups = reinterpret_cast<int2*>(at_offset(base, off));
    off += align256(sizeof(int2) * P);
    iw.bytes = off;
    return iw;
}

// what the instance calls check before the checks they share with the class calls; each refusal has its own message
int check_inst_args(const char* who, int P, int mode, const unsigned char* inst, const int* inst_of) {
    FFB6D_REQUIRE(mode == 0 || mode == 1, "%s: mode must be 0 (map) or 1 (nearest), got %d", who, mode);
    FFB6D_REQUIRE(P <= 65535, "%s: %d problems, at most 65535 to a call", who, P);
    FFB6D_REQUIRE(mode == 1 || inst || P <= 0, "%s: the map mode needs the instance map (inst is NULL)", who);
    FFB6D_REQUIRE(inst_of || P <= 0, "%s: null pointer (inst_of)", who);
    return 0;
}

// what differs between the calls: the poses they measure under (T, done) and where the results go (rows, partial sums)
CorrArgs make_corr_args(const Workspace& w, int64_t set_stride, const int* class_of, const double* T, const int* done, const void* prepared,
                        int64_t total, int n_cls, float max_dist, int* idx_out, float* d2_out, double* partials) {
    CorrArgs a;
    a.sets = w.sets; a.counts = w.counts; a.stride = set_stride; a.class_of = class_of; a.T = T; a.done = done;
    a.m = prepared_view(prepared, prepared_layout(total, n_cls), n_cls);
    a.n_cls = n_cls; a.max_d2 = max_dist * max_dist; a.form = g_form; a.idx_out = idx_out; a.d2_out = d2_out; a.partials = partials;
    a.tiles = w.tiles; a.pairs = g_pairs; a.normals = nullptr;
    return a;
}

SolveArgs make_solve_args(const Workspace& w, const int* class_of, const Prepared& m, int n_cls, int min_pairs, double tol) {
    SolveArgs s;
    s.counts = w.counts; s.class_of = class_of; s.m = m; s.n_cls = n_cls; s.partials = w.partials; s.tiles = w.tiles; s.T = w.T;
    s.done = w.done; s.iters = w.iters; s.n_pairs = w.n_pairs; s.rms = w.rms; s.min_pairs = min_pairs; s.tol = tol;
    s.rms_plane = w.rms_plane; s.min_eig = 0.0;
    return s;
}

int copy_results(const Workspace& w, int P, double* T, int* n_pairs, float* rms, int* iters, hipStream_t st) {
    if (T) FFB6D_HIP_TRY(hipMemcpyAsync(T, w.T, sizeof(double) * 12 * P, hipMemcpyDeviceToDevice, st));
    if (n_pairs) FFB6D_HIP_TRY(hipMemcpyAsync(n_pairs, w.n_pairs, sizeof(int) * P, hipMemcpyDeviceToDevice, st));
    if (rms) FFB6D_HIP_TRY(hipMemcpyAsync(rms, w.rms, sizeof(float) * P, hipMemcpyDeviceToDevice, st));
    if (iters) FFB6D_HIP_TRY(hipMemcpyAsync(iters, w.iters, sizeof(int) * P, hipMemcpyDeviceToDevice, st));
    return 0;
}

// What the plane calls add to the point calls: the metric's name for the messages, the normals, min_eig and one more output.
// The point calls pass kPoint and nulls, and run exactly what they ran before the plane metric existed.
struct Metric {
    int id;
    const char* who;
    const void* normals;
    double min_eig;
    float* rms_plane;
};

int check_metric_args(const Metric& mt, int P) {
    if (mt.id != kPlane) return 0;
    FFB6D_REQUIRE(mt.min_eig >= 0.0 && mt.min_eig < 1.0, "%s: min_eig must be in [0, 1), got %g", mt.who, mt.min_eig);
    FFB6D_REQUIRE(mt.normals || P <= 0, "%s: the plane metric needs the model normals (normals is NULL)", mt.who);
    return 0;
}

int refine_class(const Metric& mt, const void* prepared, int n_cls, int64_t total, const float* pcld, const void* mask, int mask_bits,
                 const unsigned char* keep, const int* frame_of, const int* class_of, const double* T0, int P, int B, int N, int64_t set_stride,
                 float max_dist, int max_iter, double tol, int min_pairs, double* T, int* n_pairs, float* rms, int* iters, void* workspace,
                 size_t workspace_bytes, ffb6d_stream_t stream) {
    FFB6D_REQUIRE(max_iter >= 0 && tol >= 0.0 && min_pairs >= 1, "%s: bad max_iter=%d / tol=%g / min_pairs=%d", mt.who, max_iter, tol, min_pairs);
    int rc = check_metric_args(mt, P);
    if (rc != 0) return rc;
    const size_t need = P <= 0 || set_stride <= 0 ? 0 : workspace_layout(nullptr, P, set_stride, mt.id).bytes;
    rc = check_scene_args(mt.who, prepared, n_cls, total, pcld, mask, mask_bits, frame_of, class_of, T0, P, B, N, set_stride, max_dist, workspace,
                          workspace_bytes, need);
    if (rc != 0 || P == 0) return rc;
    hipStream_t st = ffb6d::as_stream(stream);
    const Workspace w = workspace_layout(workspace, P, set_stride, mt.id);
    FFB6D_HIP_TRY(hipMemsetAsync(static_cast<char*>(workspace) + w.state_off, 0, w.state_bytes, st));
    FFB6D_HIP_TRY(hipMemcpyAsync(w.T, T0, sizeof(double) * 12 * P, hipMemcpyDeviceToDevice, st));
    if (max_iter > 0) {
        const int rs = launch_select(pcld, mask, mask_bits, keep, nullptr, frame_of, class_of, nullptr, P, B, N, set_stride, w, st);
        if (rs != 0) return rs;
    }
    CorrArgs a = make_corr_args(w, set_stride, class_of, w.T, w.done, prepared, total, n_cls, max_dist, nullptr, nullptr, w.partials);
    a.normals = static_cast<const float4*>(mt.normals);
    SolveArgs s = make_solve_args(w, class_of, a.m, n_cls, min_pairs, tol);
    s.min_eig = mt.min_eig;
    const dim3 grid(static_cast<unsigned>(w.tiles), static_cast<unsigned>(P));
    for (int it = 0; it < max_iter; ++it) {
        if (mt.id == kPlane) {
            icp_correspond_kernel<kPlane><<<grid, kBlock, 0, st>>>(a);
            FFB6D_LAUNCH_CHECK();
            icp_solve_plane_kernel<<<static_cast<unsigned>(P), 64, 0, st>>>(s);
        } else {
            icp_correspond_kernel<kPoint><<<grid, kBlock, 0, st>>>(a);
            FFB6D_LAUNCH_CHECK();
            icp_solve_kernel<<<static_cast<unsigned>(P), 64, 0, st>>>(s);
        }
        FFB6D_LAUNCH_CHECK();
    }
    if (mt.rms_plane) FFB6D_HIP_TRY(hipMemcpyAsync(mt.rms_plane, w.rms_plane, sizeof(float) * P, hipMemcpyDeviceToDevice, st));
    return copy_results(w, P, T, n_pairs, rms, iters, st);
}

int refine_inst(const Metric& mt, const void* prepared, int n_cls, int64_t total, const float* pcld, const void* mask, int mask_bits,
                const unsigned char* keep, const unsigned char* inst, const int* frame_of, const int* class_of, const int* inst_of,
                const double* T0, int P, int B, int N, int64_t set_stride, float max_dist, int max_iter, double tol, int min_pairs, int mode,
                double* T, int* n_pairs, float* rms, int* iters, unsigned char* inst_out, void* workspace, size_t workspace_bytes,
                ffb6d_stream_t stream) {
    FFB6D_REQUIRE(max_iter >= 0 && tol >= 0.0 && min_pairs >= 1, "%s: bad max_iter=%d / tol=%g / min_pairs=%d", mt.who, max_iter, tol, min_pairs);
    int rc = check_inst_args(mt.who, P, mode, inst, inst_of);
    if (rc != 0) return rc;
    rc = check_metric_args(mt, P);
    if (rc != 0) return rc;
    const size_t need = P <= 0 || set_stride <= 0 ? 0 : inst_workspace_layout(nullptr, P, set_stride, mt.id).bytes;
    rc = check_scene_args(mt.who, prepared, n_cls, total, pcld, mask, mask_bits, frame_of, class_of, T0, P, B, N, set_stride, max_dist, workspace,
                          workspace_bytes, need);
    if (rc != 0) return rc;
    hipStream_t st = ffb6d::as_stream(stream);
    if (inst_out) FFB6D_HIP_TRY(hipMemsetAsync(inst_out, 0, static_cast<size_t>(B) * N, st));
    if (P == 0) return 0;
    const InstWorkspace iw = inst_workspace_layout(workspace, P, set_stride, mt.id);
    const Workspace& w = iw.w;
    FFB6D_HIP_TRY(hipMemsetAsync(static_cast<char*>(workspace) + w.state_off, 0, w.state_bytes, st));
    FFB6D_HIP_TRY(hipMemcpyAsync(w.T, T0, sizeof(double) * 12 * P, hipMemcpyDeviceToDevice, st));
    if (max_iter > 0) {
        rc = launch_select(pcld, mask, mask_bits, keep, mode == 0 ? inst : nullptr, frame_of, class_of, mode == 0 ? inst_of : nullptr, P, B, N,
                           set_stride, w, st);
        if (rc != 0) return rc;
        icp_groups_kernel<<<static_cast<unsigned>(ceil_div(P, kBlock)), kBlock, 0, st>>>(frame_of, class_of, P, mode, iw.groups);
        FFB6D_LAUNCH_CHECK();
    }
    // map: the loop of the class call on the instances' sets (the kept pairs go to the idx rows only when inst_out asks for them);
    // nearest: every problem measures its distances in every iteration, stopped or not (it goes on competing under its pose), the
    // claim kernel decides the owners and makes the sums, and the update is the class call's
    const bool nearest = mode == 1;
    CorrArgs a = make_corr_args(w, set_stride, class_of, w.T, nearest ? nullptr : w.done, prepared, total, n_cls, max_dist,
                                (nearest || inst_out) ? iw.idx_rows : nullptr, nearest ? iw.d2_rows : nullptr, nearest ? nullptr : w.partials);
    a.normals = static_cast<const float4*>(mt.normals);
    ClaimArgs c;
    c.sets = w.sets; c.counts = w.counts; c.stride = set_stride; c.class_of = class_of; c.groups = iw.groups; c.m = a.m; c.n_cls = n_cls;
    c.d2_rows = iw.d2_rows; c.idx_rows = iw.idx_rows; c.idx_out = iw.idx_rows; c.d2_out = nullptr; c.owner_out = nullptr;
    c.partials = w.partials; c.tiles = w.tiles; c.normals = a.normals; c.T = w.T;
    SolveArgs s = make_solve_args(w, class_of, a.m, n_cls, min_pairs, tol);
    s.min_eig = mt.min_eig;
    const dim3 grid(static_cast<unsigned>(w.tiles), static_cast<unsigned>(P));
    for (int it = 0; it < max_iter; ++it) {
        if (mt.id == kPlane) {
            icp_correspond_kernel<kPlane><<<grid, kBlock, 0, st>>>(a);
            FFB6D_LAUNCH_CHECK();
            if (nearest) {
                icp_claim_kernel<kPlane><<<grid, 64, 0, st>>>(c);
                FFB6D_LAUNCH_CHECK();
            }
            icp_solve_plane_kernel<<<static_cast<unsigned>(P), 64, 0, st>>>(s);
        } else {
            icp_correspond_kernel<kPoint><<<grid, kBlock, 0, st>>>(a);
            FFB6D_LAUNCH_CHECK();
            if (nearest) {
                icp_claim_kernel<kPoint><<<grid, 64, 0, st>>>(c);
                FFB6D_LAUNCH_CHECK();
            }
            icp_solve_kernel<<<static_cast<unsigned>(P), 64, 0, st>>>(s);
        }
        FFB6D_LAUNCH_CHECK();
    }
    if (inst_out && max_iter > 0) {
        icp_inst_out_kernel<<<dim3(static_cast<unsigned>(ceil_div(set_stride, kBlock)), static_cast<unsigned>(P)), kBlock, 0, st>>>(
            w.sets, w.counts, set_stride, iw.idx_rows, frame_of, inst_of, N, inst_out);
        FFB6D_LAUNCH_CHECK();
    }
    if (mt.rms_plane) FFB6D_HIP_TRY(hipMemcpyAsync(mt.rms_plane, w.rms_plane, sizeof(float) * P, hipMemcpyDeviceToDevice, st));
    return copy_results(w, P, T, n_pairs, rms, iters, st);
}

}  // namespace

extern "C" {

void ffb6d_icp_set_form(int form) { g_form = form < 0 ? -1 : (form ? 1 : 0); }

int ffb6d_icp_set_pair_counter(unsigned long long* device_counter) {
    g_pairs = device_counter;
    return 0;
}

size_t ffb6d_icp_prepared_bytes(int64_t total, int n_cls) {
    if (total < 0 || n_cls <= 0) return 0;
    return prepared_layout(total, n_cls).bytes;
}

int ffb6d_icp_prepare(const float* model_pts, const int64_t* model_begin, int n_cls, int64_t total, void* prepared, size_t prepared_bytes,
                      ffb6d_stream_t stream) {
    FFB6D_REQUIRE(n_cls > 0 && total >= 0 && total < (int64_t(1) << 31), "icp_prepare: bad sizes n_cls=%d total=%lld", n_cls, (long long)total);
    FFB6D_REQUIRE(model_begin && prepared && (total == 0 || model_pts), "icp_prepare: null pointer");
    const Layout l = prepared_layout(total, n_cls);
    if (prepared_bytes < l.bytes) return ffb6d::set_error(FFB6D_ERR_WORKSPACE, "icp_prepare: buffer %zu < %zu bytes", prepared_bytes, l.bytes);
    hipStream_t st = ffb6d::as_stream(stream);
    std::vector<int64_t> begin(static_cast<size_t>(n_cls) + 1);
    std::vector<float> pts(static_cast<size_t>(total) * 3);
    FFB6D_HIP_TRY(hipMemcpyAsync(begin.data(), model_begin, sizeof(int64_t) * begin.size(), hipMemcpyDeviceToHost, st));
    if (total > 0) FFB6D_HIP_TRY(hipMemcpyAsync(pts.data(), model_pts, sizeof(float) * pts.size(), hipMemcpyDeviceToHost, st));
    FFB6D_HIP_TRY(hipStreamSynchronize(st));
    bool ok = begin[0] == 0 && begin[n_cls] == total;
    for (int c = 0; c < n_cls && ok; ++c) ok = begin[c + 1] >= begin[c];
    FFB6D_REQUIRE(ok, "icp_prepare: model_begin is not a rising table from 0 to total=%lld", (long long)total);

    std::vector<unsigned char> blob(l.bytes, 0);
    ClassInfo* cls = reinterpret_cast<ClassInfo*>(blob.data() + l.cls);
    float4* cls_lo = reinterpret_cast<float4*>(blob.data() + l.cls_box);
    float4* cls_hi = cls_lo + n_cls;
    float4* orig = reinterpret_cast<float4*>(blob.data() + l.orig);
    float4* sorted = reinterpret_cast<float4*>(blob.data() + l.sorted);
    float4* tile_lo = reinterpret_cast<float4*>(blob.data() + l.tile_box);
    float4* tile_hi = tile_lo + l.max_tiles;
    const float inf = std::numeric_limits<float>::infinity(), qnan = std::numeric_limits<float>::quiet_NaN();
    float no_index;
    const int no_index_bits = kNoIndex;
    std::memcpy(&no_index, &no_index_bits, sizeof(float));
    for (int64_t i = 0; i < total; ++i) orig[i] = make_float4(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], 0.f);
    int tile_begin = 0;
    std::vector<unsigned long long> order;
    for (int c = 0; c < n_cls; ++c) {
        const int64_t b0 = begin[c];
        const int n = static_cast<int>(begin[c + 1] - b0);
        const int nt = (n + kTilePts - 1) / kTilePts;
        cls[c] = ClassInfo{static_cast<int>(b0), n, tile_begin, nt};
        float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
        for (int i = 0; i < n; ++i)
            for (int k = 0; k < 3; ++k) {
                const float v = pts[3 * (b0 + i) + k];
                if (v < lo[k]) lo[k] = v;
                if (v > hi[k]) hi[k] = v;
            }
        for (int k = 0; k < 3; ++k)
            if (!(lo[k] <= hi[k])) lo[k] = hi[k] = 0.f;
        cls_lo[c] = make_float4(lo[0], lo[1], lo[2], 0.f);
        cls_hi[c] = make_float4(hi[0], hi[1], hi[2], 0.f);
        order.resize(static_cast<size_t>(n));
        for (int i = 0; i < n; ++i) {
            unsigned q[3];
            for (int k = 0; k < 3; ++k) {
                const float ext = hi[k] - lo[k];
                const float v = ext > 0.f ? (pts[3 * (b0 + i) + k] - lo[k]) / ext * 1023.f : 0.f;
                q[k] = v >= 0.f ? (v < 1023.f ? static_cast<unsigned>(v) : 1023u) : 0u;      // (NaN: 0)
            }
            order[i] = (static_cast<unsigned long long>(morton10(q[0], q[1], q[2])) << 32) | static_cast<unsigned>(i);
        }
        std::sort(order.begin(), order.end());
        for (int t = 0; t < nt; ++t) {
            float tl[3] = {inf, inf, inf}, th[3] = {-inf, -inf, -inf};
            for (int k = 0; k < kTilePts; ++k) {
                const int j = t * kTilePts + k;
                float4& dst = sorted[static_cast<int64_t>(tile_begin + t) * kTilePts + k];
                if (j >= n) {
                    dst = make_float4(qnan, qnan, qnan, no_index);
                    continue;
                }
                const int i = static_cast<int>(order[j] & 0xffffffffull);
                float idx_bits;
                std::memcpy(&idx_bits, &i, sizeof(float));
                const float* pt = &pts[3 * (b0 + i)];
                dst = make_float4(pt[0], pt[1], pt[2], idx_bits);
                for (int d = 0; d < 3; ++d) {
                    if (pt[d] < tl[d]) tl[d] = pt[d];
                    if (pt[d] > th[d]) th[d] = pt[d];
                }
            }
            for (int d = 0; d < 3; ++d)
                if (!(tl[d] <= th[d])) tl[d] = th[d] = 0.f;
            tile_lo[tile_begin + t] = make_float4(tl[0], tl[1], tl[2], 0.f);
            tile_hi[tile_begin + t] = make_float4(th[0], th[1], th[2], 0.f);
        }
        tile_begin += nt;
    }
    FFB6D_HIP_TRY(hipMemcpyAsync(prepared, blob.data(), l.bytes, hipMemcpyHostToDevice, st));
    FFB6D_HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

size_t ffb6d_icp_workspace_bytes(int P, int64_t set_stride) {
    if (P <= 0 || set_stride <= 0) return 0;
    return workspace_layout(nullptr, P, set_stride).bytes;
}

int ffb6d_icp_correspond_f32(const void* prepared, int n_cls, int64_t total, const float* pcld, const void* mask, int mask_bits,
                             const unsigned char* keep, const int* frame_of, const int* class_of, const double* T, int P, int B, int N,
                             int64_t set_stride, float max_dist, int* idx, float* d2, int* counts, void* workspace, size_t workspace_bytes,
                             ffb6d_stream_t stream) {
    const int rc = check_scene_args("icp_correspond", prepared, n_cls, total, pcld, mask, mask_bits, frame_of, class_of, T, P, B, N, set_stride,
                                    max_dist, workspace, workspace_bytes, ffb6d_icp_workspace_bytes(P, set_stride));
    if (rc != 0 || P == 0) return rc;
    hipStream_t st = ffb6d::as_stream(stream);
    const Workspace w = workspace_layout(workspace, P, set_stride);
    const int rs = launch_select(pcld, mask, mask_bits, keep, nullptr, frame_of, class_of, nullptr, P, B, N, set_stride, w, st);
    if (rs != 0) return rs;
    if (idx || d2) {
        const int64_t n = static_cast<int64_t>(P) * set_stride;
        icp_fill_kernel<<<static_cast<unsigned>(ceil_div(n, kBlock)), kBlock, 0, st>>>(idx, d2, n);
        FFB6D_LAUNCH_CHECK();
        const CorrArgs a = make_corr_args(w, set_stride, class_of, T, nullptr, prepared, total, n_cls, max_dist, idx, d2, nullptr);
        icp_correspond_kernel<kPoint><<<dim3(static_cast<unsigned>(w.tiles), static_cast<unsigned>(P)), kBlock, 0, st>>>(a);
        FFB6D_LAUNCH_CHECK();
    }
    if (counts) FFB6D_HIP_TRY(hipMemcpyAsync(counts, w.counts, sizeof(int) * P, hipMemcpyDeviceToDevice, st));
    return 0;
}

int ffb6d_icp_refine_f32(const void* prepared, int n_cls, int64_t total, const float* pcld, const void* mask, int mask_bits,
                         const unsigned char* keep, const int* frame_of, const int* class_of, const double* T0, int P, int B, int N,
                         int64_t set_stride, float max_dist, int max_iter, double tol, int min_pairs, double* T, int* n_pairs, float* rms,
                         int* iters, void* workspace, size_t workspace_bytes, ffb6d_stream_t stream) {
    const Metric mt = {kPoint, "icp_refine", nullptr, 0.0, nullptr};
    return refine_class(mt, prepared, n_cls, total, pcld, mask, mask_bits, keep, frame_of, class_of, T0, P, B, N, set_stride, max_dist, max_iter,
                        tol, min_pairs, T, n_pairs, rms, iters, workspace, workspace_bytes, stream);
}

size_t ffb6d_icp_inst_workspace_bytes(int P, int64_t set_stride, int mode) {
    if (P <= 0 || set_stride <= 0 || (mode != 0 && mode != 1)) return 0;
    return inst_workspace_layout(nullptr, P, set_stride).bytes;
}

int ffb6d_icp_correspond_inst_f32(const void* prepared, int n_cls, int64_t total, const float* pcld, const void* mask, int mask_bits,
                                  const unsigned char* keep, const unsigned char* inst, const int* frame_of, const int* class_of,
                                  const int* inst_of, const double* T, int P, int B, int N, int64_t set_stride, float max_dist, int mode,
                                  int* idx, float* d2, int* counts, int* owner, void* workspace, size_t workspace_bytes,
                                  ffb6d_stream_t stream) {
    int rc = check_inst_args("icp_correspond_inst", P, mode, inst, inst_of);
    if (rc != 0) return rc;
    rc = check_scene_args("icp_correspond_inst", prepared, n_cls, total, pcld, mask, mask_bits, frame_of, class_of, T, P, B, N, set_stride,
                          max_dist, workspace, workspace_bytes, ffb6d_icp_inst_workspace_bytes(P, set_stride, mode));
    if (rc != 0 || P == 0) return rc;
    hipStream_t st = ffb6d::as_stream(stream);
    const InstWorkspace iw = inst_workspace_layout(workspace, P, set_stride);
    const Workspace& w = iw.w;
    rc = launch_select(pcld, mask, mask_bits, keep, mode == 0 ? inst : nullptr, frame_of, class_of, mode == 0 ? inst_of : nullptr, P, B, N,
                       set_stride, w, st);
    if (rc != 0) return rc;
    if (idx || d2 || owner) {
        const int64_t n = static_cast<int64_t>(P) * set_stride;
        const unsigned fill_grid = static_cast<unsigned>(ceil_div(n, kBlock));
        if (idx || d2) {
            icp_fill_kernel<<<fill_grid, kBlock, 0, st>>>(idx, d2, n);
            FFB6D_LAUNCH_CHECK();
        }
        if (owner) {
            icp_fill_kernel<<<fill_grid, kBlock, 0, st>>>(owner, nullptr, n);
            FFB6D_LAUNCH_CHECK();
        }
        icp_groups_kernel<<<static_cast<unsigned>(ceil_div(P, kBlock)), kBlock, 0, st>>>(frame_of, class_of, P, mode, iw.groups);
        FFB6D_LAUNCH_CHECK();
        const CorrArgs a = make_corr_args(w, set_stride, class_of, T, nullptr, prepared, total, n_cls, max_dist, iw.idx_rows, iw.d2_rows, nullptr);
        const dim3 grid(static_cast<unsigned>(w.tiles), static_cast<unsigned>(P));
        icp_correspond_kernel<kPoint><<<grid, kBlock, 0, st>>>(a);
        FFB6D_LAUNCH_CHECK();
        ClaimArgs c;
        c.sets = w.sets; c.counts = w.counts; c.stride = set_stride; c.class_of = class_of; c.groups = iw.groups; c.m = a.m; c.n_cls = n_cls;
        c.d2_rows = iw.d2_rows; c.idx_rows = iw.idx_rows; c.idx_out = idx; c.d2_out = d2; c.owner_out = owner; c.partials = nullptr;
        c.tiles = w.tiles; c.normals = nullptr; c.T = T;
        icp_claim_kernel<kPoint><<<grid, 64, 0, st>>>(c);
        FFB6D_LAUNCH_CHECK();
    }
    if (counts) FFB6D_HIP_TRY(hipMemcpyAsync(counts, w.counts, sizeof(int) * P, hipMemcpyDeviceToDevice, st));
    return 0;
}

int ffb6d_icp_refine_inst_f32(const void* prepared, int n_cls, int64_t total, const float* pcld, const void* mask, int mask_bits,
                              const unsigned char* keep, const unsigned char* inst, const int* frame_of, const int* class_of,
                              const int* inst_of, const double* T0, int P, int B, int N, int64_t set_stride, float max_dist, int max_iter,
                              double tol, int min_pairs, int mode, double* T, int* n_pairs, float* rms, int* iters,
                              unsigned char* inst_out, void* workspace, size_t workspace_bytes, ffb6d_stream_t stream) {
    const Metric mt = {kPoint, "icp_refine_inst", nullptr, 0.0, nullptr};
    return refine_inst(mt, prepared, n_cls, total, pcld, mask, mask_bits, keep, inst, frame_of, class_of, inst_of, T0, P, B, N, set_stride,
                       max_dist, max_iter, tol, min_pairs, mode, T, n_pairs, rms, iters, inst_out, workspace, workspace_bytes, stream);
}

// ---- the plane metric ----------------------------------------------------------------------------------------------------
size_t ffb6d_icp_normals_bytes(int64_t total) {
    if (total < 0) return 0;
    return align256(sizeof(float4) * static_cast<size_t>(total > 0 ? total : 1));
}

int ffb6d_icp_set_normals(const float* normals_in, int64_t total, void* normals, size_t normals_bytes, ffb6d_stream_t stream) {
    FFB6D_REQUIRE(total >= 0 && total < (int64_t(1) << 31), "icp_set_normals: bad total=%lld", (long long)total);
    FFB6D_REQUIRE(normals && (total == 0 || normals_in), "icp_set_normals: null pointer");
    if (normals_bytes < ffb6d_icp_normals_bytes(total))
        return ffb6d::set_error(FFB6D_ERR_WORKSPACE, "icp_set_normals: buffer %zu < %zu bytes", normals_bytes, ffb6d_icp_normals_bytes(total));
    if (total == 0) return 0;
    icp_set_normals_kernel<<<static_cast<unsigned>(ceil_div(total, kBlock)), kBlock, 0, ffb6d::as_stream(stream)>>>(
        normals_in, total, static_cast<float4*>(normals));
    FFB6D_LAUNCH_CHECK();
    return 0;
}

int ffb6d_icp_estimate_normals_f32(const float* model_pts, const int64_t* model_begin, int n_cls, int64_t total, void* normals,
                                   size_t normals_bytes, ffb6d_stream_t stream) {
    FFB6D_REQUIRE(n_cls > 0 && total >= 0 && total < (int64_t(1) << 31), "icp_estimate_normals: bad sizes n_cls=%d total=%lld", n_cls,
                  (long long)total);
    FFB6D_REQUIRE(model_begin && normals && (total == 0 || model_pts), "icp_estimate_normals: null pointer");
    if (normals_bytes < ffb6d_icp_normals_bytes(total))
        return ffb6d::set_error(FFB6D_ERR_WORKSPACE, "icp_estimate_normals: buffer %zu < %zu bytes", normals_bytes,
                                ffb6d_icp_normals_bytes(total));
    hipStream_t st = ffb6d::as_stream(stream);
    std::vector<int64_t> begin(static_cast<size_t>(n_cls) + 1);
    FFB6D_HIP_TRY(hipMemcpyAsync(begin.data(), model_begin, sizeof(int64_t) * begin.size(), hipMemcpyDeviceToHost, st));
    FFB6D_HIP_TRY(hipStreamSynchronize(st));
    bool ok = begin[0] == 0 && begin[n_cls] == total;
    for (int c = 0; c < n_cls && ok; ++c) ok = begin[c + 1] >= begin[c];
    FFB6D_REQUIRE(ok, "icp_estimate_normals: model_begin is not a rising table from 0 to total=%lld", (long long)total);
    // scratch for the largest class: its neighbour rows and what the search asks for
    size_t idx_bytes = 0, knn_bytes = 0;
    for (int c = 0; c < n_cls; ++c) {
        const int64_t n = begin[c + 1] - begin[c];
        const int k = static_cast<int>(std::min<int64_t>(kNormalK, n));
        if (n < 3) continue;
        idx_bytes = std::max(idx_bytes, align256(sizeof(int) * static_cast<size_t>(n) * k));
        knn_bytes = std::max(knn_bytes, ffb6d_knn_workspace_bytes(1, n, n, k));
    }
    char* scratch = nullptr;
    if (idx_bytes + knn_bytes > 0) FFB6D_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&scratch), idx_bytes + knn_bytes));
    int rc = 0;
    for (int c = 0; c < n_cls && rc == 0; ++c) {
        const int64_t n = begin[c + 1] - begin[c];
        if (n == 0) continue;
        const int k = static_cast<int>(std::min<int64_t>(kNormalK, n));
        const float* pts = model_pts + 3 * begin[c];
        int* rows = reinterpret_cast<int*>(scratch);
        if (n >= 3)
            rc = ffb6d_knn_batch_device(pts, pts, 1, n, n, k, nullptr, rows, nullptr, knn_bytes ? scratch + idx_bytes : nullptr, knn_bytes, stream);
        if (rc != 0) break;
        icp_normals_kernel<<<static_cast<unsigned>(ceil_div(n, kBlock)), kBlock, 0, st>>>(pts, rows, static_cast<int>(n), k,
                                                                                          static_cast<float4*>(normals) + begin[c]);
        if (hipGetLastError() != hipSuccess) rc = ffb6d::set_error(FFB6D_ERR_HIP, "icp_estimate_normals: kernel launch failed");
    }
    const hipError_t es = hipStreamSynchronize(st);               // (once per model set, like ffb6d_icp_prepare: the scratch is freed below)
    if (scratch) (void)hipFree(scratch);
    if (rc == 0 && es != hipSuccess) rc = ffb6d::set_error(FFB6D_ERR_HIP, "icp_estimate_normals: %s", hipGetErrorString(es));
    return rc;
}

size_t ffb6d_icp_plane_workspace_bytes(int P, int64_t set_stride) {
    if (P <= 0 || set_stride <= 0) return 0;
    return workspace_layout(nullptr, P, set_stride, kPlane).bytes;
}

size_t ffb6d_icp_plane_inst_workspace_bytes(int P, int64_t set_stride, int mode) {
    if (P <= 0 || set_stride <= 0 || (mode != 0 && mode != 1)) return 0;
    return inst_workspace_layout(nullptr, P, set_stride, kPlane).bytes;
}

int ffb6d_icp_refine_plane_f32(const void* prepared, const void* normals, int n_cls, int64_t total, const float* pcld, const void* mask,
                               int mask_bits, const unsigned char* keep, const int* frame_of, const int* class_of, const double* T0, int P, int B,
                               int N, int64_t set_stride, float max_dist, int max_iter, double tol, int min_pairs, double min_eig, double* T,
                               int* n_pairs, float* rms, float* rms_plane, int* iters, void* workspace, size_t workspace_bytes,
                               ffb6d_stream_t stream) {
    const Metric mt = {kPlane, "icp_refine_plane", normals, min_eig, rms_plane};
    return refine_class(mt, prepared, n_cls, total, pcld, mask, mask_bits, keep, frame_of, class_of, T0, P, B, N, set_stride, max_dist, max_iter,
                        tol, min_pairs, T, n_pairs, rms, iters, workspace, workspace_bytes, stream);
}

int ffb6d_icp_refine_plane_inst_f32(const void* prepared, const void* normals, int n_cls, int64_t total, const float* pcld, const void* mask,
                                    int mask_bits, const unsigned char* keep, const unsigned char* inst, const int* frame_of,
                                    const int* class_of, const int* inst_of, const double* T0, int P, int B, int N, int64_t set_stride,
                                    float max_dist, int max_iter, double tol, int min_pairs, double min_eig, int mode, double* T, int* n_pairs,
                                    float* rms, float* rms_plane, int* iters, unsigned char* inst_out, void* workspace, size_t workspace_bytes,
                                    ffb6d_stream_t stream) {
    const Metric mt = {kPlane, "icp_refine_plane_inst", normals, min_eig, rms_plane};
    return refine_inst(mt, prepared, n_cls, total, pcld, mask, mask_bits, keep, inst, frame_of, class_of, inst_of, T0, P, B, N, set_stride,
                       max_dist, max_iter, tol, min_pairs, mode, T, n_pairs, rms, iters, inst_out, workspace, workspace_bytes, stream);
}

}  // extern "C"
