// ffb6d_amd/csrc/bop_eval.hip -- the BOP pose errors of a batch of (estimated, ground-truth) poses: MSSD / MSPD and VSD
// (include/ffb6d_bop.h states every formula; tests/bop_ref.py restates them in numpy).
//
// MSSD / MSPD are (points x symmetries) pair evaluations per row in double, a max over the points inside a min over the symmetries.
//   sym_max_kernel: one workgroup = (row, block of kSymBlock symmetries, chunk of kChunk points).  The first 12 kSymBlock threads
//     compose gt_T with the block's symmetries into LDS; then the points go across the lanes: a thread transforms and projects its
//     point under the estimate once, keeps it in registers and walks the block's symmetries (the composed transforms are LDS
//     broadcasts) with both running maxima of every symmetry in registers -- both errors out of one pass over the points.  The
//     maxima are reduced over the wave with shuffles, over the workgroup through one LDS slot per wave, and written per
//     (row, symmetry, chunk) into the workspace.
//   sym_min_kernel: one wavefront per row: max over the chunks, min over the symmetries, NaN for the rows the header lists.
//   Squared distances are >= 0 or +inf (a NaN is turned into +inf where it arises), so max and min do not depend on their order and
//   partial maxima need neither atomics nor an initialised workspace.
// VSD is a streaming pass over three float images.
//   vsd_count_kernel: grid (runs of kRunPx pixels, rows); a lane takes 4 consecutive pixels of each image per step (one 16-byte access
//     where the rows keep that alignment, single floats otherwise and for the tail), keeps the 2 + 16 counters in registers, and the
//     workgroup writes ONE set of partial counts (wave shuffles, then LDS).  Partial counts, not atomics into a slot, as in
//     color_jitter.hip: integer sums are exact either way and the workspace may hold anything on entry.
//   vsd_finish_kernel: one wavefront per row adds the partial counts and writes counts and vsd.
// The library is built with -ffp-contract=off; float division and __fsqrt_rn are correctly rounded.
#include <cfloat>
#include <climits>

#include "bop_common.h"
#include "ffb6d_bop.h"

namespace {

using namespace ffb6d::bop;                         // the run of pixels, Camera, ray_dist, load_px, aligned: shared with bop_scene.hip

constexpr int kSymBlock = 8;                        // symmetries per workgroup: 16 running maxima per thread
constexpr int kPer = 4;                             // points per thread
constexpr int kChunk = kThreads * kPer;             // points per workgroup
constexpr int kCounters = 2 + FFB6D_BOP_MAX_TAUS;

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : v > hi ? hi : v; }
__device__ __forceinline__ bool finite64(double v) { return (v - v) == 0.0; }                 // false for NaN and the infinities
__device__ __forceinline__ double inf64() { return __builtin_huge_val(); }
__device__ __forceinline__ double max64(double a, double b) { return b > a ? b : a; }
__device__ __forceinline__ double min64(double a, double b) { return b < a ? b : a; }

__device__ __forceinline__ double shfl_xor64(double v, int mask)
{
    return __builtin_bit_cast(double, __shfl_xor(__builtin_bit_cast(unsigned long long, v), mask, 64));
}

struct Tables {
    const float* pts;
    const int64_t* begin;
    int n_cls;
    int64_t total, max_points;
    const double *sym_R, *sym_t;
    const int64_t* sym_begin;
    int64_t Stot, max_syms;
    const int *class_of, *frame_of;
    const double *est_T, *gt_T;
    const double* K;
    int B;
};

struct Row {
    bool ok;            // false: NaN in both outputs
    int b, n, ns;       // frame, points and symmetries scored (ns >= 1)
    int64_t p0, s0;     // first point / symmetry of the class
    bool identity;      // the class has no entries: the identity alone
};

// the one statement of what a row is; both kernels of a call use it.  Nothing is read through an id that is out of range.
__device__ __forceinline__ Row row_of(const Tables& t, int q)
{
    Row r;
    r.ok = false;
    r.b = t.frame_of[q];
    r.n = 0; r.ns = 1; r.p0 = 0; r.s0 = 0; r.identity = true;
    const int c = t.class_of[q];
    if (c < 0 || c >= t.n_cls || r.b < 0 || r.b >= t.B) return r;
    r.p0 = clamp64(t.begin[c], 0, t.total);
    const int64_t n = clamp64(t.begin[c + 1], r.p0, t.total) - r.p0;
    r.n = static_cast<int>(n < t.max_points ? n : t.max_points);
    if (r.n == 0) return r;
    bool fin = true;
    for (int k = 0; k < 12; ++k) fin = fin && finite64(t.est_T[12 * static_cast<int64_t>(q) + k]) && finite64(t.gt_T[12 * static_cast<int64_t>(q) + k]);
    if (!fin) return r;
    r.s0 = clamp64(t.sym_begin[c], 0, t.Stot);
    const int64_t ns = clamp64(t.sym_begin[c + 1], r.s0, t.Stot) - r.s0;
    r.ns = static_cast<int>(ns < t.max_syms ? ns : t.max_syms);
    r.identity = r.ns == 0;
    if (r.identity) r.ns = 1;
    r.ok = true;
    return r;
}

template <bool kSurf, bool kProj>
__global__ __launch_bounds__(kThreads) void sym_max_kernel(Tables t, int n_chunks, int s_pad, int Q, double* __restrict__ ws)
{
    const int chunk = blockIdx.x, sblock = blockIdx.y, q = blockIdx.z;
    const int tid = threadIdx.x;
    const Row row = row_of(t, q);
    const int i0 = chunk * kChunk, sb0 = sblock * kSymBlock;
    if (!row.ok || i0 >= row.n || sb0 >= row.ns) return;        // uniform over the workgroup
    const int nsb = min(kSymBlock, row.ns - sb0);
    const double* Te = t.est_T + 12 * static_cast<int64_t>(q);
    const double* Tg = t.gt_T + 12 * static_cast<int64_t>(q);

    __shared__ double comp[kSymBlock][12];                      // [Rg'|tg'] row-major of the block's symmetries
    __shared__ double red[kWaves][2 * kSymBlock];
    if (tid < 12 * kSymBlock) {
        const int s = tid / 12, i = (tid % 12) / 4, j = tid % 4;
        if (s < nsb) {
            const double a0 = Tg[4 * i], a1 = Tg[4 * i + 1], a2 = Tg[4 * i + 2];
            double b0, b1, b2;
            if (row.identity) {
                b0 = j == 0 ? 1.0 : 0.0; b1 = j == 1 ? 1.0 : 0.0; b2 = j == 2 ? 1.0 : 0.0;
            } else if (j < 3) {
                const double* Rs = t.sym_R + 9 * (row.s0 + sb0 + s);
                b0 = Rs[j]; b1 = Rs[3 + j]; b2 = Rs[6 + j];
            } else {
                const double* ts = t.sym_t + 3 * (row.s0 + sb0 + s);
                b0 = ts[0]; b1 = ts[1]; b2 = ts[2];
            }
            double v = (a0 * b0 + a1 * b1) + a2 * b2;
            if (j == 3) v = v + Tg[4 * i + 3];
            comp[s][4 * i + j] = v;
        }
    }
    __syncthreads();

    const double* Kb = t.K + 9 * static_cast<int64_t>(row.b);
    const double fx = Kb[0], fy = Kb[4], cx = Kb[2], cy = Kb[5];
    double e[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) e[k] = Te[k];
    double ms[kSymBlock], mp[kSymBlock];
#pragma unroll
    for (int s = 0; s < kSymBlock; ++s) ms[s] = mp[s] = 0.0;

    const float* p = t.pts + 3 * row.p0;
    for (int k = 0; k < kPer; ++k) {
        const int i = i0 + k * kThreads + tid;
        if (i >= row.n) break;
        const double x = static_cast<double>(p[3 * static_cast<int64_t>(i)]), y = static_cast<double>(p[3 * static_cast<int64_t>(i) + 1]),
                     z = static_cast<double>(p[3 * static_cast<int64_t>(i) + 2]);
        const double Xe = ((e[0] * x + e[1] * y) + e[2] * z) + e[3];
        const double Ye = ((e[4] * x + e[5] * y) + e[6] * z) + e[7];
        const double Ze = ((e[8] * x + e[9] * y) + e[10] * z) + e[11];
        double ue = 0.0, ve = 0.0;
        if (kProj) {
            ue = (fx * Xe) / Ze + cx;
            ve = (fy * Ye) / Ze + cy;
        }
#pragma unroll
        for (int s = 0; s < kSymBlock; ++s) {
            if (s < nsb) {                                      // uniform
                const double* g = comp[s];                      // the same address in every lane: broadcasts
                const double Xg = ((g[0] * x + g[1] * y) + g[2] * z) + g[3];
                const double Yg = ((g[4] * x + g[5] * y) + g[6] * z) + g[7];
                const double Zg = ((g[8] * x + g[9] * y) + g[10] * z) + g[11];
                if (kSurf) {
                    const double dx = Xe - Xg, dy = Ye - Yg, dz = Ze - Zg;
                    const double d2 = (dx * dx + dy * dy) + dz * dz;
                    ms[s] = max64(ms[s], d2 >= 0.0 ? d2 : inf64());
                }
                if (kProj) {
                    const double ug = (fx * Xg) / Zg + cx, vg = (fy * Yg) / Zg + cy;
                    const double du = ue - ug, dv = ve - vg;
                    const double d2 = du * du + dv * dv;
                    mp[s] = max64(mp[s], (Ze > 0.0 && Zg > 0.0 && d2 >= 0.0) ? d2 : inf64());
                }
            }
        }
    }

#pragma unroll
    for (int s = 0; s < kSymBlock; ++s) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            if (kSurf) ms[s] = max64(ms[s], shfl_xor64(ms[s], m));
            if (kProj) mp[s] = max64(mp[s], shfl_xor64(mp[s], m));
        }
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int s = 0; s < kSymBlock; ++s) {
            red[tid >> 6][s] = ms[s];
            red[tid >> 6][kSymBlock + s] = mp[s];
        }
    }
    __syncthreads();
    if (tid < 2 * kSymBlock) {
        const int s = tid % kSymBlock;
        const bool proj = tid >= kSymBlock;
        if (s < nsb && (proj ? kProj : kSurf)) {
            double m = red[0][tid];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) m = max64(m, red[w][tid]);
            const int64_t at = (static_cast<int64_t>(q) * s_pad + sb0 + s) * n_chunks + chunk;
            ws[at + (proj ? static_cast<int64_t>(Q) * s_pad * n_chunks : 0)] = m;
        }
    }
}

__global__ __launch_bounds__(64) void sym_min_kernel(Tables t, int n_chunks, int s_pad, int Q, const double* __restrict__ ws,
                                                     double* __restrict__ mssd2, double* __restrict__ mspd2)
{
    const int q = blockIdx.x, tid = threadIdx.x;
    const Row row = row_of(t, q);
    if (!row.ok) {
        if (tid == 0) {
            if (mssd2) mssd2[q] = __builtin_nan("");
            if (mspd2) mspd2[q] = __builtin_nan("");
        }
        return;
    }
    const int used = (row.n + kChunk - 1) / kChunk;
    const int64_t half = static_cast<int64_t>(Q) * s_pad * n_chunks;
    double bs = inf64(), bp = inf64();
    for (int s = tid; s < row.ns; s += 64) {
        const double* w = ws + (static_cast<int64_t>(q) * s_pad + s) * n_chunks;
        double m_s = 0.0, m_p = 0.0;
        for (int ch = 0; ch < used; ++ch) {
            if (mssd2) m_s = max64(m_s, w[ch]);
            if (mspd2) m_p = max64(m_p, w[half + ch]);
        }
        bs = min64(bs, m_s);
        bp = min64(bp, m_p);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        bs = min64(bs, shfl_xor64(bs, m));
        bp = min64(bp, shfl_xor64(bp, m));
    }
    if (tid == 0) {
        if (mssd2) mssd2[q] = bs;
        if (mspd2) mspd2[q] = bp;
    }
}

// ---- VSD ----------------------------------------------------------------------------------------------------------------------

// Camera, ray_dist and load_px: csrc/bop_common.h

__device__ __forceinline__ bool vsd_row_ok(const int* class_of, const int* frame_of, int q, int n_cls, int B)
{
    const int c = class_of[q], b = frame_of[q];
    return c >= 0 && c < n_cls && b >= 0 && b < B;
}

template <int kVec>
__global__ __launch_bounds__(kThreads) void vsd_count_kernel(const float* __restrict__ depth_test, const float* __restrict__ depth_est,
                                                             const float* __restrict__ depth_gt, const int* __restrict__ class_of,
                                                             const int* __restrict__ frame_of, const double* __restrict__ K, int B, int HW,
                                                             int W, const float* __restrict__ diameter, int n_cls, float delta,
                                                             const float* __restrict__ taus, int n_tau, int* __restrict__ partial,
                                                             int n_parts)
{
    __shared__ int red[kWaves][kCounters];
    const int q = blockIdx.y, tid = threadIdx.x;
    if (!vsd_row_ok(class_of, frame_of, q, n_cls, B)) return;   // uniform; the finish kernel does not read this row's partial counts
    const int b = frame_of[q];
    const float diam = diameter[class_of[q]];
    Camera cam;
    const double* Kb = K + 9 * static_cast<int64_t>(b);
    cam.fx = static_cast<float>(Kb[0]); cam.fy = static_cast<float>(Kb[4]);
    cam.cx = static_cast<float>(Kb[2]); cam.cy = static_cast<float>(Kb[5]);
    float tau[FFB6D_BOP_MAX_TAUS];
#pragma unroll
    for (int k = 0; k < FFB6D_BOP_MAX_TAUS; ++k) tau[k] = k < n_tau ? taus[k] : 0.f;
    const float* it = depth_test + static_cast<int64_t>(b) * HW;
    const float* ie = depth_est + static_cast<int64_t>(q) * HW;
    const float* ig = depth_gt + static_cast<int64_t>(q) * HW;
    const int lo = blockIdx.x * kRunPx;                         // < HW <= INT_MAX - kRunPx: lo + kRunPx does not overflow
    const int hi = HW - lo > kRunPx ? lo + kRunPx : HW;
    int cnt[kCounters];
#pragma unroll
    for (int k = 0; k < kCounters; ++k) cnt[k] = 0;
    for (int step = 0; step < kSteps; ++step) {
        const int p0 = lo + (step * kThreads + tid) * kPx;
        if (p0 >= hi) break;
        const int n = hi - p0 >= kPx ? kPx : hi - p0;
        float zt[kPx], ze[kPx], zg[kPx];
        load_px<kVec>(it + p0, n, zt);
        load_px<kVec>(ie + p0, n, ze);
        load_px<kVec>(ig + p0, n, zg);
#pragma unroll
        for (int j = 0; j < kPx; ++j) {
            if (j < n) {
                const int r = (p0 + j) / W, c = (p0 + j) - r * W;
                const float t = (zt[j] > 0.f && zt[j] <= FLT_MAX) ? zt[j] : 0.f;     // not finite or <= 0: no measurement
                const float dt = ray_dist(t, r, c, cam), de = ray_dist(ze[j], r, c, cam), dg = ray_dist(zg[j], r, c, cam);
                const bool vis_gt = dg > 0.f && (dt == 0.f || dg - dt <= delta);
                const bool vis_est = de > 0.f && (dt == 0.f || de - dt <= delta || vis_gt);
                cnt[0] += (vis_gt || vis_est) ? 1 : 0;
                if (vis_gt && vis_est) {
                    cnt[1] += 1;
                    const float err = fabsf(dg - de) / diam;
#pragma unroll
                    for (int k = 0; k < FFB6D_BOP_MAX_TAUS; ++k) cnt[2 + k] += (k < n_tau && err >= tau[k]) ? 1 : 0;
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kCounters; ++k) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) cnt[k] += __shfl_xor(cnt[k], m, 64);
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < kCounters; ++k) red[tid >> 6][k] = cnt[k];
    }
    __syncthreads();
    if (tid < kCounters) {
        int s = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) s += red[w][tid];
        partial[(static_cast<int64_t>(q) * n_parts + blockIdx.x) * kCounters + tid] = s;
    }
}

__global__ __launch_bounds__(64) void vsd_finish_kernel(const int* __restrict__ class_of, const int* __restrict__ frame_of, int n_cls, int B,
                                                        const int* __restrict__ partial, int n_parts, int n_tau, int* __restrict__ counts,
                                                        double* __restrict__ vsd)
{
    const int q = blockIdx.x, tid = threadIdx.x;
    int* cq = counts + static_cast<int64_t>(q) * (2 + n_tau);
    double* vq = vsd + static_cast<int64_t>(q) * n_tau;
    if (!vsd_row_ok(class_of, frame_of, q, n_cls, B)) {
        if (tid < 2 + n_tau) cq[tid] = 0;
        if (tid < n_tau) vq[tid] = __builtin_nan("");
        return;
    }
    int cnt[kCounters];
#pragma unroll
    for (int k = 0; k < kCounters; ++k) cnt[k] = 0;
    for (int i = tid; i < n_parts; i += 64) {
        const int* p = partial + (static_cast<int64_t>(q) * n_parts + i) * kCounters;
#pragma unroll
        for (int k = 0; k < kCounters; ++k) cnt[k] += p[k];
    }
#pragma unroll
    for (int k = 0; k < kCounters; ++k) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) cnt[k] += __shfl_xor(cnt[k], m, 64);
    }
    if (tid == 0) {
        cq[0] = cnt[0];
        cq[1] = cnt[1];
#pragma unroll
        for (int k = 0; k < FFB6D_BOP_MAX_TAUS; ++k) {
            if (k < n_tau) {
                cq[2 + k] = cnt[2 + k];
                vq[k] = cnt[0] == 0 ? 1.0 : static_cast<double>(cnt[2 + k] + (cnt[0] - cnt[1])) / static_cast<double>(cnt[0]);
            }
        }
    }
}

inline int64_t sym_pad(int64_t max_syms) { return ffb6d::ceil_div(max_syms > 0 ? max_syms : 1, kSymBlock) * kSymBlock; }

}  // namespace

extern "C" {

size_t ffb6d_bop_mssd_mspd_workspace_bytes(int Q, int64_t max_points, int64_t max_syms)
{
    if (Q <= 0 || max_points <= 0 || max_syms < 0 || max_points > INT_MAX - kChunk || max_syms > INT_MAX - kSymBlock) return 0;
    const size_t bytes = static_cast<size_t>(Q) * static_cast<size_t>(sym_pad(max_syms)) *
                         static_cast<size_t>(ffb6d::ceil_div(max_points, kChunk)) * 2 * sizeof(double);
    return (bytes + 255) / 256 * 256;
}

int ffb6d_bop_mssd_mspd_f64(const float* model_pts, const int64_t* model_begin, int n_cls, int64_t total, int64_t max_points,
                            const double* sym_R, const double* sym_t, const int64_t* sym_begin, int64_t Stot, int64_t max_syms,
                            const int* class_of, const int* frame_of, const double* est_T, const double* gt_T, int Q,
                            const double* K, int B, double* mssd2, double* mspd2, void* workspace, size_t workspace_bytes,
                            ffb6d_stream_t stream)
{
    FFB6D_REQUIRE(Q >= 0 && Q <= 65535 && n_cls > 0 && B > 0, "ffb6d_bop_mssd_mspd_f64: bad sizes Q = %d (at most 65535), n_cls = %d, B = %d",
                  Q, n_cls, B);
    FFB6D_REQUIRE(total >= 0 && max_points >= 0 && max_points <= total && max_points <= INT_MAX - kChunk && Stot >= 0 && max_syms >= 0 &&
                      max_syms <= Stot && sym_pad(max_syms) / kSymBlock <= 65535,
                  "ffb6d_bop_mssd_mspd_f64: bad tables: total = %lld, max_points = %lld, Stot = %lld, max_syms = %lld (at most %d)",
                  static_cast<long long>(total), static_cast<long long>(max_points), static_cast<long long>(Stot),
                  static_cast<long long>(max_syms), 65535 * kSymBlock);
    FFB6D_REQUIRE(mssd2 || mspd2, "ffb6d_bop_mssd_mspd_f64: no output");
    if (Q == 0) return FFB6D_OK;
    FFB6D_REQUIRE(model_begin && sym_begin && class_of && frame_of && est_T && gt_T && K && (model_pts || total == 0) &&
                      ((sym_R && sym_t) || Stot == 0),
                  "ffb6d_bop_mssd_mspd_f64: a null pointer");
    const size_t need = ffb6d_bop_mssd_mspd_workspace_bytes(Q, max_points, max_syms);
    if (workspace_bytes < need || (need > 0 && (workspace == nullptr || !aligned(workspace, 8))))
        return ffb6d::set_error(FFB6D_ERR_WORKSPACE, "ffb6d_bop_mssd_mspd_f64: workspace of %zu bytes, %zu needed (or null, or not 8-byte aligned)",
                                workspace_bytes, need);
    const Tables t{model_pts, model_begin, n_cls, total, max_points, sym_R, sym_t, sym_begin, Stot, max_syms,
                   class_of, frame_of, est_T, gt_T, K, B};
    const int s_pad = static_cast<int>(sym_pad(max_syms));
    const int n_chunks = static_cast<int>(ffb6d::ceil_div(max_points, kChunk));
    FFB6D_REQUIRE(n_chunks <= INT_MAX / 2, "ffb6d_bop_mssd_mspd_f64: %d point chunks", n_chunks);
    hipStream_t st = ffb6d::as_stream(stream);
    double* ws = static_cast<double*>(workspace);
    if (n_chunks > 0) {
        const dim3 grid(static_cast<unsigned>(n_chunks), static_cast<unsigned>(s_pad / kSymBlock), static_cast<unsigned>(Q));
        if (mssd2 && mspd2) sym_max_kernel<true, true><<<grid, dim3(kThreads), 0, st>>>(t, n_chunks, s_pad, Q, ws);
        else if (mssd2) sym_max_kernel<true, false><<<grid, dim3(kThreads), 0, st>>>(t, n_chunks, s_pad, Q, ws);
        else sym_max_kernel<false, true><<<grid, dim3(kThreads), 0, st>>>(t, n_chunks, s_pad, Q, ws);
        FFB6D_LAUNCH_CHECK();
    }
    sym_min_kernel<<<dim3(static_cast<unsigned>(Q)), dim3(64), 0, st>>>(t, n_chunks, s_pad, Q, ws, mssd2, mspd2);
    FFB6D_LAUNCH_CHECK();
    return FFB6D_OK;
}

size_t ffb6d_bop_vsd_workspace_bytes(int Q, int H, int W)
{
    if (Q <= 0 || H <= 0 || W <= 0 || static_cast<int64_t>(H) * W > INT_MAX - kRunPx) return 0;
    const size_t bytes = static_cast<size_t>(Q) * static_cast<size_t>(ffb6d::ceil_div(static_cast<int64_t>(H) * W, kRunPx)) * kCounters * sizeof(int);
    return (bytes + 255) / 256 * 256;
}

int ffb6d_bop_vsd_f32(const float* depth_test, const float* depth_est, const float* depth_gt, const int* class_of,
                      const int* frame_of, int Q, const double* K, int B, int H, int W, const float* diameter, int n_cls,
                      float delta, const float* taus, int n_tau, int* counts, double* vsd, void* workspace,
                      size_t workspace_bytes, ffb6d_stream_t stream)
{
    FFB6D_REQUIRE(Q >= 0 && Q <= 65535 && n_cls > 0 && B > 0 && H > 0 && W > 0 && static_cast<int64_t>(H) * W <= INT_MAX - kRunPx,
                  "ffb6d_bop_vsd_f32: bad sizes Q = %d (at most 65535), n_cls = %d, B = %d, H = %d, W = %d (H*W < 2^31 - 4096)", Q, n_cls, B, H, W);
    FFB6D_REQUIRE(n_tau >= 1 && n_tau <= FFB6D_BOP_MAX_TAUS, "ffb6d_bop_vsd_f32: n_tau = %d outside [1, %d]", n_tau, FFB6D_BOP_MAX_TAUS);
    if (Q == 0) return FFB6D_OK;
    FFB6D_REQUIRE(depth_test && depth_est && depth_gt && class_of && frame_of && K && diameter && taus && counts && vsd,
                  "ffb6d_bop_vsd_f32: a null pointer");
    const size_t need = ffb6d_bop_vsd_workspace_bytes(Q, H, W);
    if (workspace == nullptr || workspace_bytes < need || !aligned(workspace, 4))
        return ffb6d::set_error(FFB6D_ERR_WORKSPACE, "ffb6d_bop_vsd_f32: workspace of %zu bytes, %zu needed (or null, or not 4-byte aligned)",
                                workspace_bytes, need);
    const int HW = H * W;
    const int n_parts = static_cast<int>(ffb6d::ceil_div(HW, kRunPx));
    int* partial = static_cast<int*>(workspace);
    hipStream_t st = ffb6d::as_stream(stream);
    const dim3 grid(static_cast<unsigned>(n_parts), static_cast<unsigned>(Q));
    if (HW % 4 == 0 && aligned(depth_test, 16) && aligned(depth_est, 16) && aligned(depth_gt, 16))
        vsd_count_kernel<4><<<grid, dim3(kThreads), 0, st>>>(depth_test, depth_est, depth_gt, class_of, frame_of, K, B, HW, W, diameter, n_cls,
                                                             delta, taus, n_tau, partial, n_parts);
    else
        vsd_count_kernel<1><<<grid, dim3(kThreads), 0, st>>>(depth_test, depth_est, depth_gt, class_of, frame_of, K, B, HW, W, diameter, n_cls,
                                                             delta, taus, n_tau, partial, n_parts);
    FFB6D_LAUNCH_CHECK();
    vsd_finish_kernel<<<dim3(static_cast<unsigned>(Q)), dim3(64), 0, st>>>(class_of, frame_of, n_cls, B, partial, n_parts, n_tau, counts, vsd);
    FFB6D_LAUNCH_CHECK();
    return FFB6D_OK;
}

}  // extern "C"
