// ffb6d_amd/csrc/render.hip -- gfx950 z-buffer rasteriser of posed, vertex-coloured triangle meshes (include/ffb6d_render.h):
// I instances (frame, class, pose) into B frames of rgb / depth / label.  The reference has its synthetic frames made by an
// external library whose source it does not carry; the algorithm is stated in the header and restated in numpy by
// tests/render_ref.py.
//
// Per call:
//   render_vertex_kernel   thread = (instance, vertex): camera frame and projection in double, the screen vertex
//                          {Xs, Ys in 1/256 pixel, zf, usable} written once per instance
//   render_raster_kernel   thread = (instance, face): set-up in integers (exact), then the candidate pixels of the clamped
//                          bounding box; every covered sample sends key = depth bits << 32 | instance << 22 | face to the key
//                          image with a 64-bit global minimum atomic (no return value: the lane does not wait for it)
//   render_resolve_kernel  thread = pixel, after the kernel boundary: the winning key names (instance, face); barycentrics and
//                          colour are recomputed from that one triangle with the raster pass's own arithmetic
// The smallest key wins whatever the arrival order, so every run and every form gives the same bits.
//
// Two ways to walk the candidate pixels, same results (the per-sample arithmetic is one function):
//   form 0  the lane walks its own triangle's box: right for meshes at working distance (a few pixels per triangle)
//   form 1  the triangles of a wavefront are taken one at a time by all 64 lanes, the box cut into 8 x 8 pixel tiles: a
//           close-up triangle of tens of thousands of samples no longer serialises on one lane
//   form -1 both in one launch: boxes of more than kWaveArea pixels go the second way
#include <cmath>

#include "common.h"
#include "ffb6d_render.h"

namespace {

using ffb6d::ceil_div;

constexpr int kBlock = 256;
constexpr int kInstBits = 10, kFaceBits = 22;
constexpr long long kWaveArea = 256;          // form -1: a box of more candidate pixels than this is walked by the wavefront
constexpr unsigned long long kNoKey = ~0ull;  // above every key: the depth bits of a key are those of a positive float
constexpr double kSubPixel = 256.0, kMaxScreen = 8388608.0;      // 2^23 sub-pixel units

struct alignas(16) ScreenVert { int xs, ys; float zf; int usable; };

struct Meshes {
    const float* verts;
    const unsigned char* colors;
    const int* faces;
    const int64_t* vert_begin;
    const int64_t* face_begin;
    int n_cls;
    int64_t Vtot, Ftot, max_verts, max_faces;
};

struct Scene {
    const int* frame_of;
    const int* class_of;
    const double* T;
    const double* K;
    int I, B, H, W;
    float z_near;
};

struct ClassRange { int64_t vb, fb; int nv, nf; };

// three screen vertices (after the swap that makes A2 positive), their indices within the class, and what follows from them
struct Tri {
    int x[3], y[3];
    float zf[3];
    int vi[3];
    long long a2;
    int cmin, cmax, rmin, rmax;               // candidate pixels; empty when cmin > cmax or rmin > rmax
};

size_t align256(size_t x) { return (x + 255) & ~static_cast<size_t>(255); }

int g_form = 0;

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// rows of class c, clamped so that no table content leads outside the arrays
__device__ __forceinline__ ClassRange class_range(const Meshes& m, int c)
{
    ClassRange r;
    r.vb = clamp64(m.vert_begin[c], 0, m.Vtot);
    r.fb = clamp64(m.face_begin[c], 0, m.Ftot);
    const int64_t nv = clamp64(m.vert_begin[c + 1], r.vb, m.Vtot) - r.vb, nf = clamp64(m.face_begin[c + 1], r.fb, m.Ftot) - r.fb;
    r.nv = static_cast<int>(nv < m.max_verts ? nv : m.max_verts);
    r.nf = static_cast<int>(nf < m.max_faces ? nf : m.max_faces);
    return r;
}

__device__ __forceinline__ bool instance_ok(const Meshes& m, const Scene& s, int i, int& frame, int& cls)
{
    frame = s.frame_of[i];
    cls = s.class_of[i];
    return frame >= 0 && frame < s.B && cls >= 0 && cls < m.n_cls;
}

__global__ __launch_bounds__(kBlock) void render_vertex_kernel(Meshes m, Scene s, ScreenVert* sv)
{
    const int i = blockIdx.y;
    const int64_t v = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    int frame, cls;
    if (!instance_ok(m, s, i, frame, cls)) return;
    const ClassRange r = class_range(m, cls);
    if (v >= r.nv) return;
    const float* p = m.verts + 3 * (r.vb + v);
    const double x = p[0], y = p[1], z = p[2];
    const double* t = s.T + 12 * static_cast<int64_t>(i);
    const double* k = s.K + 9 * static_cast<int64_t>(frame);
    const double xc = ((t[0] * x + t[1] * y) + t[2] * z) + t[3];
    const double yc = ((t[4] * x + t[5] * y) + t[6] * z) + t[7];
    const double zc = ((t[8] * x + t[9] * y) + t[10] * z) + t[11];
    const float zf = static_cast<float>(zc);
    const double su = kSubPixel * ((k[0] * xc) / zc + k[2]);
    const double sw = kSubPixel * ((k[4] * yc) / zc + k[5]);
    const bool ok = (zf >= s.z_near) && (fabs(su) <= kMaxScreen) && (fabs(sw) <= kMaxScreen);      // false for NaN
    ScreenVert o;
    o.xs = ok ? static_cast<int>(llrint(su)) : 0;
    o.ys = ok ? static_cast<int>(llrint(sw)) : 0;
    o.zf = zf;
    o.usable = ok ? 1 : 0;
    sv[static_cast<int64_t>(i) * m.max_verts + v] = o;
}

// A2, the swap, the candidate pixels.  false: the triangle covers nothing.
__device__ __forceinline__ bool derive(Tri& t, int H, int W)
{
    long long a2 = static_cast<long long>(t.x[1] - t.x[0]) * (t.y[2] - t.y[0]) - static_cast<long long>(t.x[2] - t.x[0]) * (t.y[1] - t.y[0]);
    if (a2 == 0) return false;
    if (a2 < 0) {
        const int x = t.x[1], y = t.y[1], vi = t.vi[1];
        const float zf = t.zf[1];
        t.x[1] = t.x[2]; t.y[1] = t.y[2]; t.vi[1] = t.vi[2]; t.zf[1] = t.zf[2];
        t.x[2] = x; t.y[2] = y; t.vi[2] = vi; t.zf[2] = zf;
        a2 = -a2;
    }
    t.a2 = a2;
    const int xlo = min(t.x[0], min(t.x[1], t.x[2])), xhi = max(t.x[0], max(t.x[1], t.x[2]));
    const int ylo = min(t.y[0], min(t.y[1], t.y[2])), yhi = max(t.y[0], max(t.y[1], t.y[2]));
    t.cmin = max(0, (xlo + 255) >> 8);        // the first sample at or right of xlo (>> floors)
    t.cmax = min(W - 1, xhi >> 8);
    t.rmin = max(0, (ylo + 255) >> 8);
    t.rmax = min(H - 1, yhi >> 8);
    return true;
}

// the triangle of (instance, face f of its class) from the screen vertices; false: dropped
__device__ __forceinline__ bool load_tri(const Meshes& m, const ClassRange& r, const ScreenVert* sv_inst, int f, int H, int W, Tri& t)
{
    const int* fv = m.faces + 3 * (r.fb + f);
    bool ok = true;
    for (int k = 0; k < 3; ++k) {
        const int vi = fv[k];
        t.vi[k] = vi;
        if (vi < 0 || vi >= r.nv) { ok = false; t.x[k] = t.y[k] = 0; t.zf[k] = 0.f; continue; }
        const ScreenVert q = sv_inst[vi];
        t.x[k] = q.xs; t.y[k] = q.ys; t.zf[k] = q.zf;
        ok = ok && q.usable != 0;
    }
    return ok && derive(t, H, W);
}

__device__ __forceinline__ bool owns(long long e, int dx, int dy) { return e > 0 || (e == 0 && (dy > 0 || (dy == 0 && dx < 0))); }

// edge functions of the sample of pixel (row, col); true when it is covered
__device__ __forceinline__ bool sample(const Tri& t, int row, int col, long long e[3])
{
    const int px = col << 8, py = row << 8;
    bool in = true;
    for (int i = 0; i < 3; ++i) {
        const int a = i == 2 ? 0 : i + 1, b = i == 0 ? 2 : i - 1;          // edge i: a -> b, the other two in cyclic order
        const int dx = t.x[b] - t.x[a], dy = t.y[b] - t.y[a];
        e[i] = static_cast<long long>(dx) * (py - t.y[a]) - static_cast<long long>(dy) * (px - t.x[a]);
        in = in && owns(e[i], dx, dy);
    }
    return in;
}

// biz[i] = b_i * iz_i; returns w
__device__ __forceinline__ double weights(const Tri& t, const long long e[3], double biz[3])
{
    const double a = static_cast<double>(t.a2);
    for (int i = 0; i < 3; ++i) {
        const double b = static_cast<double>(e[i]) / a;
        const double iz = 1.0 / static_cast<double>(t.zf[i]);
        biz[i] = b * iz;
    }
    return (biz[0] + biz[1]) + biz[2];
}

__device__ __forceinline__ void shade(const Tri& t, int row, int col, unsigned long long low, unsigned long long* frame_keys, int W)
{
    long long e[3];
    if (!sample(t, row, col, e)) return;
    double biz[3];
    const double w = weights(t, e, biz);
    const float z = static_cast<float>(1.0 / w);
    const unsigned long long key = (static_cast<unsigned long long>(__float_as_uint(z)) << 32) | low;
    atomicMin(frame_keys + static_cast<int64_t>(row) * W + col, key);
}

__global__ __launch_bounds__(kBlock) void render_raster_kernel(Meshes m, Scene s, const ScreenVert* sv, unsigned long long* keys, int form)
{
    const int i = blockIdx.y;
    const int64_t f64 = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    int frame, cls;
    Tri t = {};
    bool live = false;
    unsigned long long* frame_keys = keys;
    if (instance_ok(m, s, i, frame, cls)) {                                  // block-uniform
        const ClassRange r = class_range(m, cls);
        if (f64 < r.nf) live = load_tri(m, r, sv + static_cast<int64_t>(i) * m.max_verts, static_cast<int>(f64), s.H, s.W, t);
        frame_keys = keys + static_cast<int64_t>(frame) * s.H * s.W;
    }
    live = live && t.cmin <= t.cmax && t.rmin <= t.rmax;
    const unsigned low = (static_cast<unsigned>(i) << kFaceBits) | static_cast<unsigned>(f64);
    bool wide = false;
    if (live && form != 0)
        wide = form > 0 || static_cast<long long>(t.cmax - t.cmin + 1) * (t.rmax - t.rmin + 1) > kWaveArea;
    if (live && !wide)
        for (int row = t.rmin; row <= t.rmax; ++row)
            for (int col = t.cmin; col <= t.cmax; ++col) shade(t, row, col, low, frame_keys, s.W);
    if (form == 0) return;                                                   // kernel-uniform
    // the wavefront takes its wide triangles one after the other: every lane gets the triangle of lane `src`
    const int lane = threadIdx.x & 63, lx = lane & 7, ly = lane >> 3;
    unsigned long long todo = __ballot(wide);
    while (todo != 0) {
        const int src = __ffsll(static_cast<long long>(todo)) - 1;
        todo &= todo - 1;
        Tri q;
        for (int k = 0; k < 3; ++k) {
            q.x[k] = __shfl(t.x[k], src, 64);
            q.y[k] = __shfl(t.y[k], src, 64);
            q.zf[k] = __shfl(t.zf[k], src, 64);
            q.vi[k] = 0;
        }
        const unsigned qlow = __shfl(low, src, 64);
        derive(q, s.H, s.W);                                                 // already swapped: A2 and the box again
        for (int r0 = q.rmin; r0 <= q.rmax; r0 += 8)
            for (int c0 = q.cmin; c0 <= q.cmax; c0 += 8) {
                const int row = r0 + ly, col = c0 + lx;
                if (row <= q.rmax && col <= q.cmax) shade(q, row, col, qlow, frame_keys, s.W);
            }
    }
}

__global__ __launch_bounds__(kBlock) void render_resolve_kernel(Meshes m, Scene s, const ScreenVert* sv, const unsigned long long* keys,
                                                                unsigned char* rgb, float* depth, int* label, int* inst, int* face,
                                                                int* visible)
{
    const int64_t hw = static_cast<int64_t>(s.H) * s.W, n = hw * s.B;
    const int64_t p = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    int owner = -1;
    if (p < n) {
        const unsigned long long key = keys[p];
        const unsigned pu = static_cast<unsigned>(p), hwu = static_cast<unsigned>(hw);        // n < 2^31
        const int64_t b = pu / hwu, rem = pu - static_cast<unsigned>(b) * hwu;
        float z = 0.f;
        int lab = 0, f = -1;
        unsigned char c[3] = {0, 0, 0};
        if (key != kNoKey) {
            z = __uint_as_float(static_cast<unsigned>(key >> 32));
            owner = static_cast<int>((key >> kFaceBits) & ((1u << kInstBits) - 1));
            f = static_cast<int>(key & ((1u << kFaceBits) - 1));
            lab = s.class_of[owner];
            if (rgb) {
                const int row = static_cast<int>(static_cast<unsigned>(rem) / static_cast<unsigned>(s.W)), col = static_cast<int>(rem) - row * s.W;
                const ClassRange r = class_range(m, lab);
                Tri t;
                load_tri(m, r, sv + static_cast<int64_t>(owner) * m.max_verts, f, s.H, s.W, t);
                long long e[3];
                sample(t, row, col, e);
                double biz[3];
                const double w = weights(t, e, biz);
                const unsigned char* c0 = m.colors + 3 * (r.vb + t.vi[0]);
                const unsigned char* c1 = m.colors + 3 * (r.vb + t.vi[1]);
                const unsigned char* c2 = m.colors + 3 * (r.vb + t.vi[2]);
                for (int ch = 0; ch < 3; ++ch) {
                    const double v = ((biz[0] * c0[ch] + biz[1] * c1[ch]) + biz[2] * c2[ch]) / w;
                    const double q = floor(v + 0.5);
                    c[ch] = static_cast<unsigned char>(q < 255.0 ? (q > 0.0 ? q : 0.0) : 255.0);      // min(255, .); c >= 0
                }
            }
        }
        if (rgb)
            for (int ch = 0; ch < 3; ++ch) rgb[(b * 3 + ch) * hw + rem] = c[ch];
        if (depth) depth[p] = z;
        if (label) label[p] = lab;
        if (inst) inst[p] = owner;
        if (face) face[p] = f;
    }
    if (visible == nullptr) return;                                          // kernel-uniform
    // pixels of one wavefront mostly share their owner: one add per distinct owner and wavefront
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(owner >= 0);
    while (todo != 0) {
        const int src = __ffsll(static_cast<long long>(todo)) - 1;
        const int lead = __shfl(owner, src, 64);
        const unsigned long long same = __ballot(owner == lead);
        if (lane == src) atomicAdd(visible + lead, __popcll(same));
        todo &= ~same;
    }
}

struct Workspace { unsigned long long* keys; ScreenVert* sv; size_t keys_bytes, bytes; };

Workspace workspace_layout(void* base, int I, int64_t max_verts, int B, int H, int W)
{
    Workspace w;
    char* p = static_cast<char*>(base);
    w.keys_bytes = sizeof(unsigned long long) * static_cast<size_t>(B) * H * W;
    size_t off = align256(w.keys_bytes);
    w.keys = reinterpret_cast<unsigned long long*>(p);
    w.sv = reinterpret_cast<ScreenVert*>(p + off);
    off += align256(sizeof(ScreenVert) * static_cast<size_t>(I) * static_cast<size_t>(max_verts));
    w.bytes = off;
    return w;
}

bool sizes_ok(int I, int64_t max_verts, int B, int H, int W)
{
    return I >= 0 && I <= FFB6D_RENDER_MAX_INSTANCES && max_verts >= 0 && max_verts < (int64_t(1) << 31) && B > 0 && H > 0 && W > 0 &&
           static_cast<int64_t>(B) * H * W < (int64_t(1) << 31);
}

}  // namespace

extern "C" {

void ffb6d_render_set_form(int form) { g_form = form < 0 ? -1 : (form ? 1 : 0); }

size_t ffb6d_render_workspace_bytes(int I, int64_t max_verts, int B, int H, int W)
{
    if (!sizes_ok(I, max_verts, B, H, W)) return 0;
    return workspace_layout(nullptr, I, max_verts, B, H, W).bytes;
}

int ffb6d_render_f32(const float* verts, const unsigned char* colors, const int* faces, const int64_t* vert_begin,
                     const int64_t* face_begin, int n_cls, int64_t Vtot, int64_t Ftot, int64_t max_verts, int64_t max_faces,
                     const int* frame_of, const int* class_of, const double* T, int I, const double* K, int B, int H, int W,
                     float z_near, unsigned char* rgb, float* depth, int* label, int* inst, int* face, int* visible,
                     void* workspace, size_t workspace_bytes, ffb6d_stream_t stream)
{
    FFB6D_REQUIRE(sizes_ok(I, max_verts, B, H, W), "render: bad sizes I=%d (at most %d) max_verts=%lld B=%d H=%d W=%d (B*H*W < 2^31)", I,
                  FFB6D_RENDER_MAX_INSTANCES, (long long)max_verts, B, H, W);
    FFB6D_REQUIRE(n_cls > 0 && Vtot >= 0 && Ftot >= 0 && max_verts <= Vtot && max_faces >= 0 && max_faces <= Ftot,
                  "render: bad mesh set n_cls=%d Vtot=%lld Ftot=%lld max_verts=%lld max_faces=%lld", n_cls, (long long)Vtot, (long long)Ftot,
                  (long long)max_verts, (long long)max_faces);
    FFB6D_REQUIRE(max_faces <= FFB6D_RENDER_MAX_FACES, "render: max_faces %lld above 2^22 faces per class", (long long)max_faces);
    FFB6D_REQUIRE(z_near > 0.f, "render: z_near must be positive, got %g", (double)z_near);
    FFB6D_REQUIRE(rgb || depth || label || inst || face || visible, "render: no output given");
    const bool draw = I > 0 && max_verts > 0 && max_faces > 0;
    FFB6D_REQUIRE(vert_begin && face_begin && (Vtot == 0 || (verts && colors)) && (Ftot == 0 || faces), "render: null pointer in the mesh set");
    FFB6D_REQUIRE(I == 0 || (frame_of && class_of && T && K), "render: null pointer in the call");
    const size_t need = ffb6d_render_workspace_bytes(I, max_verts, B, H, W);
    if (!workspace || workspace_bytes < need)
        return ffb6d::set_error(FFB6D_ERR_WORKSPACE, "render: workspace %zu < %zu bytes", workspace_bytes, need);
    hipStream_t st = ffb6d::as_stream(stream);
    const Workspace w = workspace_layout(workspace, I, max_verts, B, H, W);
    Meshes m;
    m.verts = verts; m.colors = colors; m.faces = faces; m.vert_begin = vert_begin; m.face_begin = face_begin; m.n_cls = n_cls;
    m.Vtot = Vtot; m.Ftot = Ftot; m.max_verts = max_verts; m.max_faces = max_faces;
    Scene s;
    s.frame_of = frame_of; s.class_of = class_of; s.T = T; s.K = K; s.I = I; s.B = B; s.H = H; s.W = W; s.z_near = z_near;
    FFB6D_HIP_TRY(hipMemsetAsync(w.keys, 0xff, w.keys_bytes, st));
    if (visible && I > 0) FFB6D_HIP_TRY(hipMemsetAsync(visible, 0, sizeof(int) * I, st));
    if (draw) {
        render_vertex_kernel<<<dim3(static_cast<unsigned>(ceil_div(max_verts, kBlock)), static_cast<unsigned>(I)), kBlock, 0, st>>>(m, s, w.sv);
        FFB6D_LAUNCH_CHECK();
        render_raster_kernel<<<dim3(static_cast<unsigned>(ceil_div(max_faces, kBlock)), static_cast<unsigned>(I)), kBlock, 0, st>>>(
            m, s, w.sv, w.keys, g_form);
        FFB6D_LAUNCH_CHECK();
    }
    if (rgb || depth || label || inst || face || (visible && I > 0)) {
        const int64_t n = static_cast<int64_t>(B) * H * W;
        render_resolve_kernel<<<static_cast<unsigned>(ceil_div(n, kBlock)), kBlock, 0, st>>>(m, s, w.sv, w.keys, rgb, depth, label, inst, face,
                                                                                              visible);
        FFB6D_LAUNCH_CHECK();
    }
    return 0;
}

}  // extern "C"
