// scripts/probes/wino4_phase_probe.hip -- where does the time of the fused Winograd convolution (csrc/winograd_fused.h) go?
// Phase-removal builds of both workgroup shapes (form 1: one workgroup per CU; form 3: two), each leaving ONE phase out -- the input
// transform (LDS left as it is), the MFMAs, the reloads of U (the first two groups' fragments are held), the epilogue -- timed alone on
// the chip with device events next to the full kernel, on the three layer shapes of the benchmark.  The results of the partial builds
// mean nothing and are never looked at; the library never launches them.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -Iinclude -Iffb6d_amd/csrc scripts/probes/wino4_phase_probe.hip \
//         ffb6d_amd/csrc/errors.hip -o wino4_phase_probe
//   ./wino4_phase_probe            one line per (shape, form, build): median / min / max of 5 rounds of 20 launches, microseconds
//   ./wino4_phase_probe full       the two full kernels only
//   ./wino4_phase_probe full pmc N ... shape N (0, 1, 2) only, 6 launches per form (for a counter run: rocprofv3 --pmc ... -- ./wino4_phase_probe full pmc N)
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "winograd_fused.h"

using namespace ffb6d;
using namespace ffb6d::wino;

#define CHECK(e)                                                                                          \
    do {                                                                                                  \
        hipError_t err__ = (e);                                                                           \
        if (err__ != hipSuccess) {                                                                        \
            fprintf(stderr, "%s: %s (line %d)\n", #e, hipGetErrorString(err__), __LINE__);               \
            return 1;                                                                                     \
        }                                                                                                 \
    } while (0)

__global__ void fill_kernel(float* p, size_t n, unsigned seed)
{
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const unsigned h = ((unsigned)i + seed) * 2654435761u;
        p[i] = (float)(h >> 8) * (1.f / 16777216.f) - .5f;
    }
}

struct Shape { int B, H, W, C, O; };
struct Args {
    const float *x, *u, *scale, *shift, *res;
    float* out;
    WinoGeom g;
    int O;
    unsigned xb, ub, ob;
};

template <int FORM, int SKIP>
void launch(const Args& a)
{
    const dim3 grid((unsigned)ceil_div(a.g.T, 16), (unsigned)(a.O / 64));
    if constexpr (FORM == 1)
        hipLaunchKernelGGL((wino4_conv_f32_kernel<4, 64, SKIP>), grid, dim3(256), 0, 0, a.x, a.u, a.scale, a.shift, a.res, nullptr, nullptr,
                           a.out, a.g, a.O, a.xb, a.ub, a.ob, 0.f);
    else
        hipLaunchKernelGGL(wino4_conv2_f32_kernel<SKIP>, grid, dim3(256), 0, 0, a.x, a.u, a.scale, a.shift, a.res, nullptr, nullptr, a.out,
                           a.g, a.O, a.xb, a.ub, a.ob, 0.f);
}

typedef void (*Launch)(const Args&);
struct Build { const char* name; Launch form1, form3; };
static const Build BUILDS[] = {
    {"full", launch<1, 0>, launch<3, 0>},
    {"no_transform", launch<1, SKIP_TRANSFORM>, launch<3, SKIP_TRANSFORM>},
    {"no_mfma", launch<1, SKIP_MFMA>, launch<3, SKIP_MFMA>},
    {"no_u_reload", launch<1, SKIP_U>, launch<3, SKIP_U>},
    {"no_epilogue", launch<1, SKIP_EPILOGUE>, launch<3, SKIP_EPILOGUE>},
    {"mfma_only", launch<1, SKIP_TRANSFORM | SKIP_U | SKIP_EPILOGUE>, launch<3, SKIP_TRANSFORM | SKIP_U | SKIP_EPILOGUE>},
};

int main(int argc, char** argv)
{
    const char* const only = argc > 1 ? argv[1] : nullptr;      // one build by name
    const bool pmc = argc > 2 && !strcmp(argv[2], "pmc");
    const int only_shape = argc > 3 ? atoi(argv[3]) : -1;
    const Shape shapes[] = {{8, 120, 160, 64, 64}, {8, 60, 80, 128, 128}, {8, 60, 80, 128, 256}};
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    for (const Shape& s : shapes) {
        if (only_shape >= 0 && &s != &shapes[only_shape]) continue;
        const size_t px = (size_t)s.B * s.H * s.W, nx = px * s.C, no = px * s.O, nu = (size_t)36 * s.O * s.C;
        float *x, *u, *par, *res, *out;
        CHECK(hipMalloc(&x, nx * 4));
        CHECK(hipMalloc(&u, nu * 4));
        CHECK(hipMalloc(&par, 2 * s.O * 4));
        CHECK(hipMalloc(&res, no * 4));
        CHECK(hipMalloc(&out, no * 4));
        hipLaunchKernelGGL(fill_kernel, dim3(1024), dim3(256), 0, 0, x, nx, 1u);
        hipLaunchKernelGGL(fill_kernel, dim3(1024), dim3(256), 0, 0, u, nu, 2u);
        hipLaunchKernelGGL(fill_kernel, dim3(1), dim3(256), 0, 0, par, (size_t)2 * s.O, 3u);
        hipLaunchKernelGGL(fill_kernel, dim3(1024), dim3(256), 0, 0, res, no, 4u);
        CHECK(hipDeviceSynchronize());
        Args a;
        a.x = x; a.u = u; a.scale = par; a.shift = par + s.O; a.res = res; a.out = out; a.O = s.O;
        a.g.H = s.H; a.g.W = s.W; a.g.C = s.C; a.g.TH = (s.H + 3) / 4; a.g.TW = (s.W + 3) / 4; a.g.T = s.B * a.g.TH * a.g.TW; a.g.Tp = 0;
        a.xb = (unsigned)(nx * 4); a.ub = (unsigned)(nu * 4); a.ob = (unsigned)(no * 4);
        for (const Build& b : BUILDS) {
            if (only && strcmp(b.name, only)) continue;
            for (int form = 1; form <= 3; form += 2) {
                const Launch fn = form == 1 ? b.form1 : b.form3;
                const int rounds = pmc ? 1 : 5, reps = pmc ? 3 : 20;
                std::vector<float> us;
                for (int r = 0; r < rounds; ++r) {
                    for (int i = 0; i < 3; ++i) fn(a);
                    CHECK(hipEventRecord(e0, 0));
                    for (int i = 0; i < reps; ++i) fn(a);
                    CHECK(hipEventRecord(e1, 0));
                    CHECK(hipEventSynchronize(e1));
                    CHECK(hipGetLastError());
                    float ms = 0.f;
                    CHECK(hipEventElapsedTime(&ms, e0, e1));
                    us.push_back(1e3f * ms / reps);
                }
                std::sort(us.begin(), us.end());
                printf("%dx%dx%d %3d->%3d form %d %-13s median %7.1f  min %7.1f  max %7.1f us\n", s.B, s.H, s.W, s.C, s.O, form, b.name,
                       us[us.size() / 2], us.front(), us.back());
                fflush(stdout);
            }
        }
        CHECK(hipFree(x)); CHECK(hipFree(u)); CHECK(hipFree(par)); CHECK(hipFree(res)); CHECK(hipFree(out));
    }
    return 0;
}
