// scripts/icp_instances_sanitize.cpp -- stand-alone host program: the instance calls of include/ffb6d_refine.h, built from csrc/icp.hip
// for the HOST against the SIMT emulator (tests/simt), on a tiny ragged case in both modes and all forms of the search.  Meant to be
// compiled with -fsanitize=address,undefined (scripts/icp_instances_sanitize.py builds and runs it); it checks return codes and a
// few invariants, the sanitizers check every access of the kernels and of the host code around them.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "ffb6d_refine.h"

extern "C" const char* ffb6d_last_error();

namespace {

uint32_t g_state = 12345u;
float rnd() {                                   // [0, 1)
    g_state = g_state * 1664525u + 1013904223u;
    return static_cast<float>(g_state >> 8) / 16777216.0f;
}

#define CHECK(cond)                                                                         \
    do {                                                                                    \
        if (!(cond)) {                                                                      \
            std::fprintf(stderr, "%s:%d: %s failed: %s\n", __FILE__, __LINE__, #cond, ffb6d_last_error()); \
            std::exit(1);                                                                   \
        }                                                                                   \
    } while (0)

struct Problem { int frame, cls, inst; };

}  // namespace

int main() {
    const int B = 2, N = 192, n_cls = 5;
    const int sizes[n_cls] = {0, 130, 70, 0, 1100};
    std::vector<int64_t> begin(n_cls + 1, 0);
    for (int c = 0; c < n_cls; ++c) begin[c + 1] = begin[c] + sizes[c];
    const int64_t total = begin[n_cls];
    std::vector<float> model(static_cast<size_t>(total) * 3);
    for (auto& v : model) v = 0.12f * rnd() - 0.06f;
    const size_t pbytes = ffb6d_icp_prepared_bytes(total, n_cls);
    std::vector<unsigned char> prepared(pbytes);
    CHECK(ffb6d_icp_prepare(model.data(), begin.data(), n_cls, total, prepared.data(), pbytes, nullptr) == 0);

    // instances: (frame, class, id, points of its own, points of instance 0, offset along x)
    struct Placed { int frame, cls, id, n, n_free; float dx; };
    const Placed placed[] = {{0, 1, 1, 64, 4, 0.0f}, {0, 1, 2, 65, 3, 0.13f}, {0, 1, 3, 7, 3, -0.13f}, {0, 1, 255, 5, 0, 0.26f},
                             {1, 4, 1, 30, 3, 0.0f}, {1, 4, 2, 25, 3, 0.14f}, {1, 2, 1, 40, 5, 0.3f}, {1, 3, 1, 8, 2, -0.3f}};
    std::vector<float> pcld(static_cast<size_t>(B) * N * 3);
    for (auto& v : pcld) v = 2.0f * rnd() - 1.0f;
    std::vector<int64_t> mask64(static_cast<size_t>(B) * N, 0);
    std::vector<unsigned char> inst(static_cast<size_t>(B) * N, 0), keep(static_cast<size_t>(B) * N);
    int next[B] = {0, 0};
    for (const Placed& pl : placed) {
        for (int k = 0; k < pl.n + pl.n_free; ++k) {
            const int i = next[pl.frame]++;
            CHECK(i < N);
            const size_t at = static_cast<size_t>(pl.frame) * N + i;
            float pt[3] = {0.05f * rnd(), 0.05f * rnd(), 0.05f * rnd()};
            if (sizes[pl.cls] > 0) {
                const int64_t m = begin[pl.cls] + static_cast<int64_t>(rnd() * sizes[pl.cls]);
                for (int d = 0; d < 3; ++d) pt[d] = model[m * 3 + d] + 0.002f * (rnd() - 0.5f);
            }
            pcld[at * 3 + 0] = pt[0] + pl.dx;
            pcld[at * 3 + 1] = pt[1];
            pcld[at * 3 + 2] = pt[2] + 0.8f;
            mask64[at] = pl.cls;
            inst[at] = k < pl.n ? static_cast<unsigned char>(pl.id) : 0;
        }
    }
    for (int k = 0; k < 3; ++k) pcld[k * 3 + 1] = std::numeric_limits<float>::quiet_NaN();      // NaN points of instance 1
    for (auto& v : keep) v = rnd() < 0.8f;
    std::vector<int32_t> mask32(mask64.begin(), mask64.end());

    const Problem problems[] = {{0, 1, 1}, {0, 1, 2}, {0, 1, 3}, {1, 4, 1}, {1, 4, 2}, {1, 2, 1}, {0, 1, 2}, {0, 1, 9}, {0, 1, 255},
                                {1, 4, 0}, {1, 4, 256}, {7, 1, 1}, {1, 3, 1}};
    const float dxs[] = {0.0f, 0.13f, -0.13f, 0.0f, 0.14f, 0.3f, 0.131f, 0.002f, 0.26f, 0.001f, 0.141f, 0.0f, -0.3f};
    const int P = static_cast<int>(sizeof(problems) / sizeof(problems[0]));
    std::vector<int> frame_of(P), class_of(P), inst_of(P);
    std::vector<double> T0(static_cast<size_t>(P) * 12, 0.0);
    for (int p = 0; p < P; ++p) {
        frame_of[p] = problems[p].frame;
        class_of[p] = problems[p].cls;
        inst_of[p] = problems[p].inst;
        double* T = &T0[static_cast<size_t>(p) * 12];
        const double a = 0.02 * (p + 1);        // a small rotation about z, a few millimetres off in translation
        T[0] = std::cos(a); T[1] = -std::sin(a); T[4] = std::sin(a); T[5] = std::cos(a); T[10] = 1.0;
        T[3] = dxs[p] + 0.003; T[7] = -0.002; T[11] = 0.8 + 0.001;
    }

    CHECK(ffb6d_icp_inst_workspace_bytes(P, N, 2) == 0);
    int runs = 0;
    for (int mode = 0; mode <= 1; ++mode) {
        const size_t wbytes = ffb6d_icp_inst_workspace_bytes(P, N, mode);
        CHECK(wbytes > ffb6d_icp_workspace_bytes(P, N));
        std::vector<unsigned char> ws(wbytes);                                   // exactly the bytes asked for: an overrun is reported
        for (int form = -1; form <= 1; ++form) {
            ffb6d_icp_set_form(form);
            for (int bits = 32; bits <= 64; bits += 32) {
                const void* mask = bits == 64 ? static_cast<const void*>(mask64.data()) : static_cast<const void*>(mask32.data());
                for (int with_keep = 0; with_keep <= 1; ++with_keep) {
                    const unsigned char* kp = with_keep ? keep.data() : nullptr;
                    const unsigned char* im = (mode == 1 && with_keep) ? nullptr : inst.data();      // nearest mode: also without a map
                    std::vector<int> idx(static_cast<size_t>(P) * N), counts(P), owner(static_cast<size_t>(P) * N);
                    std::vector<float> d2(static_cast<size_t>(P) * N);
                    for (float max_dist : {std::numeric_limits<float>::infinity(), 0.006f}) {
                        CHECK(ffb6d_icp_correspond_inst_f32(prepared.data(), n_cls, total, pcld.data(), mask, bits, kp, im, frame_of.data(),
                                                            class_of.data(), inst_of.data(), T0.data(), P, B, N, N, max_dist, mode, idx.data(),
                                                            d2.data(), counts.data(), owner.data(), ws.data(), wbytes, nullptr) == 0);
                        for (int p = 0; p < P; ++p)
                            for (int j = 0; j < N; ++j) {
                                const size_t at = static_cast<size_t>(p) * N + j;
                                CHECK(idx[at] >= -1 && idx[at] < 1100 && owner[at] >= -1 && owner[at] < P);
                                CHECK(j < counts[p] || (idx[at] == -1 && owner[at] == -1));
                                CHECK(idx[at] < 0 || owner[at] == p);
                            }
                        CHECK(counts[11] == 0 && (mode == 1 || (counts[7] == 0 && counts[9] == 0 && counts[10] == 0)));
                    }
                    for (double tol : {0.0, 3e-4}) {
                        std::vector<double> T(static_cast<size_t>(P) * 12);
                        std::vector<int> n_pairs(P), iters(P);
                        std::vector<float> rms(P);
                        std::vector<unsigned char> out(static_cast<size_t>(B) * N, 7);
                        CHECK(ffb6d_icp_refine_inst_f32(prepared.data(), n_cls, total, pcld.data(), mask, bits, kp, im, frame_of.data(),
                                                        class_of.data(), inst_of.data(), T0.data(), P, B, N, N, 0.012f, 6, tol, 3, mode, T.data(),
                                                        n_pairs.data(), rms.data(), iters.data(), out.data(), ws.data(), wbytes, nullptr) == 0);
                        CHECK(iters[11] == 0 && iters[12] == 0 && n_pairs[11] == 0 && n_pairs[12] == 0);
                        for (int k = 0; k < 12; ++k) CHECK(T[11 * 12 + k] == T0[11 * 12 + k] && T[12 * 12 + k] == T0[12 * 12 + k]);
                        CHECK(iters[1] >= 1 && n_pairs[1] >= 3);
                        for (size_t i = 0; i < out.size(); ++i) CHECK(out[i] != 7 && (out[i] == 0 || mask64[i] == 1 || mask64[i] == 2 || mask64[i] == 4));
                        ++runs;
                    }
                    // outputs are optional
                    CHECK(ffb6d_icp_refine_inst_f32(prepared.data(), n_cls, total, pcld.data(), mask, bits, kp, im, frame_of.data(), class_of.data(),
                                                    inst_of.data(), T0.data(), P, B, N, N, 0.012f, 2, 0.0, 3, mode, nullptr, nullptr, nullptr,
                                                    nullptr, nullptr, ws.data(), wbytes, nullptr) == 0);
                    CHECK(ffb6d_icp_correspond_inst_f32(prepared.data(), n_cls, total, pcld.data(), mask, bits, kp, im, frame_of.data(),
                                                        class_of.data(), inst_of.data(), T0.data(), P, B, N, N, 0.01f, mode, nullptr, nullptr,
                                                        counts.data(), owner.data(), ws.data(), wbytes, nullptr) == 0);
                }
            }
        }
        // refusals: nothing is launched
        CHECK(ffb6d_icp_refine_inst_f32(prepared.data(), n_cls, total, pcld.data(), mask64.data(), 64, nullptr, inst.data(), frame_of.data(),
                                        class_of.data(), inst_of.data(), T0.data(), P, B, N, N, 0.012f, 2, 0.0, 3, mode, nullptr, nullptr, nullptr,
                                        nullptr, nullptr, ws.data(), wbytes - 1, nullptr) == FFB6D_ERR_WORKSPACE);
    }
    CHECK(ffb6d_icp_refine_inst_f32(prepared.data(), n_cls, total, pcld.data(), mask64.data(), 64, nullptr, nullptr, frame_of.data(), class_of.data(),
                                    inst_of.data(), T0.data(), P, B, N, N, 0.012f, 2, 0.0, 3, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                                    nullptr) == FFB6D_ERR_ARG);
    ffb6d_icp_set_form(0);
    std::printf("icp_instances_sanitize: %d loops in 2 modes x 3 forms x 2 mask widths x keep on/off: ok\n", runs);
    return 0;
}
