// ffb6d_amd/csrc/mlp_pm_split.hip -- the long-row fp32 shared-MLP GEMMs as six bf16 MFMA products of split operands (gfx950).
//
// Reference: the same 1x1 Conv + BatchNorm + activation wrappers as csrc/mlp_pm.hip (ffb6d/models/pytorch_utils.py:75-129):
//   out[r, m] = act( sum_k W[m, k] * X[r, k] + bias[m] + Y[yrow(r), m] ),   fp32 in, fp32 out.
//
// Arithmetic.  A finite fp32 number a is the sum of three bf16 numbers a0 = bf16(a), a1 = bf16(a - a0), a2 = bf16(a - a0 - a1)
// (round to nearest even; both subtractions are exact; exact while the lowest set bit of a is >= 2^-133, i.e. for every a with
// |a| >= 2^-110 -- below that the sum misses a by less than 2^-133).  W . X is then nine bf16 products; the six with i + j <= 2 carry
// everything above 2^-23 sum |w||x|: each part is within 2^-8 of what it rounds, the dropped terms are a1 b2 + a2 b1 + a2 b2
// <= (2^-24 + 2^-24 + 2^-32) |a||b|.  v_mfma_f32_32x32x16_bf16 runs at 16 x the rate of v_mfma_f32_32x32x2_f32, six of them per
// fragment pair and 16 k make a roof of 2.6 x the fp32 MFMA's.
//   Order (fixed: results repeat bit for bit): within a k16 step the small terms first, (w part, x part) =
//   (0,2), (1,1), (2,0), (0,1), (1,0), (0,0), then k ascending; one accumulator set.
//   FINITE INPUTS ONLY: +-inf in an operand gives NaN (inf - inf in the split); |x| above the largest finite bf16 (3.3895e38)
//   overflows when it is rounded.  split_form_ok() is the host check of everything else.
//
// Form.  Tile = 256 channels x 128 points (a batched launch's rows_per_w is a multiple of 128: a tile multiplies one matrix), 8 waves =
// 2 (channel halves) x 4 (point quarters), a wave owns 128 channels x 32 points = 4 MFMA tiles (64 accumulator registers); one
// workgroup per CU, two waves per SIMD.  A step = 32 k:
//   * W comes PRE-SPLIT (ffb6d_mlp_pm_split_w: three bf16 images [3][rows][K], made once per weight version) and enters LDS by
//     LDS-DMA (`buffer_load_dwordx4 ... lds`, as csrc/mlp_pm_big.hip): six 1 KB pieces per wave and step, 16 image rows of 64 bytes each;
//   * X stays fp32 in memory: every thread loads 8 k of one row (32 bytes), splits them in registers and writes one 16-byte chunk to
//     each of the three X images;
//   * image rows are 64 bytes (4 chunks of 16); LDS chunk c of row r holds the row's chunk c ^ ((r >> 3) & 3): the sixteen lanes a
//     ds_read_b128 serves per cycle (rows {0-3, 12-15, 20-27} / {4-11, 16-19, 28-31} of a 32-row fragment) then hit sixteen
//     different 16-byte bank groups (four rows fill a 256-byte bank row; r >> 3 differs between the four row quads of a group);
//   * a ring of two 72 KB slots, one barrier per step; W(s + 1) is requested piece by piece between the MFMAs of step s, X travels
//     one step further ahead in registers (loaded in step s - 1, split and written in step s, multiplied in step s + 1), and every
//     wait is counted: none waits for a request younger than the one it needs (the loop's comment has the sequence).
//     A ring of four 16-k slots, requested three half-steps ahead, was measured and dropped: its barrier per 24 MFMAs cost more
//     (3-10 % per launch) than its longer cover gained (profiles/split_ring_forms.jsonl; DESIGN.md 4a form 6 has what is and is not measured).
// XCD-aware order as the other long-row forms: all channel tiles of a point tile on one XCD.  Epilogue: pm_epilogue (fp32).
#include <algorithm>
#include <type_traits>

#include "common.h"
#include "ffb6d_ops.h"
#include "mlp_pm_common.h"

namespace ffb6d {
namespace pm {
namespace {

constexpr int SP_BLK = 512;
constexpr int SP_KS = 32;                             // k of a ring slot = of a loop iteration
constexpr int SP_RB = 2 * SP_KS;                      // bytes of an image row per slot (bf16)
constexpr int SP_WIMG = 256 * SP_RB;                  // one W part: 256 channels
constexpr int SP_XIMG = 128 * SP_RB;                  // one X part: 128 points
constexpr int SP_XBASE = 3 * SP_WIMG;
constexpr int SP_SLOT = 3 * SP_WIMG + 3 * SP_XIMG;
constexpr int SP_NS = 2;                              // slots of the ring
constexpr int SP_LDS = SP_NS * SP_SLOT;               // 144 KB
static_assert(SP_LDS <= 160 * 1024, "LDS layout");
constexpr int SP_NW = 6;                              // LDS-DMA instructions (1 KB each) per wave and slot: 3 parts x 2 halves
constexpr int SP_NV = 2;                              // 16-byte X loads per thread and slot
constexpr int SP_NOP = SP_NW + SP_NV;                 // vector-memory operations a wave issues per loop iteration

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// a = a0 + a1 + a2 (see the header): the k-th element of three 8-element chunks
__device__ __forceinline__ void split3(float a, __bf16& a0, __bf16& a1, __bf16& a2)
{
    a0 = (__bf16)a;
    const float r1 = a - (float)a0;
    a1 = (__bf16)r1;
    a2 = (__bf16)(r1 - (float)a1);
}

__global__ void __launch_bounds__(256) split_w_kernel(const float* __restrict__ w, __bf16* __restrict__ w3, long long n)
{
    for (long long e = blockIdx.x * 256LL + threadIdx.x; e < n; e += 256LL * gridDim.x) {
        __bf16 a0, a1, a2;
        split3(w[e], a0, a1, a2);
        w3[e] = a0;
        w3[n + e] = a1;
        w3[2 * n + e] = a2;
    }
}

// VAR (the library instantiates 0 only; timing probes with wrong results): bit 0 = no split (the X images get the raw upper halves),
// bit 1 = no MFMAs, bit 2 = no epilogue
template <int VAR>
__global__ void __launch_bounds__(SP_BLK)
mlp_pm_split_kernel(const PmParams p, const unsigned part_bytes)
{
    constexpr int OOB = 0x7ffffff0;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];      // [SP_NS slots][W0 | W1 | W2 | X0 | X1 | X2]

    const int t = blockIdx.x;
    const int xcd = t & 7, sl = t >> 3;
    const int pt = (sl / p.n_ct) * 8 + xcd;
    const int ct = sl % p.n_ct;
    if (pt >= p.n_pt) return;
    const int r0 = pt * 128, c0 = ct * 256;

    const int lane = threadIdx.x & 63;
    const int l31 = lane & 31, kh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const int K = p.k1;
    const int nslot = K / SP_KS;                      // at least SP_NS (launcher: K >= 64)
    const int wrow0 = p.rows_per_w ? (r0 / p.rows_per_w) * p.cout : 0;        // the tile's matrix: its first row in the images

    const unsigned char* w3 = static_cast<const unsigned char*>(p.w);
    const __amdgpu_buffer_rsrc_t rs_w[3] = {make_rsrc(w3, part_bytes), make_rsrc(w3 + part_bytes, part_bytes),
                                            make_rsrc(w3 + 2 * (size_t)part_bytes, part_bytes)};
    const __amdgpu_buffer_rsrc_t rs_x = make_rsrc(p.x1, span_bytes((unsigned)p.rows, p.ld1, p.k1, 4));

    // W loader: instruction (part, h) of wave w fills image rows 128 h + 16 w .. + 15; lane -> row + (lane >> 2), LDS chunk lane & 3,
    // which holds the row's chunk (lane & 3) ^ ((row >> 3) & 3)
    const int lrow = 16 * wave + (lane >> 2);
    const int lchunk = ((lane & 3) ^ ((lrow >> 3) & 3)) * 16;
    int w_off[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int ch = c0 + 128 * h + lrow;
        w_off[h] = ch < p.cout ? (wrow0 + ch) * (K * 2) + lchunk : OOB;
    }
    // slot j of the K range into ring slot rs; past the end of K (j >= nslot) the same number of operations is issued, all lanes out
    // of range (zeros land in a free ring slot): the counted waits below count operations, so every iteration must issue the same ones
    auto request_w = [&](int j, int rs, int q0 = 0, int q1 = SP_NW) {         // pieces q0 .. q1 - 1 of the wave's six
        const bool in = j < nslot;
        const int so = in ? j * SP_RB : 0;
        unsigned char* wi = lds + rs * SP_SLOT + wave * (16 * SP_RB);
#pragma unroll
        for (int pi = 0; pi < 3; ++pi)
#pragma unroll
            for (int h = 0; h < 2; ++h)
                if (pi * 2 + h >= q0 && pi * 2 + h < q1)
                    lds_dma16(rs_w[pi], wi + pi * SP_WIMG + h * (128 * SP_RB), in ? w_off[h] : OOB, so);
    };

    // X loader: thread -> point row tid >> 2, floats 8 (tid & 3) .. + 7 of the slot's 32 = chunk tid & 3 of the row's three images
    const int xrow = threadIdx.x >> 2, xq = threadIdx.x & 3;
    const bool xlive = r0 + xrow < p.rows;
    int x_off[SP_NV];
#pragma unroll
    for (int q = 0; q < SP_NV; ++q) x_off[q] = xlive ? (r0 + xrow) * p.ld1 * 4 + xq * 32 + 16 * q : OOB;
    const int x_dst = SP_XBASE + xrow * SP_RB + ((xq ^ ((xrow >> 3) & 3)) * 16);
    auto load_x = [&](int j, u32x4 (&v)[SP_NV]) {
        const bool in = j < nslot;
        const int so = in ? j * (SP_KS * 4) : 0;
#pragma unroll
        for (int q = 0; q < SP_NV; ++q) v[q] = __builtin_amdgcn_raw_buffer_load_b128(rs_x, in ? x_off[q] : OOB, so, 0);
    };
    // pair q (floats 2 q, 2 q + 1 of the thread's eight) of the three images' words
    auto split_pair = [&](const u32x4 (&v)[SP_NV], int q, unsigned (&o)[3][4]) {
        if constexpr (VAR & 1) {
            o[0][q] = (v[q >> 1][2 * (q & 1)] >> 16) | (v[q >> 1][2 * (q & 1) + 1] & 0xffff0000u);
            o[1][q] = 0u; o[2][q] = 0u;
        } else {
            bf16x2 b0, b1, b2;
            __bf16 s0, s1, s2;
            split3(__uint_as_float(v[q >> 1][2 * (q & 1)]), s0, s1, s2);
            b0[0] = s0; b1[0] = s1; b2[0] = s2;
            split3(__uint_as_float(v[q >> 1][2 * (q & 1) + 1]), s0, s1, s2);
            b0[1] = s0; b1[1] = s1; b2[1] = s2;
            o[0][q] = __builtin_bit_cast(unsigned, b0);
            o[1][q] = __builtin_bit_cast(unsigned, b1);
            o[2][q] = __builtin_bit_cast(unsigned, b2);
        }
    };
    auto store_x = [&](int rs, const unsigned (&o)[3][4]) {
        unsigned char* xi = lds + rs * SP_SLOT + x_dst;
#pragma unroll
        for (int pj = 0; pj < 3; ++pj) *reinterpret_cast<u32x4*>(xi + pj * SP_XIMG) = u32x4{o[pj][0], o[pj][1], o[pj][2], o[pj][3]};
    };
    auto write_x = [&](int rs, const u32x4 (&v)[SP_NV]) {
        unsigned o[3][4];
#pragma unroll
        for (int q = 0; q < 4; ++q) split_pair(v, q, o);
        store_x(rs, o);
    };

    // fragment reads: lane l31 of a 32-row MFMA tile reads chunk 2 ks + kh of its row = LDS chunk (2 ks + kh) ^ ((l31 >> 3) & 3)
    // (tile rows start at multiples of 32)
    const int fsw = (l31 >> 3) & 3;
    const int a_row = (wm * 128 + l31) * SP_RB, b_row = SP_XBASE + (wn * 32 + l31) * SP_RB;
    f32x16 acc[4][1];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][0][r] = 0.f;

    // reads q0 .. q1 - 1 of the 15 fragment reads of a k16 sub-step, in the order the terms first need them: group g = X part 2 - g,
    // then the four tiles of W part g (term g multiplies exactly these; terms 3-5 use them again)
    auto frags = [&](int rs, int ks, u32x4 (&a)[3][4], u32x4 (&b)[3], int q0 = 0, int q1 = 15) {
        const unsigned char* im = lds + rs * SP_SLOT;
        const int fo = ((2 * ks + kh) ^ fsw) * 16;
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            if (5 * g >= q0 && 5 * g < q1) b[2 - g] = *reinterpret_cast<const u32x4*>(im + b_row + (2 - g) * SP_XIMG + fo);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (5 * g + 1 + i >= q0 && 5 * g + 1 + i < q1)
                    a[g][i] = *reinterpret_cast<const u32x4*>(im + g * SP_WIMG + a_row + i * (32 * SP_RB) + fo);
        }
    };
    // terms t0 .. t1 - 1 of a k16 sub-step's six (24 MFMAs per wave): small terms first; the four tiles of a term are independent MFMAs
    auto mma = [&](const u32x4 (&a)[3][4], const u32x4 (&b)[3], int t0, int t1) {
        if constexpr (VAR & 2) {
            if (t0 == 0) {
#pragma unroll
                for (int pi = 0; pi < 3; ++pi)
#pragma unroll
                    for (int i = 0; i < 4; ++i) use_here(a[pi][i][0] ^ b[pi][3]);
            }
            return;
        }
        constexpr int TW[6] = {0, 1, 2, 0, 1, 0}, TX[6] = {2, 1, 0, 1, 0, 0};
#pragma unroll
        for (int tm = 0; tm < 6; ++tm) {
            if (tm < t0 || tm >= t1) continue;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a[TW[tm]][i]),
                                                                   __builtin_bit_cast(bf16x8, b[TX[tm]]), acc[i][0], 0, 0, 0);
        }
    };

    // The ring.  Step j (32 k) lives in ring slot j & 1.  At the top of iteration h: W(h) and X(h) are in LDS and published, the
    // registers xr hold (or wait for) X(h + 1).  Iteration h, per wave:
    //   15 ds_read_b128 of sub-step 0, in term order
    //   six times: 4 MFMAs of a term | one piece of W(h + 1) into the slot iteration h - 1 read (freed by its barrier) | 2-3 fragment
    //              reads of sub-step 1                                                                            6 vm operations
    //   the two loads of X(h + 2) into the registers X(h) left                                                    2 vm operations
    //   s_waitcnt vmcnt(8): X(h + 1), loaded one iteration ago -- the eight operations issued since stay in flight
    //   four times: 4 MFMAs of a term of sub-step 1 with the split of a pair of X(h + 1) between them; 4 MFMAs, the three ds_write_b128
    //              of X(h + 1) into slot (h + 1) & 1; 4 MFMAs
    //   s_waitcnt vmcnt(2) lgkmcnt(0): the wave's own pieces of W(h + 1) have landed (the loads of X(h + 2) are younger and stay in
    //              flight), its writes of X(h + 1) are done, its fragment reads of slot h returned before the MFMAs
    //   s_barrier: slot (h + 1) & 1 is published, slot h & 1 is free.
    // The main loop holds no other vector-memory wait (checked in the compiled loop: vmcnt(8) / vmcnt(2) only).  Past the end of K the
    // same operations are issued out of range (zeros, into a free slot): the waits count operations.  The half turn behind the loop
    // (K % 64 == 32) is the tile's last step: everything it requests is past the end of K, the compiler drops its dead X loads and
    // places smaller counts of its own for the register uses, and its vmcnt(2) may leave dead W pieces (zeros into the free slot) in
    // flight.  Nothing reads what it requests, and the vmcnt(0) behind it keeps those pieces from landing after the wave has ended.
    constexpr int WAIT_X = (SP_NS - 1) * SP_NOP, WAIT_W = SP_NV + (SP_NS - 2) * SP_NOP;
    u32x4 xr[SP_NS][SP_NV];
    // (the start-up issues in the loop's order, W(0) then X(1): the compiler's own count for a use of xr is the smallest over all
    // paths to it, and a start-up with fewer operations behind X(1) would shorten the loop's wait for X for good)
    load_x(0, xr[0]);
#pragma unroll
    for (int j = 0; j < SP_NS - 1; ++j) {
        __builtin_amdgcn_sched_barrier(0);
        request_w(j, j);
        __builtin_amdgcn_sched_barrier(0);
        load_x(j + 1, xr[j + 1]);
    }
    __builtin_amdgcn_sched_barrier(0);
    write_x(0, xr[0]);
    __builtin_amdgcn_sched_barrier(0);
    ring_wait<SP_NV>();                               // (the wave's pieces of W(0) have landed -- only the loads of X(1) are younger -- and its
    __builtin_amdgcn_s_barrier();                     // writes of X(0) are done: slot 0 is published)
    __builtin_amdgcn_sched_barrier(0);
    // (straight-line iterations, no branch inside: past the end of K the loads deliver zeros, which are written into a free ring slot)
    auto iteration = [&](int h, auto uc) {
        constexpr int u = decltype(uc)::value;
        u32x4 a[2][3][4], b[2][3];
        frags(u, 0, a[0], b[0], 0, 5);                // (in term order: the first MFMA waits for five reads, not fifteen)
        __builtin_amdgcn_sched_barrier(0);
        frags(u, 0, a[0], b[0], 5, 10);
        __builtin_amdgcn_sched_barrier(0);
        frags(u, 0, a[0], b[0], 10, 15);
        // the first sub-step's six terms; behind each, under its four MFMAs: one piece of W(h + SP_NS - 1) -- a piece costs the wave
        // ~100 issue cycles, which both waves of a SIMD would otherwise spend side by side behind the barrier with the MFMA unit idle
        // -- and a share of the second sub-step's fragment reads (one exposed LDS latency per iteration instead of two)
#pragma unroll
        for (int tm = 0; tm < 6; ++tm) {
            __builtin_amdgcn_sched_barrier(0);
            mma(a[0], b[0], tm, tm + 1);
            __builtin_amdgcn_sched_barrier(0);
            request_w(h + SP_NS - 1, (u + SP_NS - 1) % SP_NS, tm, tm + 1);
            frags(u, 1, a[1], b[1], tm < 3 ? 3 * tm : 9 + 2 * (tm - 3), tm < 3 ? 3 * tm + 3 : 11 + 2 * (tm - 3));
        }
        __builtin_amdgcn_sched_barrier(0);            // (the waits count operations in this order: W pieces, then X)
        load_x(h + SP_NS, xr[u]);
        __builtin_amdgcn_sched_barrier(0);
        // the second sub-step; the split of X(h + 1) rides in the vector-ALU slots between its MFMAs, a pair of floats per term
        // (~20 instructions under four MFMAs), the three stores after the fifth term
        lds_dma_wait<WAIT_X>();
        unsigned o[3][4];
#pragma unroll
        for (int tm = 0; tm < 6; ++tm) {
            __builtin_amdgcn_sched_barrier(0);
            mma(a[1], b[1], tm, tm + 1);
            if (tm < 4) {
                split_pair(xr[(u + 1) % SP_NS], tm, o);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);        // one MFMA ...
                    __builtin_amdgcn_sched_group_barrier(0x002, 5, 0);        // ... five vector-ALU instructions
                }
            }
            if (tm == 4) store_x((u + 1) % SP_NS, o);
        }
        __builtin_amdgcn_sched_barrier(0);
        ring_wait<WAIT_W>();
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
    };
    int h0 = 0;
    for (; h0 + SP_NS <= nslot; h0 += SP_NS) {
        iteration(h0, std::integral_constant<int, 0>());
        iteration(h0 + 1, std::integral_constant<int, 1>());
    }
    if (h0 < nslot) iteration(h0, std::integral_constant<int, 0>());          // K % 64 == 32: half a turn is left (workgroup-uniform)
    lds_dma_wait<0>();                               // (the requests past the end of K: nothing of this wave's may land in LDS after it ends)
    if constexpr (VAR & 4) {
        if (p.act != 77) return;
    }
    pm_epilogue<float, 4, 1, false>(p, acc, c0, r0, wm, wn, l31, kh);
}

template <int VAR>
bool launch_split(PmParams& p, unsigned part_bytes, hipStream_t st)
{
    static int attr_set[kMaxDevices + 1];
    const int slot = device_slot();
    if (!cache_get(attr_set, slot)) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&mlp_pm_split_kernel<VAR>), hipFuncAttributeMaxDynamicSharedMemorySize, SP_LDS) !=
            hipSuccess)
            return false;
        cache_set(attr_set, slot, 1);
    }
    p.n_ct = (int)ceil_div(p.cout, 256);
    p.n_pt = (int)ceil_div(p.rows, 128);
    const unsigned grid = (unsigned)(ceil_div(p.n_pt, 8) * 8 * p.n_ct);
    hipLaunchKernelGGL(mlp_pm_split_kernel<VAR>, dim3(grid), dim3(SP_BLK), SP_LDS, st, p, part_bytes);
    return true;
}

// can the split-bf16 form run this launch?  (w_rows = rows of the pre-split images: cout, or matrices x cout of a batched launch)
bool split_form_ok(const PmParams& p, int64_t w_rows, int64_t y_rows)
{
    const int64_t K = p.k1;
    return p.k2 == 0 && !p.x2 && !p.xidx && p.act >= 0 && p.act <= 2 && K % 32 == 0 && K >= 64 && (p.cout & 3) == 0 &&
           (p.ld1 & 3) == 0 && ((reinterpret_cast<uintptr_t>(p.x1) | reinterpret_cast<uintptr_t>(p.w)) & 15) == 0 &&
           ((int64_t)p.rows + 256) * p.ld1 * 4 < (1LL << 31) && ((int64_t)p.rows + 256) * p.ldo * 4 < (1LL << 31) &&
           (w_rows + 256) * K * 2 < (1LL << 31) && (!p.y || (y_rows + 256) * p.ldy * 4 < (1LL << 31));
}

}  // namespace
}  // namespace pm
}  // namespace ffb6d

using namespace ffb6d;
using namespace ffb6d::pm;

extern "C" int ffb6d_mlp_pm_split_w(const float* w, void* w3, int64_t n, ffb6d_stream_t stream)
{
    FFB6D_REQUIRE(n >= 0, "mlp_pm_split_w: bad size");
    if (n == 0) return FFB6D_OK;
    FFB6D_REQUIRE(w && w3, "mlp_pm_split_w: null pointer");
    const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(n, 256), 4096);
    hipLaunchKernelGGL(split_w_kernel, dim3(grid), dim3(256), 0, as_stream(stream), w, static_cast<__bf16*>(w3), (long long)n);
    FFB6D_LAUNCH_CHECK();
    return FFB6D_OK;
}

extern "C" int ffb6d_mlp_pm_split_f32(const void* w3, const float* bias, const float* x1, int64_t k1, int64_t ld1, const void* x1_idx,
                                      int64_t x1_rows_per_frame, const float* x2, int64_t k2, int64_t ld2, const float* y, int64_t ldy,
                                      const void* y_idx, int64_t y_rows_per_frame, int idx_bits, int64_t rows_per_frame, float* out,
                                      int64_t ldo, int64_t rows, int64_t cout, int act, int variant, ffb6d_stream_t stream)
{
    (void)x1_rows_per_frame; (void)ld2;
    FFB6D_REQUIRE(rows >= 0 && cout >= 1 && k1 >= 1 && k2 >= 0, "mlp_pm_split: bad shape");
#ifndef FFB6D_SPLIT_PROBES
    FFB6D_REQUIRE(variant == 0, "mlp_pm_split: the library carries variant 0 only");
#endif
    if (rows == 0) return FFB6D_OK;
    FFB6D_REQUIRE(w3 && x1 && out, "mlp_pm_split: null pointer");
    FFB6D_REQUIRE(ld1 >= k1 && ldo >= cout, "mlp_pm_split: row stride smaller than the row");
    FFB6D_REQUIRE(!y_idx || y, "mlp_pm_split: gather indices without rows to gather");
    FFB6D_REQUIRE(!y_idx || ((idx_bits == 32 || idx_bits == 64) && rows_per_frame >= 1 && rows % rows_per_frame == 0 && y_rows_per_frame >= 1),
                  "mlp_pm_split: index arrays need idx_bits 32/64 and rows_per_frame dividing rows");
    FFB6D_REQUIRE(!y || ldy >= cout, "mlp_pm_split: ldy smaller than cout");
    PmParams p;
    p.w = w3; p.bias = bias; p.x1 = x1; p.xidx = x1_idx; p.x2 = x2; p.y = y; p.gidx = y_idx; p.out = out;
    p.rows = (int)rows; p.cout = (int)cout; p.k1 = (int)k1; p.k2 = (int)k2; p.ld1 = (int)ld1; p.ld2 = 4;
    p.ldy = (int)ldy; p.ldo = (int)ldo; p.P = (int)(y_idx ? rows_per_frame : rows); p.py = (int)y_rows_per_frame; p.px = 0;
    p.act = act; p.idx64 = idx_bits == 64;
    const int64_t y_rows = y ? (y_idx ? rows / rows_per_frame * y_rows_per_frame : rows) : 0;
    FFB6D_REQUIRE(rows < (1LL << 31) && cout < (1LL << 31) && k1 < (1LL << 31) && ld1 < (1LL << 31) && ldo < (1LL << 31) && ldy < (1LL << 31) &&
                  split_form_ok(p, cout, y_rows),
                  "mlp_pm_split: the split-bf16 form needs one ungathered fp32 source with K %% 32 == 0, K >= 64, cout %% 4 == 0, "
                  "16-byte aligned operand rows, act 0..2 and buffers under 2 GiB");
    const unsigned part_bytes = (unsigned)(cout * k1 * 2);
    bool ok;
    switch (variant) {
#ifdef FFB6D_SPLIT_PROBES                             // (a probe build of this file: phase-removal variants, wrong results)
        case 1: ok = launch_split<1>(p, part_bytes, as_stream(stream)); break;
        case 2: ok = launch_split<2>(p, part_bytes, as_stream(stream)); break;
        case 4: ok = launch_split<4>(p, part_bytes, as_stream(stream)); break;
        case 6: ok = launch_split<6>(p, part_bytes, as_stream(stream)); break;
#endif
        default: ok = launch_split<0>(p, part_bytes, as_stream(stream)); break;
    }
    if (!ok)
        return set_error(FFB6D_ERR_HIP, "mlp_pm_split: hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
    FFB6D_LAUNCH_CHECK();
    return FFB6D_OK;
}

extern "C" int ffb6d_mlp_pm_split_batched_f32(const void* w3, int64_t n_w, int64_t rows_per_w, const float* x, int64_t k, int64_t ld,
                                              float* out, int64_t ldo, int64_t rows, int64_t cout, ffb6d_stream_t stream)
{
    FFB6D_REQUIRE(rows >= 0 && cout >= 1 && k >= 1 && n_w >= 1, "mlp_pm_split_batched: bad shape");
    FFB6D_REQUIRE(rows_per_w >= 128 && rows_per_w % 128 == 0 && rows_per_w < (1LL << 31),
                  "mlp_pm_split_batched: rows_per_w must be a positive multiple of 128 (got %lld): a point tile multiplies one matrix",
                  (long long)rows_per_w);
    if (rows == 0) return FFB6D_OK;
    FFB6D_REQUIRE(w3 && x && out, "mlp_pm_split_batched: null pointer");
    FFB6D_REQUIRE(ld >= k && ldo >= cout && ceil_div(rows, rows_per_w) <= n_w, "mlp_pm_split_batched: stride smaller than the row, or more "
                  "rows than matrices");
    PmParams p;
    p.w = w3; p.bias = nullptr; p.x1 = x; p.xidx = nullptr; p.x2 = nullptr; p.y = nullptr; p.gidx = nullptr; p.out = out;
    p.rows = (int)rows; p.cout = (int)cout; p.k1 = (int)k; p.k2 = 0; p.ld1 = (int)ld; p.ld2 = 4; p.ldy = 0; p.ldo = (int)ldo;
    p.P = (int)rows; p.py = 0; p.px = 0; p.act = 0; p.idx64 = 0;
    p.rows_per_w = (int)rows_per_w; p.w_stride = (int)(cout * k);
    FFB6D_REQUIRE(rows < (1LL << 31) && cout < (1LL << 31) && k < (1LL << 31) && ld < (1LL << 31) && ldo < (1LL << 31) &&
                  n_w * cout < (1LL << 31) && split_form_ok(p, n_w * cout, 0),
                  "mlp_pm_split_batched: needs K %% 32 == 0, K >= 64, cout %% 4 == 0, 16-byte aligned rows and buffers under 2 GiB");
    if (!launch_split<0>(p, (unsigned)(n_w * cout * k * 2), as_stream(stream)))
        return set_error(FFB6D_ERR_HIP, "mlp_pm_split_batched: hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
    FFB6D_LAUNCH_CHECK();
    return FFB6D_OK;
}
