// moe_mx_decode_ring.hpp -- one pass of a wave of the weight-streaming MXFP4 forwards: the ring of loads, the selection at the consumer,
// the MFMAs.  moe_mx_decode.hip (libnnop_hip_moe_mx_decode.so) and moe_mx_decode_glu.hip (libnnop_hip_moe_mx_decode_glu.so) both compile
// it: header-only code in an unnamed namespace, as mx_convert8 of moe_mx.hpp is; nothing is linked between the two libraries.
//
// A wave owns kNT = 4 MFMA row tiles of 16 weight rows.  A reduction step is 128 values of k = 4 blocks of 32: lane (r = lane % 16,
// q = lane / 16) loads, per row tile, the 16 bytes of block 4 step + q of weight row r and that block's scale byte; mx_convert8 turns word
// i of the block into k = 32 q + 8 i ... 8 i + 7 of the step, which is the row operand of the i-th v_mfma_f32_16x16x32 of the step as it
// stands.  The k order inside an MFMA is free where both operands agree, so the x operand of lane (m = lane % 16, q) is the matching 64
// contiguous bytes of row m: four 16-byte loads.  acc[tile][g] ends as 4 consecutive weight rows (4 q ... 4 q + 3 of the tile) of row m.
//
// The ring: kDepth steps of loads (kDepth kNT = 8 weight blocks of 16 bytes, their scale bytes, the x pieces) are in flight per wave; the
// loop consumes slot d and refills it with step + kDepth.  Every load is unconditional, from an address clamped to a row and block that
// exist, and what does not exist is replaced at the consumer: word 0 with scale byte 127 (+0) for a weight row at or beyond its tile's end
// or a block >= K / 32, zeros for an x row the caller marks as absent or a block beyond K.  So the compiler sees straight-line loads
// consumed in issue order and waits with counted vmcnt, and masking is by selection: no byte of another expert, of a row the caller did
// not name or of padding enters a product.
//
// What the two kernels choose: the weight row at which each of the four tiles starts and ends (`base`, `end`: a tile's rows are
// base[i] ... base[i] + 15, those >= end[i] do not exist), the x row of each lane and group (`xr`, `xok`), and what happens to the
// accumulators (`epi`).  The sum of one output element runs over the steps in ascending order and over i = 0 ... 3 inside a step, into one
// fp32 accumulator: a function of K and the type alone, whatever the caller chose.
#pragma once
#include "moe_mx.hpp"
#include "moe_gemm_tile.hpp"

namespace nnop {
namespace {

constexpr int kNT = 4;                       // MFMA row tiles (16 weight rows each) per wave
constexpr int kStepBlocks = 4;               // a reduction step: 4 blocks of 32, one per k group of the MFMA
// The ring depth in steps.  kDepth kNT = 8 weight loads of 16 bytes are in flight per lane, 8 KiB per wave; at the 2 waves per SIMD the
// registers allow (profiles/r06/kernel_resources.txt) that is 64 KiB per CU, near the 72 KiB that hide most of an HBM miss (about 900
// cycles) on this chip.  A third step costs about 54 VGPRs; it and a third wave per SIMD (96 KiB either way) were timed and changed
// nothing: the depth is not what bounds this kernel.
constexpr int kDepth = 2;
// Accumulator groups (16 rows each) of one pass.  The count is chosen per expert on the device, inside one kernel, so the registers of
// the largest count are every expert's: 4 groups would take the kernel to one wave per SIMD.
constexpr int kMaxGroups = 2;

// the packed weights of one call: N weight rows per expert, K values per row
struct RingWeights {
    const uint8_t* blocks;
    const uint8_t* scales;
    long long ld_q, ld_s;  // bytes
    int K, N;
};

// One pass of a wave: the x rows xr[g] (lane % 16 picks the row of group g; xok[g] false: a row of zeros) against the weight rows of
// expert e that base / end name, all of K; epi(acc) receives acc[i][g][j], the sum of x row (g, lane % 16) with weight row
// base[i] + 4 (lane / 16) + j.
template <typename T, bool XA, int G, typename Epi>
__device__ __forceinline__ void decode_ring(const RingWeights& p, int e, const int (&base)[kNT], const int (&end)[kNT], const T* const (&xr)[G],
                                            const bool (&xok)[G], int lane, Epi&& epi) {
    typedef T tvec __attribute__((ext_vector_type(8)));
    const int fr = lane & 15, fq = lane >> 4;
    const int nb = p.K / kMxBlock;

    // the lane's weight row of each tile, clamped to one that exists
    const uint8_t* wq[kNT];
    const uint8_t* ws[kNT];
    bool wok[kNT];
#pragma unroll
    for (int i = 0; i < kNT; ++i) {
        const int n = base[i] + fr;
        wok[i] = n < end[i];
        const long long row = (long long)e * p.N + (wok[i] ? n : end[i] - 1);
        wq[i] = p.blocks + row * p.ld_q;
        ws[i] = p.scales + row * p.ld_s;
    }

    struct Slot {
        uint4 w[kNT];
        uint32_t e[kNT];
        tvec x[G][4];
    };
    Slot ring[kDepth];
    f32x4 acc[kNT][G];
#pragma unroll
    for (int i = 0; i < kNT; ++i)
#pragma unroll
        for (int g = 0; g < G; ++g) acc[i][g] = f32x4{0.f, 0.f, 0.f, 0.f};

    // loads only: nothing here waits for what it fetched
    auto load = [&](Slot& s, int step) {
        const int b = min(kStepBlocks * step + fq, nb - 1);
#pragma unroll
        for (int i = 0; i < kNT; ++i) {
            s.w[i] = *reinterpret_cast<const uint4*>(wq[i] + 16 * b);
            s.e[i] = ws[i][b];
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const T* src = xr[g] + kMxBlock * b;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (XA) {
                    s.x[g][i] = *reinterpret_cast<const tvec*>(src + 8 * i);
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) s.x[g][i][j] = src[8 * i + j];
                }
            }
        }
    };
    // selection, conversion, MFMAs: word i of a block beside piece i of the x rows
    auto consume = [&](const Slot& s, int step) {
        const bool bok = kStepBlocks * step + fq < nb;
        tvec zero;
#pragma unroll
        for (int j = 0; j < 8; ++j) zero[j] = (T)0.f;
        tvec xv[G][4];
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int i = 0; i < 4; ++i) xv[g][i] = xok[g] && bok ? s.x[g][i] : zero;
#pragma unroll
        for (int i = 0; i < kNT; ++i) {
            const bool ok = wok[i] && bok;
            const uint32_t sc = ok ? s.e[i] : 127u;
            const uint32_t words[4] = {ok ? s.w[i].x : 0u, ok ? s.w[i].y : 0u, ok ? s.w[i].z : 0u, ok ? s.w[i].w : 0u};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const tvec a = mx_convert8<T>(words[j], sc);
#pragma unroll
                for (int g = 0; g < G; ++g) acc[i][g] = Mma<T>::run(a, xv[g][j], acc[i][g]);  // rows of the result: n, columns: m
            }
        }
    };

    const int steps = (nb + kStepBlocks - 1) / kStepBlocks;
#pragma unroll
    for (int d = 0; d < kDepth; ++d) load(ring[d], d);
    // A step beyond the last one adds +0 to every accumulator; how many there are depends on K alone.  pin() keeps the loads of a slot
    // between the work on two slots (the empty statement for the optimiser, the scheduling barrier for the instruction scheduler): left
    // alone, the compiler gathers the loads of an iteration, waits for all of them and computes, and the ring is gone.
    auto pin = [] {
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
    };
    for (int s0 = 0; s0 < steps; s0 += kDepth) {
#pragma unroll
        for (int d = 0; d < kDepth; ++d) {
            pin();
            consume(ring[d], s0 + d);
            pin();
            load(ring[d], s0 + d + kDepth);
        }
    }
    epi(acc);
}

}  // namespace
}  // namespace nnop
