// fa_fwd_w64.hpp -- forward kernel, "64 query rows per wave, one wave per SIMD" form (16-bit types, E = 64 / 128).
//
// What `_flash_attention_fwd!` computes (src/attention.jl:1-131), third program form next to fa_fwd.hpp (32 rows per
// wave, 2 waves per SIMD) and fa_fwd_split.hpp (32 rows per wave, 4 waves per SIMD).  The structure is the one the CDNA4
// guide measures fastest for attention on this part: a workgroup = 4 waves = 256 query rows, each wave owns 64 rows (two
// 32-row blocks z = 0, 1) and the WHOLE register file of its SIMD (512 registers per lane):
//
//   * O^T accumulators (2 x E/32 tiles = 128 registers at E = 128) and the Q fragments (64) live in the ACCUMULATOR
//     file; the arch VGPRs hold two score tiles (this kv tile's and the next one's), K / V fragments and the softmax
//     temporaries.  hipcc cannot be made to split the files that way with MFMA builtins (it moves score tiles through
//     AGPRs: ~440 v_accvgpr moves per kv tile, measured 1.3x slower -- DESIGN.md section 5), so every MFMA here is
//     inline asm with explicit register classes ("a" = accumulator file): the compiler only allocates.
//   * every K / V fragment read from LDS feeds TWO MFMAs (z = 0, 1): half the LDS bytes per FLOP of the 32-row forms.
//   * K / V tiles arrive by LDS-DMA (buffer_load_dwordx4 ... lds: 1 KiB per wave-instruction, no staging registers, no
//     ds_write; see "LDS-DMA" below): the LDS images are the same swizzled RowImg / blocked ColImg as everywhere else, the
//     swizzle is applied to each lane's SOURCE offset (the DMA destination is lane-linear); rings of 3 slots, loads issued
//     two tiles ahead right after the tile's barrier, retired by a wait before the next barrier (raw s_barrier: the DMA
//     stays in flight across everything else).
//   * one barrier per kv tile.  The loop body is software-pipelined across tiles and HAND-PLACED: it is a sequence of
//     "slots" -- the LDS fragment read three fragments ahead, one MFMA, and a share of the other tile's softmax VALU work
//     dealt out by issue COST (W64Plan below: QK^T of tile t+1 beside exp / sum / convert of tile t; PV of tile t beside the
//     rest of the softmax and the row max of tile t+1) -- each pinned by sched_barrier(0), because hipcc does not interleave
//     inline-asm MFMAs with VALU work on its own (it models an asm statement as a 1-cycle instruction).
//   * wait states the compiler would pad around a builtin MFMA are explicit (hipcc pads nothing around asm):
//     MFMA result -> VALU read (fence_mfma_result), VALU result -> MFMA operand (fence_valu_operand).
//
// Modes: 0 plain (KL % 64 == 0, every logit live) / 1 masked (causal, key padding, ragged KL); the pair-bias mode stays
// on fa_fwd.hpp.  Same numerics contract as the other forms (fp32 softmax, deferred row max with threshold 2^8, O
// normalised once in the epilogue, residuals ms / ls per src/attention.jl:128-129).
#pragma once
#include <utility>
#include "fa_fwd.hpp"

// timing-only ablations of the hand-placed loop (make DEV=1 VAR=-DNNOP_W64_ABL=mask; results WRONG by construction), a bit mask:
//   1 no LDS-DMA in the loop   2 no tile barrier   4 no softmax arithmetic   8 no row max   16 no LDS fragment reads
#if !defined(NNOP_DEV_BUILD)
#undef NNOP_W64_ABL
#endif
#ifndef NNOP_W64_ABL
#define NNOP_W64_ABL 0
#endif
// diagnostic (make DEV=1 VAR=-DNNOP_W64_STAMP=1; results WRONG by construction): wave 0 of every workgroup overwrites the
// start of its first output row with s_memtime / s_memrealtime stamps (kernel entry, loop entry, loop exit, end) --
// tools/w64_stamp.py turns them into cycles per kv tile and the in-kernel clock (MI355X_MICROARCH.md, "in-kernel clock")
#if !defined(NNOP_DEV_BUILD)
#undef NNOP_W64_STAMP
#endif
#ifndef NNOP_W64_STAMP
#define NNOP_W64_STAMP 0
#endif
// E = 64 and E = 128: scale * log2(e) folded into Q (rounded to T once) and the exponent reference -m2 loaded as the INITIAL
// accumulator of QK^T, so that a logit leaves the matrix pipe ready for v_exp_f32 (no v_fma per logit).  See the header.
#ifndef NNOP_W64_PRESCALE
#define NNOP_W64_PRESCALE 1
#endif
// row sums of P on the matrix pipe (ones x P^T, one MFMA per 16-key step and query block, accumulated in the accumulator
// file) instead of one v_add per logit: in this form the WAVE'S ISSUE is the bound, the matrix pipe has slack
#ifndef NNOP_W64_MFMASUM
#define NNOP_W64_MFMASUM 1
#endif
#ifndef NNOP_W64_SUM_MAXE
#define NNOP_W64_SUM_MAXE 64
#endif
#ifndef NNOP_W64_RF8
#define NNOP_W64_RF8 0
#endif
// o stored with the nontemporal hint (streamed past L2: less dirty data to write back when the kernel ends)
#ifndef NNOP_W64_NT
#define NNOP_W64_NT 0
#endif
// softmax: how many exp issues lie between an element's v_exp_f32 and its first consumer (row-sum add / convert)
#ifndef NNOP_W64_LAG
#define NNOP_W64_LAG 3
#endif
#ifndef NNOP_W64_PF64
#define NNOP_W64_PF64 3
#endif
#ifndef NNOP_W64_PF128
#define NNOP_W64_PF128 3
#endif

namespace nnop {

// compile-time loop: f(integral_constant<int, 0>) ... f(integral_constant<int, N-1>).  The hand-placed loop body must not
// depend on the unroller (its size estimate of a body full of `if (i == ...)` blocks exceeds the pragma threshold and the
// loop then stays rolled, with every register array indexed at run time).
template <int... I, typename F> NNOP_DEV void static_for_impl(std::integer_sequence<int, I...>, F&& f) {
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, typename F> NNOP_DEV void static_for(F&& f) { static_for_impl(std::make_integer_sequence<int, N>{}, f); }

// ---- inline-asm MFMAs with explicit register files ------------------------------------------------------------------
// volatile: an MFMA keeps its place among the other volatile statements of its slot (the pins of the softmax work) -- hipcc
// otherwise sinks it below the slot's VALU work, and the matrix pipe idles meanwhile.
template <typename T> struct MfmaAsm;
#define NNOP_MFMA_ASM(TYPE, FRAG, MNEMONIC)                                                                     \
    template <> struct MfmaAsm<TYPE> {                                                                          \
        /* D(vgpr) = A(vgpr) x B(acc file) */                                                                   \
        static NNOP_DEV f32x16 qk_first(FRAG a, FRAG bq) {                                                      \
            f32x16 d;                                                                                           \
            asm volatile(MNEMONIC " %0, %1, %2, 0" : "=&v"(d) : "v"(a), "a"(bq));                                        \
            return d;                                                                                           \
        }                                                                                                       \
        /* D(vgpr) = A(vgpr) x B(vgpr) */                                                                       \
        static NNOP_DEV f32x16 qk_first_v(FRAG a, FRAG b) {                                                     \
            f32x16 d;                                                                                           \
            asm volatile(MNEMONIC " %0, %1, %2, 0" : "=&v"(d) : "v"(a), "v"(b));                                         \
            return d;                                                                                           \
        }                                                                                                       \
        static NNOP_DEV void qk_acc_v(f32x16& d, FRAG a, FRAG b) {                                              \
            asm volatile(MNEMONIC " %0, %1, %2, %0" : "+v"(d) : "v"(a), "v"(b));                                         \
        }                                                                                                       \
        /* D(vgpr) = A(vgpr) x B(acc file) + C(vgpr), C kept */                                                 \
        static NNOP_DEV f32x16 qk_init(FRAG a, FRAG bq, const f32x16& c) {                                      \
            f32x16 d;                                                                                           \
            asm volatile(MNEMONIC " %0, %1, %2, %3" : "=&v"(d) : "v"(a), "a"(bq), "v"(c));                               \
            return d;                                                                                           \
        }                                                                                                       \
        static NNOP_DEV void qk_acc(f32x16& d, FRAG a, FRAG bq) {                                               \
            asm volatile(MNEMONIC " %0, %1, %2, %0" : "+v"(d) : "v"(a), "a"(bq));                                        \
        }                                                                                                       \
        /* O(acc file) += A(vgpr) x B(vgpr) */                                                                  \
        static NNOP_DEV void pv_acc(f32x16& o, FRAG a, FRAG b) {                                                \
            asm volatile(MNEMONIC " %0, %1, %2, %0" : "+a"(o) : "v"(a), "v"(b));                                         \
        }                                                                                                       \
    };
NNOP_MFMA_ASM(__bf16, bf16x8, "v_mfma_f32_32x32x16_bf16")
NNOP_MFMA_ASM(_Float16, f16x8, "v_mfma_f32_32x32x16_f16")
#undef NNOP_MFMA_ASM

// MFMA result -> first non-MFMA reader: the wait states hipcc does not insert after an asm MFMA.  The data dependence
// through the operands keeps every reader below the statement.  Not the table's 12 states: the last MFMA may itself have been
// issued behind another one that still occupied the matrix pipe, and its final pass (accumulator registers 12..15) then
// lands up to two MFMA times = 64 cycles after its issue -- measured: with `s_nop 15; s_nop 3` (20 cycles) the epilogue read
// stale registers 13..15 of the last-written O tile in ~0.1 % of the rows, differently from run to run; 64 cycles were clean.
// RULE: a fence idles 128 cycles = 2 x the longest distance that reasoning allows (and > 6 x the distance measured unsafe).
// All sites (prologue score tile, rescale, epilogue, leaving a copy of the loop body) run once per workgroup or rarer.  A run
// of reads behind ONE fence needs the idle time once: the first statement is the fence, the others only carry the data
// dependence (acc_after_fence) -- asm volatile statements keep their order.
#define NNOP_FENCE_128 "s_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15"
NNOP_DEV void fence_mfma_result(f32x16& a, f32x16& b, f32x16& c, f32x16& d) {
    asm volatile(NNOP_FENCE_128 : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
}
NNOP_DEV void fence_acc_result(f32x16& a) { asm volatile(NNOP_FENCE_128 : "+a"(a)); }
NNOP_DEV void acc_after_fence(f32x16& a) { asm volatile("" : "+a"(a)); }
// VALU-written registers -> MFMA A/B operand inside an asm statement: 2 wait states
template <typename F> NNOP_DEV void fence_valu_operand(F& a, F& b) { asm volatile("s_nop 1" : "+v"(a), "+v"(b)); }

// Q fragment: 16 bytes per lane straight from HBM into the accumulator file (an MFMA B operand may be an AGPR).  The
// load is invisible to hipcc's wait-count bookkeeping: the destination is valid only after the `s_waitcnt vmcnt(0)` of
// q_landed(), which takes the fragments as operands so that no consumer can be scheduled above it.
template <typename F> NNOP_DEV F load_q_frag(const void* gptr) {
    F d;
    asm volatile("global_load_dwordx4 %0, %1, off" : "=a"(d) : "v"(gptr) : "memory");
    return d;
}

// ---- LDS-DMA ---------------------------------------------------------------------------------------------------------
// K / V tiles go HBM -> LDS with buffer_load_dwordx4 ... lds: lane l of a wave copies 16 bytes from
//   base(V#) + soffset + voffset(lane) + imm      to LDS byte      M0 + imm + 16 l .
// A wave owns NJ CONSECUTIVE 1-KiB pieces of a tile image, so one M0 (the image's ring slot + the wave's share) and one scalar
// offset (the tile) serve all of them, the piece being selected by the immediate (which both addresses add): per tile and
// tensor 2 scalar instructions + NJ loads instead of 3 scalar instructions per piece -- on a wave whose ISSUE is the bound, a
// scalar instruction costs as much as a vector one (tools/ubench/gapcost.hip).  The image's swizzle is applied to the lane's
// SOURCE offset (the destination is lane-linear).  The descriptor's NUM_RECORDS is the byte size of the (batch, kv-head)
// tensor; on gfx950 the range check covers soffset + voffset + imm (measured: tools/ubench/probe_buf.hip,
// profiles/r02/probe_buf.log), so the rows of the last tile past KL are out of range and read as zeros -- finite data
// behind the mask -- with no per-lane clamping.
// M0 is written in the statement of a tensor's first piece and stays for its other pieces; nothing else in these kernels uses
// M0 (gfx950 DS instructions need no M0 setup; tools/audit_w64.py fails on any other M0 access).
NNOP_DEV u32x4 make_rsrc(const void* base, uint32_t bytes) {
    const uint64_t a = (uint64_t)(uintptr_t)base;
    u32x4 r;
    r[0] = __builtin_amdgcn_readfirstlane((uint32_t)a);
    r[1] = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32) & 0xffffu);       // stride 0: raw buffer
    r[2] = bytes;
    r[3] = 0x00020000u;                                                         // DATA_FORMAT = 32 (untyped dword access)
    return r;
}
template <int J, bool FIRST> NNOP_DEV void dma_piece(u32x4 rsrc, uint32_t voff, uint32_t soff, uint32_t lds_dst) {
    if constexpr (FIRST)
        asm volatile("s_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %2 offen offset:%4 lds"
                     :: "v"(voff), "s"(rsrc), "s"(soff), "s"(lds_dst), "n"(J * 1024) : "memory");
    else
        asm volatile("buffer_load_dwordx4 %0, %1, %2 offen offset:%3 lds" :: "v"(voff), "s"(rsrc), "s"(soff), "n"(J * 1024) : "memory");
}

// ---- the slot plan ------------------------------------------------------------------------------------------------
// One iteration of the loop is NX + NY2 "slots" (one MFMA each).  Besides its MFMA a slot carries fixed work (the LDS
// fragment read-ahead, an LDS-DMA piece, ...) and a share of two streams of movable work: the softmax steps of tile t
// (0 .. 63 + LAG: step n issues the exp of element n and finishes element n - LAG -- row-sum add, and the 16-bit convert of
// the pair it closes) and the row-max items of tile t + 1.  A wave issues in order: a slot lasts max(32, 8 + issue cost of its
// fillers) cycles (v_exp_f32 8, other VALU / DS / scalar 4, an LDS-DMA piece ~24 with its M0 setup: MI355X_MICROARCH.md,
// tools/w64_gaps.py), so the streams are dealt out by COST: the smallest per-slot budget `cap` for which a greedy in-order
// fill places everything inside its window -- a softmax step no later than the slot before the first MFMA that reads the P^T
// word it completes; a row-max item no earlier than two slots behind the last MFMA that writes the logits it reads.
// NJ2: LDS-DMA pieces per wave and iteration (both tensors); EV: columns of V / O the workgroup handles (E, or E / 2 at E = 256)
template <int E, bool SUM, bool MASKED, int NJ2, int LAG, int EV = E> struct W64Plan {
    static constexpr int KS = E / 16, EB = EV / 32, NKF = 2 * KS;
    static constexpr int NX = 2 * NKF, G = 2 * EB + (SUM ? 2 : 0), NY2 = 4 * G, NSLOT = NX + NY2, NYB = NY2 / 2;
    static constexpr int NSTEP = 64 + LAG, NMX = 34;
    static constexpr int DSTRIDE = NYB + 2 * NJ2 <= NY2 ? 2 : 1;       // a DMA piece every second slot behind the barrier where that fits
    static_assert(NYB + DSTRIDE * (NJ2 - 1) + 2 <= NY2, "the DMA batch fits behind the barrier");
    static constexpr bool dma_at(int i) { return i > NYB && (i - NYB - 1) % DSTRIDE == 0 && (i - NYB - 1) / DSTRIDE < NJ2; }   // i: phase-Y slot
    static constexpr int dma_index(int i) { return (i - NYB - 1) / DSTRIDE; }
    static constexpr int MASK_SLOT = NX + 2;            // masked mode: tile t+1 is masked here, its row max starts behind it
    static constexpr int ADDR_SLOT = NX + 1;            // scalar address arithmetic of the iteration's DMA batch
    int sm_end[NSLOT] = {};                             // softmax steps [sm_end[s-1], sm_end[s]) run in slot s
    int mx_end[NSLOT] = {};
    int cost[NSLOT] = {};                               // modelled filler cost per slot (reporting)
    int cap = 0;

    // fixed work in front of the MFMA of slot s (s = NSLOT: slot 0 of the next iteration, behind the loop's back edge)
    static constexpr int pre_cost(int s) {
        if (s >= NSLOT) return 8 + 12 + 28;             // read-ahead + image bases + ring rotation, loop control, rescale branch
        if (s < NX) return (s & 1) == 0 ? 8 : 0;        // K fragment read-ahead: v_xor + ds_read_b128
        const int i = s - NX, w = i % G, wp = w - (SUM ? 2 : 0);
        const bool is_sum = SUM && w < 2;
        int c = 0;
        if (!is_sum && (wp & 1) == 0) c += 8;           // V fragment (two transposed reads) or a K(t+2) fragment
        if (dma_at(i)) c += 24;                         // LDS-DMA piece
        return c;
    }
    // fixed work between the MFMA of slot s and the next one (the movable streams share this gap)
    static constexpr int fixed_cost(int s) {
        int c = pre_cost(s + 1);
        if (s == ADDR_SLOT) c += 40;
        if (MASKED && s == MASK_SLOT) c += 16;
        if (s == NSLOT - 1) c += 24;                    // rescale test of tile t+1
        return c;
    }
    static constexpr int step_cost(int n) {
        int c = n < 64 ? 8 : 0;
        const int m = n - LAG;
        if (m >= 0) c += (SUM ? 0 : 4) + ((m & 1) ? 4 : 0);
        return c;
    }
    // last slot that may hold step n: the one before the first MFMA reading the P^T word that element n - LAG belongs to
    static constexpr int step_deadline(int n) {
        const int m = n < LAG ? 0 : n - LAG, c = m >> 3, kk = c >> 1, z = c & 1;
        return NX + kk * G + z - 1;
    }
    static constexpr int mx_cost(int u) { return u < 32 ? 4 : 28; }
    static constexpr int mx_earliest(int u) {
        // (masked mode: the same -- a tile that turns out to need its mask redoes the items that ran before the mask slot)
        const int q = u >> 1;
        return q < 8 ? NX / 2 + 2 : NX + 2;             // logits of key block 0 are complete half way through phase X
    }
    static constexpr int kMxDeadline = NSLOT - 2;       // the rescale test of the last slot reads the finished row max

    constexpr bool fill(int budget) {
        // row-max items as LATE as their deadline allows (the tail of phase Y has nothing else to do: every P^T word is due
        // before the last 16-key step), softmax steps as EARLY as the budget allows
        int u = NMX;
        for (int sl = NSLOT - 1; sl >= 0; --sl) {
            int used = fixed_cost(sl);
            mx_end[sl] = u;
            if (sl <= kMxDeadline)
                while (u > 0 && mx_earliest(u - 1) <= sl && used + mx_cost(u - 1) <= budget) used += mx_cost(--u);
            cost[sl] = used;
        }
        if (u > 0) return false;
        int n = 0, over = 0;                            // over: worst overfill caused by a deadline-forced placement
        for (int sl = 0; sl < NSLOT; ++sl) {
            int used = cost[sl];
            while (n < NSTEP && (used + step_cost(n) <= budget || step_deadline(n) <= sl)) {
                used += step_cost(n++);
                if (used > budget && used - budget > over) over = used - budget;
            }
            sm_end[sl] = n;
            cost[sl] = used;
        }
        cap = budget;
        return n == NSTEP && over <= 4;
    }
    static constexpr W64Plan make() {
        W64Plan pl{};
        for (int b = 12; b <= 96; b += 2)
            if (pl.fill(b)) break;
        return pl;
    }
};

template <typename T, int E, int EV = E> constexpr int fa_fwd_w64_lds_bytes(bool masked) {
    return 3 * (RowImg<T, E>::bytes(64) + ColImg<T, EV>::bytes(64)) + (masked ? 16 + 8 * kMaxMaskTiles : 0);
}

// EV: the columns of V / O this workgroup handles.  EV = E except at E = 256, where the O^T accumulators of 64 rows x 256 columns would
// be the whole accumulator file: the grid then holds every block twice, each copy contracting Q K^T over all of E (Q fragments: 128
// registers) but accumulating one 128-column half of O (+33 % MFMA work for a spill-free kernel; the 32-row form spills 62-152).
// SINK: learned attention sinks (fa_fwd.hpp), merged in the epilogue
#include "fa_fwd_w64_kernel.inc"

}  // namespace nnop
