// fa_fwd_duo.hpp -- forward kernel, "two waves per SIMD in alternating phases" form (16-bit types; E = 64 with 64- or 32-row waves,
// E = 128 with 32-row waves, E = 32 with 64-row waves).  The text below describes the E = 64, 64-row form; the variants are at its end.
//
// What `_flash_attention_fwd!` computes (src/attention.jl:1-131; its hot loop :49-121), fourth program form.  Why it exists: at
// E = 64 one 32x32x16 MFMA covers only two score elements per lane, and each element costs one v_exp_f32 (8 cycles of the SIMD's
// vector port) plus ~3 plain VALU instructions (4 each for a single wave) -- a wave that owns its SIMD alone (fa_fwd_w64.hpp)
// issues 2067 cycles of instructions per 64 x 64 tile against 1280 cycles of matrix-pipe work, i.e. the WAVE, not the pipe, is the
// bound.  Two waves on a SIMD issue into the vector port independently, and one wave's VALU work runs beside the other's MFMAs
// (tools/ubench/pingpong.hip, profiles/r04/pingpong.log: the same instruction mix runs 2461 cycles per tile serially in one wave,
// 1482 as two waves in opposite phases).
//
//   * workgroup = 8 waves = 256 query rows of one (batch, q-head).  Waves w and w + 4 (SIMD partners: a workgroup's waves go to the
//     SIMDs cyclically) own the SAME 64 query rows and split the KEYS: group 0 (waves 0-3) takes the even kv tiles, group 1 the odd
//     ones, each with its own online-softmax state (reference, sum, O); the two partial results are merged once, through LDS, in
//     the epilogue (each partner finishes and stores 32 of the 64 rows).  64 rows per wave keep what the one-wave form has: every K /
//     V fragment read from LDS feeds two MFMAs (z = 0, 1).
//   * a wave alternates a MATRIX phase M(t) -- row sums of P(t-2) (8 MFMAs 16x16x32 with a selector operand, see below), O +=
//     V(t-2)^T P(t-2)^T (16 MFMAs), S(t) = K(t) Q^T (16), fragment reads three ahead, and at its END the LDS-DMA batch K(t+4), V(t+2) --
//     and a VECTOR phase V(t): [rare: mask] row max, test, [rare: raise the reference] P = exp2(s c - m), packed in place.  The matrix
//     phase holds NOTHING but MFMAs and fragment reads: a VALU or LDS-DMA instruction between them stalls the in-order wave while its
//     partner's vector phase holds the port, and the pipe idles (measured both ways: DESIGN.md section 4.1d, profiles/r04/
//     duo_ablations.log).  Group 1 runs a phase behind group 0, so each SIMD always holds one wave in M and one in V; ONE s_barrier per
//     iteration (group 0 behind V, group 1 behind M).  Nothing is software-pipelined INSIDE a wave; the hardware overlaps the partners.
//   * registers (256 per wave, all arch VGPRs): O^T (64), Q fragments (32), row-sum accumulators (8), one score tile (64) whose
//     registers also take the packed P^T words, a fragment ring (16), state and temporaries (32); 32 are hipcc's across the loop.
//     hipcc could not be made to allocate this (given virtual 16-register tuples it moved whole tiles between phases and spilled the
//     Q fragments: 228-660 bytes of scratch per lane in every C++ form tried; naming the accumulator file halves the arch budget), so
//     every tile has a HOME register and the whole loop is ONE asm statement per mode, generated with those registers
//     (tools/gen_duo_asm.py -> fa_fwd_duo_asm.inc, register map and loop structure in the generator's header); hipcc copies each tile
//     in once.  It pads nothing inside asm: the stream carries its own s_waitcnt and wait states, audited by the generator
//     (check_stream) and tests/test_duo_codegen.py.
//   * K / V rings of 6 slots per tensor, 3 per key group (read now / landed or landing / free), filled by LDS-DMA (the group that
//     reads a tile also copies it): the batch K(t+4), V(t+2) issued at the tail of M(t) goes to the group's free slots (what they
//     held was read two barriers back), is waited for one iteration later (vmcnt(4)) and read in M(t+4) / M(t+4).
//
//   * variants (template parameter NZ = 32-row query blocks per wave; the generator's set_nz):
//     NZ = 1, E = 64   the same loop without its z = 1 half: 32 rows per wave, 128 per workgroup -- for launches whose 256-row blocks
//                      would leave CUs idle (fa_launch.hpp small_grid_prefers_32_row_waves).  The partners finish the same 32 rows, group 0
//                      the first half of the columns and the residuals, group 1 the second.
//     NZ = 2, E = 32   the E = 64 loop with two contraction steps and one column block of O^T per query block (8 + 8 + 8 MFMAs per tile against
//                      the same 128 logits per lane: the vector phase is the bound outright); grids of >= 256 blocks.
//     NZ = 1, E = 128  O^T is again 64 registers (32 rows x 128 columns), Q eight fragments; tiles of 16 KiB -> 2 ring slots per key group,
//                      the LDS-DMA batch (8 pieces per wave) in the VECTOR phase behind the barrier that closes the matrix phase whose
//                      slots it overwrites, a barrier behind every phase.  LDS-bound per tile (slower than fa_fwd_w64.hpp on grids that
//                      fill the chip), launched on small grids only (fa_fwd_inst.hpp fwd_form_of).
//
// Modes: 0 plain / 1 masked (causal, key padding, ragged KL).  Exact fp32 scale only.  Same numerics contract as the other forms
// (fp32 softmax, deferred row max with threshold 2^8, O normalised once, residuals ms / ls per src/attention.jl:128-129); the
// summation order over keys differs from the one-wave form (two partial sums per row), so results agree to rounding, not bitwise.
#pragma once
#include "fa_fwd_w64.hpp"
#include "fa_fwd_duo_asm.inc"

#if !defined(NNOP_DEV_BUILD)
#undef NNOP_DUO_STAMP
#undef NNOP_DUO_PRIO
#endif
#ifndef NNOP_DUO_STAMP
#define NNOP_DUO_STAMP 0
#endif
#ifndef NNOP_DUO_PRIO
#define NNOP_DUO_PRIO 0
#endif

namespace nnop {

// Operands of the generated loop statement: every tile in its home register (register map: tools/gen_duo_asm.py)
#if NNOP_DUO_VALU_SUMS
#define NNOP_DUO_SUMS_OPERAND , "+{v[248:251]}"(lsum)
#else
#define NNOP_DUO_SUMS_OPERAND
#endif
#if NNOP_DUO_STAMP
#define NNOP_DUO_PROF_OPERAND , "+{v[224:231]}"(profv)
#else
#define NNOP_DUO_PROF_OPERAND
#endif
#define NNOP_DUO_OPERANDS                                                                                                        \
    "+{v[0:15]}"(oacc[0][0]), "+{v[16:31]}"(oacc[0][1]), "+{v[32:47]}"(oacc[1][0]), "+{v[48:63]}"(oacc[1][1]), "+{v[64:79]}"(qf[0]),   \
        "+{v[80:95]}"(qf[1]), "+{v[96:99]}"(lacc[0]), "+{v[100:103]}"(lacc[1]), "+{v[104:107]}"(sel), "+{v[112:127]}"(sc[0][0]),      \
        "+{v[128:143]}"(sc[0][1]), "+{v[144:159]}"(sc[1][0]), "+{v[160:175]}"(sc[1][1]), "+{v[192:195]}"(mstate), [st] "+s"(s_t),      \
        [ska] "+s"(s_ka), [skb] "+s"(s_kb), [skc] "+s"(s_kc), [sva] "+s"(s_va), [svb] "+s"(s_vb), [svc] "+s"(s_vc) NNOP_DUO_PROF_OPERAND NNOP_DUO_SUMS_OPERAND \
        : "{v[196:203]}"(vconst), [sh] "s"(s_h), [snlive] "s"(s_nlive), [slast] "s"(s_last), [sc2] "s"(c2), [scq0] "s"(s_cq0),            \
          [svbits] "s"(s_vbits), [krs] "s"(krs), [vrs] "s"(vrs)                                                                       \
        : "memory", "vcc", "scc", "v108", "v109", "v110", "v111", "v176", "v177", "v178", "v179", "v180", "v181", "v182", "v183", "v184", \
          "v185", "v186", "v187", "v188", "v189", "v190", "v191", "v204", "v205", "v206", "v207", "v208", "v209", "v210", "v211", "v212",   \
          "v213", "v214", "v215", "v216", "v217", "v218", "v219", "v220", "v221", "v222", "v223", "s56", "s57", "s58", "s59", "s60", "s61",  \
          "s62", "s63", "s64", "s65", "s66", "s67", "s68", "s69", "s70", "s71", "s72", "s73", "s74", "s75", "s76", "s77"

// NZ = 1: the z = 0 tiles only; v[144:175] (the z = 1 score tile's registers) are the loop's 8-slot fragment ring
#define NNOP_DUO1_OPERANDS                                                                                                       \
    "+{v[0:15]}"(oacc[0][0]), "+{v[16:31]}"(oacc[0][1]), "+{v[64:79]}"(qf[0]), "+{v[96:99]}"(lacc[0]), "+{v[104:107]}"(sel),              \
        "+{v[112:127]}"(sc[0][0]), "+{v[128:143]}"(sc[0][1]), "+{v[192:195]}"(mstate), [st] "+s"(s_t), [ska] "+s"(s_ka), [skb] "+s"(s_kb), \
        [skc] "+s"(s_kc), [sva] "+s"(s_va), [svb] "+s"(s_vb), [svc] "+s"(s_vc)                                                         \
        : "{v[196:203]}"(vconst), [sh] "s"(s_h), [snlive] "s"(s_nlive), [slast] "s"(s_last), [sc2] "s"(c2), [scq0] "s"(s_cq0),            \
          [svbits] "s"(s_vbits), [krs] "s"(krs), [vrs] "s"(vrs)                                                                       \
        : "memory", "vcc", "scc", "v108", "v109", "v110", "v111", "v144", "v145", "v146", "v147", "v148", "v149", "v150", "v151", "v152", \
          "v153", "v154", "v155", "v156", "v157", "v158", "v159", "v160", "v161", "v162", "v163", "v164", "v165", "v166", "v167", "v168",   \
          "v169", "v170", "v171", "v172", "v173", "v174", "v175", "v176", "v177", "v178", "v179", "v180", "v181", "v182", "v183", "v204",   \
          "v205", "v206", "v207", "v208", "v209", "v210", "v211", "v212", "v213", "v214", "v215", "v216", "v217", "v218", "v219", "v220",   \
          "v221", "v222", "v223", "s56", "s57", "s58", "s59", "s60", "s61", "s62", "s63", "s64", "s65", "s66", "s67", "s68", "s69", "s70",    \
          "s71", "s72", "s73", "s74", "s75", "s76", "s77"

// E = 32 (NZ = 2): one column block of O^T per query block (v[0:15], v[32:47]), two Q fragments each (v[64:71], v[80:87]); the rest as E = 64
#define NNOP_DUO32_OPERANDS                                                                                                      \
    "+{v[0:15]}"(oacc[0][0]), "+{v[32:47]}"(oacc[NZ - 1][0]), "+{v[64:79]}"(qf[0]), "+{v[80:95]}"(qf[NQT - 1]), "+{v[96:99]}"(lacc[0]),  \
        "+{v[100:103]}"(lacc[NZ - 1]), "+{v[104:107]}"(sel), "+{v[112:127]}"(sc[0][0]), "+{v[128:143]}"(sc[0][1]),                       \
        "+{v[144:159]}"(sc[NZ - 1][0]), "+{v[160:175]}"(sc[NZ - 1][1]), "+{v[192:195]}"(mstate), [st] "+s"(s_t), [ska] "+s"(s_ka),        \
        [skb] "+s"(s_kb), [skc] "+s"(s_kc), [sva] "+s"(s_va), [svb] "+s"(s_vb), [svc] "+s"(s_vc)                                        \
        : "{v[196:203]}"(vconst), [sh] "s"(s_h), [snlive] "s"(s_nlive), [slast] "s"(s_last), [sc2] "s"(c2), [scq0] "s"(s_cq0),            \
          [svbits] "s"(s_vbits), [krs] "s"(krs), [vrs] "s"(vrs)                                                                       \
        : "memory", "vcc", "scc", "v108", "v109", "v110", "v111", "v176", "v177", "v178", "v179", "v180", "v181", "v182", "v183", "v184", \
          "v185", "v186", "v187", "v188", "v189", "v190", "v191", "v204", "v205", "v206", "v207", "v208", "v209", "v210", "v211", "v212",   \
          "v213", "v214", "v215", "v216", "v217", "v218", "v219", "v220", "v221", "v222", "v223", "s56", "s57", "s58", "s59", "s60", "s61",  \
          "s62", "s63", "s64", "s65", "s66", "s67", "s68", "s69", "s70", "s71", "s72", "s73", "s74", "s75", "s76", "s77"

// E = 128 (NZ = 1): O^T = 4 column blocks, Q = 8 fragments; v[100:103] more K fragment addresses, v[180:182] more DMA offsets
#define NNOP_DUO128_OPERANDS                                                                                                     \
    "+{v[0:15]}"(oacc[0][0]), "+{v[16:31]}"(oacc[0][1]), "+{v[32:47]}"(oacc[0][EB - 2]), "+{v[48:63]}"(oacc[0][EB - 1]),                  \
        "+{v[64:79]}"(qf[0]), "+{v[80:95]}"(qf[NQT - 1]), "+{v[96:99]}"(lacc[0]), "+{v[104:107]}"(sel), "+{v[112:127]}"(sc[0][0]),        \
        "+{v[128:143]}"(sc[0][1]), "+{v[192:195]}"(mstate), [st] "+s"(s_t), [ska] "+s"(s_ka), [skb] "+s"(s_kb), [skc] "+s"(s_kc),         \
        [sva] "+s"(s_va), [svb] "+s"(s_vb), [svc] "+s"(s_vc)                                                                            \
        : "{v[196:203]}"(vconst), [sh] "s"(s_h), [snlive] "s"(s_nlive), [slast] "s"(s_last), [sc2] "s"(c2), [scq0] "s"(s_cq0),            \
          [svbits] "s"(s_vbits), [krs] "s"(krs), [vrs] "s"(vrs)                                                                       \
        : "memory", "vcc", "scc", "v100", "v101", "v102", "v103", "v108", "v109", "v110", "v111", "v144", "v145", "v146", "v147", "v148",  \
          "v149", "v150", "v151", "v152", "v153", "v154", "v155", "v156", "v157", "v158", "v159", "v160", "v161", "v162", "v163", "v164",   \
          "v165", "v166", "v167", "v168", "v169", "v170", "v171", "v172", "v173", "v174", "v175", "v176", "v177", "v178", "v179", "v180",   \
          "v181", "v182", "v183", "v204", "v205", "v206", "v207", "v208", "v209", "v210", "v211", "v212", "v213", "v214", "v215", "v216",   \
          "v217", "v218", "v219", "v220", "v221", "v222", "v223", "s56", "s57", "s58", "s59", "s60", "s61", "s62", "s63", "s64", "s65",     \
          "s66", "s67", "s68", "s69", "s70", "s71", "s72", "s73", "s74", "s75", "s76", "s77"

constexpr int kDuoXchgBytes = 8 * (8192 + 3 * 256);          // epilogue exchange: per wave 32 fp32 per lane + (l, m2, mt)
// ring slots per key group and ring / barriers per iteration: properties of the generated loop of an embedding dim (fa_fwd_duo_asm.inc)
template <int E> constexpr int duo_slots_per_group() { return E == 128 ? NNOP_DUO128_SLOTS_PER_GROUP : NNOP_DUO_SLOTS_PER_GROUP; }
template <int E> constexpr bool duo_sync_one() { return (E == 128 ? NNOP_DUO128_SYNC_ONE : NNOP_DUO_SYNC_ONE) != 0; }
template <typename T, int E> constexpr int fa_fwd_duo_lds_bytes(bool masked) {
    constexpr int ring = 2 * duo_slots_per_group<E>() * (RowImg<T, E>::bytes(64) + ColImg<T, E>::bytes(64));
    return (ring > kDuoXchgBytes ? ring : kDuoXchgBytes) + (masked ? 16 + 8 * kMaxMaskTiles : 0);
}

// NZ: 32-row query blocks per wave.  2: 64 rows per wave, 256 per workgroup (the form described above).  1: the same loop with the z = 1
// half left out -- 32 rows per wave, 128 per workgroup, for problems whose 256-row blocks cannot fill the chip (twice the workgroups;
// every fragment then feeds one MFMA and the per-iteration overheads are paid per 32 rows: ~8 % more cycles per row).
// SINK: learned attention sinks (fa_fwd.hpp), merged with the partner's partial in `take`
#include "fa_fwd_duo_kernel.inc"

}  // namespace nnop
