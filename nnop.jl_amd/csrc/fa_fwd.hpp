// fa_fwd.hpp -- gfx950 flash-attention forward kernel (template; instantiated per dtype in
// fa_fwd_*.hip).
//
// Computes what `_flash_attention_fwd!` computes (src/attention.jl:1-131): per (q-tile, q-head,
// batch)  S = scale*Q K^T (+pair), causal / key-padding mask -> -inf, online softmax, O = P V,
// and the residuals ms (row max) and ls (row sum of exp(s - ms)).  It is a different program:
//
//   reference (attention.jl)                      this kernel
//   -----------------------------------------    ---------------------------------------------
//   1 thread = 1 query row, scalar FMAs out of    1 wave = QB blocks of 32 query rows, both
//   LDS (mma!, mma.jl:6-48), T accumulation       contractions on MFMA 32x32x16 (bf16/f16) /
//                                                 32x32x2 (f32), fp32 accumulation
//   S, P round-trip through s_shm                 S^T = K Q^T ("swapped"): the query sits on the
//                                                 lane, its 32 keys in registers -> softmax is
//                                                 in-register, and exp(S^T) IS the B operand of
//                                                 O^T = V^T P^T (no LDS for S or P)
//   O normalised after every tile (FA-1)          O un-normalised, one divide in the epilogue
//   5 barriers / kv tile                          1 barrier / kv tile (K ring + V ring in LDS)
//   uncoalesced per-row loads                     16-byte coalesced tile loads, issued ahead,
//                                                 written to LDS after the compute phase
//   QK^T, softmax, PV strictly one after the      software-pipelined across tiles INSIDE a wave:
//   other                                         one straight-line block holds the QK^T MFMAs of
//                                                 tile t+1, the exp/convert of tile t, the PV
//                                                 MFMAs of tile t and the row max of tile t+1
//   scale, max-subtraction, exp in T              one fp32 fma + v_exp per logit: P = exp2(s*c - m);
//                                                 rescale deferred (threshold 2^8); row sums by MFMA
//                                                 (all-ones A operand) where registers allow
//
// Work decomposition: workgroup = NW waves x QB x 32 consecutive query rows of one (batch, q-head);
// kv tiles of BK keys.  QB = 2 (64 rows per wave, one wave per SIMD, 512-register budget) halves the
// LDS fragment bytes per MFMA -- every K / V fragment read from LDS feeds two MFMAs -- which is what
// bounds the QB = 1 form (measured: per kv tile a wave waited ~700 cycles for its fragments and
// ~470 at the barrier against ~1100 in the MFMA block; profiles/r01/).  Linear workgroup ids are
// remapped so that the workgroups sharing one (batch, kv-head) -- the same K/V bytes -- run on one
// XCD's L2.
#pragma once
#include <type_traits>
#include "fa_common.hpp"

// Timing-only ablation builds (make DEV=1 ABL=n OUTDIR=../lib_abl<n>): results are WRONG by construction.
//   1 no per-interval barrier   2 no exp   3 no PV MFMAs   4 no QK^T MFMAs   5 no LDS fragment reads
//   6 no HBM->LDS staging       7 no row-sum MFMAs          8 no row max
// The release build (no NNOP_DEV_BUILD) pins NNOP_ABL to 0: none of that code exists in the shipped library.
#if !defined(NNOP_DEV_BUILD)
#undef NNOP_ABL
#endif
#ifndef NNOP_ABL
#define NNOP_ABL 0
#endif
// Variant switches for A/B timing (make DEV=1 VAR="-DNNOP_V_...=0"); defaults are the shipped configuration and the
// only one a release build can have.
#if !defined(NNOP_DEV_BUILD)
#undef NNOP_V_PREFETCH
#undef NNOP_V_DEEP
#undef NNOP_V_MFMASUM
#undef NNOP_V_SETPRIO
#endif
#ifndef NNOP_V_PREFETCH
#define NNOP_V_PREFETCH 1
#endif
#ifndef NNOP_V_DEEP
#define NNOP_V_DEEP 1
#endif
#ifndef NNOP_V_MFMASUM
#define NNOP_V_MFMASUM 1
#endif
#ifndef NNOP_V_SETPRIO
#define NNOP_V_SETPRIO 0
#endif

namespace nnop {

// key padding: one 64-bit validity word per 64 keys is kept in LDS for up to this many words (64K keys)
constexpr int kMaxMaskTiles = 1024;

struct FwdParams {
    void*       o;
    void*       ms;
    void*       ls;
    const void* q;
    const void* k;
    const void* v;
    const void* pair;        // nullable, [B][KL][QL][QH]
    const uint8_t* kpad;     // nullable, [B][KL]
    int   QL, KL, QH, KH, B;
    int   causal;
    int   n_qblk;            // ceil(QL / (32*QB*NW))
    int   n_wg;              // n_qblk * QH * B
    float scale;             // 1/sqrt(E)
    int   persist_hx = 0;    // persistent form: heads per XCD when QH % 8 == 0 (the XCD's columns = those heads of every batch), else 0
    int   persist = 0;       // fa_fwd_w64_kernel: blocks per workgroup of the persistent form (grid = 256 workgroups), 0 = one block per workgroup
    int   persist_asc = 0;   // persistent form: q-blocks of a column in ASCENDING order (light blocks first), see fwd_persist_plan
    int   causal_alt = 0;    // fa_fwd_kernel, causal: g > 0 -- every second run of g consecutive blocks of an XCD's dispatch order (whole columns) runs its q-blocks ascending (launch_fwd_cfg)
    // fa_fwd_kernel<..., WIN = true> and fa_fwd_generic_kernel: sliding window (FaWindow, normalised), -1 = unbounded side.  Behind
    // the older fields, so that their kernel-argument offsets stay where they were.
    int   win_left = -1;
    int   win_right = -1;
    // the SINK = true instantiations of every form: learned per-head attention sinks, fp32 [QH], merged in the epilogue (sink_merge).
    // Behind the window for the same reason.
    const float* sinks = nullptr;
    // the CAP = true instantiations of fa_fwd_kernel and fa_fwd_generic_kernel: logit soft-capping, the two folded constants of
    // SoftcapK (fa_launch.hpp).  Behind the sinks for the same reason.
    float cap_ka = 0.f;
    float cap_kb = 0.f;
#ifdef NNOP_DEV_BUILD
    int   stagger = 0;       // experiment: s_sleep units for the odd co-resident workgroup (0 = off)
#endif
};

// MODE 0: plain   -- KL % BK == 0, no causal, no kpad, no pair: every logit is live
// MODE 1: masked  -- causal and/or key padding and/or ragged KL
// MODE 2: pair    -- masked + additive pair bias
// WIN (MODE 1 / 2 only): sliding window p.win_left / p.win_right.  The workgroup walks kv tiles [t_lo, t_hi) only; loop indices
// are RELATIVE to t_lo (tile t of the walk is kv tile t0 + t), each wave computes only its own live tiles [w_lo, n_live), one
// tile per interval (no software pipeline, see kPipe), and takes the per-element select only on tiles that cross a window
// edge, the diagonal, KL or a key-padding word (tile_needs_mask).  WIN = false compiles to the code without a window.
// SINK: learned attention sinks (p.sinks, non-null), merged in the epilogue.  SINK = false (the calls without sinks) compiles the sink
// code away.
// CAP (MODE 1 / 2 only, instantiated with WIN = true only): logit soft-capping, x = c * tanh(s * scale / c) (+ pair), applied in finish_x
// to the raw accumulators; the tile is then in log2 units, as with a pair bias.  CAP = false (the calls without a cap) compiles it away.
#include "fa_fwd_kernel.inc"

// LDS bytes the kernel needs: K ring of 2 + V ring of 2 + one scratch slot + (key padding) one 64-bit validity
// word per kv tile for up to kMaxMaskTiles tiles (longer sequences fall back to reading the mask per tile).
template <typename T, int E, int BK> constexpr int fa_fwd_lds_bytes() {
    return 2 * (RowImg<T, E>::bytes(BK) + ColImg<T, E>::bytes(BK)) + 16 + 8 * kMaxMaskTiles;
}

}  // namespace nnop
