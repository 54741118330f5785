// fa_fwd_inst.hpp -- host-side dispatch for the forward kernel; included by the three per-dtype
// translation units so that they compile in parallel.
//
// Replaces the reference's host launcher heuristics (src/attention.jl:146-163, :193-218): there the
// workgroup size is the largest of (256..16) whose backward LDS footprint fits; here the tile is
// fixed by the MFMA shape (32 queries per wave, BK keys per step) and only the number of waves per
// workgroup is chosen, from how many workgroups the problem yields against the chip's 256 CUs.
#pragma once
#include "fa_fwd.hpp"
#include "fa_fwd_split.hpp"
#include "fa_fwd_w64.hpp"
#include "fa_fwd_duo.hpp"
#include "fa_generic.hpp"
#ifdef NNOP_DEV_BUILD
#include <stdlib.h>
#endif
#include "fa_launch.hpp"
#include <math.h>

namespace nnop {

#ifdef NNOP_DEV_BUILD
static inline int dev_env_int(const char* name, int dflt) {
    const char* s = getenv(name);
    return (s && *s) ? atoi(s) : dflt;
}
#endif

// Everything in FwdParams that is a plain function of (descriptor, arguments, query rows per workgroup); the rest is zero / unbounded.
// A launcher then sets only what is its own (causal_alt, the persist fields, stagger).  rows = 0: the plain-HIP kernel, whose grid is
// not one of row blocks.  (The split, w64 and duo kernels never read pair, and the split kernel neither kpad nor causal: those forms
// are chosen only for calls that have none -- fwd_form_of: mode != 2, mode == 0 -- so the arguments pass through as they are.)
static inline int fwd_params(FwdParams& p, const nnop_fa_desc& d, const FwdArgs& a, int rows) {
    p = FwdParams{};
    p.o = a.o; p.ms = a.ms; p.ls = a.ls;
    p.q = a.q; p.k = a.k; p.v = a.v; p.pair = a.pair; p.kpad = a.kpad;
    p.sinks = a.sinks;
    p.QL = d.ql; p.KL = d.kl; p.QH = d.qh; p.KH = d.kh; p.B = d.batch;
    p.causal = d.causal ? 1 : 0;
    p.scale = (float)(1.0 / sqrt((double)d.emb));    // T(inv(sqrt(QE))), src/attention.jl:154
    p.win_left = a.win.left; p.win_right = a.win.right;
    if (a.softcap != 0.f) { const SoftcapK ck = softcap_k(1.0 / sqrt((double)d.emb), a.softcap); p.cap_ka = ck.ka; p.cap_kb = ck.kb; }
    if (rows > 0) {
        p.n_qblk = (d.ql + rows - 1) / rows;
        const long long n_wg = (long long)p.n_qblk * d.qh * d.batch;
        if (n_wg <= 0 || n_wg > 0x7fffffffLL) return NNOP_ERR_SHAPE;
        p.n_wg = (int)n_wg;
    }
    return NNOP_OK;
}

template <typename T, int E, int NW, int MODE, int QB, bool WIN = false, bool CAP = false, bool SINK = false>
static int launch_fwd_cfg(const nnop_fa_desc& d, const FwdArgs& a, hipStream_t s) {
    // learned sinks: the SINK = true instantiation of the kernel (fa_fwd.hpp; the code of the calls without them stays as it is), from the
    // SINK = true instantiation of this launcher, so that every kernel has its own LDS opt-in word below.  The other launchers likewise.
    if constexpr (!SINK) {
        if (a.sinks) return launch_fwd_cfg<T, E, NW, MODE, QB, WIN, CAP, true>(d, a, s);
    }
    // 64-key tiles, except the E = 128 pair-bias body (register budget) and fp32 E = 128
    // (LDS: 2 x (K + V) x 64 keys x 512 B = 128 KiB would leave one workgroup per CU)
    constexpr int BK = (E >= 256 || (E >= 128 && (MODE == 2 || sizeof(T) == 4))) ? 32 : 64;
    constexpr int lds = fa_fwd_lds_bytes<T, E, BK>();
    static_assert(lds <= 160 * 1024, "LDS budget (160 KiB per CU on gfx950)");
    constexpr auto kern = fa_fwd_kernel<T, E, NW, BK, MODE, QB, WIN, SINK, CAP>;
    static unsigned long long lds_done = 0;
    if (ensure_dynamic_lds(kern, lds, &lds_done) != NNOP_OK) return NNOP_ERR_HIP;
    FwdParams p;
    if (const int st = fwd_params(p, d, a, 32 * QB * NW); st != NNOP_OK) return st;
    // Causal launches of a few rounds: pair heavy with light blocks on a CU (fa_launch.hpp causal_alt_run).  Measured (round 4,
    // profiles/r04/causal_alt.log): fp32 E64 L4096 H4 B4 545.6 -> 319.6 us, fp32 E32 301 -> 180, fp32 E16 233 -> 142, bf16 E16 69.8 -> 53.0,
    // fp32 E64 L2048 H8 B8 (4 rounds) 473 -> 428; GQA at 4 rounds -5 %, 8 rounds and more -12 % (the rule stops before).  Where ONE workgroup
    // fills a CU there is nothing to pair (E = 128 with 8 waves; fp32 E = 128 with 4 waves fits two).
    // (a window: every block walks about the same number of tiles -- nothing to pair)
    p.causal_alt = (!WIN && MODE != 2 && (E <= 64 || (E == 128 && sizeof(T) == 4 && NW == 4)))
                       ? causal_alt_run(d.causal != 0, p.n_wg, (long long)d.qh * d.batch, d.qh / d.kh, p.n_qblk) : 0;
    int lds_launch = lds;
#ifdef NNOP_DEV_BUILD
    // experiments (make DEV=1 only): de-phase co-resident workgroups; pad LDS to limit workgroups per CU
    p.stagger = dev_env_int("NNOP_FWD_STAGGER", 0);
    lds_launch += dev_env_int("NNOP_FWD_LDS_PAD", 0);
    if (lds_launch > lds && lds_launch > 64 * 1024 &&
        hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds_launch) != hipSuccess) {
        (void)hipGetLastError();
        return NNOP_ERR_HIP;
    }
#endif
    hipLaunchKernelGGL(kern, dim3((unsigned)p.n_wg), dim3(NW * 64), lds_launch, s, p);
    return hipGetLastError() == hipSuccess ? NNOP_OK : NNOP_ERR_HIP;
}

// split-KV form (fa_fwd_split.hpp): 16 waves per workgroup, plain mode, 16-bit types, E <= 64.
// (A v_mfma_f32_16x16x32 body of this form was built and measured 7 % slower in round 1 -- twice the MFMA issues on the port
// that is the bottleneck; DESIGN.md section 5 -- and is no longer in the tree.)
template <typename T, int E, bool SINK = false>
static int launch_fwd_split(const nnop_fa_desc& d, const FwdArgs& a, hipStream_t s) {
    if constexpr (!SINK) {
        if (a.sinks) return launch_fwd_split<T, E, true>(d, a, s);
    }
    constexpr int lds = fa_fwd_split_lds_bytes<T, E>();
    constexpr auto kern = fa_fwd_split_kernel<T, E, SINK>;
    static_assert(lds <= 160 * 1024, "LDS budget");
    static unsigned long long lds_done = 0;
    if (ensure_dynamic_lds(kern, lds, &lds_done) != NNOP_OK) return NNOP_ERR_HIP;
    FwdParams p;
    if (const int st = fwd_params(p, d, a, 256); st != NNOP_OK) return st;
    hipLaunchKernelGGL(kern, dim3((unsigned)p.n_wg), dim3(1024), lds, s, p);
    return hipGetLastError() == hipSuccess ? NNOP_OK : NNOP_ERR_HIP;
}

// Persistent form of the masked-mode kernels (fa_fwd_w64.hpp, fa_fwd_duo.hpp): the rule is persist_list (fa_launch.hpp).  Fills
// p.persist / p.persist_hx / p.persist_asc and the grid when the form applies.
static inline void fwd_persist_plan(const nnop_fa_desc& d, const FwdArgs& a, FwdParams& p, long long& grid) {
    // (auto: under a causal mask without key padding -- there the static list balances exactly and measured +3..4 % at E = 128
    // L 8192-16384, +23 % at E = 64 L4096 H16 B4; equal-work blocks gain nothing (+-0.3 %), and per-batch key lengths make a
    // static list 15 % SLOWER than the dispatcher's dynamic order: C4)
    // per-batch key lengths WITHOUT a causal mask: balanced as well once every XCD takes an eighth of the heads of every batch
    const bool pays = (d.causal && !a.kpad) || (!d.causal && a.kpad && d.qh % 8 == 0);
    const PersistList l = persist_list((long long)d.batch * d.qh, d.qh, p.n_qblk, tune_get(kTuneFwdPersist), pays);
    if (l.steps == 0) return;
    p.persist = l.steps;
    p.persist_hx = l.hx;
    // Order of a column's q-blocks: descending (heaviest first).  The ascending order (light blocks first, so that every
    // workgroup starts at kv tile 0 together and the heavy blocks follow staggered inside each other's L2 window) was built and
    // measured in round 4: same time (+-0.1 %: C3 3912 vs 3918 us, C5 shard 15084 vs 15100 us), MORE fabric traffic at the C5
    // shard (7.93 vs 6.11 GB per launch; C3 2.34 vs 2.32 GB) -- profiles/r04/persist_order.log.  Knob kTuneFwdPersistAsc (1 = ascending).
    p.persist_asc = tune_get(kTuneFwdPersistAsc) > 0 ? 1 : 0;
    grid = 256;
}

// 64-rows-per-wave form (fa_fwd_w64.hpp): 4 waves x 64 rows, 16-bit types, E = 64 / 128, plain and masked modes
template <typename T, int E, int MODE, bool PRE, bool SINK = false>
static int launch_fwd_w64(const nnop_fa_desc& d, const FwdArgs& a, hipStream_t s) {
    if constexpr (!SINK) {
        if (a.sinks) return launch_fwd_w64<T, E, MODE, PRE, true>(d, a, s);
    }
    constexpr int EV = E == 256 ? 128 : E;                   // E = 256: two 128-column halves of O per block (fa_fwd_w64.hpp)
    constexpr int lds = fa_fwd_w64_lds_bytes<T, E, EV>(MODE != 0);
    static_assert(lds <= 160 * 1024, "LDS budget");
    constexpr auto kern = fa_fwd_w64_kernel<T, E, MODE, PRE, EV, SINK>;
    static unsigned long long lds_done = 0;
    if (ensure_dynamic_lds(kern, lds, &lds_done) != NNOP_OK) return NNOP_ERR_HIP;
    FwdParams p;
    if (const int st = fwd_params(p, d, a, 256); st != NNOP_OK) return st;
    long long grid = (long long)p.n_wg * (E / EV);
    if (grid > 0x7fffffffLL) return NNOP_ERR_SHAPE;
    if constexpr (EV == E && MODE == 1) fwd_persist_plan(d, a, p, grid);
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(256), lds, s, p);
    return hipGetLastError() == hipSuccess ? NNOP_OK : NNOP_ERR_HIP;
}

// two waves per SIMD in alternating phases (fa_fwd_duo.hpp): 8 waves, 256 query rows per workgroup, 16-bit types, E = 64
// (NZ = 1: 32 rows per wave, 128 per workgroup -- fwd_duo_nz below)
template <typename T, int E, int MODE, int NZ, bool SINK = false>
static int launch_fwd_duo(const nnop_fa_desc& d, const FwdArgs& a, hipStream_t s) {
    if constexpr (!SINK) {
        if (a.sinks) return launch_fwd_duo<T, E, MODE, NZ, true>(d, a, s);
    }
    constexpr int lds = fa_fwd_duo_lds_bytes<T, E>(MODE != 0);
    static_assert(lds <= 160 * 1024, "LDS budget");
    constexpr auto kern = fa_fwd_duo_kernel<T, E, MODE, NZ, SINK>;
    static unsigned long long lds_done = 0;
    if (ensure_dynamic_lds(kern, lds, &lds_done) != NNOP_OK) return NNOP_ERR_HIP;
    FwdParams p;
    if (const int st = fwd_params(p, d, a, 128 * NZ); st != NNOP_OK) return st;
    long long grid = p.n_wg;
    if constexpr (MODE == 1) fwd_persist_plan(d, a, p, grid);
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(512), lds, s, p);
    return hipGetLastError() == hipSuccess ? NNOP_OK : NNOP_ERR_HIP;
}

// The launcher's choice of kernel form, as a plain function of the descriptor (also reported through nnop_debug_fwd_form).
//   mode: 0 plain (every logit live), 1 masked (causal / key padding / ragged KL / sliding window), 2 + pair bias
//   (a soft cap runs the masked bodies as well: fa_fwd.hpp CAP)
static inline int fwd_mode(const nnop_fa_desc& d, bool has_pair, bool has_mask, bool win_on, bool capped) {
    return has_pair ? 2 : ((d.causal || has_mask || win_on || capped || (d.kl % 64) != 0) ? 1 : 0);
}
// Workgroups of a forward grid with `rows` query rows each
static inline long long fwd_wg(const nnop_fa_desc& d, int rows) { return (long long)((d.ql + rows - 1) / rows) * d.qh * d.batch; }
// Can the one-wave / two-wave forms (fa_fwd_w64.hpp, fa_fwd_duo.hpp) address this problem?  No pair bias; masked mode keeps the per-tile
// validity words in LDS (KL <= 64 Ki); their LDS-DMA addresses a (batch, kv-head) tensor through a 32-bit buffer offset.
static inline bool fwd_wide_fits(const nnop_fa_desc& d, int mode) {
    return mode != 2 && (mode == 0 || d.kl <= 64 * kMaxMaskTiles) && (long long)d.kl * d.emb * 2 < (1LL << 32);
}
// Rows per wave of the two-waves-per-SIMD form at E = 64: 64 (NZ = 2, 256-row workgroups), or 32 (NZ = 1: twice the workgroups) where the
// 256-row blocks leave CUs idle (small_grid_prefers_32_row_waves, fa_launch.hpp; L1024 H8 B4: 19.8 -> 14.0 us; L2048 H4 B4: 30.9 -> 21.4 us;
// causal L4096 H8 B2: 57.6 -> 45.1 us; L8192 H8 B1: 104.6 -> 79.6 us).  Knob kTuneFwdDuo: 2 / 3 force NZ = 2 / 1.
static inline int fwd_duo_nz(const nnop_fa_desc& d) {
    const int duo = tune_get(kTuneFwdDuo);
    if (duo == 2) return 2;
    if (duo == 3) return 1;
    return small_grid_prefers_32_row_waves(d.ql, (long long)d.qh * d.batch, d.causal != 0) ? 1 : 2;
}
// wg256 / wg128: fwd_wg of 256- and 128-row workgroups
static inline int fwd_form_of(const nnop_fa_desc& d, int mode, bool win_on, bool capped, long long wg256, long long wg128) {
    const bool b16 = d.dtype != NNOP_F32;
    const int E = d.emb;
    // the early exits of launch_fwd: embedding dims outside the tiled set (16-bit E = 256 runs the 32-row tiled kernel)
    if (E != 256 && emb_generic(E)) return kFormGeneric;
    // a sliding window (FaWindow::on) exists in the 32-row kernel only (fa_fwd.hpp WIN), not in the duo / w64 / split forms; so does a
    // soft cap (CAP)
    if (win_on || capped) return kFormRow32;
    const bool fits = fwd_wide_fits(d, mode);
    if (b16 && E == 256) {
        // E = 256: the 64-row form with two 128-column halves of O per block (spill-free; the 32-row form spills 62-152 registers
        // and measured 214 TFLOP/s at L2048 H8 B2).  No pair bias; masked mode up to 64 Ki keys; a few kv tiles.
        const int w64 = tune_get(kTuneFwdW64);
        if (fits && w64 != 0 && d.kl >= 128) return kFormW64;
    }
    if (b16 && (E == 64 || E == 128)) {
        // 64-row waves (fa_fwd_w64.hpp): 4 waves x 64 rows, one wave per SIMD with the whole register file.  Measured
        // against the 32-row forms after the round-2 schedule work (bf16 / fp16, MI355X, tools/w64_check.py): faster wherever
        // there are a few kv tiles and enough 256-row workgroups -- E = 64 plain +13..21 % from KL = 256 and 64 workgroups
        // up; E = 64 causal / padded +10..20 % from KL = 512 and 128 workgroups; E = 128 +9..47 % from KL = 256, except plain
        // problems with <= 128 workgroups (-3 %: the 32-row form splits them into twice as many) and KL = 128 (-33 %: the
        // prologue).  Masked mode needs the per-tile validity words in LDS (KL <= 64 Ki), the pair-bias mode stays on the
        // 32-row kernel.  Knob kTuneFwdW64: 0 never, 1 wherever instantiated, auto = the rule below.
        const int w64 = tune_get(kTuneFwdW64);
        const bool masked = mode == 1;
        const bool pays = E == 128 ? (d.kl >= 256 && (wg256 >= 160 || (masked && wg256 >= 64)))
                                   : (masked ? (d.kl >= 512 && wg256 >= 128) : (d.kl >= 256 && wg256 >= 64));
        // E = 64, exact scale: two waves per SIMD in alternating matrix / vector phases (fa_fwd_duo.hpp).  Measured against the
        // one-wave form on one box (tools/duo_check.py, profiles/r04/duo_sweep.log): 10-22 % faster from KL = 1024 up in plain mode at
        // every grid size (32 .. 4096 workgroups), 3-20 % faster in masked mode from KL = 2048 (from KL = 1024 with >= 128
        // workgroups); slower below (KL = 512: +10..19 %: the prologue holds three tiles and the epilogue merges two key groups).
        // Knob kTuneFwdDuo: 0 never, 1 wherever instantiated, auto = this rule.
        if (E == 128 && fits && tune_get(kTuneFwdExactScale) != 0) {
            // E = 128: the two-wave form exists with 32-row waves only (fa_fwd_duo.hpp: 128-row workgroups whose partner waves split the
            // keys).  Per tile it is 10-14 % SLOWER than the one-wave form (every fragment read feeds one MFMA: LDS-bound; C3 4388 vs
            // 3972 us), but it has twice the workgroups and halves a block's critical path: measured (profiles/r04/duo128_sweep.log)
            // 1.1-1.3x faster while the 128-row blocks fit one round (L2048 H8 B2: 42.9 -> 36.5 us), 1.3-1.7x under a causal mask
            // (L2048 H8 B2: 54.0 -> 33.4 us; L4096 H8 B1: 97.2 -> 57.8; L8192 H8 B1: 189 -> 135), and still ahead up to two rounds in
            // masked mode from KL = 2048 (causal L2048 H8 B4: 56.6 -> 44.3; lens L2048 B4: 68.8 -> 62.4).  KL = 256: a tie.
            const int duo = tune_get(kTuneFwdDuo);
            const long long cus = device_cu_count() > 0 ? device_cu_count() : 256;
            const bool duo_pays = d.kl >= 512 && (wg128 <= cus || (masked && d.kl >= 2048 && wg128 <= 2 * cus));
            if (duo >= 1 || (duo < 0 && w64 != 1 && duo_pays)) return kFormDuo;
        }
        if (E == 64 && fits && tune_get(kTuneFwdExactScale) != 0) {
            const int duo = tune_get(kTuneFwdDuo);
            // With 32-row waves (small grids, fwd_duo_nz) it wins from KL = 256 in every mode: 9-11 us against 13-16 us at KL = 512, 64-256
            // 128-row blocks; 7.4-9.4 us against 9.6-10.4 us at KL = 256 (profiles/r04/nz1_small.log).
            const bool duo_pays = fwd_duo_nz(d) == 1 ? d.kl >= 256 : (masked ? (d.kl >= 2048 || (d.kl >= 1024 && wg256 >= 128)) : d.kl >= 1024);
            if (duo >= 1 || (duo < 0 && w64 != 1 && duo_pays)) return kFormDuo;
        }
        if (fits && (w64 == 1 || (w64 < 0 && pays))) return kFormW64;
    }
    if (b16 && E == 32 && fits) {
        // E = 32: the two-waves-per-SIMD form with 64-row waves (fa_fwd_duo.hpp).  The softmax, not the matrix pipe, is the bound of every
        // form at E = 32 (they take as long as at E = 64).  Measured (profiles/r04/duo32_sweep.log), grids of >= 256 blocks: masked mode
        // 1.1-1.5x faster from KL = 1024 (causal L2048 H8 B8 61.2 -> 40.8 us, L4096 H8 B8 164 -> 125; key padding +2..12 %), plain mode
        // +3..6 % from KL = 2048; smaller grids lose (the 32-row forms have twice the workgroups).  Knob kTuneFwdDuo.
        const int duo = tune_get(kTuneFwdDuo);
        const bool duo_pays = wg256 >= 256 && (mode == 1 ? d.kl >= 1024 : d.kl >= 2048);
        if (duo >= 1 || (duo < 0 && duo_pays)) return kFormDuo;
    }
    if (b16 && E <= 64) {
        // plain mode: 16-wave split-KV workgroups (4 waves per SIMD); measured 5-13 % faster than the 8-wave form from 64 to
        // 4096 workgroups.  Knob kTuneFwdSplit: 0 off, 1 / auto on.
        if (mode == 0 && d.ql > 128 && d.kl >= 128 && tune_get(kTuneFwdSplit) != 0) return kFormSplit;
    }
    return kFormRow32;
}

template <typename T, int E>
static int launch_fwd_e(const nnop_fa_desc& d, const FwdArgs& a, hipStream_t s) {
    const bool win_on = a.win.on(), capped = a.softcap != 0.f;
    const int mode = fwd_mode(d, a.pair != nullptr, a.kpad != nullptr, win_on, capped);
    const long long wg256 = fwd_wg(d, 256), wg128 = fwd_wg(d, 128);
    const int form = fwd_form_of(d, mode, win_on, capped, wg256, wg128);
    if constexpr (sizeof(T) == 2 && E == 256) {
        if (form == kFormW64) return mode == 0 ? launch_fwd_w64<T, E, 0, false>(d, a, s) : launch_fwd_w64<T, E, 1, false>(d, a, s);    // exact scale only
    }
    if constexpr (sizeof(T) == 2 && E == 128) {
        if (form == kFormDuo) return mode == 0 ? launch_fwd_duo<T, E, 0, 1>(d, a, s) : launch_fwd_duo<T, E, 1, 1>(d, a, s);
    }
    if constexpr (sizeof(T) == 2 && E == 32) {
        if (form == kFormDuo) return mode == 0 ? launch_fwd_duo<T, E, 0, 2>(d, a, s) : launch_fwd_duo<T, E, 1, 2>(d, a, s);
    }
    if constexpr (sizeof(T) == 2 && E == 64) {
        if (form == kFormDuo) {
            if (fwd_duo_nz(d) == 1) return mode == 0 ? launch_fwd_duo<T, E, 0, 1>(d, a, s) : launch_fwd_duo<T, E, 1, 1>(d, a, s);
            return mode == 0 ? launch_fwd_duo<T, E, 0, 2>(d, a, s) : launch_fwd_duo<T, E, 1, 2>(d, a, s);
        }
    }
    if constexpr (sizeof(T) == 2 && (E == 64 || E == 128)) {
        if (form == kFormW64) {
            // The scale.  DEFAULT: exact -- scale * log2(e) applied in fp32 inside the exponent (one v_fma per logit).  Opt-in
            // (kTuneFwdExactScale = 0 / NNOP_FWD_EXACT_SCALE=0): folded into Q, rounded to T once, 8-12 % faster -- but every
            // channel of a query then carries a relative rounding of 2^-9 (bf16) / 2^-12 (fp16), and two near-tied keys that load
            // DIFFERENT channels get different errors: measured (tools/fold_sweep.py, profiles/r03/fold_sweep.log) the folded form
            // leaves the standard parity tolerance from |s * scale| ~ 5 (one outlier channel per key) / ~ 20 (dense directions) at
            // E = 64 -- inside what trained models produce -- while the exact form stays at 0.3 of the tolerance up to 65.  The
            // reference scales S itself in T (src/attention.jl:55), i.e. is coarser than either; parity is judged against the oracle.
            const bool exact = tune_get(kTuneFwdExactScale) != 0;
            if (mode == 0) return exact ? launch_fwd_w64<T, E, 0, false>(d, a, s) : launch_fwd_w64<T, E, 0, true>(d, a, s);
            return exact ? launch_fwd_w64<T, E, 1, false>(d, a, s) : launch_fwd_w64<T, E, 1, true>(d, a, s);
        }
    }
    if constexpr (sizeof(T) == 2 && E <= 64) {
        if (form == kFormSplit) return launch_fwd_split<T, E>(d, a, s);
    }
    // kFormRow32
    if (win_on || capped) {
        // sliding window: the 32-row kernel's WIN body, 4 waves (128-row workgroups: a block's rows span less of the window, and a
        // windowed grid has as many blocks as the causal one).  Logit soft-capping: the CAP instantiations of that body, same shape;
        // without a window its bounds stay -1 (unbounded)
        if (capped) return mode == 2 ? launch_fwd_cfg<T, E, 4, 2, 1, true, true>(d, a, s) : launch_fwd_cfg<T, E, 4, 1, 1, true, true>(d, a, s);
        return mode == 2 ? launch_fwd_cfg<T, E, 4, 2, 1, true>(d, a, s) : launch_fwd_cfg<T, E, 4, 1, 1, true>(d, a, s);
    }
    // Workgroup shape of the 32-row form: 8 waves x 32 rows (256-row workgroups) when that still yields >= one
    // workgroup per CU, else 4 waves x 32 rows so that small problems spread over more CUs.
    int nw = 8, qb = 1;
    if (wg256 < 256 || d.ql <= 128) nw = 4;
    // causal, E <= 64: the waves of a 256-row workgroup see 1..4 x the keys of its first wave and wait for the last one
    // at every barrier; 128-row workgroups waste half as much.  Measured (bf16, MI355X): E64 L4096 H16 B4 356 -> 304 us
    // (+17 %).  Only while that still leaves >= 2 workgroups per CU.  At E = 128 and long sequences the 8-wave form is
    // equal (C3: 5.60 vs 5.62-5.70 ms) or better (C5 shard: 20.4 vs 21.2-21.6 ms).
    // At E = 128 only for short sequences (QL <= 2048: L1024 314 -> 269 us, L2048 485 -> 469 us; from L4096 on the 8-wave
    // form wins: 723 vs 762-858 us).
    if (d.causal && wg128 >= 512 && (E <= 64 || d.ql <= 2048)) nw = 4;
    // fp32 E = 128 under a causal mask: two 4-wave workgroups fit a CU where one 8-wave workgroup does, and with the alternating block order
    // (launch_fwd_cfg) they pair heavy with light: L4096 H8 B2 1019.6 -> 627.0 us.  Only where that order applies.
    if constexpr (sizeof(T) == 4 && E == 128) {
        if (mode == 1 && causal_alt_run(d.causal != 0, wg128, (long long)d.qh * d.batch, d.qh / d.kh, (d.ql + 127) / 128) > 0) nw = 4;
    }
    if (E >= 128 && mode == 2) nw = 4;               // the E=128 pair-bias body: 4 waves per workgroup
    if (E >= 256) nw = 4;                            // E = 256: one form (it spills at the 256-register cap as it is)
    if (const int t = tune_get(kTuneFwdNW); t == 4 || t == 8) nw = t;
#ifdef NNOP_DEV_BUILD
    // QB = 2 with builtin MFMAs (experiment, make DEV=1): hipcc shuttles the score tiles between AGPRs and VGPRs
    // (~440 v_accvgpr moves per kv tile), 1.3x slower than QB = 1.  The shipped 64-row form is fa_fwd_w64.hpp.
    qb = dev_env_int("NNOP_FWD_QB", qb);
    if constexpr (sizeof(T) == 2 && E <= 64) {
        if (qb == 2 && mode == 0) return launch_fwd_cfg<T, E, 4, 0, 2>(d, a, s);
    }
#endif
    if constexpr (E < 256) {
        if (nw == 8) return mode == 0 ? launch_fwd_cfg<T, E, 8, 0, 1>(d, a, s) : mode == 1 ? launch_fwd_cfg<T, E, 8, 1, 1>(d, a, s) : launch_fwd_cfg<T, E, 8, 2, 1>(d, a, s);
    }
    return mode == 0 ? launch_fwd_cfg<T, E, 4, 0, 1>(d, a, s) : mode == 1 ? launch_fwd_cfg<T, E, 4, 1, 1>(d, a, s) : launch_fwd_cfg<T, E, 4, 2, 1>(d, a, s);
}

template <typename T> static int launch_fwd_generic(const nnop_fa_desc& d, const FwdArgs& a, hipStream_t s) {
    FwdParams p;
    fwd_params(p, d, a, 0);
    const long long n_rows = (long long)d.batch * d.qh * d.ql;
    const long long grid = (n_rows + 3) / 4;
    if (grid > 0x7fffffffLL) return NNOP_ERR_SHAPE;
    const bool sink = a.sinks != nullptr, cap = a.softcap != 0.f;
    const auto kern = cap ? (sink ? fa_fwd_generic_kernel<T, true, true> : fa_fwd_generic_kernel<T, false, true>)
                          : (sink ? fa_fwd_generic_kernel<T, true, false> : fa_fwd_generic_kernel<T, false, false>);
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(256), 0, s, p, d.emb, n_rows);
    return hipGetLastError() == hipSuccess ? NNOP_OK : NNOP_ERR_HIP;
}

template <typename T> int launch_fwd(const nnop_fa_desc& d, const FwdArgs& a, hipStream_t s) {
    // E = 256: 16-bit -- the 64-row form (two column halves), or the 32-row tiled kernel with 32-key tiles for what that form does not
    // take (pair bias, short / very long key axes).  fp32 -- the 32-row tiled kernel, 4 waves with the whole register file each (O^T
    // 128 + Q fragments 128 registers; K / V rings of 32-key tiles = 128 KiB of LDS); its BACKWARD does not fit and stays on fa_generic.hpp.
    if (d.emb == 256) return launch_fwd_e<T, 256>(d, a, s);
    if (emb_generic(d.emb)) return launch_fwd_generic<T>(d, a, s);
    switch (d.emb) {
        case 16:  return launch_fwd_e<T, 16>(d, a, s);
        case 32:  return launch_fwd_e<T, 32>(d, a, s);
        case 64:  return launch_fwd_e<T, 64>(d, a, s);
        case 128: return launch_fwd_e<T, 128>(d, a, s);
        default:  return NNOP_ERR_EMB_UNSUPPORTED;
    }
}

}  // namespace nnop
