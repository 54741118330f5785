// paged_prefill_kernel.hpp -- the kernel body of prefill attention over a paged KV cache, shared header-only (nothing is linked) by
// libnnop_hip_paged_prefill.so (paged_prefill.hip: 16-bit pages) and libnnop_hip_paged_prefill_fp8.so (paged_prefill_fp8.hip: pages of
// E4M3 codes).  The two differ in ONE place, the staging of a tile -- what a thread loads from a page row and what it writes into the
// LDS image -- which is the `Stage` policy below; the work split, the address path, the images and everything that reads them are one
// text.
//
// Decode (paged_attn.hip) is bandwidth-bound: it streams K into operand registers per wave and shares nothing.  Prefill is matrix-bound:
// a K/V tile is used by every row of a workgroup, so it goes through LDS.  Of paged_attn.hip only the address rule is kept -- key j of
// sequence b is row j & (page_size - 1) of page table[b][j >> log2(page_size)], a 16-key block lies in one page, its entry is
// wave-uniform, clamped into the live blocks in front of the lookup and into the pool behind it.
//
//   - Work.  A workgroup is (sequence b, KV head, block of TB = 128 / G tokens of b); its 128 rows are those tokens times the G query
//     heads of the KV head (row r: token r / G, head r % G), 32 per wave, so a tile is fetched once for all G heads.  128 - TB G rows
//     and the rows behind a sequence's last token are dead: their Q is zero, their scores are replaced, nothing of them is stored.
//     The grid is KH (T / TB + B), the host's bound of sum_b ceil(n_b / TB).  Each wave finds the block of its workgroup's slot by a
//     scan over cu_seqlens_q -- 64 sequences per step, one per lane, an inclusive prefix through six shuffles and one ballot -- so no
//     list, no workspace and no kernel in front.  Slots behind the last block exit.  A sequence's blocks are issued last one first:
//     it has the longest key range.
//   - Keys of a block.  Tiles of 32 keys from lo / 32, lo = max(0, p_first - window) or 0, to the tile of p_last; nothing else is
//     touched.  A wave skips the products of a tile none of its rows sees, and only a tile that the diagonal or the window's edge cuts
//     FOR THAT WAVE takes the loop body with the per-score selection.
//   - Tile movement.  global -> registers -> LDS, two images of K and of V.  The loads of tile t + 1 are issued in front of the
//     products of tile t and stored behind them into the other image; one barrier per tile then says both that the image is whole and
//     that the other one has been read.  A thread moves Stage::CH pieces of a K row and as many of V; each lies in one 16-key block, so
//     its table entry is wave-uniform.  The entries of tile t + 2 are fetched right behind the loads of tile t + 1 and wait in
//     registers for one tile: entry -> address -> load is off the loop's critical path (paged_attn.hip's fetch / load split).
//   - Images.  Always 16-bit elements of T, whatever the pages hold.  A K row is read by one lane as 16-byte pieces (ds_read_b128, the
//     32 lanes of a half-wave at 32 rows of one column): rows 2 E + 16 bytes apart put 16 rows in 16 different bank quads.  V is read
//     through ds_read_b64_tr_b16, 4 rows of 64 contiguous bytes per 32 lanes: rows 2 E + 64 bytes apart put those four runs of 16 banks
//     side by side.
//   - Products on the 32x32x16 MFMA, scores transposed: S^T = K Q^T with K as the A operand and Q stationary in registers, so a query
//     row is an accumulator column: a lane holds 16 scores of one row, the lane 32 further the other 16, and the row's max and sum cost
//     one cross-lane step each.  Accumulator element 8 kk + j of half h is key 16 kk + 8 (j / 4) + 4 h + j % 4 of the tile; read as
//     slot 8 h + j of k-step kk it IS the B operand of O^T += V^T P^T, so P is rounded to T in registers and never touches LDS -- the V^T
//     operand is gathered in that key order instead, which is two transposing reads of four keys each.
//   - Softmax in the base-2 domain: one fma and one v_exp_f32 per score (scale log2(e) folded in), fp32 throughout, O rescaled only
//     when some row's max moved.  The sink joins in the epilogue as one more column; a row without a key gives +0 and its sink.
//
// A Stage names: Params (PpParams or a struct derived from it); elem, the type the pool's strides count; RC, the pieces of a page row
// (thread tid holds piece tid % RC of row tid / RC, and of the rows kThreads / RC further); CH, the pieces of K, and of V, a thread
// moves per tile; COLS, the elements of a piece; reg, the registers that hold one from its load to its store; load(); store(), which
// writes the piece's 2 COLS bytes of the image; scale2(), the factor of the scores; out_factor(), the factor of the epilogue.
//
// A Part names which of a block's key tiles a workgroup walks and what it leaves behind.  PpWhole, the default: all of them, and the
// finished rows (sink, division, one rounding) in o and lse.  PpChunk (libnnop_hip_paged_prefill_split.so, paged_prefill_split.hip):
// the workgroups of a block are `splits` in number, chunk c = blockIdx.x % splits walks tiles t_lo + c per ... of the block's
// t_lo ... t_hi, per = ceil(n / splits), and every live row leaves its fp32 un-normalised O and its (m, l) of the base-2 domain in a
// workspace for a merge kernel.  A Part has: kPartial; group(), the (slot, KV head) index of the workgroup; first() and last(), the
// tile range; finish(), the partial epilogue (never called when kPartial is false).
#pragma once
#include <type_traits>
#include "paged_prefill.hpp"

namespace nnop {
namespace {  // a kernel's text, included by the one kernel file of a library: internal to it, as it was in paged_prefill.hip

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

template <typename T> struct Pp;
template <> struct Pp<__bf16> {
    typedef bf16x8 frag;
    static __device__ __forceinline__ f32x16 mma(frag a, frag b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};
template <> struct Pp<_Float16> {
    typedef f16x8 frag;
    static __device__ __forceinline__ f32x16 mma(frag a, frag b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
};

struct PpParams {
    void* o;
    float* lse;
    const void* q;
    const void* k;
    const void* v;
    const int32_t* table;
    const int32_t* cu;
    const int32_t* seqlens;
    const float* sinks;
    // q and o: elements; the pools: Stage::elem; ts: int32 entries between two rows of the table
    long long ks_p, ks_h, ks_l, vs_p, vs_h, vs_l, ts, qs_t, qs_h, os_t, os_h;
    int T, QH, G, KH, TB, batch, cap, window;
    int lg_page, num_pages;  // log2(page_size), pages of the pool
    float scale2;            // log2(e) / sqrt(E)
};

constexpr float kPpNegInf = -__builtin_huge_valf();
constexpr float kPpLog2e = 1.4426950408889634f, kPpLn2 = 0.6931471805599453f;
constexpr int kPpThreads = 64 * kPpWaves;

// 16-bit pages: a piece is 16 bytes of a row and goes into the image as it is
template <typename T, int E> struct PpStage16 {
    typedef PpParams Params;
    typedef T elem;
    typedef u32x4 reg;
    static constexpr int RC = E / 8, CH = kPpTile * RC / kPpThreads, COLS = 8;
    static __device__ __forceinline__ reg load(const elem* at) { return *reinterpret_cast<const u32x4*>(at); }
    static __device__ __forceinline__ void store(char* at, reg r) { *reinterpret_cast<u32x4*>(at) = r; }
    static __device__ __forceinline__ float scale2(const Params& p, int) { return p.scale2; }
    static __device__ __forceinline__ float out_factor(float inv, const Params&, int) { return inv; }
};

// every tile of the block; the epilogue below finishes the rows
struct PpWhole {
    static constexpr bool kPartial = false;
    __device__ __forceinline__ unsigned group(unsigned block) const { return block; }
    __device__ __forceinline__ int first(int t_lo, int) const { return t_lo; }
    __device__ __forceinline__ int last(int, int t_hi) const { return t_hi; }
    template <int E, typename Acc>
    __device__ __forceinline__ void finish(const Acc*, float, float, long long, int, int, int) const {}
};

// chunk blockIdx.x % splits of the block's tiles; o_part [splits][T][QH][E] and ml_part [splits][T][QH][2] fp32 behind it, so that the
// 16-byte stores of a lane's four consecutive columns stay aligned
struct PpChunk {
    static constexpr bool kPartial = true;
    float* o_part;
    float* ml_part;
    int splits;
    __device__ __forceinline__ int chunk() const { return blockIdx.x % splits; }
    __device__ __forceinline__ unsigned group(unsigned block) const { return block / splits; }
    __device__ __forceinline__ int per(int t_lo, int t_hi) const { return (max(t_hi - t_lo + 1, 0) + splits - 1) / splits; }
    __device__ __forceinline__ int first(int t_lo, int t_hi) const { return t_lo + chunk() * per(t_lo, t_hi); }
    // behind the block's last tile, or with per = 0, the chunk has no tile: last() < first()
    __device__ __forceinline__ int last(int t_lo, int t_hi) const { return min(first(t_lo, t_hi) + per(t_lo, t_hi) - 1, t_hi); }
    // A live row's (m, l), and its O unless it saw no key in the chunk (m = -inf, l = 0): the merge selects such a chunk out by its l
    // and never reads that O.  Accumulator element 4 j + c of block et is column 32 et + 8 j + 4 fh + c, as in the epilogue below.
    template <int E, typename Acc>
    __device__ __forceinline__ void finish(const Acc* oacc, float m_run, float l_run, long long tok, int T, int QH, int head) const {
        const int fh = (threadIdx.x & 63) >> 5;
        const long long row = ((long long)chunk() * T + tok) * QH + head;
        if (fh == 0) *reinterpret_cast<float2*>(ml_part + 2 * row) = float2{m_run, l_run};
        if (!(l_run > 0.f)) return;
        float* orow = o_part + row * E + 4 * fh;
#pragma unroll
        for (int et = 0; et < E / 32; ++et)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                *reinterpret_cast<float4*>(orow + 32 * et + 8 * j) =
                    float4{oacc[et][4 * j], oacc[et][4 * j + 1], oacc[et][4 * j + 2], oacc[et][4 * j + 3]};
    }
};

template <typename T, int E, typename Stage, typename Part = PpWhole>
__device__ __forceinline__ void paged_prefill_body(const typename Stage::Params& p, const Part part = Part{}) {
    typedef typename Pp<T>::frag frag;
    typedef typename Stage::elem elem;
    constexpr float kNegInf = kPpNegInf, kLog2e = kPpLog2e, kLn2 = kPpLn2;
    constexpr int kThreads = kPpThreads;
    constexpr int ES = E / 16;            // k-steps of the scores
    constexpr int ET = E / 32;            // 32-row blocks of O^T
    constexpr int RC = Stage::RC;         // pieces of a row
    constexpr int CH = Stage::CH;         // pieces of K, and of V, that a thread moves per tile
    constexpr int PB = 2 * Stage::COLS;   // bytes of a piece in the image
    constexpr int KROWB = 2 * E + 16, VROWB = 2 * E + 64;  // bytes between two rows of the K and of the V image
    constexpr int KIMG = kPpTile * KROWB, VIMG = kPpTile * VROWB;
    static_assert(RC * Stage::COLS == E && CH * kThreads == kPpTile * RC, "the threads' pieces are the tile");
    static_assert((RC == 8 && CH == 1) || (RC == 16 && CH == 2), "a thread's piece i lies in one 16-key block of the tile");
    __shared__ __attribute__((aligned(16))) char kimg[2 * KIMG];
    __shared__ __attribute__((aligned(16))) char vimg[2 * VIMG];

    const int tid = threadIdx.x, lane = tid & 63, fn = lane & 31, fh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // uniform to the compiler: the table address follows
    const unsigned group = part.group(blockIdx.x);
    const int kvh = group % p.KH, slot = group / p.KH;
    auto cu_at = [&](int i) { return min(max(p.cu[i], 0), p.T); };

    // ---- which block: the first sequence whose inclusive count of blocks exceeds the slot ----
    int b = -1, first = 0, blocks = 0;
    for (int b0 = 0, base = 0; b0 < p.batch; b0 += 64) {
        const int bb = min(b0 + lane, p.batch - 1);
        const int cnt = b0 + lane < p.batch ? (max(cu_at(bb + 1) - cu_at(bb), 0) + p.TB - 1) / p.TB : 0;
        int incl = cnt;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d);
            incl += lane >= d ? up : 0;
        }
        incl += base;
        const unsigned long long hit = __ballot(slot < incl);
        if (hit) {  // the first lane whose count passes the slot has a block: its own count moved the sum
            const int l = __builtin_ctzll(hit);
            b = b0 + l, blocks = __shfl(cnt, l), first = __shfl(incl, l) - blocks;
            break;
        }
        base = __shfl(incl, 63);
    }
    if (b < 0) return;  // a surplus workgroup, all of it
    b = __builtin_amdgcn_readfirstlane(b);
    const int blk = __builtin_amdgcn_readfirstlane(blocks - 1 - (slot - first));  // the last block of a sequence first
    const int q0 = cu_at(b), nb = max(cu_at(b + 1) - q0, 0);
    const int tok0 = blk * p.TB, ntok = min(p.TB, nb - tok0);  // >= 1
    const int hi = min(max(p.seqlens[b], 0), p.cap);
    const int pos0 = hi - nb + tok0;                           // where the block's first token stands; below 0 if seqlens[b] < n_b
    const int p_last = pos0 + ntok - 1;
    const int seq_lo = p.window < 0 ? 0 : max(0, max(hi - nb, 0) - p.window);  // the first key any query of the sequence sees
    const int lo = p.window < 0 ? 0 : max(0, max(pos0, 0) - p.window);
    const int blk_t_lo = lo / kPpTile, blk_t_hi = p_last >= 0 ? p_last / kPpTile : -1;  // inclusive; none if every row stands below 0
    const int t_lo = part.first(blk_t_lo, blk_t_hi), t_hi = part.last(blk_t_lo, blk_t_hi);  // what this workgroup walks of them

    // the query row of this lane, and what the wave's rows see between them
    const int r = 32 * wave + fn, rtok = r / p.G, rg = r - rtok * p.G;
    const bool row_ok = rtok < ntok;
    const int ppos = pos0 + rtok;
    const int row_lo = p.window < 0 ? 0 : max(ppos, 0) - p.window;
    const int live = ntok * p.G;  // rows of the block with a token
    const bool wave_ok = 32 * wave < live;
    const int pmin = pos0 + 32 * wave / p.G, pmax = pos0 + (min(32 * wave + 31, live - 1)) / p.G;
    const long long tok = q0 + tok0 + min(rtok, ntok - 1);
    const int head = kvh * p.G + rg;
    frag qf[ES];
    {
        const T* qrow = (const T*)p.q + tok * p.qs_t + head * p.qs_h + 8 * fh;
#pragma unroll
        for (int s = 0; s < ES; ++s) {
            const uint4 w = *reinterpret_cast<const uint4*>(qrow + 16 * s);
            qf[s] = __builtin_bit_cast(frag, row_ok ? w : uint4{0u, 0u, 0u, 0u});
        }
    }

    // ---- the address path ----
    const int32_t* tab = p.table + b * p.ts;
    const int blk_lo = seq_lo >> 4, blk_hi = (max(hi, 1) - 1) >> 4;  // the 16-key blocks that hold a live key
    const int row_mask = (1 << p.lg_page) - 1, blk_shift = p.lg_page - 4;
    const int crow = tid / RC, ccol = tid % RC;  // piece i of the thread: row crow + i (kThreads / RC) of the tile, piece ccol of the row
    const elem* kbase = (const elem*)p.k + kvh * p.ks_h + Stage::COLS * ccol;
    const elem* vbase = (const elem*)p.v + kvh * p.vs_h + Stage::COLS * ccol;
    auto chunk_blk = [&](int i) { return RC == 8 ? wave >> 1 : i; };  // the 16-key block of the tile that piece i lies in: uniform
    int ids[CH];
    typename Stage::reg kreg[CH], vreg[CH];
    // loads of live entries only, from uniform addresses; nothing here waits for what it fetched
    auto fetch = [&](int t) {
#pragma unroll
        for (int i = 0; i < CH; ++i) ids[i] = tab[min(max(2 * t + chunk_blk(i), blk_lo), blk_hi) >> blk_shift];
    };
    // K and V loads only, from entries fetched a tile earlier: an id is clamped into the pool, then multiplied in 64 bits
    auto load = [&](int t) {
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const long long pg = min(max(__builtin_amdgcn_readfirstlane(ids[i]), 0), p.num_pages - 1);
            const int key = max(min(kPpTile * t + crow + i * (kThreads / RC), hi - 1), seq_lo);
            kreg[i] = Stage::load(kbase + pg * p.ks_p + (key & row_mask) * p.ks_l);
            vreg[i] = Stage::load(vbase + pg * p.vs_p + (key & row_mask) * p.vs_l);
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int row = crow + i * (kThreads / RC);
            Stage::store(kimg + buf * KIMG + row * KROWB + PB * ccol, kreg[i]);
            Stage::store(vimg + buf * VIMG + row * VROWB + PB * ccol, vreg[i]);
        }
    };

    const float scale2 = Stage::scale2(p, kvh);  // the one factor of the scores
    float m_run = kNegInf, l_run = 0.f;  // base-2 domain
    f32x16 oacc[ET];
#pragma unroll
    for (int et = 0; et < ET; ++et)
#pragma unroll
        for (int i = 0; i < 16; ++i) oacc[et][i] = 0.f;

    typedef __attribute__((address_space(3))) s16x4* lds_tr_p;
    const char* kld = kimg + fn * KROWB + 16 * fh;
    // a group of 16 lanes reads 4 keys x 16 columns and gets them transposed: lane i of it addresses key i / 4, columns 4 (i % 4) ...
    const char* vld = vimg + (4 * fh + ((lane & 15) >> 2)) * VROWB + 2 * (16 * ((lane >> 4) & 1) + 4 * (lane & 3));

    auto consume = [&](int buf, int t, auto cut) {
        f32x16 s;
#pragma unroll
        for (int i = 0; i < 16; ++i) s[i] = 0.f;
#pragma unroll
        for (int e = 0; e < ES; ++e) {
            s = Pp<T>::mma(__builtin_bit_cast(frag, *reinterpret_cast<const uint4*>(kld + buf * KIMG + 32 * e)), qf[e], s);
            if (e % 4 == 3) __builtin_amdgcn_sched_barrier(0);  // four K operands at a time: the register budget of two waves per SIMD
        }
        // selection: the score of a key this row does not see is replaced, whatever it is
        float mx = kNegInf;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if (cut.value) {
                const int key = kPpTile * t + 8 * (i >> 2) + 4 * fh + (i & 3);
                s[i] = row_ok && key <= ppos && key >= row_lo ? s[i] : kNegInf;
            }
            mx = fmaxf(mx, s[i]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float m_new = fmaxf(m_run, mx * scale2);
        const float m_ref = m_new == kNegInf ? 0.f : m_new;  // a row that has seen no key yet: every exponential below is 2^-inf = 0
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_ref);
        float ps = 0.f;
        frag pf[2];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float e = __builtin_amdgcn_exp2f(__builtin_fmaf(s[i], scale2, -m_ref));
            ps += e;
            pf[i >> 3][i & 7] = (T)e;
        }
        ps += __shfl_xor(ps, 32);
        l_run = l_run * alpha + ps;
        m_run = m_new;
        if (__ballot(alpha != 1.f)) {
#pragma unroll
            for (int et = 0; et < ET; ++et) oacc[et] *= alpha;
        }
#pragma unroll
        for (int et = 0; et < ET; ++et) {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const char* at = vld + buf * VIMG + 16 * kk * VROWB + 64 * et;
                const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr_p)at);
                const s16x4 d = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr_p)(at + 8 * VROWB));
                const s16x8 vf = {a[0], a[1], a[2], a[3], d[0], d[1], d[2], d[3]};
                oacc[et] = Pp<T>::mma(__builtin_bit_cast(frag, vf), pf[kk], oacc[et]);
            }
            if (et % 2 == 1) __builtin_amdgcn_sched_barrier(0);  // the V operands of two blocks at a time: the register budget of two waves per SIMD
        }
    };

    // the loads of a tile stay in front of the products of the tile before it, its stores behind them
    auto pin = [] {
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
    };
    if (t_lo <= t_hi) {
        fetch(t_lo);
        load(t_lo);  // the one place where loads wait for the table
        pin();
        if (t_lo < t_hi) fetch(t_lo + 1);
        store(0);
        __syncthreads();
    }
    for (int t = t_lo; t <= t_hi; ++t) {
        const int buf = (t - t_lo) & 1;
        if (t < t_hi) load(t + 1);
        pin();
        if (t + 1 < t_hi) fetch(t + 2);
        pin();
        const int k0 = kPpTile * t;
        const bool unseen = !wave_ok || k0 > pmax || (p.window >= 0 && k0 + kPpTile - 1 < max(pmin, 0) - p.window);
        const bool whole = k0 + kPpTile - 1 <= pmin && (p.window < 0 || k0 >= pmax - p.window);
        if (!unseen) {
            if (whole)
                consume(buf, t, std::false_type{});
            else
                consume(buf, t, std::true_type{});
        }
        pin();
        if (t < t_hi) store(buf ^ 1);
        __syncthreads();  // the other image is whole, and this one has been read by every wave
    }
    if (!row_ok) return;
    if constexpr (Part::kPartial) {
        part.template finish<E>(oacc, m_run, l_run, tok, p.T, p.QH, head);
        return;
    }

    // the sink joins as one more column, then divide, round once, store
    const float sink_e = p.sinks ? p.sinks[head] : kNegInf, sink = sink_e * kLog2e;
    const float M2 = fmaxf(m_run, sink);
    const float m2_ref = M2 == kNegInf ? 0.f : M2;
    const float a = __builtin_amdgcn_exp2f(m_run - m2_ref);
    const float L2 = l_run * a + __builtin_amdgcn_exp2f(sink - m2_ref);
    const float inv = Stage::out_factor(L2 > 0.f ? a / L2 : 0.f, p, kvh);
    T* orow = (T*)p.o + tok * p.os_t + head * p.os_h + 4 * fh;
#pragma unroll
    for (int et = 0; et < ET; ++et)
#pragma unroll
        for (int j = 0; j < 4; ++j) {  // accumulator element 4 j + c of block et: column 32 et + 8 j + 4 h + c of o
            typedef T t4 __attribute__((ext_vector_type(4)));
            t4 w;
#pragma unroll
            for (int c = 0; c < 4; ++c) w[c] = (T)(oacc[et][4 * j + c] * inv);
            *reinterpret_cast<t4*>(orow + 32 * et + 8 * j) = w;
        }
    // a row without a key has its sink for lse, bit for bit: the way through base 2 and back would round it
    if (fh == 0 && p.lse) p.lse[tok * p.QH + head] = m_run == kNegInf ? sink_e : (M2 + __log2f(L2)) * kLn2;
}

// what launch_paged_prefill and launch_paged_prefill_fp8 fill alike from a descriptor that has passed its checks (D: either one)
template <typename D> static inline void paged_prefill_fill(PpParams& p, const D& d) {
    p.ks_p = d.k_stride_p, p.ks_h = d.k_stride_h, p.ks_l = d.k_stride_l;
    p.vs_p = d.v_stride_p, p.vs_h = d.v_stride_h, p.vs_l = d.v_stride_l, p.ts = d.table_stride;
    p.qs_t = d.q_stride_t, p.qs_h = d.q_stride_h, p.os_t = d.o_stride_t, p.os_h = d.o_stride_h;
    p.T = d.tokens, p.QH = d.qh, p.G = d.qh / d.kh, p.KH = d.kh, p.TB = paged_prefill_block_tokens(d), p.batch = d.batch;
    p.cap = (int)((long long)d.max_pages * d.page_size);
    p.lg_page = __builtin_ctz((unsigned)d.page_size), p.num_pages = d.num_pages;
    // a window that reaches past the table removes no key: it is no window, and `position - window` cannot wrap in the kernel
    p.window = d.window_left >= p.cap ? -1 : d.window_left;
    p.scale2 = d.emb == 64 ? 0.18033688011112042f : 0.12751743082459868f;  // log2(e) / sqrt(E), rounded once
}

}  // namespace
}  // namespace nnop
