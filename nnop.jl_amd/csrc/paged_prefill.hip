// paged_prefill.hip -- the kernel of libnnop_hip_paged_prefill.so (include/nnop_hip_paged_prefill.h): attention of a variable number of
// new tokens per sequence over a KV cache kept as a pool of pages with an int32 block table per sequence.
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
//     that the other one has been read.  A thread moves E / 64 16-byte chunks of K and as many of V; each lies in one 16-key block, so
//     its table entry is wave-uniform.  The entries of tile t + 2 are fetched right behind the loads of tile t + 1 and wait in
//     registers for one tile: entry -> address -> load is off the loop's critical path (paged_attn.hip's fetch / load split).
//   - Images.  A K row is read by one lane as 16-byte pieces (ds_read_b128, the 32 lanes of a half-wave at 32 rows of one column): rows
//     2 E + 16 bytes apart put 16 rows in 16 different bank quads.  V is read through ds_read_b64_tr_b16, 4 rows of 64 contiguous bytes
//     per 32 lanes: rows 2 E + 64 bytes apart put those four runs of 16 banks side by side.
//   - Products on the 32x32x16 MFMA, scores transposed: S^T = K Q^T with K as the A operand and Q stationary in registers, so a query
//     row is an accumulator column: a lane holds 16 scores of one row, the lane 32 further the other 16, and the row's max and sum cost
//     one cross-lane step each.  Accumulator element 8 kk + j of half h is key 16 kk + 8 (j / 4) + 4 h + j % 4 of the tile; read as
//     slot 8 h + j of k-step kk it IS the B operand of O^T += V^T P^T, so P is rounded to T in registers and never touches LDS -- the V^T
//     operand is gathered in that key order instead, which is two transposing reads of four keys each.
//   - Softmax in the base-2 domain: one fma and one v_exp_f32 per score (scale log2(e) folded in), fp32 throughout, O rescaled only
//     when some row's max moved.  The sink joins in the epilogue as one more column; a row without a key gives +0 and its sink.
#include <type_traits>
#include "paged_prefill.hpp"
#include "host_common.hpp"

namespace nnop {
namespace {

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
    long long ks_p, ks_h, ks_l, vs_p, vs_h, vs_l, ts, qs_t, qs_h, os_t, os_h;  // elements; ts: int32 entries between two rows of the table
    int T, QH, G, KH, TB, batch, cap, window;
    int lg_page, num_pages;  // log2(page_size), pages of the pool
    float scale2;            // log2(e) / sqrt(E)
};

constexpr float kNegInf = -__builtin_huge_valf();
constexpr float kLog2e = 1.4426950408889634f, kLn2 = 0.6931471805599453f;
constexpr int kThreads = 64 * kPpWaves;

template <typename T, int E>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(2, 2))) void paged_prefill_kernel(const PpParams p) {
    typedef typename Pp<T>::frag frag;
    constexpr int ES = E / 16;            // k-steps of the scores
    constexpr int ET = E / 32;            // 32-row blocks of O^T
    constexpr int RC = E / 8;             // 16-byte chunks of a row
    constexpr int CH = kPpTile * RC / kThreads;  // chunks of K, and of V, that a thread moves per tile
    constexpr int KROWB = 2 * E + 16, VROWB = 2 * E + 64;  // bytes between two rows of the K and of the V image
    constexpr int KIMG = kPpTile * KROWB, VIMG = kPpTile * VROWB;
    static_assert(CH == E / 64 && (kThreads / RC) * CH == kPpTile, "a thread's chunk i lies in one 16-key block of the tile");
    __shared__ __attribute__((aligned(16))) char kimg[2 * KIMG];
    __shared__ __attribute__((aligned(16))) char vimg[2 * VIMG];

    const int tid = threadIdx.x, lane = tid & 63, fn = lane & 31, fh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // uniform to the compiler: the table address follows
    const int kvh = blockIdx.x % p.KH, slot = blockIdx.x / p.KH;
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
    const int t_lo = lo / kPpTile, t_hi = p_last >= 0 ? p_last / kPpTile : -1;  // inclusive; none if every row stands below 0

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
    const int crow = tid / RC, ccol = tid % RC;  // chunk i of the thread: row crow + i (kThreads / RC) of the tile, 16-byte chunk ccol
    const T* kbase = (const T*)p.k + kvh * p.ks_h + 8 * ccol;
    const T* vbase = (const T*)p.v + kvh * p.vs_h + 8 * ccol;
    auto chunk_blk = [&](int i) { return E == 64 ? wave >> 1 : i; };  // the 16-key block of the tile that chunk i lies in: uniform
    int ids[CH];
    u32x4 kreg[CH], vreg[CH];
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
            kreg[i] = *reinterpret_cast<const u32x4*>(kbase + pg * p.ks_p + (key & row_mask) * p.ks_l);
            vreg[i] = *reinterpret_cast<const u32x4*>(vbase + pg * p.vs_p + (key & row_mask) * p.vs_l);
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int row = crow + i * (kThreads / RC);
            *reinterpret_cast<u32x4*>(kimg + buf * KIMG + row * KROWB + 16 * ccol) = kreg[i];
            *reinterpret_cast<u32x4*>(vimg + buf * VIMG + row * VROWB + 16 * ccol) = vreg[i];
        }
    };

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
        const float m_new = fmaxf(m_run, mx * p.scale2);
        const float m_ref = m_new == kNegInf ? 0.f : m_new;  // a row that has seen no key yet: every exponential below is 2^-inf = 0
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_ref);
        float ps = 0.f;
        frag pf[2];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float e = __builtin_amdgcn_exp2f(__builtin_fmaf(s[i], p.scale2, -m_ref));
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

    // the sink joins as one more column, then divide, round once, store
    const float sink_e = p.sinks ? p.sinks[head] : kNegInf, sink = sink_e * kLog2e;
    const float M2 = fmaxf(m_run, sink);
    const float m2_ref = M2 == kNegInf ? 0.f : M2;
    const float a = __builtin_amdgcn_exp2f(m_run - m2_ref);
    const float L2 = l_run * a + __builtin_amdgcn_exp2f(sink - m2_ref);
    const float inv = L2 > 0.f ? a / L2 : 0.f;
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

template <typename T, int E> int launch(const PpParams& p, long long groups, hipStream_t s) {
    hipLaunchKernelGGL((paged_prefill_kernel<T, E>), dim3((unsigned)groups), dim3(kThreads), 0, s, p);
    return hipGetLastError() == hipSuccess ? (int)NNOP_OK : (int)NNOP_ERR_HIP;
}

}  // namespace

int launch_paged_prefill(const nnop_paged_prefill_desc& d, void* o, float* lse, const void* q, const void* k, const void* v,
                         const int32_t* block_table, const int32_t* cu_seqlens_q, const int32_t* seqlens, const float* sinks,
                         hipStream_t stream) {
    PpParams p;
    p.o = o, p.lse = lse, p.q = q, p.k = k, p.v = v, p.table = block_table, p.cu = cu_seqlens_q, p.seqlens = seqlens, p.sinks = sinks;
    p.ks_p = d.k_stride_p, p.ks_h = d.k_stride_h, p.ks_l = d.k_stride_l;
    p.vs_p = d.v_stride_p, p.vs_h = d.v_stride_h, p.vs_l = d.v_stride_l, p.ts = d.table_stride;
    p.qs_t = d.q_stride_t, p.qs_h = d.q_stride_h, p.os_t = d.o_stride_t, p.os_h = d.o_stride_h;
    p.T = d.tokens, p.QH = d.qh, p.G = d.qh / d.kh, p.KH = d.kh, p.TB = paged_prefill_block_tokens(d), p.batch = d.batch;
    p.cap = (int)((long long)d.max_pages * d.page_size);
    p.lg_page = __builtin_ctz((unsigned)d.page_size), p.num_pages = d.num_pages;
    // a window that reaches past the table removes no key: it is no window, and `position - window` cannot wrap in the kernel
    p.window = d.window_left >= p.cap ? -1 : d.window_left;
    p.scale2 = d.emb == 64 ? 0.18033688011112042f : 0.12751743082459868f;  // log2(e) / sqrt(E), rounded once
    const long long groups = d.kh * paged_prefill_max_blocks(d);
    if (d.dtype == NNOP_BF16) return d.emb == 64 ? launch<__bf16, 64>(p, groups, stream) : launch<__bf16, 128>(p, groups, stream);
    return d.emb == 64 ? launch<_Float16, 64>(p, groups, stream) : launch<_Float16, 128>(p, groups, stream);
}

}  // namespace nnop
