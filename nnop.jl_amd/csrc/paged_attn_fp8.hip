// paged_attn_fp8.hip -- the kernels of libnnop_hip_paged_attn_fp8.so (include/nnop_hip_paged_attn_fp8.h): decode_attn_fp8.hip's
// attention of QL new tokens per sequence over one-byte E4M3 codes, with the cache kept as paged_attn.hip reads it: a pool of
// fixed-size pages and an int32 block table per sequence.
//
// What is decode_attn_fp8.hip's, statement for statement, so that the two calls give the same bits on the same codes: the work split
// (a workgroup is (sequence b, KV head, chunk c), four waves, tiles of 32 keys round-robin), the rows (R = G QL columns of one MFMA
// operand), the conversion (v_cvt_scalef32_pk_{bf16,f16}_fp8 at scale 1.0f), the scores (a key row's 16 bytes per lane straight from
// global memory, expanded into the A operand of v_mfma_f32_16x16x32), the one factor k_scale / sqrt(E), the online softmax in
// registers, P V through the wave-private LDS image of raw bytes (rows in image_row's order, row stride E + 16 bytes, read back with
// ds_read_b64_tr_b8), masking by selection, the merge of the waves and of the chunks in ascending order, the sink, v_scale and the dead
// rows.  The comments of decode_attn_fp8.hip explain those; they are not repeated here.
//
// What is paged_attn.hip's is where a key row lies: key j of sequence b is row j & (page_size - 1) of page
// table[b][j >> log2(page_size)].  page_size is a power of two >= 16, so a 16-key block of a tile lies in one page; a tile needs two
// table entries, the same for every lane of the wave, for K and for V.  The lookups are wave-uniform (readfirstlane on the wave index
// and on the entry, scalar arithmetic for the page offsets, which are bytes in 64 bits); a block index is clamped into
// [lo >> 4, (hi - 1) >> 4] in front of the lookup and a lane's key into [lo, hi - 1] -- NOT into [0, hi - 1] as the dense kernel
// does: a key in front of lo would name a page whose entry is not read -- so only entries of pages with a visible key are read and the
// clamped key lies in the block whose entry was fetched; every id is clamped into [0, num_pages - 1] before it forms an address.
// What the clamps duplicated is replaced at the consumer, so the clamp's lower end changes no bit.
//
// What is new is how the two meet.  The ring here holds four tiles per wave, not two, and entry -> address -> load is a dependent
// chain the dense kernel does not have.  Each of the four slots owns two registers for the entries of its NEXT refill.  They are
// fetched right behind the slot's previous refill, a whole loop iteration -- four consumes -- earlier:
//
//     consume(slot d)   waits for slot d's K and V data
//     load(slot d)      needs ids[d]: fetched right behind slot d's previous loads, so it arrived right behind the data just waited for
//     fetch(ids[d])     for the refill one iteration from here
//
// Vector loads return in order, so the refill's wait for its two entries counts down to what was issued behind them -- the loads and
// entries of the other three slots -- and leaves those in flight; with the refill itself, four tiles.  In front of the loop the chain
// is paid once: all eight entries first, then the slots in the loop's order (loads, then the next entries), so that the loop's first
// waits count what the later ones count.  Eight registers per wave beside the 252 of the dense kernel at E = 128.  The page's address
// is scalar and a lane's offset inside the page 32 bits (the C boundary checks that a page's rows lie within 2^32 bytes), so a load
// is global_load (scalar base, lane offset) and the lanes do no 64-bit multiplies: with per-lane 64-bit addresses the compiler's
// multiply-adds read register pairs whose upper half happened to be another slot's entry still in flight, and that false dependency
// drained a slot.  Staging the chunk's slice of the table in LDS was the other choice: it saves those eight registers, which are not short,
// and costs a copy loop per chunk with a barrier or a wave-private image, an LDS read and a readfirstlane per entry in the loop (the
// same dependent wait, now on the LDS counter that the V image's reads use), and either a bound on a chunk's length or a refill of the
// slice -- with 64 splits of 2^31 keys a chunk is a million tiles.  DESIGN.md section 4.22.
#include "paged_attn_fp8.hpp"
#include "host_common.hpp"

namespace nnop {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// the MFMA and the conversion of the two codes in the low (hi = false) or high half of w
template <typename T> struct Pf;
template <> struct Pf<__bf16> {
    typedef bf16x8 frag;
    typedef bf16x2 pair;
    static __device__ __forceinline__ f32x4 mma(frag a, frag b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
    template <bool HI> static __device__ __forceinline__ pair cvt(uint32_t w) { return __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)w, 1.0f, HI); }
};
template <> struct Pf<_Float16> {
    typedef f16x8 frag;
    typedef f16x2 pair;
    static __device__ __forceinline__ f32x4 mma(frag a, frag b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
    template <bool HI> static __device__ __forceinline__ pair cvt(uint32_t w) { return __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)w, 1.0f, HI); }
};

// eight codes, byte 0 of w0 first, as one operand
template <typename T> __device__ __forceinline__ typename Pf<T>::frag expand8(uint32_t w0, uint32_t w1) {
    const typename Pf<T>::pair a = Pf<T>::template cvt<false>(w0), b = Pf<T>::template cvt<true>(w0);
    const typename Pf<T>::pair c = Pf<T>::template cvt<false>(w1), d = Pf<T>::template cvt<true>(w1);
    return typename Pf<T>::frag{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}

struct PfParams {
    void* o;
    float* lse;
    const void* q;
    const uint8_t* k;
    const uint8_t* v;
    const float* k_scale;
    const float* v_scale;
    const int32_t* table;
    const int32_t* seqlens;
    const float* sinks;
    float* ws;
    long long ks_p, ks_h, vs_p, vs_h;  // bytes
    long long ts;                      // int32 entries between two rows of the table
    uint32_t ks_l, vs_l;               // bytes between two rows of a page: (page_size - 1) of them and a row fit in 32 bits
    int QL, G, KH, cap, window, splits, batch;
    int lg_page, num_pages;  // log2(page_size), pages of the pool
    float scale;             // 1 / sqrt(E)
};

constexpr float kNegInf = -__builtin_huge_valf();

// the (m, l) pairs lie behind the O rows of every (b, kvh, chunk, row)
__device__ __forceinline__ float* ws_ml(const PfParams& p, int E) {
    return p.ws + (size_t)p.batch * p.KH * p.splits * (p.G * p.QL) * (size_t)E;
}

// the image row of key `key` of a tile: key 16 h + 4 g + j -> 8 g + 4 h + j
__device__ __forceinline__ int image_row(int key) { return 8 * ((key >> 2) & 3) + 4 * (key >> 4) + (key & 3); }

template <typename T, int E>
__global__ __launch_bounds__(64 * kDaWaves) void paged_attn_fp8_kernel(const PfParams p) {
    typedef typename Pf<T>::frag frag;
    constexpr int ES = E / 32;              // E-steps of the scores
    constexpr int KL = E / 64;              // 16-byte loads of a lane per key block: each feeds two E-steps
    constexpr int ET = E / 16;              // 16-row blocks of O^T
    constexpr int RC = E / 16;              // 16-byte chunks of a row
    constexpr int VCH = kDaTile * RC / 64;  // V chunks of a lane per tile; the first half lies in the tile's first 16-key block
    constexpr int ROWB = E + 16;            // bytes between two rows of the V image: an odd number of 16-byte units
    constexpr int IMG = kDaTile * ROWB;
    constexpr int MERGE = kDaWaves * ET * 4 * 64 * 4 + 2 * kDaWaves * kDaRows * 4;
    // the wave-private V images; after the loop the same bytes carry the waves' (O, m, l) to wave 0, which needs more of them
    __shared__ __attribute__((aligned(16))) char smem[MERGE > kDaWaves * IMG ? MERGE : kDaWaves * IMG];
    // two passes of 16 rows at E = 64, four of 8 at E = 128: pass i lies in block i / (VCH / 2)
    static_assert((64 / RC) * (VCH / 2) == 16, "a V pass of a lane lies in one 16-key block");

    const int bid = blockIdx.x;
    const int c = bid % p.splits, kvh = (bid / p.splits) % p.KH, b = bid / (p.splits * p.KH);
    const int tid = threadIdx.x, lane = tid & 63, fm = lane & 15, fq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // uniform to the compiler: the tile index and the table address follow
    const int R = p.G * p.QL;
    const long long rowbase = ((long long)b * p.KH + kvh) * R;  // first of the R rows of q, o, lse

    const int hi = min(max(p.seqlens[b], 0), p.cap);
    const int lo = p.window < 0 ? 0 : max(0, hi - p.QL - p.window);  // the first key any query of the sequence sees
    const int t_lo = lo / kDaTile, t_hi = (hi + kDaTile - 1) / kDaTile;
    const int per = (t_hi - t_lo + p.splits - 1) / p.splits;
    const int t0 = t_lo + c * per, t1 = min(t_hi, t0 + per);
    const long long part = ((long long)b * p.KH + kvh) * p.splits + c;  // this chunk's place in the workspace

    if (t0 >= t1) {  // no tile: nothing of the table or the pool is read
        if (p.splits > 1) {
            if (tid < R) {
                float* ml = ws_ml(p, E) + (part * R + tid) * 2;
                ml[0] = kNegInf;
                ml[1] = 0.f;
            }
        } else {  // the sequence sees no key at all: o = +0, lse = the sink
            T* o = (T*)p.o + rowbase * E;
            for (int i = tid; i < R * E; i += 64 * kDaWaves) o[i] = (T)0.f;
            if (tid < R && p.lse) p.lse[rowbase + tid] = p.sinks ? p.sinks[kvh * p.G + tid / p.QL] : kNegInf;
        }
        return;
    }

    const float sc = (p.k_scale ? p.k_scale[kvh] : 1.f) * p.scale;  // the one factor of the scores

    // pin() as in decode_attn_fp8.hip: the refill of a slot stays between the work on two slots, and the image's reads and writes stay
    // in order.  Here it also keeps a slot's next table entries behind that slot's loads, so no K or V load of a refill is issued
    // behind a lookup of the same refill, and in front of the loop it keeps the order the loop's waits count on.
    auto pin = [] {
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
    };

    // the query row of this lane: where it stands and what it sees
    const bool row_ok = fm < R;
    const int ppos = hi - p.QL + fm % p.QL;
    const int row_lo = p.window < 0 ? 0 : ppos - p.window;
    frag qf[ES];
    {
        const T* qrow = (const T*)p.q + (rowbase + min(fm, R - 1)) * E + 16 * fq;
#pragma unroll
        for (int s = 0; s < ES; ++s) {
            const uint4 w = *reinterpret_cast<const uint4*>(qrow + 64 * (s >> 1) + 8 * (s & 1));
            qf[s] = __builtin_bit_cast(frag, row_ok ? w : uint4{0u, 0u, 0u, 0u});
        }
    }

    const uint8_t* kbase = p.k + kvh * p.ks_h;  // scalar: a lane's column, 16 fq or 16 (lane % RC), joins its row's offset
    const uint8_t* vbase = p.v + kvh * p.vs_h;
    const uint32_t kcol = 16 * fq, vcol = 16 * (lane % RC);
    const int vrow = lane / RC;  // V chunk i of the lane: key vrow + i (64 / RC) of the tile, 16-byte chunk lane % RC
    char* img = smem + wave * IMG;
    char* vst = img + 16 * (lane % RC);
    typedef __attribute__((address_space(3))) i32x2* lds_tr_p;
    const char* vld = img + (8 * fq + (fm >> 1)) * ROWB + 8 * (fm & 1);

    // ---- the address path ----
    const int32_t* tab = p.table + b * p.ts;
    const int blk_lo = lo >> 4, blk_hi = (hi - 1) >> 4;  // the 16-key blocks that hold a live key: hi >= 1 here
    const int row_mask = (1 << p.lg_page) - 1, blk_shift = p.lg_page - 4;
    struct Ids {
        int raw[2];  // the table entries of the two 16-key blocks of a tile, as they were read
    };
    // loads of live entries only, from uniform addresses; nothing here waits for what it fetched
    auto fetch = [&](Ids& s, int t) {
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) s.raw[kb] = tab[min(max(2 * t + kb, blk_lo), blk_hi) >> blk_shift];
    };

    struct Slot {
        uint4 k[2][KL];
        uint4 v[VCH];
    };
    Slot ring[kPfRing];
    Ids ids[kPfRing];
    // K and V loads only, from entries fetched a refill earlier: an id is clamped into the pool, then multiplied in 64 bits.  The page's
    // address is scalar; a lane adds its row's offset inside the page, which the C boundary has checked to fit in 32 bits, so a load
    // is (scalar base, 32-bit lane offset) and the lanes do no 64-bit arithmetic
    auto load = [&](Slot& s, const Ids& id, int t) {
        const uint8_t *kpage[2], *vpage[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            const int pg = min(max(__builtin_amdgcn_readfirstlane(id.raw[kb]), 0), p.num_pages - 1);
            kpage[kb] = kbase + pg * p.ks_p, vpage[kb] = vbase + pg * p.vs_p;
        }
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            const int key = max(min(kDaTile * t + 16 * kb + fm, hi - 1), lo);
            const uint32_t off = (uint32_t)(key & row_mask) * p.ks_l + kcol;
#pragma unroll
            for (int e = 0; e < KL; ++e) s.k[kb][e] = *reinterpret_cast<const uint4*>(kpage[kb] + (off + 64 * e));
        }
#pragma unroll
        for (int i = 0; i < VCH; ++i) {
            const int key = max(min(kDaTile * t + vrow + i * (64 / RC), hi - 1), lo);
            const uint32_t off = (uint32_t)(key & row_mask) * p.vs_l + vcol;
            s.v[i] = *reinterpret_cast<const uint4*>(vpage[i / (VCH / 2)] + off);
        }
    };

    float m_run = kNegInf, l_run = 0.f;
    f32x4 oacc[ET];
#pragma unroll
    for (int et = 0; et < ET; ++et) oacc[et] = f32x4{0.f, 0.f, 0.f, 0.f};

    auto consume = [&](const Slot& s, int t) {
        f32x4 sacc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int e = 0; e < KL; ++e)
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                const uint4 w = s.k[kb][e];
                sacc[kb] = Pf<T>::mma(expand8<T>(w.x, w.y), qf[2 * e], sacc[kb]);
                sacc[kb] = Pf<T>::mma(expand8<T>(w.z, w.w), qf[2 * e + 1], sacc[kb]);
            }
        // selection: the score of a key this row does not see is replaced, whatever it is
        float x[8], mx = kNegInf;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int key = kDaTile * t + 16 * (i >> 2) + 4 * fq + (i & 3);
            const bool ok = row_ok && key <= ppos && key >= row_lo;
            x[i] = ok ? sacc[i >> 2][i & 3] * sc : kNegInf;
            mx = fmaxf(mx, x[i]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float m_new = fmaxf(m_run, mx);
        const float m_ref = m_new == kNegInf ? 0.f : m_new;  // a row that has seen no key yet: every exponential below is exp(-inf) = 0
        const float alpha = __expf(m_run - m_ref);
        float ps = 0.f;
        frag pf;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float e = __expf(x[i] - m_ref);
            ps += e;
            pf[i] = (T)e;
        }
        ps += __shfl_xor(ps, 16);
        ps += __shfl_xor(ps, 32);
        l_run = l_run * alpha + ps;
        m_run = m_new;
#pragma unroll
        for (int et = 0; et < ET; ++et) oacc[et] *= alpha;
        // the V tile into the wave's image, its bytes as they are; a row no query of the sequence sees becomes zero bytes
#pragma unroll
        for (int i = 0; i < VCH; ++i) {
            const int rel = vrow + i * (64 / RC), key = kDaTile * t + rel;
            const bool ok = key >= lo && key < hi;
            *reinterpret_cast<uint4*>(vst + image_row(rel) * ROWB) = ok ? s.v[i] : uint4{0u, 0u, 0u, 0u};
        }
        asm volatile("" ::: "memory");
#pragma unroll
        for (int et = 0; et < ET; ++et) {
            const i32x2 a = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_tr_p)(vld + 16 * et));
            oacc[et] = Pf<T>::mma(expand8<T>((uint32_t)a[0], (uint32_t)a[1]), pf, oacc[et]);
        }
    };

    int t = t0 + wave;
#pragma unroll
    for (int d = 0; d < kPfRing; ++d) fetch(ids[d], t + d * kDaWaves);
    pin();  // the one place where loads wait for the table
    // in the loop's order -- a slot's loads, then its next entries -- so that the loop's first wait for an entry counts what the later
    // ones count
#pragma unroll
    for (int d = 0; d < kPfRing; ++d) {
        pin();
        load(ring[d], ids[d], t + d * kDaWaves);
        pin();
        fetch(ids[d], t + (kPfRing + d) * kDaWaves);
    }
    for (; t < t1; t += kPfRing * kDaWaves) {
#pragma unroll
        for (int d = 0; d < kPfRing; ++d) {
            pin();
            if (d == 0 || t + d * kDaWaves < t1) consume(ring[d], t + d * kDaWaves);
            pin();
            load(ring[d], ids[d], t + (kPfRing + d) * kDaWaves);
            pin();
            fetch(ids[d], t + (2 * kPfRing + d) * kDaWaves);  // for this slot's next refill, one iteration from here
        }
    }

    // ---- the four waves' (O, m, l) to wave 0, which sums them in ascending wave order ----
    float* mo = reinterpret_cast<float*>(smem);               // [wave][4 et + j][lane]
    float* mm = mo + kDaWaves * ET * 4 * 64;                  // [wave][row]
    float* ll = mm + kDaWaves * kDaRows;
    __syncthreads();  // every wave has left its image
#pragma unroll
    for (int et = 0; et < ET; ++et)
#pragma unroll
        for (int j = 0; j < 4; ++j) mo[((wave * ET + et) * 4 + j) * 64 + lane] = oacc[et][j];
    if (fq == 0) {
        mm[wave * kDaRows + fm] = m_run;
        ll[wave * kDaRows + fm] = l_run;
    }
    __syncthreads();
    if (wave != 0) return;

    float M = kNegInf;
#pragma unroll
    for (int w = 0; w < kDaWaves; ++w) M = fmaxf(M, mm[w * kDaRows + fm]);
    const float m_ref = M == kNegInf ? 0.f : M;
    float L = 0.f;
#pragma unroll
    for (int et = 0; et < ET; ++et) oacc[et] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int w = 0; w < kDaWaves; ++w) {
        const float a = __expf(mm[w * kDaRows + fm] - m_ref);  // a wave without a tile: exp(-inf) = 0 beside its zeros
        L += ll[w * kDaRows + fm] * a;
#pragma unroll
        for (int et = 0; et < ET; ++et)
#pragma unroll
            for (int j = 0; j < 4; ++j) oacc[et][j] += mo[((w * ET + et) * 4 + j) * 64 + lane] * a;
    }
    if (!row_ok) return;

    if (p.splits > 1) {
        float* orow = p.ws + (part * R + fm) * E + 4 * fq;
#pragma unroll
        for (int et = 0; et < ET; ++et)
#pragma unroll
            for (int j = 0; j < 4; ++j) orow[16 * et + j] = oacc[et][j];  // the workspace is promised to 4 bytes only
        if (fq == 0) {
            float* ml = ws_ml(p, E) + (part * R + fm) * 2;
            ml[0] = M;
            ml[1] = L;
        }
        return;
    }
    // one split: the sink joins as one more column, then divide, scale by v_scale, round, store
    const float sink = p.sinks ? p.sinks[kvh * p.G + fm / p.QL] : kNegInf;
    const float vs = p.v_scale ? p.v_scale[kvh] : 1.f;
    const float M2 = fmaxf(M, sink);
    const float m2_ref = M2 == kNegInf ? 0.f : M2;
    const float a = __expf(M - m2_ref);
    const float L2 = L * a + __expf(sink - m2_ref);
    const float inv = L2 > 0.f ? a / L2 : 0.f;
    T* orow = (T*)p.o + (rowbase + fm) * E + 4 * fq;
#pragma unroll
    for (int et = 0; et < ET; ++et) {
        typedef T t4 __attribute__((ext_vector_type(4)));
        t4 r;
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = (T)(oacc[et][j] * inv * vs);
        *reinterpret_cast<t4*>(orow + 16 * et) = r;
    }
    if (fq == 0 && p.lse) p.lse[rowbase + fm] = L2 > 0.f ? M2 + __logf(L2) : kNegInf;
}

// decode_attn_fp8_merge_kernel restated on PfParams: one wave per row of o, the chunks of the row in ascending order, a chunk that had
// no tile (m = -inf, l = 0, no O written) skipped by selection; v_scale joins after the division.
template <typename T, int E>
__global__ __launch_bounds__(64) void paged_attn_fp8_merge_kernel(const PfParams p) {
    const int R = p.G * p.QL;
    const long long row = blockIdx.x;                  // (b KH + kvh) R + r: the row of o and lse
    const long long bk = row / R;
    const int r = (int)(row % R), lane = threadIdx.x;
    const int kvh = (int)(bk % p.KH), h = kvh * p.G + r / p.QL;
    const float* ml = ws_ml(p, E);
    const float sink = p.sinks ? p.sinks[h] : kNegInf;
    const float vs = p.v_scale ? p.v_scale[kvh] : 1.f;
    float M = sink;
    for (int c = 0; c < p.splits; ++c) M = fmaxf(M, ml[((bk * p.splits + c) * R + r) * 2]);
    const float m_ref = M == kNegInf ? 0.f : M;
    float L = 0.f, acc[E / 64];
#pragma unroll
    for (int i = 0; i < E / 64; ++i) acc[i] = 0.f;
    for (int c = 0; c < p.splits; ++c) {
        const long long part = (bk * p.splits + c) * R + r;
        const float m = ml[part * 2], l = ml[part * 2 + 1];
        const bool live = m != kNegInf;
        const float a = __expf(m - m_ref);
        L += live ? l * a : 0.f;
#pragma unroll
        for (int i = 0; i < E / 64; ++i) {
            const float o = p.ws[part * E + lane + 64 * i];
            acc[i] += live ? o * a : 0.f;
        }
    }
    L += __expf(sink - m_ref);
    const float inv = L > 0.f ? 1.f / L : 0.f;
#pragma unroll
    for (int i = 0; i < E / 64; ++i) ((T*)p.o)[row * E + lane + 64 * i] = (T)(acc[i] * inv * vs);
    if (lane == 0 && p.lse) p.lse[row] = L > 0.f ? M + __logf(L) : kNegInf;
}

template <typename T, int E> int launch(const PfParams& p, hipStream_t s) {
    const int groups = p.batch * p.KH * p.splits;
    hipLaunchKernelGGL((paged_attn_fp8_kernel<T, E>), dim3(groups), dim3(64 * kDaWaves), 0, s, p);
    if (p.splits > 1)
        hipLaunchKernelGGL((paged_attn_fp8_merge_kernel<T, E>), dim3(p.batch * p.KH * p.G * p.QL), dim3(64), 0, s, p);
    return hipGetLastError() == hipSuccess ? (int)NNOP_OK : (int)NNOP_ERR_HIP;
}

}  // namespace

int launch_paged_attn_fp8(const nnop_paged_attn_fp8_desc& d, int splits, void* o, float* lse, const void* q, const void* k, const void* v,
                          const float* k_scale, const float* v_scale, const int32_t* block_table, const int32_t* seqlens,
                          const float* sinks, float* workspace, hipStream_t stream) {
    PfParams p;
    p.o = o, p.lse = lse, p.q = q, p.k = (const uint8_t*)k, p.v = (const uint8_t*)v, p.k_scale = k_scale, p.v_scale = v_scale;
    p.table = block_table, p.seqlens = seqlens, p.sinks = sinks, p.ws = workspace;
    p.ks_p = d.k_stride_p, p.ks_h = d.k_stride_h, p.ks_l = (uint32_t)d.k_stride_l;
    p.vs_p = d.v_stride_p, p.vs_h = d.v_stride_h, p.vs_l = (uint32_t)d.v_stride_l, p.ts = d.table_stride;
    p.QL = d.ql, p.G = d.qh / d.kh, p.KH = d.kh, p.cap = d.max_pages * d.page_size, p.splits = splits, p.batch = d.batch;
    p.lg_page = __builtin_ctz((unsigned)d.page_size), p.num_pages = d.num_pages;
    // a window that reaches past the table removes no key: it is no window, and `hi - QL - window` cannot wrap in the kernel
    p.window = d.window_left >= p.cap ? -1 : d.window_left;
    p.scale = d.emb == 64 ? 0.125f : 0.08838834764831845f;  // 1 / sqrt(E), rounded once
    if (d.dtype == NNOP_BF16) return d.emb == 64 ? launch<__bf16, 64>(p, stream) : launch<__bf16, 128>(p, stream);
    return d.emb == 64 ? launch<_Float16, 64>(p, stream) : launch<_Float16, 128>(p, stream);
}

}  // namespace nnop
