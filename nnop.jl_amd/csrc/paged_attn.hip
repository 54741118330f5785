// paged_attn.hip -- the kernels of libnnop_hip_paged_attn.so (include/nnop_hip_paged_attn.h): decode_attn.hip's attention of QL new tokens
// per sequence, over a KV cache kept as a pool of fixed-size pages with an int32 block table per sequence.
//
// What is decode_attn.hip's, statement for statement, so that the two calls give the same bits on the same keys: the work split (a
// workgroup is (sequence b, KV head, chunk c), four waves, tiles of 32 keys round-robin), the rows (R = G QL columns of one MFMA operand),
// the scores (K rows straight from global memory into the A operand), the online softmax in registers, P V through the wave-private LDS
// image and ds_read_b64_tr_b16, masking by selection, the merge of the waves and of the chunks in ascending order, the sink, the dead
// rows.  The comments of decode_attn.hip explain those; they are not repeated here.
//
// What is new is where a key row lies.  Key j of sequence b is row j & (page_size - 1) of page table[b][j >> log2(page_size)] of the
// pool.  page_size is a power of two >= 16, so a 16-key block of a tile lies in one page: a tile needs two table entries, and they are
// the same for every lane of the wave, for K and for V.
//
//   - The lookups are wave-uniform.  The wave index goes through readfirstlane, b comes from blockIdx and [lo, hi) from seqlens[b], so
//     the tile index, the block index and the table address are uniform: one request per entry and wave.  In front of the loop the
//     compiler emits scalar loads; inside it, behind the image's stores, it cannot show the table unwritten and emits a vector load
//     from the uniform address.  fetch() therefore only loads: the entry waits in a register, and load() makes it a scalar
//     (readfirstlane), clamps it and multiplies -- so the page offsets of a refill are scalar arithmetic either way.
//   - Only live entries are read.  A block index is clamped into [lo >> 4, (hi - 1) >> 4] in front of the lookup and a lane's key into
//     [lo, hi - 1]; the clamped key lies in the clamped block (a block that holds a live key keeps its keys inside itself, a block in
//     front of lo sends every key to lo, one behind hi every key to hi - 1), so key >> log2(page_size) is the entry that was fetched.
//     What the clamp duplicated is replaced at the consumer, as in decode_attn.hip.
//   - A page id forms no address outside the pool: every id is clamped into [0, num_pages - 1] and then multiplied by the page stride in
//     64 bits.
//   - The table is not on the ring's critical path.  entry -> address -> load is a dependent chain the dense kernel does not have.  The
//     two ids of a refill are fetched right behind the slot's PREVIOUS refill -- a whole loop iteration earlier, with a consume of each
//     slot in between -- and wait in two registers per slot.  Vector loads return in order, so an entry arrives right behind the
//     slot's own K and V data, which the consume in front of the refill has waited for anyway: the refill's wait for its two entries
//     leaves the other slot's loads in flight.  In front of the loop the chain is paid once.  (Staging the chunk's slice of the table
//     in LDS was the other choice: it needs a barrier or a wave-private copy, LDS reads in the loop, and a bound on the chunk's length;
//     four registers need none of that.)
#include "paged_attn.hpp"
#include "host_common.hpp"

namespace nnop {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

template <typename T> struct Pa;
template <> struct Pa<__bf16> {
    typedef bf16x8 frag;
    static __device__ __forceinline__ f32x4 mma(frag a, frag b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};
template <> struct Pa<_Float16> {
    typedef f16x8 frag;
    static __device__ __forceinline__ f32x4 mma(frag a, frag b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};

struct PaParams {
    void* o;
    float* lse;
    const void* q;
    const void* k;
    const void* v;
    const int32_t* table;
    const int32_t* seqlens;
    const float* sinks;
    float* ws;
    long long ks_p, ks_h, ks_l, vs_p, vs_h, vs_l, ts;  // elements; ts: int32 entries between two rows of the table
    int QL, G, KH, cap, window, splits, batch;
    int lg_page, num_pages;  // log2(page_size), pages of the pool
    float scale;
};

constexpr float kNegInf = -__builtin_huge_valf();

// the (m, l) pairs lie behind the O rows of every (b, kvh, chunk, row)
__device__ __forceinline__ float* ws_ml(const PaParams& p, int E) {
    return p.ws + (size_t)p.batch * p.KH * p.splits * (p.G * p.QL) * (size_t)E;
}

template <typename T, int E>
__global__ __launch_bounds__(64 * kDaWaves) void paged_attn_kernel(const PaParams p) {
    typedef typename Pa<T>::frag frag;
    constexpr int ES = E / 32;              // E-steps of the scores
    constexpr int ET = E / 16;              // 16-row blocks of O^T
    constexpr int RC = E / 8;               // 16-byte chunks of a row
    constexpr int VCH = kDaTile * RC / 64;  // V chunks of a lane per tile; the first half lies in the tile's first 16-key block
    constexpr int ROWB = 2 * E + 32;        // bytes between two rows of the V image
    constexpr int IMG = kDaTile * ROWB;
    __shared__ __attribute__((aligned(16))) char smem[kDaWaves * IMG];
    static_assert(kDaWaves * IMG >= kDaWaves * ET * 4 * 64 * 4 + 2 * kDaWaves * kDaRows * 4, "the merge reuses the images");
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

    // the query row of this lane: where it stands and what it sees
    const bool row_ok = fm < R;
    const int ppos = hi - p.QL + fm % p.QL;
    const int row_lo = p.window < 0 ? 0 : ppos - p.window;
    frag qf[ES];
    {
        const T* qrow = (const T*)p.q + (rowbase + min(fm, R - 1)) * E + 8 * fq;
#pragma unroll
        for (int s = 0; s < ES; ++s) {
            const uint4 w = *reinterpret_cast<const uint4*>(qrow + 32 * s);
            qf[s] = __builtin_bit_cast(frag, row_ok ? w : uint4{0u, 0u, 0u, 0u});
        }
    }

    const T* kbase = (const T*)p.k + kvh * p.ks_h + 8 * fq;
    const T* vbase = (const T*)p.v + kvh * p.vs_h + 8 * (lane % RC);
    const int vrow = lane / RC;  // V chunk i of the lane: row vrow + i (64 / RC) of the tile, 16-byte chunk lane % RC
    char* img = smem + wave * IMG;
    char* vst = img + vrow * ROWB + 16 * (lane % RC);
    typedef __attribute__((address_space(3))) s16x4* lds_tr_p;
    const char* vld = img + (4 * fq + (fm >> 2)) * ROWB + 8 * (fm & 3);

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
        uint4 k[2][ES];
        uint4 v[VCH];
    };
    Slot ring[2];
    Ids ids[2];
    // K and V loads only, from entries fetched a refill earlier: an id is clamped into the pool, then multiplied in 64 bits
    auto load = [&](Slot& s, const Ids& id, int t) {
        long long kpage[2], vpage[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            const int pg = min(max(__builtin_amdgcn_readfirstlane(id.raw[kb]), 0), p.num_pages - 1);
            kpage[kb] = pg * p.ks_p, vpage[kb] = pg * p.vs_p;
        }
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            const int key = max(min(kDaTile * t + 16 * kb + fm, hi - 1), lo);
            const T* row = kbase + kpage[kb] + (key & row_mask) * p.ks_l;
#pragma unroll
            for (int e = 0; e < ES; ++e) s.k[kb][e] = *reinterpret_cast<const uint4*>(row + 32 * e);
        }
#pragma unroll
        for (int i = 0; i < VCH; ++i) {
            const int key = max(min(kDaTile * t + vrow + i * (64 / RC), hi - 1), lo);
            s.v[i] = *reinterpret_cast<const uint4*>(vbase + vpage[i / (VCH / 2)] + (key & row_mask) * p.vs_l);
        }
    };

    float m_run = kNegInf, l_run = 0.f;
    f32x4 oacc[ET];
#pragma unroll
    for (int et = 0; et < ET; ++et) oacc[et] = f32x4{0.f, 0.f, 0.f, 0.f};

    auto consume = [&](const Slot& s, int t) {
        f32x4 sacc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int e = 0; e < ES; ++e)
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) sacc[kb] = Pa<T>::mma(__builtin_bit_cast(frag, s.k[kb][e]), qf[e], sacc[kb]);
        // selection: the score of a key this row does not see is replaced, whatever it is
        float x[8], mx = kNegInf;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int key = kDaTile * t + 16 * (i >> 2) + 4 * fq + (i & 3);
            const bool ok = row_ok && key <= ppos && key >= row_lo;
            x[i] = ok ? sacc[i >> 2][i & 3] * p.scale : kNegInf;
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
        // the V tile into the wave's image; a row no query of the sequence sees becomes zeros
#pragma unroll
        for (int i = 0; i < VCH; ++i) {
            const int key = kDaTile * t + vrow + i * (64 / RC);
            const bool ok = key >= lo && key < hi;
            *reinterpret_cast<uint4*>(vst + i * (64 / RC) * ROWB) = ok ? s.v[i] : uint4{0u, 0u, 0u, 0u};
        }
        asm volatile("" ::: "memory");
#pragma unroll
        for (int et = 0; et < ET; ++et) {
            const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr_p)(vld + 32 * et));
            const s16x4 d = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr_p)(vld + 32 * et + 16 * ROWB));
            const s16x8 vf = {a[0], a[1], a[2], a[3], d[0], d[1], d[2], d[3]};
            oacc[et] = Pa<T>::mma(__builtin_bit_cast(frag, vf), pf, oacc[et]);
        }
    };

    // pin() as in decode_attn.hip: the refill of a slot stays between the work on two slots.  Here it also keeps a slot's next table
    // entries behind that slot's loads, so no K or V load of a refill is issued behind a lookup of the same refill.
    auto pin = [] {
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
    };
    int t = t0 + wave;
    fetch(ids[0], t);
    fetch(ids[1], t + kDaWaves);
    pin();  // the one place where loads wait for the table
    // in the loop's order -- a slot's loads, then its next entries -- so that the loop's first wait for an entry counts what the later
    // ones count: with both slots' loads in front of both fetches, every refill waited down to vmcnt(2) and drained the other slot
    load(ring[0], ids[0], t);
    pin();
    fetch(ids[0], t + 2 * kDaWaves);
    pin();
    load(ring[1], ids[1], t + kDaWaves);
    pin();
    fetch(ids[1], t + 3 * kDaWaves);
    for (; t < t1; t += 2 * kDaWaves) {
        pin();
        consume(ring[0], t);
        pin();
        load(ring[0], ids[0], t + 2 * kDaWaves);
        pin();
        fetch(ids[0], t + 4 * kDaWaves);  // for this slot's next refill, one iteration from here
        pin();
        if (t + kDaWaves < t1) consume(ring[1], t + kDaWaves);
        pin();
        load(ring[1], ids[1], t + 3 * kDaWaves);
        pin();
        fetch(ids[1], t + 5 * kDaWaves);
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
    // one split: the sink joins as one more column, then divide, round, store
    const float sink = p.sinks ? p.sinks[kvh * p.G + fm / p.QL] : kNegInf;
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
        for (int j = 0; j < 4; ++j) r[j] = (T)(oacc[et][j] * inv);
        *reinterpret_cast<t4*>(orow + 16 * et) = r;
    }
    if (fq == 0 && p.lse) p.lse[rowbase + fm] = L2 > 0.f ? M2 + __logf(L2) : kNegInf;
}

// decode_attn_merge_kernel restated on PaParams: one wave per row of o, the chunks of the row in ascending order, a chunk that had no
// tile (m = -inf, l = 0, no O written) skipped by selection.
template <typename T, int E>
__global__ __launch_bounds__(64) void paged_attn_merge_kernel(const PaParams p) {
    const int R = p.G * p.QL;
    const long long row = blockIdx.x;                  // (b KH + kvh) R + r: the row of o and lse
    const long long bk = row / R;
    const int r = (int)(row % R), lane = threadIdx.x;
    const int h = (int)(bk % p.KH) * p.G + r / p.QL;
    const float* ml = ws_ml(p, E);
    const float sink = p.sinks ? p.sinks[h] : kNegInf;
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
    for (int i = 0; i < E / 64; ++i) ((T*)p.o)[row * E + lane + 64 * i] = (T)(acc[i] * inv);
    if (lane == 0 && p.lse) p.lse[row] = L > 0.f ? M + __logf(L) : kNegInf;
}

template <typename T, int E> int launch(const PaParams& p, hipStream_t s) {
    const int groups = p.batch * p.KH * p.splits;
    hipLaunchKernelGGL((paged_attn_kernel<T, E>), dim3(groups), dim3(64 * kDaWaves), 0, s, p);
    if (p.splits > 1)
        hipLaunchKernelGGL((paged_attn_merge_kernel<T, E>), dim3(p.batch * p.KH * p.G * p.QL), dim3(64), 0, s, p);
    return hipGetLastError() == hipSuccess ? (int)NNOP_OK : (int)NNOP_ERR_HIP;
}

}  // namespace

int launch_paged_attn(const nnop_paged_attn_desc& d, int splits, void* o, float* lse, const void* q, const void* k, const void* v,
                      const int32_t* block_table, const int32_t* seqlens, const float* sinks, float* workspace, hipStream_t stream) {
    PaParams p;
    p.o = o, p.lse = lse, p.q = q, p.k = k, p.v = v, p.table = block_table, p.seqlens = seqlens, p.sinks = sinks, p.ws = workspace;
    p.ks_p = d.k_stride_p, p.ks_h = d.k_stride_h, p.ks_l = d.k_stride_l;
    p.vs_p = d.v_stride_p, p.vs_h = d.v_stride_h, p.vs_l = d.v_stride_l, p.ts = d.table_stride;
    p.QL = d.ql, p.G = d.qh / d.kh, p.KH = d.kh, p.cap = d.max_pages * d.page_size, p.splits = splits, p.batch = d.batch;
    p.lg_page = __builtin_ctz((unsigned)d.page_size), p.num_pages = d.num_pages;
    // a window that reaches past the table removes no key: it is no window, and `hi - QL - window` cannot wrap in the kernel
    p.window = d.window_left >= p.cap ? -1 : d.window_left;
    p.scale = d.emb == 64 ? 0.125f : 0.08838834764831845f;  // 1 / sqrt(E), rounded once
    if (d.dtype == NNOP_BF16) return d.emb == 64 ? launch<__bf16, 64>(p, stream) : launch<__bf16, 128>(p, stream);
    return d.emb == 64 ? launch<_Float16, 64>(p, stream) : launch<_Float16, 128>(p, stream);
}

}  // namespace nnop
