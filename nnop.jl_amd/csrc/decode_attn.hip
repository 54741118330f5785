// decode_attn.hip -- the kernels of libnnop_hip_decode_attn.so (include/nnop_hip_decode_attn.h): attention of QL new tokens per sequence
// over a KV cache, split over the cache (split-KV), with the query heads of a KV head packed into one matrix operand.
//
// Work.  A workgroup is (sequence b, KV head, chunk c), four waves.  The R = G QL rows (row r = g QL + i: query head kvh G + g, token i --
// R consecutive rows of q, o and lse) are the 16 columns of one MFMA operand; columns >= R are zeros and are never stored.  The live key
// range [lo, hi) of the sequence (hi = seqlens[b] clamped into [0, cap]; lo = 0 or the first key the oldest query's window reaches) is
// cut into `splits` runs of ceil(tiles / splits) tiles of 32 keys; chunk c takes the c-th run, its waves take its tiles round-robin.
//
// Scores.  S^T[32 keys][16 rows] = K Q^T by v_mfma_f32_16x16x32: K rows are the A operand, straight from global memory -- lane (r = lane %
// 16, q = lane / 16) loads the 16 bytes e = 32 s + 8 q ... + 7 of key row 16 kb + r for each key block kb and E-step s, so the steps of a
// lane group cover whole 128-byte lines -- and Q is the B operand, loaded once (lane (m, q): row m, the same e) and kept.  The result
// leaves lane (m, q) with keys 16 kb + 4 q + j (j = 0 ... 3; kb = 0, 1) of query row m: 4 + 4 keys of one row.
//
// Softmax, online, in those registers: the row maximum and sum run over the lane's 8 values and over the four lane groups by two
// xor-shuffles (16, 32), which leave the four lanes of a row with the same bits.  (m, l, O^T) are private to a wave.
//
// P V.  O^T[E][16 rows] += V^T[E][32 keys] P^T[32 keys][16 rows]: the 8 probabilities of a lane are the B operand as they stand, with the
// keys in the order k = 8 q + j -> key 4 q + j, k = 8 q + 4 + j -> key 16 + 4 q + j.  V^T is the A operand and needs a transpose: the wave
// stores its V tile row-major into a wave-private LDS image (rows that no query sees replaced by zeros there) and reads it back with
// ds_read_b64_tr_b16, the 4 x 16 hardware transpose: in a group of 16 lanes, lane 4 a + p names 4 columns 4 p ... of row a, and lane i
// receives column i of rows 0 ... 3.  Group q names the keys 4 q + a (and 16 + 4 q + a in a second read), which is the permutation above.
// The image is wave-private and LDS operations of a wave complete in order, so the loop has no barrier.
//
// The ring.  Two tiles of K and V loads are in flight per wave; the loop consumes slot d and refills it with the wave's tile after next.
// Every load is unconditional from a key index clamped into [0, hi - 1]; what the clamp duplicated is replaced at the consumer.
//
// End of a chunk: the four waves merge through LDS in ascending wave order (wave 0 does the sums).  At one split the workgroup adds the
// sink, divides, rounds and stores; otherwise it writes fp32 (O, m, l) and decode_attn_merge_kernel merges a row's chunks in ascending
// order, skipping by selection the chunks that had no tile (their O was never written).
#include "decode_attn.hpp"
#include "host_common.hpp"

namespace nnop {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

template <typename T> struct Da;
template <> struct Da<__bf16> {
    typedef bf16x8 frag;
    static __device__ __forceinline__ f32x4 mma(frag a, frag b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};
template <> struct Da<_Float16> {
    typedef f16x8 frag;
    static __device__ __forceinline__ f32x4 mma(frag a, frag b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};

struct DaParams {
    void* o;
    float* lse;
    const void* q;
    const void* k;
    const void* v;
    const int32_t* seqlens;
    const float* sinks;
    float* ws;
    long long ks_b, ks_h, ks_l, vs_b, vs_h, vs_l;  // elements
    int QL, G, KH, cap, window, splits, batch;
    float scale;
};

constexpr float kNegInf = -__builtin_huge_valf();

// the (m, l) pairs lie behind the O rows of every (b, kvh, chunk, row)
__device__ __forceinline__ float* ws_ml(const DaParams& p, int E) {
    return p.ws + (size_t)p.batch * p.KH * p.splits * (p.G * p.QL) * (size_t)E;
}

template <typename T, int E>
__global__ __launch_bounds__(64 * kDaWaves) void decode_attn_kernel(const DaParams p) {
    typedef typename Da<T>::frag frag;
    constexpr int ES = E / 32;              // E-steps of the scores
    constexpr int ET = E / 16;              // 16-row blocks of O^T
    constexpr int RC = E / 8;               // 16-byte chunks of a row
    constexpr int VCH = kDaTile * RC / 64;  // V chunks of a lane per tile
    constexpr int ROWB = 2 * E + 32;        // bytes between two rows of the V image: 8 consecutive rows start in 8 different 32-byte bank groups
    constexpr int IMG = kDaTile * ROWB;
    // the wave-private V images; after the loop the same bytes carry the waves' (O, m, l) to wave 0
    __shared__ __attribute__((aligned(16))) char smem[kDaWaves * IMG];
    static_assert(kDaWaves * IMG >= kDaWaves * ET * 4 * 64 * 4 + 2 * kDaWaves * kDaRows * 4, "the merge reuses the images");

    const int bid = blockIdx.x;
    const int c = bid % p.splits, kvh = (bid / p.splits) % p.KH, b = bid / (p.splits * p.KH);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, fm = lane & 15, fq = lane >> 4;
    const int R = p.G * p.QL;
    const long long rowbase = ((long long)b * p.KH + kvh) * R;  // first of the R rows of q, o, lse

    const int hi = min(max(p.seqlens[b], 0), p.cap);
    const int lo = p.window < 0 ? 0 : max(0, hi - p.QL - p.window);  // the first key any query of the sequence sees
    const int t_lo = lo / kDaTile, t_hi = (hi + kDaTile - 1) / kDaTile;
    const int per = (t_hi - t_lo + p.splits - 1) / p.splits;
    const int t0 = t_lo + c * per, t1 = min(t_hi, t0 + per);
    const long long part = ((long long)b * p.KH + kvh) * p.splits + c;  // this chunk's place in the workspace

    if (t0 >= t1) {  // no tile: nothing of the cache is read
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

    const T* kbase = (const T*)p.k + b * p.ks_b + kvh * p.ks_h + 8 * fq;
    const T* vbase = (const T*)p.v + b * p.vs_b + kvh * p.vs_h + 8 * (lane % RC);
    const int vrow = lane / RC;  // V chunk i of the lane: row vrow + i (64 / RC) of the tile, 16-byte chunk lane % RC
    char* img = smem + wave * IMG;
    char* vst = img + vrow * ROWB + 16 * (lane % RC);
    typedef __attribute__((address_space(3))) s16x4* lds_tr_p;
    const char* vld = img + (4 * fq + (fm >> 2)) * ROWB + 8 * (fm & 3);

    struct Slot {
        uint4 k[2][ES];
        uint4 v[VCH];
    };
    Slot ring[2];
    // loads only: nothing here waits for what it fetched
    auto load = [&](Slot& s, int t) {
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            const int key = max(min(kDaTile * t + 16 * kb + fm, hi - 1), 0);
            const T* row = kbase + key * p.ks_l;
#pragma unroll
            for (int e = 0; e < ES; ++e) s.k[kb][e] = *reinterpret_cast<const uint4*>(row + 32 * e);
        }
#pragma unroll
        for (int i = 0; i < VCH; ++i) {
            const int key = max(min(kDaTile * t + vrow + i * (64 / RC), hi - 1), 0);
            s.v[i] = *reinterpret_cast<const uint4*>(vbase + key * p.vs_l);
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
            for (int kb = 0; kb < 2; ++kb) sacc[kb] = Da<T>::mma(__builtin_bit_cast(frag, s.k[kb][e]), qf[e], sacc[kb]);
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
            oacc[et] = Da<T>::mma(__builtin_bit_cast(frag, vf), pf, oacc[et]);
        }
    };

    // pin() keeps the refill of a slot between the work on two slots (section 4.16 of DESIGN.md: left alone, the compiler gathers the
    // loads of an iteration, waits for all of them and computes, and the ring is gone); it also orders the image's reads and writes
    auto pin = [] {
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
    };
    int t = t0 + wave;
    load(ring[0], t);
    load(ring[1], t + kDaWaves);
    for (; t < t1; t += 2 * kDaWaves) {
        pin();
        consume(ring[0], t);
        pin();
        load(ring[0], t + 2 * kDaWaves);
        pin();
        if (t + kDaWaves < t1) consume(ring[1], t + kDaWaves);
        pin();
        load(ring[1], t + 3 * kDaWaves);
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

// One wave per row of o: the chunks of the row in ascending order.  A chunk that had no tile wrote (m = -inf, l = 0) and no O: it is
// skipped by selection, so nothing of its unwritten O enters the sum.
template <typename T, int E>
__global__ __launch_bounds__(64) void decode_attn_merge_kernel(const DaParams p) {
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

template <typename T, int E> int launch(const DaParams& p, hipStream_t s) {
    const int groups = p.batch * p.KH * p.splits;
    hipLaunchKernelGGL((decode_attn_kernel<T, E>), dim3(groups), dim3(64 * kDaWaves), 0, s, p);
    if (p.splits > 1)
        hipLaunchKernelGGL((decode_attn_merge_kernel<T, E>), dim3(p.batch * p.KH * p.G * p.QL), dim3(64), 0, s, p);
    return hipGetLastError() == hipSuccess ? (int)NNOP_OK : (int)NNOP_ERR_HIP;
}

}  // namespace

int launch_decode_attn(const nnop_decode_attn_desc& d, int splits, void* o, float* lse, const void* q, const void* k, const void* v,
                       const int32_t* seqlens, const float* sinks, float* workspace, hipStream_t stream) {
    DaParams p;
    p.o = o, p.lse = lse, p.q = q, p.k = k, p.v = v, p.seqlens = seqlens, p.sinks = sinks, p.ws = workspace;
    p.ks_b = d.k_stride_b, p.ks_h = d.k_stride_h, p.ks_l = d.k_stride_l;
    p.vs_b = d.v_stride_b, p.vs_h = d.v_stride_h, p.vs_l = d.v_stride_l;
    p.QL = d.ql, p.G = d.qh / d.kh, p.KH = d.kh, p.cap = d.capacity, p.splits = splits, p.batch = d.batch;
    // a window that reaches past the cache removes no key: it is no window, and `hi - QL - window` cannot wrap in the kernel
    p.window = d.window_left >= d.capacity ? -1 : d.window_left;
    p.scale = d.emb == 64 ? 0.125f : 0.08838834764831845f;  // 1 / sqrt(E), rounded once
    if (d.dtype == NNOP_BF16) return d.emb == 64 ? launch<__bf16, 64>(p, stream) : launch<__bf16, 128>(p, stream);
    return d.emb == 64 ? launch<_Float16, 64>(p, stream) : launch<_Float16, 128>(p, stream);
}

}  // namespace nnop
