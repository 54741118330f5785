// decode_attn_fp8.hip -- the kernels of libnnop_hip_decode_attn_fp8.so (include/nnop_hip_decode_attn_fp8.h): decode_attn.hip's attention of
// QL new tokens per sequence over a KV cache whose K and V are one-byte OCP E4M3 codes, read where they lie and expanded to T (the type
// of q and o) in registers.  Work split, rows, softmax, selection, merge order and every contract are decode_attn.hip's; what follows is
// the data path, which is new.
//
// Conversion.  v_cvt_scalef32_pk_{bf16,f16}_fp8 with the scale operand 1.0f turns the two codes of one half of a 32-bit word (the low
// byte first) into two T values, exactly: every finite E4M3 value (2^-9 ... 448, 3 mantissa bits) is a bfloat16 and a float16 value, and
// the NaN codes 0x7F / 0xFF give NaN.  Eight codes -- two words -- are four conversions and one MFMA operand.  Both products stay
// v_mfma_f32_16x16x32_{bf16,f16} on T with fp32 accumulation; the probabilities are rounded to T as before, not to 8 bits.
//
// Scores.  S^T[32 keys][16 rows] = K Q^T.  A key row is E bytes.  Lane (r = lane % 16, g = lane / 16) loads the 16 bytes e = 64 s + 16 g
// ... + 15 of key row 16 kb + r: one global_load_dwordx4 per key block at E = 64, two at E = 128, the four lane groups covering 64-byte
// pieces of a row.  Its low 8 bytes are the A operand of E-step 2 s, its high 8 bytes that of E-step 2 s + 1, so the k-index 8 g + j of
// step 2 s + u is column e = 64 s + 16 g + 8 u + j.  Q, the B operand, is loaded once with the same e <- k mapping: lane (m, g) holds
// the 16 values e = 64 s + 16 g ... of row m as two operands.  No LDS on this path.  The result leaves lane (m, g) with keys
// 16 kb + 4 g + j of row m, as in decode_attn.hip.
//
// P V.  O^T[E][16 rows] += V^T[E][32 keys] P^T.  The lane's 8 probabilities are the B operand as they stand: k = 8 g + a is key 4 g + a
// for a < 4 and key 16 + 4 g + (a - 4) for a >= 4.  V^T is the A operand.  The wave stores its V tile as raw bytes, row-major, into a
// wave-private LDS image (a row no query of the sequence sees as zero bytes, +0 in E4M3) and reads it back with ds_read_b64_tr_b8, the
// 8 x 16 hardware transpose of bytes: in a group of 16 lanes, lane 2 a + p (a = 0 ... 7, p = 0, 1) names the 8 bytes of columns 8 p ...
// 8 p + 7 of row a, and lane i receives column i of rows 0 ... 7, row a in byte a of its 64 bits (established on an MI355X with a
// pattern of byte positions; the 16-bit form of decode_attn.hip is the same rule with 4 rows and 4 columns per lane).  One read per 16
// columns of E hands a lane its 8 keys of one e-column -- the 16-bit kernel needs two -- and four conversions make them the A operand.
// The image holds the keys in the order the reads want them: key 16 h + 4 g + j of the tile lies in image row 8 g + 4 h + j, so lane
// 2 a + p of group g names image row 8 g + a, which is the key of k = 8 g + a above.
// Row stride E + 16 bytes: an odd number of 16-byte units, so the 16 image rows that the two groups of a half wave name in one read
// (rows 8 g ... 8 g + 7, 16 bytes each) start in 16 different 16-byte bank groups of the 256 bytes the LDS serves per pass.
// The image is wave-private and LDS operations of a wave complete in order, so the loop has no barrier.
//
// The ring.  A tile is half the bytes of the 16-bit kernel's, so four tiles of K and V loads are in flight per wave (E = 128: 4 x (4 + 4)
// loads of 16 bytes per lane, the 32 loads of the 16-bit kernel's two tiles); the loop consumes slot d and refills it with the wave's
// fourth tile from there, pin() between the two.  Loads are unconditional from a key index clamped into [0, hi - 1].
//
// Scales.  k_scale[kvh] / sqrt(E) is formed once in fp32 and multiplies the fp32 scores, so the sink, m, l and lse are in the scaled
// domain.  v_scale[kvh] multiplies the fp32 O after the division and before its one rounding, in the kernel that divides: the chunk
// kernel at one split, the merge kernel otherwise.  The partial results in the workspace are unscaled.
//
// End of a chunk and the merge of the chunks: decode_attn.hip's, restated here with that factor (the tenth library's objects are not
// touched, and nothing is linked from it).
#include "decode_attn_fp8.hpp"
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
template <typename T> struct Df;
template <> struct Df<__bf16> {
    typedef bf16x8 frag;
    typedef bf16x2 pair;
    static __device__ __forceinline__ f32x4 mma(frag a, frag b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
    template <bool HI> static __device__ __forceinline__ pair cvt(uint32_t w) { return __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)w, 1.0f, HI); }
};
template <> struct Df<_Float16> {
    typedef f16x8 frag;
    typedef f16x2 pair;
    static __device__ __forceinline__ f32x4 mma(frag a, frag b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
    template <bool HI> static __device__ __forceinline__ pair cvt(uint32_t w) { return __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)w, 1.0f, HI); }
};

// eight codes, byte 0 of w0 first, as one operand
template <typename T> __device__ __forceinline__ typename Df<T>::frag expand8(uint32_t w0, uint32_t w1) {
    const typename Df<T>::pair a = Df<T>::template cvt<false>(w0), b = Df<T>::template cvt<true>(w0);
    const typename Df<T>::pair c = Df<T>::template cvt<false>(w1), d = Df<T>::template cvt<true>(w1);
    return typename Df<T>::frag{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}

struct DfParams {
    void* o;
    float* lse;
    const void* q;
    const uint8_t* k;
    const uint8_t* v;
    const float* k_scale;
    const float* v_scale;
    const int32_t* seqlens;
    const float* sinks;
    float* ws;
    long long ks_b, ks_h, ks_l, vs_b, vs_h, vs_l;  // bytes
    int QL, G, KH, cap, window, splits, batch;
    float scale;  // 1 / sqrt(E)
};

constexpr float kNegInf = -__builtin_huge_valf();

// the (m, l) pairs lie behind the O rows of every (b, kvh, chunk, row)
__device__ __forceinline__ float* ws_ml(const DfParams& p, int E) {
    return p.ws + (size_t)p.batch * p.KH * p.splits * (p.G * p.QL) * (size_t)E;
}

// the image row of key `key` of a tile: key 16 h + 4 g + j -> 8 g + 4 h + j
__device__ __forceinline__ int image_row(int key) { return 8 * ((key >> 2) & 3) + 4 * (key >> 4) + (key & 3); }

template <typename T, int E>
__global__ __launch_bounds__(64 * kDaWaves) void decode_attn_fp8_kernel(const DfParams p) {
    typedef typename Df<T>::frag frag;
    constexpr int ES = E / 32;              // E-steps of the scores
    constexpr int KL = E / 64;              // 16-byte loads of a lane per key block: each feeds two E-steps
    constexpr int ET = E / 16;              // 16-row blocks of O^T
    constexpr int RC = E / 16;              // 16-byte chunks of a row
    constexpr int VCH = kDaTile * RC / 64;  // V chunks of a lane per tile
    constexpr int ROWB = E + 16;            // bytes between two rows of the V image: an odd number of 16-byte units
    constexpr int IMG = kDaTile * ROWB;
    constexpr int MERGE = kDaWaves * ET * 4 * 64 * 4 + 2 * kDaWaves * kDaRows * 4;
    // the wave-private V images; after the loop the same bytes carry the waves' (O, m, l) to wave 0, which needs more of them
    __shared__ __attribute__((aligned(16))) char smem[MERGE > kDaWaves * IMG ? MERGE : kDaWaves * IMG];

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

    const float sc = (p.k_scale ? p.k_scale[kvh] : 1.f) * p.scale;  // the one factor of the scores

    // pin() keeps the refill of a slot between the work on two slots (section 4.16 of DESIGN.md: left alone, the compiler gathers the
    // loads of an iteration, waits for all of them and computes, and the ring is gone); it also orders the image's reads and writes.
    // In front of the loop it keeps the loads in the order the loop's waits count on: Q, then the four slots one after the other.
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

    const uint8_t* kbase = p.k + b * p.ks_b + kvh * p.ks_h + 16 * fq;
    const uint8_t* vbase = p.v + b * p.vs_b + kvh * p.vs_h + 16 * (lane % RC);
    const int vrow = lane / RC;  // V chunk i of the lane: key vrow + i (64 / RC) of the tile, 16-byte chunk lane % RC
    char* img = smem + wave * IMG;
    char* vst = img + 16 * (lane % RC);
    typedef __attribute__((address_space(3))) i32x2* lds_tr_p;
    const char* vld = img + (8 * fq + (fm >> 1)) * ROWB + 8 * (fm & 1);

    struct Slot {
        uint4 k[2][KL];
        uint4 v[VCH];
    };
    Slot ring[kDfRing];
    // loads only: nothing here waits for what it fetched
    auto load = [&](Slot& s, int t) {
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            const int key = max(min(kDaTile * t + 16 * kb + fm, hi - 1), 0);
            const uint8_t* row = kbase + key * p.ks_l;
#pragma unroll
            for (int e = 0; e < KL; ++e) s.k[kb][e] = *reinterpret_cast<const uint4*>(row + 64 * e);
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
        for (int e = 0; e < KL; ++e)
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                const uint4 w = s.k[kb][e];
                sacc[kb] = Df<T>::mma(expand8<T>(w.x, w.y), qf[2 * e], sacc[kb]);
                sacc[kb] = Df<T>::mma(expand8<T>(w.z, w.w), qf[2 * e + 1], sacc[kb]);
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
            oacc[et] = Df<T>::mma(expand8<T>((uint32_t)a[0], (uint32_t)a[1]), pf, oacc[et]);
        }
    };

    int t = t0 + wave;
#pragma unroll
    for (int d = 0; d < kDfRing; ++d) {
        pin();
        load(ring[d], t + d * kDaWaves);
    }
    for (; t < t1; t += kDfRing * kDaWaves) {
#pragma unroll
        for (int d = 0; d < kDfRing; ++d) {
            pin();
            if (d == 0 || t + d * kDaWaves < t1) consume(ring[d], t + d * kDaWaves);
            pin();
            load(ring[d], t + (kDfRing + d) * kDaWaves);
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

// One wave per row of o: the chunks of the row in ascending order.  A chunk that had no tile wrote (m = -inf, l = 0) and no O: it is
// skipped by selection, so nothing of its unwritten O enters the sum.  v_scale joins after the division.
template <typename T, int E>
__global__ __launch_bounds__(64) void decode_attn_fp8_merge_kernel(const DfParams p) {
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

template <typename T, int E> int launch(const DfParams& p, hipStream_t s) {
    const int groups = p.batch * p.KH * p.splits;
    hipLaunchKernelGGL((decode_attn_fp8_kernel<T, E>), dim3(groups), dim3(64 * kDaWaves), 0, s, p);
    if (p.splits > 1)
        hipLaunchKernelGGL((decode_attn_fp8_merge_kernel<T, E>), dim3(p.batch * p.KH * p.G * p.QL), dim3(64), 0, s, p);
    return hipGetLastError() == hipSuccess ? (int)NNOP_OK : (int)NNOP_ERR_HIP;
}

}  // namespace

int launch_decode_attn_fp8(const nnop_decode_attn_fp8_desc& d, int splits, void* o, float* lse, const void* q, const void* k, const void* v,
                           const float* k_scale, const float* v_scale, const int32_t* seqlens, const float* sinks, float* workspace,
                           hipStream_t stream) {
    DfParams p;
    p.o = o, p.lse = lse, p.q = q, p.k = (const uint8_t*)k, p.v = (const uint8_t*)v, p.k_scale = k_scale, p.v_scale = v_scale;
    p.seqlens = seqlens, p.sinks = sinks, p.ws = workspace;
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
