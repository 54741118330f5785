// paged_kv_write.hip -- the kernel of libnnop_hip_paged_kv_write.so (include/nnop_hip_paged_kv_write.h): the K and V rows of a step's new
// tokens go into the pages of a paged KV cache, as they are into a 16-bit pool or as E4M3 codes into an FP8 pool, K and V in one launch.
//
// The kernel moves 2 T KH E elements once and computes next to nothing, so its design is about two things: every access is 16 bytes
// wide, and what it costs to find out WHERE a token goes is paid once per wave, in scalar registers, and hidden under the token's loads.
//
//   - Work.  A workgroup takes kKvwBlockTokens consecutive tokens, wave w of its four the tokens w, w + 4, ... of them, one at a time.
//     The kernel has no reuse to gain from a large block, and the waves in flight are what covers the memory latency: measured
//     (DESIGN.md 4.25), blocks of 8, 16 and 32 tokens were level or slower than 4 at every shape, by up to 3x at decode sizes, so the
//     header's constant is 4 and a wave of this build has ONE token -- the loop below then runs once and the next-token fetch is
//     compiled away; both serve a build with a larger block, which tools/perf_paged_kv_write.py times as a further arm.
//   - The wave's state, all of it wave-uniform and in SGPRs: the sequence b of the token (cu[b] <= t < cu[b + 1]) with its bounds, its
//     clamped length and the offset from a token index to a position; then per token the position p, the ONE table entry
//     table[b][p / page_size], the row p mod page_size and the decision to skip.  The sequence is found by a scan over cu_seqlens_q,
//     64 sequences per step, one per lane, one ballot (the model is paged_prefill_kernel.hpp's search for a block); a wave's tokens
//     ascend, so the scan goes on from the sequence of the token before and is not run at all while the token lies in front of that
//     sequence's end.  A token in front of its sequence's begin belongs to none (cu_seqlens_q was not ascending) and is skipped.
//   - Rows.  A token's K row is KH E elements in KH runs of E, k_stride_h apart, and so is its V row.  A lane owns pieces of 16 bytes OF
//     THE POOL: 8 elements, one 16-byte load, for a 16-bit pool; 16 elements, two 16-byte loads, for E4M3.  Piece c is columns
//     (c mod (E / W)) W ... of head c / (E / W); lane l holds pieces l, l + 64, ... of K and the same of V.  A round is kKvwRound = 1024
//     elements of each -- KH 8 at E 128: four loads a lane -- and all loads of a round are issued in front of its first store; a
//     token with more takes more rounds.  The pieces behind a row's end (KH no power of two, KH E below a round) are predicated off:
//     neither loaded nor stored.
//   - The next token's state -- a scan if it crosses into another sequence, cu[b], cu[b + 1], seqlens[b], then the table entry -- is
//     fetched behind the issue of the first round's loads and in front of its stores, so the chain of dependent scalar loads runs under
//     the vector loads.  The entry is judged (inside [0, P)?) only where the next iteration uses it.
//   - E4M3: fp32(x) / scale[h] is the compiler's correctly rounded fp32 division (HIP's default; this file is built without fast-math
//     flags), the clamp is two compare-and-selects, which let a NaN through where v_min / v_max / v_med3 would return the bound, and
//     v_cvt_pk_fp8_f32 rounds two values to OCP E4M3 codes, ties to even, into one half of a dword.  The clamp stands in front of it
//     because without FP16_OVFL the instruction answers an overflow with NaN, E4M3 having no infinity.  Four dwords of codes are one
//     16-byte store: no byte-wide store anywhere.
//   - No LDS, no barrier, no atomics, plain vector stores.
#include <type_traits>
#include "paged_kv_write.hpp"
#include "host_common.hpp"

namespace nnop {
namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

struct KvwParams {
    const void* k;
    const void* v;
    void* kp;
    void* vp;
    const float* k_scale;
    const float* v_scale;
    const int32_t* table;
    const int32_t* cu;
    const int32_t* seqlens;
    long long ks_t, ks_h, vs_t, vs_h;                        // the sources: elements
    long long kps_p, kps_h, kps_l, vps_p, vps_h, vps_l, ts;  // the pools: pool elements; ts: int32 entries between two rows of the table
    int T, KH, batch, cap, lg_page, num_pages;
};

struct KvwSlot { int page, row; };  // page -1: the token has none

template <typename T> __device__ __forceinline__ float kvw_f32(unsigned bits);  // the low 16 bits as a T
template <> __device__ __forceinline__ float kvw_f32<__bf16>(unsigned bits) { return __builtin_bit_cast(float, bits << 16); }
template <> __device__ __forceinline__ float kvw_f32<_Float16>(unsigned bits) { return (float)__builtin_bit_cast(_Float16, (unsigned short)bits); }

// NaN fails both comparisons and passes
__device__ __forceinline__ float kvw_clamp(float y) {
    y = y > 448.f ? 448.f : y;
    return y < -448.f ? -448.f : y;
}

// four values of T in two dwords -> their four codes in one
template <typename T> __device__ __forceinline__ unsigned kvw_quant4(unsigned w0, unsigned w1, float s) {
    const float a = kvw_clamp(kvw_f32<T>(w0 & 0xffffu) / s), b = kvw_clamp(kvw_f32<T>(w0 >> 16) / s);
    const float c = kvw_clamp(kvw_f32<T>(w1 & 0xffffu) / s), d = kvw_clamp(kvw_f32<T>(w1 >> 16) / s);
    int r = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
    r = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, r, true);
    return (unsigned)r;
}

template <typename T, int FMT, int E>
__global__ __launch_bounds__(kKvwThreads) void paged_kv_write_kernel(const KvwParams p) {
    constexpr bool F8 = FMT == NNOP_PAGED_KV_WRITE_E4M3;
    constexpr int W = F8 ? 16 : 8;           // elements of a piece: 16 bytes of the pool
    constexpr int L = W / 8;                 // its 16-byte loads
    constexpr int J = kKvwRound / (64 * W);  // pieces of K, and of V, that a lane holds per round
    constexpr int RP = E / W;                // pieces of a head's run
    typedef typename std::conditional<F8, unsigned char, T>::type pelem;
    static_assert(J >= 1 && (RP & (RP - 1)) == 0, "a round is whole pieces per lane; head and column of a piece are a shift and a mask");

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int t_end = (int)min((long long)p.T, ((long long)blockIdx.x + 1) * kKvwBlockTokens);
    int t = blockIdx.x * kKvwBlockTokens + wave;
    if (t >= t_end) return;
    const int pieces = p.KH * RP;  // of a token's K row
    auto cu_at = [&](int i) { return min(max(p.cu[i], 0), p.T); };

    // ---- the sequence of the wave's token: b, its tokens [lo, end), its keys hi, and p = base + t ----
    int b = -1, lo = 0, end = 0, hi = 0, base = 0;  // end = 0: the first token scans
    auto locate = [&](int tok) -> KvwSlot {
        if (tok >= end) {  // the first sequence behind b whose end lies behind the token
            int found = p.batch;
            for (int b0 = b + 1; b0 < p.batch; b0 += 64) {
                const int bb = b0 + lane;
                const int e = cu_at(min(bb, p.batch - 1) + 1);
                const unsigned long long hit = __ballot(bb < p.batch && tok < e);
                if (hit) {
                    found = b0 + __builtin_ctzll(hit);
                    break;
                }
            }
            b = __builtin_amdgcn_readfirstlane(found);
            if (b < p.batch) {
                lo = cu_at(b), end = cu_at(b + 1);
                hi = min(max(p.seqlens[b], 0), p.cap);
                base = hi - (end - lo) - lo;  // end > tok >= 0; a lo behind end is caught below
            } else {
                lo = end = 0x7fffffff, hi = 0;  // no sequence for this token or any behind it
            }
        }
        const int pos = base + tok;
        if (tok < lo || (unsigned)pos >= (unsigned)hi) return KvwSlot{-1, 0};  // pos < 0, or no token of b; pos < hi <= cap
        return KvwSlot{p.table[(long long)b * p.ts + (pos >> p.lg_page)], pos & ((1 << p.lg_page) - 1)};
    };

    KvwSlot cur = locate(t);
    for (;;) {
        const int tn = t + kKvwWaves;
        KvwSlot nxt{-1, 0};
        if ((unsigned)cur.page < (unsigned)p.num_pages) {  // an id outside the pool -- -1: a page elsewhere -- writes nothing
            const T* ksrc = (const T*)p.k + (long long)t * p.ks_t;
            const T* vsrc = (const T*)p.v + (long long)t * p.vs_t;
            pelem* kdst = (pelem*)p.kp + (long long)cur.page * p.kps_p + (long long)cur.row * p.kps_l;
            pelem* vdst = (pelem*)p.vp + (long long)cur.page * p.vps_p + (long long)cur.row * p.vps_l;
            for (int c0 = 0; c0 < pieces; c0 += 64 * J) {
                u32x4 rk[J][L], rv[J][L];
                float sk[J], sv[J];
#pragma unroll
                for (int j = 0; j < J; ++j) {
                    const int c = c0 + 64 * j + lane, h = c / RP, col = (c % RP) * W;
                    if (c < pieces) {
#pragma unroll
                        for (int l = 0; l < L; ++l) {
                            rk[j][l] = *reinterpret_cast<const u32x4*>(ksrc + h * p.ks_h + col + 8 * l);
                            rv[j][l] = *reinterpret_cast<const u32x4*>(vsrc + h * p.vs_h + col + 8 * l);
                        }
                        if (F8) sk[j] = p.k_scale ? p.k_scale[h] : 1.f, sv[j] = p.v_scale ? p.v_scale[h] : 1.f;
                    }
                }
                if (c0 == 0 && tn < t_end) nxt = locate(tn);  // under the loads
#pragma unroll
                for (int j = 0; j < J; ++j) {
                    const int c = c0 + 64 * j + lane, h = c / RP, col = (c % RP) * W;
                    if (c < pieces) {
                        u32x4 ok, ov;
                        if constexpr (F8) {
                            ok = u32x4{kvw_quant4<T>(rk[j][0].x, rk[j][0].y, sk[j]), kvw_quant4<T>(rk[j][0].z, rk[j][0].w, sk[j]),
                                       kvw_quant4<T>(rk[j][1].x, rk[j][1].y, sk[j]), kvw_quant4<T>(rk[j][1].z, rk[j][1].w, sk[j])};
                            ov = u32x4{kvw_quant4<T>(rv[j][0].x, rv[j][0].y, sv[j]), kvw_quant4<T>(rv[j][0].z, rv[j][0].w, sv[j]),
                                       kvw_quant4<T>(rv[j][1].x, rv[j][1].y, sv[j]), kvw_quant4<T>(rv[j][1].z, rv[j][1].w, sv[j])};
                        } else {
                            ok = rk[j][0], ov = rv[j][0];
                        }
                        *reinterpret_cast<u32x4*>(kdst + h * p.kps_h + col) = ok;
                        *reinterpret_cast<u32x4*>(vdst + h * p.vps_h + col) = ov;
                    }
                }
            }
        } else if (tn < t_end) {
            nxt = locate(tn);
        }
        if (tn >= t_end) break;
        t = tn, cur = nxt;
    }
}

template <typename T, int FMT, int E> int launch(const KvwParams& p, long long groups, hipStream_t s) {
    hipLaunchKernelGGL((paged_kv_write_kernel<T, FMT, E>), dim3((unsigned)groups), dim3(kKvwThreads), 0, s, p);
    return hipGetLastError() == hipSuccess ? (int)NNOP_OK : (int)NNOP_ERR_HIP;
}

template <typename T, int FMT> int launch_emb(const nnop_paged_kv_write_desc& d, const KvwParams& p, hipStream_t s) {
    const long long groups = paged_kv_write_groups(d);
    return d.emb == 64 ? launch<T, FMT, 64>(p, groups, s) : launch<T, FMT, 128>(p, groups, s);
}

}  // namespace

int launch_paged_kv_write(const nnop_paged_kv_write_desc& d, void* k_pages, void* v_pages, const void* k, const void* v,
                          const float* k_scale, const float* v_scale, const int32_t* block_table, const int32_t* cu_seqlens_q,
                          const int32_t* seqlens, hipStream_t stream) {
    KvwParams p;
    p.k = k, p.v = v, p.kp = k_pages, p.vp = v_pages, p.k_scale = k_scale, p.v_scale = v_scale;
    p.table = block_table, p.cu = cu_seqlens_q, p.seqlens = seqlens;
    p.ks_t = d.k_stride_t, p.ks_h = d.k_stride_h, p.vs_t = d.v_stride_t, p.vs_h = d.v_stride_h;
    p.kps_p = d.kp_stride_p, p.kps_h = d.kp_stride_h, p.kps_l = d.kp_stride_l;
    p.vps_p = d.vp_stride_p, p.vps_h = d.vp_stride_h, p.vps_l = d.vp_stride_l, p.ts = d.table_stride;
    p.T = d.tokens, p.KH = d.kh, p.batch = d.batch, p.cap = d.max_pages * d.page_size;
    p.lg_page = __builtin_ctz((unsigned)d.page_size), p.num_pages = d.num_pages;
    constexpr int F16 = NNOP_PAGED_KV_WRITE_16BIT, F8 = NNOP_PAGED_KV_WRITE_E4M3;
    if (d.dtype == NNOP_BF16)
        return d.kv_format == F8 ? launch_emb<__bf16, F8>(d, p, stream) : launch_emb<__bf16, F16>(d, p, stream);
    return d.kv_format == F8 ? launch_emb<_Float16, F8>(d, p, stream) : launch_emb<_Float16, F16>(d, p, stream);
}

}  // namespace nnop
