// paged_prefill_split.hip -- the kernels of libnnop_hip_paged_prefill_split.so (include/nnop_hip_paged_prefill_split.h): prefill attention
// over a paged KV cache with the key axis of every row block cut into chunks, for a short run of new tokens behind a long context, where
// KH (T / TB + B) workgroups of a long key range each do not fill the chip.
//
// Pass 1 is paged_prefill_kernel.hpp's text -- the block search, the address path, the two LDS images, the transposed scores on the
// 32x32x16 MFMA, the base-2 softmax -- instantiated with the PpChunk policy: `splits` workgroups per (block, KV head), chunk c walking
// tiles t_lo + c per ... min(t_lo + (c + 1) per - 1, t_hi), per = ceil((t_hi - t_lo + 1) / splits), and leaving each live row's fp32
// un-normalised O and (m, l) in the workspace.  A chunk without a tile touches no table entry and no page and writes (-inf, 0) for its
// live rows, so every slot the merge reads was written by this call.
//
// Pass 2, the merge: a wave per (token, head) row of the tokens in front of cu_seqlens_q[B], four rows per workgroup.  Lane c holds
// chunk c's (m, l) -- at most 64 chunks, so a wave holds them all -- the row's maximum joins the sink, and the live chunks (l > 0) are
// summed in ascending order, four chunks' O in flight at a time, lane i at columns i, i + 64: coalesced fp32 reads.  A chunk with
// l = 0 is selected out by the ballot that steers the loop: its O is never read, whatever the workspace held on entry.
//
// At a resolved count of 1 the launcher runs the thirteenth library's instantiation (PpWhole) of the same text under the same flags: no
// merge, no workspace, that library's bits.
#include "paged_prefill_kernel.hpp"
#include "paged_prefill_split.hpp"
#include "host_common.hpp"

namespace nnop {
namespace {

template <typename T, int E>
__global__ __launch_bounds__(kPpThreads) __attribute__((amdgpu_waves_per_eu(2, 2))) void paged_prefill_kernel(const PpParams p) {
    paged_prefill_body<T, E, PpStage16<T, E>>(p);
}

template <typename T, int E>
__global__ __launch_bounds__(kPpThreads) __attribute__((amdgpu_waves_per_eu(2, 2))) void paged_prefill_split_kernel(const PpParams p,
                                                                                                                  const PpChunk part) {
    paged_prefill_body<T, E, PpStage16<T, E>, PpChunk>(p, part);
}

struct PpsMerge {
    void* o;
    float* lse;
    const float* o_part;   // [splits][T][QH][E]
    const float* ml_part;  // [splits][T][QH][2]
    const int32_t* cu;
    const float* sinks;
    long long os_t, os_h;
    int T, QH, batch, splits;
};

template <typename T, int E>
__global__ __launch_bounds__(64 * kPpsMergeRows) void paged_prefill_split_merge_kernel(const PpsMerge p) {
    constexpr int NC = E / 64;  // columns of a lane
    constexpr int kAhead = 4;   // chunks whose O is in flight together
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long row = (long long)blockIdx.x * kPpsMergeRows + wave;
    if (row >= (long long)p.T * p.QH) return;
    const int t = (int)(row / p.QH), head = (int)(row - (long long)t * p.QH);
    if (t >= min(max(p.cu[p.batch], 0), p.T)) return;  // a token outside every sequence: pass 1 wrote nothing for it, o stays as it is

    float m = kPpNegInf, l = 0.f;
    if (lane < p.splits) {
        const float2 ml = *reinterpret_cast<const float2*>(p.ml_part + 2 * (((long long)lane * p.T + t) * p.QH + head));
        m = ml.x, l = ml.y;
    }
    const unsigned long long seen = __ballot(l > 0.f);  // the chunks in which the row saw a key; the others are (-inf, 0)
    const float sink_e = p.sinks ? p.sinks[head] : kPpNegInf, sink = sink_e * kPpLog2e;
    float M = m;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) M = fmaxf(M, __shfl_xor(M, d));
    M = fmaxf(M, sink);
    const float m_ref = M == kPpNegInf ? 0.f : M;
    const float w = __builtin_amdgcn_exp2f(m - m_ref), lw = l * w;

    float L = 0.f, acc[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) acc[i] = 0.f;
    const long long chunk_stride = (long long)p.T * p.QH * E;
    const float* orow = p.o_part + ((long long)t * p.QH + head) * E + lane;
    for (unsigned long long left = seen; left;) {  // ascending c, kAhead live chunks a step
        int c[kAhead], last = 0;
        bool on[kAhead];
        float x[kAhead][NC];
#pragma unroll
        for (int k = 0; k < kAhead; ++k) {
            on[k] = left != 0;
            c[k] = last = on[k] ? __builtin_ctzll(left) : last;  // behind the last live chunk: that chunk once more, loaded and dropped
            left &= left - 1;                                   // 0 stays 0
#pragma unroll
            for (int i = 0; i < NC; ++i) x[k][i] = orow[c[k] * chunk_stride + 64 * i];
        }
#pragma unroll
        for (int k = 0; k < kAhead; ++k) {
            if (!on[k]) break;
            const float wc = __shfl(w, c[k]);
            L += __shfl(lw, c[k]);
#pragma unroll
            for (int i = 0; i < NC; ++i) acc[i] = __builtin_fmaf(x[k][i], wc, acc[i]);
        }
    }
    // the sink joins as one more column, then divide, round once, store
    L += __builtin_amdgcn_exp2f(sink - m_ref);
    const float inv = L > 0.f ? 1.f / L : 0.f;
    T* out = (T*)p.o + t * p.os_t + head * p.os_h + lane;
#pragma unroll
    for (int i = 0; i < NC; ++i) out[64 * i] = (T)(acc[i] * inv);
    // a row without a key has its sink for lse, bit for bit, as in the one-pass epilogue
    if (lane == 0 && p.lse) p.lse[row] = !seen ? sink_e : (M + __log2f(L)) * kPpLn2;
}

template <typename T, int E> int launch(const PpParams& p, const PpChunk& part, const PpsMerge& mg, long long groups, hipStream_t s) {
    if (part.splits == 1) {
        hipLaunchKernelGGL((paged_prefill_kernel<T, E>), dim3((unsigned)groups), dim3(kPpThreads), 0, s, p);
        return hipGetLastError() == hipSuccess ? (int)NNOP_OK : (int)NNOP_ERR_HIP;
    }
    hipLaunchKernelGGL((paged_prefill_split_kernel<T, E>), dim3((unsigned)(groups * part.splits)), dim3(kPpThreads), 0, s, p, part);
    if (hipGetLastError() != hipSuccess) return NNOP_ERR_HIP;
    const long long rows = (long long)p.T * p.QH;
    hipLaunchKernelGGL((paged_prefill_split_merge_kernel<T, E>), dim3((unsigned)((rows + kPpsMergeRows - 1) / kPpsMergeRows)),
                       dim3(64 * kPpsMergeRows), 0, s, mg);
    return hipGetLastError() == hipSuccess ? (int)NNOP_OK : (int)NNOP_ERR_HIP;
}

}  // namespace

int launch_paged_prefill_split(const nnop_paged_prefill_desc& d, int splits, void* o, float* lse, const void* q, const void* k,
                               const void* v, const int32_t* block_table, const int32_t* cu_seqlens_q, const int32_t* seqlens,
                               const float* sinks, float* workspace, hipStream_t stream) {
    PpParams p;
    p.o = o, p.lse = lse, p.q = q, p.k = k, p.v = v, p.table = block_table, p.cu = cu_seqlens_q, p.seqlens = seqlens, p.sinks = sinks;
    paged_prefill_fill(p, d);
    const long long groups = d.kh * paged_prefill_max_blocks(d);
    PpChunk part;
    part.splits = splits;
    part.o_part = workspace;
    part.ml_part = workspace ? workspace + (size_t)splits * d.tokens * d.qh * d.emb : nullptr;
    PpsMerge mg;
    mg.o = o, mg.lse = lse, mg.o_part = part.o_part, mg.ml_part = part.ml_part, mg.cu = cu_seqlens_q, mg.sinks = sinks;
    mg.os_t = d.o_stride_t, mg.os_h = d.o_stride_h, mg.T = d.tokens, mg.QH = d.qh, mg.batch = d.batch, mg.splits = splits;
    if (d.dtype == NNOP_BF16) return d.emb == 64 ? launch<__bf16, 64>(p, part, mg, groups, stream) : launch<__bf16, 128>(p, part, mg, groups, stream);
    return d.emb == 64 ? launch<_Float16, 64>(p, part, mg, groups, stream) : launch<_Float16, 128>(p, part, mg, groups, stream);
}

}  // namespace nnop
