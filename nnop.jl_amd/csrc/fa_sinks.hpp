// fa_sinks.hpp -- gradient of the learned attention sinks (nnop_fa_bwd_sinks).
//
// A sink is one more column of every row's softmax with no value vector: p_i,sink = exp(sigma_h - ms_i) / ls_i, and
//     dsigma_h = -sum_{b,i} p_i,sink * delta_i,      delta_i = sum_e dO_ie o_ie.
// dQ, dK, dV and dpair need nothing new: the backward kernels recompute P from (ms, ls), which already include the sink.  This
// pass depends on dO, o, ms, ls alone -- never on the per-row constants that the backward forms keep in the workspace (the fused
// 64-row form holds them only as T-split fragments) -- so dsinks is bitwise the same whichever backward kernels ran.  It runs
// behind them on the same stream and reuses the (then free) workspace for its partial sums.  No atomics: two stages in a fixed
// order.
//   1. one workgroup per (batch, head, chunk of rows): the chunk's sink weights into LDS, then dO and o streamed once, 16 bytes per
//      lane where the layout allows; the workgroup's sum (wave butterflies of row_common.hpp, one LDS hop) -> workspace.
//   2. one wave per head: that head's partials, batch-major, chunks in order.
#pragma once
#include "fa_launch.hpp"
#include "row_common.hpp"

namespace nnop {

struct SinkGradParams {
    const void* d_o;
    const void* o;
    const void* ms;
    const void* ls;
    const float* sinks;    // [QH]
    float* dsinks;         // [QH]
    float* part;           // [B][QH][n_chunk] workgroup partial sums (workspace)
    int QL, QH, B;
    int lg_e;              // log2(E)
    int chunk;             // rows per chunk
    int n_chunk;           // chunks per (batch, head)
};

constexpr int kSinkChunkMax = 1024;

// VEC: elements per load -- 16 bytes (E * sizeof(T) a multiple of 16 and 16-byte aligned bases) or 1
template <typename T, int VEC>
__global__ __launch_bounds__(256) void fa_sinks_partial_kernel(const SinkGradParams p) {
    __shared__ float w[kSinkChunkMax];
    __shared__ float slots[4];
    const int tid = threadIdx.x;
    const int c = (int)(blockIdx.x % (unsigned)p.n_chunk);
    const long long bh = (long long)(blockIdx.x / (unsigned)p.n_chunk);
    const int qh = (int)(bh % p.QH);
    const float sg = p.sinks[qh];
    float acc = 0.f;
    if (sg != -INFINITY) {                                        // workgroup-uniform; sigma = -inf: no sink, a zero gradient
        const int r0 = c * p.chunk;
        const int nrows = p.QL - r0 < p.chunk ? p.QL - r0 : p.chunk;
        const size_t row0 = (size_t)bh * p.QL + r0;
        for (int i = tid; i < nrows; i += 256) {
            const float m = to_f32(((const T*)p.ms)[row0 + i]);
            const float l = to_f32(((const T*)p.ls)[row0 + i]);
            w[i] = expf(sg - m) / l;                              // the sink's share of the row
        }
        __syncthreads();
        const T* __restrict__ a = (const T*)p.d_o + (row0 << p.lg_e);
        const T* __restrict__ b = (const T*)p.o + (row0 << p.lg_e);
        const int n = nrows << p.lg_e;
        typedef T tv __attribute__((ext_vector_type(VEC)));
        for (int e = tid * VEC; e < n; e += 256 * VEC) {
            const tv x = *reinterpret_cast<const tv*>(a + e);
            const tv y = *reinterpret_cast<const tv*>(b + e);
            float dot = 0.f;
#pragma unroll
            for (int j = 0; j < VEC; ++j) dot += to_f32(x[j]) * to_f32(y[j]);
            const float wi = w[e >> p.lg_e];                      // a vector never straddles two rows
            if (wi != 0.f) acc += wi * dot;                       // a row the sink does not reach adds nothing, even a NaN row
        }
    }
    acc = group_allreduce<256>(acc, SumOp{}, slots);
    if (tid == 0) p.part[blockIdx.x] = acc;
}

template <typename T>
__global__ __launch_bounds__(64) void fa_sinks_reduce_kernel(const SinkGradParams p) {
    const int qh = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int n = p.B * p.n_chunk;
    float acc = 0.f;
    for (int j = lane; j < n; j += 64) {
        const int b = j / p.n_chunk, c = j - b * p.n_chunk;
        acc += p.part[((size_t)b * p.QH + qh) * p.n_chunk + c];
    }
    acc = wave_allreduce(acc, SumOp{});
    if (lane == 0) p.dsinks[qh] = 0.f - acc;                      // (+0, not -0, for a head without a sink)
}

template <typename T> int launch_bwd_sinks(const nnop_fa_desc& d, const BwdArgs& a, hipStream_t s) {
    SinkGradParams p;
    p.d_o = a.d_o; p.o = a.o; p.ms = a.ms; p.ls = a.ls;
    p.sinks = a.sinks; p.dsinks = a.dsinks;
    p.part = (float*)a.workspace;
    p.QL = d.ql; p.QH = d.qh; p.B = d.batch;
    p.lg_e = __builtin_ctz((unsigned)d.emb);
    int chunk = 8192 / d.emb;                                     // ~8 Ki elements of each tensor per workgroup
    if (chunk < 16) chunk = 16;
    if (chunk > kSinkChunkMax) chunk = kSinkChunkMax;
    p.chunk = chunk;
    p.n_chunk = (d.ql + chunk - 1) / chunk;
    // the partials, B * QH * n_chunk <= B * QH * QL floats, fit the workspace that launch_bwd was given (>= 2 fp32 per query row)
    const long long grid = (long long)d.batch * d.qh * p.n_chunk;
    if (grid > 0x7fffffffLL || (long long)d.batch * p.n_chunk > 0x7fffffffLL) return NNOP_ERR_SHAPE;
    constexpr int V16 = 16 / (int)sizeof(T);
    const bool vec = (d.emb % V16) == 0 && ((uintptr_t)a.d_o & 15) == 0 && ((uintptr_t)a.o & 15) == 0;
    if (vec) hipLaunchKernelGGL((fa_sinks_partial_kernel<T, V16>), dim3((unsigned)grid), dim3(256), 0, s, p);
    else hipLaunchKernelGGL((fa_sinks_partial_kernel<T, 1>), dim3((unsigned)grid), dim3(256), 0, s, p);
    hipLaunchKernelGGL((fa_sinks_reduce_kernel<T>), dim3((unsigned)d.qh), dim3(64), 0, s, p);
    return hipGetLastError() == hipSuccess ? NNOP_OK : NNOP_ERR_HIP;
}

}  // namespace nnop
