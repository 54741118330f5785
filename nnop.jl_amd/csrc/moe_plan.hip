// moe_plan.hip -- the expert dispatch plan for gfx950 (include/nnop_hip_moe.h): a stable counting sort of the T k flat assignment
// ids by expert.
//
// Four launches, no atomics, the same result on every run:
//   1. moe_plan_hist     every wave takes a contiguous chunk of flat ids (kPlanChunk = 64: one pass of the ranking loop; longer
//                        chunks once there would be above kPlanMaxChunks of them) and counts it into its own histogram
//                        hist[chunk][E] in the workspace, all E words written;
//   2. moe_plan_colscan  one workgroup per expert: the exclusive prefix of that expert's column over the chunks, in place, and
//                        counts[e].  A thread owns a contiguous run of chunks, the 256 run totals meet in an LDS scan;
//   3. moe_plan_escan    one workgroup: offsets = the exclusive prefix of counts;
//   4. moe_plan_scatter  every wave walks its chunk again, 64 ids at a time, from the start positions offsets[e] + hist[chunk][e].
// Ranking equal experts among the 64 lanes (steps 1 and 4): each distinct expert among the lanes not yet ranked is taken in turn -- the
// first such lane's expert is broadcast, a ballot marks its lanes, a lane's rank is the popcount of the ballot below it.  The running
// positions live in a per-wave LDS array touched once per 64 ids; a wave's LDS operations execute in order, no barrier is needed.
// An entry outside [0, E) never becomes active: it is not counted and gets slot -1.  perm[offsets[E] ...] is filled with -1 by the wave
// whose chunk covers those positions.
// Bound: latency -- the ranking loop runs once per distinct expert of a 64-id batch.
#include "fa_common.hpp"
#include "moe.hpp"

namespace nnop {

constexpr int kPlanChunk = 64;           // flat ids per wave
constexpr int kPlanMaxChunks = 4096;     // above: longer chunks (the workspace stays <= 16 MiB)
constexpr int kPlanWaves = 4;            // waves per workgroup of steps 1 and 4

struct MoePlanParams {
    const int32_t* idx;
    int32_t *counts, *offsets, *perm, *slot, *hist;
    long long N;                         // T k
    int E, chunk, n_chunks;
};

static inline void moe_plan_chunks(long long N, int& chunk, int& n_chunks) {
    long long c = (N + kPlanMaxChunks - 1) / kPlanMaxChunks;
    c = (c + 63) / 64 * 64;
    if (c < kPlanChunk) c = kPlanChunk;
    chunk = (int)c;                                                 // < 2^31 / 4096 + 64
    n_chunks = (int)((N + c - 1) / c);
}

size_t moe_plan_ws_bytes(const nnop_moe_plan_desc& d) {
    int chunk, n_chunks;
    moe_plan_chunks((long long)d.tokens * d.topk, chunk, n_chunks);
    return ((size_t)n_chunks * (size_t)d.experts * sizeof(int32_t) + 15) & ~(size_t)15;
}

// The lanes of a wave exchange values through the wave's own LDS array.  The hardware executes a wave's LDS operations in order; this
// keeps the compiler from moving or merging them across the point (wavefront scope: no cache operation, no barrier instruction).
NNOP_DEV void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Among the lanes with `valid`: rank = how many lower lanes hold the same e, cnt = how many lanes hold it.  Wave-uniform control flow.
NNOP_DEV void moe_match(int e, bool valid, int lane, int& rank, int& cnt) {
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned long long todo = __ballot(valid);
    rank = 0; cnt = 0;
    while (todo) {
        const int first = __builtin_ctzll(todo);
        const int e0 = __builtin_amdgcn_readlane(e, first);
        const bool same = valid && e == e0;
        const unsigned long long m = __ballot(same);
        if (same) { rank = __popcll(m & below); cnt = __popcll(m); }
        todo &= ~m;                                                 // m holds lane `first`: the loop ends
    }
}

__global__ __launch_bounds__(kPlanWaves * 64) void moe_plan_hist_kernel(const MoePlanParams p) {
    __shared__ int32_t cnt_all[kPlanWaves][kMoeMaxExperts];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int chunk = blockIdx.x * kPlanWaves + wave;
    if (chunk >= p.n_chunks) return;                                // a whole wave; there is no barrier in this kernel
    for (int e = lane; e < p.E; e += 64) cnt_all[wave][e] = 0;
    wave_lds_fence();
    const long long a = (long long)chunk * p.chunk;
    const long long b = a + p.chunk < p.N ? a + p.chunk : p.N;
    for (long long base = a; base < b; base += 64) {
        const long long i = base + lane;
        const int e = i < b ? p.idx[i] : -1;
        const bool valid = (unsigned)e < (unsigned)p.E;
        int rank, c;
        moe_match(e, valid, lane, rank, c);
        if (valid && rank == 0) cnt_all[wave][e] += c;              // one lane per distinct expert
        wave_lds_fence();
    }
    int32_t* __restrict__ hist = p.hist + (size_t)chunk * p.E;
    for (int e = lane; e < p.E; e += 64) hist[e] = cnt_all[wave][e];
}

// inclusive scan of one value per thread over a workgroup of NT threads
template <int NT> NNOP_DEV int block_inclusive_scan(int v, int32_t* sm) {
    const int tid = threadIdx.x;
    sm[tid] = v;
    __syncthreads();
#pragma unroll
    for (int off = 1; off < NT; off <<= 1) {
        const int add = tid >= off ? sm[tid - off] : 0;
        __syncthreads();
        sm[tid] += add;
        __syncthreads();
    }
    return sm[tid];
}

__global__ __launch_bounds__(256) void moe_plan_colscan_kernel(const MoePlanParams p) {
    __shared__ int32_t sm[256];
    const int e = blockIdx.x, tid = threadIdx.x;
    const int run = (p.n_chunks + 255) / 256;
    const int c0 = tid * run < p.n_chunks ? tid * run : p.n_chunks;
    const int c1 = c0 + run < p.n_chunks ? c0 + run : p.n_chunks;
    int32_t* col = p.hist + e;
    int s = 0;
    for (int c = c0; c < c1; ++c) s += col[(size_t)c * p.E];
    const int incl = block_inclusive_scan<256>(s, sm);
    int at = incl - s;
    for (int c = c0; c < c1; ++c) {
        const int v = col[(size_t)c * p.E];
        col[(size_t)c * p.E] = at;
        at += v;
    }
    if (tid == 255) p.counts[e] = incl;
}

__global__ __launch_bounds__(kMoeMaxExperts) void moe_plan_escan_kernel(const MoePlanParams p) {
    __shared__ int32_t sm[kMoeMaxExperts];
    const int tid = threadIdx.x;
    const int v = tid < p.E ? p.counts[tid] : 0;
    const int incl = block_inclusive_scan<kMoeMaxExperts>(v, sm);
    if (tid < p.E) p.offsets[tid] = incl - v;
    if (tid == kMoeMaxExperts - 1) p.offsets[p.E] = incl;
}

__global__ __launch_bounds__(kPlanWaves * 64) void moe_plan_scatter_kernel(const MoePlanParams p) {
    __shared__ int32_t pos_all[kPlanWaves][kMoeMaxExperts];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int chunk = blockIdx.x * kPlanWaves + wave;
    if (chunk >= p.n_chunks) return;                                // a whole wave; there is no barrier in this kernel
    const int32_t* __restrict__ hist = p.hist + (size_t)chunk * p.E;
    for (int e = lane; e < p.E; e += 64) pos_all[wave][e] = p.offsets[e] + hist[e];
    wave_lds_fence();
    const int total = p.offsets[p.E];
    const long long a = (long long)chunk * p.chunk;
    const long long b = a + p.chunk < p.N ? a + p.chunk : p.N;
    for (long long base = a; base < b; base += 64) {
        const long long i = base + lane;
        const int e = i < b ? p.idx[i] : -1;
        const bool valid = (unsigned)e < (unsigned)p.E;
        int rank, c;
        moe_match(e, valid, lane, rank, c);
        int at = -1;
        if (valid) at = pos_all[wave][e] + rank;                    // every lane of an expert reads before its first lane writes
        wave_lds_fence();
        if (valid && rank == 0) pos_all[wave][e] = at + c;
        wave_lds_fence();
        if (i < b) {
            p.slot[i] = at;
            if (valid && (long long)at < p.N) p.perm[at] = (int32_t)i;   // at < total <= N unless idx changed between the passes
            if (i >= total) p.perm[i] = -1;                         // the tail: positions no valid entry is sent to
        }
    }
}

int launch_moe_plan(const nnop_moe_plan_desc& d, int32_t* counts, int32_t* offsets, int32_t* perm, int32_t* slot, const int32_t* idx,
                    void* workspace, hipStream_t s) {
    MoePlanParams p{};
    p.idx = idx; p.counts = counts; p.offsets = offsets; p.perm = perm; p.slot = slot; p.hist = (int32_t*)workspace;
    p.N = (long long)d.tokens * d.topk;
    p.E = d.experts;
    moe_plan_chunks(p.N, p.chunk, p.n_chunks);
    const dim3 waves((unsigned)((p.n_chunks + kPlanWaves - 1) / kPlanWaves));
    hipLaunchKernelGGL(moe_plan_hist_kernel, waves, dim3(kPlanWaves * 64), 0, s, p);
    hipLaunchKernelGGL(moe_plan_colscan_kernel, dim3((unsigned)p.E), dim3(256), 0, s, p);
    hipLaunchKernelGGL(moe_plan_escan_kernel, dim3(1), dim3(kMoeMaxExperts), 0, s, p);
    hipLaunchKernelGGL(moe_plan_scatter_kernel, waves, dim3(kPlanWaves * 64), 0, s, p);
    return hipGetLastError() == hipSuccess ? NNOP_OK : NNOP_ERR_HIP;
}

}  // namespace nnop
