// paged_prefill.hip -- the kernel of libnnop_hip_paged_prefill.so (include/nnop_hip_paged_prefill.h): attention of a variable number of
// new tokens per sequence over a KV cache kept as a pool of pages with an int32 block table per sequence.
//
// The kernel's text -- the work split, the address path, the two LDS images of K and of V, the transposed scores on the 32x32x16 MFMA,
// the base-2 softmax and the epilogue -- is paged_prefill_kernel.hpp's, which explains it; libnnop_hip_paged_prefill_fp8.so
// instantiates the same text with another staging policy (header-only: nothing is linked).  This library stages 16-bit pages
// (PpStage16): a thread moves E / 64 16-byte chunks of K and as many of V per tile, from the page row into the image as they are.
#include "paged_prefill_kernel.hpp"
#include "host_common.hpp"

namespace nnop {
namespace {

template <typename T, int E>
__global__ __launch_bounds__(kPpThreads) __attribute__((amdgpu_waves_per_eu(2, 2))) void paged_prefill_kernel(const PpParams p) {
    paged_prefill_body<T, E, PpStage16<T, E>>(p);
}

template <typename T, int E> int launch(const PpParams& p, long long groups, hipStream_t s) {
    hipLaunchKernelGGL((paged_prefill_kernel<T, E>), dim3((unsigned)groups), dim3(kPpThreads), 0, s, p);
    return hipGetLastError() == hipSuccess ? (int)NNOP_OK : (int)NNOP_ERR_HIP;
}

}  // namespace

int launch_paged_prefill(const nnop_paged_prefill_desc& d, void* o, float* lse, const void* q, const void* k, const void* v,
                         const int32_t* block_table, const int32_t* cu_seqlens_q, const int32_t* seqlens, const float* sinks,
                         hipStream_t stream) {
    PpParams p;
    p.o = o, p.lse = lse, p.q = q, p.k = k, p.v = v, p.table = block_table, p.cu = cu_seqlens_q, p.seqlens = seqlens, p.sinks = sinks;
    paged_prefill_fill(p, d);
    const long long groups = d.kh * paged_prefill_max_blocks(d);
    if (d.dtype == NNOP_BF16) return d.emb == 64 ? launch<__bf16, 64>(p, groups, stream) : launch<__bf16, 128>(p, groups, stream);
    return d.emb == 64 ? launch<_Float16, 64>(p, groups, stream) : launch<_Float16, 128>(p, groups, stream);
}

}  // namespace nnop
