// nnop_paged_prefill_fp8_capi.cpp -- the extern "C" boundary of libnnop_hip_paged_prefill_fp8.so, declared in
// include/nnop_hip_paged_prefill_fp8.h.
//
// Every argument check happens here, in the header's order, before anything touches the device: the thirteenth library's checks with the
// fourteenth's additions (kv_format, pool strides in bytes and multiples of 16, the two scales among the optional pointers).  The
// library exports these three functions and nothing else (nnop_paged_prefill_fp8.map); it links nothing from the other fourteen.
#include "paged_prefill_fp8.hpp"
#include "host_common.hpp"

#define NNOP_PAGED_PREFILL_FP8_API extern "C" __attribute__((visibility("default")))

namespace nnop {

static int check_desc(const nnop_paged_prefill_fp8_desc* d) {
    if (!d) return NNOP_ERR_NULL;
    if (d->dtype != NNOP_F16 && d->dtype != NNOP_BF16) return NNOP_ERR_DTYPE;
    if (d->flags != 0 || d->kv_format != NNOP_PAGED_PREFILL_FP8_E4M3 || d->reserved != 0 || d->reserved2 != 0) return NNOP_ERR_OPTS;
    if (d->window_left < -1) return NNOP_ERR_OPTS;
    if (d->emb != 64 && d->emb != 128) return NNOP_ERR_SHAPE;
    if (d->tokens < 1 || d->batch < 1 || d->qh < 1 || d->kh < 1 || d->qh % d->kh != 0) return NNOP_ERR_SHAPE;
    if (d->qh / d->kh > NNOP_PAGED_PREFILL_FP8_MAX_GROUP) return NNOP_ERR_SHAPE;
    if (d->page_size < NNOP_PAGED_PREFILL_FP8_MIN_PAGE_SIZE || (d->page_size & (d->page_size - 1)) != 0) return NNOP_ERR_SHAPE;
    if (d->max_pages < 1 || d->num_pages < 1) return NNOP_ERR_SHAPE;
    if ((long long)d->max_pages * d->page_size > 0x7fffffffLL) return NNOP_ERR_SHAPE;
    for (int64_t s : {d->k_stride_p, d->k_stride_h, d->k_stride_l, d->v_stride_p, d->v_stride_h, d->v_stride_l})  // bytes
        if (s < d->emb || s % 16 != 0) return NNOP_ERR_SHAPE;
    for (int64_t s : {d->q_stride_h, d->o_stride_h})  // elements
        if (s < d->emb || s % 8 != 0) return NNOP_ERR_SHAPE;
    for (int64_t s : {d->q_stride_t, d->o_stride_t})
        if (s < (int64_t)d->qh * d->emb || s % 8 != 0) return NNOP_ERR_SHAPE;
    if (d->table_stride < d->max_pages) return NNOP_ERR_SHAPE;
    if (d->kh * paged_prefill_max_blocks(*d) > 0x7fffffffLL) return NNOP_ERR_SHAPE;  // the grid
    if ((long long)d->tokens * d->qh > 0x7fffffffLL) return NNOP_ERR_SHAPE;           // the rows of lse
    return NNOP_OK;
}

}  // namespace nnop

using namespace nnop;

NNOP_PAGED_PREFILL_FP8_API int nnop_paged_prefill_fp8_abi_version(void) { return NNOP_HIP_PAGED_PREFILL_FP8_ABI_VERSION; }

NNOP_PAGED_PREFILL_FP8_API int nnop_paged_prefill_fp8_plan(const nnop_paged_prefill_fp8_desc* d, size_t* workspace_bytes_out) {
    if (!workspace_bytes_out) return NNOP_ERR_NULL;
    const int st = check_desc(d);
    if (st != NNOP_OK) return st;
    *workspace_bytes_out = 0;  // a workgroup finds its block by a search over cu_seqlens_q: no list is kept
    return NNOP_OK;
}

NNOP_PAGED_PREFILL_FP8_API int nnop_paged_prefill_fp8(const nnop_paged_prefill_fp8_desc* d, void* o, float* lse, const void* q, const void* k,
                                                      const void* v, const float* k_scale, const float* v_scale,
                                                      const int32_t* block_table, const int32_t* cu_seqlens_q, const int32_t* seqlens,
                                                      const float* sinks, void* workspace, size_t workspace_bytes, nnop_stream_t stream) {
    int st = check_desc(d);
    if (st != NNOP_OK) return st;
    st = check_ptrs({{{o, q, k, v}, 16}, {{block_table, cu_seqlens_q, seqlens}, 4}});
    if (st != NNOP_OK) return st;
    for (const void* opt : {(const void*)lse, (const void*)k_scale, (const void*)v_scale, (const void*)sinks, (const void*)workspace})
        if (misaligned(opt, 4)) return NNOP_ERR_ALIGN;  // the optional ones: NULL is aligned
    (void)workspace_bytes;  // 0 are needed
    return launch_paged_prefill_fp8(*d, o, lse, q, k, v, k_scale, v_scale, block_table, cu_seqlens_q, seqlens, sinks, (hipStream_t)stream);
}
