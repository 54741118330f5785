// nnop_paged_prefill_split_capi.cpp -- the extern "C" boundary of libnnop_hip_paged_prefill_split.so, declared in
// include/nnop_hip_paged_prefill_split.h.
//
// Every argument check happens here, in the header's order, before anything touches the device.  The library exports these three
// functions and nothing else (nnop_paged_prefill_split.map); it links nothing from the other fifteen libraries.  The checks are the
// thirteenth library's with `reserved` read as the split count.
#include "paged_prefill_split.hpp"
#include "host_common.hpp"

#define NNOP_PAGED_PREFILL_SPLIT_API extern "C" __attribute__((visibility("default")))

namespace nnop {

static int check_desc(const nnop_paged_prefill_desc* d) {
    if (!d) return NNOP_ERR_NULL;
    if (d->dtype != NNOP_F16 && d->dtype != NNOP_BF16) return NNOP_ERR_DTYPE;
    if (d->flags != 0 || d->reserved < 0 || d->reserved > kPpsMaxSplits) return NNOP_ERR_OPTS;
    if (d->window_left < -1) return NNOP_ERR_OPTS;
    if (d->emb != 64 && d->emb != 128) return NNOP_ERR_SHAPE;
    if (d->tokens < 1 || d->batch < 1 || d->qh < 1 || d->kh < 1 || d->qh % d->kh != 0) return NNOP_ERR_SHAPE;
    if (d->qh / d->kh > NNOP_PAGED_PREFILL_MAX_GROUP) return NNOP_ERR_SHAPE;
    if (d->page_size < NNOP_PAGED_PREFILL_MIN_PAGE_SIZE || (d->page_size & (d->page_size - 1)) != 0) return NNOP_ERR_SHAPE;
    if (d->max_pages < 1 || d->num_pages < 1) return NNOP_ERR_SHAPE;
    if ((long long)d->max_pages * d->page_size > 0x7fffffffLL) return NNOP_ERR_SHAPE;
    for (int64_t s : {d->k_stride_p, d->k_stride_h, d->k_stride_l, d->v_stride_p, d->v_stride_h, d->v_stride_l, d->q_stride_h, d->o_stride_h})
        if (s < d->emb || s % 8 != 0) return NNOP_ERR_SHAPE;
    for (int64_t s : {d->q_stride_t, d->o_stride_t})
        if (s < (int64_t)d->qh * d->emb || s % 8 != 0) return NNOP_ERR_SHAPE;
    if (d->table_stride < d->max_pages) return NNOP_ERR_SHAPE;
    if (d->kh * paged_prefill_max_blocks(*d) * paged_prefill_splits(*d) > 0x7fffffffLL) return NNOP_ERR_SHAPE;  // the grid of pass 1
    if ((long long)d->tokens * d->qh > 0x7fffffffLL) return NNOP_ERR_SHAPE;  // the rows of lse and of the merge
    return NNOP_OK;
}

}  // namespace nnop

using namespace nnop;

NNOP_PAGED_PREFILL_SPLIT_API int nnop_paged_prefill_split_abi_version(void) { return NNOP_HIP_PAGED_PREFILL_SPLIT_ABI_VERSION; }

NNOP_PAGED_PREFILL_SPLIT_API int nnop_paged_prefill_split_plan(const nnop_paged_prefill_desc* d, int32_t* splits_out,
                                                               size_t* workspace_bytes_out) {
    if (!splits_out || !workspace_bytes_out) return NNOP_ERR_NULL;
    const int st = check_desc(d);
    if (st != NNOP_OK) return st;
    *splits_out = paged_prefill_splits(*d);
    *workspace_bytes_out = paged_prefill_split_workspace_bytes(*d, *splits_out);
    return NNOP_OK;
}

NNOP_PAGED_PREFILL_SPLIT_API int nnop_paged_prefill_split(const nnop_paged_prefill_desc* d, void* o, float* lse, const void* q,
                                                          const void* k, const void* v, const int32_t* block_table,
                                                          const int32_t* cu_seqlens_q, const int32_t* seqlens, const float* sinks,
                                                          void* workspace, size_t workspace_bytes, nnop_stream_t stream) {
    int st = check_desc(d);
    if (st != NNOP_OK) return st;
    const int splits = paged_prefill_splits(*d);
    const size_t need = paged_prefill_split_workspace_bytes(*d, splits);
    st = check_ptrs({{{o, q, k, v}, 16}, {{block_table, cu_seqlens_q, seqlens}, 4}},
                    [&] { return need > 0 && !workspace ? (int)NNOP_ERR_NULL : (int)NNOP_OK; });
    if (st != NNOP_OK) return st;
    for (const void* opt : {(const void*)lse, (const void*)sinks})
        if (misaligned(opt, 4)) return NNOP_ERR_ALIGN;  // the optional ones: NULL is aligned
    if (misaligned(workspace, 16)) return NNOP_ERR_ALIGN;
    if (workspace_bytes < need) return NNOP_ERR_WORKSPACE;
    return launch_paged_prefill_split(*d, splits, o, lse, q, k, v, block_table, cu_seqlens_q, seqlens, sinks,
                                      need ? (float*)workspace : nullptr, (hipStream_t)stream);
}
