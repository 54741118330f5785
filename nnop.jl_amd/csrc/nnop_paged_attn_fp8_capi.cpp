// nnop_paged_attn_fp8_capi.cpp -- the extern "C" boundary of libnnop_hip_paged_attn_fp8.so, declared in
// include/nnop_hip_paged_attn_fp8.h.
//
// Every argument check happens here, in the header's order, before anything touches the device.  The library exports these three
// functions and nothing else (nnop_paged_attn_fp8.map); it links nothing from the other thirteen libraries.  The split rule and the
// workspace formula are decode_attn.hpp's, read through a 16-bit dense descriptor of capacity max_pages page_size.
#include "paged_attn_fp8.hpp"
#include "host_common.hpp"

#define NNOP_PAGED_ATTN_FP8_API extern "C" __attribute__((visibility("default")))

namespace nnop {

static int check_desc(const nnop_paged_attn_fp8_desc* d) {
    if (!d) return NNOP_ERR_NULL;
    if (d->dtype != NNOP_F16 && d->dtype != NNOP_BF16) return NNOP_ERR_DTYPE;
    if (d->flags != 0 || d->kv_format != NNOP_PAGED_ATTN_FP8_E4M3 || d->reserved != 0) return NNOP_ERR_OPTS;
    if (d->window_left < -1 || d->splits < 0 || d->splits > kDaMaxSplits) return NNOP_ERR_OPTS;
    if (d->emb != 64 && d->emb != 128) return NNOP_ERR_SHAPE;
    if (d->batch < 1 || d->qh < 1 || d->kh < 1 || d->qh % d->kh != 0 || d->ql < 1) return NNOP_ERR_SHAPE;
    if ((long long)(d->qh / d->kh) * d->ql > kDaRows) return NNOP_ERR_SHAPE;
    if (d->page_size < NNOP_PAGED_ATTN_FP8_MIN_PAGE_SIZE || (d->page_size & (d->page_size - 1)) != 0) return NNOP_ERR_SHAPE;
    if (d->max_pages < 1 || d->num_pages < 1) return NNOP_ERR_SHAPE;
    const long long cap = (long long)d->max_pages * d->page_size;
    if (cap > 0x7fffffffLL || cap < d->ql) return NNOP_ERR_SHAPE;
    for (int64_t s : {d->k_stride_p, d->k_stride_h, d->k_stride_l, d->v_stride_p, d->v_stride_h, d->v_stride_l})
        if (s < d->emb || s % 16 != 0) return NNOP_ERR_SHAPE;
    for (int64_t s : {d->k_stride_l, d->v_stride_l})  // a lane's offset inside a page is 32 bits: (page_size - 1) s + emb <= 2^32 - 1
        if (s > (0xffffffffLL - d->emb) / (d->page_size - 1)) return NNOP_ERR_SHAPE;
    if (d->table_stride < d->max_pages) return NNOP_ERR_SHAPE;
    if ((long long)d->batch * d->kh * decode_attn_splits(paged_attn_fp8_as_dense(*d)) > 0x7fffffffLL) return NNOP_ERR_SHAPE;  // the chunks' grid
    if ((long long)d->batch * d->qh * d->ql > 0x7fffffffLL) return NNOP_ERR_SHAPE;  // the grid of the merge: rows of o
    return NNOP_OK;
}

}  // namespace nnop

using namespace nnop;

NNOP_PAGED_ATTN_FP8_API int nnop_paged_attn_fp8_abi_version(void) { return NNOP_HIP_PAGED_ATTN_FP8_ABI_VERSION; }

NNOP_PAGED_ATTN_FP8_API int nnop_paged_attn_fp8_plan(const nnop_paged_attn_fp8_desc* d, int32_t* splits_out, size_t* workspace_bytes_out) {
    if (!splits_out || !workspace_bytes_out) return NNOP_ERR_NULL;
    const int st = check_desc(d);
    if (st != NNOP_OK) return st;
    const nnop_decode_attn_desc dense = paged_attn_fp8_as_dense(*d);
    *splits_out = decode_attn_splits(dense);
    *workspace_bytes_out = decode_attn_workspace_bytes(dense, *splits_out);
    return NNOP_OK;
}

NNOP_PAGED_ATTN_FP8_API int nnop_paged_attn_fp8(const nnop_paged_attn_fp8_desc* d, void* o, float* lse, const void* q, const void* k,
                                                const void* v, const float* k_scale, const float* v_scale, const int32_t* block_table,
                                                const int32_t* seqlens, const float* sinks, void* workspace, size_t workspace_bytes,
                                                nnop_stream_t stream) {
    int st = check_desc(d);
    if (st != NNOP_OK) return st;
    const nnop_decode_attn_desc dense = paged_attn_fp8_as_dense(*d);
    const int splits = decode_attn_splits(dense);
    const size_t need = decode_attn_workspace_bytes(dense, splits);
    st = check_ptrs({{{o, q, k, v}, 16}, {{block_table, seqlens}, 4}}, [&] { return need > 0 && !workspace ? (int)NNOP_ERR_NULL : (int)NNOP_OK; });
    if (st != NNOP_OK) return st;
    for (const void* opt : {(const void*)lse, (const void*)k_scale, (const void*)v_scale, (const void*)sinks, (const void*)workspace})
        if (misaligned(opt, 4)) return NNOP_ERR_ALIGN;  // the optional ones: NULL is aligned
    if (workspace_bytes < need) return NNOP_ERR_WORKSPACE;
    return launch_paged_attn_fp8(*d, splits, o, lse, q, k, v, k_scale, v_scale, block_table, seqlens, sinks, (float*)workspace,
                                 (hipStream_t)stream);
}
