// nnop_mla_decode_capi.cpp -- the extern "C" boundary of libnnop_hip_mla_decode.so, declared in include/nnop_hip_mla_decode.h.
//
// Every argument check happens here, in the header's order, before anything touches the device.  The library exports these three
// functions and nothing else (nnop_mla_decode.map); it links nothing from the other seventeen libraries.
#include "mla_decode.hpp"
#include "host_common.hpp"

#define NNOP_MLA_DECODE_API extern "C" __attribute__((visibility("default")))

namespace nnop {

static int check_desc(const nnop_mla_decode_desc* d) {
    if (!d) return NNOP_ERR_NULL;
    if (d->dtype != NNOP_F16 && d->dtype != NNOP_BF16) return NNOP_ERR_DTYPE;
    if (d->flags != 0 || d->reserved0 != 0 || d->reserved1 != 0) return NNOP_ERR_OPTS;
    if (d->splits < 0 || d->splits > kMlaMaxSplits) return NNOP_ERR_OPTS;
    if (!finite(d->softmax_scale) || !(d->softmax_scale > 0.f)) return NNOP_ERR_OPTS;
    if (d->batch < 1 || d->ql < 1 || d->ql > NNOP_MLA_DECODE_MAX_QL) return NNOP_ERR_SHAPE;
    if (d->qh < 16 || d->qh > NNOP_MLA_DECODE_MAX_HEADS || d->qh % 16 != 0) return NNOP_ERR_SHAPE;
    if (d->page_size < NNOP_MLA_DECODE_MIN_PAGE_SIZE || (d->page_size & (d->page_size - 1)) != 0) return NNOP_ERR_SHAPE;
    if (d->max_pages < 1 || d->num_pages < 1) return NNOP_ERR_SHAPE;
    const long long cap = (long long)d->max_pages * d->page_size;
    if (cap > 0x7fffffffLL || cap < d->ql) return NNOP_ERR_SHAPE;
    for (int64_t s : {d->q_stride_b, d->q_stride_h, d->q_stride_l, d->kv_stride_p, d->kv_stride_l})
        if (s < kMlaW || s % 8 != 0) return NNOP_ERR_SHAPE;
    if (d->table_stride < d->max_pages) return NNOP_ERR_SHAPE;
    if ((long long)d->batch * d->ql * mla_decode_head_blocks(*d) * mla_decode_splits(*d) > 0x7fffffffLL) return NNOP_ERR_SHAPE;  // the chunks' grid
    if ((long long)d->batch * d->qh * d->ql > 0x7fffffffLL) return NNOP_ERR_SHAPE;  // the grid of the merge: rows of o
    return NNOP_OK;
}

}  // namespace nnop

using namespace nnop;

NNOP_MLA_DECODE_API int nnop_mla_decode_abi_version(void) { return NNOP_HIP_MLA_DECODE_ABI_VERSION; }

NNOP_MLA_DECODE_API int nnop_mla_decode_plan(const nnop_mla_decode_desc* d, int32_t* splits_out, size_t* workspace_bytes_out) {
    if (!splits_out || !workspace_bytes_out) return NNOP_ERR_NULL;
    const int st = check_desc(d);
    if (st != NNOP_OK) return st;
    *splits_out = mla_decode_splits(*d);
    *workspace_bytes_out = mla_decode_workspace_bytes(*d, *splits_out);
    return NNOP_OK;
}

NNOP_MLA_DECODE_API int nnop_mla_decode(const nnop_mla_decode_desc* d, void* o, float* lse, const void* q, const void* kv,
                                        const int32_t* block_table, const int32_t* seqlens, void* workspace, size_t workspace_bytes,
                                        nnop_stream_t stream) {
    int st = check_desc(d);
    if (st != NNOP_OK) return st;
    const int splits = mla_decode_splits(*d);
    const size_t need = mla_decode_workspace_bytes(*d, splits);
    st = check_ptrs({{{o, q, kv}, 16}, {{block_table, seqlens}, 4}}, [&] { return need > 0 && !workspace ? (int)NNOP_ERR_NULL : (int)NNOP_OK; });
    if (st != NNOP_OK) return st;
    for (const void* opt : {(const void*)lse, (const void*)workspace})
        if (misaligned(opt, 4)) return NNOP_ERR_ALIGN;  // the optional ones: NULL is aligned
    if (workspace_bytes < need) return NNOP_ERR_WORKSPACE;
    return launch_mla_decode(*d, splits, o, lse, q, kv, block_table, seqlens, (float*)workspace, (hipStream_t)stream);
}
