// nnop_paged_kv_write_capi.cpp -- the extern "C" boundary of libnnop_hip_paged_kv_write.so, declared in include/nnop_hip_paged_kv_write.h.
//
// Every argument check happens here, in the header's order, before anything touches the device.  The library exports these two
// functions and nothing else (nnop_paged_kv_write.map); it links nothing from the other sixteen libraries.
#include "paged_kv_write.hpp"
#include "host_common.hpp"

#define NNOP_PAGED_KV_WRITE_API extern "C" __attribute__((visibility("default")))

namespace nnop {

static int check_desc(const nnop_paged_kv_write_desc* d, bool scales) {
    if (!d) return NNOP_ERR_NULL;
    if (d->dtype != NNOP_F16 && d->dtype != NNOP_BF16) return NNOP_ERR_DTYPE;
    if (d->flags != 0 || d->reserved != 0 || d->reserved2 != 0) return NNOP_ERR_OPTS;
    if (d->kv_format != NNOP_PAGED_KV_WRITE_16BIT && d->kv_format != NNOP_PAGED_KV_WRITE_E4M3) return NNOP_ERR_OPTS;
    if (scales && d->kv_format == NNOP_PAGED_KV_WRITE_16BIT) return NNOP_ERR_OPTS;
    if (d->emb != 64 && d->emb != 128) return NNOP_ERR_SHAPE;
    if (d->tokens < 1 || d->batch < 1 || d->kh < 1) return NNOP_ERR_SHAPE;
    if ((long long)d->kh * d->emb > 0x7fffffffLL) return NNOP_ERR_SHAPE;
    if (d->page_size < NNOP_PAGED_KV_WRITE_MIN_PAGE_SIZE || (d->page_size & (d->page_size - 1)) != 0) return NNOP_ERR_SHAPE;
    if (d->max_pages < 1 || d->num_pages < 1) return NNOP_ERR_SHAPE;
    if ((long long)d->max_pages * d->page_size > 0x7fffffffLL) return NNOP_ERR_SHAPE;
    const int unit = d->kv_format == NNOP_PAGED_KV_WRITE_E4M3 ? 16 : 8;  // 16 bytes in pool elements
    for (int64_t s : {d->kp_stride_p, d->kp_stride_h, d->kp_stride_l, d->vp_stride_p, d->vp_stride_h, d->vp_stride_l})
        if (s < d->emb || s % unit != 0) return NNOP_ERR_SHAPE;
    for (int64_t s : {d->k_stride_h, d->v_stride_h})
        if (s < d->emb || s % 8 != 0) return NNOP_ERR_SHAPE;
    for (int64_t s : {d->k_stride_t, d->v_stride_t})
        if (s < (int64_t)d->kh * d->emb || s % 8 != 0) return NNOP_ERR_SHAPE;
    if (d->table_stride < d->max_pages) return NNOP_ERR_SHAPE;
    return NNOP_OK;
}

}  // namespace nnop

using namespace nnop;

NNOP_PAGED_KV_WRITE_API int nnop_paged_kv_write_abi_version(void) { return NNOP_HIP_PAGED_KV_WRITE_ABI_VERSION; }

NNOP_PAGED_KV_WRITE_API int nnop_paged_kv_write(const nnop_paged_kv_write_desc* d, void* k_pages, void* v_pages, const void* k, const void* v,
                                                const float* k_scale, const float* v_scale, const int32_t* block_table,
                                                const int32_t* cu_seqlens_q, const int32_t* seqlens, nnop_stream_t stream) {
    int st = check_desc(d, k_scale || v_scale);
    if (st != NNOP_OK) return st;
    st = check_ptrs({{{k_pages, v_pages, k, v}, 16}, {{block_table, cu_seqlens_q, seqlens}, 4}});
    if (st != NNOP_OK) return st;
    for (const void* opt : {(const void*)k_scale, (const void*)v_scale})
        if (misaligned(opt, 4)) return NNOP_ERR_ALIGN;  // the optional ones: NULL is aligned
    return launch_paged_kv_write(*d, k_pages, v_pages, k, v, k_scale, v_scale, block_table, cu_seqlens_q, seqlens, (hipStream_t)stream);
}
