// nnop_decode_attn_fp8_capi.cpp -- the extern "C" boundary of libnnop_hip_decode_attn_fp8.so, declared in
// include/nnop_hip_decode_attn_fp8.h.
//
// Every argument check happens here, in the header's order, before anything touches the device.  The library exports these three
// functions and nothing else (nnop_decode_attn_fp8.map); it links nothing from the other ten libraries.  The split rule and the
// workspace formula are decode_attn.hpp's, read through the 16-bit descriptor of the same layout.
#include "decode_attn_fp8.hpp"
#include "host_common.hpp"

#define NNOP_DECODE_ATTN_FP8_API extern "C" __attribute__((visibility("default")))

namespace nnop {

static int check_desc(const nnop_decode_attn_fp8_desc* d) {
    if (!d) return NNOP_ERR_NULL;
    if (d->dtype != NNOP_F16 && d->dtype != NNOP_BF16) return NNOP_ERR_DTYPE;
    if (d->flags != 0 || d->kv_format != NNOP_DECODE_ATTN_FP8_E4M3 || d->reserved != 0) return NNOP_ERR_OPTS;
    if (d->window_left < -1 || d->splits < 0 || d->splits > kDaMaxSplits) return NNOP_ERR_OPTS;
    if (d->emb != 64 && d->emb != 128) return NNOP_ERR_SHAPE;
    if (d->batch < 1 || d->qh < 1 || d->kh < 1 || d->qh % d->kh != 0 || d->ql < 1) return NNOP_ERR_SHAPE;
    if ((long long)(d->qh / d->kh) * d->ql > kDaRows || d->capacity < d->ql) return NNOP_ERR_SHAPE;
    for (int64_t s : {d->k_stride_b, d->k_stride_h, d->k_stride_l, d->v_stride_b, d->v_stride_h, d->v_stride_l})
        if (s < d->emb || s % 16 != 0) return NNOP_ERR_SHAPE;
    if ((long long)d->batch * d->kh * decode_attn_splits(decode_attn_fp8_as_16bit(*d)) > 0x7fffffffLL) return NNOP_ERR_SHAPE;  // the chunks' grid
    if ((long long)d->batch * d->qh * d->ql > 0x7fffffffLL) return NNOP_ERR_SHAPE;  // the grid of the merge: rows of o
    return NNOP_OK;
}

}  // namespace nnop

using namespace nnop;

NNOP_DECODE_ATTN_FP8_API int nnop_decode_attn_fp8_abi_version(void) { return NNOP_HIP_DECODE_ATTN_FP8_ABI_VERSION; }

NNOP_DECODE_ATTN_FP8_API int nnop_decode_attn_fp8_plan(const nnop_decode_attn_fp8_desc* d, int32_t* splits_out, size_t* workspace_bytes_out) {
    if (!splits_out || !workspace_bytes_out) return NNOP_ERR_NULL;
    const int st = check_desc(d);
    if (st != NNOP_OK) return st;
    const nnop_decode_attn_desc d16 = decode_attn_fp8_as_16bit(*d);
    *splits_out = decode_attn_splits(d16);
    *workspace_bytes_out = decode_attn_workspace_bytes(d16, *splits_out);
    return NNOP_OK;
}

NNOP_DECODE_ATTN_FP8_API int nnop_decode_attn_fp8(const nnop_decode_attn_fp8_desc* d, void* o, float* lse, const void* q, const void* k,
                                                  const void* v, const float* k_scale, const float* v_scale, const int32_t* seqlens,
                                                  const float* sinks, void* workspace, size_t workspace_bytes, nnop_stream_t stream) {
    int st = check_desc(d);
    if (st != NNOP_OK) return st;
    const nnop_decode_attn_desc d16 = decode_attn_fp8_as_16bit(*d);
    const int splits = decode_attn_splits(d16);
    const size_t need = decode_attn_workspace_bytes(d16, splits);
    st = check_ptrs({{{o, q, k, v}, 16}, {{seqlens}, 4}}, [&] { return need > 0 && !workspace ? (int)NNOP_ERR_NULL : (int)NNOP_OK; });
    if (st != NNOP_OK) return st;
    for (const void* opt : {(const void*)lse, (const void*)k_scale, (const void*)v_scale, (const void*)sinks, (const void*)workspace})
        if (misaligned(opt, 4)) return NNOP_ERR_ALIGN;  // the optional ones: NULL is aligned
    if (workspace_bytes < need) return NNOP_ERR_WORKSPACE;
    return launch_decode_attn_fp8(*d, splits, o, lse, q, k, v, k_scale, v_scale, seqlens, sinks, (float*)workspace, (hipStream_t)stream);
}
