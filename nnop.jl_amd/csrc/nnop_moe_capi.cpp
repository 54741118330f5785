// nnop_moe_capi.cpp -- the extern "C" boundary of libnnop_hip_moe.so, declared in include/nnop_hip_moe.h.
//
// Every argument check happens here, in the header's order, before anything touches the device.  The library exports these five
// functions and nothing else (nnop_moe.map); it links nothing from libnnop_hip.so or libnnop_hip_ext.so.
#include "moe.hpp"
#include "host_common.hpp"

#define NNOP_MOE_API extern "C" __attribute__((visibility("default")))

namespace nnop {

// dtype, then options, then shape (the descriptor must not be NULL)
static int check_router_desc(const nnop_moe_router_desc* d) {
    if (!known_dtype(d->dtype)) return NNOP_ERR_DTYPE;
    if (d->norm != NNOP_MOE_NORM_TOPK && d->norm != NNOP_MOE_NORM_ALL) return NNOP_ERR_OPTS;
    if (d->reserved[0] != 0 || d->reserved[1] != 0) return NNOP_ERR_OPTS;
    if (d->experts < 1 || d->experts > kMoeMaxExperts) return NNOP_ERR_SHAPE;
    if (d->topk < 1 || d->topk > kMoeMaxTopk || d->topk > d->experts) return NNOP_ERR_SHAPE;
    if (d->tokens < 1 || d->ld < d->experts) return NNOP_ERR_SHAPE;
    if ((long long)d->tokens * d->topk > 0x7fffffffLL) return NNOP_ERR_SHAPE;
    return NNOP_OK;
}

// options, then shape
static int check_plan_desc(const nnop_moe_plan_desc* d) {
    if (d->reserved[0] != 0) return NNOP_ERR_OPTS;
    if (d->tokens < 1 || d->topk < 1 || d->experts < 1 || d->experts > kMoeMaxExperts) return NNOP_ERR_SHAPE;
    if ((long long)d->tokens * d->topk > 0x7fffffffLL) return NNOP_ERR_SHAPE;
    return NNOP_OK;
}

}  // namespace nnop

using namespace nnop;

NNOP_MOE_API int nnop_moe_abi_version(void) { return NNOP_HIP_MOE_ABI_VERSION; }

NNOP_MOE_API int nnop_moe_router(const nnop_moe_router_desc* d, int32_t* idx, float* w, float* lse, const void* logits,
                                 nnop_stream_t stream) {
    if (!d) return NNOP_ERR_NULL;
    int st = check_router_desc(d);
    if (st != NNOP_OK) return st;
    st = check_ptrs({{{logits}, dtype_bytes(d->dtype)}, {{idx, w, lse}, 4}});
    if (st != NNOP_OK) return st;
    return launch_moe_router_fwd(*d, idx, w, lse, logits, (hipStream_t)stream);
}

NNOP_MOE_API int nnop_moe_router_bwd(const nnop_moe_router_desc* d, void* dlogits, const float* dw, const float* dlse, const float* w,
                                     const int32_t* idx, const float* lse, const void* logits, nnop_stream_t stream) {
    if (!d) return NNOP_ERR_NULL;
    int st = check_router_desc(d);
    if (st != NNOP_OK) return st;
    st = check_ptrs({{{dlogits, logits}, dtype_bytes(d->dtype)}, {{dw, w, idx, lse}, 4}});
    if (st != NNOP_OK) return st;
    if (misaligned(dlse, 4)) return NNOP_ERR_ALIGN;                 // optional: NULL counts as 0, and as aligned
    return launch_moe_router_bwd(*d, dlogits, dw, dlse, w, idx, lse, logits, (hipStream_t)stream);
}

NNOP_MOE_API size_t nnop_moe_plan_workspace_bytes(const nnop_moe_plan_desc* d) {
    if (!d || check_plan_desc(d) != NNOP_OK) return 0;
    return moe_plan_ws_bytes(*d);
}

NNOP_MOE_API int nnop_moe_plan(const nnop_moe_plan_desc* d, int32_t* counts, int32_t* offsets, int32_t* perm, int32_t* slot,
                               const int32_t* idx, void* workspace, size_t workspace_bytes, nnop_stream_t stream) {
    if (!d) return NNOP_ERR_NULL;
    int st = check_plan_desc(d);
    if (st != NNOP_OK) return st;
    st = check_ptrs({{{counts, offsets, perm, slot, idx}, 4}, {{workspace}, 16}});
    if (st != NNOP_OK) return st;
    if (workspace_bytes < moe_plan_ws_bytes(*d)) return NNOP_ERR_WORKSPACE;
    return launch_moe_plan(*d, counts, offsets, perm, slot, idx, workspace, (hipStream_t)stream);
}
