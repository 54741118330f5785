// nnop_moe_capi.cpp -- the extern "C" boundary of libnnop_hip_moe.so, declared in include/nnop_hip_moe.h.
//
// Every argument check happens here, in the header's order, before anything touches the device.  The library exports these five
// functions and nothing else (nnop_moe.map); it links nothing from libnnop_hip.so or libnnop_hip_ext.so.
#include "moe.hpp"
#include <stdint.h>

#define NNOP_MOE_API extern "C" __attribute__((visibility("default")))

namespace nnop {

static inline bool known_dtype(int32_t t) { return t == NNOP_F32 || t == NNOP_F16 || t == NNOP_BF16; }
static inline size_t dtype_bytes(int32_t t) { return t == NNOP_F32 ? 4 : 2; }
static inline bool misaligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

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

// NULL, then alignment: `elems` are of dtype, `words` fp32 or int32
static int check_ptrs(int32_t dtype, const void* const* elems, int n_elems, const void* const* words, int n_words) {
    for (int i = 0; i < n_elems; ++i)
        if (!elems[i]) return NNOP_ERR_NULL;
    for (int i = 0; i < n_words; ++i)
        if (!words[i]) return NNOP_ERR_NULL;
    for (int i = 0; i < n_elems; ++i)
        if (misaligned(elems[i], dtype_bytes(dtype))) return NNOP_ERR_ALIGN;
    for (int i = 0; i < n_words; ++i)
        if (misaligned(words[i], 4)) return NNOP_ERR_ALIGN;
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
    const void* const elems[] = {logits};
    const void* const words[] = {idx, w, lse};
    st = check_ptrs(d->dtype, elems, 1, words, 3);
    if (st != NNOP_OK) return st;
    return launch_moe_router_fwd(*d, idx, w, lse, logits, (hipStream_t)stream);
}

NNOP_MOE_API int nnop_moe_router_bwd(const nnop_moe_router_desc* d, void* dlogits, const float* dw, const float* dlse, const float* w,
                                     const int32_t* idx, const float* lse, const void* logits, nnop_stream_t stream) {
    if (!d) return NNOP_ERR_NULL;
    int st = check_router_desc(d);
    if (st != NNOP_OK) return st;
    const void* const elems[] = {dlogits, logits};
    const void* const words[] = {dw, w, idx, lse};
    st = check_ptrs(d->dtype, elems, 2, words, 4);
    if (st != NNOP_OK) return st;
    if (dlse && misaligned(dlse, 4)) return NNOP_ERR_ALIGN;         // optional: NULL counts as 0
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
    const void* const words[] = {counts, offsets, perm, slot, idx};
    for (const void* q : words)
        if (!q) return NNOP_ERR_NULL;
    if (!workspace) return NNOP_ERR_NULL;
    for (const void* q : words)
        if (misaligned(q, 4)) return NNOP_ERR_ALIGN;
    if (misaligned(workspace, 16)) return NNOP_ERR_ALIGN;
    if (workspace_bytes < moe_plan_ws_bytes(*d)) return NNOP_ERR_WORKSPACE;
    return launch_moe_plan(*d, counts, offsets, perm, slot, idx, workspace, (hipStream_t)stream);
}
