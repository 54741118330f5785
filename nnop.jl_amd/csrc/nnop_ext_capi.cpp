// nnop_ext_capi.cpp -- the extern "C" boundary of libnnop_hip_ext.so, declared in include/nnop_hip_ext.h.
//
// Every argument check happens here, in the header's order, before anything touches the device.  The library exports these four
// functions and nothing else (nnop_ext.map); it links nothing from libnnop_hip.so.
#include "qk_norm_rope.hpp"
#include <stdint.h>

#define NNOP_EXT_API extern "C" __attribute__((visibility("default")))

namespace nnop {

static inline bool known_dtype(int32_t t) { return t == NNOP_F32 || t == NNOP_F16 || t == NNOP_BF16; }
static inline size_t dtype_bytes(int32_t t) { return t == NNOP_F32 ? 4 : 2; }
static inline bool misaligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

// dtype, then options, then shape (the descriptor must not be NULL)
static int check_qknr_desc(const nnop_qknr_desc* d) {
    if (!known_dtype(d->dtype) || !known_dtype(d->w_dtype) || !known_dtype(d->cs_dtype)) return NNOP_ERR_DTYPE;
    if ((d->w_dtype != NNOP_F32 && d->w_dtype != d->dtype) || (d->cs_dtype != NNOP_F32 && d->cs_dtype != d->dtype)) return NNOP_ERR_DTYPE;
    if (d->reserved[0] != 0 || d->reserved[1] != 0) return NNOP_ERR_OPTS;
    if (!(d->eps >= 0.f && d->eps <= 3.4028234664e38f)) return NNOP_ERR_OPTS;                    // (the comparisons are false for NaN)
    if (!(d->offset >= -3.4028234664e38f && d->offset <= 3.4028234664e38f)) return NNOP_ERR_OPTS;
    if (d->dim <= 0 || (d->dim & 1) || d->dim > 512) return NNOP_ERR_SHAPE;
    if (d->seq <= 0 || d->qh <= 0 || d->kh <= 0 || d->batch <= 0) return NNOP_ERR_SHAPE;
    // one launch: the kernels index head rows with 32 bits
    const long long bl = (long long)d->batch * d->seq;                                           // < 2^62
    if (bl > 0x7fffffffLL || bl * ((long long)d->qh + d->kh) > 0x7fffffffLL) return NNOP_ERR_SHAPE;  // (the product < 2^63)
    return NNOP_OK;
}

// NULL, then alignment: `elems` are of dtype, `ws` of w_dtype, `cs` of cs_dtype, `f32s` fp32
static int check_qknr_ptrs(const nnop_qknr_desc* d, const void* const* elems, int n_elems, const void* const* ws,
                           const void* const* cs, const void* const* f32s, int n_f32s, const void* workspace, bool has_ws) {
    for (int i = 0; i < n_elems; ++i)
        if (!elems[i]) return NNOP_ERR_NULL;
    for (int i = 0; i < 2; ++i)
        if (!ws[i] || !cs[i]) return NNOP_ERR_NULL;
    for (int i = 0; i < n_f32s; ++i)
        if (!f32s[i]) return NNOP_ERR_NULL;
    if (has_ws && !workspace) return NNOP_ERR_NULL;
    for (int i = 0; i < n_elems; ++i)
        if (misaligned(elems[i], dtype_bytes(d->dtype))) return NNOP_ERR_ALIGN;
    for (int i = 0; i < 2; ++i)
        if (misaligned(ws[i], dtype_bytes(d->w_dtype)) || misaligned(cs[i], dtype_bytes(d->cs_dtype))) return NNOP_ERR_ALIGN;
    for (int i = 0; i < n_f32s; ++i)
        if (misaligned(f32s[i], sizeof(float))) return NNOP_ERR_ALIGN;
    if (has_ws && misaligned(workspace, 16)) return NNOP_ERR_ALIGN;
    return NNOP_OK;
}

}  // namespace nnop

using namespace nnop;

NNOP_EXT_API int nnop_ext_abi_version(void) { return NNOP_HIP_EXT_ABI_VERSION; }

NNOP_EXT_API int nnop_qk_norm_rope(const nnop_qknr_desc* d, void* q_out, void* k_out, const void* q, const void* k, const void* wq,
                                   const void* wk, const void* cos, const void* sin, nnop_stream_t stream) {
    if (!d) return NNOP_ERR_NULL;
    int st = check_qknr_desc(d);
    if (st != NNOP_OK) return st;
    const void* const elems[] = {q_out, k_out, q, k};
    const void* const ws[] = {wq, wk};
    const void* const cs[] = {cos, sin};
    st = check_qknr_ptrs(d, elems, 4, ws, cs, nullptr, 0, nullptr, false);
    if (st != NNOP_OK) return st;
    return launch_qknr_fwd(*d, q_out, k_out, q, k, wq, wk, cos, sin, (hipStream_t)stream);
}

NNOP_EXT_API size_t nnop_qk_norm_rope_bwd_workspace_bytes(const nnop_qknr_desc* d) {
    if (!d || check_qknr_desc(d) != NNOP_OK) return 0;
    return qknr_bwd_ws_bytes(*d);
}

NNOP_EXT_API int nnop_qk_norm_rope_bwd(const nnop_qknr_desc* d, void* dq, void* dk, float* dwq, float* dwk, const void* dq_out,
                                       const void* dk_out, const void* q, const void* k, const void* wq, const void* wk,
                                       const void* cos, const void* sin, void* workspace, size_t workspace_bytes,
                                       nnop_stream_t stream) {
    if (!d) return NNOP_ERR_NULL;
    int st = check_qknr_desc(d);
    if (st != NNOP_OK) return st;
    const void* const elems[] = {dq, dk, dq_out, dk_out, q, k};
    const void* const ws[] = {wq, wk};
    const void* const cs[] = {cos, sin};
    const void* const f32s[] = {dwq, dwk};
    st = check_qknr_ptrs(d, elems, 6, ws, cs, f32s, 2, workspace, true);
    if (st != NNOP_OK) return st;
    if (workspace_bytes < qknr_bwd_ws_bytes(*d)) return NNOP_ERR_WORKSPACE;
    return launch_qknr_bwd(*d, dq, dk, dwq, dwk, dq_out, dk_out, q, k, wq, wk, cos, sin, workspace, (hipStream_t)stream);
}
