// nnop_ext_capi.cpp -- the extern "C" boundary of libnnop_hip_ext.so, declared in include/nnop_hip_ext.h.
//
// Every argument check happens here, in the header's order, before anything touches the device.  The library exports these four
// functions and nothing else (nnop_ext.map); it links nothing from libnnop_hip.so.
#include "qk_norm_rope.hpp"
#include "host_common.hpp"

#define NNOP_EXT_API extern "C" __attribute__((visibility("default")))

namespace nnop {

// dtype, then options, then shape (the descriptor must not be NULL)
static int check_qknr_desc(const nnop_qknr_desc* d) {
    if (!known_dtype(d->dtype) || !known_dtype(d->w_dtype) || !known_dtype(d->cs_dtype)) return NNOP_ERR_DTYPE;
    if ((d->w_dtype != NNOP_F32 && d->w_dtype != d->dtype) || (d->cs_dtype != NNOP_F32 && d->cs_dtype != d->dtype)) return NNOP_ERR_DTYPE;
    if (d->reserved[0] != 0 || d->reserved[1] != 0) return NNOP_ERR_OPTS;
    if (!finite_nonneg(d->eps) || !finite(d->offset)) return NNOP_ERR_OPTS;
    if (d->dim <= 0 || (d->dim & 1) || d->dim > 512) return NNOP_ERR_SHAPE;
    if (d->seq <= 0 || d->qh <= 0 || d->kh <= 0 || d->batch <= 0) return NNOP_ERR_SHAPE;
    // one launch: the kernels index head rows with 32 bits
    const long long bl = (long long)d->batch * d->seq;                                           // < 2^62
    if (bl > 0x7fffffffLL || bl * ((long long)d->qh + d->kh) > 0x7fffffffLL) return NNOP_ERR_SHAPE;  // (the product < 2^63)
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
    st = check_ptrs({{{q_out, k_out, q, k}, dtype_bytes(d->dtype)},
                     {{wq, wk}, dtype_bytes(d->w_dtype)},
                     {{cos, sin}, dtype_bytes(d->cs_dtype)}});
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
    st = check_ptrs({{{dq, dk, dq_out, dk_out, q, k}, dtype_bytes(d->dtype)},
                     {{wq, wk}, dtype_bytes(d->w_dtype)},
                     {{cos, sin}, dtype_bytes(d->cs_dtype)},
                     {{dwq, dwk}, sizeof(float)},
                     {{workspace}, 16}});
    if (st != NNOP_OK) return st;
    if (workspace_bytes < qknr_bwd_ws_bytes(*d)) return NNOP_ERR_WORKSPACE;
    return launch_qknr_bwd(*d, dq, dk, dwq, dwk, dq_out, dk_out, q, k, wq, wk, cos, sin, workspace, (hipStream_t)stream);
}
