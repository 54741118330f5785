// nnop_moe_linear_capi.cpp -- the extern "C" boundary of libnnop_hip_moe_linear.so, declared in include/nnop_hip_moe_linear.h.
//
// Every argument check happens here, in the header's order, before anything touches the device.  The library exports these five
// functions and nothing else (nnop_moe_linear.map); it links nothing from the other five libraries.
#include "moe_linear.hpp"
#include "host_common.hpp"

#define NNOP_MOE_LINEAR_API extern "C" __attribute__((visibility("default")))

namespace nnop {

// the descriptor itself, then dtype, options, shape: the same for the four calls.  The pointers are each call's own.
static int check_desc(MoeLinearCall which, const nnop_moe_linear_desc* d) {
    if (!d) return NNOP_ERR_NULL;
    if (!known_dtype(d->dtype)) return NNOP_ERR_DTYPE;
    if (d->grad_dtype != d->dtype && d->grad_dtype != NNOP_F32) return NNOP_ERR_DTYPE;
    if ((d->flags & ~(NNOP_MOE_LINEAR_KN | NNOP_MOE_LINEAR_ACCUMULATE)) != 0) return NNOP_ERR_OPTS;
    if (d->reserved[0] != 0 || d->reserved[1] != 0 || d->reserved[2] != 0) return NNOP_ERR_OPTS;
    if (d->rows < 1 || d->experts < 1 || d->experts > kMoeLinearMaxExperts) return NNOP_ERR_SHAPE;
    if (d->in_dim < 1 || d->in_dim > kMoeLinearMaxDim || d->out_dim < 1 || d->out_dim > kMoeLinearMaxDim) return NNOP_ERR_SHAPE;
    const int32_t wcols = (d->flags & NNOP_MOE_LINEAR_KN) ? d->out_dim : d->in_dim;
    if (d->ld_x < d->in_dim || d->ld_y < d->out_dim || d->ld_w < wcols || d->ld_dw < wcols) return NNOP_ERR_SHAPE;
    if (d->ld_b < d->out_dim || d->ld_db < d->out_dim) return NNOP_ERR_SHAPE;
    if (moe_linear_workgroups(which, *d) > 0x7fffffffLL) return NNOP_ERR_SHAPE;
    return NNOP_OK;
}

}  // namespace nnop

using namespace nnop;

NNOP_MOE_LINEAR_API int nnop_moe_linear_abi_version(void) { return NNOP_HIP_MOE_LINEAR_ABI_VERSION; }

NNOP_MOE_LINEAR_API int nnop_moe_linear(const nnop_moe_linear_desc* d, void* ys, const void* xs, const void* w, const void* bias,
                                        const int32_t* offsets, nnop_stream_t stream) {
    int st = check_desc(kMoeLinearFwd, d);
    if (st != NNOP_OK) return st;
    st = check_ptrs({{{ys, xs, w}, dtype_bytes(d->dtype)}, {{offsets}, 4}});
    if (st != NNOP_OK) return st;
    if (misaligned(bias, dtype_bytes(d->dtype))) return NNOP_ERR_ALIGN;  // the one optional pointer: NULL is aligned
    return launch_moe_linear(kMoeLinearFwd, *d, ys, xs, w, bias, offsets, (hipStream_t)stream);
}

NNOP_MOE_LINEAR_API int nnop_moe_linear_bwd_x(const nnop_moe_linear_desc* d, void* dxs, const void* dys, const void* w,
                                              const int32_t* offsets, nnop_stream_t stream) {
    int st = check_desc(kMoeLinearBwdX, d);
    if (st != NNOP_OK) return st;
    st = check_ptrs({{{dxs, dys, w}, dtype_bytes(d->dtype)}, {{offsets}, 4}});
    if (st != NNOP_OK) return st;
    return launch_moe_linear(kMoeLinearBwdX, *d, dxs, dys, w, nullptr, offsets, (hipStream_t)stream);
}

NNOP_MOE_LINEAR_API int nnop_moe_linear_bwd_w(const nnop_moe_linear_desc* d, void* dw, const void* dys, const void* xs,
                                              const int32_t* offsets, nnop_stream_t stream) {
    int st = check_desc(kMoeLinearBwdW, d);
    if (st != NNOP_OK) return st;
    st = check_ptrs({{{dw}, dtype_bytes(d->grad_dtype)}, {{dys, xs}, dtype_bytes(d->dtype)}, {{offsets}, 4}});
    if (st != NNOP_OK) return st;
    return launch_moe_linear(kMoeLinearBwdW, *d, dw, dys, xs, nullptr, offsets, (hipStream_t)stream);
}

NNOP_MOE_LINEAR_API int nnop_moe_linear_bwd_b(const nnop_moe_linear_desc* d, void* db, const void* dys, const int32_t* offsets,
                                              nnop_stream_t stream) {
    int st = check_desc(kMoeLinearBwdB, d);
    if (st != NNOP_OK) return st;
    st = check_ptrs({{{db}, dtype_bytes(d->grad_dtype)}, {{dys}, dtype_bytes(d->dtype)}, {{offsets}, 4}});
    if (st != NNOP_OK) return st;
    return launch_moe_linear_bias_bwd(*d, db, dys, offsets, (hipStream_t)stream);
}
