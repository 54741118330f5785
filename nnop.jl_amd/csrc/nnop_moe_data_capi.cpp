// nnop_moe_data_capi.cpp -- the extern "C" boundary of libnnop_hip_moe_data.so, declared in include/nnop_hip_moe_data.h.
//
// Every argument check happens here, in the header's order, before anything touches the device.  The library exports these five
// functions and nothing else (nnop_moe_data.map); it links nothing from the other three libraries.
#include "moe_data.hpp"
#include "host_common.hpp"

#define NNOP_MOE_DATA_API extern "C" __attribute__((visibility("default")))

namespace nnop {

// the descriptor itself, then dtype, options, shape
static int check_rows_desc(const nnop_moe_rows_desc* d) {
    if (!d) return NNOP_ERR_NULL;
    if (!known_dtype(d->dtype)) return NNOP_ERR_DTYPE;
    if (d->reserved[0] != 0 || d->reserved[1] != 0) return NNOP_ERR_OPTS;
    if (d->tokens < 1 || d->topk < 1 || d->topk > kMoeRowsMaxTopk) return NNOP_ERR_SHAPE;
    if (d->dim < 1 || d->dim > kMoeRowsMaxDim || d->ld_tok < d->dim || d->ld_slot < d->dim) return NNOP_ERR_SHAPE;
    if ((long long)d->tokens * d->topk > 0x7fffffffLL) return NNOP_ERR_SHAPE;
    return NNOP_OK;
}

}  // namespace nnop

using namespace nnop;

NNOP_MOE_DATA_API int nnop_moe_data_abi_version(void) { return NNOP_HIP_MOE_DATA_ABI_VERSION; }

NNOP_MOE_DATA_API int nnop_moe_permute(const nnop_moe_rows_desc* d, void* xs, const void* x, const int32_t* perm, nnop_stream_t stream) {
    int st = check_rows_desc(d);
    if (st != NNOP_OK) return st;
    st = check_ptrs({{{xs, x}, dtype_bytes(d->dtype)}, {{perm}, 4}});
    if (st != NNOP_OK) return st;
    return launch_moe_gather(*d, xs, x, perm, (hipStream_t)stream);
}

NNOP_MOE_DATA_API int nnop_moe_permute_bwd(const nnop_moe_rows_desc* d, void* dx, const void* dxs, const int32_t* slot,
                                           nnop_stream_t stream) {
    int st = check_rows_desc(d);
    if (st != NNOP_OK) return st;
    st = check_ptrs({{{dx, dxs}, dtype_bytes(d->dtype)}, {{slot}, 4}});
    if (st != NNOP_OK) return st;
    return launch_moe_reduce(*d, dx, dxs, nullptr, slot, (hipStream_t)stream);
}

NNOP_MOE_DATA_API int nnop_moe_combine(const nnop_moe_rows_desc* d, void* y, const void* ys, const float* w, const int32_t* slot,
                                       nnop_stream_t stream) {
    int st = check_rows_desc(d);
    if (st != NNOP_OK) return st;
    st = check_ptrs({{{y, ys}, dtype_bytes(d->dtype)}, {{w, slot}, 4}});
    if (st != NNOP_OK) return st;
    return launch_moe_reduce(*d, y, ys, w, slot, (hipStream_t)stream);
}

NNOP_MOE_DATA_API int nnop_moe_combine_bwd(const nnop_moe_rows_desc* d, void* dys, float* dw, const void* dy, const void* ys,
                                           const float* w, const int32_t* perm, const int32_t* slot, nnop_stream_t stream) {
    int st = check_rows_desc(d);
    if (st != NNOP_OK) return st;
    st = check_ptrs({{{dys, dy, ys}, dtype_bytes(d->dtype)}, {{dw, w, perm, slot}, 4}});
    if (st != NNOP_OK) return st;
    return launch_moe_combine_bwd(*d, dys, dw, dy, ys, w, perm, slot, (hipStream_t)stream);
}
