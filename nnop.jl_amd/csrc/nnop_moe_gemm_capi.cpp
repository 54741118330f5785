// nnop_moe_gemm_capi.cpp -- the extern "C" boundary of libnnop_hip_moe_gemm.so, declared in include/nnop_hip_moe_gemm.h.
//
// Every argument check happens here, in the header's order, before anything touches the device.  The library exports these four
// functions and nothing else (nnop_moe_gemm.map); it links nothing from the other libraries.
#include "moe_gemm.hpp"
#include "host_common.hpp"

#define NNOP_MOE_GEMM_API extern "C" __attribute__((visibility("default")))

namespace nnop {

// the descriptor itself, then dtype, options, shape; then the pointers (out, a, b are arrays of `dtype`)
static int check_gemm(MoeGemmProduct which, const nnop_moe_gemm_desc* d, const void* out, const void* a, const void* b,
                      const int32_t* offsets) {
    if (!d) return NNOP_ERR_NULL;
    if (!known_dtype(d->dtype)) return NNOP_ERR_DTYPE;
    if (d->reserved[0] != 0 || d->reserved[1] != 0) return NNOP_ERR_OPTS;
    if (d->rows < 1 || d->experts < 1 || d->experts > kMoeGemmMaxExperts) return NNOP_ERR_SHAPE;
    if (d->in_dim < 1 || d->in_dim > kMoeGemmMaxDim || d->out_dim < 1 || d->out_dim > kMoeGemmMaxDim) return NNOP_ERR_SHAPE;
    if (d->ld_x < d->in_dim || d->ld_y < d->out_dim || d->ld_w < d->in_dim) return NNOP_ERR_SHAPE;
    if (moe_gemm_workgroups(which, *d) > 0x7fffffffLL) return NNOP_ERR_SHAPE;
    return check_ptrs({{{out, a, b}, dtype_bytes(d->dtype)}, {{offsets}, 4}});
}

}  // namespace nnop

using namespace nnop;

NNOP_MOE_GEMM_API int nnop_moe_gemm_abi_version(void) { return NNOP_HIP_MOE_GEMM_ABI_VERSION; }

NNOP_MOE_GEMM_API int nnop_moe_gemm(const nnop_moe_gemm_desc* d, void* ys, const void* xs, const void* w, const int32_t* offsets,
                                    nnop_stream_t stream) {
    const int st = check_gemm(kMoeGemmFwd, d, ys, xs, w, offsets);
    if (st != NNOP_OK) return st;
    return launch_moe_gemm(kMoeGemmFwd, *d, ys, xs, w, offsets, (hipStream_t)stream);
}

NNOP_MOE_GEMM_API int nnop_moe_gemm_bwd_x(const nnop_moe_gemm_desc* d, void* dxs, const void* dys, const void* w, const int32_t* offsets,
                                          nnop_stream_t stream) {
    const int st = check_gemm(kMoeGemmBwdX, d, dxs, dys, w, offsets);
    if (st != NNOP_OK) return st;
    return launch_moe_gemm(kMoeGemmBwdX, *d, dxs, dys, w, offsets, (hipStream_t)stream);
}

NNOP_MOE_GEMM_API int nnop_moe_gemm_bwd_w(const nnop_moe_gemm_desc* d, void* dw, const void* dys, const void* xs, const int32_t* offsets,
                                          nnop_stream_t stream) {
    const int st = check_gemm(kMoeGemmBwdW, d, dw, dys, xs, offsets);
    if (st != NNOP_OK) return st;
    return launch_moe_gemm(kMoeGemmBwdW, *d, dw, dys, xs, offsets, (hipStream_t)stream);
}
