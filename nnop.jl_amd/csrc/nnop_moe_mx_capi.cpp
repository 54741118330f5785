// nnop_moe_mx_capi.cpp -- the extern "C" boundary of libnnop_hip_moe_mx.so, declared in include/nnop_hip_moe_mx.h.
//
// Every argument check happens here, in the header's order, before anything touches the device.  The library exports these five
// functions and nothing else (nnop_moe_mx.map); it links nothing from the other six libraries.
#include "moe_mx.hpp"
#include "host_common.hpp"

#define NNOP_MOE_MX_API extern "C" __attribute__((visibility("default")))

namespace nnop {

// the descriptor itself, then dtype, options, shape: the same for the two products.  The pointers are each call's own.
static int check_desc(bool bwd_x, const nnop_moe_mx_desc* d) {
    if (!d) return NNOP_ERR_NULL;
    if (d->dtype != NNOP_F16 && d->dtype != NNOP_BF16) return NNOP_ERR_DTYPE;
    if (d->flags != 0) return NNOP_ERR_OPTS;
    for (int32_t r : d->reserved)
        if (r != 0) return NNOP_ERR_OPTS;
    if (d->rows < 1 || d->experts < 1 || d->experts > kMoeMxMaxExperts) return NNOP_ERR_SHAPE;
    if (d->in_dim < 1 || d->in_dim > kMoeMxMaxDim || d->out_dim < 1 || d->out_dim > kMoeMxMaxDim) return NNOP_ERR_SHAPE;
    if (d->in_dim % kMxBlock != 0) return NNOP_ERR_SHAPE;
    if (d->ld_x < d->in_dim || d->ld_y < d->out_dim || d->ld_b < d->out_dim) return NNOP_ERR_SHAPE;
    if (d->ld_q < d->in_dim / 2 || d->ld_q % 16 != 0 || d->ld_s < d->in_dim / kMxBlock) return NNOP_ERR_SHAPE;
    if (moe_mx_workgroups(bwd_x, *d) > 0x7fffffffLL) return NNOP_ERR_SHAPE;
    return NNOP_OK;
}

static int check_rows_desc(const nnop_mxfp4_desc* d) {
    if (!d) return NNOP_ERR_NULL;
    if (!known_dtype(d->dtype)) return NNOP_ERR_DTYPE;
    if (d->reserved != 0) return NNOP_ERR_OPTS;
    if (d->rows < 1 || d->cols < kMxBlock || d->cols > kMxfp4MaxCols || d->cols % kMxBlock != 0) return NNOP_ERR_SHAPE;
    if (d->ld < d->cols || d->ld_q < d->cols / 2 || d->ld_q % 16 != 0 || d->ld_s < d->cols / kMxBlock) return NNOP_ERR_SHAPE;
    if (d->rows > kMxfp4MaxPieces / (d->cols / 8)) return NNOP_ERR_SHAPE;
    return NNOP_OK;
}

}  // namespace nnop

using namespace nnop;

NNOP_MOE_MX_API int nnop_moe_mx_abi_version(void) { return NNOP_HIP_MOE_MX_ABI_VERSION; }

NNOP_MOE_MX_API int nnop_moe_mx_linear(const nnop_moe_mx_desc* d, void* ys, const void* xs, const uint8_t* blocks, const uint8_t* scales,
                                       const void* bias, const int32_t* offsets, nnop_stream_t stream) {
    int st = check_desc(false, d);
    if (st != NNOP_OK) return st;
    st = check_ptrs({{{ys, xs}, dtype_bytes(d->dtype)}, {{blocks}, 16}, {{scales}, 1}, {{offsets}, 4}});
    if (st != NNOP_OK) return st;
    if (misaligned(bias, dtype_bytes(d->dtype))) return NNOP_ERR_ALIGN;  // the one optional pointer: NULL is aligned
    return launch_moe_mx_linear(false, *d, ys, xs, blocks, scales, bias, offsets, (hipStream_t)stream);
}

NNOP_MOE_MX_API int nnop_moe_mx_linear_bwd_x(const nnop_moe_mx_desc* d, void* dxs, const void* dys, const uint8_t* blocks,
                                             const uint8_t* scales, const int32_t* offsets, nnop_stream_t stream) {
    int st = check_desc(true, d);
    if (st != NNOP_OK) return st;
    st = check_ptrs({{{dxs, dys}, dtype_bytes(d->dtype)}, {{blocks}, 16}, {{scales}, 1}, {{offsets}, 4}});
    if (st != NNOP_OK) return st;
    return launch_moe_mx_linear(true, *d, dxs, dys, blocks, scales, nullptr, offsets, (hipStream_t)stream);
}

NNOP_MOE_MX_API int nnop_mxfp4_dequant(const nnop_mxfp4_desc* d, void* out, const uint8_t* blocks, const uint8_t* scales,
                                       nnop_stream_t stream) {
    int st = check_rows_desc(d);
    if (st != NNOP_OK) return st;
    st = check_ptrs({{{out}, dtype_bytes(d->dtype)}, {{blocks}, 16}, {{scales}, 1}});
    if (st != NNOP_OK) return st;
    return launch_mxfp4_dequant(*d, out, blocks, scales, (hipStream_t)stream);
}

NNOP_MOE_MX_API int nnop_mxfp4_quant(const nnop_mxfp4_desc* d, uint8_t* blocks, uint8_t* scales, const void* in, nnop_stream_t stream) {
    int st = check_rows_desc(d);
    if (st != NNOP_OK) return st;
    st = check_ptrs({{{in}, dtype_bytes(d->dtype)}, {{blocks}, 16}, {{scales}, 1}});
    if (st != NNOP_OK) return st;
    return launch_mxfp4_quant(*d, blocks, scales, in, (hipStream_t)stream);
}
