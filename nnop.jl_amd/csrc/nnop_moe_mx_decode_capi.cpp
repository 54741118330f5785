// nnop_moe_mx_decode_capi.cpp -- the extern "C" boundary of libnnop_hip_moe_mx_decode.so, declared in include/nnop_hip_moe_mx_decode.h.
//
// Every argument check happens here, in the header's order, before anything touches the device: the checks of nnop_moe_mx_linear
// (nnop_moe_mx_capi.cpp) with this kernel's grid in the place of the tile count.  The library exports these two functions and nothing
// else (nnop_moe_mx_decode.map); it links nothing from the other seven libraries.
#include "moe_mx_decode.hpp"
#include "host_common.hpp"

#define NNOP_MOE_MX_DECODE_API extern "C" __attribute__((visibility("default")))

namespace nnop {

constexpr int kBlock = 32;  // elements that share a scale byte

static int check_desc(const nnop_moe_mx_decode_desc* d) {
    if (!d) return NNOP_ERR_NULL;
    if (d->dtype != NNOP_F16 && d->dtype != NNOP_BF16) return NNOP_ERR_DTYPE;
    if (d->flags != 0) return NNOP_ERR_OPTS;
    for (int32_t r : d->reserved)
        if (r != 0) return NNOP_ERR_OPTS;
    if (d->rows < 1 || d->experts < 1 || d->experts > kMoeMxDecodeMaxExperts) return NNOP_ERR_SHAPE;
    if (d->in_dim < 1 || d->in_dim > kMoeMxDecodeMaxDim || d->out_dim < 1 || d->out_dim > kMoeMxDecodeMaxDim) return NNOP_ERR_SHAPE;
    if (d->in_dim % kBlock != 0) return NNOP_ERR_SHAPE;
    if (d->ld_x < d->in_dim || d->ld_y < d->out_dim || d->ld_b < d->out_dim) return NNOP_ERR_SHAPE;
    if (d->ld_q < d->in_dim / 2 || d->ld_q % 16 != 0 || d->ld_s < d->in_dim / kBlock) return NNOP_ERR_SHAPE;
    if (moe_mx_decode_workgroups(*d) > 0x7fffffffLL) return NNOP_ERR_SHAPE;
    return NNOP_OK;
}

}  // namespace nnop

using namespace nnop;

NNOP_MOE_MX_DECODE_API int nnop_moe_mx_decode_abi_version(void) { return NNOP_HIP_MOE_MX_DECODE_ABI_VERSION; }

NNOP_MOE_MX_DECODE_API int nnop_moe_mx_decode_linear(const nnop_moe_mx_decode_desc* d, void* ys, const void* xs, const uint8_t* blocks,
                                                     const uint8_t* scales, const void* bias, const int32_t* offsets,
                                                     nnop_stream_t stream) {
    int st = check_desc(d);
    if (st != NNOP_OK) return st;
    st = check_ptrs({{{ys, xs}, dtype_bytes(d->dtype)}, {{blocks}, 16}, {{scales}, 1}, {{offsets}, 4}});
    if (st != NNOP_OK) return st;
    if (misaligned(bias, dtype_bytes(d->dtype))) return NNOP_ERR_ALIGN;  // the one optional pointer: NULL is aligned
    return launch_moe_mx_decode_linear(*d, ys, xs, blocks, scales, bias, offsets, (hipStream_t)stream);
}
