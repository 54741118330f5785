// nnop_moe_mx_decode_glu_capi.cpp -- the extern "C" boundary of libnnop_hip_moe_mx_decode_glu.so, declared in
// include/nnop_hip_moe_mx_decode_glu.h.
//
// Every argument check happens here, in the header's order, before anything touches the device: the checks of nnop_moe_mx_decode_linear
// (nnop_moe_mx_decode_capi.cpp) with N = 2 I, the option checks of nnop_glu (nnop_capi.cpp) and the geometry of nnop_moe_permute where a
// perm is given.  The library exports these two functions and nothing else (nnop_moe_mx_decode_glu.map); it links nothing from the other
// eight libraries.
#include "moe_mx_decode_glu.hpp"
#include "host_common.hpp"

#define NNOP_MOE_MX_DECODE_GLU_API extern "C" __attribute__((visibility("default")))

namespace nnop {

constexpr int kBlock = 32;  // elements that share a scale byte

static int check_desc(const nnop_moe_mx_decode_glu_desc* d, const void* perm) {
    if (!d) return NNOP_ERR_NULL;
    if (d->dtype != NNOP_F16 && d->dtype != NNOP_BF16) return NNOP_ERR_DTYPE;
    if (d->flags != 0) return NNOP_ERR_OPTS;
    for (int32_t r : d->reserved)
        if (r != 0) return NNOP_ERR_OPTS;
    if (d->act < NNOP_GLU_SILU || d->act > NNOP_GLU_SWIGLU_OAI) return NNOP_ERR_OPTS;
    if (d->layout != NNOP_MOE_GLU_INTERLEAVED && d->layout != NNOP_MOE_GLU_HALVES) return NNOP_ERR_OPTS;
    if (d->act == NNOP_GLU_SWIGLU_OAI && !(finite(d->alpha) && finite(d->limit) && d->limit > 0.f)) return NNOP_ERR_OPTS;
    if (d->rows < 1 || d->experts < 1 || d->experts > kMoeMxDecodeGluMaxExperts) return NNOP_ERR_SHAPE;
    if (d->in_dim < 1 || d->in_dim > kMoeMxDecodeGluMaxIn || d->inter_dim < 1 || d->inter_dim > kMoeMxDecodeGluMaxInter) return NNOP_ERR_SHAPE;
    if (d->in_dim % kBlock != 0) return NNOP_ERR_SHAPE;
    if (d->ld_x < d->in_dim || d->ld_h < d->inter_dim || d->ld_b < 2 * d->inter_dim) return NNOP_ERR_SHAPE;
    if (d->ld_q < d->in_dim / 2 || d->ld_q % 16 != 0 || d->ld_s < d->in_dim / kBlock) return NNOP_ERR_SHAPE;
    if (d->tokens < 0 || d->topk < 0) return NNOP_ERR_SHAPE;
    if (d->tokens != 0 || d->topk != 0) {
        if (d->tokens < 1 || d->topk < 1 || d->topk > kMoeMxDecodeGluMaxTopk) return NNOP_ERR_SHAPE;
        if ((long long)d->tokens * d->topk > 0x7fffffffLL) return NNOP_ERR_SHAPE;
    }
    if ((perm != nullptr) != (d->tokens != 0)) return NNOP_ERR_SHAPE;
    if (moe_mx_decode_glu_workgroups(*d) > 0x7fffffffLL) return NNOP_ERR_SHAPE;
    return NNOP_OK;
}

}  // namespace nnop

using namespace nnop;

NNOP_MOE_MX_DECODE_GLU_API int nnop_moe_mx_decode_glu_abi_version(void) { return NNOP_HIP_MOE_MX_DECODE_GLU_ABI_VERSION; }

NNOP_MOE_MX_DECODE_GLU_API int nnop_moe_mx_decode_glu(const nnop_moe_mx_decode_glu_desc* d, void* h, const void* x, const uint8_t* blocks,
                                                      const uint8_t* scales, const void* bias, const int32_t* offsets, const int32_t* perm,
                                                      nnop_stream_t stream) {
    int st = check_desc(d, perm);
    if (st != NNOP_OK) return st;
    st = check_ptrs({{{h, x}, dtype_bytes(d->dtype)}, {{blocks}, 16}, {{scales}, 1}, {{offsets}, 4}});
    if (st != NNOP_OK) return st;
    // the optional pointers: NULL is aligned
    if (misaligned(bias, dtype_bytes(d->dtype)) || misaligned(perm, 4)) return NNOP_ERR_ALIGN;
    return launch_moe_mx_decode_glu(*d, h, x, blocks, scales, bias, offsets, perm, (hipStream_t)stream);
}
