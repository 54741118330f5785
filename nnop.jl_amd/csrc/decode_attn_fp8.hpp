// decode_attn_fp8.hpp -- what the C boundary (nnop_decode_attn_fp8_capi.cpp) and the kernels (decode_attn_fp8.hip) of
// libnnop_hip_decode_attn_fp8.so share.  The work split (tile, waves, rows), the split rule and the workspace formula are the tenth
// library's, taken from decode_attn.hpp as header-only code: nothing is linked from libnnop_hip_decode_attn.so.
#pragma once
#include "decode_attn.hpp"
#include "../../include/nnop_hip_decode_attn_fp8.h"

namespace nnop {

constexpr int kDfRing = 4;  // tiles of K and V loads in flight per wave: the bytes of the 16-bit kernel's two

// the descriptor as the tenth library's rule reads it: the two layouts are the same 96 bytes, kv_format in the place of reserved[0]
static inline nnop_decode_attn_desc decode_attn_fp8_as_16bit(const nnop_decode_attn_fp8_desc& d) {
    nnop_decode_attn_desc r = {};
    r.dtype = d.dtype, r.emb = d.emb, r.ql = d.ql, r.qh = d.qh, r.kh = d.kh, r.batch = d.batch, r.capacity = d.capacity;
    r.window_left = d.window_left, r.splits = d.splits;
    return r;
}
static_assert(sizeof(nnop_decode_attn_fp8_desc) == sizeof(nnop_decode_attn_desc) && sizeof(nnop_decode_attn_desc) == 96, "one layout");

// d has passed every check of the C boundary; `splits` is the resolved count
int launch_decode_attn_fp8(const nnop_decode_attn_fp8_desc& d, int splits, void* o, float* lse, const void* q, const void* k, const void* v,
                           const float* k_scale, const float* v_scale, const int32_t* seqlens, const float* sinks, float* workspace,
                           hipStream_t stream);

}  // namespace nnop
