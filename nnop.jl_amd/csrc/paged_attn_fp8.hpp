// paged_attn_fp8.hpp -- what the C boundary (nnop_paged_attn_fp8_capi.cpp) and the kernels (paged_attn_fp8.hip) of
// libnnop_hip_paged_attn_fp8.so share.  The work split (tile, waves, rows), the split rule and the workspace formula are the tenth
// library's, taken from decode_attn.hpp as header-only code with capacity = max_pages page_size; the depth of the ring is the eleventh
// library's kDfRing, restated here so that nothing but decode_attn.hpp is read from another library.  Nothing is linked from one.
#pragma once
#include "decode_attn.hpp"
#include "../../include/nnop_hip_paged_attn_fp8.h"

namespace nnop {

constexpr int kPfRing = 4;  // tiles of K and V loads in flight per wave: decode_attn_fp8.hpp's kDfRing

// the descriptor as the tenth library's rule reads it; max_pages page_size has been checked to fit (the rule reads no stride)
static inline nnop_decode_attn_desc paged_attn_fp8_as_dense(const nnop_paged_attn_fp8_desc& d) {
    nnop_decode_attn_desc r = {};
    r.dtype = d.dtype, r.emb = d.emb, r.ql = d.ql, r.qh = d.qh, r.kh = d.kh, r.batch = d.batch;
    r.capacity = (int32_t)((int64_t)d.max_pages * d.page_size);
    r.window_left = d.window_left, r.splits = d.splits;
    return r;
}
static_assert(sizeof(nnop_paged_attn_fp8_desc) == 112, "the twelfth library's 104 bytes, kv_format and reserved");

// d has passed every check of the C boundary; `splits` is the resolved count
int launch_paged_attn_fp8(const nnop_paged_attn_fp8_desc& d, int splits, void* o, float* lse, const void* q, const void* k, const void* v,
                          const float* k_scale, const float* v_scale, const int32_t* block_table, const int32_t* seqlens,
                          const float* sinks, float* workspace, hipStream_t stream);

}  // namespace nnop
