// paged_attn.hpp -- what the C boundary (nnop_paged_attn_capi.cpp) and the kernels (paged_attn.hip) of libnnop_hip_paged_attn.so share.
// The work split (tile, waves, rows), the split rule and the workspace formula are the tenth library's, taken from decode_attn.hpp as
// header-only code with capacity = max_pages page_size: nothing is linked from libnnop_hip_decode_attn.so.
#pragma once
#include "decode_attn.hpp"
#include "../../include/nnop_hip_paged_attn.h"

namespace nnop {

// the descriptor as the tenth library's rule reads it; max_pages page_size has been checked to fit (the rule reads no stride)
static inline nnop_decode_attn_desc paged_attn_as_dense(const nnop_paged_attn_desc& d) {
    nnop_decode_attn_desc r = {};
    r.dtype = d.dtype, r.emb = d.emb, r.ql = d.ql, r.qh = d.qh, r.kh = d.kh, r.batch = d.batch;
    r.capacity = (int32_t)((int64_t)d.max_pages * d.page_size);
    r.window_left = d.window_left, r.splits = d.splits;
    return r;
}
static_assert(sizeof(nnop_paged_attn_desc) == 104, "the tenth library's 96 bytes and table_stride");

// d has passed every check of the C boundary; `splits` is the resolved count
int launch_paged_attn(const nnop_paged_attn_desc& d, int splits, void* o, float* lse, const void* q, const void* k, const void* v,
                      const int32_t* block_table, const int32_t* seqlens, const float* sinks, float* workspace, hipStream_t stream);

}  // namespace nnop
