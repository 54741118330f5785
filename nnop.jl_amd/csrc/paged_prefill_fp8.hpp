// paged_prefill_fp8.hpp -- what the C boundary (nnop_paged_prefill_fp8_capi.cpp) and the kernels (paged_prefill_fp8.hip) of
// libnnop_hip_paged_prefill_fp8.so share.  The row block, the key tile and the two figures the host derives from them (the tokens of a
// block, the bound of the grid) are the thirteenth library's, taken from paged_prefill.hpp as header-only code.  Nothing is linked.
#pragma once
#include "paged_prefill.hpp"
#include "../../include/nnop_hip_paged_prefill_fp8.h"

namespace nnop {

static_assert(NNOP_PAGED_PREFILL_FP8_BLOCK_ROWS == kPpRows, "the thirteenth library's row block");
static_assert(sizeof(nnop_paged_prefill_fp8_desc) == 144, "the thirteenth library's 136 bytes, kv_format and reserved2");

// d has passed every check of the C boundary
int launch_paged_prefill_fp8(const nnop_paged_prefill_fp8_desc& d, void* o, float* lse, const void* q, const void* k, const void* v,
                             const float* k_scale, const float* v_scale, const int32_t* block_table, const int32_t* cu_seqlens_q,
                             const int32_t* seqlens, const float* sinks, hipStream_t stream);

}  // namespace nnop
