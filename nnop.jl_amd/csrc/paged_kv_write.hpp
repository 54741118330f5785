// paged_kv_write.hpp -- what the C boundary (nnop_paged_kv_write_capi.cpp) and the kernel (paged_kv_write.hip) of
// libnnop_hip_paged_kv_write.so share: the split of the work and the launcher's signature.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/nnop_hip_paged_kv_write.h"

namespace nnop {

constexpr int kKvwBlockTokens = NNOP_PAGED_KV_WRITE_BLOCK_TOKENS;  // consecutive tokens of a workgroup
constexpr int kKvwWaves = 4;                                       // a wave takes tokens wave, wave + 4, ... of the block
constexpr int kKvwThreads = 64 * kKvwWaves;
constexpr int kKvwRound = 1024;  // elements of a K row, and of a V row, that a wave holds in registers at once: KH 8 at E 128
static_assert(kKvwBlockTokens % kKvwWaves == 0, "every wave gets the same number of tokens");
static_assert(sizeof(nnop_paged_kv_write_desc) == 136, "twelve int32 and eleven int64");

// the grid: host values alone
static inline long long paged_kv_write_groups(const nnop_paged_kv_write_desc& d) {
    return ((long long)d.tokens + kKvwBlockTokens - 1) / kKvwBlockTokens;
}

// d has passed every check of the C boundary
int launch_paged_kv_write(const nnop_paged_kv_write_desc& d, void* k_pages, void* v_pages, const void* k, const void* v,
                          const float* k_scale, const float* v_scale, const int32_t* block_table, const int32_t* cu_seqlens_q,
                          const int32_t* seqlens, hipStream_t stream);

}  // namespace nnop
