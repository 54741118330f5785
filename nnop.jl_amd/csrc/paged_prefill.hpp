// paged_prefill.hpp -- what the C boundary (nnop_paged_prefill_capi.cpp) and the kernels (paged_prefill.hip) of
// libnnop_hip_paged_prefill.so share: the row block, the key tile and the two figures the host derives from them.  The fifteenth library
// (paged_prefill_fp8.hpp) reads the constants and the two figures too, on its own descriptor D: header-only, nothing is linked.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/nnop_hip_paged_prefill.h"

namespace nnop {

constexpr int kPpRows = NNOP_PAGED_PREFILL_BLOCK_ROWS;  // rows of a workgroup
constexpr int kPpWaves = 4;                             // 32 rows each: one 32-wide MFMA operand
constexpr int kPpTile = 32;                             // keys of a tile: one 32 x 32 block of scores per wave
static_assert(kPpRows == 32 * kPpWaves, "a wave owns 32 rows");
static_assert(sizeof(nnop_paged_prefill_desc) == 136, "the twelfth library's 104 bytes and the strides of q and o");

// tokens of a row block: its rows are these tokens times the G query heads of a KV head; 128 - TB G < G rows are dead
template <typename D> static inline int paged_prefill_block_tokens(const D& d) { return kPpRows / (d.qh / d.kh); }
// the bound of sum_b ceil(n_b / TB) that the grid is sized by: host values alone
template <typename D> static inline long long paged_prefill_max_blocks(const D& d) {
    return (long long)d.tokens / paged_prefill_block_tokens(d) + d.batch;
}

// d has passed every check of the C boundary
int launch_paged_prefill(const nnop_paged_prefill_desc& d, void* o, float* lse, const void* q, const void* k, const void* v,
                         const int32_t* block_table, const int32_t* cu_seqlens_q, const int32_t* seqlens, const float* sinks,
                         hipStream_t stream);

}  // namespace nnop
