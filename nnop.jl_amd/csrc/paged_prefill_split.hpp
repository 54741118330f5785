// paged_prefill_split.hpp -- what the C boundary (nnop_paged_prefill_split_capi.cpp) and the kernels (paged_prefill_split.hip) of
// libnnop_hip_paged_prefill_split.so share: the split rule, the workspace formula and the launcher's prototype.  The row block, the key
// tile and the bound of the blocks are paged_prefill.hpp's (header-only, nothing is linked).
#pragma once
#include "paged_prefill.hpp"
#include "../../include/nnop_hip_paged_prefill_split.h"

namespace nnop {

constexpr int kPpsMaxSplits = NNOP_PAGED_PREFILL_SPLIT_MAX_SPLITS;
constexpr int kPpsTargetGroups = 512;  // two resident workgroups for each of the 256 compute units: waves_per_eu(2, 2) with four waves
constexpr int kPpsMinChunkTiles = NNOP_PAGED_PREFILL_SPLIT_MIN_CHUNK_TILES;  // what 4, 8 and 16 measured
constexpr int kPpsMergeRows = 4;       // rows of a merge workgroup, a wave each

// the rule of include/nnop_hip_paged_prefill_split.h, from host values alone; d.reserved is the caller's count, 0 for this rule
static inline int paged_prefill_splits(const nnop_paged_prefill_desc& d) {
    if (d.reserved >= 1) return d.reserved;
    const long long groups = d.kh * paged_prefill_max_blocks(d);
    long long tiles = ((long long)d.max_pages * d.page_size + kPpTile - 1) / kPpTile;
    if (d.window_left >= 0) {
        const long long live = ((long long)paged_prefill_block_tokens(d) + d.window_left) / kPpTile + 2;
        tiles = tiles < live ? tiles : live;
    }
    long long s = (kPpsTargetGroups + groups - 1) / groups;
    if (s > tiles / kPpsMinChunkTiles) s = tiles / kPpsMinChunkTiles;
    if (s < 1) s = 1;
    return (int)(s > kPpsMaxSplits ? kPpsMaxSplits : s);
}

// fp32 partial results of every (chunk, token, head): emb values of O, then (m, l) behind all of them
static inline size_t paged_prefill_split_workspace_bytes(const nnop_paged_prefill_desc& d, int splits) {
    if (splits <= 1) return 0;
    return sizeof(float) * (size_t)d.tokens * (size_t)d.qh * (size_t)splits * (size_t)(d.emb + 2);
}

// d has passed every check of the C boundary; `splits` is the resolved count, and `workspace` holds the bytes above when it exceeds 1
int launch_paged_prefill_split(const nnop_paged_prefill_desc& d, int splits, void* o, float* lse, const void* q, const void* k,
                               const void* v, const int32_t* block_table, const int32_t* cu_seqlens_q, const int32_t* seqlens,
                               const float* sinks, float* workspace, hipStream_t stream);

}  // namespace nnop
