// mla_decode.hpp -- what the C boundary (nnop_mla_decode_capi.cpp) and the kernels (mla_decode.hip) of libnnop_hip_mla_decode.so share: the
// constants of the work split, the host-side plan and the launcher's prototype.  Nothing of the other seventeen libraries is linked or
// included; the few shared lines (the MFMA wrapper, the merge) are restated in mla_decode.hip in the form this kernel needs.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/nnop_hip_mla_decode.h"

namespace nnop {

constexpr int kMlaW = NNOP_MLA_DECODE_WIDTH;    // a row of q and of the cache
constexpr int kMlaV = NNOP_MLA_DECODE_LATENT;   // the columns that are the value; a row of o
constexpr int kMlaTile = 32;                    // keys of a tile: two 16-key blocks of v_mfma_f32_16x16x32
constexpr int kMlaWaves = 4;                    // waves of a workgroup: 16 heads each
constexpr int kMlaBlockHeads = 16 * kMlaWaves;  // heads of a head block
constexpr int kMlaMinTiles = 4;                 // tiles of a chunk the automatic rule keeps
constexpr int kMlaMaxSplits = NNOP_MLA_DECODE_MAX_SPLITS;
constexpr int kMlaTargetGroups = 512;           // about two workgroups for each of the 256 compute units of an MI355X

static inline int mla_decode_head_blocks(const nnop_mla_decode_desc& d) { return (d.qh + kMlaBlockHeads - 1) / kMlaBlockHeads; }

// the rule of include/nnop_hip_mla_decode.h, from host values alone
static inline int mla_decode_splits(const nnop_mla_decode_desc& d) {
    if (d.splits >= 1) return d.splits;
    const long long tiles = ((long long)d.max_pages * d.page_size + kMlaTile - 1) / kMlaTile;
    const long long groups = (long long)d.batch * d.ql * mla_decode_head_blocks(d);
    long long s = (kMlaTargetGroups + groups - 1) / groups;
    if (s > tiles / kMlaMinTiles) s = tiles / kMlaMinTiles;
    if (s < 1) s = 1;
    return (int)(s > kMlaMaxSplits ? kMlaMaxSplits : s);
}

// fp32 partial results of every (row, chunk): 512 values of O and (m, l)
static inline size_t mla_decode_workspace_bytes(const nnop_mla_decode_desc& d, int splits) {
    if (splits <= 1) return 0;
    return sizeof(float) * (size_t)d.batch * (size_t)d.qh * (size_t)d.ql * (size_t)splits * (size_t)(kMlaV + 2);
}

// d has passed every check of the C boundary; `splits` is the resolved count
int launch_mla_decode(const nnop_mla_decode_desc& d, int splits, void* o, float* lse, const void* q, const void* kv,
                      const int32_t* block_table, const int32_t* seqlens, float* workspace, hipStream_t stream);

}  // namespace nnop
