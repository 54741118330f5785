// decode_attn.hpp -- what the C boundary (nnop_decode_attn_capi.cpp) and the kernels (decode_attn.hip) of libnnop_hip_decode_attn.so share:
// the constants of the work split, the host-side plan and the launcher's prototype.  Nothing of the other nine libraries is linked; the
// few shared lines (the MFMA wrapper of moe_gemm_tile.hpp) are restated in decode_attn.hip in the form this kernel needs.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/nnop_hip_decode_attn.h"

namespace nnop {

constexpr int kDaTile = 32;        // keys of a tile: two 16-key blocks of v_mfma_f32_16x16x32
constexpr int kDaWaves = 4;        // waves of a workgroup; they take the tiles of a chunk round-robin
constexpr int kDaRows = NNOP_DECODE_ATTN_MAX_ROWS;
constexpr int kDaMaxSplits = NNOP_DECODE_ATTN_MAX_SPLITS;
constexpr int kDaTargetGroups = 512;  // about two workgroups for each of the 256 compute units of an MI355X

// the rule of include/nnop_hip_decode_attn.h, from host values alone
static inline int decode_attn_splits(const nnop_decode_attn_desc& d) {
    if (d.splits >= 1) return d.splits;
    long long tiles = ((long long)d.capacity + kDaTile - 1) / kDaTile;
    if (d.window_left >= 0) {
        const long long live = ((long long)d.ql + d.window_left) / kDaTile + 2;
        tiles = tiles < live ? tiles : live;
    }
    const long long groups = (long long)d.batch * d.kh;
    long long s = (kDaTargetGroups + groups - 1) / groups;
    if (s > tiles / kDaWaves) s = tiles / kDaWaves;
    if (s < 1) s = 1;
    return (int)(s > kDaMaxSplits ? kDaMaxSplits : s);
}

// fp32 partial results of every (row, chunk): emb values of O and (m, l)
static inline size_t decode_attn_workspace_bytes(const nnop_decode_attn_desc& d, int splits) {
    if (splits <= 1) return 0;
    return sizeof(float) * (size_t)d.batch * (size_t)d.qh * (size_t)d.ql * (size_t)splits * (size_t)(d.emb + 2);
}

// d has passed every check of the C boundary; `splits` is the resolved count
int launch_decode_attn(const nnop_decode_attn_desc& d, int splits, void* o, float* lse, const void* q, const void* k, const void* v,
                       const int32_t* seqlens, const float* sinks, float* workspace, hipStream_t stream);

}  // namespace nnop
