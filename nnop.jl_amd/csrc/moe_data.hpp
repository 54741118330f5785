// moe_data.hpp -- what nnop_moe_data_capi.cpp needs of moe_rows.hip (libnnop_hip_moe_data.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "../../include/nnop_hip_moe_data.h"

namespace nnop {

constexpr int kMoeRowsMaxTopk = 64;
constexpr int kMoeRowsMaxDim = 65536;

// xs[s] = x[perm[s] / k], a row of +0 for a skipped slot
int launch_moe_gather(const nnop_moe_rows_desc& d, void* xs, const void* x, const int32_t* perm, hipStream_t s);
// out[t] = sum_j w[t][j] rows[slot[t][j]] over the valid j; w == nullptr: every weight 1 (the pullback of the gather)
int launch_moe_reduce(const nnop_moe_rows_desc& d, void* out, const void* rows, const float* w, const int32_t* slot, hipStream_t s);
int launch_moe_combine_bwd(const nnop_moe_rows_desc& d, void* dys, float* dw, const void* dy, const void* ys, const float* w,
                           const int32_t* perm, const int32_t* slot, hipStream_t s);

}  // namespace nnop
