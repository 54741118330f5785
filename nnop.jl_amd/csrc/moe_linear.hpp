// moe_linear.hpp -- what nnop_moe_linear_capi.cpp needs of moe_linear.hip (libnnop_hip_moe_linear.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "../../include/nnop_hip_moe_linear.h"

namespace nnop {

constexpr int kMoeLinearMaxExperts = 1024;
constexpr int kMoeLinearMaxDim = 65536;

// the four calls of the header; the caller has checked moe_linear_workgroups() <= 2^31 - 1
enum MoeLinearCall { kMoeLinearFwd = 0, kMoeLinearBwdX = 1, kMoeLinearBwdW = 2, kMoeLinearBwdB = 3 };
// the three products: out / a / b are (ys, xs, w), (dxs, dys, w), (dw, dys, xs); bias may be NULL and is read by the forward only
int launch_moe_linear(MoeLinearCall which, const nnop_moe_linear_desc& d, void* out, const void* a, const void* b, const void* bias,
                      const int32_t* offsets, hipStream_t s);
int launch_moe_linear_bias_bwd(const nnop_moe_linear_desc& d, void* db, const void* dys, const int32_t* offsets, hipStream_t s);
// the number of workgroups a call would start, computed in 64 bits
long long moe_linear_workgroups(MoeLinearCall which, const nnop_moe_linear_desc& d);

}  // namespace nnop
