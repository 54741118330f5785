// moe_gemm.hpp -- what nnop_moe_gemm_capi.cpp needs of moe_gemm.hip (libnnop_hip_moe_gemm.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "../../include/nnop_hip_moe_gemm.h"

namespace nnop {

constexpr int kMoeGemmMaxExperts = 1024;
constexpr int kMoeGemmMaxDim = 65536;

// the three products of the header; the caller has checked moe_gemm_workgroups() <= 2^31 - 1
enum MoeGemmProduct { kMoeGemmFwd = 0, kMoeGemmBwdX = 1, kMoeGemmBwdW = 2 };
int launch_moe_gemm(MoeGemmProduct which, const nnop_moe_gemm_desc& d, void* out, const void* a, const void* b, const int32_t* offsets,
                    hipStream_t s);
// the number of workgroups launch_moe_gemm would start, computed in 64 bits
long long moe_gemm_workgroups(MoeGemmProduct which, const nnop_moe_gemm_desc& d);

}  // namespace nnop
