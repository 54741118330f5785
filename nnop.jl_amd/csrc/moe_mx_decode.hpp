// moe_mx_decode.hpp -- what nnop_moe_mx_decode_capi.cpp needs of moe_mx_decode.hip (libnnop_hip_moe_mx_decode.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/nnop_hip_moe_mx_decode.h"

namespace nnop {

constexpr int kMoeMxDecodeMaxExperts = 1024;
constexpr int kMoeMxDecodeMaxDim = 65536;
constexpr int kMoeMxDecodeCols = 256;   // output columns (weight rows) of one workgroup: 4 waves of 4 MFMA row tiles of 16

// the forward; the caller has checked moe_mx_decode_workgroups() <= 2^31 - 1.  bias may be NULL
int launch_moe_mx_decode_linear(const nnop_moe_mx_decode_desc& d, void* ys, const void* xs, const uint8_t* blocks, const uint8_t* scales,
                                const void* bias, const int32_t* offsets, hipStream_t s);
// the number of workgroups the forward starts (E column groups per expert), computed in 64 bits
long long moe_mx_decode_workgroups(const nnop_moe_mx_decode_desc& d);

}  // namespace nnop
