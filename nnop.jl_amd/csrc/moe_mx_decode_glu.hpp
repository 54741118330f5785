// moe_mx_decode_glu.hpp -- what nnop_moe_mx_decode_glu_capi.cpp needs of moe_mx_decode_glu.hip (libnnop_hip_moe_mx_decode_glu.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/nnop_hip_moe_mx_decode_glu.h"

namespace nnop {

constexpr int kMoeMxDecodeGluMaxExperts = 1024;
constexpr int kMoeMxDecodeGluMaxIn = 65536;
constexpr int kMoeMxDecodeGluMaxInter = 32768;  // N = 2 I <= 65536, the eighth library's bound on the weight rows of an expert
constexpr int kMoeMxDecodeGluMaxTopk = 64;
constexpr int kMoeMxDecodeGluCols = 128;        // columns of h of one workgroup: 256 weight rows, 4 waves of 4 MFMA row tiles of 16

// the forward; the caller has checked the descriptor and moe_mx_decode_glu_workgroups() <= 2^31 - 1.  bias and perm may be NULL
int launch_moe_mx_decode_glu(const nnop_moe_mx_decode_glu_desc& d, void* h, const void* x, const uint8_t* blocks, const uint8_t* scales,
                             const void* bias, const int32_t* offsets, const int32_t* perm, hipStream_t s);
// the number of workgroups the forward starts (E column groups per expert), computed in 64 bits
long long moe_mx_decode_glu_workgroups(const nnop_moe_mx_decode_glu_desc& d);

}  // namespace nnop
