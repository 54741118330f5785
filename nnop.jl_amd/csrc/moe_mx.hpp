// moe_mx.hpp -- what nnop_moe_mx_capi.cpp needs of moe_mx.hip (libnnop_hip_moe_mx.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "../../include/nnop_hip_moe_mx.h"

namespace nnop {

constexpr int kMoeMxMaxExperts = 1024;
constexpr int kMoeMxMaxDim = 65536;
constexpr int kMxBlock = 32;                       // elements that share a scale byte
constexpr int kMxfp4MaxCols = 1 << 30;
constexpr long long kMxfp4MaxPieces = 1LL << 39;   // rows K / 8: the quantiser's threads, 256 to a workgroup

// the two products; the caller has checked moe_mx_workgroups() <= 2^31 - 1.  out / a are (ys, xs) or (dxs, dys); bias may be NULL and is
// read by the forward only
int launch_moe_mx_linear(bool bwd_x, const nnop_moe_mx_desc& d, void* out, const void* a, const uint8_t* blocks, const uint8_t* scales,
                         const void* bias, const int32_t* offsets, hipStream_t s);
// the number of workgroups a product would start, computed in 64 bits
long long moe_mx_workgroups(bool bwd_x, const nnop_moe_mx_desc& d);

int launch_mxfp4_dequant(const nnop_mxfp4_desc& d, void* out, const uint8_t* blocks, const uint8_t* scales, hipStream_t s);
int launch_mxfp4_quant(const nnop_mxfp4_desc& d, uint8_t* blocks, uint8_t* scales, const void* in, hipStream_t s);

}  // namespace nnop
