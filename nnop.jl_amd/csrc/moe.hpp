// moe.hpp -- what nnop_moe_capi.cpp needs of moe_router.hip and moe_plan.hip (libnnop_hip_moe.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "../../include/nnop_hip_moe.h"

namespace nnop {

constexpr int kMoeMaxExperts = 1024;
constexpr int kMoeMaxTopk = 16;

int launch_moe_router_fwd(const nnop_moe_router_desc& d, int32_t* idx, float* w, float* lse, const void* logits, hipStream_t s);
int launch_moe_router_bwd(const nnop_moe_router_desc& d, void* dlogits, const float* dw, const float* dlse, const float* w,
                          const int32_t* idx, const float* lse, const void* logits, hipStream_t s);

// bytes of per-chunk histograms the plan needs (a function of the descriptor alone)
size_t moe_plan_ws_bytes(const nnop_moe_plan_desc& d);
int launch_moe_plan(const nnop_moe_plan_desc& d, int32_t* counts, int32_t* offsets, int32_t* perm, int32_t* slot, const int32_t* idx,
                    void* workspace, hipStream_t s);

}  // namespace nnop
