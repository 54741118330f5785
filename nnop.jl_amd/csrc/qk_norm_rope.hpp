// qk_norm_rope.hpp -- what nnop_ext_capi.cpp needs of qk_norm_rope.hip (libnnop_hip_ext.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "../../include/nnop_hip_ext.h"

namespace nnop {

// bytes of fp32 partial dw rows the pullback needs (a function of the descriptor alone, whichever kernel runs)
size_t qknr_bwd_ws_bytes(const nnop_qknr_desc& d);
int launch_qknr_fwd(const nnop_qknr_desc& d, void* qo, void* ko, const void* q, const void* k, const void* wq, const void* wk,
                    const void* cos, const void* sin, hipStream_t s);
int launch_qknr_bwd(const nnop_qknr_desc& d, void* dq, void* dk, float* dwq, float* dwk, const void* gq, const void* gk,
                    const void* q, const void* k, const void* wq, const void* wk, const void* cos, const void* sin,
                    void* workspace, hipStream_t s);

}  // namespace nnop
