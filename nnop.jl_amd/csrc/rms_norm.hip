// rms_norm.hip -- RMSNorm forward and pullback, plain and with the fused residual add (kernels in norm_common.hpp, LN = false).
#include "norm_common.hpp"

namespace nnop {

size_t norm_ws_bytes(const nnop_norm_desc& d, bool ln) { return norm_bwd_ws_bytes(d, ln); }

int launch_rms_norm(const nnop_norm_desc& d, void* y, float* rms, const void* x, const void* w, float offset, float eps,
                    hipStream_t s) {
    NormParams p = norm_params(d);
    p.out = y; p.a = x; p.w = w; p.stat0 = rms; p.offset = offset; p.eps = eps;
    return launch_norm_fwd<false, false>(d, p, s);
}

int launch_rms_norm_bwd(const nnop_norm_desc& d, void* dx, float* dw, const void* dy, const float* rms, const void* x,
                        const void* w, float offset, void* ws, hipStream_t s) {
    NormParams p = norm_params(d);
    p.out = dx; p.a = dy; p.x = x; p.w = w; p.stat0 = const_cast<float*>(rms); p.offset = offset;
    p.part_w = (float*)ws;
    return launch_norm_bwd<false, false>(d, p, dw, nullptr, s);
}

// ---- fused residual add (ADD = true kernels) -------------------------------------------------------------------
int launch_add_rms_norm(const nnop_norm_desc& d, void* y, void* h, float* rms, const void* x, const void* residual,
                        const void* w, float offset, float eps, hipStream_t s) {
    NormParams p = norm_params(d);
    p.out = y; p.h = h; p.a = x; p.r = residual; p.w = w; p.stat0 = rms; p.offset = offset; p.eps = eps;
    return launch_norm_fwd<false, true>(d, p, s);
}

int launch_add_rms_norm_bwd(const nnop_norm_desc& d, void* dx, float* dw, const void* dy, const void* dh, const float* rms,
                            const void* h, const void* w, float offset, void* ws, hipStream_t s) {
    if (!dh) return launch_rms_norm_bwd(d, dx, dw, dy, rms, h, w, offset, ws, s);     // nothing to add: the plain pullback
    NormParams p = norm_params(d);
    p.out = dx; p.a = dy; p.r = dh; p.x = h; p.w = w; p.stat0 = const_cast<float*>(rms); p.offset = offset;
    p.part_w = (float*)ws;
    return launch_norm_bwd<false, true>(d, p, dw, nullptr, s);
}

}  // namespace nnop
