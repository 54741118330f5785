// glu_act.hpp -- the gated activations a(g), a'(g) and the `up` side, ONE function each: glu.hip (libnnop_hip.so, nnop_glu / nnop_glu_bwd)
// and moe_mx_decode_glu.hip (libnnop_hip_moe_mx_decode_glu.so, the activation in the epilogue of the decode forward) both compile this
// text with the same floating-point flags (BASEFLAGS), so the same fp32 gate and up give the same bits in either library.  Header-only
// code; nothing is linked between the libraries.
#pragma once
#include <hip/hip_runtime.h>
#include "fa_common.hpp"
#include "../../include/nnop_hip.h"

// Every path, layout and direction must give bitwise the same a(g) and a'(g): nothing below may be contracted into an FMA differently
// from one instantiation to the next.  Contraction is off from here to the end of the translation unit that includes this header; where
// an FMA is wanted it is written out (fmaf).
#pragma clang fp contract(off)

namespace nnop {

// ---- the activations: a(g) and a'(g), ONE function each, shared by every kernel that includes this ------------------------------------
// sigma(t) and 1 - sigma(t) without cancellation or overflow: e = exp(-|t|) <= 1, sigma(|t|) = 1 / (1 + e),
// sigma(-|t|) = e / (1 + e).  |t| is clamped at 128 first, which changes no result (exp(-104) is already 0 in fp32, so
// sigma is exactly 0 or 1 beyond) and keeps t * w below finite for an infinite t (a product that overflowed).
struct GluSig { float s, w, t; };    // sigma(t), sigma(t) (1 - sigma(t)), t clamped
NNOP_DEV GluSig glu_sigmoid(float t) {
    const float tc = fminf(fmaxf(t, -128.f), 128.f);
    const float e = expf(-fabsf(tc));
    const float r = __builtin_amdgcn_rcpf(1.f + e);
    const float lo = e * r;
    return GluSig{tc >= 0.f ? r : lo, lo * r, tc};
}

template <int ACT> struct GluAct;
// SwiGLU: a = g sigma(g), a' = sigma + g sigma (1 - sigma).  Large g: sigma = 1 and w = 0 exactly, a = g, a' = 1; large
// negative g: sigma = 0, a = a' = 0.
template <> struct GluAct<NNOP_GLU_SILU> {
    NNOP_DEV static void eval(float g, float, float, float& a, float& da) {
        const GluSig z = glu_sigmoid(g);
        a = g * z.s;
        da = fmaf(z.t, z.w, z.s);
    }
};
// GeGLU, tanh form: 0.5 (1 + tanh(x)) = sigma(2x), so a = g sigma(t), t = 2 sqrt(2/pi) g (1 + 0.044715 g^2), and
// a' = sigma + g t' sigma (1 - sigma), t' = 2 sqrt(2/pi) (1 + 3 * 0.044715 g^2).  The polynomials take g clamped at
// +-64 (t(64) is far past 128: nothing changes), so g^2 and g^3 stay finite and g t' w is finite * 0 beyond, never 0 * inf.
template <> struct GluAct<NNOP_GLU_GELU_TANH> {
    NNOP_DEV static void eval(float g, float, float, float& a, float& da) {
        constexpr float k2 = 1.5957691216057308f, c = 0.044715f;       // 2 sqrt(2 / pi)
        const float gc = fminf(fmaxf(g, -64.f), 64.f);
        const float g2 = gc * gc;
        const float t = (k2 * gc) * fmaf(c, g2, 1.f);
        const float tp = k2 * fmaf(3.f * c, g2, 1.f);
        const GluSig z = glu_sigmoid(t);
        a = g * z.s;
        da = fmaf(gc * tp, z.w, z.s);
    }
};
// GeGLU, exact: a = g Phi(g), Phi(g) = 0.5 erfc(-g / sqrt 2) (erfc: no cancellation in the lower tail, which
// 0.5 (1 + erf) has), a' = Phi + g phi(g), phi(g) = exp(-g^2 / 2) / sqrt(2 pi).  phi takes g clamped at +-64
// (exp(-2048) = 0 already), so g^2 cannot overflow.
template <> struct GluAct<NNOP_GLU_GELU_ERF> {
    NNOP_DEV static void eval(float g, float, float, float& a, float& da) {
        const float cdf = 0.5f * erfcf(g * -0.70710678118654752f);
        const float gc = fminf(fmaxf(g, -64.f), 64.f);
        const float pdf = expf(-0.5f * (gc * gc)) * 0.3989422804014327f;
        a = g * cdf;
        da = fmaf(gc, pdf, cdf);
    }
};
// gpt-oss: g' = min(g, limit), a = g' sigma(alpha g'), a' = sigma + alpha g' sigma (1 - sigma) where g <= limit, else 0
// (torch's clamp convention: the gradient passes on the bound).
template <> struct GluAct<NNOP_GLU_SWIGLU_OAI> {
    NNOP_DEV static void eval(float g, float alpha, float limit, float& a, float& da) {
        const float gp = fminf(g, limit);
        const GluSig z = glu_sigmoid(alpha * gp);
        a = gp * z.s;
        da = g <= limit ? fmaf(z.t, z.w, z.s) : 0.f;
    }
};

// the `up` side: u itself, or for gpt-oss clamp(u, -limit, limit) + 1 with the clamp's gradient mask
template <int ACT> NNOP_DEV void glu_up(float u, float limit, float& uu, float& um) {
    if constexpr (ACT == NNOP_GLU_SWIGLU_OAI) {
        uu = fminf(fmaxf(u, -limit), limit) + 1.f;
        um = (u >= -limit && u <= limit) ? 1.f : 0.f;
    } else {
        uu = u; um = 1.f;
    }
}

template <int ACT> NNOP_DEV float glu_fwd_elem(float g, float u, float alpha, float limit) {
    float a, da, uu, um;
    GluAct<ACT>::eval(g, alpha, limit, a, da);
    glu_up<ACT>(u, limit, uu, um);
    return a * uu;
}
template <int ACT> NNOP_DEV void glu_bwd_elem(float dy, float g, float u, float alpha, float limit, float& dg, float& du) {
    float a, da, uu, um;
    GluAct<ACT>::eval(g, alpha, limit, a, da);
    glu_up<ACT>(u, limit, uu, um);
    dg = (dy * uu) * da;
    du = (dy * a) * um;
}

}  // namespace nnop
