/*
 * nnop_hip_ext.h -- C ABI of libnnop_hip_ext.so: operators beyond the NNop drop-in boundary of nnop_hip.h.
 *
 * nnop_hip.h mirrors NNop.jl's operators one for one and its ABI is frozen with them.  Operators that NNop.jl does not have live
 * in this second library with an ABI version of its own, the way flash-attn ships its rotary, layer-norm and xentropy kernels as
 * separate extensions.  The two libraries link nothing from each other; this header takes nnop_dtype, nnop_status and
 * nnop_stream_t from nnop_hip.h, and a status code is turned into text by the main library's nnop_strerror().
 * gfx950 (MI355X) only, like the main library.  Launches are asynchronous on the caller's stream; nothing is allocated.
 */
#ifndef NNOP_HIP_EXT_H
#define NNOP_HIP_EXT_H

#include "nnop_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NNOP_HIP_EXT_ABI_VERSION 1
int nnop_ext_abi_version(void);

/*
 * Fused QK-norm + RoPE: the per-head RMSNorm that Qwen3, Gemma 3 and OLMo 2 put on q and k, then the Llama rotary embedding,
 * in one pass over q and k (2 row-sized moves per tensor instead of the 4 of rms_norm, rms_norm, llama_rope; the normalised
 * value is never rounded to the element type between norm and rotation).
 *
 * Layouts are those of nnop_llama_rope:  q [B][QH][L][D], k [B][KH][L][D] of `dtype`;  cos, sin [B][L][D] of `cs_dtype`
 * (only the first D/2 of a row are read);  wq, wk [D] of `w_dtype`, two separate weights.
 * Per head row x (fp32 arithmetic, one rounding to `dtype` on store):
 *     rstd = 1/sqrt(mean(x^2) + eps)          n = x * rstd * (w + offset)
 *     y[i] = n[i] c[i] - n[i+D/2] s[i]        y[i+D/2] = n[i+D/2] c[i] + n[i] s[i]           i < D/2
 * Pullback, with rstd recomputed from x (the forward saves nothing):
 *     dn = the rotation of dy with sin_sign = -1      m = dn (w + offset)      dd = sum(m x)
 *     dx = rstd m - rstd^3 (dd/D) x                   dw[j] = sum over rows of dn[j] x[j] rstd        (fp32)
 * dwq sums over the B QH L rows of q, dwk over the B KH L rows of k.  dw is deterministic: per-workgroup partial rows in the
 * caller's workspace, folded in a fixed order by a second kernel, no atomics; every partial the fold reads is written first,
 * whatever the workspace held.
 *
 * Shapes: every even D in 2 ... 512.  D % 16 == 0 with D/16 a power of two (16, 32, 64, 128, 256, 512) and 16-byte-aligned bases
 * take the 16-byte path (D/16 lanes per row); everything else an element-wise kernel.
 * Aliasing: q_out == q, k_out == k, dq == dq_out and dk == dk_out are allowed and give bitwise the out-of-place result.
 *
 * Checks, in this order, all before any device work:
 *   NNOP_ERR_DTYPE      one of the three dtypes is unknown, or w_dtype / cs_dtype is neither NNOP_F32 nor dtype
 *   NNOP_ERR_OPTS       a reserved field is not 0, eps is not finite or is negative, offset is not finite
 *   NNOP_ERR_SHAPE      D odd, D > 512, a non-positive extent, or more work than one launch takes (2^31 - 1 head rows)
 *   NNOP_ERR_NULL       a NULL pointer (the descriptor itself: first of all)
 *   NNOP_ERR_ALIGN      a base not aligned to its element size, or a workspace not aligned to 16 bytes
 *   NNOP_ERR_WORKSPACE  workspace_bytes < nnop_qk_norm_rope_bwd_workspace_bytes()
 *
 * reserved[] is kept for what this version leaves out: partial rotary (rot_dim < D), interleaved (GPT-J) pairing, a norm-only
 * or rope-only mode, a saved rstd, q without k.
 */
typedef struct nnop_qknr_desc {
    int32_t dtype;      /* nnop_dtype of q, k, outputs and incoming/outgoing gradients */
    int32_t w_dtype;    /* wq, wk: NNOP_F32 or dtype */
    int32_t cs_dtype;   /* cos, sin: NNOP_F32 or dtype */
    int32_t dim, seq, qh, kh, batch;   /* D, L, QH, KH, B */
    float   eps, offset;               /* g = w + offset (Gemma: 1) */
    int32_t reserved[2];               /* 0 */
} nnop_qknr_desc;                      /* 48 bytes */

int nnop_qk_norm_rope(const nnop_qknr_desc* d, void* q_out, void* k_out, const void* q, const void* k,
                      const void* wq, const void* wk, const void* cos, const void* sin, nnop_stream_t stream);
/* 0 for NULL and for a descriptor that fails the descriptor checks */
size_t nnop_qk_norm_rope_bwd_workspace_bytes(const nnop_qknr_desc* d);
int nnop_qk_norm_rope_bwd(const nnop_qknr_desc* d, void* dq, void* dk, float* dwq, float* dwk,
                          const void* dq_out, const void* dk_out, const void* q, const void* k,
                          const void* wq, const void* wk, const void* cos, const void* sin,
                          void* workspace, size_t workspace_bytes, nnop_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NNOP_HIP_EXT_H */
