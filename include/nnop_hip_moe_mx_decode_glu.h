/*
 * nnop_hip_moe_mx_decode_glu.h -- C ABI of libnnop_hip_moe_mx_decode_glu.so: the first half of an expert MLP at decode sizes in one
 * launch.  It is the weight-streaming forward of nnop_hip_moe_mx_decode.h on a fused gate-up projection (MXFP4 weights, 2 I rows per
 * expert) with the gated activation of nnop_glu (nnop_hip.h) in its epilogue and, optionally, the token gather of nnop_moe_permute
 * (nnop_hip_moe_data.h) in front: what nnop_moe_permute -> nnop_moe_mx_decode_linear -> nnop_glu compute in three launches, without the
 * [S][2 I] pre-activations ever being rounded, written or read back.  There is no pullback here: the gradients are those of the three
 * calls it replaces.
 *
 * A ninth library beside libnnop_hip.so (nnop_hip.h), libnnop_hip_ext.so, libnnop_hip_moe.so, libnnop_hip_moe_data.so,
 * libnnop_hip_moe_gemm.so, libnnop_hip_moe_linear.so, libnnop_hip_moe_mx.so and libnnop_hip_moe_mx_decode.so, built the same way as the
 * eighth: an ABI version of its own, nothing linked from the other eight, only this header's functions exported.  nnop_dtype,
 * nnop_status, nnop_stream_t and the nnop_glu_act values come from nnop_hip.h; a status code is turned into text by the main library's
 * nnop_strerror().  gfx950 (MI355X) only.  The launch is asynchronous on the caller's stream; nothing is allocated and there is no
 * workspace.
 *
 * The format is that of nnop_hip_moe_mx.h (OCP Microscaling Formats v1.0, MXFP4): 32 values share a scale byte e (2^(e - 127); 255: NaN)
 * and are 4-bit E2M1 codes, 16 bytes per block, element 2j in the low nibble of byte j.
 */
#ifndef NNOP_HIP_MOE_MX_DECODE_GLU_H
#define NNOP_HIP_MOE_MX_DECODE_GLU_H

#include "nnop_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NNOP_HIP_MOE_MX_DECODE_GLU_ABI_VERSION 1
int nnop_moe_mx_decode_glu_abi_version(void);

/* where gate and up lie among the N = 2 I weight rows (and bias columns) of an expert */
#define NNOP_MOE_GLU_INTERLEAVED 0 /* gate of output j is row 2j, up row 2j + 1 (gpt-oss) */
#define NNOP_MOE_GLU_HALVES      1 /* gate of output j is row j, up row I + j */

/*
 * S slot rows, E experts, K input features, I output features of h; the packed weights have N = 2 I rows per expert.  W_e(n, c) is the
 * value nnop_mxfp4_dequant gives for element c of weight row n of expert e, in `dtype`.
 *
 *   offsets [E+1] int32              as nnop_moe_plan writes it
 *   perm    [S] int32                as nnop_moe_plan writes it, or NULL
 *   x       [S][ld_x] of `dtype`     perm NULL: slot order, K columns;  with perm: [T][ld_x], token order
 *   h       [S][ld_h] of `dtype`     slot order, I columns
 *   blocks  [E][2 I][ld_q] uint8     K / 2 bytes of a row are read; experts lie 2 I ld_q bytes apart
 *   scales  [E][2 I][ld_s] uint8     K / 32 bytes of a row are read; experts lie 2 I ld_s bytes apart
 *   bias    [E][ld_b] of `dtype`     2 I columns; NULL: no bias
 *
 *   p[s][n] = sum_c xrow(s)[c] W_e(n, c) + bias[e][n]             fp32, offsets[e] <= s < offsets[e+1]
 *   h[s][j] = round( a(gate) * upside(up) )                       gate, up = p[s][2j], p[s][2j+1]   (interleaved)
 *                                                                 gate, up = p[s][j],  p[s][I+j]    (halves)
 *   xrow(s) = x[s]                                                perm NULL
 *   xrow(s) = x[perm[s] / topk] if (uint32)perm[s] < tokens topk, else a row of +0      with perm
 *
 * a and upside are those of nnop_glu for `act` (NNOP_GLU_SILU, _GELU_TANH, _GELU_ERF: upside(u) = u; NNOP_GLU_SWIGLU_OAI: a(g) =
 * g' sigma(alpha g'), g' = min(g, limit), upside(u) = clamp(u, -limit, limit) + 1).  Every row of h outside every expert comes back as +0
 * in the columns that exist.  Padding columns are untouched.
 *
 * Contracts:
 *   - Precision: the pre-activations p stay fp32.  Sums are fp32 on the matrix cores, the bias is added in fp32, the activation is
 *     evaluated in fp32, and there is one rounding, on the store.
 *   - Summation order: p is summed in the order of nnop_moe_mx_decode_linear, a function of K and `dtype` alone.  A row's bits do not
 *     depend on the plan, on its slot, on its neighbours, or on whether it came through perm; the two layouts give the same bits for the
 *     same weights and bias laid out either way.
 *   - No atomics, no workspace, no allocation, no sync; the call can be captured in a graph.  Two runs are bitwise equal.
 *   - offsets is read on the device, clamped into [0, S].  perm is read on the device; an entry outside [0, tokens topk) is a row of +0,
 *     so its row of h is the activation of the bias alone, exactly what nnop_moe_permute followed by the linear layer gives.  Nothing is
 *     read or written out of bounds whatever either array holds.
 *   - Masking is by selection: the blocks and scales of another expert (a scale byte of 255 included), the rows of x that no valid perm
 *     entry of an expert's range names (without perm: the rows outside an expert) and the padding never enter a result that is kept.
 *   - Same inputs, same code: the fp32 pre-activations are the ones nnop_moe_mx_decode_linear rounds, and the activation code is
 *     nnop_glu's.  Wherever every p is exactly representable in `dtype`, h equals nnop_glu applied to nnop_moe_mx_decode_linear's output,
 *     bit for bit.  Elsewhere h carries one rounding where that composition carries two.
 *   - Made for few rows per expert, as nnop_moe_mx_decode_linear is: an expert with up to 32 rows streams its weights once.
 *   - x takes 16-byte loads where ld_x is a multiple of 8 and x is 16-byte aligned, element-wise loads otherwise.  Interleaved: h takes
 *     4-byte stores where ld_h is even and h is 4-byte aligned.  Halves: h takes 8-byte stores where ld_h is a multiple of 4 and h is
 *     8-byte aligned.  The bias takes 8-byte loads where ld_b (halves: and I) is a multiple of 4 and the bias is 8-byte aligned.
 *     Element-wise accesses otherwise.  Any I >= 1.
 *
 * Checks, in this order, all before any device work:
 *   NNOP_ERR_NULL    the descriptor itself is NULL
 *   NNOP_ERR_DTYPE   dtype is not NNOP_F16 or NNOP_BF16
 *   NNOP_ERR_OPTS    flags is not 0, or a reserved field is not 0; an unknown act or layout; with NNOP_GLU_SWIGLU_OAI only (the fields
 *                    are ignored otherwise) an alpha that is not finite or a limit that is not finite and positive
 *   NNOP_ERR_SHAPE   S < 1, E outside 1 ... 1024, K outside 1 ... 65536, I outside 1 ... 32768 (N = 2 I <= 65536), K no multiple of 32,
 *                    ld_x < K, ld_h < I, ld_b < 2 I, ld_q < K / 2 or no multiple of 16, ld_s < K / 32; tokens or topk below 0, or, when
 *                    either is not 0, tokens < 1, topk outside 1 ... 64 or tokens topk > 2^31 - 1; perm NULL while tokens and topk are
 *                    not 0, or perm given while they are 0; more than 2^31 - 1 workgroups (E ceil(I / 128): the bounds on E and I keep
 *                    it below that)
 *   NNOP_ERR_NULL    a NULL pointer; bias and perm are the optional ones
 *   NNOP_ERR_ALIGN  a row array or the bias not aligned to its element size, blocks not aligned to 16 bytes, offsets or perm not to 4
 */
typedef struct nnop_moe_mx_decode_glu_desc {
    int32_t dtype;        /* nnop_dtype of the rows and the bias: NNOP_F16 or NNOP_BF16 */
    int32_t rows;         /* S */
    int32_t experts;      /* E */
    int32_t in_dim;       /* K, a multiple of 32 */
    int32_t inter_dim;    /* I: the columns of h; the packed weights have 2 I rows per expert */
    int32_t ld_x;         /* row stride of x in elements */
    int32_t ld_h;         /* row stride of h in elements */
    int32_t ld_b;         /* row stride of bias in elements: >= 2 I */
    int32_t ld_q;         /* bytes between two packed weight rows: >= K / 2, a multiple of 16 */
    int32_t ld_s;         /* bytes between two scale rows: >= K / 32 */
    int32_t act;          /* nnop_glu_act */
    int32_t layout;       /* NNOP_MOE_GLU_INTERLEAVED or NNOP_MOE_GLU_HALVES */
    int32_t tokens;       /* T with perm, 0 without */
    int32_t topk;         /* k with perm (1 ... 64), 0 without */
    float alpha;          /* NNOP_GLU_SWIGLU_OAI only */
    float limit;          /* NNOP_GLU_SWIGLU_OAI only */
    uint32_t flags;       /* 0 */
    int32_t reserved[3];  /* 0 */
} nnop_moe_mx_decode_glu_desc; /* 80 bytes */

int nnop_moe_mx_decode_glu(const nnop_moe_mx_decode_glu_desc* d, void* h, const void* x, const uint8_t* blocks, const uint8_t* scales,
                           const void* bias, const int32_t* offsets, const int32_t* perm, nnop_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NNOP_HIP_MOE_MX_DECODE_GLU_H */
