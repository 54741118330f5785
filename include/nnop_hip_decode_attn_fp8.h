/*
 * nnop_hip_decode_attn_fp8.h -- C ABI of libnnop_hip_decode_attn_fp8.so: the attention of a decode step (nnop_hip_decode_attn.h) over a
 * KV cache kept in 8-bit floating point.  K and V are one-byte OCP E4M3 codes ("fn": no infinities, NaN = 0x7F / 0xFF) with one fp32
 * scale per KV head each; q, o and the arithmetic stay float16 / bfloat16 with fp32 accumulation.  The codes are read where they lie
 * and expanded in registers, exactly: every finite E4M3 value is a float16 and a bfloat16 value.  Half the cache bytes of the 16-bit
 * call per step, and no dequantised copy of the cache.
 *
 * An eleventh library beside libnnop_hip.so (nnop_hip.h), libnnop_hip_ext.so, libnnop_hip_moe.so, libnnop_hip_moe_data.so,
 * libnnop_hip_moe_gemm.so, libnnop_hip_moe_linear.so, libnnop_hip_moe_mx.so, libnnop_hip_moe_mx_decode.so,
 * libnnop_hip_moe_mx_decode_glu.so and libnnop_hip_decode_attn.so, built the same way as the tenth: an ABI version of its own, nothing
 * linked from the other ten, only this header's functions exported.  nnop_dtype, nnop_status and nnop_stream_t come from nnop_hip.h; a
 * status code is turned into text by the main library's nnop_strerror().  gfx950 (MI355X) only.  The launch is asynchronous on the
 * caller's stream; nothing is allocated; the workspace is the caller's.
 */
#ifndef NNOP_HIP_DECODE_ATTN_FP8_H
#define NNOP_HIP_DECODE_ATTN_FP8_H

#include "nnop_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NNOP_HIP_DECODE_ATTN_FP8_ABI_VERSION 1
int nnop_decode_attn_fp8_abi_version(void);

#define NNOP_DECODE_ATTN_FP8_MAX_ROWS   16 /* G QL, the rows of one 16-wide matrix operand */
#define NNOP_DECODE_ATTN_FP8_MAX_SPLITS 64
#define NNOP_DECODE_ATTN_FP8_E4M3       0  /* kv_format: OCP E4M3, torch.float8_e4m3fn */

/*
 * T = `dtype`, B sequences, QH query heads, KH KV heads, G = QH / KH, E = emb, cap = capacity.
 *
 *   q        [B][QH][QL][E] of T, contiguous
 *   k, v     bytes: the code of element (b, kvh, j, e) of k lies at k + b k_stride_b + kvh k_stride_h + j k_stride_l + e (an element is a
 *            byte, so the strides are bytes), v likewise: [B][KH][cap][E] and [B][cap][KH][E] caches are both read where they lie
 *   k_scale  [KH] fp32 ON THE DEVICE or NULL (= 1): the value of a K element is its code's value times k_scale[kvh]
 *   v_scale  [KH] fp32 ON THE DEVICE or NULL (= 1): likewise for V
 *   seqlens  [B] int32 ON THE DEVICE: the valid keys of each sequence INCLUDING its QL new ones; read on the device, clamped into [0, cap]
 *   sinks    [QH] fp32 or NULL: one more softmax column per query head that has no value vector
 *   o        [B][QH][QL][E] of T
 *   lse      [B][QH][QL] fp32 or NULL
 *
 * Alignment is bottom-right.  Query i of sequence b stands at position p = seqlens[b] - QL + i and sees key j iff
 *   0 <= j <= p,  j < seqlens[b],  and window_left < 0 or j >= p - window_left.
 * A window_left >= capacity removes no key and is taken as no window.
 * x_j = (q . code(k_j)) (k_scale[kvh] / sqrt(E)): the factor is formed once in fp32 and applied to the fp32 scores;
 * o = v_scale[kvh] sum_j softmax(x [, sigma_h])_j code(v_j), the scale applied in fp32 in front of the one rounding of o;
 * lse = log(sum_j exp(x_j) [+ exp(sigma_h)]).  The sink and lse are in the domain of the scaled scores, as in nnop_decode_attn.
 *
 * A row that sees no key (p < 0, seqlens[b] = 0) gives o = +0, and lse = sigma_h with a sink, -inf without one (or with a sink of -inf),
 * as in nnop_decode_attn and for its reason: a decode batch under graph capture carries padded sequences of length 0.
 * A NaN code in a cache row that a query sees propagates: that query's row of o is NaN.
 *
 * Contracts:
 *   - Device-side lengths, host-side grid: the grid depends on batch, kh and the resolved split count alone.  No sync, no allocation, no
 *     atomics; the call can be captured in a graph and replayed after seqlens, the cache contents and the scales have changed.  Two runs
 *     are bitwise equal.
 *   - Masking is by selection: nothing of a cache row that no query of its sequence sees -- rows at or behind seqlens[b], rows in front
 *     of the window, another sequence's rows -- enters a result, even where such a row holds the NaN code.  Their scores are replaced,
 *     and their V rows are replaced by zero bytes (+0) in front of the second product (0 x NaN is NaN on the matrix cores).  Loads are
 *     unconditional, from addresses clamped to a cache row that exists.
 *   - Batch independence: the bits of sequence b's rows depend on its q, its visible cache rows, the scales, seqlens[b] and the host
 *     values (QL, E, G, window_left, the resolved split count) alone -- not on B, nor on the other sequences or their lengths.  The
 *     chunk boundaries of a sequence are computed on the device from its own live key range.
 *   - Precision: the conversion of a code to T is exact; both matrix products are on T with fp32 accumulation (the 8-bit matrix
 *     instructions are not used: the probabilities are rounded to T, not to 8 bits); fp32 scores, softmax and accumulation; one
 *     rounding of o to T; lse is fp32.
 *
 * Work split.  The live range of sequence b is [lo, hi): hi = seqlens[b], lo = 0 or, with a window, max(0, hi - QL - window_left)
 * rounded down to a tile of 32 keys.  It is cut into `splits` runs of ceil(tiles / splits) whole tiles; chunk c takes the c-th run, and a
 * chunk without tiles contributes nothing.  With more than one split, fp32 partial results go through the workspace and a second kernel
 * merges the chunks of a row in ascending order.
 *
 * The automatic split count (splits = 0), from host values only -- nnop_decode_attn's rule, so the two calls plan alike:
 *   tiles  = ceil(capacity / 32); with a window: min(that, (ql + window_left) / 32 + 2)
 *   splits = ceil(512 / (batch kh))          about two workgroups for each of the 256 compute units
 *   splits = min(splits, tiles / 4)          no chunk below one round of the four waves of a workgroup
 *   splits = min(max(splits, 1), 64)
 * A forced count (splits >= 1) is used as it is, up to 64.
 * workspace bytes = 0 at one split, else 4 batch qh ql splits (emb + 2).
 *
 * Checks, in this order, all before any device work:
 *   NNOP_ERR_NULL       the descriptor itself is NULL (nnop_decode_attn_fp8_plan: or an output pointer)
 *   NNOP_ERR_DTYPE      dtype is not NNOP_F16 or NNOP_BF16
 *   NNOP_ERR_OPTS       flags is not 0, kv_format is not NNOP_DECODE_ATTN_FP8_E4M3, or reserved is not 0; window_left < -1; splits < 0 or
 *                       > 64
 *   NNOP_ERR_SHAPE      emb not 64 or 128; batch, qh or kh < 1; qh no multiple of kh; ql < 1; (qh / kh) ql > 16; capacity < ql; a stride
 *                       below emb or no multiple of 16; batch kh splits or batch qh ql (the rows of o) > 2^31 - 1
 *   NNOP_ERR_NULL       a NULL pointer; lse, k_scale, v_scale, sinks and, at a resolved split count of 1, the workspace are the optional
 *                       ones
 *   NNOP_ERR_ALIGN      q, k, v or o not aligned to 16 bytes; k_scale, v_scale, seqlens, sinks, lse or the workspace not to 4
 *   NNOP_ERR_WORKSPACE  workspace_bytes below what nnop_decode_attn_fp8_plan reports
 */
typedef struct nnop_decode_attn_fp8_desc {
    int32_t dtype;        /* nnop_dtype of q and o: NNOP_F16 or NNOP_BF16 */
    int32_t emb;          /* E: 64 or 128 */
    int32_t ql;           /* new tokens per sequence */
    int32_t qh;           /* query heads */
    int32_t kh;           /* KV heads */
    int32_t batch;        /* B */
    int32_t capacity;     /* rows of a sequence's cache */
    int32_t window_left;  /* -1: none */
    int32_t splits;       /* 0: automatic; >= 1: forced */
    uint32_t flags;       /* 0 */
    int32_t kv_format;    /* NNOP_DECODE_ATTN_FP8_E4M3 */
    int32_t reserved;     /* 0 */
    int64_t k_stride_b, k_stride_h, k_stride_l;  /* bytes */
    int64_t v_stride_b, v_stride_h, v_stride_l;  /* bytes */
} nnop_decode_attn_fp8_desc; /* 96 bytes: the layout of nnop_decode_attn_desc, kv_format in the place of reserved[0] */

/* Host only: the split count the call will use and the workspace it then needs.  The descriptor checks above, in their order. */
int nnop_decode_attn_fp8_plan(const nnop_decode_attn_fp8_desc* d, int32_t* splits_out, size_t* workspace_bytes_out);

int nnop_decode_attn_fp8(const nnop_decode_attn_fp8_desc* d, void* o, float* lse, const void* q, const void* k, const void* v,
                         const float* k_scale, const float* v_scale, const int32_t* seqlens, const float* sinks, void* workspace,
                         size_t workspace_bytes, nnop_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NNOP_HIP_DECODE_ATTN_FP8_H */
