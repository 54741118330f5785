/*
 * nnop_hip_paged_prefill.h -- C ABI of libnnop_hip_paged_prefill.so: the attention of a PREFILL step over a paged KV cache.  Every
 * sequence brings its own number of new tokens (a prompt behind a cached prefix, a chunk of a chunked prefill, the rows of a speculative
 * verification); their queries are packed token-major, and the keys and values -- the new tokens' included, which the caller has already
 * written -- are read from the pages where they lie (nnop_hip_paged_attn.h's pools and block table).  float16 / bfloat16, forward only.
 *
 * A thirteenth library beside libnnop_hip.so (nnop_hip.h), libnnop_hip_ext.so, libnnop_hip_moe.so, libnnop_hip_moe_data.so,
 * libnnop_hip_moe_gemm.so, libnnop_hip_moe_linear.so, libnnop_hip_moe_mx.so, libnnop_hip_moe_mx_decode.so,
 * libnnop_hip_moe_mx_decode_glu.so, libnnop_hip_decode_attn.so, libnnop_hip_decode_attn_fp8.so and libnnop_hip_paged_attn.so, built the
 * same way as the twelfth: an ABI version of its own, nothing linked from the other twelve, only this header's functions exported.
 * nnop_dtype, nnop_status and nnop_stream_t come from nnop_hip.h; a status code is turned into text by the main library's
 * nnop_strerror().  gfx950 (MI355X) only.  The launch is asynchronous on the caller's stream; nothing is allocated.
 */
#ifndef NNOP_HIP_PAGED_PREFILL_H
#define NNOP_HIP_PAGED_PREFILL_H

#include "nnop_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NNOP_HIP_PAGED_PREFILL_ABI_VERSION 1
int nnop_paged_prefill_abi_version(void);

#define NNOP_PAGED_PREFILL_BLOCK_ROWS    128 /* rows of a workgroup: (tokens of a block) x G, four waves of 32 */
#define NNOP_PAGED_PREFILL_MAX_GROUP     16  /* G = QH / KH */
#define NNOP_PAGED_PREFILL_MIN_PAGE_SIZE 16  /* a 16-key block of a tile lies in one page */

/*
 * D = `dtype`, T = `tokens` (the new tokens of all sequences), B sequences, QH query heads, KH KV heads, G = QH / KH, E = emb,
 * P = num_pages, cap = max_pages page_size.
 *
 *   q, o          [T][QH][E] of D: element (t, h, e) of q lies at q + t q_stride_t + h q_stride_h + e (strides in elements), o likewise
 *                 with its own strides; the tokens of sequence b are cu_seqlens_q[b] ... cu_seqlens_q[b + 1] - 1
 *   k, v          nnop_paged_attn's pools, with their three strides each; block_table as there
 *   cu_seqlens_q  [B + 1] int32 ON THE DEVICE, non-decreasing, cu[0] = 0; n_b = cu[b + 1] - cu[b].  Read on the device, every entry
 *                 clamped into [0, T] (a decreasing pair gives n_b = 0)
 *   seqlens       [B] int32 ON THE DEVICE: the valid keys of each sequence INCLUDING its n_b new ones; read on the device, clamped into
 *                 [0, cap]
 *   sinks         [QH] fp32 or NULL;  lse [T][QH] fp32, contiguous, or NULL
 *
 * What a query sees is nnop_paged_attn's rule with a QL of its own per sequence: query i of sequence b stands at
 * p = seqlens[b] - n_b + i and sees keys max(0, p - window_left) ... p (0 ... p without a window; a window_left >= cap is no window);
 * key j is row j mod page_size of page block_table[b][j / page_size]; the scale is 1 / sqrt(E); a sink is one more column of the
 * softmax; a row that sees no key -- p < 0 included, which seqlens[b] < n_b brings about -- has o = +0 and lse = its sink, or -inf
 * without one.  Never NaN.
 *
 * Contracts: nnop_paged_attn's, restated for this call.
 *   - The grid and the workspace size come from host values alone (T, B, QH, KH, E); cu_seqlens_q, seqlens and the table are read on
 *     the device.  No sync, no allocation, no atomics.  A captured graph follows cu_seqlens_q, seqlens, the table and the pages at
 *     fixed T and B.  Two runs are bitwise equal.
 *   - Masking is by selection: a pool row that no query of its sequence sees may hold NaN.
 *   - Only live table entries are read: those of the pages that hold a key of [lo, hi), hi = seqlens[b], lo = 0 or
 *     max(0, hi - n_b - window_left).  Within a live page, rows outside [lo, hi) are never loaded.
 *   - A page id forms no address outside the pool: every id read is clamped into [0, num_pages - 1] before it is multiplied by a page
 *     stride, in 64 bits.
 *   - Batch independence: the bits of a sequence's rows depend on its q, n_b, seqlens[b], the visible rows of its own pages and the host
 *     values (E, G, window_left) alone -- not on P, on where its pages lie, on page_size, or on the other sequences of the call.  Row
 *     blocks therefore start at a sequence's first token and never straddle two sequences.
 *   - fp32 scores, softmax and accumulation, one rounding of o.
 *
 * Work: a workgroup is (sequence, KV head, block of TB = 128 / G tokens of that sequence); the grid is kh (tokens / TB + batch), the
 * bound of sum_b ceil(n_b / TB), and every workgroup finds its block by a search over cu_seqlens_q.  So the workspace is 0 bytes:
 * nnop_paged_prefill_plan reports it, and `workspace` may be NULL.
 *
 * Checks, in this order, all before any device work:
 *   NNOP_ERR_NULL       the descriptor itself is NULL (nnop_paged_prefill_plan: or the output pointer)
 *   NNOP_ERR_DTYPE      dtype is not NNOP_F16 or NNOP_BF16
 *   NNOP_ERR_OPTS       flags or reserved is not 0; window_left < -1
 *   NNOP_ERR_SHAPE      emb not 64 or 128; tokens, batch, qh or kh < 1; qh no multiple of kh; qh / kh > 16; page_size below 16 or no
 *                       power of two; max_pages or num_pages < 1; max_pages page_size > 2^31 - 1; a K or V stride below emb or no
 *                       multiple of 8 elements; q_stride_h or o_stride_h below emb, q_stride_t or o_stride_t below qh emb, or one of
 *                       them no multiple of 8; table_stride < max_pages; kh (tokens / TB + batch) or tokens qh > 2^31 - 1
 *   NNOP_ERR_NULL       a NULL pointer; lse, sinks and the workspace are the optional ones
 *   NNOP_ERR_ALIGN      q, k, v or o not aligned to 16 bytes; block_table, cu_seqlens_q, seqlens, sinks, lse or the workspace not to 4
 *   NNOP_ERR_WORKSPACE  workspace_bytes below what nnop_paged_prefill_plan reports (0: never)
 */
typedef struct nnop_paged_prefill_desc {
    int32_t dtype;        /* nnop_dtype: NNOP_F16 or NNOP_BF16 */
    int32_t emb;          /* E: 64 or 128 */
    int32_t tokens;       /* T */
    int32_t qh;           /* query heads */
    int32_t kh;           /* KV heads */
    int32_t batch;        /* B */
    int32_t max_pages;    /* entries of a sequence's row of the table */
    int32_t window_left;  /* -1: none */
    int32_t reserved;     /* 0 */
    uint32_t flags;       /* 0 */
    int32_t page_size;    /* keys of a page: a power of two, 16 or more */
    int32_t num_pages;    /* P: pages of the pool; ids are clamped into [0, P - 1] */
    int64_t k_stride_p, k_stride_h, k_stride_l;  /* elements */
    int64_t v_stride_p, v_stride_h, v_stride_l;  /* elements */
    int64_t table_stride;                        /* int32 entries between two sequences' rows of the table, >= max_pages */
    int64_t q_stride_t, q_stride_h;              /* elements */
    int64_t o_stride_t, o_stride_h;              /* elements */
} nnop_paged_prefill_desc; /* 136 bytes: nnop_paged_attn_desc with tokens for ql, reserved for splits, and the four strides of q and o */

/* Host only: the workspace the call needs (0).  The descriptor checks above, in their order. */
int nnop_paged_prefill_plan(const nnop_paged_prefill_desc* d, size_t* workspace_bytes_out);

int nnop_paged_prefill(const nnop_paged_prefill_desc* d, void* o, float* lse, const void* q, const void* k, const void* v,
                       const int32_t* block_table, const int32_t* cu_seqlens_q, const int32_t* seqlens, const float* sinks,
                       void* workspace, size_t workspace_bytes, nnop_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NNOP_HIP_PAGED_PREFILL_H */
