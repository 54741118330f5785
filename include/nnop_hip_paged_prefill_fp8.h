/*
 * nnop_hip_paged_prefill_fp8.h -- C ABI of libnnop_hip_paged_prefill_fp8.so: the attention of a PREFILL step (nnop_hip_paged_prefill.h)
 * over a paged KV cache of one-byte OCP E4M3 codes (nnop_hip_paged_attn_fp8.h's pools: pages of codes with one fp32 scale per KV head
 * for K and for V).  Every sequence brings its own number of new tokens; their queries are packed token-major, and the keys and values
 * -- the new tokens' included, which the caller has already quantised and written -- are read from the pages where they lie.  The codes
 * are expanded to the type of q in the registers that stage a tile for LDS: no dense copy of a sequence's keys is gathered per step and
 * no 16-bit copy of the pool is kept.  A caller who keeps an E4M3 pool runs its prefill steps here and its decode steps through
 * nnop_paged_attn_fp8 over the same pages.  float16 / bfloat16 queries, forward only.
 *
 * A fifteenth library beside libnnop_hip.so (nnop_hip.h), libnnop_hip_ext.so, libnnop_hip_moe.so, libnnop_hip_moe_data.so,
 * libnnop_hip_moe_gemm.so, libnnop_hip_moe_linear.so, libnnop_hip_moe_mx.so, libnnop_hip_moe_mx_decode.so,
 * libnnop_hip_moe_mx_decode_glu.so, libnnop_hip_decode_attn.so, libnnop_hip_decode_attn_fp8.so, libnnop_hip_paged_attn.so,
 * libnnop_hip_paged_prefill.so and libnnop_hip_paged_attn_fp8.so, built the same way as the twelfth: an ABI version of its own, nothing
 * linked from the other fourteen, only this header's functions exported.  nnop_dtype, nnop_status and nnop_stream_t come from
 * nnop_hip.h; a status code is turned into text by the main library's nnop_strerror().  gfx950 (MI355X) only.  The launch is
 * asynchronous on the caller's stream; nothing is allocated.
 */
#ifndef NNOP_HIP_PAGED_PREFILL_FP8_H
#define NNOP_HIP_PAGED_PREFILL_FP8_H

#include "nnop_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NNOP_HIP_PAGED_PREFILL_FP8_ABI_VERSION 1
int nnop_paged_prefill_fp8_abi_version(void);

#define NNOP_PAGED_PREFILL_FP8_BLOCK_ROWS    128 /* rows of a workgroup: (tokens of a block) x G, four waves of 32 */
#define NNOP_PAGED_PREFILL_FP8_MAX_GROUP     16  /* G = QH / KH */
#define NNOP_PAGED_PREFILL_FP8_MIN_PAGE_SIZE 16  /* a 16-key block of a tile lies in one page */
#define NNOP_PAGED_PREFILL_FP8_E4M3          0   /* kv_format: OCP E4M3, torch.float8_e4m3fn */

/*
 * D = `dtype`, T = `tokens` (the new tokens of all sequences), B sequences, QH query heads, KH KV heads, G = QH / KH, E = emb,
 * P = num_pages, cap = max_pages page_size.
 *
 *   q, o          [T][QH][E] of D: element (t, h, e) of q lies at q + t q_stride_t + h q_stride_h + e (strides in elements), o likewise
 *                 with its own strides; the tokens of sequence b are cu_seqlens_q[b] ... cu_seqlens_q[b + 1] - 1
 *   k, v          the pools, bytes: the code of element (page, kvh, r, e) of k lies at k + page k_stride_p + kvh k_stride_h +
 *                 r k_stride_l + e (an element is a byte, so the strides are bytes), v likewise with its own strides:
 *                 [P][KH][page_size][E] and [P][page_size][KH][E] pools are both read where they lie
 *   k_scale       [KH] fp32 ON THE DEVICE or NULL (= 1): the value of a K element is its code's value times k_scale[kvh]
 *   v_scale       [KH] fp32 ON THE DEVICE or NULL (= 1): likewise for V
 *   block_table   int32 ON THE DEVICE: entry (b, n) at block_table + b table_stride + n, n < max_pages, is the page that holds keys
 *                 n page_size ... (n + 1) page_size - 1 of sequence b; K and V share it
 *   cu_seqlens_q  [B + 1] int32 ON THE DEVICE, non-decreasing, cu[0] = 0; n_b = cu[b + 1] - cu[b].  Read on the device, every entry
 *                 clamped into [0, T] (a decreasing pair gives n_b = 0)
 *   seqlens       [B] int32 ON THE DEVICE: the valid keys of each sequence INCLUDING its n_b new ones; read on the device, clamped into
 *                 [0, cap]
 *   sinks         [QH] fp32 or NULL;  lse [T][QH] fp32, contiguous, or NULL
 *
 * What a query sees is nnop_paged_prefill's rule: query i of sequence b stands at p = seqlens[b] - n_b + i and sees keys
 * max(0, p - window_left) ... p (0 ... p without a window; a window_left >= cap is no window); key j is row j mod page_size of page
 * block_table[b][j / page_size].  The scales are nnop_decode_attn_fp8's: k_scale[kvh] / sqrt(E) is ONE factor on the fp32 scores, so
 * sinks and lse are in the domain of the scaled scores; v_scale[kvh] multiplies the fp32 o after the division and in front of its one
 * rounding.  A sink is one more column of the softmax; a row that sees no key -- p < 0 included, which seqlens[b] < n_b brings about --
 * has o = +0 and lse = its sink, or -inf without one.  A NaN code (0x7F, 0xFF) in a row some query of the sequence sees gives NaN; one
 * in a row that no query of its sequence sees changes nothing.
 *
 * Contracts: nnop_paged_prefill's, restated for this call, and the conversion.
 *   - The grid and the workspace size come from host values alone (T, B, QH, KH, E); cu_seqlens_q, seqlens, the table and the scales
 *     are read on the device.  No sync, no allocation, no atomics.  A captured graph follows cu_seqlens_q, seqlens, the table, the
 *     pages and the scales at fixed T and B.  Two runs are bitwise equal.
 *   - Masking is by selection: a pool row that no query of its sequence sees may hold anything, the NaN codes included.
 *   - Only live table entries are read: those of the pages that hold a key of [lo, hi), hi = seqlens[b], lo = 0 or
 *     max(0, hi - n_b - window_left).  Within a live page, rows outside [lo, hi) are never loaded.
 *   - A page id forms no address outside the pool: every id read is clamped into [0, num_pages - 1] before it is multiplied by a page
 *     stride, in 64 bits.
 *   - Batch independence: the bits of a sequence's rows depend on its q, n_b, seqlens[b], the visible rows of its own pages, the
 *     scales and the host values (E, G, window_left) alone -- not on P, on where its pages lie, on page_size, or on the other
 *     sequences of the call.
 *   - The conversion of a code to D is exact (all 254 finite codes are values of float16 and of bfloat16) and the scales never touch
 *     the codes.  Both products run on D with fp32 accumulation; fp32 scores, softmax and accumulation, one rounding of o.  So without
 *     scales o and lse equal, bit for bit, what nnop_paged_prefill gives on a pool that holds the same values in D.
 *
 * Work: nnop_paged_prefill's.  A workgroup is (sequence, KV head, block of TB = 128 / G tokens of that sequence); the grid is
 * kh (tokens / TB + batch), and every workgroup finds its block by a search over cu_seqlens_q.  So the workspace is 0 bytes:
 * nnop_paged_prefill_fp8_plan reports it, and `workspace` may be NULL.
 *
 * Checks, in this order, all before any device work:
 *   NNOP_ERR_NULL       the descriptor itself is NULL (nnop_paged_prefill_fp8_plan: or the output pointer)
 *   NNOP_ERR_DTYPE      dtype is not NNOP_F16 or NNOP_BF16
 *   NNOP_ERR_OPTS       flags is not 0, kv_format is not NNOP_PAGED_PREFILL_FP8_E4M3, or reserved or reserved2 is not 0;
 *                       window_left < -1
 *   NNOP_ERR_SHAPE      emb not 64 or 128; tokens, batch, qh or kh < 1; qh no multiple of kh; qh / kh > 16; page_size below 16 or no
 *                       power of two; max_pages or num_pages < 1; max_pages page_size > 2^31 - 1; a K or V stride below emb or no
 *                       multiple of 16 bytes; q_stride_h or o_stride_h below emb, q_stride_t or o_stride_t below qh emb, or one of
 *                       them no multiple of 8 elements; table_stride < max_pages; kh (tokens / TB + batch) or tokens qh > 2^31 - 1
 *   NNOP_ERR_NULL       a NULL pointer; lse, k_scale, v_scale, sinks and the workspace are the optional ones
 *   NNOP_ERR_ALIGN      q, k, v or o not aligned to 16 bytes; k_scale, v_scale, block_table, cu_seqlens_q, seqlens, sinks, lse or the
 *                       workspace not to 4
 *   NNOP_ERR_WORKSPACE  workspace_bytes below what nnop_paged_prefill_fp8_plan reports (0: never)
 */
typedef struct nnop_paged_prefill_fp8_desc {
    int32_t dtype;        /* nnop_dtype of q and o: NNOP_F16 or NNOP_BF16 */
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
    int32_t kv_format;    /* NNOP_PAGED_PREFILL_FP8_E4M3 */
    int32_t reserved2;    /* 0 */
    int64_t k_stride_p, k_stride_h, k_stride_l;  /* bytes */
    int64_t v_stride_p, v_stride_h, v_stride_l;  /* bytes */
    int64_t table_stride;                        /* int32 entries between two sequences' rows of the table, >= max_pages */
    int64_t q_stride_t, q_stride_h;              /* elements */
    int64_t o_stride_t, o_stride_h;              /* elements */
} nnop_paged_prefill_fp8_desc; /* 144 bytes: nnop_paged_prefill_desc with kv_format and reserved2 in front of the strides */

/* Host only: the workspace the call needs (0).  The descriptor checks above, in their order. */
int nnop_paged_prefill_fp8_plan(const nnop_paged_prefill_fp8_desc* d, size_t* workspace_bytes_out);

int nnop_paged_prefill_fp8(const nnop_paged_prefill_fp8_desc* d, void* o, float* lse, const void* q, const void* k, const void* v,
                           const float* k_scale, const float* v_scale, const int32_t* block_table, const int32_t* cu_seqlens_q,
                           const int32_t* seqlens, const float* sinks, void* workspace, size_t workspace_bytes, nnop_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NNOP_HIP_PAGED_PREFILL_FP8_H */
