/*
 * nnop_hip_paged_attn_fp8.h -- C ABI of libnnop_hip_paged_attn_fp8.so: the attention of a decode step (nnop_hip_decode_attn.h) over a
 * PAGED KV cache of one-byte OCP E4M3 codes.  The cache is a pool of pages of page_size keys each and an int32 block table per
 * sequence (nnop_hip_paged_attn.h), the pages hold codes with one fp32 scale per KV head for K and for V (nnop_hip_decode_attn_fp8.h).
 * The pages are read where they lie and the codes are expanded in registers: no dense copy of a sequence's keys is gathered per step
 * and no 16-bit copy of the pool is kept.  The arithmetic, rows, split rule, merge order and every result bit are
 * nnop_decode_attn_fp8's.
 *
 * A fourteenth library beside libnnop_hip.so (nnop_hip.h), libnnop_hip_ext.so, libnnop_hip_moe.so, libnnop_hip_moe_data.so,
 * libnnop_hip_moe_gemm.so, libnnop_hip_moe_linear.so, libnnop_hip_moe_mx.so, libnnop_hip_moe_mx_decode.so,
 * libnnop_hip_moe_mx_decode_glu.so, libnnop_hip_decode_attn.so, libnnop_hip_decode_attn_fp8.so, libnnop_hip_paged_attn.so and
 * libnnop_hip_paged_prefill.so, built the same way as the twelfth: an ABI version of its own, nothing linked from the other thirteen,
 * only this header's functions exported.  nnop_dtype, nnop_status and nnop_stream_t come from nnop_hip.h; a status code is turned into
 * text by the main library's nnop_strerror().  gfx950 (MI355X) only.  The launch is asynchronous on the caller's stream; nothing is
 * allocated; the workspace is the caller's.
 */
#ifndef NNOP_HIP_PAGED_ATTN_FP8_H
#define NNOP_HIP_PAGED_ATTN_FP8_H

#include "nnop_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NNOP_HIP_PAGED_ATTN_FP8_ABI_VERSION 1
int nnop_paged_attn_fp8_abi_version(void);

#define NNOP_PAGED_ATTN_FP8_MAX_ROWS      16 /* G QL, the rows of one 16-wide matrix operand */
#define NNOP_PAGED_ATTN_FP8_MAX_SPLITS    64
#define NNOP_PAGED_ATTN_FP8_MIN_PAGE_SIZE 16 /* a 16-key block of a tile lies in one page */
#define NNOP_PAGED_ATTN_FP8_E4M3          0  /* kv_format: OCP E4M3, torch.float8_e4m3fn */

/*
 * T = `dtype`, B sequences, QH query heads, KH KV heads, G = QH / KH, E = emb, P = num_pages, cap = max_pages page_size.
 *
 *   q            [B][QH][QL][E] of T, contiguous
 *   k, v         the pools, bytes: the code of element (page, kvh, r, e) of k lies at k + page k_stride_p + kvh k_stride_h +
 *                r k_stride_l + e (an element is a byte, so the strides are bytes), v likewise with its own strides:
 *                [P][KH][page_size][E] and [P][page_size][KH][E] pools are both read where they lie
 *   k_scale      [KH] fp32 ON THE DEVICE or NULL (= 1): the value of a K element is its code's value times k_scale[kvh]
 *   v_scale      [KH] fp32 ON THE DEVICE or NULL (= 1): likewise for V
 *   block_table  int32 ON THE DEVICE: entry (b, n) at block_table + b table_stride + n, n < max_pages, is the page that holds keys
 *                n page_size ... (n + 1) page_size - 1 of sequence b; K and V share it
 *   seqlens      [B] int32 ON THE DEVICE: the valid keys of each sequence INCLUDING its QL new ones; read on the device, clamped into
 *                [0, cap]
 *   sinks        [QH] fp32 or NULL;  o [B][QH][QL][E] of T;  lse [B][QH][QL] fp32 or NULL
 *
 * Key j of sequence b is row j mod page_size of page block_table[b][j / page_size].  With that, everything is nnop_decode_attn_fp8's,
 * word for word: the rule of what a query sees (bottom-right alignment, window_left, a window_left >= cap taken as no window), the one
 * factor k_scale[kvh] / sqrt(E) on the fp32 scores, v_scale[kvh] on the fp32 o after the division and in front of its one rounding,
 * sinks and lse in the domain of the scaled scores, the dead rows (o = +0, lse = the sink or -inf), a NaN code in a visible row giving
 * NaN.
 *
 * Contracts: nnop_decode_attn_fp8's (device-side lengths and a grid from host values alone; no sync, no allocation, no atomics; two
 * runs bitwise equal; masking by selection, the V rows no query sees replaced by zero bytes; the exact conversion of a code to T, both
 * products on T with fp32 accumulation, one rounding of o), and four more:
 *   1. Same bits as the dense call: at the same resolved split count, o and lse equal bit for bit what nnop_decode_attn_fp8 gives on
 *      the same codes gathered into a dense cache of capacity cap.  Paging changes addresses, not arithmetic.
 *   2. Only live table entries are read: the entries of the pages that hold a key of [lo, hi), hi = seqlens[b], lo = 0 or
 *      max(0, hi - QL - window_left).  Entries in front of the window or behind seqlens[b] may hold anything; a sequence of length 0
 *      reads none.  Within a live page, rows outside [lo, hi) are never loaded.  Every id read is clamped into [0, num_pages - 1]
 *      before it is multiplied by a page stride, in 64 bits: a wrong table gives wrong numbers, never an access outside the pool.
 *   3. Batch independence covers the pool: the bits of sequence b's rows depend on its q, seqlens[b], the visible rows of its own
 *      pages, the scales and the host values (QL, E, G, window_left, the resolved split count) alone -- not on P, on where its pages
 *      lie in the pool, on page_size, or on the other sequences and their pages.
 *   4. A call captured in a graph follows seqlens, the table, the pages and the scales: all four are read on the device at replay.
 *
 * The automatic split count and the workspace are nnop_decode_attn's with capacity = max_pages page_size:
 *   tiles  = ceil(cap / 32); with a window: min(that, (ql + window_left) / 32 + 2)
 *   splits = min(max(min(ceil(512 / (batch kh)), tiles / 4), 1), 64); a forced count (splits >= 1) is used as it is, up to 64
 *   workspace bytes = 0 at one split, else 4 batch qh ql splits (emb + 2).
 *
 * Checks, in this order, all before any device work:
 *   NNOP_ERR_NULL       the descriptor itself is NULL (nnop_paged_attn_fp8_plan: or an output pointer)
 *   NNOP_ERR_DTYPE      dtype is not NNOP_F16 or NNOP_BF16
 *   NNOP_ERR_OPTS       flags is not 0, kv_format is not NNOP_PAGED_ATTN_FP8_E4M3, or reserved is not 0; window_left < -1; splits < 0
 *                       or > 64
 *   NNOP_ERR_SHAPE      emb not 64 or 128; batch, qh or kh < 1; qh no multiple of kh; ql < 1; (qh / kh) ql > 16; page_size below 16 or no
 *                       power of two; max_pages or num_pages < 1; max_pages page_size > 2^31 - 1 or < ql; a K or V stride below emb or
 *                       no multiple of 16 bytes; the rows of a page not within 2^32 bytes, (page_size - 1) stride_l + emb > 2^32 - 1
 *                       (the page offsets are 64 bits, a row's offset inside its page is 32); table_stride < max_pages; batch kh splits
 *                       or batch qh ql (the rows of o) > 2^31 - 1
 *   NNOP_ERR_NULL       a NULL pointer; lse, k_scale, v_scale, sinks and, at a resolved split count of 1, the workspace are the
 *                       optional ones
 *   NNOP_ERR_ALIGN      q, k, v or o not aligned to 16 bytes; k_scale, v_scale, block_table, seqlens, sinks, lse or the workspace not
 *                       to 4
 *   NNOP_ERR_WORKSPACE  workspace_bytes below what nnop_paged_attn_fp8_plan reports
 */
typedef struct nnop_paged_attn_fp8_desc {
    int32_t dtype;        /* nnop_dtype of q and o: NNOP_F16 or NNOP_BF16 */
    int32_t emb;          /* E: 64 or 128 */
    int32_t ql;           /* new tokens per sequence */
    int32_t qh;           /* query heads */
    int32_t kh;           /* KV heads */
    int32_t batch;        /* B */
    int32_t max_pages;    /* entries of a sequence's row of the table */
    int32_t window_left;  /* -1: none */
    int32_t splits;       /* 0: automatic; >= 1: forced */
    uint32_t flags;       /* 0 */
    int32_t page_size;    /* keys of a page: a power of two, 16 or more */
    int32_t num_pages;    /* P: pages of the pool; ids are clamped into [0, P - 1] */
    int32_t kv_format;    /* NNOP_PAGED_ATTN_FP8_E4M3 */
    int32_t reserved;     /* 0 */
    int64_t k_stride_p, k_stride_h, k_stride_l;  /* bytes */
    int64_t v_stride_p, v_stride_h, v_stride_l;  /* bytes */
    int64_t table_stride;                        /* int32 entries between two sequences' rows of the table, >= max_pages */
} nnop_paged_attn_fp8_desc; /* 112 bytes: nnop_paged_attn_desc with kv_format and reserved in front of the strides */

/* Host only: the split count the call will use and the workspace it then needs.  The descriptor checks above, in their order. */
int nnop_paged_attn_fp8_plan(const nnop_paged_attn_fp8_desc* d, int32_t* splits_out, size_t* workspace_bytes_out);

int nnop_paged_attn_fp8(const nnop_paged_attn_fp8_desc* d, void* o, float* lse, const void* q, const void* k, const void* v,
                        const float* k_scale, const float* v_scale, const int32_t* block_table, const int32_t* seqlens,
                        const float* sinks, void* workspace, size_t workspace_bytes, nnop_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NNOP_HIP_PAGED_ATTN_FP8_H */
