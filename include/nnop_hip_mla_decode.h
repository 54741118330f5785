/*
 * nnop_hip_mla_decode.h -- C ABI of libnnop_hip_mla_decode.so: the attention of a decode step of multi-head latent attention (MLA, as
 * DeepSeek-V2 / V3 / R1 and Kimi-K2 use it) in its weight-absorbed form, over a PAGED LATENT cache.  There is one "KV head": a row of 576
 * values per key -- 512 compressed latent values followed by 64 rotary values -- which is the key (all 576 columns) and the value (the
 * first 512 columns) of every query head.  The cache is a pool of pages of page_size such rows and an int32 block table per sequence, read
 * where they lie; up to 128 query heads attend to it.  float16 / bfloat16.
 *
 * An eighteenth library beside libnnop_hip.so (nnop_hip.h) and the sixteen that nnop_hip_paged_kv_write.h lists with itself, built the
 * same way: an ABI version of its own, nothing linked from the other seventeen, only this header's functions exported.  nnop_dtype,
 * nnop_status and nnop_stream_t come from nnop_hip.h; a status code is turned into text by the main library's nnop_strerror().  gfx950
 * (MI355X) only.  The launch is asynchronous on the caller's stream; nothing is allocated; the workspace is the caller's.
 */
#ifndef NNOP_HIP_MLA_DECODE_H
#define NNOP_HIP_MLA_DECODE_H

#include "nnop_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NNOP_HIP_MLA_DECODE_ABI_VERSION 1
int nnop_mla_decode_abi_version(void);

#define NNOP_MLA_DECODE_WIDTH         576 /* a row of q and of the cache: 512 latent + 64 rotary values */
#define NNOP_MLA_DECODE_LATENT        512 /* a row of o */
#define NNOP_MLA_DECODE_MAX_HEADS     128 /* QH: a multiple of 16 */
#define NNOP_MLA_DECODE_MAX_QL        8
#define NNOP_MLA_DECODE_MAX_SPLITS    64
#define NNOP_MLA_DECODE_MIN_PAGE_SIZE 16  /* a 16-key block of a tile lies in one page */

/*
 * T = `dtype`, B sequences, QH query heads, QL new tokens per sequence, P = num_pages, cap = max_pages page_size.
 *
 *   q            element (b, h, i, e), e < 576, at q + b q_stride_b + h q_stride_h + i q_stride_l + e (strides in elements): the absorbed
 *                query q_nope W_UK (512 values) followed by the rotary part (64); [B][QH][QL][576] and [B][QL][QH][576] are both read
 *                where they lie
 *   kv           the pool: value e of row r of page g at kv + g kv_stride_p + r kv_stride_l + e, of T
 *   block_table  int32 ON THE DEVICE: entry (b, n) at block_table + b table_stride + n, n < max_pages, is the page that holds keys
 *                n page_size ... (n + 1) page_size - 1 of sequence b
 *   seqlens      [B] int32 ON THE DEVICE: the valid keys of each sequence INCLUDING its QL new ones; read on the device, clamped into
 *                [0, cap]
 *   o            [B][QH][QL][512] of T, contiguous;  lse [B][QH][QL] fp32 or NULL
 *
 * Key j of sequence b is the row c_j = row j mod page_size of page block_table[b][j / page_size].  Row (b, h, i) stands at
 * p = seqlens[b] - QL + i and sees keys 0 ... p:
 *   x_j = softmax_scale <q[b,h,i,:576], c_j[:576]>   in fp32
 *   o[b,h,i,:] = sum_j softmax(x)_j c_j[:512]        fp32 accumulation, one rounding to T
 *   lse[b,h,i] = log sum_j exp(x_j)
 * A row that sees no key (p < 0) has o = +0 and lse = -inf.  No window, no sinks.  softmax_scale is the caller's: 192^-1/2 for DeepSeek's
 * 128 + 64 wide heads (not 576^-1/2), another value under YaRN.
 *
 * Contracts:
 *   - The grid comes from host values alone; lengths and the table are read on the device.  No sync, no allocation, no atomics.  A
 *     captured graph follows seqlens, the table and the pages.  Two runs are bitwise equal.
 *   - Masking is by selection: every pool row that no query of its sequence sees may hold anything, NaN included.
 *   - Only live table entries are read: those of the pages that hold a key of [0, seqlens[b]).  A sequence of length 0 reads none.
 *   - A page id forms no address outside the pool: every id read is clamped into [0, num_pages - 1] before it is multiplied by the page
 *     stride, in 64 bits.  A wrong table gives wrong numbers, never an access outside the pool.
 *   - At a fixed resolved split count the bits of sequence b's rows depend on its q, seqlens[b], the visible rows of its own pages and the
 *     host values alone -- not on B, on P, on where its pages lie, or on the other sequences.
 *   - The workspace may hold anything on entry.
 *
 * The split count: every row's keys are cut into `splits` chunks of whole 32-key tiles; a second kernel merges the chunks in ascending
 * order.  The automatic rule, from host values alone:
 *   tiles  = ceil(cap / 32)
 *   groups = batch ql ceil(qh / 64)
 *   splits = min(max(min(ceil(512 / groups), tiles / 4), 1), 64); a forced count (splits >= 1) is used as it is, up to 64
 *   workspace bytes = 0 at one split (no merge runs), else 4 batch qh ql splits (512 + 2).
 *
 * Checks, in this order, all before any device work:
 *   NNOP_ERR_NULL       the descriptor itself is NULL (nnop_mla_decode_plan: or an output pointer)
 *   NNOP_ERR_DTYPE      dtype is not NNOP_F16 or NNOP_BF16
 *   NNOP_ERR_OPTS       flags or a reserved field is not 0; splits < 0 or > 64; softmax_scale not finite or not > 0
 *   NNOP_ERR_SHAPE      batch < 1; ql < 1 or > 8; qh < 16, > 128 or no multiple of 16; page_size below 16 or no power of two; max_pages or
 *                       num_pages < 1; max_pages page_size > 2^31 - 1 or < ql; a stride of q or of the pool below 576 or no multiple of 8
 *                       elements; table_stride < max_pages; batch ql ceil(qh / 64) splits or batch qh ql (the rows of o) > 2^31 - 1
 *   NNOP_ERR_NULL       a NULL pointer; lse and, at a resolved split count of 1, the workspace are the optional ones
 *   NNOP_ERR_ALIGN      q, kv or o not aligned to 16 bytes; block_table, seqlens, lse or the workspace not to 4
 *   NNOP_ERR_WORKSPACE  workspace_bytes below what nnop_mla_decode_plan reports
 */
typedef struct nnop_mla_decode_desc {
    int32_t dtype;        /* nnop_dtype: NNOP_F16 or NNOP_BF16 */
    int32_t ql;           /* new tokens per sequence, 1 ... 8 */
    int32_t qh;           /* query heads: 16, 32, ... 128 */
    int32_t batch;        /* B */
    int32_t max_pages;    /* entries of a sequence's row of the table */
    int32_t page_size;    /* keys of a page: a power of two, 16 or more */
    int32_t num_pages;    /* P: pages of the pool; ids are clamped into [0, P - 1] */
    int32_t splits;       /* 0: automatic; >= 1: forced */
    uint32_t flags;       /* 0 */
    int32_t reserved0, reserved1; /* 0 */
    float softmax_scale;  /* finite, > 0 */
    int64_t q_stride_b, q_stride_h, q_stride_l; /* elements */
    int64_t kv_stride_p, kv_stride_l;           /* elements */
    int64_t table_stride;                       /* int32 entries between two sequences' rows of the table, >= max_pages */
} nnop_mla_decode_desc; /* 96 bytes */

/* Host only: the split count the call will use and the workspace it then needs.  The descriptor checks above, in their order. */
int nnop_mla_decode_plan(const nnop_mla_decode_desc* d, int32_t* splits_out, size_t* workspace_bytes_out);

int nnop_mla_decode(const nnop_mla_decode_desc* d, void* o, float* lse, const void* q, const void* kv, const int32_t* block_table,
                    const int32_t* seqlens, void* workspace, size_t workspace_bytes, nnop_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NNOP_HIP_MLA_DECODE_H */
