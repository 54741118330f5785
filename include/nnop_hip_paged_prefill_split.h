/*
 * nnop_hip_paged_prefill_split.h -- C ABI of libnnop_hip_paged_prefill_split.so: nnop_hip_paged_prefill.h's attention of a PREFILL step
 * over a paged KV cache with the KEY AXIS CUT (split-KV), for few new tokens behind a long context -- a chunk of a chunked prefill behind
 * 32K-128K keys, a short follow-up turn behind a long cached prefix, speculative verification of more than 16 rows per sequence at a
 * moderate batch -- where that call's KH (T / TB + B) workgroups, each walking a whole key range alone, do not fill the chip.
 * float16 / bfloat16 queries and pages, forward only.  (Pages of E4M3 codes are not served here: nnop_hip_paged_prefill_fp8.h has no
 * split form yet.)
 *
 * A sixteenth library beside libnnop_hip.so (nnop_hip.h) and the fourteen that nnop_hip_paged_prefill_fp8.h lists, built the same way
 * as the thirteenth: an ABI version of its own, nothing linked from the other fifteen, only this header's functions exported.  The
 * descriptor is the thirteenth library's, nnop_paged_prefill_desc, with `reserved` read as the split count.  nnop_dtype, nnop_status and
 * nnop_stream_t come from nnop_hip.h; a status code is turned into text by the main library's nnop_strerror().  gfx950 (MI355X) only.
 * The launches are asynchronous on the caller's stream; nothing is allocated.
 */
#ifndef NNOP_HIP_PAGED_PREFILL_SPLIT_H
#define NNOP_HIP_PAGED_PREFILL_SPLIT_H

#include "nnop_hip_paged_prefill.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NNOP_HIP_PAGED_PREFILL_SPLIT_ABI_VERSION 1
int nnop_paged_prefill_split_abi_version(void);

#define NNOP_PAGED_PREFILL_SPLIT_MAX_SPLITS      64 /* chunks of a block's key range, as in nnop_hip_decode_attn.h */
#define NNOP_PAGED_PREFILL_SPLIT_MIN_CHUNK_TILES 8  /* 32-key tiles a chunk of the automatic rule holds at least */

/*
 * Arguments, restated from nnop_hip_paged_prefill.h.  D = `dtype`, T = `tokens` (the new tokens of all sequences), B sequences, QH query
 * heads, KH KV heads, G = QH / KH, E = emb, P = num_pages, cap = max_pages page_size, TB = 128 / G.
 *
 *   q, o          [T][QH][E] of D: element (t, h, e) of q lies at q + t q_stride_t + h q_stride_h + e (strides in elements), o likewise
 *                 with its own strides; the tokens of sequence b are cu_seqlens_q[b] ... cu_seqlens_q[b + 1] - 1
 *   k, v          nnop_paged_attn's pools of D, with their three strides each; block_table as there
 *   cu_seqlens_q  [B + 1] int32 ON THE DEVICE, non-decreasing, cu[0] = 0; n_b = cu[b + 1] - cu[b].  Read on the device, every entry
 *                 clamped into [0, T] (a decreasing pair gives n_b = 0)
 *   seqlens       [B] int32 ON THE DEVICE: the valid keys of each sequence INCLUDING its n_b new ones; read on the device, clamped into
 *                 [0, cap]
 *   sinks         [QH] fp32 or NULL;  lse [T][QH] fp32, contiguous, or NULL
 *   reserved      the split count: 0 for the automatic rule below, 1 ... 64 to force it
 *   workspace     fp32, 16-byte aligned, nnop_paged_prefill_split_plan's bytes; may hold anything on entry, NaN included
 *
 * What a query sees is nnop_paged_prefill's rule: query i of sequence b stands at p = seqlens[b] - n_b + i and sees keys
 * max(0, p - window_left) ... p (0 ... p without a window; a window_left >= cap is no window); key j is row j mod page_size of page
 * block_table[b][j / page_size]; the scale is 1 / sqrt(E); a sink is one more column of the softmax; a row that sees no key -- p < 0
 * included -- has o = +0 and lse = its sink, or -inf without one.  Never NaN.
 *
 * Work.  A row block is nnop_paged_prefill's: (sequence b, KV head, TB tokens of b), found by the same search over cu_seqlens_q.  Its
 * key tiles of 32 are t_lo ... t_hi, computed on the device as there.  With n = t_hi - t_lo + 1 and per = ceil(n / splits), chunk c takes
 * tiles t_lo + c per ... min(t_lo + (c + 1) per - 1, t_hi); the grid is KH (T / TB + B) splits, from host values alone.  A (block, chunk)
 * without a tile reads no table entry and no page and makes no product.  Pass 1 writes, for every live row and chunk, the fp32
 * un-normalised O (E values) and (m, l) of the base-2 softmax -- (-inf, 0) where the row saw no key in the chunk -- into the workspace:
 * O as [splits][T][QH][E], (m, l) as [splits][T][QH][2] behind all of O.  Pass 2, a wave per (token, head) row of the tokens in front
 * of cu_seqlens_q[B], takes M = max(m_c, sink log2 e), sums l_c 2^(m_c - M) and O_c 2^(m_c - M) over the chunks with l_c > 0 in
 * ascending c in fp32 -- a chunk with l_c = 0 is selected out, its O never read -- adds the sink's column, divides, rounds once and stores
 * o and lse.  Every slot pass 2 reads was written by pass 1 of the same call.
 *
 * The split count.  With `reserved` = 0: groups = KH (T / TB + B); splits = ceil(512 / groups), two resident workgroups on each of 256
 * compute units; at most tiles / 8 (NNOP_PAGED_PREFILL_SPLIT_MIN_CHUNK_TILES), tiles = ceil(cap / 32) or, with a window,
 * min(that, (TB + window_left) / 32 + 2); clamped into 1 ... 64.  So groups >= 512 gives 1.  workspace_bytes =
 * 4 T QH splits (E + 2) for more than one split and 0 for one.  At a resolved count of 1 no merge runs, the workspace is not touched
 * and may be NULL, and o and lse are nnop_paged_prefill's bit for bit.
 *
 * Contracts: nnop_paged_prefill's, restated, with the resolved split count added to what the bits depend on.
 *   - The grid, the split count and the workspace size come from host values alone (T, B, QH, KH, E, cap, window_left, reserved);
 *     cu_seqlens_q, seqlens and the table are read on the device.  No sync, no allocation, no atomics; the merge order is fixed.  A
 *     captured graph follows cu_seqlens_q, seqlens, the table and the pages at fixed T, B and split count.  Two runs are bitwise equal.
 *   - Masking is by selection: a pool row that no query of its sequence sees may hold NaN, and so may the whole workspace on entry.
 *   - Only live table entries are read: those of the pages that hold a key of [lo, hi), hi = seqlens[b], lo = 0 or
 *     max(0, hi - n_b - window_left).  Within a live page, rows outside [lo, hi) are never loaded.
 *   - A page id forms no address outside the pool: every id read is clamped into [0, num_pages - 1] before it is multiplied by a page
 *     stride, in 64 bits.
 *   - Batch independence: the bits of a sequence's rows depend on its q, n_b, seqlens[b], the visible rows of its own pages, the host
 *     values (E, G, window_left) and the resolved split count alone -- not on P, on where its pages lie, on page_size, or on the other
 *     sequences of the call: the chunk boundaries of a block follow from the sequence's own values and that count.  (The AUTOMATIC
 *     count depends on T and B: fix the count to compare calls of different batches.)
 *   - fp32 scores, softmax, partial results and merge, one rounding of o.
 *
 * Checks, in this order, all before any device work:
 *   NNOP_ERR_NULL       the descriptor itself is NULL (nnop_paged_prefill_split_plan: or an output pointer)
 *   NNOP_ERR_DTYPE      dtype is not NNOP_F16 or NNOP_BF16
 *   NNOP_ERR_OPTS       flags is not 0; reserved (the split count) outside 0 ... 64; window_left < -1
 *   NNOP_ERR_SHAPE      emb not 64 or 128; tokens, batch, qh or kh < 1; qh no multiple of kh; qh / kh > 16; page_size below 16 or no
 *                       power of two; max_pages or num_pages < 1; max_pages page_size > 2^31 - 1; a K or V stride below emb or no
 *                       multiple of 8 elements; q_stride_h or o_stride_h below emb, q_stride_t or o_stride_t below qh emb, or one of
 *                       them no multiple of 8; table_stride < max_pages; kh (tokens / TB + batch) splits (the resolved count) or
 *                       tokens qh > 2^31 - 1
 *   NNOP_ERR_NULL       a NULL pointer; lse and sinks are optional, and so is the workspace at a resolved count of 1
 *   NNOP_ERR_ALIGN      q, k, v or o not aligned to 16 bytes; block_table, cu_seqlens_q, seqlens, sinks or lse not to 4; the workspace
 *                       not to 16
 *   NNOP_ERR_WORKSPACE  workspace_bytes below what nnop_paged_prefill_split_plan reports
 */

/* Host only: the split count the call will use and the workspace it needs.  The descriptor checks above, in their order. */
int nnop_paged_prefill_split_plan(const nnop_paged_prefill_desc* d, int32_t* splits_out, size_t* workspace_bytes_out);

int nnop_paged_prefill_split(const nnop_paged_prefill_desc* d, void* o, float* lse, const void* q, const void* k, const void* v,
                             const int32_t* block_table, const int32_t* cu_seqlens_q, const int32_t* seqlens, const float* sinks,
                             void* workspace, size_t workspace_bytes, nnop_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NNOP_HIP_PAGED_PREFILL_SPLIT_H */
