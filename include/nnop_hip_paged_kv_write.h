/*
 * nnop_hip_paged_kv_write.h -- C ABI of libnnop_hip_paged_kv_write.so: the WRITE side of the paged KV cache.  The keys and values of the
 * new tokens of a serving step -- packed token-major, as nnop_paged_prefill takes q -- go into the pages that the paged attention calls
 * (nnop_hip_paged_attn.h, nnop_hip_paged_prefill.h, their _fp8 and _split forms) read: a bit-for-bit copy into a 16-bit pool, or one-byte
 * OCP E4M3 codes into an FP8 pool, by the quantisation rule below, which is the project's one statement of how a value becomes a code.
 * One launch writes K and V.  float16 / bfloat16 sources.
 *
 * A seventeenth library beside libnnop_hip.so (nnop_hip.h), libnnop_hip_ext.so, libnnop_hip_moe.so, libnnop_hip_moe_data.so,
 * libnnop_hip_moe_gemm.so, libnnop_hip_moe_linear.so, libnnop_hip_moe_mx.so, libnnop_hip_moe_mx_decode.so,
 * libnnop_hip_moe_mx_decode_glu.so, libnnop_hip_decode_attn.so, libnnop_hip_decode_attn_fp8.so, libnnop_hip_paged_attn.so,
 * libnnop_hip_paged_prefill.so, libnnop_hip_paged_attn_fp8.so, libnnop_hip_paged_prefill_fp8.so and libnnop_hip_paged_prefill_split.so,
 * built the same way: an ABI version of its own, nothing linked from the other sixteen, only this header's functions exported.
 * nnop_dtype, nnop_status and nnop_stream_t come from nnop_hip.h; a status code is turned into text by the main library's
 * nnop_strerror().  gfx950 (MI355X) only.  The launch is asynchronous on the caller's stream; nothing is allocated and there is no
 * workspace.
 */
#ifndef NNOP_HIP_PAGED_KV_WRITE_H
#define NNOP_HIP_PAGED_KV_WRITE_H

#include "nnop_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NNOP_HIP_PAGED_KV_WRITE_ABI_VERSION 1
int nnop_paged_kv_write_abi_version(void);

#ifndef NNOP_PAGED_KV_WRITE_BLOCK_TOKENS      /* a build for tools/perf_paged_kv_write.py's --lib arms sets another multiple of 4 */
#define NNOP_PAGED_KV_WRITE_BLOCK_TOKENS  4   /* consecutive tokens of a workgroup: four waves, one token at a time each -- as measured,
                                                 one token a wave: 8, 16 and 32 were slower or level at every shape */
#endif
#define NNOP_PAGED_KV_WRITE_MIN_PAGE_SIZE 16  /* the reading calls' */
#define NNOP_PAGED_KV_WRITE_16BIT         0   /* kv_format: the pools hold `dtype`; a row is copied bit for bit */
#define NNOP_PAGED_KV_WRITE_E4M3          1   /* kv_format: the pools hold OCP E4M3 codes, torch.float8_e4m3fn */

/*
 * D = `dtype`, T = `tokens` (the new tokens of all sequences), B sequences, KH KV heads, E = emb, P = num_pages,
 * cap = max_pages page_size.
 *
 *   k, v          [T][KH][E] of D, the sources: element (t, h, e) of k lies at k + t k_stride_t + h k_stride_h + e (strides in elements),
 *                 v likewise with its own strides, so the K and V slices of a fused QKV projection [T][(QH + 2 KH) E] are read where
 *                 they lie; the tokens of sequence b are cu_seqlens_q[b] ... cu_seqlens_q[b + 1] - 1
 *   k_pages,      the pools, WRITTEN: element (page, h, r, e) of k_pages lies at k_pages + page kp_stride_p + h kp_stride_h +
 *   v_pages       r kp_stride_l + e, v_pages likewise with its own strides, in pool elements -- elements of D with
 *                 NNOP_PAGED_KV_WRITE_16BIT, bytes with NNOP_PAGED_KV_WRITE_E4M3: [P][KH][page_size][E] and [P][page_size][KH][E] pools
 *                 are both written where they lie.  Both pools have the one format
 *   k_scale,      [KH] fp32 ON THE DEVICE or NULL (= 1), NNOP_PAGED_KV_WRITE_E4M3 only: what nnop_paged_attn_fp8 and
 *   v_scale       nnop_paged_prefill_fp8 multiply a code's value by
 *   block_table   int32 ON THE DEVICE: entry (b, n) at block_table + b table_stride + n, n < max_pages, is the page that holds keys
 *                 n page_size ... (n + 1) page_size - 1 of sequence b; K and V share it
 *   cu_seqlens_q  [B + 1] int32 ON THE DEVICE, non-decreasing, cu[0] = 0; n_b = cu[b + 1] - cu[b].  Read on the device, every entry
 *                 clamped into [0, T] (a decreasing pair gives n_b = 0)
 *   seqlens       [B] int32 ON THE DEVICE: the keys of each sequence INCLUDING its n_b new ones; read on the device, clamped into
 *                 [0, cap]
 *
 * Where a token goes: token i of sequence b stands at p = seqlens[b] - n_b + i, the position at which nnop_paged_prefill places its
 * query.  Its K row and its V row of KV head h go to row p mod page_size of page block_table[b][p / page_size].  A token is SKIPPED --
 * it writes nothing, and nothing of its source rows is read -- when p < 0, which seqlens[b] < n_b brings about, or when its table entry
 * lies outside [0, P): -1 is "a page of another rank", the convention of nnop_moe_permute and nnop_moe_combine.  Unlike the reading
 * calls this one does not clamp a bad id: a clamped write would destroy another sequence's page.  A token that no sequence of
 * cu_seqlens_q owns is skipped too.
 *
 * The quantisation rule (NNOP_PAGED_KV_WRITE_E4M3), stated here once for the project:
 *
 *     code = RNE_to_E4M3( clamp( fp32(x) / scale[h], -448, +448 ) )
 *
 * with a correctly rounded fp32 division, ties to the even code, results below half the smallest subnormal (2^-10) to +-0 with their
 * sign, +-inf and everything beyond +-448 to +-448, and a NaN to a NaN code (0x7F or 0xFF).  It is
 * (x.float() / s).clamp(-448, 448).to(torch.float8_e4m3fn) bit for bit.  Scales are finite, positive, normal floats; with any other
 * scale the codes are unspecified, and the writes still stay inside the rows described above.
 *
 * Contracts: the paged calls', restated for this one.
 *   - The grid comes from host values alone (T, KH, E); cu_seqlens_q, seqlens, the table and the scales are read on the device.  No sync,
 *     no allocation, no workspace, no atomics.  A captured graph follows cu_seqlens_q, seqlens, the table, the source rows and the scales
 *     at fixed T and B.  Two runs are bitwise equal.
 *   - Only the table entries of pages that receive a token are read.  Every address is formed in 64 bits.
 *   - Nothing else in the pools is touched: every byte of every row that receives no token keeps its value, and of a row that receives
 *     one, the E elements of each KV head are written and nothing between them.
 *   - What a sequence's tokens write depends on its source rows, n_b, seqlens[b], its table entries and the scales alone -- not on P, on
 *     where its pages lie, or on the other sequences of the call.
 *   - If the table sends two tokens to the same slot, every aligned 16-byte piece of the slot's rows holds what one of the two tokens
 *     writes there, whole; which of the two is unspecified, piece by piece.
 *
 * Work: a workgroup takes NNOP_PAGED_KV_WRITE_BLOCK_TOKENS consecutive tokens and each of its four waves one token at a time; the grid is
 * ceil(T / NNOP_PAGED_KV_WRITE_BLOCK_TOKENS).  A wave finds its token's sequence by a search over cu_seqlens_q and keeps it, the
 * position, the table entry and the skip decision in scalar registers; its lanes move the rows in 16-byte pieces.
 *
 * Checks, in this order, all before any device work:
 *   NNOP_ERR_NULL       the descriptor itself is NULL
 *   NNOP_ERR_DTYPE      dtype is not NNOP_F16 or NNOP_BF16
 *   NNOP_ERR_OPTS       flags, reserved or reserved2 is not 0; kv_format is neither of the two; k_scale or v_scale is not NULL with
 *                       NNOP_PAGED_KV_WRITE_16BIT
 *   NNOP_ERR_SHAPE      emb not 64 or 128; tokens, batch or kh < 1; kh emb > 2^31 - 1; page_size below 16 or no power of two; max_pages
 *                       or num_pages < 1; max_pages page_size > 2^31 - 1; a pool stride below emb or no multiple of 16 bytes;
 *                       k_stride_h or v_stride_h below emb, k_stride_t or v_stride_t below kh emb, or one of them no multiple of 8
 *                       elements; table_stride < max_pages
 *   NNOP_ERR_NULL       a NULL pointer; k_scale and v_scale are the optional ones
 *   NNOP_ERR_ALIGN      k, v, k_pages or v_pages not aligned to 16 bytes; k_scale, v_scale, block_table, cu_seqlens_q or seqlens not to 4
 */
typedef struct nnop_paged_kv_write_desc {
    int32_t dtype;        /* nnop_dtype of k and v: NNOP_F16 or NNOP_BF16 */
    int32_t emb;          /* E: 64 or 128 */
    int32_t tokens;       /* T */
    int32_t kh;           /* KV heads */
    int32_t batch;        /* B */
    int32_t max_pages;    /* entries of a sequence's row of the table */
    int32_t page_size;    /* keys of a page: a power of two, 16 or more */
    int32_t num_pages;    /* P: pages of the pool; an id outside [0, P) skips its token */
    int32_t kv_format;    /* NNOP_PAGED_KV_WRITE_16BIT or NNOP_PAGED_KV_WRITE_E4M3 */
    int32_t reserved;     /* 0 */
    uint32_t flags;       /* 0 */
    int32_t reserved2;    /* 0 */
    int64_t kp_stride_p, kp_stride_h, kp_stride_l;  /* pool elements: elements of D or bytes */
    int64_t vp_stride_p, vp_stride_h, vp_stride_l;
    int64_t table_stride;                           /* int32 entries between two sequences' rows of the table, >= max_pages */
    int64_t k_stride_t, k_stride_h;                 /* elements of D */
    int64_t v_stride_t, v_stride_h;
} nnop_paged_kv_write_desc; /* 136 bytes */

int nnop_paged_kv_write(const nnop_paged_kv_write_desc* d, void* k_pages, void* v_pages, const void* k, const void* v,
                        const float* k_scale, const float* v_scale, const int32_t* block_table, const int32_t* cu_seqlens_q,
                        const int32_t* seqlens, nnop_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NNOP_HIP_PAGED_KV_WRITE_H */
