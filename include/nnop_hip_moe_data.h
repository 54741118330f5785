/*
 * nnop_hip_moe_data.h -- C ABI of libnnop_hip_moe_data.so: the data movement of a mixture-of-experts layer, the token permute in front
 * of the expert GEMMs and the weighted combine behind them, each with its pullback.  They consume the plan of nnop_moe_plan
 * (nnop_hip_moe.h); the expert GEMMs between them (a grouped GEMM over the plan's offsets) are the fifth library's, nnop_hip_moe_gemm.h.
 *
 * A fourth library beside libnnop_hip.so (nnop_hip.h), libnnop_hip_ext.so (nnop_hip_ext.h) and libnnop_hip_moe.so (nnop_hip_moe.h),
 * built the same way as the second and third: an ABI version of its own, nothing linked from the other three, only this header's
 * functions exported.  nnop_dtype, nnop_status and nnop_stream_t come from nnop_hip.h; a status code is turned into text by the main
 * library's nnop_strerror().  gfx950 (MI355X) only.  Launches are asynchronous on the caller's stream; nothing is allocated and there
 * is no workspace.
 */
#ifndef NNOP_HIP_MOE_DATA_H
#define NNOP_HIP_MOE_DATA_H

#include "nnop_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NNOP_HIP_MOE_DATA_ABI_VERSION 1
int nnop_moe_data_abi_version(void);

/*
 * T tokens, k assignments per token, rows of D elements, S = T k slot rows.
 *
 *   perm [S] int32, slot [T][k] int32     the arrays of nnop_moe_plan: perm[s] = the flat id t k + j in slot s, slot its inverse
 *   x, dx, y, dy   [T][ld_tok]  of `dtype`    token order
 *   xs, dxs, ys, dys [S][ld_slot] of `dtype`  slot (expert-sorted) order
 *   w, dw [T][k] fp32                     as the gate produces them
 * Columns D ... ld-1 of a row array are padding: neither read nor written.
 *
 * An entry v of perm or slot is VALID iff (uint32_t)v < S; everything else (-1, whatever else the arrays might hold) is SKIPPED.
 * Nothing is read or written out of bounds whatever perm and slot contain.
 *
 *   nnop_moe_permute      xs[s]  = x[perm[s] / k]                        valid perm[s];  else a row of +0
 *   nnop_moe_permute_bwd  dx[t]  = sum_j dxs[slot[t][j]]                 over valid j;   none valid: +0
 *   nnop_moe_combine      y[t]   = sum_j w[t][j] ys[slot[t][j]]          over valid j;   none valid: +0
 *   nnop_moe_combine_bwd  dys[s] = w.flat[perm[s]] dy[perm[s] / k]       valid perm[s];  else a row of +0
 *                         dw[t][j] = sum_c dy[t][c] ys[slot[t][j]][c]    valid slot;     else +0
 *
 * Contracts:
 *   - Every element of every output row in columns < D is written exactly once per call, the rows of skipped slots included: a caller
 *     never pre-zeroes anything, and a grouped GEMM over the tail of xs reads zeros.  (nnop_moe_combine_bwd writes the rows of dys with
 *     a valid perm[s] through slot and the others through perm; "exactly once" there rests on slot being the inverse of perm, as the
 *     plan makes them.  With anything else a row may be written twice or not at all; nothing is written out of bounds.)
 *   - Permute is a copy: the rows of xs are the rows of x bit for bit.
 *   - Sums over j are accumulated in fp32 in the order j = 0 ... k-1 and rounded to `dtype` once, on the store.  nnop_moe_permute_bwd
 *     is the sum of nnop_moe_combine with every weight 1, by the same kernel.
 *   - dw is accumulated in fp32 over the row, without atomics, in an order that depends on the descriptor and on whether the arrays
 *     allow 16-byte accesses (below), on nothing else: two runs are bitwise equal.
 *   - A token may name one expert twice: nothing here requires distinct slots per token.
 *   - Not in place: the inputs and outputs of one call do not overlap.  This is not checked.
 *
 * Rows move in 16-byte pieces where D, ld_tok and ld_slot are multiples of 16 / sizeof(dtype) and every row array's base is 16-byte
 * aligned; everything else takes an element-wise path of the same structure.  Row offsets are computed in 64 bits.
 *
 * Checks, in this order, all before any device work, the same for the four calls:
 *   NNOP_ERR_NULL    the descriptor itself is NULL (first of all)
 *   NNOP_ERR_DTYPE   dtype is unknown
 *   NNOP_ERR_OPTS    a reserved field is not 0
 *   NNOP_ERR_SHAPE   T < 1, k outside 1 ... 64, D outside 1 ... 65536, ld_tok < D, ld_slot < D, or T k > 2^31 - 1
 *   NNOP_ERR_NULL    a NULL pointer: none is optional
 *   NNOP_ERR_ALIGN   a row array not aligned to the element size, an fp32 or int32 array not aligned to 4 bytes
 */
typedef struct nnop_moe_rows_desc {
    int32_t dtype;        /* nnop_dtype of the row arrays */
    int32_t tokens;       /* T */
    int32_t topk;         /* k */
    int32_t dim;          /* D */
    int32_t ld_tok;       /* row stride of x, dx, y, dy in elements */
    int32_t ld_slot;      /* row stride of xs, dxs, ys, dys in elements */
    int32_t reserved[2];  /* 0: kept for a row count below T k (capacity) and for a slot-order scale */
} nnop_moe_rows_desc;     /* 32 bytes */

int nnop_moe_permute(const nnop_moe_rows_desc* d, void* xs, const void* x, const int32_t* perm, nnop_stream_t stream);
int nnop_moe_permute_bwd(const nnop_moe_rows_desc* d, void* dx, const void* dxs, const int32_t* slot, nnop_stream_t stream);
int nnop_moe_combine(const nnop_moe_rows_desc* d, void* y, const void* ys, const float* w, const int32_t* slot, nnop_stream_t stream);
int nnop_moe_combine_bwd(const nnop_moe_rows_desc* d, void* dys, float* dw, const void* dy, const void* ys, const float* w,
                         const int32_t* perm, const int32_t* slot, nnop_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NNOP_HIP_MOE_DATA_H */
