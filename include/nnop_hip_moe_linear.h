/*
 * nnop_hip_moe_linear.h -- C ABI of libnnop_hip_moe_linear.so: the expert linear layers of a mixture-of-experts layer as a checkpoint
 * ships them -- the grouped GEMM of nnop_hip_moe_gemm.h with a per-expert bias, weights in either [E][N][K] or [E][K][N] order, and
 * weight and bias gradients that can be accumulated, in fp32 beside 16-bit operands.  It runs where nnop_moe_gemm runs:
 * router -> plan -> permute -> linear -> glu -> linear -> combine.
 *
 * A sixth library beside libnnop_hip.so (nnop_hip.h), libnnop_hip_ext.so (nnop_hip_ext.h), libnnop_hip_moe.so (nnop_hip_moe.h),
 * libnnop_hip_moe_data.so (nnop_hip_moe_data.h) and libnnop_hip_moe_gemm.so (nnop_hip_moe_gemm.h), built the same way as the fifth: an ABI
 * version of its own, nothing linked from the other five, only this header's functions exported.  The boundary of the fifth library is
 * frozen (its two reserved words stay 0), which is why this one exists.  nnop_dtype, nnop_status and nnop_stream_t come from nnop_hip.h;
 * a status code is turned into text by the main library's nnop_strerror().  gfx950 (MI355X) only.  Launches are asynchronous on the
 * caller's stream; nothing is allocated and there is no workspace.
 */
#ifndef NNOP_HIP_MOE_LINEAR_H
#define NNOP_HIP_MOE_LINEAR_H

#include "nnop_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NNOP_HIP_MOE_LINEAR_ABI_VERSION 1
int nnop_moe_linear_abi_version(void);

/* flags of nnop_moe_linear_desc */
#define NNOP_MOE_LINEAR_KN 1u         /* w, dw are [E][K][ld] with the N outputs contiguous; without it [E][N][ld] with the K inputs contiguous */
#define NNOP_MOE_LINEAR_ACCUMULATE 2u /* nnop_moe_linear_bwd_w and _bwd_b add to what dw / db hold */

/*
 * S slot rows (the plan's T k), E experts, K input and N output features.  W_e(n, c) is the coefficient of input c in output n of
 * expert e, wherever the layout puts it.
 *
 *   offsets [E+1] int32                 as nnop_moe_plan writes it: expert e owns the slot rows offsets[e] ... offsets[e+1]-1
 *   xs, dxs [S][ld_x] of `dtype`        slot (expert-sorted) order, K columns
 *   ys, dys [S][ld_y] of `dtype`        slot order, N columns
 *   w       of `dtype`                  without NNOP_MOE_LINEAR_KN: [E][N][ld_w], W_e(n, c) = w[e][n][c], ld_w >= K (stacked nn.Linear)
 *                                       with it:                    [E][K][ld_w], W_e(n, c) = w[e][c][n], ld_w >= N (x @ W checkpoints)
 *                                       experts lie N ld_w / K ld_w elements apart
 *   dw      of `grad_dtype`             the layout of w with ld_dw in the place of ld_w
 *   bias    [E][ld_b] of `dtype`        N columns; NULL: no bias
 *   db      [E][ld_db] of `grad_dtype`  N columns
 * grad_dtype is dtype, or NNOP_F32 beside a 16-bit dtype (an fp32 main gradient).  Columns behind the K / N of an array are padding:
 * neither read nor written.
 *
 * With every offset clamped into [0, S], lo_e = offsets[e], hi_e = offsets[e+1], and an empty range where hi_e <= lo_e:
 *
 *   nnop_moe_linear        ys[s][n]  = sum_c xs[s][c] W_e(n, c) + bias[e][n]     lo_e <= s < hi_e;  every other row of ys: +0 in columns
 *                                                                                < N, and no bias
 *   nnop_moe_linear_bwd_x  dxs[s][c] = sum_n dys[s][n] W_e(n, c)                 lo_e <= s < hi_e;  every other row of dxs: +0
 *   nnop_moe_linear_bwd_w  dW_e(n, c) = sum_{s in [lo_e, hi_e)} dys[s][n] xs[s][c]     stored where the layout puts W_e(n, c)
 *   nnop_moe_linear_bwd_b  db[e][n]   = sum_{s in [lo_e, hi_e)} dys[s][n]
 *
 *   Without NNOP_MOE_LINEAR_ACCUMULATE the two gradients are stored, and an expert without rows gets +0 everywhere.  With it
 *   new = round_to_grad_dtype(float(old) + the fp32 sum), and dw[e], db[e] of an expert without rows are neither read nor written.
 *
 * Contracts (those of nnop_hip_moe_gemm.h carry over):
 *   - offsets is read on the device.  There is no device-to-host copy, no sync and no allocation: the four calls can be captured in a
 *     graph.  Grids are sized on the host from S, E, K, N alone; surplus workgroups leave.
 *   - Nothing is read or written out of bounds whatever offsets holds: every loop bound on the device is a descriptor field or a clamped
 *     offset.  With offsets that are not non-decreasing a row may be written twice, by the wrong expert or not at all.  With the plan's
 *     offsets every output element in range is written exactly once: a caller never pre-zeroes.
 *   - Masking is by selection: rows outside an expert's range, and the bias of another expert, never enter a result that is kept,
 *     whatever they hold, NaN and Inf included.  The rows behind offsets[E] are not read at all.
 *   - Sums are fp32: on the matrix cores for the three products, on the vector units for db.  The bias is added in fp32 to the fp32
 *     accumulator; there is one rounding, on the store.  There are no atomics and no split over a reduction axis between workgroups, so
 *     two runs are bitwise equal.  The order of the db sum depends on N and the element type alone: the rows of an expert are dealt to
 *     the row lanes of one workgroup in turn, each lane adds its rows in ascending order, the lanes' sums are added in ascending order.
 *   - Without a bias, without either flag and with grad_dtype = dtype the three products are those of nnop_hip_moe_gemm.h bit for bit.
 *     With NNOP_MOE_LINEAR_KN, ys and dxs equal those of the transposed weights without it bit for bit.
 *   - Not in place: the inputs and outputs of one call do not overlap (dw and db are read only under NNOP_MOE_LINEAR_ACCUMULATE).
 *     This is not checked.
 *
 * The fast path of a call is taken where K, N and every row stride the call uses are multiples of 8 elements and every base it uses is
 * 16-byte aligned (nnop_moe_linear_bwd_b: N, ld_y and dys): global accesses are then 8 or 16 bytes wide.  Everything else takes an
 * element-wise path of the same structure.  Row offsets are computed in 64 bits.
 *
 * Checks, in this order, all before any device work, the same for the four calls (every field is judged by every call):
 *   NNOP_ERR_NULL    the descriptor itself is NULL (first of all)
 *   NNOP_ERR_DTYPE   dtype is unknown; grad_dtype is neither dtype nor NNOP_F32
 *   NNOP_ERR_OPTS    a flag bit other than the two above is set, or a reserved field is not 0
 *   NNOP_ERR_SHAPE   S < 1, E outside 1 ... 1024, K or N outside 1 ... 65536, ld_x < K, ld_y < N, ld_w or ld_dw below K (N with
 *                    NNOP_MOE_LINEAR_KN), ld_b < N, ld_db < N, or more than 2^31 - 1 output tiles of 128 x 128
 *   NNOP_ERR_NULL    a NULL pointer; bias is the only optional one
 *   NNOP_ERR_ALIGN   an array not aligned to its element size (dw, db: that of grad_dtype), offsets not aligned to 4 bytes
 */
typedef struct nnop_moe_linear_desc {
    int32_t dtype;        /* nnop_dtype of the rows, the weights and the bias */
    int32_t grad_dtype;   /* nnop_dtype of dw and db: dtype, or NNOP_F32 */
    int32_t rows;         /* S */
    int32_t experts;      /* E */
    int32_t in_dim;       /* K */
    int32_t out_dim;      /* N */
    int32_t ld_x;         /* row stride of xs, dxs in elements */
    int32_t ld_y;         /* row stride of ys, dys in elements */
    int32_t ld_w;         /* row stride of a weight row in elements */
    int32_t ld_dw;        /* row stride of a weight-gradient row in elements of grad_dtype */
    int32_t ld_b;         /* row stride of bias in elements */
    int32_t ld_db;        /* row stride of db in elements of grad_dtype */
    uint32_t flags;       /* NNOP_MOE_LINEAR_KN | NNOP_MOE_LINEAR_ACCUMULATE */
    int32_t reserved[3];  /* 0 */
} nnop_moe_linear_desc;   /* 64 bytes */

int nnop_moe_linear(const nnop_moe_linear_desc* d, void* ys, const void* xs, const void* w, const void* bias, const int32_t* offsets,
                    nnop_stream_t stream);
int nnop_moe_linear_bwd_x(const nnop_moe_linear_desc* d, void* dxs, const void* dys, const void* w, const int32_t* offsets,
                          nnop_stream_t stream);
int nnop_moe_linear_bwd_w(const nnop_moe_linear_desc* d, void* dw, const void* dys, const void* xs, const int32_t* offsets,
                          nnop_stream_t stream);
int nnop_moe_linear_bwd_b(const nnop_moe_linear_desc* d, void* db, const void* dys, const int32_t* offsets, nnop_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NNOP_HIP_MOE_LINEAR_H */
