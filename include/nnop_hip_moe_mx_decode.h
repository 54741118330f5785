/*
 * nnop_hip_moe_mx_decode.h -- C ABI of libnnop_hip_moe_mx_decode.so: the forward of the expert linear layer on MXFP4 weights
 * (nnop_moe_mx_linear of nnop_hip_moe_mx.h) made for few rows per expert, the sizes of a decode step.  It takes that call's inputs and
 * gives that call's result under the contracts below; what differs is the kernel: the packed weights are streamed once from memory into
 * the registers that feed the matrix cores, many loads in flight per wave, where the 128 x 128 tile of the seventh library waits for one
 * trip to memory per reduction step.  There is no pullback here: the gradients are nnop_moe_mx_linear_bwd_x of the seventh library and
 * nnop_moe_linear_bwd_b of the sixth.
 *
 * An eighth library beside libnnop_hip.so (nnop_hip.h), libnnop_hip_ext.so, libnnop_hip_moe.so, libnnop_hip_moe_data.so,
 * libnnop_hip_moe_gemm.so, libnnop_hip_moe_linear.so and libnnop_hip_moe_mx.so, built the same way as the seventh: an ABI version of its
 * own, nothing linked from the other seven, only this header's functions exported.  nnop_dtype, nnop_status and nnop_stream_t come from
 * nnop_hip.h; a status code is turned into text by the main library's nnop_strerror().  gfx950 (MI355X) only.  The launch is asynchronous
 * on the caller's stream; nothing is allocated and there is no workspace.
 *
 * The format is that of nnop_hip_moe_mx.h (OCP Microscaling Formats v1.0, MXFP4): 32 values share a scale byte e (2^(e - 127); 255: NaN)
 * and are 4-bit E2M1 codes, 16 bytes per block, element 2j in the low nibble of byte j.
 */
#ifndef NNOP_HIP_MOE_MX_DECODE_H
#define NNOP_HIP_MOE_MX_DECODE_H

#include "nnop_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NNOP_HIP_MOE_MX_DECODE_ABI_VERSION 1
int nnop_moe_mx_decode_abi_version(void);

/*
 * S slot rows, E experts, K input and N output features.  W_e(n, c) is the value nnop_mxfp4_dequant gives for element c of weight row n
 * of expert e, in `dtype`.
 *
 *   offsets [E+1] int32              as nnop_moe_plan writes it
 *   xs      [S][ld_x] of `dtype`     slot order, K columns
 *   ys      [S][ld_y] of `dtype`     slot order, N columns
 *   blocks  [E][N][ld_q] uint8       K / 2 bytes of a row are read; experts lie N ld_q bytes apart
 *   scales  [E][N][ld_s] uint8       K / 32 bytes of a row are read; experts lie N ld_s bytes apart
 *   bias    [E][ld_b] of `dtype`     N columns; NULL: no bias
 *
 *   nnop_moe_mx_decode_linear  ys[s][n] = sum_c xs[s][c] W_e(n, c) + bias[e][n]     offsets[e] <= s < offsets[e+1]
 *   Every other row of ys comes back as +0 in the columns that exist.  Padding columns are untouched.
 *
 * Contracts:
 *   - Sums are fp32 on the matrix cores, the bias is added in fp32, there is one rounding, on the store.  No atomics, no workspace, no
 *     allocation, no sync; the call can be captured in a graph.  Two runs are bitwise equal.
 *   - offsets is read on the device, clamped into [0, S].  Nothing is read or written out of bounds whatever offsets holds.
 *   - The terms of one output element are added in an order that is a function of K and `dtype` alone -- not of S, E, the plan or where
 *     in its expert's range a row lies.  So a row's bits do not depend on the plan or on the other rows of the batch: the same xs row
 *     sent to the same expert gives the same ys row, bit for bit, in any batch.
 *   - That order is not the 128 x 128 tile's: the result is NOT promised bit-equal to nnop_moe_mx_linear.  Both are fp32 sums of the same
 *     products and lie inside any bound that does not depend on the order of summation.
 *   - Masking is by selection: the blocks and scales of another expert (a scale byte of 255 included), the rows outside an expert and
 *     the padding never enter a result that is kept.
 *   - Made for few rows per expert: an expert with up to 32 rows streams its weights once; more rows stream them once per 32 rows.  It
 *     is correct for any plan and slower than nnop_moe_mx_linear from a few dozen rows per expert on.
 *   - xs takes 16-byte loads where ld_x is a multiple of 8 and xs is 16-byte aligned; ys (with a bias: and the bias) takes 8-byte
 *     accesses where ld_y (ld_b) is a multiple of 4 and the base is 8-byte aligned; element-wise accesses otherwise.  Any N >= 1.
 *
 * Checks, in this order, all before any device work:
 *   NNOP_ERR_NULL    the descriptor itself is NULL
 *   NNOP_ERR_DTYPE   dtype is not NNOP_F16 or NNOP_BF16
 *   NNOP_ERR_OPTS    flags is not 0, or a reserved field is not 0
 *   NNOP_ERR_SHAPE   S < 1, E outside 1 ... 1024, K or N outside 1 ... 65536, K no multiple of 32, ld_x < K, ld_y < N, ld_b < N,
 *                    ld_q < K / 2 or no multiple of 16, ld_s < K / 32, or more than 2^31 - 1 workgroups (E ceil(N / 256): the bounds on E
 *                    and N keep it below that)
 *   NNOP_ERR_NULL    a NULL pointer; bias is the only optional one
 *   NNOP_ERR_ALIGN   a row array or the bias not aligned to its element size, blocks not aligned to 16 bytes, offsets not to 4
 */
typedef struct nnop_moe_mx_decode_desc {
    int32_t dtype;        /* nnop_dtype of the rows and the bias: NNOP_F16 or NNOP_BF16 */
    int32_t rows;         /* S */
    int32_t experts;      /* E */
    int32_t in_dim;       /* K, a multiple of 32 */
    int32_t out_dim;      /* N */
    int32_t ld_x;         /* row stride of xs in elements */
    int32_t ld_y;         /* row stride of ys in elements */
    int32_t ld_b;         /* row stride of bias in elements */
    int32_t ld_q;         /* bytes between two packed weight rows: >= K / 2, a multiple of 16 */
    int32_t ld_s;         /* bytes between two scale rows: >= K / 32 */
    uint32_t flags;       /* 0 */
    int32_t reserved[5];  /* 0 */
} nnop_moe_mx_decode_desc; /* 64 bytes */

int nnop_moe_mx_decode_linear(const nnop_moe_mx_decode_desc* d, void* ys, const void* xs, const uint8_t* blocks, const uint8_t* scales,
                              const void* bias, const int32_t* offsets, nnop_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NNOP_HIP_MOE_MX_DECODE_H */
