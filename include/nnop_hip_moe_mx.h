/*
 * nnop_hip_moe_mx.h -- C ABI of libnnop_hip_moe_mx.so: the expert linear layers of nnop_hip_moe_linear.h on MXFP4 weights as a gpt-oss
 * checkpoint ships them (gate_up_proj_blocks / _scales, down_proj_blocks / _scales), read where they lie -- the forward and the pullback
 * to the rows -- and the two conversions between that form and an array of floats.  Packed weights are frozen: there is no weight
 * gradient.  The bias gradient is nnop_moe_linear_bwd_b of the sixth library.
 *
 * A seventh library beside libnnop_hip.so (nnop_hip.h), libnnop_hip_ext.so, libnnop_hip_moe.so, libnnop_hip_moe_data.so,
 * libnnop_hip_moe_gemm.so and libnnop_hip_moe_linear.so, built the same way as the sixth: an ABI version of its own, nothing linked from
 * the other six, only this header's functions exported.  nnop_dtype, nnop_status and nnop_stream_t come from nnop_hip.h; a status code is
 * turned into text by the main library's nnop_strerror().  gfx950 (MI355X) only.  Launches are asynchronous on the caller's stream;
 * nothing is allocated and there is no workspace.
 *
 * The format (OCP Microscaling Formats v1.0, MXFP4): a row of K values, K a multiple of 32, is K / 32 blocks.
 *   blocks  uint8, 16 bytes per block: byte j holds element 2j in its low nibble and element 2j + 1 in its high nibble
 *   scales  uint8, one byte per block
 *   A nibble c is E2M1: bit 3 is the sign, c & 7 = 0 ... 7 are the magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6 (c = 8 is -0).
 *   A scale byte e = 0 ... 254 is 2^(e - 127); e = 255 is NaN: every element of that block is NaN.
 *   value = magnitude(c) 2^(e - 127), rounded to the target type to nearest even: too large a value becomes +-Inf, subnormal results are
 *   kept.  In float32 and bfloat16 the product is exact unless it overflows (magnitudes 4 and 6 at e = 253, 2 and above at e = 254).
 *
 * The quantiser (the floor rule of that specification), per block, on the inputs converted exactly to float32:
 *   any element not finite       scale byte 255, every nibble 0
 *   amax = max |x| = 0           scale byte 0, every nibble is the sign alone (+-0)
 *   otherwise                    s = clamp(floor(log2(amax)) - 2, -127, 127), scale byte s + 127; |x| / 2^s goes to the nearest magnitude,
 *                                a tie to the one with the even nibble (0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4,
 *                                5 -> 4), anything above 6 to 6; the sign is kept
 */
#ifndef NNOP_HIP_MOE_MX_H
#define NNOP_HIP_MOE_MX_H

#include "nnop_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NNOP_HIP_MOE_MX_ABI_VERSION 1
int nnop_moe_mx_abi_version(void);

/*
 * S slot rows, E experts, K input and N output features, as in nnop_hip_moe_linear.h.  W_e(n, c) is the dequantised value of element c
 * of weight row n of expert e, rounded to `dtype`.
 *
 *   offsets [E+1] int32              as nnop_moe_plan writes it
 *   xs, dxs [S][ld_x] of `dtype`     slot order, K columns
 *   ys, dys [S][ld_y] of `dtype`     slot order, N columns
 *   blocks  [E][N][ld_q] uint8       K / 2 bytes of a row are read; experts lie N ld_q bytes apart
 *   scales  [E][N][ld_s] uint8       K / 32 bytes of a row are read; experts lie N ld_s bytes apart
 *   bias    [E][ld_b] of `dtype`     N columns; NULL: no bias
 *
 *   nnop_moe_mx_linear        ys[s][n]  = sum_c xs[s][c] W_e(n, c) + bias[e][n]     offsets[e] <= s < offsets[e+1]
 *   nnop_moe_mx_linear_bwd_x  dxs[s][c] = sum_n dys[s][n] W_e(n, c)
 *   Every other row of ys / dxs comes back as +0 in the columns that exist.
 *
 * Contracts: those of nnop_hip_moe_linear.h, unchanged.  offsets is read on the device, clamped into [0, S]; no sync, no allocation, the
 * calls can be captured in a graph.  Nothing is read or written out of bounds whatever offsets holds.  Masking is by selection: the
 * blocks and scales of another expert (a NaN scale included) and the rows outside an expert never enter a result that is kept.  Sums are
 * fp32 on the matrix cores, the bias is added in fp32, there is one rounding, on the store; no atomics, so two runs are bitwise equal.
 *   - The weights are expanded to `dtype` in the registers that stage them; everything behind that is the code of nnop_moe_linear.  So
 *     ys and dxs equal those of nnop_moe_linear / nnop_moe_linear_bwd_x on nnop_mxfp4_dequant(blocks, scales) in [E][N][K] order, bit for
 *     bit.
 *   - The rows take the 16-byte path where K, N, ld_x, ld_y (the forward with a bias: ld_b) are multiples of 8 and xs / ys / bias (dxs /
 *     dys) are 16-byte aligned, and an element-wise path otherwise.  The packed operand has the aligned form only.
 *
 * Checks, in this order, all before any device work, the same for the two calls:
 *   NNOP_ERR_NULL    the descriptor itself is NULL
 *   NNOP_ERR_DTYPE   dtype is not NNOP_F16 or NNOP_BF16
 *   NNOP_ERR_OPTS    flags is not 0, or a reserved field is not 0
 *   NNOP_ERR_SHAPE   S < 1, E outside 1 ... 1024, K or N outside 1 ... 65536, K no multiple of 32, ld_x < K, ld_y < N, ld_b < N,
 *                    ld_q < K / 2 or no multiple of 16, ld_s < K / 32, or more than 2^31 - 1 output tiles of 128 x 128
 *   NNOP_ERR_NULL    a NULL pointer; bias is the only optional one
 *   NNOP_ERR_ALIGN   a row array or the bias not aligned to its element size, blocks not aligned to 16 bytes, offsets not to 4
 */
typedef struct nnop_moe_mx_desc {
    int32_t dtype;        /* nnop_dtype of the rows and the bias: NNOP_F16 or NNOP_BF16 */
    int32_t rows;         /* S */
    int32_t experts;      /* E */
    int32_t in_dim;       /* K, a multiple of 32 */
    int32_t out_dim;      /* N */
    int32_t ld_x;         /* row stride of xs, dxs in elements */
    int32_t ld_y;         /* row stride of ys, dys in elements */
    int32_t ld_b;         /* row stride of bias in elements */
    int32_t ld_q;         /* bytes between two packed weight rows: >= K / 2, a multiple of 16 */
    int32_t ld_s;         /* bytes between two scale rows: >= K / 32 */
    uint32_t flags;       /* 0 */
    int32_t reserved[5];  /* 0 */
} nnop_moe_mx_desc;       /* 64 bytes */

int nnop_moe_mx_linear(const nnop_moe_mx_desc* d, void* ys, const void* xs, const uint8_t* blocks, const uint8_t* scales,
                       const void* bias, const int32_t* offsets, nnop_stream_t stream);
int nnop_moe_mx_linear_bwd_x(const nnop_moe_mx_desc* d, void* dxs, const void* dys, const uint8_t* blocks, const uint8_t* scales,
                             const int32_t* offsets, nnop_stream_t stream);

/*
 * The conversions, row by row: `rows` rows of `cols` = K values.
 *
 *   nnop_mxfp4_dequant  out[r][c] = value(blocks[r], scales[r])[c] rounded to `dtype`          out    [rows][ld] of `dtype`
 *   nnop_mxfp4_quant    (blocks[r], scales[r]) = the quantiser above of in[r][0 ... K-1]        in     [rows][ld] of `dtype`
 *                                                                                              blocks [rows][ld_q], scales [rows][ld_s]
 * Columns behind K, K / 2 and K / 32 are padding: neither read nor written.  The conversion of nnop_mxfp4_dequant is the one the two
 * products above apply to their weights (one device function).  Accesses to out / in are 16 bytes wide where ld is a multiple of 16
 * bytes of elements and the base is 16-byte aligned, element-wise otherwise.
 *
 * Checks, in this order, all before any device work, the same for the two calls:
 *   NNOP_ERR_NULL    the descriptor itself is NULL
 *   NNOP_ERR_DTYPE   dtype is unknown
 *   NNOP_ERR_OPTS    the reserved field is not 0
 *   NNOP_ERR_SHAPE   rows < 1, K outside 32 ... 2^30 or no multiple of 32, ld < K, ld_q < K / 2 or no multiple of 16, ld_s < K / 32, or
 *                    rows K / 8 above 2^39 (the grid)
 *   NNOP_ERR_NULL    a NULL pointer
 *   NNOP_ERR_ALIGN   out / in not aligned to its element size, blocks not aligned to 16 bytes
 */
typedef struct nnop_mxfp4_desc {
    int32_t dtype;     /* nnop_dtype of out / in */
    int32_t reserved;  /* 0 */
    int64_t rows;
    int32_t cols;      /* K, a multiple of 32 */
    int32_t ld;        /* row stride of out / in in elements */
    int32_t ld_q;      /* bytes between two rows of blocks: >= K / 2, a multiple of 16 */
    int32_t ld_s;      /* bytes between two rows of scales: >= K / 32 */
} nnop_mxfp4_desc;     /* 32 bytes */

int nnop_mxfp4_dequant(const nnop_mxfp4_desc* d, void* out, const uint8_t* blocks, const uint8_t* scales, nnop_stream_t stream);
int nnop_mxfp4_quant(const nnop_mxfp4_desc* d, uint8_t* blocks, uint8_t* scales, const void* in, nnop_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NNOP_HIP_MOE_MX_H */
