/*
 * nnop_hip_moe_gemm.h -- C ABI of libnnop_hip_moe_gemm.so: the expert GEMMs of a mixture-of-experts layer, one grouped GEMM over the
 * dispatch plan of nnop_moe_plan (nnop_hip_moe.h), with its two pullbacks.  It runs between nnop_moe_permute and nnop_moe_combine
 * (nnop_hip_moe_data.h): router -> plan -> permute -> GEMM -> glu -> GEMM -> combine.
 *
 * A fifth library beside libnnop_hip.so (nnop_hip.h), libnnop_hip_ext.so (nnop_hip_ext.h), libnnop_hip_moe.so (nnop_hip_moe.h) and
 * libnnop_hip_moe_data.so (nnop_hip_moe_data.h), built the same way as the third and fourth: an ABI version of its own, nothing linked
 * from the other four, only this header's functions exported.  nnop_dtype, nnop_status and nnop_stream_t come from nnop_hip.h; a status
 * code is turned into text by the main library's nnop_strerror().  gfx950 (MI355X) only.  Launches are asynchronous on the caller's
 * stream; nothing is allocated and there is no workspace.
 */
#ifndef NNOP_HIP_MOE_GEMM_H
#define NNOP_HIP_MOE_GEMM_H

#include "nnop_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NNOP_HIP_MOE_GEMM_ABI_VERSION 1
int nnop_moe_gemm_abi_version(void);

/*
 * S slot rows (the plan's T k), E experts, K input and N output features.
 *
 *   offsets [E+1] int32                 as nnop_moe_plan writes it: expert e owns the slot rows offsets[e] ... offsets[e+1]-1
 *   xs, dxs [S][ld_x] of `dtype`        slot (expert-sorted) order, K columns
 *   ys, dys [S][ld_y] of `dtype`        slot order, N columns
 *   w, dw   [E][N][ld_w] of `dtype`     stacked nn.Linear weights: row n of expert e holds the K input coefficients, experts lie
 *                                       N ld_w elements apart
 * Columns K ... ld_x-1, N ... ld_y-1 and K ... ld_w-1 are padding: neither read nor written.
 *
 * With every offset clamped into [0, S], lo_e = offsets[e], hi_e = offsets[e+1], and an empty range where hi_e <= lo_e:
 *
 *   nnop_moe_gemm        ys[s][n]    = sum_c xs[s][c]  w[e][n][c]     lo_e <= s < hi_e;   every other row of ys:  +0 in columns < N
 *   nnop_moe_gemm_bwd_x  dxs[s][c]   = sum_n dys[s][n] w[e][n][c]     lo_e <= s < hi_e;   every other row of dxs: +0 in columns < K
 *   nnop_moe_gemm_bwd_w  dw[e][n][c] = sum_{s in [lo_e, hi_e)} dys[s][n] xs[s][c]         an expert without rows: +0 everywhere
 *
 * Contracts:
 *   - offsets is read on the device.  There is no device-to-host copy, no sync and no allocation: the three calls can be captured in a
 *     graph.  The grid is sized on the host from S and E alone (with a row tile of BM rows there are at most S / BM + min(E, S)
 *     non-empty row tiles, and two more ranges for the rows in front of the first and behind the last expert); each workgroup finds its
 *     (expert, tile) from offsets itself, and surplus workgroups leave.
 *   - Nothing is read or written out of bounds whatever offsets holds: every loop bound on the device is a descriptor field or a clamped
 *     offset, so garbage offsets can make the result meaningless but cannot make a kernel run away.  With offsets that are not
 *     non-decreasing a row may be written twice, by the wrong expert or not at all.  With the plan's offsets every element in columns
 *     < N / < K of every output row, and every element of dw in columns < K, is written exactly once: a caller never pre-zeroes.
 *   - Rows outside an expert's range are never read into a product that is kept: the last row tile of an expert, and the last reduction
 *     step of nnop_moe_gemm_bwd_w, select zeros for them (no multiplication by 0), whatever those rows hold, NaN and Inf included.
 *     The rows behind offsets[E] are not read at all.
 *   - Accumulation is in fp32 on the matrix cores, with one rounding to `dtype` on the store.  There are no atomics and no split over
 *     the reduction axis, so two runs are bitwise equal.  For nnop_moe_gemm_bwd_w the reduction axis is the expert's rows: one workgroup
 *     owns an (expert, N-tile, K-tile) and walks that expert's rows.
 *   - Not in place: the inputs and outputs of one call do not overlap.  This is not checked.
 *
 * The fast path is taken where K, N, ld_x, ld_y and ld_w are multiples of 8 elements and the three bases are 16-byte aligned: global
 * accesses are then 16 bytes wide.  Everything else takes an element-wise path of the same structure.  Row offsets are computed in 64
 * bits; E N ld_w may exceed 2^31.
 *
 * Checks, in this order, all before any device work, the same for the three calls:
 *   NNOP_ERR_NULL    the descriptor itself is NULL (first of all)
 *   NNOP_ERR_DTYPE   dtype is unknown
 *   NNOP_ERR_OPTS    a reserved field is not 0
 *   NNOP_ERR_SHAPE   S < 1, E outside 1 ... 1024, K or N outside 1 ... 65536, ld_x < K, ld_y < N, ld_w < K, or more than 2^31 - 1
 *                    output tiles of 128 x 128 (no array that fits a device's memory comes near that)
 *   NNOP_ERR_NULL    a NULL pointer: none is optional
 *   NNOP_ERR_ALIGN   a row or weight array not aligned to the element size, offsets not aligned to 4 bytes
 */
typedef struct nnop_moe_gemm_desc {
    int32_t dtype;        /* nnop_dtype of the row and weight arrays */
    int32_t rows;         /* S */
    int32_t experts;      /* E */
    int32_t in_dim;       /* K */
    int32_t out_dim;      /* N */
    int32_t ld_x;         /* row stride of xs, dxs in elements */
    int32_t ld_y;         /* row stride of ys, dys in elements */
    int32_t ld_w;         /* row stride of a weight row in elements */
    int32_t reserved[2];  /* 0: kept for a per-expert bias, a [E][K][N] weight layout and accumulation into dw */
} nnop_moe_gemm_desc;     /* 40 bytes */

int nnop_moe_gemm(const nnop_moe_gemm_desc* d, void* ys, const void* xs, const void* w, const int32_t* offsets, nnop_stream_t stream);
int nnop_moe_gemm_bwd_x(const nnop_moe_gemm_desc* d, void* dxs, const void* dys, const void* w, const int32_t* offsets,
                        nnop_stream_t stream);
int nnop_moe_gemm_bwd_w(const nnop_moe_gemm_desc* d, void* dw, const void* dys, const void* xs, const int32_t* offsets,
                        nnop_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NNOP_HIP_MOE_GEMM_H */
