/*
 * nnop_hip_moe.h -- C ABI of libnnop_hip_moe.so: mixture-of-experts routing (the top-k gate and the expert dispatch plan).
 *
 * A third library beside libnnop_hip.so (nnop_hip.h, frozen with NNop.jl's operators) and libnnop_hip_ext.so (nnop_hip_ext.h), built the
 * same way as the second: an ABI version of its own, nothing linked from the other two, only this header's functions exported.
 * nnop_dtype, nnop_status and nnop_stream_t come from nnop_hip.h; a status code is turned into text by the main library's
 * nnop_strerror().  gfx950 (MI355X) only.  Launches are asynchronous on the caller's stream; nothing is allocated.
 */
#ifndef NNOP_HIP_MOE_H
#define NNOP_HIP_MOE_H

#include "nnop_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NNOP_HIP_MOE_ABI_VERSION 1
int nnop_moe_abi_version(void);

/*
 * The gate: top-k selection over E expert logits per token, the routing weights and the row's log-sum-exp.
 *
 *   logits [T][ld] of `dtype`, ld >= E in elements (columns E .. ld-1 are padding: neither read nor written)
 *   idx [T][k] int32    w [T][k] fp32    lse [T] fp32
 *
 * Selection, on the logits upcast to fp32 (exact, the same for both norms): the larger value first; NaN ranks above +inf; equal values
 * (-0 and +0, NaN and NaN included) go to the lower expert index.  idx[t] is in selection order, best first, and always holds k distinct
 * values in [0, E), whatever the row contains.
 * Weights, in fp32:   lse = log sum_e exp(x[e])   (over all E)
 *   NNOP_MOE_NORM_TOPK   w[j] = exp(x[idx[j]] - x[idx[0]]) / sum_i exp(x[idx[i]] - x[idx[0]])       softmax over the k selected logits
 *   NNOP_MOE_NORM_ALL    w[j] = exp(x[idx[j]] - lse)                                                the full softmax, gathered
 * A row for which these formulas give NaN in IEEE arithmetic (a NaN or +inf logit, or every logit -inf) has NaN weights, that row only.
 *
 * Pullback: dlogits [T][ld] of `dtype`, every column < E written once.  With p[e] = exp(x[e] - lse) recomputed from the saved lse
 * (nothing of size T x E is saved) and S = sum_j w[j] dw[j]:
 *   NORM_TOPK   dlogits[e] = sum_{j: idx[j] = e} w[j] (dw[j] - S)  +  dlse p[e]
 *   NORM_ALL    dlogits[e] = sum_{j: idx[j] = e} w[j] dw[j]        +  (dlse - S) p[e]
 * dlse (fp32 [T], the cotangent of lse, e.g. of a router z-loss) may be NULL and then counts as 0; with NORM_TOPK and no dlse the logits
 * are not read and every entry outside idx[t] is an exact zero.
 *
 * Shapes: every E in 1 ... 1024, every k in 1 ... min(E, 16).  Rows whose length, stride and bases allow it move in 16-byte pieces
 * (E and ld multiples of 16 / sizeof(dtype), 16-byte-aligned logits / dlogits); everything else element-wise.
 *
 * Checks, in this order, all before any device work:
 *   NNOP_ERR_DTYPE   dtype is unknown
 *   NNOP_ERR_OPTS    norm is neither of the two values, or a reserved field is not 0
 *   NNOP_ERR_SHAPE   E outside 1 ... 1024, k outside 1 ... min(E, 16), T < 1, ld < E, or T k > 2^31 - 1
 *   NNOP_ERR_NULL    a NULL pointer other than dlse (the descriptor itself: first of all)
 *   NNOP_ERR_ALIGN   logits / dlogits not aligned to the element size, an fp32 or int32 array not aligned to 4 bytes
 *
 * reserved[] is kept for what this version leaves out: sigmoid scoring with a selection bias and group-limited choice.
 */
typedef enum nnop_moe_norm {
    NNOP_MOE_NORM_TOPK = 0,
    NNOP_MOE_NORM_ALL  = 1
} nnop_moe_norm;

typedef struct nnop_moe_router_desc {
    int32_t dtype;         /* nnop_dtype of logits and dlogits */
    int32_t tokens;        /* T */
    int32_t experts;       /* E */
    int32_t topk;          /* k */
    int32_t ld;            /* row stride of logits and dlogits, in elements */
    int32_t norm;          /* nnop_moe_norm */
    int32_t reserved[2];   /* 0 */
} nnop_moe_router_desc;    /* 32 bytes */

int nnop_moe_router(const nnop_moe_router_desc* d, int32_t* idx, float* w, float* lse, const void* logits, nnop_stream_t stream);
int nnop_moe_router_bwd(const nnop_moe_router_desc* d, void* dlogits, const float* dw, const float* dlse, const float* w,
                        const int32_t* idx, const float* lse, const void* logits, nnop_stream_t stream);

/*
 * The dispatch plan: a stable counting sort of the T k flat assignment ids t k + j by expert.
 *
 *   idx [T][k] int32, from any producer (distinct entries are not required)
 *   counts [E]       assignments per expert
 *   offsets [E + 1]  the exclusive prefix of counts; offsets[E] = the number of valid assignments
 *   perm [T k]       perm[s] = the flat id in expert-sorted slot s (within one expert: ascending), -1 for s >= offsets[E]
 *   slot [T][k]      the inverse: perm[slot[t][j]] = t k + j
 * An entry outside [0, E) (expert-parallel callers mark non-local experts with -1) is skipped: counted nowhere, its slot is -1.
 * Nothing is written out of bounds whatever idx holds.
 *
 * Deterministic, no atomics: every wave counts a contiguous chunk of flat ids into its own histogram in the workspace, two scan
 * kernels turn the histograms into start positions (over chunks, then over experts), and a scatter pass ranks equal experts inside a
 * chunk in flat-id order.  Every workspace word that is read is written first, whatever the workspace held.
 *
 * Checks, in this order:  NNOP_ERR_OPTS a reserved field is not 0;  NNOP_ERR_SHAPE T < 1, k < 1, E outside 1 ... 1024 or T k > 2^31 - 1;
 * NNOP_ERR_NULL;  NNOP_ERR_ALIGN an array not aligned to 4 bytes or a workspace not aligned to 16;  NNOP_ERR_WORKSPACE
 * workspace_bytes < nnop_moe_plan_workspace_bytes().
 */
typedef struct nnop_moe_plan_desc {
    int32_t tokens;        /* T */
    int32_t topk;          /* k */
    int32_t experts;       /* E */
    int32_t reserved[1];   /* 0 */
} nnop_moe_plan_desc;      /* 16 bytes */

/* 0 for NULL and for a descriptor that fails the descriptor checks */
size_t nnop_moe_plan_workspace_bytes(const nnop_moe_plan_desc* d);
int nnop_moe_plan(const nnop_moe_plan_desc* d, int32_t* counts, int32_t* offsets, int32_t* perm, int32_t* slot, const int32_t* idx,
                  void* workspace, size_t workspace_bytes, nnop_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NNOP_HIP_MOE_H */
