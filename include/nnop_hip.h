/*
 * nnop_hip.h -- C ABI of libnnop_hip.so: MI355X (gfx950) Flash Attention behind NNop.jl's
 * operator boundary.
 *
 * These are exactly the entry points a Julia package extension of the shape of
 * ext/NNopAMDGPUExt.jl:1-11 `ccall`s to replace, for ROCArray arguments, the two generic
 * host functions of the reference:
 *
 *   NNop._flash_attention(q,k,v,pair; causal,kpad_mask) -> (o, ms, ls)   src/attention.jl:133-177
 *   NNop.∇flash_attention(Δ,o,ms,ls,q,k,v,pair; causal,kpad_mask)
 *                                      -> (dq, dk, dv, dpair|nothing)   src/attention_bwd.jl:199-275
 *   NNop._shared_memory(backend, device_id) -> UInt64                    ext/NNopAMDGPUExt.jl:6-9
 *
 * (binding shown in INTEGRATION.md; shipped, source-only, in nnop.jl_amd/julia/).
 *
 * Conventions
 *   - Plain pointers and sizes only; no C++ / torch types cross this boundary.
 *   - Every pointer is a DEVICE pointer on the current HIP device; the caller owns every
 *     buffer, outputs and workspace included (replaces the reference's internal
 *     `similar` / `KA.zeros`, src/attention.jl:166-168, src/attention_bwd.jl:224-238).
 *   - All tensors dense, contiguous, E fastest -- Julia column-major (E,L,H,B) is the same
 *     memory as C row-major [B][H][L][E]:
 *        q,o,dO,dq : [B][QH][QL][E]      k,v,dk,dv : [B][KH][KL][E]
 *        ms,ls     : [B][QH][QL]         (dtype T, src/attention.jl:167-168)
 *        pair,dpair: [B][KL][QL][QH]     (Julia (QH,QL,KL,B), src/attention.jl:62)
 *        kpad_mask : [B][KL], 1 byte per element, nonzero = key is valid (Julia Bool matrix
 *                    (KL,B), src/attention.jl:76)
 *   - Launches are asynchronous on the passed stream; nothing synchronises, allocates or
 *     frees; no pointer is retained after return (src/attention.jl:170-176 never syncs).
 *   - Re-entrant; no mutable global state.  Safe from concurrent host threads on different
 *     streams / devices.  The caller selects the device (hipSetDevice) before calling.
 *   - Errors are returned, never thrown: 0 = success, negative = nnop_status.  The host shim
 *     re-raises with the reference's messages (src/attention.jl:141-144).
 */
#ifndef NNOP_HIP_H
#define NNOP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* element type T of q,k,v,o,ms,ls,pair and all gradients (they share one T,
 * src/attention.jl:134-137) */
typedef enum nnop_dtype {
    NNOP_F32  = 0,
    NNOP_F16  = 1,
    NNOP_BF16 = 2
} nnop_dtype;

typedef enum nnop_status {
    NNOP_OK                 =  0,
    NNOP_ERR_EMB_MISMATCH   = -1,  /* "Embedding dim of Q `..` must be the same as of K" (attention.jl:141) */
    NNOP_ERR_KV_SHAPE       = -2,  /* "Shapes of K and V must be the same"               (attention.jl:142) */
    NNOP_ERR_EMB_NOT_POW2   = -3,  /* "Only power-of-2 embedding dims are supported."     (attention.jl:143) */
    NNOP_ERR_HEADS          = -4,  /* "Number of query heads must be divisible by ..."    (attention.jl:144) */
    NNOP_ERR_DTYPE          = -5,  /* dtype not one of nnop_dtype (Julia: MethodError)                       */
    NNOP_ERR_NULL           = -6,  /* a required pointer is NULL                                             */
    NNOP_ERR_EMB_UNSUPPORTED= -7,  /* power of two above 512 ("Failed to find groupsize
                                      ... Shared Memory constraint", attention.jl:204)                       */
    NNOP_ERR_SHAPE          = -8,  /* a non-positive / overflowing dimension                                 */
    NNOP_ERR_WORKSPACE      = -9,  /* workspace smaller than nnop_fa_bwd_workspace_bytes                      */
    NNOP_ERR_HIP            = -10, /* HIP runtime error at launch (hipGetLastError)                          */
    NNOP_ERR_ALIGN          = -11, /* a tensor or workspace base address is not aligned as the kernels need:
                                      16 bytes for q, k, v, o, dO, dq, dk, dv and the workspace
                                      (the MFMA kernels move them with 16-byte vector accesses and LDS-DMA),
                                      the element size for pair / dpair (a batch slice of a bias, nnop_fa_shards'
                                      pair_off, starts at any element) and for ms, ls.  Embedding dims that run the plain-HIP
                                      kernels (not 16 / 32 / 64 / 128 / 256) need element alignment only.      */
    NNOP_ERR_OPTS           = -12  /* invalid attention options (nnop_fa_opts): a reserved field is not 0, or a window
                                      side is below -1 (ABI version 7); nnop_glu_desc: an unknown act or layout, or
                                      a bad alpha / limit                                                        */
} nnop_status;

/*
 * Problem descriptor.  The reference reads all of this from the array sizes
 * (src/attention.jl:138-139); across a C boundary the caller states it.
 * `emb_k`, `kl_v`, `kh_v`, `emb_v` carry the K / V sizes that the reference's checks
 * compare (E of K vs Q; size(k) == size(v)), so that those checks -- and their error
 * codes -- live behind the boundary like they do in the reference.
 */
typedef struct nnop_fa_desc {
    int32_t dtype;    /* nnop_dtype */
    int32_t emb;      /* E  = size(q,1) */
    int32_t ql;       /* QL = size(q,2) */
    int32_t kl;       /* KL = size(k,2) */
    int32_t qh;       /* QH = size(q,3) */
    int32_t kh;       /* KH = size(k,3) */
    int32_t batch;    /* B  = size(q,4) */
    int32_t causal;   /* keyword `causal` (required in the reference, attention_crc.jl:7) */
    int32_t emb_k;    /* size(k,1); 0 means "same as emb" */
    int32_t emb_v;    /* size(v,1); 0 means "same as emb" */
    int32_t kl_v;     /* size(v,2); 0 means "same as kl"  */
    int32_t kh_v;     /* size(v,3); 0 means "same as kh"  */
} nnop_fa_desc;

/* Opaque to the ABI: a hipStream_t.  Declared void* so that C callers need no HIP headers. */
typedef void* nnop_stream_t;

/*
 * Forward: contract of NNop._flash_attention (src/attention.jl:133-177) + kernel
 * _flash_attention_fwd! (src/attention.jl:1-131).
 *   o  = softmax(scale * q k^T (+pair) masked) v
 *   ms = row max of the scaled+biased+masked logits   (src/attention.jl:128)
 *   ls = sum_j exp(logit_j - ms)                       (src/attention.jl:129)
 * `pair` and `kpad_mask` may be NULL (Julia `nothing`).
 */
int nnop_fa_fwd(const nnop_fa_desc* d,
                void* o, void* ms, void* ls,
                const void* q, const void* k, const void* v,
                const void* pair, const uint8_t* kpad_mask,
                nnop_stream_t stream);

/*
 * Per-call attention options (ABI version 7), for nnop_fa_fwd_ex / nnop_fa_bwd_ex.  NULL means "no options" and is exactly
 * nnop_fa_fwd / nnop_fa_bwd.
 *
 * Sliding-window (local) attention, flash-attn's `window_size` convention: query row i sees key j only if
 *     (window_left  < 0 || j >= i - window_left)  and  (window_right < 0 || j <= i + window_right)
 * on top of the causal rule (j <= i) and kpad_mask.  -1 = that side is unbounded; a value below -1 is NNOP_ERR_OPTS.
 * The window is TOP-LEFT aligned whatever QL and KL are: query i lines up with key i, as the causal mask does
 * (src/attention.jl:41-43).  A row that sees no key follows the usual convention (NaN in o, -inf in ms, dq = 0).
 * A side that removes no key (window_left >= QL - 1, window_right >= KL - 1, or any window_right >= 0 under causal) counts as
 * unbounded; when both sides are, the call is exactly the call without options.  A window needs no extra workspace.
 * `reserved` must be all 0 (room for later per-call options).
 */
typedef struct nnop_fa_opts {
    int32_t window_left;
    int32_t window_right;
    int32_t reserved[6];
} nnop_fa_opts;

int nnop_fa_fwd_ex(const nnop_fa_desc* d, const nnop_fa_opts* opts,
                   void* o, void* ms, void* ls,
                   const void* q, const void* k, const void* v,
                   const void* pair, const uint8_t* kpad_mask,
                   nnop_stream_t stream);

/*
 * Learned per-head attention sinks (gpt-oss): nnop_fa_fwd_ex / nnop_fa_bwd_ex plus one trainable logit per QUERY head.
 *   sinks : fp32 [QH], in the units of the scaled logits (scale * q.k).  Under GQA the query heads of one kv head each keep their own.
 * The sink joins every row's softmax as one more column that has no value vector:
 *   p_ij = exp(s_ij - m_i) / (sum_j' exp(s_ij' - m_i) + exp(sigma_h - m_i)),   o_i = sum_j p_ij v_j
 * i.e. concatenate sigma_h to the row's logits, softmax, drop the sink's column (rows of p then need not sum to 1).  The causal rule,
 * the window, kpad_mask and pair act on the real keys only (pair has no entry for the sink); the sink column is seen by every row.
 *   ms = max(row max of the real logits, sigma_h), rounded to T as always;  ls = sum_j exp(s_ij - ms) + exp(sigma_h - ms), relative to the
 *        rounded ms.  (o, ms, ls) stay self-consistent: the backward recomputes the right P from them.
 *   A row that sees no key but a finite sink is NOT dead: o = 0, ms = sigma_h (rounded to T), ls = exp(sigma_h - ms) (1 up to that
 *   rounding); in the backward its dq is 0 and it adds 0 to dsinks.
 *   sigma_h = -inf is allowed and means "no sink" for that head: its results are the results without sinks.  +inf or NaN give NaN rows
 *   (not checked).  A large sigma does not overflow (sigma = +200 with logits near 0: o ~ 0, ms = 200, ls ~ 1).
 * Backward: dq, dk, dv, dpair as for nnop_fa_bwd_ex, and
 *   dsinks : fp32 [QH], fully overwritten:  dsinks_h = -sum_{b,i} exp(sigma_h - ms_bhi) / ls_bhi * sum_e dO_bhie o_bhie,
 *            computed from the T-valued ms, ls, o and dO that the call receives; bitwise the same whichever backward kernels run, and
 *            run to run (fixed-order reduction, no atomics).
 * sinks == NULL is exactly nnop_fa_fwd_ex / nnop_fa_bwd_ex (dsinks is then ignored, as dpair is without pair).  With sinks, a NULL
 * dsinks is NNOP_ERR_NULL.  sinks and dsinks need 4-byte alignment (else NNOP_ERR_ALIGN).  Checks: the descriptor, the options, NULL
 * pointers, alignment, in that order.  A sink needs no extra workspace: nnop_fa_bwd_workspace_bytes(_pair) are unchanged.
 * Not supported by the sharding rectangles of nnop_fa_shards: a sharded dsinks would be a partial sum over batches.
 */
int nnop_fa_fwd_sinks(const nnop_fa_desc* d, const nnop_fa_opts* opts, const float* sinks,
                      void* o, void* ms, void* ls,
                      const void* q, const void* k, const void* v,
                      const void* pair, const uint8_t* kpad_mask,
                      nnop_stream_t stream);

/*
 * Logit soft-capping (Gemma-2: c = 50, Grok-1: c = 30; flash-attn's `softcap`): nnop_fa_fwd_sinks / nnop_fa_bwd_sinks plus a cap c > 0
 * on the SCALED scores.  With scale = 1/sqrt(E):
 *     s_ij = scale * q_i.k_j
 *     z_ij = c * tanh(s_ij / c)                  the capped score
 *     x_ij = z_ij + pair_ij                      pair is added AFTER the cap and is never capped
 *     x_ij = -inf where the causal rule, the window or kpad_mask hide key j from query i
 *     P    = softmax_j(x_ij [, sinks_h as one more column, not capped]),   o = P v
 *     ms, ls: row max and sum-exp of x (with the sink where given), as always
 * Backward, with dS = P o (dP - delta), the gradient with respect to x, as always:
 *     dpair = dS                                 unchanged
 *     dS'   = dS o (1 - (z / c)^2)               through the tanh
 *     dQ = scale dS' K     dK = scale dS'^T Q (summed over the GQA group)     dV = P^T dO (unchanged)     dsinks: unchanged
 * Rows that see no key keep their convention (NaN in o, ms = -inf, dq = 0).  The cap arithmetic is fp32 for every element type.
 * softcap == 0 means no cap: the call is exactly nnop_fa_fwd_sinks / nnop_fa_bwd_sinks (the same kernels, bitwise the same results).
 * A negative, NaN or infinite softcap is NNOP_ERR_OPTS.  Checks: the descriptor, the options, the cap, NULL pointers, alignment, in
 * that order.  The forward and the backward of one problem take the same cap.  A cap needs no extra workspace
 * (nnop_fa_bwd_workspace_bytes(_pair) are unchanged); with a cap and a pair bias the backward always takes the direct path, whatever
 * `workspace_bytes` is (as with a window).
 */
int nnop_fa_fwd_softcap(const nnop_fa_desc* d, const nnop_fa_opts* opts, const float* sinks, float softcap,
                        void* o, void* ms, void* ls,
                        const void* q, const void* k, const void* v,
                        const void* pair, const uint8_t* kpad_mask,
                        nnop_stream_t stream);

/*
 * Scratch the backward needs (replaces the reference's internal Δ_scaled / δ temporaries,
 * src/attention_bwd.jl:224-225).  Returns 0 for an invalid descriptor.
 */
size_t nnop_fa_bwd_workspace_bytes(const nnop_fa_desc* d);

/*
 * The same for a call WITH a pair bias (ABI version 5).  `pair` / `dpair` are [B][KL][QL][QH] with the head fastest
 * (src/attention.jl:62): per head their elements are QH apart, which a (batch, head) kernel can only touch one element per
 * lane.  Given this much scratch -- the small workspace + two head-major bias-sized matrices (a copy of the bias, dS), padded to
 * multiples of 64 -- nnop_fa_bwd re-packs the bias once, runs its kernels on 16-byte accesses and unpacks dpair at the end
 * (bf16 E=64 L=2048 H=4 B=4: see DESIGN.md).  A caller that passes only nnop_fa_bwd_workspace_bytes() gets the same results
 * from the direct (slow) path; nnop_fa_bwd picks by `workspace_bytes`.  Returns 0 for an invalid descriptor.
 */
size_t nnop_fa_bwd_workspace_bytes_pair(const nnop_fa_desc* d);

/*
 * Backward: contract of NNop.∇flash_attention (src/attention_bwd.jl:199-275) + kernels
 * _flash_attention_bwd_preprocess! (:163-197) and _flash_attention_bwd! (:1-161).
 * Writes dq, dk, dv (fully overwritten -- the caller need not zero them) and, when `pair`
 * is non-NULL, dpair (which must then be non-NULL too).  `d_o` is the cotangent Δ.
 */
int nnop_fa_bwd(const nnop_fa_desc* d,
                void* dq, void* dk, void* dv, void* dpair,
                const void* d_o, const void* o, const void* ms, const void* ls,
                const void* q, const void* k, const void* v,
                const void* pair, const uint8_t* kpad_mask,
                void* workspace, size_t workspace_bytes,
                nnop_stream_t stream);
/* The same with per-call options (nnop_fa_opts above; NULL = none).  The forward and the backward of one problem take the
 * same options.  With a window and a pair bias the backward never uses the staged scratch of
 * nnop_fa_bwd_workspace_bytes_pair (it takes the direct path whatever `workspace_bytes` is). */
int nnop_fa_bwd_ex(const nnop_fa_desc* d, const nnop_fa_opts* opts,
                   void* dq, void* dk, void* dv, void* dpair,
                   const void* d_o, const void* o, const void* ms, const void* ls,
                   const void* q, const void* k, const void* v,
                   const void* pair, const uint8_t* kpad_mask,
                   void* workspace, size_t workspace_bytes,
                   nnop_stream_t stream);
/* The same with learned attention sinks (nnop_fa_fwd_sinks above; sinks == NULL: exactly nnop_fa_bwd_ex, dsinks ignored). */
int nnop_fa_bwd_sinks(const nnop_fa_desc* d, const nnop_fa_opts* opts, const float* sinks, float* dsinks,
                      void* dq, void* dk, void* dv, void* dpair,
                      const void* d_o, const void* o, const void* ms, const void* ls,
                      const void* q, const void* k, const void* v,
                      const void* pair, const uint8_t* kpad_mask,
                      void* workspace, size_t workspace_bytes,
                      nnop_stream_t stream);

/* The same with logit soft-capping (nnop_fa_fwd_softcap above; softcap == 0: exactly nnop_fa_bwd_sinks). */
int nnop_fa_bwd_softcap(const nnop_fa_desc* d, const nnop_fa_opts* opts, const float* sinks, float* dsinks, float softcap,
                        void* dq, void* dk, void* dv, void* dpair,
                        const void* d_o, const void* o, const void* ms, const void* ls,
                        const void* q, const void* k, const void* v,
                        const void* pair, const uint8_t* kpad_mask,
                        void* workspace, size_t workspace_bytes,
                        nnop_stream_t stream);

/*
 * Llama rotary embedding: contract of NNop._llama_rope(q, k, cos, sin; bwd)
 * (src/rope/llama_rope.jl:69-89) + kernel llama_rope! (:24-65).  For every row x of q and of k:
 *     out[i]       = x[i] * cos[i] - x[i + D/2] * (sin_sign * sin[i])
 *     out[i + D/2] = x[i + D/2] * cos[i] + x[i] * (sin_sign * sin[i])          i < D/2
 * with cos, sin indexed by (position, batch) and shared by all heads.  sin_sign = +1: llama_rope;
 * sin_sign = -1: the pullback ∇llama_rope applied to (dq, dk) (:92).  Out of place (the reference copies q, k and
 * rotates the copies, :75-76); q_out == q / k_out == k (in place) is allowed.
 *   q, q_out : [B][QH][L][D]    k, k_out : [B][KH][L][D]    cos, sin : [B][L][D] (only the first D/2 of a row are read)
 *   dtype: element type of q, k;  cs_dtype: element type of cos, sin -- NNOP_F32 (what LlamaRotaryEmbedding
 *   returns, :15-22) or the same as dtype.  D must be even.  The arithmetic is fp32, one rounding to T on store.
 */
typedef struct nnop_rope_desc {
    int32_t dtype;     /* nnop_dtype of q, k */
    int32_t cs_dtype;  /* nnop_dtype of cos, sin */
    int32_t dim;       /* D  = size(q,1) */
    int32_t seq;       /* L  = size(q,2) == size(k,2) */
    int32_t qh;        /* size(q,3) */
    int32_t kh;        /* size(k,3) */
    int32_t batch;     /* size(q,4) == size(k,4) */
} nnop_rope_desc;

int nnop_llama_rope(const nnop_rope_desc* d, void* q_out, void* k_out, const void* q, const void* k,
                    const void* cos, const void* sin, float sin_sign, nnop_stream_t stream);

/*
 * Online softmax: NNop.online_softmax(x) (src/softmax.jl:60-68, kernel
 * online_softmax! :19-58, reduction monoid MD / md_reduce :1-16 through @groupreduce, src/groupreduce.jl:13-43) and
 * its pullback ∇online_softmax(Δ, y) (src/softmax.jl:70-80).
 *   x, y, dy, dx : [batch][N]  == Julia matrix (N, batch); softmax along N (dims = 1 in Julia).
 *   y[b][:]  = exp(x[b][:] - max) / sum(exp(x[b][:] - max))
 *   dx[b][:] = y[b][:] * (dy[b][:] - sum(dy[b][:] * y[b][:]))
 * One element type T for all arrays (the reference: y = similar(x)); fp32 arithmetic, one rounding on store.
 * Any N >= 1; rows whose byte length is a multiple of 16 (and up to 16384 fp32 / 32768 16-bit elements) are
 * held in registers and touch HBM once.
 */
typedef struct nnop_softmax_desc {
    int32_t dtype;   /* nnop_dtype */
    int32_t n;       /* N = size(x,1) */
    int64_t batch;   /* size(x,2) */
} nnop_softmax_desc;

int nnop_online_softmax(const nnop_softmax_desc* d, void* y, const void* x, nnop_stream_t stream);
int nnop_online_softmax_bwd(const nnop_softmax_desc* d, void* dx, const void* dy, const void* y,
                            nnop_stream_t stream);

/*
 * RMSNorm and LayerNorm.
 *   NNop._rms_norm(x, w; ϵ, offset) -> (y, rms)                  src/rms_norm.jl:117-137 (kernel :3-38)
 *   NNop.∇rms_norm(Δ, rms, x, w; offset) -> (dx, dw)              src/rms_norm.jl:139-169 (kernel :43-115)
 *   NNop._layer_norm(x, w, b; ϵ) -> (y, μ, Σ)                     src/layer_norm.jl:150-170 (kernel :8-63)
 *   NNop.∇layer_norm(Δ, μ, Σ, x, w, b) -> (dx, dw, db)            src/layer_norm.jl:172-204 (kernel :65-148)
 * x, y, dy, dx : [n][emb] == Julia (emb, n), element type `dtype`;  w, b : [emb], element type `w_dtype`
 * (NNOP_F32 or the same as dtype);  rms, mu, sigma : fp32 [n] (the caches the reference keeps for the pullback:
 * rms = sigma = 1/sqrt(var + eps));  RMSNorm dw : fp32 [emb] (rms_norm.jl:146);  LayerNorm dw, db : `w_dtype` [emb]
 * (layer_norm.jl:179-180).  Any emb >= 1.  fp32 arithmetic, one rounding on store.
 * The pullbacks need caller-owned scratch of nnop_norm_bwd_workspace_bytes() (replaces the reference's
 * (n/4, emb) partial-sum arrays, rms_norm.jl:146, layer_norm.jl:179-180); dx, dw, db are fully overwritten.
 */
typedef struct nnop_norm_desc {
    int32_t dtype;     /* nnop_dtype of x, y, dy, dx */
    int32_t w_dtype;   /* nnop_dtype of w, b (and of LayerNorm's dw, db) */
    int32_t emb;       /* size(x,1) */
    int32_t reserved;  /* must be 0 */
    int64_t n;         /* size(x,2) */
} nnop_norm_desc;

int nnop_rms_norm(const nnop_norm_desc* d, void* y, float* rms, const void* x, const void* w,
                  float offset, float eps, nnop_stream_t stream);
int nnop_rms_norm_bwd(const nnop_norm_desc* d, void* dx, float* dw, const void* dy, const float* rms,
                      const void* x, const void* w, float offset,
                      void* workspace, size_t workspace_bytes, nnop_stream_t stream);
int nnop_layer_norm(const nnop_norm_desc* d, void* y, float* mu, float* sigma, const void* x, const void* w,
                    const void* b, float eps, nnop_stream_t stream);
int nnop_layer_norm_bwd(const nnop_norm_desc* d, void* dx, void* dw, void* db, const void* dy, const float* mu,
                        const float* sigma, const void* x, const void* w,
                        void* workspace, size_t workspace_bytes, nnop_stream_t stream);
/* layer_norm: 0 = RMSNorm pullback, 1 = LayerNorm pullback.  Returns 0 for an invalid descriptor. */
size_t nnop_norm_bwd_workspace_bytes(const nnop_norm_desc* d, int layer_norm);

/*
 * Residual add fused into RMSNorm / LayerNorm (no counterpart in the reference; the pre-norm block's `h = x + residual;
 * y = norm(h)` in one pass over memory: 4 row-sized arrays moved instead of 5 forward, 4 instead of 6 in the pullback).
 *   add_rms_norm(x, residual, w; ϵ, offset) -> (y, h, rms)        add_layer_norm(x, residual, w, b; ϵ) -> (y, h, μ, Σ)
 * Forward:  h = T(fp32(x) + fp32(residual)) -- one fp32 add, one rounding to the element type T -- is written out, and the
 * statistics and y are those of the plain operator applied to the ROUNDED h: rms / mu, sigma / y are what nnop_rms_norm /
 * nnop_layer_norm return for input h, so the pullback, which reads h from memory, sees exactly what the forward normalised.
 * x, residual, h, y : [n][emb] of `dtype`;  w, b, offset, eps, the statistics and the w_dtype rules: as for the plain operators
 * (same nnop_norm_desc, same validation).  h may be the same buffer as x or as residual (same base address: the in-place
 * update of the residual stream); partial overlap is undefined.  y must not overlap an input.
 * Pullback: dy is the cotangent of y, dh the cotangent of h (what the rest of the residual stream sends back; may be NULL).
 * ONE gradient dx is written, the gradient of x and of residual alike (they are equal):  dx = T(g + fp32(dh)), g being the
 * fp32, not yet rounded, input gradient the plain pullback computes from (dy, h, w, statistics) -- one rounding, not two.
 * dw (and db) are exactly the plain pullback's (fp32 [emb] for RMSNorm, `w_dtype` for LayerNorm; same partial rows, same
 * fixed-order fold, no atomics).  dh == NULL gives exactly the results of nnop_rms_norm_bwd / nnop_layer_norm_bwd on h.
 * dx may be the same buffer as dh (accumulate into the stream's gradient).  Workspace: nnop_norm_bwd_workspace_bytes().
 * Checks, in this order: descriptor, NULL pointers (dh exempt), workspace size.
 */
int nnop_add_rms_norm(const nnop_norm_desc* d, void* y, void* h, float* rms, const void* x, const void* residual,
                      const void* w, float offset, float eps, nnop_stream_t stream);
int nnop_add_rms_norm_bwd(const nnop_norm_desc* d, void* dx, float* dw, const void* dy, const void* dh /* may be NULL */,
                          const float* rms, const void* h, const void* w, float offset,
                          void* workspace, size_t workspace_bytes, nnop_stream_t stream);
int nnop_add_layer_norm(const nnop_norm_desc* d, void* y, void* h, float* mu, float* sigma, const void* x,
                        const void* residual, const void* w, const void* b, float eps, nnop_stream_t stream);
int nnop_add_layer_norm_bwd(const nnop_norm_desc* d, void* dx, void* dw, void* db, const void* dy,
                            const void* dh /* may be NULL */, const float* mu, const float* sigma, const void* h,
                            const void* w, void* workspace, size_t workspace_bytes, nnop_stream_t stream);

/*
 * Gated MLP activations (no counterpart in the reference): y = a(gate) * up, the element-wise step of a Llama / Gemma / gpt-oss MLP,
 * forward and pullback in one pass over memory each (3 row-sized arrays moved forward instead of the two-op form's 5; 5 in the pullback
 * instead of about 10).  fp32 arithmetic for every element type, one rounding on store.
 *   NNOP_GLU_SILU        a(g) = g sigma(g)                                                  SwiGLU (Llama, Mistral, Qwen)
 *   NNOP_GLU_GELU_TANH   a(g) = 0.5 g (1 + tanh(sqrt(2/pi) (g + 0.044715 g^3)))              GeGLU (Gemma)
 *   NNOP_GLU_GELU_ERF    a(g) = 0.5 g (1 + erf(g / sqrt 2))                                  GeGLU with the exact GELU
 *   NNOP_GLU_SWIGLU_OAI  g' = min(g, limit), u' = clamp(u, -limit, limit), y = g' sigma(alpha g') (u' + 1)      gpt-oss (alpha = 1.702, limit = 7)
 * Pullback: dgate = dy * up * a'(gate), dup = dy * a(gate); a and a' are recomputed from gate and up, nothing else is kept from the
 * forward.  SWIGLU_OAI: the gradient passes through a clamp where the input is inside or ON the bound (torch's convention), and is 0
 * outside; y and the gradients use u' + 1 and g'.  At large finite gates a and a' are finite and equal their limits (a = g, a' = 1 on
 * the positive side; 0 and 0 on the negative side).
 * Layouts (`ld` in elements):
 *   NNOP_GLU_SPLIT        gate, up : [rows] rows of n elements, ld >= n apart, ONE ld for both.  Two dense matrices: ld = n.  The halves
 *                         of a fused gate-up projection gu [rows][2n]: gate = gu, up = gu + n, ld = 2n -- no copy.  y, dy : dense [rows][n].
 *                         dgate, dup : strided like gate, up; the elements between n and ld of a row are never written.
 *   NNOP_GLU_INTERLEAVED  gate = gu[:, 0::2], up = gu[:, 1::2] of ONE array gu [rows][2n] (gpt-oss); ld must be 2n; `up` / `dup` must be NULL
 *                         and `gate` / `dgate` are gu / dgu, dgu in the same layout.  y, dy : dense [rows][n].
 * Aliasing that is allowed (element-wise safe; the same base address AND the same stride only): dgate may be gate, dup may be up, dgu may be
 * gu; in the split forward y may be gate or up when ld == n.  ANY other overlap between an output and another argument is undefined.
 * Every shape and alignment works: when all bases are 16-byte aligned and n and ld are multiples of 16 bytes' worth of elements the kernels
 * move 16 bytes per access, otherwise single elements (slower, never an error).
 * Checks, in this order, all before any device work: the descriptor -- NNOP_ERR_DTYPE; NNOP_ERR_OPTS for an unknown act or layout and, with
 * SWIGLU_OAI only (the fields are ignored otherwise), an alpha that is not finite or a limit that is not finite and positive; NNOP_ERR_SHAPE
 * for rows <= 0, n <= 0, reserved != 0, a split ld < n, an interleaved ld != 2n, or more work than one launch takes -- then NNOP_ERR_NULL for a
 * NULL pointer (and for a non-NULL up / dup with the interleaved layout), then NNOP_ERR_ALIGN for a base not aligned to the element size.
 * No workspace; asynchronous on the stream like every other entry point.
 */
typedef enum nnop_glu_act {
    NNOP_GLU_SILU       = 0,
    NNOP_GLU_GELU_TANH  = 1,
    NNOP_GLU_GELU_ERF   = 2,
    NNOP_GLU_SWIGLU_OAI = 3
} nnop_glu_act;
typedef enum nnop_glu_layout {
    NNOP_GLU_SPLIT       = 0,
    NNOP_GLU_INTERLEAVED = 1
} nnop_glu_layout;
typedef struct nnop_glu_desc {
    int32_t dtype;     /* nnop_dtype of every array */
    int32_t act;       /* nnop_glu_act */
    int32_t layout;    /* nnop_glu_layout */
    int32_t reserved;  /* must be 0 */
    int64_t rows;
    int64_t n;         /* row length of y (and of gate, up) */
    int64_t ld;        /* row stride of gate, up, dgate, dup in elements; interleaved: 2n */
    float   alpha;     /* SWIGLU_OAI only */
    float   limit;     /* SWIGLU_OAI only */
} nnop_glu_desc;

int nnop_glu(const nnop_glu_desc* d, void* y, const void* gate, const void* up /* NULL iff interleaved */, nnop_stream_t stream);
int nnop_glu_bwd(const nnop_glu_desc* d, void* dgate, void* dup /* NULL iff interleaved */, const void* dy,
                 const void* gate, const void* up /* NULL iff interleaved */, nnop_stream_t stream);

/*
 * Cross-entropy loss over the classes of a row (no counterpart in the reference): the loss over an LM head's logits, forward and
 * pullback in one pass over memory each.  The forward reads every logit once and writes 8 bytes per row; the pullback reads once and
 * writes once; nothing of size rows x n is kept in between (the row's log-sum-exp is).  fp32 arithmetic for every element type.
 * For a row x[0..n) with target t:
 *   z_j  = x_j, or c tanh(x_j / c) with softcap = c > 0 (Gemma-2's final-logit cap: c = 30)
 *   lse  = log sum_j exp(z_j),  p_j = exp(z_j - lse)
 *   loss = (1 - eps) (lse - z_t) + eps (lse - mean_j z_j) + zeta lse^2       eps = label_smoothing (torch's meaning), zeta = z_loss
 *   dx_j = g [ p_j (1 + 2 zeta lse) - (1 - eps) [j = t] - eps / n ] (1 - (z_j / c)^2)       g = dloss of the row; the last factor is 1
 *                                                                                           without a cap
 * Special rows.  Stored target == ignore_index (compared before index_base is subtracted): loss = 0, lse is written, dx = 0 (written).
 * Any other target outside [0, n) after index_base is subtracted: loss = NaN and the whole dx row is NaN; the bad index is never turned
 * into an address, no other row is affected, and nothing asserts, traps or synchronises.  -inf logits have p = 0 and gradient 0; a row
 * that is all -inf gives NaN, a -inf at the target gives +inf loss.
 * logits : [rows] rows of n elements, ld >= n apart; dlogits likewise with ld_grad; the elements [n, ld_grad) of a dlogits row are never
 * written.  dlogits may be logits itself (same base, ld_grad == ld): the in-place gradient; any other overlap is undefined.
 * Every shape and alignment works: rows whose start is not 16-byte aligned (odd ld, an offset base) take element accesses.
 * Checks, in this order, all before any device work: NNOP_ERR_DTYPE; NNOP_ERR_OPTS for index_bytes not 4 / 8, index_base not 0 / 1, a
 * reserved field not 0, label_smoothing outside [0, 1], a z_loss or softcap that is NaN, infinite or negative; NNOP_ERR_SHAPE for
 * rows <= 0, n <= 0, ld < n, ld_grad < n (pullback only), n or rows above 2^31 - 1; NNOP_ERR_NULL; NNOP_ERR_ALIGN for logits / dlogits
 * not aligned to the element size, loss / lse / dloss to 4 bytes, targets to index_bytes.
 * No workspace; asynchronous on the stream like every other entry point.
 */
typedef struct nnop_xent_desc {
    int32_t dtype;          /* nnop_dtype of logits and dlogits */
    int32_t index_bytes;    /* 4 or 8: int32 / int64 targets */
    int64_t rows, n;        /* tokens, classes */
    int64_t ld, ld_grad;    /* row strides in elements of logits / dlogits, each >= n (ld_grad is read by _bwd only) */
    int64_t ignore_index;   /* compared with the stored target value, before index_base is subtracted */
    int32_t index_base;     /* 0 (C, torch) or 1 (Julia) */
    int32_t reserved;       /* 0 */
    float   label_smoothing;/* [0, 1] */
    float   z_loss;         /* finite, >= 0 */
    float   softcap;        /* 0 = none, else finite and > 0 */
    float   reserved_f;     /* 0 */
} nnop_xent_desc;

int nnop_cross_entropy(const nnop_xent_desc* d, float* loss /* [rows] */, float* lse /* [rows] */, const void* logits,
                       const void* targets, nnop_stream_t stream);
int nnop_cross_entropy_bwd(const nnop_xent_desc* d, void* dlogits, const float* dloss /* [rows] */, const float* lse,
                           const void* logits, const void* targets, nnop_stream_t stream);

/*
 * Sharding over several devices (ABI version 6).  The reference has no multi-GPU code; its (batch, kv-head) slices -- a KV head with its
 * QH / KH query heads -- are independent in forward and backward (src/attention.jl:27-28,33; src/attention_bwd.jl:28-29,34), so a host
 * that owns several devices gives rank g of `world` the contiguous unit range [g U / world, (g+1) U / world), U = batch * kh, units
 * numbered u = b * kh + h (batch slowest, as in memory).  In the [B][H][L][E] layout that range is at most three DENSE rectangles
 * (tail of the first batch, whole batches, head of the last batch); each is a problem of its own for nnop_fa_fwd / nnop_fa_bwd at the
 * element offsets below -- pointer arithmetic only, no copies, no collective.  Host-only: touches no device.
 * Returns the number of rectangles written to `out` (0..3), or a negative nnop_status for an invalid descriptor / world / rank.
 * Rectangles split only batch and heads, never the sequence axes: a caller with per-call options (nnop_fa_opts, e.g. a window)
 * passes the same options to nnop_fa_fwd_ex / nnop_fa_bwd_ex of every rectangle.
 */
typedef struct nnop_fa_shard {
    nnop_fa_desc desc;   /* the rectangle as a problem: batch, qh, kh replaced; everything else as in the full problem */
    int32_t  b0, b1;     /* batches  [b0, b1)  of the full problem */
    int32_t  kh0, kh1;   /* kv heads [kh0, kh1) (query heads [kh0, kh1) * qh / kh) */
    uint64_t q_off;      /* ELEMENT offset of the rectangle in q, o, dO, dq   ([B][QH][QL][E]) */
    uint64_t kv_off;     /* ... in k, v, dk, dv                               ([B][KH][KL][E]) */
    uint64_t row_off;    /* ... in ms, ls                                     ([B][QH][QL])    */
    uint64_t mask_off;   /* BYTE offset in kpad_mask                          ([B][KL])        */
    int64_t  pair_off;   /* element offset in pair / dpair ([B][KL][QL][QH]) when the rectangle holds ALL heads of its batches;
                            -1 otherwise: part of a batch's heads is not a dense sub-array of the head-fastest bias layout (the caller
                            then hands that rectangle a head-sliced copy, or shards whole batches: world <= batch) */
} nnop_fa_shard;
int nnop_fa_shards(const nnop_fa_desc* d, int world, int rank, nnop_fa_shard out[3]);

/* NNop._shared_memory(::ROCBackend, device_id) (ext/NNopAMDGPUExt.jl:6-9):
 * hipDeviceProp_t.sharedMemPerBlock of `device` (0-based HIP ordinal). */
int nnop_shared_memory(int device, uint64_t* bytes);

/* Human-readable text for an nnop_status (static storage; never NULL). */
const char* nnop_strerror(int status);

/* ABI version of this header: bumped on any incompatible change. */
#define NNOP_HIP_ABI_VERSION 7
int nnop_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* NNOP_HIP_H */
