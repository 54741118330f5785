// nnop_capi.cpp -- the extern "C" boundary declared in include/nnop_hip.h.
//
// Mirrors the host side of the reference operator: the four argument checks of
// `_flash_attention` / `∇flash_attention` (src/attention.jl:141-144, src/attention_bwd.jl:210-213)
// become status codes; allocation of outputs and scratch moves to the caller; the launch is
// asynchronous on the caller's stream (src/attention.jl:170-176 never synchronises either).
#include "fa_launch.hpp"
#include "host_common.hpp"
#include "nnop_debug.h"
#include "tuning.hpp"
#include <limits.h>
#include <stdlib.h>
#include <mutex>

namespace nnop {

// ---- launch-shape overrides (tuning.hpp): environment parsed once, then a table of ints ------------
static int g_tune[kTuneCount];
static int g_debug_hooks = 0;                                // NNOP_DEBUG_HOOKS=1 in the environment at the first launch: nnop_debug_set works
static std::once_flag g_tune_once;
static void tune_init() {
    static const char* const names[kTuneCount] = {"NNOP_FWD_SPLIT", "NNOP_FWD_NW",       "NNOP_FWD_W64",
                                                  "NNOP_BWD_BIG7",  "NNOP_NORM_BWD_CAP", "NNOP_BWD_NW",
                                                  "NNOP_FWD_EXACT_SCALE", "NNOP_BWD_W64", nullptr, "NNOP_FWD_PERSIST", "NNOP_BWD_PERSIST",
                                                  "NNOP_FWD_DUO", "NNOP_FWD_PERSIST_ASC", "NNOP_BWD_NARROW", "NNOP_FWD_CAUSAL_ALT"};
    // (kTuneBwdStages has no environment variable: it makes the backward INCOMPLETE -- a measurement aid that only the test hook
    // nnop_debug_set can switch on, csrc/nnop_debug.h)
    for (int k = 0; k < kTuneCount; ++k) {
        const char* s = names[k] ? getenv(names[k]) : nullptr;
        __atomic_store_n(&g_tune[k], (s && *s) ? atoi(s) : -1, __ATOMIC_RELAXED);
    }
    const char* h = getenv("NNOP_DEBUG_HOOKS");
    __atomic_store_n(&g_debug_hooks, (h && *h && atoi(h) != 0) ? 1 : 0, __ATOMIC_RELAXED);
}
int tune_get(int key) {
    std::call_once(g_tune_once, tune_init);
    return __atomic_load_n(&g_tune[key], __ATOMIC_RELAXED);
}

static int check_desc(const nnop_fa_desc* d) {
    if (!d) return NNOP_ERR_NULL;
    if (!known_dtype(d->dtype)) return NNOP_ERR_DTYPE;
    if (d->emb <= 0 || d->ql <= 0 || d->kl <= 0 || d->qh <= 0 || d->kh <= 0 || d->batch <= 0) return NNOP_ERR_SHAPE;
    const int emb_k = d->emb_k ? d->emb_k : d->emb;
    const int emb_v = d->emb_v ? d->emb_v : emb_k;
    const int kl_v  = d->kl_v ? d->kl_v : d->kl;
    const int kh_v  = d->kh_v ? d->kh_v : d->kh;
    // order of the reference's checks, src/attention.jl:141-144
    if (d->emb != emb_k) return NNOP_ERR_EMB_MISMATCH;
    if (emb_v != emb_k || kl_v != d->kl || kh_v != d->kh) return NNOP_ERR_KV_SHAPE;
    if ((d->emb & (d->emb - 1)) != 0) return NNOP_ERR_EMB_NOT_POW2;
    if (d->qh % d->kh != 0) return NNOP_ERR_HEADS;
    if (!emb_supported(d->emb)) return NNOP_ERR_EMB_UNSUPPORTED;
    // index arithmetic inside the kernels is 32-bit per (batch, head) slice
    if ((long long)d->ql * d->emb > 0x7fffffffLL || (long long)d->kl * d->emb > 0x7fffffffLL) return NNOP_ERR_SHAPE;
    return NNOP_OK;
}
// Base alignment (NNOP_ERR_ALIGN): the MFMA kernels move q, k, v, o, the gradients and the workspace with 16-byte vector
// accesses and LDS-DMA from the raw base; the plain-HIP kernels (embedding dims outside the tiled set) access single elements.
// pair / dpair need the element size only: the forward and the direct backward path gather the bias element by element, the staged
// path's pack / unpack kernels take 16-byte vectors only from a 16-byte aligned base (pair_tile.hpp), and a batch slice of a bias
// (nnop_fa_shards: pair_off = b0 * KL * QL * QH elements) starts at any element.
// The optional arguments (pair, dpair, sinks, dsinks) go through `misaligned` as they are: NULL counts as aligned.
static inline size_t tensor_align(const nnop_fa_desc* d) {
    const bool tiled = emb_tiled(d->emb) || d->emb == 256;
    return tiled ? 16 : dtype_bytes(d->dtype);
}
// per-call options (checked after check_desc, whose order is the reference's)
static int check_opts(const nnop_fa_opts* o) {
    if (!o) return NNOP_OK;
    for (int i = 0; i < 6; ++i)
        if (o->reserved[i] != 0) return NNOP_ERR_OPTS;
    if (o->window_left < -1 || o->window_right < -1) return NNOP_ERR_OPTS;
    return NNOP_OK;
}
// logit soft-capping (checked after the options): 0 = none, else finite and positive
static int check_softcap(float c) { return finite_nonneg(c) ? NNOP_OK : NNOP_ERR_OPTS; }
// pair / dpair [B][KL][QL][QH]: inside one kv tile the kernels address the bias with 32-bit element offsets
// (local key < 64) * QL * QH
static int check_pair(const nnop_fa_desc* d) {
    return ((long long)d->ql * d->qh * 64 > 0x7fffffffLL) ? NNOP_ERR_SHAPE : NNOP_OK;
}
}  // namespace nnop

using namespace nnop;

extern "C" {

int nnop_abi_version(void) { return NNOP_HIP_ABI_VERSION; }

// test-only hooks, declared in csrc/nnop_debug.h (not in the public header)
int nnop_debug_set(int key, int value) {
    if (key < 0 || key >= kTuneCount) return INT_MIN;
    (void)tune_get(key);                                   // make sure the environment has been parsed first
    // LOCKED unless the process started with NNOP_DEBUG_HOOKS=1 (the test-suite and bench.py's per-kernel leg do): a host that merely
    // links the library cannot flip process-wide kernel selection -- or, through bwd_stages, make nnop_fa_bwd skip passes
    if (!__atomic_load_n(&g_debug_hooks, __ATOMIC_RELAXED)) return INT_MIN;
    return __atomic_exchange_n(&g_tune[key], value, __ATOMIC_RELAXED);
}
// (one body per direction, the _cap one: the narrower hooks are it without a cap / without options, as nnop_fa_fwd is nnop_fa_fwd_softcap)
int nnop_debug_fwd_form(const nnop_fa_desc* d, int has_pair, int has_mask) {
    return nnop_debug_fwd_form_cap(d, nullptr, 0.f, has_pair, has_mask);
}
int nnop_debug_bwd_form(const nnop_fa_desc* d, int has_pair, int has_mask) {
    return nnop_debug_bwd_form_cap(d, nullptr, 0.f, has_pair, has_mask);
}
int nnop_debug_fwd_form_ex(const nnop_fa_desc* d, const nnop_fa_opts* opts, int has_pair, int has_mask) {
    return nnop_debug_fwd_form_cap(d, opts, 0.f, has_pair, has_mask);
}
int nnop_debug_bwd_form_ex(const nnop_fa_desc* d, const nnop_fa_opts* opts, int has_pair, int has_mask) {
    return nnop_debug_bwd_form_cap(d, opts, 0.f, has_pair, has_mask);
}
int nnop_debug_fwd_form_cap(const nnop_fa_desc* d, const nnop_fa_opts* opts, float softcap, int has_pair, int has_mask) {
    int st = check_desc(d);
    if (st == NNOP_OK) st = check_opts(opts);
    if (st == NNOP_OK) st = check_softcap(softcap);
    if (st != NNOP_OK) return st;
    return fwd_form(*d, has_pair != 0, has_mask != 0, fa_window(*d, opts).on(), softcap != 0.f);
}
int nnop_debug_bwd_form_cap(const nnop_fa_desc* d, const nnop_fa_opts* opts, float softcap, int has_pair, int) {
    int st = check_desc(d);
    if (st == NNOP_OK) st = check_opts(opts);
    if (st == NNOP_OK) st = check_softcap(softcap);
    if (st != NNOP_OK) return st;
    return bwd_forms(*d, has_pair != 0, fa_window(*d, opts).on(), softcap != 0.f);
}
int nnop_debug_dev_build(void) {
#ifdef NNOP_DEV_BUILD
    return 1;
#else
    return 0;
#endif
}

const char* nnop_strerror(int status) {
    switch (status) {
        case NNOP_OK: return "success";
        case NNOP_ERR_EMB_MISMATCH: return "Embedding dim of Q must be the same as of K.";
        case NNOP_ERR_KV_SHAPE: return "Shapes of K and V must be the same.";
        case NNOP_ERR_EMB_NOT_POW2: return "Only power-of-2 embedding dims are supported.";
        case NNOP_ERR_HEADS: return "Number of query heads must be divisible by number of KV heads.";
        case NNOP_ERR_DTYPE: return "Unsupported element type (expected Float32, Float16 or BFloat16).";
        case NNOP_ERR_NULL: return "A required pointer argument is NULL.";
        case NNOP_ERR_EMB_UNSUPPORTED:
            return "Failed to find a Flash Attention tile configuration for this embedding dim (supported: the powers of two 1 ... 512).";
        case NNOP_ERR_SHAPE: return "A dimension is non-positive or too large.";
        case NNOP_ERR_WORKSPACE: return "Backward workspace is smaller than nnop_*_bwd_workspace_bytes().";
        case NNOP_ERR_HIP: return "HIP runtime error at kernel launch.";
        case NNOP_ERR_ALIGN:
            return "A tensor or workspace base address is misaligned (16 bytes for q, k, v, o, dq, dk, dv and workspace; the element size for pair, dpair, ms, ls "
                   "and for the arrays of nnop_glu; nnop_cross_entropy: the element size for logits and dlogits, 4 bytes for loss, lse and dloss, "
                   "index_bytes for targets).";
        case NNOP_ERR_OPTS:
            return "Invalid options (attention: a reserved field is not 0, a window side is below -1, or a soft cap is negative or not finite; "
                   "nnop_glu: an unknown act or layout, or with swiglu_oai an alpha that is not finite or a limit that is not finite and positive; "
                   "nnop_cross_entropy: index_bytes not 4 or 8, index_base not 0 or 1, a reserved field not 0, label_smoothing outside [0, 1], "
                   "or a z_loss or softcap that is negative or not finite).";
        default: return "unknown nnop status";
    }
}

int nnop_fa_shards(const nnop_fa_desc* d, int world, int rank, nnop_fa_shard out[3]) {
    const int st = check_desc(d);
    if (st != NNOP_OK) return st;
    if (!out) return NNOP_ERR_NULL;
    if (world <= 0 || rank < 0 || rank >= world) return NNOP_ERR_SHAPE;
    const long long units = (long long)d->batch * d->kh;
    const long long lo = units * rank / world, hi = units * (rank + 1) / world;
    const int rep = d->qh / d->kh;
    int n = 0;
    long long u = lo;
    while (u < hi && n < 3) {
        const int b = (int)(u / d->kh), kh = (int)(u % d->kh);
        nnop_fa_shard& r = out[n++];
        r.desc = *d;
        if (kh == 0 && hi - u >= d->kh) {                  // whole batches
            const int nb = (int)((hi - u) / d->kh);
            r.b0 = b; r.b1 = b + nb; r.kh0 = 0; r.kh1 = d->kh;
            u += (long long)nb * d->kh;
        } else {                                           // part of one batch
            const long long left = hi - u;
            const int kh1 = (int)(kh + left < d->kh ? kh + left : d->kh);
            r.b0 = b; r.b1 = b + 1; r.kh0 = kh; r.kh1 = kh1;
            u += kh1 - kh;
        }
        r.desc.batch = r.b1 - r.b0;
        r.desc.kh = r.kh1 - r.kh0;
        r.desc.qh = r.desc.kh * rep;
        r.desc.kh_v = 0;
        const uint64_t qhead = (uint64_t)r.b0 * d->qh + (uint64_t)r.kh0 * rep, kvhead = (uint64_t)r.b0 * d->kh + r.kh0;
        r.q_off = qhead * d->ql * d->emb;
        r.kv_off = kvhead * d->kl * d->emb;
        r.row_off = qhead * d->ql;
        r.mask_off = (uint64_t)r.b0 * d->kl;
        r.pair_off = (r.kh0 == 0 && r.kh1 == d->kh) ? (int64_t)((uint64_t)r.b0 * d->kl * d->ql * d->qh) : -1;
    }
    return n;
}

int nnop_shared_memory(int device, uint64_t* bytes) {
    if (!bytes) return NNOP_ERR_NULL;
    int v = 0;
    // hipDeviceProp_t.sharedMemPerBlock, as ext/NNopAMDGPUExt.jl:6-9 reads it
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, device) != hipSuccess) {
        (void)hipGetLastError();
        return NNOP_ERR_HIP;
    }
    *bytes = (uint64_t)v;
    return NNOP_OK;
}

int nnop_fa_fwd(const nnop_fa_desc* d, void* o, void* ms, void* ls, const void* q, const void* k,
                const void* v, const void* pair, const uint8_t* kpad_mask, nnop_stream_t stream) {
    return nnop_fa_fwd_ex(d, nullptr, o, ms, ls, q, k, v, pair, kpad_mask, stream);
}

int nnop_fa_fwd_ex(const nnop_fa_desc* d, const nnop_fa_opts* opts, void* o, void* ms, void* ls, const void* q, const void* k,
                   const void* v, const void* pair, const uint8_t* kpad_mask, nnop_stream_t stream) {
    return nnop_fa_fwd_sinks(d, opts, nullptr, o, ms, ls, q, k, v, pair, kpad_mask, stream);
}

int nnop_fa_fwd_sinks(const nnop_fa_desc* d, const nnop_fa_opts* opts, const float* sinks, void* o, void* ms, void* ls,
                      const void* q, const void* k, const void* v, const void* pair, const uint8_t* kpad_mask,
                      nnop_stream_t stream) {
    return nnop_fa_fwd_softcap(d, opts, sinks, 0.f, o, ms, ls, q, k, v, pair, kpad_mask, stream);
}

int nnop_fa_fwd_softcap(const nnop_fa_desc* d, const nnop_fa_opts* opts, const float* sinks, float softcap, void* o, void* ms,
                        void* ls, const void* q, const void* k, const void* v, const void* pair, const uint8_t* kpad_mask,
                        nnop_stream_t stream) {
    int st = check_desc(d);
    if (st == NNOP_OK) st = check_opts(opts);
    if (st == NNOP_OK) st = check_softcap(softcap);
    if (st != NNOP_OK) return st;
    if (!o || !ms || !ls || !q || !k || !v) return NNOP_ERR_NULL;
    if (pair && check_pair(d) != NNOP_OK) return NNOP_ERR_SHAPE;
    {
        const size_t ta = tensor_align(d), ea = dtype_bytes(d->dtype);
        if (misaligned(o, ta) || misaligned(q, ta) || misaligned(k, ta) || misaligned(v, ta) || misaligned(pair, ea) ||
            misaligned(ms, ea) || misaligned(ls, ea) || misaligned(sinks, sizeof(float)))
            return NNOP_ERR_ALIGN;
    }
    FwdArgs a{o, ms, ls, q, k, v, pair, kpad_mask, fa_window(*d, opts), sinks, softcap};
    hipStream_t s = (hipStream_t)stream;
    return dispatch_dtype(d->dtype, [&](auto t) { return launch_fwd<typename decltype(t)::type>(*d, a, s); });
}

int nnop_llama_rope(const nnop_rope_desc* d, void* q_out, void* k_out, const void* q, const void* k,
                    const void* cos, const void* sin, float sin_sign, nnop_stream_t stream) {
    if (!d) return NNOP_ERR_NULL;
    if (!known_dtype(d->dtype)) return NNOP_ERR_DTYPE;
    if (d->cs_dtype != NNOP_F32 && d->cs_dtype != d->dtype) return NNOP_ERR_DTYPE;
    if (d->dim <= 0 || (d->dim & 1) || d->seq <= 0 || d->qh <= 0 || d->kh <= 0 || d->batch <= 0) return NNOP_ERR_SHAPE;
    if (!q_out || !k_out || !q || !k || !cos || !sin) return NNOP_ERR_NULL;
    return launch_rope(*d, q_out, k_out, q, k, cos, sin, sin_sign, (hipStream_t)stream);
}

static int check_softmax(const nnop_softmax_desc* d) {
    if (!d) return NNOP_ERR_NULL;
    if (!known_dtype(d->dtype)) return NNOP_ERR_DTYPE;
    if (d->n <= 0 || d->batch <= 0) return NNOP_ERR_SHAPE;
    return NNOP_OK;
}

int nnop_online_softmax(const nnop_softmax_desc* d, void* y, const void* x, nnop_stream_t stream) {
    const int st = check_softmax(d);
    if (st != NNOP_OK) return st;
    if (!y || !x) return NNOP_ERR_NULL;
    return launch_softmax(*d, y, x, nullptr, false, (hipStream_t)stream);
}

int nnop_online_softmax_bwd(const nnop_softmax_desc* d, void* dx, const void* dy, const void* y,
                            nnop_stream_t stream) {
    const int st = check_softmax(d);
    if (st != NNOP_OK) return st;
    if (!dx || !dy || !y) return NNOP_ERR_NULL;
    return launch_softmax(*d, dx, dy, y, true, (hipStream_t)stream);
}

static int check_norm(const nnop_norm_desc* d) {
    if (!d) return NNOP_ERR_NULL;
    if (!known_dtype(d->dtype)) return NNOP_ERR_DTYPE;
    if (d->w_dtype != NNOP_F32 && d->w_dtype != d->dtype) return NNOP_ERR_DTYPE;
    if (d->emb <= 0 || d->n <= 0 || d->n > 0x7fffffffLL || d->reserved != 0) return NNOP_ERR_SHAPE;
    return NNOP_OK;
}

int nnop_rms_norm(const nnop_norm_desc* d, void* y, float* rms, const void* x, const void* w, float offset, float eps,
                  nnop_stream_t stream) {
    const int st = check_norm(d);
    if (st != NNOP_OK) return st;
    if (!y || !rms || !x || !w) return NNOP_ERR_NULL;
    return launch_rms_norm(*d, y, rms, x, w, offset, eps, (hipStream_t)stream);
}

int nnop_rms_norm_bwd(const nnop_norm_desc* d, void* dx, float* dw, const void* dy, const float* rms, const void* x,
                      const void* w, float offset, void* workspace, size_t workspace_bytes, nnop_stream_t stream) {
    const int st = check_norm(d);
    if (st != NNOP_OK) return st;
    if (!dx || !dw || !dy || !rms || !x || !w || !workspace) return NNOP_ERR_NULL;
    if (workspace_bytes < norm_ws_bytes(*d, false)) return NNOP_ERR_WORKSPACE;
    return launch_rms_norm_bwd(*d, dx, dw, dy, rms, x, w, offset, workspace, (hipStream_t)stream);
}

int nnop_layer_norm(const nnop_norm_desc* d, void* y, float* mu, float* sigma, const void* x, const void* w,
                    const void* b, float eps, nnop_stream_t stream) {
    const int st = check_norm(d);
    if (st != NNOP_OK) return st;
    if (!y || !mu || !sigma || !x || !w || !b) return NNOP_ERR_NULL;
    return launch_layer_norm(*d, y, mu, sigma, x, w, b, eps, (hipStream_t)stream);
}

int nnop_layer_norm_bwd(const nnop_norm_desc* d, void* dx, void* dw, void* db, const void* dy, const float* mu,
                        const float* sigma, const void* x, const void* w, void* workspace, size_t workspace_bytes,
                        nnop_stream_t stream) {
    const int st = check_norm(d);
    if (st != NNOP_OK) return st;
    if (!dx || !dw || !db || !dy || !mu || !sigma || !x || !w || !workspace) return NNOP_ERR_NULL;
    if (workspace_bytes < norm_ws_bytes(*d, true)) return NNOP_ERR_WORKSPACE;
    return launch_layer_norm_bwd(*d, dx, dw, db, dy, mu, sigma, x, w, workspace, (hipStream_t)stream);
}

int nnop_add_rms_norm(const nnop_norm_desc* d, void* y, void* h, float* rms, const void* x, const void* residual,
                      const void* w, float offset, float eps, nnop_stream_t stream) {
    const int st = check_norm(d);
    if (st != NNOP_OK) return st;
    if (!y || !h || !rms || !x || !residual || !w) return NNOP_ERR_NULL;
    return launch_add_rms_norm(*d, y, h, rms, x, residual, w, offset, eps, (hipStream_t)stream);
}

int nnop_add_rms_norm_bwd(const nnop_norm_desc* d, void* dx, float* dw, const void* dy, const void* dh, const float* rms,
                          const void* h, const void* w, float offset, void* workspace, size_t workspace_bytes,
                          nnop_stream_t stream) {
    const int st = check_norm(d);
    if (st != NNOP_OK) return st;
    if (!dx || !dw || !dy || !rms || !h || !w || !workspace) return NNOP_ERR_NULL;      // dh may be NULL
    if (workspace_bytes < norm_ws_bytes(*d, false)) return NNOP_ERR_WORKSPACE;
    return launch_add_rms_norm_bwd(*d, dx, dw, dy, dh, rms, h, w, offset, workspace, (hipStream_t)stream);
}

int nnop_add_layer_norm(const nnop_norm_desc* d, void* y, void* h, float* mu, float* sigma, const void* x,
                        const void* residual, const void* w, const void* b, float eps, nnop_stream_t stream) {
    const int st = check_norm(d);
    if (st != NNOP_OK) return st;
    if (!y || !h || !mu || !sigma || !x || !residual || !w || !b) return NNOP_ERR_NULL;
    return launch_add_layer_norm(*d, y, h, mu, sigma, x, residual, w, b, eps, (hipStream_t)stream);
}

int nnop_add_layer_norm_bwd(const nnop_norm_desc* d, void* dx, void* dw, void* db, const void* dy, const void* dh,
                            const float* mu, const float* sigma, const void* h, const void* w, void* workspace,
                            size_t workspace_bytes, nnop_stream_t stream) {
    const int st = check_norm(d);
    if (st != NNOP_OK) return st;
    if (!dx || !dw || !db || !dy || !mu || !sigma || !h || !w || !workspace) return NNOP_ERR_NULL;   // dh may be NULL
    if (workspace_bytes < norm_ws_bytes(*d, true)) return NNOP_ERR_WORKSPACE;
    return launch_add_layer_norm_bwd(*d, dx, dw, db, dy, dh, mu, sigma, h, w, workspace, (hipStream_t)stream);
}

// descriptor, then pointers, then alignment; `ptrs`: the arguments that must be non-NULL, `absent`: those that the interleaved
// layout forbids (up, dup)
static int check_glu(const nnop_glu_desc* d, std::initializer_list<const void*> ptrs, std::initializer_list<const void*> absent) {
    if (!d) return NNOP_ERR_NULL;
    if (!known_dtype(d->dtype)) return NNOP_ERR_DTYPE;
    if (d->act < NNOP_GLU_SILU || d->act > NNOP_GLU_SWIGLU_OAI) return NNOP_ERR_OPTS;
    if (d->layout != NNOP_GLU_SPLIT && d->layout != NNOP_GLU_INTERLEAVED) return NNOP_ERR_OPTS;
    if (d->act == NNOP_GLU_SWIGLU_OAI && !(finite(d->alpha) && finite(d->limit) && d->limit > 0.f)) return NNOP_ERR_OPTS;
    if (d->rows <= 0 || d->n <= 0 || d->reserved != 0) return NNOP_ERR_SHAPE;
    const bool il = d->layout == NNOP_GLU_INTERLEAVED;
    if (il ? (d->n > LLONG_MAX / 2 || d->ld != 2 * d->n) : d->ld < d->n) return NNOP_ERR_SHAPE;
    const size_t ea = dtype_bytes(d->dtype);
    const int st = check_ptrs({{ptrs, ea}}, [&] {
        for (const void* q : absent)
            if (il ? q != nullptr : q == nullptr) return NNOP_ERR_NULL;
        return NNOP_OK;
    });
    if (st != NNOP_OK) return st;
    for (const void* q : absent)
        if (misaligned(q, ea)) return NNOP_ERR_ALIGN;
    return NNOP_OK;
}

int nnop_glu(const nnop_glu_desc* d, void* y, const void* gate, const void* up, nnop_stream_t stream) {
    const int st = check_glu(d, {y, gate}, {up});
    if (st != NNOP_OK) return st;
    return launch_glu(*d, y, gate, up, (hipStream_t)stream);
}

int nnop_glu_bwd(const nnop_glu_desc* d, void* dgate, void* dup, const void* dy, const void* gate, const void* up,
                 nnop_stream_t stream) {
    const int st = check_glu(d, {dgate, dy, gate}, {dup, up});
    if (st != NNOP_OK) return st;
    return launch_glu_bwd(*d, dgate, dup, dy, gate, up, (hipStream_t)stream);
}

// descriptor (dtype, options, shape), then pointers, then alignment; `elems`: logits / dlogits (element size), `f32s`: loss, lse, dloss
static int check_xent(const nnop_xent_desc* d, bool bwd, std::initializer_list<const void*> elems,
                      std::initializer_list<const void*> f32s, const void* targets) {
    if (!d) return NNOP_ERR_NULL;
    if (!known_dtype(d->dtype)) return NNOP_ERR_DTYPE;
    if (d->index_bytes != 4 && d->index_bytes != 8) return NNOP_ERR_OPTS;
    if (d->index_base != 0 && d->index_base != 1) return NNOP_ERR_OPTS;
    if (d->reserved != 0 || !(d->reserved_f == 0.f)) return NNOP_ERR_OPTS;
    if (!(d->label_smoothing >= 0.f && d->label_smoothing <= 1.f)) return NNOP_ERR_OPTS;      // (the comparisons are false for NaN)
    if (!finite_nonneg(d->z_loss) || !finite_nonneg(d->softcap)) return NNOP_ERR_OPTS;
    if (d->rows <= 0 || d->n <= 0 || d->ld < d->n || (bwd && d->ld_grad < d->n)) return NNOP_ERR_SHAPE;
    if (d->n > 0x7fffffffLL || d->rows > 0x7fffffffLL) return NNOP_ERR_SHAPE;
    return check_ptrs({{elems, dtype_bytes(d->dtype)}, {f32s, sizeof(float)}, {{targets}, (size_t)d->index_bytes}});
}

int nnop_cross_entropy(const nnop_xent_desc* d, float* loss, float* lse, const void* logits, const void* targets,
                       nnop_stream_t stream) {
    const int st = check_xent(d, false, {logits}, {loss, lse}, targets);
    if (st != NNOP_OK) return st;
    return launch_xent(*d, loss, lse, logits, targets, (hipStream_t)stream);
}

int nnop_cross_entropy_bwd(const nnop_xent_desc* d, void* dlogits, const float* dloss, const float* lse, const void* logits,
                           const void* targets, nnop_stream_t stream) {
    const int st = check_xent(d, true, {dlogits, logits}, {dloss, lse}, targets);
    if (st != NNOP_OK) return st;
    return launch_xent_bwd(*d, dlogits, dloss, lse, logits, targets, (hipStream_t)stream);
}

size_t nnop_norm_bwd_workspace_bytes(const nnop_norm_desc* d, int layer_norm) {
    if (check_norm(d) != NNOP_OK) return 0;
    return norm_ws_bytes(*d, layer_norm != 0);
}

size_t nnop_fa_bwd_workspace_bytes(const nnop_fa_desc* d) {
    if (check_desc(d) != NNOP_OK) return 0;
    return bwd_workspace_bytes(*d);
}
size_t nnop_fa_bwd_workspace_bytes_pair(const nnop_fa_desc* d) {
    if (check_desc(d) != NNOP_OK || check_pair(d) != NNOP_OK) return 0;
    return bwd_workspace_bytes_pair(*d);
}

int nnop_fa_bwd(const nnop_fa_desc* d, void* dq, void* dk, void* dv, void* dpair, const void* d_o,
                const void* o, const void* ms, const void* ls, const void* q, const void* k,
                const void* v, const void* pair, const uint8_t* kpad_mask, void* workspace,
                size_t workspace_bytes, nnop_stream_t stream) {
    return nnop_fa_bwd_ex(d, nullptr, dq, dk, dv, dpair, d_o, o, ms, ls, q, k, v, pair, kpad_mask, workspace, workspace_bytes,
                          stream);
}

int nnop_fa_bwd_ex(const nnop_fa_desc* d, const nnop_fa_opts* opts, void* dq, void* dk, void* dv, void* dpair, const void* d_o,
                   const void* o, const void* ms, const void* ls, const void* q, const void* k, const void* v, const void* pair,
                   const uint8_t* kpad_mask, void* workspace, size_t workspace_bytes, nnop_stream_t stream) {
    return nnop_fa_bwd_sinks(d, opts, nullptr, nullptr, dq, dk, dv, dpair, d_o, o, ms, ls, q, k, v, pair, kpad_mask, workspace,
                             workspace_bytes, stream);
}

int nnop_fa_bwd_sinks(const nnop_fa_desc* d, const nnop_fa_opts* opts, const float* sinks, float* dsinks, void* dq, void* dk,
                      void* dv, void* dpair, const void* d_o, const void* o, const void* ms, const void* ls, const void* q,
                      const void* k, const void* v, const void* pair, const uint8_t* kpad_mask, void* workspace,
                      size_t workspace_bytes, nnop_stream_t stream) {
    return nnop_fa_bwd_softcap(d, opts, sinks, dsinks, 0.f, dq, dk, dv, dpair, d_o, o, ms, ls, q, k, v, pair, kpad_mask, workspace,
                               workspace_bytes, stream);
}

int nnop_fa_bwd_softcap(const nnop_fa_desc* d, const nnop_fa_opts* opts, const float* sinks, float* dsinks, float softcap, void* dq,
                        void* dk, void* dv, void* dpair, const void* d_o, const void* o, const void* ms, const void* ls,
                        const void* q, const void* k, const void* v, const void* pair, const uint8_t* kpad_mask, void* workspace,
                        size_t workspace_bytes, nnop_stream_t stream) {
    int st = check_desc(d);
    if (st == NNOP_OK) st = check_opts(opts);
    if (st == NNOP_OK) st = check_softcap(softcap);
    if (st != NNOP_OK) return st;
    if (!sinks) dsinks = nullptr;                          // ignored without sinks, as dpair is without pair
    if (!dq || !dk || !dv || !d_o || !o || !ms || !ls || !q || !k || !v || !workspace) return NNOP_ERR_NULL;
    if (pair && !dpair) return NNOP_ERR_NULL;
    if (sinks && !dsinks) return NNOP_ERR_NULL;
    if (pair && check_pair(d) != NNOP_OK) return NNOP_ERR_SHAPE;
    if (workspace_bytes < bwd_workspace_bytes(*d)) return NNOP_ERR_WORKSPACE;
    {
        const size_t ta = tensor_align(d), ea = dtype_bytes(d->dtype);
        if (misaligned(dq, ta) || misaligned(dk, ta) || misaligned(dv, ta) || misaligned(dpair, ea) || misaligned(d_o, ta) ||
            misaligned(o, ta) || misaligned(q, ta) || misaligned(k, ta) || misaligned(v, ta) || misaligned(pair, ea) ||
            misaligned(ms, ea) || misaligned(ls, ea) || misaligned(workspace, 16) || misaligned(sinks, sizeof(float)) ||
            misaligned(dsinks, sizeof(float)))
            return NNOP_ERR_ALIGN;
    }
    BwdArgs a{dq, dk, dv, dpair, d_o, o, ms, ls, q, k, v, pair, kpad_mask, workspace, workspace_bytes, fa_window(*d, opts),
              sinks, dsinks, softcap};
    hipStream_t s = (hipStream_t)stream;
    // dQ, dK, dV (and dpair) need nothing for a sink: they recompute P from (ms, ls), which include it.  dsinks: one more pass behind them
    return dispatch_dtype(d->dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        const int st = launch_bwd<T>(*d, a, s);
        return (st == NNOP_OK && sinks) ? launch_bwd_sinks<T>(*d, a, s) : st;
    });
}

}  // extern "C"
