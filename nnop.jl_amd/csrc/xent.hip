// xent.hip -- cross-entropy loss over the classes of a row for gfx950 (HBM-streaming), forward and pullback.
//
// No counterpart in the reference.  The loss over an LM head's logits x [rows][n] (include/nnop_hip.h, nnop_cross_entropy):
//   z_j = x_j | c tanh(x_j / c),  lse = log sum_j exp(z_j),  loss = (1 - eps)(lse - z_t) + eps (lse - mean z) + zeta lse^2
//   dx_j = g [p_j (1 + 2 zeta lse) - (1 - eps)[j = t] - eps / n] (1 - (z_j / c)^2),  p_j = exp(z_j - lse)
// Forward: ONE pass, a streaming reduction; the row never lives in registers, so any n works.  A lane folds the chunks it
// loads into a pair (m, d) with sum = d * exp(m): per batch of U chunks the maximum first, then ONE rescale of d and one
// exp2 per element of (z - m) log2(e).  (A running maximum with a rare-rescale branch saves nothing here: a lane sees 16 - 64 chunks of a
// vocabulary row, so in most batches SOME lane of the wave has a new maximum and the wave takes the branch anyway.)
// Lanes, then waves, combine with group_allreduce; with label smoothing the same pass carries sum z.
// Pullback: element-wise with the row's lse, g and target as uniform values: load, compute, store.  The target's
// -(1 - eps) is one compare per 16-byte chunk (the lane that holds the chunk patches it before the store), none per element.
// Launch forms: wave per row (4 rows per workgroup) for short rows, workgroup (256 lanes) per row for vocabularies;
// xent_workgroup_per_row is the one rule.  16-byte accesses when the row starts are 16-byte aligned (base and ld; n
// itself may be odd: the n % VEC last elements are single accesses of the first lanes), else single elements.
// No LDS beyond the reduction slots, no atomics, no workspace.  Bound: HBM (plain); VALU with a cap (two v_exp_f32 and
// one v_rcp_f32 per element).
#include <limits.h>
#include "row_common.hpp"
#include "fa_launch.hpp"

// The vector and the element path must round alike (a dense gradient of an odd vocabulary is bitwise the in-place gradient of
// its padded view): nothing below may be contracted into an FMA differently from one instantiation to the next.  Contraction is
// off for the whole file; where an FMA is wanted it is written out.
#pragma clang fp contract(off)

namespace nnop {

struct XentParams {
    float *loss, *lse_out;           // fwd
    void* dx;                        // bwd
    const float *dloss, *lse_in;     // bwd
    const void *x, *tgt;
    long long ld, ld_grad, ignore;
    int n, idx8, base;
    float eps, zeta, cap, ka, inv_n; // ka = 2 log2(e) / c (cap_tanh)
};

// Chunks in flight per lane: 64 bytes of loads per lane ahead of the fold.
#ifndef NNOP_XENT_U
#define NNOP_XENT_U 4
#endif
// Row length in bytes from which a row gets a workgroup of its own (below: a wave).  Measured on MI355X with each form forced
// (profiles/xent/perf_crossover.jsonl): at 8 KiB the wave form is still up to 2x ahead in the forward, from
// 16 KiB on the workgroup form is 3 - 11 % ahead in both directions (the capped bf16 forward alone breaks even at 32 KiB).
#ifndef NNOP_XENT_WG_BYTES
#define NNOP_XENT_WG_BYTES 16384
#endif
static inline bool xent_workgroup_per_row(long long n, size_t elem_bytes) {
    return (unsigned long long)n * elem_bytes >= (unsigned long long)NNOP_XENT_WG_BYTES;
}

// (maximum, denominator, sum of z): sum_j exp(z_j) = d * exp(m); s only with label smoothing.  m is a logit itself, hence exact, and
// every exponent is the rounded difference (z - m) times log2(e): a row whose mass sits on one huge logit (1e4) gets d = 1 and
// lse = m to the last bit.  (With the reference kept in log2 units, m * log2(e) rounded, lse = (m2 + log2 d) ln 2 is one ulp of
// 1e4 = 1e-3 off, and the pullback's p_t - 1 with it.)
struct XAcc { float m, d, s; };
NNOP_DEV XAcc xent_combine(XAcc a, XAcc b) {
    const float mn = fmaxf(a.m, b.m);
    const float ref = mn == -INFINITY ? 0.f : mn;                 // (-inf) - (-inf): both sides are empty, d stays 0
    return XAcc{mn, a.d * fast_exp2((a.m - ref) * kLog2e) + b.d * fast_exp2((b.m - ref) * kLog2e), a.s + b.s};
}
template <int STEP> NNOP_DEV XAcc fold(XAcc v, int) {
    return xent_combine(v, XAcc{xlane<STEP>(v.m), xlane<STEP>(v.d), xlane<STEP>(v.s)});
}
NNOP_DEV XAcc combine(XAcc a, XAcc b, int) { return xent_combine(a, b); }

// the capped logit: th = tanh(x / c), z = c th (th = 0 without a cap)
template <bool CAP> NNOP_DEV float xent_z(float x, const XentParams& p, float& th) {
    if constexpr (CAP) {
        th = cap_tanh(x, p.ka);
        return p.cap * th;
    } else {
        th = 0.f;
        return x;
    }
}

// N values into (m, d): the maximum first, one rescale, N exponentials.  Dead slots hold -inf.
template <int N> NNOP_DEV void xent_fold(XAcc& a, const float (&z)[N]) {
    float mc = z[0];
#pragma unroll
    for (int i = 1; i < N; ++i) mc = fmaxf(mc, z[i]);
    const float mn = fmaxf(a.m, mc);
    const float ref = mn == -INFINITY ? 0.f : mn;
    float d = a.d * fast_exp2((a.m - ref) * kLog2e);
#pragma unroll
    for (int i = 0; i < N; ++i) d += fast_exp2((z[i] - ref) * kLog2e);
    a.m = mn;
    a.d = d;
}

// the stored target of a row; ok: it is a class of this row (never true for ignore_index), tu: the class
struct XentTarget { bool ignored, ok; unsigned tu; };
NNOP_DEV XentTarget xent_target(const XentParams& p, size_t row) {
    const long long stored = p.idx8 ? ((const long long*)p.tgt)[row] : (long long)((const int*)p.tgt)[row];
    const unsigned long long tu = (unsigned long long)stored - (unsigned long long)p.base;
    XentTarget t;
    t.ignored = stored == p.ignore;
    t.ok = !t.ignored && tu < (unsigned long long)p.n;
    t.tu = t.ok ? (unsigned)tu : 0u;                             // a bad index never becomes an address
    return t;
}

// ---- forward ----------------------------------------------------------------------------------------------------------
// G lanes per row (64: 4 rows per workgroup; 256: one), VEC elements per access.
template <typename T, int VEC, int G, bool CAP, bool SMOOTH>
__global__ __launch_bounds__(256) void xent_fwd_kernel(const XentParams p, const long long rows) {
    typedef T tv __attribute__((ext_vector_type(VEC)));
    constexpr int RPB = 256 / G, U = NNOP_XENT_U;
    __shared__ XAcc slots[G > 64 ? G / 64 : 1];
    const int lane = threadIdx.x % G;
    const long long row = (long long)blockIdx.x * RPB + threadIdx.x / G;
    if (G == 64 && row >= rows) return;                           // whole waves only; G = 256: the grid is the rows
    const T* __restrict__ x = (const T*)p.x + (size_t)row * (size_t)p.ld;
    const int nch = p.n / VEC;
    XAcc a{-INFINITY, 0.f, 0.f};
    float th;
    int c = lane;
    for (; c + (U - 1) * G < nch; c += U * G) {
        tv v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = *reinterpret_cast<const tv*>(x + (size_t)(c + u * G) * VEC);
        float z[U * VEC];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int i = 0; i < VEC; ++i) z[u * VEC + i] = xent_z<CAP>(to_f32(v[u][i]), p, th);
        xent_fold(a, z);
        if constexpr (SMOOTH) {
#pragma unroll
            for (int i = 0; i < U * VEC; ++i) a.s += z[i];
        }
    }
    if (c < nch) {                                                // the last, partial batch
        tv v[U] = {};
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (c + u * G < nch) v[u] = *reinterpret_cast<const tv*>(x + (size_t)(c + u * G) * VEC);
        float z[U * VEC];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool live = c + u * G < nch;
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                const float zz = xent_z<CAP>(to_f32(v[u][i]), p, th);
                z[u * VEC + i] = live ? zz : -INFINITY;
                if constexpr (SMOOTH) a.s += live ? zz : 0.f;
            }
        }
        xent_fold(a, z);
    }
    if constexpr (VEC > 1) {                                      // the n % VEC last elements
        const int e = nch * VEC + lane;
        if (e < p.n) {
            const float z[1] = {xent_z<CAP>(to_f32(x[e]), p, th)};
            xent_fold(a, z);
            if constexpr (SMOOTH) a.s += z[0];
        }
    }
    const XAcc tot = group_allreduce<G>(a, 0, slots);
    if (lane == 0) {
        const float lse = tot.m + logf(tot.d);
        const XentTarget t = xent_target(p, (size_t)row);
        float loss = 0.f;
        if (!t.ignored) {
            const float zt = xent_z<CAP>(to_f32(x[t.tu]), p, th);
            loss = lse - zt;
            if constexpr (SMOOTH) loss = (1.f - p.eps) * loss + p.eps * (lse - tot.s * p.inv_n);
            if (p.zeta != 0.f) loss = __builtin_fmaf(p.zeta * lse, lse, loss);
            if (!t.ok) loss = __builtin_nanf("");
        }
        p.loss[row] = loss;
        p.lse_out[row] = lse;
    }
}

// ---- pullback ---------------------------------------------------------------------------------------------------------
// Every element is stored through round_store (row_common.hpp): the vector and the element path round alike.
// dx may be x itself: a lane reads its chunks before it writes them, and no lane touches another lane's chunk -- hence no
// __restrict__ on either.
template <typename T, int VEC, int G, bool CAP>
__global__ __launch_bounds__(256) void xent_bwd_kernel(const XentParams p, const long long rows) {
    typedef T tv __attribute__((ext_vector_type(VEC)));
    constexpr int RPB = 256 / G, U = NNOP_XENT_U;
    const int lane = threadIdx.x % G;
    const long long row = (long long)blockIdx.x * RPB + threadIdx.x / G;
    if (G == 64 && row >= rows) return;
    const T* x = (const T*)p.x + (size_t)row * (size_t)p.ld;
    T* dx = (T*)p.dx + (size_t)row * (size_t)p.ld_grad;
    const int nch = p.n / VEC;
    const XentTarget t = xent_target(p, (size_t)row);
    if (!t.ok) {                                                  // uniform over the row's lanes: zeros (ignored) or NaN (invalid)
        const T f = from_f32<T>(t.ignored ? 0.f : __builtin_nanf(""));
        tv fv;
#pragma unroll
        for (int i = 0; i < VEC; ++i) fv[i] = f;
        for (int c = lane; c < nch; c += G) *reinterpret_cast<tv*>(dx + (size_t)c * VEC) = fv;
        if constexpr (VEC > 1) {
            const int e = nch * VEC + lane;
            if (e < p.n) dx[e] = f;
        }
        return;
    }
    const float g = p.dloss[row], lse = p.lse_in[row];
    const float A = g * __builtin_fmaf(2.f * p.zeta, lse, 1.f), B = g * p.eps * p.inv_n, Gt = g * (1.f - p.eps);
    const int tc = (int)(t.tu / VEC), tj = (int)(t.tu % VEC);
    // one element before the cap's derivative: A p - B
    auto elem = [&](float xv, float& th) {
        const float z = xent_z<CAP>(xv, p, th);
        return __builtin_fmaf(A, fast_exp2((z - lse) * kLog2e), -B);
    };
    auto chunk = [&](const tv v, const int cc) {
        float f[VEC], th[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) f[i] = elem(to_f32(v[i]), th[i]);
        if (cc == tc) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) f[i] = (i == tj) ? f[i] - Gt : f[i];
        }
        tv o;
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            if constexpr (CAP) f[i] *= __builtin_fmaf(-th[i], th[i], 1.f);
            o[i] = round_store<T>(f[i]);
        }
        *reinterpret_cast<tv*>(dx + (size_t)cc * VEC) = o;
    };
    int c = lane;
    for (; c + (U - 1) * G < nch; c += U * G) {
        tv v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = *reinterpret_cast<const tv*>(x + (size_t)(c + u * G) * VEC);
#pragma unroll
        for (int u = 0; u < U; ++u) chunk(v[u], c + u * G);
    }
    if (c < nch) {
        tv v[U] = {};
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (c + u * G < nch) v[u] = *reinterpret_cast<const tv*>(x + (size_t)(c + u * G) * VEC);
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (c + u * G < nch) chunk(v[u], c + u * G);
    }
    if constexpr (VEC > 1) {
        const int e = nch * VEC + lane;
        if (e < p.n) {
            float th;
            float f = elem(to_f32(x[e]), th);
            if ((unsigned)e == t.tu) f -= Gt;
            if constexpr (CAP) f *= __builtin_fmaf(-th, th, 1.f);
            dx[e] = round_store<T>(f);
        }
    }
}

// ---- launch -----------------------------------------------------------------------------------------------------------
template <typename T, int VEC, int G, bool BWD>
static void launch_xent_form(const XentParams& p, long long rows, hipStream_t s) {
    constexpr int RPB = 256 / G;
    const dim3 grid((unsigned)((rows + RPB - 1) / RPB)), block(256);
    const bool cap = p.cap != 0.f, smooth = p.eps != 0.f;
    if constexpr (BWD) {
        if (cap) hipLaunchKernelGGL((xent_bwd_kernel<T, VEC, G, true>), grid, block, 0, s, p, rows);
        else hipLaunchKernelGGL((xent_bwd_kernel<T, VEC, G, false>), grid, block, 0, s, p, rows);
    } else {
        if (cap && smooth) hipLaunchKernelGGL((xent_fwd_kernel<T, VEC, G, true, true>), grid, block, 0, s, p, rows);
        else if (cap) hipLaunchKernelGGL((xent_fwd_kernel<T, VEC, G, true, false>), grid, block, 0, s, p, rows);
        else if (smooth) hipLaunchKernelGGL((xent_fwd_kernel<T, VEC, G, false, true>), grid, block, 0, s, p, rows);
        else hipLaunchKernelGGL((xent_fwd_kernel<T, VEC, G, false, false>), grid, block, 0, s, p, rows);
    }
}

template <typename T, bool BWD> static int launch_xent_t(const XentParams& p, long long rows, hipStream_t s) {
    constexpr int V = 16 / (int)sizeof(T);
    // the vector path issues 16-byte accesses at multiples of V elements from every row start: bases 16-byte aligned and the
    // strides multiples of V (a padded vocabulary: n = 50257, ld = 50304).  Odd strides and offset views take single elements.
    const bool vec = aligned16({p.x, BWD ? p.dx : nullptr}) && p.ld % V == 0 && (!BWD || p.ld_grad % V == 0);
    const bool wg = xent_workgroup_per_row(p.n, sizeof(T));
    if (vec) {
        if (wg) launch_xent_form<T, V, 256, BWD>(p, rows, s);
        else launch_xent_form<T, V, 64, BWD>(p, rows, s);
    } else {
        if (wg) launch_xent_form<T, 1, 256, BWD>(p, rows, s);
        else launch_xent_form<T, 1, 64, BWD>(p, rows, s);
    }
    return hipGetLastError() == hipSuccess ? NNOP_OK : NNOP_ERR_HIP;
}

template <bool BWD> static int launch_xent_any(const nnop_xent_desc& d, XentParams p, hipStream_t s) {
    if (d.n > 0x7fffffffLL || d.rows > 0x7fffffffLL) return NNOP_ERR_SHAPE;
    const long long ldmax = d.ld > d.ld_grad || !BWD ? d.ld : d.ld_grad;
    if (ldmax > (LLONG_MAX >> 4) / d.rows) return NNOP_ERR_SHAPE;                // rows * ld in bytes fits 64 bits
    p.ld = d.ld; p.ld_grad = d.ld_grad; p.ignore = d.ignore_index;
    p.n = (int)d.n; p.idx8 = d.index_bytes == 8; p.base = d.index_base;
    p.eps = d.label_smoothing; p.zeta = d.z_loss; p.cap = d.softcap;
    p.ka = d.softcap != 0.f ? softcap_k(1.0, d.softcap).ka : 0.f;
    p.inv_n = (float)(1.0 / (double)d.n);
    return dispatch_dtype(d.dtype, [&](auto t) { return launch_xent_t<typename decltype(t)::type, BWD>(p, d.rows, s); });
}

int launch_xent(const nnop_xent_desc& d, float* loss, float* lse, const void* logits, const void* targets, hipStream_t s) {
    XentParams p{};
    p.loss = loss; p.lse_out = lse; p.x = logits; p.tgt = targets;
    return launch_xent_any<false>(d, p, s);
}

int launch_xent_bwd(const nnop_xent_desc& d, void* dlogits, const float* dloss, const float* lse, const void* logits,
                    const void* targets, hipStream_t s) {
    XentParams p{};
    p.dx = dlogits; p.dloss = dloss; p.lse_in = lse; p.x = logits; p.tgt = targets;
    return launch_xent_any<true>(d, p, s);
}

}  // namespace nnop
