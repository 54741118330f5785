// moe_router.hip -- the mixture-of-experts gate for gfx950, forward and pullback: include/nnop_hip_moe.h.
//
// Forward: a group of LPR = 16 / 32 / 64 lanes of a wave owns a row of E <= 1024 logits (4 / 2 / 1 rows per wave) and holds it in
// registers as NE <= 16 order-preserving 32-bit keys per lane: key(x) is monotone in x, NaN on top, -0 folded onto +0, and 0 for a slot
// that is padding or already taken (below the key of -inf, so such a slot is never chosen while a real one is left: k <= E).  Top-k is
// k rounds of arg-max: the lane's best (strict >, slots in ascending expert order: the lower index wins a tie), then the butterfly of
// row_common.hpp on the pair (key, ~index) compared as one 64-bit number -- DPP within 16 lanes, v_permlane16/32_swap above, no LDS,
// no barrier.  Round j's winner stays on lane j of the group, so the k weights are computed and stored by k lanes at once.
// Round 0 yields the row maximum; the weights use expf, not the fast form, and the denominator of lse is summed and its logarithm
// taken in fp64: the row is tiny, the gate of w is 2e-6, and the pullback's p = exp(x - lse) inherits every error of lse.
// Pullback: no cross-lane traffic at all.  Every lane reads the row's k (idx, w, dw) triples itself (one address per group: a
// broadcast), forms c p[e] for its own columns from the saved lse and adds the selected entries where an index is its own; the k-term
// sum S and the final additions are in fp64.
// Bound: launch latency and the k dependent reduction rounds; the logits of 8192 tokens x 128 experts are 2 MB.
//
// No lane leaves the forward kernel in front of a cross-lane exchange: a group past the last row works on the last row and stores nothing.
#include "row_common.hpp"
#include "moe.hpp"

namespace nnop {

struct MoeRouterParams {
    const void* logits;
    void* dlogits;
    int32_t* idx;           // forward: written;  pullback: read
    float *w, *lse;         // likewise
    const float *dw, *dlse;
    int T, E, K, norm;
    long long ld;
};

NNOP_DEV uint32_t moe_key(float x) {
    if (x != x) return 0xFFFFFFFFu;
    uint32_t b = __float_as_uint(x);
    if ((b << 1) == 0) b = 0;                                       // -0 -> +0
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
// the value of a key (NaN for the NaN key; a -0 comes back as +0)
NNOP_DEV float moe_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

template <int STEP> NNOP_DEV uint32_t xlane_u(uint32_t x) { return __float_as_uint(xlane<STEP>(__uint_as_float(x))); }

// one butterfly step on (key, nidx): the larger key, then the larger nidx = ~index (the lower index)
template <int STEP> NNOP_DEV void ki_fold(uint32_t& k, uint32_t& n) {
    const uint32_t pk = xlane_u<STEP>(k), pn = xlane_u<STEP>(n);
    const bool take = pk > k || (pk == k && pn > n);
    k = take ? pk : k;
    n = take ? pn : n;
}
template <int G> NNOP_DEV void ki_allreduce(uint32_t& k, uint32_t& n) {
    ki_fold<1>(k, n); ki_fold<2>(k, n); ki_fold<4>(k, n); ki_fold<8>(k, n);
    if constexpr (G > 16) ki_fold<16>(k, n);
    if constexpr (G > 32) ki_fold<32>(k, n);
}
// the same in fp64, the two words of a value exchanged one by one (the denominator of lse: its rounding would otherwise be of the
// size of the one rounding the saved fp32 lse has anyway)
template <int STEP> NNOP_DEV double xlane_d(double x) {
    return __hiloint2double((int)xlane_u<STEP>((uint32_t)__double2hiint(x)), (int)xlane_u<STEP>((uint32_t)__double2loint(x)));
}
template <int G> NNOP_DEV double moe_group_sum(double v) {
    v += xlane_d<1>(v); v += xlane_d<2>(v); v += xlane_d<4>(v); v += xlane_d<8>(v);
    if constexpr (G > 16) v += xlane_d<16>(v);
    if constexpr (G > 32) v += xlane_d<32>(v);
    return v;
}

// Slot s of lane li holds expert ((s / VEC) * LPR + li) * VEC + s % VEC: VEC = 1 is the element-wise layout (a wave's load is one
// contiguous run), VEC = 16 / sizeof(T) the 16-byte one.  Ascending in s.
template <int VEC, int LPR> NNOP_DEV int moe_col(int s, int li) { return ((s / VEC) * LPR + li) * VEC + s % VEC; }

// the row's columns < E as fp32, `fill` elsewhere
template <typename T, int VEC, int LPR, int NE> NNOP_DEV void moe_load_row(float (&v)[NE], const T* row, int E, int li, float fill) {
    typedef T tv __attribute__((ext_vector_type(VEC)));
#pragma unroll
    for (int j = 0; j < NE / VEC; ++j) {
        const int e0 = (j * LPR + li) * VEC;
        if constexpr (VEC > 1) {
            tv t;
            const bool in = e0 < E;                                 // E % VEC == 0: a piece is inside or outside as a whole
            if (in) t = *reinterpret_cast<const tv*>(row + e0);
#pragma unroll
            for (int i = 0; i < VEC; ++i) v[j * VEC + i] = in ? to_f32(t[i]) : fill;
        } else {
            v[j] = e0 < E ? to_f32(row[e0]) : fill;
        }
    }
}

template <typename T, int VEC, int LPR, int NE>
__global__ __launch_bounds__(256) void moe_router_fwd_kernel(const MoeRouterParams p) {
    const int li = threadIdx.x % LPR;
    long long row = ((long long)blockIdx.x * 256 + threadIdx.x) / LPR;
    const bool live = row < p.T;
    if (!live) row = p.T - 1;                                       // (see the head of the file)
    uint32_t key[NE];
    {
        float v[NE];
        moe_load_row<T, VEC, LPR, NE>(v, (const T*)p.logits + (size_t)row * p.ld, p.E, li, 0.f);
#pragma unroll
        for (int s = 0; s < NE; ++s) key[s] = moe_col<VEC, LPR>(s, li) < p.E ? moe_key(v[s]) : 0u;
    }
    float m = 0.f, my_v = 0.f;
    double sum = 0.0;
    int my_e = 0;
    for (int r = 0; r < p.K; ++r) {
        uint32_t bk = key[0];
        int bs = 0;
#pragma unroll
        for (int s = 1; s < NE; ++s)
            if (key[s] > bk) { bk = key[s]; bs = s; }
        uint32_t bn = ~(uint32_t)moe_col<VEC, LPR>(bs, li);
        ki_allreduce<LPR>(bk, bn);
        const int e = (int)~bn;
        const float v = moe_unkey(bk);
        if (r == 0) {                                               // the row maximum: the denominator of lse, over every column
            m = v;
#pragma unroll
            for (int s = 0; s < NE; ++s) sum += key[s] ? (double)expf(moe_unkey(key[s]) - m) : 0.0;
        }
        if (li == r) { my_v = v; my_e = e; }
#pragma unroll
        for (int s = 0; s < NE; ++s)
            if (moe_col<VEC, LPR>(s, li) == e) key[s] = 0u;
    }
    sum = moe_group_sum<LPR>(sum);
    const float lse = (float)((double)m + log(sum));
    const bool mine = li < p.K;
    // Both norms divide exp(v - m) by a sum: the selected logits are near the maximum, so v - m is small and carries less rounding
    // than v - lse would.  Sum and quotient in fp64, one rounding to fp32: the pullback multiplies the saved weight of a dominant
    // expert (w near 1) by cotangents of order 1 and cancels, so an ulp of w there is an ulp of 1 in dlogits.
    const double ej = mine ? (double)expf(my_v - m) : 0.0;
    const float wj = (float)(ej / (p.norm == NNOP_MOE_NORM_TOPK ? moe_group_sum<LPR>(ej) : sum));
    if (live && mine) {
        p.idx[(size_t)row * p.K + li] = my_e;
        p.w[(size_t)row * p.K + li] = wj;
    }
    if (live && li == 0) p.lse[row] = lse;
}

template <typename T, int VEC, int LPR, int NE>
__global__ __launch_bounds__(256) void moe_router_bwd_kernel(const MoeRouterParams p) {
    typedef T tv __attribute__((ext_vector_type(VEC)));
    const int li = threadIdx.x % LPR;
    const long long row = ((long long)blockIdx.x * 256 + threadIdx.x) / LPR;
    if (row >= p.T) return;                                         // no cross-lane exchange in this kernel
    const int32_t* __restrict__ idx = p.idx + (size_t)row * p.K;
    const float* __restrict__ w = p.w + (size_t)row * p.K;
    const float* __restrict__ dw = p.dw + (size_t)row * p.K;
    // S, the coefficients and the final sums in fp64: k + a few operations per element, and the differences dw - S and
    // w dw - S p, which cancel for a dominant expert, then cost one rounding instead of several
    double S = 0.0;
    for (int j = 0; j < p.K; ++j) S += (double)w[j] * (double)dw[j];
    const bool topk = p.norm == NNOP_MOE_NORM_TOPK;
    const bool has_p = p.dlse || !topk;
    const double dl = p.dlse ? (double)p.dlse[row] : 0.0;
    const double c = topk ? dl : dl - S;
    float pr[NE];
    if (has_p) {
        const float lse = p.lse[row];
        moe_load_row<T, VEC, LPR, NE>(pr, (const T*)p.logits + (size_t)row * p.ld, p.E, li, 0.f);
#pragma unroll
        for (int s = 0; s < NE; ++s) pr[s] = expf(pr[s] - lse);
        if (!topk)                                                  // p of a selected expert is its saved weight, to the last bit
            for (int j = 0; j < p.K; ++j) {
                const int e = idx[j];
                const float wj = w[j];
#pragma unroll
                for (int s = 0; s < NE; ++s)
                    if (moe_col<VEC, LPR>(s, li) == e) pr[s] = wj;
            }
    }
    double out[NE];
#pragma unroll
    for (int s = 0; s < NE; ++s) out[s] = has_p ? c * (double)pr[s] : 0.0;
    for (int j = 0; j < p.K; ++j) {
        const int e = idx[j];
        const double sel = (double)w[j] * (topk ? (double)dw[j] - S : (double)dw[j]);
#pragma unroll
        for (int s = 0; s < NE; ++s)
            if (moe_col<VEC, LPR>(s, li) == e) out[s] += sel;
    }
    T* y = (T*)p.dlogits + (size_t)row * p.ld;
#pragma unroll
    for (int j = 0; j < NE / VEC; ++j) {
        const int e0 = (j * LPR + li) * VEC;
        if (e0 < p.E) {
            if constexpr (VEC > 1) {
                tv t;
#pragma unroll
                for (int i = 0; i < VEC; ++i) t[i] = from_f32<T>((float)out[j * VEC + i]);
                *reinterpret_cast<tv*>(y + e0) = t;
            } else {
                y[e0] = from_f32<T>((float)out[j]);
            }
        }
    }
}

template <typename T, int VEC, int LPR, int NE> static void launch_shape(const MoeRouterParams& p, bool bwd, hipStream_t s) {
    const long long items = (long long)p.T * LPR;
    const dim3 grid((unsigned)((items + 255) / 256)), block(256);
    if (bwd) hipLaunchKernelGGL((moe_router_bwd_kernel<T, VEC, LPR, NE>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((moe_router_fwd_kernel<T, VEC, LPR, NE>), grid, block, 0, s, p);
}

template <typename T> static int launch_moe_router_t(const MoeRouterParams& p, bool bwd, hipStream_t s) {
    constexpr int VEC = 16 / (int)sizeof(T);
    const int E = p.E;
    const bool vec = E % VEC == 0 && p.ld % VEC == 0 && (bwd ? aligned16({p.logits, p.dlogits}) : aligned16({p.logits}));
    if (vec) {
        const int pieces = E / VEC;                                 // <= 256 (fp32), <= 128 (16-bit): at most 16 columns per lane
        if (pieces <= 16) launch_shape<T, VEC, 16, VEC>(p, bwd, s);
        else if (pieces <= 32) launch_shape<T, VEC, 32, VEC>(p, bwd, s);
        else if (pieces <= 64) launch_shape<T, VEC, 64, VEC>(p, bwd, s);
        else if (pieces <= 128) launch_shape<T, VEC, 64, 2 * VEC>(p, bwd, s);
        else if constexpr (VEC == 4) launch_shape<T, VEC, 64, 4 * VEC>(p, bwd, s);
    } else {
        if (E <= 16) launch_shape<T, 1, 16, 1>(p, bwd, s);
        else if (E <= 32) launch_shape<T, 1, 32, 1>(p, bwd, s);
        else if (E <= 64) launch_shape<T, 1, 64, 1>(p, bwd, s);
        else if (E <= 128) launch_shape<T, 1, 64, 2>(p, bwd, s);
        else if (E <= 256) launch_shape<T, 1, 64, 4>(p, bwd, s);
        else if (E <= 512) launch_shape<T, 1, 64, 8>(p, bwd, s);
        else launch_shape<T, 1, 64, 16>(p, bwd, s);
    }
    return hipGetLastError() == hipSuccess ? NNOP_OK : NNOP_ERR_HIP;
}

static int launch_moe_router(const nnop_moe_router_desc& d, MoeRouterParams p, bool bwd, hipStream_t s) {
    p.T = d.tokens; p.E = d.experts; p.K = d.topk; p.norm = d.norm; p.ld = d.ld;
    return dispatch_dtype(d.dtype, [&](auto t) { return launch_moe_router_t<typename decltype(t)::type>(p, bwd, s); });
}

int launch_moe_router_fwd(const nnop_moe_router_desc& d, int32_t* idx, float* w, float* lse, const void* logits, hipStream_t s) {
    MoeRouterParams p{};
    p.logits = logits; p.idx = idx; p.w = w; p.lse = lse;
    return launch_moe_router(d, p, false, s);
}

int launch_moe_router_bwd(const nnop_moe_router_desc& d, void* dlogits, const float* dw, const float* dlse, const float* w,
                          const int32_t* idx, const float* lse, const void* logits, hipStream_t s) {
    MoeRouterParams p{};
    p.logits = logits; p.dlogits = dlogits; p.dw = dw; p.dlse = dlse;
    p.idx = const_cast<int32_t*>(idx); p.w = const_cast<float*>(w); p.lse = const_cast<float*>(lse);
    return launch_moe_router(d, p, true, s);
}

}  // namespace nnop
