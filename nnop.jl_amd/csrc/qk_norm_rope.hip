// qk_norm_rope.hip -- fused QK-norm + RoPE for gfx950 (HBM-streaming), forward and pullback: include/nnop_hip_ext.h.
//
// The per-head RMSNorm of Qwen3 / Gemma 3 / OLMo 2 on q and k, then the Llama rotary embedding.  As three calls (rms_norm on q,
// rms_norm on k, llama_rope) the rows move four times and the norm kernels give a 128-element row a whole wave (row_common.hpp:
// 16 of 64 lanes hold data).  Here: the work decomposition of rope.hip -- D/16 lanes per head row, a lane holding 8 elements of
// the first half and their 8 partners of the second half -- with the row's sum of squares folded over that 2^k-lane group by
// xlane<> butterflies in front of the rotation.  Rows of q and k form one flat grid; cos / sin (shared by the heads of a
// (position, batch)) come through L2.  fp32 arithmetic, one rounding on store; nothing is saved for the pullback, which reads x
// anyway and recomputes rstd.
// Pullback: persistent workgroups, a group of lanes walks rows g, g + n_groups, .. of q, then of k, every lane owning fixed columns,
// so dwq / dwk accumulate in registers; one partial row per workgroup and tensor, folded by a second kernel
// (row_common.hpp fold_partial_rows_kernel) in a fixed order.
// Bound: HBM -- forward 2 (|q| + |k|), pullback 3 (|q| + |k|) (+ the tables, + the partials).
//
// No lane leaves a kernel in front of a cross-lane exchange: a group past the last row works on a clamped row and skips its stores.
#include "row_common.hpp"
#include "qk_norm_rope.hpp"

namespace nnop {

struct QknrParams {
    void *qo, *ko;                    // forward: q_out, k_out;  pullback: dq, dk
    const void *gq, *gk;              // pullback: dq_out, dk_out (the incoming cotangents)
    const void *q, *k, *wq, *wk, *cos, *sin;
    float* part;                      // pullback: [2][n_parts][D] fp32 partial dw rows, q's then k's
    int D, L, QH, KH;
    float eps, offset, inv_d;
    long long rows_q, rows_k;         // head rows of q, of k
    int n_parts;                      // pullback: workgroups
};

// One lane's share of half a row, as loaded.  VEC: 8 consecutive elements at 8 * li, moved with 16-byte accesses (an 8 x fp32
// chunk as two of them: 16-byte alignment of the bases is all the path needs).  Otherwise (li = lane of a 64-lane wave that owns
// the row): elements li, li + 64, li + 128, li + 192 where they exist (half <= 256), zero where not.
template <typename E, bool VEC> struct HalfRegs {
    static constexpr int NE = VEC ? 8 : 4;
    typedef E ev __attribute__((ext_vector_type(NE)));
    ev r;
    NNOP_DEV static int col(int li, int i) { return VEC ? li * 8 + i : li + 64 * i; }
    NNOP_DEV void load(const E* base, int li, int half) {
        if constexpr (VEC) {
            constexpr int PER = 16 / (int)sizeof(E);
            typedef E pv __attribute__((ext_vector_type(PER)));
#pragma unroll
            for (int k = 0; k < 8 / PER; ++k) {
                const pv t = *reinterpret_cast<const pv*>(base + li * 8 + k * PER);
#pragma unroll
                for (int i = 0; i < PER; ++i) r[k * PER + i] = t[i];
            }
        } else {
#pragma unroll
            for (int i = 0; i < NE; ++i) {
                const int c = li + 64 * i;
                r[i] = from_f32<E>(0.f);
                if (c < half) r[i] = base[c];
            }
        }
    }
    NNOP_DEV float get(int i) const { return to_f32(r[i]); }
    NNOP_DEV static void store(E* base, int li, int half, const float (&o)[NE]) {
        if constexpr (VEC) {
            constexpr int PER = 16 / (int)sizeof(E);
            typedef E pv __attribute__((ext_vector_type(PER)));
#pragma unroll
            for (int k = 0; k < 8 / PER; ++k) {
                pv t;
#pragma unroll
                for (int i = 0; i < PER; ++i) t[i] = from_f32<E>(o[k * PER + i]);
                *reinterpret_cast<pv*>(base + li * 8 + k * PER) = t;
            }
        } else {
#pragma unroll
            for (int i = 0; i < NE; ++i) {
                const int c = li + 64 * i;
                if (c < half) base[c] = from_f32<E>(o[i]);
            }
        }
    }
};

// where a head row of one tensor lives: r = (b * H + h) * L + l is its row index in memory as well
struct QknrRow { size_t x, cs; };
NNOP_DEV QknrRow qknr_row(long long r, int H, int L, int D) {
    const unsigned bh = (unsigned)r / (unsigned)L;                  // r < 2^31 (checked by the C API): 32-bit divisions
    const unsigned l = (unsigned)r - bh * (unsigned)L;
    const unsigned b = bh / (unsigned)H;
    return QknrRow{(size_t)r * D, ((size_t)b * L + l) * D};
}

// LPR: lanes per row.  1 .. 32: the 16-byte path, D = 16 * LPR.  64: the element-wise path, any even D <= 512, a wave per row.
template <typename T, typename W, typename CS, int LPR>
__global__ __launch_bounds__(256) void qknr_fwd_kernel(const QknrParams p) {
    constexpr bool VEC = LPR < 64;
    constexpr int NE = HalfRegs<T, VEC>::NE;
    const int li = threadIdx.x % LPR;
    const int half = p.D >> 1;
    long long row = ((long long)blockIdx.x * 256 + threadIdx.x) / LPR;
    const bool live = row < p.rows_q + p.rows_k;
    if (!live) row = p.rows_q + p.rows_k - 1;                       // (see the head of the file)
    const bool is_k = row >= p.rows_q;
    if (is_k) row -= p.rows_q;
    const QknrRow at = qknr_row(row, is_k ? p.KH : p.QH, p.L, p.D);
    // x and y may be one buffer: plain pointers; a lane loads its elements before it stores them and no other lane touches them
    const T* x = (const T*)(is_k ? p.k : p.q) + at.x;
    T* y = (T*)(is_k ? p.ko : p.qo) + at.x;
    const W* __restrict__ w = (const W*)(is_k ? p.wk : p.wq);
    HalfRegs<T, VEC> x1, x2;
    HalfRegs<CS, VEC> cc, ss;
    HalfRegs<W, VEC> w1, w2;
    x1.load(x, li, half); x2.load(x + half, li, half);
    cc.load((const CS*)p.cos + at.cs, li, half); ss.load((const CS*)p.sin + at.cs, li, half);
    w1.load(w, li, half); w2.load(w + half, li, half);
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < NE; ++i) { sq = __builtin_fmaf(x1.get(i), x1.get(i), sq); sq = __builtin_fmaf(x2.get(i), x2.get(i), sq); }
    sq = group_sum<LPR>(sq);
    const float rstd = 1.0f / sqrtf(sq * p.inv_d + p.eps);
    float o1[NE], o2[NE];
#pragma unroll
    for (int i = 0; i < NE; ++i) {
        const float n1 = x1.get(i) * rstd * (w1.get(i) + p.offset), n2 = x2.get(i) * rstd * (w2.get(i) + p.offset);
        const float c = cc.get(i), s = ss.get(i);
        o1[i] = n1 * c - n2 * s;
        o2[i] = n2 * c + n1 * s;
    }
    if (live) {
        HalfRegs<T, VEC>::store(y, li, half, o1);
        HalfRegs<T, VEC>::store(y + half, li, half, o2);
    }
}

// grid = n_parts persistent workgroups of RPB = 256 / LPR groups; group (b, sub) takes rows b * RPB + sub, + n_parts * RPB, ..
// The trip count is the workgroup's, not the group's: every lane runs every iteration (clamped row, nothing stored or summed).
template <typename T, typename W, typename CS, int LPR>
__global__ __launch_bounds__(256) void qknr_bwd_kernel(const QknrParams p) {
    constexpr bool VEC = LPR < 64;
    constexpr int NE = HalfRegs<T, VEC>::NE;
    constexpr int RPB = 256 / LPR;
    constexpr int DC = VEC ? LPR * 16 : 512;                        // columns a group's slice of `comb` holds
    __shared__ float comb[RPB * DC];
    const int li = threadIdx.x % LPR, sub = threadIdx.x / LPR;
    const int half = p.D >> 1;
    const long long stride = (long long)p.n_parts * RPB;
    for (int t = 0; t < 2; ++t) {                                   // q, then k
        const long long rows = t ? p.rows_k : p.rows_q;
        const int H = t ? p.KH : p.QH;
        const T* xb = (const T*)(t ? p.k : p.q);
        const T* gb = (const T*)(t ? p.gk : p.gq);                  // may be the buffer of ob: plain pointers, as in the forward
        T* ob = (T*)(t ? p.ko : p.qo);
        const W* __restrict__ w = (const W*)(t ? p.wk : p.wq);
        float g1[NE], g2[NE], dw1[NE], dw2[NE];
        {
            HalfRegs<W, VEC> w1, w2;
            w1.load(w, li, half); w2.load(w + half, li, half);
#pragma unroll
            for (int i = 0; i < NE; ++i) { g1[i] = w1.get(i) + p.offset; g2[i] = w2.get(i) + p.offset; dw1[i] = 0.f; dw2[i] = 0.f; }
        }
        for (long long base = (long long)blockIdx.x * RPB; base < rows; base += stride) {
            long long row = base + sub;
            const bool live = row < rows;
            if (!live) row = rows - 1;
            const QknrRow at = qknr_row(row, H, p.L, p.D);
            HalfRegs<T, VEC> x1, x2, d1, d2;
            HalfRegs<CS, VEC> cc, ss;
            x1.load(xb + at.x, li, half); x2.load(xb + at.x + half, li, half);
            d1.load(gb + at.x, li, half); d2.load(gb + at.x + half, li, half);
            cc.load((const CS*)p.cos + at.cs, li, half); ss.load((const CS*)p.sin + at.cs, li, half);
            float n1[NE], n2[NE];                                   // dn: the rotation of dy with sin_sign = -1
            Sum2 acc{0.f, 0.f};                                     // a: sum x^2, b: dd = sum m x
#pragma unroll
            for (int i = 0; i < NE; ++i) {
                const float a = d1.get(i), b = d2.get(i), c = cc.get(i), s = ss.get(i);
                n1[i] = a * c + b * s;
                n2[i] = b * c - a * s;
                const float xa = x1.get(i), xc = x2.get(i);
                acc.a = __builtin_fmaf(xa, xa, acc.a); acc.a = __builtin_fmaf(xc, xc, acc.a);
                acc.b = __builtin_fmaf(n1[i] * g1[i], xa, acc.b); acc.b = __builtin_fmaf(n2[i] * g2[i], xc, acc.b);
            }
            acc.a = group_sum<LPR>(acc.a);
            acc.b = group_sum<LPR>(acc.b);
            const float rstd = 1.0f / sqrtf(acc.a * p.inv_d + p.eps);
            const float kx = -p.inv_d * rstd * rstd * acc.b * rstd;  // -rstd^3 dd / D
            const float lv = live ? rstd : 0.f;                     // a clamped row adds nothing to dw
            float o1[NE], o2[NE];
#pragma unroll
            for (int i = 0; i < NE; ++i) {
                const float xa = x1.get(i), xc = x2.get(i);
                dw1[i] = __builtin_fmaf(n1[i], xa * lv, dw1[i]);
                dw2[i] = __builtin_fmaf(n2[i], xc * lv, dw2[i]);
                o1[i] = __builtin_fmaf(n1[i] * g1[i], rstd, kx * xa);
                o2[i] = __builtin_fmaf(n2[i] * g2[i], rstd, kx * xc);
            }
            if (live) {
                HalfRegs<T, VEC>::store(ob + at.x, li, half, o1);
                HalfRegs<T, VEC>::store(ob + at.x + half, li, half, o2);
            }
        }
        // fold the workgroup's groups in a fixed order: one partial row per workgroup and tensor, every column of it written
        if (t) __syncthreads();                                     // q's fold has read comb
#pragma unroll
        for (int i = 0; i < NE; ++i) {
            const int c = HalfRegs<T, VEC>::col(li, i);
            if (VEC || c < half) { comb[sub * DC + c] = dw1[i]; comb[sub * DC + half + c] = dw2[i]; }
        }
        __syncthreads();
        float* part = p.part + ((size_t)t * p.n_parts + blockIdx.x) * p.D;
        for (int c = threadIdx.x; c < p.D; c += 256) {
            float s = comb[c];
            for (int g = 1; g < RPB; ++g) s += comb[g * DC + c];
            part[c] = s;
        }
    }
}

// Partial rows of the pullback: every group gets >= 4 rows of the longer tensor when there are that many, at most kQknrCap
// workgroups (4 per CU: what the pullback's ~116 VGPRs per lane keep resident, one round).  The workspace is sized for the
// narrowest workgroup (4 rows).
constexpr int kQknrCap = 1024;
static inline long long qknr_parts(long long rows_q, long long rows_k, int rpb) {
    const long long rows = rows_q > rows_k ? rows_q : rows_k;
    const long long n = (rows + 4LL * rpb - 1) / (4LL * rpb);
    return n < 1 ? 1 : (n > kQknrCap ? kQknrCap : n);
}
size_t qknr_bwd_ws_bytes(const nnop_qknr_desc& d) {
    const long long bl = (long long)d.batch * d.seq;
    return (size_t)qknr_parts(bl * d.qh, bl * d.kh, 4) * 2 * (size_t)d.dim * sizeof(float);
}

// lanes per row of the 16-byte path, 0 where D has none
static inline int qknr_lpr(int D) {
    const int n = D / 16;
    return (D % 16 == 0 && (n & (n - 1)) == 0 && n >= 1 && n <= 32) ? n : 0;
}

template <typename T, typename W, typename CS, int LPR> static void launch_fwd_lpr(const QknrParams& p, hipStream_t s) {
    const long long items = (p.rows_q + p.rows_k) * LPR;
    hipLaunchKernelGGL((qknr_fwd_kernel<T, W, CS, LPR>), dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, p);
}
template <typename T, typename W, typename CS, int LPR> static void launch_bwd_lpr(QknrParams& p, hipStream_t s) {
    p.n_parts = (int)qknr_parts(p.rows_q, p.rows_k, 256 / LPR);
    hipLaunchKernelGGL((qknr_bwd_kernel<T, W, CS, LPR>), dim3((unsigned)p.n_parts), dim3(256), 0, s, p);
}

template <typename T, typename W, typename CS> static int launch_qknr_t(QknrParams p, bool bwd, float* dwq, float* dwk, hipStream_t s) {
    const bool al = aligned16({p.qo, p.ko, p.gq, p.gk, p.q, p.k, p.wq, p.wk, p.cos, p.sin});
    const int lpr = al ? qknr_lpr(p.D) : 0;
#define NNOP_QKNR_CASE(N) case N: if (bwd) launch_bwd_lpr<T, W, CS, (N ? N : 64)>(p, s); else launch_fwd_lpr<T, W, CS, (N ? N : 64)>(p, s); break;
    switch (lpr) {
        NNOP_QKNR_CASE(1) NNOP_QKNR_CASE(2) NNOP_QKNR_CASE(4) NNOP_QKNR_CASE(8) NNOP_QKNR_CASE(16) NNOP_QKNR_CASE(32)
        NNOP_QKNR_CASE(0)
    }
#undef NNOP_QKNR_CASE
    if (bwd)                                                        // dwq from q's partial rows, dwk from k's behind them
        hipLaunchKernelGGL((fold_partial_rows_kernel<float>), dim3((unsigned)((p.D + 31) / 32), 2), dim3(1024), 0, s, dwq, dwk,
                           (const float*)p.part, (const float*)p.part + (size_t)p.n_parts * p.D, p.n_parts, p.D);
    return hipGetLastError() == hipSuccess ? NNOP_OK : NNOP_ERR_HIP;
}

static int launch_qknr(const nnop_qknr_desc& d, QknrParams p, bool bwd, float* dwq, float* dwk, hipStream_t s) {
    p.D = d.dim; p.L = d.seq; p.QH = d.qh; p.KH = d.kh;
    p.eps = d.eps; p.offset = d.offset; p.inv_d = 1.0f / (float)d.dim;
    p.rows_q = (long long)d.batch * d.qh * d.seq;
    p.rows_k = (long long)d.batch * d.kh * d.seq;
    p.n_parts = 0;
    return dispatch_dtype_side(d.dtype, d.w_dtype, [&](auto t, auto w) {
        using T = typename decltype(t)::type;
        using W = typename decltype(w)::type;
        return d.cs_dtype == NNOP_F32 ? launch_qknr_t<T, W, float>(p, bwd, dwq, dwk, s) : launch_qknr_t<T, W, T>(p, bwd, dwq, dwk, s);
    });
}

int launch_qknr_fwd(const nnop_qknr_desc& d, void* qo, void* ko, const void* q, const void* k, const void* wq, const void* wk,
                    const void* cos, const void* sin, hipStream_t s) {
    QknrParams p{};
    p.qo = qo; p.ko = ko; p.q = q; p.k = k; p.wq = wq; p.wk = wk; p.cos = cos; p.sin = sin;
    return launch_qknr(d, p, false, nullptr, nullptr, s);
}

int launch_qknr_bwd(const nnop_qknr_desc& d, void* dq, void* dk, float* dwq, float* dwk, const void* gq, const void* gk,
                    const void* q, const void* k, const void* wq, const void* wk, const void* cos, const void* sin,
                    void* workspace, hipStream_t s) {
    QknrParams p{};
    p.qo = dq; p.ko = dk; p.gq = gq; p.gk = gk; p.q = q; p.k = k; p.wq = wq; p.wk = wk; p.cos = cos; p.sin = sin;
    p.part = (float*)workspace;
    return launch_qknr(d, p, true, dwq, dwk, s);
}

}  // namespace nnop
