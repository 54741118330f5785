// moe_mx_decode_glu.hip -- the kernel of libnnop_hip_moe_mx_decode_glu.so (include/nnop_hip_moe_mx_decode_glu.h): the weight-streaming
// MXFP4 forward of moe_mx_decode.hip on a fused gate-up projection, with the gated activation in its epilogue and, optionally, the token
// gather in front.  gfx950 (MI355X) only.
//
// What it replaces is three launches, moe_permute -> moe_mx_decode_linear (K -> 2 I) -> glu: the [S][2 I] pre-activations are rounded to
// 16 bits, written, read back and activated.  Here they stay in the accumulators.  The pass of a wave over K is decode_ring of
// moe_mx_decode_ring.hpp, the ring the eighth library runs, so a pre-activation is summed in that library's order, a function of K and the
// type alone; the activations are glu_act.hpp's, the text glu.hip compiles, under the same floating-point flags.
//
// Work: workgroup (e, c) is expert e and the columns 128 c ... 128 c + 127 of h = 256 weight rows, all of K; the grid is E ceil(I / 128),
// fixed on the host.  Wave w owns kNT = 4 MFMA row tiles of 16 weight rows, and a lane's accumulator acc[i][g] holds 4 consecutive weight
// rows of tile i for one x row.
//   interleaved  (gate of column j is weight row 2 j, up row 2 j + 1)  the wave's rows are n0 = 256 c + 64 w ... n0 + 63, tile i starts at
//                n0 + 16 i, and acc[i][g][0 .. 3] are (gate, up) of columns (n0 + 16 i + 4 q) / 2 and the next one: a 4-byte store
//                where ld_h is even and h is 4-byte aligned, element-wise otherwise.
//   halves       (gate row j, up row I + j)  the wave's columns are j0 = 128 c + 32 w ... j0 + 31; tiles 0, 1 are the gate rows
//                j0 + 16 i, tiles 2, 3 the up rows I + j0 + 16 (i - 2); acc[i][g][j] pairs with acc[i + 2][g][j]: an 8-byte store of 4
//                columns where ld_h is a multiple of 4 and h is 8-byte aligned.  I need not be a multiple of 16: a tile's rows are clamped
//                and selected per lane.
// Either way p = acc + bias in fp32, h = a(gate) * upside(up) in fp32, one rounding through round_store as in glu.hip.
//
// Gather: with perm, a lane's x row of group g is x + (perm[m0 + m] / k) * ld_x where the entry lies in [0, T k); one 4-byte load per
// lane and pass, in front of the ring.  An entry outside, or a slot beyond the pass's rows, points at the token of the pass's first slot
// (which lane 0 fetches anyway), or at row 0 where that entry is invalid itself, with xok = false: the ring's loads stay unconditional and
// what they fetched is replaced by zeros at the consumer.  Such a row of h is still written: it is the activation of the bias alone.
//
// Rows outside every expert are written as +0 as in moe_mx_decode.hip: those in front of offsets[0] by the workgroups of expert 0, those
// behind offsets[E] by the workgroups of expert E - 1, each in its own columns.  No LDS, no barrier, no atomics, no workspace.
#include "moe_mx_decode_glu.hpp"
#include "moe_mx_decode_ring.hpp"
#include "row_common.hpp"
#include "glu_act.hpp"
#include <type_traits>

namespace nnop {
namespace {

static_assert(16 * kNT * (kThreads / 64) == 2 * kMoeMxDecodeGluCols, "four waves cover the workgroup's 256 weight rows");

struct GluDecodeParams {
    void* h;
    const void* x;
    const uint8_t* blocks;
    const uint8_t* scales;
    const void* bias;  // NULL: none
    const int32_t* offsets;
    const int32_t* perm;  // NULL: x is in slot order
    long long ld_x, ld_h, ld_b;  // elements
    long long ld_q, ld_s;        // bytes
    int S, E, K, I;
    int ct;            // column groups per expert
    uint32_t TK, k;    // with perm: tokens * topk, topk
    int hvec;          // h takes vector stores (interleaved: 4 bytes, halves: 8)
    int bvec;          // the bias takes 8-byte loads
    float alpha, limit;
};

// rows r0 ... r1 - 1 of the workgroup's columns j0 ... j0 + 127 become +0
template <typename T> __device__ __forceinline__ void zero_rows(const GluDecodeParams& p, int r0, int r1, int j0, int t) {
    const int c = j0 + 2 * (t & 63);
    if (c >= p.I) return;
    const T z = (T)0.f;
    for (int r = r0 + (t >> 6); r < r1; r += kThreads / 64) {
        T* dst = static_cast<T*>(p.h) + r * p.ld_h + c;
        dst[0] = z;
        if (c + 1 < p.I) dst[1] = z;
    }
}

// One pass of a wave: slot rows m0 ... m0 + rows - 1 (rows <= 16 G) of expert e against the wave's 64 weight rows; c0 is the wave's
// first weight row (interleaved) or its first column of h (halves).
template <typename T, bool XA, int ACT, bool HALVES, bool GATHER, int G>
__device__ __forceinline__ void glu_pass(const GluDecodeParams& p, int e, int c0, int m0, int rows, int lane) {
    typedef T t2 __attribute__((ext_vector_type(2)));
    typedef T t4 __attribute__((ext_vector_type(4)));
    const int fr = lane & 15, fq = lane >> 4;
    const int N = 2 * p.I;
    const RingWeights w{p.blocks, p.scales, p.ld_q, p.ld_s, p.K, N};
    int base[kNT], end[kNT];
#pragma unroll
    for (int i = 0; i < kNT; ++i) {
        if constexpr (HALVES) {
            base[i] = (i < 2 ? 0 : p.I) + c0 + 16 * (i & 1);
            end[i] = i < 2 ? p.I : N;
        } else {
            base[i] = c0 + 16 * i;
            end[i] = N;
        }
    }
    const T* xr[G];
    bool xok[G];
    if constexpr (GATHER) {
        int tok[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int m = 16 * g + fr;
            const bool in = m < rows;
            const uint32_t idx = (uint32_t)p.perm[m0 + (in ? m : 0)];
            const bool valid = idx < p.TK;
            tok[g] = valid ? (int)(idx / p.k) : -1;
            xok[g] = in && valid;
        }
        const int first = __builtin_amdgcn_readfirstlane(tok[0]);  // lane 0 holds slot m0, which exists
        const int fallback = first < 0 ? 0 : first;
#pragma unroll
        for (int g = 0; g < G; ++g) xr[g] = static_cast<const T*>(p.x) + (long long)(xok[g] ? tok[g] : fallback) * p.ld_x;
    } else {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int m = 16 * g + fr;
            xok[g] = m < rows;
            xr[g] = static_cast<const T*>(p.x) + (long long)(m0 + (xok[g] ? m : 0)) * p.ld_x;
        }
    }
    decode_ring<T, XA, G>(w, e, base, end, xr, xok, lane, [&](const f32x4 (&acc)[kNT][G]) {
        const T* bias = p.bias ? static_cast<const T*>(p.bias) + e * p.ld_b : nullptr;
        // four pre-activation columns n ... n + 3 of the bias, those < lim, in fp32
        auto bias4 = [&](int n, int lim, bool whole) {
            f32x4 bv = f32x4{0.f, 0.f, 0.f, 0.f};
            if (bias != nullptr) {
                if (p.bvec && whole) {
                    const t4 v = *reinterpret_cast<const t4*>(bias + n);
#pragma unroll
                    for (int j = 0; j < 4; ++j) bv[j] = (float)v[j];
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (n + j < lim) bv[j] = (float)bias[n + j];
                }
            }
            return bv;
        };
        if constexpr (HALVES) {
            // acc[i][g][j], acc[i + 2][g][j] are gate and up of h[m0 + 16 g + fr][c0 + 16 i + 4 fq + j], i = 0, 1
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int c = c0 + 16 * i + 4 * fq;
                if (c >= p.I) continue;
                const bool whole = c + 3 < p.I;
                const f32x4 bg = bias4(c, p.I, whole), bu = bias4(p.I + c, N, whole);
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const int m = 16 * g + fr;
                    if (m >= rows) continue;
                    const f32x4 vg = acc[i][g] + bg, vu = acc[i + 2][g] + bu;
                    T out[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) out[j] = round_store<T>(glu_fwd_elem<ACT>(vg[j], vu[j], p.alpha, p.limit));
                    T* dst = static_cast<T*>(p.h) + (long long)(m0 + m) * p.ld_h + c;
                    if (p.hvec && whole) {
                        *reinterpret_cast<t4*>(dst) = t4{out[0], out[1], out[2], out[3]};
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (c + j < p.I) dst[j] = out[j];
                    }
                }
            }
        } else {
            // acc[i][g][0 .. 3] are gate, up, gate, up of h[m0 + 16 g + fr][(c0 + 16 i + 4 fq) / 2 + {0, 1}]
#pragma unroll
            for (int i = 0; i < kNT; ++i) {
                const int n = c0 + 16 * i + 4 * fq;
                if (n >= N) continue;  // n and N are even: n + 1 < N
                const bool whole = n + 3 < N;
                const f32x4 bv = bias4(n, N, whole);
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const int m = 16 * g + fr;
                    if (m >= rows) continue;
                    const f32x4 v = acc[i][g] + bv;
                    const T h0 = round_store<T>(glu_fwd_elem<ACT>(v[0], v[1], p.alpha, p.limit));
                    const T h1 = round_store<T>(glu_fwd_elem<ACT>(v[2], v[3], p.alpha, p.limit));
                    T* dst = static_cast<T*>(p.h) + (long long)(m0 + m) * p.ld_h + n / 2;
                    if (p.hvec && whole) {
                        *reinterpret_cast<t2*>(dst) = t2{h0, h1};
                    } else {
                        dst[0] = h0;
                        if (whole) dst[1] = h1;
                    }
                }
            }
        }
    });
}

template <typename T, bool XA, int ACT, bool HALVES, bool GATHER>
__global__ __launch_bounds__(kThreads) void moe_mx_decode_glu_kernel(const GluDecodeParams p) {
    const int t = threadIdx.x;
    const int e = blockIdx.x / (unsigned)p.ct, j0 = (blockIdx.x % (unsigned)p.ct) * kMoeMxDecodeGluCols;
    const int lo = clamped_offset(p.offsets, e, p.S), hi = clamped_offset(p.offsets, e + 1, p.S);
    if (e == 0) zero_rows<T>(p, 0, lo, j0, t);
    if (e == p.E - 1) zero_rows<T>(p, hi, p.S, j0, t);
    if (hi <= lo) return;  // no rows: no weight byte is loaded
    // the wave's first weight row (interleaved: 64 rows = 32 columns of h) or first column of h (halves: 32 columns)
    const int c0 = HALVES ? j0 + (t >> 6) * 32 : 2 * j0 + (t >> 6) * 64;
    if (c0 >= (HALVES ? p.I : 2 * p.I)) return;  // no barrier follows: a wave without columns may leave
    for (int m0 = lo; m0 < hi; m0 += 16 * kMaxGroups) {
        const int rows = min(hi - m0, 16 * kMaxGroups);
        if (kMaxGroups == 1 || rows <= 16) glu_pass<T, XA, ACT, HALVES, GATHER, 1>(p, e, c0, m0, rows, t & 63);
        else glu_pass<T, XA, ACT, HALVES, GATHER, kMaxGroups>(p, e, c0, m0, rows, t & 63);
    }
}

template <typename T, bool XA, int ACT, bool HALVES> int launch_gather(const GluDecodeParams& p, dim3 grid, hipStream_t s) {
    if (p.perm) hipLaunchKernelGGL((moe_mx_decode_glu_kernel<T, XA, ACT, HALVES, true>), grid, dim3(kThreads), 0, s, p);
    else hipLaunchKernelGGL((moe_mx_decode_glu_kernel<T, XA, ACT, HALVES, false>), grid, dim3(kThreads), 0, s, p);
    return hipGetLastError() == hipSuccess ? (int)NNOP_OK : (int)NNOP_ERR_HIP;
}

template <typename T, bool XA> int launch_act(int act, bool halves, const GluDecodeParams& p, dim3 grid, hipStream_t s) {
    switch (act) {
#define NNOP_GLU_CASE(A) \
        case A: return halves ? launch_gather<T, XA, A, true>(p, grid, s) : launch_gather<T, XA, A, false>(p, grid, s);
        NNOP_GLU_CASE(NNOP_GLU_SILU)
        NNOP_GLU_CASE(NNOP_GLU_GELU_TANH)
        NNOP_GLU_CASE(NNOP_GLU_GELU_ERF)
        NNOP_GLU_CASE(NNOP_GLU_SWIGLU_OAI)
#undef NNOP_GLU_CASE
    }
    return NNOP_ERR_OPTS;
}

}  // namespace

long long moe_mx_decode_glu_workgroups(const nnop_moe_mx_decode_glu_desc& d) {
    return (long long)d.experts * (((long long)d.inter_dim + kMoeMxDecodeGluCols - 1) / kMoeMxDecodeGluCols);
}

int launch_moe_mx_decode_glu(const nnop_moe_mx_decode_glu_desc& d, void* h, const void* x, const uint8_t* blocks, const uint8_t* scales,
                             const void* bias, const int32_t* offsets, const int32_t* perm, hipStream_t s) {
    GluDecodeParams p;
    p.h = h, p.x = x, p.blocks = blocks, p.scales = scales, p.bias = bias, p.offsets = offsets, p.perm = perm;
    p.ld_x = d.ld_x, p.ld_h = d.ld_h, p.ld_b = d.ld_b, p.ld_q = d.ld_q, p.ld_s = d.ld_s;
    p.S = d.rows, p.E = d.experts, p.K = d.in_dim, p.I = d.inter_dim;
    p.ct = (d.inter_dim + kMoeMxDecodeGluCols - 1) / kMoeMxDecodeGluCols;
    p.TK = perm ? (uint32_t)d.tokens * (uint32_t)d.topk : 0u;
    p.k = perm ? (uint32_t)d.topk : 1u;
    p.alpha = d.alpha, p.limit = d.limit;
    const bool halves = d.layout == NNOP_MOE_GLU_HALVES;
    const auto mult = [](long long v, long long m) { return v % m == 0; };
    const long long hb = halves ? 4 : 2;  // elements of one vector store of h
    p.hvec = mult(d.ld_h, hb) && mult((long long)(uintptr_t)h, 2 * hb);
    p.bvec = bias && mult(d.ld_b, 4) && mult((long long)(uintptr_t)bias, 8) && (!halves || mult(d.inter_dim, 4));
    const bool xa = mult(d.ld_x, 8) && aligned16({x});  // K is a multiple of 32
    const dim3 grid((unsigned)moe_mx_decode_glu_workgroups(d));
    return dispatch_dtype(d.dtype, [&](auto tag) {
        typedef typename decltype(tag)::type T;
        if constexpr (std::is_same<T, float>::value) {
            return (int)NNOP_ERR_DTYPE;  // the C boundary has refused it
        } else {
            return xa ? launch_act<T, true>(d.act, halves, p, grid, s) : launch_act<T, false>(d.act, halves, p, grid, s);
        }
    });
}

}  // namespace nnop
