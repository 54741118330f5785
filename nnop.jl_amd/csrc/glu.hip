// glu.hip -- gated MLP activations y = act(gate) * up for gfx950 (HBM-streaming), forward and pullback.
//
// No counterpart in the reference.  The one element-wise step of a Llama / Gemma / gpt-oss MLP: SwiGLU, GeGLU (tanh and
// exact GELU) and the clamped gpt-oss SwiGLU.  Forward moves 3 row-sized arrays (the two-op form moves 5), the pullback 5
// (autograd of the two-op form: about 10); a and a' are recomputed from gate and up, nothing else is saved.
// Work item = one 16-byte chunk of an output row; consecutive lanes take consecutive chunks, then consecutive rows, so
// every load / store instruction of a wave is contiguous within a row.  Two addressing modes:
//   split        gate, up: two pointers with one row stride ld >= n (two dense matrices: ld = n; the halves of a fused
//                gate-up projection [rows][2n]: up = gate + n, ld = 2n); y, dy dense [rows][n]; dgate, dup strided like
//                gate, up (the padding between n and ld is never written)
//   interleaved  gu [rows][2n], gate = gu[:, 0::2], up = gu[:, 1::2] (gpt-oss); a lane loads 32 contiguous bytes and
//                de-interleaves in registers; dgu in the same layout
// Arithmetic in fp32, one rounding on store.  No LDS, no atomics, no workspace.
// Bound: HBM.
#include <limits.h>
#include "row_common.hpp"
#include "fa_launch.hpp"
#include "glu_act.hpp"

// Every path, layout and direction must give bitwise the same a(g) and a'(g): nothing below may be contracted into an
// FMA differently from one instantiation to the next.  Contraction is off for the whole file; where an FMA is wanted
// it is written out (fmaf).
#pragma clang fp contract(off)

namespace nnop {

struct GluParams {
    void *o0, *o1;                   // fwd: y, -;  bwd: dgate | dgu, dup | -
    const void *dy, *g, *u;          // interleaved: g = gu, u = nullptr
    long long n, ld;                 // row length of y; row stride of gate / up (elements)
    long long cpr, n_items;          // chunks per row of y, rows * cpr
    int small;                       // n_items < 2^32: the row / column split is a 32-bit division
    float alpha, limit;              // swiglu_oai
};

// Chunks in flight per lane.  Measured on MI355X (profiles/glu/perf_chunks_in_flight.jsonl): 2 is up to
// 8 % and 4 up to 10 % slower than 1 at the large shapes (8 waves per SIMD keep enough loads in flight; 4 costs occupancy).
#ifndef NNOP_GLU_U
#define NNOP_GLU_U 1
#endif

// ---- the activations: GluSig, glu_sigmoid, GluAct<>, glu_up, glu_fwd_elem, glu_bwd_elem live in glu_act.hpp (included above), which
// the decode forward with the activation in its epilogue (moe_mx_decode_glu.hip) compiles too.

// ---- the kernel -------------------------------------------------------------------------------------------------------
// VEC: elements per 16-byte chunk on the vector path (8 x 16-bit, 4 x fp32), 1 on the element-wise path (n or ld no
// multiple of that, or a base that is not 16-byte aligned).  IL: interleaved layout.  U: chunks in flight per lane; the
// U chunks of a lane are 256 chunks apart, so each of the U load instructions of a wave is contiguous.
// Every result is stored through round_store (row_common.hpp): the vector and the element path round alike.
// The pointers carry no __restrict__: an output may be the input it replaces (include/nnop_hip.h); a lane reads its
// chunk before it writes it, and no lane touches another lane's chunk.
template <typename T, int ACT, bool IL, bool BWD, int VEC, int U>
__global__ __launch_bounds__(256) void glu_kernel(const GluParams p) {
    typedef T tv __attribute__((ext_vector_type(VEC)));
    const long long base = (long long)blockIdx.x * (256 * U) + threadIdx.x;
    long long ig[U], io[U];          // element offsets: in gate / up (or gu), in y / dy
    bool live[U];
    tv gv[U], uv[U], dv[U];
#pragma unroll
    for (int k = 0; k < U; ++k) {
        const long long it = base + (long long)k * 256;
        live[k] = it < p.n_items;
        io[k] = it * VEC;
        if constexpr (IL) {
            ig[k] = 2 * io[k];
        } else if (p.ld == p.n) {
            ig[k] = io[k];
        } else {
            const long long row = p.small ? (long long)((uint32_t)it / (uint32_t)p.cpr) : it / p.cpr;
            ig[k] = row * p.ld + (it - row * p.cpr) * VEC;
        }
        if (live[k]) {
            if constexpr (IL) {
                // 2 VEC consecutive elements (g0 u0 g1 u1 ...) as two chunks
                const tv lo = *reinterpret_cast<const tv*>((const T*)p.g + ig[k]);
                const tv hi = *reinterpret_cast<const tv*>((const T*)p.g + ig[k] + VEC);
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    gv[k][j] = (2 * j < VEC) ? lo[(2 * j) % VEC] : hi[(2 * j) % VEC];
                    uv[k][j] = (2 * j + 1 < VEC) ? lo[(2 * j + 1) % VEC] : hi[(2 * j + 1) % VEC];
                }
            } else {
                gv[k] = *reinterpret_cast<const tv*>((const T*)p.g + ig[k]);
                uv[k] = *reinterpret_cast<const tv*>((const T*)p.u + ig[k]);
            }
            if constexpr (BWD) dv[k] = *reinterpret_cast<const tv*>((const T*)p.dy + io[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < U; ++k) {
        if (!live[k]) continue;
        if constexpr (!BWD) {
            tv y;
#pragma unroll
            for (int j = 0; j < VEC; ++j)
                y[j] = round_store<T>(glu_fwd_elem<ACT>(to_f32(gv[k][j]), to_f32(uv[k][j]), p.alpha, p.limit));
            *reinterpret_cast<tv*>((T*)p.o0 + io[k]) = y;
        } else {
            tv dg, du;
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                float a, b;
                glu_bwd_elem<ACT>(to_f32(dv[k][j]), to_f32(gv[k][j]), to_f32(uv[k][j]), p.alpha, p.limit, a, b);
                dg[j] = round_store<T>(a); du[j] = round_store<T>(b);
            }
            if constexpr (IL) {
                tv lo, hi;
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    if (2 * j < VEC) { lo[(2 * j) % VEC] = dg[j]; } else { hi[(2 * j) % VEC] = dg[j]; }
                    if (2 * j + 1 < VEC) { lo[(2 * j + 1) % VEC] = du[j]; } else { hi[(2 * j + 1) % VEC] = du[j]; }
                }
                *reinterpret_cast<tv*>((T*)p.o0 + ig[k]) = lo;
                *reinterpret_cast<tv*>((T*)p.o0 + ig[k] + VEC) = hi;
            } else {
                *reinterpret_cast<tv*>((T*)p.o0 + ig[k]) = dg;
                *reinterpret_cast<tv*>((T*)p.o1 + ig[k]) = du;
            }
        }
    }
}

template <typename T, int ACT, bool IL, bool BWD>
static int launch_glu_t(GluParams p, long long rows, hipStream_t s) {
    constexpr int V = 16 / (int)sizeof(T), U = NNOP_GLU_U;
    // the vector path issues 16-byte accesses at multiples of V elements from every base: all bases 16-byte aligned, n and
    // ld multiples of V (the halves of a packed projection, up = gate + n, pass exactly when n is).  Everything else --
    // odd n, an offset view, a misaligned half -- takes the element-wise instantiation.
    const bool vec = aligned16({p.o0, p.o1, p.dy, p.g, p.u}) && p.n % V == 0 && p.ld % V == 0;
    if (p.ld > (LLONG_MAX >> 4) / rows) return NNOP_ERR_SHAPE;                     // rows * ld in bytes fits 64 bits
    p.cpr = vec ? p.n / V : p.n;
    p.n_items = rows * p.cpr;
    p.small = p.n_items <= 0xffffffffLL;
    const long long grid = (p.n_items + 256 * U - 1) / (256 * U);
    if (grid <= 0 || grid > 0x7fffffffLL) return NNOP_ERR_SHAPE;
    if (vec) hipLaunchKernelGGL((glu_kernel<T, ACT, IL, BWD, V, U>), dim3((unsigned)grid), dim3(256), 0, s, p);
    else hipLaunchKernelGGL((glu_kernel<T, ACT, IL, BWD, 1, U>), dim3((unsigned)grid), dim3(256), 0, s, p);
    return hipGetLastError() == hipSuccess ? NNOP_OK : NNOP_ERR_HIP;
}

template <typename T, bool BWD> static int launch_glu_act(const nnop_glu_desc& d, const GluParams& p, hipStream_t s) {
    const bool il = d.layout == NNOP_GLU_INTERLEAVED;
    switch (d.act) {
#define NNOP_GLU_CASE(A) \
        case A: return il ? launch_glu_t<T, A, true, BWD>(p, d.rows, s) : launch_glu_t<T, A, false, BWD>(p, d.rows, s);
        NNOP_GLU_CASE(NNOP_GLU_SILU)
        NNOP_GLU_CASE(NNOP_GLU_GELU_TANH)
        NNOP_GLU_CASE(NNOP_GLU_GELU_ERF)
        NNOP_GLU_CASE(NNOP_GLU_SWIGLU_OAI)
#undef NNOP_GLU_CASE
    }
    return NNOP_ERR_OPTS;
}

template <bool BWD> static int launch_glu_any(const nnop_glu_desc& d, GluParams p, hipStream_t s) {
    p.n = d.n; p.ld = d.ld;
    p.alpha = d.alpha; p.limit = d.limit;
    p.cpr = p.n_items = 0; p.small = 0;                          // set per instantiation in launch_glu_t
    return dispatch_dtype(d.dtype, [&](auto t) { return launch_glu_act<typename decltype(t)::type, BWD>(d, p, s); });
}

int launch_glu(const nnop_glu_desc& d, void* y, const void* gate, const void* up, hipStream_t s) {
    GluParams p;
    p.o0 = y; p.o1 = nullptr; p.dy = nullptr; p.g = gate; p.u = up;
    return launch_glu_any<false>(d, p, s);
}

int launch_glu_bwd(const nnop_glu_desc& d, void* dgate, void* dup, const void* dy, const void* gate, const void* up,
                   hipStream_t s) {
    GluParams p;
    p.o0 = dgate; p.o1 = dup; p.dy = dy; p.g = gate; p.u = up;
    return launch_glu_any<true>(d, p, s);
}

}  // namespace nnop
