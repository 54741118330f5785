// moe_mx_decode.hip -- the kernel of libnnop_hip_moe_mx_decode.so (include/nnop_hip_moe_mx_decode.h): the forward of the expert linear
// layer on MXFP4 weights for few rows per expert.  gfx950 (MI355X) only.
//
// The 128 x 128 tile of moe_mx.hip keeps one reduction step of loads in flight per workgroup; with a handful of rows per expert its time is
// the number of steps times one trip to memory.  This kernel streams the packed weights once, from global memory straight into the
// registers of the lane that feeds them to the matrix cores, with a ring of loads in flight per wave, and has no LDS and no barrier.
//
// Work: workgroup (e, c) is expert e and the output columns (weight rows) 256 c ... 256 c + 255, all of K; the grid is E ceil(N / 256),
// fixed on the host.  offsets[e], offsets[e+1] are read here and clamped into [0, S].  Wave w owns kNT = 4 MFMA row tiles of 16 weight
// rows, 64 in all.  The pass of a wave over K -- the ring of loads in flight, the clamped addresses, the selection at the consumer, the
// MFMAs -- is decode_ring of moe_mx_decode_ring.hpp, which the ninth library (moe_mx_decode_glu.hip) instantiates too; this kernel gives
// it the tiles n0 + 16 i, the x rows of the pass (a slot m >= the pass's rows reads the pass's first row, which the lanes of slot 0 fetch
// anyway: no further traffic) and the store below.  acc[tile][g] ends as 4 consecutive n (4 q ... 4 q + 3) of row m.  Masking is by
// selection: no byte of another expert, of a row outside this expert or of padding enters a product.
//
// Rows: an expert with up to 16 rows takes one accumulator group per tile in one pass over its weights, up to 32 two (the x pieces of the
// second group ride in the same ring); more rows loop over passes of 32, which find the workgroup's 256 weight rows in L2.  The sum of
// one output element runs over the steps in ascending order and over i = 0 ... 3 inside a step, into one fp32 accumulator: a function of
// K and the type alone.  An MFMA's output (m, n) depends on operand row m and column n only, so a row's bits do not depend on the plan,
// on its slot, on the group count or on its neighbours.
//
// Epilogue: the bias in fp32, one rounding, 8-byte stores where ld_y (with a bias: ld_b) is a multiple of 4, the bases are 8-byte aligned
// and the 4 columns exist, element-wise stores otherwise.  The rows in front of offsets[0] are written as +0 by the workgroups of expert
// 0, those behind offsets[E] by the workgroups of expert E - 1, each in its own columns, before they look at their expert's rows; a
// workgroup whose expert has no rows returns after that, before any weight load.
#include "moe_mx_decode.hpp"
#include "moe_mx_decode_ring.hpp"
#include "host_common.hpp"
#include <type_traits>

namespace nnop {
namespace {

constexpr int kWaveCols = 16 * kNT;
static_assert(kWaveCols * (kThreads / 64) == kMoeMxDecodeCols, "four waves cover the workgroup's columns");

struct DecodeParams {
    void* ys;
    const void* xs;
    const uint8_t* blocks;
    const uint8_t* scales;
    const void* bias;  // NULL: none
    const int32_t* offsets;
    long long ld_x, ld_y, ld_b;  // elements
    long long ld_q, ld_s;        // bytes
    int S, E, K, N;
    int ct;   // column groups per expert
    int vec;  // ys (and bias) take 8-byte accesses
};

// rows r0 ... r1 - 1 of the workgroup's columns c0 ... c0 + 255 become +0
template <typename T> __device__ __forceinline__ void zero_rows(const DecodeParams& p, int r0, int r1, int c0, int t) {
    typedef T t4 __attribute__((ext_vector_type(4)));
    const int c = c0 + 4 * (t & 63);
    if (c >= p.N) return;
    const T z = (T)0.f;
    for (int r = r0 + (t >> 6); r < r1; r += kThreads / 64) {
        T* dst = static_cast<T*>(p.ys) + r * p.ld_y + c;
        if (p.vec && c + 3 < p.N) {
            *reinterpret_cast<t4*>(dst) = t4{z, z, z, z};
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (c + j < p.N) dst[j] = z;
        }
    }
}

// One pass of a wave: rows m0 ... m0 + rows - 1 (rows <= 16 G) of expert e against weight rows n0 ... n0 + 63, all of K, on the ring of
// moe_mx_decode_ring.hpp: tile i starts at weight row n0 + 16 i, a lane's x row of group g is row m0 + 16 g + lane % 16 (a slot beyond the
// pass's rows reads the pass's first row, which the lanes of slot 0 fetch anyway: no further traffic), and the epilogue is the store below.
template <typename T, bool XA, int G> __device__ __forceinline__ void decode_pass(const DecodeParams& p, int e, int n0, int m0, int rows, int lane) {
    typedef T t4 __attribute__((ext_vector_type(4)));
    const int fr = lane & 15, fq = lane >> 4;
    const RingWeights w{p.blocks, p.scales, p.ld_q, p.ld_s, p.K, p.N};
    int base[kNT], end[kNT];
#pragma unroll
    for (int i = 0; i < kNT; ++i) base[i] = n0 + 16 * i, end[i] = p.N;
    const T* xr[G];
    bool xok[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int m = 16 * g + fr;
        xok[g] = m < rows;
        xr[g] = static_cast<const T*>(p.xs) + (long long)(m0 + (xok[g] ? m : 0)) * p.ld_x;
    }
    decode_ring<T, XA, G>(w, e, base, end, xr, xok, lane, [&](const f32x4 (&acc)[kNT][G]) {
        // acc[i][g][j] is ys[m0 + 16 g + fr][n0 + 16 i + 4 fq + j]
        const T* bias = p.bias ? static_cast<const T*>(p.bias) + e * p.ld_b : nullptr;
#pragma unroll
        for (int i = 0; i < kNT; ++i) {
            const int n = n0 + 16 * i + 4 * fq;
            if (n >= p.N) continue;
            const bool whole = p.vec && n + 3 < p.N;
            f32x4 bv = f32x4{0.f, 0.f, 0.f, 0.f};
            if (bias != nullptr) {
                if (whole) {
                    const t4 v = *reinterpret_cast<const t4*>(bias + n);
#pragma unroll
                    for (int j = 0; j < 4; ++j) bv[j] = (float)v[j];
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (n + j < p.N) bv[j] = (float)bias[n + j];
                }
            }
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const int m = 16 * g + fr;
                if (m >= rows) continue;
                const f32x4 v = acc[i][g] + bv;
                T* dst = static_cast<T*>(p.ys) + (long long)(m0 + m) * p.ld_y + n;
                if (whole) {
                    *reinterpret_cast<t4*>(dst) = t4{(T)v[0], (T)v[1], (T)v[2], (T)v[3]};
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (n + j < p.N) dst[j] = (T)v[j];
                }
            }
        }
    });
}

template <typename T, bool XA> __global__ __launch_bounds__(kThreads) void moe_mx_decode_kernel(const DecodeParams p) {
    const int t = threadIdx.x;
    const int e = blockIdx.x / (unsigned)p.ct, c0 = (blockIdx.x % (unsigned)p.ct) * kMoeMxDecodeCols;
    const int lo = clamped_offset(p.offsets, e, p.S), hi = clamped_offset(p.offsets, e + 1, p.S);
    if (e == 0) zero_rows<T>(p, 0, lo, c0, t);
    if (e == p.E - 1) zero_rows<T>(p, hi, p.S, c0, t);
    if (hi <= lo) return;  // no rows: no weight byte is loaded
    const int n0 = c0 + (t >> 6) * kWaveCols;
    if (n0 >= p.N) return;  // no barrier follows: a wave without columns may leave
    for (int m0 = lo; m0 < hi; m0 += 16 * kMaxGroups) {
        const int rows = min(hi - m0, 16 * kMaxGroups);
        if (kMaxGroups == 1 || rows <= 16) decode_pass<T, XA, 1>(p, e, n0, m0, rows, t & 63);
        else decode_pass<T, XA, kMaxGroups>(p, e, n0, m0, rows, t & 63);
    }
}

}  // namespace

long long moe_mx_decode_workgroups(const nnop_moe_mx_decode_desc& d) {
    return (long long)d.experts * (((long long)d.out_dim + kMoeMxDecodeCols - 1) / kMoeMxDecodeCols);
}

int launch_moe_mx_decode_linear(const nnop_moe_mx_decode_desc& d, void* ys, const void* xs, const uint8_t* blocks, const uint8_t* scales,
                                const void* bias, const int32_t* offsets, hipStream_t s) {
    DecodeParams p;
    p.ys = ys, p.xs = xs, p.blocks = blocks, p.scales = scales, p.bias = bias, p.offsets = offsets;
    p.ld_x = d.ld_x, p.ld_y = d.ld_y, p.ld_b = d.ld_b, p.ld_q = d.ld_q, p.ld_s = d.ld_s;
    p.S = d.rows, p.E = d.experts, p.K = d.in_dim, p.N = d.out_dim;
    p.ct = (d.out_dim + kMoeMxDecodeCols - 1) / kMoeMxDecodeCols;
    const auto mult = [](long long v, long long m) { return v % m == 0; };
    p.vec = mult(d.ld_y, 4) && mult((long long)(uintptr_t)ys, 8) && (!bias || (mult(d.ld_b, 4) && mult((long long)(uintptr_t)bias, 8)));
    const bool xa = mult(d.ld_x, 8) && aligned16({xs});  // K is a multiple of 32
    const dim3 grid((unsigned)moe_mx_decode_workgroups(d)), block(kThreads);
    return dispatch_dtype(d.dtype, [&](auto tag) {
        typedef typename decltype(tag)::type T;
        if constexpr (std::is_same<T, float>::value) {
            return (int)NNOP_ERR_DTYPE;  // the C boundary has refused it
        } else {
            if (xa) hipLaunchKernelGGL((moe_mx_decode_kernel<T, true>), grid, block, 0, s, p);
            else hipLaunchKernelGGL((moe_mx_decode_kernel<T, false>), grid, block, 0, s, p);
            return hipGetLastError() == hipSuccess ? (int)NNOP_OK : (int)NNOP_ERR_HIP;
        }
    });
}

}  // namespace nnop
