// moe_mx.hpp -- what nnop_moe_mx_capi.cpp needs of moe_mx.hip (libnnop_hip_moe_mx.so), and the MXFP4 conversion that moe_mx.hip and
// moe_mx_decode.hip (libnnop_hip_moe_mx_decode.so) both compile: header-only code, nothing is linked between the two libraries.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/nnop_hip_moe_mx.h"

namespace nnop {

constexpr int kMoeMxMaxExperts = 1024;
constexpr int kMoeMxMaxDim = 65536;
constexpr int kMxBlock = 32;                       // elements that share a scale byte
constexpr int kMxfp4MaxCols = 1 << 30;
constexpr long long kMxfp4MaxPieces = 1LL << 39;   // rows K / 8: the quantiser's threads, 256 to a workgroup

// the two products; the caller has checked moe_mx_workgroups() <= 2^31 - 1.  out / a are (ys, xs) or (dxs, dys); bias may be NULL and is
// read by the forward only
int launch_moe_mx_linear(bool bwd_x, const nnop_moe_mx_desc& d, void* out, const void* a, const uint8_t* blocks, const uint8_t* scales,
                         const void* bias, const int32_t* offsets, hipStream_t s);
// the number of workgroups a product would start, computed in 64 bits
long long moe_mx_workgroups(bool bwd_x, const nnop_moe_mx_desc& d);

int launch_mxfp4_dequant(const nnop_mxfp4_desc& d, void* out, const uint8_t* blocks, const uint8_t* scales, hipStream_t s);
int launch_mxfp4_quant(const nnop_mxfp4_desc& d, uint8_t* blocks, uint8_t* scales, const void* in, hipStream_t s);

// mx_convert8<T> is the one place where a code becomes a number: one 32-bit word (8 codes, element i in bits 4i ... 4i + 3) and the
// block's scale byte e become 8 values of T.  It is four v_cvt_scalef32_pk_{bf16,f16,f32}_fp4, each of which converts the two codes of
// one byte, the low nibble first, and applies the scale, which it takes from the exponent field of a float32: e << 23 is that float for
// every byte, 0 (2^-127) and 255 (NaN) included.  On the MI355X the instruction gives the header's value for all 16 x 256 (code, scale
// byte) pairs in the three types: subnormal results are kept, float16 results round to nearest even, too large a value becomes Inf, -0
// stays -0 (tests/test_zzzzzzzzz_moe_mx_gpu.py::test_exhaustive_table is that statement; another part has to pass it before it may run
// this).  An unnamed namespace, as in moe_gemm_tile.hpp: each library gets its own copy.
namespace {

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// the instruction of each type: the two codes of byte SEL of w, scaled by the power of two in the exponent field of `scale`
template <typename T> struct MxHw;
template <> struct MxHw<__bf16> {
    typedef bf16x2 pair;
    template <int SEL> static __device__ __forceinline__ pair cvt(uint32_t w, float scale) {
        return __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, SEL);
    }
};
template <> struct MxHw<_Float16> {
    typedef f16x2 pair;
    template <int SEL> static __device__ __forceinline__ pair cvt(uint32_t w, float scale) {
        return __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, scale, SEL);
    }
};
template <> struct MxHw<float> {
    typedef f32x2 pair;
    template <int SEL> static __device__ __forceinline__ pair cvt(uint32_t w, float scale) {
        return __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, scale, SEL);
    }
};

template <typename T> using vec8 = T __attribute__((ext_vector_type(8)));

template <typename T> __device__ __forceinline__ vec8<T> mx_convert8(uint32_t w, uint32_t e) {
    typedef MxHw<T> Hw;
    const float scale = __builtin_bit_cast(float, e << 23);
    const typename Hw::pair p0 = Hw::template cvt<0>(w, scale), p1 = Hw::template cvt<1>(w, scale);
    const typename Hw::pair p2 = Hw::template cvt<2>(w, scale), p3 = Hw::template cvt<3>(w, scale);
    return vec8<T>{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
}

}  // namespace

}  // namespace nnop
