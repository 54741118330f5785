// paged_prefill_fp8.hip -- the kernel of libnnop_hip_paged_prefill_fp8.so (include/nnop_hip_paged_prefill_fp8.h): paged_prefill.hip's
// attention of a variable number of new tokens per sequence, over pages that hold one-byte E4M3 codes with one fp32 scale per KV head.
//
// The kernel is paged_prefill_kernel.hpp's text with another staging policy.  The codes are expanded to the type of q in the registers
// that stage a tile, so the two LDS images of K and of V hold 16-bit elements exactly as in the thirteenth library, and the operand reads
// (ds_read_b128 for K, ds_read_b64_tr_b16 for V), the products, the softmax and the epilogue are that library's, statement for statement.
//
//   - Why at staging and not at the operand read (which is what the decode kernel, paged_attn_fp8.hip, does).  Decode is bandwidth-bound
//     and shares nothing: a wave converts what it alone consumes.  Prefill is matrix-bound and a tile is shared by all four waves:
//     expanding at the operand read would convert every tile four times, between an LDS read and the MFMA that waits for it.  At
//     staging a tile is converted once, by the 256 threads together, behind the products of the tile before -- where the 16-bit kernel
//     has nothing but its stores.
//   - global -> registers.  A tile of K is 32 rows of E bytes: E / 8 bytes per thread.  Thread tid holds piece tid % 8 of row tid / 8
//     -- 8 codes (one 8-byte load) at E = 64, 16 codes (one 16-byte load) at E = 128 -- so a wave's pieces are rows 8 w ... 8 w + 7,
//     inside the 16-key block w / 2 of the tile, whose table entry is therefore wave-uniform at both E (the 16-bit kernel at E = 128
//     needs two entries per thread, this one one).  V likewise.  The staging registers are half the 16-bit kernel's: 4 at E = 64, 8 at
//     E = 128.  The strides are bytes and multiples of 16, the pool's base is aligned to 16 and a piece starts at a multiple of its
//     size, so every load is naturally aligned.
//   - registers -> LDS.  v_cvt_scalef32_pk_{bf16,f16}_fp8 at scale 1.0f, two codes per instruction, right in front of the store: exact
//     for all 254 finite codes in both types, NaN for the two NaN codes.  The piece's 2 COLS bytes go to the offset the 16-bit kernel's
//     piece of the same columns has: one ds_write_b128 at E = 64, two at E = 128.  The conversions need four (eight) registers beyond
//     the piece for as long as the store takes, at the point of the loop where the score and P registers are dead.
//   - The scales never touch the codes: k_scale[kvh] multiplies scale2 = log2(e) / sqrt(E) once in the prologue, v_scale[kvh] the
//     epilogue's factor a / L once.  With both absent the factors are the 16-bit kernel's own, which is why that kernel's bits come out.
//
// The object takes paged_prefill.o's flags (the Makefile says why).  DESIGN.md section 4.23.
#include "paged_prefill_fp8.hpp"
#include "paged_prefill_kernel.hpp"
#include "host_common.hpp"

namespace nnop {
namespace {

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

// the two codes in the low (HI = false) or high half of w, as they stand in an image: element 0 in the low 16 bits
template <typename T> struct Cvt;
template <> struct Cvt<__bf16> {
    template <bool HI> static __device__ __forceinline__ unsigned pair(unsigned w) {
        return __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)w, 1.0f, HI));
    }
};
template <> struct Cvt<_Float16> {
    template <bool HI> static __device__ __forceinline__ unsigned pair(unsigned w) {
        return __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)w, 1.0f, HI));
    }
};

// eight codes, byte 0 of w0 first, as 16 bytes of an image row
template <typename T> __device__ __forceinline__ u32x4 expand8(unsigned w0, unsigned w1) {
    return u32x4{Cvt<T>::template pair<false>(w0), Cvt<T>::template pair<true>(w0), Cvt<T>::template pair<false>(w1),
                 Cvt<T>::template pair<true>(w1)};
}

struct PpFp8Params : PpParams {
    const float* k_scale;
    const float* v_scale;
};

// pages of E4M3 codes: a piece is an eighth of a row, E / 8 codes, and goes into the image as E / 8 elements of T
template <typename T, int E> struct PpStageFp8 {
    typedef PpFp8Params Params;
    typedef uint8_t elem;
    typedef typename std::conditional<E == 64, u32x2, u32x4>::type reg;
    static constexpr int RC = 8, CH = 1, COLS = E / 8;
    static __device__ __forceinline__ reg load(const elem* at) { return *reinterpret_cast<const reg*>(at); }
    static __device__ __forceinline__ void store(char* at, reg r) {
        *reinterpret_cast<u32x4*>(at) = expand8<T>(r[0], r[1]);
        if constexpr (E == 128) *reinterpret_cast<u32x4*>(at + 16) = expand8<T>(r[2], r[3]);
    }
    static __device__ __forceinline__ float scale2(const Params& p, int kvh) { return p.scale2 * (p.k_scale ? p.k_scale[kvh] : 1.f); }
    static __device__ __forceinline__ float out_factor(float inv, const Params& p, int kvh) { return inv * (p.v_scale ? p.v_scale[kvh] : 1.f); }
};

template <typename T, int E>
__global__ __launch_bounds__(kPpThreads) __attribute__((amdgpu_waves_per_eu(2, 2))) void paged_prefill_fp8_kernel(const PpFp8Params p) {
    paged_prefill_body<T, E, PpStageFp8<T, E>>(p);
}

template <typename T, int E> int launch(const PpFp8Params& p, long long groups, hipStream_t s) {
    hipLaunchKernelGGL((paged_prefill_fp8_kernel<T, E>), dim3((unsigned)groups), dim3(kPpThreads), 0, s, p);
    return hipGetLastError() == hipSuccess ? (int)NNOP_OK : (int)NNOP_ERR_HIP;
}

}  // namespace

int launch_paged_prefill_fp8(const nnop_paged_prefill_fp8_desc& d, void* o, float* lse, const void* q, const void* k, const void* v,
                             const float* k_scale, const float* v_scale, const int32_t* block_table, const int32_t* cu_seqlens_q,
                             const int32_t* seqlens, const float* sinks, hipStream_t stream) {
    PpFp8Params p;
    p.o = o, p.lse = lse, p.q = q, p.k = k, p.v = v, p.table = block_table, p.cu = cu_seqlens_q, p.seqlens = seqlens, p.sinks = sinks;
    p.k_scale = k_scale, p.v_scale = v_scale;
    paged_prefill_fill(p, d);  // the pools' strides are bytes here: PpStageFp8::elem
    const long long groups = d.kh * paged_prefill_max_blocks(d);
    if (d.dtype == NNOP_BF16) return d.emb == 64 ? launch<__bf16, 64>(p, groups, stream) : launch<__bf16, 128>(p, groups, stream);
    return d.emb == 64 ? launch<_Float16, 64>(p, groups, stream) : launch<_Float16, 128>(p, groups, stream);
}

}  // namespace nnop
