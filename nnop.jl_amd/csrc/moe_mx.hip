// moe_mx.hip -- the kernels of libnnop_hip_moe_mx.so (include/nnop_hip_moe_mx.h): the expert linear layers on MXFP4 weights (forward and
// the pullback to the rows) and the two conversions between packed and plain weights.  gfx950 (MI355X) only.
//
// mx_convert8<T> (moe_mx.hpp) is the one place where a code becomes a number.  The dequant kernel and the staging of the two products
// both call it, so they cannot disagree.
//
// The two products are the tile of moe_gemm_tile.hpp with PackedStage in the place of the dense B stage.  Its pieces are the dense
// stage's -- PROD 0 (forward): 8 consecutive r of image row x are 4 packed bytes of weight row n0 + x and the scale byte of block r / 32;
// PROD 1 (bwd_x, the transposing stage): 8 consecutive x of reduction row r are 4 packed bytes of weight row r and the scale byte of
// block (n0 + x) / 32 -- so a thread fetches four 32-bit words and four scale bytes where the dense stage fetches four 16-byte pieces.
// load() only fetches; the words are expanded at the head of write(), behind the MFMAs of the step, so the wait for the weights lies
// where the dense stage has it and the staging registers between the two hold 8 words, not 16.  From there on write() is Stage's:
// the LDS image is the dense one byte for byte, and fragment reads, MFMA order, epilogue and bounds are the code of the sixth library.
// What does not exist (rows beyond the expert or N, r beyond the reduction) is not loaded: its word is 0 and its scale 127, which is +0.
//
// mxfp4_dequant_kernel: one thread per block of 32 -- a 16-byte load, the scale byte, four conversions, stores of 16 bytes.
// mxfp4_quant_kernel: four lanes per block of 32, eight elements each; amax over the magnitudes' bit patterns (ordered like the values)
// by two shuffles, floor(log2(amax)) from its exponent field (a subnormal amax: from its leading bit), |x| 2^-s by v_ldexp_f32, the code
// by seven compares against the midpoints with the tie rule in the choice of > and >=.  Off the hot path; not tuned.
#include "moe_mx.hpp"
#include "moe_gemm_tile.hpp"
#include "host_common.hpp"
#include <type_traits>

namespace nnop {
namespace {

// ---- the two products ---------------------------------------------------------------------------------------------------------------
struct MxSrc {
    const uint8_t* q;  // packed bytes of (x = 0, r = 0) of the step
    const uint8_t* s;  // its scale byte
    long long ld_s;
};
struct MxExtra {
    const uint8_t* scales;
    long long ld_s, sstride;  // bytes between two scale rows and between the scale matrices of two experts
};

// The B stage for packed weights [n][K / 2] + [n][K / 32]; GemmParams::b, ldb and wstride are the blocks, in bytes.
template <typename T, bool TR> struct PackedStage : Stage<T, TR, true> {
    static_assert(sizeof(T) == 2, "a reduction step of 64 elements: two blocks");
    typedef Stage<T, TR, true> Dense;
    typedef MxSrc Src;
    typedef MxExtra Extra;
    static constexpr int BK = kRowBytes / 2;
    uint32_t word[kPieces], scale[kPieces];

    static __device__ __forceinline__ Src origin(const GemmParams& p, const Extra& x, long long e, int n0) {
        const uint8_t* q = static_cast<const uint8_t*>(p.b) + e * p.wstride;
        const uint8_t* s = x.scales + e * x.sstride;
        return TR ? Src{q + n0 / 2, s + n0 / kMxBlock, x.ld_s} : Src{q + n0 * p.ldb, s + n0 * x.ld_s, x.ld_s};
    }
    static __device__ __forceinline__ Src advance(Src b, const GemmParams& p, const Extra&) {
        return TR ? Src{b.q + BK * p.ldb, b.s + BK * b.ld_s, b.ld_s} : Src{b.q + BK / 2, b.s + BK / kMxBlock, b.ld_s};
    }

    // xleft, rleft and `ld` (bytes) as Stage::load takes them.  A piece exists as a whole or not at all: along the packed axis the
    // extents are multiples of 32.
    __device__ __forceinline__ void load(Src b, long long ld, int xleft, int rleft, int t) {
#pragma unroll
        for (int p = 0; p < kPieces; ++p) {
            const int x = TR ? Dense::EPC * (t % Dense::XC) : t / 8 + 32 * p;
            const int r = TR ? 4 * (t / Dense::XC) + p : Dense::EPC * (t % 8);
            const int row = TR ? r : x, col = TR ? x : r;  // the weight row and the first of 8 elements along it
            uint32_t w = 0, e = 127;
            if (x < xleft && r < rleft) {
                w = *reinterpret_cast<const uint32_t*>(b.q + row * ld + col / 2);
                e = b.s[row * b.ld_s + col / kMxBlock];
            }
            word[p] = w;
            scale[p] = e;
        }
    }

    __device__ __forceinline__ void write(unsigned char* image, int t) {
#pragma unroll
        for (int p = 0; p < kPieces; ++p) this->v[p] = mx_convert8<T>(word[p], scale[p]);
        Dense::write(image, t);
    }
};

template <typename T, int PROD, bool ALIGNED, int EPI>
__global__ __launch_bounds__(kThreads) void moe_mx_kernel(const GemmParams p, const TileBias tb, const MxExtra xb) {
    moe_gemm_tile<T, PROD, ALIGNED, EPI, T, PackedStage<T, PROD != 0>>(p, tb, xb);
}

inline bool mult8(std::initializer_list<long long> v) {
    long long u = 0;
    for (long long x : v) u |= x;
    return (u & 7) == 0;
}

// ---- the conversions ------------------------------------------------------------------------------------------------------------------
struct MxRowsParams {
    void* rows;        // out (dequant) or in (quant)
    uint8_t* blocks;
    uint8_t* scales;
    long long total;   // threads that have work
    long long ld, ld_q, ld_s;
    int per_row;       // threads per row: K / 32 (dequant), K / 8 (quant)
};

template <typename T, bool ALIGNED> __global__ __launch_bounds__(kThreads) void mxfp4_dequant_kernel(const MxRowsParams p) {
    constexpr int EPC = 16 / (int)sizeof(T);
    typedef T tvec __attribute__((ext_vector_type(EPC)));
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= p.total) return;
    const long long row = i / p.per_row;
    const int blk = (int)(i - row * p.per_row);
    const uint4 q = *reinterpret_cast<const uint4*>(p.blocks + row * p.ld_q + 16 * blk);
    const uint32_t e = p.scales[row * p.ld_s + blk];
    const uint32_t words[4] = {q.x, q.y, q.z, q.w};
    T* dst = static_cast<T*>(p.rows) + row * p.ld + kMxBlock * blk;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const vec8<T> v = mx_convert8<T>(words[j], e);
        if (ALIGNED) {
#pragma unroll
            for (int h = 0; h < 8 / EPC; ++h) {
                tvec o;
#pragma unroll
                for (int k = 0; k < EPC; ++k) o[k] = v[EPC * h + k];
                *reinterpret_cast<tvec*>(dst + 8 * j + EPC * h) = o;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) dst[8 * j + k] = v[k];
        }
    }
}

template <typename T, bool ALIGNED> __global__ __launch_bounds__(kThreads) void mxfp4_quant_kernel(const MxRowsParams p) {
    constexpr int EPC = 16 / (int)sizeof(T);
    typedef T tvec __attribute__((ext_vector_type(EPC)));
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= p.total) return;  // the four lanes of a block leave together: total is a multiple of 4
    const long long row = i / p.per_row;
    const int piece = (int)(i - row * p.per_row);
    const T* src = static_cast<const T*>(p.rows) + row * p.ld + 8 * piece;
    float x[8];
    if (ALIGNED) {
#pragma unroll
        for (int h = 0; h < 8 / EPC; ++h) {
            const tvec v = *reinterpret_cast<const tvec*>(src + EPC * h);
#pragma unroll
            for (int k = 0; k < EPC; ++k) x[EPC * h + k] = (float)v[k];
        }
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = (float)src[k];
    }
    // the largest magnitude as a bit pattern: ordered like the values, Inf and NaN above every finite number
    uint32_t amax = 0, signs = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t bits = __builtin_bit_cast(uint32_t, x[k]);
        amax = max(amax, bits & 0x7fffffffu);
        signs |= (bits >> 31) << (4 * k + 3);
    }
    amax = max(amax, (uint32_t)__shfl_xor((int)amax, 1));
    amax = max(amax, (uint32_t)__shfl_xor((int)amax, 2));
    uint32_t e, word;
    if (amax >= 0x7f800000u) {
        e = 255, word = 0;
    } else if (amax == 0) {
        e = 0, word = signs;
    } else {
        const int field = (int)(amax >> 23);
        const int floor_log2 = field ? field - 127 : (31 - __clz((int)amax)) - 149;
        const int s = min(max(floor_log2 - 2, -127), 127);
        e = (uint32_t)(s + 127), word = signs;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float y = ldexpf(fabsf(x[k]), -s);  // < 8; exact unless below 2^-126, far under the first midpoint
            const uint32_t m = (y > 0.25f) + (y >= 0.75f) + (y > 1.25f) + (y >= 1.75f) + (y > 2.5f) + (y >= 3.5f) + (y > 5.f);
            word |= m << (4 * k);
        }
    }
    *reinterpret_cast<uint32_t*>(p.blocks + row * p.ld_q + 4 * piece) = word;
    if ((piece & 3) == 0) p.scales[row * p.ld_s + piece / 4] = (uint8_t)e;
}

}  // namespace

long long moe_mx_workgroups(bool bwd_x, const nnop_moe_mx_desc& d) {
    return row_tile_slots(d.rows, d.experts) * tiles_of(bwd_x ? d.in_dim : d.out_dim);
}

int launch_moe_mx_linear(bool bwd_x, const nnop_moe_mx_desc& d, void* out, const void* a, const uint8_t* blocks, const uint8_t* scales,
                         const void* bias, const int32_t* offsets, hipStream_t s) {
    const long long wgs = moe_mx_workgroups(bwd_x, d);  // <= 2^31 - 1: the C boundary has checked it with the shape
    const long long K = d.in_dim, N = d.out_dim;
    GemmParams p;
    p.out = out;
    p.a = a;
    p.b = blocks;
    p.offsets = offsets;
    p.S = d.rows;
    p.E = d.experts;
    p.M = 0;
    p.ldb = d.ld_q;
    p.wstride = N * d.ld_q;
    bool fast = mult8({K, N, d.ld_x, d.ld_y});
    if (!bwd_x) {  // ys = xs W^T + bias
        p.lda = d.ld_x, p.ldc = d.ld_y;
        p.N = d.out_dim, p.R = d.in_dim;
        fast = fast && mult8({bias ? d.ld_b : 0}) && aligned16({out, a, bias});
    } else {  // dxs = dys W
        p.lda = d.ld_y, p.ldc = d.ld_x;
        p.N = d.in_dim, p.R = d.out_dim;
        fast = fast && aligned16({out, a});
    }
    p.nt = (int)tiles_of(p.N);
    p.mt = (int)(wgs / p.nt);
    const TileBias tb{bias, d.ld_b};
    const MxExtra xb{scales, d.ld_s, N * d.ld_s};
    const dim3 grid((unsigned)wgs), block(kThreads);
    return dispatch_dtype(d.dtype, [&](auto tag) {
        typedef typename decltype(tag)::type T;
        if constexpr (std::is_same<T, float>::value) {
            return (int)NNOP_ERR_DTYPE;  // the C boundary has refused it
        } else {
            auto go = [&](auto pr, auto epi) {
                constexpr int PROD = decltype(pr)::value, EPI = decltype(epi)::value;
                if (fast) hipLaunchKernelGGL((moe_mx_kernel<T, PROD, true, EPI>), grid, block, 0, s, p, tb, xb);
                else hipLaunchKernelGGL((moe_mx_kernel<T, PROD, false, EPI>), grid, block, 0, s, p, tb, xb);
            };
            using I0 = std::integral_constant<int, 0>;
            using I1 = std::integral_constant<int, 1>;
            if (bwd_x) go(I1{}, I0{});
            else if (bias != nullptr) go(I0{}, I1{});
            else go(I0{}, I0{});
            return hipGetLastError() == hipSuccess ? (int)NNOP_OK : (int)NNOP_ERR_HIP;
        }
    });
}

namespace {
// rows of `dtype` that take 16-byte accesses
inline bool rows16(const nnop_mxfp4_desc& d, const void* rows) {
    return ((long long)d.ld * (long long)dtype_bytes(d.dtype)) % 16 == 0 && aligned16({rows});
}
inline MxRowsParams rows_params(const nnop_mxfp4_desc& d, const void* rows, const uint8_t* blocks, const uint8_t* scales, int per_thread) {
    MxRowsParams p;
    p.rows = const_cast<void*>(rows);
    p.blocks = const_cast<uint8_t*>(blocks);
    p.scales = const_cast<uint8_t*>(scales);
    p.per_row = d.cols / per_thread;
    p.total = d.rows * p.per_row;
    p.ld = d.ld, p.ld_q = d.ld_q, p.ld_s = d.ld_s;
    return p;
}
}  // namespace

int launch_mxfp4_dequant(const nnop_mxfp4_desc& d, void* out, const uint8_t* blocks, const uint8_t* scales, hipStream_t s) {
    const MxRowsParams p = rows_params(d, out, blocks, scales, kMxBlock);
    const dim3 grid((unsigned)((p.total + kThreads - 1) / kThreads)), block(kThreads);
    const bool fast = rows16(d, out);
    return dispatch_dtype(d.dtype, [&](auto tag) {
        typedef typename decltype(tag)::type T;
        if (fast) hipLaunchKernelGGL((mxfp4_dequant_kernel<T, true>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((mxfp4_dequant_kernel<T, false>), grid, block, 0, s, p);
        return hipGetLastError() == hipSuccess ? NNOP_OK : NNOP_ERR_HIP;
    });
}

int launch_mxfp4_quant(const nnop_mxfp4_desc& d, uint8_t* blocks, uint8_t* scales, const void* in, hipStream_t s) {
    const MxRowsParams p = rows_params(d, in, blocks, scales, 8);
    const dim3 grid((unsigned)((p.total + kThreads - 1) / kThreads)), block(kThreads);
    const bool fast = rows16(d, in);
    return dispatch_dtype(d.dtype, [&](auto tag) {
        typedef typename decltype(tag)::type T;
        if (fast) hipLaunchKernelGGL((mxfp4_quant_kernel<T, true>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((mxfp4_quant_kernel<T, false>), grid, block, 0, s, p);
        return hipGetLastError() == hipSuccess ? NNOP_OK : NNOP_ERR_HIP;
    });
}

}  // namespace nnop
