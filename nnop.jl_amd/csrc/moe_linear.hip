// moe_linear.hip -- the kernels of libnnop_hip_moe_linear.so (include/nnop_hip_moe_linear.h): the expert linear layers of a
// mixture-of-experts layer with a per-expert bias, weights in [E][N][K] or [E][K][N] order, and accumulating weight and bias gradients.
// gfx950 (MI355X) only.
//
// The three products are the shared tile body of moe_gemm_tile.hpp (staging, LDS images, MFMA order, bounds: documented there) behind
// moe_linear_kernel<T, PROD, ALIGNED, EPI, OutT>.  The weight layout is launcher work alone -- it decides which of the three stagings a
// call takes and what the tile's m, n, r are; W_e(n, c) is the coefficient of input c in output n:
//     call     layout     PROD        A (m, r)          B (n, r)                      C            n of the tile   r
//     forward  [E][N][K]  0 "NT"      xs  [s][c]        w[e] [n][c]  contiguous       ys  [s][n]   output n < N    c < K
//     forward  [E][K][N]  1 "NN"      xs  [s][c]        w[e] [c][n]  strided in r     ys  [s][n]   output n < N    c < K
//     bwd_x    [E][N][K]  1 "NN"      dys [s][n]        w[e] [n][c]  strided in r     dxs [s][c]   input  c < K    n < N
//     bwd_x    [E][K][N]  0 "NT"      dys [s][n]        w[e] [c][n]  contiguous       dxs [s][c]   input  c < K    n < N
//     bwd_w    [E][N][K]  2 "TN"      dys [s][n]  m = n xs  [s][c]   n = c            dw[e] [n][c]                 s in [lo, hi)
//     bwd_w    [E][K][N]  2 "TN"      xs  [s][c]  m = c dys [s][n]   n = n            dw[e] [c][n]                 s in [lo, hi)
// The forward of either layout ends with the tile's n running over output features, so the bias epilogue (EPI 1) exists for PROD 0 and 1
// and reads bias[e][n0 + n].  A forward without bias and bwd_x take EPI 0.  bwd_w takes EPI 0 or, accumulating, EPI 2, each with OutT = T
// or, for an fp32 gradient beside 16-bit operands, float.  Nothing else is instantiated.
//
// moe_linear_bias_bwd_kernel is the one kernel that is not a GEMM: db[e][n] = sum of dys[s][n] over the expert's rows, a segmented column
// sum that reads every byte of dys once.  One workgroup owns (expert, a chunk of CL * EPC columns); EPC = 16 bytes of elements, CL (a power
// of two <= 64, the smallest that covers N) lanes lie along the columns and 256 / CL row lanes along the rows, so a row of the chunk is
// read as up to 1 KiB of consecutive 16-byte loads.  Row lane l takes rows lo + l, lo + l + 256 / CL, ... in ascending order, four loads in
// flight per thread, and adds them in that order in fp32; the row lanes' sums meet in LDS and are added in ascending l by the thread that
// stores the column: an order that depends on N and the element type, not on the grid, the data or what ran before.  No atomics.
#include "moe_linear.hpp"
#include "moe_gemm_tile.hpp"
#include "host_common.hpp"
#include <type_traits>

namespace nnop {
namespace {

template <typename T, int PROD, bool ALIGNED, int EPI, typename OutT>
__global__ __launch_bounds__(kThreads) void moe_linear_kernel(const GemmParams p, const TileBias tb) {
    moe_gemm_tile<T, PROD, ALIGNED, EPI, OutT>(p, tb);
}

struct BiasBwdParams {
    void* db;
    const void* dys;
    const int32_t* offsets;
    long long ld_y, ld_db;
    int S, N;
    int cl_log2;     // CL = 1 << cl_log2 lanes along the columns
    int accumulate;
};
constexpr int kBiasRowsInFlight = 4;

template <typename T, typename OutT, bool ALIGNED>
__global__ __launch_bounds__(kThreads) void moe_linear_bias_bwd_kernel(const BiasBwdParams p) {
    constexpr int EPC = 16 / (int)sizeof(T);
    typedef T tvec __attribute__((ext_vector_type(EPC)));
    __shared__ float part[kThreads * EPC];  // [row lane][CL * EPC columns]

    const int t = threadIdx.x, e = blockIdx.x;
    const int cg = t & ((1 << p.cl_log2) - 1), rl = t >> p.cl_log2, rg = kThreads >> p.cl_log2;
    const int width = EPC << p.cl_log2, c0 = blockIdx.y * width;  // c0 < N: the grid has ceil(N / width) chunks
    const int lo = clamped_offset(p.offsets, e, p.S), hi = clamped_offset(p.offsets, e + 1, p.S);
    if (p.accumulate && hi <= lo) return;  // nothing to add: db[e] keeps its bits

    const int c = c0 + EPC * cg, cleft = p.N - c;  // this thread's EPC columns; cleft of them exist
    float acc[EPC];
#pragma unroll
    for (int i = 0; i < EPC; ++i) acc[i] = 0.f;
    if (cleft > 0) {
        const T* src = static_cast<const T*>(p.dys) + c;
        for (long long r = (long long)lo + rl; r < hi; r += (long long)kBiasRowsInFlight * rg) {
            tvec v[kBiasRowsInFlight];
#pragma unroll
            for (int u = 0; u < kBiasRowsInFlight; ++u) {
                const long long rr = r + (long long)u * rg;
                tvec z;
#pragma unroll
                for (int i = 0; i < EPC; ++i) z[i] = (T)0.f;
                if (rr < hi) {
                    const T* row = src + rr * p.ld_y;
                    if (ALIGNED) {
                        z = *reinterpret_cast<const tvec*>(row);  // N % 8 == 0: the piece exists as a whole
                    } else {
#pragma unroll
                        for (int i = 0; i < EPC; ++i)
                            if (i < cleft) z[i] = row[i];
                    }
                }
                v[u] = z;
            }
#pragma unroll
            for (int u = 0; u < kBiasRowsInFlight; ++u)
#pragma unroll
                for (int i = 0; i < EPC; ++i) acc[i] += (float)v[u][i];
        }
    }
#pragma unroll
    for (int i = 0; i < EPC; ++i) part[rl * width + EPC * cg + i] = acc[i];
    __syncthreads();
    OutT* dst = static_cast<OutT*>(p.db) + (long long)e * p.ld_db + c0;
    for (int col = t; col < width; col += kThreads) {
        if (c0 + col >= p.N) break;
        float sum = part[col];
        for (int l = 1; l < rg; ++l) sum += part[l * width + col];
        dst[col] = (OutT)(p.accumulate ? (float)dst[col] + sum : sum);
    }
}

inline bool kn(const nnop_moe_linear_desc& d) { return (d.flags & NNOP_MOE_LINEAR_KN) != 0; }
inline bool mult8(std::initializer_list<long long> v) {
    long long u = 0;
    for (long long x : v) u |= x;
    return (u & 7) == 0;
}
// CL of the bias gradient as log2: the smallest power of two with CL * EPC >= N, at most 64
inline int bias_cl_log2(int N, int epc) {
    int s = 0;
    while (s < 6 && (epc << s) < N) ++s;
    return s;
}

}  // namespace

long long moe_linear_workgroups(MoeLinearCall which, const nnop_moe_linear_desc& d) {
    const long long S = d.rows, E = d.experts, K = d.in_dim, N = d.out_dim;
    if (which == kMoeLinearBwdW) return E * tiles_of(N) * tiles_of(K);
    if (which == kMoeLinearBwdB) {
        const int epc = 16 / (int)dtype_bytes(d.dtype);
        const long long width = (long long)epc << bias_cl_log2(d.out_dim, epc);
        return E * ((N + width - 1) / width);
    }
    return row_tile_slots(S, E) * tiles_of(which == kMoeLinearFwd ? N : K);
}

int launch_moe_linear(MoeLinearCall which, const nnop_moe_linear_desc& d, void* out, const void* a, const void* b, const void* bias,
                      const int32_t* offsets, hipStream_t s) {
    const long long wgs = moe_linear_workgroups(which, d);  // <= 2^31 - 1: the C boundary has checked it with the shape
    const long long K = d.in_dim, N = d.out_dim;
    GemmParams p;
    p.out = out;
    p.a = a;
    p.b = b;
    p.offsets = offsets;
    p.S = d.rows;
    p.E = d.experts;
    p.M = 0;
    int prod;
    bool fast = mult8({K, N});
    if (which == kMoeLinearFwd) {  // ys = xs W^T + bias
        prod = kn(d) ? 1 : 0;
        p.lda = d.ld_x, p.ldb = d.ld_w, p.ldc = d.ld_y;
        p.N = d.out_dim, p.R = d.in_dim;
        p.wstride = (kn(d) ? K : N) * d.ld_w;
        fast = fast && mult8({d.ld_x, d.ld_w, d.ld_y, bias ? d.ld_b : 0}) && aligned16({out, a, b, bias});
    } else if (which == kMoeLinearBwdX) {  // dxs = dys W
        prod = kn(d) ? 0 : 1;
        p.lda = d.ld_y, p.ldb = d.ld_w, p.ldc = d.ld_x;
        p.N = d.in_dim, p.R = d.out_dim;
        p.wstride = (kn(d) ? K : N) * d.ld_w;
        fast = fast && mult8({d.ld_x, d.ld_w, d.ld_y}) && aligned16({out, a, b});
    } else {  // dW_e = dys[lo:hi]^T xs[lo:hi], or its transpose: the operands change places
        prod = 2;
        if (kn(d)) {
            p.a = b, p.b = a;
            p.lda = d.ld_x, p.ldb = d.ld_y;
            p.M = d.in_dim, p.N = d.out_dim;
        } else {
            p.lda = d.ld_y, p.ldb = d.ld_x;
            p.M = d.out_dim, p.N = d.in_dim;
        }
        p.ldc = d.ld_dw, p.R = 0;
        p.wstride = (kn(d) ? K : N) * d.ld_dw;
        fast = fast && mult8({d.ld_x, d.ld_y, d.ld_dw}) && aligned16({out, a, b});
    }
    p.nt = (int)tiles_of(p.N);
    p.mt = prod == 2 ? (int)tiles_of(p.M) : (int)(wgs / p.nt);
    const TileBias tb{bias, d.ld_b};
    const bool acc = (d.flags & NNOP_MOE_LINEAR_ACCUMULATE) != 0, wide = d.grad_dtype != d.dtype;
    const dim3 grid((unsigned)wgs), block(kThreads);
    return dispatch_dtype(d.dtype, [&](auto tag) {
        typedef typename decltype(tag)::type T;
        auto go = [&](auto pr, auto al, auto epi, auto otag) {
            typedef typename decltype(otag)::type OutT;
            hipLaunchKernelGGL((moe_linear_kernel<T, decltype(pr)::value, decltype(al)::value, decltype(epi)::value, OutT>), grid, block, 0, s,
                               p, tb);
        };
        auto with_path = [&](auto pr, auto epi, auto otag) {
            if (fast) go(pr, std::true_type{}, epi, otag);
            else go(pr, std::false_type{}, epi, otag);
        };
        using I0 = std::integral_constant<int, 0>;
        using I1 = std::integral_constant<int, 1>;
        using I2 = std::integral_constant<int, 2>;
        if (prod == 2) {
            auto with_epi = [&](auto otag) {
                if (acc) with_path(I2{}, I2{}, otag);
                else with_path(I2{}, I0{}, otag);
            };
            if constexpr (!std::is_same<T, float>::value) {
                if (wide) with_epi(TypeTag<float>{});
                else with_epi(tag);
            } else {
                with_epi(tag);
            }
        } else {
            const bool with_bias = which == kMoeLinearFwd && bias != nullptr;
            auto with_epi = [&](auto pr) {
                if (with_bias) with_path(pr, I1{}, tag);
                else with_path(pr, I0{}, tag);
            };
            if (prod == 0) with_epi(I0{});
            else with_epi(I1{});
        }
        return hipGetLastError() == hipSuccess ? NNOP_OK : NNOP_ERR_HIP;
    });
}

int launch_moe_linear_bias_bwd(const nnop_moe_linear_desc& d, void* db, const void* dys, const int32_t* offsets, hipStream_t s) {
    const int epc = 16 / (int)dtype_bytes(d.dtype);
    BiasBwdParams p;
    p.db = db;
    p.dys = dys;
    p.offsets = offsets;
    p.ld_y = d.ld_y, p.ld_db = d.ld_db;
    p.S = d.rows, p.N = d.out_dim;
    p.cl_log2 = bias_cl_log2(d.out_dim, epc);
    p.accumulate = (d.flags & NNOP_MOE_LINEAR_ACCUMULATE) != 0;
    const long long width = (long long)epc << p.cl_log2;
    const dim3 grid((unsigned)d.experts, (unsigned)((d.out_dim + width - 1) / width)), block(kThreads);
    const bool fast = mult8({d.out_dim, d.ld_y}) && aligned16({dys}), wide = d.grad_dtype != d.dtype;
    return dispatch_dtype(d.dtype, [&](auto tag) {
        typedef typename decltype(tag)::type T;
        auto go = [&](auto otag) {
            typedef typename decltype(otag)::type OutT;
            if (fast) hipLaunchKernelGGL((moe_linear_bias_bwd_kernel<T, OutT, true>), grid, block, 0, s, p);
            else hipLaunchKernelGGL((moe_linear_bias_bwd_kernel<T, OutT, false>), grid, block, 0, s, p);
        };
        if constexpr (!std::is_same<T, float>::value) {
            if (wide) go(TypeTag<float>{});
            else go(tag);
        } else {
            go(tag);
        }
        return hipGetLastError() == hipSuccess ? NNOP_OK : NNOP_ERR_HIP;
    });
}

}  // namespace nnop
