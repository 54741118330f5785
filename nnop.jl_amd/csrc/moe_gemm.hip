// moe_gemm.hip -- the grouped GEMM of libnnop_hip_moe_gemm.so (include/nnop_hip_moe_gemm.h): the expert GEMMs of a mixture-of-experts
// layer over the row ranges of the dispatch plan, and their two pullbacks.  gfx950 (MI355X) only.
//
// One kernel template, moe_gemm_kernel<T, PROD, ALIGNED>, computes
//     C[m][n] = sum_r A(m, r) B(n, r)
// on a 128 x 128 output tile: the shared tile body of moe_gemm_tile.hpp (staging, LDS images, MFMA order, bounds: documented there) with
// no epilogue and the output in the type of the operands.  The three products of this library:
//     PROD  product   m         n         r               A                        B
//     0     forward   slot row  n < N     c < K           xs   [m][r]  contiguous  w[e] [n][r]  contiguous      ("NT")
//     1     bwd_x     slot row  c < K     n < N           dys  [m][r]  contiguous  w[e] [r][n]  strided in r    ("NN")
//     2     bwd_w     n < N     c < K     s in [lo, hi)   dys  [r][m]  strided     xs   [r][n]  strided         ("TN")
#include "moe_gemm.hpp"
#include "moe_gemm_tile.hpp"
#include "host_common.hpp"
#include <type_traits>

namespace nnop {
namespace {

template <typename T, int PROD, bool ALIGNED> __global__ __launch_bounds__(kThreads) void moe_gemm_kernel(const GemmParams p) {
    moe_gemm_tile<T, PROD, ALIGNED, 0, T>(p, TileBias{nullptr, 0});
}

}  // namespace

long long moe_gemm_workgroups(MoeGemmProduct which, const nnop_moe_gemm_desc& d) {
    const long long S = d.rows, E = d.experts, K = d.in_dim, N = d.out_dim;
    if (which == kMoeGemmBwdW) return E * tiles_of(N) * tiles_of(K);
    return row_tile_slots(S, E) * tiles_of(which == kMoeGemmFwd ? N : K);
}

int launch_moe_gemm(MoeGemmProduct which, const nnop_moe_gemm_desc& d, void* out, const void* a, const void* b, const int32_t* offsets,
                    hipStream_t s) {
    const long long wgs = moe_gemm_workgroups(which, d);  // <= 2^31 - 1: the C boundary has checked it with the shape
    GemmParams p;
    p.out = out;
    p.a = a;
    p.b = b;
    p.offsets = offsets;
    p.S = d.rows;
    p.E = d.experts;
    p.wstride = (long long)d.out_dim * d.ld_w;
    p.M = 0;
    if (which == kMoeGemmFwd) {  // ys = xs w^T
        p.lda = d.ld_x, p.ldb = d.ld_w, p.ldc = d.ld_y;
        p.N = d.out_dim, p.R = d.in_dim;
    } else if (which == kMoeGemmBwdX) {  // dxs = dys w
        p.lda = d.ld_y, p.ldb = d.ld_w, p.ldc = d.ld_x;
        p.N = d.in_dim, p.R = d.out_dim;
    } else {  // dw[e] = dys[lo:hi]^T xs[lo:hi]
        p.lda = d.ld_y, p.ldb = d.ld_x, p.ldc = d.ld_w;
        p.M = d.out_dim, p.N = d.in_dim, p.R = 0;
    }
    p.nt = (int)tiles_of(p.N);
    p.mt = which == kMoeGemmBwdW ? (int)tiles_of(p.M) : (int)(wgs / p.nt);
    const bool fast = d.in_dim % 8 == 0 && d.out_dim % 8 == 0 && d.ld_x % 8 == 0 && d.ld_y % 8 == 0 && d.ld_w % 8 == 0 &&
                      aligned16({out, a, b});
    const dim3 grid((unsigned)wgs), block(kThreads);
    return dispatch_dtype(d.dtype, [&](auto tag) {
        typedef typename decltype(tag)::type T;
        auto go = [&](auto prod, auto al) {
            hipLaunchKernelGGL((moe_gemm_kernel<T, decltype(prod)::value, decltype(al)::value>), grid, block, 0, s, p);
        };
        auto with_path = [&](auto prod) {
            if (fast) go(prod, std::true_type{});
            else go(prod, std::false_type{});
        };
        if (which == kMoeGemmFwd) with_path(std::integral_constant<int, 0>{});
        else if (which == kMoeGemmBwdX) with_path(std::integral_constant<int, 1>{});
        else with_path(std::integral_constant<int, 2>{});
        return hipGetLastError() == hipSuccess ? NNOP_OK : NNOP_ERR_HIP;
    });
}

}  // namespace nnop
