// moe_rows.hip -- the row movers of a mixture-of-experts layer for gfx950: include/nnop_hip_moe_data.h.
//
// Three kernels, one template each over the element type and the piece width VEC: VEC = 16 / sizeof(T) moves a row in 16-byte pieces
// (D, both strides and every base allow it), VEC = 1 is the element-wise path of the same structure.  A row is `pieces` = D / VEC
// pieces; piece c of a row belongs to lane c % 64 of the wave that owns its 64-piece run, so every load and store instruction of a
// wave covers one contiguous segment (1 KiB in the 16-byte path), as RowRegs arranges it.
//
//  * gather (slot-major: permute; ZERO_ONLY: the skipped rows of dys): a wave per slot row and column chunk of 64 GPP pieces, four
//    rows per workgroup.  perm[s] is one load per wave (a wave-uniform address, read back with v_readfirstlane), t = perm[s] / k one
//    scalar unsigned division; the GPP loads are issued together, then the stores; a skipped slot stores zeros and loads nothing.
//    The row is never converted: a bit-for-bit copy.
//  * reduce (token-major: combine, and permute_bwd with w == nullptr): a wave per token and column chunk of 64 RPP pieces.  Lane j
//    loads slot[t][j] and w[t][j] once (k <= 64) and the wave reads them back lane by lane.  The slot rows are loaded in batches of
//    RJB values of j -- RJB RPP independent 16-byte loads per lane in flight -- and accumulated in fp32 in ascending j; one rounding
//    on the store (round_store).  A skipped j contributes nothing (it is not a product with zero: a NaN weight there stays out).
//  * combine_bwd (token-major, a group of G = 64 or 256 lanes per token): dy[t] is read once and held in registers where the row fits
//    the group (pieces <= G CPP), re-read per pair of j from the cache otherwise.  Two values of j at a time: the ys row pieces are
//    loaded, the lane's part of both dot products is accumulated in fp32 in piece order, w[t][j] dy[t] is rounded and stored to row
//    slot[t][j] of dys, and the pair of partial sums folds through wave_allreduce and, for G = 256, one LDS hop (Sum2).  The order
//    of that sum is a function of (D, VEC, G) alone.  The rows of dys no valid slot names get their zeros from the ZERO_ONLY gather
//    launched behind it, which looks only at perm[s].
// No atomics, no workspace: every store is a vector store of a lane's own piece (or of dw by one lane).
//
// Bounds: an index v is used only behind (uint32_t)v < S, so a row offset is below S ld_slot resp. T ld_tok (64-bit arithmetic: S
// ld_slot passes 2^31 at 65536 tokens x 8 x 4096), a column is used only behind piece < pieces, and w / dw are indexed by t k + j
// with t < T, j < k, or by a valid perm[s] < S.  Rows are walked by a grid-stride loop, so the grid stays small whatever S is.
#include "row_common.hpp"
#include "moe_data.hpp"

namespace nnop {

struct MoeRowsParams {
    void* out;               // gather: xs;  reduce: y / dx;  combine_bwd: dys
    const void* in;          // gather: x;   reduce: ys / dxs;  combine_bwd: ys
    const void* dy;          // combine_bwd
    float* dw;               // combine_bwd
    const float* w;          // reduce: nullptr = every weight 1;  combine_bwd
    const int32_t* perm;
    const int32_t* slot;
    int T, K, S, pieces;     // pieces = D / VEC
    long long ld_tok, ld_slot;
};

constexpr int kGatherPieces = 4;     // GPP: pieces per lane of a gather wave
constexpr int kReducePieces = 2;     // RPP
constexpr int kReduceBatch = 4;      // RJB
constexpr int kCombinePieces = 4;    // CPP
constexpr int kMaxRowBlocks = 1 << 20;

// VEC elements of a row: 16 bytes, or one element
template <typename T, int VEC> struct Piece {
    typedef T tv __attribute__((ext_vector_type(VEC)));
    tv v;
    NNOP_DEV void zero() {
#pragma unroll
        for (int i = 0; i < VEC; ++i) v[i] = from_f32<T>(0.f);
    }
    NNOP_DEV void load(const T* __restrict__ p) { v = *reinterpret_cast<const tv*>(p); }
    NNOP_DEV void store(T* __restrict__ p) const { *reinterpret_cast<tv*>(p) = v; }
    NNOP_DEV float get(int i) const { return to_f32(v[i]); }
    NNOP_DEV void set(int i, T x) { v[i] = x; }
};

NNOP_DEV int wave_id() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }
NNOP_DEV bool moe_valid(int32_t v, int S) { return (uint32_t)v < (uint32_t)S; }

// ---- gather -------------------------------------------------------------------------------------------------------------------------
// grid (row blocks, column chunks), 256 lanes = 4 slot rows
template <typename T, int VEC, bool ZERO_ONLY>
__global__ __launch_bounds__(256) void moe_gather_kernel(const MoeRowsParams p) {
    constexpr int PP = kGatherPieces;
    const int lane = threadIdx.x & 63;
    const int piece0 = blockIdx.y * (64 * PP) + lane;
    for (long long s = (long long)blockIdx.x * 4 + wave_id(); s < p.S; s += (long long)gridDim.x * 4) {
        const int32_t pv = p.perm[s];
        const bool ok = moe_valid(pv, p.S);
        if (ZERO_ONLY && ok) continue;
        const T* __restrict__ src = (const T*)p.in + (size_t)((uint32_t)pv / (uint32_t)p.K) * p.ld_tok;   // used only if ok
        T* __restrict__ dst = (T*)p.out + (size_t)s * p.ld_slot;
        Piece<T, VEC> v[PP];
#pragma unroll
        for (int pp = 0; pp < PP; ++pp) {
            const int c = piece0 + pp * 64;
            v[pp].zero();
            if (!ZERO_ONLY && ok && c < p.pieces) v[pp].load(src + (size_t)c * VEC);
        }
#pragma unroll
        for (int pp = 0; pp < PP; ++pp) {
            const int c = piece0 + pp * 64;
            if (c < p.pieces) v[pp].store(dst + (size_t)c * VEC);
        }
    }
}

// ---- reduce -------------------------------------------------------------------------------------------------------------------------
// grid (token blocks, column chunks), 256 lanes = 4 tokens
template <typename T, int VEC>
__global__ __launch_bounds__(256) void moe_reduce_kernel(const MoeRowsParams p) {
    constexpr int PP = kReducePieces, JB = kReduceBatch;
    const int lane = threadIdx.x & 63;
    const int piece0 = blockIdx.y * (64 * PP) + lane;
    for (long long t = (long long)blockIdx.x * 4 + wave_id(); t < p.T; t += (long long)gridDim.x * 4) {
        int my_slot = -1;
        float my_w = 1.f;
        if (lane < p.K) {
            my_slot = p.slot[(size_t)t * p.K + lane];
            if (p.w) my_w = p.w[(size_t)t * p.K + lane];
        }
        float acc[PP][VEC];
#pragma unroll
        for (int pp = 0; pp < PP; ++pp)
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[pp][i] = 0.f;
        for (int j0 = 0; j0 < p.K; j0 += JB) {
            Piece<T, VEC> v[JB][PP];
            bool ok[JB];
            float wj[JB];
#pragma unroll
            for (int jj = 0; jj < JB; ++jj) {
                const int j = j0 + jj < p.K ? j0 + jj : p.K - 1;      // a lane that exists; the batch's tail is masked by `ok`
                const int32_t sl = __builtin_amdgcn_readlane(my_slot, j);
                wj[jj] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_w), j));
                ok[jj] = j0 + jj < p.K && moe_valid(sl, p.S);
                const T* __restrict__ src = (const T*)p.in + (size_t)(uint32_t)sl * p.ld_slot;             // used only if ok
#pragma unroll
                for (int pp = 0; pp < PP; ++pp) {
                    const int c = piece0 + pp * 64;
                    v[jj][pp].zero();
                    if (ok[jj] && c < p.pieces) v[jj][pp].load(src + (size_t)c * VEC);
                }
            }
#pragma unroll
            for (int jj = 0; jj < JB; ++jj)
                if (ok[jj]) {
#pragma unroll
                    for (int pp = 0; pp < PP; ++pp)
#pragma unroll
                        for (int i = 0; i < VEC; ++i) acc[pp][i] = fmaf(wj[jj], v[jj][pp].get(i), acc[pp][i]);
                }
        }
        T* __restrict__ dst = (T*)p.out + (size_t)t * p.ld_tok;
#pragma unroll
        for (int pp = 0; pp < PP; ++pp) {
            const int c = piece0 + pp * 64;
            Piece<T, VEC> o;
#pragma unroll
            for (int i = 0; i < VEC; ++i) o.set(i, round_store<T>(acc[pp][i]));
            if (c < p.pieces) o.store(dst + (size_t)c * VEC);
        }
    }
}

// ---- combine_bwd --------------------------------------------------------------------------------------------------------------------
// G = 64: grid (token blocks), 256 lanes = 4 tokens, no barrier.  G = 256: a workgroup per token; every lane of it takes the same
// trips through both loops (t, k and pieces are the workgroup's), so the barrier of the LDS hop is met by all.
template <typename T, int VEC, int G, bool FITS>
__global__ __launch_bounds__(256) void moe_combine_bwd_kernel(const MoeRowsParams p) {
    constexpr int PP = kCombinePieces, TPB = 256 / G;
    __shared__ Sum2 slots[2][4];
    const int lane = threadIdx.x % G;
    const int sub = G == 64 ? wave_id() : 0;
    int hop = 0;                                                     // the two slot sets alternate from hop to hop, across tokens too
    for (long long t = (long long)blockIdx.x * TPB + sub; t < p.T; t += (long long)gridDim.x * TPB) {
        const T* __restrict__ dyr = (const T*)p.dy + (size_t)t * p.ld_tok;
        Piece<T, VEC> g[PP];
        if constexpr (FITS) {
#pragma unroll
            for (int pp = 0; pp < PP; ++pp) {
                const int c = lane + pp * G;
                g[pp].zero();
                if (c < p.pieces) g[pp].load(dyr + (size_t)c * VEC);
            }
        }
        for (int j0 = 0; j0 < p.K; j0 += 2, ++hop) {
            const bool has1 = j0 + 1 < p.K;
            const int32_t sl0 = p.slot[(size_t)t * p.K + j0], sl1 = has1 ? p.slot[(size_t)t * p.K + j0 + 1] : -1;
            const bool ok0 = moe_valid(sl0, p.S), ok1 = moe_valid(sl1, p.S);
            const float w0 = p.w[(size_t)t * p.K + j0], w1 = has1 ? p.w[(size_t)t * p.K + j0 + 1] : 0.f;
            const T* __restrict__ ys0 = (const T*)p.in + (size_t)(uint32_t)sl0 * p.ld_slot;                 // used only if ok0
            const T* __restrict__ ys1 = (const T*)p.in + (size_t)(uint32_t)sl1 * p.ld_slot;
            T* __restrict__ d0 = (T*)p.out + (size_t)(uint32_t)sl0 * p.ld_slot;
            T* __restrict__ d1 = (T*)p.out + (size_t)(uint32_t)sl1 * p.ld_slot;
            Sum2 part{0.f, 0.f};
            for (int base = 0; base < (FITS ? 1 : p.pieces); base += G * PP) {
                Piece<T, VEC> a[PP], b[PP];
#pragma unroll
                for (int pp = 0; pp < PP; ++pp) {
                    const int c = base + lane + pp * G;
                    const bool in = c < p.pieces;
                    if constexpr (!FITS) {
                        g[pp].zero();
                        if (in) g[pp].load(dyr + (size_t)c * VEC);
                    }
                    a[pp].zero();
                    b[pp].zero();
                    if (in && ok0) a[pp].load(ys0 + (size_t)c * VEC);
                    if (in && ok1) b[pp].load(ys1 + (size_t)c * VEC);
                }
#pragma unroll
                for (int pp = 0; pp < PP; ++pp) {
                    const int c = base + lane + pp * G;
                    const bool in = c < p.pieces;
                    Piece<T, VEC> o0, o1;
#pragma unroll
                    for (int i = 0; i < VEC; ++i) {
                        const float gi = g[pp].get(i);
                        part.a = fmaf(gi, a[pp].get(i), part.a);
                        part.b = fmaf(gi, b[pp].get(i), part.b);
                        o0.set(i, round_store<T>(w0 * gi));
                        o1.set(i, round_store<T>(w1 * gi));
                    }
                    if (in && ok0) o0.store(d0 + (size_t)c * VEC);
                    if (in && ok1) o1.store(d1 + (size_t)c * VEC);
                }
            }
            part = group_allreduce<G>(part, 0, slots[hop & 1]);
            if (lane == 0) {
                p.dw[(size_t)t * p.K + j0] = ok0 ? part.a : 0.f;
                if (has1) p.dw[(size_t)t * p.K + j0 + 1] = ok1 ? part.b : 0.f;
            }
        }
    }
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------------
static inline unsigned row_blocks(long long rows, int per_block) {
    const long long n = (rows + per_block - 1) / per_block;
    return (unsigned)(n < kMaxRowBlocks ? n : kMaxRowBlocks);
}
static inline unsigned col_chunks(int pieces, int per_wave) { return (unsigned)((pieces + per_wave - 1) / per_wave); }

static MoeRowsParams rows_params(const nnop_moe_rows_desc& d) {
    MoeRowsParams p{};
    p.T = d.tokens; p.K = d.topk; p.S = d.tokens * d.topk; p.ld_tok = d.ld_tok; p.ld_slot = d.ld_slot;
    return p;
}

// f(T tag, VEC constant) with p.pieces set: the 16-byte path where D, both strides and `bases` allow it, else element-wise
template <typename F> static int dispatch_rows(const nnop_moe_rows_desc& d, MoeRowsParams& p, std::initializer_list<const void*> bases, F&& f) {
    return dispatch_dtype(d.dtype, [&](auto t) {
        typedef typename decltype(t)::type T;
        constexpr int VEC = 16 / (int)sizeof(T);
        if (d.dim % VEC == 0 && d.ld_tok % VEC == 0 && d.ld_slot % VEC == 0 && aligned16(bases)) {
            p.pieces = d.dim / VEC;
            f(t, std::integral_constant<int, VEC>{});
        } else {
            p.pieces = d.dim;
            f(t, std::integral_constant<int, 1>{});
        }
        return hipGetLastError() == hipSuccess ? NNOP_OK : NNOP_ERR_HIP;
    });
}

template <typename T, int VEC, bool ZERO_ONLY> static void launch_gather(const MoeRowsParams& p, hipStream_t s) {
    const dim3 grid(row_blocks(p.S, 4), col_chunks(p.pieces, 64 * kGatherPieces)), block(256);
    hipLaunchKernelGGL((moe_gather_kernel<T, VEC, ZERO_ONLY>), grid, block, 0, s, p);
}

int launch_moe_gather(const nnop_moe_rows_desc& d, void* xs, const void* x, const int32_t* perm, hipStream_t s) {
    MoeRowsParams p = rows_params(d);
    p.out = xs; p.in = x; p.perm = perm;
    return dispatch_rows(d, p, {xs, x}, [&](auto t, auto vec) { launch_gather<typename decltype(t)::type, decltype(vec)::value, false>(p, s); });
}

int launch_moe_reduce(const nnop_moe_rows_desc& d, void* out, const void* rows, const float* w, const int32_t* slot, hipStream_t s) {
    MoeRowsParams p = rows_params(d);
    p.out = out; p.in = rows; p.w = w; p.slot = slot;
    return dispatch_rows(d, p, {out, rows}, [&](auto t, auto vec) {
        const dim3 grid(row_blocks(p.T, 4), col_chunks(p.pieces, 64 * kReducePieces)), block(256);
        hipLaunchKernelGGL((moe_reduce_kernel<typename decltype(t)::type, decltype(vec)::value>), grid, block, 0, s, p);
    });
}

int launch_moe_combine_bwd(const nnop_moe_rows_desc& d, void* dys, float* dw, const void* dy, const void* ys, const float* w,
                           const int32_t* perm, const int32_t* slot, hipStream_t s) {
    MoeRowsParams p = rows_params(d);
    p.out = dys; p.in = ys; p.dy = dy; p.dw = dw; p.w = w; p.perm = perm; p.slot = slot;
    return dispatch_rows(d, p, {dys, dy, ys}, [&](auto t, auto vec) {
        typedef typename decltype(t)::type T;
        constexpr int VEC = decltype(vec)::value;
        const dim3 block(256);
        if (p.pieces <= 64 * kCombinePieces)
            hipLaunchKernelGGL((moe_combine_bwd_kernel<T, VEC, 64, true>), dim3(row_blocks(p.T, 4)), block, 0, s, p);
        else if (p.pieces <= 256 * kCombinePieces)
            hipLaunchKernelGGL((moe_combine_bwd_kernel<T, VEC, 256, true>), dim3(row_blocks(p.T, 1)), block, 0, s, p);
        else
            hipLaunchKernelGGL((moe_combine_bwd_kernel<T, VEC, 256, false>), dim3(row_blocks(p.T, 1)), block, 0, s, p);
        launch_gather<T, VEC, true>(p, s);                           // the rows of dys that no valid slot names
    });
}

}  // namespace nnop
