// moe_gemm_tile.hpp -- the one MFMA tile of the three grouped-GEMM libraries: libnnop_hip_moe_gemm.so (moe_gemm.hip),
// libnnop_hip_moe_linear.so (moe_linear.hip) and libnnop_hip_moe_mx.so (moe_mx.hip) instantiate it; nothing is linked between them.
// gfx950 (MI355X) only.
//
// moe_gemm_tile<T, PROD, ALIGNED, EPI, OutT, StageB> computes
//     C[m][n] = epilogue( sum_r A(m, r) B(n, r) )
// on a 128 x 128 output tile with 4 waves (2 x 2, 64 x 64 each, 4 x 4 MFMA tiles of 16 x 16) and fp32 accumulators.  The three products
// differ in what m, n, r are and in how an operand lies in memory:
//     PROD  product   m         n         r               A                        B
//     0     "NT"      slot row  n < N     r < R           rows [m][r]  contiguous  w[e] [n][r]  contiguous
//     1     "NN"      slot row  n < N     r < R           rows [m][r]  contiguous  w[e] [r][n]  strided in r
//     2     "TN"      m < M     n < N     s in [lo, hi)   rows [r][m]  strided     rows [r][n]  strided
// (for [E][N][K] weights: the forward, bwd_x and bwd_w in that order; what a [E][K][N] layout maps to: moe_linear.hip).
// Both operands are staged through LDS as images [128 rows][128 bytes] with r contiguous (64 16-bit or 32 fp32 elements per reduction
// step), two buffers each (64 KiB in all, two workgroups per CU): the global loads of step k+1 are issued before the MFMAs of step k and
// written to the other buffer after them, one barrier per step.  A contiguous operand is written in 16-byte pieces; a strided one is
// transposed in the write pass (a thread holds 4 consecutive r of each of its columns and writes them as one 8- or 16-byte piece).
// The 16-byte chunk index of an image row is XOR-ed with sw(row), which makes the 16 rows of one fragment read hit 16 different bank
// groups.  Fragments are read with 16-byte LDS reads: a lane of k-group q reads chunks q and q + 4; the 16-bit types feed each chunk
// to one v_mfma_f32_16x16x32, fp32 feeds element i of it to the i-th of four v_mfma_f32_16x16x4_f32 (any k order is legal where A and B
// agree).  The MFMA's row operand is the B image, so a lane ends up with 4 consecutive n of one m and stores 8 or 16 bytes.
//
// The epilogue works on those groups of 4, in fp32, in front of the one rounding of the store:
//     EPI 0  nothing
//     EPI 1  + bias[e][n]    (PROD 0 / 1) the lane loads the 4 x 4 bias values of its columns once, behind the main loop; a tile of the
//                            rows outside the experts loads none and stays +0
//     EPI 2  + old           (PROD 2) the lane loads what C holds, masked like its store; the workgroups of an expert without rows
//                            return before any load, so that expert's C keeps its bits
// OutT is T, or float beside a 16-bit T (PROD 2: an fp32 weight gradient).
//
// StageB is how the B operand of PROD 0 / 1 gets from memory into the staging registers: by default Stage<T, TRB, ALIGNED>, which reads
// elements of T.  Another policy (moe_mx.hip: packed MXFP4 weights) has the interface of Stage -- Src, Extra, origin(), advance(),
// load(), write() -- and must hold in v[], when Stage's write() stores it, what the dense load of the expanded operand would have left;
// the LDS image, the fragment reads, the MFMA order, the epilogue and the bounds are then those of the dense product.
//
// Nothing outside [0, S) x [0, ld) and the E weight matrices is touched whatever `offsets` holds: offsets are clamped into [0, S] where
// they are read, and every loop bound is a descriptor field or such a clamped value.  Rows outside the tile's range (an expert's end,
// the end of the reduction range of PROD 2, columns beyond the extents) are not loaded; the staging registers are set to zero instead,
// so what those rows hold (NaN, Inf) never enters a product.
//
// Everything sits in an unnamed namespace: each library gets its own copy, and the kernels of moe_gemm.hip keep the names they had when
// this text lived there.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nnop {

constexpr int kMoeGemmTile = 128;   // BM = BN: the output tile of one workgroup

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int kTile = kMoeGemmTile;        // BM = BN
constexpr int kRowBytes = 128;             // one image row: BK elements
constexpr int kImage = kTile * kRowBytes;  // 16 KiB
constexpr int kThreads = 256;
constexpr int kPieces = kImage / (kThreads * 16);  // 16-byte pieces per thread and operand: 4

struct GemmParams {
    void* out;
    const void* a;
    const void* b;
    const int32_t* offsets;
    long long lda, ldb, ldc;  // row strides in elements
    long long wstride;        // elements between the weight matrices of two experts
    int S, E;
    int M, N, R;              // the extents of m, n, r where they are descriptor fields (PROD 2: R unused, PROD 0/1: M unused)
    int mt, nt;               // tiles along m (PROD 0/1: the row-tile slots of the grid) and n
};

// what EPI 1 adds: bias [E][ld] of the type of the operands
struct TileBias {
    const void* bias;
    long long ld;
};

__device__ __forceinline__ int clamped_offset(const int32_t* off, int i, int S) {
    const int v = off[i];
    return v < 0 ? 0 : (v > S ? S : v);
}
// Segment i of the slot rows, i = 0 ... E+1: the rows in front of the first expert, the E experts, the rows behind the last one.
__device__ __forceinline__ void segment(const int32_t* off, int i, int E, int S, int& lo, int& hi) {
    lo = i == 0 ? 0 : clamped_offset(off, i - 1, S);
    hi = i == E + 1 ? S : clamped_offset(off, i, S);
}
__device__ __forceinline__ long long segment_tiles(const int32_t* off, int i, int E, int S) {
    int lo, hi;
    segment(off, i, E, S, lo, hi);
    return hi > lo ? ((long long)(hi - lo) + kTile - 1) / kTile : 0;
}

// sw(row): the XOR on the 16-byte chunk index of an image row
__device__ __forceinline__ int sw(int row) { return ((row >> 1) ^ (row >> 4)) & 7; }

template <typename T> struct Mma;
template <> struct Mma<__bf16> {
    static __device__ __forceinline__ f32x4 run(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};
template <> struct Mma<_Float16> {
    static __device__ __forceinline__ f32x4 run(f16x8 a, f16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};
template <> struct Mma<float> {
    static __device__ __forceinline__ f32x4 run(f32x4 a, f32x4 b, f32x4 c) {
#pragma unroll
        for (int i = 0; i < 4; ++i) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[i], c, 0, 0, 0);
        return c;
    }
};

// One operand's share of a reduction step in a thread's registers: kPieces pieces of EPC elements.
//   TR = false  image row x = t / 8 + 32 p, chunk t % 8: EPC consecutive r of one row           (memory: [x][r])
//   TR = true   reduction row 4 (t / XC) + p, EPC consecutive x from EPC (t % XC), XC = 128 / EPC  (memory: [r][x])
// `base` points at (x = 0, r = 0) of the step; xleft and rleft are how many x and r of the step exist.  What does not exist is zero.
template <typename T, bool TR, bool ALIGNED> struct Stage {
    static constexpr int EPC = 16 / (int)sizeof(T);
    static constexpr int XC = kTile / EPC;
    typedef T tvec __attribute__((ext_vector_type(EPC)));
    typedef T t4 __attribute__((ext_vector_type(4)));
    typedef const T* Src;  // where an operand's step begins: (x = 0, r = 0)
    struct Extra {};       // what a policy needs beyond GemmParams: nothing here
    tvec v[kPieces];

    // the B operand of PROD 0 / 1: column tile n0 of expert e, and one reduction step further along r
    static __device__ __forceinline__ Src origin(const GemmParams& p, const Extra&, long long e, int n0) {
        return static_cast<const T*>(p.b) + (e * p.wstride + (TR ? (long long)n0 : n0 * p.ldb));
    }
    static __device__ __forceinline__ Src advance(Src b, const GemmParams& p, const Extra&) {
        return b + (TR ? (kRowBytes / (int)sizeof(T)) * p.ldb : (long long)(kRowBytes / (int)sizeof(T)));
    }

    __device__ __forceinline__ void load(const T* base, long long ld, int xleft, int rleft, int t) {
#pragma unroll
        for (int p = 0; p < kPieces; ++p) {
            const int x = TR ? EPC * (t % XC) : t / 8 + 32 * p;
            const int r = TR ? 4 * (t / XC) + p : EPC * (t % 8);
            const T* src = TR ? base + r * ld + x : base + x * ld + r;
            const int cleft = TR ? xleft - x : rleft - r;  // elements left along the piece
            const bool row_ok = TR ? r < rleft : x < xleft;
            tvec z;
#pragma unroll
            for (int i = 0; i < EPC; ++i) z[i] = (T)0.f;
            if (ALIGNED) {
                if (row_ok && cleft > 0) z = *reinterpret_cast<const tvec*>(src);
            } else {
#pragma unroll
                for (int i = 0; i < EPC; ++i)
                    if (row_ok && i < cleft) z[i] = src[i];
            }
            v[p] = z;
        }
    }

    __device__ __forceinline__ void write(unsigned char* image, int t) const {
        if (!TR) {
#pragma unroll
            for (int p = 0; p < kPieces; ++p) {
                const int x = t / 8 + 32 * p, c = t % 8;
                *reinterpret_cast<tvec*>(image + x * kRowBytes + ((c ^ sw(x)) << 4)) = v[p];
            }
        } else {
            const int byte = 4 * (t / XC) * (int)sizeof(T);  // of r = 4 (t / XC) within the image row
#pragma unroll
            for (int i = 0; i < EPC; ++i) {
                const int x = EPC * (t % XC) + i;
                t4 o;
#pragma unroll
                for (int p = 0; p < 4; ++p) o[p] = v[p][i];
                *reinterpret_cast<t4*>(image + x * kRowBytes + (((byte >> 4) ^ sw(x)) << 4) + (byte & 15)) = o;
            }
        }
    }
};
static_assert(kPieces == 4, "the transposing write packs kPieces = 4 consecutive r");

// The body of a workgroup, 64 KiB of LDS included.  tb is read for EPI 1 only.
template <typename T, int PROD, bool ALIGNED, int EPI, typename OutT, typename StageB = Stage<T, PROD != 0, ALIGNED>>
__device__ __forceinline__ void moe_gemm_tile(const GemmParams p, const TileBias tb, const typename StageB::Extra xb = {}) {
    static_assert(EPI == 0 || (EPI == 1 && PROD != 2) || (EPI == 2 && PROD == 2), "bias beside the row products, + old beside bwd_w");
    constexpr int EPC = 16 / (int)sizeof(T);
    constexpr int BK = kRowBytes / (int)sizeof(T);
    constexpr bool TRA = PROD == 2, TRB = PROD != 0;
    typedef T tvec __attribute__((ext_vector_type(EPC)));
    typedef T t4 __attribute__((ext_vector_type(4)));
    typedef OutT o4 __attribute__((ext_vector_type(4)));
    __shared__ __attribute__((aligned(16))) unsigned char smem[4 * kImage];  // A0 B0 A1 B1

    const int t = threadIdx.x;
    // Workgroup id -> position in the tile order: ids that share an XCD (id % 8) get consecutive positions, so the row tiles of one expert
    // that read the same weight tile (PROD 0/1), or the tiles of one expert that read the same rows (PROD 2), share that XCD's L2.
    const unsigned nwg = gridDim.x, id = blockIdx.x;
    const unsigned q8 = nwg >> 3, r8 = nwg & 7, xcd = id & 7;
    const unsigned pos = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (id >> 3);

    const T* a = static_cast<const T*>(p.a);
    typename StageB::Src b;
    OutT* out = static_cast<OutT*>(p.out);
    const T* bias = nullptr;   // EPI 1: the bias of this tile's columns; stays null for a tile of +0
    int mleft, nleft, rtotal;  // rows and columns of the tile that exist (<= 128), length of the reduction
    if constexpr (PROD != 2) {
        const long long ti = pos % (unsigned)p.mt;
        const int ct = pos / (unsigned)p.mt;
        // wave 0 finds the (segment, tile) of row-tile slot ti: each lane sums the tiles of `per` consecutive segments, a scan over the
        // lanes places ti in one lane's share, that lane walks its share again.
        int* info = reinterpret_cast<int*>(smem);
        if (t < 64) {
            const int nseg = p.E + 2, per = (nseg + 63) >> 6, beg = t * per;
            long long mine = 0;
            for (int j = 0; j < per; ++j)
                if (beg + j < nseg) mine += segment_tiles(p.offsets, beg + j, p.E, p.S);
            long long incl = mine;
            for (int d = 1; d < 64; d <<= 1) {
                const long long o = __shfl_up(incl, d);
                if (t >= d) incl += o;
            }
            bool found = false;
            long long run = incl - mine;
            if (ti >= run && ti < incl) {
                for (int j = 0; j < per; ++j) {
                    if (beg + j < nseg && !found) {
                        const long long n = segment_tiles(p.offsets, beg + j, p.E, p.S);
                        if (ti < run + n) {
                            found = true;
                            info[0] = beg + j;
                            info[1] = (int)(ti - run);
                        }
                        run += n;
                    }
                }
            }
            if (__ballot(found) == 0 && t == 0) info[0] = -1;
        }
        __syncthreads();
        const int seg = info[0], tile = info[1];
        __syncthreads();
        if (seg < 0) return;  // a surplus workgroup
        int lo, hi;
        segment(p.offsets, seg, p.E, p.S, lo, hi);
        const int m0 = lo + tile * kTile;  // < hi <= S
        const int n0 = ct * kTile;
        mleft = min(hi - m0, kTile);
        nleft = min(p.N - n0, kTile);
        const bool expert = seg >= 1 && seg <= p.E;
        rtotal = expert ? p.R : 0;  // the rows in front of and behind the experts: a tile of +0
        const long long e = expert ? seg - 1 : 0;
        a += m0 * p.lda;
        b = StageB::origin(p, xb, e, n0);
        out += m0 * p.ldc + n0;
        if (EPI == 1 && expert) bias = static_cast<const T*>(tb.bias) + e * tb.ld + n0;
    } else {
        const unsigned per_e = (unsigned)p.mt * (unsigned)p.nt;
        const int e = pos / per_e, rem = pos % per_e;
        const int m0 = (rem / p.nt) * kTile, n0 = (rem % p.nt) * kTile;
        const int lo = clamped_offset(p.offsets, e, p.S), hi = clamped_offset(p.offsets, e + 1, p.S);
        mleft = min(p.M - m0, kTile);
        nleft = min(p.N - n0, kTile);
        rtotal = hi > lo ? hi - lo : 0;
        if (EPI == 2 && rtotal == 0) return;  // nothing to add: what C holds stays, bit for bit
        a += lo * p.lda + m0;
        b = static_cast<const T*>(p.b) + (lo * p.ldb + n0);
        out += e * p.wstride + m0 * p.ldc + n0;
    }

    const int lane = t & 63, wave = t >> 6, wm = wave >> 1, wn = wave & 1, fr = lane & 15, fq = lane >> 4;
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // one reduction step further along r: contiguous operands move BK columns, strided ones BK rows
    const long long step_a = TRA ? BK * p.lda : (long long)BK;
    const int steps = (int)(((long long)rtotal + BK - 1) / BK);
    Stage<T, TRA, ALIGNED> sa;
    StageB sb;
    if (steps > 0) {
        sa.load(a, p.lda, mleft, rtotal, t);
        sb.load(b, p.ldb, nleft, rtotal, t);
        sa.write(smem, t);
        sb.write(smem + kImage, t);
    }
    __syncthreads();
    for (int k = 0; k < steps; ++k) {
        unsigned char* cur = smem + (k & 1) * 2 * kImage;
        unsigned char* nxt = smem + ((k + 1) & 1) * 2 * kImage;
        const bool more = k + 1 < steps;
        if (more) {
            a += step_a;
            b = StageB::advance(b, p, xb);
            sa.load(a, p.lda, mleft, rtotal - (k + 1) * BK, t);
            sb.load(b, p.ldb, nleft, rtotal - (k + 1) * BK, t);
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            tvec fa[4], fb[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int ra = wm * 64 + i * 16 + fr, rb = wn * 64 + i * 16 + fr;
                fa[i] = *reinterpret_cast<const tvec*>(cur + ra * kRowBytes + (((fq + 4 * h) ^ sw(ra)) << 4));
                fb[i] = *reinterpret_cast<const tvec*>(cur + kImage + rb * kRowBytes + (((fq + 4 * h) ^ sw(rb)) << 4));
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = Mma<T>::run(fb[j], fa[i], acc[i][j]);  // rows of the result: n, columns: m
        }
        if (more) {
            sa.write(nxt, t);
            sb.write(nxt + kImage, t);
        }
        __syncthreads();
    }

    // acc[i][j][g] is C[m = wm 64 + 16 i + fr][n = wn 64 + 16 j + 4 fq + g]
    if (EPI == 1) {
        if (bias != nullptr) {  // the 4 x 4 bias values of the lane's columns, once; the same for each of its 4 rows
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int n = wn * 64 + j * 16 + 4 * fq;
                f32x4 bv = f32x4{0.f, 0.f, 0.f, 0.f};
                if (ALIGNED) {
                    if (n < nleft) {
                        const t4 v = *reinterpret_cast<const t4*>(bias + n);
#pragma unroll
                        for (int g = 0; g < 4; ++g) bv[g] = (float)v[g];
                    }
                } else {
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        if (n + g < nleft) bv[g] = (float)bias[n + g];
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i][j] += bv;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = wm * 64 + i * 16 + fr;
        if (m >= mleft) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = wn * 64 + j * 16 + 4 * fq;
            OutT* dst = out + m * p.ldc + n;
            if (ALIGNED) {
                if (n < nleft) {
                    o4 o;
                    if (EPI == 2) {
                        const o4 old = *reinterpret_cast<const o4*>(dst);
#pragma unroll
                        for (int g = 0; g < 4; ++g) o[g] = (OutT)((float)old[g] + acc[i][j][g]);
                    } else {
#pragma unroll
                        for (int g = 0; g < 4; ++g) o[g] = (OutT)acc[i][j][g];
                    }
                    *reinterpret_cast<o4*>(dst) = o;
                }
            } else {
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    if (n + g < nleft) dst[g] = EPI == 2 ? (OutT)((float)dst[g] + acc[i][j][g]) : (OutT)acc[i][j][g];
            }
        }
    }
}

static inline long long tiles_of(long long n) { return (n + kTile - 1) / kTile; }
// the row-tile slots of PROD 0 / 1: at most S / BM full row tiles, and one partial tile for each non-empty one of the E + 2 row ranges
static inline long long row_tile_slots(long long S, long long E) { return S / kTile + (E + 2 < S ? E + 2 : S); }

}  // namespace
}  // namespace nnop
