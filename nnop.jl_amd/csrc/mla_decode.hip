// mla_decode.hip -- the kernels of libnnop_hip_mla_decode.so (include/nnop_hip_mla_decode.h): the decode step of multi-head latent attention
// in its weight-absorbed form, over a paged latent cache.  A key is one row of 576 values; it is the key of every query head (all 576
// columns) and the value of every query head (the first 512 columns).
//
// This is not decode_attn.hip with another width.  That kernel packs the <= 16 rows of one KV head into one MFMA operand and streams K
// and V past them from global memory: it is bound by cache bytes.  Here 16 ... 128 heads share one key row, so a tile is fetched from
// HBM once per workgroup and reused by up to 64 heads out of LDS, and K and V are the same bytes read two ways.
//
//   - Work split.  A workgroup is (sequence b, new token i, head block of up to 64 heads, chunk c of the token's key range); the grid
//     comes from host values alone.  It has one wave per 16 heads of its block -- four at QH >= 64, QH / 16 below that, so no wave is
//     launched without heads except in the ragged last block of QH = 80, 96 or 112, whose spare waves still move their share of every
//     tile.  Wave w owns heads 16 w ... 16 w + 15 as the 16 columns of the B operand of v_mfma_f32_16x16x32.
//   - Q.  The wave's 16 x 576 slice goes from global memory straight into the 18 B-operand fragments of the scores (72 VGPRs), through
//     q's own strides, and stays there for the whole chunk.
//   - The latent tile.  32 keys x 576 values = 36,864 bytes, fetched by all waves in 16-byte pieces (9 per lane with four waves) into
//     registers and from there into an LDS image.  There are two images: the loads of tile t + 1 are issued in front of tile t's products
//     and stored behind them, so one barrier per tile suffices -- the image written in iteration t was last read in iteration t - 1.
//     With one wave a lane moves 36 pieces and with two 18; they go in four and two passes, between the first product and the parts
//     of the second, so that at most 12 wait in registers.
//     A row of the image is 1152 + 16 bytes: PADDED, not swizzled.  1152 bytes are 288 dwords = 32 mod 64 banks, so the 16 rows of an
//     operand read would meet in two banks; at 292 dwords the rows start at 36 r mod 64 -- 16 distinct multiples of 4 -- and a 16-byte
//     read of 16 rows covers the 64 banks once.  The transposing reads take 8 bytes from 4 lanes per row of 4 rows: 32 distinct banks.
//   - One image, two reads.  S^T = C Q^T reads the image row-wise (ds_read_b128) as the A operand over all 576 columns: a lane then
//     holds, for its head, the scores of keys 4 fq ... 4 fq + 3 of both 16-key blocks -- which is the B operand layout of the second
//     product, so P goes back into the MFMA from registers.  O^T += C[:, :512]^T P^T reads the same image through ds_read_b64_tr_b16,
//     the way decode_attn.hip reads V: 32 blocks of 16 latent columns.  V is never stored separately.
//   - Softmax: online, fp32, in registers; the scale is applied to the fp32 scores; a key is selected by its index against the token's
//     limit n = seqlens[b] - QL + i + 1, whatever its score is.  Rows of a tile at or behind n are stored into the image as zeros and
//     never loaded, so NaN behind a sequence's end reaches neither product.  Rescaling O is skipped where no row of the wave moved its
//     maximum (x * 1 = x: the same bits).
//   - O^T of a wave is 512 x 16 fp32 = 128 accumulator registers per lane.  With Q resident that is one wave per SIMD, which four-wave
//     workgroups of 74,752 LDS bytes give anyway (two per compute unit).
//   - Paging as in paged_attn.hip: page_size >= 16 is a power of two, so a 16-key block lies in one page and a tile needs two table
//     entries, both wave-uniform.  They are fetched a tile ahead -- right behind the loads of the tile in front -- and wait in two
//     registers; a block index is clamped into the live blocks and a key into [0, n - 1] before the lookup, so only live entries are read;
//     an id is clamped into [0, P - 1] and multiplied in 64 bits.
//   - Merge: a wave per (b, h, i) row joins the chunks in ascending order and rounds once, as decode_attn.hip's merge does.
#include "mla_decode.hpp"
#include "host_common.hpp"

namespace nnop {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

template <typename T> struct Ml;
template <> struct Ml<__bf16> {
    typedef bf16x8 frag;
    static __device__ __forceinline__ f32x4 mma(frag a, frag b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};
template <> struct Ml<_Float16> {
    typedef f16x8 frag;
    static __device__ __forceinline__ f32x4 mma(frag a, frag b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};

struct MlaParams {
    void* o;
    float* lse;
    const void* q;
    const void* kv;
    const int32_t* table;
    const int32_t* seqlens;
    float* ws;
    long long qs_b, qs_h, qs_l, cs_p, cs_l, ts;  // elements; ts: int32 entries between two rows of the table
    int QL, QH, HB, cap, splits, batch;
    int lg_page, num_pages;
    float scale;
};

constexpr float kNegInf = -__builtin_huge_valf();
constexpr int kRowBytes = 2 * kMlaW + 16;       // a row of the image: 1152 bytes and the pad
constexpr int kImgBytes = kMlaTile * kRowBytes;  // 37,376

// the (m, l) pairs lie behind the O rows of every (row, chunk)
__device__ __forceinline__ float* ws_ml(const MlaParams& p) {
    return p.ws + (size_t)p.batch * p.QH * p.QL * p.splits * (size_t)kMlaV;
}

template <typename T, int NW>
__global__ __launch_bounds__(64 * NW) void mla_decode_kernel(const MlaParams p) {
    typedef typename Ml<T>::frag frag;
    constexpr int NT = 64 * NW;
    constexpr int ES = kMlaW / 32;               // 18 reduction steps of the scores
    constexpr int ET = kMlaV / 16;               // 32 blocks of 16 latent columns of O^T
    constexpr int RC = kMlaW / 8;                // 72 16-byte pieces of a row
    constexpr int PIECES = kMlaTile * RC / NT;   // of a lane per tile: 9, 12, 18 or 36
    constexpr int PASSES = NW == 1 ? 4 : NW == 2 ? 2 : 1;  // at most 12 pieces wait in a lane's registers
    constexpr int PER = PIECES / PASSES;
    static_assert(PIECES * NT == kMlaTile * RC && PER * PASSES == PIECES, "the lanes share a tile evenly");
    __shared__ __attribute__((aligned(16))) char smem[2 * kImgBytes];

    int r = blockIdx.x;
    const int c = r % p.splits;
    r /= p.splits;
    const int hb = r % p.HB;
    r /= p.HB;
    const int i = r % p.QL, b = r / p.QL;
    const int tid = threadIdx.x, lane = tid & 63, fm = lane & 15, fq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h0 = kMlaBlockHeads * hb + 16 * wave;
    const bool has = h0 < p.QH;  // QH is a multiple of 16: a wave has 16 heads or none
    const long long row = ((long long)b * p.QH + min(h0 + fm, p.QH - 1)) * p.QL + i;  // this lane's row of o and lse

    const int hi = min(max(p.seqlens[b], 0), p.cap);
    const int n = max(hi - p.QL + i + 1, 0);  // the token sees keys 0 ... n - 1
    const int tiles = (n + kMlaTile - 1) / kMlaTile;
    const int per = (tiles + p.splits - 1) / p.splits;
    const int t0 = c * per, t1 = min(tiles, t0 + per);

    if (t0 >= t1) {  // no tile: nothing of the table or the pool is read
        if (!has) return;
        if (p.splits > 1) {
            if (fq == 0) {
                float* ml = ws_ml(p) + (row * p.splits + c) * 2;
                ml[0] = kNegInf;
                ml[1] = 0.f;
            }
        } else {  // the token sees no key at all: o = +0, lse = -inf
            for (int hh = 0; hh < 16; ++hh) {
                T* orow = (T*)p.o + (((long long)b * p.QH + h0 + hh) * p.QL + i) * kMlaV;
                *reinterpret_cast<uint4*>(orow + 8 * lane) = uint4{0u, 0u, 0u, 0u};
            }
            if (fq == 0 && p.lse) p.lse[row] = kNegInf;
        }
        return;
    }

    frag qf[ES];
    {
        const T* qrow = (const T*)p.q + b * p.qs_b + min(h0 + fm, p.QH - 1) * p.qs_h + i * p.qs_l + 8 * fq;
#pragma unroll
        for (int s = 0; s < ES; ++s) qf[s] = __builtin_bit_cast(frag, *reinterpret_cast<const uint4*>(qrow + 32 * s));
    }

    // ---- the address path ----
    const int32_t* tab = p.table + b * p.ts;
    const int blk_hi = (n - 1) >> 4;  // the last 16-key block that holds a visible key: n >= 1 here
    const int row_mask = (1 << p.lg_page) - 1, blk_shift = p.lg_page - 4;
    struct Ids {
        int raw[2];  // the table entries of the two 16-key blocks of a tile, as they were read
    };
    auto fetch = [&](Ids& s, int t) {
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) s.raw[kb] = tab[min(2 * t + kb, blk_hi) >> blk_shift];
    };
    const T* cbase = (const T*)p.kv;
    uint4 stage[PER];
    // Pass `ps` of tile t into the staging registers.  A pass is PROWS whole rows, so piece k of a lane is the same 16 bytes of a row
    // in every pass, PROWS rows further down: x = tid + NT k is piece x % 72 of row x / 72 + ps PROWS.  A row at or behind n is not loaded.
    constexpr int PROWS = kMlaTile / PASSES;
    static_assert(PER * NT == PROWS * RC, "a pass is whole rows");
    auto load = [&](const Ids& id, int t, int ps) {
        long long page[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
            page[kb] = min(max(__builtin_amdgcn_readfirstlane(id.raw[kb]), 0), p.num_pages - 1) * p.cs_p;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int x = tid + NT * k, rr = x / RC + ps * PROWS, cc = x % RC;
            const int key = kMlaTile * t + rr;
            const T* src = cbase + page[rr >> 4] + (min(key, n - 1) & row_mask) * p.cs_l + 8 * cc;
            stage[k] = *reinterpret_cast<const uint4*>(src);
            if (key >= n) stage[k] = uint4{0u, 0u, 0u, 0u};
        }
    };
    auto store = [&](char* img, int ps) {
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int x = tid + NT * k, rr = x / RC, cc = x % RC;
            *reinterpret_cast<uint4*>(img + ps * PROWS * kRowBytes + rr * kRowBytes + 16 * cc) = stage[k];
        }
    };

    float m_run = kNegInf, l_run = 0.f;
    f32x4 oacc[ET];
#pragma unroll
    for (int et = 0; et < ET; ++et) oacc[et] = f32x4{0.f, 0.f, 0.f, 0.f};
    frag pf;
    typedef __attribute__((address_space(3))) s16x4* lds_tr_p;

    // S^T of the tile from the image's rows, the online softmax, P into pf
    auto scores = [&](const char* img, int t) {
        f32x4 sacc[2][2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) sacc[kb][0] = sacc[kb][1] = f32x4{0.f, 0.f, 0.f, 0.f};
        const char* krow = img + fm * kRowBytes + 16 * fq;
#pragma unroll
        for (int s = 0; s < ES; ++s)
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                const uint4 a = *reinterpret_cast<const uint4*>(krow + 16 * kb * kRowBytes + 64 * s);
                sacc[kb][s & 1] = Ml<T>::mma(__builtin_bit_cast(frag, a), qf[s], sacc[kb][s & 1]);
            }
        float x[8], mx = kNegInf;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int key = kMlaTile * t + 16 * (j >> 2) + 4 * fq + (j & 3);
            x[j] = key < n ? (sacc[j >> 2][0][j & 3] + sacc[j >> 2][1][j & 3]) * p.scale : kNegInf;
            mx = fmaxf(mx, x[j]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float m_new = fmaxf(m_run, mx);
        const float m_ref = m_new == kNegInf ? 0.f : m_new;
        const float alpha = __expf(m_run - m_ref);
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float e = __expf(x[j] - m_ref);
            sum += e;
            pf[j] = (T)e;
        }
        sum += __shfl_xor(sum, 16);
        sum += __shfl_xor(sum, 32);
        l_run = l_run * alpha + sum;
        m_run = m_new;
        if (__builtin_amdgcn_ballot_w64(alpha != 1.f) != 0) {
#pragma unroll
            for (int et = 0; et < ET; ++et) oacc[et] *= alpha;
        }
    };
    // O^T += C[:, :512]^T P^T from the same image, transposed on the way out of LDS
    auto values = [&](const char* img, int et0, int et1) {
        const char* vld = img + (4 * fq + (fm >> 2)) * kRowBytes + 8 * (fm & 3);
#pragma unroll
        for (int et = et0; et < et1; ++et) {
            const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr_p)(vld + 32 * et));
            const s16x4 d = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr_p)(vld + 32 * et + 16 * kRowBytes));
            const s16x8 vf = {a[0], a[1], a[2], a[3], d[0], d[1], d[2], d[3]};
            oacc[et] = Ml<T>::mma(__builtin_bit_cast(frag, vf), pf, oacc[et]);
        }
    };

    Ids ids;
    fetch(ids, t0);
#pragma unroll
    for (int ps = 0; ps < PASSES; ++ps) {
        load(ids, t0, ps);
        store(smem, ps);
    }
    fetch(ids, t0 + 1);
    __syncthreads();
    for (int t = t0; t < t1; ++t) {
        char* cur = smem + ((t - t0) & 1) * kImgBytes;
        char* nxt = smem + ((t - t0 + 1) & 1) * kImgBytes;
        const bool more = t + 1 < t1;  // uniform
        Ids next = ids;
        if (more) {
            load(ids, t + 1, 0);
            fetch(next, t + 2);  // behind the tile's loads; needed an iteration from here
        }
        if (has) scores(cur, t);
        // the second product in PASSES - 1 parts (one part where the tile moves in one pass), a pass of the next tile between two parts
        constexpr int PARTS = PASSES > 1 ? PASSES - 1 : 1;
#pragma unroll
        for (int ps = 1; ps <= PARTS; ++ps) {
            if (PASSES > 1 && more) {
                store(nxt, ps - 1);
                load(ids, t + 1, ps);
            }
            if (has) values(cur, ET * (ps - 1) / PARTS, ET * ps / PARTS);
        }
        if (more) store(nxt, PASSES - 1);
        ids = next;
        __syncthreads();
    }
    if (!has) return;

    if (p.splits > 1) {
        const long long part = row * p.splits + c;
        float* orow = p.ws + part * kMlaV + 4 * fq;
#pragma unroll
        for (int et = 0; et < ET; ++et)
#pragma unroll
            for (int j = 0; j < 4; ++j) orow[16 * et + j] = oacc[et][j];  // the workspace is promised to 4 bytes only
        if (fq == 0) {
            float* ml = ws_ml(p) + part * 2;
            ml[0] = m_run;
            ml[1] = l_run;
        }
        return;
    }
    const float inv = l_run > 0.f ? 1.f / l_run : 0.f;
    T* orow = (T*)p.o + row * kMlaV + 4 * fq;
#pragma unroll
    for (int et = 0; et < ET; ++et) {
        typedef T t4 __attribute__((ext_vector_type(4)));
        t4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (T)(oacc[et][j] * inv);
        *reinterpret_cast<t4*>(orow + 16 * et) = v;
    }
    if (fq == 0 && p.lse) p.lse[row] = l_run > 0.f ? m_run + __logf(l_run) : kNegInf;
}

// decode_attn.hip's merge restated on MlaParams: one wave per row of o, the chunks of the row in ascending order, a chunk that had no
// tile (m = -inf, l = 0, no O written) skipped by selection; a row no chunk of which had a tile gives o = +0, lse = -inf.
template <typename T>
__global__ __launch_bounds__(64) void mla_decode_merge_kernel(const MlaParams p) {
    const long long row = blockIdx.x;
    const int lane = threadIdx.x;
    const float* ml = ws_ml(p);
    float M = kNegInf;
    for (int c = 0; c < p.splits; ++c) M = fmaxf(M, ml[(row * p.splits + c) * 2]);
    const float m_ref = M == kNegInf ? 0.f : M;
    float L = 0.f, acc[kMlaV / 64];
#pragma unroll
    for (int k = 0; k < kMlaV / 64; ++k) acc[k] = 0.f;
    for (int c = 0; c < p.splits; ++c) {
        const long long part = row * p.splits + c;
        const float m = ml[part * 2], l = ml[part * 2 + 1];
        const bool live = m != kNegInf;
        const float a = __expf(m - m_ref);
        L += live ? l * a : 0.f;
#pragma unroll
        for (int k = 0; k < kMlaV / 64; ++k) {
            const float o = p.ws[part * kMlaV + lane + 64 * k];
            acc[k] += live ? o * a : 0.f;
        }
    }
    const float inv = L > 0.f ? 1.f / L : 0.f;
#pragma unroll
    for (int k = 0; k < kMlaV / 64; ++k) ((T*)p.o)[row * kMlaV + lane + 64 * k] = (T)(acc[k] * inv);
    if (lane == 0 && p.lse) p.lse[row] = L > 0.f ? M + __logf(L) : kNegInf;
}

template <typename T, int NW> int launch(const MlaParams& p, hipStream_t s) {
    const int groups = p.batch * p.QL * p.HB * p.splits;
    hipLaunchKernelGGL((mla_decode_kernel<T, NW>), dim3(groups), dim3(64 * NW), 0, s, p);
    if (p.splits > 1) hipLaunchKernelGGL((mla_decode_merge_kernel<T>), dim3(p.batch * p.QH * p.QL), dim3(64), 0, s, p);
    return hipGetLastError() == hipSuccess ? (int)NNOP_OK : (int)NNOP_ERR_HIP;
}

template <typename T> int launch_waves(const MlaParams& p, hipStream_t s) {
    switch (p.QH >= kMlaBlockHeads ? kMlaWaves : p.QH / 16) {  // only the waves that have heads
        case 1: return launch<T, 1>(p, s);
        case 2: return launch<T, 2>(p, s);
        case 3: return launch<T, 3>(p, s);
    }
    return launch<T, 4>(p, s);
}

}  // namespace

int launch_mla_decode(const nnop_mla_decode_desc& d, int splits, void* o, float* lse, const void* q, const void* kv,
                      const int32_t* block_table, const int32_t* seqlens, float* workspace, hipStream_t stream) {
    MlaParams p;
    p.o = o, p.lse = lse, p.q = q, p.kv = kv, p.table = block_table, p.seqlens = seqlens, p.ws = workspace;
    p.qs_b = d.q_stride_b, p.qs_h = d.q_stride_h, p.qs_l = d.q_stride_l, p.cs_p = d.kv_stride_p, p.cs_l = d.kv_stride_l, p.ts = d.table_stride;
    p.QL = d.ql, p.QH = d.qh, p.HB = mla_decode_head_blocks(d), p.cap = d.max_pages * d.page_size, p.splits = splits, p.batch = d.batch;
    p.lg_page = __builtin_ctz((unsigned)d.page_size), p.num_pages = d.num_pages;
    p.scale = d.softmax_scale;
    return d.dtype == NNOP_BF16 ? launch_waves<__bf16>(p, stream) : launch_waves<_Float16>(p, stream);
}

}  // namespace nnop
