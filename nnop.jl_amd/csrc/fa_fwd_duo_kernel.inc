// fa_fwd_duo_kernel.inc -- the body of fa_fwd_duo_kernel (fa_fwd_duo.hpp).
// SINK = learned attention sinks merged in the epilogue: an instantiation of its own, so that the kernel of the calls without sinks is
// this text with the sink code compiled away.
template <typename T, int E, int MODE, int NZ = 2, bool SINK = false>
__global__ __launch_bounds__(512) void fa_fwd_duo_kernel(const FwdParams p) {
    static_assert(sizeof(T) == 2 && ((E == 64 && (NZ == 1 || NZ == 2)) || (E == 128 && NZ == 1) || (E == 32 && NZ == 2)),
                  "16-bit element types; E = 64, E = 128 with 32-row waves, E = 32 with 64-row waves");
    constexpr int RW = 32 * NZ, RB = 4 * RW;                  // query rows per wave / per workgroup
    using frag_t = typename Elem<T>::frag;
    using KImg   = RowImg<T, E>;
    using VImg   = ColImg<T, E>;
    constexpr bool kGeneral = MODE != 0;
    constexpr int BK = 64, KB = 2, KS = E / 16, EB = E / 32, NS = 2 * duo_slots_per_group<E>();
    constexpr int KBYTES = KImg::bytes(BK), VBYTES = VImg::bytes(BK);
    constexpr int RING = NS * (KBYTES + VBYTES);
    constexpr int MASK_OFF = RING > kDuoXchgBytes ? RING : kDuoXchgBytes;
    constexpr int TILE_BYTES = BK * E * (int)sizeof(T);
    constexpr int NJK = KBYTES / 4096, NJV = VBYTES / 4096;   // DMA pieces per wave and tile (the 4 waves of a group copy a tile)
    static_assert(NJK * 4096 == KBYTES && NJV * 4096 == VBYTES && NJK <= 4 && NJV <= 4, "four waves x NJ pieces = one image");

    extern __shared__ __attribute__((aligned(16))) char smem[];
#if NNOP_DUO_STAMP
    uint64_t stamp[8];
    stamp[0] = __builtin_amdgcn_s_memtime();
    stamp[1] = __builtin_amdgcn_s_memrealtime();
#endif
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 2, wq = wave & 3;                 // key group (tile parity) / 64-row slice of the block
    const int r = lane & 31, h = lane >> 5;

    // ---- persistent form (p.persist = blocks per workgroup; 0: one block per workgroup): the static, balanced block list of
    // fa_fwd_w64.hpp -- XCD x owns an eighth of the (batch, q-head) columns, its blocks (q-blocks descending inside a column) are dealt
    // out 32 at a time alternately forwards and backwards over its 32 workgroups ----------------------------------------------------
    const int n_steps_pers = (kGeneral && p.persist > 0) ? p.persist : 1;
    for (int pstep = 0; pstep < n_steps_pers; ++pstep) {
    int qblk, bh;
    if (kGeneral && p.persist > 0) {
        const int x = (int)blockIdx.x & 7, c = (int)blockIdx.x >> 3;
        const int pos = 32 * pstep + ((pstep & 1) ? 31 - c : c);
        const int col = pos / p.n_qblk;
        qblk = p.persist_asc ? pos - col * p.n_qblk : p.n_qblk - 1 - (pos - col * p.n_qblk);
        if (p.persist_hx > 0) bh = (col / p.persist_hx) * p.QH + x * p.persist_hx + col % p.persist_hx;
        else bh = x * ((p.B * p.QH) >> 3) + col;
    } else {
        const int lin = xcd_remap_chunked((int)blockIdx.x, p.n_wg, p.n_qblk * (p.QH / p.KH));
        qblk = lin % p.n_qblk;
        bh = lin / p.n_qblk;
        if (kGeneral && p.causal) qblk = p.n_qblk - 1 - qblk; // heaviest q-blocks first
    }
    const int b = bh / p.QH, qh = bh - b * p.QH;
    const int kvh = qh / (p.QH / p.KH);                       // cld(q_head, n_q_per_kv), 0-based (src/attention.jl:28)
    const int q0w = qblk * RB + wq * RW;                      // first query row of this wave (and of its partner)
    int qi[NZ];
#pragma unroll
    for (int z = 0; z < NZ; ++z) qi[z] = q0w + 32 * z + r;

    const T* __restrict__ qp = (const T*)p.q + ((size_t)bh * p.QL) * E;
    const char* __restrict__ kp = (const char*)((const T*)p.k + ((size_t)(b * p.KH + kvh) * p.KL) * E);
    const char* __restrict__ vp = (const char*)((const T*)p.v + ((size_t)(b * p.KH + kvh) * p.KL) * E);
    const uint8_t* __restrict__ mp = kGeneral && p.kpad ? p.kpad + (size_t)b * p.KL : nullptr;

    const uint32_t lds0 = (uint32_t)(uintptr_t)smem;
    const uint32_t kring = lds0, vring = lds0 + NS * KBYTES;
    uint64_t* const vbits = reinterpret_cast<uint64_t*>(smem + MASK_OFF + 16);

    // ---- number of kv tiles (workgroup) / live tiles (this wave): as in fa_fwd_w64.hpp ---------------------------------------------
    int n_tiles = (p.KL + BK - 1) / BK;
    int causal_q0 = 0x3fffffff;
    int qlim[2] = {0x3fffffff, 0x3fffffff};                  // (entry 1 unused at NZ = 1)
    if constexpr (kGeneral) {
        if (p.causal) {
            int q_last = qblk * RB + RB - 1;
            if (q_last > p.QL - 1) q_last = p.QL - 1;
            const int t_c = q_last / BK + 1;
            if (t_c < n_tiles) n_tiles = t_c;
            causal_q0 = q0w;
#pragma unroll
            for (int z = 0; z < NZ; ++z) qlim[z] = qi[z];
        }
        if (mp) {
            int* slot = reinterpret_cast<int*>(smem + MASK_OFF);
            const int nk = n_tiles * BK < p.KL ? n_tiles * BK : p.KL;
            const int last = kpad_scan(mp, p.KL, nk, vbits, kMaxMaskTiles, slot, tid, 512);
            const int t_m = last / BK + 1;
            if (t_m < n_tiles) n_tiles = t_m;
        } else {
            for (int w = tid; w < n_tiles; w += 512) {
                const int left = p.KL - w * BK;
                vbits[w] = left >= 64 ? ~0ull : ((1ull << left) - 1ull);
            }
            __syncthreads();
        }
    }
    int n_live = n_tiles;
    if (kGeneral && p.causal) {
        const int t_w = (q0w + RW - 1) / BK + 1;
        if (t_w < n_live) n_live = t_w;
    }

    // ---- per-lane DMA source offsets inside a tile (the image's layout applied to the SOURCE; fa_fwd_w64.hpp) ---------------------
    uint32_t k_voff[NJK];
#pragma unroll
    for (int j = 0; j < NJK; ++j) {
        const int off = (wq * NJK + j) * 1024 + lane * 16;
        const int row = off / KImg::kRowBytes, phys = (off % KImg::kRowBytes) >> 4;
        k_voff[j] = (uint32_t)(row * KImg::kRowBytes + ((phys ^ KImg::xor_of(row)) << 4) - j * 1024);
    }
    uint32_t v_voff;
    {
        const int off = (wq * NJV) * 1024 + lane * 16;
        const int blk = off >> 8, rg = blk / VImg::kEB, eb = blk % VImg::kEB, rr = (off >> 6) & 3, c4 = (off >> 4) & 3;
        v_voff = (uint32_t)((4 * rg + rr) * KImg::kRowBytes + ((4 * eb + c4) << 4));
    }
    static_assert((1024 / 256) % VImg::kEB == 0 && (4 * (1024 / 256 / VImg::kEB)) * VImg::kRowBytes == 1024, "V image: 1 KiB = whole row groups");
    const uint32_t wave_off_k = (uint32_t)(wq * NJK * 1024), wave_off_v = (uint32_t)(wq * NJV * 1024);
    const uint32_t kv_bytes = (uint32_t)p.KL * (uint32_t)KImg::kRowBytes;
    const u32x4 krs = make_rsrc(kp, kv_bytes), vrs = make_rsrc(vp, kv_bytes);
    // past the last tile the LAST tile is copied again (into a ring slot nobody reads any more): no branch around an issue
    auto tile_off = [&](int t) -> uint32_t { return (uint32_t)(t < n_tiles ? t : n_tiles - 1) * (uint32_t)TILE_BYTES; };
    auto issue_k_piece = [&](uint32_t soff, uint32_t dst, auto jc) {
        constexpr int j = decltype(jc)::value;
        dma_piece<j, j == 0>(krs, k_voff[j], soff, dst);
    };
    // Rings of NS slots, NS / 2 per key group.  At iteration t (LDS byte address + this wave's DMA share): kA = slot of K(t), read in M(t);
    // kB = slot of K(t+2); kC = the free slot, target of K(t+4) (with 2 slots per group: kA again, and the batch is then issued behind the
    // barrier that closes M(t)).  vA = slot of V(t-2), read in M(t); vB = slot of V(t); vC = free, target of V(t+2).  The group's slots
    // rotate (A, B, C) <- (B, C, A) per iteration.
    constexpr int SPG = duo_slots_per_group<E>();
    const uint32_t kA = kring + wave_off_k + (uint32_t)(SPG * grp) * KBYTES, kB = kA + KBYTES, kC = kA + (SPG - 1) * KBYTES;
    const uint32_t vA = vring + wave_off_v + (uint32_t)(SPG * grp) * VBYTES, vB = vA + VBYTES, vC = vA + (SPG - 1) * VBYTES;
    // ragged KL: rows of the last tile past KL are outside the descriptor's range -- the ring must not hold non-finite garbage there
    if (kGeneral && (p.KL & (BK - 1)) != 0) {
        for (int i = tid * 16; i < RING; i += 512 * 16) *reinterpret_cast<u32x4*>(smem + i) = u32x4{0, 0, 0, 0};
        __syncthreads();
    }
    // ---- prologue: the group's first tiles in flight -- K(g), K(g+2), V(g) (the loop's first batch is K(g+4), V(g+2)) -----------------
    static_for<NJK>([&](auto jc) { issue_k_piece(tile_off(grp), kA, jc); });
    const float c2 = p.scale * kLog2e;
    // Q fragments: asm loads (invisible to hipcc's wait-count bookkeeping, like the LDS-DMA around them), valid behind the counted wait
    // below, which takes them as operands
    f32x4 qw[NZ][KS];
#pragma unroll
    for (int z = 0; z < NZ; ++z) {
        const int qc = qi[z] < p.QL ? qi[z] : p.QL - 1;
        const T* qrow = qp + (size_t)qc * E;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(qw[z][ks]) : "v"(qrow + 16 * ks + 8 * h) : "memory");
    }
    f32x16 oacc[NZ][EB];
    f32x4 lacc[NZ];                                            // row sums: registers 0 / 1 of lanes 0..15 = queries lane, lane + 16 (SumMfma)
#pragma unroll
    for (int z = 0; z < NZ; ++z) {
#pragma unroll
        for (int eb = 0; eb < EB; ++eb)
#pragma unroll
            for (int i = 0; i < 16; ++i) oacc[z][eb][i] = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) lacc[z][i] = 0.f;
    }
    // Row sums of P on the matrix pipe with the 16x16x32 shape: half the pipe time and a quarter of the accumulator registers of a
    // ones x P^T product in the 32x32x16 shape.  The B operand is a P^T fragment AS IT IS (lane (r, h) = lane l: 8 keys of query r): the
    // 16x16x32 instruction reads lane l as column l % 16, contraction group l / 16, i.e. it would add queries r and r + 16 together --
    // unless the A operand separates them: row m of A is one where contraction group g has g % 2 == m (rows 2..15 zero), so
    //   D[0][n] = sum over the keys of query n,   D[1][n] = the same for query n + 16      (n = 0..15),
    // which land in accumulator registers 0 and 1 of lanes 0..15 (the other lanes and registers hold zero rows).
    f32x4 sel;
    {
        frag_t sf;
#pragma unroll
        for (int j = 0; j < 8; ++j) sf[j] = from_f32<T>((((lane >> 4) & 1) == (lane & 15)) ? 1.0f : 0.0f);
        sel = __builtin_bit_cast(f32x4, sf);
    }
    static_for<NJK>([&](auto jc) { issue_k_piece(tile_off(grp + 2), kB, jc); });
    static_for<NJV>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        dma_piece<j, j == 0>(vrs, v_voff, tile_off(grp), vB);
    });
    const uint32_t k_lane = (uint32_t)(r * KImg::kRowBytes + ((KImg::xor_of(r) ^ h) << 4)) - wave_off_k;
    const uint32_t v_lane = (uint32_t)VImg::lane_base(lane) - wave_off_v;
    // K(grp) and Q landed (every wave's pieces: barrier); K(grp+2) and V(grp) -- the NJK + NJV pieces issued last -- stay in flight: the
    // loop's first counted wait (end of V(grp)) retires them, in time for M(grp+2).  The Q fragments pass through the statement.
    if constexpr (E == 32)
        asm volatile("s_waitcnt vmcnt(%c[n])\n\ts_barrier" : "+v"(qw[0][0]), "+v"(qw[0][KS - 1]), "+v"(qw[NZ - 1][0]), "+v"(qw[NZ - 1][KS - 1]) : [n] "n"(NJK + NJV) : "memory");
    else if constexpr (E == 128)
        asm volatile("s_waitcnt vmcnt(%c[n])\n\ts_barrier"
                     : "+v"(qw[0][0]), "+v"(qw[0][1]), "+v"(qw[0][2]), "+v"(qw[0][3]), "+v"(qw[0][KS - 4]), "+v"(qw[0][KS - 3]), "+v"(qw[0][KS - 2]),
                       "+v"(qw[0][KS - 1])
                     : [n] "n"(NJK + NJV) : "memory");
    else if constexpr (NZ == 2)
        asm volatile("s_waitcnt vmcnt(%c[n])\n\ts_barrier"
                     : "+v"(qw[0][0]), "+v"(qw[0][1]), "+v"(qw[0][2]), "+v"(qw[0][3]), "+v"(qw[NZ - 1][0]), "+v"(qw[NZ - 1][1]), "+v"(qw[NZ - 1][2]),
                       "+v"(qw[NZ - 1][3])
                     : [n] "n"(NJK + NJV) : "memory");
    else
        asm volatile("s_waitcnt vmcnt(%c[n])\n\ts_barrier" : "+v"(qw[0][0]), "+v"(qw[0][1]), "+v"(qw[0][2]), "+v"(qw[0][3]) : [n] "n"(NJK + NJV) : "memory");
    // the fragments (16-deep steps of E) as 16-register tuples: v[64:79], v[80:95] = query blocks 0, 1 at E = 64 / steps 0-3, 4-7 at E = 128
    // (E = 32: two fragments per query block, in the first half of that block's tuple)
    constexpr int NQT = E == 32 ? NZ : NZ * KS / 4;
    f32x16 qf[NQT];
    if constexpr (E == 32) {
#pragma unroll
        for (int z = 0; z < NZ; ++z)
#pragma unroll
            for (int i = 0; i < 16; ++i) qf[z][i] = i < 4 * KS ? qw[z][(i >> 2) % KS][i & 3] : 0.f;
    } else {
#pragma unroll
        for (int z = 0; z < NZ; ++z)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                for (int i = 0; i < 4; ++i) qf[(z * KS + ks) / 4][4 * (ks & 3) + i] = qw[z][ks][i];
    }
#if NNOP_DUO_STAMP
    stamp[2] = __builtin_amdgcn_s_memtime();
    stamp[3] = __builtin_amdgcn_s_memrealtime();
#endif

    // the score tile S(t)^T: [z][key block].  V(t) packs P(t)^T IN PLACE: the 8 logits of 16-key step kk (registers 8 (kk & 1) .. + 7 of
    // sc[z][kk >> 1]) become 4 operand words in the first 4 of those registers.
    f32x16 sc[NZ][KB];
#pragma unroll
    for (int z = 0; z < NZ; ++z)
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
            for (int i = 0; i < 16; ++i) sc[z][kb][i] = 0.f;

    // ---- the phase loop (generated, tools/gen_duo_asm.py): half-steps h = 0 .. n_tiles + 1, one barrier each; group g runs the matrix
    // phase M(t) at h = t for t = g (mod 2) -- [row sums of P(t-2)] [O += V(t-2)^T P(t-2)^T] [S(t) = K(t) Q^T], the LDS-DMA of K(t+2) and
    // V(t) in its gaps -- and the vector phase V(t) at h = t + 1: mask, row max, (rare) raise of the reference, P = exp2(s c - m) packed
    // as MFMA operand words ------------------------------------------------------------------------------------------------------------
    f32x4 mstate = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};       // m2[0..1] (exponent reference), mt[0..1] (true row max)
    typedef uint32_t u32x8 __attribute__((ext_vector_type(8)));
    u32x8 vconst;
    vconst[0] = k_voff[0]; vconst[1] = k_voff[NJK > 1 ? 1 : 0]; vconst[2] = v_voff; vconst[3] = k_lane; vconst[4] = v_lane;
    vconst[5] = (uint32_t)qlim[0]; vconst[6] = (uint32_t)qlim[1]; vconst[7] = (uint32_t)(4 * h);
    // the loop's scalar state (wave-uniform: hipcc hands them over in scalar registers)
    int s_t = grp, s_h = n_tiles + 2, s_nlive = n_live, s_cq0 = causal_q0;
    uint32_t s_ka = kA, s_kb = kB, s_kc = kC, s_va = vA, s_vb = vB, s_vc = vC;
    const uint32_t s_last = (uint32_t)(n_tiles - 1) * (uint32_t)TILE_BYTES, s_vbits = (uint32_t)(uintptr_t)vbits;
#if NNOP_DUO_STAMP
    f32x8 profv = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#endif
#if NNOP_DUO_VALU_SUMS
    f32x4 lsum = {0.f, 0.f, 0.f, 0.f};                        // row sums, VALU form: two chains per query block, this lane's half of the keys
#endif
#if NNOP_DUO_PRIO == 2
    if (grp) __builtin_amdgcn_s_setprio(1);
#endif
    if constexpr (!duo_sync_one<E>()) {
        if (grp) asm volatile("s_barrier" ::: "memory");      // half-step 0: group 1 has nothing to do yet
    }
#if NNOP_DUO_STAMP
#define NNOP_DUO_LOOP_MASKED NNOP_DUO_LOOP_MASKED_PROF
#define NNOP_DUO_LOOP_PLAIN NNOP_DUO_LOOP_PLAIN_PROF
#endif
    // (experiments, make DEV=1 VAR=-DNNOP_DUO_PRIO=n: 1 matrix phase at s_setprio 1, 2 waves 4-7 at priority 1 throughout, 3 vector phase at 1)
#if NNOP_DUO_PRIO == 1
#define NNOP_DUO_PRIO_ARGS "s_setprio 1", "s_setprio 0", "", ""
#elif NNOP_DUO_PRIO == 3
#define NNOP_DUO_PRIO_ARGS "", "", "s_setprio 1", "s_setprio 0"
#else
#define NNOP_DUO_PRIO_ARGS "", "", "", ""
#endif
#define NNOP_DUO_X(M, ...) M(__VA_ARGS__)
    if constexpr (E == 32) {
        if constexpr (std::is_same<T, __bf16>::value) {
            if constexpr (kGeneral) asm volatile(NNOP_DUO_X(NNOP_DUO32_LOOP_MASKED, "bf16", NNOP_DUO_PRIO_ARGS) : NNOP_DUO32_OPERANDS);
            else asm volatile(NNOP_DUO_X(NNOP_DUO32_LOOP_PLAIN, "bf16", NNOP_DUO_PRIO_ARGS) : NNOP_DUO32_OPERANDS);
        } else {
            if constexpr (kGeneral) asm volatile(NNOP_DUO_X(NNOP_DUO32_LOOP_MASKED, "f16", NNOP_DUO_PRIO_ARGS) : NNOP_DUO32_OPERANDS);
            else asm volatile(NNOP_DUO_X(NNOP_DUO32_LOOP_PLAIN, "f16", NNOP_DUO_PRIO_ARGS) : NNOP_DUO32_OPERANDS);
        }
    } else if constexpr (NZ == 2) {
        if constexpr (std::is_same<T, __bf16>::value) {
            if constexpr (kGeneral) asm volatile(NNOP_DUO_X(NNOP_DUO_LOOP_MASKED, "bf16", NNOP_DUO_PRIO_ARGS) : NNOP_DUO_OPERANDS);
            else asm volatile(NNOP_DUO_X(NNOP_DUO_LOOP_PLAIN, "bf16", NNOP_DUO_PRIO_ARGS) : NNOP_DUO_OPERANDS);
        } else {
            if constexpr (kGeneral) asm volatile(NNOP_DUO_X(NNOP_DUO_LOOP_MASKED, "f16", NNOP_DUO_PRIO_ARGS) : NNOP_DUO_OPERANDS);
            else asm volatile(NNOP_DUO_X(NNOP_DUO_LOOP_PLAIN, "f16", NNOP_DUO_PRIO_ARGS) : NNOP_DUO_OPERANDS);
        }
    } else if constexpr (E == 128) {
        if constexpr (std::is_same<T, __bf16>::value) {
            if constexpr (kGeneral) asm volatile(NNOP_DUO_X(NNOP_DUO128_LOOP_MASKED, "bf16", NNOP_DUO_PRIO_ARGS) : NNOP_DUO128_OPERANDS);
            else asm volatile(NNOP_DUO_X(NNOP_DUO128_LOOP_PLAIN, "bf16", NNOP_DUO_PRIO_ARGS) : NNOP_DUO128_OPERANDS);
        } else {
            if constexpr (kGeneral) asm volatile(NNOP_DUO_X(NNOP_DUO128_LOOP_MASKED, "f16", NNOP_DUO_PRIO_ARGS) : NNOP_DUO128_OPERANDS);
            else asm volatile(NNOP_DUO_X(NNOP_DUO128_LOOP_PLAIN, "f16", NNOP_DUO_PRIO_ARGS) : NNOP_DUO128_OPERANDS);
        }
    } else {
        if constexpr (std::is_same<T, __bf16>::value) {
            if constexpr (kGeneral) asm volatile(NNOP_DUO_X(NNOP_DUO1_LOOP_MASKED, "bf16", NNOP_DUO_PRIO_ARGS) : NNOP_DUO1_OPERANDS);
            else asm volatile(NNOP_DUO_X(NNOP_DUO1_LOOP_PLAIN, "bf16", NNOP_DUO_PRIO_ARGS) : NNOP_DUO1_OPERANDS);
        } else {
            if constexpr (kGeneral) asm volatile(NNOP_DUO_X(NNOP_DUO1_LOOP_MASKED, "f16", NNOP_DUO_PRIO_ARGS) : NNOP_DUO1_OPERANDS);
            else asm volatile(NNOP_DUO_X(NNOP_DUO1_LOOP_PLAIN, "f16", NNOP_DUO_PRIO_ARGS) : NNOP_DUO1_OPERANDS);
        }
    }
    // (the loop keeps the true row max per lane half -- lane l ^ 32 holds the same query's other keys: combined here, once)
    float m2[NZ], mt[NZ];
#pragma unroll
    for (int z = 0; z < NZ; ++z) {
        m2[z] = mstate[z];
        mt[z] = half_swap_max(mstate[2 + z]);
    }
#if NNOP_DUO_STAMP
    stamp[4] = __builtin_amdgcn_s_memtime();
    stamp[5] = __builtin_amdgcn_s_memrealtime();
#endif
    // the rings are dead from here on (the exchange buffer overlays them): every DMA landed, every wave past its last fragment read
    asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");

    // ---- epilogue: the partners exchange one 32-row half each through LDS, merge the two key groups, normalise, store --------------
    asm volatile(NNOP_FENCE_128 ::: "memory");                // the last MFMAs have written O and the row sums
    __builtin_amdgcn_sched_barrier(0);
    // wave w writes the half it gives away into its own exchange block; after the barrier it reads its partner's block (the other
    // key group's partial result for the rows it keeps)
    char* const mine = smem + wave * (8192 + 3 * 256);
    const char* const theirs = smem + (wave ^ 4) * (8192 + 3 * 256);
#if NNOP_DUO_VALU_SUMS
    lacc[0][0] = half_swap_sum(lsum[0] + lsum[1]);            // (both lane halves: lane l ^ 32 holds the same query's other keys)
    if constexpr (NZ == 2) lacc[NZ - 1][0] = half_swap_sum(lsum[2] + lsum[3]);
    auto row_sum = [&](const f32x4& l) -> float { return l[0]; };
#else
    auto row_sum = [&](const f32x4& l) -> float {            // this lane's query r: lane r % 16, register r / 16
        const float l0 = __shfl(l[0], r & 15), l1 = __shfl(l[1], r & 15);
        return (r & 16) ? l1 : l0;
    };
#endif
    // what a wave gives away / keeps: at NZ = 2 a whole 32-row block z (all E columns), at NZ = 1 one 32-column half eb of its only block
    auto give = [&](auto givec, auto eb0c, auto nebc) {
        constexpr int ZG = decltype(givec)::value, EB0 = decltype(eb0c)::value, NEB = decltype(nebc)::value;
#pragma unroll
        for (int eb = EB0; eb < EB0 + NEB; ++eb) {
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const f32x4 w = {oacc[ZG][eb][4 * g4], oacc[ZG][eb][4 * g4 + 1], oacc[ZG][eb][4 * g4 + 2], oacc[ZG][eb][4 * g4 + 3]};
                *reinterpret_cast<f32x4*>(mine + (((eb - EB0) * 4 + g4) * 64 + lane) * 16) = w;
            }
        }
        float* sm = reinterpret_cast<float*>(mine + 8192);
        sm[lane] = row_sum(lacc[ZG]);
        sm[64 + lane] = m2[ZG];
        sm[128 + lane] = mt[ZG];
    };
    float sink2 = -INFINITY;
    if constexpr (SINK) sink2 = p.sinks[qh] * kLog2e;                     // one load per block
    auto take = [&](auto keepc, auto eb0c, auto nebc, auto statsc) {
        constexpr int ZK = decltype(keepc)::value, EB0 = decltype(eb0c)::value, NEB = decltype(nebc)::value;
        constexpr bool kStats = decltype(statsc)::value;
        const float* so_ = reinterpret_cast<const float*>(theirs + 8192);
        const float l_o = so_[lane], m_o = so_[64 + lane], mt_o = so_[128 + lane];
        const float l_m = row_sum(lacc[ZK]), m_m = m2[ZK];
        float mm = fmaxf(m_m, m_o);
        float a = m_m == -INFINITY ? 0.f : fast_exp2(m_m - mm);
        float bsc = m_o == -INFINITY ? 0.f : fast_exp2(m_o - mm);
        float ltot = a * l_m + bsc * l_o;
        float mtt = fmaxf(mt[ZK], mt_o);
        if constexpr (SINK) {                                // the sink (nnop_fa_fwd_sinks): a third partial (wave-uniform)
            const float g = sink_merge(sink2, mm, ltot, mtt);
            a *= g;
            bsc *= g;
        }
        const float inv = 1.0f / ltot;                       // ltot == 0 (no visible key, no sink) -> NaN rows, as the naive formula gives
        const float ai = a * inv, bi = bsc * inv;
        T* orow = (T*)p.o + ((size_t)bh * p.QL + (qi[ZK] < p.QL ? qi[ZK] : p.QL - 1)) * E;
#pragma unroll
        for (int eb = EB0; eb < EB0 + NEB; ++eb) {
            uint32_t pk[4][2];
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                typedef T t4 __attribute__((ext_vector_type(4)));
                const f32x4 ot = *reinterpret_cast<const f32x4*>(theirs + (((eb - EB0) * 4 + g4) * 64 + lane) * 16);
                const f32x4 w = {oacc[ZK][eb][4 * g4] * ai + ot[0] * bi, oacc[ZK][eb][4 * g4 + 1] * ai + ot[1] * bi,
                                 oacc[ZK][eb][4 * g4 + 2] * ai + ot[2] * bi, oacc[ZK][eb][4 * g4 + 3] * ai + ot[3] * bi};
                const u32x2 u = __builtin_bit_cast(u32x2, __builtin_convertvector(w, t4));
                pk[g4][0] = u[0];
                pk[g4][1] = u[1];
            }
#pragma unroll
            for (int g4 = 0; g4 < 4; g4 += 2) {
                // lanes 0-31 end up with e = 32 eb + 8 g + (0..7), lanes 32-63 with e = 32 eb + 8 (g+1) + (0..7)
                const auto x0 = __builtin_amdgcn_permlane32_swap(pk[g4][0], pk[g4 + 1][0], false, false);
                const auto x1 = __builtin_amdgcn_permlane32_swap(pk[g4][1], pk[g4 + 1][1], false, false);
                const u32x4 lo = {x0[0], x1[0], x0[1], x1[1]};
                if (qi[ZK] < p.QL) *reinterpret_cast<u32x4*>(orow + 32 * eb + 8 * g4 + 8 * h) = lo;
            }
        }
        if (kStats && qi[ZK] < p.QL && h == 0) {
            // residual contract (src/attention.jl:128-129): ms = row max (natural-log units) rounded to T, ls relative to the ROUNDED ms
            const size_t so = (size_t)bh * p.QL + qi[ZK];
            const T m_t = from_f32<T>(mtt * kLn2);
            const float m_back = to_f32(m_t);
            float l_out = ltot;
            if (mtt != -INFINITY) l_out = ltot * fast_exp2(mm - m_back * kLog2e);
            ((T*)p.ms)[so] = m_t;
            ((T*)p.ls)[so] = from_f32<T>(l_out);
        }
    };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    using IE = std::integral_constant<int, EB>;
    if constexpr (NZ == 2) {
        // group 0 keeps the rows of z = 0 and gives z = 1 away, group 1 the other way round
        if (grp == 0) give(I1{}, I0{}, IE{});
        else give(I0{}, I0{}, IE{});
        __syncthreads();
        if (grp == 0) take(I0{}, I0{}, IE{}, std::true_type{});
        else take(I1{}, I0{}, IE{}, std::true_type{});
    } else {
        // both partners finish the same 32 rows: group 0 the first half of the columns (and the residuals), group 1 the second
        using IH = std::integral_constant<int, EB / 2>;       // (E = 64: 1 block of 32 columns each, E = 128: 2)
        if (grp == 0) give(I0{}, IH{}, IH{});
        else give(I0{}, I0{}, IH{});
        __syncthreads();
        if (grp == 0) take(I0{}, I0{}, IH{}, std::true_type{});
        else take(I0{}, IH{}, IH{}, std::false_type{});
    }
#if NNOP_DUO_STAMP
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    stamp[6] = __builtin_amdgcn_s_memtime();
    stamp[7] = __builtin_amdgcn_s_memrealtime();
    if (tid == 0) {
        uint64_t* dbg = reinterpret_cast<uint64_t*>((T*)p.o + ((size_t)bh * p.QL + q0w) * E);
        for (int i = 0; i < 8; ++i) dbg[i] = stamp[i];
        dbg[8] = (uint64_t)n_tiles;
        dbg[9] = stamp[2];
        dbg[10] = stamp[2];
        for (int i = 0; i < 5; ++i) dbg[11 + i] = (uint64_t)__float_as_uint(profv[i]);     // cycles in M, barrier, V, DMA wait, barrier (wave 0)
    }
    if (tid == 256) {                                         // the same five of wave 4 (key group 1), in the block's second row
        uint64_t* dbg = reinterpret_cast<uint64_t*>((T*)p.o + ((size_t)bh * p.QL + q0w + 1) * E);
        for (int i = 0; i < 5; ++i) dbg[i] = (uint64_t)__float_as_uint(profv[i]);
    }
#endif
    // the next block's prologue overwrites the rings / the exchange buffer / the validity words: every wave is done with them
    if (pstep + 1 < n_steps_pers) __syncthreads();
    }   // blocks of this workgroup
}
