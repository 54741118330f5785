// fa_fwd_generic_kernel.inc -- the body of fa_fwd_generic_kernel (fa_generic.hpp).
// SINK = learned attention sinks merged in the epilogue, CAP = logit soft-capping with the runtime constants p.cap_ka / p.cap_kb:
// instantiations of their own, so that the kernel of the calls without them is this text with the feature compiled away.
template <typename T, bool SINK = false, bool CAP = false>
__global__ __launch_bounds__(256) void fa_fwd_generic_kernel(const FwdParams p, int E, long long n_rows) {
    __shared__ float qs_all[4][kGenericMaxE];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + wave;
    if (row >= n_rows) return;                                    // wave-uniform; no workgroup barrier below
    const int qi = (int)(row % p.QL);
    const int bh = (int)(row / p.QL);
    const int b = bh / p.QH, qh = bh - b * p.QH;
    const int kvh = qh / (p.QH / p.KH);
    float* qs = qs_all[wave];
    const T* q = (const T*)p.q + row * E;
    for (int e = lane; e < E; e += 64) qs[e] = to_f32(q[e]);
    __builtin_amdgcn_wave_barrier();
    const T* kb = (const T*)p.k + ((size_t)(b * p.KH + kvh) * p.KL) * E;
    const T* vb = (const T*)p.v + ((size_t)(b * p.KH + kvh) * p.KL) * E;
    const uint8_t* mp = p.kpad ? p.kpad + (size_t)b * p.KL : nullptr;
    int kbeg, kend;
    generic_key_range(p.causal, p.win_left, p.win_right, qi, p.KL, kbeg, kend);
    float m = -INFINITY, l = 0.f, oacc[kGenericMaxE / 64];
#pragma unroll
    for (int j = 0; j < kGenericMaxE / 64; ++j) oacc[j] = 0.f;
    for (int k0 = kbeg; k0 < kend; k0 += 64) {
        const int k = k0 + lane;
        const bool valid = k < kend && (!mp || mp[k] != 0);
        const int kc = k < p.KL ? k : p.KL - 1;
        float s = dot_lds(qs, kb + (size_t)kc * E, E);
        if constexpr (CAP) s = cap_tanh(s, p.cap_ka) * (p.cap_kb * kLn2);     // c * tanh(s * scale / c), before the bias
        else s *= p.scale;
        if (p.pair) s += to_f32(((const T*)p.pair)[(((size_t)b * p.KL + kc) * p.QL + qi) * p.QH + qh]);
        if (!valid) s = -INFINITY;
        const float m_new = fmaxf(m, wave_max64(s));
        if (m_new == -INFINITY) continue;                         // no visible key so far (wave-uniform)
        const float pr = valid ? __expf(s - m_new) : 0.f;
        const float alpha = __expf(m - m_new);                   // m = -inf -> 0
        l = l * alpha + wave_sum64(pr);
        m = m_new;
#pragma unroll
        for (int j = 0; j < kGenericMaxE / 64; ++j) oacc[j] *= alpha;
        const int nk = kend - k0 < 64 ? kend - k0 : 64;
        for (int kk = 0; kk < nk; ++kk) {
            const float pk = lane_bcast(pr, kk);
            const T* vr = vb + (size_t)(k0 + kk) * E;
#pragma unroll
            for (int j = 0; j < kGenericMaxE / 64; ++j) {
                const int e = lane + 64 * j;
                if (e < E) oacc[j] += pk * to_f32(vr[e]);
            }
        }
    }
    float osc = 1.f;
    if constexpr (SINK) {
        const float sg = p.sinks[qh];
        if (sg != -INFINITY) {                                    // the sink (nnop_fa_fwd_sinks), natural units: one more partial
            const float mm = fmaxf(m, sg);
            osc = __expf(m - mm);                                 // m = -inf -> 0
            l = l * osc + __expf(sg - mm);
            m = mm;
        }
    }
    const float inv = osc / l;                                    // l == 0 (no visible key, no sink) -> NaN row, as the naive formula gives
    T* o = (T*)p.o + row * E;
#pragma unroll
    for (int j = 0; j < kGenericMaxE / 64; ++j) {
        const int e = lane + 64 * j;
        if (e < E) o[e] = from_f32<T>(oacc[j] * inv);
    }
    if (lane == 0) {
        // residual contract (src/attention.jl:128-129): ms = row max rounded to T, ls relative to the ROUNDED ms
        const T m_t = from_f32<T>(m);
        float l_out = l;
        if (m != -INFINITY) l_out = l * __expf(m - to_f32(m_t));
        ((T*)p.ms)[row] = m_t;
        ((T*)p.ls)[row] = from_f32<T>(l_out);
    }
}
