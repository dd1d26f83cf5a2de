// ssd_gru_seq_kernels.h -- the text of the recurrence kernels; included by ssd_gru_seq.hip once per form (GRU_H0 0: from a zero state,
// GRU_H0 1: from a given state, see GruH0).  Not a header in its own right.
//
// GRU_H0 1: step 0 is not computed.  Forward: each compute lane LOADS its four features of the row's given state (in front of the
// prefetch of gi) and publishes them like any step's result -- LDS operand image, staging image -> hs[0], zeros for rzn / ghn of step 0;
// gi[0] is never read; steps t >= 1 are the same code.  Backward: the walk ends at t = 1; step 0 stages zeros for d_gi[0] and dgh[0],
// adds nothing to dL/db_h and sends no gradient into the given state.  hs[0] is h_{t-1} of step 1, so the d_wh product after the walk
// (launch_gru_seq_bwd) is unchanged.
#if GRU_H0
#define GRU_FWD_KERNEL k_gru_seq_fwd_h0
#define GRU_BWD_KERNEL k_gru_seq_bwd_h0
#define GRU_H0_PARAM const GruH0 h0,
#define GRU_T1 1                   /* the first step that is computed */
#else
#define GRU_FWD_KERNEL k_gru_seq_fwd
#define GRU_BWD_KERNEL k_gru_seq_bwd
#define GRU_H0_PARAM
#define GRU_T1 0
#endif
#if !GRU_H0
constexpr int FST = 324;            // staging row stride (floats): [hs 64 | r 64 | z 64 | n 64 | gh_n 64] + pad, 1296 B = 16 * 81
// BF: the labelled reduced-precision variant (learner_dtype: bf16): W_h and the state as single bf16 terms, ONE v_mfma_f32_16x16x32_bf16
// per product (6 per step instead of 18), no scales (bf16 has f32's exponent range), f32 accumulation and gate arithmetic.
#endif
template <bool TRAIN, bool BF = false>
__global__ __launch_bounds__(GRU_THREADS) void GRU_FWD_KERNEL(const GruParts gi, const GruW W, GRU_H0_PARAM
                                                             float* __restrict__ hs, float* __restrict__ rzn, float* __restrict__ ghn, int T, int G,
                                                             int B, int tiles, int32_t* __restrict__ err) {
    __shared__ __attribute__((aligned(16))) _Float16 hx[2][2][16][HSH];   // [buffer][term][row][feature]
    __shared__ __attribute__((aligned(16))) float st[2][16][FST];         // [buffer][row][staged results of the step]
    const int tid = threadIdx.x, lane = tid & 63, ft = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = blockIdx.x / tiles, tile = blockIdx.x - g * tiles;
    if (ft == GRU_COMPUTE_WAVES) {                                     // the writer wave
        float* hs_t = hs + (((size_t)g * T) * B + tile * 16) * GH + 4 * lane;          // + t * B * GH
        float* rzn_t = TRAIN ? rzn + ((size_t)g * B + tile * 16) * G3 + 4 * lane : nullptr;   // + t * G * B * G3
        float* ghn_t = TRAIN ? ghn + ((size_t)g * B + tile * 16) * GH + 4 * lane : nullptr;   // + t * G * B * GH
        for (int t = 0; t < T; ++t) {
            lds_barrier();                                             // the step's image is complete
            const float* im = &st[t & 1][0][0];
            f32x4 vh[4], vr[TRAIN ? 12 : 1], vn[TRAIN ? 4 : 1];
#pragma unroll
            for (int i = 0; i < 4; ++i) { int r, c; piece_rc<GH>(i, lane, r, c); vh[i] = *reinterpret_cast<const f32x4*>(im + r * FST + c); }
            if constexpr (TRAIN) {
#pragma unroll
                for (int i = 0; i < 12; ++i) { int r, c; piece_rc<G3>(i, lane, r, c); vr[i] = *reinterpret_cast<const f32x4*>(im + r * FST + GH + c); }
#pragma unroll
                for (int i = 0; i < 4; ++i) { int r, c; piece_rc<GH>(i, lane, r, c); vn[i] = *reinterpret_cast<const f32x4*>(im + r * FST + 4 * GH + c); }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(hs_t + (size_t)t * B * GH + 256 * i) = vh[i];
            if constexpr (TRAIN) {
#pragma unroll
                for (int i = 0; i < 12; ++i) *reinterpret_cast<f32x4*>(rzn_t + (size_t)t * G * B * G3 + 256 * i) = vr[i];
#pragma unroll
                for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(ghn_t + (size_t)t * G * B * GH + 256 * i) = vn[i];
            }
        }
        return;
    }
    const int m = lane & 15, q = lane >> 4;
    const int row = tile * 16 + m, rc = row;
    const float* __restrict__ wh = gru_wh(W, g);                       // this weight set's [64, 192] / [192]
    const float* __restrict__ bh = gru_bh(W, g);
    // resident A fragments: lane (q, m) = output feature gate * 64 + 16 ft + m, reduction indices k = 32 s + 8 q + j
    u32x4 ah[3][2], al[3][2];
    bool out_of_range = false;                                        // ONE test after the 48 loads: a branch per value made each load wait for the one before (14 us)
#pragma unroll
    for (int gate = 0; gate < 3; ++gate)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if constexpr (BF) {
                b8 h;
#pragma unroll
                for (int j = 0; j < 8; ++j) h[j] = (__bf16)wh[(size_t)(32 * s + 8 * q + j) * G3 + gate * GH + 16 * ft + m];
                ah[gate][s] = __builtin_bit_cast(u32x4, h); al[gate][s] = ah[gate][s];
            } else {
                h8 h, l;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float w = wh[(size_t)(32 * s + 8 * q + j) * G3 + gate * GH + 16 * ft + m] * GRU_WS;
                    out_of_range |= !(fabsf(w) <= F16_MAX);            // |W_h| >= 1 023.5 (or NaN): outside the split's range; |h| < 1 needs no check
                    h[j] = (_Float16)w; l[j] = (_Float16)(w - (float)h[j]);
                }
                ah[gate][s] = __builtin_bit_cast(u32x4, h); al[gate][s] = __builtin_bit_cast(u32x4, l);
            }
        }
    if (out_of_range && err) atomicOr(err, ERR_F16_RANGE);
    f32x4 bias[3];
#pragma unroll
    for (int gate = 0; gate < 3; ++gate) bias[gate] = *reinterpret_cast<const f32x4*>(bh + gate * GH + 16 * ft + 4 * q);
    const int fo = 16 * ft + 4 * q;                                   // this lane's 4 features
#if GRU_H0
    f32x4 hown = *reinterpret_cast<const f32x4*>(gru_h0_base(h0, g) + (size_t)rc * h0.row_stride + fo);   // the given state, in front of the prefetch
#else
    f32x4 hown = {0.f, 0.f, 0.f, 0.f};                                // h_{t-1}[row m][fo .. fo + 3]
#endif
    u32x4 xh[2] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}}, xl[2] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};   // B operand: h_0 = 0
    // The step's input-side projections are requested PF steps ahead; the compute waves issue no stores, so a counted wait for a
    // prefetched projection waits for nothing younger.
    constexpr int PF = 4;
    f32x4 gbuf[PF][3];
    const float* gbase = gru_part_base(gi, g) + (size_t)rc * G3 + fo;
    auto load_gi = [&](int t, f32x4 (&d)[3]) {
        const float* gir = gbase + (size_t)t * gi.t_stride;
        d[0] = *reinterpret_cast<const f32x4*>(gir); d[1] = *reinterpret_cast<const f32x4*>(gir + GH); d[2] = *reinterpret_cast<const f32x4*>(gir + 2 * GH);
    };
#pragma unroll
    for (int d = 0; d < PF; ++d)
        if (GRU_T1 + d < T) load_gi(GRU_T1 + d, gbuf[d]);
    auto step = [&](int t, f32x4 (&gb)[3]) {
        const f32x4 gr = gb[0], gz = gb[1], gn = gb[2];
        if (t + PF < T) load_gi(t + PF, gb);
        f32x4 acc[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        if (GRU_H0 || t > 0) {                                         // small terms first; the three gates' chains interleave
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                if constexpr (BF) {
#pragma unroll
                    for (int gate = 0; gate < 3; ++gate) acc[gate] = mmab(ah[gate][s], xh[s], acc[gate]);
                } else {
#pragma unroll
                    for (int gate = 0; gate < 3; ++gate) acc[gate] = mma16(al[gate][s], xh[s], acc[gate]);
#pragma unroll
                    for (int gate = 0; gate < 3; ++gate) acc[gate] = mma16(ah[gate][s], xl[s], acc[gate]);
#pragma unroll
                    for (int gate = 0; gate < 3; ++gate) acc[gate] = mma16(ah[gate][s], xh[s], acc[gate]);
                }
            }
        }
        f32x4 hn, rg, zg, ng, an;
        constexpr float INVS = BF ? 1.f : GRU_INV;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            rg[r] = sigm_fast(gr[r] + fmaf(acc[0][r], INVS, bias[0][r]));
            zg[r] = sigm_fast(gz[r] + fmaf(acc[1][r], INVS, bias[1][r]));
            an[r] = fmaf(acc[2][r], INVS, bias[2][r]);                 // gh_n
            ng[r] = tanh_fast_(gn[r] + rg[r] * an[r]);
            hn[r] = (1.f - zg[r]) * ng[r] + zg[r] * hown[r];
        }
        hown = hn;
        if constexpr (BF) {   // this lane's 4 new values as bf16 -> the LDS image the other waves read their B operand from
            b4 h;
#pragma unroll
            for (int r = 0; r < 4; ++r) h[r] = (__bf16)hn[r];
            *reinterpret_cast<u32x2*>(&hx[t & 1][0][m][fo]) = __builtin_bit_cast(u32x2, h);
        } else {   // ... as scaled hi / lo f16 terms
            h4 h, l;
#pragma unroll
            for (int r = 0; r < 4; ++r) { const float x = hn[r] * GRU_XS; h[r] = (_Float16)x; l[r] = (_Float16)(x - (float)h[r]); }
            *reinterpret_cast<u32x2*>(&hx[t & 1][0][m][fo]) = __builtin_bit_cast(u32x2, h);
            *reinterpret_cast<u32x2*>(&hx[t & 1][1][m][fo]) = __builtin_bit_cast(u32x2, l);
        }
        {   // results of the step -> staging image (the writer wave takes them to hs / rzn / ghn)
            float* o = &st[t & 1][m][fo];
            *reinterpret_cast<f32x4*>(o) = hn;
            if constexpr (TRAIN) {
                *reinterpret_cast<f32x4*>(o + GH) = rg; *reinterpret_cast<f32x4*>(o + 2 * GH) = zg; *reinterpret_cast<f32x4*>(o + 3 * GH) = ng;
                *reinterpret_cast<f32x4*>(o + 4 * GH) = an;
            }
        }
        lds_barrier();
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            xh[s] = *reinterpret_cast<const u32x4*>(&hx[t & 1][0][m][32 * s + 8 * q]);
            if constexpr (!BF) xl[s] = *reinterpret_cast<const u32x4*>(&hx[t & 1][1][m][32 * s + 8 * q]);
        }
    };
#if GRU_H0
    {   // step 0: the given state through the paths of any step's result (operand image, staging image, barrier)
        if constexpr (BF) {
            b4 h;
#pragma unroll
            for (int r = 0; r < 4; ++r) h[r] = (__bf16)hown[r];
            *reinterpret_cast<u32x2*>(&hx[0][0][m][fo]) = __builtin_bit_cast(u32x2, h);
        } else {
            h4 h, l;
#pragma unroll
            for (int r = 0; r < 4; ++r) { const float x = hown[r] * GRU_XS; h[r] = (_Float16)x; l[r] = (_Float16)(x - (float)h[r]); }
            *reinterpret_cast<u32x2*>(&hx[0][0][m][fo]) = __builtin_bit_cast(u32x2, h);
            *reinterpret_cast<u32x2*>(&hx[0][1][m][fo]) = __builtin_bit_cast(u32x2, l);
        }
        float* o = &st[0][m][fo];
        *reinterpret_cast<f32x4*>(o) = hown;
        if constexpr (TRAIN) {
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            *reinterpret_cast<f32x4*>(o + GH) = z; *reinterpret_cast<f32x4*>(o + 2 * GH) = z; *reinterpret_cast<f32x4*>(o + 3 * GH) = z;
            *reinterpret_cast<f32x4*>(o + 4 * GH) = z;
        }
        lds_barrier();
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            xh[s] = *reinterpret_cast<const u32x4*>(&hx[0][0][m][32 * s + 8 * q]);
            if constexpr (!BF) xl[s] = *reinterpret_cast<const u32x4*>(&hx[0][1][m][32 * s + 8 * q]);
        }
    }
#endif
    int t0 = GRU_T1;
    for (; t0 + PF <= T; t0 += PF) {                                   // whole groups: the PF register sets rotate by unrolling
#pragma unroll
        for (int d = 0; d < PF; ++d) step(t0 + d, gbuf[d]);
    }
#pragma unroll
    for (int d = 0; d < PF; ++d)
        if (t0 + d < T) step(t0 + d, gbuf[d]);
}

#if !GRU_H0
// dhs [G, T, B, 64] (dL/d hs), hs, rzn, ghn, wh as above -> d_gi [T, G, B, 192], dgh [G, T, B, 192] (dL/dgh_t, the B operand of the
// weight gradient), d_bh_part [G, tiles, 192].  The recurrence carries dL/dh only: dL/dh_{t-1} = direct + dL/dgh_t W_h^T.  Gradients
// span too many decades for fixed-scale f16 splits, and gfx950's f32 MFMA runs at the VALU rate (48 of them per step were the
// kernel's critical path), so the product is evaluated on v_mfma_f32_16x16x32_bf16 from THREE-term bf16 splits x = b1 + b2 + b3
// (bf16 has f32's exponent range; 3 x 8 significand bits) keeping the six partial products of order <= 2^-16: f32-equivalent,
// 36 MFMAs of 16 cycles per step.  dL/dW_h = sum_t h_{t-1}^T dL/dgh_t does not feed the recurrence: it is one product per weight
// set over all (t, row) pairs, computed afterwards (launch_gru_seq_bwd) instead of inside this kernel's 100-step latency chain.
constexpr int DSB = 200;               // LDS row stride of the bf16 dL/dgh image (halves): 400 B = 16 * odd (mod 256)
__device__ __forceinline__ void split3(float x, __bf16& t1, __bf16& t2, __bf16& t3) {
    t1 = (__bf16)x; const float r1 = x - (float)t1;                   // both subtractions are exact
    t2 = (__bf16)r1; const float r2 = r1 - (float)t2;
    t3 = (__bf16)r2;
}

constexpr int BST = 260;            // staging row stride (floats): [d_r 64 | d_z 64 | d_n 64 | d_hn 64] + pad, 1040 B = 16 * 65
constexpr int GRU_BWD_LDS = 2 * 3 * 16 * DSB * 2 + 2 * 16 * BST * 4;   // bf16 operand image + f32 staging image: 71 680 B (dynamic)
// BF: single bf16 terms (learner_dtype: bf16): 6 MFMAs per step instead of 36.
#endif
template <bool BF>
__global__ __launch_bounds__(GRU_THREADS) void GRU_BWD_KERNEL(const GruParts dhs, const float* __restrict__ hs, const float* __restrict__ rzn,
                                                             const float* __restrict__ ghn, const GruW W, const GruParts d_gi,
                                                             float* __restrict__ dgh, float* __restrict__ d_bh_part, int T, int G, int B, int tiles) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gru_lds[];
    __bf16 (*dgb)[3][16][DSB] = reinterpret_cast<__bf16 (*)[3][16][DSB]>(gru_lds);                    // dL/dgh of the step: [buffer][term][row][192]
    float (*st)[16][BST] = reinterpret_cast<float (*)[16][BST]>(gru_lds + 2 * 3 * 16 * DSB * 2);         // [buffer][row][staged results of the step]
    const int tid = threadIdx.x, lane = tid & 63, ft = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = blockIdx.x / tiles, tile = blockIdx.x - g * tiles;
    if (ft == GRU_COMPUTE_WAVES) {                                     // the writer wave (see k_gru_seq_fwd)
        float* dgi_t = gru_part_base(d_gi, g) + (size_t)tile * 16 * G3 + 4 * lane;        // + t * t_stride
        float* dgh_t = dgh + (((size_t)g * T) * B + tile * 16) * G3 + 4 * lane;           // + t * B * G3
        for (int t = T - 1; t >= 0; --t) {
            lds_barrier();
            const float* im = &st[t & 1][0][0];
            f32x4 vg[12], vh[12];
#pragma unroll
            for (int i = 0; i < 12; ++i) {
                int r, c; piece_rc<G3>(i, lane, r, c);
                vg[i] = *reinterpret_cast<const f32x4*>(im + r * BST + c);                              // d_r | d_z | d_n
                vh[i] = *reinterpret_cast<const f32x4*>(im + r * BST + c + (c >= 2 * GH ? GH : 0));     // d_r | d_z | d_hn
            }
#pragma unroll
            for (int i = 0; i < 12; ++i) *reinterpret_cast<f32x4*>(dgi_t + (size_t)t * d_gi.t_stride + 256 * i) = vg[i];
#pragma unroll
            for (int i = 0; i < 12; ++i) *reinterpret_cast<f32x4*>(dgh_t + (size_t)t * B * G3 + 256 * i) = vh[i];
        }
        return;
    }
    const int m = lane & 15, q = lane >> 4;
    const int row = tile * 16 + m, rc = row;                          // B is a multiple of 16 (the host pads): see k_gru_seq_fwd
    const int fo = 16 * ft + 4 * q;
    const float* __restrict__ wh = gru_wh(W, g);
    // resident A fragments of W_h: lane (q, m) = hidden feature 16 ft + m, reduction indices (gate outputs) k = 32 s + 8 q + j
    u32x4 wa[6][3];
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        b8 t1, t2, t3;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            __bf16 x1, x2, x3;
            split3(wh[(size_t)(16 * ft + m) * G3 + 32 * s + 8 * q + j], x1, x2, x3);
            t1[j] = x1; t2[j] = x2; t3[j] = x3;
        }
        wa[s][0] = __builtin_bit_cast(u32x4, t1); wa[s][1] = __builtin_bit_cast(u32x4, t2); wa[s][2] = __builtin_bit_cast(u32x4, t3);
    }
    f32x4 dbh[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    f32x4 carry = {0.f, 0.f, 0.f, 0.f};                                // dL/dh_t arriving from step t + 1
    // everything a step reads from global memory is requested PF steps ahead; the compute waves issue no stores (see k_gru_seq_fwd)
    constexpr int PF = 2;                                              // 2 steps ~ 2 us ahead; 4 would need 48 more registers than the 256 a wave has when 5 waves share 4 SIMDs
    struct StepIn { f32x4 dout, rg, zg, ng, gn, hprev; };
    const float* dbase = gru_part_base(dhs, g) + (size_t)rc * GH + fo;      // dL/dhs of this set: parts [sets, T, B, 64], + t * t_stride
    auto load_step = [&](int t, StepIn& in) {
        const size_t tr = ((size_t)t * G + g) * B + rc;
        in.dout = *reinterpret_cast<const f32x4*>(dbase + (size_t)t * dhs.t_stride);
        const float* s = rzn + tr * G3 + fo;
        in.rg = *reinterpret_cast<const f32x4*>(s); in.zg = *reinterpret_cast<const f32x4*>(s + GH); in.ng = *reinterpret_cast<const f32x4*>(s + 2 * GH);
        in.gn = *reinterpret_cast<const f32x4*>(ghn + tr * GH + fo);
        in.hprev = f32x4{0.f, 0.f, 0.f, 0.f};
        if (t > 0) in.hprev = *reinterpret_cast<const f32x4*>(hs + (((size_t)g * T + (t - 1)) * B + rc) * GH + fo);
    };
    StepIn buf[PF];
#pragma unroll
    for (int d = 0; d < PF; ++d)
        if (T - 1 - d >= GRU_T1) load_step(T - 1 - d, buf[d]);
    auto step = [&](int t, StepIn& in) {
        const int pb = t & 1;
        const f32x4 dout = in.dout, rg = in.rg, zg = in.zg, ng = in.ng, gn = in.gn, hprev = in.hprev;
        if (t - PF >= GRU_T1) load_step(t - PF, in);
        f32x4 d_r, d_z, d_n, d_hn, direct;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float dh = dout[r] + carry[r];
            d_n[r] = dh * (1.f - zg[r]) * (1.f - ng[r] * ng[r]);       // through tanh
            d_z[r] = dh * (hprev[r] - ng[r]) * zg[r] * (1.f - zg[r]);  // through sigmoid
            d_r[r] = d_n[r] * gn[r] * rg[r] * (1.f - rg[r]);
            d_hn[r] = d_n[r] * rg[r];                                  // dL/dgh_n
            direct[r] = dh * zg[r];
        }
        {   // this lane's 12 values as three bf16 terms (BF: one) -> the LDS image the other waves read their B operand from
            const f32x4 v[3] = {d_r, d_z, d_hn};
#pragma unroll
            for (int gate = 0; gate < 3; ++gate) {
                b4 t1, t2, t3;
#pragma unroll
                for (int r = 0; r < 4; ++r) { __bf16 x1, x2, x3; split3(v[gate][r], x1, x2, x3); t1[r] = x1; t2[r] = x2; t3[r] = x3; }
                *reinterpret_cast<u32x2*>(&dgb[pb][0][m][gate * GH + fo]) = __builtin_bit_cast(u32x2, t1);
                if constexpr (!BF) {
                    *reinterpret_cast<u32x2*>(&dgb[pb][1][m][gate * GH + fo]) = __builtin_bit_cast(u32x2, t2);
                    *reinterpret_cast<u32x2*>(&dgb[pb][2][m][gate * GH + fo]) = __builtin_bit_cast(u32x2, t3);
                }
            }
        }
        {   // the step's results -> staging image (the writer wave takes them to d_gi and dgh)
            float* o = &st[pb][m][fo];
            *reinterpret_cast<f32x4*>(o) = d_r; *reinterpret_cast<f32x4*>(o + GH) = d_z; *reinterpret_cast<f32x4*>(o + 2 * GH) = d_n;
            *reinterpret_cast<f32x4*>(o + 3 * GH) = d_hn;
        }
        dbh[0] += d_r; dbh[1] += d_z; dbh[2] += d_hn;
        lds_barrier();
        // dL/dh_{t-1}, matrix part: D[feature 16 ft + 4 q + reg][row m] = sum_k W_h[feature][k] dL/dgh[row][k]; partial products by
        // order of magnitude into three accumulators (smallest first when they are added)
        f32x4 a3 = {0.f, 0.f, 0.f, 0.f}, a2 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 6; ++s) {
            u32x4 bt[3];
#pragma unroll
            for (int term = 0; term < (BF ? 1 : 3); ++term) bt[term] = *reinterpret_cast<const u32x4*>(&dgb[pb][term][m][32 * s + 8 * q]);
            if constexpr (BF) {
                a1 = mmab(wa[s][0], bt[0], a1);
            } else {
                a3 = mmab(wa[s][0], bt[2], a3); a2 = mmab(wa[s][0], bt[1], a2); a1 = mmab(wa[s][0], bt[0], a1);
                a3 = mmab(wa[s][2], bt[0], a3); a2 = mmab(wa[s][1], bt[0], a2);
                a3 = mmab(wa[s][1], bt[1], a3);
            }
        }
        carry = direct + ((a3 + a2) + a1);
        // the next step writes the other LDS buffer; the one after next is ordered behind the next barrier
    };
    int t0 = T - 1;
    for (; t0 - (PF - 1) >= GRU_T1; t0 -= PF) {                           // whole groups: the PF register sets rotate by unrolling
#pragma unroll
        for (int d = 0; d < PF; ++d) step(t0 - d, buf[d]);
    }
#pragma unroll
    for (int d = 0; d < PF; ++d)
        if (t0 - d >= GRU_T1) step(t0 - d, buf[d]);
#if GRU_H0
    {   // step 0: zeros for the writer wave, and its last barrier
        float* o = &st[0][m][fo];
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        *reinterpret_cast<f32x4*>(o) = z; *reinterpret_cast<f32x4*>(o + GH) = z; *reinterpret_cast<f32x4*>(o + 2 * GH) = z;
        *reinterpret_cast<f32x4*>(o + 3 * GH) = z;
        lds_barrier();
    }
#endif
    // dL/db_h: column sums over the tile's rows (the 16 lanes that share q)
#pragma unroll
    for (int gate = 0; gate < 3; ++gate)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float v = dbh[gate][r];
#pragma unroll
            for (int sh = 8; sh >= 1; sh >>= 1) v += __shfl_xor(v, sh);
            if (m == 0) d_bh_part[((size_t)g * tiles + tile) * G3 + gate * GH + fo + r] = v;
        }
}
#undef GRU_FWD_KERNEL
#undef GRU_BWD_KERNEL
#undef GRU_H0_PARAM
#undef GRU_T1
