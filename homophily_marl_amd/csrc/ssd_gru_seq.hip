// ssd_gru_seq.hip -- the learner's recurrence as ONE forward and ONE backward launch over all T timesteps.
//
// Reference: HomophilyLearner.train evaluates the controller for t = 0..T-1 from a zero hidden state (homophily_learner.py:68-91),
// each step running the hand-written GRU cell of HomophilyAgent (homophily_agent.py:162-165,188-191):
//     r = s(gi_r + gh_r), z = s(gi_z + gh_z), n = tanh(gi_n + r * gh_n), h' = (1 - z) n + z h,   gh = h W_h + b_h
// The input-side projections gi = x W_i + b_i do not depend on the recurrence and are computed for all T at once by the caller
// (one batched GEMM); what is left per step is a [B, 64] x [64, 192] product and the gate arithmetic -- at the learner's batch
// (B = 16 episodes) a latency chain of ~10 tiny launches per step and direction.  Here one workgroup owns one (weight set g,
// 16-row tile) and walks the whole sequence:
//   * 4 compute waves (+ a writer wave that takes each step's results from an LDS staging image to HBM, so that no compute wave
//     ever waits for a store); wave w owns hidden features 16 w .. 16 w + 15 (all three gates); its slice of W_h lives in registers for all T as
//     MFMA A operands, products are computed in the transposed form of ssd_policy_mfma.hip (activation row on the lane, 4
//     consecutive features in the lane's registers), so the gate arithmetic is lane-local;
//   * forward: v_mfma_f32_16x16x32_f16 on two-term f16 splits (f32-equivalent; |h| < 1), the new state crosses the waves through a
//     double-buffered LDS image of the split terms: one barrier per step;
//   * backward walks t = T-1 .. 0 with the carried dL/dh in registers (exact f32 MFMAs); dL/dW_h is one product over all
//     (t, row) pairs computed after the walk (the x^T g role of csrc/ssd_bmm.hip).
// H = 64 is fixed.  Rows are independent sequences: any B (tiles of 16, the last one masked).
#include "ssd_policy_common.h"

namespace ssd {

using f32x4 = __attribute__((ext_vector_type(4))) float;
using u32x4 = __attribute__((ext_vector_type(4))) uint32_t;
using u32x2 = __attribute__((ext_vector_type(2))) uint32_t;
using h8 = __attribute__((ext_vector_type(8))) _Float16;
using h4 = __attribute__((ext_vector_type(4))) _Float16;

constexpr int GH = 64, G3 = 192;                        // hidden, 3 * hidden
constexpr int HSH = 72;                                  // LDS row stride of the f16 state image (halves): 144 B = 16 * odd -> conflict-free b128 reads
// forward: f32-equivalent products on the f16 matrix cores from two-term splits (ssd_policy_mfma.hip); exact power-of-two scales
// keep the low terms in f16's normal range (|h| < 1, |W_h| ~ 0.1)
constexpr float GRU_WS = 64.f, GRU_XS = 16.f, GRU_INV = 1.f / (GRU_WS * GRU_XS);

__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }   // backward-side helpers keep libm accuracy
// sigmoid / tanh on v_exp_f32 + v_rcp_f32 (1 ulp each), as the rollout heads
__device__ __forceinline__ float sigm_fast(float x) { return __builtin_amdgcn_rcpf(1.f + __expf(-x)); }
__device__ __forceinline__ float tanh_fast_(float x) {
    const float ax = fminf(fabsf(x), 15.f);
    const float t = 1.f - 2.f * __builtin_amdgcn_rcpf(__expf(2.f * ax) + 1.f);
    return copysignf(t, x);
}
// The workgroup barrier of a recurrence step orders LDS traffic only: wait for this wave's LDS operations and join.
__device__ __forceinline__ void lds_barrier() {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#endif
}
// Results leave through a WRITER wave.  gfx950 retires a wave's loads and stores through one in-order counter: a compute wave that
// stores its step's results waits, at its next counted wait for a prefetched input, for those stores to be acknowledged by memory as
// well (measured: 5 result stores per step cost the forward walk 33 us of 90, the backward walk 56 us of 165).  So the compute waves
// put a step's results into an LDS staging image next to the state image (same barrier), and wave 4 -- which never waits for
// memory -- copies the image of step t to HBM in 1 KiB pieces while the compute waves are in step t + 1.  Rows of the staging image
// are padded to 16 * odd bytes (mod 256): b128 accesses of 16 lanes with different rows fall on different banks.
constexpr int GRU_COMPUTE_WAVES = 4, GRU_THREADS = (GRU_COMPUTE_WAVES + 1) * 64;
// piece i (1 KiB) of a [16, ROWF] f32 tile, lane l: the lane's 16 bytes lie in row (1024 i + 16 l) / (4 ROWF) at byte column (..) % (4 ROWF)
template <int ROWF>
__device__ __forceinline__ void piece_rc(int i, int lane, int& row, int& colf) {
    const int off = 1024 * i + 16 * lane;
    row = off / (4 * ROWF); colf = (off - row * 4 * ROWF) >> 2;
}
__device__ __forceinline__ f32x4 mma16(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, a), __builtin_bit_cast(h8, b), c, 0, 0, 0);
}
using b8 = __attribute__((ext_vector_type(8))) __bf16;
using b4 = __attribute__((ext_vector_type(4))) __bf16;
__device__ __forceinline__ f32x4 mmab(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(b8, a), __builtin_bit_cast(b8, b), c, 0, 0, 0);
}

// gi [T, G, B, 192], wh [G, 64, 192], bh [G, 192] -> hs [G, T, B, 64]; optional (training) rzn [T, G, B, 192], ghn [T, G, B, 64]
// One workgroup per (weight set g, 16-row tile), 4 compute waves + the writer; wave ft owns hidden features 16 ft .. 16 ft + 15 of the three gates.
// Per step: gh^T = W_h^T h^T as 18 v_mfma_f32_16x16x32_f16 (3 gates x 2 K-steps x 3 split products; the W_h slice stays in
// registers as hi / lo fragments for all T), lane-local gate arithmetic, and the new state goes to the other waves through a
// double-buffered LDS image that already holds the hi / lo f16 terms (one barrier per step; each lane splits only its own 4 values).
// B is a multiple of 16 (the host pads): no row predicate and no branch inside the steps, so that the compiler's vmcnt accounting
// stays exact.
// Where the input-side projections (forward) / their gradients (backward) live: up to 4 separately allocated parts of G / n_parts
// weight sets each.  Time-major [T, G, B, 192] (one part) is t_stride = G B 192, set_stride = B 192; the per-agent affine layers'
// own output [sets, T, B, 192] (set-major) is set_stride = T B 192, t_stride = B 192 -- the learner hands its four projection outputs
// (live / target net x env / inc head) over as they are, without concatenating or transposing 12-25 MB copies.
struct GruParts {
    float* p[4];
    int spp;                       // weight sets per part
    long set_stride, t_stride;     // elements
};
__device__ __forceinline__ float* gru_part_base(const GruParts& P, int g) {
    const int part = g / P.spp;
    float* b = part == 0 ? P.p[0] : (part == 1 ? P.p[1] : (part == 2 ? P.p[2] : P.p[3]));
    return b + (size_t)(g - part * P.spp) * P.set_stride;
}

// The recurrence weights as up to 4 separately allocated parts of G / n_parts weight sets each (wh [sets, 64, 192], bh [sets, 192]): the
// learner hands over the live net's and the target net's images as they are (no concatenation per step).
struct GruW {
    const float* wh[4];
    const float* bh[4];
    int spp;                       // weight sets per part
};
__device__ __forceinline__ const float* gru_wh(const GruW& W, int g) {
    const int part = g / W.spp;
    const float* b = part == 0 ? W.wh[0] : (part == 1 ? W.wh[1] : (part == 2 ? W.wh[2] : W.wh[3]));
    return b + (size_t)(g - part * W.spp) * GH * G3;
}
__device__ __forceinline__ const float* gru_bh(const GruW& W, int g) {
    const int part = g / W.spp;
    const float* b = part == 0 ? W.bh[0] : (part == 1 ? W.bh[1] : (part == 2 ? W.bh[2] : W.bh[3]));
    return b + (size_t)(g - part * W.spp) * G3;
}

// A GIVEN state instead of zero (train_stored_state: the rollout's stored recurrent state): step 0 is not computed, hs[0] := h0.  One
// pointer per projection part, so that the learner hands over batch["hidden"][:, 0] as it lies in the static batch:
// h0 of (set g, row) = p[g / spp] + (g % spp) * set_stride + row * row_stride, 64 floats.
struct GruH0 {
    const float* p[4];
    int spp;                       // weight sets per part
    long set_stride, row_stride;   // elements
};
__device__ __forceinline__ const float* gru_h0_base(const GruH0& P, int g) {
    const int part = g / P.spp;
    const float* b = part == 0 ? P.p[0] : (part == 1 ? P.p[1] : (part == 2 ? P.p[2] : P.p[3]));
    return b + (size_t)(g - part * P.spp) * P.set_stride;
}

// The two kernels, compiled twice from ONE text: from a zero state (k_gru_seq_fwd / k_gru_seq_bwd) and from a given state
// (k_gru_seq_fwd_h0 / k_gru_seq_bwd_h0).  The preprocessor, not a template parameter, selects the form: the zero-state kernels keep
// their names, signatures and instruction streams.
#define GRU_H0 0
#include "ssd_gru_seq_kernels.h"
#undef GRU_H0
#define GRU_H0 1
#include "ssd_gru_seq_kernels.h"
#undef GRU_H0

static GruParts gru_parts(float* const* parts, int n_parts, int T, int G, int B) {
    GruParts P;
    for (int k = 0; k < 4; ++k) P.p[k] = parts[k < n_parts ? k : 0];
    if (n_parts <= 0) {            // one time-major tensor [T, G, B, 192]
        P.spp = G; P.set_stride = (long)B * G3; P.t_stride = (long)G * B * G3;
    } else {                       // n_parts set-major tensors [G / n_parts, T, B, 192]
        P.spp = G / n_parts; P.set_stride = (long)T * B * G3; P.t_stride = (long)B * G3;
    }
    return P;
}

// n_parts 0: gi_parts[0] is one time-major tensor; else set-major parts (see GruParts)
static GruW gru_w(const float* const* wh_parts, const float* const* bh_parts, int n_wparts, int G) {
    GruW W;
    const int np = n_wparts < 1 ? 1 : n_wparts;
    for (int k = 0; k < 4; ++k) { W.wh[k] = wh_parts[k < np ? k : 0]; W.bh[k] = bh_parts ? bh_parts[k < np ? k : 0] : nullptr; }
    W.spp = G / np;
    return W;
}
// h0_parts (or null: from zero): one pointer per gi part (n_parts 0: one), see GruH0
void launch_gru_seq_fwd(const float* const* gi_parts, int n_parts, const float* const* wh_parts, const float* const* bh_parts, int n_wparts, float* hs,
                        float* rzn, float* ghn, int T, int G, int B, hipStream_t s, const float* const* h0_parts, long h0_set_stride, long h0_row_stride) {
    const int tiles = (B + 15) / 16;
    const GruW W = gru_w(wh_parts, bh_parts, n_wparts, G);
    const GruParts P = gru_parts(const_cast<float* const*>(reinterpret_cast<const float* const*>(gi_parts)), n_parts, T, G, B);
    int32_t* err = numeric_err_word();
    const bool bf = learner_precision() == 1;
    if (h0_parts) {
        GruH0 H;
        const int np = n_parts < 1 ? 1 : n_parts;
        for (int k = 0; k < 4; ++k) H.p[k] = h0_parts[k < np ? k : 0];
        H.spp = G / np; H.set_stride = h0_set_stride; H.row_stride = h0_row_stride;
#define SSD_GF0(TR_, BF_) hipLaunchKernelGGL((k_gru_seq_fwd_h0<TR_, BF_>), dim3(G * tiles), dim3(GRU_THREADS), 0, s, P, W, H, hs, rzn, ghn, T, G, B, tiles, err)
        if (rzn) { if (bf) SSD_GF0(true, true); else SSD_GF0(true, false); }
        else { if (bf) SSD_GF0(false, true); else SSD_GF0(false, false); }
#undef SSD_GF0
        return;
    }
#define SSD_GF(TR_, BF_) hipLaunchKernelGGL((k_gru_seq_fwd<TR_, BF_>), dim3(G * tiles), dim3(GRU_THREADS), 0, s, P, W, hs, rzn, ghn, T, G, B, tiles, err)
    if (rzn) { if (bf) SSD_GF(true, true); else SSD_GF(true, false); }
    else { if (bf) SSD_GF(false, true); else SSD_GF(false, false); }
#undef SSD_GF
}
// Gn <= G: only the first Gn weight sets are walked (the sets whose outputs carry a gradient: the live net's; the target net's follow);
// rzn / ghn keep their [T, G, B, .] strides, dgh / d_wh / d_bh_part are [Gn, ...].  dhs_parts: n_parts (or one, n_parts 0) tensors
// [sets, T, B, 64]; parts past Gn are not read.
void launch_gru_seq_bwd(const float* const* dhs_parts, const float* hs, const float* rzn, const float* ghn, const float* const* wh_parts, int n_wparts,
                        float* const* d_gi_parts, int n_parts, float* dgh, float* d_wh, float* d_bh_part, int T, int G, int Gn, int B, hipStream_t s, bool h0) {
    const int tiles = (B + 15) / 16;
    const GruW W = gru_w(wh_parts, nullptr, n_wparts, G);
    GruParts D;
    {
        const int np = n_parts < 1 ? 1 : n_parts;
        for (int k = 0; k < 4; ++k) D.p[k] = const_cast<float*>(dhs_parts[(k < np && k * (G / np) < Gn) ? k : 0]);
        D.spp = G / np; D.set_stride = (long)T * B * GH; D.t_stride = (long)B * GH;
    }
    const GruParts P = gru_parts(d_gi_parts, n_parts, T, G, B);
    static bool attr_done_dev[64] = {};                                // the attribute is per device
    int dev = 0;
    if (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64 && !attr_done_dev[dev]) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gru_seq_bwd<false>), hipFuncAttributeMaxDynamicSharedMemorySize, GRU_BWD_LDS);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gru_seq_bwd<true>), hipFuncAttributeMaxDynamicSharedMemorySize, GRU_BWD_LDS);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gru_seq_bwd_h0<false>), hipFuncAttributeMaxDynamicSharedMemorySize, GRU_BWD_LDS);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gru_seq_bwd_h0<true>), hipFuncAttributeMaxDynamicSharedMemorySize, GRU_BWD_LDS);
        attr_done_dev[dev] = true;                                     // a refused attribute shows as a launch error (ssd_poll_error / hipGetLastError)
    }
    if (h0) {
        if (learner_precision() == 1) hipLaunchKernelGGL(k_gru_seq_bwd_h0<true>, dim3(Gn * tiles), dim3(GRU_THREADS), GRU_BWD_LDS, s, D, hs, rzn, ghn, W, P, dgh, d_bh_part, T, G, B, tiles);
        else hipLaunchKernelGGL(k_gru_seq_bwd_h0<false>, dim3(Gn * tiles), dim3(GRU_THREADS), GRU_BWD_LDS, s, D, hs, rzn, ghn, W, P, dgh, d_bh_part, T, G, B, tiles);
    } else if (learner_precision() == 1) hipLaunchKernelGGL(k_gru_seq_bwd<true>, dim3(Gn * tiles), dim3(GRU_THREADS), GRU_BWD_LDS, s, D, hs, rzn, ghn, W, P, dgh, d_bh_part, T, G, B, tiles);
    else hipLaunchKernelGGL(k_gru_seq_bwd<false>, dim3(Gn * tiles), dim3(GRU_THREADS), GRU_BWD_LDS, s, D, hs, rzn, ghn, W, P, dgh, d_bh_part, T, G, B, tiles);
    // dL/dW_h[g] = sum_{t >= 1, b} h_{t-1}[b]^T dL/dgh_t[b]: rows (t, b) of hs [G, T, B, 64] against rows (t + 1, b) of dgh [G, T, B, 192] --
    // the x^T g role of the per-agent-layer kernel (csrc/ssd_bmm.hip: K = (T - 1) B rows split over 16 waves per tile, exact f32)
    if (T > 1) launch_bias_bmm_bwd(dgh + (size_t)B * G3, hs, nullptr, nullptr, d_wh, nullptr, nullptr, Gn, (T - 1) * B, GH, G3, s, (long)T * B * GH, (long)T * B * G3);
    else (void)hipMemsetAsync(d_wh, 0, (size_t)Gn * GH * G3 * sizeof(float), s);
}

}  // namespace ssd
