// ssd_social_reward.hip -- reward models over a finished rollout (include/ssd_hip_reward.h: ssd_social_reward): inequity aversion
// (Hughes et al. 2018) and prosocial (team-mixed) rewards, the standard Cleanup / Harvest baselines on independent learners.
//
// Inequity aversion carries each agent's smoothed reward e_t = d e_{t-1} + r_t from the first slot of the episode, so it cannot be formed
// inside a sampled training window; it is formed once per rollout over the episode storage, raw reward -> shaped reward, and the shaped
// field travels through the replay buffer like every other.  The arithmetic and its order are the contract of the header: f32, one
// rounding per operation (-ffp-contract=off), sums over the partners j in ascending j, skipping the agent itself.
//
// Shape: serial in t, parallel over (env, agent), n <= 10.  One 16-lane group per env, four envs per wave, one wave per workgroup; lane
// a < n of a group owns agent a and keeps e[a] (and its three f64 statistics) in registers.  The partners' values come by __shfl with
// width 16 (a cross-lane move inside the group: no LDS memory, no barrier).  The loads of a chunk of kChunk slots do not depend on the
// recurrence: they are all issued before the chunk's first scan step, so the scan pays one memory trip per chunk, not per slot.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/ssd_hip_reward.h"
#include "ssd_device.h"

namespace ssd {

constexpr int kRewardGroup = 16;                       // lanes per env
constexpr int kRewardEnvsPerWave = 64 / kRewardGroup;  // one wave per workgroup
constexpr int kRewardChunk = 10;                       // slots whose loads are in flight together

// MODEL SSD_REWARD_IA: p0 = a_s, p1 = b_s, p2 = d.  MODEL SSD_REWARD_PROSOCIAL: p0 = c_own, p1 = c_oth.
// T = t_slots - 1 scanned slots; slot T (the bootstrap slot) is written 0.  Lanes a >= n and groups past n_env load and store nothing, but
// take part in the shuffles (every lane of the wave runs the same trip counts: T, n and the chunking are uniform).
template <int MODEL>
__global__ __launch_bounds__(64) void k_social_reward(const float* __restrict__ src, float* __restrict__ dst, double* __restrict__ acc, int n_env, int T, int n,
                                                      int src_env_stride, int src_slot_stride, int dst_env_stride, int dst_slot_stride, float p0, float p1,
                                                      float p2) {
    const int a = threadIdx.x & (kRewardGroup - 1);
    const int env = blockIdx.x * kRewardEnvsPerWave + (threadIdx.x >> 4);
    const bool live = env < n_env && a < n;
    const float* s = src + (live ? (long)env * src_env_stride + a : 0);
    float* o = dst + (live ? (long)env * dst_env_stride + a : 0);
    double* st = acc && live ? acc + ((long)env * n + a) * 3 : nullptr;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    if (st) { s0 = st[0]; s1 = st[1]; s2 = st[2]; }
    float e = 0.0f;
    for (int t0 = 0; t0 < T; t0 += kRewardChunk) {
        float r[kRewardChunk];
#pragma unroll
        for (int c = 0; c < kRewardChunk; ++c) r[c] = live && t0 + c < T ? s[(t0 + c) * src_slot_stride] : 0.0f;
#pragma unroll
        for (int c = 0; c < kRewardChunk; ++c) {
            if (t0 + c >= T) break;                    // uniform
            float u, second, third;
            if (MODEL == SSD_REWARD_IA) {
                e = p2 * e + r[c];
                float envy = 0.0f, guilt = 0.0f;
                for (int j = 0; j < n; ++j) {
                    const float ej = __shfl(e, j, kRewardGroup);
                    if (j != a) {
                        envy += fmaxf(ej - e, 0.0f);
                        guilt += fmaxf(e - ej, 0.0f);
                    }
                }
                second = p0 * envy;
                third = p1 * guilt;
                u = (r[c] - second) - third;
            } else {
                float others = 0.0f;
                for (int j = 0; j < n; ++j) {
                    const float rj = __shfl(r[c], j, kRewardGroup);
                    if (j != a) others += rj;
                }
                second = p1 * others;
                third = 0.0f;
                u = p0 * r[c] + second;
            }
            if (live) o[(t0 + c) * dst_slot_stride] = u;
            s0 += (double)u; s1 += (double)second; s2 += (double)third;
        }
    }
    if (live) o[T * dst_slot_stride] = 0.0f;
    if (st) { st[0] = s0; st[1] = s1; st[2] = s2; }
}

void launch_social_reward(int model, const float* src, float* dst, double* acc, int n_env, int t_slots, int n, int src_env_stride, int src_slot_stride,
                          int dst_env_stride, int dst_slot_stride, float p0, float p1, float p2, hipStream_t s) {
    const dim3 grid((n_env + kRewardEnvsPerWave - 1) / kRewardEnvsPerWave), block(64);
    if (model == SSD_REWARD_IA)
        hipLaunchKernelGGL(k_social_reward<SSD_REWARD_IA>, grid, block, 0, s, src, dst, acc, n_env, t_slots - 1, n, src_env_stride, src_slot_stride,
                           dst_env_stride, dst_slot_stride, p0, p1, p2);
    else
        hipLaunchKernelGGL(k_social_reward<SSD_REWARD_PROSOCIAL>, grid, block, 0, s, src, dst, acc, n_env, t_slots - 1, n, src_env_stride, src_slot_stride,
                           dst_env_stride, dst_slot_stride, p0, p1, p2);
}

}  // namespace ssd
