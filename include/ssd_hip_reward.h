/* ssd_hip_reward.h -- the entry point of libssd_hip.so that shapes a finished rollout's rewards by a reward model: inequity aversion
 * (Hughes et al. 2018) or prosocial (team-mixed) rewards.  A companion of ssd_hip.h (types, status codes, ssd_last_error, the ABI
 * version: all there); mirrored by homophily_marl_amd/abi.py: REWARD_SIGNATURES.  The function returns an ssd_status.
 *
 * Input   reward f32 [n_env, t_slots, n_agents]: the raw env rewards as stored; slot t_slots - 1 is the bootstrap slot (not read).
 * Output  shaped f32, the same logical shape; slot t_slots - 1 is written 0.
 * Element (env, t, i) of either lies at env * env_stride + t * slot_stride + i (strides in elements, slot_stride >= n_agents, env_stride >=
 * t_slots * slot_stride: the rollout storage may be a slab inside a replay buffer); nothing between the logical elements is touched.
 *
 * All arithmetic is f32 with one rounding per operation (fl), no fused multiply-add.  Sums over j run in ascending j, skipping i,
 * accumulated left to right from 0.  n = n_agents; the scalars are computed once by the caller in f32.
 *
 * SSD_REWARD_IA (p0 = a_s = fl(alpha / (n - 1)), p1 = b_s = fl(beta / (n - 1)), p2 = d, the decay of the smoothed reward, in [0, 1)):
 *   e_t[j]  = fl(fl(d * e_{t-1}[j]) + r_t[j]),  e_{-1} = 0
 *   envy_i  = sum_j max(fl(e_t[j] - e_t[i]), 0)
 *   guilt_i = sum_j max(fl(e_t[i] - e_t[j]), 0)
 *   u_t[i]  = fl(fl(r_t[i] - fl(a_s * envy_i)) - fl(b_s * guilt_i))
 *   The scan does not read `terminated`: these envs end at the episode limit, so e runs from slot 0 to slot t_slots - 2 of every env.
 * SSD_REWARD_PROSOCIAL (p0 = c_own = fl(1 - rho), p1 = c_oth = fl(rho / (n - 1)), p2 unused):
 *   u_t[i]  = fl(fl(c_own * r_t[i]) + fl(c_oth * S_i)),  S_i = sum_j r_t[j]
 *
 * acc (nullable) f64 [n_env, n_agents, 3]: the lane that owns (env, agent) adds, in ascending t, one term per slot t < t_slots - 1 to
 *   column 0: u_t[i];  column 1: fl(a_s * envy_i), prosocial fl(c_oth * S_i);  column 2: fl(b_s * guilt_i), prosocial 0.
 * No atomics: a run equals its restatement in plain loops to the bit, statistics included.
 *
 * SSD_ERR_INVALID, before any launch: a NULL reward or shaped; shaped == reward or overlapping extents; a model other than the two;
 * n_env < 1; t_slots < 2; n_agents outside 2 .. SSD_MAX_AGENTS; a slot stride below n_agents; an env stride below t_slots * slot_stride;
 * a negative or non-finite p0 / p1; for SSD_REWARD_IA p2 outside [0, 1) or NaN; an extent past 2^31 - 1 elements; a reward or
 * shaped pointer that is not 4-byte aligned; an acc that is not 8-byte aligned (it is read and written as f64). */
#ifndef SSD_HIP_REWARD_H
#define SSD_HIP_REWARD_H

#include "ssd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SSD_REWARD_IA 1
#define SSD_REWARD_PROSOCIAL 2

int ssd_social_reward(int32_t model, const float* reward, float* shaped, double* acc, int32_t n_env, int32_t t_slots, int32_t n_agents,
                      int32_t src_env_stride, int32_t src_slot_stride, int32_t dst_env_stride, int32_t dst_slot_stride, float p0, float p1, float p2,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSD_HIP_REWARD_H */
