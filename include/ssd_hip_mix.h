/* ssd_hip_mix.h -- the entry point of libssd_hip.so for the value-decomposition mixer of the env head (config key mixer: "vdn"): the
 * team's TD error formed from the agents' errors behind the loss launch.  A companion of ssd_hip.h (ssd_td_loss_args, status codes,
 * ssd_last_error, the ABI version, SSD_MAX_AGENTS, SSD_ROWS32_MAX, SSD_TD_LOSS_PARTIALS: all there); mirrored by
 * homophily_marl_amd/abi.py: MIX_SIGNATURES.  The function returns an ssd_status.
 *
 * ssd_team_td(args, stream)
 *   args: the struct the caller has just handed to ssd_td_sim_loss(args, 1, stream) -- the same operands, no member more.  That launch
 *   must have run ON THE SAME STREAM in front of this one: it wrote dq_env (every element, the zeros of the rows included), dq_inc and
 *   the partials' columns, and this launch rewrites a part of them in place.
 *
 *   With T = t_slots - 1 and, per (b, t < T, agent i), mask, live, r_env,i, chosen_i and tmax_i exactly the expressions of the loss
 *   launch's one-step kernel in its f32 operation order (ssd_hip.h: ssd_td_sim_loss; r_env,i reads args->reward, whichever storage
 *   field the caller pointed it at):
 *       td_i    = chosen_i - (r_env,i + gamma_env live tmax_i)                         td_lambda == 0: the loss launch's td_env, the same bits
 *       td_i    = partials[row_i][5] - partials[row_i][13]                            td_lambda > 0: chosen_env - G_env, as the loss launch
 *                                                                                     formed them (this launch DEPENDS on those two columns)
 *       td_team = fl(...fl(fl(td_0 + td_1) + td_2)... + td_{n-1})                      f32, ascending i, one rounding per add
 *       dq_env[b][t][i][a_i]  = fl(fl(fl(fl(fl(2 td_team) mask) mask) / dens[0]) n)   for every i; the other n_actions - 1 entries of the
 *                                                                                     row keep the loss launch's 0
 *       partials[row_i][2]    = fl(fl(td_team mask) fl(td_team mask))                 for every i
 *   so the n rows of one (b, t) hold identical bits, and the sum of column 2 over all rows divided by dens[0] is
 *   n sum_{b,t} (mask td_team)^2 / dens[0]: the loss of PyMARL's QLearner under its VDNMixer (summed chosen values, summed selected
 *   targets, the team reward, one mask entry per (b, t)).  The factor n of the seed is that sum's derivative: each of the n equal rows
 *   depends on q_env[b][t][i][a_i].
 *   Nothing else is written: the bootstrap slot t = T keeps its zero rows, the partials' columns 0, 1 and 3 .. 15 keep their values
 *   (13 stays the PER-AGENT return), dq_inc and every input are untouched.  The inc head has no mixer.
 *   One launch; no atomics, no LDS memory, no scratch memory; built without floating-point contraction like the loss kernel: a run equals
 *   its restatement in plain f32 loops to the bit.  Only 4-byte alignment of the f32 / i32 operands is needed (actions, actions_inc and
 *   filled are read as the loss launch reads them); terminated is a byte array.
 *   SSD_ERR_INVALID, before any launch, each with a message that names ssd_team_td: NULL args; batch < 1, t_slots < 2 or n_actions < 1;
 *   n_agents outside 2 .. SSD_MAX_AGENTS; batch * t_slots * n_agents over SSD_ROWS32_MAX; an operand this launch reads or writes
 *   (q_env, tq_env, actions, actions_inc, avail, reward, terminated, filled, dens, dq_env, partials) that is NULL, or -- terminated
 *   aside -- not 4-byte aligned; seq_len <= 0 or reward_scale == 0; td_lambda below 0, above 1 or NaN. */
#ifndef SSD_HIP_MIX_H
#define SSD_HIP_MIX_H

#include "ssd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int ssd_team_td(const ssd_td_loss_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSD_HIP_MIX_H */
