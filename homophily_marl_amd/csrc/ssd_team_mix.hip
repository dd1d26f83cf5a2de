// ssd_team_mix.hip -- the value-decomposition mixer of the env head (include/ssd_hip_mix.h: ssd_team_td; config key mixer: "vdn").
//
// VDN's team value is the plain sum of the agents' values, so the team's TD error is the sum of the agents' TD errors and the loss
// kernels need no second copy: this one launch runs behind the unchanged loss launch on the same operands and rewrites the env head's
// gradient seeds (one element per row) and column 2 of the partials.  The column sums, the logged loss, the priority write-back and
// its importance weights, the clip, Adam, Polyak and the tie of shared heads then read the team's numbers without knowing of a mixer.
//
// The arithmetic and its order are the contract of the header: f32, one rounding per operation (-ffp-contract=off), the agents added
// in ascending order.  With td_lambda == 0 every agent's td is restated with the expressions and the operation order of
// k_td_sim_loss<1> (csrc/ssd_learner.hip), so it carries that kernel's bits; with td_lambda > 0 it is column 5 minus column 13 of the
// row the lambda kernel wrote.
//
// Shape: one 16-lane group per (b, t < T), lane i < n of the group owns agent i (n <= 10), sixteen groups per workgroup.  A lane forms
// its agent's td; every lane then reads the n of them by __shfl with width 16 (a cross-lane move inside the group: no LDS memory, no
// barrier) and adds them in the same ascending order, so the n rows of a (b, t) get the same bits.  Lanes i >= n and groups past the
// last (b, t) load and store nothing but take part in the shuffles (n is uniform).  The launch moves a few hundred bytes per row and
// sits at the launch floor; nothing here is tuned beyond letting the agents' loads run side by side.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/ssd_hip_mix.h"
#include "ssd_device.h"

namespace ssd {

constexpr int kMixGroup = 16;                          // lanes per (b, t)
constexpr int kMixBlock = 256;
constexpr int kMixPairsPerBlock = kMixBlock / kMixGroup;
constexpr float kMixNeg = -9999999.f;                  // the reference's masked_fill value, as in k_td_sim_loss

__global__ __launch_bounds__(kMixBlock) void k_team_td(ssd_td_loss_args a) {
    const int T1 = a.t_slots, T = T1 - 1, n = a.n_agents, A = a.n_actions;
    const int i = threadIdx.x & (kMixGroup - 1);
    const int pair = blockIdx.x * kMixPairsPerBlock + (threadIdx.x >> 4);       // (b, t) over the T loss rows of every episode
    const bool own = pair < a.batch * T && i < n;
    float td = 0.f, mask = 0.f;
    float* seed = nullptr;
    float* out = nullptr;
    if (own) {
        const int b = pair / T, t = pair - b * T, bt = b * T1 + t, it = bt * n + i;
        const size_t row = (size_t)bt * n;                                      // (b, t, agent 0)
        out = a.partials + ((size_t)pair * n + i) * SSD_TD_LOSS_PARTIALS;
        mask = (float)a.filled[bt] * (t ? 1.f - (float)a.terminated[bt - 1] : 1.f);
        const size_t qe = (size_t)it * A, qe1 = qe + (size_t)n * A;             // (b, t, i) and (b, t + 1, i)
        const int a_t = (int)a.actions[row + i];
        seed = a.dq_env + qe + a_t;
        if (a.td_lambda > 0.f) {
            td = out[5] - out[13];                                              // chosen_env - G_env of the lambda kernel
        } else {
            // ---- the one-step td_env of k_td_sim_loss<1>, expression for expression -----------------------------------------------
            const int64_t* ainc = a.actions_inc + row * n;                      // [giver][receiver] at (b, t)
            int rp = 0, rn = 0;
            for (int j = 0; j < n; ++j) {
                if (j == i) continue;
                const int64_t x = ainc[(size_t)j * n + i];
                rp += x == 1; rn += x == 2;
            }
            const float r = a.reward[row + i] / a.reward_scale;
            const float rv = (float)(rp - rn);
            const float r_env = (r + rv * a.incentive_ratio * a.incentive) / a.seq_len;
            const float live = 1.f - (float)a.terminated[bt];
            const float chosen_env = a.q_env[qe + a_t];
            float bq = -INFINITY, tmax_env = kMixNeg;
            for (int k = 0; k < A; ++k) {
                const bool ok = a.avail[qe1 + k] != 0;
                const float q = a.double_q ? (ok ? a.q_env[qe1 + k] : kMixNeg) : (ok ? a.tq_env[qe1 + k] : kMixNeg);
                if (q > bq) { bq = q; tmax_env = ok ? a.tq_env[qe1 + k] : kMixNeg; }   // first maximum
            }
            td = chosen_env - (r_env + a.gamma_env * live * tmax_env);
        }
    }
    // ---- the team's error: ascending agents, one rounding per add, the same bits in every lane of the group ---------------------------
    float team = __shfl(td, 0, kMixGroup);
    for (int k = 1; k < n; ++k) team = team + __shfl(td, k, kMixGroup);
    if (own) {
        const float den0 = a.dens[0];
        *seed = (2.f * team * mask * mask / den0) * (float)n;
        out[2] = (team * mask) * (team * mask);
    }
}

void launch_team_td(const ssd_td_loss_args* a, hipStream_t s) {
    const int pairs = a->batch * (a->t_slots - 1);
    hipLaunchKernelGGL(k_team_td, dim3((pairs + kMixPairsPerBlock - 1) / kMixPairsPerBlock), dim3(kMixBlock), 0, s, *a);
}

}  // namespace ssd
