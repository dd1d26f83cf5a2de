// ssd_learner.hip -- the two integer/elementwise pieces of the homophily learner that sit on the data path.
//   k_build_inputs        HomophilyMAC._build_inputs tail   (controllers/homophily_controller.py:137-184)
//   k_incentive_transfer  incentive reward transfer         (learners/homophily_learner.py:94-115)
//   k_td_sim_loss         double-Q TD losses of both heads + similarity loss, forward AND the gradient w.r.t. the Q-values in one
//                         launch (learners/homophily_learner.py:94-217)
//   k_td_lambda_loss      the same loss with TD(lambda) targets for both heads (td_lambda > 0): one workgroup per (episode, agent),
//                         a backward weighted scan over t
// All but the last are elementwise / row kernels over [B(*T)*n] rows; one thread per output element / row.
#include "ssd_device.h"

namespace ssd {

__global__ void k_build_inputs(int32_t rows, int32_t n, int32_t A, int32_t t0, const int64_t* __restrict__ last_actions,
                               const float* __restrict__ last_reward, const int64_t* __restrict__ last_actions_inc,
                               const float* __restrict__ pos, float pos_scale, float* __restrict__ out,
                               int32_t out_stride, int32_t out_offset) {
    const int width = A + n + 4;
    const size_t total = (size_t)rows * width;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int row = (int)(idx / width), k = (int)(idx - (size_t)row * width);
        const int b = row / n, i = row - b * n;
        const int agent_major = t0 & 2;
        // t0 >> 8 = T > 0: the rows are [batch, T] and the three history tensors hold every step's OWN values -- the previous step is
        // row b - 1, none at the first step of an episode (the learner's time-batched assembly, no shifted copies)
        const int hist_T = t0 >> 8;
        const int t_zero = (t0 & 1) || (hist_T && b % hist_T == 0);
        const size_t pb = hist_T ? (size_t)b - 1 : (size_t)b, prow = pb * n + i;
        float v;
        if (k < A) v = (!t_zero && last_actions[prow] == k) ? 1.f : 0.f;                 // one-hot of the last action (:137-141)
        else if (k < A + n) v = (k - A == i) ? 1.f : 0.f;                            // agent id (:142-143)
        else if (k == A + n) {                                                       // sign(last reward) (:145-150)
            const float r = t_zero ? 0.f : last_reward[prow];
            v = (float)((r > 0.f) - (r < 0.f));
        } else if (k == A + n + 1) {                                                 // sign(#recv+ - #recv-) (:152-164)
            int recv = 0;
            if (!t_zero)
                for (int g = 0; g < n; ++g) {
                    if (g == i) continue;                                            // inc_mask_actions: no self incentive
                    const int64_t x = last_actions_inc[(pb * n + g) * n + i];
                    recv += (x == 1) - (x == 2);
                }
            v = (float)((recv > 0) - (recv < 0));
        } else v = pos[(size_t)row * 2 + (k - A - n - 2)] / pos_scale;               // pos / ||(H, W)|| (:179-181)
        const size_t orow = agent_major ? (size_t)i * (rows / n) + b : (size_t)row;
        out[orow * out_stride + out_offset + k] = v;
    }
}

// The same rows for any _build_inputs flag set: every block at the column the layout gives it (negative = absent).
__global__ void k_build_inputs_flags(int32_t rows, int32_t n, int32_t A, int32_t t0, BuildInputsLayout L,
                                     const int64_t* __restrict__ last_actions, const float* __restrict__ last_reward,
                                     const int64_t* __restrict__ last_actions_inc, const float* __restrict__ pos, float pos_scale,
                                     float* __restrict__ out, int32_t out_stride, int32_t out_offset) {
    const int width = L.width;
    const size_t total = (size_t)rows * width;
    const int agent_major = t0 & 2, hist_T = t0 >> 8;                    // hist_T: see k_build_inputs
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int row = (int)(idx / width), k = (int)(idx - (size_t)row * width);
        const int b = row / n, i = row - b * n;
        const int t_zero = (t0 & 1) || (hist_T && b % hist_T == 0);
        const size_t pb = hist_T ? (size_t)b - 1 : (size_t)b, prow = pb * n + i;
        float v = 0.f;
        if (L.o_act >= 0 && k >= L.o_act && k < L.o_act + A) v = (!t_zero && last_actions[prow] == k - L.o_act) ? 1.f : 0.f;  // (:137-141)
        else if (L.o_id >= 0 && k >= L.o_id && k < L.o_id + n) v = (k - L.o_id == i) ? 1.f : 0.f;                              // (:142-143)
        else if (k == L.o_r) {                                                                                                   // (:145-150)
            const float r = t_zero ? 0.f : last_reward[prow];
            v = (float)((r > 0.f) - (r < 0.f));
        } else if (k == L.o_i) {                                                                                                 // (:152-164)
            int recv = 0;
            if (!t_zero)
                for (int g = 0; g < n; ++g) {
                    if (g == i) continue;
                    const int64_t x = last_actions_inc[(pb * n + g) * n + i];
                    recv += (x == 1) - (x == 2);
                }
            v = (float)((recv > 0) - (recv < 0));
        } else if (L.o_oth >= 0 && k >= L.o_oth && k < L.o_oth + n * A) {          // everybody's last action, agent order (:166-173)
            const int g = (k - L.o_oth) / A, a = (k - L.o_oth) - g * A;
            v = (!t_zero && last_actions[pb * n + g] == a) ? 1.f : 0.f;
        } else if (L.o_dist >= 0 && k >= L.o_dist && k < L.o_dist + n) {           // 1 - |pos_i - pos_g| / ||(H, W)|| (:174-178)
            const int g = k - L.o_dist;
            const float dx = pos[(size_t)row * 2] - pos[((size_t)b * n + g) * 2], dy = pos[(size_t)row * 2 + 1] - pos[((size_t)b * n + g) * 2 + 1];
            v = 1.f - sqrtf(dx * dx + dy * dy) / pos_scale;
        } else if (L.o_pos >= 0 && k >= L.o_pos && k < L.o_pos + 2) v = pos[(size_t)row * 2 + (k - L.o_pos)] / pos_scale;       // (:179-181)
        const size_t orow = agent_major ? (size_t)i * (rows / n) + b : (size_t)row;
        out[orow * out_stride + out_offset + k] = v;
    }
}

BuildInputsLayout build_inputs_layout(int n, int A, uint32_t input_flags) {
    const uint32_t fl = input_flags ? (input_flags & ~SSD_INPUT_EXPLICIT) : (uint32_t)SSD_INPUT_FLAGS_SHIPPED;
    BuildInputsLayout L;
    int col = 0;
    auto take = [&](uint32_t bit, int w) { const int o = (fl & bit) ? col : -1; if (fl & bit) col += w; return o; };
    L.o_act = take(SSD_INPUT_LAST_ACTION, A);                            // the reference's order (homophily_controller.py:137-184)
    L.o_id = take(SSD_INPUT_AGENT_ID, n);
    L.o_r = take(SSD_INPUT_REWARD, 1);
    L.o_i = take(SSD_INPUT_INC_REWARD, 1);
    L.o_oth = take(SSD_INPUT_OTHERS_LAST_ACTION, n * A);
    L.o_dist = take(SSD_INPUT_DISTANCE, n);
    L.o_pos = take(SSD_INPUT_AGENT_POS, 2);
    L.width = col;
    return L;
}

__global__ void k_incentive_transfer(int32_t B, int32_t T, int32_t n, const int64_t* __restrict__ a_inc,
                                     const float* __restrict__ rewards, float effect_ratio, float cost_ratio,
                                     float incentive, float seq_len, float* __restrict__ give, float* __restrict__ recv_pos,
                                     float* __restrict__ recv_neg, float* __restrict__ recv_zero, float* __restrict__ r_env,
                                     float* __restrict__ r_inc) {
    const size_t total = (size_t)B * T * n;
    for (size_t it = (size_t)blockIdx.x * blockDim.x + threadIdx.x; it < total; it += (size_t)gridDim.x * blockDim.x) {
        const size_t bt = it / n;
        const int i = (int)(it - bt * n);
        const int b = (int)(bt / T), t = (int)(bt - (size_t)b * T);
        const int64_t* m = a_inc + bt * n * n;
        int g = 0, rp = 0, rn = 0;
        for (int j = 0; j < n; ++j) {
            if (j == i) continue;
            g += m[(size_t)i * n + j] != 0;            // give: i -> j  (:101)
            const int64_t x = m[(size_t)j * n + i];    // receive: j -> i (:102-103)
            rp += x == 1; rn += x == 2;
        }
        recv_pos[it] = (float)rp; recv_neg[it] = (float)rn; recv_zero[it] = (float)(n - 1 - rp - rn);
        if (t < T - 1) {
            const size_t i1 = ((size_t)b * (T - 1) + t) * n + i;
            give[i1] = (float)g;
            const float r = rewards[i1];
            r_env[i1] = (r + (float)(rp - rn) * effect_ratio * incentive) / seq_len;   // :113
            r_inc[i1] = (r - (float)g * cost_ratio * incentive) / seq_len;             // :114
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// k_td_sim_loss: what homophily_learner.py:94-217 builds out of ~100 tensor ops (and autograd differentiates with ~200 more), per
// (episode b, transition t, agent i) in one thread:
//   incentive transfer (:94-115)   give_i, recv+-_i -> rewards_for_env / rewards_for_inc = (r +- ...) / max_seq_length
//   env head TD (:118-177)         double-Q: a* = argmax of the LIVE q_env[t+1] over the available actions, value from the TARGET net;
//                                  td = q_env[t, a_t] - (r_env + gamma_env (1 - terminated) tq_env[t+1, a*])
//   inc head TD                    per receiver j != i: a*_j = argmax_c q_inc[t+1, i, j, c];
//                                  td = sum_j q_inc[t, i, j, a_inc_ij] - (r_inc + gamma_inc (1 - terminated) sum_j tq_inc[t+1, i, j, a*_j])
//     consider_others_inc (:122-126,148-171), with recv_c,j(t) = the RECEIVER j's received counts (zero, +, -) at t (receive_*
//     [bs, t, n].unsqueeze(2) broadcasts over the giver i):
//                                  chosen_ij = sum_c q_inc[t, i, j, c] recv_c,j(t) / (n - 1);
//                                  tmax_ij = (tq_inc[t+1, i, j, a*_j] + sum_c tq_inc[t+1, i, j, c] recv_c,j(t+1) - tq_inc[t+1, i, j, a_inc(t+1)_ij]) / (n - 1)
//   similarity loss (:184-217)     window (sim_horizon) activity flags -> cluster = 2 rw + cn (the exact-value rule standing in for x-means,
//                                  SURVEY.md 8c), idle = cn + rw; for every ordered triple i != k != j != i with equal clusters:
//                                  clamp_min(-log softmax(q_inc[t, i, j])[a_inc_kj], threshold) * idle_i * idle_k
//   L = (sum (td_env mask)^2 + sum (td_inc mask)^2) / den0 + w_sim * sum_sim / (1 + den1),   den = the GLOBAL denominators (data parallel)
// Outputs: per-thread partial sums (the caller adds them in a fixed order) and, MODE 1, dL/dq_env and dL/dq_inc -- each thread owns
// the gradient rows of its (b, t, i), so nothing is accumulated across threads (deterministic).  MODE 0: the two denominators only.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr float kNeg = -9999999.f;            // the reference's masked_fill value (homophily_learner.py:137,150)
template <int MODE>
__global__ __launch_bounds__(128) void k_td_sim_loss(ssd_td_loss_args a) {
    const int B = a.batch, T1 = a.t_slots, T = T1 - 1, n = a.n_agents, A = a.n_actions;
    const int total = B * T1 * n;
    const int it = blockIdx.x * blockDim.x + threadIdx.x;
    if (it >= total) return;
    const int i = it % n, bt = it / n, t = bt % T1, b = bt / T1;
    float* dqe = MODE ? a.dq_env + (size_t)it * A : nullptr;
    float* dqi = MODE ? a.dq_inc + (size_t)it * n * 3 : nullptr;
    if (t == T) {                              // the bootstrap slot: its Q-values enter the targets only (no gradient)
        if (MODE) { for (int k = 0; k < A; ++k) dqe[k] = 0.f; for (int k = 0; k < n * 3; ++k) dqi[k] = 0.f; }
        return;
    }
    float* out = a.partials + ((size_t)(b * T + t) * n + i) * SSD_TD_LOSS_PARTIALS;
    const size_t row = (size_t)bt * n;                                          // (b, t, agent 0)
    const float mask = (float)a.filled[bt] * (t ? 1.f - (float)a.terminated[bt - 1] : 1.f);   // :62-64
    // ---- similarity mask: window flags of every agent (:184-191), cluster / idle (:194-206) ------------------------------------
    uint32_t cn_bits = 0, rw_bits = 0;
    const int t_lo = t - a.sim_horizon + 1 > 0 ? t - a.sim_horizon + 1 : 0;
    for (int k = 0; k < n; ++k) {
        float cn = 0.f, rw = 0.f;
        for (int tau = t_lo; tau <= t; ++tau) {
            const size_t e = ((size_t)b * T1 + tau) * n + k;
            cn += a.clean_num[e] > 0.f ? 1.f : 0.f;
            rw += a.reward[e] / a.reward_scale;
        }
        cn_bits |= (cn > 0.f ? 1u : 0u) << k; rw_bits |= (rw > 0.f ? 1u : 0u) << k;
    }
    const int cn_i = (cn_bits >> i) & 1, rw_i = (rw_bits >> i) & 1, cl_i = 2 * rw_i + cn_i, idle_i = cn_i + rw_i;
    // sim(i, k) = [cluster_i == cluster_k] idle_i idle_k  (0, 1, 2 or 4)
    auto sim_ik = [&](int k) -> float {
        const int cn_k = (cn_bits >> k) & 1, rw_k = (rw_bits >> k) & 1;
        return (2 * rw_k + cn_k == cl_i) ? (float)(idle_i * (cn_k + rw_k)) : 0.f;
    };
    float sim_sum = 0.f;
    for (int k = 0; k < n; ++k) { if (k != i) sim_sum += sim_ik(k) * (float)(n - 2); }   // receivers j != i, j != k
    out[0] = mask; out[1] = sim_sum;
    if (!MODE) return;
    // ---- incentive transfer (:94-115) ----------------------------------------------------------------------------------------------
    const int64_t* ainc = a.actions_inc + row * n;                              // [giver][receiver] at (b, t)
    int give = 0, rp = 0, rn = 0;
    for (int j = 0; j < n; ++j) {
        if (j == i) continue;
        give += ainc[(size_t)i * n + j] != 0;
        const int64_t x = ainc[(size_t)j * n + i];
        rp += x == 1; rn += x == 2;
    }
    const float r = a.reward[row + i] / a.reward_scale;
    const float clean = a.clean_num[row + i] > 0.f ? 1.f : 0.f;
    const float rv = (float)(rp - rn);
    const float r_env = (r + rv * a.incentive_ratio * a.incentive) / a.seq_len;
    const float r_inc = (r - (float)give * a.incentive_cost * a.incentive) / a.seq_len;
    const float live = 1.f - (float)a.terminated[bt];
    const float den0 = a.dens[0], den1 = 1.f + a.dens[1];
    // ---- env head (:118-177) ---------------------------------------------------------------------------------------------------
    const size_t qe = (size_t)it * A, qe1 = qe + (size_t)n * A;                 // (b, t, i) and (b, t + 1, i)
    const int a_t = (int)a.actions[row + i];
    const float chosen_env = a.q_env[qe + a_t];
    float tmax_env;
    {
        int best = 0; float bq = -INFINITY, btq = kNeg;
        for (int k = 0; k < A; ++k) {
            const bool ok = a.avail[qe1 + k] != 0;
            const float q = a.double_q ? (ok ? a.q_env[qe1 + k] : kNeg) : (ok ? a.tq_env[qe1 + k] : kNeg);
            if (q > bq) { bq = q; best = k; btq = ok ? a.tq_env[qe1 + k] : kNeg; }   // first maximum
        }
        (void)best;
        tmax_env = btq;
    }
    const float td_env = chosen_env - (r_env + a.gamma_env * live * tmax_env);
    const float g_env = 2.f * td_env * mask * mask / den0;
    for (int k = 0; k < A; ++k) dqe[k] = k == a_t ? g_env : 0.f;
    // ---- inc head: TD over the receivers j != i ---------------------------------------------------------------------------------
    const size_t qi = (size_t)it * n * 3, qi1 = qi + (size_t)n * n * 3;
    // consider_others_inc: the chosen value and the target weigh receiver j's received counts (zero, +, -) at t and t + 1, over n - 1
    const bool others = a.consider_others_inc != 0;
    const int64_t* ainc1 = ainc + (size_t)n * n;                                // (b, t + 1)
    auto recv_of = [&](const int64_t* acts, int j, float& r0, float& r1, float& r2) {
        int p = 0, m = 0;
        for (int g = 0; g < n; ++g) {
            if (g == j) continue;
            const int64_t x = acts[(size_t)g * n + j];
            p += x == 1; m += x == 2;
        }
        r0 = (float)(n - 1 - p - m); r1 = (float)p; r2 = (float)m;
    };
    float sum_chosen = 0.f, sum_tmax = 0.f, q_inc_taken = 0.f;
    for (int j = 0; j < n; ++j) {
        const int c = (int)ainc[(size_t)i * n + j];
        const float qc = a.q_inc[qi + j * 3 + c];
        q_inc_taken += qc;
        if (j == i) continue;
        const float* sel = (a.double_q ? a.q_inc : a.tq_inc) + qi1 + j * 3;
        const int best = sel[1] > sel[0] ? (sel[2] > sel[1] ? 2 : 1) : (sel[2] > sel[0] ? 2 : 0);   // first maximum
        const float* tq = a.tq_inc + qi1 + j * 3;
        if (others) {
            const float* q = a.q_inc + qi + j * 3;
            float r0, r1, r2;
            recv_of(ainc, j, r0, r1, r2);
            sum_chosen += (q[0] * r0 + q[1] * r1 + q[2] * r2) / (float)(n - 1);
            recv_of(ainc1, j, r0, r1, r2);
            const float other = tq[0] * r0 + tq[1] * r1 + tq[2] * r2;
            sum_tmax += (tq[best] + other - tq[(int)ainc1[(size_t)i * n + j]]) / (float)(n - 1);
        } else {
            sum_chosen += qc;
            sum_tmax += tq[best];
        }
    }
    const float td_inc = sum_chosen - (r_inc + a.gamma_inc * live * sum_tmax);
    const float g_inc = 2.f * td_inc * mask * mask / den0;
    // d chosen_ij / d q_inc[t, i, j, x]: 1 at the taken action, or recv_x,j(t) / (n - 1) with consider_others_inc
    const float gd = g_inc / (float)(n - 1);
    // ---- similarity loss (:208-217) and the inc gradient rows ------------------------------------------------------------------------
    float sim_num = 0.f;
    const float wsim = a.sim_loss_weight / den1;
    for (int j = 0; j < n; ++j) {
        const float q0 = a.q_inc[qi + j * 3], q1 = a.q_inc[qi + j * 3 + 1], q2 = a.q_inc[qi + j * 3 + 2];
        const float mx = fmaxf(q0, fmaxf(q1, q2));
        const float e0 = expf(q0 - mx), e1 = expf(q1 - mx), e2 = expf(q2 - mx), es = e0 + e1 + e2;
        const float p[3] = {e0 / es, e1 / es, e2 / es};
        float g[3] = {0.f, 0.f, 0.f};
        if (j != i) {
            for (int k = 0; k < n; ++k) {
                if (k == i || k == j) continue;
                const float sm = sim_ik(k);
                if (sm == 0.f) continue;
                const int c = (int)ainc[(size_t)k * n + j];                     // the incentive action k actually gave j
                const float nl = -logf(c == 0 ? p[0] : c == 1 ? p[1] : p[2]);
                sim_num += fmaxf(nl, a.sim_threshold) * sm;
                if (nl >= a.sim_threshold) {                                    // clamp_min passes the gradient where input >= min
                    g[0] += sm * (p[0] - (c == 0 ? 1.f : 0.f)); g[1] += sm * (p[1] - (c == 1 ? 1.f : 0.f)); g[2] += sm * (p[2] - (c == 2 ? 1.f : 0.f));
                }
            }
        }
        const int cij = (int)ainc[(size_t)i * n + j];
        if (others && j != i) {
            float r0, r1, r2;
            recv_of(ainc, j, r0, r1, r2);
            dqi[j * 3] = wsim * g[0] + gd * r0; dqi[j * 3 + 1] = wsim * g[1] + gd * r1; dqi[j * 3 + 2] = wsim * g[2] + gd * r2;
        } else {
            for (int x = 0; x < 3; ++x) dqi[j * 3 + x] = wsim * g[x] + ((j != i && x == cij) ? g_inc : 0.f);
        }
    }
    out[2] = (td_env * mask) * (td_env * mask); out[3] = (td_inc * mask) * (td_inc * mask); out[4] = sim_num;
    out[5] = chosen_env; out[6] = q_inc_taken; out[7] = (float)give; out[8] = rv;
    out[9] = clean * rv; out[10] = clean; out[11] = r * rv; out[12] = r;
}

// ---------------------------------------------------------------------------------------------------------------------------
// k_td_lambda_loss: the same loss with TD(lambda) targets for both heads (td_lambda > 0; the reference ships the recursion as
// utils/rl_utils.py:4-14, build_td_lambda_targets).  With a_h = lambda gamma_h and, per row t of one (episode b, agent i),
//   b_h,t = mask_t (r_h,t + (1 - lambda) gamma_h V_h,t+1 live_t)          V = tmax_env / sum_tmax, the one-step bootstrap values
//   G_h,T = V_h,T (1 - sum_{t<T} terminated[b, t]),   G_h,t = a_h G_h,t+1 + b_h,t,   td_h,t = chosen_h,t - G_h,t
// One workgroup per (b, i), one thread per row; the episode is walked in chunks of 256 rows from its END backwards (thread 255 of
// the first chunk is row T - 1, so G_T enters as that chunk's carry and any T works).  Per chunk: every thread evaluates its row's
// one-step pieces with the expressions and operation order of k_td_sim_loss<1>; a weighted suffix scan S_p = sum_{q >= p} a^(q-p) b_q
// inside each wave (six __shfl_down steps with the weights a, a^2, a^4 .. a^32); lane 0 of every wave publishes its S through LDS and
// every thread chains the four of them behind the incoming carry in the same fixed order (C_3 = carry, C_w = S_head[w+1] + a^64
// C_w+1), so G_p = S_p + a^(64 - lane) C_wave and the next chunk's carry is G of thread 0.  No atomics, nothing crosses workgroups.
// With -ffp-contract=off a row's b_h,t is mask times the bits of the one-step target, and for a lambda whose a^2 underflows
// (2^-100) td is the one-step td wherever mask is 1.  partials columns 0 .. 12 as k_td_sim_loss<1>, 13 / 14 = G_env,t / G_inc,t.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_td_lambda_loss(ssd_td_loss_args a) {
    __shared__ float s_head[2][4], s_boot[2];
    __shared__ int s_term[4];
    const int T1 = a.t_slots, T = T1 - 1, n = a.n_agents, A = a.n_actions;
    const int b = blockIdx.x / n, i = blockIdx.x - b * n;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // the bootstrap slot: its Q-values enter the targets only (no gradient)
    {
        const size_t itT = ((size_t)b * T1 + T) * n + i;
        for (int k = tid; k < A; k += 256) a.dq_env[itT * A + k] = 0.f;
        for (int k = tid; k < n * 3; k += 256) a.dq_inc[itT * n * 3 + k] = 0.f;
    }
    // 1 - sum_{t < T} terminated[b, t]: the flags are 0 / 1, so the sum is exact in any order
    int nterm = 0;
    for (int t = tid; t < T; t += 256) nterm += (int)a.terminated[(size_t)b * T1 + t];
    for (int d = 32; d; d >>= 1) nterm += __shfl_down(nterm, d);
    if (lane == 0) s_term[wave] = nterm;
    // a_h^(2^j), j = 0 .. 6, and this lane's a_h^(64 - lane)
    const float lam = a.td_lambda;
    const float c_env = (1.f - lam) * a.gamma_env, c_inc = (1.f - lam) * a.gamma_inc;
    float we[7], wi[7];
    we[0] = lam * a.gamma_env; wi[0] = lam * a.gamma_inc;
    for (int j = 1; j < 7; ++j) { we[j] = we[j - 1] * we[j - 1]; wi[j] = wi[j - 1] * wi[j - 1]; }
    float pe = 1.f, pi = 1.f;
    for (int j = 0; j < 7; ++j)
        if (((64 - lane) >> j) & 1) { pe *= we[j]; pi *= wi[j]; }
    const float den0 = a.dens[0], den1 = 1.f + a.dens[1];
    const bool others = a.consider_others_inc != 0;
    float carry_env = 0.f, carry_inc = 0.f;
    for (int c1 = T; c1 > 0; c1 -= 256) {                                       // rows [c1 - 256, c1), thread 255 = row c1 - 1
        const int t = c1 - 256 + tid;
        const bool valid = t >= 0;
        const int bt = b * T1 + (valid ? t : 0), it = bt * n + i;
        const size_t row = (size_t)bt * n;                                      // (b, t, agent 0)
        const int64_t* ainc = a.actions_inc + row * n;                          // [giver][receiver] at (b, t)
        const size_t qi = (size_t)it * n * 3, qi1 = qi + (size_t)n * n * 3;
        float mask = 0.f, sim_sum = 0.f, r = 0.f, clean = 0.f, rv = 0.f, chosen_env = 0.f, sum_chosen = 0.f, q_inc_taken = 0.f;
        float b_env = 0.f, b_inc = 0.f;
        uint32_t cn_bits = 0, rw_bits = 0;
        int give = 0, a_t = 0, cl_i = 0, idle_i = 0;
        // sim(i, k) = [cluster_i == cluster_k] idle_i idle_k  (0, 1, 2 or 4)
        auto sim_ik = [&](int k) -> float {
            const int cn_k = (cn_bits >> k) & 1, rw_k = (rw_bits >> k) & 1;
            return (2 * rw_k + cn_k == cl_i) ? (float)(idle_i * (cn_k + rw_k)) : 0.f;
        };
        auto recv_of = [&](const int64_t* acts, int j, float& r0, float& r1, float& r2) {
            int p = 0, m = 0;
            for (int g = 0; g < n; ++g) {
                if (g == j) continue;
                const int64_t x = acts[(size_t)g * n + j];
                p += x == 1; m += x == 2;
            }
            r0 = (float)(n - 1 - p - m); r1 = (float)p; r2 = (float)m;
        };
        if (valid) {
            mask = (float)a.filled[bt] * (t ? 1.f - (float)a.terminated[bt - 1] : 1.f);   // :62-64
            // ---- similarity mask: window flags of every agent (:184-191), cluster / idle (:194-206) --------------------------------
            const int t_lo = t - a.sim_horizon + 1 > 0 ? t - a.sim_horizon + 1 : 0;
            for (int k = 0; k < n; ++k) {
                float cn = 0.f, rw = 0.f;
                for (int tau = t_lo; tau <= t; ++tau) {
                    const size_t e = ((size_t)b * T1 + tau) * n + k;
                    cn += a.clean_num[e] > 0.f ? 1.f : 0.f;
                    rw += a.reward[e] / a.reward_scale;
                }
                cn_bits |= (cn > 0.f ? 1u : 0u) << k; rw_bits |= (rw > 0.f ? 1u : 0u) << k;
            }
            const int cn_i = (cn_bits >> i) & 1, rw_i = (rw_bits >> i) & 1;
            cl_i = 2 * rw_i + cn_i; idle_i = cn_i + rw_i;
            for (int k = 0; k < n; ++k) { if (k != i) sim_sum += sim_ik(k) * (float)(n - 2); }   // receivers j != i, j != k
            // ---- incentive transfer (:94-115) ------------------------------------------------------------------------------------------
            int rp = 0, rn = 0;
            for (int j = 0; j < n; ++j) {
                if (j == i) continue;
                give += ainc[(size_t)i * n + j] != 0;
                const int64_t x = ainc[(size_t)j * n + i];
                rp += x == 1; rn += x == 2;
            }
            r = a.reward[row + i] / a.reward_scale;
            clean = a.clean_num[row + i] > 0.f ? 1.f : 0.f;
            rv = (float)(rp - rn);
            const float r_env = (r + rv * a.incentive_ratio * a.incentive) / a.seq_len;
            const float r_inc = (r - (float)give * a.incentive_cost * a.incentive) / a.seq_len;
            const float live = 1.f - (float)a.terminated[bt];
            // ---- env head: chosen value and bootstrap value (:118-177) -------------------------------------------------------------------
            const size_t qe = (size_t)it * A, qe1 = qe + (size_t)n * A;             // (b, t, i) and (b, t + 1, i)
            a_t = (int)a.actions[row + i];
            chosen_env = a.q_env[qe + a_t];
            float bq = -INFINITY, tmax_env = kNeg;
            for (int k = 0; k < A; ++k) {
                const bool ok = a.avail[qe1 + k] != 0;
                const float q = a.double_q ? (ok ? a.q_env[qe1 + k] : kNeg) : (ok ? a.tq_env[qe1 + k] : kNeg);
                if (q > bq) { bq = q; tmax_env = ok ? a.tq_env[qe1 + k] : kNeg; }    // first maximum
            }
            // ---- inc head over the receivers j != i --------------------------------------------------------------------------------------
            const int64_t* ainc1 = ainc + (size_t)n * n;                            // (b, t + 1)
            float sum_tmax = 0.f;
            for (int j = 0; j < n; ++j) {
                const int c = (int)ainc[(size_t)i * n + j];
                const float qc = a.q_inc[qi + j * 3 + c];
                q_inc_taken += qc;
                if (j == i) continue;
                const float* sel = (a.double_q ? a.q_inc : a.tq_inc) + qi1 + j * 3;
                const int best = sel[1] > sel[0] ? (sel[2] > sel[1] ? 2 : 1) : (sel[2] > sel[0] ? 2 : 0);   // first maximum
                const float* tq = a.tq_inc + qi1 + j * 3;
                if (others) {
                    const float* q = a.q_inc + qi + j * 3;
                    float r0, r1, r2;
                    recv_of(ainc, j, r0, r1, r2);
                    sum_chosen += (q[0] * r0 + q[1] * r1 + q[2] * r2) / (float)(n - 1);
                    recv_of(ainc1, j, r0, r1, r2);
                    const float other = tq[0] * r0 + tq[1] * r1 + tq[2] * r2;
                    sum_tmax += (tq[best] + other - tq[(int)ainc1[(size_t)i * n + j]]) / (float)(n - 1);
                } else {
                    sum_chosen += qc;
                    sum_tmax += tq[best];
                }
            }
            b_env = mask * (r_env + c_env * tmax_env * live);
            b_inc = mask * (r_inc + c_inc * sum_tmax * live);
            if (t == T - 1) { s_boot[0] = tmax_env; s_boot[1] = sum_tmax; }       // V_h,T: first chunk, thread 255
        }
        // ---- weighted suffix scan inside the wave -------------------------------------------------------------------------------------
        float s_env = b_env, s_inc = b_inc;
        for (int j = 0; j < 6; ++j) {
            const int d = 1 << j;
            const float oe = __shfl_down(s_env, d), oi = __shfl_down(s_inc, d);
            if (lane + d < 64) { s_env += we[j] * oe; s_inc += wi[j] * oi; }
        }
        if (lane == 0) { s_head[0][wave] = s_env; s_head[1][wave] = s_inc; }
        __syncthreads();
        // ---- the four waves behind the carry, fixed order ---------------------------------------------------------------------------
        if (c1 == T) {
            const float not_term = 1.f - (float)(((s_term[0] + s_term[1]) + s_term[2]) + s_term[3]);
            carry_env = s_boot[0] * not_term; carry_inc = s_boot[1] * not_term;
        }
        float cw_env = carry_env, cw_inc = carry_inc;                               // C_3
        for (int w = 3; w >= 0; --w) {
            if (w == wave) { s_env += pe * cw_env; s_inc += pi * cw_inc; }        // G of this row
            cw_env = s_head[0][w] + we[6] * cw_env; cw_inc = s_head[1][w] + wi[6] * cw_inc;
        }
        carry_env = cw_env; carry_inc = cw_inc;                                     // G of thread 0: the next chunk's carry
        __syncthreads();                                                            // s_head is rewritten by the next chunk
        if (!valid) continue;
        // ---- td, gradient rows, partials ---------------------------------------------------------------------------------------------
        float* out = a.partials + ((size_t)(b * T + t) * n + i) * SSD_TD_LOSS_PARTIALS;
        float* dqe = a.dq_env + (size_t)it * A;
        float* dqi = a.dq_inc + qi;
        const float td_env = chosen_env - s_env;
        const float g_env = 2.f * td_env * mask * mask / den0;
        for (int k = 0; k < A; ++k) dqe[k] = k == a_t ? g_env : 0.f;
        const float td_inc = sum_chosen - s_inc;
        const float g_inc = 2.f * td_inc * mask * mask / den0;
        // d chosen_ij / d q_inc[t, i, j, x]: 1 at the taken action, or recv_x,j(t) / (n - 1) with consider_others_inc
        const float gd = g_inc / (float)(n - 1);
        // ---- similarity loss (:208-217) and the inc gradient rows ------------------------------------------------------------------------
        float sim_num = 0.f;
        const float wsim = a.sim_loss_weight / den1;
        for (int j = 0; j < n; ++j) {
            const float q0 = a.q_inc[qi + j * 3], q1 = a.q_inc[qi + j * 3 + 1], q2 = a.q_inc[qi + j * 3 + 2];
            const float mx = fmaxf(q0, fmaxf(q1, q2));
            const float e0 = expf(q0 - mx), e1 = expf(q1 - mx), e2 = expf(q2 - mx), es = e0 + e1 + e2;
            const float p[3] = {e0 / es, e1 / es, e2 / es};
            float g[3] = {0.f, 0.f, 0.f};
            if (j != i) {
                for (int k = 0; k < n; ++k) {
                    if (k == i || k == j) continue;
                    const float sm = sim_ik(k);
                    if (sm == 0.f) continue;
                    const int c = (int)ainc[(size_t)k * n + j];                     // the incentive action k actually gave j
                    const float nl = -logf(c == 0 ? p[0] : c == 1 ? p[1] : p[2]);
                    sim_num += fmaxf(nl, a.sim_threshold) * sm;
                    if (nl >= a.sim_threshold) {                                    // clamp_min passes the gradient where input >= min
                        g[0] += sm * (p[0] - (c == 0 ? 1.f : 0.f)); g[1] += sm * (p[1] - (c == 1 ? 1.f : 0.f)); g[2] += sm * (p[2] - (c == 2 ? 1.f : 0.f));
                    }
                }
            }
            const int cij = (int)ainc[(size_t)i * n + j];
            if (others && j != i) {
                float r0, r1, r2;
                recv_of(ainc, j, r0, r1, r2);
                dqi[j * 3] = wsim * g[0] + gd * r0; dqi[j * 3 + 1] = wsim * g[1] + gd * r1; dqi[j * 3 + 2] = wsim * g[2] + gd * r2;
            } else {
                for (int x = 0; x < 3; ++x) dqi[j * 3 + x] = wsim * g[x] + ((j != i && x == cij) ? g_inc : 0.f);
            }
        }
        out[0] = mask; out[1] = sim_sum;
        out[2] = (td_env * mask) * (td_env * mask); out[3] = (td_inc * mask) * (td_inc * mask); out[4] = sim_num;
        out[5] = chosen_env; out[6] = q_inc_taken; out[7] = (float)give; out[8] = rv;
        out[9] = clean * rv; out[10] = clean; out[11] = r * rv; out[12] = r;
        out[13] = s_env; out[14] = s_inc;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// k_column_sums: out[g, c] = sum_r x[g, r, c] (bias gradients: the row sums of dL/dY).  One workgroup per (g, 64 columns): 4 waves
// each sum every 4th row of their column (coalesced across the 64 columns), then the four partial sums are added in a fixed
// order through LDS -- deterministic, no cross-workgroup hand-off (ATen's multi-block reductions keep arrival semaphores that a
// memset node clears; inside replayed hipGraphs they were observed to return other reductions' partial sums on this stack).
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_column_sums(const float* __restrict__ x, float* __restrict__ out, int R, int C, int chunk) {
    __shared__ float part[4][64];
    const int lane = threadIdx.x & 63, rg = threadIdx.x >> 6, c = blockIdx.x * 64 + lane, g = blockIdx.y;
    const int r0 = blockIdx.z * chunk, r1 = r0 + chunk < R ? r0 + chunk : R;       // this workgroup's rows
    float s0 = 0.f, s1 = 0.f;                                          // two chains: independent loads in flight
    if (c < C) {
        const float* p = x + (size_t)g * R * C + c;
        int r = r0 + rg;
        for (; r + 4 < r1; r += 8) { s0 += p[(size_t)r * C]; s1 += p[(size_t)(r + 4) * C]; }
        if (r < r1) s0 += p[(size_t)r * C];
    }
    part[rg][lane] = s0 + s1;
    __syncthreads();
    if (rg == 0 && c < C) out[((size_t)g * gridDim.z + blockIdx.z) * C + c] = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
}

// ---------------------------------------------------------------------------------------------------------------------------
// k_copy_blocks: up to SSD_COPY_BLOCKS_MAX strided 2-D block copies in one launch (blockIdx.y = block, table by value in the
// kernel arguments): the side-by-side r | z | n images of the GRU parameters and the split of their gradients.
// ---------------------------------------------------------------------------------------------------------------------------
struct CopyTable { ssd_block_copy e[SSD_COPY_BLOCKS_MAX]; };
__global__ __launch_bounds__(256) void k_copy_blocks(CopyTable t) {
    const ssd_block_copy b = t.e[blockIdx.y];
    const int total = b.rows * b.cols;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int r = i / b.cols, c = i - r * b.cols;
        b.dst[(size_t)r * b.dst_stride + c] = b.src[(size_t)r * b.src_stride + c];
    }
}

// k_fill_blocks: up to SSD_FILL_BLOCKS_MAX 32-bit pattern fills in one launch (blockIdx.y = block): the runner state an episode opens
// with (previous actions -1, previous reward / incentive actions / returns / hidden states / time index 0) was seven fill launches.
struct FillTable { ssd_block_fill e[SSD_FILL_BLOCKS_MAX]; };
__global__ __launch_bounds__(256) void k_fill_blocks(FillTable t) {
    const ssd_block_fill b = t.e[blockIdx.y];
    uint32_t* d = static_cast<uint32_t*>(b.dst);
    const size_t words = (size_t)b.bytes >> 2;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (size_t)gridDim.x * 256) d[i] = b.value;
}
void launch_fill_blocks(const ssd_block_fill* blocks, int count, hipStream_t stream) {
    FillTable t;
    size_t most = 4;
    for (int i = 0; i < SSD_FILL_BLOCKS_MAX; ++i) {
        t.e[i] = blocks[i < count ? i : 0];
        if (i < count && (size_t)blocks[i].bytes > most) most = (size_t)blocks[i].bytes;
    }
    int gx = (int)((most / 4 + 1023) / 1024);                          // 4 words per thread for the largest block
    if (gx < 1) gx = 1;
    if (gx > 256) gx = 256;
    hipLaunchKernelGGL(k_fill_blocks, dim3(gx, count), dim3(256), 0, stream, t);
}

// k_runner_stats: the device side of EpisodeRunner's episode statistics (episode_runner.py:121-152) for one rollout of all envs:
// acc[0..3] += sum collective_return, sum equality, sum of the agents' episode returns, sum of their squares, in f64, one workgroup,
// a fixed-order tree (deterministic) -- ten ATen launches (casts, four reductions, a product, a concatenation, an addition) before.
__global__ __launch_bounds__(1024) void k_runner_stats(const float* __restrict__ coll, const float* __restrict__ eq, const float* __restrict__ ret,
                                                       int n_env, int n_ret, double* __restrict__ acc) {
    __shared__ double red[4][1024];
    const int t = threadIdx.x;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = t; i < n_env; i += 1024) { s[0] += (double)coll[i]; s[1] += (double)eq[i]; }
    for (int i = t; i < n_ret; i += 1024) { const double r = (double)ret[i]; s[2] += r; s[3] += r * r; }
#pragma unroll
    for (int k = 0; k < 4; ++k) red[k][t] = s[k];
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if (t < w) {
#pragma unroll
            for (int k = 0; k < 4; ++k) red[k][t] += red[k][t + w];
        }
        __syncthreads();
    }
    if (t < 4) acc[t] += red[t][0];
}
void launch_runner_stats(const float* coll, const float* eq, const float* ret, int n_env, int n_ret, double* acc, hipStream_t stream) {
    hipLaunchKernelGGL(k_runner_stats, dim3(1), dim3(1024), 0, stream, coll, eq, ret, n_env, n_ret, acc);
}

// ---------------------------------------------------------------------------------------------------------------------------
// k_behaviour_partials / k_behaviour_finish: the per-agent behaviour statistics of one rollout (ssd_behaviour_stats; the block table is
// in include/ssd_hip.h), all in integers.
// A wave walks one env at a time.  Lane = (time row tl, receiver j) with j = lane % n fixed for the whole kernel: 64 / n time rows per
// pass, so everything that is indexed by the agent alone lives in the lane's registers as int64 sums over all of the wave's envs and
// reaches LDS once, at the end; only the counters whose index depends on the DATA (action_count, inc_count) are LDS atomics per
// element.  A lane reads its receiver's column of the n x n incentive block of its time row (n loads of 8 bytes; the n lanes of a row
// cover its n * n * 8 contiguous bytes between them), its action, reward and clean_num.  Every load's address is clamped into the env's
// own block (time row 0 for a lane past T, the diagonal element for a giver index past n) and the value masked: no load behind a
// data-dependent branch, slot T is never addressed.  The per-episode sums C, Hh of a receiver are added over its lanes by 64 / n
// bpermutes at the end of the env; lanes 0 .. n-1 then hold the agents' roles, a ballot counts the cleaners.
// Integer sums commute: the LDS atomics' order does not show.  A workgroup writes its own row of the workspace; the second launch
// (one workgroup) adds the rows in index order into the f64 accumulator.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int BEH_WAVES = SSD_BEHAVIOUR_WAVES;
constexpr int BEH_LEN_MAX = SSD_BEHAVIOUR_LEN(SSD_MAX_AGENTS, 16);

__device__ __forceinline__ void beh_add(long long* cnt, int k, long long v) {
    atomicAdd(reinterpret_cast<unsigned long long*>(cnt + k), (unsigned long long)v);
}
__device__ __forceinline__ int beh_round(float x) {                    // nearest integer; NaN -> 0, |x| > 2^24 -> 2^24
    x = x == x ? x : 0.f;
    return (int)rintf(fminf(fmaxf(x, -16777216.f), 16777216.f));
}

__global__ __launch_bounds__(64 * BEH_WAVES) void k_behaviour_partials(const int64_t* __restrict__ actions, const int64_t* __restrict__ actions_inc,
                                                                       const float* __restrict__ reward, const float* __restrict__ clean,
                                                                       int n_env, int T, int n, int A, long long* __restrict__ ws) {
    __shared__ long long cnt[BEH_LEN_MAX];
    const int len = SSD_BEHAVIOUR_LEN(n, A);
    for (int k = threadIdx.x; k < len; k += 64 * BEH_WAVES) cnt[k] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tpw = 64 / n, nn = n * n;                                // time rows per pass
    const int tl = lane / n, j = lane - tl * n;
    const bool active = tl < tpw;
    const int o_act = 5 * n, o_inc = o_act + n * A, o_rc = o_inc + 3 * nn, o_role = o_rc + 2 * n, o_hist = o_role + 4 * n, o_ep = o_hist + n + 1;
    long long s_r = 0, s_c = 0, s_cl = 0, s_hv = 0, s_ht = 0, s_rc = 0, s_rr = 0, envs = 0;
    const size_t row = (size_t)(T + 1) * n;                            // elements of one env in the [n_env, T + 1, n] fields
    for (long b = (long)blockIdx.x * BEH_WAVES + wave; b < n_env; b += (long)gridDim.x * BEH_WAVES) {
        const int64_t* a_e = actions + (size_t)b * row;
        const int64_t* ai_e = actions_inc + (size_t)b * row * n;
        const float* r_e = reward + (size_t)b * row;
        const float* c_e = clean + (size_t)b * row;
        int C = 0, Hh = 0;
        for (int t0 = 0; t0 < T; t0 += tpw) {
            const int t = t0 + tl;
            const bool valid = active && t < T;
            const int tc = valid ? t : 0, m = tc * n + j;
            long long v[SSD_MAX_AGENTS];
#pragma unroll
            for (int i = 0; i < SSD_MAX_AGENTS; ++i) v[i] = ai_e[tc * nn + (i < n ? i : j) * n + j];
            const long long a = a_e[m];
            const int r = valid ? beh_round(r_e[m]) : 0, c = valid ? beh_round(c_e[m]) : 0;
            int rv = 0;
#pragma unroll
            for (int i = 0; i < SSD_MAX_AGENTS; ++i) {
                const bool ok = valid && i < n && i != j;
                if (ok && (unsigned long long)v[i] < 3ull) beh_add(cnt, o_inc + (i * n + j) * 3 + (int)v[i], 1);
                rv += (ok && v[i] == 1) - (ok && v[i] == 2);
            }
            if (valid && (unsigned long long)a < (unsigned long long)A) beh_add(cnt, o_act + j * A + (int)a, 1);
            const int cl = c > 0, hv = r > 0;
            s_r += r; s_c += c; s_cl += cl; s_hv += hv; s_ht += hv ? t : 0;
            s_rc += cl ? rv : 0; s_rr += (long long)r * rv;
            C += cl; Hh += hv;
        }
        int Cs = 0, Hs = 0;                                            // lanes 0 .. n-1: the episode sums of agent `lane`
        for (int k = 0; k < tpw; ++k) {
            const int src = (lane + k * n) & 63;
            Cs += __shfl(C, src); Hs += __shfl(Hh, src);
        }
        const bool agent = lane < n, cleaner = agent && Cs > Hs;
        if (agent) beh_add(cnt, o_role + lane * 4 + ((Cs == 0 && Hs == 0) ? 0 : Cs > Hs ? 1 : Hs > Cs ? 2 : 3), 1);
        const int n_cleaners = __popcll(__ballot(cleaner));
        if (lane == 0) beh_add(cnt, o_hist + n_cleaners, 1);
        envs += 1;
    }
    if (active) {
        beh_add(cnt, j, s_r); beh_add(cnt, n + j, s_c); beh_add(cnt, 2 * n + j, s_cl); beh_add(cnt, 3 * n + j, s_hv); beh_add(cnt, 4 * n + j, s_ht);
        beh_add(cnt, o_rc + j, s_rc); beh_add(cnt, o_rc + n + j, s_rr);
    }
    if (lane == 0) { beh_add(cnt, o_ep, envs); beh_add(cnt, o_ep + 1, envs * T); }
    __syncthreads();
    for (int k = threadIdx.x; k < len; k += 64 * BEH_WAVES) ws[(size_t)blockIdx.x * len + k] = cnt[k];
}

__global__ __launch_bounds__(256) void k_behaviour_finish(const long long* __restrict__ ws, int groups, int len, double* __restrict__ acc) {
    for (int k = threadIdx.x; k < len; k += 256) {
        long long s = 0;
        for (int g = 0; g < groups; ++g) s += ws[(size_t)g * len + k];
        acc[k] += (double)s;
    }
}

void launch_behaviour_stats(const ssd_behaviour_args* a, hipStream_t stream) {
    int groups = a->n_env / BEH_WAVES + (a->n_env % BEH_WAVES ? 1 : 0);
    if (groups > SSD_BEHAVIOUR_MAX_GROUPS) groups = SSD_BEHAVIOUR_MAX_GROUPS;
    long long* ws = reinterpret_cast<long long*>(a->workspace);
    hipLaunchKernelGGL(k_behaviour_partials, dim3(groups), dim3(64 * BEH_WAVES), 0, stream, a->actions, a->actions_inc, a->reward, a->clean_num,
                       a->n_env, a->t_slots - 1, a->n_agents, a->n_actions, ws);
    hipLaunchKernelGGL(k_behaviour_finish, dim3(1), dim3(256), 0, stream, ws, groups, SSD_BEHAVIOUR_LEN(a->n_agents, a->n_actions), a->acc);
}

static int grid_for(size_t total);
// k_dueling_q: q = v + a - mean_k a per (agent, row) of the learner's time-batched heads, output in the batch layout [B, T, n, inner, K];
// BWD: da = dq - mean_k dq, dv = sum_k dq.  One thread per (agent, row); K <= 16.  ld: floats per row of a (and da); v / dv rows have the
// same stride when `merged` (advantages and value are columns 0..K-1 and K of ONE layer output [n, rows, K + 1]), else 1.
// gs (BWD, merged, nullable): the row-group sums of the gradient, gs[i, tb, 0..K] = sum over the `inner` rows of (i, tb) -- what the part
// of the layer input that is shared by the group (the incentive head's h_i under all receivers j) receives.
template <bool BWD>
__global__ __launch_bounds__(256) void k_dueling_q(const float* __restrict__ a, const float* __restrict__ v, float* __restrict__ q,
                                                   const float* __restrict__ dq, float* __restrict__ da, float* __restrict__ dv, int n, int T, int B,
                                                   int inner, int K, int ld, int merged, float* __restrict__ gs, const float* __restrict__ a_b,
                                                   const float* __restrict__ v_b, float* __restrict__ q_b, int n_a) {
    const long rows = (long)T * B * inner, total = rows * n;
    const int vld = merged ? ld : 1;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        int i = (int)(idx / rows);
        const long r = idx - (long)i * rows;
        const long tb = r / inner;
        const int j = (int)(r - tb * inner), t = (int)(tb / B), b = (int)(tb - (long)t * B);
        // !BWD, n_a > 0: a second group of sets (the target net's next to the live net's): sets i >= n_a are the sets 0 .. n - n_a - 1
        // of a_b / v_b / q_b
        const bool grp_b = !BWD && n_a && i >= n_a;
        const int ng = !BWD && n_a ? (grp_b ? n - n_a : n_a) : n;
        if (grp_b) i -= n_a;
        const size_t qo = ((((size_t)b * T + t) * ng + i) * inner + j) * K, ao = ((size_t)i * rows + r) * ld;
        float x[16], sum = 0.f;
        for (int k = 0; k < K; ++k) { x[k] = BWD ? dq[qo + k] : (grp_b ? a_b : a)[ao + k]; sum += x[k]; }
        if (BWD) {
            const float mean = sum / (float)K;
            for (int k = 0; k < K; ++k) da[ao + k] = x[k] - mean;
            dv[((size_t)i * rows + r) * vld] = sum;
            if (gs && j == 0) {                                        // this thread also adds the group's rows in order (deterministic)
                float g[17];
                for (int k = 0; k <= K; ++k) g[k] = 0.f;
                for (int jj = 0; jj < inner; ++jj) {
                    const size_t qj = qo + (size_t)jj * K;
                    float y[16], s2 = 0.f;
                    for (int k = 0; k < K; ++k) { y[k] = dq[qj + k]; s2 += y[k]; }
                    const float m2 = s2 / (float)K;
                    for (int k = 0; k < K; ++k) g[k] += y[k] - m2;
                    g[K] += s2;
                }
                float* go = gs + ((size_t)i * (rows / inner) + tb) * (K + 1);
                for (int k = 0; k <= K; ++k) go[k] = g[k];
            }
        } else {
            const float vv = (grp_b ? v_b : v)[((size_t)i * rows + r) * vld], mean = sum / (float)K;
            float* qg = grp_b ? q_b : q;
            for (int k = 0; k < K; ++k) qg[qo + k] = (vv + x[k]) - mean;              // v + a - mean(a), in the reference's order
        }
    }
}

void launch_dueling_q(const float* a, const float* v, float* q, const float* dq, float* da, float* dv, int n, int T, int B, int inner, int K,
                      hipStream_t stream, int ld, int merged, float* gs, const float* a_b, const float* v_b, float* q_b, int n_b) {
    // forward with a second group (a_b, v_b, q_b: n_b sets): the kernel sees n + n_b sets, the first n of them the first group's
    const int n_a = (!dq && n_b > 0) ? n : 0;
    if (n_a) n += n_b;
    const size_t total = (size_t)n * T * B * inner;
    if (ld <= 0) ld = K;
    if (dq) hipLaunchKernelGGL(k_dueling_q<true>, dim3(grid_for(total)), dim3(256), 0, stream, a, v, q, dq, da, dv, n, T, B, inner, K, ld, merged, gs, a_b, v_b, q_b, n_a);
    else hipLaunchKernelGGL(k_dueling_q<false>, dim3(grid_for(total)), dim3(256), 0, stream, a, v, q, dq, da, dv, n, T, B, inner, K, ld, merged, gs, a_b, v_b, q_b, n_a);
}

// k_gather_rows: rows ids[e] of up to SSD_COPY_BLOCKS_MAX fields into consecutive rows of their destinations (blockIdx.y = field,
// blockIdx.z = e); 4-byte accesses at any alignment for the bulk of a row, bytes for its tail.
struct GatherTable { ssd_row_gather f[SSD_COPY_BLOCKS_MAX]; };
typedef uint32_t u32_unaligned __attribute__((aligned(1)));
__global__ __launch_bounds__(256) void k_gather_rows(GatherTable t, const int64_t* __restrict__ ids) {
    const ssd_row_gather f = t.f[blockIdx.y];
    const uint8_t* src = static_cast<const uint8_t*>(f.src) + (size_t)ids[blockIdx.z] * f.row_bytes;
    uint8_t* dst = static_cast<uint8_t*>(f.dst) + (size_t)blockIdx.z * f.row_bytes;
    const long words = f.row_bytes >> 2;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < words; i += (long)gridDim.x * 256)
        *reinterpret_cast<u32_unaligned*>(dst + 4 * i) = *reinterpret_cast<const u32_unaligned*>(src + 4 * i);
    if (blockIdx.x == 0 && (long)threadIdx.x < (f.row_bytes & 3)) dst[4 * words + threadIdx.x] = src[4 * words + threadIdx.x];
}

void launch_gather_rows(const ssd_row_gather* fields, int count, const int64_t* ids, int n_ids, hipStream_t stream) {
    GatherTable t;
    int64_t most = 4;
    for (int i = 0; i < SSD_COPY_BLOCKS_MAX; ++i) {
        t.f[i] = fields[i < count ? i : 0];
        if (i < count && fields[i].row_bytes > most) most = fields[i].row_bytes;
    }
    int gx = (int)((most / 4 + 1023) / 1024);                             // 4 words per thread for the longest row
    if (gx < 1) gx = 1;
    if (gx > 32) gx = 32;
    hipLaunchKernelGGL(k_gather_rows, dim3(gx, count, n_ids), dim3(256), 0, stream, t, ids);
}

// k_sample_draw<S>: the one replay draw kernel (ssd_sample_ids: t0 null; ssd_sample_windows: t0 given).  ids: `count` distinct episode
// ids out of [0, population), uniformly, from a counter generator keyed by (seed, call) -- ReplayBuffer.sample's
// np.random.choice(replace = False) (episode_buffer.py:240-244) without a host draw or an H2D copy.  Floyd's subset sampling (a uniform
// count-subset with count draws, no population-sized permutation), then a Fisher-Yates pass over the count picks.  t0, where asked
// for: one window start per id from the draws the ids do not use, t0[e] = floor(draw(2 count + e) n_starts / 2^32) (include/ssd_hip.h);
// t0 is a kernel argument, so the branch on it is uniform, and with a null t0 no start is formed or written.
// One wave.  Every draw depends on its index alone, so the lanes form all of them first: the Floyd candidates t_i and the Fisher-Yates
// partners k_i go to LDS, the starts straight out.  What stays serial is the chain over the picks, and that runs in registers: pick
// s * 64 + l lives in p[s] of lane l (S = ceil(count / 64) slots, -1 while unset), "already picked" is S compares per lane and a
// ballot, a swap two readlanes and two predicated moves; the next step's t / k is fetched from LDS a step ahead.  (One thread walking
// the picks in LDS is no faster at 16 ids and takes 41 us at 64 ids and 118 us at 128: the compares are quadratic in count.)
__device__ __forceinline__ uint32_t sample_draw(uint32_t s0, uint32_t s1, uint32_t call, uint32_t i) {
    uint32_t x = s0 ^ (call * 0x9E3779B9u);
    x ^= x >> 17; x *= 0xed5ad4bbu; x ^= x >> 11; x *= 0xac4c1b51u; x ^= x >> 15; x *= 0x31848babu; x ^= x >> 14;
    x ^= s1 + i * 0x85EBCA6Bu;
    x ^= x >> 17; x *= 0xed5ad4bbu; x ^= x >> 11; x *= 0xac4c1b51u; x ^= x >> 15; x *= 0x31848babu; x ^= x >> 14;
    return x;
}
template <int S>
__global__ __launch_bounds__(64) void k_sample_draw(uint32_t s0, uint32_t s1, uint32_t call, int population, int count, int n_starts,
                                                    int64_t* __restrict__ ids, int64_t* __restrict__ t0) {
    __shared__ int32_t tv[SSD_SAMPLE_IDS_MAX], kv[SSD_SAMPLE_IDS_MAX];
    if (blockIdx.x != 0) return;
    const int lane = threadIdx.x;
    for (int i = lane; i < count; i += 64) {
        tv[i] = (int)(((uint64_t)sample_draw(s0, s1, call, (uint32_t)i) * (uint32_t)(population - count + i + 1)) >> 32);
        kv[i] = (int)(((uint64_t)sample_draw(s0, s1, call, (uint32_t)(count + i)) * (uint32_t)(i + 1)) >> 32);      // (kv[0] is never used)
        if (t0) t0[i] = (int64_t)(((uint64_t)sample_draw(s0, s1, call, (uint32_t)(2 * count + i)) * (uint32_t)n_starts) >> 32);
    }
    __syncthreads();
    int32_t p[S];
#pragma unroll
    for (int s = 0; s < S; ++s) p[s] = -1;
    int t = tv[0];
    for (int i = 0; i < count; ++i) {                                    // Floyd: pick[i] = t_i, or j = population - count + i if t_i is taken
        const int t_next = tv[i + 1 < count ? i + 1 : i];
        bool found = false;
#pragma unroll
        for (int s = 0; s < S; ++s) found |= p[s] == t;
        const int v = __ballot(found) ? population - count + i : t;
#pragma unroll
        for (int s = 0; s < S; ++s)
            if (s == (i >> 6) && lane == (i & 63)) p[s] = v;
        t = t_next;
    }
    int k = kv[count - 1];
    for (int i = count - 1; i > 0; --i) {                                // Fisher-Yates: swap(pick[i], pick[k_i])
        const int k_next = kv[i - 1];
        const int ku = __builtin_amdgcn_readfirstlane(k);
        int va = 0, vb = 0;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            va = s == (i >> 6) ? p[s] : va;
            vb = s == (ku >> 6) ? p[s] : vb;
        }
        const int a = __builtin_amdgcn_readlane(va, i & 63), b = __builtin_amdgcn_readlane(vb, ku & 63);
#pragma unroll
        for (int s = 0; s < S; ++s) {
            if (s == (i >> 6) && lane == (i & 63)) p[s] = b;
            if (s == (ku >> 6) && lane == (ku & 63)) p[s] = a;
        }
        k = k_next;
    }
#pragma unroll
    for (int s = 0; s < S; ++s)
        if (s * 64 + lane < count) ids[s * 64 + lane] = (int64_t)p[s];
}
void launch_sample_draw(uint64_t seed, uint32_t call, int population, int count, int n_starts, int64_t* ids, int64_t* t0, hipStream_t stream) {
    const uint32_t s0 = (uint32_t)seed, s1 = (uint32_t)(seed >> 32);
    if (count <= 64) hipLaunchKernelGGL(k_sample_draw<1>, dim3(1), dim3(64), 0, stream, s0, s1, call, population, count, n_starts, ids, t0);
    else if (count <= 128) hipLaunchKernelGGL(k_sample_draw<2>, dim3(1), dim3(64), 0, stream, s0, s1, call, population, count, n_starts, ids, t0);
    else if (count <= 256) hipLaunchKernelGGL(k_sample_draw<4>, dim3(1), dim3(64), 0, stream, s0, s1, call, population, count, n_starts, ids, t0);
    else hipLaunchKernelGGL(k_sample_draw<SSD_SAMPLE_IDS_MAX / 64>, dim3(1), dim3(64), 0, stream, s0, s1, call, population, count, n_starts, ids, t0);
}

// k_gather_windows: windows [t0[e], t0[e] + win_slots) of rows ids[e] of up to SSD_COPY_BLOCKS_MAX fields into consecutive rows of
// their destinations (ssd_gather_windows).  One 1-D grid: field f owns the workgroups [block0[f], block0[f + 1]).
// A copied field's destination is ONE dense byte range [dst, dst + n_ids W), W = win_slots slot_bytes, cut into the 16-byte-aligned
// granules of its absolute address.  A thread takes GATHER_UNROLL granules.  A granule that lies inside the range and inside one
// window is one 16-byte load at the source's alignment (t0 slot_bytes lands anywhere) and one aligned 16-byte store; the loads of a
// thread's granules are all issued before its first store.  The other granules -- the range's two ends, and wherever a window ends
// inside a granule (W = 2 for `terminated` at win_slots 2: eight windows per granule) -- go byte by byte, each byte from its own
// window.  Which way a granule goes depends on the launch's arguments only, never on ids or t0.
// The `filled` field goes by int64 slots: the load is unconditional and the burn-in rule a multiplication.
constexpr int GATHER_UNROLL = 2;
struct WindowField { const uint8_t* src; uint8_t* dst; int64_t slot_bytes; int32_t block0, filled; };
struct WindowTable { WindowField f[SSD_COPY_BLOCKS_MAX]; };
struct __attribute__((packed, aligned(1))) u128_unaligned { uint32_t v[4]; };
__global__ __launch_bounds__(256) void k_gather_windows(WindowTable t, int count, const int64_t* __restrict__ ids, const int64_t* __restrict__ t0,
                                                        int n_ids, int src_slots, int win_slots, int burn_in) {
    int fi = 0;
    for (int i = 1; i < count; ++i) fi = (int)blockIdx.x >= t.f[i].block0 ? i : fi;
    const WindowField f = t.f[fi];
    const int blk = (int)blockIdx.x - f.block0;
    if (f.filled) {
        const int64_t total = (int64_t)n_ids * win_slots;
        const int64_t i = (int64_t)blk * 256 + threadIdx.x;
        if (i < total) {
            const int e = (int)(i / win_slots), r = (int)(i - (int64_t)e * win_slots);
            const int64_t start = t0[e];
            const int64_t v = reinterpret_cast<const int64_t*>(f.src)[(ids[e] * src_slots + start) + r];
            reinterpret_cast<int64_t*>(f.dst)[i] = v * (int64_t)(r >= (start > 0 ? burn_in : 0));
        }
        return;
    }
    const uint64_t W = (uint64_t)win_slots * (uint64_t)f.slot_bytes, D = (uint64_t)n_ids * W;
    const uint64_t row = (uint64_t)src_slots * (uint64_t)f.slot_bytes;
    const uint64_t d0 = reinterpret_cast<uint64_t>(f.dst), dA = d0 & ~(uint64_t)15;
    const uint64_t granules = (d0 + D - dA + 15) >> 4;
    uint64_t first[GATHER_UNROLL], w[GATHER_UNROLL];
    const uint8_t* s[GATHER_UNROLL];
    int e[GATHER_UNROLL], len[GATHER_UNROLL];
    bool wide[GATHER_UNROLL];
#pragma unroll
    for (int u = 0; u < GATHER_UNROLL; ++u) {
        const uint64_t g = ((uint64_t)blk * GATHER_UNROLL + u) * 256 + threadIdx.x;
        const uint64_t lo = dA + (g << 4);
        uint64_t a = lo < d0 ? d0 : lo, b = lo + 16 < d0 + D ? lo + 16 : d0 + D;
        if (g >= granules) a = b = d0;                                   // past the field's last granule: nothing to do
        first[u] = a - d0;
        len[u] = (int)(b - a);
        const uint64_t o = len[u] > 0 ? first[u] : 0;
        e[u] = (int)(o / W);
        w[u] = o - (uint64_t)e[u] * W;
        wide[u] = len[u] == 16 && w[u] + 16 <= W;
    }
#pragma unroll
    for (int u = 0; u < GATHER_UNROLL; ++u)                              // e < n_ids always (o < D, or o = 0)
        s[u] = f.src + ((uint64_t)ids[e[u]] * row + (uint64_t)t0[e[u]] * (uint64_t)f.slot_bytes);
    u128_unaligned v[GATHER_UNROLL];
#pragma unroll
    for (int u = 0; u < GATHER_UNROLL; ++u)
        if (wide[u]) v[u] = *reinterpret_cast<const u128_unaligned*>(s[u] + w[u]);
#pragma unroll
    for (int u = 0; u < GATHER_UNROLL; ++u)
        if (wide[u]) *reinterpret_cast<uint4*>(f.dst + first[u]) = make_uint4(v[u].v[0], v[u].v[1], v[u].v[2], v[u].v[3]);
#pragma unroll
    for (int u = 0; u < GATHER_UNROLL; ++u) {
        if (wide[u] || len[u] <= 0) continue;
        int ee = e[u];
        uint64_t ww = w[u];
        const uint8_t* ss = s[u];
        for (int k = 0; k < len[u]; ++k) {
            f.dst[first[u] + k] = ss[ww];
            if (++ww == W && k + 1 < len[u]) {                           // the next byte opens window ee + 1 (< n_ids: it lies inside the range)
                ww = 0;
                ++ee;
                ss = f.src + ((uint64_t)ids[ee] * row + (uint64_t)t0[ee] * (uint64_t)f.slot_bytes);
            }
        }
    }
}
void launch_gather_windows(const ssd_window_field* fields, int count, const int64_t* ids, const int64_t* t0, int n_ids, int src_slots,
                           int win_slots, int burn_in, hipStream_t stream) {
    WindowTable t;
    int blocks = 0;
    for (int i = 0; i < SSD_COPY_BLOCKS_MAX; ++i) {
        const ssd_window_field& f = fields[i < count ? i : 0];
        t.f[i] = WindowField{static_cast<const uint8_t*>(f.src), static_cast<uint8_t*>(f.dst), f.slot_bytes, blocks, f.filled};
        if (i >= count) continue;
        const uint64_t D = (uint64_t)n_ids * (uint64_t)win_slots * (uint64_t)f.slot_bytes;
        // a copied field: its granules (one more when dst is not 16-byte aligned), GATHER_UNROLL per thread; `filled`: a slot per thread
        const uint64_t items = f.filled ? (uint64_t)n_ids * (uint64_t)win_slots : ((reinterpret_cast<uint64_t>(f.dst) & 15) + D + 15) >> 4;
        const uint64_t per_block = f.filled ? 256 : 256 * GATHER_UNROLL;
        blocks += (int)((items + per_block - 1) / per_block);
    }
    hipLaunchKernelGGL(k_gather_windows, dim3(blocks), dim3(256), 0, stream, t, count, ids, t0, n_ids, src_slots, win_slots, burn_in);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Prioritised replay (ssd_priority_sample / ssd_priority_update; the contract is in include/ssd_hip.h).
// k_priority_sample: one workgroup of 1024 threads.  Pass 1: the table's maximum (strided, coalesced).  Pass 2: thread t owns the
// contiguous chunk [t chunk, (t + 1) chunk), chunk = ceil(population / 1024), and adds its qeff in u64 (16-byte loads when the chunk
// is a multiple of four entries).  The 1024 chunk sums are scanned: six __shfl_up steps inside a wave, the sixteen wave totals
// through LDS, every thread adding the totals of the waves before its own in index order; the inclusive sums stay in LDS.  Thread
// e < count forms its stratum's x, finds the first chunk whose inclusive sum passes x by binary search and walks that chunk.  All
// sums are integers: nothing depends on an order.  x rises with e, so the ids are non-decreasing and "distinct" is a count of the
// places where neighbours differ.  The second and third reads of the table come from L2.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int PRI_THREADS = 1024;
__device__ __forceinline__ uint64_t pri_shfl_up(uint64_t v, int d) {
    const uint32_t lo = __shfl_up((uint32_t)v, d), hi = __shfl_up((uint32_t)(v >> 32), d);
    return ((uint64_t)hi << 32) | lo;
}
__global__ __launch_bounds__(PRI_THREADS) void k_priority_sample(ssd_priority_sample_args a) {
    __shared__ uint64_t s_cum[PRI_THREADS];
    __shared__ uint64_t s_wave[PRI_THREADS / 64];
    __shared__ uint32_t s_red[PRI_THREADS];
    __shared__ float s_w[PRI_THREADS];
    __shared__ int32_t s_id[PRI_THREADS];
    if (blockIdx.x != 0) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int P = a.population, count = a.count;
    const uint32_t* __restrict__ tab = a.table;
    // pass 1: qmax
    uint32_t m = 0;
    for (int k = tid; k < P; k += PRI_THREADS) { const uint32_t q = tab[k]; m = q > m ? q : m; }
    s_red[tid] = m;
    __syncthreads();
    for (int w = PRI_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) { const uint32_t o = s_red[tid + w]; if (o > s_red[tid]) s_red[tid] = o; }
        __syncthreads();
    }
    const uint32_t qmax = s_red[0] ? s_red[0] : SSD_PRIORITY_ONE;
    __syncthreads();
    // pass 2: chunk sums
    const int chunk = (P + PRI_THREADS - 1) / PRI_THREADS;
    const int k0 = tid * chunk < P ? tid * chunk : P, k1 = k0 + chunk < P ? k0 + chunk : P;
    uint64_t sum = 0;
    if ((chunk & 3) == 0 && (reinterpret_cast<uintptr_t>(tab) & 15) == 0) {       // k0 is a multiple of 4; so is k1, or it is P
        int k = k0;
        for (; k + 4 <= k1; k += 4) {
            const uint4 v = *reinterpret_cast<const uint4*>(tab + k);
            sum += (uint64_t)(v.x ? v.x : qmax) + (v.y ? v.y : qmax) + (v.z ? v.z : qmax) + (v.w ? v.w : qmax);
        }
        for (; k < k1; ++k) { const uint32_t q = tab[k]; sum += q ? q : qmax; }
    } else {
        for (int k = k0; k < k1; ++k) { const uint32_t q = tab[k]; sum += q ? q : qmax; }
    }
    // inclusive scan of the chunk sums
    uint64_t inc = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t o = pri_shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    uint64_t before = 0;
    for (int w = 0; w < wave; ++w) before += s_wave[w];
    s_cum[tid] = inc + before;
    __syncthreads();
    const uint64_t total = s_cum[PRI_THREADS - 1];
    // the draws
    const uint32_t s0 = (uint32_t)a.seed, s1 = (uint32_t)(a.seed >> 32);
    int id = 0;
    uint32_t qe = 0xFFFFFFFFu;
    if (tid < count) {
        const uint64_t lo = total * (uint64_t)tid / (uint64_t)count, hi = total * (uint64_t)(tid + 1) / (uint64_t)count;   // total < 2^44, tid + 1 <= 2^10
        const uint64_t width = hi - lo, d = sample_draw(s0, s1, a.call, (uint32_t)tid);
        const uint64_t x = lo + d * (width >> 32) + ((d * (width & 0xFFFFFFFFull)) >> 32);          // floor(d width / 2^32), exactly
        int c_lo = 0, c_hi = PRI_THREADS - 1;                                                      // s_cum[1023] = total > x
        while (c_lo < c_hi) {
            const int mid = (c_lo + c_hi) >> 1;
            if (s_cum[mid] > x) c_hi = mid; else c_lo = mid + 1;
        }
        uint64_t acc = c_lo ? s_cum[c_lo - 1] : 0;
        const int w0 = c_lo * chunk, w1 = w0 + chunk < P ? w0 + chunk : P;                           // s_cum[c_lo] > acc: the chunk is not empty
        id = w1 - 1;
        qe = qmax;
        for (int k = w0; k < w1; ++k) {
            const uint32_t q = tab[k], v = q ? q : qmax;
            acc += v;
            if (acc > x) { id = k; qe = v; break; }
        }
        a.ids[tid] = (int64_t)id;
        a.t0[tid] = (int64_t)(((uint64_t)sample_draw(s0, s1, a.call, (uint32_t)(2 * count + tid)) * (uint32_t)a.n_starts) >> 32);
    }
    // the smallest sampled qeff carries the largest weight
    s_id[tid] = id;
    s_red[tid] = qe;
    __syncthreads();
    for (int w = PRI_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) { const uint32_t o = s_red[tid + w]; if (o < s_red[tid]) s_red[tid] = o; }
        __syncthreads();
    }
    const uint32_t qmin = s_red[0];
    __syncthreads();
    float wgt = 2.f;
    if (tid < count) {
        wgt = (float)pow((double)qe / (double)qmin, -(double)a.beta);
        a.weights[tid] = wgt;
    }
    s_w[tid] = wgt;
    s_red[tid] = (tid > 0 && tid < count && id != s_id[tid - 1]) ? 1u : 0u;
    __syncthreads();
    for (int w = PRI_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) { s_w[tid] = fminf(s_w[tid], s_w[tid + w]); s_red[tid] += s_red[tid + w]; }
        __syncthreads();
    }
    if (tid == 0) {
        a.log[0] = (float)((double)total / (double)P / (double)SSD_PRIORITY_ONE);
        a.log[1] = (float)((double)qmax / (double)SSD_PRIORITY_ONE);
        a.log[2] = s_w[0];
        a.log[3] = (float)(1u + s_red[0]);
    }
}
// k_priority_sample_seq (n_segments >= 1): the table holds n_segments entries per slot; the same draw over entries, the drawn entry filed
// and mapped to (slot, window start) where k_priority_sample draws a uniform start.  A copy, not a second instantiation of a shared
// body: as a template the compiler commuted one add of k_priority_sample, and that kernel's instruction stream is kept as it was.
// Whatever changes above changes here.
__global__ __launch_bounds__(PRI_THREADS) void k_priority_sample_seq(ssd_priority_sample_args a) {
    __shared__ uint64_t s_cum[PRI_THREADS];
    __shared__ uint64_t s_wave[PRI_THREADS / 64];
    __shared__ uint32_t s_red[PRI_THREADS];
    __shared__ float s_w[PRI_THREADS];
    __shared__ int32_t s_id[PRI_THREADS];
    if (blockIdx.x != 0) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int P = a.population, count = a.count;
    const uint32_t* __restrict__ tab = a.table;
    // pass 1: qmax
    uint32_t m = 0;
    for (int k = tid; k < P; k += PRI_THREADS) { const uint32_t q = tab[k]; m = q > m ? q : m; }
    s_red[tid] = m;
    __syncthreads();
    for (int w = PRI_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) { const uint32_t o = s_red[tid + w]; if (o > s_red[tid]) s_red[tid] = o; }
        __syncthreads();
    }
    const uint32_t qmax = s_red[0] ? s_red[0] : SSD_PRIORITY_ONE;
    __syncthreads();
    // pass 2: chunk sums
    const int chunk = (P + PRI_THREADS - 1) / PRI_THREADS;
    const int k0 = tid * chunk < P ? tid * chunk : P, k1 = k0 + chunk < P ? k0 + chunk : P;
    uint64_t sum = 0;
    if ((chunk & 3) == 0 && (reinterpret_cast<uintptr_t>(tab) & 15) == 0) {       // k0 is a multiple of 4; so is k1, or it is P
        int k = k0;
        for (; k + 4 <= k1; k += 4) {
            const uint4 v = *reinterpret_cast<const uint4*>(tab + k);
            sum += (uint64_t)(v.x ? v.x : qmax) + (v.y ? v.y : qmax) + (v.z ? v.z : qmax) + (v.w ? v.w : qmax);
        }
        for (; k < k1; ++k) { const uint32_t q = tab[k]; sum += q ? q : qmax; }
    } else {
        for (int k = k0; k < k1; ++k) { const uint32_t q = tab[k]; sum += q ? q : qmax; }
    }
    // inclusive scan of the chunk sums
    uint64_t inc = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t o = pri_shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    uint64_t before = 0;
    for (int w = 0; w < wave; ++w) before += s_wave[w];
    s_cum[tid] = inc + before;
    __syncthreads();
    const uint64_t total = s_cum[PRI_THREADS - 1];
    // the draws
    const uint32_t s0 = (uint32_t)a.seed, s1 = (uint32_t)(a.seed >> 32);
    int id = 0;
    uint32_t qe = 0xFFFFFFFFu;
    if (tid < count) {
        const uint64_t lo = total * (uint64_t)tid / (uint64_t)count, hi = total * (uint64_t)(tid + 1) / (uint64_t)count;   // total < 2^44, tid + 1 <= 2^10
        const uint64_t width = hi - lo, d = sample_draw(s0, s1, a.call, (uint32_t)tid);
        const uint64_t x = lo + d * (width >> 32) + ((d * (width & 0xFFFFFFFFull)) >> 32);          // floor(d width / 2^32), exactly
        int c_lo = 0, c_hi = PRI_THREADS - 1;                                                      // s_cum[1023] = total > x
        while (c_lo < c_hi) {
            const int mid = (c_lo + c_hi) >> 1;
            if (s_cum[mid] > x) c_hi = mid; else c_lo = mid + 1;
        }
        uint64_t acc = c_lo ? s_cum[c_lo - 1] : 0;
        const int w0 = c_lo * chunk, w1 = w0 + chunk < P ? w0 + chunk : P;                           // s_cum[c_lo] > acc: the chunk is not empty
        id = w1 - 1;
        qe = qmax;
        for (int k = w0; k < w1; ++k) {
            const uint32_t q = tab[k], v = q ? q : qmax;
            acc += v;
            if (acc > x) { id = k; qe = v; break; }
        }
        const int64_t start = (int64_t)(id % a.n_segments) * a.seg_stride;
        a.entries[tid] = (int64_t)id;
        a.ids[tid] = (int64_t)(id / a.n_segments);
        a.t0[tid] = start < a.last_start ? start : (int64_t)a.last_start;
    }
    // the smallest sampled qeff carries the largest weight
    s_id[tid] = id;
    s_red[tid] = qe;
    __syncthreads();
    for (int w = PRI_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) { const uint32_t o = s_red[tid + w]; if (o < s_red[tid]) s_red[tid] = o; }
        __syncthreads();
    }
    const uint32_t qmin = s_red[0];
    __syncthreads();
    float wgt = 2.f;
    if (tid < count) {
        wgt = (float)pow((double)qe / (double)qmin, -(double)a.beta);
        a.weights[tid] = wgt;
    }
    s_w[tid] = wgt;
    s_red[tid] = (tid > 0 && tid < count && id != s_id[tid - 1]) ? 1u : 0u;
    __syncthreads();
    for (int w = PRI_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) { s_w[tid] = fminf(s_w[tid], s_w[tid + w]); s_red[tid] += s_red[tid + w]; }
        __syncthreads();
    }
    if (tid == 0) {
        a.log[0] = (float)((double)total / (double)P / (double)SSD_PRIORITY_ONE);
        a.log[1] = (float)((double)qmax / (double)SSD_PRIORITY_ONE);
        a.log[2] = s_w[0];
        a.log[3] = (float)(1u + s_red[0]);
    }
}
void launch_priority_sample(const ssd_priority_sample_args* a, hipStream_t stream) {
    if (a->n_segments) hipLaunchKernelGGL(k_priority_sample_seq, dim3(1), dim3(PRI_THREADS), 0, stream, *a);
    else hipLaunchKernelGGL(k_priority_sample, dim3(1), dim3(PRI_THREADS), 0, stream, *a);
}

// k_priority_rows: sample e = blockIdx.x.  Its T n rows of partials -> q_new[e]; then its blocks of dq_env / dq_inc times weights[e].
// pri_scale: the block [p, p + len) of floats, any 4-byte alignment: scalar elements up to the first 16-byte boundary, float4 in
// between, scalar elements behind the last whole float4.
__device__ __forceinline__ void pri_scale(float* __restrict__ p, size_t len, float w, int tid) {
    size_t head = ((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) >> 2;
    head = head < len ? head : len;
    const size_t body = (len - head) >> 2, tail0 = head + (body << 2);
    if ((size_t)tid < head) p[tid] *= w;
    float4* __restrict__ p4 = reinterpret_cast<float4*>(p + head);
    for (size_t k = tid; k < body; k += 256) {
        float4 v = p4[k];
        v.x *= w; v.y *= w; v.z *= w; v.w *= w;
        p4[k] = v;
    }
    if (tail0 + (size_t)tid < len) p[tail0 + tid] *= w;
}
__global__ __launch_bounds__(256) void k_priority_rows(ssd_priority_update_args a) {
    __shared__ float s_sum[256], s_cnt[256], s_max[256];
    const int e = blockIdx.x, tid = threadIdx.x;
    const int T1 = a.t_slots, n = a.n_agents, R = (T1 - 1) * n;
    const float* __restrict__ rows = a.partials + (size_t)e * R * SSD_TD_LOSS_PARTIALS;
    float sum = 0.f, cnt = 0.f, mx = 0.f;
    for (int r = tid; r < R; r += 256) {
        const float4 v = *reinterpret_cast<const float4*>(rows + (size_t)r * SSD_TD_LOSS_PARTIALS);     // columns 0 .. 3 (rows are 64 bytes)
        const float d = sqrtf(v.z + v.w);
        sum += d; cnt += v.x; mx = fmaxf(mx, d);
    }
    s_sum[tid] = sum; s_cnt[tid] = cnt; s_max[tid] = mx;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) { s_sum[tid] += s_sum[tid + w]; s_cnt[tid] += s_cnt[tid + w]; s_max[tid] = fmaxf(s_max[tid], s_max[tid + w]); }
        __syncthreads();
    }
    if (tid == 0) {
        const float p = a.eta * s_max[0] + (1.f - a.eta) * s_sum[0] / fmaxf(1.f, s_cnt[0]) + a.eps;
        float q = powf(p, a.alpha) * (float)SSD_PRIORITY_ONE;
        q = q == q ? q : (float)SSD_PRIORITY_MAX;
        a.q_new[e] = (uint32_t)rintf(fminf(fmaxf(q, 1.f), (float)SSD_PRIORITY_MAX));
    }
    const float w = a.weights[e];
    const size_t le = (size_t)T1 * n * a.n_actions, li = (size_t)T1 * n * n * 3;
    pri_scale(a.dq_env + (size_t)e * le, le, w, tid);
    pri_scale(a.dq_inc + (size_t)e * li, li, w, tid);
}
// k_priority_apply: one workgroup; thread e owns sample e (batch <= 1024).  One writer per table slot: the largest value, the
// smallest index among equals.
__global__ __launch_bounds__(PRI_THREADS) void k_priority_apply(ssd_priority_update_args a) {
    __shared__ int64_t s_id[PRI_THREADS];
    __shared__ uint32_t s_q[PRI_THREADS];
    if (blockIdx.x != 0) return;
    const int e = threadIdx.x, B = a.batch;
    int64_t id = -1;
    uint32_t q = 0;
    if (e < B) { id = a.ids[e]; q = a.q_new[e]; }
    s_id[e] = id; s_q[e] = q;
    __syncthreads();
    if (e >= B || id < 0 || id >= (int64_t)a.table_len) return;
    bool wins = true;
    for (int o = 0; o < B; ++o) {
        const uint32_t qo = s_q[o];
        if (s_id[o] == id && (qo > q || (qo == q && o < e))) wins = false;
    }
    if (wins) a.table[id] = q;
}
void launch_priority_update(const ssd_priority_update_args* a, hipStream_t stream) {
    hipLaunchKernelGGL(k_priority_rows, dim3(a->batch), dim3(256), 0, stream, *a);
    hipLaunchKernelGGL(k_priority_apply, dim3(1), dim3(PRI_THREADS), 0, stream, *a);
}

// k_rollout_priority (ssd_rollout_priority; the contract is in include/ssd_hip.h): the priority an episode enters the table with, from
// the rollout's own one-step TD errors, one launch per timestep slot behind the inc head.  16 lanes per env, four envs per wave, lane
// g & 15 = agent (n <= 10); a thread owns its (env, agent) pair's carry and acc.  At slot t it forms row t - 1 with the expressions
// and operation order of k_td_sim_loss<1> (plain branch, q = tq) and of k_priority_rows; at t = T the env's agents are reduced by
// __shfl reads of registers (every lane of the wave takes part, idle ones with zeros) and lane 0 of the env writes q_init.  Every
// lane walks its own row of A floats with scalar-width loads; in FastPolicy's agent-major layout the lanes of one env lie N A floats
// apart, so a wave touches about n segments of 4 A floats (the four envs' rows of one agent are neighbours) -- not a coalesced read.
// The launch reads ~0.5 KB per env and sits at the launch floor, so the access pattern was left at that.
__global__ __launch_bounds__(256) void k_rollout_priority(const ssd_rollout_priority_args a) {
    const int64_t t = *a.t_index;
    const int T1 = a.t_slots, T = T1 - 1, n = a.n_agents, A = a.n_actions;
    if (t < 0 || t > T) return;                                                 // (uniform over the launch)
    const int lane = threadIdx.x & 63, i = lane & 15, base = lane & 48;
    const int64_t env = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    const bool active = env < a.n_env && i < n;
    float mx = 0.f, sum = 0.f, cnt = 0.f;
    if (active) {
        const float* __restrict__ qe = a.q_env + (int64_t)i * a.q_env_agent_stride + env * a.q_env_env_stride;
        const float* __restrict__ qi = a.q_inc + (int64_t)i * a.q_inc_agent_stride + env * a.q_inc_env_stride;
        float* __restrict__ carry = a.carry + (env * n + i) * 2;
        float* __restrict__ acc = a.acc + (env * n + i) * 3;
        if (t > 0) {
            mx = acc[0]; sum = acc[1]; cnt = acc[2];
            const int64_t bt = env * T1 + (t - 1);                              // (env, slot t - 1)
            const float mask = (a.filled ? (float)a.filled[bt] : 1.f) * (t - 1 ? 1.f - (float)a.terminated[bt - 1] : 1.f);
            const int64_t* __restrict__ ainc = a.actions_inc + bt * n * n;      // [giver][receiver]
            int give = 0, rp = 0, rn = 0;
            for (int j = 0; j < n; ++j) {
                if (j == i) continue;
                give += ainc[(int64_t)i * n + j] != 0;
                const int64_t x = ainc[(int64_t)j * n + i];
                rp += x == 1; rn += x == 2;
            }
            const float r = a.reward[bt * n + i] / a.reward_scale;
            const float rv = (float)(rp - rn);
            const float r_env = (r + rv * a.incentive_ratio * a.incentive) / a.seq_len;
            const float r_inc = (r - (float)give * a.incentive_cost * a.incentive) / a.seq_len;
            const float live = 1.f - (float)a.terminated[bt];
            float v_env = -INFINITY;
            for (int k = 0; k < A; ++k) {
                const float q = (a.avail_bits >> k) & 1u ? qe[k] : kNeg;
                if (q > v_env) v_env = q;
            }
            float v_inc = 0.f;
            for (int j = 0; j < n; ++j) {
                if (j == i) continue;
                const float* s = qi + j * 3;
                v_inc += s[1] > s[0] ? (s[2] > s[1] ? s[2] : s[1]) : (s[2] > s[0] ? s[2] : s[0]);
            }
            const float td_env = carry[0] - (r_env + a.gamma_env * live * v_env);
            const float td_inc = carry[1] - (r_inc + a.gamma_inc * live * v_inc);
            const float d = sqrtf((td_env * mask) * (td_env * mask) + (td_inc * mask) * (td_inc * mask));
            mx = fmaxf(mx, d); sum += d; cnt += mask;
        }
        acc[0] = mx; acc[1] = sum; acc[2] = cnt;
        if (t < T) {
            const int64_t row = (env * T1 + t) * n + i;                         // (env, slot t, agent i)
            int64_t a_t = a.actions[row];
            a_t = a_t < 0 ? 0 : a_t >= A ? A - 1 : a_t;
            const int64_t* __restrict__ mine = a.actions_inc + row * n;
            float chosen = 0.f;
            for (int j = 0; j < n; ++j) {
                if (j == i) continue;
                int64_t c = mine[j];
                c = c < 0 ? 0 : c > 2 ? 2 : c;
                chosen += qi[j * 3 + c];
            }
            carry[0] = qe[a_t]; carry[1] = chosen;
        }
    }
    if (t < T) return;
    // t == T: the env's agents, lanes base .. base + n - 1 of this wave
    float m = mx;
    for (int w = 8; w > 0; w >>= 1) m = fmaxf(m, __shfl_xor(m, w));             // lanes n .. 15 hold 0 <= every d
    float s = 0.f, c = 0.f;
    for (int j = 0; j < n; ++j) { s += __shfl(sum, base + j); c += __shfl(cnt, base + j); }
    if (active && i == 0) {
        const float p = a.eta * m + (1.f - a.eta) * s / fmaxf(1.f, c) + a.eps;
        float q = powf(p, a.alpha) * (float)SSD_PRIORITY_ONE;
        q = q == q ? q : (float)SSD_PRIORITY_MAX;
        a.q_init[env] = (uint32_t)rintf(fminf(fmaxf(q, 1.f), (float)SSD_PRIORITY_MAX));
    }
}
// The per-window kernel's pieces.  rollout_priority_row / rollout_priority_carry / rollout_priority_value restate k_rollout_priority's
// row, carry and tail statement for statement (same expressions, same f32 operation order); k_rollout_priority itself keeps its text:
// routed through these functions its block layout changed, and that kernel's instruction stream is kept as it was.  Whatever changes
// above changes here.
// rollout_priority_row: d and mask of row t - 1 (t >= 1) of (env, agent i) from carry, slot t - 1 of the storage and this slot's Q.
__device__ __forceinline__ void rollout_priority_row(const ssd_rollout_priority_args& a, int64_t env, int i, int64_t t, const float* __restrict__ qe,
                                                     const float* __restrict__ qi, const float* carry, float& d, float& mask) {
    const int T1 = a.t_slots, n = a.n_agents, A = a.n_actions;
    const int64_t bt = env * T1 + (t - 1);                                      // (env, slot t - 1)
    mask = (a.filled ? (float)a.filled[bt] : 1.f) * (t - 1 ? 1.f - (float)a.terminated[bt - 1] : 1.f);
    const int64_t* __restrict__ ainc = a.actions_inc + bt * n * n;              // [giver][receiver]
    int give = 0, rp = 0, rn = 0;
    for (int j = 0; j < n; ++j) {
        if (j == i) continue;
        give += ainc[(int64_t)i * n + j] != 0;
        const int64_t x = ainc[(int64_t)j * n + i];
        rp += x == 1; rn += x == 2;
    }
    const float r = a.reward[bt * n + i] / a.reward_scale;
    const float rv = (float)(rp - rn);
    const float r_env = (r + rv * a.incentive_ratio * a.incentive) / a.seq_len;
    const float r_inc = (r - (float)give * a.incentive_cost * a.incentive) / a.seq_len;
    const float live = 1.f - (float)a.terminated[bt];
    float v_env = -INFINITY;
    for (int k = 0; k < A; ++k) {
        const float q = (a.avail_bits >> k) & 1u ? qe[k] : kNeg;
        if (q > v_env) v_env = q;
    }
    float v_inc = 0.f;
    for (int j = 0; j < n; ++j) {
        if (j == i) continue;
        const float* s = qi + j * 3;
        v_inc += s[1] > s[0] ? (s[2] > s[1] ? s[2] : s[1]) : (s[2] > s[0] ? s[2] : s[0]);
    }
    const float td_env = carry[0] - (r_env + a.gamma_env * live * v_env);
    const float td_inc = carry[1] - (r_inc + a.gamma_inc * live * v_inc);
    d = sqrtf((td_env * mask) * (td_env * mask) + (td_inc * mask) * (td_inc * mask));
}
// rollout_priority_carry: the Q-values of the actions the heads just filed in slot t (t < T), for the row the next launch forms.
__device__ __forceinline__ void rollout_priority_carry(const ssd_rollout_priority_args& a, int64_t env, int i, int64_t t, const float* __restrict__ qe,
                                                       const float* __restrict__ qi, float* carry) {
    const int n = a.n_agents, A = a.n_actions;
    const int64_t row = (env * a.t_slots + t) * n + i;                          // (env, slot t, agent i)
    int64_t a_t = a.actions[row];
    a_t = a_t < 0 ? 0 : a_t >= A ? A - 1 : a_t;
    const int64_t* __restrict__ mine = a.actions_inc + row * n;
    float chosen = 0.f;
    for (int j = 0; j < n; ++j) {
        if (j == i) continue;
        int64_t c = mine[j];
        c = c < 0 ? 0 : c > 2 ? 2 : c;
        chosen += qi[j * 3 + c];
    }
    carry[0] = qe[a_t]; carry[1] = chosen;
}
// rollout_priority_value: (max d, sum d, sum mask) of a set of rows -> the fixed-point priority (k_priority_rows' tail).
__device__ __forceinline__ uint32_t rollout_priority_value(const ssd_rollout_priority_args& a, float m, float s, float c) {
    const float p = a.eta * m + (1.f - a.eta) * s / fmaxf(1.f, c) + a.eps;
    float q = powf(p, a.alpha) * (float)SSD_PRIORITY_ONE;
    q = q == q ? q : (float)SSD_PRIORITY_MAX;
    return (uint32_t)rintf(fminf(fmaxf(q, 1.f), (float)SSD_PRIORITY_MAX));
}
// k_rollout_priority_seq (n_segments = S >= 1): a priority per window of the stride grid.  The same lanes, rows and carry; acc is
// [N, n, S, 3] and row t - 1 goes into the accumulators of the windows whose loss rows contain it -- k from the first window that
// still reaches the row to the last that has started, each tested (the clamped last window is off the stride) -- and into no other.
// At t == T every window's accumulators are read back by the thread that wrote them and reduced over the agents as above.
__global__ __launch_bounds__(256) void k_rollout_priority_seq(const ssd_rollout_priority_args a) {
    const int64_t t = *a.t_index;
    const int T = a.t_slots - 1, n = a.n_agents, S = a.n_segments, L = a.win_len, st = a.seg_stride, last = T - L;
    if (t < 0 || t > T) return;                                                 // (uniform over the launch)
    const int lane = threadIdx.x & 63, i = lane & 15, base = lane & 48;
    const int64_t env = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    const bool active = env < a.n_env && i < n;
    float* acc = a.acc + (env * n + i) * (int64_t)S * 3;                        // (dereferenced by active lanes only)
    if (active) {
        const float* __restrict__ qe = a.q_env + (int64_t)i * a.q_env_agent_stride + env * a.q_env_env_stride;
        const float* __restrict__ qi = a.q_inc + (int64_t)i * a.q_inc_agent_stride + env * a.q_inc_env_stride;
        float* carry = a.carry + (env * n + i) * 2;
        if (t == 0) {
            for (int k = 0; k < S * 3; ++k) acc[k] = 0.f;
        } else {
            float d, mask;
            rollout_priority_row(a, env, i, t, qe, qi, carry, d, mask);
            const int row = (int)t - 1;
            const int k_lo = row < L ? 0 : (row - L) / st + 1;                  // the smallest k with k st + L > row
            const int k_hi = row / st + 1 < S - 1 ? row / st + 1 : S - 1;       // no later window has started (the last one may be clamped back)
            for (int k = k_lo; k <= k_hi; ++k) {
                const int start = k * st < last ? k * st : last;
                if (row < start + (start > 0 ? a.burn_in : 0) || row >= start + L) continue;
                float* w = acc + k * 3;
                w[0] = fmaxf(w[0], d); w[1] += d; w[2] += mask;
            }
        }
        if (t < T) rollout_priority_carry(a, env, i, t, qe, qi, carry);
    }
    if (t < T) return;
    for (int k = 0; k < S; ++k) {                                               // (uniform: every lane of the wave takes part)
        float mx = 0.f, sum = 0.f, cnt = 0.f;
        if (active) { mx = acc[k * 3]; sum = acc[k * 3 + 1]; cnt = acc[k * 3 + 2]; }
        float m = mx;
        for (int w = 8; w > 0; w >>= 1) m = fmaxf(m, __shfl_xor(m, w));
        float s = 0.f, c = 0.f;
        for (int j = 0; j < n; ++j) { s += __shfl(sum, base + j); c += __shfl(cnt, base + j); }
        if (active && i == 0) a.q_init[env * S + k] = rollout_priority_value(a, m, s, c);
    }
}
void launch_rollout_priority(const ssd_rollout_priority_args* a, hipStream_t stream) {
    const dim3 grid((unsigned)((a->n_env + 15) / 16));
    if (a->n_segments) hipLaunchKernelGGL(k_rollout_priority_seq, grid, dim3(256), 0, stream, *a);
    else hipLaunchKernelGGL(k_rollout_priority, grid, dim3(256), 0, stream, *a);
}

void launch_copy_blocks(const ssd_block_copy* blocks, int count, hipStream_t stream) {
    CopyTable t;
    int most = 1;
    for (int i = 0; i < SSD_COPY_BLOCKS_MAX; ++i) {
        t.e[i] = blocks[i < count ? i : 0];
        if (i < count && blocks[i].rows * blocks[i].cols > most) most = blocks[i].rows * blocks[i].cols;
    }
    int gx = (most + 1023) / 1024;                                     // 4 elements per thread for the largest block
    if (gx > 64) gx = 64;
    hipLaunchKernelGGL(k_copy_blocks, dim3(gx, count), dim3(256), 0, stream, t);
}

// ---------------------------------------------------------------------------------------------------------------------------
// k_gradsq_partials / k_clip_adam: both gradient clips and both Adam steps of the learner over the flat gradient buffer
// (include/ssd_hip.h: ssd_clip_adam_step; homophily_learner.py:223-226).  1024 elements per workgroup, 4 per thread.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int ADAM_CHUNK = 1024;
// What the two Adam launches read of ssd_clip_adam_args: the members before polyak_jobs, at their offsets.  They take THIS by value, so
// members appended to the public struct leave their kernel-argument segment (and `chunks` behind it) where it was.
struct ClipAdamCore {
    float* flat_grad;
    int64_t total;
    const ssd_adam_job* jobs;
    int32_t n_jobs;
    float* partials;
    float lr_inc, lr_env, beta1, beta2, eps, clip;
};
static_assert(sizeof(ClipAdamCore) == offsetof(ssd_clip_adam_args, polyak_jobs) && offsetof(ClipAdamCore, partials) == offsetof(ssd_clip_adam_args, partials) &&
              offsetof(ClipAdamCore, lr_inc) == offsetof(ssd_clip_adam_args, lr_inc) && offsetof(ClipAdamCore, clip) == offsetof(ssd_clip_adam_args, clip),
              "ClipAdamCore is the head of ssd_clip_adam_args");
__device__ __forceinline__ float block_sum_256(float v, float* red) {      // fixed-order tree over 256 threads
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

// job (parameter tensor) of flat element `base`, given the ascending first elements j_off[0 .. n_jobs]
__device__ __forceinline__ int adam_job_of(const long* j_off, int n_jobs, long base) {
    int lo = 0, hi = n_jobs - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (j_off[mid] <= base) lo = mid; else hi = mid - 1; }
    return lo;
}

__global__ __launch_bounds__(256) void k_gradsq_partials(ClipAdamCore a) {
    __shared__ float red[256];
    __shared__ long j_off[SSD_ADAM_MAX_JOBS + 1];
    __shared__ int j_seg[SSD_ADAM_MAX_JOBS];
    if ((int)threadIdx.x < a.n_jobs) {
        const ssd_adam_job j = a.jobs[threadIdx.x];
        j_off[threadIdx.x] = j.offset; j_seg[threadIdx.x] = j.segment;
        if ((int)threadIdx.x == a.n_jobs - 1) j_off[a.n_jobs] = j.offset + j.numel;
    }
    __syncthreads();
    const long base = (long)blockIdx.x * ADAM_CHUNK + threadIdx.x * 4;
    float s[3] = {0.f, 0.f, 0.f};
    if (base < a.total) {
        int job = adam_job_of(j_off, a.n_jobs, base);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long i = base + r;
            if (i < a.total) {
                while (i >= j_off[job + 1]) ++job;
                const float g = a.flat_grad[i];
                const float gg = g * g;
                const int seg = j_seg[job];
                s[0] += seg == 0 ? gg : 0.f; s[1] += seg == 1 ? gg : 0.f; s[2] += seg == 2 ? gg : 0.f;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float v = block_sum_256(s[k], red);
        if (threadIdx.x == 0) a.partials[(size_t)blockIdx.x * 3 + k] = v;
    }
    if (blockIdx.x == 0 && (int)threadIdx.x < a.n_jobs) {                   // step counters (read by the second launch only)
        const ssd_adam_job j = a.jobs[threadIdx.x];
        if (j.step[0]) *j.step[0] += 1.f;
        if (j.step[1]) *j.step[1] += 1.f;
    }
}

__global__ __launch_bounds__(256) void k_clip_adam(ClipAdamCore a, int chunks) {
    __shared__ float red[256];
    __shared__ long j_off[SSD_ADAM_MAX_JOBS + 1];
    __shared__ float j_size[SSD_ADAM_MAX_JOBS][2], j_rsq[SSD_ADAM_MAX_JOBS][2];   // lr / (1 - b1^t), 1 / sqrt(1 - b2^t) per optimiser
    const int t = threadIdx.x;
    float S[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {                                          // the chunk sums in a fixed order
        float v = 0.f;
        for (int c = t; c < chunks; c += 256) v += a.partials[(size_t)c * 3 + k];
        S[k] = block_sum_256(v, red);
    }
    // torch.clamp(clip_coef, max = 1) keeps a NaN coefficient (clip_grad_norm_ then spreads it over every gradient of the group);
    // fminf alone would return 1 and hide a non-finite norm
    const float r_inc = a.clip / (sqrtf(S[0] + S[2]) + 1e-6f);
    const float c_inc = r_inc != r_inc ? r_inc : fminf(1.f, r_inc);
    const float r_env = a.clip / (sqrtf(c_inc * c_inc * S[0] + S[1]) + 1e-6f);
    const float c_env = r_env != r_env ? r_env : fminf(1.f, r_env);
    if (t < a.n_jobs) {
        const ssd_adam_job j = a.jobs[t];
        j_off[t] = j.offset;
        if (t == a.n_jobs - 1) j_off[a.n_jobs] = j.offset + j.numel;
#pragma unroll
        for (int o = 0; o < 2; ++o) {
            const float st = j.step[o] ? *j.step[o] : 1.f;
            const float bc1 = (float)(1.0 - pow((double)a.beta1, (double)st)), bc2 = (float)(1.0 - pow((double)a.beta2, (double)st));
            j_size[t][o] = (o == 0 ? a.lr_inc : a.lr_env) / bc1;
            j_rsq[t][o] = sqrtf(bc2);
        }
    }
    __syncthreads();
    const long base = (long)blockIdx.x * ADAM_CHUNK + t * 4;
    if (base >= a.total) return;
    int job = adam_job_of(j_off, a.n_jobs, base);
    const float w1 = 1.f - a.beta1, w2 = 1.f - a.beta2;
    for (int r = 0; r < 4; ++r) {
        const long i = base + r;
        if (i >= a.total) break;
        while (i >= j_off[job + 1]) ++job;
        const ssd_adam_job j = a.jobs[job];
        const long e = i - j.offset;
        float g = a.flat_grad[i];
        g = j.segment == 0 ? (g * c_inc) * c_env : (j.segment == 1 ? g * c_env : g * c_inc);   // clip inc first, then env
        a.flat_grad[i] = g;
        float p = j.param[e];
#pragma unroll
        for (int o = 0; o < 2; ++o) {                                      // optimiser_inc.step(), then optimiser_env.step()
            if (!j.exp_avg[o]) continue;
            float m = j.exp_avg[o][e], v = j.exp_avg_sq[o][e];
            m = m + w1 * (g - m);                                          // lerp(m, g, 1 - beta1)
            v = a.beta2 * v + (w2 * g) * g;
            j.exp_avg[o][e] = m; j.exp_avg_sq[o][e] = v;
            const float denom = sqrtf(v) / j_rsq[job][o] + a.eps;
            p -= (j_size[job][o] * m) / denom;
        }
        j.param[e] = p;
    }
}

// k_polyak: the Polyak target update behind the Adam launch (include/ssd_hip.h: ssd_clip_adam_step, "Polyak target update").  All jobs
// in one launch of SSD_POLYAK_WORKGROUPS workgroups: the jobs' element counts are scanned in LDS (the table is device memory: the host
// cannot size a grid by it), a workgroup owns one contiguous range of the concatenated element space, a thread strides it by 256.
__global__ __launch_bounds__(256) void k_polyak(const ssd_polyak_job* __restrict__ jobs, int n_jobs, float tau, float c, float* __restrict__ partials) {
    __shared__ float red[256];
    __shared__ long scan[2][SSD_POLYAK_MAX_JOBS];
    __shared__ long j_off[SSD_POLYAK_MAX_JOBS + 1];
    __shared__ ssd_polyak_job j_tab[SSD_POLYAK_MAX_JOBS];
    const int t = threadIdx.x;
    if (t < SSD_POLYAK_MAX_JOBS) {
        long cnt = 0;
        if (t < n_jobs) {
            const ssd_polyak_job j = jobs[t];
            j_tab[t] = j;
            const long e = (long)j.rows * (long)j.cols;
            if (j.rows >= 1 && j.cols >= 1 && j.dst_row_stride >= (int64_t)j.cols && e < (1l << 31)) cnt = e;     // else: skipped
        }
        scan[0][t] = cnt;
    }
    __syncthreads();
    int cur = 0;
    for (int s = 1; s < SSD_POLYAK_MAX_JOBS; s <<= 1) {                      // inclusive scan of the counts (Hillis-Steele, 7 rounds)
        if (t < SSD_POLYAK_MAX_JOBS) scan[cur ^ 1][t] = scan[cur][t] + (t >= s ? scan[cur][t - s] : 0);
        cur ^= 1;
        __syncthreads();
    }
    if (t < n_jobs) j_off[t + 1] = scan[cur][t];
    if (t == 0) j_off[0] = 0;
    __syncthreads();
    const long total = j_off[n_jobs];
    const long per = ((total + 256l * SSD_POLYAK_WORKGROUPS - 1) / (256l * SSD_POLYAK_WORKGROUPS)) * 256l;
    const long begin = (long)blockIdx.x * per;
    const long end = begin + per < total ? begin + per : total;
    float s_gap = 0.f, s_live = 0.f;
    long i = begin + t;
    if (i < end) {
        int job = 0, hi = n_jobs - 1;                                      // the last job whose first element is <= i
        while (job < hi) { const int mid = (job + hi + 1) >> 1; if (j_off[mid] <= i) job = mid; else hi = mid - 1; }
        for (; i < end; i += 256) {
            while (i >= j_off[job + 1]) ++job;                             // (i < total = j_off[n_jobs]: stops at a job that holds i)
            const uint32_t e = (uint32_t)(i - j_off[job]);
            const uint32_t cols = (uint32_t)j_tab[job].cols;
            const bool whole = j_tab[job].dst_row_stride == (int64_t)cols;
            float* d = j_tab[job].dst + (whole ? (size_t)e : (size_t)(e / cols) * (size_t)j_tab[job].dst_row_stride + (e % cols));
            const float l = j_tab[job].src[e];
            const float a = *d * c, b = l * tau;                           // three roundings (the library is built without contraction)
            const float v = a + b;
            *d = v;
            if (whole) { const float g = l - v; s_gap += g * g; s_live += l * l; }
        }
    }
    if (partials) {
        const float g = block_sum_256(s_gap, red), w = block_sum_256(s_live, red);
        if (t == 0) { partials[(size_t)blockIdx.x * 2] = g; partials[(size_t)blockIdx.x * 2 + 1] = w; }
    }
}

void launch_clip_adam(const ssd_clip_adam_args* a, hipStream_t stream) {
    const int chunks = (int)((a->total + ADAM_CHUNK - 1) / ADAM_CHUNK);
    ClipAdamCore core;
    core.flat_grad = a->flat_grad; core.total = a->total; core.jobs = a->jobs; core.n_jobs = a->n_jobs; core.partials = a->partials;
    core.lr_inc = a->lr_inc; core.lr_env = a->lr_env; core.beta1 = a->beta1; core.beta2 = a->beta2; core.eps = a->eps; core.clip = a->clip;
    hipLaunchKernelGGL(k_gradsq_partials, dim3(chunks), dim3(256), 0, stream, core);
    hipLaunchKernelGGL(k_clip_adam, dim3(chunks), dim3(256), 0, stream, core, chunks);
    if (a->n_polyak > 0) {
        const float c = 1.f - a->target_tau;
        hipLaunchKernelGGL(k_polyak, dim3(SSD_POLYAK_WORKGROUPS), dim3(256), 0, stream, a->polyak_jobs, (int)a->n_polyak, a->target_tau, c, a->polyak_partials);
    }
}

static int grid_for(size_t total) {
    size_t b = (total + 255) / 256;
    return (int)(b < 1 ? 1 : b > 4096 ? 4096 : b);
}

void launch_build_inputs(int32_t batch, int32_t n, int32_t A, int32_t t0, const int64_t* last_actions,
                         const float* last_reward, const int64_t* last_actions_inc, const float* pos, float pos_scale,
                         float* out, int32_t out_stride, int32_t out_offset, hipStream_t stream) {
    const size_t total = (size_t)batch * n * (A + n + 4);
    hipLaunchKernelGGL(k_build_inputs, dim3(grid_for(total)), dim3(256), 0, stream, batch * n, n, A, t0, last_actions,
                       last_reward, last_actions_inc, pos, pos_scale, out, out_stride, out_offset);
}

void launch_build_inputs_flags(int32_t batch, int32_t n, int32_t A, int32_t t0, uint32_t input_flags, const int64_t* last_actions,
                               const float* last_reward, const int64_t* last_actions_inc, const float* pos, float pos_scale,
                               float* out, int32_t out_stride, int32_t out_offset, hipStream_t stream) {
    const BuildInputsLayout L = build_inputs_layout(n, A, input_flags);
    if (L.width < 1) return;                                            // no tail blocks at all
    const size_t total = (size_t)batch * n * L.width;
    hipLaunchKernelGGL(k_build_inputs_flags, dim3(grid_for(total)), dim3(256), 0, stream, batch * n, n, A, t0, L, last_actions,
                       last_reward, last_actions_inc, pos, pos_scale, out, out_stride, out_offset);
}

// other_j = [one-hot(a_j), pos_j / scale, orient_j, r_j, clean_j, apple_den_j] (homophily_agent.py:194-201) of every (episode b, step t,
// agent j) as other [T * B, n, A + 7] (rows t * B + b: the layout the time-batched incentive head consumes), and the one-hot alone a
// second time as act_tm [n, T * B, A] (agent-major: the extra input columns of fc1_inc).  One thread per (b, t, j): the reference
// builds this from F.one_hot, a division, a concatenation and two permuted copies -- six launches here, plus two per network for act_tm.
__global__ __launch_bounds__(256) void k_unroll_other(const int64_t* __restrict__ actions, const float* __restrict__ pos, const float* __restrict__ orient,
                                                      const float* __restrict__ reward, const float* __restrict__ clean, const float* __restrict__ den,
                                                      float pos_scale, int B, int T, int n, int A, float* __restrict__ other, float* __restrict__ act_tm) {
    const int it = blockIdx.x * 256 + threadIdx.x;
    if (it >= B * T * n) return;
    const int j = it % n, bt = it / n, t = bt % T, b = bt / T;
    const int a = (int)actions[it];
    const int E = A + 7;
    float* o = other + ((size_t)(t * B + b) * n + j) * E;
    float* at = act_tm + ((size_t)j * T * B + (size_t)t * B + b) * A;
    for (int k = 0; k < A; ++k) { const float v = k == a ? 1.f : 0.f; o[k] = v; at[k] = v; }
    o[A] = pos[(size_t)it * 2] / pos_scale; o[A + 1] = pos[(size_t)it * 2 + 1] / pos_scale;
    o[A + 2] = orient[(size_t)it * 2]; o[A + 3] = orient[(size_t)it * 2 + 1];
    o[A + 4] = reward[it]; o[A + 5] = clean[it]; o[A + 6] = den[it];
}
void launch_unroll_other(const int64_t* actions, const float* pos, const float* orient, const float* reward, const float* clean, const float* den,
                         float pos_scale, int B, int T, int n, int A, float* other, float* act_tm, hipStream_t stream) {
    const int total = B * T * n;
    hipLaunchKernelGGL(k_unroll_other, dim3((total + 255) / 256), dim3(256), 0, stream, actions, pos, orient, reward, clean, den, pos_scale, B, T, n, A, other, act_tm);
}

void launch_incentive_transfer(int32_t B, int32_t T, int32_t n, const int64_t* a_inc, const float* rewards,
                               float effect_ratio, float cost_ratio, float incentive, float seq_len, float* give,
                               float* recv_pos, float* recv_neg, float* recv_zero, float* r_env, float* r_inc,
                               hipStream_t stream) {
    const size_t total = (size_t)B * T * n;
    hipLaunchKernelGGL(k_incentive_transfer, dim3(grid_for(total)), dim3(256), 0, stream, B, T, n, a_inc, rewards,
                       effect_ratio, cost_ratio, incentive, seq_len, give, recv_pos, recv_neg, recv_zero, r_env, r_inc);
}

// Two deterministic stages when there are many rows: chunks of COLSUM_CHUNK rows -> workspace [G, chunks, C] -> out [G, C].
void launch_column_sums(const float* x, float* out, int G, int R, int C, float* workspace, hipStream_t stream) {
    const int chunks = (R + SSD_COLSUM_CHUNK - 1) / SSD_COLSUM_CHUNK;
    if (chunks <= 1 || !workspace) {
        hipLaunchKernelGGL(k_column_sums, dim3((C + 63) / 64, G, 1), dim3(256), 0, stream, x, out, R, C, R);
        return;
    }
    hipLaunchKernelGGL(k_column_sums, dim3((C + 63) / 64, G, chunks), dim3(256), 0, stream, x, workspace, R, C, SSD_COLSUM_CHUNK);
    hipLaunchKernelGGL(k_column_sums, dim3((C + 63) / 64, G, 1), dim3(256), 0, stream, workspace, out, chunks, C, chunks);
}

void launch_td_sim_loss(const ssd_td_loss_args* a, int mode, hipStream_t stream) {
    const int total = a->batch * a->t_slots * a->n_agents;
    const dim3 grid((total + 127) / 128), block(128);
    if (mode && a->td_lambda > 0.f) hipLaunchKernelGGL(k_td_lambda_loss, dim3(a->batch * a->n_agents), dim3(256), 0, stream, *a);
    else if (mode) hipLaunchKernelGGL(k_td_sim_loss<1>, grid, block, 0, stream, *a);
    else hipLaunchKernelGGL(k_td_sim_loss<0>, grid, block, 0, stream, *a);
}

}  // namespace ssd
