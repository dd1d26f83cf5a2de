/* ssd_hip_train.h -- the entry points of libssd_hip.so that serve the learner's train step alone: launches shared by the live and the
 * target net, and the row assembly in front of fc1.  A companion of ssd_hip.h (types, status codes, ssd_last_error, the ABI version:
 * all there); mirrored by homophily_marl_amd/abi.py: TRAIN_SIGNATURES.  Every function returns an ssd_status. */
#ifndef SSD_HIP_TRAIN_H
#define SSD_HIP_TRAIN_H

#include "ssd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Two operand groups of one layer shape in ONE launch each (the learner evaluates its live and its target net on the same batch: the
 * same layer twice, on independent operands).  Group a has n_a weight sets, group b n_b; rows, widths and flags are shared.  Every set
 * is computed by the kernel, and with the arithmetic, of the single launch, so each output equals the single launch's bit for bit.
 *   ssd_bias_bmm_pair_fwd      in2 == 0 (x2_a, x2_b NULL): y = b + x w as ssd_bias_bmm_fwd, or ssd_bias_bmm_leaky_fwd with leaky != 0.
 *                              in2 > 0: the two-source rows of ssd_bias_bmm2_fwd, and in1 may be any width when in2 is no multiple of 4
 *                              (the per-element loads select the source per column).
 *   ssd_dueling_head_pair_fwd  ssd_dueling_head_fwd of y_a [n_a, ...] -> q_a [B, T, n_a, inner, K] and y_b [n_b, ...] -> q_b.
 * SSD_ERR_INVALID: a NULL operand of either group, a set count below 1 (a second group always comes with its count; one group alone
 * is the single launch), a second source without in2 or the reverse. */
int ssd_bias_bmm_pair_fwd(const float* x_a, const float* x2_a, const float* w_a, const float* b_a, float* y_a, int32_t n_a, const float* x_b,
                          const float* x2_b, const float* w_b, const float* b_b, float* y_b, int32_t n_b, int32_t rows, int32_t in1, int32_t in2,
                          int32_t out, int32_t x1_div, int32_t x2_shared, int32_t leaky, void* stream);
int ssd_dueling_head_pair_fwd(const float* y_a, float* q_a, int32_t n_a, const float* y_b, float* q_b, int32_t n_b, int32_t T, int32_t B, int32_t inner,
                              int32_t K, void* stream);
/* fc1's input rows of the learner's time-batched evaluation, assembled where the two fc1 layers read them (csrc/ssd_train_rows.hip):
 *   ssd_fc1_rows_fwd  feat_a f32 [B * T * n, feat_w] (rows (b * T + t) * n + i: the encoder's output), tail f32 [B * T * n, tail_w] (the
 *                     non-visual input columns, same rows; NULL with tail_w 0), act f32 [n, T * B, act_w] (the one-hot actions, rows
 *                     t * B + b) -> x_env_a [n, T * B, feat_w + tail_w] = [feat | tail] and x_inc_a [n, T * B, feat_w + tail_w + act_w] =
 *                     [feat | tail | act], rows t * B + b.  feat_b, x_env_b, x_inc_b (all three or none): the same for a second net on the
 *                     same tail and act, in the same launch.
 *   ssd_fc1_rows_bwd  d_feat [B * T * n, feat_w] = d_x_env[.., :feat_w] + d_x_inc[.., :feat_w], in feat's row order, rows d_feat_stride >= feat_w
 *                     floats apart (the leading columns of wider rows: the layout of a concatenation's sliced gradient).
 * Copies and one addition of two values: no rounding differs from the tensor operations'. */
int ssd_fc1_rows_fwd(const float* feat_a, const float* feat_b, const float* tail, const float* act, float* x_env_a, float* x_inc_a, float* x_env_b,
                     float* x_inc_b, int32_t B, int32_t T, int32_t n, int32_t feat_w, int32_t tail_w, int32_t act_w, void* stream);
int ssd_fc1_rows_bwd(const float* d_x_env, const float* d_x_inc, float* d_feat, int32_t B, int32_t T, int32_t n, int32_t feat_w, int32_t tail_w, int32_t act_w,
                     int32_t d_feat_stride, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSD_HIP_TRAIN_H */
