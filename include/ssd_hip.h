/*
 * ssd_hip.h -- C ABI of the MI355X-native vectorised SSD (Cleanup / Harvest) grid world.
 *
 * This is the drop-in boundary for the hot path of drdh/Homophily-MARL.  The reference has no FFI at all:
 * its env is reached through Python duck-typing (src/envs/__init__.py:6-11, src/envs/multiagentenv.py:8-75).
 * Every entry point below therefore cites the reference *Python* interface it replaces; the host-side
 * mirror of that interface lives in homophily_marl_amd/envs/ and calls these symbols through ctypes.
 *
 * Conventions
 *   - return 0 on success, a negative ssd_status otherwise; the message is in ssd_last_error() (thread local).
 *   - no C++ exception crosses this boundary, nothing aborts.
 *   - the caller owns every in/out array (device pointers for ssd_*, host pointers for the oracle's
 *     ssd_cpu_* mirror); the library owns only the opaque handle.
 *   - all GPU entry points are asynchronous on the hipStream_t passed as `void* stream` (0 = null stream).
 *   - one handle = one device; calls on one handle are not re-entrant.
 *
 * Cell alphabet of the world grid (u8 codes): 0 ' ', 1 '@', 2 'A', 3 'H', 4 'R', 5 'S'
 * (src/envs/ssd/map_env.py:132,817-820; src/envs/ssd/cleanup.py:117-124).
 * Orientation codes: 0 LEFT, 1 RIGHT, 2 UP, 3 DOWN = list(ORIENTATIONS) order (map_env.py:28-31,791-793).
 * Positions are [row, col] (map_env.py:20-31).
 */
#ifndef SSD_HIP_H
#define SSD_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSD_ABI_VERSION 10   /* (still 10 with ssd_policy_head.pipeline_gather and .epsilon_rows appended: zero = as before) */

#define SSD_MAX_AGENTS 10   /* maps hold at most 10 spawn points; agent ids >= 10 break the reference (map_env.py:370) */
#define SSD_MAX_CELLS 1024  /* H*W upper bound (largest reference map is 48x18 = 864) */
#define SSD_MAX_SPAWN 16    /* spawn points ('P' cells) under random_spawn_point (the reference maps hold 3 / 5 / 10) */
#define SSD_MAX_SITES 256   /* apple / waste site list upper bound (largest: 206 apple sites) */

typedef enum ssd_status {
    SSD_OK = 0,
    SSD_ERR_INVALID = -1,     /* bad argument / unsupported configuration */
    SSD_ERR_DEVICE = -2,      /* HIP runtime error */
    SSD_ERR_NOMEM = -3,
    SSD_ERR_UNSUPPORTED = -4
} ssd_status;

enum { SSD_ENV_CLEANUP = 0, SSD_ENV_HARVEST = 1 };
enum { SSD_RNG_TAPE = 0, SSD_RNG_COUNTER = 1 };
enum { SSD_OBS_F32 = 0, SSD_OBS_BF16 = 1, SSD_OBS_U8 = 2, SSD_OBS_CODE = 3 };
enum { SSD_COLOR_SIMPLIFIED = 0, SSD_COLOR_FULL = 1 };

/* Constructor arguments.  Replaces CleanupEnv.__init__ / HarvestEnv.__init__ kwargs
 * (cleanup.py:29-61, harvest.py:18-29, config/envs/cleanup.yaml:3-15). */
typedef struct ssd_config {
    int32_t env_kind;            /* SSD_ENV_* */
    int32_t height, width;       /* map rows, cols */
    const char* ascii_map;       /* height*width chars, row-major, alphabet of constants.py:1-10 */
    int32_t n_agents;            /* <= SSD_MAX_AGENTS */
    int32_t n_env;               /* envs in this handle (this rank's shard) */
    int32_t view_size;           /* v; window edge V = 2v+1 */
    int32_t episode_limit;       /* terminated iff steps >= episode_limit (map_env.py:890-894) */
    int32_t random_spawn_point;  /* extra_args.random_spawn_point: 1 = every agent's spawn_point() shuffles the spawn list first */
    int32_t spawn_rotation;      /* extra_args.random_spawn_rotation: 0..3, or -1 = None = random */
    int32_t obs_color;           /* SSD_COLOR_* (extra_args.obs_color) */
    int32_t rng_mode;            /* SSD_RNG_* */
    int32_t device;              /* HIP device ordinal (ignored by the ssd_cpu_* mirror) */
    uint32_t env_id_base;        /* global id of env 0 of this shard (COUNTER streams are keyed by global id) */
    uint64_t seed;               /* COUNTER mode key */
    /* Cleanup thresholds (cleanup.py:31-54) */
    double threshold_depletion, threshold_restoration, waste_spawn_prob, apple_respawn_prob;
    /* Harvest SPAWN_PROB[min(k,3)] (harvest.py:20-22,118) */
    double harvest_spawn_prob[4];
} ssd_config;

/* One call's worth of recorded random draws (TAPE mode; appendix A.6 of SURVEY.md).  All arrays are
 * per env, row-major, and may be NULL in COUNTER mode.
 *   move_order  : result of np.random.shuffle over the MOVE/STAY list (map_env.py:540-542): the agent ids in
 *                 shuffled order, 0xFF padded.
 *   uniforms    : every np.random.rand(1)[0] of the call in consumption order (cleanup.py:172,183, harvest.py:119).
 *   waste_order : self.waste_points after random.shuffle (cleanup.py:178) as indices into the row-major waste
 *                 site list; only read when the call shuffles.
 *   spawn_rot   : np.random.randint(4) per agent at reset (map_env.py:789); only read when spawn_rotation = -1.
 *   spawn_order : self.spawn_points after the random.shuffle of agent a's spawn_point() call (map_env.py:776-777) as indices into
 *                 the row-major list of distinct spawn points (map_env.py:140-146); the agent takes the LAST free point of that
 *                 order.  spawn_list_len = n_spawn_points for Harvest and 2 * n_spawn_points for Cleanup, whose constructor appends
 *                 every point a second time (cleanup.py:79-80): each point id then appears twice. */
typedef struct ssd_tape {
    const uint8_t* move_order;   /* [n_env, n_agents] */
    const double* uniforms;      /* [n_env, uniforms_stride] */
    int32_t uniforms_stride;
    const uint8_t* waste_order;  /* [n_env, n_waste_sites] */
    const uint8_t* spawn_rot;    /* [n_env, n_agents] */
    const uint8_t* spawn_order;  /* [n_env, n_agents, spawn_list_len]; only read by resets with random_spawn_point = 1 */
} ssd_tape;

/* Outputs of one transition.  Replaces the return of MapEnv.step (map_env.py:874-915):
 * reward f64[n] -> f32, terminated, info{clean_num, apple_den, collective_return, equality_metric}. */
typedef struct ssd_step_out {
    float* reward;              /* [n_env, n] */
    float* clean_num;           /* [n_env, n] */
    float* apple_den;           /* [n_env, n] (same value for every agent, map_env.py:291-292) */
    uint8_t* terminated;        /* [n_env] */
    float* collective_return;   /* [n_env], written at termination (map_env.py:901-912), nullable */
    float* equality;            /* [n_env], written at termination, nullable */
    int32_t* n_draws;           /* [n_env] uniforms consumed by the call (parity check of the draw count), nullable */
} ssd_step_out;

/* Outputs of an observation pass.  Replaces get_obs / get_state / get_agent_pos / get_agent_orientation
 * (map_env.py:917-957).  Every pointer is nullable: only non-NULL outputs are produced.
 *   obs   : [n_env, n, 3, V, V] as f32 / bf16 (values k/256) or u8 (values k), or with SSD_OBS_CODE
 *           [n_env, n, V, V] u8 cell classes (0 nothing, 1 apple, 2 waste, 3 wall-or-agent; simplified colours only).
 *   state : [n_env, 3, H, W] f32. */
typedef struct ssd_obs_out {
    void* obs;
    int32_t obs_format;         /* SSD_OBS_* */
    float* state;
    float* pos;                 /* [n_env, n, 2] row, col as float */
    float* orient;              /* [n_env, n, 2] ORIENTATIONS vector as float */
    /* Optional placement of `obs` inside an episode storage [n_env, t_slots, n, ...] (EpisodeBatch.update of the "obs" key,
     * episode_runner.py:59-67, without the copy): env b's block is written at element offset
     * b * obs_env_stride + ep_step * obs_slot_stride, ep_step being the env's step counter AFTER the call (0 after a reset).
     * Both 0 (default): dense [n_env, n, ...].  GPU library only. */
    int64_t obs_env_stride, obs_slot_stride;
    /* obs_t_slots (0 = unchecked): number of time slots of that storage.  A call whose slot would be >= obs_t_slots (stepping an
     * env past its episode storage) never touches another env's block: its observation lands in the env's own LAST slot and the
     * sticky bit 16 of ssd_poll_error is raised. */
    int32_t obs_t_slots;
    /* obs_code (nullable; simplified colours; together with a f32 / bf16 / u8 `obs`): additionally emit the window as one
     * CHANNEL-MASK byte per cell (bit 0 = R = waste, bit 1 = G = apple, bit 2 = B = wall or agent; 0 = nothing: the planes of the
     * simplified palette are one-hot, so a cell is 0, 1, 2 or 4 -- SSD_CODE_CHANNEL_MASK) into a dense side buffer
     * u8 [n_env, n, obs_code_agent_stride], obs_code_agent_stride = V * V rounded up to 16, 16-byte aligned.  This is what the
     * rollout-time encoder (ssd_policy_encode) consumes: 225 B instead of 2 700 B per agent-step at V = 15. */
    uint8_t* obs_code;
} ssd_obs_out;
#define SSD_CODE_AGENT_STRIDE(V) ((((V) * (V)) + 15) & ~15)
/* byte alphabets of per-cell windows: the SSD_OBS_CODE observation format (0 nothing, 1 apple, 2 waste, 3 wall-or-agent) and the
 * channel masks of ssd_obs_out.obs_code */
enum { SSD_CODE_CLASS = 0, SSD_CODE_CHANNEL_MASK = 1 };

/* Raw env state for parity tests and KATs (Agent.set_pos etc. in the reference). */
typedef struct ssd_state {
    uint8_t* grid;              /* [n_env, H*W] cell codes */
    int16_t* pos;               /* [n_env, n, 2] */
    uint8_t* orient;            /* [n_env, n] */
    int32_t* ep_reward;         /* [n_env, n] cumulative episode reward (self.rewards, map_env.py:885-888) */
    int32_t* ep_step;           /* [n_env] self._episode_steps */
    uint32_t* epoch;            /* [n_env] COUNTER-mode episode counter (resets so far) */
} ssd_state;

typedef struct ssd_env ssd_env; /* opaque */

int ssd_abi_version(void);
const char* ssd_last_error(void);

/* REGISTRY[env](**env_args)  (envs/__init__.py:6-11, runners/episode_runner.py:15) */
int ssd_create(const ssd_config* cfg, ssd_env** out);
int ssd_destroy(ssd_env* env);

/* MapEnv.reset (map_env.py:986-993 -> _reset :297-326).  env_mask: u8[n_env] device pointer, nullable = all. */
int ssd_reset(ssd_env* env, const uint8_t* env_mask, const ssd_tape* tape, ssd_step_out* out, void* stream);
/* MapEnv.step (map_env.py:874-915).  actions: int32[n_env, n] device pointer. */
int ssd_step(ssd_env* env, const int32_t* actions, const ssd_tape* tape, ssd_step_out* out, void* stream);
/* get_obs / get_state / get_agent_pos / get_agent_orientation (map_env.py:917-957) */
int ssd_observe(ssd_env* env, ssd_obs_out* out, void* stream);
/* step immediately followed by observe of the new state, in one launch (the rollout inner loop,
 * runners/episode_runner.py:57-97: env.step then next iteration's get_obs). */
int ssd_step_observe(ssd_env* env, const int32_t* actions, const ssd_tape* tape, ssd_step_out* out,
                     ssd_obs_out* obs, void* stream);

/* Sticky device-side error bits (1 action out of range = KeyError in action_map, agent.py:174-176,235-237;
 * 2 malformed tape; 4 agent_by_pos KeyError; 8 tape overrun; 16 observation slot >= obs_t_slots; 64 bad ssd_render env id / slot).
 * Synchronises the device; clears the bits. */
int ssd_poll_error(ssd_env* env, int32_t* bits);

/* Render mode (MapEnv._render with is_replay / render, map_env.py:448-475).  on != 0 allocates the beam record and switches the
 * handle's step / step_observe to the kernels that write it (every step records the cells each agent's FIRE / CLEAN beams covered;
 * resets clear the record of the envs they reset); on == 0 frees it.  Call outside any stream capture. */
int ssd_set_render(ssd_env* env, int32_t on);
/* Full-colour frames of the envs env_ids[0..n_sel) (int32 device array) as get_map_with_agents_beam() through map_to_colors with
 * color_map: u8 [n_sel, H, W, 3] written at frames + (*slot) * slot_stride bytes (slot: int32 device pointer read by the kernel,
 * nullable = 0; the caller sizes the buffer for every slot it passes).  Needs render mode.  An env id outside 0..n_env-1 or a
 * negative slot writes nothing for that env and raises error bit 64 (ssd_poll_error). */
int ssd_render(ssd_env* env, const int32_t* env_ids, int32_t n_sel, uint8_t* frames, const int32_t* slot, int64_t slot_stride,
               void* stream);

int ssd_export_state(ssd_env* env, ssd_state* dst, void* stream);
int ssd_import_state(ssd_env* env, const ssd_state* src, void* stream);

/* Static facts derived from the map (get_env_info, map_env.py:1008-1019 and the site lists of
 * cleanup.py:72-90 / harvest.py:31-35). */
typedef struct ssd_info {
    int32_t n_actions;          /* 9 Cleanup, 8 Harvest (agent.py:153-154,207-209) */
    int32_t n_apple_sites, n_waste_sites, n_spawn_points;
    int32_t max_uniforms;       /* upper bound of uniforms consumed by one call = apple sites + waste sites */
    int32_t obs_edge;           /* V */
} ssd_info;
int ssd_get_info(const ssd_env* env, ssd_info* out);

/* HomophilyMAC._build_inputs tail (controllers/homophily_controller.py:137-184): everything except the conv
 * encoder.  Writes [B*n, A + n + 1 + 1 + 2] = onehot(last action) | onehot(id) | sign(last reward) |
 * sign(#recv+ - #recv-) | pos/||(H,W)||.  t0 is a flag word: bit 0 selects the t == 0 branch (zeros for the three history
 * terms; a last action of -1 has the same effect per row), bit 1 writes agent-major rows (i * batch + b) instead of (b * n + i);
 * bits 8.. = T > 0: `batch` counts [episodes, T] rows and the three history tensors hold every step's OWN action / reward / incentives
 * -- the kernel reads the row of the previous timestep and takes the t == 0 branch at the first step of each episode (the learner's
 * time-batched assembly without shifted copies of the tensors). */
/* Any n_agents / n_actions >= 1 is computed (the kernels loop over them; SSD_MAX_AGENTS bounds the env, not these); refused with
 * SSD_ERR_INVALID: batch * n_agents or the widest row (out_offset + n * n_actions + n_actions + 2 n + 4) past 2^31 - 1, out_offset < 0. */
int ssd_build_inputs(int32_t batch, int32_t n_agents, int32_t n_actions, int32_t t0,
                     const int64_t* last_actions /*[B,n]*/, const float* last_reward /*[B,n]*/,
                     const int64_t* last_actions_inc /*[B,n,n]*/, const float* pos /*[B,n,2]*/,
                     float pos_scale, float* out, int32_t out_stride, int32_t out_offset, void* stream);

/* Incentive reward transfer (learners/homophily_learner.py:94-115).  actions_inc int64[B,T,n,n] (giver dim 2,
 * receiver dim 3), rewards f32[B,T-1,n].  Outputs f32: give[B,T-1,n], recv_pos/neg/zero[B,T,n],
 * rewards_for_env/inc[B,T-1,n] = (r +/- ...) / seq_len with seq_len = batch.max_seq_length (true division). */
/* The time-batched incentive head's per-receiver features (homophily_agent.py:194-201) of a sampled batch, one launch:
 * actions i64 [B, T, n], pos / orient f32 [B, T, n, 2], reward / clean_num / apple_den f32 [B, T, n] (contiguous) ->
 * other f32 [T * B, n, n_actions + 7] = [one-hot(a_j), pos_j / pos_scale, orient_j, r_j, clean_j, apple_den_j] at row t * B + b, and
 * act_tm f32 [n, T * B, n_actions] = the one-hot alone, agent-major (the extra input columns of fc1_inc). */
/* Row kernels that form `workgroup * 256 + thread` in 32 bits (ssd_unroll_other, ssd_td_sim_loss): the last workgroup's index must still
 * fit, so the row count stops one workgroup short of 2^31 - 1; more is refused (SSD_ERR_INVALID). */
#define SSD_ROWS32_MAX (INT32_MAX - 256)
/* ssd_unroll_other: any n_agents / n_actions >= 1 (an action outside [0, n_actions), e.g. -1, gives an all-zero one-hot); batch * T *
 * n_agents over SSD_ROWS32_MAX is refused.  ssd_incentive_transfer: any n_agents >= 1,
 * 64-bit row arithmetic throughout -- nothing to refuse beyond the sizes below 1 (T below 2). */
int ssd_unroll_other(const int64_t* actions, const float* pos, const float* orient, const float* reward, const float* clean_num, const float* apple_den,
                     float pos_scale, int32_t batch, int32_t T, int32_t n_agents, int32_t n_actions, float* other, float* act_tm, void* stream);
int ssd_incentive_transfer(int32_t batch, int32_t T, int32_t n_agents, const int64_t* actions_inc,
                           const float* rewards, float effect_ratio, float cost_ratio, float incentive,
                           float seq_len, float* give, float* recv_pos, float* recv_neg, float* recv_zero,
                           float* rewards_for_env, float* rewards_for_inc, void* stream);

/* ssd_column_sums: out f32 [groups, cols] = sum over rows of x f32 [groups, rows, cols] (contiguous): the bias gradients of the
 * learner's affine layers (the row sums of dL/dY).  Deterministic; with workspace f32 [groups, ceil(rows / SSD_COLSUM_CHUNK), cols]
 * (nullable) two launches: chunk sums, then their sum -- no cross-workgroup hand-off inside a launch. */
#define SSD_COLSUM_CHUNK 64
int ssd_column_sums(const float* x, float* out, int32_t groups, int32_t rows, int32_t cols, float* workspace, void* stream);

/* ssd_copy_blocks: `count` (1..SSD_COPY_BLOCKS_MAX) strided 2-D f32 block copies as ONE launch,
 * dst[r * dst_stride + c] = src[r * src_stride + c] for r < rows, c < cols (strides in floats; blocks must not overlap).  `blocks` is a
 * HOST array read during the call.  The learner packs the r / z / n blocks of the GRU parameters of both heads side by side with it
 * (homophily_agent.py:83-112 keeps them as 24 separate tensors) and splits the gradients again: 2 launches instead of 8 concatenations
 * and 24 strided copies per train step. */
/* ssd_dueling_q: the dueling combination of the learner's time-batched heads (homophily_agent.py:168-170, 203-207: q = v + a - mean_k a)
 * written straight in the batch layout the loss reads -- a f32 [n, rows, K], v f32 [n, rows, 1] with rows = T * B * inner in time-major
 * order r = (t * B + b) * inner + j (what ssd_bias_bmm_fwd leaves) -> q f32 [B, T, n, inner, K] (inner = 1: q_env; inner = n: q_inc) --
 * and its backward dq -> (da, dv) in the layers' layout: one launch each instead of mean / sub / add / permuted copy and their autograd. */
int ssd_dueling_q_fwd(const float* a, const float* v, float* q, int32_t n, int32_t T, int32_t B, int32_t inner, int32_t K, void* stream);
int ssd_dueling_q_bwd(const float* dq, float* da, float* dv, int32_t n, int32_t T, int32_t B, int32_t inner, int32_t K, void* stream);

/* ssd_gather_rows: dst_f[e] = src_f[ids[e]] for e < n_ids and every field f < count (1..SSD_COPY_BLOCKS_MAX) as ONE launch; a field is
 * a dense array of rows of row_bytes bytes (any alignment).  ReplayBuffer.sample (episode_buffer.py:240-244) draws 16 episodes out of
 * thirteen storage fields with it: one launch instead of one indexing kernel per field.  `fields` is a HOST array read during the call,
 * ids a DEVICE array of n_ids int64 (each within the fields' rows: the caller checks). */
/* Any row_bytes >= 1 is copied: the kernel strides over a row with its whole grid, so rows longer than one grid sweep (32 x 256 x 4
 * bytes) take several passes (tests/test_learner_kernel_bounds.py: row_bytes = 131072 + 4). */
typedef struct ssd_row_gather {
    const void* src;
    void* dst;
    int64_t row_bytes;
} ssd_row_gather;
int ssd_gather_rows(const ssd_row_gather* fields, int32_t count, const int64_t* ids, int32_t n_ids, void* stream);

/* ssd_sample_ids: ids[0 .. count) = `count` DISTINCT episode indices drawn uniformly from [0, population) on the device --
 * ReplayBuffer.sample's `np.random.choice(episodes_in_buffer, batch_size, replace=False)` (episode_buffer.py:240-244) without a host
 * draw or an H2D copy of the indices.  Counter generator keyed by (seed, call): the caller advances `call` per sample; the same
 * (seed, call, population, count) gives the same ids on every device (a restatement for host tensors: ops.sample_ids).  Floyd's
 * subset sampling + a Fisher-Yates pass over the picks; a bounded draw is floor(u32 * m / 2^32) (bias < m / 2^32).  ids: DEVICE int64.
 * One draw kernel serves this export and ssd_sample_windows (k_sample_draw, the former k_sample_windows; the single-thread
 * k_sample_ids is gone): here it runs without a t0 and forms no starts. */
#define SSD_SAMPLE_IDS_MAX 1024
int ssd_sample_ids(uint64_t seed, uint32_t call, int32_t population, int32_t count, int64_t* ids, void* stream);

#define SSD_COPY_BLOCKS_MAX 32
/* rows * cols of one block: the kernel walks a block with a 32-bit index in strides of the whole grid (64 x 256 threads), so the last
 * stride past the end must still fit; a larger block is refused (SSD_ERR_INVALID). */
#define SSD_COPY_BLOCK_ELEMS_MAX (INT32_MAX - 64 * 256)
typedef struct ssd_block_copy {
    const float* src;
    float* dst;
    int32_t rows, cols, src_stride, dst_stride;
} ssd_block_copy;
int ssd_copy_blocks(const ssd_block_copy* blocks, int32_t count, void* stream);

/* ssd_fill_blocks: `count` (1..SSD_FILL_BLOCKS_MAX) fills with a 32-bit pattern as ONE launch (dst 4-byte aligned, bytes a multiple of
 * 4; `blocks` is a HOST array read during the call).  The vectorised runner opens an episode with it: previous actions -1 (i64: the
 * pattern 0xFFFFFFFF), previous reward / incentive actions / episode returns / hidden states / time index 0 (episode_runner.py:48-60,
 * homophily_controller.py:95-99 init_hidden) -- seven fill launches before. */
#define SSD_FILL_BLOCKS_MAX 16
typedef struct ssd_block_fill {
    void* dst;
    int64_t bytes;
    uint32_t value;
    uint32_t reserved;
} ssd_block_fill;
int ssd_fill_blocks(const ssd_block_fill* blocks, int32_t count, void* stream);

/* ssd_runner_stats: one rollout's share of EpisodeRunner's statistics (episode_runner.py:121-152) added to a device accumulator,
 * acc f64 [4] += { sum collective_return [n_env], sum equality [n_env], sum episode_return [n_returns], sum episode_return^2 }:
 * one launch, f64, fixed summation order; the host reads acc at its log interval. */
int ssd_runner_stats(const float* collective_return, const float* equality, const float* episode_return, int32_t n_env, int32_t n_returns,
                     double* acc, void* stream);

/* ssd_behaviour_stats: what the agents of one rollout DID, per agent, added to a device accumulator -- the picture behind the four
 * scalars of ssd_runner_stats (the reference has no counterpart beyond the learner's four log values incentives_to_cleanup_per,
 * incentives_to_harvest_per, value_give_mean, value_receive_mean over its 16 sampled episodes, homophily_learner.py:234-238).
 * The fields are those of an episode storage, contiguous, over t_slots = T + 1 time slots.  The sums run over every env b and every
 * slot t < T: slot T holds only the bootstrap actions and is never read.  No mask: the vectorised runners fill every slot.
 *   recv+_j(b,t) = #{i != j : actions_inc[b,t,i,j] == 1},  recv-_j likewise for 2,  rv = recv+ - recv-,
 *   r = reward, c = clean_num, both rounded to the nearest integer (a NaN counts as 0, a magnitude above 2^24 as 2^24),
 *   cl = c > 0 (the learner's binarisation, homophily_learner.py:59-60),  hv = r > 0.
 * acc f64 [SSD_BEHAVIOUR_LEN(n, A)], blocks in this order (n = n_agents, A = n_actions):
 *   reward_sum     [n]        sum r
 *   clean_sum      [n]        sum c
 *   clean_steps    [n]        sum cl
 *   harvest_steps  [n]        sum hv
 *   harvest_time   [n]        sum t hv
 *   action_count   [n, A]     #{actions == a}; values outside [0, A) are ignored
 *   inc_count      [n, n, 3]  #{actions_inc[i -> j] == c}, i != j; the diagonal is 0 whatever is stored there
 *                             (homophily_learner.py:98); values outside 0..2 are ignored
 *   recv_on_clean  [n]        per receiver j: sum cl rv
 *   recv_on_reward [n]        per receiver j: sum r rv
 *   role_count     [n, 4]     envs in which the agent was idle, cleaner, harvester, mixed: with C = sum_t cl and Hh = sum_t hv of the
 *                             episode, idle: C == 0 && Hh == 0; cleaner: C > Hh; harvester: Hh > C; mixed: C == Hh > 0
 *   cleaners_hist  [n + 1]    number of envs with exactly k cleaner agents
 *   n_episodes     [1]        n_env
 *   n_steps        [1]        n_env T
 * Every entry is an integer and is accumulated in integers (64-bit throughout: per-lane sums, LDS counters, one int64 row of
 * `workspace` per workgroup), so the result does not depend on the order of summation and acc += is exact in f64 below 2^53.
 * Two launches, no workgroup reads what another workgroup of the same launch wrote: k_behaviour_partials (G = min(
 * SSD_BEHAVIOUR_MAX_GROUPS, ceil(n_env / SSD_BEHAVIOUR_WAVES)) workgroups of SSD_BEHAVIOUR_WAVES waves, a wave per env, writes rows [0, G) of workspace -- every
 * column; the other rows are not touched) and k_behaviour_finish (one workgroup adds the rows in index order into acc).
 * With n_agents == 1 there are no pairs: inc_count and recv_* stay 0.
 * Refused (SSD_ERR_INVALID): NULL args or a NULL member pointer; n_env < 1; t_slots < 2; n_agents outside 1 .. SSD_MAX_AGENTS;
 * n_actions outside 1 .. 16; t_slots * n_agents * n_agents above INT32_MAX (an element's index inside one env's block of
 * actions_inc is 32-bit; offsets across envs, the time sums and every counter are 64-bit, so n_env has no bound of its own).
 * Refusal checks: tests/test_behaviour_host.py. */
#define SSD_BEHAVIOUR_MAX_GROUPS 256
#define SSD_BEHAVIOUR_WAVES 16
#define SSD_BEHAVIOUR_LEN(n, A) (12 * (n) + (n) * (A) + 3 * (n) * (n) + 3)
typedef struct ssd_behaviour_args {
    int32_t n_env, t_slots, n_agents, n_actions;
    const int64_t* actions;      /* [n_env, t_slots, n] */
    const int64_t* actions_inc;  /* [n_env, t_slots, n(giver), n(receiver)] */
    const float *reward, *clean_num;   /* [n_env, t_slots, n], integer-valued (what the env kernels write); rounded to nearest */
    int64_t* workspace;          /* [SSD_BEHAVIOUR_MAX_GROUPS, LEN] */
    double* acc;                 /* [LEN]  += this rollout */
} ssd_behaviour_args;
int ssd_behaviour_stats(const ssd_behaviour_args* args, void* stream);

/* Training on sampled time windows (config keys train_window / train_burn_in): one window of win_slots = L + 1 consecutive slots
 * [t0, t0 + L] per sampled episode, drawn and gathered on the device.  Refusal checks:
 * tests/test_train_window_host.py.
 *
 * ssd_sample_windows: ids[0 .. count) exactly as ssd_sample_ids gives them for the same (seed, call, population, count) -- the same
 * kernel writes them; turning windows on does not change which episodes are sampled -- and t0[e] uniform on [0, n_starts):
 *     t0[e] = floor(draw(2 * count + e) * n_starts / 2^32)
 * where draw(i) is the counter generator's 32-bit draw number i of (seed, call), all arithmetic in u32 (mix32p: "Exploration draws"
 * below), s0 / s1 the low / high 32 bits of seed:
 *     draw(i) = mix32p(mix32p(s0 ^ (call * 0x9E3779B9)) ^ (s1 + i * 0x85EBCA6B))
 * The ids are Floyd's subset sampling and a Fisher-Yates pass, every bounded draw floor(draw * m / 2^32):
 *     for i = 0 .. count - 1:  j = population - count + i;  t = floor(draw(i) * (j + 1) / 2^32);  pick[i] = t already picked ? j : t
 *     for i = count - 1 .. 1:  k = floor(draw(count + i) * (i + 1) / 2^32);  swap(pick[i], pick[k])
 * so the id draws use i < 2 * count and the starts the indices from 2 * count on.  ONE launch; ids, t0: DEVICE int64
 * [count].  A restatement for host tensors: ops.sample_windows.  Refused (SSD_ERR_INVALID): a NULL pointer, n_starts < 1, and what
 * ssd_sample_ids refuses (count outside 1 .. min(population, SSD_SAMPLE_IDS_MAX)). */
int ssd_sample_windows(uint64_t seed, uint32_t call, int32_t population, int32_t count, int32_t n_starts, int64_t* ids, int64_t* t0,
                       void* stream);

/* ssd_gather_windows: for every field f < count (1..SSD_COPY_BLOCKS_MAX) and every e < n_ids, win_slots * slot_bytes_f contiguous
 * bytes from  src_f + (ids[e] * src_slots + t0[e]) * slot_bytes_f  to  dst_f + e * win_slots * slot_bytes_f, as ONE launch; ids and
 * t0 (DEVICE int64 [n_ids]) are read on the device, nothing crosses the host boundary.  A field is a dense array of rows of src_slots
 * slots of slot_bytes bytes, at any alignment; offsets across episodes are 64-bit.  A destination is one dense byte range: the kernel
 * writes its 16-byte-aligned granules with one 16-byte store each (the source, whose alignment depends on t0, is read with loads of
 * any alignment) and the granules that cross a window's end or the range's ends byte by byte.
 * At most one field is flagged `filled` (slot_bytes 8: int64 slots, src and dst 8-byte aligned).  It is not copied but written with
 * the burn-in rule: dst[e, r] = src[ids[e], t0[e] + r] * (r >= K_e), K_e = burn_in if t0[e] > 0, K_e = 0 if t0[e] == 0 (there the
 * zero hidden state is the true state).
 * The device validates neither ids nor t0: THE CALLER GUARANTEES 0 <= ids[e] < rows_f and 0 <= t0[e], t0[e] + win_slots <= src_slots.
 * Then no load leaves [src_f, src_f + rows_f * src_slots * slot_bytes_f) and no store leaves the n_ids * win_slots destination slots.
 * `fields` is a HOST array read during the call.  Refused (SSD_ERR_INVALID): a NULL pointer (fields, ids, t0, a field's src / dst);
 * count outside 1 .. SSD_COPY_BLOCKS_MAX; n_ids outside 1 .. 65535; win_slots outside 2 .. src_slots; burn_in outside
 * 0 .. win_slots - 2; slot_bytes < 1; a field whose destination is over 64 GiB; more than one `filled` field, or one whose
 * slot_bytes != 8 or whose pointers are not 8-byte aligned. */
typedef struct ssd_window_field {
    const void* src;
    void* dst;
    int64_t slot_bytes;
    int32_t filled;        /* 1: the `filled` mask (see above); 0: a plain copy */
    int32_t reserved;
} ssd_window_field;
int ssd_gather_windows(const ssd_window_field* fields, int32_t count, const int64_t* ids, const int64_t* t0, int32_t n_ids,
                       int32_t src_slots, int32_t win_slots, int32_t burn_in, void* stream);

/* Prioritised replay (config key prioritized_replay, default off; per_alpha / per_beta / per_beta_anneal_steps / per_eta / per_eps):
 * proportional draws, importance weights and new priorities on the device.  The reference has no counterpart (its
 * ReplayBuffer.sample is np.random.choice).  Refusal checks: tests/test_priority_host.py.
 *
 * Priority table: one u32 per buffer slot, fixed point: SSD_PRIORITY_ONE is 1.0, stored values lie in [1, SSD_PRIORITY_MAX], 0 means
 * "never trained on".  Integers, so that every sum is an integer sum: the order of summation cannot show and a draw is the same on
 * every device (the argument of ssd_behaviour_stats).
 *   qmax    = the largest table[k], k < population, or SSD_PRIORITY_ONE if all of them are 0
 *   qeff[k] = table[k] ? table[k] : qmax          (a new episode is sampled at the current maximum; no state between calls)
 *   total   = sum_k qeff[k]                       (u64; population <= SSD_PRIORITY_POP_MAX = 2^20, so total < 2^44)
 *
 * ssd_priority_sample: ONE launch, one workgroup.  Stratified, with replacement; draw(i) is the generator of ssd_sample_windows for
 * (seed, call).  For e < count:
 *   lo = floor(total * e / count);   hi = floor(total * (e + 1) / count)          (hi > lo wherever total >= count)
 *   x  = lo + floor(draw(e) * (hi - lo) / 2^32)                                   (exact integers; the product is split, it passes 64 bits)
 *   ids[e] = the smallest k with cum[k] > x,  cum[k] = qeff[0] + .. + qeff[k]
 *   t0[e]  = floor(draw(2 * count + e) * n_starts / 2^32)                         (as ssd_sample_windows; n_starts = 1: t0 = 0)
 *   w_raw[e] = (population * qeff[ids[e]] / total)^(-beta);   weights[e] = w_raw[e] / max_e' w_raw[e']
 * count may exceed population (one episode can own several strata: duplicate ids are legal); where total < count a stratum can be
 * empty (hi == lo) and x = lo.  x rises with e, so the ids come out in non-decreasing order.  The weights are evaluated in f64 as
 * (qeff[ids[e]] / qmin)^(-beta), qmin the smallest sampled qeff -- the same number, the common factor population / total cancelled --
 * and rounded to f32: the largest weight is exactly 1, and with beta = 0 every weight is.
 * log f32 [4] = mean of qeff / SSD_PRIORITY_ONE over the population, max of the same, the smallest weight, the number of distinct ids.
 * The kernel: pass 1 the maximum; pass 2 one contiguous chunk of ceil(population / 1024) entries per thread summed in u64; a
 * workgroup prefix scan of the 1024 chunk sums (a wave scan by shuffles, the sixteen wave totals through LDS, chained in index
 * order); thread e binary-searches the chunk sums and walks one chunk.  The table is read through L2 (three times at most); no
 * atomics, no scratch.  table: DEVICE u32 [>= population]; ids, t0: DEVICE int64 [count]; weights: DEVICE f32 [count].
 * Refused (SSD_ERR_INVALID): NULL args or a NULL member pointer; population outside 1 .. SSD_PRIORITY_POP_MAX; count outside
 * 1 .. SSD_SAMPLE_IDS_MAX; n_starts < 1; beta outside [0, 1] or NaN; a table that is not 4-byte aligned.
 *
 * A priority per training window (config key per_unit: "window"; n_segments >= 1): the table holds n_segments = S entries per buffer
 * slot, entry (slot, k) at slot * S + k, one per window of the slot's episode on a stride grid: window k starts at
 * start_k = min(k * seg_stride, last_start), last_start = T - L (the last window is clamped so that the episode's tail is covered).
 * `population` counts ENTRIES (episodes * S).  The draw is the draw above on the flat table, unchanged -- qmax, qeff, total, strata,
 * x, weights and log over entries, log[3] = the number of distinct entries -- written by a second kernel, k_priority_sample_seq (the
 * same body instantiated a second time), which files the drawn entry and maps it:
 *   entries[e] = the smallest f with cum[f] > x;   ids[e] = entries[e] / S;   t0[e] = min((entries[e] % S) * seg_stride, last_start)
 * n_starts is not read and draw(2 * count + e) is not consumed.  Several strata landing in one episode are several windows of it (or
 * one window several times).  entries: DEVICE int64 [count], what ssd_priority_update takes as ids with table_len = slots * S.
 * n_segments == 0: the launch above, entries may be NULL.  Refused in addition: n_segments < 0 or over SSD_PRIORITY_SEGMENTS_MAX; with
 * n_segments >= 1: NULL entries; seg_stride < 1; last_start < 0; (n_segments - 1) * seg_stride < last_start (the grid would not
 * reach the last start); population not a multiple of n_segments. */
#define SSD_PRIORITY_SEGMENTS_MAX 256
#define SSD_PRIORITY_ONE 65536u
#define SSD_PRIORITY_MAX 16777216u
#define SSD_PRIORITY_POP_MAX 1048576
typedef struct ssd_priority_sample_args {
    uint64_t seed;
    uint32_t call;
    int32_t population, count, n_starts;
    float beta;
    const uint32_t* table;
    int64_t *ids, *t0;
    float* weights;
    float* log;                  /* [4] */
    int32_t n_segments, seg_stride, last_start;      /* 0: one entry per slot, the members behind are not read */
    int64_t* entries;            /* [count], n_segments >= 1 */
} ssd_priority_sample_args;
int ssd_priority_sample(const ssd_priority_sample_args* args, void* stream);

/* ssd_priority_update: after ssd_td_sim_loss (mode 1; either kernel) of a batch of `batch` samples over t_slots = T + 1 slots:
 * the new priorities of the trained samples from the loss kernel's `partials`, the importance weights applied to the gradient
 * seeds, the table written.  Two launches on the stream; no workgroup reads what another workgroup of the same launch wrote.
 * k_priority_rows (one workgroup of 256 threads per sample e) over the sample's T * n rows of partials (col0 = mask,
 * col2 = (td_env mask)^2, col3 = (td_inc mask)^2):
 *   d_row = sqrt(col2 + col3)
 *   p     = eta * max_rows d_row + (1 - eta) * (sum_rows d_row) / max(1, sum_rows col0) + eps
 *   q_new[e] = clamp(round_to_nearest(p^alpha * SSD_PRIORITY_ONE), 1, SSD_PRIORITY_MAX)          (a NaN counts as SSD_PRIORITY_MAX)
 * in f32.  Rows without loss (the unfilled tail, burn-in rows, rows after termination) have mask 0 and both squares 0: they add
 * nothing; a sample with no loss row gets p = eps.  The float max does not depend on the order; the sums are deterministic: thread t
 * adds its rows t, t + 256, t + 512 .. in rising order, and the 256 thread sums are added by the fixed tree of the optimiser's
 * partial sums (stride 128, 64 .. 1: element t += element t + stride).
 * The same workgroup then multiplies every element of the sample's block of dq_env [batch, t_slots, n, A] and of dq_inc
 * [batch, t_slots, n, n, 3] by weights[e] in place -- one f32 multiply per element, 16-byte accesses between scalar edges.  The train
 * step then minimises sum_e weights[e] L_e, L_e the sample's share of the loss over the unchanged global denominators.
 * k_priority_apply (one workgroup): table[ids[e]] = max over the e' with ids[e'] == ids[e] of q_new[e']: thread e writes iff no e'
 * carries the same id with a larger value, or the same value and a smaller index (ids and values in LDS, `batch` compares per
 * thread): one writer per slot, whatever the launch order.  An id outside [0, table_len) is skipped.
 * Refused (SSD_ERR_INVALID): NULL args or a NULL member pointer; batch outside 1 .. SSD_SAMPLE_IDS_MAX; t_slots < 2; n_agents,
 * n_actions or table_len < 1; table_len over SSD_PRIORITY_POP_MAX; alpha or eta outside [0, 1] or NaN; eps <= 0 or NaN; batch *
 * t_slots * n_agents over SSD_ROWS32_MAX; partials not 16-byte aligned (its rows are read as 16-byte columns 0 .. 3), dq_env / dq_inc
 * not 4-byte aligned. */
typedef struct ssd_priority_update_args {
    int32_t batch, t_slots, n_agents, n_actions, table_len;
    float alpha, eta, eps;
    const float* partials;       /* [batch * (t_slots - 1) * n_agents, SSD_TD_LOSS_PARTIALS] */
    const int64_t* ids;          /* [batch] */
    const float* weights;        /* [batch] */
    float *dq_env, *dq_inc;      /* scaled in place */
    uint32_t* q_new;             /* [batch] staging */
    uint32_t* table;             /* [table_len] */
} ssd_priority_update_args;
int ssd_priority_update(const ssd_priority_update_args* args, void* stream);

/* ssd_rollout_priority (config key per_initial_priority: "rollout"; default "max" = the zero entry above): the priority an episode
 * enters the table with, formed by the rollout from the TD errors of what it just produced (Ape-X / R2D2), ONE launch per timestep
 * slot behind the inc head of slot t = *t_index (the slot scalar ssd_store_hidden reads).  Online: no Q-value is kept per slot.
 * Refusal checks: tests/test_rollout_priority_host.py.
 *
 * The value is ssd_priority_update's formula and f32 operation sequence over the episode's T * n rows (t, agent i), T = t_slots - 1:
 *   d      = sqrt((td_env mask)^2 + (td_inc mask)^2)
 *   p      = eta * max d + (1 - eta) * (sum d) / max(1, sum mask) + eps
 *   q_init = clamp(round_to_nearest(p^alpha * SSD_PRIORITY_ONE), 1, SSD_PRIORITY_MAX)                (a NaN counts as SSD_PRIORITY_MAX)
 * where td is the ONE-STEP TD error of k_td_sim_loss<1> (its plain branch: no consider_others_inc, no td_lambda, whatever the learner
 * runs with) evaluated with the acting network as live AND target net.  For row t of env b, agent i, from slot t of the storage:
 *   give, rp, rn = incentives i gave / received (+) / received (-);   r = reward[b, t, i] / reward_scale
 *   r_env = (r + (rp - rn) incentive_ratio incentive) / seq_len;      r_inc = (r - give incentive_cost incentive) / seq_len
 *   mask  = filled[b, t] (t ? 1 - terminated[b, t - 1] : 1);          live = 1 - terminated[b, t]
 *   td_env = Q_env,t[i, a_t] - (r_env + gamma_env live max_{k available} Q_env,t+1[i, k])
 *   td_inc = sum_{j != i} Q_inc,t[i, j, a_inc,t[i, j]] - (r_inc + gamma_inc live sum_{j != i} max_c Q_inc,t+1[i, j, c])
 * Q_t is what the heads computed at slot t (exploration does not enter it); live = target, so double_q selects the same value.  The
 * value is a starting estimate: the first train step on the episode overwrites it (ssd_priority_update).
 * The mask is the learner's: it looks one slot back only and row 0 is never masked by `terminated`.  An env that terminates AT slot 0
 * therefore keeps row 0 (with live = 0) and does NOT get p = eps; the rows behind a termination add nothing because a runner leaves
 * them unfilled.  p = eps belongs to an env without a filled slot.
 *
 * The launch at slot t, per (env, agent) -- 16 lanes per env, four envs per wave, one thread per agent:
 *   t == 0        acc = (0, 0, 0)
 *   1 <= t <= T   row t - 1 from carry (chosen_env, chosen_inc of slot t - 1), slot t - 1 of the storage and this slot's Q:
 *                 acc.max = fmaxf(acc.max, d); acc.sum += d; acc.cnt += mask     (so every agent's sums run in rising t)
 *   t < T         carry = (Q_env,t[i, actions[b, t, i]], sum_{j != i} Q_inc,t[i, j, actions_inc[b, t, i, j]]) (j rising), the actions the
 *                 heads just filed in slot t (an index outside its range is clamped into it)
 *   t == T        additionally the env's agents are reduced inside their wave by cross-lane reads of registers (the max is order-free; sum d
 *                 and sum mask are added agent 0, 1 .. n - 1 in that order) and q_init[env] is written
 *   otherwise     nothing is written
 * No thread reads what another thread of the same launch wrote: carry / acc belong to their (env, agent); the other agents'
 * actions_inc of slot t - 1 were filed by earlier launches.  Plain loads and vector stores, no atomics, no scratch, no LDS; 64-bit
 * offsets into the storage.
 * q_env f32 is read as q_env[agent * q_env_agent_stride + env * q_env_env_stride + k], q_inc likewise as [.. + j * 3 + c] (elements):
 * FastPolicy's agent-major q_out [n, N, A] / [n, N, n, 3] is (N A, A) / (N n 3, n 3); the generic timestep's env-major [N, n, A] /
 * [N, n, n, 3] is (A, n A) / (n 3, n n 3).  avail_bits: bit k = env action k available.  Storage fields of the episode being written:
 * actions i64 [N, T + 1, n], actions_inc i64 [N, T + 1, n, n] (giver, receiver), reward f32 [N, T + 1, n], terminated u8 [N, T + 1],
 * filled i64 [N, T + 1] (nullable: all ones).  Caller-owned state: carry f32 [N, n, 2], acc f32 [N, n, 3] (max d, sum d, sum mask),
 * q_init u32 [N].
 * Refused (SSD_ERR_INVALID, nothing launched): NULL args or a NULL member pointer other than filled; n_env < 1 or over 2^24; t_slots < 2;
 * n_agents outside 2 .. SSD_MAX_AGENTS; n_actions outside 1 .. 16; none of the low n_actions bits of avail_bits set; alpha or eta outside
 * [0, 1] or NaN; eps, seq_len or reward_scale <= 0 or NaN; a negative stride; q_env, q_inc, reward, carry, acc or q_init not 4-byte
 * aligned, t_index, actions, actions_inc or filled not 8-byte aligned.
 *
 * A priority per training window (per_unit: "window"; n_segments = S >= 1): a second kernel, k_rollout_priority_seq, same launch
 * shape.  Window k of the grid (ssd_priority_sample) starts at start_k = min(k * seg_stride, T - win_len); its loss rows are
 * start_k + K_k <= row < start_k + win_len, K_k = burn_in if start_k > 0 else 0 (the rule of ssd_gather_windows).  Every window enters
 * the table with the value above over ITS loss rows, all agents: q_init u32 [N, S], acc f32 [N, n, S, 3].  d and mask of a row are
 * the ones above (the same device function; seq_len is the episode's, whatever train_window_norm says); only the aggregation changes:
 *   t == 0        the pair's S accumulators = (0, 0, 0)
 *   1 <= t <= T   row t - 1 formed ONCE and added to the (max, sum, cnt) of every window whose loss rows contain it -- at most
 *                 ceil(win_len / seg_stride) + 1 windows; no other accumulator is read or written; each window's sums run in rising t
 *   t == T        additionally, for every k, the env's agents are reduced as above (max order-free, sums agent 0 .. n - 1) and
 *                 q_init[env, k] is written (a thread re-reads accumulators it wrote itself, no other thread's)
 * With S = 1 (win_len = T) q_init and acc are bit for bit those of n_segments = 0.  Refused in addition: n_segments < 0 or over
 * SSD_PRIORITY_SEGMENTS_MAX; with n_segments >= 1: win_len outside 1 .. t_slots - 1; seg_stride outside 1 .. win_len;
 * ceil(win_len / seg_stride) over 8; burn_in outside 0 .. win_len - 1; n_segments != ceil((T - win_len) / seg_stride) + 1. */
typedef struct ssd_rollout_priority_args {
    const int64_t* t_index;      /* device scalar */
    int32_t n_env, n_agents, n_actions, t_slots;
    uint32_t avail_bits;
    int32_t reserved;            /* 0 */
    const float *q_env, *q_inc;
    int64_t q_env_agent_stride, q_env_env_stride, q_inc_agent_stride, q_inc_env_stride;      /* elements */
    const int64_t *actions, *actions_inc;
    const float* reward;
    const uint8_t* terminated;
    const int64_t* filled;       /* nullable */
    float gamma_env, gamma_inc, reward_scale, incentive_ratio, incentive_cost, incentive, seq_len, alpha, eta, eps;
    float *carry, *acc;
    uint32_t* q_init;            /* [n_env], or [n_env, n_segments] */
    int32_t n_segments, win_len, seg_stride, burn_in;    /* 0: one priority per episode, the members behind are not read */
} ssd_rollout_priority_args;
int ssd_rollout_priority(const ssd_rollout_priority_args* args, void* stream);

/* ssd_clip_adam_step: the optimiser tail of HomophilyLearner.cal_loss_and_step (homophily_learner.py:223-226) --
 *   clip_grad_norm_(params_inc, clip); clip_grad_norm_(params_env, clip); optimiser_inc.step(); optimiser_env.step()
 * with the conv encoder a member of BOTH parameter groups (homophily_agent.py:127-146: its gradient is scaled by both clips, the second
 * norm sees the first scaling, and both Adams move it, each with its own moments) -- as TWO launches over the flat gradient buffer
 * instead of ~20 (2 x multi-tensor norm + scalar arithmetic + multi-tensor scale, 2 x fused Adam + step counters):
 *   1. per 1024-element chunk, the sums of squares of the three segments (encoder / env head / inc head, per job); every step counter += 1
 *   2. every workgroup adds the chunk sums in a fixed order (deterministic; no atomics, no cross-workgroup hand-off), forms
 *      c_inc = min(1, clip / (sqrt(S_enc + S_inc) + 1e-6)), c_env = min(1, clip / (sqrt(c_inc^2 S_enc + S_env) + 1e-6)), writes the
 *      scaled gradients back and applies torch.optim.Adam's update (no weight decay / amsgrad; lerp form of the first moment,
 *      bias corrections from the per-parameter step counters) -- inc optimiser first, then env, as the reference steps them.
 * jobs: DEVICE array, one per parameter tensor in flat-buffer order; state index 0 = the inc optimiser's (exp_avg, exp_avg_sq, step),
 * 1 = the env optimiser's; a parameter outside an optimiser has NULLs there.  partials: f32 [ceil(total / 1024)][3] workspace.
 *
 * Polyak target update (config key target_tau; members from polyak_jobs on, all zero / NULL: exactly the two launches above).  With
 * n_polyak > 0 ONE more launch behind the second moves every destination element of every job by
 *     t_new = fl(fl(t * c) + fl(l * tau)),   c = fl(1 - tau),   all f32: three roundings, no fused multiply-add
 * where l is the job's source element as the Adam launch left it (tau = 1: c = 0 and t_new = l).  A job is one 2-D block: src
 * contiguous [rows, cols], dst rows of cols elements dst_row_stride elements apart -- a target parameter (dst_row_stride == cols) or a
 * parameter's slice inside a concatenated copy of target weights (dst_row_stride > cols; the elements between the rows belong to
 * other jobs and are neither read nor written).  Blocks of different jobs must not overlap.  src and dst need 4-byte alignment only.
 * The launch is SSD_POLYAK_WORKGROUPS workgroups of 256 threads over the jobs' elements numbered job after job, row-major within a
 * job (E in all): workgroup w owns elements [w P, (w + 1) P), P = 256 ceil(E / (256 SSD_POLYAK_WORKGROUPS)), and its thread t takes
 * w P + t, w P + t + 256, ... in rising order.  Every element is written exactly once; no atomics, no cross-workgroup hand-off.
 * polyak_partials (nullable): f32 [SSD_POLYAK_WORKGROUPS][2]; workgroup w writes {sum (l - t_new)^2, sum l^2} over ITS elements of the
 * jobs with dst_row_stride == cols (the parameters; slices add nothing).  Order: every thread adds fl(d * d), d = fl(l - t_new)
 * (resp. fl(l * l)) to an f32 accumulator starting at 0 in the order it takes its elements; the 256 accumulators a[0 .. 255] are then
 * folded as  for s = 128, 64, .., 1: a[t] = fl(a[t] + a[t + s]) for t < s;  a[0] is written.
 * DEVICE array polyak_jobs: a job with rows < 1, cols < 1, dst_row_stride < cols or rows * cols >= 2^31 is skipped (the table's
 * builder checks them: abi.polyak_job_table).  Refused before any launch: n_polyak outside 0 .. SSD_POLYAK_MAX_JOBS; polyak_jobs NULL
 * with n_polyak > 0; target_tau outside [0, 1] or NaN; target_tau == 0 with n_polyak > 0. */
#define SSD_ADAM_MAX_JOBS 64
#define SSD_POLYAK_MAX_JOBS 128
#define SSD_POLYAK_WORKGROUPS 256
typedef struct ssd_polyak_job {
    const float* src;              /* [rows, cols] contiguous: the live parameter */
    float* dst;
    int32_t rows, cols;
    int64_t dst_row_stride;        /* elements */
} ssd_polyak_job;
typedef struct ssd_adam_job {
    float* param;
    int64_t offset;                /* first element in the flat gradient buffer */
    int32_t numel, segment;        /* segment: 0 encoder (both optimisers), 1 env head, 2 inc head */
    float* exp_avg[2];
    float* exp_avg_sq[2];
    float* step[2];                /* f32 device scalars (torch's capturable / fused Adam keeps them so) */
} ssd_adam_job;
typedef struct ssd_clip_adam_args {
    float* flat_grad;
    int64_t total;                 /* elements of flat_grad = sum of the jobs' numel (the jobs tile it in order) */
    const ssd_adam_job* jobs;
    int32_t n_jobs;
    float* partials;
    float lr_inc, lr_env, beta1, beta2, eps, clip;
    const ssd_polyak_job* polyak_jobs;   /* DEVICE array (nullable with n_polyak == 0) */
    int32_t n_polyak;
    float target_tau;
    float* polyak_partials;        /* nullable */
} ssd_clip_adam_args;
int ssd_clip_adam_step(const ssd_clip_adam_args* args, void* stream);

/* ssd_td_sim_loss: the loss of HomophilyLearner.cal_loss_and_step (learners/homophily_learner.py:94-217) -- incentive reward
 * transfer, double-Q TD losses of the env head and the incentive head, the similarity loss with the exact-value clustering rule --
 * AND its gradient w.r.t. the live Q-values in one launch (the reference builds it from ~100 tensor ops that autograd differentiates).
 * All tensors are over the batch's T+1 time slots (t_slots = batch.max_seq_length), contiguous:
 *   q_env, tq_env f32 [B, T+1, n, A] (live / target net, masked by avail as the reference does); q_inc, tq_inc f32 [B, T+1, n, n, 3];
 *   actions i64 [B, T+1, n]; actions_inc i64 [B, T+1, n(giver), n(receiver)]; avail i32 [B, T+1, n, A]; reward, clean_num f32 [B, T+1, n];
 *   terminated u8 [B, T+1]; filled i64 [B, T+1].
 * mode 0: only the per-row denominators: partials[:, 0] = mask, partials[:, 1] = sum of sim_loss_mask (their sums are
 *         mask.sum() and sim_loss_mask.sum(); data parallel: all-reduce them before mode 1).
 * mode 1: dens f32 [2] = the GLOBAL (mask.sum(), sim_loss_mask.sum()); writes dq_env / dq_inc (shapes of q_env / q_inc, every element)
 *         = d loss / d q with loss = (sum (td_env mask)^2 + sum (td_inc mask)^2) / dens[0] + sim_loss_weight sum_sim / (1 + dens[1]),
 *         and partials f32 [B * T * n, SSD_TD_LOSS_PARTIALS] per (b, t, i): 0 mask, 1 sim mask sum, 2 (td_env mask)^2,
 *         3 (td_inc mask)^2, 4 similarity terms, 5 q_env taken, 6 sum_j q_inc taken, 7 give, 8 recv+ - recv-, 9 clean (recv+ - recv-),
 *         10 clean flag, 11 r (recv+ - recv-), 12 r  -- the caller adds the rows in a fixed order (losses and the learner's log values).
 * consider_others_inc (config/algs/homophily.yaml, default False; homophily_learner.py:118-164): with rz, rp, rn = the received counts
 *         (zero, +, -) of the RECEIVER j (receive_*.unsqueeze(2) broadcasts over the giver i) and j != i, the inc head's chosen value is
 *         (q_inc[t,i,j,0] rz_j(t) + q_inc[t,i,j,1] rp_j(t) + q_inc[t,i,j,2] rn_j(t)) / (n-1) and its target
 *         (tmax_self + sum_c tq_inc[t+1,i,j,c] recv_c,j(t+1) - tq_inc[t+1,i,j,a_inc[t+1,i,j]]) / (n-1), tmax_self being the double_q /
 *         plain-max selection; dq_inc[t,i,j,c] = (similarity part) + g_inc recv_c,j(t) / (n-1).  The logged q_inc taken stays the
 *         gather at a_inc.
 * Refused (SSD_ERR_INVALID): n_agents outside 2 .. SSD_MAX_AGENTS (the agents' window flags are bits of one word), batch * t_slots *
 * n_agents over SSD_ROWS32_MAX (32-bit thread index), in mode 1 a td_lambda below 0, above 1 or NaN.  partials columns 13 .. 15 are
 * never written while td_lambda is 0.
 * td_lambda (learner config key of the same name, default 0; mode 0 ignores it): 0 = the one-step targets above, same kernel, same
 *         numbers.  In (0, 1] both heads take TD(lambda) targets from one launch of a second kernel (one workgroup per (episode,
 *         agent), a backward scan over t; any T): with T = t_slots - 1, V_h,t+1 the bootstrap value the one-step target of row t uses
 *         (env: the selected tq_env[t+1]; inc: sum_{j != i} of the selected / consider_others_inc value), r_h,t the head's reward,
 *         mask_t and live_t = 1 - terminated[b, t] as above,
 *             G_h,T = V_h,T (1 - sum_{t < T} terminated[b, t]),
 *             G_h,t = td_lambda gamma_h G_h,t+1 + mask_t (r_h,t + (1 - td_lambda) gamma_h live_t V_h,t+1),   t = T-1 .. 0,
 *         and td_h,t = chosen_h,t - G_h,t; everything downstream (squared errors, gradient rows, similarity loss, columns 0 .. 12) is
 *         unchanged in form.  partials column 13 = G_env,t and 14 = G_inc,t of the row; column 15 is still never written.
 *         The member follows sim_loss_weight, in the four bytes that were padding in front of the first pointer (the fifteen 4-byte
 *         scalars end at byte 60, q_env sits at 64): sizeof and the offset of every other member are unchanged, and
 *         consider_others_inc stays the last member. */
#define SSD_TD_LOSS_PARTIALS 16
typedef struct ssd_td_loss_args {
    int32_t batch, t_slots, n_agents, n_actions, sim_horizon, double_q;
    float gamma_env, gamma_inc, reward_scale, incentive_ratio, incentive_cost, incentive, seq_len, sim_threshold, sim_loss_weight;
    float td_lambda;
    const float *q_env, *q_inc, *tq_env, *tq_inc;
    const int64_t *actions, *actions_inc;
    const int32_t* avail;
    const float *reward, *clean_num;
    const uint8_t* terminated;
    const int64_t* filled;
    const float* dens;
    float *dq_env, *dq_inc, *partials;
    int32_t consider_others_inc;
} ssd_td_loss_args;
int ssd_td_sim_loss(const ssd_td_loss_args* args, int32_t mode, void* stream);

/* ---- rollout-time (inference) controller pieces that are not GEMMs (csrc/ssd_policy.hip) -----------------------------
 * ssd_encoder: HomophilyAgent.rgb_preprocess (homophily_agent.py:20-27,213-214) = Conv2d(3, conv_out, 3, 1) + LeakyReLU +
 *   Flatten + Linear(conv_out * (V-2)^2, feat_out) + LeakyReLU on obs f32 [rows, 3, V, V] -> out[row * out_stride + 0..feat_out).
 *   agent_major: rows are (env b, agent i); write row (i * (rows / n_agents) + b) instead (per-agent batched GEMM layout).
 *   view_edge 3 .. 36: a workgroup stages four windows (4 * (3 V^2 + 4) floats) in the 64 KiB of LDS a launch gets without raising
 *   its attribute; a larger edge is SSD_ERR_INVALID (ssd_conv_leaky, one window + 168 floats of weights: 3 .. 73).
 * ssd_gru_gates: the gate arithmetic of the hand-written GRU cell (homophily_agent.py:162-165,188-191) on gi = x W_i + b_i,
 *   gh = h W_h + b_h, both [rows, 3 * hidden] in (r, z, n) order; h [rows, hidden] is updated in place.
 * ssd_dueling_pick: q = v + a - mean(a) (homophily_agent.py:168-170,204-206) on av [rows, n_actions + 1] (advantages, then the
 *   value) followed by the epsilon-greedy choice of EpsilonGreedyActionSelector (action_selectors.py:44-68) with the available
 *   mask avail u8[n_actions] (NULL = all).  epsilon f32 and step i64 are device scalars; rows are agent-major (i, b) or, with
 *   pairs = 1, (i, b, j) with the diagonal i == j forced to 0 (homophily_controller.py:44-46); actions are written env-major
 *   [batch, n] / [batch, n, n].  q_out (nullable) receives q [rows, n_actions].  The exploration draw of a row is keyed by
 *   (seed, *step, (env_id_base + b) * n + i [, * n + j]): the GLOBAL env id, so env shards draw what the unsharded job draws.
 *   n_actions 1 .. 16 (the mask is gathered into 16 bits; SSD_ERR_UNSUPPORTED above that, like K of ssd_dueling_q_*). */
int ssd_encoder(const float* obs, int32_t rows, int32_t view_edge, int32_t conv_out, int32_t feat_out, const float* conv_w,
                const float* conv_b, const float* lin_w, const float* lin_b, float* out, int32_t out_stride, int32_t n_agents,
                int32_t agent_major, float* store_obs, int64_t store_env_stride, const int64_t* store_t, void* stream);
/* store_obs (nullable): additionally copy the observation of row (env b, agent i) to
 * store_obs[b * store_env_stride + (*store_t) * n_agents * 3VV + i * 3VV ...], i.e. into obs[b, t] of an episode storage
 * f32 [n_env, T+1, n, 3, V, V] (EpisodeBatch.update of the "obs" key, episode_runner.py:59-67) with store_env_stride =
 * (T+1) * n * 3VV and the time index read from device memory. */

/* ssd_conv_leaky: only the Conv2d(3, conv_out, 3, 1) + LeakyReLU + Flatten part of rgb_preprocess: out f32 [rows, conv_out*(V-2)^2]
 * (row order as agent_major says); the Linear layer behind it is a plain GEMM.  store_* as in ssd_encoder. */
int ssd_conv_leaky(const float* obs, int32_t rows, int32_t view_edge, int32_t conv_out, const float* conv_w, const float* conv_b,
                   float* out, int32_t n_agents, int32_t agent_major, float* store_obs, int64_t store_env_stride,
                   const int64_t* store_t, void* stream);

/* One launch for the small per-timestep fields of an episode storage [n_env, t_slots, ...] (the EpisodeBatch.update calls of
 * episode_runner.py:59-93): every non-NULL source is written to dst[(b * t_slots + *t_index), ...]; actions also as one-hot. */
typedef struct ssd_store_step {
    const int64_t* t_index;     /* device scalar */
    int32_t n_env, n_agents, n_actions, t_slots;
    const float *pos, *orient;                       /* [n_env, n, 2] */
    const float *reward, *clean_num, *apple_den;     /* [n_env, n] */
    const uint8_t* terminated;                       /* [n_env] */
    const int64_t *actions, *actions_inc;            /* [n_env, n], [n_env, n, n] */
    float *dst_pos, *dst_orient, *dst_reward, *dst_clean_num, *dst_apple_den, *dst_actions_onehot;
    uint8_t* dst_terminated;
    int64_t *dst_actions, *dst_actions_inc;
    /* optional runner state carried to the next timestep by the same launch (all nullable): the "previous" action / reward /
     * incentive inputs of the controller, the running episode return (+= reward), and two device counters that this launch
     * does not read itself (so one thread can update them without a grid-wide barrier): *next_t_out = *t_index + 1 and
     * *counter_inc += 1.  next_t_out must not alias t_index (ssd_policy_encode's slot_t_copy provides the second scalar). */
    int64_t* prev_actions;          /* [n_env, n]    <- actions */
    float* prev_reward;             /* [n_env, n]    <- reward */
    int64_t* prev_actions_inc;      /* [n_env, n, n] <- actions_inc */
    float* ep_return;               /* [n_env, n]    += reward */
    int64_t* next_t_out;
    int64_t* counter_inc;
} ssd_store_step;
int ssd_store_step_launch(const ssd_store_step* args, void* stream);

/* ssd_store_hidden (config key train_stored_state, default off): the rollout's recurrent state filed with the episode, one launch per
 * timestep after the inc head of slot t (R2D2's stored state).  The state filed in slot t is the state AFTER the controller consumed
 * slot t -- the one the heads of slot t produced Q_t from.  dst f32 [n_env, t_slots, n_agents, 128] = [h_env 64 | h_inc 64] per agent;
 * only slot *t_index is written, and nothing at all when *t_index lies outside [0, t_slots).  The sources are read as
 * h[agent * src_agent_stride + env * src_env_stride + 0..63] (elements): FastPolicy's agent-major [n, N, 64] is (N * 64, 64), the
 * generic timestep's [N, n, 1, 64] is (64, n * 64).  k_store_hidden: one thread per 16 bytes, 64-bit offsets, no atomics; the launch
 * writes no scalar.  Refusal checks: tests/test_stored_state_host.py.
 * Refused (SSD_ERR_INVALID): NULL args or a NULL member pointer; n_env, n_agents or t_slots below 1; h_env, h_inc or dst not 16-byte
 * aligned; a negative source stride or one that is not a multiple of 4 elements. */
typedef struct ssd_store_hidden_args {
    const int64_t* t_index;     /* device scalar */
    int32_t n_env, n_agents, t_slots;
    int32_t reserved;           /* 0 */
    const float *h_env, *h_inc;
    int64_t src_agent_stride, src_env_stride;        /* elements */
    float* dst;
} ssd_store_hidden_args;
int ssd_store_hidden(const ssd_store_hidden_args* args, void* stream);

int ssd_gru_gates(const float* gi, const float* gh, float* h, int32_t rows, int32_t hidden, void* stream);
/* ssd_gru_gates / _fwd / _bwd: any rows >= 1 and any hidden >= 1 (elementwise kernels that stride over rows x hidden with a grid of at
 * most 4096 workgroups; 64-bit offsets) -- the bounds suite runs hidden 1, 3, 64, 65. */
/* Training forms of the GRU gate arithmetic: forward also stores (r, z, n) [rows, 3 * hidden]; backward turns dL/dh_new into
 * dL/dgi, dL/dgh [rows, 3 * hidden] and the direct part of dL/dh_prev [rows, hidden]. */
int ssd_gru_gates_fwd(const float* gi, const float* gh, const float* h, float* h_new, float* rzn, int32_t rows, int32_t hidden, void* stream);
int ssd_gru_gates_bwd(const float* dh_new, const float* rzn, const float* gh, const float* h, float* d_gi, float* d_gh, float* dh_prev,
                      int32_t rows, int32_t hidden, void* stream);
int ssd_dueling_pick(const float* av, int32_t rows, int32_t n_actions, const uint8_t* avail, const float* epsilon, const int64_t* step,
                     uint32_t seed, int32_t n_agents, int32_t batch, int32_t pairs, int64_t* actions, float* q_out, uint32_t env_id_base,
                     void* stream);

/* ---- the learner's recurrence over all T timesteps in one launch per direction (csrc/ssd_gru_seq.hip) -----------------------
 * The GRU cell of HomophilyAgent (homophily_agent.py:162-165,188-191) unrolled from a zero state as the learner does
 * (homophily_learner.py:68-91), hidden = 64.  gi f32 [T, G, B, 192] = x_t W_i + b_i in (r, z, n) order for G independent weight
 * sets (agents x heads) and B sequences (B a multiple of 16: pad); wh [G, 64, 192], bh [G, 192]; hs f32 [G, T, B, 64] receives h_1..h_T.
 * Training: rzn [T, G, B, 192] and ghn [T, G, B, 64] (both or neither) receive the gates and the hidden-side n pre-activation.
 * Backward: dhs = dL/dhs -> d_gi [T, G, B, 192], d_wh [G, 64, 192], d_bh_part [G, ceil(B/16), 192] (partial sums per 16-row tile;
 * the caller adds them over the tile axis); dgh [G, T, B, 192] is workspace (dL/d(h W_h + b_h) per step, the operand of d_wh). */
int ssd_gru_seq_fwd(const float* gi, const float* wh, const float* bh, float* hs, float* rzn, float* ghn, int32_t T, int32_t G, int32_t B,
                    void* stream);
int ssd_gru_seq_bwd(const float* dhs, const float* hs, const float* rzn, const float* ghn, const float* wh, float* d_gi, float* dgh,
                    float* d_wh, float* d_bh_part, int32_t T, int32_t G, int32_t B, void* stream);
/* The same two launches with the input-side projections given as n_parts (1..4) separately allocated SET-MAJOR tensors
 * gi_parts[k] f32 [G / n_parts, T, B, 192] (what ssd_bias_bmm_fwd leaves for a group of weight sets; the learner passes live / target net
 * x env / inc head as they are -- no concatenation, no transpose to time-major), and their gradients written into d_gi_parts[k] of the
 * same shape (every part must be valid memory; a part that needs no gradient is scratch).  hs, rzn, ghn, dgh, d_wh, d_bh_part as above. */
int ssd_gru_seq_fwd_parts(const float* const* gi_parts, int32_t n_parts, const float* const* wh_parts, const float* const* bh_parts, int32_t n_wparts,
                          float* hs, float* rzn, float* ghn, int32_t T, int32_t G, int32_t B, void* stream);
int ssd_gru_seq_bwd_parts(const float* const* dhs_parts, const float* hs, const float* rzn, const float* ghn, const float* const* wh_parts,
                          int32_t n_wparts, float* const* d_gi_parts, int32_t n_parts, float* dgh, float* d_wh, float* d_bh_part, int32_t T, int32_t G,
                          int32_t G_grad, int32_t B, void* stream);
/* ABI 7: the recurrence weights of the _parts launches come as n_wparts (1..4) separately allocated tensors wh_parts[k] f32 [G / n_wparts, 64, 192]
 * and bh_parts[k] f32 [G / n_wparts, 192] over the sets in order (the learner: live net [2n], target net [2n] -- no concatenation per step);
 * d_wh and d_bh_part stay single outputs.  The backward walks only the first G_grad sets (a whole number of gi parts: the sets whose
 * states carry a gradient -- the live net's, the target net's follow): dhs_parts[k] f32 [G / n_parts, T, B, 64] are the gradients of the
 * states per gi part (parts past G_grad are not read), d_gi_parts past G_grad are not written, dgh [G_grad, T, B, 192],
 * d_wh [G_grad, 64, 192], d_bh_part [G_grad, tiles, 192]; hs / rzn / ghn keep the forward's shapes over all G sets. */

/* The recurrence from a GIVEN state (train_stored_state: a sampled window starts from the state the rollout stored; the reference has no
 * counterpart, its learner unrolls whole episodes from zeros).  Step 0 is not computed, it is loaded: hs[:, 0] := h0, steps 1 .. T - 1
 * run as in ssd_gru_seq_fwd_parts; gi of step 0 is never read; rzn / ghn of step 0 receive zeros.  The given state is data: the
 * backward writes zeros to d_gi of step 0 (and to dgh of step 0), adds nothing of step 0 to d_bh_part and sends no gradient into h0;
 * d_wh = sum_{t >= 1} h_{t-1}^T dL/dgh_t is the product of ssd_gru_seq_bwd_parts with hs[:, 0] = h0 (T = 1: zeros).
 * n_parts 1..4: set-major gi parts as in ssd_gru_seq_fwd_parts; n_parts 0: gi_parts[0] is ONE time-major tensor [T, G, B, 192] (the
 * form of ssd_gru_seq_fwd: ragged batches, the host pads h0 with the batch).  h0_parts: max(1, n_parts) pointers, one per gi part;
 * the state of set g (part k = g / spp, spp = G / max(1, n_parts)) and row b is the 64 floats at
 *   h0_parts[k] + (g - k * spp) * h0_set_stride + b * h0_row_stride        (elements)
 * so a contiguous [G, B, 64] is one pointer per part with strides (B * 64, 64), and the learner hands over batch["hidden"][:, 0] of
 * a [B, W, n, 128] field in place: pointers p, p + 64, p, p + 64 (live env / inc, target env / inc), set stride 128, row stride
 * W * n * 128.  Every row b < B is read (B a multiple of 16).  Kernels k_gru_seq_fwd_h0 / k_gru_seq_bwd_h0: the text of the
 * zero-state kernels compiled a second time (csrc/ssd_gru_seq_kernels.h); the compute waves issue no stores, the steps hold no row
 * predicate.
 * Refused (SSD_ERR_INVALID) like the _parts forms, and: a NULL or not 16-byte aligned h0 part; a negative h0 stride or one that is
 * not a multiple of 4 elements. */
int ssd_gru_seq_fwd_h0(const float* const* gi_parts, int32_t n_parts, const float* const* wh_parts, const float* const* bh_parts, int32_t n_wparts,
                       const float* const* h0_parts, int64_t h0_set_stride, int64_t h0_row_stride, float* hs, float* rzn, float* ghn, int32_t T,
                       int32_t G, int32_t B, void* stream);
int ssd_gru_seq_bwd_h0(const float* const* dhs_parts, const float* hs, const float* rzn, const float* ghn, const float* const* wh_parts,
                       int32_t n_wparts, float* const* d_gi_parts, int32_t n_parts, float* dgh, float* d_wh, float* d_bh_part, int32_t T, int32_t G,
                       int32_t G_grad, int32_t B, void* stream);

/* ---- the learner's per-agent affine layers (csrc/ssd_bmm.hip) ---------------------------------------------------------------
 * th.baddbmm(b, x, w) over the agent axis (homophily_agent.py:154-208: fc1, GRU input projections, dueling heads) and its backward,
 * f32 (exact-f32 MFMAs), contiguous tensors: x [n, rows, in], w [n, in, out], b [n, out], y / g [n, rows, out].
 *   fwd: y = b + x w
 *   bwd: dx = g w^T, dw = x^T g, db = column sums of g; each output nullable (dx needs w, dw / db need x); one launch --
 *        two when a long row axis (>= 4096 rows) meets few dw tiles: the rows are then cut into chunks whose partial tiles a
 *        second small launch adds in order through a 1 MiB scratch that belongs to (device, stream): launches on different streams
 *        never share one --, deterministic.  The scratch of a stream is allocated at its first launch; a stream that is going to CAPTURE
 *        such launches reserves its scratch before the capture starts (ssd_bmm_reserve_scratch; inside a capture nothing can be
 *        allocated and the launch stays unchunked).  Operand sets of 2^30 elements or more: SSD_ERR_UNSUPPORTED.  slope_of (nullable, [n, rows, in]): dx is multiplied elementwise by LeakyReLU'(.) taken from
 *        the sign of slope_of (the backward through a LeakyReLU whose OUTPUT is slope_of). */
int ssd_bias_bmm_fwd(const float* x, const float* w, const float* b, float* y, int32_t n, int32_t rows, int32_t in, int32_t out, void* stream);
/* The same layer followed by nn.LeakyReLU() (slope 0.01), as HomophilyAgent applies it to fc1 (homophily_agent.py:158,182):
 *   leaky_fwd: y = LeakyReLU(b + x w);   leaky_bwd: g is the gradient w.r.t. y, y the forward's output -- g is multiplied by
 *   LeakyReLU'(.) (taken from the sign of y) where it is loaded, then dx, dw, db as ssd_bias_bmm_bwd.  Two elementwise launches per
 *   layer and direction less. */
int ssd_bias_bmm_leaky_fwd(const float* x, const float* w, const float* b, float* y, int32_t n, int32_t rows, int32_t in, int32_t out, void* stream);
int ssd_bias_bmm_leaky_bwd(const float* g, const float* y, const float* x, const float* w, float* dx, float* dw, float* db, const float* slope_of,
                           int32_t n, int32_t rows, int32_t in, int32_t out, void* stream);
int ssd_bias_bmm_bwd(const float* g, const float* x, const float* w, float* dx, float* dw, float* db, const float* slope_of, int32_t n,
                     int32_t rows, int32_t in, int32_t out, void* stream);
/* ---- ABI 7: the dueling heads of the learner as ONE layer per head + one dueling launch ---------------------------------------------
 * The reference evaluates the advantage and the value layer of a head separately (homophily_agent.py:166-170,202-207) and, for the
 * incentive head, on materialised rows [h_i | other_j] of every ordered pair (:194-201).  Here the two layers are the columns 0..K-1 and K
 * of one weight [n, in, K + 1] (the caller concatenates the parameters once per step), and the pair rows are never built:
 *   ssd_bias_bmm2_fwd    y[g][r] = b[g] + [x1[g][r / x1_div] | x2[(g)][r]] w[g]: TWO-SOURCE rows -- columns [0, in1) from x1 f32
 *                        [n, rows / x1_div, in1] (h_i, the same for the x1_div receivers j), columns [in1, in1 + in2) from x2 f32
 *                        [rows, in2] shared by all weight sets (x2_shared) or [n, rows, in2]; in1 a multiple of 16.
 *   ssd_bias_bmm2_bwd_w  dw [n, in1 + in2, out] = rows^T g and db = column sums of g for the same two-source rows (either nullable).
 *   ssd_bias_bmm_bwd_x   dx [n, rows, in] = g w^T where w[g] are the LEADING `in` rows of a wider layer (w_set floats between two weight sets):
 *                        the gradient of x1 from the row-group sums of g (ssd_dueling_head_bwd's gs).
 *   ssd_dueling_head_fwd q [B, T, n, inner, K] = v + a - mean_k a from y f32 [n, T * B * inner, K + 1] (a = columns 0..K-1, v = column K).
 *   ssd_dueling_head_bwd dq -> dy (same shape as y: da = dq - mean_k dq, dv = sum_k dq) and, when gs is given, gs f32 [n, T * B, K + 1] =
 *                        the sum of dy over the `inner` rows of every (agent, t, b) in row order (deterministic). */
int ssd_bias_bmm2_fwd(const float* x1, const float* x2, const float* w, const float* b, float* y, int32_t n, int32_t rows, int32_t in1, int32_t in2,
                      int32_t out, int32_t x1_div, int32_t x2_shared, void* stream);
int ssd_bias_bmm2_bwd_w(const float* g, const float* x1, const float* x2, float* dw, float* db, int32_t n, int32_t rows, int32_t in1, int32_t in2,
                        int32_t out, int32_t x1_div, int32_t x2_shared, void* stream);
int ssd_bias_bmm_bwd_x(const float* g, const float* w, float* dx, int32_t n, int32_t rows, int32_t in, int32_t out, int64_t w_set, void* stream);
int ssd_dueling_head_fwd(const float* y, float* q, int32_t n, int32_t T, int32_t B, int32_t inner, int32_t K, void* stream);
int ssd_dueling_head_bwd(const float* dq, float* dy, float* gs, int32_t n, int32_t T, int32_t B, int32_t inner, int32_t K, void* stream);
/* Make the row-chunk scratch of `stream` on the current device exist (SSD_ERR_DEVICE when it cannot be allocated). */
int ssd_bmm_reserve_scratch(void* stream);
/* Arithmetic of the LEARNER's matrix products from now on (process-wide; a launch takes the value at launch -- or capture -- time):
 *   2 (default)  f32: ssd_bias_bmm_* on exact-f32 MFMAs, ssd_gru_seq_* on two- / three-term split products (f32-equivalent);
 *   1            the labelled reduced-precision variant (config key learner_dtype: bf16): operands rounded to bf16, ONE
 *                v_mfma_f32_16x16x32_bf16 per 32 reduction indices in ssd_bias_bmm_fwd / _bwd (dx, dw), ssd_gru_seq_fwd / _bwd and
 *                the weight gradient of W_h; f32 accumulation, f32 parameters / optimiser state / loss.  The learner's encoder
 *                forward (ssd_policy_encode with `act`) takes precision 1 fragment images from ssd_policy_pack_encoder.
 * SSD_ERR_INVALID for any other value. */
int ssd_set_learner_precision(int32_t precision);
int ssd_learner_precision(void);

/* Weight (and bias) gradient of the encoder's Conv2d(3, 6, 3) on windows given as SSD_OBS_CODE class codes u8 [rows, V, V]
 * (V odd, 3 .. 63; ABI 9: every edge, before 15 / 31 only): d_conv = dL/d(conv output) f32 [rows, 6, V-2, V-2] -> partial f32 [ssd_conv_wgrad_partial_rows(rows), 168]: per
 * wave, 162 weight-gradient sums in conv_w order [oc][ch][dy][dx] (the planes' 255/256 included) followed by the 6 bias sums; the
 * caller adds the rows (ssd_column_sums).  Rows past the last wave's windows are written as zeros. */
#define SSD_CONV_WGRAD_COLS 168
int ssd_conv_wgrad_partial_rows(int32_t rows);
int ssd_conv_wgrad_codes(const uint8_t* codes, const float* d_conv, float* partial, int32_t rows, int32_t view_edge, void* stream);

/* ---- fused rollout-time controller step (csrc/ssd_policy_mfma.hip) -------------------------------------------------------
 * What HomophilyMAC.select_actions_env / select_actions_inc evaluate (homophily_controller.py:30-65, 127-184 on top of
 * homophily_agent.py:20-27,154-214 and action_selectors.py:44-68) as THREE launches per timestep:
 *   ssd_policy_encode   rgb_preprocess: Conv2d(3, 6, 3) + LeakyReLU + Flatten + Linear(6 (V-2)^2, 32) [+ LeakyReLU]
 *   ssd_policy_head_env input tail (one-hot last action, agent id, sign of last reward, sign of received incentives, pos / scale)
 *                       -> fc1_env + LeakyReLU -> GRU cell -> dueling Q -> epsilon-greedy over the available actions
 *   ssd_policy_head_inc [inputs | one-hot(action)] -> fc1_inc + LeakyReLU -> GRU cell -> per ordered pair (i -> j)
 *                       [h_i | one-hot(a_j), pos_j / scale, orient_j, r_j, clean_j, apple_den_j] -> dueling Q -> epsilon-greedy, diagonal 0
 * All matrix products run on the 16-bit matrix cores (v_mfma_f32_16x16x32_{f16,bf16}, f32 accumulate).  `precision`:
 *   2  f32-equivalent (the default, the reference's dtype): every f32 operand is split into two f16 terms x = hi + lo (22
 *      significand bits) and a product is evaluated as hi*hi + hi*lo + lo*hi -- three MFMAs; the one-hot observation planes are exact
 *      in f16, so the conv needs two.  Weights and activations carry exact power-of-two scales that keep the lo terms in the normal
 *      f16 range; measured deviation from the reference's f32 Q-values < 1e-5 (tests/test_policy_mfma.py).
 *   1  bf16: single bf16 terms, one MFMA per product (the "bf16 Q-net" of BASELINE.json configs[1]; rollout inference only).
 * hidden = 64, n_feat = 32, conv_out = 6 are fixed (config/default.yaml:44,59-63).
 *
 * Weights are passed as kernel-ready FRAGMENT IMAGES built on the device by ssd_policy_pack_* from the reference-shaped f32
 * parameters (names and shapes of homophily_agent.py:37-125, [1, n, in, out] contiguous).  A fragment is the A operand of one
 * MFMA: 64 lanes x 8 values, lane l = (q = l >> 4, m = l & 15) holding row m of a 16-row output tile at the 8 reduction indices of
 * its quarter q -- 1 KiB, read by one ds_read_b128 / global_load_dwordx4 per lane.  All products are computed TRANSPOSED
 * (D^T = W^T X^T: the weight is the A operand, 16 activation rows are the B operand), and the reduction index of step s, quarter q,
 * element j is k = 32 s + 16 (j >> 2) + 4 q + (j & 3), which makes an MFMA result tile the B operand of the next product without
 * any lane movement (fc1 -> GRU -> dueling chain in registers).
 *
 * Head image (per agent, SSD_POLICY_IMAGE_BYTES(precision) bytes, 16-byte aligned), stored IN THE ORDER THE HEAD KERNEL CONSUMES IT in
 * pieces of 1 KiB (one LDS-DMA wave instruction each), 8 pieces to a chunk: the kernel STREAMS the image through a small ring in LDS
 * behind its own arithmetic (a head workgroup holds 48 KiB of it at a time, not 118 KB):
 *   per K-STEP c < 14 of the chain, [term t < precision][output tile ot < 4] fragments at piece 4 precision c + 4 t + ot:
 *     c = s: fc1 (s = the 32-deep half of the reduction); c = 2 + 2 g + s: GRU input side, gate g = r, z, n; c = 8 + 2 g + s: hidden side;
 *   then the resident chunk (8 pieces from piece 56 precision): fc2's [term t][s < 2] fragments (advantage rows, then the value row;
 *     inc: the h part) at + 2 t + s; the f32 tail at + 2 precision -- biases fc1[64] gru_i[192] gru_h[192] fc2[16], then (inc) the pair
 *     part of fc2 f32 [16 extra features][4] -- zero-padded to SSD_POLICY_TAIL_PIECES pieces; zero padding to the end of the chunk.
 * Activations are agent-major: inputs f32 [n, n_env, 64] (columns 0..31 = encoder output; the env head fills 32..63: tail then
 * zeros), h f32 [n, n_env, 64] updated in place. q_out (nullable): env f32 [n, n_env, n_actions]; inc f32 [n, n_env, n, 3].
 * Exploration draws: the package's counter generator keyed by (seed, *step, GLOBAL env id = env_id_base + env, agent[, j]) --
 * a shard of a larger job draws what the unsharded job draws for the same envs (ssd_dueling_pick uses the same key).
 * The generator (csrc/ssd_policy_common.h: dueling_pick_bits; restated on the host by tests/explore_util.py, which every pick site
 * equals bit for bit -- tests/test_exploration_draws.py), all arithmetic in uint32 unless said otherwise:
 *   mix32p(x): x ^= x>>17; x *= 0xed5ad4bb; x ^= x>>11; x *= 0xac4c1b51; x ^= x>>15; x *= 0x31848bab; x ^= x>>14
 *   x0 = mix32p(seed ^ mix32p(u32(step) * 0x9E3779B9 + key));   x1 = mix32p(x0 ^ 0x85EBCA6B)
 *   explore  <=>  f32(x0 >> 8) * 2^-24 < eps           (f32 compare; eps is the f32 device scalar: never for eps <= 0 or NaN,
 *                                                       always for eps >= 1)
 *   with ssd_policy_head.epsilon_rows (a rate per env, e.g. the Ape-X ladder eps^(1 + alpha g / (G - 1))): row b -- the LOCAL env
 *   index of the launch -- of both heads
 *   explore  <=>  f32(x0 >> 8) * 2^-24 < epsilon_rows[b]    (the same f32 compare; `epsilon` stays required and is not read for
 *                                                       the rows; key, seed, step, pick, greedy rule and the inc head's zero
 *                                                       diagonal are unchanged; ssd_dueling_pick has the scalar only)
 *   pick =(u64(x1) * popcount(live)) >> 32  ->  the pick-th lowest AVAILABLE action;  no action available: the greedy result
 *   key  = (env_id_base + b) * n + i                    env head
 *   key  = ((env_id_base + b) * n + i) * n + j          inc head (diagonal forced to 0 afterwards, draw or not)
 *   seed = ssd_policy_head.seed (FastPolicy: its seed for the env head, seed ^ 0x5bd1e995 for the inc head);  step = *step mod 2^32
 *   greedy = first maximum of v + a_k - mean(a) over the available k (action 0 when none is available)
 * The rollout advances *step once per timestep slot, the closing slot T included, and never resets it: the four-launch timestep's
 * encoder before the heads read it (ssd_policy_encode_args.counter_inc), the pipelined timestep's inc head after they did
 * (next_step_out) from a counter that starts at RunnerPlan.counter_start -- one ahead wherever a four-launch sequence exists to
 * be matched (every window edge but 15 / 31, and the gathered layouts), so that slot t of episode e draws at step
 * 1 + e (T + 1) + t in both; the pipelined dense timestep at 15 / 31 starts at 0 and draws at e (T + 1) + t. */
#define SSD_POLICY_HEAD_FRAGS 58
#define SSD_POLICY_HEAD_TAIL_FLOATS (464 + 64)
#define SSD_POLICY_TAIL_PIECES 3
#define SSD_POLICY_IMAGE_PIECES(precision) (56 * (precision) + 8)              /* 14 K-steps x 4 precision pieces + the resident chunk */
#define SSD_POLICY_IMAGE_BYTES(precision) (SSD_POLICY_IMAGE_PIECES(precision) * 1024)
typedef struct ssd_policy_head {
    int32_t n_env, n_agents, n_actions, input_shape;
    float pos_scale;
    uint32_t seed;
    float* inputs;                 /* [n, n_env, 64] */
    float* h;                      /* [n, n_env, 64] */
    const void* weights;           /* [n, SSD_POLICY_IMAGE_BYTES(precision)] from ssd_policy_pack_head */
    const uint8_t* avail;          /* env: u8 [n_actions] or NULL */
    const float* epsilon;          /* device scalar */
    const int64_t* step;           /* device scalar */
    /* env head: previous timestep (last action -1 = none) and the current position */
    const int64_t* prev_actions;   /* [n_env, n] */
    const float* prev_reward;      /* [n_env, n] */
    const int64_t* prev_actions_inc; /* [n_env, n, n] */
    const float* pos;              /* [n_env, n, 2] */
    /* inc head: the env actions just taken, the PRE-step pose and this step's outcome */
    const int64_t* actions;        /* [n_env, n] */
    const float *pos_pre, *orient_pre;   /* [n_env, n, 2] */
    const float *reward, *clean_num, *apple_den;   /* [n_env, n] */
    int64_t* out_actions;          /* env: [n_env, n]; inc: [n_env, n, n] */
    float* q_out;                  /* nullable */
    /* env head, optional by-products for the runner (all nullable): the actions again as int32 (the env's action type), and
     * copies of the current pose (pos, orient [n_env, n, 2]) taken before the env step overwrites it */
    const float* orient;
    int32_t* out_actions_i32;
    float *pos_copy, *orient_copy;
    /* Optional: the head also files its results in the episode storage [n_env, t_slots, ...] at time slot *t_index (what
     * ssd_store_step_launch does as a separate launch; every pointer nullable = skipped; nothing is filed when *t_index >= t_slots),
     * and carries the runner state:
     *   env head: dst_actions, dst_actions_onehot, dst_pos, dst_orient (the current pose), prev_actions_out <- actions
     *   inc head: dst_actions_inc, prev_actions_inc_out <- actions_inc; dst_reward / dst_clean_num / dst_apple_den /
     *             dst_terminated <- this step's reward, clean_num, apple_den, terminated; prev_reward_out <- reward;
     *             ep_return += reward; *next_t_out = *t_index + 1 (next_t_out must not alias t_index). */
    const int64_t* t_index;
    int32_t t_slots;
    float *dst_pos, *dst_orient, *dst_actions_onehot, *dst_reward, *dst_clean_num, *dst_apple_den;
    uint8_t* dst_terminated;
    const uint8_t* terminated;     /* [n_env] */
    int64_t *dst_actions, *dst_actions_inc;
    int64_t *prev_actions_out, *prev_actions_inc_out;
    float *prev_reward_out, *ep_return;
    int64_t* next_t_out;
    /* ---- ABI 2 ---- */
    int32_t precision;             /* 2 (f32-equivalent, default when 0) or 1 (bf16) -- must match the image */
    uint32_t env_id_base;          /* global id of env 0 of this shard (exploration key) */
    /* env head: the encoder's unfinished output (ssd_policy_encode with bands > 1): features = LeakyReLU(lin_b + sum over bands
     * of feat_part[band][agent-major row][32]); written to inputs[:, 0..31] by this launch.  NULL: inputs[:, 0..31] are final. */
    const float* feat_part;
    int32_t feat_bands;
    const float* lin_b;            /* [32] */
    /* ---- ABI 3 ---- */
    /* env head: which blocks _build_inputs appends after the 32 encoder features (homophily_controller.py:137-184, in that order;
     * SSD_INPUT_* bits, or-ed with SSD_INPUT_EXPLICIT so that the empty set can be told from 0).  0 = SSD_INPUT_FLAGS_SHIPPED
     * (config/default.yaml).  input_shape must equal 32 + the blocks' widths and
     * input_shape + n_actions <= 64.  SSD_INPUT_OTHERS_LAST_ACTION (both heads): the block's n * n_actions columns are not columns of
     * the 64-column image -- see others_rows below; input_shape is then the reference's full width (32 + all set blocks) and the limit
     * is on the DENSE width: input_shape - n * n_actions + n_actions <= 64. */
    uint32_t input_flags;
    /* Counter hand-over of the pipelined rollout (all nullable).  inc head: *next_step_out = *step + 1 (like next_t_out for the time
     * index).  env head: *t_copy_out = *t_index, *step_copy_out = *step.  A launch never writes a scalar that it reads: the env head
     * reads the masters and writes the copies, the inc head reads the copies and writes the masters. */
    int64_t *next_step_out, *t_copy_out, *step_copy_out;
    /* ---- ABI 7 ---- */
    /* Compact runner state for the env head's input phase (all optional).  recv_inc: the previous step's incentive actions as
     * RECEIVER-major bytes u8 [n(receiver), n_env, 16] (byte g = what giver g sent this receiver: 0 / 1 / 2; the receiver's own byte
     * and bytes >= n are 0): when given, the env head reads it instead of prev_actions_inc [n_env, n(giver), n(receiver)] i64 -- one
     * 4-byte load per lane over 256 contiguous bytes per 16-row tile instead of n 8-byte loads over n x 16 cache lines.
     * recv_inc_out: the inc head writes byte `agent` of every receiver's record next to prev_actions_inc_out (the caller zeroes the
     * array when an episode opens, like prev_actions_inc).  avail_bits: bit 31 set = bits 0 .. n_actions - 1 ARE the availability
     * mask of `avail` (a constant of the env class): the env head then issues no loads for it. */
    const uint8_t* recv_inc;
    uint8_t* recv_inc_out;
    uint32_t avail_bits;
    /* ---- appended in ABI 10 (zero = as before) ---- */
    /* obs_others_last_action (input_flags has SSD_INPUT_OTHERS_LAST_ACTION; env head and inc head).  The block is n one-hot vectors,
     * so its product with fc1 is a sum of n weight rows: the heads add others_rows[agent][g * n_actions + a_g][0..63] for every agent g
     * with a previous action a_g >= 0 to fc1's output (exact f32 rows, both precisions); the six dense blocks occupy compacted
     * columns of `inputs` and of the image as if the block were absent (the inc head's one-hot action follows them).
     *   others_rows      f32 [n(owner), n * n_actions, 64] from ssd_policy_pack_head, 16-byte aligned
     *   prev_record      every agent's previous env action as one byte per agent, 16 bytes per env (u8 [n_env, 16]; 0xFF = no previous
     *                    step; bytes >= n unused), 16-byte aligned: what this timestep READS (both heads of a timestep read the same)
     *   prev_record_out  env head, nullable: byte `agent` of every env's record <- the action picked.  It must be the OTHER buffer of a
     *                    pair selected by the timestep's parity: the workgroups of the other agents read prev_record in the same
     *                    launch, and the inc head of this timestep still reads it afterwards.
     * Missing others_rows / prev_record, n_agents > SSD_MAX_AGENTS, prev_record_out on the inc head or equal to prev_record:
     * SSD_ERR_INVALID.  ssd_policy_head_inc_encode refuses the flag (SSD_ERR_UNSUPPORTED): these configurations take the four
     * standalone launches per timestep, or ssd_policy_head_inc_encode with pipeline_gather as their third of three. */
    const float* others_rows;
    const uint8_t* prev_record;
    uint8_t* prev_record_out;
    /* ---- appended for SSD_INPUT_GATHER_ONEHOT (zero = as before) ---- */
    /* input_flags has SSD_INPUT_GATHER_ONEHOT (env head and inc head): EVERY one-hot block leaves the 64-column image -- the agent's
     * own last action, the agent id, the others' last actions (if SSD_INPUT_OTHERS_LAST_ACTION is set too) and the inc head's one-hot
     * of the action just chosen.  Each is one row of fc1 per one-hot vector, added as exact f32 where the bias is added.  The dense
     * blocks (32 features | sign r | sign inc | distances | pos, each iff flagged: at most 46 columns at n = 10) occupy compacted
     * columns of `inputs` and of the image, zeros behind them; input_shape is the reference's full width.
     *   onehot_rows   f32 [n(owner), SSD_ONEHOT_ROWS(n, n_actions, flags), 64] from ssd_policy_pack_head, 16-byte aligned; per owner:
     *                 row 0 = fc1's row of the owner's agent-id column (zeros without SSD_INPUT_AGENT_ID; constant per agent, so it
     *                 acts as a second bias row), rows 1 .. A = the last-action block (zeros without SSD_INPUT_LAST_ACTION), rows
     *                 1 + A .. 2A = the inc head's action block (zeros in the env head's table), then the n * A rows of the others'
     *                 last-action block if flagged.
     *   prev_record / prev_record_out as above: byte `agent` is the agent's own previous action (prev_actions is not read for the
     *                 input row), 0xFF / any value outside [0, n_actions) adds zeros.  others_rows is not used.
     * Missing onehot_rows / prev_record, misalignment, n_agents > SSD_MAX_AGENTS, prev_record_out on the inc head or equal to
     * prev_record: SSD_ERR_INVALID.  input_shape != 32 + the widths of all flagged blocks: SSD_ERR_UNSUPPORTED.
     * ssd_policy_head_inc_encode refuses the bit (SSD_ERR_UNSUPPORTED) unless pipeline_gather is set. */
    const float* onehot_rows;
    /* ---- appended for the pipelined launch of the gathered layouts (zero = as before) ---- */
    int32_t pipeline_gather;       /* read by ssd_policy_head_inc_encode only: nonzero = take the gathered fused launch (declared below
                                      the encoder's arguments) for a head that carries one of the two gather bits */
    /* ---- appended for a rate per env (zero = as before: every row explores at *epsilon) ---- */
    const float* epsilon_rows;     /* nullable: f32 [n_env], 4-byte aligned.  Row b (local env index) of ssd_policy_head_env,
                                      ssd_policy_head_inc and every path of ssd_policy_head_inc_encode (dense, any-view, gathered)
                                      explores at epsilon_rows[b] instead of *epsilon ("Exploration draws" above).  Misaligned:
                                      SSD_ERR_INVALID. */
} ssd_policy_head;
#define SSD_INPUT_LAST_ACTION 1u   /* obs_last_action: one-hot of the previous env action, n_actions columns */
#define SSD_INPUT_AGENT_ID    2u   /* obs_agent_id: one-hot of the agent, n columns */
#define SSD_INPUT_REWARD      4u   /* obs_reward: sign of the previous reward */
#define SSD_INPUT_INC_REWARD  8u   /* obs_inc_reward: sign(#rewards - #punishments received at the previous step) */
#define SSD_INPUT_DISTANCE    16u  /* obs_distance: 1 - |pos - pos_g| / pos_scale for every agent g, n columns */
#define SSD_INPUT_AGENT_POS   32u  /* obs_agent_pos: pos / pos_scale, 2 columns */
#define SSD_INPUT_OTHERS_LAST_ACTION 64u   /* obs_others_last_action: every agent's last-action one-hot, n * n_actions columns, between
                                             the received-incentive sign and the distances -- ssd_build_inputs_flags builds the columns;
                                             the fused heads gather fc1's rows instead (ssd_policy_head.others_rows) */
#define SSD_INPUT_GATHER_ONEHOT 0x100u   /* not a block: the LAYOUT in which the fused heads gather fc1's rows for every one-hot block
                                           (ssd_policy_head.onehot_rows) -- any flag set then fits the 64-column image at n <= 10.
                                           (0x80 stays unassigned: no head builds it.) */
#define SSD_ONEHOT_ROWS(n, A, flags) (1 + 2 * (A) + (((flags) & SSD_INPUT_OTHERS_LAST_ACTION) ? (n) * (A) : 0))
#define SSD_INPUT_EXPLICIT    0x80000000u   /* marks a given flag word (the empty set is SSD_INPUT_EXPLICIT alone) */
#define SSD_INPUT_FLAGS_SHIPPED (SSD_INPUT_LAST_ACTION | SSD_INPUT_AGENT_ID | SSD_INPUT_REWARD | SSD_INPUT_INC_REWARD | SSD_INPUT_AGENT_POS)
/* ssd_build_inputs for ANY _build_inputs flag set (homophily_controller.py:137-184; the learner's time-batched input assembly):
 * input_flags as in ssd_policy_head (0 = the shipped set) plus SSD_INPUT_OTHERS_LAST_ACTION.  Writes the blocks, in the reference's
 * order, into out[:, out_offset : out_offset + width]; width = ssd_build_inputs_width(...). */
int ssd_build_inputs_width(int32_t n_agents, int32_t n_actions, uint32_t input_flags);
int ssd_build_inputs_flags(int32_t batch, int32_t n_agents, int32_t n_actions, int32_t t0, uint32_t input_flags,
                           const int64_t* last_actions, const float* last_reward, const int64_t* last_actions_inc, const float* pos,
                           float pos_scale, float* out, int32_t out_stride, int32_t out_offset, void* stream);
int ssd_policy_head_env(const ssd_policy_head* args, void* stream);
int ssd_policy_head_inc(const ssd_policy_head* args, void* stream);
/* How a head launch of (n_env, n_agents) is cut on the current device: workgroups per agent, compute waves per workgroup (a 16-row
 * tile each) and the number of tiles the busiest wave walks -- 1 while the grid fits the chip (the kernels without a back edge),
 * more beyond (Cleanup-10 x 8192: the looped instantiations).  fused_with_encoder selects the launch: 0 = the standalone heads of
 * the dense input layouts (8 compute waves), 1 = the inc head inside ssd_policy_head_inc_encode (7; with pipeline_gather: the same
 * cut, always walked by the looped head), 2 = the standalone heads of the gathered layouts (SSD_INPUT_OTHERS_LAST_ACTION /
 * SSD_INPUT_GATHER_ONEHOT: 7 compute waves, so they loop from a smaller n_env on).  Any other value is SSD_ERR_INVALID. */
int ssd_policy_head_plan(int32_t n_env, int32_t n_agents, int32_t fused_with_encoder, int32_t* workgroups_per_agent, int32_t* compute_waves,
                         int32_t* tiles_per_wave);
/* The inc head of timestep t and ssd_policy_encode of timestep t + 1 as ONE launch (declared below the encoder's arguments):
 * ssd_policy_head_inc_encode. */

/* The reference-shaped parameters of one head (homophily_agent.py:37-125; every tensor [1, n, in, out] / [1, n, 1, out] f32,
 * contiguous, device memory).  w_i / w_h / b_i / b_h in (r, z, n) order.  env: fc1_in = input_shape, fc2_in = 64, fc2_out = n_actions;
 * inc: fc1_in = input_shape + n_actions, fc2_in = 64 + n_actions + 7, fc2_out = 3. */
typedef struct ssd_policy_head_params {
    const float *fc1_w, *fc1_b;
    const float *w_i[3], *w_h[3], *b_i[3], *b_h[3];
    const float *fc2_w, *fc2_b, *fc2_v_w, *fc2_v_b;
    int32_t n_agents, fc1_in, fc2_in, fc2_out;
    /* ---- appended in ABI 10 (zero = as before) ---- */
    /* input_flags with SSD_INPUT_OTHERS_LAST_ACTION (SSD_INPUT_* of the controller's flag set; n_actions = the env's action count):
     * fc1_in is the reference's full width (inc: + n_actions).  The rows of fc1_w on both sides of the others' last-action block are
     * packed into the 64-column image in compacted order (fc1_in - n_agents * n_actions <= 64), the block's n_agents * n_actions rows
     * are written as they are to others_rows f32 [n, n_agents * n_actions, 64] (16-byte aligned) by the same launch. */
    uint32_t input_flags;
    int32_t n_actions;
    float* others_rows;
    /* ---- appended for SSD_INPUT_GATHER_ONEHOT (zero = as before) ---- */
    /* input_flags with SSD_INPUT_GATHER_ONEHOT: fc1_in is the reference's full width (env head) or that + n_actions (inc head);
     * anything else is SSD_ERR_UNSUPPORTED.  The rows of the dense blocks are packed into the image in compacted order and the
     * one-hot blocks' rows are written to onehot_rows f32 [n, SSD_ONEHOT_ROWS, 64] (layout: ssd_policy_head.onehot_rows; 16-byte
     * aligned, null: SSD_ERR_INVALID) by the same launch.  others_rows is not used.  Images of every other layout are unchanged. */
    float* onehot_rows;
} ssd_policy_head_params;
/* image: [n, SSD_POLICY_IMAGE_BYTES(precision)] */
int ssd_policy_pack_head(const ssd_policy_head_params* params, int32_t precision, void* image, void* stream);

/* ssd_policy_encode: rgb_preprocess for odd window edges V = 3 .. 63 (view_size 1 .. 31) of the SIMPLIFIED palette: the Toeplitz layout
 * below for 15 x 15 (view_size 7) and 31 x 31 (view_size 15) windows, the class-LUT layout (SSD_ENCODE_LAYOUT_LUT) for every edge
 * (ABI 9; other edges than 15 / 31 with `act` too: the learner's training forward there).  Even edges, V < 3 and V > 63 are refused.
 * Input: one byte per window cell in either alphabet (`alphabet`: SSD_CODE_CLASS = the SSD_OBS_CODE classes of an episode storage,
 * SSD_CODE_CHANNEL_MASK = the side buffer of ssd_obs_out.obs_code); the three colour planes are rebuilt in LDS as one-hot bytes, so the
 * conv is a banded (Toeplitz) GEMM over 16 batch rows per MFMA and the whole encoder runs on the matrix cores:
 *   conv   D[(2 output channels) x (8 positions of an output row)][16 batch rows] += A[.][K] x B[K][batch rows] per input row dy:
 *          K = 3 planes x the 10-cell window of the 8 positions, laid out as three quarters of 8 cells + a "tail" quarter that holds
 *          cells 8, 9 of the three planes (30 of 32 K entries carry data; 9 of them are taps of a given output).
 *          A = Toeplitz image of the 3 x 3 taps (ssd_policy_pack_encoder), B = plane bytes read from LDS (one ds_read_b64 + 4 v_perm)
 *   Linear two neighbouring conv result tiles (16 positions x 2 channels) ARE the B operand of a Linear K-step (no transposition,
 *          no LDS)
 * The class of row (env b, agent i) cell c is read at codes[b * env_stride + (*slot_t) * slot_stride + i * agent_stride + c]
 * (slot_t NULL: slot 0): the dense side buffer of ssd_obs_out.obs_code (env_stride = n * agent_stride, slot_stride = 0) or an
 * episode storage of class codes u8 [n_env, t_slots, n, V, V] (agent_stride = V * V).  code_bytes = readable bytes behind `codes`;
 * the kernel reads whole aligned 4-byte words, never one that holds no byte of [codes, codes + code_bytes).
 * Output rows are agent-major (i * n_env + b) when agent_major, else (b * n + i).
 *   V = 15: one launch computes the whole Linear sum; out[row * out_stride + 0..31] = LeakyReLU(. + lin_b)   (part = NULL)
 *   V = 31: the 29 output rows are cut into SSD_ENCODE_BANDS(31) = 3 bands evaluated by different workgroups; band k writes its
 *           partial Linear sum to part[k][row][32] and the consumer (ssd_policy_head_env: feat_part / feat_bands / lin_b) adds
 *           them in band order, adds the bias and applies the LeakyReLU (out = NULL).
 * slot_t_copy (nullable) receives *slot_t: a second copy of the time index for the kernels that file results and advance slot_t
 * (ssd_policy_head.t_index / next_t_out, ssd_store_step_launch).  counter_inc (nullable): *counter_inc += 1 (the exploration-draw
 * counter read by the heads that follow; this kernel does not read it).
 * Fragment images (ssd_policy_pack_encoder from conv_w f32 [6, 3, 3, 3] and lin_w f32 [32, 6 (V-2)^2]):
 *   conv_frags [term][s 3][dy 3][lane][8]: element (q, m, j) = tap weight w[oc][ch][dy][d] * 255/256, oc = 2 s + (m >> 3),
 *              position p = m & 7; q < 3: ch = q, cell = j; q = 3: ch = j >> 1, cell = 8 + (j & 1) (j < 6); d = cell - p in 0..2, else 0
 *   lin_frags  [unit = ((y * XTP + xtp) * 3 + s)][output tile 2][term][lane][8]: element (q, m, j) = lin_w[16 Mt + m][oc * P + y * O + x],
 *              r = 4 q + (j & 3), oc = 2 s + (r >> 3), x = 8 (2 xtp + (j >> 2)) + (r & 7), 0 where x >= O   (XTP = 1 / 2 pairs of
 *              8-position tiles per output row) */
/* SSD_ENCODE_LAYOUT_LUT (ssd_policy_encode_args.layout; at 15 / 31 launches without `act`): the CONVOLUTION AS A TABLE SUM.  A window cell is one
 * of four classes and lights at most one plane at 255/256, so the three taps of input row dy contribute to all six channels a value
 * that depends only on the three classes under them: conv[c](y, x) = sum_dy T[dy][cls(y+dy, x) + 4 cls(y+dy, x+1) + 16 cls(y+dy, x+2)][c]
 * (T[0] carries the bias) -- exact f32 sums of entries built by ssd_policy_pack_encoder_lut, no matrix-core work for the conv.  Images:
 *   conv_frags = the table f32 [3 dy][64 idx][6 channels] (SSD_ENCODE_LUT_TABLE_BYTES; precision 2: scaled by 256, the split scale of
 *                the conv activations), classes as in SSD_OBS_CODE (2 waste -> R, 1 apple -> G, 3 wall / agent -> B);
 *   lin_frags  = [K-step gs][output tile 2][term][lane][8] with K-steps numbered through the bands (band k: ceil(rows_k * O / 4) of
 *                them, SSD_ENCODE_LUT_KSTEPS(V) in all): element (q, m, j) = lin_w[16 Mt + m][j * P + y * O + x] for j < 6, the position
 *                p = 4 s + q of the band (s = gs - the band's first K-step; y = band * R + p / O, x = p mod O), 0 for j >= 6 and past the band.
 * The kernel keeps the window rows in LDS as packed 2-bit classes; lane (q, m) evaluates position 4 s + q of batch row m and its six
 * channel values ARE its B operand of the Linear's K-step s: 258 MFMAs per 16-row tile (15 x 15) instead of 702. */
#define SSD_ENCODE_LAYOUT_TOEPLITZ 0
#define SSD_ENCODE_LAYOUT_LUT 1
#define SSD_ENCODE_LUT_TABLE_BYTES (3 * 64 * 6 * 4)
/* Band geometry of an odd window edge V = 3 .. 63 (O = V - 2 output rows): O <= 13 is one band; else ceil(O / 10) bands, at most 6
 * (the env head folds at most 6 band sums), of SSD_ENCODE_BAND_ROWS(V) = ceil(O / bands) rows, the last band holding the rest.
 * 15 -> 1 band of 13 rows, 31 -> 3 bands of 10 rows, 63 -> 6 bands of 11 rows. */
#define SSD_ENCODE_EDGE_MIN 3
#define SSD_ENCODE_EDGE_MAX 63
#define SSD_ENCODE_BANDS_MAX 6
#define SSD_ENCODE_NB0_(O) ((O) <= 13 ? 1 : ((O) + 9) / 10 < SSD_ENCODE_BANDS_MAX ? ((O) + 9) / 10 : SSD_ENCODE_BANDS_MAX)
#define SSD_ENCODE_BAND_ROWS(V) (((V) - 2 + SSD_ENCODE_NB0_((V) - 2) - 1) / SSD_ENCODE_NB0_((V) - 2))
#define SSD_ENCODE_BANDS(V) (((V) - 2 + SSD_ENCODE_BAND_ROWS(V) - 1) / SSD_ENCODE_BAND_ROWS(V))
/* K-steps of 4 positions: ceil(R * O / 4) per full band, ceil(rows of the last band * O / 4) for the last (15 -> 43, 31 -> 212) */
#define SSD_ENCODE_LUT_KSTEPS(V)                                                                                                   \
    ((SSD_ENCODE_BANDS(V) - 1) * ((SSD_ENCODE_BAND_ROWS(V) * ((V) - 2) + 3) / 4) +                                                 \
     (((V) - 2 - (SSD_ENCODE_BANDS(V) - 1) * SSD_ENCODE_BAND_ROWS(V)) * ((V) - 2) + 3) / 4)
#define SSD_ENCODE_LUT_LIN_BYTES(V, precision) (SSD_ENCODE_LUT_KSTEPS(V) * 2 * (precision) * 1024)
#define SSD_ENCODE_UNITS(V) ((V) == 31 ? 29 * 2 * 3 : 13 * 1 * 3)
#define SSD_ENCODE_CONV_FRAG_BYTES(V, precision) ((precision) * 9 * 1024)
#define SSD_ENCODE_LIN_FRAG_BYTES(V, precision) (SSD_ENCODE_UNITS(V) * 2 * (precision) * 1024)
typedef struct ssd_policy_encode_args {
    const uint8_t* codes;
    int64_t code_bytes, env_stride, slot_stride, agent_stride;
    const int64_t* slot_t;
    int32_t rows, view_edge, n_agents, agent_major, precision;
    const void *conv_frags, *lin_frags;
    const float *conv_b, *lin_b;
    float* out; int32_t out_stride;
    float* part;
    int64_t* slot_t_copy;
    int64_t* counter_inc;
    int32_t alphabet;              /* SSD_CODE_CLASS / SSD_CODE_CHANNEL_MASK */
    float* act;                    /* nullable (precision 2 only): LeakyReLU(conv) f32 [rows, 6, V-2, V-2], row = b * n + i: the
                                      activations the learner's backward needs (the training forward of the encoder) */
    int32_t slot_add;              /* the time slot read is *slot_t + slot_add (the pipelined rollout encodes slot t + 1 while the
                                      device time index still says t); the caller keeps it inside the storage */
    int32_t layout;                /* ABI 7: SSD_ENCODE_LAYOUT_TOEPLITZ (0: images of ssd_policy_pack_encoder; V = 15 / 31) or
                                      SSD_ENCODE_LAYOUT_LUT (images of ssd_policy_pack_encoder_lut; with `act` only for V other than 15 / 31) */
} ssd_policy_encode_args;
int ssd_policy_encode(const ssd_policy_encode_args* args, void* stream);
/* ssd_policy_head_inc(inc_args) and ssd_policy_encode(enc_args) as ONE launch -- the pipelined rollout's third launch of a timestep:
 * both follow the env step of t and share no data (the inc head reads the input rows of t, the encoder reads the observation of slot
 * t + 1 and must write a DIFFERENT `inputs` buffer / `part`), so one launch-to-launch gap of the timestep disappears.  enc_args: no
 * act, no slot_t_copy / counter_inc (the heads hand the counters over, see ssd_policy_head); same precision as inc_args.  Every
 * window edge ssd_policy_encode takes: 15 x 15 / 31 x 31 under either layout (their own instantiations), every other odd edge
 * 3 .. 63 under SSD_ENCODE_LAYOUT_LUT (one run-time-geometry instantiation per precision, action count and looped / unlooped
 * head).  The Toeplitz layout at another edge, an even edge or one outside 3 .. 63: SSD_ERR_UNSUPPORTED. */
int ssd_policy_head_inc_encode(const ssd_policy_head* inc_args, const ssd_policy_encode_args* enc_args, void* stream);
/* The same launch for the gathered head layouts, asked for by inc_args->pipeline_gather != 0: inc_args carries
 * SSD_INPUT_OTHERS_LAST_ACTION or SSD_INPUT_GATHER_ONEHOT (with others_rows / onehot_rows and prev_record as ssd_policy_head_inc takes
 * them; prev_record_out null), enc_args SSD_ENCODE_LAYOUT_LUT at any odd edge 3 .. 63, 15 and 31 included (the run-time-geometry
 * encoder half at every edge; its features are bit for bit those of ssd_policy_encode).  One instantiation per precision, action
 * count (9 / 8) and layout: the head half is the looped gather head at any grid.  pipeline_gather on a head without either bit, the
 * Toeplitz layout, an even edge or one outside 3 .. 63, another action count: SSD_ERR_UNSUPPORTED.  Everything ssd_policy_head_inc /
 * ssd_policy_encode refuse, act / slot_t_copy / counter_inc, two precisions, enc_args->out == inc_args->inputs, enc_args->slot_t ==
 * inc_args->next_t_out: SSD_ERR_INVALID.  With pipeline_gather zero both bits are refused as before (SSD_ERR_UNSUPPORTED). */
/* conv_b (f32 [6]): read only for the range bound of the conv activations (see SSD_ERRBIT_F16_RANGE). */
/* conv_w f32 [6, 3, 3, 3], conv_b [6], lin_w [32, 6 (V-2)^2] -> the images of SSD_ENCODE_LAYOUT_LUT: table (SSD_ENCODE_LUT_TABLE_BYTES,
 * 16-byte aligned) and lin_frags (SSD_ENCODE_LUT_LIN_BYTES(V, precision)); V odd, 3 .. 63. */
int ssd_policy_pack_encoder_lut(const float* conv_w, const float* conv_b, const float* lin_w, int32_t view_edge, int32_t precision, void* table,
                                void* lin_frags, void* stream);
int ssd_policy_pack_encoder(const float* conv_w, const float* conv_b, const float* lin_w, int32_t view_edge, int32_t precision, void* conv_frags,
                            void* lin_frags, void* stream);

/* Range guard of the two-term f16 split products (precision 2; homophily_agent.py:154-208 computed in f32 by the reference).  The
 * splits use fixed power-of-two scales: head weights x 64, head activations x 16, conv weights / conv activations / Linear weights
 * x 256, the learner's recurrence W_h x 64.  A scaled value beyond f16's 65 504 would turn the product into inf / NaN silently, so
 * the kernels raise the sticky bit SSD_ERRBIT_F16_RANGE in the device's numeric-status word instead: the pack kernels for every
 * weight term and -- from the weights alone -- for the worst-case conv activation; the rollout heads for the activations they scale
 * (the fc1 operand and fc1's output; hidden states are < 1); the recurrence kernel for W_h.  ssd_numeric_status returns and
 * clears the word (it synchronises the device); ssd_poll_error ORs it into an env's bits. */
#define SSD_ERRBIT_F16_RANGE 32
int ssd_numeric_status(int32_t* bits);

/* ---- COUNTER-mode generator (shared definition) ---------------------------------------------
 * Two levels, so that the expensive part is computed once per EPISODE (by the reset call) and kept in the env state:
 *   episode = number of resets of this env including the one that opened the current episode (1, 2, ...)
 *   b[0..3] = philox4x32_10(counter = {0, 0, env_global_id, episode}, key = {seed_lo, seed_hi})
 *   c       = call index inside the episode: 0 for the reset call, (steps completed so far) + 1 for a step call
 *   x(stream, k) = mix32(b[stream] ^ (c << 16) ^ k),  stream = SSD_STREAM_*  (one Philox word per stream; k, c < 65536)
 *   mix32(x): x ^= x >> 17; x *= 0xed5ad4bb; x ^= x >> 11; x *= 0xac4c1b51; x ^= x >> 15; x *= 0x31848bab; x ^= x >> 14
 *             (the "triple32" integer hash, a bijection on 32 bits)
 *   uniform number k of the call: u = (x(UNIFORM, k) >> 8) * 2^-24 as double, compared `u < p` in fp64
 *   shuffles: stable sort of the items by (x(stream, item index) >> 8, item index)   (24-bit key: key | index fits 32 bits)
 *   spawn rotation of agent a: x(SPAWN_ROT, a) >> 30
 *   spawn list shuffle of agent a (random_spawn_point): sort of the list elements e = copy * n_spawn_points + point id
 *             (copy = 0, and 1 for Cleanup's duplicated list) by (x(SPAWN_ROT, 256 + 32 a + e) >> 8, e); at most SSD_MAX_SPAWN = 16 points
 * ssd_state.epoch carries `episode`; importing it re-derives b.                                                        */
enum { SSD_STREAM_UNIFORM = 0, SSD_STREAM_MOVE = 1, SSD_STREAM_WASTE = 2, SSD_STREAM_SPAWN_ROT = 3 };

#ifdef __cplusplus
}
#endif
#endif /* SSD_HIP_H */
