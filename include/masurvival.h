/*
 * masurvival.h -- C-ABI of the MI355X-native batched MaSurvival env step.
 *
 * This is the drop-in boundary for the reference's hot path
 *   MaSurvival.step  (reference: masurvival/envs/masurvival_env.py:76-90)
 *   -> Simulation.step (reference: masurvival/simulation.py:233-242)
 * batched over N independent envs that live in HBM as struct-of-arrays.
 *
 * Plain C types only: every I/O pointer is a DEVICE pointer owned by the
 * caller unless stated otherwise; `stream` is a hipStream_t passed as void*.
 * Calls are stream-ordered and asynchronous (no implicit device sync) and are
 * not re-entrant per handle.  Errors: 0 = ok, negative = error code, with a
 * thread-local message from mas_last_error().  Nothing aborts or throws
 * across this ABI.
 */
#ifndef MASURVIVAL_H
#define MASURVIVAL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MAS_ABI_VERSION 3  /* 2: mas_gae takes the caller's partial-sum scratch; 3: mas_adv_normalize */

#define MAS_OK 0
#define MAS_ERR_INVALID_ARG (-1)
#define MAS_ERR_UNSUPPORTED (-2)
#define MAS_ERR_HIP (-3)
#define MAS_ERR_OOM (-4)

#define MAS_MAX_ZONE_PHASES 8

/* Resolved env configuration: the POD lowering of onevsone_heals_config
 * (reference masurvival_env.py:140-238) after MaSurvival.__init__'s rewrites
 * (masurvival_env.py:293-389).  The Python front-end (masurvival.config)
 * builds it with the reference's one-level merge semantics. */
typedef struct mas_config {
    int32_t n_agents;          /* agents.n_agents                 (:166-169) */
    int32_t n_heals;           /* heals.reset_spawns.n_items      (:210-214) */
    int32_t n_boxes;           /* boxes.reset_spawns.n_boxes      (:191-195) */
    int32_t teams;             /* teams.twoteams -> TwoTeams       (:340-342) */
    int32_t ownership;         /* boxes.ownership -> OwnedObject*  (:196,345) */
    int32_t melee_cooldown;    /* >0: Melee(cooldown); 0: ContinuousMelee (:309-312) */
    int32_t omniscient;        /* observation.omniscent            (:141-143) */
    int32_t gameover_mode;     /* 0 = 'alldead', 1 = 'lastalive'   (:154-156) */
    float r_alive, r_dead, r_kill, r_death; /* reward_scheme      (:144-153) */
    int32_t grid_size;         /* spawn_grid.grid_size             (:158-161) */
    double floor_size;         /* spawn_grid.floor_size (= room size) */
    double agent_size;         /* agents.agent_size (diameter)     (:168) */
    float impulse[3];          /* motors.impulse                   (:177-180) */
    int32_t agent_health;      /* health.health                    (:181-183) */
    float melee_range;         /* melee.range                      (:184-190) */
    int32_t melee_damage;      /* melee.damage */
    double box_size;           /* boxes.reset_spawns.box_size */
    int32_t box_health;        /* boxes.health                     (:208) */
    int32_t randomized_boxes;  /* 'randomized_shape' in boxes      (:362-366) */
    double avg_w, std_w, avg_h, std_h, min_w, min_h; /* RandomizeBoxShapes (semantics.py:97-120) */
    double box_item_size;      /* boxes.item.item_size             (:204-207) */
    float box_item_offset;     /* boxes.item.offset */
    double heal_size;          /* heals.reset_spawns.item_size */
    int32_t healing;           /* heals.heal.healing               (:215-217) */
    int32_t slots;             /* inventory.slots                  (:219-221) */
    float pickup_radius;       /* auto_pickup.shape = circle(0.5)  (:222-224) */
    float give_radius;         /* give.shape = circle(2)           (:225-227) */
    float deathdrop_radius;    /* death_drop.radius                (:228-230) */
    int32_t zone_phases;       /* safe_zone.phases                 (:231-237) */
    int32_t zone_cooldown;
    int32_t zone_damage;
    int32_t zone_n_radii;      /* len(safe_zone.radiuses) (a 0 radius is appended) */
    double zone_radii[MAS_MAX_ZONE_PHASES];
    int32_t zone_random_centers; /* centers == 'random' */
    float zone_centers[MAS_MAX_ZONE_PHASES][2]; /* used when !zone_random_centers */
    float cam_depth;           /* cameras.depth                    (:173-176) */
    double cam_fov;            /* cameras.fov (radians, double as in Python) */
    double wall_aspect_ratio;  /* ThickRoomWalls default 100 (semantics.py:685) */
    /* Lidars(n_lasers, fov, depth) (simulation.py:357-392) as the last agents
     * module, observed as the 'lidars' key (the reference leaves
     * the module unwired, masurvival_env.py:392,857-858).  0 = off. */
    int32_t lidar_n_lasers;    /* lidars.n_lasers (0, or 2..MAS_MAX_LASERS) */
    float lidar_depth;         /* lidars.depth */
    double lidar_fov;          /* lidars.fov (radians, double as in Python) */
} mas_config;

#define MAS_MAX_LASERS 32

/* Observation layout: one flat float32 row of `obs_dim` per agent; the keys
 * are laid out in observation_space (gym Dict, sorted-key) order, each key's
 * per-agent sub-array flattened C-order (compute_obs_space :391-447). */
#define MAS_MAX_KEYS 16
typedef struct mas_obs_layout {
    int32_t n_agents;
    int32_t obs_dim;
    int32_t n_keys;
    char key_name[MAS_MAX_KEYS][24];
    int32_t key_offset[MAS_MAX_KEYS];   /* float offset inside the row */
    int32_t key_ndim[MAS_MAX_KEYS];     /* ndim of the per-agent sub-array */
    int32_t key_shape[MAS_MAX_KEYS][2]; /* per-agent sub-array shape */
} mas_obs_layout;

typedef struct mas_handle mas_handle;

/* replaces MaSurvival.__init__ (masurvival_env.py:293-389): validates the
 * config, allocates the SoA state of n_envs envs on `device` (HBM-resident,
 * no allocation afterwards). */
int mas_create(const mas_config* cfg, int64_t n_envs, int32_t device, mas_handle** out);
int mas_destroy(mas_handle* h);

/* replaces compute_obs_space (masurvival_env.py:391-447). */
int mas_get_obs_layout(const mas_handle* h, mas_obs_layout* out);
int64_t mas_num_envs(const mas_handle* h);

/* replaces the np_random assignment (masurvival_env.py:50,67,455-465):
 * per-env numpy PCG64 bit-generator state, HOST array [n_envs][6] of
 * {state_hi, state_lo, inc_hi, inc_lo, has_uint32, uinteger}
 * (numpy.random.PCG64().state).  One stream per env, shared by the spawn
 * shuffle, box shapes, zone centres and death drops as in the reference. */
int mas_seed(mas_handle* h, const uint64_t* host_rng_states, void* stream);

/* replaces BaseEnv.reset (masurvival_env.py:59-74) for every env whose
 * env_mask byte is non-zero (env_mask == NULL: all envs).  Writes the reset
 * observation rows of those envs into obs [n_envs][n_agents][obs_dim]. */
int mas_reset(mas_handle* h, const uint8_t* env_mask, float* obs, void* stream);

/* replaces BaseEnv.step (masurvival_env.py:76-90): actions int8
 * [n_envs][n_agents][6] (MultiDiscrete [3,3,3,2,2,2], dead agents ignored),
 * writes obs [n_envs][n_agents][obs_dim], rewards [n_envs][n_agents],
 * done [n_envs].  auto_reset != 0: an env that is done is reset in the same
 * launch and its obs rows hold the first observation of the new episode
 * (rewards/done still describe the finished step). */
int mas_step(mas_handle* h, const int8_t* actions, float* obs, float* rewards,
             uint8_t* done, int32_t auto_reset, void* stream);

/* mas_step with the observation rows written as the PPO consumer's bf16
 * policy input instead of fp32 obs: x_bf16 [n_envs * n_agents][x_stride]
 * (x_stride a multiple of 4 >= obs_dim, 8-B aligned), columns [0, obs_dim)
 * of each row = the fp32 row of mas_step rounded to bf16 (round to nearest
 * even, the conversion mas_policy_act applies to fp32 rows), the other
 * columns untouched (the caller's bias column and padding stay).  Rewards,
 * done and the env state are those of mas_step, bit for bit.  Not for the
 * lidars key or a config whose auto-reset runs in the separate reset launch
 * (MAS_ERR_UNSUPPORTED: use mas_step).  No reference equivalent (the rollout
 * side). */
int mas_step_x(mas_handle* h, const int8_t* actions, void* x_bf16, int64_t x_stride, float* rewards,
               uint8_t* done, int32_t auto_reset, void* stream);
/* 1 when mas_step_x can run this handle with this auto_reset, else 0. */
int mas_step_x_supported(const mas_handle* h, int32_t auto_reset);

/* Per-env episode statistics (flush_stats, masurvival_env.py:471-508):
 * device float [n_envs][MAS_STATS_WIDTH] laid out as
 * [0,8) reward0..reward{R-1}, [8,16) kills0..kills{R-1}, 16 steps,
 * 17 heals_used, 18 boxes_placed, with R = 2 (teams) or n_agents (unused
 * slots 0).  Accumulated since the last flush. */
#define MAS_STATS_WIDTH 19
int mas_flush_stats(mas_handle* h, float* stats, void* stream);

/* mas_alive (an addition within ABI version 3): which agents are alive, as
 * DEVICE float alive[n_envs][n_agents] of 1.0f / 0.0f -- the env's alive
 * mask, so the agents whose actions the next mas_step reads ("dead agents
 * ignored" above).  It describes the state the last written observation rows
 * describe: after an auto-reset step a reset env's agents are all alive.  An
 * agent the zone killed in the last step, whose observation already shows
 * health <= 0 but which acts once more before it is removed, counts as alive.
 * fp32 because it is a loss weight (mas_policy_train_w) and mas_rows_select
 * gathers fp32 arrays.  Stream-ordered, allocates nothing, does not
 * synchronise, capturable.  MAS_ERR_INVALID_ARG for a null handle or output,
 * before any device work. */
int mas_alive(mas_handle* h, float* alive, void* stream);

/* Raw SoA state image (checkpoint / parity state injection).  Byte size of
 * the image and copies to/from a caller DEVICE buffer of that size. */
int64_t mas_state_bytes(const mas_handle* h);
int mas_get_state(mas_handle* h, void* dst, void* stream);
int mas_set_state(mas_handle* h, const void* src, void* stream);

/* Rollout side (SURVEY.md 8(a) a24 -- new, the reference has no trainer):
 * GAE(gamma, lambda) over an on-device rollout buffer of T steps and
 * n_columns = n_envs * n_agents agent columns, all DEVICE pointers:
 *   rewards [T][n_columns], values [T+1][n_columns] (row T = bootstrap value
 *   of the observation after the last step), done [T][n_envs] (mas_step's
 *   done; any nonzero byte is done, and column m reads the flag of env
 *   m / n_agents),
 *   advantages/returns [T][n_columns] (out), adv_sums double[2] (out:
 *   sum and sum of squares of the advantages, for normalisation).
 *   delta_t = r_t + gamma * V_{t+1} * (1 - d_t) - V_t
 *   A_t     = delta_t + gamma * lambda * (1 - d_t) * A_{t+1},  A_T = 0
 *   returns_t = A_t + V_t
 * with d_t = 1 where the byte is nonzero.  At a done step an auto-reset
 * env's next value and the later advantages are multiplied by zero: a finite
 * V_{t+1} or A_{t+1} drops out, a non-finite one (inf, NaN) still gives NaN
 * and propagates to every earlier step of the column.
 * scratch: DEVICE double[mas_gae_scratch_doubles(n_columns)], the call's
 * per-workgroup partial sums (no initialisation needed; the library keeps
 * no state between calls, so calls on different streams -- or handles,
 * trainers, threads -- may run concurrently as long as each has its own
 * scratch and outputs).  adv_sums is summed in a fixed order: the same
 * inputs give the same bits.
 * MAS_GAE_SCAN=1 (environment, read per call) selects the wavefront scan
 * over time instead of the per-column walk; same results within fp32
 * rounding.                                                            */
int64_t mas_gae_scratch_doubles(int64_t n_columns);
int mas_gae(int32_t T, int64_t n_columns, int32_t n_agents, const float* rewards, const float* values,
            const uint8_t* done, float gamma, float lam, float* advantages, float* returns, double* adv_sums,
            double* scratch, void* stream);
/* Running return normalisation of the rewards (additions within ABI version
 * 3; VecNormalize's reward half, batched per rollout).  All pointers are
 * DEVICE pointers; both calls are stream-ordered, allocate nothing, do not
 * synchronise and can be captured; an argument error is MAS_ERR_INVALID_ARG
 * before any device work.
 *
 * mas_ret_stats: every column m keeps a running discounted return
 * ret_carry[m] (fp32, in/out: it persists across rollouts, 0 at the start).
 * Step t = 0..T-1 of the rollout does, in this order,
 *   R = fl32(fl32(gamma * R) + rewards[t][m])      two roundings, no fma
 *   sums[0] += R,  sums[1] += R^2                  in double: both terms exact
 *   if done[t][m / n_agents] != 0: R = 0           after the step has counted
 * and sums [2] receives the two totals over all T * n_columns steps (written,
 * not added to).  Every column counts.  scratch:
 * double[mas_ret_stats_scratch_doubles(n_columns)] (-1 for n_columns < 1; never
 * more than mas_gae_scratch_doubles(n_columns), so a GAE scratch serves calls
 * ordered on one stream), the call's per-workgroup partial sums, summed in a
 * fixed order: the same inputs give the same bits, whatever scratch held.
 * Refused: T < 1, n_columns no positive multiple of n_agents, a null pointer,
 * n_columns too large for the grid, gamma not finite.
 *
 * The batch record (T * n_columns, sums[0], sums[1]) merges into a running
 * (count, mean, m2) through mas_obs_norm_merge(1, ...), whose inv_std output
 * is the reward scale (float)(1 / sqrt(m2 / count + eps)); the mean is not
 * subtracted from a reward.
 *
 * mas_gae_scaled: mas_gae (either form, MAS_GAE_SCAN read per call) on
 *   r' = clamp(fl32(r * reward_scale[0]), -reward_clip, reward_clip)
 * in place of r: the product is rounded on its own, x < -c ? -c : (x > c ? c : x)
 * lets a NaN through as torch.clamp does, and the scale is read on the device
 * from reward_scale (float[1]), so no host copy orders the call after the
 * merge that wrote it.  rewards itself is not written.  With a scale of 1 and
 * a clip of +inf the results are mas_gae's bit for bit.  Refused besides
 * mas_gae's refusals: a null reward_scale, reward_clip NaN or <= 0 (+inf is
 * allowed). */
int64_t mas_ret_stats_scratch_doubles(int64_t n_columns);
int mas_ret_stats(int32_t T, int64_t n_columns, int32_t n_agents, const float* rewards,
                  const uint8_t* done, float gamma, float* ret_carry /* [n_columns], in/out */,
                  double* sums /* [2] */, double* scratch, void* stream);
int mas_gae_scaled(int32_t T, int64_t n_columns, int32_t n_agents, const float* rewards,
                   const float* values, const uint8_t* done, float gamma, float lam,
                   const float* reward_scale /* DEVICE float[1] */, float reward_clip,
                   float* advantages, float* returns, double* adv_sums, double* scratch, void* stream);
/* Episode statistics of a rollout (additions within ABI version 3): the
 * episodes the rollout finished, their lengths, every agent slot's
 * undiscounted return and which side won.  All pointers are DEVICE pointers;
 * the call is stream-ordered, allocates nothing, does not synchronise and can
 * be captured.  rewards and done are only read.
 *
 * Per env e, steps t = 0..T-1 in order, agents a ascending, from the carries
 * G[a] = ret_carry[e * n_agents + a] (fp64) and len = len_carry[e] (both
 * in/out: they persist across rollouts, 0 at the start):
 *   G[a] += (double)rewards[t][e][a]      one fp64 add per step
 *   len  += 1
 *   if done[t][e] != 0:                    (any nonzero byte)
 *       episodes += 1;  sum_len += len;  sum_len2 += len * len
 *       sum_G[a] += G[a];  sum_G2[a] += G[a] * G[a]     each product rounded once
 *       s0 = the sum of G[a] over the agents in side_mask, a ascending, from
 *            +0.0;  s1 = the same over the other agents
 *       wins0 += s0 > s1;  wins1 += s1 > s0;  draws += s0 == s1
 *       G[:] = 0;  len = 0
 * The step that ends an episode counts towards it: the rewards of step t
 * belong to the episode that done[t] closes.  A NaN side sum is none of win,
 * loss or draw.  len * len is formed in fp64.
 *
 *   record = [episodes, sum_len, sum_len2, wins0, wins1, draws,
 *             sum_G[0..n_agents), sum_G2[0..n_agents)]
 * double[6 + 2 * n_agents], the totals over all envs of this call (written,
 * not added to).  With side_mask 0 or all agents there are no two sides and
 * entries 3..5 are 0.  The integer entries (0..5) are exact while below 2^53.
 * The envs' terms are added in a fixed order that is not the envs' order.
 *
 * scratch: double[mas_episode_stats_scratch_doubles(n_envs, n_agents)] (-1 for
 * n_envs < 1, n_agents outside 1..8, the agent counts the call takes, or a
 * grid that does not fit), the call's per-workgroup partial sums: the same
 * inputs give the same bits, whatever scratch held.
 *
 * MAS_ERR_INVALID_ARG before any HIP call, the shape first and then the
 * pointers: T <= 0, n_envs <= 0, n_agents < 1, a side_mask bit at or above
 * n_agents, a null pointer, n_envs too large for the grid.  After those,
 * n_agents > 8 (the capacity classes' limit: an env's returns live in
 * registers) is MAS_ERR_UNSUPPORTED with nothing launched. */
int64_t mas_episode_stats_scratch_doubles(int64_t n_envs, int32_t n_agents);
int mas_episode_stats(int32_t T, int64_t n_envs, int32_t n_agents, uint32_t side_mask,
                      const float* rewards,  /* [T][n_envs * n_agents] */
                      const uint8_t* done,   /* [T][n_envs], any nonzero byte is done */
                      double* ret_carry,     /* [n_envs * n_agents] in/out */
                      int32_t* len_carry,    /* [n_envs] in/out */
                      double* record,        /* [6 + 2 * n_agents], written, not added to */
                      double* scratch, void* stream);
/* mas_adv_normalize: the n advantages (DEVICE float, 16-B aligned)
 * normalised in place from stats = DEVICE double[3] (sum, sum of squares,
 * count: mas_gae's adv_sums and the count, summed over ranks):
 *   mean = sum / count, var = max(sum_sq / count - mean^2, 0)   (double)
 *   adv  = (adv - (float)mean) / ((float)sqrt(var) + 1e-8f)     (float)
 * one launch, the roundings of the torch expression it replaces
 * (adv.sub_(mean.float()).div_(var.sqrt().float() + 1e-8)). */
int mas_adv_normalize(int64_t n, float* adv, const double* stats, void* stream);

/* Rollout side: sample the six action heads (MultiDiscrete [3,3,3,2,2,2]) of
 * n_rows agent rows from logits [n_rows][row_stride] (first 15 floats of a
 * row: the heads' logits in order), Gumbel-max with a counter-based RNG keyed
 * by (seed, step, row); writes actions int8 [n_rows][6] and the log-prob of
 * the drawn actions float [n_rows].  Batched form of the reference's policy
 * act() (demo.py:14-22).  DEVICE pointers.
 *
 * The stream, so that a host can reproduce a rollout's draws (uint64
 * arithmetic that wraps; tests/sampler_ref.py restates it in numpy):
 *   mix64(z): z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 *             z = (z ^ z >> 27) * 0x94D049BB133111EB; return z ^ z >> 31
 *             (SplitMix64's output function)
 *   base = mix64(seed ^ mix64(step * 0x100000001B3 + row))
 *   r    = mix64(base + 4 * head + option)     head 0..5, option 0..n_head-1
 *   u    = ((float)(r >> 40) + 0.5f) * 2^-24   in fp32
 * row is the row's index in the whole batch (first_row + the row of the call
 * for the mas_policy_act_* forms).  r >> 40 < 2^24 converts exactly; the sum
 * with 0.5f is exact below 2^23 and rounds to even above, so u lies in
 * (0, 1]: r >> 40 = 0 gives 2^-25 and r >> 40 = 2^24 - 1 gives 1.0.  An
 * option's score is logit - log(-log(u)) in fp32, and the head's action the
 * first option with the greatest score (a strict > scan from option 0).
 * u = 1.0 scores +inf: that option is drawn whatever the logits, once in 2^24
 * draws, with a finite log-prob. */
int mas_sample_actions(int64_t n_rows, const float* logits, int64_t row_stride, uint64_t seed, uint64_t step,
                       int8_t* actions, float* logp, void* stream);

/* Rollout / update side (SURVEY.md 8(a) a24 -- new): the shared-parameter
 * policy MLP obs_dim -> 256 -> 256 (tanh) -> 16 (the six heads' 15 logits,
 * then the value) as fused bf16-MFMA kernels with fp32 accumulation.  The
 * reference has no policy; its demo's act() (demo.py:14-22) is the random
 * policy this replaces.  All pointers are DEVICE pointers.
 *
 * mas_policy_pack fills a packed image of mas_policy_packed_bytes(obs_dim)
 * bytes from the fp32 parameters W1 [256][obs_dim], b1 [256], W2 [256][256],
 * b2 [256], W3 [16][256], b3 [16] (row-major, torch nn.Linear layout).
 *
 * mas_policy_act: forward of n_rows agent rows of obs [n_rows][obs_dim] fp32
 * plus Gumbel-max sampling of the six heads with the RNG of
 * mas_sample_actions; writes actions int8 [n_rows][6], logp and value
 * [n_rows], and, when x_bf16 != NULL, the bf16 copy of the rows
 * [n_rows][x_stride] (x_stride a multiple of 8 >= 16*ceil(obs_dim/16)) that
 * mas_policy_train reads: columns [0, 16*ceil(obs_dim/16)) are written, the
 * row's obs_dim values, then 1.0 in column obs_dim (a bias column for the
 * caller's dW1 GEMM) when it falls in that range, then zeros.
 * mas_policy_act_rows: the same for the rows [first_row, first_row + n_rows)
 * of a larger batch (obs, x_bf16, actions, logp, value point at that slice):
 * the sampling RNG is keyed by the row's index in the whole batch, so shards
 * launched on separate streams draw exactly what one launch over the batch
 * draws (mas_policy_act = first_row 0).
 *
 * mas_policy_train: forward of x_bf16 rows, the per-row gradient of the PPO
 * loss  mean(-min(r A, clip(r, 1-clip, 1+clip) A)) + vf_coef mean((v-ret)^2)
 * - ent_coef mean(entropy)  (r = exp(logp(actions) - old_logp); `scale` =
 * 1/rows of the minibatch), and the backward data path; writes feature-major
 * bf16 h1, h2, dA1, dA2 [256][n_rows] (dA = gradient at the pre-activation)
 * and dz [16][n_rows], from which the caller forms the weight gradients
 * (dW1 = dA1 x, dW2 = dA2 h1^T, dW3 = dz h2^T, db = row sums; a row of ones
 * appended to h1 / h2 and the bias column of x give the db's from the same
 * GEMMs), and
 * partials [mas_policy_blocks(n_rows)][4] = per-block sums of the clipped
 * surrogate loss, (v-ret)^2, entropy and the clipped-row count. */
/* mas_render_view: one env's bodies for rendering (debugging / GIF frames;
 * replaces what rendering.py:118-613 reads from the Box2D world).
 * Synchronous: waits for the device, then copies MAS_RENDER_VIEW_FLOATS
 * floats to host `out`:
 *   [0] n_agents  [1] n_boxes  [2] n_box_items  [3] n_heals
 *   [4..6] safe zone centre x, y, radius   [7..9] agent / box / heal slots
 *   (AM, BM, HM of the capacity class)   [10] floor size
 *   [12 + 5k] wall k = 0..3: centre x, y, angle, half extents x, y
 *   [32 ...] AM agents (x, y, angle, alive, health), BM boxes (x, y, hx, hy,
 *   health), BM box items (x, y, hx, hy), HM heals (x, y); entries past the
 *   counts are unused. */
#define MAS_RENDER_VIEW_FLOATS 320
int mas_render_view(mas_handle* h, int64_t env, float* out);

int64_t mas_policy_packed_bytes(int32_t obs_dim);
int64_t mas_policy_blocks(int64_t n_rows);
int mas_policy_pack(int32_t obs_dim, const float* w1, const float* b1, const float* w2, const float* b2,
                    const float* w3, const float* b3, void* packed, void* stream);
int mas_policy_act(const void* packed, int32_t obs_dim, int64_t n_rows, const float* obs, void* x_bf16,
                   int64_t x_stride, uint64_t seed, uint64_t step, int8_t* actions, float* logp, float* value,
                   void* stream);
int mas_policy_act_rows(const void* packed, int32_t obs_dim, int64_t n_rows, int64_t first_row, const float* obs,
                        void* x_bf16, int64_t x_stride, uint64_t seed, uint64_t step, int8_t* actions, float* logp,
                        float* value, void* stream);
/* mas_policy_act_x: mas_policy_act_rows over bf16 input rows x_bf16
 * [n_rows][x_stride] (mas_step_x's rows: columns past obs_dim are ignored --
 * W1 is zero there), which are not written; the same actions, log-probs and
 * values as mas_policy_act_rows on the fp32 rows they were rounded from. */
int mas_policy_act_x(const void* packed, int32_t obs_dim, int64_t n_rows, int64_t first_row, const void* x_bf16,
                     int64_t x_stride, uint64_t seed, uint64_t step, int8_t* actions, float* logp, float* value,
                     void* stream);
/* mas_policy_act_sel (an addition within ABI version 3): mas_policy_act_x
 * over the selected agents of whole envs, sampled or greedy -- what lets two
 * packed policies act in one env.  The slice is n_envs envs of n_agents rows
 * each (row = env * n_agents + agent; the pointers address the slice's first
 * row, first_row is its index in the whole batch, as for
 * mas_policy_act_rows).  Bit a of agent_mask selects agent a of every env:
 * the kernel runs over the n_envs * popcount(agent_mask) selected rows and
 * neither reads nor writes the rows of the other agents, so calls with
 * disjoint masks fill disjoint rows of the same output buffers.  The sampling
 * RNG is keyed by first_row + the row's index in the slice: a selected row
 * gets exactly the actions, log-prob and value mas_policy_act_x gives it.
 * greedy != 0: each head takes the arg-max of its logits (after the bias,
 * fp32; the lowest index wins a tie) and seed / step are unused; logp is the
 * log-prob of that choice, bit-identical to a sampled call's that drew it.
 * logits_out (may be NULL; fp32 [rows][16], 16-B aligned): the selected rows'
 * 15 logits and then the value, the values the choice was made from.
 * MAS_ERR_INVALID_ARG, before any device work: n_agents outside 1..32, a zero
 * agent_mask, a mask bit at or above n_agents, n_envs < 0, a null packed,
 * x_bf16, actions, logp or value, or an x_stride / alignment mas_policy_act_x
 * refuses.  n_envs == 0 is MAS_OK and launches nothing. */
int mas_policy_act_sel(const void* packed, int32_t obs_dim, int64_t n_envs, int32_t n_agents,
                       uint32_t agent_mask, int64_t first_row, const void* x_bf16, int64_t x_stride,
                       uint64_t seed, uint64_t step, int32_t greedy,
                       int8_t* actions, float* logp, float* value, float* logits_out, void* stream);
/* mas_rows_select (an addition within ABI version 3): gather the rows of the
 * selected agents of n_envs whole envs (row = env * n_agents + agent; bit a of
 * agent_mask selects agent a, as for mas_policy_act_sel) into dense arrays of
 * n_envs * popcount(agent_mask) rows, in (env, ascending agent) order: output
 * row j is input row (j / m) * n_agents + (the (j % m)-th set bit of the
 * mask), m = popcount(agent_mask).  What lets a trainer that owns only some
 * agents run GAE and the mas_policy_train / mas_policy_dw kernels on its rows alone
 * (time steps fold into n_envs: a [T][N][A] rollout is T * N envs).
 * Every array pair is optional (NULL in and out together skips it); a pair
 * with one NULL is an error.  x: columns [0, x_cols) of each selected row are
 * copied bit for bit as 16-B chunks, the other columns of x_out are not
 * written.  actions: 6 bytes per row.  f32_in / f32_out: HOST arrays of
 * n_f32 <= 4 DEVICE pointers, [rows] fp32 each, read on the host and passed to
 * the kernel by value.  Rows of unselected agents are never read and nothing
 * past output row n_envs * m is written.  One launch serves all the arrays;
 * the call is stream-ordered, allocates nothing and does not synchronise.
 * MAS_ERR_INVALID_ARG, before any device work: n_agents outside 1..32, a zero
 * agent_mask, a mask bit at or above n_agents, n_envs < 0 (or so large that a
 * byte offset passes 2^63), n_f32 outside 0..4, a half-NULL pair, x_cols not
 * a positive multiple of 8 or larger than either stride, a stride that is not
 * a multiple of 8, x pointers not 16-B aligned (actions 2-B, fp32 4-B), an
 * output pointer equal to its input.  n_envs == 0, or every pair NULL, is
 * MAS_OK and launches nothing. */
int mas_rows_select(int64_t n_envs, int32_t n_agents, uint32_t agent_mask,
                    const void* x_bf16, int64_t x_stride,      /* [rows][x_stride] bf16 */
                    void* x_out, int64_t x_out_stride, int32_t x_cols,
                    const int8_t* actions, int8_t* actions_out, /* [rows][6] */
                    int32_t n_f32, const float* const* f32_in, float* const* f32_out,
                    void* stream);
/* mas_bot_act (an addition within ABI version 3): scripted baseline opponents
 * on the device.  Fills the action rows of the bit-selected agents of n_envs
 * whole envs from their bf16 observation rows, by a fixed rule: the slot of
 * mas_policy_act_sel with no network.  Rows and mask are addressed as there
 * (row = env * n_agents + agent with n_agents = cfg->n_agents; bit a of
 * agent_mask selects agent a of every env); only the selected rows are read,
 * columns at or past the config's obs_dim never, and only their 6 action bytes
 * are written.  x_bf16 [rows][x_stride]: 16-B aligned, x_stride a multiple of
 * 8 >= 16*ceil(obs_dim/16) (mas_policy_act_sel's rules); actions 2-B aligned.
 * The column offsets (mas_get_obs_layout's) and the thresholds come from cfg on
 * the host at every call: no handle, so the call serves any row buffer of that
 * config.  Stream-ordered, allocates nothing, never synchronises, capturable;
 * no random numbers: the same row bits give the same action bytes.
 *
 * The rule.  A bf16 value is exact in fp32, so the inputs are exact.  All
 * arithmetic is fp32, every operation rounded on its own (no fma), IEEE divide
 * and sqrt; x^2 means x * x; the decimal constants below are their nearest
 * fp32.  From the row (an agent record is [id, (team when cfg->teams), health,
 * x, y, angle, vx, vy, w]):
 *   self: health, pos = (x, y), theta = angle, w (angular velocity), team
 *   zone: zone_c = zone[0..1], zone_r = zone[2]
 *   others[j], others_mask[j]  j < n_agents - 1;  heals[k] = (x, y),
 *   heals_mask[k]  k < n_heals;  heal_slot_mask          (when n_heals > 0)
 * Actions a[0..5] (MultiDiscrete [3,3,3,2,2,2]; 1 is "nothing" in a[0..2]):
 *   kind IDLE, or health <= 0:  a = [1,1,1,0,0,0], and nothing below applies.
 *   a[1] = 1, a[5] = 0.
 *   a[4] = 1 exactly when n_heals > 0 and heal_slot_mask == 0 and
 *          health <= agent_health - healing (an integer, exact in fp32).
 * Target, the first that applies:
 *   1. e = pos - zone_c, m = max(zone_r - 1, 0):  |e|^2 > m^2  (|e|^2 =
 *      e.x^2 + e.y^2): the zone centre.
 *   2. FORAGER with n_heals > 0: the heal k with heals_mask[k] == 0 and not
 *      |heals[k] - zone_c|^2 > m^2 (a heal outside the zone's margin is left
 *      alone) of the least |heals[k] - pos|^2, if there is one.
 *   3. the other agent j with others_mask[j] == 0, health_j > 0 and, when
 *      cfg->teams, team_j != team, of the least |pos_j - pos|^2, if there is
 *      one; FORAGER takes it unless that least value is > 4^2 (only within 4 m).
 *   Among equal squared distances the lowest index (k or j) wins.
 *   4. no target: a = [1, 1, 2, 0, a[4], 0] (turn counter-clockwise in place).
 * Steering towards target t:  d = t - pos, l = sqrt(d.x^2 + d.y^2),
 *   h = ((float)cos, (float)sin) of (double)theta from the library's shared
 *   double sincos (Cody-Waite reduction, fdlibm kernels), c = h.x d.x + h.y d.y,
 *   s = h.x d.y - h.y d.x,  u = s - (0.25 w) l   (the turn leads its own
 *   angular velocity by 0.25 s: the bang-bang turn alone overshoots),
 *   b = 0.15 l:
 *   a[2] = 2 if u > b; else 0 if -b > u; else 2 if 0 > c; else 1.
 *   a[0] = 2 if c > 0.8 l and l > stop, stop = 1.25 for an enemy (3.) and
 *          0.25 for the zone centre or a heal (it has arrived); else 1.
 *   a[3] = 1 if the target is an enemy, not l > reach and c > 0.9 l, where
 *          reach = (float)(melee_range + agent_size / 2) formed in double;
 *          else 0.
 *
 * MAS_ERR_INVALID_ARG, before any device work: a null cfg or a config
 * mas_create refuses (one that no compiled capacity class fits included), an
 * unknown kind, a zero agent_mask or a mask bit at or
 * above n_agents (or n_agents > 32), n_envs < 0 or so many selected rows that
 * the block count passes 2^31, a null x_bf16 or actions, a bad stride or
 * alignment.  n_envs == 0 is MAS_OK and launches nothing. */
#define MAS_BOT_IDLE 0
#define MAS_BOT_HUNTER 1
#define MAS_BOT_FORAGER 2
int mas_bot_act(const mas_config* cfg, int32_t kind, int64_t n_envs, uint32_t agent_mask,
                const void* x_bf16, int64_t x_stride, int8_t* actions, void* stream);
/* Running observation normalisation (additions within ABI version 3).  The
 * normaliser (per-column mean and 1 / std) is never applied to a row: it is
 * folded into the packed layer-1 weights, W1 ((x - mean) * s) + b1 =
 * (W1 diag(s)) x + (b1 - W1 (mean * s)), so every consumer of a packed image
 * (mas_policy_act*, mas_policy_train*) acts on raw rows unchanged.  All
 * pointers are DEVICE pointers; every call is stream-ordered, allocates
 * nothing, does not synchronise and can be captured; an argument error is
 * MAS_ERR_INVALID_ARG before any device work.
 *
 * mas_obs_stats: sums[0][c] = sum over the rows of x[r][c], sums[1][c] = sum
 * of x[r][c]^2, c < n_cols; sums is [2][n_cols] doubles, x_bf16 is
 * [n_rows][x_stride] bf16 (16-B aligned, x_stride a multiple of 8, n_cols in
 * 1..x_stride and any remainder mod 8).  Columns at or past n_cols never
 * reach the output, whatever they hold.  Accumulated in fp64 (every term is
 * exact) in a fixed order over a grid that depends on (n_rows, n_cols)
 * alone: the same inputs give the same bits, whatever scratch held.  scratch:
 * double[mas_obs_stats_scratch_doubles(n_rows, n_cols)] (-1 for n_rows < 0 or
 * n_cols < 1), the call's partial records; concurrent calls need their own.
 * n_rows == 0 zero-fills sums.  Refused: n_rows < 0, n_cols outside
 * 1..x_stride, x_stride no positive multiple of 8, x_bf16 not 16-B aligned
 * (or null with rows to read), sums or scratch null or not 8-B aligned.
 *
 * mas_obs_norm_merge: one batch into the running state, Chan's parallel
 * update in fp64.  state [1 + 2 n_cols] = count, mean[], m2[]; batch
 * [1 + 2 n_cols] = count_b, sum[], sum of squares[] (mas_obs_stats writes at
 * batch + 1, the caller fills count_b; several ranks all-reduce the whole
 * array first).  With n_b = count_b, n = count + n_b:
 *   mean_b = sum / n_b,  m2_b = max(sumsq - n_b mean_b^2, 0),  d = mean_b - mean,
 *   mean += d n_b / n,  m2 += m2_b + d^2 count n_b / n,  count = n;
 * n_b == 0 leaves the state as it is.  Always written: mean_out[c] =
 * (float)mean, inv_std_out[c] = (float)(1 / sqrt(m2 / count + eps)), and 0, 1
 * (the identity) while count == 0.  eps is the only bound on inv_std
 * (<= 1 / sqrt(eps)): the fold cannot clip a normalised value.
 *
 * mas_policy_pack_norm: mas_policy_pack with the fold.  The layer-1 fragment
 * element is bf16(w1[f][k] * inv_std[k]) (an fp32 product, round to nearest
 * even); the bias is (float)((double)b1[f] - sum_k (double)w1r[f][k] *
 * (double)mean[k]), k ascending, w1r the ROUNDED bf16 weight -- the kernels
 * multiply x by those, so a column that sits at its mean cancels exactly --
 * then scaled as mas_policy_pack scales b1.  The rest of the image is
 * mas_policy_pack's.  mean == NULL and inv_std == NULL: mas_policy_pack, byte
 * for byte; only one of them NULL is an error. */
int64_t mas_obs_stats_scratch_doubles(int64_t n_rows, int32_t n_cols);
int mas_obs_stats(int64_t n_rows, int32_t n_cols, const void* x_bf16, int64_t x_stride,
                  double* sums, double* scratch, void* stream);
int mas_obs_norm_merge(int32_t n_cols, double* state, const double* batch, double eps,
                       float* mean_out, float* inv_std_out, void* stream);
int mas_policy_pack_norm(int32_t obs_dim, const float* w1, const float* b1, const float* w2,
                         const float* b2, const float* w3, const float* b3,
                         const float* mean, const float* inv_std, void* packed, void* stream);
int mas_policy_train(const void* packed, int32_t obs_dim, int64_t n_rows, const void* x_bf16, int64_t x_stride,
                     const int8_t* actions, const float* old_logp, const float* adv, const float* ret, float clip,
                     float vf_coef, float ent_coef, float scale, void* h1, void* h2, void* da1, void* da2, void* dz,
                     float* partials, void* stream);
/* mas_policy_train_ld: mas_policy_train with the row stride `ld` >= n_rows
 * of h1, h2, dA1, dA2, dz ([256 | 16][ld]; mas_policy_train: ld = n_rows).
 * A power-of-two stride (the trainer's 4.2M-row minibatch) puts every
 * feature row on the same HBM channels; a padded one reads and writes them
 * about 30 % faster. */
int mas_policy_train_ld(const void* packed, int32_t obs_dim, int64_t n_rows, const void* x_bf16, int64_t x_stride,
                        const int8_t* actions, const float* old_logp, const float* adv, const float* ret, float clip,
                        float vf_coef, float ent_coef, float scale, void* h1, void* h2, void* da1, void* da2, void* dz,
                        int64_t ld, float* partials, void* stream);
/* mas_policy_train_dw3: mas_policy_train_ld with the layer-3 weight gradient
 * accumulated inside the train kernel: h2 and dz are neither written nor
 * read (no buffers for them), and dw3_out [16*256 + 16] receives what
 * mas_policy_dw(16, 256, ...) computes from them (dW3 row-major, then db3):
 * bit-identical to it where its split-K records fall on 256-row blocks and
 * fill the GPU (the trainer's minibatches of 1310720 and 4194304 rows),
 * else the same fp32 sums of the same bf16 operands in another order;
 * deterministic from call to call either way.
 * scratch: mas_policy_dw_scratch(16, 256, n_rows) floats.
 * Only where the persistent train kernel covers every row: n_rows a multiple
 * of 256, 16*ceil(obs_dim/16) in {144, 160}, ld even and at most 2^32 / 514;
 * the environment variables MAS_POL_DW3=0 or MAS_POL_DB=0 (read per call)
 * switch it off.  Otherwise MAS_ERR_UNSUPPORTED: nothing is launched or
 * written, and the caller uses mas_policy_train_ld + mas_policy_dw. */
int mas_policy_train_dw3(const void* packed, int32_t obs_dim, int64_t n_rows, const void* x_bf16, int64_t x_stride,
                         const int8_t* actions, const float* old_logp, const float* adv, const float* ret, float clip,
                         float vf_coef, float ent_coef, float scale, void* h1, void* da1, void* da2, int64_t ld,
                         float* partials, float* dw3_out, float* scratch, void* stream);
/* mas_policy_train_w (an addition within ABI version 3): mas_policy_train_ld
 * with a weight per row on the POLICY terms of the loss -- what lets a
 * trainer mask the rows of dead agents (mas_alive), whose actions the env
 * ignores.  row_w: DEVICE float [n_rows], 4-B aligned, values >= 0.  With
 * w the row's weight, the row's gradient and loss terms are
 *   dz[k]  = scale w (glp (onehot - p) + ent_coef p (logsoftmax + H_head))
 *            for the 15 logits,
 *   dz[15] = scale vf_coef 2 (v - ret)             (not weighted),
 *   partials columns: w (-min(s1, s2)), (v - ret)^2, w entropy, w clipped.
 * The value term stays on for every row: a dead agent still receives reward
 * until the episode ends, and a live row's GAE bootstraps from the value of
 * the next, possibly dead, row.  A row with w == 0 gives exactly zero (+-0)
 * for its 15 logit gradients and its weighted loss terms whatever its other
 * inputs are (a selection, not a product: its ratio may be inf); w == 1 on
 * every row gives mas_policy_train_ld's outputs bit for bit.  The caller
 * chooses the normalisation (the trainer: scale = 1 / n_rows and w = active
 * n_rows / sum(active), so that the weighted columns sum to means over the
 * active rows).  The kernels and their dispatch (and MAS_POL_DB, MAS_POL_CW,
 * MAS_POL_FORCE_OFF64) are mas_policy_train_ld's; there is no row-major form.
 * MAS_ERR_INVALID_ARG, before any device work: a null or misaligned row_w
 * and whatever mas_policy_train_ld refuses.
 * mas_policy_train_dw3_w: the same for mas_policy_train_dw3, with its
 * conditions and its MAS_ERR_UNSUPPORTED (then: mas_policy_train_w +
 * mas_policy_dw); compared with that pair as mas_policy_train_dw3 is with
 * its own. */
int mas_policy_train_w(const void* packed, int32_t obs_dim, int64_t n_rows, const void* x_bf16, int64_t x_stride,
                       const int8_t* actions, const float* old_logp, const float* adv, const float* ret,
                       const float* row_w, float clip, float vf_coef, float ent_coef, float scale, void* h1, void* h2,
                       void* da1, void* da2, void* dz, int64_t ld, float* partials, void* stream);
int mas_policy_train_dw3_w(const void* packed, int32_t obs_dim, int64_t n_rows, const void* x_bf16, int64_t x_stride,
                           const int8_t* actions, const float* old_logp, const float* adv, const float* ret,
                           const float* row_w, float clip, float vf_coef, float ent_coef, float scale, void* h1,
                           void* da1, void* da2, int64_t ld, float* partials, float* dw3_out, float* scratch,
                           void* stream);
/* mas_policy_train_rm: the same kernel writing the activations ROW-major,
 * each lane storing its own row as 16-B chunks (no lane exchange):
 * h1, h2 [n_rows][ld_h] (ld_h >= 257, a multiple of 8; the caller keeps
 * column 256 = 1, the bias column, the kernel writes columns 0..255),
 * dA1, dA2 [n_rows][256], dz [n_rows][16] (outputs in natural order).
 * Within every 32-column tile the 256 hidden columns are stored permuted:
 * column c holds hidden feature mas_policy_rm_feature(c).  The weight
 * gradients are then the row-sum GEMMs dW2 = dA2^T h1, dW3 = dz^T h2,
 * dW1 = dA1^T x with rows / columns mapped back through that permutation. */
int mas_policy_train_rm(const void* packed, int32_t obs_dim, int64_t n_rows, const void* x_bf16, int64_t x_stride,
                        const int8_t* actions, const float* old_logp, const float* adv, const float* ret, float clip,
                        float vf_coef, float ent_coef, float scale, void* h1, void* h2, int64_t ld_h, void* da1,
                        void* da2, void* dz, float* partials, void* stream);
int32_t mas_policy_rm_feature(int32_t col);

/* mas_policy_adam: one PPO optimizer step over flat fp32 buffers of n
 * parameters, replacing torch.nn.utils.clip_grad_norm_(params, max_norm)
 * followed by torch.optim.Adam.step() (no weight decay, no amsgrad):
 * g' = grad_scale * grads (1 / world size after a summing all-reduce),
 * scaled by min(1, max_norm / (|g'|_2 + 1e-6)) (max_norm <= 0: no clipping),
 * then exp_avg, exp_avg_sq and params updated in place with the bias
 * corrections of `step` (>= 1, the step being taken).  grads is not written.
 * scratch: mas_policy_adam_scratch() floats. */
int64_t mas_policy_adam_scratch(void);
int mas_policy_adam(int64_t n, float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float grad_scale,
                    float max_norm, double lr, double beta1, double beta2, double eps, int64_t step, float* scratch,
                    void* stream);

/* mas_policy_dw: the weight and bias gradients of one policy layer from the
 * feature-major activations mas_policy_train writes, over the minibatch rows:
 * out[F*G + F] = (a [F][K] . b [G][K]^T, row sums of a) in fp32, a / b bf16
 * with K contiguous (row strides lda / ldb >= K, multiples of 8, 16-B aligned
 * rows); F = 256 (dW2 from dA2 and h1) or 16 (dW3 from dz and h2), G = 256,
 * K a multiple of 32.  scratch: mas_policy_dw_scratch(F, G, K) floats of
 * split-K partial sums.  Replaces the caller's GEMMs over the ones-row trick
 * for layers 2 and 3 (K % 64 == 0: the LDS-staged kernel); the dW1 GEMM
 * reads x row-major and stays a GEMM. */
int64_t mas_policy_dw_scratch(int32_t f, int32_t g, int64_t k);
int mas_policy_dw(int32_t f, int32_t g, int64_t k, const void* a, int64_t lda, const void* b, int64_t ldb, float* out,
                  float* scratch, void* stream);

/* Diagnostics (synchronises the device): host_out[0] = envs of the last
 * mas_step that left the contact-free physics fast path and ran the general
 * physics kernel (contacts, TOI events, box despawns). */
int mas_debug_counters(mas_handle* h, int64_t* host_out);

/* Diagnostics (synchronises the device): host_out[0] = appends to the
 * general-path env list (and the slow list) that their bounds refused since
 * mas_create.  The lists hold one entry per env and are emptied every step,
 * so this is 0 unless a kernel breaks that invariant; the tests assert it. */
int mas_debug_guards(mas_handle* h, int64_t* host_out);

/* Diagnostics (synchronises the device): host_out[0] = boxes, box items and
 * heals that were not spawned since mas_create because the env already held
 * the config's n_boxes / n_heals of them, the slots an observation row has.
 * Only the copies of double pickups make more items than a reset deals. */
int mas_debug_spawn_refused(mas_handle* h, int64_t* host_out);

/* Test diagnostics: bit 0 of `on` sends every env of every following
 * mas_step through the general physics path (the contact-free fast path
 * gives up for all envs); bit 1 (the former one-lane-per-env general
 * kernels, removed) is rejected with MAS_ERR_UNSUPPORTED and changes nothing;
 * bit 3 keeps mas_step on the caller's stream.  Default (MAS_SPLIT unset or
 * 2 in the environment at mas_create): the slow split, the envs whose last
 * general-path step had a SolveTOI at the sub-step cap (or >= MAS_SLOW_K,
 * default 4, TOI events) run their general path and post phases on the side
 * stream while the caller's stream runs the rest; it is on for 8 steps after
 * the general kernels last flagged such an env (a host-mapped signal), else
 * mas_step runs on one stream.  Bit 3 (or MAS_SPLIT=0): the caller's stream
 * alone -- the form a caller may capture into a graph and replay (the
 * general-path list is emptied on the device).  Bit 2 (the former
 * all-general split) is rejected with MAS_ERR_INVALID_ARG.  Results are
 * unchanged (every path is exact): A/B and parity tests only. */
int mas_debug_force_general(mas_handle* h, int32_t on);

/* Action validation.  The reference asserts action_space.contains(actions)
 * before every step (masurvival_env.py:80).  A kernel cannot raise, so
 * mas_step clamps each out-of-range entry into MultiDiscrete([3,3,3,2,2,2])
 * and counts the env-step; this returns that count since the handle was
 * created or last reset (synchronises; reset != 0 zeroes it).  The Python
 * facades check on the host before calling (MaSurvival.step always,
 * VecMaSurvival.step(validate=True)). */
int mas_invalid_actions(mas_handle* h, int64_t* host_count, int32_t reset);

/* Test diagnostics: copies the per-env "left the contact-free fast path in
 * the last mas_step" flags (uint8 [n_envs], device) into `flags`
 * (stream-ordered; no synchronisation). */
int mas_debug_gen_flags(mas_handle* h, uint8_t* flags, void* stream);

/* Test diagnostics: while `counts` (device int32 [n_envs], or NULL to stop)
 * is set, every mas_step adds per env the number of b2World::SolveTOI
 * events of its agents, plus 65536 for each agent whose SolveTOI reached
 * Box2D's sub-step cap (b2_maxSubSteps = 8 per contact). */
int mas_debug_set_toi_counter(mas_handle* h, int32_t* counts);

const char* mas_last_error(void);
int32_t mas_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MASURVIVAL_H */
