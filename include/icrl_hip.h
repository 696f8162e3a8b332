/* libicrl_hip.so — C ABI of the MI355X-native ICRL rollout+update hot path.
 *
 * The reference (shehryar-malik/icrl) is pure Python: its "FFI" for this path is the set of numpy / torch
 * calls made by the classes listed next to each entry point below (paths relative to /root/reference).
 * Each function here replaces the arithmetic of one such call site with a hand-written gfx950 kernel.
 *
 * Conventions (all entry points):
 *   - every pointer is DEVICE memory owned by the caller (torch-allocated HBM in the Python host);
 *     the library never allocates or frees user-visible memory;
 *   - `stream` is a hipStream_t (passed as void* so that the header needs no HIP include); work is
 *     enqueued asynchronously on it, there is no hidden synchronisation;
 *   - the return value is a hipError_t as int (0 = hipSuccess); nothing throws or aborts;
 *   - one host thread per GPU / process; re-entrant across devices, not thread-safe on shared buffers;
 *   - [T,N,...] arrays are time-major, contiguous, float32 unless stated (RolloutBufferWithCost layout,
 *     stable_baselines3/common/buffers.py:468-491).
 *   - structs are plain C, passed by pointer to HOST memory (they hold device pointers + scalars) and are
 *     only read during the call.
 *
 * Co-residency precondition of the PERSISTENT launches (icrl_rollout_collect[_ex|_batch], icrl_ppo_lag_train[_batch]): the
 * workgroups of ONE run wait for each other inside the launch (granule exchange), so they must all be resident at the same
 * time: n_envs workgroups of 256 threads for the rollout (<= 128 envs; the many-environment kernel sizes its grid to what
 * hipOccupancyMaxActiveBlocksPerMultiprocessor reports), 3 (6 when a minibatch is two chunks at obs_dim > 64) workgroups for
 * the update, each filling a CU's LDS.  The SINGLE-RUN entry points issue these grids with hipLaunchCooperativeKernel (round 4): the
 * runtime refuses a grid it cannot make co-resident (the rollout then falls back to per-step launches), after the library's own
 * check of the occupancy the runtime reports; the *_batch grids are ordinary launches.  Whatever else occupies CUs for long at the same time —
 * another stream of this process, or ANOTHER PROCESS on the same GPU, which no host-side check of this process can see — can
 * keep a workgroup of a run from being scheduled; its peers then spin (bounded: ~2 s per exchange, s_sleep between polls), the
 * launch ends with icrl_agent_t.status bit 0 / stats[11] set and the host raises — buffers and statistics of that call are
 * invalid, nothing hangs.  Runs of one *_batch grid do not wait for each other: a run whose workgroups do not fit yet starts
 * when earlier runs of the grid have finished (dispatch is in grid order).
 * XCD placement (speed only): the update launches and the batched multi-env rollout are 1-D grids in which the workgroups of run r sit
 * at 8 M (r / 8) + r % 8 + 8 j, j < M (M = 3 | 6 | workgroups of the rollout; surplus workgroups of the grid leave at once) — workgroups are
 * dealt round-robin over the 8 XCDs, so a run then sits on ONE XCD, and granules stored with workgroup scope stay in that XCD's L2 for
 * the other workgroups' polls.  Nothing relies on it: every workgroup publishes its HW_REG_XCC_ID once per launch and the workgroup-scope
 * stores are used only where all workgroups of a run reported the same XCD; batched grids too large for every XCD to hold its share at
 * once (32 CUs) keep the run-major layout (3 | 6 | G, n_runs) and agent-scope stores.
 */
#ifndef ICRL_HIP_H
#define ICRL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------------------------
 * Data descriptors
 * ------------------------------------------------------------------------------------------------------------------ */

/* Synthetic HCWithPos- / AntWall-shaped vectorised environment (oracle/synth_env.py is the spec).
 * Stands in for SubprocVecEnv + gym envs (stable_baselines3/common/vec_env/subproc_vec_env.py:14-50,104-113;
 * custom_envs/envs/half_cheetah.py:138-195, ant.py:40-108): float64 state, time-limit dones, auto-reset. */
typedef struct {
  int32_t n_envs, obs_dim, act_dim, max_steps;
  int32_t reward_form;    /* 0: |dx|/dt - 0.1|a|^2 (HC)   1: |xy| + 1 - 0.5|a|^2 (Ant)
                           * 2: LapGridWorld, 3: ConstrainedLapGridWorld (custom_envs/envs/lap_grid_world.py:62-240;
                           *    obs_dim 1, act_dim 1 = the Discrete(2) action index as a float; B / key unused)
                           * 4: PointCircle, 5: PointCircleTest (ends at |x| > 3), 6: PointCircleTestBack (ends at x < -3),
                           * 7: PointNullReward, 8: PointNullRewardTest (custom_envs/envs/point.py:22-276 stepped exactly;
                           *    obs_dim 9, act_dim 2, max_steps 150; B / key unused; the variant decides how an episode
                           *    ends, wall_terminate is not read)
                           * 9: PointTrack (point.py:284-376: the Point kinematics, reward movement + track, never ends early)
                           * 10: DD2B, 11: CDD2B (+ the constraint rectangle), 12: DDCDD2B (as 11, start (3, 5)): the dense discrete
                           *    Two Bridges envs (custom_envs/envs/two_bridges.py:94-117,237-328 stepped exactly; obs_dim 2,
                           *    act_dim 1 = the Discrete(4) action index as a float, max_steps 200)
                           * 13: C2B, 14: CC2B (+ the constraint rectangle): the continuous ones (:331-418; obs_dim 3 = x, y, ori,
                           *    act_dim 2 clipped to +-2, max_steps 200).  9..14: B / key unused, episodes end at max_steps only */
  int32_t wall_terminate; /* "Test" variants: done & reward 0 when obs[0] <= -3 */
  int32_t broken;         /* AntWallBroken: action[4:] = 0 */
  int32_t _pad;
  const double* B;        /* [obs_dim, act_dim] dynamics matrix */
  double* s;              /* [N, obs_dim] raw state == last raw observation (== VecCostWrapper.previous_obs) */
  int32_t* t_ep;          /* [N] step inside the episode */
  uint32_t* step_count;   /* [N] counter of the per-env random stream */
  const uint32_t* key;    /* [N] stream key = seed + global env index */
} icrl_env_t;

/* VecNormalizeWithCost state (stable_baselines3/common/vec_env/vec_normalize.py:9-181,184-278;
 * RunningMeanStd: common/running_mean_std.py:6-39).  All float64 as in the reference. */
typedef struct {
  int32_t training, norm_obs, norm_reward, norm_cost;
  double clip_obs, clip_reward, clip_cost, reward_gamma, cost_gamma, epsilon;
  double* obs_mean;   /* [obs_dim] */
  double* obs_var;    /* [obs_dim] */
  double* obs_count;  /* [1] */
  double* ret_stats;  /* [3] mean, var, count of ret_rms */
  double* cost_stats; /* [3] mean, var, count of cost_rms */
  double* ret;        /* [N] discounted reward return */
  double* cost_ret;   /* [N] discounted cost return */
} icrl_norm_t;

/* ActorTwoCriticsPolicy parameters (stable_baselines3/common/policies.py:598-779): three tanh MLPs obs->h1->h2
 * (pi, vf, cvf), heads h2->act / 1 / 1, state-independent log_std.  `params` is ONE flat float32 buffer in the
 * reference's state_dict order: log_std[A] (absent when discrete), then for pi, vf, cvf: W1[h1,obs] b1[h1] W2[h2,h1]
 * b2[h2], then action_net W[A,h2] b[A], value_net W[1,h2] b[1], cost_value_net W[1,h2] b[1].
 *
 * Any other MlpExtractor architecture (common/torch_layers.py:129-254: `-sl` shared trunk, `-pl / -rvl / -cvl` of any depth) is
 * described by `arch`, HOST memory: { n_shared, widths..., n_pi, widths..., n_vf, widths..., n_cvf, widths... } with 0..4 layers per
 * group and 1..256 units per layer (a branch without layers feeds its head from the trunk, or from the observation).  h1 / h2 are then
 * ignored and `params` holds the natural, unpadded layout in state_dict order: log_std, the trunk's layers (W[out,in] b[out] each),
 * policy_net's, value_net's, cost_value_net's, then the three heads.  Such a policy is served by icrl_policy_forward,
 * icrl_policy_evaluate, icrl_ppo_lag_train, icrl_rollout_collect(_ex) and icrl_sample_episodes (generic-shape path: one persistent launch
 * per update / rollout / sampling call like the fast path, slower per step — DESIGN.md section 8); the *_batch entry points refuse it. */
typedef struct {
  int32_t obs_dim, act_dim, h1, h2;
  int32_t discrete; /* 1: Categorical over act_dim logits (LGW), 0: DiagGaussian */
  int32_t n_params;
  float* params;     /* [n_params] */
  float* params_t;   /* [n_params] transposed copy for the forward kernels (written by icrl_policy_prepare; icrl_ppo_lag_train keeps it current) */
  const int32_t* arch; /* NULL: two hidden layers per branch (h1, h2), no shared trunk */
} icrl_policy_t;

/* ConstraintNet zeta_theta (icrl/constraint_net.py:14-130,258-299): ReLU MLP + sigmoid over
 * concat(clip(obs), clip(acs))[select_dim]; cost = 1 - zeta.  n_hidden hidden layers of h1 .. h4 units (`-cl`, torch_layers.py:93-126):
 * 1 or 2 layers of up to 64 units inside the fused rollouts; 0..4 layers through icrl_cost_mlp_forward / icrl_disc_reward /
 * icrl_cn_train* (64 rows per workgroup) as long as the 64-row activation images fit the 160 KB LDS — e.g. 2 x 128, 3 x 96, 4 x 64 units
 * (refused with the byte count otherwise).  params flat in state_dict order: W0[h1,in] b0[h1] (W1[h2,h1] b1[h2] ...) Wo[1,h] bo[1]. */
typedef struct {
  int32_t obs_dim, acs_dim, in_dim, n_hidden, h1, h2, h3, h4;
  int32_t is_discrete;  /* one-hot the action first */
  int32_t n_params;
  double clip_obs;           /* < 0: no clipping (what ConstraintNet.load builds, constraint_net.py:394-399) */
  const int32_t* select_dim; /* [in_dim] indices into concat(obs, acs) */
  const float* action_low;   /* [acs_dim] or NULL: no action clipping */
  const float* action_high;  /* [acs_dim] or NULL */
  const double* obs_mean;    /* [obs_dim] or NULL (--cn_normalize) */
  const double* obs_var;     /* [obs_dim] or NULL */
  double eps;
  float* params;             /* [n_params] */
  float* params_t;           /* [n_params] transposed copy (written by icrl_costnet_prepare) */
} icrl_costnet_t;

/* Analytic (closed-form) cost: the ground-truth constraints of icrl/true_constraint_net.py:13-55 and the null cost, evaluated on
 * (previous raw observation float64, clipped action float32) exactly where the constraint net is.  Its first four int32 alias the
 * first four of icrl_costnet_t; n_hidden == ICRL_COST_FN is the tag: every entry point that takes `const icrl_costnet_t* cn` reads a
 * descriptor carrying it as an icrl_cost_fn_t (cast the pointer).  Served by icrl_rollout_collect[_ex][_mon], icrl_host_step[_mon],
 * icrl_cost_mlp_forward (= icrl_cost_fn_rows) and, for seed batches, icrl_rollout_collect_batch_cost; refused with a reason by
 * icrl_rollout_collect_batch[_mon], icrl_cn_train*, icrl_cn_prepare,
 * icrl_disc_reward and icrl_costnet_prepare.  (The other tagged descriptor is icrl_cost_disc_t below: n_hidden == ICRL_COST_DISC.)
 * Operation for operation what numpy computes in the reference's callables:
 *   NULL           0
 *   WALL_BEHIND    obs[index] <= lo                      (float64 compare on the raw observation; wall_behind)
 *   WALL_INFRONT   obs[index] >= hi                      (wall_infront)
 *   WALL_BOTH      float(obs[index] <= lo) + float(obs[index] >= hi)   (wall_behind_and_infront; 2 when lo >= hi and both hold)
 *   TORQUE         any_a |acs[a]| > (float)lo, a < acs_dim   (float32 compare on the clipped action; torque_constraint)
 *   ACTION_EQUALS  discrete action == index              (lap_grid_world: index 1)
 * The result is a float 0 / 1 / 2. */
#define ICRL_COST_FN (-1)            /* value of n_hidden that marks an analytic cost */
#define ICRL_COST_NULL 0
#define ICRL_COST_WALL_BEHIND 1
#define ICRL_COST_WALL_INFRONT 2
#define ICRL_COST_WALL_BOTH 3
#define ICRL_COST_TORQUE 4
#define ICRL_COST_ACTION_EQUALS 5
typedef struct {
  int32_t obs_dim, acs_dim, in_dim /* 0 */, n_hidden /* ICRL_COST_FN */;
  int32_t kind;     /* ICRL_COST_* */
  int32_t index;    /* observation column (wall kinds) / action value (ACTION_EQUALS) */
  double lo, hi;    /* thresholds */
} icrl_cost_fn_t;

/* Discriminator cost: a constraint net read as D = zeta instead of 1 - zeta — the cost of `cpg --load_gail` (icrl/cpg.py:54-83:
 * GailDiscriminator.reward_function(previous raw obs, clipped action, apply_log = False)).  Like icrl_cost_fn_t a tagged descriptor
 * behind a `const icrl_costnet_t*`: its first four int32 alias the first four of icrl_costnet_t (copies of the inner net's, n_hidden
 * excepted), n_hidden == ICRL_COST_DISC is the tag, `net` the constraint net proper, prepared (icrl_costnet_prepare) and limited as a
 * constraint net is.  zeta is computed once and returned: the bits of icrl_disc_reward(net, ..., apply_log = 0), never 1 - (1 - zeta).
 * Served by icrl_rollout_collect[_ex][_mon] on every route of a single run, icrl_host_step[_mon] and icrl_cost_mlp_forward; refused
 * with a reason by icrl_rollout_collect_batch[_mon | _cost] (the batched kernels have no discriminator form), icrl_cn_train*,
 * icrl_cn_prepare, icrl_costnet_prepare, icrl_disc_reward and the GAIL batch entry points (hand those the inner net). */
#define ICRL_COST_DISC (-2)          /* value of n_hidden that marks a discriminator cost */
typedef struct {
  int32_t obs_dim, acs_dim, in_dim, n_hidden /* ICRL_COST_DISC */;
  const icrl_costnet_t* net;
} icrl_cost_disc_t;

/* Region cost: a user-defined ground-truth constraint, described by data and evaluated by the rollout kernels themselves on (previous
 * raw observation float64, clipped action float32; one column, the class index, beside a discrete policy).  The third tagged
 * descriptor behind a `const icrl_costnet_t*`: n_hidden == ICRL_COST_REGION.  Column c < obs_dim is observation column c, column
 * obs_dim + j action column j; every value is taken as float64 (widening a float32 is exact).  1..8 clauses of 1..8 terms each:
 *   BOX        true iff for every term  a[k] <= x_k && x_k <= b[k]            (a = lo, b = hi; +-inf allowed)
 *   HALFSPACE  acc = c; in term order acc = acc + a[k] * x_k; true iff acc >= 0   (a = w, c = the offset; every product and every
 *              sum rounded once to float64, no fused multiply-add)
 *   BALL       acc = 0; in term order d = x_k - a[k], acc = acc + d * d; true iff acc <= c   (a = centre, c = radius * radius,
 *              computed once on the host)
 * `negate` flips a clause; IEEE comparisons, so a NaN makes the un-negated clause false.  combine: ANY 1 if any clause is true,
 * ALL 1 if every clause is true, SUM the number of true clauses; the result is a float.  Every analytic kind is a member of the family
 * (wall_behind(p, i) = box on column i with hi = p; torque(t) = negated box [-t, t] over all action columns; ...).
 * `clauses` is a HOST pointer (every check runs on it before the first HIP call), `d_clauses` a DEVICE pointer to the same
 * n_clauses * sizeof(icrl_region_clause_t) bytes, uploaded once by the caller like a prepared params_t; the kernels copy the table into
 * LDS before their step loop.  Served by icrl_rollout_collect[_ex][_mon] on every route of a single run but the generic-shape ones,
 * icrl_host_step[_mon], icrl_cost_mlp_forward and icrl_cost_region_rows; refused with a reason by every *_batch* rollout,
 * icrl_rollout_collect_sde, generic-shape policies, icrl_cn_train*, icrl_cn_prepare, icrl_costnet_prepare, icrl_disc_reward, the GAIL
 * batch entry points and as the inner net of an icrl_cost_disc_t. */
#define ICRL_COST_REGION (-3)        /* value of n_hidden that marks a region cost */
#define ICRL_REGION_MAX_CLAUSES 8
#define ICRL_REGION_MAX_TERMS 8
#define ICRL_REGION_BOX 0
#define ICRL_REGION_HALFSPACE 1
#define ICRL_REGION_BALL 2
#define ICRL_REGION_ANY 0
#define ICRL_REGION_ALL 1
#define ICRL_REGION_SUM 2
typedef struct {
  int32_t type /* ICRL_REGION_BOX | HALFSPACE | BALL */, negate, n_terms, _pad;
  int32_t col[ICRL_REGION_MAX_TERMS];
  double a[ICRL_REGION_MAX_TERMS], b[ICRL_REGION_MAX_TERMS];
  double c;
} icrl_region_clause_t;
typedef struct {
  int32_t obs_dim, acs_dim, in_dim /* 0 */, n_hidden /* ICRL_COST_REGION */;
  int32_t n_clauses, combine /* ICRL_REGION_ANY | ALL | SUM */;
  const icrl_region_clause_t* clauses;      /* host */
  const icrl_region_clause_t* d_clauses;    /* device, the same bytes */
} icrl_cost_region_t;

/* RolloutBufferWithCost arrays (stable_baselines3/common/buffers.py:443-491), time-major [T,N,...] float32. */
typedef struct {
  int32_t T, N, obs_dim, act_store; /* act_store = act_dim (Box) or 1 (Discrete) */
  float *observations, *new_observations, *orig_observations, *new_orig_observations; /* [T,N,obs] */
  float* actions;                                                                      /* [T,N,act_store] */
  float *dones, *log_probs, *rewards, *reward_values, *costs, *orig_costs, *cost_values;
  float *reward_advantages, *reward_returns, *cost_advantages, *cost_returns; /* [T,N] */
  void* gae_ws;             /* optional workspace of the GAE launch (see icrl_gae_dual_ws): device memory, zeroed once when */
  long long gae_ws_bytes;   /* allocated, afterwards written by GAE launches only.  NULL: one workgroup per column tile */
} icrl_buffer_t;
#define ICRL_GAE_WS_BYTES (256 * (256 * 8 + 4) + 64)   /* 256 maps + flags, + the status word */

/* What OnPolicyWithCostAlgorithm carries between steps (common/on_policy_algorithm.py:367-416, base_class.py:346-353)
 * plus per-step scratch. */
typedef struct {
  double* last_obs;      /* [N,obs] normalised observation fed to the policy (== _last_obs) */
  uint8_t* last_dones;   /* [N] */
  double* raw_rew;       /* [N] scratch: un-normalised reward of the step (== get_original_reward) */
  float* raw_cost;       /* [N] scratch: zeta-cost of the step (== get_original_cost) */
  uint8_t* dones;        /* [N] scratch: done flags of the step */
  float* last_v_r;       /* [N] values of the last forward (GAE bootstrap, on_policy_algorithm.py:417) */
  float* last_v_c;       /* [N] */
  float* act_clipped;    /* [N,act] scratch: action handed to the env */
  int* status;           /* [1] or NULL: the persistent rollout ORs bit 0 into it when an inter-workgroup exchange timed out
                          * (a workgroup was not resident); the buffer contents are then invalid and the caller must raise */
  void* xch_ws;          /* optional exchange workspace of the persistent rollout (device memory, any contents) ... */
  long long xch_ws_bytes;/* ... and its size; >= ICRL_ROLLOUT_WS_BYTES(N, obs) suffices for both persistent kernels.  NULL / too small: the not yet
                          * computed reward_advantages plane of the buffer is used when T is large enough, else per-step launches */
} icrl_agent_t;
#define ICRL_ROLLOUT_WS_BYTES(n_envs, obs_dim) (48 * (size_t)(n_envs) * (size_t)(obs_dim) + 96 * (size_t)(n_envs) + 64 * (size_t)(obs_dim) + 2048)

/* PPO-Lagrangian update hyper-parameters (stable_baselines3/ppo_lag/ppo_lag.py:67-103,177-196; Adam eps 1e-5 from
 * common/policies.py:357-361). */
typedef struct {
  int32_t batch_size, n_epochs, use_target_kl, _pad;
  float clip_range, ent_coef, reward_vf_coef, cost_vf_coef, max_grad_norm, target_kl;
  float clip_range_reward_vf, clip_range_cost_vf; /* < 0: no value clipping (the default) */
  float lr, adam_beta1, adam_beta2, adam_eps;
} icrl_ppo_hyper_t;

/* ConstraintNet.train hyper-parameters (icrl/constraint_net.py:15-42,137-229). */
typedef struct {
  int32_t iterations, importance_sampling, per_step, gail;
  float reg_coeff, eps, target_kl_old_new, target_kl_new_old; /* target < 0 (== -1): that KL test is disabled */
  float lr, adam_beta1, adam_beta2, adam_eps;
} icrl_cn_hyper_t;

#define ICRL_PPO_SPLIT_BYTES (2560 * 1024) /* exchange space of the multi-workgroup updates: partial gradients (2 step parities x 3 networks x up to 4 parts), updated parameters */
/* granule slots (512 B) + the schedule tables: 16 B per optimiser step and 8 B per 64-row chunk (up to four per step) */
#define ICRL_PPO_PLAN_BYTES(n_steps) (768 + 48 * (size_t)(n_steps))
#define ICRL_PPO_SYNC_BYTES(n_epochs, n_minibatches, n_rows) \
  (ICRL_PPO_PLAN_BYTES((size_t)(n_epochs) * (size_t)(n_minibatches)) + 4 * (size_t)(n_epochs) * (size_t)(n_rows) + 256 + ICRL_PPO_SPLIT_BYTES)
/* generic-shape update (hidden widths above 64, a policy with `arch`, or batch_size above 256): its scratch lies BEHIND the regular
 * workspace, sync_ws then holds ICRL_PPO_SYNC_BYTES(...) + ICRL_PPO_GENERIC_BYTES(...) bytes.  row_floats = the outputs of every layer
 * of one row = icrl_ppo_generic_row_floats(pol) (6 h + act_dim + 2 for the padded two-layer layout of common width h) */
#define ICRL_PPO_GENERIC_BYTES(batch_size, row_floats, n_params) \
  (4 * (64 + (size_t)(batch_size) * (24 + 1 + 16 + 2 * (size_t)(row_floats)) + (size_t)(n_params) + ((size_t)(n_params) + 255) / 256 + 1088 + \
        ICRL_PPO_GENERIC_PERSIST_FLOATS(batch_size, n_params)))
/* the one-launch form of the generic-shape update (up to 32 row tiles of 16 rows, up to 131 072 parameters): per-tile partial gradients */
#define ICRL_PPO_GENERIC_PERSIST_FLOATS(batch_size, n_params) \
  ((((batch_size) + 15) / 16 <= 32 && (n_params) <= 131072) ? (size_t)(((batch_size) + 15) / 16 + 1) * (size_t)(n_params) + 1024 : (size_t)0)
#define ICRL_CN_METRICS 24 /* floats per iteration in the metrics array of icrl_cn_train */

/* ------------------------------------------------------------------------------------------------------------------
 * Entry points
 * ------------------------------------------------------------------------------------------------------------------ */

/* ABI version (major*100+minor). */
int icrl_abi_version(void);   /* 107: icrl_debug_last_route (additive since, no bump: icrl_ppo_stream_ws_bytes, icrl_ppo_lag_train_stream, word [4] of the update route); 106: icrl_explained_variance, icrl_gae_dual_ws_bytes + the status word of the GAE workspace; 105: icrl_buffer_add, icrl_is_weights, icrl_cn_loss_fwd_bwd; 104: the fine-grained update entry points (csrc/fine.hip); 103: icrl_debug_stream_ref; 102: icrl_policy_t.arch; 101: icrl_sample_episodes takes stream_row0 / total_rows; the *_batch entry points */

/* Every entry point returns a hipError_t.  When it is hipErrorInvalidValue because the arguments are outside what the
 * kernels were built for (env count, widths, batch size ...; the reference's Python raises ValueError / AssertionError with a
 * message at the same places, e.g. stable_baselines3/common/buffers.py:352, on_policy_algorithm.py:141), the reason is kept
 * as text for the calling host thread until the next refusal; icrl_clear_error() empties it. */
const char* icrl_last_error(void);
void icrl_clear_error(void);

/* Dual reward+cost GAE over a [T,N] rollout in ONE launch.
 * Replaces RolloutBufferWithCost.compute_returns_and_advantage / _compute_returns_and_advantage
 *   (stable_baselines3/common/buffers.py:493-552), including its dtype behaviour: float32 delta for t<T-1,
 *   float64 running advantage, float32 rounding on store, returns = adv + values in float32.
 * dones[t,n] is the done flag ENTERING step t (what the buffer stores); last_dones[n] the final step's flag (0/1 bytes).
 * Algorithmic traffic: 36 B per transition (5 loads + 4 stores of 4 B). */
int icrl_gae_dual(const float* rewards, const float* costs, const float* reward_values, const float* cost_values,
                  const float* dones, const float* last_v_r, const float* last_v_c, const uint8_t* last_dones,
                  float* adv_r, float* adv_c, float* ret_r, float* ret_c,
                  int T, int N, double reward_gamma, double reward_gae_lambda, double cost_gamma, double cost_gae_lambda,
                  void* stream);

/* Same kernel with the launch shape forced (roofline sweep): waves_per_tile in {1,4,16}; 0 = library heuristic;
 * 101 / 105 / 106 = one-wave-per-tile shapes with 1 / 4 / 4 tiles per workgroup and 8 / 8 / 16 rows in flight;
 * 107..112 = four columns per lane (16-byte accesses; N % 4 == 0): 2 / 4 / 8 rows in flight with 4 waves (107-109) or 1 wave
 * (110-112) per workgroup.  All 1xx shapes are bit-exact replicas of the sequential scan. */
int icrl_gae_dual_ex(const float* rewards, const float* costs, const float* reward_values, const float* cost_values,
                     const float* dones, const float* last_v_r, const float* last_v_c, const uint8_t* last_dones,
                     float* adv_r, float* adv_c, float* ret_r, float* ret_c,
                     int T, int N, double reward_gamma, double reward_gae_lambda, double cost_gamma, double cost_gae_lambda,
                     int waves_per_tile, void* stream);

/* The same scan with a caller-owned workspace (zeroed once at allocation and written by these launches only).  Up to 65 472 envs and
 * T <= 2048 (round 6): the REGISTER-RESIDENT split scan — ceil(T / 128) workgroups per 64-env column tile, each wave keeps its 16 rows in
 * registers between the two passes of a two-level scan over affine maps, so every byte is read once (the BASELINE-size launch, 64 envs x
 * 2048 rows, walks 16 rows per wave instead of 128; 8 192 .. 65 472 envs get 2 048 .. 16 368 workgroups instead of one wave per tile).
 * It needs icrl_gae_dual_ws_bytes(T, N) bytes; ICRL_GAE_WS_BYTES suffices for up to 1024 envs at T <= 2048.  With less (or T > 2048) and up
 * to 128 column tiles: the older two-pass split over up to 16 workgroups per tile.
 * The LAST 4 bytes of the workspace (of its size rounded down to 8) are the launch's STATUS word: every wait for another workgroup's map is
 * bounded (~seconds); a map that never arrives ends the wait with status = 1 and invalid outputs — the caller checks and clears it.
 * waves_per_tile as above, or 200 + C to force the two-pass split with C workgroups per tile, 500 the register-resident split; 300 + C and
 * 501 are those two with one map withheld and a short limit (fault injection for the tests).  ws == NULL: identical to icrl_gae_dual_ex. */
size_t icrl_gae_dual_ws_bytes(int T, int N);
int icrl_gae_dual_ws(const float* rewards, const float* costs, const float* reward_values, const float* cost_values,
                     const float* dones, const float* last_v_r, const float* last_v_c, const uint8_t* last_dones,
                     float* adv_r, float* adv_c, float* ret_r, float* ret_c,
                     int T, int N, double reward_gamma, double reward_gae_lambda, double cost_gamma, double cost_gae_lambda,
                     int waves_per_tile, void* ws, long long ws_bytes, void* stream);

/* Write the transposed ([in][out]) weight copies the rollout-time kernels read coalesced.  Call after every change of
 * `params` (policy: after train(); cost net: after ConstraintNet.train / load). */
int icrl_policy_prepare(const icrl_policy_t* pol, void* stream);
int icrl_costnet_prepare(const icrl_costnet_t* cn, void* stream);

/* ActorTwoCriticsPolicy.forward (policies.py:716-731) for N observations: sample (mean + noise*std, or inverse-CDF on
 * `noise` uniforms when discrete; deterministic: mean / argmax), log-prob, both values.
 * obs: [N,obs] float64 (cast to float32 like preprocess_obs, preprocessing.py:61).  noise: [N,act] standard normals
 * ([N] uniforms when discrete) or NULL when deterministic.  actions: [N,act_store] unclipped; act_clipped: [N,act]
 * clipped to [low,high] (on_policy_algorithm.py:381-382; NULL low/high: no clipping).  Any output may be NULL.
 * Policies stored with h1 = h2 > 64 (a multiple of 64 up to 256; obs up to 1024) or described by `arch` run the generic-shape kernel
 * here and in icrl_policy_evaluate (it reads the per-layer transposes icrl_policy_prepare leaves in params_t); icrl_rollout_collect(_ex)
 * then runs the whole rollout as ONE persistent launch around that forward (up to 128 envs with a constraint net of at most two layers
 * of 64 units; otherwise the reference's per-step loop as four launches per step: policy forward, constraint-net cost, env step,
 * normaliser) and icrl_sample_episodes runs its episode loop with that forward;
 * the *_batch entry points refuse such shapes with a message. */
int icrl_policy_forward(const icrl_policy_t* pol, const double* obs, const float* noise, int N, int deterministic,
                        const float* action_low, const float* action_high,
                        float* actions, float* act_clipped, float* v_r, float* v_c, float* log_prob, void* stream);

/* same, with options in `do_gae`: bit 0 = run the final dual-GAE launch (0: the caller launches icrl_gae_dual itself, e.g.
 * bracketed by events); bit 1 = force one launch pair per env step; bit 2 = diagnostic phase timers.  By default ALL T steps run in ONE persistent launch
 * where one of the kernels serves the shape — which one, in which order, and what is left to the launch pair per step (AntWall with
 * 37..114 envs, for one) is stated once, in the comment above icrl_rollout_collect_ex_mon in csrc/rollout_collect.hip; icrl_debug_last_route reports
 * what a call took.  Up to 96 envs with N * obs_dim <= 4096 (128 envs with frozen statistics) that is one workgroup per env, one
 * device-wide barrier per step, normaliser statistics replicated bit-identically in every workgroup; its exchange scratch is
 * icrl_agent_t.xch_ws, or the not yet computed reward_advantages plane of the buffer when xch_ws is absent or too small. */
int icrl_rollout_collect_ex(const icrl_env_t* env, const icrl_norm_t* nm, const icrl_policy_t* pol, const icrl_costnet_t* cn,
                            const icrl_buffer_t* buf, const icrl_agent_t* ag, const float* noise,
                            const float* action_low, const float* action_high,
                            double reward_gamma, double reward_gae_lambda, double cost_gamma, double cost_gae_lambda,
                            int do_gae, void* stream);

/* Rollout over HOST envs (Python simulators, vec_env.HostVecEnv): one launch per env step, T + 1 launches per rollout
 * (k = 0 .. T), one workgroup of 256 threads per env, no inter-workgroup waiting inside a launch.  Launch k
 *   - finishes step k - 1 (k >= 1): reads the staging block the host copied in before the launch (raw obs f64 [N, O] | raw rew
 *     f64 [N] | done u8 [N]) and the raw costs launch k - 1 computed, updates the normaliser's statistics (replicated in every
 *     workgroup, numpy's order, as icrl_rollout_collect_ex does), normalises its env and writes buffer row k - 1 (new_observations,
 *     new_orig_observations, rewards, costs), ag.last_obs / last_dones / raw_rew / dones and row n of `s`;
 *   - acts for step k (k < T): policy forward on noise row k, cost net on (s, clipped action), the pre-step fields of buffer row k,
 *     ag.raw_cost / act_clipped / last_v_r / last_v_c, and the clipped action (Discrete: the index) into `act_host`.
 * The running statistics and the returns ret / cost_ret travel between launches in two copies in `ws` (step parity); the last
 * launch (k == T) also writes them to the icrl_norm_t arrays.  No GAE: the caller runs icrl_gae_dual after launch T.
 * Served: policies / constraint nets of the one-workgroup-per-env image (icrl_rollout_collect_ex's fused shapes), N <= 128,
 * obs_dim <= 128, nm->training; anything else is refused with a reason (the host then runs the per-step loop). */
typedef struct icrl_host_step_t {
  int T;                 /* rollout length: launches k = 0 .. T */
  int _pad;
  const void* stage;     /* device copy of the staging block: raw obs f64 [N, O] | raw rew f64 [N] | done u8 [N] */
  double* s;             /* [N, O] float64: the raw observations of the envs' last step (HostVecEnv.s, VecCostWrapper.previous_obs) */
  float* act_host;       /* HOST address of page-locked memory (hipHostMalloc / hipHostRegister; the call maps it with hipHostGetDevicePointer):
                            [N, act] float32 clipped actions ([N, 1] action index when discrete) */
  void* ws;              /* icrl_host_step_ws_bytes(N, O) bytes of device memory */
  long long ws_bytes;
} icrl_host_step_t;

size_t icrl_host_step_ws_bytes(int N, int obs_dim);
int icrl_host_step(const icrl_norm_t* nm, const icrl_policy_t* pol, const icrl_costnet_t* cn, const icrl_buffer_t* buf,
                   const icrl_agent_t* ag, const icrl_host_step_t* hs, const float* noise, const float* action_low,
                   const float* action_high, int k, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Training-episode statistics: the reference's Monitor wrapper + ep_info_buffer (rollout/ep_rew_mean, rollout/ep_len_mean)
 * ------------------------------------------------------------------------------------------------------------------
 * stable_baselines3/common/monitor.py:91-122 (Monitor.step around every single env), common/base_class.py:328-332, 368-389
 * (ep_info_buffer = deque(maxlen=100), _update_info_buffer once per env step over the envs in index order).
 * Optional and additive: the `_mon` forms of the rollout entry points take this descriptor and store the raw (un-normalised) env
 * reward of every step — the double they store into icrl_agent_t.raw_rew — into raw_rewards[t * N + n] as well; with a NULL
 * descriptor they ARE the entry points without the suffix (which forward with NULL).  icrl_monitor_scan, called once after a rollout on
 * the rollout's stream, turns the plane into episode records:
 *   - per env, ep_ret is the sequential float64 sum in step order of the raw rewards since the episode began (from +0.0), ep_len the
 *     step count; both carry over from one rollout to the next (the caller zeroes them where it resets the envs);
 *   - the done flag of step t is dones_plane[(t + 1) * N + n] for t < rows - 1 (the buffer stores the flag ENTERING a step) and
 *     last_dones[n] for t = rows - 1; a time-limit end counts;
 *   - when step t of env n is done, (ep_ret, ep_len) is appended and both restart from zero.  Append order: step-major, env index
 *     ascending within a step.  Record number i (counted from 0 since the caller last zeroed win_state[0]) lies in slot i % 100;
 *     win_state[0] counts all records: min(win_state[0], 100) slots are valid, the oldest is slot win_state[0] % 100 once the ring is full;
 *   - rows < T: a rollout a callback ended after `rows` steps.
 * Returns are stored UNROUNDED (the reference rounds to 6 decimals in Python; so does the host).  Two plain launches, no waiting
 * between workgroups, no host synchronisation. */
typedef struct {
  double* raw_rewards;        /* [T, N] float64, time-major */
  double* ep_ret;             /* [N] raw return of the episode in progress */
  int32_t* ep_len;            /* [N] its length so far */
  double* win_ret;            /* [100] ring of finished episodes: raw return */
  int32_t* win_len;           /* [100] length */
  int32_t* win_state;         /* [2] records appended since the last clear | reserved */
  int32_t* ws;                /* icrl_monitor_ws_bytes(T, N) bytes of device scratch, any contents (only icrl_monitor_scan reads it) */
  long long ws_bytes;
} icrl_monitor_t;

size_t icrl_monitor_ws_bytes(int T, int N);
int icrl_monitor_scan(const icrl_monitor_t* m, const float* dones_plane, const uint8_t* last_dones, int T, int N, int rows, void* stream);

/* icrl_rollout_collect_ex / icrl_host_step with the raw-reward plane of `mon` (NULL: exactly the entry point without the suffix) */
int icrl_rollout_collect_ex_mon(const icrl_env_t* env, const icrl_norm_t* nm, const icrl_policy_t* pol, const icrl_costnet_t* cn,
                                const icrl_buffer_t* buf, const icrl_agent_t* ag, const float* noise,
                                const float* action_low, const float* action_high,
                                double reward_gamma, double reward_gae_lambda, double cost_gamma, double cost_gae_lambda,
                                int do_gae, const icrl_monitor_t* mon, void* stream);
int icrl_host_step_mon(const icrl_norm_t* nm, const icrl_policy_t* pol, const icrl_costnet_t* cn, const icrl_buffer_t* buf,
                       const icrl_agent_t* ag, const icrl_host_step_t* hs, const float* noise, const float* action_low,
                       const float* action_high, int k, const icrl_monitor_t* mon, void* stream);

/* Sampling / evaluation episodes over ONE HOST env (utils.HostEpisodeRun): one launch per env step, `rows` + 1 launches at most
 * (k = 0 .. rows), one workgroup of 256 threads, a plain launch.  Launch k is one pass of icrl_sample_episodes' loop around the env
 * step, the raw observation coming from the staging block the host copied in before the launch (raw obs f64 [O] first): the reset
 * observation for k = 0, else what the env returned for step k - 1 (after `done`: the auto-reset observation).  It
 *   - normalises with the frozen statistics of `nm` (norm_obs, epsilon, clip_obs; nothing of `nm` is written);
 *   - for k >= 1 writes row k - 1 of orig_obs / obs: the observation after step k - 1;
 *   - with `act` != 0 runs the policy forward (mode when `deterministic` or noise == NULL, else sampled on noise row k) and writes
 *     the clipped action (Discrete: the index) to `act_host` and to row k of `actions`.
 * The launch after the last episode's last step passes act = 0: it only finishes that step.  Episode returns and lengths are the
 * host's (it has every reward and done flag).
 * Served: what icrl_host_step serves of the policy (the one-workgroup-per-env image), obs_dim <= 128, num_envs == 1, a frozen
 * normaliser; anything else is refused with a reason (the host then runs the per-step loop). */
typedef struct icrl_host_episode_t {
  int num_envs;          /* 1 */
  int obs_dim;
  int rows;              /* rows of `noise` and of the outputs (episodes x the env's step limit) */
  int deterministic;
  const void* stage;     /* device copy of the staging block: raw obs f64 [O] | ... */
  float* act_host;       /* HOST address of page-locked memory (see icrl_host_step_t): [act] float32 clipped action ([1] index when discrete) */
  double* orig_obs;      /* [rows, O] raw observation AFTER each step */
  double* obs;           /* same, normalised */
  float* actions;        /* [rows, act] clipped action that produced it ([rows, 1] index when discrete) */
} icrl_host_episode_t;

int icrl_host_episode_step(const icrl_norm_t* nm, const icrl_policy_t* pol, const icrl_host_episode_t* he, const float* noise,
                           const float* action_low, const float* action_high, int k, int act, void* stream);

/* ActorTwoCriticsPolicy.evaluate_actions (policies.py:752-767): values, log-prob of the GIVEN actions and the entropy of
 * the action distribution (used by compute_kl, icrl/utils.py:421-437).  actions [N,act_store] float32. */
int icrl_policy_evaluate(const icrl_policy_t* pol, const double* obs, const float* actions, int N, float* v_r, float* v_c,
                         float* log_prob, float* entropy, void* stream);

/* sample_from_agent (icrl/utils.py:323-357) / evaluate_policy (stable_baselines3/common/evaluation.py:10-67) on single-env
 * streams, one persistent workgroup per stream: env->n_envs independent streams each run `episodes_per_stream` episodes
 * back to back (auto-reset between them, like a 1-env VecEnv) with FROZEN normaliser statistics (nm->training must be 0).
 * Row k of a stream records the observation AFTER step k (raw in orig_obs, normalised in obs) next to the clipped action
 * of step k — the (s_{t+1}, a_t) pairing of the reference — at rows [stream*rows_per_stream + k].  noise: standard normals
 * [n_streams*rows_per_stream, act] (NULL or deterministic != 0: mode of the distribution).  do_reset: draw the initial
 * state first (VecEnv.reset).  Per-episode un-normalised reward sums and lengths go to ep_rewards / ep_lengths.
 * stream_row0 ([n_streams] int32 on the device, or NULL): first row of every stream in the noise and output arrays instead of
 * stream * rows_per_stream, total_rows = rows of those arrays.  This is how episodes of a sequential 1-env loop that may end
 * early (the "Test" envs) run as parallel streams: the host guesses every episode's position in the loop (its start row = the
 * steps taken before it, which is also its position in the env's random stream, env->step_count), runs all of them, and
 * repeats with the positions the measured lengths imply until they agree; rows are then exactly the sequential loop's. */
int icrl_sample_episodes(const icrl_env_t* env, const icrl_norm_t* nm, const icrl_policy_t* pol, const float* noise,
                         const float* action_low, const float* action_high, int episodes_per_stream, int rows_per_stream,
                         int deterministic, int do_reset, const int32_t* stream_row0, int total_rows, double* orig_obs,
                         double* obs, float* actions, double* ep_rewards, int32_t* ep_lengths, void* stream);

/* ConstraintNet.cost_function (icrl/constraint_net.py:121-130): cost[n] = 1 - zeta(prepare(obs[n], acs[n])).
 * obs [N,obs] float64, acs [N,acs] float32 (class index in acs[n,0] when discrete).  With an icrl_cost_disc_t behind `cn`:
 * cost[n] = zeta, what icrl_disc_reward(cn->net, ..., apply_log = 0) stores. */
int icrl_cost_mlp_forward(const icrl_costnet_t* cn, const double* obs, const float* acs, int N, float* cost, void* stream);

/* An analytic cost on N rows: cost[n] = f(obs[n], acs[n]), one row per thread.  obs [N, obs_dim] float64, acs [N, acs_dim] float32
 * ([N, 1] class index for ACTION_EQUALS); either may be NULL for a kind that does not read it.  icrl_cost_mlp_forward with an analytic
 * descriptor forwards here. */
int icrl_cost_fn_rows(const icrl_cost_fn_t* cf, const double* obs, const float* acs, int N, float* cost, void* stream);

/* A region cost on N rows, the twin of icrl_cost_fn_rows: cost[n] = f(obs[n], acs[n]).  obs [N, obs_dim] float64, acs [N, acs_dim]
 * float32 ([N, 1] class index beside a discrete policy); either may be NULL when no clause reads it.  icrl_cost_mlp_forward with a
 * region descriptor forwards here. */
int icrl_cost_region_rows(const icrl_cost_region_t* cf, const double* obs, const float* acs, int N, float* cost, void* stream);

/* GailDiscriminator.reward_function (icrl/gail_utils.py:147-157): the same network read the other way round — the
 * discriminator output D = sigmoid(MLP(prepare(obs, acs))) itself (apply_log = 0) or log(D + eps) (apply_log = 1, the
 * GAIL-constraint baseline's reward, eps = cn->eps).  out: [N] float32. */
int icrl_disc_reward(const icrl_costnet_t* cn, const double* obs, const float* acs, int N, float* out, int apply_log,
                     void* stream);

/* SynthVecEnv.reset / .step: the batched stand-in for SubprocVecEnv.step_async/step_wait.  step: actions [N,act] float32
 * (already clipped), writes raw reward [N] float64 and done [N] bytes, advances env->s in place (auto-reset). */
int icrl_synth_env_reset(const icrl_env_t* env, void* stream);
int icrl_synth_env_step(const icrl_env_t* env, const float* actions, double* raw_rew, uint8_t* dones, void* stream);

/* VecNormalizeWithCost.reset (vec_normalize.py:148-157,270-278): zero ret / cost_ret, feed a zero batch into ret_rms /
 * cost_rms when training, write normalize_obs(raw_obs) to obs_out [N,obs] float64. */
int icrl_vecnorm_reset(const icrl_norm_t* nm, const double* raw_obs, int N, int obs_dim, double* obs_out, void* stream);

/* VecNormalizeWithCost.step_wait after the env + cost wrapper (vec_normalize.py:81-100,220-243): running-moment merge
 * (obs, discounted reward return, discounted cost return), normalise + clip, zero the returns of finished envs.
 * raw_cost may be NULL (env stack without cost wrapper).  Outputs float64 [N,obs] / [N] / [N] (cost_out may be NULL). */
int icrl_vecnorm_step(const icrl_norm_t* nm, const double* raw_obs, const double* raw_rew, const float* raw_cost,
                      const uint8_t* dones, int N, int obs_dim, double* obs_out, double* rew_out, double* cost_out,
                      void* stream);

/* OnPolicyWithCostAlgorithm.collect_rollouts (common/on_policy_algorithm.py:340-421) fused on the device: T steps of
 * {policy forward -> clip -> env step -> cost_function(previous raw obs, action) -> VecNormalizeWithCost -> buffer.add},
 * then the dual GAE.  noise: [T,N,act] standard normals.  ONE persistent launch for all T steps where the shape allows
 * (see icrl_rollout_collect_ex: <= 128 envs one workgroup per env with replicated statistics, up to 1024 envs 4 envs per
 * workgroup with the float64 statistics partitioned by observation column), otherwise 2 launches per step; + 1 launch for
 * GAE; no host sync. */
int icrl_rollout_collect(const icrl_env_t* env, const icrl_norm_t* nm, const icrl_policy_t* pol, const icrl_costnet_t* cn,
                         const icrl_buffer_t* buf, const icrl_agent_t* ag, const float* noise,
                         const float* action_low, const float* action_high,
                         double reward_gamma, double reward_gae_lambda, double cost_gamma, double cost_gae_lambda,
                         void* stream);

/* PPOLagrangian.train (stable_baselines3/ppo_lag/ppo_lag.py:196-299) as ONE persistent launch: for every epoch, for every
 * minibatch of the permutation: gather (buffers.py:594-627, env-major flat index i -> env = i / T, t = i % T),
 * evaluate_actions (policies.py:752-767), advantage normalisation / centring, clipped surrogate + nu * cost term, two value
 * MSEs, entropy, backward, global-norm clip (max_grad_norm), Adam, approx-KL early stop after a full epoch.
 * Three workgroups (policy | reward critic | cost critic — the three MLPs are independent) keep their weights in LDS and
 * their Adam moments in registers; the only coupling per step is the squared gradient norm (3 floats, 8-byte granules).
 *   exp_avg / exp_avg_sq: [n_params] Adam moments (policy.optimizer state), adam_step: [1] int32 step counter (device);
 *   perms: [n_epochs, T*N] int32 permutations;  nu: [1] current Lagrange multiplier (device);
 *   stats: [32 + n_epochs] float32 (device): 0 early_stop_epoch, 1 optimiser steps done, 2..6 sums over minibatches of
 *          entropy_loss / policy_loss / reward_value_loss / cost_value_loss / clip_fraction, 7 mean approx_kl of the last
 *          epoch, 8..10 last minibatch's policy+entropy / reward-value / cost-value loss terms, 11 status (0 ok),
 *          32+e mean approx_kl of epoch e;
 *   sync_ws: >= ICRL_PPO_SYNC_BYTES(n_epochs, ceil(T*N / batch_size), T*N) bytes of device scratch: the inter-workgroup granules
 *            (zeroed by the call) + the schedule tables the call fills (per optimiser step: minibatch rows, Adam bias
 *            corrections; per 64-row chunk: permutation offset; the permutations mapped to storage offsets).
 *   hp->_pad: bit 0 = write per-phase cycle counts to stats[12..31] (diagnostic); kernel selection (default: wave pairs, two
 *            waves per SIMD; obs > 64: row-owning waves): bit 2 = row-owning waves (one wave per SIMD), bit 1 = the column-split
 *            tiles kernel; the row-owning kernel runs TWO workgroups per network when batch_size > 64 (each computes one 64-row
 *            chunk of a minibatch, partial gradients exchanged as granules) unless bit 3 is set.  obs <= 32 (HCWithPos, LapGridWorld): the
 *            wave-quad kernel — FOUR workgroups per network (12 per run on one XCD; 16 rows of every 64-row chunk each, the four partial
 *            gradients summed as (q0 + q1) + (q2 + q3) by all four; round 6), TWO with bit 5 (32 rows each; also what batches of 17..40
 *            runs get), the wave-pair kernel (one) with bit 4.  obs 65..128 (AntWall), single-run calls: FOUR workgroups per network as well
 *            (wave quads with the row-owning kernel's parameter ownership; minibatches of 65..128 rows take both 64-row chunks in one pass);
 *            bit 2 or bit 5 keep the row-owning kernel there.  Bit 0 selects separate instantiations of the kernels (the timers cost every
 *            launch ~2.5 % as a run-time flag).  Bit 6 (tests): the last workgroup of a four-workgroups-per-network launch leaves at once —
 *            the others' bounded waits must end the launch with stats[11] set.
 * Shapes outside the persistent kernels — a policy stored with hidden width h1 = h2 > 64 (a multiple of 64 up to 256: the reference's
 * -pl / -rvl / -cvl flags take any width, icrl/utils.py:636-655), a policy described by `arch` (shared trunk, other depths) or
 * batch_size > 256 (buffers.py:594-612 slices any size) — run through the generic-shape path (csrc/generic.hip): ONE persistent
 * cooperative launch on one XCD (up to 512-row batches, 131 072 parameters, rows that fit the LDS; otherwise three plain launches per
 * optimiser step), same statistics layout, of hp->_pad only bit 0 (phase timers in stats[12..28]) and bit 6 (tests: one workgroup leaves, the bounded waits must end the launch with stats[11] set); sync_ws must then hold ICRL_PPO_SYNC_BYTES(...) +
 * ICRL_PPO_GENERIC_BYTES(batch_size, icrl_ppo_generic_row_floats(pol), n_params) bytes. */
int icrl_ppo_lag_train(const icrl_policy_t* pol, float* exp_avg, float* exp_avg_sq, int32_t* adam_step,
                       const icrl_buffer_t* buf, const int32_t* perms, const float* nu, const icrl_ppo_hyper_t* hp,
                       float* stats, void* sync_ws, void* stream);
/* icrl_ppo_lag_train with the minibatches gathered BEFORE the persistent launch (csrc/ppo_stream.hip): the permutations of all epochs
 * are known up front, so two plain launches over the whole device write every minibatch, in step order, as one contiguous record per
 * 16-row tile ([obs_dim + act_store + 7][16 rows] floats: observations, stored actions, old log-prob, reward / cost advantage, old
 * reward value, reward return, old cost value, cost return; rows beyond a ragged chunk repeat the chunk's first row) and a table of
 * {mean, 1 / (std + 1e-8), cost mean} of the advantages per optimiser step; the step loop then reads records instead of carrying an
 * index pipeline, scattered 4-byte gathers and the statistics on every dependent step.  Same values, same order of every sum: results
 * are bit-identical to icrl_ppo_lag_train.
 *   icrl_ppo_stream_ws_bytes: bytes of records + table for this call (host arithmetic, no launch); 0 with the reason in icrl_last_error()
 *     where the stream does not serve the call.  Served: what runs as a single-run wave-quad launch (obs_dim <= 32, hidden 64 x 64 without
 *     `arch`, batch_size 2..256, no kernel override in hp->_pad bits 1, 2, 4) whose records stay below 4 GiB.
 *   icrl_ppo_lag_train_stream: with stream_ws (device, 256-byte aligned, any contents) of at least that many bytes and a served call, the
 *     pre-pass on `stream` followed by the STREAM instantiation of the wave-quad kernel; otherwise (NULL, too small, not served) exactly
 *     icrl_ppo_lag_train — same kernels, same results.  Word [4] of the update family's route record says which. */
size_t icrl_ppo_stream_ws_bytes(const icrl_policy_t* pol, const icrl_buffer_t* buf, const icrl_ppo_hyper_t* hp);
int icrl_ppo_lag_train_stream(const icrl_policy_t* pol, float* exp_avg, float* exp_avg_sq, int32_t* adam_step,
                              const icrl_buffer_t* buf, const int32_t* perms, const float* nu, const icrl_ppo_hyper_t* hp,
                              float* stats, void* sync_ws, void* stream_ws, long long stream_ws_bytes, void* stream);
/* the `row_floats` argument of ICRL_PPO_GENERIC_BYTES for this policy (host arithmetic, no launch), or -1 with the reason in
 * icrl_last_error() when the generic-shape path does not serve its architecture */
int icrl_ppo_generic_row_floats(const icrl_policy_t* pol);

/* ------------------------------------------------------------------------------------------------------------------
 * Batched forms: several INDEPENDENT runs (seeds) of identical shape in ONE launch, run = blockIdx.y
 * ------------------------------------------------------------------------------------------------------------------
 * One run of BASELINE configs[1] occupies 3 CUs during its update and 64 during a rollout; the reference runs seeds as separate
 * processes (README.md:14-21, one `python run_me.py` per seed).  Here n_runs runs share one grid: every *_batch entry point takes
 * an array of n_runs job descriptors in HOST memory (same fields as the arguments of the single-run entry point it mirrors),
 * requires all runs to agree in every shape that decides the grid (refused otherwise), and computes for each run exactly what
 * the single-run call computes with the same kernel (bit-identical: tests/test_seed_batch_gpu.py, tests/test_routes_gpu.py).  The
 * rollout and GAE kernels all agree bit for bit, so there the kernel does not matter.  The update does not: up to 16 runs of obs <= 32
 * get the kernel a run alone gets (wave quads, four workgroups per network); 17..40 runs its two-workgroup form and more than 40 the
 * wave-pair kernel (hp._pad bits 5 / 4 on a single run), which sum partial gradients in another order.  The contract for more than 16
 * runs is therefore: bit-identical to the single-run call with that hp._pad bit, within the update's bound against the oracle, and
 * NOT promised bit-identical to the default single-run call (observed at 4 envs x 8 steps, minibatches of 16: the two-workgroup form
 * happened to equal it, the wave-pair kernel differed; an observation at one shape, not a guarantee).  icrl_debug_last_route says which
 * kernel a call took.
 *   args_ws: device scratch of >= n_runs * ICRL_BATCH_ARGS_BYTES bytes, any contents; it receives the per-run argument blocks
 *            (written on `stream` before the launch) and must not be reused by another call before this one has completed. */
#define ICRL_BATCH_ARGS_BYTES 1024

/* icrl_rollout_collect_ex for n_runs runs: ONE persistent launch + ONE batched dual-GAE launch (do_gae bit 0).  Two batched forms, in
 * the order the comment above icrl_rollout_collect_ex_mon in csrc/rollout_collect.hip states: the multi-env kernel (several envs per workgroup) and
 * the one-workgroup-per-env kernel, grid (n_envs, n_runs) (n_envs <= 128, n_envs x obs_dim <= 4096: BASELINE configs[1]); every run
 * needs its exchange workspace (icrl_agent_t.xch_ws) or T * N * 4 >= ICRL_ROLLOUT_WS_BYTES.
 * args_ws: 2 x n_runs x ICRL_BATCH_ARGS_BYTES (rollout + GAE argument blocks). */
typedef struct {
  const icrl_env_t* env;
  const icrl_norm_t* nm;
  const icrl_policy_t* pol;
  const icrl_costnet_t* cn;     /* NULL in every run or in none */
  const icrl_buffer_t* buf;
  const icrl_agent_t* ag;
  const float* noise;           /* [T, N, act] */
} icrl_rollout_job_t;
int icrl_rollout_collect_batch(int n_runs, const icrl_rollout_job_t* jobs, const float* action_low, const float* action_high,
                               double reward_gamma, double reward_gae_lambda, double cost_gamma, double cost_gae_lambda,
                               int do_gae, void* args_ws, long long args_ws_bytes, void* stream);

/* the same with one icrl_monitor_t per run (`mons`: n_runs descriptors in host memory, or NULL = icrl_rollout_collect_batch) */
int icrl_rollout_collect_batch_mon(int n_runs, const icrl_rollout_job_t* jobs, const icrl_monitor_t* mons, const float* action_low,
                                   const float* action_high, double reward_gamma, double reward_gae_lambda, double cost_gamma,
                                   double cost_gae_lambda, int do_gae, void* args_ws, long long args_ws_bytes, void* stream);

/* the batched rollout of runs against a FIXED cost (cpg seed batches).  Behind jobs[r].cn one of: a constraint net in every run,
 * NULL in every run (both: exactly icrl_rollout_collect_batch_mon, `mons` may be NULL), or an analytic descriptor (icrl_cost_fn_t,
 * n_hidden == ICRL_COST_FN) in every run — each run's descriptor travels in its own argument block and is read once before the step
 * loop, so the runs of a batch may differ in its kind, index and thresholds; grids and shapes are shared.  Every descriptor passes
 * the checks of icrl_rollout_collect_ex; a batch that mixes analytic runs with constraint-net (or cost-free) runs is refused, all of
 * it on the host before the first device call.  Kernel forms, shapes and the "no batched form for this shape" refusal are those of
 * icrl_rollout_collect_batch_mon. */
int icrl_rollout_collect_batch_cost(int n_runs, const icrl_rollout_job_t* jobs, const icrl_monitor_t* mons /* may be NULL */,
                                    const float* action_low, const float* action_high, double reward_gamma, double reward_gae_lambda,
                                    double cost_gamma, double cost_gae_lambda, int do_gae, void* args_ws, long long args_ws_bytes,
                                    void* stream);

/* icrl_gae_dual_ws for n_runs [T,N] rollouts of one shape: ONE launch of the two-level scan, grid (tiles * C, n_runs), every run
 * with its own workspace; shapes the split scan does not serve are issued as n_runs single launches. */
typedef struct {
  const float *rewards, *costs, *reward_values, *cost_values, *dones, *last_v_r, *last_v_c;
  const uint8_t* last_dones;
  float *adv_r, *adv_c, *ret_r, *ret_c;
  void* ws;
  long long ws_bytes;
} icrl_gae_job_t;
int icrl_gae_dual_batch(int n_runs, const icrl_gae_job_t* jobs, int T, int N, double reward_gamma, double reward_gae_lambda,
                        double cost_gamma, double cost_gae_lambda, void* args_ws, long long args_ws_bytes, void* stream);

/* icrl_sample_episodes for n_runs runs: grid (n_streams, n_runs); every run has its own env streams, frozen normaliser, policy,
 * noise and outputs; the shape arguments are common. */
typedef struct {
  const icrl_env_t* env;
  const icrl_norm_t* nm;
  const icrl_policy_t* pol;
  const float* noise;
  const int32_t* stream_row0;   /* or NULL (see icrl_sample_episodes) */
  int32_t total_rows, _pad;
  double *orig_obs, *obs;
  float* actions;
  double* ep_rewards;
  int32_t* ep_lengths;
} icrl_sample_job_t;
int icrl_sample_episodes_batch(int n_runs, const icrl_sample_job_t* jobs, const float* action_low, const float* action_high,
                               int episodes_per_stream, int rows_per_stream, int deterministic, int do_reset,
                               void* args_ws, long long args_ws_bytes, void* stream);

/* The episodes of sequential 1-env loops in ONE launch, their positions settled inside it (csrc/rollout.hip ChainArgs, DESIGN.md
 * section 11): job j = env->n_envs episodes of one loop, stream k = episode k, one episode per stream; grid (largest stream count, n_jobs).
 * Computes what icrl_sample_episodes computes with ONE stream running the job's episodes back to back — rows, episode sums and lengths,
 * and in env->s / t_ep / step_count of the LAST stream the state that loop ends in — also when episodes end early: a stream starts from
 * the guess k * max_steps, learns its true start row from its predecessor while both run, starts over when the two differ, and copies
 * its rows to their place once that start is final.  Jobs may differ in env flags, statistics, policy, noise and stream count.
 *   env: per-stream state arrays [n_streams] (s, t_ep, key as for icrl_sample_episodes; step_count is written, not read);
 *   base_count: [1] int32 on the device, the loop's env->step_count before episode 0; noise / outputs: [n_streams * max_steps, ..] rows;
 *   fixed_len: episodes always run max_steps (the guesses are exact: no polling, no copy); exec_steps: [n_streams] env steps every
 *   stream executed including abandoned runs, or NULL.  do_reset: episode 0 starts from a reset (else from env->s[0], t_ep[0]).
 *   ws: >= icrl_sample_episodes_chain_ws_bytes(n_jobs, jobs) bytes of device scratch, any contents; its first word is 0 afterwards unless
 *   a stream gave up waiting for its predecessor (its ep_lengths entry is then -1).  args_ws: n_jobs * ICRL_BATCH_ARGS_BYTES.
 * Refused (hipErrorInvalidValue, reason starting "icrl_sample_episodes_chain: refused:"; callers take the multi-pass path): more
 * streams in total than the device has compute units, a generic-shape policy, episodes_per_stream != 1, observation widths on both
 * sides of 32 in one launch. */
typedef struct {
  const icrl_env_t* env;
  const icrl_norm_t* nm;
  const icrl_policy_t* pol;
  const float* noise;           /* or NULL (mode of the distribution) */
  const int32_t* base_count;
  int32_t episodes_per_stream, deterministic, fixed_len, _pad;
  double *orig_obs, *obs;
  float* actions;
  double* ep_rewards;
  int32_t* ep_lengths;
  int32_t* exec_steps;
} icrl_chain_job_t;
size_t icrl_sample_episodes_chain_ws_bytes(int n_jobs, const icrl_chain_job_t* jobs);
int icrl_sample_episodes_chain(int n_jobs, const icrl_chain_job_t* jobs, const float* action_low, const float* action_high, int do_reset,
                               void* ws, long long ws_bytes, void* args_ws, long long args_ws_bytes, void* stream);

/* icrl_cn_train (full-batch mode) for n_runs constraint nets of one architecture: the four launches of an iteration carry all runs
 * (grid.y = run; row counts may differ between runs: grids are sized for the largest, iteration counts likewise). */
typedef struct {
  const icrl_costnet_t* cn;
  float *exp_avg, *exp_avg_sq;
  int32_t* adam_step;
  const float *nominal, *expert;
  int32_t Nn, Ne;
  const int32_t *ep_offsets, *row_episode;
  int32_t n_ep, _pad;
  const icrl_cn_hyper_t* hp;
  float *work, *metrics;
} icrl_cn_train_job_t;
int icrl_cn_train_batch(int n_runs, const icrl_cn_train_job_t* jobs, void* args_ws, long long args_ws_bytes, void* stream);

/* icrl_ppo_lag_train for n_runs runs: 3 | 6 persistent workgroups per run in one grid (layout: "XCD placement" at the top). */
typedef struct {
  const icrl_policy_t* pol;
  float *exp_avg, *exp_avg_sq;
  int32_t* adam_step;
  const icrl_buffer_t* buf;
  const int32_t* perms;
  const float* nu;
  const icrl_ppo_hyper_t* hp;
  float* stats;
  void* sync_ws;
} icrl_ppo_train_job_t;
int icrl_ppo_lag_train_batch(int n_runs, const icrl_ppo_train_job_t* jobs, void* args_ws, long long args_ws_bytes, void* stream);

/* ConstraintNet.prepare_data (icrl/constraint_net.py:258-270): out[n,:] = float32(concat(clip(normalise(obs)), clip(one-hot?
 * acs))[select_dim]).  obs [N,obs] float64, acs [N,acs] float32 (class index when discrete), out [N,in_dim] float32. */
int icrl_cn_prepare(const icrl_costnet_t* cn, const double* obs, const float* acs, int N, float* out, void* stream);

/* ConstraintNet.train after prepare_data (icrl/constraint_net.py:155-229) for the default full-batch mode
 * (batch_size None): per iteration {forward of all nominal + expert rows, compute_is_weights (:231-256: per-episode float32
 * products, KL(old||new), KL(new||old), per-step or per-episode weights incl. the [B,1,1]x[B,1] broadcast of the per-step
 * mode), early-stop test, loss (likelihood-ratio or BCE "gail" form), backward, Adam}.  4 launches per iteration, no host
 * sync; iterations after an early stop are no-ops.
 *   nominal [Nn,in_dim], expert [Ne,in_dim] float32;  ep_offsets [n_ep+1] int32 row offsets of the nominal episodes;
 *   row_episode [Nn] int32;  exp_avg / exp_avg_sq [n_params], adam_step [1] int32 (device): optimiser state;
 *   work: device scratch of icrl_cn_train_work_floats(...) floats;
 *   metrics [iterations][ICRL_CN_METRICS] float32 (device), per iteration i (values of the forward pass made at the START of
 *   iteration i): 0 stop flag, 1 kl_old_new, 2 kl_new_old, 3 is_mean, 4 is_max, 5 is_min, 6 cn_loss, 7 expert_loss,
 *   8 unweighted_nominal_loss, 9 nominal_loss, 10 regularizer_loss, 11..13 nominal preds max/min/mean, 14..16 expert preds
 *   max/min/mean, 17 executed (1 if the optimiser step of this iteration ran). */
size_t icrl_cn_train_work_floats(int n_params, int Nn, int Ne, int n_ep);
int icrl_cn_train(const icrl_costnet_t* cn, float* exp_avg, float* exp_avg_sq, int32_t* adam_step,
                  const float* nominal, const float* expert, int Nn, int Ne,
                  const int32_t* ep_offsets, const int32_t* row_episode, int n_ep,
                  const icrl_cn_hyper_t* hp, float* work, float* metrics, void* stream);

/* Diagnostic: which kernels the calling host thread's last call of a fused family launched.  The entry points below choose among several
 * launch forms by shape, workspace and device (the single statement of the rollout's order is the comment above
 * icrl_rollout_collect_ex_mon in csrc/rollout_collect.hip; prepare_train in csrc/ppo_train.hip and icrl_gae_dual_ws in csrc/gae.hip for the
 * other two) and step to the next form silently; this says which one ran.  Host state only, thread-local like icrl_last_error():
 * a call clears its family's record on entry and writes it behind its launch, so a call refused before any launch leaves route 0.
 * out8 receives 8 int32 (unused words 0).  Returns 0; a family outside 0..2 or a NULL out8 is refused with a message.
 *   ICRL_FAMILY_ROLLOUT  icrl_rollout_collect[_ex][_mon], icrl_rollout_collect_sde and icrl_rollout_collect_batch[_mon | _cost]:
 *     [0] ICRL_ROUTE_*   [1] ICRL_WS_* (a batch: of its last run)   [2] working workgroups per run   [3] envs per workgroup (0: per-step)
 *     [4] ICRL_PICK_* bits of the instantiation, the batched one-workgroup-per-env kernel's MINW at ICRL_PICK_MINW_SHIFT
 *     [5] packed XCD layout (multi kernels)   [6] n_runs   [7] launches of the rollout proper, the GAE excluded: 1, 2 T (per-step),
 *     4 T (generic per-step with a constraint net; 3 T without one)
 *   ICRL_FAMILY_UPDATE   icrl_ppo_lag_train[_batch]:
 *     [0] 0..7 as prepare_train names them (0 wave pairs, 1 row-owning waves, 2 the same with two workgroups per network, 3 column-split
 *         tiles, 4 wave quads with two workgroups per network, 5 with four, 6 / 7 four workgroups per network at obs 65..128),
 *         ICRL_UPDATE_GENERIC_PERSISTENT, ICRL_UPDATE_GENERIC_LAUNCHES
 *     [1] workgroups per network (ICRL_UPDATE_GENERIC_PERSISTENT: of the whole grid)   [2] n_runs   [3] 1 packed XCD grid | 0 run-major
 *     [4] 1 the step loop read the pre-gathered minibatch stream (icrl_ppo_lag_train_stream) | 0 it gathered its rows itself
 *   ICRL_FAMILY_GAE     icrl_gae_dual[_ex | _ws | _batch] (a rollout with do_gae bit 0 ends in one of them):
 *     [0] ICRL_GAE_*   [1] the sequential kernel's shape code (4, 16, 101, 105..112), else the workgroups per tile C   [2] column tiles
 *     [3] n_runs */
#define ICRL_FAMILY_ROLLOUT 0
#define ICRL_FAMILY_UPDATE 1
#define ICRL_FAMILY_GAE 2
#define ICRL_N_FAMILIES 3
#define ICRL_ROUTE_NONE 0
#define ICRL_ROUTE_PER_STEP 1
#define ICRL_ROUTE_PERSISTENT 2
#define ICRL_ROUTE_WIDE 3
#define ICRL_ROUTE_MULTI 4
#define ICRL_ROUTE_GENERIC_PERSISTENT 5
#define ICRL_ROUTE_GENERIC_PER_STEP 6
#define ICRL_ROUTE_PERSISTENT_BATCH 7
#define ICRL_ROUTE_MULTI_BATCH 8
#define ICRL_WS_NONE 0
#define ICRL_WS_XCH 1     /* icrl_agent_t.xch_ws */
#define ICRL_WS_PLANE 2   /* the buffer's reward_advantages plane */
#define ICRL_PICK_SMALL 1
#define ICRL_PICK_ANALYTIC 2
#define ICRL_PICK_MON 4
#define ICRL_PICK_GRAN 8
#define ICRL_PICK_CN128 16
#define ICRL_PICK_DISC 32     /* the constraint net read as D (icrl_cost_disc_t) */
#define ICRL_PICK_SDE 64      /* the kernels with the gSDE head (icrl_rollout_collect_sde) */
#define ICRL_PICK_REGION 128  /* the kernels whose cost wave evaluates a region cost (icrl_cost_region_t) */
#define ICRL_PICK_MINW_SHIFT 8
#define ICRL_UPDATE_GENERIC_PERSISTENT 8
#define ICRL_UPDATE_GENERIC_LAUNCHES 9
#define ICRL_GAE_SEQUENTIAL 1
#define ICRL_GAE_SPLIT 2            /* two-pass split scan */
#define ICRL_GAE_REGSPLIT 3         /* register-resident split scan */
#define ICRL_GAE_BATCH_SPLIT 4
#define ICRL_GAE_BATCH_REGSPLIT 5
#define ICRL_GAE_BATCH_SINGLES 6    /* a batch issued as n_runs single launches */
int icrl_debug_last_route(int family, int32_t* out8);

/* Diagnostic: cycles per phase of workgroup 0 of the last persistent rollout that ran with do_gae bit 2 set
 * (out8: policy+env, barrier, tail, steps, exchange load, statistics, normalise, 0). */
int icrl_debug_rollout_profile(unsigned long long* out8);
/* the same for the many-environment persistent kernel: 5 phase sums + T of wave 0 ([0..7]) and of the owner wave ([8..15]) of
 * workgroup 0 (do_gae bit 2) or of the last workgroup, which owns no statistic (do_gae bit 3). */
int icrl_debug_rollout_profile_wide(unsigned long long* out16);
/* per workgroup of that kernel, step T/2 of a profiled launch: 100 MHz timestamps at the end of its env phase, of its owner's
 * gather, of its owner's publish (0 when it owns no statistic) and when it had read all statistics: out[4 * n_workgroups]. */
int icrl_debug_rollout_trace_wide(unsigned long long* out, int n_workgroups);

/* ------------------------------------------------------------------------------------------------------------------
 * Fine-grained pieces of the update, for a host that keeps its MLPs in torch (csrc/fine.hip)
 * ------------------------------------------------------------------------------------------------------------------
 * icrl_ppo_lag_train runs the whole of PPOLagrangian.train() in one launch.  A maintainer who keeps `policy.evaluate_actions` and
 * autograd in torch can bind these instead, one call site at a time (INTEGRATION.md section 5 shows the loop):
 *   rollout_buffer.get(batch_size)         stable_baselines3/common/buffers.py:594-627  -> icrl_minibatch_gather
 *   advantage normalisation                ppo_lag/ppo_lag.py:219-222                   -> icrl_adv_stats
 *   loss terms + their gradients           ppo_lag/ppo_lag.py:224-281                   -> icrl_ppo_lag_loss_fwd_bwd
 *   clip_grad_norm_ + optimizer.step()     ppo_lag/ppo_lag.py:283-288                   -> icrl_clip_adam_step
 *   dual.update_parameter(average_cost)    common/dual_variable.py:47-57                -> icrl_dual_step
 *   rollout_buffer.add(...)                common/buffers.py:554-592                    -> icrl_buffer_add
 *   compute_is_weights / the cn loss       icrl/constraint_net.py:231-256, 188-202      -> icrl_is_weights, icrl_cn_loss_fwd_bwd
 * and, for a host that keeps no torch network at all (csrc/mlp_grad.hip; icrl_amd/torch_ops.py wraps them as autograd functions):
 *   policy.evaluate_actions + autograd     common/policies.py:752-767                   -> icrl_policy_fwd_bwd
 *   constraint_net.forward + autograd      icrl/constraint_net.py:101-130               -> icrl_cost_mlp_fwd_bwd
 * Launch-bound by construction (a minibatch is 64..512 rows); the fused persistent kernels are the fast path. */

/* flat_idx[n]: env-major indices (i = env * T + t, buffers.py:53-65) -> the rows of the [T, N] buffer: obs [n, obs_dim], actions
 * [n, act_store], and per-row scalars [n]; any output but obs may be NULL. */
int icrl_minibatch_gather(const icrl_buffer_t* buf, const int32_t* flat_idx, int n, float* obs, float* actions, float* old_log_prob,
                          float* adv_r, float* adv_c, float* ret_r, float* ret_c, float* old_v_r, float* old_v_c, void* stream);
/* out4 = {mean(adv_r), 1 / (std(adv_r) + 1e-8) with torch's unbiased std, mean(adv_c), std(adv_r)}; n >= 2. */
int icrl_adv_stats(const float* adv_r, const float* adv_c, int n, float* out4, void* stream);
/* common/utils.py:43-59 `explained_variance(y_pred, y_true)` = 1 - Var[y_true - y_pred] / Var[y_true] (NaN when Var[y_true] == 0), float64
 * over n float32 values, the mean subtracted first as np.var does (a nearly constant critic does not cancel; NaN exactly when y_true is
 * constant, for n < 2^29: up to there the sum of n equal float32 values is exact in float64), for one or two pairs in one call (the second pair may be NULL as a whole; then out2[1] is not written).
 * Call site replaced: ppo_lag/ppo_lag.py:311-312 — NB the reference passes (returns, values), i.e. y_pred = returns, y_true = values.
 * work: 8 x 256 doubles of device scratch; out2: device float32. */
int icrl_explained_variance(const float* y_pred_a, const float* y_true_a, const float* y_pred_b, const float* y_true_b, long long n,
                            double* work, float* out2, void* stream);
/* The PPO-Lagrangian loss of ONE minibatch on the networks' outputs (all [n] float32; adv_r / adv_c RAW: they are normalised /
 * centred inside as ppo_lag.py:219-222 does): terms8 = {loss, policy_loss, reward_value_loss, cost_value_loss, entropy_loss,
 * approx_kl, clip_fraction, 0}; d_log_prob / d_v_r / d_v_c / d_entropy = d loss / d that output, what loss.backward() would send
 * into `log_prob.backward(...)` etc.  old_v_r / old_v_c NULL: no value clipping; entropy NULL: the reference's -mean(-log_prob)
 * estimate (its gradient then goes into d_log_prob; d_entropy is not written).  nu: device pointer.  2 <= n <= 65536. */
int icrl_ppo_lag_loss_fwd_bwd(const float* log_prob, const float* old_log_prob, const float* adv_r, const float* adv_c, const float* v_r,
                              const float* v_c, const float* ret_r, const float* ret_c, const float* old_v_r, const float* old_v_c,
                              const float* entropy, const float* nu, const icrl_ppo_hyper_t* hp, int n, float* terms8, float* d_log_prob,
                              float* d_v_r, float* d_v_c, float* d_entropy, void* stream);
/* torch.nn.utils.clip_grad_norm_(max_grad_norm) followed by torch.optim.Adam.step() on ONE flat parameter buffer (hp: lr, betas, eps,
 * max_grad_norm; bias corrections in double from *adam_step + 1, which is then incremented on the device).  work: 256 floats of
 * scratch; out2 (may be NULL) = {total norm, clip coefficient}. */
int icrl_clip_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int32_t* adam_step, long long n,
                        const icrl_ppo_hyper_t* hp, float* work, float* out2, void* stream);
/* DualVariable.update_parameter on the device: state4 = {log_nu, exp_avg, exp_avg_sq, nu} (nu = softplus(log_nu) is rewritten, so
 * state4 + 3 can be the `nu` argument of the update), *adam_step its Adam step count; cost from cost_dev[0] when not NULL, else
 * cost_host; clamp_log_nu = the clamp floor in log_nu space (the reference's double inverse softplus, dual_variable.py:19-29);
 * loss_out (may be NULL) = -nu * (cost - budget). */
int icrl_dual_step(float* state4, int32_t* adam_step, const float* cost_dev, float cost_host, float budget, float learning_rate,
                   float clamp_log_nu, float* loss_out, void* stream);

/* RolloutBufferWithCost.add (stable_baselines3/common/buffers.py:554-592): one step's arrays of all N envs (observations float64
 * [N, obs_dim] x 4, action float32 [N, act_store], reward / cost float64 [N], the rest float32 / uint8 [N]) -> row t of the buffer. */
int icrl_buffer_add(const icrl_buffer_t* buf, int t, const double* obs, const double* orig_obs, const double* new_obs, const double* new_orig_obs,
                    const float* action, const double* reward, const double* cost, const float* orig_cost, const uint8_t* done,
                    const float* reward_value, const float* cost_value, const float* log_prob, void* stream);
/* ConstraintNet.compute_is_weights (icrl/constraint_net.py:231-256): preds_old / preds_new [N] = zeta of the start-of-call and of the current
 * network on the nominal rows, episodes = rows ep_offsets[e] .. ep_offsets[e + 1] (n_ep + 1 offsets); weights [N] per step (ratio / mean
 * ratio) or per episode (repeated over its rows); ep_prod [n_ep] scratch / output (float32 products, overflowing like the reference's);
 * out4 = {kl_old_new, kl_new_old, mean ratio, sum of the products}. */
int icrl_is_weights(const float* preds_old, const float* preds_new, int N, const int32_t* ep_offsets, int n_ep, float eps, int per_step,
                    float* weights, float* ep_prod, float* out4, void* stream);
/* The constraint-net loss of one (mini)batch on the network's outputs (icrl/constraint_net.py:188-202): terms6 = {loss, expert_loss,
 * nominal_loss, regularizer, mean(log(nominal + eps)), 0}; d_nominal / d_expert = d loss / d prediction (for preds.backward(...)).
 * is_weights NULL: ones.  mode bit 0: the GAIL discriminator's BCE (gail_utils.py); bit 1: the per-step broadcast quirk of the
 * reference (nominal_loss = mean(w) * mean(log zeta)). */
int icrl_cn_loss_fwd_bwd(const float* nominal_preds, const float* expert_preds, const float* is_weights, int Bn, int Be, float reg_coeff, float eps,
                         int mode, float* terms6, float* d_nominal, float* d_expert, void* stream);

/* Forward and backward of the policy's three networks for ARBITRARY upstream gradients (csrc/mlp_grad.hip).  Outputs as
 * ActorTwoCriticsPolicy.evaluate_actions (common/policies.py:752-767) on obs [N, obs_dim] float32 (what icrl_minibatch_gather writes) and
 * actions [N, act_store]: v_r, v_c, log_prob, entropy [N] each, any may be NULL.  grad [n_params] is OVERWRITTEN with
 *   sum_n d_v_r[n] dv_r[n]/dθ + d_v_c[n] dv_c[n]/dθ + d_log_prob[n] dlog_prob[n]/dθ + d_entropy[n] dentropy[n]/dθ
 * in the layout of pol->params (log_std takes the log-prob and the entropy part; Categorical: the entropy goes through the logits; entries
 * of a zero-padded layer get exactly 0).  A NULL d_* stands for zeros; grad NULL (then every d_* NULL) = forward only, the same output bits.
 * Reads pol->params, never params_t: no icrl_policy_prepare is needed between optimiser steps.  The backward recomputes the forward.
 * Arithmetic in float64 on the float32 parameters and inputs: outputs and grad are the float64 values rounded once to float32.
 * Deterministic: row tiles of 16 are summed in a fixed order, at most 64 float64 partial sums in ws, added in index order by a second plain
 * launch; no atomics, no cooperative launch.  Served: arch == NULL, h1 == h2 <= 64, obs_dim <= 128, act_dim <= 16, 1 <= N <= 65536;
 * everything else, a NULL required pointer and a ws below icrl_policy_fwd_bwd_ws_bytes (needed with grad only; 0 + a reason for a
 * refused shape) return hipErrorInvalidValue with the reason, before any device call. */
size_t icrl_policy_fwd_bwd_ws_bytes(const icrl_policy_t* pol, int N);
int icrl_policy_fwd_bwd(const icrl_policy_t* pol, const float* obs, const float* actions, int N, const float* d_v_r, const float* d_v_c,
                        const float* d_log_prob, const float* d_entropy, float* v_r, float* v_c, float* log_prob, float* entropy, float* grad,
                        void* ws, long long ws_bytes, void* stream);
/* The gSDE forms of icrl_policy_forward and icrl_policy_fwd_bwd (csrc/sde.hip; stable_baselines3/common/distributions.py:408-601 with what
 * PPOLagrangian(use_sde=True) builds: full_std, exp, no squashing, learn_features = False).  A gSDE policy keeps the ordinary descriptor; its
 * buffer holds log_std as a MATRIX — logical [H, A] over the policy branch's last tanh layer (the latent), stored [64, A] with zero rows beyond
 * H, still the first tensor — and n_params = the diagonal layout's + 63 * act_dim says so: every other entry point that checks n_params refuses it.
 *   variance of action a = sum_h latent_h^2 exp(2 log_std[h][a]) + 1e-6, the latent units in ascending order, the latent DETACHED in it.
 * icrl_policy_forward_sde: obs [N, obs_dim] float64 -> actions = mean + latent . E (the mean when deterministic), their clip to
 * [action_low, action_high] (both NULL: act_clipped = actions), v_r, v_c, log_prob [N]; any output may be NULL.  expl: exploration matrices
 * [64, A] float32 row-major (zero rows beyond H are never read), row i's at expl + i * expl_stride: expl_stride = 64 * act_dim gives one matrix per
 * row, 0 one matrix for all rows; NULL with deterministic only.  One workgroup per row at every N; the three branch forwards are
 * icrl_policy_forward's own (below 64 rows), so mean, v_r and v_c carry its bits for the same network weights; the head is float64 on the
 * float32 latent, rounded once.  Reads params_t for the network: icrl_policy_prepare on the descriptor of the network alone — params and
 * params_t + 63 * act_dim, n_params - 63 * act_dim — leaves it there (ActorTwoCriticsPolicy.prepare does that).
 * icrl_policy_sde_fwd_bwd: the contract of icrl_policy_fwd_bwd word for word — float64 on float32 parameters rounded once, grad OVERWRITTEN in
 * the layout of pol->params (the [64, A] log_std block first, its padded rows exactly 0; log_std takes the variance part of log_prob and entropy,
 * the network the mean part only), NULL d_* = zeros, grad NULL = forward only with the same output bits, fixed-order tile sums through ws, plain
 * launches, no atomics.  Served: arch == NULL, continuous, h1 == h2 <= 64, obs_dim <= 128, act_dim <= 16, 1 <= N <= 65536; everything else
 * returns hipErrorInvalidValue with the reason before any device call. */
int icrl_policy_forward_sde(const icrl_policy_t* pol, const double* obs, const float* expl, long long expl_stride, int N, int deterministic,
                            const float* action_low, const float* action_high, float* actions, float* act_clipped, float* v_r, float* v_c,
                            float* log_prob, void* stream);
/* The rollout of a gSDE agent in the library (csrc/rollout_collect.hip): icrl_rollout_collect_ex for a policy with the state-dependent-noise head.
 * The exploration matrices a rollout uses are known before its first step — one draw at the start, one every sample_freq steps — so the
 * caller draws them up front, in the per-step loop's order (ActorTwoCriticsPolicy.noise_schedule), and the kernels compute what that loop
 * computes around icrl_policy_forward_sde: per step the forward of the network, then the head in float64 on the float32 latent (the
 * arithmetic of icrl_policy_forward_sde term for term), the clip, the env step, the cost, the normaliser, the buffer row.
 *   pol   the gSDE descriptor (n_params = the diagonal layout's + 63 * act_dim), params_t as icrl_policy_prepare leaves it on the descriptor of
 *         the network alone (see icrl_policy_forward_sde)
 *   expl  [n_draws][N][64][act_dim] float32: the matrix of env n while draw d is current (rows beyond the latent width zero); step t uses draw
 *         t / sample_freq when sample_freq > 0, draw 0 when it is negative; n_draws >= ceil(T / sample_freq) (or 1).  Must stay alive until
 *         the launch has run.
 *   cn    as for icrl_rollout_collect_ex: a constraint net of the one-workgroup-per-env image, an analytic cost (icrl_cost_fn_t) or NULL
 *   do_gae  bit 0: the dual GAE behind the rollout; bit 1: force the per-step launches
 * Routes: ONE persistent launch, one workgroup per env (rollout_persistent_sde_kernel: no Point env, N <= 128, N obs <= 4096, a workspace,
 * a co-resident grid; every exchange wait bounded, a timed-out one reported through icrl_agent_t.status), else two launches per step
 * (act_step_sde_kernel | norm_step).  Both write the ICRL_FAMILY_ROLLOUT record with ICRL_PICK_SDE set; the two routes agree bit for bit.
 * Refused with hipErrorInvalidValue and the reason, on the host, before any device call: a NULL pointer, a diagonal-layout n_params, a discrete
 * policy, an `arch` descriptor or hidden widths other than the stored 64 x 64, obs_dim above 128 or act_dim above 16, env / policy / buffer
 * shapes that differ, n_draws below what T and sample_freq use, sample_freq 0, a do_gae bit above 1, a discriminator cost
 * (icrl_cost_disc_t), a generic-shape constraint net, more than 4096 envs.
 * Not served in this form: phase timers, the raw-reward plane (icrl_monitor_t), seed batches, the multi-env and column-partitioned kernels. */
int icrl_rollout_collect_sde(const icrl_env_t* env, const icrl_norm_t* nm, const icrl_policy_t* pol, const icrl_costnet_t* cn,
                             const icrl_buffer_t* buf, const icrl_agent_t* ag, const float* expl, int n_draws, int sample_freq,
                             const float* action_low, const float* action_high, double reward_gamma, double reward_gae_lambda,
                             double cost_gamma, double cost_gae_lambda, int do_gae, void* stream);
/* Sampling and evaluation episodes of a gSDE agent as ONE launch (csrc/rollout.hip): icrl_sample_episodes and
 * icrl_sample_episodes_chain for a policy with the state-dependent-noise head.  In a 1-env episode loop the exploration matrices are never
 * redrawn and get_noise picks E0, so ONE matrix serves every step of every episode: there is no schedule and no per-step noise row.  The
 * kernels compute what the per-step loop computes around icrl_policy_forward_sde, bit for bit: the forward of the network, then on the
 * float32 latent the float64 fma chain noise = sum_h latent[h] * expl[h][a] in ascending h, action = (float)(mean + noise), the clip, the env
 * step, the row.  The samplers store no log-prob, so the variance half of the head is not evaluated.
 *   pol   the gSDE descriptor (n_params = the diagonal layout's + 63 * act_dim), params_t as icrl_policy_prepare leaves it on the descriptor
 *         of the network alone (see icrl_policy_forward_sde)
 *   expl  icrl_sample_episodes_sde: [64][act_dim] float32 on the device, the stored shape of the policy's E0 (rows beyond the latent width
 *         zero), or NULL: the mode (the mean clipped to the box, what icrl_policy_forward_sde(deterministic = 1) returns).
 *         icrl_sample_episodes_chain_sde: a HOST array of n_jobs such device pointers; a NULL entry means that job takes the mode.
 *         The matrices must stay alive until the launch has run.
 *   Everything else is as for icrl_sample_episodes / icrl_sample_episodes_chain (jobs: icrl_chain_job_t, unchanged, its `noise` NULL and its
 *   `deterministic` set exactly where expl[j] is NULL; ws sized by icrl_sample_episodes_chain_ws_bytes, args_ws n_jobs * ICRL_BATCH_ARGS_BYTES).
 * Refused with hipErrorInvalidValue and the reason, on the host, before any device call: a NULL required pointer, a diagonal-layout n_params
 * (icrl_sample_episodes serves that policy), a discrete policy, an `arch` descriptor or hidden widths other than the stored 64 x 64, obs_dim
 * above 128 or act_dim above 16, env against policy dimensions, a training normaliser, rows that do not fit, stream_row0 without total_rows,
 * a job with a noise array, a job whose `deterministic` disagrees with expl[j] == NULL.  The chained entry point refuses what
 * icrl_sample_episodes_chain refuses, with a reason starting "icrl_sample_episodes_chain_sde: refused:" (callers take the multi-pass path):
 * more streams than compute units, a Point env, episodes_per_stream != 1, observation widths on both sides of 32 in one launch.
 * Not served in this form: a batch (seed batches), generic shapes, host envs, a log-prob output. */
int icrl_sample_episodes_sde(const icrl_env_t* env, const icrl_norm_t* nm, const icrl_policy_t* pol, const float* expl,
                             const float* action_low, const float* action_high, int episodes_per_stream, int rows_per_stream, int do_reset,
                             const int32_t* stream_row0, int total_rows, double* orig_obs, double* obs, float* actions, double* ep_rewards,
                             int32_t* ep_lengths, void* stream);
int icrl_sample_episodes_chain_sde(int n_jobs, const icrl_chain_job_t* jobs, const float* const* expl, const float* action_low,
                                   const float* action_high, int do_reset, void* ws, long long ws_bytes, void* args_ws, long long args_ws_bytes,
                                   void* stream);
size_t icrl_policy_sde_fwd_bwd_ws_bytes(const icrl_policy_t* pol, int N);
int icrl_policy_sde_fwd_bwd(const icrl_policy_t* pol, const float* obs, const float* actions, int N, const float* d_v_r, const float* d_v_c,
                            const float* d_log_prob, const float* d_entropy, float* v_r, float* v_c, float* log_prob, float* entropy, float* grad,
                            void* ws, long long ws_bytes, void* stream);
/* icrl_ppo_lag_train for a gSDE policy (csrc/ppo_train_sde.hip; kernel: csrc/ppo_train_tiles.hip, HEAD_SDE): PPOLagrangian.train of an agent built with use_sde=True as ONE persistent
 * launch — the column-split tiles kernel of icrl_ppo_lag_train (three workgroups, one per network, weights in LDS, Adam moments in registers,
 * one 8-byte granule per workgroup and step for the gradient norm) with the state-dependent-noise head in the policy workgroup: the variances
 * as a second head GEMM on the squared latent and an LDS image of exp(2 log_std) that is rebuilt after every Adam step, log-prob and entropy per
 * row, d log_std as a GEMM of the head-weight gradient's shape, the latent detached in the variance, the [64, A] entries of log_std and both
 * moments owned in registers, padded rows exactly 0 throughout.  float32 on the matrix core: against the fine-grained loop
 * (icrl_policy_sde_fwd_bwd: float64 rounded once) results differ in the last bits.
 *   The arguments, the statistics row and the contract are icrl_ppo_lag_train's; pol is the gSDE descriptor (n_params = the diagonal layout's
 *   + 63 * act_dim), hp->_pad: bit 0 only (phase timers).  After the launch the call refreshes params_t as icrl_policy_forward_sde reads it
 *   (icrl_policy_prepare on the descriptor of the network alone), so the next rollout needs no further call.  The call leaves the
 *   ICRL_FAMILY_UPDATE route record as it is.  Every inter-workgroup wait is bounded and reports through stats[11].
 *   Served: arch == NULL, continuous, h1 == h2 == 64 (narrower layers stored zero-padded), obs_dim 1..128, act_dim 1..16, batch_size 2..128,
 *   n_epochs >= 1, buf->act_store == act_dim (obs_dim 65..128 takes 161 920 of the workgroup's 163 840 bytes of LDS: the per-row variances
 *   live in spare columns of another image).  Everything else, a NULL pointer and a buffer / policy obs_dim mismatch return
 *   hipErrorInvalidValue with the reason before any device call.
 *   icrl_ppo_lag_train_sde_ws_bytes: bytes of sync_ws for this call (host arithmetic; = ICRL_PPO_SYNC_BYTES(n_epochs, ceil(T*N / batch_size),
 *   T*N)), 0 with the reason in icrl_last_error() where the call is not served. */
size_t icrl_ppo_lag_train_sde_ws_bytes(const icrl_policy_t* pol, const icrl_buffer_t* buf, const icrl_ppo_hyper_t* hp);
int icrl_ppo_lag_train_sde(const icrl_policy_t* pol, float* exp_avg, float* exp_avg_sq, int32_t* adam_step, const icrl_buffer_t* buf,
                           const int32_t* perms, const float* nu, const icrl_ppo_hyper_t* hp, float* stats, void* sync_ws, void* stream);
/* The same for a constraint net on x [N, in_dim] (the rows icrl_cn_prepare writes): zeta = sigmoid(MLP_relu(x)) [N] (may be NULL),
 * grad [n_params] overwritten with sum_n d_zeta[n] dzeta[n]/dθ.  d_zeta and grad both NULL = forward only.  Served: one or two hidden
 * layers of up to 64 units, in_dim <= 128, 1 <= N <= 65536; the tagged descriptors (icrl_cost_fn_t, icrl_cost_disc_t) are refused. */
size_t icrl_cost_mlp_fwd_bwd_ws_bytes(const icrl_costnet_t* cn, int N);
int icrl_cost_mlp_fwd_bwd(const icrl_costnet_t* cn, const float* x, int N, const float* d_zeta, float* zeta, float* grad, void* ws,
                          long long ws_bytes, void* stream);

/* The two calls above with the gradients of the INPUTS (csrc/mlp_grad.hip, the DIN form of the same kernel; icrl_amd/torch_ops.py
 * input_grads=True, ConstraintNet.input_gradients).  Opt-in beside the calls above, which keep their signatures and bits; outputs and grad
 * of an `_in` call are bit-equal to theirs on the same arguments.
 * icrl_policy_fwd_bwd_in: the arguments of icrl_policy_fwd_bwd plus
 *   d_obs     [N, obs_dim]  = sum over pi, vf, cvf (in that order, float64, rounded once) of d loss / d obs through each branch,
 *   d_actions [N, act_dim]  = -d_log_prob[n] (a - mean) / var, the Gaussian head's d loss / d action (the entropy does not depend on it).
 *   Either may be NULL; d_actions must be NULL for a discrete policy (a class index has no gradient; the Categorical entropy's
 *   dependence on obs goes through the logits and is in d_obs).  grad may be NULL while d_obs / d_actions are given: the parameter sums
 *   still go to ws, only their fold into grad is skipped.  The upstream d_* are allowed whenever any of the three outputs is given; all
 *   three NULL is refused (forward only: icrl_policy_fwd_bwd).
 *   Per tile of 16 rows: d x[r][k] = sum_{j < h1, ascending} dz1[r][j] W1[j][k], a float64 fma chain on the float32 weights; a row
 *   belongs to one tile, so nothing is summed across workgroups; each branch writes a float64 slice [N, obs_dim] of ws and one more plain
 *   launch adds the three and rounds.  No atomics; the same call gives the same bits; rows at or beyond N are not written.
 *   ws: ALWAYS needed, icrl_policy_fwd_bwd_in_ws_bytes(pol, N) = (min(ceil(N / 16), 64) n_params + 3 N obs_dim) doubles.
 *   Served: what icrl_policy_fwd_bwd serves; a gSDE layout is refused through n_params.
 * icrl_cost_mlp_fwd_bwd_in: the arguments of icrl_cost_mlp_fwd_bwd plus d_x [N, in_dim] = d loss / d x, the float64 value rounded once
 *   (one network: written by the kernel itself).  d_zeta is required; grad or d_x may be NULL, not both.  ws: ALWAYS needed,
 *   icrl_cost_mlp_fwd_bwd_in_ws_bytes(cn, N) (= icrl_cost_mlp_fwd_bwd_ws_bytes).
 * icrl_cn_prepare_bwd: the chain rule through icrl_cn_prepare (icrl/constraint_net.py:258-299), d_x [N, in_dim] -> d_obs [N, obs_dim]
 *   float64 and d_acs [N, acs_dim] float32 (either may be NULL, not both; d_acs must be NULL for a discrete net).  A kernel of its own,
 *   allocates nothing.  For a source column: the d_x of the selected positions that read it are added in ascending position, in float64
 *   (select_dim may name a column more than once, and an observation column through acs_select_dim); then the clip's derivative, 1
 *   where -clip_obs <= normalised obs <= clip_obs resp. action_low <= a <= action_high (both ends inclusive, as torch.clamp), recomputed
 *   from obs / acs in float64 resp. float32; then 1 / sqrt(var + eps) where the net normalises.  Columns nothing selects get 0.
 * Everything else (the shapes the siblings refuse, the tagged descriptors, a ws below the *_ws_bytes value, d_actions / d_acs with a
 * discrete descriptor, no output requested, a NULL required pointer) returns hipErrorInvalidValue with the reason before any device
 * call.  The calls allocate nothing, do not synchronise and write no route record. */
size_t icrl_policy_fwd_bwd_in_ws_bytes(const icrl_policy_t* pol, int N);
int icrl_policy_fwd_bwd_in(const icrl_policy_t* pol, const float* obs, const float* actions, int N, const float* d_v_r, const float* d_v_c,
                           const float* d_log_prob, const float* d_entropy, float* v_r, float* v_c, float* log_prob, float* entropy, float* grad,
                           float* d_obs, float* d_actions, void* ws, long long ws_bytes, void* stream);
size_t icrl_cost_mlp_fwd_bwd_in_ws_bytes(const icrl_costnet_t* cn, int N);
int icrl_cost_mlp_fwd_bwd_in(const icrl_costnet_t* cn, const float* x, int N, const float* d_zeta, float* zeta, float* grad, float* d_x, void* ws,
                             long long ws_bytes, void* stream);
int icrl_cn_prepare_bwd(const icrl_costnet_t* cn, const double* obs, const float* acs, int N, const float* d_x, double* d_obs, float* d_acs,
                        void* stream);

/* One full-batch regression step of MLP(in -> h1 -> ReLU -> h2 -> ReLU -> out), the reference's create_mlp(in, out, [h1, h2]) with no
 * output squashing: the rollout-end step of the exploration callbacks (icrl/exploration.py:50-67, 227-261; csrc/reg_mlp.hip).
 * params / exp_avg / exp_avg_sq: flat float32 buffers of EXACTLY n_params = h1 (in + 1) + h2 (h1 + 1) + out (h2 + 1) entries in torch's
 * state_dict order, row-major: W1 [h1, in], b1, W2 [h2, h1], b2, W3 [out, h2], b3.  Inputs: xa [rows, in_a] and xb [rows, in_b], row-major,
 * read as ONE concatenated row of in = in_a + in_b values (the buffer's observations and actions planes in their time-major row
 * order; xa may be NULL when in_a == 0); target [rows, out].  Per call, on the parameters as they are:
 *   e = (MLP(x) - target)^2 per element; row_err[r] = sum_j e[r, j] (float32 [rows]; may be NULL);
 *   loss = mean over rows x out of e = MSELoss(reduction='none').mean(); backward of loss; one torch.optim.Adam step (lr, beta1,
 *   beta2, eps as the doubles torch holds; no weight decay, no clipping; bias corrections in double from *adam_step + 1, which is then incremented on the device);
 *   out4 (device) = {loss, mean(row_err), population std(row_err) as np.std, 0}, all from the PRE-step predictions.
 * Arithmetic: the forward pass, the errors and their row sums in float64 on the matrix cores (v_mfma_f64_16x16x4_f64 on the float32
 * parameters and inputs): row_err, the loss and the statistics are the float64 values rounded once.  The backward products of a 32-row
 * group are float32 tiles (v_mfma_f32_16x16x4_f32, exact float32) of the float32 roundings of errors and activations; their sums over
 * groups and workgroups, and the bias sums, are float64, rounded once.  Layers are zero-padded to the 16 x 4 granule in LDS and
 * registers only.  Three plain launches, no cooperative launch, no waits between workgroups, no atomics; the grid is
 * min(ceil(rows / 32), 256) workgroups and every sum has a fixed order: the same call from the same state gives the same bits.
 * Served: 1 <= h1, h2 <= 64, 0 <= in_a <= 128, 1 <= in_b <= 16, 1 <= out <= 128, 1 <= rows <= 2^21.  Everything else, a NULL required
 * pointer and a ws below icrl_reg_mlp_ws_bytes(...) (0 + a reason for a refused shape) return hipErrorInvalidValue with the reason,
 * before any device call.  Allocates nothing, does not synchronise. */
size_t icrl_reg_mlp_ws_bytes(long long rows, int in_a, int in_b, int h1, int h2, int out);
int icrl_reg_mlp_step(float* params, float* exp_avg, float* exp_avg_sq, int32_t* adam_step, const float* xa, const float* xb,
                      const float* target, long long rows, int in_a, int in_b, int h1, int h2, int out, double lr, double beta1,
                      double beta2, double eps, float* row_err, float* out4, void* ws, long long ws_bytes, void* stream);
/* LambdaShapingCallback's `cost_advantages /= (1 + exploration_reward)` (icrl/exploration.py:311): adv[r] = adv[r] / (1.0f + row_err[r]),
 * a correctly rounded float32 division, bit for bit numpy's; rows >= 1. */
int icrl_shape_advantages(float* adv, const float* row_err, long long rows, void* stream);

/* One full-batch classifier step of sigmoid(MLP(in -> h1 -> ReLU -> h2 -> ReLU -> 1)), the reference's create_mlp(in, 1, [h1, h2]) + Sigmoid
 * with BCELoss and Adam: the rollout-end step of CostShapingCallback (icrl/exploration.py:106-128; csrc/cost_shaping.hip).
 * params / exp_avg / exp_avg_sq: flat float32 buffers of EXACTLY n_params = h1 (in + 1) + h2 (h1 + 1) + (h2 + 1) entries in torch's state_dict
 * order, row-major, as in icrl_reg_mlp_step.  Inputs: xa [rows, in_a] FLOAT64 (the un-normalised observations; each value is rounded to
 * float32 on the load, the reference's `.float()`; may be NULL when in_a == 0) and xb [rows, in_b] float32, read as ONE concatenated row;
 * target [rows] float32.  Per call, on the parameters as they are:
 *   p = sigmoid(MLP(x));  loss = mean_r -(y log p + (1 - y) log(1 - p)), each log clamped at -100 as torch's BCELoss does; backward of the
 *   loss (dL/dz as torch forms it: (p - y) / max((1 - p) p, 1e-12) * (1 - p) p); one torch.optim.Adam step (bias corrections in double from
 *   *adam_step + 1, which is then incremented on the device);
 *   out4 (device, FLOAT64 [4]) = {loss, mean(p), mean(target), 0}, all from the PRE-step predictions.
 * Arithmetic and structure as in icrl_reg_mlp_step: the forward pass (hidden layers on v_mfma_f64_16x16x4_f64, the one-unit head per row
 * in unit order), the sigmoid, the logs and the row sums are float64 on the float32 parameters and inputs; the backward products of a
 * 32-row group are float32 (v_mfma_f32_16x16x4_f32 tiles for the hidden layers, VALU products for the one-unit output layer) on the float32
 * roundings; sums across groups, workgroups and biases are float64 in a fixed order, rounded once.  Plain launches, no cooperative launch,
 * no waits between workgroups, no atomics; the grid is min(ceil(rows / 32), 256) workgroups: the same call from the same state gives the
 * same bits.  Served: 1 <= h1, h2 <= 64, 0 <= in_a <= 128, 1 <= in_b <= 16, 1 <= rows <= 2^21.  Everything else, a NULL required pointer
 * and a ws below icrl_cls_mlp_ws_bytes(...) (0 + a reason for a refused shape) return hipErrorInvalidValue with the reason, before any
 * device call.  Allocates nothing, does not synchronise. */
size_t icrl_cls_mlp_ws_bytes(long long rows, int in_a, int in_b, int h1, int h2);
int icrl_cls_mlp_step(float* params, float* exp_avg, float* exp_avg_sq, int32_t* adam_step, const double* xa, const float* xb,
                      const float* target, long long rows, int in_a, int in_b, int h1, int h2, double lr, double beta1, double beta2,
                      double eps, double* out4, void* ws, long long ws_bytes, void* stream);
/* The shaped cost of CostShapingCallback onto the rewards plane (icrl/exploration.py:142-162).  rewards [rows] float32, in / out.
 * With params (the ALREADY STEPPED network, same layout and inputs as above; target unused): shaped[r] = log(float32(p[r])), the float32 log
 * of the float32-rounded prediction as numpy takes it (-inf where that prediction is 0), and rewards[r] += shaped[r], a float32 add.
 * With params == NULL (xa, xb unused; target required): shaped[r] = log(1e-3) * target[r] in float64 and
 * rewards[r] = float32(float64(rewards[r]) + shaped[r]), rounded once.
 * out4 (device, FLOAT64 [4]) = {mean, min, max of shaped, 0}: min and max exact; the mean a float64 sum in fixed order over n — without
 * params it is formed as log(1e-3) * (sum of target / rows), so that it equals log(1e-3) * mean(target) to the bit.
 * ws: at least 8192 bytes (icrl_cls_mlp_ws_bytes(...) always suffices).  Shapes, refusals and determinism as above. */
int icrl_cost_shaping_apply(const float* params, const double* xa, const float* xb, const float* target, long long rows, int in_a, int in_b,
                            int h1, int h2, float* rewards, double* out4, void* ws, long long ws_bytes, void* stream);

/* Diagnostic (bench.py `roofline.copy_gbs`; no reference counterpart): the memory traffic of the streaming dual-GAE launch without
 * its recurrence.  mode 0: grid, access pattern and bytes of icrl_gae_dual at N >= 131 072 (five [T,N] float arrays read, four written,
 * 16-byte non-temporal accesses, one wave per 256 columns walking the rows downwards); mode 1: in0..in3 copied to out0..out3 by
 * four flat grid-stride float4 copies (in4 unused).  N % 4 == 0. */
int icrl_debug_stream_ref(const float* in0, const float* in1, const float* in2, const float* in3, const float* in4,
                          float* out0, float* out1, float* out2, float* out3, int T, int N, int mode, void* stream);

/* Minibatch mode of ConstraintNet.train (`--cn_batch_size`; icrl/constraint_net.py:181-206 with get() :300-316): per
 * iteration the importance weights / early-stop test on ALL nominal rows as above, then one optimiser step per batch of
 * `batch_size` indices out of perms[iteration] ([iterations][min(Nn,Ne)] int32 on the device, the caller's
 * np.random.permutation stream); a batch takes the same row indices from the nominal and the expert set.  metrics rows hold
 * the importance-sampling statistics of the iteration and the loss terms / predictions of its LAST batch (what the
 * reference reports).  work: icrl_cn_train_work_floats(...) floats as for icrl_cn_train. */
int icrl_cn_train_minibatch(const icrl_costnet_t* cn, float* exp_avg, float* exp_avg_sq, int32_t* adam_step,
                            const float* nominal, const float* expert, int Nn, int Ne,
                            const int32_t* ep_offsets, const int32_t* row_episode, int n_ep,
                            const icrl_cn_hyper_t* hp, const int32_t* perms, int batch_size, float* work,
                            float* metrics, void* stream);

/* icrl_cn_train_minibatch for n_runs constraint nets / discriminators of one architecture and one batch_size: the launch sequence of the
 * single-run call with all runs in every launch (grid.y = run).  Per iteration: forward + finalize on all rows, then per minibatch k
 * the minibatch forward, finalize, backward and Adam with step index itr * n_batches + k.  Runs may differ in Nn, Ne and n_ep — hence in
 * min(Nn, Ne), in their number of minibatches and in the length of the ragged last one — and in hp (iterations, learning rate, loss form,
 * importance-sampling mode): the grids and the launch sequence are sized for the largest run, and a launch a run does not have is a no-op
 * for it.  The index slice and length of minibatch (itr, k) are derived in the kernels from the run's argument block.  Per run the call
 * computes the bits icrl_cn_train_minibatch computes (tests/test_gail_seed_batch_gpu.py).  Refused on the host, before the first device
 * call: n_runs outside 1..65535, a small args_ws, NULL perms, batch_size <= 0, runs that differ in network shape or batch_size, an
 * analytic descriptor behind `cn`.
 * Call sites: ConstraintNet.train in minibatch mode (icrl/constraint_net.py:181-206, 300-316) and GailDiscriminator.train
 * (icrl/gail_utils.py:163-208), which always trains through it. */
typedef struct {
  const icrl_costnet_t* cn;
  float *exp_avg, *exp_avg_sq;
  int32_t* adam_step;
  const float *nominal, *expert;
  int32_t Nn, Ne;
  const int32_t *ep_offsets, *row_episode;
  int32_t n_ep, _pad;
  const icrl_cn_hyper_t* hp;
  float *work, *metrics;
  const int32_t* perms;         /* [iterations][min(Nn, Ne)] on the device */
  int32_t batch_size, _pad2;
} icrl_cn_train_mb_job_t;
int icrl_cn_train_minibatch_batch(int n_runs, const icrl_cn_train_mb_job_t* jobs, void* args_ws, long long args_ws_bytes, void* stream);

/* The rollout-end work of the GAIL baseline's callback (icrl/gail_utils.py:500-571) around the discriminator step, for n_runs runs:
 * one job per run, grid.y = run, rows may differ between runs (grids are sized for the largest).
 *   disc:         the run's discriminator (never an analytic descriptor);   true_cost: the ground-truth cost, or NULL (no ground truth)
 *   observations: the buffer's NORMALISED float32 observations [rows, disc->obs_dim];   actions: [rows, act] float32 (act = 1 when discrete)
 *   obs_mean / obs_var: [obs] float64 running moments, or both NULL (norm_obs off);   epsilon: VecNormalize's epsilon
 *   raw_obs: [rows, obs] float64, output of the first call and input of the second;   rewards: [rows] float32, in / out
 *   cost_mean: [1] float64, output;   learn_cost: the --learn_cost flag
 * icrl_gail_unnormalize_batch: raw_obs = float64(obs) * sqrt(var + eps) + mean, product and sum rounded separately (what
 *   VecNormalize.unnormalize_obs computes, icrl/gail_utils.py:539-542); cost_mean = mean of true_cost(raw_obs, actions) over the rows — the
 *   costs are 0, 1 or 2, counted in integers; the mean is count * (1.0 / rows) in float64, the way torch's device mean finishes (the
 *   bits of c.double().mean(); count / rows can differ in the last place) — or 0 for NULL.
 * icrl_gail_relabel_batch: r = log(D(raw_obs, actions) + eps) through the row forward of icrl_disc_reward (icrl/gail_utils.py:147-157:
 *   reward_function with apply_log), then rewards += r with learn_cost and rewards = r without (icrl/gail_utils.py:555-560).  The
 *   discriminators of a batch share one shape.
 * Both: refusals (n_runs, args_ws, rows <= 0, NULL arrays, one of obs_mean / obs_var without the other, an analytic `disc`, a bad
 * true_cost descriptor) are made on the host before the first device call. */
typedef struct {
  const icrl_costnet_t* disc;
  const icrl_cost_fn_t* true_cost;
  const float* observations;
  const float* actions;
  const double *obs_mean, *obs_var;
  double epsilon;
  double* raw_obs;
  float* rewards;
  double* cost_mean;
  int32_t rows, learn_cost;
} icrl_gail_job_t;
int icrl_gail_unnormalize_batch(int n_runs, const icrl_gail_job_t* jobs, void* args_ws, long long args_ws_bytes, void* stream);
int icrl_gail_relabel_batch(int n_runs, const icrl_gail_job_t* jobs, void* args_ws, long long args_ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ICRL_HIP_H */
