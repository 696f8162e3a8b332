// What the rollout kernels (rollout.hip) and the dispatch of the fused rollouts (rollout_collect.hip) share — gfx950: the argument blocks of
// the kernels, the limits and dynamic-LDS sizes the route ladders test, the kernel choice as data (KernelPick), the shape checks of the
// entry points, the argument builder, and the launchers rollout.hip exports.
#pragma once
#include <stdio.h>
#include <stdlib.h>

#include "common.h"
#include "cost_fn.h"
#include "generic.h"

namespace icrl {

// ---- argument blocks (the kernels that read them: rollout.hip)
struct ActStepArgs {
  icrl_env_t env;
  union {                 // has_cn: the constraint net, or (the CIT == 0 instantiations) the analytic cost in the same bytes
    icrl_costnet_t cn;
    icrl_cost_fn_t cf;
    icrl_cost_region_t cr;      // the REGION forms: count, combine rule and the device pointer of the clause table
  };
  icrl_buffer_t buf;
  icrl_agent_t ag;
  PolLayout pl;
  CnLayout cl;
  const float* PT;
  const float* noise;   // [T,N,act] (or [T,N] uniforms when discrete)
  const float* alow;
  const float* ahigh;
  int has_cn;
  double* raw_plane;    // [T,N] float64 or NULL: the raw env reward of every step (icrl_monitor_t.raw_rewards), stored next to ag.raw_rew
};

// ---- gSDE (icrl_rollout_collect_sde): the exploration matrices of the whole rollout are drawn up front, in the per-step loop's order, and
// travel as a kernel argument of their own beside the argument blocks above, which keep their layout.
struct SdeArgs {
  const float* expl;        // [n_draws][N][MAX_H][A] float32: the matrix env n uses while draw d is current
  long long draw_stride;    // N * MAX_H * A
  long long env_stride;     // MAX_H * A
  int sample_freq;          // > 0: step t uses draw t / sample_freq; < 0: draw 0 throughout
  const float* ls;          // log_std [MAX_H][A] as it lies in `params` (rows beyond the latent width are zero and meet a zero latent)
};

// act_step_generic_kernel: the rest of a generic-shape step behind the forward and cost launches
struct GenStepArgs {
  icrl_env_t env;
  icrl_buffer_t buf;
  icrl_agent_t ag;
  int has_cn;           // 1: ag.raw_cost holds the constraint net's cost of this step; 2: the analytic cost `cf`, evaluated here
  double* raw_plane;    // see ActStepArgs
  icrl_cost_fn_t cf;
};

// norm_step_kernel / norm_step_small_kernel: VecNormalizeWithCost.step_wait for all envs
struct NormStepArgs {
  icrl_norm_t nm;
  const double* raw_obs;   // [N,O]
  const double* raw_rew;   // [N]
  const float* raw_cost;   // [N] or NULL
  const uint8_t* dones;    // [N]
  int N, O;
  double* obs_out;         // [N,O] float64 or NULL
  double* rew_out;         // [N] or NULL
  double* cost_out;        // [N] or NULL
  float* obs_f32;          // buffer.new_observations[t] or NULL
  float* rew_f32;          // buffer.rewards[t] or NULL
  float* cost_f32;         // buffer.costs[t] or NULL
  uint8_t* last_dones;     // [N] or NULL: receives dones
};

constexpr int NORM_MAX_N = 4096;                 // envs handled by the single-workgroup normaliser (and per GPU)
constexpr int WIDE_MAX_N = 1024;                 // rollout_wide_kernel's static buffers; beyond: rollout_multi_kernel
constexpr int NORM_MAX_LEAVES = NORM_MAX_N / 64 + 2;
constexpr int NORM_CHUNK = 4096;                 // doubles of raw obs staged in LDS per pass

// the persistent rollout, one workgroup per env (rollout_persistent_body)
struct PersistArgs {
  ActStepArgs act;
  icrl_norm_t nm;
  int T;
  double* xch_obs;     // [2][N][O]
  double* xch_rew;     // [2][N]
  float* xch_cost;     // [2][N]
  unsigned* xch_done;  // [2][N]
  unsigned* counter;   // [N] barrier flags, zeroed before the launch
  unsigned long long* xg;   // granule mode: [2][N][2 obs + 4] self-validating 8-byte words {step tag | 32 payload bits}, zeroed
  unsigned g_magic;         // floor(2^32 / (2 obs + 4)) for the index split
  int prof;            // diagnostic phase timers (do_gae bit 2)
};

constexpr int GRAN_MAX = 12;    // 8-byte words of exchange area per thread in record mode (N (2 obs + 4) <= 256 * GRAN_MAX) ...
constexpr int REC_MAX = GRAN_MAX / 2;   // ... = 16-byte records a thread polls per step
// dynamic LDS of the persistent rollout: the transposed observation block [obs][N + 64] and the dynamics matrix [obs][act], sized
// for the launch's shapes (HC x 64: 19 KB instead of the 114 KB of the largest admissible shape, so that several workgroups —
// several runs of a batched launch — share a CU)
static inline size_t persist_dyn_lds(int N, int O, int A) { return ((size_t)O * (size_t)(N + 64) + (size_t)O * (size_t)A) * sizeof(double); }
static inline size_t persist_sde_dyn_lds(int N, int O, int A) { return persist_dyn_lds(N, O, A) + (size_t)MAX_H * (size_t)A * (sizeof(double) + sizeof(float)); }

// rollout_generic_kernel
struct GenRolloutArgs {
  PersistArgs p;
  GenNet net;
  const float* P;      // the policy's parameters in their natural layout (log_std of the Gaussian head)
};

// rollout_wide_kernel (at most WIDE_E envs per workgroup) and the multi-env kernels
constexpr int WIDE_E = 4;

struct WideArgs {
  ActStepArgs act;
  icrl_norm_t nm;
  int T, G;                    // steps; grid size (workgroup g serves envs g, g + G, ...)
  int prof;                    // diagnostic phase timers of workgroup `prof - 1` (do_gae bit 2: workgroup 0; bit 3: the last one)
  unsigned long long* xg;      // [2][N][2 obs + 4] env granules {step tag | 32 payload bits}, zeroed before the launch
  unsigned long long* sg;      // [2][4 obs + 4] statistics granules, zeroed before the launch
  unsigned long long* xcc;     // multi-env kernel, packed batched launches: G zeroed words (the workgroups' XCD ids), else NULL
};

static inline size_t multi_dyn_lds(int N, int O, int A, int owners) {
  // dynamics matrix | per owner wave: column buffer (N + 64) | ret / cost owners: done flags [2][N] bytes.  (The discounted returns of
  // the previous step stay in nm.ret / nm.cost_ret: only their owner wave touches them during the launch.)
  return ((size_t)O * A + (size_t)owners * (size_t)(N + 64)) * sizeof(double) + 2 * (size_t)((N + 15) / 16 * 16);
}

// ---- which instantiation serves a shape, as data: the with_*_kernel dispatch of rollout.hip turns it into a kernel
struct KernelPick {
  bool small = false;      // small_shape(): the <2, .> register images, else <8, .>
  bool analytic = false;   // an icrl_cost_fn_t behind the cost pointer: CIT == 0 (no cost-net register image), no phase timers
  bool mon = false;        // the instantiations that store the raw-reward plane (ActStepArgs.raw_plane); no phase timers
  bool cn128 = false;      // multi kernels: the cost net reads <= 128 inputs (AntWall: 121) — 32 instead of 40 first-layer k steps in the register image
  bool gran = false;       // one-workgroup-per-env kernels: granule mode (N (2 obs + 4) <= 256 GRAN_MAX)
  bool prof = false;       // tools: the instantiations with the phase timers (do_gae bits 2 / 3)
  bool disc = false;       // an icrl_cost_disc_t behind the cost pointer: the kernels whose cost wave returns zeta; single runs, no phase timers
  bool sde = false;        // icrl_rollout_collect_sde: the kernels with the gSDE head (with_act_step_sde_kernel, with_persistent_sde_kernel)
  bool region = false;     // an icrl_cost_region_t behind the cost pointer: the CIT == 0 image with the region cost wave; single runs, no phase timers
  int E = 0;              // multi kernels: envs per workgroup (multi_shape)
  int minw = 1;            // batched one-workgroup-per-env kernels: workgroups per CU the register allocation leaves room for
  // what the dispatch (with_*_kernel, rollout.hip) instantiated, written by it for the route record (pick_bits): the MINW of with_persistent_batch_kernel,
  // whether with_image took the <8, 8> image
  mutable int used_minw = 0;
  mutable bool used_cn128 = false;
};

// observations of <= 32 columns beside a cost net of <= 32 inputs.  `net` is the constraint net proper: NULL without a cost and NULL
// for an analytic cost, which has no inputs to count
static inline bool small_shape(int O, const icrl_costnet_t* net) { return O <= 32 && (net == nullptr || net->in_dim <= 32); }

// ---- shape checks of the entry points
static inline bool dims_ok(const icrl_policy_t* p) {      // what the fused kernels serve: two hidden layers per branch, no shared trunk
  return p->arch == nullptr && p->obs_dim > 0 && p->obs_dim <= MAX_OBS && p->act_dim > 0 && p->act_dim <= MAX_ACT && p->h1 > 0 && p->h1 <= MAX_H &&
         p->h2 > 0 && p->h2 <= MAX_H;
}
static inline bool cn_ok(const icrl_costnet_t* cn) {
  return cn->in_dim > 0 && cn->in_dim <= MAX_CN_IN && cn->h1 > 0 && cn->h1 <= MAX_H && (cn->n_hidden == 1 ||
         (cn->n_hidden == 2 && cn->h2 > 0 && cn->h2 <= MAX_H)) && cn->obs_dim <= MAX_OBS && cn->acs_dim <= MAX_ACT;
}
static inline int bad_dims(const char* who, const icrl_policy_t* p) {
  return fail("%s: policy obs_dim %d (1..%d), act_dim %d (1..%d), hidden (%d, %d) (1..%d each)%s; wider policies, shared trunks and other depths run "
              "through the generic-shape entry points: icrl_policy_forward / icrl_policy_evaluate / icrl_ppo_lag_train and the per-step rollout", who,
              p->obs_dim, MAX_OBS, p->act_dim, MAX_ACT, p->h1, p->h2, MAX_H, p->arch != nullptr ? ", an `arch` descriptor" : "");
}
static inline int bad_cn(const char* who, const icrl_costnet_t* cn) {
  return fail("%s: constraint net in_dim %d (1..%d), %d hidden layers (1 or 2) of (%d, %d) (1..%d; wider and deeper nets: icrl_cost_mlp_forward / icrl_disc_reward / icrl_cn_train and the per-step rollout), obs_dim %d (<= %d), acs_dim %d (<= %d)", who,
              cn->in_dim, MAX_CN_IN, cn->n_hidden, cn->h1, cn->h2, MAX_H, cn->obs_dim, MAX_OBS, cn->acs_dim, MAX_ACT);
}

// ---- the argument block every rollout kernel starts from.  env NULL: the caller fills a.env (host envs).  net | cf: the constraint net
// or the analytic cost, at most one of them.  table_forward: the generic-shape kernel, which reads only obs / act / discrete of the layout.
static inline void fill_act_args(ActStepArgs& a, const icrl_env_t* env, const icrl_buffer_t* buf, const icrl_agent_t* ag, const icrl_policy_t* pol,
                          bool table_forward, const icrl_costnet_t* net, const icrl_cost_fn_t* cf, const float* noise, const float* action_low,
                          const float* action_high, double* raw_plane) {
  if (env != nullptr) a.env = *env;
  a.buf = *buf; a.ag = *ag; a.raw_plane = raw_plane;
  a.pl = make_pol_layout(pol->obs_dim, pol->act_dim, table_forward ? MAX_H : pol->h1, table_forward ? MAX_H : pol->h2, pol->discrete);
  a.PT = pol->params_t; a.noise = noise; a.alow = action_low; a.ahigh = action_high;
  a.has_cn = net != nullptr || cf != nullptr;
  if (net) { a.cn = *net; a.cl = make_cn_layout(net->in_dim, net->n_hidden, net->h1, net->h2); }
  else if (cf) a.cf = *cf;
}

// the raw-reward plane of a monitor descriptor (NULL descriptor: no plane, the kernels then store nothing extra)
static inline int mon_plane(const char* who, const icrl_monitor_t* mon, double** plane) {
  *plane = nullptr;
  if (mon == nullptr) return 0;
  if (mon->raw_rewards == nullptr) return fail("%s: icrl_monitor_t.raw_rewards is NULL (a [T, N] float64 plane is required)", who);
  *plane = mon->raw_rewards;
  return 0;
}

// ---- launchers: what rollout_collect.hip asks of rollout.hip.  Each picks its instantiation from `k` (with_*_kernel, which writes k.used_minw /
// k.used_cn128) and launches it on `s`; the return value is the HIP error of the launch, or -1: the grid cannot be co-resident on this
// device (the caller tries its next route)
void launch_act_step(const KernelPick& k, int N, hipStream_t s, const ActStepArgs& a, int t);
void launch_act_step_sde(const KernelPick& k, int N, hipStream_t s, const ActStepArgs& a, const SdeArgs& sd, int t);
void launch_act_step_generic(int N, hipStream_t s, const GenStepArgs& g, int t);
void launch_norm_step(const NormStepArgs& a, hipStream_t s);
int launch_rollout_generic(const KernelPick& k, int N, size_t dyn, hipStream_t s, GenRolloutArgs& ga);
int launch_rollout_persistent(const KernelPick& k, int N, size_t dyn, hipStream_t s, PersistArgs& p);
int launch_rollout_persistent_sde(const KernelPick& k, int N, size_t dyn, hipStream_t s, PersistArgs& p, SdeArgs& sd);
int launch_rollout_persistent_batch(const KernelPick& k, int N, int n_runs, size_t dyn, hipStream_t s, const PersistArgs* d_args);
int rollout_wide_blocks_per_cu(const KernelPick& k, int* per_cu);      // the occupancy answer (a hipError_t) of the instantiation `k` names
int launch_rollout_wide(const KernelPick& k, int G, hipStream_t s, WideArgs& p);
int launch_rollout_multi(const KernelPick& k, WideArgs& p, int G, size_t dyn, hipStream_t s, int* packed_out);
int launch_rollout_multi_batch(const KernelPick& k, const WideArgs* d_args, int n_runs, int G, size_t dyn, hipStream_t s, int* packed_out);
// the argument block of one run of a batched launch, to device memory (common.h: put_args)
int put_rollout_args(const PersistArgs& p, PersistArgs* dst, hipStream_t s);
int put_rollout_args(const WideArgs& p, WideArgs* dst, hipStream_t s);

}  // namespace icrl
