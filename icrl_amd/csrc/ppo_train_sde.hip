// PPO-Lagrangian update of a gSDE policy as ONE persistent launch: the entry points — gfx950.
//
// ref: stable_baselines3/ppo_lag/ppo_lag.py:196-299 (PPOLagrangian.train), common/distributions.py:408-601 (StateDependentNoiseDistribution
//      with full_std, exp, no squashing, learn_features = False).
//
// The kernel is the column-split tiles kernel with the state-dependent-noise head (csrc/ppo_train_tiles.hip, HEAD_SDE; its header describes
// the head).  Here: what the call serves (train_sde_check: host arithmetic only, every refusal before any device call), the workspace size,
// and the host steps of a call — the two memsets, the launch, the transposes the next rollout reads.  The update family's route record
// (ICRL_FAMILY_UPDATE) is never touched.
#include "ppo_common.h"

using namespace icrl;

namespace {

// 0, or the fail() code of a call the kernel does not serve: host arithmetic only
int train_sde_check(const char* who, const icrl_policy_t* pol, const icrl_buffer_t* buf, const icrl_ppo_hyper_t* hp) {
  if (pol == nullptr || buf == nullptr || hp == nullptr) return fail("%s: NULL argument (pol, buf and hp are required)", who);
  if (pol->arch != nullptr || pol->h1 != HD || pol->h2 != HD)
    return fail("%s: hidden widths (%d, %d)%s; the persistent gSDE update is built for two hidden layers per branch stored %d x %d, no `arch`", who, pol->h1, pol->h2,
                pol->arch != nullptr ? " with an `arch` descriptor" : "", HD, HD);
  if (pol->obs_dim < 1 || pol->obs_dim > MAX_OBS || pol->act_dim < 1 || pol->act_dim > MAX_ACT)
    return fail("%s: obs_dim %d (1..%d) / act_dim %d (1..%d)", who, pol->obs_dim, MAX_OBS, pol->act_dim, MAX_ACT);
  if (pol->discrete) return fail("%s: a discrete policy has no gSDE head (Box action spaces only)", who);
  const PolLayout L = make_sde_layout(pol->obs_dim, pol->act_dim, pol->h1, pol->h2);
  if (pol->n_params != L.n)
    return fail("%s: n_params %d, the gSDE (log_std [64, act_dim]) layout of (%d, %d, %d, %d) has %d (the diagonal layout %d: icrl_ppo_lag_train serves that one)", who,
                pol->n_params, pol->obs_dim, pol->act_dim, pol->h1, pol->h2, L.n, L.n - (MAX_H - 1) * pol->act_dim);
  if (hp->batch_size < 2 || hp->batch_size > SDE_MAX_B || hp->n_epochs < 1)
    return fail("%s: batch_size %d (2..%d: one minibatch = at most two 64-row chunks), n_epochs %d (>= 1)", who, hp->batch_size, SDE_MAX_B, hp->n_epochs);
  if (hp->n_epochs >= (1 << 19)) return fail("%s: n_epochs %d, limit 2^19", who, hp->n_epochs);
  if (buf->obs_dim != pol->obs_dim || buf->T < 1 || buf->N < 1)
    return fail("%s: buffer obs_dim %d vs policy %d, T = %d, N = %d", who, buf->obs_dim, pol->obs_dim, buf->T, buf->N);
  if (buf->act_store != pol->act_dim)
    return fail("%s: buffer act_store %d, a continuous policy of act_dim %d stores %d floats per action", who, buf->act_store, pol->act_dim, pol->act_dim);
  if ((long long)buf->T * buf->N >= (1ll << 31) || (long long)buf->T * buf->N * (pol->obs_dim > 16 ? pol->obs_dim : 16) >= (1ll << 30))
    return fail("%s: %d x %d transitions x obs_dim %d overflow the kernel's 32-bit element offsets (limit 2^30 floats per plane)", who, buf->T, buf->N, pol->obs_dim);
  const long long n_mb = ((long long)buf->T * buf->N + hp->batch_size - 1) / hp->batch_size;
  if ((long long)hp->n_epochs * n_mb >= (1ll << 31)) return fail("%s: %lld optimiser steps per call, limit 2^31", who, (long long)hp->n_epochs * n_mb);
  return 0;
}

}  // namespace

extern "C" size_t icrl_ppo_lag_train_sde_ws_bytes(const icrl_policy_t* pol, const icrl_buffer_t* buf, const icrl_ppo_hyper_t* hp) {
  if (train_sde_check("icrl_ppo_lag_train_sde_ws_bytes", pol, buf, hp) != 0) return 0;
  const size_t n_total = (size_t)buf->T * (size_t)buf->N;
  const size_t n_mb = (n_total + hp->batch_size - 1) / hp->batch_size;
  return ICRL_PPO_SYNC_BYTES(hp->n_epochs, n_mb, n_total);
}

extern "C" int icrl_ppo_lag_train_sde(const icrl_policy_t* pol, float* exp_avg, float* exp_avg_sq, int32_t* adam_step, const icrl_buffer_t* buf,
                                      const int32_t* perms, const float* nu, const icrl_ppo_hyper_t* hp, float* stats, void* sync_ws, void* stream) {
  const char* who = "icrl_ppo_lag_train_sde";
  if (const int e = train_sde_check(who, pol, buf, hp)) return e;
  if (pol->params == nullptr || pol->params_t == nullptr || exp_avg == nullptr || exp_avg_sq == nullptr || adam_step == nullptr || perms == nullptr || nu == nullptr ||
      stats == nullptr || sync_ws == nullptr)
    return fail("%s: NULL argument (pol->params, pol->params_t, exp_avg, exp_avg_sq, adam_step, perms, nu, stats and sync_ws are required)", who);
  if (buf->observations == nullptr || buf->actions == nullptr || buf->log_probs == nullptr || buf->reward_advantages == nullptr || buf->cost_advantages == nullptr ||
      buf->reward_returns == nullptr || buf->cost_returns == nullptr || buf->reward_values == nullptr || buf->cost_values == nullptr)
    return fail("%s: NULL buffer plane (observations, actions, log_probs, both advantages, returns and values are read)", who);
  hipStream_t s = (hipStream_t)stream;
  TrainArgs a;
  a.L = make_sde_layout(pol->obs_dim, pol->act_dim, pol->h1, pol->h2);
  a.params = pol->params; a.exp_avg = exp_avg; a.exp_avg_sq = exp_avg_sq; a.adam_t = adam_step;
  a.buf = *buf; a.perms = perms; a.nu = nu; a.hp = *hp; a.stats = stats; a.xch = (u64*)sync_ws;
  a.t_magic = buf->T == 1 ? 0xFFFFFFFFu : (unsigned)((1ull << 32) / (unsigned long long)buf->T);
  a.plan_steps = nullptr; a.plan_chunks = nullptr; a.n_steps = 0; a.gx = nullptr; a.srec = nullptr; a.sstat = nullptr;
  hipError_t e = hipMemsetAsync(sync_ws, 0, 512, s);      // granule slots (prepare_train's layout: 2 step parities x 4 words are used)
  if (e != hipSuccess) return (int)e;
  e = hipMemsetAsync(stats, 0, (32 + hp->n_epochs) * sizeof(float), s);
  if (e != hipSuccess) return (int)e;
  int packed = 0;      // (three workgroups, no packed form — and no route record: that is the update family's)
  const int err = launch_train_tiles(a, (pol->obs_dim + 15) / 16, HEAD_SDE, s, &packed);
  if (err != 0) return err;
  // what icrl_policy_forward_sde reads: the network's transposes, for the descriptor of the network alone (rollout.hip: launch_policy_forward_sde)
  icrl_policy_t net = *pol;
  const int skip = (MAX_H - 1) * pol->act_dim;
  net.params = pol->params + skip; net.params_t = pol->params_t + skip; net.n_params = pol->n_params - skip; net.discrete = 0;
  return icrl_policy_prepare(&net, stream);
}
