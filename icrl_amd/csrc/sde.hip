// Generalised state-dependent exploration (gSDE) for the two-critics policy — gfx950.
//
// ref: stable_baselines3/common/distributions.py:408-601 (StateDependentNoiseDistribution), common/policies.py:434-441, 671-690, 716-779 — with
// what PPOLagrangian(use_sde=True) builds: full_std, exp (no expln), no squashing, no sde_net_arch, hence learn_features = False.
//
// The head replaces the diagonal Gaussian's vector log_std [A] by a matrix log_std [H, A] over the policy branch's last tanh layer (the latent):
//   sample    action = mean + latent . E                          E ~ Normal(0, exp(log_std)), drawn by the host (reset_noise), one per env
//   density   Normal(mean, sqrt(sum_h latent_h^2 exp(2 log_std[h, a]) + 1e-6)) per action, log_prob / entropy summed over the actions
//   gradient  log_std through the variance; the network through the mean only (the latent is detached in the variance)
// A gSDE policy keeps the ordinary descriptor (icrl_policy_t is unchanged); its buffer differs in the first tensor alone: log_std is stored
// [MAX_H, A], rows beyond the last hidden width zero (common.h: make_sde_layout), and n_params says so — every other entry point compares
// n_params with the diagonal layout, or is kept away by the Python layer, and refuses such a descriptor.
//
// The two entry points are the gSDE forms of icrl_policy_forward and icrl_policy_fwd_bwd and share their kernels' arithmetic:
//   icrl_policy_forward_sde  -> rollout.hip: policy_forward_sde_kernel = policy_forward_block (the three branch forwards, bit for bit) + the head
//   icrl_policy_sde_fwd_bwd  -> mlp_grad.hip: mlp_fwd_bwd_kernel<tanh, SDE> (branch forward / backward shared, float64 rounded once) + the head
// Here: the argument checks, all on the host before any device call.
#include "common.h"

using namespace icrl;

extern "C" int icrl_policy_forward_sde(const icrl_policy_t* pol, const double* obs, const float* expl, long long expl_stride, int N, int deterministic,
                                       const float* action_low, const float* action_high, float* actions, float* act_clipped, float* v_r, float* v_c,
                                       float* log_prob, void* stream) {
  const char* who = "icrl_policy_forward_sde";
  if (const int e = sde_fwd_bwd_check(who, pol, N)) return e;      // (the same served set as the update's entry point)
  if (pol->params == nullptr || pol->params_t == nullptr || obs == nullptr) return fail("%s: NULL argument (pol->params, pol->params_t and obs are required)", who);
  if (!deterministic && expl == nullptr) return fail("%s: a sampled forward needs the exploration matrices (expl NULL with deterministic = 0)", who);
  const long long per_row = (long long)MAX_H * pol->act_dim;
  if (expl_stride != 0 && expl_stride != per_row)
    return fail("%s: expl_stride %lld (0: one matrix for all rows; %lld = %d * act_dim: one per row)", who, expl_stride, per_row, MAX_H);
  return launch_policy_forward_sde(pol, obs, expl, expl_stride, N, deterministic, action_low, action_high, actions, act_clipped, v_r, v_c, log_prob,
                                   (hipStream_t)stream);
}

extern "C" size_t icrl_policy_sde_fwd_bwd_ws_bytes(const icrl_policy_t* pol, int N) {
  if (sde_fwd_bwd_check("icrl_policy_sde_fwd_bwd_ws_bytes", pol, N) != 0) return 0;
  return (size_t)sde_fwd_bwd_parts(N) * (size_t)pol->n_params * sizeof(double);
}

extern "C" int icrl_policy_sde_fwd_bwd(const icrl_policy_t* pol, const float* obs, const float* actions, int N, const float* d_v_r, const float* d_v_c,
                                       const float* d_log_prob, const float* d_entropy, float* v_r, float* v_c, float* log_prob, float* entropy,
                                       float* grad, void* ws, long long ws_bytes, void* stream) {
  const char* who = "icrl_policy_sde_fwd_bwd";
  if (const int e = sde_fwd_bwd_check(who, pol, N)) return e;
  if (pol->params == nullptr || obs == nullptr || actions == nullptr) return fail("%s: NULL argument (pol->params, obs and actions are required)", who);
  if (grad == nullptr && (d_v_r != nullptr || d_v_c != nullptr || d_log_prob != nullptr || d_entropy != nullptr))
    return fail("%s: upstream gradients without `grad` (grad NULL = forward only: pass no d_* then)", who);
  const long long need = (long long)sde_fwd_bwd_parts(N) * pol->n_params * (long long)sizeof(double);
  if (grad != nullptr && (ws == nullptr || ws_bytes < need))
    return fail("%s: ws of %lld bytes, icrl_policy_sde_fwd_bwd_ws_bytes(pol, %d) = %lld", who, ws == nullptr ? 0LL : ws_bytes, N, need);
  return launch_sde_fwd_bwd(pol, obs, actions, N, d_v_r, d_v_c, d_log_prob, d_entropy, v_r, v_c, log_prob, entropy, grad, ws, (hipStream_t)stream);
}
