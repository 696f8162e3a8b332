// Analytic costs (icrl_cost_fn_t): the ground-truth constraints of icrl/true_constraint_net.py:40-54, 104-111 and the null cost as
// closed forms on (previous raw observation, clipped action) — what the rollout kernels hold in LDS in the wave that runs the
// constraint net.  A descriptor whose n_hidden is ICRL_COST_FN travels through every `const icrl_costnet_t*` argument.
// Discriminator costs (icrl_cost_disc_t, n_hidden == ICRL_COST_DISC) travel the same way: a constraint net read as D = zeta instead of
// 1 - zeta (cpg --load_gail).  The entry point unwraps `net` and picks the kernels whose cost wave returns zeta (KernelPick::disc).
#pragma once
#include "common.h"

namespace icrl {

inline const icrl_cost_fn_t* as_cost_fn(const icrl_costnet_t* cn) {
  return (cn != nullptr && cn->n_hidden == ICRL_COST_FN) ? reinterpret_cast<const icrl_cost_fn_t*>(cn) : nullptr;
}

// the entry points that serve no analytic cost
inline int refuse_cost_fn(const char* who) {
  return fail("%s: an analytic cost descriptor (n_hidden == ICRL_COST_FN) is not served here: icrl_rollout_collect[_ex][_mon], icrl_host_step[_mon], "
              "icrl_cost_mlp_forward and icrl_cost_fn_rows take one", who);
}

inline const icrl_cost_disc_t* as_cost_disc(const icrl_costnet_t* cn) {
  return (cn != nullptr && cn->n_hidden == ICRL_COST_DISC) ? reinterpret_cast<const icrl_cost_disc_t*>(cn) : nullptr;
}

// the entry points that serve no discriminator cost
inline int refuse_cost_disc(const char* who) {
  return fail("%s: a discriminator cost descriptor (icrl_cost_disc_t, n_hidden == ICRL_COST_DISC) is not served here: icrl_rollout_collect[_ex][_mon], "
              "icrl_host_step[_mon] and icrl_cost_mlp_forward take one; the batched rollout kernels have no discriminator form yet, and "
              "training, preparing or icrl_disc_reward want the inner net (icrl_cost_disc_t.net) itself", who);
}

// the inner net of a discriminator cost, or a reason; what the net must satisfy beyond that (cn_ok / bad_cn, params_t) is checked by the
// entry point exactly as for a constraint net handed over directly
inline int cost_disc_check(const char* who, const icrl_cost_disc_t* d) {
  const icrl_costnet_t* net = d->net;
  if (net == nullptr) return fail("%s: discriminator cost descriptor (icrl_cost_disc_t) with a NULL inner net", who);
  if (net->n_hidden < 0) return fail("%s: discriminator cost descriptor (icrl_cost_disc_t) whose inner net is itself a tagged descriptor (n_hidden %d)", who, net->n_hidden);
  if (d->obs_dim != net->obs_dim || d->acs_dim != net->acs_dim || d->in_dim != net->in_dim)
    return fail("%s: discriminator cost descriptor (icrl_cost_disc_t) says obs_dim %d, acs_dim %d, in_dim %d, its inner net %d, %d, %d", who, d->obs_dim,
                d->acs_dim, d->in_dim, net->obs_dim, net->acs_dim, net->in_dim);
  return 0;
}

// discrete: 1 / 0 = the action space of the policy the cost runs beside, -1 = unknown (rows of a caller's own arrays);
// obs_dim / act_dim: the env's (<= 0: unknown)
inline int cost_fn_check(const char* who, const icrl_cost_fn_t* f, int obs_dim, int act_dim, int discrete) {
  if (f->in_dim != 0) return fail("%s: analytic cost with in_dim = %d (must be 0)", who, f->in_dim);
  if (f->kind < ICRL_COST_NULL || f->kind > ICRL_COST_ACTION_EQUALS) return fail("%s: analytic cost of unknown kind %d (0..%d)", who, f->kind, ICRL_COST_ACTION_EQUALS);
  if (obs_dim > 0 && f->obs_dim != obs_dim) return fail("%s: analytic cost built for obs_dim %d, the env has %d", who, f->obs_dim, obs_dim);
  const bool wall = f->kind == ICRL_COST_WALL_BEHIND || f->kind == ICRL_COST_WALL_INFRONT || f->kind == ICRL_COST_WALL_BOTH;
  if (wall && (f->index < 0 || f->index >= f->obs_dim))
    return fail("%s: analytic wall cost on observation column %d outside the observation (obs_dim %d)", who, f->index, f->obs_dim);
  if (f->kind == ICRL_COST_TORQUE) {
    if (discrete == 1) return fail("%s: the torque cost needs a Box action space, the policy's is discrete", who);
    if (f->acs_dim < 1 || (act_dim > 0 && f->acs_dim != act_dim)) return fail("%s: torque cost over %d action components, the env has %d", who, f->acs_dim, act_dim);
  }
  if (f->kind == ICRL_COST_ACTION_EQUALS && discrete == 0) return fail("%s: the action-equals cost needs a discrete action space, the policy's is a Box", who);
  return 0;
}

// The cost of one (observation, action) row.  In the rollout kernels it is called by the wave that calls cost_forward_wave for a
// constraint net, on the same two LDS rows: every lane reads the same addresses (broadcast) and returns the cost.  `f` is a private
// copy made before the step loop, so its fields sit in registers; `index` is wave-uniform.
__device__ __forceinline__ float cost_fn_wave(const icrl_cost_fn_t& f, const double* obs_row, const float* acs_row) {
  switch (f.kind) {
    case ICRL_COST_WALL_BEHIND: return obs_row[f.index] <= f.lo ? 1.f : 0.f;
    case ICRL_COST_WALL_INFRONT: return obs_row[f.index] >= f.hi ? 1.f : 0.f;
    case ICRL_COST_WALL_BOTH: {
      const double o = obs_row[f.index];
      return (o <= f.lo ? 1.f : 0.f) + (o >= f.hi ? 1.f : 0.f);
    }
    case ICRL_COST_TORQUE: {      // numpy compares the float32 array with the threshold as a float32
      const float thr = (float)f.lo;
      bool any = false;
      for (int a = 0; a < f.acs_dim; ++a) any = any || fabsf(acs_row[a]) > thr;
      return any ? 1.f : 0.f;
    }
    case ICRL_COST_ACTION_EQUALS: return acs_row[0] == (float)f.index ? 1.f : 0.f;
    default: return 0.f;
  }
}

}  // namespace icrl
