// Analytic costs (icrl_cost_fn_t): the ground-truth constraints of icrl/true_constraint_net.py:40-54, 104-111 and the null cost as
// closed forms on (previous raw observation, clipped action) — what the rollout kernels hold in LDS in the wave that runs the
// constraint net.  A descriptor whose n_hidden is ICRL_COST_FN travels through every `const icrl_costnet_t*` argument.
// Discriminator costs (icrl_cost_disc_t, n_hidden == ICRL_COST_DISC) travel the same way: a constraint net read as D = zeta instead of
// 1 - zeta (cpg --load_gail).  The entry point unwraps `net` and picks the kernels whose cost wave returns zeta (KernelPick::disc).
// Region costs (icrl_cost_region_t, n_hidden == ICRL_COST_REGION) are the third: a user-defined constraint as a table of box / halfspace /
// ball clauses, copied into LDS before the step loop and evaluated by the cost wave (cost_region_wave, KernelPick::region).
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
  if (net->n_hidden == ICRL_COST_REGION)
    return fail("%s: discriminator cost descriptor (icrl_cost_disc_t) whose inner net is a region cost descriptor (icrl_cost_region_t): a region "
                "cost is no network to read as D", who);
  if (net->n_hidden < 0) return fail("%s: discriminator cost descriptor (icrl_cost_disc_t) whose inner net is itself a tagged descriptor (n_hidden %d)", who, net->n_hidden);
  if (d->obs_dim != net->obs_dim || d->acs_dim != net->acs_dim || d->in_dim != net->in_dim)
    return fail("%s: discriminator cost descriptor (icrl_cost_disc_t) says obs_dim %d, acs_dim %d, in_dim %d, its inner net %d, %d, %d", who, d->obs_dim,
                d->acs_dim, d->in_dim, net->obs_dim, net->acs_dim, net->in_dim);
  return 0;
}

inline const icrl_cost_region_t* as_cost_region(const icrl_costnet_t* cn) {
  return (cn != nullptr && cn->n_hidden == ICRL_COST_REGION) ? reinterpret_cast<const icrl_cost_region_t*>(cn) : nullptr;
}

// the entry points that serve no region cost
inline int refuse_cost_region(const char* who) {
  return fail("%s: a region cost descriptor (icrl_cost_region_t, n_hidden == ICRL_COST_REGION) is not served here: icrl_rollout_collect[_ex][_mon] "
              "beside a policy of the one-workgroup-per-env image, icrl_host_step[_mon], icrl_cost_mlp_forward and icrl_cost_region_rows take one; "
              "the batched, gSDE and generic-shape rollout kernels have no region form, and training, preparing or icrl_disc_reward want a "
              "constraint net", who);
}

// A region descriptor is checked on its HOST clause table, before any HIP call.  discrete: 1 / 0 = the action space of the policy the
// cost runs beside, -1 = unknown (rows of a caller's own arrays); obs_dim / act_dim: the env's (<= 0: unknown).  An action column must
// be one the policy's action space provides: column 0 alone beside a discrete policy, columns < act_dim beside a Box.
inline int cost_region_check(const char* who, const icrl_cost_region_t* r, int obs_dim, int act_dim, int discrete) {
  if (r->in_dim != 0) return fail("%s: region cost (icrl_cost_region_t) with in_dim = %d (must be 0)", who, r->in_dim);
  if (r->obs_dim < 0 || r->acs_dim < 0 || r->obs_dim + r->acs_dim < 1)
    return fail("%s: region cost (icrl_cost_region_t) with obs_dim %d, acs_dim %d", who, r->obs_dim, r->acs_dim);
  if (obs_dim > 0 && r->obs_dim != obs_dim) return fail("%s: region cost (icrl_cost_region_t) built for obs_dim %d, the env has %d", who, r->obs_dim, obs_dim);
  if (r->n_clauses < 1 || r->n_clauses > ICRL_REGION_MAX_CLAUSES)
    return fail("%s: region cost (icrl_cost_region_t) with %d clauses (1..%d)", who, r->n_clauses, ICRL_REGION_MAX_CLAUSES);
  if (r->combine < ICRL_REGION_ANY || r->combine > ICRL_REGION_SUM)
    return fail("%s: region cost (icrl_cost_region_t) with unknown combine rule %d (0..%d)", who, r->combine, ICRL_REGION_SUM);
  if (r->clauses == nullptr) return fail("%s: region cost (icrl_cost_region_t) with a NULL host clause table", who);
  if (r->d_clauses == nullptr) return fail("%s: region cost (icrl_cost_region_t) with a NULL device clause table", who);
  const int acs_have = discrete == 1 ? 1 : (discrete == 0 && act_dim > 0 ? act_dim : r->acs_dim);
  for (int c = 0; c < r->n_clauses; ++c) {
    const icrl_region_clause_t& q = r->clauses[c];
    if (q.type < ICRL_REGION_BOX || q.type > ICRL_REGION_BALL)
      return fail("%s: region cost (icrl_cost_region_t): clause %d of unknown type %d (0..%d)", who, c, q.type, ICRL_REGION_BALL);
    if (q.n_terms < 1 || q.n_terms > ICRL_REGION_MAX_TERMS)
      return fail("%s: region cost (icrl_cost_region_t): clause %d with %d terms (1..%d)", who, c, q.n_terms, ICRL_REGION_MAX_TERMS);
    for (int k = 0; k < q.n_terms; ++k) {
      if (q.col[k] < 0 || q.col[k] >= r->obs_dim + r->acs_dim)
        return fail("%s: region cost (icrl_cost_region_t): clause %d, term %d reads column %d outside obs_dim %d + acs_dim %d", who, c, k, q.col[k],
                    r->obs_dim, r->acs_dim);
      if (q.col[k] >= r->obs_dim && q.col[k] - r->obs_dim >= acs_have)
        return fail("%s: region cost (icrl_cost_region_t): clause %d, term %d reads action column %d, the policy's action space provides %d", who, c,
                    k, q.col[k] - r->obs_dim, acs_have);
    }
    if (q.type == ICRL_REGION_BALL && !(q.c >= 0.0))
      return fail("%s: region cost (icrl_cost_region_t): clause %d is a ball with r2 = %g (must be >= 0)", who, c, q.c);
  }
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

// ---- region costs (icrl_cost_region_t).  The clause table lies in LDS (region_table_load, once before the step loop; the rows kernel
// reads it from its own LDS copy too): a by-value kernel argument is never indexed dynamically.  One clause on one row, in the order the
// header states: every product and sum is an operation of its own (the project compiles with -ffp-contract=off).
__device__ __forceinline__ bool region_clause(const icrl_region_clause_t& q, const double* obs_row, const float* acs_row, int O) {
  const int type = q.type;
  double acc = type == ICRL_REGION_HALFSPACE ? q.c : 0.0;
  bool in = true;
  for (int k = 0; k < q.n_terms; ++k) {
    const int col = q.col[k];
    const double x = col < O ? obs_row[col] : (double)acs_row[col - O];
    const double ak = q.a[k];
    if (type == ICRL_REGION_BOX) in = in && (ak <= x && x <= q.b[k]);
    else if (type == ICRL_REGION_HALFSPACE) acc = acc + ak * x;
    else { const double d = x - ak; acc = acc + d * d; }
  }
  const bool r = type == ICRL_REGION_BOX ? in : (type == ICRL_REGION_HALFSPACE ? acc >= 0.0 : acc <= q.c);
  return q.negate ? !r : r;
}

// what the launch carries of a descriptor: the bytes of the argument block that otherwise hold the analytic cost (same size)
static_assert(sizeof(icrl_cost_region_t) == sizeof(icrl_cost_fn_t), "a region descriptor travels in the analytic descriptor's slot");
static_assert(sizeof(icrl_region_clause_t) % sizeof(double) == 0, "the clause table is copied as 8-byte words");

// all threads of the workgroup: device table -> LDS; a workgroup barrier must follow before the first cost_region_*
__device__ __forceinline__ void region_table_load(icrl_region_clause_t* tab, const icrl_cost_region_t& r, int tid, int threads) {
  const double* src = reinterpret_cast<const double*>(as_global(r.d_clauses));
  double* dst = reinterpret_cast<double*>(tab);
  const int words = r.n_clauses * (int)(sizeof(icrl_region_clause_t) / sizeof(double));
  for (int i = tid; i < words; i += threads) dst[i] = src[i];
}

// one row, one thread: the clauses one after the other (the rows kernel; the multi-env kernel's one lane per env)
__device__ __forceinline__ float cost_region_row(const icrl_region_clause_t* tab, int n_clauses, int combine, const double* obs_row,
                                                 const float* acs_row, int O) {
  int cnt = 0;
  for (int c = 0; c < n_clauses; ++c) cnt += region_clause(tab[c], obs_row, acs_row, O) ? 1 : 0;
  if (combine == ICRL_REGION_ANY) return cnt > 0 ? 1.f : 0.f;
  if (combine == ICRL_REGION_ALL) return cnt == n_clauses ? 1.f : 0.f;
  return (float)cnt;
}

// The cost wave of the one-env-per-workgroup kernels, called where cost_fn_wave is, on the same two LDS rows: lane c evaluates clause c
// over its terms (broadcast reads of the rows), a ballot gives any / all / the count.  Every lane returns the same cost.
__device__ __forceinline__ float cost_region_wave(const icrl_region_clause_t* tab, int n_clauses, int combine, const double* obs_row,
                                                  const float* acs_row, int O) {
  const int lane = threadIdx.x & 63;
  bool t = false;
  if (lane < n_clauses) t = region_clause(tab[lane], obs_row, acs_row, O);
  const int cnt = __popcll(__ballot(t));
  if (combine == ICRL_REGION_ANY) return cnt > 0 ? 1.f : 0.f;
  if (combine == ICRL_REGION_ALL) return cnt == n_clauses ? 1.f : 0.f;
  return (float)cnt;
}

}  // namespace icrl
