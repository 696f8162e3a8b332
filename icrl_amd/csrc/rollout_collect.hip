// The fused rollouts' dispatch — gfx950: icrl_rollout_collect and its forms (_ex, _ex_mon, _batch, _batch_mon, _batch_cost, _sde), i.e.
// OnPolicyWithCostAlgorithm.collect_rollouts (ref: stable_baselines3/common/on_policy_algorithm.py:367-416) as the fewest launches the
// shapes allow.  The route ladders, the exchange workspaces, the route record and the GAE tails are here; the kernels and the
// launchers over them are in rollout.hip (declared in rollout_launch.h).
#include "rollout_launch.h"

using namespace icrl;

// =================================================================================================================
// exchange workspaces, the route record's pick word, GAE tails, the route ladders
// =================================================================================================================

// multi-env kernel: E envs per workgroup, G = ceil(N / E) workgroups per run, at most four statistics owners per workgroup
static bool multi_shape(int N, int n_stats, int* E, int* G) {
  const int gmin = (n_stats + 3) / 4;
  const int per = N / gmin;
  const char* force = getenv("ICRL_MULTI_E");      // tools only: force the envs per workgroup (4 | 8 | 16)
  if (force != nullptr && (atoi(force) == 4 || atoi(force) == 8 || atoi(force) == 16) && per >= atoi(force)) *E = atoi(force);
  else if (per >= 16 && N > 8 * 256) *E = 16;        // more than 2048 envs: 16 per workgroup keep the grid at <= 256 workgroups
  else if (per >= 8) *E = 8;
  else if (per >= 4) *E = 4;
  else return false;
  *G = (N + *E - 1) / *E;
  return *G >= gmin;
}

// the route record's word 4: the KernelPick fields that chose the instantiation of `route` (ICRL_PICK_*), nothing that it ignores;
// the <8, 8> image and MINW as the dispatch that launched it wrote them down (call this after the launch)
static int pick_bits(const KernelPick& k, int route) {
  int b = (k.small ? ICRL_PICK_SMALL : 0) | (k.analytic ? ICRL_PICK_ANALYTIC : 0) | (k.disc ? ICRL_PICK_DISC : 0) | (k.sde ? ICRL_PICK_SDE : 0) |
          (k.region ? ICRL_PICK_REGION : 0);
  if (route == ICRL_ROUTE_PER_STEP || route == ICRL_ROUTE_GENERIC_PER_STEP) return b;
  b |= k.mon ? ICRL_PICK_MON : 0;
  if (route == ICRL_ROUTE_PERSISTENT || route == ICRL_ROUTE_PERSISTENT_BATCH) b |= k.gran ? ICRL_PICK_GRAN : 0;
  if ((route == ICRL_ROUTE_MULTI || route == ICRL_ROUTE_MULTI_BATCH) && k.used_cn128) b |= ICRL_PICK_CN128;
  if (route == ICRL_ROUTE_PERSISTENT_BATCH) b |= k.used_minw << ICRL_PICK_MINW_SHIFT;
  return b;
}

// ---- exchange workspaces.  A run's workspace is the agent's xch_ws when that holds `need` bytes, else the not yet computed
// reward_advantages plane of the buffer (GAE fills it afterwards), else NULL: the route is then not taken.
static char* exchange_ws(const icrl_agent_t* ag, const icrl_buffer_t* buf, size_t need) {
  if (ag->xch_ws != nullptr && (size_t)ag->xch_ws_bytes >= need) return reinterpret_cast<char*>(ag->xch_ws);
  return (size_t)buf->T * buf->N * sizeof(float) >= need ? reinterpret_cast<char*>(buf->reward_advantages) : nullptr;
}
// where exchange_ws took `ws` from, for the route record (ICRL_WS_*)
static int ws_source(const icrl_agent_t* ag, const char* ws) {
  return ws == nullptr ? ICRL_WS_NONE : (ws == reinterpret_cast<const char*>(ag->xch_ws) ? ICRL_WS_XCH : ICRL_WS_PLANE);
}

// one-workgroup-per-env kernels (PersistArgs):  xch_obs | xch_rew | xch_cost | xch_done (to 256 B) | counter (512 B) | xg (granule mode)
// = 48 N O + 96 N + 1024 bytes at most.  persist_ws_carve returns the bytes to clear from p.counter on.
static size_t persist_ws_bytes(int N, int O, bool gran) {
  return (size_t)16 * N * O + (size_t)16 * N + (size_t)8 * N + (size_t)8 * N + 1024 + (gran ? (size_t)16 * N * (2 * O + 4) : 0);
}
static size_t persist_ws_carve(char* ws, int N, int O, bool gran, PersistArgs& p) {
  const int G = 2 * O + 4;
  char* base = ws;
  p.xch_obs = reinterpret_cast<double*>(base); base += (size_t)16 * N * O;
  p.xch_rew = reinterpret_cast<double*>(base); base += (size_t)16 * N;
  p.xch_cost = reinterpret_cast<float*>(base); base += (size_t)8 * N;
  p.xch_done = reinterpret_cast<unsigned*>(base); base += ((size_t)8 * N + 255) / 256 * 256;
  p.counter = reinterpret_cast<unsigned*>(base); base += 512;
  p.xg = reinterpret_cast<unsigned long long*>(base);
  p.g_magic = (unsigned)((1ull << 32) / (unsigned long long)(G / 2));      // index split by the records per env (obs + 2)
  return 512 + (gran ? (size_t)16 * N * G : 0);
}

// statistics partitioned by column (WideArgs: the wide and the multi kernels):  xg [2][N][2 O + 4] | sg [2][4 O + 4] | 256 spare bytes
// = 32 N O + 64 N + 64 O + 320 bytes.  with_xcc: the multi kernels' XCD ids (G <= 32 words) in the spare bytes.  wide_ws_carve
// returns the bytes to clear from p.xg on.
// Both layouts stay below ICRL_ROLLOUT_WS_BYTES(N, obs) = 48 N O + 96 N + 64 O + 2048, which the header promises for either.
static size_t wide_ws_bytes(int N, int O) { return 16 * (size_t)N * (2 * (size_t)O + 4) + 16 * (4 * (size_t)O + 4) + 256; }
static size_t wide_ws_carve(char* ws, int N, int O, bool with_xcc, WideArgs& p) {
  const size_t GX = 2 * (size_t)O + 4, GS = 4 * (size_t)O + 4;
  p.xg = reinterpret_cast<unsigned long long*>(ws);
  p.sg = p.xg + 2 * (size_t)N * GX;
  p.xcc = with_xcc ? p.sg + 2 * GS : nullptr;
  return 16 * (size_t)N * GX + 16 * GS + (p.xcc ? 256 : 0);
}

// ---- tails: the dual GAE behind a rollout (do_gae bit 0), or the rollout's error
static int finish_with_gae(int err, int do_gae, const icrl_buffer_t* buf, const icrl_agent_t* ag, double reward_gamma, double reward_gae_lambda,
                           double cost_gamma, double cost_gae_lambda, void* stream) {
  if (err || !(do_gae & 1)) return err;
  return icrl_gae_dual_ws(buf->rewards, buf->costs, buf->reward_values, buf->cost_values, buf->dones, ag->last_v_r, ag->last_v_c,
                          ag->last_dones, buf->reward_advantages, buf->cost_advantages, buf->reward_returns, buf->cost_returns, buf->T, buf->N,
                          reward_gamma, reward_gae_lambda, cost_gamma, cost_gae_lambda, 0, buf->gae_ws, buf->gae_ws_bytes, stream);
}
// dual GAE of every run in one launch; its argument blocks go behind the rollout's in args_ws (both launches are in flight together)
static int finish_batch_with_gae(int err, int do_gae, int n_runs, const icrl_rollout_job_t* jobs, double reward_gamma, double reward_gae_lambda,
                                 double cost_gamma, double cost_gae_lambda, void* args_ws, long long args_ws_bytes, void* stream) {
  if (err || !(do_gae & 1)) return err;
  if (args_ws_bytes < 2ll * n_runs * ICRL_BATCH_ARGS_BYTES)
    return fail("icrl_rollout_collect_batch: args_ws needs 2 x n_runs x ICRL_BATCH_ARGS_BYTES = %lld B when the GAE launch is included", 2ll * n_runs * ICRL_BATCH_ARGS_BYTES);
  return icrl_gae_dual_batch_impl(n_runs, jobs, reward_gamma, reward_gae_lambda, cost_gamma, cost_gae_lambda,
                                  (char*)args_ws + (size_t)n_runs * ICRL_BATCH_ARGS_BYTES, stream);
}

// Routes of a single run, in the order they are tried (-1 from a launcher, a refused cooperative launch or a missing workspace: the next one):
//   generic persistent   layers above 64 units / `arch`, cost net within the register image, !(do_gae & 2), N <= 128, N obs <= 4096,
//                        granule mode, transposed weights                                      rollout_generic_kernel
//   generic per-step     every other generic shape: four launches per step                      policy_generic | cn_cost_rows | act_step_generic | norm_step
//   multi                do_gae & 32 or N > 1024 or a Point env at N <= 96; !(do_gae & 2), training, Box actions, multi_shape, workspace      rollout_multi[_analytic]_kernel
//   wide                 !(do_gae & 2), training, N > 96 or N obs > 4096 or do_gae & 16, N <= 1024, <= WIDE_E envs per workgroup,
//                        grid >= obs + 2, workspace                                             rollout_wide_kernel
//   persistent           !(do_gae & 2), not a Point env, N <= 128, N obs <= 4096, workspace       rollout_persistent_kernel
//   per-step             everything else: two launches per step                                 act_step_kernel | norm_step
//                        (with training statistics and Box actions that is: fewer envs than multi / wide take AND more than persistent takes —
//                        AntWall, obs 113, at 37..114 envs: 37 x 113 > 4096, 114 < obs + 2 workgroups, 114 / 29 < 4 envs per owner group — and Point
//                        envs below 12; with frozen statistics or Discrete actions: above 128 envs or 4096 observation doubles)
// A discriminator cost (icrl_cost_disc_t, cost_fn.h) takes the route its inner net would take as a constraint net, on every rung, in that
// rung's D form (rollout_generic_disc_kernel, rollout_multi_net_as_discriminator_kernel, rollout_persistent_disc_kernel; wide and per-step:
// the kernel instantiated with CIT | CIT_DISC; generic per-step: cn_cost_rows / cost_forward with mode 1);
// the phase-timer bits of do_gae are ignored with one, and ICRL_PICK_DISC is set in the record.
// What a call took is kept per host thread: icrl_debug_last_route (errors.hip), written where a route returns after its launch.
// Routes of a batch (rollout_collect_batch_impl):
//   multi                !ICRL_BATCH_NO_MULTI, not `few`, Box actions, training, multi_shape, every run has a workspace      rollout_multi_batch[_analytic]_kernel
//   persistent           N <= 128, N obs <= 4096 (else refused)                                 rollout_persistent_batch[_analytic]_kernel
extern "C" int icrl_rollout_collect_ex_mon(const icrl_env_t* env, const icrl_norm_t* nm, const icrl_policy_t* pol,
                                           const icrl_costnet_t* cn_arg, const icrl_buffer_t* buf, const icrl_agent_t* ag,
                                           const float* noise, const float* action_low, const float* action_high,
                                           double reward_gamma, double reward_gae_lambda, double cost_gamma, double cost_gae_lambda,
                                           int do_gae, const icrl_monitor_t* mon, void* stream) {
  note_route(ICRL_FAMILY_ROLLOUT);      // (route 0 until a ladder rung below has launched)
  double* raw_plane = nullptr;
  if (int e = mon_plane("icrl_rollout_collect_ex_mon", mon, &raw_plane)) return e;
  const int N = env->n_envs, O = env->obs_dim, T = buf->T;
  // an analytic cost (icrl_cost_fn_t behind the constraint-net pointer): `cn` stays the "this chain has a cost" flag, `net` is the
  // constraint net proper (NULL then) — only `net` is ever read as an icrl_costnet_t
  const icrl_cost_fn_t* const cf = as_cost_fn(cn_arg);
  if (cf != nullptr)
    if (int e = cost_fn_check("icrl_rollout_collect", cf, O, pol->discrete ? 0 : pol->act_dim, pol->discrete ? 1 : 0)) return e;
  // a discriminator cost (icrl_cost_disc_t): `net` is its inner net, checked and routed below as a constraint net is; k.disc picks
  // the kernels whose cost wave returns zeta
  const icrl_cost_disc_t* const cd = as_cost_disc(cn_arg);
  if (cd != nullptr)
    if (int e = cost_disc_check("icrl_rollout_collect", cd)) return e;
  // a region cost (icrl_cost_region_t): checked on its host table here, the CIT == 0 image with the region cost wave below (k.region)
  const icrl_cost_region_t* const cr = as_cost_region(cn_arg);
  if (cr != nullptr) {
    if (int e = cost_region_check("icrl_rollout_collect", cr, O, pol->discrete ? 0 : pol->act_dim, pol->discrete ? 1 : 0)) return e;
    if (policy_is_wide(pol))
      return fail("icrl_rollout_collect: a region cost descriptor (icrl_cost_region_t) beside a generic-shape policy is not served: the "
                  "generic-shape rollout kernels have no region form");
  }
  const icrl_costnet_t* const net = (cf != nullptr || cr != nullptr) ? nullptr : (cd != nullptr ? cd->net : cn_arg);
  const bool cn = cn_arg != nullptr;
  const bool generic = policy_is_wide(pol) || (net != nullptr && costnet_is_wide(net));      // shapes of the generic-shape path: per-step launches
  if (!generic && !dims_ok(pol)) return bad_dims("icrl_rollout_collect", pol);
  if (pol->obs_dim != O || buf->N != N || buf->obs_dim != O)
    return fail("icrl_rollout_collect: env (%d envs, obs_dim %d) vs policy obs_dim %d vs buffer (%d envs, obs_dim %d)", N, O, pol->obs_dim, buf->N, buf->obs_dim);
  if (!generic && net != nullptr && !cn_ok(net)) return bad_cn("icrl_rollout_collect", net);
  if (N > NORM_MAX_N)
    return fail("icrl_rollout_collect: %d envs on one GPU, limit %d (shard the envs over ranks: the float64 normaliser statistics are one "
                "numpy-ordered chain per column)", N, NORM_MAX_N);
  hipStream_t s = (hipStream_t)stream;
  KernelPick k;
  k.small = small_shape(O, net); k.analytic = cf != nullptr; k.disc = cd != nullptr; k.region = cr != nullptr; k.mon = raw_plane != nullptr;
  auto finish = [&](int err) { return finish_with_gae(err, do_gae, buf, ag, reward_gamma, reward_gae_lambda, cost_gamma, cost_gae_lambda, stream); };
  // the route record, written where a rung returns after its launch(es): workspace source, working workgroups, envs per workgroup, packed, launches
  auto routed = [&](int err, int route, const char* ws, int wgs, int E, int packed, int launches) {
    if (err == 0) note_route(ICRL_FAMILY_ROLLOUT, route, ws_source(ag, ws), wgs, E, pick_bits(k, route), packed, 1, launches);
    return err;
  };
  if (generic) {
    // a policy with layers above 64 units / an `arch` descriptor, or a constraint net above 64 units / two layers: the reference's
    // per-step loop as four launches per step on this stream — policy_generic_kernel (generic.hip), cn_cost_rows_kernel (cn_train.hip),
    // act_step_generic_kernel, the normaliser — no host work in between
    if (O > MAX_OBS || env->act_dim > MAX_ACT || T < 1)
      return fail("icrl_rollout_collect (generic-shape path): obs_dim %d (<= %d), act_dim %d (<= %d), T = %d", O, MAX_OBS, env->act_dim, MAX_ACT, T);
    if (buf->act_store != (pol->discrete ? 1 : pol->act_dim) || (!pol->discrete && env->act_dim != pol->act_dim))
      return fail("icrl_rollout_collect (generic-shape path): buffer act_store %d / env act_dim %d vs policy act_dim %d (discrete: act_store 1)",
                  buf->act_store, env->act_dim, pol->act_dim);
    // ONE persistent launch (rollout_generic_kernel: the loop of rollout_persistent_kernel around the table-driven forward) when the
    // shapes are those of the one-workgroup-per-env kernel and the constraint net fits its register image; do_gae & 2 forces the per-step launches
    if (policy_is_wide(pol) && (net == nullptr || (!costnet_is_wide(net) && cn_ok(net))) && !(do_gae & 2) && N <= 128 && N * O <= NORM_CHUNK &&
        O * env->act_dim <= MAX_OBS * MAX_ACT && (size_t)N * (2 * O + 4) <= (size_t)256 * GRAN_MAX && pol->params_t != nullptr) {
      GenRolloutArgs ga;
      if (int e = make_gen_net(pol, &ga.net, "icrl_rollout_collect")) return e;
      ga.P = pol->params;
      char* ws = exchange_ws(ag, buf, persist_ws_bytes(N, O, true));      // (granule mode: the condition above)
      if (ws != nullptr) {
        PersistArgs& p = ga.p;
        fill_act_args(p.act, env, buf, ag, pol, true, net, cf, noise, action_low, action_high, raw_plane);
        p.nm = *nm; p.T = T; p.prof = (do_gae & 4) != 0;
        const size_t clear = persist_ws_carve(ws, N, O, true, p);
        hipError_t e = hipMemsetAsync(p.counter, 0, clear, s);
        if (e != hipSuccess) return (int)e;
        const size_t dyn = persist_dyn_lds(N, O, env->act_dim);
        const int perr = launch_rollout_generic(k, N, dyn, s, ga);
        if (perr >= 0) return finish(routed(perr != 0 ? perr : (int)hipGetLastError(), ICRL_ROUTE_GENERIC_PERSISTENT, ws, N, 1, 0, 1));
      }
    }
    GenStepArgs g;
    g.env = *env; g.buf = *buf; g.ag = *ag; g.has_cn = cf != nullptr ? 2 : (cn ? 1 : 0); g.raw_plane = raw_plane;
    g.cf = cf != nullptr ? *cf : icrl_cost_fn_t{};      // (the analytic cost is evaluated inside act_step_generic_kernel: no cost launch)
    const int AS = buf->act_store;
    for (int t = 0; t < T; ++t) {
      const size_t row = (size_t)t * N;
      int err = policy_is_wide(pol)
          ? launch_policy_generic(pol, ag->last_obs, noise ? noise + row * AS : nullptr, N, 0, action_low, action_high, buf->actions + row * AS, ag->act_clipped,
                                  buf->reward_values + row, buf->cost_values + row, buf->log_probs + row, nullptr, nullptr, s)
          : icrl_policy_forward(pol, ag->last_obs, noise ? noise + row * AS : nullptr, N, 0, action_low, action_high, buf->actions + row * AS, ag->act_clipped,
                                buf->reward_values + row, buf->cost_values + row, buf->log_probs + row, stream);
      if (err) return err;
      if (net != nullptr) {
        err = icrl_cost_mlp_forward(cn_arg, env->s, ag->act_clipped, N, ag->raw_cost, stream);      // (a discriminator descriptor: D)
        if (err) return err;
      }
      launch_act_step_generic(N, s, g, t);
      NormStepArgs b{*nm, env->s, ag->raw_rew, cn ? ag->raw_cost : nullptr, ag->dones, N, O, ag->last_obs, nullptr, nullptr,
                     buf->new_observations + row * O, buf->rewards + row, buf->costs + row, ag->last_dones};
      launch_norm_step(b, s);
    }
    return finish(routed((int)hipGetLastError(), ICRL_ROUTE_GENERIC_PER_STEP, nullptr, N, 0, 0, (net != nullptr ? 4 : 3) * T));
  }
  ActStepArgs a;
  fill_act_args(a, env, buf, ag, pol, false, net, cf, noise, action_low, action_high, raw_plane);
  if (cr != nullptr) { a.cr = *cr; a.has_cn = 1; }      // (the descriptor in the analytic cost's bytes; the kernels read n_clauses, combine, d_clauses)
  // several environments per workgroup, interleaved (rollout_multi_kernel): do_gae bit 5
  // (the Point envs at the sizes of the one-workgroup-per-env kernel come here too: that kernel is built without their step, env_step_wave)
  const bool point = env->reward_form >= 4;
  if (((do_gae & 32) || N > WIDE_MAX_N || (point && N <= 96 && !(do_gae & 16))) && !(do_gae & 2) && nm->training && !pol->discrete && N <= NORM_MAX_N && T >= 1) {
    int E = 0, G = 0;
    const int n_stats = O + (cn ? 2 : 1);
    char* ws = exchange_ws(ag, buf, wide_ws_bytes(N, O));
    if (multi_shape(N, n_stats, &E, &G) && ws != nullptr) {
      WideArgs p;
      p.act = a; p.nm = *nm; p.T = T; p.G = G; p.prof = (do_gae & 4) ? 1 : ((do_gae & 8) ? G : 0);
      const size_t clear = wide_ws_carve(ws, N, O, G <= 32, p);
      hipError_t e = hipMemsetAsync(p.xg, 0, clear, s);
      if (e != hipSuccess) return (int)e;
      k.cn128 = !net || net->in_dim <= 128; k.E = E;
      const size_t mdyn = multi_dyn_lds(N, O, env->act_dim, (n_stats + G - 1) / G);
      int packed = 0;
      const int err = launch_rollout_multi(k, p, G, mdyn, s, &packed);
      if (err >= 0) return finish(routed(err, ICRL_ROUTE_MULTI, ws, G, E, packed, 1));
    }
  }
  // many environments: persistent launch with the statistics partitioned by observation column (rollout_wide_kernel); measured
  // against the replicated-statistics kernel at HC widths: 64 envs 9.6 vs 9.5 us per step, 128 envs 9.9 vs 13.9
  if (!(do_gae & 2) && nm->training && (N > 96 || N * O > NORM_CHUNK || (do_gae & 16)) && N <= WIDE_MAX_N && O * env->act_dim <= MAX_OBS * MAX_ACT && T >= 1) {
    int dev = 0, cus = 0, per_cu = 0;
    k.prof = false;      // (the occupancy has always been asked of the instantiation without phase timers)
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
        rollout_wide_blocks_per_cu(k, &per_cu) == (int)hipSuccess &&
        per_cu > 0) {
      const int max_g = per_cu * cus;
      const int E = (N + max_g - 1) / max_g;                 // envs per workgroup
      const int G = (N + E - 1) / E;                         // balanced grid
      char* ws = exchange_ws(ag, buf, wide_ws_bytes(N, O));
      if (getenv("ICRL_DEBUG")) fprintf(stderr, "icrl_rollout_collect: wide persistent kernel N=%d obs=%d: %d workgroup(s) per CU x %d CUs -> E=%d envs per workgroup, grid %d\n", N, O, per_cu, cus, E, G);
      if (E <= WIDE_E && G >= O + 2 && ws != nullptr) {
        WideArgs p;
        p.act = a; p.nm = *nm; p.T = T; p.G = G; p.prof = (do_gae & 4) ? 1 : ((do_gae & 8) ? G : 0);
        const size_t clear = wide_ws_carve(ws, N, O, false, p);
        hipError_t e = hipMemsetAsync(p.xg, 0, clear, s);
        if (e != hipSuccess) return (int)e;
        if (k.mon || k.analytic || k.disc || k.region) p.prof = 0;      // (with the plane, an analytic, a discriminator or a region cost: the instantiations without phase timers)
        k.prof = p.prof != 0;
        const int err = launch_rollout_wide(k, G, s, p);
        if (err == (int)hipErrorCooperativeLaunchTooLarge) { (void)hipGetLastError(); goto per_step; }
        return finish(routed(err, ICRL_ROUTE_WIDE, ws, G, E, 0, 1));
      }
    }
  }
  // persistent path: one launch for all T steps (see rollout_persistent_kernel).  do_gae & 2 forces the per-step launches.
  {
    const bool gran = (size_t)N * (2 * O + 4) <= (size_t)256 * GRAN_MAX;
    char* ws = exchange_ws(ag, buf, persist_ws_bytes(N, O, gran));
    if (!(do_gae & 2) && !point && N <= 128 && N * O <= NORM_CHUNK && O * env->act_dim <= MAX_OBS * MAX_ACT && T >= 1 && ws != nullptr) {
      PersistArgs p;
      p.act = a; p.nm = *nm; p.T = T; p.prof = (do_gae & 4) != 0;
      const size_t clear = persist_ws_carve(ws, N, O, gran, p);
      hipError_t e = hipMemsetAsync(p.counter, 0, clear, s);
      if (e != hipSuccess) return (int)e;
      if (k.mon || k.analytic || k.disc || k.region) p.prof = 0;      // (with the plane, an analytic, a discriminator or a region cost: the instantiations without phase timers)
      k.gran = gran; k.prof = p.prof != 0;
      const size_t dyn = persist_dyn_lds(N, O, env->act_dim);
      const int perr = launch_rollout_persistent(k, N, dyn, s, p);
      const int err = perr > 0 ? perr : (int)hipGetLastError();
      if (perr < 0) goto per_step;
      return finish(routed(err, ICRL_ROUTE_PERSISTENT, ws, N, 1, 0, 1));
    }
  }
per_step:
  for (int t = 0; t < T; ++t) {
    launch_act_step(k, N, s, a, t);
    const size_t row = (size_t)t * N;
    NormStepArgs b{*nm, env->s, ag->raw_rew, cn ? ag->raw_cost : nullptr, ag->dones, N, O, ag->last_obs, nullptr, nullptr,
                   buf->new_observations + row * O, buf->rewards + row, buf->costs + row, ag->last_dones};
    launch_norm_step(b, s);
  }
  return finish(routed((int)hipGetLastError(), ICRL_ROUTE_PER_STEP, nullptr, N, 0, 0, 2 * T));
}

// what one run of a batch must share with run 0 and satisfy by itself.  same_training is inherited, not designed: the multi route also
// compares nm->training between the runs, the one-workgroup-per-env route does not
static int batch_run_check(int r, const icrl_rollout_job_t& j, const icrl_rollout_job_t& j0, bool analytic, bool same_training) {
  const int N = j0.env->n_envs, O = j0.env->obs_dim;
  const bool has_cn = j0.cn != nullptr;
  if (j.env->n_envs != N || j.env->obs_dim != O || j.env->act_dim != j0.env->act_dim || j.buf->T != j0.buf->T || j.buf->N != N ||
      j.pol->obs_dim != O || j.pol->act_dim != j0.pol->act_dim || j.pol->discrete != j0.pol->discrete || (j.cn != nullptr) != has_cn ||
      (has_cn && (j.cn->in_dim != j0.cn->in_dim || j.cn->n_hidden != j0.cn->n_hidden)) || (same_training && j.nm->training != j0.nm->training))
    return fail("icrl_rollout_collect_batch: run %d differs from run 0 in a shape (envs / obs / act / T / discrete / constraint net)", r);
  if (!dims_ok(j.pol)) return bad_dims("icrl_rollout_collect_batch", j.pol);
  if (j.buf->obs_dim != O) return fail("icrl_rollout_collect_batch: run %d: buffer obs_dim %d vs env %d", r, j.buf->obs_dim, O);
  if (!analytic && j.cn != nullptr && !cn_ok(j.cn)) return bad_cn("icrl_rollout_collect_batch", j.cn);
  return 0;
}

// fill_act_args for run r of a batch (its monitor plane from mons[r])
static int batch_act_args(ActStepArgs& a, int r, const icrl_rollout_job_t& j, const icrl_monitor_t* mons, bool analytic, const float* action_low,
                          const float* action_high) {
  double* raw_plane = nullptr;
  if (int e = mon_plane("icrl_rollout_collect_batch_mon", mons ? mons + r : nullptr, &raw_plane)) return e;
  fill_act_args(a, j.env, j.buf, j.ag, j.pol, false, analytic ? nullptr : j.cn, analytic ? as_cost_fn(j.cn) : nullptr, j.noise, action_low, action_high,
                raw_plane);
  return 0;
}

// icrl_rollout_collect for n_runs runs: ONE persistent launch + ONE batched dual-GAE launch.  Shapes that neither batched kernel
// serves are refused (the caller then issues the single-run calls).
// analytic: every jobs[r].cn is an icrl_cost_fn_t that passed cost_fn_check (icrl_rollout_collect_batch_cost) — the CIT == 0 kernels;
// otherwise every jobs[r].cn is a constraint net, or NULL in every run
static int rollout_collect_batch_impl(int n_runs, const icrl_rollout_job_t* jobs, const icrl_monitor_t* mons, const float* action_low,
                                      const float* action_high, double reward_gamma, double reward_gae_lambda, double cost_gamma,
                                      double cost_gae_lambda, int do_gae, void* args_ws, long long args_ws_bytes, void* stream, bool analytic) {
  static_assert(sizeof(PersistArgs) <= ICRL_BATCH_ARGS_BYTES, "ICRL_BATCH_ARGS_BYTES");
  static_assert(sizeof(WideArgs) <= ICRL_BATCH_ARGS_BYTES, "ICRL_BATCH_ARGS_BYTES");
  if (args_ws == nullptr || args_ws_bytes < (long long)n_runs * ICRL_BATCH_ARGS_BYTES)
    return fail("icrl_rollout_collect_batch: args_ws holds %lld B, %d runs need %lld", args_ws_bytes, n_runs, (long long)n_runs * ICRL_BATCH_ARGS_BYTES);
  hipStream_t s = (hipStream_t)stream;
  const icrl_rollout_job_t& j0 = jobs[0];
  const int N = j0.env->n_envs, O = j0.env->obs_dim, T = j0.buf->T;
  const bool has_cn = j0.cn != nullptr;
  const icrl_costnet_t* const net0 = analytic ? nullptr : j0.cn;
  KernelPick k;
  k.small = small_shape(O, net0); k.analytic = analytic; k.mon = mons != nullptr;
  auto finish = [&](int err) {
    return finish_batch_with_gae(err, do_gae, n_runs, jobs, reward_gamma, reward_gae_lambda, cost_gamma, cost_gae_lambda, args_ws, args_ws_bytes, stream);
  };
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 256;
  // ---- preferred: several envs per workgroup, interleaved (G = N / E workgroups per run: all runs resident together)
  {
    int E = 0, G = 0;
    const int n_stats = O + (has_cn ? 2 : 1);
    static const bool no_multi = getenv("ICRL_BATCH_NO_MULTI") != nullptr;      // tools: the one-workgroup-per-env kernel instead
    // (few small runs: one workgroup per env keeps every env's step at its latency floor and all of them fit the chip at once)
    const bool few = (long long)n_runs * N <= cus && N <= 128 && N * O <= NORM_CHUNK;
    if (!no_multi && !few && !j0.pol->discrete && j0.nm->training && N <= NORM_MAX_N && T >= 1 && multi_shape(N, n_stats, &E, &G)) {
      WideArgs* d_args = (WideArgs*)args_ws;
      bool ok = true;
      int src = ICRL_WS_NONE;      // (of the last run: the record has one word for it)
      for (int r = 0; r < n_runs && ok; ++r) {
        const icrl_rollout_job_t& j = jobs[r];
        if (int e_ = batch_run_check(r, j, j0, analytic, true)) return e_;
        char* ws = exchange_ws(j.ag, j.buf, wide_ws_bytes(N, O));
        if (ws == nullptr) { ok = false; break; }
        src = ws_source(j.ag, ws);
        WideArgs p;
        if (int e_ = batch_act_args(p.act, r, j, mons, analytic, action_low, action_high)) return e_;
        p.nm = *j.nm; p.T = T; p.G = G; p.prof = 0;
        const size_t clear = wide_ws_carve(ws, N, O, G <= 32, p);
        hipError_t e = hipMemsetAsync(p.xg, 0, clear, s);
        if (e != hipSuccess) return (int)e;
        const int pe = put_rollout_args(p, d_args + r, s);
        if (pe) return pe;
      }
      if (ok) {
        k.cn128 = net0 == nullptr || net0->in_dim <= 128; k.E = E;
        const size_t mdyn = multi_dyn_lds(N, O, j0.env->act_dim, (n_stats + G - 1) / G);
        int packed = 0;
        const int err = launch_rollout_multi_batch(k, d_args, n_runs, G, mdyn, s, &packed);
        if (err == 0) note_route(ICRL_FAMILY_ROLLOUT, ICRL_ROUTE_MULTI_BATCH, src, G, E, pick_bits(k, ICRL_ROUTE_MULTI_BATCH), packed, n_runs, 1);
        if (err >= 0) return finish(err);
      }
    }
  }
  // ---- one workgroup per env: grid (N, n_runs), run = blockIdx.y (N <= 128 and N x obs <= 4096: BASELINE configs[1])
  if (!(N <= 128 && N * O <= NORM_CHUNK && O * j0.env->act_dim <= MAX_OBS * MAX_ACT && T >= 1))
    return fail("icrl_rollout_collect_batch: %d envs x obs %d: no batched form for this shape (multi-env kernel: continuous actions, training statistics, >= 4 envs per statistics-owner group; one workgroup per env: <= 128 envs, envs x obs <= %d)", N, O, NORM_CHUNK);
  const bool gran = (size_t)N * (2 * O + 4) <= (size_t)256 * GRAN_MAX;
  const size_t need = persist_ws_bytes(N, O, gran);
  PersistArgs* d_args = (PersistArgs*)args_ws;
  int src = ICRL_WS_NONE;
  for (int r = 0; r < n_runs; ++r) {
    const icrl_rollout_job_t& j = jobs[r];
    if (int e_ = batch_run_check(r, j, j0, analytic, false)) return e_;
    char* ws = exchange_ws(j.ag, j.buf, need);
    if (ws == nullptr) return fail("icrl_rollout_collect_batch: run %d: exchange workspace of %zu B needed (icrl_agent_t.xch_ws, ICRL_ROLLOUT_WS_BYTES)", r, need);
    src = ws_source(j.ag, ws);
    PersistArgs p;
    if (int e_ = batch_act_args(p.act, r, j, mons, analytic, action_low, action_high)) return e_;
    p.nm = *j.nm; p.T = T; p.prof = 0;
    const size_t clear = persist_ws_carve(ws, N, O, gran, p);
    hipError_t e = hipMemsetAsync(p.counter, 0, clear, s);
    if (e != hipSuccess) return (int)e;
    const int pe = put_rollout_args(p, d_args + r, s);
    if (pe) return pe;
  }
  // ICRL_ROLLOUT_MINW (tools) picks the register allocation; otherwise the full register file per workgroup when all workgroups of
  // the grid fit one per CU — up to 4 runs of 64 envs: 17 ms per 2048-step rollout against 29.6 with the two-per-CU allocation,
  // measured at S = 1 and 4
  static const int minw_env = getenv("ICRL_ROLLOUT_MINW") ? atoi(getenv("ICRL_ROLLOUT_MINW")) : 0;
  k.gran = gran; k.minw = minw_env > 0 ? minw_env : ((long long)n_runs * N <= cus ? 1 : 2);
  const size_t dyn = persist_dyn_lds(N, O, j0.env->act_dim);
  const int err = launch_rollout_persistent_batch(k, N, n_runs, dyn, s, d_args);
  if (err == 0) note_route(ICRL_FAMILY_ROLLOUT, ICRL_ROUTE_PERSISTENT_BATCH, src, N, 1, pick_bits(k, ICRL_ROUTE_PERSISTENT_BATCH), 0, n_runs, 1);
  return finish(err);
}

extern "C" int icrl_rollout_collect_batch_mon(int n_runs, const icrl_rollout_job_t* jobs, const icrl_monitor_t* mons, const float* action_low,
                                              const float* action_high, double reward_gamma, double reward_gae_lambda, double cost_gamma,
                                              double cost_gae_lambda, int do_gae, void* args_ws, long long args_ws_bytes, void* stream) {
  note_route(ICRL_FAMILY_ROLLOUT);      // (the one clear of a batched call: rollout_collect_batch_impl below writes the record behind its launch)
  if (n_runs < 1 || n_runs > 65535) return fail("icrl_rollout_collect_batch: n_runs = %d (1..65535)", n_runs);
  for (int r = 0; r < n_runs; ++r)      // (the analytic form is icrl_rollout_collect_batch_cost's)
    if (as_cost_fn(jobs[r].cn)) return refuse_cost_fn("icrl_rollout_collect_batch");
  for (int r = 0; r < n_runs; ++r)
    if (as_cost_disc(jobs[r].cn)) return refuse_cost_disc("icrl_rollout_collect_batch");
  for (int r = 0; r < n_runs; ++r)
    if (as_cost_region(jobs[r].cn)) return refuse_cost_region("icrl_rollout_collect_batch");
  return rollout_collect_batch_impl(n_runs, jobs, mons, action_low, action_high, reward_gamma, reward_gae_lambda, cost_gamma, cost_gae_lambda, do_gae,
                                    args_ws, args_ws_bytes, stream, false);
}

// icrl_rollout_collect_batch_mon for runs against a FIXED cost (cpg seed batches): behind jobs[r].cn a constraint net in every run, NULL
// in every run (both: exactly icrl_rollout_collect_batch_mon) or an analytic descriptor in every run (the CIT == 0 batched kernels; the
// runs may differ in the descriptor's kind and values).  Everything is checked on the host before the first device call.
extern "C" int icrl_rollout_collect_batch_cost(int n_runs, const icrl_rollout_job_t* jobs, const icrl_monitor_t* mons, const float* action_low,
                                               const float* action_high, double reward_gamma, double reward_gae_lambda, double cost_gamma,
                                               double cost_gae_lambda, int do_gae, void* args_ws, long long args_ws_bytes, void* stream) {
  note_route(ICRL_FAMILY_ROLLOUT);
  if (n_runs < 1 || n_runs > 65535) return fail("icrl_rollout_collect_batch_cost: n_runs = %d (1..65535)", n_runs);
  int n_fn = 0, n_net = 0;
  for (int r = 0; r < n_runs; ++r) {
    if (as_cost_disc(jobs[r].cn)) return refuse_cost_disc("icrl_rollout_collect_batch_cost");
    if (as_cost_region(jobs[r].cn)) return refuse_cost_region("icrl_rollout_collect_batch_cost");
    if (as_cost_fn(jobs[r].cn)) ++n_fn;
    else if (jobs[r].cn != nullptr) ++n_net;
  }
  if (n_fn != 0 && n_fn != n_runs)
    return fail("icrl_rollout_collect_batch_cost: %d of %d runs carry an analytic cost, %d a constraint net, %d none: a batch is one kernel, so "
                "every run carries an analytic descriptor, or none does", n_fn, n_runs, n_net, n_runs - n_fn - n_net);
  for (int r = 0; r < n_fn; ++r) {
    const icrl_rollout_job_t& j = jobs[r];
    if (int e = cost_fn_check("icrl_rollout_collect_batch_cost", as_cost_fn(j.cn), j.env->obs_dim, j.pol->discrete ? 0 : j.pol->act_dim, j.pol->discrete ? 1 : 0)) return e;
  }
  return rollout_collect_batch_impl(n_runs, jobs, mons, action_low, action_high, reward_gamma, reward_gae_lambda, cost_gamma, cost_gae_lambda, do_gae,
                                    args_ws, args_ws_bytes, stream, n_fn != 0);
}

extern "C" int icrl_rollout_collect_ex(const icrl_env_t* env, const icrl_norm_t* nm, const icrl_policy_t* pol,
                                       const icrl_costnet_t* cn, const icrl_buffer_t* buf, const icrl_agent_t* ag,
                                       const float* noise, const float* action_low, const float* action_high,
                                       double reward_gamma, double reward_gae_lambda, double cost_gamma, double cost_gae_lambda,
                                       int do_gae, void* stream) {
  return icrl_rollout_collect_ex_mon(env, nm, pol, cn, buf, ag, noise, action_low, action_high, reward_gamma, reward_gae_lambda,
                                     cost_gamma, cost_gae_lambda, do_gae, nullptr, stream);
}

extern "C" int icrl_rollout_collect_batch(int n_runs, const icrl_rollout_job_t* jobs, const float* action_low, const float* action_high,
                                          double reward_gamma, double reward_gae_lambda, double cost_gamma, double cost_gae_lambda,
                                          int do_gae, void* args_ws, long long args_ws_bytes, void* stream) {
  return icrl_rollout_collect_batch_mon(n_runs, jobs, nullptr, action_low, action_high, reward_gamma, reward_gae_lambda, cost_gamma,
                                        cost_gae_lambda, do_gae, args_ws, args_ws_bytes, stream);
}

extern "C" int icrl_rollout_collect(const icrl_env_t* env, const icrl_norm_t* nm, const icrl_policy_t* pol,
                                    const icrl_costnet_t* cn, const icrl_buffer_t* buf, const icrl_agent_t* ag,
                                    const float* noise, const float* action_low, const float* action_high,
                                    double reward_gamma, double reward_gae_lambda, double cost_gamma, double cost_gae_lambda,
                                    void* stream) {
  return icrl_rollout_collect_ex(env, nm, pol, cn, buf, ag, noise, action_low, action_high, reward_gamma, reward_gae_lambda,
                                 cost_gamma, cost_gae_lambda, 1, stream);
}

// ---- the rollout of a gSDE agent.  The matrices `expl` are drawn by the caller before the launch, in the order of the per-step loop
// (ActorTwoCriticsPolicy.noise_schedule).  Routes, in the order they are tried:
//   persistent   !(do_gae & 2), not a Point env, N <= 128, N obs <= 4096, workspace, co-resident      rollout_persistent_sde_kernel
//   per-step     everything else: two launches per step                                              act_step_sde_kernel | norm_step
// The multi-env and column-partitioned kernels have no gSDE form.  Every refusal is made on the host before any device call.
extern "C" int icrl_rollout_collect_sde(const icrl_env_t* env, const icrl_norm_t* nm, const icrl_policy_t* pol, const icrl_costnet_t* cn_arg,
                                        const icrl_buffer_t* buf, const icrl_agent_t* ag, const float* expl, int n_draws, int sample_freq,
                                        const float* action_low, const float* action_high, double reward_gamma, double reward_gae_lambda,
                                        double cost_gamma, double cost_gae_lambda, int do_gae, void* stream) {
  const char* who = "icrl_rollout_collect_sde";
  note_route(ICRL_FAMILY_ROLLOUT);
  if (env == nullptr || nm == nullptr || pol == nullptr || buf == nullptr || ag == nullptr || expl == nullptr)
    return fail("%s: NULL argument (env, nm, pol, buf, ag and expl are required)", who);
  if (as_cost_region(cn_arg) != nullptr) return refuse_cost_region(who);      // (the gSDE kernels have no region form)
  if (pol->params == nullptr || pol->params_t == nullptr) return fail("%s: NULL argument (pol->params and pol->params_t are required)", who);
  if ((action_low == nullptr) != (action_high == nullptr)) return fail("%s: NULL argument (action_low and action_high: both or neither)", who);
  if (pol->discrete) return fail("%s: a discrete policy has no gSDE head", who);
  if (pol->arch != nullptr || pol->h1 != MAX_H || pol->h2 != MAX_H)
    return fail("%s: hidden widths (%d, %d)%s; the gSDE rollout serves the fast kind: two hidden layers per branch, stored %d x %d, no `arch`", who, pol->h1,
                pol->h2, pol->arch != nullptr ? " with an `arch` descriptor" : "", MAX_H, MAX_H);
  if (pol->obs_dim < 1 || pol->obs_dim > MAX_OBS || pol->act_dim < 1 || pol->act_dim > MAX_ACT)
    return fail("%s: policy obs_dim %d (1..%d), act_dim %d (1..%d)", who, pol->obs_dim, MAX_OBS, pol->act_dim, MAX_ACT);
  const int n_diag = make_pol_layout(pol->obs_dim, pol->act_dim, pol->h1, pol->h2, 0).n, n_sde = make_sde_layout(pol->obs_dim, pol->act_dim, pol->h1, pol->h2).n;
  if (pol->n_params != n_sde)
    return fail("%s: n_params %d, the gSDE (log_std [%d, act_dim]) layout of (%d, %d, %d, %d) has %d%s", who, pol->n_params, MAX_H, pol->obs_dim, pol->act_dim,
                pol->h1, pol->h2, n_sde, pol->n_params == n_diag ? " (that is the diagonal layout's count: icrl_rollout_collect_ex serves that policy)" : "");
  const int N = env->n_envs, O = env->obs_dim, A = pol->act_dim, T = buf->T;
  if (pol->obs_dim != O || env->act_dim != A || buf->N != N || buf->obs_dim != O || buf->act_store != A || N < 1 || T < 1)
    return fail("%s: env (%d envs, obs_dim %d, act_dim %d) vs policy (obs_dim %d, act_dim %d) vs buffer (T = %d, %d envs, obs_dim %d, act_store %d)", who, N, O,
                env->act_dim, pol->obs_dim, A, T, buf->N, buf->obs_dim, buf->act_store);
  if (N > NORM_MAX_N)
    return fail("%s: %d envs on one GPU, limit %d (shard the envs over ranks: the float64 normaliser statistics are one numpy-ordered chain per column)", who,
                N, NORM_MAX_N);
  if (sample_freq == 0) return fail("%s: sample_freq 0 (> 0: a draw every sample_freq steps; < 0: one draw for the rollout)", who);
  const int need_draws = sample_freq > 0 ? (T + sample_freq - 1) / sample_freq : 1;
  if (n_draws < need_draws) return fail("%s: n_draws %d, T = %d steps at sample_freq %d use %d", who, n_draws, T, sample_freq, need_draws);
  if (do_gae & ~3) return fail("%s: do_gae %d (bit 0: the dual GAE behind the rollout, bit 1: the per-step launches; no other bit is served)", who, do_gae);
  const icrl_cost_fn_t* const cf = as_cost_fn(cn_arg);
  if (cf != nullptr)
    if (int e = cost_fn_check(who, cf, O, A, 0)) return e;
  if (as_cost_disc(cn_arg) != nullptr)
    return fail("%s: a discriminator cost descriptor (icrl_cost_disc_t) is not served: the gSDE kernels have no discriminator form", who);
  const icrl_costnet_t* const net = cf != nullptr ? nullptr : cn_arg;
  if (net != nullptr && (costnet_is_wide(net) || !cn_ok(net)))
    return fail("%s: a generic-shape constraint net (in_dim %d, %d hidden layers of (%d, %d), obs_dim %d, acs_dim %d) is not served: one or two hidden layers of "
                "up to %d units, in_dim <= %d", who, net->in_dim, net->n_hidden, net->h1, net->h2, net->obs_dim, net->acs_dim, MAX_H, MAX_CN_IN);
  const bool cn = cn_arg != nullptr;
  hipStream_t s = (hipStream_t)stream;
  KernelPick k;
  k.small = small_shape(O, net); k.analytic = cf != nullptr; k.sde = true;
  // the network alone, as launch_policy_forward_sde reads it: the diagonal layout, its transposes behind the matrix's first 63 rows
  icrl_policy_t netpol = *pol;
  netpol.params_t = pol->params_t + (MAX_H - 1) * A;
  ActStepArgs a;
  fill_act_args(a, env, buf, ag, &netpol, false, net, cf, nullptr, action_low, action_high, nullptr);
  SdeArgs sd{expl, (long long)N * MAX_H * A, (long long)MAX_H * A, sample_freq, pol->params};
  auto finish = [&](int err) { return finish_with_gae(err, do_gae, buf, ag, reward_gamma, reward_gae_lambda, cost_gamma, cost_gae_lambda, stream); };
  auto routed = [&](int err, int route, const char* ws, int wgs, int E, int launches) {
    if (err == 0) note_route(ICRL_FAMILY_ROLLOUT, route, ws_source(ag, ws), wgs, E, pick_bits(k, route), 0, 1, launches);
    return err;
  };
  {
    const bool gran = (size_t)N * (2 * O + 4) <= (size_t)256 * GRAN_MAX;
    char* ws = exchange_ws(ag, buf, persist_ws_bytes(N, O, gran));
    if (!(do_gae & 2) && env->reward_form < 4 && N <= 128 && N * O <= NORM_CHUNK && ws != nullptr) {
      PersistArgs p;
      p.act = a; p.nm = *nm; p.T = T; p.prof = 0;
      const size_t clear = persist_ws_carve(ws, N, O, gran, p);
      hipError_t e = hipMemsetAsync(p.counter, 0, clear, s);
      if (e != hipSuccess) return (int)e;
      k.gran = gran;
      const size_t dyn = persist_sde_dyn_lds(N, O, A);
      const int perr = launch_rollout_persistent_sde(k, N, dyn, s, p, sd);
      if (perr >= 0) return finish(routed(perr > 0 ? perr : (int)hipGetLastError(), ICRL_ROUTE_PERSISTENT, ws, N, 1, 1));
    }
  }
  for (int t = 0; t < T; ++t) {
    launch_act_step_sde(k, N, s, a, sd, t);
    const size_t row = (size_t)t * N;
    NormStepArgs b{*nm, env->s, ag->raw_rew, cn ? ag->raw_cost : nullptr, ag->dones, N, O, ag->last_obs, nullptr, nullptr,
                   buf->new_observations + row * O, buf->rewards + row, buf->costs + row, ag->last_dones};
    launch_norm_step(b, s);
  }
  return finish(routed((int)hipGetLastError(), ICRL_ROUTE_PER_STEP, nullptr, N, 0, 2 * T));
}
