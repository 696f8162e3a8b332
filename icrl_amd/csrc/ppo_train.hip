// PPO-Lagrangian update as ONE persistent launch: the dispatch layer of the update family — gfx950.
//
// ref: stable_baselines3/ppo_lag/ppo_lag.py:196-299 (epoch / minibatch loop of PPOLagrangian.train), common/buffers.py:594-627 (get /
//      _get_samples).
//
// The reference performs n_epochs * ceil(T*N / batch) DEPENDENT optimiser steps on a 64..256-row minibatch through three small independent
// MLPs; parity forbids re-ordering or merging those steps, so every kernel of the family runs all of them in one launch.  This file holds
// what they share on the host: the argument checks and pre-kernels of a run (permutation offsets, the schedule tables of ppo_common.h),
// the choice of the kernel (prepare_train: kinds 0..7; the kernels live in ppo_train_{pairs,rows,tiles,halves,quarters,quarters2}.hip, the
// generic-shape path in generic.hip), the route record and the icrl_ppo_lag_train* entry points.  The gSDE update has its own entry point
// (ppo_train_sde.hip) on the tiles kernel.
#include "ppo_common.h"

namespace icrl {

// flat env-major indices of the permutations (buffers.py:53-65: i -> env = i / T, t = i % T) -> [T,N] storage offsets, once per
// launch instead of once per gathered row inside the persistent kernel
__global__ void ppo_perm_offsets_kernel(const int* __restrict__ perms, long long n, int T, int N, int* __restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int idx = perms[i];
  const int env = idx / T, t = idx - env * T;
  out[i] = t * N + env;
}

__global__ void ppo_plan_kernel(const int* adam_t, int n_steps, int n_mb, int n_total, int B, double lr, double b1, double b2,
                                PlanStep* steps, PlanChunk* chunks, int two_per_step) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_steps + 2) return;
  if (i >= n_steps) { steps[i] = PlanStep{0.f, 0.f, 0, 0}; return; }
  const int e = i / n_mb, mb = i % n_mb, p = mb * B;
  const int nb = n_total - p < B ? n_total - p : B;
  const int cpm = (B + RB - 1) / RB;
  const int nb_last = n_total - (n_mb - 1) * B;
  const int cpe = (n_mb - 1) * cpm + (nb_last + RB - 1) / RB;
  const int g0 = e * cpe + mb * cpm, nch = (nb + RB - 1) / RB;
  const double t = (double)(adam_t[0] + i + 1);
  steps[i] = PlanStep{(float)(lr / (1.0 - pow(b1, t))), (float)(1.0 / sqrt(1.0 - pow(b2, t))),
                      nb | ((mb == 0) << NB_FIRST) | ((mb == n_mb - 1) << NB_LAST) | (e << NB_EPOCH), e * n_total + p};
  if (chunks == nullptr) return;      // (the generic-shape path reads the step table only)
  if (two_per_step) {      // two workgroups per network: chunk c of step i at 2 i + c, an absent second chunk as 0 rows
    for (int c = 0; c < 2; ++c) chunks[2 * i + c] = c < nch ? PlanChunk{e * n_total + p + RB * c, nb - RB * c < RB ? nb - RB * c : RB} : PlanChunk{0, 0};
    if (i == n_steps - 1)
      for (int c = 0; c < 10; ++c) chunks[2 * n_steps + c] = PlanChunk{0, 0};
    return;
  }
  for (int c = 0; c < nch; ++c) chunks[g0 + c] = PlanChunk{e * n_total + p + RB * c, nb - RB * c < RB ? nb - RB * c : RB};
  if (i == n_steps - 1)
    for (int c = 0; c < 5; ++c) chunks[g0 + nch + c] = PlanChunk{0, 0};
}

}  // namespace icrl

using namespace icrl;

// argument checks + the pre-kernels (granule / statistics reset, permutation offsets, schedule tables) of ONE run; fills `a` and
// reports which persistent kernel runs it: 0 wave pairs, 1 row-owning waves, 2 row-owning waves with two workgroups per network,
// 3 column-split tiles, 6 / 7 four workgroups per network at obs 65..128 (single-run launches; 7: minibatches of 65..128 rows in one pass), 4 wave quads with two workgroups per network (obs <= 32, launches of up to HALVES_MAX_RUNS runs: beyond that the
// compute units are what runs out and a run keeps one per network).  < 0: refused (return value of fail()) or a HIP error, in *err.
// FOUR workgroups per network where two would run (round 6: 6.46 against 6.74 us per optimiser step at HC shapes); ICRL_QUARTERS=0 keeps two (A/B)
static bool quarters_default() {
  static const int v = [] { const char* e = getenv("ICRL_QUARTERS"); return e != nullptr ? (e[0] == '1' ? 1 : 0) : 1; }();
  return v != 0;
}

static int prepare_train(const icrl_policy_t* pol, float* exp_avg, float* exp_avg_sq, int32_t* adam_step, const icrl_buffer_t* buf,
                         const int32_t* perms, const float* nu, const icrl_ppo_hyper_t* hp, float* stats, void* sync_ws,
                         hipStream_t s, TrainArgs& a, int* err, int n_runs) {
  auto bad = [&](int e) { *err = e; return -1; };
  if (pol->arch != nullptr || pol->h1 != HD || pol->h2 != HD)
    return bad(fail("icrl_ppo_lag_train: hidden widths (%d, %d)%s; the persistent update kernels are built for %d x %d (the reference's default net_arch)", pol->h1, pol->h2,
                    pol->arch != nullptr ? " with an `arch` descriptor" : "", HD, HD));
  if (pol->obs_dim < 1 || pol->obs_dim > 128 || pol->act_dim < 1 || pol->act_dim > 16)
    return bad(fail("icrl_ppo_lag_train: obs_dim %d (1..128) / act_dim %d (1..16)", pol->obs_dim, pol->act_dim));
  if (hp->batch_size < 2 || hp->batch_size > MAXB || hp->n_epochs < 1)
    return bad(fail("icrl_ppo_lag_train: batch_size %d (2..%d: one minibatch = at most four 64-row chunks of one workgroup), n_epochs %d (>= 1)", hp->batch_size, MAXB, hp->n_epochs));
  if (hp->n_epochs >= (1 << 19)) return bad(fail("icrl_ppo_lag_train: n_epochs %d, limit 2^19", hp->n_epochs));
  if (hp->batch_size > 128 && (hp->_pad & 2))
    return bad(fail("icrl_ppo_lag_train: batch_size %d: the column-split tiles kernel (hp->_pad & 2) stops at 128 rows", hp->batch_size));
  if (buf->obs_dim != pol->obs_dim || buf->T < 1)
    return bad(fail("icrl_ppo_lag_train: buffer obs_dim %d vs policy %d, T = %d", buf->obs_dim, pol->obs_dim, buf->T));
  if ((long long)buf->T * buf->N >= (1ll << 31) || (long long)buf->T * buf->N * (pol->obs_dim > 16 ? pol->obs_dim : 16) >= (1ll << 30))
    return bad(fail("icrl_ppo_lag_train: %d x %d transitions x obs_dim %d overflow the kernel's 32-bit element offsets (limit 2^30 floats per plane)", buf->T, buf->N, pol->obs_dim));
  if (pol->discrete && buf->act_store != 1) return bad(fail("icrl_ppo_lag_train: discrete policy needs act_store = 1 (action index), got %d", buf->act_store));
  a.L = make_pol_layout(pol->obs_dim, pol->act_dim, pol->h1, pol->h2, pol->discrete);
  a.params = pol->params; a.exp_avg = exp_avg; a.exp_avg_sq = exp_avg_sq; a.adam_t = adam_step;
  a.buf = *buf; a.perms = perms; a.nu = nu; a.hp = *hp; a.stats = stats; a.xch = (u64*)sync_ws;
  a.t_magic = buf->T == 1 ? 0xFFFFFFFFu : (unsigned)((1ull << 32) / (unsigned long long)buf->T);
  a.plan_steps = nullptr; a.plan_chunks = nullptr; a.n_steps = 0; a.gx = nullptr; a.srec = nullptr; a.sstat = nullptr;
  hipError_t e = hipMemsetAsync(sync_ws, 0, 512, s);      // granule slots: 2 step parities x (3 roles x 8 waves, padded to 32) x 8 B
  if (e != hipSuccess) return bad((int)e);
  e = hipMemsetAsync(stats, 0, (32 + hp->n_epochs) * sizeof(float), s);
  if (e != hipSuccess) return bad((int)e);
  const int nt1 = (pol->obs_dim + 15) / 16;
  // default: wave pairs (two waves per SIMD, 6 barriers per step); hp._pad & 4: row-owning waves (one wave per SIMD, 3 barriers
  // per step; 5 when obs > 64); hp._pad & 2: the column-split tiles kernel
  if (nt1 > 8 || (hp->_pad & 2)) {
    if (hp->batch_size > 128) return bad(fail("icrl_ppo_lag_train: batch_size %d with obs_dim %d: the column-split tiles kernel stops at 128 rows", hp->batch_size, pol->obs_dim));
    return 3;
  }
  const int n_total = buf->T * buf->N;
  const int n_mb = (n_total + hp->batch_size - 1) / hp->batch_size;
  const long long n_steps = (long long)hp->n_epochs * n_mb;
  if (n_steps >= (1ll << 21)) return bad(fail("icrl_ppo_lag_train: %lld optimiser steps per call, limit 2^21", n_steps));      // epoch index lives in the upper bits of nb_flags
  PlanStep* steps = reinterpret_cast<PlanStep*>((char*)sync_ws + 512);
  PlanChunk* chunks = reinterpret_cast<PlanChunk*>(steps + n_steps + 2);
  a.plan_steps = steps; a.plan_chunks = chunks; a.n_steps = (int)n_steps;
  {
    // after the plan tables: 16 B per step (+2 entries) and 8 B per chunk (<= 4 chunks per step at batch_size 256, +10 entries):
    // 512 + 16 (n + 2) + 8 (4 n + 10) <= 768 + 48 n  (ICRL_PPO_PLAN_BYTES)
    int* offs = reinterpret_cast<int*>((char*)sync_ws + ICRL_PPO_PLAN_BYTES(n_steps));
    const long long n = (long long)hp->n_epochs * n_total;
    hipLaunchKernelGGL(ppo_perm_offsets_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, perms, n, buf->T, buf->N, offs);
    a.perms = offs;
  }
  // obs <= 64: wave pairs; wider (AntWall 113: dz1^T must share h2^T's LDS, two chunks per minibatch) the row-owning waves,
  // with TWO workgroups per network when a minibatch has two chunks (each computes one, partial gradients exchanged;
  // hp._pad & 8 keeps one workgroup per network)
  // obs 65..128, single-run launches: FOUR workgroups per network, wave quads + the row-owning kernel's parameter ownership
  // (ppo_train_quarters.hip; round 6); hp._pad & 4 keeps the row-owning kernel, hp._pad & 32 / ICRL_QUARTERS=0 its two-workgroup form
  const bool quarters_wide = nt1 > 4 && n_runs == 1 && !(hp->_pad & (4 | 32)) && quarters_default();
  // ... minibatches of 65..128 rows (the reference's AntWall batch size): both 64-row chunks in ONE pass, two row tiles per wave (ppo_train_quarters2.hip;
  // the chunk plan with two entries per step); ICRL_QUARTERS_PASSES=1 keeps the chunk-by-chunk form (A/B)
  static const bool one_pass = [] { const char* e = getenv("ICRL_QUARTERS_PASSES"); return e == nullptr || e[0] != '1'; }();
  const bool quarters_wide2 = quarters_wide && one_pass && hp->batch_size > RB && hp->batch_size <= 2 * RB;
  const bool rows = !quarters_wide && ((hp->_pad & 4) || nt1 > 4);
  const bool split = rows && hp->batch_size > RB && hp->batch_size <= 2 * RB && !(hp->_pad & 8);     // (three or four chunks: one workgroup walks them)
  // hp._pad & 16: the wave-pair kernel (one workgroup per network) where the wave-quad kernel would run
  // (5: four workgroups per network — round 6; hp._pad & 32 keeps two)
  const bool halves = !rows && n_runs <= HALVES_MAX_RUNS && nt1 <= 2 && !(hp->_pad & 16);
  const bool quarters = halves && n_runs <= QUARTERS_MAX_RUNS && !(hp->_pad & 32) && quarters_default();
  hipLaunchKernelGGL(ppo_plan_kernel, dim3((unsigned)((n_steps + 2 + 255) / 256)), dim3(256), 0, s, adam_step, (int)n_steps, n_mb,
                     n_total, hp->batch_size, (double)hp->lr, (double)hp->adam_beta1, (double)hp->adam_beta2, steps, chunks, (int)(split || quarters_wide2));
  if (split || halves || quarters_wide) {
    const size_t off = (ICRL_PPO_PLAN_BYTES(n_steps) + 4 * (size_t)hp->n_epochs * n_total + 255) / 256 * 256;      // behind the permutation offsets
    a.gx = reinterpret_cast<u64*>((char*)sync_ws + off);
    e = hipMemsetAsync(a.gx, 0, ICRL_PPO_SPLIT_BYTES, s);
    if (e != hipSuccess) return bad((int)e);
  }
  if (quarters_wide) return quarters_wide2 ? 7 : 6;
  return rows ? (split ? 2 : 1) : (halves ? (quarters ? 5 : 4) : 0);
}

// shapes the persistent kernels refuse (hidden widths above 64, architectures given by icrl_policy_t.arch, minibatches above 256 rows):
// the generic-shape path of generic.hip, three plain launches per optimiser step.  Its scratch lies behind the regular workspace:
// sync_ws must then hold ICRL_PPO_SYNC_BYTES(...) + ICRL_PPO_GENERIC_BYTES(batch_size, row_floats, n_params) bytes.
static int train_generic(const icrl_policy_t* pol, float* exp_avg, float* exp_avg_sq, int32_t* adam_step, const icrl_buffer_t* buf,
                         const int32_t* perms, const float* nu, const icrl_ppo_hyper_t* hp, float* stats, void* sync_ws, hipStream_t s) {
  if (hp->batch_size < 2 || hp->n_epochs < 1) return fail("icrl_ppo_lag_train: batch_size %d (>= 2), n_epochs %d (>= 1)", hp->batch_size, hp->n_epochs);
  if (pol->arch != nullptr) { if (int e = policy_generic_check(pol, "icrl_ppo_lag_train")) return e; }
  else if (pol->h1 != pol->h2 || pol->h1 % 64 != 0 || pol->h1 > 256 || pol->obs_dim < 1 || pol->obs_dim > 1024 || pol->act_dim < 1 || pol->act_dim > 16)
    return fail("icrl_ppo_lag_train: hidden widths (%d, %d), obs_dim %d, act_dim %d: the persistent kernels are built for %d x %d (narrower layers stored "
                "zero-padded), obs <= 128, act <= 16; the generic-shape path for a common padded width that is a multiple of 64 up to 256, obs <= 1024",
                pol->h1, pol->h2, pol->obs_dim, pol->act_dim, HD, HD);
  if (buf->obs_dim != pol->obs_dim || buf->T < 1) return fail("icrl_ppo_lag_train: buffer obs_dim %d vs policy %d, T = %d", buf->obs_dim, pol->obs_dim, buf->T);
  if ((long long)buf->T * buf->N * (pol->obs_dim > 16 ? pol->obs_dim : 16) >= (1ll << 31))
    return fail("icrl_ppo_lag_train: %d x %d transitions x obs_dim %d overflow 32-bit element offsets", buf->T, buf->N, pol->obs_dim);
  if (pol->discrete && buf->act_store != 1) return fail("icrl_ppo_lag_train: discrete policy needs act_store = 1 (action index), got %d", buf->act_store);
  const int n_total = buf->T * buf->N;
  const int n_mb = (n_total + hp->batch_size - 1) / hp->batch_size;
  const long long n_steps = (long long)hp->n_epochs * n_mb;
  hipError_t e = hipMemsetAsync(stats, 0, (32 + hp->n_epochs) * sizeof(float), s);
  if (e != hipSuccess) return (int)e;
  int* offs = reinterpret_cast<int*>((char*)sync_ws + ICRL_PPO_PLAN_BYTES(n_steps));
  const long long n = (long long)hp->n_epochs * n_total;
  hipLaunchKernelGGL(ppo_perm_offsets_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, perms, n, buf->T, buf->N, offs);
  char* scratch = (char*)sync_ws + ICRL_PPO_SYNC_BYTES(hp->n_epochs, n_mb, n_total);
  const int err = launch_train_generic(pol, exp_avg, exp_avg_sq, adam_step, buf, offs, nu, hp, stats, scratch, sync_ws, s);
  // the generic kernels keep THEIR transposed image in params_t; a policy the fast forward kernels serve (this call came here for its
  // batch size) gets the image those kernels read back
  if (err == 0 && !policy_is_wide(pol)) return icrl_policy_prepare(pol, (void*)s);
  return err;
}

// the route record of a launched update, its one writer (the generic-shape path has its own in generic.hip): workgroups per network
// of `kind` (prepare_train) and the grid layout the launcher reported, behind the launcher's error
static int routed_update(int err, int kind, int n_runs, int packed, int streamed = 0) {
  static const int wgs[8] = {1, 1, 2, 1, 2, 4, 4, 4};
  if (err == 0) note_route(ICRL_FAMILY_UPDATE, kind, wgs[kind], n_runs, packed, streamed);
  return err;
}

extern "C" int icrl_ppo_generic_row_floats(const icrl_policy_t* pol) { return generic_row_floats(pol); }

// bytes of the minibatch stream of this call (records + statistics table), 0 with the reason as the last error where the stream does not serve it: the
// shapes of the single-run wave-quad launches (prepare_train's kinds 4 and 5) and a workspace the kernel's 32-bit byte offsets reach
extern "C" size_t icrl_ppo_stream_ws_bytes(const icrl_policy_t* pol, const icrl_buffer_t* buf, const icrl_ppo_hyper_t* hp) {
  auto no = [](int) { return (size_t)0; };
  if (pol->arch != nullptr || pol->h1 != HD || pol->h2 != HD)
    return no(fail("icrl_ppo_stream_ws_bytes: hidden widths (%d, %d)%s: the minibatch stream serves the wave-quad update kernel (%d x %d, no `arch` descriptor)", pol->h1, pol->h2,
                   pol->arch != nullptr ? " with an `arch` descriptor" : "", HD, HD));
  if (pol->obs_dim < 1 || pol->obs_dim > 32 || pol->act_dim < 1 || pol->act_dim > 16)
    return no(fail("icrl_ppo_stream_ws_bytes: obs_dim %d / act_dim %d: the minibatch stream serves the wave-quad update kernel (obs_dim 1..32, act_dim 1..16)", pol->obs_dim, pol->act_dim));
  if (hp->batch_size < 2 || hp->batch_size > MAXB || hp->n_epochs < 1)
    return no(fail("icrl_ppo_stream_ws_bytes: batch_size %d (2..%d), n_epochs %d (>= 1): the minibatch stream serves the persistent update kernels' minibatches", hp->batch_size, MAXB, hp->n_epochs));
  if (hp->_pad & (2 | 4 | 16))
    return no(fail("icrl_ppo_stream_ws_bytes: hp->_pad = %d asks for another update kernel; the minibatch stream serves the wave-quad kernel", hp->_pad));
  if (buf->obs_dim != pol->obs_dim || buf->T < 1 || buf->N < 1 || buf->act_store < 1 || buf->act_store > 16 || (long long)buf->T * buf->N >= (1ll << 31))
    return no(fail("icrl_ppo_stream_ws_bytes: buffer obs_dim %d vs policy %d, T = %d, N = %d, act_store = %d", buf->obs_dim, pol->obs_dim, buf->T, buf->N, buf->act_store));
  const int n_total = buf->T * buf->N;
  const long long n_mb = (n_total + hp->batch_size - 1) / hp->batch_size, n_steps = (long long)hp->n_epochs * n_mb;
  const long long n_chunks = stream_n_chunks(n_total, hp->batch_size, hp->n_epochs);
  const double approx = 4.0 * (double)(n_chunks + 1) * 64.0 * (double)(pol->obs_dim + buf->act_store + SR_PLANES);
  if (n_steps >= (1ll << 21) || approx >= 4294967296.0 - 65536.0)
    return no(fail("icrl_ppo_stream_ws_bytes: %lld optimiser steps, %.0f bytes of records: beyond the kernel's 32-bit byte offsets into the stream", n_steps, approx));
  return stream_bytes(pol->obs_dim, buf->act_store, n_chunks, n_steps);
}

static int train_single(const icrl_policy_t* pol, float* exp_avg, float* exp_avg_sq, int32_t* adam_step,
                        const icrl_buffer_t* buf, const int32_t* perms, const float* nu,
                        const icrl_ppo_hyper_t* hp, float* stats, void* sync_ws, void* stream_ws, long long stream_ws_bytes, void* stream) {
  TrainArgs a;
  hipStream_t s = (hipStream_t)stream;
  note_route(ICRL_FAMILY_UPDATE);
  if (policy_is_wide(pol) || hp->batch_size > MAXB)      // (kinds 8 / 9: written by launch_train_generic)
    return train_generic(pol, exp_avg, exp_avg_sq, adam_step, buf, perms, nu, hp, stats, sync_ws, s);
  int err = 0;
  const int kind = prepare_train(pol, exp_avg, exp_avg_sq, adam_step, buf, perms, nu, hp, stats, sync_ws, s, a, &err, 1);
  if (kind < 0) return err;
  const int nt1 = (pol->obs_dim + 15) / 16;
  int packed = 0, streamed = 0;
  auto routed = [&](int e) { return routed_update(e, kind, 1, packed, streamed); };
  if ((kind == 4 || kind == 5) && stream_ws != nullptr) {      // the minibatch stream, where the caller brought room for it
    const size_t need = icrl_ppo_stream_ws_bytes(pol, buf, hp);
    if (need == 0) icrl_clear_error();      // (not served: the in-kernel gather, silently — this entry point then IS icrl_ppo_lag_train)
    else if (stream_ws_bytes >= (long long)need) {
      if (const int e = launch_stream_prepass(a, stream_ws, s)) return e;
      streamed = 1;
    }
  }
  if (kind == 4 || kind == 5) return routed(launch_train_halves(a, pol->discrete != 0, kind == 5 ? 4 : 2, s, &packed));
  if (kind == 6) return routed(launch_train_quarters_wide(a, pol->discrete != 0, s, &packed));
  if (kind == 7) return routed(launch_train_quarters_wide2(a, pol->discrete != 0, s, &packed));
  if (kind == 0) return routed(launch_train_pairs(a, nt1, pol->discrete != 0, s, &packed));
  if (kind <= 2) return routed(launch_train_rows(a, nt1, pol->discrete != 0, kind == 2, s, &packed));
  return routed(launch_train_tiles(a, nt1, pol->discrete ? HEAD_CAT : HEAD_GAUSS, s, &packed));      // (kind 3)
}

extern "C" int icrl_ppo_lag_train(const icrl_policy_t* pol, float* exp_avg, float* exp_avg_sq, int32_t* adam_step,
                                  const icrl_buffer_t* buf, const int32_t* perms, const float* nu,
                                  const icrl_ppo_hyper_t* hp, float* stats, void* sync_ws, void* stream) {
  return train_single(pol, exp_avg, exp_avg_sq, adam_step, buf, perms, nu, hp, stats, sync_ws, nullptr, 0, stream);
}

extern "C" int icrl_ppo_lag_train_stream(const icrl_policy_t* pol, float* exp_avg, float* exp_avg_sq, int32_t* adam_step,
                                         const icrl_buffer_t* buf, const int32_t* perms, const float* nu,
                                         const icrl_ppo_hyper_t* hp, float* stats, void* sync_ws, void* stream_ws, long long stream_ws_bytes, void* stream) {
  return train_single(pol, exp_avg, exp_avg_sq, adam_step, buf, perms, nu, hp, stats, sync_ws, stream_ws, stream_ws_bytes, stream);
}

extern "C" int icrl_ppo_lag_train_batch(int n_runs, const icrl_ppo_train_job_t* jobs, void* args_ws, long long args_ws_bytes,
                                        void* stream) {
  note_route(ICRL_FAMILY_UPDATE);
  if (n_runs < 1 || n_runs > 65535) return fail("icrl_ppo_lag_train_batch: n_runs = %d (1..65535)", n_runs);
  if (args_ws == nullptr || args_ws_bytes < (long long)n_runs * (long long)sizeof(TrainArgs))
    return fail("icrl_ppo_lag_train_batch: args_ws holds %lld B, %d runs need %lld (ICRL_BATCH_ARGS_BYTES each)", args_ws_bytes, n_runs,
                (long long)n_runs * (long long)sizeof(TrainArgs));
  static_assert(sizeof(TrainArgs) <= ICRL_BATCH_ARGS_BYTES, "ICRL_BATCH_ARGS_BYTES");
  hipStream_t s = (hipStream_t)stream;
  TrainArgs* d_args = (TrainArgs*)args_ws;
  int kind0 = -1, packed = 0;
  const icrl_ppo_train_job_t& j0 = jobs[0];
  for (int r = 0; r < n_runs; ++r) {
    const icrl_ppo_train_job_t& j = jobs[r];
    if (j.pol->obs_dim != j0.pol->obs_dim || j.pol->act_dim != j0.pol->act_dim || j.pol->discrete != j0.pol->discrete ||
        j.hp->batch_size != j0.hp->batch_size || j.hp->n_epochs != j0.hp->n_epochs || j.hp->_pad != j0.hp->_pad ||
        j.buf->T != j0.buf->T || j.buf->N != j0.buf->N || j.buf->act_store != j0.buf->act_store)
      return fail("icrl_ppo_lag_train_batch: run %d differs from run 0 in a shape (obs / act / discrete / batch_size / n_epochs / T / N): the runs of a batch share one grid", r);
    TrainArgs a;
    int err = 0;
    const int kind = prepare_train(j.pol, j.exp_avg, j.exp_avg_sq, j.adam_step, j.buf, j.perms, j.nu, j.hp, j.stats, j.sync_ws, s, a, &err, n_runs);
    if (kind < 0) return err;
    if (kind == 3) return fail("icrl_ppo_lag_train_batch: the column-split tiles kernel (hp->_pad & 2) has no batched form");
    if (r == 0) kind0 = kind;
    if (kind == 6) { const int e = launch_train_quarters_wide(a, j.pol->discrete != 0, s, &packed); return routed_update(e, kind, 1, packed); }      // (a one-run batch at obs 65..128: the single-run launch)
    if (kind == 7) { const int e = launch_train_quarters_wide2(a, j.pol->discrete != 0, s, &packed); return routed_update(e, kind, 1, packed); }
    const int e = put_args(a, d_args + r, s);
    if (e != 0) return e;
  }
  const int nt1 = (j0.pol->obs_dim + 15) / 16;
  int err;
  if (kind0 == 4 || kind0 == 5) err = launch_train_halves_batch(d_args, n_runs, j0.pol->obs_dim, j0.pol->discrete != 0, kind0 == 5 ? 4 : 2, (j0.hp->_pad & 1) != 0, s, &packed);
  else if (kind0 == 0) err = launch_train_pairs_batch(d_args, n_runs, j0.pol->obs_dim, nt1, j0.pol->discrete != 0, (j0.hp->_pad & 1) != 0, s, &packed);
  else err = launch_train_rows_batch(d_args, n_runs, nt1, j0.pol->discrete != 0, kind0 == 2, s, &packed);
  return routed_update(err, kind0, n_runs, packed);
}
