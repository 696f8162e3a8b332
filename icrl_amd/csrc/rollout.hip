// Rollout-time kernels — gfx950.
//
// One environment step of OnPolicyWithCostAlgorithm.collect_rollouts
// (ref: stable_baselines3/common/on_policy_algorithm.py:367-416) is two launches:
//
//   act_step_kernel   one workgroup (3 waves = pi | vf | cvf) per environment:
//                     policy forward (ref: policies.py:716-731, torch_layers.py:245-254, distributions.py:143-171)
//                     -> clip -> synthetic env step + auto-reset (spec: oracle/synth_env.py)
//                     -> cost_function(previous raw obs, clipped action) (ref: icrl/constraint_net.py:121-130,258-299;
//                        vec_cost_wrapper.py:51-66) -> the buffer fields that do not need the normaliser
//                        (ref: buffers.py:554-592).
//   norm_step_kernel  one workgroup for all environments: running-moment merge of obs / discounted reward return /
//                     discounted cost return in float64 with numpy's reduction order, normalise + clip, remaining
//                     buffer fields (ref: vec_normalize.py:81-123,220-261; running_mean_std.py:19-39).
//
// The same device functions back the fine-grained C-ABI entry points (icrl_policy_forward, icrl_cost_mlp_forward,
// icrl_synth_env_step, icrl_vecnorm_step) that the Python VecEnv / ConstraintNet classes call one at a time.
//
// Weights are read from the transposed copies ([in][out]) written by *_prepare so that the 64 lanes of a wave
// (one lane per output unit) load 256 contiguous bytes per input index.
#include <stdio.h>
#include <stdlib.h>

#include "common.h"
#include "cost_fn.h"
#include "generic.h"
#include "rollout_launch.h"

namespace icrl {

// =================================================================================================================
// transposed weight copies
// =================================================================================================================
__global__ void policy_transpose_kernel(PolLayout L, const float* __restrict__ p, float* __restrict__ pt) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < L.n; i += gridDim.x * blockDim.x) {
    int dst = i;
    for (int w = 0; w < 3; ++w) {
      if (i >= L.W1[w] && i < L.b1[w]) { int r = i - L.W1[w]; int j = r / L.O, k = r % L.O; dst = L.W1[w] + k * L.H1 + j; }
      if (i >= L.W2[w] && i < L.b2[w]) { int r = i - L.W2[w]; int j = r / L.H1, k = r % L.H1; dst = L.W2[w] + k * L.H2 + j; }
    }
    if (i >= L.Wa && i < L.ba) { int r = i - L.Wa; int a = r / L.H2, j = r % L.H2; dst = L.Wa + j * L.A + a; }
    pt[dst] = p[i];
  }
}

__global__ void costnet_transpose_kernel(CnLayout L, const float* __restrict__ p, float* __restrict__ pt) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < L.n; i += gridDim.x * blockDim.x) {
    int dst = i;
    if (i >= L.W0 && i < L.b0) { int r = i - L.W0; int j = r / L.in, k = r % L.in; dst = L.W0 + k * L.H1 + j; }
    if (L.nh == 2 && i >= L.W1 && i < L.b1) { int r = i - L.W1; int j = r / L.H1, k = r % L.H1; dst = L.W1 + k * L.H2 + j; }
    pt[dst] = p[i];
  }
}

// =================================================================================================================
// device building blocks (called by a 192-thread workgroup handling ONE environment)
// =================================================================================================================
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct ActShared {
  alignas(16) double s_old[MAX_OBS];   // raw observation before the step (== VecCostWrapper.previous_obs)
  alignas(16) double s_new[MAX_OBS];   // raw observation after the step (post auto-reset)
  alignas(16) float x[MAX_OBS];        // normalised observation, float32 (policy input)
  alignas(16) float h[3][MAX_H];
  alignas(16) float g[3][MAX_H];
  alignas(16) float cx[MAX_CN_IN];     // cost-net input
  alignas(16) float ch[2][MAX_H];
  float act_raw[MAX_ACT];
  float act_clip[MAX_ACT];
  float scal[4];           // v_r, v_c, log_prob, (unused)
};

// One lane's slice of the three MLPs, held in registers: lane j of wave w (pi | vf | cvf) owns column j of W1^T and
// W2^T of network w; lanes < A of wave 0 own a column of the action head, the value waves one head weight per lane.
// All loads are issued back to back (one memory latency for the whole network instead of one per input index); a
// persistent kernel loads them ONCE for all its steps.
// ONE register image per wave for both roles: a wave is either a policy wave (pi / vf / cvf) or the cost-net wave, never both,
// but the compiler cannot know that and would keep two full weight sets live in every wave (at AntWall widths 263 + 232
// values: 468 registers spilled to scratch, the cost wave alone 50 k cycles per step).  The two roles' arrays of equal type
// share storage through anonymous unions (same element type: plain aliases, no type punning).
template <int OCT, int CIT>
struct WaveRegs {
  static constexpr int NA = 16 * (OCT > CIT ? OCT : CIT);
  union { float w1[NA]; float c0[NA]; };          // policy: W1 column of hidden unit `lane` (16 OCT used) | cost net: W0 column (16 CIT)
  union { float w2[MAX_H]; float c1[MAX_H]; };    // second layer column
  float wh[MAX_H];   // wave 0: head column of action `lane`; waves 1/2: wh[0] = value-head weight of hidden unit `lane`
  union { float b1; float cb0; };
  union { float b2; float cb1; };
  union { float bh; float cbo; };
  union { float ls; float co; };
  float sd, lsd, i2v;   // Gaussian head constants of action `lane`: exp(log_std), log(exp(log_std)), 1 / (2 sd^2) denominators
  int sel[(16 * (CIT > 0 ? CIT : 1) + WAVE - 1) / WAVE];   // cost net: select_dim entries this lane prepares
};
template <int OCT> using PolRegs = WaveRegs<OCT, 0>;
template <int CIT> using CnRegs = WaveRegs<0, CIT>;

template <int OCT, class Regs>
__device__ __forceinline__ void load_pol_regs(const PolLayout& L, const float* __restrict__ PT, Regs& R) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j1 = lane < L.H1 ? lane : 0, j2 = lane < L.H2 ? lane : 0;
#pragma unroll
  for (int k = 0; k < 16 * OCT; ++k) R.w1[k] = (w < 3 && k < L.O) ? PT[L.W1[w] + k * L.H1 + j1] : 0.f;
#pragma unroll
  for (int k = 0; k < MAX_H; ++k) R.w2[k] = (w < 3 && k < L.H1) ? PT[L.W2[w] + k * L.H2 + j2] : 0.f;
  R.b1 = w < 3 ? PT[L.b1[w] + j1] : 0.f;
  R.b2 = w < 3 ? PT[L.b2[w] + j2] : 0.f;
  R.bh = 0.f; R.ls = 0.f; R.sd = 1.f; R.lsd = 0.f; R.i2v = 2.f;
  if (w == 0) {
    const int a = lane < L.A ? lane : 0;
#pragma unroll
    for (int j = 0; j < MAX_H; ++j) R.wh[j] = j < L.H2 ? PT[L.Wa + j * L.A + a] : 0.f;
    R.bh = PT[L.ba + a];
    if (!L.discrete) R.ls = PT[L.log_std + a];
    // constants of the whole rollout: evaluated once here instead of once per env step (same expressions as before)
    R.sd = expf(R.ls); R.lsd = logf(R.sd); R.i2v = 2.f * (R.sd * R.sd);
  } else if (w < 3) {
#pragma unroll
    for (int j = 1; j < MAX_H; ++j) R.wh[j] = 0.f;
    R.wh[0] = PT[(w == 1 ? L.Wv : L.Wc) + j2];
    R.bh = PT[w == 1 ? L.bv : L.bc];
  }
}

// three tanh MLPs + heads for the observation in sh.x.  Must be called by all threads of the workgroup (waves >= 3 only
// take part in the barriers).
template <int OCT, class Regs>
__device__ __forceinline__ void policy_forward_block(const PolLayout& L, const Regs& R, ActShared& sh,
                                                     const float* noise_row, int deterministic,
                                                     const float* alow, const float* ahigh,
                                                     const float* given = nullptr /* evaluate_actions: actions to score */) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // activations are pulled from LDS as whole float4 rows first (broadcast reads), then consumed from registers: one LDS
  // latency per layer instead of one per input.  Pad weights are zero, so no bounds test is needed in the FMA chains.
  if (w < 3) {
    f32x4 xs[4 * OCT];
#pragma unroll
    for (int i = 0; i < 4 * OCT; ++i) xs[i] = *reinterpret_cast<const f32x4*>(&sh.x[4 * i]);
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 16 * OCT; ++k) acc = fmaf(R.w1[k], xs[k >> 2][k & 3], acc);
    sh.h[w][lane] = lane < L.H1 ? fast_tanh(acc + R.b1) : 0.f;   // pad lanes store 0 (0 * garbage would poison the next layer)
  }
  __syncthreads();
  if (w < 3) {
    f32x4 hs[MAX_H / 4];
#pragma unroll
    for (int i = 0; i < MAX_H / 4; ++i) hs[i] = *reinterpret_cast<const f32x4*>(&sh.h[w][4 * i]);
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < MAX_H; ++k) acc = fmaf(R.w2[k], hs[k >> 2][k & 3], acc);
    sh.g[w][lane] = lane < L.H2 ? fast_tanh(acc + R.b2) : 0.f;
  }
  __syncthreads();
  if (w == 0) {
    float mean = 0.f;
    {
      f32x4 gs[MAX_H / 4];
#pragma unroll
      for (int i = 0; i < MAX_H / 4; ++i) gs[i] = *reinterpret_cast<const f32x4*>(&sh.g[0][4 * i]);
      float acc = 0.f;
#pragma unroll
      for (int j = 0; j < MAX_H; ++j) acc = fmaf(R.wh[j], gs[j >> 2][j & 3], acc);
      mean = acc + R.bh;
    }
    if (!L.discrete) {
      float lp = 0.f, entl = 0.f;
      if (lane < L.A) {
        const float std = R.sd;
        float act = mean;
        if (given != nullptr) act = given[lane];
        else if (!deterministic) act = mean + noise_row[lane] * std;   // Normal.rsample: loc + eps * scale
        const float diff = act - mean;
        // Normal.log_prob: -((x - mu)^2) / (2 var) - log(std) - log(sqrt(2 pi))
        lp = -(diff * diff) / R.i2v - R.lsd - LOG_SQRT_2PI_F;
        entl = HALF_LOG_2PI_PLUS_HALF_F + R.lsd;
        sh.act_raw[lane] = act;
        float c = act;
        if (alow != nullptr && ahigh != nullptr) c = fminf(fmaxf(act, alow[lane]), ahigh[lane]);
        sh.act_clip[lane] = c;
      }
      lp = wave_sum_fast(lp);
      // entropy of the diagonal Gaussian: sum_a 0.5 + 0.5 log(2 pi) + log sigma_a
      const float ent = wave_sum_fast(entl);
      if (lane == 0) { sh.scal[2] = lp; sh.scal[3] = ent; }
    } else {
      // Categorical(logits): log-softmax, inverse-CDF sample on the injected uniform (spec: oracle/nets.py forward)
      float m = wave_max(lane < L.A ? mean : -INFINITY);
      float e = lane < L.A ? expf(mean - m) : 0.f;
      float lse = m + logf(wave_sum(e));
      float logp = mean - lse;
      float p = lane < L.A ? expf(logp) : 0.f;
      float cdf = 0.f;
      int action = 0;
      if (given != nullptr) {
        action = (int)given[0];
      } else if (deterministic) {
        float best = wave_max(lane < L.A ? p : -1.f);
        unsigned long long ball = __ballot(lane < L.A && p == best);
        action = __ffsll((long long)ball) - 1;
      } else {
        const float u = noise_row[0];
        int cnt = 0;
        for (int a = 0; a < L.A; ++a) {     // sequential inclusive prefix sum, like th.cumsum
          cdf += __shfl(p, a, 64);
          cnt += (u >= cdf) ? 1 : 0;
        }
        action = cnt < L.A - 1 ? cnt : L.A - 1;
      }
      const float lp = __shfl(logp, action, 64);
      const float ent = -wave_sum(lane < L.A ? logp * p : 0.f);
      if (lane == 0) { sh.scal[2] = lp; sh.scal[3] = ent; sh.act_raw[0] = (float)action; sh.act_clip[0] = (float)action; }
    }
  } else if (w < 3) {
    float part = lane < L.H2 ? R.wh[0] * sh.g[w][lane] : 0.f;
    part = wave_sum_fast(part);
    if (lane == 0) sh.scal[w - 1] = part + R.bh;
  }
}

// policy_forward_block for the persistent rollout's step chain (rollout_persistent_body): the same three MLPs and heads, every expression
// and its order as above, but wave 0 leaves with nothing but the action behind it.
//  - sh.h[w] / sh.g[w] are written and read by wave w alone, so a wave-local ordering (the wave's LDS stores performed, no instruction moved
//    across) stands where the block form has two workgroup barriers: no wave waits for another one before the caller's hand-off barrier;
//  - the log-prob is not evaluated here: wave 0 returns `act - mean` of its lane (Gaussian head) and the caller evaluates chain_log_prob
//    behind its record stores; the Categorical head needs the log-softmax for its sample and returns the log-prob itself;
//  - the value waves return their value (every lane) and store it themselves; sh.scal is not written; the entropy, which no rollout
//    kernel reads, is not computed.
// Sampling only (no `given`, not deterministic).  Returns 0 in waves >= 3.
__device__ __forceinline__ void wave_lds_order() {
  __builtin_amdgcn_s_waitcnt(0xC07F);      // lgkmcnt(0)
  __builtin_amdgcn_wave_barrier();
}
template <int OCT, class Regs>
__device__ __forceinline__ float policy_forward_chain(const PolLayout& L, const Regs& R, ActShared& sh, const float* noise_row,
                                                      const float* alow, const float* ahigh) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (w >= 3) return 0.f;
  {
    f32x4 xs[4 * OCT];
#pragma unroll
    for (int i = 0; i < 4 * OCT; ++i) xs[i] = *reinterpret_cast<const f32x4*>(&sh.x[4 * i]);
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 16 * OCT; ++k) acc = fmaf(R.w1[k], xs[k >> 2][k & 3], acc);
    sh.h[w][lane] = lane < L.H1 ? fast_tanh(acc + R.b1) : 0.f;   // pad lanes store 0 (0 * garbage would poison the next layer)
  }
  wave_lds_order();
  {
    f32x4 hs[MAX_H / 4];
#pragma unroll
    for (int i = 0; i < MAX_H / 4; ++i) hs[i] = *reinterpret_cast<const f32x4*>(&sh.h[w][4 * i]);
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < MAX_H; ++k) acc = fmaf(R.w2[k], hs[k >> 2][k & 3], acc);
    sh.g[w][lane] = lane < L.H2 ? fast_tanh(acc + R.b2) : 0.f;
  }
  wave_lds_order();
  if (w != 0) {
    float part = lane < L.H2 ? R.wh[0] * sh.g[w][lane] : 0.f;
    part = wave_sum_fast(part);
    return part + R.bh;
  }
  float mean = 0.f;
  {
    f32x4 gs[MAX_H / 4];
#pragma unroll
    for (int i = 0; i < MAX_H / 4; ++i) gs[i] = *reinterpret_cast<const f32x4*>(&sh.g[0][4 * i]);
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < MAX_H; ++j) acc = fmaf(R.wh[j], gs[j >> 2][j & 3], acc);
    mean = acc + R.bh;
  }
  if (!L.discrete) {
    float diff = 0.f;
    if (lane < L.A) {
      const float act = mean + noise_row[lane] * R.sd;   // Normal.rsample: loc + eps * scale
      diff = act - mean;
      sh.act_raw[lane] = act;
      float c = act;
      if (alow != nullptr && ahigh != nullptr) c = fminf(fmaxf(act, alow[lane]), ahigh[lane]);
      sh.act_clip[lane] = c;
    }
    return diff;
  }
  // Categorical(logits): log-softmax, inverse-CDF sample on the injected uniform (spec: oracle/nets.py forward)
  float m = wave_max(lane < L.A ? mean : -INFINITY);
  float e = lane < L.A ? expf(mean - m) : 0.f;
  float lse = m + logf(wave_sum(e));
  float logp = mean - lse;
  float p = lane < L.A ? expf(logp) : 0.f;
  float cdf = 0.f;
  const float u = noise_row[0];
  int cnt = 0;
  for (int a = 0; a < L.A; ++a) {     // sequential inclusive prefix sum, like th.cumsum
    cdf += __shfl(p, a, 64);
    cnt += (u >= cdf) ? 1 : 0;
  }
  const int action = cnt < L.A - 1 ? cnt : L.A - 1;
  if (lane == 0) { sh.act_raw[0] = (float)action; sh.act_clip[0] = (float)action; }
  return __shfl(logp, action, 64);
}
// the log-prob of the action policy_forward_chain sampled, from what wave 0 got back (`head`); result in every lane
template <class Regs>
__device__ __forceinline__ float chain_log_prob(const PolLayout& L, const Regs& R, float head) {
  if (L.discrete) return head;
  const int lane = threadIdx.x & 63;
  float lp = 0.f;
  // Normal.log_prob: -((x - mu)^2) / (2 var) - log(std) - log(sqrt(2 pi))
  if (lane < L.A) lp = -(head * head) / R.i2v - R.lsd - LOG_SQRT_2PI_F;
  return wave_sum_fast(lp);
}

// cost-net weights of one lane (lane j <-> hidden unit j), loaded with independent loads before they are needed (WaveRegs c0 / c1 / ...)
template <int CIT, class Regs>
__device__ __forceinline__ void load_cn_regs(const icrl_costnet_t& cn, const CnLayout& L, Regs& R) {
  const int lane = threadIdx.x & 63;
  const float* PT = cn.params_t;
  const int j1 = lane < L.H1 ? lane : 0, j2 = lane < L.H2 ? lane : 0;
#pragma unroll
  for (int k = 0; k < 16 * CIT; ++k) R.c0[k] = k < L.in ? PT[L.W0 + k * L.H1 + j1] : 0.f;
#pragma unroll
  for (int k = 0; k < MAX_H; ++k) R.c1[k] = (L.nh == 2 && k < L.H1) ? PT[L.W1 + k * L.H2 + j2] : 0.f;
  R.cb0 = PT[L.b0 + j1];
  R.cb1 = L.nh == 2 ? PT[L.b1 + j2] : 0.f;
  R.co = PT[L.Wo + j2];
  R.cbo = PT[L.bo];
#pragma unroll
  for (int i = 0; i < (16 * CIT + WAVE - 1) / WAVE; ++i) { const int idx = lane + i * WAVE; R.sel[i] = idx < L.in ? cn.select_dim[idx] : -1; }
}

// cost = 1 - sigmoid(ReLU-MLP(prepare(obs, acs))); called by ONE wave. obs_row: float64 raw obs (LDS or global),
// acs_row: float32 actions.  cx: >= 16*CIT floats (16-byte aligned), ch: [2][MAX_H].  Returns the cost in every lane.
template <int CIT, class Regs>
__device__ __forceinline__ float cost_forward_wave(const icrl_costnet_t& cn, const CnLayout& L, const Regs& R,
                                                   const double* obs_row, const float* acs_row, float* cx, float (*ch)[MAX_H],
                                                   int mode = 0 /* 0: cost = 1 - zeta; 1: zeta; 2: log(zeta + eps) */) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int i = 0; i < (16 * CIT + WAVE - 1) / WAVE; ++i) {
    const int idx = lane + i * WAVE;
    const int sel = R.sel[i];
    float v = 0.f;
    if (sel >= 0) {
      if (sel < cn.obs_dim) {
        double o = obs_row[sel];
        if (cn.obs_mean != nullptr && cn.obs_var != nullptr) o = (o - cn.obs_mean[sel]) / sqrt(cn.obs_var[sel] + cn.eps);
        if (cn.clip_obs >= 0.0) o = fmin(fmax(o, -cn.clip_obs), cn.clip_obs);
        v = (float)o;
      } else {
        const int a = sel - cn.obs_dim;
        float x;
        if (cn.is_discrete) x = ((int)acs_row[0] == a) ? 1.f : 0.f;
        else x = acs_row[a];
        if (cn.action_low != nullptr && cn.action_high != nullptr) x = fminf(fmaxf(x, cn.action_low[a]), cn.action_high[a]);
        v = x;
      }
    }
    if (idx < 16 * CIT) cx[idx] = v;       // pad entries are written as 0
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): LDS writes of this wave visible to its own reads
  {
    f32x4 xs[4 * CIT];
#pragma unroll
    for (int i = 0; i < 4 * CIT; ++i) xs[i] = *reinterpret_cast<const f32x4*>(&cx[4 * i]);
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 16 * CIT; ++k) acc = fmaf(R.c0[k], xs[k >> 2][k & 3], acc);
    ch[0][lane] = lane < L.H1 ? fmaxf(acc + R.cb0, 0.f) : 0.f;
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0xC07F);
  int last = 0;
  if (L.nh == 2) {
    f32x4 hs[MAX_H / 4];
#pragma unroll
    for (int i = 0; i < MAX_H / 4; ++i) hs[i] = *reinterpret_cast<const f32x4*>(&ch[0][4 * i]);
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < MAX_H; ++k) acc = fmaf(R.c1[k], hs[k >> 2][k & 3], acc);
    ch[1][lane] = lane < L.H2 ? fmaxf(acc + R.cb1, 0.f) : 0.f;
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xC07F);
    last = 1;
  }
  float part = lane < L.H2 ? R.co * ch[last][lane] : 0.f;
  const float z = wave_sum_fast(part) + R.cbo;
  const float zeta = 1.f / (1.f + expf(-z));
  if (mode == 1) return zeta;
  if (mode == 2) return logf(zeta + (float)cn.eps);
  return 1.f - zeta;
}

// synthetic env step for env n; called by ONE wave.  act: float32 clipped actions (LDS or global).
// Returns reward / done in every lane; writes env.s, t_ep, step_count.  s_old: float64 previous state (LDS copy).
// observation an env (re)starts from: the synthetic envs draw it from their stream, LapGridWorld always starts in cell 0
// POINT = false: the kernels that do not serve the Point envs (see env_step_wave)
template <bool POINT = true>
__device__ __forceinline__ double env_reset_value(const icrl_env_t& e, uint32_t key, uint32_t ctr, int i) {
  // the Point envs: init_qpos = init_qvel = 0, reset noise scale 0 (point.py:147-160); the Two Bridges envs: the start position,
  // (3, 5) for DDCDD2B and (0, 0) otherwise (two_bridges.py:80-86,323-328), the continuous ones zeros (:344-356)
  if (POINT && e.reward_form >= 4) return e.reward_form == 12 ? (i == 0 ? 3.0 : 5.0) : 0.0;
  if (e.reward_form >= 2) return -1.0;   // ((0 - 0) * 2) / 40 - 1
  return (unit_uniform(key, ctr, (uint32_t)(e.obs_dim + i)) - 0.5) * 0.2;
}

// LapGridWorld / ConstrainedLapGridWorld (ref: custom_envs/custom_envs/envs/lap_grid_world.py:62-119,197-240; spec:
// oracle/lap_grid.py): 40 cells, coins worth 3 at 5/15/25/35, action 0 forward / 1 backward, 200-step episodes.
// The state IS the observation 2*pos/40 - 1 (float64), so the cell index is recovered exactly by rounding.
__device__ __forceinline__ void lap_grid_step_wave(const icrl_env_t& e, int n, const double* s_old, const float* act,
                                                   uint32_t& ctr_io, int& tep_io, double* s_new_lds, double& reward,
                                                   int& done) {
  const int lane = threadIdx.x & 63;
  const int pos_old = (int)llrint((s_old[0] + 1.0) * 20.0);
  const int ac = (int)act[0];
  int pos = pos_old, d = 0;
  double rew;
  if (ac == 0) {
    pos = pos_old + 1 == 40 ? 0 : pos_old + 1;
    rew = (pos % 10 == 5) ? 3.0 : 0.0;
  } else if (e.reward_form == 3) {   // constrained: moving backward is penalised and ends the episode
    rew = -1.0;
    d = 1;
  } else {
    pos = pos_old == 0 ? 39 : pos_old - 1;
    rew = (pos % 10 == 5) ? 3.0 : 0.0;
  }
  const int tep = tep_io + 1;
  if (tep >= e.max_steps) d = 1;
  if (d) pos = 0;
  const double v = ((double)pos * 2.0) / 40.0 - 1.0;
  tep_io = d ? 0 : tep;
  ctr_io = ctr_io + 1u;
  if (lane == 0) {
    e.s[n] = v;
    if (s_new_lds != nullptr) s_new_lds[0] = v;
    e.t_ep[n] = tep_io;
    e.step_count[n] = ctr_io;
  }
  reward = rew;
  done = d;
}

struct PointStep { double rew; int done; };
// The Two Bridges envs (ref: custom_envs/custom_envs/envs/two_bridges.py:94-117,251-311,358-410 and envs/utils.py:9-69; reward_form
// 10 DD2B, 11 CDD2B, 12 DDCDD2B: obs (x, y), the action is the index 0..3 as a float; 13 C2B, 14 CC2B: obs (x, y, ori), two actions
// clipped to +-2).  A 20 x 20 field, three water rectangles that leave two bridges, on forms 11 / 12 / 14 the constraint
// rectangle over the lower bridge.  float64, one rounding per operation, the reference's operation order; the segment tests compare
// the orientation value with 0 exactly as the reference does (the discrete agent walks along lattice lines: the collinear cases count).
// None of the envs ends an episode itself: gym's TimeLimit does.  An action index outside 0..3 moves nowhere (the reference raises
// a KeyError there).
__device__ __forceinline__ int bridge_orientation(double p0, double p1, double q0, double q1, double r0, double r1) {
  const double val = ((q1 - p1) * (r0 - q0)) - ((q0 - p0) * (r1 - q1));      // utils.py:15-20
  return val == 0.0 ? 0 : (val > 0.0 ? 1 : -1);
}
__device__ __forceinline__ bool bridge_on_segment(double p0, double p1, double q0, double q1, double r0, double r1) {      // :9-13
  return r0 <= fmax(p0, q0) && r0 >= fmin(p0, q0) && r1 <= fmax(p1, q1) && r1 >= fmin(p1, q1);
}
// in_regions for ONE rectangle (origin (ox, oy), width w, height h): an end point strictly inside, or the move meets a boundary segment
__device__ __forceinline__ bool bridge_in_region(double sx, double sy, double nx, double ny, double ox, double oy, double w, double h) {
  const double x1 = ox + w, y1 = oy + h;
  if (sx > ox && sx < x1 && sy > oy && sy < y1) return true;      // :62-69, strict
  if (nx > ox && nx < x1 && ny > oy && ny < y1) return true;
  bool hit = false;
#pragma unroll 1
  for (int b = 0; b < 4; ++b) {                                    // boundaries(): bottom, left, right, top (:53-60)
    const double bp0 = b == 2 ? x1 : ox, bp1 = b == 3 ? y1 : oy;
    const double bq0 = b == 1 ? ox : x1, bq1 = b == 0 ? oy : y1;
    const int o1 = bridge_orientation(sx, sy, nx, ny, bp0, bp1);   // intersects((prev, next), bound) (:22-37)
    const int o2 = bridge_orientation(sx, sy, nx, ny, bq0, bq1);
    const int o3 = bridge_orientation(bp0, bp1, bq0, bq1, sx, sy);
    const int o4 = bridge_orientation(bp0, bp1, bq0, bq1, nx, ny);
    if (o1 != o2 && o3 != o4) hit = true;
    if (o1 == 0 && bridge_on_segment(sx, sy, nx, ny, bp0, bp1)) hit = true;
    if (o2 == 0 && bridge_on_segment(sx, sy, nx, ny, bq0, bq1)) hit = true;
    if (o3 == 0 && bridge_on_segment(bp0, bp1, bq0, bq1, sx, sy)) hit = true;
    if (o4 == 0 && bridge_on_segment(bp0, bp1, bq0, bq1, nx, ny)) hit = true;
  }
  return hit;
}
// Every lane computes the env's whole step; lane i < obs_dim stores component i.  Not inlined, arguments by value, (reward, done) back
// in registers: point_step_wave's conventions and reasons.
__device__ __noinline__ PointStep bridge_step_wave(int form, int max_steps, double* s_all, int32_t* t_ep_all, uint32_t* step_count_all,
                                                   int n, double x0, double y0, double ori0, float act0, float act1, uint32_t ctr_new,
                                                   int tep, double* s_new_lds) {
  const int lane = threadIdx.x & 63;
  const bool cont = form >= 13;
  double nx, ny, ori = 0.0;
  if (cont) {
    const double a0 = fmin(fmax((double)act0, -2.0), 2.0);         // two_bridges.py:359
    const double a1 = fmin(fmax((double)act1, -2.0), 2.0);
    ori = ori0 + a1;                                               // :362-363 (kept when the move is rejected)
    double sn, cs;
    sincos(ori, &sn, &cs);
    const double dx = cs * a0, dy = sn * a0;                       // :364-365
    nx = fmin(fmax(x0 + dx, -20.0), 20.0);                         // :369-370
    ny = fmin(fmax(y0 + dy, -20.0), 20.0);
  } else {
    const int ix = (int)act0;                                      // :244-247: 0.7 * {(1, 0), (-1, 0), (0, 1), (0, -1)}
    const double mx = ix == 0 ? 0.7 : (ix == 1 ? -0.7 : 0.0), my = ix == 2 ? 0.7 : (ix == 3 ? -0.7 : 0.0);
    nx = rint((x0 + mx) * 1e6) / 1e6;                              // np.around(state + action, 6) (:281)
    ny = rint((y0 + my) * 1e6) / 1e6;
  }
  bool rejected = fmin(nx, ny) < 0.0 || fmax(nx, ny) > 20.0;       // :283, :382
  const int n_regions = (form == 10 || form == 13) ? 3 : 4;        // water ((4,0),4,5), ((4,6),4,8), ((4,15),4,5); constraint ((4,5),4,1)
#pragma unroll 1
  for (int r = 0; r < n_regions; ++r) {
    const double oy = r == 0 ? 0.0 : (r == 1 ? 6.0 : (r == 2 ? 15.0 : 5.0)), h = r == 1 ? 8.0 : (r == 3 ? 1.0 : 5.0);
    if (!rejected && bridge_in_region(x0, y0, nx, ny, 4.0, oy, 4.0, h)) rejected = true;
  }
  double rew;
  if (rejected) {                                                  // back in the same spot (:286-289)
    nx = x0; ny = y0; rew = -2.0;
  } else {
    const double gx = 20.0 - nx, gy = 0.0 - ny;
    const double d2 = gx * gx + gy * gy;
    if (d2 < 1.0) rew = cont ? 250.0 : 12.0;                       // the goal: no end of the episode (:291-296, :390-393)
    else if (nx > 4.0) {                                           // the right half (:298-306, :397-405)
      rew = 10.0 / sqrt(d2);
      if (cont && ny < 6.0) rew = rew * 20.0;
    } else rew = -1.0;                                             // the left half
  }
  const int d = tep >= max_steps ? 1 : 0;                          // gym's TimeLimit: the reward is kept
  const int O = cont ? 3 : 2;
  if (lane < O) {
    double v = lane == 0 ? nx : (lane == 1 ? ny : ori);
    if (d) v = form == 12 ? (lane == 0 ? 3.0 : 5.0) : 0.0;         // on done: the start position (env_reset_value)
    as_global(s_all)[(size_t)n * O + lane] = v;
    if (s_new_lds != nullptr) s_new_lds[lane] = v;
  }
  if (lane == 0) {
    as_global(t_ep_all)[n] = d ? 0 : tep;
    as_global(step_count_all)[n] = ctr_new;
  }
  return PointStep{rew, d};
}

// The Point envs (ref: custom_envs/custom_envs/envs/point.py:22-376; reward_form 4 PointCircle, 5 PointCircleTest,
// 6 PointCircleTestBack, 7 PointNullReward, 8 PointNullRewardTest, 9 PointTrack; obs 9 = qpos (x, y, ori), qvel (0, 0, 0), torso position
// (x, y, 0)): closed-form kinematics in float64, one rounding per operation, the reference's operation order.
// Every lane computes the env's whole step; lane i < 9 stores component i.  Not inlined: the double-precision sincos is a long
// sequence that would otherwise enter the register allocation of every rollout kernel; so the env's scalars and arrays come in
// by value, as for env_step_wave3, and the reward / done pair comes back in registers.
__device__ __noinline__ PointStep point_step_wave(int form, int max_steps, double* s_all, int32_t* t_ep_all, uint32_t* step_count_all,
                                                  int n, double x0, double y0, double ori0, float act0, float act1, uint32_t ctr_new,
                                                  int tep, double* s_new_lds) {
  // the Two Bridges forms: their own callee, same signature.  musttail: a jump, not a call, so this function keeps no return address
  // and has no stack frame (without it the compiler calls and spills one register: 16 bytes of scratch in every caller)
  if (form >= 10) [[clang::musttail]] return bridge_step_wave(form, max_steps, s_all, t_ep_all, step_count_all, n, x0, y0, form >= 13 ? ori0 : 0.0, act0, act1, ctr_new, tep, s_new_lds);
  const int lane = threadIdx.x & 63;
  const double a0 = fmin(fmax((double)act0, -0.25), 0.25);         // point.py:167
  const double a1 = fmin(fmax((double)act1, -0.25), 0.25);
  const double ori = ori0 + a1;                                    // :169-170
  double sn, cs;
  sincos(ori, &sn, &cs);
  const double dx = cs * a0, dy = sn * a0;                         // :173-174
  const double x = fmin(fmax(x0 + dx, -40.0), 40.0);               // :177-178
  const double y = fmin(fmax(y0 + dy, -40.0), 40.0);
  double rew = 1.0;                                                // the null reward (:82)
  if (form <= 6) {                                                 // the circle reward (:185-186)
    const double num = y * dx - x * dy;
    rew = num / (1.0 + fabs(sqrt(x * x + y * y) - 10.0));
  } else if (form == 9) {                                          // PointTrack: movement + track reward, ctrl weight 0.0 (:353-368)
    const double ctrl = a0 * a0 + a1 * a1;
    const double track = fabs(sqrt(x * x + y * y) - 10.0) < 2.0 ? 1.0 : 0.0;
    rew = (((-y) * dx + x * dy) + track) + 0.0 * ctrl;
  }
  int d = 0;
  // STRICT inequalities (:98, :230, :266): x == -3 does not end the episode
  if ((form == 5 || form == 8) && (x > 3.0 || x < -3.0)) { d = 1; if (form == 5) rew = 0.0; }
  if (form == 6 && x < -3.0) { d = 1; rew = 0.0; }
  if (tep >= max_steps) d = 1;                                     // gym's TimeLimit: the reward is kept
  if (lane < 9) {
    double v = 0.0;                                                // on done: reset to all zeros (:147-160, noise scale 0)
    if (!d) v = (lane == 0 || lane == 6) ? x : (lane == 1 || lane == 7) ? y : lane == 2 ? ori : 0.0;
    as_global(s_all)[(size_t)n * 9 + lane] = v;
    if (s_new_lds != nullptr) s_new_lds[lane] = v;
  }
  if (lane == 0) {
    as_global(t_ep_all)[n] = d ? 0 : tep;
    as_global(step_count_all)[n] = ctr_new;
  }
  return PointStep{rew, d};
}

// POINT = false: without the branch to the Point step.  Even a never-taken call constrains the register allocation of its caller
// (values that live across it must avoid what the callee clobbers): rollout_persistent_kernel, whose step loop is tuned at HC shapes
// with every register in use, measured 8.2 instead of 8.0 us per step with it, and the chained episode kernel is part of the same
// headline; both are built without it, and the host routes the Point envs past them (icrl_rollout_collect: the multi-env kernel or
// the per-step launches; icrl_sample_episodes_chain refuses, the caller then settles the positions pass by pass).
template <bool POINT = true>
__device__ __forceinline__ void env_step_wave(const icrl_env_t& e, int n, const double* s_old, const float* act,
                                              uint32_t key, uint32_t& ctr_io, int& tep_io, double* s_new_lds,
                                              double& reward, int& done) {
  if (POINT && e.reward_form >= 4) {
    const int tep = tep_io + 1;
    ctr_io = ctr_io + 1u;
    // (one call site: the Two Bridges forms branch on inside the callee, so that a caller saves and restores its live registers around
    // one call, as before them; a discrete bridge env has no second action, and its s_old[2] is an unused LDS word)
    const PointStep r = point_step_wave(e.reward_form, e.max_steps, e.s, e.t_ep, e.step_count, n, s_old[0], s_old[1], s_old[2],
                                        act[0], e.act_dim > 1 ? act[1] : 0.f, ctr_io, tep, s_new_lds);
    tep_io = r.done ? 0 : tep;
    reward = r.rew;
    done = r.done;
    return;
  }
  if (e.reward_form >= 2) {
    lap_grid_step_wave(e, n, s_old, act, ctr_io, tep_io, s_new_lds, reward, done);
    return;
  }
  const int lane = threadIdx.x & 63;
  const int O = e.obs_dim, A = e.act_dim;
  double a[MAX_ACT];
  double sq = 0.0;
#pragma unroll
  for (int j = 0; j < MAX_ACT; ++j) {
    a[j] = 0.0;
    if (j < A) {
      a[j] = (double)act[j];
      if (e.broken && j >= 4) a[j] = 0.0;
      sq = sq + a[j] * a[j];
    }
  }
  const uint32_t ctr = ctr_io;
  double ns[2];  // this lane's components i = lane, lane + 64
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int i = lane + r * WAVE;
    ns[r] = 0.0;
    if (i < O) {
      double acc = 0.99 * s_old[i];
      const double* Bi = e.B + (size_t)i * A;
#pragma unroll
      for (int j = 0; j < MAX_ACT; ++j)
        if (j < A) acc = acc + Bi[j] * a[j];
      const double eps = (unit_uniform(key, ctr, (uint32_t)i) - 0.5) * 3.4641016151377544;
      ns[r] = acc + 0.01 * eps;
    }
  }
  const double n0 = __shfl(ns[0], 0, 64);
  const double n1 = __shfl(ns[0], 1, 64);
  double rew;
  if (e.reward_form == 0) rew = fabs(n0 - s_old[0]) / 0.05 - 0.1 * sq;
  else rew = (sqrt(n0 * n0 + n1 * n1) + 1.0) - 0.5 * sq;
  int d = 0;
  if (e.wall_terminate && n0 <= -3.0) { rew = 0.0; d = 1; }
  const int tep = tep_io + 1;
  if (tep >= e.max_steps) d = 1;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int i = lane + r * WAVE;
    if (i < O) {
      double v = ns[r];
      if (d) v = env_reset_value<false>(e, key, ctr + 1u, i);   // auto-reset draw (the Point envs returned above)
      e.s[(size_t)n * O + i] = v;
      if (s_new_lds != nullptr) s_new_lds[i] = v;
    }
  }
  tep_io = d ? 0 : tep;
  ctr_io = ctr + 1u;
  if (lane == 0) {
    e.t_ep[n] = tep_io;
    e.step_count[n] = ctr_io;
  }
  reward = rew;
  done = d;
}

// =================================================================================================================
// kernel A: policy forward + env step + cost + pre-normaliser buffer fields, one workgroup per env (ActStepArgs: rollout_launch.h)
// =================================================================================================================
// DISC: the constraint net read as D = zeta (icrl_cost_disc_t, cost_fn.h) — a compile-time form of cost_forward_wave's `mode` in every
// rollout kernel: the forms that existed before it keep their device code, symbol for symbol.  Where a family's kernels are wrappers
// around a shared body (one workgroup per env, generic, multi) the D form is a wrapper of its own name around the body with DISC = true.
// Here, in rollout_wide_kernel and in host_step_kernel the kernel IS the body (moving it into a by-reference body function changed the
// register allocation of all 18 shipped instantiations), so the D form is the same kernel instantiated with CIT | CIT_DISC.
constexpr int CIT_DISC = 0x100;
// REGION: a region cost (icrl_cost_region_t, cost_fn.h) in the cost wave of the CIT == 0 image, a compile-time form in the same two
// manners: CIT_REGION on the kernels that are their bodies, wrappers of their own names around a trailing `bool REGION` elsewhere.  The
// clause table is copied from the descriptor's device pointer into LDS once, before the step loop (REGION_TABLE: the array exists in
// the REGION instantiations alone), and the cost wave calls cost_region_wave where it called cost_fn_wave.
constexpr int CIT_REGION = 0x200;
#define REGION_TABLE(a_, tid_, threads_)                                                  \
  icrl_region_clause_t* rtab = nullptr;                                                   \
  if constexpr (REGION) {                                                                 \
    __shared__ icrl_region_clause_t rtab_s[ICRL_REGION_MAX_CLAUSES];                      \
    rtab = rtab_s;                                                                        \
    region_table_load(rtab_s, (a_).cr, (tid_), (threads_));                               \
  }
template <int OCT, int CITF>
__global__ void __launch_bounds__(256) act_step_kernel(ActStepArgs a, int t) {
  constexpr int CIT = CITF & 0xff;                     // the cost-net image proper
  constexpr bool DISC = (CITF & CIT_DISC) != 0;        // the constraint net read as D = zeta (icrl_cost_disc_t)
  constexpr bool REGION = (CITF & CIT_REGION) != 0;    // a region cost (icrl_cost_region_t) on the CIT == 0 image
  __shared__ ActShared sh;
  REGION_TABLE(a, (int)threadIdx.x, 256)      // (the barrier behind the observation load below publishes it)
  WaveRegs<OCT, CIT> R;                // one image: policy weights in waves 0..2, cost-net weights in wave 3
  WaveRegs<OCT, CIT>& C = R;
  load_pol_regs<OCT>(a.pl, a.PT, R);   // every weight load of the step is in flight before anything waits
  if constexpr (CIT > 0) { if (threadIdx.x >= 192 && a.has_cn) load_cn_regs<CIT>(a.cn, a.cl, C); }   // wave 3 = cost net
  const icrl_cost_fn_t cf = a.cf;      // analytic cost (CIT == 0): kind, index and thresholds are read once, before the step loop
  const int n = blockIdx.x;
  const uint32_t e_key = a.env.key[n];
  uint32_t e_ctr = a.env.step_count[n];
  int e_tep = a.env.t_ep[n];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int O = a.pl.O, A = a.pl.A, N = a.env.n_envs;
  const int AS = a.buf.act_store;
  for (int i = tid; i < MAX_OBS; i += 256) {
    sh.x[i] = i < O ? (float)a.ag.last_obs[(size_t)n * O + i] : 0.f;     // preprocess_obs: .float(); pad = 0
    if (i < O) sh.s_old[i] = a.env.s[(size_t)n * O + i];
  }
  __syncthreads();
  const size_t tn = (size_t)t * N + n;
  const float* noise_row = a.noise + tn * (a.pl.discrete ? 1 : A);
  policy_forward_block<OCT>(a.pl, R, sh, noise_row, 0, a.alow, a.ahigh);
  __syncthreads();
  if (w == 0) {
    double rew; int done;
    env_step_wave(a.env, n, sh.s_old, sh.act_clip, e_key, e_ctr, e_tep, sh.s_new, rew, done);
    float* nob = a.buf.new_orig_observations + tn * O;
    for (int i = lane; i < O; i += WAVE) nob[i] = (float)sh.s_new[i];
    if (lane == 0) {
      a.ag.raw_rew[n] = rew; a.ag.dones[n] = (uint8_t)done;
      if (a.raw_plane != nullptr) a.raw_plane[tn] = rew;
    }
  } else if (w == 3) {
    float cost = 0.f;
    if constexpr (REGION) cost = cost_region_wave(rtab, a.cr.n_clauses, a.cr.combine, sh.s_old, sh.act_clip, O);
    else if constexpr (CIT == 0) cost = cost_fn_wave(cf, sh.s_old, sh.act_clip);
    else if (a.has_cn) cost = cost_forward_wave<CIT>(a.cn, a.cl, C, sh.s_old, sh.act_clip, sh.cx, sh.ch, DISC ? 1 : 0);
    if (lane == 0) { a.ag.raw_cost[n] = cost; a.buf.orig_costs[tn] = cost; }
  } else if (w == 2) {
    float* ob = a.buf.observations + tn * O;
    float* oob = a.buf.orig_observations + tn * O;
    for (int i = lane; i < O; i += WAVE) { ob[i] = sh.x[i]; oob[i] = (float)sh.s_old[i]; }
    if (lane < AS) a.buf.actions[tn * AS + lane] = sh.act_raw[lane];
    if (lane < A && !a.pl.discrete) a.ag.act_clipped[(size_t)n * A + lane] = sh.act_clip[lane];
    if (lane == 0) {
      a.buf.dones[tn] = (float)a.ag.last_dones[n];
      a.buf.reward_values[tn] = sh.scal[0];
      a.buf.cost_values[tn] = sh.scal[1];
      a.buf.log_probs[tn] = sh.scal[2];
      a.ag.last_v_r[n] = sh.scal[0];
      a.ag.last_v_c[n] = sh.scal[1];
    }
  }
}

__device__ __forceinline__ int sde_draw_of(int t, int sample_freq) { return sample_freq > 0 ? t / sample_freq : 0; }

// The head of policy_forward_sde_kernel on wave 0, behind policy_forward_block(deterministic = 1): sh.act_raw holds the mean and sh.g[0] the
// latent, both written by this wave (the latent before a workgroup barrier).  Same arithmetic, term for term: float64 fma chains over the
// latent units in ascending order, action = (float)(mean + noise), the log-prob summed in action order, the clip to the action box.  Leaves
// sh.act_raw, sh.act_clip and sh.scal[2] for the env step, the cost wave and the buffer stores, which read them behind the caller's barrier.
// E: this env's current matrix (LDS or global); e2(i): exp(2 log_std) of entry i — evaluated per call, or read from the launch's LDS image.
template <class E2>
__device__ __forceinline__ void sde_head_wave(ActShared& sh, int A, int H2, const float* E, E2 e2, const float* alow, const float* ahigh) {
  const int lane = threadIdx.x & 63;
  double lp = 0.;
  if (lane < A) {
    const float mean = sh.act_raw[lane];
    double noise = 0., var = 0.;
#pragma unroll 8      // (the two chains stay sequential; unrolled, the operands of eight terms are fetched together)
    for (int h = 0; h < H2; ++h) {
      const double l = sh.g[0][h];
      noise = fma(l, (double)E[h * A + lane], noise);
      var = fma(l * l, e2(h * A + lane), var);
    }
    var += 1e-6;
    const float act = (float)((double)mean + noise);
    const double diff = (double)act - (double)mean;
    lp = -(diff * diff) / (2. * var) - 0.5 * log(var) - 0.918938533204672741780329736406;
    float clip = act;
    if (alow != nullptr && ahigh != nullptr) clip = fminf(fmaxf(act, alow[lane]), ahigh[lane]);
    sh.act_raw[lane] = act;
    sh.act_clip[lane] = clip;
  }
  double tot = 0.;      // in action order, every lane the same chain
  for (int a = 0; a < A; ++a) tot += __shfl(lp, a, 64);
  if (lane == 0) sh.scal[2] = (float)tot;
}

// act_step_kernel for a gSDE policy: the same step with the head above (exp per call, as policy_forward_sde_kernel does); a.pl / a.PT are
// the diagonal layout and the transposes of the network alone (launch_policy_forward_sde), a.noise is not read.  norm_step_kernel follows.
template <int OCT, int CIT>
__global__ void __launch_bounds__(256) act_step_sde_kernel(ActStepArgs a, SdeArgs sd, int t) {
  __shared__ ActShared sh;
  WaveRegs<OCT, CIT> R;
  WaveRegs<OCT, CIT>& C = R;
  load_pol_regs<OCT>(a.pl, a.PT, R);
  if constexpr (CIT > 0) { if (threadIdx.x >= 192 && a.has_cn) load_cn_regs<CIT>(a.cn, a.cl, C); }
  const icrl_cost_fn_t cf = a.cf;
  const int n = blockIdx.x;
  const uint32_t e_key = a.env.key[n];
  uint32_t e_ctr = a.env.step_count[n];
  int e_tep = a.env.t_ep[n];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int O = a.pl.O, A = a.pl.A, N = a.env.n_envs;
  const int AS = a.buf.act_store;
  for (int i = tid; i < MAX_OBS; i += 256) {
    sh.x[i] = i < O ? (float)a.ag.last_obs[(size_t)n * O + i] : 0.f;
    if (i < O) sh.s_old[i] = a.env.s[(size_t)n * O + i];
  }
  __syncthreads();
  const size_t tn = (size_t)t * N + n;
  policy_forward_block<OCT>(a.pl, R, sh, nullptr, 1, nullptr, nullptr);
  if (w == 0) {
    const float* E = sd.expl + (size_t)sde_draw_of(t, sd.sample_freq) * (size_t)sd.draw_stride + (size_t)n * (size_t)sd.env_stride;
    const float* __restrict__ ls = sd.ls;
    sde_head_wave(sh, A, a.pl.H2, E, [&](int i) { return exp(2. * (double)ls[i]); }, a.alow, a.ahigh);
  }
  __syncthreads();
  if (w == 0) {
    double rew; int done;
    env_step_wave(a.env, n, sh.s_old, sh.act_clip, e_key, e_ctr, e_tep, sh.s_new, rew, done);
    float* nob = a.buf.new_orig_observations + tn * O;
    for (int i = lane; i < O; i += WAVE) nob[i] = (float)sh.s_new[i];
    if (lane == 0) { a.ag.raw_rew[n] = rew; a.ag.dones[n] = (uint8_t)done; }
  } else if (w == 3) {
    float cost = 0.f;
    if constexpr (CIT == 0) cost = cost_fn_wave(cf, sh.s_old, sh.act_clip);
    else if (a.has_cn) cost = cost_forward_wave<CIT>(a.cn, a.cl, C, sh.s_old, sh.act_clip, sh.cx, sh.ch, 0);
    if (lane == 0) { a.ag.raw_cost[n] = cost; a.buf.orig_costs[tn] = cost; }
  } else if (w == 2) {
    float* ob = a.buf.observations + tn * O;
    float* oob = a.buf.orig_observations + tn * O;
    for (int i = lane; i < O; i += WAVE) { ob[i] = sh.x[i]; oob[i] = (float)sh.s_old[i]; }
    if (lane < AS) a.buf.actions[tn * AS + lane] = sh.act_raw[lane];
    if (lane < A) a.ag.act_clipped[(size_t)n * A + lane] = sh.act_clip[lane];
    if (lane == 0) {
      a.buf.dones[tn] = (float)a.ag.last_dones[n];
      a.buf.reward_values[tn] = sh.scal[0];
      a.buf.cost_values[tn] = sh.scal[1];
      a.buf.log_probs[tn] = sh.scal[2];
      a.ag.last_v_r[n] = sh.scal[0];
      a.ag.last_v_c[n] = sh.scal[1];
    }
  }
}

// act_step_kernel for policies / constraint nets the one-workgroup-per-env image does not hold (generic-shape path): the policy
// forward (policy_generic_kernel: actions, values, log-probs straight into row t of the buffer, clipped actions into ag.act_clipped)
// and the cost (cn_cost_rows_kernel: ag.raw_cost) have run as launches of their own on the same stream; this kernel is the rest
// of the step for env n — env step, the pre-normaliser buffer fields, the values of this forward for the GAE bootstrap.  One wave.
__global__ void __launch_bounds__(64) act_step_generic_kernel(GenStepArgs a, int t) {
  __shared__ double s_old[MAX_OBS], s_new[MAX_OBS];
  __shared__ float act_clip[MAX_ACT];
  const int n = blockIdx.x, lane = threadIdx.x;
  const int O = a.env.obs_dim, N = a.env.n_envs, AS = a.buf.act_store;
  const uint32_t e_key = a.env.key[n];
  uint32_t e_ctr = a.env.step_count[n];
  int e_tep = a.env.t_ep[n];
  const size_t tn = (size_t)t * N + n;
  float* ob = a.buf.observations + tn * O;
  float* oob = a.buf.orig_observations + tn * O;
  for (int i = lane; i < O; i += WAVE) {
    const double s = a.env.s[(size_t)n * O + i];
    s_old[i] = s;
    oob[i] = (float)s;
    ob[i] = (float)a.ag.last_obs[(size_t)n * O + i];      // preprocess_obs: .float()
  }
  if (lane < AS) act_clip[lane] = a.ag.act_clipped[(size_t)n * AS + lane];
  __syncthreads();
  double rew; int done;
  env_step_wave(a.env, n, s_old, act_clip, e_key, e_ctr, e_tep, s_new, rew, done);
  float* nob = a.buf.new_orig_observations + tn * O;
  for (int i = lane; i < O; i += WAVE) nob[i] = (float)s_new[i];
  if (lane == 0) {
    a.ag.raw_rew[n] = rew; a.ag.dones[n] = (uint8_t)done;
    if (a.raw_plane != nullptr) a.raw_plane[tn] = rew;
    const float cost = a.has_cn == 2 ? cost_fn_wave(a.cf, s_old, act_clip) : (a.has_cn ? a.ag.raw_cost[n] : 0.f);
    a.ag.raw_cost[n] = cost; a.buf.orig_costs[tn] = cost;
    a.buf.dones[tn] = (float)a.ag.last_dones[n];
    a.ag.last_v_r[n] = a.buf.reward_values[tn];
    a.ag.last_v_c[n] = a.buf.cost_values[tn];
  }
}

// =================================================================================================================
// kernel B: VecNormalizeWithCost.step_wait for all envs, one workgroup (NormStepArgs: rollout_launch.h)
// =================================================================================================================
// Chan merge with the reference's operation order (running_mean_std.py:25-39).
__device__ __forceinline__ void chan_merge(double& mean, double& var, double count, double b_mean, double b_var,
                                           double b_count) {
  const double delta = b_mean - mean;
  const double tot = count + b_count;
  const double new_mean = mean + delta * b_count / tot;
  const double m_a = var * count;
  const double m_b = b_var * b_count;
  const double m_2 = m_a + m_b + (delta * delta) * count * b_count / (count + b_count);
  mean = new_mean;
  var = m_2 / (count + b_count);
}

// ---- numpy-ordered 1-D sum, parallelised without changing the rounding order -------------------------------------
// np.sum of a contiguous float64 vector splits recursively (n2 = n/2 rounded down to a multiple of 8) until blocks of
// <= 128 elements, sums each block with 8 strided accumulators + a fixed combine tree + sequential tail, and adds the
// block results back up the recursion.  Blocks and accumulators are independent, so (block, accumulator) pairs map to
// threads; only the tiny combine runs on one thread.
struct NormShared {
  double chunk[NORM_CHUNK];
  double vec[2][NORM_MAX_N];                     // ret / cost_ret (then their squared deviations)
  double part[2][NORM_MAX_LEAVES][8];
  double leaf[2][NORM_MAX_LEAVES];
  double total[2];
  int leaf_off[NORM_MAX_LEAVES], leaf_len[NORM_MAX_LEAVES], n_leaves;
};

__device__ inline double np_combine(int l, const double* leaf, int& idx) {
  if (l <= 128) return leaf[idx++];
  int n2 = l / 2;
  n2 -= n2 % 8;
  const double a = np_combine(n2, leaf, idx);
  const double b = np_combine(l - n2, leaf, idx);
  return a + b;
}

// sums sh.vec[0][0:n] and (if two) sh.vec[1][0:n] into sh.total[]; all threads of the block must call.
__device__ inline void block_np_sum(NormShared& sh, int n, bool two) {
  const int tid = threadIdx.x, nt = blockDim.x;
  if (tid == 0) {
    int so[16], sl[16], sp = 1, cnt = 0;
    so[0] = 0; sl[0] = n;
    while (sp) {
      --sp;
      const int o = so[sp], l = sl[sp];
      if (l <= 128) { sh.leaf_off[cnt] = o; sh.leaf_len[cnt] = l; ++cnt; }
      else { int n2 = l / 2; n2 -= n2 % 8; so[sp] = o + n2; sl[sp] = l - n2; ++sp; so[sp] = o; sl[sp] = n2; ++sp; }
    }
    sh.n_leaves = cnt;
  }
  __syncthreads();
  const int nl = sh.n_leaves, nv = two ? 2 : 1;
  for (int job = tid; job < nv * nl * 8; job += nt) {
    const int v = job / (nl * 8), L = (job / 8) % nl, k = job % 8;
    const int o = sh.leaf_off[L], l = sh.leaf_len[L];
    const double* a = sh.vec[v] + o;
    if (l >= 8) {
      double r = a[k];
      for (int i = 8; i < l - (l % 8); i += 8) r += a[i + k];
      sh.part[v][L][k] = r;
    }
  }
  __syncthreads();
  for (int job = tid; job < nv * nl; job += nt) {
    const int v = job / nl, L = job % nl;
    const int o = sh.leaf_off[L], l = sh.leaf_len[L];
    const double* a = sh.vec[v] + o;
    double res;
    if (l < 8) {
      res = 0.0;
      for (int i = 0; i < l; ++i) res += a[i];
    } else {
      const double* r = sh.part[v][L];
      res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
      for (int i = l - (l % 8); i < l; ++i) res += a[i];
    }
    sh.leaf[v][L] = res;
  }
  __syncthreads();
  if (tid < nv) { int idx = 0; sh.total[tid] = np_combine(n, sh.leaf[tid], idx); }
  __syncthreads();
}

__global__ void __launch_bounds__(1024) norm_step_kernel(NormStepArgs a) {
  __shared__ NormShared sh;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int N = a.N, O = a.O;
  const icrl_norm_t& nm = a.nm;
  const bool has_cost = a.raw_cost != nullptr;
  if (nm.training) {
    // ---- discounted returns (vec_normalize.py:102-105, 245-248), then np.mean / np.var of them
    for (int n = tid; n < N; n += nt) {
      const double r = nm.ret[n] * nm.reward_gamma + a.raw_rew[n];
      nm.ret[n] = r; sh.vec[0][n] = r;
      if (has_cost) { const double c = nm.cost_ret[n] * nm.cost_gamma + (double)a.raw_cost[n]; nm.cost_ret[n] = c; sh.vec[1][n] = c; }
    }
    __syncthreads();
    block_np_sum(sh, N, has_cost);
    const double bm_r = sh.total[0] / (double)N, bm_c = sh.total[1] / (double)N;
    __syncthreads();
    for (int n = tid; n < N; n += nt) {
      const double d = sh.vec[0][n] - bm_r; sh.vec[0][n] = d * d;
      if (has_cost) { const double e = sh.vec[1][n] - bm_c; sh.vec[1][n] = e * e; }
    }
    __syncthreads();
    block_np_sum(sh, N, has_cost);
    if (tid == 0) {
      double m = nm.ret_stats[0], v = nm.ret_stats[1];
      chan_merge(m, v, nm.ret_stats[2], bm_r, sh.total[0] / (double)N, (double)N);
      nm.ret_stats[0] = m; nm.ret_stats[1] = v; nm.ret_stats[2] = (double)N + nm.ret_stats[2];
      if (has_cost) {
        m = nm.cost_stats[0]; v = nm.cost_stats[1];
        chan_merge(m, v, nm.cost_stats[2], bm_c, sh.total[1] / (double)N, (double)N);
        nm.cost_stats[0] = m; nm.cost_stats[1] = v; nm.cost_stats[2] = (double)N + nm.cost_stats[2];
      }
    }
    // ---- obs_rms.update: numpy's axis-0 reduction adds the rows in order; rows are staged through LDS in chunks
    // (coalesced, all threads) and one thread per column accumulates them sequentially.
    const int rows_per = NORM_CHUNK / O;
    double sum = 0.0, bm = 0.0;
    for (int pass = 0; pass < 2; ++pass) {
      sum = 0.0;
      for (int r0 = 0; r0 < N; r0 += rows_per) {
        const int rows = (N - r0) < rows_per ? (N - r0) : rows_per;
        __syncthreads();
        for (int i = tid; i < rows * O; i += nt) sh.chunk[i] = a.raw_obs[(size_t)r0 * O + i];
        __syncthreads();
        if (tid < O) {
          if (pass == 0) for (int r = 0; r < rows; ++r) sum += sh.chunk[r * O + tid];
          else for (int r = 0; r < rows; ++r) { const double d = sh.chunk[r * O + tid] - bm; sum += d * d; }
        }
      }
      if (pass == 0) bm = sum / (double)N;
    }
    if (tid < O) {
      double m = nm.obs_mean[tid], v = nm.obs_var[tid];
      chan_merge(m, v, nm.obs_count[0], bm, sum / (double)N, (double)N);
      nm.obs_mean[tid] = m; nm.obs_var[tid] = v;
    }
    __syncthreads();
    if (tid == 0) nm.obs_count[0] = (double)N + nm.obs_count[0];
    __threadfence_block();
    __syncthreads();
  }
  // ---- normalise + clip (vec_normalize.py:107-123, 254-261)
  for (int idx = tid; idx < N * O; idx += nt) {
    const int j = idx % O;
    double o = a.raw_obs[idx];
    if (nm.norm_obs) o = fmin(fmax((o - nm.obs_mean[j]) / sqrt(nm.obs_var[j] + nm.epsilon), -nm.clip_obs), nm.clip_obs);
    if (a.obs_out) a.obs_out[idx] = o;
    if (a.obs_f32) a.obs_f32[idx] = (float)o;
  }
  const double rden = sqrt(nm.ret_stats[1] + nm.epsilon);
  const double cden = sqrt(nm.cost_stats[1] + nm.epsilon);
  for (int n = tid; n < N; n += nt) {
    double r = a.raw_rew[n];
    if (nm.norm_reward) r = fmin(fmax(r / rden, -nm.clip_reward), nm.clip_reward);
    if (a.rew_out) a.rew_out[n] = r;
    if (a.rew_f32) a.rew_f32[n] = (float)r;
    const int d = a.dones[n];
    if (d) nm.ret[n] = 0.0;
    if (has_cost) {
      double c = (double)a.raw_cost[n];
      if (nm.norm_cost) c = fmin(fmax(c / cden, -nm.clip_cost), nm.clip_cost);
      if (a.cost_out) a.cost_out[n] = c;
      if (a.cost_f32) a.cost_f32[n] = (float)c;
      if (d) nm.cost_ret[n] = 0.0;
    }
    if (a.last_dones) a.last_dones[n] = (uint8_t)d;
  }
}

// ---- small-problem variant (N <= 128, N*O <= NORM_CHUNK: e.g. HCWithPos with 64 envs): every input is pulled into LDS /
// registers with ONE round of global loads, the three statistics are computed concurrently by different waves
// (observation columns: threads < O; reward return: wave 15; cost return: wave 14 — for N <= 128 numpy's pairwise sum is a
// single 8-accumulator leaf, which 8 lanes reproduce exactly), one barrier, then everything is normalised from LDS.
// numpy's pairwise sum for n in {128, 256, 512, 1024} (leaves of exactly 128, a balanced tree above them), evaluated by one
// wave: lane 8 L + k owns accumulator k of leaf L (a 16-add chain instead of n adds in every lane); the xor butterflies
// reproduce the leaf's ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) and the recursion's left + right (float64 addition is commutative
// bit for bit, so only the association matters).  Result in every lane.  Other n: np_pairwise_sum (common.h).
__device__ __forceinline__ double np_pairwise_sum_wave(const double* a, int n) {
  const int leaves = n >> 7;
  if ((n & 127) != 0 || (leaves & (leaves - 1)) != 0 || leaves > 8) return np_pairwise_sum(a, n);
  const int lane = threadIdx.x & 63;
  const int L = lane >> 3, k = lane & 7;
  const double* p = a + 128 * (L < leaves ? L : 0) + k;
  double v[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) v[i] = p[8 * i];
  double r = v[0];
#pragma unroll
  for (int i = 1; i < 16; ++i) r += v[i];
  r += __shfl_xor(r, 1, 64);
  r += __shfl_xor(r, 2, 64);
  r += __shfl_xor(r, 4, 64);
  if (leaves >= 2) r += __shfl_xor(r, 8, 64);
  if (leaves >= 4) r += __shfl_xor(r, 16, 64);
  if (leaves >= 8) r += __shfl_xor(r, 32, 64);
  return __shfl(r, 0, 64);
}

__device__ __forceinline__ double np_leaf_sum_wave(const double* a, int n) {
  // numpy pairwise sum of n <= 128 contiguous doubles, evaluated by one wave; result valid in every lane
  const int lane = threadIdx.x & 63;
  if (n < 8) {
    double r = 0.0;
    for (int i = 0; i < n; ++i) r += a[i];
    return r;
  }
  double r = 0.0;
  if (lane < 8) {
    r = a[lane];
    for (int i = 8; i < n - (n % 8); i += 8) r += a[i + lane];
  }
  const double r0 = __shfl(r, 0, 64), r1 = __shfl(r, 1, 64), r2 = __shfl(r, 2, 64), r3 = __shfl(r, 3, 64);
  const double r4 = __shfl(r, 4, 64), r5 = __shfl(r, 5, 64), r6 = __shfl(r, 6, 64), r7 = __shfl(r, 7, 64);
  double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
  for (int i = n - (n % 8); i < n; ++i) res += a[i];
  return res;
}

// obs_rms.update's batch moments of one observation column, in numpy's axis-0 order (rows added one after the other — a serial
// float64 recurrence).  The LDS reads are issued sixteen at a time and only the additions stay on the dependent chain; left
// to itself the compiler pairs every read with its add and exposes the LDS latency 2 N times.
__device__ __forceinline__ void column_moments(const double* col, int stride, int N, double& bm, double& bv) {
  // two register batches in flight: the reads of batch k + 1 are issued before the additions of batch k
  auto load16 = [&](int r0, double (&v)[16]) {
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = col[(r0 + k < N ? r0 + k : N - 1) * stride];
  };
  double va[16], vb[16];
  double sum = 0.0;
  load16(0, va);
  for (int r0 = 0; r0 < N; r0 += 32) {
    load16(r0 + 16 < N ? r0 + 16 : 0, vb);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < 16; ++k) if (r0 + k < N) sum += va[k];
    load16(r0 + 32 < N ? r0 + 32 : 0, va);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < 16; ++k) if (r0 + 16 + k < N) sum += vb[k];
  }
  bm = sum / (double)N;
  double sq = 0.0;
  // (va holds rows 0..15 again: the last prefetch of the loop above wrapped around)
  for (int r0 = 0; r0 < N; r0 += 32) {
    load16(r0 + 16 < N ? r0 + 16 : 0, vb);
#pragma unroll
    for (int k = 0; k < 16; ++k) { const double d = va[k] - bm; va[k] = d * d; }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < 16; ++k) if (r0 + k < N) sq += va[k];
    load16(r0 + 32 < N ? r0 + 32 : 0, va);
#pragma unroll
    for (int k = 0; k < 16; ++k) { const double d = vb[k] - bm; vb[k] = d * d; }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < 16; ++k) if (r0 + 16 + k < N) sq += vb[k];
  }
  bv = sq / (double)N;
}

// the same moments for a column stored CONTIGUOUSLY (persistent rollout: the exchanged observations are transposed into LDS), so
// every read is a ds_read with an immediate offset from one running base; the column is padded with >= 32 readable entries.
__device__ __forceinline__ void column_moments_contig(const double* col, int N, double& bm, double& bv) {
  // One dependent float64 add per row is the floor (numpy's axis-0 order is a single chain); everything else stays off that
  // chain: rows are fetched 16 at a time one batch ahead, and only the last, partial block of 32 carries the `row < N` selects
  // (a select per row on the chain costs more than the add itself).
  double va[16], vb[16];
  double sum = 0.0;
  const int NF = N & ~31;              // rows in full blocks of 32
#pragma unroll
  for (int k = 0; k < 16; ++k) va[k] = col[k];
  int r0 = 0;
  for (; r0 < NF; r0 += 32) {
#pragma unroll
    for (int k = 0; k < 16; ++k) vb[k] = col[r0 + 16 + k];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < 16; ++k) sum += va[k];
#pragma unroll
    for (int k = 0; k < 16; ++k) va[k] = col[r0 + 32 + k];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < 16; ++k) sum += vb[k];
  }
  if (r0 < N) {
#pragma unroll
    for (int k = 0; k < 16; ++k) vb[k] = col[r0 + 16 + k];
#pragma unroll
    for (int k = 0; k < 16; ++k) if (r0 + k < N) sum += va[k];
#pragma unroll
    for (int k = 0; k < 16; ++k) if (r0 + 16 + k < N) sum += vb[k];
  }
  bm = sum / (double)N;
  double sq = 0.0;
#pragma unroll
  for (int k = 0; k < 16; ++k) va[k] = col[k];
  for (r0 = 0; r0 < NF; r0 += 32) {
#pragma unroll
    for (int k = 0; k < 16; ++k) vb[k] = col[r0 + 16 + k];
#pragma unroll
    for (int k = 0; k < 16; ++k) { const double d = va[k] - bm; va[k] = d * d; }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < 16; ++k) sq += va[k];
#pragma unroll
    for (int k = 0; k < 16; ++k) va[k] = col[r0 + 32 + k];
#pragma unroll
    for (int k = 0; k < 16; ++k) { const double d = vb[k] - bm; vb[k] = d * d; }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < 16; ++k) sq += vb[k];
  }
  if (r0 < N) {
#pragma unroll
    for (int k = 0; k < 16; ++k) vb[k] = col[r0 + 16 + k];
#pragma unroll
    for (int k = 0; k < 16; ++k) { const double d = va[k] - bm; va[k] = d * d; }
#pragma unroll
    for (int k = 0; k < 16; ++k) { const double d = vb[k] - bm; vb[k] = d * d; }
#pragma unroll
    for (int k = 0; k < 16; ++k) if (r0 + k < N) sq += va[k];
#pragma unroll
    for (int k = 0; k < 16; ++k) if (r0 + 16 + k < N) sq += vb[k];
  }
  bv = sq / (double)N;
}

__global__ void __launch_bounds__(1024) norm_step_small_kernel(NormStepArgs a) {
  __shared__ double chunk[NORM_CHUNK];
  __shared__ double vec[2][128], dev2[2][128];
  __shared__ double mean_s[MAX_OBS], var_s[MAX_OBS];
  __shared__ double dens[2];
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wv = tid >> 6;
  const int N = a.N, O = a.O;
  const icrl_norm_t& nm = a.nm;
  const bool has_cost = a.raw_cost != nullptr;
  // ---- one round of loads
  for (int i = tid; i < N * O; i += nt) chunk[i] = a.raw_obs[i];
  if (tid < N) {
    double r = nm.ret[tid], c = has_cost ? nm.cost_ret[tid] : 0.0;
    if (nm.training) {
      r = r * nm.reward_gamma + a.raw_rew[tid];
      if (has_cost) c = c * nm.cost_gamma + (double)a.raw_cost[tid];
    }
    vec[0][tid] = r; vec[1][tid] = c;
  }
  double o_mean = 0.0, o_var = 1.0, o_cnt = 0.0;
  if (tid < O) { o_mean = nm.obs_mean[tid]; o_var = nm.obs_var[tid]; o_cnt = nm.obs_count[0]; }
  __syncthreads();
  if (nm.training) {
    if (tid < O) {           // obs_rms.update: rows added in order (numpy's axis-0 reduction)
      double bm, bv;
      column_moments(chunk + tid, O, N, bm, bv);
      chan_merge(o_mean, o_var, o_cnt, bm, bv, (double)N);
      nm.obs_mean[tid] = o_mean; nm.obs_var[tid] = o_var;
      if (tid == 0) nm.obs_count[0] = (double)N + o_cnt;
    }
    if (wv == 15 || (wv == 14 && has_cost)) {     // ret_rms / cost_rms: numpy pairwise order
      const int v = wv == 15 ? 0 : 1;
      double* st = v == 0 ? nm.ret_stats : nm.cost_stats;
      const double bm = np_leaf_sum_wave(vec[v], N) / (double)N;
      for (int i = lane; i < N; i += 64) { const double d = vec[v][i] - bm; dev2[v][i] = d * d; }
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_s_waitcnt(0xC07F);
      const double bv = np_leaf_sum_wave(dev2[v], N) / (double)N;
      double m = st[0], var = st[1];
      const double cnt = st[2];
      chan_merge(m, var, cnt, bm, bv, (double)N);
      if (lane == 0) { st[0] = m; st[1] = var; st[2] = (double)N + cnt; }
      if (lane == 0) dens[v] = sqrt(var + nm.epsilon);
    }
  } else {
    if (tid == 0) { dens[0] = sqrt(nm.ret_stats[1] + nm.epsilon); dens[1] = sqrt(nm.cost_stats[1] + nm.epsilon); }
  }
  if (nm.training && !has_cost && tid == 0) dens[1] = sqrt(nm.cost_stats[1] + nm.epsilon);
  if (tid < O) { mean_s[tid] = o_mean; var_s[tid] = o_var; }
  __syncthreads();
  // ---- normalise + clip from LDS
  for (int idx = tid; idx < N * O; idx += nt) {
    const int j = idx % O;
    double o = chunk[idx];
    if (nm.norm_obs) o = fmin(fmax((o - mean_s[j]) / sqrt(var_s[j] + nm.epsilon), -nm.clip_obs), nm.clip_obs);
    if (a.obs_out) a.obs_out[idx] = o;
    if (a.obs_f32) a.obs_f32[idx] = (float)o;
  }
  if (tid < N) {
    const int n = tid;
    double r = a.raw_rew[n];
    if (nm.norm_reward) r = fmin(fmax(r / dens[0], -nm.clip_reward), nm.clip_reward);
    if (a.rew_out) a.rew_out[n] = r;
    if (a.rew_f32) a.rew_f32[n] = (float)r;
    const int d = a.dones[n];
    if (nm.training || d) nm.ret[n] = d ? 0.0 : vec[0][n];
    if (has_cost) {
      double c = (double)a.raw_cost[n];
      if (nm.norm_cost) c = fmin(fmax(c / dens[1], -nm.clip_cost), nm.clip_cost);
      if (a.cost_out) a.cost_out[n] = c;
      if (a.cost_f32) a.cost_f32[n] = (float)c;
      if (nm.training || d) nm.cost_ret[n] = d ? 0.0 : vec[1][n];
    }
    if (a.last_dones) a.last_dones[n] = (uint8_t)d;
  }
}

// =================================================================================================================
// persistent rollout: ALL T steps of collect_rollouts in one launch (N <= 128 envs, N * obs <= NORM_CHUNK)
//
// One workgroup per env runs kernel A's work for its env; the normaliser needs every env's raw observation / reward / cost of
// the step, so the workgroups exchange them through global memory and meet at ONE device-wide barrier per step.  After
// the barrier EVERY workgroup evaluates kernel B's statistics update redundantly — same inputs, same (numpy) summation order,
// hence bit-identical replicas of obs_rms / ret_rms / cost_rms / ret / cost_ret in each workgroup's registers and LDS — and
// normalises only its own env.  The exchange arrays are double-buffered by step parity, which is what makes a single barrier
// per step sufficient (a workgroup can be at most one phase ahead of the slowest one).  Policy / cost-net weights, the
// dynamics matrix and the replicated statistics are loaded once for the whole rollout.
// =================================================================================================================
// diagnostic: cycles per phase of workgroup 0 of the last persistent rollout (policy+env | barrier | statistics), steps
constexpr int NORM_MAX_N_TRACE = 1024;
constexpr int CHAIN_TRACE_BASE = 4 * 128;      // g_wide_trace words behind those of the persistent rollout's (<= 128) workgroups: its chain timers
__device__ unsigned long long g_rollout_prof[8];
__device__ unsigned long long g_rollout_prof_wide[16];
__device__ unsigned long long g_wide_trace[NORM_MAX_N_TRACE * 4];   // per workgroup, one step: s_memrealtime at phase-A end / gather end / publish / statistics read     // rollout_wide_kernel: [0..7] wave 0, [8..15] wave 1 (owner) of the profiled workgroup
__device__ __forceinline__ unsigned long long prof_now() {
  unsigned long long t;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  return t;
}

// Exchange between the workgroups of the persistent rollout.  Every exchanged word is written and read with agent-scope
// relaxed atomics (write-through stores / cache-bypassing loads: cdna_hip_programming.md Guideline 16), so no bulk cache
// write-back / invalidate fence is needed — those cost ~4 us per step on this part.  Ordering: the publisher drains its
// stores (s_waitcnt vmcnt(0)) before it raises its flag; consumers read data only after they have seen the flag.
__device__ __forceinline__ void xstore(double* p, double v) {
  __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void xstore(float* p, float v) {
  __hip_atomic_store(reinterpret_cast<unsigned*>(p), __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void xstore(unsigned* p, unsigned v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double xload(const double* p) {
  return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ float xload(const float* p) {
  return __uint_as_float(__hip_atomic_load(reinterpret_cast<const unsigned*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ unsigned xload(const unsigned* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void gstore(unsigned long long* p, unsigned tag, unsigned payload) {
  __hip_atomic_store(p, ((unsigned long long)tag << 32) | (unsigned long long)payload, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long gload(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// device-wide barrier over the N (<= 128) workgroups: workgroup n raises its own flag word to `value` (no read-modify-write
// contention on one address), wave 0 polls all N flags with one or two loads per lane.  Flags only grow: no reset.
__device__ __forceinline__ void grid_barrier(unsigned* flags, int N, int n, unsigned value, int& spin_limit) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this thread's exchange stores have been performed
  __syncthreads();                                      // ... and everybody else's in the workgroup
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    if (lane == 0) xstore(flags + n, value);
    int spins = 0;
    bool ok = false;
    while (spins < spin_limit && !ok) {
      const unsigned v0 = lane < N ? xload(flags + lane) : value;
      const unsigned v1 = lane + 64 < N ? xload(flags + lane + 64) : value;
      ok = __all(v0 >= value && v1 >= value);
      ++spins;
    }
    if (!ok) spin_limit = 1;      // caller reports through icrl_agent_t.status
  }
  __syncthreads();
}

// GRAN: every exchanged float64 travels in its own 16-byte record with the step number at both ends (the datum is the flag:
// cdna_hip_programming.md Guideline 16; a torn access shows an old tag in one half).  Consumers poll the records themselves, so a
// step costs ONE trip through the memory system after the slowest producer instead of three (drain stores -> raise flag -> see
// flag -> fetch data).  (Until the end of round 3: one 8-byte {tag, 32 bits} granule per half-word — twice the memory
// instructions, and the all-to-all read of 64 workgroups ran into the chip's rate of uncached loads.)
// PROF: the diagnostic phase timers (do_gae bit 2) as a compile-time variant: as a run-time flag their seven 64-bit accumulators sat in scalar registers
// across the step loop of every launch (ppo_train_halves.hip: 2.5 % there)
// MON: store the raw reward of every step into ActStepArgs.raw_plane (icrl_monitor_t.raw_rewards) — a compile-time variant like PROF: the
// instantiations without it are the kernels as they were, with not one more value in the step loop's registers
// SDE: the gSDE head (sde_head_wave) behind a deterministic forward, a compile-time form like MON and DISC: the instantiations without it keep
// their code.  The launch's dynamic LDS then carries, behind the dynamics matrix, the float64 image of exp(2 log_std) [MAX_H][A] — log_std does
// not change during a rollout: one exp per entry and launch, the per-call kernel's own bits — and the env's current exploration matrix
// [MAX_H][A] float32, refilled from registers only where the draw index changes; the next draw's matrix is fetched one step ahead, as the
// noise row is.
template <int OCT, int CIT, bool GRAN, bool PROF = false, bool MON = false, bool POINT = true, bool DISC = false, bool SDE = false, bool REGION = false>
__device__ __forceinline__ void rollout_persistent_body(const PersistArgs& p, const SdeArgs& sd = SdeArgs()) {
  extern __shared__ __attribute__((aligned(16))) double dyn_lds[];
  __shared__ ActShared sh;
  double* const chunk = dyn_lds;                          // raw observations of the step, TRANSPOSED: [obs][NP], NP = N + 64
  double* const Bl = dyn_lds + p.act.pl.O * (p.act.env.n_envs + 64);
  __shared__ double vec[2][128], dev2[2][128], ret_s[128], cret_s[128], rawr_s[128];
  __shared__ float rawc_s[128];
  __shared__ double dens[2];
  __shared__ float noise_s[MAX_ACT], alow_s[MAX_ACT], ahigh_s[MAX_ACT];     // action box: read every step, kept out of global memory
  __shared__ int done_s[128];
  __shared__ int last_done_s;
  const ActStepArgs& a = p.act;
  REGION_TABLE(a, (int)threadIdx.x, 256)      // (published by the step loop's first barrier)
  // private copies of the structs whose pointers the step loop goes through, every pointer marked as a global-memory pointer
  // (common.h: as_global — in a batched launch the block comes from LDS / memory and the accesses would be flat_* otherwise)
  icrl_norm_t nm = p.nm; globalize(nm);
  icrl_buffer_t buf = a.buf; globalize(buf);
  icrl_agent_t ag = a.ag; globalize(ag);
  icrl_costnet_t cnet = a.cn; globalize(cnet);
  unsigned long long* const xg_all = as_global(p.xg);
  const float* const noise_g = as_global(a.noise);
  double* const raw_plane = MON ? as_global(a.raw_plane) : nullptr;
  WaveRegs<OCT, CIT> R;                // one image: policy weights in waves 0..2, cost-net weights in wave 3
  WaveRegs<OCT, CIT>& C = R;
  load_pol_regs<OCT>(a.pl, a.PT, R);
  if constexpr (CIT > 0) { if (threadIdx.x >= 192 && a.has_cn) load_cn_regs<CIT>(a.cn, a.cl, C); }
  const icrl_cost_fn_t cf = a.cf;      // analytic cost (CIT == 0): kind, index and thresholds are read once, before the step loop
  const int n = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int O = a.pl.O, A = a.pl.A, N = a.env.n_envs, T = p.T;
  const int AS = buf.act_store;
  const int NA = a.pl.discrete ? 1 : A;       // noise values per env step
  const int NP = N + 64;                      // padded column length of the transposed observation block
  const int G = 2 * O + 4;                    // 8-byte words per env and step of the exchange area
  // Exchange records (GRAN): 16 bytes {tag, lo, hi, tag} — a float64 with this step's tag at both ends (a torn 16-byte access shows an
  // old tag in one half).  Per env: obs_dim observation records, one reward record (the done flag in the top bit of its second tag), one
  // cost record = R16 = obs_dim + 2 records = the same G x 8 bytes as one 8-byte {tag, word} granule per 32-bit word, but HALF the
  // memory instructions: 64 workgroups x 2560 granule loads per step ran into the chip's rate of uncached loads (~62 G/s).
  const int R16 = O + 2;
  typedef unsigned int rec_u4 __attribute__((ext_vector_type(4)));
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(xg_all, 0, 2 * N * G * 8, 0x00020000);
  auto rstore = [&](int byte_off, rec_u4 v) { __builtin_amdgcn_raw_buffer_store_b128(v, xrs, byte_off, 0, 16); };     // sc1
  auto rload = [&](int byte_off) -> rec_u4 { return __builtin_amdgcn_raw_buffer_load_b128(xrs, byte_off, 0, 16); };
  for (int i = tid; i < O * NP; i += 256) chunk[i] = 0.0;
  // gSDE (persist_sde_dyn_lds): the two images behind the dynamics matrix, and the matrix entries this thread carries from global memory to LDS
  constexpr int SDE_REGS = MAX_H * MAX_ACT / 256;
  double* const e2_s = SDE ? Bl + O * a.env.act_dim : nullptr;                        // exp(2 log_std) [MAX_H][A]
  float* const E_s = SDE ? reinterpret_cast<float*>(e2_s + MAX_H * A) : nullptr;      // this env's current matrix [MAX_H][A]
  const float* const expl_n = SDE ? as_global(sd.expl) + (size_t)n * (size_t)sd.env_stride : nullptr;
  float e_reg[SDE_REGS];
  if constexpr (SDE) {
    const float* const ls_g = as_global(sd.ls);
    for (int i = tid; i < MAX_H * A; i += 256) e2_s[i] = exp(2. * (double)ls_g[i]);
#pragma unroll
    for (int k = 0; k < SDE_REGS; ++k) { const int i = k * 256 + tid; e_reg[k] = i < MAX_H * A ? expl_n[i] : 0.f; }      // draw 0
  }
  const bool has_cost = a.has_cn != 0;
  const uint32_t e_key = a.env.key[n];
  uint32_t e_ctr = a.env.step_count[n];
  int e_tep = a.env.t_ep[n];
  icrl_env_t env = a.env; globalize(env);
  for (int i = tid; i < O * a.env.act_dim; i += 256) Bl[i] = a.env.B[i];
  env.B = Bl;
  const bool has_box = a.alow != nullptr && a.ahigh != nullptr;
  if (tid < MAX_ACT) { alow_s[tid] = (has_box && tid < A) ? a.alow[tid] : 0.f; ahigh_s[tid] = (has_box && tid < A) ? a.ahigh[tid] : 0.f; }
  for (int i = tid; i < MAX_OBS; i += 256) {
    sh.x[i] = i < O ? (float)ag.last_obs[(size_t)n * O + i] : 0.f;
    if (i < O) sh.s_old[i] = a.env.s[(size_t)n * O + i];
  }
  if (tid < N) { ret_s[tid] = nm.ret[tid]; cret_s[tid] = nm.cost_ret[tid]; }
  if (tid == 0) last_done_s = ag.last_dones[n];
  // replicated running statistics: observation columns in threads < O, ret_rms in wave 3, cost_rms in wave 2
  double o_mean = 0.0, o_var = 1.0, o_cnt = 0.0, o_last = 0.0;
  if (tid < O) { o_mean = nm.obs_mean[tid]; o_var = nm.obs_var[tid]; o_cnt = nm.obs_count[0]; o_last = ag.last_obs[(size_t)n * O + tid]; }
  double st_m = 0.0, st_v = 1.0, st_c = 0.0;
  if (w == 3) { st_m = nm.ret_stats[0]; st_v = nm.ret_stats[1]; st_c = nm.ret_stats[2]; }
  if (w == 2) { st_m = nm.cost_stats[0]; st_v = nm.cost_stats[1]; st_c = nm.cost_stats[2]; }
  float noise_reg = (!SDE && tid < NA) ? noise_g[(size_t)n * NA + tid] : 0.f;
  double fin_rew = 0.0; float fin_cost = 0.f; int fin_done = 0;
  unsigned long long pc0 = 0, pc1 = 0, pc2 = 0, pc3 = 0, pc4 = 0, pc5 = 0, pc_rounds = 0, tl = PROF ? prof_now() : 0ull;
  // PROF: the step chain of workgroup 0 in finer pieces, on thread 0 (wave 0 carries the chain): cycles from one mark to the next, summed over
  // the steps — CH_FWD .. CH_REST below; fc[CH_PUB_AT]: the sum of the cycles from the step's start to the publish.  Written to g_wide_trace
  // behind the per-workgroup words (CHAIN_TRACE_BASE), read by tools/rollout_only.py.
  enum { CH_FWD, CH_HANDOFF, CH_ENV, CH_PUBLISH, CH_AFTER_PUB, CH_POLL, CH_SCATTER, CH_VEC, CH_COLUMNS, CH_MERGE, CH_NORMALISE, CH_REST, CH_PUB_AT, CH_N };
  unsigned long long fc[CH_N] = {0}, fl = 0, f0 = 0;
  auto mark = [&](int k) { if (PROF) { const unsigned long long now = prof_now(); fc[k] += now - fl; fl = now; } };
  constexpr int TAIL = 192;      // the thread of the step's tail (and of fin_rew / fin_cost / fin_done)
  int spin_limit = 1 << 22;
  if constexpr (!SDE) __syncthreads();      // the set-up above, once: inside the loop no wave reads what another wrote before the hand-off barrier
  for (int t = 0; t < T; ++t) {
    const int par = t & 1;
    const size_t tn = (size_t)t * N + n;
    const unsigned gtag = (unsigned)(t + 1);
    if (PROF) { fl = prof_now(); f0 = fl; }
    if (!SDE && tid < NA) {
      noise_s[tid] = noise_reg;
      if (t + 1 < T) noise_reg = noise_g[((size_t)(t + 1) * N + n) * NA + tid];     // lands during this step
    }
    if constexpr (SDE) {
      const int sf = sd.sample_freq;
      if (t == 0 || (sf > 0 && t % sf == 0)) {      // a new draw: its matrix waits in the registers
#pragma unroll
        for (int k = 0; k < SDE_REGS; ++k) { const int i = k * 256 + tid; if (i < MAX_H * A) E_s[i] = e_reg[k]; }
      }
      if (t + 1 < T && sf > 0 && (t + 1) % sf == 0) {      // the next step starts a draw: its matrix lands during this step
        const float* const nxt = expl_n + (size_t)((t + 1) / sf) * (size_t)sd.draw_stride;
#pragma unroll
        for (int k = 0; k < SDE_REGS; ++k) { const int i = k * 256 + tid; e_reg[k] = i < MAX_H * A ? nxt[i] : 0.f; }
      }
    }
    if constexpr (SDE) __syncthreads();      // the exploration matrix is filled by all four waves
    else wave_lds_order();                   // noise_s: written and read by wave 0
    // ---------------- phase A: kernel A's work for env n ----------------
    float head = 0.f;      // policy_forward_chain: wave 0's log-prob operand, the value of waves 1 / 2
    if constexpr (SDE) {
      // the mean and the latent, then the head on wave 0, which rewrites its own act_raw / act_clip / scal[2] (LDS accesses of one wave are
      // ordered: no barrier in between); the barrier below publishes them to the env step, the cost wave and the buffer stores
      policy_forward_block<OCT>(a.pl, R, sh, nullptr, 1, nullptr, nullptr);
      if (w == 0) sde_head_wave(sh, A, a.pl.H2, E_s, [&](int i) { return e2_s[i]; }, has_box ? alow_s : nullptr, has_box ? ahigh_s : nullptr);
    } else {
      head = policy_forward_chain<OCT>(a.pl, R, sh, noise_s, has_box ? alow_s : nullptr, has_box ? ahigh_s : nullptr);
    }
    mark(CH_FWD);
    __syncthreads();      // the hand-off: act_clip / act_raw (and s_old, x of the last step) to the env step, the cost wave and the storing waves
    mark(CH_HANDOFF);
    if (SDE && w < 3) head = sh.scal[w == 0 ? 2 : w - 1];      // (the block form's words: log-prob, v_r, v_c)
    if (w == 0) {
      double rew; int done;
      env_step_wave<POINT>(env, n, sh.s_old, sh.act_clip, e_key, e_ctr, e_tep, sh.s_new, rew, done);
      mark(CH_ENV);
      float* nob = buf.new_orig_observations + tn * O;
      if (GRAN) {
        const int rec0 = ((par * N + n) * R16) * 16;       // byte offset of this env's records of this parity
        for (int i = lane; i < O; i += WAVE) {
          const double v = sh.s_new[i];
          nob[i] = (float)v;
          const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
          rstore(rec0 + 16 * i, rec_u4{gtag, (unsigned)bits, (unsigned)(bits >> 32), gtag});
        }
        if (lane == 0) {       // reward record: the done flag rides in the top bit of its second tag
          const unsigned long long bits = (unsigned long long)__double_as_longlong(rew);
          rstore(rec0 + 16 * O, rec_u4{gtag, (unsigned)bits, (unsigned)(bits >> 32), gtag | (done ? 0x80000000u : 0u)});
        }
      } else {
        double* xo = as_global(p.xch_obs) + ((size_t)par * N + n) * O;
        for (int i = lane; i < O; i += WAVE) { const double v = sh.s_new[i]; nob[i] = (float)v; xstore(xo + i, v); }
        if (lane == 0) { xstore(as_global(p.xch_rew) + par * N + n, rew); xstore(as_global(p.xch_done) + par * N + n, (unsigned)done); }
      }
      if (PROF) { mark(CH_PUBLISH); fc[CH_PUB_AT] += fl - f0; }
      // the log-prob, which nothing in this step waits for: evaluated while the records are in flight
      const float lp = SDE ? head : chain_log_prob(a.pl, R, head);
      if (lane == 0) buf.log_probs[tn] = lp;
      mark(CH_AFTER_PUB);
    } else if (w == 3) {
      float cost = 0.f;
      if constexpr (REGION) cost = cost_region_wave(rtab, a.cr.n_clauses, a.cr.combine, sh.s_old, sh.act_clip, O);
      else if constexpr (CIT == 0) cost = cost_fn_wave(cf, sh.s_old, sh.act_clip);
      else if (a.has_cn) cost = cost_forward_wave<CIT>(cnet, a.cl, C, sh.s_old, sh.act_clip, sh.cx, sh.ch, DISC ? 1 : 0);
      if (lane == 0) {
        if (GRAN) rstore(((par * N + n) * R16 + O + 1) * 16, rec_u4{gtag, __float_as_uint(cost), 0u, gtag});
        else xstore(as_global(p.xch_cost) + par * N + n, cost);
        buf.orig_costs[tn] = cost;
      }
    } else if (w == 2) {
      float* ob = buf.observations + tn * O;
      float* oob = buf.orig_observations + tn * O;
      for (int i = lane; i < O; i += WAVE) { ob[i] = sh.x[i]; oob[i] = (float)sh.s_old[i]; }
      if (lane < AS) buf.actions[tn * AS + lane] = sh.act_raw[lane];
      if (lane < A && !a.pl.discrete) ag.act_clipped[(size_t)n * A + lane] = sh.act_clip[lane];
      if (lane == 0) {       // (each wave stores what it computed: the log-prob above, v_r below)
        buf.dones[tn] = (float)last_done_s;
        buf.cost_values[tn] = head;
        ag.last_v_c[n] = head;
      }
    } else {
      if (lane == 0) { buf.reward_values[tn] = head; ag.last_v_r[n] = head; }
    }
    if (PROF) { const unsigned long long tn_ = prof_now(); pc0 += tn_ - tl; tl = tn_; }
    if (PROF && t == T / 2 && lane == 0) g_wide_trace[4 * n + w] = __builtin_amdgcn_s_memrealtime();   // per wave: end of its phase-A part
    if (GRAN) {
      // poll this thread's records of ALL envs until every one carries this step's tag at both ends, then scatter the payloads
      const int rbase = par * N * R16 * 16;
      const int total = N * R16;
      rec_u4 g[REC_MAX];
#pragma unroll
      for (int k = 0; k < REC_MAX; ++k) g[k] = (k * 256 + tid < total) ? rload(rbase + (k * 256 + tid) * 16) : rec_u4{gtag, 0u, 0u, gtag};
      bool ok = false;
      int rounds = 0;
      for (int spins = 0; spins < spin_limit && !ok; ++spins) {
        ok = true;
#pragma unroll
        for (int k = 0; k < REC_MAX; ++k)
          if (g[k][0] != gtag || (g[k][3] & 0x7fffffffu) != gtag) { g[k] = rload(rbase + (k * 256 + tid) * 16); ok = false; }
        ++rounds;
      }
      if (PROF && tid == 0) { pc_rounds += (unsigned long long)rounds; }
      mark(CH_POLL);
      if (!ok) spin_limit = 1;      // a peer never showed up (a workgroup was not resident): stop waiting ~2 s per step; reported below
#pragma unroll
      for (int k = 0; k < REC_MAX; ++k) {
        const int idx = k * 256 + tid;
        if (idx < total) {
          unsigned rr = __umulhi((unsigned)idx, p.g_magic);
          int slot = idx - (int)rr * R16;
          if (slot >= R16) { slot -= R16; ++rr; }
          const double v = __longlong_as_double((long long)(((unsigned long long)g[k][2] << 32) | (unsigned long long)g[k][1]));
          if (slot < O) chunk[slot * NP + (int)rr] = v;
          else if (slot == O) { rawr_s[rr] = v; done_s[rr] = (int)(g[k][3] >> 31); }
          else rawc_s[rr] = has_cost ? __uint_as_float(g[k][1]) : 0.f;
        }
      }
      __syncthreads();
    } else {
      grid_barrier(as_global(p.counter), N, n, (unsigned)(t + 1), spin_limit);
    }
    if (PROF) { const unsigned long long tn_ = prof_now(); pc1 += tn_ - tl; tl = tn_; }
    mark(CH_SCATTER);
    // ---------------- phase B: kernel B's statistics, replicated; normalise own env ----------------
    if constexpr (GRAN) {
      // this step's running returns, on the wave that sums them below (ret: wave 3, cost_ret: wave 2) and that alone reads and writes
      // ret_s / cret_s / vec inside the loop: a wave-local ordering, no workgroup barrier between the scatter and the column chains
      if (w == 3) {
        for (int i = lane; i < N; i += 64) {
          const double rr = rawr_s[i];
          double r = ret_s[i];
          if (nm.training) r = r * nm.reward_gamma + rr;
          vec[0][i] = r;
        }
      } else if (w == 2) {
        for (int i = lane; i < N; i += 64) {
          const float rc = rawc_s[i];
          double c = has_cost ? cret_s[i] : 0.0;
          if (nm.training && has_cost) c = c * nm.cost_gamma + (double)rc;
          vec[1][i] = c;
        }
      }
      if (w >= 2) wave_lds_order();
    } else
    {
      if (!GRAN) {
        const double* xo = as_global(p.xch_obs) + (size_t)par * N * O;
        for (int i = tid; i < N * O; i += 256) { const int rr = i / O, j = i - rr * O; chunk[j * NP + rr] = xload(xo + i); }
      }
      if (tid < N) {
        if (!GRAN) {
          rawr_s[tid] = xload(as_global(p.xch_rew) + par * N + tid);
          rawc_s[tid] = has_cost ? xload(as_global(p.xch_cost) + par * N + tid) : 0.f;
          done_s[tid] = (int)xload(as_global(p.xch_done) + par * N + tid);
        }
        const double rr = rawr_s[tid];
        const float rc = rawc_s[tid];
        double r = ret_s[tid], c = has_cost ? cret_s[tid] : 0.0;
        if (nm.training) {
          r = r * nm.reward_gamma + rr;
          if (has_cost) c = c * nm.cost_gamma + (double)rc;
        }
        vec[0][tid] = r; vec[1][tid] = c;
      }
      __syncthreads();
    }
    if (PROF) { const unsigned long long tn_ = prof_now(); pc3 += tn_ - tl; tl = tn_; }
    mark(CH_VEC);
    if (nm.training) {
      if (tid < O) {           // obs_rms.update: rows added in order (numpy's axis-0 reduction)
        double bm, bv;
        column_moments_contig(chunk + tid * NP, N, bm, bv);
        mark(CH_COLUMNS);
        chan_merge(o_mean, o_var, o_cnt, bm, bv, (double)N);
        o_cnt = (double)N + o_cnt;
        mark(CH_MERGE);
      }
      if (w == 3 || (w == 2 && has_cost)) {     // ret_rms / cost_rms: numpy pairwise order
        const int v = w == 3 ? 0 : 1;
        const double bm = np_leaf_sum_wave(vec[v], N) / (double)N;
        for (int i = lane; i < N; i += 64) { const double d = vec[v][i] - bm; dev2[v][i] = d * d; }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_waitcnt(0xC07F);
        const double bv = np_leaf_sum_wave(dev2[v], N) / (double)N;
        chan_merge(st_m, st_v, st_c, bm, bv, (double)N);
        st_c = (double)N + st_c;
      }
    }
    if (lane == 0 && w == 3) dens[0] = sqrt(st_v + nm.epsilon);
    if (lane == 0 && w == 2) dens[1] = sqrt(st_v + nm.epsilon);
    if (PROF) { const unsigned long long tn_ = prof_now(); pc4 += tn_ - tl; tl = tn_; }
    if (tid < O) {             // own env: normalise + clip, next policy input
      double o = chunk[tid * NP + n];
      if (nm.norm_obs) o = fmin(fmax((o - o_mean) / sqrt(o_var + nm.epsilon), -nm.clip_obs), nm.clip_obs);
      o_last = o;
      sh.x[tid] = (float)o;
      buf.new_observations[tn * O + tid] = (float)o;
      sh.s_old[tid] = sh.s_new[tid];
    }
    __syncthreads();
    if (PROF) { const unsigned long long tn_ = prof_now(); pc5 += tn_ - tl; tl = tn_; }
    mark(CH_NORMALISE);
    if (GRAN) {
      if (w == 3) {
        for (int i = lane; i < N; i += 64) { const int d = done_s[i]; if (nm.training || d) ret_s[i] = d ? 0.0 : vec[0][i]; }
      } else if (w == 2 && has_cost) {
        for (int i = lane; i < N; i += 64) { const int d = done_s[i]; if (nm.training || d) cret_s[i] = d ? 0.0 : vec[1][i]; }
      }
    } else
    if (tid < N) {
      const int d = done_s[tid];
      if (nm.training || d) { ret_s[tid] = d ? 0.0 : vec[0][tid]; if (has_cost) cret_s[tid] = d ? 0.0 : vec[1][tid]; }
    }
    // the step's tail — the own env's reward and cost normalised and stored, two float64 divisions — on lane 0 of the cost wave, which has
    // nothing else to do before the next hand-off barrier (wave 0 goes straight on to the next policy forward)
    if (tid == TAIL) {
      double r = rawr_s[n];
      fin_rew = r; fin_cost = rawc_s[n]; fin_done = done_s[n];
      if (nm.norm_reward) r = fmin(fmax(r / dens[0], -nm.clip_reward), nm.clip_reward);
      buf.rewards[tn] = (float)r;
      if (has_cost) {
        double c = (double)rawc_s[n];
        if (nm.norm_cost) c = fmin(fmax(c / dens[1], -nm.clip_cost), nm.clip_cost);
        buf.costs[tn] = (float)c;
      }
      last_done_s = done_s[n];
      if (MON) raw_plane[tn] = fin_rew;
    }
    if (PROF) { const unsigned long long tn_ = prof_now(); pc2 += tn_ - tl; tl = tn_; }
    mark(CH_REST);
  }
  if (PROF && n == 0 && tid == 0) { g_rollout_prof[0] = pc0; g_rollout_prof[1] = pc1; g_rollout_prof[2] = pc2; g_rollout_prof[3] = (unsigned long long)T; g_rollout_prof[4] = pc3; g_rollout_prof[5] = pc4; g_rollout_prof[6] = pc5; g_rollout_prof[7] = pc_rounds; }
  if (PROF && n == 0 && tid == 0) {
#pragma unroll
    for (int k = 0; k < CH_N; ++k) g_wide_trace[CHAIN_TRACE_BASE + k] = fc[k];
  }
  // a timed-out exchange means stale granules went into the statistics and the buffer: tell the host (it raises)
  if (spin_limit == 1 && ag.status != nullptr && (tid & 63) == 0) atomicOr(ag.status, 1);
  // ---- leave the agent / wrapper state exactly where the per-step path leaves it
  __syncthreads();
  if (tid < O) ag.last_obs[(size_t)n * O + tid] = o_last;
  if (tid == TAIL) {
    ag.last_dones[n] = (uint8_t)last_done_s;
    ag.raw_rew[n] = fin_rew; ag.dones[n] = (uint8_t)fin_done;
    if (has_cost) ag.raw_cost[n] = fin_cost;
  }
  if (n == 0) {
    if (tid < O) { nm.obs_mean[tid] = o_mean; nm.obs_var[tid] = o_var; }
    if (tid == 0) nm.obs_count[0] = o_cnt;
    if (lane == 0 && w == 3) { nm.ret_stats[0] = st_m; nm.ret_stats[1] = st_v; nm.ret_stats[2] = st_c; }
    if (lane == 0 && w == 2 && has_cost) { nm.cost_stats[0] = st_m; nm.cost_stats[1] = st_v; nm.cost_stats[2] = st_c; }
    if (tid < N) { nm.ret[tid] = ret_s[tid]; if (has_cost) nm.cost_ret[tid] = cret_s[tid]; }
  }
}

// The persistent rollout for a generic-shape policy (hidden layers above 64 units or an `arch` descriptor; the constraint net one the
// register image holds): the same loop, phase A's policy forward = the table-driven forward of generic.hip (gen_mlp_forward +
// gen_policy_head: bit-identical to policy_generic_kernel, i.e. to the per-step launches) in its four-units-per-lane form (generic.h:
// gen_mlp_forward_quads — waves 0..2 = the three slots of the table).
template <int OCT, int CIT, bool MON, bool DISC = false>
__device__ __forceinline__ void rollout_generic_body(const GenRolloutArgs& ga) {
  constexpr bool GRAN = true;
  const PersistArgs& p = ga.p;
  const GenNet& net = ga.net;
  __shared__ float gact[GEN_MAX_ROW];
  extern __shared__ __attribute__((aligned(16))) double dyn_lds[];
  __shared__ ActShared sh;
  double* const chunk = dyn_lds;                          // raw observations of the step, TRANSPOSED: [obs][NP], NP = N + 64
  double* const Bl = dyn_lds + p.act.pl.O * (p.act.env.n_envs + 64);
  __shared__ double vec[2][128], dev2[2][128], ret_s[128], cret_s[128], rawr_s[128];
  __shared__ float rawc_s[128];
  __shared__ double dens[2];
  __shared__ float noise_s[MAX_ACT], alow_s[MAX_ACT], ahigh_s[MAX_ACT];     // action box: read every step, kept out of global memory
  __shared__ int done_s[128];
  __shared__ int last_done_s;
  const ActStepArgs& a = p.act;
  // private copies of the structs whose pointers the step loop goes through, every pointer marked as a global-memory pointer
  // (common.h: as_global — in a batched launch the block comes from LDS / memory and the accesses would be flat_* otherwise)
  icrl_norm_t nm = p.nm; globalize(nm);
  icrl_buffer_t buf = a.buf; globalize(buf);
  icrl_agent_t ag = a.ag; globalize(ag);
  icrl_costnet_t cnet = a.cn; globalize(cnet);
  unsigned long long* const xg_all = as_global(p.xg);
  const float* const noise_g = as_global(a.noise);
  double* const raw_plane = MON ? as_global(a.raw_plane) : nullptr;
  WaveRegs<OCT, CIT> R;                // one image: policy weights in waves 0..2, cost-net weights in wave 3
  WaveRegs<OCT, CIT>& C = R;
  if constexpr (CIT > 0) { if ((threadIdx.x >> 6) == 3 && a.has_cn) load_cn_regs<CIT>(a.cn, a.cl, C); }
  const icrl_cost_fn_t cf = a.cf;      // analytic cost (CIT == 0): kind, index and thresholds are read once, before the step loop
  const int n = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63;
  const int ctid = tid < 256 ? tid : (1 << 28);      // (the threads beyond the first 256 only take part in the forward)
  const float* const Pn = as_global(ga.P);
  const float* const PTn = as_global(a.PT);
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int O = a.pl.O, A = a.pl.A, N = a.env.n_envs, T = p.T;
  const int AS = buf.act_store;
  const int NA = a.pl.discrete ? 1 : A;       // noise values per env step
  const int NP = N + 64;                      // padded column length of the transposed observation block
  const int G = 2 * O + 4;                    // 8-byte words per env and step of the exchange area
  // Exchange records (GRAN): 16 bytes {tag, lo, hi, tag} — a float64 with this step's tag at both ends (a torn 16-byte access shows an
  // old tag in one half).  Per env: obs_dim observation records, one reward record (the done flag in the top bit of its second tag), one
  // cost record = R16 = obs_dim + 2 records = the same G x 8 bytes as one 8-byte {tag, word} granule per 32-bit word, but HALF the
  // memory instructions: 64 workgroups x 2560 granule loads per step ran into the chip's rate of uncached loads (~62 G/s).
  const int R16 = O + 2;
  typedef unsigned int rec_u4 __attribute__((ext_vector_type(4)));
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(xg_all, 0, 2 * N * G * 8, 0x00020000);
  auto rstore = [&](int byte_off, rec_u4 v) { __builtin_amdgcn_raw_buffer_store_b128(v, xrs, byte_off, 0, 16); };     // sc1
  auto rload = [&](int byte_off) -> rec_u4 { return __builtin_amdgcn_raw_buffer_load_b128(xrs, byte_off, 0, 16); };
  for (int i = ctid; i < O * NP; i += 256) chunk[i] = 0.0;
  const bool has_cost = a.has_cn != 0;
  const uint32_t e_key = a.env.key[n];
  uint32_t e_ctr = a.env.step_count[n];
  int e_tep = a.env.t_ep[n];
  icrl_env_t env = a.env; globalize(env);
  for (int i = ctid; i < O * a.env.act_dim; i += 256) Bl[i] = a.env.B[i];
  env.B = Bl;
  const bool has_box = a.alow != nullptr && a.ahigh != nullptr;
  if (tid < MAX_ACT) { alow_s[tid] = (has_box && tid < A) ? a.alow[tid] : 0.f; ahigh_s[tid] = (has_box && tid < A) ? a.ahigh[tid] : 0.f; }
  for (int i = ctid; i < MAX_OBS; i += 256) {
    sh.x[i] = i < O ? (float)ag.last_obs[(size_t)n * O + i] : 0.f;
    if (i < O) sh.s_old[i] = a.env.s[(size_t)n * O + i];
  }
  if (tid < N) { ret_s[tid] = nm.ret[tid]; cret_s[tid] = nm.cost_ret[tid]; }
  if (tid == 0) last_done_s = ag.last_dones[n];
  // replicated running statistics: observation columns in threads < O, ret_rms in wave 3, cost_rms in wave 2
  double o_mean = 0.0, o_var = 1.0, o_cnt = 0.0, o_last = 0.0;
  if (tid < O) { o_mean = nm.obs_mean[tid]; o_var = nm.obs_var[tid]; o_cnt = nm.obs_count[0]; o_last = ag.last_obs[(size_t)n * O + tid]; }
  double st_m = 0.0, st_v = 1.0, st_c = 0.0;
  if (w == 3) { st_m = nm.ret_stats[0]; st_v = nm.ret_stats[1]; st_c = nm.ret_stats[2]; }
  if (w == 2) { st_m = nm.cost_stats[0]; st_v = nm.cost_stats[1]; st_c = nm.cost_stats[2]; }
  float noise_reg = (tid < NA) ? noise_g[(size_t)n * NA + tid] : 0.f;
  double fin_rew = 0.0; float fin_cost = 0.f; int fin_done = 0;
  unsigned long long pc0 = 0, pc1 = 0, pc2 = 0, pc3 = 0, pc4 = 0, pc5 = 0, pc_rounds = 0, tl = p.prof ? prof_now() : 0ull;
  int spin_limit = 1 << 22;
  for (int t = 0; t < T; ++t) {
    const int par = t & 1;
    const size_t tn = (size_t)t * N + n;
    const unsigned gtag = (unsigned)(t + 1);
    if (tid < NA) {
      noise_s[tid] = noise_reg;
      if (t + 1 < T) noise_reg = noise_g[((size_t)(t + 1) * N + n) * NA + tid];     // lands during this step
    }
    __syncthreads();
    // ---------------- phase A: kernel A's work for env n ----------------
    gen_mlp_forward_quads(net, PTn, sh.x, gact, w, lane);
    if (tid == 0) {
      float lp, ent;
      gen_policy_head(net, Pn, gact + net.layer[net.head[0]].act_off, noise_s, 0, has_box ? alow_s : nullptr, has_box ? ahigh_s : nullptr, nullptr,
                      sh.act_raw, sh.act_clip, lp, ent);
      sh.scal[0] = gact[net.layer[net.head[1]].act_off]; sh.scal[1] = gact[net.layer[net.head[2]].act_off]; sh.scal[2] = lp;
    }
    __syncthreads();
    if (w == 0) {
      double rew; int done;
      env_step_wave(env, n, sh.s_old, sh.act_clip, e_key, e_ctr, e_tep, sh.s_new, rew, done);
      float* nob = buf.new_orig_observations + tn * O;
      if (GRAN) {
        const int rec0 = ((par * N + n) * R16) * 16;       // byte offset of this env's records of this parity
        for (int i = lane; i < O; i += WAVE) {
          const double v = sh.s_new[i];
          nob[i] = (float)v;
          const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
          rstore(rec0 + 16 * i, rec_u4{gtag, (unsigned)bits, (unsigned)(bits >> 32), gtag});
        }
        if (lane == 0) {       // reward record: the done flag rides in the top bit of its second tag
          const unsigned long long bits = (unsigned long long)__double_as_longlong(rew);
          rstore(rec0 + 16 * O, rec_u4{gtag, (unsigned)bits, (unsigned)(bits >> 32), gtag | (done ? 0x80000000u : 0u)});
        }
      } else {
        double* xo = as_global(p.xch_obs) + ((size_t)par * N + n) * O;
        for (int i = lane; i < O; i += WAVE) { const double v = sh.s_new[i]; nob[i] = (float)v; xstore(xo + i, v); }
        if (lane == 0) { xstore(as_global(p.xch_rew) + par * N + n, rew); xstore(as_global(p.xch_done) + par * N + n, (unsigned)done); }
      }
    } else if (w == 3) {
      float cost = 0.f;
      if constexpr (CIT == 0) cost = cost_fn_wave(cf, sh.s_old, sh.act_clip);
      else if (a.has_cn) cost = cost_forward_wave<CIT>(cnet, a.cl, C, sh.s_old, sh.act_clip, sh.cx, sh.ch, DISC ? 1 : 0);
      if (lane == 0) {
        if (GRAN) rstore(((par * N + n) * R16 + O + 1) * 16, rec_u4{gtag, __float_as_uint(cost), 0u, gtag});
        else xstore(as_global(p.xch_cost) + par * N + n, cost);
        buf.orig_costs[tn] = cost;
      }
    } else if (w == 2) {
      float* ob = buf.observations + tn * O;
      float* oob = buf.orig_observations + tn * O;
      for (int i = lane; i < O; i += WAVE) { ob[i] = sh.x[i]; oob[i] = (float)sh.s_old[i]; }
      if (lane < AS) buf.actions[tn * AS + lane] = sh.act_raw[lane];
      if (lane < A && !a.pl.discrete) ag.act_clipped[(size_t)n * A + lane] = sh.act_clip[lane];
      if (lane == 0) {
        buf.dones[tn] = (float)last_done_s;
        buf.reward_values[tn] = sh.scal[0];
        buf.cost_values[tn] = sh.scal[1];
        buf.log_probs[tn] = sh.scal[2];
        ag.last_v_r[n] = sh.scal[0];
        ag.last_v_c[n] = sh.scal[1];
      }
    }
    if (p.prof) { const unsigned long long tn_ = prof_now(); pc0 += tn_ - tl; tl = tn_; }
    if (p.prof && t == T / 2 && lane == 0) g_wide_trace[4 * n + w] = __builtin_amdgcn_s_memrealtime();   // per wave: end of its phase-A part
    if (GRAN) {
      // poll this thread's records of ALL envs until every one carries this step's tag at both ends, then scatter the payloads
      const int rbase = par * N * R16 * 16;
      const int total = N * R16;
      rec_u4 g[REC_MAX];
#pragma unroll
      for (int k = 0; k < REC_MAX; ++k) g[k] = (k * 256 + ctid < total) ? rload(rbase + (k * 256 + ctid) * 16) : rec_u4{gtag, 0u, 0u, gtag};
      bool ok = false;
      int rounds = 0;
      for (int spins = 0; spins < spin_limit && !ok; ++spins) {
        ok = true;
#pragma unroll
        for (int k = 0; k < REC_MAX; ++k)
          if (g[k][0] != gtag || (g[k][3] & 0x7fffffffu) != gtag) { g[k] = rload(rbase + (k * 256 + ctid) * 16); ok = false; }
        ++rounds;
      }
      if (p.prof && tid == 0) { pc_rounds += (unsigned long long)rounds; }
      if (!ok) spin_limit = 1;      // a peer never showed up (a workgroup was not resident): stop waiting ~2 s per step; reported below
#pragma unroll
      for (int k = 0; k < REC_MAX; ++k) {
        const int idx = k * 256 + ctid;
        if (idx < total) {
          unsigned rr = __umulhi((unsigned)idx, p.g_magic);
          int slot = idx - (int)rr * R16;
          if (slot >= R16) { slot -= R16; ++rr; }
          const double v = __longlong_as_double((long long)(((unsigned long long)g[k][2] << 32) | (unsigned long long)g[k][1]));
          if (slot < O) chunk[slot * NP + (int)rr] = v;
          else if (slot == O) { rawr_s[rr] = v; done_s[rr] = (int)(g[k][3] >> 31); }
          else rawc_s[rr] = has_cost ? __uint_as_float(g[k][1]) : 0.f;
        }
      }
      __syncthreads();
    } else {
      grid_barrier(as_global(p.counter), N, n, (unsigned)(t + 1), spin_limit);
    }
    if (p.prof) { const unsigned long long tn_ = prof_now(); pc1 += tn_ - tl; tl = tn_; }
    // ---------------- phase B: kernel B's statistics, replicated; normalise own env ----------------
    {
      if (!GRAN) {
        const double* xo = as_global(p.xch_obs) + (size_t)par * N * O;
        for (int i = tid; i < N * O; i += 256) { const int rr = i / O, j = i - rr * O; chunk[j * NP + rr] = xload(xo + i); }
      }
      if (tid < N) {
        if (!GRAN) {
          rawr_s[tid] = xload(as_global(p.xch_rew) + par * N + tid);
          rawc_s[tid] = has_cost ? xload(as_global(p.xch_cost) + par * N + tid) : 0.f;
          done_s[tid] = (int)xload(as_global(p.xch_done) + par * N + tid);
        }
        const double rr = rawr_s[tid];
        const float rc = rawc_s[tid];
        double r = ret_s[tid], c = has_cost ? cret_s[tid] : 0.0;
        if (nm.training) {
          r = r * nm.reward_gamma + rr;
          if (has_cost) c = c * nm.cost_gamma + (double)rc;
        }
        vec[0][tid] = r; vec[1][tid] = c;
      }
    }
    __syncthreads();
    if (p.prof) { const unsigned long long tn_ = prof_now(); pc3 += tn_ - tl; tl = tn_; }
    if (nm.training) {
      if (tid < O) {           // obs_rms.update: rows added in order (numpy's axis-0 reduction)
        double bm, bv;
        column_moments_contig(chunk + tid * NP, N, bm, bv);
        chan_merge(o_mean, o_var, o_cnt, bm, bv, (double)N);
        o_cnt = (double)N + o_cnt;
      }
      if (w == 3 || (w == 2 && has_cost)) {     // ret_rms / cost_rms: numpy pairwise order
        const int v = w == 3 ? 0 : 1;
        const double bm = np_leaf_sum_wave(vec[v], N) / (double)N;
        for (int i = lane; i < N; i += 64) { const double d = vec[v][i] - bm; dev2[v][i] = d * d; }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_waitcnt(0xC07F);
        const double bv = np_leaf_sum_wave(dev2[v], N) / (double)N;
        chan_merge(st_m, st_v, st_c, bm, bv, (double)N);
        st_c = (double)N + st_c;
      }
    }
    if (lane == 0 && w == 3) dens[0] = sqrt(st_v + nm.epsilon);
    if (lane == 0 && w == 2) dens[1] = sqrt(st_v + nm.epsilon);
    if (p.prof) { const unsigned long long tn_ = prof_now(); pc4 += tn_ - tl; tl = tn_; }
    if (tid < O) {             // own env: normalise + clip, next policy input
      double o = chunk[tid * NP + n];
      if (nm.norm_obs) o = fmin(fmax((o - o_mean) / sqrt(o_var + nm.epsilon), -nm.clip_obs), nm.clip_obs);
      o_last = o;
      sh.x[tid] = (float)o;
      buf.new_observations[tn * O + tid] = (float)o;
      sh.s_old[tid] = sh.s_new[tid];
    }
    __syncthreads();
    if (p.prof) { const unsigned long long tn_ = prof_now(); pc5 += tn_ - tl; tl = tn_; }
    if (tid < N) {
      const int d = done_s[tid];
      if (nm.training || d) { ret_s[tid] = d ? 0.0 : vec[0][tid]; if (has_cost) cret_s[tid] = d ? 0.0 : vec[1][tid]; }
    }
    if (tid == 0) {
      double r = rawr_s[n];
      fin_rew = r; fin_cost = rawc_s[n]; fin_done = done_s[n];
      if (nm.norm_reward) r = fmin(fmax(r / dens[0], -nm.clip_reward), nm.clip_reward);
      buf.rewards[tn] = (float)r;
      if (has_cost) {
        double c = (double)rawc_s[n];
        if (nm.norm_cost) c = fmin(fmax(c / dens[1], -nm.clip_cost), nm.clip_cost);
        buf.costs[tn] = (float)c;
      }
      last_done_s = done_s[n];
      if (MON) raw_plane[tn] = fin_rew;
    }
    if (p.prof) { const unsigned long long tn_ = prof_now(); pc2 += tn_ - tl; tl = tn_; }
  }
  if (p.prof && n == 0 && tid == 0) { g_rollout_prof[0] = pc0; g_rollout_prof[1] = pc1; g_rollout_prof[2] = pc2; g_rollout_prof[3] = (unsigned long long)T; g_rollout_prof[4] = pc3; g_rollout_prof[5] = pc4; g_rollout_prof[6] = pc5; g_rollout_prof[7] = pc_rounds; }
  // a timed-out exchange means stale granules went into the statistics and the buffer: tell the host (it raises)
  if (spin_limit == 1 && ag.status != nullptr && (tid & 63) == 0) atomicOr(ag.status, 1);
  // ---- leave the agent / wrapper state exactly where the per-step path leaves it
  __syncthreads();
  if (tid < O) ag.last_obs[(size_t)n * O + tid] = o_last;
  if (tid == 0) {
    ag.last_dones[n] = (uint8_t)last_done_s;
    ag.raw_rew[n] = fin_rew; ag.dones[n] = (uint8_t)fin_done;
    if (has_cost) ag.raw_cost[n] = fin_cost;
  }
  if (n == 0) {
    if (tid < O) { nm.obs_mean[tid] = o_mean; nm.obs_var[tid] = o_var; }
    if (tid == 0) nm.obs_count[0] = o_cnt;
    if (lane == 0 && w == 3) { nm.ret_stats[0] = st_m; nm.ret_stats[1] = st_v; nm.ret_stats[2] = st_c; }
    if (lane == 0 && w == 2 && has_cost) { nm.cost_stats[0] = st_m; nm.cost_stats[1] = st_v; nm.cost_stats[2] = st_c; }
    if (tid < N) { nm.ret[tid] = ret_s[tid]; if (has_cost) nm.cost_ret[tid] = cret_s[tid]; }
  }
}

template <int OCT, int CIT, bool MON = false>
__global__ void __launch_bounds__(256) rollout_generic_kernel(GenRolloutArgs ga) {
  rollout_generic_body<OCT, CIT, MON>(ga);
}

template <int OCT, int CIT, bool GRAN, bool PROF = false, bool MON = false>
__global__ void __launch_bounds__(256) rollout_persistent_kernel(PersistArgs p) {
  rollout_persistent_body<OCT, CIT, GRAN, PROF, MON, false>(p);      // (without the Point step: env_step_wave)
}

// the discriminator-cost forms (DISC, see act_step_kernel) of the two kernels above, single runs, no phase timers
template <int OCT, int CIT, bool MON = false>
__global__ void __launch_bounds__(256) rollout_generic_disc_kernel(GenRolloutArgs ga) {
  rollout_generic_body<OCT, CIT, MON, true>(ga);
}
template <int OCT, int CIT, bool GRAN, bool MON = false>
__global__ void __launch_bounds__(256) rollout_persistent_disc_kernel(PersistArgs p) {
  rollout_persistent_body<OCT, CIT, GRAN, false, MON, false, true>(p);
}
// the gSDE form (SDE, see rollout_persistent_body): single runs, no phase timers, no raw-reward plane, no Point step, cost = 1 - zeta;
// dynamic LDS: persist_sde_dyn_lds
template <int OCT, int CIT, bool GRAN>
__global__ void __launch_bounds__(256) rollout_persistent_sde_kernel(PersistArgs p, SdeArgs sd) {
  rollout_persistent_body<OCT, CIT, GRAN, false, false, false, false, true>(p, sd);
}
// the region-cost form (REGION, see act_step_kernel) on the CIT == 0 image: single runs, no phase timers
template <int OCT, bool GRAN, bool MON = false>
__global__ void __launch_bounds__(256) rollout_persistent_region_kernel(PersistArgs p) {
  rollout_persistent_body<OCT, 0, GRAN, false, MON, false, false, false, true>(p);
}

// several independent runs in ONE launch: grid (N, n_runs), run = blockIdx.y, argument blocks in device memory.  Workgroups are
// dispatched x-fastest, so a run's N workgroups become resident together and the oldest run of the grid is always complete: runs
// whose workgroups do not fit yet simply start when earlier runs have finished (the exchange waits are bounded by seconds).
// MINW: waves per SIMD the register allocation must leave room for (= workgroups per CU: each workgroup has one wave per SIMD)
template <int OCT, int CIT, bool GRAN, int MINW, bool MON = false>
__global__ void __launch_bounds__(256, MINW) rollout_persistent_batch_kernel(const PersistArgs* __restrict__ runs) {
  __shared__ PersistArgs p;
  {
    const unsigned* src = reinterpret_cast<const unsigned*>(runs + blockIdx.y);
    unsigned* dst = reinterpret_cast<unsigned*>(&p);
    for (unsigned i = threadIdx.x; i < sizeof(PersistArgs) / 4; i += 256) dst[i] = src[i];
  }
  __syncthreads();
  rollout_persistent_body<OCT, CIT, GRAN, false, MON>(p);
}

// the batched launch with an analytic cost per run (CIT == 0: no cost-net register image), a kernel of its own name like
// rollout_multi_analytic_kernel below.  Every run's descriptor (ActStepArgs.cf) sits in its own argument block and is read once,
// before the step loop: the runs of a grid may differ in kind, index and thresholds.
template <int OCT, bool GRAN, int MINW, bool MON = false>
__global__ void __launch_bounds__(256, MINW) rollout_persistent_batch_analytic_kernel(const PersistArgs* __restrict__ runs) {
  __shared__ PersistArgs p;
  {
    const unsigned* src = reinterpret_cast<const unsigned*>(runs + blockIdx.y);
    unsigned* dst = reinterpret_cast<unsigned*>(&p);
    for (unsigned i = threadIdx.x; i < sizeof(PersistArgs) / 4; i += 256) dst[i] = src[i];
  }
  __syncthreads();
  rollout_persistent_body<OCT, 0, GRAN, false, MON>(p);
}

// =================================================================================================================
// persistent rollout for MANY environments (128 < N <= 1024, or N x obs > 4096): BASELINE configs[2..4] per-GPU shards
// =================================================================================================================
// Same contract as rollout_persistent_kernel (ALL T steps in one launch, buffers / normaliser / agent state bit-identical to
// the per-step launches), different statistics phase.  Replicating the whole [N, obs] observation block in every workgroup
// costs N x obs granule reads per workgroup and step (59 k at AntWall x 256); here the float64 statistics are PARTITIONED:
//   workgroup j < obs        owns observation column j: gathers that column from all N envs (2 N granules), runs numpy's
//                            axis-0 reduction for it (one sequential chain per column: the order, hence every bit, is kept),
//                            merges into the running moments and publishes (mean_j, var_j) as 4 granules;
//   workgroup obs, obs + 1   own ret_rms / cost_rms: discounted returns of all envs, numpy's pairwise sums, merged moments ->
//                            the two normalisation denominators as granules;
//   every workgroup          then reads the 4 obs + 4 statistics granules and normalises its own envs.
// Two hops per step instead of one, but 2 N + 4 obs granules per workgroup instead of N (2 obs + 4).  A workgroup serves
// E = ceil(N / grid) envs one after the other (grid <= what is co-resident: one workgroup per CU at AntWall widths).

template <int OCT, int CITF, bool PROF = false, bool MON = false>      // PROF: the phase timers (do_gae bits 2 / 3) as a compile-time variant, MON: the raw-reward plane (rollout_persistent_body); CITF: CIT [| CIT_DISC] (act_step_kernel)
__global__ void __launch_bounds__(256) rollout_wide_kernel(WideArgs p) {
  constexpr int CIT = CITF & 0xff;                     // the cost-net image proper
  constexpr bool DISC = (CITF & CIT_DISC) != 0;        // the constraint net read as D = zeta (icrl_cost_disc_t)
  constexpr bool REGION = (CITF & CIT_REGION) != 0;    // a region cost (icrl_cost_region_t) on the CIT == 0 image
  REGION_TABLE(p.act, (int)threadIdx.x, 256)           // (published by the barrier in front of the step loop)
  __shared__ ActShared sh[WIDE_E];
  __shared__ double Bl[MAX_OBS * MAX_ACT];
  __shared__ double colbuf[WIDE_MAX_N + 64], dev2buf[WIDE_MAX_N], retbuf[WIDE_MAX_N];
  __shared__ double mean_s[MAX_OBS], var_s[MAX_OBS], dens_s[2];
  __shared__ double olast[WIDE_E][MAX_OBS], rew_s[WIDE_E];
  __shared__ float noise_s[2][WIDE_E][MAX_ACT], alow_s[MAX_ACT], ahigh_s[MAX_ACT], cost_s[WIDE_E];
  __shared__ unsigned ctr_s[WIDE_E];
  __shared__ int tep_s[WIDE_E], last_done_s[WIDE_E], done_s[WIDE_E], done_all[WIDE_MAX_N];
  const ActStepArgs& a = p.act;
  const icrl_norm_t& nm = p.nm;
  WaveRegs<OCT, CIT> R;                // one image: policy weights in waves 0..2, cost-net weights in wave 3
  WaveRegs<OCT, CIT>& C = R;
  load_pol_regs<OCT>(a.pl, a.PT, R);
  if constexpr (CIT > 0) { if (threadIdx.x >= 192 && a.has_cn) load_cn_regs<CIT>(a.cn, a.cl, C); }
  const icrl_cost_fn_t cf = a.cf;      // analytic cost (CIT == 0): kind, index and thresholds are read once, before the step loop
  const int g = blockIdx.x, G = p.G;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int O = a.pl.O, A = a.pl.A, N = a.env.n_envs, T = p.T;
  const int AS = a.buf.act_store;
  const int NA = a.pl.discrete ? 1 : A;
  const int GX = 2 * O + 4, GS = 4 * O + 4;
  // Exchange records: 16 bytes {tag, lo, hi, tag} instead of two 8-byte {tag, word} granules per float64 (same bytes, half the memory
  // instructions; the done flag rides in the top bit of the reward record's second tag).  Per env R16 = obs + 2 records (obs columns,
  // reward, cost); statistics: (mean, var) per column, then the ret / cost denominators.
  const int R16 = O + 2;
  typedef unsigned int rec_u4 __attribute__((ext_vector_type(4)));
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(p.xg, 0, 2 * N * GX * 8, 0x00020000);
  const __amdgpu_buffer_rsrc_t srs = __builtin_amdgcn_make_buffer_rsrc(p.sg, 0, 2 * GS * 8, 0x00020000);
  auto rstore = [](const __amdgpu_buffer_rsrc_t& rs, int byte_off, rec_u4 v) { __builtin_amdgcn_raw_buffer_store_b128(v, rs, byte_off, 0, 16); };   // sc1
  auto rload = [](const __amdgpu_buffer_rsrc_t& rs, int byte_off) -> rec_u4 { return __builtin_amdgcn_raw_buffer_load_b128(rs, byte_off, 0, 16); };
  const int E = (N - g + G - 1) / G;                 // envs of this workgroup (>= 1: G <= N)
  const bool has_cost = a.has_cn != 0;
  const bool has_box = a.alow != nullptr && a.ahigh != nullptr;
  icrl_env_t env = a.env;
  for (int i = tid; i < O * a.env.act_dim; i += 256) Bl[i] = a.env.B[i];
  env.B = Bl;
  if (tid < MAX_ACT) { alow_s[tid] = (has_box && tid < A) ? a.alow[tid] : 0.f; ahigh_s[tid] = (has_box && tid < A) ? a.ahigh[tid] : 0.f; }
  for (int e = 0; e < E; ++e) {
    const int n = g + e * G;
    for (int i = tid; i < MAX_OBS; i += 256) {
      sh[e].x[i] = i < O ? (float)a.ag.last_obs[(size_t)n * O + i] : 0.f;
      if (i < O) { sh[e].s_old[i] = a.env.s[(size_t)n * O + i]; olast[e][i] = a.ag.last_obs[(size_t)n * O + i]; }
    }
    if (tid == 0) { ctr_s[e] = a.env.step_count[n]; tep_s[e] = a.env.t_ep[n]; last_done_s[e] = a.ag.last_dones[n]; }
  }
  // owner roles of this workgroup (its wave 1 does the owner work)
  const int own_col = g < O ? g : -1;
  const bool own_ret = g == O, own_cost = has_cost && g == O + 1;
  double o_mean = 0.0, o_var = 1.0, o_cnt = 0.0;         // wave 1: running moments of the owned statistic
  if (own_col >= 0) { o_mean = nm.obs_mean[own_col]; o_var = nm.obs_var[own_col]; o_cnt = nm.obs_count[0]; }
  if (own_ret) { o_mean = nm.ret_stats[0]; o_var = nm.ret_stats[1]; o_cnt = nm.ret_stats[2]; }
  if (own_cost) { o_mean = nm.cost_stats[0]; o_var = nm.cost_stats[1]; o_cnt = nm.cost_stats[2]; }
  if (own_ret || own_cost)
    for (int i = tid; i < N; i += 256) retbuf[i] = own_ret ? nm.ret[i] : nm.cost_ret[i];
  // noise of step 0
  if (tid < WIDE_E * MAX_ACT) {
    const int e = tid / MAX_ACT, k = tid % MAX_ACT;
    if (e < E && k < NA) noise_s[0][e][k] = a.noise[((size_t)(g + e * G)) * NA + k];
  }
  int spin_limit = 1 << 22;
  __syncthreads();
  const bool prof = PROF && p.prof != 0 && g == p.prof - 1;
  unsigned long long pc0 = 0, pc1 = 0, pc2 = 0, pc3 = 0, pc4 = 0, tl = prof ? prof_now() : 0ull;
  for (int t = 0; t < T; ++t) {
    const int par = t & 1;
    const unsigned gtag = (unsigned)(t + 1);
    // prefetch the next step's noise (lands during this step)
    float noise_next = 0.f;
    const int pe = tid / MAX_ACT, pk = tid % MAX_ACT;
    const bool pf = tid < WIDE_E * MAX_ACT && pe < E && pk < NA && t + 1 < T;
    if (pf) noise_next = a.noise[((size_t)(t + 1) * N + g + pe * G) * NA + pk];
    // ---------------- phase A: policy forward, env step, cost, buffer rows for each env of this workgroup ----------------
    for (int e = 0; e < E; ++e) {
      const int n = g + e * G;
      const size_t tn = (size_t)t * N + n;
      policy_forward_block<OCT>(a.pl, R, sh[e], noise_s[par][e], 0, has_box ? alow_s : nullptr, has_box ? ahigh_s : nullptr);
      __syncthreads();
      const int xrec = (par * N + n) * R16 * 16;      // byte offset of the env's records of this parity
      if (w == 0) {
        double rew; int done;
        uint32_t e_ctr = ctr_s[e];
        int e_tep = tep_s[e];
        env_step_wave(env, n, sh[e].s_old, sh[e].act_clip, a.env.key[n], e_ctr, e_tep, sh[e].s_new, rew, done);
        float* nob = a.buf.new_orig_observations + tn * O;
        for (int i = lane; i < O; i += WAVE) {
          const double v = sh[e].s_new[i];
          nob[i] = (float)v;
          const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
          rstore(xrs, xrec + 16 * i, rec_u4{gtag, (unsigned)bits, (unsigned)(bits >> 32), gtag});
        }
        if (lane == 0) {
          const unsigned long long bits = (unsigned long long)__double_as_longlong(rew);
          rstore(xrs, xrec + 16 * O, rec_u4{gtag, (unsigned)bits, (unsigned)(bits >> 32), gtag | (done ? 0x80000000u : 0u)});
          ctr_s[e] = e_ctr; tep_s[e] = e_tep; rew_s[e] = rew; done_s[e] = done;
        }
      } else if (w == 3) {
        float cost = 0.f;
        if constexpr (REGION) cost = cost_region_wave(rtab, a.cr.n_clauses, a.cr.combine, sh[e].s_old, sh[e].act_clip, O);
        else if constexpr (CIT == 0) cost = cost_fn_wave(cf, sh[e].s_old, sh[e].act_clip);
        else if (a.has_cn) cost = cost_forward_wave<CIT>(a.cn, a.cl, C, sh[e].s_old, sh[e].act_clip, sh[e].cx, sh[e].ch, DISC ? 1 : 0);
        if (lane == 0) {
          rstore(xrs, xrec + 16 * (O + 1), rec_u4{gtag, __float_as_uint(cost), 0u, gtag});
          a.buf.orig_costs[tn] = cost;
          cost_s[e] = cost;
        }
      } else if (w == 2) {
        float* ob = a.buf.observations + tn * O;
        float* oob = a.buf.orig_observations + tn * O;
        for (int i = lane; i < O; i += WAVE) { ob[i] = sh[e].x[i]; oob[i] = (float)sh[e].s_old[i]; }
        if (lane < AS) a.buf.actions[tn * AS + lane] = sh[e].act_raw[lane];
        if (lane < A && !a.pl.discrete) a.ag.act_clipped[(size_t)n * A + lane] = sh[e].act_clip[lane];
        if (lane == 0) {
          a.buf.dones[tn] = (float)last_done_s[e];
          a.buf.reward_values[tn] = sh[e].scal[0];
          a.buf.cost_values[tn] = sh[e].scal[1];
          a.buf.log_probs[tn] = sh[e].scal[2];
          a.ag.last_v_r[n] = sh[e].scal[0];
          a.ag.last_v_c[n] = sh[e].scal[1];
        }
      }
    }
    if (prof) { const unsigned long long tn_ = prof_now(); pc0 += tn_ - tl; tl = tn_; }     // policy + env + rows (this wave's part)
    const bool trace = PROF && p.prof != 0 && t == T / 2 && lane == 0;
    if (trace && w == 0) g_wide_trace[4 * g + 0] = __builtin_amdgcn_s_memrealtime();
    // ---------------- phase B1: the owners (wave 1) gather their statistic from all envs and publish it ----------------
    if (w == 1 && (own_col >= 0 || own_ret || own_cost)) {
      const int slot = own_col >= 0 ? own_col : (own_ret ? O : O + 1);      // the record of every env this owner gathers
      const bool wide = !own_cost;                                   // a float64 in the record, or the float32 cost
      const int gbase = par * N * R16 * 16;
      // four blocks of 64 envs per polling round: all their loads are in flight together (one trip through the memory system
      // per round instead of one per block)
      for (int i0 = 0; i0 < N; i0 += 4 * WAVE) {
        rec_u4 g0[4], gd[4];          // gd: the reward record of the env — the cost owner takes the done flag from its tag
        bool ok[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { g0[k] = gd[k] = rec_u4{0u, 0u, 0u, 0u}; ok[k] = i0 + k * WAVE + lane >= N; }
        for (int spins = 0; spins < spin_limit; ++spins) {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int i = i0 + k * WAVE + lane;
            if (!ok[k]) { g0[k] = rload(xrs, gbase + (i * R16 + slot) * 16); gd[k] = own_cost ? rload(xrs, gbase + (i * R16 + O) * 16) : g0[k]; }
          }
          bool all = true;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            if (!ok[k]) ok[k] = g0[k][0] == gtag && (g0[k][3] & 0x7fffffffu) == gtag && gd[k][0] == gtag && (gd[k][3] & 0x7fffffffu) == gtag;
            all = all && ok[k];
          }
          if (__all(all)) break;
          if (spins + 1 == spin_limit) spin_limit = 1;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int i = i0 + k * WAVE + lane;
          if (i < N) {
            double v;
            if (wide) v = __longlong_as_double((long long)(((unsigned long long)g0[k][2] << 32) | (unsigned long long)g0[k][1]));
            else v = (double)__uint_as_float(g0[k][1]);
            if (own_col >= 0) colbuf[i] = v;
            else {
              const double ret = retbuf[i] * (own_ret ? nm.reward_gamma : nm.cost_gamma) + v;     // vec_normalize.py:102, 245
              colbuf[i] = ret;
              done_all[i] = (int)(gd[k][3] >> 31);
            }
          }
        }
      }
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_s_waitcnt(0xC07F);
      if (prof) { const unsigned long long tn_ = prof_now(); pc1 += tn_ - tl; tl = tn_; }   // owner: gather (wait for all envs)
      if (trace) g_wide_trace[4 * g + 1] = __builtin_amdgcn_s_memrealtime();
      double bm, bv;
      if (own_col >= 0) {
        column_moments_contig(colbuf, N, bm, bv);                   // every lane computes the same chain (numpy's axis-0 order)
      } else {
        bm = np_pairwise_sum_wave(colbuf, N) / (double)N;           // numpy's 1-D pairwise order
        for (int i = lane; i < N; i += WAVE) { const double d = colbuf[i] - bm; dev2buf[i] = d * d; }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_waitcnt(0xC07F);
        bv = np_pairwise_sum_wave(dev2buf, N) / (double)N;
      }
      chan_merge(o_mean, o_var, o_cnt, bm, bv, (double)N);
      o_cnt = (double)N + o_cnt;
      const int sbase = par * (GS / 2) * 16;          // statistics records of this parity: (mean, var) per column, then the two denominators
      if (lane == 0) {
        if (own_col >= 0) {
          const unsigned long long mb = (unsigned long long)__double_as_longlong(o_mean), vb = (unsigned long long)__double_as_longlong(o_var);
          rstore(srs, sbase + 32 * own_col, rec_u4{gtag, (unsigned)mb, (unsigned)(mb >> 32), gtag});
          rstore(srs, sbase + 32 * own_col + 16, rec_u4{gtag, (unsigned)vb, (unsigned)(vb >> 32), gtag});
        } else {
          const unsigned long long db = (unsigned long long)__double_as_longlong(sqrt(o_var + nm.epsilon));
          rstore(srs, sbase + (2 * O + (own_ret ? 0 : 1)) * 16, rec_u4{gtag, (unsigned)db, (unsigned)(db >> 32), gtag});
        }
      }
      if (own_col < 0)      // returns of finished episodes restart at 0 (vec_normalize.py:99, 241)
        for (int i = lane; i < N; i += WAVE) retbuf[i] = done_all[i] ? 0.0 : colbuf[i];
      if (prof) { const unsigned long long tn_ = prof_now(); pc2 += tn_ - tl; tl = tn_; }   // owner: moments + merge + publish
      if (trace) g_wide_trace[4 * g + 2] = __builtin_amdgcn_s_memrealtime();
    }
    // ---------------- phase B2: everybody reads the statistics granules, then normalises its own envs ----------------
    {
      const int sbase = par * (GS / 2) * 16;
      const int total = has_cost ? GS / 2 : GS / 2 - 1;              // records: (mean, var) per column, ret denominator, cost denominator
      for (int i0 = 0; i0 < total; i0 += 256) {
        const int i = i0 + tid;
        rec_u4 gv = rec_u4{gtag, 0u, 0u, gtag};
        bool ok = i >= total;
        for (int spins = 0; spins < spin_limit && !ok; ++spins) {
          gv = rload(srs, sbase + i * 16);
          ok = gv[0] == gtag && gv[3] == gtag;
          if (!ok) __builtin_amdgcn_s_sleep(1);
        }
        if (!ok) spin_limit = 1;
        if (i < total) {
          const double v = __longlong_as_double((long long)(((unsigned long long)gv[2] << 32) | (unsigned long long)gv[1]));
          if (i < 2 * O) { if (i & 1) var_s[i >> 1] = v; else mean_s[i >> 1] = v; }
          else dens_s[i - 2 * O] = v;
        }
      }
    }
    __syncthreads();
    if (prof) { const unsigned long long tn_ = prof_now(); pc3 += tn_ - tl; tl = tn_; }     // statistics granules arrived
    if (trace && w == 0) g_wide_trace[4 * g + 3] = __builtin_amdgcn_s_memrealtime();
    for (int e = 0; e < E; ++e) {
      const int n = g + e * G;
      const size_t tn = (size_t)t * N + n;
      if (tid < O) {
        double o = sh[e].s_new[tid];
        if (nm.norm_obs) o = fmin(fmax((o - mean_s[tid]) / sqrt(var_s[tid] + nm.epsilon), -nm.clip_obs), nm.clip_obs);
        olast[e][tid] = o;
        sh[e].x[tid] = (float)o;
        a.buf.new_observations[tn * O + tid] = (float)o;
        sh[e].s_old[tid] = sh[e].s_new[tid];
      }
      if (tid == 64) {
        double r = rew_s[e];
          if (nm.norm_reward) r = fmin(fmax(r / dens_s[0], -nm.clip_reward), nm.clip_reward);
        a.buf.rewards[tn] = (float)r;
        if (has_cost) {
          double c = (double)cost_s[e];
          if (nm.norm_cost) c = fmin(fmax(c / dens_s[1], -nm.clip_cost), nm.clip_cost);
          a.buf.costs[tn] = (float)c;
        }
        last_done_s[e] = done_s[e];
        if (MON) a.raw_plane[tn] = rew_s[e];
      }
    }
    if (pf) noise_s[par ^ 1][pe][pk] = noise_next;
    __syncthreads();
    if (prof) { const unsigned long long tn_ = prof_now(); pc4 += tn_ - tl; tl = tn_; }     // normalise + rows
  }
  if (prof && (tid == 0 || tid == 64)) {      // wave 0: policy wave's view; wave 1: the owner's
    unsigned long long* o = g_rollout_prof_wide + (tid == 64 ? 8 : 0);
    o[0] = pc0; o[1] = pc1; o[2] = pc2; o[3] = pc3; o[4] = pc4; o[5] = (unsigned long long)T;
  }
  if (spin_limit == 1 && a.ag.status != nullptr && (tid & 63) == 0) atomicOr(a.ag.status, 1);
  // ---- leave the agent / wrapper / normaliser state exactly where the per-step path leaves it
  for (int e = 0; e < E; ++e) {
    const int n = g + e * G;
    if (tid < O) a.ag.last_obs[(size_t)n * O + tid] = olast[e][tid];
    if (tid == 0) {
      a.ag.last_dones[n] = (uint8_t)last_done_s[e];
      a.ag.raw_rew[n] = rew_s[e]; a.ag.dones[n] = (uint8_t)done_s[e];
      if (has_cost) a.ag.raw_cost[n] = cost_s[e];
    }
  }
  if (w == 1 && lane == 0) {
    if (own_col >= 0) { nm.obs_mean[own_col] = o_mean; nm.obs_var[own_col] = o_var; if (own_col == 0) nm.obs_count[0] = o_cnt; }
    if (own_ret) { nm.ret_stats[0] = o_mean; nm.ret_stats[1] = o_var; nm.ret_stats[2] = o_cnt; }
    if (own_cost) { nm.cost_stats[0] = o_mean; nm.cost_stats[1] = o_var; nm.cost_stats[2] = o_cnt; }
  }
  if (w == 1 && (own_ret || own_cost))
    for (int i = lane; i < N; i += WAVE) { if (own_ret) nm.ret[i] = retbuf[i]; else nm.cost_ret[i] = retbuf[i]; }
}

// =================================================================================================================
// persistent rollout with SEVERAL environments per workgroup, evaluated INTERLEAVED (throughput form)
// =================================================================================================================
// Same contract and bit-identical results as rollout_persistent_kernel / rollout_wide_kernel (every per-env operation is the
// same arithmetic: the k-ascending fmaf chains of the other kernels, evaluated here as fp32 MFMA tiles — TileRegs below —, the same
// tanh, the same float64 env step, numpy-ordered statistics), different use of the machine.  Those kernels give one environment a
// workgroup (or walk a workgroup's environments one after the other): an env step is then a 7-8 k cycle chain of dependent
// latencies.  Here workgroup g of a run serves E environments g, g + G, ... and runs every layer for all of them at once (16 units
// x 16 envs per MFMA, the weights register-resident as A operands, the activations read from LDS as B operands).  E environments
// cost little more than one, so a run needs G = N / E workgroups instead of N, all runs of a
// batched launch (icrl_rollout_collect_batch, run = blockIdx.y) are resident together, and the exchange shrinks with G:
//   phase A   layers 1, 2, heads for E envs (waves pi | vf | cvf); env steps spread over waves 0..2, cost net on wave 3;
//             raw obs / reward / cost / done published as self-validating 16-byte records (as in the other two kernels)
//   phase B1  statistic s (observation column, ret_rms, cost_rms) is owned by wave s / G of workgroup s % G: up to four
//             owners per workgroup work side by side (gather 2 N granules, numpy-ordered moments, merge, publish)
//   phase B2  every workgroup reads the 4 obs + 4 statistics granules and normalises its E envs
constexpr int MULTI_OP = 128;     // padded per-env row of the LDS state arrays (>= MAX_OBS)
// rows that feed the MFMA B operand (lane (r, q) reads element 4 ks + q of row r): a row stride of 4 mod 32 floats spreads the 64
// lanes of a read over all banks (two lanes per bank: the minimum); strides of 64 / 128 would put 16 lanes on one bank
constexpr int MULTI_XS = MULTI_OP + 4;
constexpr int MULTI_HS = MAX_H + 4;
#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)
// per-wave constants read back as 16-byte rows where they are used (they would cost 84 registers per lane next to the weights):
// by unit j: b1 | b2 | output weight (value / cost-value / cost net);  by action a (wave 0): bias | exp(log_std) | log(sd) | 2 sd^2;  [CST_BO]: output bias
constexpr int CST_B1 = 0, CST_B2 = 64, CST_WO = 128, CST_BA = 192, CST_SD = 208, CST_LSD = 224, CST_I2V = 240, CST_BO = 256, MULTI_CST = 260;

template <int E, int CIT>
struct MultiShared {
  alignas(16) float x[E][MULTI_XS];          // normalised observation (policy input), pad = 0
  alignas(16) double s_old[E][MULTI_OP];
  alignas(16) double s_new[E][MULTI_OP];
  alignas(16) double olast[E][MULTI_OP];     // normalised observation in float64 (== _last_obs)
  alignas(16) float h[4][E][MULTI_HS];       // per wave (pi | vf | cvf | cost net): the layer output it turns into its next B operand
  alignas(16) float cx[E][16 * CIT + 4];     // cost-net inputs of every env
  alignas(16) float cst[4][MULTI_CST];       // per wave: biases / output weights by unit, Gaussian head constants by action (TileRegs)
  alignas(16) float act_raw[E][MAX_ACT];
  alignas(16) float act_clip[E][MAX_ACT];
  alignas(16) float noise[2][E][MAX_ACT];
  alignas(16) float alow[MAX_ACT];
  alignas(16) float ahigh[MAX_ACT];
  int xcd_local;                             // all workgroups of this run share this XCD (rollout_multi_body)
  float scal[E][4], cost[E];
  double rew[E], mean[MAX_OBS], var[MAX_OBS], dens[2];
  unsigned ctr[E], key[E];
  int tep[E], last_done[E], done[E];
};

// Register image of one wave of the multi-env kernel: the weights as MFMA A operands.  v_mfma_f32_16x16x4_f32 accumulates its four
// products one after the other in k order with the rounding of fmaf (tools/ubench: a chain of them equals the chain
// acc = fmaf(w[k], x[k], acc), k ascending, bit for bit in 51 200 of 51 200 outputs), so Z^T[unit][env] = W . X^T evaluated as
// 16-unit x 16-env tiles gives every (unit, env) exactly the value of the per-environment fmaf chains of the other rollout kernels.
// Lane (r = lane % 16, q = lane / 16): A operand of tile t, k step ks = W[unit 16 t + r][k = 4 ks + q]; the tile's result registers
// i = 0..3 hold unit 16 t + 4 q + i of env r.
template <int OCT, int CIT>
struct TileRegs {
  static constexpr int K1 = 4 * (OCT > CIT ? OCT : CIT);
  float w1[4][K1];        // first layer (policy nets: 4 OCT k steps used | cost net: 4 CIT)
  float w2[4][16];        // second layer
  float wh[16];           // wave 0: Wa[action r][k = 4 ks + q] at [ks] (the other per-unit / per-action constants: MultiShared::cst)
  static constexpr int NSEL = (16 * (CIT > 0 ? CIT : 1) + WAVE - 1) / WAVE;
  int sel[NSEL];          // cost net: select_dim entries this lane prepares ...
  float plo[NSEL], phi[NSEL];        // ... their action bounds (ConstraintNet.clip_actions) ...
  double pmean[NSEL], pden[NSEL];    // ... and observation statistics (--cn_normalize: mean, sqrt(var + eps)): constants of the rollout
};

template <int OCT, int CIT>
__device__ __forceinline__ void load_pol_tiles(const PolLayout& L, const float* __restrict__ PT, TileRegs<OCT, CIT>& R, float* cst) {
  const int lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int net = w < 3 ? w : 0;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int ju = 16 * t + r;
#pragma unroll
    for (int ks = 0; ks < 4 * OCT; ++ks) { const int k = 4 * ks + q; R.w1[t][ks] = (ju < L.H1 && k < L.O) ? PT[L.W1[net] + k * L.H1 + ju] : 0.f; }
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) { const int k = 4 * ks + q; R.w2[t][ks] = (ju < L.H2 && k < L.H1) ? PT[L.W2[net] + k * L.H2 + ju] : 0.f; }
  }
#pragma unroll
  for (int ks = 0; ks < 16; ++ks) { const int k = 4 * ks + q; R.wh[ks] = (w == 0 && r < L.A && k < L.H2) ? PT[L.Wa + k * L.A + r] : 0.f; }
  {
    const int j = lane;
    cst[CST_B1 + j] = j < L.H1 ? PT[L.b1[net] + j] : 0.f;
    cst[CST_B2 + j] = j < L.H2 ? PT[L.b2[net] + j] : 0.f;
    cst[CST_WO + j] = (w != 0 && j < L.H2) ? PT[(w == 1 ? L.Wv : L.Wc) + j] : 0.f;
    if (j < 16) {
      // constants of the whole rollout: evaluated once here instead of once per env step (same expressions as load_pol_regs)
      const int a = j < L.A ? j : 0;
      const float ls = (w == 0 && !L.discrete) ? PT[L.log_std + a] : 0.f;
      const float sd = expf(ls);
      cst[CST_BA + j] = w == 0 ? PT[L.ba + a] : 0.f;
      cst[CST_SD + j] = sd; cst[CST_LSD + j] = logf(sd); cst[CST_I2V + j] = 2.f * (sd * sd);
    }
    if (j == 0) cst[CST_BO] = w == 0 ? 0.f : PT[w == 1 ? L.bv : L.bc];
  }
}

template <int OCT, int CIT>
__device__ __forceinline__ void load_cn_tiles(const icrl_costnet_t& cn, const CnLayout& L, TileRegs<OCT, CIT>& R, float* cst) {
  const int lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
  const float* PT = cn.params_t;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int ju = 16 * t + r;
#pragma unroll
    for (int ks = 0; ks < 4 * CIT; ++ks) { const int k = 4 * ks + q; R.w1[t][ks] = (ju < L.H1 && k < L.in) ? PT[L.W0 + k * L.H1 + ju] : 0.f; }
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) { const int k = 4 * ks + q; R.w2[t][ks] = (L.nh == 2 && ju < L.H2 && k < L.H1) ? PT[L.W1 + k * L.H2 + ju] : 0.f; }
  }
#pragma unroll
  for (int ks = 0; ks < 16; ++ks) R.wh[ks] = 0.f;
  {
    const int j = lane;
    cst[CST_B1 + j] = j < L.H1 ? PT[L.b0 + j] : 0.f;
    cst[CST_B2 + j] = (L.nh == 2 && j < L.H2) ? PT[L.b1 + j] : 0.f;
    cst[CST_WO + j] = j < L.H2 ? PT[L.Wo + j] : 0.f;
    if (j == 0) cst[CST_BO] = PT[L.bo];
  }
#pragma unroll
  for (int i = 0; i < (16 * CIT + WAVE - 1) / WAVE; ++i) {
    const int idx = lane + i * WAVE;
    const int sel = idx < L.in ? cn.select_dim[idx] : -1;
    R.sel[i] = sel;
    R.plo[i] = 0.f; R.phi[i] = 0.f; R.pmean[i] = 0.0; R.pden[i] = 1.0;
    if (sel >= 0 && sel < cn.obs_dim) {
      if (cn.obs_mean != nullptr && cn.obs_var != nullptr) { R.pmean[i] = cn.obs_mean[sel]; R.pden[i] = sqrt(cn.obs_var[sel] + cn.eps); }
    } else if (sel >= 0) {
      const int ai = sel - cn.obs_dim;
      if (cn.action_low != nullptr && cn.action_high != nullptr) { R.plo[i] = cn.action_low[ai]; R.phi[i] = cn.action_high[ai]; }
    }
  }
}

// wave_sum_fast's association for a value that lives as [tile t][i] = element 16 t + 4 q + i of env r: element c + 16 m sits in
// lane c + 16 m there, here c = 4 q + i and m = t.  wave_sum_fast: u[c] = (v[c] + v[c + 32]) + (v[c + 16] + v[c + 48]), then the
// 16 u's as ((u0 + u1) + (u2 + u3)) quads, quads pairwise, halves.  Returns the sum of env r in all four q lanes.
__device__ __forceinline__ float tile_sum64(const f32x4 (&v)[4]) {
  float u[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) u[i] = (v[0][i] + v[2][i]) + (v[1][i] + v[3][i]);
  const float quad = (u[0] + u[1]) + (u[2] + u[3]);
  return xor32_sum(xor16_sum(quad));
}

// synthetic env step of up to THREE environments at once by one wave (obs_dim <= 21): lane 21 s + i handles component i of the env in
// slot s.  em / n / mine are PER-LANE: the env's slot in the workgroup's LDS state, its index in the run, and whether the lane has an
// env at all.  The per-component arithmetic, the reward and the auto-reset draw are env_step_wave's, operation for operation; only
// the lanes they run on differ.  Leaves s_new, ctr, tep, rew, done of every handled env in `sh`.
template <int E, int CIT>
__device__ __noinline__ void env_step_wave3(int O, int A, int flags, int max_steps, const double __attribute__((address_space(3)))* B,
                                            double* s_all, int32_t* t_ep_all, uint32_t* step_count_all,
                                            MultiShared<E, CIT> __attribute__((address_space(3)))* shp,
                                            int em, int n, bool mine, int ci, int slot) {
  // (not inlined — inlined, the kernel spills; so everything comes in by value: the env's few scalars (flags = broken | reward_form << 1
  // | wall_terminate << 8), the workgroup's LDS state and the LDS copy of the dynamics matrix as LDS-address-space pointers, the env
  // arrays as global pointers — through a struct reference every access would be a flat_* instruction)
  MultiShared<E, CIT> __attribute__((address_space(3)))& sh = *shp;
  const bool broken = flags & 1, wall_terminate = (flags >> 8) & 1;
  const int reward_form = (flags >> 1) & 127;
  const bool live = mine && ci < O;
  double a[MAX_ACT];
  double sq = 0.0;
#pragma unroll
  for (int j = 0; j < MAX_ACT; ++j) {
    a[j] = 0.0;
    if (j < A) {
      a[j] = (double)sh.act_clip[em][j];
      if (broken && j >= 4) a[j] = 0.0;
      sq = sq + a[j] * a[j];
    }
  }
  const uint32_t ky = sh.key[em], ct = sh.ctr[em];
  const int i = ci < O ? ci : 0;
  double ns = 0.0;
  {
    double acc = 0.99 * sh.s_old[em][i];
    const double __attribute__((address_space(3)))* Bi = B + (size_t)i * A;
#pragma unroll
    for (int j = 0; j < MAX_ACT; ++j)
      if (j < A) acc = acc + Bi[j] * a[j];
    const double eps = (unit_uniform(ky, ct, (uint32_t)i) - 0.5) * 3.4641016151377544;
    ns = acc + 0.01 * eps;
  }
  const int base = 21 * (slot < 3 ? slot : 0);
  const double n0 = __shfl(ns, base, 64);
  const double n1 = __shfl(ns, base + 1, 64);
  double rw;
  if (reward_form == 0) rw = fabs(n0 - sh.s_old[em][0]) / 0.05 - 0.1 * sq;
  else rw = (sqrt(n0 * n0 + n1 * n1) + 1.0) - 0.5 * sq;
  int d = 0;
  if (wall_terminate && n0 <= -3.0) { rw = 0.0; d = 1; }
  const int tep = sh.tep[em] + 1;
  if (tep >= max_steps) d = 1;
  __builtin_amdgcn_wave_barrier();           // every lane has read ctr / tep / s_old before lane 0 of a slot replaces them
  if (live) {
    double v = ns;
    if (d) v = reward_form >= 2 ? -1.0 : (unit_uniform(ky, ct + 1u, (uint32_t)(O + i)) - 0.5) * 0.2;   // auto-reset draw (env_reset_value)
    as_global(s_all)[(size_t)n * O + i] = v;
    sh.s_new[em][i] = v;
  }
  if (mine && ci == 0) {
    const int tnew = d ? 0 : tep;
    sh.tep[em] = tnew; sh.ctr[em] = ct + 1u; sh.rew[em] = rw; sh.done[em] = d;
    as_global(t_ep_all)[n] = tnew; as_global(step_count_all)[n] = ct + 1u;
  }
}

template <int OCT, int CIT, int E, bool MON, bool DISC = false, bool REGION = false>
__device__ __forceinline__ void rollout_multi_body(const WideArgs& p, const int g_arg) {
  extern __shared__ __attribute__((aligned(16))) double dyn_lds[];
  __shared__ MultiShared<E, CIT> sh;
  const ActStepArgs& a = p.act;
  REGION_TABLE(a, (int)threadIdx.x, 256)      // (published by the barriers in front of the step loop)
  // private copies of the structs whose pointers the step loop goes through, every pointer marked as a global-memory pointer
  // (common.h: as_global — in a batched launch the block comes from memory and the accesses would be flat_* otherwise)
  icrl_norm_t nm = p.nm; globalize(nm);
  icrl_buffer_t buf = a.buf; globalize(buf);
  icrl_agent_t ag = a.ag; globalize(ag);
  icrl_costnet_t cnet = a.cn; globalize(cnet);
  unsigned long long* const xg_all = as_global(p.xg);      // granules of every env, both parities
  unsigned long long* const sg_all = as_global(p.sg);      // statistics granules
  const float* const noise_g = as_global(a.noise);
  double* const raw_plane = MON ? as_global(a.raw_plane) : nullptr;
  TileRegs<OCT, CIT> R;                // waves 0..2: policy / value / cost-value net, wave 3: cost net — as MFMA A operands
  if constexpr (CIT > 0) {
    if (threadIdx.x >= 192 && a.has_cn) load_cn_tiles<OCT, CIT>(a.cn, a.cl, R, sh.cst[3]);
    else load_pol_tiles<OCT, CIT>(a.pl, a.PT, R, sh.cst[threadIdx.x >> 6]);
  } else {                             // analytic cost (CIT == 0): no cost tiles are loaded or run
    load_pol_tiles<OCT, CIT>(a.pl, a.PT, R, sh.cst[threadIdx.x >> 6]);
  }
  const icrl_cost_fn_t cf = a.cf;      // analytic cost: kind, index and thresholds are read once, before the step loop
  const int g = g_arg, G = p.G;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int O = a.pl.O, A = a.pl.A, N = a.env.n_envs, T = p.T;
  const int AS = buf.act_store;
  const int GX = 2 * O + 4, GS = 4 * O + 4;
  // Exchange records: 16 bytes {tag, lo, hi, tag} instead of two 8-byte {tag, word} granules per float64 (same bytes, half the memory
  // instructions; the done flag rides in the top bit of the reward record's second tag).  Per env R16 = obs + 2 records (obs columns,
  // reward, cost); statistics: (mean, var) per column, then the ret / cost denominators.
  const int R16 = O + 2;
  typedef unsigned int rec_u4 __attribute__((ext_vector_type(4)));
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(xg_all, 0, 2 * N * GX * 8, 0x00020000);
  const __amdgpu_buffer_rsrc_t srs = __builtin_amdgcn_make_buffer_rsrc(sg_all, 0, 2 * GS * 8, 0x00020000);
  // record stores: `sc1` (agent scope), or `sc0` when every workgroup of this run sits on this XCD (xcd_local, set below): the line then
  // stays in the XCD's L2 for the other workgroups' `sc1` loads instead of being dropped (ppo_common.h, "XCD placement"; measured at
  // HC x 64, 8 envs per workgroup: 12.2 -> 10.7 us per step).  Records carry their step tag at both ends: a stale read retries.
  bool xcd_local = false;
  auto rstore = [&](const __amdgpu_buffer_rsrc_t& rs, int byte_off, rec_u4 v) {
    if (xcd_local) __builtin_amdgcn_raw_buffer_store_b128(v, rs, byte_off, 0, 1);      // sc0
    else __builtin_amdgcn_raw_buffer_store_b128(v, rs, byte_off, 0, 16);               // sc1
  };
  auto rload = [](const __amdgpu_buffer_rsrc_t& rs, int byte_off) -> rec_u4 { return __builtin_amdgcn_raw_buffer_load_b128(rs, byte_off, 0, 16); };
  const int Eg = (N - g + G - 1) / G;                // envs of this workgroup (1 .. E)
  const bool has_cost = a.has_cn != 0;
  const bool has_box = a.alow != nullptr && a.ahigh != nullptr;
  const int n_stats = O + (has_cost ? 2 : 1);
  const int owners = (n_stats + G - 1) / G;          // owner waves per workgroup (<= 4: checked by the launcher)
  double* const Bl = dyn_lds;
  double* const colbuf = Bl + O * a.env.act_dim + (size_t)w * (N + 64);      // this wave's column buffer (owner waves only)
  unsigned char* const done_bufs = reinterpret_cast<unsigned char*>(Bl + O * a.env.act_dim + (size_t)owners * (N + 64));
  icrl_env_t env = a.env; globalize(env);
  for (int i = tid; i < O * a.env.act_dim; i += 256) Bl[i] = a.env.B[i];
  env.B = Bl;
  const int env_flags = (env.broken ? 1 : 0) | (env.reward_form << 1) | (env.wall_terminate ? 256 : 0);
  if (tid < MAX_ACT) { sh.alow[tid] = (has_box && tid < A) ? a.alow[tid] : 0.f; sh.ahigh[tid] = (has_box && tid < A) ? a.ahigh[tid] : 0.f; }
  for (int idx = tid; idx < E * MULTI_OP; idx += 256) {
    const int e = idx / MULTI_OP, i = idx % MULTI_OP;
    const bool live = e < Eg && i < O;
    const int n = g + e * G;
    const double lo = live ? ag.last_obs[(size_t)n * O + i] : 0.0;
    sh.x[e][i] = (float)lo;
    sh.olast[e][i] = lo;
    sh.s_old[e][i] = live ? a.env.s[(size_t)n * O + i] : 0.0;
    sh.s_new[e][i] = 0.0;
  }
  if (tid < E) {
    const int e = tid, n = g + (e < Eg ? e : 0) * G;
    sh.ctr[e] = a.env.step_count[n]; sh.tep[e] = a.env.t_ep[n]; sh.last_done[e] = ag.last_dones[n]; sh.key[e] = a.env.key[n];
    sh.rew[e] = 0.0; sh.cost[e] = 0.f; sh.done[e] = 0;
  }
  // the statistic this WAVE owns (if any): sid = g + w * G
  const int sid = g + w * G;
  const bool owner = w < owners && sid < n_stats;
  const int own_col = (owner && sid < O) ? sid : -1;
  const bool own_ret = owner && sid == O, own_cost = owner && has_cost && sid == O + 1;
  double* const retbuf = own_cost ? nm.cost_ret : nm.ret;           // [N] in global memory: this wave is its only user during the launch
  unsigned char* const done_all = done_bufs + (own_cost ? (size_t)((N + 15) / 16 * 16) : 0);
  double o_mean = 0.0, o_var = 1.0, o_cnt = 0.0;
  if (own_col >= 0) { o_mean = nm.obs_mean[own_col]; o_var = nm.obs_var[own_col]; o_cnt = nm.obs_count[0]; }
  if (own_ret) { o_mean = nm.ret_stats[0]; o_var = nm.ret_stats[1]; o_cnt = nm.ret_stats[2]; }
  if (own_cost) { o_mean = nm.cost_stats[0]; o_var = nm.cost_stats[1]; o_cnt = nm.cost_stats[2]; }
  const int NA = A;                                  // (continuous actions only: the launcher keeps discrete policies elsewhere)
  if (tid < E * MAX_ACT) {
    const int e = tid / MAX_ACT, k = tid % MAX_ACT;
    sh.noise[0][e][k] = (e < Eg && k < NA) ? noise_g[((size_t)(g + e * G)) * NA + k] : 0.f;
  }
  const int r16 = lane & 15, q4 = lane >> 4;          // MFMA lane coordinates: env row r16, k / unit quarter q4
  const int er = r16 < E ? r16 : E - 1;               // rows beyond E replicate the last env's row (their results are not used)
  const int nk1 = (O + 3) / 4, nkc = a.has_cn ? (a.cl.in + 3) / 4 : 0;
  const int pH1 = a.pl.H1, pH2 = a.pl.H2, cH1 = a.cl.H1, cH2 = a.cl.H2, cnh = a.cl.nh;      // (read once: the block may live in LDS)
  const bool cn_norm = a.has_cn && cnet.obs_mean != nullptr && cnet.obs_var != nullptr;
  const bool cn_box = a.has_cn && cnet.action_low != nullptr && cnet.action_high != nullptr;
  const double cn_clip = cnet.clip_obs;
  int spin_limit = 1 << 22;
  if (p.xcc != nullptr && tid == 0) sh.xcd_local = all_on_one_xcd(as_global(p.xcc), 1, g, G) ? 1 : 0;
  __syncthreads();
  if (p.xcc != nullptr) xcd_local = __builtin_amdgcn_readfirstlane(sh.xcd_local) != 0;
  const bool prof = p.prof != 0 && g == p.prof - 1 && blockIdx.y == 0;
  unsigned long long pc0 = 0, pc1 = 0, pc2 = 0, pc3 = 0, pc4 = 0, pcA = 0, pcB = 0, tl = prof ? prof_now() : 0ull;
  for (int t = 0; t < T; ++t) {
    const int par = t & 1;
    const unsigned gtag = (unsigned)(t + 1);
    float noise_next = 0.f;
    const int pe = tid / MAX_ACT, pk = tid % MAX_ACT;
    const bool pf = tid < E * MAX_ACT && pe < Eg && pk < NA && t + 1 < T;
    if (pf) noise_next = noise_g[((size_t)(t + 1) * N + g + pe * G) * NA + pk];
    // ---------------- phase A: the three MLPs for all E envs at once, as MFMA tiles (TileRegs) ----------------
    // A wave consumes only its own network's activations: the hand-over between layers (result layout [unit 16 t + 4 q + i][env r]
    // -> B operand layout [k = 4 ks + q][env r]) goes through the wave's own LDS rows, no workgroup barrier until the heads are done.
    if (w < 3) {
      f32x4 z[4], cb[4];
      float bop[16];
      const float* const cw = &sh.cst[w][4 * q4];       // this lane's slice of the wave's constants: + CST_x + 16 t
#pragma unroll
      for (int t = 0; t < 4; ++t) { z[t] = f32x4{0.f, 0.f, 0.f, 0.f}; cb[t] = *reinterpret_cast<const f32x4*>(cw + CST_B1 + 16 * t); }
      {
        const float* xb = &sh.x[er][q4];
        float bx[4 * OCT];              // every B operand of the layer in flight before the first MFMA (pad columns are zero)
#pragma unroll
        for (int ks = 0; ks < 4 * OCT; ++ks) bx[ks] = xb[4 * ks];
#pragma unroll
        for (int ks = 0; ks < 4 * OCT; ++ks) {
          if (ks < nk1) {               // (k steps that only meet padding — zero weights — are not issued)
#pragma unroll
            for (int t = 0; t < 4; ++t) z[t] = MFMA16(R.w1[t][ks], bx[ks], z[t]);
          }
        }
      }
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) z[t][i] = 16 * t + 4 * q4 + i < pH1 ? fast_tanh(z[t][i] + cb[t][i]) : 0.f;
      if (r16 < E) {
#pragma unroll
        for (int t = 0; t < 4; ++t) *reinterpret_cast<f32x4*>(&sh.h[w][r16][16 * t + 4 * q4]) = z[t];
      }
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_s_waitcnt(0xC07F);
      {
        const float* hb = &sh.h[w][er][q4];
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) bop[ks] = hb[4 * ks];
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) { z[t] = f32x4{0.f, 0.f, 0.f, 0.f}; cb[t] = *reinterpret_cast<const f32x4*>(cw + CST_B2 + 16 * t); }
#pragma unroll
      for (int ks = 0; ks < 16; ++ks)
#pragma unroll
        for (int t = 0; t < 4; ++t) z[t] = MFMA16(R.w2[t][ks], bop[ks], z[t]);
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) z[t][i] = 16 * t + 4 * q4 + i < pH2 ? fast_tanh(z[t][i] + cb[t][i]) : 0.f;
      if (w == 0) {                     // action head + Gaussian sample / log-prob of every env: lane (r, q) holds actions 4 q + i of env r
        __builtin_amdgcn_wave_barrier();        // (every lane's reads of h are consumed: the MFMAs above used them)
        if (r16 < E) {
#pragma unroll
          for (int t = 0; t < 4; ++t) *reinterpret_cast<f32x4*>(&sh.h[0][r16][16 * t + 4 * q4]) = z[t];
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_waitcnt(0xC07F);
        {
          const float* hb = &sh.h[0][er][q4];
#pragma unroll
          for (int ks = 0; ks < 16; ++ks) bop[ks] = hb[4 * ks];
        }
        f32x4 m = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) m = MFMA16(R.wh[ks], bop[ks], m);
        const f32x4 nz = *reinterpret_cast<const f32x4*>(&sh.noise[par][er][4 * q4]);
        const f32x4 lo = *reinterpret_cast<const f32x4*>(&sh.alow[4 * q4]);
        const f32x4 hi = *reinterpret_cast<const f32x4*>(&sh.ahigh[4 * q4]);
        const f32x4 hb_ = *reinterpret_cast<const f32x4*>(cw + CST_BA), sd_ = *reinterpret_cast<const f32x4*>(cw + CST_SD);
        const f32x4 lsd_ = *reinterpret_cast<const f32x4*>(cw + CST_LSD), i2v_ = *reinterpret_cast<const f32x4*>(cw + CST_I2V);
        f32x4 araw, aclip;
        float u[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float mean = m[i] + hb_[i];
          float lp = 0.f, act = 0.f, c = 0.f;
          if (4 * q4 + i < A) {
            act = mean + nz[i] * sd_[i];                  // Normal.rsample: loc + eps * scale
            const float diff = act - mean;
            lp = -(diff * diff) / i2v_[i] - lsd_[i] - LOG_SQRT_2PI_F;
            c = act;
            if (has_box) c = fminf(fmaxf(act, lo[i]), hi[i]);
          }
          araw[i] = act; aclip[i] = c;
          u[i] = (lp + 0.f) + (0.f + 0.f);                // wave_sum_fast over lane = action: lanes 16.. hold 0
        }
        const float lp_env = xor32_sum(xor16_sum((u[0] + u[1]) + (u[2] + u[3])));
        if (r16 < E) {
          *reinterpret_cast<f32x4*>(&sh.act_raw[r16][4 * q4]) = araw;
          *reinterpret_cast<f32x4*>(&sh.act_clip[r16][4 * q4]) = aclip;
          if (q4 == 0) sh.scal[r16][2] = lp_env;
        }
      } else {                          // value heads: products with the output weights, summed in wave_sum_fast's order
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const f32x4 wo = *reinterpret_cast<const f32x4*>(cw + CST_WO + 16 * t);
#pragma unroll
          for (int i = 0; i < 4; ++i) z[t][i] = 16 * t + 4 * q4 + i < pH2 ? wo[i] * z[t][i] : 0.f;
        }
        const float v = tile_sum64(z) + sh.cst[w][CST_BO];
        if (r16 < E && q4 == 0) sh.scal[r16][w - 1] = v;
      }
    }
    __syncthreads();
    if (prof) { const unsigned long long tn_ = prof_now(); pc0 += tn_ - tl; tl = tn_; }     // the three MLPs + heads
    // ---------------- env steps (waves 0..2), cost net (wave 3), buffer rows ----------------
    if (OCT <= 2 && w < 3 && O <= 21 && env.reward_form < 2) {
      // narrow observations: THREE envs per pass, lane 21 s + i = component i of slot s (env 3 q + s; triple q on wave q % 3)
      const int slot = lane / 21, ci = lane - 21 * slot;
      for (int q = w; 3 * q < Eg; q += 3) {
        const int e = 3 * q + slot;
        const bool mine = slot < 3 && e < Eg;
        const int em = mine ? e : 3 * q;
        const int n = g + em * G;
        const size_t tn = (size_t)t * N + n;
        const int xrec = (par * N + n) * R16 * 16;      // byte offset of the env's records of this parity
        if (mine) {       // rows that depend on the pre-step state only
          if (ci < O) { buf.observations[tn * O + ci] = sh.x[em][ci]; buf.orig_observations[tn * O + ci] = (float)sh.s_old[em][ci]; }
          if (ci < AS) buf.actions[tn * AS + ci] = sh.act_raw[em][ci];
          if (ci < A) ag.act_clipped[(size_t)n * A + ci] = sh.act_clip[em][ci];
          if (ci == 0) {
            buf.dones[tn] = (float)sh.last_done[em];
            buf.reward_values[tn] = sh.scal[em][0];
            buf.cost_values[tn] = sh.scal[em][1];
            buf.log_probs[tn] = sh.scal[em][2];
            ag.last_v_r[n] = sh.scal[em][0];
            ag.last_v_c[n] = sh.scal[em][1];
          }
        }
        env_step_wave3<E, CIT>(O, env.act_dim, env_flags, env.max_steps, (const double __attribute__((address_space(3)))*)Bl, env.s, env.t_ep, env.step_count,
                               (MultiShared<E, CIT> __attribute__((address_space(3)))*)&sh, em, n, mine, ci, slot);
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_waitcnt(0xC07F);      // the wave's LDS writes (s_new, rew, done) are visible to its own reads
        if (mine) {
          if (ci < O) {
            const double v = sh.s_new[em][ci];
            buf.new_orig_observations[tn * O + ci] = (float)v;
            const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
            rstore(xrs, xrec + 16 * ci, rec_u4{gtag, (unsigned)bits, (unsigned)(bits >> 32), gtag});
          }
          if (ci == 0) {
            const unsigned long long bits = (unsigned long long)__double_as_longlong(sh.rew[em]);
            rstore(xrs, xrec + 16 * O, rec_u4{gtag, (unsigned)bits, (unsigned)(bits >> 32), gtag | (sh.done[em] ? 0x80000000u : 0u)});
          }
        }
      }
    } else if (w < 3) {
      for (int e = w; e < Eg; e += 3) {
        const int n = g + e * G;
        const size_t tn = (size_t)t * N + n;
        const int xrec = (par * N + n) * R16 * 16;      // byte offset of the env's records of this parity
        // rows that depend on the pre-step state only
        float* ob = buf.observations + tn * O;
        float* oob = buf.orig_observations + tn * O;
        for (int i = lane; i < O; i += WAVE) { ob[i] = sh.x[e][i]; oob[i] = (float)sh.s_old[e][i]; }
        if (lane < AS) buf.actions[tn * AS + lane] = sh.act_raw[e][lane];
        if (lane < A) ag.act_clipped[(size_t)n * A + lane] = sh.act_clip[e][lane];
        if (lane == 0) {
          buf.dones[tn] = (float)sh.last_done[e];
          buf.reward_values[tn] = sh.scal[e][0];
          buf.cost_values[tn] = sh.scal[e][1];
          buf.log_probs[tn] = sh.scal[e][2];
          ag.last_v_r[n] = sh.scal[e][0];
          ag.last_v_c[n] = sh.scal[e][1];
        }
        double rew; int done;
        uint32_t e_ctr = sh.ctr[e];
        int e_tep = sh.tep[e];
        env_step_wave(env, n, sh.s_old[e], sh.act_clip[e], sh.key[e], e_ctr, e_tep, sh.s_new[e], rew, done);
        float* nob = buf.new_orig_observations + tn * O;
        for (int i = lane; i < O; i += WAVE) {
          const double v = sh.s_new[e][i];
          nob[i] = (float)v;
          const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
          rstore(xrs, xrec + 16 * i, rec_u4{gtag, (unsigned)bits, (unsigned)(bits >> 32), gtag});
        }
        if (lane == 0) {
          const unsigned long long bits = (unsigned long long)__double_as_longlong(rew);
          rstore(xrs, xrec + 16 * O, rec_u4{gtag, (unsigned)bits, (unsigned)(bits >> 32), gtag | (done ? 0x80000000u : 0u)});
          sh.ctr[e] = e_ctr; sh.tep[e] = e_tep; sh.rew[e] = rew; sh.done[e] = done;
        }
      }
    } else if constexpr (CIT == 0) {
      // analytic cost (wave 3): one lane per env does the compare on the env's own rows
      if (lane < Eg) {
        const int n = g + lane * G;
        float cost;
        if constexpr (REGION) cost = cost_region_row(rtab, a.cr.n_clauses, a.cr.combine, sh.s_old[lane], sh.act_clip[lane], O);
        else cost = cost_fn_wave(cf, sh.s_old[lane], sh.act_clip[lane]);
        rstore(xrs, ((par * N + n) * R16 + O + 1) * 16, rec_u4{gtag, __float_as_uint(cost), 0u, gtag});
        buf.orig_costs[(size_t)t * N + n] = cost;
        sh.cost[lane] = cost;
      }
    } else if (has_cost) {
      // cost net of all E envs at once (wave 3): prepare() per env into cx, then the ReLU layers as MFMA tiles
#pragma unroll
      for (int i = 0; i < (16 * CIT + WAVE - 1) / WAVE; ++i) {
        // this lane's input component idx = lane + 64 i of EVERY env: the loads of all envs first (no branch between them), then the
        // arithmetic of prepare() — operation for operation cost_forward_wave's
        const int idx = lane + i * WAVE;
        const int sel = R.sel[i];
        const bool is_obs = sel >= 0 && sel < cnet.obs_dim, is_act = sel >= cnet.obs_dim;
        const int so = is_obs ? sel : 0, sa = is_act ? sel - cnet.obs_dim : 0;
        double ov[E];
        float av[E], a0[E];
#pragma unroll
        for (int e = 0; e < E; ++e) { ov[e] = sh.s_old[e][so]; av[e] = sh.act_clip[e][sa]; a0[e] = sh.act_clip[e][0]; }
#pragma unroll
        for (int e = 0; e < E; ++e) {
          float v = 0.f;
          if (is_obs) {
            double o = ov[e];
            if (cn_norm) o = (o - R.pmean[i]) / R.pden[i];
            if (cn_clip >= 0.0) o = fmin(fmax(o, -cn_clip), cn_clip);
            v = (float)o;
          } else if (is_act) {
            float x;
            if (cnet.is_discrete) x = ((int)a0[e] == sa) ? 1.f : 0.f;
            else x = av[e];
            if (cn_box) x = fminf(fmaxf(x, R.plo[i]), R.phi[i]);
            v = x;
          }
          if (idx < 16 * CIT) sh.cx[e][idx] = v;       // pad entries are written as 0
        }
      }
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_s_waitcnt(0xC07F);
      if (prof) pcA += prof_now() - tl;                 // (cost wave: inputs prepared)
      const int erc = r16 < Eg ? r16 : Eg - 1;          // (rows beyond the workgroup's envs replicate the last one)
      f32x4 z[4], cb[4];
      const float* const cw = &sh.cst[3][4 * q4];
#pragma unroll
      for (int t = 0; t < 4; ++t) { z[t] = f32x4{0.f, 0.f, 0.f, 0.f}; cb[t] = *reinterpret_cast<const f32x4*>(cw + CST_B1 + 16 * t); }
      {
        const float* xb = &sh.cx[erc][q4];
        float bx[4 * CIT];
#pragma unroll
        for (int ks = 0; ks < 4 * CIT; ++ks) bx[ks] = xb[4 * ks];
#pragma unroll
        for (int ks = 0; ks < 4 * CIT; ++ks) {
          if (ks < nkc) {
#pragma unroll
            for (int t = 0; t < 4; ++t)
              if (16 * t < cH1) z[t] = MFMA16(R.w1[t][ks], bx[ks], z[t]);
          }
        }
      }
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) z[t][i] = 16 * t + 4 * q4 + i < cH1 ? fmaxf(z[t][i] + cb[t][i], 0.f) : 0.f;
      if (cnh == 2) {
        if (r16 < E) {
#pragma unroll
          for (int t = 0; t < 4; ++t) *reinterpret_cast<f32x4*>(&sh.h[3][r16][16 * t + 4 * q4]) = z[t];
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_waitcnt(0xC07F);
        float bop[16];
        {
          const float* hb = &sh.h[3][er][q4];
#pragma unroll
          for (int ks = 0; ks < 16; ++ks) bop[ks] = hb[4 * ks];
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) { z[t] = f32x4{0.f, 0.f, 0.f, 0.f}; cb[t] = *reinterpret_cast<const f32x4*>(cw + CST_B2 + 16 * t); }
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
          if (4 * ks < cH1) {
#pragma unroll
            for (int t = 0; t < 4; ++t)
              if (16 * t < cH2) z[t] = MFMA16(R.w2[t][ks], bop[ks], z[t]);
          }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int i = 0; i < 4; ++i) z[t][i] = 16 * t + 4 * q4 + i < cH2 ? fmaxf(z[t][i] + cb[t][i], 0.f) : 0.f;
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const f32x4 wo = *reinterpret_cast<const f32x4*>(cw + CST_WO + 16 * t);
#pragma unroll
        for (int i = 0; i < 4; ++i) z[t][i] = 16 * t + 4 * q4 + i < cH2 ? wo[i] * z[t][i] : 0.f;
      }
      if (prof) pcB += prof_now() - tl;                 // (cost wave: hidden layers done)
      const float zz = tile_sum64(z) + sh.cst[3][CST_BO];
      const float zeta = 1.f / (1.f + expf(-zz));
      const float cost = DISC ? zeta : 1.f - zeta;
      if (q4 == 0 && r16 < Eg) {
        const int n = g + r16 * G;
        rstore(xrs, ((par * N + n) * R16 + O + 1) * 16, rec_u4{gtag, __float_as_uint(cost), 0u, gtag});
        buf.orig_costs[(size_t)t * N + n] = cost;
        sh.cost[r16] = cost;
      }
    } else {
      if (lane < Eg) {
        const int n = g + lane * G;
        rstore(xrs, ((par * N + n) * R16 + O + 1) * 16, rec_u4{gtag, __float_as_uint(0.f), 0u, gtag});
        buf.orig_costs[(size_t)t * N + n] = 0.f;
        sh.cost[lane] = 0.f;
      }
    }
    if (prof) { const unsigned long long tn_ = prof_now(); pc1 += tn_ - tl; tl = tn_; }     // env steps / cost net + rows (this wave's part)
    // ---------------- phase B1: owner waves gather their statistic from all envs and publish it ----------------
    if (own_col >= 0 || own_ret || own_cost) {
      const int slot = own_col >= 0 ? own_col : (own_ret ? O : O + 1);      // the record of every env this owner gathers
      const bool wide = !own_cost;                                   // a float64 in the record, or the float32 cost
      const int gbase = par * N * R16 * 16;
      for (int i0 = 0; i0 < N; i0 += 4 * WAVE) {
        rec_u4 g0[4], gd[4];          // gd: the reward record of the env — the cost owner takes the done flag from its tag
        bool ok[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { g0[k] = gd[k] = rec_u4{0u, 0u, 0u, 0u}; ok[k] = i0 + k * WAVE + lane >= N; }
        double rprev[4] = {0.0, 0.0, 0.0, 0.0};      // previous discounted returns (return owners): in flight while the granules are polled
        if (own_col < 0) {
#pragma unroll
          for (int k = 0; k < 4; ++k) { const int i = i0 + k * WAVE + lane; if (i < N) rprev[k] = retbuf[i]; }
        }
        for (int spins = 0; spins < spin_limit; ++spins) {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int i = i0 + k * WAVE + lane;
            if (!ok[k]) { g0[k] = rload(xrs, gbase + (i * R16 + slot) * 16); gd[k] = own_cost ? rload(xrs, gbase + (i * R16 + O) * 16) : g0[k]; }
          }
          bool all = true;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            if (!ok[k]) ok[k] = g0[k][0] == gtag && (g0[k][3] & 0x7fffffffu) == gtag && gd[k][0] == gtag && (gd[k][3] & 0x7fffffffu) == gtag;
            all = all && ok[k];
          }
          if (__all(all)) break;
          if (spins + 1 == spin_limit) spin_limit = 1;
          __builtin_amdgcn_s_sleep(1);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int i = i0 + k * WAVE + lane;
          if (i < N) {
            double v;
            if (wide) v = __longlong_as_double((long long)(((unsigned long long)g0[k][2] << 32) | (unsigned long long)g0[k][1]));
            else v = (double)__uint_as_float(g0[k][1]);
            if (own_col >= 0) colbuf[i] = v;
            else {
              colbuf[i] = rprev[k] * (own_ret ? nm.reward_gamma : nm.cost_gamma) + v;      // vec_normalize.py:102, 245
              done_all[i] = (unsigned char)(gd[k][3] >> 31);
            }
          }
        }
      }
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_s_waitcnt(0xC07F);
      double bm, bv;
      if (own_col >= 0) {
        column_moments_contig(colbuf, N, bm, bv);                   // every lane computes the same chain (numpy's axis-0 order)
      } else {
        bm = np_pairwise_sum_wave(colbuf, N) / (double)N;           // numpy's 1-D pairwise order
        // returns of finished episodes restart at 0 (vec_normalize.py:99, 241); then the squared deviations in place
        for (int i = lane; i < N; i += WAVE) { const double c = colbuf[i]; retbuf[i] = done_all[i] ? 0.0 : c; const double d = c - bm; colbuf[i] = d * d; }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_waitcnt(0xC07F);
        bv = np_pairwise_sum_wave(colbuf, N) / (double)N;
      }
      chan_merge(o_mean, o_var, o_cnt, bm, bv, (double)N);
      o_cnt = (double)N + o_cnt;
      const int sbase = par * (GS / 2) * 16;          // statistics records of this parity: (mean, var) per column, then the two denominators
      if (lane == 0) {
        if (own_col >= 0) {
          const unsigned long long mb = (unsigned long long)__double_as_longlong(o_mean), vb = (unsigned long long)__double_as_longlong(o_var);
          rstore(srs, sbase + 32 * own_col, rec_u4{gtag, (unsigned)mb, (unsigned)(mb >> 32), gtag});
          rstore(srs, sbase + 32 * own_col + 16, rec_u4{gtag, (unsigned)vb, (unsigned)(vb >> 32), gtag});
        } else {
          const unsigned long long db = (unsigned long long)__double_as_longlong(sqrt(o_var + nm.epsilon));
          rstore(srs, sbase + (2 * O + (own_ret ? 0 : 1)) * 16, rec_u4{gtag, (unsigned)db, (unsigned)(db >> 32), gtag});
        }
      }
    }
    if (prof) { const unsigned long long tn_ = prof_now(); pc2 += tn_ - tl; tl = tn_; }     // owner: gather + moments + publish
    // ---------------- phase B2: everybody reads the statistics granules, then normalises its envs ----------------
    {
      const int sbase = par * (GS / 2) * 16;
      const int total = has_cost ? GS / 2 : GS / 2 - 1;              // records: (mean, var) per column, ret denominator, cost denominator
      for (int i0 = 0; i0 < total; i0 += 256) {
        const int i = i0 + tid;
        rec_u4 gv = rec_u4{gtag, 0u, 0u, gtag};
        bool ok = i >= total;
        for (int spins = 0; spins < spin_limit && !ok; ++spins) {
          gv = rload(srs, sbase + i * 16);
          ok = gv[0] == gtag && gv[3] == gtag;
          if (!ok) __builtin_amdgcn_s_sleep(1);
        }
        if (!ok) spin_limit = 1;
        if (i < total) {
          const double v = __longlong_as_double((long long)(((unsigned long long)gv[2] << 32) | (unsigned long long)gv[1]));
          if (i < 2 * O) { if (i & 1) sh.var[i >> 1] = v; else sh.mean[i >> 1] = v; }
          else sh.dens[i - 2 * O] = v;
        }
      }
    }
    __syncthreads();
    if (prof) { const unsigned long long tn_ = prof_now(); pc3 += tn_ - tl; tl = tn_; }     // statistics granules arrived (+ barrier)
    for (int idx = tid; idx < Eg * O; idx += 256) {      // (env, component) pairs spread over all threads: one float64 sqrt + division each
      const int e = idx / O, i = idx - e * O;
      {
        const size_t tn = (size_t)t * N + g + e * G;
        const double raw = sh.s_new[e][i];
        double o = raw;
        if (nm.norm_obs) o = fmin(fmax((o - sh.mean[i]) / sqrt(sh.var[i] + nm.epsilon), -nm.clip_obs), nm.clip_obs);
        sh.olast[e][i] = o;
        sh.x[e][i] = (float)o;
        buf.new_observations[tn * O + i] = (float)o;
        sh.s_old[e][i] = raw;
      }
    }
    if (tid < Eg) {
      const int e = tid;
      const size_t tn = (size_t)t * N + g + e * G;
      double r = sh.rew[e];
      if (nm.norm_reward) r = fmin(fmax(r / sh.dens[0], -nm.clip_reward), nm.clip_reward);
      buf.rewards[tn] = (float)r;
      if (has_cost) {
        double c = (double)sh.cost[e];
        if (nm.norm_cost) c = fmin(fmax(c / sh.dens[1], -nm.clip_cost), nm.clip_cost);
        buf.costs[tn] = (float)c;
      }
      sh.last_done[e] = sh.done[e];
      if (MON) raw_plane[tn] = sh.rew[e];
    }
    if (pf) sh.noise[par ^ 1][pe][pk] = noise_next;
    __syncthreads();
    if (prof) { const unsigned long long tn_ = prof_now(); pc4 += tn_ - tl; tl = tn_; }     // normalise + rows
  }
  if (prof && (tid == 0 || tid == 192)) {      // wave 0: a policy / env wave's view; wave 3: the cost wave's
    unsigned long long* o = g_rollout_prof_wide + (tid == 192 ? 8 : 0);
    o[0] = pc0; o[1] = pc1; o[2] = pc2; o[3] = pc3; o[4] = pc4; o[5] = (unsigned long long)T; o[6] = pcA; o[7] = pcB;
  }
  if (spin_limit == 1 && ag.status != nullptr && (tid & 63) == 0) atomicOr(ag.status, 1);
  // ---- leave the agent / wrapper / normaliser state exactly where the per-step path leaves it
  for (int idx = tid; idx < Eg * MULTI_OP; idx += 256) {
    const int e = idx / MULTI_OP, i = idx % MULTI_OP;
    if (i < O) ag.last_obs[(size_t)(g + e * G) * O + i] = sh.olast[e][i];
  }
  if (tid < Eg) {
    const int e = tid, n = g + e * G;
    ag.last_dones[n] = (uint8_t)sh.last_done[e];
    ag.raw_rew[n] = sh.rew[e]; ag.dones[n] = (uint8_t)sh.done[e];
    if (has_cost) ag.raw_cost[n] = sh.cost[e];
  }
  if (lane == 0) {
    if (own_col >= 0) { nm.obs_mean[own_col] = o_mean; nm.obs_var[own_col] = o_var; if (own_col == 0) nm.obs_count[0] = o_cnt; }
    if (own_ret) { nm.ret_stats[0] = o_mean; nm.ret_stats[1] = o_var; nm.ret_stats[2] = o_cnt; }
    if (own_cost) { nm.cost_stats[0] = o_mean; nm.cost_stats[1] = o_var; nm.cost_stats[2] = o_cnt; }
  }
}

template <int OCT, int CIT, int E, bool MON = false>
__global__ void __launch_bounds__(256) rollout_multi_kernel(WideArgs p, int packed) {
  if (packed && (blockIdx.x & 7)) return;      // the G <= 32 workgroups on one XCD: workgroups 0, 8, 16, ... (ppo_common.h, "XCD placement")
  rollout_multi_body<OCT, CIT, E, MON>(p, packed ? (int)(blockIdx.x >> 3) : (int)blockIdx.x);
}

// several independent runs in ONE launch: grid (G, n_runs), run = blockIdx.y
// the analytic-cost form (CIT == 0: no cost tiles) as a kernel of its own name, single-run launches only.  The name sorts behind
// every other kernel that calls env_step_wave3: the compiler numbers those kernels in name order and passes the number to the callee
// (s15), so an instantiation of rollout_multi_kernel itself would renumber — and thereby change one immediate in — the shipped ones
template <int OCT, int E, bool MON = false>
__global__ void __launch_bounds__(256) rollout_multi_analytic_kernel(WideArgs p, int packed) {
  if (packed && (blockIdx.x & 7) != 0) return;
  rollout_multi_body<OCT, 0, E, MON>(p, packed ? (int)(blockIdx.x >> 3) : (int)blockIdx.x);
}

template <int OCT, int CIT, int E, bool MON = false>
__global__ void __launch_bounds__(256) rollout_multi_batch_kernel(const WideArgs* __restrict__ runs, int n_runs, int G, int packed) {
  __shared__ WideArgs p;
  int run = (int)blockIdx.y, g = (int)blockIdx.x;
  if (packed) {      // the G workgroups of a run on one XCD: workgroups b, b + 8, ... (ppo_common.h, "XCD placement")
    const int id = (int)blockIdx.x, per = 8 * G;
    run = (id / per) * 8 + (id & 7);
    g = (id % per) >> 3;
    if (run >= n_runs) return;
  }
  {
    const unsigned* src = reinterpret_cast<const unsigned*>(runs + run);
    unsigned* dst = reinterpret_cast<unsigned*>(&p);
    for (unsigned i = threadIdx.x; i < sizeof(WideArgs) / 4; i += 256) dst[i] = src[i];
  }
  __syncthreads();
  rollout_multi_body<OCT, CIT, E, MON>(p, g);
}

// rollout_multi_batch_kernel with an analytic cost per run (CIT == 0), under a name that sorts behind rollout_multi_analytic_kernel's
// for the reason given there: the instantiations that existed before keep their numbers, hence their device code
template <int OCT, int E, bool MON = false>
__global__ void __launch_bounds__(256) rollout_multi_batch_analytic_kernel(const WideArgs* __restrict__ runs, int n_runs, int G, int packed) {
  __shared__ WideArgs p;
  int run = (int)blockIdx.y, g = (int)blockIdx.x;
  if (packed) {      // the G workgroups of a run on one XCD: workgroups b, b + 8, ... (rollout_multi_batch_kernel)
    const int id = (int)blockIdx.x, per = 8 * G;
    run = (id / per) * 8 + (id & 7);
    g = (id % per) >> 3;
    if (run >= n_runs) return;
  }
  {
    const unsigned* src = reinterpret_cast<const unsigned*>(runs + run);
    unsigned* dst = reinterpret_cast<unsigned*>(&p);
    for (unsigned i = threadIdx.x; i < sizeof(WideArgs) / 4; i += 256) dst[i] = src[i];
  }
  __syncthreads();
  rollout_multi_body<OCT, 0, E, MON>(p, g);
}

// the discriminator-cost form (DISC) of rollout_multi_kernel, single runs.  It calls the env_step_wave3 instantiations the kernels above
// call, so its name sorts behind all of theirs (mangled: by length first) for the reason given at rollout_multi_analytic_kernel
template <int OCT, int CIT, int E, bool MON = false>
__global__ void __launch_bounds__(256) rollout_multi_net_as_discriminator_kernel(WideArgs p, int packed) {
  if (packed && (blockIdx.x & 7) != 0) return;
  rollout_multi_body<OCT, CIT, E, MON, true>(p, packed ? (int)(blockIdx.x >> 3) : (int)blockIdx.x);
}

// the region-cost form (REGION) of rollout_multi_analytic_kernel, single runs: one lane per env walks the clause table.  It calls the
// env_step_wave3<E, 0> instantiations, so its name sorts behind rollout_multi_net_as_discriminator_kernel's (mangled: by length first)
// for the reason given at rollout_multi_analytic_kernel
template <int OCT, int E, bool MON = false>
__global__ void __launch_bounds__(256) rollout_multi_with_a_region_cost_wave_kernel(WideArgs p, int packed) {
  if (packed && (blockIdx.x & 7) != 0) return;
  rollout_multi_body<OCT, 0, E, MON, false, true>(p, packed ? (int)(blockIdx.x >> 3) : (int)blockIdx.x);
}

// VecNormalizeWithCost.reset (vec_normalize.py:148-157, 270-278)
__global__ void __launch_bounds__(1024) norm_reset_kernel(icrl_norm_t nm, const double* raw_obs, int N, int O,
                                                          double* obs_out) {
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int n = tid; n < N; n += nt) { nm.ret[n] = 0.0; nm.cost_ret[n] = 0.0; }
  __syncthreads();
  if (nm.training && tid == 0) {
    // ret = ret * gamma + ret = 0 -> update with a zero batch: mean 0, var 0, count N
    double m = nm.ret_stats[0], v = nm.ret_stats[1];
    chan_merge(m, v, nm.ret_stats[2], 0.0, 0.0, (double)N);
    nm.ret_stats[0] = m; nm.ret_stats[1] = v; nm.ret_stats[2] = (double)N + nm.ret_stats[2];
    m = nm.cost_stats[0]; v = nm.cost_stats[1];
    chan_merge(m, v, nm.cost_stats[2], 0.0, 0.0, (double)N);
    nm.cost_stats[0] = m; nm.cost_stats[1] = v; nm.cost_stats[2] = (double)N + nm.cost_stats[2];
  }
  for (int idx = tid; idx < N * O; idx += nt) {
    const int j = idx % O;
    double o = raw_obs[idx];
    if (nm.norm_obs) o = fmin(fmax((o - nm.obs_mean[j]) / sqrt(nm.obs_var[j] + nm.epsilon), -nm.clip_obs), nm.clip_obs);
    obs_out[idx] = o;
  }
}

// =================================================================================================================
// fine-grained kernels behind the per-call C ABI
// =================================================================================================================
template <int OCT>
__global__ void __launch_bounds__(192) policy_forward_kernel(PolLayout pl, const float* PT, const double* obs,
                                                             const float* noise, int deterministic, const float* alow,
                                                             const float* ahigh, float* actions, float* act_clipped,
                                                             float* v_r, float* v_c, float* log_prob,
                                                             const float* given, float* entropy) {
  __shared__ ActShared sh;
  PolRegs<OCT> R;
  load_pol_regs<OCT>(pl, PT, R);
  const int n = blockIdx.x, tid = threadIdx.x;
  for (int i = tid; i < MAX_OBS; i += 192) sh.x[i] = i < pl.O ? (float)obs[(size_t)n * pl.O + i] : 0.f;
  __syncthreads();
  const float* noise_row = noise ? noise + (size_t)n * (pl.discrete ? 1 : pl.A) : nullptr;
  const int AS = pl.discrete ? 1 : pl.A;
  policy_forward_block<OCT>(pl, R, sh, noise_row, deterministic || noise == nullptr, alow, ahigh,
                            given ? given + (size_t)n * AS : nullptr);
  __syncthreads();
  if (tid < AS) {
    if (actions) actions[(size_t)n * AS + tid] = sh.act_raw[tid];
    if (act_clipped) act_clipped[(size_t)n * AS + tid] = sh.act_clip[tid];
  }
  if (tid == 0) {
    if (v_r) v_r[n] = sh.scal[0];
    if (v_c) v_c[n] = sh.scal[1];
    if (log_prob) log_prob[n] = sh.scal[2];
    if (entropy) entropy[n] = sh.scal[3];
  }
}

// policy_forward_kernel with the gSDE head (policies.py use_sde; distributions.py:525-587): the three branch forwards ARE
// policy_forward_block's (deterministic: act_raw = mean, g[0] = the policy branch's last tanh layer = latent_sde), so mean, v_r and v_c carry
// icrl_policy_forward's bits for the same network weights.  Behind it lane a < A of wave 0 takes, over the latent units in ascending order,
//   noise_a = sum_h latent_h E[h][a]        (E: this row's exploration matrix [MAX_H][A], or the one matrix when expl_stride == 0)
//   var_a   = sum_h latent_h^2 exp(2 log_std[h][a]) + 1e-6
// in float64 on the float32 latent (rounded once), action = mean + noise, log_prob = sum_a Normal(mean_a, sqrt(var_a)).log_prob(action_a).
// PT: the transposes of the NETWORK (pl: the diagonal layout, whose log_std slot is the matrix's last row); ls: the matrix in `params`.
template <int OCT>
__global__ void __launch_bounds__(192) policy_forward_sde_kernel(PolLayout pl, const float* PT, const float* __restrict__ ls, const double* obs,
                                                                 const float* __restrict__ expl, long long expl_stride, int deterministic,
                                                                 const float* alow, const float* ahigh, float* actions, float* act_clipped,
                                                                 float* v_r, float* v_c, float* log_prob) {
  __shared__ ActShared sh;
  PolRegs<OCT> R;
  load_pol_regs<OCT>(pl, PT, R);
  const int n = blockIdx.x, tid = threadIdx.x, A = pl.A;
  for (int i = tid; i < MAX_OBS; i += 192) sh.x[i] = i < pl.O ? (float)obs[(size_t)n * pl.O + i] : 0.f;
  __syncthreads();
  policy_forward_block<OCT>(pl, R, sh, nullptr, 1, nullptr, nullptr);
  __syncthreads();
  if (tid < WAVE) {      // wave 0
    double lp = 0.;
    float act = 0.f, clip = 0.f;
    if (tid < A) {
      const float mean = sh.act_raw[tid];
      const float* E = (deterministic || expl == nullptr) ? nullptr : expl + (size_t)n * (size_t)expl_stride;
      double noise = 0., var = 0.;
      for (int h = 0; h < pl.H2; ++h) {
        const double l = sh.g[0][h];
        if (E != nullptr) noise = fma(l, (double)E[h * A + tid], noise);
        var = fma(l * l, exp(2. * (double)ls[h * A + tid]), var);
      }
      var += 1e-6;
      act = E != nullptr ? (float)((double)mean + noise) : mean;
      const double diff = (double)act - (double)mean;
      lp = -(diff * diff) / (2. * var) - 0.5 * log(var) - 0.918938533204672741780329736406;
      clip = act;
      if (alow != nullptr && ahigh != nullptr) clip = fminf(fmaxf(act, alow[tid]), ahigh[tid]);
      if (actions) actions[(size_t)n * A + tid] = act;
      if (act_clipped) act_clipped[(size_t)n * A + tid] = clip;
    }
    double tot = 0.;      // in action order, every lane the same chain
    for (int a = 0; a < A; ++a) tot += __shfl(lp, a, 64);
    if (tid == 0) {
      if (v_r) v_r[n] = sh.scal[0];
      if (v_c) v_c[n] = sh.scal[1];
      if (log_prob) log_prob[n] = (float)tot;
    }
  }
}

// The same forward for MANY rows (policy.evaluate_actions over the nominal / expert samples of the KL metrics, forward over a batch):
// 16 rows per workgroup pass as fp32 MFMA tiles, exactly as rollout_multi_kernel evaluates 16 environments — every (unit, row) gets the
// value of policy_forward_block's fmaf chain (TileRegs), the heads and the log-probability / entropy sums are taken in
// wave_sum_fast's association.  Continuous actions only.  Waves: pi | vf | cvf; a workgroup walks tiles blockIdx.x, + gridDim.x, ...
template <int OCT>
__global__ void __launch_bounds__(192) policy_rows_kernel(PolLayout pl, const float* __restrict__ PT, const double* __restrict__ obs,
                                                          const float* __restrict__ noise, int deterministic, const float* __restrict__ alow,
                                                          const float* __restrict__ ahigh, float* actions, float* act_clipped, float* v_r,
                                                          float* v_c, float* log_prob, const float* __restrict__ given, float* entropy, int N) {
  constexpr int XS = 16 * OCT + 4;                       // row strides of 4 mod 32 floats: conflict-free B-operand reads
  __shared__ __attribute__((aligned(16))) float x[16][XS];
  __shared__ __attribute__((aligned(16))) float hbuf[3][16][MULTI_HS];
  __shared__ __attribute__((aligned(16))) float cst[3][MULTI_CST];
  TileRegs<OCT, 1> R;
  load_pol_tiles<OCT, 1>(pl, PT, R, cst[threadIdx.x >> 6]);
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, q4 = lane >> 4;
  const int O = pl.O, A = pl.A, H1 = pl.H1, H2 = pl.H2;
  const int nk1 = (O + 3) / 4;
  const bool has_box = alow != nullptr && ahigh != nullptr;
  const bool sample = given == nullptr && !deterministic && noise != nullptr;
  for (int i = tid; i < 16 * XS; i += 192) (&x[0][0])[i] = 0.f;          // pad columns stay zero
  const int n_tiles = (N + 15) / 16;
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int n0 = 16 * tile;
    const int rows = N - n0 < 16 ? N - n0 : 16;
    __syncthreads();                                      // the previous tile's x is consumed (first pass: the zero fill, cst)
    for (int i = tid; i < rows * O; i += 192) { const int rr = i / O, k = i - rr * O; x[rr][k] = (float)obs[(size_t)(n0 + rr) * O + k]; }
    __syncthreads();
    const int er = r16 < rows ? r16 : rows - 1;           // rows beyond the tile replicate its last row (their results are not stored)
    f32x4 z[4], cb[4];
    float bop[16];
    const float* const cw = &cst[w][4 * q4];
#pragma unroll
    for (int t = 0; t < 4; ++t) { z[t] = f32x4{0.f, 0.f, 0.f, 0.f}; cb[t] = *reinterpret_cast<const f32x4*>(cw + CST_B1 + 16 * t); }
    {
      const float* xb = &x[er][q4];
      float bx[4 * OCT];
#pragma unroll
      for (int ks = 0; ks < 4 * OCT; ++ks) bx[ks] = xb[4 * ks];
#pragma unroll
      for (int ks = 0; ks < 4 * OCT; ++ks) {
        if (ks < nk1) {
#pragma unroll
          for (int t = 0; t < 4; ++t) z[t] = MFMA16(R.w1[t][ks], bx[ks], z[t]);
        }
      }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) z[t][i] = 16 * t + 4 * q4 + i < H1 ? fast_tanh(z[t][i] + cb[t][i]) : 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) *reinterpret_cast<f32x4*>(&hbuf[w][r16][16 * t + 4 * q4]) = z[t];
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xC07F);
    {
      const float* hb = &hbuf[w][r16][q4];
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) bop[ks] = hb[4 * ks];
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) { z[t] = f32x4{0.f, 0.f, 0.f, 0.f}; cb[t] = *reinterpret_cast<const f32x4*>(cw + CST_B2 + 16 * t); }
#pragma unroll
    for (int ks = 0; ks < 16; ++ks)
#pragma unroll
      for (int t = 0; t < 4; ++t) z[t] = MFMA16(R.w2[t][ks], bop[ks], z[t]);
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) z[t][i] = 16 * t + 4 * q4 + i < H2 ? fast_tanh(z[t][i] + cb[t][i]) : 0.f;
    const int n = n0 + r16;
    const bool live = r16 < rows;
    if (w == 0) {
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int t = 0; t < 4; ++t) *reinterpret_cast<f32x4*>(&hbuf[0][r16][16 * t + 4 * q4]) = z[t];
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_s_waitcnt(0xC07F);
      {
        const float* hb = &hbuf[0][r16][q4];
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) bop[ks] = hb[4 * ks];
      }
      f32x4 m = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) m = MFMA16(R.wh[ks], bop[ks], m);
      const f32x4 hb_ = *reinterpret_cast<const f32x4*>(cw + CST_BA), sd_ = *reinterpret_cast<const f32x4*>(cw + CST_SD);
      const f32x4 lsd_ = *reinterpret_cast<const f32x4*>(cw + CST_LSD), i2v_ = *reinterpret_cast<const f32x4*>(cw + CST_I2V);
      float u[4], ue[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int ai = 4 * q4 + i;
        const float mean = m[i] + hb_[i];
        float lp = 0.f, entl = 0.f;
        if (ai < A) {
          const size_t at = (size_t)(live ? n : n0) * A + ai;
          float act = mean;
          if (given != nullptr) act = given[at];
          else if (sample) act = mean + noise[at] * sd_[i];             // Normal.rsample: loc + eps * scale
          const float diff = act - mean;
          lp = -(diff * diff) / i2v_[i] - lsd_[i] - LOG_SQRT_2PI_F;
          entl = HALF_LOG_2PI_PLUS_HALF_F + lsd_[i];
          if (live) {
            if (actions) actions[at] = act;
            if (act_clipped) act_clipped[at] = has_box ? fminf(fmaxf(act, alow[ai]), ahigh[ai]) : act;
          }
        }
        u[i] = (lp + 0.f) + (0.f + 0.f);                 // wave_sum_fast over lane = action: lanes 16.. hold 0
        ue[i] = (entl + 0.f) + (0.f + 0.f);
      }
      const float lp_row = xor32_sum(xor16_sum((u[0] + u[1]) + (u[2] + u[3])));
      const float ent_row = xor32_sum(xor16_sum((ue[0] + ue[1]) + (ue[2] + ue[3])));
      if (live && q4 == 0) {
        if (log_prob) log_prob[n] = lp_row;
        if (entropy) entropy[n] = ent_row;
      }
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const f32x4 wo = *reinterpret_cast<const f32x4*>(cw + CST_WO + 16 * t);
#pragma unroll
        for (int i = 0; i < 4; ++i) z[t][i] = 16 * t + 4 * q4 + i < H2 ? wo[i] * z[t][i] : 0.f;
      }
      const float v = tile_sum64(z) + cst[w][CST_BO];
      float* const dst = w == 1 ? v_r : v_c;
      if (live && q4 == 0 && dst) dst[n] = v;
    }
  }
}

template <int CIT>
__global__ void __launch_bounds__(64) cost_forward_kernel(icrl_costnet_t cn, CnLayout cl, const double* obs,
                                                          const float* acs, int N, float* cost, int mode = 0) {
  __shared__ __attribute__((aligned(16))) float cx[MAX_CN_IN];
  __shared__ __attribute__((aligned(16))) float ch[2][MAX_H];
  CnRegs<CIT> C;
  load_cn_regs<CIT>(cn, cl, C);
  const int n = blockIdx.x;
  const int AS = cn.is_discrete ? 1 : cn.acs_dim;
  const float c = cost_forward_wave<CIT>(cn, cl, C, obs + (size_t)n * cn.obs_dim, acs + (size_t)n * AS, cx, ch, mode);
  if (threadIdx.x == 0) cost[n] = c;
}

// ---- the rollout-end work of the GAIL callback around the discriminator step (icrl_gail_unnormalize_batch / icrl_gail_relabel_batch):
// run = blockIdx.y, argument blocks in device memory, grids sized for the largest run
struct GailArgs {
  icrl_costnet_t cn;            // the discriminator
  CnLayout cl;
  icrl_cost_fn_t f;             // the ground-truth cost (has_cost)
  const float* obs;             // [rows, obs_dim] normalised float32
  const float* acs;             // [rows, AS]
  const double *mean, *var;     // or NULL
  double eps;
  double* raw;                  // [rows, obs_dim]
  float* rewards;               // [rows]
  double* cost_mean;            // [1]
  int rows, obs_dim, has_cost, learn_cost;
};

// raw = float64(obs) * sqrt(var + eps) + mean: the product and the sum are rounded separately (torch issues a mul and an add)
__global__ void __launch_bounds__(256) gail_unnormalize_kernel(const GailArgs* __restrict__ runs) {
  const GailArgs& a = runs[blockIdx.y];
  const long long total = (long long)a.rows * a.obs_dim;
  const double *mean = a.mean, *var = a.var;
  const double eps = a.eps;
  const float* obs = a.obs;
  double* raw = a.raw;
  const int O = a.obs_dim;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    double v = (double)obs[i];
    if (mean != nullptr) {
      const int k = (int)(i % O);
      v = __dadd_rn(__dmul_rn(v, sqrt(__dadd_rn(var[k], eps))), mean[k]);
    }
    raw[i] = v;
  }
}

// cost_mean = mean of the ground-truth cost over the run's rows: one workgroup per run; the costs are 0, 1 or 2, so they are counted in
// integers (any order is exact).  The mean is count * (1.0 / rows), two roundings: that is how torch's device reduction finishes a mean
// (sum times the reciprocal of the row count), so the bits are those of c.double().mean() on the device; count / rows can differ from it
// in the last place (89 of 132 rows does).  Runs after gail_unnormalize_kernel.
__global__ void __launch_bounds__(1024) gail_cost_mean_kernel(const GailArgs* __restrict__ runs) {
  __shared__ long long part[16];
  const GailArgs& a = runs[blockIdx.y];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  long long cnt = 0;
  if (a.has_cost) {
    const icrl_cost_fn_t f = a.f;
    const int AS = f.kind == ICRL_COST_ACTION_EQUALS ? 1 : f.acs_dim;
    for (int n = tid; n < a.rows; n += 1024) cnt += (long long)cost_fn_wave(f, a.raw + (size_t)n * a.obs_dim, a.acs + (size_t)n * AS);
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) cnt += __shfl_xor(cnt, m, 64);
  if (lane == 0) part[wv] = cnt;
  __syncthreads();
  if (tid == 0) {
    long long t = 0;
    for (int w = 0; w < 16; ++w) t += part[w];
    a.cost_mean[0] = a.has_cost ? __dmul_rn((double)t, 1.0 / (double)a.rows) : 0.0;
  }
}

// rewards (+)= log(D(raw, acs) + eps): cost_forward_kernel's row forward in mode 2, one wave per row — the bits of icrl_disc_reward
template <int CIT>
__global__ void __launch_bounds__(64) gail_relabel_kernel(const GailArgs* __restrict__ runs) {
  __shared__ __attribute__((aligned(16))) float cx[MAX_CN_IN];
  __shared__ __attribute__((aligned(16))) float ch[2][MAX_H];
  const int n = blockIdx.x;
  if (n >= runs[blockIdx.y].rows) return;
  GailArgs a = runs[blockIdx.y];
  globalize(a.cn);
  CnRegs<CIT> C;
  load_cn_regs<CIT>(a.cn, a.cl, C);
  const int AS = a.cn.is_discrete ? 1 : a.cn.acs_dim;
  const float r = cost_forward_wave<CIT>(a.cn, a.cl, C, a.raw + (size_t)n * a.cn.obs_dim, a.acs + (size_t)n * AS, cx, ch, 2);
  if (threadIdx.x == 0) a.rewards[n] = a.learn_cost ? a.rewards[n] + r : r;
}

// an analytic cost on N rows of the caller's arrays (icrl_cost_fn_rows): one row per thread, grid-stride, no LDS
__global__ void __launch_bounds__(256) cost_fn_rows_kernel(icrl_cost_fn_t f, const double* __restrict__ obs, const float* __restrict__ acs, int N,
                                                           float* __restrict__ cost) {
  const int AS = f.kind == ICRL_COST_ACTION_EQUALS ? 1 : f.acs_dim;      // (the class index when discrete)
  for (int n = blockIdx.x * blockDim.x + threadIdx.x; n < N; n += gridDim.x * blockDim.x)
    cost[n] = cost_fn_wave(f, obs + (size_t)n * f.obs_dim, acs + (size_t)n * AS);
}

// a region cost on N rows of the caller's arrays (icrl_cost_region_rows): the clause table into LDS, then one row per thread, grid-stride
__global__ void __launch_bounds__(256) cost_region_rows_kernel(icrl_cost_region_t r, const double* __restrict__ obs, const float* __restrict__ acs, int N,
                                                               float* __restrict__ cost) {
  __shared__ icrl_region_clause_t tab[ICRL_REGION_MAX_CLAUSES];
  region_table_load(tab, r, (int)threadIdx.x, 256);
  __syncthreads();
  for (int n = blockIdx.x * 256 + threadIdx.x; n < N; n += gridDim.x * 256)
    cost[n] = cost_region_row(tab, r.n_clauses, r.combine, obs + (size_t)n * r.obs_dim, acs + (size_t)n * r.acs_dim, r.obs_dim);
}

__global__ void __launch_bounds__(64) env_step_kernel(icrl_env_t e, const float* actions, double* raw_rew, uint8_t* dones) {
  __shared__ double s_old[MAX_OBS];
  const int n = blockIdx.x;
  for (int i = threadIdx.x; i < e.obs_dim; i += WAVE) s_old[i] = e.s[(size_t)n * e.obs_dim + i];
  __syncthreads();
  double rew; int done;
  uint32_t ctr = e.step_count[n];
  int tep = e.t_ep[n];
  env_step_wave(e, n, s_old, actions + (size_t)n * e.act_dim, e.key[n], ctr, tep, nullptr, rew, done);
  if (threadIdx.x == 0) { raw_rew[n] = rew; dones[n] = (uint8_t)done; }
}

__global__ void env_reset_kernel(icrl_env_t e) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const int O = e.obs_dim;
  if (idx < e.n_envs * O) {
    const int n = idx / O, i = idx % O;
    e.s[idx] = env_reset_value(e, e.key[n], e.step_count[n], i);
    if (i == 0) e.t_ep[n] = 0;
  }
}

// =================================================================================================================
// persistent single-env episode sampler: sample_from_agent / evaluate_policy (icrl/utils.py:323-357, evaluation.py:10-67)
// One workgroup per independent env stream runs its episodes start to finish inside ONE launch: frozen-statistics
// normalise -> policy forward (sample or mode) -> clip -> env step (+auto-reset) -> record (s_{t+1}, a_t), reward.
// =================================================================================================================
struct SampleArgs {
  icrl_env_t env;          // arrays sized [n_streams]; env.s etc. are this call's scratch state
  icrl_norm_t nm;          // training must be 0: statistics are only read
  PolLayout pl;
  const float* PT;
  int pt_in_lds;
  const float* noise;      // [n_streams][rows_per_stream][act] or NULL (deterministic)
  const float* alow;
  const float* ahigh;
  int episodes_per_stream, rows_per_stream, deterministic, do_reset;
  const int* stream_row0;  // [n_streams] first row (noise in, outputs out) of every stream, or NULL: stream * rows_per_stream
  int total_rows;          // rows of the noise / output arrays (only read with stream_row0)
  double* orig_obs;        // [n_streams*rows_per_stream, obs] raw observation AFTER each step
  double* obs;             // same, normalised
  float* actions;          // [.., act_store] clipped action that produced it
  double* ep_rewards;      // [n_streams*episodes_per_stream]
  int* ep_lengths;         // [n_streams*episodes_per_stream]
};

// The chained form (CHAIN, icrl_sample_episodes_chain): stream k IS episode k of the sequential 1-env loop, and the position it starts
// from is settled inside the launch.  pos_k (first the guess k * max_steps) fixes the env's random-stream counter base + pos_k, the
// action-noise row pos_k + i and the reset draw.  One word per stream, next_start[k] = {start row of episode k + 1 : 31 bits | final : 1},
// written and read with single agent-scope relaxed atomics; nothing is read behind it, so it needs no fence.  A stream publishes
// pos_k + max_steps when it (re)starts and pos_k + len_k when its episode ends, looks at its predecessor's word every step (the load is
// issued at the top of the step by an otherwise idle wave and consumed after the env step), and starts over from the start it finds
// there when that differs from pos_k.  It is validated once that word is final and equals pos_k; validated and finished, it writes its
// episode sum and length and publishes its own word with the final bit.  While it runs a stream writes rows only to a slot of its own
// (rows k * max_steps + i of the slot arrays), so that a late store of an abandoned run can never land on validated rows; once final it
// copies its len_k rows to [pos_k, pos_k + len_k) of the outputs, which are disjoint between streams.  A fixed_len job's guesses are
// exact: it neither polls nor copies (its slot arrays are the outputs).  
struct ChainArgs {
  SampleArgs s;            // outputs: the arrays of the sequential loop; env: per-stream scratch state [n_streams]
  unsigned* next_start;    // [n_streams] position words, CHAIN_UNSET before the launch
  unsigned* status;        // [1] set to 1 when a bounded wait ran out
  int* exec_steps;         // [n_streams] env steps the stream executed, abandoned runs included (or NULL)
  double* slot_orig;       // [n_streams * max_steps, obs] private rows (the outputs themselves when fixed_len)
  double* slot_obs;
  float* slot_act;
  const int* base_count;   // [1] the env's random-stream counter before episode 0
  int fixed_len, n_streams;
};
constexpr unsigned CHAIN_UNSET = 0xFFFFFFFEu;      // "nothing published yet": no start ever reaches 2^31 - 1 rows

// SDE (icrl_sample_episodes_sde / _chain_sde): a gSDE policy, a compile-time form like MON, DISC and SDE of rollout_persistent_body: the
// instantiations without it keep their code.  An episode loop never redraws: one env means get_noise picks E0, so ONE matrix `expl` [MAX_H][A]
// serves every step of every episode of the launch (NULL: the mode).  It is fetched once, in front of the step loop, into a float32 LDS image
// [MAX_H][A] (4 KB at A = 16; as 64 registers of wave 0 the <8> kernels reached 512 VGPRs and spilled: DESIGN.md section 26), and a restart
// of a chained stream does not refetch it; a.pl / a.PT describe the network alone (the diagonal layout, the
// transposes behind the matrix's first 63 rows, as icrl_rollout_collect_sde builds them) and a.noise is not read.  The sampler stores no
// log-prob, so the head is the action half of sde_head_wave alone, term for term: no variance chain, no log, no division, no exp.
template <int OCT, bool CHAIN = false, bool SDE = false>
__device__ __forceinline__ void sample_episodes_body(const SampleArgs& a, const ChainArgs* c = nullptr, const float* expl = nullptr) {
  __shared__ ActShared sh;
  PolRegs<OCT> R;
  load_pol_regs<OCT>(a.pl, a.PT, R);    // once for every step of every episode of this stream
  const float* E_s = nullptr;           // SDE: the LDS image of the exploration matrix, or NULL (the mode)
  if constexpr (SDE) {
    __shared__ float E_img[MAX_H * MAX_ACT];
    const float* const E_g = as_global(expl);
    if (E_g != nullptr) {               // (read behind the barriers in front of the first step, like the dynamics matrix below)
      for (int i = threadIdx.x; i < MAX_H * a.pl.A; i += 192) E_img[i] = E_g[i];
      E_s = E_img;
    }
  }
  __shared__ int s_done;
  __shared__ double s_rew;
  __shared__ unsigned s_word;                  // CHAIN: the predecessor's position word as this step saw it
  __shared__ double Bl[MAX_OBS * MAX_ACT];     // dynamics matrix: read every step, kept out of the global-memory latency
  __shared__ float noise_s[MAX_ACT], alow_s[MAX_ACT], ahigh_s[MAX_ACT];
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int O = a.pl.O, A = a.pl.A;
  const int AS = a.pl.discrete ? 1 : A;
  icrl_env_t env = a.env; globalize(env);
  // what the step loop reads of the argument block, once (a batched launch keeps the block in LDS; pointers: common.h as_global)
  const float* const noise_g = SDE ? nullptr : as_global(a.noise);
  float* const actions_g = as_global(CHAIN ? c->slot_act : a.actions);
  double* const orig_obs_g = as_global(CHAIN ? c->slot_orig : a.orig_obs);
  double* const obs_g = as_global(CHAIN ? c->slot_obs : a.obs);
  const int norm_obs = a.nm.norm_obs, deterministic = a.deterministic;
  const double clip_obs = a.nm.clip_obs;
  for (int i = tid; i < O * a.env.act_dim; i += 192) Bl[i] = a.env.B[i];
  env.B = Bl;
  const bool has_box = a.alow != nullptr && a.ahigh != nullptr;
  if (tid < MAX_ACT) { alow_s[tid] = (has_box && tid < A) ? a.alow[tid] : 0.f; ahigh_s[tid] = (has_box && tid < A) ? a.ahigh[tid] : 0.f; }
  const uint32_t e_key = a.env.key[n];
  uint32_t e_ctr = a.env.step_count[n];
  int e_tep = a.env.t_ep[n];
  // frozen normaliser statistics of this thread's observation components (i = tid, O <= 128 < 192)
  double n_mean = 0.0, n_den = 1.0;
  if (tid < O && a.nm.norm_obs) { n_mean = a.nm.obs_mean[tid]; n_den = sqrt(a.nm.obs_var[tid] + a.nm.epsilon); }
  for (int i = tid; i < MAX_OBS; i += 192) sh.x[i] = 0.f;
  // CHAIN: where this stream believes its episode starts, whether that is settled, and what it has executed so far
  const int max_steps = a.env.max_steps;
  unsigned* const words = CHAIN ? as_global(c->next_start) : nullptr;
  const uint32_t base = CHAIN ? (uint32_t)as_global(c->base_count)[0] : 0u;
  const size_t slot0 = CHAIN ? (size_t)n * max_steps : 0;
  unsigned pos = CHAIN ? (unsigned)n * (unsigned)max_steps : 0u;
  bool validated = !CHAIN || n == 0 || c->fixed_len != 0;
  int executed = 0;
  bool again;
  do {
  again = false;
  if (CHAIN) {
    __syncthreads();       // (a restart: every thread has left the step it abandoned)
    e_ctr = base + pos;    // wraps like the env's own counter
    if (n > 0 || a.do_reset) e_tep = 0;
    if (tid == 0 && !c->fixed_len) xstore(words + n, (pos + (unsigned)max_steps) << 1);
  }
  if (tid < O) {
    double v = a.env.s[(size_t)n * O + tid];
    if (a.do_reset || (CHAIN && n > 0)) v = env_reset_value<!CHAIN>(a.env, e_key, e_ctr, tid);
    sh.s_new[tid] = v;
  }
  if (!CHAIN && a.do_reset) e_tep = 0;
  __syncthreads();
  size_t row = CHAIN ? (size_t)pos : a.stream_row0 != nullptr ? (size_t)a.stream_row0[n] : (size_t)n * a.rows_per_stream;
  const size_t row_end = (CHAIN || a.stream_row0 != nullptr) ? (size_t)a.total_rows : row + a.rows_per_stream;
  float noise_reg = (noise_g != nullptr && tid < AS) ? noise_g[row * AS + tid] : 0.f;   // noise of the first step
  for (int ep = 0; ep < a.episodes_per_stream; ++ep) {
    double ep_rew = 0.0;
    int ep_len = 0;
    while (true) {
      unsigned word = CHAIN_UNSET;
      if (CHAIN && !validated && tid == 128) word = xload(words + n - 1);      // consumed after the env step
      if (tid < O) {
        const double raw = sh.s_new[tid];
        double o = raw;
        if (norm_obs) o = fmin(fmax((raw - n_mean) / n_den, -clip_obs), clip_obs);
        sh.s_old[tid] = raw;
        sh.x[tid] = (float)o;
      }
      if (noise_g != nullptr && tid < AS) {
        noise_s[tid] = noise_reg;
        if (row + 1 < row_end) noise_reg = noise_g[(row + 1) * AS + tid];      // next step's noise lands during this step
      }
      __syncthreads();
      if constexpr (SDE) {
        // the mean clipped to the box (the mode: what icrl_policy_forward_sde(deterministic = 1) returns), then, where the launch has a matrix, the
        // action half of sde_head_wave on wave 0, which rewrites its own act_raw / act_clip (the latent lies behind a barrier of the forward; LDS
        // accesses of one wave are ordered): the barrier below publishes them to the env step
        policy_forward_block<OCT>(a.pl, R, sh, nullptr, 1, has_box ? alow_s : nullptr, has_box ? ahigh_s : nullptr);
        if (w == 0 && E_s != nullptr && lane < A) {
          const float mean = sh.act_raw[lane];
          const int H2 = a.pl.H2;
          double noise = 0.;
#pragma unroll 8      // (one sequential chain in ascending h, as sde_head_wave's; unrolled, the operands of eight terms are fetched together)
          for (int h = 0; h < H2; ++h) noise = fma((double)sh.g[0][h], (double)E_s[h * A + lane], noise);
          const float act = (float)((double)mean + noise);
          float clip = act;
          if (has_box) clip = fminf(fmaxf(act, alow_s[lane]), ahigh_s[lane]);
          sh.act_raw[lane] = act;
          sh.act_clip[lane] = clip;
        }
      } else {
      policy_forward_block<OCT>(a.pl, R, sh, noise_g ? noise_s : nullptr, deterministic || noise_g == nullptr,
                                has_box ? alow_s : nullptr, has_box ? ahigh_s : nullptr);
      }
      __syncthreads();
      const bool in_rows = CHAIN || row < row_end;      // (a stream whose speculative start row was too late can run off the arrays)
      const size_t orow = CHAIN ? slot0 + (size_t)ep_len : row;
      if (w == 0) {
        double rew; int done;
        env_step_wave<!CHAIN>(env, n, sh.s_old, sh.act_clip, e_key, e_ctr, e_tep, sh.s_new, rew, done);
        if (lane == 0) { s_done = done; s_rew = rew; }
        if (lane < AS && in_rows) actions_g[orow * AS + lane] = sh.act_clip[lane];
      }
      if (CHAIN && tid == 128) s_word = word;
      __syncthreads();
      if (tid < O && in_rows) {
        const double raw = sh.s_new[tid];
        double o = raw;
        if (norm_obs) o = fmin(fmax((raw - n_mean) / n_den, -clip_obs), clip_obs);
        orig_obs_g[orow * O + tid] = raw;
        obs_g[orow * O + tid] = o;
      }
      ep_rew += s_rew;     // episode_reward += reward (un-normalised: norm_reward is False on sampling / eval envs)
      ++ep_len;
      ++row;
      const int done = s_done;
      if (CHAIN) {
        ++executed;
        const unsigned pw = s_word;
        if (!validated && pw != CHAIN_UNSET) {
          if ((pw >> 1) != pos) { pos = pw >> 1; again = true; }
          validated = (pw & 1u) != 0u;
        }
      }
      __syncthreads();
      if (CHAIN && again) break;
      if (done) break;
    }
    if (CHAIN) {
      if (again) break;
      // finished: tell the successor where it starts (provisional until this stream is validated), then wait for the predecessor's last word
      if (tid == 0 && !validated) xstore(words + n, (pos + (unsigned)ep_len) << 1);
      for (int spins = 0; !validated && !again; ++spins) {
        if (spins == (1 << 22)) {      // the predecessor never finished (its workgroup was not resident): report and leave
          if (tid == 0) { atomicOr(as_global(c->status), 1u); a.ep_lengths[n] = -1; }
          return;
        }
        if (tid == 0) s_word = xload(words + n - 1);
        __syncthreads();
        const unsigned pw = s_word;
        if (pw != CHAIN_UNSET) {
          if ((pw >> 1) != pos) { pos = pw >> 1; again = true; }
          validated = (pw & 1u) != 0u;
        }
        __syncthreads();
        if (!validated && !again) __builtin_amdgcn_s_sleep(32);
      }
      if (again) break;
      if (tid == 0) {
        a.ep_rewards[n] = ep_rew; a.ep_lengths[n] = ep_len;
        if (c->exec_steps != nullptr) c->exec_steps[n] = executed;
        if (!c->fixed_len) xstore(words + n, ((pos + (unsigned)ep_len) << 1) | 1u);
      }
      if (!c->fixed_len) {      // the validated rows, from the slot to their place in the sequential loop's arrays
        const size_t nd = (size_t)ep_len * O, na = (size_t)ep_len * AS;
        const double* so = orig_obs_g + slot0 * O; const double* sn = obs_g + slot0 * O; const float* sa = actions_g + slot0 * AS;
        double* dorig = as_global(a.orig_obs) + (size_t)pos * O; double* dobs = as_global(a.obs) + (size_t)pos * O;
        float* dact = as_global(a.actions) + (size_t)pos * AS;
#pragma unroll 4
        for (size_t i = tid; i < nd; i += 192) { dorig[i] = so[i]; dobs[i] = sn[i]; }
#pragma unroll 4
        for (size_t i = tid; i < na; i += 192) dact[i] = sa[i];
      }
    } else if (tid == 0) { a.ep_rewards[(size_t)n * a.episodes_per_stream + ep] = ep_rew; a.ep_lengths[(size_t)n * a.episodes_per_stream + ep] = ep_len; }
  }
  } while (CHAIN && again);
}

template <int OCT>
__global__ void __launch_bounds__(192) sample_episodes_kernel(SampleArgs a) {
  sample_episodes_body<OCT>(a);
}

// several runs' streams in ONE launch: grid (n_streams, n_runs), run = blockIdx.y (streams of different runs never interact)
template <int OCT>
__global__ void __launch_bounds__(192) sample_episodes_batch_kernel(const SampleArgs* __restrict__ runs) {
  __shared__ SampleArgs a;
  {
    const unsigned* src = reinterpret_cast<const unsigned*>(runs + blockIdx.y);
    unsigned* dst = reinterpret_cast<unsigned*>(&a);
    for (unsigned i = threadIdx.x; i < sizeof(SampleArgs) / 4; i += 192) dst[i] = src[i];
  }
  __syncthreads();
  sample_episodes_body<OCT>(a);
}

// the chained sampler: grid (max streams of a job, jobs); jobs may differ in env flags, statistics, policy and stream count
template <int OCT>
__global__ void __launch_bounds__(192) sample_episodes_chain_kernel(const ChainArgs* __restrict__ jobs) {
  __shared__ ChainArgs c;
  {
    const unsigned* src = reinterpret_cast<const unsigned*>(jobs + blockIdx.y);
    unsigned* dst = reinterpret_cast<unsigned*>(&c);
    for (unsigned i = threadIdx.x; i < sizeof(ChainArgs) / 4; i += 192) dst[i] = src[i];
  }
  __syncthreads();
  if ((int)blockIdx.x >= c.n_streams) return;
  sample_episodes_body<OCT, true>(c.s, &c);
}

// before the launch, on the same stream: the job's argument block, its position words unset, the status word cleared
__global__ void __launch_bounds__(64) chain_prep_kernel(ChainArgs v, ChainArgs* dst, int clear_status) {
  if (threadIdx.x == 0) { *dst = v; if (clear_status) *v.status = 0u; }
  for (int i = threadIdx.x; i < v.n_streams; i += 64) v.next_start[i] = CHAIN_UNSET;
}

// ---- the samplers of a gSDE policy (icrl_sample_episodes_sde, icrl_sample_episodes_chain_sde): the bodies above with SDE = true.  SampleArgs
// and ChainArgs keep their layout; the matrix pointer travels beside them — a second kernel argument here, per job behind the job's ChainArgs there.
template <int OCT>
__global__ void __launch_bounds__(192) sample_episodes_sde_kernel(SampleArgs a, const float* expl) {
  sample_episodes_body<OCT, false, true>(a, nullptr, expl);
}

struct ChainSdeArgs {
  ChainArgs c;
  const float* expl;       // [MAX_H][A] float32, or NULL: this job takes the mode
};

template <int OCT>
__global__ void __launch_bounds__(192) sample_episodes_chain_sde_kernel(const ChainSdeArgs* __restrict__ jobs) {
  __shared__ ChainSdeArgs c;
  {
    const unsigned* src = reinterpret_cast<const unsigned*>(jobs + blockIdx.y);
    unsigned* dst = reinterpret_cast<unsigned*>(&c);
    for (unsigned i = threadIdx.x; i < sizeof(ChainSdeArgs) / 4; i += 192) dst[i] = src[i];
  }
  __syncthreads();
  if ((int)blockIdx.x >= c.c.n_streams) return;
  sample_episodes_body<OCT, true, true>(c.c.s, &c.c, c.expl);
}

__global__ void __launch_bounds__(64) chain_prep_sde_kernel(ChainSdeArgs v, ChainSdeArgs* dst, int clear_status) {
  if (threadIdx.x == 0) { *dst = v; if (clear_status) *v.c.status = 0u; }
  for (int i = threadIdx.x; i < v.c.n_streams; i += 64) v.c.next_start[i] = CHAIN_UNSET;
}

// =================================================================================================================
// rollout over host envs (icrl_host_step): one launch per env step, one workgroup per env, no waiting between workgroups.
// Launch k finishes step k - 1 from the staging block (the statistics pass of rollout_persistent_body, replicated, reading the
// observation columns straight from the staging block in global memory) and then runs act_step_kernel's work for step k minus
// the env step.  What every workgroup reads and one workgroup writes — running statistics, the returns, the raw costs of the
// previous launch — lives in two copies selected by step parity (HostCopy).
// =================================================================================================================
struct HostStepArgs {
  ActStepArgs act;
  icrl_norm_t nm;
  icrl_host_step_t hs;
  int N;
};

// one copy of the state carried between launches, in doubles: obs mean [O] | obs var [O] | obs count | ret_stats [3] |
// cost_stats [3] | ret [N] | cost_ret [N] | raw cost [N]
__host__ __device__ inline size_t host_copy_doubles(int N, int O) { return (size_t)2 * O + 7 + (size_t)3 * N; }
struct HostCopy {
  double *mean, *var, *count, *ret_stats, *cost_stats, *ret, *cost_ret, *cost;
  __device__ HostCopy(double* base, int N, int O)
      : mean(base), var(base + O), count(base + 2 * O), ret_stats(base + 2 * O + 1), cost_stats(base + 2 * O + 4),
        ret(base + 2 * O + 7), cost_ret(base + 2 * O + 7 + N), cost(base + 2 * O + 7 + 2 * N) {}
};

template <int OCT, int CITF>      // CITF: CIT [| CIT_DISC] (act_step_kernel)
__global__ void __launch_bounds__(256) host_step_kernel(HostStepArgs h, int k) {
  constexpr int CIT = CITF & 0xff;                     // the cost-net image proper
  constexpr bool DISC = (CITF & CIT_DISC) != 0;        // the constraint net read as D = zeta (icrl_cost_disc_t)
  constexpr bool REGION = (CITF & CIT_REGION) != 0;    // a region cost (icrl_cost_region_t) on the CIT == 0 image
  REGION_TABLE(h.act, (int)threadIdx.x, 256)           // (published by the barriers in front of the act phase)
  __shared__ ActShared sh;
  __shared__ double vec[2][128], dev2[2][128], ret_s[128], cret_s[128], rawr_s[128];
  __shared__ float rawc_s[128];
  __shared__ double dens[2];
  __shared__ int done_s[128];
  __shared__ int last_done_s;
  const ActStepArgs& a = h.act;
  const icrl_norm_t& nm = h.nm;
  WaveRegs<OCT, CIT> R;                // one image: policy weights in waves 0..2, cost-net weights in wave 3
  WaveRegs<OCT, CIT>& C = R;
  const int T = h.hs.T;
  if (k < T) {
    load_pol_regs<OCT>(a.pl, a.PT, R);
    if constexpr (CIT > 0) { if (threadIdx.x >= 192 && a.has_cn) load_cn_regs<CIT>(a.cn, a.cl, C); }
  }
  const icrl_cost_fn_t cf = a.cf;      // analytic cost (CIT == 0): kind, index and thresholds are read once, before the step loop
  const int n = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int O = a.pl.O, A = a.pl.A, N = h.N;
  const int AS = a.buf.act_store;
  const bool has_cost = a.has_cn != 0;
  double* const ws = reinterpret_cast<double*>(h.hs.ws);
  const size_t CP = host_copy_doubles(N, O);
  const HostCopy src(ws + (size_t)((k + 1) & 1) * CP, N, O);      // written by launch k - 1
  const HostCopy dst(ws + (size_t)(k & 1) * CP, N, O);            // written here (workgroup 0), read by launch k + 1
  const double* const st_obs = reinterpret_cast<const double*>(h.hs.stage);
  const double* const st_rew = st_obs + (size_t)N * O;
  const uint8_t* const st_done = reinterpret_cast<const uint8_t*>(st_rew + N);
  if (k == 0) {
    // the rollout's first launch: the state as the previous rollout (or reset) left it
    for (int i = tid; i < MAX_OBS; i += 256) {
      sh.x[i] = i < O ? (float)a.ag.last_obs[(size_t)n * O + i] : 0.f;
      if (i < O) sh.s_old[i] = h.hs.s[(size_t)n * O + i];
    }
    if (tid == 0) last_done_s = a.ag.last_dones[n];
    if (n == 0) {        // launch 1 reads copy 0
      if (tid < O) { dst.mean[tid] = nm.obs_mean[tid]; dst.var[tid] = nm.obs_var[tid]; }
      if (tid == 0) dst.count[0] = nm.obs_count[0];
      if (tid < 3) { dst.ret_stats[tid] = nm.ret_stats[tid]; if (has_cost) dst.cost_stats[tid] = nm.cost_stats[tid]; }
      if (tid < N) { dst.ret[tid] = nm.ret[tid]; if (has_cost) dst.cost_ret[tid] = nm.cost_ret[tid]; }
    }
  } else {
    // ---------------- finish step k - 1 (rollout_persistent_body's phase B over the staging block) ----------------
    const size_t tn = (size_t)(k - 1) * N + n;
    double o_mean = 0.0, o_var = 1.0, o_cnt = 0.0;
    if (tid < O) { o_mean = src.mean[tid]; o_var = src.var[tid]; o_cnt = src.count[0]; }
    double st_m = 0.0, st_v = 1.0, st_c = 0.0;
    if (w == 3) { st_m = src.ret_stats[0]; st_v = src.ret_stats[1]; st_c = src.ret_stats[2]; }
    if (w == 2 && has_cost) { st_m = src.cost_stats[0]; st_v = src.cost_stats[1]; st_c = src.cost_stats[2]; }
    if (tid < N) {
      const double rr = st_rew[tid];
      const float rc = has_cost ? (float)src.cost[tid] : 0.f;
      const double r0 = src.ret[tid], c0 = has_cost ? src.cost_ret[tid] : 0.0;
      ret_s[tid] = r0; cret_s[tid] = c0;
      rawr_s[tid] = rr; rawc_s[tid] = rc; done_s[tid] = (int)st_done[tid];
      double r = r0, c = c0;
      if (nm.training) {
        r = r * nm.reward_gamma + rr;
        if (has_cost) c = c * nm.cost_gamma + (double)rc;
      }
      vec[0][tid] = r; vec[1][tid] = c;
    }
    __syncthreads();
    if (nm.training) {
      if (tid < O) {           // obs_rms.update: rows added in order (numpy's axis-0 reduction)
        double bm, bv;
        column_moments(st_obs + tid, O, N, bm, bv);
        chan_merge(o_mean, o_var, o_cnt, bm, bv, (double)N);
        o_cnt = (double)N + o_cnt;
      }
      if (w == 3 || (w == 2 && has_cost)) {     // ret_rms / cost_rms: numpy pairwise order
        const int v = w == 3 ? 0 : 1;
        const double bm = np_leaf_sum_wave(vec[v], N) / (double)N;
        for (int i = lane; i < N; i += 64) { const double d = vec[v][i] - bm; dev2[v][i] = d * d; }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_waitcnt(0xC07F);
        const double bv = np_leaf_sum_wave(dev2[v], N) / (double)N;
        chan_merge(st_m, st_v, st_c, bm, bv, (double)N);
        st_c = (double)N + st_c;
      }
    }
    if (lane == 0 && w == 3) dens[0] = sqrt(st_v + nm.epsilon);
    if (lane == 0 && w == 2) dens[1] = sqrt(st_v + nm.epsilon);
    if (tid >= O && tid < MAX_OBS) sh.x[tid] = 0.f;      // pad = 0 (the forward reads whole float4 rows against zero pad weights)
    if (tid < O) {             // own env: normalise + clip, next policy input
      const double raw = st_obs[(size_t)n * O + tid];
      double o = raw;
      if (nm.norm_obs) o = fmin(fmax((o - o_mean) / sqrt(o_var + nm.epsilon), -nm.clip_obs), nm.clip_obs);
      sh.x[tid] = (float)o;
      sh.s_old[tid] = raw;
      a.buf.new_observations[tn * O + tid] = (float)o;
      a.buf.new_orig_observations[tn * O + tid] = (float)raw;
      a.ag.last_obs[(size_t)n * O + tid] = o;
      h.hs.s[(size_t)n * O + tid] = raw;
    }
    __syncthreads();
    if (tid < N) {
      const int d = done_s[tid];
      if (nm.training || d) { ret_s[tid] = d ? 0.0 : vec[0][tid]; if (has_cost) cret_s[tid] = d ? 0.0 : vec[1][tid]; }
    }
    if (tid == 0) {
      double r = rawr_s[n];
      if (nm.norm_reward) r = fmin(fmax(r / dens[0], -nm.clip_reward), nm.clip_reward);
      a.buf.rewards[tn] = (float)r;
      if (has_cost) {
        double c = (double)rawc_s[n];
        if (nm.norm_cost) c = fmin(fmax(c / dens[1], -nm.clip_cost), nm.clip_cost);
        a.buf.costs[tn] = (float)c;
      }
      last_done_s = done_s[n];
      a.ag.last_dones[n] = (uint8_t)done_s[n];
      a.ag.raw_rew[n] = rawr_s[n];
      if (a.raw_plane != nullptr) a.raw_plane[tn] = rawr_s[n];
      a.ag.dones[n] = (uint8_t)done_s[n];
    }
    if (n == 0) {              // the statistics for launch k + 1; after the rollout's last step also the normaliser's own arrays
      const bool last = k == T;
      if (tid < O) {
        dst.mean[tid] = o_mean; dst.var[tid] = o_var;
        if (last) { nm.obs_mean[tid] = o_mean; nm.obs_var[tid] = o_var; }
      }
      if (tid == 0) { dst.count[0] = o_cnt; if (last) nm.obs_count[0] = o_cnt; }
      if (lane == 0 && w == 3) {
        dst.ret_stats[0] = st_m; dst.ret_stats[1] = st_v; dst.ret_stats[2] = st_c;
        if (last) { nm.ret_stats[0] = st_m; nm.ret_stats[1] = st_v; nm.ret_stats[2] = st_c; }
      }
      if (lane == 0 && w == 2 && has_cost) {
        dst.cost_stats[0] = st_m; dst.cost_stats[1] = st_v; dst.cost_stats[2] = st_c;
        if (last) { nm.cost_stats[0] = st_m; nm.cost_stats[1] = st_v; nm.cost_stats[2] = st_c; }
      }
    }
    __syncthreads();
    if (n == 0 && tid < N) {
      dst.ret[tid] = ret_s[tid];
      if (has_cost) dst.cost_ret[tid] = cret_s[tid];
      if (k == T) { nm.ret[tid] = ret_s[tid]; if (has_cost) nm.cost_ret[tid] = cret_s[tid]; }
    }
  }
  if (k >= T) return;
  // ---------------- act for step k: act_step_kernel minus the env step ----------------
  __syncthreads();
  const size_t tn = (size_t)k * N + n;
  const float* noise_row = a.noise + tn * (a.pl.discrete ? 1 : A);
  policy_forward_block<OCT>(a.pl, R, sh, noise_row, 0, a.alow, a.ahigh);
  __syncthreads();
  if (w == 0) {
    const int AH = a.pl.discrete ? 1 : A;       // the host reads the clipped action (the index when discrete) after its sync
    if (lane < AH) h.hs.act_host[(size_t)n * AH + lane] = sh.act_clip[lane];
  } else if (w == 3) {
    float cost = 0.f;
    if constexpr (REGION) cost = cost_region_wave(rtab, a.cr.n_clauses, a.cr.combine, sh.s_old, sh.act_clip, O);
    else if constexpr (CIT == 0) cost = cost_fn_wave(cf, sh.s_old, sh.act_clip);
    else if (a.has_cn) cost = cost_forward_wave<CIT>(a.cn, a.cl, C, sh.s_old, sh.act_clip, sh.cx, sh.ch, DISC ? 1 : 0);
    if (lane == 0) {
      a.ag.raw_cost[n] = cost; a.buf.orig_costs[tn] = cost;
      dst.cost[n] = (double)cost;              // read by every workgroup of launch k + 1 (ag.raw_cost[n] is rewritten by launch k + 1)
    }
  } else if (w == 2) {
    float* ob = a.buf.observations + tn * O;
    float* oob = a.buf.orig_observations + tn * O;
    for (int i = lane; i < O; i += WAVE) { ob[i] = sh.x[i]; oob[i] = (float)sh.s_old[i]; }
    if (lane < AS) a.buf.actions[tn * AS + lane] = sh.act_raw[lane];
    if (lane < A && !a.pl.discrete) a.ag.act_clipped[(size_t)n * A + lane] = sh.act_clip[lane];
    if (lane == 0) {
      a.buf.dones[tn] = (float)last_done_s;
      a.buf.reward_values[tn] = sh.scal[0];
      a.buf.cost_values[tn] = sh.scal[1];
      a.buf.log_probs[tn] = sh.scal[2];
      a.ag.last_v_r[n] = sh.scal[0];
      a.ag.last_v_c[n] = sh.scal[1];
    }
  }
}

// =================================================================================================================
// sampling / evaluation episodes over ONE host env (icrl_host_episode_step): one launch per env step, one workgroup.  Launch k is
// one pass of sample_episodes_body around the env step — same expressions, same order — with the raw observation read from the
// staging block instead of produced by env_step_wave: normalise (frozen statistics), record row k - 1, forward, action out.
// Nothing is carried between launches on the device (the statistics are frozen, the episode sums are the host's); no cost wave.
// =================================================================================================================
struct HostEpisodeArgs {
  icrl_norm_t nm;          // training must be 0: statistics are only read
  icrl_host_episode_t he;  // act_host: the device's mapping of the host address
  PolLayout pl;
  const float* PT;
  const float* noise;      // [rows][act] or NULL (deterministic)
  const float* alow;
  const float* ahigh;
};

template <int OCT>
__global__ void __launch_bounds__(256) host_episode_kernel(HostEpisodeArgs h, int k, int act) {
  __shared__ ActShared sh;
  PolRegs<OCT> R;                      // waves 0..2; wave 3 only takes part in the barriers
  if (act) load_pol_regs<OCT>(h.pl, h.PT, R);
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int O = h.pl.O, A = h.pl.A;
  const int AS = h.pl.discrete ? 1 : A;
  const icrl_norm_t& nm = h.nm;
  const double* const st_obs = reinterpret_cast<const double*>(h.he.stage);
  if (tid >= O && tid < MAX_OBS) sh.x[tid] = 0.f;        // pad = 0 (the forward reads whole float4 rows against zero pad weights)
  if (tid < O) {
    const double raw = st_obs[tid];
    double o = raw;
    if (nm.norm_obs) {
      const double n_mean = nm.obs_mean[tid], n_den = sqrt(nm.obs_var[tid] + nm.epsilon);
      o = fmin(fmax((raw - n_mean) / n_den, -nm.clip_obs), nm.clip_obs);
    }
    sh.x[tid] = (float)o;
    if (k >= 1) {                      // the observation after step k - 1
      h.he.orig_obs[(size_t)(k - 1) * O + tid] = raw;
      h.he.obs[(size_t)(k - 1) * O + tid] = o;
    }
  }
  if (!act) return;
  __syncthreads();
  const bool has_box = h.alow != nullptr && h.ahigh != nullptr;
  policy_forward_block<OCT>(h.pl, R, sh, h.noise != nullptr ? h.noise + (size_t)k * AS : nullptr, h.he.deterministic || h.noise == nullptr,
                            has_box ? h.alow : nullptr, has_box ? h.ahigh : nullptr);
  __syncthreads();
  if (w == 0 && lane < AS) {           // the host reads the clipped action (the index when discrete) after its sync
    const float c = sh.act_clip[lane];
    h.he.act_host[lane] = c;
    h.he.actions[(size_t)k * AS + lane] = c;
  }
}

// rows from which icrl_policy_forward / icrl_policy_evaluate take the 16-rows-per-pass MFMA kernel (below: one workgroup per row)
constexpr int ROWS_KERNEL_MIN = 64;

// icrl_policy_forward_sde (sde.hip checked the descriptor): one workgroup per row at every N, the kernel icrl_policy_forward takes below
// ROWS_KERNEL_MIN rows.  The network's transposes lie in params_t where icrl_policy_prepare leaves them for the descriptor of the network
// alone — (params, params_t) + (MAX_H - 1) * act_dim, n_params less as much: the diagonal layout with the matrix's last row as log_std.
int launch_policy_forward_sde(const icrl_policy_t* p, const double* obs, const float* expl, long long expl_stride, int N, int deterministic, const float* alow,
                              const float* ahigh, float* actions, float* act_clipped, float* v_r, float* v_c, float* log_prob, hipStream_t s) {
  const PolLayout L = make_pol_layout(p->obs_dim, p->act_dim, p->h1, p->h2, 0);
  const float* PT = p->params_t + (MAX_H - 1) * p->act_dim;
  if (L.O <= 32)
    hipLaunchKernelGGL(policy_forward_sde_kernel<2>, dim3(N), dim3(192), 0, s, L, PT, (const float*)p->params, obs, expl, expl_stride, deterministic, alow,
                       ahigh, actions, act_clipped, v_r, v_c, log_prob);
  else
    hipLaunchKernelGGL(policy_forward_sde_kernel<8>, dim3(N), dim3(192), 0, s, L, PT, (const float*)p->params, obs, expl, expl_stride, deterministic, alow,
                       ahigh, actions, act_clipped, v_r, v_c, log_prob);
  return (int)hipGetLastError();
}

}  // namespace icrl

using namespace icrl;

extern "C" int icrl_policy_prepare(const icrl_policy_t* p, void* stream) {
  if (policy_is_wide(p)) return launch_generic_transpose(p, (hipStream_t)stream);      // generic-shape path: per-layer transposes (generic.hip)
  if (!dims_ok(p)) return bad_dims("icrl_policy_prepare", p);
  PolLayout L = make_pol_layout(p->obs_dim, p->act_dim, p->h1, p->h2, p->discrete);
  if (L.n != p->n_params) return fail("icrl_policy_prepare: n_params = %d, the layout needs %d", p->n_params, L.n);
  hipLaunchKernelGGL(policy_transpose_kernel, dim3((L.n + 255) / 256), dim3(256), 0, (hipStream_t)stream, L, p->params, p->params_t);
  return (int)hipGetLastError();
}

extern "C" int icrl_costnet_prepare(const icrl_costnet_t* cn, void* stream) {
  if (as_cost_fn(cn)) return refuse_cost_fn("icrl_costnet_prepare");
  if (as_cost_disc(cn)) return refuse_cost_disc("icrl_costnet_prepare");      // (prepare the inner net)
  if (as_cost_region(cn)) return refuse_cost_region("icrl_costnet_prepare");
  if (cn->n_hidden > 2 || cn->n_hidden == 0) return 0;      // served 64 rows per workgroup from `params` (cn_train.hip): no transposed copy
  if (!costnet_is_wide(cn) && !cn_ok(cn)) return bad_cn("icrl_costnet_prepare", cn);
  CnLayout L = make_cn_layout(cn->in_dim, cn->n_hidden, cn->h1, cn->h2);
  if (L.n != cn->n_params) return fail("icrl_costnet_prepare: n_params = %d, the layout needs %d", cn->n_params, L.n);
  hipLaunchKernelGGL(costnet_transpose_kernel, dim3((L.n + 255) / 256), dim3(256), 0, (hipStream_t)stream, L, cn->params, cn->params_t);
  return (int)hipGetLastError();
}

extern "C" int icrl_policy_forward(const icrl_policy_t* p, const double* obs, const float* noise, int N, int deterministic,
                                   const float* action_low, const float* action_high, float* actions, float* act_clipped,
                                   float* v_r, float* v_c, float* log_prob, void* stream) {
  if (N <= 0) return fail("policy forward / evaluate: N = %d rows", N);
  if (policy_is_wide(p))      // hidden widths above 64: the generic-shape kernel (generic.hip)
    return launch_policy_generic(p, obs, noise, N, deterministic, action_low, action_high, actions, act_clipped, v_r, v_c, log_prob, nullptr, nullptr,
                                 (hipStream_t)stream);
  if (!dims_ok(p)) return bad_dims("policy forward / evaluate", p);
  PolLayout L = make_pol_layout(p->obs_dim, p->act_dim, p->h1, p->h2, p->discrete);
  if (p->n_params != L.n)      // (a gSDE policy's buffer — log_std a matrix — is served by icrl_policy_forward_sde / icrl_policy_sde_fwd_bwd alone)
    return fail("policy forward / evaluate: n_params = %d, the layout of (%d, %d, %d, %d) needs %d", p->n_params, p->obs_dim, p->act_dim, p->h1, p->h2, L.n);
  if (N >= ROWS_KERNEL_MIN && !p->discrete) {
    const int grid = (N + 15) / 16 < 1024 ? (N + 15) / 16 : 1024;
    if (L.O <= 32)
      hipLaunchKernelGGL(policy_rows_kernel<2>, dim3(grid), dim3(192), 0, (hipStream_t)stream, L, p->params_t, obs, noise, deterministic,
                         action_low, action_high, actions, act_clipped, v_r, v_c, log_prob, (const float*)nullptr, (float*)nullptr, N);
    else
      hipLaunchKernelGGL(policy_rows_kernel<8>, dim3(grid), dim3(192), 0, (hipStream_t)stream, L, p->params_t, obs, noise, deterministic,
                         action_low, action_high, actions, act_clipped, v_r, v_c, log_prob, (const float*)nullptr, (float*)nullptr, N);
    return (int)hipGetLastError();
  }
  if (L.O <= 32)
    hipLaunchKernelGGL(policy_forward_kernel<2>, dim3(N), dim3(192), 0, (hipStream_t)stream, L, p->params_t, obs, noise,
                       deterministic, action_low, action_high, actions, act_clipped, v_r, v_c, log_prob,
                       (const float*)nullptr, (float*)nullptr);
  else
    hipLaunchKernelGGL(policy_forward_kernel<8>, dim3(N), dim3(192), 0, (hipStream_t)stream, L, p->params_t, obs, noise,
                       deterministic, action_low, action_high, actions, act_clipped, v_r, v_c, log_prob,
                       (const float*)nullptr, (float*)nullptr);
  return (int)hipGetLastError();
}

extern "C" int icrl_policy_evaluate(const icrl_policy_t* p, const double* obs, const float* actions, int N, float* v_r,
                                    float* v_c, float* log_prob, float* entropy, void* stream) {
  if (N <= 0) return fail("policy forward / evaluate: N = %d rows", N);
  if (policy_is_wide(p))
    return launch_policy_generic(p, obs, nullptr, N, 1, nullptr, nullptr, nullptr, nullptr, v_r, v_c, log_prob, actions, entropy, (hipStream_t)stream);
  if (!dims_ok(p)) return bad_dims("policy forward / evaluate", p);
  PolLayout L = make_pol_layout(p->obs_dim, p->act_dim, p->h1, p->h2, p->discrete);
  if (p->n_params != L.n)      // (a gSDE policy's buffer — log_std a matrix — is served by icrl_policy_forward_sde / icrl_policy_sde_fwd_bwd alone)
    return fail("policy forward / evaluate: n_params = %d, the layout of (%d, %d, %d, %d) needs %d", p->n_params, p->obs_dim, p->act_dim, p->h1, p->h2, L.n);
  if (N >= ROWS_KERNEL_MIN && !p->discrete) {
    const int grid = (N + 15) / 16 < 1024 ? (N + 15) / 16 : 1024;
    if (L.O <= 32)
      hipLaunchKernelGGL(policy_rows_kernel<2>, dim3(grid), dim3(192), 0, (hipStream_t)stream, L, p->params_t, obs, (const float*)nullptr, 1,
                         (const float*)nullptr, (const float*)nullptr, (float*)nullptr, (float*)nullptr, v_r, v_c, log_prob, actions, entropy, N);
    else
      hipLaunchKernelGGL(policy_rows_kernel<8>, dim3(grid), dim3(192), 0, (hipStream_t)stream, L, p->params_t, obs, (const float*)nullptr, 1,
                         (const float*)nullptr, (const float*)nullptr, (float*)nullptr, (float*)nullptr, v_r, v_c, log_prob, actions, entropy, N);
    return (int)hipGetLastError();
  }
  if (L.O <= 32)
    hipLaunchKernelGGL(policy_forward_kernel<2>, dim3(N), dim3(192), 0, (hipStream_t)stream, L, p->params_t, obs,
                       (const float*)nullptr, 1, (const float*)nullptr, (const float*)nullptr, (float*)nullptr, (float*)nullptr,
                       v_r, v_c, log_prob, actions, entropy);
  else
    hipLaunchKernelGGL(policy_forward_kernel<8>, dim3(N), dim3(192), 0, (hipStream_t)stream, L, p->params_t, obs,
                       (const float*)nullptr, 1, (const float*)nullptr, (const float*)nullptr, (float*)nullptr, (float*)nullptr,
                       v_r, v_c, log_prob, actions, entropy);
  return (int)hipGetLastError();
}

// sample_episodes_kernel for the policies of the generic-shape path (layers above 64 units, shared trunk, other depths): the same
// persistent episode loop, one workgroup per stream, with the table-driven forward of generic.h on the trunk + policy branch (slot 0;
// the value branches are not needed here) and the weights read from the per-layer transposes every step (L2-resident).
struct GenSampleArgs {
  icrl_env_t env;
  icrl_norm_t nm;
  const float* P;
  const float* PT;
  const float* noise;
  const float* alow;
  const float* ahigh;
  int episodes_per_stream, rows_per_stream, deterministic, do_reset;
  const int* stream_row0;
  int total_rows;
  double* orig_obs;
  double* obs;
  float* actions;
  double* ep_rewards;
  int* ep_lengths;
};

__global__ void __launch_bounds__(GEN_MAX_H) sample_episodes_generic_kernel(GenNet net, GenSampleArgs a) {
  __shared__ float x[MAX_OBS];
  __shared__ float act[GEN_MAX_ROW];
  __shared__ double s_old[MAX_OBS], s_new[MAX_OBS], n_mean[MAX_OBS], n_den[MAX_OBS];
  __shared__ double Bl[MAX_OBS * MAX_ACT];
  __shared__ float act_raw[MAX_ACT], act_clip[MAX_ACT], noise_s[MAX_ACT], alow_s[MAX_ACT], ahigh_s[MAX_ACT];
  __shared__ int s_done;
  __shared__ double s_rew;
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, nt = blockDim.x;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int O = net.O, A = net.A, AS = net.discrete ? 1 : A;
  icrl_env_t env = a.env;
  const int norm_obs = a.nm.norm_obs, deterministic = a.deterministic;
  const double clip_obs = a.nm.clip_obs;
  for (int i = tid; i < O * a.env.act_dim; i += nt) Bl[i] = a.env.B[i];
  env.B = Bl;
  const bool has_box = a.alow != nullptr && a.ahigh != nullptr;
  if (tid < MAX_ACT) { alow_s[tid] = (has_box && tid < A) ? a.alow[tid] : 0.f; ahigh_s[tid] = (has_box && tid < A) ? a.ahigh[tid] : 0.f; }
  const uint32_t e_key = a.env.key[n];
  uint32_t e_ctr = a.env.step_count[n];
  int e_tep = a.env.t_ep[n];
  for (int i = tid; i < O; i += nt) {      // frozen normaliser statistics; the state the stream starts from
    n_mean[i] = a.nm.norm_obs ? a.nm.obs_mean[i] : 0.0;
    n_den[i] = a.nm.norm_obs ? sqrt(a.nm.obs_var[i] + a.nm.epsilon) : 1.0;
    double v = a.env.s[(size_t)n * O + i];
    if (a.do_reset) v = env_reset_value(a.env, e_key, e_ctr, i);
    s_new[i] = v;
  }
  if (a.do_reset) e_tep = 0;
  __syncthreads();
  size_t row = a.stream_row0 != nullptr ? (size_t)a.stream_row0[n] : (size_t)n * a.rows_per_stream;
  const size_t row_end = a.stream_row0 != nullptr ? (size_t)a.total_rows : row + a.rows_per_stream;
  for (int ep = 0; ep < a.episodes_per_stream; ++ep) {
    double ep_rew = 0.0;
    int ep_len = 0;
    while (true) {
      for (int i = tid; i < O; i += nt) {
        const double raw = s_new[i];
        double o = raw;
        if (norm_obs) o = fmin(fmax((raw - n_mean[i]) / n_den[i], -clip_obs), clip_obs);
        s_old[i] = raw;
        x[i] = (float)o;
      }
      const bool in_rows = row < row_end;      // (a stream whose speculative start row was too late can run off the arrays)
      if (a.noise != nullptr && tid < AS) noise_s[tid] = in_rows ? a.noise[row * AS + tid] : 0.f;
      __syncthreads();
      gen_mlp_forward(net, a.PT, x, act, 0, tid);
      if (tid == 0) {
        float lp, ent;
        gen_policy_head(net, a.P, act + net.layer[net.head[0]].act_off, a.noise != nullptr ? noise_s : nullptr, deterministic || a.noise == nullptr,
                        has_box ? alow_s : nullptr, has_box ? ahigh_s : nullptr, nullptr, act_raw, act_clip, lp, ent);
      }
      __syncthreads();
      if (w == 0) {
        double rew; int done;
        env_step_wave(env, n, s_old, act_clip, e_key, e_ctr, e_tep, s_new, rew, done);
        if (lane == 0) { s_done = done; s_rew = rew; }
        if (lane < AS && in_rows) a.actions[row * AS + lane] = act_clip[lane];
      }
      __syncthreads();
      if (in_rows)
        for (int i = tid; i < O; i += nt) {
          const double raw = s_new[i];
          double o = raw;
          if (norm_obs) o = fmin(fmax((raw - n_mean[i]) / n_den[i], -clip_obs), clip_obs);
          a.orig_obs[row * O + i] = raw;
          a.obs[row * O + i] = o;
        }
      ep_rew += s_rew;     // episode_reward += reward (un-normalised: norm_reward is False on sampling / eval envs)
      ++ep_len;
      ++row;
      const int done = s_done;
      __syncthreads();
      if (done) break;
    }
    if (tid == 0) { a.ep_rewards[(size_t)n * a.episodes_per_stream + ep] = ep_rew; a.ep_lengths[(size_t)n * a.episodes_per_stream + ep] = ep_len; }
  }
}

static int make_sample_args(const icrl_env_t* env, const icrl_norm_t* nm, const icrl_policy_t* pol, const float* noise,
                            const float* action_low, const float* action_high, int episodes_per_stream, int rows_per_stream,
                            int deterministic, int do_reset, const int32_t* stream_row0, int total_rows, double* orig_obs, double* obs,
                            float* actions, double* ep_rewards, int32_t* ep_lengths, SampleArgs& a) {
  if (!dims_ok(pol)) return bad_dims("icrl_sample_episodes", pol);
  if (env->obs_dim != pol->obs_dim || nm->training)
    return fail("icrl_sample_episodes: env obs_dim %d vs policy %d; the normaliser must be frozen (training = %d)", env->obs_dim, pol->obs_dim, nm->training);
  if (episodes_per_stream * env->max_steps > rows_per_stream)
    return fail("icrl_sample_episodes: %d episodes x %d steps do not fit %d rows per stream", episodes_per_stream, env->max_steps, rows_per_stream);
  if (stream_row0 != nullptr && total_rows < 1) return fail("icrl_sample_episodes: stream_row0 given with total_rows = %d", total_rows);
  a.stream_row0 = stream_row0; a.total_rows = total_rows;
  a.env = *env; a.nm = *nm; a.pl = make_pol_layout(pol->obs_dim, pol->act_dim, pol->h1, pol->h2, pol->discrete);
  a.PT = pol->params_t; a.noise = noise; a.alow = action_low; a.ahigh = action_high;
  a.episodes_per_stream = episodes_per_stream; a.rows_per_stream = rows_per_stream; a.deterministic = deterministic;
  a.do_reset = do_reset; a.orig_obs = orig_obs; a.obs = obs; a.actions = actions; a.ep_rewards = ep_rewards; a.ep_lengths = ep_lengths;
  a.pt_in_lds = 0;
  return 0;
}

extern "C" int icrl_sample_episodes(const icrl_env_t* env, const icrl_norm_t* nm, const icrl_policy_t* pol, const float* noise,
                                    const float* action_low, const float* action_high, int episodes_per_stream,
                                    int rows_per_stream, int deterministic, int do_reset, const int32_t* stream_row0, int total_rows,
                                    double* orig_obs, double* obs, float* actions, double* ep_rewards, int32_t* ep_lengths,
                                    void* stream) {
  if (policy_is_wide(pol)) {      // generic-shape path: the same persistent loop with the table-driven forward
    GenNet net;
    if (int e = make_gen_net(pol, &net, "icrl_sample_episodes")) return e;
    if (env->obs_dim != pol->obs_dim || nm->training || env->obs_dim > MAX_OBS || env->act_dim > MAX_ACT || pol->params_t == nullptr)
      return fail("icrl_sample_episodes (generic-shape path): env obs_dim %d vs policy %d (<= %d), act_dim %d (<= %d); the normaliser must be frozen "
                  "(training = %d); params_t %s", env->obs_dim, pol->obs_dim, MAX_OBS, env->act_dim, MAX_ACT, nm->training, pol->params_t ? "set" : "NULL");
    if (episodes_per_stream * env->max_steps > rows_per_stream)
      return fail("icrl_sample_episodes: %d episodes x %d steps do not fit %d rows per stream", episodes_per_stream, env->max_steps, rows_per_stream);
    if (stream_row0 != nullptr && total_rows < 1) return fail("icrl_sample_episodes: stream_row0 given with total_rows = %d", total_rows);
    GenSampleArgs g{*env, *nm, pol->params, pol->params_t, noise, action_low, action_high, episodes_per_stream, rows_per_stream, deterministic, do_reset,
                    stream_row0, total_rows, orig_obs, obs, actions, ep_rewards, ep_lengths};
    hipLaunchKernelGGL(sample_episodes_generic_kernel, dim3(env->n_envs), dim3(net.W), 0, (hipStream_t)stream, net, g);
    return (int)hipGetLastError();
  }
  SampleArgs a;
  const int bad = make_sample_args(env, nm, pol, noise, action_low, action_high, episodes_per_stream, rows_per_stream, deterministic,
                                   do_reset, stream_row0, total_rows, orig_obs, obs, actions, ep_rewards, ep_lengths, a);
  if (bad) return bad;
  if (a.pl.O <= 32) hipLaunchKernelGGL(sample_episodes_kernel<2>, dim3(env->n_envs), dim3(192), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(sample_episodes_kernel<8>, dim3(env->n_envs), dim3(192), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

extern "C" int icrl_sample_episodes_batch(int n_runs, const icrl_sample_job_t* jobs, const float* action_low, const float* action_high,
                                          int episodes_per_stream, int rows_per_stream, int deterministic, int do_reset,
                                          void* args_ws, long long args_ws_bytes, void* stream) {
  static_assert(sizeof(SampleArgs) <= ICRL_BATCH_ARGS_BYTES, "ICRL_BATCH_ARGS_BYTES");
  if (n_runs < 1 || n_runs > 65535) return fail("icrl_sample_episodes_batch: n_runs = %d (1..65535)", n_runs);
  if (args_ws == nullptr || args_ws_bytes < (long long)n_runs * ICRL_BATCH_ARGS_BYTES)
    return fail("icrl_sample_episodes_batch: args_ws holds %lld B, %d runs need %lld", args_ws_bytes, n_runs, (long long)n_runs * ICRL_BATCH_ARGS_BYTES);
  hipStream_t s = (hipStream_t)stream;
  SampleArgs* d_args = (SampleArgs*)args_ws;
  const icrl_sample_job_t& j0 = jobs[0];
  for (int r = 0; r < n_runs; ++r) {
    const icrl_sample_job_t& j = jobs[r];
    if (j.env->n_envs != j0.env->n_envs || j.env->obs_dim != j0.env->obs_dim || j.pol->act_dim != j0.pol->act_dim ||
        j.pol->discrete != j0.pol->discrete || j.env->max_steps != j0.env->max_steps)
      return fail("icrl_sample_episodes_batch: run %d differs from run 0 in a shape (streams / obs / act / discrete / max_steps)", r);
    SampleArgs a;
    const int bad = make_sample_args(j.env, j.nm, j.pol, j.noise, action_low, action_high, episodes_per_stream, rows_per_stream,
                                     deterministic, do_reset, j.stream_row0, j.total_rows, j.orig_obs, j.obs, j.actions, j.ep_rewards,
                                     j.ep_lengths, a);
    if (bad) return bad;
    const int e = put_args(a, d_args + r, s);
    if (e) return e;
  }
  if (j0.pol->obs_dim <= 32) hipLaunchKernelGGL(sample_episodes_batch_kernel<2>, dim3(j0.env->n_envs, n_runs), dim3(192), 0, s, d_args);
  else hipLaunchKernelGGL(sample_episodes_batch_kernel<8>, dim3(j0.env->n_envs, n_runs), dim3(192), 0, s, d_args);
  return (int)hipGetLastError();
}

// ---- icrl_sample_episodes_chain: workspace = [status word | position words of all jobs | private row slots of the jobs that may end early]
static size_t chain_align(size_t b) { return (b + 255) / 256 * 256; }
static size_t chain_slot_bytes(const icrl_chain_job_t& j) {      // orig_obs, obs, actions rows of one job's slots
  if (j.fixed_len) return 0;
  const size_t rows = (size_t)j.env->n_envs * j.env->max_steps;
  const size_t AS = j.pol->discrete ? 1 : j.pol->act_dim;
  return 2 * chain_align(rows * j.env->obs_dim * sizeof(double)) + chain_align(rows * AS * sizeof(float));
}
static int chain_total_streams(int n_jobs, const icrl_chain_job_t* jobs) {
  long long t = 0;
  for (int r = 0; r < n_jobs; ++r) t += jobs[r].env->n_envs > 0 ? jobs[r].env->n_envs : 0;
  return t > (1 << 30) ? (1 << 30) : (int)t;
}

extern "C" size_t icrl_sample_episodes_chain_ws_bytes(int n_jobs, const icrl_chain_job_t* jobs) {
  if (n_jobs < 1 || jobs == nullptr) return 0;
  size_t b = 256 + chain_align((size_t)chain_total_streams(n_jobs, jobs) * sizeof(unsigned));
  for (int r = 0; r < n_jobs; ++r) b += chain_slot_bytes(jobs[r]);
  return b;
}

extern "C" int icrl_sample_episodes_chain(int n_jobs, const icrl_chain_job_t* jobs, const float* action_low, const float* action_high,
                                          int do_reset, void* ws, long long ws_bytes, void* args_ws, long long args_ws_bytes, void* stream) {
  static_assert(sizeof(ChainArgs) <= ICRL_BATCH_ARGS_BYTES, "ICRL_BATCH_ARGS_BYTES");
  if (n_jobs < 1 || n_jobs > 65535 || jobs == nullptr) return fail("icrl_sample_episodes_chain: n_jobs = %d (1..65535)", n_jobs);
  // what the chained kernel does not serve (the caller takes the multi-pass path): the reason starts with "refused"
  static int n_cu = 0;
  if (n_cu == 0) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) n_cu = 0;
  }
  const int total = chain_total_streams(n_jobs, jobs);
  if (total > n_cu)
    return fail("icrl_sample_episodes_chain: refused: %d streams on %d compute units (every stream must be resident while its successors wait)", total, n_cu);
  int max_streams = 0;
  for (int r = 0; r < n_jobs; ++r) {
    const icrl_chain_job_t& j = jobs[r];
    if (policy_is_wide(j.pol)) return fail("icrl_sample_episodes_chain: refused: job %d has a generic-shape policy", r);
    if (j.env->reward_form >= 4) return fail("icrl_sample_episodes_chain: refused: job %d steps a Point env (reward_form %d): the chained kernel is built without its step", r, j.env->reward_form);
    if (j.episodes_per_stream != 1) return fail("icrl_sample_episodes_chain: refused: job %d runs %d episodes per stream (1 only)", r, j.episodes_per_stream);
    if ((j.pol->obs_dim <= 32) != (jobs[0].pol->obs_dim <= 32)) return fail("icrl_sample_episodes_chain: refused: job %d and job 0 take different kernels (obs %d / %d)", r, j.pol->obs_dim, jobs[0].pol->obs_dim);
    if (j.env->n_envs < 1 || j.base_count == nullptr) return fail("icrl_sample_episodes_chain: job %d: %d streams, base_count %p", r, j.env->n_envs, (const void*)j.base_count);
    if ((long long)j.env->n_envs * j.env->max_steps >= (1ll << 31) - 1) return fail("icrl_sample_episodes_chain: job %d: %d streams x %d steps do not fit a 31-bit row", r, j.env->n_envs, j.env->max_steps);
    if (j.env->n_envs > max_streams) max_streams = j.env->n_envs;
  }
  const long long need = (long long)icrl_sample_episodes_chain_ws_bytes(n_jobs, jobs);
  if (ws == nullptr || ws_bytes < need) return fail("icrl_sample_episodes_chain: ws holds %lld B, the jobs need %lld", ws_bytes, need);
  if (args_ws == nullptr || args_ws_bytes < (long long)n_jobs * ICRL_BATCH_ARGS_BYTES)
    return fail("icrl_sample_episodes_chain: args_ws holds %lld B, %d jobs need %lld", args_ws_bytes, n_jobs, (long long)n_jobs * ICRL_BATCH_ARGS_BYTES);
  hipStream_t s = (hipStream_t)stream;
  ChainArgs* d_args = (ChainArgs*)args_ws;
  char* const base = (char*)ws;
  unsigned* words = (unsigned*)(base + 256);
  char* slots = base + 256 + chain_align((size_t)total * sizeof(unsigned));
  for (int r = 0; r < n_jobs; ++r) {
    const icrl_chain_job_t& j = jobs[r];
    const int rows = j.env->n_envs * j.env->max_steps;
    ChainArgs c;
    const int bad = make_sample_args(j.env, j.nm, j.pol, j.noise, action_low, action_high, 1, j.env->max_steps, j.deterministic, do_reset, nullptr,
                                     rows, j.orig_obs, j.obs, j.actions, j.ep_rewards, j.ep_lengths, c.s);
    if (bad) return bad;
    c.next_start = words; words += j.env->n_envs;
    c.status = (unsigned*)base;
    c.exec_steps = j.exec_steps;
    c.base_count = j.base_count;
    c.fixed_len = j.fixed_len != 0; c.n_streams = j.env->n_envs;
    if (c.fixed_len) { c.slot_orig = j.orig_obs; c.slot_obs = j.obs; c.slot_act = j.actions; }
    else {
      const size_t AS = j.pol->discrete ? 1 : j.pol->act_dim;
      const size_t ob = chain_align((size_t)rows * j.env->obs_dim * sizeof(double));
      c.slot_orig = (double*)slots; c.slot_obs = (double*)(slots + ob); c.slot_act = (float*)(slots + 2 * ob);
      slots += 2 * ob + chain_align((size_t)rows * AS * sizeof(float));
    }
    hipLaunchKernelGGL(chain_prep_kernel, dim3(1), dim3(64), 0, s, c, d_args + r, (int)(r == 0));
    if (const int e = (int)hipGetLastError()) return e;
  }
  if (jobs[0].pol->obs_dim <= 32) hipLaunchKernelGGL(sample_episodes_chain_kernel<2>, dim3(max_streams, n_jobs), dim3(192), 0, s, d_args);
  else hipLaunchKernelGGL(sample_episodes_chain_kernel<8>, dim3(max_streams, n_jobs), dim3(192), 0, s, d_args);
  return (int)hipGetLastError();
}

// ---- the samplers of a gSDE policy.  What both entry points check of one (env, normaliser, policy) triple, on the host, before any device call.
static int sde_sample_check(const char* who, const char* where, const icrl_env_t* env, const icrl_norm_t* nm, const icrl_policy_t* pol) {
  if (env == nullptr || nm == nullptr || pol == nullptr) return fail("%s:%s NULL argument (env, nm and pol are required)", who, where);
  if (pol->params == nullptr || pol->params_t == nullptr) return fail("%s:%s NULL argument (pol->params and pol->params_t are required)", who, where);
  if (pol->discrete) return fail("%s:%s a discrete policy has no gSDE head", who, where);
  if (pol->arch != nullptr || pol->h1 != MAX_H || pol->h2 != MAX_H)
    return fail("%s:%s hidden widths (%d, %d)%s; the gSDE sampler serves the fast kind: two hidden layers per branch, stored %d x %d, no `arch`", who, where,
                pol->h1, pol->h2, pol->arch != nullptr ? " with an `arch` descriptor" : "", MAX_H, MAX_H);
  if (pol->obs_dim < 1 || pol->obs_dim > MAX_OBS || pol->act_dim < 1 || pol->act_dim > MAX_ACT)
    return fail("%s:%s policy obs_dim %d (1..%d), act_dim %d (1..%d)", who, where, pol->obs_dim, MAX_OBS, pol->act_dim, MAX_ACT);
  const int n_diag = make_pol_layout(pol->obs_dim, pol->act_dim, pol->h1, pol->h2, 0).n, n_sde = make_sde_layout(pol->obs_dim, pol->act_dim, pol->h1, pol->h2).n;
  if (pol->n_params != n_sde)
    return fail("%s:%s n_params %d, the gSDE (log_std [%d, act_dim]) layout of (%d, %d, %d, %d) has %d%s", who, where, pol->n_params, MAX_H, pol->obs_dim,
                pol->act_dim, pol->h1, pol->h2, n_sde, pol->n_params == n_diag ? " (that is the diagonal layout's count: icrl_sample_episodes serves that policy)" : "");
  if (env->obs_dim != pol->obs_dim || env->act_dim != pol->act_dim || env->n_envs < 1)
    return fail("%s:%s env (%d streams, obs_dim %d, act_dim %d) vs policy (obs_dim %d, act_dim %d)", who, where, env->n_envs, env->obs_dim, env->act_dim,
                pol->obs_dim, pol->act_dim);
  if (nm->training) return fail("%s:%s the normaliser must be frozen (training = %d)", who, where, nm->training);
  return 0;
}

// the network alone, as launch_policy_forward_sde reads it: the diagonal layout, its transposes behind the matrix's first 63 rows
static icrl_policy_t sde_net_policy(const icrl_policy_t* pol) {
  icrl_policy_t netpol = *pol;
  netpol.params_t = pol->params_t + (MAX_H - 1) * pol->act_dim;
  return netpol;
}

extern "C" int icrl_sample_episodes_sde(const icrl_env_t* env, const icrl_norm_t* nm, const icrl_policy_t* pol, const float* expl,
                                        const float* action_low, const float* action_high, int episodes_per_stream, int rows_per_stream,
                                        int do_reset, const int32_t* stream_row0, int total_rows, double* orig_obs, double* obs, float* actions,
                                        double* ep_rewards, int32_t* ep_lengths, void* stream) {
  const char* who = "icrl_sample_episodes_sde";
  if (int e = sde_sample_check(who, "", env, nm, pol)) return e;
  if (orig_obs == nullptr || obs == nullptr || actions == nullptr || ep_rewards == nullptr || ep_lengths == nullptr)
    return fail("%s: NULL argument (orig_obs, obs, actions, ep_rewards and ep_lengths are required)", who);
  if ((action_low == nullptr) != (action_high == nullptr)) return fail("%s: NULL argument (action_low and action_high: both or neither)", who);
  if (episodes_per_stream < 1 || (long long)episodes_per_stream * env->max_steps > rows_per_stream)
    return fail("%s: %d episodes x %d steps do not fit %d rows per stream", who, episodes_per_stream, env->max_steps, rows_per_stream);
  if (stream_row0 != nullptr && total_rows < 1) return fail("%s: stream_row0 given with total_rows = %d", who, total_rows);
  const icrl_policy_t netpol = sde_net_policy(pol);
  SampleArgs a;
  const int bad = make_sample_args(env, nm, &netpol, nullptr, action_low, action_high, episodes_per_stream, rows_per_stream, expl == nullptr, do_reset,
                                   stream_row0, total_rows, orig_obs, obs, actions, ep_rewards, ep_lengths, a);
  if (bad) return bad;
  if (a.pl.O <= 32) hipLaunchKernelGGL(sample_episodes_sde_kernel<2>, dim3(env->n_envs), dim3(192), 0, (hipStream_t)stream, a, expl);
  else hipLaunchKernelGGL(sample_episodes_sde_kernel<8>, dim3(env->n_envs), dim3(192), 0, (hipStream_t)stream, a, expl);
  return (int)hipGetLastError();
}

extern "C" int icrl_sample_episodes_chain_sde(int n_jobs, const icrl_chain_job_t* jobs, const float* const* expl, const float* action_low,
                                              const float* action_high, int do_reset, void* ws, long long ws_bytes, void* args_ws,
                                              long long args_ws_bytes, void* stream) {
  static_assert(sizeof(ChainSdeArgs) <= ICRL_BATCH_ARGS_BYTES, "ICRL_BATCH_ARGS_BYTES");
  const char* who = "icrl_sample_episodes_chain_sde";
  if (n_jobs < 1 || n_jobs > 65535 || jobs == nullptr) return fail("%s: n_jobs = %d (1..65535)", who, n_jobs);
  if (expl == nullptr) return fail("%s: NULL argument (expl: one device pointer per job, NULL entries for the jobs that take the mode)", who);
  if ((action_low == nullptr) != (action_high == nullptr)) return fail("%s: NULL argument (action_low and action_high: both or neither)", who);
  for (int r = 0; r < n_jobs; ++r) {
    const icrl_chain_job_t& j = jobs[r];
    char where[24];
    snprintf(where, sizeof(where), " job %d:", r);
    if (int e = sde_sample_check(who, where, j.env, j.nm, j.pol)) return e;
    if (j.orig_obs == nullptr || j.obs == nullptr || j.actions == nullptr || j.ep_rewards == nullptr || j.ep_lengths == nullptr)
      return fail("%s: job %d: NULL argument (orig_obs, obs, actions, ep_rewards and ep_lengths are required)", who, r);
    if (j.noise != nullptr) return fail("%s: job %d has a noise array; a gSDE policy's exploration is its matrix (expl[%d]), not a per-step draw", who, r, r);
    if ((j.deterministic != 0) != (expl[r] == nullptr))
      return fail("%s: job %d: deterministic = %d with expl[%d] %s (the mode has no matrix, a sampling job needs one)", who, r, j.deterministic, r,
                  expl[r] == nullptr ? "NULL" : "set");
  }
  // what the chained kernel does not serve (the caller takes the multi-pass path): the reason starts with "refused", as icrl_sample_episodes_chain's
  int max_streams = 0;
  for (int r = 0; r < n_jobs; ++r) {
    const icrl_chain_job_t& j = jobs[r];
    if (j.env->reward_form >= 4) return fail("%s: refused: job %d steps a Point env (reward_form %d): the chained kernel is built without its step", who, r, j.env->reward_form);
    if (j.episodes_per_stream != 1) return fail("%s: refused: job %d runs %d episodes per stream (1 only)", who, r, j.episodes_per_stream);
    if ((j.pol->obs_dim <= 32) != (jobs[0].pol->obs_dim <= 32)) return fail("%s: refused: job %d and job 0 take different kernels (obs %d / %d)", who, r, j.pol->obs_dim, jobs[0].pol->obs_dim);
    if (j.base_count == nullptr) return fail("%s: job %d: %d streams, base_count %p", who, r, j.env->n_envs, (const void*)j.base_count);
    if ((long long)j.env->n_envs * j.env->max_steps >= (1ll << 31) - 1) return fail("%s: job %d: %d streams x %d steps do not fit a 31-bit row", who, r, j.env->n_envs, j.env->max_steps);
    if (j.env->n_envs > max_streams) max_streams = j.env->n_envs;
  }
  static int n_cu = 0;
  if (n_cu == 0) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) n_cu = 0;
  }
  const int total = chain_total_streams(n_jobs, jobs);
  if (total > n_cu) return fail("%s: refused: %d streams on %d compute units (every stream must be resident while its successors wait)", who, total, n_cu);
  const long long need = (long long)icrl_sample_episodes_chain_ws_bytes(n_jobs, jobs);
  if (ws == nullptr || ws_bytes < need) return fail("%s: ws holds %lld B, the jobs need %lld", who, ws_bytes, need);
  if (args_ws == nullptr || args_ws_bytes < (long long)n_jobs * ICRL_BATCH_ARGS_BYTES)
    return fail("%s: args_ws holds %lld B, %d jobs need %lld", who, args_ws_bytes, n_jobs, (long long)n_jobs * ICRL_BATCH_ARGS_BYTES);
  hipStream_t s = (hipStream_t)stream;
  ChainSdeArgs* d_args = (ChainSdeArgs*)args_ws;
  char* const base = (char*)ws;
  unsigned* words = (unsigned*)(base + 256);
  char* slots = base + 256 + chain_align((size_t)total * sizeof(unsigned));
  for (int r = 0; r < n_jobs; ++r) {
    const icrl_chain_job_t& j = jobs[r];
    const int rows = j.env->n_envs * j.env->max_steps;
    const icrl_policy_t netpol = sde_net_policy(j.pol);
    ChainSdeArgs v;
    ChainArgs& c = v.c;
    const int bad = make_sample_args(j.env, j.nm, &netpol, nullptr, action_low, action_high, 1, j.env->max_steps, j.deterministic, do_reset, nullptr, rows,
                                     j.orig_obs, j.obs, j.actions, j.ep_rewards, j.ep_lengths, c.s);
    if (bad) return bad;
    v.expl = expl[r];
    c.next_start = words; words += j.env->n_envs;
    c.status = (unsigned*)base;
    c.exec_steps = j.exec_steps;
    c.base_count = j.base_count;
    c.fixed_len = j.fixed_len != 0; c.n_streams = j.env->n_envs;
    if (c.fixed_len) { c.slot_orig = j.orig_obs; c.slot_obs = j.obs; c.slot_act = j.actions; }
    else {      // (the slot sizes of icrl_sample_episodes_chain_ws_bytes: a continuous policy, act_dim floats per row)
      const size_t ob = chain_align((size_t)rows * j.env->obs_dim * sizeof(double));
      c.slot_orig = (double*)slots; c.slot_obs = (double*)(slots + ob); c.slot_act = (float*)(slots + 2 * ob);
      slots += 2 * ob + chain_align((size_t)rows * j.pol->act_dim * sizeof(float));
    }
    hipLaunchKernelGGL(chain_prep_sde_kernel, dim3(1), dim3(64), 0, s, v, d_args + r, (int)(r == 0));
    if (const int e = (int)hipGetLastError()) return e;
  }
  if (jobs[0].pol->obs_dim <= 32) hipLaunchKernelGGL(sample_episodes_chain_sde_kernel<2>, dim3(max_streams, n_jobs), dim3(192), 0, s, d_args);
  else hipLaunchKernelGGL(sample_episodes_chain_sde_kernel<8>, dim3(max_streams, n_jobs), dim3(192), 0, s, d_args);
  return (int)hipGetLastError();
}

extern "C" int icrl_cost_region_rows(const icrl_cost_region_t* cr, const double* obs, const float* acs, int N, float* cost, void* stream) {
  if (cr == nullptr || cr->n_hidden != ICRL_COST_REGION)
    return fail("icrl_cost_region_rows: not a region cost descriptor (icrl_cost_region_t: n_hidden must be ICRL_COST_REGION)");
  if (int e = cost_region_check("icrl_cost_region_rows", cr, 0, 0, -1)) return e;
  if (N <= 0 || cost == nullptr) return fail("icrl_cost_region_rows: N = %d rows, cost = %p", N, (void*)cost);
  for (int c = 0; c < cr->n_clauses; ++c)
    for (int k = 0; k < cr->clauses[c].n_terms; ++k) {
      const bool is_obs = cr->clauses[c].col[k] < cr->obs_dim;
      if ((is_obs ? (const void*)obs : (const void*)acs) == nullptr)
        return fail("icrl_cost_region_rows: region cost (icrl_cost_region_t): clause %d, term %d reads the %s, which is NULL", c, k, is_obs ? "observations" : "actions");
    }
  const int grid = (N + 255) / 256 < 1024 ? (N + 255) / 256 : 1024;
  hipLaunchKernelGGL(cost_region_rows_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, *cr, obs, acs, N, cost);
  return (int)hipGetLastError();
}

extern "C" int icrl_cost_fn_rows(const icrl_cost_fn_t* cf, const double* obs, const float* acs, int N, float* cost, void* stream) {
  if (cf == nullptr || cf->n_hidden != ICRL_COST_FN) return fail("icrl_cost_fn_rows: not an analytic cost descriptor (n_hidden must be ICRL_COST_FN)");
  if (int e = cost_fn_check("icrl_cost_fn_rows", cf, 0, 0, -1)) return e;
  if (N <= 0 || cost == nullptr) return fail("icrl_cost_fn_rows: N = %d rows, cost = %p", N, (void*)cost);
  const bool wall = cf->kind == ICRL_COST_WALL_BEHIND || cf->kind == ICRL_COST_WALL_INFRONT || cf->kind == ICRL_COST_WALL_BOTH;
  if ((wall && obs == nullptr) || ((cf->kind == ICRL_COST_TORQUE || cf->kind == ICRL_COST_ACTION_EQUALS) && acs == nullptr))
    return fail("icrl_cost_fn_rows: cost kind %d reads the %s, which is NULL", cf->kind, wall ? "observations" : "actions");
  const int grid = (N + 255) / 256 < 1024 ? (N + 255) / 256 : 1024;
  hipLaunchKernelGGL(cost_fn_rows_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, *cf, obs, acs, N, cost);
  return (int)hipGetLastError();
}

extern "C" int icrl_cost_mlp_forward(const icrl_costnet_t* cn, const double* obs, const float* acs, int N, float* cost,
                                     void* stream) {
  if (const icrl_cost_fn_t* cf = as_cost_fn(cn)) return icrl_cost_fn_rows(cf, obs, acs, N, cost, stream);
  if (const icrl_cost_region_t* cr = as_cost_region(cn)) return icrl_cost_region_rows(cr, obs, acs, N, cost, stream);
  if (const icrl_cost_disc_t* cd = as_cost_disc(cn)) {      // the inner net read as D: one zeta, stored as it is
    if (int e = cost_disc_check("icrl_cost_mlp_forward", cd)) return e;
    return icrl_disc_reward(cd->net, obs, acs, N, cost, 0, stream);
  }
  if (N <= 0) return fail("cost forward: N = %d rows", N);
  if (costnet_is_wide(cn)) return launch_cn_cost_rows(cn, obs, acs, N, cost, 0, (hipStream_t)stream);
  if (!cn_ok(cn)) return bad_cn("cost forward", cn);
  CnLayout L = make_cn_layout(cn->in_dim, cn->n_hidden, cn->h1, cn->h2);
  if (cn->in_dim <= 32) hipLaunchKernelGGL(cost_forward_kernel<2>, dim3(N), dim3(64), 0, (hipStream_t)stream, *cn, L, obs, acs, N, cost, 0);
  else hipLaunchKernelGGL(cost_forward_kernel<10>, dim3(N), dim3(64), 0, (hipStream_t)stream, *cn, L, obs, acs, N, cost, 0);
  return (int)hipGetLastError();
}

extern "C" int icrl_disc_reward(const icrl_costnet_t* cn, const double* obs, const float* acs, int N, float* out, int apply_log,
                                void* stream) {
  if (as_cost_fn(cn)) return refuse_cost_fn("icrl_disc_reward");
  if (as_cost_disc(cn)) return refuse_cost_disc("icrl_disc_reward");
  if (as_cost_region(cn)) return refuse_cost_region("icrl_disc_reward");
  if (N <= 0) return fail("cost forward: N = %d rows", N);
  if (costnet_is_wide(cn)) return launch_cn_cost_rows(cn, obs, acs, N, out, apply_log ? 2 : 1, (hipStream_t)stream);
  if (!cn_ok(cn)) return bad_cn("cost forward", cn);
  CnLayout L = make_cn_layout(cn->in_dim, cn->n_hidden, cn->h1, cn->h2);
  const int mode = apply_log ? 2 : 1;
  if (cn->in_dim <= 32) hipLaunchKernelGGL(cost_forward_kernel<2>, dim3(N), dim3(64), 0, (hipStream_t)stream, *cn, L, obs, acs, N, out, mode);
  else hipLaunchKernelGGL(cost_forward_kernel<10>, dim3(N), dim3(64), 0, (hipStream_t)stream, *cn, L, obs, acs, N, out, mode);
  return (int)hipGetLastError();
}

// argument checks of the two GAIL entry points + the runs' argument blocks (host memory: `out`, n_runs entries)
static int make_gail_args(const char* who, int n_runs, const icrl_gail_job_t* jobs, void* args_ws, long long args_ws_bytes, GailArgs* out, bool relabel) {
  static_assert(sizeof(GailArgs) <= ICRL_BATCH_ARGS_BYTES, "ICRL_BATCH_ARGS_BYTES");
  if (args_ws == nullptr || args_ws_bytes < (long long)n_runs * ICRL_BATCH_ARGS_BYTES)
    return fail("%s: args_ws holds %lld B, %d runs need %lld", who, args_ws_bytes, n_runs, (long long)n_runs * ICRL_BATCH_ARGS_BYTES);
  for (int r = 0; r < n_runs; ++r) {
    const icrl_gail_job_t& j = jobs[r];
    GailArgs& a = out[r];
    if (j.disc == nullptr) return fail("%s: run %d has no discriminator descriptor", who, r);
    if (as_cost_fn(j.disc)) return refuse_cost_fn(who);
    if (as_cost_disc(j.disc)) return refuse_cost_disc(who);
    if (as_cost_region(j.disc)) return refuse_cost_region(who);
    if (j.rows <= 0) return fail("%s: run %d: rows = %d", who, r, j.rows);
    if (j.actions == nullptr || j.raw_obs == nullptr) return fail("%s: run %d: actions = %p, raw_obs = %p", who, r, (const void*)j.actions, (void*)j.raw_obs);
    if (j.disc->obs_dim < 1) return fail("%s: run %d: obs_dim = %d", who, r, j.disc->obs_dim);
    a.has_cost = 0;
    if (!relabel) {
      if (j.observations == nullptr || j.cost_mean == nullptr)
        return fail("%s: run %d: observations = %p, cost_mean = %p", who, r, (const void*)j.observations, (void*)j.cost_mean);
      if ((j.obs_mean == nullptr) != (j.obs_var == nullptr)) return fail("%s: run %d: obs_mean and obs_var come together or not at all", who, r);
      if (j.true_cost != nullptr) {
        if (j.true_cost->n_hidden != ICRL_COST_FN) return fail("%s: run %d: true_cost is not an analytic cost descriptor (n_hidden must be ICRL_COST_FN)", who, r);
        if (int e = cost_fn_check(who, j.true_cost, 0, 0, -1)) return e;
        const bool wall = j.true_cost->kind == ICRL_COST_WALL_BEHIND || j.true_cost->kind == ICRL_COST_WALL_INFRONT || j.true_cost->kind == ICRL_COST_WALL_BOTH;
        if (wall && j.true_cost->obs_dim != j.disc->obs_dim)
          return fail("%s: run %d: wall cost built for obs_dim %d, the rows have %d", who, r, j.true_cost->obs_dim, j.disc->obs_dim);
        const int act_store = j.disc->is_discrete ? 1 : j.disc->acs_dim;
        if (j.true_cost->kind == ICRL_COST_TORQUE && j.true_cost->acs_dim != act_store)
          return fail("%s: run %d: torque cost over %d action components, the rows have %d", who, r, j.true_cost->acs_dim, act_store);
        a.f = *j.true_cost; a.has_cost = 1;
      }
    } else {
      if (j.rewards == nullptr) return fail("%s: run %d: rewards = NULL", who, r);
      const icrl_costnet_t* c0 = jobs[0].disc;
      if (j.disc->in_dim != c0->in_dim || j.disc->n_hidden != c0->n_hidden || j.disc->h1 != c0->h1 || j.disc->h2 != c0->h2 || j.disc->h3 != c0->h3 ||
          j.disc->h4 != c0->h4 || j.disc->n_params != c0->n_params)
        return fail("%s: run %d's discriminator shape differs from run 0's (the runs of a batch share one grid)", who, r);
      if (!costnet_is_wide(j.disc)) {
        if (!cn_ok(j.disc)) return bad_cn(who, j.disc);
        a.cl = make_cn_layout(j.disc->in_dim, j.disc->n_hidden, j.disc->h1, j.disc->h2);
      }
    }
    a.cn = *j.disc;
    a.obs = j.observations; a.acs = j.actions; a.mean = j.obs_mean; a.var = j.obs_var; a.eps = j.epsilon; a.raw = j.raw_obs;
    a.rewards = j.rewards; a.cost_mean = j.cost_mean; a.rows = j.rows; a.obs_dim = j.disc->obs_dim; a.learn_cost = j.learn_cost != 0;
  }
  return 0;
}

extern "C" int icrl_gail_unnormalize_batch(int n_runs, const icrl_gail_job_t* jobs, void* args_ws, long long args_ws_bytes, void* stream) {
  const char* who = "icrl_gail_unnormalize_batch";
  if (n_runs < 1 || n_runs > 65535 || jobs == nullptr) return fail("%s: n_runs = %d (1..65535)", who, n_runs);
  GailArgs stack_args[8];
  GailArgs* args = n_runs <= 8 ? stack_args : new GailArgs[n_runs];
  int bad = make_gail_args(who, n_runs, jobs, args_ws, args_ws_bytes, args, false);
  hipStream_t s = (hipStream_t)stream;
  long long total_max = 0;
  for (int r = 0; r < n_runs && !bad; ++r) {
    const long long t = (long long)args[r].rows * args[r].obs_dim;
    total_max = t > total_max ? t : total_max;
    bad = put_args(args[r], (GailArgs*)args_ws + r, s);
  }
  if (args != stack_args) delete[] args;
  if (bad) return bad;
  const long long blocks = (total_max + 255) / 256;
  hipLaunchKernelGGL(gail_unnormalize_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048), n_runs), dim3(256), 0, s, (const GailArgs*)args_ws);
  hipLaunchKernelGGL(gail_cost_mean_kernel, dim3(1, n_runs), dim3(1024), 0, s, (const GailArgs*)args_ws);
  return (int)hipGetLastError();
}

extern "C" int icrl_gail_relabel_batch(int n_runs, const icrl_gail_job_t* jobs, void* args_ws, long long args_ws_bytes, void* stream) {
  const char* who = "icrl_gail_relabel_batch";
  if (n_runs < 1 || n_runs > 65535 || jobs == nullptr) return fail("%s: n_runs = %d (1..65535)", who, n_runs);
  GailArgs stack_args[8];
  GailArgs* args = n_runs <= 8 ? stack_args : new GailArgs[n_runs];
  int bad = make_gail_args(who, n_runs, jobs, args_ws, args_ws_bytes, args, true);
  hipStream_t s = (hipStream_t)stream;
  const bool wide = !bad && costnet_is_wide(jobs[0].disc);
  if (wide) {      // a hidden layer above 64 units, or 0 / 3 / 4 of them: 64 rows per workgroup (cn_train.hip), as icrl_disc_reward does
    if (args != stack_args) delete[] args;
    return launch_gail_relabel_rows(n_runs, jobs, args_ws, s);
  }
  int rows_max = 0;
  for (int r = 0; r < n_runs && !bad; ++r) {
    rows_max = args[r].rows > rows_max ? args[r].rows : rows_max;
    bad = put_args(args[r], (GailArgs*)args_ws + r, s);
  }
  if (args != stack_args) delete[] args;
  if (bad) return bad;
  if (jobs[0].disc->in_dim <= 32) hipLaunchKernelGGL(gail_relabel_kernel<2>, dim3(rows_max, n_runs), dim3(64), 0, s, (const GailArgs*)args_ws);
  else hipLaunchKernelGGL(gail_relabel_kernel<10>, dim3(rows_max, n_runs), dim3(64), 0, s, (const GailArgs*)args_ws);
  return (int)hipGetLastError();
}

extern "C" int icrl_synth_env_reset(const icrl_env_t* env, void* stream) {
  if (env->obs_dim > MAX_OBS || env->act_dim > MAX_ACT) return fail("synthetic env: obs_dim %d (<= %d), act_dim %d (<= %d)", env->obs_dim, MAX_OBS, env->act_dim, MAX_ACT);
  const int total = env->n_envs * env->obs_dim;
  hipLaunchKernelGGL(env_reset_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, *env);
  return (int)hipGetLastError();
}

extern "C" int icrl_synth_env_step(const icrl_env_t* env, const float* actions, double* raw_rew, uint8_t* dones, void* stream) {
  if (env->obs_dim > MAX_OBS || env->act_dim > MAX_ACT) return fail("synthetic env: obs_dim %d (<= %d), act_dim %d (<= %d)", env->obs_dim, MAX_OBS, env->act_dim, MAX_ACT);
  hipLaunchKernelGGL(env_step_kernel, dim3(env->n_envs), dim3(64), 0, (hipStream_t)stream, *env, actions, raw_rew, dones);
  return (int)hipGetLastError();
}

void icrl::launch_norm_step(const NormStepArgs& a, hipStream_t s) {
  if (a.N <= 128 && a.N * a.O <= NORM_CHUNK) hipLaunchKernelGGL(norm_step_small_kernel, dim3(1), dim3(1024), 0, s, a);
  else hipLaunchKernelGGL(norm_step_kernel, dim3(1), dim3(1024), 0, s, a);
}

extern "C" int icrl_vecnorm_reset(const icrl_norm_t* nm, const double* raw_obs, int N, int obs_dim, double* obs_out, void* stream) {
  if (N <= 0 || N > NORM_MAX_N || obs_dim > MAX_OBS)
    return fail("VecNormalize step: %d envs (1..%d per GPU: the float64 statistics are one numpy-ordered chain per column), obs_dim %d (<= %d)", N, NORM_MAX_N, obs_dim, MAX_OBS);
  hipLaunchKernelGGL(norm_reset_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, *nm, raw_obs, N, obs_dim, obs_out);
  return (int)hipGetLastError();
}

extern "C" int icrl_vecnorm_step(const icrl_norm_t* nm, const double* raw_obs, const double* raw_rew, const float* raw_cost,
                                 const uint8_t* dones, int N, int obs_dim, double* obs_out, double* rew_out, double* cost_out,
                                 void* stream) {
  if (N <= 0 || N > NORM_MAX_N || obs_dim > MAX_OBS)
    return fail("VecNormalize step: %d envs (1..%d per GPU: the float64 statistics are one numpy-ordered chain per column), obs_dim %d (<= %d)", N, NORM_MAX_N, obs_dim, MAX_OBS);
  NormStepArgs a{*nm, raw_obs, raw_rew, raw_cost, dones, N, obs_dim, obs_out, rew_out, cost_out, nullptr, nullptr, nullptr, nullptr};
  launch_norm_step(a, (hipStream_t)stream);
  return (int)hipGetLastError();
}

extern "C" int icrl_debug_rollout_profile_wide(unsigned long long* out16) {
  return (int)hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_rollout_prof_wide), sizeof(unsigned long long) * 16);
}
extern "C" int icrl_debug_rollout_trace_wide(unsigned long long* out, int n_workgroups) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wide_trace), sizeof(unsigned long long) * 4 * (size_t)(n_workgroups < NORM_MAX_N_TRACE ? n_workgroups : NORM_MAX_N_TRACE));
}

extern "C" int icrl_debug_rollout_profile(unsigned long long* out4) {
  return (int)hipMemcpyFromSymbol(out4, HIP_SYMBOL(g_rollout_prof), sizeof(unsigned long long) * 8);
}

// =================================================================================================================
// launch layer of the fused rollouts: kernel choice and launchers (the route ladders that call them: rollout_collect.hip)
// =================================================================================================================

// all N workgroups of the persistent rollout must be co-resident (they wait for each other every step): ask the runtime
// how many blocks of this kernel one CU takes.  The answer is advisory (MI355X_MICROARCH.md: it can read one high for
// SGPR-heavy kernels), hence the bounded spins + status word as the backstop.
template <typename K>
static bool persistent_fits(K kernel, int blocks, size_t dyn_lds = 0) {
  int dev = 0, cus = 0, per_cu = 0;
  if (hipGetDevice(&dev) != hipSuccess) return false;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return false;
  if (dyn_lds > 48 * 1024 && hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn_lds) != hipSuccess) return false;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, dyn_lds) != hipSuccess) return false;
  if (getenv("ICRL_DEBUG")) fprintf(stderr, "icrl: persistent kernel: %d workgroup(s) per CU x %d CUs (%zu B dynamic LDS), %d needed\n", per_cu, cus, dyn_lds, blocks);
  return (long long)per_cu * cus >= blocks;
}

template <int OCT, int CIT> struct Image { static constexpr int oct = OCT, cit = CIT; };
template <int V> struct Int { static constexpr int value = V; };
template <bool V> struct Flag { static constexpr bool value = V; };
template <class F> static int with_flag(bool b, F&& f) { return b ? f(Flag<true>{}) : f(Flag<false>{}); }

// ---- which instantiation serves a shape.  One function per kernel family, used for the occupancy query and for the launch alike:
// each hands the chosen kernel to `f` and returns what `f` returns.  Together they name exactly the instantiations the library
// ships.  What is not listed (phase timers with a monitor plane, an analytic or a discriminator cost, MINW 2 / 3 outside small +
// granules, <8, 8> outside the multi kernels, a discriminator cost in a batch) does not exist, and the `if constexpr`s keep it that way:
// every instantiation costs compile time.
// the register images <OCT, CIT> (k steps of the policy / cost-net first layers held in registers); CN128: the family has the <8, 8> image
template <bool CN128 = false, class F>
static int with_image(const KernelPick& k, F&& f) {
  k.used_cn128 = false;
  if (k.analytic || k.region) return k.small ? f(Image<2, 0>{}) : f(Image<8, 0>{});
  if (k.small) return f(Image<2, 2>{});
  if constexpr (CN128) {
    if (k.cn128) { k.used_cn128 = true; return f(Image<8, 8>{}); }
  }
  return f(Image<8, 10>{});
}

template <class F> static int with_act_step_kernel(const KernelPick& k, F&& f) {
  return with_image(k, [&](auto im) {
    constexpr int OCT = decltype(im)::oct, CIT = decltype(im)::cit;
    if constexpr (CIT != 0) {
      if (k.disc) return f(act_step_kernel<OCT, CIT | CIT_DISC>);
    } else {
      if (k.region) return f(act_step_kernel<OCT, CIT_REGION>);
    }
    return f(act_step_kernel<OCT, CIT>);
  });
}
template <class F> static int with_host_step_kernel(const KernelPick& k, F&& f) {
  return with_image(k, [&](auto im) {
    constexpr int OCT = decltype(im)::oct, CIT = decltype(im)::cit;
    if constexpr (CIT != 0) {
      if (k.disc) return f(host_step_kernel<OCT, CIT | CIT_DISC>);
    } else {
      if (k.region) return f(host_step_kernel<OCT, CIT_REGION>);
    }
    return f(host_step_kernel<OCT, CIT>);
  });
}
template <class F> static int with_generic_kernel(const KernelPick& k, F&& f) {
  return with_image(k, [&](auto im) {
    constexpr int OCT = decltype(im)::oct, CIT = decltype(im)::cit;
    if constexpr (CIT != 0) {
      if (k.disc) return k.mon ? f(rollout_generic_disc_kernel<OCT, CIT, true>) : f(rollout_generic_disc_kernel<OCT, CIT>);
    }
    return k.mon ? f(rollout_generic_kernel<OCT, CIT, true>) : f(rollout_generic_kernel<OCT, CIT>);
  });
}
template <class F> static int with_persistent_kernel(const KernelPick& k, F&& f) {
  return with_image(k, [&](auto im) { return with_flag(k.gran, [&](auto gran) {
    constexpr int OCT = decltype(im)::oct, CIT = decltype(im)::cit;
    constexpr bool GRAN = decltype(gran)::value;
    if constexpr (CIT != 0) {
      if (k.disc) return k.mon ? f(rollout_persistent_disc_kernel<OCT, CIT, GRAN, true>) : f(rollout_persistent_disc_kernel<OCT, CIT, GRAN>);
    } else {
      if (k.region) return k.mon ? f(rollout_persistent_region_kernel<OCT, GRAN, true>) : f(rollout_persistent_region_kernel<OCT, GRAN>);
    }
    if (k.mon) return f(rollout_persistent_kernel<OCT, CIT, GRAN, false, true>);
    if constexpr (CIT != 0) {
      if (k.prof) return f(rollout_persistent_kernel<OCT, CIT, GRAN, true>);
    }
    return f(rollout_persistent_kernel<OCT, CIT, GRAN>);
  }); });
}
// the gSDE forms: the four images, a constraint net read as 1 - zeta, an analytic cost or none; the one-workgroup-per-env kernel in both exchange modes
template <class F> static int with_act_step_sde_kernel(const KernelPick& k, F&& f) {
  return with_image(k, [&](auto im) { return f(act_step_sde_kernel<decltype(im)::oct, decltype(im)::cit>); });
}
template <class F> static int with_persistent_sde_kernel(const KernelPick& k, F&& f) {
  return with_image(k, [&](auto im) { return with_flag(k.gran, [&](auto gran) {
    return f(rollout_persistent_sde_kernel<decltype(im)::oct, decltype(im)::cit, decltype(gran)::value>);
  }); });
}
template <class F> static int with_wide_kernel(const KernelPick& k, F&& f) {
  return with_image(k, [&](auto im) {
    constexpr int OCT = decltype(im)::oct, CIT = decltype(im)::cit;
    if constexpr (CIT != 0) {
      if (k.disc) return k.mon ? f(rollout_wide_kernel<OCT, CIT | CIT_DISC, false, true>) : f(rollout_wide_kernel<OCT, CIT | CIT_DISC>);
    } else {
      if (k.region) return k.mon ? f(rollout_wide_kernel<OCT, CIT_REGION, false, true>) : f(rollout_wide_kernel<OCT, CIT_REGION>);
    }
    if (k.mon) return f(rollout_wide_kernel<OCT, CIT, false, true>);
    if constexpr (CIT != 0) {
      if (k.prof) return f(rollout_wide_kernel<OCT, CIT, true>);
    }
    return f(rollout_wide_kernel<OCT, CIT>);
  });
}
// registers: the narrow (HC-width) kernel leaves room for several workgroups per CU, so that several runs of the grid are resident
// together: MINW 1 | 2 | 3 with small + granules, 2 with small alone, 1 at the wide widths
template <class F> static int with_persistent_batch_kernel(const KernelPick& k, F&& f) {
  return with_image(k, [&](auto im) { return with_flag(k.mon, [&](auto mon) {
    constexpr int OCT = decltype(im)::oct, CIT = decltype(im)::cit;
    constexpr bool MON = decltype(mon)::value;
    auto kernel = [&](auto gran, auto minw) {      // (the analytic cost: a kernel of its own name, see there)
      constexpr bool GRAN = decltype(gran)::value;
      constexpr int MINW = decltype(minw)::value;
      k.used_minw = MINW;
      if constexpr (CIT == 0) return f(rollout_persistent_batch_analytic_kernel<OCT, GRAN, MINW, MON>);
      else return f(rollout_persistent_batch_kernel<OCT, CIT, GRAN, MINW, MON>);
    };
    if constexpr (OCT == 2) {
      if (!k.gran) return kernel(Flag<false>{}, Int<2>{});
      return k.minw >= 3 ? kernel(Flag<true>{}, Int<3>{}) : (k.minw == 2 ? kernel(Flag<true>{}, Int<2>{}) : kernel(Flag<true>{}, Int<1>{}));
    } else {
      return k.gran ? kernel(Flag<true>{}, Int<1>{}) : kernel(Flag<false>{}, Int<1>{});
    }
  }); });
}
// BATCH: the kernels that read n_runs argument blocks from device memory
template <bool BATCH, class F> static int with_multi_kernel(const KernelPick& k, F&& f) {
  return with_image<true>(k, [&](auto im) { return with_flag(k.mon, [&](auto mon) {
    constexpr int OCT = decltype(im)::oct, CIT = decltype(im)::cit;
    constexpr bool MON = decltype(mon)::value;
    auto kernel = [&](auto e) {      // (the analytic cost: kernels of their own names, see there)
      constexpr int E = decltype(e)::value;
      if constexpr (BATCH && CIT == 0) return f(rollout_multi_batch_analytic_kernel<OCT, E, MON>);
      else if constexpr (BATCH) return f(rollout_multi_batch_kernel<OCT, CIT, E, MON>);
      else if constexpr (CIT == 0) return k.region ? f(rollout_multi_with_a_region_cost_wave_kernel<OCT, E, MON>) : f(rollout_multi_analytic_kernel<OCT, E, MON>);
      else return k.disc ? f(rollout_multi_net_as_discriminator_kernel<OCT, CIT, E, MON>) : f(rollout_multi_kernel<OCT, CIT, E, MON>);
    };
    return k.E == 16 ? kernel(Int<16>{}) : (k.E == 8 ? kernel(Int<8>{}) : kernel(Int<4>{}));
  }); });
}

// ---- launchers.  -1: the grid cannot be co-resident on this device (the caller tries its next route)
static bool xcd_pack() {
  static const bool no_pack = getenv("ICRL_NO_XCD_PACK") != nullptr;
  return !no_pack;
}

// single run, one workgroup per env
template <class K, class A>
static int launch_per_env(K kernel, int N, size_t dyn, hipStream_t s, A& args) {
  if (!persistent_fits(kernel, N, dyn)) return -1;
  const hipError_t e = launch_coresident(kernel, dim3(N), dim3(256), dyn, s, args);
  if (e == hipErrorCooperativeLaunchTooLarge) { (void)hipGetLastError(); return -1; }
  return (int)e;
}

// single run of a multi kernel: G workgroups, or (packed) workgroups 0, 8, 16, ... of 8 (G - 1) + 1 so that all G sit on one XCD
template <class K>
static int launch_multi_run(K kernel, WideArgs& p, int G, size_t dyn, hipStream_t s, int* packed_out) {
  if (!persistent_fits(kernel, G, dyn)) return -1;
  const int packed = xcd_pack() && p.xcc != nullptr && G <= 32;
  *packed_out = packed;
  void* params[] = {(void*)&p, (void*)&packed};
  const hipError_t e = hipLaunchCooperativeKernel((const void*)kernel, dim3(packed ? 8 * (G - 1) + 1 : G), dim3(256), params, (unsigned)dyn, s);
  if (e == hipErrorCooperativeLaunchTooLarge) { (void)hipGetLastError(); return -1; }
  return (int)e;
}

// n_runs runs of a multi kernel, argument blocks in device memory
template <class K>
static int launch_multi_runs(K kernel, const WideArgs* d_args, int n_runs, int G, size_t dyn, hipStream_t s, int* packed_out) {
  if (!persistent_fits(kernel, G, dyn)) return -1;
  // packed layout (a run's G workgroups on ONE XCD: workgroups b, b + 8, ...) when every XCD can hold its share of the grid at once
  // (32 CUs each); otherwise run-major, whose runs become resident oldest first
  int per_cu = 0;
  const int groups = (n_runs + 7) / 8;
  const bool packed = xcd_pack() && G <= 32 && hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, dyn) == hipSuccess && groups * G <= 32 * per_cu;
  *packed_out = packed ? 1 : 0;
  if (packed) hipLaunchKernelGGL(kernel, dim3(8 * G * groups), dim3(256), dyn, s, d_args, n_runs, G, 1);
  else hipLaunchKernelGGL(kernel, dim3(G, n_runs), dim3(256), dyn, s, d_args, n_runs, G, 0);
  return (int)hipGetLastError();
}

// launch_per_env for the gSDE form, which takes a second kernel argument
template <class K>
static int launch_per_env_sde(K kernel, int N, size_t dyn, hipStream_t s, PersistArgs& p, SdeArgs& sd) {
  if (!persistent_fits(kernel, N, dyn)) return -1;
  static const bool plain = getenv("ICRL_PLAIN_LAUNCH") != nullptr;
  hipError_t e;
  if (plain) {
    hipLaunchKernelGGL(kernel, dim3(N), dim3(256), dyn, s, p, sd);
    e = hipGetLastError();
  } else {
    void* params[] = {(void*)&p, (void*)&sd};
    e = hipLaunchCooperativeKernel((const void*)kernel, dim3(N), dim3(256), params, (unsigned)dyn, s);
  }
  if (e == hipErrorCooperativeLaunchTooLarge) { (void)hipGetLastError(); return -1; }
  return (int)e;
}

// ---- what rollout_collect.hip calls (rollout_launch.h)
namespace icrl {
void launch_act_step(const KernelPick& k, int N, hipStream_t s, const ActStepArgs& a, int t) {
  with_act_step_kernel(k, [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(N), dim3(256), 0, s, a, t); return 0; });
}
void launch_act_step_sde(const KernelPick& k, int N, hipStream_t s, const ActStepArgs& a, const SdeArgs& sd, int t) {
  with_act_step_sde_kernel(k, [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(N), dim3(256), 0, s, a, sd, t); return 0; });
}
void launch_act_step_generic(int N, hipStream_t s, const GenStepArgs& g, int t) { hipLaunchKernelGGL(act_step_generic_kernel, dim3(N), dim3(64), 0, s, g, t); }
int launch_rollout_generic(const KernelPick& k, int N, size_t dyn, hipStream_t s, GenRolloutArgs& ga) {
  return with_generic_kernel(k, [&](auto kernel) { return launch_per_env(kernel, N, dyn, s, ga); });
}
int launch_rollout_persistent(const KernelPick& k, int N, size_t dyn, hipStream_t s, PersistArgs& p) {
  return with_persistent_kernel(k, [&](auto kernel) { return launch_per_env(kernel, N, dyn, s, p); });
}
int launch_rollout_persistent_sde(const KernelPick& k, int N, size_t dyn, hipStream_t s, PersistArgs& p, SdeArgs& sd) {
  return with_persistent_sde_kernel(k, [&](auto kernel) { return launch_per_env_sde(kernel, N, dyn, s, p, sd); });
}
int launch_rollout_persistent_batch(const KernelPick& k, int N, int n_runs, size_t dyn, hipStream_t s, const PersistArgs* d_args) {
  return with_persistent_batch_kernel(k, [&](auto kernel) -> int {
    if (!persistent_fits(kernel, N, dyn)) return fail("icrl_rollout_collect_batch: the %d workgroups of one run do not fit the device", N);
    hipLaunchKernelGGL(kernel, dim3(N, n_runs), dim3(256), dyn, s, d_args);
    return (int)hipGetLastError();
  });
}
int rollout_wide_blocks_per_cu(const KernelPick& k, int* per_cu) {
  return with_wide_kernel(k, [&](auto kernel) { return (int)hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, (const void*)kernel, 256, 0); });
}
int launch_rollout_wide(const KernelPick& k, int G, hipStream_t s, WideArgs& p) {
  return with_wide_kernel(k, [&](auto kernel) { return (int)launch_coresident(kernel, dim3(G), dim3(256), 0, s, p); });
}
int launch_rollout_multi(const KernelPick& k, WideArgs& p, int G, size_t dyn, hipStream_t s, int* packed_out) {
  return with_multi_kernel<false>(k, [&](auto kernel) { return launch_multi_run(kernel, p, G, dyn, s, packed_out); });
}
int launch_rollout_multi_batch(const KernelPick& k, const WideArgs* d_args, int n_runs, int G, size_t dyn, hipStream_t s, int* packed_out) {
  return with_multi_kernel<true>(k, [&](auto kernel) { return launch_multi_runs(kernel, d_args, n_runs, G, dyn, s, packed_out); });
}
int put_rollout_args(const PersistArgs& p, PersistArgs* dst, hipStream_t s) { return put_args(p, dst, s); }
int put_rollout_args(const WideArgs& p, WideArgs* dst, hipStream_t s) { return put_args(p, dst, s); }
}  // namespace icrl

// ---- rollout over host envs: one launch per env step (host_step_kernel) ----
extern "C" size_t icrl_host_step_ws_bytes(int N, int obs_dim) {
  return N < 1 || obs_dim < 1 ? 0 : 2 * host_copy_doubles(N, obs_dim) * sizeof(double);
}

extern "C" int icrl_host_step_mon(const icrl_norm_t* nm, const icrl_policy_t* pol, const icrl_costnet_t* cn, const icrl_buffer_t* buf,
                                  const icrl_agent_t* ag, const icrl_host_step_t* hs, const float* noise, const float* action_low,
                                  const float* action_high, int k, const icrl_monitor_t* mon, void* stream) {
  double* raw_plane = nullptr;
  if (int e = mon_plane("icrl_host_step_mon", mon, &raw_plane)) return e;
  if (nm == nullptr || pol == nullptr || buf == nullptr || ag == nullptr || hs == nullptr) return fail("icrl_host_step: NULL descriptor");
  const int N = buf->N, O = buf->obs_dim, T = hs->T;
  if (policy_is_wide(pol) || !dims_ok(pol)) return bad_dims("icrl_host_step", pol);
  const icrl_cost_fn_t* const cf = as_cost_fn(cn);
  if (cf != nullptr) {
    if (int e = cost_fn_check("icrl_host_step", cf, O, pol->discrete ? 0 : pol->act_dim, pol->discrete ? 1 : 0)) return e;
  }
  const icrl_cost_disc_t* const cd = as_cost_disc(cn);
  if (cd != nullptr)
    if (int e = cost_disc_check("icrl_host_step", cd)) return e;
  const icrl_cost_region_t* const cr = as_cost_region(cn);
  if (cr != nullptr)
    if (int e = cost_region_check("icrl_host_step", cr, O, pol->discrete ? 0 : pol->act_dim, pol->discrete ? 1 : 0)) return e;
  const icrl_costnet_t* const net = (cf != nullptr || cr != nullptr) ? nullptr : (cd != nullptr ? cd->net : cn);      // the constraint net proper
  if (net != nullptr && (costnet_is_wide(net) || !cn_ok(net))) return bad_cn("icrl_host_step", net);
  if (N < 1 || N > 128 || O < 1 || O > MAX_OBS || pol->obs_dim != O)
    return fail("icrl_host_step: %d envs (1..128), obs_dim %d (1..%d), policy obs_dim %d: other shapes take the per-step loop", N, O, MAX_OBS, pol->obs_dim);
  if (!nm->training) return fail("icrl_host_step: the normaliser is not training (statistics frozen): the per-step loop serves that");
  if (T < 1 || buf->T != T || k < 0 || k > T) return fail("icrl_host_step: launch k = %d of T = %d (buffer T = %d)", k, T, buf->T);
  if (buf->act_store != (pol->discrete ? 1 : pol->act_dim)) return fail("icrl_host_step: buffer act_store %d vs policy act_dim %d", buf->act_store, pol->act_dim);
  if (hs->stage == nullptr || hs->s == nullptr || hs->act_host == nullptr || hs->ws == nullptr || pol->params_t == nullptr || (k < T && noise == nullptr) ||
      (size_t)hs->ws_bytes < icrl_host_step_ws_bytes(N, O))
    return fail("icrl_host_step: staging / raw-obs / action / workspace pointers, transposed policy, noise and %zu workspace bytes are required (got %lld)",
                icrl_host_step_ws_bytes(N, O), hs->ws_bytes);
  HostStepArgs h{};
  ActStepArgs& a = h.act;
  a.env.n_envs = N; a.env.obs_dim = O; a.env.act_dim = pol->discrete ? 1 : pol->act_dim;
  fill_act_args(a, nullptr, buf, ag, pol, false, net, cf, noise, action_low, action_high, raw_plane);
  if (cr != nullptr) { a.cr = *cr; a.has_cn = 1; }
  h.nm = *nm; h.hs = *hs; h.N = N;
  // act_host is a HOST address (a pinned allocation or a registered host range): the kernel stores through the device's mapping of it
  void* act_dev = nullptr;
  if (hipHostGetDevicePointer(&act_dev, hs->act_host, 0) != hipSuccess || act_dev == nullptr) {
    (void)hipGetLastError();
    return fail("icrl_host_step: act_host %p is not page-locked host memory mapped for the device (hipHostMalloc / hipHostRegister)", (void*)hs->act_host);
  }
  h.hs.act_host = reinterpret_cast<float*>(act_dev);
  hipStream_t s = (hipStream_t)stream;
  KernelPick pick;
  pick.small = small_shape(O, net); pick.analytic = cf != nullptr; pick.disc = cd != nullptr; pick.region = cr != nullptr;
  with_host_step_kernel(pick, [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(N), dim3(256), 0, s, h, k); return 0; });
  return (int)hipGetLastError();
}

extern "C" int icrl_host_step(const icrl_norm_t* nm, const icrl_policy_t* pol, const icrl_costnet_t* cn, const icrl_buffer_t* buf,
                              const icrl_agent_t* ag, const icrl_host_step_t* hs, const float* noise, const float* action_low,
                              const float* action_high, int k, void* stream) {
  return icrl_host_step_mon(nm, pol, cn, buf, ag, hs, noise, action_low, action_high, k, nullptr, stream);
}

// ---- sampling / evaluation episodes over one host env: one launch per env step (host_episode_kernel) ----
extern "C" int icrl_host_episode_step(const icrl_norm_t* nm, const icrl_policy_t* pol, const icrl_host_episode_t* he, const float* noise,
                                      const float* action_low, const float* action_high, int k, int act, void* stream) {
  if (nm == nullptr || pol == nullptr || he == nullptr) return fail("icrl_host_episode_step: NULL descriptor");
  const int O = he->obs_dim, rows = he->rows;
  if (policy_is_wide(pol) || !dims_ok(pol)) return bad_dims("icrl_host_episode_step", pol);
  if (he->num_envs != 1 || O < 1 || O > MAX_OBS || pol->obs_dim != O)
    return fail("icrl_host_episode_step: %d envs (1), obs_dim %d (1..%d), policy obs_dim %d: other shapes take the per-step loop", he->num_envs, O, MAX_OBS, pol->obs_dim);
  if (nm->training) return fail("icrl_host_episode_step: the normaliser must be frozen (training = %d)", nm->training);
  if (rows < 1 || k < 0 || k > rows || (act && k == rows)) return fail("icrl_host_episode_step: launch k = %d (act = %d) of %d rows", k, act, rows);
  if (he->stage == nullptr || he->act_host == nullptr || he->orig_obs == nullptr || he->obs == nullptr || he->actions == nullptr || pol->params_t == nullptr)
    return fail("icrl_host_episode_step: staging / action / output pointers and the transposed policy are required");
  HostEpisodeArgs h{};
  h.nm = *nm; h.he = *he;
  h.pl = make_pol_layout(pol->obs_dim, pol->act_dim, pol->h1, pol->h2, pol->discrete);
  h.PT = pol->params_t; h.noise = noise; h.alow = action_low; h.ahigh = action_high;
  // act_host is a HOST address (a pinned allocation or a registered host range): the kernel stores through the device's mapping of it
  void* act_dev = nullptr;
  if (hipHostGetDevicePointer(&act_dev, he->act_host, 0) != hipSuccess || act_dev == nullptr) {
    (void)hipGetLastError();
    return fail("icrl_host_episode_step: act_host %p is not page-locked host memory mapped for the device (hipHostMalloc / hipHostRegister)", (void*)he->act_host);
  }
  h.he.act_host = reinterpret_cast<float*>(act_dev);
  hipStream_t s = (hipStream_t)stream;
  // (host_step_kernel's <2, 2> / <8, 10> split by observation width; its second parameter sizes the cost wave, which is absent here)
  if (h.pl.O <= 32) hipLaunchKernelGGL(host_episode_kernel<2>, dim3(1), dim3(256), 0, s, h, k, act);
  else hipLaunchKernelGGL(host_episode_kernel<8>, dim3(1), dim3(256), 0, s, h, k, act);
  return (int)hipGetLastError();
}
