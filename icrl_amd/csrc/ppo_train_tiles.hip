// PPO-Lagrangian update as ONE persistent launch, the column-split tiles kernel — gfx950.  One body for three policy heads: diagonal
// Gaussian, Categorical (icrl_ppo_lag_train with hp._pad & 2, csrc/ppo_train.hip) and gSDE (icrl_ppo_lag_train_sde, csrc/ppo_train_sde.hip).
//
// ref: stable_baselines3/ppo_lag/ppo_lag.py:196-299 (epoch / minibatch loop of PPOLagrangian.train),
//      common/buffers.py:594-627 (get / _get_samples), common/policies.py:752-767 (evaluate_actions),
//      common/distributions.py:143-171 (DiagGaussian log_prob / entropy), :274-288 (Categorical), :408-601
//      (StateDependentNoiseDistribution with full_std, exp, no squashing, learn_features = False), torch.optim.Adam, clip_grad_norm_.
//
// The reference performs n_epochs * ceil(T*N / batch) DEPENDENT optimiser steps on a 64..128-row minibatch through three
// small independent MLPs (pi, vf, cvf: obs -> 64 -> 64 -> {act | 1 | 1}).  Parity forbids re-ordering or merging those
// steps, so the step latency is what matters.  Mapping:
//
//   * grid = 3 workgroups x 512 threads: workgroup r owns network r.  The only quantity coupling the networks inside a
//     step is the global gradient norm (clip_grad_norm_ over ALL policy parameters): each workgroup publishes its partial
//     sum of squares as an 8-byte {step tag, value} granule (agent-scope relaxed store) and polls the other two (guide:
//     cdna_hip_programming.md §6 Guideline 16, form R2 — the datum is the flag).  Granule slots are double-buffered by step
//     parity; a workgroup can never be more than one step ahead of the others.  While the granules are in flight the
//     workgroup already stages the NEXT minibatch (LDS commit + advantage statistics).
//   * 8 waves = 2 per SIMD: wave (rt, hf) owns row tile rt (16 of the chunk's 64 rows) and column half hf of every 64-wide
//     GEMM output, so while one wave of a SIMD runs its VALU epilogue / LDS traffic the other one feeds the matrix core.
//   * the network's weights stay in LDS for the whole launch (fp32 master copy); Adam moments and the accumulating weight
//     gradients stay in REGISTERS in MFMA C-layout: the lane that receives dW[j][k] from the matrix core owns m, v and the
//     update of W[j][k].  Inside the loop only the gathered minibatch rows (prefetched one chunk ahead into registers,
//     their permutation indices two chunks ahead) and the 3 granules touch global memory.
//   * all eight GEMMs of a step (3 forward, 5 backward) run on v_mfma_f32_16x16x4_f32 (exact fp32 FMA chains).  K is
//     enumerated as k = 16*js + 4*(lane/16) + e: an operand whose K runs along the LDS row is fetched with ONE ds_read_b128
//     per four MFMA steps, conflict-free at row strides = 8 mod 16 floats; operands whose K runs across rows use
//     ds_read_b32.  Every GEMM first stages its operands in registers, then issues its MFMAs back to back.
//   * minibatches larger than 64 rows are processed in 64-row chunks that accumulate into the same gradient registers.
//
// The gSDE head (HEAD_SDE) replaces the diagonal head in the policy workgroup; the two critics' workgroups run the same code under every
// head.  The head (csrc/sde.hip's header, the float64 SDE form of mlp_fwd_bwd_kernel in csrc/mlp_grad.hip):
//
//   parameters  log_std [64, A] first in the flat buffer (common.h: make_sde_layout), rows beyond the last hidden width zero.  Wave (rt, 1) of
//               the policy workgroup owns log_std[16 rt + lane % 16][4 (lane / 16) + i] — parameter, both Adam moments and the gradient — in
//               registers, in the C-layout in which the matrix core delivers its gradient; wave (rt, 0) owns the head weights as under the
//               other heads (whose log_std [A] is owned by threads 144..159 instead).
//   forward     mean = Wa . h2 + ba on the hf = 0 wave of every row tile, as under the other heads; beside it the hf = 1 wave computes
//               var[b][a] = sum_h h2[b][h]^2 E2[h][a] + 1e-6 as a second head GEMM on v_mfma_f32_16x16x4_f32: the A operand is h2 squared in
//               registers as it is staged, the B operand the LDS image E2T[a][h] = exp(2 log_std[h][a]) (laid out like the head weights, so the
//               same ds_read_b128 fetch).  Its owners rewrite the image after every Adam step.
//   loss        Normal(mean, sqrt(var)) per row and action: log_prob = sum_a -(x - mean)^2 / (2 var) - log(var) / 2 - log sqrt(2 pi),
//               entropy = sum_a 1/2 + log(2 pi) / 2 + log(var) / 2 — per ROW, so the entropy bonus is a mean over the minibatch.
//   backward    d mean = dlp (x - mean) / var;  d var = dlp ((x - mean)^2 / var - 1) / (2 var) + dent / (2 var)   (dent = -ent_coef / rows);
//               d log_std[h][a] = 2 E2[h][a] sum_b d var[b][a] h2[b][h]^2: a GEMM of the shape of the head-weight gradient, on the hf = 1
//               waves while the hf = 0 waves run that one.  The latent is detached in the variance: d h2 receives the mean path only.
//   padding     a padded latent unit is exactly 0, so is its square, its log_std gradient and (g = m = v = 0) its Adam update.
//
// gSDE serves obs <= 128 (two, four or eight 16-column tiles), continuous actions, minibatches of up to 128 rows.  LDS: the exp(2 log_std)
// image is the one addition (4.5 KB); the per-row variances and their gradients live in spare columns of the dz2 rows, which is why the two
// head-gradient GEMMs then run in front of the stage that writes dz2 (one barrier more per chunk than under the other heads).  obs 65..128
// then takes 161 920 of the workgroup's 163 840 bytes, and the kernel is built for one workgroup per compute unit (the other heads: two).
//
// Built with -ffp-contract=off; FMA is used only where written (fmaf / MFMA).
#include "ppo_common.h"

namespace icrl {

constexpr int TH = 512;  // threads per workgroup (8 waves, 2 per SIMD)
constexpr int SO = 24;   // LDS row stride of 16-wide matrices

template <int NT1, int HEAD>
struct Smem {  // offsets in floats (all multiples of 4: 16-byte aligned rows); an image a head does not have is empty
  static constexpr bool SDE = HEAD == HEAD_SDE;
  static constexpr int O16 = 16 * NT1, SX = O16 + 8;
  static constexpr int W1 = 0;
  static constexpr int W2 = W1 + HD * SX;
  static constexpr int WH = W2 + HD * SH;
  static constexpr int E2T = WH + 16 * SH;    // gSDE: [16][SH] exp(2 log_std[h][a]) at a * SH + h (policy workgroup)
  static constexpr int B1 = E2T + (SDE ? 16 * SH : 0);
  static constexpr int B2 = B1 + HD;
  static constexpr int BH = B2 + HD;
  static constexpr int LS = BH + 16;          // not gSDE: [16] log_std
  static constexpr int X = LS + (SDE ? 0 : 16);
  static constexpr int H1 = X + RB * SX;
  static constexpr int H2 = H1 + RB * SH;     // h2, later dz1
  static constexpr int DZ = H2 + RB * SH;     // dz2; before the backward its rows hold the chunk's actions / scalars
  static constexpr int DO = DZ + RB * SH;     // head output, overwritten (after a barrier) by d loss / d output
  static constexpr int RED1 = DO + RB * SO;   // [4][64] per-row-tile column sums of dz1
  static constexpr int RED2 = RED1 + 4 * HD;  // [4][64] per-row-tile column sums of dz2
  static constexpr int PBH = RED2 + 4 * HD;   // [4][16] per-row-tile column sums of dOut
  static constexpr int PLS = PBH + 64;        // not gSDE: [4][16] per-row-tile d log_std partials
  static constexpr int PST = PLS + (SDE ? 0 : 64);   // [4][8] per-row-tile loss statistics
  static constexpr int MISC = PST + 32;       // [48] block-reduction scratch + broadcast scalars
  static constexpr int GAU = MISC + 48;       // not gSDE: [3][16] per-action 1/var, 0.5/var, log(sd) + log(sqrt(2 pi))
  static constexpr int TOTAL = GAU + (SDE ? 0 : 48);
  // per-row side data of the chunk lives in the (not yet used) dz rows: columns 0..15 actions, 16 old log-prob | old value,
  // 17 raw reward advantage | return, 18 raw cost advantage; gSDE: columns 24..39 (policy) the row's variances, overwritten (after the
  // barrier that also frees the head outputs) by d loss / d variance, which the log_std GEMM consumes BEFORE dz2 is written over the rows
  static constexpr int ACT = DZ, OLP = DZ + 16, ADR = DZ + 17, ADC = DZ + 18, VR = DZ + 24;
};

// Two __global__ shells around ONE body text (ppo_train_tiles_body.h: the statements of the kernel, written against NT1, HEAD and the
// argument block `a`).  The diagonal and Categorical heads leave room for two workgroups per compute unit; the gSDE head's registers
// (log_std, its moments and gradient beside the head weights') are budgeted for one, so the two launch bounds differ.  The body is
// included, not called: a __forceinline__ body under thin wrappers (the form of ppo_train_quarters2.hip) is simplified as a function of
// its own before it is inlined, and that alone changed the schedule of every instantiation (DESIGN.md §24's note of 2026-10-20).
template <int NT1, int HEAD>
__global__ void __launch_bounds__(TH, 2) ppo_train_tiles_kernel(TrainArgs a) {
  static_assert(HEAD == HEAD_GAUSS || HEAD == HEAD_CAT, "the gSDE head: ppo_train_tiles_sde_kernel");
#include "ppo_train_tiles_body.h"
}

template <int NT1>
__global__ void __launch_bounds__(TH) ppo_train_tiles_sde_kernel(TrainArgs a) {
  constexpr int HEAD = HEAD_SDE;
#include "ppo_train_tiles_body.h"
}

}  // namespace icrl

using namespace icrl;

template <int NT1, int HEAD>
static int launch_tiles(const TrainArgs& a, hipStream_t s) {
  static_assert(Smem<NT1, HEAD>::TOTAL * sizeof(float) <= 160 * 1024, "LDS budget");
  const size_t bytes = (size_t)Smem<NT1, HEAD>::TOTAL * sizeof(float);
  void (*kernel)(TrainArgs);
  if constexpr (HEAD == HEAD_SDE) kernel = ppo_train_tiles_sde_kernel<NT1>;
  else kernel = ppo_train_tiles_kernel<NT1, HEAD>;
  hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) return (int)e;
  TrainArgs arg = a;
  return (int)launch_coresident(kernel, dim3(3), dim3(TH), bytes, s, arg);
}

template <int HEAD>
static int launch_tiles_nt1(const TrainArgs& a, int nt1, hipStream_t s) {
  if (nt1 <= 2) return launch_tiles<2, HEAD>(a, s);
  if (nt1 <= 4) return launch_tiles<4, HEAD>(a, s);
  return launch_tiles<8, HEAD>(a, s);
}

int icrl::launch_train_tiles(const TrainArgs& a, int nt1, int head, hipStream_t s, int* packed) {
  *packed = 0;      // (three workgroups, no packed form)
  if (head == HEAD_SDE) return launch_tiles_nt1<HEAD_SDE>(a, nt1, s);
  return head == HEAD_CAT ? launch_tiles_nt1<HEAD_CAT>(a, nt1, s) : launch_tiles_nt1<HEAD_GAUSS>(a, nt1, s);
}
