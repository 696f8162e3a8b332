// One full-batch regression step of MLP(in -> h1 -> ReLU -> h2 -> ReLU -> out) with an MSE loss and Adam — gfx950.
//
// The rollout-end work of the reference's exploration callbacks (icrl/exploration.py:50-67, 227-261, 291-317): a small predictor /
// cost network takes ONE optimiser step on all T x N rows of the rollout buffer, and the per-row squared error of the PRE-step
// prediction is the exploration reward.  icrl_reg_mlp_step is that step on a flat float32 parameter buffer in torch's state_dict
// order (W1 [h1, in], b1, W2 [h2, h1], b2, W3 [out, h2], b3), reading the buffer's observation and action planes as one
// concatenated row (no torch.cat copy); icrl_shape_advantages is `cost_advantages /= 1 + exploration_reward`.
//
// Three plain launches, no cooperative launch, no waiting between workgroups, no float atomics:
//   1. reg_mlp_tile_kernel: a workgroup (8 waves) owns the 32-row groups grp = blockIdx.x, += gridDim.x.  The weights sit in LDS for the
//      whole launch, zero-padded to the MFMA granule (16 output units, 4 inputs) — the padding lives in LDS and registers only.  The
//      FORWARD pass, the errors and their row sums are float64 (v_mfma_f64_16x16x4_f64 on the float32 parameters and inputs, hidden
//      activations kept as float64 images): row_err, the loss and the statistics are the float64 values rounded once, as the siblings
//      of mlp_grad.hip give them.  The BACKWARD products are v_mfma_f32_16x16x4_f32 (exact float32, the reference's precision) on
//      the float32 roundings of the errors and activations.  All of them work on TRANSPOSED activations: a layer is
//      out^T [F x rows] = W [F x K] . in^T [K x rows], whose result layout (lane = row, registers = 4 consecutive units) is stored
//      to the [unit][row] image the next layer's B operand, the weight-gradient products (K = the 32 rows) and the bias sums read.
//      Weight-gradient tiles are owned by waves and stay in REGISTERS across all groups of the workgroup (a group's 32-row product is
//      a float32 tile, the sum over the groups and the bias sums are float64); at the end the workgroup writes its sums of the REAL
//      entries, rounded once, to its own slice of ws, and its float64 sums of row_err and row_err^2.
//   2. reg_mlp_adam_kernel: per parameter, the slices are added in index order in float64, scaled by 2 / (rows * out), rounded once,
//      and torch's single-tensor Adam is applied, operation by operation as torch rounds.
//   3. reg_mlp_stats_kernel: the statistics sums are added in index order -> out4; *adam_step += 1.
// The grid is a function of rows alone and every sum has a fixed order: a call is deterministic bit for bit.
#include "common.h"

namespace icrl {
namespace {

typedef float v4f __attribute__((ext_vector_type(4)));
typedef double v4d __attribute__((ext_vector_type(4)));

constexpr int RM_THREADS = 512;
constexpr int RM_WAVES = RM_THREADS / 64;
constexpr int RM_ROWS = 32;          // rows of a group: two MFMA row tiles
constexpr int RM_SR = 34;            // row stride (floats) of the float32 [unit][row] images (inputs, upstream gradients)
constexpr int RM_SRD = 33;           // row stride (doubles) of the float64 [unit][row] images of the hidden activations
constexpr int RM_MAX_WG = 256;
constexpr int RM_MAX_H = 64, RM_MAX_INA = 128, RM_MAX_INB = 16, RM_MAX_OUT = 128;
constexpr int RM_MAX_ROWS = 1 << 21;
constexpr int RM_STAT_DOUBLES = 2 * RM_MAX_WG;      // head of ws: {sum row_err, sum row_err^2} per workgroup
// weight-gradient tiles (16 x 16) a wave owns at most: dW3 8 x 4, dW2 4 x 4, dW1 4 x 9 over 8 waves
constexpr int RM_T3 = 4, RM_T2 = 2, RM_T1 = 5;

struct RmDims {
  int in_a, in_b, in, h1, h2, out;
  int inp4, inp16, h1p, h2p, outp;     // in rounded up to 4 (the K step) and 16 (a tile of dW1 columns); widths rounded up to 16
  int sw1, sw2, sw3;                   // row strides of the weight images
  int oW1, ob1, oW2, ob2, oW3, ob3, np;
  int lW1, lW2, lW3, lb1, lb2, lb3, lX, lH1, lH2, lD, lRed, lds_floats;
};

// a stride of 2 mod 4 floats: the 16 units of an A-operand read start on 16 different even banks, their 4 inputs beside them
inline int rm_wstride(int K) { return ((K + 3) & ~3) + 2; }

inline RmDims rm_dims(int in_a, int in_b, int h1, int h2, int out) {
  RmDims d;
  d.in_a = in_a; d.in_b = in_b; d.in = in_a + in_b; d.h1 = h1; d.h2 = h2; d.out = out;
  d.inp4 = (d.in + 3) & ~3; d.inp16 = (d.in + 15) & ~15;
  d.h1p = (h1 + 15) & ~15; d.h2p = (h2 + 15) & ~15; d.outp = (out + 15) & ~15;
  d.sw1 = rm_wstride(d.inp4); d.sw2 = rm_wstride(d.h1p); d.sw3 = rm_wstride(d.h2p);
  d.oW1 = 0; d.ob1 = d.oW1 + h1 * d.in; d.oW2 = d.ob1 + h1; d.ob2 = d.oW2 + h2 * h1; d.oW3 = d.ob2 + h2; d.ob3 = d.oW3 + out * h2;
  d.np = d.ob3 + out;
  int o = 0;
  d.lW1 = o; o += d.h1p * d.sw1;
  d.lW2 = o; o += d.h2p * d.sw2;
  d.lW3 = o; o += d.outp * d.sw3;
  d.lb1 = o; o += d.h1p;
  d.lb2 = o; o += d.h2p;
  d.lb3 = o; o += d.outp;
  d.lX = o; o += d.inp16 * RM_SR;
  o = (o + 1) & ~1;                    // the hidden activations are doubles
  d.lH1 = o; o += 2 * d.h1p * RM_SRD;
  d.lH2 = o; o += 2 * d.h2p * RM_SRD;
  int dmax = d.outp > d.h1p ? d.outp : d.h1p;
  if (d.h2p > dmax) dmax = d.h2p;
  d.lD = o; o += dmax * RM_SR;
  o = (o + 1) & ~1;                    // 8 unit tiles x 32 rows of float64 partial row errors; 64 doubles at the end
  d.lRed = o; o += 16 * RM_ROWS;
  d.lds_floats = o;
  return d;
}

inline int rm_grid(int rows) {
  const int groups = (rows + RM_ROWS - 1) / RM_ROWS;
  return groups < RM_MAX_WG ? groups : RM_MAX_WG;
}

struct RmArgs {
  RmDims d;
  const float* params;
  const float* xa;
  const float* xb;
  const float* target;
  float* row_err;
  int rows;
  double* stats;      // [gridDim.x][2]
  float* part;        // [gridDim.x][np]
};

// acc += A [16 x 4 ksteps] . B [4 ksteps x 16]: A(f, k) at A[f * fa + k * ka], B(k, n) at B[k * kb + n * nb]; lane (g = lane >> 4, i = lane & 15)
// feeds A(i, 4 kk + g) and B(4 kk + g, i) and receives rows 4 g + r, column i in register r.  B may be a float64 image (rounded on the read).
template <class TB>
__device__ __forceinline__ v4f rm_tile(const float* A, int fa, int ka, const TB* B, int kb, int nb, int ksteps, int g, int i, v4f acc) {
  const float* pa = A + i * fa + g * ka;
  const TB* pb = B + g * kb + i * nb;
  const int sa = 4 * ka, sb = 4 * kb;
  // two chains, even and odd K steps: a dependent v_mfma_f32_16x16x4_f32 waits 40 cycles where an independent one issues after 32, and each
  // chain rounds half as often
  v4f odd = {0.f, 0.f, 0.f, 0.f};
  int kk = 0;
  for (; kk + 1 < ksteps; kk += 2) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[kk * sa], (float)pb[kk * sb], acc, 0, 0, 0);
    odd = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[(kk + 1) * sa], (float)pb[(kk + 1) * sb], odd, 0, 0, 0);
  }
  if (kk < ksteps) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[kk * sa], (float)pb[kk * sb], acc, 0, 0, 0);
  return acc + odd;
}

// the same product in float64 (v_mfma_f64_16x16x4_f64) for the forward pass: the operands are fed as above, the result has ANOTHER layout:
// rows g + 4 r, column i in register r
template <class TB>
__device__ __forceinline__ v4d rm_tile_d(const float* A, int fa, int ka, const TB* B, int kb, int nb, int ksteps, int g, int i) {
  const float* pa = A + i * fa + g * ka;
  const TB* pb = B + g * kb + i * nb;
  const int sa = 4 * ka, sb = 4 * kb;
  v4d acc = {0., 0., 0., 0.}, odd = {0., 0., 0., 0.};
  int kk = 0;
  for (; kk + 1 < ksteps; kk += 2) {
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64((double)pa[kk * sa], (double)pb[kk * sb], acc, 0, 0, 0);
    odd = __builtin_amdgcn_mfma_f64_16x16x4f64((double)pa[(kk + 1) * sa], (double)pb[(kk + 1) * sb], odd, 0, 0, 0);
  }
  if (kk < ksteps) acc = __builtin_amdgcn_mfma_f64_16x16x4f64((double)pa[kk * sa], (double)pb[kk * sb], acc, 0, 0, 0);
  return acc + odd;
}

__global__ void __launch_bounds__(RM_THREADS) reg_mlp_tile_kernel(RmArgs a) {
  extern __shared__ float lds[];
  const RmDims& d = a.d;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, g = lane >> 4, i = lane & 15;
  float *sW1 = lds + d.lW1, *sW2 = lds + d.lW2, *sW3 = lds + d.lW3, *sb1 = lds + d.lb1, *sb2 = lds + d.lb2, *sb3 = lds + d.lb3;
  float *sX = lds + d.lX, *sD = lds + d.lD;
  double *sH1 = reinterpret_cast<double*>(lds + d.lH1), *sH2 = reinterpret_cast<double*>(lds + d.lH2), *sRed = reinterpret_cast<double*>(lds + d.lRed);
  const int SR = RM_SR, SRD = RM_SRD;

  // ---- the zero-padded images of the parameters
  for (int k = tid; k < d.lds_floats; k += RM_THREADS) lds[k] = 0.f;
  __syncthreads();
  for (int e = tid; e < d.h1 * d.in; e += RM_THREADS) { const int f = e / d.in; sW1[f * d.sw1 + (e - f * d.in)] = a.params[d.oW1 + e]; }
  for (int e = tid; e < d.h2 * d.h1; e += RM_THREADS) { const int f = e / d.h1; sW2[f * d.sw2 + (e - f * d.h1)] = a.params[d.oW2 + e]; }
  for (int e = tid; e < d.out * d.h2; e += RM_THREADS) { const int f = e / d.h2; sW3[f * d.sw3 + (e - f * d.h2)] = a.params[d.oW3 + e]; }
  if (tid < d.h1) sb1[tid] = a.params[d.ob1 + tid];
  if (tid < d.h2) sb2[tid] = a.params[d.ob2 + tid];
  if (tid < d.out) sb3[tid] = a.params[d.ob3 + tid];
  __syncthreads();

  const int n1f = d.h1p >> 4, n2f = d.h2p >> 4, n3f = d.outp >> 4, n1n = d.inp16 >> 4;
  const int nt3 = n3f * n2f, nt2 = n2f * n1f, nt1 = n1f * n1n;
  const v4f zero4 = {0.f, 0.f, 0.f, 0.f};
  // weight gradients: a group's 32-row product is float32 (one MFMA tile), the sum over the workgroup's groups float64
  const v4d zero4d = {0., 0., 0., 0.};
  v4d acc3[RM_T3], acc2[RM_T2], acc1[RM_T1];
#pragma unroll
  for (int s = 0; s < RM_T3; ++s) acc3[s] = zero4d;
#pragma unroll
  for (int s = 0; s < RM_T2; ++s) acc2[s] = zero4d;
#pragma unroll
  for (int s = 0; s < RM_T1; ++s) acc1[s] = zero4d;
  double db3 = 0., db2 = 0., db1 = 0.;      // bias gradients: plain sums over all rows of the workgroup, kept in float64
  double sE = 0., sE2 = 0.;

  const int groups = (a.rows + RM_ROWS - 1) / RM_ROWS;
  // a hidden layer is at most 4 unit tiles x 2 row tiles = one job per wave; the output layer at most 8 x 2 = two
  const int hft = wv >> 1, hrt = wv & 1;
  for (int grp = blockIdx.x; grp < groups; grp += gridDim.x) {
    const int row0 = grp * RM_ROWS;
    const int nvalid = a.rows - row0 < RM_ROWS ? a.rows - row0 : RM_ROWS;

    // ---- the group's inputs -> sX [input][row]; rows past the end are zeros
    if (d.in_a > 0) {
      const float* src = a.xa + (size_t)row0 * d.in_a;
      for (int e = tid; e < RM_ROWS * d.in_a; e += RM_THREADS) {
        const int r = e / d.in_a, c = e - r * d.in_a;
        sX[c * SR + r] = r < nvalid ? src[e] : 0.f;
      }
    }
    {
      const float* src = a.xb + (size_t)row0 * d.in_b;
      for (int e = tid; e < RM_ROWS * d.in_b; e += RM_THREADS) {
        const int r = e / d.in_b, c = e - r * d.in_b;
        sX[(d.in_a + c) * SR + r] = r < nvalid ? src[e] : 0.f;
      }
    }
    __syncthreads();

    // ---- forward, in float64 on the float32 parameters and inputs (the hidden activations stay float64 between the layers)
    if (hft < n1f) {
      const v4d z = rm_tile_d(sW1 + hft * 16 * d.sw1, d.sw1, 1, sX + hrt * 16, SR, 1, d.inp4 >> 2, g, i);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = hft * 16 + g + 4 * r;
        const double h = z[r] + (double)sb1[f];
        sH1[f * SRD + hrt * 16 + i] = h > 0. ? h : 0.;
      }
    }
    __syncthreads();
    if (hft < n2f) {
      const v4d z = rm_tile_d(sW2 + hft * 16 * d.sw2, d.sw2, 1, sH1 + hrt * 16, SRD, 1, d.h1p >> 2, g, i);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = hft * 16 + g + 4 * r;
        const double h = z[r] + (double)sb2[f];
        sH2[f * SRD + hrt * 16 + i] = h > 0. ? h : 0.;
      }
    }
    __syncthreads();
    // output layer: the error per element, its float32 rounding -> sD (what the backward pass reads), its square summed per row in float64:
    // the lane's four units, then the four lane groups of the tile -> sRed [unit tile][row]
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int job = wv + RM_WAVES * s, ft = job >> 1, rt = job & 1;
      if (ft < n3f) {
        const v4d z = rm_tile_d(sW3 + ft * 16 * d.sw3, d.sw3, 1, sH2 + rt * 16, SRD, 1, d.h2p >> 2, g, i);
        const int row = rt * 16 + i;
        double e = 0.;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int f = ft * 16 + g + 4 * r;
          double diff = 0.;      // padded units and rows past the end: no error, no gradient
          if (f < d.out && row < nvalid) diff = (z[r] + (double)sb3[f]) - (double)a.target[(size_t)(row0 + row) * d.out + f];
          sD[f * SR + row] = (float)diff;
          e += diff * diff;
        }
        e += __shfl_xor(e, 16);
        e += __shfl_xor(e, 32);
        if (g == 0) sRed[ft * RM_ROWS + row] = e;
      }
    }
    __syncthreads();

    // ---- output layer: db3, dW3 += D . H2^T, dH2 = W3^T . D
    if (tid < d.out)
      for (int r = 0; r < RM_ROWS; ++r) db3 += (double)sD[tid * SR + r];
#pragma unroll
    for (int s = 0; s < RM_T3; ++s) {
      const int t = wv + RM_WAVES * s;
      if (t < nt3) {
        const int ft = t / n2f, nt = t - ft * n2f;
        acc3[s] += __builtin_convertvector(rm_tile(sD + ft * 16 * SR, SR, 1, sH2 + nt * 16 * SRD, 1, SRD, RM_ROWS >> 2, g, i, zero4), v4d);
      }
    }
    v4f dh = zero4;
    if (hft < n2f) dh = rm_tile(sW3 + hft * 16, 1, d.sw3, sD + hrt * 16, SR, 1, d.outp >> 2, g, i, zero4);
    __syncthreads();
    if (tid < RM_ROWS && tid < nvalid) {
      double tot = 0.;      // (the statistics take the float64 row sums, before row_err's rounding)
      for (int ft = 0; ft < n3f; ++ft) tot += sRed[ft * RM_ROWS + tid];
      if (a.row_err != nullptr) a.row_err[row0 + tid] = (float)tot;
      sE += tot; sE2 += tot * tot;
    }
    if (hft < n2f) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = hft * 16 + 4 * g + r, row = hrt * 16 + i;
        sD[f * SR + row] = sH2[f * SRD + row] > 0. ? dh[r] : 0.f;
      }
    }
    __syncthreads();

    // ---- second hidden layer: db2, dW2 += dZ2 . H1^T, dH1 = W2^T . dZ2
    if (tid < d.h2)
      for (int r = 0; r < RM_ROWS; ++r) db2 += (double)sD[tid * SR + r];
#pragma unroll
    for (int s = 0; s < RM_T2; ++s) {
      const int t = wv + RM_WAVES * s;
      if (t < nt2) {
        const int ft = t / n1f, nt = t - ft * n1f;
        acc2[s] += __builtin_convertvector(rm_tile(sD + ft * 16 * SR, SR, 1, sH1 + nt * 16 * SRD, 1, SRD, RM_ROWS >> 2, g, i, zero4), v4d);
      }
    }
    dh = zero4;
    if (hft < n1f) dh = rm_tile(sW2 + hft * 16, 1, d.sw2, sD + hrt * 16, SR, 1, d.h2p >> 2, g, i, zero4);
    __syncthreads();
    if (hft < n1f) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = hft * 16 + 4 * g + r, row = hrt * 16 + i;
        sD[f * SR + row] = sH1[f * SRD + row] > 0. ? dh[r] : 0.f;
      }
    }
    __syncthreads();

    // ---- first hidden layer: db1, dW1 += dZ1 . X^T
    if (tid < d.h1)
      for (int r = 0; r < RM_ROWS; ++r) db1 += (double)sD[tid * SR + r];
#pragma unroll
    for (int s = 0; s < RM_T1; ++s) {
      const int t = wv + RM_WAVES * s;
      if (t < nt1) {
        const int ft = t / n1n, nt = t - ft * n1n;
        acc1[s] += __builtin_convertvector(rm_tile(sD + ft * 16 * SR, SR, 1, sX + nt * 16 * SR, 1, SR, RM_ROWS >> 2, g, i, zero4), v4d);
      }
    }
    __syncthreads();
  }

  // ---- this workgroup's sums of the real entries -> its slice
  float* dst = a.part + (size_t)blockIdx.x * d.np;
#pragma unroll
  for (int s = 0; s < RM_T3; ++s) {
    const int t = wv + RM_WAVES * s;
    if (t < nt3) {
      const int ft = t / n2f, nt = t - ft * n2f, col = nt * 16 + i;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = ft * 16 + 4 * g + r;
        if (f < d.out && col < d.h2) dst[d.oW3 + f * d.h2 + col] = (float)acc3[s][r];
      }
    }
  }
#pragma unroll
  for (int s = 0; s < RM_T2; ++s) {
    const int t = wv + RM_WAVES * s;
    if (t < nt2) {
      const int ft = t / n1f, nt = t - ft * n1f, col = nt * 16 + i;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = ft * 16 + 4 * g + r;
        if (f < d.h2 && col < d.h1) dst[d.oW2 + f * d.h1 + col] = (float)acc2[s][r];
      }
    }
  }
#pragma unroll
  for (int s = 0; s < RM_T1; ++s) {
    const int t = wv + RM_WAVES * s;
    if (t < nt1) {
      const int ft = t / n1n, nt = t - ft * n1n, col = nt * 16 + i;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = ft * 16 + 4 * g + r;
        if (f < d.h1 && col < d.in) dst[d.oW1 + f * d.in + col] = (float)acc1[s][r];
      }
    }
  }
  if (tid < d.out) dst[d.ob3 + tid] = (float)db3;
  if (tid < d.h2) dst[d.ob2 + tid] = (float)db2;
  if (tid < d.h1) dst[d.ob1 + tid] = (float)db1;
  double* sdd = sRed;
  if (tid < RM_ROWS) { sdd[tid] = sE; sdd[RM_ROWS + tid] = sE2; }
  __syncthreads();
  if (tid == 0) {
    double e = 0., e2 = 0.;
    for (int r = 0; r < RM_ROWS; ++r) { e += sdd[r]; e2 += sdd[RM_ROWS + r]; }
    a.stats[2 * blockIdx.x] = e; a.stats[2 * blockIdx.x + 1] = e2;
  }
}

// grad = (float)(scale * (part[0] + part[1] + ...)) in that order, then torch.optim.Adam's single-tensor step
__global__ void __launch_bounds__(256) reg_mlp_adam_kernel(float* p, float* m, float* v, const int* adam_t, int n, const float* __restrict__ part, int n_part,
                                                           double scale, double lr, double beta1, double beta2, double eps) {
  __shared__ float bc[2];
  if (threadIdx.x == 0) {
    const double t = (double)(adam_t[0] + 1);
    bc[0] = (float)(-(lr / (1.0 - pow(beta1, t))));      // -step_size
    bc[1] = (float)sqrt(1.0 - pow(beta2, t));
  }
  __syncthreads();
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  double s = (double)part[idx];
  for (int w = 1; w < n_part; ++w) s += (double)part[(size_t)w * n + idx];
  const float gi = (float)(s * scale);
  // torch's single-tensor Adam, operation by operation as its CPU kernels round (the library is built with -ffp-contract=off):
  //   exp_avg.lerp_(grad, 1 - beta1)                       fma(w, grad - m, m)
  //   exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1-beta2) v * beta2 + ((1 - beta2) * grad) * grad
  //   denom = exp_avg_sq.sqrt() / sqrt(bias2) + eps;  param.addcdiv_(exp_avg, denom, value=-lr / bias1)
  // with the scalars computed in double, as Python does, and rounded to float32 once (1 - (float)0.999 would be 1.3e-5 off 0.001)
  const float b2 = (float)beta2, w1 = (float)(1.0 - beta1), w2 = (float)(1.0 - beta2);
  const float mo = m[idx];
  const float mi = fmaf(w1, gi - mo, mo);
  const float vi = v[idx] * b2 + (w2 * gi) * gi;
  m[idx] = mi; v[idx] = vi;
  const float denom = sqrtf(vi) / bc[1] + (float)eps;
  p[idx] = p[idx] + (bc[0] * mi) / denom;
}

// out4 = {MSE, mean(row_err), population std(row_err), 0}; *adam_step += 1
__global__ void __launch_bounds__(256) reg_mlp_stats_kernel(const double* __restrict__ stats, int n_part, int rows, int out, float* out4, int* adam_t) {
  __shared__ double sd[2 * RM_MAX_WG];
  const int tid = threadIdx.x;
  if (tid < n_part) { sd[2 * tid] = stats[2 * tid]; sd[2 * tid + 1] = stats[2 * tid + 1]; }
  __syncthreads();
  if (tid != 0) return;
  double e = 0., e2 = 0.;
  for (int w = 0; w < n_part; ++w) { e += sd[2 * w]; e2 += sd[2 * w + 1]; }
  const double mean = e / (double)rows;
  double var = e2 / (double)rows - mean * mean;
  if (var < 0.) var = 0.;
  out4[0] = (float)(e / ((double)rows * (double)out)); out4[1] = (float)mean; out4[2] = (float)sqrt(var); out4[3] = 0.f;
  adam_t[0] += 1;
}

__global__ void __launch_bounds__(256) shape_adv_kernel(float* adv, const float* __restrict__ row_err, long long n) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k < n) adv[k] = adv[k] / (1.0f + row_err[k]);
}

// 0, or the fail() code of a shape that is not served
int rm_check(const char* who, long long rows, int in_a, int in_b, int h1, int h2, int out) {
  if (h1 < 1 || h1 > RM_MAX_H || h2 < 1 || h2 > RM_MAX_H)
    return fail("%s: hidden layers (%d, %d) are not served (two hidden layers of 1..%d units each)", who, h1, h2, RM_MAX_H);
  if (in_a < 0 || in_a > RM_MAX_INA) return fail("%s: in_a %d (0..%d)", who, in_a, RM_MAX_INA);
  if (in_b < 1 || in_b > RM_MAX_INB) return fail("%s: in_b %d (1..%d)", who, in_b, RM_MAX_INB);
  if (out < 1 || out > RM_MAX_OUT) return fail("%s: out %d (1..%d)", who, out, RM_MAX_OUT);
  if (rows < 1 || rows > RM_MAX_ROWS) return fail("%s: rows = %lld (1..%d)", who, rows, RM_MAX_ROWS);
  return 0;
}

inline long long rm_ws_bytes(int rows, const RmDims& d) {
  return (long long)RM_STAT_DOUBLES * (long long)sizeof(double) + (long long)rm_grid(rows) * d.np * (long long)sizeof(float);
}

}  // namespace
}  // namespace icrl

using namespace icrl;

extern "C" size_t icrl_reg_mlp_ws_bytes(long long rows, int in_a, int in_b, int h1, int h2, int out) {
  if (rm_check("icrl_reg_mlp_ws_bytes", rows, in_a, in_b, h1, h2, out) != 0) return 0;
  return (size_t)rm_ws_bytes((int)rows, rm_dims(in_a, in_b, h1, h2, out));
}

extern "C" int icrl_reg_mlp_step(float* params, float* exp_avg, float* exp_avg_sq, int32_t* adam_step, const float* xa, const float* xb,
                                 const float* target, long long rows, int in_a, int in_b, int h1, int h2, int out, double lr, double beta1,
                                 double beta2, double eps, float* row_err, float* out4, void* ws, long long ws_bytes, void* stream) {
  const char* who = "icrl_reg_mlp_step";
  if (const int e = rm_check(who, rows, in_a, in_b, h1, h2, out)) return e;
  if (!params || !exp_avg || !exp_avg_sq || !adam_step || !xb || !target || !out4 || (in_a > 0 && !xa))
    return fail("%s: NULL argument (params, exp_avg, exp_avg_sq, adam_step, xb, target and out4 are required, xa when in_a > 0; row_err may be NULL)", who);
  const RmDims d = rm_dims(in_a, in_b, h1, h2, out);
  const long long need = rm_ws_bytes((int)rows, d);
  if (ws == nullptr || ws_bytes < need)
    return fail("%s: ws of %lld bytes, icrl_reg_mlp_ws_bytes(%lld, %d, %d, %d, %d, %d) = %lld", who, ws == nullptr ? 0LL : ws_bytes, rows, in_a, in_b, h1, h2, out, need);
  hipStream_t s = (hipStream_t)stream;
  const int grid = rm_grid((int)rows);
  RmArgs a;
  a.d = d; a.params = params; a.xa = xa; a.xb = xb; a.target = target; a.row_err = row_err; a.rows = (int)rows;
  a.stats = (double*)ws; a.part = (float*)((char*)ws + RM_STAT_DOUBLES * sizeof(double));
  const size_t lds = (size_t)d.lds_floats * sizeof(float);
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)reg_mlp_tile_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(reg_mlp_tile_kernel, dim3(grid), dim3(RM_THREADS), lds, s, a);
  hipLaunchKernelGGL(reg_mlp_adam_kernel, dim3((d.np + 255) / 256), dim3(256), 0, s, params, exp_avg, exp_avg_sq, (const int*)adam_step, d.np,
                     (const float*)a.part, grid, 2.0 / ((double)rows * (double)out), lr, beta1, beta2, eps);
  hipLaunchKernelGGL(reg_mlp_stats_kernel, dim3(1), dim3(256), 0, s, (const double*)a.stats, grid, (int)rows, out, out4, (int*)adam_step);
  return (int)hipGetLastError();
}

extern "C" int icrl_shape_advantages(float* adv, const float* row_err, long long rows, void* stream) {
  if (!adv || !row_err || rows < 1) return fail("icrl_shape_advantages: rows = %lld, NULL argument", rows);
  hipLaunchKernelGGL(shape_adv_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, adv, row_err, rows);
  return (int)hipGetLastError();
}
