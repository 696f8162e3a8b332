// One full-batch classifier step of sigmoid(MLP(in -> h1 -> ReLU -> h2 -> ReLU -> 1)) with a BCE loss and Adam, and the shaped cost the
// stepped network (or the true cost itself) adds to the rollout's rewards — gfx950.
//
// The rollout-end work of the reference's CostShapingCallback (icrl/exploration.py:73-169, `gail -ucsc [-ucn]`): the cost network takes ONE
// optimiser step on all T x N rows of (raw observation, stored action) -> true cost, then log(prediction of the STEPPED network) — or, without
// the network, log(1e-3) * true cost — is added to the buffer's rewards.  icrl_cls_mlp_step is the step, icrl_cost_shaping_apply the second
// pass; both read xa as float64 (the un-normalised observations), rounded to float32 on the load (the reference's `.float()`).
//
// The step is the sibling of icrl_reg_mlp_step (reg_mlp.hip) with a classifier head, and keeps its structure: a workgroup (8 waves) owns the
// 32-row groups grp = blockIdx.x, += gridDim.x, the weights sit in LDS zero-padded to the MFMA granule, the forward pass of the hidden
// layers is v_mfma_f64_16x16x4_f64 on the float32 parameters and inputs, the backward products of a group are v_mfma_f32_16x16x4_f32 tiles
// summed over the groups in float64, every workgroup writes its sums to its own slice of ws, and cls_mlp_adam_kernel adds the slices in index
// order.  What differs is the one-unit output layer, which no 16-unit tile pays for: 32 lanes take one row each — z = W3 . h2 + b3 in float64
// in unit order, p = sigmoid(z), the row's BCE term with both logs clamped at -100 (torch's BCELoss), dL/dz as torch's backward forms it
// ((p - y) / max((1 - p) p, 1e-12) * (1 - p) p), all float64 — and the output layer's gradient products (dW3 = dz . h2^T, dh2 = W3^T . dz)
// are float32 VALU products of the same float32 roundings, a group's 32 rows at a time, summed over the groups in float64 like the tiles.
// Plain launches, no cooperative launch, no waiting between workgroups, no atomics; the grid is a function of rows alone and every sum has a
// fixed order: a call is deterministic bit for bit.
#include "common.h"

namespace icrl {
namespace {

typedef float v4f __attribute__((ext_vector_type(4)));
typedef double v4d __attribute__((ext_vector_type(4)));

constexpr int CS_THREADS = 512;
constexpr int CS_WAVES = CS_THREADS / 64;
constexpr int CS_ROWS = 32;          // rows of a group: two MFMA row tiles
constexpr int CS_SR = 34;            // row stride (floats) of the float32 [unit][row] images (inputs, upstream gradients)
constexpr int CS_SRD = 33;           // row stride (doubles) of the float64 [unit][row] images of the hidden activations
constexpr int CS_MAX_WG = 256;
constexpr int CS_MAX_H = 64, CS_MAX_INA = 128, CS_MAX_INB = 16;
constexpr int CS_MAX_ROWS = 1 << 21;
constexpr int CS_STAT = 4;                               // doubles per workgroup at the head of ws
constexpr int CS_STAT_DOUBLES = CS_STAT * CS_MAX_WG;
constexpr int CS_T2 = 2, CS_T1 = 5;                      // weight-gradient tiles (16 x 16) a wave owns at most: dW2 4 x 4, dW1 4 x 9 over 8 waves
constexpr double CS_LOG_1EM3 = -6.907755278982137;       // log(1e-3), the float64 numpy gives

struct CsDims {
  int in_a, in_b, in, h1, h2;
  int inp4, inp16, h1p, h2p;           // in rounded up to 4 (the K step) and 16 (a tile of dW1 columns); widths rounded up to 16
  int sw1, sw2;                        // row strides of the weight images
  int oW1, ob1, oW2, ob2, oW3, ob3, np;
  int lW1, lW2, lW3, lb1, lb2, lX, lH1, lH2, lD, lDz, lRed, lds_floats;
};

// a stride of 2 mod 4 floats: the 16 units of an A-operand read start on 16 different even banks, their 4 inputs beside them
inline int cs_wstride(int K) { return ((K + 3) & ~3) + 2; }

inline CsDims cs_dims(int in_a, int in_b, int h1, int h2) {
  CsDims d;
  d.in_a = in_a; d.in_b = in_b; d.in = in_a + in_b; d.h1 = h1; d.h2 = h2;
  d.inp4 = (d.in + 3) & ~3; d.inp16 = (d.in + 15) & ~15;
  d.h1p = (h1 + 15) & ~15; d.h2p = (h2 + 15) & ~15;
  d.sw1 = cs_wstride(d.inp4); d.sw2 = cs_wstride(d.h1p);
  d.oW1 = 0; d.ob1 = d.oW1 + h1 * d.in; d.oW2 = d.ob1 + h1; d.ob2 = d.oW2 + h2 * h1; d.oW3 = d.ob2 + h2; d.ob3 = d.oW3 + h2;
  d.np = d.ob3 + 1;
  int o = 0;
  d.lW1 = o; o += d.h1p * d.sw1;
  d.lW2 = o; o += d.h2p * d.sw2;
  d.lW3 = o; o += d.h2p;
  d.lb1 = o; o += d.h1p;
  d.lb2 = o; o += d.h2p;
  d.lX = o; o += d.inp16 * CS_SR;
  o = (o + 1) & ~1;                    // the hidden activations are doubles
  d.lH1 = o; o += 2 * d.h1p * CS_SRD;
  d.lH2 = o; o += 2 * d.h2p * CS_SRD;
  d.lD = o; o += (d.h1p > d.h2p ? d.h1p : d.h2p) * CS_SR;
  d.lDz = o; o += CS_ROWS;
  o = (o + 1) & ~1;                    // 3 x 32 doubles of per-row statistics at the end
  d.lRed = o; o += 2 * 3 * CS_ROWS;
  d.lds_floats = o;
  return d;
}

inline int cs_grid(long long rows) {
  const long long groups = (rows + CS_ROWS - 1) / CS_ROWS;
  return (int)(groups < CS_MAX_WG ? groups : CS_MAX_WG);
}

struct CsArgs {
  CsDims d;
  const float* params;
  const double* xa;
  const float* xb;
  const float* target;
  float* rewards;     // the apply pass only
  int rows;
  double* stats;      // [gridDim.x][CS_STAT]
  float* part;        // [gridDim.x][np], the step only
};

// acc += A [16 x 4 ksteps] . B [4 ksteps x 16]: A(f, k) at A[f * fa + k * ka], B(k, n) at B[k * kb + n * nb]; lane (g = lane >> 4, i = lane & 15)
// feeds A(i, 4 kk + g) and B(4 kk + g, i) and receives rows 4 g + r, column i in register r.  B may be a float64 image (rounded on the read).
// Two chains, even and odd K steps, as in reg_mlp.hip.
template <class TB>
__device__ __forceinline__ v4f cs_tile(const float* A, int fa, int ka, const TB* B, int kb, int nb, int ksteps, int g, int i, v4f acc) {
  const float* pa = A + i * fa + g * ka;
  const TB* pb = B + g * kb + i * nb;
  const int sa = 4 * ka, sb = 4 * kb;
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
__device__ __forceinline__ v4d cs_tile_d(const float* A, int fa, int ka, const TB* B, int kb, int nb, int ksteps, int g, int i) {
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

// TRAIN: forward, the BCE terms and the backward pass -> this workgroup's gradient sums and {sum loss, sum p, sum y}.
// !TRAIN: forward only; shaped = log(float32(p)) added to rewards -> {sum, min, max of shaped}.
template <bool TRAIN>
__global__ void __launch_bounds__(CS_THREADS) cls_tile_kernel(CsArgs a) {
  extern __shared__ float lds[];
  const CsDims& d = a.d;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, g = lane >> 4, i = lane & 15;
  float *sW1 = lds + d.lW1, *sW2 = lds + d.lW2, *sW3 = lds + d.lW3, *sb1 = lds + d.lb1, *sb2 = lds + d.lb2;
  float *sX = lds + d.lX, *sD = lds + d.lD, *sDz = lds + d.lDz;
  double *sH1 = reinterpret_cast<double*>(lds + d.lH1), *sH2 = reinterpret_cast<double*>(lds + d.lH2), *sRed = reinterpret_cast<double*>(lds + d.lRed);
  const int SR = CS_SR, SRD = CS_SRD;

  // ---- the zero-padded images of the parameters
  for (int k = tid; k < d.lds_floats; k += CS_THREADS) lds[k] = 0.f;
  __syncthreads();
  for (int e = tid; e < d.h1 * d.in; e += CS_THREADS) { const int f = e / d.in; sW1[f * d.sw1 + (e - f * d.in)] = a.params[d.oW1 + e]; }
  for (int e = tid; e < d.h2 * d.h1; e += CS_THREADS) { const int f = e / d.h1; sW2[f * d.sw2 + (e - f * d.h1)] = a.params[d.oW2 + e]; }
  if (tid < d.h1) sb1[tid] = a.params[d.ob1 + tid];
  if (tid < d.h2) { sb2[tid] = a.params[d.ob2 + tid]; sW3[tid] = a.params[d.oW3 + tid]; }
  const double b3 = (double)a.params[d.ob3];
  __syncthreads();

  const int n1f = d.h1p >> 4, n2f = d.h2p >> 4, n1n = d.inp16 >> 4;
  const int nt2 = n2f * n1f, nt1 = n1f * n1n;
  const v4f zero4 = {0.f, 0.f, 0.f, 0.f};
  const v4d zero4d = {0., 0., 0., 0.};
  // weight gradients: a group's 32-row product is float32, the sum over the workgroup's groups float64
  v4d acc2[CS_T2], acc1[CS_T1];
#pragma unroll
  for (int s = 0; s < CS_T2; ++s) acc2[s] = zero4d;
#pragma unroll
  for (int s = 0; s < CS_T1; ++s) acc1[s] = zero4d;
  double dw3 = 0., db3 = 0., db2 = 0., db1 = 0.;
  // per row lane (tid < 32): TRAIN {sum loss, sum p, sum y}; apply {sum, min, max of shaped}
  double s0 = 0., s1 = TRAIN ? 0. : __builtin_inf(), s2 = TRAIN ? 0. : -__builtin_inf();

  const int groups = (a.rows + CS_ROWS - 1) / CS_ROWS;
  const int hft = wv >> 1, hrt = wv & 1;      // a hidden layer is at most 4 unit tiles x 2 row tiles = one job per wave
  for (int grp = blockIdx.x; grp < groups; grp += gridDim.x) {
    const int row0 = grp * CS_ROWS;
    const int nvalid = a.rows - row0 < CS_ROWS ? a.rows - row0 : CS_ROWS;

    // ---- the group's inputs -> sX [input][row]; rows past the end are zeros.  Every load is issued (a row past the end reads the group's
    // last live row): no load sits under a branch
    if (d.in_a > 0) {
      const double* src = a.xa + (size_t)row0 * d.in_a;
      for (int e = tid; e < CS_ROWS * d.in_a; e += CS_THREADS) {
        const int r = e / d.in_a, c = e - r * d.in_a;
        const float v = (float)src[(r < nvalid ? r : nvalid - 1) * d.in_a + c];
        sX[c * SR + r] = r < nvalid ? v : 0.f;
      }
    }
    {
      const float* src = a.xb + (size_t)row0 * d.in_b;
      for (int e = tid; e < CS_ROWS * d.in_b; e += CS_THREADS) {
        const int r = e / d.in_b, c = e - r * d.in_b;
        const float v = src[(r < nvalid ? r : nvalid - 1) * d.in_b + c];
        sX[(d.in_a + c) * SR + r] = r < nvalid ? v : 0.f;
      }
    }
    __syncthreads();

    // ---- forward, in float64 on the float32 parameters and inputs (the hidden activations stay float64 between the layers)
    if (hft < n1f) {
      const v4d z = cs_tile_d(sW1 + hft * 16 * d.sw1, d.sw1, 1, sX + hrt * 16, SR, 1, d.inp4 >> 2, g, i);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = hft * 16 + g + 4 * r;
        const double h = z[r] + (double)sb1[f];
        sH1[f * SRD + hrt * 16 + i] = h > 0. ? h : 0.;
      }
    }
    __syncthreads();
    if (hft < n2f) {
      const v4d z = cs_tile_d(sW2 + hft * 16 * d.sw2, d.sw2, 1, sH1 + hrt * 16, SRD, 1, d.h1p >> 2, g, i);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = hft * 16 + g + 4 * r;
        const double h = z[r] + (double)sb2[f];
        sH2[f * SRD + hrt * 16 + i] = h > 0. ? h : 0.;
      }
    }
    __syncthreads();

    // ---- the head: one row per lane, units in index order
    if (tid < CS_ROWS) {
      const bool live = tid < nvalid;
      double z = 0.;
      for (int f = 0; f < d.h2; ++f) z += (double)sW3[f] * sH2[f * SRD + tid];
      z += b3;
      const double pr = 1.0 / (1.0 + exp(-z));
      if (TRAIN) {
        const double y = (double)a.target[row0 + (live ? tid : nvalid - 1)];
        double lp = log(pr), lq = log(1.0 - pr);
        lp = lp < -100. ? -100. : lp; lq = lq < -100. ? -100. : lq;
        const double loss = (y - 1.0) * lq - y * lp;
        const double pq = (1.0 - pr) * pr;
        const double dz = (pr - y) / (pq < 1e-12 ? 1e-12 : pq) * pq;
        sDz[tid] = live ? (float)dz : 0.f;      // rows past the end: no gradient
        if (live) { s0 += loss; s1 += pr; s2 += y; }
      } else if (live) {
        const float shaped = (float)log((double)(float)pr);      // the log of the float32 prediction, rounded once; -inf at 0
        a.rewards[row0 + tid] = a.rewards[row0 + tid] + shaped;
        const double sd = (double)shaped;
        s0 += sd; s1 = sd < s1 ? sd : s1; s2 = sd > s2 ? sd : s2;
      }
    }
    if (!TRAIN) continue;      // (the next group's writes of sH2 come two barriers after this read)
    __syncthreads();

    // ---- output layer: db3, dW3 += dz . H2^T, dH2 = W3^T . dz under the ReLU mask
    if (tid < d.h2) {
      float acc = 0.f;
      for (int r = 0; r < CS_ROWS; ++r) acc += sDz[r] * (float)sH2[tid * SRD + r];
      dw3 += (double)acc;
    }
    if (tid == 64)
      for (int r = 0; r < CS_ROWS; ++r) db3 += (double)sDz[r];
    for (int e = tid; e < d.h2p * CS_ROWS; e += CS_THREADS) {
      const int f = e >> 5, row = e & 31;
      sD[f * SR + row] = sH2[f * SRD + row] > 0. ? sW3[f] * sDz[row] : 0.f;
    }
    __syncthreads();

    // ---- second hidden layer: db2, dW2 += dZ2 . H1^T, dH1 = W2^T . dZ2
    if (tid < d.h2)
      for (int r = 0; r < CS_ROWS; ++r) db2 += (double)sD[tid * SR + r];
#pragma unroll
    for (int s = 0; s < CS_T2; ++s) {
      const int t = wv + CS_WAVES * s;
      if (t < nt2) {
        const int ft = t / n1f, nt = t - ft * n1f;
        acc2[s] += __builtin_convertvector(cs_tile(sD + ft * 16 * SR, SR, 1, sH1 + nt * 16 * SRD, 1, SRD, CS_ROWS >> 2, g, i, zero4), v4d);
      }
    }
    v4f dh = zero4;
    if (hft < n1f) dh = cs_tile(sW2 + hft * 16, 1, d.sw2, sD + hrt * 16, SR, 1, d.h2p >> 2, g, i, zero4);
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
      for (int r = 0; r < CS_ROWS; ++r) db1 += (double)sD[tid * SR + r];
#pragma unroll
    for (int s = 0; s < CS_T1; ++s) {
      const int t = wv + CS_WAVES * s;
      if (t < nt1) {
        const int ft = t / n1n, nt = t - ft * n1n;
        acc1[s] += __builtin_convertvector(cs_tile(sD + ft * 16 * SR, SR, 1, sX + nt * 16 * SR, 1, SR, CS_ROWS >> 2, g, i, zero4), v4d);
      }
    }
    __syncthreads();
  }

  if (TRAIN) {      // ---- this workgroup's sums of the real entries -> its slice
    float* dst = a.part + (size_t)blockIdx.x * d.np;
#pragma unroll
    for (int s = 0; s < CS_T2; ++s) {
      const int t = wv + CS_WAVES * s;
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
    for (int s = 0; s < CS_T1; ++s) {
      const int t = wv + CS_WAVES * s;
      if (t < nt1) {
        const int ft = t / n1n, nt = t - ft * n1n, col = nt * 16 + i;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int f = ft * 16 + 4 * g + r;
          if (f < d.h1 && col < d.in) dst[d.oW1 + f * d.in + col] = (float)acc1[s][r];
        }
      }
    }
    if (tid < d.h2) { dst[d.oW3 + tid] = (float)dw3; dst[d.ob2 + tid] = (float)db2; }
    if (tid == 64) dst[d.ob3] = (float)db3;
    if (tid < d.h1) dst[d.ob1 + tid] = (float)db1;
  }
  __syncthreads();      // (the apply pass leaves its loop without one)
  if (tid < CS_ROWS) { sRed[tid] = s0; sRed[CS_ROWS + tid] = s1; sRed[2 * CS_ROWS + tid] = s2; }
  __syncthreads();
  if (tid == 0) {
    double t0 = sRed[0], t1 = sRed[CS_ROWS], t2 = sRed[2 * CS_ROWS];
    for (int r = 1; r < CS_ROWS; ++r) {
      const double u1 = sRed[CS_ROWS + r], u2 = sRed[2 * CS_ROWS + r];
      t0 += sRed[r];
      if (TRAIN) { t1 += u1; t2 += u2; } else { t1 = u1 < t1 ? u1 : t1; t2 = u2 > t2 ? u2 : t2; }
    }
    double* st = a.stats + CS_STAT * blockIdx.x;
    st[0] = t0; st[1] = t1; st[2] = t2; st[3] = 0.;
  }
}

// grad = (float)(scale * (part[0] + part[1] + ...)) in that order, then torch.optim.Adam's single-tensor step, operation by operation as its
// kernels round (reg_mlp.hip's reg_mlp_adam_kernel has the derivation; the library is built with -ffp-contract=off)
__global__ void __launch_bounds__(256) cls_mlp_adam_kernel(float* p, float* m, float* v, const int* adam_t, int n, const float* __restrict__ part, int n_part,
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
  const float b2 = (float)beta2, w1 = (float)(1.0 - beta1), w2 = (float)(1.0 - beta2);
  const float mo = m[idx];
  const float mi = fmaf(w1, gi - mo, mo);
  const float vi = v[idx] * b2 + (w2 * gi) * gi;
  m[idx] = mi; v[idx] = vi;
  const float denom = sqrtf(vi) / bc[1] + (float)eps;
  p[idx] = p[idx] + (bc[0] * mi) / denom;
}

// step: out4 = {loss, mean(p), mean(target), 0}; *adam_step += 1.
// apply: out4 = {mean, min, max of shaped, 0}; scale != 0 (the branch without a network): the sums are of the targets, shaped = scale * target
__global__ void __launch_bounds__(256) cls_stats_kernel(const double* __restrict__ stats, int n_part, long long rows, double* out4, int* adam_t, double scale) {
  __shared__ double sd[CS_STAT_DOUBLES];
  const int tid = threadIdx.x;
  if (tid < n_part)
    for (int k = 0; k < 3; ++k) sd[CS_STAT * tid + k] = stats[CS_STAT * tid + k];
  __syncthreads();
  if (tid != 0) return;
  double t0 = sd[0], t1 = sd[1], t2 = sd[2];
  for (int w = 1; w < n_part; ++w) {
    const double u1 = sd[CS_STAT * w + 1], u2 = sd[CS_STAT * w + 2];
    t0 += sd[CS_STAT * w];
    if (adam_t != nullptr) { t1 += u1; t2 += u2; } else { t1 = u1 < t1 ? u1 : t1; t2 = u2 > t2 ? u2 : t2; }
  }
  const double n = (double)rows;
  if (adam_t != nullptr) {
    out4[0] = t0 / n; out4[1] = t1 / n; out4[2] = t2 / n; out4[3] = 0.;
    adam_t[0] += 1;
  } else if (scale != 0.) {      // scale < 0: the smallest shaped value belongs to the largest target
    out4[0] = scale * (t0 / n); out4[1] = scale * t2; out4[2] = scale * t1; out4[3] = 0.;
  } else {
    out4[0] = t0 / n; out4[1] = t1; out4[2] = t2; out4[3] = 0.;
  }
}

// the branch without a network: rewards[r] = float32(float64(rewards[r]) + scale * target[r]); per workgroup {sum, min, max of target}
__global__ void __launch_bounds__(256) cost_scale_kernel(const float* __restrict__ target, float* rewards, long long rows, double scale, double* stats) {
  __shared__ double sd[3 * 256];
  const int tid = threadIdx.x;
  double s = 0., mn = __builtin_inf(), mx = -__builtin_inf();
  for (long long r = (long long)blockIdx.x * 256 + tid; r < rows; r += (long long)gridDim.x * 256) {
    const double y = (double)target[r];
    rewards[r] = (float)((double)rewards[r] + scale * y);
    s += y; mn = y < mn ? y : mn; mx = y > mx ? y : mx;
  }
  sd[tid] = s; sd[256 + tid] = mn; sd[512 + tid] = mx;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if (tid < w) {
      sd[tid] += sd[tid + w];
      sd[256 + tid] = sd[256 + tid + w] < sd[256 + tid] ? sd[256 + tid + w] : sd[256 + tid];
      sd[512 + tid] = sd[512 + tid + w] > sd[512 + tid] ? sd[512 + tid + w] : sd[512 + tid];
    }
    __syncthreads();
  }
  if (tid == 0) {
    double* st = stats + CS_STAT * blockIdx.x;
    st[0] = sd[0]; st[1] = sd[256]; st[2] = sd[512]; st[3] = 0.;
  }
}

// 0, or the fail() code of a shape that is not served
int cs_check(const char* who, long long rows, int in_a, int in_b, int h1, int h2) {
  if (h1 < 1 || h1 > CS_MAX_H || h2 < 1 || h2 > CS_MAX_H)
    return fail("%s: hidden layers (%d, %d) are not served (two hidden layers of 1..%d units each)", who, h1, h2, CS_MAX_H);
  if (in_a < 0 || in_a > CS_MAX_INA) return fail("%s: in_a %d (0..%d)", who, in_a, CS_MAX_INA);
  if (in_b < 1 || in_b > CS_MAX_INB) return fail("%s: in_b %d (1..%d)", who, in_b, CS_MAX_INB);
  if (rows < 1 || rows > CS_MAX_ROWS) return fail("%s: rows = %lld (1..%d)", who, rows, CS_MAX_ROWS);
  return 0;
}

inline long long cs_ws_bytes(long long rows, const CsDims& d) {
  return (long long)CS_STAT_DOUBLES * (long long)sizeof(double) + (long long)cs_grid(rows) * d.np * (long long)sizeof(float);
}

template <bool TRAIN>
int cs_launch_tiles(const CsArgs& a, int grid, hipStream_t s) {
  const size_t lds = (size_t)a.d.lds_floats * sizeof(float);
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)cls_tile_kernel<TRAIN>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(cls_tile_kernel<TRAIN>, dim3(grid), dim3(CS_THREADS), lds, s, a);
  return 0;
}

}  // namespace
}  // namespace icrl

using namespace icrl;

extern "C" size_t icrl_cls_mlp_ws_bytes(long long rows, int in_a, int in_b, int h1, int h2) {
  if (cs_check("icrl_cls_mlp_ws_bytes", rows, in_a, in_b, h1, h2) != 0) return 0;
  return (size_t)cs_ws_bytes(rows, cs_dims(in_a, in_b, h1, h2));
}

extern "C" int icrl_cls_mlp_step(float* params, float* exp_avg, float* exp_avg_sq, int32_t* adam_step, const double* xa, const float* xb,
                                 const float* target, long long rows, int in_a, int in_b, int h1, int h2, double lr, double beta1, double beta2,
                                 double eps, double* out4, void* ws, long long ws_bytes, void* stream) {
  const char* who = "icrl_cls_mlp_step";
  if (const int e = cs_check(who, rows, in_a, in_b, h1, h2)) return e;
  if (!params || !exp_avg || !exp_avg_sq || !adam_step || !xb || !target || !out4 || (in_a > 0 && !xa))
    return fail("%s: NULL argument (params, exp_avg, exp_avg_sq, adam_step, xb, target and out4 are required, xa when in_a > 0)", who);
  const CsDims d = cs_dims(in_a, in_b, h1, h2);
  const long long need = cs_ws_bytes(rows, d);
  if (ws == nullptr || ws_bytes < need)
    return fail("%s: ws of %lld bytes, icrl_cls_mlp_ws_bytes(%lld, %d, %d, %d, %d) = %lld", who, ws == nullptr ? 0LL : ws_bytes, rows, in_a, in_b, h1, h2, need);
  hipStream_t s = (hipStream_t)stream;
  const int grid = cs_grid(rows);
  CsArgs a;
  a.d = d; a.params = params; a.xa = xa; a.xb = xb; a.target = target; a.rewards = nullptr; a.rows = (int)rows;
  a.stats = (double*)ws; a.part = (float*)((char*)ws + CS_STAT_DOUBLES * sizeof(double));
  if (const int e = cs_launch_tiles<true>(a, grid, s)) return e;
  hipLaunchKernelGGL(cls_mlp_adam_kernel, dim3((d.np + 255) / 256), dim3(256), 0, s, params, exp_avg, exp_avg_sq, (const int*)adam_step, d.np,
                     (const float*)a.part, grid, 1.0 / (double)rows, lr, beta1, beta2, eps);
  hipLaunchKernelGGL(cls_stats_kernel, dim3(1), dim3(256), 0, s, (const double*)a.stats, grid, rows, out4, (int*)adam_step, 0.0);
  return (int)hipGetLastError();
}

extern "C" int icrl_cost_shaping_apply(const float* params, const double* xa, const float* xb, const float* target, long long rows, int in_a, int in_b,
                                       int h1, int h2, float* rewards, double* out4, void* ws, long long ws_bytes, void* stream) {
  const char* who = "icrl_cost_shaping_apply";
  if (const int e = cs_check(who, rows, in_a, in_b, h1, h2)) return e;
  if (!rewards || !out4) return fail("%s: NULL argument (rewards and out4 are required)", who);
  if (params != nullptr && (!xb || (in_a > 0 && !xa))) return fail("%s: NULL argument (with params: xb is required, xa when in_a > 0)", who);
  if (params == nullptr && !target) return fail("%s: NULL argument (without params: target is required)", who);
  const long long need = (long long)CS_STAT_DOUBLES * (long long)sizeof(double);
  if (ws == nullptr || ws_bytes < need) return fail("%s: ws of %lld bytes, %lld are needed", who, ws == nullptr ? 0LL : ws_bytes, need);
  hipStream_t s = (hipStream_t)stream;
  if (params == nullptr) {
    const long long blocks = (rows + 255) / 256;
    const int grid = (int)(blocks < CS_MAX_WG ? blocks : CS_MAX_WG);
    hipLaunchKernelGGL(cost_scale_kernel, dim3(grid), dim3(256), 0, s, target, rewards, rows, CS_LOG_1EM3, (double*)ws);
    hipLaunchKernelGGL(cls_stats_kernel, dim3(1), dim3(256), 0, s, (const double*)ws, grid, rows, out4, (int*)nullptr, CS_LOG_1EM3);
    return (int)hipGetLastError();
  }
  const int grid = cs_grid(rows);
  CsArgs a;
  a.d = cs_dims(in_a, in_b, h1, h2); a.params = params; a.xa = xa; a.xb = xb; a.target = target; a.rewards = rewards; a.rows = (int)rows;
  a.stats = (double*)ws; a.part = nullptr;
  if (const int e = cs_launch_tiles<false>(a, grid, s)) return e;
  hipLaunchKernelGGL(cls_stats_kernel, dim3(1), dim3(256), 0, s, (const double*)ws, grid, rows, out4, (int*)nullptr, 0.0);
  return (int)hipGetLastError();
}
