// Forward + backward of the two-critics policy and of the constraint net for ARBITRARY upstream gradients — gfx950.
//
// The last torch piece of the fine-grained loop (fine.hip): `policy.evaluate_actions`, `constraint_net.forward`
// and `torch.autograd.backward` through them.  icrl_policy_fwd_bwd / icrl_cost_mlp_fwd_bwd return the networks' outputs and, given
// d loss / d output per row, d loss / d params in the layout of `params` — so any loss a host writes on (v_r, v_c, log_prob, entropy) or
// on zeta trains the library's own flat buffers.  They read `params` (never params_t), allocate nothing and do not synchronise.
//
// One kernel serves both: a workgroup owns one network (policy: blockIdx.y = pi | vf | cvf — the three branches share nothing but the
// observation) and walks row tiles of 16 (tile = blockIdx.x, += gridDim.x).  Weights sit in LDS for the whole launch as the float32 values
// they are (rows padded by one word: lane j reads W[j][k] without bank conflicts); everything computed from them is FLOAT64: the
// activations of the tile in LDS between the layers, the head, and the weight gradients, which stay in REGISTERS across the tiles (4 x 4
// blocks per thread).  gfx950 runs float64 FMAs at half the float32 rate and these calls are launch-bound, so the step costs little, and
// the result no longer depends on the order of any sum at float32 level: outputs and gradients are the float64 values rounded ONCE to
// float32 — what float64 autograd gives, which is what the tests compare with (a float32 evaluation lands up to a few ulps of the
// larger gradients away from it, sometimes by luck much closer: no bound derived from one holds for another).  At the end every
// workgroup writes its sums to its own float64 slice of `ws` (at most 64 slices) and a second plain launch adds the slices in index order
// and rounds: no atomics, no waiting, the same bits on every call.
// A forward-only call (grad == NULL) runs the same code up to the outputs, hence the same output bits.
//
// Input gradients (the `_in` entry points; DIN = true): d loss / d (first pre-activation) of a tile sits in LDS as float64 (sdz1) next to the
// first layer's weights (sW1), so d loss / d x[r][k] = sum_{j < H1, ascending} sdz1[r][j] W1[j][k] is one more product per tile, a float64 fma
// chain spread over the 256 threads.  A row belongs to one tile: nothing is summed across workgroups.  The policy's three branches share the
// observation: each writes its float64 slice [N][K] of ws and a second plain launch adds pi + vf + cvf in that order and rounds once.  The
// Gaussian head's d loss / d action is the negative of d loss / d mean, which the head block holds already.  The instantiations without DIN take
// the argument block they always took and compile to what they compiled to.
// (-ffp-contract=off as for the rest of the library: every FMA here is an explicit fma().)
#include "common.h"
#include "cost_fn.h"

namespace icrl {
namespace {

constexpr int MG_ROWS = 16;        // rows of a tile
constexpr int MG_THREADS = 256;
constexpr int MG_H = 64;           // hidden width of the LDS images (narrower layers are zero-filled: their units give act(0) = 0 and gradient 0)
constexpr int MG_WSTRIDE = 65;     // row stride (floats) of the hidden / head weight images
constexpr int MG_ASTRIDE = 66;     // row stride (doubles) of the activation images: 16-byte reads stay aligned, the 16 rows of a tile hit 16 bank pairs
constexpr int MG_MAX_PARTS = 64;   // slices of partial sums in ws
constexpr int MG_MAX_N = 65536;
constexpr double MG_LOG_SQRT_2PI = 0.918938533204672741780329736406;
enum { MG_GAUSS = 0, MG_CATEG = 1, MG_VALUE = 2, MG_ZETA = 3, MG_SDE = 4 };

struct MgNet {
  int K, H1, H2, AO, nh, kind;      // inputs, hidden widths, head outputs, hidden layers (1 | 2), what the head's outputs become
  int W1, b1, W2, b2, Wh, bh, ls;   // offsets into params (W2 / b2 unused when nh == 1; ls: log_std, GAUSS [AO] | SDE [MG_H][AO])
  const float* d_out;               // VALUE / ZETA: d loss / d output [N] or NULL (zeros)
  float* out;                       // VALUE / ZETA: output [N] or NULL
};

struct MgArgs {
  MgNet net[3];
  const float* params;
  const float* x;                   // [N, K]
  const float* actions;             // [N, act_store] (policy)
  int act_store, N, n_params;
  const float* d_lp;                // policy head: d loss / d log_prob, d entropy [N] or NULL (zeros)
  const float* d_ent;
  float* lp;                        // [N] or NULL
  float* ent;
  double* part;                     // [gridDim.x][n_params] partial sums; NULL: forward only
};

// the `_in` forms: where the input gradients go (NULL: not asked for)
struct MgArgsIn : MgArgs {
  double* dx64;                     // policy: [3][N][K] float64, slice = blockIdx.y; folded by mlp_dx_fold_kernel
  float* dx32;                      // one network: d loss / d x [N, K], rounded here
  float* d_act;                     // Gaussian head: d loss / d actions [N, act_store]
};
template <bool DIN> struct MgArgsOf { typedef MgArgs type; };
template <> struct MgArgsOf<true> { typedef MgArgsIn type; };

inline int mg_parts(int N) {
  const int tiles = (N + MG_ROWS - 1) / MG_ROWS;
  return tiles < MG_MAX_PARTS ? tiles : MG_MAX_PARTS;
}
// LDS: the float images (weights, biases, log_std, the tile's inputs, the upstream rows), then the double images (three activation
// images, the head's outputs and the log_std terms)
inline size_t mg_lds_floats(int K) {
  const int KP = (K + 3) & ~3;
  return (size_t)MG_H * (KP + 1) + MG_H * MG_WSTRIDE + 16 * MG_WSTRIDE + 160 + (size_t)MG_ROWS * KP + 32;
}
// (the gSDE head adds one double image: exp(2 log_std) [64][16])
inline size_t mg_lds_bytes(int K, bool sde = false) {
  return mg_lds_floats(K) * sizeof(float) + (3 * MG_ROWS * MG_ASTRIDE + 512 + (sde ? MG_H * 16 : 0)) * sizeof(double);
}

template <bool RELU>
__device__ __forceinline__ double mg_act(double z) {
  if (RELU) return z > 0. ? z : 0.;
  return tanh(z);
}
template <bool RELU>
__device__ __forceinline__ double mg_dact(double h) {      // d act / d pre-activation from the activation itself
  if (RELU) return h > 0. ? 1. : 0.;
  return 1. - h * h;
}

// four consecutive values of a float / double image (16-byte aligned) as doubles
__device__ __forceinline__ void mg_load4(const float* p, double (&v)[4]) {
  const float4 f = *reinterpret_cast<const float4*>(p);
  v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
}
__device__ __forceinline__ void mg_load4(const double* p, double (&v)[4]) {
  const double2 a = *reinterpret_cast<const double2*>(p), b = *reinterpret_cast<const double2*>(p + 2);
  v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
}

// out[r][j] = act(b[j] + sum_k W[j][k] in[r][k]) for the 4 rows of this wave, unit j = lane; K4 a multiple of 4
template <bool RELU, class T>
__device__ __forceinline__ void mg_layer(const float* sW, int wstride, const float* sb, const T* in, int istride, int K4, double* out, int lane, int wv) {
  const int r0 = 4 * wv;
  double acc[4];
  for (int q = 0; q < 4; ++q) acc[q] = sb[lane];
  const float* w = sW + lane * wstride;
  for (int k = 0; k < K4; k += 4) {
    const double w0 = w[k], w1 = w[k + 1], w2 = w[k + 2], w3 = w[k + 3];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      double v[4];
      mg_load4(in + (r0 + q) * istride + k, v);
      acc[q] = fma(w3, v[3], fma(w2, v[2], fma(w1, v[1], fma(w0, v[0], acc[q]))));
    }
  }
  for (int q = 0; q < 4; ++q) out[(r0 + q) * MG_ASTRIDE + lane] = mg_act<RELU>(acc[q]);
}

// acc[jj][kk] += sum_r dz[r][j0 + jj] in[r][k0 + kk]
template <class T>
__device__ __forceinline__ void mg_outer(double (&acc)[4][4], const double* dz, int j0, const T* in, int istride, int k0) {
  for (int r = 0; r < MG_ROWS; ++r) {
    double dd[4], vv[4];
    mg_load4(dz + r * MG_ASTRIDE + j0, dd);
    mg_load4(in + r * istride + k0, vv);
#pragma unroll
    for (int jj = 0; jj < 4; ++jj)
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) acc[jj][kk] = fma(dd[jj], vv[kk], acc[jj][kk]);
  }
}

// SDE: the policy branch may carry the state-dependent-noise head (MG_SDE; distributions.py:408-601 with full_std, exp, no squashing,
// learn_features = False): log_std is a matrix [MG_H][AO] (rows beyond the last hidden width zero, like every padding), the variance of
// action c is sum_h latent_h^2 exp(2 log_std[h][c]) + 1e-6 over the latent units in ascending order, and the latent is DETACHED in it:
// log_std takes the log-prob's and the entropy's variance part, the network only the mean part.
template <bool RELU, bool SDE = false, bool DIN = false>
__global__ void __launch_bounds__(MG_THREADS) mlp_fwd_bwd_kernel(typename MgArgsOf<DIN>::type a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const MgNet n = a.net[blockIdx.y];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int K = n.K, KP = (K + 3) & ~3, S1 = KP + 1, HL = n.nh == 2 ? n.H2 : n.H1;
  float* sW1 = sm;                                  // [64][S1]
  float* sW2 = sW1 + MG_H * S1;                     // [64][65]
  float* sWh = sW2 + MG_H * MG_WSTRIDE;             // [16][65]
  float* sb1 = sWh + 16 * MG_WSTRIDE;               // [64]
  float* sb2 = sb1 + 64;                            // [64]
  float* sbh = sb2 + 64;                            // [16]
  float* sls = sbh + 16;                            // [16]
  float* sx = sls + 16;                             // [16][KP]
  float* srow = sx + MG_ROWS * KP;                  // d_lp[16], d_ent[16]
  double* sh1 = reinterpret_cast<double*>(srow + 32);      // [16][66]  (every float image above is a multiple of 4 floats: 16-byte aligned)
  double* sh2 = sh1 + MG_ROWS * MG_ASTRIDE;
  double* sdz = sh2 + MG_ROWS * MG_ASTRIDE;
  double* so = sdz + MG_ROWS * MG_ASTRIDE;          // [16][16] head outputs, then d loss / d head outputs
  double* sdf = so + 256;                           // [16][16] per-row d loss / d log_std (SDE: the variances, then d loss / d variance)
  double* sE2 = sdf + 256;                          // SDE only: [64][16] exp(2 log_std[h][c])
  const float* __restrict__ P = a.params;

  // ---- weights -> LDS, zero beyond the real widths
  for (int i = tid; i < MG_H * S1; i += MG_THREADS) {
    const int j = i / S1, k = i - j * S1;
    sW1[i] = (j < n.H1 && k < K) ? P[n.W1 + j * K + k] : 0.f;
  }
  for (int i = tid; i < MG_H * MG_WSTRIDE; i += MG_THREADS) {
    const int j = i / MG_WSTRIDE, k = i - j * MG_WSTRIDE;
    sW2[i] = (n.nh == 2 && j < n.H2 && k < n.H1) ? P[n.W2 + j * n.H1 + k] : 0.f;
  }
  for (int i = tid; i < 16 * MG_WSTRIDE; i += MG_THREADS) {
    const int o = i / MG_WSTRIDE, k = i - o * MG_WSTRIDE;
    sWh[i] = (o < n.AO && k < HL) ? P[n.Wh + o * HL + k] : 0.f;
  }
  if (tid < 64) {
    sb1[tid] = tid < n.H1 ? P[n.b1 + tid] : 0.f;
    sb2[tid] = (n.nh == 2 && tid < n.H2) ? P[n.b2 + tid] : 0.f;
  } else if (tid < 80) {
    const int o = tid - 64;
    sbh[o] = o < n.AO ? P[n.bh + o] : 0.f;
    sls[o] = (n.kind == MG_GAUSS && o < n.AO) ? P[n.ls + o] : 0.f;
  }
  if (SDE)
    for (int i = tid; i < MG_H * 16; i += MG_THREADS) {
      const int h = i >> 4, c = i & 15;
      sE2[i] = (n.kind == MG_SDE && c < n.AO) ? exp(2. * (double)P[n.ls + h * n.AO + c]) : 0.;
    }

  double accW1[2][4][4], accW2[4][4], accWh[4], accb = 0.;
  for (int h = 0; h < 2; ++h)
    for (int jj = 0; jj < 4; ++jj)
      for (int kk = 0; kk < 4; ++kk) accW1[h][jj][kk] = 0.;
  for (int jj = 0; jj < 4; ++jj)
    for (int kk = 0; kk < 4; ++kk) accW2[jj][kk] = 0.;
  for (int c = 0; c < 4; ++c) accWh[c] = 0.;
  double accLs[4] = {0., 0., 0., 0.};      // SDE: sum over rows of d loss / d var[r][o] * latent[r][k0 + c]^2
  const int bj0 = (tid & 15) * 4, bk0 = (tid >> 4) * 4;      // this thread's 4 x 4 block of a 64 x 64 weight gradient
  double* const hl = n.nh == 2 ? sh2 : sh1;                  // what the head reads
  double* const sdz1 = n.nh == 2 ? sh2 : sdz;                // where d loss / d (first pre-activation) ends up

  for (int tile = blockIdx.x; tile * MG_ROWS < a.N; tile += gridDim.x) {
    const int row0 = tile * MG_ROWS;
    __syncthreads();      // the weights are in place / the previous tile is done with the images
    for (int i = tid; i < MG_ROWS * KP; i += MG_THREADS) {
      const int r = i / KP, k = i - r * KP, row = row0 + r;
      sx[i] = (row < a.N && k < K) ? a.x[(size_t)row * K + k] : 0.f;
    }
    if (tid < 32) {
      const int row = row0 + (tid & 15);
      const float* src = tid < 16 ? a.d_lp : a.d_ent;
      srow[tid] = (row < a.N && src != nullptr) ? src[row] : 0.f;
    }
    __syncthreads();
    // ---- forward
    mg_layer<RELU>(sW1, S1, sb1, sx, KP, KP, sh1, lane, wv);
    __syncthreads();
    if (n.nh == 2) {
      mg_layer<RELU>(sW2, MG_WSTRIDE, sb2, sh1, MG_ASTRIDE, MG_H, sh2, lane, wv);
      __syncthreads();
    }
    {
      const int o = tid >> 4, r = tid & 15;
      if (o < n.AO) {
        double acc = sbh[o];
        for (int k = 0; k < MG_H; ++k) acc = fma((double)sWh[o * MG_WSTRIDE + k], hl[r * MG_ASTRIDE + k], acc);
        so[r * 16 + o] = acc;
        if (SDE && n.kind == MG_SDE) {
          double var = 0.;
          for (int k = 0; k < MG_H; ++k) {
            const double l = hl[r * MG_ASTRIDE + k];
            var = fma(l * l, sE2[k * 16 + o], var);
          }
          sdf[r * 16 + o] = var + 1e-6;
        }
      }
    }
    __syncthreads();
    // ---- the head's outputs of row r, and d loss / d (head output) in their place (zero for a row beyond N)
    if (tid < MG_ROWS) {
      const int r = tid, row = row0 + r;
      const bool live = row < a.N;
      if (n.kind == MG_GAUSS) {      // distributions.py:143-161: Normal(mean, exp(log_std)).log_prob summed; entropy of the same scale
        const double dlp = srow[r], den = srow[16 + r];
        double lp = 0., en = 0.;
        for (int c = 0; c < n.AO; ++c) {
          const double ls = sls[c], sd = exp(ls), var = sd * sd;
          const double act = live ? (double)a.actions[(size_t)row * a.act_store + c] : 0.;
          const double diff = act - so[r * 16 + c];
          lp += -(diff * diff) / (2. * var) - ls - MG_LOG_SQRT_2PI;
          en += 0.5 + MG_LOG_SQRT_2PI + ls;
          so[r * 16 + c] = dlp * (diff / var);                               // d log_prob / d mean
          if constexpr (DIN) {                                               // d log_prob / d action = -d log_prob / d mean
            if (live && a.d_act != nullptr) a.d_act[(size_t)row * a.act_store + c] = (float)(-so[r * 16 + c]);
          }
          sdf[r * 16 + c] = dlp * (diff * diff / var - 1.) + den;          // d log_prob / d log_std, d entropy / d log_std = 1
        }
        if (live && a.lp != nullptr) a.lp[row] = (float)lp;
        if (live && a.ent != nullptr) a.ent[row] = (float)en;
      } else if (SDE && n.kind == MG_SDE) {      // distributions.py:525-562: Normal(mean, sqrt(var)), log_prob and entropy summed over the actions
        const double dlp = srow[r], den = srow[16 + r];
        double lp = 0., en = 0.;
        for (int c = 0; c < n.AO; ++c) {
          const double var = sdf[r * 16 + c], lsd = 0.5 * log(var);
          const double act = live ? (double)a.actions[(size_t)row * a.act_store + c] : 0.;
          const double diff = act - so[r * 16 + c];
          lp += -(diff * diff) / (2. * var) - lsd - MG_LOG_SQRT_2PI;
          en += 0.5 + MG_LOG_SQRT_2PI + lsd;
          so[r * 16 + c] = dlp * (diff / var);                                                  // d log_prob / d mean
          sdf[r * 16 + c] = dlp * ((diff * diff / var - 1.) / (2. * var)) + den / (2. * var);      // d log_prob / d var, d entropy / d var
        }
        if (live && a.lp != nullptr) a.lp[row] = (float)lp;
        if (live && a.ent != nullptr) a.ent[row] = (float)en;
      } else if (n.kind == MG_CATEG) {      // distributions.py:249-298: Categorical(logits)
        const double dlp = srow[r], den = srow[16 + r];
        int ai = live ? (int)a.actions[(size_t)row * a.act_store] : 0;
        ai = ai < 0 ? 0 : (ai >= n.AO ? n.AO - 1 : ai);
        double m = so[r * 16];
        for (int c = 1; c < n.AO; ++c) m = fmax(m, so[r * 16 + c]);
        double s = 0.;
        for (int c = 0; c < n.AO; ++c) s += exp(so[r * 16 + c] - m);
        const double lse = m + log(s);
        double en = 0.;
        for (int c = 0; c < n.AO; ++c) {
          const double lg = so[r * 16 + c] - lse;
          en -= exp(lg) * lg;
        }
        const double lp = so[r * 16 + ai] - lse;
        for (int c = 0; c < n.AO; ++c) {
          const double lg = so[r * 16 + c] - lse, p = exp(lg);
          so[r * 16 + c] = dlp * ((c == ai ? 1. : 0.) - p) - den * (p * (lg + en));      // d H / d logit_c = -p_c (log p_c + H)
        }
        if (live && a.lp != nullptr) a.lp[row] = (float)lp;
        if (live && a.ent != nullptr) a.ent[row] = (float)en;
      } else {
        const double d = (live && n.d_out != nullptr) ? (double)n.d_out[row] : 0.;
        double v = so[r * 16];
        if (n.kind == MG_ZETA) {
          v = 1. / (1. + exp(-v));
          so[r * 16] = d * (v * (1. - v));
        } else {
          so[r * 16] = d;
        }
        if (live && n.out != nullptr) n.out[row] = (float)v;
      }
    }
    if (a.part == nullptr) continue;      // forward only (uniform over the grid)
    __syncthreads();
    // ---- backward: head
    {
      const int o = tid >> 4, k0 = (tid & 15) * 4;
      if (o < n.AO)
        for (int r = 0; r < MG_ROWS; ++r) {
          const double d = so[r * 16 + o];
          double h[4];
          mg_load4(hl + r * MG_ASTRIDE + k0, h);
          for (int c = 0; c < 4; ++c) accWh[c] = fma(d, h[c], accWh[c]);
          if (SDE && n.kind == MG_SDE) {      // (the latent enters the variance as a constant: nothing goes back into it from here)
            const double dv = sdf[r * 16 + o];
            for (int c = 0; c < 4; ++c) accLs[c] = fma(dv, h[c] * h[c], accLs[c]);
          }
        }
      if (tid >= 128 && tid < 144 && tid - 128 < n.AO)
        for (int r = 0; r < MG_ROWS; ++r) accb += so[r * 16 + tid - 128];
      if (tid >= 144 && tid < 160 && tid - 144 < n.AO && n.kind == MG_GAUSS)
        for (int r = 0; r < MG_ROWS; ++r) accb += sdf[r * 16 + tid - 144];
      for (int q = 0; q < 4; ++q) {
        const int r = 4 * wv + q;
        double d = 0.;
        for (int c = 0; c < n.AO; ++c) d = fma(so[r * 16 + c], (double)sWh[c * MG_WSTRIDE + lane], d);
        sdz[r * MG_ASTRIDE + lane] = d * mg_dact<RELU>(hl[r * MG_ASTRIDE + lane]);
      }
    }
    __syncthreads();
    // ---- second hidden layer
    if (n.nh == 2) {
      mg_outer(accW2, sdz, bj0, sh1, MG_ASTRIDE, bk0);
      if (tid >= 64 && tid < 128)
        for (int r = 0; r < MG_ROWS; ++r) accb += sdz[r * MG_ASTRIDE + tid - 64];
      double d[4] = {0., 0., 0., 0.};
      for (int j = 0; j < MG_H; ++j) {
        const double w = sW2[j * MG_WSTRIDE + lane];
        for (int q = 0; q < 4; ++q) d[q] = fma(sdz[(4 * wv + q) * MG_ASTRIDE + j], w, d[q]);
      }
      for (int q = 0; q < 4; ++q) {      // (h2 was last read before the barrier above: its image takes the next gradient)
        const int r = 4 * wv + q;
        sdz1[r * MG_ASTRIDE + lane] = d[q] * mg_dact<RELU>(sh1[r * MG_ASTRIDE + lane]);
      }
      __syncthreads();
    }
    // ---- first hidden layer
#pragma unroll
    for (int h = 0; h < 2; ++h)
      if (bk0 + 64 * h < KP) mg_outer(accW1[h], sdz1, bj0, sx, KP, bk0 + 64 * h);
    if (tid < 64)
      for (int r = 0; r < MG_ROWS; ++r) accb += sdz1[r * MG_ASTRIDE + tid];
    // ---- d loss / d x of the tile's rows: sdz1 and sW1 are read only until the next tile's top barrier; the padding columns k >= K of sW1
    // are zero and not written, rows at or beyond N are not written
    if constexpr (DIN) {
      if (a.dx64 != nullptr || a.dx32 != nullptr)
        for (int i = tid; i < MG_ROWS * KP; i += MG_THREADS) {
          const int r = i / KP, k = i - r * KP, row = row0 + r;
          if (k >= K || row >= a.N) continue;
          double acc = 0.;
          for (int j = 0; j < n.H1; ++j) acc = fma(sdz1[r * MG_ASTRIDE + j], (double)sW1[j * S1 + k], acc);
          if (a.dx64 != nullptr) a.dx64[((size_t)blockIdx.y * a.N + row) * K + k] = acc;
          else a.dx32[(size_t)row * K + k] = (float)acc;
        }
    }
  }
  if (a.part == nullptr) return;

  // ---- this workgroup's sums -> its slice (every entry of the network's tensors is written, zeros included)
  double* dst = a.part + (size_t)blockIdx.x * a.n_params;
  for (int h = 0; h < 2; ++h)
    for (int jj = 0; jj < 4; ++jj)
      for (int kk = 0; kk < 4; ++kk) {
        const int j = bj0 + jj, k = bk0 + 64 * h + kk;
        if (j < n.H1 && k < K) dst[n.W1 + j * K + k] = accW1[h][jj][kk];
      }
  if (n.nh == 2)
    for (int jj = 0; jj < 4; ++jj)
      for (int kk = 0; kk < 4; ++kk) {
        const int j = bj0 + jj, k = bk0 + kk;
        if (j < n.H2 && k < n.H1) dst[n.W2 + j * n.H1 + k] = accW2[jj][kk];
      }
  {
    const int o = tid >> 4, k0 = (tid & 15) * 4;
    if (o < n.AO)
      for (int c = 0; c < 4; ++c)
        if (k0 + c < HL) dst[n.Wh + o * HL + k0 + c] = accWh[c];
    // d var / d log_std[h][o] = 2 latent_h^2 exp(2 log_std[h][o]); all MG_H stored rows (a padded latent unit is exactly 0: so is its row)
    if (SDE && n.kind == MG_SDE && o < n.AO)
      for (int c = 0; c < 4; ++c) dst[n.ls + (k0 + c) * n.AO + o] = 2. * sE2[(k0 + c) * 16 + o] * accLs[c];
  }
  if (tid < 64) { if (tid < n.H1) dst[n.b1 + tid] = accb; }
  else if (tid < 128) { if (n.nh == 2 && tid - 64 < n.H2) dst[n.b2 + tid - 64] = accb; }
  else if (tid < 144) { if (tid - 128 < n.AO) dst[n.bh + tid - 128] = accb; }
  else if (tid < 160) { if (n.kind == MG_GAUSS && tid - 144 < n.AO) dst[n.ls + tid - 144] = accb; }
}

// grad[i] = (float)(part[0][i] + part[1][i] + ...) in that order
__global__ void __launch_bounds__(256) mlp_grad_fold_kernel(const double* __restrict__ part, int n_parts, int n, float* __restrict__ grad) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double s = part[i];
  for (int p = 1; p < n_parts; ++p) s += part[(size_t)p * n + i];
  grad[i] = (float)s;
}

// d_obs[i] = (float)(dx[0][i] + dx[1][i] + dx[2][i]): pi, vf, cvf in that order
__global__ void __launch_bounds__(256) mlp_dx_fold_kernel(const double* __restrict__ dx, long long n, float* __restrict__ d_obs) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  d_obs[i] = (float)((dx[i] + dx[n + i]) + dx[2 * n + i]);
}

// [N, cols] of the source columns of icrl_cn_prepare: column s < obs_dim an observation, obs_dim + k an action (continuous nets only).
// sum over the selected positions i with select_dim[i] == s of d_x[n][i], ascending i, float64; then the clip's derivative (1 inside the
// closed interval, as torch.clamp) and, for a normalised observation, 1 / sqrt(var + eps): the order of autograd through prepare_data
__global__ void __launch_bounds__(256) cn_prepare_bwd_kernel(icrl_costnet_t cn, const double* __restrict__ obs, const float* __restrict__ acs, int N,
                                                             const float* __restrict__ d_x, double* __restrict__ d_obs, float* __restrict__ d_acs) {
  const int cols = cn.obs_dim + (d_acs != nullptr ? cn.acs_dim : 0);
  const long long total = (long long)N * cols;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const int n = (int)(idx / cols), s = (int)(idx - (long long)n * cols);
    if (s < cn.obs_dim && d_obs == nullptr) continue;
    const float* g = d_x + (size_t)n * cn.in_dim;
    double acc = 0.;
    for (int i = 0; i < cn.in_dim; ++i)
      if (cn.select_dim[i] == s) acc += (double)g[i];
    if (s < cn.obs_dim) {
      double o = obs[(size_t)n * cn.obs_dim + s], scale = 1.;
      if (cn.obs_mean != nullptr && cn.obs_var != nullptr) {
        const double sd = sqrt(cn.obs_var[s] + cn.eps);
        o = (o - cn.obs_mean[s]) / sd;
        scale = 1. / sd;
      }
      if (cn.clip_obs >= 0.0 && !(o >= -cn.clip_obs && o <= cn.clip_obs)) acc = 0.;
      d_obs[(size_t)n * cn.obs_dim + s] = acc * scale;
    } else {
      const int k = s - cn.obs_dim;
      const float x = acs[(size_t)n * cn.acs_dim + k];
      if (cn.action_low != nullptr && cn.action_high != nullptr && !(x >= cn.action_low[k] && x <= cn.action_high[k])) acc = 0.;
      d_acs[(size_t)n * cn.acs_dim + k] = (float)acc;
    }
  }
}

template <bool RELU, bool SDE = false>
int mg_launch(MgArgs& a, int n_nets, int max_k, float* grad, void* ws, hipStream_t s) {
  const int parts = mg_parts(a.N);
  const bool bwd = grad != nullptr;
  a.part = bwd ? (double*)ws : nullptr;
  const size_t lds = mg_lds_bytes(max_k, SDE);
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)mlp_fwd_bwd_kernel<RELU, SDE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL((mlp_fwd_bwd_kernel<RELU, SDE>), dim3(parts, n_nets), dim3(MG_THREADS), lds, s, a);
  if (bwd) hipLaunchKernelGGL(mlp_grad_fold_kernel, dim3((a.n_params + 255) / 256), dim3(256), 0, s, (const double*)ws, parts, a.n_params, grad);
  return (int)hipGetLastError();
}

// the `_in` forms: ws = the partial sums of the parameters (always written; folded into grad when it is asked for), then, for the policy's
// d_obs, three float64 slices [N][K]
template <bool RELU>
int mg_launch_in(MgArgsIn& a, int n_nets, int max_k, float* grad, float* d_x, void* ws, hipStream_t s) {
  const int parts = mg_parts(a.N);
  a.part = (double*)ws;
  a.dx64 = (n_nets == 3 && d_x != nullptr) ? (double*)ws + (size_t)parts * a.n_params : nullptr;
  a.dx32 = n_nets == 1 ? d_x : nullptr;
  const size_t lds = mg_lds_bytes(max_k, false);
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)mlp_fwd_bwd_kernel<RELU, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL((mlp_fwd_bwd_kernel<RELU, false, true>), dim3(parts, n_nets), dim3(MG_THREADS), lds, s, a);
  if (grad != nullptr) hipLaunchKernelGGL(mlp_grad_fold_kernel, dim3((a.n_params + 255) / 256), dim3(256), 0, s, (const double*)ws, parts, a.n_params, grad);
  if (a.dx64 != nullptr) {
    const long long n = (long long)a.N * max_k;
    hipLaunchKernelGGL(mlp_dx_fold_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const double*)a.dx64, n, d_x);
  }
  return (int)hipGetLastError();
}

inline long long mg_policy_in_ws(const icrl_policy_t* pol, int N) {
  return ((long long)mg_parts(N) * pol->n_params + 3LL * N * pol->obs_dim) * (long long)sizeof(double);
}

// 0, or the fail() code of a policy these entry points do not serve
int mg_policy_check(const char* who, const icrl_policy_t* p, int N, bool sde = false) {
  if (p == nullptr) return fail("%s: NULL policy descriptor", who);
  if (p->arch != nullptr)
    return fail("%s: a policy described by an `arch` array is not served (arch == NULL, two hidden layers per branch with h1 == h2 <= %d)", who, MAX_H);
  if (p->h1 != p->h2 || p->h1 < 1 || p->h1 > MAX_H)
    return fail("%s: hidden widths (%d, %d) are not served (h1 == h2 <= %d; narrower layers are stored zero-padded)", who, p->h1, p->h2, MAX_H);
  if (p->obs_dim < 1 || p->obs_dim > MAX_OBS) return fail("%s: obs_dim %d (1..%d)", who, p->obs_dim, MAX_OBS);
  if (p->act_dim < 1 || p->act_dim > MAX_ACT) return fail("%s: act_dim %d (1..%d)", who, p->act_dim, MAX_ACT);
  if (N < 1 || N > MG_MAX_N) return fail("%s: N = %d rows (1..%d)", who, N, MG_MAX_N);
  if (sde && p->discrete) return fail("%s: a discrete policy has no gSDE head (Box action spaces only)", who);
  const PolLayout L = sde ? make_sde_layout(p->obs_dim, p->act_dim, p->h1, p->h2) : make_pol_layout(p->obs_dim, p->act_dim, p->h1, p->h2, p->discrete);
  if (p->n_params != L.n)
    return fail("%s: n_params %d, the %slayout of (%d, %d, %d, %d) has %d", who, p->n_params, sde ? "gSDE (log_std [64, act_dim]) " : "", p->obs_dim, p->act_dim,
                p->h1, p->h2, L.n);
  return 0;
}

int mg_costnet_check(const char* who, const icrl_costnet_t* cn, int N) {
  if (cn == nullptr) return fail("%s: NULL constraint-net descriptor", who);
  if (as_cost_fn(cn)) return refuse_cost_fn(who);
  if (as_cost_disc(cn)) return refuse_cost_disc(who);
  if (as_cost_region(cn)) return refuse_cost_region(who);
  if (cn->n_hidden < 1 || cn->n_hidden > 2) return fail("%s: %d hidden layers are not served (1..2 of up to %d units)", who, cn->n_hidden, MAX_H);
  if (cn->h1 < 1 || cn->h1 > MAX_H || (cn->n_hidden == 2 && (cn->h2 < 1 || cn->h2 > MAX_H)))
    return fail("%s: hidden layers (%d, %d) are not served (1..2 of up to %d units)", who, cn->h1, cn->n_hidden == 2 ? cn->h2 : 0, MAX_H);
  if (cn->in_dim < 1 || cn->in_dim > MAX_OBS) return fail("%s: in_dim %d (1..%d)", who, cn->in_dim, MAX_OBS);
  if (N < 1 || N > MG_MAX_N) return fail("%s: N = %d rows (1..%d)", who, N, MG_MAX_N);
  const CnLayout L = make_cn_layout(cn->in_dim, cn->n_hidden, cn->h1, cn->h2);
  if (cn->n_params != L.n) return fail("%s: n_params %d, the layout of %d inputs and (%d, %d) has %d", who, cn->n_params, cn->in_dim, cn->h1, cn->n_hidden == 2 ? cn->h2 : 0, L.n);
  return 0;
}

}  // namespace

// ---- the gSDE head behind icrl_policy_sde_fwd_bwd (sde.hip: the exported entry points)
int sde_fwd_bwd_check(const char* who, const icrl_policy_t* p, int N) { return mg_policy_check(who, p, N, true); }
int sde_fwd_bwd_parts(int N) { return mg_parts(N); }
int launch_sde_fwd_bwd(const icrl_policy_t* pol, const float* obs, const float* actions, int N, const float* d_v_r, const float* d_v_c, const float* d_log_prob,
                       const float* d_entropy, float* v_r, float* v_c, float* log_prob, float* entropy, float* grad, void* ws, hipStream_t s) {
  const PolLayout L = make_sde_layout(pol->obs_dim, pol->act_dim, pol->h1, pol->h2);
  MgArgs a = {};
  for (int b = 0; b < 3; ++b) {
    MgNet& n = a.net[b];
    n.K = L.O; n.H1 = L.H1; n.H2 = L.H2; n.nh = 2;
    n.W1 = L.W1[b]; n.b1 = L.b1[b]; n.W2 = L.W2[b]; n.b2 = L.b2[b]; n.ls = L.log_std;
  }
  a.net[0].AO = L.A; a.net[0].kind = MG_SDE; a.net[0].Wh = L.Wa; a.net[0].bh = L.ba;
  a.net[1].AO = 1; a.net[1].kind = MG_VALUE; a.net[1].Wh = L.Wv; a.net[1].bh = L.bv; a.net[1].d_out = d_v_r; a.net[1].out = v_r;
  a.net[2].AO = 1; a.net[2].kind = MG_VALUE; a.net[2].Wh = L.Wc; a.net[2].bh = L.bc; a.net[2].d_out = d_v_c; a.net[2].out = v_c;
  a.params = pol->params; a.x = obs; a.actions = actions; a.act_store = L.A; a.N = N; a.n_params = L.n;
  a.d_lp = d_log_prob; a.d_ent = d_entropy; a.lp = log_prob; a.ent = entropy;
  return mg_launch<false, true>(a, 3, L.O, grad, ws, s);
}

}  // namespace icrl

using namespace icrl;

extern "C" size_t icrl_policy_fwd_bwd_ws_bytes(const icrl_policy_t* pol, int N) {
  if (mg_policy_check("icrl_policy_fwd_bwd_ws_bytes", pol, N) != 0) return 0;
  return (size_t)mg_parts(N) * (size_t)pol->n_params * sizeof(double);
}

extern "C" int icrl_policy_fwd_bwd(const icrl_policy_t* pol, const float* obs, const float* actions, int N, const float* d_v_r, const float* d_v_c,
                                   const float* d_log_prob, const float* d_entropy, float* v_r, float* v_c, float* log_prob, float* entropy, float* grad,
                                   void* ws, long long ws_bytes, void* stream) {
  const char* who = "icrl_policy_fwd_bwd";
  if (const int e = mg_policy_check(who, pol, N)) return e;
  if (pol->params == nullptr || obs == nullptr || actions == nullptr) return fail("%s: NULL argument (pol->params, obs and actions are required)", who);
  if (grad == nullptr && (d_v_r != nullptr || d_v_c != nullptr || d_log_prob != nullptr || d_entropy != nullptr))
    return fail("%s: upstream gradients without `grad` (grad NULL = forward only: pass no d_* then)", who);
  const long long need = (long long)mg_parts(N) * pol->n_params * (long long)sizeof(double);
  if (grad != nullptr && (ws == nullptr || ws_bytes < need))
    return fail("%s: ws of %lld bytes, icrl_policy_fwd_bwd_ws_bytes(pol, %d) = %lld", who, ws == nullptr ? 0LL : ws_bytes, N, need);
  const PolLayout L = make_pol_layout(pol->obs_dim, pol->act_dim, pol->h1, pol->h2, pol->discrete);
  MgArgs a = {};
  for (int b = 0; b < 3; ++b) {
    MgNet& n = a.net[b];
    n.K = L.O; n.H1 = L.H1; n.H2 = L.H2; n.nh = 2;
    n.W1 = L.W1[b]; n.b1 = L.b1[b]; n.W2 = L.W2[b]; n.b2 = L.b2[b]; n.ls = L.log_std;
  }
  a.net[0].AO = L.A; a.net[0].kind = pol->discrete ? MG_CATEG : MG_GAUSS; a.net[0].Wh = L.Wa; a.net[0].bh = L.ba;
  a.net[1].AO = 1; a.net[1].kind = MG_VALUE; a.net[1].Wh = L.Wv; a.net[1].bh = L.bv; a.net[1].d_out = d_v_r; a.net[1].out = v_r;
  a.net[2].AO = 1; a.net[2].kind = MG_VALUE; a.net[2].Wh = L.Wc; a.net[2].bh = L.bc; a.net[2].d_out = d_v_c; a.net[2].out = v_c;
  a.params = pol->params; a.x = obs; a.actions = actions; a.act_store = pol->discrete ? 1 : L.A; a.N = N; a.n_params = L.n;
  a.d_lp = d_log_prob; a.d_ent = d_entropy; a.lp = log_prob; a.ent = entropy;
  return mg_launch<false>(a, 3, L.O, grad, ws, (hipStream_t)stream);
}

extern "C" size_t icrl_cost_mlp_fwd_bwd_ws_bytes(const icrl_costnet_t* cn, int N) {
  if (mg_costnet_check("icrl_cost_mlp_fwd_bwd_ws_bytes", cn, N) != 0) return 0;
  return (size_t)mg_parts(N) * (size_t)cn->n_params * sizeof(double);
}

extern "C" int icrl_cost_mlp_fwd_bwd(const icrl_costnet_t* cn, const float* x, int N, const float* d_zeta, float* zeta, float* grad, void* ws,
                                     long long ws_bytes, void* stream) {
  const char* who = "icrl_cost_mlp_fwd_bwd";
  if (const int e = mg_costnet_check(who, cn, N)) return e;
  if (cn->params == nullptr || x == nullptr) return fail("%s: NULL argument (cn->params and x are required)", who);
  if ((d_zeta == nullptr) != (grad == nullptr)) return fail("%s: d_zeta and grad go together (both NULL = forward only)", who);
  const long long need = (long long)mg_parts(N) * cn->n_params * (long long)sizeof(double);
  if (grad != nullptr && (ws == nullptr || ws_bytes < need))
    return fail("%s: ws of %lld bytes, icrl_cost_mlp_fwd_bwd_ws_bytes(cn, %d) = %lld", who, ws == nullptr ? 0LL : ws_bytes, N, need);
  const CnLayout L = make_cn_layout(cn->in_dim, cn->n_hidden, cn->h1, cn->h2);
  MgArgs a = {};
  MgNet& n = a.net[0];
  n.K = L.in; n.H1 = L.H1; n.H2 = L.H2; n.AO = 1; n.nh = L.nh; n.kind = MG_ZETA;
  n.W1 = L.W0; n.b1 = L.b0; n.W2 = L.W1; n.b2 = L.b1; n.Wh = L.Wo; n.bh = L.bo; n.ls = -1;
  n.d_out = d_zeta; n.out = zeta;
  a.params = cn->params; a.x = x; a.N = N; a.n_params = L.n;
  return mg_launch<true>(a, 1, L.in, grad, ws, (hipStream_t)stream);
}

// ---- the same two calls with the gradients of the inputs (DIN)
extern "C" size_t icrl_policy_fwd_bwd_in_ws_bytes(const icrl_policy_t* pol, int N) {
  if (mg_policy_check("icrl_policy_fwd_bwd_in_ws_bytes", pol, N) != 0) return 0;
  return (size_t)mg_policy_in_ws(pol, N);
}

extern "C" int icrl_policy_fwd_bwd_in(const icrl_policy_t* pol, const float* obs, const float* actions, int N, const float* d_v_r, const float* d_v_c,
                                      const float* d_log_prob, const float* d_entropy, float* v_r, float* v_c, float* log_prob, float* entropy, float* grad,
                                      float* d_obs, float* d_actions, void* ws, long long ws_bytes, void* stream) {
  const char* who = "icrl_policy_fwd_bwd_in";
  if (const int e = mg_policy_check(who, pol, N)) return e;
  if (pol->params == nullptr || obs == nullptr || actions == nullptr) return fail("%s: NULL argument (pol->params, obs and actions are required)", who);
  if (grad == nullptr && d_obs == nullptr && d_actions == nullptr)
    return fail("%s: no gradient output (grad, d_obs and d_actions are all NULL: icrl_policy_fwd_bwd is the forward-only call)", who);
  if (d_actions != nullptr && pol->discrete)
    return fail("%s: d_actions with a discrete policy (a class index has no gradient: pass NULL)", who);
  const long long need = mg_policy_in_ws(pol, N);
  if (ws == nullptr || ws_bytes < need)
    return fail("%s: ws of %lld bytes, icrl_policy_fwd_bwd_in_ws_bytes(pol, %d) = %lld", who, ws == nullptr ? 0LL : ws_bytes, N, need);
  const PolLayout L = make_pol_layout(pol->obs_dim, pol->act_dim, pol->h1, pol->h2, pol->discrete);
  MgArgsIn a = {};
  for (int b = 0; b < 3; ++b) {
    MgNet& n = a.net[b];
    n.K = L.O; n.H1 = L.H1; n.H2 = L.H2; n.nh = 2;
    n.W1 = L.W1[b]; n.b1 = L.b1[b]; n.W2 = L.W2[b]; n.b2 = L.b2[b]; n.ls = L.log_std;
  }
  a.net[0].AO = L.A; a.net[0].kind = pol->discrete ? MG_CATEG : MG_GAUSS; a.net[0].Wh = L.Wa; a.net[0].bh = L.ba;
  a.net[1].AO = 1; a.net[1].kind = MG_VALUE; a.net[1].Wh = L.Wv; a.net[1].bh = L.bv; a.net[1].d_out = d_v_r; a.net[1].out = v_r;
  a.net[2].AO = 1; a.net[2].kind = MG_VALUE; a.net[2].Wh = L.Wc; a.net[2].bh = L.bc; a.net[2].d_out = d_v_c; a.net[2].out = v_c;
  a.params = pol->params; a.x = obs; a.actions = actions; a.act_store = pol->discrete ? 1 : L.A; a.N = N; a.n_params = L.n;
  a.d_lp = d_log_prob; a.d_ent = d_entropy; a.lp = log_prob; a.ent = entropy;
  a.d_act = d_actions;
  return mg_launch_in<false>(a, 3, L.O, grad, d_obs, ws, (hipStream_t)stream);
}

extern "C" size_t icrl_cost_mlp_fwd_bwd_in_ws_bytes(const icrl_costnet_t* cn, int N) {
  if (mg_costnet_check("icrl_cost_mlp_fwd_bwd_in_ws_bytes", cn, N) != 0) return 0;
  return (size_t)mg_parts(N) * (size_t)cn->n_params * sizeof(double);
}

extern "C" int icrl_cost_mlp_fwd_bwd_in(const icrl_costnet_t* cn, const float* x, int N, const float* d_zeta, float* zeta, float* grad, float* d_x, void* ws,
                                        long long ws_bytes, void* stream) {
  const char* who = "icrl_cost_mlp_fwd_bwd_in";
  if (const int e = mg_costnet_check(who, cn, N)) return e;
  if (cn->params == nullptr || x == nullptr) return fail("%s: NULL argument (cn->params and x are required)", who);
  if (grad == nullptr && d_x == nullptr)
    return fail("%s: no gradient output (grad and d_x are both NULL: icrl_cost_mlp_fwd_bwd is the forward-only call)", who);
  if (d_zeta == nullptr) return fail("%s: d_zeta is required (d loss / d zeta per row)", who);
  const long long need = (long long)mg_parts(N) * cn->n_params * (long long)sizeof(double);
  if (ws == nullptr || ws_bytes < need)
    return fail("%s: ws of %lld bytes, icrl_cost_mlp_fwd_bwd_in_ws_bytes(cn, %d) = %lld", who, ws == nullptr ? 0LL : ws_bytes, N, need);
  const CnLayout L = make_cn_layout(cn->in_dim, cn->n_hidden, cn->h1, cn->h2);
  MgArgsIn a = {};
  MgNet& n = a.net[0];
  n.K = L.in; n.H1 = L.H1; n.H2 = L.H2; n.AO = 1; n.nh = L.nh; n.kind = MG_ZETA;
  n.W1 = L.W0; n.b1 = L.b0; n.W2 = L.W1; n.b2 = L.b1; n.Wh = L.Wo; n.bh = L.bo; n.ls = -1;
  n.d_out = d_zeta; n.out = zeta;
  a.params = cn->params; a.x = x; a.N = N; a.n_params = L.n;
  return mg_launch_in<true>(a, 1, L.in, grad, d_x, ws, (hipStream_t)stream);
}

extern "C" int icrl_cn_prepare_bwd(const icrl_costnet_t* cn, const double* obs, const float* acs, int N, const float* d_x, double* d_obs, float* d_acs,
                                   void* stream) {
  const char* who = "icrl_cn_prepare_bwd";
  if (cn == nullptr) return fail("%s: NULL constraint-net descriptor", who);
  if (as_cost_fn(cn)) return refuse_cost_fn(who);
  if (as_cost_disc(cn)) return refuse_cost_disc(who);
  if (as_cost_region(cn)) return refuse_cost_region(who);
  if (N <= 0) return fail("%s: N = %d rows", who, N);
  if (cn->in_dim < 1 || cn->obs_dim < 1 || cn->acs_dim < 1) return fail("%s: in_dim %d, obs_dim %d, acs_dim %d (each >= 1)", who, cn->in_dim, cn->obs_dim, cn->acs_dim);
  if (d_obs == nullptr && d_acs == nullptr) return fail("%s: no gradient output (d_obs and d_acs are both NULL)", who);
  if (d_acs != nullptr && cn->is_discrete) return fail("%s: d_acs with a discrete net (a class index has no gradient: pass NULL)", who);
  if (d_x == nullptr || cn->select_dim == nullptr || (d_obs != nullptr && obs == nullptr) || (d_acs != nullptr && acs == nullptr))
    return fail("%s: NULL argument (d_x and cn->select_dim are required; obs with d_obs, acs with d_acs)", who);
  const long long total = (long long)N * (cn->obs_dim + (d_acs != nullptr ? cn->acs_dim : 0));
  const long long blocks = (total + 255) / 256;
  hipLaunchKernelGGL(cn_prepare_bwd_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, (hipStream_t)stream, *cn, obs, acs, N, d_x, d_obs, d_acs);
  return (int)hipGetLastError();
}
