// The statements of the column-split tiles kernel (csrc/ppo_train_tiles.hip: mapping, LDS layout, the two __global__ shells that include
// this text and why they include it).  No header of its own: it is written inside a kernel, against NT1 (obs tiles), HEAD (HEAD_GAUSS /
// HEAD_CAT / HEAD_SDE) and the argument block `TrainArgs a`.  What differs between the heads is an `if constexpr` region or a condition
// on HEAD / SDE; everything else is the one common text.
  using S = Smem<NT1, HEAD>;
  constexpr bool SDE = HEAD == HEAD_SDE;
  constexpr int SX = S::SX;
  constexpr int NT1H = NT1 / 2;     // W1 / dW1 column tiles per wave
  constexpr int XR = (SX + 7) / 8;  // floats of an X row each of the 8 threads of a row stages
  static_assert(NT1 >= 2, "obs tiles are split between the two column halves");
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int role = blockIdx.x;  // 0 policy, 1 reward critic, 2 cost critic
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int rt = w & 3, hf = w >> 2;
  const int r = lane & 15, q = lane >> 4;
  const PolLayout& L = a.L;
  const int O = L.O, A = L.A;
  const int n_out = role == 0 ? A : 1;
  const int T = a.buf.T, N = a.buf.N;
  const int n_total = T * N;
  const int B = a.hp.batch_size;
  const int n_mb = (n_total + B - 1) / B;
  const int n_epochs = a.hp.n_epochs;
  const float nu = a.nu[0];
  const bool ls_owner = SDE && role == 0 && hf == 1;   // gSDE: this wave owns log_std rows 16rt..16rt+15 (C-layout: row 16rt + r, action 4q + i)

  // ---- global offsets of this role's tensors in the flat parameter buffer
  const int gW1 = L.W1[role], gb1 = L.b1[role], gW2 = L.W2[role], gb2 = L.b2[role];
  const int gWh = role == 0 ? L.Wa : (role == 1 ? L.Wv : L.Wc);
  const int gbh = role == 0 ? L.ba : (role == 1 ? L.bv : L.bc);

  // ---- load weights into LDS (zero padded), moments into registers (C-layout ownership)
  for (int i = tid; i < HD * SX; i += TH) { const int j = i / SX, k = i % SX; sm[S::W1 + i] = k < O ? a.params[gW1 + j * O + k] : 0.f; }
  for (int i = tid; i < HD * SH; i += TH) { const int j = i / SH, k = i % SH; sm[S::W2 + i] = k < HD ? a.params[gW2 + j * HD + k] : 0.f; }
  for (int i = tid; i < 16 * SH; i += TH) {
    const int o = i / SH, k = i % SH;
    sm[S::WH + i] = (o < n_out && k < HD) ? a.params[gWh + o * HD + k] : 0.f;
    if constexpr (SDE) sm[S::E2T + i] = (role == 0 && o < A && k < HD) ? expf(2.f * a.params[L.log_std + k * A + o]) : 0.f;
  }
  if (tid < HD) { sm[S::B1 + tid] = a.params[gb1 + tid]; sm[S::B2 + tid] = a.params[gb2 + tid]; }
  if (tid < 16) {
    sm[S::BH + tid] = tid < n_out ? a.params[gbh + tid] : 0.f;
    if constexpr (!SDE) sm[S::LS + tid] = (HEAD == HEAD_GAUSS && role == 0 && tid < A) ? a.params[L.log_std + tid] : 0.f;
  }

  // wave (rt, hf) owns: W1 rows 16rt.. x column tiles hf*NT1H..; W2 rows 16rt.. x column tiles 2hf, 2hf+1;
  // (hf == 0 only) head-weight columns 16rt..16rt+15; (gSDE: hf == 1, policy only) log_std rows 16rt..16rt+15
  f32x4 mW1[NT1H], vW1[NT1H], gW1r[NT1H], mW2[2], vW2[2], gW2r[2], mWh, vWh, gWhr;
  f32x4 pLs, mLs, vLs, gLs;   // gSDE
#pragma unroll
  for (int c = 0; c < NT1H; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = 16 * rt + 4 * q + i, k = 16 * (hf * NT1H + c) + r;
      mW1[c][i] = k < O ? a.exp_avg[gW1 + j * O + k] : 0.f;
      vW1[c][i] = k < O ? a.exp_avg_sq[gW1 + j * O + k] : 0.f;
    }
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = 16 * rt + 4 * q + i, k = 16 * (2 * hf + c) + r;
      mW2[c][i] = a.exp_avg[gW2 + j * HD + k];
      vW2[c][i] = a.exp_avg_sq[gW2 + j * HD + k];
    }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int o = 4 * q + i, j = 16 * rt + r;
    const bool own = hf == 0 && o < n_out;
    mWh[i] = own ? a.exp_avg[gWh + o * HD + j] : 0.f;
    vWh[i] = own ? a.exp_avg_sq[gWh + o * HD + j] : 0.f;
    if constexpr (SDE) {
      const bool lown = ls_owner && o < A;
      pLs[i] = lown ? a.params[L.log_std + j * A + o] : 0.f;
      mLs[i] = lown ? a.exp_avg[L.log_std + j * A + o] : 0.f;
      vLs[i] = lown ? a.exp_avg_sq[L.log_std + j * A + o] : 0.f;
    }
  }
  // thread-owned vector parameters: tid 0..63 b1, 64..127 b2, 128..143 head bias, 144..159 log_std (diagonal head, policy only)
  int vec_g = -1, vec_s = 0;
  if (tid < 64) { vec_g = gb1 + tid; vec_s = S::B1 + tid; }
  else if (tid < 128) { vec_g = gb2 + tid - 64; vec_s = S::B2 + tid - 64; }
  else if (tid < 144) { if (tid - 128 < n_out) { vec_g = gbh + tid - 128; vec_s = S::BH + tid - 128; } }
  else if (tid < 160) { if (HEAD == HEAD_GAUSS && role == 0 && tid - 144 < A) { vec_g = L.log_std + tid - 144; vec_s = S::LS + tid - 144; } }
  float mB = 0.f, vB = 0.f, gB = 0.f;
  if (vec_g >= 0) { mB = a.exp_avg[vec_g]; vB = a.exp_avg_sq[vec_g]; }

  const int t0 = a.adam_t[0];
  double b1pow = pow((double)a.hp.adam_beta1, (double)t0), b2pow = pow((double)a.hp.adam_beta2, (double)t0);
  const float w1 = (float)(1.0 - (double)a.hp.adam_beta1);
  const float w2 = (float)(1.0 - (double)a.hp.adam_beta2);
  const float clip = a.hp.clip_range;
  const float vclip = role == 1 ? a.hp.clip_range_reward_vf : a.hp.clip_range_cost_vf;
  const float vcoef = role == 1 ? a.hp.reward_vf_coef : a.hp.cost_vf_coef;

  // ---------------------------------------------------------------------------------------------------------------
  // row stream helpers
  // ---------------------------------------------------------------------------------------------------------------
  auto cur_rows = [&](const Cursor& c) {   // rows of the 64-row chunk that starts at c
    int left = B - c.m;
    if (n_total - c.p < left) left = n_total - c.p;
    return left < RB ? left : RB;
  };
  auto cur_advance = [&](Cursor c) {
    const int rows = cur_rows(c);
    c.p += rows; c.m += rows;
    if (c.p >= n_total) { c.p = 0; c.m = 0; ++c.e; }
    else if (c.m >= B) c.m = 0;
    return c;
  };
  // flat env-major index -> [T,N] storage offset (ref: buffers.py:53-65): env = idx / T, t = idx % T
  auto to_off = [&](int idx) -> unsigned {
    unsigned env = __umulhi((unsigned)idx, a.t_magic);
    int t = idx - (int)env * T;
    if (t >= T) { t -= T; ++env; }
    if (t >= T) { t -= T; ++env; }
    return (unsigned)t * (unsigned)N + env;
  };
  // this thread's row of a chunk: b = tid/8 (part = tid%8 splits the row's floats)
  const int gb_row = tid >> 3, gpart = tid & 7;
  auto load_idx = [&](const Cursor& c) -> int {
    if (c.e >= n_epochs || gb_row >= cur_rows(c)) return -1;
    return a.perms[(size_t)c.e * n_total + c.p + gb_row];
  };
  // row data of one chunk held in registers between "issue" and "commit"
  float px[XR], pact[2], psc0 = 0.f, psc1 = 0.f, psc2 = 0.f;
  auto issue_rows = [&](int idx) {
    const bool valid = idx >= 0;
    const size_t off = valid ? (size_t)to_off(idx) : 0;
    const float* orow = a.buf.observations + off * O;
#pragma unroll
    for (int i = 0; i < XR; ++i) { const int k = gpart + 8 * i; px[i] = (valid && k < O) ? orow[k] : 0.f; }
    if (role == 0) {
      const float* arow = a.buf.actions + off * a.buf.act_store;
#pragma unroll
      for (int i = 0; i < 2; ++i) { const int k = gpart + 8 * i; pact[i] = (valid && k < a.buf.act_store) ? arow[k] : 0.f; }
      if (gpart == 0) {
        psc0 = valid ? a.buf.log_probs[off] : 0.f;
        psc1 = valid ? a.buf.reward_advantages[off] : 0.f;
        psc2 = valid ? a.buf.cost_advantages[off] : 0.f;
      }
    } else if (gpart == 0) {
      const float* rets = role == 1 ? a.buf.reward_returns : a.buf.cost_returns;
      const float* olds = role == 1 ? a.buf.reward_values : a.buf.cost_values;
      psc1 = valid ? rets[off] : 0.f;
      psc0 = valid ? olds[off] : 0.f;
    }
  };
  auto commit_rows = [&]() {
#pragma unroll
    for (int i = 0; i < XR; ++i) { const int k = gpart + 8 * i; if (k < SX) sm[S::X + gb_row * SX + k] = px[i]; }
    if (role == 0) {
#pragma unroll
      for (int i = 0; i < 2; ++i) sm[S::ACT + gb_row * SH + gpart + 8 * i] = pact[i];
      if (gpart == 0) { sm[S::OLP + gb_row * SH] = psc0; sm[S::ADR + gb_row * SH] = psc1; sm[S::ADC + gb_row * SH] = psc2; }
    } else if (gpart == 0) {
      sm[S::OLP + gb_row * SH] = psc0; sm[S::ADR + gb_row * SH] = psc1;
    }
  };
  // advantage statistics of a minibatch (policy role): thread tid < nb holds row tid's (A_r, A_c)
  float sar = 0.f, sac = 0.f;
  auto mb_rows_at = [&](int p) { const int left = n_total - p; return left < B ? left : B; };
  auto stat_idx = [&](int e, int p) -> int {   // minibatch starting at position p of epoch e
    if (role != 0 || e >= n_epochs || tid >= mb_rows_at(p)) return -1;
    return a.perms[(size_t)e * n_total + p + tid];
  };
  auto issue_stats = [&](int idx) {
    sar = 0.f; sac = 0.f;
    if (idx >= 0) {
      const unsigned off = to_off(idx);
      sar = a.buf.reward_advantages[off];
      sac = a.buf.cost_advantages[off];
    }
  };
  float mean_r = 0.f, std_r = 1.f, mean_c = 0.f;
  auto compute_stats = [&](int nb) {  // all threads of a policy workgroup; uses sar / sac.  ONE block reduction.
    if (role != 0) return;
    const bool in = tid < nb;
    float s_r = wave_sum_fast(in ? sar : 0.f), s_c = wave_sum_fast(in ? sac : 0.f), s_rr = wave_sum_fast(in ? sar * sar : 0.f);
    lds_barrier();
    if (lane == 0) { sm[S::MISC + 16 + w] = s_r; sm[S::MISC + 24 + w] = s_c; sm[S::MISC + 32 + w] = s_rr; }
    lds_barrier();
    // minibatches have <= 128 rows: only waves 0 and 1 carry data
    s_r = sm[S::MISC + 16] + sm[S::MISC + 17];
    s_c = sm[S::MISC + 24] + sm[S::MISC + 25];
    s_rr = sm[S::MISC + 32] + sm[S::MISC + 33];
    mean_r = s_r / (float)nb;
    mean_c = s_c / (float)nb;
    // unbiased variance from the raw moments (advantages are O(1): fp32 cancellation stays ~1e-6 relative)
    const float var = fmaxf(s_rr - s_r * mean_r, 0.f) / (float)(nb - 1);
    std_r = sqrtf(var);
  };
  auto refresh_gauss = [&]() {   // diagonal head: threads 144..159 own log_std: derived constants of the Gaussian head
    if (HEAD == HEAD_GAUSS && role == 0 && tid >= 144 && tid < 160) {
      const int k = tid - 144;
      const float sd = __expf(sm[S::LS + k]);
      const float iv = __builtin_amdgcn_rcpf(sd * sd);
      sm[S::GAU + k] = k < A ? iv : 0.f;
      sm[S::GAU + 16 + k] = k < A ? 0.5f * iv : 0.f;
      sm[S::GAU + 32 + k] = k < A ? __logf(sd) + LOG_SQRT_2PI_F : 0.f;
    }
  };
  // running statistics (thread 0 of each role)
  float st_ent = 0.f, st_pg = 0.f, st_vl = 0.f, st_cf = 0.f, last_loss = 0.f;
  int steps_done = 0, early_stop_epoch = n_epochs, status = 0;
  if (tid == 0) { sm[S::MISC + 12] = 0.f; sm[S::MISC + 13] = 0.f; }

  // ---- pipeline prologue: chunk 0 rows -> LDS, chunk 1 / 2 indices in flight; minibatch 0 statistics
  Cursor c_nx2 = cur_advance(Cursor{0, 0, 0});
  int idx_next = load_idx(c_nx2);
  c_nx2 = cur_advance(c_nx2);
  int idx_nx2 = load_idx(c_nx2);
  issue_rows(load_idx(Cursor{0, 0, 0}));
  issue_stats(stat_idx(0, 0));
  refresh_gauss();
  // (epoch, position) of the minibatch whose statistics indices are in flight: the one after the current
  int s_e = 0, s_p = mb_rows_at(0);
  if (s_p >= n_total) { s_p = 0; s_e = 1; }
  int sidx_next = stat_idx(s_e, s_p);
  __syncthreads();
  commit_rows();
  compute_stats(mb_rows_at(0));
  __syncthreads();

  const bool prof = (a.hp._pad & 1) != 0;
  unsigned long long ph[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long t_last = prof ? stamp() : 0ull;

  unsigned step = 0;
  bool stop = false;
  for (int epoch = 0; epoch < n_epochs && !stop; ++epoch) {
    float kl_sum = 0.f;  // thread 0, policy role
    for (int mb = 0; mb < n_mb && !stop; ++mb) {
      ++step;
      const int nb = mb_rows_at(mb * B);
      const float c_mean_r = mean_r, c_mean_c = mean_c;   // statistics of THIS minibatch
      const float c_istd_r = 1.f / (std_r + 1e-8f);
      const float cpol_nb = 1.f / ((1.f + nu) * (float)nb);
      // statistics prefetch: advantages of the NEXT minibatch's rows (indices loaded a step ago), indices of the one after
      issue_stats(sidx_next);
      {
        s_p += mb_rows_at(s_p);
        if (s_p >= n_total) { s_p = 0; ++s_e; }
        sidx_next = stat_idx(s_e, s_p);
      }
      // ---- zero gradient accumulators
#pragma unroll
      for (int c = 0; c < NT1H; ++c) gW1r[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < 2; ++c) gW2r[c] = f32x4{0.f, 0.f, 0.f, 0.f};
      gWhr = f32x4{0.f, 0.f, 0.f, 0.f};
      if constexpr (SDE) gLs = f32x4{0.f, 0.f, 0.f, 0.f};
      gB = 0.f;
      float mb_s0 = 0.f, mb_s1 = 0.f, mb_s2 = 0.f, mb_s3 = 0.f, mb_s4 = 0.f;  // thread 0: minibatch sums of the loss statistics

      const int n_chunks = (nb + RB - 1) / RB;
      for (int ch = 0; ch < n_chunks; ++ch) {
        const int nrows = (nb - ch * RB) < RB ? (nb - ch * RB) : RB;
        if (ch > 0) {  // chunk 0 of a step was committed during the previous step's granule wait (or the prologue)
          commit_rows();
          lds_barrier();
        }
        // ================= forward: wave (rt, hf): rows 16rt.., output columns 32hf..32hf+31 =================
        f32x4 h1t[2], h2t[2];   // this wave's h1 / h2 tiles stay in registers for the backward epilogues
        {
          f32x4 av[NT1], bv[2][NT1];
          const float* pa = sm + S::X + (16 * rt + r) * SX + 4 * q;
          const float* pb = sm + S::W1 + (32 * hf + r) * SX + 4 * q;
#pragma unroll
          for (int js = 0; js < NT1; ++js) {
            av[js] = lds128(pa + 16 * js);
#pragma unroll
            for (int c = 0; c < 2; ++c) bv[c][js] = lds128(pb + c * 16 * SX + 16 * js);
          }
          __builtin_amdgcn_sched_barrier(0);   // all operand reads are issued before the first MFMA
          f32x4 acc[2];
#pragma unroll
          for (int c = 0; c < 2; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int js = 0; js < NT1; ++js)
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
              for (int c = 0; c < 2; ++c) acc[c] = MFMA_F32(av[js][e], bv[c][js][e], acc[c]);
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            const int col = 32 * hf + 16 * c + r;
            const float bias = sm[S::B1 + col];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              h1t[c][i] = fast_tanh(acc[c][i] + bias);
              sm[S::H1 + (16 * rt + 4 * q + i) * SH + col] = h1t[c][i];
            }
          }
        }
        // prefetch (under the first GEMM's shadow): rows of the next chunk of the stream, indices of the one after the next
        issue_rows(idx_next);
        idx_next = idx_nx2;
        c_nx2 = cur_advance(c_nx2);
        idx_nx2 = load_idx(c_nx2);
        lds_barrier();  // (A1) both column halves of h1 written
        {
          f32x4 av[4], bv[2][4];
          const float* pa = sm + S::H1 + (16 * rt + r) * SH + 4 * q;
          const float* pb = sm + S::W2 + (32 * hf + r) * SH + 4 * q;
#pragma unroll
          for (int js = 0; js < 4; ++js) {
            av[js] = lds128(pa + 16 * js);
#pragma unroll
            for (int c = 0; c < 2; ++c) bv[c][js] = lds128(pb + c * 16 * SH + 16 * js);
          }
          __builtin_amdgcn_sched_barrier(0);
          f32x4 acc[2];
#pragma unroll
          for (int c = 0; c < 2; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int js = 0; js < 4; ++js)
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
              for (int c = 0; c < 2; ++c) acc[c] = MFMA_F32(av[js][e], bv[c][js][e], acc[c]);
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            const int col = 32 * hf + 16 * c + r;
            const float bias = sm[S::B2 + col];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              h2t[c][i] = fast_tanh(acc[c][i] + bias);
              sm[S::H2 + (16 * rt + 4 * q + i) * SH + col] = h2t[c][i];
            }
          }
        }
        lds_barrier();  // (A2) h2 complete
        if (hf == 0 || (SDE && role == 0)) {
          // hf == 0: the head, [16 rows] x [16 outputs], K = 64.  gSDE, hf == 1 (policy): the variances, the same GEMM on h2^2 and exp(2 log_std)
          const bool mean = !SDE || hf == 0;
          f32x4 av[4], bv[4];
          const float* pa = sm + S::H2 + (16 * rt + r) * SH + 4 * q;
          const float* pb = sm + (mean ? S::WH : S::E2T) + r * SH + 4 * q;
#pragma unroll
          for (int js = 0; js < 4; ++js) { av[js] = lds128(pa + 16 * js); bv[js] = lds128(pb + 16 * js); }
          if (SDE && hf == 1) {
#pragma unroll
            for (int js = 0; js < 4; ++js)
#pragma unroll
              for (int e = 0; e < 4; ++e) av[js][e] = av[js][e] * av[js][e];
          }
          __builtin_amdgcn_sched_barrier(0);
          f32x4 acc[4];   // four independent chains (one per js), summed afterwards
#pragma unroll
          for (int js = 0; js < 4; ++js) {
            acc[js] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[js] = MFMA_F32(av[js][e], bv[js][e], acc[js]);
          }
          const float bias = mean ? sm[S::BH + r] : 1e-6f;
          if constexpr (SDE) {   // the variances go to their columns of the dz rows
            float* dst = sm + (mean ? S::DO : S::VR);
            const int dstride = mean ? SO : SH;
#pragma unroll
            for (int i = 0; i < 4; ++i)
              dst[(16 * rt + 4 * q + i) * dstride + r] = ((acc[0][i] + acc[1][i]) + (acc[2][i] + acc[3][i])) + bias;
          } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
              sm[S::DO + (16 * rt + 4 * q + i) * SO + r] = ((acc[0][i] + acc[1][i]) + (acc[2][i] + acc[3][i])) + bias;
          }
        }
        lds_barrier();  // (A3) head outputs (gSDE: and variances) visible to both waves of a row tile
        STAMP(0)   // forward
        // ============ loss + d loss / d head output: row 16rt + r; lane group q and half hf split the actions ============
        {
          const int b = 16 * rt + r;
          const bool valid = b < nrows;
          float* dor = sm + S::DO + b * SO;     // holds the head output of row b; overwritten with its gradient
          if (role == 0) {
            float* vrr = sm + S::VR + b * SH;    // gSDE: the variances of row b; overwritten with d loss / d variance
            float lg[4], pr[4];                  // Categorical: log-softmax and probabilities of the classes k = q + 4 i
            float dd[4], iv[4];                  // Normal heads: x - mean and 1 / var of the actions k = q + 4 i
            int act = 0;                         // Categorical: the class taken
            float lp = 0.f, ent = 0.f;           // log-prob of the row; its entropy (the diagonal head's does not depend on the row)
            if constexpr (HEAD == HEAD_CAT) {
              // Categorical(logits) (ref: distributions.py:274-288): lane group q holds the logits k = q + 4 i of row b
              float zmax = -INFINITY;
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                const int k = q + 4 * i;
                lg[i] = k < A ? dor[k] : -INFINITY;
                zmax = fmaxf(zmax, lg[i]);
              }
              zmax = xor16_max(xor32_max(zmax));
              float se = 0.f;
#pragma unroll
              for (int i = 0; i < 4; ++i) se += (q + 4 * i < A) ? expf(lg[i] - zmax) : 0.f;
              se = quad_rows_sum(se);
              const float lse = zmax + logf(se);
              act = (int)sm[S::ACT + b * SH];
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                const int k = q + 4 * i;
                lg[i] = k < A ? lg[i] - lse : 0.f;         // log-softmax
                pr[i] = k < A ? expf(lg[i]) : 0.f;
                lp += (k == act) ? lg[i] : 0.f;
                ent -= pr[i] * lg[i];
              }
            } else {
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                const int k = q + 4 * i;                      // every wave of the pair evaluates the whole row
                const bool ka = k < A;
                float var = 1.f;                              // gSDE: the row's variance of action k
                if constexpr (SDE) var = ka ? vrr[k] : 1.f;
                dd[i] = sm[S::ACT + b * SH + k] - dor[k];     // pad actions / outputs are 0
                if constexpr (HEAD == HEAD_GAUSS) {           // the variances are the step's (refresh_gauss)
                  iv[i] = sm[S::GAU + k];
                  lp += -(dd[i] * dd[i]) * sm[S::GAU + 16 + k] - sm[S::GAU + 32 + k];
                } else {
                  iv[i] = 1.f / var;
                  const float hlv = 0.5f * logf(var);
                  lp += ka ? -(dd[i] * dd[i]) * (0.5f * iv[i]) - hlv - LOG_SQRT_2PI_F : 0.f;
                  ent += ka ? HALF_LOG_2PI_PLUS_HALF_F + hlv : 0.f;
                }
              }
            }
            lp = quad_rows_sum(lp);
            if constexpr (HEAD != HEAD_GAUSS) ent = quad_rows_sum(ent);
            const float old_lp = sm[S::OLP + b * SH];
            const float ratio = __expf(lp - old_lp);
            const float Ar = (sm[S::ADR + b * SH] - c_mean_r) * c_istd_r;
            const float Ac = sm[S::ADC + b * SH] - c_mean_c;
            const float s1 = Ar * ratio;
            const float rc = fminf(fmaxf(ratio, 1.f - clip), 1.f + clip);
            const float s2 = Ar * rc;
            const float gsel = (s1 <= s2) ? Ar : 0.f;                       // d min(s1, s2) / d ratio
            const float dlp = valid ? cpol_nb * (-gsel + nu * Ac) * ratio : 0.f;  // d loss / d log_prob
            // loss += ent_coef * (-mean H).  Categorical: d/dz_k = ent_coef / nb * p_k (log p_k + H); gSDE: d loss / d entropy of the row
            float dent = 0.f;
            if constexpr (HEAD == HEAD_CAT) dent = valid ? a.hp.ent_coef / (float)nb : 0.f;
            if constexpr (HEAD == HEAD_SDE) dent = valid ? -a.hp.ent_coef / (float)nb : 0.f;
            lds_barrier();   // (L) both waves of the pair have read the head outputs (and variances) before they are overwritten
#pragma unroll
            for (int ii = 0; ii < 2; ++ii) {
              const int i = 2 * hf + ii;                    // this wave writes / reduces the actions k = q + 4i of its half
              const int k = q + 4 * i;
              float dk, d2 = 0.f;      // d loss / d head output k; beside it d loss / d log_std_k (diagonal head) or d loss / d var_k (gSDE)
              if constexpr (HEAD == HEAD_CAT) {
                const float pk = hf == 0 ? pr[ii] : pr[2 + ii];
                const float lk = hf == 0 ? lg[ii] : lg[2 + ii];
                dk = k < A ? dlp * ((k == act ? 1.f : 0.f) - pk) + dent * (pk * (lk + ent)) : 0.f;
              } else {
                const float ddi = hf == 0 ? dd[ii] : dd[2 + ii];
                const float ivi = hf == 0 ? iv[ii] : iv[2 + ii];
                dk = dlp * (ddi * ivi);
                if constexpr (HEAD == HEAD_GAUSS) d2 = (k < A) ? dlp * ((ddi * ddi) * ivi - 1.f) : 0.f;
                else d2 = (k < A) ? dlp * (((ddi * ddi) * ivi - 1.f) * (0.5f * ivi)) + dent * (0.5f * ivi) : 0.f;
              }
              dor[k] = dk;
              if constexpr (SDE) vrr[k] = d2;
              const float colsum = sum16(dk);
              float lssum = 0.f;
              if constexpr (HEAD == HEAD_GAUSS) lssum = sum16(d2);
              if (r == 0) {
                sm[S::PBH + rt * 16 + k] = colsum;
                if constexpr (!SDE) sm[S::PLS + rt * 16 + k] = lssum;
              }
            }
            if (hf == 0) {
              const float v0 = sum16(valid ? fminf(s1, s2) : 0.f);
              const float v1 = sum16(valid ? Ac * ratio : 0.f);
              const float v2 = sum16(valid ? (fabsf(ratio - 1.f) > clip ? 1.f : 0.f) : 0.f);
              const float v3 = sum16(valid ? old_lp - lp : 0.f);
              float v4 = 0.f;
              if constexpr (HEAD != HEAD_GAUSS) v4 = sum16(valid ? ent : 0.f);
              if (lane == 0) {
                sm[S::PST + rt * 8 + 0] = v0; sm[S::PST + rt * 8 + 1] = v1; sm[S::PST + rt * 8 + 2] = v2; sm[S::PST + rt * 8 + 3] = v3;
                if constexpr (HEAD != HEAD_GAUSS) sm[S::PST + rt * 8 + 4] = v4;
              }
            }
          } else {
            const float v = dor[0];
            const float R = sm[S::ADR + b * SH];
            float vp = v, pass = 1.f;
            if (vclip >= 0.f) {
              const float old = sm[S::OLP + b * SH];
              const float dv = v - old;
              vp = old + fminf(fmaxf(dv, -vclip), vclip);
              pass = (dv >= -vclip && dv <= vclip) ? 1.f : 0.f;
            }
            const float e = vp - R;
            const float d0 = valid ? vcoef * 2.f * e / (float)nb * pass : 0.f;
            lds_barrier();   // (L)
            if (hf == 0) {
              if (q == 0) {
                dor[0] = d0;
#pragma unroll
                for (int k = 1; k < 16; ++k) dor[k] = 0.f;
              }
              const float colsum = sum16(d0);
              const float se = sum16(valid ? e * e : 0.f);
              if (lane == 0) {
                sm[S::PBH + rt * 16] = colsum;
#pragma unroll
                for (int k = 1; k < 16; ++k) sm[S::PBH + rt * 16 + k] = 0.f;
                sm[S::PST + rt * 8 + 0] = se;
              }
            }
          }
        }
        lds_barrier();  // (A4) d loss / d output (gSDE: and d loss / d variance) of the row tile complete (written by both halves)
        STAMP(1)   // loss
        // ================= backward =================
        if constexpr (SDE) {
          // gSDE: the two head-gradient GEMMs first.  They read dOut, d variance (in the dz rows) and h2, all complete behind (A4)
          if (hf == 0 || role == 0) {
            // hf == 0: dWh[o][j] += sum_b dOut[b][o] h2[b][j]   (columns 16rt..16rt+15); b = 16 js + 4 q + e
            // hf == 1 (policy): S[a][h] += sum_b dVar[b][a] h2[b][h]^2, the same GEMM on the variance gradients and the squared latent
            float av[4][4], bv[4][4];
            const int astride = hf == 0 ? SO : SH;
            const float* pa = sm + (hf == 0 ? S::DO : S::VR) + (4 * q) * astride + r;
            const float* pb = sm + S::H2 + (4 * q) * SH + 16 * rt + r;
#pragma unroll
            for (int js = 0; js < 4; ++js)
#pragma unroll
              for (int e = 0; e < 4; ++e) { av[js][e] = pa[(16 * js + e) * astride]; bv[js][e] = pb[(16 * js + e) * SH]; }
            if (hf == 1) {
#pragma unroll
              for (int js = 0; js < 4; ++js)
#pragma unroll
                for (int e = 0; e < 4; ++e) bv[js][e] = bv[js][e] * bv[js][e];
            }
            __builtin_amdgcn_sched_barrier(0);
            f32x4 acc[4];
#pragma unroll
            for (int js = 0; js < 4; ++js) {
              acc[js] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
              for (int e = 0; e < 4; ++e) acc[js] = MFMA_F32(av[js][e], bv[js][e], acc[js]);
            }
            if (hf == 0) {
#pragma unroll
              for (int i = 0; i < 4; ++i) gWhr[i] += (acc[0][i] + acc[1][i]) + (acc[2][i] + acc[3][i]);
            } else {
#pragma unroll
              for (int i = 0; i < 4; ++i) gLs[i] += (acc[0][i] + acc[1][i]) + (acc[2][i] + acc[3][i]);
            }
          }
          lds_barrier();  // (A5) the log_std GEMM has read d variance out of the dz rows: dz2 may be written over them
        }
        {  // dH2 = dOut . Wh  -> dz2 = dH2 * (1 - h2^2) (own rows, own column half), column sums for d b2.  gSDE: the mean path only, the
           // latent is detached in the variance
          const f32x4 av = lds128(sm + S::DO + (16 * rt + r) * SO + 4 * q);   // k = a = 4q + e
          float bv[2][4];
          const float* pb = sm + S::WH + (4 * q) * SH + 32 * hf + r;
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int c = 0; c < 2; ++c) bv[c][e] = pb[e * SH + 16 * c];
          f32x4 acc[2];
#pragma unroll
          for (int c = 0; c < 2; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int c = 0; c < 2; ++c) acc[c] = MFMA_F32(av[e], bv[c][e], acc[c]);
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            const int col = 32 * hf + 16 * c + r;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              acc[c][i] = acc[c][i] * (1.f - h2t[c][i] * h2t[c][i]);
              sm[S::DZ + (16 * rt + 4 * q + i) * SH + col] = acc[c][i];
            }
            const float cs = tile_colsum(acc[c]);
            if (q == 0) sm[S::RED2 + rt * HD + col] = cs;
          }
        }
        lds_barrier();  // (2) dz2 and its column sums of ALL rows visible (not gSDE: dOut, h2)
        if constexpr (!SDE) {
          if (hf == 0) {  // dWh[o][j] += sum_b dOut[b][o] h2[b][j]   (columns 16rt..16rt+15); b = 16 js + 4 q + e
            float av[4][4], bv[4][4];
            const float* pa = sm + S::DO + (4 * q) * SO + r;
            const float* pb = sm + S::H2 + (4 * q) * SH + 16 * rt + r;
#pragma unroll
            for (int js = 0; js < 4; ++js)
#pragma unroll
              for (int e = 0; e < 4; ++e) { av[js][e] = pa[(16 * js + e) * SO]; bv[js][e] = pb[(16 * js + e) * SH]; }
            __builtin_amdgcn_sched_barrier(0);
            f32x4 acc[4];
#pragma unroll
            for (int js = 0; js < 4; ++js) {
              acc[js] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
              for (int e = 0; e < 4; ++e) acc[js] = MFMA_F32(av[js][e], bv[js][e], acc[js]);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) gWhr[i] += (acc[0][i] + acc[1][i]) + (acc[2][i] + acc[3][i]);
          }
        }
        // owners fold the per-row-tile partials of this chunk (b2, head bias, not gSDE: log_std, loss statistics)
        if (tid >= 64 && tid < 128) {
          const int j = tid - 64;
          gB += (sm[S::RED2 + j] + sm[S::RED2 + HD + j]) + (sm[S::RED2 + 2 * HD + j] + sm[S::RED2 + 3 * HD + j]);
        } else if (tid >= 128 && tid < 144) {
          const int k = tid - 128;
          gB += (sm[S::PBH + k] + sm[S::PBH + 16 + k]) + (sm[S::PBH + 32 + k] + sm[S::PBH + 48 + k]);
        } else if (!SDE && tid >= 144 && tid < 160) {
          const int k = tid - 144;
          gB += (sm[S::PLS + k] + sm[S::PLS + 16 + k]) + (sm[S::PLS + 32 + k] + sm[S::PLS + 48 + k]);
        }
        if (tid == 0) {
          mb_s0 += (sm[S::PST + 0] + sm[S::PST + 8]) + (sm[S::PST + 16] + sm[S::PST + 24]);
          mb_s1 += (sm[S::PST + 1] + sm[S::PST + 9]) + (sm[S::PST + 17] + sm[S::PST + 25]);
          mb_s2 += (sm[S::PST + 2] + sm[S::PST + 10]) + (sm[S::PST + 18] + sm[S::PST + 26]);
          mb_s3 += (sm[S::PST + 3] + sm[S::PST + 11]) + (sm[S::PST + 19] + sm[S::PST + 27]);
          if (HEAD != HEAD_GAUSS) mb_s4 += (sm[S::PST + 4] + sm[S::PST + 12]) + (sm[S::PST + 20] + sm[S::PST + 28]);
        }
        lds_barrier();  // (2b) every wave is done reading h2: its buffer becomes dz1
        {  // dH1 = dz2 . W2 (own rows, own column half) -> dz1 = dH1 * (1 - h1^2), stored over h2
          f32x4 av[4];
          const float* pa = sm + S::DZ + (16 * rt + r) * SH + 4 * q;
          const float* pb = sm + S::W2 + (4 * q) * SH + 32 * hf + r;
#pragma unroll
          for (int js = 0; js < 4; ++js) av[js] = lds128(pa + 16 * js);
          float bv[4][2][4];
#pragma unroll
          for (int js = 0; js < 4; ++js)
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
              for (int c = 0; c < 2; ++c) bv[js][c][e] = pb[(16 * js + e) * SH + 16 * c];
          __builtin_amdgcn_sched_barrier(0);
          f32x4 acc[2];
#pragma unroll
          for (int c = 0; c < 2; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int js = 0; js < 4; ++js)
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
              for (int c = 0; c < 2; ++c) acc[c] = MFMA_F32(av[js][e], bv[js][c][e], acc[c]);
          // dW2[j][k] += sum_b dz2[b][j] h1[b][k]  (rows j = 16rt.., columns 32hf..): its MFMAs are independent of the
          // epilogue below, so the scheduler can hide the epilogue's VALU / LDS work under them
          float a2[4][4], b2v[4][2][4];
          const float* pa2 = sm + S::DZ + (4 * q) * SH + 16 * rt + r;
          const float* pb2 = sm + S::H1 + (4 * q) * SH + 32 * hf + r;
#pragma unroll
          for (int js = 0; js < 4; ++js)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              a2[js][e] = pa2[(16 * js + e) * SH];
#pragma unroll
              for (int c = 0; c < 2; ++c) b2v[js][c][e] = pb2[(16 * js + e) * SH + 16 * c];
            }
#pragma unroll
          for (int js = 0; js < 4; ++js)
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
              for (int c = 0; c < 2; ++c) gW2r[c] = MFMA_F32(a2[js][e], b2v[js][c][e], gW2r[c]);
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            const int col = 32 * hf + 16 * c + r;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              acc[c][i] = acc[c][i] * (1.f - h1t[c][i] * h1t[c][i]);
              sm[S::H2 + (16 * rt + 4 * q + i) * SH + col] = acc[c][i];
            }
            const float cs = tile_colsum(acc[c]);
            if (q == 0) sm[S::RED1 + rt * HD + col] = cs;
          }
        }
        lds_barrier();  // (3) dz1 of all rows visible
        {  // dW1[j][k] += sum_b dz1[b][j] x[b][k]   (rows j = 16rt.., column tiles hf*NT1H..)
          float av[4][4];
          const float* pa = sm + S::H2 + (4 * q) * SH + 16 * rt + r;
          const float* pb = sm + S::X + (4 * q) * SX + 16 * hf * NT1H + r;
#pragma unroll
          for (int js = 0; js < 4; ++js)
#pragma unroll
            for (int e = 0; e < 4; ++e) av[js][e] = pa[(16 * js + e) * SH];
#pragma unroll
          for (int js = 0; js < 4; ++js) {
            float bv[NT1H][4];
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
              for (int c = 0; c < NT1H; ++c) bv[c][e] = pb[(16 * js + e) * SX + 16 * c];
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
              for (int c = 0; c < NT1H; ++c) gW1r[c] = MFMA_F32(av[js][e], bv[c][e], gW1r[c]);
          }
        }
        if (tid < 64) gB += (sm[S::RED1 + tid] + sm[S::RED1 + HD + tid]) + (sm[S::RED1 + 2 * HD + tid] + sm[S::RED1 + 3 * HD + tid]);
        lds_barrier();  // (4) chunk buffers free
        STAMP(2)   // backward
      }  // chunks

      // entropy term of the policy loss: d(ent_coef * -mean(H)) / d log_std = -ent_coef (H = sum_a 0.5 + 0.5 log 2pi + log sigma)
      if (HEAD == HEAD_GAUSS && role == 0 && tid >= 144 && tid < 144 + A) gB += -a.hp.ent_coef;
      // gSDE: d var / d log_std[h][a] = 2 latent_h^2 exp(2 log_std[h][a]): the factor of the owner's own entry of the image, once per step
      if (ls_owner) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int o = 4 * q + i;
          gLs[i] = o < A ? (2.f * sm[S::E2T + o * SH + 16 * rt + r]) * gLs[i] : 0.f;
        }
      }

      // ================= global gradient norm: local sum of squares -> 8-byte granules =================
      float ss = 0.f;
#pragma unroll
      for (int c = 0; c < NT1H; ++c)
#pragma unroll
        for (int i = 0; i < 4; ++i) ss += gW1r[c][i] * gW1r[c][i];
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int i = 0; i < 4; ++i) ss += gW2r[c][i] * gW2r[c][i];
#pragma unroll
      for (int i = 0; i < 4; ++i) ss += gWhr[i] * gWhr[i];
      if (ls_owner) {
#pragma unroll
        for (int i = 0; i < 4; ++i) ss += gLs[i] * gLs[i];
      }
      if (vec_g >= 0) ss += gB * gB;
      ss = wave_sum_fast(ss);
      if (lane == 0) sm[S::MISC + w] = ss;
      lds_barrier();
      // the early-stop decision rides on the policy workgroup's granule; publish first, book-keep afterwards
      if (tid == 0) {
        ss = ((sm[S::MISC + 0] + sm[S::MISC + 1]) + (sm[S::MISC + 2] + sm[S::MISC + 3])) +
             ((sm[S::MISC + 4] + sm[S::MISC + 5]) + (sm[S::MISC + 6] + sm[S::MISC + 7]));
        bool want_stop = false;
        float mean_kl = 0.f;
        if (role == 0) {
          kl_sum += mb_s3 / (float)nb;
          if (mb == n_mb - 1) {
            mean_kl = kl_sum / (float)n_mb;
            if (a.hp.use_target_kl && mean_kl > 1.5f * a.hp.target_kl) { want_stop = true; early_stop_epoch = epoch; }
          }
        }
        const unsigned tag = step | (want_stop ? 0x80000000u : 0u);
        __hip_atomic_store(a.xch + (step & 1) * 4 + role, ((u64)tag << 32) | (u64)__float_as_uint(ss), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        ++steps_done;
        if (role == 0) {
          float ent = 0.f;
          if (HEAD != HEAD_GAUSS) ent = mb_s4 / (float)nb;
          else for (int k = 0; k < A; ++k) ent += HALF_LOG_2PI_PLUS_HALF_F + sm[S::LS + k];
          const float entropy_loss = -ent;
          const float pl = (-(mb_s0 / (float)nb) + nu * (mb_s1 / (float)nb)) / (1.f + nu);
          st_ent += entropy_loss; st_pg += pl; st_cf += mb_s2 / (float)nb;
          last_loss = pl + a.hp.ent_coef * entropy_loss;
          if (mb == n_mb - 1) { a.stats[32 + epoch] = mean_kl; a.stats[7] = mean_kl; }
        } else {
          const float vl = mb_s0 / (float)nb;
          st_vl += vl;
          last_loss = vl;
        }
      }
      STAMP(3)   // gradient norm + publish
      // ---- while the granules travel: stage the next minibatch (rows -> LDS, advantage statistics)
      commit_rows();
      {
        const int pn = (mb + 1 < n_mb) ? (mb + 1) * B : 0;
        compute_stats(mb_rows_at(pn));
      }
      STAMP(4)   // next-minibatch staging
      if (tid < 3) {   // bounded wait: a workgroup that does not show up ends the launch through the status word
        u64 v = 0;
        int spins = 0;
        bool ok = false;
        while (spins < (1 << 24)) {
          v = __hip_atomic_load(a.xch + (step & 1) * 4 + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if ((unsigned)((v >> 32) & 0x7fffffffu) == step) { ok = true; break; }
          __builtin_amdgcn_s_sleep(1);
          ++spins;
        }
        sm[S::MISC + 8 + tid] = __uint_as_float((unsigned)(v & 0xffffffffu));
        if (tid == 0) sm[S::MISC + 12] = (v >> 63) ? 1.f : 0.f;
        if (!ok) sm[S::MISC + 13] = 1.f;
      } else if (tid == 3) {   // Adam's bias corrections in double, once per step, while the others poll
        b1pow *= (double)a.hp.adam_beta1;
        b2pow *= (double)a.hp.adam_beta2;
        sm[S::MISC + 14] = (float)((double)a.hp.lr / (1.0 - b1pow));
        sm[S::MISC + 15] = (float)(1.0 / sqrt(1.0 - b2pow));
      }
      lds_barrier();
      STAMP(5)   // granule wait
      const float total = sqrtf((sm[S::MISC + 8] + sm[S::MISC + 9]) + sm[S::MISC + 10]);
      stop = sm[S::MISC + 12] != 0.f;
      if (sm[S::MISC + 13] != 0.f) { status = 1; stop = true; }
      float coef = a.hp.max_grad_norm / (total + 1e-6f);
      coef = coef > 1.f ? 1.f : coef;

      // ================= Adam (torch.optim.Adam, single-tensor form) on register-resident moments =================
      const float step_size = sm[S::MISC + 14];
      const float inv_bc2_sqrt = sm[S::MISC + 15];
      const float b2f = a.hp.adam_beta2, epsf = a.hp.adam_eps;
      auto adam = [&](float g, float& m, float& v, float p) -> float {
        g = g * coef;
        m = m + (g - m) * w1;
        v = v * b2f + w2 * (g * g);
        const float denom = __builtin_amdgcn_sqrtf(v) * inv_bc2_sqrt + epsf;     // v_sqrt_f32 / v_rcp_f32: 1 ulp each
        return p - step_size * (m * __builtin_amdgcn_rcpf(denom));
      };
      if (status == 0) {
#pragma unroll
        for (int c = 0; c < NT1H; ++c)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int j = 16 * rt + 4 * q + i, k = 16 * (hf * NT1H + c) + r;
            if (k < O) { float* pw = sm + S::W1 + j * SX + k; float m_ = mW1[c][i], v_ = vW1[c][i]; *pw = adam(gW1r[c][i], m_, v_, *pw); mW1[c][i] = m_; vW1[c][i] = v_; }
          }
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            float* pw = sm + S::W2 + (16 * rt + 4 * q + i) * SH + 16 * (2 * hf + c) + r;
            float m_ = mW2[c][i], v_ = vW2[c][i];
            *pw = adam(gW2r[c][i], m_, v_, *pw);
            mW2[c][i] = m_; vW2[c][i] = v_;
          }
        if (hf == 0) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int o = 4 * q + i;
            if (o < n_out) { float* pw = sm + S::WH + o * SH + 16 * rt + r; float m_ = mWh[i], v_ = vWh[i]; *pw = adam(gWhr[i], m_, v_, *pw); mWh[i] = m_; vWh[i] = v_; }
          }
        } else if (SDE && role == 0) {   // gSDE: log_std and its entry of the exp(2 log_std) image
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int o = 4 * q + i;
            if (o < A) {
              float m_ = mLs[i], v_ = vLs[i];
              const float p_ = adam(gLs[i], m_, v_, pLs[i]);
              pLs[i] = p_; mLs[i] = m_; vLs[i] = v_;
              sm[S::E2T + o * SH + 16 * rt + r] = expf(2.f * p_);
            }
          }
        }
        if (vec_g >= 0) sm[vec_s] = adam(gB, mB, vB, sm[vec_s]);
        refresh_gauss();
      }
      if (tid == 0) { sm[S::MISC + 12] = 0.f; sm[S::MISC + 13] = 0.f; }
      lds_barrier();
      STAMP(6)   // Adam
    }  // minibatches
  }    // epochs

  __syncthreads();
  // ---- write back weights, moments, statistics
  for (int i = tid; i < HD * O; i += TH) { const int j = i / O, k = i % O; a.params[gW1 + i] = sm[S::W1 + j * SX + k]; }
  for (int i = tid; i < HD * HD; i += TH) { const int j = i / HD, k = i % HD; a.params[gW2 + i] = sm[S::W2 + j * SH + k]; }
  for (int i = tid; i < n_out * HD; i += TH) { const int o = i / HD, k = i % HD; a.params[gWh + i] = sm[S::WH + o * SH + k]; }
  if (vec_g >= 0) { a.params[vec_g] = sm[vec_s]; a.exp_avg[vec_g] = mB; a.exp_avg_sq[vec_g] = vB; }
#pragma unroll
  for (int c = 0; c < NT1H; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = 16 * rt + 4 * q + i, k = 16 * (hf * NT1H + c) + r;
      if (k < O) { a.exp_avg[gW1 + j * O + k] = mW1[c][i]; a.exp_avg_sq[gW1 + j * O + k] = vW1[c][i]; }
    }
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = 16 * rt + 4 * q + i, k = 16 * (2 * hf + c) + r;
      a.exp_avg[gW2 + j * HD + k] = mW2[c][i];
      a.exp_avg_sq[gW2 + j * HD + k] = vW2[c][i];
    }
  if (hf == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int o = 4 * q + i, j = 16 * rt + r;
      if (o < n_out) { a.exp_avg[gWh + o * HD + j] = mWh[i]; a.exp_avg_sq[gWh + o * HD + j] = vWh[i]; }
    }
  } else if (SDE && role == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int o = 4 * q + i, j = 16 * rt + r;
      if (o < A) { a.params[L.log_std + j * A + o] = pLs[i]; a.exp_avg[L.log_std + j * A + o] = mLs[i]; a.exp_avg_sq[L.log_std + j * A + o] = vLs[i]; }
    }
  }
  if (tid == 0 && prof) {
    for (int k = 0; k < 7; ++k) {
      const int slot = 12 + 7 * role + k;
      if (slot < 32) a.stats[slot] = (float)((double)ph[k] / (double)(steps_done > 0 ? steps_done : 1));
    }
  }
  if (tid == 0) {
    if (role == 0) {
      a.stats[0] = (float)early_stop_epoch;
      a.stats[1] = (float)steps_done;
      a.stats[2] = st_ent; a.stats[3] = st_pg; a.stats[6] = st_cf;
      a.stats[8] = last_loss;
      a.stats[11] = (float)status;
      a.adam_t[0] = t0 + steps_done;
    } else if (role == 1) {
      a.stats[4] = st_vl; a.stats[9] = last_loss;
    } else {
      a.stats[5] = st_vl; a.stats[10] = last_loss;
    }
  }
