// The pre-gathered minibatch stream of the PPO-Lagrangian update (icrl_ppo_lag_train_stream) — gfx950.
//
// ref: stable_baselines3/common/buffers.py:594-627 (the minibatch gather), ppo_lag/ppo_lag.py:215-219 (advantage normalisation).
//
// The permutations of all epochs are known before the persistent update kernel starts.  Its step loop is a chain of dependent optimiser
// steps on 12 compute units; gathering every minibatch row by row inside that chain puts an index pipeline, ~2 k scattered 4-byte
// requests and the advantage statistics on each step while the rest of the device idles.  Here two plain launches over ALL epochs do
// that work with the whole device in front of the persistent launch: the rows of every minibatch, in step order, as one contiguous
// record per 16-row tile (layout: ppo_common.h, StreamRec), and {mean, 1 / (std + 1e-8), cost mean} of the advantages per step.
// The values are the ones the in-kernel gather stages and forms (same rows for ragged chunks, same partial sums in the same order),
// so the update's results are bit-identical in both forms.
#include "ppo_common.h"

namespace icrl {

constexpr int SREC_TH = 256;   // one workgroup per record: 16 rows x 16 component lanes

// record 4 g + tile of chunk g (g == n_chunks: the plan's zero entry behind the last chunk, what the loop's last prefetch reads)
__global__ void __launch_bounds__(SREC_TH) ppo_stream_gather_kernel(const PlanChunk* __restrict__ chunks, const int* __restrict__ perms, icrl_buffer_t buf, StreamRec L,
                                                                    float* __restrict__ out) {
  const int rec = (int)blockIdx.x, g = rec >> 2, tile = rec & 3;
  const int row = (int)threadIdx.x & 15, cl = (int)threadIdx.x >> 4;
  const PlanChunk c = chunks[g];
  const int pos = 16 * tile + row;                                  // position of the row in its 64-row chunk
  const unsigned off = (unsigned)perms[c.perm_base + (pos < c.rows ? pos : 0)];      // (the in-kernel gather's clamp: chunk_idx)
  float* const o = out + (size_t)rec * (size_t)L.floats() + row;
  const float* const planes[SR_PLANES] = {buf.log_probs, buf.reward_advantages, buf.cost_advantages, buf.reward_values, buf.reward_returns, buf.cost_values, buf.cost_returns};
  for (int comp = cl; comp < L.comps(); comp += 16) {
    float v;
    if (comp < L.O) v = buf.observations[off * (unsigned)L.O + (unsigned)comp];
    else if (comp < L.O + L.AS) v = buf.actions[off * (unsigned)L.AS + (unsigned)(comp - L.O)];
    else {
      const int pl = comp - L.O - L.AS;
      const float* p = planes[0];
#pragma unroll
      for (int k = 1; k < SR_PLANES; ++k) p = pl == k ? planes[k] : p;
      v = p[off];
    }
    o[16 * comp] = v;
  }
}

// one workgroup per optimiser step, wave w = rows 64 w .. of the minibatch (the in-kernel form's waves SW0 .. SW0 + 3, same lanes)
__global__ void __launch_bounds__(256) ppo_stream_stats_kernel(const PlanStep* __restrict__ steps, const int* __restrict__ perms, const float* __restrict__ adv_r,
                                                               const float* __restrict__ adv_c, int n_steps, int big_mb, float* __restrict__ out) {
  __shared__ float part[12];
  const int i = (int)blockIdx.x, stid = (int)threadIdx.x, w = stid >> 6;
  float* const o = out + 4 * (size_t)i;
  if (i >= n_steps) {      // the two entries behind the last step: read by the step table's pipeline, never used
    if (stid == 0) { o[0] = 0.f; o[1] = 1.f; o[2] = 0.f; o[3] = 0.f; }
    return;
  }
  const PlanStep p = steps[i];
  const int nb = p.nb_flags & NB_MASK;
  const unsigned off = (unsigned)perms[p.perm_base + (stid < nb ? stid : 0)];
  const float sar = adv_r[off], sac = adv_c[off];
  float s_r, s_c, s_rr;
  adv_wave_partials(stid < nb, sar, sac, s_r, s_c, s_rr);
  if ((stid & 63) == 0) { part[3 * w] = s_r; part[3 * w + 1] = s_c; part[3 * w + 2] = s_rr; }
  __syncthreads();
  if (stid == 0) {
    float mean_r, istd_r, mean_c;
    adv_stats_from_partials(part, big_mb != 0, nb, mean_r, istd_r, mean_c);
    o[0] = mean_r; o[1] = istd_r; o[2] = mean_c; o[3] = 0.f;
  }
}

// chunks of a launch in plan order (ppo_plan_kernel, one entry per chunk)
long long stream_n_chunks(int n_total, int batch_size, int n_epochs) {
  const long long n_mb = (n_total + batch_size - 1) / batch_size, cpm = (batch_size + RB - 1) / RB;
  const long long nb_last = n_total - (n_mb - 1) * batch_size;
  return (long long)n_epochs * ((n_mb - 1) * cpm + (nb_last + RB - 1) / RB);
}
size_t stream_rec_bytes(int obs, int act_store, long long n_chunks) {
  const StreamRec L{obs, act_store};
  return ((size_t)4 * (size_t)(n_chunks + 1) * (size_t)L.floats() * sizeof(float) + 255) / 256 * 256;
}
size_t stream_bytes(int obs, int act_store, long long n_chunks, long long n_steps) {
  return stream_rec_bytes(obs, act_store, n_chunks) + 16 * (size_t)(n_steps + 2);
}

// a.perms (storage offsets), a.plan_steps and a.plan_chunks are written by launches already enqueued on s (prepare_train); sets a.srec / a.sstat
int launch_stream_prepass(TrainArgs& a, void* ws, hipStream_t s) {
  const int n_total = a.buf.T * a.buf.N;
  const long long n_chunks = stream_n_chunks(n_total, a.hp.batch_size, a.hp.n_epochs);
  float* const rec = (float*)ws;
  float* const stat = (float*)((char*)ws + stream_rec_bytes(a.L.O, a.buf.act_store, n_chunks));
  const StreamRec L{a.L.O, a.buf.act_store};
  hipLaunchKernelGGL(ppo_stream_gather_kernel, dim3((unsigned)(4 * (n_chunks + 1))), dim3(SREC_TH), 0, s, a.plan_chunks, a.perms, a.buf, L, rec);
  hipLaunchKernelGGL(ppo_stream_stats_kernel, dim3((unsigned)(a.n_steps + 2)), dim3(256), 0, s, a.plan_steps, a.perms, a.buf.reward_advantages, a.buf.cost_advantages,
                     a.n_steps, (int)(a.hp.batch_size > 128), stat);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  a.srec = rec; a.sstat = stat;
  return 0;
}

}  // namespace icrl
