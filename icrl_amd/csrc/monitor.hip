// Training-episode statistics (the reference's Monitor wrapper + ep_info_buffer) from the raw-reward plane of a rollout — gfx950.
//
//   Monitor.step                 stable_baselines3/common/monitor.py:91-122      per env: rewards.append(r); on done: sum, len -> info["episode"]
//   _update_info_buffer          stable_baselines3/common/base_class.py:368-389  once per env step, envs in index order: ep_info_buffer.extend
//   ep_info_buffer               base_class.py:328-332                           deque(maxlen=100)
//
// The rollout kernels (rollout.hip) leave the raw reward of every step in icrl_monitor_t.raw_rewards [T, N] float64.  icrl_monitor_scan
// turns the plane into episode records, two plain launches on the rollout's stream:
//
//   monitor_count_kernel   one wave per row t: the done flags of the row in 64-column chunks, ballot + popcount ->
//                          pre[t][c] (records of row t in columns below chunk c) and row_cnt[t].  Reads the flags only, every row independent.
//   monitor_scan_kernel    one wave per 64-column chunk, one lane per env: the sequential float64 sum of the env's rewards in step order
//                          (the only order constraint of the whole pass), restarted from +0.0 after every done.  The rank of a record in the
//                          reference's append order (step-major, env index ascending within a step) is
//                              records of earlier rows (running sum of row_cnt) + pre[t][c] + done lanes below this one (ballot),
//                          so a lane knows, without talking to another workgroup, whether its record is one of the last 100 of this call and
//                          which ring slot it takes.  The adds of a column depend on each other, its loads do not: SCAN_ROWS rows are loaded
//                          ahead of the rows being summed, every load unconditional (row indices are clamped, not branched on).
//
// Nothing waits for another workgroup; every loop is bounded by `rows` or by N / 64.
#include "common.h"

namespace icrl {
namespace {

constexpr int RING = 100;          // ep_info_buffer: deque(maxlen=100)
constexpr int SCAN_ROWS = 8;       // rows in flight per lane ahead of the running sum

// workspace, in ints: [0] the ring's record count at the start of the call | [4 ..) row_cnt[T] | pre[T][NC]
__host__ __device__ inline size_t mon_ws_ints(int T, int N) { return 4 + (size_t)T + (size_t)T * (size_t)((N + 63) / 64); }

struct MonArgs {
  icrl_monitor_t m;
  const float* dones;              // buffer.dones [T, N]: row t + 1 holds the done flags of step t
  const unsigned char* last_dones; // [N]: the done flags of step rows - 1
  int N, rows, NC;
};

__global__ void __launch_bounds__(256) monitor_count_kernel(MonArgs a) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  int* const ws = a.m.ws;
  if (blockIdx.x == 0 && threadIdx.x == 0) ws[0] = a.m.win_state[0];
  if (t >= a.rows) return;
  int* const row_cnt = ws + 4;
  int* const pre = row_cnt + a.rows;
  const bool last = t == a.rows - 1;
  const float* const drow = a.dones + (size_t)(last ? t : t + 1) * a.N;
  int run = 0;
  for (int c = 0; c < a.NC; ++c) {
    const int n = c * 64 + lane;
    bool d = false;
    if (n < a.N) d = last ? a.last_dones[n] != 0 : drow[n] != 0.f;
    if (lane == 0) pre[(size_t)t * a.NC + c] = run;
    run += __popcll(__ballot(d));
  }
  if (lane == 0) row_cnt[t] = run;
}

__global__ void __launch_bounds__(64) monitor_scan_kernel(MonArgs a) {
  const int lane = threadIdx.x, c = blockIdx.x;
  const int N = a.N, rows = a.rows, NC = a.NC;
  const int n = c * 64 + lane;
  const bool valid = n < N;
  const int nn = valid ? n : N - 1;
  const int* const ws = a.m.ws;
  const int* const row_cnt = ws + 4;
  const int* const pre = row_cnt + rows + c;
  int tot = 0;
  for (int t = lane; t < rows; t += 64) tot += row_cnt[t];
  for (int s = 32; s > 0; s >>= 1) tot += __shfl_xor(tot, s);
  const unsigned cnt0 = (unsigned)ws[0];
  const int thresh = tot - RING;                 // records of this call with a rank below it have left the ring again
  double ret = a.m.ep_ret[nn];
  int len = a.m.ep_len[nn];
  const bool last_d = a.last_dones[nn] != 0;
  const double* const raw = a.m.raw_rewards + nn;
  const float* const dn = a.dones + nn;
  const unsigned long long below = (1ull << lane) - 1ull;
  int rowbase = 0;
  double xa[SCAN_ROWS]; float da[SCAN_ROWS]; int ca[SCAN_ROWS], pa[SCAN_ROWS];
  auto load = [&](int t, double& x, float& d, int& rc, int& pr) {
    const int tt = min(t, rows - 1), td = min(t + 1, rows - 1);
    x = raw[(size_t)tt * N]; d = dn[(size_t)td * N]; rc = row_cnt[tt]; pr = pre[(size_t)tt * NC];
  };
#pragma unroll
  for (int i = 0; i < SCAN_ROWS; ++i) load(i, xa[i], da[i], ca[i], pa[i]);
  for (int t0 = 0; t0 < rows; t0 += SCAN_ROWS) {
    double xb[SCAN_ROWS]; float db[SCAN_ROWS]; int cb[SCAN_ROWS], pb[SCAN_ROWS];
#pragma unroll
    for (int i = 0; i < SCAN_ROWS; ++i) load(t0 + SCAN_ROWS + i, xb[i], db[i], cb[i], pb[i]);
#pragma unroll
    for (int i = 0; i < SCAN_ROWS; ++i) {
      const int t = t0 + i;
      if (t < rows) {                            // (uniform)
        ret = ret + xa[i];
        len += 1;
        const bool d = valid && (t == rows - 1 ? last_d : da[i] != 0.f);
        const unsigned long long b = __ballot(d);
        if (d) {
          const int rank = rowbase + pa[i] + __popcll(b & below);
          if (rank >= thresh) {
            const unsigned slot = (cnt0 + (unsigned)rank) % (unsigned)RING;
            a.m.win_ret[slot] = ret;
            a.m.win_len[slot] = len;
          }
          ret = 0.0;
          len = 0;
        }
        rowbase += ca[i];
      }
    }
#pragma unroll
    for (int i = 0; i < SCAN_ROWS; ++i) { xa[i] = xb[i]; da[i] = db[i]; ca[i] = cb[i]; pa[i] = pb[i]; }
  }
  if (valid) { a.m.ep_ret[n] = ret; a.m.ep_len[n] = len; }
  if (c == 0 && lane == 0) a.m.win_state[0] = (int)(cnt0 + (unsigned)tot);
}

}  // namespace
}  // namespace icrl

using namespace icrl;

extern "C" size_t icrl_monitor_ws_bytes(int T, int N) { return T < 1 || N < 1 ? 0 : mon_ws_ints(T, N) * sizeof(int); }

extern "C" int icrl_monitor_scan(const icrl_monitor_t* m, const float* dones_plane, const unsigned char* last_dones, int T, int N, int rows,
                                 void* stream) {
  if (m == nullptr) return fail("icrl_monitor_scan: NULL descriptor");
  if (T < 1 || N < 1 || rows < 1 || rows > T) return fail("icrl_monitor_scan: rows = %d of T = %d (1..T), N = %d", rows, T, N);
  if (m->raw_rewards == nullptr || m->ep_ret == nullptr || m->ep_len == nullptr || m->win_ret == nullptr || m->win_len == nullptr ||
      m->win_state == nullptr || dones_plane == nullptr || last_dones == nullptr)
    return fail("icrl_monitor_scan: the plane, the carries, the ring, its state, the dones plane and last_dones are all required");
  if (m->ws == nullptr || (size_t)m->ws_bytes < icrl_monitor_ws_bytes(rows, N))
    return fail("icrl_monitor_scan: workspace of %zu B needed (icrl_monitor_ws_bytes), got %lld", icrl_monitor_ws_bytes(rows, N), m->ws_bytes);
  MonArgs a{*m, dones_plane, last_dones, N, rows, (N + 63) / 64};
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(monitor_count_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, a);
  hipLaunchKernelGGL(monitor_scan_kernel, dim3(a.NC), dim3(64), 0, s, a);
  return (int)hipGetLastError();
}
