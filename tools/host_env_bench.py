"""Per-env-step cost of rollouts over host envs, one process, one GPU ("Host envs"):

  (a) host path      PPOLagrangian._collect_rollouts_host (one staging copy + one icrl_host_step launch per env step)
  (b) stepped path   PPOLagrangian._collect_rollouts_stepped over the same host env (policy.forward, env.step through the wrappers)
  (c) env alone      HostVecEnv.step_host over the same envs
  (d) device env     the persistent rollout over HipSynthVecEnv (HCWithPos-v0), for reference

The host env is a do-nothing HC-shaped numpy env (obs 18, act 6), so (a) - (c) is device and transfer overhead.  Each figure is
one timed rollout of T steps after a warm-up rollout.  usage: python tools/host_env_bench.py [--T 1024] [--N 8 64 128]

--episodes E adds the episode mode: us per env step of utils.sample_from_agent, E fixed-length episodes (1000 steps) of ONE env:

  (a) host path      utils.HostEpisodeRun (one staging copy + one icrl_host_episode_step launch per env step)
  (b) stepped path   utils.SteppedEpisodeRun over the same host env, forced with ICRL_HOST_EPISODES_STEPPED=1, same process
  (c) env alone      HostVecEnv.step_host over the same env
  (d) device env     icrl_sample_episodes over HipSynthVecEnv (HCWithPos-v0), sequential episodes in one launch

printed as one more JSON line after the rollout table (--N with no value skips that table).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class NullHC:
    """HC-shaped, no dynamics: zeros in, zeros out, never done."""

    def __init__(self):
        from icrl_amd import spaces
        self.observation_space = spaces.Box(-np.inf, np.inf, (18,), np.float64)
        self.action_space = spaces.Box(-1.0, 1.0, (6,), np.float32)
        self._max_episode_steps = 1000
        self._obs = np.zeros(18, np.float64)

    def seed(self, s=None):
        return [s]

    def reset(self):
        return self._obs

    def step(self, a):
        return self._obs, 0.0, False, {}


class NullHCEpisodes(NullHC):
    """NullHC whose episodes end at the 1000-step limit (the episode mode needs `done`)."""

    def __init__(self):
        super().__init__()
        self._t = 0

    def reset(self):
        self._t = 0
        return self._obs

    def step(self, a):
        self._t += 1
        return self._obs, 0.0, self._t >= self._max_episode_steps, {}


def _agent(env, T):
    import torch
    from icrl_amd.constraint_net import ConstraintNet
    from icrl_amd.ppo_lag import PPOLagrangian
    lo = -np.ones(6, np.float32)
    torch.manual_seed(0)
    cn = ConstraintNet(18, 6, [64, 64], None, lambda x: 0.05, None, None, False, 0.5, clip_obs=20, action_low=lo, action_high=-lo)
    env.set_cost_function(cn.cost_function)
    agent = PPOLagrangian("TwoCriticsMlpPolicy", env, n_steps=T, seed=0)
    agent._setup_learn(10 * T * env.num_envs)
    return agent


def _time(fn):
    import torch
    fn()                                   # warm-up rollout
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def episodes(E):
    """the episode mode: one warm-up and one timed sample_from_agent of E episodes per figure."""
    import torch
    from icrl_amd import utils
    from icrl_amd.ppo_lag import PPOLagrangian
    from icrl_amd.vec_env import DummyVecEnv, VecNormalizeWithCost
    steps = 1000 * E
    denv = utils.make_eval_env("HCWithPos-v0", False, seed=0)
    agent = PPOLagrangian("TwoCriticsMlpPolicy", utils.make_train_env("HCWithPos-v0", None, True, 0, 1, cost_info_str="cost", reward_gamma=0.99, cost_gamma=0.99), n_steps=64, seed=0)
    henv = VecNormalizeWithCost(DummyVecEnv([NullHCEpisodes]), training=False, norm_reward=False, norm_cost=False)
    noise = torch.randn(steps, 6, device="cuda")

    def sample(env, stepped):
        if stepped:
            os.environ["ICRL_HOST_EPISODES_STEPPED"] = "1"
        else:
            os.environ.pop("ICRL_HOST_EPISODES_STEPPED", None)
        try:
            run = utils._run_episodes(agent, env, E, False, noise, False)
        finally:
            os.environ.pop("ICRL_HOST_EPISODES_STEPPED", None)
        assert int(run.lengths.sum()) == steps
        return run
    assert isinstance(sample(henv, False), utils.HostEpisodeRun) and isinstance(sample(henv, True), utils.SteppedEpisodeRun)
    a = _time(lambda: sample(henv, False))
    b = _time(lambda: sample(henv, True))
    act = np.zeros((1, 6), np.float32)
    c = _time(lambda: [henv.unwrapped.step_host(act) for _ in range(steps)])
    d = _time(lambda: sample(denv, False))
    row = dict(mode="episodes", episodes=E, steps=steps, host_path_us=1e6 * a / steps, stepped_path_us=1e6 * b / steps,
               env_alone_us=1e6 * c / steps, device_env_us=1e6 * d / steps)
    print(json.dumps({k: (round(v, 2) if isinstance(v, float) else v) for k, v in row.items()}), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=1024)
    ap.add_argument("--N", type=int, nargs="*", default=[8, 64, 128])
    ap.add_argument("--episodes", type=int, default=0, help="episode mode: this many 1000-step episodes of one env per figure (0: off)")
    args = ap.parse_args()
    import torch
    from icrl_amd import utils
    from icrl_amd.vec_env import DummyVecEnv, VecCostWrapper, VecNormalizeWithCost
    T, rows = args.T, []
    for N in args.N:
        env = VecNormalizeWithCost(VecCostWrapper(DummyVecEnv([NullHC] * N)))
        agent = _agent(env, T)
        henv = env.unwrapped
        assert agent._host_rollout_ok("cost", T, agent.rollout_buffer)
        a = _time(lambda: agent.collect_rollouts(env, None, agent.rollout_buffer, T, "cost"))
        b = _time(lambda: agent._collect_rollouts_stepped(env, None, agent.rollout_buffer, T, "cost",
                                                          noise=agent._draw_action_noise(T)))
        act = np.zeros((N, 6), np.float32)
        c = _time(lambda: [henv.step_host(act) for _ in range(T)])
        denv = utils.make_train_env("HCWithPos-v0", None, True, 0, N, cost_info_str="cost", reward_gamma=0.99, cost_gamma=0.99)
        dagent = _agent(denv, T)
        d = _time(lambda: dagent.collect_rollouts(denv, None, dagent.rollout_buffer, T, "cost"))
        row = dict(N=N, T=T, host_path_us=1e6 * a / T, stepped_path_us=1e6 * b / T, env_alone_us=1e6 * c / T, device_env_us=1e6 * d / T)
        rows.append(row)
        print(json.dumps({k: (round(v, 2) if isinstance(v, float) else v) for k, v in row.items()}), flush=True)
    if args.episodes > 0:
        rows.append(episodes(args.episodes))
    return rows


if __name__ == "__main__":
    main()
