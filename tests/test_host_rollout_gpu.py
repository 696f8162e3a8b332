"""GPU: the rollout over host envs (PPOLagrangian._collect_rollouts_host: one icrl_host_step launch per env step) against the device
chain's per-step launches (rollout_kernel="steps") — every buffer plane, the normaliser state and the agent's carry-over state
bit-identical, across two consecutive rollouts and across episode ends; the actions each host env received are the clipped actions."""
import numpy as np
import pytest
import torch

import tests.helpers.host_envs  # noqa: F401  (registers the Host* ids)

pytestmark = pytest.mark.gpu

_BUF_KEYS = ("observations", "orig_observations", "new_observations", "new_orig_observations", "actions", "rewards", "costs",
             "orig_costs", "dones", "log_probs", "reward_values", "cost_values", "reward_advantages", "cost_advantages",
             "reward_returns", "cost_returns")
_DEVICE = {"hc": ("hc", False), "hctest": ("hc", False), "ant": ("ant", False), "antbroken": ("ant", True), "lgw": ("lgw", False),
           "clgw": ("clgw", False)}
_HOST = {"hc": "HostHCWithPos-v0", "hctest": "HostHCWithPosTest-v0", "ant": "HostAntWall-v0", "antbroken": "HostAntWallBroken-v0",
         "lgw": "HostLGW-v0", "clgw": "HostCLGW-v0"}
_EARLY_END = ("clgw", "hctest")      # episodes also end before the time limit (the wall at obs[0] <= -3, the backward action)


def _chain(bottom, cost, norm, seed, hid, norm_kwargs=None):
    from icrl_amd.constraint_net import ConstraintNet
    from icrl_amd.vec_env import VecCostWrapper, VecNormalizeWithCost
    env = VecCostWrapper(bottom) if cost else bottom
    env = VecNormalizeWithCost(env, norm_obs=norm, norm_reward=norm, norm_cost=norm, **(norm_kwargs or {}))
    cn = None
    if cost:
        od, ad = bottom.observation_space.shape[0], bottom.action_space.shape[0]
        lo = -np.ones(ad, np.float32)
        torch.manual_seed(seed)
        cn = ConstraintNet(od, ad, hid, None, lambda x: 0.05, None, None, False, 0.5, clip_obs=20, action_low=lo, action_high=-lo)
        env.set_cost_function(cn.cost_function)
    return env, cn


def _agents(kind, N, T, seed=5, cost=True, norm=True, subproc=False, agent_kwargs=None, norm_kwargs=None):
    from icrl_amd import envs
    from icrl_amd.ppo_lag import PPOLagrangian
    from icrl_amd.vec_env import DummyVecEnv, HipSynthVecEnv, SubprocVecEnv
    k, broken = _DEVICE[kind]
    hid = [20] if k in ("hc", "lgw", "clgw") else [40, 40]
    e_d, cn_d = _chain(HipSynthVecEnv(N, k, seed, broken=broken, wall_terminate=kind in _EARLY_END), cost, norm, seed, hid, norm_kwargs)
    fns = [envs.spec(_HOST[kind])] * N
    e_h, cn_h = _chain((SubprocVecEnv if subproc else DummyVecEnv)(fns), cost, norm, seed, hid, norm_kwargs)
    a_d = PPOLagrangian("TwoCriticsMlpPolicy", e_d, n_steps=T, seed=seed, **(agent_kwargs or {}))
    a_h = PPOLagrangian("TwoCriticsMlpPolicy", e_h, n_steps=T, seed=seed, **(agent_kwargs or {}))
    a_h.policy.load_state_dict(a_d.policy.state_dict())
    if cost:
        cn_h.load_state_dict(cn_d.state_dict())
    a_d.rollout_kernel = "steps"
    return (a_d, e_d), (a_h, e_h)


def _noise(kind, N, T, rollouts=2, shift=0.0):
    rng = np.random.RandomState(8)
    if kind in ("lgw", "clgw"):
        return torch.as_tensor(rng.rand(rollouts, T, N).astype(np.float32), device="cuda")
    ad = 6 if kind in ("hc", "hctest") else 8
    return torch.as_tensor((rng.randn(rollouts, T, N, ad) + shift).astype(np.float32), device="cuda")


def _assert_same(a_d, e_d, a_h, e_h, it=None, carry=True):
    for k in _BUF_KEYS:
        got, ref = getattr(a_h.rollout_buffer, k).cpu().numpy(), getattr(a_d.rollout_buffer, k).cpu().numpy()
        assert np.array_equal(got, ref), (it, k, np.abs(got - ref).max())
    for name in ("obs_rms", "ret_rms", "cost_rms"):
        rh, rd = getattr(e_h, name), getattr(e_d, name)
        assert np.array_equal(np.asarray(rh.mean), np.asarray(rd.mean)) and np.array_equal(np.asarray(rh.var), np.asarray(rd.var)), name
        assert rh.count == rd.count, name
    assert torch.equal(e_h.ret, e_d.ret) and torch.equal(e_h.cost_ret, e_d.cost_ret)
    assert torch.equal(a_h._last_obs, a_d._last_obs) and torch.equal(a_h._ag["last_dones"], a_d._ag["last_dones"])
    assert torch.equal(e_h.unwrapped.s, e_d.unwrapped.s)
    for k in ("raw_cost", "act_clipped", "last_v_r", "last_v_c") if carry else ():      # (the per-step loop keeps these in its locals)
        assert torch.equal(a_h._ag[k], a_d._ag[k]), k


def _received_actions(e_h):
    return np.stack([np.stack([np.asarray(a, np.float64).reshape(-1) for a in acts]) for acts in e_h.unwrapped.get_attr("actions")], 1)


@pytest.mark.parametrize("kind,N,T,cost,norm,subproc", [
    ("hc", 1, 16, True, True, False), ("hc", 7, 24, True, True, False), ("hc", 64, 20, True, True, False), ("hc", 128, 12, True, True, False),
    ("ant", 16, 12, True, True, False), ("antbroken", 8, 12, True, True, False),
    ("lgw", 8, 30, False, False, False), ("clgw", 8, 30, False, False, False),
    ("hc", 8, 16, False, True, False),                      # no cost wrapper (the GAIL chain)
    ("hc", 4, 16, True, True, True),                        # SubprocVecEnv through the host path
])
def test_host_rollout_equals_device_rollout(kind, N, T, cost, norm, subproc, norm_kwargs=None, policy_state=None):
    (a_d, e_d), (a_h, e_h) = _agents(kind, N, T, cost=cost, norm=norm, subproc=subproc, norm_kwargs=norm_kwargs)
    if policy_state is not None:      # a named state of helpers/policy_states.py on top of the fresh policy, in both chains
        from helpers import policy_states
        sd = policy_states.state(policy_state, a_d.policy.state_dict(), a_d.policy.act_dim)
        a_d.policy.load_state_dict(sd); a_h.policy.load_state_dict(sd)
    noise = _noise(kind, N, T)
    a_d._setup_learn(2 * N * T); a_h._setup_learn(2 * N * T)
    limit = e_d.unwrapped.max_steps
    e_d.unwrapped.t_ep.fill_(limit - T // 2)                # every env crosses its time limit inside the first rollout
    e_h.unwrapped.env_method("set_t_ep", limit - T // 2)
    calls = []
    for it in range(2):
        a_d.collect_rollouts(e_d, None, a_d.rollout_buffer, T, "cost", noise=noise[it])
        routed = a_h._host_rollout_ok("cost", T, a_h.rollout_buffer)
        calls.append(routed)
        a_h.collect_rollouts(e_h, None, a_h.rollout_buffer, T, "cost", noise=noise[it])
        _assert_same(a_d, e_d, a_h, e_h, it)
        if it == 0:
            assert a_h.rollout_buffer.dones.sum().item() == N or kind == "clgw"
    assert all(calls)
    # what each host env received is the clipped action of its row (the action index when discrete)
    got = _received_actions(e_h)                                      # [2T, N, act]
    assert got.shape[0] == 2 * T
    last = a_h.rollout_buffer.actions.cpu().numpy().astype(np.float64)      # rows of the second rollout
    if kind in ("lgw", "clgw"):
        assert np.array_equal(got[T:], last)
    else:
        lo, hi = e_h.action_space.low, e_h.action_space.high
        assert np.array_equal(got[T:], np.clip(a_h.rollout_buffer.actions.cpu().numpy(), lo, hi).astype(np.float64))
        assert np.array_equal(got[-1], a_h._ag["act_clipped"].cpu().numpy().astype(np.float64))
    e_h.close()


def _host_agent(kind, N, T, seed=5, streams=None):
    """one agent over a DummyVecEnv chain with a constraint net (no device twin)."""
    from icrl_amd import envs
    from icrl_amd.ppo_lag import PPOLagrangian
    from icrl_amd.vec_env import DummyVecEnv
    env, _ = _chain(DummyVecEnv([envs.spec(_HOST[kind])] * N), True, True, seed, [20])
    return PPOLagrangian("TwoCriticsMlpPolicy", env, n_steps=T, seed=seed, streams=streams), env


def test_host_path_equals_stepped_path_and_alternates():
    """the launch-per-step path and the per-step loop over the same host env: identical, also when the two alternate between rollouts."""
    kind, N, T = "hc", 6, 20
    a_h, e_h = _host_agent(kind, N, T)
    a_s, e_s = _host_agent(kind, N, T)          # same seed: same policy and constraint net
    noise = _noise(kind, N, T, rollouts=3)
    a_h._setup_learn(3 * N * T); a_s._setup_learn(3 * N * T)
    for env in (e_h, e_s):
        env.unwrapped.env_method("set_t_ep", 1000 - T // 2)
    for it, a_s_stepped in enumerate((True, False, True)):      # a_h: always the host path; a_s: per-step loop, host path, per-step loop
        a_h.collect_rollouts(e_h, None, a_h.rollout_buffer, T, "cost", noise=noise[it])
        if a_s_stepped:
            a_s._collect_rollouts_stepped(e_s, None, a_s.rollout_buffer, T, "cost", noise=noise[it])
        else:
            a_s.collect_rollouts(e_s, None, a_s.rollout_buffer, T, "cost", noise=noise[it])
        _assert_same(a_s, e_s, a_h, e_h, it, carry=False)


def test_biased_policy_episodes_end_at_different_steps():
    """HCWithPosTest: actions pushed towards the wall (obs[0] <= -3 ends the episode with reward 0), so episodes end early, at steps that
    differ from env to env and from the time limit — host and device chains stay bit-identical across those ends."""
    from icrl_amd.vec_env import dynamics_matrix
    N, T = 8, 48
    (a_d, e_d), (a_h, e_h) = _agents("hctest", N, T)
    shift = -3.0 * np.sign(dynamics_matrix("hc")[0])          # drives obs[0] down: the wall is hit after ~12 steps
    noise = _noise("hctest", N, T, shift=shift)
    a_d._setup_learn(2 * N * T); a_h._setup_learn(2 * N * T)
    for it in range(2):
        a_d.collect_rollouts(e_d, None, a_d.rollout_buffer, T, "cost", noise=noise[it])
        assert a_h._host_rollout_ok("cost", T, a_h.rollout_buffer)
        a_h.collect_rollouts(e_h, None, a_h.rollout_buffer, T, "cost", noise=noise[it])
        _assert_same(a_d, e_d, a_h, e_h, it)
        starts = a_h.rollout_buffer.dones.cpu().numpy()                       # [T, N]: 1 where an episode begins
        first = [int(np.nonzero(starts[1:, n])[0][0]) + 1 for n in range(N)]
        assert len(set(first)) > 1 and max(first) < T, first                 # early ends, not all at the same step
        assert np.all(starts[1:].sum(0) >= 2)


class _StopAt:
    """callback that ends the rollout at its k-th on_step()."""

    def __init__(self, k):
        self.k, self.calls = k, 0

    def on_rollout_start(self):
        pass

    def on_step(self):
        self.calls += 1
        return self.calls < self.k

    def on_rollout_end(self):
        pass


def test_callback_stop_leaves_the_normaliser_like_the_per_step_loop():
    """a callback ending the rollout after k env steps: the normaliser's statistics and returns and the wrappers' last-step state are
    those of the per-step loop stopped at the same step."""
    kind, N, T, k = "hc", 6, 20, 7
    a_h, e_h = _host_agent(kind, N, T)
    a_s, e_s = _host_agent(kind, N, T)
    noise = _noise(kind, N, T, rollouts=1)
    a_h._setup_learn(N * T); a_s._setup_learn(N * T)
    assert a_h.collect_rollouts(e_h, _StopAt(k), a_h.rollout_buffer, T, "cost", noise=noise[0]) is False
    assert a_s._collect_rollouts_stepped(e_s, _StopAt(k), a_s.rollout_buffer, T, "cost", noise=noise[0]) is False
    assert a_h.num_timesteps == a_s.num_timesteps == k * N
    for name in ("obs_rms", "ret_rms", "cost_rms"):
        rh, rs = getattr(e_h, name), getattr(e_s, name)
        assert np.array_equal(np.asarray(rh.mean), np.asarray(rs.mean)) and np.array_equal(np.asarray(rh.var), np.asarray(rs.var)), name
        assert rh.count == rs.count, name
    assert torch.equal(e_h.ret, e_s.ret) and torch.equal(e_h.cost_ret, e_s.cost_ret)
    assert torch.equal(e_h.get_original_obs(), e_s.get_original_obs()) and torch.equal(e_h.venv.previous_obs, e_s.venv.previous_obs)
    # the agent's carry-over observation is the envs' state after the last step (the per-step loop returns before it updates its own,
    # which leaves it one step behind the envs)
    assert torch.equal(a_h._last_original_obs, e_s.get_original_obs())


def test_learn_two_iterations_equals_device_chain():
    """learn() for two iterations with injected random streams: the host chain (launch per step) and the device chain (one persistent
    launch per rollout) end with bit-identical policy parameters, Adam state, dual variable and train/* values."""
    from icrl_amd import logger
    from icrl_amd.streams import PrivateStreams
    N, T = 8, 64
    (a_d, e_d), (a_h, e_h) = _agents("hc", N, T, agent_kwargs=dict(batch_size=64, n_epochs=2))
    a_d.rollout_kernel = "auto"
    out = []
    for a in (a_d, a_h):
        a.streams = PrivateStreams(3)
        logger.configure()
        a.learn(total_timesteps=2 * N * T, cost_function="cost")
        out.append(dict(logger.Logger.CURRENT.name_to_value))
    assert a_d._n_updates == a_h._n_updates == 2 * 2
    assert torch.equal(a_h.policy.params, a_d.policy.params)
    assert torch.equal(a_h.policy.exp_avg, a_d.policy.exp_avg) and torch.equal(a_h.policy.exp_avg_sq, a_d.policy.exp_avg_sq)
    assert a_h.policy.adam_step == a_d.policy.adam_step
    assert a_h.dual.nu().item() == a_d.dual.nu().item()
    train = sorted(k for k in out[0] if k.startswith("train/"))
    assert train and train == sorted(k for k in out[1] if k.startswith("train/"))
    for key in train:
        assert out[1][key] == out[0][key], (key, out[1][key], out[0][key])


def _same_metric(x, y):
    return x == y or (isinstance(x, float) and isinstance(y, float) and np.isnan(x) and np.isnan(y))


def test_icrl_over_registered_host_envs_repeats_the_device_run(tmp_path):
    """icrl() end to end, 2 outer iterations at a reduced size: `--env_module tests.helpers.host_envs -tei HostHCWithPos-v0 -eei
    HostHCWithPosTest-v0` (train env: SubprocVecEnv of 8 worker processes; sampling / evaluation: the per-step episode loop over a
    DummyVecEnv) logs what the HCWithPos-v0 / HCWithPosTest-v0 run with the same seed logs.  Excluded: the wall-clock entries, and
    true/cost with best_true/best_cost — utils.get_true_cost_function knows the reference's ids only, so for the Host* ids it returns
    null_cost (the reference's behaviour for unknown ids) while HCWithPosTest-v0 gets the wall cost."""
    import types
    import os
    from icrl_amd.icrl import build_parser, icrl
    from icrl_amd.vec_env import SubprocVecEnv
    here = os.path.dirname(os.path.abspath(__file__))
    common = ["icrl", "-er", "2", "-ep", os.path.join(here, "golden/expert_hc.npz"), "-tk", "0.01", "-cl", "20", "-bi", "4", "-ft", "2000",
              "-ni", "2", "-clr", "0.05", "-crc", "0.5", "-psis", "-nt", "8", "--n_steps", "128", "-s", "0", "-v", "0"]
    runs = []
    for ids in (["-tei", "HCWithPos-v0", "-eei", "HCWithPosTest-v0"],
                ["--env_module", "tests.helpers.host_envs", "-tei", "HostHCWithPos-v0", "-eei", "HostHCWithPosTest-v0"]):
        cfg = vars(build_parser().parse_args(common + ids))
        cfg.update(rank=0, world_size=1)
        metrics, agent, cn, env = icrl(types.SimpleNamespace(**cfg), log=None)
        runs.append(metrics)
        if ids[0] == "--env_module":
            assert isinstance(env.unwrapped, SubprocVecEnv) and agent._host_rollout_ok("cost", agent.n_steps, agent.rollout_buffer)
            env.close()
    wall_clock = {"time(m)", "forward/fps", "forward/time_elapsed", "time/fps", "time/time_elapsed"}
    true_cost = {"true/cost", "best_true/best_cost"}
    for dev, host in zip(*runs):
        assert set(dev) == set(host)
        for key in sorted(set(dev) - wall_clock - true_cost):
            assert _same_metric(host[key], dev[key]), (key, host[key], dev[key])
        assert host["true/cost"] == 0.0                     # null_cost


@pytest.mark.parametrize("case", ["n200", "wide", "callable"])
def test_fallbacks_take_the_stepped_path(case):
    """shapes the kernel does not serve take the per-step loop (same noise draws as the fused path) and match the device chain."""
    from icrl_amd.true_constraint_net import null_cost
    N, T = (200, 6) if case == "n200" else (8, 12)
    kw = dict(policy_kwargs=dict(net_arch=[dict(pi=[128, 128], vf=[64, 64], cvf=[64, 64])])) if case == "wide" else None
    (a_d, e_d), (a_h, e_h) = _agents("hc", N, T, agent_kwargs=kw)
    cost = null_cost if case == "callable" else "cost"
    assert not a_h._host_rollout_ok(cost, T, a_h.rollout_buffer)
    noise = _noise("hc", N, T, rollouts=1)
    a_d._setup_learn(N * T); a_h._setup_learn(N * T)
    a_d.collect_rollouts(e_d, None, a_d.rollout_buffer, T, cost, noise=noise[0])
    a_h.collect_rollouts(e_h, None, a_h.rollout_buffer, T, cost, noise=noise[0])
    for k in _BUF_KEYS:
        got, ref = getattr(a_h.rollout_buffer, k).cpu().numpy(), getattr(a_d.rollout_buffer, k).cpu().numpy()
        assert np.allclose(got, ref, rtol=1e-5, atol=1e-6), (case, k, np.abs(got - ref).max())
    e_h.close()
