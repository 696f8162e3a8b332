"""gSDE rollout cases for tests/test_sde_rollout_gpu.py: agents built like _pair_of_agents in tests/test_rollout_gpu.py, each with a gSDE policy at
a trained-like state (helpers/sde_update_cases.trained_like: log_std uniform in [-1.5, 0.5]) and a streams object whose sde_noise(shape) serves a
recorded numpy sequence — so every agent of a case holds the same matrices whichever way it collects: one persistent launch, the per-step
launches, or the Python loop (which asks for the same normals in the same order)."""
import numpy as np
import torch

from helpers import routes
from helpers import sde_update_cases as U

BUF_KEYS = ("observations", "orig_observations", "new_observations", "new_orig_observations", "actions", "rewards", "costs", "orig_costs", "dones", "log_probs",
            "reward_values", "cost_values", "reward_advantages", "cost_advantages", "reward_returns", "cost_returns")
AG_KEYS = ("raw_rew", "raw_cost", "dones", "last_v_r", "last_v_c", "act_clipped")
DIMS = {"hc": (18, 6, 1000), "ant": (113, 8, 500)}      # obs, act, the env's time limit
PL = dict(pi=[32, 48], vf=[64, 64], cvf=[64, 64])       # -pl 32 48: a padded latent


class RecordedNoise:
    """the `streams` protocol's sde_noise alone: standard normals from a numpy generator of its own, every answer kept (float32, in call order)"""

    def __init__(self, seed):
        self.rng = np.random.RandomState(seed)
        self.calls = []

    def sde_noise(self, shape):
        z = self.rng.randn(*shape).astype(np.float32)
        self.calls.append(z)
        return z


def agents(N, T, ssf, modes, seed=13, kind="hc", cost="net", arch=None):
    """one agent per entry of `modes`, all in the same state: "auto" (sde_fused_rollout, the launch the library picks), "steps" (sde_fused_rollout with
    rollout_kernel = "steps": the per-step launches), "loop" (the switch off: the Python loop).  cost: "net" a constraint net, "wall" the analytic
    wall cost on observation column 0, "none" no cost wrapper in the chain.  Returns [(agent, env)]."""
    from icrl_amd.constraint_net import ConstraintNet
    from icrl_amd.ppo_lag import PPOLagrangian
    from icrl_amd.true_constraint_net import AnalyticCost
    from icrl_amd.vec_env import HipSynthVecEnv, VecCostWrapper, VecNormalizeWithCost
    od, ad, limit = DIMS[kind]
    lo = -np.ones(ad, np.float32)
    out, cns = [], []
    for mode in modes:
        torch.manual_seed(seed)
        base = HipSynthVecEnv(N, kind, seed)
        env = VecNormalizeWithCost(base if cost == "none" else VecCostWrapper(base))
        if cost == "net":
            cns.append(ConstraintNet(od, ad, [20] if kind == "hc" else [40, 40], None, lambda x: 0.05, None, None, False, 0.5, clip_obs=20, action_low=lo, action_high=-lo))
            env.set_cost_function(cns[-1].cost_function)
        elif cost == "wall":
            env.set_cost_function(AnalyticCost.wall_behind(0.0))      # threshold 0: both outcomes occur on this env
        kw = dict(policy_kwargs=dict(net_arch=[dict(arch)])) if arch is not None else {}
        agent = PPOLagrangian("TwoCriticsMlpPolicy", env, n_steps=T, seed=seed, use_sde=True, sde_sample_freq=ssf, sde_fused_rollout=mode != "loop",
                              streams=RecordedNoise(seed + 1), **kw)
        if mode == "steps":
            agent.rollout_kernel = "steps"
        out.append((agent, env))
    for cn in cns[1:]:
        cn.load_state_dict(cns[0].state_dict())
    U.trained_like(out[0][0].policy, 100 + seed)
    for agent, _ in out[1:]:
        agent.policy.load_state_dict(out[0][0].policy.state_dict())
    for agent, env in out:
        agent._setup_learn(2 * N * T)
        env.unwrapped.t_ep.fill_(limit - T // 2)      # every env crosses its time limit inside the first rollout
    return out


def expect_route(agent, route, N, T, what):
    """the record of the agent's last rollout call: the route with ICRL_PICK_SDE set (persistent: N workgroups, one launch; per-step: 2 T launches)"""
    from icrl_amd import _lib
    want = dict(route="persistent", wgs=N, launches=1, n_runs=1) if route == "persistent" else dict(route="per-step", launches=2 * T, n_runs=1)
    got = routes.check_rollout(want, what)
    assert got["pick"] & _lib.PICK_SDE, (what, got)
    assert agent.last_sde_rollout == "fused" and agent.last_sde_rollout_reason is None, (agent.last_sde_rollout, agent.last_sde_rollout_reason)
    return got


def assert_rollouts_bit_equal(a, b, it):
    (a_p, e_p), (a_s, e_s) = a, b
    for k in BUF_KEYS:
        got, ref = getattr(a_p.rollout_buffer, k).cpu().numpy(), getattr(a_s.rollout_buffer, k).cpu().numpy()
        assert np.array_equal(got, ref), (it, k, np.abs(got - ref).max())
    for name in ("obs_rms", "ret_rms", "cost_rms"):
        rp, rs = getattr(e_p, name), getattr(e_s, name)
        assert np.array_equal(np.asarray(rp.mean), np.asarray(rs.mean)) and np.array_equal(np.asarray(rp.var), np.asarray(rs.var)), (it, name)
        assert rp.count == rs.count, (it, name)
    assert torch.equal(e_p.ret, e_s.ret) and torch.equal(e_p.cost_ret, e_s.cost_ret)
    assert torch.equal(a_p._last_obs, a_s._last_obs) and torch.equal(a_p._ag["last_dones"], a_s._ag["last_dones"])
    assert torch.equal(e_p.unwrapped.s, e_s.unwrapped.s) and torch.equal(e_p.unwrapped.t_ep, e_s.unwrapped.t_ep)
    for k in AG_KEYS:
        assert torch.equal(a_p._ag[k], a_s._ag[k]), (it, k)


def matrices_of_step(agent, rollout, t, T, ssf):
    """from the recorded normals alone: the matrices [N, H, A] (float64) the loop holds at step t of rollout `rollout` (0-based) — each reset_noise asks
    for (H, A) then (n, H, A); a rollout makes 1 + ceil(T / ssf) of them (one with ssf < 0); with one env the (H, A) matrix is the one in use"""
    per = 1 + (-(-T // ssf) if ssf > 0 else 0)
    d = rollout * per + (1 + t // ssf if ssf > 0 else 0)
    calls = agent.streams.calls
    z = calls[2 * d][None] if agent.n_envs == 1 else calls[2 * d + 1]
    std = np.exp(agent.policy.log_std.cpu().numpy())      # float32, as reset_noise multiplies
    return (z * std).astype(np.float64)
