"""Per-env-step cost of a rollout whose env cost is an analytic cost (true_constraint_net.AnalyticCost), one process, one GPU
(DESIGN.md section 13).  HC-shaped device env (HCWithPos-v0), 64 envs, T = 512, one timed rollout after a warm-up rollout:

  (a) fused     wall_behind(0.0) inside the persistent rollout launch (icrl_rollout_collect_ex with an icrl_cost_fn_t)
  (b) stepped   the same cost object through the per-step loop (ICRL_ANALYTIC_COST_STEPPED=1: PPOLagrangian._collect_rollouts_stepped,
                the path `cpg` without --cn_path took before the descriptor existed)
  (c) net       the persistent rollout with a [20] constraint net, for reference ((a) does strictly less device work)

the same three for a discriminator cost (gail_utils.DiscriminatorCost, the cost of `cpg --load_gail`):

  (d) fused     a [40, 40] discriminator read as D inside the persistent rollout launch (icrl_cost_disc_t)
  (e) stepped   the same object through the per-step loop (ICRL_DISC_COST_STEPPED=1: the path `cpg --load_gail` took before)
  (f) net       the persistent rollout with a [40, 40] constraint net: the device work of (d) but for one subtraction

three legs for a region cost (true_constraint_net.RegionCost, the cost of `--cost_spec`), interleaved with (a) in
--region_runs passes of one process, (a) being the yardstick of (g):

  (g) fused     a RegionCost written as wall_behind(0.0) inside the persistent rollout launch (icrl_cost_region_t)
  (h) stepped   the same object through the per-step loop (ICRL_REGION_COST_STEPPED=1)
  (i) fused     an 8 x 8 spec (8 clauses of 8 terms) inside the persistent rollout launch

and (a), (b) for 8 envs over the do-nothing host env of tools/host_env_bench.py (icrl_host_step against the per-step loop).
One JSON line per figure set, microseconds per env step.  usage: python tools/cost_fn_bench.py [--T 512] [--N 64] [--host_N 8] [--region_runs 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _time(fn):
    import torch
    fn()                                   # warm-up rollout
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _agent(env, T, cost):
    from icrl_amd.ppo_lag import PPOLagrangian
    env.set_cost_function(cost)
    agent = PPOLagrangian("TwoCriticsMlpPolicy", env, n_steps=T, seed=0)
    agent._setup_learn(10 * T * env.num_envs)
    return agent


_SWITCHES = ("ICRL_ANALYTIC_COST_STEPPED", "ICRL_DISC_COST_STEPPED", "ICRL_REGION_COST_STEPPED")


def _full_spec(obs_dim, acs_dim):
    """8 clauses of 8 terms each, the three types in turn, combine = sum"""
    total = obs_dim + acs_dim
    clauses = []
    for c in range(8):
        idx = [(3 * c + 5 * k) % total for k in range(8)]
        cols = [f"obs:{i}" if i < obs_dim else f"act:{i - obs_dim}" for i in idx]
        if c % 3 == 0:
            q = dict(type="box", cols=cols, lo=[-1.0 - 0.125 * k for k in range(8)], hi=[1.0 + 0.125 * k for k in range(8)])
        elif c % 3 == 1:
            q = dict(type="halfspace", cols=cols, w=[(0.5, -0.25, 1.0, -2.0)[(k + c) % 4] for k in range(8)], b=0.125 * (c - 4))
        else:
            q = dict(type="ball", cols=cols, center=[0.125 * ((k + c) % 5 - 2) for k in range(8)], radius=2.0 + 0.25 * c)
        clauses.append(q)
    return dict(combine="sum", clauses=clauses)


def _rollout(agent, env, T, stepped):
    """one rollout through collect_rollouts, the switch deciding the path; returns which path ran."""
    for switch in _SWITCHES:
        if stepped:
            os.environ[switch] = "1"
        else:
            os.environ.pop(switch, None)
    try:
        fused = agent._fused_rollout_ok("cost", T, agent.rollout_buffer) or agent._host_rollout_ok("cost", T, agent.rollout_buffer)
        agent.collect_rollouts(env, None, agent.rollout_buffer, T, "cost")
    finally:
        for switch in _SWITCHES:
            os.environ.pop(switch, None)
    return fused


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=512)
    ap.add_argument("--N", type=int, default=64)
    ap.add_argument("--host_N", type=int, default=8)
    ap.add_argument("--region_runs", type=int, default=3)
    args = ap.parse_args()
    import torch
    from host_env_bench import NullHC
    from icrl_amd import utils
    from icrl_amd.constraint_net import ConstraintNet
    from icrl_amd.gail_utils import DiscriminatorCost, GailDiscriminator
    from icrl_amd.true_constraint_net import AnalyticCost, RegionCost
    from icrl_amd.vec_env import DummyVecEnv, VecCostWrapper, VecNormalizeWithCost
    T, N = args.T, args.N

    def device_env():
        return utils.make_train_env("HCWithPos-v0", None, True, 0, N, cost_info_str="cost", reward_gamma=0.99, cost_gamma=0.99)
    env = device_env()
    agent = _agent(env, T, AnalyticCost.wall_behind(0.0))
    assert _rollout(agent, env, T, False) and not _rollout(agent, env, T, True)
    a = _time(lambda: _rollout(agent, env, T, False))
    b = _time(lambda: _rollout(agent, env, T, True))
    lo = -np.ones(6, np.float32)
    torch.manual_seed(0)
    cn = ConstraintNet(18, 6, [20], None, lambda x: 0.05, None, None, False, 0.5, clip_obs=20, action_low=lo, action_high=-lo)
    nenv = device_env()
    nagent = _agent(nenv, T, cn.cost_function)
    c = _time(lambda: _rollout(nagent, nenv, T, False))
    row = dict(env="device", N=N, T=T, fused_analytic_us=1e6 * a / T, stepped_analytic_us=1e6 * b / T, fused_net_us=1e6 * c / T)
    print(json.dumps({k: (round(v, 2) if isinstance(v, float) else v) for k, v in row.items()}), flush=True)
    rows = [row]
    # (d) - (f): a [40, 40] discriminator as the env cost, fused and through the per-step loop, and the constraint net of the same shape
    torch.manual_seed(0)
    disc = GailDiscriminator(18, 6, [40, 40], None, lambda x: 0.0, None, None, False, optimizer_class=None)
    denv = device_env()
    dagent = _agent(denv, T, DiscriminatorCost(disc))
    assert _rollout(dagent, denv, T, False) and not _rollout(dagent, denv, T, True)
    d = _time(lambda: _rollout(dagent, denv, T, False))
    e = _time(lambda: _rollout(dagent, denv, T, True))
    torch.manual_seed(0)
    cn2 = ConstraintNet(18, 6, [40, 40], None, lambda x: 0.05, None, None, False, 0.5, clip_obs=None, action_low=None, action_high=None)
    fenv = device_env()
    fagent = _agent(fenv, T, cn2.cost_function)
    f = _time(lambda: _rollout(fagent, fenv, T, False))
    row = dict(env="device", cost="discriminator [40, 40]", N=N, T=T, fused_disc_us=1e6 * d / T, stepped_disc_us=1e6 * e / T, fused_net_us=1e6 * f / T,
               stepped_over_fused=e / d)
    print(json.dumps({k: (round(v, 2) if isinstance(v, float) else v) for k, v in row.items()}), flush=True)
    rows.append(row)
    if args.region_runs > 0:      # (g) - (i), each pass next to (a) of the same pass
        genv, ienv = device_env(), device_env()
        gagent = _agent(genv, T, RegionCost.wall_behind(0.0, 0, 18, 6))
        iagent = _agent(ienv, T, RegionCost.from_spec(_full_spec(18, 6), 18, 6))
        assert _rollout(gagent, genv, T, False) and not _rollout(gagent, genv, T, True) and _rollout(iagent, ienv, T, False)
        for run in range(args.region_runs):
            a = _time(lambda: _rollout(agent, env, T, False))
            g = _time(lambda: _rollout(gagent, genv, T, False))
            h = _time(lambda: _rollout(gagent, genv, T, True))
            i = _time(lambda: _rollout(iagent, ienv, T, False))
            row = dict(env="device", cost="region", run=run + 1, N=N, T=T, fused_analytic_us=1e6 * a / T, fused_region_wall_us=1e6 * g / T,
                       stepped_region_wall_us=1e6 * h / T, fused_region_8x8_us=1e6 * i / T, stepped_over_fused=h / g)
            print(json.dumps({k: (round(v, 2) if isinstance(v, float) else v) for k, v in row.items()}), flush=True)
            rows.append(row)
    if args.host_N > 0:
        H = args.host_N
        henv = VecNormalizeWithCost(VecCostWrapper(DummyVecEnv([NullHC] * H)))
        hagent = _agent(henv, T, AnalyticCost.wall_behind(0.0))
        assert _rollout(hagent, henv, T, False) and not _rollout(hagent, henv, T, True)
        a = _time(lambda: _rollout(hagent, henv, T, False))
        b = _time(lambda: _rollout(hagent, henv, T, True))
        row = dict(env="host", N=H, T=T, fused_analytic_us=1e6 * a / T, stepped_analytic_us=1e6 * b / T)
        print(json.dumps({k: (round(v, 2) if isinstance(v, float) else v) for k, v in row.items()}), flush=True)
        rows.append(row)
    return rows


if __name__ == "__main__":
    main()
