"""GPU: the Point envs on the device (icrl_env_t.reward_form 4..8, point_step_wave in csrc/rollout.hip).

Same float32 actions on both sides (the step kernel against the reference's recording g23): the bounds of tests/test_point_env_cpu.py —
ori bit for bit, x / y within k * 2^-46 after k steps of an episode, reward within 4 k * 2^-46, dones equal, sequences "back" / "front"
bit for bit.  The bound rests on device sin / cos within 2 ulp (HIP's documented double-precision bound for sin, cos and sincos) and the
host's within 1 ulp: |error| <= 3 ulp(1) of a value <= 1, times |a0| <= 0.25, inside the 4 ulp(1) * 0.25 the bound budgets per step.

Device-computed actions (fused rollouts, sampling, learn()): float32 action differences enter an env that integrates them; the figures
are those of tests/test_rollout_gpu.py::test_fused_rollout_vs_port (planes rtol 5e-4 / atol 5e-5, moments rtol 1e-5) and of
tests/test_icrl_trajectory_gpu.py (learn()).
"""
import os
import types

import numpy as np
import pytest
import torch

from helpers import point_env, routes
from oracle import loop as o_loop, nets as o_nets, stats as o_stats
from oracle.streams import SeededStreams
from test_point_env_cpu import IDS, KINDS, SEQS, compare_with_golden

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
POINT_CN = os.path.join(HERE, "golden", "ref_artifacts", "point_best_cn_model.pt")
_BUF_KEYS = ("observations", "orig_observations", "new_observations", "new_orig_observations", "actions", "rewards", "costs",
             "orig_costs", "dones", "log_probs", "reward_values", "cost_values", "reward_advantages", "cost_advantages",
             "reward_returns", "cost_returns")


def _port_stack(n, kind, training=True, norm_reward=True, norm_cost=True, cost_fn=None):
    env = point_env.PointVecEnv(n, kind)
    norm = o_stats.NormState(n, env.obs_dim, training=training, norm_obs=True, norm_reward=norm_reward, norm_cost=norm_cost, clip_obs=10.0,
                             clip_reward=10.0, clip_cost=10.0, reward_gamma=0.99, cost_gamma=0.99, epsilon=1e-8)
    return o_loop.EnvStack(env, norm, cost_fn)


def _wall_cost(obs, acs):
    return (obs[..., 0] <= -3.0).astype(np.float32)


def _load_point_cn():
    """the transfer of icrl/cpg.py:89-103: the AntWall-trained net on the Point env's x / y, through the (quirky) load."""
    from icrl_amd.constraint_net import ConstraintNet
    lo = np.full(2, -0.25, np.float32)
    cn = ConstraintNet.load(POINT_CN, obs_dim=9, acs_dim=2, is_discrete=False, obs_select_dim=[0, 1], acs_select_dim=[-1],
                            clip_obs=None, obs_mean=None, obs_var=None, action_low=lo, action_high=-lo)
    ocn = o_nets.CostNet(9, 2, [40, 40], False, [0, 1], [-1], None, None, None)      # what the off-by-one load() leaves
    ocn.load_state_dict(cn.state_dict())
    return cn, ocn


def test_point_constraint_net_loads():
    cn, _ = _load_point_cn()
    assert list(cn.select_dim) == [0, 1] and cn.input_dims == 2 and list(cn.hidden_sizes) == [40, 40]
    assert (cn.obs_dim, cn.acs_dim) == (9, 2) and cn.clip_obs is None and cn.action_low is None and not cn.wide
    obs = np.zeros((3, 9)); obs[:, 0] = (-5.0, 0.0, 5.0)
    c = cn.cost_function(obs, np.zeros((3, 2), np.float32))
    assert np.all(np.isfinite(c)) and np.all((0 <= c) & (c <= 1))


# ---- 1. the step kernel against the reference's recording ------------------------------------------------------------------------
@pytest.mark.parametrize("env_id", list(IDS))
def test_step_kernel_vs_reference_recording(golden, env_id):
    from icrl_amd.vec_env import HipSynthVecEnv
    g = golden("g23_point_env")
    kind = IDS[env_id][0]
    worst = [0.0, 0.0]
    for seq in SEQS:
        acts = torch.as_tensor(g[f"{kind}/{seq}/actions"], device="cuda")
        S, N = acts.shape[:2]
        env = HipSynthVecEnv.make(env_id, N, seed=3)
        env.s.fill_(7.0)
        assert not env.reset().any().item() and not env.t_ep.any().item()
        obs, rew, done, tep = (torch.empty(S, N, 9, dtype=torch.float64, device="cuda"), torch.empty(S, N, dtype=torch.float64, device="cuda"),
                               torch.empty(S, N, dtype=torch.uint8, device="cuda"), torch.empty(S, N, dtype=torch.int32, device="cuda"))
        for t in range(S):
            obs[t], rew[t], done[t], _ = env.step(acts[t])
            tep[t] = env.t_ep
        obs, rew, done, tep = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy().astype(bool), tep.cpu().numpy()
        ex, er = compare_with_golden(g, kind, seq, obs, rew, done)
        worst = [max(worst[0], ex), max(worst[1], er)]
        # t_ep: the step's index within its episode, 0 after an end; auto-reset to zeros; the step counter advances by one per step
        run = np.zeros(N, np.int64)
        for t in range(S):
            run = np.where(done[t], 0, run + 1)
            assert np.array_equal(tep[t], run), (seq, t)
        assert not obs[done].any() and (tep < 150).all()
        assert np.array_equal(env.step_count.cpu().numpy(), np.full(N, S))
    print(f"{env_id}: worst x / y error {worst[0]:.3f} and reward error {worst[1]:.3f} of their bounds")


# ---- 2. fused rollouts against the CPU port over the numpy definition ------------------------------------------------------------
# "auto": the multi-env kernel at 12 <= N <= 96 (the one-workgroup-per-env persistent kernel is built without the Point step, see
# env_step_wave), the per-step launches below 12 envs, the column-partitioned kernel above 96 (128); "multi": several envs per workgroup
# forced (its Point envs step through env_step_wave, one env per wave; 8 envs: refused by its shape rule, per-step launches);
# "steps": one launch per env step
# (envs, rollout_kernel) -> what icrl_rollout_collect must have launched (9 observations: 11 statistics, the multi-env kernel takes >= 12 envs)
_ROUTES = {(4, "auto"): "per-step", (64, "auto"): dict(route="multi", envs_per_wg=8, wgs=8), (64, "multi"): dict(route="multi", envs_per_wg=8, wgs=8),
           (8, "multi"): "per-step", (128, "auto"): dict(route="wide", wgs=128), (4, "steps"): "per-step"}


@pytest.mark.parametrize("cost", ["wall", "cn"])
@pytest.mark.parametrize("N,T,kernel", [(4, 160, "auto"), (64, 40, "auto"), (64, 40, "multi"), pytest.param(8, 160, "multi", id="8-160-multi-falls-to-per-step"), (128, 20, "auto"), (4, 40, "steps")])
def test_fused_rollout_vs_port(N, T, kernel, cost):
    from icrl_amd.ppo_lag import PPOLagrangian
    from icrl_amd.true_constraint_net import AnalyticCost
    from icrl_amd.vec_env import HipSynthVecEnv, VecCostWrapper, VecNormalizeWithCost
    torch.manual_seed(5)
    env = VecNormalizeWithCost(VecCostWrapper(HipSynthVecEnv(N, "point_circle", 7)))
    if cost == "wall":
        env.set_cost_function(AnalyticCost.wall_behind(-3))
        port_cost = _wall_cost
    else:
        cn, ocn = _load_point_cn()
        env.set_cost_function(cn.cost_function)
        port_cost = ocn.cost_function
    agent = PPOLagrangian("TwoCriticsMlpPolicy", env, n_steps=T, seed=7)
    agent.rollout_kernel = kernel
    assert agent._fused_chain() is not None
    sd = agent.policy.state_dict()
    # a wide action distribution (std e^0.5 against a box of 0.25): the clip is active on most draws, and some envs reach the wall at -3
    sd["log_std"] = torch.full((2,), 0.5)
    sd["action_net.bias"] = torch.as_tensor([-0.2, 0.02])
    agent.policy.load_state_dict(sd)
    stack = _port_stack(N, "point_circle", cost_fn=port_cost)
    port = o_loop.PortAgent(stack, n_steps=T, seed=7)
    port.policy.load_state_dict(agent.policy.state_dict())
    near_end = 150 - T // 3 if T < 150 else None      # every env crosses an episode end inside the rollout
    noise = np.random.RandomState(2).randn(T, N, 2).astype(np.float32)
    agent._setup_learn(N * T)
    port.num_timesteps = 0
    port._last_obs = stack.reset(); port._last_dones = np.zeros(N, bool); port._last_original_obs = stack.old_obs.copy()
    if near_end is not None:
        env.unwrapped.t_ep.fill_(near_end)
        stack.env.t_ep[:] = near_end
    agent.collect_rollouts(env, None, agent.rollout_buffer, T, "cost", noise=torch.as_tensor(noise, device="cuda"))
    routes.check_rollout(_ROUTES[N, kernel], f"point {N} {kernel} {cost}")
    agent.check_rollout_status()
    b = port.collect_rollouts(noise)
    rb = agent.rollout_buffer
    assert b.dones.sum() >= N            # every env crossed an episode end (T >= 150: the time limit)
    if cost == "wall" and T >= 150:
        assert b.orig_costs.sum() > 0    # the wall was reached: the cost plane is not all zeros
    for k in _BUF_KEYS:
        got, ref = getattr(rb, k).cpu().numpy().reshape(T, N, -1), getattr(b, k).reshape(T, N, -1)
        assert np.allclose(got, ref, rtol=5e-4, atol=5e-5), (k, np.abs(got - ref).max())
    assert np.allclose(env.obs_rms.mean, stack.norm.obs_rms.mean, rtol=1e-5, atol=1e-6)
    assert np.allclose(env.obs_rms.var, stack.norm.obs_rms.var, rtol=1e-5, atol=1e-8)
    assert abs(env.ret_rms.var - stack.norm.ret_rms.var) <= 1e-5 * max(1.0, stack.norm.ret_rms.var)
    assert env.obs_rms.count == stack.norm.obs_rms.count
    assert np.array_equal(env.unwrapped.t_ep.cpu().numpy(), stack.env.t_ep)


# ---- 3. episodes that end early: sampling and evaluation on PointCircleTestBack ---------------------------------------------------
def _driven_agent():
    """a policy whose mean action is (-0.25 after the clip, ~0): the point runs into the wall at x = -3 after 13 steps or a few more,
    depending on how far the heading noise turns it."""
    from icrl_amd import utils
    from icrl_amd.ppo_lag import PPOLagrangian
    from icrl_amd.true_constraint_net import AnalyticCost
    train_env = utils.make_train_env("PointCircle-v0", None, True, 5, 4, cost_info_str="cost", reward_gamma=0.99, cost_gamma=0.99)
    train_env.set_cost_function(AnalyticCost.wall_behind(-3))
    agent = PPOLagrangian("TwoCriticsMlpPolicy", train_env, n_steps=32, seed=5)
    sd = agent.policy.state_dict()
    sd["action_net.bias"] = torch.as_tensor([-2.0, 0.0])
    sd["log_std"] = torch.as_tensor([-1.0, -1.0])
    agent.policy.load_state_dict(sd)
    port = o_loop.PortAgent(_port_stack(4, "point_circle"), n_steps=32, seed=5)
    port.policy.load_state_dict(sd)
    return agent, port


def test_early_ending_episodes_vs_port():
    from icrl_amd import utils
    n_ep = 6
    agent, port = _driven_agent()
    noise = np.random.RandomState(3).randn(n_ep * 150, 2).astype(np.float32)
    # the port's sequential one-env loop
    est = _port_stack(1, "point_circle_test_back", training=False, norm_reward=False, norm_cost=False)
    port.stack = est
    p_oo, p_o, p_a, p_r, p_l = o_loop.sample_from_agent(port, est, n_ep, noise)
    assert p_l.min() < 150 and p_l.min() >= 13, p_l                       # at least one episode ended early (and none before step 13)
    ends = np.cumsum(p_l) - 1
    x_end = p_oo[:, 0]
    # the condition under which lengths are comparable: no x of the port within 1e-4 of the wall (the rollout tolerance is 5e-5)
    raw_x = []
    chk = point_env.PointVecEnv(1, "point_circle")       # the same actions through the env without a wall: the x the wall test saw
    k = 0
    for L in p_l:
        chk.reset()
        for _ in range(L):
            raw_x.append(chk.step(p_a[k:k + 1])[0][0, 0]); k += 1
    assert np.abs(np.asarray(raw_x) + 3.0).min() >= 1e-4
    assert (np.asarray(raw_x)[ends[p_l < 150]] < -3.0).all() and not x_end[ends].any()      # ended at the wall; rows hold the reset observation
    # the device: as sample_from_agent / evaluate_policy call it (chain=True) and the pass-by-pass protocol asked for directly
    for chain in (True, False):
        eenv = utils.make_eval_env("PointCircleTestBack-v0", False, seed=5)
        assert eenv.unwrapped.wall_terminate
        run = utils._run_episodes(agent, eenv, n_ep, False, noise, parallel=True, chain=chain)
        assert isinstance(run, utils.EpisodeRun) and not run.fixed_len and run.n_episodes == n_ep
        # every stream but the first started from a guessed position (150 steps per earlier episode): at least one was revised.  (chain=True,
        # what sample_from_agent asks for: the chained kernel does not serve the Point envs, so the positions are settled pass by pass too)
        assert not run.chain_ok()
        assert run.passes >= 2 and run.n_streams in (n_ep, 1)
        oo, o, a, r, l = utils.sample_result(run)
        assert list(l) == list(p_l), (chain, l, p_l)
        for name, got, ref in (("orig_obs", oo, p_oo), ("obs", o, p_o), ("actions", a, p_a)):
            got = got.cpu().numpy()
            assert got.shape == ref.shape and np.allclose(got, ref, rtol=5e-4, atol=5e-5), (chain, name, np.abs(got - ref).max())
        assert np.allclose(r, p_r, rtol=5e-4, atol=5e-5), (chain, r, p_r)
        assert not eenv.unwrapped.s.any().item() and int(eenv.unwrapped.step_count[0].item()) == int(p_l.sum())
    # evaluate_policy: the same episodes' returns
    eenv = utils.make_eval_env("PointCircleTestBack-v0", False, seed=5)
    er, el = utils.evaluate_policy(agent, eenv, n_ep, deterministic=False, return_episode_rewards=True, noise=noise)
    assert list(el) == list(p_l) and np.allclose(er, p_r, rtol=5e-4, atol=5e-5)
    est2 = _port_stack(1, "point_circle_test_back", training=False, norm_reward=False, norm_cost=False)
    port.stack = est2
    pm, ps = o_loop.evaluate_policy(port, est2, n_ep, noise)
    gm, gs = utils.evaluate_policy(agent, utils.make_eval_env("PointCircleTestBack-v0", False, seed=5), n_ep, deterministic=False, noise=noise)
    assert abs(gm - pm) <= 5e-5 + 5e-4 * abs(pm) and abs(gs - ps) <= 5e-5 + 5e-4 * abs(ps)


# ---- 4. the reference's README command (README.md:65), scaled down ---------------------------------------------------------------
def _cpg_cfg(seed, extra=(), nt=4, n_steps=160, rollouts=2):
    from icrl_amd.cpg import build_parser
    argv = ["cpg", "-p", "ICRL-FE2", "--group", "Point-CT-ICRL", "--cn_path", POINT_CN, "-cosd", "0", "1", "-casd", "-1", "-tei", "PointCircle-v0",
            "-eei", "PointCircleTestBack-v0", "-tk", "0.01", "-t", str(rollouts * nt * n_steps), "-plr", "1.0",
            "-nt", str(nt), "--n_steps", str(n_steps), "-s", str(seed), "-v", "0", *extra]
    cfg = vars(build_parser().parse_args(argv))
    cfg.update(rank=0, world_size=1)
    return types.SimpleNamespace(**cfg)


def _tclose(a, b, rtol, atol):
    return abs(a - b) <= atol + rtol * abs(b)


def test_readme_cpg_command_vs_port():
    from icrl_amd import cpg as C, logger
    N, T = 4, 160
    cfg = _cpg_cfg(4)
    cfg.streams = SeededStreams(21)
    model, cb, learn_cost, hist = C.setup(cfg, log=None)
    # the port over the same streams, from the same initial networks
    _, ocn = _load_point_cn()
    stack = _port_stack(N, "point_circle", cost_fn=ocn.cost_function)
    port = o_loop.PortAgent(stack, n_steps=T, batch_size=64, n_epochs=10, target_kl=0.01, penalty_learning_rate=1.0, seed=4)
    port.policy.load_state_dict(model.policy.state_dict())
    model.learn(total_timesteps=int(cfg.timesteps), cost_function=learn_cost, callback=cb)
    hist = hist.history
    lg = dict(logger.Logger.CURRENT.name_to_value)
    assert model.num_timesteps == 2 * N * T and len(hist) == 2
    cn = model.env.venv.constraint_net()
    assert cn is not None and list(cn.select_dim) == [0, 1] and cn.clip_obs is None
    assert model.env.unwrapped.kind == "point_circle" and model.action_space.high.tolist() == [0.25, 0.25]
    bad = {k: v for k, v in lg.items() if isinstance(v, (int, float, np.floating)) and not np.isfinite(v)}
    assert not bad and len(lg) > 10, bad
    assert all(np.isfinite(v) for h in hist for v in h.values()) and "rollout/adjusted_reward" in hist[-1]
    port.learn(2 * N * T, streams=SeededStreams(21))
    assert port.num_timesteps == 2 * N * T
    # tolerances of tests/test_icrl_trajectory_gpu.py (its learn() / forward cases)
    assert abs(lg["train/nu"] - port.logs["train/nu"]) <= 1e-5
    assert lg["train/early_stop_epoch"] == port.logs["train/early_stop_epoch"]
    for k in ("train/average_cost", "train/policy_gradient_loss", "train/reward_value_loss", "train/cost_value_loss",
              "train/mean_reward_advantages", "train/mean_cost_advantages", "train/std"):
        assert _tclose(lg[k], port.logs[k], 2e-4, 2e-5), (k, lg[k], port.logs[k])
    for k, v in model.policy.state_dict().items():
        ref = port.policy.params[k].detach().numpy()
        assert np.allclose(v.numpy(), ref, rtol=1e-3, atol=2e-5), (k, np.abs(v.numpy() - ref).max())


def test_cpg_without_cn_path_trains_against_the_wall():
    """`cpg` without -cp on the Point ids: the ground-truth cost of PointCircleTestBack-v0, wall_behind(-3), inside the rollout launch."""
    from icrl_amd import cpg as C
    cfg = _cpg_cfg(1)
    cfg.cn_path = None
    model, hist = C.cpg(cfg, log=None)
    cost = model.env.venv.analytic_cost()
    assert cost is not None and cost.name == "wall_behind" and cost.lo == -3
    rb = model.rollout_buffer
    assert np.array_equal(rb.orig_costs.cpu().numpy(), (rb.orig_observations.cpu().numpy()[..., 0] <= -3.0).astype(np.float32))
    assert np.isfinite(model.dual.nu().item()) and len(hist) == 2


# ---- 5. a seed batch of two PointCircle runs equals the runs alone, bit for bit ---------------------------------------------------
def test_seed_batch_equals_solo_runs():
    from icrl_amd import cpg as C
    from icrl_amd.seed_batch import run_cpg_seed_batch
    from icrl_amd.streams import PrivateStreams
    seeds = [0, 1]
    mk = lambda sd: _cpg_cfg(sd, ("-ne", "4", "--eval_every_rollouts", "1"), nt=4, n_steps=160, rollouts=1)

    def snap(model, history):
        pol, env, rb = model.policy, model.env, model.rollout_buffer
        return dict(params=pol.params.cpu().numpy().copy(), exp_avg_sq=pol.exp_avg_sq.cpu().numpy().copy(), obs_mean=np.asarray(env.obs_rms.mean).copy(),
                    ret_var=float(env.ret_rms.var), cost_rms=(float(env.cost_rms.mean), float(env.cost_rms.var), float(env.cost_rms.count)),
                    nu=float(model.dual.nu().item()), rewards=rb.rewards.cpu().numpy().copy(), costs=rb.costs.cpu().numpy().copy(),
                    obs=rb.orig_observations.cpu().numpy().copy(), history=[dict(h) for h in history])

    solo = []
    for sd in seeds:
        cfg = mk(sd)
        cfg.streams, cfg.eval_noise_from_streams = PrivateStreams(sd), True
        model, cb, learn_cost, hist = C.setup(cfg, log=None)
        model.learn(total_timesteps=int(cfg.timesteps), cost_function=learn_cost, callback=cb)
        solo.append(snap(model, hist.history))
    out = run_cpg_seed_batch([mk(sd) for sd in seeds])
    assert len(out) == 2 and solo[0]["params"].tobytes() != solo[1]["params"].tobytes()
    for sd, (model, history), want in zip(seeds, out, solo):
        got = snap(model, history)
        assert model.num_timesteps == 4 * 160
        for k in ("params", "exp_avg_sq", "obs_mean", "rewards", "costs", "obs"):
            assert np.array_equal(got[k], want[k]), (sd, k)
        assert got["ret_var"] == want["ret_var"] and got["cost_rms"] == want["cost_rms"] and got["nu"] == want["nu"], sd
        assert len(got["history"]) == len(want["history"]) == 1
        for a, b in zip(got["history"], want["history"]):
            assert a == b, (sd, a, b)
        assert np.abs(got["obs"][..., 0]).max() > 0.5      # the point moved


# ---- 6. --episode_stats on PointNullReward-v0: +1 per step, 150 steps per episode, no tolerance -----------------------------------
def test_episode_stats_on_null_reward():
    from icrl_amd import cpg as C, logger
    cfg = _cpg_cfg(2, ("--episode_stats",), nt=4, n_steps=150, rollouts=2)
    cfg.train_env_id, cfg.eval_env_id, cfg.cn_path = "PointNullReward-v0", "PointNullRewardTest-v0", None
    model, hist = C.cpg(cfg, log=None)
    lg = logger.Logger.CURRENT.name_to_value
    assert model.num_timesteps == 2 * 4 * 150
    assert lg["rollout/ep_rew_mean"] == 150.0 and lg["rollout/ep_len_mean"] == 150.0
    assert model.env.venv.analytic_cost().name == "wall_behind_and_infront"
