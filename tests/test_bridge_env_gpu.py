"""GPU: the dense Two Bridges envs and PointTrack on the device (icrl_env_t.reward_form 9..14: point_step_wave / bridge_step_wave in
csrc/rollout.hip).

1. The step kernel on the recorded float32 actions against the reference's recording g24, at the bounds of tests/test_bridge_env_cpu.py
   (derived there and in DESIGN §21): discrete positions / dones / constant rewards bit for bit and the dense reward within 4 * 2^-52
   relative; continuous ori bit for bit, x / y within k * 2^-47, the dense reward within (400 k + 25) * 2^-47; PointTrack at the Point
   bounds.  The device's sin / cos are within 2 ulp and its sqrt within 1 ulp (HIP's documented double-precision bounds).
2. Every fused launch form against the per-step launches, bit for bit, over two rollouts with carry-over.  The multi-env kernel takes
   continuous actions only (its launcher keeps discrete policies elsewhere, as for LapGridWorld): a Categorical policy at 16 envs runs
   as per-step launches of the fused act-step kernel, and the column-partitioned kernel is its one-launch form (forced at 16 envs,
   chosen above 96).
3. sample_from_agent / evaluate_policy against the per-step episode loop.
4. cpg end to end: inside the fused launches with the null cost, through the per-step loop against BridgesCost, and a seed batch.
"""
import types

import numpy as np
import pytest
import torch

from helpers import bridge_env, routes
from test_bridge_env_cpu import IDS, SEQS, compare_with_golden

pytestmark = pytest.mark.gpu
BUF_KEYS = ("observations", "orig_observations", "new_observations", "new_orig_observations", "actions", "rewards", "costs",
            "orig_costs", "dones", "log_probs", "reward_values", "cost_values", "reward_advantages", "cost_advantages",
            "reward_returns", "cost_returns")
RIGHT, LEFT, UP, DOWN = 0, 1, 2, 3


# ---- 1. the step kernel against the reference's recording ------------------------------------------------------------------------
@pytest.mark.parametrize("env_id", list(IDS))
def test_step_kernel_vs_reference_recording(golden, env_id):
    from icrl_amd.vec_env import HipSynthVecEnv
    g = golden("g24_bridge_env")
    kind = IDS[env_id]
    O, A, max_steps = bridge_env.DIMS[kind]
    start = torch.zeros(O, dtype=torch.float64, device="cuda")
    if kind == "ddcdd2b":
        start[:2] = torch.as_tensor([3.0, 5.0], dtype=torch.float64)
    worst = [0.0, 0.0]
    for seq in SEQS[kind]:
        acts = torch.as_tensor(g[f"{kind}/{seq}/actions"], device="cuda")
        S, N = acts.shape[:2]
        env = HipSynthVecEnv.make(env_id, N, seed=3)
        env.s.fill_(7.0)
        assert torch.equal(env.reset(), start.repeat(N, 1)) and not env.t_ep.any().item()
        obs, rew, done, tep = (torch.empty(S, N, O, dtype=torch.float64, device="cuda"), torch.empty(S, N, dtype=torch.float64, device="cuda"),
                               torch.empty(S, N, dtype=torch.uint8, device="cuda"), torch.empty(S, N, dtype=torch.int32, device="cuda"))
        for t in range(S):
            obs[t], rew[t], done[t], _ = env.step(acts[t])
            tep[t] = env.t_ep
        obs, rew, done, tep = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy().astype(bool), tep.cpu().numpy()
        ex, er = compare_with_golden(g, kind, seq, obs, rew, done)
        worst = [max(worst[0], ex), max(worst[1], er)]
        # t_ep: the step's index within its episode, 0 after an end; auto-reset to the start; the step counter advances by one per step
        run = np.zeros(N, np.int64)
        for t in range(S):
            run = np.where(done[t], 0, run + 1)
            assert np.array_equal(tep[t], run), (seq, t)
        assert np.array_equal(obs[done], np.tile(start.cpu().numpy(), (int(done.sum()), 1))) and (tep < max_steps).all()
        assert done.sum() == N * (S // max_steps)
        assert np.array_equal(env.step_count.cpu().numpy(), np.full(N, S))
    print(f"{env_id}: worst x / y error {worst[0]:.3f} and reward error {worst[1]:.3f} of their bounds")


def test_action_index_outside_the_moves_stays_put():
    """documented: an index outside 0..3 (the reference raises a KeyError) moves nowhere and is rewarded as a step to the same place."""
    from icrl_amd.vec_env import HipSynthVecEnv
    env = HipSynthVecEnv.make("DD2B-v0", 2, seed=0)
    env.reset()
    obs, rew, done, _ = env.step(torch.as_tensor([[7.0], [-1.0]], device="cuda"))
    assert not obs.any().item() and rew.tolist() == [-1.0, -1.0] and not done.any().item()


# ---- 2. every fused launch form against the per-step launches --------------------------------------------------------------------
def _policy_state(agent, kind):
    """a trained-like state: the discrete agent heads right and down (into the water's edge at x = 3.5 and the wall at y = 0 within a
    few steps), the continuous one moves with a wide distribution (std e^0.5 against a box of 2: the clip is active on many draws)."""
    sd = agent.policy.state_dict()
    if kind == "dd2b":
        sd["action_net.bias"] = torch.as_tensor([1.5, -1.0, 0.0, 0.5])
    else:
        sd["log_std"] = torch.full((2,), 0.5)
        sd["action_net.bias"] = torch.as_tensor([1.0, 0.1])
    agent.policy.load_state_dict(sd)


def _pair(N, T, seed, kind):
    from icrl_amd.ppo_lag import PPOLagrangian
    from icrl_amd.true_constraint_net import AnalyticCost
    from icrl_amd.vec_env import HipSynthVecEnv, VecCostWrapper, VecNormalizeWithCost
    out = []
    for _ in range(2):
        torch.manual_seed(seed)
        env = VecNormalizeWithCost(VecCostWrapper(HipSynthVecEnv(N, kind, seed)))
        env.set_cost_function(AnalyticCost.wall_infront(1.0))      # obs[0] >= 1: a cost plane that is not constant
        agent = PPOLagrangian("TwoCriticsMlpPolicy", env, n_steps=T, seed=seed)
        _policy_state(agent, kind)
        out.append((agent, env))
    out[1][0].policy.load_state_dict(out[0][0].policy.state_dict())
    return out


def _noise(kind, rollouts, T, N, seed=8):
    rng = np.random.RandomState(seed)
    if kind == "dd2b":
        return torch.as_tensor(rng.rand(rollouts, T, N).astype(np.float32), device="cuda")
    return torch.as_tensor(rng.randn(rollouts, T, N, 2).astype(np.float32), device="cuda")


def _assert_identical(a_p, e_p, a_s, e_s, it):
    for k in BUF_KEYS:
        got, ref = getattr(a_p.rollout_buffer, k).cpu().numpy(), getattr(a_s.rollout_buffer, k).cpu().numpy()
        assert np.array_equal(got, ref), (it, k, np.abs(got - ref).max())
    for name in ("obs_rms", "ret_rms", "cost_rms"):
        rp, rs = getattr(e_p, name), getattr(e_s, name)
        assert np.array_equal(np.asarray(rp.mean), np.asarray(rs.mean)) and np.array_equal(np.asarray(rp.var), np.asarray(rs.var)), name
        assert rp.count == rs.count, name
    assert torch.equal(e_p.ret, e_s.ret) and torch.equal(e_p.cost_ret, e_s.cost_ret)
    assert torch.equal(a_p._last_obs, a_s._last_obs) and torch.equal(a_p._ag["last_dones"], a_s._ag["last_dones"])
    for k in ("s", "t_ep", "step_count"):
        assert torch.equal(getattr(e_p.unwrapped, k), getattr(e_s.unwrapped, k)), k
    for k in ("raw_rew", "raw_cost", "dones", "last_v_r", "last_v_c"):
        assert torch.equal(a_p._ag[k], a_s._ag[k]), k


# (kind, envs, T, rollout_kernel) -> what icrl_rollout_collect must have launched
_FORMS = [
    ("c2b", 16, 64, "auto", dict(route="multi", launches=1)),
    ("dd2b", 16, 64, "auto", dict(route="per-step", launches=128)),      # a Categorical policy: not the multi-env kernel's
    ("dd2b", 16, 64, "wide", dict(route="wide", launches=1)),
    ("c2b", 100, 32, "auto", dict(route="wide", wgs=100, launches=1)),
    ("dd2b", 100, 32, "auto", dict(route="wide", wgs=100, launches=1)),
    ("c2b", 4, 64, "auto", dict(route="per-step", launches=128)),
    ("dd2b", 4, 64, "auto", dict(route="per-step", launches=128)),
]


@pytest.mark.parametrize("kind,N,T,kernel,route", [pytest.param(*f, id="-".join(map(str, f[:4]))) for f in _FORMS])
def test_launch_forms_equal_per_step_launches(kind, N, T, kernel, route):
    (a_p, e_p), (a_s, e_s) = _pair(N, T, 13, kind)
    assert a_p._fused_chain() is not None and a_p._fused_rollout_ok("cost", T, a_p.rollout_buffer)
    a_s.rollout_kernel, a_p.rollout_kernel = "steps", kernel
    noise = _noise(kind, 2, T, N)
    a_p._setup_learn(2 * N * T); a_s._setup_learn(2 * N * T)
    for env in (e_p, e_s):
        env.unwrapped.t_ep.fill_(200 - T // 2)           # every env crosses its time limit inside the first rollout
    for it in range(2):
        a_p.collect_rollouts(e_p, None, a_p.rollout_buffer, T, "cost", noise=noise[it])
        got = routes.check_rollout(route, f"{kind} {N} {T} {kernel}")
        assert got["pick"] & routes.PICK_ANALYTIC
        a_s.collect_rollouts(e_s, None, a_s.rollout_buffer, T, "cost", noise=noise[it])
        routes.check_rollout(dict(route="per-step", launches=2 * T), "steps")
        a_p.check_rollout_status()
        _assert_identical(a_p, e_p, a_s, e_s, it)
        rb = a_p.rollout_buffer
        assert rb.dones.sum().item() == (N if it == 0 else 0)
        o, o2, a, d = (x.cpu().numpy() for x in (rb.orig_observations, rb.new_orig_observations, rb.actions, rb.dones))
        a = a.reshape(T, N, -1)
        # (dones[t] flags that the observation of row t starts an episode: row t - 1 then holds the reset, not the step's own position)
        ended = np.concatenate([d.reshape(T, N)[1:], a_p._ag["last_dones"].cpu().numpy().reshape(1, N)]).astype(bool)
        stayed = (o2[..., :2] == o[..., :2]).all(axis=-1) & ~ended
        if kind == "dd2b":
            assert (stayed & (o[..., 0] == 3.5) & (a[..., 0] == RIGHT)).any(), "no move into the water's edge was rejected"
            assert (stayed & (o[..., 1] == 0.0) & (a[..., 0] == DOWN)).any() or (stayed & (o[..., 0] == 0.0) & (a[..., 0] == LEFT)).any(), "no wall"
            assert set(np.unique(a)) == {0.0, 1.0, 2.0, 3.0}
        else:
            assert stayed.any() and (~stayed).any()      # rejected moves and accepted ones
        assert it == 1 or rb.orig_costs.cpu().numpy().std() > 0      # (the first rollout starts at x = 0 and passes x = 1)


# ---- 3. sampling and evaluation episodes against the per-step episode loop -------------------------------------------------------
@pytest.mark.parametrize("env_id,kind", [("CDD2B-v0", "dd2b"), ("CC2B-v0", "c2b")])
def test_episodes_vs_per_step_loop(env_id, kind):
    from icrl_amd import utils
    from icrl_amd.ppo_lag import PPOLagrangian
    from icrl_amd.true_constraint_net import AnalyticCost
    n_ep = 3
    train_env = utils.make_train_env(env_id, None, True, 5, 4, cost_info_str="cost", reward_gamma=0.99, cost_gamma=0.99)
    train_env.set_cost_function(AnalyticCost.null())
    agent = PPOLagrangian("TwoCriticsMlpPolicy", train_env, n_steps=32, seed=5)
    _policy_state(agent, kind)
    rng = np.random.RandomState(3)
    noise = rng.rand(n_ep * 200).astype(np.float32) if kind == "dd2b" else rng.randn(n_ep * 200, 2).astype(np.float32)
    outs = []
    for which in ("kernel", "sequential", "stepped"):
        eenv = utils.make_eval_env(env_id, False, seed=5)
        assert eenv.unwrapped.kind == IDS[env_id] and not eenv.unwrapped.wall_terminate
        if which == "stepped":
            run = utils.SteppedEpisodeRun(agent, eenv, n_ep, False, noise)
        else:
            run = utils._run_episodes(agent, eenv, n_ep, False, noise, parallel=which == "kernel", chain=True)
            assert isinstance(run, utils.EpisodeRun) and run.fixed_len and not run.chain_ok()      # the chained sampler refuses these forms
            assert run.n_streams == (n_ep if which == "kernel" else 1) and run.passes == 1
        oo, o, a, r, l = utils.sample_result(run)
        outs.append((oo.cpu().numpy(), o.cpu().numpy(), a.cpu().numpy(), np.asarray(r), np.asarray(l)))
        assert list(l) == [200] * n_ep
        assert int(eenv.unwrapped.step_count[0].item()) == 200 * n_ep
    for name, other in (("sequential", outs[1]), ("stepped", outs[2])):
        for i, what in enumerate(("orig_obs", "obs", "actions", "ep_rewards", "lengths")):
            assert np.array_equal(outs[0][i], other[i]), (name, what)
    oo = outs[0][0]
    assert (np.diff(oo[:200, :2], axis=0) == 0).all(axis=1).any() and (oo[199::200, :2] == 0).all()      # rejected moves; rows of an end: the start
    if env_id == "CDD2B-v0":
        assert not ((oo[:, 0] > 4) & (oo[:, 0] < 8) & (oo[:, 1] > 5) & (oo[:, 1] < 6)).any()      # the constrained bridge is closed
    er, el = utils.evaluate_policy(agent, utils.make_eval_env(env_id, False, seed=5), n_ep, deterministic=False, return_episode_rewards=True, noise=noise)
    assert list(el) == [200] * n_ep and np.array_equal(np.asarray(er), outs[2][3])


# ---- 4. cpg end to end -----------------------------------------------------------------------------------------------------------
def _cpg_cfg(seed, tei, eei, nt, n_steps, timesteps, extra=()):
    from icrl_amd.cpg import build_parser
    argv = ["cpg", "-p", "ICRL-FE2", "--group", "Bridges", "-tei", tei, "-eei", eei, "-t", str(timesteps), "-nt", str(nt), "--n_steps", str(n_steps),
            "-s", str(seed), "-v", "0", *extra]
    cfg = vars(build_parser().parse_args(argv))
    cfg.update(rank=0, world_size=1)
    return types.SimpleNamespace(**cfg)


def _count_stepped(monkeypatch):
    from icrl_amd.ppo_lag import PPOLagrangian
    calls, inner = [], PPOLagrangian._collect_rollouts_stepped

    def counted(self, *a, **k):
        calls.append(routes.rollout()["route"])
        return inner(self, *a, **k)
    monkeypatch.setattr(PPOLagrangian, "_collect_rollouts_stepped", counted)
    return calls


def _record_routes(monkeypatch):
    from icrl_amd.ppo_lag import PPOLagrangian
    seen, inner = [], PPOLagrangian.collect_rollouts

    def recorded(self, *a, **k):
        out = inner(self, *a, **k)
        seen.append(routes.rollout())
        return out
    monkeypatch.setattr(PPOLagrangian, "collect_rollouts", recorded)
    return seen


@pytest.mark.parametrize("tei,eei,route", [("C2B-v0", "CC2B-v0", dict(route="multi", launches=1)),
                                           ("DD2B-v0", "CDD2B-v0", dict(route="per-step", launches=128))])
def test_cpg_null_cost_runs_in_the_fused_launches(monkeypatch, tei, eei, route):
    """`cpg -tei DD2B-v0 -eei CDD2B-v0 --use_null_cost -nt 16 --n_steps 64 -t 2048` and the same over C2B / CC2B: no rollout takes the
    Python per-step loop; the continuous one is ONE launch of the multi-env kernel per rollout, the discrete one the library's
    per-step launches (the multi-env kernel takes no Categorical policy)."""
    from icrl_amd import cpg as C, logger
    stepped, seen = _count_stepped(monkeypatch), _record_routes(monkeypatch)
    model, hist = C.cpg(_cpg_cfg(2, tei, eei, 16, 64, 2048, ("--use_null_cost",)), log=None)
    assert model.num_timesteps == 2048 and len(hist) == 2 and not stepped and len(seen) == 2
    for got in seen:
        for k, v in route.items():
            assert got[k] == v, (k, got)
        assert got["pick"] & routes.PICK_ANALYTIC
    assert model.env.venv.analytic_cost().name == "null_cost" and model.env.unwrapped.kind == IDS[tei]
    lg = dict(logger.Logger.CURRENT.name_to_value)
    bad = {k: v for k, v in lg.items() if isinstance(v, (int, float, np.floating)) and not np.isfinite(v)}
    assert not bad and len(lg) > 10, bad
    assert not model.rollout_buffer.orig_costs.any().item()
    o = model.rollout_buffer.orig_observations.cpu().numpy()
    assert o[..., :2].min() >= 0 and o[..., :2].max() <= 20 and o[..., 0].max() > 0.5      # inside the field, and the agent moved


def test_cpg_against_the_bridge_cost_takes_the_per_step_loop(monkeypatch):
    """`cpg -tei CDD2B-v0 -eei CDD2B-v0 -nt 4 --n_steps 32 -t 256`: the ground-truth cost is BridgesCost, a plain callable."""
    from icrl_amd import cpg as C
    from icrl_amd.true_constraint_net import BridgesCost
    stepped = _count_stepped(monkeypatch)
    model, hist = C.cpg(_cpg_cfg(1, "CDD2B-v0", "CDD2B-v0", 4, 32, 256), log=None)
    cost = model.env.venv.cost_function
    assert isinstance(cost, BridgesCost) and model.env.venv.analytic_cost() is None and model.env.venv.constraint_net() is None
    assert len(stepped) == 2 and model.num_timesteps == 256 and len(hist) == 2
    rb = model.rollout_buffer
    want = cost(rb.orig_observations.cpu().numpy(), rb.actions.cpu().numpy())
    assert np.array_equal(rb.orig_costs.cpu().numpy().reshape(want.shape), want.astype(np.float32))
    assert np.isfinite(model.dual.nu().item())


def test_seed_batch_equals_solo_runs():
    """a two-seed `--seeds` batch on DD2B-v0 with --use_null_cost equals the runs alone, bit for bit (tests/test_cpg_seed_batch_gpu.py)."""
    from icrl_amd import cpg as C
    from icrl_amd.seed_batch import run_cpg_seed_batch
    from icrl_amd.streams import PrivateStreams
    seeds = [0, 1]
    mk = lambda sd: _cpg_cfg(sd, "DD2B-v0", "CDD2B-v0", 4, 64, 256, ("--use_null_cost", "-ne", "2", "--eval_every_rollouts", "1"))

    def snap(model, history):
        pol, env, rb = model.policy, model.env, model.rollout_buffer
        return dict(params=pol.params.cpu().numpy().copy(), exp_avg_sq=pol.exp_avg_sq.cpu().numpy().copy(), obs_mean=np.asarray(env.obs_rms.mean).copy(),
                    ret_var=float(env.ret_rms.var), nu=float(model.dual.nu().item()), rewards=rb.rewards.cpu().numpy().copy(),
                    actions=rb.actions.cpu().numpy().copy(), obs=rb.orig_observations.cpu().numpy().copy(), history=[dict(h) for h in history])

    solo = []
    for sd in seeds:
        cfg = mk(sd)
        cfg.streams, cfg.eval_noise_from_streams = PrivateStreams(sd), True
        model, cb, learn_cost, hist = C.setup(cfg, log=None)
        model.learn(total_timesteps=int(cfg.timesteps), cost_function=learn_cost, callback=cb)
        solo.append(snap(model, hist.history))
    out = run_cpg_seed_batch([mk(sd) for sd in seeds])
    batch_route = routes.rollout()
    assert len(out) == 2 and solo[0]["params"].tobytes() != solo[1]["params"].tobytes()
    for sd, (model, history), want in zip(seeds, out, solo):
        got = snap(model, history)
        assert model.num_timesteps == 256
        for k in ("params", "exp_avg_sq", "obs_mean", "rewards", "actions", "obs"):
            assert np.array_equal(got[k], want[k]), (sd, k)
        assert got["ret_var"] == want["ret_var"] and got["nu"] == want["nu"], sd
        assert len(got["history"]) == len(want["history"]) == 1 and got["history"] == want["history"], sd
        assert got["obs"][..., :2].max() > 0.5      # the agent moved
    print("[route] the batch's last rollout:", batch_route)
