"""GPU: seed batches of cpg runs (icrl_amd/seed_batch.py: CpgSeedBatch) — the batched rollout kernels with a per-run analytic cost
(icrl_rollout_collect_batch_cost) against the single-run launches, bit for bit; whole batched cpg runs (rollouts, updates, evaluations
and callbacks of all runs in lock-step) against the same runs alone; the refusals."""
import os
import types

import numpy as np
import pytest
import torch

from helpers import routes

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

_BUF_KEYS = ("observations", "orig_observations", "new_observations", "new_orig_observations", "actions", "rewards", "costs",
             "orig_costs", "dones", "log_probs", "reward_values", "cost_values", "reward_advantages", "cost_advantages",
             "reward_returns", "cost_returns")


def _cost(name):
    from icrl_amd.true_constraint_net import AnalyticCost
    return {"wall": lambda: AnalyticCost.wall_behind(0.0), "torque": lambda: AnalyticCost.torque(0.5),
            "both": lambda: AnalyticCost.wall_behind_and_infront(-0.25, 0.25), "null": AnalyticCost.null,
            "action": lambda: AnalyticCost.action_equals(1)}[name]()


def _twin_chains(kind, N, T, costs, mon):
    """per run two agents over twin chains VecNormalizeWithCost -> VecCostWrapper(AnalyticCost) -> HipSynthVecEnv; the runs differ in
    the env seed, the policy and (where `costs` does) the cost descriptor."""
    from icrl_amd.ppo_lag import PPOLagrangian
    from icrl_amd.vec_env import HipSynthVecEnv, VecCostWrapper, VecNormalizeWithCost
    norm = dict(norm_obs=False, norm_reward=False) if kind == "clgw" else {}
    runs = []
    for r, cost in enumerate(costs):
        seed = 13 + 7 * r
        pair = []
        for _ in range(2):
            torch.manual_seed(seed)
            env = VecNormalizeWithCost(VecCostWrapper(HipSynthVecEnv(N, kind, seed)), **norm)
            env.set_cost_function(_cost(cost))
            pair.append((PPOLagrangian("TwoCriticsMlpPolicy", env, n_steps=T, seed=seed, episode_stats=bool(mon)), env))
        pair[1][0].policy.load_state_dict(pair[0][0].policy.state_dict())
        runs.append(pair)
    return runs


def _noise(kind, S, rollouts, T, N, seed=8, scale=0.5):
    """(scaled so that |action| > 0.5 happens in some rows and not in others: the policy's initial std is 1)"""
    rng = np.random.RandomState(seed)
    if kind == "clgw":
        return torch.as_tensor(rng.rand(S, rollouts, T, N).astype(np.float32), device="cuda")
    ad = 6 if kind == "hc" else 8
    return torch.as_tensor((scale * rng.randn(S, rollouts, T, N, ad)).astype(np.float32), device="cuda")


def _assert_identical(a_p, e_p, a_s, e_s, tag):
    for k in _BUF_KEYS:
        got, ref = getattr(a_p.rollout_buffer, k).cpu().numpy(), getattr(a_s.rollout_buffer, k).cpu().numpy()
        assert np.array_equal(got, ref), (tag, k, np.abs(got - ref).max())
    for name in ("obs_rms", "ret_rms", "cost_rms"):
        rp, rs = getattr(e_p, name), getattr(e_s, name)
        assert np.array_equal(np.asarray(rp.mean), np.asarray(rs.mean)) and np.array_equal(np.asarray(rp.var), np.asarray(rs.var)), (tag, name)
        assert rp.count == rs.count, (tag, name)
    assert torch.equal(e_p.ret, e_s.ret) and torch.equal(e_p.cost_ret, e_s.cost_ret), tag
    assert torch.equal(a_p._last_obs, a_s._last_obs) and torch.equal(a_p._ag["last_dones"], a_s._ag["last_dones"]), tag
    assert torch.equal(e_p.unwrapped.s, e_s.unwrapped.s) and torch.equal(e_p.unwrapped.t_ep, e_s.unwrapped.t_ep), tag
    for k in ("raw_cost", "act_clipped", "last_v_r", "last_v_c"):
        assert torch.equal(a_p._ag[k], a_s._ag[k]), (tag, k)
    if a_p._mon is not None:
        for k in ("raw_rewards", "ep_ret", "ep_len", "win_state"):
            assert torch.equal(a_p._mon[k], a_s._mon[k]), (tag, k)


def _numpy_cost(cost, rb, env, T, N):
    """the closed forms on the rollout's own buffer (tests/test_cost_fn_gpu.py: _numpy_cost)"""
    if cost == "wall":
        return (rb.orig_observations.cpu().numpy()[..., 0] <= 0.0).astype(np.float32)
    if cost == "both":
        col = rb.orig_observations.cpu().numpy()[..., 0]
        return (col <= -0.25).astype(np.float32) + (col >= 0.25).astype(np.float32)
    if cost == "torque":
        acs = np.clip(rb.actions.cpu().numpy(), env.action_space.low, env.action_space.high)
        return np.any(np.abs(acs) > np.float32(0.5), axis=-1).astype(np.float32)
    if cost == "action":
        return (rb.actions.cpu().numpy().reshape(T, N) == 1).astype(np.float32)
    return np.zeros((T, N), np.float32)


def _batched_rollout(agents, noises):
    """the agents' rollouts through ONE icrl_rollout_collect_batch_cost call (called directly: no per-run fall-back can stand in)."""
    from icrl_amd import _lib
    from icrl_amd.structs import MonitorT, RolloutJobT, addr, p
    jobs = [a._rollout_begin(None, a.rollout_buffer, a.n_steps, nz) for a, nz in zip(agents, noises)]
    arr = (RolloutJobT * len(jobs))(*[RolloutJobT(addr(j["env"]), addr(j["nm"]), addr(j["pol"]), addr(j["cn"]), addr(j["buf"]), addr(j["ag"]), p(j["noise"]))
                                     for j in jobs])
    a0 = agents[0]
    marr = None if a0._mon is None else (MonitorT * len(agents))(*[a._mon["struct"] for a in agents])
    ws = torch.empty(2 * len(jobs) * _lib.BATCH_ARGS_BYTES, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().icrl_rollout_collect_batch_cost(len(jobs), arr, marr, p(a0._alow), p(a0._ahigh), float(a0.reward_gamma), float(a0.reward_gae_lambda),
                                                          float(a0.cost_gamma), float(a0.cost_gae_lambda), 1, p(ws), ws.numel(), _lib.current_stream()),
               "icrl_rollout_collect_batch_cost")
    for a, j in zip(agents, jobs):
        a._rollout_end(j, a.env, None, a.rollout_buffer, a.n_steps)
    torch.cuda.synchronize()


# ---- 1. batched analytic rollouts against the single-run launches, bit for bit ------------------------------------------------------------
_SHAPES = [("hc", 7, 33, ("wall", "torque", "both")), ("ant", 16, 6, ("wall", "torque")), ("ant", 128, 6, ("wall", "torque", "null")),
           ("hc", 132, 24, ("torque", "wall")), ("clgw", 5, 40, ("action", "null", "action")),
           ("ant", 12, 6, ("torque", "wall")), ("hc", 80, 12, ("wall", "torque"))]


# (kind, envs) -> (the words of a `few` batch, of any other batch; None: no other form serves the shape).  minw: the MINW the
# one-workgroup-per-env kernel is instantiated with (the docstring's last template argument)
_PB1, _PB2 = dict(route="persistent-batch", minw=1, envs_per_wg=1), dict(route="persistent-batch", minw=2, envs_per_wg=1)
_BATCH_ROUTES = {("hc", 7): (_PB1, None), ("ant", 16): (_PB1, None), ("ant", 128): (_PB1, dict(route="multi-batch", envs_per_wg=4, wgs=32)),
                 ("hc", 132): (None, dict(route="multi-batch", envs_per_wg=8, wgs=17)), ("clgw", 5): (_PB1, _PB2), ("ant", 12): (_PB1, None),
                 ("hc", 80): (_PB2, dict(route="multi-batch", envs_per_wg=8, wgs=10))}


@pytest.mark.parametrize("mon", [False, True], ids=["plain", "mon"])
@pytest.mark.parametrize("kind,N,T,costs", _SHAPES, ids=[f"{k}-{n}x{t}-S{len(c)}" for k, n, t, c in _SHAPES])
def test_batched_analytic_rollouts_equal_single_run_ones(kind, N, T, costs, mon):
    """Two consecutive rollouts of S runs, run by run through icrl_rollout_collect_ex[_mon] and through ONE icrl_rollout_collect_batch_cost
    call on twin chains: all 16 buffer planes, the running moments, returns, last observations / dones, env state and the agent carry are
    equal bit for bit, and the first rollout's costs equal the numpy closed form on the rollout's own buffer.

    Kernels the batched call launches on an MI355X (256 CUs), as the dispatch of rollout_collect_batch_impl (csrc/rollout_collect.hip) selects them
    (`mon` adds the template argument MON = true); the selection is asserted behind every batched call from the library's own record of it
    (icrl_debug_last_route: _BATCH_ROUTES, with `few` = runs x envs within the device's compute units).
      hc-7x33-S3     rollout_persistent_batch_analytic_kernel<2, true, 1>     one workgroup per env, OCT 2, granule exchange, ragged count
      ant-16x6-S2    rollout_persistent_batch_analytic_kernel<8, false, 1>    one workgroup per env, OCT 8 (16 x 230 words: record exchange off)
      ant-128x6-S3   rollout_multi_batch_analytic_kernel<8, 4>                384 envs' worth of workgroups > CUs: 4 envs per workgroup, G = 32
      hc-132x24-S2   rollout_multi_batch_analytic_kernel<2, 8>                above 128 envs: multi-env form at OCT 2, G = 17
      clgw-5x40-S3   rollout_persistent_batch_analytic_kernel<2, true, 1>     discrete actions, action_equals / null / action_equals
      ant-12x6-S2    rollout_persistent_batch_analytic_kernel<8, true, 1>     OCT 8 with the record exchange (12 x 230 words <= 3072)
      hc-80x12-S2    rollout_persistent_batch_analytic_kernel<2, false, 2>    OCT 2 without it (80 x 40 words > 3072)
    """
    S = len(costs)
    runs = _twin_chains(kind, N, T, costs, mon)
    noise = _noise(kind, S, 2, T, N)
    limit = {"hc": 1000, "ant": 500}.get(kind)
    for pair in runs:
        for a, e in pair:
            a._setup_learn(2 * N * T)
            if limit is not None:
                e.unwrapped.t_ep.fill_(limit - T // 2)           # every env crosses its time limit inside the first rollout
    fired = []
    for it in range(2):
        for r, ((a_s, e_s), _) in enumerate(runs):
            a_s.collect_rollouts(e_s, None, a_s.rollout_buffer, T, "cost", noise=noise[r, it])
            a_s.check_rollout_status()
        _batched_rollout([pair[1][0] for pair in runs], [noise[r, it] for r in range(S)])
        few = S * N <= torch.cuda.get_device_properties(0).multi_processor_count and N <= 128
        want = _BATCH_ROUTES[kind, N]
        want = dict(want[0] if few or want[1] is None else want[1], n_runs=S, launches=1)
        got_route = routes.check_rollout(want, f"{kind} {N} x {S}")
        L = routes
        assert got_route["pick"] & L.PICK_ANALYTIC and bool(got_route["pick"] & L.PICK_MON) == mon and bool(got_route["pick"] & L.PICK_SMALL) == (kind != "ant")
        if got_route["route"] == "persistent-batch":
            assert bool(got_route["pick"] & L.PICK_GRAN) == (N * (2 * {"hc": 18, "ant": 113, "clgw": 1}[kind] + 4) <= 3072)
        for r, ((a_s, e_s), (a_b, e_b)) in enumerate(runs):
            a_b.check_rollout_status()
            _assert_identical(a_b, e_b, a_s, e_s, (it, r))
            if it == 0:
                got = a_b.rollout_buffer.orig_costs.cpu().numpy()
                assert np.array_equal(got, _numpy_cost(costs[r], a_b.rollout_buffer, e_b, T, N)), r
                fired.append((costs[r], float(got.mean())))
                if costs[r] == "null":
                    assert got.max() == 0.0
    # the closed forms were exercised on both sides of their thresholds: some rows fire, not all
    live = [m for c, m in fired if c != "null"]
    assert 0.0 < np.mean(live) and min(live) < (2.0 if "both" in costs else 1.0), fired
    # the runs of the batch really are different runs
    firsts = [pair[1][0].rollout_buffer.rewards.cpu().numpy() for pair in runs]
    assert all(not np.array_equal(firsts[0], f) for f in firsts[1:])


def test_c_abi_refuses_a_batch_that_mixes_a_constraint_net_with_an_analytic_cost():
    from icrl_amd import _lib
    from icrl_amd.constraint_net import ConstraintNet
    from icrl_amd.structs import RolloutJobT, addr, p
    (a0, e0), (a1, e1) = _twin_chains("hc", 4, 8, ("wall",), False)[0]
    lo = -np.ones(6, np.float32)
    cn = ConstraintNet(18, 6, [20], None, lambda x: 0.05, None, None, False, 0.5, clip_obs=20, action_low=lo, action_high=-lo)
    e1.set_cost_function(cn.cost_function)
    agents = [a0, a1]
    for a in agents:
        a._setup_learn(32)
    jobs = [a._rollout_begin(None, a.rollout_buffer, a.n_steps, None) for a in agents]
    arr = (RolloutJobT * 2)(*[RolloutJobT(addr(j["env"]), addr(j["nm"]), addr(j["pol"]), addr(j["cn"]), addr(j["buf"]), addr(j["ag"]), p(j["noise"])) for j in jobs])
    ws = torch.empty(4 * _lib.BATCH_ARGS_BYTES, dtype=torch.uint8, device="cuda")
    before = a0.rollout_buffer.rewards.clone()
    with pytest.raises(ValueError, match="every run carries an analytic descriptor, or none does"):
        _lib.check(_lib.lib().icrl_rollout_collect_batch_cost(2, arr, None, p(a0._alow), p(a0._ahigh), 0.99, 0.95, 0.99, 0.95, 1, p(ws), ws.numel(),
                                                              _lib.current_stream()), "icrl_rollout_collect_batch_cost")
    torch.cuda.synchronize()
    assert torch.equal(a0.rollout_buffer.rewards, before)          # nothing was launched


# ---- 2. batched cpg against solo cpg ------------------------------------------------------------------------------------------------------
_HC = ("-tei", "HCWithPos-v0", "-eei", "HCWithPosTest-v0", "-nt", "8", "-ns", "64", "-t", str(3 * 8 * 64))
_ANT = ("-tei", "AntWallBroken-v0", "-eei", "AntWallBrokenTest-v0", "-nt", "16", "-ns", "32", "-t", str(2 * 16 * 32),
        "-cp", os.path.join(HERE, "golden/cn_antbroken.npz"))
_HIST_KEYS = ("nu", "rollout/adjusted_reward", "eval/true_cost", "eval/mean_reward", "eval/best_mean_reward")


def _cfg(seed, shape=_HC, extra=(), save_dir=None):
    from icrl_amd.cpg import build_parser
    argv = ["cpg", *shape, "-ne", "4", "--eval_every_rollouts", "1", "-s", str(seed), "-v", "0", *extra]
    cfg = vars(build_parser().parse_args(argv))
    cfg.update(rank=0, world_size=1, save_dir=save_dir)
    if save_dir:
        os.makedirs(save_dir, exist_ok=True)
    return types.SimpleNamespace(**cfg)


def _solo(cfg):
    """the run alone through cpg.setup + learn, with the private streams and the evaluation-noise opt-in a batch gives it."""
    from icrl_amd import cpg as C
    from icrl_amd.streams import PrivateStreams
    cfg.streams = PrivateStreams(cfg.seed)
    cfg.eval_noise_from_streams = True
    model, cb, learn_cost, hist = C.setup(cfg, log=None)
    model.learn(total_timesteps=int(cfg.timesteps), cost_function=learn_cost, callback=cb)
    return model, hist.history


def _snapshot(model, history):
    pol, env, rb = model.policy, model.env, model.rollout_buffer
    return dict(params=pol.params.cpu().numpy().copy(), exp_avg_sq=pol.exp_avg_sq.cpu().numpy().copy(), obs_mean=np.asarray(env.obs_rms.mean).copy(),
                ret_var=float(env.ret_rms.var), cost_rms=(float(env.cost_rms.mean), float(env.cost_rms.var), float(env.cost_rms.count)),
                nu=float(model.dual.nu().item()), rewards=rb.rewards.cpu().numpy().copy(), costs=rb.costs.cpu().numpy().copy(),
                history=[dict(h) for h in history])


def _assert_same_run(got, want, tag):
    for k in ("params", "exp_avg_sq", "obs_mean", "rewards", "costs"):
        assert np.array_equal(got[k], want[k]), (tag, k)
    assert got["ret_var"] == want["ret_var"] and got["cost_rms"] == want["cost_rms"] and got["nu"] == want["nu"], tag
    assert len(got["history"]) == len(want["history"]) > 0, tag
    for a, b in zip(got["history"], want["history"]):
        assert a.keys() == b.keys(), (tag, a.keys(), b.keys())
        assert all(k in a for k in _HIST_KEYS), (tag, a.keys())
        for k in a:
            assert a[k] == b[k], (tag, k, a[k], b[k])


_CASES = [(_HC, ()), (_HC, ("--use_null_cost",)), (_HC, ("--use_pid",)), (_HC, ("--episode_stats",)), (_ANT, ())]


@pytest.mark.parametrize("shape,extra", _CASES, ids=["ground_truth", "null_cost", "pid", "episode_stats", "ant_transfer"])
def test_batched_cpg_equals_solo_cpg(shape, extra):
    """seeds 0..3, each alone and then all four in one batch: parameters, Adam second moments, the running moments, nu, the last buffer's
    rewards and costs and every history record are equal, bit for bit and value for value.  HCWithPos 8 envs x 64 steps x 3 rollouts
    against the ground-truth wall cost, the null cost, with the PID dual and with episode statistics; AntWallBroken 16 x 32 x 2 against
    the committed constraint net (the constraint-net batch path under the same driver).  Evaluation after every rollout."""
    from icrl_amd.seed_batch import run_cpg_seed_batch
    seeds = [0, 1, 2, 3]
    solo = [_snapshot(*_solo(_cfg(sd, shape, extra))) for sd in seeds]
    out = run_cpg_seed_batch([_cfg(sd, shape, extra) for sd in seeds])
    assert len(out) == len(seeds)
    # the batch's last rollout was ONE launch for the four runs (4 x 8 / 4 x 16 envs: one workgroup per env, the whole register file), and
    # so was its last update at HalfCheetah widths (up to 16 runs: the kernel a run alone gets); at AntWall widths the updates go run
    # after run through the single-run call (SeedBatch.per_run_wide_updates: four workgroups per network, minibatches of 64 rows)
    got = routes.check_rollout(dict(route="persistent-batch", n_runs=len(seeds), minw=1, launches=1, wgs=16 if shape is _ANT else 8), "cpg batch")
    assert bool(got["pick"] & routes.PICK_ANALYTIC) == (shape is _HC) and bool(got["pick"] & routes.PICK_MON) == ("--episode_stats" in extra)
    routes.check_update(dict(kind=6, n_runs=1, wgs_per_network=4) if shape is _ANT else dict(kind=5, n_runs=len(seeds), wgs_per_network=4), "cpg batch")
    assert len({s["params"].tobytes() for s in solo}) == len(seeds)            # the runs really are different runs
    for sd, (model, history), want in zip(seeds, out, solo):
        assert model.num_timesteps == int(_cfg(sd, shape, extra).timesteps)
        _assert_same_run(_snapshot(model, history), want, sd)
    if "--use_null_cost" in extra:
        assert all(float(m.rollout_buffer.orig_costs.abs().max().item()) == 0.0 for m, _ in out)
    elif shape is _HC:
        # the ground-truth cost of HCWithPos is the wall at x = -3 (true_constraint_net.TRUE_COSTS), which 192 steps from the start do not
        # reach: what can be checked is that every run carries that cost and that its buffer holds the closed form on its own observations
        for m, _ in out:
            cost = m.env.venv.analytic_cost()
            assert cost is not None and cost.name == "wall_behind"
            rb = m.rollout_buffer
            assert np.array_equal(rb.orig_costs.cpu().numpy(), (rb.orig_observations.cpu().numpy()[..., 0] <= -3.0).astype(np.float32))


def test_batched_cpg_saves_per_run(tmp_path):
    from icrl_amd import cpg as C
    from icrl_amd.ppo_lag import PPOLagrangian
    from icrl_amd.seed_batch import run_cpg_seed_batch
    seeds = [0, 1]
    solo_dir = str(tmp_path / "solo")
    model, _ = _solo(_cfg(1, save_dir=solo_dir))
    base = vars(_cfg(0, save_dir=str(tmp_path / "batch")))
    base["seeds"] = seeds
    out = run_cpg_seed_batch(C.seed_configs(base))
    for sd in seeds:
        d = str(tmp_path / "batch" / f"seed_{sd}")
        for name in ("best_model.zip", "train_env_stats.pkl", "final_model_policy.pth", "config.json"):
            assert os.path.isfile(os.path.join(d, name)), (sd, name)
    assert os.path.isfile(os.path.join(solo_dir, "best_model.zip"))
    got = PPOLagrangian.load(os.path.join(str(tmp_path / "batch" / "seed_1"), "best_model"))
    want = PPOLagrangian.load(os.path.join(solo_dir, "best_model"))
    assert torch.equal(got.policy.params, want.policy.params)
    final = torch.load(os.path.join(str(tmp_path / "batch" / "seed_1"), "final_model_policy.pth"))
    for k, v in out[1][0].policy.state_dict().items():
        assert torch.equal(final[k].cpu(), v.cpu()), k
    assert torch.equal(out[1][0].policy.params, model.policy.params)


# ---- 3. refusals --------------------------------------------------------------------------------------------------------------------------
def test_batch_refuses_what_it_cannot_run_in_lock_step(monkeypatch):
    from icrl_amd.seed_batch import CpgSeedBatch
    with pytest.raises(ValueError, match="num_threads"):
        CpgSeedBatch([_cfg(0), _cfg(1, ("-tei", "HCWithPos-v0", "-eei", "HCWithPosTest-v0", "-nt", "4", "-ns", "64", "-t", str(3 * 8 * 64)))])
    with pytest.raises(ValueError, match="use_null_cost"):
        CpgSeedBatch([_cfg(0), _cfg(1, extra=("--use_null_cost",))])
    with pytest.raises(ValueError, match="load_gail"):
        CpgSeedBatch([_cfg(0, extra=("--load_gail", "-cp", "unused.pt")), _cfg(1, extra=("--load_gail", "-cp", "unused.pt"))])
    import tests.helpers.host_envs  # noqa: F401  (registers the Host* ids)
    with pytest.raises(ValueError, match="not device-resident envs"):
        CpgSeedBatch([_cfg(s, ("-tei", "HostHCWithPos-v0", "-eei", "HostHCWithPosTest-v0", "-nt", "8", "-ns", "64", "-t", "1024")) for s in (0, 1)])
    with pytest.raises(ValueError, match="generic-shape path"):
        CpgSeedBatch([_cfg(s, extra=("-pl", "128", "128")) for s in (0, 1)])
    with pytest.raises(ValueError, match="-cis None"):
        CpgSeedBatch([_cfg(s, extra=("-cis", "None")) for s in (0, 1)])
    monkeypatch.setenv("ICRL_ANALYTIC_COST_STEPPED", "1")
    with pytest.raises(ValueError, match="ICRL_ANALYTIC_COST_STEPPED"):
        CpgSeedBatch([_cfg(0), _cfg(1)])
