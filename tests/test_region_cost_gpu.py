"""GPU: region costs (true_constraint_net.RegionCost / icrl_cost_region_t) — the rows kernel against the one-row-at-a-time evaluator of
tests/helpers/region_cost_cases.py bit for bit; a RegionCost written as a wall / two walls / a torque limit against the AnalyticCost in
every launch form, all planes identical; general specs in every fused form against the per-step launches and the per-step cost against
the evaluator on the state cloned before the step; the fused launch against the per-step loop under ICRL_REGION_COST_STEPPED=1; host
envs; `cpg --cost_spec` and `icrl --cost_spec` end to end."""
import json
import os
import types

import numpy as np
import pytest
import torch

import tests.helpers.host_envs  # noqa: F401  (registers the Host* ids)
from helpers import region_cost_cases as RC
from helpers import routes

pytestmark = pytest.mark.gpu

_BUF_KEYS = ("observations", "orig_observations", "new_observations", "new_orig_observations", "actions", "rewards", "costs",
             "orig_costs", "dones", "log_probs", "reward_values", "cost_values", "reward_advantages", "cost_advantages",
             "reward_returns", "cost_returns")
_DIMS = {"hc": (18, 6), "ant": (113, 8)}


def _pick_region():
    from icrl_amd import _lib
    return _lib.PICK_REGION


def _agents(N, T, seed, kind, costs, **norm):
    """one agent per cost object over twin device chains VecNormalizeWithCost -> VecCostWrapper(cost) -> HipSynthVecEnv, same policy"""
    from icrl_amd.ppo_lag import PPOLagrangian
    from icrl_amd.vec_env import HipSynthVecEnv, VecCostWrapper, VecNormalizeWithCost
    out = []
    for cost in costs:
        torch.manual_seed(seed)
        env = VecNormalizeWithCost(VecCostWrapper(HipSynthVecEnv(N, kind, seed)), **norm)
        env.set_cost_function(cost)
        out.append((PPOLagrangian("TwoCriticsMlpPolicy", env, n_steps=T, seed=seed), env))
    for a, _ in out[1:]:
        a.policy.load_state_dict(out[0][0].policy.state_dict())
    return out


def _noise(kind, rollouts, T, N, seed=8, scale=0.5):
    rng = np.random.RandomState(seed)
    return torch.as_tensor((scale * rng.randn(rollouts, T, N, _DIMS[kind][1])).astype(np.float32), device="cuda")


def _assert_identical(a_p, e_p, a_s, e_s, it=None):
    for k in _BUF_KEYS:
        got, ref = getattr(a_p.rollout_buffer, k).cpu().numpy(), getattr(a_s.rollout_buffer, k).cpu().numpy()
        assert np.array_equal(got, ref), (it, k, np.abs(got - ref).max())
    for name in ("obs_rms", "ret_rms", "cost_rms"):
        rp, rs = getattr(e_p, name), getattr(e_s, name)
        assert np.array_equal(np.asarray(rp.mean), np.asarray(rs.mean)) and np.array_equal(np.asarray(rp.var), np.asarray(rs.var)), name
        assert rp.count == rs.count, name
    assert torch.equal(e_p.ret, e_s.ret) and torch.equal(e_p.cost_ret, e_s.cost_ret)
    assert torch.equal(a_p._last_obs, a_s._last_obs) and torch.equal(a_p._ag["last_dones"], a_s._ag["last_dones"])
    assert torch.equal(e_p.unwrapped.s, e_s.unwrapped.s) and torch.equal(e_p.unwrapped.t_ep, e_s.unwrapped.t_ep)
    for k in ("raw_rew", "raw_cost", "dones", "last_v_r", "last_v_c", "act_clipped"):
        assert torch.equal(a_p._ag[k], a_s._ag[k]), k


def _both_outcomes(agent, what):
    """the condition on a compared rollout: its orig_costs plane holds both zero and non-zero rows"""
    c = agent.rollout_buffer.orig_costs
    assert bool((c == 0).any()) and bool((c != 0).any()), (what, float(c.min()), float(c.max()))


# ---- 1. icrl_cost_region_rows against the evaluator, exact ----------------------------------------------------------------------------------
_ROWS_GRID = 1024 * 256      # cost_region_rows_kernel: min(blocks, 1024) x 256 threads; row 262144 is thread 0's second
_BASE = 250                  # distinct rows of the large case (the evaluator is plain Python: its result is computed once and tiled)


def _specs(od, ad, disc):
    specs = RC.product_specs(od, ad) + [("8x8", RC.full_spec(od, ad))]
    return specs if disc else specs + RC.general_specs(od, ad)


@pytest.mark.parametrize("N,od,ad,disc", [(N, od, ad, disc) for od, ad, disc in ((18, 6, False), (113, 8, False), (2, 1, True)) for N in (1, 63)] +
                         [(_ROWS_GRID + 256, 18, 6, False)])
def test_rows_kernel_equals_the_row_evaluator(N, od, ad, disc):
    """N = 262400: one block's worth of threads takes a second row; the rows repeat with period 250 (no divisor of 256 but 2), so the second
    trip meets the threshold rows.  N = 1: the row is a threshold row of the spec's first clause."""
    from icrl_amd import _lib
    from icrl_amd.structs import p
    from icrl_amd.true_constraint_net import RegionCost
    specs = _specs(od, ad, disc)
    if N > _ROWS_GRID:
        specs = specs[::5] + [specs[18]]
    for i, (name, spec) in enumerate(specs):
        rc = RegionCost.from_spec(spec, od, ad, disc)
        base_n = min(N, _BASE)
        obs, acs, n_edge = RC.rows_for(spec, 300 + i, base_n, od, ad, disc)
        want = RC.evaluate(spec, obs, acs)
        if name != "8x8" or not disc:
            assert n_edge >= 1 and RC.on_threshold(spec, list(obs[0]), acs[0]), name
        if N > base_n:
            idx = np.arange(N) % base_n
            obs, acs, want = np.ascontiguousarray(obs[idx]), np.ascontiguousarray(acs[idx]), want[idx]
        to, ta = torch.as_tensor(obs, device="cuda"), torch.as_tensor(acs, device="cuda")
        got = rc(to, ta)
        assert torch.is_tensor(got) and got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (N,), name
        assert np.array_equal(got.cpu().numpy(), want), (name, np.flatnonzero(got.cpu().numpy() != want)[:8])
        if N <= _BASE:
            assert np.array_equal(rc(obs, acs), want), name      # the numpy form of the same object
        if N == 63:      # the descriptor through icrl_cost_mlp_forward; leading batch dimensions
            out = torch.full((N,), -1.0, device="cuda")
            _lib.check(_lib.lib().icrl_cost_mlp_forward(_lib.byref(rc.struct()), p(to), p(ta), N, p(out), _lib.current_stream()), "icrl_cost_mlp_forward")
            assert torch.equal(out, got), name
            g2 = rc(to[:60].reshape(4, 15, od), ta[:60].reshape(4, 15, -1))
            assert tuple(g2.shape) == (4, 15) and torch.equal(g2.reshape(-1), got[:60]), name
    if disc and N == 63:      # a discrete action as the buffer stores it: [N]
        rc = RegionCost.action_equals(1, od)
        a = torch.as_tensor(np.arange(N) % 3, dtype=torch.float32, device="cuda")
        assert np.array_equal(rc(None, a).cpu().numpy(), (np.arange(N) % 3 == 1).astype(np.float32))


# ---- 2. a RegionCost written as an analytic kind against the AnalyticCost, every launch form ------------------------------------------------
# the launch forms of tests/test_cost_fn_gpu.py (ant 40 "multi" cannot hold the multi-env kernel's statistics owners and runs the per-step
# launches, as there) and the per-step launches themselves
_FORM_ROUTES = {("hc", 7, "auto"): dict(route="persistent", wgs=7), ("hc", 130, "auto"): dict(route="wide", wgs=130),
                ("ant", 256, "auto"): dict(route="wide", wgs=256), ("hc", 20, "multi"): dict(route="multi", envs_per_wg=4, wgs=5),
                ("ant", 40, "multi"): "per-step", ("ant", 128, "multi"): dict(route="multi", envs_per_wg=4, wgs=32),
                ("hc", 7, "steps"): "per-step", ("ant", 8, "steps"): "per-step"}
_FORMS = [("hc", 7, 33, "auto"), ("hc", 130, 24, "auto"), ("ant", 256, 6, "auto"), ("hc", 20, 33, "multi"), ("ant", 40, 10, "multi"),
          ("ant", 128, 6, "multi"), ("hc", 7, 33, "steps"), ("ant", 8, 10, "steps")]
_DRY = {}


def _dry_interval(kind, N, T, kernel, noise, limit):
    """where observation column 0 lies in BOTH rollouts of this form (the observations of a rollout do not depend on the cost): the
    interval the two rollouts' [5 %, 95 %] ranges share, from a dry run with the same seed, computed once per form"""
    key = (kind, N, T, kernel)
    if key not in _DRY:
        from icrl_amd.true_constraint_net import AnalyticCost
        ((agent, env),) = _agents(N, T, 13, kind, [AnalyticCost.null()])
        agent.rollout_kernel = kernel
        agent._setup_learn(2 * N * T)
        env.unwrapped.t_ep.fill_(limit - T // 2)
        spans = []
        for it in range(2):
            agent.collect_rollouts(env, None, agent.rollout_buffer, T, "cost", noise=noise[it])
            col = np.sort(agent.rollout_buffer.orig_observations[..., 0].cpu().numpy().astype(np.float64).reshape(-1))
            spans.append((col[int(0.05 * len(col))], col[int(0.95 * len(col)) - 1]))
        lo, hi = max(s[0] for s in spans), min(s[1] for s in spans)
        assert lo < hi, spans
        _DRY[key] = (float(lo), float(hi))
    return _DRY[key]


@pytest.mark.parametrize("cost", ["wall", "both", "torque"])
@pytest.mark.parametrize("kind,N,T,kernel", [pytest.param(*f, id="-".join(map(str, f))) for f in _FORMS])
def test_region_cost_written_as_an_analytic_kind_equals_the_analytic_kernels(kind, N, T, kernel, cost):
    from icrl_amd.true_constraint_net import AnalyticCost, RegionCost
    od, ad = _DIMS[kind]
    limit = 1000 if kind == "hc" else 500
    noise = _noise(kind, 2, T, N)
    if cost == "torque":
        rc, ac = RegionCost.torque(0.5, od, ad), AnalyticCost.torque(0.5)
    else:
        lo, hi = _dry_interval(kind, N, T, kernel, noise, limit)
        mid, q1, q3 = 0.5 * (lo + hi), lo + 0.25 * (hi - lo), lo + 0.75 * (hi - lo)
        if cost == "wall":
            rc, ac = RegionCost.wall_behind(mid, 0, od, ad), AnalyticCost.wall_behind(mid, 0)
        else:
            rc, ac = RegionCost.wall_behind_and_infront(q1, q3, 0, od, ad), AnalyticCost.wall_behind_and_infront(q1, q3, 0)
    (a_r, e_r), (a_a, e_a) = _agents(N, T, 13, kind, [rc, ac])
    assert a_r._fused_chain() is not None and a_r._fused_rollout_ok("cost", T, a_r.rollout_buffer) and e_r.venv.region_cost() is rc
    a_r.rollout_kernel = a_a.rollout_kernel = kernel
    a_r._setup_learn(2 * N * T); a_a._setup_learn(2 * N * T)
    for env in (e_r, e_a):
        env.unwrapped.t_ep.fill_(limit - T // 2)           # every env crosses its time limit inside the first rollout
    route = _FORM_ROUTES[kind, N, kernel]
    for it in range(2):
        a_r.collect_rollouts(e_r, None, a_r.rollout_buffer, T, "cost", noise=noise[it])
        got = routes.check_rollout(route, f"region {kind} {N} {kernel} {cost}")
        assert got["pick"] & _pick_region() and not got["pick"] & routes.PICK_ANALYTIC
        a_a.collect_rollouts(e_a, None, a_a.rollout_buffer, T, "cost", noise=noise[it])
        got = routes.check_rollout(route, f"analytic {kind} {N} {kernel} {cost}")
        assert got["pick"] & routes.PICK_ANALYTIC and not got["pick"] & _pick_region()
        a_r.check_rollout_status(); a_a.check_rollout_status()
        _both_outcomes(a_r, (it, "region")); _both_outcomes(a_a, (it, "analytic"))
        _assert_identical(a_r, e_r, a_a, e_a, it)
        assert a_r.rollout_buffer.dones.sum().item() == (N if it == 0 else a_a.rollout_buffer.dones.sum().item())


# ---- 3. general specs: every fused form against the per-step launches; the per-step cost against the evaluator --------------------------------
def _general(kind, N, T, kernel, noise, limit, which):
    od, ad = _DIMS[kind]
    lo, hi = _dry_interval(kind, N, T, kernel, noise, limit)
    name, spec = RC.general_specs(od, ad, centre=0.5 * (lo + hi), scale=0.25 * (hi - lo) + 0.25)[which]
    return name, spec


@pytest.mark.parametrize("which", [0, 1, 2], ids=["halfspace", "neg-ball", "box-and-ball"])
@pytest.mark.parametrize("kind,N,T,kernel", [pytest.param(*f, id="-".join(map(str, f))) for f in _FORMS[:6]])
def test_general_specs_in_every_fused_form_equal_the_per_step_launches(kind, N, T, kernel, which):
    from icrl_amd.true_constraint_net import RegionCost
    od, ad = _DIMS[kind]
    limit = 1000 if kind == "hc" else 500
    noise = _noise(kind, 2, T, N)
    name, spec = _general(kind, N, T, kernel, noise, limit, which)
    (a_p, e_p), (a_s, e_s) = _agents(N, T, 13, kind, [RegionCost.from_spec(spec, od, ad), RegionCost.from_spec(json.dumps(spec), od, ad)])
    a_p.rollout_kernel, a_s.rollout_kernel = kernel, "steps"
    a_p._setup_learn(2 * N * T); a_s._setup_learn(2 * N * T)
    for env in (e_p, e_s):
        env.unwrapped.t_ep.fill_(limit - T // 2)
    for it in range(2):
        a_p.collect_rollouts(e_p, None, a_p.rollout_buffer, T, "cost", noise=noise[it])
        got = routes.check_rollout(_FORM_ROUTES[kind, N, kernel], f"{kind} {N} {kernel} {name}")
        assert got["pick"] & _pick_region()
        a_s.collect_rollouts(e_s, None, a_s.rollout_buffer, T, "cost", noise=noise[it])
        got = routes.check_rollout(dict(route="per-step", launches=2 * T), "steps")
        assert got["pick"] & _pick_region()
        a_p.check_rollout_status()
        _both_outcomes(a_p, (it, name)); _both_outcomes(a_s, (it, name, "steps"))
        _assert_identical(a_p, e_p, a_s, e_s, it)


@pytest.mark.parametrize("kind", ["hc", "ant"])
def test_per_step_cost_is_the_evaluator_on_the_steps_state(kind):
    from icrl_amd.true_constraint_net import RegionCost
    od, ad = _DIMS[kind]
    N = 8
    specs = RC.general_specs(od, ad, centre=0.0, scale=0.5) + [("8x8", RC.full_spec(od, ad))]
    for name, spec in specs:
        ((agent, env),) = _agents(N, 1, 5, kind, [RegionCost.from_spec(spec, od, ad)])
        agent.rollout_kernel = "steps"
        agent._setup_learn(4 * N)
        for it in range(3):          # (from the second step on the state is no longer the reset state)
            s_before = env.unwrapped.s.clone()
            agent.collect_rollouts(env, None, agent.rollout_buffer, 1, "cost", noise=_noise(kind, 1, 1, N, seed=it)[0])
            got = routes.check_rollout(dict(route="per-step", launches=2), kind)
            assert got["pick"] & _pick_region()
            want = RC.evaluate(spec, s_before.cpu().numpy().reshape(N, od), agent._ag["act_clipped"].cpu().numpy().reshape(N, ad))
            assert np.array_equal(agent._ag["raw_cost"].cpu().numpy().reshape(-1), want), (name, it)
            assert np.array_equal(agent.rollout_buffer.orig_costs.cpu().numpy().reshape(-1), want), (name, it)


def test_discrete_policy_and_the_action_column():
    """CLGW: the class index is action column 0 (action_equals(1) as a region cost against the analytic kind, fused and per-step)"""
    from icrl_amd.ppo_lag import PPOLagrangian
    from icrl_amd.true_constraint_net import AnalyticCost, RegionCost
    from icrl_amd.vec_env import HipSynthVecEnv, VecCostWrapper, VecNormalizeWithCost
    N, T, seed = 4, 50, 3
    out = []
    for cost, kernel in ((None, "auto"), (None, "steps"), (AnalyticCost.action_equals(1), "auto")):
        torch.manual_seed(seed)
        env = VecNormalizeWithCost(VecCostWrapper(HipSynthVecEnv(N, "clgw", seed)), norm_obs=False, norm_reward=False)
        env.set_cost_function(cost if cost is not None else RegionCost.action_equals(1, env.observation_space.shape[0]))
        agent = PPOLagrangian("TwoCriticsMlpPolicy", env, n_steps=T, seed=seed)
        agent.rollout_kernel = kernel
        out.append((agent, env))
    for a, _ in out[1:]:
        a.policy.load_state_dict(out[0][0].policy.state_dict())
    noise = torch.as_tensor(np.random.RandomState(8).rand(2, T, N).astype(np.float32), device="cuda")
    for a, _ in out:
        a._setup_learn(2 * N * T)
    for it in range(2):
        for i, (a, e) in enumerate(out):
            a.collect_rollouts(e, None, a.rollout_buffer, T, "cost", noise=noise[it])
            got = routes.rollout()
            assert (got["route"] == "per-step") == (i == 1) and got["launches"] == (2 * T if i == 1 else 1), got
            assert bool(got["pick"] & _pick_region()) == (i < 2)
            a.check_rollout_status()
        _both_outcomes(out[0][0], it)
        _assert_identical(out[0][0], out[0][1], out[1][0], out[1][1], it)
        _assert_identical(out[0][0], out[0][1], out[2][0], out[2][1], it)
        rb = out[0][0].rollout_buffer
        assert np.array_equal(rb.orig_costs.cpu().numpy(), (rb.actions.cpu().numpy().reshape(T, N) == 1).astype(np.float32))


# ---- 4. the fused launch against the per-step loop over the same object --------------------------------------------------------------------
def test_fused_rollout_equals_the_stepped_loop_under_the_switch(monkeypatch):
    from icrl_amd import _lib
    from icrl_amd.ppo_lag import PPOLagrangian
    from icrl_amd.true_constraint_net import RegionCost
    N, T = 8, 64
    noise = _noise("hc", 2, T, N, seed=3)
    spec = RC.general_specs(18, 6, centre=0.0, scale=0.5)[0][1]
    (a_f, e_f), (a_s, e_s) = _agents(N, T, 11, "hc", [RegionCost.from_spec(spec, 18, 6), RegionCost.from_spec(spec, 18, 6)])
    a_f._setup_learn(2 * N * T); a_s._setup_learn(2 * N * T)
    calls = []
    inner = PPOLagrangian._collect_rollouts_stepped

    def counted(self, *a, **k):
        calls.append(self)
        return inner(self, *a, **k)
    monkeypatch.setattr(PPOLagrangian, "_collect_rollouts_stepped", counted)
    for it in range(2):
        a_f.collect_rollouts(e_f, None, a_f.rollout_buffer, T, "cost", noise=noise[it])
        got = routes.check_rollout(dict(route="persistent", wgs=N, launches=1), "fused")
        assert got["pick"] & _lib.PICK_REGION and len(calls) == it
        monkeypatch.setenv("ICRL_REGION_COST_STEPPED", "1")
        assert a_s._fused_chain() is None and not a_s._fused_rollout_ok("cost", T, a_s.rollout_buffer)
        a_s.collect_rollouts(e_s, None, a_s.rollout_buffer, T, "cost", noise=noise[it])
        assert len(calls) == it + 1 and calls[-1] is a_s
        monkeypatch.setenv("ICRL_REGION_COST_STEPPED", "0")
        assert a_s._fused_chain() is not None
        _both_outcomes(a_f, it)
        diffs = {k: (getattr(a_s.rollout_buffer, k) - getattr(a_f.rollout_buffer, k)).abs().max().item() for k in _BUF_KEYS}
        print(f"[stepped vs fused] rollout {it}: max |diff| per plane {diffs}")
        for k in _BUF_KEYS:      # every plane identical
            assert torch.equal(getattr(a_s.rollout_buffer, k), getattr(a_f.rollout_buffer, k)), (it, k, diffs)
    assert a_s.num_timesteps == a_f.num_timesteps == 2 * N * T


# ---- 5. host envs --------------------------------------------------------------------------------------------------------------------------
def test_host_env_rollout_with_the_descriptor(monkeypatch):
    from icrl_amd import envs
    from icrl_amd.ppo_lag import PPOLagrangian
    from icrl_amd.true_constraint_net import RegionCost
    from icrl_amd.vec_env import DummyVecEnv, VecCostWrapper, VecNormalizeWithCost
    N, T, seed = 8, 16, 5
    spec = RC.general_specs(18, 6, centre=0.0, scale=0.5)[0][1]
    pairs = []
    for _ in range(2):
        env = VecNormalizeWithCost(VecCostWrapper(DummyVecEnv([envs.spec("HostHCWithPos-v0")] * N)))
        env.set_cost_function(RegionCost.from_spec(spec, 18, 6))
        pairs.append((PPOLagrangian("TwoCriticsMlpPolicy", env, n_steps=T, seed=seed), env))
    (a_h, e_h), (a_s, e_s) = pairs
    a_s.policy.load_state_dict(a_h.policy.state_dict())
    noise = _noise("hc", 2, T, N)
    a_h._setup_learn(2 * N * T); a_s._setup_learn(2 * N * T)
    for env in (e_h, e_s):
        env.unwrapped.env_method("set_t_ep", 1000 - T // 2)      # every env crosses its time limit inside the first rollout
    stepped = []
    inner = PPOLagrangian._collect_rollouts_stepped

    def counted(self, *a, **k):
        stepped.append(self)
        return inner(self, *a, **k)
    monkeypatch.setattr(PPOLagrangian, "_collect_rollouts_stepped", counted)
    for it in range(2):
        assert a_h._host_rollout_ok("cost", T, a_h.rollout_buffer)
        a_h.collect_rollouts(e_h, None, a_h.rollout_buffer, T, "cost", noise=noise[it])
        assert not stepped
        a_s._collect_rollouts_stepped(e_s, None, a_s.rollout_buffer, T, "cost", noise=noise[it])
        for k in _BUF_KEYS:
            got, ref = getattr(a_h.rollout_buffer, k).cpu().numpy(), getattr(a_s.rollout_buffer, k).cpu().numpy()
            assert np.array_equal(got, ref), (it, k, np.abs(got - ref).max())
        for name in ("obs_rms", "ret_rms", "cost_rms"):
            rh, rs = getattr(e_h, name), getattr(e_s, name)
            assert np.array_equal(np.asarray(rh.mean), np.asarray(rs.mean)) and np.array_equal(np.asarray(rh.var), np.asarray(rs.var)) and rh.count == rs.count, name
        assert torch.equal(e_h.ret, e_s.ret) and torch.equal(e_h.cost_ret, e_s.cost_ret)
        assert torch.equal(a_h._last_obs, a_s._last_obs) and torch.equal(e_h.unwrapped.s, e_s.unwrapped.s)
        _both_outcomes(a_h, it)
        stepped.clear()
    monkeypatch.undo()
    e_h.close(); e_s.close()


# ---- 6. end to end ----------------------------------------------------------------------------------------------------------------------------
def _cpg_cost_spec(spec, extra, monkeypatch):
    from icrl_amd import _lib
    from icrl_amd.cpg import build_parser, cpg
    from icrl_amd.ppo_lag import PPOLagrangian
    stepped, picks = [], []
    inner = PPOLagrangian._collect_rollouts_stepped

    def counted(self, *a, **k):
        stepped.append(1)
        return inner(self, *a, **k)
    monkeypatch.setattr(PPOLagrangian, "_collect_rollouts_stepped", counted)
    launch = PPOLagrangian._rollout_launch

    def recorded(self, job):
        launch(self, job)
        picks.append(routes.rollout())
    monkeypatch.setattr(PPOLagrangian, "_rollout_launch", recorded)
    argv = ["cpg", "--cost_spec", spec, *extra, "--n_steps", "64", "-t", "2048", "-ne", "2", "-s", "2", "-v", "0"]
    cfg = vars(build_parser().parse_args(argv)); cfg.update(rank=0, world_size=1, save_dir=None)
    model, hist = cpg(types.SimpleNamespace(**cfg), log=None)
    monkeypatch.undo()
    assert not stepped and model.num_timesteps == 2048
    assert all(r["pick"] & _lib.PICK_REGION and r["launches"] == 1 for r in picks), picks
    return model, hist, picks


def _buffer_cost(model, spec, low, high):
    rb = model.rollout_buffer
    obs = rb.orig_observations.cpu().numpy().astype(np.float64)
    acs = np.clip(rb.actions.cpu().numpy(), low, high)
    return RC.evaluate(spec, obs.reshape(-1, obs.shape[-1]), acs.reshape(-1, acs.shape[-1])).reshape(obs.shape[:2])


def test_cpg_cost_spec_hc_runs_in_the_persistent_kernel(tmp_path, monkeypatch):
    from icrl_amd.true_constraint_net import RegionCost
    spec = {"combine": "any", "clauses": [{"type": "halfspace", "cols": ["obs:0", "act:5"], "w": [-1.0, 0.5], "b": 0.0},
                                          {"type": "box", "cols": ["act:0", "act:1"], "lo": [0.5, None], "hi": [None, -0.5]}]}
    path = tmp_path / "hc_region.json"
    path.write_text(json.dumps(spec))
    model, hist, picks = _cpg_cost_spec(str(path), ["-tei", "HCWithPos-v0", "-eei", "HCWithPosTest-v0", "-nt", "8"], monkeypatch)
    assert len(picks) == 4 and all(r["route"] == "persistent" for r in picks), picks
    cost = model.env.venv.region_cost()
    assert isinstance(cost, RegionCost) and cost.name == "hc_region.json" and cost is model.env.venv.cost_function
    got = model.rollout_buffer.orig_costs.cpu().numpy()
    # (the float32 copy of the raw observation in the buffer decides a float64 halfspace differently only within float32 rounding of its
    # boundary: the rows whose |acc| is below that are left out, and they are few)
    o, a = model.rollout_buffer.orig_observations.cpu().numpy().astype(np.float64), np.clip(model.rollout_buffer.actions.cpu().numpy(), -1.0, 1.0)
    clear = np.abs(-o[..., 0] + 0.5 * a[..., 5].astype(np.float64)) > 1e-5
    want = _buffer_cost(model, spec, -1.0, 1.0)
    assert clear.mean() > 0.99 and np.array_equal(got[clear], want[clear])
    assert 0.0 < got.mean() < 1.0 and got.shape == (64, 8)
    assert len(hist) == 4 and all(np.isfinite(h["rollout/adjusted_reward"]) and np.isfinite(h["eval/true_cost"]) for h in hist)


def test_cpg_cost_spec_point_circle_runs_in_the_multi_env_kernel(monkeypatch):
    """the README's example: PointCircle with a forbidden disc"""
    spec = {"clauses": [{"type": "ball", "cols": ["obs:0", "obs:1"], "center": [0.0, 0.0], "radius": 0.25}]}
    model, hist, picks = _cpg_cost_spec(json.dumps(spec), ["-tei", "PointCircle-v0", "-eei", "PointCircle-v0", "-nt", "16"], monkeypatch)
    assert len(picks) == 2 and all(r["route"] == "multi" for r in picks), picks
    got = model.rollout_buffer.orig_costs.cpu().numpy()
    o = model.rollout_buffer.orig_observations.cpu().numpy().astype(np.float64)
    clear = np.abs(o[..., 0] ** 2 + o[..., 1] ** 2 - 0.0625) > 1e-6      # (see the HC test: the buffer keeps a float32 copy of the observation)
    want = _buffer_cost(model, spec, -0.25, 0.25)
    assert clear.mean() > 0.99 and np.array_equal(got[clear], want[clear]) and got.shape == (64, 16)
    assert set(np.unique(got)) <= {0.0, 1.0} and len(hist) == 2


def test_icrl_cost_spec_true_cost_is_the_evaluators_mean_over_the_sampled_rows(tmp_path, monkeypatch):
    from icrl_amd import icrl as I
    from icrl_amd.true_constraint_net import RegionCost
    spec = {"combine": "sum", "clauses": [{"type": "box", "cols": ["act:0"], "lo": [0.25]}, {"type": "ball", "cols": ["act:1", "act:2"], "center": [0.0, 0.0], "radius": 0.5}]}
    seen = []
    inner = I.mean_cost

    def recorded(fn, obs, acs):
        v = inner(fn, obs, acs)
        seen.append((fn, obs.detach().cpu().numpy().copy() if torch.is_tensor(obs) else np.array(obs), acs.detach().cpu().numpy().copy() if torch.is_tensor(acs) else np.array(acs), v))
        return v
    monkeypatch.setattr(I, "mean_cost", recorded)
    here = os.path.dirname(os.path.abspath(__file__))
    argv = ["icrl", "--cost_spec", json.dumps(spec), "-er", "2", "-ep", os.path.join(here, "golden/expert_hc.npz"), "-tk", "0.01", "-cl", "20", "-bi", "2",
            "-ft", "1024", "-ni", "1", "-tei", "HCWithPos-v0", "-eei", "HCWithPosTest-v0", "-clr", "0.05", "-aclr", "0.9", "-crc", "0.5", "-psis",
            "-ctkno", "2.5", "-nt", "8", "--n_steps", "128", "-s", "0", "--save_dir", str(tmp_path), "-v", "0"]
    cfg = vars(I.build_parser().parse_args(argv))
    cfg.update(rank=0, world_size=1)
    metrics, agent, cn, env = I.icrl(types.SimpleNamespace(**cfg), log=None)
    monkeypatch.undo()
    assert len(metrics) == 1 and len(seen) == 1
    fn, obs, acs, value = seen[0]
    assert isinstance(fn, RegionCost) and (fn.obs_dim, fn.acs_dim) == (18, 6)
    want = RC.evaluate(spec, obs.reshape(-1, 18), acs.reshape(-1, 6))
    # the rows' costs bit for bit; the logged mean is their float64 mean (sum of small integers: exact) up to the rounding of the division,
    # which torch and numpy do not place alike (2 eps relative)
    assert np.array_equal(fn(torch.as_tensor(obs, device="cuda"), torch.as_tensor(acs, device="cuda")).cpu().numpy().reshape(-1), want)
    exact = float(want.astype(np.float64).sum()) / want.size
    assert metrics[0]["true/cost"] == value and abs(value - exact) <= 2 * np.finfo(np.float64).eps * exact, (value, exact)
    assert 0.0 < value < 2.0
