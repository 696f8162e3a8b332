"""GPU: analytic costs (true_constraint_net.AnalyticCost / icrl_cost_fn_t) inside the fused rollout launches — the rows kernel against
numpy, every persistent kernel form against the per-step launches bit for bit, the costs of a rollout against numpy on the rollout's own
buffer, the fused path against the per-step loop over the same cost object, the discrete and the host-env chains, and cpg end to end."""
import os
import types

import numpy as np
import pytest
import torch

import tests.helpers.host_envs  # noqa: F401  (registers the Host* ids)
from helpers import routes
from helpers.cost_fn_cases import boundary_acs, boundary_obs

pytestmark = pytest.mark.gpu

_BUF_KEYS = ("observations", "orig_observations", "new_observations", "new_orig_observations", "actions", "rewards", "costs",
             "orig_costs", "dones", "log_probs", "reward_values", "cost_values", "reward_advantages", "cost_advantages",
             "reward_returns", "cost_returns")
_WIDE_POLICY = dict(policy_kwargs=dict(net_arch=[dict(pi=[128, 96], vf=[80, 128], cvf=[128, 128])]))


def _cost(name):
    from icrl_amd.true_constraint_net import AnalyticCost
    return {"wall": lambda: AnalyticCost.wall_behind(0.0), "torque": lambda: AnalyticCost.torque(0.5),
            "both": lambda: AnalyticCost.wall_behind_and_infront(-0.25, 0.25), "null": AnalyticCost.null,
            "action": lambda: AnalyticCost.action_equals(1)}[name]()


def _pair(N, T, seed, kind, cost, agent_kwargs=None, **norm):
    """two agents over twin device chains VecNormalizeWithCost -> VecCostWrapper(AnalyticCost) -> HipSynthVecEnv, same policy."""
    from icrl_amd.ppo_lag import PPOLagrangian
    from icrl_amd.vec_env import HipSynthVecEnv, VecCostWrapper, VecNormalizeWithCost
    out = []
    for _ in range(2):
        torch.manual_seed(seed)
        env = VecNormalizeWithCost(VecCostWrapper(HipSynthVecEnv(N, kind, seed)), **norm)
        env.set_cost_function(_cost(cost))
        out.append((PPOLagrangian("TwoCriticsMlpPolicy", env, n_steps=T, seed=seed, **(agent_kwargs or {})), env))
    out[1][0].policy.load_state_dict(out[0][0].policy.state_dict())
    return out


def _noise(kind, rollouts, T, N, seed=8, scale=0.5):
    """(scaled so that |action| > 0.5 happens in some rows and not in others: the policy's initial std is 1)"""
    rng = np.random.RandomState(seed)
    if kind in ("lgw", "clgw"):
        return torch.as_tensor(rng.rand(rollouts, T, N).astype(np.float32), device="cuda")
    ad = 6 if kind == "hc" else 8
    return torch.as_tensor((scale * rng.randn(rollouts, T, N, ad)).astype(np.float32), device="cuda")


def _assert_identical(a_p, e_p, a_s, e_s, it=None, carry=True):
    for k in _BUF_KEYS:
        got, ref = getattr(a_p.rollout_buffer, k).cpu().numpy(), getattr(a_s.rollout_buffer, k).cpu().numpy()
        assert np.array_equal(got, ref), (it, k, np.abs(got - ref).max())
    for name in ("obs_rms", "ret_rms", "cost_rms"):
        rp, rs = getattr(e_p, name), getattr(e_s, name)
        assert np.array_equal(np.asarray(rp.mean), np.asarray(rs.mean)) and np.array_equal(np.asarray(rp.var), np.asarray(rs.var)), name
        assert rp.count == rs.count, name
    assert torch.equal(e_p.ret, e_s.ret) and torch.equal(e_p.cost_ret, e_s.cost_ret)
    assert torch.equal(a_p._last_obs, a_s._last_obs) and torch.equal(a_p._ag["last_dones"], a_s._ag["last_dones"])
    assert torch.equal(e_p.unwrapped.s, e_s.unwrapped.s)
    for k in ("raw_cost", "act_clipped", "last_v_r", "last_v_c") if carry else ():
        assert torch.equal(a_p._ag[k], a_s._ag[k]), k


def _numpy_cost(cost, rb, env):
    """the closed form on the rollout's own buffer: the wall on the float32 copy of the raw observation (the sign survives the store),
    the torque on the clipped actions the env received."""
    if cost == "wall":
        return (rb.orig_observations.cpu().numpy()[..., 0] <= 0.0).astype(np.float32)
    if cost == "torque":
        acs = np.clip(rb.actions.cpu().numpy(), env.action_space.low, env.action_space.high)
        return np.any(np.abs(acs) > np.float32(0.5), axis=-1).astype(np.float32)
    raise KeyError(cost)


# ---- 1. icrl_cost_fn_rows against numpy, exact --------------------------------------------------------------------------------------
_ROWS_GRID = 1024 * 256      # cost_fn_rows_kernel: min(blocks, 1024) x 256 threads; row 262144 is thread 0's second


@pytest.mark.parametrize("N,od,ad", [(N, od, ad) for od, ad in ((18, 6), (113, 8)) for N in (1, 63, 257)] + [(_ROWS_GRID + 256, 18, 6)])
def test_rows_kernel_equals_numpy(N, od, ad):
    """N = 262400: one block's worth of threads takes a second row, and those rows are the edge rows (tiled), so that the second trip meets
    the thresholds themselves."""
    from icrl_amd.true_constraint_net import AnalyticCost
    rng = np.random.RandomState(N + od)
    index = od - 1
    lo, hi, thr = -0.3, 0.7, 0.3
    obs = rng.randn(N, od) * 0.8
    edge = boundary_obs(lo, hi, index, od)
    obs[:min(N, len(edge))] = edge[:N]
    if N == 1:
        obs[0, index] = lo                                   # the threshold itself
    acs = (rng.randn(N, ad) * 0.3).astype(np.float32)
    eacs = boundary_acs(thr, ad)
    acs[:min(N, len(eacs))] = eacs[:N]
    if N == 1:
        acs[0, ad - 1] = -np.nextafter(np.float32(thr), np.float32(1))
    if N > _ROWS_GRID:
        tail = N - _ROWS_GRID
        assert tail >= len(edge) and tail >= len(eacs)
        obs[_ROWS_GRID:] = edge[np.arange(tail) % len(edge)]
        acs[_ROWS_GRID:] = eacs[np.arange(tail) % len(eacs)]
    disc = rng.randint(0, 3, size=(N, 1)).astype(np.float32)
    to, ta, td = (torch.as_tensor(x, device="cuda") for x in (obs, acs, disc))
    col = obs[:, index]
    cases = [(AnalyticCost.null(), np.zeros(N), (to, ta)),
             (AnalyticCost.wall_behind(lo, index), col <= lo, (to, None)),
             (AnalyticCost.wall_infront(hi, index), col >= hi, (to, ta)),
             (AnalyticCost.wall_behind_and_infront(lo, hi, index), (col <= lo).astype(np.float32) + (col >= hi).astype(np.float32), (to, None)),
             (AnalyticCost.wall_behind_and_infront(hi, lo, index), (col <= hi).astype(np.float32) + (col >= lo).astype(np.float32), (to, ta)),
             (AnalyticCost.torque(thr), np.any(np.abs(acs) > np.float32(thr), axis=-1), (None, ta)),
             (AnalyticCost.torque(thr), np.any(np.abs(acs) > np.float32(thr), axis=-1), (to, ta)),
             (AnalyticCost.action_equals(1), disc[:, 0] == 1, (None, td)),
             (AnalyticCost.action_equals(2), disc[:, 0] == 2, (to, td[:, 0].contiguous()))]
    for fn, want, args in cases:
        got = fn(*args)
        assert torch.is_tensor(got) and got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (N,), fn
        assert np.array_equal(got.cpu().numpy(), np.asarray(want, np.float32)), fn
        host = fn(*(None if a is None else a.cpu().numpy() for a in args))      # the numpy form of the same object
        assert np.array_equal(np.asarray(host, np.float32), np.asarray(want, np.float32)), fn
    if N == 257:        # leading batch dimensions, and the descriptor through icrl_cost_mlp_forward
        from icrl_amd import _lib
        from icrl_amd.structs import p
        got = AnalyticCost.wall_behind(lo, index)(to[:256].reshape(4, 64, od), None)
        assert tuple(got.shape) == (4, 64) and np.array_equal(got.cpu().numpy().reshape(-1), (col[:256] <= lo).astype(np.float32))
        out = torch.full((N,), -1.0, device="cuda")
        cf = AnalyticCost.torque(thr).struct(od, ad)
        _lib.check(_lib.lib().icrl_cost_mlp_forward(_lib.byref(cf), p(to), p(ta), N, p(out), _lib.current_stream()), "icrl_cost_mlp_forward")
        assert np.array_equal(out.cpu().numpy(), np.any(np.abs(acs) > np.float32(thr), axis=-1).astype(np.float32))


# ---- 2. every persistent kernel form against the per-step launches, bit for bit -----------------------------------------------------
# one-workgroup-per-env | wide, two hops | wide, Ant (OCT 8) | multi, E = 4 with a ragged last workgroup | multi at Ant widths (40 envs
# cannot hold the 115 statistics owners of the multi-env kernel, nor the 115 workgroups of the wide kernel, and are 4520 > 4096 observation
# doubles: they run the per-step launches on both sides, which only shows that the forced flag is harmless there; 128 envs = 32 workgroups
# of 4 reach the multi-env kernel) | generic persistent kernel around a policy with layers above 64 units
# _FORM_ROUTES: what icrl_rollout_collect must have launched for each, asserted behind the call
_FORM_ROUTES = {("hc", 7, "auto"): "persistent", ("hc", 130, "auto"): dict(route="wide", wgs=130), ("ant", 256, "auto"): dict(route="wide", wgs=256),
                ("hc", 20, "multi"): dict(route="multi", envs_per_wg=4, wgs=5), ("ant", 40, "multi"): "per-step",
                ("ant", 128, "multi"): dict(route="multi", envs_per_wg=4, wgs=32), ("hc", 12, "wide-policy"): "generic-persistent"}
_FORMS = [("hc", 7, 33, "auto"), ("hc", 130, 24, "auto"), ("ant", 256, 6, "auto"), ("hc", 20, 33, "multi"), ("ant", 40, 10, "multi"),
          ("ant", 128, 6, "multi"), ("hc", 12, 40, "wide-policy")]


def _form_cases():
    """every form under both costs; a forced kernel that does not take its shape carries what runs instead in its id"""
    out = []
    for f in _FORMS:
        route = _FORM_ROUTES[f[0], f[1], f[3]]
        falls = f[3] == "multi" and route == "per-step"
        for c in ("wall", "torque"):
            out.append(pytest.param(*f, c, id="-".join(str(x) for x in f) + ("-falls-to-per-step" if falls else "") + "-" + c))
    return out + [pytest.param("hc", 7, 33, "auto", "both", id="hc-7-33-auto-both")]


@pytest.mark.parametrize("kind,N,T,kernel,cost", _form_cases())
def test_persistent_forms_equal_per_step_launches(kind, N, T, kernel, cost):
    limit = 1000 if kind == "hc" else 500
    akw = _WIDE_POLICY if kernel == "wide-policy" else None
    (a_p, e_p), (a_s, e_s) = _pair(N, T, 13, kind, cost, agent_kwargs=akw)
    assert a_p._fused_chain() is not None and a_p._fused_rollout_ok("cost", T, a_p.rollout_buffer)
    a_s.rollout_kernel = "steps"
    if kernel == "wide-policy":
        assert a_p.policy.wide
    else:
        a_p.rollout_kernel = kernel
    noise = _noise(kind, 2, T, N)
    a_p._setup_learn(2 * N * T); a_s._setup_learn(2 * N * T)
    for env in (e_p, e_s):
        env.unwrapped.t_ep.fill_(limit - T // 2)           # every env crosses its time limit inside the first rollout
    fired = []
    for it in range(2):
        a_p.collect_rollouts(e_p, None, a_p.rollout_buffer, T, "cost", noise=noise[it])
        got = routes.check_rollout(_FORM_ROUTES[kind, N, kernel], f"{kind} {N} {kernel} {cost}")
        assert got["pick"] & routes.PICK_ANALYTIC      # (the instantiations without a cost-net register image)
        a_s.collect_rollouts(e_s, None, a_s.rollout_buffer, T, "cost", noise=noise[it])
        # (the launches per step: two, or the generic-shape path's policy forward, env step and normaliser — the analytic cost needs no launch)
        routes.check_rollout(dict(route="generic-per-step", launches=3 * T) if kernel == "wide-policy" else dict(route="per-step", launches=2 * T), "steps")
        a_p.check_rollout_status()
        _assert_identical(a_p, e_p, a_s, e_s, it)
        assert a_p.rollout_buffer.dones.sum().item() == (N if it == 0 else a_s.rollout_buffer.dones.sum().item())
        fired.append(float(a_p.rollout_buffer.orig_costs.mean().item()))
        if cost in ("wall", "torque"):
            assert np.array_equal(a_p.rollout_buffer.orig_costs.cpu().numpy(), _numpy_cost(cost, a_p.rollout_buffer, e_p)), it
    assert torch.equal(e_p.unwrapped.t_ep, e_s.unwrapped.t_ep)
    for k in ("raw_rew", "dones"):
        assert torch.equal(a_p._ag[k], a_s._ag[k]), k
    assert 0.0 < np.mean(fired) < (2.0 if cost == "both" else 1.0), fired


# ---- 3. the costs of a fused rollout against numpy on its own buffer ----------------------------------------------------------------
@pytest.mark.parametrize("cost", ["wall", "torque"])
def test_rollout_costs_equal_numpy_on_the_rollouts_buffer(cost):
    N, T = 4, 30
    (agent, env), _ = _pair(N, T, 2, "hc", cost, norm_cost=False)
    agent._setup_learn(N * T)
    agent.collect_rollouts(env, None, agent.rollout_buffer, T, "cost", noise=_noise("hc", 1, T, N, seed=2)[0])
    agent.check_rollout_status()
    rb = agent.rollout_buffer
    got, want = rb.orig_costs.cpu().numpy(), _numpy_cost(cost, rb, env)
    assert np.array_equal(got, want)
    assert 0.0 < got.mean() < 1.0, got.mean()
    assert np.array_equal(rb.costs.cpu().numpy(), got)          # norm_cost off: the buffer's cost is the raw one


# ---- 4. the fused launch against the per-step loop over the same cost object --------------------------------------------------------
@pytest.mark.parametrize("cost", ["wall", "torque"])
def test_fused_rollout_equals_the_stepped_loop(cost):
    N, T = 16, 48
    (a_f, e_f), (a_s, e_s) = _pair(N, T, 11, "hc", cost)
    noise = _noise("hc", 2, T, N, seed=3)
    a_f._setup_learn(2 * N * T); a_s._setup_learn(2 * N * T)
    for it in range(2):
        a_f.collect_rollouts(e_f, None, a_f.rollout_buffer, T, "cost", noise=noise[it])
        a_s._collect_rollouts_stepped(e_s, None, a_s.rollout_buffer, T, "cost", noise=noise[it])
        for a, e in ((a_f, e_f), (a_s, e_s)):       # each run's costs are the closed form on its own observations / actions
            assert np.array_equal(a.rollout_buffer.orig_costs.cpu().numpy(), _numpy_cost(cost, a.rollout_buffer, e)), it
        assert torch.equal(a_f.rollout_buffer.orig_costs, a_s.rollout_buffer.orig_costs), it      # no cost flipped between the two drivers
        for k in _BUF_KEYS:
            got, ref = getattr(a_s.rollout_buffer, k).cpu().numpy(), getattr(a_f.rollout_buffer, k).cpu().numpy()
            assert np.allclose(got, ref, rtol=2e-5, atol=2e-6), (it, k, np.abs(got - ref).max())
        assert 0.0 < float(a_f.rollout_buffer.orig_costs.mean().item()) < 1.0
    assert np.allclose(e_s.obs_rms.mean, e_f.obs_rms.mean, rtol=0, atol=1e-12)
    assert abs(e_s.cost_rms.var - e_f.cost_rms.var) < 1e-12 and abs(e_s.cost_rms.mean - e_f.cost_rms.mean) < 1e-12
    assert a_s.num_timesteps == a_f.num_timesteps == 2 * N * T


def test_the_switch_forces_the_stepped_loop(monkeypatch):
    (agent, env), _ = _pair(4, 8, 1, "hc", "wall")
    assert agent._fused_chain() is not None
    monkeypatch.setenv("ICRL_ANALYTIC_COST_STEPPED", "1")
    assert agent._fused_chain() is None and not agent._fused_rollout_ok("cost", 8, agent.rollout_buffer)
    monkeypatch.setenv("ICRL_ANALYTIC_COST_STEPPED", "0")
    assert agent._fused_chain() is not None


# ---- 5. discrete actions --------------------------------------------------------------------------------------------------------------
def test_discrete_action_equals_cost():
    N, T = 4, 50
    (a_p, e_p), (a_s, e_s) = _pair(N, T, 3, "clgw", "action", norm_obs=False, norm_reward=False)
    a_s.rollout_kernel = "steps"
    noise = _noise("clgw", 2, T, N)
    a_p._setup_learn(2 * N * T); a_s._setup_learn(2 * N * T)
    for it in range(2):
        a_p.collect_rollouts(e_p, None, a_p.rollout_buffer, T, "cost", noise=noise[it])
        a_s.collect_rollouts(e_s, None, a_s.rollout_buffer, T, "cost", noise=noise[it])
        a_p.check_rollout_status()
        _assert_identical(a_p, e_p, a_s, e_s, it)
        rb = a_p.rollout_buffer
        want = (rb.actions.cpu().numpy().reshape(T, N) == 1).astype(np.float32)
        assert np.array_equal(rb.orig_costs.cpu().numpy(), want) and 0.0 < want.mean() < 1.0


# ---- 6. host envs -----------------------------------------------------------------------------------------------------------------------
def test_host_env_rollout_and_episodes(monkeypatch):
    from icrl_amd import envs, utils
    from icrl_amd.ppo_lag import PPOLagrangian
    from icrl_amd.vec_env import DummyVecEnv, HipSynthVecEnv, VecCostWrapper, VecNormalizeWithCost, dynamics_matrix
    N, T, seed = 7, 20, 5
    e_d = VecNormalizeWithCost(VecCostWrapper(HipSynthVecEnv(N, "hc", seed)))
    e_h = VecNormalizeWithCost(VecCostWrapper(DummyVecEnv([envs.spec("HostHCWithPos-v0")] * N)))
    for e in (e_d, e_h):
        e.set_cost_function(_cost("wall"))
    a_d = PPOLagrangian("TwoCriticsMlpPolicy", e_d, n_steps=T, seed=seed)
    a_h = PPOLagrangian("TwoCriticsMlpPolicy", e_h, n_steps=T, seed=seed)
    a_h.policy.load_state_dict(a_d.policy.state_dict())
    a_d.rollout_kernel = "steps"
    noise = _noise("hc", 2, T, N)
    a_d._setup_learn(2 * N * T); a_h._setup_learn(2 * N * T)
    e_d.unwrapped.t_ep.fill_(1000 - T // 2)
    e_h.unwrapped.env_method("set_t_ep", 1000 - T // 2)
    stepped = []
    monkeypatch.setattr(PPOLagrangian, "_collect_rollouts_stepped", lambda self, *a, **k: stepped.append(1))
    for it in range(2):
        a_d.collect_rollouts(e_d, None, a_d.rollout_buffer, T, "cost", noise=noise[it])
        assert a_h._host_rollout_ok("cost", T, a_h.rollout_buffer)
        a_h.collect_rollouts(e_h, None, a_h.rollout_buffer, T, "cost", noise=noise[it])
        _assert_identical(a_h, e_h, a_d, e_d, it)
        got = a_h.rollout_buffer.orig_costs.cpu().numpy()
        assert np.array_equal(got, _numpy_cost("wall", a_h.rollout_buffer, e_h)) and 0.0 < got.mean() < 1.0
    assert not stepped
    monkeypatch.undo()
    e_h.close()
    # sampling episodes over a 1-env host chain whose cost wrapper holds an AnalyticCost: the one-launch-per-step path, same rows as the loop
    sd = a_h.policy.state_dict()
    sd["action_net.bias"] = torch.as_tensor(-0.5 * np.sign(dynamics_matrix("hc")[0]), dtype=torch.float32)      # towards the wall: short episodes
    a_h.policy.load_state_dict(sd)
    n_ep = 2
    runs = []
    for forced in ("0", "1"):
        monkeypatch.setenv("ICRL_HOST_EPISODES_STEPPED", forced)
        ev = utils.make_eval_env("HostHCWithPosTest-v0", True, normalize_obs=True, seed=3)
        ev.set_cost_function(_cost("wall"))
        assert utils.host_episodes_ok(a_h, ev) == (forced == "0")
        rows = n_ep * ev.unwrapped.max_steps
        ep_noise = np.random.RandomState(0).randn(rows, 6).astype(np.float32)
        runs.append([np.asarray(x.cpu().numpy() if torch.is_tensor(x) else x) for x in utils.sample_from_agent(a_h, ev, n_ep, noise=ep_noise)])
    for g, r in zip(*runs):
        assert g.shape == r.shape and np.array_equal(g, r)
    assert runs[0][4].max() < 1000


# ---- 7. cpg end to end ------------------------------------------------------------------------------------------------------------------
def _cpg(extra, monkeypatch, stepped_switch=None):
    from icrl_amd.cpg import build_parser, cpg
    from icrl_amd.ppo_lag import PPOLagrangian
    if stepped_switch is not None:
        monkeypatch.setenv("ICRL_ANALYTIC_COST_STEPPED", stepped_switch)
    calls = []
    inner = PPOLagrangian._collect_rollouts_stepped

    def counted(self, *a, **k):
        calls.append(1)
        return inner(self, *a, **k)
    monkeypatch.setattr(PPOLagrangian, "_collect_rollouts_stepped", counted)
    argv = ["cpg", "-tei", "HCWithPos-v0", "-eei", "HCWithPosTest-v0", "-nt", "8", "-ns", "64", "-t", "1024", "-ne", "2", "-s", "0", "-v", "0"] + extra
    cfg = vars(build_parser().parse_args(argv)); cfg.update(rank=0, world_size=1, save_dir=None)
    model, hist = cpg(types.SimpleNamespace(**cfg), log=None)
    monkeypatch.undo()
    return model, hist, len(calls)


def test_cpg_runs_its_rollouts_fused(monkeypatch):
    from icrl_amd.true_constraint_net import AnalyticCost
    for switch, want_calls in (("0", 0), ("1", 2)):
        model, hist, calls = _cpg([], monkeypatch, switch)
        assert calls == want_calls, (switch, calls)
        assert isinstance(model.env.venv.analytic_cost(), AnalyticCost) and model.env.venv.analytic_cost().name == "wall_behind"
        assert model.num_timesteps == 1024 and len(hist) == 2 and model.policy.adam_step > 0
        for h in hist:
            assert np.isfinite(h["eval/true_cost"]) and np.isfinite(h["rollout/adjusted_reward"]), h
    model, hist, calls = _cpg(["--use_null_cost"], monkeypatch, "0")
    assert calls == 0 and model.env.venv.analytic_cost().name == "null_cost"
    assert float(model.rollout_buffer.orig_costs.abs().max().item()) == 0.0 and float(model.rollout_buffer.costs.abs().max().item()) == 0.0
    assert model.policy.adam_step > 0 and len(hist) == 2 and all(np.isfinite(h["rollout/adjusted_reward"]) for h in hist)


# ---- 8. a callable handed to learn() keeps the per-step loop ------------------------------------------------------------------------------
def test_learn_with_a_callable_still_takes_the_stepped_loop(monkeypatch):
    from icrl_amd.ppo_lag import PPOLagrangian
    from icrl_amd.true_constraint_net import null_cost
    N, T = 4, 16
    (agent, env), _ = _pair(N, T, 5, "hc", "wall", agent_kwargs=dict(batch_size=32, n_epochs=1))
    assert agent._fused_chain() is not None
    calls = []
    inner = PPOLagrangian._collect_rollouts_stepped

    def counted(self, *a, **k):
        calls.append(1)
        return inner(self, *a, **k)
    monkeypatch.setattr(PPOLagrangian, "_collect_rollouts_stepped", counted)
    agent.learn(N * T, cost_function=null_cost)
    assert len(calls) == 1
    assert float(agent.rollout_buffer.costs.abs().max().item()) == 0.0 and agent.policy.adam_step > 0
    agent.learn(N * T, cost_function="cost")          # the string key: the fused launch, the wrapper's AnalyticCost
    assert len(calls) == 1
