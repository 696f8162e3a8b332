"""GPU: sampling / evaluation episodes over host envs (utils.HostEpisodeRun: one icrl_host_episode_step launch per env step) against
the device sampler (icrl_sample_episodes over the device twin of the same env) and against the per-step loop
(utils.SteppedEpisodeRun) — rows, episode sums, lengths and the state left in the env chain, bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import tests.helpers.host_envs  # noqa: F401  (registers the Host* ids)

pytestmark = pytest.mark.gpu

# kind -> (device id, host twin, id of the train env the agent is built over)
_IDS = {"hc": ("HCWithPos-v0", "HostHCWithPos-v0", "HCWithPos-v0"), "hctest": ("HCWithPosTest-v0", "HostHCWithPosTest-v0", "HCWithPos-v0"),
        "ant": ("AntWall-v0", "HostAntWall-v0", "AntWall-v0"), "lgw": ("LGW-v0", "HostLGW-v0", "LGW-v0"),
        "clgw": ("CLGW-v0", "HostCLGW-v0", "LGW-v0")}
_DISCRETE = ("lgw", "clgw")
_EARLY_END = ("hctest", "clgw")      # episodes also end before the time limit (the wall at obs[0] <= -3, the backward action)
_WIDE = dict(net_arch=[dict(pi=[128, 128], vf=[64, 64], cvf=[64, 64])])


def _agent(kind, seed=3, policy_kwargs=None):
    """a fresh policy over a 4-env device train chain of the kind; for hctest its action bias drives obs[0] towards the wall, so that
    with unit noise episodes end after a few dozen steps, at lengths that differ from episode to episode."""
    from icrl_amd import utils
    from icrl_amd.ppo_lag import PPOLagrangian
    from icrl_amd.vec_env import dynamics_matrix
    norm = kind not in _DISCRETE
    env = utils.make_train_env(_IDS[kind][2], None, True, seed, 4, normalize_obs=norm, normalize_reward=norm, normalize_cost=norm,
                               cost_info_str="cost", reward_gamma=0.99, cost_gamma=0.99)
    agent = PPOLagrangian("TwoCriticsMlpPolicy", env, n_steps=32, seed=seed, policy_kwargs=policy_kwargs)
    if kind == "hctest":
        sd = agent.policy.state_dict()
        sd["action_net.bias"] = torch.as_tensor(-0.5 * np.sign(dynamics_matrix("hc")[0]), dtype=torch.float32)
        agent.policy.load_state_dict(sd)
    if kind == "clgw":        # mostly forward: the backward action (the end of a CLGW episode) comes after a few steps, not at the first
        sd = agent.policy.state_dict()
        sd["action_net.bias"] = torch.as_tensor([1.5, 0.0], dtype=torch.float32)
        agent.policy.load_state_dict(sd)
    return agent


def _eval_env(env_id, norm=True, seed=3, cost_wrapper=False):
    """utils.make_eval_env with frozen statistics that are not the initial (0, 1) ones."""
    from icrl_amd import utils
    env = utils.make_eval_env(env_id, cost_wrapper, normalize_obs=norm, seed=seed)
    O = env.observation_space.shape[0]
    rng = np.random.RandomState(11)
    env.obs_rms.assign(0.3 * rng.randn(O), 0.5 + rng.rand(O), 100.0)
    return env


def _noise(kind, agent, env, n_ep, seed=0):
    rows = n_ep * env.unwrapped.max_steps
    rng = np.random.RandomState(seed)
    if kind in _DISCRETE:
        return rng.rand(rows).astype(np.float32)
    return rng.randn(rows, agent.policy.act_dim).astype(np.float32)


def _np(result):
    oo, o, a, r, l = result
    return oo.cpu().numpy(), o.cpu().numpy(), a.cpu().numpy(), np.asarray(r), np.asarray(l)


def _assert_same_result(got, ref, what=""):
    for name, g, r in zip(("orig_obs", "obs", "actions", "ep_rewards", "lengths"), got, ref):
        assert g.shape == r.shape, (what, name, g.shape, r.shape)
        assert g.dtype == r.dtype, (what, name, g.dtype, r.dtype)
        assert np.array_equal(g, r), (what, name, np.abs(g.astype(np.float64) - r.astype(np.float64)).max())


def _cost_net(od, ad, discrete=False):
    from icrl_amd.constraint_net import ConstraintNet
    torch.manual_seed(7)
    if discrete:
        return ConstraintNet(od, ad, [20], None, lambda x: 0.003, None, None, True, clip_obs=20)
    lo = -np.ones(ad, np.float32)
    return ConstraintNet(od, ad, [20], None, lambda x: 0.05, None, None, False, 0.5, clip_obs=20, action_low=lo, action_high=-lo)


# ---- 1. host path == device sampler ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,norm", [("hc", True), ("hc", False), ("ant", True), ("ant", False), ("lgw", True), ("lgw", False),
                                       ("clgw", True), ("clgw", False), ("hctest", True), ("hctest", False)])
def test_host_sampling_equals_device_sampler(kind, norm):
    from icrl_amd import utils
    agent = _agent(kind)
    n_ep = 4 if kind in _EARLY_END else 2
    d_env, h_env = _eval_env(_IDS[kind][0], norm), _eval_env(_IDS[kind][1], norm)
    noise = _noise(kind, agent, d_env, n_ep)
    ref = _np(utils.sample_from_agent(agent, d_env, n_ep, noise=noise, parallel=False))
    run = utils._run_episodes(agent, h_env, n_ep, False, noise, False)
    assert isinstance(run, utils.HostEpisodeRun)
    got = _np(utils.sample_result(run))
    print(kind, norm, "lengths", got[4], "ep_rewards", got[3])
    _assert_same_result(got, ref, kind)
    assert got[0].shape[0] == got[4].sum()
    if kind == "hctest":      # early ends at different steps; the later episodes started from auto-reset observations
        assert got[4].max() < d_env.unwrapped.max_steps and len(set(got[4].tolist())) > 1, got[4]
    elif kind == "clgw":
        assert got[4].max() < d_env.unwrapped.max_steps and got[4].max() > 1, got[4]
    else:
        assert list(got[4]) == [d_env.unwrapped.max_steps] * n_ep
    if norm:
        assert not np.array_equal(got[0], got[1])
    else:
        assert np.array_equal(got[0], got[1])
    # sample_from_agent itself takes the same route
    h2 = _eval_env(_IDS[kind][1], norm)
    _assert_same_result(_np(utils.sample_from_agent(agent, h2, n_ep, noise=noise)), ref, kind)


# ---- 2. host path == per-step loop, and the chain state afterwards ----------------------------------------------------------------
def _shared_bottom_chains(seed=5):
    """one 1-env host env under BOTH a frozen evaluation chain and a training chain with a constraint net, and an agent over the latter."""
    from icrl_amd import envs
    from icrl_amd.ppo_lag import PPOLagrangian
    from icrl_amd.vec_env import DummyVecEnv, VecCostWrapper, VecNormalizeWithCost
    bottom = DummyVecEnv([envs.spec("HostHCWithPosTest-v0")])
    bottom.seed(seed)
    train = VecNormalizeWithCost(VecCostWrapper(bottom))
    cn = _cost_net(18, 6)
    train.set_cost_function(cn.cost_function)
    ev = VecNormalizeWithCost(bottom, training=False, norm_reward=False, norm_cost=False)
    rng = np.random.RandomState(11)
    ev.obs_rms.assign(0.3 * rng.randn(18), 0.5 + rng.rand(18), 100.0)
    agent = PPOLagrangian("TwoCriticsMlpPolicy", train, n_steps=16, seed=seed)
    return agent, train, ev, cn


def test_host_path_equals_stepped_path_and_leaves_the_same_chain():
    from icrl_amd import utils
    from icrl_amd.vec_env import dynamics_matrix
    n_ep, T = 3, 16
    sides = []
    for cls in (utils.HostEpisodeRun, utils.SteppedEpisodeRun):
        agent, train, ev, cn = _shared_bottom_chains()
        sd = agent.policy.state_dict()
        sd["action_net.bias"] = torch.as_tensor(-0.5 * np.sign(dynamics_matrix("hc")[0]), dtype=torch.float32)
        agent.policy.load_state_dict(sd)
        agent._setup_learn(2 * T)
        sides.append((cls, agent, train, ev))
    rows = n_ep * 1000
    noise = [np.random.RandomState(s).randn(rows, 6).astype(np.float32) for s in (0, 1)]
    rnoise = torch.as_tensor(np.random.RandomState(2).randn(T, 1, 6).astype(np.float32), device="cuda")
    out = []
    for cls, agent, train, ev in sides:
        res = []
        assert utils.host_episodes_ok(agent, ev)
        run = cls(agent, ev, n_ep, False, noise[0])
        res.append(_np(utils.sample_result(run)))
        henv = ev.unwrapped
        state = dict(s=henv.s.clone(), old_obs=ev.get_original_obs(), old_reward=ev.get_original_reward(), ret=ev.ret.clone(),
                     cost_ret=ev.cost_ret.clone(), training=ev.training)
        # a second run on the chain the first one left (through the class again), then a rollout on the train chain over the same env
        res.append(_np(utils.sample_result(cls(agent, ev, n_ep, False, noise[1]))))
        agent.collect_rollouts(train, None, agent.rollout_buffer, T, "cost", noise=rnoise)
        buf = {k: getattr(agent.rollout_buffer, k).cpu().numpy().copy() for k in ("observations", "orig_observations", "new_observations",
                                                                                  "actions", "rewards", "costs", "orig_costs", "dones")}
        out.append((res, state, buf, henv.s.clone()))
    (h_res, h_state, h_buf, h_s), (s_res, s_state, s_buf, s_s) = out
    _assert_same_result(h_res[0], s_res[0], "first run")
    assert len(set(h_res[0][4].tolist())) > 1 and h_res[0][4].max() < 1000
    for k in ("s", "old_obs", "old_reward", "ret", "cost_ret"):
        assert h_state[k].shape == s_state[k].shape and torch.equal(h_state[k], s_state[k]), k
    assert h_state["training"] is False and s_state["training"] is False
    _assert_same_result(h_res[1], s_res[1], "second run")
    for k in h_buf:
        assert np.array_equal(h_buf[k], s_buf[k]), k
    assert torch.equal(h_s, s_s)


def test_training_flag_is_restored_on_a_training_chain():
    """sampling over a chain whose normaliser is training: statistics frozen for the run and untouched by it, the flag restored."""
    from icrl_amd import utils
    agent, train, ev, cn = _shared_bottom_chains()
    ev.training = True
    before = (ev.obs_rms.mean, ev.obs_rms.var, ev.obs_rms.count, ev.ret_rms.mean, ev.ret_rms.var, ev.ret_rms.count)
    run = utils._run_episodes(agent, ev, 1, True, None, False)
    assert isinstance(run, utils.HostEpisodeRun) and ev.training is True
    after = (ev.obs_rms.mean, ev.obs_rms.var, ev.obs_rms.count, ev.ret_rms.mean, ev.ret_rms.var, ev.ret_rms.count)
    for b, a in zip(before, after):
        assert np.array_equal(np.asarray(b), np.asarray(a))


# ---- 3. evaluate_policy -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hctest", "clgw", "hc"])
def test_evaluate_policy_deterministic_equals_device_env(kind):
    from icrl_amd import utils
    agent = _agent(kind)
    n_ep = 2 if kind == "hc" else 6
    d_env, h_env = _eval_env(_IDS[kind][0]), _eval_env(_IDS[kind][1])
    d_mean, d_std = utils.evaluate_policy(agent, d_env, n_ep, deterministic=True)
    h_mean, h_std = utils.evaluate_policy(agent, h_env, n_ep, deterministic=True)
    print(kind, "mean", h_mean, d_mean, "std", h_std, d_std)
    assert h_mean == d_mean and h_std == d_std
    d_r, d_l = utils.evaluate_policy(agent, d_env, n_ep, deterministic=True, return_episode_rewards=True)
    h_r, h_l = utils.evaluate_policy(agent, h_env, n_ep, deterministic=True, return_episode_rewards=True)
    assert list(h_l) == list(d_l) and list(h_r) == list(d_r)
    if kind == "hctest":
        assert max(h_l) < 1000


# ---- 4. dispatch --------------------------------------------------------------------------------------------------------------------
def test_dispatch_served_switch_and_generic_shape(monkeypatch):
    """a served chain: HostEpisodeRun; the same chain with ICRL_HOST_EPISODES_STEPPED=1: SteppedEpisodeRun, same rows.  A generic-shape
    policy: SteppedEpisodeRun — the parent's route, whose rows are the device sampler's for that policy (the generic-shape sampler
    equals the per-step loop, tests/test_icrl_loop_gpu.py) — so every route returns the rows of the device env."""
    from icrl_amd import utils
    kind, n_ep = "hctest", 3
    agent = _agent(kind)
    noise = _noise(kind, agent, _eval_env(_IDS[kind][0]), n_ep)
    ref = _np(utils.sample_from_agent(agent, _eval_env(_IDS[kind][0]), n_ep, noise=noise, parallel=False))
    monkeypatch.delenv("ICRL_HOST_EPISODES_STEPPED", raising=False)
    run = utils._run_episodes(agent, _eval_env(_IDS[kind][1]), n_ep, False, noise, False)
    assert isinstance(run, utils.HostEpisodeRun)
    _assert_same_result(_np(utils.sample_result(run)), ref, "served")
    monkeypatch.setenv("ICRL_HOST_EPISODES_STEPPED", "1")
    run = utils._run_episodes(agent, _eval_env(_IDS[kind][1]), n_ep, False, noise, False)
    assert isinstance(run, utils.SteppedEpisodeRun)
    _assert_same_result(_np(utils.sample_result(run)), ref, "switch")
    monkeypatch.delenv("ICRL_HOST_EPISODES_STEPPED")
    wide = _agent(kind, policy_kwargs=_WIDE)
    assert wide.policy.wide and not utils.host_episodes_ok(wide, _eval_env(_IDS[kind][1]))
    wref = _np(utils.sample_from_agent(wide, _eval_env(_IDS[kind][0]), n_ep, noise=noise, parallel=False))
    run = utils._run_episodes(wide, _eval_env(_IDS[kind][1]), n_ep, False, noise, False)
    assert isinstance(run, utils.SteppedEpisodeRun)
    _assert_same_result(_np(utils.sample_result(run)), wref, "generic shape")


def test_missing_episode_limit_is_still_refused():
    from icrl_amd import utils
    agent = _agent("hc")
    env = _eval_env("HostHCWithPos-v0")
    env.unwrapped.max_steps = None
    with pytest.raises(ValueError, match="max_episode_steps"):
        utils.sample_from_agent(agent, env, 1)


# ---- 5. one launch per step -----------------------------------------------------------------------------------------------------------
class _Calls:
    """counts the calls of icrl_host_episode_step (the ctypes function, wrapped) and of every step_wait of the chain's classes."""

    def __init__(self, monkeypatch):
        from icrl_amd import _lib, vec_env
        self.launches, self.step_waits = 0, 0
        lib = _lib.lib()
        fn = lib.icrl_host_episode_step

        def counted(*a):
            self.launches += 1
            return fn(*a)
        monkeypatch.setattr(lib, "icrl_host_episode_step", counted)
        for cls in (vec_env.VecNormalize, vec_env.VecCostWrapper, vec_env.HostVecEnv):
            orig = cls.step_wait

            def step_wait(this, _orig=orig):
                self.step_waits += 1
                return _orig(this)
            monkeypatch.setattr(cls, "step_wait", step_wait)


@pytest.mark.parametrize("kind", ["hctest", "lgw"])
def test_one_launch_per_env_step_and_no_wrapper_step(kind, monkeypatch):
    from icrl_amd import utils
    agent = _agent(kind)
    n_ep = 3
    env = _eval_env(_IDS[kind][1])
    noise = _noise(kind, agent, env, n_ep)
    calls = _Calls(monkeypatch)
    run = utils._run_episodes(agent, env, n_ep, False, noise, False)
    total = int(run.lengths.sum())
    assert isinstance(run, utils.HostEpisodeRun)
    assert calls.launches == total + 1, (calls.launches, total)
    assert calls.step_waits == 0
    assert len(env.unwrapped.envs[0].actions) == total            # the env was stepped once per recorded row
    got = np.stack([np.asarray(a, np.float64).reshape(-1) for a in env.unwrapped.envs[0].actions])
    assert np.array_equal(got, run.rows_of("actions").cpu().numpy().astype(np.float64))      # ... with the clipped action of that row


def test_cost_wrapper_chain_with_a_constraint_net_is_served(monkeypatch):
    """cpg's evaluation env (use_cost_wrapper=True, a ConstraintNet's cost function): served, its forward skipped; the rows of the chain
    without the wrapper, and previous_obs / the normaliser's last observation as the per-step loop leaves them."""
    from icrl_amd import utils
    kind, n_ep = "hctest", 3
    agent = _agent(kind)
    cn = _cost_net(18, 6)
    noise = _noise(kind, agent, _eval_env(_IDS[kind][1]), n_ep)
    plain = _np(utils.sample_result(utils._run_episodes(agent, _eval_env(_IDS[kind][1]), n_ep, False, noise, False)))
    env_h, env_s = (_eval_env(_IDS[kind][1], cost_wrapper=True) for _ in range(2))
    for e in (env_h, env_s):
        e.set_cost_function(cn.cost_function)
        assert e.venv.constraint_net() is cn
    stepped = utils.SteppedEpisodeRun(agent, env_s, n_ep, False, noise)
    forwards = []
    monkeypatch.setattr(cn, "cost_function_device", lambda *a, **k: forwards.append(1))
    calls = _Calls(monkeypatch)
    run = utils._run_episodes(agent, env_h, n_ep, False, noise, False)
    assert isinstance(run, utils.HostEpisodeRun) and calls.step_waits == 0 and not forwards
    assert calls.launches == int(run.lengths.sum()) + 1
    _assert_same_result(_np(utils.sample_result(run)), plain, "with the cost wrapper")
    _assert_same_result(_np(utils.sample_result(run)), _np(utils.sample_result(stepped)), "per-step loop")
    assert env_h.venv.previous_obs.shape == env_s.venv.previous_obs.shape and torch.equal(env_h.venv.previous_obs, env_s.venv.previous_obs)
    assert torch.equal(env_h.get_original_obs(), env_s.get_original_obs())
    assert torch.equal(env_h.unwrapped.s, env_s.unwrapped.s)
    assert torch.equal(env_h.venv.actions, env_s.venv.actions)
    assert torch.equal(env_h.ret, env_s.ret) and torch.equal(env_h.cost_ret, env_s.cost_ret)
    # a cost wrapper that was never given a cost function is served as well
    bare = _eval_env(_IDS[kind][1], cost_wrapper=True)
    assert bare.venv.cost_function is None
    run = utils._run_episodes(agent, bare, n_ep, False, noise, False)
    assert isinstance(run, utils.HostEpisodeRun)
    _assert_same_result(_np(utils.sample_result(run)), plain, "cost wrapper without a cost function")


def test_python_cost_callable_takes_the_per_step_loop():
    from icrl_amd import utils
    kind, n_ep = "hctest", 2
    agent = _agent(kind)
    seen = []

    def cost(obs, acs):
        seen.append((obs.shape, acs.shape))
        return np.zeros(obs.shape[0], np.float32)
    env = _eval_env(_IDS[kind][1], cost_wrapper=True)
    env.set_cost_function(cost)
    noise = _noise(kind, agent, env, n_ep)
    assert not utils.host_episodes_ok(agent, env)
    run = utils._run_episodes(agent, env, n_ep, False, noise, False)
    assert isinstance(run, utils.SteppedEpisodeRun)
    assert len(seen) == int(run.lengths.sum())
    ref = _np(utils.sample_result(utils._run_episodes(agent, _eval_env(_IDS[kind][1]), n_ep, False, noise, False)))
    _assert_same_result(_np(utils.sample_result(run)), ref, "callable")


# ---- 6. argument errors (host-side checks; nothing is launched) ---------------------------------------------------------------------
def _raw_call(agent, env, num_envs=1, pol=None, act_host=None, k=0, act=1, rows=8):
    from icrl_amd import _lib
    from icrl_amd.structs import HostEpisodeT, p
    henv = env.unwrapped
    O, A = henv.obs_dim, agent.policy.act_dim
    st = henv.staging()
    out = dict(orig_obs=torch.full((rows, O), -7.0, dtype=torch.float64, device="cuda"), obs=torch.full((rows, O), -7.0, dtype=torch.float64, device="cuda"),
               actions=torch.full((rows, A), -7.0, device="cuda"))
    st["act"].fill_(-7.0)
    noise = torch.zeros(rows, A, device="cuda")
    he = HostEpisodeT(num_envs, O, rows, 0, p(st["dev"]), st["act"].data_ptr() if act_host is None else act_host, p(out["orig_obs"]),
                      p(out["obs"]), p(out["actions"]))
    was = env.training
    env.training = False
    nm = env.struct()
    env.training = was
    ps = (pol or agent.policy).struct()
    lib, b = _lib.lib(), _lib.byref
    err = lib.icrl_host_episode_step(b(nm), b(ps), b(he), p(noise), None, None, k, act, _lib.current_stream())
    torch.cuda.synchronize()
    untouched = all(bool((t == -7.0).all()) for t in out.values()) and bool((st["act"] == -7.0).all())
    return err, untouched


@pytest.mark.parametrize("case", ["two_envs", "generic_shape", "unpinned", "row", "null"])
def test_argument_errors_are_refused_with_a_message(case):
    from icrl_amd import _lib
    agent = _agent("hc")
    env = _eval_env("HostHCWithPos-v0")
    keep = ctypes.create_string_buffer(64)          # ordinary host memory: not page-locked
    if case == "two_envs":
        err, untouched = _raw_call(agent, env, num_envs=2)
        words = ("icrl_host_episode_step", "2 envs", "per-step loop")
    elif case == "generic_shape":
        err, untouched = _raw_call(agent, env, pol=_agent("hc", policy_kwargs=_WIDE).policy)
        words = ("icrl_host_episode_step", "per-step")
    elif case == "unpinned":
        err, untouched = _raw_call(agent, env, act_host=ctypes.addressof(keep))
        words = ("icrl_host_episode_step", "page-locked")
    elif case == "row":
        err, untouched = _raw_call(agent, env, k=8, act=1, rows=8)        # the launch after the last row must not act
        words = ("icrl_host_episode_step", "k = 8")
    else:
        err = _lib.lib().icrl_host_episode_step(None, None, None, None, None, None, 0, 1, _lib.current_stream())
        untouched, words = True, ("icrl_host_episode_step", "NULL descriptor")
    assert err == 1 and untouched
    with pytest.raises(ValueError) as e:
        _lib.check(err, "icrl_host_episode_step")
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_raw_call_launches_when_the_arguments_are_fine():
    """the counterpart of the refusals above: the same call with good arguments does launch and does write."""
    agent = _agent("hc")
    env = _eval_env("HostHCWithPos-v0")
    err, untouched = _raw_call(agent, env)
    assert err == 0 and not untouched


# ---- 7. SubprocVecEnv -----------------------------------------------------------------------------------------------------------------
def test_subproc_vec_env_equals_dummy_vec_env():
    from icrl_amd import envs, utils
    from icrl_amd.vec_env import DummyVecEnv, SubprocVecEnv, VecNormalizeWithCost
    kind, n_ep = "hctest", 3
    agent = _agent(kind)
    res = []
    for cls in (DummyVecEnv, SubprocVecEnv):
        bottom = cls([envs.spec(_IDS[kind][1])])
        bottom.seed(3)
        env = VecNormalizeWithCost(bottom, training=False, norm_reward=False, norm_cost=False)
        rng = np.random.RandomState(11)
        env.obs_rms.assign(0.3 * rng.randn(18), 0.5 + rng.rand(18), 100.0)
        noise = _noise(kind, agent, env, n_ep)
        run = utils._run_episodes(agent, env, n_ep, False, noise, False)
        assert isinstance(run, utils.HostEpisodeRun)
        res.append(_np(utils.sample_result(run)))
        bottom.close()
    _assert_same_result(res[1], res[0], "SubprocVecEnv")
