"""GPU: training-episode statistics (rollout/ep_rew_mean, rollout/ep_len_mean) — the raw-reward plane every rollout kernel form writes,
icrl_monitor_scan, the window the host reads, learn()'s semantics, and that nothing moves while the feature is switched off.

The truth of the kernel-form cases is an independent restatement: a twin env stepped from Python with the clipped actions of the fused
rollout (host envs: the envs' own rewards and dones, recorded by the test), fed into a plain-Python Monitor.  Everything is compared
bit for bit."""
import os
import types
from collections import deque

import numpy as np
import pytest
import torch

from helpers import routes

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("rollout/ep_rew_mean", "rollout/ep_len_mean")
LIMIT = 37          # shortened episode limit of the device envs


def _seq_sum(xs):
    """`sum(self.rewards)` of the reference's Monitor (monitor.py:107) on the interpreter it was written for: a sequential sum from the
    integer 0 (interpreters from 3.12 on compensate float sums inside sum(); the episode return the reference logged is the plain one)."""
    s = 0
    for x in xs:
        s = s + x
    return s


class PyMonitor:
    """monitor.py:100-122 + base_class.py:383-387 for N envs: per env a list of rewards; on done an {"r", "l"} record into a
    deque(maxlen=100), envs in index order within a step."""

    def __init__(self, n):
        self.rewards = [[] for _ in range(n)]
        self.buf = deque(maxlen=100)
        self.total = 0
        self.partial_steps = 0      # steps that ended several, but not all envs

    def step(self, rew, done, record=True):
        for n, (r, d) in enumerate(zip(rew, done)):
            self.rewards[n].append(float(r))
            if d:
                if record:
                    self.buf.append((round(float(_seq_sum(self.rewards[n])), 6), len(self.rewards[n])))
                    self.total += 1
                self.rewards[n] = []
        k = int(np.sum(done))
        self.partial_steps += int(1 < k < len(done))

    def records(self):
        return [r for r, _ in self.buf], [l for _, l in self.buf]


def _logged(agent):
    from icrl_amd import logger
    logger.configure()
    agent.start_time = agent.start_time or 1.0
    agent._training_infos(1)
    return dict(logger.Logger.CURRENT.name_to_value)


def _check_against(agent, mon, N, straddle=True):
    """window, logged means and carries of `agent` against the plain-Python monitor, after the preconditions on the truth side."""
    rs, ls = mon.records()
    assert mon.total >= 1, "no episode ended inside the test"
    if N > 1:
        assert mon.partial_steps >= 1, "no step ended several but not all envs: the within-step order would not show"
    if N >= 64:
        assert mon.total > 100, f"only {mon.total} episodes: the ring did not wrap"
    if straddle:
        assert any(len(r) > 0 for r in mon.rewards), "no episode in progress at the end"
    got_r, got_l = agent.episode_window()
    assert got_l == ls
    assert got_r == rs
    m = _logged(agent)
    assert m[KEYS[0]] == np.mean(rs) and m[KEYS[1]] == np.mean(ls)
    ep_ret, ep_len = agent._mon["ep_ret"].cpu().numpy(), agent._mon["ep_len"].cpu().numpy()
    assert ep_len.tolist() == [len(r) for r in mon.rewards]
    want = np.array([float(_seq_sum(r)) if r else 0.0 for r in mon.rewards])
    assert np.array_equal(ep_ret, want), np.abs(ep_ret - want).max()
    assert int(agent._mon["win_state"][0].item()) == mon.total


# ---------------------------------------------------------------------------------------------------------------------------------
# device envs: every kernel form
# ---------------------------------------------------------------------------------------------------------------------------------
def _device_agent(N, T, kind, seed, episode_stats=True, policy_kwargs=None, cn_hid=None, **akw):
    from icrl_amd.constraint_net import ConstraintNet
    from icrl_amd.ppo_lag import PPOLagrangian
    from icrl_amd.vec_env import HipSynthVecEnv, VecCostWrapper, VecNormalizeWithCost
    torch.manual_seed(seed)
    disc = kind in ("lgw", "clgw")
    norm = not disc
    env = VecNormalizeWithCost(VecCostWrapper(HipSynthVecEnv(N, kind, seed)), norm_obs=norm, norm_reward=norm, norm_cost=norm)
    if disc:
        cn = ConstraintNet(1, 2, cn_hid or [20], None, lambda x: 0.003, None, None, True, clip_obs=20)
    else:
        od, ad = (18, 6) if kind == "hc" else (113, 8)
        lo = -np.ones(ad, np.float32)
        cn = ConstraintNet(od, ad, cn_hid or ([20] if kind == "hc" else [40, 40]), None, lambda x: 0.05, None, None, False, 0.5, clip_obs=20,
                           action_low=lo, action_high=-lo)
    env.set_cost_function(cn.cost_function)
    kw = dict(policy_kwargs=policy_kwargs) if policy_kwargs else {}
    agent = PPOLagrangian("TwoCriticsMlpPolicy", env, n_steps=T, seed=seed, episode_stats=episode_stats, **kw, **akw)
    return agent, env, cn


def _phases(N):
    """where in their (shortened) episodes the envs start: groups of envs share a phase, so some steps end several but not all envs."""
    return torch.as_tensor([(3 * (n % 4) + 11 * ((n // 8) % 3)) % LIMIT for n in range(N)], dtype=torch.int32, device="cuda")


def _twin(N, kind, seed):
    from icrl_amd.vec_env import HipSynthVecEnv
    twin = HipSynthVecEnv(N, kind, seed)
    twin.max_steps = LIMIT
    twin.reset()
    twin.t_ep.copy_(_phases(N))
    return twin


def _start(agent, env, N, T, rollouts=3):
    env.unwrapped.max_steps = LIMIT
    agent._setup_learn(rollouts * N * T)
    env.unwrapped.t_ep.copy_(_phases(N))


def _noise(kind, N, T, rollouts, seed=8):
    rng = np.random.RandomState(seed)
    if kind in ("lgw", "clgw"):
        return torch.as_tensor(rng.rand(rollouts, T, N).astype(np.float32), device="cuda")
    return torch.as_tensor(rng.randn(rollouts, T, N, 6 if kind == "hc" else 8).astype(np.float32), device="cuda")


def _twin_rows(twin, agent, rows):
    """step the twin with the clipped rows of the rollout's actions plane: raw rewards [rows, N] float64, dones [rows, N]."""
    acts = agent.rollout_buffer.actions[:rows]
    if agent._alow is not None:
        acts = torch.max(torch.min(acts, agent._ahigh), agent._alow)
    rew, done = [], []
    for t in range(rows):
        _, r, d, _ = twin.step(acts[t])
        rew.append(r.cpu().numpy().copy()); done.append(d.cpu().numpy().astype(bool))
    return np.stack(rew), np.stack(done)


def _feed(mon, agent, rew, done, rows, unrecorded=None):
    """plane and done flags of the rollout against the truth, then the truth into the plain-Python monitor."""
    plane = agent._mon["raw_rewards"].cpu().numpy()
    assert np.array_equal(plane[:rows], rew[:rows])
    for t in range(rows):
        mon.step(rew[t], done[t])
    if unrecorded is not None:
        mon.step(rew[unrecorded], done[unrecorded], record=False)


CASES = {
    # id: (N, T, kind, rollout_kernel, agent kwargs, constraint-net hidden sizes)
    "persistent-hc-1": (1, 64, "hc", None, {}, None),
    "persistent-hc-7": (7, 64, "hc", None, {}, None),
    "persistent-hc-64": (64, 128, "hc", None, {}, None),
    "wide-hc-128": (128, 64, "hc", None, {}, None),      # (more than 96 envs: the column-partitioned kernel without being asked for)
    "steps-hc-16": (16, 64, "hc", "steps", {}, None),
    "wide-ant-256": (256, 32, "ant", "wide", {}, None),
    "multi-hc-64": (64, 128, "hc", "multi", {}, None),
    "multi-hc-2048": (2048, 32, "hc", "multi", {}, None),
    "generic-policy-hc-12": (12, 64, "hc", None, dict(policy_kwargs=dict(net_arch=[dict(pi=[128, 96], vf=[80, 128], cvf=[128, 128])])), None),
    "wide-cn-hc-12": (12, 64, "hc", None, {}, [128, 128]),
    "lgw-6": (6, 64, "lgw", None, {}, None),
    "clgw-6": (6, 64, "clgw", None, {}, None),
}


# what icrl_rollout_collect_ex_mon must have launched for each form (helpers/routes.py); every one-launch form is the instantiation that
# stores the raw-reward plane
ROUTES = {"persistent-hc-1": "persistent", "persistent-hc-7": "persistent", "persistent-hc-64": "persistent", "wide-hc-128": "wide",
          "steps-hc-16": "per-step", "wide-ant-256": "wide", "multi-hc-64": "multi", "multi-hc-2048": "multi",
          "generic-policy-hc-12": "generic-persistent", "wide-cn-hc-12": "generic-per-step", "lgw-6": "persistent", "clgw-6": "persistent"}


@pytest.mark.parametrize("case", list(CASES))
def test_kernel_form_against_python_monitor(case):
    N, T, kind, kernel, akw, cn_hid = CASES[case]
    seed = 7
    agent, env, cn = _device_agent(N, T, kind, seed, cn_hid=cn_hid, **akw)
    if kernel is not None:
        agent.rollout_kernel = kernel
    if case == "generic-policy-hc-12":
        assert agent.policy.wide
    if case == "wide-cn-hc-12":
        assert cn.wide
    assert agent._fused_chain() is not None
    _start(agent, env, N, T)
    twin = _twin(N, kind, seed)
    noise = _noise(kind, N, T, 3)
    mon = PyMonitor(N)
    ended_inside = 0
    for it in range(3):
        assert agent.collect_rollouts(env, None, agent.rollout_buffer, T, "cost", noise=noise[it]) is True
        got = routes.check_rollout(ROUTES[case], case)
        assert bool(got["pick"] & routes.PICK_MON) == (not ROUTES[case].endswith("per-step"))
        agent.check_rollout_status()
        rew, done = _twin_rows(twin, agent, T)
        # the buffer's own done flags are the twin's (row t + 1 = step t; last_dones = the last step)
        assert np.array_equal(agent.rollout_buffer.dones.cpu().numpy()[1:] != 0, done[:-1])
        assert np.array_equal(agent._ag["last_dones"].cpu().numpy() != 0, done[-1])
        ended_inside += int(done[1:-1].any())
        _feed(mon, agent, rew, done, T)
    assert ended_inside == 3, "episodes must end inside every rollout"
    assert min(_phases(N).tolist()) + 3 * T > LIMIT and (3 * T) % LIMIT != 0      # episodes straddle the rollout boundaries
    _check_against(agent, mon, N)


def test_seed_batch_entry_point_against_python_monitor():
    """three runs through icrl_rollout_collect_batch_mon (one descriptor per run), as seed_batch.SeedBatch launches them."""
    from icrl_amd import _lib
    from icrl_amd.seed_batch import SeedBatch
    N, T, S = 8, 64, 3
    runs = [_device_agent(N, T, "hc", 20 + r) for r in range(S)]
    sb = SeedBatch.__new__(SeedBatch)
    sb.args_ws = torch.empty(2 * S * _lib.BATCH_ARGS_BYTES, dtype=torch.uint8, device="cuda")
    twins, mons = [], [PyMonitor(N) for _ in range(S)]
    for r, (agent, env, _) in enumerate(runs):
        _start(agent, env, N, T)
        twins.append(_twin(N, "hc", 20 + r))
    noise = [_noise("hc", N, T, 3, seed=30 + r) for r in range(S)]
    agents = [a for a, _, _ in runs]
    for it in range(3):
        jobs = [a._rollout_begin(None, a.rollout_buffer, T, noise[r][it]) for r, a in enumerate(agents)]
        sb._launch_rollouts(agents, jobs)
        # 3 x 8 envs: ONE launch of the one-workgroup-per-env batch kernel, the instantiation that stores the raw-reward plane
        got = routes.check_rollout(dict(route="persistent-batch", n_runs=S, wgs=N, launches=1, minw=1), "3 x 8 with monitors")
        assert got["pick"] & _lib.PICK_MON
        for r, (a, env, _) in enumerate(runs):
            a._rollout_end(jobs[r], env, None, a.rollout_buffer, T)
            a.check_rollout_status()
            rew, done = _twin_rows(twins[r], a, T)
            _feed(mons[r], a, rew, done, T)
    for r, a in enumerate(agents):
        _check_against(a, mons[r], N)
    assert len({tuple(a.episode_window()[0]) for a in agents}) == S      # every run has its own records


def _null_cost(obs, acs):
    return np.zeros(obs.shape[0], np.float32)


def test_stepped_path_with_a_callable_cost():
    N, T, seed = 6, 64, 9
    agent, env, _ = _device_agent(N, T, "hc", seed)
    _start(agent, env, N, T)
    twin = _twin(N, "hc", seed)
    noise = _noise("hc", N, T, 3)
    mon = PyMonitor(N)
    for it in range(3):
        assert not agent._fused_rollout_ok(_null_cost, T, agent.rollout_buffer)
        assert agent.collect_rollouts(env, None, agent.rollout_buffer, T, _null_cost, noise=noise[it]) is True
        rew, done = _twin_rows(twin, agent, T)
        _feed(mon, agent, rew, done, T)
    _check_against(agent, mon, N)


class _StopAfter:
    """a callback whose on_step() returns False at its k-th call (k = 1, 2, ...)."""

    def __init__(self, k):
        self.k, self.calls = k, 0

    def on_rollout_start(self):
        self.calls = 0

    def on_step(self):
        self.calls += 1
        return self.calls < self.k

    def on_rollout_end(self):
        pass


def test_stepped_rollout_that_a_callback_ends_early():
    """on_step() returns False at step k (0-based k = 40 of T = 64): steps 0 .. k - 1 are recorded, step k was made by the envs — the
    reference's Monitor has its reward and has started a new episode where it ended one — but never reached ep_info_buffer
    (on_policy_algorithm.py:400-403)."""
    N, T, seed, k = 6, 64, 9, 40
    agent, env, _ = _device_agent(N, T, "hc", seed)
    _start(agent, env, N, T)
    twin = _twin(N, "hc", seed)
    noise = _noise("hc", N, T, 3)
    mon = PyMonitor(N)
    for it in range(2):
        assert agent._collect_rollouts_stepped(env, None, agent.rollout_buffer, T, "cost", noise=noise[it]) is True
        rew, done = _twin_rows(twin, agent, T)
        _feed(mon, agent, rew, done, T)
    before = mon.total
    assert agent._collect_rollouts_stepped(env, _StopAfter(k + 1), agent.rollout_buffer, T, "cost", noise=noise[2]) is False
    # rows 0 .. k - 1 are in the buffer; the action of step k is what the policy drew on noise row k from the observation after step k - 1
    rew, done = _twin_rows(twin, agent, k)
    last = agent.policy.last_clipped
    _, r_k, d_k, _ = twin.step(last)
    rew = np.concatenate([rew, r_k.cpu().numpy()[None]]); done = np.concatenate([done, d_k.cpu().numpy().astype(bool)[None]])
    _feed(mon, agent, rew, done, k, unrecorded=k)
    assert mon.total > before
    _check_against(agent, mon, N, straddle=False)


# ---------------------------------------------------------------------------------------------------------------------------------
# host envs: the launch-per-step path
# ---------------------------------------------------------------------------------------------------------------------------------
def _host_agent(N, T, seed, subproc, episode_stats=True):
    from helpers import short_host_envs  # noqa: F401  (registers HostShortEpisodes-v0)
    from icrl_amd import envs
    from icrl_amd.constraint_net import ConstraintNet
    from icrl_amd.ppo_lag import PPOLagrangian
    from icrl_amd.vec_env import DummyVecEnv, SubprocVecEnv, VecCostWrapper, VecNormalizeWithCost
    import tests.helpers.short_host_envs  # noqa: F401  (the name the worker processes import)
    bottom = (SubprocVecEnv if subproc else DummyVecEnv)([envs.spec("HostShortEpisodes-v0")] * N)
    env = VecNormalizeWithCost(VecCostWrapper(bottom))
    torch.manual_seed(seed)
    lo = -np.ones(2, np.float32)
    cn = ConstraintNet(3, 2, [20], None, lambda x: 0.05, None, None, False, 0.5, clip_obs=20, action_low=lo, action_high=-lo)
    env.set_cost_function(cn.cost_function)
    agent = PPOLagrangian("TwoCriticsMlpPolicy", env, n_steps=T, seed=seed, episode_stats=episode_stats)
    return agent, env, bottom


@pytest.mark.parametrize("subproc", [False, True], ids=["dummy", "subproc"])
def test_host_path_against_python_monitor(subproc):
    """truth = the host envs' own rewards and dones, recorded where the rollout receives them."""
    N, T, seed = 9, 48, 4
    agent, env, bottom = _host_agent(N, T, seed, subproc)
    try:
        seen = []
        inner = bottom.step_host

        def recording(actions):
            obs, rew, done, infos = inner(actions)
            seen.append((np.array(rew, np.float64, copy=True), np.array(done, bool, copy=True)))
            return obs, rew, done, infos
        bottom.step_host = recording
        agent._setup_learn(3 * N * T)
        rng = np.random.RandomState(3)
        mon = PyMonitor(N)
        for it in range(3):
            assert agent._host_rollout_ok("cost", T, agent.rollout_buffer)
            del seen[:]
            noise = torch.as_tensor(rng.randn(T, N, 2).astype(np.float32), device="cuda")
            assert agent.collect_rollouts(env, None, agent.rollout_buffer, T, "cost", noise=noise) is True
            assert len(seen) == T
            rew, done = np.stack([s[0] for s in seen]), np.stack([s[1] for s in seen])
            assert done[1:-1].any()
            _feed(mon, agent, rew, done, T)
        _check_against(agent, mon, N)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# against the reference's own numbers (g8)
# ---------------------------------------------------------------------------------------------------------------------------------
def test_icrl_lgw_three_iterations_episode_stats_vs_reference(golden):
    """the setup of test_icrl_trajectory_gpu.test_icrl_lgw_three_iterations_vs_reference with episode_stats on: the two keys equal
    what the reference logged (each learn() finishes four episodes of 200 steps, whole-number rewards, a mean of four values)."""
    from icrl_amd.icrl import build_parser, setup, outer_iteration
    from oracle.streams import RecordedStreams
    g = golden("g8_icrl_lgw")
    expert = os.path.join(HERE, "golden/expert_lgw.npz")
    argv = [str(a) for a in g["argv"]] + ["-ep", expert, "--expert_agent_path", expert, "-v", "0"]
    argv[argv.index("-d") + 1] = "cuda"
    cfg = vars(build_parser().parse_args(argv))
    cfg.update(rank=0, world_size=1, streams=RecordedStreams(g), episode_stats=True)
    st = setup(types.SimpleNamespace(**cfg))
    sub = lambda prefix: {k[len(prefix):]: g[k] for k in g.files if k.startswith(prefix)}
    st["agent"].policy.load_state_dict(sub("w0/"))
    st["constraint_net"].load_state_dict(sub("cn0/"))
    names = [str(k) for k in g["metric_keys"]]
    assert set(KEYS) <= set(names)
    for it in range(3):
        m = outer_iteration(st, it)
        ref = dict(zip(names, g["metrics"][it]))
        for k in KEYS:
            print(it, k, m.get(k), ref[k])
            assert k in m, (it, k)
            assert float(m[k]) == float(ref[k]), (it, k, m[k], ref[k])


# ---------------------------------------------------------------------------------------------------------------------------------
# nothing existing moves
# ---------------------------------------------------------------------------------------------------------------------------------
_BUF_KEYS = ("observations", "orig_observations", "new_observations", "new_orig_observations", "actions", "rewards", "costs",
             "orig_costs", "dones", "log_probs", "reward_values", "cost_values", "reward_advantages", "cost_advantages",
             "reward_returns", "cost_returns")


def _assert_same_state(a_off, e_off, a_on, e_on):
    for k in _BUF_KEYS:
        assert torch.equal(getattr(a_off.rollout_buffer, k), getattr(a_on.rollout_buffer, k)), k
    for rms in ("obs_rms", "ret_rms", "cost_rms"):
        x, y = getattr(e_off, rms), getattr(e_on, rms)
        assert np.array_equal(np.asarray(x.mean), np.asarray(y.mean)) and np.array_equal(np.asarray(x.var), np.asarray(y.var)) and x.count == y.count, rms
    assert torch.equal(e_off.ret, e_on.ret) and torch.equal(e_off.cost_ret, e_on.cost_ret)
    assert torch.equal(a_off._last_obs, a_on._last_obs) and torch.equal(a_off._ag["last_dones"], a_on._ag["last_dones"])
    assert a_off.num_timesteps == a_on.num_timesteps
    assert torch.equal(a_off.policy.params, a_on.policy.params)


@pytest.mark.parametrize("form", ["persistent-hc-64", "wide-ant-256", "multi-hc-2048", "host"])
def test_switched_off_nothing_moves(form):
    """two identically built agents, one switched off and one on, same noise: two rollouts and one train() leave bit-identical buffers,
    normaliser statistics, agent state and parameters; switched off there is no plane and neither key is logged."""
    from icrl_amd import logger
    if form == "host":
        N, T = 6, 32
        (a_off, e_off, _), (a_on, e_on, _) = _host_agent(N, T, 4, False, episode_stats=False), _host_agent(N, T, 4, False, episode_stats=True)
        ad = 2
    else:
        N, T, kind, kernel, _, _ = CASES[form]
        T = min(T, 32)
        (a_off, e_off, _), (a_on, e_on, _) = _device_agent(N, T, kind, 5, episode_stats=False), _device_agent(N, T, kind, 5, episode_stats=True)
        a_off.rollout_kernel = a_on.rollout_kernel = kernel or "auto"
        ad = 6 if kind == "hc" else 8
    try:
        assert a_off._mon is None and a_off.episode_stats is False and a_on._mon is not None
        with pytest.raises(RuntimeError, match="episode statistics are off"):
            a_off.episode_window()
        noise = torch.as_tensor(np.random.RandomState(1).randn(2, T, N, ad).astype(np.float32), device="cuda")
        perms = np.stack([np.random.RandomState(2).permutation(N * T) for _ in range(a_off.n_epochs)])
        for a, e in ((a_off, e_off), (a_on, e_on)):
            if form != "host":
                e.unwrapped.max_steps = LIMIT
            a._setup_learn(2 * N * T)
            for it in range(2):
                a.collect_rollouts(e, None, a.rollout_buffer, T, "cost", noise=noise[it])
            a.train(perms=perms)
        _assert_same_state(a_off, e_off, a_on, e_on)
        m_off, m_on = _logged(a_off), _logged(a_on)
        assert not set(KEYS) & set(m_off)
        assert set(KEYS) <= set(m_on)
        assert {k: v for k, v in m_on.items() if k not in KEYS and not k.startswith("time/")} == {k: v for k, v in m_off.items() if not k.startswith("time/")}
    finally:
        e_off.close(); e_on.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# learn() semantics and the switches
# ---------------------------------------------------------------------------------------------------------------------------------
class _KeepLogs:
    """what every log dump of learn() held for the two keys."""

    def __init__(self):
        self.rows = []

    def __enter__(self):
        from icrl_amd import logger
        logger.configure()
        self._cur, self._dump = logger.Logger.CURRENT, logger.Logger.CURRENT.dump

        def dump(step=0):
            self.rows.append({k: self._cur.name_to_value[k] for k in KEYS if k in self._cur.name_to_value})
            self._dump(step)
        self._cur.dump = dump
        return self

    def __exit__(self, *exc):
        self._cur.dump = self._dump


def test_learn_window_and_carries():
    N, T = 4, 64
    agent, env, _ = _device_agent(N, T, "hc", 3, batch_size=64, n_epochs=1)
    env.unwrapped.max_steps = 50
    with _KeepLogs() as logs:
        agent.learn(2 * N * T)
    assert len(logs.rows) == 2
    # rollout 1: steps 0 .. 63 end one episode per env (50 steps); rollout 2: steps 64 .. 127 end the second (step 99)
    assert logs.rows[0][KEYS[1]] == 50.0 and logs.rows[1][KEYS[1]] == 50.0
    r1, l1 = agent.episode_window()
    assert l1 == [50] * (2 * N) and agent._mon["ep_len"].tolist() == [28] * N
    # a second learn() with the default reset_num_timesteps=True: the window and the carries start again (envs are reset)
    with _KeepLogs() as logs:
        agent.learn(N * T)
    r2, l2 = agent.episode_window()
    assert l2 == [50] * N and logs.rows[0][KEYS[1]] == 50.0 and logs.rows[0][KEYS[0]] == np.mean(r2)
    assert r2 != r1[:N]
    assert agent._mon["ep_len"].tolist() == [14] * N
    # reset_num_timesteps=False: both continue — the episodes in progress (14 steps in) end after 36 more steps
    carried = agent._mon["ep_ret"].clone()
    with _KeepLogs() as logs:
        agent.learn(N * T, reset_num_timesteps=False)
    r3, l3 = agent.episode_window()
    assert l3 == [50] * (2 * N) and r3[:N] == r2
    assert logs.rows[0][KEYS[0]] == np.mean(r3)
    assert agent._mon["ep_len"].tolist() == [28] * N and not torch.equal(carried, agent._mon["ep_ret"])


def test_nothing_is_logged_before_the_first_episode_has_ended():
    N, T = 4, 64
    agent, env, _ = _device_agent(N, T, "hc", 3, batch_size=64, n_epochs=1)      # limit 1000
    with _KeepLogs() as logs:
        agent.learn(2 * N * T)
    assert logs.rows == [{}, {}]
    assert agent.episode_window() == ([], [])
    assert agent._mon["ep_len"].tolist() == [2 * T] * N


def test_environment_switch_is_read_when_the_keyword_is_none(monkeypatch):
    monkeypatch.setenv("ICRL_EPISODE_STATS", "1")
    agent, _, _ = _device_agent(2, 8, "hc", 0, episode_stats=None)
    assert agent.episode_stats is True and agent._mon is not None
    agent, _, _ = _device_agent(2, 8, "hc", 0, episode_stats=False)      # the keyword wins
    assert agent._mon is None
    monkeypatch.setenv("ICRL_EPISODE_STATS", "0")
    assert _device_agent(2, 8, "hc", 0, episode_stats=None)[0]._mon is None
    monkeypatch.delenv("ICRL_EPISODE_STATS")
    assert _device_agent(2, 8, "hc", 0, episode_stats=None)[0]._mon is None
