"""GPU: the chained episode sampler (icrl_sample_episodes_chain) — the episodes of a sequential 1-env loop as
parallel streams whose positions are settled inside ONE launch — against the existing one-stream launch that runs the same episodes
back to back (icrl_sample_episodes, n_streams = 1, episodes_per_stream = n): every row, episode sum, length and the env's end state
must be bit-identical, whichever episodes end early.  HC shapes (obs 18, act 6, hidden 64), episodes of at most M = 48 steps."""
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

M = 48            # episode limit of the envs here (the kernels read env.max_steps)
N_EP = 6
CASES = {         # which episodes end early
    "a_none": [False] * N_EP,
    "b_first": [True] + [False] * (N_EP - 1),
    "c_several_and_last": [False, True, False, True, True, True],
    "d_all": [True] * N_EP,
}
_cache = {}


def _hc_agent():
    if "hc" not in _cache:
        from icrl_amd import utils
        from icrl_amd.constraint_net import ConstraintNet
        from icrl_amd.ppo_lag import PPOLagrangian
        train_env = utils.make_train_env("HCWithPos-v0", None, True, 5, 4, cost_info_str="cost", reward_gamma=0.99, cost_gamma=0.99)
        lo = -np.ones(6, np.float32)
        cn = ConstraintNet(18, 6, [20], None, lambda x: 0.05, None, None, False, clip_obs=20, action_low=lo, action_high=-lo)
        train_env.set_cost_function(cn.cost_function)
        agent = PPOLagrangian("TwoCriticsMlpPolicy", train_env, n_steps=32, seed=5)
        _cache["hc"] = (agent, train_env.unwrapped.B.cpu().numpy().reshape(18, 6)[0].copy())
    return _cache["hc"]


def _env(env_id, seed=5, stats_seed=None, **kw):
    from icrl_amd import utils
    env = utils.make_eval_env(env_id, False, seed=seed, **kw)
    env.unwrapped.max_steps = M
    if stats_seed is not None:      # normaliser statistics of its own
        r = np.random.RandomState(stats_seed)
        d = env.unwrapped.obs_dim
        env.obs_rms.assign(r.randn(d) * 0.1, 0.5 + r.rand(d), 100.0)
    return env


def _one_stream(agent, env, n, noise):
    """ground truth: ONE stream runs the n episodes back to back in the existing launch"""
    from icrl_amd import utils
    run = utils.EpisodeRun(agent, env, n, False, noise, parallel=False)
    run.prepare(n_streams=1)
    assert run.n_streams == 1 and run.eps_per == n
    run.launch()
    assert run.finish()
    return run


def _chain(agent, env, n, noise):
    from icrl_amd import utils
    run = utils.EpisodeRun(agent, env, n, False, noise, parallel=True)
    assert run.chain_ok() and run.n_streams == n
    assert utils.launch_chain([run.prepare_chain()])
    run.finish_chain()
    return run


def _snapshot(run, env):
    return dict(orig_obs=run.rows_of("orig_obs").clone(), obs=run.rows_of("obs").clone(), actions=run.rows_of("actions").clone(),
                ep_rewards=run.out["ep_rewards"].clone(), ep_lengths=run.out["ep_lengths"].clone(), s=env.unwrapped.s.clone(),
                step_count=env.unwrapped.step_count.clone())


def _assert_equal(got, want):
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k


def _hc_noise(pattern):
    """action noise [N_EP * M, 6] under which exactly the episodes marked in `pattern` end early on the Test env (the others run to the
    limit), with the ground truth computed ONCE per pattern.  The policy's mean action is small and its std is 1, so the action of a row is
    essentially that row's noise: rows of an early episode push obs[0] towards the wall at -3 with a strength of their own (different
    lengths), all other rows are small.  An episode's rows start where its predecessors ended, so the pattern is laid down episode by
    episode against the one-stream launch."""
    key = tuple(pattern)
    if key not in _cache:
        agent, B0 = _hc_agent()
        rng = np.random.RandomState(7)
        quiet = (0.05 * rng.randn(N_EP * M, 6)).astype(np.float32)
        noise, pos = quiet.copy(), 0
        for k, early in enumerate(pattern):
            length = M
            if early:
                noise[pos:pos + M] = (-np.sign(B0) * (0.55 + 0.07 * k)).astype(np.float32) + quiet[pos:pos + M]
                length = int(_one_stream(agent, _env("HCWithPosTest-v0"), N_EP, noise).lengths[k])
                noise[pos + length:pos + M] = quiet[pos + length:pos + M]
            pos += length
        env = _env("HCWithPosTest-v0")
        truth = _one_stream(agent, env, N_EP, noise)
        _cache[key] = (noise, _snapshot(truth, env))
    return _cache[key]


@pytest.mark.parametrize("case", list(CASES))
def test_chain_equals_one_stream(case, monkeypatch):
    """cases (a)-(d): no episode / only episode 0 / several including the last / all episodes end early"""
    from icrl_amd import utils
    pattern = CASES[case]
    agent, _ = _hc_agent()
    noise, want = _hc_noise(pattern)
    lengths = want["ep_lengths"].cpu().numpy()
    print(case, "ground-truth lengths", lengths.tolist())
    assert [bool(l < M) for l in lengths] == pattern            # the case property, on the ground truth
    early = lengths[lengths < M]
    assert len(early) < 2 or len(set(early.tolist())) > 1       # early episodes end at different lengths
    env = _env("HCWithPosTest-v0")
    run = _chain(agent, env, N_EP, noise)
    assert run.passes == 1
    _assert_equal(_snapshot(run, env), want)
    assert run.rows_of("orig_obs").shape[0] == int(lengths.sum())
    executed = run.out["exec_steps"].cpu().numpy()
    print(case, "executed steps per stream", executed.tolist())
    assert (executed >= lengths).all()
    if any(pattern):
        # no stream executes more than the multi-pass path makes every stream execute: passes x M
        monkeypatch.setenv("ICRL_EPISODE_CHAIN", "0")
        env0 = _env("HCWithPosTest-v0")
        old = utils._run_episodes(agent, env0, N_EP, False, noise, parallel=True)
        _assert_equal(_snapshot(old, env0), want)
        print(case, "multi-pass path:", old.passes, "passes")
        assert old.passes >= 2
        assert int(executed.max()) <= old.passes * M, (executed.tolist(), old.passes)
    else:
        assert executed.tolist() == [M] * N_EP


def test_chain_fixed_length_env():
    """a train-style env (episodes never end early): the fixed_len job — no polling, rows written in place"""
    agent, _ = _hc_agent()
    noise = np.random.RandomState(3).randn(4 * M, 6).astype(np.float32)
    env = _env("HCWithPos-v0", seed=2)
    want_run = _one_stream(agent, env, 4, noise)
    want = _snapshot(want_run, env)
    assert want["ep_lengths"].tolist() == [M] * 4
    env = _env("HCWithPos-v0", seed=2)
    run = _chain(agent, env, 4, noise)
    assert run.fixed_len
    _assert_equal(_snapshot(run, env), want)


def test_chain_discrete_policy():
    """case (e): a Categorical policy on the constrained lap grid world, where a backward move ends the episode"""
    from icrl_amd import utils
    from icrl_amd.ppo_lag import PPOLagrangian
    train_env = utils.make_train_env("LGW-v0", None, True, 1, 2, normalize_obs=False, normalize_reward=False, normalize_cost=False)
    agent = PPOLagrangian("TwoCriticsMlpPolicy", train_env, n_steps=32, seed=1)
    assert agent.policy.discrete
    sd = agent.policy.state_dict()
    sd["action_net.bias"] = torch.as_tensor([2.5, 0.0], dtype=torch.float32)      # mostly forward: episodes of some length
    agent.policy.load_state_dict(sd)
    n = 8
    noise = np.random.RandomState(11).rand(n * M).astype(np.float32)
    env = _env("CLGW-v0", seed=1, normalize_obs=False)
    want = _snapshot(_one_stream(agent, env, n, noise), env)
    lengths = want["ep_lengths"].cpu().numpy()
    print("discrete ground-truth lengths", lengths.tolist())
    assert (lengths < M).sum() >= 2 and len(set(lengths.tolist())) > 2
    env = _env("CLGW-v0", seed=1, normalize_obs=False)
    run = _chain(agent, env, n, noise)
    _assert_equal(_snapshot(run, env), want)


def test_two_jobs_in_one_launch_equal_two_launches():
    """the fused sampling + evaluation launch: a fixed-length job of 4 streams and an early-ending job of 6, with different normaliser
    statistics, against the same two jobs launched separately — and utils.sample_and_evaluate against the two sequential calls"""
    from icrl_amd import utils
    agent, _ = _hc_agent()
    e_noise, _ = _hc_noise(CASES["c_several_and_last"])
    s_noise = np.random.RandomState(3).randn(4 * M, 6).astype(np.float32)

    def envs():
        return _env("HCWithPos-v0", seed=2, stats_seed=21), _env("HCWithPosTest-v0", stats_seed=22)
    senv, eenv = envs()
    want_s = _snapshot(_chain(agent, senv, 4, s_noise), senv)
    want_e = _snapshot(_chain(agent, eenv, N_EP, e_noise), eenv)
    assert want_s["ep_lengths"].tolist() == [M] * 4 and 0 < (want_e["ep_lengths"] < M).sum().item() < N_EP
    # (the separate launches are themselves the sequential loop's rows)
    s1, e1 = envs()
    _assert_equal(want_s, _snapshot(_one_stream(agent, s1, 4, s_noise), s1))
    _assert_equal(want_e, _snapshot(_one_stream(agent, e1, N_EP, e_noise), e1))
    senv, eenv = envs()
    s_run = utils.EpisodeRun(agent, senv, 4, False, s_noise, True)
    e_run = utils.EpisodeRun(agent, eenv, N_EP, False, e_noise, False)
    assert s_run.fixed_len and not e_run.fixed_len and s_run.n_streams == 4 and e_run.n_streams == N_EP
    assert utils.launch_chain([s_run.prepare_chain(), e_run.prepare_chain()])
    s_run.finish_chain(); e_run.finish_chain()
    _assert_equal(_snapshot(s_run, senv), want_s)
    _assert_equal(_snapshot(e_run, eenv), want_e)
    # the host entry: what sample_from_agent and evaluate_policy return
    senv, eenv = envs()
    (oo, o, a, r, l), (er, el) = utils.sample_and_evaluate(agent, senv, 4, eenv, N_EP, deterministic=False, sample_noise=s_noise,
                                                           eval_noise=e_noise, return_episode_rewards=True)
    s2, e2 = envs()
    oo2, o2, a2, r2, l2 = utils.sample_from_agent(agent, s2, 4, noise=s_noise)
    er2, el2 = utils.evaluate_policy(agent, e2, N_EP, deterministic=False, noise=e_noise, return_episode_rewards=True)
    assert torch.equal(oo, oo2) and torch.equal(o, o2) and torch.equal(a, a2) and np.array_equal(r, r2) and np.array_equal(l, l2)
    assert np.array_equal(er, er2) and np.array_equal(el, el2)
    assert torch.equal(senv.unwrapped.s, s2.unwrapped.s) and torch.equal(eenv.unwrapped.step_count, e2.unwrapped.step_count)


def test_chain_refusals():
    """what the entry point does not serve is refused with a reason, and the caller takes the multi-pass path"""
    from icrl_amd import utils
    agent, _ = _hc_agent()
    noise, want = _hc_noise(CASES["d_all"])
    env = _env("HCWithPosTest-v0")
    run = utils.EpisodeRun(agent, env, N_EP, False, noise, True).prepare_chain()
    run.job.episodes_per_stream = 2
    assert utils.launch_chain([run]) is False
    env = _env("HCWithPosTest-v0")
    run = utils.EpisodeRun(agent, env, N_EP, False, noise, True)
    run.chain_ok = lambda: False
    utils._launch_and_finish(run)
    assert run.passes >= 2
    _assert_equal(_snapshot(run, env), want)


@pytest.mark.parametrize("rng", ["device", "seeded"])
def test_outer_iterations_equal_with_and_without_chain(rng, tmp_path, monkeypatch):
    """two outer iterations of icrl (4 envs, n_steps 64, 4 nominal episodes): every logged metric is identical with the chained, fused
    episode launch and with ICRL_EPISODE_CHAIN=0 (separate phases, multi-pass positions); wall-clock entries excluded"""
    from icrl_amd.icrl import build_parser, outer_iteration, setup
    from oracle.streams import SeededStreams
    here = os.path.dirname(os.path.abspath(__file__))
    expert = os.path.join(here, "golden/expert_hc.npz")
    argv = ["icrl", "-er", "4", "-ep", expert, "--expert_agent_path", expert, "-tk", "0.01", "-cl", "20", "-bi", "3", "-ft", "512", "-ni", "2",
            "-tei", "HCWithPos-v0", "-eei", "HCWithPosTest-v0", "-clr", "0.05", "-crc", "0.5", "-psis", "-nt", "4", "--n_steps", "64", "-ne", "2",
            "-s", "0", "-v", "0"]
    runs = []
    for switch in ("1", "0"):
        monkeypatch.setenv("ICRL_EPISODE_CHAIN", switch)
        cfg = vars(build_parser().parse_args(argv))
        cfg.update(rank=0, world_size=1, save_dir=None)
        if rng == "seeded":
            cfg.update(streams=SeededStreams(13))
        torch.manual_seed(0)
        st = setup(types.SimpleNamespace(**cfg))
        runs.append([outer_iteration(st, itr) for itr in range(2)])
    for on, off in zip(*runs):
        keys = sorted(k for k in on if "time" not in k and "fps" not in k)
        assert keys == sorted(k for k in off if "time" not in k and "fps" not in k)
        for k in keys:
            a, b = on[k], off[k]
            assert a == b or (a != a and b != b), (k, a, b)
