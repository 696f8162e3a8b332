"""GPU: sampling and evaluation episodes of a gSDE agent as one launch (icrl_sample_episodes_sde / icrl_sample_episodes_chain_sde through
utils.EpisodeRun).

1. the launch against the per-step loop (utils.SteppedEpisodeRun), bit for bit: rows, episode sums, lengths, the env's end state;
2. the generator: nothing is drawn, except the loop's own reset_noise(1) when the policy holds no matrices;
3. independent of both paths: the clipped action of every row from the previous row's recorded observation, in numpy;
4. sample_and_evaluate: the two phases as two jobs of one launch;
5. through cpg.setup: learn() with an EvalCallback and a sample_from_agent, against the twin under ICRL_SDE_EPISODES_STEPPED=1.
Episodes run at most M = 48 steps, 6 episodes at most."""
import types

import numpy as np
import pytest
import torch

from helpers import sde_episode_cases as E

pytestmark = pytest.mark.gpu

M, N_EP = E.M, 6
_cache = {}


def _agent(env_id, **kw):
    key = (env_id, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _cache:
        _cache[key] = E.agent(env_id, **kw)
    return _cache[key]


def _loop(ag, env_id, n, deterministic, **kw):
    """the loop's result, once per case"""
    key = ("loop", id(ag), env_id, n, deterministic, tuple(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = E.loop(ag, env_id, n, deterministic, **kw)[0]
    return _cache[key]


def _fused(ag, run):
    from icrl_amd import utils
    assert isinstance(run, utils.EpisodeRun) and run.sde, type(run)
    assert ag.last_sde_episodes == "fused" and ag.last_sde_episodes_reason is None, (ag.last_sde_episodes, ag.last_sde_episodes_reason)


def _case_property(case, lengths):
    lengths = [int(x) for x in lengths]
    if case == "none":
        assert min(lengths) == M, lengths
    elif case == "all":
        assert max(lengths) < M and len(set(lengths)) >= 2, lengths
    else:
        assert min(lengths) < M and max(lengths) == M, lengths


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deterministic", [False, True])
def test_fixed_length_episodes_take_the_chained_kernel_without_polling(deterministic, monkeypatch):
    monkeypatch.delenv("ICRL_SDE_EPISODES_STEPPED", raising=False)
    monkeypatch.delenv("ICRL_EPISODE_CHAIN", raising=False)
    ag = _agent("HCWithPos-v0")
    want = _loop(ag, "HCWithPos-v0", N_EP, deterministic)
    assert want["ep_lengths"].tolist() == [M] * N_EP
    got, run = E.launch(ag, "HCWithPos-v0", N_EP, deterministic)
    _fused(ag, run)
    assert run.fixed_len and run.n_streams == N_EP and run.passes == 1 and "exec_steps" in run.out      # the chained launch
    assert (run.expl is None) == deterministic
    E.assert_equal(got, want, f"hc x {N_EP}, deterministic {deterministic}")


@pytest.mark.parametrize("case,deterministic", [("none", False), ("all", False), ("some", False), ("some", True)])
def test_early_ending_episodes_settle_their_positions_inside_the_launch(case, deterministic, monkeypatch):
    monkeypatch.delenv("ICRL_SDE_EPISODES_STEPPED", raising=False)
    monkeypatch.delenv("ICRL_EPISODE_CHAIN", raising=False)
    ag = _agent("HCWithPosTest-v0", steer=E.STEER[case])
    want = _loop(ag, "HCWithPosTest-v0", N_EP, deterministic)
    print(f"SDE_EPISODES_LENGTHS {case} deterministic {deterministic}: {want['ep_lengths'].tolist()}")
    _case_property(case, want["ep_lengths"].tolist())
    got, run = E.launch(ag, "HCWithPosTest-v0", N_EP, deterministic)
    _fused(ag, run)
    assert not run.fixed_len and run.n_streams == N_EP and run.passes == 1 and "exec_steps" in run.out
    E.assert_equal(got, want, f"hctest {case}, deterministic {deterministic}")


def test_the_passes_with_the_chain_switched_off(monkeypatch):
    """ICRL_EPISODE_CHAIN=0: the plain kernel with stream_row0, positions settled by repeated launches"""
    monkeypatch.delenv("ICRL_SDE_EPISODES_STEPPED", raising=False)
    monkeypatch.setenv("ICRL_EPISODE_CHAIN", "0")
    ag = _agent("HCWithPosTest-v0", steer=E.STEER["some"])
    want = _loop(ag, "HCWithPosTest-v0", N_EP, False)
    _case_property("some", want["ep_lengths"].tolist())
    got, run = E.launch(ag, "HCWithPosTest-v0", N_EP, False)
    _fused(ag, run)
    assert run.passes >= 2 and "exec_steps" not in run.out
    E.assert_equal(got, want, "hctest some, passes")


def test_a_padded_latent():
    """-pl 32 48: rows 48..63 of the stored matrix and of the latent are zero"""
    ag = _agent("HCWithPos-v0", arch=E.PL)
    assert ag.policy.sde_latent == 48 and not ag.policy.sde_E0[48:].any() and ag.policy.sde_E0[:48].abs().min() > 0
    want = _loop(ag, "HCWithPos-v0", 3, False)
    got, run = E.launch(ag, "HCWithPos-v0", 3, False)
    _fused(ag, run)
    E.assert_equal(got, want, "hc -pl 32 48")


def test_antwall_takes_the_wide_observation_kernel():
    ag = _agent("AntWall-v0")
    assert ag.policy.obs_dim == 113 and ag.policy.act_dim == 8
    want = _loop(ag, "AntWall-v0", 3, False, max_steps=24)
    assert want["ep_lengths"].tolist() == [24] * 3
    got, run = E.launch(ag, "AntWall-v0", 3, False, max_steps=24)
    _fused(ag, run)
    assert run.n_streams == 3
    E.assert_equal(got, want, "ant 3 x 24")


def test_one_episode_is_one_stream_of_the_plain_kernel():
    ag = _agent("HCWithPos-v0")
    want = _loop(ag, "HCWithPos-v0", 1, False)
    got, run = E.launch(ag, "HCWithPos-v0", 1, False)
    _fused(ag, run)
    assert run.n_streams == 1 and not run.chain_ok() and run.passes == 1
    E.assert_equal(got, want, "hc x 1")


def test_a_point_env_takes_the_plain_kernel_pass_by_pass():
    """the chained entry point refuses a Point env (tests/test_sde_episodes_cpu.py), so the passes run: the plain kernel's Point step"""
    ag = _agent("PointCircleTest-v0")
    want = _loop(ag, "PointCircleTest-v0", 3, False)
    got, run = E.launch(ag, "PointCircleTest-v0", 3, False)
    _fused(ag, run)
    assert run.senv.reward_form >= 4 and not run.chain_ok() and "exec_steps" not in run.out
    E.assert_equal(got, want, "point circle test x 3")


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------------
def test_nothing_is_drawn_from_the_generator_when_the_policy_holds_its_matrices(monkeypatch):
    from icrl_amd import utils
    monkeypatch.delenv("ICRL_SDE_EPISODES_STEPPED", raising=False)
    ag = _agent("HCWithPos-v0")
    E0 = ag.policy.sde_E0
    torch.manual_seed(77)
    before = torch.cuda.get_rng_state()
    utils.sample_from_agent(ag, E.eval_env("HCWithPos-v0"), 3)
    assert ag.last_sde_episodes == "fused"
    assert torch.equal(torch.cuda.get_rng_state(), before)
    assert ag.policy.sde_E0 is E0, "the policy's matrices are left as they were"


def test_a_policy_without_matrices_makes_the_loops_one_draw_and_the_mode_makes_none(monkeypatch):
    from icrl_amd import utils
    monkeypatch.delenv("ICRL_SDE_EPISODES_STEPPED", raising=False)
    ag, twin = E.agent("HCWithPos-v0", noise=False), E.agent("HCWithPos-v0", noise=False)
    assert ag.policy.sde_E is None and twin.policy.sde_E is None
    # the mode: nothing drawn, nothing installed
    torch.manual_seed(31)
    before = torch.cuda.get_rng_state()
    utils.evaluate_policy(ag, E.eval_env("HCWithPos-v0"), 2, deterministic=True)
    assert ag.last_sde_episodes == "fused" and ag.policy.sde_E is None and ag.policy.sde_E0 is None
    assert torch.equal(torch.cuda.get_rng_state(), before)
    # sampling: the draw _forward_sde makes at the loop's first step
    torch.manual_seed(31)
    utils.sample_from_agent(ag, E.eval_env("HCWithPos-v0"), 2)
    after = torch.cuda.get_rng_state()
    torch.manual_seed(31)
    twin.policy.reset_noise(1)
    assert torch.equal(ag.policy.sde_E0, twin.policy.sde_E0) and torch.equal(ag.policy.sde_E, twin.policy.sde_E)
    assert torch.equal(torch.cuda.get_rng_state(), after), "the generator ends where the loop leaves it"


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_id,case", [("HCWithPos-v0", None), ("HCWithPosTest-v0", "some")])
def test_every_action_follows_from_the_previous_rows_observation_and_e0(env_id, case, monkeypatch):
    """Row k's clipped action against the numpy head (float64) on row k - 1's recorded normalised observation cast to float32 — the post-step
    observation the sampler records is the next step's policy input, across episode ends too (the auto-reset observation).  Bound: 1e-5 of the
    actions' scale, the project's bound for a float32 MLP output.  Measured on an MI355X: see DESIGN.md section 26."""
    from icrl_amd import utils
    monkeypatch.delenv("ICRL_SDE_EPISODES_STEPPED", raising=False)
    ag = _agent(env_id, steer=None if case is None else E.STEER[case])
    pol = ag.policy
    sd = {k: v.numpy() for k, v in pol.state_dict().items()}
    E0 = pol.sde_E0[:pol.sde_latent].cpu().numpy()
    _, obs, actions, _, lengths = utils.sample_from_agent(ag, E.eval_env(env_id), N_EP)
    assert ag.last_sde_episodes == "fused"
    if case is not None:
        _case_property(case, lengths)
    obs, actions = obs.cpu().numpy(), actions.cpu().numpy()
    assert len(obs) == int(np.sum(lengths)) > M
    want = E.head_numpy_actions(sd, E0, obs[:-1].astype(np.float32))
    err = float(np.abs(actions[1:] - want).max() / max(1.0, np.abs(want).max()))
    inside = float((np.abs(want) < 1.0).mean())
    print(f"SDE_EPISODES_HEAD {env_id}: max |launch - numpy| = {err:.3g} of scale over {len(want)} rows, {inside:.2f} of the entries inside the box")
    assert inside > 0.2, "the clip must not hide the head"
    assert err <= 1e-5, err


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deterministic", [False, True])
def test_sample_and_evaluate_runs_both_phases_as_two_jobs_of_one_launch(deterministic, monkeypatch):
    from icrl_amd import utils
    monkeypatch.delenv("ICRL_SDE_EPISODES_STEPPED", raising=False)
    monkeypatch.delenv("ICRL_EPISODE_CHAIN", raising=False)
    ag = _agent("HCWithPosTest-v0", steer=E.STEER["some"])
    calls = []
    real = utils.launch_chain
    monkeypatch.setattr(utils, "launch_chain", lambda runs: calls.append(len(runs)) or real(runs))
    ag.last_sde_episodes = None
    s_got, e_got = utils.sample_and_evaluate(ag, E.eval_env("HCWithPos-v0"), 4, E.eval_env("HCWithPosTest-v0", seed=9), n_eval_episodes=3,
                                             deterministic=deterministic, return_episode_rewards=True)
    assert calls == [2] and ag.last_sde_episodes == "fused"
    s_want = utils.sample_from_agent(ag, E.eval_env("HCWithPos-v0"), 4)
    e_want = utils.evaluate_policy(ag, E.eval_env("HCWithPosTest-v0", seed=9), 3, deterministic=deterministic, return_episode_rewards=True)
    for k in range(3):
        assert torch.equal(s_got[k], s_want[k]), k
    assert np.array_equal(s_got[3], s_want[3]) and np.array_equal(s_got[4], s_want[4])
    assert np.array_equal(np.asarray(e_got[0]), np.asarray(e_want[0])) and list(e_got[1]) == list(e_want[1])
    # and the sequential calls are the loop's
    want = _loop(ag, "HCWithPosTest-v0", 3, deterministic, seed=9)
    assert np.array_equal(np.asarray(e_got[0]), want["ep_rewards"].cpu().numpy()) and list(e_got[1]) == want["ep_lengths"].tolist()


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------------
_CPG = ("-tei", "HCWithPos-v0", "-eei", "HCWithPosTest-v0", "-nt", "4", "--n_steps", "32", "-t", "128", "-ee", "32", "-us", "-sfr", "-ssf", "8")


def _cpg_run(seed=0):
    from icrl_amd import callbacks, cpg as Cpg, utils
    cfg = vars(Cpg.build_parser().parse_args(["cpg", *_CPG, "-s", str(seed), "-v", "0"]))
    cfg.update(rank=0, world_size=1)
    cfg = types.SimpleNamespace(**cfg)
    model, cb, learn_cost, _hist = Cpg.setup(cfg, log=None)
    ev, = [c for c in cb.callbacks if isinstance(c, callbacks.EvalCallback)]
    ev.eval_env.unwrapped.max_steps = M
    torch.manual_seed(200 + seed)
    model.learn(total_timesteps=int(cfg.timesteps), cost_function=learn_cost, callback=cb)
    assert len(ev.evaluations_results) == 1, "the EvalCallback fires once"
    after_eval = (model.last_sde_episodes, model.last_sde_episodes_reason)
    env = E.eval_env("HCWithPos-v0")
    rows = utils.sample_from_agent(model, env, 3)
    model.check_rollout_status()
    return model, ev, rows, after_eval


def test_cpg_evaluates_and_samples_with_the_launch_and_its_twin_under_the_switch_gives_the_same(monkeypatch):
    monkeypatch.delenv("ICRL_SDE_EPISODES_STEPPED", raising=False)
    monkeypatch.delenv("ICRL_SDE_ROLLOUT_FUSED", raising=False)
    model, ev, rows, after_eval = _cpg_run()
    assert after_eval == ("fused", None) and (model.last_sde_episodes, model.last_sde_episodes_reason) == ("fused", None)
    assert model.last_sde_rollout == "fused"
    monkeypatch.setenv("ICRL_SDE_EPISODES_STEPPED", "1")
    twin, tev, trows, t_after_eval = _cpg_run()
    assert t_after_eval == ("loop", "ICRL_SDE_EPISODES_STEPPED=1")
    assert (twin.last_sde_episodes, twin.last_sde_episodes_reason) == ("loop", "ICRL_SDE_EPISODES_STEPPED=1")
    assert ev.evaluations_results == tev.evaluations_results and ev.evaluations_length == tev.evaluations_length
    assert max(ev.evaluations_length[0]) <= M
    for k in range(3):
        assert torch.equal(rows[k], trows[k]), k
    assert np.array_equal(rows[3], trows[3]) and np.array_equal(rows[4], trows[4])
    assert torch.equal(model.policy.params, twin.policy.params) and torch.equal(model.policy.sde_E0, twin.policy.sde_E0)
