"""GPU: the gSDE rollout as a launch of the library (icrl_rollout_collect_sde; PPOLagrangian(sde_fused_rollout=True), --sde_fused_rollout).

1. the persistent launch against the per-step launches, bit for bit (the rule of test_persistent_rollout_equals_per_step_launches), both routes
   asserted with ICRL_PICK_SDE;
2. the per-step launches against the Python loop on the same matrices, within the bounds of test_stepped_rollout_equals_fused_rollout;
3. independent of both GPU paths: actions and log-probs recomputed in numpy from the buffer's observations and the recorded normals;
4. through cpg.setup: the flag, the twin without it under the same seed, learn() and train(), every reason for the loop, the environment switch.
Every case runs two consecutive rollouts, and every env crosses its time limit inside the first."""
import types

import numpy as np
import pytest
import torch

from helpers import routes as R
from helpers import sde_cases as C
from helpers import sde_rollout_cases as S

pytestmark = pytest.mark.gpu


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------------
#   hc 7 x 33 ssf 8: a ragged cadence; hc 64 x 24 ssf -1: record mode, one draw; hc 80 x 12 ssf 5: flag mode at HC width (80 * 40 > 3072 exchange
#   words); ant 32 x 12 ssf 1: the <8, 10> image, flag mode, a redraw every step; hc 1 x 20 ssf 4: the E0 of each draw; hc 7 x 20 -pl 32 48: a padded
#   latent; the analytic wall cost (the <2, 0> image) and no cost at all
PERSISTENT_CASES = [("hc", 7, 33, 8, "net", None, True), ("hc", 64, 24, -1, "net", None, True), ("hc", 80, 12, 5, "net", None, False),
                    ("ant", 32, 12, 1, "net", None, False), ("hc", 1, 20, 4, "net", None, True), ("hc", 7, 20, 8, "net", S.PL, True),
                    ("hc", 7, 20, 8, "wall", None, True), ("hc", 7, 20, 8, "none", None, True)]


@pytest.mark.parametrize("kind,N,T,ssf,cost,arch,gran", PERSISTENT_CASES)
def test_persistent_sde_rollout_equals_the_per_step_launches(kind, N, T, ssf, cost, arch, gran):
    from icrl_amd import _lib
    p, s = S.agents(N, T, ssf, ("auto", "steps"), kind=kind, cost=cost, arch=arch)

    def check(it):
        p[0].check_rollout_status()
        S.assert_rollouts_bit_equal(p, s, it)
        assert p[0].rollout_buffer.dones.sum().item() == (N if it == 0 else s[0].rollout_buffer.dones.sum().item())
        if cost == "wall":
            c = p[0].rollout_buffer.orig_costs
            assert 0.0 < float(c.mean()) < 1.0 and torch.equal(c, (p[0].rollout_buffer.orig_observations[..., 0] <= 0.0).float())
        if cost == "none":
            assert not p[0].rollout_buffer.orig_costs.any() and not p[0].rollout_buffer.costs.any()

    for it in range(2):
        assert p[0].collect_rollouts(p[1], None, p[0].rollout_buffer, T, "cost") is True
        got = S.expect_route(p[0], "persistent", N, T, f"{kind} {N} x {T} ssf {ssf} {cost}")
        assert bool(got["pick"] & _lib.PICK_GRAN) == gran and bool(got["pick"] & _lib.PICK_SMALL) == (kind == "hc")
        assert bool(got["pick"] & _lib.PICK_ANALYTIC) == (cost == "wall")
        assert s[0].collect_rollouts(s[1], None, s[0].rollout_buffer, T, "cost") is True
        S.expect_route(s[0], "per-step", N, T, f"{kind} {N} x {T} steps")
        check(it)
    assert p[0].num_timesteps == s[0].num_timesteps == 2 * N * T
    # the schedule is kept alive until the next rollout, and the policy holds the last draw as after the loop
    D = -(-T // ssf) if ssf > 0 else 1
    assert tuple(p[0]._keepalive[0].shape) == (D, N, 64, S.DIMS[kind][1])
    assert torch.equal(p[0].policy.sde_E, s[0].policy.sde_E) and torch.equal(p[0].policy.sde_E0, s[0].policy.sde_E0)


def test_more_than_128_envs_take_the_per_step_launches_by_themselves():
    N, T, ssf = 130, 10, 4
    (a, env), = S.agents(N, T, ssf, ("auto",))
    sd = {k: v.numpy() for k, v in a.policy.state_dict().items()}
    for it in range(2):
        assert a.collect_rollouts(env, None, a.rollout_buffer, T, "cost") is True
        S.expect_route(a, "per-step", N, T, "hc 130 x 10, nothing forced")
        a.check_rollout_status()
        _check_head(a, sd, it, T, ssf)
        if it == 0:      # every env crossed its time limit
            assert a.rollout_buffer.dones.sum().item() == N


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------------
def test_per_step_sde_launches_equal_the_python_loop_on_the_same_matrices():
    """different kernels for the forward (act_step_sde_kernel's head against policy_forward_sde_kernel's) and for the normaliser's pieces: the bounds of
    test_stepped_rollout_equals_fused_rollout — rtol 2e-5, atol 2e-6 on the buffer planes, 1e-12 on the statistics.  Measured on an MI355X: see
    DESIGN.md, the section on the gSDE rollout."""
    N, T, ssf = 16, 48, 8
    f, l = S.agents(N, T, ssf, ("steps", "loop"), seed=11)
    for it in range(2):
        assert f[0].collect_rollouts(f[1], None, f[0].rollout_buffer, T, "cost") is True
        S.expect_route(f[0], "per-step", N, T, "hc 16 x 48 steps")
        assert l[0].collect_rollouts(l[1], None, l[0].rollout_buffer, T, "cost") is True
        assert l[0].last_sde_rollout == "loop" and l[0].last_sde_rollout_reason == "sde_fused_rollout is off"
        R.check_rollout(dict(route="per-step", launches=2 * T), "the loop calls no rollout entry point: the record stays")
        worst = {}
        for k in S.BUF_KEYS:
            got, ref = getattr(f[0].rollout_buffer, k).cpu().numpy(), getattr(l[0].rollout_buffer, k).cpu().numpy()
            worst[k] = float(np.abs(got - ref).max())
            print(f"SDE_ROLLOUT_VS_LOOP rollout {it} {k}: max |launches - loop| = {worst[k]:.3g}")
        for k in S.BUF_KEYS:
            got, ref = getattr(f[0].rollout_buffer, k).cpu().numpy(), getattr(l[0].rollout_buffer, k).cpu().numpy()
            assert np.allclose(got, ref, rtol=2e-5, atol=2e-6), (it, k, worst[k])
        assert torch.equal(f[0].policy.sde_E, l[0].policy.sde_E) and len(f[0].streams.calls) == len(l[0].streams.calls) == 2 * (it + 1) * (1 + T // ssf)
    assert np.allclose(f[1].obs_rms.mean, l[1].obs_rms.mean, rtol=0, atol=1e-12) and np.allclose(f[1].obs_rms.var, l[1].obs_rms.var, rtol=0, atol=1e-12)
    assert abs(f[1].cost_rms.var - l[1].cost_rms.var) < 1e-12 and abs(f[1].ret_rms.var - l[1].ret_rms.var) < 1e-12
    assert f[1].obs_rms.count == l[1].obs_rms.count and f[0].num_timesteps == l[0].num_timesteps == 2 * N * T


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------------
def _check_head(agent, sd, rollout, T, ssf):
    """actions[t, n] = mean + latent . E[draw(t)][n] and the log-probs, in numpy float64 from the buffer's observations and the recorded normals:
    1e-5 of scale, the project's bound for a float32 forward (test_learn_collects_with_the_matrices_it_holds_and_trains_log_std)"""
    rb = agent.rollout_buffer
    obs, act, lp = rb.observations.cpu().numpy(), rb.actions.cpu().numpy(), rb.log_probs.cpu().numpy()
    worst_a = worst_lp = 0.0
    for t in range(T):
        E = S.matrices_of_step(agent, rollout, t, T, ssf)
        out, _ = C.head_numpy(sd, obs[t], act[t])
        want = out["mean"] + np.einsum("nh,nha->na", out["latent"], E)
        ea, el = np.abs(act[t] - want).max() / max(1.0, np.abs(want).max()), np.abs(lp[t] - out["log_prob"]).max() / np.abs(out["log_prob"]).max()
        worst_a, worst_lp = max(worst_a, ea), max(worst_lp, el)
        assert ea <= 1e-5 and el <= 1e-5, (t, ea, el)
    print(f"SDE_ROLLOUT_HEAD {agent.n_envs} x {T} ssf {ssf} rollout {rollout}: actions {worst_a:.3g}, log-probs {worst_lp:.3g} of scale")


@pytest.mark.parametrize("T,ssf", [(20, 8), (12, 1)])
@pytest.mark.parametrize("mode", ["auto", "steps"])
def test_actions_and_log_probs_follow_from_the_observations_and_the_schedule(T, ssf, mode):
    N = 7
    (a, env), = S.agents(N, T, ssf, (mode,), seed=5)
    sd = {k: v.numpy() for k, v in a.policy.state_dict().items()}
    for it in range(2):
        assert a.collect_rollouts(env, None, a.rollout_buffer, T, "cost") is True
        S.expect_route(a, "persistent" if mode == "auto" else "per-step", N, T, f"hc 7 x {T} ssf {ssf} {mode}")
        a.check_rollout_status()
        _check_head(a, sd, it, T, ssf)
        if ssf == 1:      # a redraw every step: consecutive steps hold different matrices
            assert not np.array_equal(S.matrices_of_step(a, it, 0, T, ssf), S.matrices_of_step(a, it, 1, T, ssf))
    clipped = a._ag["act_clipped"].cpu().numpy()
    assert np.array_equal(clipped, np.clip(a.rollout_buffer.actions[-1].cpu().numpy(), -1.0, 1.0))


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------------
_CPG = ("-tei", "HCWithPos-v0", "-eei", "HCWithPosTest-v0", "-nt", "4", "--n_steps", "32", "-t", "256", "-us", "-ssf", "8")


def _setup(extra, seed=0):
    from icrl_amd import cpg as Cpg
    cfg = vars(Cpg.build_parser().parse_args(["cpg", *_CPG, "-s", str(seed), "-v", "0", *extra]))
    cfg.update(rank=0, world_size=1)
    cfg = types.SimpleNamespace(**cfg)
    return cfg, Cpg.setup(cfg, log=None)


def test_cpg_with_the_flag_collects_with_one_launch_and_its_twin_without_it_makes_the_same_draws(monkeypatch):
    monkeypatch.delenv("ICRL_SDE_ROLLOUT_FUSED", raising=False)
    cfg, (model, cb, learn_cost, hist) = _setup(["-sfr"])
    _, (twin, _cb, twin_cost, _h) = _setup([])
    assert model.sde_fused_rollout is True and twin.sde_fused_rollout is False and model.streams is None and twin.streams is None
    model._setup_learn(128); twin._setup_learn(128)
    for it in range(2):
        torch.manual_seed(100 + it)
        assert model.collect_rollouts(model.env, None, model.rollout_buffer, 32, learn_cost) is True
        got = S.expect_route(model, "persistent", 4, 32, "cpg -us -sfr -ssf 8 -nt 4")
        assert got["wgs"] == 4
        model.check_rollout_status()
        torch.manual_seed(100 + it)
        assert twin.collect_rollouts(twin.env, None, twin.rollout_buffer, 32, twin_cost) is True
        assert twin.last_sde_rollout == "loop" and twin.last_sde_rollout_reason == "sde_fused_rollout is off"
        # the up-front draws are the loop's draws: the same last matrices, and the same generator state behind them
        assert torch.equal(model.policy.sde_E, twin.policy.sde_E) and torch.equal(model.policy.sde_E0, twin.policy.sde_E0)
        for k in S.BUF_KEYS:
            a, b = getattr(model.rollout_buffer, k).cpu().numpy(), getattr(twin.rollout_buffer, k).cpu().numpy()
            assert np.allclose(a, b, rtol=2e-5, atol=2e-6), (it, k, np.abs(a - b).max())
    assert np.allclose(model.env.obs_rms.mean, twin.env.obs_rms.mean, rtol=0, atol=1e-12)
    model.train()
    assert model.last_sde_update == "fused", model.last_sde_update_reason
    model.learn(total_timesteps=int(cfg.timesteps), cost_function=learn_cost, callback=cb)
    assert model.last_sde_rollout == "fused" and model.num_timesteps == 256 and torch.isfinite(model.policy.params).all()
    assert torch.isfinite(model.rollout_buffer.reward_advantages).all() and len(hist.history) >= 1
    model.check_rollout_status()


def test_every_reason_for_the_loop_and_the_environment_switch(monkeypatch):
    from icrl_amd.true_constraint_net import null_cost
    monkeypatch.delenv("ICRL_SDE_ROLLOUT_FUSED", raising=False)
    # --episode_stats: the gSDE kernels do not store the raw-reward plane
    _, (m, _cb, cost, _h) = _setup(["-sfr", "--episode_stats"])
    m._setup_learn(128)
    assert m.collect_rollouts(m.env, None, m.rollout_buffer, 32, cost) is True
    assert m.last_sde_rollout == "loop" and m.last_sde_rollout_reason.startswith("episode_stats")
    # a callable cost_function, the byte cap, a partial rollout — on one agent; then the launch again
    _, (m, _cb, cost, _h) = _setup(["-sfr"])
    m._setup_learn(128)
    assert m.collect_rollouts(m.env, None, m.rollout_buffer, 32, null_cost) is True
    assert (m.last_sde_rollout, m.last_sde_rollout_reason) == ("loop", "a callable cost_function")
    m.sde_fused_max_bytes = 1
    assert m.collect_rollouts(m.env, None, m.rollout_buffer, 32, cost) is True
    assert m.last_sde_rollout == "loop" and m.last_sde_rollout_reason == f"the schedule of {4 * 4 * 4 * 64 * 6} bytes exceeds sde_fused_max_bytes = 1"
    m.sde_fused_max_bytes = 512 << 20
    assert m.collect_rollouts(m.env, None, m.rollout_buffer, 32, cost) is True
    S.expect_route(m, "persistent", 4, 32, "after the fallbacks: the launch")
    m.rollout_kernel = "steps"
    assert m.collect_rollouts(m.env, None, m.rollout_buffer, 32, cost) is True
    S.expect_route(m, "per-step", 4, 32, 'rollout_kernel = "steps"')
    m.check_rollout_status()
    # the environment switch, for tools that take no flag
    monkeypatch.setenv("ICRL_SDE_ROLLOUT_FUSED", "1")
    _, (m, _cb, cost, _h) = _setup([])
    assert m.sde_fused_rollout is True
    m._setup_learn(128)
    assert m.collect_rollouts(m.env, None, m.rollout_buffer, 32, cost) is True
    S.expect_route(m, "persistent", 4, 32, "ICRL_SDE_ROLLOUT_FUSED=1")
    m.check_rollout_status()
