"""GPU: the step chain of the one-workgroup-per-env persistent rollout (rollout_persistent_body in csrc/rollout.hip) against the per-step
launches (`rollout_kernel = "steps"`: do_gae bit 1), bit for bit: every buffer plane, the normaliser's moments, counts and running returns, the
agent's last_* / raw_* / dones state and status word 0.

What the cases are chosen for: inside a step the body orders its waves with wave-local waits where the per-step kernels use workgroup
barriers, stores the log-prob and the two values from the waves that computed them, advances the running returns on the statistics waves
(one or two envs per lane) and normalises the own env's reward and cost on the cost wave.  N in {1, 3, 8, 33, 64, 96, 128} covers powers
of two and other counts (a form of the batch moments that multiplies by 1 / N where that is exact was measured and is not in the tree; the
cases stay), a masked last block of 32 rows (1, 3, 8, 33) and full blocks only (64, 96, 128), one polled record per thread up to five
(64 envs x 20 records over 256 threads) and the flag exchange of the shapes beyond 12 words per thread (96, 128), which keeps the barrier in
front of the column chains.  T = 24..40 with every env crossing its time limit
inside the first rollout: dones, resets and the zeroed running returns occur.  Every case asserts that the launch under test was the
persistent kernel (icrl_debug_last_route), so a ladder that moved fails the case instead of comparing two other forms."""
import numpy as np
import pytest
import torch

from helpers import routes

pytestmark = pytest.mark.gpu

_ONE = dict(route="persistent", launches=1, envs_per_wg=1, ws=1)


def _cn_pair(kind, N, T, norm=None, agent_kwargs=None):
    import test_rollout_gpu as tr
    (a_p, e_p, _), (a_s, e_s, _) = tr._pair_of_agents(N, T, 13, kind, norm_kwargs=norm, agent_kwargs=agent_kwargs)
    return (a_p, e_p), (a_s, e_s)


def _analytic_pair(kind, N, T, cost, **norm):
    import test_cost_fn_gpu as tc
    return tuple(tc._pair(N, T, 13, kind, cost, **norm))


def _costless_pair(kind, N, T):
    """no cost wrapper in the chain (the GAIL baseline's chain): costs are 0, no cost statistics"""
    from icrl_amd.ppo_lag import PPOLagrangian
    from icrl_amd.vec_env import HipSynthVecEnv, VecNormalizeWithCost
    out = []
    for _ in range(2):
        torch.manual_seed(13)
        env = VecNormalizeWithCost(HipSynthVecEnv(N, kind, 13))
        out.append((PPOLagrangian("TwoCriticsMlpPolicy", env, n_steps=T, seed=13), env))
    out[1][0].policy.load_state_dict(out[0][0].policy.state_dict())
    return tuple(out)


def _lgw_pair(N, T):
    import test_routes_gpu as tg
    return tuple(tg._lgw_pair(N, T)[:2])


def _noise(a_p, T, N, rollouts=2):
    rng = np.random.RandomState(8)
    if hasattr(a_p.action_space, "n"):        # Discrete: one uniform per env step
        return torch.as_tensor(rng.rand(rollouts, T, N).astype(np.float32), device="cuda")
    return torch.as_tensor(rng.randn(rollouts, T, N, a_p.action_space.shape[0]).astype(np.float32), device="cuda")


def _status0(agent):
    return int(agent._ag["status"].flatten()[0].item())


def _compare(pair, T, N, expect, tag, steps_side="steps", prof=False):
    """two consecutive rollouts of the twin chains; `steps_side`: the rollout_kernel of the reference side"""
    import test_routes_gpu as tg
    (a_p, e_p), (a_s, e_s) = pair
    a_p.rollout_kernel, a_s.rollout_kernel = "auto", steps_side
    if prof:
        a_p.profile_phases = 1
    noise = _noise(a_p, T, N)
    a_p._setup_learn(2 * N * T); a_s._setup_learn(2 * N * T)
    limit = e_p.unwrapped.max_steps
    for env in (e_p, e_s):
        env.unwrapped.t_ep.fill_(limit - T // 2)           # every env crosses its time limit inside the first rollout
    for it in range(2):
        a_p.collect_rollouts(e_p, None, a_p.rollout_buffer, T, "cost", noise=noise[it])
        got = routes.check_rollout(dict(expect, wgs=N, n_runs=1), f"{tag} auto")
        a_s.collect_rollouts(e_s, None, a_s.rollout_buffer, T, "cost", noise=noise[it])
        if steps_side == "steps":
            assert routes.rollout()["route"] == "per-step", tag
        else:
            routes.check_rollout(dict(expect, wgs=N, n_runs=1), f"{tag} reference side")
        assert _status0(a_p) == 0 and _status0(a_s) == 0, (tag, it)
        a_p.check_rollout_status()
        tg._assert_twins(a_p, e_p, a_s, e_s, (tag, it))
        if it == 0:      # (the planes are the twins': equal already; this says that episodes did end inside the rollout)
            assert a_p.rollout_buffer.dones.sum().item() >= N, (tag, a_p.rollout_buffer.dones.sum().item())
    return got


def _gran(N, obs):
    return N * (2 * obs + 4) <= 256 * 12      # record mode: at most 12 exchange words per thread


# ---- constraint net, training statistics: the N ladder (N = 128 with training statistics is the wide kernel's: see the frozen case) ----
@pytest.mark.parametrize("N,T", [(1, 40), (3, 33), (8, 24), (33, 27), (64, 32), (96, 24)])
def test_constraint_net_chain_equals_per_step_launches(N, T):
    got = _compare(_cn_pair("hc", N, T), T, N, _ONE, f"hc {N} cn")
    assert bool(got["pick"] & routes.PICK_GRAN) == _gran(N, 18) and not got["pick"] & routes.PICK_ANALYTIC


# ---- frozen statistics (`training` off): no moments, no running returns; 128 envs = the largest grid, flag exchange ----
@pytest.mark.parametrize("N,T", [(8, 30), (128, 24)])
def test_frozen_statistics_chain_equals_per_step_launches(N, T):
    got = _compare(_cn_pair("hc", N, T, norm=dict(training=False)), T, N, _ONE, f"hc {N} frozen")
    assert bool(got["pick"] & routes.PICK_GRAN) == _gran(N, 18)


# ---- one normalisation off at a time ----
@pytest.mark.parametrize("off", ["norm_obs", "norm_reward", "norm_cost"])
def test_one_normalisation_off_chain_equals_per_step_launches(off):
    N, T = 33, 26
    _compare(_cn_pair("hc", N, T, norm={off: False}), T, N, _ONE, f"hc {N} {off} off")


# ---- the cost forms: an analytic cost and the null cost (no cost-net register image), and a chain without a cost ----
@pytest.mark.parametrize("cost", ["torque", "null", "none"])
def test_cost_forms_chain_equals_per_step_launches(cost):
    N, T = 64, 25
    pair = _costless_pair("hc", N, T) if cost == "none" else _analytic_pair("hc", N, T, cost)
    got = _compare(pair, T, N, _ONE, f"hc {N} cost {cost}")
    if cost != "none":
        assert got["pick"] & routes.PICK_ANALYTIC      # (the instantiations without a cost-net register image)
    if cost == "torque":
        assert 0.0 < float(pair[0][0].rollout_buffer.orig_costs.mean().item()) < 1.0
    else:
        assert float(pair[0][0].rollout_buffer.orig_costs.abs().max().item()) == 0.0


# ---- the raw-reward plane (MON instantiation) ----
def test_monitor_chain_equals_per_step_launches():
    N, T = 8, 36
    pair = _cn_pair("hc", N, T, agent_kwargs=dict(episode_stats=True))
    got = _compare(pair, T, N, _ONE, f"hc {N} mon")
    assert got["pick"] & routes.PICK_MON
    (a_p, _), (a_s, _) = pair
    assert torch.equal(a_p._mon["raw_rewards"], a_s._mon["raw_rewards"]) and float(a_p._mon["raw_rewards"].abs().sum().item()) > 0.0


# ---- a discrete head (LapGridWorld shapes: obs 1, two actions, no normalisation) ----
def test_discrete_head_chain_equals_per_step_launches():
    N, T = 8, 40
    _compare(_lgw_pair(N, T), T, N, _ONE, f"lgw {N}")


# ---- AntWall widths: obs 113 (OCT 8), 8 actions, a two-layer constraint net ----
def test_antwall_width_chain_equals_per_step_launches():
    N, T = 8, 24
    got = _compare(_cn_pair("ant", N, T), T, N, _ONE, f"ant {N}")
    assert got["pick"] & routes.PICK_GRAN


# ---- the phase-timer instantiation computes what the production one computes ----
def test_profiled_chain_equals_the_production_chain():
    N, T = 33, 28
    _compare(_cn_pair("hc", N, T), T, N, _ONE, f"hc {N} prof", steps_side="auto", prof=True)


# ---- the phase-timer words are read from the kernel family that ran last ----
def _timer_words(entry, n, *args):
    import ctypes
    from icrl_amd import _lib
    out = (ctypes.c_ulonglong * n)()
    _lib.check(getattr(_lib.lib(), entry)(out, *args), entry)
    return list(out)


def test_phase_timers_are_read_from_the_family_that_ran_last():
    """Three profiled rollouts in one process, one per kernel family that writes timer words (g_rollout_prof, g_rollout_prof_wide and
    g_wide_trace of csrc/rollout.hip; no other test reads the icrl_debug_rollout_* entry points, the tools only print them): behind each,
    the step count among the words is this call's T — the three T differ, so the words of an earlier call cannot pass — and the timers
    beside it have run.  The trace check is the weakest: its first word is only known to be non-zero once a profiled family has run."""
    torch.cuda.synchronize()
    for kernel, N, T, route, entry, t_words in (("auto", 4, 6, "persistent", "icrl_debug_rollout_profile", (3,)),
                                                ("wide", 24, 7, "wide", "icrl_debug_rollout_profile_wide", (5, 13)),
                                                ("multi", 24, 9, "multi", "icrl_debug_rollout_profile_wide", (5, 13))):
        (agent, env), _ = _cn_pair("hc", N, T)
        agent.rollout_kernel, agent.profile_phases = kernel, 1
        agent._setup_learn(N * T)
        agent.collect_rollouts(env, None, agent.rollout_buffer, T, "cost", noise=_noise(agent, T, N, 1)[0])
        got = routes.check_rollout(dict(route=route, n_runs=1, launches=1), f"profiled {kernel}")
        if route == "multi":
            assert got["envs_per_wg"] == 4 and got["wgs"] == 6, got
        torch.cuda.synchronize()
        agent.check_rollout_status()
        words = _timer_words(entry, 8 if route == "persistent" else 16)
        print(f"[timers] {kernel} N={N} T={T}: {words}")
        for w in t_words:
            assert words[w] == T, (kernel, w, words)
            block = words[:3] + words[4:7] if route == "persistent" else words[w - 5:w]
            assert any(block), (kernel, w, words)
        if route != "multi":
            trace = _timer_words("icrl_debug_rollout_trace_wide", 4 * N, N)
            print(f"[timers] {kernel} trace: {trace[:8]}")
            assert trace[0] != 0, (kernel, trace[:8])
