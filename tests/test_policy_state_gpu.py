"""GPU: every copy of the Gaussian action head (csrc/rollout.hip: load_pol_regs / policy_forward_block, the wide kernel's natural-layout
copy, the multi-env kernel's CST_* constants, policy_rows_kernel; csrc/generic.h and generic.hip; csrc/ppo_train*.hip) at a TRAINED
policy state (tests/helpers/policy_states.py): log_std away from 0 and different per action, an action head whose means cross the action
bounds.  At the state PPOLagrangian.__init__ leaves (sigma = 1, log sigma = 0, 2 sigma^2 = 2 sigma = 2, means of ~0.005) a head that
drops -log sigma, confuses sigma with sigma^2, reads log_std[0] for every action, forgets to refresh its constants after log_std's Adam step
or skips the clip of the deterministic action passes every other kernel-level test.

Every test asserts the conditions C1..C6 of helpers/policy_states.py on its inputs from the ORACLE's buffers before a kernel runs, and prints
its worst plane in units of its bound.  Bounds are those of the tests mirrored, unchanged: rollouts rtol 5e-4 / atol 5e-5, forward rtol 1e-5 /
atol 2e-6, samplers _assert_sample, updates ADAM_DEV_BOUND.  The forward bound was sized at sigma = 1; at sigma ~ 0.35 an error of a mean
enters the log-prob 1 / sigma^2 ~ 8 times larger.  Measured on the oracle (float32 against float64 on the cases' inputs, largest per plane
over every per-row case, in units of the forward bound): values 0.17, log-prob 0.07, entropy 0.01, actions 0.32 (`ref`, sampled) / 0.21
(`shaped`, deterministic) — three times each stays within the bound, so no bound is re-derived.

Worst deviation per family on MI355X, in units of its bound: per-row entry points 0.27 (`ref`, hc 1000, cost values); fused rollouts 0.016
under `shaped`, 0.45 under `ref` (multi hc 300x12, reward advantages); evaluate_actions after a rollout 0.000 (bit-equal log-probs), on the
oracle's buffer 0.24; updates 0.75 of ADAM_DEV_BOUND (ant 3x50 B100 set B), 0.30 under `ref`.  Wall time of this file: 17 s.

Mutations, each built into one kernel copy and run once (failed tests of this file / the kernel's earlier tests):
  lp without -lsd, policy_forward_block                          21 failed (rows < 64, fused auto / wide / steps, evaluate path, batch 8x32) / green
  i2v = 2 sd, multi-env CST_I2V (shared with policy_rows_kernel) 19 failed (fused multi, rows >= 64, evaluate path, batch 96x16) / green
  act = mean + noise sd sd, policy_forward_block                 15 failed (fused auto / wide / steps, sampler, batch 8x32) / green
      (rollout_wide_kernel has no Gaussian head of its own: it calls policy_forward_block)
  log_std[0] for every action, policy_rows_kernel                11 failed (rows >= 64, evaluate path) / green
  entl without lsd, generic.h                                    6 failed (rows wide / trunk / deep / trunk-only / bare) / green
  g2 = dd^2 sqrt(iv) - 1, ppo_train_quarters2.hip                4 failed (ant 24x16 B128, ant 3x50 B100, sets A and B) / green
  refresh_gauss only before the first step, ppo_train_halves.hip 12 failed (every hc case) / 7 earlier `halves` tests fail as well: a stale sigma
      after log_std's first Adam step is already visible at log_std = 0; no case at a larger learning rate was needed (and none exists
      on hc 8x32 B64 E3: at every rate that moves log_std by 0.05, 4.5e-3 .. 2e-2, clip_fraction leaves check_trace's [0.3, 0.9])
  no clip when deterministic, policy_forward_block               5 failed (sampler 64-wide, rows 33 / 63) / green
  run 0's parameter block in both batched rollout kernels        2 failed (8x32, 96x16) / test_batched_runs_equal_solo_runs fails too (the
      mutation takes run 0's whole block, not log_std alone: log_std has no pointer of its own in the kernel's arguments)
test_sampling_and_evaluation_vs_port is repeated with its own scale and the half of the condition two classes can meet (the largest of two
probabilities is never below 0.5): pmax >= 0.9 in >= 10 % of the rows and pmax <= 0.6 in >= 10 % (helpers/policy_states.py: lgw_sampler_case).
Samplers, worst plane in units of _assert_sample's bounds: 0.42 (`ref`, sampled actions; chained, pass-by-pass and host alike), 0.09 deterministic;
LGW / CLGW: 0 of 600 actions differ from the oracle's.
"""
import os

import numpy as np
import pytest
import torch

from helpers import norm_cases as nc, policy_states as ps, routes
from oracle import loop as o_loop, nets as o_nets

pytestmark = pytest.mark.gpu

RTOL, ATOL = ps.ROLL_RTOL, ps.ROLL_ATOL
F_RTOL, F_ATOL = ps.FWD_RTOL, ps.FWD_ATOL


def _report(tag, worst):
    top = max(worst, key=worst.get)
    print(f"[policy state] {tag}: worst plane {top} at {worst[top]:.3f} of the bound")


def _cmp(tag, pairs, rtol, atol):
    """pairs: name -> (got, ref); prints the worst plane in units of the bound, then asserts each."""
    worst = {k: nc.in_bounds(np.asarray(g).reshape(-1), np.asarray(r).reshape(-1), rtol, atol) for k, (g, r) in pairs.items()}
    _report(tag, worst)
    for k, (g, r) in pairs.items():
        g, r = np.asarray(g).reshape(-1), np.asarray(r).reshape(-1)
        assert np.allclose(g, r, rtol=rtol, atol=atol), (tag, k, np.abs(g - r).max(), worst[k])


# ---- a. per-row entry points ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,pstate", ps.ROW_CASES, ids=[f"{k}-{n}-{s}" for k, n, s in ps.ROW_CASES])
def test_policy_rows_vs_oracle_at_state(kind, n, pstate):
    """test_policy_rows_kernel_vs_oracle / test_policy_forward_vs_oracle at a trained state: evaluate_actions (values, log-prob, entropy),
    forward with noise, forward(deterministic=True) and last_clipped of both calls against the oracle (policy_forward_kernel below 64
    rows, policy_rows_kernel from 64, policy_generic_kernel for the other architectures)."""
    from icrl_amd.policies import ActorTwoCriticsPolicy
    from icrl_amd import spaces
    op, net_arch, od, ad, fresh, obs, act, noise = ps.check_rows(kind, n, pstate)      # C1, C5, C6 (asserted inside)
    torch.manual_seed(11)
    pol = ActorTwoCriticsPolicy(spaces.Box(-np.inf, np.inf, (od,), np.float64), spaces.Box(-1, 1, (ad,), np.float32), **(dict(net_arch=net_arch) if net_arch else {}))
    assert all(torch.equal(v, fresh[k]) for k, v in pol.state_dict().items())      # the product draws the oracle's fresh policy
    pol.load_state_dict(op.state_dict())
    t = torch.as_tensor
    with torch.no_grad():
        e = op.evaluate_actions(t(obs), t(act))
        f = op.forward(t(obs), noise=t(noise))
        d = op.forward(t(obs), deterministic=True)
    num = lambda xs: [x.cpu().numpy() if x.is_cuda else x.numpy() for x in xs]
    got = num(pol.evaluate_actions(obs, act))
    pairs = {"eval/" + k: (g, r) for k, g, r in zip(("reward_values", "cost_values", "log_prob", "entropy"), got, num(e))}
    got = num(pol.forward(obs, deterministic=False, noise=noise))
    pairs.update({"forward/" + k: (g, r) for k, g, r in zip(("actions", "reward_values", "cost_values", "log_prob"), got, num(f))})
    pairs["forward/last_clipped"] = (pol.last_clipped.cpu().numpy(), np.clip(f[0].numpy(), -1, 1))
    got = num(pol.forward(obs, deterministic=True))
    pairs.update({"deterministic/" + k: (g, r) for k, g, r in zip(("actions", "reward_values", "cost_values", "log_prob"), got, num(d))})
    clipped = pol.last_clipped.cpu().numpy()
    pairs["deterministic/last_clipped"] = (clipped, np.clip(d[0].numpy(), -1, 1))
    _cmp(f"rows {kind} {n} {pstate}", pairs, F_RTOL, F_ATOL)
    assert np.abs(clipped).max() == 1.0 and (clipped == 1.0).sum() >= ps.DET_COUNT and (clipped == -1.0).sum() >= ps.DET_COUNT
    # predict() is the clipped action
    assert torch.equal(pol.predict(obs, deterministic=True)[0], pol.last_clipped) and np.array_equal(pol.last_clipped.cpu().numpy(), clipped)


# ---- b. fused rollouts against the port, c. their log-probs against the evaluate path ----------------------------------------------------------
def _rollout(kernel, kind, N, T, pstate, **how):
    """conditions C1..C4 from the oracle, then the GPU twin's rollout; returns (oracle case, agent, env)."""
    import test_normalizer_settings_gpu as tn
    wide = kernel == "wide-policy"
    arch = nc.WIDE_ARCH if wide else None
    o, counters = ps.rollout_case(kind, N, T, pstate, net_arch=arch, **how)
    assert o["buf"].dones.sum() == N
    ps.check_rollout(o, counters, RTOL, ATOL)
    agent, env = tn._gpu_chain(kind, N, T, {}, o, kernel, arch)
    agent.collect_rollouts(env, None, agent.rollout_buffer, T, "cost", noise=torch.as_tensor(o["noise"], device="cuda"))
    agent.check_rollout_status()
    return o, agent, env


@pytest.mark.parametrize("kernel,kind,N,T,pstate", ps.FUSED, ids=[f"{k}-{e}-{n}x{t}-{s}" for k, e, n, t, s in ps.FUSED])
def test_fused_rollout_vs_port_at_state(kernel, kind, N, T, pstate):
    """test_fused_rollout_vs_port_under_settings' comparison (same planes, same statistics checks, same bound, default normaliser) with the
    policy at a trained state."""
    import test_normalizer_settings_gpu as tn
    o, agent, env = _rollout(kernel, kind, N, T, pstate)
    b, norm, rb = o["buf"], o["norm"], agent.rollout_buffer
    _cmp(f"fused {kernel} {kind} {N}x{T} {pstate}", {k: (getattr(rb, k).cpu().numpy(), getattr(b, k)) for k in tn._PLANES}, RTOL, ATOL)
    assert np.allclose(env.obs_rms.mean, norm.obs_rms.mean, rtol=1e-5, atol=1e-6)
    assert np.allclose(env.obs_rms.var, norm.obs_rms.var, rtol=1e-5, atol=1e-8)
    assert abs(env.ret_rms.var - norm.ret_rms.var) <= 1e-5 * max(1.0, norm.ret_rms.var)
    assert abs(env.cost_rms.var - norm.cost_rms.var) <= 1e-5 * max(1.0, norm.cost_rms.var)
    assert env.obs_rms.count == norm.obs_rms.count


@pytest.mark.parametrize("kernel,kind,N,T,pstate", ps.EVAL_AFTER, ids=[f"{k}-{e}-{n}x{t}-{s}" for k, e, n, t, s in ps.EVAL_AFTER])
def test_rollout_log_probs_equal_the_evaluate_path(kernel, kind, N, T, pstate):
    """A rollout's own log-probs are sum(-eps^2 / 2 - log sigma_a) - const: they see log_std only through its sum.  evaluate_actions on the
    rollout's observations and stored actions must reproduce log_probs and both value planes within the forward bound — which ties the
    sigma of the sampling kernels to the sigma of the density kernels, per action — and equal the oracle's evaluate_actions on the
    oracle's buffer."""
    o, agent, env = _rollout(kernel, kind, N, T, pstate)
    b, rb, op = o["buf"], agent.rollout_buffer, o["port"].policy
    od, ad = b.observations.shape[-1], b.actions.shape[-1]
    # C6 on the stored actions: a uniform sigma in the density gives other log-probs
    ou = o_nets.TwoCriticPolicy.__new__(o_nets.TwoCriticPolicy)
    ou.__dict__.update(op.__dict__)
    ou.params = {k: v.detach().clone() for k, v in op.params.items()}
    ou.params["log_std"] = torch.full_like(ou.params["log_std"], float(ou.params["log_std"].double().mean()))
    ps.check_density(op, ou, b.observations.reshape(-1, od), b.actions.reshape(-1, ad), F_RTOL, F_ATOL)
    v_r, v_c, lp, _ = [x.cpu().numpy().reshape(-1) for x in agent.policy.evaluate_actions(rb.observations.reshape(-1, od), rb.actions.reshape(-1, ad))]
    pairs = {"log_probs": (lp, rb.log_probs.cpu().numpy()), "reward_values": (v_r, rb.reward_values.cpu().numpy()),
             "cost_values": (v_c, rb.cost_values.cpu().numpy())}
    o_vr, o_vc, o_lp, _ = [x.numpy().reshape(-1) for x in _no_grad(op.evaluate_actions, torch.as_tensor(b.observations.reshape(-1, od)),
                                                                   torch.as_tensor(b.actions.reshape(-1, ad)))]
    o_pairs = {"log_probs": (o_lp, b.log_probs), "reward_values": (o_vr, b.reward_values), "cost_values": (o_vc, b.cost_values)}
    _cmp(f"oracle evaluate after its rollout {kind} {N}x{T} {pstate}", o_pairs, F_RTOL, F_ATOL)      # (the oracle's two paths agree)
    _cmp(f"evaluate after rollout {kernel} {kind} {N}x{T} {pstate}", pairs, F_RTOL, F_ATOL)
    # ... and the GPU's evaluate_actions on the ORACLE's buffer equals the oracle's
    v_r, v_c, lp, _ = [x.cpu().numpy().reshape(-1) for x in agent.policy.evaluate_actions(b.observations.reshape(-1, od), b.actions.reshape(-1, ad))]
    _cmp(f"evaluate on the oracle's buffer {kind} {N}x{T} {pstate}", {"log_probs": (lp, o_lp), "reward_values": (v_r, o_vr), "cost_values": (v_c, o_vc)},
         F_RTOL, F_ATOL)


def _no_grad(fn, *a):
    with torch.no_grad():
        return fn(*a)


# ---- d. kernel against kernel, bit for bit ------------------------------------------------------------------------------------------------------
def _twin_conditions(kind, N, T, pstate="shaped", **how):
    o, counters = ps.rollout_case(kind, N, T, pstate, **how)
    ps.check_rollout(o, counters, RTOL, ATOL)


@pytest.mark.parametrize("kernel", ["auto", "wide", "multi"])
@pytest.mark.parametrize("kind,N,T", [("hc", 7, 33), ("hc", 130, 24), ("hc", 300, 12), ("ant", 32, 20)])
def test_one_launch_rollouts_equal_per_step_launches_at_state(kind, N, T, kernel):
    """test_persistent_rollout_equals_per_step_launches with both chains under `shaped`."""
    import test_rollout_gpu as tr
    _twin_conditions(kind, N, T, seed=13, noise_seed=8, rollouts=2)      # the oracle's run of the body's first rollout
    tr.test_persistent_rollout_equals_per_step_launches(kind, N, T, kernel=kernel, policy_state="shaped")


def test_generic_shape_rollout_equals_python_loop_at_state():
    import test_rollout_gpu as tr
    from helpers.arches import ARCHES
    _twin_conditions("hc", 12, 40, net_arch=ARCHES["trunk"], seed=11, noise_seed=3, rollouts=2, cross_end=False)
    tr.test_generic_shape_rollout_equals_python_loop("hc", "trunk", 12, policy_state="shaped")


@pytest.mark.parametrize("kind,N,T", [("hc", 7, 24), ("ant", 16, 12)])
def test_host_rollout_equals_device_rollout_at_state(kind, N, T):
    """host_step_kernel against the per-step launches (which section b ties to the oracle), both chains under `shaped`: bit-identical."""
    import test_host_rollout_gpu as th
    _twin_conditions(kind, N, T, seed=5, noise_seed=8, rollouts=2)
    th.test_host_rollout_equals_device_rollout(kind, N, T, True, True, False, policy_state="shaped")


# ---- e. samplers ------------------------------------------------------------------------------------------------------------------------------------
_N_EP = 3


def _eval_env(train_env, env_id="HCWithPosTest-v0"):
    from icrl_amd import utils
    from icrl_amd.vec_env import VecNormalizeWithCost, sync_envs_normalization
    eenv = VecNormalizeWithCost(utils.make_vec_env(env_id, 1, 3, dummy_vec_env=True), training=False, norm_reward=False, norm_cost=False)
    sync_envs_normalization(train_env, eenv)
    return eenv


_SAMPLE_BOUNDS = (("orig_obs", 1e-4, 2e-5), ("obs", 1e-4, 2e-4), ("actions", 1e-4, 2e-5), ("ep_rewards", 1e-5, 1e-3))      # _assert_sample's


def _sample(got, want, what):
    """prints the worst plane of a sampler's result in units of _assert_sample's bounds, then runs _assert_sample itself, unchanged."""
    import test_normalizer_settings_gpu as tn
    if list(got[4]) == list(want[4]):
        num = lambda x: x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
        _report(what, {k: nc.in_bounds(num(g), w, rtol, atol) for (k, rtol, atol), g, w in zip(_SAMPLE_BOUNDS, got, want)})
    tn._assert_sample(got, want, what)


@pytest.mark.parametrize("shape,pstate", ps.SAMPLERS, ids=["64-wide-ref", "trunk-shaped"])
def test_samplers_at_state(shape, pstate):
    """sample_from_agent (chained launch), the pass-by-pass launch (sample_episodes_kernel; `trunk`: sample_episodes_generic_kernel), a host
    eval env (64-wide policy: host_episode_kernel) and evaluate_policy with deterministic=False / True on HCWithPosTest against the oracle's
    loops, with the policy at a trained state; deterministic episodes also row by row."""
    import tests.helpers.host_envs  # noqa: F401  (registers the Host* ids)
    import test_normalizer_settings_gpu as tn
    from icrl_amd import utils
    c = ps.sampler_case(shape, pstate, _N_EP)      # the oracle's side; C1 and C5 (on its deterministic episodes) asserted inside
    o, noise = c["o"], c["noise"]
    agent, env = tn._gpu_chain("hc", 4, 32, {}, o, net_arch=c["net_arch"], seed=c["seed"])
    agent.collect_rollouts(env, None, agent.rollout_buffer, 32, "cost", noise=torch.as_tensor(o["noise"], device="cuda"))
    agent.check_rollout_status()
    eenv = _eval_env(env)
    norm = o["norm"]
    assert np.allclose(eenv.obs_rms.mean, norm.obs_rms.mean, rtol=1e-5, atol=1e-6) and np.allclose(eenv.obs_rms.var, norm.obs_rms.var, rtol=1e-5, atol=1e-8)
    _sample(utils.sample_from_agent(agent, eenv, _N_EP, noise=noise), c["want"], f"sample_from_agent {shape or '64-wide'} {pstate}")
    run = utils._run_episodes(agent, _eval_env(env), _N_EP, False, noise, parallel=True)
    assert isinstance(run, utils.EpisodeRun)
    _sample(utils.sample_result(run), c["want"], f"pass by pass {shape or '64-wide'} {pstate}")
    run = utils._run_episodes(agent, _eval_env(env), _N_EP, True, None, parallel=False, chain=True)
    _sample(utils.sample_result(run), c["want_det"], f"deterministic episodes {shape or '64-wide'} {pstate}")
    acts = utils.sample_result(run)[2].cpu().numpy()
    assert np.abs(acts).max() == 1.0 and (acts == 1.0).sum() >= ps.DET_COUNT and (acts == -1.0).sum() >= ps.DET_COUNT
    for det, want in ((False, c["eval"]), (True, c["eval_det"])):
        mean_r, std_r = utils.evaluate_policy(agent, _eval_env(env), _N_EP, deterministic=det, noise=None if det else noise)
        print(f"[policy state] evaluate_policy {shape or '64-wide'} {pstate} deterministic={det}: {mean_r:.6f} +- {std_r:.6f} (oracle {want[0]:.6f} +- {want[1]:.6f})")
        assert abs(mean_r - want[0]) < 1e-3 * max(1, abs(want[0])) and abs(std_r - want[1]) < 1e-3 * max(1, abs(want[1])), (det, mean_r, std_r, want)
    if shape is None:
        for det, want in ((False, c["want"]), (True, c["want_det"])):
            henv = _eval_env(env, "HostHCWithPosTest-v0")
            hrun = utils._run_episodes(agent, henv, _N_EP, det, None if det else noise, False)
            assert isinstance(hrun, utils.HostEpisodeRun)
            _sample(utils.sample_result(hrun), want, f"host eval env deterministic={det} {shape or '64-wide'} {pstate}")
            henv.close()


# ---- f. batched launches read each run's own policy ----------------------------------------------------------------------------------------------
_BATCH_STATES = (None, "shaped", "ref")


@pytest.mark.parametrize("N,T", [(8, 32), (96, 16)])      # rollout_persistent_batch_kernel / rollout_multi_batch_kernel
def test_batched_rollout_reads_each_runs_own_policy(N, T):
    """three hc runs with the same seeds and noise but policy states fresh, `shaped` and `ref` through ONE icrl_rollout_collect_batch call: each
    run's buffer and statistics equal, bit for bit, the same run launched alone (test_batched_launch_reads_each_runs_own_normaliser's harness)."""
    import test_cpg_seed_batch_gpu as tb
    import test_rollout_gpu as tr
    from icrl_amd import _lib
    from icrl_amd.structs import RolloutJobT, addr, p
    # ---- conditions, from the oracle: C1..C4 for the two trained states, and three action planes that differ pairwise
    for s in _BATCH_STATES[1:]:
        _twin_conditions("hc", N, T, pstate=s, noise_seed=8)
    os_ = [nc.oracle_buf("hc", N, T, {}, noise_seed=8, policy_state=s) for s in _BATCH_STATES]
    for i in range(3):
        for j in range(i):
            assert nc.in_bounds(os_[i]["buf"].actions, os_[j]["buf"].actions, RTOL, ATOL) >= ps.MIN_SHIFT, (i, j)
    # ---- the launches
    pairs = [tr._pair_of_agents(N, T, 7, policy_state=s) for s in _BATCH_STATES]
    noise = torch.as_tensor(os_[0]["noise"], device="cuda")
    for (a_s, e_s, _), (a_b, e_b, _) in pairs:
        a_s.rollout_kernel = "multi"
        for a, e in ((a_s, e_s), (a_b, e_b)):
            a._setup_learn(N * T)
            e.unwrapped.t_ep.fill_(os_[0]["start"])
        a_s.collect_rollouts(e_s, None, a_s.rollout_buffer, T, "cost", noise=noise)
        routes.check_rollout("multi" if N >= 20 else "persistent", f"solo {N}")      # (fewer than 20 hc envs: the forced multi-env kernel declines)
        a_s.check_rollout_status()
    agents = [pair[1][0] for pair in pairs]
    jobs = [a._rollout_begin(None, a.rollout_buffer, T, noise) for a in agents]
    arr = (RolloutJobT * 3)(*[RolloutJobT(addr(j["env"]), addr(j["nm"]), addr(j["pol"]), addr(j["cn"]), addr(j["buf"]), addr(j["ag"]), p(j["noise"]))
                              for j in jobs])
    a0 = agents[0]
    ws = torch.empty(2 * 3 * _lib.BATCH_ARGS_BYTES, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().icrl_rollout_collect_batch(3, arr, p(a0._alow), p(a0._ahigh), float(a0.reward_gamma), float(a0.reward_gae_lambda),
                                                     float(a0.cost_gamma), float(a0.cost_gae_lambda), 1, p(ws), ws.numel(), _lib.current_stream()),
               "icrl_rollout_collect_batch")
    # (3 x N workgroups within the compute units: one workgroup per env; beyond: the multi-env kernel, 8 envs per workgroup)
    few = 3 * N <= torch.cuda.get_device_properties(0).multi_processor_count
    routes.check_rollout(dict(route="persistent-batch", minw=1) if few else dict(route="multi-batch", envs_per_wg=8), f"3 x {N}")
    for a, j in zip(agents, jobs):
        a._rollout_end(j, a.env, None, a.rollout_buffer, T)
    torch.cuda.synchronize()
    for r, ((a_s, e_s, _), (a_b, e_b, _)) in enumerate(pairs):
        a_b.check_rollout_status()
        tb._assert_identical(a_b, e_b, a_s, e_s, r)
    planes = [a.rollout_buffer.actions.cpu().numpy() for a in agents]
    assert all(not np.array_equal(planes[i], planes[j]) for i in range(3) for j in range(i))
    # the solo runs are the oracle's (the batch is tied to them bit for bit)
    for o, (pair_s, _) in zip(os_, pairs):
        got = pair_s[0].rollout_buffer
        for k in ("actions", "log_probs"):
            assert np.allclose(getattr(got, k).cpu().numpy().reshape(T, N, -1), getattr(o["buf"], k).reshape(T, N, -1), rtol=RTOL, atol=ATOL), k


def test_batched_update_reads_each_runs_own_policy():
    """the same three states through ONE launch_trains call, set A on the banded buffer of each state: parameters, both Adam moments and
    stats[0:11] of each run equal, bit for bit, the run trained alone (test_batched_update_reads_each_runs_own_hyper_parameters' harness)."""
    from helpers import ppo_hparam_cases as H
    from icrl_amd.ppo_lag import PPOLagrangian
    from icrl_amd.seed_batch import launch_trains
    from icrl_amd import _lib
    from icrl_amd.vec_env import HipSynthVecEnv, VecCostWrapper, VecNormalizeWithCost
    N, T, B, E = 8, 32, 64, 2
    for s in _BATCH_STATES[1:]:      # C1 and C6 of the two trained runs, from the oracle, before anything is built (check_trace: in agent())
        ps.check_update_density("hc", N, T, B, E, "A", s)

    def agent(pstate):
        env = VecNormalizeWithCost(VecCostWrapper(HipSynthVecEnv(N, "hc", 0)))
        a = PPOLagrangian("TwoCriticsMlpPolicy", env, n_steps=T, seed=0, batch_size=B, n_epochs=E, target_kl=None, learning_rate=3e-4, clip_range=0.2,
                          **H.hparams("A"))
        if pstate is not None:
            a.policy.load_state_dict(ps.state(pstate, a.policy.state_dict(), 6))
        case = H.oracle_case("hc", "", N, T, B, E, "A", a.policy.state_dict(), nu=a.dual.nu().item(), state=pstate)
        H.check_trace(case["trace"], case["hp"], n_steps=E * (-(-N * T // B)))
        rb = a.rollout_buffer
        for k, v in case["buf"].items():
            getattr(rb, k).copy_(torch.as_tensor(np.asarray(v, np.float32)).reshape(getattr(rb, k).shape))
        rb.full = True
        return a, case

    def snapshot(a):
        pol = a.policy
        return [t.cpu().numpy().copy() for t in (pol.params, pol.exp_avg, pol.exp_avg_sq, a._train_ws["stats"][:11])]

    solo = []
    for s in _BATCH_STATES:
        a, case = agent(s)
        a.train(perms=case["perms"])
        solo.append(snapshot(a))
    assert all(not np.array_equal(solo[i][0], solo[j][0]) for i in range(3) for j in range(i))
    agents, jobs = [], []
    for s in _BATCH_STATES:
        a, case = agent(s)
        agents.append(a)
        jobs.append(a._train_begin(case["perms"]))
    args_ws = torch.empty(len(agents) * _lib.BATCH_ARGS_BYTES, dtype=torch.uint8, device=agents[0].device)
    launch_trains(agents, jobs, args_ws)
    torch.cuda.synchronize()
    for i, (a, j) in enumerate(zip(agents, jobs)):
        got = snapshot(a)
        assert float(a._train_ws["stats"][11]) == 0
        for name, g_, s_ in zip(("params", "exp_avg", "exp_avg_sq", "stats"), got, solo[i]):
            assert np.array_equal(g_, s_), (_BATCH_STATES[i], name, np.abs(g_ - s_).max())
        a._train_end(j)


# ---- g. update kernels against the oracle ---------------------------------------------------------------------------------------------------------
def _update_cases():
    import test_ppo_train_gpu as tp
    return ps.update_cases(tp._hp_cases())


@pytest.mark.parametrize("kind,N,T,B,E,hset,train_kernel,pstate", _update_cases())
def test_train_vs_oracle_at_state(kind, N, T, B, E, hset, train_kernel, pstate):
    """test_train_hparams_vs_oracle (same _compare_with_oracle, same bounds; check_trace asserted from the oracle's trace first) starting from
    a trained state: d log-prob / d log_std = diff^2 / sigma^2 - 1, the entropy's sum of log sigma and the Gaussian constants refreshed
    after each Adam step of log_std, in every update-kernel family."""
    import test_ppo_train_gpu as tp
    ps.check_update_density(kind, N, T, B, E, hset, pstate)      # C1, C6 on the case's actions
    tp.test_train_hparams_vs_oracle(kind, N, T, B, E, hset, train_kernel, policy_state=pstate)


def test_ant_chunk_by_chunk_form_at_128_rows_at_state():
    """the 128-row AntWall case under `shaped` through ppo_train_quarters.hip where ppo_train_quarters2.hip would run
    (ICRL_QUARTERS_PASSES=1; child process: the switch is read once per process)."""
    import subprocess, sys
    env = dict(os.environ, ICRL_QUARTERS_PASSES="1")
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", "test_train_vs_oracle_at_state and ant-24-16-128-2-A-None-shaped",
                          "-p", "no:cacheprovider"], env=env, capture_output=True, text=True, timeout=300, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert out.returncode == 0 and "1 passed" in out.stdout, out.stdout[-3000:]


# ---- h. categorical head -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("O,A,N,T,B,E,ent", ps.LGW_CASES)
def test_categorical_update_vs_oracle_with_a_peaked_head(O, A, N, T, B, E, ent):
    """test_categorical_update_vs_oracle with action_net.weight x LGW_K: rows with a near-certain class (>= 0.9) beside rows without a
    favourite (<= 0.5), asserted on the oracle inside the case."""
    import test_lap_grid_gpu as tl
    tl._categorical_case(O, A, N, T, B, E, ent, False, head_scale=ps.LGW_K)


def test_sampling_and_evaluation_vs_port_with_a_peaked_head():
    """test_sampling_and_evaluation_vs_port (sample_from_agent on LGW-v0, sequential and parallel streams; evaluate_policy on CLGW-v0) with
    action_net.weight x LGW_SAMPLER_K: a softmax saturated in a fifth of the rows and near-uniform in a third, drawn by inverse CDF — the
    discrete branch of policy_forward_block in the chained and the pass-by-pass samplers.  The oracle's side (lgw_sampler_case) asserts the two
    shares, that no uniform lies within 1e-5 of a class boundary — so every action must equal the oracle's, where the fresh-head test allows
    0.5 % to differ — and that the evaluation episodes end early at different steps."""
    import test_lap_grid_gpu as tl
    from icrl_amd import utils
    c = ps.lgw_sampler_case()
    agent, env, cn = tl._lgw_agent(2, 32, ps.LGW_SAMPLER_SEED)
    assert all(torch.equal(v, c["fresh"][k]) for k, v in agent.policy.state_dict().items())      # the product draws the oracle's fresh policy
    agent.policy.load_state_dict(c["sd"])
    p_oo, p_o, p_a, p_r, p_l = c["want"]
    senv = utils.make_eval_env("LGW-v0", False, normalize_obs=False)
    for parallel in (False, True):
        oo, o, a, r, l = utils.sample_from_agent(agent, senv, 3, noise=c["u"], parallel=parallel)
        same = a.cpu().numpy().reshape(-1) == p_a.reshape(-1)
        print(f"[policy state] lgw sample_from_agent parallel={parallel}: {int((~same).sum())} of {same.size} actions differ from the oracle's "
              f"(smallest |u - boundary| on the oracle {c['margin']:.3g})")
        assert list(l) == list(p_l) == [200, 200, 200]
        assert same.all()
        assert np.array_equal(oo.cpu().numpy(), p_oo) and np.array_equal(o.cpu().numpy(), p_o) and np.allclose(r, p_r)
    eenv = utils.make_eval_env("CLGW-v0", False, normalize_obs=False)
    er, el = utils.evaluate_policy(agent, eenv, 10, deterministic=False, noise=c["u2"], return_episode_rewards=True)
    assert list(el) == c["lens"] and np.allclose(er, c["rews"]) and min(el) < 200
