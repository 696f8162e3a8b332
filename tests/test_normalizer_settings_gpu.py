"""GPU: the normaliser's clips, epsilon and gammas in every kernel that carries a copy of VecNormalizeWithCost's arithmetic
(csrc/rollout.hip: the per-step normaliser kernels, the persistent / wide / multi-env / generic-shape rollouts, the host-env step, the
frozen-statistics samplers, the batched launches, GAIL's un-normalise step) — at settings where each of them changes the result
(tests/helpers/norm_cases.py).  Every test asserts the conditions on its inputs from the ORACLE's buffers first: the clips are reached
on the sides the case claims, and the run differs from its counter-run (gammas swapped / default epsilon) by >= 50 comparison bounds.
"""
import numpy as np
import pytest
import torch

from helpers import norm_cases as nc, routes
from oracle import loop as o_loop, stats as o_stats

pytestmark = pytest.mark.gpu

RTOL, ATOL = 5e-4, 5e-5          # the bound of test_rollout_gpu.py::test_fused_rollout_vs_port, unchanged
TIGHT = nc.CASES["tight"]


# ---- a. per-step entry points, bit for bit against oracle.stats ------------------------------------------------------------------------------
def _oracle_steps(N, kw, seed):
    """reset + 5 steps of oracle.stats under kw on the inputs of the case (drawn from RandomState(seed)); per step the inputs, the
    outputs and the state that the kernel's is compared with."""
    rng = np.random.RandomState(seed)
    st = o_stats.NormState(N, 18, **kw)
    raw0 = rng.randn(N, 18) * 4
    out = dict(raw0=raw0, obs0=o_stats.norm_reset(st, raw0), steps=[])
    for _ in range(5):
        obs, rew = rng.randn(N, 18) * 7 + 1, rng.randn(N) * 3
        cost, done = rng.randn(N).astype(np.float32), rng.rand(N) < 0.2      # signed raw costs: both cost-clip sides occur
        oo, ro, co = o_stats.norm_step(st, obs, rew, cost, done)
        out["steps"].append(dict(obs=obs, rew=rew, cost=cost, done=done, obs_n=oo, rew_n=ro, cost_n=co, ret=st.ret.copy(), cost_ret=st.cost_ret.copy(),
                                 ret_var=float(st.ret_rms.var), cost_var=float(st.cost_rms.var), obs_var=st.obs_rms.var.copy()))
    return out


# the inputs' stream is seeded with N (as in test_vecnormalize_numpy_reduction_order); a size whose default seed misses one of the conditions
# below gets another seed here, never another condition (N = 1 has five costs in all: seed 1 puts none of them at the lower clip)
_STEP_SEEDS = {1: 2}


@pytest.mark.parametrize("case", list(nc.CASES))
@pytest.mark.parametrize("N", [1, 8, 128, 129, 1000, 3000])      # norm_step_small_kernel up to 128 envs, norm_step_kernel beyond
def test_per_step_entry_points(N, case):
    """icrl_vecnorm_reset / icrl_vecnorm_step (norm_reset_kernel, norm_step_small_kernel, norm_step_kernel) through env._norm_call:
    outputs, ret / cost_ret and the running variances equal oracle.stats bit for bit under every named setting."""
    from icrl_amd import _lib
    from icrl_amd.structs import p
    from icrl_amd.vec_env import HipSynthVecEnv, VecNormalizeWithCost, VecCostWrapper
    kw, full = nc.CASES[case], nc.settings(case)
    seed = _STEP_SEEDS.get(N, N)
    ref, counter = _oracle_steps(N, kw, seed), _oracle_steps(N, nc.counter_settings(case), seed)
    # ---- conditions on the inputs, from the oracle alone
    tight = full["clip_obs"] < nc.DEFAULTS["clip_obs"]
    pooled = lambda k: np.stack([s[k] for s in ref["steps"]])
    few = N < 128          # (few entries: at least one at each bound over the 5 steps instead of a share)
    if tight and full["norm_obs"]:
        nc.assert_share("reset obs", ref["obs0"], full["clip_obs"], count_only=few)
        nc.assert_share("obs", pooled("obs_n"), full["clip_obs"], count_only=few)
    elif tight:
        assert np.array_equal(ref["obs0"], ref["raw0"]) and np.abs(pooled("obs_n")).max() > full["clip_obs"]
    if tight and full["norm_reward"]:
        nc.assert_share("rew", pooled("rew_n"), full["clip_reward"], count_only=few)
    elif tight:
        assert np.array_equal(pooled("rew_n"), pooled("rew")) and np.abs(pooled("rew_n")).max() > full["clip_reward"]
    if tight and full["norm_cost"]:
        nc.assert_share("cost", pooled("cost_n"), full["clip_cost"], count_only=few)
    elif tight:
        assert np.array_equal(pooled("cost_n"), pooled("cost")) and np.abs(pooled("cost_n")).max() > full["clip_cost"]
    # the counter-run (gammas swapped / default epsilon) is another result: in the last step's discounted returns / in most outputs
    last, clast = ref["steps"][-1], counter["steps"][-1]
    if "epsilon" in kw:
        for k in ("obs_n", "rew_n", "cost_n"):
            assert np.mean(last[k] != clast[k]) > 0.9, k
    else:
        assert np.mean(last["ret"] != clast["ret"]) > 0.5 and np.mean(last["cost_ret"] != clast["cost_ret"]) > 0.5
        assert last["ret_var"] != clast["ret_var"] and last["cost_var"] != clast["cost_var"]
    # ---- the kernels
    env = VecNormalizeWithCost(VecCostWrapper(HipSynthVecEnv(N, "hc")), **kw)
    dev = lambda x, dt: torch.as_tensor(x, device="cuda").to(dt).contiguous()
    nm, raw0 = env.struct(), dev(ref["raw0"], torch.float64)      # (what VecNormalize.reset launches, on the case's reset batch)
    _lib.check(_lib.lib().icrl_vecnorm_reset(_lib.byref(nm), p(raw0), N, 18, p(env._obs_out), _lib.current_stream()), "icrl_vecnorm_reset")
    assert np.array_equal(env._obs_out.cpu().numpy(), ref["obs0"])
    for t, s in enumerate(ref["steps"]):
        env._norm_call(dev(s["obs"], torch.float64), dev(s["rew"], torch.float64), dev(s["cost"], torch.float32), dev(s["done"], torch.uint8))
        assert np.array_equal(env._obs_out.cpu().numpy(), s["obs_n"]), t
        assert np.array_equal(env._rew_out.cpu().numpy(), s["rew_n"]), t
        assert np.array_equal(env._cost_out.cpu().numpy(), s["cost_n"]), t
        assert np.array_equal(env.ret.cpu().numpy(), s["ret"]) and np.array_equal(env.cost_ret.cpu().numpy(), s["cost_ret"]), t
        assert env.ret_rms.var == s["ret_var"] and env.cost_rms.var == s["cost_var"], t
        assert np.array_equal(env.obs_rms.var, s["obs_var"]), t


# ---- b. fused rollouts against the port --------------------------------------------------------------------------------------------------------
_PLANES = ("observations", "orig_observations", "new_observations", "actions", "rewards", "costs", "orig_costs", "dones", "log_probs",
           "reward_values", "cost_values", "reward_advantages", "cost_advantages", "reward_returns", "cost_returns")
# kernel forced through agent.rollout_kernel: auto = rollout_persistent_kernel (<= 96 envs), wide = rollout_wide_kernel, multi =
# rollout_multi_kernel, steps = the per-step launches (act_step_kernel + norm_step[_small]_kernel); wide-policy = the generic-shape
# persistent kernel (rollout_generic_kernel).  Every kernel has an hc case (upper reward clip) and an ant / antbroken one (lower).
# ant 128x10 on multi: rollout_multi_kernel takes a shape only with >= 4 envs per group of statistics owners (115 statistics: >= 116
# envs); ant 32x20 with `multi` forced is served by the persistent kernel, so this is the Ant case that RUNS the multi-env kernel.
# The last field is what icrl_rollout_collect must have launched (helpers/routes.py), asserted behind the call.
_FUSED = [("auto", "hc", 7, 33, "tight", "persistent"), ("auto", "hc", 64, 40, "tight", "persistent"), ("auto", "ant", 32, 20, "tight", "persistent"),
          ("auto", "hc", 64, 40, "eps", "persistent"),
          ("wide", "hc", 130, 24, "tight", "wide"), ("wide", "antbroken", 512, 10, "tight", "wide"),
          ("multi", "hc", 37, 21, "tight", "multi"), ("multi", "hc", 300, 12, "tight", "multi"), ("multi", "ant", 32, 20, "tight", "persistent"),
          ("multi", "hc", 37, 21, "eps", "multi"), ("multi", "ant", 128, 10, "tight", "multi"),
          ("steps", "hc", 7, 33, "tight", "per-step"), ("steps", "ant", 32, 20, "tight", "per-step"),
          ("wide-policy", "hc", 16, 40, "tight", "generic-persistent"),
          ("auto", "hc", 64, 40, "tight_no_rew", "persistent"), ("multi", "hc", 64, 40, "tight_no_rew", "multi"),
          ("auto", "hc", 64, 40, "tight_no_obs", "persistent"), ("multi", "hc", 64, 40, "tight_no_obs", "multi")]


def _gpu_chain(kind, N, T, kw, o, kernel="auto", net_arch=None, seed=7):
    """the GPU twin of nc.oracle_buf's stack: same weights (loaded from the oracle's), same start, the named rollout kernel."""
    from icrl_amd.constraint_net import ConstraintNet
    from icrl_amd.ppo_lag import PPOLagrangian
    from icrl_amd.vec_env import HipSynthVecEnv, VecCostWrapper, VecNormalizeWithCost
    broken = kind == "antbroken"
    ekind = "ant" if broken else kind
    od, ad = (18, 6) if ekind == "hc" else (113, 8)
    hid = [20] if ekind == "hc" else [40, 40]
    lo = -np.ones(ad, np.float32)
    env = VecNormalizeWithCost(VecCostWrapper(HipSynthVecEnv(N, ekind, seed, broken=broken)), **kw)
    cn = ConstraintNet(od, ad, hid, None, lambda x: 0.05, None, None, False, 0.5, clip_obs=20, action_low=lo, action_high=-lo)
    cn.load_state_dict(o["cn_sd"])
    env.set_cost_function(cn.cost_function)
    akw = dict(policy_kwargs=dict(net_arch=net_arch)) if net_arch else {}
    agent = PPOLagrangian("TwoCriticsMlpPolicy", env, n_steps=T, seed=seed, **akw)
    agent.policy.load_state_dict(o["policy_sd"])
    if net_arch:
        assert agent.policy.wide and agent._fused_chain() is not None
    else:
        agent.rollout_kernel = kernel
    agent._setup_learn(N * T)
    env.unwrapped.t_ep.fill_(o["start"])
    return agent, env


def _fused_id(k, e, n, t, c, route):
    """a forced kernel that does not take its shape carries what runs instead in its id"""
    return f"{k}-{e}-{n}x{t}-{c}" + (f"-falls-to-{route}" if k in ("wide", "multi") and route != k else "")


@pytest.mark.parametrize("kernel,kind,N,T,case,route", _FUSED, ids=[_fused_id(*f) for f in _FUSED])
def test_fused_rollout_vs_port_under_settings(kernel, kind, N, T, case, route):
    """test_fused_rollout_vs_port's comparison (same planes, same statistics checks, same bound) with the normaliser at a named setting."""
    wide = kernel == "wide-policy"
    o = nc.oracle_rollout(kind, N, T, case, net_arch=nc.WIDE_ARCH if wide else None)
    b, norm = o["buf"], o["norm"]
    nc.check_rollout_inputs(case, kind, b, o["counter"], N, RTOL, ATOL)
    agent, env = _gpu_chain(kind, N, T, nc.CASES[case], o, kernel, nc.WIDE_ARCH if wide else None)
    agent.collect_rollouts(env, None, agent.rollout_buffer, T, "cost", noise=torch.as_tensor(o["noise"], device="cuda"))
    routes.check_rollout(route, f"{kernel} {kind} {N}x{T} {case}")
    agent.check_rollout_status()
    rb = agent.rollout_buffer
    worst = {}
    for k in _PLANES:
        got, ref = getattr(rb, k).cpu().numpy().reshape(T, N, -1), getattr(b, k).reshape(T, N, -1)
        worst[k] = nc.in_bounds(got, ref, RTOL, ATOL)
    top = max(worst, key=worst.get)
    print(f"[normalizer settings] {kernel} {kind} {N}x{T} {case}: worst plane {top} at {worst[top]:.3f} of the bound")
    for k in _PLANES:
        got, ref = getattr(rb, k).cpu().numpy().reshape(T, N, -1), getattr(b, k).reshape(T, N, -1)
        assert np.allclose(got, ref, rtol=RTOL, atol=ATOL), (k, np.abs(got - ref).max(), worst[k])
    # float64 running moments over N x T samples (the samples themselves carry the fp32 action differences)
    assert np.allclose(env.obs_rms.mean, norm.obs_rms.mean, rtol=1e-5, atol=1e-6)
    assert np.allclose(env.obs_rms.var, norm.obs_rms.var, rtol=1e-5, atol=1e-8)
    assert abs(env.ret_rms.var - norm.ret_rms.var) <= 1e-5 * max(1.0, norm.ret_rms.var)
    assert abs(env.cost_rms.var - norm.cost_rms.var) <= 1e-5 * max(1.0, norm.cost_rms.var)
    assert env.obs_rms.count == norm.obs_rms.count


# ---- c. kernel against kernel, bit for bit ----------------------------------------------------------------------------------------------------
# what each case launches: test_rollout_gpu.ONE_LAUNCH_ROUTES, asserted in the body.  hc 7 and ant 32 are fewer envs than `wide` (obs + 2
# workgroups: 20 / 115) and `multi` (4 envs per group of statistics owners: 20 / 116) take: forced, they run what `auto` runs there, the
# one-workgroup-per-env kernel, and their ids say so; hc 20, ant 115 and ant 116 are the smallest shapes the named kernels do run.
def _tight_cases():
    out = []
    for kernel in ("auto", "wide", "multi"):
        for kind, N, T in (("hc", 7, 33), ("hc", 130, 24), ("hc", 300, 12), ("ant", 32, 20)):
            falls = kernel != "auto" and (kind, N) in (("hc", 7), ("ant", 32))
            out.append(pytest.param(kind, N, T, kernel, id=f"{kind}-{N}-{T}-{kernel}" + ("-falls-to-persistent" if falls else "")))
    out += [pytest.param("hc", 20, 12, "wide", id="hc-20-12-wide"), pytest.param("hc", 20, 12, "multi", id="hc-20-12-multi"),
            pytest.param("ant", 115, 20, "wide", id="ant-115-20-wide"), pytest.param("ant", 116, 20, "multi", id="ant-116-20-multi")]
    return out


@pytest.mark.parametrize("kind,N,T,kernel", _tight_cases())
def test_one_launch_rollouts_equal_per_step_launches_under_tight(kind, N, T, kernel):
    """test_persistent_rollout_equals_per_step_launches with both chains under `tight` (a forced kernel that does not take a shape leaves
    it to the next one in line: wide needs >= obs + 2 workgroups, multi >= 4 envs per group of statistics owners)."""
    import test_rollout_gpu as tr
    o = nc.oracle_rollout(kind, N, T, "tight", seed=13, noise_seed=8, rollouts=2)      # the oracle's run of the body's first rollout
    nc.check_rollout_inputs("tight", kind, o["buf"], o["counter"], N, RTOL, ATOL)
    tr.test_persistent_rollout_equals_per_step_launches(kind, N, T, kernel=kernel, norm_kwargs=TIGHT)


def test_generic_shape_rollout_equals_python_loop_under_tight():
    import test_rollout_gpu as tr
    from helpers.arches import ARCHES
    o = nc.oracle_rollout("hc", 12, 40, "tight", net_arch=ARCHES["trunk"], seed=11, noise_seed=3, rollouts=2, cross_end=False)
    nc.check_rollout_inputs("tight", "hc", o["buf"], o["counter"], 12, RTOL, ATOL, cross_end=False)
    tr.test_generic_shape_rollout_equals_python_loop("hc", "trunk", 12, norm_kwargs=TIGHT)


# ---- d. host-env step -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,N,T", [("hc", 7, 24), ("ant", 16, 12)])
def test_host_rollout_equals_device_rollout_under_tight(kind, N, T):
    """host_step_kernel against the per-step launches (which section b ties to the oracle), both chains under `tight`: bit-identical."""
    import test_host_rollout_gpu as th
    o = nc.oracle_rollout(kind, N, T, "tight", seed=5, noise_seed=8, rollouts=2)
    nc.check_rollout_inputs("tight", kind, o["buf"], o["counter"], N, RTOL, ATOL)
    th.test_host_rollout_equals_device_rollout(kind, N, T, True, True, False, norm_kwargs=TIGHT)


# ---- e. samplers with frozen statistics ---------------------------------------------------------------------------------------------------------
_EVAL_KW = dict(clip_obs=1.5, epsilon=0.25)
_N_EP = 3


def _sampler_case(shape):
    """train env + agent that has taken one rollout (4 envs x 32 steps), the oracle's twin, and the oracle's episodes on an eval stack with
    clip_obs 1.5 / epsilon 0.25 after syncing the statistics; the policy's action bias seeks the wall of HCWithPosTest (short episodes)."""
    from helpers.arches import ARCHES, oracle_arch_kwargs
    from icrl_amd.ppo_lag import PPOLagrangian
    net_arch = ARCHES[shape] if shape else None
    o = nc.oracle_buf("hc", 4, 32, {}, net_arch=net_arch, seed=3, noise_seed=5, cross_end=False)
    agent, env = _gpu_chain("hc", 4, 32, {}, o, net_arch=net_arch, seed=3)
    agent.collect_rollouts(env, None, agent.rollout_buffer, 32, "cost", noise=torch.as_tensor(o["noise"], device="cuda"))
    agent.check_rollout_status()
    sd = agent.policy.state_dict()
    B0 = np.random.RandomState(1234).randn(18, 6)[0] * 0.05
    sd["action_net.bias"] = torch.as_tensor(-np.sign(B0) * 2.0, dtype=torch.float32)
    agent.policy.load_state_dict(sd)
    port = o_loop.PortAgent(o_loop.make_stack(4, "hc", 3), n_steps=32, seed=3, **(oracle_arch_kwargs(net_arch) if net_arch else {}))
    port.policy.load_state_dict(sd)
    noise = np.random.RandomState(0).randn(_N_EP * 1000, 6).astype(np.float32) * 0.1

    def oracle_eval_stack():
        est = o_loop.make_stack(1, "hc", 3, training=False, norm_reward=False, norm_cost=False, wall_terminate=True, **_EVAL_KW)
        o_loop.sync_normalization(o["norm"], est.norm)
        port.stack = est
        return est
    want = o_loop.sample_from_agent(port, oracle_eval_stack(), _N_EP, noise)
    want_eval = o_loop.evaluate_policy(port, oracle_eval_stack(), _N_EP, noise)
    return agent, env, noise, want, want_eval, o["norm"]


def _eval_env(train_env, env_id="HCWithPosTest-v0"):
    from icrl_amd import utils
    from icrl_amd.vec_env import VecNormalizeWithCost, sync_envs_normalization
    eenv = VecNormalizeWithCost(utils.make_vec_env(env_id, 1, 3, dummy_vec_env=True), training=False, norm_reward=False, norm_cost=False, **_EVAL_KW)
    sync_envs_normalization(train_env, eenv)
    return eenv


def _assert_sample(got, want, what):
    oo, o, a, r, l = got
    assert list(l) == list(want[4]), (what, l, want[4])
    assert np.allclose(oo.cpu().numpy(), want[0], rtol=1e-4, atol=2e-5), what      # the tolerances of test_sample_from_agent_reference_golden
    assert np.allclose(o.cpu().numpy(), want[1], rtol=1e-4, atol=2e-4), what
    assert np.allclose(a.cpu().numpy(), want[2], rtol=1e-4, atol=2e-5), what
    assert np.allclose(r, want[3], rtol=1e-5, atol=1e-3), what


@pytest.mark.parametrize("shape", [None, "trunk"], ids=["64-wide", "trunk"])
def test_samplers_with_frozen_statistics_clip_and_epsilon(shape):
    """sample_from_agent / evaluate_policy on an eval env with clip_obs 1.5 and epsilon 0.25 against the oracle's loops: the chained launch
    (sample_episodes_chain_kernel), the pass-by-pass launch (sample_episodes_kernel; for `trunk` sample_episodes_generic_kernel) and, for
    the 64-wide policy, a host eval env (host_episode_kernel)."""
    import tests.helpers.host_envs  # noqa: F401  (registers the Host* ids)
    from icrl_amd import utils
    agent, env, noise, want, want_eval, norm = _sampler_case(shape)
    # ---- conditions, from the oracle: short episodes, observations at both clips, and clip / epsilon both visible
    obs_n = want[1]
    assert max(want[4]) < 1000 and obs_n.shape[0] == sum(want[4])
    share = nc.share_at(obs_n, 1.5) + nc.share_at(obs_n, -1.5)
    assert nc.SHARE[0] <= share <= nc.SHARE[1] and nc.share_at(obs_n, 1.5) > 0 and nc.share_at(obs_n, -1.5) > 0, share
    dflt = o_stats.NormState(1, 18, training=False)          # the same rows under the default clip and epsilon
    dflt.obs_rms = norm.obs_rms
    obs_d = o_stats.normalize_obs(dflt, want[0])
    inner = np.abs(obs_n) < 1.5                              # (where the clip is not reached, epsilon alone moves the observation)
    assert np.abs(obs_n).max() == 1.5 and np.abs(obs_d).max() > 1.5 and nc.in_bounds(obs_d[inner], obs_n[inner], 1e-4, 2e-4) >= nc.MIN_SHIFT
    # ---- the kernels
    eenv = _eval_env(env)
    assert np.allclose(eenv.obs_rms.mean, norm.obs_rms.mean, rtol=1e-5, atol=1e-6) and np.allclose(eenv.obs_rms.var, norm.obs_rms.var, rtol=1e-5, atol=1e-8)
    got = utils.sample_from_agent(agent, eenv, _N_EP, noise=noise)                    # chained launch where it serves
    _assert_sample(got, want, "sample_from_agent")
    run = utils._run_episodes(agent, _eval_env(env), _N_EP, False, noise, parallel=True)      # pass by pass: sample_episodes[_generic]_kernel
    assert isinstance(run, utils.EpisodeRun)
    _assert_sample(utils.sample_result(run), want, "pass by pass")
    mean_r, std_r = utils.evaluate_policy(agent, _eval_env(env), _N_EP, deterministic=False, noise=noise)
    assert abs(mean_r - want_eval[0]) < 1e-3 * max(1, abs(want_eval[0])) and abs(std_r - want_eval[1]) < 1e-3 * max(1, abs(want_eval[1]))
    if shape is None:
        henv = _eval_env(env, "HostHCWithPosTest-v0")
        hrun = utils._run_episodes(agent, henv, _N_EP, False, noise, False)
        assert isinstance(hrun, utils.HostEpisodeRun)
        _assert_sample(utils.sample_result(hrun), want, "host eval env")
        henv.close()


# ---- f. one batched launch, a different normaliser block per run ---------------------------------------------------------------------------
_BATCH_KW = (TIGHT, {}, dict(epsilon=0.25, reward_gamma=0.95))


# 3 runs x 8 envs fit the chip one workgroup per env: rollout_persistent_batch_kernel; 3 x 96 envs do not: rollout_multi_batch_kernel
@pytest.mark.parametrize("N,T", [(8, 32), (96, 16)])
def test_batched_launch_reads_each_runs_own_normaliser(N, T):
    """three hc runs with the same weights, seeds and noise but different normaliser settings through ONE icrl_rollout_collect_batch call:
    each run's buffer and statistics equal, bit for bit, the same run launched alone (rollout_kernel = "multi")."""
    import test_cpg_seed_batch_gpu as tb
    import test_rollout_gpu as tr
    from icrl_amd import _lib
    from icrl_amd.structs import RolloutJobT, addr, p
    # ---- conditions, from the oracle: the tight run reaches its clips, and the three settings give three different reward planes
    o = nc.oracle_rollout("hc", N, T, "tight", noise_seed=8)
    nc.check_rollout_inputs("tight", "hc", o["buf"], o["counter"], N, RTOL, ATOL)
    bufs = [nc.oracle_buf("hc", N, T, kw, noise_seed=8)["buf"] for kw in _BATCH_KW]
    for i in range(3):
        for j in range(i):
            assert nc.in_bounds(bufs[i].rewards, bufs[j].rewards, RTOL, ATOL) >= nc.MIN_SHIFT, (i, j)
    # ---- the launches
    pairs = [tr._pair_of_agents(N, T, 7, norm_kwargs=kw) for kw in _BATCH_KW]
    noise = torch.as_tensor(o["noise"], device="cuda")
    for (a_s, e_s, _), (a_b, e_b, _) in pairs:
        a_s.rollout_kernel = "multi"
        for a, e in ((a_s, e_s), (a_b, e_b)):
            a._setup_learn(N * T)
            e.unwrapped.t_ep.fill_(o["start"])
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
    planes = [a.rollout_buffer.rewards.cpu().numpy() for a in agents]
    assert all(not np.array_equal(planes[i], planes[j]) for i in range(3) for j in range(i))


# ---- g. GAIL's un-normalise step ---------------------------------------------------------------------------------------------------------------------
def test_gail_unnormalize_reads_epsilon():
    """icrl_gail_unnormalize_batch with epsilon = 0.25: raw_obs equals obs.double() * sqrt(var + eps) + mean (float64) bit for bit."""
    import test_gail_seed_batch_gpu as tg
    runs = tg._gail_runs(18, 6, False, True, ("wall", "both", "torque"), (30,), 0, eps=0.25)
    for r in runs:      # the condition: with the default epsilon every row would come out elsewhere, by far more than a rounding
        dflt = r["obs"].double() * torch.sqrt(r["var"] + 1e-8) + r["mean"]
        assert r["eps"] == 0.25 and ((dflt - r["ref_raw"]).abs().amax(dim=1) > 1e-3).all()
    tg._run_gail_kernels(runs, 0, 18, 6)
    for i, r in enumerate(runs):
        assert torch.equal(r["raw"], r["ref_raw"]), (i, (r["raw"] - r["ref_raw"]).abs().max().item())
