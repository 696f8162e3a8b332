"""GPU: the launch ladders at their edges.  Every fused entry point chooses among several launch forms by shape, workspace and device and
steps to the next one silently (the rollout's order: the comment above icrl_rollout_collect_ex_mon in csrc/rollout_collect.hip; the update's:
prepare_train in csrc/ppo_train.hip; the GAE's: icrl_gae_dual_ws in csrc/gae.hip).  Each case here sits on one side of a threshold, asserts
what the call launched (icrl_debug_last_route through helpers/routes.py) and compares what it left, bit for bit, with the form on the
other side: a ladder that moved would fail the route, a kernel that is wrong at the edge of its range the comparison.  Expectations that
depend on the device are computed from its compute-unit count, never from a constant."""
import numpy as np
import pytest
import torch

from helpers import routes

pytestmark = pytest.mark.gpu

_KEYS = ("observations", "orig_observations", "new_observations", "new_orig_observations", "actions", "rewards", "costs", "orig_costs", "dones",
         "log_probs", "reward_values", "cost_values", "reward_advantages", "cost_advantages", "reward_returns", "cost_returns")


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _assert_twins(a_p, e_p, a_s, e_s, tag, keys=_KEYS):
    """every buffer plane, the normaliser state and the carry-over arrays (test_persistent_rollout_equals_per_step_launches' list)."""
    for k in keys:
        got, ref = getattr(a_p.rollout_buffer, k).cpu().numpy(), getattr(a_s.rollout_buffer, k).cpu().numpy()
        assert np.array_equal(got, ref), (tag, k, np.abs(got.astype(np.float64) - ref.astype(np.float64)).max())
    for name in ("obs_rms", "ret_rms", "cost_rms"):
        rp, rs = getattr(e_p, name), getattr(e_s, name)
        assert np.array_equal(np.asarray(rp.mean), np.asarray(rs.mean)) and np.array_equal(np.asarray(rp.var), np.asarray(rs.var)), (tag, name)
        assert rp.count == rs.count, (tag, name)
    assert torch.equal(e_p.ret, e_s.ret) and torch.equal(e_p.cost_ret, e_s.cost_ret), tag
    assert torch.equal(a_p._last_obs, a_s._last_obs) and torch.equal(a_p._ag["last_dones"], a_s._ag["last_dones"]), tag
    assert torch.equal(e_p.unwrapped.s, e_s.unwrapped.s) and torch.equal(e_p.unwrapped.t_ep, e_s.unwrapped.t_ep), tag
    for k in ("raw_rew", "raw_cost", "dones", "last_v_r", "last_v_c", "act_clipped"):
        assert torch.equal(a_p._ag[k], a_s._ag[k]), (tag, k)


# ---- the pairs of identical chains ----------------------------------------------------------------------------------------------------
def _synth_pair(kind, N, T, frozen=False):
    import test_rollout_gpu as tr
    (a_p, e_p, _), (a_s, e_s, _) = tr._pair_of_agents(N, T, 13, kind, norm_kwargs=dict(training=False) if frozen else None)
    ad = 6 if kind == "hc" else 8
    return (a_p, e_p), (a_s, e_s), (T, N, ad), {"hc": 1000, "ant": 500}[kind]


def _lgw_pair(N, T):
    import test_lap_grid_gpu as tl
    a_p, e_p, c_p = tl._lgw_agent(N, T, 3)
    a_s, e_s, c_s = tl._lgw_agent(N, T, 3)
    c_s.load_state_dict(c_p.state_dict())
    a_s.policy.load_state_dict(a_p.policy.state_dict())
    return (a_p, e_p), (a_s, e_s), (T, N), None


def _point_pair(N, T):
    from icrl_amd.ppo_lag import PPOLagrangian
    from icrl_amd.true_constraint_net import AnalyticCost
    from icrl_amd.vec_env import HipSynthVecEnv, VecCostWrapper, VecNormalizeWithCost
    out = []
    for _ in range(2):
        torch.manual_seed(13)
        env = VecNormalizeWithCost(VecCostWrapper(HipSynthVecEnv(N, "point_circle", 13)))
        env.set_cost_function(AnalyticCost.wall_behind(-3))
        agent = PPOLagrangian("TwoCriticsMlpPolicy", env, n_steps=T, seed=13)
        sd = agent.policy.state_dict()
        sd["log_std"] = torch.full((2,), 0.5)      # (tests/test_point_env_gpu.py: the clip active on most draws)
        agent.policy.load_state_dict(sd)
        out.append((agent, env))
    out[1][0].policy.load_state_dict(out[0][0].policy.state_dict())
    return out[0], out[1], (T, N, 2), 150


def _one_launch_against_steps(pair, kernel, expect, tag):
    """the body of test_persistent_rollout_equals_per_step_launches with the route of both sides asserted behind each call."""
    (a_p, e_p), (a_s, e_s), noise_shape, limit = pair
    T, N = noise_shape[:2]
    a_p.rollout_kernel, a_s.rollout_kernel = kernel, "steps"
    rng = np.random.RandomState(8)
    draw = (lambda: rng.rand(*noise_shape)) if len(noise_shape) == 2 else (lambda: rng.randn(*noise_shape))      # Discrete: uniforms
    noise = torch.as_tensor(np.stack([draw(), draw()]).astype(np.float32), device="cuda")
    a_p._setup_learn(2 * N * T); a_s._setup_learn(2 * N * T)
    if limit is not None:
        for env in (e_p, e_s):
            env.unwrapped.t_ep.fill_(limit - T // 2)           # every env crosses its time limit inside the first rollout
    got = None
    for it in range(2):
        a_p.collect_rollouts(e_p, None, a_p.rollout_buffer, T, "cost", noise=noise[it])
        got = routes.check_rollout(dict(expect, n_runs=1), f"{tag} {kernel}")
        a_s.collect_rollouts(e_s, None, a_s.rollout_buffer, T, "cost", noise=noise[it])
        routes.check_rollout(dict(route="per-step", launches=2 * T, envs_per_wg=0, wgs=N, ws=0), f"{tag} steps")
        a_p.check_rollout_status()
        _assert_twins(a_p, e_p, a_s, e_s, (tag, it))
        if limit is not None:
            assert a_p.rollout_buffer.dones.sum().item() == (N if it == 0 else a_s.rollout_buffer.dones.sum().item())
    return got


# ---- 1. single runs -------------------------------------------------------------------------------------------------------------------
_ONE = dict(launches=1)
# id: (pair factory, its arguments, rollout_kernel, the words the call must leave).  hc: 18 observations (20 statistics with a constraint
# net: the multi kernel takes >= 4 envs per group of 5 statistics owners = 20 envs, the wide kernel obs + 2 = 20 workgroups); ant: 113
# (115 statistics: 116 envs / 115 workgroups; 36 x 113 <= 4096 < 37 x 113 observation doubles for the one-workgroup-per-env kernel)
_SINGLE = {
    "hc-96-auto": (_synth_pair, ("hc", 96, 8), "auto", dict(_ONE, route="persistent", wgs=96, envs_per_wg=1, ws=1)),
    "hc-97-auto": (_synth_pair, ("hc", 97, 8), "auto", dict(_ONE, route="wide", ws=1)),
    "hc-1024-auto": (_synth_pair, ("hc", 1024, 3), "auto", dict(_ONE, route="wide", ws=1)),
    "hc-1025-auto": (_synth_pair, ("hc", 1025, 3), "auto", dict(_ONE, route="multi", envs_per_wg=8, wgs=129, ws=1)),
    "hc-19-multi-falls-to-persistent": (_synth_pair, ("hc", 19, 12), "multi", dict(_ONE, route="persistent", wgs=19, ws=1)),
    "hc-20-multi": (_synth_pair, ("hc", 20, 12), "multi", dict(_ONE, route="multi", envs_per_wg=4, wgs=5, packed=1, ws=1)),
    "ant-36-auto": (_synth_pair, ("ant", 36, 8), "auto", dict(_ONE, route="persistent", wgs=36, ws=1)),
    "ant-37-auto": (_synth_pair, ("ant", 37, 8), "auto", dict(route="per-step", launches=16)),
    "ant-114-auto": (_synth_pair, ("ant", 114, 6), "auto", dict(route="per-step", launches=12)),
    "ant-115-auto": (_synth_pair, ("ant", 115, 6), "auto", dict(_ONE, route="wide", wgs=115, envs_per_wg=1, ws=1)),
    "hc-128-frozen": (_synth_pair, ("hc", 128, 8, True), "auto", dict(_ONE, route="persistent", wgs=128, envs_per_wg=1, ws=1)),
    "hc-129-frozen": (_synth_pair, ("hc", 129, 8, True), "auto", dict(route="per-step", launches=16)),
    "lgw-8-discrete": (_lgw_pair, (8, 12), "auto", dict(_ONE, route="persistent", wgs=8, ws=1)),
    "point-11-auto": (_point_pair, (11, 12), "auto", dict(route="per-step", launches=24)),
    "point-12-auto": (_point_pair, (12, 12), "auto", dict(_ONE, route="multi", envs_per_wg=4, wgs=3, ws=1)),
    "point-96-auto": (_point_pair, (96, 8), "auto", dict(_ONE, route="multi", envs_per_wg=8, wgs=12, ws=1)),
    "point-97-auto": (_point_pair, (97, 8), "auto", dict(_ONE, route="wide", ws=1)),
    "hc-8-steps": (_synth_pair, ("hc", 8, 12), "steps", dict(route="per-step", launches=24, envs_per_wg=0)),
}


@pytest.mark.parametrize("case", list(_SINGLE))
def test_single_run_ladder_at_its_edges(case):
    make, args, kernel, expect = _SINGLE[case]
    pair = make(*args)
    N = pair[2][1]
    obs = pair[0][1].observation_space.shape[0]
    got = _one_launch_against_steps(pair, kernel, expect, case)
    if expect["route"] == "wide":
        # one workgroup per compute-unit slot: E = ceil(N / (slots x CUs)) envs per workgroup, a balanced grid of at least obs + 2
        E, G = got["envs_per_wg"], got["wgs"]
        assert 1 <= E <= 4 and G >= obs + 2 and G * E >= N and (G - 1) * E < N, (E, G, N)
    if expect["route"] == "persistent":
        small = obs <= 32
        assert bool(got["pick"] & routes.PICK_SMALL) == small and bool(got["pick"] & routes.PICK_GRAN) == (N * (2 * obs + 4) <= 256 * 12)


# ---- 2. where the exchange workspace comes from -------------------------------------------------------------------------------------
def _persist_ws_bytes(N, O):
    """the one-workgroup-per-env kernel's workspace (include/icrl_hip.h, icrl_agent_t.xch_ws; csrc/rollout_collect.hip persist_ws_carve):
    xch_obs f64 [2][N][O] | xch_rew f64 [2][N] | xch_cost f32 [2][N] | xch_done u32 [2][N] | counters, to 1024 B with the padding |
    granule records u64 [2][N][2 O + 4] when N (2 O + 4) <= 256 x 12"""
    gran = N * (2 * O + 4) <= 256 * 12
    return 16 * N * O + 16 * N + 8 * N + 8 * N + 1024 + (16 * N * (2 * O + 4) if gran else 0)


@pytest.mark.parametrize("side", ["plane-large-enough", "plane-one-row-short"])
def test_exchange_workspace_from_the_advantage_plane(side):
    """8 hc envs whose agent has no exchange workspace (icrl_agent_t.xch_ws of one word).  The header promises the not yet computed
    reward_advantages plane in its place once T x N x 4 bytes hold the layout: at the first such T the persistent kernel runs on the plane
    (source 2) and leaves, reward_advantages included, what the run on xch_ws leaves; one row fewer and the rollout is per-step launches."""
    N, O = 8, 18
    need = _persist_ws_bytes(N, O)
    T = -(-need // (4 * N)) - (side == "plane-one-row-short")
    assert (T * N * 4 >= need) == (side == "plane-large-enough") and (T + 1) * N * 4 >= need > (T - 1) * N * 4
    (a_p, e_p), (a_s, e_s), shape, _ = _synth_pair("hc", N, T)
    a_p._ag["xch_ws"] = torch.zeros(1, dtype=torch.int64, device="cuda")
    noise = torch.as_tensor(np.random.RandomState(8).randn(*shape).astype(np.float32), device="cuda")
    a_p._setup_learn(N * T); a_s._setup_learn(N * T)
    a_p.collect_rollouts(e_p, None, a_p.rollout_buffer, T, "cost", noise=noise)
    if side == "plane-large-enough":
        routes.check_rollout(dict(route="persistent", ws=2, wgs=N, launches=1), "plane")
    else:
        routes.check_rollout(dict(route="per-step", ws=0, launches=2 * T), "plane one row short")
    a_s.collect_rollouts(e_s, None, a_s.rollout_buffer, T, "cost", noise=noise)
    routes.check_rollout(dict(route="persistent", ws=1, wgs=N, launches=1), "xch_ws")
    a_p.check_rollout_status(); a_s.check_rollout_status()
    _assert_twins(a_p, e_p, a_s, e_s, side)


# ---- 3. batched rollouts --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["few", "multi-packed", "frozen-above-the-cus", "multi-run-major"])
def test_batched_rollout_ladder(case):
    """icrl_rollout_collect_batch: a `few` batch (n_runs x N <= compute units) on the one-workgroup-per-env kernel with the whole register file
    (MINW 1); 5 x 64 hc on the multi-env kernel, 8 envs per workgroup, every run's 8 workgroups on one XCD; a frozen normaliser (no multi-env
    form) in more workgroups than compute units: the one-workgroup-per-env kernel, two workgroups per compute unit (MINW 2); runs of 33
    workgroups, more than the packed layout takes: run-major.  Every run bit for bit what it leaves alone."""
    import test_rollout_gpu as tr
    from icrl_amd import _lib
    from icrl_amd.structs import RolloutJobT, addr, p
    cus = _cus()
    if case == "few":
        N, T, S, frozen = 8, 8, 3, False
        assert S * N <= cus
        expect = dict(route="persistent-batch", minw=1, wgs=N, envs_per_wg=1)
    elif case == "multi-packed":
        N, T, S, frozen = 64, 6, max(5, cus // 64 + 1), False
        assert S * N > cus
        expect = dict(route="multi-batch", envs_per_wg=8, wgs=8, packed=1)
    elif case == "frozen-above-the-cus":
        N, T, S, frozen = 96, 6, cus // 96 + 1, True
        assert S * N > cus
        expect = dict(route="persistent-batch", minw=2, wgs=N, envs_per_wg=1)
    else:
        N, T, S, frozen = 264, 4, 2, False      # 8 envs per workgroup: 33 workgroups per run > 32
        expect = dict(route="multi-batch", envs_per_wg=8, wgs=33, packed=0)
    nk = dict(training=False) if frozen else None
    pairs = [tr._pair_of_agents(N, T, 20 + r, norm_kwargs=nk) for r in range(S)]
    noise = torch.as_tensor(np.random.RandomState(8).randn(S, T, N, 6).astype(np.float32), device="cuda")
    for r, ((a_s, e_s, _), (a_b, e_b, _)) in enumerate(pairs):
        a_s.rollout_kernel = "auto" if frozen or N < 20 else "multi"      # (fewer than 20 hc envs: the multi-env kernel declines)
        for a, e in ((a_s, e_s), (a_b, e_b)):
            a._setup_learn(N * T)
            e.unwrapped.t_ep.fill_(1000 - T // 2)
        a_s.collect_rollouts(e_s, None, a_s.rollout_buffer, T, "cost", noise=noise[r])
        routes.check_rollout(dict(route="persistent" if frozen or N < 20 else "multi", n_runs=1), f"{case} solo {r}")
        a_s.check_rollout_status()
    agents = [pair[1][0] for pair in pairs]
    jobs = [a._rollout_begin(None, a.rollout_buffer, T, noise[r]) for r, a in enumerate(agents)]
    arr = (RolloutJobT * S)(*[RolloutJobT(addr(j["env"]), addr(j["nm"]), addr(j["pol"]), addr(j["cn"]), addr(j["buf"]), addr(j["ag"]), p(j["noise"]))
                              for j in jobs])
    a0 = agents[0]
    ws = torch.empty(2 * S * _lib.BATCH_ARGS_BYTES, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().icrl_rollout_collect_batch(S, arr, p(a0._alow), p(a0._ahigh), float(a0.reward_gamma), float(a0.reward_gae_lambda),
                                                     float(a0.cost_gamma), float(a0.cost_gae_lambda), 1, p(ws), ws.numel(), _lib.current_stream()),
               "icrl_rollout_collect_batch")
    routes.check_rollout(dict(expect, n_runs=S, launches=1, ws=1), case)
    for a, j in zip(agents, jobs):
        a._rollout_end(j, a.env, None, a.rollout_buffer, T)
    torch.cuda.synchronize()
    for r, ((a_s, e_s, _), (a_b, e_b, _)) in enumerate(pairs):
        a_b.check_rollout_status()
        _assert_twins(a_b, e_b, a_s, e_s, (case, r))


# ---- 4. the update --------------------------------------------------------------------------------------------------------------------
_UN, _UT, _UB, _UE = 4, 8, 16, 2      # hc 4 envs x 8 steps, minibatches of 16, 2 epochs: 4 optimiser steps


def _update_agent(train_kernel=None):
    import test_ppo_train_gpu as tp
    a = tp._agent("hc", _UN, _UT, batch_size=_UB, n_epochs=_UE, target_kl=None, learning_rate=3e-4, clip_range=0.2)
    if train_kernel is not None:
        a.train_kernel = train_kernel
    return a


def _update_case():
    """one oracle case for every run: the buffer and three permutation sets (a run's index mod 3 picks its own)."""
    import test_ppo_train_gpu as tp
    from oracle import nets as o_nets
    rng = np.random.RandomState(_UN * _UT)
    a = _update_agent()
    sd0 = a.policy.state_dict()
    obs = rng.randn(_UT, _UN, 18).astype(np.float32)
    op = o_nets.TwoCriticPolicy(18, 6); op.load_state_dict(sd0)
    with torch.no_grad():
        act, vr, vc, lp = op.forward(torch.as_tensor(obs.reshape(-1, 18)))
    sh = (_UT, _UN)
    buf = dict(observations=obs, actions=act.numpy().reshape(_UT, _UN, 6), log_probs=lp.numpy().reshape(sh), reward_values=vr.numpy().reshape(sh),
               cost_values=vc.numpy().reshape(sh), reward_advantages=rng.randn(*sh).astype(np.float32) * 2, cost_advantages=rng.rand(*sh).astype(np.float32),
               reward_returns=rng.randn(*sh).astype(np.float32), cost_returns=rng.rand(*sh).astype(np.float32), orig_costs=rng.rand(*sh).astype(np.float32))
    perms = [np.stack([rng.permutation(_UT * _UN) for _ in range(_UE)]) for _ in range(3)]
    oracle = []
    for pm in perms:
        pol, out = tp._oracle_train(sd0, buf, pm, "hc", a.dual.nu().item(), lr=3e-4, batch_size=_UB, n_epochs=_UE, clip_range=0.2, target_kl=None)
        oracle.append({k: p_.detach().numpy() for k, p_ in pol.params.items()})
    return buf, perms, oracle


def _update_snapshot(a):
    pol = a.policy
    return [t.cpu().numpy().copy() for t in (pol.params, pol.exp_avg, pol.exp_avg_sq, a._train_ws["stats"][:11])]


@pytest.fixture(scope="module")
def update_case():
    import test_ppo_train_gpu as tp
    buf, perms, oracle = _update_case()
    solo = {}
    for family, kind in ((None, 5), ("halves", 4), ("pairs", 0)):
        for i, pm in enumerate(perms):
            a = _update_agent(family)
            tp._fill(a, buf)
            a.train(perms=pm)
            routes.check_update(dict(kind=kind, n_runs=1, wgs_per_network={5: 4, 4: 2, 0: 1}[kind]), f"solo {family or 'default'}")
            assert float(a._train_ws["stats"][11]) == 0
            solo[family, i] = _update_snapshot(a)
    return buf, perms, oracle, solo


@pytest.mark.parametrize("S,kind,family", [(16, 5, None), (17, 4, "halves"), (40, 4, "halves"), (41, 0, "pairs")])
def test_batched_update_ladder(update_case, S, kind, family):
    """icrl_ppo_lag_train_batch gives up to 16 runs the wave-quad kernel with four workgroups per network (what a run alone gets), 17..40
    its two-workgroup form and more the wave-pair kernel.  Every run of the batch equals, bit for bit, the run alone on THAT kernel
    (train_kernel = halves / pairs); against the default single run it is within the oracle bound of the update kernels (the forms sum
    their partial gradients in different orders), and it is printed whether it is bit-equal to it."""
    import test_ppo_train_gpu as tp
    from icrl_amd import _lib
    from icrl_amd.seed_batch import launch_trains
    buf, perms, oracle, solo = update_case
    agents, jobs = [], []
    for r in range(S):
        a = _update_agent()
        tp._fill(a, buf)
        agents.append(a)
        jobs.append(a._train_begin(perms[r % 3]))
    args_ws = torch.empty(S * _lib.BATCH_ARGS_BYTES, dtype=torch.uint8, device=agents[0].device)
    launch_trains(agents, jobs, args_ws)
    routes.check_update(dict(kind=kind, n_runs=S, wgs_per_network={5: 4, 4: 2, 0: 1}[kind]), f"{S} runs")
    torch.cuda.synchronize()
    same_as_default = True
    lr, n_steps = 3e-4, _UE * (_UN * _UT // _UB)
    for r, (a, j) in enumerate(zip(agents, jobs)):
        got = _update_snapshot(a)
        assert float(a._train_ws["stats"][11]) == 0
        for name, g_, s_ in zip(("params", "exp_avg", "exp_avg_sq", "stats"), got, solo[family, r % 3]):
            assert np.array_equal(g_, s_), (r, name, np.abs(g_ - s_).max())
        same_as_default = same_as_default and all(np.array_equal(g_, s_) for g_, s_ in zip(got, solo[None, r % 3]))
        a._train_end(j)
        worst = max(float(np.abs(v.numpy() - oracle[r % 3][k]).max()) for k, v in a.policy.state_dict().items())
        worst_d = float(np.abs(got[0] - solo[None, r % 3][0]).max())
        assert worst <= tp.ADAM_DEV_BOUND * lr * n_steps + 2e-7, (r, worst)
        assert worst_d <= tp.ADAM_DEV_BOUND * lr * n_steps + 2e-7, (r, worst_d)      # (the same bound, with the default single run as the reference)
    print(f"[route] {S} runs, kind {kind}: bit-equal to the default single run: {same_as_default}")
    if kind == 5:
        assert same_as_default


# id: (the kind a single run must get, test_train_vs_oracle's (kind, N, T, B, E, train_kernel); None: the Categorical case at obs 40)
_SINGLE_KINDS = {
    "obs40-pairs": (0, None), "ant-B64-quarters": (6, ("ant", 6, 32, 64, 2, None)), "ant-B128-quarters2": (7, ("ant", 24, 16, 128, 2, None)),
    "ant-B256-quarters": (6, ("ant", 4, 80, 256, 2, None)), "ant-rows-B128-split": (2, ("ant", 24, 16, 128, 2, "rows")),
    "ant-rows1": (1, ("ant", 24, 16, 128, 2, "rows1")), "hc-tiles": (3, ("hc", 4, 8, 16, 2, "tiles")), "hc-wide-generic": (8, ("hc-wide", 8, 32, 64, 3, None)),
}


@pytest.mark.parametrize("case", list(_SINGLE_KINDS))
def test_single_run_update_kinds(case):
    """what prepare_train gives one run: wave pairs at obs 33..64, four workgroups per network at obs 65..128 (chunk by chunk; both chunks in
    one pass at 65..128 rows), the row-owning kernel in both forms, the column-split tiles, the generic-shape path — each through the oracle
    comparison of test_train_vs_oracle."""
    import test_ppo_train_gpu as tp
    kind, args = _SINGLE_KINDS[case]
    if args is None:      # obs 40 (test_lap_grid_gpu's Categorical case at that width: wave pairs, the quad kernel stops at 32)
        import test_lap_grid_gpu as tl
        tl._categorical_case(40, 16, 8, 16, 128, 2, 0.05, False)
        routes.check_update(dict(kind=0, wgs_per_network=1, n_runs=1), case)
        return
    k, N, T, B, E, tk = args
    tp.test_train_vs_oracle(k, N, T, B, E, None, train_kernel=tk)
    routes.check_update(dict(kind=kind, n_runs=1), case)


def test_generic_update_as_launches_per_step():
    """ICRL_GEN_LAUNCHES (read once per process: a child) sends the generic-shape update to its three launches per optimiser step: kind 9."""
    import os, subprocess, sys
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import test_ppo_train_gpu as tp\nfrom helpers import routes\n"
            "tp.test_train_vs_oracle('hc-wide', 8, 32, 64, 3, None)\n"
            "routes.check_update(dict(kind=9, n_runs=1, packed=0), 'launches')\nprint('CHILD OK')\n") % (
                os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, ICRL_GEN_LAUNCHES="1"), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "CHILD OK" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])


# ---- 5. the dual GAE, waves_per_tile = 0 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["no-workspace", "register-resident", "two-pass", "workspace-too-small", "batch-one-run-without"])
def test_gae_automatic_choice(case):
    """icrl_gae_dual_ws with waves_per_tile = 0 over two column tiles (70 envs), each against the oracle at the bound of its form: no
    workspace and T = 8 -> one wave per tile (shape 101); a workspace of icrl_gae_dual_ws_bytes at T = 300 -> the register-resident split,
    three chunks; T = 2304 -> the two-pass split; 8 KB of workspace at T = 300 hold neither split (2 x 3 and 2 x 4 maps of 2052 B): 16 waves
    per tile; a batch whose second run has no workspace -> single launches."""
    import test_gae_gpu as tg
    from helpers import gae_cases as G
    from icrl_amd import _lib, structs as S
    N = 70
    if case == "batch-one-run-without":
        T, n_runs = 300, 3
        runs = [tg._BatchRun(T, N, 2000 + r, with_ws=r != 1) for r in range(n_runs)]
        garr = (S.GaeJobT * n_runs)(*[r.job() for r in runs])
        args_ws = torch.zeros(n_runs * _lib.BATCH_ARGS_BYTES, dtype=torch.uint8, device="cuda:0")
        _lib.check(_lib.lib().icrl_gae_dual_batch(n_runs, garr, T, N, *[float(p) for p in tg._SWAP_PARAMS], _lib.ptr(args_ws), args_ws.numel(),
                                                  _lib.current_stream()), "icrl_gae_dual_batch")
        routes.check_gae(dict(route="batch-singles", tiles=2, n_runs=n_runs), case)
        torch.cuda.synchronize()
        for r in runs:
            tg._check_guard(r.outs, T)
            for got, key in zip(r.outs, G.OUT_KEYS):
                tg._dev_bounds(got[:T], r.o[key], key)
        return
    T = {"no-workspace": 8, "two-pass": 2304}.get(case, 300)
    arrs, o = tg._swap_case(T, N, 77)
    ws = {"no-workspace": None, "workspace-too-small": torch.zeros(1024, dtype=torch.int64, device="cuda:0")}.get(case, tg._ws(T, N))
    (outs,) = tg._run_guarded(arrs, tg._SWAP_PARAMS, 0, ws)
    expect = {"no-workspace": dict(route="sequential", code=101), "register-resident": dict(route="regsplit", code=3),
              "two-pass": dict(route="split", code=16), "workspace-too-small": dict(route="sequential", code=16)}[case]
    routes.check_gae(dict(expect, tiles=2, n_runs=1), case)
    for got, key in zip(outs, G.OUT_KEYS):
        tg._assert_split_bounds(got, o[key], key)
    if ws is not None:
        assert tg._status(ws) == 0
