"""GPU: the cost-shaping callback's classifier step (icrl_cls_mlp_step) and second pass (icrl_cost_shaping_apply), the callback on a filled
buffer and inside `gail -ucsc [-ucn]`, against the reference's own callback as recorded in tests/golden/g27_cost_shaping.npz and against the
float64 torch restatement of tests/helpers/cost_shaping_cases.

Tolerance rule for every quantity compared with a reference: 4 x max |ref32 - ref64| of that quantity + 1e-12, compared against ref32 (both
implementations sit about one float32 rounding from the exact value: a factor 2; another 2 for a different summation order); the fixture's
cap conditions keep the rule from hiding a failure.  helpers.exploration_cases.check prints the measured distance next to the bound."""
import json
import types

import numpy as np
import pytest
import torch

from helpers import cost_shaping_cases as S
from helpers import routes

pytestmark = pytest.mark.gpu
SENTINEL = 7.25


@pytest.fixture(scope="module")
def golden():
    return S.load_golden()


@pytest.fixture(scope="module")
def refs(golden):
    """the twin in both precisions, once: per-step Adam moments (the fixture keeps the last step's)."""
    return {(c, d): S.recompute(golden, c, d) for c in S.CASES for d in (torch.float32, torch.float64)}


def _padded(values, dtype=torch.float32):
    """a copy of `values` (or that many zeros) followed by 64 sentinel words: (the plane, the whole allocation)."""
    n = values if isinstance(values, int) else int(np.asarray(values).size)
    whole = torch.full((n + 64,), SENTINEL, dtype=dtype, device="cuda")
    if isinstance(values, int):
        whole[:n] = 0
    else:
        whole[:n] = torch.as_tensor(np.ascontiguousarray(values).reshape(-1), dtype=dtype)
    return whole[:n], whole


def _net(in_dim, hidden, sd, rows, in_a, in_b):
    """a ClassifierNet whose params / moments / out8 / workspace sit in sentinel-padded allocations (the workspace of exactly the bytes
    icrl_cls_mlp_ws_bytes asks for)."""
    from icrl_amd import _lib
    from icrl_amd.exploration import ClassifierNet
    net = ClassifierNet(in_dim, hidden, lr=S.LR, device="cuda")
    net._whole = []
    for name in ("params", "exp_avg", "exp_avg_sq"):
        plane, whole = _padded(net.n_params)
        setattr(net, name, plane); net._whole.append(whole)
    plane, whole = _padded(8, torch.float64)
    net.out8 = plane; net._whole.append(whole)
    need = int(_lib.lib().icrl_cls_mlp_ws_bytes(rows, in_a, in_b, hidden[0], hidden[1]))
    assert need > 0
    plane, whole = _padded((need + 7) // 8, torch.float64)
    net._ws = plane.view(torch.int64); net._whole.append(whole)
    net.load_state_dict(sd)
    return net


def _sentinels_intact(*wholes):
    for w in wholes:
        assert torch.all(w[-64:] == SENTINEL).item()


def _inputs(raw, actions, true, rewards):
    """the device planes of one rollout end, each sentinel-padded: xa float64, xb, target, rewards, a zero plane for the shaped costs alone."""
    rows = rewards.size
    xa, w0 = _padded(raw, torch.float64)
    xb, w1 = _padded(actions)
    target, w2 = _padded(np.asarray(true, dtype=np.float32))
    rew, w3 = _padded(rewards)
    shaped, w4 = _padded(rows)
    return dict(xa=xa.view(rows, -1), xb=xb.view(rows, -1), target=target, rewards=rew, shaped=shaped, whole=[w0, w1, w2, w3, w4])


def _rollout_end(net, d, use_nn=True):
    """step, the shaped costs alone (onto zeros: 0 + shaped is exact), then the rewards plane -> the eight scalars on the host."""
    net.step(d["xa"], d["xb"], d["target"])
    net.apply(d["xa"], d["xb"], d["target"], d["shaped"], use_nn=use_nn)
    net.apply(d["xa"], d["xb"], d["target"], d["rewards"], use_nn=use_nn)
    return net.out8.cpu().numpy().copy()


def _check_derived(name, got, want32, rows32, rows64, misses=None):
    """a mean, min or max of per-row values errs by at most the largest per-row error, so it is held to the rule's bound for the per-row
    plane (rows32, rows64) — the two references' own means can cancel to far below any row's distance, and their extremes are single
    elements.  Used where no fixture with cap conditions stands behind the scalar."""
    d, t = abs(float(got) - float(want32)), S.tol(rows32, rows64)
    print(f"{name}: |got - ref32| = {d:.3e}, bound of its rows 4 max|ref32 - ref64| + 1e-12 = {t:.3e}")
    if misses is not None and not d <= t:
        misses.append((name, d, t))
    assert misses is not None or d <= t, (name, d, t)


def _check_mean_p(name, got, p32, p64, misses=None):
    """out4[1], the mean pre-step prediction (not a logged key)."""
    _check_derived(name, got, np.mean(p32, dtype=np.float64), p32, p64, misses)


@pytest.mark.parametrize("case", list(S.CASES))
def test_steps_against_the_fixture(golden, refs, case):
    """three chained rollout ends: parameters, both Adam moments, the pre-step loss, the per-row shaped cost, the rewards plane and the five
    logged scalars against the reference's callback (the per-step moments against the twin the CPU suite ties to the fixture)."""
    misses = []
    obs, act, T, N, hidden = S.CASES[case]
    seed, rows = int(golden[f"{case}_seed"]), T * N
    net = _net(obs + act, hidden, S.state_dict_of(golden, f"{case}_init"), rows, obs, act)
    r32, r64 = refs[case, torch.float32], refs[case, torch.float64]
    for r in range(S.ROLLOUTS):
        pl, raw, true = S.case_inputs(seed, case, r)
        d = _inputs(raw, pl["actions"], true, pl["rewards"])
        out8 = _rollout_end(net, d)
        g = lambda stem: (golden[f"{case}_{stem}_r{r}_32"], S.ref64_of(golden, f"{case}_{stem}_r{r}"))      # noqa: E731
        S.check(f"{case} r{r} params", net.params.cpu().numpy(), *g("params"), misses)
        for name in ("exp_avg", "exp_avg_sq"):
            S.check(f"{case} r{r} {name}", getattr(net, name).cpu().numpy(), r32[f"{name}_r{r}"], r64[f"{name}_r{r}"], misses)
        S.check(f"{case} r{r} shaped", d["shaped"].cpu().numpy().reshape(T, N), *g("shaped"), misses)
        S.check(f"{case} r{r} rewards", d["rewards"].cpu().numpy().reshape(T, N), *g("rewards"), misses)
        log32, log64 = g("log")
        for j, got in enumerate((out8[2], out8[4], out8[5], out8[6], out8[0])):
            S.check(f"{case} r{r} {S.LOG_KEYS[j]}", got, log32[j], log64[j], misses)
        _check_mean_p(f"{case} r{r} mean(p)", out8[1], r32[f"p_pre_r{r}"], r64[f"p_pre_r{r}"], misses)
        assert out8[3] == 0.0 and out8[7] == 0.0
        _sentinels_intact(*d["whole"])
    for name in ("exp_avg", "exp_avg_sq"):
        key = f"{case}_{name}_r{S.ROLLOUTS - 1}"
        S.check(key, getattr(net, name).cpu().numpy(), golden[key + "_32"], S.ref64_of(golden, key), misses)
    assert int(net.adam_step.item()) == S.ROLLOUTS
    _sentinels_intact(*net._whole)
    assert not misses, misses


def _against_twin(obs, act, rows, hidden, n_steps, seed, all_ones=False, all_through_xb=False):
    """n_steps chained rollout ends on `rows` rows against the float32 and float64 twins of an nn.Sequential built here, by the rule.
    all_through_xb: in_a = 0, the float32 (observation | action) rows handed over as one xb plane and xa = None."""
    torch.manual_seed(seed)
    net32 = S.make_net(obs + act, hidden)
    sd = {k: v.clone() for k, v in net32.state_dict().items()}
    rs = np.random.RandomState(seed)
    raw = (2.0 * rs.randn(rows, 1, obs)).astype(np.float32 if all_through_xb else np.float64).astype(np.float64)
    actions = (1.5 * np.tanh(rs.randn(rows, 1, act))).astype(np.float32)
    rewards = rs.randn(rows, 1).astype(np.float32)
    true = np.ones((rows, 1), dtype=bool) if all_ones else raw[..., 0] <= 0.0
    ref = {}
    for dtype in (torch.float32, torch.float64):
        tw = S.make_net(obs + act, hidden, sd, dtype)
        opt = torch.optim.Adam(tw.parameters(), lr=S.LR)
        rw, steps = rewards, []
        for _ in range(n_steps):
            steps.append(S.twin_rollout_end(tw, opt, raw, actions, rw, true, dtype))
            rw = rewards      # (every step shapes a fresh copy of the same rewards plane)
        ref[dtype] = dict(steps=steps, params=S.flat(tw), exp_avg=S.adam_flat(opt, tw, "exp_avg"), exp_avg_sq=S.adam_flat(opt, tw, "exp_avg_sq"))
    in_a, in_b = (0, obs + act) if all_through_xb else (obs, act)
    net = _net(obs + act, hidden, sd, rows, in_a, in_b)
    for s in range(n_steps):
        d = _inputs(raw, actions, true, rewards)
        if all_through_xb:
            xb, w = _padded(np.concatenate([raw.reshape(rows, obs).astype(np.float32), actions.reshape(rows, act)], -1))
            d["xa"], d["xb"] = None, xb.view(rows, obs + act)
            d["whole"].append(w)
        out8 = _rollout_end(net, d)
        e32, e64 = ref[torch.float32]["steps"][s], ref[torch.float64]["steps"][s]
        S.check(f"step {s} shaped", d["shaped"].cpu().numpy(), e32["shaped"].reshape(-1), e64["shaped"].reshape(-1))
        S.check(f"step {s} rewards", d["rewards"].cpu().numpy(), e32["rewards"].reshape(-1), e64["rewards"].reshape(-1))
        S.check(f"step {s} {S.LOG_KEYS[0]}", out8[2], e32["log"][0], e64["log"][0])
        y = true.reshape(-1).astype(np.float64)
        terms = [-(y * np.log(e["p_pre"].astype(np.float64)) + (1 - y) * np.log1p(-e["p_pre"].astype(np.float64))) for e in (e32, e64)]
        _check_derived(f"step {s} {S.LOG_KEYS[4]}", out8[0], e32["log"][4], *terms)      # the loss: the mean of the per-row BCE terms
        for j, got in ((1, out8[4]), (2, out8[5]), (3, out8[6])):
            _check_derived(f"step {s} {S.LOG_KEYS[j]}", got, e32["log"][j], e32["shaped"], e64["shaped"])
        got_shaped = d["shaped"].cpu().numpy().astype(np.float64)
        assert out8[5] == got_shaped.min() and out8[6] == got_shaped.max()      # exact, of the plane the call wrote
        _check_mean_p(f"step {s} mean(p)", out8[1], e32["p_pre"], e64["p_pre"])
        _sentinels_intact(*d["whole"])
    for name in ("params", "exp_avg", "exp_avg_sq"):
        S.check(name, getattr(net, name).cpu().numpy(), ref[torch.float32][name], ref[torch.float64][name])
    _sentinels_intact(*net._whole)


@pytest.mark.parametrize("rows", [1, 33, 8191, 8193])
def test_row_and_grid_edges(rows):
    """cls_tile_kernel walks 32-row groups on min(groups, 256) workgroups.  1 row: one group with one live row; 33: a second group with one;
    8191: 256 groups, the last one ragged; 8193: 257 groups, workgroup 0 alone takes a second one, which holds a single live row."""
    assert min(-(-rows // 32), 256) == {1: 1, 33: 2, 8191: 256, 8193: 256}[rows]
    _against_twin(9, 2, rows, (50, 50), 2, 20 + rows)


def test_all_targets_one():
    _against_twin(9, 2, 45, (50, 50), 2, 31, all_ones=True)


def test_all_inputs_through_xb():
    """in_a = 0 (xa = None), the 11 inputs in the float32 xb plane, 45 rows."""
    _against_twin(9, 2, 45, (50, 50), 2, 32, all_through_xb=True)


def test_the_largest_served_shape():
    """in_a 128, in_b 16, hidden 64 / 64: no padding in the hidden layers, every weight-gradient tile of every wave in use, the largest LDS
    image the kernel asks for; 45 rows: one full group and a ragged one."""
    _against_twin(128, 16, 45, (64, 64), 2, 33)


@pytest.mark.parametrize("use_nn", [True, False])
def test_the_same_call_twice_gives_the_same_bits(golden, use_nn):
    obs, act, T, N, hidden = S.CASES["c"]
    pl, raw, _ = S.case_inputs(5, "c", 0)
    true = raw[..., 0] <= float(np.median(raw[..., 0]))
    outs = []
    for _ in range(2):
        net = _net(obs + act, hidden, S.state_dict_of(golden, "c_init"), T * N, obs, act)
        d = _inputs(raw, pl["actions"], true, pl["rewards"])
        for _ in range(2):
            out8 = _rollout_end(net, d, use_nn=use_nn)
        outs.append([t.cpu().numpy().copy() for t in (net.params, net.exp_avg, net.exp_avg_sq, d["rewards"], d["shaped"])] + [out8])
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("rows", [15, 4099, 70001])
def test_without_the_network_the_rewards_take_the_scaled_true_cost_bit_for_bit(rows):
    """params == NULL: rewards = float32(float64(rewards) + log(1e-3) * target) and out4 is the closed form; 70 001 rows: past one trip of the
    256-workgroup walk."""
    from icrl_amd import _lib
    rs = np.random.RandomState(rows)
    target = rs.randint(0, 3, rows).astype(np.float32)
    before = (rs.randn(rows) * 10 ** rs.uniform(-3, 3, rows)).astype(np.float32)
    t, w0 = _padded(target)
    rew, w1 = _padded(before)
    out4, w2 = _padded(4, torch.float64)
    ws, w3 = _padded(1024, torch.float64)
    _lib.check(_lib.lib().icrl_cost_shaping_apply(None, None, None, _lib.ptr(t), rows, 9, 2, 50, 50, _lib.ptr(rew), _lib.ptr(out4), _lib.ptr(ws), 8192,
                                                  _lib.current_stream()), "icrl_cost_shaping_apply")
    want = (before.astype(np.float64) + np.log(1e-3) * target).astype(np.float32)
    assert np.array_equal(rew.cpu().numpy(), want)
    mean_true = np.mean(target.astype(np.float64))
    assert out4.cpu().numpy().tolist() == [np.log(1e-3) * mean_true, np.log(1e-3) * float(target.max()), np.log(1e-3) * float(target.min()), 0.0]
    _sentinels_intact(w0, w1, w2, w3)


# ---- the callback on a filled buffer ----------------------------------------------------------------------------------------------------
def _stub_model(obs, act, T, N, norm, seed):
    from icrl_amd import spaces
    from icrl_amd.buffers import RolloutBufferWithCost
    from icrl_amd.vec_env import VecNormalize
    ospace, aspace = spaces.Box(-np.inf, np.inf, (obs,)), spaces.Box(-1.0, 1.0, (act,))
    rb = RolloutBufferWithCost(T, ospace, aspace, device="cuda", n_envs=N, reward_gae_lambda=0.95, cost_gae_lambda=0.95)
    ag = dict(last_v_r=torch.zeros(N, device="cuda"), last_v_c=torch.zeros(N, device="cuda"), last_dones=torch.zeros(N, dtype=torch.uint8, device="cuda"))
    mean, var = S.statistics(seed, obs)
    rms = types.SimpleNamespace(d_mean=torch.as_tensor(mean, device="cuda"), d_var=torch.as_tensor(var, device="cuda"))
    env = types.SimpleNamespace(action_space=aspace, norm_obs=norm, obs_rms=rms, epsilon=S.EPSILON, device=torch.device("cuda"))
    env.unnormalize_obs = lambda o: VecNormalize.unnormalize_obs(env, o)      # the env's own method on the stub's statistics
    return types.SimpleNamespace(rollout_buffer=rb, env=env, policy=types.SimpleNamespace(discrete=False), _ag=ag)


def _fill(rb, pl):
    for k, v in pl.items():
        getattr(rb, k).copy_(torch.as_tensor(v))
    rb.full = True


@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("cost", ["analytic", "region", "callable"])
def test_callback_feeds_raw_observations_and_the_cost_objects_own_targets(golden, norm, cost):
    from icrl_amd import logger
    from icrl_amd.exploration import CostShapingCallback
    from icrl_amd.true_constraint_net import AnalyticCost, RegionCost
    obs, act, T, N, hidden = S.CASES["a"]
    seed = int(golden["a_seed"])
    thr = S.threshold(seed, "a") if norm else 0.1
    tc = {"analytic": AnalyticCost.wall_behind(thr), "region": RegionCost.wall_behind(thr, 0, obs, act), "callable": S.wall(thr)}[cost]
    logger.configure()
    model = _stub_model(obs, act, T, N, norm, seed)
    cb = CostShapingCallback(tc, obs, act, True, cost_net_hidden_layers=list(hidden), device="cuda")
    cb.init_callback(model)
    cb.cost_net.load_state_dict(S.state_dict_of(golden, "a_init"))
    rb = model.rollout_buffer
    pl = S.planes(seed, 0, obs, act, T, N)
    _fill(rb, pl)
    cb.on_rollout_end()
    raw = cb.raw_observations
    assert raw.dtype == torch.float64 and tuple(raw.shape) == (T, N, obs)
    assert torch.equal(raw, torch.as_tensor(model.env.unnormalize_obs(rb.observations), dtype=torch.float64))
    host = S.unnormalize(pl["observations"], *S.statistics(seed, obs)) if norm else pl["observations"].astype(np.float64)
    assert np.array_equal(raw.cpu().numpy(), host)
    want = np.asarray(tc(host, pl["actions"]), dtype=np.float32).reshape(-1)
    assert 0 < want.sum() < want.size
    assert np.array_equal(cb.true_costs.cpu().numpy(), want)
    rec = cb.history[-1]
    assert list(rec) == list(S.LOG_KEYS) and all(np.isfinite(v) for v in rec.values())
    assert rec["CostShaping/mean_true_cost"] == float(np.mean(want.astype(np.float64)))
    assert all(logger.Logger.CURRENT.name_to_value[k] == v for k, v in rec.items())
    if norm and cost == "analytic":      # the fixture's first rollout end, through the callback
        misses = []
        S.check("rewards", rb.rewards.cpu().numpy(), golden["a_rewards_r0_32"], S.ref64_of(golden, "a_rewards_r0"), misses)
        log32, log64 = golden["a_log_r0_32"], S.ref64_of(golden, "a_log_r0")
        for j, k in enumerate(S.LOG_KEYS):
            S.check(k, rec[k], log32[j], log64[j], misses)
        assert not misses, misses


def test_recompute_advantages_reaches_the_advantages_and_returns(golden):
    from icrl_amd.exploration import CostShapingCallback
    from icrl_amd.true_constraint_net import AnalyticCost
    obs, act, T, N, hidden = S.CASES["a"]
    seed = int(golden["a_seed"])
    pl = S.planes(seed, 0, obs, act, T, N)
    rs = np.random.RandomState(4)
    pl.update(reward_values=rs.randn(T, N).astype(np.float32), cost_values=rs.randn(T, N).astype(np.float32),
              dones=(rs.rand(T, N) < 0.2).astype(np.float32))
    last_v_r = torch.as_tensor(rs.randn(N).astype(np.float32))
    for recompute in (False, True):
        model = _stub_model(obs, act, T, N, True, seed)
        model._ag["last_v_r"].copy_(last_v_r)
        rb = model.rollout_buffer
        _fill(rb, pl)
        rb.compute_returns_and_advantage(model._ag["last_v_r"], model._ag["last_v_c"], model._ag["last_dones"])
        before = rb.reward_advantages.clone()
        cb = CostShapingCallback(AnalyticCost.wall_behind(S.threshold(seed, "a")), obs, act, True, cost_net_hidden_layers=list(hidden), device="cuda",
                                 recompute_advantages=recompute)
        cb.init_callback(model)
        cb.cost_net.load_state_dict(S.state_dict_of(golden, "a_init"))
        cb.on_rollout_end()
        assert not torch.equal(rb.rewards.cpu(), torch.as_tensor(pl["rewards"]))
        if not recompute:      # the reference's default: the stored rewards change, what the update consumes does not
            assert torch.equal(rb.reward_advantages, before)
            continue
        copy = _stub_model(obs, act, T, N, True, seed).rollout_buffer
        _fill(copy, pl)
        copy.rewards.copy_(rb.rewards)
        copy.compute_returns_and_advantage(model._ag["last_v_r"], model._ag["last_v_c"], model._ag["last_dones"])
        for k in ("reward_advantages", "reward_returns", "cost_advantages", "cost_returns"):
            assert torch.equal(getattr(rb, k), getattr(copy, k)), k
        assert not torch.equal(rb.reward_advantages, before)


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
_GAIL = ("-tei", "HCWithPos-v0", "-eei", "HCWithPosTest-v0", "-nt", "4", "-ns", "32", "-t", "256", "-s", "0", "-v", "0")
# a halfspace on the raw x position, x >= 0: the envs start within +-0.1 of 0 and move either way
_SPEC = json.dumps({"combine": "any", "clauses": [{"type": "halfspace", "cols": ["obs:0"], "w": [1.0], "b": 0.0}]})


def _probe(shaping):
    """a callback that rides in the list behind the shaping callback: at every rollout end the route of the rollout just collected, and the
    cost object's own mean over the un-normalised buffer."""
    from icrl_amd import callbacks

    class Probe(callbacks.BaseCallback):
        def __init__(self):
            super().__init__(0)
            self.routes, self.means = [], []

        def _on_rollout_end(self):
            self.routes.append(routes.rollout())
            if shaping is not None:
                rb = self.model.rollout_buffer
                raw = torch.as_tensor(self.training_env.unnormalize_obs(rb.observations), dtype=torch.float64)
                assert torch.equal(raw, shaping.raw_observations)
                c = np.asarray(shaping.true_cost_function(raw.cpu().numpy(), rb.actions.cpu().numpy()), dtype=np.float64)
                self.means.append(float(np.mean(c)))

    return Probe()


def _gail(extra):
    from icrl_amd import gail as G, logger
    cfg = vars(G.build_parser().parse_args(["gail", *_GAIL, *extra]))
    cfg.update(rank=0, world_size=1)
    cfg = types.SimpleNamespace(**cfg)
    logger.configure()
    model, cb, disc, update = G.setup(cfg, log=None)
    from icrl_amd.exploration import CostShapingCallback
    probe = _probe(update if isinstance(update, CostShapingCallback) else None)
    cb.callbacks.insert(1, probe)
    model.learn(total_timesteps=int(cfg.timesteps), callback=cb)
    G.finish(cfg, model, disc)
    return model, cb, update, probe


@pytest.fixture(scope="module")
def plain_routes():
    """the rollout routes of the same gail run without the flag."""
    return _gail(())[3].routes


@pytest.mark.parametrize("extra", [(), ("--cost_spec", _SPEC)], ids=["env-cost", "cost-spec"])
@pytest.mark.parametrize("use_nn", [True, False], ids=["ucn", "no-ucn"])
def test_gail_with_the_flag_end_to_end(plain_routes, extra, use_nn):
    from icrl_amd.exploration import CostShapingCallback
    from icrl_amd.gail_utils import GailCallback
    model, cb, update, probe = _gail(("-ucsc",) + (("-ucn",) if use_nn else ()) + extra)
    assert isinstance(update, CostShapingCallback) and update.use_nn == use_nn
    assert not any(isinstance(c, GailCallback) for c in cb.callbacks)
    hist = update.history
    assert len(hist) == 2 == len(probe.routes)
    for rec, mean, route, plain in zip(hist, probe.means, probe.routes, plain_routes):
        print(rec)
        assert list(rec) == list(S.LOG_KEYS) and all(np.isfinite(v) for v in rec.values()), rec
        assert rec["CostShaping/mean_true_cost"] == mean
        if extra:
            assert 0.0 < mean < 1.0, mean      # both classes occur
        if not use_nn:
            assert rec["CostShaping/mean_shaped_cost"] == np.log(1e-3) * rec["CostShaping/mean_true_cost"]
        assert route["route"] != "none" and route == plain, (route, plain)
    assert torch.isfinite(update.cost_net.params).all().item() and int(update.cost_net.adam_step.item()) == 2
    assert torch.isfinite(model.policy.params).all().item()
