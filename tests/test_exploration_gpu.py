"""GPU: the exploration callbacks' regression step (icrl_reg_mlp_step), the advantage shaping (icrl_shape_advantages), the callbacks on a
filled buffer and inside cpg / icrl, against the reference's own callbacks as recorded in tests/golden/g25_exploration.npz.

Tolerance rule for every quantity compared with the reference: 4 x max |ref32 - ref64| of that quantity + 1e-12, compared against ref32 (both
implementations sit about one float32 rounding from the exact value: a factor 2; another 2 for a different summation order); the fixture's
cap conditions keep the rule from hiding a failure.  helpers.exploration_cases.check prints the measured distance next to the bound."""
import os
import types

import numpy as np
import pytest
import torch

from helpers import exploration_cases as X

pytestmark = pytest.mark.gpu
SENTINEL = 7.25


@pytest.fixture(scope="module")
def golden():
    return X.load_golden()


@pytest.fixture(scope="module")
def refs(golden):
    """the torch recomputation in both precisions, once: per-step parameters and Adam moments (the fixture keeps the final parameters)."""
    return {(c, d): X.recompute(golden, c, "l", d) for c in X.CASES for d in (torch.float32, torch.float64)}


def _padded(n, dtype=torch.float32):
    """n values followed by 64 sentinel words: (the plane, the whole allocation)."""
    whole = torch.full((n + 64,), SENTINEL, dtype=dtype, device="cuda")
    return whole[:n], whole


def _net(in_dim, out_dim, hidden, sd):
    """a RegressionNet whose params / moments / out4 sit in sentinel-padded allocations."""
    from icrl_amd.exploration import RegressionNet
    net = RegressionNet(in_dim, out_dim, hidden, lr=X.LR, device="cuda")
    net._whole = []
    for name in ("params", "exp_avg", "exp_avg_sq"):
        plane, whole = _padded(net.n_params)
        plane.copy_(getattr(net, name)); setattr(net, name, plane); net._whole.append(whole)
    plane, whole = _padded(4)
    net.out4 = plane; net._whole.append(whole)
    net.load_state_dict(sd)
    return net


def _sentinels_intact(*wholes):
    for w in wholes:
        assert torch.all(w[-64:] == SENTINEL).item()


def _dev(pl):
    return {k: torch.as_tensor(v, device="cuda").contiguous() for k, v in pl.items()}


@pytest.mark.parametrize("case", list(X.CASES))
def test_steps_against_the_fixture(golden, refs, case):
    """three chained steps of the predictor and of the out = 1 cost net: row_err, out4 and the final parameters against the reference's
    callbacks, the parameters and both Adam moments of every step against the torch recomputation the CPU suite ties to the fixture."""
    misses = []
    obs, act, T, N, hidden = X.CASES[case]
    seed, rows = int(golden[f"{case}_seed"]), T * N
    pred = _net(obs + act, obs, hidden, X.state_dict_of(golden, f"{case}_l_pred_init"))
    cost = _net(obs + act, 1, hidden, X.state_dict_of(golden, f"{case}_l_cost_init"))
    row_err, row_whole = _padded(rows)
    r32, r64 = refs[case, torch.float32], refs[case, torch.float64]
    for r in range(X.ROLLOUTS):
        pl = _dev(X.planes(seed, r, obs, act, T, N))
        c4 = cost.step(pl["observations"], pl["actions"], pl["costs"]).cpu().numpy().copy()
        p4 = pred.step(pl["observations"], pl["actions"], pl["new_observations"], row_err).cpu().numpy().copy()
        key = f"{case}_l_row_err_r{r}"
        X.check(key, row_err.cpu().numpy(), golden[key + "_32"].reshape(-1), X.ref64_of(golden, key).reshape(-1), misses)
        log32, log64 = golden[f"{case}_l_log_r{r}_32"], X.ref64_of(golden, f"{case}_l_log_r{r}")      # mean, std, predictor MSE, cost MSE
        for name, got, j in (("mean", p4[1], 0), ("std", p4[2], 1), ("pred loss", p4[0], 2), ("cost loss", c4[0], 3)):
            X.check(f"{case} r{r} out4 {name}", got, log32[j], log64[j], misses)
        assert p4[3] == 0.0 and c4[3] == 0.0
        for short, net in (("pred", pred), ("cost", cost)):
            for name in ("params", "exp_avg", "exp_avg_sq"):
                X.check(f"{case} r{r} {short} {name}", getattr(net, name).cpu().numpy(), r32[f"{short}_{name}_r{r}"], r64[f"{short}_{name}_r{r}"], misses)
    for short, net in (("pred", pred), ("cost", cost)):
        key = f"{case}_l_{short}_params"
        X.check(key, net.params.cpu().numpy(), golden[key + "_32"], X.ref64_of(golden, key), misses)
        assert int(net.adam_step.item()) == X.ROLLOUTS
        _sentinels_intact(*net._whole)
    _sentinels_intact(row_whole)
    assert not misses, misses


def test_the_same_call_twice_gives_the_same_bits(golden):
    obs, act, T, N, hidden = X.CASES["c"]
    pl = _dev(X.planes(5, 0, obs, act, T, N))
    outs = []
    for _ in range(2):
        net = _net(obs + act, obs, hidden, X.state_dict_of(golden, "c_l_pred_init"))
        row_err = torch.zeros(T * N, device="cuda")
        for _ in range(2):
            out4 = net.step(pl["observations"], pl["actions"], pl["new_observations"], row_err)
        outs.append([t.cpu().numpy().copy() for t in (net.params, net.exp_avg, net.exp_avg_sq, row_err, out4)])
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def _against_torch(obs, act, out_dim, rows, hidden, n_steps, seed, all_through_xb=False):
    """n_steps chained steps on `rows` rows against float32 and float64 torch runs of an nn.Sequential built here, by the rule.
    all_through_xb: in_a = 0, the (observation | action) rows handed over as one xb plane and xa = None."""
    torch.manual_seed(seed)
    net32 = X.make_net(obs + act, out_dim, hidden)
    sd = {k: v.clone() for k, v in net32.state_dict().items()}
    net64 = X.make_net(obs + act, out_dim, hidden, sd, torch.float64)
    pl = X.planes(seed + 66, 0, obs, act, rows, 1)
    target = pl["new_observations"].reshape(rows, -1)[:, :out_dim].copy()
    ref = {}
    for net, np_t in ((net32, np.float32), (net64, np.float64)):
        opt = torch.optim.Adam(net.parameters(), lr=X.LR)
        x = torch.from_numpy(np.concatenate([pl["observations"], pl["actions"]], -1).reshape(rows, -1).astype(np_t))
        steps = [X.torch_step(net, opt, x, torch.from_numpy(target.astype(np_t))) for _ in range(n_steps)]
        ref[np_t] = dict(steps=steps, params=X.flat(net), exp_avg=X.adam_flat(opt, net, "exp_avg"), exp_avg_sq=X.adam_flat(opt, net, "exp_avg_sq"))
    dev = _dev(pl)
    d_target = torch.as_tensor(target, device="cuda").contiguous()
    net = _net(obs + act, out_dim, hidden, sd)
    row_err, row_whole = _padded(rows)
    xa, xb = dev["observations"], dev["actions"]
    if all_through_xb:
        xa, xb = None, torch.cat([xa.reshape(rows, obs), xb.reshape(rows, act)], -1).contiguous()
        assert tuple(xb.shape) == (rows, obs + act)
    for s in range(n_steps):
        out4 = net.step(xa, xb, d_target, row_err).cpu().numpy()
        e32, e64 = ref[np.float32]["steps"][s], ref[np.float64]["steps"][s]
        X.check(f"step {s} row_err", row_err.cpu().numpy(), e32[0], e64[0])
        X.check(f"step {s} loss", out4[0], e32[1], e64[1])
        X.check(f"step {s} mean", out4[1], np.mean(e32[0]), np.mean(e64[0]))
        X.check(f"step {s} std", out4[2], np.std(e32[0]), np.std(e64[0]))
    for name in ("params", "exp_avg", "exp_avg_sq"):
        X.check(name, getattr(net, name).cpu().numpy(), ref[np.float32][name], ref[np.float64][name])
    _sentinels_intact(row_whole, *net._whole)


def test_more_rows_than_the_sibling_entry_points_serve():
    """70 001 rows at (obs 9, act 2): above the 65 536 rows of icrl_cost_mlp_fwd_bwd, every workgroup walks several groups, ragged tail."""
    _against_torch(9, 2, 9, 70001, (50, 50), 2, 11)


@pytest.mark.parametrize("rows", [8192, 8193])
def test_the_edge_of_the_grid_cap(rows):
    """reg_mlp_tile_kernel walks 32-row groups on min(groups, 256) workgroups.  8192 rows: 256 groups, every workgroup takes exactly one;
    8193 rows: 257 groups, workgroup 0 alone takes a second one, which holds a single live row."""
    assert -(-rows // 32) == 256 + (rows > 8192)
    _against_torch(9, 2, 9, rows, (50, 50), 2, 13)


def test_all_inputs_through_xb():
    """in_a = 0 (xa = None), the 11 inputs in the xb plane, 45 rows: a served shape (rm_check: in_a 0..) that no caller takes."""
    _against_torch(9, 2, 9, 45, (50, 50), 2, 14, all_through_xb=True)


def test_the_largest_served_shape():
    """in_a 128, in_b 16, hidden 64 / 64, out 128: no padding anywhere, every weight-gradient tile of every wave in use, and the largest
    LDS image the kernel asks for (158 KB of the 160 KB); 45 rows: one full group and a ragged one."""
    _against_torch(128, 16, 128, 45, (64, 64), 2, 12)


def test_buffers_hold_exactly_n_params_at_the_reference_widths():
    from icrl_amd.exploration import RegressionNet
    net = RegressionNet(24, 18, [50, 50], device="cuda")
    assert net.n_params == 50 * 24 + 50 + 50 * 50 + 50 + 18 * 50 + 18
    assert net.params.numel() == net.exp_avg.numel() == net.exp_avg_sq.numel() == net.n_params
    sd = net.state_dict()
    assert list(sd) == list(X.KEYS) and sd["0.weight"].shape == (50, 24) and sd["4.weight"].shape == (18, 50)
    ref = X.make_net(24, 18, (50, 50), sd)
    assert np.array_equal(X.flat(ref), net.params.cpu().numpy())


@pytest.mark.parametrize("rows", [15, 4099])
def test_shape_advantages_is_torch_float32_division_bit_for_bit(rows):
    from icrl_amd import _lib
    rs = np.random.RandomState(rows)
    adv, whole = _padded(rows)
    adv.copy_(torch.as_tensor(rs.randn(rows).astype(np.float32)))
    err = torch.as_tensor((rs.rand(rows) * 10 ** rs.uniform(-6, 3, rows)).astype(np.float32), device="cuda")
    want = (adv.cpu() / (1 + err.cpu())).numpy()
    _lib.check(_lib.lib().icrl_shape_advantages(_lib.ptr(adv), _lib.ptr(err), rows, _lib.current_stream()), "icrl_shape_advantages")
    assert np.array_equal(adv.cpu().numpy(), want)
    _sentinels_intact(whole)


def _stub_model(obs, act, T, N):
    from icrl_amd import spaces
    from icrl_amd.buffers import RolloutBufferWithCost
    ospace, aspace = spaces.Box(-np.inf, np.inf, (obs,)), spaces.Box(-1.0, 1.0, (act,))
    rb = RolloutBufferWithCost(T, ospace, aspace, device="cuda", n_envs=N, reward_gae_lambda=0.95, cost_gae_lambda=0.95)
    ag = dict(last_v_r=torch.zeros(N, device="cuda"), last_v_c=torch.zeros(N, device="cuda"), last_dones=torch.zeros(N, dtype=torch.uint8, device="cuda"))
    return types.SimpleNamespace(rollout_buffer=rb, env=types.SimpleNamespace(action_space=aspace), policy=types.SimpleNamespace(discrete=False), _ag=ag)


def _fill(rb, pl):
    for k, v in pl.items():
        getattr(rb, k).copy_(torch.as_tensor(v))
    rb.full = True


@pytest.mark.parametrize("case", list(X.CASES))
def test_callbacks_against_the_fixture(golden, case):
    """both callbacks on a filled RolloutBufferWithCost with a stub model, three rollouts: the rewards plane after the exploration callback
    and every logged key within the rule; cost_advantages after the lambda callback bit for bit a / (1 + row_err) of the kernel's row_err."""
    misses = []
    from icrl_amd import logger
    from icrl_amd.exploration import ExplorationRewardCallback, LambdaShapingCallback
    obs, act, T, N, hidden = X.CASES[case]
    seed = int(golden[f"{case}_seed"])
    logger.configure()
    model = _stub_model(obs, act, T, N)
    ecb = ExplorationRewardCallback(obs, act, hidden_layers=list(hidden), device="cuda")
    lcb = LambdaShapingCallback(obs, act, cost_net_hidden_layers=list(hidden), predictor_net_hidden_layers=list(hidden), device="cuda")
    ecb.init_callback(model); lcb.init_callback(model)
    ecb.predictor_network.load_state_dict(X.state_dict_of(golden, f"{case}_e_pred_init"))
    lcb.predictor_network.load_state_dict(X.state_dict_of(golden, f"{case}_l_pred_init"))
    lcb.cost_net.load_state_dict(X.state_dict_of(golden, f"{case}_l_cost_init"))
    rb = model.rollout_buffer
    for r in range(X.ROLLOUTS):
        pl = X.planes(seed, r, obs, act, T, N)
        _fill(rb, pl)
        ecb.on_rollout_end()
        key = f"{case}_e_rewards_r{r}"
        X.check(key, rb.rewards.cpu().numpy(), golden[key + "_32"], X.ref64_of(golden, key), misses)
        X.check(f"{case}_e_log_r{r}", logger.Logger.CURRENT.name_to_value["exploration/predictor_network_loss"], golden[f"{case}_e_log_r{r}_32"][0],
                X.ref64_of(golden, f"{case}_e_log_r{r}")[0], misses)
        _fill(rb, pl)
        lcb.on_rollout_end()
        want = torch.as_tensor(pl["cost_advantages"]) / (1 + lcb.row_err.cpu().view(T, N))
        assert np.array_equal(rb.cost_advantages.cpu().numpy(), want.numpy())
        key = f"{case}_l_cost_adv_r{r}"
        X.check(key, rb.cost_advantages.cpu().numpy(), golden[key + "_32"], X.ref64_of(golden, key), misses)
        log32, log64 = golden[f"{case}_l_log_r{r}_32"], X.ref64_of(golden, f"{case}_l_log_r{r}")
        for j, k in enumerate(("exploration/mean_exploration_reward", "exploration/std_exploration_reward", "exploration/predictor_network_loss",
                               "exploration/cost_network_loss")):
            X.check(f"{case} r{r} {k}", logger.Logger.CURRENT.name_to_value[k], log32[j], log64[j], misses)
    assert len(ecb.history) == len(lcb.history) == X.ROLLOUTS
    assert not misses, misses


def test_recompute_advantages_reaches_the_advantages_and_returns(golden):
    from icrl_amd.exploration import ExplorationRewardCallback
    obs, act, T, N, hidden = X.CASES["a"]
    pl = X.planes(3, 0, obs, act, T, N)
    rs = np.random.RandomState(4)
    pl.update(reward_values=rs.randn(T, N).astype(np.float32), cost_values=rs.randn(T, N).astype(np.float32),
              dones=(rs.rand(T, N) < 0.2).astype(np.float32))
    got = {}
    for recompute in (False, True):
        model = _stub_model(obs, act, T, N)
        model._ag["last_v_r"].copy_(torch.as_tensor(rs.randn(N).astype(np.float32)))
        rb = model.rollout_buffer
        _fill(rb, pl)
        rb.compute_returns_and_advantage(model._ag["last_v_r"], model._ag["last_v_c"], model._ag["last_dones"])
        before = rb.reward_advantages.clone()
        cb = ExplorationRewardCallback(obs, act, hidden_layers=list(hidden), device="cuda", recompute_advantages=recompute)
        cb.init_callback(model)
        cb.predictor_network.load_state_dict(X.state_dict_of(golden, "a_e_pred_init"))
        cb.on_rollout_end()
        if not recompute:      # the reference's default: the stored rewards change, what the update consumes does not
            assert torch.equal(rb.reward_advantages, before) and not torch.equal(rb.rewards.cpu(), torch.as_tensor(pl["rewards"]))
            continue
        copy = _stub_model(obs, act, T, N).rollout_buffer
        _fill(copy, pl)
        copy.rewards.copy_(rb.rewards)
        copy.compute_returns_and_advantage(model._ag["last_v_r"], model._ag["last_v_c"], model._ag["last_dones"])
        for k in ("reward_advantages", "reward_returns", "cost_advantages", "cost_returns"):
            assert torch.equal(getattr(rb, k), getattr(copy, k)), k
        assert not torch.equal(rb.reward_advantages, before)


_CPG = ("-tei", "HCWithPos-v0", "-eei", "HCWithPosTest-v0", "-nt", "4", "--n_steps", "32", "-t", "256")
_KEYS = ("exploration/mean_exploration_reward", "exploration/std_exploration_reward", "exploration/predictor_network_loss", "exploration/cost_network_loss")


def _cpg(extra, seed=0):
    from icrl_amd import cpg as C
    from icrl_amd.streams import PrivateStreams
    cfg = vars(C.build_parser().parse_args(["cpg", *_CPG, "-s", str(seed), "-v", "0", *extra]))
    cfg.update(rank=0, world_size=1, streams=PrivateStreams(seed), eval_noise_from_streams=True)
    cfg = types.SimpleNamespace(**cfg)
    model, cb, learn_cost, hist = C.setup(cfg, log=None)
    model.learn(total_timesteps=int(cfg.timesteps), cost_function=learn_cost, callback=cb)
    return model.policy.params.cpu().numpy().copy(), hist.history


def test_cpg_with_both_flags_end_to_end(monkeypatch):
    """cpg -uls -ucde: every history record carries the exploration keys; a control run whose (test-only) callback shapes the cost advantages
    itself with torch from the same row_err ends with the same policy bits — the update, pre-gathered minibatch stream included, consumes
    the shaped plane — and the run without -uls ends elsewhere."""
    from icrl_amd import exploration
    params, history = _cpg(("-uls", "-ucde"))
    assert len(history) == 2
    for rec in history:
        assert all(k in rec and np.isfinite(rec[k]) for k in _KEYS), rec

    class Control(exploration.LambdaShapingCallback):
        def _on_rollout_end(self):
            rb = self.model.rollout_buffer
            rows = rb.buffer_size * rb.n_envs
            self.row_err = torch.empty(rows, device=rb.device)
            self.cost_net.step(rb.observations, rb.actions, rb.costs)
            self.predictor_network.step(rb.observations, rb.actions, rb.new_observations, self.row_err)
            rb.cost_advantages.copy_(rb.cost_advantages / (1 + self.row_err.view(rb.buffer_size, rb.n_envs)))

    monkeypatch.setattr(exploration, "LambdaShapingCallback", Control)
    control, _ = _cpg(("-uls", "-ucde"))
    monkeypatch.undo()
    assert np.array_equal(params, control)
    plain, plain_history = _cpg(("-ucde",))
    assert not np.array_equal(params, plain)
    assert all("exploration/cost_network_loss" not in rec and "exploration/predictor_network_loss" in rec for rec in plain_history)
    none, none_history = _cpg(())
    assert all(not any(k.startswith("exploration/") for k in rec) for rec in none_history)
    assert np.array_equal(plain, none)      # the reference's no-effect default of the curiosity callback


def test_icrl_with_the_curiosity_flag():
    """icrl -ucde, two outer iterations: the callback logs exploration/predictor_network_loss at every rollout end of the forward steps, and
    the policy ends bit-identical to the run without the flag on the same streams — the reference's no-effect default (its callback runs
    after GAE and changes only the stored rewards), stated as such."""
    from icrl_amd import icrl as I, logger
    from icrl_amd.icrl import build_parser
    from icrl_amd.streams import PrivateStreams
    expert = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden/expert_hc.npz")
    out = {}
    for extra in ((), ("-ucde",)):
        argv = ["icrl", "-er", "2", "-ep", expert, "-cl", "20", "-bi", "2", "-ft", str(2 * 4 * 32), "-ni", "2", "-tei", "HCWithPos-v0", "-eei", "HCWithPosTest-v0",
                "-nt", "4", "--n_steps", "32", "-ne", "2", "-s", "0", "-v", "0", *extra]
        cfg = vars(build_parser().parse_args(argv))
        cfg.update(rank=0, world_size=1, streams=PrivateStreams(0))
        logger.configure()
        st = I.setup(types.SimpleNamespace(**cfg))
        for it in range(2):
            I.outer_iteration(st, it)
        out[extra] = (st["agent"].policy.params.cpu().numpy().copy(), st.get("exploration_callback"))
    assert out[()][1] is None
    hist = out[("-ucde",)][1].history
    assert len(hist) == 4 and all(np.isfinite(h["exploration/predictor_network_loss"]) and h["exploration/predictor_network_loss"] > 0 for h in hist)
    assert np.array_equal(out[()][0], out[("-ucde",)][0])


def test_discrete_action_spaces_are_refused():
    from icrl_amd import cpg as C
    cfg = vars(C.build_parser().parse_args(["cpg", "-tei", "DD2B-v0", "-eei", "CDD2B-v0", "--use_null_cost", "-uls", "-s", "0", "-v", "0"]))
    cfg.update(rank=0, world_size=1)
    with pytest.raises(ValueError) as e:
        C.setup(types.SimpleNamespace(**cfg), log=None)
    assert "Box action space is needed" in str(e.value) and "--use_lambda_shaping" in str(e.value)
