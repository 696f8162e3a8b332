"""GPU: the input gradients of the policy and of the constraint net (csrc/mlp_grad.hip: icrl_policy_fwd_bwd_in, icrl_cost_mlp_fwd_bwd_in,
icrl_cn_prepare_bwd) through the C ABI, icrl_amd/torch_ops.py input_grads=True, ConstraintNet.saliency and `icrl --cn_saliency`.

Input gradients are compared with float64 CPU autograd of the oracle's networks with the inputs as leaves, under the rule of
tests/helpers/input_grad_cases.py (|kernel - float64| <= 4 dev32 per tensor, dev32 stored there).  Every case prints its figures
(`MLP_GRAD IN ...`) before it asserts."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from helpers import input_grad_cases as G
from helpers import mlp_grad_cases as M

pytestmark = pytest.mark.gpu
OUTS = G.OUTS
FILL, OVER = 7.0, 3      # outputs are pre-filled and over-allocated by OVER rows: rows at or beyond N must keep the fill


def _dev(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).cuda().contiguous()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ---- the policy -------------------------------------------------------------------------------------------------------------------------------------
def _policy_in(c, flat, obs, act, ups, grad=True, d_obs=True, d_act=True, fill=FILL):
    """one icrl_policy_fwd_bwd_in call -> outputs dict, grad | None, d_obs [n + OVER, obs_dim] | None, d_actions [n + OVER, act_dim] | None (numpy)"""
    from icrl_amd import _lib, structs as S
    L = _lib.lib()
    n = obs.shape[0]
    pol = S.PolicyT(c["obs_dim"], c["act_dim"], M.HW, M.HW, int(c["discrete"]), flat.numel(), _lib.ptr(flat), None, None)
    nbytes = L.icrl_policy_fwd_bwd_in_ws_bytes(ctypes.byref(pol), n)
    assert nbytes > 0, L.icrl_last_error()
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
    outs = {k: torch.full((n,), fill, device="cuda") for k in OUTS}
    g = torch.full((flat.numel(),), fill, device="cuda") if grad else None
    dx = torch.full((n + OVER, c["obs_dim"]), fill, device="cuda") if d_obs else None
    da = torch.full((n + OVER, c["act_dim"]), fill, device="cuda") if d_act else None
    _lib.check(L.icrl_policy_fwd_bwd_in(ctypes.byref(pol), _lib.ptr(obs), _lib.ptr(act), n, *[_lib.ptr(ups.get(k)) for k in OUTS], *[_lib.ptr(outs[k]) for k in OUTS],
                                        _lib.ptr(g), _lib.ptr(dx), _lib.ptr(da), _lib.ptr(ws), nbytes, _lib.current_stream()), "icrl_policy_fwd_bwd_in")
    cpu = lambda t: None if t is None else t.cpu().numpy()
    return {k: v.cpu().numpy() for k, v in outs.items()}, cpu(g), cpu(dx), cpu(da)


def _policy_parent(c, flat, obs, act, ups, fill=FILL):
    from icrl_amd import _lib, structs as S
    L = _lib.lib()
    n = obs.shape[0]
    pol = S.PolicyT(c["obs_dim"], c["act_dim"], M.HW, M.HW, int(c["discrete"]), flat.numel(), _lib.ptr(flat), None, None)
    nbytes = L.icrl_policy_fwd_bwd_ws_bytes(ctypes.byref(pol), n)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
    outs = {k: torch.full((n,), fill, device="cuda") for k in OUTS}
    g = torch.full((flat.numel(),), fill, device="cuda")
    _lib.check(L.icrl_policy_fwd_bwd(ctypes.byref(pol), _lib.ptr(obs), _lib.ptr(act), n, *[_lib.ptr(ups.get(k)) for k in OUTS], *[_lib.ptr(outs[k]) for k in OUTS],
                                     _lib.ptr(g), _lib.ptr(ws), nbytes, _lib.current_stream()), "icrl_policy_fwd_bwd")
    return {k: v.cpu().numpy() for k, v in outs.items()}, g.cpu().numpy()


@pytest.mark.parametrize("shape,n", G.POLICY_CASES, ids=[G.case_id(s, n) for s, n in G.POLICY_CASES])
def test_policy_input_gradients_vs_float64_autograd(shape, n):
    """all four upstream gradients at once at a trained state: d_obs against float64 autograd and against (pi + vf) + cvf of three float64 runs,
    d_actions against float64 autograd; outputs and grad bit-equal to icrl_policy_fwd_bwd's; the same bits twice; rows beyond N untouched; a NULL
    d_actions / d_obs / grad leaves the others' bits alone."""
    c = G.policy_case(shape, n)
    tag, box = G.case_id(shape, n), not c["discrete"]
    flat, obs, act = _dev(c["flat"]), _dev(c["obs"]), _dev(c["actions"])
    ups = {k: _dev(v) for k, v in c["ups"].items()}
    outs, g, dx, da = _policy_in(c, flat, obs, act, ups, d_act=box)
    dev32 = G.DEV32[tag]
    names = ["d_obs"] + (["d_actions"] if box else [])
    G.check(tag, names, [dx[:n]] + ([da[:n]] if box else []), [c["d_obs64"]] + ([c["d_act64"]] if box else []), dev32)
    G.check(tag + " (pi + vf) + cvf", ["d_obs"], [dx[:n]], [c["d_obs_sum64"]], dev32[:1])
    assert np.all(dx[n:] == FILL) and (not box or np.all(da[n:] == FILL))
    p_outs, p_g = _policy_parent(c, flat, obs, act, ups)
    assert _same(g, p_g)
    for k in OUTS:
        assert _same(outs[k], p_outs[k]), k
    outs2, g2, dx2, da2 = _policy_in(c, flat, obs, act, ups, d_act=box, fill=-1.0)
    assert _same(g, g2) and _same(dx[:n], dx2[:n]) and (not box or _same(da[:n], da2[:n]))
    _, g3, dx3, none = _policy_in(c, flat, obs, act, ups, d_act=False)
    assert none is None and _same(dx3, dx) and _same(g3, g)
    _, none, dx4, _ = _policy_in(c, flat, obs, act, ups, grad=False, d_act=False)      # grad NULL: the parameter sums stay in scratch
    assert none is None and _same(dx4, dx)
    if box:
        _, g5, none, da5 = _policy_in(c, flat, obs, act, ups, d_obs=False)
        assert none is None and _same(da5, da) and _same(g5, g)


def test_one_branch_at_a_time_gives_that_branchs_gradient():
    """v_r alone, v_c alone, log_prob + entropy alone: each against its own float64 run (the other branches contribute exact zeros)"""
    c = G.policy_case("o17a5", 17)
    flat, obs, act = _dev(c["flat"]), _dev(c["obs"]), _dev(c["actions"])
    dev32 = G.DEV32["o17a5-17"]
    zero = np.zeros(17, np.float32)
    for keep in (("log_prob", "entropy"), ("v_r",), ("v_c",)):
        ups = {k: (c["ups"][k] if k in keep else zero) for k in OUTS}
        ref = G._policy_input_grads(c, torch.float64, ups)[0]
        _, _, dx, da = _policy_in(c, flat, obs, act, {k: (_dev(c["ups"][k]) if k in keep else None) for k in OUTS})
        G.check("o17a5-17 " + "+".join(keep), ["d_obs"], [dx[:17]], [ref], dev32[:1])
        if "log_prob" not in keep:
            assert not da[:17].any()


# ---- the constraint net -----------------------------------------------------------------------------------------------------------------------------
def _constraint_net(c):
    from icrl_amd.constraint_net import ConstraintNet
    lo = None if c["discrete"] else -np.ones(c["acs_dim"], np.float32)
    cn = ConstraintNet(c["obs_dim"], c["acs_dim"], list(c["hidden"]), None, lambda x: 0.05, None, None, c["discrete"], 0.5,
                       None if c["osel"] is None else list(c["osel"]), None if c["asel"] is None else list(c["asel"]), clip_obs=G.CLIP_OBS,
                       action_low=lo, action_high=None if lo is None else -lo)
    cn.load_state_dict(c["sd"])
    return cn


def _cost_in(cn, x, up, grad=True, d_x=True, fill=FILL):
    from icrl_amd import _lib
    L, s, n = _lib.lib(), cn.struct(), x.shape[0]
    nbytes = L.icrl_cost_mlp_fwd_bwd_in_ws_bytes(ctypes.byref(s), n)
    assert nbytes > 0, L.icrl_last_error()
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
    zeta = torch.full((n,), fill, device="cuda")
    g = torch.full((cn.n_params,), fill, device="cuda") if grad else None
    dx = torch.full((n + OVER, x.shape[1]), fill, device="cuda") if d_x else None
    _lib.check(L.icrl_cost_mlp_fwd_bwd_in(ctypes.byref(s), _lib.ptr(x), n, _lib.ptr(up), _lib.ptr(zeta), _lib.ptr(g), _lib.ptr(dx), _lib.ptr(ws), nbytes,
                                          _lib.current_stream()), "icrl_cost_mlp_fwd_bwd_in")
    return zeta.cpu().numpy(), (None if g is None else g.cpu().numpy()), dx


def _prepare_bwd(s, obs, acs, d_x, n, obs_dim, acs_dim, want_acs, fill=FILL):
    from icrl_amd import _lib
    d_obs = torch.full((n + OVER, obs_dim), fill, dtype=torch.float64, device="cuda")
    d_acs = torch.full((n + OVER, acs_dim), fill, device="cuda") if want_acs else None
    _lib.check(_lib.lib().icrl_cn_prepare_bwd(ctypes.byref(s), _lib.ptr(obs), _lib.ptr(acs), n, _lib.ptr(d_x), _lib.ptr(d_obs), _lib.ptr(d_acs),
                                              _lib.current_stream()), "icrl_cn_prepare_bwd")
    return d_obs.cpu().numpy(), (None if d_acs is None else d_acs.cpu().numpy())


@pytest.mark.parametrize("shape,n", G.COST_CASES, ids=[G.case_id(s, n) for s, n in G.COST_CASES])
def test_cost_net_input_gradients_vs_float64_autograd(shape, n):
    """d_x against float64 autograd with x as the leaf; zeta and grad bit-equal to icrl_cost_mlp_fwd_bwd's; the same bits twice; rows beyond N
    untouched; then icrl_cn_prepare_bwd on that d_x: the full chain obs, acs -> zeta against float64 autograd through prepare_data restated."""
    from icrl_amd import _lib
    c = G.cost_case(shape, n)
    assert c["zmin"] >= G.RELU_MARGIN, c["zmin"]
    tag, dev32, box = "cost-" + G.case_id(shape, n), G.DEV32["cost-" + G.case_id(shape, n)], not c["discrete"]
    cn = _constraint_net(c)
    obs, acs, up = _dev(c["obs"], torch.float64), _dev(c["acs"]), _dev(c["up"])
    x = cn.prepare_data(obs, acs)
    assert _same(x.cpu().numpy(), c["x"])
    zeta, g, dx = _cost_in(cn, x, up)
    G.check(tag, ["d_x"], [dx[:n].cpu().numpy()], [c["d_x64"]], dev32[:1])
    assert torch.all(dx[n:] == FILL)
    L, s = _lib.lib(), cn.struct()
    nbytes = L.icrl_cost_mlp_fwd_bwd_ws_bytes(ctypes.byref(s), n)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
    p_zeta, p_g = torch.full((n,), FILL, device="cuda"), torch.full((cn.n_params,), FILL, device="cuda")
    _lib.check(L.icrl_cost_mlp_fwd_bwd(ctypes.byref(s), _lib.ptr(x), n, _lib.ptr(up), _lib.ptr(p_zeta), _lib.ptr(p_g), _lib.ptr(ws), nbytes, _lib.current_stream()),
               "icrl_cost_mlp_fwd_bwd")
    assert _same(zeta, p_zeta.cpu().numpy()) and _same(g, p_g.cpu().numpy())
    zeta2, g2, dx2 = _cost_in(cn, x, up, fill=-1.0)
    assert _same(zeta, zeta2) and _same(g, g2) and _same(dx[:n].cpu().numpy(), dx2[:n].cpu().numpy())
    _, none, dx3 = _cost_in(cn, x, up, grad=False)
    assert none is None and _same(dx3.cpu().numpy(), dx.cpu().numpy())
    _, g4, none = _cost_in(cn, x, up, d_x=False)
    assert none is None and _same(g4, g)
    # the chain rule through prepare_data
    d_obs, d_acs = _prepare_bwd(s, obs, acs, dx[:n].contiguous(), n, c["obs_dim"], c["acs_dim"], box)
    assert np.all(d_obs[n:] == FILL) and (not box or np.all(d_acs[n:] == FILL))
    G.check(tag + " chain", ["d_obs"] + (["d_acs"] if box else []), [d_obs[:n]] + ([d_acs[:n]] if box else []),
            [c["d_obs64"]] + ([c["d_acs64"]] if box else []), dev32[1:])
    assert not d_obs[0, :2].any()      # row 0, columns 0 and 1 lie beyond the observation clip: exactly 0
    d_obs2, _ = _prepare_bwd(s, obs, acs, dx[:n].contiguous(), n, c["obs_dim"], c["acs_dim"], False, fill=-1.0)
    assert _same(d_obs2[:n], d_obs[:n])      # a NULL d_acs leaves d_obs alone; the same bits twice


@pytest.mark.parametrize("name", G.PREPARE_CASES)
def test_the_chain_rule_kernel_agrees_with_float64_autograd_of_prepare_data(name):
    from icrl_amd import _lib, structs as S
    c = G.prepare_case(name)
    sp, n = c["spec"], c["n"]
    sel = _dev(np.asarray(sp["select_dim"], np.int32), torch.int32)
    f32 = lambda v: None if v is None else _dev(v)
    f64 = lambda v: None if v is None else _dev(v, torch.float64)
    low, high, mean, var = f32(sp["low"]), f32(sp["high"]), f64(sp["mean"]), f64(sp["var"])
    params = torch.zeros(8, device="cuda")
    s = S.CostNetT(sp["obs_dim"], sp["acs_dim"], len(sp["select_dim"]), 1, 4, 0, 0, 0, int(sp["is_discrete"]), 8, float(sp["clip_obs"]), _lib.ptr(sel), _lib.ptr(low),
                   _lib.ptr(high), _lib.ptr(mean), _lib.ptr(var), float(sp["eps"]), _lib.ptr(params), None)
    obs, acs, d_x = _dev(c["obs"], torch.float64), _dev(c["acs"]), _dev(c["d_x"])
    x = torch.empty(n, len(sp["select_dim"]), device="cuda")      # the forward it differentiates, against the restatement
    _lib.check(_lib.lib().icrl_cn_prepare(ctypes.byref(s), _lib.ptr(obs), _lib.ptr(acs), n, _lib.ptr(x), _lib.current_stream()), "icrl_cn_prepare")
    ref_x = G.prepare_torch(sp, torch.as_tensor(c["obs"]), torch.as_tensor(c["acs"]) if sp["is_discrete"] else torch.as_tensor(c["acs"]).double())
    assert np.array_equal(x.cpu().numpy(), ref_x.float().numpy())
    d_obs, d_acs = _prepare_bwd(s, obs, acs, d_x, n, sp["obs_dim"], sp["acs_dim"], not sp["is_discrete"])
    err = np.abs(d_obs[:n] - c["d_obs64"])
    print(f"MLP_GRAD IN prepare {name}: max |kernel - autograd| d_obs = {err.max():.3g}")
    assert np.all(err <= G.PREPARE_RTOL_OBS * np.abs(c["d_obs64"])) and np.all(d_obs[n:] == FILL)
    if not sp["is_discrete"]:
        assert np.all(np.abs(d_acs[:n].astype(np.float64) - c["d_acs64"]) <= G.PREPARE_RTOL_ACS * np.abs(c["d_acs64"])) and np.all(d_acs[n:] == FILL)
    ref_obs, ref_acs = G.prepare_bwd_numpy(sp, c["obs"], c["acs"], c["d_x"])      # the numpy statement has the kernel's own order: the same bits
    assert _same(d_obs[:n], ref_obs) and (sp["is_discrete"] or _same(d_acs[:n], ref_acs))


# ---- torch_ops ------------------------------------------------------------------------------------------------------------------------------------------
def _box(n, dtype):
    from icrl_amd import spaces
    return spaces.Box(-np.inf if dtype == np.float64 else -1, np.inf if dtype == np.float64 else 1, (n,), dtype)


def test_a_custom_policy_loss_fills_the_inputs_gradients_through_autograd():
    from icrl_amd import torch_ops as T
    from icrl_amd.policies import ActorTwoCriticsPolicy
    c = G.policy_loss_case()
    pol = ActorTwoCriticsPolicy(_box(c["obs_dim"], np.float64), _box(c["act_dim"], np.float32))
    pol.load_state_dict(c["sd"])
    w, t = _dev(c["w"]), _dev(c["t"])
    obs, act = _dev(c["obs"]).requires_grad_(True), _dev(c["actions"]).requires_grad_(True)
    mine = pol.params.detach().clone().requires_grad_(True)
    M.policy_loss(*T.evaluate_actions(pol, obs, act, params=mine, input_grads=True), w, t).backward()
    G.check("loss-policy", ["d_obs", "d_actions"], [obs.grad.cpu().numpy(), act.grad.cpu().numpy()], [c["d_obs64"], c["d_act64"]], G.DEV32["loss-policy"])
    assert obs.grad.dtype == torch.float32 and act.grad.dtype == torch.float32
    # the parameter leaf: the bits of the call without input gradients, whose inputs still get none
    plain = pol.params.detach().clone().requires_grad_(True)
    obs_p = _dev(c["obs"]).requires_grad_(True)
    M.policy_loss(*T.evaluate_actions(pol, obs_p, _dev(c["actions"]), params=plain), w, t).backward()
    assert torch.equal(mine.grad, plain.grad) and obs_p.grad is None
    # a second backward accumulates like any leaf (the same bits twice: exactly 2 x)
    g_obs, g_act, g_par = obs.grad.clone(), act.grad.clone(), mine.grad.clone()
    M.policy_loss(*T.evaluate_actions(pol, obs, act, params=mine, input_grads=True), w, t).backward()
    assert torch.equal(obs.grad, 2 * g_obs) and torch.equal(act.grad, 2 * g_act) and torch.equal(mine.grad, 2 * g_par)
    # only the tensors that ask for it: actions alone
    act2 = _dev(c["actions"]).requires_grad_(True)
    obs2 = _dev(c["obs"])
    M.policy_loss(*T.evaluate_actions(pol, obs2, act2, input_grads=True), w, t).backward()
    assert torch.equal(act2.grad, g_act) and obs2.grad is None


def test_a_custom_zeta_loss_fills_the_inputs_gradients_through_autograd():
    from icrl_amd import torch_ops as T
    c = G.zeta_loss_case()
    cn = _constraint_net(c)
    obs, acs = _dev(c["obs"], torch.float64).requires_grad_(True), _dev(c["acs"]).requires_grad_(True)
    mine = cn.params.detach().clone().requires_grad_(True)
    z = T.zeta(cn, obs, acs, params=mine, input_grads=True)
    M.zeta_loss(z).backward()
    assert obs.grad.dtype == torch.float64 and acs.grad.dtype == torch.float32
    G.check("loss-zeta", ["d_obs", "d_acs"], [obs.grad.cpu().numpy(), acs.grad.cpu().numpy()], [c["d_obs64"], c["d_acs64"]], G.DEV32["loss-zeta"])
    plain = cn.params.detach().clone().requires_grad_(True)
    z_p = T.zeta(cn, c["obs"], c["acs"], params=plain)
    assert torch.equal(z_p, z)
    M.zeta_loss(z_p).backward()
    assert torch.equal(mine.grad, plain.grad)
    g_obs, g_par = obs.grad.clone(), mine.grad.clone()
    M.zeta_loss(T.zeta(cn, obs, acs, params=mine, input_grads=True)).backward()
    assert torch.equal(obs.grad, 2 * g_obs) and torch.equal(mine.grad, 2 * g_par)


def test_unserved_shapes_and_row_counts_raise_with_the_librarys_reason():
    from icrl_amd import torch_ops as T
    from icrl_amd.constraint_net import ConstraintNet
    cn = ConstraintNet(18, 6, [96, 96], None, lambda x: 0.05, None, None, False, 0.5)
    with pytest.raises(NotImplementedError, match=r"hidden layers \(96, 96\) are not served \(1\.\.2 of up to 64 units\)"):
        T.zeta(cn, np.zeros((4, 18)), np.zeros((4, 6), np.float32), input_grads=True)
    with pytest.raises(NotImplementedError, match=r"hidden layers \(96, 96\) are not served"):
        cn.input_gradients(np.zeros((4, 18)), np.zeros((4, 6), np.float32))
    ok = ConstraintNet(18, 6, [20], None, lambda x: 0.05, None, None, False, 0.5)
    with pytest.raises(NotImplementedError, match=r"N = 65537 rows \(1\.\.65536\)"):
        T.zeta(ok, np.zeros((65537, 18)), np.zeros((65537, 6), np.float32), input_grads=True)


# ---- saliency -------------------------------------------------------------------------------------------------------------------------------------------
def test_saliency_is_exactly_zero_for_inputs_whose_first_layer_columns_are_zero():
    """18 observations and the 6 real action columns (acs_select_dim 18..23 of the concatenated vector); the first-layer columns of observation 7
    and action 2 are zeroed.  input_gradients walks chunks of at most INPUT_GRAD_ROWS rows: with the chunk at 128 rows, 300 rows take three."""
    from icrl_amd.constraint_net import ConstraintNet
    torch.manual_seed(3)
    lo = -np.ones(6, np.float32)
    cn = ConstraintNet(18, 6, [64, 64], None, lambda x: 0.05, None, None, False, 0.5, None, list(range(18, 24)), clip_obs=10.0, action_low=lo, action_high=-lo)
    sd = cn.state_dict()
    sd["0.weight"][:, 7] = 0.0
    sd["0.weight"][:, 18 + 2] = 0.0
    cn.load_state_dict(sd)
    rng = np.random.RandomState(5)
    obs, acs = rng.randn(300, 18), (0.4 * rng.randn(300, 6)).astype(np.float32)
    sal = cn.saliency(obs, acs)
    assert sal["obs"].dtype == np.float64 and sal["obs"].shape == (18,) and sal["acs"].dtype == np.float64 and sal["acs"].shape == (6,)
    print("MLP_GRAD IN saliency obs", sal["obs"], "acs", sal["acs"])
    assert sal["obs"][7] == 0.0 and sal["acs"][2] == 0.0
    assert np.all(np.delete(sal["obs"], 7) > 0) and np.all(np.delete(sal["acs"], 2) > 0)
    d_obs, d_acs = cn.input_gradients(obs, acs)
    assert d_obs.shape == (300, 18) and d_obs.dtype == torch.float64 and d_acs.shape == (300, 6) and d_acs.dtype == torch.float32
    cn.INPUT_GRAD_ROWS = 128
    d_obs2, d_acs2 = cn.input_gradients(obs, acs)
    assert torch.equal(d_obs, d_obs2) and torch.equal(d_acs, d_acs2)
    # cost = 1 - zeta: the negative of torch_ops' d zeta / d input
    from icrl_amd import torch_ops as T
    o = _dev(obs, torch.float64).requires_grad_(True)
    T.zeta(cn, o, acs, input_grads=True).sum().backward()
    assert torch.equal(o.grad, -d_obs)


# ---- icrl --cn_saliency ---------------------------------------------------------------------------------------------------------------------------------
def _run(extra):
    from icrl_amd.icrl import build_parser, icrl
    here = os.path.dirname(os.path.abspath(__file__))
    argv = ["icrl", "-tei", "HCWithPos-v0", "-eei", "HCWithPosTest-v0", "-ep", os.path.join(here, "golden/expert_hc.npz"), "-nt", "4", "-ns", "64", "-ft", "256",
            "-er", "2", "-bi", "2", "-ni", "2", "-cl", "20", "-s", "0", "-v", "0", *extra]
    cfg = vars(build_parser().parse_args(argv))
    cfg.update(rank=0, world_size=1)
    return icrl(types.SimpleNamespace(**cfg), log=None)[0]


def test_the_flag_logs_every_input_column_and_changes_nothing_else():
    with_flag, without = _run(["--cn_saliency"]), _run([])
    assert len(with_flag) == len(without) == 2
    keys = [f"backward/saliency_obs_{i}" for i in range(18)] + [f"backward/saliency_acs_{j}" for j in range(6)]
    for m_on, m_off in zip(with_flag, without):
        for k in keys:
            assert k in m_on and np.isfinite(m_on[k]) and m_on[k] >= 0.0, k
        assert not any("saliency" in k for k in m_off)
        assert any(m_on[k] > 0 for k in keys[:18])
        clock = [k for k in m_on if k == "time(m)" or k.startswith("time/")]      # wall-clock readings (minutes, fps, seconds): not computed
        rest = [k for k in m_on if k not in keys and k not in clock]
        assert sorted(rest + clock) == sorted(m_off) and len(rest) >= 20
        for k in rest:      # the flag draws no random number and changes no state: every other metric has the same bits
            a, b = np.float64(m_on[k]), np.float64(m_off[k])
            assert a.tobytes() == b.tobytes() or (np.isnan(a) and np.isnan(b)), (k, a, b)
