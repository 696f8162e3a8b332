"""GPU: icrl_policy_fwd_bwd / icrl_cost_mlp_fwd_bwd (csrc/mlp_grad.hip) through the C ABI and icrl_amd/torch_ops.py on top of them.

Gradients are compared with float64 CPU autograd of the oracle's networks under the rule of tests/helpers/mlp_grad_cases.py
(|kernel - float64| <= 4 dev32 per parameter tensor, dev32 stored there); outputs under the project's fp32-MLP tolerance.  Every case prints
its figures (`MLP_GRAD ...`) before it asserts."""
import ctypes
from collections import OrderedDict

import numpy as np
import pytest
import torch

from helpers import mlp_grad_cases as M

pytestmark = pytest.mark.gpu
OUTS = ("v_r", "v_c", "log_prob", "entropy")


def _dev(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).cuda().contiguous()


def _policy_call(flat, obs_dim, act_dim, discrete, obs, actions, ups=None, grad=True, fill=7.0):
    """one icrl_policy_fwd_bwd call on device tensors -> (outputs dict of numpy, grad numpy or None).  ups: dict name -> device tensor or None."""
    from icrl_amd import _lib, structs as S
    L = _lib.lib()
    n = obs.shape[0]
    pol = S.PolicyT(obs_dim, act_dim, M.HW, M.HW, int(discrete), flat.numel(), _lib.ptr(flat), None, None)
    outs = {k: torch.full((n,), fill, device="cuda") for k in OUTS}
    g = ws = None
    nbytes = 0
    if grad:
        nbytes = L.icrl_policy_fwd_bwd_ws_bytes(ctypes.byref(pol), n)
        assert nbytes > 0, L.icrl_last_error()
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
        g = torch.full((flat.numel(),), fill, device="cuda")      # pre-filled: the call overwrites, it does not accumulate
    ups = ups or {}
    _lib.check(L.icrl_policy_fwd_bwd(ctypes.byref(pol), _lib.ptr(obs), _lib.ptr(actions), n, *[_lib.ptr(ups.get(k)) for k in OUTS],
                                     *[_lib.ptr(outs[k]) for k in OUTS], _lib.ptr(g), _lib.ptr(ws), nbytes, _lib.current_stream()), "icrl_policy_fwd_bwd")
    return {k: v.cpu().numpy() for k, v in outs.items()}, (g.cpu().numpy() if grad else None)


def _policy_case_on_device(c):
    return _dev(c["flat"]), _dev(c["obs"]), _dev(c["actions"]), {k: _dev(v) for k, v in c["ups"].items()}


# ---- 1. the reference's own steps with no torch network -------------------------------------------------------------------------------------------
def test_three_reference_steps_without_a_torch_network(golden):
    """ppo_lag.py:216-288 on tests/golden/g4 (the reference's policy / optimizer objects stepped 3 x on one batch): icrl_policy_fwd_bwd forward,
    icrl_ppo_lag_loss_fwd_bwd, icrl_policy_fwd_bwd backward, icrl_clip_adam_step — at the tolerances
    test_loss_fwd_bwd_and_clip_adam_reproduce_the_reference_steps applies to the same quantities.  A gradient tensor that misses that test's
    atol 2e-7 is decided by the 4 dev32 rule against float64 autograd of the oracle at the same parameters and upstream gradients (dev32
    measured here, float32 against float64 CPU autograd); the test prints which tensors took that route."""
    from icrl_amd import _lib, structs as S
    L = _lib.lib()
    g = golden("g4_ppo_minibatch")
    B = int(g["obs"].shape[0])
    shape = (18, 6, False, (64, 64))
    names = list(M.oracle_policy(shape).params)
    sd = OrderedDict((k, torch.as_tensor(g["w0/" + k])) for k in names)
    shapes = OrderedDict((k, tuple(v.shape)) for k, v in sd.items())
    flat = _dev(M.pack_policy(sd, 18))
    n = flat.numel()
    m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    work, out2, terms = torch.zeros(256, device="cuda"), torch.zeros(2, device="cuda"), torch.zeros(8, device="cuda")
    hp = S.PpoHyperT(B, 1, 0, 0)
    hp.clip_range, hp.ent_coef, hp.reward_vf_coef, hp.cost_vf_coef, hp.max_grad_norm = float(g["clip"]), 0.0, 0.5, 0.5, 0.5
    hp.clip_range_reward_vf = hp.clip_range_cost_vf = -1.0
    hp.lr, hp.adam_beta1, hp.adam_beta2, hp.adam_eps = float(g["lr"]), 0.9, 0.999, 1e-5
    nu = _dev(np.float32([float(g["nu"])]))
    dev = {k: _dev(g[k]) for k in ("old_lp", "adv_r", "adv_c", "ret_r", "ret_c")}
    obs, act = _dev(g["obs"]), _dev(g["act"])
    pol = S.PolicyT(18, 6, 64, 64, 0, n, _lib.ptr(flat), None, None)
    nbytes = L.icrl_policy_fwd_bwd_ws_bytes(ctypes.byref(pol), B)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
    o = {k: torch.empty(B, device="cuda") for k in OUTS}
    d = {k: torch.empty(B, device="cuda") for k in OUTS}
    grad = torch.empty(n, device="cuda")
    st = _lib.current_stream()
    by_rule = []
    for s in range(3):
        _lib.check(L.icrl_policy_fwd_bwd(ctypes.byref(pol), _lib.ptr(obs), _lib.ptr(act), B, None, None, None, None, *[_lib.ptr(o[k]) for k in OUTS],
                                         None, None, 0, st), "icrl_policy_fwd_bwd")
        _lib.check(L.icrl_ppo_lag_loss_fwd_bwd(_lib.ptr(o["log_prob"]), _lib.ptr(dev["old_lp"]), _lib.ptr(dev["adv_r"]), _lib.ptr(dev["adv_c"]), _lib.ptr(o["v_r"]),
                                               _lib.ptr(o["v_c"]), _lib.ptr(dev["ret_r"]), _lib.ptr(dev["ret_c"]), None, None, _lib.ptr(o["entropy"]), _lib.ptr(nu),
                                               ctypes.byref(hp), B, _lib.ptr(terms), _lib.ptr(d["log_prob"]), _lib.ptr(d["v_r"]), _lib.ptr(d["v_c"]),
                                               _lib.ptr(d["entropy"]), st), "icrl_ppo_lag_loss_fwd_bwd")
        t = terms.cpu().numpy()
        for i, key in enumerate(("loss", "policy_loss", "rvl", "cvl", "entropy_loss", "approx_kl", "clip_fraction")):
            ref = float(g[f"s{s}/{key}"])
            print(f"MLP_GRAD g4 step {s} {key}: {t[i]:.9g} vs {ref:.9g}")
            assert abs(t[i] - ref) <= 2e-6 + 2e-5 * abs(ref), (s, key, t[i], ref)
        grad.fill_(7.0)
        _lib.check(L.icrl_policy_fwd_bwd(ctypes.byref(pol), _lib.ptr(obs), _lib.ptr(act), B, *[_lib.ptr(d[k]) for k in OUTS], None, None, None, None,
                                         _lib.ptr(grad), _lib.ptr(ws), nbytes, st), "icrl_policy_fwd_bwd")
        got = M.unpack_flat(grad.cpu().numpy(), shapes)
        missed = []
        for k in names:
            ref = g[f"s{s}/grad/{k}"]
            err = np.abs(got[k] - ref).max()
            print(f"MLP_GRAD g4 step {s} grad {k}: max |kernel - reference| = {err:.3g}")
            if not np.allclose(got[k], ref, rtol=2e-4, atol=2e-7):
                missed.append(k)
        if missed:      # summation order, or wrong?  float64 autograd of the oracle at these parameters and upstream gradients decides
            cur = M.unpack_flat(flat.cpu().numpy(), shapes)
            ups = {k: d[k].cpu().numpy() for k in OUTS}
            _, g64 = M.policy_grads(M.oracle_policy(shape, cur, torch.float64), g["obs"], g["act"], ups, torch.float64)
            _, g32 = M.policy_grads(M.oracle_policy(shape, cur, torch.float32), g["obs"], g["act"], ups, torch.float32)
            sub = OrderedDict((k, g64[k]) for k in missed)
            M.check_grads(f"g4 step {s} (by the dev32 rule)", got, sub, [float(np.abs(g32[k] - g64[k]).max()) for k in missed])
            by_rule += [(s, k) for k in missed]
        _lib.check(L.icrl_clip_adam_step(_lib.ptr(flat), _lib.ptr(grad), _lib.ptr(m), _lib.ptr(v), _lib.ptr(step), n, ctypes.byref(hp), _lib.ptr(work),
                                         _lib.ptr(out2), st), "icrl_clip_adam_step")
        assert abs(out2[0].item() - float(g[f"s{s}/grad_norm"])) <= 1e-5 * max(1.0, float(g[f"s{s}/grad_norm"]))
        new = M.unpack_flat(flat.cpu().numpy(), shapes)
        for k in names:
            ref = g[f"s{s}/after/{k}"]
            assert np.allclose(new[k], ref, rtol=1e-5, atol=3e-7), (s, k, np.abs(new[k] - ref).max())
    print(f"MLP_GRAD g4: tensors decided by the dev32 rule: {by_rule}")
    assert int(step.item()) == 3


# ---- 2. policy gradients against float64 autograd -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,n", M.POLICY_CASES, ids=[M.case_id(s, n) for s, n in M.POLICY_CASES])
def test_policy_outputs_and_gradients_vs_float64_autograd(shape, n):
    """random upstream gradients in all four outputs, a trained-like state; grad pre-filled with 7.0 (overwritten, not accumulated); the padding
    entries of the 64-wide layout exactly 0.0 (g13: logical widths 32-48 / 64-32 / 16-64); the forward-only call gives the same output bits."""
    c = M.policy_case(shape, n)
    flat, obs, act, ups = _policy_case_on_device(c)
    outs, g = _policy_call(flat, c["obs_dim"], c["act_dim"], c["discrete"], obs, act, ups)
    tag = M.case_id(shape, n)
    M.check_outputs(tag, outs, c["out64"])
    parts, pads = M.unpack_policy(g, c["logical_shapes"], c["obs_dim"])
    for k, pad in pads.items():
        assert pad.size == 0 or not pad.any(), (k, "padding entries of grad must be exactly 0.0")
    if shape == "g13":
        assert sum(p.size for p in pads.values()) > 3000      # the case is about them
    M.check_grads(tag, parts, c["g64"], M.DEV32[tag])
    fwd, none = _policy_call(flat, c["obs_dim"], c["act_dim"], c["discrete"], obs, act, None, grad=False, fill=-3.0)
    assert none is None
    for k in OUTS:
        assert np.array_equal(fwd[k].view(np.uint32), outs[k].view(np.uint32)), k


@pytest.mark.parametrize("shape", ["hc", "lgw"])
def test_a_null_upstream_pointer_is_a_vector_of_zeros(shape):
    c = M.policy_case(shape, 100)
    flat, obs, act, ups = _policy_case_on_device(c)
    zeros = torch.zeros(100, device="cuda")
    for k in OUTS + ("all",):
        null = {q: (None if q == k or k == "all" else ups[q]) for q in OUTS}
        explicit = {q: (zeros if q == k or k == "all" else ups[q]) for q in OUTS}
        _, g_null = _policy_call(flat, c["obs_dim"], c["act_dim"], c["discrete"], obs, act, null)
        _, g_zero = _policy_call(flat, c["obs_dim"], c["act_dim"], c["discrete"], obs, act, explicit)
        assert np.array_equal(g_null.view(np.uint32), g_zero.view(np.uint32)), k
        if k == "all":
            assert not g_null.any()
        else:
            assert g_null.any()


# ---- 3. determinism -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [257, 4096])
def test_the_same_call_twice_gives_the_same_bits(n):
    """N = 4096: 256 row tiles over the 64 workgroups of a network, four tiles each, 64 partial sums folded in index order."""
    rng = np.random.RandomState(n)
    c = M.policy_case("ant", 257)
    flat = _dev(c["flat"])
    obs, act = _dev(rng.randn(n, 113).astype(np.float32)), _dev(rng.randn(n, 8).astype(np.float32))
    ups = {k: _dev(rng.randn(n).astype(np.float32)) for k in OUTS}
    o1, g1 = _policy_call(flat, 113, 8, False, obs, act, ups)
    o2, g2 = _policy_call(flat, 113, 8, False, obs, act, ups, fill=-1.0)
    assert np.isfinite(g1).all() and np.abs(g1).max() > 0
    assert np.array_equal(g1.view(np.uint32), g2.view(np.uint32))
    for k in OUTS:
        assert np.array_equal(o1[k].view(np.uint32), o2[k].view(np.uint32)), k


# ---- 4. cost-net gradients against float64 autograd ----------------------------------------------------------------------------------------------
def _cost_call(c, flat, x, up, grad=True, fill=7.0):
    from icrl_amd import _lib, structs as S
    L = _lib.lib()
    n, hs = x.shape[0], list(c["hidden"])
    h = hs + [0] * (4 - len(hs))
    cn = S.CostNetT(c["obs_dim"], c["acs_dim"], c["in_dim"], len(hs), h[0], h[1], h[2], h[3], 0, flat.numel(), 10.0, None, None, None, None, None, 1e-5,
                    _lib.ptr(flat), None)
    zeta = torch.full((n,), fill, device="cuda")
    g = ws = None
    nbytes = 0
    if grad:
        nbytes = L.icrl_cost_mlp_fwd_bwd_ws_bytes(ctypes.byref(cn), n)
        assert nbytes > 0, L.icrl_last_error()
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
        g = torch.full((flat.numel(),), fill, device="cuda")
    _lib.check(L.icrl_cost_mlp_fwd_bwd(ctypes.byref(cn), _lib.ptr(x), n, _lib.ptr(up) if grad else None, _lib.ptr(zeta), _lib.ptr(g), _lib.ptr(ws), nbytes,
                                       _lib.current_stream()), "icrl_cost_mlp_fwd_bwd")
    return zeta.cpu().numpy(), (g.cpu().numpy() if grad else None)


@pytest.mark.parametrize("shape,n", M.COST_CASES, ids=[M.case_id(s, n) for s, n in M.COST_CASES])
def test_cost_net_outputs_and_gradients_vs_float64_autograd(shape, n):
    c = M.cost_case(shape, n)
    assert c["zmin"] >= M.RELU_MARGIN, c["zmin"]      # no hidden unit of the float64 oracle near its kink: float32 takes the same side
    flat, x, up = _dev(c["flat"]), _dev(c["x"]), _dev(c["up"])
    zeta, g = _cost_call(c, flat, x, up)
    tag = "cost-" + M.case_id(shape, n)
    M.check_outputs(tag, dict(zeta=zeta), dict(zeta=c["zeta64"]))
    M.check_grads(tag, M.unpack_flat(g, c["shapes"]), c["g64"], M.DEV32[tag])
    fwd, none = _cost_call(c, flat, x, up, grad=False, fill=-3.0)
    assert none is None and np.array_equal(fwd.view(np.uint32), zeta.view(np.uint32))


# ---- 5. the autograd functions -------------------------------------------------------------------------------------------------------------------------
def _box(n, dtype):
    from icrl_amd import spaces
    return spaces.Box(-np.inf if dtype == np.float64 else -1, np.inf if dtype == np.float64 else 1, (n,), dtype)


def _hc_policy(c):
    from icrl_amd.policies import ActorTwoCriticsPolicy
    pol = ActorTwoCriticsPolicy(_box(c["obs_dim"], np.float64), _box(c["act_dim"], np.float32))
    pol.load_state_dict(c["sd"])
    return pol


def test_a_custom_policy_loss_trains_the_flat_buffer_through_autograd():
    from icrl_amd import torch_ops as T
    c = M.policy_loss_case()
    pol = _hc_policy(c)
    w, t = _dev(c["w"]), _dev(c["t"])
    obs, act = _dev(c["obs"]), _dev(c["actions"])
    leaf = T.leaf(pol)
    assert leaf.is_leaf and leaf.requires_grad and leaf.data_ptr() == pol.params.data_ptr() and not pol.params.requires_grad and leaf.grad is None
    loss = M.policy_loss(*T.evaluate_actions(pol, obs, act), w, t)
    loss.backward()
    g1 = leaf.grad.clone()
    parts, pads = M.unpack_policy(g1.cpu().numpy(), c["logical_shapes"], c["obs_dim"])
    M.check_grads("loss-policy", parts, c["g64"], M.DEV32["loss-policy"])
    # a second backward accumulates like any leaf (the same bits twice: exactly 2 x)
    M.policy_loss(*T.evaluate_actions(pol, obs, act), w, t).backward()
    assert torch.equal(leaf.grad, 2 * g1)
    # an explicit leaf in the same layout gets the same gradient; the inputs get none
    mine = pol.params.detach().clone().requires_grad_(True)
    obs_g = obs.clone().requires_grad_(True)
    M.policy_loss(*T.evaluate_actions(pol, obs_g, act, params=mine), w, t).backward()
    assert torch.equal(mine.grad, g1) and obs_g.grad is None
    assert set(pol._torch_ops_ws) == {("policy", c["n"])}      # one workspace per (object, N)


def test_a_custom_zeta_loss_trains_the_flat_buffer_through_autograd():
    from icrl_amd import torch_ops as T
    from icrl_amd.constraint_net import ConstraintNet
    c = M.zeta_loss_case()
    lo = -np.ones(c["acs_dim"], np.float32)
    cn = ConstraintNet(c["obs_dim"], c["acs_dim"], list(c["hidden"]), None, lambda x: 0.05, None, None, False, 0.5, clip_obs=10.0, action_low=lo, action_high=-lo)
    cn.load_state_dict(c["sd"])
    z = T.zeta(cn, c["obs"], c["acs"])
    M.check_outputs("loss-zeta", dict(zeta=z.detach().cpu().numpy()), dict(zeta=c["zeta64"]))
    assert np.allclose(1.0 - z.detach().cpu().numpy(), cn.cost_function(c["obs"], c["acs"]), rtol=1e-5, atol=2e-6)
    M.zeta_loss(z).backward()
    g1 = T.leaf(cn).grad.clone()
    M.check_grads("loss-zeta", M.unpack_flat(g1.cpu().numpy(), c["shapes"]), c["g64"], M.DEV32["loss-zeta"])
    M.zeta_loss(T.zeta(cn, c["obs"], c["acs"])).backward()
    assert torch.equal(T.leaf(cn).grad, 2 * g1)


def test_unserved_shapes_raise_with_the_librarys_reason():
    from icrl_amd import torch_ops as T
    from icrl_amd.constraint_net import ConstraintNet
    from icrl_amd.policies import ActorTwoCriticsPolicy
    wide = ActorTwoCriticsPolicy(_box(18, np.float64), _box(6, np.float32), net_arch=[dict(pi=[128, 128], vf=[128, 128], cvf=[128, 128])])
    with pytest.raises(NotImplementedError, match=r"hidden widths \(128, 128\).*h1 == h2 <= 64"):
        T.evaluate_actions(wide, torch.zeros(4, 18), torch.zeros(4, 6))
    trunk = ActorTwoCriticsPolicy(_box(18, np.float64), _box(6, np.float32), net_arch=[32, dict(pi=[32], vf=[32], cvf=[32])])
    with pytest.raises(NotImplementedError, match=r"`arch` array is not served"):
        T.evaluate_actions(trunk, torch.zeros(4, 18), torch.zeros(4, 6))
    cn = ConstraintNet(18, 6, [96, 96], None, lambda x: 0.05, None, None, False, 0.5)
    with pytest.raises(NotImplementedError, match=r"hidden layers \(96, 96\) are not served \(1\.\.2 of up to 64 units\)"):
        T.zeta(cn, np.zeros((4, 18)), np.zeros((4, 6), np.float32))


# ---- 6. nothing else moved -----------------------------------------------------------------------------------------------------------------------------
def test_the_existing_evaluate_actions_and_the_route_records_are_untouched():
    """ActorTwoCriticsPolicy.evaluate_actions (icrl_policy_evaluate: params_t, the fast tanh) and torch_ops.evaluate_actions are two kernels:
    the same rows agree within the output tolerance; the new calls write no route record."""
    from icrl_amd import _lib, torch_ops as T
    c = M.policy_case("hc", 100)
    pol = _hc_policy(c)
    before = [_lib.last_route(f) for f in (_lib.FAMILY_ROLLOUT, _lib.FAMILY_UPDATE, _lib.FAMILY_GAE)]
    params0 = pol.params.clone()
    new = T.evaluate_actions(pol, _dev(c["obs"]), _dev(c["actions"]))
    sum(o.sum() for o in new).backward()
    cc = M.cost_case("h20", 64)
    _cost_call(cc, _dev(cc["flat"]), _dev(cc["x"]), _dev(cc["up"]))
    assert [_lib.last_route(f) for f in (_lib.FAMILY_ROLLOUT, _lib.FAMILY_UPDATE, _lib.FAMILY_GAE)] == before
    assert torch.equal(pol.params, params0)
    old = pol.evaluate_actions(torch.as_tensor(c["obs"], dtype=torch.float64), c["actions"])
    for k, a, b in zip(OUTS, old, new):
        a, b = a.flatten().cpu().numpy().astype(np.float64), b.detach().cpu().numpy().astype(np.float64)
        rtol, atol = M.OUT_TOL[k]
        print(f"MLP_GRAD old-vs-new {k}: max |icrl_policy_evaluate - icrl_policy_fwd_bwd| = {np.abs(a - b).max():.3g}")
        assert np.all(np.abs(a - b) <= atol + rtol * np.abs(b)), (k, np.abs(a - b).max())
