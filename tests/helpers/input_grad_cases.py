"""Cases and float64 references of the INPUT gradients of the fused network forward + backward (csrc/mlp_grad.hip: icrl_policy_fwd_bwd_in,
icrl_cost_mlp_fwd_bwd_in, icrl_cn_prepare_bwd; icrl_amd/torch_ops.py input_grads=True).  Everything here runs on the CPU.

The networks are the oracle's, as tests/helpers/mlp_grad_cases.py builds them (oracle_policy at a trained state, oracle_costnet); the
reference of an input gradient is FLOAT64 autograd of those networks with the inputs as leaves, and the bound is that file's rule, per
input-gradient tensor and max-abs:
    |kernel - float64| <= GRAD_UNITS (4) * dev32,    dev32 = max |float32 CPU autograd - float64 CPU autograd| of the same case
dev32 is a property of the case, measured on the reference networks, never on the kernel; it is stored in DEV32 below, written by
    python tests/helpers/input_grad_cases.py          (prints the tables; torch 2.10 CPU, default threads)

Margins (asserted when a case is built, before any kernel runs):
  * every ReLU pre-activation of the float64 net has |z| >= RELU_MARGIN (the seed of a constraint-net case is picked here: COST_SEED);
  * no clipped operand lies within CLIP_MARGIN of a clip bound, and every constraint-net case has an operand strictly beyond each bound of
    each clip it reads, so the zero branch of the clip's derivative is exercised;
  * no Gaussian row has action == mean.
"""
import functools
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for _p in (_ROOT, os.path.join(_ROOT, "tests")):      # (run as a script: `oracle` and `helpers` are found from the repository root / tests)
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import nets as o_nets      # noqa: E402
from helpers import mlp_grad_cases as M      # noqa: E402

OUTS = ("v_r", "v_c", "log_prob", "entropy")
GRAD_UNITS, RELU_MARGIN, CLIP_MARGIN = M.GRAD_UNITS, M.RELU_MARGIN, 1e-6
# (obs, act) of the issue, by their names in mlp_grad_cases.POLICY_SHAPES; "lgw": discrete, 1 observation, 2 classes; "g13": logical widths
# 32-48 / 64-32 / 16-64 stored zero-padded to 64
POLICY_SHAPES = ("o1a1", "o17a5", "o33a1", "o65a1", "o128a16", "lgw", "g13")
POLICY_ROWS = (1, 16, 17, 257, 1025)      # the tile edge, a ragged tile, several workgroups, 65 tiles on 64 workgroups: a second trip of the walk
POLICY_CASES = [(s, n) for s in POLICY_SHAPES for n in POLICY_ROWS]
# "h20": one hidden layer (sdz1 = sdz); "point": -cosd 0 1 -casd -1 (in_dim 2); "disc": one-hot actions
COST_SHAPES = ("h20", "h64", "ant", "point", "disc")
COST_ROWS = (1, 63, 65, 1025)
COST_CASES = [(s, n) for s in COST_SHAPES for n in COST_ROWS]
DISC_SHAPE = (6, 4, (32, 24))             # obs_dim, classes, hidden of the discrete net
CLIP_OBS, ACT_BOUND = 10.0, 1.0


def case_id(shape, n):
    return f"{shape}-{n}"


# ---- policy -----------------------------------------------------------------------------------------------------------------------------------------
def _policy_input_grads(c, dtype, ups=None):
    """autograd of sum_n (d_v_r v_r + d_v_c v_c + d_lp log_prob + d_ent entropy) over obs and (Box) actions -> d_obs, d_actions | None, min |a - mean|"""
    ups = c["ups"] if ups is None else ups
    pol = M.oracle_policy(c["shape"], c["sd"], dtype)
    obs = torch.as_tensor(c["obs"]).to(dtype).requires_grad_(True)
    act = torch.as_tensor(c["actions"]).to(dtype)
    if not c["discrete"]:
        act.requires_grad_(True)
    v_r, v_c, lp, ent = pol.evaluate_actions(obs, act)
    outs = dict(v_r=v_r.flatten(), v_c=v_c.flatten(), log_prob=lp, entropy=ent)
    torch.autograd.backward([outs[k] for k in OUTS], [torch.as_tensor(ups[k]).to(dtype) for k in OUTS])
    diff = np.inf if c["discrete"] else float((act.detach() - pol.heads(obs.detach())[0].detach()).abs().min())
    return obs.grad.double().numpy(), (None if c["discrete"] else act.grad.double().numpy()), diff


@functools.lru_cache(maxsize=None)
def policy_case(shape, n):
    """mlp_grad_cases.policy_case (inputs, upstream gradients, the trained state) plus the float64 input gradients: d_obs, d_actions (None
    when discrete) with all four upstream gradients at once, and d_obs_sum = (pi + vf) + cvf of three float64 runs with one branch's upstream
    gradients each (log_prob and entropy: pi; v_r: vf; v_c: cvf)."""
    c = dict(M.policy_case(shape, n))
    d_obs, d_act, diff = _policy_input_grads(c, torch.float64)
    assert diff > 0.0, (shape, n, "a Gaussian row with action == mean")
    zero = np.zeros(n, np.float32)
    branch = []
    for keep in (("log_prob", "entropy"), ("v_r",), ("v_c",)):
        branch.append(_policy_input_grads(c, torch.float64, {k: (c["ups"][k] if k in keep else zero) for k in OUTS})[0])
    c.update(d_obs64=d_obs, d_act64=d_act, d_obs_sum64=(branch[0] + branch[1]) + branch[2])
    return c


def policy_dev32(shape, n):
    c = policy_case(shape, n)
    d_obs, d_act, _ = _policy_input_grads(c, torch.float32)
    return [float(np.abs(d_obs - c["d_obs64"]).max())] + ([] if d_act is None else [float(np.abs(d_act - c["d_act64"]).max())])


# ---- prepare_data and its chain rule, restated ---------------------------------------------------------------------------------------------------
def prep_spec(obs_dim, acs_dim, select_dim, is_discrete=False, clip_obs=CLIP_OBS, low=None, high=None, mean=None, var=None, eps=1e-5):
    f = lambda v, t: None if v is None else np.asarray(v, t)
    return dict(obs_dim=obs_dim, acs_dim=acs_dim, select_dim=[int(i) for i in select_dim], is_discrete=bool(is_discrete), clip_obs=clip_obs,
                low=f(low, np.float32), high=f(high, np.float32), mean=f(mean, np.float64), var=f(var, np.float64), eps=eps)


def spec_of(net):
    """the spec of an oracle CostNet"""
    return prep_spec(net.obs_dim, net.acs_dim, net.select_dim, net.is_discrete, net.clip_obs, net.action_low, net.action_high, net.obs_mean, net.obs_var, net.eps)


def prepare_torch(spec, obs, acs):
    """prepare_data (icrl/constraint_net.py:258-299) in differentiable torch, float64 throughout: obs [N, obs_dim] float64, acs [N, acs_dim]
    float64 (or class indices [N, 1] when discrete) -> x [N, in_dim] float64."""
    if spec["mean"] is not None and spec["var"] is not None:
        obs = (obs - torch.as_tensor(spec["mean"])) / torch.sqrt(torch.as_tensor(spec["var"]) + spec["eps"])
    if spec["clip_obs"] is not None:
        obs = torch.clamp(obs, -spec["clip_obs"], spec["clip_obs"])
    if spec["is_discrete"]:
        acs = torch.nn.functional.one_hot(acs.long().flatten(), spec["acs_dim"]).double()
    if spec["low"] is not None and spec["high"] is not None:
        acs = torch.clamp(acs, torch.as_tensor(spec["low"]).double(), torch.as_tensor(spec["high"]).double())
    return torch.cat([obs, acs], dim=-1)[:, spec["select_dim"]]


def prepare_bwd_autograd(spec, obs, acs, d_x):
    """float64 autograd of prepare_torch for the upstream d_x [N, in_dim] -> d_obs float64, d_acs float32 | None"""
    o = torch.as_tensor(np.asarray(obs, np.float64)).requires_grad_(True)
    a = torch.as_tensor(np.asarray(acs, np.float32))
    if not spec["is_discrete"]:
        a.requires_grad_(True)
    x = prepare_torch(spec, o, a if spec["is_discrete"] else a.double())
    x.backward(torch.as_tensor(np.asarray(d_x, np.float32)).double())
    return o.grad.numpy(), (None if spec["is_discrete"] else a.grad.numpy())


def prepare_bwd_numpy(spec, obs, acs, d_x):
    """icrl_cn_prepare_bwd stated in numpy: per source column the d_x of the selected positions that read it, added in ascending position in
    float64; then the clip's derivative (closed interval); then 1 / sqrt(var + eps) where the net normalises."""
    obs, d_x = np.asarray(obs, np.float64), np.asarray(d_x, np.float32)
    n, od, ad = obs.shape[0], spec["obs_dim"], spec["acs_dim"]
    acc = np.zeros((n, od + ad), np.float64)
    for i, s in enumerate(spec["select_dim"]):
        acc[:, s] += d_x[:, i].astype(np.float64)
    o, scale = obs, np.ones(od)
    if spec["mean"] is not None and spec["var"] is not None:
        sd = np.sqrt(spec["var"] + spec["eps"])
        o, scale = (obs - spec["mean"]) / sd, 1.0 / sd
    d_obs = acc[:, :od]
    if spec["clip_obs"] is not None:
        d_obs = np.where((o >= -spec["clip_obs"]) & (o <= spec["clip_obs"]), d_obs, 0.0)
    d_obs = d_obs * scale
    if spec["is_discrete"]:
        return d_obs, None
    d_acs = acc[:, od:]
    if spec["low"] is not None and spec["high"] is not None:
        a = np.asarray(acs, np.float32)
        d_acs = np.where((a >= spec["low"]) & (a <= spec["high"]), d_acs, 0.0)
    return d_obs, d_acs.astype(np.float32)


def clip_margins(spec, obs, acs):
    """(distance of the nearest clipped operand to a clip bound, [operands beyond -clip_obs, +clip_obs, low, high])"""
    o = np.asarray(obs, np.float64)
    if spec["mean"] is not None and spec["var"] is not None:
        o = (o - spec["mean"]) / np.sqrt(spec["var"] + spec["eps"])
    dist, beyond = np.inf, [0, 0, 0, 0]
    if spec["clip_obs"] is not None:
        dist = min(dist, float(np.abs(np.abs(o) - spec["clip_obs"]).min()))
        beyond[0], beyond[1] = int((o < -spec["clip_obs"]).sum()), int((o > spec["clip_obs"]).sum())
    if not spec["is_discrete"] and spec["low"] is not None and spec["high"] is not None:
        a = np.asarray(acs, np.float64)
        dist = min(dist, float(np.abs(a - spec["low"]).min()), float(np.abs(a - spec["high"]).min()))
        beyond[2], beyond[3] = int((a < spec["low"]).sum()), int((a > spec["high"]).sum())
    return dist, beyond


# the cases of icrl_cn_prepare_bwd alone (tests/test_input_grad_cpu.py: numpy against autograd; tests/test_input_grad_gpu.py: the kernel)
@functools.lru_cache(maxsize=None)
def prepare_case(name, n=37):
    rng = np.random.RandomState(len(name) + 11 * n)
    if name == "dup":          # duplicates, and observation columns 1 and 0 selected through acs_select_dim (the kept quirk); 6 = action column 1
        od, ad = 5, 3
        spec = prep_spec(od, ad, [0, 2, 2, 4] + [1, 6, 6, 0, 7], False, 1.5, -0.5 * np.ones(ad), 0.5 * np.ones(ad), rng.randn(od), rng.uniform(0.5, 2.0, od))
    elif name == "onehot":     # a discrete net: class indices in, one-hot columns, no action gradient
        od, ad = 4, 3
        spec = prep_spec(od, ad, list(range(od)) + list(range(ad)), True, 1.5, None, None, rng.randn(od), rng.uniform(0.5, 2.0, od))
    elif name == "plain":      # no normalisation, no selection beyond the default quirk: range(obs_dim) + range(acs_dim)
        od, ad = 6, 2
        spec = prep_spec(od, ad, list(range(od)) + list(range(ad)), False, 1.5, -0.5 * np.ones(ad), 0.5 * np.ones(ad))
    else:
        raise KeyError(name)
    obs = 1.5 * rng.randn(n, od)
    acs = rng.randint(0, ad, (n, 1)).astype(np.float32) if spec["is_discrete"] else (0.6 * rng.randn(n, ad)).astype(np.float32)
    d_x = rng.randn(n, len(spec["select_dim"])).astype(np.float32)
    dist, beyond = clip_margins(spec, obs, acs)
    assert dist >= CLIP_MARGIN, (name, dist)
    assert beyond[0] > 0 and beyond[1] > 0 and (spec["is_discrete"] or (beyond[2] > 0 and beyond[3] > 0)), (name, beyond)      # rows on both sides of both clips
    ref_obs, ref_acs = prepare_bwd_autograd(spec, obs, acs, d_x)
    return dict(name=name, n=n, spec=spec, obs=obs, acs=acs, d_x=d_x, d_obs64=ref_obs, d_acs64=ref_acs)


PREPARE_CASES = ("dup", "onehot", "plain")
# a sum of at most three float32 terms in float64 and one division against one multiplication by the reciprocal: a few float64 ulps
PREPARE_RTOL_OBS = 8 * 2.0 ** -52
PREPARE_RTOL_ACS = 2.0 ** -23      # the float64 sum rounded once to float32, against autograd's rounding of the same sum in another order


# ---- constraint nets --------------------------------------------------------------------------------------------------------------------------------
def oracle_costnet(shape, dtype, seed):
    """mlp_grad_cases.oracle_costnet for its named shapes; "disc": the same construction with one-hot actions"""
    if shape != "disc":
        return M.oracle_costnet(shape, dtype, seed)
    obs_dim, n_cls, hidden = DISC_SHAPE
    torch.manual_seed(seed)
    net = o_nets.CostNet(obs_dim, n_cls, list(hidden), True, None, None, CLIP_OBS, None, None)
    net.params = OrderedDict((k, v.detach().to(dtype).clone().requires_grad_(True)) for k, v in net.params.items())
    return net


def _cost_inputs(net, n, seed):
    """rows with operands strictly beyond both bounds of both clips (row 0) and none within CLIP_MARGIN of one"""
    rng = np.random.RandomState(100 + seed + 7 * n)
    obs = 2.0 * rng.randn(n, net.obs_dim)
    obs[0, 0], obs[0, 1] = 12.5, -11.25      # (columns 0 and 1: every shape here selects them)
    if net.is_discrete:
        acs = rng.randint(0, net.acs_dim, (n, 1)).astype(np.float32)
    else:
        acs = (0.8 * rng.randn(n, net.acs_dim)).astype(np.float32)
        acs[0, 0], acs[0, -1] = 1.5, -1.75
    up = rng.randn(n).astype(np.float32)
    return obs, acs, up


def _net_forward(net, x, dtype):
    h, zmin = x, np.inf
    for i in range(net.n_layers - 1):
        z = torch.nn.functional.linear(h, net.params[f"{2 * i}.weight"], net.params[f"{2 * i}.bias"])
        zmin = min(zmin, float(z.detach().abs().min()))
        h = torch.relu(z)
    return torch.sigmoid(torch.nn.functional.linear(h, net.params[f"{2 * (net.n_layers - 1)}.weight"], net.params[f"{2 * (net.n_layers - 1)}.bias"])).flatten(), zmin


def _cost_input_grads(shape, seed, obs, acs, up, dtype):
    """autograd with the inputs as leaves -> d_x (x [N, in_dim] the float32 rows icrl_cn_prepare writes, as a leaf), d_obs, d_acs | None (the
    full chain obs, acs -> zeta: prepare_torch in float64, the network evaluated AT the float32 rounding of its rows, as the device does,
    the gradient passed straight through that rounding), zeta, min |z|"""
    net = oracle_costnet(shape, dtype, seed)
    spec = spec_of(net)
    x32 = net.prepare(obs, acs).numpy()
    x = torch.as_tensor(x32).to(dtype).requires_grad_(True)
    zeta, zmin = _net_forward(net, x, dtype)
    zeta.backward(torch.as_tensor(up).to(dtype))
    o = torch.as_tensor(np.asarray(obs, np.float64)).requires_grad_(True)
    a = torch.as_tensor(acs)
    if not net.is_discrete:
        a.requires_grad_(True)
    xx = prepare_torch(spec, o, a if net.is_discrete else a.double())
    xx = xx + (xx.detach().float().double() - xx.detach())
    assert np.array_equal(xx.detach().float().numpy(), x32)
    z2, _ = _net_forward(net, xx.to(dtype), dtype)
    z2.backward(torch.as_tensor(up).to(dtype))
    return (x.grad.double().numpy(), o.grad.numpy(), None if net.is_discrete else a.grad.double().numpy(), zeta.detach().double().numpy(), zmin, x32, spec)


@functools.lru_cache(maxsize=None)
def cost_case(shape, n):
    seed = COST_SEED[case_id(shape, n)]
    net = oracle_costnet(shape, torch.float64, seed)
    obs, acs, up = _cost_inputs(net, n, seed)
    d_x, d_obs, d_acs, zeta, zmin, x32, spec = _cost_input_grads(shape, seed, obs, acs, up, torch.float64)
    dist, beyond = clip_margins(spec, obs, acs)
    assert dist >= CLIP_MARGIN, (shape, n, dist)
    assert beyond[0] > 0 and beyond[1] > 0 and (net.is_discrete or (beyond[2] > 0 and beyond[3] > 0)), (shape, n, beyond)
    sd = OrderedDict((k, v.detach().float()) for k, v in oracle_costnet(shape, torch.float32, seed).params.items())
    return dict(shape=shape, n=n, seed=seed, obs_dim=net.obs_dim, acs_dim=net.acs_dim, hidden=tuple(net.hidden), discrete=net.is_discrete, spec=spec,
                osel=None if shape != "point" else M.COST_SHAPES["point"][3], asel=None if shape != "point" else M.COST_SHAPES["point"][4],
                obs=obs, acs=acs, up=up, x=x32, in_dim=x32.shape[1], zeta64=zeta, zmin=zmin, d_x64=d_x, d_obs64=d_obs, d_acs64=d_acs, sd=sd, flat=M.pack_flat(sd))


def cost_dev32(shape, n):
    c = cost_case(shape, n)
    d_x, d_obs, d_acs, *_ = _cost_input_grads(shape, c["seed"], c["obs"], c["acs"], c["up"], torch.float32)
    return [float(np.abs(d_x - c["d_x64"]).max()), float(np.abs(d_obs - c["d_obs64"]).max())] + ([] if d_acs is None else [float(np.abs(d_acs - c["d_acs64"]).max())])


def pick_cost_seed(shape, n):
    for seed in range(200):
        net = oracle_costnet(shape, torch.float64, seed)
        obs, acs, _ = _cost_inputs(net, n, seed)
        _, zmin = _net_forward(net, net.prepare(obs, acs).double(), torch.float64)
        if zmin >= 2 * RELU_MARGIN:
            return seed, zmin
    raise AssertionError((shape, n))


# ---- torch_ops: custom losses with the inputs as leaves -------------------------------------------------------------------------------------------
LOSS_POLICY, LOSS_COST = ("o17a5", 257), ("h64", 65)


def _policy_loss_grads(dtype):
    c = policy_case(*LOSS_POLICY)
    rng = np.random.RandomState(7)
    w, t = rng.randn(c["n"]).astype(np.float32), rng.randn(c["n"]).astype(np.float32)
    pol = M.oracle_policy(c["shape"], c["sd"], dtype)
    obs = torch.as_tensor(c["obs"]).to(dtype).requires_grad_(True)
    act = torch.as_tensor(c["actions"]).to(dtype).requires_grad_(True)
    v_r, v_c, lp, ent = pol.evaluate_actions(obs, act)
    M.policy_loss(v_r.flatten(), v_c.flatten(), lp, ent, torch.as_tensor(w).to(dtype), torch.as_tensor(t).to(dtype)).backward()
    return w, t, obs.grad.double().numpy(), act.grad.double().numpy()


def _zeta_loss_grads(dtype):
    c = cost_case(*LOSS_COST)
    net = oracle_costnet(c["shape"], dtype, c["seed"])
    o = torch.as_tensor(c["obs"]).requires_grad_(True)
    a = torch.as_tensor(c["acs"]).requires_grad_(True)
    xx = prepare_torch(c["spec"], o, a.double())
    xx = xx + (xx.detach().float().double() - xx.detach())
    zeta, _ = _net_forward(net, xx.to(dtype), dtype)
    M.zeta_loss(zeta).backward()
    return o.grad.numpy(), a.grad.double().numpy()


@functools.lru_cache(maxsize=None)
def policy_loss_case():
    w, t, d_obs, d_act = _policy_loss_grads(torch.float64)
    return dict(policy_case(*LOSS_POLICY), w=w, t=t, d_obs64=d_obs, d_act64=d_act)


@functools.lru_cache(maxsize=None)
def zeta_loss_case():
    d_obs, d_acs = _zeta_loss_grads(torch.float64)
    return dict(cost_case(*LOSS_COST), d_obs64=d_obs, d_acs64=d_acs)


def loss_dev32():
    p, z = policy_loss_case(), zeta_loss_case()
    _, _, po, pa = _policy_loss_grads(torch.float32)
    zo, za = _zeta_loss_grads(torch.float32)
    return ([float(np.abs(po - p["d_obs64"]).max()), float(np.abs(pa - p["d_act64"]).max())],
            [float(np.abs(zo - z["d_obs64"]).max()), float(np.abs(za - z["d_acs64"]).max())])


def check(tag, names, got, ref, dev32):
    """per tensor: print |kernel - float64| / dev32, then assert it is <= GRAD_UNITS (mlp_grad_cases.check_grads on a list of tensors)"""
    g = OrderedDict(zip(names, got))
    return M.check_grads("IN " + tag, g, OrderedDict(zip(names, ref)), dev32)


# COST_SEED: the first seed whose float64 net keeps every ReLU pre-activation of the case at least 2 RELU_MARGIN from 0 (pick_cost_seed);
# DEV32: one number per input-gradient tensor — policy: d_obs, d_actions (Box); cost: d_x, d_obs, d_acs (Box); loss-*: d_obs, d_actions / d_acs
# TABLES_BEGIN
COST_SEED = {
    'h20-1': 0,      # min |z| = 0.0478
    'h20-63': 0,      # min |z| = 9.6e-05
    'h20-65': 0,      # min |z| = 7.58e-05
    'h20-1025': 0,      # min |z| = 4.56e-05
    'h64-1': 0,      # min |z| = 0.0213
    'h64-63': 1,      # min |z| = 0.000177
    'h64-65': 1,      # min |z| = 4.22e-05
    'h64-1025': 38,      # min |z| = 2.38e-05
    'ant-1': 0,      # min |z| = 0.00235
    'ant-63': 0,      # min |z| = 4.02e-05
    'ant-65': 0,      # min |z| = 0.000332
    'ant-1025': 6,      # min |z| = 2.08e-05
    'point-1': 0,      # min |z| = 0.0123
    'point-63': 0,      # min |z| = 7.93e-05
    'point-65': 0,      # min |z| = 7.79e-05
    'point-1025': 2,      # min |z| = 2.08e-05
    'disc-1': 0,      # min |z| = 0.0244
    'disc-63': 0,      # min |z| = 5.29e-05
    'disc-65': 0,      # min |z| = 0.000109
    'disc-1025': 1,      # min |z| = 2.1e-05
}
DEV32 = {
    'o1a1-1': [5e-10, 2.13e-07],
    'o1a1-16': [1.98e-07, 5.06e-07],
    'o1a1-17': [2.22e-07, 3.22e-07],
    'o1a1-257': [3.84e-07, 1.17e-06],
    'o1a1-1025': [8.06e-07, 1.49e-06],
    'o17a5-1': [1.6e-07, 7.87e-08],
    'o17a5-16': [6.91e-07, 1.58e-06],
    'o17a5-17': [1.45e-06, 2.84e-06],
    'o17a5-257': [3.14e-06, 4.83e-06],
    'o17a5-1025': [5.56e-06, 4.69e-06],
    'o33a1-1': [1.15e-07, 1.3e-07],
    'o33a1-16': [5.22e-07, 5e-07],
    'o33a1-17': [8.38e-07, 1.68e-06],
    'o33a1-257': [7.01e-07, 1.23e-06],
    'o33a1-1025': [1.09e-06, 1.48e-06],
    'o65a1-1': [3.05e-07, 9.42e-07],
    'o65a1-16': [4.38e-07, 4.56e-07],
    'o65a1-17': [4.67e-07, 4.57e-07],
    'o65a1-257': [6.39e-07, 1.27e-06],
    'o65a1-1025': [1.51e-06, 1.83e-06],
    'o128a16-1': [5.88e-07, 1.14e-06],
    'o128a16-16': [1.07e-05, 7.94e-06],
    'o128a16-17': [5e-06, 8.21e-06],
    'o128a16-257': [9.97e-06, 1.44e-05],
    'o128a16-1025': [1.46e-05, 2.2e-05],
    'lgw-1': [1.34e-08],
    'lgw-16': [2.55e-07],
    'lgw-17': [2.4e-07],
    'lgw-257': [3.41e-07],
    'lgw-1025': [4.08e-07],
    'g13-1': [4.3e-07, 4.97e-07],
    'g13-16': [1.01e-06, 2.68e-06],
    'g13-17': [1.16e-06, 1.9e-06],
    'g13-257': [2.55e-06, 4.13e-06],
    'g13-1025': [2.71e-06, 6.34e-06],
    'cost-h20-1': [2.44e-09, 3.35e-09, 0],
    'cost-h20-63': [8.96e-09, 1.13e-08, 0],
    'cost-h20-65': [5.12e-09, 5.12e-09, 0],
    'cost-h20-1025': [1.94e-08, 2.03e-08, 0],
    'cost-h64-1': [1.42e-09, 1.61e-09, 0],
    'cost-h64-63': [6.49e-09, 6.49e-09, 0],
    'cost-h64-65': [5.32e-09, 7.92e-09, 0],
    'cost-h64-1025': [1.1e-08, 1.1e-08, 0],
    'cost-ant-1': [1.82e-09, 1.84e-09, 0],
    'cost-ant-63': [4.06e-09, 4.06e-09, 0],
    'cost-ant-65': [2.59e-09, 2.59e-09, 0],
    'cost-ant-1025': [3.56e-09, 3.56e-09, 0],
    'cost-point-1': [6.88e-10, 0, 0],
    'cost-point-63': [8.12e-09, 1.25e-08, 0],
    'cost-point-65': [7.51e-09, 6.05e-09, 0],
    'cost-point-1025': [1.58e-08, 2.32e-08, 0],
    'cost-disc-1': [2.24e-09, 2.04e-09],
    'cost-disc-63': [4.66e-09, 7.15e-09],
    'cost-disc-65': [4.87e-09, 6.79e-09],
    'cost-disc-1025': [7.66e-09, 7.66e-09],
    'loss-policy': [3.82e-06, 2.82e-06],
    'loss-zeta': [1.05e-10, 0],
}
# TABLES_END


if __name__ == "__main__":
    print("COST_SEED = {")
    for s, n in COST_CASES:
        seed, zmin = pick_cost_seed(s, n)
        COST_SEED[case_id(s, n)] = seed
        print(f"    {case_id(s, n)!r}: {seed},      # min |z| = {zmin:.3g}")
    print("}")
    print("DEV32 = {")
    for s, n in POLICY_CASES:
        print(f"    {case_id(s, n)!r}: [" + ", ".join(f"{d:.3g}" for d in policy_dev32(s, n)) + "],")
    for s, n in COST_CASES:
        print(f"    {'cost-' + case_id(s, n)!r}: [" + ", ".join(f"{d:.3g}" for d in cost_dev32(s, n)) + "],")
    lp, lz = loss_dev32()
    print("    'loss-policy': [" + ", ".join(f"{d:.3g}" for d in lp) + "],")
    print("    'loss-zeta': [" + ", ".join(f"{d:.3g}" for d in lz) + "],")
    print("}")
    # what rounding the float64 reference once to float32 costs against the bound: the least a correct kernel can show
    for s, n in POLICY_CASES:
        c, d = policy_case(s, n), policy_dev32(s, n)
        r = [float(np.abs(c["d_obs64"].astype(np.float32) - c["d_obs64"]).max()) / d[0]] + ([] if c["d_act64"] is None else
                                                                                            [float(np.abs(c["d_act64"].astype(np.float32) - c["d_act64"]).max()) / d[1]])
        print(f"# {case_id(s, n)}: one rounding / dev32 = " + ", ".join(f"{v:.2f}" for v in r))
    for s, n in COST_CASES:
        c, d = cost_case(s, n), cost_dev32(s, n)
        print(f"# cost-{case_id(s, n)}: one rounding of d_x / dev32 = {float(np.abs(c['d_x64'].astype(np.float32) - c['d_x64']).max()) / d[0]:.2f}")
