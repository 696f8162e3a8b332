"""Cases and float64 references of the fused network forward + backward (csrc/mlp_grad.hip; icrl_policy_fwd_bwd, icrl_cost_mlp_fwd_bwd,
icrl_amd/torch_ops.py).  Everything here runs on the CPU: the oracle's networks (oracle/nets.py) under torch autograd.

The reference of a gradient is FLOAT64 autograd of the oracle network: its parameters cast to float64, the same float32 inputs and upstream
gradients.  The bound, per parameter tensor and max-abs:
    |kernel - float64| <= 4 * dev32,    dev32 = max |float32 CPU autograd - float64 CPU autograd| of the same case
Three units follow ROW_GRAD_F32_DEV of tests/test_fine_grained_gpu.py (sums in another order than torch's), one more covers the device's
tanh / exp / log within HIP's documented 2 ulp of the host's.  dev32 is a property of the case, not of the kernel: it is measured here, on the
CPU, and stored in DEV32 below by
    python tests/helpers/mlp_grad_cases.py          (prints the table; torch 2.10 CPU, default threads)
tests/test_mlp_grad_cpu.py checks that the table has an entry, nonzero or exact by construction, for every case.

Policy states are TRAINED-like, not the initial one: log_std uniform in [-1.5, 0.5], every tensor perturbed by 0.1 N(0, 1), actions N(0, 1), so
that d log_std and the action head's gradients are not small.  Constraint nets keep torch's default initialisation; a ReLU unit whose
pre-activation is nearly 0 may flip between float32 and float64, so every case asserts min |z| >= RELU_MARGIN on the float64 oracle before any
kernel runs (the seed is picked here, on the CPU; no row is ever left out).
"""
import functools
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from oracle import nets as o_nets      # noqa: E402

HW = 64                                                 # storage width of a hidden layer (icrl_amd/policies.py: HW)
G13_WIDTHS = dict(policy_net=(32, 48), value_net=(64, 32), cost_value_net=(16, 64))      # oracle/gen_golden.py: g13_widths
# name -> obs_dim, act_dim, discrete, hidden.  "lgw": the LapGridWorld policy (icrl_amd/vec_env.py: KINDS["lgw"] = 1 observation, Discrete(2))
POLICY_SHAPES = OrderedDict(hc=(18, 6, False, (64, 64)), ant=(113, 8, False, (64, 64)), point=(9, 2, False, (64, 64)), lgw=(1, 2, True, (64, 64)),
                            g13=(18, 6, False, G13_WIDTHS))
# widths between hc and ant (tests/helpers/width_cases.py): the 16-column tile edges of the observation and both extremes of the action head
WIDTH_SHAPES = ((1, 1), (17, 5), (32, 16), (33, 1), (64, 16), (65, 1), (128, 16))
WIDTH_ROWS = (17, 100)
POLICY_SHAPES.update((f"o{o}a{a}", (o, a, False, (64, 64))) for o, a in WIDTH_SHAPES)
POLICY_ROWS = (1, 15, 16, 17, 64, 100, 257)             # the row-tile edge (16), a ragged last tile, more than one workgroup
# past the grid cap of mlp_fwd_bwd_kernel (16-row tiles on min(tiles, 64) workgroups; weight gradients stay in registers across a workgroup's
# tiles): 1025 rows = 65 tiles, workgroup 0 alone walks a second one, which holds one live row; 2064 rows = 129 tiles, workgroup 0 walks three,
# the others two; 65536 rows = the served maximum, 64 tiles per workgroup
POLICY_ROWS_WALK = (1025, 2064)
POLICY_CASES = ([(s, n) for s in ("hc", "ant", "point", "lgw") for n in POLICY_ROWS] + [("g13", 100)]
                + [(s, n) for s in ("hc", "ant") for n in POLICY_ROWS_WALK] + [("lgw", 1025), ("hc", 65536)]
                + [(f"o{o}a{a}", n) for o, a in WIDTH_SHAPES for n in WIDTH_ROWS])
# name -> obs_dim, acs_dim, hidden, obs_select_dim, acs_select_dim.  "point": the Point fixture's selection (-cosd 0 1 -casd -1)
COST_SHAPES = OrderedDict(h20=(18, 6, (20,), None, None), h64=(18, 6, (64, 64), None, None), ant=(113, 8, (40, 40), None, None),
                          point=(9, 2, (40, 40), (0, 1), (-1,)))
COST_ROWS = (1, 63, 64, 65, 257)
COST_CASES = [(s, n) for s in COST_SHAPES for n in COST_ROWS] + [(s, n) for s in ("h20", "ant") for n in POLICY_ROWS_WALK]      # h20: sdz1 = sdz
RELU_MARGIN = 1e-5
COST_SEED = {("ant", 257): 2, ("ant", 1025): 3, ("ant", 2064): 18}      # every other case: seed 0 (min |z| asserted in cost_case)
OUT_TOL = dict(v_r=(1e-5, 2e-6), v_c=(1e-5, 2e-6), zeta=(1e-5, 2e-6), log_prob=(1e-5, 2e-5), entropy=(1e-5, 2e-5))      # rtol, atol: the fp32-MLP tolerance
GRAD_UNITS = 4.0


def case_id(shape, n):
    return f"{shape}-{n}"


# ---- the flat device layout (icrl_amd/policies.py: _pad / _physical_shape): hidden layers stored 64 wide, zeros beyond the logical widths
def physical_shape(name, shp, obs_dim):
    if name == "log_std":
        return tuple(shp)
    if name.startswith("mlp_extractor."):
        first = name.split(".")[2] == "0"
        return (HW, obs_dim if first else HW) if name.endswith("weight") else (HW,)
    return (shp[0], HW) if name.endswith("weight") else tuple(shp)


def pack_policy(tensors, obs_dim):
    """OrderedDict of logical tensors (state_dict order) -> flat float32 numpy vector in the device layout."""
    out = []
    for k, v in tensors.items():
        v = np.asarray(v.detach().numpy() if torch.is_tensor(v) else v, np.float32)
        full = np.zeros(physical_shape(k, v.shape, obs_dim), np.float32)
        full[tuple(slice(0, m) for m in v.shape)] = v
        out.append(full.ravel())
    return np.concatenate(out)


def unpack_policy(flat, logical_shapes, obs_dim):
    """flat device-layout vector -> (OrderedDict name -> logical part, OrderedDict name -> the padding entries as a flat array)."""
    flat = np.asarray(flat)
    parts, pads, off = OrderedDict(), OrderedDict(), 0
    for k, shp in logical_shapes.items():
        phys = physical_shape(k, shp, obs_dim)
        n = int(np.prod(phys))
        full = flat[off:off + n].reshape(phys)
        mask = np.ones(phys, bool)
        mask[tuple(slice(0, m) for m in shp)] = False
        parts[k], pads[k] = full[tuple(slice(0, m) for m in shp)].copy(), full[mask].copy()
        off += n
    assert off == flat.size, (off, flat.size)
    return parts, pads


def pack_flat(tensors):
    return np.concatenate([np.asarray(v.detach().numpy() if torch.is_tensor(v) else v, np.float32).ravel() for v in tensors.values()])


def unpack_flat(flat, shapes):
    out, off = OrderedDict(), 0
    for k, shp in shapes.items():
        n = int(np.prod(shp))
        out[k] = np.asarray(flat[off:off + n]).reshape(shp).copy()
        off += n
    assert off == len(flat)
    return out


# ---- the oracle policy at any dtype (oracle.nets.TwoCriticPolicy.latents casts the observation to float32: the float64 run walks the branches itself)
def oracle_policy(shape, sd=None, dtype=torch.float32):
    obs_dim, act_dim, discrete, hidden = POLICY_SHAPES[shape] if isinstance(shape, str) else shape
    pol = o_nets.TwoCriticPolicy(obs_dim, act_dim, hidden, discrete=discrete, ortho_init=sd is None)
    if sd is not None:
        pol.load_state_dict(sd)
    pol.params = OrderedDict((k, v.detach().to(dtype).clone().requires_grad_(True)) for k, v in pol.params.items())
    pol.latents = lambda obs: tuple(pol._branch(obs.to(dtype), b, len(pol.widths[b])) for b in pol.BRANCHES)
    return pol


def policy_grads(pol, obs, actions, ups, dtype):
    """autograd of sum_n (d_v_r v_r + d_v_c v_c + d_lp log_prob + d_ent entropy) over pol's parameters -> (outputs, grads), numpy float64."""
    for v in pol.params.values():
        v.grad = None
    v_r, v_c, lp, ent = pol.evaluate_actions(torch.as_tensor(obs).to(dtype), torch.as_tensor(actions).to(dtype))
    outs = dict(v_r=v_r.flatten(), v_c=v_c.flatten(), log_prob=lp, entropy=ent)
    torch.autograd.backward([outs[k] for k in ("v_r", "v_c", "log_prob", "entropy")],
                            [torch.as_tensor(ups[k]).to(dtype) for k in ("v_r", "v_c", "log_prob", "entropy")])
    return ({k: v.detach().double().numpy() for k, v in outs.items()},
            OrderedDict((k, (v.grad if v.grad is not None else torch.zeros_like(v)).double().numpy()) for k, v in pol.params.items()))


def trained_state(shape, seed=0):
    """the perturbed state of a named policy shape: an OrderedDict of float32 tensors in state_dict order.  Drawn with numpy alone (the
    initial weights have the scale of the reference's orthogonal initialisation, gain / sqrt(larger dimension); its QR goes through LAPACK and
    is not the same bits on every CPU), so that the case, and with it its float64 reference, is the same on every machine."""
    obs_dim, act_dim, discrete, hidden = POLICY_SHAPES[shape]
    pol = o_nets.TwoCriticPolicy(obs_dim, act_dim, hidden, discrete=discrete, ortho_init=False)      # names and shapes
    rng = np.random.RandomState(2000 + seed)
    sd = OrderedDict()
    for k, v in pol.params.items():
        shp = tuple(v.shape)
        if k == "log_std":
            val = rng.uniform(-1.5, 0.5, shp)
        elif k.endswith("weight"):
            gain = 0.01 if k == "action_net.weight" else (1.0 if k in ("value_net.weight", "cost_value_net.weight") else np.sqrt(2.0))
            val = gain * rng.randn(*shp) / np.sqrt(max(shp)) + 0.1 * rng.randn(*shp)
        else:
            val = 0.1 * rng.randn(*shp)
        sd[k] = torch.as_tensor(val.astype(np.float32))
    return sd


@functools.lru_cache(maxsize=None)
def policy_case(shape, n):
    """inputs, upstream gradients and the float64 reference of one case; computed once, shared, never written to."""
    obs_dim, act_dim, discrete, hidden = POLICY_SHAPES[shape]
    sd = trained_state(shape)
    rng = np.random.RandomState(31 * n + len(shape))
    obs = rng.randn(n, obs_dim).astype(np.float32)
    actions = rng.randint(0, act_dim, (n, 1)).astype(np.float32) if discrete else rng.randn(n, act_dim).astype(np.float32)
    ups = {k: rng.randn(n).astype(np.float32) for k in ("v_r", "v_c", "log_prob", "entropy")}
    out64, g64 = policy_grads(oracle_policy(shape, sd, torch.float64), obs, actions, ups, torch.float64)
    return dict(shape=shape, n=n, obs_dim=obs_dim, act_dim=act_dim, discrete=discrete, sd=sd, obs=obs, actions=actions, ups=ups, out64=out64, g64=g64,
                logical_shapes=OrderedDict((k, tuple(v.shape)) for k, v in sd.items()), flat=pack_policy(sd, obs_dim))


def policy_dev32(shape, n):
    c = policy_case(shape, n)
    _, g32 = policy_grads(oracle_policy(shape, c["sd"], torch.float32), c["obs"], c["actions"], c["ups"], torch.float32)
    return [float(np.abs(g32[k] - c["g64"][k]).max()) for k in c["g64"]]


# ---- constraint nets
def oracle_costnet(shape, dtype=torch.float32, seed=0):
    obs_dim, acs_dim, hidden, osel, asel = COST_SHAPES[shape]
    torch.manual_seed(seed)
    lo = -np.ones(acs_dim, np.float32)
    net = o_nets.CostNet(obs_dim, acs_dim, list(hidden), False, None if osel is None else list(osel), None if asel is None else list(asel), 10.0, lo, -lo)
    net.params = OrderedDict((k, v.detach().to(dtype).clone().requires_grad_(True)) for k, v in net.params.items())
    return net


def cost_grads(net, x, up, dtype):
    for v in net.params.values():
        v.grad = None
    h, zmin = torch.as_tensor(x).to(dtype), np.inf
    for i in range(net.n_layers - 1):      # the hidden pre-activations, for the ReLU margin
        z = torch.nn.functional.linear(h, net.params[f"{2 * i}.weight"], net.params[f"{2 * i}.bias"])
        zmin = min(zmin, float(z.detach().abs().min()))
        h = torch.relu(z)
    zeta = net.forward(torch.as_tensor(x).to(dtype)).flatten()
    zeta.backward(torch.as_tensor(up).to(dtype))
    return zeta.detach().double().numpy(), OrderedDict((k, v.grad.double().numpy()) for k, v in net.params.items()), zmin


@functools.lru_cache(maxsize=None)
def cost_case(shape, n):
    obs_dim, acs_dim, hidden, osel, asel = COST_SHAPES[shape]
    seed = COST_SEED.get((shape, n), 0)
    net64 = oracle_costnet(shape, torch.float64, seed)      # (seeds torch: the same weights at both dtypes)
    np.random.seed(seed)
    torch.manual_seed(seed)
    obs = 2.0 * np.random.randn(n, obs_dim)
    acs = np.clip(np.random.randn(n, acs_dim), -1.0, 1.0).astype(np.float32)
    up = np.random.randn(n).astype(np.float32)
    x = net64.prepare(obs, acs).numpy()      # float32 rows: what icrl_cn_prepare writes
    zeta64, g64, zmin = cost_grads(net64, x, up, torch.float64)
    sd = OrderedDict((k, v.detach().float()) for k, v in oracle_costnet(shape, torch.float32, seed).params.items())
    return dict(shape=shape, n=n, seed=seed, obs_dim=obs_dim, acs_dim=acs_dim, hidden=hidden, osel=osel, asel=asel, obs=obs, acs=acs, x=x, up=up, zeta64=zeta64,
                g64=g64, zmin=zmin, sd=sd, shapes=OrderedDict((k, tuple(v.shape)) for k, v in sd.items()), flat=pack_flat(sd), in_dim=x.shape[1])


def cost_dev32(shape, n):
    c = cost_case(shape, n)
    _, g32, _ = cost_grads(oracle_costnet(shape, torch.float32, c["seed"]), c["x"], c["up"], torch.float32)
    return [float(np.abs(g32[k] - c["g64"][k]).max()) for k in c["g64"]]


# ---- custom torch losses through icrl_amd/torch_ops.py: the same expressions on the oracle's outputs
def policy_loss(v_r, v_c, log_prob, entropy, w, t):
    return (log_prob * w).sum() + (v_r ** 2).mean() + 0.3 * (v_c - t).abs().mean() - 0.01 * entropy.mean()


def zeta_loss(zeta):
    return -(torch.log(zeta + 1e-5)).mean()


LOSS_POLICY, LOSS_COST = ("hc", 100), ("h64", 65)


def _policy_loss_grads(dtype):
    c = policy_case(*LOSS_POLICY)
    rng = np.random.RandomState(7)
    w, t = rng.randn(c["n"]).astype(np.float32), rng.randn(c["n"]).astype(np.float32)
    pol = oracle_policy(c["shape"], c["sd"], dtype)
    v_r, v_c, lp, ent = pol.evaluate_actions(torch.as_tensor(c["obs"]).to(dtype), torch.as_tensor(c["actions"]).to(dtype))
    policy_loss(v_r.flatten(), v_c.flatten(), lp, ent, torch.as_tensor(w).to(dtype), torch.as_tensor(t).to(dtype)).backward()
    return w, t, OrderedDict((k, v.grad.double().numpy()) for k, v in pol.params.items())


def _zeta_loss_grads(dtype):
    c = cost_case(*LOSS_COST)
    net = oracle_costnet(c["shape"], dtype, c["seed"])
    zeta_loss(net.forward(torch.as_tensor(c["x"]).to(dtype)).flatten()).backward()
    return OrderedDict((k, v.grad.double().numpy()) for k, v in net.params.items())


@functools.lru_cache(maxsize=None)
def policy_loss_case():
    w, t, g64 = _policy_loss_grads(torch.float64)
    return dict(policy_case(*LOSS_POLICY), w=w, t=t, g64=g64)


@functools.lru_cache(maxsize=None)
def zeta_loss_case():
    return dict(cost_case(*LOSS_COST), g64=_zeta_loss_grads(torch.float64))


def loss_dev32():
    p64, z64 = policy_loss_case()["g64"], zeta_loss_case()["g64"]
    p32, z32 = _policy_loss_grads(torch.float32)[2], _zeta_loss_grads(torch.float32)
    return [float(np.abs(p32[k] - p64[k]).max()) for k in p64], [float(np.abs(z32[k] - z64[k]).max()) for k in z64]


def check_grads(tag, got, g64, dev32, report=None):
    """per tensor: print |kernel - float64| / dev32, then assert it is <= GRAD_UNITS.  Returns the largest ratio (exact tensors count as 0)."""
    worst, bad = 0.0, []
    for (k, ref), d in zip(g64.items(), dev32):
        err = float(np.abs(np.asarray(got[k], np.float64) - ref).max())
        ratio = err / d if d > 0 else (0.0 if err == 0 else np.inf)
        print(f"MLP_GRAD {tag} {k}: |kernel - float64| = {err:.3g}, dev32 = {d:.3g}, ratio {ratio:.2f} (largest entry {np.abs(ref).max():.3g})")
        worst = max(worst, ratio)
        if err > GRAD_UNITS * d:
            bad.append((k, err, d))
    if report is not None:
        report.append((tag, worst))
    assert not bad, (tag, bad)
    return worst


def check_outputs(tag, got, ref):
    for k, v in got.items():
        rtol, atol = OUT_TOL[k]
        err = np.abs(np.asarray(v, np.float64) - ref[k])
        print(f"MLP_GRAD {tag} {k}: max |kernel - float64| = {err.max():.3g}")
        assert np.all(err <= atol + rtol * np.abs(ref[k])), (tag, k, err.max())


# dev32 per case: one number per parameter tensor, in state_dict order (DEV32_BEGIN .. DEV32_END is what the command above prints)
# DEV32_BEGIN
DEV32 = {
    'hc-1': [2.13e-06, 1.38e-06, 6.85e-07, 7.55e-07, 6.65e-07, 6.03e-08, 2.75e-08, 2.72e-08, 1.77e-08, 2.47e-08, 1.11e-08, 1.13e-08, 9.44e-09, 1.64e-06, 1.15e-06, 1.29e-07, 0, 3.68e-08, 0],
    'hc-15': [7.05e-06, 3.04e-06, 2.4e-06, 2e-06, 1.51e-06, 4.12e-07, 1.92e-07, 2.43e-07, 1.49e-07, 6.97e-07, 4.43e-07, 2.44e-07, 3.66e-07, 7.91e-06, 3.93e-06, 9.46e-07, 8.94e-08, 1.19e-06, 1.49e-07],
    'hc-16': [3.02e-06, 2.49e-06, 1.34e-06, 1.54e-06, 8.24e-07, 8.51e-07, 2.74e-07, 2.3e-07, 2.03e-07, 5.93e-07, 2.74e-07, 2.93e-07, 1.38e-07, 4.66e-06, 2.44e-06, 7.54e-07, 1.42e-07, 7.62e-07, 3.32e-07],
    'hc-17': [1.1e-05, 4.91e-06, 2.99e-06, 3.31e-06, 2.59e-06, 4.81e-07, 3.98e-07, 2.76e-07, 1.41e-07, 5.77e-07, 2.15e-07, 2.76e-07, 3.35e-07, 1.21e-05, 3.68e-06, 1.28e-06, 3.5e-07, 1.11e-06, 9.87e-08],
    'hc-64': [6.98e-06, 5.53e-06, 3.12e-06, 4.69e-06, 2.68e-06, 1.38e-06, 6.01e-07, 5.3e-07, 3.22e-07, 2.6e-06, 5.05e-07, 9.74e-07, 3.5e-07, 1.36e-05, 4.03e-06, 2.05e-06, 6.67e-07, 2.93e-06, 5.59e-08],
    'hc-100': [3.59e-05, 1.08e-05, 5.7e-06, 7.64e-06, 3.76e-06, 1.3e-06, 1.06e-06, 8.43e-07, 4.39e-07, 1.56e-06, 5.88e-07, 1.16e-06, 4.43e-07, 3.93e-05, 1.44e-05, 2.37e-06, 7.77e-07, 3.21e-06, 4.94e-08],
    'hc-257': [3.04e-05, 3.3e-05, 1.42e-05, 1.8e-05, 1.18e-05, 4.55e-06, 9.39e-07, 1.97e-06, 9.01e-07, 6.68e-06, 9.91e-07, 3.34e-06, 6.86e-07, 8.36e-05, 2.12e-05, 1.16e-05, 8.25e-07, 1.14e-05, 1.24e-07],
    'ant-1': [2.44e-06, 1.01e-06, 3.95e-07, 5.83e-07, 2.69e-07, 2.9e-08, 1.24e-08, 1.73e-08, 1.57e-08, 1.9e-07, 8.01e-08, 9.63e-08, 2.88e-08, 2.93e-06, 3.32e-07, 3.67e-08, 0, 2.03e-07, 0],
    'ant-15': [4.48e-05, 7.35e-06, 3.75e-06, 5.09e-06, 4.25e-06, 4.76e-07, 1.64e-07, 3.98e-07, 1.69e-07, 9.91e-07, 4.09e-07, 7.38e-07, 2.5e-07, 2.53e-05, 9.38e-06, 1.27e-06, 5.96e-08, 1.44e-06, 3.28e-07],
    'ant-16': [1.85e-05, 1.02e-05, 5.07e-06, 7.07e-06, 4.46e-06, 8.69e-07, 2.35e-07, 4.28e-07, 2.4e-07, 1.38e-06, 5.94e-07, 4.65e-07, 3.01e-07, 2.84e-05, 7.62e-06, 1.07e-06, 1.34e-07, 1.22e-06, 1.24e-07],
    'ant-17': [6.83e-06, 5.97e-06, 2.68e-06, 3.93e-06, 2.59e-06, 5.67e-07, 2.41e-07, 6.05e-07, 3.99e-07, 6.39e-07, 3.44e-07, 5e-07, 2.05e-07, 2e-05, 7.11e-06, 1.79e-06, 1.04e-07, 9.56e-07, 4.47e-07],
    'ant-64': [3.91e-05, 1.86e-05, 7.47e-06, 1.41e-05, 7.91e-06, 1.12e-06, 5.66e-07, 1.38e-06, 4.18e-07, 2.09e-06, 9.1e-07, 1.72e-06, 9.65e-07, 5.05e-05, 1.71e-05, 3.95e-06, 7.12e-07, 3.65e-06, 1.15e-07],
    'ant-100': [2.56e-05, 2.76e-05, 7.3e-06, 1.53e-05, 5.93e-06, 2.15e-06, 7.81e-07, 1.51e-06, 8.57e-07, 2.03e-06, 1.21e-06, 1.58e-06, 6.99e-07, 9.37e-05, 2.18e-05, 4.62e-06, 9.25e-07, 4.28e-06, 9.59e-08],
    'ant-257': [6.53e-05, 4.69e-05, 1.8e-05, 4.75e-05, 1.94e-05, 3.64e-06, 2.16e-06, 4.81e-06, 1.79e-06, 4.4e-06, 1.21e-06, 4.99e-06, 1.28e-06, 0.000132, 4.7e-05, 1.38e-05, 2.54e-06, 9.62e-06, 5.38e-07],
    'point-1': [5.68e-08, 2.39e-08, 1.48e-08, 7.01e-09, 5.68e-09, 2.05e-07, 1.28e-07, 5.31e-08, 3.85e-08, 1.82e-07, 1.25e-07, 7.11e-08, 8.07e-08, 2.96e-08, 1.16e-08, 2.38e-07, 0, 2.11e-07, 0],
    'point-15': [3.94e-06, 8.47e-07, 7.88e-07, 4.26e-07, 4.63e-07, 5.36e-07, 2.73e-07, 2.98e-07, 2.45e-07, 3.89e-07, 4.42e-07, 2.05e-07, 2.52e-07, 1.96e-06, 1.44e-06, 8e-07, 2.68e-07, 8.07e-07, 1.81e-07],
    'point-16': [1.91e-06, 6.69e-07, 5.97e-07, 2.49e-07, 1.67e-07, 6.42e-07, 3.44e-07, 1.91e-07, 2.39e-07, 5.67e-07, 5.7e-07, 2.49e-07, 1.84e-07, 1.43e-06, 6.79e-07, 7.25e-07, 1.86e-07, 7.22e-07, 2.46e-07],
    'point-17': [4.37e-06, 1.05e-06, 6.6e-07, 4.64e-07, 4.92e-07, 3.45e-07, 4.03e-07, 3.72e-07, 1.08e-07, 3.61e-07, 1.7e-07, 1.64e-07, 1.64e-07, 3.01e-06, 2.13e-06, 7.32e-07, 2.22e-07, 9.56e-07, 4.47e-08],
    'point-64': [6.38e-06, 2.1e-06, 1.32e-06, 1.06e-06, 6.32e-07, 1.44e-06, 4.13e-07, 6.05e-07, 2.44e-07, 2.59e-06, 6.92e-07, 1.1e-06, 4.42e-07, 5.57e-06, 2.75e-06, 1.79e-06, 2.09e-07, 3.21e-06, 4e-08],
    'point-100': [5.54e-07, 5.94e-06, 1.39e-06, 1.99e-06, 1.24e-06, 1.3e-06, 5.32e-07, 5.36e-07, 3.03e-07, 1.98e-06, 1.13e-06, 1.42e-06, 4.3e-07, 1.03e-05, 3.73e-06, 2.2e-06, 3.66e-07, 2.18e-06, 9.1e-07],
    'point-257': [1.3e-05, 6.64e-06, 1.72e-06, 3.57e-06, 1.19e-06, 5.09e-06, 1.29e-06, 4.77e-06, 6.07e-07, 3.42e-06, 1.78e-06, 2.37e-06, 1.03e-06, 2.3e-05, 4.22e-06, 5.72e-06, 9.47e-07, 4.73e-06, 2.51e-06],
    'lgw-1': [8.17e-09, 3.32e-08, 4.33e-09, 1.86e-08, 1.49e-08, 5.52e-08, 6.72e-09, 1.15e-08, 6.18e-09, 2.5e-08, 2.7e-09, 8.5e-09, 2.77e-08, 6.31e-08, 3.97e-08, 0, 1.25e-08, 0],
    'lgw-15': [2.27e-07, 1.93e-07, 1.03e-07, 1.57e-07, 2.99e-07, 3.19e-07, 7.78e-08, 1.4e-07, 3.54e-07, 4.35e-07, 9.84e-08, 1.29e-07, 4.66e-07, 4.98e-07, 4.96e-07, 8.94e-08, 4.95e-07, 2.05e-08],
    'lgw-16': [2.77e-07, 2.86e-07, 1.08e-07, 9.97e-08, 5.97e-07, 4.07e-07, 1.22e-07, 7.1e-08, 4.01e-07, 3.14e-07, 1.1e-07, 1.06e-07, 5.39e-07, 6.37e-08, 4.26e-07, 1.04e-07, 4.26e-07, 7.45e-09],
    'lgw-17': [2.86e-07, 2.97e-07, 6.42e-08, 1.24e-07, 4.59e-07, 3.75e-07, 8.46e-08, 1.08e-07, 4.51e-07, 5.98e-07, 1.37e-07, 2.8e-07, 5.27e-07, 2.69e-07, 5.99e-07, 7.45e-08, 7.46e-07, 3.01e-07],
    'lgw-64': [4.37e-07, 3.07e-07, 1.14e-07, 1.3e-07, 1.29e-06, 1.32e-06, 3.8e-07, 5.83e-07, 6.62e-07, 1.04e-06, 2e-07, 4.63e-07, 6.17e-07, 2.89e-07, 1.92e-06, 2.01e-07, 9.95e-07, 1.75e-07],
    'lgw-100': [1.06e-06, 7.54e-07, 7.14e-07, 4.23e-07, 3.39e-06, 9.73e-07, 1.33e-06, 7.1e-07, 9e-07, 1.3e-06, 4.64e-07, 5.51e-07, 3.68e-06, 8.6e-07, 2.65e-06, 1.26e-06, 1.25e-06, 6.49e-07],
    'lgw-257': [1.46e-06, 2.13e-06, 1.13e-06, 6.91e-07, 1.15e-06, 2.12e-06, 6.24e-07, 1.04e-06, 2.54e-06, 2.63e-06, 7.38e-07, 7.21e-07, 3.84e-06, 2.37e-06, 1.72e-06, 9.13e-07, 2.21e-06, 7.54e-07],
    'g13-100': [7.71e-06, 7.83e-06, 6.83e-06, 5.75e-06, 3.32e-06, 1.55e-06, 7.14e-07, 1.98e-06, 1.01e-06, 1.27e-06, 5.44e-07, 2.6e-06, 6.37e-07, 3.54e-05, 2.13e-05, 1.88e-06, 1.66e-06, 5.59e-06, 1.11e-06],
    'hc-1025': [8.51e-05, 4.71e-05, 1.76e-05, 2.9e-05, 1.47e-05, 4.65e-06, 2.89e-06, 5.12e-06, 3.14e-06, 6.43e-06, 2.41e-06, 5.84e-06, 2.23e-06, 8.04e-05, 1.95e-05, 1.29e-05, 9.09e-07, 1.44e-05, 3.21e-06],
    'hc-2064': [4.89e-05, 5.85e-05, 2.14e-05, 3.95e-05, 1.82e-05, 8.82e-06, 2.95e-06, 8.82e-06, 3.23e-06, 1.05e-05, 2.96e-06, 6.97e-06, 3.78e-06, 0.000207, 3.16e-05, 2.35e-05, 3.02e-06, 1.83e-05, 2.98e-06],
    'ant-1025': [0.000477, 0.000135, 2.96e-05, 7.47e-05, 4.17e-05, 5.33e-06, 2.46e-06, 6.43e-06, 2.33e-06, 7.32e-06, 2.33e-06, 9.36e-06, 3.14e-06, 0.000313, 4.93e-05, 1.67e-05, 2.03e-07, 1.24e-05, 1.55e-06],
    'ant-2064': [0.000169, 0.000129, 4.1e-05, 9.37e-05, 3.44e-05, 8.19e-06, 3.14e-06, 1.2e-05, 2.98e-06, 1.21e-05, 3.63e-06, 1.24e-05, 3.19e-06, 0.000575, 0.00015, 2.29e-05, 1.16e-07, 1.8e-05, 8.86e-06],
    'lgw-1025': [2.04e-06, 2.55e-06, 1.18e-06, 1.24e-06, 2.43e-06, 3.72e-06, 2.12e-06, 2.54e-06, 3.59e-06, 3.74e-06, 2.55e-06, 1.62e-06, 4.87e-06, 4.1e-06, 7.4e-06, 6.65e-06, 5.42e-06, 5.69e-06],
    'hc-65536': [0.000845, 0.000307, 0.000191, 0.000253, 0.000101, 4.93e-05, 2.11e-05, 4.14e-05, 1.23e-05, 5.39e-05, 2.84e-05, 5.09e-05, 1.89e-05, 0.00121, 0.000262, 0.000571, 2.2e-05, 0.000448, 8.47e-06],
    'o1a1-17': [3.08e-07, 3.59e-07, 3.72e-07, 1.06e-07, 1.89e-07, 6.8e-07, 7.23e-07, 1.28e-07, 4.47e-07, 4.38e-07, 3.72e-07, 8.97e-08, 1.42e-07, 7.99e-07, 5.14e-07, 6.78e-07, 1.01e-07, 4.47e-07, 3.41e-07],
    'o1a1-100': [6.43e-06, 1.45e-06, 2.18e-06, 5.74e-07, 9.43e-07, 1.6e-06, 1.65e-06, 2.95e-07, 4.46e-07, 2.7e-06, 1.9e-06, 8.04e-07, 7.59e-07, 3.81e-06, 4.09e-06, 1.76e-06, 5.16e-08, 1.56e-06, 9.3e-07],
    'o17a5-17': [6.23e-06, 3.62e-06, 2.16e-06, 2.16e-06, 2.15e-06, 9.06e-07, 5.99e-07, 3.54e-07, 2.98e-07, 9.45e-07, 3.83e-07, 4.51e-07, 1.54e-07, 7.62e-06, 5.6e-06, 1.14e-06, 2.7e-08, 8.95e-07, 2.12e-07],
    'o17a5-100': [1.37e-05, 1.73e-05, 6.91e-06, 6.9e-06, 3.25e-06, 1.08e-06, 6.17e-07, 1.49e-06, 7.42e-07, 2.52e-06, 1.01e-06, 2.01e-06, 4.87e-07, 2.71e-05, 1.23e-05, 2.97e-06, 2.4e-07, 2.34e-06, 4.29e-07],
    'o32a16-17': [5.36e-05, 3.08e-05, 1.35e-05, 7.85e-06, 6.23e-06, 7.61e-07, 3.85e-07, 4.34e-07, 2.16e-07, 7.56e-07, 3.7e-07, 3.04e-07, 3.81e-07, 3.79e-05, 1.94e-05, 1.28e-06, 5.08e-08, 1.1e-06, 5.69e-07],
    'o32a16-100': [5.73e-05, 3.91e-05, 1.59e-05, 2.42e-05, 9.54e-06, 2.62e-06, 7.15e-07, 1.64e-06, 1.28e-06, 2.66e-06, 8.65e-07, 1.66e-06, 5.07e-07, 0.000129, 2e-05, 3.39e-06, 9.16e-07, 3.51e-06, 3.8e-07],
    'o33a1-17': [5.32e-07, 1.59e-06, 5.14e-07, 8.22e-07, 6.87e-07, 5.81e-07, 2.44e-07, 5.21e-07, 3.19e-07, 4.14e-07, 2.29e-07, 2.52e-07, 2.77e-07, 4.05e-06, 1.42e-06, 1.66e-06, 3.43e-07, 8.21e-07, 5.59e-08],
    'o33a1-100': [8.56e-07, 2.75e-06, 1.04e-06, 1.71e-06, 1.64e-06, 2.09e-06, 8.08e-07, 1.65e-06, 6.45e-07, 2.08e-06, 5.29e-07, 1.65e-06, 3.4e-07, 1.11e-05, 3.9e-06, 8.18e-06, 6.03e-07, 2.37e-06, 5.62e-07],
    'o64a16-17': [2.3e-05, 9.42e-06, 4.25e-06, 8.28e-06, 3.8e-06, 7.36e-07, 3.22e-07, 4.68e-07, 1.45e-07, 7.36e-07, 4.13e-07, 5.22e-07, 4.03e-07, 2.77e-05, 6.88e-06, 8.68e-07, 1.49e-08, 1.56e-06, 1.73e-07],
    'o64a16-100': [4.47e-05, 4.08e-05, 1.39e-05, 3.12e-05, 1.4e-05, 1.84e-06, 8.67e-07, 1.68e-06, 8.66e-07, 1.53e-06, 7.18e-07, 2.08e-06, 4.36e-07, 7.36e-05, 3.57e-05, 3.32e-06, 6.22e-07, 3.13e-06, 1.55e-06],
    'o65a1-17': [5.18e-07, 1.51e-06, 3.34e-07, 8.09e-07, 5.41e-07, 4.99e-07, 3.25e-07, 3.58e-07, 3.52e-07, 7.32e-07, 3.09e-07, 6.46e-07, 3.22e-07, 2.64e-06, 1.11e-06, 1.62e-06, 5.96e-08, 1.16e-06, 3.99e-07],
    'o65a1-100': [5.07e-06, 3.44e-06, 1.43e-06, 2.22e-06, 1.22e-06, 1.86e-06, 1.33e-06, 1.73e-06, 7.14e-07, 2.04e-06, 8.97e-07, 1.05e-06, 7.92e-07, 1.5e-05, 5.3e-06, 4.39e-06, 2.14e-07, 3.46e-06, 9.46e-07],
    'o128a16-17': [1.8e-05, 1.34e-05, 7.27e-06, 9.63e-06, 5.12e-06, 6.14e-07, 3.71e-07, 4.67e-07, 4.14e-07, 1.67e-06, 8.45e-07, 1.04e-06, 2.68e-07, 3.59e-05, 1.72e-05, 1.28e-06, 4.37e-07, 1.94e-06, 5.96e-08],
    'o128a16-100': [4.62e-05, 3.62e-05, 1.6e-05, 2.9e-05, 1.6e-05, 2.24e-06, 6.8e-07, 2.1e-06, 9.24e-07, 1.73e-06, 7.6e-07, 1.4e-06, 7.27e-07, 9.96e-05, 4.74e-05, 5.67e-06, 2.38e-07, 4.13e-06, 4.8e-07],
    'cost-h20-1': [3.22e-08, 5.11e-09, 8.86e-08, 1.7e-08],
    'cost-h20-63': [1.85e-07, 4.33e-08, 5.14e-07, 4.17e-09],
    'cost-h20-64': [1.74e-07, 3.19e-08, 9.02e-07, 3.99e-07],
    'cost-h20-65': [2.44e-07, 6.49e-08, 7.22e-07, 1.19e-07],
    'cost-h20-257': [6.48e-07, 8.56e-08, 2.94e-06, 3.48e-07],
    'cost-h64-1': [2.68e-08, 5.52e-09, 2.43e-08, 2.94e-09, 1.08e-07, 1.57e-08],
    'cost-h64-63': [1.17e-07, 1.5e-08, 7.3e-08, 2.62e-08, 4.94e-07, 1.35e-07],
    'cost-h64-64': [6.74e-08, 1.94e-08, 7.78e-08, 2.33e-08, 2.74e-07, 2.01e-07],
    'cost-h64-65': [6.51e-08, 2.12e-08, 7.1e-08, 2.58e-08, 3.74e-07, 1.32e-07],
    'cost-h64-257': [2.28e-07, 3.23e-08, 2.56e-07, 6.32e-08, 6.27e-07, 5.57e-07],
    'cost-ant-1': [8.47e-09, 1.49e-09, 1.17e-08, 1.55e-09, 4.09e-08, 1.79e-09],
    'cost-ant-63': [2.41e-07, 1.23e-08, 1.55e-07, 3.15e-08, 4.22e-07, 9.41e-08],
    'cost-ant-64': [2.13e-07, 2.1e-08, 1.48e-07, 2.88e-08, 5.81e-07, 7.49e-08],
    'cost-ant-65': [1.58e-07, 2.95e-08, 1.7e-07, 4.35e-08, 7.01e-07, 1.68e-08],
    'cost-ant-257': [4.69e-07, 3.62e-08, 3.58e-07, 8.2e-08, 8.24e-07, 4.34e-08],
    'cost-point-1': [9.33e-09, 2.96e-09, 1.47e-08, 3.85e-09, 3.28e-08, 1.98e-08],
    'cost-point-63': [4.98e-08, 1.57e-08, 8.34e-08, 2.69e-08, 3.61e-07, 1.52e-07],
    'cost-point-64': [4.64e-08, 9.65e-09, 5.1e-08, 1.91e-08, 4.8e-07, 8.35e-08],
    'cost-point-65': [2.05e-08, 1.88e-08, 8.6e-08, 3.71e-08, 2.77e-07, 5.87e-07],
    'cost-point-257': [2.37e-07, 2.59e-08, 6e-07, 1.03e-07, 6.63e-07, 7.95e-08],
    'cost-h20-1025': [1.14e-06, 1.53e-07, 1.9e-06, 3e-07],
    'cost-h20-2064': [2.01e-06, 3.12e-07, 4.01e-06, 1.39e-06],
    'cost-ant-1025': [5.5e-07, 1.21e-07, 6.43e-07, 1.53e-07, 2.71e-06, 2.64e-07],
    'cost-ant-2064': [9.24e-07, 9.6e-08, 1.02e-06, 2.9e-07, 3.69e-06, 1.37e-06],
    'loss-policy': [1.97e-05, 1.28e-05, 5.84e-06, 1.31e-05, 3.96e-06, 2.22e-08, 1.18e-08, 2.21e-08, 1.39e-08, 5.94e-09, 1.58e-09, 4.05e-09, 2.72e-09, 3.26e-05, 3.98e-06, 7.16e-08, 3.73e-08, 8.47e-09, 2.38e-09],
    'loss-zeta': [2.42e-09, 9.37e-10, 8.61e-09, 5.61e-09, 4.79e-08, 4.26e-08],
}
# cost-h20-1: seed 0, min |z| = 0.0817
# cost-h20-63: seed 0, min |z| = 0.000526
# cost-h20-64: seed 0, min |z| = 0.000526
# cost-h20-65: seed 0, min |z| = 0.000526
# cost-h20-257: seed 0, min |z| = 5.47e-05
# cost-h64-1: seed 0, min |z| = 0.00893
# cost-h64-63: seed 0, min |z| = 6.22e-05
# cost-h64-64: seed 0, min |z| = 6.22e-05
# cost-h64-65: seed 0, min |z| = 6.22e-05
# cost-h64-257: seed 0, min |z| = 5.53e-05
# cost-ant-1: seed 0, min |z| = 0.00284
# cost-ant-63: seed 0, min |z| = 9.3e-05
# cost-ant-64: seed 0, min |z| = 9.3e-05
# cost-ant-65: seed 0, min |z| = 9.3e-05
# cost-ant-257: seed 2, min |z| = 4.43e-05
# cost-point-1: seed 0, min |z| = 0.0128
# cost-point-63: seed 0, min |z| = 0.000258
# cost-point-64: seed 0, min |z| = 0.000258
# cost-point-65: seed 0, min |z| = 0.000258
# cost-point-257: seed 0, min |z| = 9.38e-05
# cost-h20-1025: seed 0, min |z| = 5.47e-05
# cost-h20-2064: seed 0, min |z| = 4.21e-05
# cost-ant-1025: seed 3, min |z| = 1.01e-05
# cost-ant-2064: seed 18, min |z| = 1.07e-05
# DEV32_END


if __name__ == "__main__":
    print("DEV32 = {")
    for s, n in POLICY_CASES:
        print(f"    {case_id(s, n)!r}: [" + ", ".join(f"{d:.3g}" for d in policy_dev32(s, n)) + "],")
    for s, n in COST_CASES:
        print(f"    {'cost-' + case_id(s, n)!r}: [" + ", ".join(f"{d:.3g}" for d in cost_dev32(s, n)) + "],")
    lp, lz = loss_dev32()
    print("    'loss-policy': [" + ", ".join(f"{d:.3g}" for d in lp) + "],")
    print("    'loss-zeta': [" + ", ".join(f"{d:.3g}" for d in lz) + "],")
    print("}")
    for s, n in COST_CASES:
        c = cost_case(s, n)
        print(f"# cost-{case_id(s, n)}: seed {c['seed']}, min |z| = {c['zmin']:.3g}")
