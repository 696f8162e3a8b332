"""What the input gradients cost: microseconds per forward + backward call of a loss on the networks' outputs, one process,
one GPU, at the policy shapes (obs 18, act 6, N 64) and (obs 113, act 8, N 128) and for a [64, 64] constraint net on 18 + 6 inputs at N = 20 000, in
three forms:

  (a) in        torch_ops.evaluate_actions / torch_ops.zeta with input_grads=True, obs and actions (obs and acs) requiring grad
                (icrl_policy_fwd_bwd_in; icrl_cost_mlp_fwd_bwd_in + icrl_cn_prepare_bwd)
  (b) parent    the same call without input gradients (icrl_policy_fwd_bwd / icrl_cost_mlp_fwd_bwd): (a) - (b) is what the addition costs
  (c) torch     the same networks as torch modules under autograd on the device, inputs requiring grad (the generic route)

Each figure is the wall time of --iters back-to-back calls between two device synchronisations, divided by their number, after --warmup calls;
the three forms are interleaved, --runs times.  One JSON line per run and one with the medians.
usage: python tools/input_grad_bench.py [--iters 200] [--warmup 20] [--runs 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(fn, iters, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / iters


def _mlp(torch, sizes, act):
    layers = []
    for a, b in zip(sizes[:-1], sizes[1:]):
        layers += [torch.nn.Linear(a, b), act()]
    return torch.nn.Sequential(*layers[:-1]).cuda()


def policy_forms(obs_dim, act_dim, n):
    import torch
    from icrl_amd import spaces, torch_ops as T
    from icrl_amd.policies import ActorTwoCriticsPolicy
    pol = ActorTwoCriticsPolicy(spaces.Box(-np.inf, np.inf, (obs_dim,), np.float64), spaces.Box(-1, 1, (act_dim,), np.float32))
    rng = np.random.RandomState(0)
    obs = torch.as_tensor(rng.randn(n, obs_dim).astype(np.float32)).cuda()
    act = torch.as_tensor(rng.randn(n, act_dim).astype(np.float32)).cuda()
    obs_g, act_g = obs.clone().requires_grad_(True), act.clone().requires_grad_(True)
    leaf = T.leaf(pol)

    def loss(v_r, v_c, lp, ent):
        return lp.sum() + (v_r ** 2).mean() + v_c.mean() - 0.01 * ent.mean()

    def run_in():
        leaf.grad = obs_g.grad = act_g.grad = None
        loss(*T.evaluate_actions(pol, obs_g, act_g, input_grads=True)).backward()

    def run_parent():
        leaf.grad = None
        loss(*T.evaluate_actions(pol, obs, act)).backward()

    nets = [_mlp(torch, [obs_dim, 64, 64, 64], torch.nn.Tanh) for _ in range(3)]      # (_mlp puts no activation after its last layer: run_torch applies it)
    heads = [torch.nn.Linear(64, act_dim).cuda(), torch.nn.Linear(64, 1).cuda(), torch.nn.Linear(64, 1).cuda()]
    log_std = torch.zeros(act_dim, device="cuda", requires_grad=True)
    params = [p for m in nets + heads for p in m.parameters()] + [log_std]

    def run_torch():
        for p in params + [obs_g, act_g]:
            p.grad = None
        lat = [torch.tanh(m(obs_g)) for m in nets]
        mean, v_r, v_c = heads[0](lat[0]), heads[1](lat[1]).flatten(), heads[2](lat[2]).flatten()
        dist = torch.distributions.Normal(mean, torch.ones_like(mean) * log_std.exp())
        loss(v_r, v_c, dist.log_prob(act_g).sum(dim=1), dist.entropy().sum(dim=1)).backward()

    return dict(in_us=run_in, parent_us=run_parent, torch_us=run_torch)


def cost_forms(n):
    import torch
    from icrl_amd import torch_ops as T
    from icrl_amd.constraint_net import ConstraintNet
    lo = -np.ones(6, np.float32)
    torch.manual_seed(0)
    cn = ConstraintNet(18, 6, [64, 64], None, lambda x: 0.05, None, None, False, 0.5, clip_obs=10.0, action_low=lo, action_high=-lo)
    rng = np.random.RandomState(0)
    obs = torch.as_tensor(2.0 * rng.randn(n, 18)).cuda()
    acs = torch.as_tensor(rng.randn(n, 6).astype(np.float32)).cuda()
    obs_g, acs_g = obs.clone().requires_grad_(True), acs.clone().requires_grad_(True)
    leaf = T.leaf(cn)

    def run_in():
        leaf.grad = obs_g.grad = acs_g.grad = None
        (-torch.log(T.zeta(cn, obs_g, acs_g, input_grads=True) + 1e-5)).mean().backward()

    def run_parent():
        leaf.grad = None
        (-torch.log(T.zeta(cn, obs, acs) + 1e-5)).mean().backward()

    net = _mlp(torch, [cn.input_dims, 64, 64, 1], torch.nn.ReLU)
    sel = torch.as_tensor(np.asarray(cn.select_dim, np.int64)).cuda()
    low, high = torch.as_tensor(lo).cuda(), torch.as_tensor(-lo).cuda()

    def run_torch():
        for p in list(net.parameters()) + [obs_g, acs_g]:
            p.grad = None
        x = torch.cat([torch.clamp(obs_g, -10.0, 10.0), torch.clamp(acs_g, low, high).double()], dim=-1)[:, sel].float()
        (-torch.log(torch.sigmoid(net(x)).flatten() + 1e-5)).mean().backward()

    return dict(in_us=run_in, parent_us=run_parent, torch_us=run_torch)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    cases = [("policy obs 18 act 6 N 64", policy_forms(18, 6, 64)), ("policy obs 113 act 8 N 128", policy_forms(113, 8, 128)),
             ("constraint net [64, 64] N 20000", cost_forms(20000))]
    rows = []
    for name, forms in cases:
        runs = []
        for run in range(args.runs):      # interleaved: in, parent, torch, in, parent, torch, ...
            row = {k: round(_time(fn, args.iters, args.warmup), 1) for k, fn in forms.items()}
            print(json.dumps(dict(case=name, run=run + 1, **row)), flush=True)
            runs.append(row)
        med = {k: float(np.median([r[k] for r in runs])) for k in runs[0]}
        med["in_minus_parent_us"] = round(med["in_us"] - med["parent_us"], 1)
        print(json.dumps(dict(case=name, median=True, iters=args.iters, **med)), flush=True)
        rows.append((name, med))
    return rows


if __name__ == "__main__":
    main()
