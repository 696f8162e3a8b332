"""Microseconds per optimiser step of the fine-grained update loop in its two forms:

  (a) torch   the networks as torch tensors on the GPU with autograd: icrl_minibatch_gather, the torch forward, icrl_ppo_lag_loss_fwd_bwd,
              torch.autograd.backward into a flat gradient buffer, icrl_clip_adam_step — what section 3a prescribes without torch_ops;
  (b) fused   the same loop with icrl_amd.torch_ops.evaluate_actions (icrl_policy_fwd_bwd, csrc/mlp_grad.hip) in place of the torch networks.

Shapes: BASELINE configs[1] (obs 18, act 6, batch 64) and configs[2] (obs 113, act 8, batch 128).  Per run: --steps optimiser steps after --warmup
steps, one synchronisation at each end, host clock around it.  --runs runs per form, interleaved (a, b, a, b, ...).  Needs the GPU.

    python tools/fine_grained_bench.py [--steps 200 --warmup 20 --runs 3] [--out profiles/mlp_grad_bench.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from icrl_amd import _lib, spaces, structs as S, torch_ops      # noqa: E402
from icrl_amd.buffers import RolloutBufferWithCost              # noqa: E402
from icrl_amd.policies import ActorTwoCriticsPolicy             # noqa: E402

SHAPES = (("configs[1] obs 18 act 6 batch 64", 18, 6, 64), ("configs[2] obs 113 act 8 batch 128", 113, 8, 128))
P = _lib.ptr


class TorchPolicy:
    """the two-critics MLP policy as autograd leaves that VIEW one flat parameter buffer (the layout of ActorTwoCriticsPolicy.params), their
    .grad viewing one flat gradient buffer: what icrl_clip_adam_step steps."""

    def __init__(self, flat, flat_grad, shapes):
        self.leaves, off = {}, 0
        for k, shp in shapes.items():
            n = int(np.prod(shp))
            t = flat[off:off + n].view(shp).requires_grad_(True)
            t.grad = flat_grad[off:off + n].view(shp)
            self.leaves[k], off = t, off + n

    def evaluate_actions(self, obs, actions):      # policies.py:752-767 with DiagGaussianDistribution (distributions.py:114-192)
        w = self.leaves
        lat = []
        for b in ("policy_net", "value_net", "cost_value_net"):
            h = torch.tanh(F.linear(obs, w[f"mlp_extractor.{b}.0.weight"], w[f"mlp_extractor.{b}.0.bias"]))
            lat.append(torch.tanh(F.linear(h, w[f"mlp_extractor.{b}.2.weight"], w[f"mlp_extractor.{b}.2.bias"])))
        mean = F.linear(lat[0], w["action_net.weight"], w["action_net.bias"])
        dist = torch.distributions.Normal(mean, torch.ones_like(mean) * w["log_std"].exp(), validate_args=False)
        v_r = F.linear(lat[1], w["value_net.weight"], w["value_net.bias"]).flatten()
        v_c = F.linear(lat[2], w["cost_value_net.weight"], w["cost_value_net.bias"]).flatten()
        return v_r, v_c, dist.log_prob(actions).sum(dim=1), dist.entropy().sum(dim=1)


class Loop:
    def __init__(self, obs_dim, act_dim, batch, seed=0):
        torch.manual_seed(seed)
        rng = np.random.RandomState(seed)
        self.L, self.B = _lib.lib(), batch
        T, n_envs = 64, 32
        self.rb = RolloutBufferWithCost(T, spaces.Box(-np.inf, np.inf, (obs_dim,), np.float64), spaces.Box(-1, 1, (act_dim,), np.float32), "cuda", n_envs=n_envs)
        for k in ("observations", "actions", "log_probs", "reward_advantages", "cost_advantages", "reward_returns", "cost_returns", "reward_values", "cost_values"):
            t = getattr(self.rb, k)
            t.copy_(torch.as_tensor((rng.randn(*t.shape) * (0.3 if k == "log_probs" else 1.0) - (8.0 if k == "log_probs" else 0.0)).astype(np.float32)))
        self.buf = self.rb.struct()
        self.idx = torch.as_tensor(np.stack([rng.permutation(T * n_envs)[:batch] for _ in range(64)]).astype(np.int32)).cuda().contiguous()
        self.policy = ActorTwoCriticsPolicy(spaces.Box(-np.inf, np.inf, (obs_dim,), np.float64), spaces.Box(-1, 1, (act_dim,), np.float32))
        # old log-probs of the policy itself (ratio 1 at the first step, as after a rollout), so that the timed steps are finite arithmetic
        with torch.no_grad():
            lp = self.policy.evaluate_actions(self.rb.observations.reshape(-1, obs_dim).double(), self.rb.actions.reshape(-1, act_dim))[2]
            self.rb.log_probs.copy_(lp.reshape(self.rb.log_probs.shape))
        self.params0 = self.policy.params.clone()
        n = self.policy.n_params
        dev = dict(device="cuda")
        self.flat_grad = torch.zeros(n, **dev)
        self.torch_policy = TorchPolicy(self.policy.params, self.flat_grad, self.policy.shapes)
        self.m, self.v, self.step = torch.zeros(n, **dev), torch.zeros(n, **dev), torch.zeros(1, dtype=torch.int32, **dev)
        self.work, self.out2, self.terms = torch.zeros(256, **dev), torch.zeros(2, **dev), torch.zeros(8, **dev)
        self.nu = torch.full((1,), 0.5, **dev)
        self.obs, self.act = torch.empty(batch, obs_dim, **dev), torch.empty(batch, act_dim, **dev)
        self.rows = {k: torch.empty(batch, **dev) for k in ("old_lp", "adv_r", "adv_c", "ret_r", "ret_c", "old_vr", "old_vc", "d_lp", "d_vr", "d_vc", "d_ent")}
        hp = S.PpoHyperT(batch, 1, 0, 0)
        hp.clip_range, hp.ent_coef, hp.reward_vf_coef, hp.cost_vf_coef, hp.max_grad_norm = 0.2, 0.0, 0.5, 0.5, 0.5
        hp.clip_range_reward_vf = hp.clip_range_cost_vf = -1.0
        hp.lr, hp.adam_beta1, hp.adam_beta2, hp.adam_eps = 3e-5, 0.9, 0.999, 1e-5
        self.hp = hp

    def reset(self):
        self.policy.params.copy_(self.params0)
        self.m.zero_(); self.v.zero_(); self.step.zero_()

    def one_step(self, i, fused):
        L, r, B, st = self.L, self.rows, self.B, _lib.current_stream()
        _lib.check(L.icrl_minibatch_gather(ctypes.byref(self.buf), self.idx[i % 64].data_ptr(), B, P(self.obs), P(self.act), P(r["old_lp"]), P(r["adv_r"]),
                                           P(r["adv_c"]), P(r["ret_r"]), P(r["ret_c"]), P(r["old_vr"]), P(r["old_vc"]), st), "icrl_minibatch_gather")
        if fused:
            leaf = torch_ops.leaf(self.policy)
            leaf.grad = None
            v_r, v_c, lp, ent = torch_ops.evaluate_actions(self.policy, self.obs, self.act)
        else:
            self.flat_grad.zero_()                                          # optimizer.zero_grad()
            v_r, v_c, lp, ent = self.torch_policy.evaluate_actions(self.obs, self.act)
        _lib.check(L.icrl_ppo_lag_loss_fwd_bwd(lp.data_ptr(), P(r["old_lp"]), P(r["adv_r"]), P(r["adv_c"]), v_r.data_ptr(), v_c.data_ptr(), P(r["ret_r"]),
                                               P(r["ret_c"]), None, None, ent.data_ptr(), P(self.nu), ctypes.byref(self.hp), B, P(self.terms), P(r["d_lp"]),
                                               P(r["d_vr"]), P(r["d_vc"]), P(r["d_ent"]), st), "icrl_ppo_lag_loss_fwd_bwd")
        torch.autograd.backward([lp, v_r, v_c, ent], [r["d_lp"], r["d_vr"], r["d_vc"], r["d_ent"]])
        grad = torch_ops.leaf(self.policy).grad if fused else self.flat_grad
        _lib.check(L.icrl_clip_adam_step(P(self.policy.params), P(grad), P(self.m), P(self.v), P(self.step), grad.numel(), ctypes.byref(self.hp), P(self.work),
                                         P(self.out2), st), "icrl_clip_adam_step")

    def run(self, fused, steps, warmup):
        self.reset()
        for i in range(warmup):
            self.one_step(i, fused)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(warmup, warmup + steps):
            self.one_step(i, fused)
        torch.cuda.synchronize()
        return 1e6 * (time.perf_counter() - t0) / max(steps, 1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None, help="write the result as JSON to this file as well")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fine_grained_bench needs the GPU: a time measured elsewhere says nothing about it")
    result = dict(steps=a.steps, warmup=a.warmup, runs=a.runs, shapes=[])
    for name, obs_dim, act_dim, batch in SHAPES:
        loop = Loop(obs_dim, act_dim, batch)
        # the two forms take the same optimiser steps: parameters after `warmup` steps agree to float32 rounding
        loop.run(False, 0, a.warmup); pa = loop.policy.params.clone()
        loop.run(True, 0, a.warmup); pb = loop.policy.params.clone()
        agree = float((pa - pb).abs().max())
        us = dict(torch=[], fused=[])
        for _ in range(a.runs):
            us["torch"].append(round(loop.run(False, a.steps, a.warmup), 1))
            us["fused"].append(round(loop.run(True, a.steps, a.warmup), 1))
        result["shapes"].append(dict(shape=name, us_per_step_torch=us["torch"], us_per_step_fused=us["fused"], max_param_diff_after_warmup=agree))
        print(f"{name}: (a) torch networks {us['torch']} us per optimiser step, (b) torch_ops.evaluate_actions {us['fused']} us "
              f"(parameters of the two forms after {a.warmup} steps differ by at most {agree:.3g})", flush=True)
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
