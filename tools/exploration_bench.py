"""Cost of the exploration callbacks' rollout-end work (icrl_amd/exploration.py) on the device; results go to profiles/exploration.md.

    python tools/exploration_bench.py [--reps 30] [--skip_cpg]

1. microseconds per LambdaShapingCallback rollout end (cost-net step, predictor step, advantage shaping, one scalar read) at
   (T 2048, N 64, obs 18, act 6) — the flagship shape — and (2048, 512, 113, 8), on a filled buffer, host wall time between two device
   synchronisations (the callback ends in a device-to-host read, so wall time is what a rollout pays) and device time between two events;
2. the same step written here as torch modules with torch.optim.Adam on the device (the formulation the kernels replace): the same
   planes, torch.cat of observations and actions, MSELoss, backward, Adam, the division, one scalar read;
3. `cpg -tei HCWithPos-v0 -eei HCWithPosTest-v0 -nt 64 --n_steps 2048 -uls` against the same command without the flag, env-steps/s of
   learn() after one warm-up learn() in the same process.
Medians over --reps repetitions after 5 warm-up calls; one JSON line per measurement.

    python tools/exploration_bench.py --cost_shaping [--reps 30]

the rollout end of CostShapingCallback (`gail -ucsc -ucn`) at the same two shapes, kernels against the same callback written as torch modules
on the device, three interleaved runs per form; results go to profiles/cost_shaping.md."""
import argparse
import json
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ((2048, 64, 18, 6), (2048, 512, 113, 8))


def _model(T, N, obs, act):
    from icrl_amd import spaces
    from icrl_amd.buffers import RolloutBufferWithCost
    aspace = spaces.Box(-1.0, 1.0, (act,))
    rb = RolloutBufferWithCost(T, spaces.Box(-np.inf, np.inf, (obs,)), aspace, device="cuda", n_envs=N)
    g = torch.Generator(device="cuda").manual_seed(0)
    for k in ("observations", "new_observations", "actions", "costs", "cost_advantages"):
        getattr(rb, k).copy_(torch.randn(getattr(rb, k).shape, device="cuda", generator=g))
    return types.SimpleNamespace(rollout_buffer=rb, env=types.SimpleNamespace(action_space=aspace), policy=types.SimpleNamespace(discrete=False))


def _time(fn, reps):
    for _ in range(5):
        fn()
    wall, dev = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter(); e0.record()
        fn()
        e1.record(); torch.cuda.synchronize()
        wall.append(1e6 * (time.perf_counter() - t0)); dev.append(1e3 * e0.elapsed_time(e1))
    return dict(wall_us_median=statistics.median(wall), wall_us_min=min(wall), device_us_median=statistics.median(dev), device_us_min=min(dev))


class TorchLambdaShaping:
    """the reference's LambdaShapingCallback._on_rollout_end as torch modules on the device."""

    def __init__(self, obs, act, hidden=(50, 50)):
        def mlp(out):
            dims = [obs + act] + list(hidden) + [out]
            mods = []
            for k in range(3):
                mods += [torch.nn.Linear(dims[k], dims[k + 1])] + ([torch.nn.ReLU()] if k < 2 else [])
            return torch.nn.Sequential(*mods).cuda()
        self.cost_net, self.pred = mlp(1), mlp(obs)
        self.cost_opt, self.pred_opt = torch.optim.Adam(self.cost_net.parameters(), lr=3e-3), torch.optim.Adam(self.pred.parameters(), lr=3e-3)

    def rollout_end(self, rb):
        T, N = rb.buffer_size, rb.n_envs
        x = torch.cat((rb.observations.reshape(T * N, -1), rb.actions.reshape(T * N, -1)), dim=-1)
        cost_loss = torch.nn.functional.mse_loss(self.cost_net(x), rb.costs.reshape(-1, 1))
        self.cost_opt.zero_grad(); cost_loss.backward(); self.cost_opt.step()
        loss = torch.nn.functional.mse_loss(self.pred(x), rb.new_observations.reshape(T * N, -1), reduction="none")
        row_err = loss.detach().sum(dim=-1)
        mean = loss.mean()
        self.pred_opt.zero_grad(); mean.backward(); self.pred_opt.step()
        rb.cost_advantages /= (1 + row_err.view(T, N))
        return torch.stack([row_err.mean(), row_err.std(unbiased=False), mean.detach(), cost_loss.detach()]).cpu()


def bench_callbacks(reps):
    from icrl_amd import logger
    from icrl_amd.exploration import LambdaShapingCallback
    for T, N, obs, act in SHAPES:
        logger.configure()
        model = _model(T, N, obs, act)
        cb = LambdaShapingCallback(obs, act, device="cuda")
        cb.init_callback(model)
        ours = _time(cb.on_rollout_end, reps)
        ref = TorchLambdaShaping(obs, act)
        theirs = _time(lambda: ref.rollout_end(model.rollout_buffer), reps)
        print(json.dumps(dict(what="lambda_shaping_rollout_end", T=T, N=N, obs=obs, act=act, rows=T * N, kernels=ours, torch_modules=theirs,
                              speedup_wall=theirs["wall_us_median"] / ours["wall_us_median"])), flush=True)


class TorchCostShaping:
    """the reference's CostShapingCallback._on_rollout_end (use_nn_for_shaping=True) as torch modules on the device, a wall cost on column 0."""

    def __init__(self, obs, act, threshold, hidden=(50, 50)):
        dims = [obs + act] + list(hidden) + [1]
        mods = []
        for k in range(3):
            mods += [torch.nn.Linear(dims[k], dims[k + 1])] + ([torch.nn.ReLU()] if k < 2 else [])
        self.net = torch.nn.Sequential(*mods, torch.nn.Sigmoid()).cuda()
        self.opt, self.threshold = torch.optim.Adam(self.net.parameters(), lr=3e-3), threshold

    def rollout_end(self, rb, env):
        T, N = rb.buffer_size, rb.n_envs
        raw = rb.observations.double() * torch.sqrt(env.obs_rms.d_var + env.epsilon) + env.obs_rms.d_mean
        true = (raw[..., 0] <= self.threshold).double()
        x = torch.cat((raw.reshape(T * N, -1), rb.actions.double().reshape(T * N, -1)), dim=-1).float()
        loss = torch.nn.functional.binary_cross_entropy(self.net(x), true.reshape(-1, 1).float())
        self.opt.zero_grad(); loss.backward(); self.opt.step()
        with torch.no_grad():
            shaped = torch.log(self.net(x)).view(T, N)
        rb.rewards += shaped
        return torch.stack([true.mean(), shaped.mean().double(), shaped.min().double(), shaped.max().double(), loss.detach().double()]).cpu()


def bench_cost_shaping(reps, runs=3):
    """us per rollout end of CostShapingCallback (-ucsc -ucn), kernels against torch modules: `runs` interleaved runs per form (kernels,
    torch, kernels, torch, ...), each the median over `reps` calls after 5 warm-up calls; the figure of a form is the median of its runs."""
    from icrl_amd import logger
    from icrl_amd.exploration import CostShapingCallback
    from icrl_amd.true_constraint_net import AnalyticCost
    for T, N, obs, act in SHAPES:
        logger.configure()
        model = _model(T, N, obs, act)
        rms = types.SimpleNamespace(d_mean=torch.zeros(obs, dtype=torch.float64, device="cuda"), d_var=torch.ones(obs, dtype=torch.float64, device="cuda"))
        model.env.norm_obs, model.env.obs_rms, model.env.epsilon = True, rms, 1e-8
        cb = CostShapingCallback(AnalyticCost.wall_behind(-0.5), obs, act, True, device="cuda")
        cb.init_callback(model)
        ref = TorchCostShaping(obs, act, -0.5)
        forms = dict(kernels=cb.on_rollout_end, torch_modules=lambda: ref.rollout_end(model.rollout_buffer, model.env))
        got = {k: [] for k in forms}
        for _ in range(runs):
            for k, fn in forms.items():
                model.rollout_buffer.rewards.zero_()
                got[k].append(_time(fn, reps))
        wall = {k: statistics.median(r["wall_us_median"] for r in v) for k, v in got.items()}
        print(json.dumps(dict(what="cost_shaping_rollout_end", T=T, N=N, obs=obs, act=act, rows=T * N, runs=got, wall_us=wall,
                              speedup_wall=wall["torch_modules"] / wall["kernels"])), flush=True)


def bench_cpg(rollouts):
    from icrl_amd import cpg as C
    out = {}
    for name, extra in (("plain", ()), ("uls", ("-uls",))):
        steps = rollouts * 64 * 2048
        cfg = vars(C.build_parser().parse_args(["cpg", "-tei", "HCWithPos-v0", "-eei", "HCWithPosTest-v0", "-nt", "64", "--n_steps", "2048", "-t", str(steps),
                                                "-s", "0", "-v", "0", "--eval_every_rollouts", "1000", *extra]))
        cfg.update(rank=0, world_size=1)
        cfg = types.SimpleNamespace(**cfg)
        model, cb, learn_cost, _ = C.setup(cfg, log=None)
        model.learn(total_timesteps=2 * 64 * 2048, cost_function=learn_cost, callback=cb)      # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.learn(total_timesteps=steps, cost_function=learn_cost, callback=cb)
        torch.cuda.synchronize()
        out[name] = steps / (time.perf_counter() - t0)
    print(json.dumps(dict(what="cpg_env_steps_per_s", envs=64, n_steps=2048, rollouts=rollouts, plain=out["plain"], uls=out["uls"],
                          ratio=out["uls"] / out["plain"])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rollouts", type=int, default=6)
    ap.add_argument("--skip_cpg", action="store_true")
    ap.add_argument("--cost_shaping", action="store_true", help="the cost-shaping callback only (profiles/cost_shaping.md)")
    args = ap.parse_args()
    if args.cost_shaping:
        bench_cost_shaping(args.reps)
        return
    bench_callbacks(args.reps)
    if not args.skip_cpg:
        bench_cpg(args.rollouts)


if __name__ == "__main__":
    main()
