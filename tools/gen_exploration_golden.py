"""Record tests/golden/g25_exploration.npz by driving the REFERENCE's own exploration callbacks (build machine only).

    python tools/gen_exploration_golden.py --reference <checkout of the reference>

icrl/exploration.py is imported unmodified under stand-ins for `gym` and for the stable_baselines3 import chain (a BaseCallback that only
stores `verbose`, and create_mlp as the list Linear, ReLU, Linear, ReLU, Linear).  `_on_rollout_end` of ExplorationRewardCallback and of
LambdaShapingCallback runs on a stub model (buffer arrays, logger) for three consecutive rollouts, so Adam runs beyond its first step; every
case runs twice from the same initial weights: as the reference is (float32 buffers and modules) and with the modules after `.double()` on
float64 copies of the same planes.  Only arrays are written; the planes are not stored but regenerated from seeds
(tests/helpers/exploration_cases.planes).  A float64 result is stored as its float32 distance from the float32 one (`_d64` next to `_32`).

Cap conditions (another seed is taken when one fails): max |params32 - params64| <= 1e-3 * lr after every step — no Adam sign flip at a
near-zero gradient inflates the tolerance the tests derive from the two precisions — and row_err > 0 everywhere.
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import exploration_cases as X  # noqa: E402


def load_reference(ref):
    """icrl/exploration.py of the reference, imported under the stand-ins."""
    names = ("gym", "stable_baselines3", "stable_baselines3.common", "stable_baselines3.common.callbacks", "stable_baselines3.common.torch_layers")
    mods = {n: types.ModuleType(n) for n in names}

    class BaseCallback:
        def __init__(self, verbose=0):
            self.verbose, self.model, self.logger = verbose, None, None

    def create_mlp(input_dim, output_dim, net_arch):
        dims, out = [input_dim] + list(net_arch), []
        for k in range(len(net_arch)):
            out += [torch.nn.Linear(dims[k], dims[k + 1]), torch.nn.ReLU()]
        return out + [torch.nn.Linear(dims[-1], output_dim)]

    mods["stable_baselines3.common.callbacks"].BaseCallback = BaseCallback
    mods["stable_baselines3.common.torch_layers"].create_mlp = create_mlp
    mods["stable_baselines3"].common = mods["stable_baselines3.common"]
    mods["stable_baselines3.common"].callbacks = mods["stable_baselines3.common.callbacks"]
    mods["stable_baselines3.common"].torch_layers = mods["stable_baselines3.common.torch_layers"]
    saved = {n: sys.modules.get(n) for n in names}
    sys.modules.update(mods)
    try:
        spec = importlib.util.spec_from_file_location("ref_exploration", os.path.join(ref, "icrl", "exploration.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for n, m in saved.items():
            if m is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = m
    return mod


class _Logger:
    def __init__(self):
        self.values = {}

    def record(self, key, value):
        self.values[key] = float(value)


class _Model:
    def __init__(self):
        self.rollout_buffer = types.SimpleNamespace()


def _attach(cb):
    cb.model, cb.logger = _Model(), _Logger()
    cb._init_callback()
    return cb


def _fill(cb, pl, dtype):
    for k, v in pl.items():
        setattr(cb.model.rollout_buffer, k, v.astype(dtype).copy())


def _nets(cb):
    return [(n, getattr(cb, n)) for n in ("cost_net", "predictor_network") if hasattr(cb, n)]


def run_case(E, name, seed):
    """-> dict of arrays, or None when a cap condition fails."""
    obs, act, T, N, hidden = X.CASES[name]
    out = {f"{name}_seed": np.asarray(seed, dtype=np.int64), f"{name}_hidden": np.asarray(hidden, dtype=np.int64)}
    for tag in ("e", "l"):
        torch.manual_seed(seed)
        pair = []
        for dtype in (np.float32, np.float64):
            if tag == "e":
                cb = _attach(E.ExplorationRewardCallback(obs, act, hidden_layers=list(hidden)))
            else:
                cb = _attach(E.LambdaShapingCallback(obs, act, cost_net_hidden_layers=list(hidden), predictor_net_hidden_layers=list(hidden)))
            if pair:      # the same initial weights, then .double(): the optimisers keep their parameter objects
                for (_, n32), (_, n64) in zip(pair[0][1], _nets(cb)):
                    n64.load_state_dict(n32)
                    n64.double()
                pair.append((cb, None))
            else:
                pair.append((cb, [(n, {k: v.clone() for k, v in net.state_dict().items()}) for n, net in _nets(cb)]))
                for n, sd in pair[0][1]:
                    short = "cost" if n == "cost_net" else "pred"
                    for k, v in sd.items():
                        out[f"{name}_{tag}_{short}_init_{k}"] = v.numpy().copy()
        cb32, cb64 = pair[0][0], pair[1][0]

        def put(key, v32, v64):
            v32, v64 = np.asarray(v32), np.asarray(v64, dtype=np.float64)
            out[f"{name}_{tag}_{key}_32"] = v32.astype(np.float32)
            out[f"{name}_{tag}_{key}_d64"] = (v64 - v32.astype(np.float64)).astype(np.float32)

        for r in range(X.ROLLOUTS):
            pl = X.planes(seed, r, obs, act, T, N)
            _fill(cb32, pl, np.float32); _fill(cb64, pl, np.float64)
            cb32._on_rollout_end(); cb64._on_rollout_end()
            for (_, n32), (_, n64) in zip(_nets(cb32), _nets(cb64)):
                if np.max(np.abs(X.flat(n32).astype(np.float64) - X.flat(n64))) > 1e-3 * X.LR:
                    return None
            rb32, rb64 = cb32.model.rollout_buffer, cb64.model.rollout_buffer
            if tag == "e":
                put(f"rewards_r{r}", rb32.rewards, rb64.rewards)
                keys = ("exploration/predictor_network_loss",)
                if not np.all(rb64.rewards - pl["rewards"].astype(np.float64) > 0):      # (this callback keeps no copy of its row errors)
                    return None
            else:
                e32, e64 = cb32._exploration_reward, cb64._exploration_reward
                put(f"row_err_r{r}", e32, e64)
                put(f"cost_adv_r{r}", rb32.cost_advantages, rb64.cost_advantages)
                keys = ("exploration/mean_exploration_reward", "exploration/std_exploration_reward", "exploration/predictor_network_loss",
                        "exploration/cost_network_loss")
                if not (np.all(e32 > 0) and np.all(e64 > 0)):
                    return None
            put(f"log_r{r}", [cb32.logger.values[k] for k in keys], [cb64.logger.values[k] for k in keys])
        for (n, n32), (_, n64) in zip(_nets(cb32), _nets(cb64)):
            put("cost_params" if n == "cost_net" else "pred_params", X.flat(n32), X.flat(n64))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=X.GOLDEN)
    args = ap.parse_args()
    torch.set_num_threads(1)
    E = load_reference(args.reference)
    arrays = {}
    for i, name in enumerate(X.CASES):
        for seed in range(2500 + 100 * i, 2500 + 100 * i + 50):
            got = run_case(E, name, seed)
            if got is not None:
                arrays.update(got)
                print(f"case {name}: seed {seed}")
                break
        else:
            raise SystemExit(f"case {name}: no seed satisfies the cap conditions")
    np.savez_compressed(args.out, **arrays)
    size = os.path.getsize(args.out)
    print(f"{args.out}: {len(arrays)} arrays, {size} bytes")
    assert size < 1000 * 1000, "the fixture must stay under 1 MB"


if __name__ == "__main__":
    main()
