"""Record tests/golden/g27_cost_shaping.npz by driving the REFERENCE's own CostShapingCallback (build machine only).

    python tools/gen_cost_shaping_golden.py --reference <checkout of the reference>

icrl/exploration.py is imported unmodified under the stand-ins of tools/gen_exploration_golden.py.  `_on_rollout_end` of
CostShapingCallback(use_nn_for_shaping=True) runs on a stub model (buffer arrays, logger) and a stub env (unnormalize_obs with fixed
statistics) for three consecutive rollouts per case, so Adam runs beyond its first step.  Only arrays are written; the planes and statistics
are not stored but regenerated from seeds (tests/helpers/cost_shaping_cases).

The reference's predict_cost casts its input with `.float()`, so its modules cannot run after `.double()`.  The float64 reference is the
helper's torch restatement of the rollout end (twin_rollout_end) in float64; the twin is pinned by requiring its FLOAT32 form to reproduce what
the reference's callback computed — parameters, both Adam moments, the shaped costs, the rewards plane and the five logged scalars.  The
distance is printed per case and must be 0: both run the same torch kernels on the same tensors in the same order, so nothing (not even one
float32 ulp for another kernel selection) is allowed.  A float64 result is stored as its float32 distance from the float32 one (`_d64`
next to `_32`), as g25 does.

Cap conditions (another seed is taken when one fails):
  * cases a and b: each class holds at least a quarter of the rows of every rollout; case c: every target is 0;
  * every pre- and post-step prediction, in both precisions, lies in [1e-4, 1 - 1e-4]: the log's error amplification stays bounded and no
    clamp of the BCE is active;
  * the logged min and max of the shaped cost are single float32 values, one float32 step apart from their neighbours: the two precisions
    differ there by at least a quarter of that step, so that the tests' bound (4 x that distance) is not below one step, which no float32
    result other than the reference's own bits could meet;
  * max |params32 - params64| <= 1e-3 * lr after every step: no Adam sign flip at a near-zero gradient inflates the tolerance the tests
    derive from the two precisions (g25's condition).
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from helpers import cost_shaping_cases as S  # noqa: E402
from gen_exploration_golden import _Logger, _Model, load_reference  # noqa: E402


def caps_hold(case, true, p_all, p32, p64):
    frac = float(np.mean(true))
    if case == "c":
        if frac != 0.0:
            return False
    elif not 0.25 <= frac <= 0.75:
        return False
    if not all(np.all((p >= S.P_LO) & (p <= S.P_HI)) for p in p_all):
        return False
    return float(np.max(np.abs(p32.astype(np.float64) - p64))) <= 1e-3 * S.LR


def run_case(E, name, seed):
    """-> (dict of arrays, distance of the float32 twin from the reference), or None when a cap condition fails."""
    obs, act, T, N, hidden = S.CASES[name]
    thr = S.threshold(seed, name)
    mean, var = S.statistics(seed, obs)
    torch.manual_seed(seed)
    cb = E.CostShapingCallback(S.wall(thr), obs, act, True, cost_net_hidden_layers=list(hidden))
    cb.model, cb.logger = _Model(), _Logger()
    cb.training_env = types.SimpleNamespace(unnormalize_obs=lambda o: S.unnormalize(o, mean, var))
    cb._init_callback()
    init = {k: v.clone() for k, v in cb.cost_net.state_dict().items()}
    shaped_seen = []
    inner = cb.get_shaped_cost
    cb.get_shaped_cost = lambda o, a: shaped_seen.append(inner(o, a)) or shaped_seen[-1]      # (an instance attribute: the class is untouched)
    twins = {}
    for dtype in (torch.float32, torch.float64):
        net = S.make_net(obs + act, hidden, init, dtype)
        twins[dtype] = (net, torch.optim.Adam(net.parameters(), lr=S.LR))
    out = {f"{name}_seed": np.asarray(seed, dtype=np.int64), f"{name}_hidden": np.asarray(hidden, dtype=np.int64),
           f"{name}_threshold": np.asarray(thr, dtype=np.float64)}
    for k, v in init.items():
        out[f"{name}_init_{k}"] = v.numpy().copy()
    dist = 0.0

    def put(key, v32, v64):
        v32, v64 = np.asarray(v32).astype(np.float32), np.asarray(v64, dtype=np.float64)      # (a logged scalar is a Python float: stored as float32)
        out[f"{name}_{key}_32"] = v32
        out[f"{name}_{key}_d64"] = (v64 - v32.astype(np.float64)).astype(np.float32)

    def far(a, b):
        return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))))

    for r in range(S.ROLLOUTS):
        pl, raw, true = S.case_inputs(seed, name, r)
        rb = cb.model.rollout_buffer
        for k, v in pl.items():
            setattr(rb, k, v.copy())
        cb._on_rollout_end()
        ref = dict(shaped=shaped_seen[-1].reshape(T, N), rewards=rb.rewards.copy(), log=np.asarray([cb.logger.values[k] for k in S.LOG_KEYS]),
                   params=S.flat(cb.cost_net), exp_avg=S.adam_flat(cb.cost_net_optim, cb.cost_net, "exp_avg"),
                   exp_avg_sq=S.adam_flat(cb.cost_net_optim, cb.cost_net, "exp_avg_sq"))
        t = {}
        for dtype, (net, opt) in twins.items():
            t[dtype] = S.twin_rollout_end(net, opt, raw, pl["actions"], pl["rewards"], true, dtype)
            t[dtype].update(params=S.flat(net), exp_avg=S.adam_flat(opt, net, "exp_avg"), exp_avg_sq=S.adam_flat(opt, net, "exp_avg_sq"))
        t32, t64 = t[torch.float32], t[torch.float64]
        dist = max([dist] + [far(ref[k], t32[k]) for k in ref])
        p_all = [t32["p_pre"], t64["p_pre"], np.exp(t32["shaped"].astype(np.float64)), np.exp(t64["shaped"])]
        if not caps_hold(name, true, p_all, t32["params"], t64["params"]):
            return None
        for j in (2, 3):      # min and max of shaped: float32 values, so a bound below one float32 step could be met by ref32's own bits only
            if 4.0 * abs(float(ref["log"][j]) - float(t64["log"][j])) < float(np.spacing(np.float32(abs(ref["log"][j])))):
                return None
        for k in ("shaped", "rewards", "log", "params") + (("exp_avg", "exp_avg_sq") if r == S.ROLLOUTS - 1 else ()):      # (the moments: the last step's)
            put(f"{k}_r{r}", ref[k], t64[k])
        put(f"p_pre_r{r}", t32["p_pre"], t64["p_pre"])
    return out, dist


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=S.GOLDEN)
    args = ap.parse_args()
    torch.set_num_threads(1)
    E = load_reference(args.reference)
    arrays = {}
    for i, name in enumerate(S.CASES):
        for seed in range(2700 + 100 * i, 2700 + 100 * i + 50):
            got = run_case(E, name, seed)
            if got is not None:
                arrays.update(got[0])
                print(f"case {name}: seed {seed}; max |float32 twin - reference| over parameters, moments, shaped, rewards and scalars = {got[1]:.3e}")
                assert got[1] == 0.0, "the float32 twin must reproduce the reference bit for bit"
                break
        else:
            raise SystemExit(f"case {name}: no seed satisfies the cap conditions")
    np.savez_compressed(args.out, **arrays)
    size = os.path.getsize(args.out)
    print(f"{args.out}: {len(arrays)} arrays, {size} bytes")
    assert size < 1000 * 1000, "the fixture must stay under 1 MB"


if __name__ == "__main__":
    main()
