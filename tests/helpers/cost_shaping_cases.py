"""Shared by tools/gen_cost_shaping_golden.py and the cost-shaping tests: the cases of tests/golden/g27_cost_shaping.npz, the buffer planes
and normaliser statistics they regenerate from seeds, and a torch restatement ("the twin") of the rollout-end work of the reference's
CostShapingCallback (icrl/exploration.py:148-169) in either precision.  The reference's predict_cost casts its input with `.float()`, so its
own modules cannot run after `.double()`: the float64 reference is the twin, and the generator pins the twin by requiring its float32 form
to reproduce the reference's float32 results.  Tolerance rule, check() and the `_32` / `_d64` encoding are those of exploration_cases."""
import os

import numpy as np
import torch

from helpers.exploration_cases import KEYS, LR, ROLLOUTS, adam_flat, check, flat, ref64_of, state_dict_of, tol  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "g27_cost_shaping.npz")
# name -> obs, act, T, N, hidden layers (a: exactly one 32-row group, the reference's widths; b: less than a group, the widest input, odd
# widths; c: many groups and a ragged last one, every target 0 — a wall that is never reached)
CASES = {"a": (18, 6, 8, 4, (50, 50)), "b": (113, 8, 5, 3, (17, 33)), "c": (9, 2, 4099, 1, (50, 50))}
EPSILON = 1e-8                      # VecNormalize's
P_LO, P_HI = 1e-4, 1 - 1e-4         # cap condition on every prediction
LOG_KEYS = ("CostShaping/mean_true_cost", "CostShaping/mean_shaped_cost", "CostShaping/min_shaped_cost", "CostShaping/max_shaped_cost",
            "CostShaping/cost_network_loss")


def planes(seed, rollout, obs, act, T, N):
    """one rollout's buffer planes (float32: normalised observations, stored actions — beyond the clip range too — and rewards) from
    np.random.RandomState(seed + rollout) in a fixed draw order."""
    rs = np.random.RandomState(int(seed) + int(rollout))
    o = np.clip(rs.randn(T, N, obs), -10, 10).astype(np.float32)
    a = (1.5 * np.tanh(rs.randn(T, N, act))).astype(np.float32)
    return dict(observations=o, actions=a, rewards=rs.randn(T, N).astype(np.float32))


def statistics(seed, obs):
    """the normaliser's running moments of a case (float64), fixed over its rollouts."""
    rs = np.random.RandomState(int(seed) + 7919)
    return rs.randn(obs), rs.uniform(0.25, 4.0, obs)


def unnormalize(observations, mean, var):
    """VecNormalize.unnormalize_obs (vec_normalize.py:125-128): float64, product and sum rounded separately."""
    return observations * np.sqrt(var + EPSILON) + mean


def threshold(seed, case):
    """the wall position on raw observation column 0: inside the bulk for a and b, out of reach for c."""
    mean, var = statistics(seed, CASES[case][0])
    if case == "c":
        return float(mean[0] - 100.0 * np.sqrt(var[0]))
    return float(mean[0] + np.sqrt(var[0]) * np.random.RandomState(int(seed) + 104729).uniform(-0.4, 0.4))


def wall(thr):
    """true_constraint_net.wall_behind on column 0, as a plain function of (obs, acs)."""
    return lambda obs, acs: obs[..., 0] <= thr


def make_net(in_dim, hidden, state_dict=None, dtype=torch.float32):
    """create_mlp(in, 1, hidden) + Sigmoid, the Linear layers constructed in the reference's order."""
    dims = [in_dim] + list(hidden) + [1]
    mods = []
    for k in range(3):
        mods.append(torch.nn.Linear(dims[k], dims[k + 1]))
        if k < 2:
            mods.append(torch.nn.ReLU())
    net = torch.nn.Sequential(*mods, torch.nn.Sigmoid())
    if state_dict is not None:
        net.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in state_dict.items()})
    return net.to(dtype)


def twin_rollout_end(net, opt, raw, actions, rewards, true_costs, dtype):
    """steps 4-6 of the callback in `dtype` on raw [T, N, obs] float64, actions [T, N, act], rewards [T, N] float32, true_costs [T, N]:
    the input is the FLOAT32 rounding of the raw row in both precisions (it is part of what is computed, not of how precisely).
    -> dict(loss, p_pre [rows], shaped [T, N], rewards [T, N], log [5])."""
    T, N = rewards.shape
    np_t = np.float32 if dtype == torch.float32 else np.float64
    x = torch.cat((torch.from_numpy(raw.reshape(T * N, -1)), torch.from_numpy(actions.astype(float).reshape(T * N, -1))), axis=-1).float().to(dtype)
    y = torch.from_numpy(true_costs.astype(float).reshape(-1, 1)).float().to(dtype)
    pred = net(x)
    loss = torch.nn.BCELoss()(pred, y)
    opt.zero_grad()
    loss.backward()
    opt.step()
    with np.errstate(divide="ignore"):
        shaped = np.log(net(x).detach().numpy()).reshape(-1, N)
    out = rewards.astype(np_t) + shaped
    log = [np.mean(true_costs.astype(float)), np.mean(shaped), np.min(shaped), np.max(shaped), loss.item()]
    return dict(loss=loss.item(), p_pre=pred.detach().numpy().reshape(-1), shaped=shaped, rewards=out, log=np.asarray(log, dtype=np.float64))


def case_inputs(seed, case, rollout):
    """-> (planes, raw [T, N, obs] float64, true costs [T, N] bool) of one rollout of a fixture case."""
    obs, act, T, N, _ = CASES[case]
    pl = planes(seed, rollout, obs, act, T, N)
    raw = unnormalize(pl["observations"], *statistics(seed, obs))
    return pl, raw, wall(threshold(seed, case))(raw, pl["actions"])


def recompute(g, case, dtype, rollouts=ROLLOUTS):
    """the twin on a fixture case from its stored initial weights: per rollout r the keys loss_r, p_pre_r, shaped_r, rewards_r, log_r,
    params_r, exp_avg_r, exp_avg_sq_r."""
    obs, act, T, N, hidden = CASES[case]
    seed = int(g[f"{case}_seed"])
    net = make_net(obs + act, hidden, state_dict_of(g, f"{case}_init"), dtype)
    opt = torch.optim.Adam(net.parameters(), lr=LR)
    res = {}
    for r in range(rollouts):
        pl, raw, true = case_inputs(seed, case, r)
        for k, v in twin_rollout_end(net, opt, raw, pl["actions"], pl["rewards"], true, dtype).items():
            res[f"{k}_r{r}"] = v
        res[f"params_r{r}"] = flat(net)
        res[f"exp_avg_r{r}"] = adam_flat(opt, net, "exp_avg")
        res[f"exp_avg_sq_r{r}"] = adam_flat(opt, net, "exp_avg_sq")
    return res


def load_golden():
    return np.load(GOLDEN)
