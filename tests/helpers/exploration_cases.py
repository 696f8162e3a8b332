"""Shared by tools/gen_exploration_golden.py and the exploration tests: the cases of tests/golden/g25_exploration.npz, the buffer planes
they regenerate from seeds, a torch recomputation of the reference's rollout-end step in either precision, and the tolerance rule."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "g25_exploration.npz")
LR = 3e-3
ROLLOUTS = 3
# name -> obs, act, T, N, hidden layers (a: the reference's default widths, two full row tiles; b: less than one tile, the widest input, odd
# widths with h1 != h2; c: many workgroups and a ragged tail)
CASES = {"a": (18, 6, 8, 4, (50, 50)), "b": (113, 8, 5, 3, (17, 33)), "c": (9, 2, 4099, 1, (50, 50))}
KEYS = ("0.weight", "0.bias", "2.weight", "2.bias", "4.weight", "4.bias")


def planes(seed, rollout, obs, act, T, N):
    """the buffer planes of one rollout, float32, from np.random.RandomState(seed + rollout) in a fixed draw order."""
    rs = np.random.RandomState(int(seed) + int(rollout))
    o = rs.randn(T, N, obs).astype(np.float32)
    a = np.tanh(rs.randn(T, N, act)).astype(np.float32)
    w = (rs.randn(obs + act, obs) / np.sqrt(obs + act)).astype(np.float32)
    nxt = (np.concatenate([o, a], -1) @ w + 0.1 * rs.randn(T, N, obs)).astype(np.float32)
    return dict(observations=o, actions=a, new_observations=nxt, rewards=rs.randn(T, N).astype(np.float32),
                costs=(rs.rand(T, N) < 0.3).astype(np.float32), cost_advantages=rs.randn(T, N).astype(np.float32))


def make_net(in_dim, out_dim, hidden, state_dict=None, dtype=torch.float32):
    dims = [in_dim] + list(hidden) + [out_dim]
    mods = []
    for k in range(3):
        mods.append(torch.nn.Linear(dims[k], dims[k + 1]))
        if k < 2:
            mods.append(torch.nn.ReLU())
    net = torch.nn.Sequential(*mods)
    if state_dict is not None:
        net.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in state_dict.items()})
    return net.to(dtype)


def flat(net_or_sd):
    sd = net_or_sd.state_dict() if hasattr(net_or_sd, "state_dict") else net_or_sd
    return np.concatenate([np.asarray(sd[k].detach().cpu().numpy() if torch.is_tensor(sd[k]) else sd[k]).reshape(-1) for k in KEYS])


def adam_flat(opt, net, name):
    return np.concatenate([opt.state[p][name].detach().numpy().reshape(-1) for p in net.parameters()])


def torch_step(net, opt, x, target):
    """the reference's step (icrl/exploration.py:246-261): -> (row_err [rows], MSE) of the pre-step predictions, in the net's precision."""
    loss = torch.nn.MSELoss(reduction="none")(net(x), target)
    row_err = loss.clone().detach().numpy().sum(axis=-1)
    opt.zero_grad()
    loss.mean().backward()
    opt.step()
    return row_err, loss.mean().item()


def tol(ref32, ref64):
    """the rule: 4 x max |ref32 - ref64| of the quantity + 1e-12 (both implementations sit about one float32 rounding from the exact value: a
    factor 2; another 2 for a different summation order)."""
    return 4.0 * float(np.max(np.abs(np.asarray(ref32, dtype=np.float64) - np.asarray(ref64, dtype=np.float64)))) + 1e-12


def check(name, got, ref32, ref64, misses=None):
    """print the measured distance next to the bound, then assert it — or, with a `misses` list, note a miss there and go on, so that one
    test reports every quantity (its caller asserts that the list is empty at the end)."""
    d = float(np.max(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref32, dtype=np.float64))))
    t = tol(ref32, ref64)
    print(f"{name}: max|got - ref32| = {d:.3e}, bound 4 max|ref32 - ref64| + 1e-12 = {t:.3e}")
    ok = bool(np.all(np.isfinite(np.asarray(got, dtype=np.float64))) and d <= t)
    if misses is not None:
        if not ok:
            misses.append((name, d, t))
        return
    assert ok, (name, d, t)


def load_golden():
    return np.load(GOLDEN)


def ref64_of(g, key):
    """the float64 reference of `key`: stored as its float32 distance from the float32 reference (half the bytes; exact to ~1e-14 relative)."""
    return g[key + "_32"].astype(np.float64) + g[key + "_d64"].astype(np.float64)


def state_dict_of(g, prefix):
    return {k: g[f"{prefix}_{k}"] for k in KEYS}


def recompute(g, case, tag, dtype):
    """the callback `tag` ("e": ExplorationRewardCallback, "l": LambdaShapingCallback) of `case` in torch on the host, from the fixture's
    initial weights and the regenerated planes, in `dtype`: the fixture's quantities by their key stems, plus per step the parameters and
    both Adam moments of every net ("pred_params_r0", "pred_exp_avg_r0", "pred_exp_avg_sq_r0", ...) and the row errors of "e"."""
    obs, act, T, N, hidden = CASES[case]
    seed = int(g[f"{case}_seed"])
    np_t = np.float32 if dtype == torch.float32 else np.float64
    nets = {}
    for short, out_dim in (("cost", 1), ("pred", obs)) if tag == "l" else (("pred", obs),):
        net = make_net(obs + act, out_dim, hidden, state_dict_of(g, f"{case}_{tag}_{short}_init"), dtype)
        nets[short] = (net, torch.optim.Adam(net.parameters(), lr=LR))
    res = {}
    for r in range(ROLLOUTS):
        pl = {k: v.astype(np_t) for k, v in planes(seed, r, obs, act, T, N).items()}
        x = torch.from_numpy(np.concatenate([pl["observations"], pl["actions"]], -1).reshape(T * N, -1))
        logs = []
        if tag == "l":
            _, cost_loss = torch_step(*nets["cost"], x, torch.from_numpy(pl["costs"].reshape(-1, 1)))
        row_err, mse = torch_step(*nets["pred"], x, torch.from_numpy(pl["new_observations"].reshape(T * N, -1)))
        res[f"row_err_r{r}"] = row_err
        if tag == "e":
            res[f"rewards_r{r}"] = pl["rewards"] + row_err.reshape(T, N)
            logs = [np.mean(row_err)]
        else:
            res[f"cost_adv_r{r}"] = pl["cost_advantages"] / (1 + row_err.reshape(T, N))
            logs = [np.mean(row_err), np.std(row_err), mse, cost_loss]
        res[f"log_r{r}"] = np.asarray(logs, dtype=np.float64)
        for short, (net, opt) in nets.items():
            res[f"{short}_params_r{r}"] = flat(net)
            res[f"{short}_exp_avg_r{r}"] = adam_flat(opt, net, "exp_avg")
            res[f"{short}_exp_avg_sq_r{r}"] = adam_flat(opt, net, "exp_avg_sq")
    for short in nets:
        res[f"{short}_params"] = res[f"{short}_params_r{ROLLOUTS - 1}"]
    return res
