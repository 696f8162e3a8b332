"""Discriminators and agent pairs for tests/test_disc_cost_cpu.py and tests/test_disc_cost_gpu.py: the two reference-trained
gail_discriminator.pt fixtures, fresh discriminators of the shapes the rollout kernels take, and twin device chains whose cost wrapper
holds a gail_utils.DiscriminatorCost (cpg --load_gail)."""
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARTIFACTS = os.path.join(HERE, "golden", "ref_artifacts", "ConstraintTransfer", "GAIL")
POINT_PT = os.path.join(ARTIFACTS, "Point", "files", "gail_discriminator.pt")              # obs 113 / act 8 on file, inputs: x and y
ANTBROKEN_PT = os.path.join(ARTIFACTS, "AntBroken", "files", "gail_discriminator.pt")      # all 121 inputs
BUF_KEYS = ("observations", "orig_observations", "new_observations", "new_orig_observations", "actions", "rewards", "costs",
            "orig_costs", "dones", "log_probs", "reward_values", "cost_values", "reward_advantages", "cost_advantages",
            "reward_returns", "cost_returns")
ENV_DIMS = {"hc": (18, 6), "ant": (113, 8), "point_circle": (9, 2), "lgw": (1, 2)}      # obs, acs (lgw: one-hot over 2 actions)


def fresh(obs_dim, acs_dim, hidden, seed=0, is_discrete=False, out_scale=None):
    """a GailDiscriminator with torch's default initialisation under `seed`; out_scale multiplies its output layer (weights and bias):
    the sigmoid then saturates on both sides."""
    from icrl_amd.gail_utils import GailDiscriminator
    torch.manual_seed(seed)
    d = GailDiscriminator(obs_dim, acs_dim, list(hidden), None, lambda x: 0.0, None, None, is_discrete, optimizer_class=None)
    if out_scale is not None:
        sd = d.state_dict()
        last = 2 * len(hidden)
        sd[f"{last}.weight"] = sd[f"{last}.weight"] * out_scale
        sd[f"{last}.bias"] = sd[f"{last}.bias"] * out_scale
        d.load_state_dict(sd)
    return d


def load_point():
    """the Point fixture as `cpg --load_gail -cosd 0 1 -casd -1` loads it for PointCircle-v0 (obs 9, act 2)."""
    from icrl_amd.gail_utils import GailDiscriminator
    lo = np.full(2, -0.25, np.float32)
    return GailDiscriminator.load(POINT_PT, obs_dim=9, acs_dim=2, is_discrete=False, obs_select_dim=[0, 1], acs_select_dim=[-1], clip_obs=None,
                                  obs_mean=None, obs_var=None, action_low=lo, action_high=-lo)


def load_antbroken():
    from icrl_amd.gail_utils import GailDiscriminator
    lo = -np.ones(8, np.float32)
    return GailDiscriminator.load(ANTBROKEN_PT, obs_dim=113, acs_dim=8, is_discrete=False, obs_select_dim=None, acs_select_dim=None, clip_obs=None,
                                  obs_mean=None, obs_var=None, action_low=lo, action_high=-lo)


def disc_for(kind, hidden=None, seed=3):
    """the discriminator a rollout case of `kind` runs against: the fixtures where their shapes fit, else a fresh one."""
    if kind == "point_circle" and hidden is None:
        return load_point()
    if kind in ("ant", "antbroken") and hidden is None:
        return load_antbroken()
    od, ad = ENV_DIMS["ant" if kind == "antbroken" else kind]
    return fresh(od, ad, hidden or [20], seed, is_discrete=kind == "lgw")


def pair(N, T, seed, kind, hidden=None, agent_kwargs=None, **norm):
    """two agents over twin chains VecNormalizeWithCost -> VecCostWrapper(DiscriminatorCost) -> HipSynthVecEnv: same policy, same
    discriminator weights (one discriminator object each)."""
    from icrl_amd.gail_utils import DiscriminatorCost
    from icrl_amd.ppo_lag import PPOLagrangian
    from icrl_amd.vec_env import HipSynthVecEnv, VecCostWrapper, VecNormalizeWithCost
    out = []
    for _ in range(2):
        torch.manual_seed(seed)
        env = VecNormalizeWithCost(VecCostWrapper(HipSynthVecEnv(N, "ant" if kind == "antbroken" else kind, seed, broken=kind == "antbroken")), **norm)
        env.set_cost_function(DiscriminatorCost(disc_for(kind, hidden)))
        out.append((PPOLagrangian("TwoCriticsMlpPolicy", env, n_steps=T, seed=seed, **(agent_kwargs or {})), env))
    out[1][0].policy.load_state_dict(out[0][0].policy.state_dict())
    out[1][1].venv.cost_function.disc.load_state_dict(out[0][1].venv.cost_function.disc.state_dict())
    return out


def noise(kind, rollouts, T, N, seed=8):
    rng = np.random.RandomState(seed)
    if kind == "lgw":
        return torch.as_tensor(rng.rand(rollouts, T, N).astype(np.float32), device="cuda")
    ad = ENV_DIMS["ant" if kind == "antbroken" else kind][1]
    return torch.as_tensor(rng.randn(rollouts, T, N, ad).astype(np.float32), device="cuda")


def disc_reward(disc, obs, acs):
    """icrl_disc_reward(apply_log = 0) on device rows -> float32 device tensor [N]."""
    from icrl_amd import _lib
    from icrl_amd.structs import p
    out = torch.full((obs.shape[0],), -1.0, device="cuda")
    s = disc.struct()
    _lib.check(_lib.lib().icrl_disc_reward(_lib.byref(s), p(obs), p(acs), obs.shape[0], p(out), 0, _lib.current_stream()), "icrl_disc_reward")
    return out
