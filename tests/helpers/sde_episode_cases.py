"""gSDE episode cases for tests/test_sde_episodes_gpu.py: agents at a trained-like state (helpers/sde_update_cases.trained_like: log_std uniform in
[-1.5, 0.5]) holding a non-trivial E0 installed with set_noise from recorded numpy normals, 1-env evaluation stacks whose episodes run at most M
steps, and the two ways to run their episodes: the per-step loop (utils.SteppedEpisodeRun) and what utils.sample_from_agent / evaluate_policy take
(utils._run_episodes(chain=True): the sampler launches with the gSDE head)."""
import numpy as np
import torch

from helpers import sde_update_cases as U

M = 48                  # episode limit of the envs here (the kernels read env.max_steps)
PL = dict(pi=[32, 48], vf=[64, 64], cvf=[64, 64])       # -pl 32 48: zero rows of the latent
# train env the agent is built over, per eval env id
TRAIN_ID = {"HCWithPos-v0": "HCWithPos-v0", "HCWithPosTest-v0": "HCWithPos-v0", "AntWall-v0": "AntWall-v0", "PointCircleTest-v0": "PointCircle-v0"}
# action_net.bias = -c * sign(B[0]) drives obs[0] of HCWithPosTest-v0 towards the wall at -3.  The three strengths under which, for the agent of
# agent("HCWithPosTest-v0", steer=c) and 6 episodes of at most M steps on eval_env("HCWithPosTest-v0"), no / some / all episodes end early: found
# once on an MI355X with the per-step loop alone (SteppedEpisodeRun) — sampling: lengths [48] * 6 / [48, 48, 27, 48, 24, 28] / [14, 13, 13, 13, 17, 15];
# under "some" the mode gives [46, 48, 42, 45, 47, 48], "some" as well.  Every test asserts its property on the loop's own result.
STEER = {"none": 0.0, "some": 0.4, "all": 2.5}
ROW_KEYS = ("orig_obs", "obs", "actions")


def agent(env_id, seed=13, arch=None, steer=None, noise=True):
    """a gSDE agent over a 4-env train chain; noise: install E0 / E from recorded normals (else the policy holds no matrices: sde_E is None)"""
    from icrl_amd import utils
    from icrl_amd.ppo_lag import PPOLagrangian
    from icrl_amd.vec_env import dynamics_matrix
    torch.manual_seed(seed)
    env = utils.make_train_env(TRAIN_ID[env_id], None, True, seed, 4, cost_info_str="cost", reward_gamma=0.99, cost_gamma=0.99)
    kw = dict(policy_kwargs=dict(net_arch=[dict(arch)])) if arch is not None else {}
    ag = PPOLagrangian("TwoCriticsMlpPolicy", env, n_steps=32, seed=seed, use_sde=True, **kw)
    sd = U.trained_like(ag.policy, 100 + seed)
    if steer is not None:
        sd = dict(sd)
        sd["action_net.bias"] = (-steer * np.sign(dynamics_matrix("hc")[0])).astype(np.float32)
        ag.policy.load_state_dict({k: torch.as_tensor(np.asarray(v, np.float32)) for k, v in sd.items()})
    pol = ag.policy
    pol.sde_E0 = pol.sde_E = None
    if noise:
        install_noise(pol, seed + 1)
    return ag


def install_noise(pol, seed):
    """E0 [H, A] and E [1, H, A] = recorded standard normals times exp(log_std), as reset_noise scales its draws"""
    rng = np.random.RandomState(seed)
    H, A = pol.sde_latent, pol.act_dim
    z0, z = rng.randn(H, A).astype(np.float32), rng.randn(1, H, A).astype(np.float32)
    std = np.exp(pol.log_std.cpu().numpy())
    pol.set_noise(z0 * std, z * std)
    return (z0 * std).astype(np.float64)


def eval_env(env_id, seed=5, max_steps=M, stats_seed=11):
    """utils.make_eval_env with an episode limit of max_steps and frozen statistics that are not the initial (0, 1) ones"""
    from icrl_amd import utils
    env = utils.make_eval_env(env_id, False, seed=seed)
    env.unwrapped.max_steps = max_steps
    r = np.random.RandomState(stats_seed)
    d = env.unwrapped.obs_dim
    env.obs_rms.assign(0.1 * r.randn(d), 0.5 + r.rand(d), 100.0)
    return env


def snapshot(run, env):
    """rows, episode sums and lengths of a finished run, and what it left in the env chain"""
    senv = env.unwrapped
    out = {k: run.rows_of(k).clone() for k in ROW_KEYS}
    out.update(ep_rewards=run.out["ep_rewards"].clone(), ep_lengths=run.out["ep_lengths"].clone(), s=senv.s.clone(),
               step_count=senv.step_count.clone(), t_ep=senv.t_ep.clone(), old_obs=env.old_obs.reshape(1, -1).clone())
    return out


def loop(ag, env_id, n, deterministic, **kw):
    """the per-step loop on a fresh env: (snapshot, run)"""
    from icrl_amd import utils
    env = eval_env(env_id, **kw)
    run = utils.SteppedEpisodeRun(ag, env, n, deterministic, None)
    return snapshot(run, env), run


def launch(ag, env_id, n, deterministic, parallel=True, **kw):
    """what sample_from_agent (parallel) / evaluate_policy (not parallel) run, on a fresh env of the same seed: (snapshot, run)"""
    from icrl_amd import utils
    env = eval_env(env_id, **kw)
    run = utils._run_episodes(ag, env, n, deterministic, None, parallel, chain=True)
    return snapshot(run, env), run


def assert_equal(got, want, what=""):
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k, got[k].shape, want[k].shape, got[k].dtype, want[k].dtype)
        assert torch.equal(got[k], want[k]), (what, k)


def head_numpy_actions(sd, E0, obs):
    """float64: clip(mean + latent . E0) of the policy network on the rows of `obs`; E0 in its logical shape [H, A]"""
    f = lambda k: np.asarray(sd[k], np.float64)
    x = np.asarray(obs, np.float64)
    h = np.tanh(x @ f("mlp_extractor.policy_net.0.weight").T + f("mlp_extractor.policy_net.0.bias"))
    lat = np.tanh(h @ f("mlp_extractor.policy_net.2.weight").T + f("mlp_extractor.policy_net.2.bias"))
    mean = lat @ f("action_net.weight").T + f("action_net.bias")
    return np.clip(mean + lat @ np.asarray(E0, np.float64), -1.0, 1.0)
