"""gSDE update cases for tests/test_sde_update_gpu.py: an agent at a trained-like state (log_std in [-1.5, 0.5], every tensor perturbed, both
Adam moments non-zero on the real entries), a rollout buffer whose old log-probs come from the current policy on sampled actions (ratios
start near 1), the permutations — and the two runs of train(perms=...) from that one state: the fine-grained loop (ICRL_SDE_UPDATE_STEPPED=1,
the yardstick; golden g26 pins it to the reference) and the fused launch."""
import os
import types

import numpy as np
import torch

from helpers import sde_cases as C

LR = 3e-4
ADAM_DEV_BOUND = 5e-4      # tests/test_ppo_train_gpu.py: an fp32 persistent update against its reference-equivalent
SCALARS = ("train/policy_gradient_loss", "train/reward_value_loss", "train/cost_value_loss", "train/approx_kl", "train/clip_fraction", "train/entropy_loss",
           "train/loss")
ARCH64 = dict(pi=[64, 64], vf=[64, 64], cvf=[64, 64])


def make_agent(O, A, T, N, B, E, arch=None, **kw):
    from icrl_amd import logger, spaces
    from icrl_amd.ppo_lag import PPOLagrangian
    env = types.SimpleNamespace(num_envs=N, observation_space=spaces.Box(-np.inf, np.inf, (O,), np.float64), action_space=spaces.Box(-1.0, 1.0, (A,), np.float32))
    logger.configure()
    agent = PPOLagrangian("TwoCriticsMlpPolicy", env, n_steps=T, batch_size=B, n_epochs=E, penalty_initial_value=1, penalty_learning_rate=0.1, budget=0.0,
                          use_sde=True, sde_sample_freq=8, policy_kwargs=dict(net_arch=[dict(arch or ARCH64)]), **kw)
    agent.update_penalty_after = 10 ** 6      # (nu stays what it is across the two runs of a case)
    return agent


def real_mask(pol):
    """bool [n_params]: the entries of the flat buffer that are no padding."""
    parts = []
    for k, shp in pol.shapes.items():
        m = np.zeros(shp, bool)
        m[tuple(slice(0, n) for n in pol.logical_shapes[k])] = True
        parts.append(m.ravel())
    return np.concatenate(parts)


def trained_like(pol, seed):
    """a state drawn from numpy alone (the same on every device): weights ~ N(0, 1 / fan_in), biases ~ 0.1 N(0, 1), the head scaled to actions
    of order 1, log_std uniform in [-1.5, 0.5]; both moments as after some steps, zero on the padding.  Returns the state dict (numpy)."""
    rng = np.random.RandomState(seed)
    sd = {}
    for k, shp in pol.logical_shapes.items():
        if k == "log_std":
            sd[k] = rng.uniform(-1.5, 0.5, shp)
        elif len(shp) == 2:
            sd[k] = rng.randn(*shp) / np.sqrt(shp[1])
        else:
            sd[k] = 0.1 * rng.randn(*shp)
    sd["action_net.bias"] = rng.uniform(-0.5, 0.5, sd["action_net.bias"].shape)
    assert sd["log_std"].min() >= -1.5 and sd["log_std"].max() <= 0.5 and sd["log_std"].std() > 0.3
    pol.load_state_dict({k: torch.as_tensor(v.astype(np.float32)) for k, v in sd.items()})
    mask = torch.as_tensor(real_mask(pol), device=pol.params.device)
    g = rng.randn(pol.n_params).astype(np.float32)
    pol.exp_avg.copy_(torch.as_tensor(1e-3 * g, device=pol.params.device) * mask)
    pol.exp_avg_sq.copy_(torch.as_tensor((1e-6 * (0.5 + rng.rand(pol.n_params)) * g * g).astype(np.float32), device=pol.params.device) * mask)
    pol.adam_step = 7
    pol.prepare()
    return {k: v.numpy() for k, v in pol.state_dict().items()}


def planes_of(sd, T, N, O, A, E, seed):
    """the buffer's planes, flat [T * N, ...] in storage order, and the permutations: observations ~ N(0, 1); actions sampled from the current
    policy's Normal(mean, sqrt(var)); old log-probs the policy's own (float64 head, rounded once); old values near the critics' outputs;
    advantages and returns as the update tests draw them."""
    rng = np.random.RandomState(seed)
    obs = rng.randn(T * N, O).astype(np.float32)
    out, _ = C.head_numpy(sd, obs, np.zeros((T * N, A)))
    act = (out["mean"] + np.sqrt(out["var"]) * rng.randn(T * N, A)).astype(np.float32)
    out, _ = C.head_numpy(sd, obs, act)
    planes = dict(observations=obs, actions=act, log_probs=out["log_prob"], reward_values=out["v_r"] + 0.1 * rng.randn(T * N), cost_values=out["v_c"] + 0.1 * rng.randn(T * N),
                  reward_advantages=2.0 * rng.randn(T * N), cost_advantages=rng.rand(T * N), reward_returns=out["v_r"] + 0.5 * rng.randn(T * N),
                  cost_returns=out["v_c"] + 0.5 * rng.rand(T * N), orig_costs=rng.rand(T * N))
    planes = {k: np.asarray(v, np.float32) for k, v in planes.items()}
    return planes, np.stack([rng.permutation(T * N) for _ in range(E)])


def fill_buffer(agent, sd, seed):
    rb = agent.rollout_buffer
    T, N = rb.buffer_size, rb.n_envs
    planes, perms = planes_of(sd, T, N, agent.policy.obs_dim, agent.policy.act_dim, agent.n_epochs, seed)
    for k, v in planes.items():
        plane = getattr(rb, k)
        plane.copy_(torch.as_tensor(v.reshape(plane.shape)))
    rb.full, rb.pos = True, T
    return perms


def snapshot(agent):
    pol = agent.policy
    return dict(params=pol.params.clone(), exp_avg=pol.exp_avg.clone(), exp_avg_sq=pol.exp_avg_sq.clone(), adam_step=pol.adam_step, n_updates=agent._n_updates)


def restore(agent, snap):
    pol = agent.policy
    pol.params.copy_(snap["params"]); pol.exp_avg.copy_(snap["exp_avg"]); pol.exp_avg_sq.copy_(snap["exp_avg_sq"])
    pol.adam_step, agent._n_updates = snap["adam_step"], snap["n_updates"]
    pol.prepare()


def run(agent, perms, stepped, hook=None):
    """one train(perms=...) on the path asked for; returns what the comparison reads."""
    from icrl_amd import logger
    old = os.environ.pop("ICRL_SDE_UPDATE_STEPPED", None)
    if stepped:
        os.environ["ICRL_SDE_UPDATE_STEPPED"] = "1"
    agent.sde_step_hook = hook
    try:
        agent.train(perms=perms)
    finally:
        agent.sde_step_hook = None
        os.environ.pop("ICRL_SDE_UPDATE_STEPPED", None)
        if old is not None:
            os.environ["ICRL_SDE_UPDATE_STEPPED"] = old
    assert agent.last_sde_update == ("loop" if stepped or hook is not None else "fused"), (agent.last_sde_update, agent.last_sde_update_reason)
    pol, lg = agent.policy, logger.Logger.CURRENT.name_to_value
    return dict(params=pol.params.cpu().numpy().copy(), exp_avg=pol.exp_avg.cpu().numpy().copy(), exp_avg_sq=pol.exp_avg_sq.cpu().numpy().copy(), adam_step=pol.adam_step,
                log={k: float(lg[k]) for k in SCALARS}, early_stop_epoch=int(lg["train/early_stop_epoch"]), epoch_kls=np.array(agent.epoch_kls, np.float32),
                stats=agent._train_ws["stats"].cpu().numpy().copy())


def compare(tag, fused, loop, steps0, lr=LR):
    """the project's bounds for an fp32 persistent update against its reference-equivalent; returns the measured fraction of the parameter bound."""
    assert fused["early_stop_epoch"] == loop["early_stop_epoch"], (fused["early_stop_epoch"], loop["early_stop_epoch"])
    n_steps = loop["adam_step"] - steps0
    assert n_steps > 0 and fused["adam_step"] == loop["adam_step"], (fused["adam_step"], loop["adam_step"], steps0)
    worst = float(np.abs(fused["params"].astype(np.float64) - loop["params"]).max())
    bound = ADAM_DEV_BOUND * lr * n_steps + 2e-7
    print(f"SDE_ADAM_DEV {tag} steps={n_steps}: max |fused - loop| = {worst:.3g} = {worst / (lr * n_steps):.3g} x lr x steps = {worst / bound:.3g} of the bound {bound:.3g}")
    for k in SCALARS:
        print(f"SDE_SCALAR {tag} {k}: fused {fused['log'][k]!r} loop {loop['log'][k]!r}")
    print(f"SDE_KLS {tag}: fused {fused['epoch_kls'].tolist()} loop {loop['epoch_kls'].tolist()}")
    assert np.isfinite(fused["params"]).all() and worst <= bound, (worst, bound)
    for k in SCALARS:
        assert abs(fused["log"][k] - loop["log"][k]) < 2e-4 + 2e-3 * abs(loop["log"][k]), (k, fused["log"][k], loop["log"][k])
    assert np.allclose(fused["epoch_kls"], loop["epoch_kls"], atol=2e-5), (fused["epoch_kls"], loop["epoch_kls"])
    return worst / bound


def case(O, A, T, N, B, E, seed=0, arch=None, **kw):
    """(agent, the state dict it starts from, permutations, snapshot) of one case."""
    torch.manual_seed(seed)
    agent = make_agent(O, A, T, N, B, E, arch=arch, **kw)
    sd = trained_like(agent.policy, 100 + seed)
    perms = fill_buffer(agent, sd, 200 + seed)
    return agent, sd, perms, snapshot(agent)


def both(tag, agent, perms, snap, hook=None):
    """the loop, then the fused launch, from the same state; (fused, loop, fraction of the parameter bound)."""
    restore(agent, snap)
    loop = run(agent, perms, stepped=True, hook=hook)
    restore(agent, snap)
    fused = run(agent, perms, stepped=False)
    return fused, loop, compare(tag, fused, loop, snap["adam_step"], lr=float(agent.lr_schedule(1.0)))
