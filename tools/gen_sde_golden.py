"""Record tests/golden/g26_sde.npz from the REFERENCE's own gSDE policy and PPOLagrangian(use_sde=True) (build machine only).

    python tools/gen_sde_golden.py --reference <checkout of the reference>

stable_baselines3 is imported unmodified from the checkout under the third-party stand-ins of oracle/ref_shim (gym is not installed); runs on the
CPU; changes nothing under oracle/.  Only arrays are written.  For two shapes — "hc": obs 18, act 6, 64-64 everywhere; "pl": obs 11, act 3,
`-pl 32 48` (policy branch 32-48, critics 64-64) — at a TRAINED-LIKE state (every tensor moved off its initial value, log_std uniform in [-1.5, 0.5]):

  <s>/w/<name>                    the reference policy's state_dict (log_std [H, A] first)
  <s>/obs, <s>/act [48, .]        a batch (float32 values)
  <s>/E0 [H, A], <s>/E [48, H, A] fixed exploration matrices ~ Normal(0, exp(log_std))
  <s>/fwd/{actions,v_r,v_c,log_prob}     policy.forward with one matrix per row;  <s>/fwd0/...: with E0 for every row;  <s>/fwd/mean: the mode
  <s>/up/{d_v_r,d_v_c,d_log_prob,d_entropy} [48]   a fixed random upstream
  for n in 48, 17, 1 (the first n rows):
  <s>/ev<n>/{v_r,v_c,log_prob,entropy}   evaluate_actions in float32;  <s>/ev<n>_64/...: the same module in float64
  <s>/g<n>/<name>                        float32 autograd gradient of sum(upstream * outputs) w.r.t. every parameter (n = 17 and 1: "pl" only)
  <s>/dev<n>/<name>, <s>/dev<n>/out/<k>  max |float32 - float64 autograd| per gradient block / output: the reference's own float32 error, the tests' unit
  "pl" only — three teacher-forced optimiser steps of the reference's train() (n_epochs 1, batch 32 over a 2 x 48-row buffer):
  pl/train/buf/<plane> [96] env-major, pl/train/perm [96], pl/train/nu0, pl/train/w<k>/<name> (k = 1..3: after each step), pl/train/log/<key>
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"hc": (18, 6, dict(pi=[64, 64], vf=[64, 64], cvf=[64, 64])), "pl": (11, 3, dict(pi=[32, 48], vf=[64, 64], cvf=[64, 64]))}
N, T_TRAIN, N_ENVS, BATCH = 48, 48, 2, 32
OUTS = ("v_r", "v_c", "log_prob", "entropy")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "g26_sde.npz"))
    a = ap.parse_args()
    sys.path[:0] = [os.path.join(ROOT, "oracle", "ref_shim"), a.reference, os.path.join(a.reference, "custom_envs")]
    import gym
    import torch as th
    from stable_baselines3 import PPOLagrangian
    from stable_baselines3.common import logger as ref_logger
    from stable_baselines3.common.policies import ActorTwoCriticsPolicy
    from stable_baselines3.common.vec_env import VecEnv

    th.set_num_threads(1)
    out = {}

    def trained_like(policy, rng):
        sd = policy.state_dict()
        assert list(sd)[0] == "log_std"
        new = {}
        for k, v in sd.items():
            if k == "log_std":
                new[k] = th.as_tensor(rng.uniform(-1.5, 0.5, tuple(v.shape)).astype(np.float32))
            elif k.startswith("action_net"):
                new[k] = v + th.as_tensor((0.3 * rng.randn(*v.shape)).astype(np.float32))
            else:
                new[k] = v + th.as_tensor((0.05 * rng.randn(*v.shape)).astype(np.float32))
        policy.load_state_dict(new)
        return {k: v.numpy().copy() for k, v in policy.state_dict().items()}

    def set_matrices(policy, E0, E):
        policy.action_dist.exploration_mat = th.as_tensor(E0, dtype=policy.log_std.dtype)
        policy.action_dist.exploration_matrices = th.as_tensor(E, dtype=policy.log_std.dtype)

    def make(obs_space, act_space, net_arch):
        return ActorTwoCriticsPolicy(obs_space, act_space, lambda _: 3e-4, net_arch=net_arch, use_sde=True, log_std_init=0.0)

    def outputs_and_grads(policy, obs, act, up, dtype):
        pol = make(policy.observation_space, policy.action_space, policy.net_arch)      # (a fresh module: the distribution object holds non-leaf tensors)
        pol.load_state_dict(policy.state_dict())
        pol = pol.to(dtype)
        o, ac = th.as_tensor(obs).to(dtype), th.as_tensor(act).to(dtype)
        if dtype == th.float32:
            v_r, v_c, lp, ent = pol.evaluate_actions(o, ac)
        else:      # evaluate_actions line by line without extract_features, which casts the observation to float32 (policies.py:752-767)
            latent_pi, latent_vf, latent_cvf = pol.mlp_extractor(o)
            dist = pol._get_action_dist_from_latent(latent_pi, latent_pi)
            v_r, v_c, lp, ent = pol.value_net(latent_vf), pol.cost_value_net(latent_cvf), dist.log_prob(ac), dist.entropy()
        res = dict(v_r=v_r.flatten(), v_c=v_c.flatten(), log_prob=lp, entropy=ent)
        loss = sum((th.as_tensor(up["d_" + k]).to(dtype) * res[k]).sum() for k in OUTS)
        names = [k for k, _ in pol.named_parameters()]
        grads = th.autograd.grad(loss, [p for _, p in pol.named_parameters()], allow_unused=True)
        g = {k: (th.zeros_like(p) if gi is None else gi).detach().numpy() for k, gi, (_, p) in zip(names, grads, pol.named_parameters())}
        return {k: v.detach().numpy() for k, v in res.items()}, g

    for tag, (O, A, arch) in SHAPES.items():
        rng = np.random.RandomState(2600 + O)
        th.manual_seed(26)
        policy = make(gym.spaces.Box(-np.inf, np.inf, (O,), np.float64), gym.spaces.Box(-1, 1, (A,), np.float32), [arch])
        H = arch["pi"][-1]
        assert tuple(policy.log_std.shape) == (H, A) and policy.action_dist.learn_features is False
        sd = trained_like(policy, rng)
        assert list(sd) == [k for k, _ in policy.named_parameters()]
        obs = rng.randn(N, O).astype(np.float32)
        std = np.exp(sd["log_std"])
        E0 = (rng.randn(H, A) * std).astype(np.float32)
        E = (rng.randn(N, H, A) * std).astype(np.float32)
        for k, v in sd.items():
            out[f"{tag}/w/{k}"] = v
        out[f"{tag}/obs"], out[f"{tag}/E0"], out[f"{tag}/E"] = obs, E0, E
        with th.no_grad():
            set_matrices(policy, E0, E)
            actions, v_r, v_c, lp = policy.forward(th.as_tensor(obs))
            mean = policy.forward(th.as_tensor(obs), deterministic=True)[0]
            set_matrices(policy, E0, E[:1])      # a matrix count that is not the row count: E0 for every row (get_noise)
            a0, _, _, lp0 = policy.forward(th.as_tensor(obs))
        for k, v in (("actions", actions), ("v_r", v_r.flatten()), ("v_c", v_c.flatten()), ("log_prob", lp), ("mean", mean)):
            out[f"{tag}/fwd/{k}"] = v.numpy()
        out[f"{tag}/fwd0/actions"], out[f"{tag}/fwd0/log_prob"] = a0.numpy(), lp0.numpy()
        # the scored actions: the sampled ones moved a little, so that (a - mean)^2 / var is of order one and not exactly the sample's
        act = (actions.numpy() + 0.1 * rng.randn(N, A)).astype(np.float32)
        out[f"{tag}/act"] = act
        up = {"d_" + k: rng.randn(N).astype(np.float32) for k in OUTS}
        for k, v in up.items():
            out[f"{tag}/up/{k}"] = v
        for n in (48, 17, 1):
            upn = {k: v[:n] for k, v in up.items()}
            r32, g32 = outputs_and_grads(policy, obs[:n], act[:n], upn, th.float32)
            r64, g64 = outputs_and_grads(policy, obs[:n], act[:n], upn, th.float64)
            for k in OUTS:
                out[f"{tag}/ev{n}/{k}"], out[f"{tag}/ev{n}_64/{k}"] = r32[k], r64[k]
                out[f"{tag}/dev{n}/out/{k}"] = np.float64(np.abs(r32[k].astype(np.float64) - r64[k]).max())
            dev = {k: np.float64(np.abs(g32[k].astype(np.float64) - g64[k]).max()) for k in g32}
            if n == 48 or tag == "pl":      # (the file's size: the ragged and the one-row gradients are kept for the padded shape alone)
                for k in g32:
                    out[f"{tag}/g{n}/{k}"], out[f"{tag}/dev{n}/{k}"] = g32[k], dev[k]
            worst = max(dev[k] / max(np.abs(g64[k]).max(), 1e-30) for k in g32)
            print(f"{tag} n={n}: float32 vs float64 autograd, worst block max|diff| / max|grad| = {worst:.3g}; log_std block {dev['log_std']:.3g}; "
                  f"outputs {[float(out[f'{tag}/dev{n}/out/{k}']) for k in OUTS]}")
        # the detach: an entropy-only upstream reaches log_std alone
        _, gd = outputs_and_grads(policy, obs, act, dict(d_v_r=np.zeros(N, np.float32), d_v_c=np.zeros(N, np.float32), d_log_prob=np.zeros(N, np.float32),
                                                         d_entropy=up["d_entropy"]), th.float64)
        assert np.abs(gd["log_std"]).max() > 0 and all(np.abs(v).max() == 0 for k, v in gd.items() if k != "log_std")

        if tag != "pl":
            continue
        # ---- three teacher-forced optimiser steps of the reference's train()
        class _Env(VecEnv):
            def __init__(self):
                super().__init__(N_ENVS, gym.spaces.Box(-np.inf, np.inf, (O,), np.float64), gym.spaces.Box(-1, 1, (A,), np.float32))
            def reset(self): return np.zeros((N_ENVS, O))
            def step_async(self, actions): pass
            def step_wait(self): raise RuntimeError("the generator never steps")
            def close(self): pass
            def seed(self, seed=None): return [seed]
            def get_attr(self, *a_, **k_): return []
            def set_attr(self, *a_, **k_): pass
            def env_method(self, *a_, **k_): return []

        agent = PPOLagrangian("TwoCriticsMlpPolicy", _Env(), n_steps=T_TRAIN, batch_size=BATCH, n_epochs=1, target_kl=None, penalty_initial_value=1,
                              penalty_learning_rate=0.1, budget=0.0, seed=26, device="cpu", verbose=0, use_sde=True, sde_sample_freq=8,
                              policy_kwargs=dict(net_arch=[arch]))
        assert agent.use_sde and tuple(agent.policy.log_std.shape) == (H, A)
        agent.policy.load_state_dict({k: th.as_tensor(v) for k, v in sd.items()})
        R = T_TRAIN * N_ENVS
        b_obs = rng.randn(R, O).astype(np.float32)
        with th.no_grad():
            agent.policy.reset_noise(R)
            b_act, b_vr, b_vc, b_lp = agent.policy.forward(th.as_tensor(b_obs))
        planes = dict(observations=b_obs, actions=b_act.numpy(), log_probs=b_lp.numpy() + 0.05 * rng.randn(R), reward_values=b_vr.numpy().ravel() + 0.1 * rng.randn(R),
                      cost_values=b_vc.numpy().ravel() + 0.1 * rng.randn(R), reward_advantages=2 * rng.randn(R), cost_advantages=rng.rand(R),
                      reward_returns=rng.randn(R), cost_returns=rng.rand(R), orig_costs=rng.rand(R))
        planes = {k: np.asarray(v, np.float32) for k, v in planes.items()}
        rb = agent.rollout_buffer
        for k, v in planes.items():      # recorded env-major (row = env * T + t), as get() flattens the [T, N] planes it is given here
            getattr(rb, k)[...] = v.reshape((N_ENVS, T_TRAIN) + getattr(rb, k).shape[2:]).swapaxes(0, 1)
        rb.generator_ready, rb.full, rb.pos = False, True, T_TRAIN
        steps, opt = [], agent.policy.optimizer
        orig_step = opt.step
        def rec_step(*a_, **k_):
            r = orig_step(*a_, **k_)
            steps.append({k: v.detach().numpy().copy() for k, v in agent.policy.state_dict().items()})
            return r
        opt.step = rec_step
        perms, orig_perm = [], np.random.permutation
        def rec_perm(n):
            q = orig_perm(n); perms.append(q.copy()); return q
        nu0 = agent.dual.nu().item()
        ref_logger.Logger.CURRENT.name_to_value.clear()
        np.random.permutation = rec_perm
        try:
            agent.train()
        finally:
            np.random.permutation = orig_perm
        assert len(steps) == 3 and len(perms) == 1
        logs = {k: float(v) for k, v in ref_logger.Logger.CURRENT.name_to_value.items() if k.startswith("train/")}
        for k, v in planes.items():
            out[f"pl/train/buf/{k}"] = v
        out["pl/train/perm"], out["pl/train/nu0"] = perms[0].astype(np.int32), np.float64(nu0)
        for i, s in enumerate(steps):
            for k, v in s.items():
                out[f"pl/train/w{i + 1}/{k}"] = v
        for k, v in logs.items():
            out["pl/train/log/" + k.split("/")[1]] = np.float64(v)
        print("train(): 3 steps, logged", {k: round(v, 6) for k, v in logs.items()})
    np.savez_compressed(a.out, **out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
