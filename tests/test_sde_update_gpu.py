"""The gSDE update as one persistent launch (icrl_ppo_lag_train_sde, csrc/ppo_train_sde.hip) against the fine-grained loop on the same agent
state, buffer and permutations (helpers/sde_update_cases.py), and against golden g26 where the fixture holds the reference's own train().

The yardstick is the loop (ICRL_SDE_UPDATE_STEPPED=1): float64 rounded once, pinned to the reference by test_sde_gpu.py.  The launch is an fp32
evaluation in another order, so its bounds are the project's for an fp32 persistent update against its reference-equivalent
(tests/test_ppo_train_gpu.py): parameters 5e-4 x lr x steps + 2e-7, the seven train/* scalars 2e-4 + 2e-3 |x|, per-epoch KLs atol 2e-5, the same
early-stop epoch.  Every case prints its measured fraction of the parameter bound (SDE_ADAM_DEV)."""
import ctypes
import types

import numpy as np
import pytest
import torch

from helpers import routes as R
from helpers import sde_cases as C
from helpers import sde_update_cases as U

pytestmark = pytest.mark.gpu


def _padding_is_zero(pol, rows_from):
    A = pol.act_dim
    for flat in (pol.params, pol.exp_avg, pol.exp_avg_sq):
        assert not flat[:64 * A].reshape(64, A)[rows_from:].any()
    mask = torch.as_tensor(~U.real_mask(pol), device=pol.params.device)
    for flat in (pol.params, pol.exp_avg, pol.exp_avg_sq):
        assert not flat[mask].any()


def test_golden_g26_three_steps_through_the_fused_call():
    """pl: obs 11, act 3, pi [32, 48]; T 48, N 2, B 32, one epoch: the fixture's buffer and permutation, the reference's parameters after 3 steps."""
    from icrl_amd import logger
    g = C.gold()
    O, A, arch = C.SHAPES["pl"]
    T, N = 48, 2
    agent = U.make_agent(O, A, T, N, 32, 1, arch=arch, target_kl=None)
    agent.update_penalty_after = 1      # (the constructor's default: the reference's run steps its dual variable: the log holds nu after it)
    agent.policy.load_state_dict({k: torch.as_tensor(v) for k, v in C.state("pl").items()})
    assert abs(float(agent.dual.nu().item()) - float(g["pl/train/nu0"])) <= 1e-6
    rb = agent.rollout_buffer
    for k in ("observations", "actions", "log_probs", "reward_values", "cost_values", "reward_advantages", "cost_advantages", "reward_returns", "cost_returns",
              "orig_costs"):
        plane = getattr(rb, k)
        flat = g[f"pl/train/buf/{k}"]      # env-major: row = env * T + t
        plane.copy_(torch.as_tensor(flat.reshape((N, T) + tuple(plane.shape[2:])).swapaxes(0, 1).copy()).to(plane.dtype))
    rb.full, rb.pos = True, T
    agent.train(perms=g["pl/train/perm"][None])
    assert agent.last_sde_update == "fused" and agent.policy.adam_step == 3
    lr, worst = 3e-4, 0.0
    bound = U.ADAM_DEV_BOUND * lr * 3 + 2e-7
    for k, v in agent.policy.state_dict().items():
        ref = g[f"pl/train/w3/{k}"]
        err = float(np.abs(v.numpy().astype(np.float64) - ref).max())
        worst = max(worst, err)
        print(f"SDE fused g26 {k}: max |parameter - reference| = {err:.3g} ({err / bound:.3g} of the bound {bound:.3g})")
        assert v.shape == ref.shape
    print(f"SDE_ADAM_DEV g26-pl steps=3: max |fused - reference| = {worst:.3g} = {worst / bound:.3g} of the bound {bound:.3g}")
    assert worst <= bound, (worst, bound)
    log = logger.Logger.CURRENT.name_to_value
    for key, tol in (("entropy_loss", 1e-5), ("policy_gradient_loss", 1e-4), ("reward_value_loss", 1e-5), ("cost_value_loss", 1e-5), ("approx_kl", 1e-4),
                     ("clip_fraction", 1e-6), ("loss", 1e-5), ("mean_reward_advantages", 1e-5), ("mean_cost_advantages", 1e-5), ("reward_explained_variance", 1e-5),
                     ("cost_explained_variance", 1e-5), ("nu", 1e-6), ("nu_loss", 1e-6), ("average_cost", 1e-6), ("total_cost", 1e-6), ("early_stop_epoch", 0),
                     ("std", 1e-6), ("n_updates", 0), ("clip_range", 1e-7), ("learning_rate", 1e-9)):
        want, got = float(g[f"pl/train/log/{key}"]), float(log["train/" + key])
        print(f"SDE fused train log {key}: {got!r} (reference {want!r})")
        assert abs(got - want) <= tol * max(1.0, abs(want)), (key, got, want)
    _padding_is_zero(agent.policy, 48)


WALKS = [(4, 32, 64, 3),      # 128 rows: two full minibatches per epoch
         (5, 20, 64, 2),      # 100 rows: 64 + 36 (ragged)
         (5, 40, 128, 2),     # 200 rows: 128 + 72 = chunks 64 + 64 and 64 + 8
         (4, 8, 16, 2)]       # 32 rows: 16 + 16 (a minibatch below one row tile of a chunk)


@pytest.mark.parametrize("N,T,B,E", WALKS)
def test_hc_walks_follow_the_loop(N, T, B, E):
    agent, sd, perms, snap = U.case(18, 6, T, N, B, E, seed=N * T + B, target_kl=None)
    fused, loop, frac = U.both(f"hc {N}x{T} B={B} E={E}", agent, perms, snap)
    n_mb = -(-N * T // B)
    assert fused["adam_step"] - snap["adam_step"] == E * n_mb
    assert not np.array_equal(fused["params"][:64 * 6], snap["params"][:64 * 6].cpu().numpy())      # log_std moved
    _padding_is_zero(agent.policy, 64)


def test_obs_40_act_4_ragged_walk_follows_the_loop():
    """obs 40, act 4, 5 x 20 rows at batch 64 (64 + 36): the four-tile instantiation, between the two-tile HC walks above and the eight-tile case below."""
    agent, sd, perms, snap = U.case(40, 4, 20, 5, 64, 2, seed=40, target_kl=None)
    fused, loop, frac = U.both("obs40 5x20 B=64 E=2", agent, perms, snap)
    assert fused["adam_step"] - snap["adam_step"] == 4
    assert not np.array_equal(fused["params"][:64 * 4], snap["params"][:64 * 4].cpu().numpy())      # log_std moved
    _padding_is_zero(agent.policy, 64)


def test_hyper_parameters_off_their_defaults():
    kw = dict(clip_range_reward_vf=0.2, clip_range_cost_vf=0.3, ent_coef=0.01, reward_vf_coef=0.7, cost_vf_coef=0.3, max_grad_norm=0.3)
    agent, sd, perms, snap = U.case(18, 6, 32, 4, 64, 2, seed=3, target_kl=None, **kw)
    norms = []
    hook = lambda e, i: norms.append(agent._train_ws["sde"]["out2"].cpu().numpy().copy())      # {total norm, clip coefficient} of the step just made
    fused, loop, frac = U.both("hc 4x32 B=64 E=2 hparams", agent, perms, snap, hook=hook)
    assert len(norms) == 4
    print("SDE hparams: the loop's gradient norms and clip coefficients per step:", [(float(a), float(b)) for a, b in norms])
    assert all(n > 0.3 * 1.05 and c < 1.0 for n, c in norms), norms      # the norm clip is active at every step
    # the entropy bonus reaches log_std through the variance: the same case without it ends elsewhere
    restore_kw = dict(kw, ent_coef=0.0)
    agent0, _, perms0, snap0 = U.case(18, 6, 32, 4, 64, 2, seed=3, target_kl=None, **restore_kw)
    assert np.array_equal(perms0, perms) and torch.equal(snap0["params"], snap["params"])
    U.restore(agent0, snap0)
    other = U.run(agent0, perms0, stepped=False)
    assert np.abs(other["params"][:64 * 6] - fused["params"][:64 * 6]).max() > 1e-6


def test_the_target_kl_stop_is_decided_at_the_same_epoch():
    # learning_rate 3e-3: the KL estimate mean(old log-prob - log-prob) of 128 rows must outgrow its own noise within three epochs
    agent, sd, perms, snap = U.case(18, 6, 32, 4, 64, 6, seed=12, target_kl=None, learning_rate=3e-3)
    U.restore(agent, snap)
    free = U.run(agent, perms, stepped=True)
    kls = free["epoch_kls"]
    print("SDE target-KL: the loop's per-epoch KLs without a target:", kls.tolist())
    assert free["early_stop_epoch"] == 6
    limit = 0.5 * (float(kls[1]) + float(kls[2]))
    assert abs(float(kls[1]) - limit) >= 2e-4 and abs(float(kls[2]) - limit) >= 2e-4, (kls, limit)      # ten times the KL tolerance
    assert float(kls[0]) < limit and float(kls[1]) < limit < float(kls[2]), (kls, limit)
    agent.target_kl = limit / 1.5
    fused, loop, frac = U.both("hc 4x32 B=64 E=6 target_kl", agent, perms, snap)
    assert fused["early_stop_epoch"] == loop["early_stop_epoch"] == 2
    assert fused["adam_step"] - snap["adam_step"] == 3 * 2


def test_the_same_fused_call_twice_gives_the_same_bits():
    agent, sd, perms, snap = U.case(18, 6, 20, 5, 64, 2, seed=5, target_kl=None, ent_coef=0.01)
    runs = []
    for _ in range(2):
        U.restore(agent, snap)
        runs.append(U.run(agent, perms, stepped=False))
    for k in ("params", "exp_avg", "exp_avg_sq", "stats"):
        assert np.array_equal(runs[0][k], runs[1][k]), k
    assert runs[0]["adam_step"] == runs[1]["adam_step"] == snap["adam_step"] + 4


def test_the_next_rollout_sees_the_update():
    agent, sd, perms, snap = U.case(18, 6, 32, 4, 64, 2, seed=7, target_kl=None)
    U.restore(agent, snap)
    U.run(agent, perms, stepped=False)
    pol = agent.policy
    obs = np.random.RandomState(1).randn(8, 18)
    n, A = 8, pol.act_dim
    f = lambda *s: torch.zeros(*s, device="cuda")
    actions, clipped, v_r, v_c, lp = f(n, A), f(n, A), f(n), f(n), f(n)
    s = pol.struct(sde=True)
    from icrl_amd import _lib
    o = torch.as_tensor(obs, dtype=torch.float64, device="cuda").contiguous()
    _lib.check(_lib.lib().icrl_policy_forward_sde(ctypes.byref(s), o.data_ptr(), None, 0, n, 1, None, None, actions.data_ptr(), clipped.data_ptr(), v_r.data_ptr(),
                                                  v_c.data_ptr(), lp.data_ptr(), _lib.current_stream()), "icrl_policy_forward_sde")
    new_sd = {k: v.numpy() for k, v in pol.state_dict().items()}
    assert any(not np.array_equal(new_sd[k], sd[k]) for k in sd)
    want, _ = C.head_numpy(new_sd, obs, actions.cpu().numpy())
    old, _ = C.head_numpy(sd, obs, actions.cpu().numpy())
    for got, key in ((actions, "mean"), (v_r, "v_r"), (v_c, "v_c"), (lp, "log_prob")):
        got = got.cpu().numpy().astype(np.float64)
        err = float(np.abs(got - want[key]).max() / np.abs(want[key]).max())
        print(f"SDE forward after the fused update, {key}: {err:.3g} of scale")
        assert err <= 1e-5, (key, err)
    assert np.abs(old["mean"] - want["mean"]).max() > 1e-4      # ... and not what the state before the update gives


_CPG = ("-tei", "HCWithPos-v0", "-eei", "HCWithPosTest-v0", "-nt", "4", "--n_steps", "32", "-t", "256")


def _setup(extra, seed=0):
    from icrl_amd import cpg as Cpg
    from icrl_amd.streams import PrivateStreams
    cfg = vars(Cpg.build_parser().parse_args(["cpg", *_CPG, "-s", str(seed), "-v", "0", *extra]))
    cfg.update(rank=0, world_size=1, streams=PrivateStreams(seed), eval_noise_from_streams=True)
    cfg = types.SimpleNamespace(**cfg)
    return cfg, Cpg.setup(cfg, log=None)


@pytest.mark.parametrize("how,bs,want", [("default", 16, "fused"), ("env", 16, "loop"), ("hook", 16, "loop"), ("bs256", 256, "loop")])
def test_routing_through_cpg_setup(how, bs, want, monkeypatch):
    monkeypatch.delenv("ICRL_SDE_UPDATE_STEPPED", raising=False)
    cfg, (model, _cb, learn_cost, _hist) = _setup(["-us", "-bs", str(bs), "-ne", "2"])
    model._setup_learn(128)
    assert model.collect_rollouts(model.env, None, model.rollout_buffer, 32, learn_cost) is True
    if how == "env":
        monkeypatch.setenv("ICRL_SDE_UPDATE_STEPPED", "1")
    if how == "hook":
        model.sde_step_hook = lambda e, i: None
    before = R.update()
    model.train()
    assert model.last_sde_update == want, (model.last_sde_update, model.last_sde_update_reason)
    assert model.policy.adam_step == 2 * -(-128 // bs)
    assert R.update() == before, "the gSDE update must leave the update family's route record as it was"
    assert torch.isfinite(model.policy.params).all()


def test_obs_113_act_8_batch_128_follows_the_loop():
    """obs 113, act 8, batch 128, 3 x 50 rows (128 + 22: chunks 64 + 64 and 22): the eight-tile instantiation, whose LDS images fit because the
    variances live in spare columns of the dz2 rows."""
    agent, sd, perms, snap = U.case(113, 8, 50, 3, 128, 2, seed=9, target_kl=None)
    fused, loop, frac = U.both("ant 3x50 B=128 E=2", agent, perms, snap)
    assert fused["adam_step"] - snap["adam_step"] == 4
    assert not np.array_equal(fused["params"][:64 * 8], snap["params"][:64 * 8].cpu().numpy())
    _padding_is_zero(agent.policy, 64)
