"""GPU: gSDE (use_sde) against tests/golden/g26_sde.npz — the reference's own policy, autograd and train() at a trained-like state
(tools/gen_sde_golden.py; tests/test_sde_cpu.py checks the fixture against the formulas).

Bounds.  icrl_policy_forward_sde is a float32 MLP forward: 1e-5 of the array's scale against the reference's float32 values, the project's bound for
such outputs.  icrl_policy_sde_fwd_bwd computes in float64 and rounds once, the reference in float32: the unit is the reference's OWN
float32-vs-float64 difference per output / per gradient block, measured by the generator (g26 dev<n>/...), and the kernel is bound by 4 x that —
plus half a float32 spacing of the array's largest value, the rounding of the result itself, which no float32 value can undercut: on one row the
reference's float32 output sometimes lands within 1e-8 of the float64 one by luck (g26 pl/dev1/out/entropy), closer than the correctly rounded value."""
import ctypes
import types

import numpy as np
import pytest
import torch

from helpers import routes as R
from helpers import sde_cases as C

pytestmark = pytest.mark.gpu


def _p(t):
    return None if t is None else t.data_ptr()


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype).contiguous()


def _scale_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


_pols = {}


def _policies(tag):
    """(gSDE policy, diagonal policy with the same network weights), built once per shape"""
    if tag not in _pols:
        _pols[tag] = (C.policy(tag), C.policy(tag, use_sde=False))
    return _pols[tag]


def _forward(pol, obs, expl, stride, deterministic, lo=None, hi=None):
    from icrl_amd import _lib
    n, A = obs.shape[0], pol.act_dim
    out = dict(actions=torch.full((n, A), 7.0, device="cuda"), clipped=torch.full((n, A), 7.0, device="cuda"),
               v_r=torch.empty(n, device="cuda"), v_c=torch.empty(n, device="cuda"), log_prob=torch.empty(n, device="cuda"))
    s = pol.struct(sde=True)
    _lib.check(_lib.lib().icrl_policy_forward_sde(ctypes.byref(s), _p(obs), _p(expl), stride, n, int(deterministic), _p(lo), _p(hi), _p(out["actions"]),
                                                  _p(out["clipped"]), _p(out["v_r"]), _p(out["v_c"]), _p(out["log_prob"]), None), "icrl_policy_forward_sde")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _padded(E):
    """logical [.., H, A] exploration matrices -> the stored [.., 64, A] shape"""
    E = np.asarray(E, np.float32)
    out = np.zeros(E.shape[:-2] + (64, E.shape[-1]), np.float32)
    out[..., :E.shape[-2], :] = E
    return out


@pytest.mark.parametrize("tag", ["hc", "pl"])
@pytest.mark.parametrize("n", [48, 17, 1])
def test_forward_against_the_reference(tag, n):
    g = C.gold()
    pol, diag = _policies(tag)
    A = pol.act_dim
    obs = _dev(g[f"{tag}/obs"][:n], torch.float64)
    # ---- the three branch forwards are icrl_policy_forward's: bit-equal mean and values for the same network weights
    det = _forward(pol, obs, None, 0, 1)
    d_act, d_vr, d_vc, _ = diag.forward(obs, deterministic=True, clip=False)
    torch.cuda.synchronize()
    assert np.array_equal(det["actions"], d_act.cpu().numpy()), "mean"
    assert np.array_equal(det["v_r"], d_vr.cpu().numpy().ravel()) and np.array_equal(det["v_c"], d_vc.cpu().numpy().ravel())
    assert np.array_equal(det["clipped"], det["actions"])
    assert _scale_err(det["actions"], g[f"{tag}/fwd/mean"][:n]) <= 1e-5
    # ---- sampled, one matrix per row
    E = _dev(_padded(g[f"{tag}/E"][:n]))
    out = _forward(pol, obs, E, 64 * A, 0)
    for k in ("actions", "log_prob", "v_r", "v_c"):
        err = _scale_err(out[k], g[f"{tag}/fwd/{k}"][:n])
        print(f"SDE forward {tag} n={n} {k}: {err:.3g} of scale")
        if n > 1 or k in ("actions", "log_prob"):      # (one value near zero is no scale: the single row's values are covered by the bit-equality above)
            assert err <= 1e-5, (k, err)
    assert np.array_equal(out["v_r"], det["v_r"]) and np.array_equal(out["v_c"], det["v_c"])
    # ---- one matrix for all rows (expl_stride 0) = every row with its own copy of it
    E0 = _dev(_padded(g[f"{tag}/E0"]))
    one = _forward(pol, obs, E0, 0, 0)
    rep = _forward(pol, obs, E0.unsqueeze(0).repeat(n, 1, 1).contiguous(), 64 * A, 0)
    assert np.array_equal(one["actions"], rep["actions"]) and np.array_equal(one["log_prob"], rep["log_prob"])
    assert _scale_err(one["actions"], g[f"{tag}/fwd0/actions"][:n]) <= 1e-5 and _scale_err(one["log_prob"], g[f"{tag}/fwd0/log_prob"][:n]) <= 1e-5
    assert not np.array_equal(one["actions"], out["actions"])
    # ---- clipping to [lo, hi]: the raw action, the log-prob of the raw action, the clipped copy
    lo, hi = _dev(np.full(A, -0.25, np.float32)), _dev(np.full(A, 0.125, np.float32))
    cl = _forward(pol, obs, E, 64 * A, 0, lo, hi)
    assert np.array_equal(cl["actions"], out["actions"]) and np.array_equal(cl["log_prob"], out["log_prob"])
    assert np.array_equal(cl["clipped"], np.clip(out["actions"], -0.25, 0.125)) and not np.array_equal(cl["clipped"], cl["actions"])


def test_policy_forward_picks_the_matrices_as_get_noise_does():
    g = C.gold()
    pol, _ = _policies("pl")
    pol.set_noise(g["pl/E0"], g["pl/E"])
    obs = _dev(g["pl/obs"], torch.float64)
    a48 = pol.forward(obs, clip=False)[0].cpu().numpy()
    a17 = pol.forward(obs[:17], clip=False)[0].cpu().numpy()      # 17 rows, 48 matrices: E0
    a1 = pol.forward(obs[:1], clip=False)[0].cpu().numpy()
    assert _scale_err(a48, g["pl/fwd/actions"]) <= 1e-5
    assert _scale_err(a17, g["pl/fwd0/actions"][:17]) <= 1e-5 and np.array_equal(a1, a17[:1])
    assert np.array_equal(pol.predict(obs, deterministic=True)[0].cpu().numpy(), np.clip(pol.forward(obs, deterministic=True)[0].cpu().numpy(), -1, 1))


def _tol(dev, ref):
    return 4.0 * float(dev) + 0.5 * float(np.spacing(np.float32(np.abs(ref).max())))


def _fwd_bwd(pol, obs, act, up=None, grad=True, ws_bytes=None):
    from icrl_amd import _lib
    L = _lib.lib()
    n = obs.shape[0]
    s = pol.struct(sde=True)
    outs = {k: torch.empty(n, device="cuda") for k in C.OUTS}
    g = ws = None
    need = 0
    if grad:
        need = int(L.icrl_policy_sde_fwd_bwd_ws_bytes(ctypes.byref(s), n))
        assert need == min((n + 15) // 16, 64) * pol.n_params * 8
        g = torch.full((pol.n_params,), float("nan"), device="cuda")
        ws = torch.full(((need + 7) // 8,), float("nan"), dtype=torch.float64, device="cuda")
    d = {k: None if up is None or up.get(k) is None else _dev(up[k]) for k in ("d_v_r", "d_v_c", "d_log_prob", "d_entropy")}
    err = L.icrl_policy_sde_fwd_bwd(ctypes.byref(s), _p(obs), _p(act), n, _p(d["d_v_r"]), _p(d["d_v_c"]), _p(d["d_log_prob"]), _p(d["d_entropy"]), _p(outs["v_r"]),
                                    _p(outs["v_c"]), _p(outs["log_prob"]), _p(outs["entropy"]), _p(g), _p(ws), need if ws_bytes is None else ws_bytes, None)
    _lib.check(err, "icrl_policy_sde_fwd_bwd")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in outs.items()}, None if g is None else g.cpu().numpy()


@pytest.mark.parametrize("tag,n", [("hc", 48), ("pl", 48), ("pl", 17), ("pl", 1), ("hc", 17), ("hc", 1)])
def test_fwd_bwd_against_the_reference(tag, n):
    g = C.gold()
    pol, _ = _policies(tag)
    obs, act = _dev(g[f"{tag}/obs"][:n]), _dev(g[f"{tag}/act"][:n])
    up = C.upstream(tag, n)
    out, grad = _fwd_bwd(pol, obs, act, up)
    for k in C.OUTS:
        dev = float(g[f"{tag}/dev{n}/out/{k}"])
        err = float(np.abs(out[k].astype(np.float64) - g[f"{tag}/ev{n}/{k}"]).max())
        print(f"SDE fwd_bwd {tag} n={n} {k}: |kernel - reference float32| {err:.3g}, the reference's float32 error {dev:.3g}")
        assert err <= _tol(dev, g[f"{tag}/ev{n}/{k}"]), (k, err, dev)
        assert np.abs(out[k] - g[f"{tag}/ev{n}_64/{k}"]).max() <= _tol(dev, g[f"{tag}/ev{n}/{k}"])
    blocks, pads = C.split_grad(pol, grad)
    assert pads.size == pol.n_params - sum(int(np.prod(s)) for s in pol.logical_shapes.values()) and not pads.any(), "padding entries of the gradient"
    assert (pads.size > 63 * pol.act_dim) == (tag == "pl")
    assert np.isfinite(grad).all()
    if f"{tag}/g{n}/log_std" in g:      # (the ragged and the one-row gradients are recorded for the padded shape)
        for k, b in blocks.items():
            dev, ref = float(g[f"{tag}/dev{n}/{k}"]), g[f"{tag}/g{n}/{k}"]
            err = float(np.abs(b.astype(np.float64) - ref).max())
            print(f"SDE fwd_bwd {tag} n={n} grad {k}: |kernel - reference float32| {err:.3g}, the reference's float32 error {dev:.3g}, max |grad| {np.abs(ref).max():.3g}")
            assert b.shape == ref.shape and err <= _tol(dev, ref), (k, err, dev)
    else:      # the formulas' float64 log_std gradient (tests/test_sde_cpu.py ties them to the fixture)
        _, g_ls = C.head_numpy(C.state(tag), g[f"{tag}/obs"][:n], g[f"{tag}/act"][:n], up)
        assert _scale_err(blocks["log_std"], g_ls) <= 1e-6
    # ---- forward only: the same output bits; a second call: the same bits everywhere
    fo, none = _fwd_bwd(pol, obs, act, None, grad=False)
    assert none is None and all(np.array_equal(fo[k], out[k]) for k in C.OUTS)
    out2, grad2 = _fwd_bwd(pol, obs, act, up)
    assert all(np.array_equal(out2[k], out[k]) for k in C.OUTS) and np.array_equal(grad2, grad)


@pytest.mark.parametrize("tag", ["hc", "pl"])
def test_the_latent_is_detached_in_the_variance(tag):
    """an entropy-only upstream reaches log_std and nothing else: with learn_features semantics (the variance's gradient flowing into the latent)
    the policy branch would receive a gradient"""
    g = C.gold()
    pol, _ = _policies(tag)
    obs, act = _dev(g[f"{tag}/obs"]), _dev(g[f"{tag}/act"])
    _, grad = _fwd_bwd(pol, obs, act, dict(d_entropy=g[f"{tag}/up/d_entropy"]))
    blocks, _ = C.split_grad(pol, grad)
    assert np.abs(blocks["log_std"]).min() > 0
    for k, b in blocks.items():
        if k != "log_std":
            assert not b.any(), k
    _, g_ls = C.head_numpy(C.state(tag), g[f"{tag}/obs"], g[f"{tag}/act"], dict(d_log_prob=np.zeros(48), d_entropy=g[f"{tag}/up/d_entropy"]))
    assert _scale_err(blocks["log_std"], g_ls) <= 1e-6
    # zeros given explicitly = NULL
    z = np.zeros(48, np.float32)
    _, grad0 = _fwd_bwd(pol, obs, act, dict(d_v_r=z, d_v_c=z, d_log_prob=z, d_entropy=g[f"{tag}/up/d_entropy"]))
    assert np.array_equal(grad0, grad)


def test_a_small_workspace_is_refused_without_a_launch():
    g = C.gold()
    pol, _ = _policies("pl")
    obs, act = _dev(g["pl/obs"]), _dev(g["pl/act"])
    with pytest.raises(ValueError, match=r"ws of \d+ bytes, icrl_policy_sde_fwd_bwd_ws_bytes\(pol, 48\)"):
        _fwd_bwd(pol, obs, act, C.upstream("pl", 48), ws_bytes=3 * pol.n_params * 8 - 8)
    with pytest.raises(ValueError, match="n_params"):      # the diagonal entry point refuses the gSDE buffer
        pol.use_sde = False
        try:
            pol.evaluate_actions(obs.double(), act)
        finally:
            pol.use_sde = True


# ---- the agent -------------------------------------------------------------------------------------------------------------------------------
def test_three_teacher_forced_train_steps_follow_the_reference():
    from icrl_amd import logger
    from icrl_amd.ppo_lag import PPOLagrangian
    g = C.gold()
    O, A, arch = C.SHAPES["pl"]
    T, N = 48, 2
    o, a = C.spaces_of("pl")
    env = types.SimpleNamespace(num_envs=N, observation_space=o, action_space=a)
    logger.configure()
    agent = PPOLagrangian("TwoCriticsMlpPolicy", env, n_steps=T, batch_size=32, n_epochs=1, target_kl=None, penalty_initial_value=1, penalty_learning_rate=0.1,
                          budget=0.0, use_sde=True, sde_sample_freq=8, policy_kwargs=dict(net_arch=[dict(arch)]))
    agent.policy.load_state_dict({k: torch.as_tensor(v) for k, v in C.state("pl").items()})
    assert abs(float(agent.dual.nu().item()) - float(g["pl/train/nu0"])) <= 1e-6
    rb = agent.rollout_buffer
    for k in ("observations", "actions", "log_probs", "reward_values", "cost_values", "reward_advantages", "cost_advantages", "reward_returns", "cost_returns",
              "orig_costs"):
        plane = getattr(rb, k)
        flat = g[f"pl/train/buf/{k}"]      # env-major: row = env * T + t
        plane.copy_(torch.as_tensor(flat.reshape((N, T) + tuple(plane.shape[2:])).swapaxes(0, 1).copy()).to(plane.dtype))
    rb.full, rb.pos = True, T
    steps = []
    agent.sde_step_hook = lambda e, i: steps.append(agent.policy.state_dict())
    agent.train(perms=g["pl/train/perm"][None])
    assert len(steps) == 3 and agent.policy.adam_step == 3
    # the gradient blocks' bound — 4 x the reference's float32-vs-float64 difference of that block (g26 dev48) — times the step count, in the
    # parameters' own unit, plus one float32 spacing of the block's largest parameter per step (both sides store float32 parameters).  (With
    # lr = 3e-4 and Adam's eps = 1e-5 a gradient off by delta moves a parameter by at most lr * delta / eps = 30 delta, and only where |g| << eps.)
    lr = 3e-4
    for i, sd in enumerate(steps):
        for k, v in sd.items():
            ref = g[f"pl/train/w{i + 1}/{k}"]
            tol = (i + 1) * (4.0 * float(g[f"pl/dev48/{k}"]) + float(np.spacing(np.float32(np.abs(ref).max()))))
            err = float(np.abs(v.numpy().astype(np.float64) - ref).max())
            print(f"SDE train step {i + 1} {k}: max |parameter - reference| = {err:.3g} ({err / lr:.3g} of a step), bound {tol:.3g}")
            assert v.shape == ref.shape and err <= tol, (i, k, err, tol)
    moved = np.abs(steps[-1]["log_std"].numpy() - g["pl/w/log_std"]).max()
    assert 0.5 * lr < moved < 3.5 * lr
    log = logger.Logger.CURRENT.name_to_value
    # float32 means of float32 terms on both sides: 1e-5 of the value where it is a sum of like-signed terms, 1e-4 where it is a small difference of
    # larger ones (the surrogate loss, the KL estimate: means of differences of log-probs of magnitude 5..10)
    for key, tol in (("entropy_loss", 1e-5), ("policy_gradient_loss", 1e-4), ("reward_value_loss", 1e-5), ("cost_value_loss", 1e-5), ("approx_kl", 1e-4),
                     ("clip_fraction", 1e-6), ("loss", 1e-5), ("mean_reward_advantages", 1e-5), ("mean_cost_advantages", 1e-5), ("reward_explained_variance", 1e-5),
                     ("cost_explained_variance", 1e-5), ("nu", 1e-6), ("nu_loss", 1e-6), ("average_cost", 1e-6), ("total_cost", 1e-6), ("early_stop_epoch", 0),
                     ("std", 1e-6), ("n_updates", 0), ("clip_range", 1e-7), ("learning_rate", 1e-9)):
        want, got = float(g[f"pl/train/log/{key}"]), float(log["train/" + key])
        print(f"SDE train log {key}: {got!r} (reference {want!r})")
        assert abs(got - want) <= tol * max(1.0, abs(want)), (key, got, want)
    # the padding stayed zero through three Adam steps
    A_ = agent.policy.act_dim
    assert not agent.policy.params[:64 * A_].reshape(64, A_)[48:].any() and not agent.policy.exp_avg[:64 * A_].reshape(64, A_)[48:].any()


_CPG = ("-tei", "HCWithPos-v0", "-eei", "HCWithPosTest-v0", "-nt", "4", "--n_steps", "32", "-t", "256")


def _setup(extra, seed=0, timesteps=None):
    from icrl_amd import cpg as Cpg
    from icrl_amd.streams import PrivateStreams
    cfg = vars(Cpg.build_parser().parse_args(["cpg", *_CPG, "-s", str(seed), "-v", "0", *extra]))
    cfg.update(rank=0, world_size=1, streams=PrivateStreams(seed), eval_noise_from_streams=True)
    cfg = types.SimpleNamespace(**cfg)
    return cfg, Cpg.setup(cfg, log=None)


def test_learn_collects_with_the_matrices_it_holds_and_trains_log_std(tmp_path):
    from icrl_amd.ppo_lag import PPOLagrangian
    cfg, (model, _cb, learn_cost, _hist) = _setup(["-us", "-ssf", "8", "-bs", "16", "-ne", "2"])
    assert model.use_sde and model.sde_sample_freq == 8 and model.policy.use_sde
    pol, rb = model.policy, model.rollout_buffer
    held, orig = [], pol.reset_noise

    def recording(n_envs=1, streams=None):
        orig(n_envs, streams)
        held.append((rb.pos, pol.sde_E.clone()))
    pol.reset_noise = recording
    ls0 = pol.log_std.clone()
    w0 = pol.params.clone()
    pol.reset_noise = recording
    model._setup_learn(128)
    assert model.collect_rollouts(model.env, None, rb, 32, learn_cost) is True
    assert [t for t, _ in held] == [0, 0, 8, 16, 24]      # the rollout's own draw, then the cadence's (both at step 0, as in the reference)
    mats = {t: E for t, E in held}
    assert all(not torch.equal(mats[a], mats[b]) for a, b in ((0, 8), (8, 16), (16, 24)))
    assert torch.equal(pol.params, w0)
    # actions = mean + latent . E[env], recomputed from the buffer's observations with the matrices held at that step
    sd = {k: v.numpy() for k, v in pol.state_dict().items()}
    obs, act = rb.observations.cpu().numpy(), rb.actions.cpu().numpy()
    for t in range(32):
        E = mats[8 * (t // 8)][:, :64].cpu().numpy().astype(np.float64)
        out, _ = C.head_numpy(sd, obs[t], act[t])
        want = out["mean"] + np.einsum("nh,nha->na", out["latent"], E)
        assert np.abs(act[t] - want).max() <= 1e-5 * max(1.0, np.abs(want).max()), t
        assert np.abs(rb.log_probs[t].cpu().numpy() - out["log_prob"]).max() <= 1e-5 * np.abs(out["log_prob"]).max()
    model.train()
    assert not torch.equal(pol.log_std, ls0) and pol.adam_step == 2 * (128 // 16)
    pol.reset_noise = orig
    model.learn(total_timesteps=128, cost_function=learn_cost)      # learn() itself, once more from a reset
    path = model.save(str(tmp_path / "sde_agent"))
    back = PPOLagrangian.load(path, env=model.env)
    assert back.use_sde and back.sde_sample_freq == 8 and torch.equal(back.policy.params, pol.params)
    o = model._last_obs
    back.policy.set_noise(pol.sde_E0[:64], pol.sde_E[:, :64])
    for det in (True, False):
        assert torch.equal(back.predict(o, deterministic=det)[0], model.predict(o, deterministic=det)[0])
    with pytest.raises(ValueError, match="holds a gSDE policy"):
        PPOLagrangian.load(path, env=model.env, use_sde=False)


def test_cpg_with_the_flag_end_to_end():
    cfg, (model, cb, learn_cost, hist) = _setup(["-us"])
    model.learn(total_timesteps=int(cfg.timesteps), cost_function=learn_cost, callback=cb)
    assert model.num_timesteps == 256 and len(hist.history) >= 1 and torch.isfinite(model.policy.params).all()
    assert not torch.equal(model.policy.log_std, torch.zeros_like(model.policy.log_std))


def test_without_the_flag_the_same_run_takes_the_fused_routes():
    cfg, (model, cb, learn_cost, hist) = _setup([])
    assert not model.use_sde and not model.policy.use_sde and model.policy.n_params == 16654
    model._setup_learn(128)
    assert model.collect_rollouts(model.env, None, model.rollout_buffer, 32, learn_cost) is True
    R.check_rollout(dict(route="persistent", wgs=4, launches=1, n_runs=1), "cpg without -us: rollout")
    model.train()
    R.check_update(dict(kind=5, wgs_per_network=4, n_runs=1), "cpg without -us: update")
    # and a gSDE agent's rollout and update call no fused entry point: the records stay
    cfg, (sde, cb, learn_cost, hist) = _setup(["-us"])
    sde._setup_learn(128)
    assert sde.collect_rollouts(sde.env, None, sde.rollout_buffer, 32, learn_cost) is True
    sde.train()
    R.check_rollout(dict(route="persistent", wgs=4, launches=1, n_runs=1), "the gSDE rollout calls no rollout entry point: the record stays")
    R.check_update(dict(kind=5, wgs_per_network=4, n_runs=1), "the gSDE update calls no update entry point: the record stays")
