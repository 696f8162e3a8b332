"""Policy states away from the one PPOLagrangian.__init__ leaves (log_std = 0: sigma = 1, log sigma = 0, 2 sigma^2 = 2 sigma = 2; an action
head of gain 0.01: means of ~0.005, no deterministic action near a bound), and the conditions every test asserts FROM THE ORACLE'S
BUFFERS before it looks at a kernel.  At the fresh state a Gaussian head that drops -log sigma, confuses sigma with sigma^2, reads
log_std[0] for every action or skips the clip of the deterministic action passes every kernel-level test.

States are named by strings so that they can be part of a cache key:
  "shaped"   log_std per action as below (LOG_STD's rows for 6 and 8 actions, log_std_rule for every other width), action_net.weight x 50, action_net.bias = RandomState(99).uniform(-0.9, 0.9): any architecture
  "ref"      policy.pth out of tests/golden/ref_artifacts/hc_best_model.zip (the reference's trained HalfCheetah policy; 18 -> 64-64 -> 6)
and "<state>/<counter>" is a counter-state, used on the oracle's side only, to prove that the inputs discriminate:
  zero_log_std      log_std = 0
  uniform_log_std   every entry of log_std replaced by their mean
  fresh_head        the action head of the freshly initialised policy
"""
import io
import os
import zipfile

import numpy as np
import torch

from helpers import norm_cases as nc

LOG_STD = {6: [-0.6385, -0.9999, -0.6585, -1.0631, -1.0151, -0.8097],      # (hc_best_model.zip's, to four digits)
           8: [-1.2, 0.35, -0.7, -0.2, -1.0, 0.1, -0.45, -0.9]}               # both signs: sigma on both sides of 1
HEAD_SCALE, BIAS_SEED, BIAS_RANGE = 50.0, 99, 0.9


def log_std_rule(act_dim):
    """log_std of `shaped` at an action width LOG_STD has no row for: even actions -1.2, -1.07, ... (+0.13 each), odd actions 0.1, 0.14, ...
    (+0.04 each) — up to 16 actions that is [-1.2, -0.29] beside [0.1, 0.38]: every |log_std| >= 0.1, every pair at least 0.03 apart, sigma on
    both sides of 1 from 2 actions on, and neighbours in the head's lane order (actions o, o + 4, o + 8, ...) never neighbours in value."""
    assert 1 <= act_dim <= 16, act_dim
    ls = [(-1.2 + 0.13 * (a // 2)) if a % 2 == 0 else (0.1 + 0.04 * (a // 2)) for a in range(act_dim)]
    check_log_std(ls)
    assert act_dim == 1 or (min(ls) < 0 < max(ls)), ls
    return ls


def log_std_of(act_dim):
    return LOG_STD[act_dim] if act_dim in LOG_STD else log_std_rule(act_dim)
REF_ZIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "ref_artifacts", "hc_best_model.zip")
MIN_SHIFT = nc.MIN_SHIFT
BEYOND = (0.02, 0.7)          # C3: share of the stored actions beyond each action bound
MEAN_STD = 0.1                # C4
DET_SHARE, DET_COUNT = 0.003, 5      # C5
# categorical head (LGW): action_net.weight x LGW_K; on the oracle the largest class probability is >= 0.9 in >= 10 % of the rows and
# <= 0.5 in >= 10 % (found on the CPU: 18 obs x 5 classes holds both shares for k = 400..540, 40 x 16 for k = 450..1000; tests/test_policy_state_cpu.py asserts the two shares)
LGW_K = 500.0
LGW_SHARE = 0.1
# the samplers on LGW / CLGW (two classes: the largest probability is never below 0.5, so "no favourite" is pmax <= 0.6 there): agent seed 4 and
# action_net.weight x 4000 give pmax >= 0.9 in ~20 % and pmax <= 0.6 in ~35 % of the rows the oracle's episodes visit (seeds 1, 2, 3, 6, 7 reach
# only one of the two shares at any k tried; seed 4 holds both for k = 2500 .. 6000)
LGW_SAMPLER_SEED, LGW_SAMPLER_K, LGW_NO_FAVOURITE = 4, 4000.0, 0.6
LGW_DRAW_MARGIN = 1e-5      # every uniform is at least this far from its class boundary on the oracle (the kernels' softmax: ~1e-7): same actions


def _t(v):
    return v.detach().clone().float() if torch.is_tensor(v) else torch.as_tensor(np.asarray(v), dtype=torch.float32).clone()


def shaped(sd, act_dim):
    """the `shaped` state on top of a fresh state dict (a new dict; sd is left alone)."""
    out = {k: _t(v) for k, v in sd.items()}
    out["log_std"] = torch.tensor(log_std_of(act_dim), dtype=torch.float32)
    out["action_net.weight"] = out["action_net.weight"] * HEAD_SCALE
    out["action_net.bias"] = torch.as_tensor(np.random.RandomState(BIAS_SEED).uniform(-BIAS_RANGE, BIAS_RANGE, act_dim).astype(np.float32))
    return out


_REF = []


def ref():
    """policy.pth of the reference's trained HalfCheetah agent (a new dict of float32 tensors)."""
    if not _REF:
        with zipfile.ZipFile(REF_ZIP) as z:
            _REF.append(torch.load(io.BytesIO(z.read("policy.pth")), map_location="cpu", weights_only=True))
    return {k: _t(v) for k, v in _REF[0].items()}


def state(name, fresh_sd, act_dim):
    """the state dict of a named state ("shaped", "ref", "fresh" / None, or "<state>/<counter>") on top of the fresh one."""
    base, _, counter = (name or "fresh").partition("/")
    fresh = {k: _t(v) for k, v in fresh_sd.items()}
    if base == "ref":
        sd = ref()
        assert list(sd) == list(fresh) and all(sd[k].shape == fresh[k].shape for k in sd), "`ref` serves HalfCheetah shapes with the 64-64 architecture only"
    else:
        sd = {"fresh": lambda: fresh, "shaped": lambda: shaped(fresh, act_dim)}[base]()
    if counter == "zero_log_std":
        sd["log_std"] = torch.zeros_like(sd["log_std"])
    elif counter == "uniform_log_std":
        sd["log_std"] = torch.full_like(sd["log_std"], float(sd["log_std"].double().mean()))
    elif counter == "fresh_head":
        sd["action_net.weight"], sd["action_net.bias"] = fresh["action_net.weight"], fresh["action_net.bias"]
    else:
        assert not counter, name
    return sd


COUNTERS = ("zero_log_std", "uniform_log_std", "fresh_head")


# ---- conditions -----------------------------------------------------------------------------------------------------------------------------------
def check_log_std(log_std):
    """C1: every |log_std[a]| >= 0.1, pairwise differences >= 0.01 (from 2 actions on); 8 actions: both signs."""
    ls = np.asarray(log_std, np.float64).ravel()
    assert np.abs(ls).min() >= 0.1, ls
    d = np.abs(ls[:, None] - ls[None, :])[~np.eye(ls.size, dtype=bool)]
    assert d.size == 0 or d.min() >= 0.01, ls
    if ls.size == 8:
        assert (ls > 0).any() and (ls < 0).any(), ls


def rollout_means(o):
    """[T, N, A] action means of an oracle rollout: actions - noise exp(log_std), in float64."""
    sigma = np.exp(np.asarray(o["policy_sd"]["log_std"], np.float64))
    return o["buf"].actions.astype(np.float64) - o["noise"].astype(np.float64) * sigma


def check_rollout(o, counters, rtol, atol):
    """C1..C4 of a fused-rollout case.  o: nc.oracle_buf(..., policy_state=<state>); counters: counter name -> the oracle's rollout under
    "<state>/<counter>" (same seeds, same noise).  Returns the measured figures."""
    b = o["buf"]
    check_log_std(o["policy_sd"]["log_std"])
    fig = {}
    for name, planes in (("zero_log_std", ("actions", "log_probs")), ("uniform_log_std", ("actions",)), ("fresh_head", ("actions",))):
        for k in planes:
            fig[name, k] = nc.in_bounds(getattr(counters[name]["buf"], k), getattr(b, k), rtol, atol)
            assert fig[name, k] >= MIN_SHIFT, (name, k, fig[name, k])
    for side, share in (("+", float(np.mean(b.actions > 1.0))), ("-", float(np.mean(b.actions < -1.0)))):
        fig["beyond", side] = share
        assert BEYOND[0] <= share <= BEYOND[1], (side, share)
    fig["mean_std"] = float(rollout_means(o).reshape(-1, b.actions.shape[-1]).std(axis=0).min())
    assert fig["mean_std"] >= MEAN_STD, fig["mean_std"]
    return fig


def rollout_case(kind, N, T, pstate, **how):
    """the oracle's rollout under a policy state and its three counter-runs (each computed once and shared)."""
    o = nc.oracle_buf(kind, N, T, {}, policy_state=pstate, **how)
    return o, {c: nc.oracle_buf(kind, N, T, {}, policy_state=f"{pstate}/{c}", **how) for c in COUNTERS}


def check_deterministic(means, low=-1.0, high=1.0):
    """C5: the share of deterministic actions (means) beyond each bound is >= 0.003 and at least 5 entries lie beyond each."""
    m = np.asarray(means)
    out = {}
    for side, beyond in (("+", m > high), ("-", m < low)):
        out[side] = (float(beyond.mean()), int(beyond.sum()))
        assert beyond.mean() >= DET_SHARE and beyond.sum() >= DET_COUNT, (side, out[side], m.size)
    return out


def check_density(op, op_uniform, obs, act, rtol, atol):
    """C6: on the case's given actions the oracle's log-prob under uniform_log_std differs from the case's by >= 50 bounds."""
    with torch.no_grad():
        lp = op.evaluate_actions(torch.as_tensor(obs), torch.as_tensor(act))[2].numpy()
        lp_u = op_uniform.evaluate_actions(torch.as_tensor(obs), torch.as_tensor(act))[2].numpy()
    shift = nc.in_bounds(lp_u, lp, rtol, atol)
    assert shift >= MIN_SHIFT, shift
    return shift


def f64_deviation(op, obs, act=None, noise=None, deterministic=False):
    """largest |float32 - float64| per output plane of the ORACLE's policy on a case's inputs (evaluate_actions when act is given, else
    forward): the reference's own rounding error, from which a bound is re-derived where sigma < 1 amplifies it (x 3)."""
    from oracle import nets as o_nets
    o64 = o_nets.TwoCriticPolicy.__new__(o_nets.TwoCriticPolicy)
    o64.__dict__.update(op.__dict__)
    o64.params = {k: v.detach().double() for k, v in op.params.items()}
    o64.latents = lambda obs_: _latents64(o64, obs_)
    t = lambda x: None if x is None else torch.as_tensor(np.asarray(x))
    with torch.no_grad():
        if act is not None:
            a32, a64 = op.evaluate_actions(t(obs), t(act)), o64.evaluate_actions(t(obs).double(), t(act).double())
            names = ("reward_values", "cost_values", "log_prob", "entropy")
        else:
            a32 = op.forward(t(obs), t(noise), deterministic)
            a64 = o64.forward(t(obs).double(), None if noise is None else t(noise).double(), deterministic)
            names = ("actions", "reward_values", "cost_values", "log_prob")
    return {k: (x32.double().reshape(-1) - x64.reshape(-1)).abs().max().item() for k, x32, x64 in zip(names, a32, a64)}, dict(zip(names, a64))


def _latents64(pol, obs):
    sh = pol._branch(obs.float().double(), "shared_net", len(pol.shared))
    return tuple(pol._branch(sh, b, len(pol.widths[b])) for b in pol.BRANCHES)


# ---- the cases of tests/test_policy_state_gpu.py (tests/test_policy_state_cpu.py runs the conditions of each from the oracle alone) ---------------
FWD_RTOL, FWD_ATOL = 1e-5, 2e-6          # test_policy_forward_vs_oracle / test_policy_rows_kernel_vs_oracle
ROLL_RTOL, ROLL_ATOL = 5e-4, 5e-5        # test_fused_rollout_vs_port
ROW_KINDS = [("hc", 64), ("hc", 1000), ("ant", 333), ("narrow", 200), ("wide", 40), ("wide", 300), ("trunk", 150), ("deep", 70), ("trunk-only", 33), ("bare", 20)]
# below 64 rows the 64-wide policies run policy_forward_kernel (one workgroup per row, policy_forward_block: test_policy_forward_vs_oracle's
# 33 rows; under `shaped` 33 rows hold only 2 means above +1, so 63 — the last size before policy_rows_kernel takes over — stands in)
ROW_CASES = ([(k, n, "shaped") for k, n in ROW_KINDS] + [("hc", 64, "ref"), ("hc", 1000, "ref")]
             + [("hc", 63, "shaped"), ("ant", 63, "shaped"), ("hc", 33, "ref"), ("hc", 63, "ref")])
_FUSED_SHAPES = [("auto", "hc", 7, 33), ("auto", "hc", 64, 40), ("auto", "ant", 32, 20), ("wide", "hc", 130, 24), ("wide", "antbroken", 512, 10),
                 ("multi", "hc", 37, 21), ("multi", "hc", 300, 12), ("multi", "ant", 128, 10), ("steps", "hc", 7, 33), ("steps", "ant", 32, 20),
                 ("wide-policy", "hc", 16, 40)]
FUSED = [(*c, "shaped") for c in _FUSED_SHAPES] + [(*c, "ref") for c in _FUSED_SHAPES if c[1] == "hc" and c[0] != "wide-policy"]
EVAL_AFTER = [(k, e, n, t, s) for k, e, n, t in (("auto", "hc", 64, 40), ("multi", "hc", 300, 12), ("auto", "ant", 32, 20)) for s in ("shaped", "ref")
              if s == "shaped" or e == "hc"]
# (kind, N, T, B, E, set, train_kernel, state): test_train_hparams_vs_oracle's list under `shaped` (sets A and B for the default kernels, A for
# the forced ones), `ref` at two HalfCheetah shapes.  Left out under `ref`, as their inputs miss check_trace at the default band seed:
# hc 8x32 B64 set A (ratio margin 4.4e-4) and hc 4x8 B16 (clip_fraction 0.94 > 0.9)
UPDATE_REF = [("hc", 8, 32, 64, 3, "B", None, "ref"), ("hc", 8, 32, 64, 3, "E", None, "ref"), ("hc", 5, 60, 200, 2, "A", None, "ref"), ("hc", 5, 60, 200, 2, "B", None, "ref")]
SAMPLERS = [(None, "ref"), ("trunk", "shaped")]
LGW_CASES = [(18, 5, 8, 32, 64, 3, 0.01), (40, 16, 8, 16, 128, 2, 0.05)]


def update_cases(hp_cases):
    """hp_cases: test_ppo_train_gpu._hp_cases() (passed in: that module needs a GPU to import nothing, but lives beside the GPU tests)."""
    out = []
    for kind, N, T, B, E, hset, kernel in hp_cases:
        if hset in ("A", "B") if kernel is None else hset == "A":
            out.append((kind, N, T, B, E, hset, kernel, "shaped"))
    return out + UPDATE_REF


def row_policy(kind, pstate):
    """test_policy_rows_kernel_vs_oracle's oracle policy of `kind` (torch seed 11) in a named state, its uniform_log_std counter, and
    (net_arch, obs_dim, act_dim, the fresh state dict).  kind: a name, or (obs_dim, act_dim) with the default architecture."""
    from helpers.arches import ARCHES, oracle_arch_kwargs
    from oracle import nets as o_nets
    od, ad = kind if isinstance(kind, tuple) else ((113, 8) if kind == "ant" else (18, 6))
    arch = dict(pi=[40, 24], vf=[64, 20], cvf=[16, 64]) if kind == "narrow" else None
    if kind == "wide":
        arch = dict(pi=[128, 100], vf=[72, 128], cvf=[200, 256])
    net_arch = ARCHES.get(kind, [arch] if arch else None)
    okw = oracle_arch_kwargs(net_arch) if net_arch else {}
    torch.manual_seed(11)
    op = o_nets.TwoCriticPolicy(od, ad, **okw)
    fresh = op.state_dict()
    op.load_state_dict(state(pstate, fresh, ad))
    ou = o_nets.TwoCriticPolicy(od, ad, **okw)
    ou.load_state_dict(state(pstate + "/uniform_log_std", fresh, ad))
    return op, ou, net_arch, od, ad, fresh


def row_inputs(n, od, ad):
    rng = np.random.RandomState(9)      # (test_policy_rows_kernel_vs_oracle's draws)
    return (rng.randn(n, od) * 2.0).astype(np.float32), rng.randn(n, ad).astype(np.float32), rng.randn(n, ad).astype(np.float32)


def check_rows(kind, n, pstate):
    """C1, C5 and C6 of a per-row case, from the oracle alone; returns (op, net_arch, od, ad, fresh, obs, act, noise)."""
    op, ou, net_arch, od, ad, fresh = row_policy(kind, pstate)
    obs, act, noise = row_inputs(n, od, ad)
    check_log_std(op.params["log_std"].detach())
    with torch.no_grad():
        means = op.forward(torch.as_tensor(obs), deterministic=True)[0].numpy()
    check_deterministic(means)
    check_density(op, ou, obs, act, FWD_RTOL, FWD_ATOL)
    return op, net_arch, od, ad, fresh, obs, act, noise


def lgw_shares(op, obs, no_favourite=0.5):
    """(share of rows whose largest class probability is >= 0.9, share where it is <= no_favourite) on the oracle's categorical policy."""
    with torch.no_grad():
        pmax = torch.softmax(op.heads(torch.as_tensor(obs))[0], -1).max(-1)[0].numpy()
    return float((pmax >= 0.9).mean()), float((pmax <= no_favourite).mean())


_SAMPLERS = {}
# the agent's seed (policy and train env) per architecture: one whose deterministic episodes hold C5 (trunk, seed 3: 0.0019 of the means below -1)
SAMPLER_SEEDS = {None: 3, "trunk": 9}


def sampler_case(shape, pstate, n_ep):
    """The oracle's side of a sampler case: one 4 x 32 rollout (its statistics are what the eval env is synced to), then n_ep episodes on
    HCWithPosTest with the policy in a named state: sampled (noise RandomState(0).randn(n_ep * 1000, 6)) and deterministic, through
    oracle.loop.sample_from_agent and evaluate_policy.  C1, and C5 on the deterministic episodes, are asserted here."""
    from helpers.arches import ARCHES, oracle_arch_kwargs
    from oracle import loop as o_loop
    if (shape, pstate, n_ep) in _SAMPLERS:
        return _SAMPLERS[shape, pstate, n_ep]
    net_arch = ARCHES[shape] if shape else None
    seed = SAMPLER_SEEDS[shape]
    o = nc.oracle_buf("hc", 4, 32, {}, net_arch=net_arch, seed=seed, noise_seed=5, cross_end=False, policy_state=pstate)
    check_log_std(o["policy_sd"]["log_std"])
    port = o_loop.PortAgent(o_loop.make_stack(4, "hc", seed), n_steps=32, seed=seed, **(oracle_arch_kwargs(net_arch) if net_arch else {}))
    port.policy.load_state_dict(o["policy_sd"])
    noise = np.random.RandomState(0).randn(n_ep * 1000, 6).astype(np.float32)

    def stack():
        est = o_loop.make_stack(1, "hc", 3, training=False, norm_reward=False, norm_cost=False, wall_terminate=True)
        o_loop.sync_normalization(o["norm"], est.norm)
        port.stack = est
        return est
    c = dict(o=o, noise=noise, net_arch=net_arch, seed=seed, want=o_loop.sample_from_agent(port, stack(), n_ep, noise),
             want_det=o_loop.sample_from_agent(port, stack(), n_ep, None, deterministic=True), port=port, stack=stack)
    # oracle.loop.evaluate_policy runs the same episodes as sample_from_agent on the same noise (tests/test_policy_state_cpu.py checks
    # that on the short case): its mean and std are those of the episode returns above
    c["eval"], c["eval_det"] = ((float(np.mean(c[k][3])), float(np.std(c[k][3]))) for k in ("want", "want_det"))
    with torch.no_grad():      # the means at the observations the deterministic episodes visit
        means = port.policy.forward(torch.as_tensor(c["want_det"][1]), deterministic=True)[0].numpy()
    c["det"] = check_deterministic(means)
    clipped = c["want_det"][2]
    assert (clipped == 1.0).sum() >= DET_COUNT and (clipped == -1.0).sum() >= DET_COUNT
    _SAMPLERS[shape, pstate, n_ep] = c
    return c


def update_policy(kind):
    """(the fresh state dict of an update case's agent (seed 0), the oracle's architecture keywords, obs_dim, act_dim).  kind: "hc" / "ant",
    with "-<architecture>" behind it, or (obs_dim, act_dim) with the default architecture."""
    from helpers.arches import ARCHES, oracle_arch_kwargs
    from oracle import nets as o_nets
    if isinstance(kind, tuple):
        (od, ad), shape = kind, ""
    else:
        kind, _, shape = kind.partition("-")
        od, ad = (18, 6) if kind == "hc" else (113, 8)
    net_arch = [dict(pi=[128, 96], vf=[80, 128], cvf=[128, 128])] if shape == "wide" else ARCHES.get(shape)
    okw = oracle_arch_kwargs(net_arch) if net_arch is not None else {}
    torch.manual_seed(0)
    return o_nets.TwoCriticPolicy(od, ad, **okw).state_dict(), okw, od, ad


def update_case(kind, N, T, B, E, hset, pstate):
    """the oracle's update case (helpers/ppo_hparam_cases.py) from a named state, as test_train_hparams_vs_oracle builds it on the GPU side
    (the fresh policy of agent seed 0; nu = softplus of the initial penalty = 1)."""
    from helpers import ppo_hparam_cases as H
    fresh, okw, od, ad = update_policy(kind)
    k, _, shape = (kind, "", "") if isinstance(kind, tuple) else kind.partition("-")
    sd0 = state(pstate, fresh, ad)
    return H.oracle_case(k, shape, N, T, B, E, hset, sd0, oracle_kwargs=okw, nu=1.0, state=pstate), sd0, okw, od, ad


def check_update_density(kind, N, T, B, E, hset, pstate):
    """C1 and C6 of an update case: on the buffer's actions a uniform sigma gives other log-probs (by >= 50 forward bounds)."""
    from oracle import nets as o_nets
    case, sd0, okw, od, ad = update_case(kind, N, T, B, E, hset, pstate)
    check_log_std(sd0["log_std"])
    fresh = update_policy(kind)[0]
    op, ou = o_nets.TwoCriticPolicy(od, ad, **okw), o_nets.TwoCriticPolicy(od, ad, **okw)
    op.load_state_dict(sd0); ou.load_state_dict(state(pstate + "/uniform_log_std", fresh, ad))
    check_density(op, ou, case["buf"]["observations"].reshape(-1, od), case["buf"]["actions"].reshape(-1, ad), FWD_RTOL, FWD_ATOL)
    return case


_LGW = []


def lgw_sampler_case():
    """The oracle's side of the categorical samplers with a peaked head: a Discrete(2) policy (agent seed LGW_SAMPLER_SEED, action_net.weight x
    LGW_SAMPLER_K), 3 episodes of sample_from_agent on LGW-v0 and 10 evaluation episodes on CLGW-v0 (they end at the first backward move) on
    given uniforms.  Asserted here, from the oracle alone: both shares of LGW_SHARE over the rows visited, no uniform within LGW_DRAW_MARGIN of
    a class boundary (so a kernel's float32 softmax must draw the same actions), and evaluation episodes that end early, at three or more different steps."""
    from oracle import loop as o_loop
    if _LGW:
        return _LGW[0]
    mk = lambda kind, n, **kw: o_loop.make_stack(n, kind, 0, norm_obs=False, norm_reward=False, norm_cost=False, **kw)
    port = o_loop.PortAgent(mk("lgw", 2), n_steps=32, seed=LGW_SAMPLER_SEED, discrete=True)
    fresh = port.policy.state_dict()
    sd = dict(fresh)
    sd["action_net.weight"] = fresh["action_net.weight"] * LGW_SAMPLER_K
    port.policy.load_state_dict(sd)
    rng = np.random.RandomState(4)
    u, u2 = rng.rand(3 * 200).astype(np.float32), rng.rand(10 * 200).astype(np.float32)
    margins = []

    def predict(obs, noise=None, deterministic=False, _p=port.predict):      # (records how far each draw is from the class boundary)
        with torch.no_grad():
            p0 = torch.softmax(port.policy.heads(torch.as_tensor(np.asarray(obs)).reshape(-1, 1))[0], -1)[:, 0].numpy()
        margins.append(float(np.abs(np.asarray(noise, np.float32) - p0).min()))
        return _p(obs, noise, deterministic)
    port.predict = predict
    s1 = mk("lgw", 1, training=False)
    port.stack = s1
    want = o_loop.sample_from_agent(port, s1, 3, u)
    hi, lo = lgw_shares(port.policy, want[1].reshape(-1, 1).astype(np.float32), LGW_NO_FAVOURITE)
    assert hi >= LGW_SHARE and lo >= LGW_SHARE, (hi, lo)
    assert list(want[4]) == [200, 200, 200] and 0.2 < float(want[2].mean()) < 0.8
    e1 = mk("clgw", 1, training=False)
    port.stack = e1
    k, obs, lens, rews = 0, e1.reset(), [], []      # episode by episode, as test_sampling_and_evaluation_vs_port walks the port
    for ep in range(10):
        done, n, tot = False, 0, 0.0
        while not done:
            act = port.predict(obs, u2[k:k + 1]); k += 1
            obs, r, d, _ = e1.step(act)
            done = bool(d[0]); n += 1; tot += float(r[0])
        lens.append(n); rews.append(tot)
    assert min(margins) >= LGW_DRAW_MARGIN, min(margins)
    assert min(lens) < 200 and len(set(lens)) >= 3, lens
    _LGW.append(dict(sd=sd, fresh=fresh, u=u, u2=u2, want=want, lens=lens, rews=rews, shares=(hi, lo), margin=min(margins)))
    return _LGW[0]
