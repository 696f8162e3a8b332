"""Inputs that make the update kernels take every branch of the PPO-Lagrangian loss (ref: ppo_lag.py:226-288) without sitting on one of
its kinks: hyper-parameter sets, a rollout buffer built in bands, and the conditions every test asserts FROM THE ORACLE'S TRACE before it
looks at a kernel.

clamp() and min() have kinks.  A row whose ratio or value difference lies within float rounding of one can fall on different sides in the
kernel and in torch, which moves parameters by O(lr) for reasons that have nothing to do with correctness.  So old log-probs and old values
are placed in bands around the current policy's outputs:

  ratio bands   r0 = 0.5 + 0.15 u | 0.93 + 0.14 u | 1.4 + 0.3 u (band drawn uniformly from the three, u ~ U[0, 1)); log_probs = lp - log r0:
                a third of the rows starts below 1 - clip, a third inside, a third above 1 + clip (clip 0.2)
  value bands   old_value = v + s c k with s = +-1 at random and k = 0.4 u for one half of the rows ("inside" the clip c), 1.8 + 1.2 u for
                the other ("outside"), per critic with its own clip
"""
import numpy as np
import torch

from oracle import nets as o_nets, ppo as o_ppo

SET_A = dict(clip_range_reward_vf=0.2, clip_range_cost_vf=0.3, ent_coef=0.01, reward_vf_coef=0.7, cost_vf_coef=0.3, max_grad_norm=0.3)
HP_SETS = {
    "A": SET_A,                                    # everything on, the norm clip active at every step
    "B": dict(SET_A, max_grad_norm=50.0),          # ... the norm clip's coefficient capped at 1 at every step
    "C": dict(clip_range_reward_vf=0.2),           # one thing at a time (to name the term when A fails); C and D between them catch
    "D": dict(clip_range_cost_vf=0.3),             # the two critics' clips being swapped
    "E": {},                                       # defaults on the banded buffer: the ratio clip at clip_fraction ~ 0.6
}
DEFAULTS = dict(clip_range_reward_vf=None, clip_range_cost_vf=None, ent_coef=0.0, reward_vf_coef=0.5, cost_vf_coef=0.5, max_grad_norm=0.5)
# the conditions on the inputs (50 x the forward tolerances of the project: atol 2e-5 on log-probs, 2e-6 on values)
RATIO_MARGIN, VALUE_MARGIN = 1e-3, 1e-4
CLIP_FRACTION, VCLIP_SHARE = (0.3, 0.9), (0.2, 0.8)


def hparams(hset):
    return dict(DEFAULTS, **HP_SETS[hset])


def banded(rng, lp, v_r, v_c, clip_r, clip_c):
    """(log_probs, reward_values, cost_values) of the buffer, in the shape of lp / v_r / v_c (float32 arrays of the current policy's
    outputs).  A critic without a clip gets the bands of set A's (its old values are not read by the loss)."""
    lp, v_r, v_c = (np.asarray(x, np.float32) for x in (lp, v_r, v_c))
    n = lp.size
    band, u = rng.randint(3, size=n), rng.rand(n)
    r0 = np.choose(band, [0.5 + 0.15 * u, 0.93 + 0.14 * u, 1.4 + 0.3 * u])
    out = [(lp.ravel() - np.log(r0)).astype(np.float32).reshape(lp.shape)]
    for v, c, c_dflt in ((v_r, clip_r, SET_A["clip_range_reward_vf"]), (v_c, clip_c, SET_A["clip_range_cost_vf"])):
        c = c_dflt if c is None else c
        s, u = rng.choice([-1.0, 1.0], size=n), rng.rand(n)
        outside = np.zeros(n, bool)
        outside[rng.permutation(n)[:n // 2]] = True
        k = np.where(outside, 1.8 + 1.2 * u, 0.4 * u)
        out.append((v.ravel() + s * c * k).astype(np.float32).reshape(v.shape))
    return tuple(out)


def check_trace(trace, hp, n_steps=None):
    """The conditions on the inputs, from the oracle's trace (oracle.ppo.ppo_lag_train(trace=...)); every optimiser step, no row left out."""
    assert len(trace) > 0 and (n_steps is None or len(trace) == n_steps), (len(trace), n_steps)
    active = [t["grad_norm"] > hp["max_grad_norm"] for t in trace]
    for i, t in enumerate(trace):
        assert t["ratio_margin"] >= RATIO_MARGIN, (i, t)
        assert CLIP_FRACTION[0] <= t["clip_fraction"] <= CLIP_FRACTION[1], (i, t)
        for tag, c in (("r", hp["clip_range_reward_vf"]), ("c", hp["clip_range_cost_vf"])):
            if c is not None:
                assert t["v_margin_" + tag] >= VALUE_MARGIN, (i, tag, t)
                assert VCLIP_SHARE[0] <= t["vclip_share_" + tag] <= VCLIP_SHARE[1], (i, tag, t)
        assert t["grad_norm"] != hp["max_grad_norm"]
    # the norm clip takes ONE branch through the whole case: sets with max_grad_norm 50 never scale the gradient, all others always do
    assert all(active) if hp["max_grad_norm"] < 10 else not any(active), [t["grad_norm"] for t in trace]


def _np(v):
    return v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)


_CASES = {}
# the stream of the bands is seeded per shape (the same buffer under every hyper-parameter set); a shape whose default seed misses one
# of the conditions above under one of its sets gets another seed here — never another condition
BAND_SEEDS = {("hc", "wide", 8, 32, 64, 3): 4}      # (the default seed: ratio margin 4e-4 at step 10 of set B)
# ... and per (shape, policy state of helpers/policy_states.py, set), found on the CPU (tests/test_policy_state_cpu.py runs check_trace on each)
STATE_BAND_SEEDS = {("hc", "", 8, 32, 64, 3, "shaped", "B"): 2, ("hc", "", 8, 32, 64, 3, "shaped", "E"): 5, ("hc", "wide", 8, 32, 64, 3, "shaped", "B"): 3,
                    ("hc", "", 8, 128, 512, 3, "shaped", "A"): 1, ("hc", "", 8, 128, 512, 3, "shaped", "B"): 4,
                    ("hc", "", 8, 32, 64, 2, "ref", "A"): 1}      # (the default seeds: a ratio margin below 1e-3 at one step)
# ... and the widths of helpers/width_cases.py, keyed by (obs_dim, act_dim) in place of the name (tests/test_width_cases_cpu.py runs check_trace on each;
# every one of them holds check_trace at its default seed).  97 x 3 at 4x30 B40: the seed under which the padded-norm counter-oracle of
# width_cases.padded_norm_update moves a parameter by more than 10 bounds (12.3; the default seed: 5.1 — see PADDED_NORM there)
STATE_BAND_SEEDS[((97, 3), "", 4, 30, 40, 2, "shaped", "A")] = 6


def shape_of(kind):
    """(obs_dim, act_dim, learning rate) of a case: "hc" / "ant", or (obs_dim, act_dim) — 3e-4 up to four 16-column observation tiles, 3e-5 above, as for hc / ant."""
    od, ad = kind if isinstance(kind, tuple) else {"hc": (18, 6), "ant": (113, 8)}[kind]
    return od, ad, (3e-4 if od <= 64 else 3e-5)


def oracle_case(kind, shape, N, T, B, E, hset, sd0, oracle_kwargs=None, nu=None, state=None):
    """The banded buffer of one case, the permutations, and the oracle's float32 update on them — computed once per case and shared by
    every kernel family that runs it (nothing of it is modified afterwards).  state: the name of the policy state sd0 is in (part of the cache
    key and of the band seed's).  sd0: the agent's initial state dict (the same for every agent
    of a case: seed 0); returns a dict with buf, perms, hp, lr, out (the train/* scalars), params and both Adam moments (after the update), trace.
    kind: "hc" / "ant", or (obs_dim, act_dim): its draws come from seeds that include the width."""
    key = (kind, shape, N, T, B, E, hset, state)
    hit = _CASES.get(key)
    if hit is not None and hit["nu"] == nu and all(np.array_equal(hit["sd0"][k], _np(v)) for k, v in sd0.items()):
        return hit
    hp = hparams(hset)
    od, ad, lr = shape_of(kind)
    width = 1009 * od + 100003 * ad if isinstance(kind, tuple) else 0
    rng = np.random.RandomState(N * T + width)          # observations, advantages, returns, permutations: as test_train_vs_oracle draws them
    seed = BAND_SEEDS.get((kind, shape, N, T, B, E), 7919 + N * T + B + width)
    brng = np.random.RandomState(seed if state is None else STATE_BAND_SEEDS.get((kind, shape, N, T, B, E, state, hset), seed))      # the bands
    op = o_nets.TwoCriticPolicy(od, ad, **(oracle_kwargs or {}))
    op.load_state_dict(sd0)
    obs = rng.randn(T, N, od).astype(np.float32)
    with torch.no_grad():
        noise = brng.randn(T * N, ad)      # (the case's own stream, not torch's global one)
        a, vr, vc, lp = op.forward(torch.as_tensor(obs.reshape(-1, od)), noise=torch.as_tensor(noise.astype(np.float32)))
    old_lp, old_vr, old_vc = banded(brng, lp.numpy().reshape(T, N), vr.numpy().reshape(T, N), vc.numpy().reshape(T, N),
                                    hp["clip_range_reward_vf"], hp["clip_range_cost_vf"])
    acts = a.numpy().reshape(T, N, -1).astype(np.float32)
    buf = dict(observations=obs, actions=acts, log_probs=old_lp, reward_values=old_vr, cost_values=old_vc,
               reward_advantages=rng.randn(T, N).astype(np.float32) * 2, cost_advantages=rng.rand(T, N).astype(np.float32),
               reward_returns=rng.randn(T, N).astype(np.float32), cost_returns=rng.rand(T, N).astype(np.float32),
               orig_costs=rng.rand(T, N).astype(np.float32))
    perms = np.stack([rng.permutation(T * N) for _ in range(E)])
    opt = torch.optim.Adam(op.parameters(), lr=lr, eps=1e-5)
    trace = []
    out = o_ppo.ppo_lag_train(op, opt, buf, perms, nu, batch_size=B, n_epochs=E, clip_range=0.2, target_kl=None, trace=trace, **hp)
    case = dict(sd0={k: _np(v).copy() for k, v in sd0.items()}, buf=buf, perms=perms, hp=hp, lr=lr, nu=nu, out=out, trace=trace,
                params={k: p.detach().numpy().copy() for k, p in op.params.items()},
                exp_avg={k: opt.state[p]["exp_avg"].numpy().copy() for k, p in op.params.items()},
                exp_avg_sq={k: opt.state[p]["exp_avg_sq"].numpy().copy() for k, p in op.params.items()})
    _CASES[key] = case
    return case
