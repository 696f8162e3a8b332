"""Normaliser settings at which the clips, epsilon and the two gammas of VecNormalizeWithCost (ref: vec_normalize.py:81-123,184-278) are
visible in a rollout, and the conditions every test asserts FROM THE ORACLE'S BUFFERS before it looks at a kernel.

At the defaults (clips 10, epsilon 1e-8, both gammas 0.99) no normalised value of the suite's rollouts comes near a clip, the two gammas
are interchangeable and epsilon is below fp32 resolution: a kernel that drops a clip, clips one side only, swaps the two clips or the two
gammas or forgets epsilon passes.  The keyword sets below go to the product's VecNormalizeWithCost and to oracle.loop.make_stack alike.

The cost of the fused rollouts is a sigmoid output (>= 0): their LOWER cost clip cannot be reached; it is tested at the per-step entry
point only (signed raw costs through env._norm_call, tests/test_normalizer_settings_gpu.py::test_per_step_entry_points).
"""
import numpy as np

DEFAULTS = dict(clip_obs=10.0, clip_reward=10.0, clip_cost=10.0, reward_gamma=0.99, cost_gamma=0.99, epsilon=1e-8)
TIGHT = dict(clip_obs=1.5, clip_reward=0.5, clip_cost=0.7, reward_gamma=0.9, cost_gamma=0.97)
CASES = {
    "tight": TIGHT,
    "eps": dict(epsilon=0.25),                                        # the clips stay at 10: never reached
    "tight_no_rew": dict(TIGHT, norm_reward=False),                    # rewards come out raw, observations and costs clipped
    "tight_no_obs": dict(TIGHT, norm_obs=False, norm_cost=False),      # only the reward is normalised and clipped
}
SHARE = (0.05, 0.70)       # share of a clipped plane's entries that sit AT a bound, per covered side
MIN_SHIFT = 50.0           # the counter-run (gammas swapped / default epsilon) moves the planes by at least this many bounds
# the reward sides a shape reaches under `tight`: HalfCheetah rewards never reach the lower clip, Ant rewards hardly the upper one
REWARD_SIDES = {"hc": "+", "ant": "-", "antbroken": "+-"}


def settings(case):
    """the full keyword set of a case (defaults filled in)."""
    return {**DEFAULTS, "norm_obs": True, "norm_reward": True, "norm_cost": True, **CASES[case]}


def share_at(x, bound):
    """share of x's entries equal to the bound, rounded to x's type (the buffers are float32: 0.7 is not a float32)."""
    x = np.asarray(x)
    return float(np.mean(x == np.asarray(bound, x.dtype)))


def assert_share(name, x, clip, sides="+-", count_only=False):
    """x holds nothing beyond +-clip, and SHARE of its entries sit at each bound of `sides` (count_only: at least one entry)."""
    x = np.asarray(x)
    assert np.abs(x).max() <= np.asarray(clip, x.dtype), (name, np.abs(x).max(), clip)
    for side in sides:
        s = share_at(x, clip if side == "+" else -clip)
        if count_only:
            assert s > 0.0, (name, side, s)
        else:
            assert SHARE[0] <= s <= SHARE[1], (name, side, s)


def in_bounds(got, ref, rtol, atol):
    """largest |got - ref| in units of the comparison bound atol + rtol |ref| (<= 1: np.allclose holds)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref) / (atol + rtol * np.abs(ref)))) if got.size else 0.0


def counter_settings(case):
    """the run a case must tell itself apart from: `eps` against the default epsilon, the tight cases against swapped gammas."""
    kw = dict(CASES[case])
    if "epsilon" in kw:
        kw["epsilon"] = DEFAULTS["epsilon"]
    else:
        kw["reward_gamma"], kw["cost_gamma"] = kw["cost_gamma"], kw["reward_gamma"]
    return kw


def check_rollout_inputs(case, kind, buf, counter, N, rtol, atol, cross_end=True):
    """The input conditions of a fused-rollout case.  buf: the oracle's rollout under settings(case); counter: the oracle's rollout under
    counter_settings(case), same weights and noise; nothing here comes from the code under test."""
    kw = settings(case)
    assert buf.dones.sum() == (N if cross_end else 0)      # every env crossed an episode end: ret / cost_ret were zeroed mid-rollout
    tight = kw["clip_obs"] < DEFAULTS["clip_obs"]
    if tight and kw["norm_obs"]:
        assert_share("new_observations", buf.new_observations, kw["clip_obs"])
    if tight and kw["norm_reward"]:
        assert_share("rewards", buf.rewards, kw["clip_reward"], REWARD_SIDES[kind])
    if tight and kw["norm_cost"]:
        assert_share("costs", buf.costs, kw["clip_cost"], "+")      # (sigmoid cost: the lower clip is unreachable here, see the module text)
        assert buf.costs.min() >= 0.0
    if tight and not kw["norm_reward"]:
        assert np.abs(buf.rewards).max() > 3.0        # raw rewards, far beyond clip_reward = 0.5
    if tight and not kw["norm_obs"]:
        assert np.abs(buf.new_observations).max() > kw["clip_obs"] and np.array_equal(buf.new_observations, buf.new_orig_observations)
    if tight and not kw["norm_cost"]:
        assert np.array_equal(buf.costs, buf.orig_costs)
    planes = [k for k, on in (("rewards", kw["norm_reward"]), ("costs", kw["norm_cost"])) if on]
    if "epsilon" in CASES[case]:
        planes.append("new_observations")
    for k in planes:
        shift = in_bounds(getattr(counter, k), getattr(buf, k), rtol, atol)
        assert shift >= MIN_SHIFT, (case, k, shift)


_ROLLOUTS = {}
WIDE_ARCH = [dict(pi=[128, 96], vf=[80, 128], cvf=[128, 128])]      # -pl 128 96 -rvl 80 128 -cvl 128 128 (icrl/utils.py:636-655)


def oracle_buf(kind, N, T, kw, net_arch=None, seed=7, noise_seed=2, rollouts=None, cross_end=True, policy_state=None):
    """One rollout of the oracle port (oracle.loop.PortAgent.collect_rollouts) under the normaliser keywords kw, computed once per
    argument set and shared by every test that asks for it (nothing of it is modified afterwards): policy and constraint net freshly
    initialised under torch seed `seed` (the constraint net first, as the tests' GPU chains draw them), teacher-forced noise
    RandomState(noise_seed).randn([rollouts,] T, N, act)[0]; cross_end: every env starts at limit - T // 2, so that it crosses its time
    limit inside the rollout; policy_state: a name of helpers/policy_states.py, applied to the fresh policy before the rollout (it lands
    in policy_sd).  Returns a dict: buf, norm (the normaliser state after the rollout), policy_sd, cn_sd, noise, start."""
    import torch
    from helpers.arches import oracle_arch_kwargs
    from oracle import loop as o_loop, nets as o_nets
    key = (kind, N, T, tuple(sorted(kw.items())), repr(net_arch), seed, noise_seed, rollouts, cross_end, policy_state)
    if key in _ROLLOUTS:
        return _ROLLOUTS[key]
    broken = kind == "antbroken"
    ekind = "ant" if broken else kind
    od, ad = (18, 6) if ekind == "hc" else (113, 8)
    hid = [20] if ekind == "hc" else [40, 40]
    lo = -np.ones(ad, np.float32)
    start = ((1000 if ekind == "hc" else 500) - T // 2) if cross_end else 0
    rng = np.random.RandomState(noise_seed)
    noise = rng.randn(T, N, ad).astype(np.float32) if rollouts is None else rng.randn(rollouts, T, N, ad).astype(np.float32)[0]
    torch.manual_seed(seed)
    ocn = o_nets.CostNet(od, ad, hid, False, None, None, 20, lo, -lo)
    stack = o_loop.make_stack(N, ekind, seed, broken=broken, **kw)
    stack.cost_fn = ocn.cost_function
    port = o_loop.PortAgent(stack, n_steps=T, seed=seed, **(oracle_arch_kwargs(net_arch) if net_arch else {}))
    if policy_state is not None:
        from helpers import policy_states
        port.policy.load_state_dict(policy_states.state(policy_state, port.policy.state_dict(), ad))
    out = dict(cn_sd=ocn.state_dict(), policy_sd=port.policy.state_dict(), noise=noise, start=start, port=port)
    port.num_timesteps = 0
    port._last_obs = stack.reset(); port._last_dones = np.zeros(N, bool); port._last_original_obs = stack.old_obs.copy()
    stack.env.t_ep[:] = start
    out["buf"], out["norm"] = port.collect_rollouts(noise), stack.norm
    _ROLLOUTS[key] = out
    return out


def oracle_rollout(kind, N, T, case, **how):
    """The oracle's side of a case: oracle_buf under settings(case), plus `counter`, the same rollout (same weights: same seed, same
    noise) under counter_settings(case)."""
    out = dict(oracle_buf(kind, N, T, CASES[case], **how))
    out["counter"] = oracle_buf(kind, N, T, counter_settings(case), **how)["buf"]
    return out
