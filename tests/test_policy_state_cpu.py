"""CPU: the conditions C1..C6 of tests/helpers/policy_states.py for every (state, shape) pair tests/test_policy_state_gpu.py uses, from the
oracle alone — a later change of a seed, a shape or a state fails here and not on a GPU."""
import io
import zipfile

import numpy as np
import pytest
import torch

from helpers import norm_cases as nc, policy_states as ps, ppo_hparam_cases as H
from oracle import nets as o_nets


def test_states_are_what_they_claim():
    """C1 for both states; `ref`'s log_std is what the archive holds; `shaped` touches log_std and the action head only."""
    with zipfile.ZipFile(ps.REF_ZIP) as z:
        sd = torch.load(io.BytesIO(z.read("policy.pth")), map_location="cpu", weights_only=True)
    ref = ps.ref()
    assert list(ref) == list(sd) and all(torch.equal(ref[k], sd[k].float()) for k in sd) and len(sd) == 19
    assert np.allclose(ref["log_std"].numpy(), ps.LOG_STD[6], rtol=0, atol=5e-5)
    ps.check_log_std(ref["log_std"])
    assert 0.1 < float(ref["action_net.weight"].std()) < 0.2 and 0.2 < float(ref["action_net.bias"].abs().max()) < 0.3
    for od, ad in ((18, 6), (113, 8)):
        torch.manual_seed(0)
        fresh = o_nets.TwoCriticPolicy(od, ad).state_dict()
        sh = ps.state("shaped", fresh, ad)
        ps.check_log_std(sh["log_std"])
        changed = {k for k in fresh if not torch.equal(fresh[k], sh[k])}
        assert changed == {"log_std", "action_net.weight", "action_net.bias"}
        assert torch.equal(sh["action_net.weight"], fresh["action_net.weight"] * 50) and float(sh["action_net.bias"].abs().max()) <= 0.9
        assert float(ps.state("shaped/zero_log_std", fresh, ad)["log_std"].abs().max()) == 0.0
        u = ps.state("shaped/uniform_log_std", fresh, ad)["log_std"]
        assert float(u.max()) == float(u.min()) and abs(float(u[0]) - float(sh["log_std"].mean())) < 1e-6
        assert torch.equal(ps.state("shaped/fresh_head", fresh, ad)["action_net.weight"], fresh["action_net.weight"])
        assert all(torch.equal(v, fresh[k]) for k, v in ps.state(None, fresh, ad).items())
    with pytest.raises(AssertionError):
        ps.state("ref", fresh, 8)          # `ref` serves HalfCheetah shapes only


@pytest.mark.parametrize("kind,n,pstate", ps.ROW_CASES, ids=[f"{k}-{n}-{s}" for k, n, s in ps.ROW_CASES])
def test_per_row_cases(kind, n, pstate):
    """C1, C5, C6 of section a; and the oracle's own float32 rounding (against float64) stays within a third of the forward bound, so that
    the bound needs no re-derivation at these states."""
    op, net_arch, od, ad, fresh, obs, act, noise = ps.check_rows(kind, n, pstate)
    t = torch.as_tensor
    for tag, kw in (("eval", dict(act=act)), ("forward", dict(noise=noise)), ("deterministic", dict(deterministic=True))):
        _, x64 = ps.f64_deviation(op, obs, **kw)
        with torch.no_grad():
            x32 = op.evaluate_actions(t(obs), t(act)) if tag == "eval" else op.forward(t(obs), None if tag == "deterministic" else t(noise), tag == "deterministic")
        for (k, r), g in zip(x64.items(), x32):
            assert 3 * nc.in_bounds(g.numpy().reshape(-1), r.numpy().reshape(-1), ps.FWD_RTOL, ps.FWD_ATOL) <= 1.0, (tag, k)


def _fused_shapes():
    import test_policy_state_gpu as tg      # (importable without a GPU: its kernels load inside the tests)
    cases = {(kind, N, T, s, kernel == "wide-policy", 7, 2, None, True) for kernel, kind, N, T, s in ps.FUSED + ps.EVAL_AFTER}
    for kind, N, T in (("hc", 7, 33), ("hc", 130, 24), ("hc", 300, 12), ("ant", 32, 20)):
        cases.add((kind, N, T, "shaped", False, 13, 8, 2, True))
    cases |= {("hc", 7, 24, "shaped", False, 5, 8, 2, True), ("ant", 16, 12, "shaped", False, 5, 8, 2, True)}
    cases |= {("hc", N, T, s, False, 7, 8, None, True) for N, T in ((8, 32), (96, 16)) for s in tg._BATCH_STATES[1:]}
    return sorted(cases, key=repr)


@pytest.mark.parametrize("kind,N,T,pstate,wide,seed,noise_seed,rollouts,cross_end", _fused_shapes())
def test_rollout_cases(kind, N, T, pstate, wide, seed, noise_seed, rollouts, cross_end):
    """C1..C4 of sections b, c, d and f (every distinct oracle rollout they ask for)."""
    o, counters = ps.rollout_case(kind, N, T, pstate, net_arch=nc.WIDE_ARCH if wide else None, seed=seed, noise_seed=noise_seed, rollouts=rollouts,
                                  cross_end=cross_end)
    assert o["buf"].dones.sum() == N
    ps.check_rollout(o, counters, ps.ROLL_RTOL, ps.ROLL_ATOL)


def test_generic_shape_twin_and_batched_planes():
    from helpers.arches import ARCHES
    o, counters = ps.rollout_case("hc", 12, 40, "shaped", net_arch=ARCHES["trunk"], seed=11, noise_seed=3, rollouts=2, cross_end=False)
    ps.check_rollout(o, counters, ps.ROLL_RTOL, ps.ROLL_ATOL)
    for N, T in ((8, 32), (96, 16)):      # section f: the three runs' action planes differ pairwise
        bufs = [nc.oracle_buf("hc", N, T, {}, noise_seed=8, policy_state=s)["buf"] for s in (None, "shaped", "ref")]
        for i in range(3):
            for j in range(i):
                assert nc.in_bounds(bufs[i].actions, bufs[j].actions, ps.ROLL_RTOL, ps.ROLL_ATOL) >= ps.MIN_SHIFT, (N, i, j)


@pytest.mark.parametrize("shape,pstate", ps.SAMPLERS, ids=["64-wide-ref", "trunk-shaped"])
def test_sampler_cases(shape, pstate):
    """section e: C5 on the oracle's deterministic episodes; sampled and deterministic evaluations differ."""
    c = ps.sampler_case(shape, pstate, 3)
    assert c["want"][0].shape[0] == sum(c["want"][4]) and c["want_det"][0].shape[0] == sum(c["want_det"][4])
    assert abs(c["eval"][0] - c["eval_det"][0]) > 1.0
    if shape is None:      # (short episodes) the oracle's evaluate_policy gives the mean and std of sample_from_agent's episode returns
        from oracle import loop as o_loop
        assert o_loop.evaluate_policy(c["port"], c["stack"](), 3, c["noise"]) == c["eval"]
        assert o_loop.evaluate_policy(c["port"], c["stack"](), 3, None, deterministic=True) == c["eval_det"]


def _update_cases():
    import test_ppo_train_gpu as tp
    return ps.update_cases(tp._hp_cases())


@pytest.mark.parametrize("kind,N,T,B,E,hset,train_kernel,pstate", _update_cases())
def test_update_cases(kind, N, T, B, E, hset, train_kernel, pstate):
    """section g: check_trace as it stands, C1 and C6; the norm clip keeps one branch."""
    case = ps.check_update_density(kind, N, T, B, E, hset, pstate)
    H.check_trace(case["trace"], case["hp"], n_steps=E * (-(-N * T // B)))


def test_batched_update_cases():
    for s in ("shaped", "ref"):
        ps.check_update_density("hc", 8, 32, 64, 2, "A", s)
    for s in (None, "shaped", "ref"):
        case = ps.update_case("hc", 8, 32, 64, 2, "A", s)[0]
        H.check_trace(case["trace"], case["hp"], n_steps=8)


@pytest.mark.parametrize("O,A,N,T,B,E,ent", ps.LGW_CASES)
def test_categorical_head_scale(O, A, N, T, B, E, ent):
    """section h: with action_net.weight x LGW_K the largest class probability is >= 0.9 in >= 10 % of the rows and <= 0.5 in >= 10 %."""
    torch.manual_seed(0)
    op = o_nets.TwoCriticPolicy(O, A, discrete=True)
    obs = np.random.RandomState(O * A + T).randn(T, N, O).astype(np.float32).reshape(-1, O)      # (_categorical_case's draw)
    assert max(ps.lgw_shares(op, obs)[0], 0.0) == 0.0      # the fresh head: no row has a favourite
    op.params["action_net.weight"].data.mul_(ps.LGW_K)
    hi, lo = ps.lgw_shares(op, obs)
    assert hi >= ps.LGW_SHARE and lo >= ps.LGW_SHARE, (hi, lo)


def test_categorical_sampler_case():
    """section h, samplers: LGW has two classes, so "no favourite" is pmax <= 0.6; both shares, the draws' distance from the class boundaries
    and the early ends of the CLGW episodes are asserted inside the case; at the fresh head no row has a favourite."""
    c = ps.lgw_sampler_case()
    assert c["shares"][0] >= ps.LGW_SHARE and c["shares"][1] >= ps.LGW_SHARE and c["margin"] >= ps.LGW_DRAW_MARGIN
    op = o_nets.TwoCriticPolicy(1, 2, discrete=True)
    op.load_state_dict(c["fresh"])
    assert ps.lgw_shares(op, c["want"][1].reshape(-1, 1).astype(np.float32), ps.LGW_NO_FAVOURITE) == (0.0, 1.0)
