"""CPU: the conditions on the inputs of every case of tests/helpers/width_cases.py (the observation and action widths between HalfCheetah's and
AntWall's), from the oracle alone — tests/test_update_widths_gpu.py and tests/test_forward_widths_gpu.py import the same lists, so no kernel
runs inputs this file has not accepted.  And the proof that those inputs can see the fault the sweep is aimed at: the oracle with its gradient
norm taken over the padded W1 lands more than ten update bounds from the true oracle."""
import numpy as np
import pytest
import torch

from helpers import norm_cases as nc, policy_states as ps, ppo_hparam_cases as H, width_cases as W


def test_the_matrix_is_what_it_claims():
    """17 widths over the three bands, every width through the default kernel at both layouts, the expected kinds those of prepare_train."""
    assert len(W.ALL_WIDTHS) == len(set(W.ALL_WIDTHS)) == 17
    assert all(W.band(o) == b for b, ws in W.WIDTHS.items() for o, a in ws)
    assert {o for o, a in W.ALL_WIDTHS} >= {1, 16, 17, 32, 33, 48, 49, 64, 65, 128} and {a for o, a in W.ALL_WIDTHS} >= {1, 16}
    default = [c for c in W.UPDATE_CASES if c[4] is None and c[3] == "A"]
    assert sorted((c[0], c[1], c[2]) for c in default) == sorted((o, a, lay) for o, a in W.ALL_WIDTHS for lay in ("L1", "L2"))
    for o, a, lay, hset, kernel, kind in W.UPDATE_CASES:
        B = W.LAYOUTS[lay][2]
        two_chunks, b = 64 < B <= 128, W.band(o)
        want = {None: {"narrow": 5, "middle": 0, "wide": 7 if two_chunks else 6}[b], "halves": 4, "pairs": 0, "tiles": 3, "rows": 2 if two_chunks else 1, "rows1": 1}[kernel]
        assert kind == want, (o, a, lay, kernel, kind, want)
    assert len(W.UPDATE_CASES) == len(set(W.UPDATE_CASES)) == 63
    assert all(H.shape_of((o, a))[2] == (3e-5 if W.band(o) == "wide" else 3e-4) for o, a in W.ALL_WIDTHS)


@pytest.mark.parametrize("act", range(1, 17))
def test_log_std_of_every_action_width(act):
    """`shaped` at any action width: C1; both signs from 2 actions on (6 actions keep the reference's trained row, all below 0); the rows for 6
    and 8 actions are the ones the earlier cases ran."""
    ls = np.asarray(ps.log_std_of(act))
    assert ls.shape == (act,)
    ps.check_log_std(ls)
    if act not in ps.LOG_STD:
        assert ls == pytest.approx(ps.log_std_rule(act)) and (act == 1 or ls.min() < 0 < ls.max())
    assert ps.LOG_STD[6] == [-0.6385, -0.9999, -0.6585, -1.0631, -1.0151, -0.8097] and ps.LOG_STD[8] == [-1.2, 0.35, -0.7, -0.2, -1.0, 0.1, -0.45, -0.9]
    torch.manual_seed(0)
    from oracle import nets as o_nets
    fresh = o_nets.TwoCriticPolicy(17, act).state_dict()
    sh = ps.state("shaped", fresh, act)
    assert np.array_equal(sh["log_std"].numpy(), ls.astype(np.float32)) and {k for k in fresh if not torch.equal(fresh[k], sh[k])} == {"log_std", "action_net.weight", "action_net.bias"}


def test_named_cases_keep_their_inputs():
    """oracle_case by name draws what it drew before it took (obs, act): the generators' seeds of the hc / ant cases, and a width case's differ."""
    fresh, okw, od, ad = ps.update_policy("hc")
    case = H.oracle_case("hc", "", 4, 8, 16, 2, "A", fresh, nu=1.0)
    rng = np.random.RandomState(4 * 8)
    assert np.array_equal(case["buf"]["observations"], rng.randn(8, 4, 18).astype(np.float32)) and case["lr"] == 3e-4
    assert (od, ad) == (18, 6) and ps.update_policy("ant")[2:] == (113, 8) and ps.update_policy((49, 3))[2:] == (49, 3)
    other = W.update_case(17, 5, "L1", "A")[0]
    assert other["buf"]["observations"].shape == (30, 4, 17) and other["buf"]["actions"].shape == (30, 4, 5)
    assert not np.array_equal(other["buf"]["observations"][:8, :, :17], case["buf"]["observations"][:, :, :17])


@pytest.mark.parametrize("obs,act,layout,hset", W.ORACLE_CASES, ids=[f"o{o}a{a}-{lay}-{h}" for o, a, lay, h in W.ORACLE_CASES])
def test_update_cases(obs, act, layout, hset):
    """check_trace as it stands, on every optimiser step; C1 (both signs from 2 actions on); C6 against the counter-state a log_std mix-up
    amounts to; the oracle's moments are there to compare with."""
    case, sd0 = W.check_update_inputs(obs, act, layout, hset)
    assert len(case["trace"]) == W.n_steps(layout) and set(case["exp_avg"]) == set(case["exp_avg_sq"]) == set(case["params"])
    assert all(np.isfinite(v).all() and np.abs(v).max() > 0 for v in case["exp_avg_sq"].values())


@pytest.mark.parametrize("obs,act", W.PADDED_NORM_WIDTHS)
def test_inputs_see_a_norm_over_the_padded_first_layer(obs, act):
    """The fault the sweep is aimed at, on the oracle's side: the gradient norm taken over W1 padded to 16 nt1 columns, the pad columns holding
    component O - 1.  Under set A (the norm clip active at every step) the parameters after the update differ from the true oracle's by more
    than 10 update bounds — a kernel that forgets the mask in its norm cannot pass test_update_vs_oracle_at_width on these inputs.
    Measured: 38, 19 and 12.3 bounds (width_cases.PADDED_NORM_WIDTHS has the figures of the other layout and seeds)."""
    lay = W.PADDED_NORM_LAYOUT
    case, sd0 = W.check_update_inputs(obs, act, lay, "A")
    assert all(t["grad_norm"] > case["hp"]["max_grad_norm"] for t in case["trace"])
    got = W.padded_norm_update(obs, act, lay)
    dev = max(float(np.abs(got[k] - case["params"][k]).max()) for k in got)
    bound = W.ADAM_DEV_BOUND * case["lr"] * W.n_steps(lay) + 2e-7
    print(f"PADDED_NORM o{obs}a{act} {lay}: max |faulty - oracle| = {dev:.3g} = {dev / bound:.1f} bounds")
    assert dev > W.PADDED_NORM_SHIFT * bound, (dev, bound, dev / bound)


@pytest.mark.parametrize("obs,act,n", W.ROW_CASES, ids=[f"o{o}a{a}-{n}" for o, a, n in W.ROW_CASES])
def test_per_row_cases(obs, act, n):
    """C1, C6 and (from 5 actions on) C5 of the per-row cases; the oracle's own float32 rounding (against float64) stays within a third of the
    forward bound, so the bound needs no re-derivation at these widths."""
    op, net_arch, od, ad, fresh, x, acts, noise = W.check_rows(obs, act, n)
    assert (od, ad, net_arch) == (obs, act, None) and x.shape == (n, obs) and acts.shape == noise.shape == (n, act)
    t = torch.as_tensor
    for tag, kw in (("eval", dict(act=acts)), ("forward", dict(noise=noise)), ("deterministic", dict(deterministic=True))):
        _, x64 = ps.f64_deviation(op, x, **kw)
        with torch.no_grad():
            x32 = op.evaluate_actions(t(x), t(acts)) if tag == "eval" else op.forward(t(x), None if tag == "deterministic" else t(noise), tag == "deterministic")
        for (k, r), g in zip(x64.items(), x32):
            assert 3 * nc.in_bounds(g.numpy().reshape(-1), r.numpy().reshape(-1), ps.FWD_RTOL, ps.FWD_ATOL) <= 1.0, (tag, k)
