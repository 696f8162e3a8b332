"""CPU: analytic costs (icrl_cost_fn_t / true_constraint_net.AnalyticCost) — descriptor layout, the exported entry point, the host-side
refusals (argument checks run before any launch: no GPU needed) and the numpy forms against the reference's closed forms
(icrl/true_constraint_net.py:13-54, 104-111) written out here."""
import ctypes

import numpy as np
import pytest


def _lib():
    import os
    from icrl_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L


def test_descriptor_layout_aliases_the_constraint_net_header():
    from icrl_amd import structs as S
    assert ctypes.sizeof(S.CostFnT) == 6 * 4 + 2 * 8
    for name in ("obs_dim", "acs_dim", "in_dim", "n_hidden"):
        assert getattr(S.CostFnT, name).offset == getattr(S.CostNetT, name).offset, name
    assert S.CostFnT.n_hidden.offset == 12 and S.CostFnT.kind.offset == 16 and S.CostFnT.lo.offset == 24
    assert S.COST_FN == -1
    from icrl_amd.true_constraint_net import AnalyticCost
    cf = AnalyticCost.wall_behind_and_infront(-3, 3, index=2).struct(18, 6)
    assert (cf.obs_dim, cf.acs_dim, cf.in_dim, cf.n_hidden, cf.kind, cf.index, cf.lo, cf.hi) == (18, 6, 0, -1, S.COST_WALL_BOTH, 2, -3.0, 3.0)


def test_entry_point_is_declared_exported_and_the_version_stays():
    import os
    import re
    L = _lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "icrl_hip.h")).read(), flags=re.S)
    assert re.search(r"\bicrl_cost_fn_rows\s*\(", src) and "icrl_cost_fn_t" in src and "ICRL_COST_FN" in src
    assert hasattr(L.lib(), "icrl_cost_fn_rows") and len(L.SIGNATURES["icrl_cost_fn_rows"]) == 6
    assert L.lib().icrl_abi_version() == 107


def _refused(err, L, text):
    assert err == 1
    msg = L.lib().icrl_last_error().decode()
    assert text in msg, msg
    L.lib().icrl_clear_error()


def _rollout_args(S, discrete=False):
    env = S.EnvT(4, 18, 1 if discrete else 6, 1000, 0, 0, 0, 0)
    nm = S.NormT(1, 1, 1, 1)
    pol = S.PolicyT(18, 2 if discrete else 6, 64, 64, 1 if discrete else 0, 1, None, None)
    buf = S.BufferT(8, 4, 18, 1 if discrete else 6)
    ag = S.AgentT()
    return env, nm, pol, buf, ag


@pytest.mark.parametrize("fields,discrete,text", [
    (dict(kind=7), False, "unknown kind 7"),
    (dict(kind=-1), False, "unknown kind -1"),
    (dict(kind=1, index=18), False, "column 18 outside the observation (obs_dim 18)"),
    (dict(kind=2, index=-1), False, "column -1 outside the observation"),
    (dict(kind=3, index=200), False, "column 200 outside the observation"),
    (dict(kind=4), True, "torque cost needs a Box action space"),
    (dict(kind=5, index=1), False, "action-equals cost needs a discrete action space"),
    (dict(kind=1, in_dim=3), False, "in_dim = 3 (must be 0)"),
])
def test_rollout_entry_points_refuse_a_bad_descriptor(fields, discrete, text):
    from icrl_amd import structs as S
    L = _lib()
    b = ctypes.byref
    env, nm, pol, buf, ag = _rollout_args(S, discrete)
    cf = S.CostFnT(18, 2 if discrete else 6, fields.get("in_dim", 0), S.COST_FN, fields["kind"], fields.get("index", 0), 0.0, 0.0)
    err = L.lib().icrl_rollout_collect_ex(b(env), b(nm), b(pol), b(cf), b(buf), b(ag), None, None, None, 0.99, 0.95, 0.99, 0.95, 1, None)
    _refused(err, L, text)
    err = L.lib().icrl_rollout_collect(b(env), b(nm), b(pol), b(cf), b(buf), b(ag), None, None, None, 0.99, 0.95, 0.99, 0.95, None)
    _refused(err, L, text)
    hs = S.HostStepT(8, 0)
    err = L.lib().icrl_host_step(b(nm), b(pol), b(cf), b(buf), b(ag), b(hs), None, None, None, 0, None)
    _refused(err, L, text)
    if "action space" not in text:          # (the rows entry point sees no policy: the action-space pairing is the rollouts' check)
        _refused(L.lib().icrl_cost_fn_rows(b(cf), None, None, 4, None, None), L, text)
        _refused(L.lib().icrl_cost_mlp_forward(b(cf), None, None, 4, None, None), L, text)


def test_entry_points_without_an_analytic_form_refuse_the_descriptor():
    """seed batches, constraint-net training, the discriminator reward and the two prepare calls take constraint nets only."""
    from icrl_amd import structs as S
    L = _lib()
    b = ctypes.byref
    lib = L.lib()
    text = "analytic cost descriptor (n_hidden == ICRL_COST_FN) is not served here"
    env, nm, pol, buf, ag = _rollout_args(S)
    cf = S.CostFnT(18, 6, 0, S.COST_FN, S.COST_WALL_BEHIND, 0, -3.0, 0.0)
    job = S.RolloutJobT(S.addr(env), S.addr(nm), S.addr(pol), S.addr(cf), S.addr(buf), S.addr(ag), None)
    scratch = (ctypes.c_char * 4096)()
    _refused(lib.icrl_rollout_collect_batch(1, b(job), None, None, 0.99, 0.95, 0.99, 0.95, 1, ctypes.addressof(scratch), 4096, None), L, text)
    mon_sig = L.SIGNATURES.get("icrl_rollout_collect_batch_mon")
    assert mon_sig is not None
    _refused(lib.icrl_rollout_collect_batch_mon(1, b(job), None, None, None, 0.99, 0.95, 0.99, 0.95, 1, ctypes.addressof(scratch), 4096, None), L, text)
    hp = S.CnHyperT(2, 1, 0, 0)
    _refused(lib.icrl_cn_train(b(cf), None, None, None, None, None, 64, 64, None, None, 2, b(hp), None, None, None), L, text)
    _refused(lib.icrl_cn_train_minibatch(b(cf), None, None, None, None, None, 64, 64, None, None, 2, b(hp), None, 16, None, None, None), L, text)
    tj = S.CnTrainJobT(S.addr(cf), None, None, None, None, None, 64, 64, None, None, 2, 0, S.addr(hp), None, None)
    _refused(lib.icrl_cn_train_batch(1, b(tj), ctypes.addressof(scratch), 4096, None), L, text)
    _refused(lib.icrl_disc_reward(b(cf), None, None, 4, None, 0, None), L, text)
    _refused(lib.icrl_costnet_prepare(b(cf), None), L, text)
    _refused(lib.icrl_cn_prepare(b(cf), None, None, 4, None, None), L, text)
    # icrl_is_weights takes network OUTPUTS, no descriptor: there is nothing of an analytic cost it could be handed


# ---- numpy forms against the reference's closed forms ---------------------------------------------------------------------------------
from helpers.cost_fn_cases import boundary_acs, boundary_obs  # noqa: E402


@pytest.mark.parametrize("lo,hi,index", [(-3, 3, 0), (0.1, 0.7, 2), (0.25, -0.25, 1)])
def test_wall_kinds_equal_the_closed_forms_at_the_thresholds(lo, hi, index):
    from icrl_amd.true_constraint_net import AnalyticCost
    obs = boundary_obs(lo, hi, index)
    col = obs[:, index]
    got = AnalyticCost.wall_behind(lo, index)(obs, None)
    assert got.dtype == np.bool_ and np.array_equal(got, col <= lo)
    assert list(got[:3]) == [True, True, False]
    got = AnalyticCost.wall_infront(hi, index)(obs, None)
    assert got.dtype == np.bool_ and np.array_equal(got, col >= hi)
    assert list(got[3:6]) == [False, True, True]
    got = AnalyticCost.wall_behind_and_infront(lo, hi, index)(obs, None)
    want = (col <= lo).astype(np.float32) + (col >= hi).astype(np.float32)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    if lo >= hi:
        assert got.max() == 2.0
    # leading batch dimensions as the reference's functions take them
    obs3 = np.stack([obs, obs[::-1]])
    assert np.array_equal(AnalyticCost.wall_behind(lo, index)(obs3, None), obs3[..., index] <= lo)


def test_torque_compares_in_float32_around_a_threshold_that_is_not_representable():
    from icrl_amd.true_constraint_net import AnalyticCost
    thr = 0.3
    acs = boundary_acs(thr)
    got = AnalyticCost.torque(thr)(np.zeros((acs.shape[0], 3)), acs)
    t32 = np.float32(thr)
    want = np.array([any(abs(np.float32(v)) > t32 for v in row) for row in acs])
    assert got.dtype == np.bool_ and np.array_equal(got, want)
    assert np.float64(t32) != thr and want.any() and not want.all()
    assert np.array_equal(AnalyticCost.torque(thr)(None, acs), want)          # obs is not read
    assert np.array_equal(AnalyticCost.torque(thr)(None, np.stack([acs, -acs])), np.stack([want, want]))


def test_null_and_action_equals():
    from icrl_amd.true_constraint_net import AnalyticCost, lap_grid_world, null_cost
    obs = np.ones((5, 2, 3))
    got = AnalyticCost.null()(obs)
    assert got.dtype == np.float64 and got.shape == (5,) and np.array_equal(got, null_cost(obs)) and not got.any()
    acs = np.array([[0], [1], [1], [0], [2]])
    got = AnalyticCost.action_equals(1)(None, acs)
    assert got.dtype == np.bool_ and np.array_equal(got, [False, True, True, False, False])
    assert np.array_equal(got, lap_grid_world(None, acs)) and np.array_equal(AnalyticCost.action_equals(1)(None, acs[:, 0]), got)
    assert np.array_equal(AnalyticCost.action_equals(2)(None, acs.astype(np.float32)), [False, False, False, False, True])


def test_true_cost_table_is_the_references(capsys):
    from icrl_amd import structs as S
    from icrl_amd.true_constraint_net import AnalyticCost, get_true_cost_function, null_cost
    def fields(c):
        assert isinstance(c, AnalyticCost)
        return (c.kind, c.index, float(c.lo), float(c.hi))
    for env_id in ("HCWithPosTest-v0", "WalkerWithPosTest-v0", "SwimmerWithPosTest-v0", "AntWallTest-v0", "AntWallBrokenTest-v0", "PointCircleTestBack-v0"):
        assert fields(get_true_cost_function(env_id)) == (S.COST_WALL_BEHIND, 0, -3.0, 0.0), env_id
    for env_id in ("PointNullRewardTest-v0", "PointCircleTest-v0", "AntCircleTest-v0"):
        assert fields(get_true_cost_function(env_id)) == (S.COST_WALL_BOTH, 0, -3.0, 3.0), env_id
    for env_id in ("AntTest-v0", "HalfCheetahTest-v0", "Walker2dTest-v0", "SwimmerTest-v0"):
        assert fields(get_true_cost_function(env_id))[::2] == (S.COST_TORQUE, 0.5), env_id
    assert fields(get_true_cost_function("CLGW-v0"))[:2] == (S.COST_ACTION_EQUALS, 1)
    assert capsys.readouterr().out == ""
    for env_id in ("HCWithPos-v0", "CDD2B-v0", "LGW-v0"):      # unknown here (the bridge envs need the reference's gym env): the null cost, announced
        assert get_true_cost_function(env_id) is null_cost
    out = capsys.readouterr().out
    assert "Cost function for CDD2B-v0 is not implemented yet. Returning null cost function" in out and out.count("\n") == 3
    assert get_true_cost_function("HCWithPosTest-v0")(np.array([[-3.5, 0.]]), None)[0]
    assert not get_true_cost_function("HCWithPosTest-v0")(np.array([[-2.5, 0.]]), None)[0]
