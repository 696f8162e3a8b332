"""CPU: the host side of the input gradients (csrc/mlp_grad.hip: icrl_policy_fwd_bwd_in, icrl_cost_mlp_fwd_bwd_in, icrl_cn_prepare_bwd; icrl_amd/torch_ops.py
input_grads, ConstraintNet.input_gradients / saliency, `icrl --cn_saliency`) — the exports, every refusal with its reason (argument checks run on the
host before the first device call: on a machine without a GPU any device call would return another error than hipErrorInvalidValue, so `== 1` with a
reason shows that none was made), the defaults, the flag, and the chain rule through prepare_data stated in numpy against float64 autograd."""
import ctypes
import inspect
import os
import re
import types

import numpy as np
import pytest

from helpers import input_grad_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("icrl_policy_fwd_bwd_in_ws_bytes", "icrl_policy_fwd_bwd_in", "icrl_cost_mlp_fwd_bwd_in_ws_bytes", "icrl_cost_mlp_fwd_bwd_in", "icrl_cn_prepare_bwd")


def _lib():
    from icrl_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib, _lib.lib()


def _pol(obs=18, act=6, h1=64, h2=64, discrete=0, n_params=None, params=1, arch=None):
    from icrl_amd import structs as S
    if n_params is None:
        n_params = (0 if discrete else act) + 3 * (h1 * obs + h1 + h2 * h1 + h2) + act * h2 + act + 2 * (h2 + 1)
    return S.PolicyT(obs, act, h1, h2, discrete, n_params, params, None, arch)


def _cn(in_dim=24, hidden=(20,), n_params=None, params=1, discrete=0, select=1):
    from icrl_amd import structs as S
    h = list(hidden) + [0] * (4 - len(hidden))
    if n_params is None:
        n_params, last = 0, in_dim
        for w in list(hidden) + [1]:
            n_params, last = n_params + w * last + w, w
    return S.CostNetT(18, 6, in_dim, len(hidden), h[0], h[1], h[2], h[3], discrete, n_params, 10.0, select, None, None, None, None, 1e-5, params, None)


def _refused(L, err, pattern):
    assert err == 1, err      # hipErrorInvalidValue, not what a device call without a device returns
    reason = L.icrl_last_error().decode()
    L.icrl_clear_error()
    assert re.search(pattern, reason), reason


def test_the_five_symbols_are_declared_exported_and_bound_with_matching_argument_counts():
    _lib_mod, L = _lib()
    src = open(os.path.join(ROOT, "include", "icrl_hip.h")).read()
    for name in NEW:
        m = re.search(rf"\b{name}\s*\(([^;]*?)\)\s*;", src, re.S)
        assert m, f"{name} is not declared in include/icrl_hip.h"
        assert hasattr(L, name) and name in _lib_mod.SIGNATURES
        assert len(m.group(1).split(",")) == len(_lib_mod.SIGNATURES[name]), name
    assert _lib_mod.RESTYPES["icrl_policy_fwd_bwd_in_ws_bytes"] is ctypes.c_size_t and _lib_mod.RESTYPES["icrl_cost_mlp_fwd_bwd_in_ws_bytes"] is ctypes.c_size_t
    assert L.icrl_abi_version() == 107


POLICY_REFUSALS = [
    (dict(arch=True), 64, r"`arch` array is not served.*h1 == h2 <= 64"),
    (dict(h1=32, h2=64), 64, r"hidden widths \(32, 64\).*h1 == h2 <= 64"),
    (dict(h1=128, h2=128), 64, r"hidden widths \(128, 128\).*h1 == h2 <= 64"),
    (dict(obs=129), 64, r"obs_dim 129 \(1\.\.128\)"),
    (dict(act=17), 64, r"act_dim 17 \(1\.\.16\)"),
    (dict(), 0, r"N = 0 rows \(1\.\.65536\)"),
    (dict(), 65537, r"N = 65537 rows \(1\.\.65536\)"),
    (dict(n_params=5), 64, r"n_params 5, the layout of \(18, 6, 64, 64\) has 16654"),
    (dict(n_params=16654 + 63 * 6), 64, r"n_params 17032, the layout of \(18, 6, 64, 64\) has 16654"),      # a gSDE layout (log_std [64, act_dim])
]


@pytest.mark.parametrize("kw,n,pattern", POLICY_REFUSALS)
def test_policy_shapes_outside_the_served_set_are_refused_under_the_new_names(kw, n, pattern):
    _, L = _lib()
    keep = np.ascontiguousarray([0, 2, 64, 64, 2, 64, 64, 2, 64, 64], dtype=np.int32)
    kw = dict(kw)
    if kw.pop("arch", False):
        kw["arch"] = keep.ctypes.data
    pol = _pol(**kw)
    assert L.icrl_policy_fwd_bwd_in_ws_bytes(ctypes.byref(pol), n) == 0
    _refused(L, 1, "icrl_policy_fwd_bwd_in_ws_bytes: .*" + pattern)
    one = ctypes.c_void_p(1)      # (never dereferenced: the call is refused on the host)
    err = L.icrl_policy_fwd_bwd_in(ctypes.byref(pol), one, one, n, *([None] * 8), one, one, None, one, 1 << 40, None)
    _refused(L, err, "icrl_policy_fwd_bwd_in: .*" + pattern)


def test_policy_pointers_outputs_and_workspace_are_checked():
    _, L = _lib()
    one = ctypes.c_void_p(1)
    pol, fn = _pol(), L.icrl_policy_fwd_bwd_in
    need = L.icrl_policy_fwd_bwd_in_ws_bytes(ctypes.byref(pol), 64)
    assert need == (4 * 16654 + 3 * 64 * 18) * 8      # the parameter sums of four tiles, then three float64 slices [N, obs_dim]
    big = 1 << 40
    _refused(L, fn(None, one, one, 64, *([None] * 8), one, one, None, one, big, None), "NULL policy descriptor")
    _refused(L, fn(ctypes.byref(pol), None, one, 64, *([None] * 8), one, one, None, one, big, None), "NULL argument.*obs and actions are required")
    _refused(L, fn(ctypes.byref(pol), one, None, 64, *([None] * 8), one, one, None, one, big, None), "NULL argument.*obs and actions are required")
    _refused(L, fn(ctypes.byref(_pol(params=None)), one, one, 64, *([None] * 8), one, one, None, one, big, None), r"NULL argument \(pol->params")
    _refused(L, fn(ctypes.byref(pol), one, one, 64, *([None] * 8), None, None, None, one, big, None), "no gradient output.*grad, d_obs and d_actions are all NULL")
    _refused(L, fn(ctypes.byref(pol), one, one, 64, one, *([None] * 7), None, None, None, one, big, None), "no gradient output")
    lgw = _pol(1, 2, discrete=1)
    _refused(L, fn(ctypes.byref(lgw), one, one, 64, *([None] * 8), None, one, one, one, big, None), "d_actions with a discrete policy")
    # grad alone, d_obs alone, d_actions alone: each needs the workspace
    for outs in ((one, None, None), (None, one, None), (None, None, one)):
        _refused(L, fn(ctypes.byref(pol), one, one, 64, *([None] * 8), *outs, None, 0, None), rf"ws of 0 bytes, icrl_policy_fwd_bwd_in_ws_bytes\(pol, 64\) = {need}")
        _refused(L, fn(ctypes.byref(pol), one, one, 64, *([None] * 8), *outs, one, need - 1, None), rf"ws of {need - 1} bytes.*= {need}")


COST_REFUSALS = [
    (dict(hidden=(20, 20, 20)), 64, r"3 hidden layers are not served \(1\.\.2 of up to 64 units\)"),
    (dict(hidden=()), 64, r"0 hidden layers are not served"),
    (dict(hidden=(128,)), 64, r"hidden layers \(128, 0\) are not served \(1\.\.2 of up to 64 units\)"),
    (dict(hidden=(40, 65)), 64, r"hidden layers \(40, 65\) are not served"),
    (dict(in_dim=129), 64, r"in_dim 129 \(1\.\.128\)"),
    (dict(), 0, r"N = 0 rows \(1\.\.65536\)"),
    (dict(), 65537, r"N = 65537 rows"),
    (dict(n_params=7), 64, r"n_params 7, the layout of 24 inputs and \(20, 0\) has 521"),
]


@pytest.mark.parametrize("kw,n,pattern", COST_REFUSALS)
def test_constraint_nets_outside_the_served_set_are_refused_under_the_new_names(kw, n, pattern):
    _, L = _lib()
    cn, one = _cn(**kw), ctypes.c_void_p(1)
    assert L.icrl_cost_mlp_fwd_bwd_in_ws_bytes(ctypes.byref(cn), n) == 0
    _refused(L, 1, "icrl_cost_mlp_fwd_bwd_in_ws_bytes: .*" + pattern)
    _refused(L, L.icrl_cost_mlp_fwd_bwd_in(ctypes.byref(cn), one, n, one, None, one, one, one, 1 << 40, None), "icrl_cost_mlp_fwd_bwd_in: .*" + pattern)


def test_tagged_cost_descriptors_pointers_outputs_and_workspace_are_refused():
    from icrl_amd import structs as S
    _, L = _lib()
    one, big = ctypes.c_void_p(1), 1 << 40
    fn = S.CostFnT(18, 6, 0, S.COST_FN, S.COST_NULL, 0, 0.0, 0.0)
    inner = _cn()
    disc = S.CostDiscT(18, 6, 24, S.COST_DISC, ctypes.addressof(inner))
    region = S.CostRegionT(obs_dim=18, acs_dim=6, in_dim=0, n_hidden=S.COST_REGION, n_clauses=1, combine=S.REGION_ANY, clauses=1, d_clauses=1)
    for d, pattern in ((fn, "analytic cost descriptor"), (disc, "discriminator cost descriptor"), (region, "region cost descriptor")):
        assert L.icrl_cost_mlp_fwd_bwd_in_ws_bytes(ctypes.byref(d), 64) == 0
        _refused(L, 1, "icrl_cost_mlp_fwd_bwd_in_ws_bytes: an? " + pattern)
        _refused(L, L.icrl_cost_mlp_fwd_bwd_in(ctypes.byref(d), one, 64, one, None, one, one, one, big, None), "icrl_cost_mlp_fwd_bwd_in: an? " + pattern)
        _refused(L, L.icrl_cn_prepare_bwd(ctypes.byref(d), one, one, 64, one, one, one, None), "icrl_cn_prepare_bwd: an? " + pattern)
    cn, call = _cn(), L.icrl_cost_mlp_fwd_bwd_in
    need = L.icrl_cost_mlp_fwd_bwd_in_ws_bytes(ctypes.byref(cn), 64)
    assert need == 4 * 521 * 8 == L.icrl_cost_mlp_fwd_bwd_ws_bytes(ctypes.byref(cn), 64)
    _refused(L, call(None, one, 64, one, None, one, one, one, big, None), "NULL constraint-net descriptor")
    _refused(L, call(ctypes.byref(cn), None, 64, one, None, one, one, one, big, None), "NULL argument.*x are required")
    _refused(L, call(ctypes.byref(_cn(params=None)), one, 64, one, None, one, one, one, big, None), r"NULL argument \(cn->params")
    _refused(L, call(ctypes.byref(cn), one, 64, one, None, None, None, one, big, None), "no gradient output.*grad and d_x are both NULL")
    _refused(L, call(ctypes.byref(cn), one, 64, None, None, one, one, one, big, None), "d_zeta is required")
    for outs in ((one, None), (None, one)):
        _refused(L, call(ctypes.byref(cn), one, 64, one, None, *outs, None, 0, None), rf"ws of 0 bytes, icrl_cost_mlp_fwd_bwd_in_ws_bytes\(cn, 64\) = {need}")
        _refused(L, call(ctypes.byref(cn), one, 64, one, None, *outs, one, need - 4, None), rf"ws of {need - 4} bytes.*= {need}")


def test_the_chain_rule_entry_point_checks_its_arguments():
    _, L = _lib()
    one, fn = ctypes.c_void_p(1), L.icrl_cn_prepare_bwd
    cn = _cn()
    _refused(L, fn(None, one, one, 8, one, one, one, None), "icrl_cn_prepare_bwd: NULL constraint-net descriptor")
    _refused(L, fn(ctypes.byref(cn), one, one, 0, one, one, one, None), "icrl_cn_prepare_bwd: N = 0 rows")
    _refused(L, fn(ctypes.byref(cn), one, one, 8, one, None, None, None), "no gradient output.*d_obs and d_acs are both NULL")
    _refused(L, fn(ctypes.byref(_cn(discrete=1)), one, one, 8, one, one, one, None), "d_acs with a discrete net")
    _refused(L, fn(ctypes.byref(cn), one, one, 8, None, one, one, None), "NULL argument.*d_x and cn->select_dim are required")
    _refused(L, fn(ctypes.byref(_cn(select=None)), one, one, 8, one, one, one, None), "NULL argument.*d_x and cn->select_dim are required")
    _refused(L, fn(ctypes.byref(cn), None, one, 8, one, one, one, None), "NULL argument.*obs with d_obs")
    _refused(L, fn(ctypes.byref(cn), one, None, 8, one, one, one, None), "NULL argument.*acs with d_acs")
    assert L.icrl_last_error() == b""


def test_input_grads_defaults_to_false_in_both_functions():
    import icrl_amd.torch_ops as T
    for fn in (T.evaluate_actions, T.zeta):
        sig = inspect.signature(fn)
        assert sig.parameters["input_grads"].default is False
        assert list(sig.parameters)[:4] == list(inspect.signature(fn).parameters)[:4] and list(sig.parameters)[3] == "params"
    from icrl_amd.constraint_net import ConstraintNet
    assert callable(ConstraintNet.input_gradients) and callable(ConstraintNet.saliency)


def test_the_flag_is_absent_from_the_namespace_unless_given():
    from icrl_amd import icrl
    p = icrl.build_parser()
    assert "cn_saliency" not in vars(p.parse_args([]))
    assert vars(p.parse_args(["--cn_saliency"]))["cn_saliency"] is True


def _cfg(**kw):
    from icrl_amd import icrl
    cfg = vars(icrl.build_parser().parse_args(["-s", "0", "-v", "0", "--cn_saliency"]))
    cfg.update(rank=0, world_size=1, save_dir=None)
    cfg.update(kw)
    return types.SimpleNamespace(**cfg)


def test_seed_batches_ranks_and_unserved_nets_refuse_the_flag_by_name_before_anything_is_set_up():
    from icrl_amd import icrl
    from icrl_amd.seed_batch import SeedBatch
    with pytest.raises(ValueError, match="--cn_saliency") as e:
        SeedBatch([_cfg(seed=0), _cfg(seed=1)])
    assert "seed batch" in str(e.value)
    with pytest.raises(ValueError, match="--cn_saliency") as e:      # (setup refuses before it builds an env: no device here)
        icrl.setup(_cfg(world_size=2))
    assert "world_size > 1" in str(e.value)
    for layers in ([64, 64, 64], [128], [40, 96], []):
        with pytest.raises(NotImplementedError, match="--cn_saliency") as e:
            icrl.setup(_cfg(cn_layers=layers))
        assert "one or two hidden layers of up to 64 units" in str(e.value) and str(layers) in str(e.value)
    icrl.refuse_cn_saliency(_cfg())                                     # alone, a served net: nothing
    cfg = _cfg(world_size=4, cn_layers=[128, 128])
    del cfg.cn_saliency
    icrl.refuse_cn_saliency(cfg)                                        # flag not given: nothing
    icrl.refuse_cn_saliency(dict(cn_saliency=False, world_size=2))


@pytest.mark.parametrize("name", G.PREPARE_CASES)
def test_the_chain_rule_through_prepare_data_in_numpy_agrees_with_float64_autograd(name):
    """duplicate and crossed select_dim entries ("dup"), one-hot actions ("onehot"), rows on both sides of both clips (asserted by the case)."""
    c = G.prepare_case(name)
    d_obs, d_acs = G.prepare_bwd_numpy(c["spec"], c["obs"], c["acs"], c["d_x"])
    assert d_obs.dtype == np.float64 and d_obs.shape == c["obs"].shape
    err = np.abs(d_obs - c["d_obs64"])
    print(f"IN prepare {name}: max |numpy - autograd| d_obs = {err.max():.3g}")
    assert np.all(err <= G.PREPARE_RTOL_OBS * np.abs(c["d_obs64"]))
    assert np.count_nonzero(c["d_obs64"]) > 0 and np.count_nonzero(c["d_obs64"] == 0) > 0      # both branches of the clip
    if c["spec"]["is_discrete"]:
        assert d_acs is None and c["d_acs64"] is None
    else:
        assert d_acs.dtype == np.float32
        assert np.all(np.abs(d_acs.astype(np.float64) - c["d_acs64"]) <= G.PREPARE_RTOL_ACS * np.abs(c["d_acs64"]))
    if name == "dup":
        sel = c["spec"]["select_dim"]
        assert len(set(sel)) < len(sel) and any(s < c["spec"]["obs_dim"] for s in sel[4:])      # duplicates; observation columns through acs_select_dim
        assert not d_obs[:, 3].any() and not d_acs[:, 0].any()      # columns nothing selects get exactly 0
        assert np.count_nonzero(d_acs) > 0 and np.count_nonzero(d_acs[:, 1:] == 0) > 0


def test_the_tables_cover_every_case_and_the_cases_keep_their_margins():
    for s, n in G.POLICY_CASES:
        d = G.DEV32[G.case_id(s, n)]
        assert len(d) == (1 if s == "lgw" else 2) and all(v > 0 for v in d), (s, n, d)
    for s, n in G.COST_CASES:
        d = G.DEV32["cost-" + G.case_id(s, n)]
        assert len(d) == (2 if s == "disc" else 3) and d[0] > 0, (s, n, d)
        assert G.case_id(s, n) in G.COST_SEED
    assert len(G.DEV32["loss-policy"]) == 2 and len(G.DEV32["loss-zeta"]) == 2
    for s, n in (("h20", 63), ("point", 1), ("disc", 65)):      # (each case asserts its clip margins and both-sides rows when it is built)
        c = G.cost_case(s, n)
        assert c["zmin"] >= G.RELU_MARGIN, (s, n, c["zmin"])
        assert c["x"].shape == (n, c["in_dim"]) and c["x"].dtype == np.float32
    c = G.policy_case("o17a5", 17)
    assert c["d_obs64"].shape == (17, 17) and c["d_act64"].shape == (17, 5)
    assert np.abs(c["d_obs_sum64"] - c["d_obs64"]).max() <= 1e-12 * np.abs(c["d_obs64"]).max()      # the three branches add up to the whole
