"""CPU: the host side of icrl_policy_fwd_bwd / icrl_cost_mlp_fwd_bwd (csrc/mlp_grad.hip) and of icrl_amd/torch_ops.py — the exports, every refusal
with its reason (argument checks run on the host before the first device call: on a machine without a GPU any device call would return another
error than hipErrorInvalidValue, so `== 1` with a reason shows that none was made), the workspace sizes, and the cases' own conditions."""
import ctypes
import os
import re

import numpy as np
import pytest

from helpers import mlp_grad_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("icrl_policy_fwd_bwd_ws_bytes", "icrl_policy_fwd_bwd", "icrl_cost_mlp_fwd_bwd_ws_bytes", "icrl_cost_mlp_fwd_bwd")
ANT_PARAMS = 8 + 3 * (64 * 113 + 64 + 64 * 64 + 64) + 8 * 64 + 8 + 65 + 65


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


def _cn(in_dim=24, hidden=(20,), n_params=None, params=1):
    from icrl_amd import structs as S
    h = list(hidden) + [0] * (4 - len(hidden))
    if n_params is None:
        n_params, last = 0, in_dim
        for w in list(hidden) + [1]:
            n_params, last = n_params + w * last + w, w
    return S.CostNetT(18, 6, in_dim, len(hidden), h[0], h[1], h[2], h[3], 0, n_params, 10.0, None, None, None, None, None, 1e-5, params, None)


def test_the_four_symbols_are_declared_exported_and_bound():
    _lib_mod, L = _lib()
    src = open(os.path.join(ROOT, "include", "icrl_hip.h")).read()
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", src), f"{name} is not declared in include/icrl_hip.h"
        assert hasattr(L, name) and name in _lib_mod.SIGNATURES
    assert _lib_mod.RESTYPES["icrl_policy_fwd_bwd_ws_bytes"] is ctypes.c_size_t and _lib_mod.RESTYPES["icrl_cost_mlp_fwd_bwd_ws_bytes"] is ctypes.c_size_t
    assert L.icrl_abi_version() == 107
    assert os.path.exists(os.path.join(ROOT, "icrl_amd", "csrc", "mlp_grad.hip"))


def _refused(L, err, pattern):
    assert err == 1, err      # hipErrorInvalidValue, not what a device call without a device returns
    reason = L.icrl_last_error().decode()
    L.icrl_clear_error()
    assert re.search(pattern, reason), reason


POLICY_REFUSALS = [
    (dict(arch=True), 64, r"`arch` array is not served.*h1 == h2 <= 64"),
    (dict(h1=32, h2=64), 64, r"hidden widths \(32, 64\).*h1 == h2 <= 64"),
    (dict(h1=128, h2=128), 64, r"hidden widths \(128, 128\).*h1 == h2 <= 64"),
    (dict(obs=129), 64, r"obs_dim 129 \(1\.\.128\)"),
    (dict(act=17), 64, r"act_dim 17 \(1\.\.16\)"),
    (dict(), 0, r"N = 0 rows \(1\.\.65536\)"),
    (dict(), 65537, r"N = 65537 rows \(1\.\.65536\)"),
    (dict(n_params=5), 64, r"n_params 5, the layout of \(18, 6, 64, 64\) has 16654"),
]


@pytest.mark.parametrize("kw,n,pattern", POLICY_REFUSALS)
def test_policy_shapes_outside_the_served_set_are_refused_with_the_limit(kw, n, pattern):
    _, L = _lib()
    keep = np.ascontiguousarray([0, 2, 64, 64, 2, 64, 64, 2, 64, 64], dtype=np.int32)
    kw = dict(kw)
    if kw.pop("arch", False):
        kw["arch"] = keep.ctypes.data
    pol = _pol(**kw)
    assert L.icrl_policy_fwd_bwd_ws_bytes(ctypes.byref(pol), n) == 0
    _refused(L, 1, pattern)
    one = ctypes.c_void_p(1)      # (never dereferenced: the call is refused on the host)
    err = L.icrl_policy_fwd_bwd(ctypes.byref(pol), one, one, n, *([None] * 8), None, None, 0, None)
    _refused(L, err, pattern)


def test_policy_pointers_and_workspace_are_checked():
    _, L = _lib()
    one = ctypes.c_void_p(1)
    pol = _pol()
    need = L.icrl_policy_fwd_bwd_ws_bytes(ctypes.byref(pol), 64)
    assert need == 4 * 16654 * 8
    _refused(L, L.icrl_policy_fwd_bwd(None, one, one, 64, *([None] * 8), None, None, 0, None), "NULL policy descriptor")
    _refused(L, L.icrl_policy_fwd_bwd(ctypes.byref(pol), None, one, 64, *([None] * 8), None, None, 0, None), "NULL argument.*obs and actions are required")
    _refused(L, L.icrl_policy_fwd_bwd(ctypes.byref(pol), one, None, 64, *([None] * 8), None, None, 0, None), "NULL argument.*obs and actions are required")
    _refused(L, L.icrl_policy_fwd_bwd(ctypes.byref(_pol(params=None)), one, one, 64, *([None] * 8), None, None, 0, None), r"NULL argument \(pol->params")
    _refused(L, L.icrl_policy_fwd_bwd(ctypes.byref(pol), one, one, 64, one, *([None] * 7), None, None, 0, None), "upstream gradients without `grad`")
    _refused(L, L.icrl_policy_fwd_bwd(ctypes.byref(pol), one, one, 64, *([None] * 8), one, None, 0, None), rf"ws of 0 bytes.*= {need}")
    _refused(L, L.icrl_policy_fwd_bwd(ctypes.byref(pol), one, one, 64, *([None] * 8), one, one, need - 1, None), rf"ws of {need - 1} bytes.*= {need}")


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
def test_constraint_nets_outside_the_served_set_are_refused_with_the_limit(kw, n, pattern):
    _, L = _lib()
    cn = _cn(**kw)
    assert L.icrl_cost_mlp_fwd_bwd_ws_bytes(ctypes.byref(cn), n) == 0
    _refused(L, 1, pattern)
    _refused(L, L.icrl_cost_mlp_fwd_bwd(ctypes.byref(cn), ctypes.c_void_p(1), n, None, None, None, None, 0, None), pattern)


def test_tagged_cost_descriptors_pointers_and_workspace_are_refused():
    from icrl_amd import structs as S
    _, L = _lib()
    one = ctypes.c_void_p(1)
    fn = S.CostFnT(18, 6, 0, S.COST_FN, S.COST_NULL, 0, 0.0, 0.0)
    inner = _cn()
    disc = S.CostDiscT(18, 6, 24, S.COST_DISC, ctypes.addressof(inner))
    for d, pattern in ((fn, "analytic cost descriptor"), (disc, "discriminator cost descriptor")):
        assert L.icrl_cost_mlp_fwd_bwd_ws_bytes(ctypes.byref(d), 64) == 0
        _refused(L, 1, "icrl_cost_mlp_fwd_bwd_ws_bytes: an? " + pattern)
        _refused(L, L.icrl_cost_mlp_fwd_bwd(ctypes.byref(d), one, 64, None, None, None, None, 0, None), "icrl_cost_mlp_fwd_bwd: an? " + pattern)
    cn = _cn()
    need = L.icrl_cost_mlp_fwd_bwd_ws_bytes(ctypes.byref(cn), 64)
    assert need == 4 * 521 * 8
    _refused(L, L.icrl_cost_mlp_fwd_bwd(None, one, 64, None, None, None, None, 0, None), "NULL constraint-net descriptor")
    _refused(L, L.icrl_cost_mlp_fwd_bwd(ctypes.byref(cn), None, 64, None, None, None, None, 0, None), "NULL argument.*x are required")
    _refused(L, L.icrl_cost_mlp_fwd_bwd(ctypes.byref(_cn(params=None)), one, 64, None, None, None, None, 0, None), r"NULL argument \(cn->params")
    _refused(L, L.icrl_cost_mlp_fwd_bwd(ctypes.byref(cn), one, 64, one, None, None, None, 0, None), "d_zeta and grad go together")
    _refused(L, L.icrl_cost_mlp_fwd_bwd(ctypes.byref(cn), one, 64, None, None, one, None, 0, None), "d_zeta and grad go together")
    _refused(L, L.icrl_cost_mlp_fwd_bwd(ctypes.byref(cn), one, 64, one, None, one, None, 0, None), rf"ws of 0 bytes.*= {need}")
    _refused(L, L.icrl_cost_mlp_fwd_bwd(ctypes.byref(cn), one, 64, one, None, one, one, need - 4, None), rf"ws of {need - 4} bytes.*= {need}")


def test_workspace_sizes_are_monotone_in_n_and_capped():
    _, L = _lib()
    ant = _pol(113, 8)
    assert ant.n_params == ANT_PARAMS
    cn = _cn(121, (40, 40))
    for d, fn in ((ant, L.icrl_policy_fwd_bwd_ws_bytes), (cn, L.icrl_cost_mlp_fwd_bwd_ws_bytes)):
        rows = [1, 2, 15, 16, 17, 64, 128, 1000, 1024, 1025, 4096, 65535, 65536]
        sizes = [fn(ctypes.byref(d), n) for n in rows]
        assert all(s >= 8 * d.n_params for s in sizes), sizes
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
        assert sizes[-1] == sizes[rows.index(1024)] == 64 * 8 * d.n_params      # a capped number of partial sums, not one per tile
        assert sizes[-1] <= 64 * 2 ** 20
    assert L.icrl_last_error() == b""


def test_torch_ops_imports_without_a_gpu():
    import icrl_amd.torch_ops as T
    assert callable(T.evaluate_actions) and callable(T.zeta) and callable(T.leaf)


def test_the_dev32_table_covers_every_case():
    """one bound per parameter tensor of every case; zero only where float32 and float64 agree by construction: the bias of a value head
    at N = 1, whose gradient is the single upstream value itself."""
    for s, n in M.POLICY_CASES:
        d = M.DEV32[M.case_id(s, n)]
        names = list(M.trained_state(s))
        assert len(d) == len(names)
        for k, v in zip(names, d):
            assert v > 0 or (n == 1 and k in ("value_net.bias", "cost_value_net.bias")), (s, n, k)
    for s, n in M.COST_CASES:
        d = M.DEV32["cost-" + M.case_id(s, n)]
        assert len(d) == 2 * (len(M.COST_SHAPES[s][2]) + 1) and all(v > 0 for v in d), (s, n, d)


@pytest.mark.parametrize("shape,n", M.COST_CASES)
def test_no_relu_of_a_cost_case_sits_on_its_kink(shape, n):
    c = M.cost_case(shape, n)
    assert c["zmin"] >= M.RELU_MARGIN, c["zmin"]
    assert c["x"].shape == (n, c["in_dim"]) and c["x"].dtype == np.float32

