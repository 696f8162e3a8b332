"""CPU: the cost-shaping callback's entry points (icrl_cls_mlp_ws_bytes, icrl_cls_mlp_step, icrl_cost_shaping_apply) are declared, exported
and bound, and refuse what they do not serve on the host before any device call; `gail` keeps -ucsc / -ucn and refuses the flag, by name,
where it is not served; tests/golden/g27_cost_shaping.npz satisfies its cap conditions when they are recomputed from the stored arrays, and
the float32 twin of tests/helpers/cost_shaping_cases reproduces what the reference's callback recorded."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from helpers import cost_shaping_cases as S

NAMES = ("icrl_cls_mlp_ws_bytes", "icrl_cls_mlp_step", "icrl_cost_shaping_apply")
FLAG = "--use_cost_shaping_callback (-ucsc)"


def _lib():
    from icrl_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L


def _refused(err, L, text):
    assert err == 1
    msg = L.lib().icrl_last_error().decode()
    assert text in msg, msg
    L.lib().icrl_clear_error()


def test_entry_points_are_declared_exported_and_bound():
    L = _lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "icrl_hip.h")).read(), flags=re.S)
    for name, n_args in zip(NAMES, (5, 20, 14)):
        decl = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^;]*)\)\s*;" % name, src)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == n_args == len(L.SIGNATURES[name]), name
        assert hasattr(L.lib(), name)
    assert L.RESTYPES["icrl_cls_mlp_ws_bytes"] is ctypes.c_size_t
    assert L.lib().icrl_abi_version() == 107           # exports only: no struct and no existing signature changed


FAKE = ctypes.c_void_p(4096)      # non-NULL and never dereferenced on the host: a refusal comes before any device call


def _step(L, rows=32, in_a=18, in_b=6, h1=50, h2=50, ws_bytes=1 << 40, null=None):
    names = ["params", "exp_avg", "exp_avg_sq", "adam_step", "xa", "xb", "target", "out4", "ws"]
    q = {n: (None if n == null else FAKE) for n in names}
    return L.lib().icrl_cls_mlp_step(q["params"], q["exp_avg"], q["exp_avg_sq"], q["adam_step"], q["xa"], q["xb"], q["target"], rows, in_a, in_b, h1, h2,
                                     3e-3, 0.9, 0.999, 1e-8, q["out4"], q["ws"], ws_bytes, None)


def _apply(L, rows=32, in_a=18, in_b=6, h1=50, h2=50, ws_bytes=1 << 40, null=None, params=FAKE):
    names = ["xa", "xb", "target", "rewards", "out4", "ws"]
    q = {n: (None if n == null else FAKE) for n in names}
    return L.lib().icrl_cost_shaping_apply(params, q["xa"], q["xb"], q["target"], rows, in_a, in_b, h1, h2, q["rewards"], q["out4"], q["ws"], ws_bytes, None)


@pytest.mark.parametrize("kwargs,text", [
    (dict(rows=0), "rows = 0 (1..2097152)"),
    (dict(rows=(1 << 21) + 1), "rows = 2097153 (1..2097152)"),
    (dict(h1=65), "hidden layers (65, 50) are not served"),
    (dict(h2=0), "hidden layers (50, 0) are not served"),
    (dict(in_b=0), "in_b 0 (1..16)"),
    (dict(in_b=17), "in_b 17 (1..16)"),
    (dict(in_a=129), "in_a 129 (0..128)"),
    (dict(in_a=-1), "in_a -1 (0..128)"),
])
def test_unserved_shapes_are_refused_on_the_host(kwargs, text):
    L = _lib()
    _refused(_step(L, **kwargs), L, "icrl_cls_mlp_step: " + text)
    _refused(_apply(L, **kwargs), L, "icrl_cost_shaping_apply: " + text)
    _refused(_apply(L, params=None, **kwargs), L, "icrl_cost_shaping_apply: " + text)
    a = dict(rows=32, in_a=18, in_b=6, h1=50, h2=50); a.update(kwargs)
    assert L.lib().icrl_cls_mlp_ws_bytes(a["rows"], a["in_a"], a["in_b"], a["h1"], a["h2"]) == 0
    _refused(1, L, "icrl_cls_mlp_ws_bytes: " + text)


@pytest.mark.parametrize("null", ["params", "exp_avg", "exp_avg_sq", "adam_step", "xa", "xb", "target", "out4"])
def test_step_refuses_null_required_pointers(null):
    L = _lib()
    _refused(_step(L, null=null), L, "icrl_cls_mlp_step: NULL argument")


def test_step_takes_a_null_xa_only_without_columns_of_it():
    L = _lib()
    _refused(_step(L, in_a=0, null="xa", ws_bytes=0), L, "ws of 0 bytes")      # past the pointer check: refused for its ws


def test_apply_refuses_null_required_pointers():
    L = _lib()
    for null in ("rewards", "out4"):
        _refused(_apply(L, null=null), L, "icrl_cost_shaping_apply: NULL argument (rewards and out4")
        _refused(_apply(L, null=null, params=None), L, "icrl_cost_shaping_apply: NULL argument (rewards and out4")
    for null in ("xa", "xb"):
        _refused(_apply(L, null=null), L, "icrl_cost_shaping_apply: NULL argument (with params")
    _refused(_apply(L, null="target", params=None), L, "icrl_cost_shaping_apply: NULL argument (without params: target is required)")
    _refused(_apply(L, null="target", ws_bytes=0), L, "ws of 0 bytes")          # with params the target is not read: refused for its ws


def test_short_workspace_is_refused_and_its_size_is_what_the_contract_says():
    L = _lib()
    n_params = 50 * 24 + 50 + 50 * 50 + 50 + 50 + 1
    need = L.lib().icrl_cls_mlp_ws_bytes(32, 18, 6, 50, 50)
    assert need == 4 * 256 * 8 + 1 * n_params * 4          # the statistics sums, then one slice of partial sums per workgroup (32 rows: one)
    assert L.lib().icrl_cls_mlp_ws_bytes(33, 18, 6, 50, 50) == 4 * 256 * 8 + 2 * n_params * 4
    assert L.lib().icrl_cls_mlp_ws_bytes(1 << 21, 128, 16, 64, 64) == 4 * 256 * 8 + 256 * (64 * 145 + 64 * 65 + 65) * 4
    _refused(_step(L, ws_bytes=need - 1), L, f"ws of {need - 1} bytes, icrl_cls_mlp_ws_bytes(32, 18, 6, 50, 50) = {need}")
    _refused(_step(L, null="ws"), L, "ws of 0 bytes")
    _refused(_apply(L, ws_bytes=8191), L, "ws of 8191 bytes, 8192 are needed")
    _refused(_apply(L, null="ws", params=None), L, "ws of 0 bytes")


def test_the_parser_keeps_its_flags():
    from icrl_amd import gail
    c = vars(gail.build_parser().parse_args(["gail", "-ucsc", "-ucn"]))
    assert c["use_cost_shaping_callback"] and c["use_cost_net"]
    c = vars(gail.build_parser().parse_args(["gail", "--use_cost_shaping_callback"]))
    assert c["use_cost_shaping_callback"] and not c["use_cost_net"]
    c = vars(gail.build_parser().parse_args(["gail"]))
    assert not c["use_cost_shaping_callback"] and not c["use_cost_net"]


def _gail_cfg(*extra, **kw):
    from icrl_amd import gail
    cfg = vars(gail.build_parser().parse_args(["gail", "-s", "0", "-v", "0", "-ucsc", "-ucn", *extra]))
    cfg.update(rank=0, world_size=1)
    cfg.update(kw)
    return types.SimpleNamespace(**cfg)


def test_several_ranks_and_sde_are_refused_before_anything_is_launched(monkeypatch):
    from icrl_amd import gail, utils

    def no_env(*a, **k):
        raise AssertionError("an env was made before the refusal")

    monkeypatch.setattr(utils, "make_train_env", no_env)
    with pytest.raises(ValueError) as e:
        gail.setup(_gail_cfg(world_size=2))
    assert FLAG in str(e.value) and "world_size > 1" in str(e.value) and "diverge across ranks" in str(e.value)
    with pytest.raises(ValueError) as e:
        gail.setup(_gail_cfg("-us"))
    assert FLAG in str(e.value) and "--use_sde (-us) with" in str(e.value)
    from icrl_amd import exploration
    exploration.refuse_cost_shaping(types.SimpleNamespace(use_cost_shaping_callback=False, use_sde=True, world_size=2))      # flag off: nothing


@pytest.mark.parametrize("hidden,text", [([50], "hidden layers [50] are not served"), ([50, 50, 50], "hidden layers [50, 50, 50] are not served"),
                                         ([50, 65], "hidden layers (50, 65) are not served"), ([0, 50], "hidden layers (0, 50) are not served")])
def test_other_hidden_layers_are_refused(hidden, text):
    _lib()
    from icrl_amd.exploration import CostShapingCallback
    with pytest.raises(NotImplementedError) as e:
        CostShapingCallback(lambda o, a: o[..., 0] > 0, 18, 6, True, cost_net_hidden_layers=hidden)
    assert FLAG in str(e.value) and text in str(e.value) and "two hidden layers of 1..64 units each" in str(e.value)


def test_discrete_action_spaces_are_refused():
    _lib()
    from icrl_amd import spaces
    from icrl_amd.exploration import CostShapingCallback
    cb = CostShapingCallback(lambda o, a: o[..., 0] > 0, 2, 4, True)
    model = types.SimpleNamespace(env=types.SimpleNamespace(action_space=spaces.Discrete(4)), policy=types.SimpleNamespace(discrete=True))
    with pytest.raises(ValueError) as e:
        cb.init_callback(model)
    assert FLAG in str(e.value) and "Box action space is needed" in str(e.value)
    assert cb.cost_net is None


@pytest.fixture(scope="module")
def golden():
    return S.load_golden()


@pytest.fixture(scope="module")
def recomputed(golden):
    return {(c, d): S.recompute(golden, c, d) for c in S.CASES for d in (torch.float32, torch.float64)}


def test_fixture_holds_arrays_only_and_stays_small(golden):
    assert os.path.getsize(S.GOLDEN) < 1000 * 1000
    for k in golden.files:
        assert golden[k].dtype.kind in "fi", k
    for c, (obs, act, T, N, hidden) in S.CASES.items():
        assert tuple(golden[f"{c}_hidden"]) == hidden
        assert float(golden[f"{c}_threshold"]) == S.threshold(int(golden[f"{c}_seed"]), c)


@pytest.mark.parametrize("case", list(S.CASES))
def test_fixture_satisfies_its_cap_conditions(golden, case):
    seed = int(golden[f"{case}_seed"])
    for r in range(S.ROLLOUTS):
        _, _, true = S.case_inputs(seed, case, r)
        frac = float(np.mean(true))
        print(f"{case} r{r}: fraction of cost rows {frac:.3f}")
        assert frac == 0.0 if case == "c" else 0.25 <= frac <= 0.75
        assert golden[f"{case}_log_r{r}_32"][0] == np.float32(frac)
        for key, back in ((f"{case}_p_pre_r{r}", lambda v: v), (f"{case}_shaped_r{r}", np.exp)):      # post-step prediction = exp(shaped)
            for v in (golden[key + "_32"].astype(np.float64), S.ref64_of(golden, key)):
                pr = back(v)
                assert np.all((pr >= S.P_LO) & (pr <= S.P_HI)), (key, float(pr.min()), float(pr.max()))
        for j in (2, 3):      # min and max of shaped: the two precisions at least a quarter of a float32 step apart
            assert 4.0 * abs(float(golden[f"{case}_log_r{r}_d64"][j])) >= float(np.spacing(np.abs(golden[f"{case}_log_r{r}_32"][j])))
        d = float(np.max(np.abs(golden[f"{case}_params_r{r}_d64"])))
        print(f"{case} r{r}: max|params32 - params64| = {d:.3e} (cap {1e-3 * S.LR:.1e})")
        assert d <= 1e-3 * S.LR


@pytest.mark.parametrize("case", list(S.CASES))
def test_the_twin_is_what_the_reference_computed(golden, recomputed, case):
    """float32: the twin reproduces the reference's callback — bit for bit in the generator, which runs both in one process on one thread;
    here, where torch may split the 4099-row products over another number of threads, by the rule (another summation order).  float64: it
    reproduces the stored float64 reference up to the fixture's float32 encoding of the distance between the two precisions (2^-22 of that
    distance, and 1e-11 relative for another order of the sums)."""
    r32, r64 = recomputed[case, torch.float32], recomputed[case, torch.float64]
    stems = sorted({k[len(case) + 1:-3] for k in golden.files if k.startswith(case + "_") and k.endswith("_32")})
    assert len(stems) == 5 * S.ROLLOUTS + 2
    for stem in stems:
        ref32 = golden[f"{case}_{stem}_32"]
        ref64 = S.ref64_of(golden, f"{case}_{stem}")
        S.check(f"{case} {stem} (float32 twin)", np.asarray(r32[stem], dtype=np.float32).reshape(ref32.shape), ref32, ref64)
        bound = 1e-11 * max(1.0, float(np.max(np.abs(ref64)))) + 2.0 ** -22 * float(np.max(np.abs(golden[f"{case}_{stem}_d64"])))
        d = float(np.max(np.abs(np.asarray(r64[stem], dtype=np.float64).reshape(ref64.shape) - ref64)))
        print(f"{case} {stem}: max|recomputed64 - ref64| = {d:.3e}, bound {bound:.3e}")
        assert d <= bound, (stem, d, bound)


def test_gail_seed_batches_still_refuse_the_flag():
    from icrl_amd.seed_batch import GailSeedBatch
    with pytest.raises(NotImplementedError, match="use_cost_shaping_callback"):
        GailSeedBatch([_gail_cfg(seed=0), _gail_cfg(seed=1)])
