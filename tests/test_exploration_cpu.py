"""CPU: the exploration callbacks' entry points (icrl_reg_mlp_step, icrl_reg_mlp_ws_bytes, icrl_shape_advantages) are declared, exported and
bound, and refuse what they do not serve on the host before any device call; tests/golden/g25_exploration.npz satisfies its cap conditions
and a float64 torch recomputation from the regenerated planes reproduces its float64 reference; seed batches refuse the two flags."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from helpers import exploration_cases as X

NAMES = ("icrl_reg_mlp_ws_bytes", "icrl_reg_mlp_step", "icrl_shape_advantages")


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
    for name, n_args in zip(NAMES, (6, 22, 4)):
        decl = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^;]*)\)\s*;" % name, src)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == n_args == len(L.SIGNATURES[name]), name
        assert hasattr(L.lib(), name)
    assert L.RESTYPES["icrl_reg_mlp_ws_bytes"] is ctypes.c_size_t
    assert L.lib().icrl_abi_version() == 107           # exports only: no struct and no existing signature changed


def _step(L, rows=32, in_a=18, in_b=6, h1=50, h2=50, out=18, ws_bytes=None, null=None):
    """icrl_reg_mlp_step with non-NULL dummy pointers (never dereferenced on the host: a refusal comes before any device call)."""
    fake = ctypes.c_void_p(4096)
    names = ["params", "exp_avg", "exp_avg_sq", "adam_step", "xa", "xb", "target", "row_err", "out4", "ws"]
    ptrs = {n: (None if n == null else fake) for n in names}
    if ws_bytes is None:
        ws_bytes = 1 << 40
    return L.lib().icrl_reg_mlp_step(ptrs["params"], ptrs["exp_avg"], ptrs["exp_avg_sq"], ptrs["adam_step"], ptrs["xa"], ptrs["xb"], ptrs["target"], rows,
                                     in_a, in_b, h1, h2, out, 3e-3, 0.9, 0.999, 1e-8, ptrs["row_err"], ptrs["out4"], ptrs["ws"], ws_bytes, None)


@pytest.mark.parametrize("kwargs,text", [
    (dict(rows=0), "rows = 0 (1..2097152)"),
    (dict(rows=(1 << 21) + 1), "rows = 2097153 (1..2097152)"),
    (dict(h1=65), "hidden layers (65, 50) are not served"),
    (dict(h2=0), "hidden layers (50, 0) are not served"),
    (dict(in_b=0), "in_b 0 (1..16)"),
    (dict(in_b=17), "in_b 17 (1..16)"),
    (dict(in_a=129), "in_a 129 (0..128)"),
    (dict(out=129), "out 129 (1..128)"),
    (dict(out=0), "out 0 (1..128)"),
])
def test_unserved_shapes_are_refused_on_the_host(kwargs, text):
    L = _lib()
    _refused(_step(L, **kwargs), L, "icrl_reg_mlp_step: " + text)
    a = dict(rows=32, in_a=18, in_b=6, h1=50, h2=50, out=18); a.update(kwargs)
    assert L.lib().icrl_reg_mlp_ws_bytes(a["rows"], a["in_a"], a["in_b"], a["h1"], a["h2"], a["out"]) == 0
    _refused(1, L, "icrl_reg_mlp_ws_bytes: " + text)


@pytest.mark.parametrize("null", ["params", "exp_avg", "exp_avg_sq", "adam_step", "xa", "xb", "target", "out4"])
def test_null_required_pointers_are_refused(null):
    L = _lib()
    _refused(_step(L, null=null), L, "icrl_reg_mlp_step: NULL argument")


def test_short_workspace_is_refused_and_its_size_is_what_the_contract_says():
    L = _lib()
    n_params = 50 * 24 + 50 + 50 * 50 + 50 + 18 * 50 + 18
    need = L.lib().icrl_reg_mlp_ws_bytes(32, 18, 6, 50, 50, 18)
    assert need == 2 * 256 * 8 + 1 * n_params * 4          # the statistics sums, then one slice of partial sums per workgroup (32 rows: one)
    assert L.lib().icrl_reg_mlp_ws_bytes(1 << 21, 128, 16, 64, 64, 128) == 2 * 256 * 8 + 256 * (64 * 145 + 64 * 65 + 128 * 65) * 4
    _refused(_step(L, ws_bytes=need - 1), L, f"ws of {need - 1} bytes, icrl_reg_mlp_ws_bytes(32, 18, 6, 50, 50, 18) = {need}")
    _refused(_step(L, null="ws"), L, "ws of 0 bytes")


def test_shape_advantages_refuses_null_and_no_rows():
    L = _lib()
    fake = ctypes.c_void_p(4096)
    _refused(L.lib().icrl_shape_advantages(None, fake, 4, None), L, "icrl_shape_advantages")
    _refused(L.lib().icrl_shape_advantages(fake, None, 4, None), L, "icrl_shape_advantages")
    _refused(L.lib().icrl_shape_advantages(fake, fake, 0, None), L, "rows = 0")


@pytest.fixture(scope="module")
def golden():
    return X.load_golden()


@pytest.fixture(scope="module")
def recomputed(golden):
    return {(c, t, d): X.recompute(golden, c, t, d) for c in X.CASES for t in ("e", "l") for d in (torch.float32, torch.float64)}


def test_fixture_holds_arrays_only_and_stays_small(golden):
    assert os.path.getsize(X.GOLDEN) < 1000 * 1000
    for k in golden.files:
        assert golden[k].dtype.kind in "fi", k
    for c, (obs, act, T, N, hidden) in X.CASES.items():
        assert tuple(golden[f"{c}_hidden"]) == hidden


@pytest.mark.parametrize("case", list(X.CASES))
def test_fixture_satisfies_its_cap_conditions(golden, recomputed, case):
    for r in range(X.ROLLOUTS):
        assert np.all(golden[f"{case}_l_row_err_r{r}_32"] > 0) and np.all(X.ref64_of(golden, f"{case}_l_row_err_r{r}") > 0)
        obs, act, T, N, _ = X.CASES[case]
        before = X.planes(int(golden[f"{case}_seed"]), r, obs, act, T, N)["rewards"]
        assert np.all(golden[f"{case}_e_rewards_r{r}_32"] > before)
    for tag, nets in (("e", ("pred",)), ("l", ("pred", "cost"))):
        for n in nets:      # the final parameters from the fixture, every step from the recomputation in the two precisions
            d = np.max(np.abs(golden[f"{case}_{tag}_{n}_params_d64"]))
            print(f"{case} {tag} {n}: max|params32 - params64| = {d:.3e} (cap {1e-3 * X.LR:.1e})")
            assert d <= 1e-3 * X.LR
            for r in range(X.ROLLOUTS):
                p32, p64 = recomputed[case, tag, torch.float32][f"{n}_params_r{r}"], recomputed[case, tag, torch.float64][f"{n}_params_r{r}"]
                assert np.max(np.abs(p32 - p64)) <= 1e-3 * X.LR


@pytest.mark.parametrize("case", list(X.CASES))
@pytest.mark.parametrize("tag", ["e", "l"])
def test_float64_recomputation_reproduces_the_float64_reference(golden, recomputed, case, tag):
    """the regenerated planes and the in-test torch step ARE what the reference's callbacks computed: float64 against float64 leaves only
    the order of the sums (1e-11 relative to the largest value is ~1e4 float64 roundings) and the fixture's float32 encoding of the
    distance between its two precisions (2^-23 of that distance)."""
    rec = recomputed[case, tag, torch.float64]
    stems = sorted({k[len(f"{case}_{tag}_"):-3] for k in golden.files if k.startswith(f"{case}_{tag}_") and k.endswith("_32")})
    assert stems
    for stem in stems:
        ref64 = X.ref64_of(golden, f"{case}_{tag}_{stem}")
        bound = 1e-11 * max(1.0, float(np.max(np.abs(ref64)))) + 2.0 ** -22 * float(np.max(np.abs(golden[f"{case}_{tag}_{stem}_d64"])))
        d = float(np.max(np.abs(np.asarray(rec[stem], dtype=np.float64).reshape(ref64.shape) - ref64)))
        print(f"{case} {tag} {stem}: max|recomputed64 - ref64| = {d:.3e}, bound {bound:.3e}")
        assert d <= bound, (stem, d, bound)


def _cfg(**kw):
    return types.SimpleNamespace(use_curiosity_driven_exploration=False, use_lambda_shaping=False, world_size=1, **kw)


@pytest.mark.parametrize("flag,text", [("use_curiosity_driven_exploration", "--use_curiosity_driven_exploration (-ucde)"),
                                       ("use_lambda_shaping", "--use_lambda_shaping (-uls)")])
def test_seed_batches_refuse_the_flags_before_anything_is_set_up(flag, text):
    from icrl_amd import exploration
    from icrl_amd.seed_batch import CpgSeedBatch, SeedBatch
    a, b = _cfg(seed=0), _cfg(seed=1)
    setattr(b, flag, True)
    for ctor in (CpgSeedBatch, SeedBatch):
        with pytest.raises(ValueError) as e:
            ctor([a, b])
        assert text in str(e.value) and "seed batch" in str(e.value)
    c = _cfg(seed=0); setattr(c, flag, True); c.world_size = 2
    with pytest.raises(ValueError) as e:
        exploration.refuse_batched(c)
    assert text in str(e.value) and "world_size > 1" in str(e.value)
    exploration.refuse_batched(_cfg(seed=0))      # flags off: nothing


def test_parsers_keep_their_flags():
    from icrl_amd import cpg, icrl
    c = vars(cpg.build_parser().parse_args(["-uls", "-ucde"]))
    assert c["use_lambda_shaping"] and c["use_curiosity_driven_exploration"]
    assert vars(icrl.build_parser().parse_args(["-ucde"]))["use_curiosity_driven_exploration"]
