"""CPU: the host side of gSDE (use_sde; csrc/sde.hip, policies.py, ppo_lag.py) — the exports, the matrix log_std's storage, the refusals with their
reasons (argument checks run on the host before the first device call: `== 1` with a reason shows that none was made), the flags' way into the
agent, and the fixture itself: a numpy restatement of the head from its formulas against tests/golden/g26_sde.npz."""
import ast
import ctypes
import inspect
import io
import os
import re
import types
import zipfile

import numpy as np
import pytest
import torch

from helpers import sde_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("icrl_policy_forward_sde", "icrl_policy_sde_fwd_bwd_ws_bytes", "icrl_policy_sde_fwd_bwd")


def _lib():
    from icrl_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib, _lib.lib()


def _refused(L, err, pattern):
    assert err == 1, err
    reason = L.icrl_last_error().decode()
    L.icrl_clear_error()
    assert re.search(pattern, reason), reason


def _n_diag(obs, act, h=64):
    return act + 3 * (h * obs + h + h * h + h) + act * h + act + 2 * (h + 1)


def _pol(obs=18, act=6, h1=64, h2=64, discrete=0, n_params=None, params=1, params_t=1, arch=None, sde=True):
    from icrl_amd import structs as S
    if n_params is None:
        n_params = _n_diag(obs, act, h1) + (63 * act if sde else 0)
    return S.PolicyT(obs, act, h1, h2, discrete, n_params, params, params_t, arch)


def test_the_exports_are_declared_bound_and_the_abi_version_stands():
    _lib_mod, L = _lib()
    src = open(os.path.join(ROOT, "include", "icrl_hip.h")).read()
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", src), f"{name} is not declared in include/icrl_hip.h"
        assert hasattr(L, name) and name in _lib_mod.SIGNATURES
    assert _lib_mod.RESTYPES["icrl_policy_sde_fwd_bwd_ws_bytes"] is ctypes.c_size_t
    assert L.icrl_abi_version() == 107
    from icrl_amd import structs as S
    assert ctypes.sizeof(S.PolicyT) == 6 * 4 + 3 * 8
    assert os.path.exists(os.path.join(ROOT, "icrl_amd", "csrc", "sde.hip"))


@pytest.mark.parametrize("tag", ["hc", "pl"])
def test_log_std_is_a_matrix_stored_64_rows_first_in_the_buffer(tag):
    from icrl_amd.policies import state_dict_names
    O, A, arch = C.SHAPES[tag]
    H = arch["pi"][-1]
    pol = C.policy(tag, device="cpu", load=False)
    assert list(pol.shapes) == state_dict_names(False) and list(pol.shapes)[0] == "log_std"
    assert pol.logical_shapes["log_std"] == (H, A) and pol.shapes["log_std"] == (64, A)
    assert pol.n_params == _n_diag(O, A) + 63 * A
    assert tuple(pol.log_std.shape) == (H, A)
    sd = C.state(tag)
    pol.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    block = pol.params[:64 * A].reshape(64, A).numpy()
    assert np.array_equal(block[:H], sd["log_std"]) and not block[H:].any()
    assert np.array_equal(pol.log_std.numpy(), sd["log_std"])
    back = pol.state_dict()
    assert list(back) == list(sd)
    for k, v in sd.items():
        assert tuple(back[k].shape) == v.shape and np.array_equal(back[k].numpy(), v), k
    osd = pol.optimizer_state_dict(lr=3e-4)
    assert osd["state"] == {} and len(osd["param_groups"][0]["params"]) == len(sd)
    pol.adam_step = 3
    pol.exp_avg[:64 * A] = 1.0
    assert tuple(pol.optimizer_state_dict(lr=3e-4)["state"][0]["exp_avg"].shape) == (H, A)


def test_construction_is_reproducible_and_log_std_starts_at_log_std_init():
    torch.manual_seed(5)
    a = C.policy("pl", device="cpu", load=False).state_dict()
    torch.manual_seed(5)
    b = C.policy("pl", device="cpu", load=False).state_dict()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert float(a["log_std"].abs().max()) == 0.0


def test_policies_outside_the_served_set_are_refused_with_the_limit():
    from icrl_amd import spaces
    from icrl_amd.policies import ActorTwoCriticsPolicy
    o, a = C.spaces_of("hc")
    with pytest.raises(NotImplementedError, match=r"use_sde.*Box action space"):
        ActorTwoCriticsPolicy(o, spaces.Discrete(4), device="cpu", use_sde=True)
    for arch in ([32, dict(pi=[64, 64], vf=[64, 64], cvf=[64, 64])], [dict(pi=[128, 64], vf=[64, 64], cvf=[64, 64])], [dict(pi=[64], vf=[64, 64], cvf=[64, 64])]):
        with pytest.raises(NotImplementedError, match=r"use_sde.*two hidden layers per branch and widths <= 64"):
            ActorTwoCriticsPolicy(o, a, net_arch=arch, device="cpu", use_sde=True)


def test_the_other_entry_points_refuse_a_gsde_descriptor_before_any_device_call():
    _, L = _lib()
    one = ctypes.c_void_p(1)
    pol = _pol()
    assert L.icrl_policy_fwd_bwd_ws_bytes(ctypes.byref(pol), 64) == 0
    _refused(L, 1, r"n_params 17032, the layout of \(18, 6, 64, 64\) has 16654")
    _refused(L, L.icrl_policy_fwd_bwd(ctypes.byref(pol), one, one, 64, *([None] * 8), None, None, 0, None), r"n_params 17032")
    _refused(L, L.icrl_policy_prepare(ctypes.byref(pol), None), r"n_params = 17032, the layout needs 16654")
    _refused(L, L.icrl_policy_forward(ctypes.byref(pol), one, one, 4, 0, *([None] * 7), None), r"n_params = 17032, the layout of \(18, 6, 64, 64\) needs 16654")
    _refused(L, L.icrl_policy_evaluate(ctypes.byref(pol), one, one, 4, *([None] * 4), None), r"n_params = 17032")
    # the Python layer keeps a gSDE policy from every other descriptor user (the fused rollout, update and sampler launches)
    p = C.policy("hc", device="cpu", load=False)
    with pytest.raises(NotImplementedError, match=r"use_sde.*icrl_policy_forward_sde / icrl_policy_sde_fwd_bwd alone"):
        p.struct()
    assert p.struct(sde=True).n_params == 17032


SDE_REFUSALS = [
    (dict(arch=True), 64, r"`arch` array is not served.*h1 == h2 <= 64"),
    (dict(h1=32, h2=64), 64, r"hidden widths \(32, 64\).*h1 == h2 <= 64"),
    (dict(h1=128, h2=128), 64, r"hidden widths \(128, 128\)"),
    (dict(obs=129), 64, r"obs_dim 129 \(1\.\.128\)"),
    (dict(act=17), 64, r"act_dim 17 \(1\.\.16\)"),
    (dict(discrete=1), 64, r"discrete policy has no gSDE head"),
    (dict(), 0, r"N = 0 rows \(1\.\.65536\)"),
    (dict(), 65537, r"N = 65537 rows \(1\.\.65536\)"),
    (dict(sde=False), 64, r"n_params 16654, the gSDE \(log_std \[64, act_dim\]\) layout of \(18, 6, 64, 64\) has 17032"),
]


@pytest.mark.parametrize("kw,n,pattern", SDE_REFUSALS)
def test_shapes_outside_the_served_set_are_refused_by_both_entry_points(kw, n, pattern):
    _, L = _lib()
    keep = np.ascontiguousarray([0, 2, 64, 64, 2, 64, 64, 2, 64, 64], dtype=np.int32)
    kw = dict(kw)
    if kw.pop("arch", False):
        kw["arch"] = keep.ctypes.data
    pol = _pol(**kw)
    one = ctypes.c_void_p(1)
    assert L.icrl_policy_sde_fwd_bwd_ws_bytes(ctypes.byref(pol), n) == 0
    _refused(L, 1, "icrl_policy_sde_fwd_bwd_ws_bytes: .*" + pattern)
    _refused(L, L.icrl_policy_sde_fwd_bwd(ctypes.byref(pol), one, one, n, *([None] * 8), None, None, 0, None), "icrl_policy_sde_fwd_bwd: .*" + pattern)
    _refused(L, L.icrl_policy_forward_sde(ctypes.byref(pol), one, one, 0, n, 0, *([None] * 7), None), "icrl_policy_forward_sde: .*" + pattern)


def test_pointers_strides_and_workspace_are_checked():
    _, L = _lib()
    one = ctypes.c_void_p(1)
    pol = _pol()
    need = L.icrl_policy_sde_fwd_bwd_ws_bytes(ctypes.byref(pol), 64)
    assert need == 4 * 17032 * 8
    assert L.icrl_policy_sde_fwd_bwd_ws_bytes(ctypes.byref(pol), 65536) == 64 * 17032 * 8
    fb = L.icrl_policy_sde_fwd_bwd
    _refused(L, fb(None, one, one, 64, *([None] * 8), None, None, 0, None), "NULL policy descriptor")
    _refused(L, fb(ctypes.byref(pol), None, one, 64, *([None] * 8), None, None, 0, None), "NULL argument.*obs and actions are required")
    _refused(L, fb(ctypes.byref(_pol(params=None)), one, one, 64, *([None] * 8), None, None, 0, None), r"NULL argument \(pol->params")
    _refused(L, fb(ctypes.byref(pol), one, one, 64, one, *([None] * 7), None, None, 0, None), "upstream gradients without `grad`")
    _refused(L, fb(ctypes.byref(pol), one, one, 64, *([None] * 8), one, None, 0, None), rf"ws of 0 bytes.*= {need}")
    _refused(L, fb(ctypes.byref(pol), one, one, 64, *([None] * 8), one, one, need - 1, None), rf"ws of {need - 1} bytes.*= {need}")
    fw = L.icrl_policy_forward_sde
    _refused(L, fw(ctypes.byref(pol), None, one, 0, 4, 0, *([None] * 7), None), "NULL argument.*obs are required")
    _refused(L, fw(ctypes.byref(_pol(params_t=None)), one, one, 0, 4, 0, *([None] * 7), None), r"NULL argument \(pol->params, pol->params_t")
    _refused(L, fw(ctypes.byref(pol), one, None, 0, 4, 0, *([None] * 7), None), "sampled forward needs the exploration matrices")
    _refused(L, fw(ctypes.byref(pol), one, one, 6, 4, 0, *([None] * 7), None), r"expl_stride 6 \(0: one matrix for all rows; 384 = 64 \* act_dim")


def _cfg(**kw):
    base = dict(use_sde=True, use_curiosity_driven_exploration=False, use_lambda_shaping=False, world_size=1, seed=0)
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_seed_batches_callbacks_and_ranks_refuse_the_flag_before_anything_is_set_up():
    from icrl_amd import exploration
    from icrl_amd.seed_batch import CpgSeedBatch, GailSeedBatch, SeedBatch
    for ctor in (CpgSeedBatch, SeedBatch, GailSeedBatch):
        with pytest.raises(ValueError) as e:
            ctor([_cfg(use_sde=False), _cfg(seed=1)])
        assert "--use_sde (-us)" in str(e.value) and "seed batch" in str(e.value)
    for attr, text in (("use_curiosity_driven_exploration", "-ucde"), ("use_lambda_shaping", "-uls")):
        with pytest.raises(ValueError) as e:
            exploration.refuse_sde(_cfg(**{attr: True}))
        assert "--use_sde (-us)" in str(e.value) and text in str(e.value)
    with pytest.raises(ValueError) as e:
        exploration.refuse_sde(_cfg(world_size=2))
    assert "--use_sde (-us)" in str(e.value) and "world_size > 1" in str(e.value)
    exploration.refuse_sde(_cfg())                       # alone: served
    exploration.refuse_sde(_cfg(use_sde=False, use_lambda_shaping=True, world_size=4))      # flag off: nothing
    exploration.refuse_sde(dict(use_sde=False))


def test_the_flags_reach_the_agents_constructor_from_the_three_clis():
    from icrl_amd import cpg, gail, icrl, ppo_lag
    for mod in (cpg, icrl, gail):
        c = vars(mod.build_parser().parse_args(["-us", "-ssf", "8"]))
        assert c["use_sde"] is True and c["sde_sample_freq"] == 8
        assert vars(mod.build_parser().parse_args([]))["use_sde"] is False
        handed = set()
        for node in ast.walk(ast.parse(inspect.getsource(mod))):
            if isinstance(node, ast.Call) and getattr(node.func, "id", None) in ("PPOLagrangian", "PPO"):
                for kw in node.keywords:
                    if kw.arg in ("use_sde", "sde_sample_freq") and isinstance(kw.value, ast.Attribute) and kw.value.attr == kw.arg:
                        handed.add(kw.arg)
        assert handed == {"use_sde", "sde_sample_freq"}, (mod.__name__, handed)
        assert "refuse_sde" in inspect.getsource(mod.setup)
    o, a = C.spaces_of("hc")
    env = types.SimpleNamespace(num_envs=2, observation_space=o, action_space=a)
    agent = ppo_lag.PPOLagrangian("TwoCriticsMlpPolicy", env, use_sde=True, sde_sample_freq=8, _init_setup_model=False)
    assert agent.use_sde is True and agent.sde_sample_freq == 8
    assert gail.PPO("TwoCriticsMlpPolicy", env, use_sde=True, sde_sample_freq=4, _init_setup_model=False).sde_sample_freq == 4


def test_an_archive_of_the_other_kind_fails_with_a_message(tmp_path):
    from icrl_amd.ppo_lag import PPOLagrangian
    diag, sde = C.policy("pl", device="cpu", use_sde=False), C.policy("pl", device="cpu")
    def archive(pol):
        path = str(tmp_path / f"{'sde' if pol.use_sde else 'diag'}.zip")
        with zipfile.ZipFile(path, "w") as z:
            b = io.BytesIO(); torch.save(pol.state_dict(), b)
            z.writestr("policy.pth", b.getvalue())
        return path
    for holder, other, text in ((sde, diag, r"holds a diagonal-Gaussian policy \(use_sde=False, log_std \[A\]\) with log_std of shape \(3,\); this agent has a gSDE policy"),
                                (diag, sde, r"holds a gSDE policy \(use_sde=True, log_std \[H, A\]\) with log_std of shape \(48, 3\); this agent has a diagonal")):
        agent = PPOLagrangian.__new__(PPOLagrangian)
        agent.policy, agent.dual = holder, None
        before = holder.params.clone()
        with pytest.raises(ValueError, match=text):
            agent.load_parameters(archive(other), dual=False)
        assert torch.equal(holder.params, before)
        agent.load_parameters(archive(holder), dual=False)      # its own kind loads


@pytest.mark.parametrize("tag", ["hc", "pl"])
@pytest.mark.parametrize("n", [48, 17, 1])
def test_the_formulas_reproduce_the_fixture(tag, n):
    """the test of the fixture: evaluate_actions' outputs and the log_std gradient of g26 from the head's formulas (tests/helpers/sde_cases.py), to 1e-6 of each array's scale
    against the reference's float32 values on the batch of 48; the first 17 rows and the first row alone — where one value near zero is the
    whole scale of an output (v_c of row 0 of "pl" is 0.022: the reference's own float32 error is 1.7e-6 of it) — against the float64 record
    of the same module for the outputs, and against the float32 gradient like the batch."""
    g = C.gold()
    sd = C.state(tag)
    out, g_ls = C.head_numpy(sd, g[f"{tag}/obs"][:n], g[f"{tag}/act"][:n], C.upstream(tag, n))
    rel = lambda a, b: float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / np.abs(np.asarray(b, np.float64)).max())
    for k in C.OUTS:
        assert rel(out[k], g[f"{tag}/ev{n}_64/{k}"]) <= 1e-12, k
        if n == 48:
            assert rel(out[k], g[f"{tag}/ev{n}/{k}"]) <= 1e-6, (k, rel(out[k], g[f"{tag}/ev{n}/{k}"]))
    if f"{tag}/g{n}/log_std" in g:
        ref = g[f"{tag}/g{n}/log_std"]
        assert ref.shape == sd["log_std"].shape and rel(g_ls, ref) <= 1e-6, rel(g_ls, ref)
        assert np.abs(g_ls - ref).max() <= 4 * float(g[f"{tag}/dev{n}/log_std"])
    if n == 48:
        assert rel(out["mean"], g[f"{tag}/fwd/mean"]) <= 1e-6
        noise = np.einsum("nh,nha->na", out["latent"], g[f"{tag}/E"].astype(np.float64))
        assert rel(out["mean"] + noise, g[f"{tag}/fwd/actions"]) <= 1e-6
        assert rel(out["mean"] + out["latent"] @ g[f"{tag}/E0"].astype(np.float64), g[f"{tag}/fwd0/actions"]) <= 1e-6


def test_the_fixture_is_trained_like_and_small():
    g = C.gold()
    assert os.path.getsize(C.GOLDEN) < 800 * 1024
    for tag, (O, A, arch) in C.SHAPES.items():
        ls = g[f"{tag}/w/log_std"]
        assert ls.shape == (arch["pi"][-1], A) and -1.5 <= ls.min() < -1.0 and 0.0 < ls.max() <= 0.5 and ls.std() > 0.3
        assert g[f"{tag}/E"].shape == (48, arch["pi"][-1], A) and g[f"{tag}/obs"].shape == (48, O)
    assert g["pl/train/perm"].shape == (96,) and sorted(g["pl/train/perm"]) == list(range(96))
    assert all(f"pl/train/w{k}/log_std" in g for k in (1, 2, 3)) and "pl/train/log/std" in g
