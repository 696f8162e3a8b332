"""CPU: the host side of the gSDE rollout as a launch of the library (icrl_rollout_collect_sde; policies.py noise_schedule, ppo_lag.py
sde_fused_rollout) — the up-front draws against the per-step loop's own sequence of reset_noise calls, every refusal of the entry point with its
reason (the checks run on the host before the first device call: `== 1` with a reason on descriptors whose pointers are the address 1 shows that
none was made), the flag's way from the three parsers into the agent and through save / load, the export, the byte-cap decision."""
import ast
import ctypes
import inspect
import json
import os
import re
import types
import zipfile

import numpy as np
import pytest
import torch

from helpers import sde_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 1      # a pointer no check may follow


def _lib():
    from icrl_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib, _lib.lib()


# ---- noise_schedule -----------------------------------------------------------------------------------------------------------------------
class _Counting:
    """a streams object: the loop's standard normals from torch's CPU generator, every call counted with its shape"""

    def __init__(self):
        self.shapes = []

    def sde_noise(self, shape):
        self.shapes.append(tuple(shape))
        return torch.randn(shape)


def _cpu_policy(tag, seed):
    pol = C.policy(tag, device="cpu", load=False)
    H, A = pol.sde_latent, pol.act_dim
    pol.log_std.copy_(torch.as_tensor(np.random.RandomState(seed).uniform(-1.5, 0.5, (H, A)).astype(np.float32)))
    return pol


def _loop_draws(pol, n_envs, T, ssf, streams=None):
    """the reset_noise calls of _collect_rollouts_stepped, in its order: [(step, E0, E)] with step -1 for the rollout's own draw"""
    out = []
    pol.reset_noise(n_envs, streams)
    out.append((-1, pol.sde_E0.clone(), pol.sde_E.clone()))
    for t in range(T):
        if ssf > 0 and t % ssf == 0:
            pol.reset_noise(n_envs, streams)
            out.append((t, pol.sde_E0.clone(), pol.sde_E.clone()))
    return out


@pytest.mark.parametrize("T,ssf", [(32, -1), (32, 8), (20, 8), (8, 8), (7, 8), (5, 1)])
@pytest.mark.parametrize("tag,n_envs", [("hc", 5), ("pl", 3), ("hc", 1)])
def test_noise_schedule_makes_the_draws_of_the_loop(tag, n_envs, T, ssf):
    pol = _cpu_policy(tag, 3)
    H, A = pol.sde_latent, pol.act_dim
    torch.manual_seed(41)
    loop = _loop_draws(pol, n_envs, T, ssf)
    after = torch.randn(4)      # where the loop leaves the generator
    pol.sde_E0 = pol.sde_E = None
    streams = _Counting()
    torch.manual_seed(41)
    sched = pol.noise_schedule(n_envs, T, ssf, streams)
    assert torch.equal(torch.randn(4), after), "the generator ends where the loop leaves it"
    # the number of generator calls: two per draw, 1 + ceil(T / ssf) draws (one with ssf < 0), each (H, A) then (n, H, A)
    n_draws = 1 + (-(-T // ssf) if ssf > 0 else 0)
    assert len(loop) == n_draws and streams.shapes == [(H, A), (n_envs, H, A)] * n_draws
    D = -(-T // ssf) if ssf > 0 else 1
    assert D == pol.noise_schedule_draws(T, ssf)
    assert tuple(sched.shape) == (D, n_envs, 64, A) and sched.dtype == torch.float32 and sched.is_contiguous()
    # which draw each step maps to: the matrices the loop holds at step t
    held = {}
    for step, E0, E in loop:
        for t in range(max(step, 0), T):
            held[t] = E0.unsqueeze(0) if n_envs == 1 else E
    for t in range(T):
        d = t // ssf if ssf > 0 else 0
        assert torch.equal(sched[d], held[t]), (t, d)
    # the policy's own state afterwards: the last draw, as after the loop
    assert torch.equal(pol.sde_E0, loop[-1][1]) and torch.equal(pol.sde_E, loop[-1][2])
    assert not sched[:, :, H:].any() and (H == 64 or tag == "pl")      # rows beyond the latent width are zero (-pl 32 48)
    assert sched[:, :, :H].abs().min() > 0
    # without a streams object the same matrices come from the same seed
    torch.manual_seed(41)
    assert torch.equal(pol.noise_schedule(n_envs, T, ssf), sched)


def test_one_env_gets_the_e0_of_each_draw():
    pol = _cpu_policy("hc", 5)
    torch.manual_seed(7)
    loop = _loop_draws(pol, 1, 20, 4)
    torch.manual_seed(7)
    sched = pol.noise_schedule(1, 20, 4)
    assert tuple(sched.shape) == (5, 1, 64, 6)
    for d in range(5):
        assert torch.equal(sched[d, 0], loop[1 + d][1]) and not torch.equal(sched[d, 0], loop[1 + d][2][0])


# ---- the entry point's refusals -------------------------------------------------------------------------------------------------------------
def _refused(L, err, pattern):
    assert err == 1, err
    reason = L.icrl_last_error().decode()
    L.icrl_clear_error()
    assert re.search(pattern, reason), reason
    from icrl_amd import _lib
    assert _lib.last_route(_lib.FAMILY_ROLLOUT)[0] == 0, "a refused call leaves route 0"


def _n_diag(obs, act, h=64):
    return act + 3 * (h * obs + h + h * h + h) + act * h + act + 2 * (h + 1)


def _descriptors(N=4, T=32, obs=18, act=6, pol=None, env=None, buf=None):
    from icrl_amd import structs as S
    pk = dict(obs=obs, act=act, h1=64, h2=64, discrete=0, n_params=None, params=ONE, params_t=ONE, arch=None)
    pk.update(pol or {})
    if pk["n_params"] is None:
        pk["n_params"] = _n_diag(pk["obs"], pk["act"], pk["h1"]) + 63 * pk["act"]
    P = S.PolicyT(pk["obs"], pk["act"], pk["h1"], pk["h2"], pk["discrete"], pk["n_params"], pk["params"], pk["params_t"], pk["arch"])
    ek = dict(n_envs=N, obs_dim=obs, act_dim=act)
    ek.update(env or {})
    E = S.EnvT(ek["n_envs"], ek["obs_dim"], ek["act_dim"], 1000, 0, 0, 0, 0, ONE, ONE, ONE, ONE, ONE)
    M = S.NormT(1, 1, 1, 1, 10.0, 10.0, 10.0, 0.99, 0.99, 1e-8, ONE, ONE, ONE, ONE, ONE, ONE, ONE)
    bk = dict(T=T, N=N, obs_dim=obs, act_store=act)
    bk.update(buf or {})
    B = S.BufferT()
    B.T, B.N, B.obs_dim, B.act_store = bk["T"], bk["N"], bk["obs_dim"], bk["act_store"]
    for name, _ in S.BufferT._fields_[4:20]:
        setattr(B, name, ONE)
    G = S.AgentT(ONE, ONE, ONE, ONE, ONE, ONE, ONE, ONE, ONE, ONE, 1 << 30)
    return dict(env=E, nm=M, pol=P, buf=B, ag=G)


def _call(L, d, cn=None, expl=ONE, n_draws=4, sample_freq=8, do_gae=1, lo=ONE, hi=ONE, null=()):
    ref = lambda k: None if k in null else ctypes.byref(d[k])
    return L.icrl_rollout_collect_sde(ref("env"), ref("nm"), ref("pol"), None if cn is None else ctypes.byref(cn), ref("buf"), ref("ag"), expl, n_draws, sample_freq,
                                      lo, hi, 0.99, 0.95, 0.99, 0.95, do_gae, None)


def test_null_pointers_are_refused():
    _, L = _lib()
    for who in ("env", "nm", "pol", "buf", "ag"):
        _refused(L, _call(L, _descriptors(), null=(who,)), r"icrl_rollout_collect_sde: NULL argument \(env, nm, pol, buf, ag and expl are required\)")
    _refused(L, _call(L, _descriptors(), expl=None), r"NULL argument \(env, nm, pol, buf, ag and expl")
    _refused(L, _call(L, _descriptors(pol=dict(params=None))), r"NULL argument \(pol->params and pol->params_t are required\)")
    _refused(L, _call(L, _descriptors(pol=dict(params_t=None))), r"NULL argument \(pol->params and pol->params_t are required\)")
    _refused(L, _call(L, _descriptors(), lo=None), r"NULL argument \(action_low and action_high: both or neither\)")


REFUSALS = [
    (dict(pol=dict(n_params=_n_diag(18, 6))), {}, r"n_params 16654, the gSDE \(log_std \[64, act_dim\]\) layout of \(18, 6, 64, 64\) has 17032 \(that is the diagonal layout's count"),
    (dict(pol=dict(n_params=17000)), {}, r"n_params 17000, the gSDE .* has 17032$"),
    (dict(pol=dict(discrete=1)), {}, r"a discrete policy has no gSDE head"),
    (dict(pol=dict(arch=True)), {}, r"hidden widths \(64, 64\) with an `arch` descriptor; .* stored 64 x 64, no `arch`"),
    (dict(pol=dict(h1=32, h2=32)), {}, r"hidden widths \(32, 32\); .* stored 64 x 64"),
    (dict(pol=dict(h1=128, h2=128)), {}, r"hidden widths \(128, 128\)"),
    (dict(obs=129), {}, r"obs_dim 129 \(1\.\.128\)"),
    (dict(obs=0), {}, r"obs_dim 0 \(1\.\.128\)"),
    (dict(act=17), {}, r"act_dim 17 \(1\.\.16\)"),
    (dict(env=dict(obs_dim=17)), {}, r"env \(4 envs, obs_dim 17, act_dim 6\) vs policy \(obs_dim 18, act_dim 6\) vs buffer \(T = 32, 4 envs, obs_dim 18, act_store 6\)"),
    (dict(env=dict(act_dim=5)), {}, r"env \(4 envs, obs_dim 18, act_dim 5\) vs policy"),
    (dict(buf=dict(N=5)), {}, r"vs buffer \(T = 32, 5 envs"),
    (dict(buf=dict(obs_dim=17)), {}, r"vs buffer \(T = 32, 4 envs, obs_dim 17"),
    (dict(buf=dict(act_store=1)), {}, r"act_store 1\)"),
    (dict(buf=dict(T=0)), {}, r"vs buffer \(T = 0"),
    (dict(N=4097), {}, r"4097 envs on one GPU, limit 4096"),
    ({}, dict(n_draws=3), r"n_draws 3, T = 32 steps at sample_freq 8 use 4"),
    (dict(T=33), dict(n_draws=4), r"n_draws 4, T = 33 steps at sample_freq 8 use 5"),
    ({}, dict(n_draws=0, sample_freq=-1), r"n_draws 0, T = 32 steps at sample_freq -1 use 1"),
    ({}, dict(n_draws=31, sample_freq=1), r"n_draws 31, T = 32 steps at sample_freq 1 use 32"),
    ({}, dict(sample_freq=0), r"sample_freq 0 \(> 0: a draw every sample_freq steps; < 0: one draw for the rollout\)"),
    ({}, dict(do_gae=4), r"do_gae 4 \(bit 0: .*bit 1: the per-step launches; no other bit is served\)"),
    ({}, dict(do_gae=33), r"do_gae 33"),
]


@pytest.mark.parametrize("dkw,ckw,pattern", REFUSALS)
def test_calls_outside_the_served_set_are_refused_before_a_device_call(dkw, ckw, pattern):
    _, L = _lib()
    keep = np.ascontiguousarray([0, 2, 64, 64, 2, 64, 64, 2, 64, 64], dtype=np.int32)
    dkw = {k: (dict(v) if isinstance(v, dict) else v) for k, v in dkw.items()}
    if dkw.get("pol", {}).pop("arch", False):
        dkw["pol"]["arch"] = keep.ctypes.data
    _refused(L, _call(L, _descriptors(**dkw), **ckw), "^icrl_rollout_collect_sde: .*" + pattern)


def test_costs_outside_the_served_set_are_refused():
    from icrl_amd import structs as S
    _, L = _lib()
    d = _descriptors()
    net = S.CostNetT(18, 6, 24, 1, 20, 0, 0, 0, 0, 24 * 20 + 20 + 20 + 1, 20.0, ONE, None, None, None, None, 1e-5, ONE, ONE)
    disc = S.CostDiscT(18, 6, 24, S.COST_DISC, ctypes.addressof(net))
    _refused(L, _call(L, d, cn=disc), r"a discriminator cost descriptor \(icrl_cost_disc_t\) is not served")
    for kw, text in ((dict(n_hidden=3, h1=20, h2=20), r"in_dim 24, 3 hidden layers of \(20, 20\)"), (dict(n_hidden=1, h1=128, h2=0), r"1 hidden layers of \(128, 0\)"),
                     (dict(n_hidden=2, h1=64, h2=65), r"2 hidden layers of \(64, 65\)"), (dict(n_hidden=1, h1=20, h2=0, in_dim=161), r"in_dim 161")):
        wide = S.CostNetT(18, 6, kw.get("in_dim", 24), kw["n_hidden"], kw["h1"], kw["h2"], 0, 0, 0, 1, 20.0, ONE, None, None, None, None, 1e-5, ONE, ONE)
        _refused(L, _call(L, d, cn=wide), r"a generic-shape constraint net \(.*" + text + r".*is not served")
    bad_fn = S.CostFnT(17, 6, 0, S.COST_FN, S.COST_WALL_BEHIND, 0, -3.0, 0.0)      # an analytic cost goes through its own check
    _refused(L, _call(L, d, cn=bad_fn), r"icrl_rollout_collect_sde: analytic cost built for obs_dim 17, the env has 18")


def test_the_export_is_declared_bound_and_the_abi_version_stands():
    _lib_mod, L = _lib()
    src = open(os.path.join(ROOT, "include", "icrl_hip.h")).read()
    assert re.search(r"\bint\s+icrl_rollout_collect_sde\s*\(", src), "icrl_rollout_collect_sde is not declared in include/icrl_hip.h"
    assert hasattr(L, "icrl_rollout_collect_sde") and len(_lib_mod.SIGNATURES["icrl_rollout_collect_sde"]) == 17
    assert re.search(r"#define\s+ICRL_PICK_SDE\s+64\b", src) and _lib_mod.PICK_SDE == 64
    assert L.icrl_abi_version() == 107
    from icrl_amd import structs as S
    assert ctypes.sizeof(S.PolicyT) == 6 * 4 + 3 * 8 and ctypes.sizeof(S.AgentT) == 10 * 8 + 8


# ---- the flag -----------------------------------------------------------------------------------------------------------------------------
def test_the_three_parsers_accept_the_flag_and_hand_it_to_the_agent():
    from icrl_amd import cpg, gail, icrl
    for mod in (cpg, icrl, gail):
        for flag in ("-sfr", "--sde_fused_rollout"):
            assert vars(mod.build_parser().parse_args(["-us", flag]))["sde_fused_rollout"] is True
        # opt-in, and not even in the namespace unless given: stored configs and the namespaces seed batches compare stay what they were
        assert "sde_fused_rollout" not in vars(mod.build_parser().parse_args(["-us"]))
        handed = False
        for node in ast.walk(ast.parse(inspect.getsource(mod))):
            if isinstance(node, ast.Call) and getattr(node.func, "id", None) in ("PPOLagrangian", "PPO"):
                handed |= any(kw.arg == "sde_fused_rollout" for kw in node.keywords)
        assert handed, mod.__name__


def _bare_agent(monkeypatch=None, n_envs=4, **kw):
    from icrl_amd import ppo_lag
    o, a = C.spaces_of("hc")
    env = types.SimpleNamespace(num_envs=n_envs, observation_space=o, action_space=a)
    return ppo_lag.PPOLagrangian("TwoCriticsMlpPolicy", env, use_sde=True, sde_sample_freq=8, n_steps=32, _init_setup_model=False, **kw)


def test_the_constructor_and_the_environment_switch(monkeypatch):
    from icrl_amd import gail
    monkeypatch.delenv("ICRL_SDE_ROLLOUT_FUSED", raising=False)
    assert _bare_agent().sde_fused_rollout is False and _bare_agent(sde_fused_rollout=True).sde_fused_rollout is True
    assert _bare_agent().sde_fused_max_bytes == 512 << 20 and _bare_agent().last_sde_rollout is None
    o, a = C.spaces_of("hc")
    env = types.SimpleNamespace(num_envs=2, observation_space=o, action_space=a)
    assert gail.PPO("TwoCriticsMlpPolicy", env, use_sde=True, sde_fused_rollout=True, _init_setup_model=False).sde_fused_rollout is True
    monkeypatch.setenv("ICRL_SDE_ROLLOUT_FUSED", "1")
    assert _bare_agent().sde_fused_rollout is True
    monkeypatch.setenv("ICRL_SDE_ROLLOUT_FUSED", "0")
    assert _bare_agent().sde_fused_rollout is False


def test_save_and_load_keep_the_flag_and_an_archive_without_it_loads_as_off(tmp_path, monkeypatch):
    from icrl_amd.dual_variable import DualVariable
    from icrl_amd.ppo_lag import PPOLagrangian
    monkeypatch.delenv("ICRL_SDE_ROLLOUT_FUSED", raising=False)
    monkeypatch.setattr(PPOLagrangian, "_setup_model", lambda self: None)      # (the networks live on the device: not what this test is about)
    monkeypatch.setattr(PPOLagrangian, "load_parameters", lambda self, path, dual=True: None)
    for on in (True, False):
        agent = _bare_agent(sde_fused_rollout=on)
        agent.policy, agent.dual, agent.lr_schedule = C.policy("hc", device="cpu", load=False), DualVariable(0.0, 0.1, 1, None), (lambda _p: 3e-4)
        path = agent.save(str(tmp_path / f"agent_{on}"))
        with zipfile.ZipFile(path) as z:
            data = json.loads(z.read("data"))
            members = {n: z.read(n) for n in z.namelist()}
        assert data["sde_fused_rollout"] is on and data["use_sde"] is True
        back = PPOLagrangian.load(path)
        assert back.sde_fused_rollout is on and back.use_sde is True and back.sde_sample_freq == 8
        del data["sde_fused_rollout"]      # an archive written before the flag existed, or by the reference
        old = str(tmp_path / f"old_{on}.zip")
        with zipfile.ZipFile(old, "w") as z:
            for n, blob in members.items():
                z.writestr(n, json.dumps(data) if n == "data" else blob)
        assert PPOLagrangian.load(old).sde_fused_rollout is False
        assert PPOLagrangian.load(old, sde_fused_rollout=True).sde_fused_rollout is True


# ---- which rollouts the launch takes --------------------------------------------------------------------------------------------------------
def test_the_reasons_for_the_loop_and_the_byte_cap(monkeypatch):
    monkeypatch.delenv("ICRL_SDE_ROLLOUT_FUSED", raising=False)
    rb = types.SimpleNamespace(buffer_size=32)
    served = (object(), None, object())      # a device chain without a cost wrapper
    off = _bare_agent()
    off._fused_chain = lambda: served
    assert off._sde_rollout_reason("cost", 32, rb) == "sde_fused_rollout is off"
    a = _bare_agent(sde_fused_rollout=True)
    a._fused_chain = lambda: served
    assert a._sde_rollout_reason("cost", 32, rb) is None
    assert a._sde_rollout_reason(lambda o, ac: 0, 32, rb) == "a callable cost_function"
    assert a._sde_rollout_reason("cost", 16, rb) == "a partial rollout"
    a._mon = {}
    assert a._sde_rollout_reason("cost", 32, rb).startswith("episode_stats")
    a._mon = None
    a._fused_chain = lambda: None
    assert a._sde_rollout_reason("cost", 32, rb).startswith("no fused env chain (host envs")
    disc = types.SimpleNamespace(discriminator_cost=lambda: object(), constraint_net=lambda: None)
    a._fused_chain = lambda: (object(), disc, object())
    assert a._sde_rollout_reason("cost", 32, rb).startswith("a DiscriminatorCost")
    a._fused_chain = lambda: served
    # the cap: [draws, n_envs, 64, A] float32
    assert a.sde_schedule_bytes(32) == 4 * 4 * 4 * 64 * 6
    a.sde_fused_max_bytes = a.sde_schedule_bytes(32)
    assert a._sde_rollout_reason("cost", 32, rb) is None
    a.sde_fused_max_bytes = 1
    assert a._sde_rollout_reason("cost", 32, rb) == f"the schedule of {4 * 4 * 4 * 64 * 6} bytes exceeds sde_fused_max_bytes = 1"
    # ssf 1 at 256 AntWall envs x 2048 steps: 1 GiB, above the default; ssf 8 there and ssf 1 at 64 envs fit
    from icrl_amd import spaces
    big = _bare_agent(sde_fused_rollout=True, n_envs=256)
    big.action_space = spaces.Box(-1.0, 1.0, (8,), np.float32)
    big._fused_chain = lambda: served
    big.sde_sample_freq = 1
    assert big.sde_schedule_bytes(2048) == 1 << 30
    assert big._sde_rollout_reason("cost", 2048, types.SimpleNamespace(buffer_size=2048)) == f"the schedule of {1 << 30} bytes exceeds sde_fused_max_bytes = {512 << 20}"
    big.sde_sample_freq = 8
    assert big._sde_rollout_reason("cost", 2048, types.SimpleNamespace(buffer_size=2048)) is None
    big.sde_sample_freq = -1
    assert big.sde_schedule_bytes(2048) == 4 * 256 * 64 * 8
