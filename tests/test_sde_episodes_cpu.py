"""CPU: the host side of a gSDE agent's sampling / evaluation episodes as one launch (icrl_sample_episodes_sde, icrl_sample_episodes_chain_sde;
utils.EpisodeRun, utils.sde_episodes_reason) — the exports, every refusal of the two entry points with its reason (the checks run on the host
before the first device call: `== 1` with a reason on descriptors whose pointers are the address 1 shows that none was made), the switch and
the host-env reason, the header's documentation."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 1      # a pointer no check may follow
PLAIN, CHAIN = "icrl_sample_episodes_sde", "icrl_sample_episodes_chain_sde"


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


def _descriptors(N=3, obs=18, act=6, max_steps=48, reward_form=0, training=0, pol=None, env=None):
    from icrl_amd import structs as S
    pk = dict(obs=obs, act=act, h1=64, h2=64, discrete=0, n_params=None, params=ONE, params_t=ONE, arch=None)
    pk.update(pol or {})
    if pk["n_params"] is None:
        pk["n_params"] = _n_diag(pk["obs"], pk["act"], pk["h1"]) + 63 * pk["act"]
    P = S.PolicyT(pk["obs"], pk["act"], pk["h1"], pk["h2"], pk["discrete"], pk["n_params"], pk["params"], pk["params_t"], pk["arch"])
    ek = dict(n_envs=N, obs_dim=obs, act_dim=act)
    ek.update(env or {})
    E = S.EnvT(ek["n_envs"], ek["obs_dim"], ek["act_dim"], max_steps, reward_form, 0, 0, 0, ONE, ONE, ONE, ONE, ONE)
    M = S.NormT(training, 1, 1, 1, 10.0, 10.0, 10.0, 0.99, 0.99, 1e-8, ONE, ONE, ONE, ONE, ONE, ONE, ONE)
    return dict(env=E, nm=M, pol=P)


def _plain(L, d, expl=ONE, lo=ONE, hi=ONE, eps=1, rows=48, row0=None, total=0, out=(ONE,) * 5, null=()):
    ref = lambda k: None if k in null else ctypes.byref(d[k])
    return L.icrl_sample_episodes_sde(ref("env"), ref("nm"), ref("pol"), expl, lo, hi, eps, rows, 1, row0, total, *out, None)


def _job(d, noise=None, base=ONE, eps=1, deterministic=0, fixed_len=1, out=(ONE,) * 5, null=()):
    from icrl_amd import structs as S
    ref = lambda k: None if k in null else ctypes.addressof(d[k])
    return S.ChainJobT(ref("env"), ref("nm"), ref("pol"), noise, base, eps, deterministic, fixed_len, 0, *out, None)


def _chain(L, jobs, expl, lo=ONE, hi=ONE, ws=ONE, ws_bytes=1 << 30, args=ONE, args_bytes=1 << 20, n_jobs=None):
    from icrl_amd import structs as S
    n = len(jobs) if n_jobs is None else n_jobs
    arr = (S.ChainJobT * max(len(jobs), 1))(*jobs)
    ex = None if expl is None else (ctypes.c_void_p * max(len(expl), 1))(*expl)
    return L.icrl_sample_episodes_chain_sde(n, arr if jobs else None, ex, lo, hi, 1, ws, ws_bytes, args, args_bytes, None)


# ---- the exports -----------------------------------------------------------------------------------------------------------------------------
def test_both_exports_are_declared_exported_and_bound_and_the_abi_version_stands():
    _lib_mod, L = _lib()
    src = open(os.path.join(ROOT, "include", "icrl_hip.h")).read()
    for name, n_args in ((PLAIN, 17), (CHAIN, 11)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), f"{name} is not declared in include/icrl_hip.h"
        assert hasattr(L, name), f"{name} is not exported"
        assert len(_lib_mod.SIGNATURES[name]) == n_args
    assert L.icrl_abi_version() == 107
    from icrl_amd import structs as S
    assert ctypes.sizeof(S.ChainJobT) == 5 * 8 + 4 * 4 + 6 * 8 and ctypes.sizeof(S.PolicyT) == 6 * 4 + 3 * 8      # no struct changed


def test_the_header_documents_both_entry_points():
    src = open(os.path.join(ROOT, "include", "icrl_hip.h")).read()
    at = src.index("int icrl_sample_episodes_sde(")
    comment = src[src.rindex("/*", 0, at):at]
    assert at < src.index("int icrl_sample_episodes_chain_sde(") < at + 1200, "the two exports stand together under one comment block"
    for word in ("icrl_sample_episodes_sde", "icrl_sample_episodes_chain_sde", "expl", "NULL: the mode", "HOST array", "icrl_policy_forward_sde",
                 "Refused", "refused:", "diagonal-layout", "DESIGN.md section 26", "log-prob"):
        assert word in comment, word


# ---- refusals common to both entry points: the (env, normaliser, policy) triple ---------------------------------------------------------------
TRIPLE = [
    (dict(pol=dict(n_params=_n_diag(18, 6))), r"n_params 16654, the gSDE \(log_std \[64, act_dim\]\) layout of \(18, 6, 64, 64\) has 17032 \(that is the diagonal layout's count: icrl_sample_episodes serves that policy\)"),
    (dict(pol=dict(n_params=17000)), r"n_params 17000, the gSDE .* has 17032$"),
    (dict(pol=dict(discrete=1)), r"a discrete policy has no gSDE head"),
    (dict(pol=dict(arch=True)), r"hidden widths \(64, 64\) with an `arch` descriptor; .* stored 64 x 64, no `arch`"),
    (dict(pol=dict(h1=32, h2=32)), r"hidden widths \(32, 32\); .* stored 64 x 64"),
    (dict(pol=dict(h1=128, h2=128)), r"hidden widths \(128, 128\)"),
    (dict(obs=129), r"obs_dim 129 \(1\.\.128\)"),
    (dict(obs=0), r"obs_dim 0 \(1\.\.128\)"),
    (dict(act=17), r"act_dim 17 \(1\.\.16\)"),
    (dict(env=dict(obs_dim=17)), r"env \(3 streams, obs_dim 17, act_dim 6\) vs policy \(obs_dim 18, act_dim 6\)"),
    (dict(env=dict(act_dim=5)), r"env \(3 streams, obs_dim 18, act_dim 5\) vs policy"),
    (dict(env=dict(n_envs=0)), r"env \(0 streams"),
    (dict(training=1), r"the normaliser must be frozen \(training = 1\)"),
    (dict(pol=dict(params=None)), r"NULL argument.* \(pol->params and pol->params_t are required\)"),
    (dict(pol=dict(params_t=None)), r"NULL argument.* \(pol->params and pol->params_t are required\)"),
]


def _with_arch(dkw):
    keep = np.ascontiguousarray([0, 2, 64, 64, 2, 64, 64, 2, 64, 64], dtype=np.int32)
    dkw = {k: (dict(v) if isinstance(v, dict) else v) for k, v in dkw.items()}
    if dkw.get("pol", {}).pop("arch", False):
        dkw["pol"]["arch"] = keep.ctypes.data
    return dkw, keep


@pytest.mark.parametrize("dkw,pattern", TRIPLE)
def test_the_plain_entry_point_refuses_before_a_device_call(dkw, pattern):
    _, L = _lib()
    dkw, _keep = _with_arch(dkw)
    _refused(L, _plain(L, _descriptors(**dkw)), "^icrl_sample_episodes_sde: ?.*" + pattern)


@pytest.mark.parametrize("dkw,pattern", TRIPLE)
def test_the_chained_entry_point_refuses_before_a_device_call(dkw, pattern):
    _, L = _lib()
    dkw, _keep = _with_arch(dkw)
    good, bad = _descriptors(), _descriptors(**dkw)
    _refused(L, _chain(L, [_job(good), _job(bad)], [ONE, ONE]), "^icrl_sample_episodes_chain_sde: ?.*job 1:.*" + pattern)


def test_null_pointers_are_refused():
    _, L = _lib()
    d = _descriptors()
    for who in ("env", "nm", "pol"):
        _refused(L, _plain(L, d, null=(who,)), r"^icrl_sample_episodes_sde: NULL argument \(env, nm and pol are required\)")
        _refused(L, _chain(L, [_job(d, null=(who,))], [ONE]), r"^icrl_sample_episodes_chain_sde: job 0: NULL argument \(env, nm and pol are required\)")
    for k in range(5):
        out = tuple(None if i == k else ONE for i in range(5))
        _refused(L, _plain(L, d, out=out), r"NULL argument \(orig_obs, obs, actions, ep_rewards and ep_lengths are required\)")
        _refused(L, _chain(L, [_job(d, out=out)], [ONE]), r"job 0: NULL argument \(orig_obs, obs, actions, ep_rewards and ep_lengths are required\)")
    _refused(L, _plain(L, d, lo=None), r"^icrl_sample_episodes_sde: NULL argument \(action_low and action_high: both or neither\)")
    _refused(L, _chain(L, [_job(d)], [ONE], hi=None), r"^icrl_sample_episodes_chain_sde: NULL argument \(action_low and action_high: both or neither\)")
    _refused(L, _chain(L, [_job(d)], None), r"^icrl_sample_episodes_chain_sde: NULL argument \(expl: one device pointer per job")
    _refused(L, _chain(L, [], [ONE], n_jobs=1), r"^icrl_sample_episodes_chain_sde: n_jobs = 1 \(1\.\.65535\)")
    _refused(L, _chain(L, [_job(d)], [ONE], n_jobs=0), r"n_jobs = 0 \(1\.\.65535\)")


def test_rows_that_do_not_fit_and_stream_row0_without_total_rows():
    _, L = _lib()
    d = _descriptors()
    _refused(L, _plain(L, d, eps=2, rows=95), r"^icrl_sample_episodes_sde: 2 episodes x 48 steps do not fit 95 rows per stream")
    _refused(L, _plain(L, d, eps=1, rows=47), r"1 episodes x 48 steps do not fit 47 rows per stream")
    _refused(L, _plain(L, d, row0=ONE, total=0), r"^icrl_sample_episodes_sde: stream_row0 given with total_rows = 0")


def test_a_job_with_noise_or_a_deterministic_flag_that_disagrees_with_its_matrix():
    _, L = _lib()
    d = _descriptors()
    _refused(L, _chain(L, [_job(d), _job(d, noise=ONE)], [ONE, ONE]), r"^icrl_sample_episodes_chain_sde: job 1 has a noise array; a gSDE policy's exploration is its matrix")
    _refused(L, _chain(L, [_job(d, deterministic=1)], [ONE]), r"job 0: deterministic = 1 with expl\[0\] set")
    _refused(L, _chain(L, [_job(d), _job(d, deterministic=0)], [ONE, None]), r"job 1: deterministic = 0 with expl\[1\] NULL")


def test_the_chained_entry_point_keeps_its_parents_refused_conditions_under_its_own_name():
    """the reason starts with "refused:": utils.launch_chain returns False and the caller settles the positions pass by pass"""
    _, L = _lib()
    d, point, ant = _descriptors(), _descriptors(obs=11, act=2, reward_form=4), _descriptors(obs=113, act=8)      # (kept alive: the jobs hold their addresses)
    head = r"^icrl_sample_episodes_chain_sde: refused: "
    _refused(L, _chain(L, [_job(point)], [ONE]), head + r"job 0 steps a Point env \(reward_form 4\)")
    _refused(L, _chain(L, [_job(d), _job(d, eps=2)], [ONE, ONE]), head + r"job 1 runs 2 episodes per stream \(1 only\)")
    _refused(L, _chain(L, [_job(d), _job(ant)], [ONE, ONE]), head + r"job 1 and job 0 take different kernels \(obs 113 / 18\)")
    # more streams than compute units: on a host without a device the count is 0; with one, ask for more streams than any device has
    many = _descriptors(N=100000, max_steps=1)
    _refused(L, _chain(L, [_job(many)], [ONE]), head + r"100000 streams on \d+ compute units")
    # a mode job passes the same checks (no matrix, deterministic set)
    _refused(L, _chain(L, [_job(many, deterministic=1)], [None]), head + r"100000 streams on \d+ compute units")


# ---- routing ----------------------------------------------------------------------------------------------------------------------------------
def test_sde_episodes_reason_names_the_switch_and_a_host_env(monkeypatch):
    from icrl_amd import utils
    from icrl_amd.vec_env import HostVecEnv
    agent = types.SimpleNamespace(policy=types.SimpleNamespace(use_sde=True))
    device_env = types.SimpleNamespace(unwrapped=object())
    host_env = types.SimpleNamespace(unwrapped=HostVecEnv.__new__(HostVecEnv))
    monkeypatch.delenv("ICRL_SDE_EPISODES_STEPPED", raising=False)
    assert utils.sde_episodes_reason(agent, device_env) is None
    assert utils.sde_episodes_reason(agent, host_env).startswith("a host env")
    for off in ("0", "", "false"):
        monkeypatch.setenv("ICRL_SDE_EPISODES_STEPPED", off)
        assert utils.sde_episodes_reason(agent, device_env) is None
    monkeypatch.setenv("ICRL_SDE_EPISODES_STEPPED", "1")
    assert utils.sde_episodes_reason(agent, device_env) == "ICRL_SDE_EPISODES_STEPPED=1"
    assert utils.sde_episodes_reason(agent, host_env) == "ICRL_SDE_EPISODES_STEPPED=1"


def test_the_agent_carries_the_two_attributes_and_seed_batches_keep_refusing_use_sde():
    from icrl_amd import exploration, ppo_lag, spaces
    env = types.SimpleNamespace(num_envs=4, observation_space=spaces.Box(-np.inf, np.inf, (18,), np.float64), action_space=spaces.Box(-1.0, 1.0, (6,), np.float32))
    a = ppo_lag.PPOLagrangian("TwoCriticsMlpPolicy", env, use_sde=True, n_steps=32, _init_setup_model=False)
    assert a.last_sde_episodes is None and a.last_sde_episodes_reason is None
    cfg = types.SimpleNamespace(use_sde=True, seeds=[0, 1], use_curiosity_driven_exploration=False, use_lambda_shaping=False, world_size=1)
    with pytest.raises(ValueError, match="seed batch"):
        exploration.refuse_sde(cfg, seed_batch=True)
