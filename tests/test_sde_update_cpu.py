"""The gSDE update as one persistent launch, without a device: the two exports (icrl_ppo_lag_train_sde, icrl_ppo_lag_train_sde_ws_bytes) are
declared and bound, every call outside the served set is refused on the host with hipErrorInvalidValue and its reason before any device call,
and the workspace size of a served call is at least ICRL_PPO_SYNC_BYTES."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("icrl_ppo_lag_train_sde", "icrl_ppo_lag_train_sde_ws_bytes")
ONE = ctypes.c_void_p(1)


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


def _buf(T=32, N=4, obs=18, act=6, planes=1):
    from icrl_amd import structs as S
    b = S.BufferT()
    b.T, b.N, b.obs_dim, b.act_store = T, N, obs, act
    for name, _ in S.BufferT._fields_[4:20]:
        setattr(b, name, planes)
    return b


def _hp(batch_size=64, n_epochs=2):
    from icrl_amd import structs as S
    return S.PpoHyperT(batch_size, n_epochs, 0, 0, 0.2, 0.0, 0.5, 0.5, 0.5, 0.0, -1.0, -1.0, 3e-4, 0.9, 0.999, 1e-5)


def _sync_bytes(n_epochs, n_mb, n_rows):      # ICRL_PPO_SYNC_BYTES (include/icrl_hip.h)
    return 768 + 48 * n_epochs * n_mb + 4 * n_epochs * n_rows + 256 + 2560 * 1024


def _train(L, pol, buf, hp, **null):
    """icrl_ppo_lag_train_sde on host-made descriptors whose pointers are the address 1: a call that got past the checks would fault, so a
    returned reason shows that the check ran first.  null: argument names passed as NULL."""
    a = dict(exp_avg=ONE, exp_avg_sq=ONE, adam_step=ONE, perms=ONE, nu=ONE, stats=ONE, sync_ws=ONE)
    a.update({k: None for k in null})
    return L.icrl_ppo_lag_train_sde(ctypes.byref(pol) if pol is not None else None, a["exp_avg"], a["exp_avg_sq"], a["adam_step"],
                                    ctypes.byref(buf) if buf is not None else None, a["perms"], a["nu"], ctypes.byref(hp) if hp is not None else None, a["stats"],
                                    a["sync_ws"], None)


def test_the_exports_are_declared_bound_and_the_abi_version_stands():
    _lib_mod, L = _lib()
    src = open(os.path.join(ROOT, "include", "icrl_hip.h")).read()
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", src), f"{name} is not declared in include/icrl_hip.h"
        assert hasattr(L, name) and name in _lib_mod.SIGNATURES
    assert _lib_mod.SIGNATURES["icrl_ppo_lag_train_sde"] == _lib_mod.SIGNATURES["icrl_ppo_lag_train"]
    assert _lib_mod.RESTYPES["icrl_ppo_lag_train_sde_ws_bytes"] is ctypes.c_size_t
    assert L.icrl_abi_version() == 107
    from icrl_amd import structs as S
    assert ctypes.sizeof(S.PolicyT) == 6 * 4 + 3 * 8 and ctypes.sizeof(S.PpoHyperT) == 16 * 4
    assert os.path.exists(os.path.join(ROOT, "icrl_amd", "csrc", "ppo_train_sde.hip"))


REFUSALS = [
    (dict(sde=False), {}, {}, r"n_params 16654, the gSDE \(log_std \[64, act_dim\]\) layout of \(18, 6, 64, 64\) has 17032"),
    (dict(discrete=1), {}, {}, r"discrete policy has no gSDE head"),
    (dict(arch=True), {}, {}, r"hidden widths \(64, 64\) with an `arch` descriptor.*64 x 64, no `arch`"),
    (dict(h1=32, h2=32), {}, {}, r"hidden widths \(32, 32\).*stored 64 x 64"),
    (dict(h1=128, h2=128), {}, {}, r"hidden widths \(128, 128\)"),
    (dict(obs=129), dict(obs=129), {}, r"obs_dim 129 \(1\.\.128\)"),
    (dict(obs=0), dict(obs=0), {}, r"obs_dim 0 \(1\.\.128\)"),
    (dict(act=17), dict(act=17), {}, r"act_dim 17 \(1\.\.16\)"),
    (dict(), {}, dict(batch_size=129), r"batch_size 129 \(2\.\.128"),
    (dict(), {}, dict(batch_size=256), r"batch_size 256 \(2\.\.128"),
    (dict(), {}, dict(batch_size=1), r"batch_size 1 \(2\.\.128"),
    (dict(), {}, dict(n_epochs=0), r"n_epochs 0 \(>= 1\)"),
    (dict(), dict(obs=17), {}, r"buffer obs_dim 17 vs policy 18"),
    (dict(), dict(T=0), {}, r"T = 0"),
    (dict(), dict(act=5), {}, r"act_store 5, a continuous policy of act_dim 6"),
]


@pytest.mark.parametrize("pkw,bkw,hkw,pattern", REFUSALS)
def test_calls_outside_the_served_set_are_refused_by_both_entry_points_before_a_device_call(pkw, bkw, hkw, pattern):
    _, L = _lib()
    keep = np.ascontiguousarray([0, 2, 64, 64, 2, 64, 64, 2, 64, 64], dtype=np.int32)
    pkw = dict(pkw)
    if pkw.pop("arch", False):
        pkw["arch"] = keep.ctypes.data
    pol, buf, hp = _pol(**pkw), _buf(**bkw), _hp(**hkw)
    assert L.icrl_ppo_lag_train_sde_ws_bytes(ctypes.byref(pol), ctypes.byref(buf), ctypes.byref(hp)) == 0
    _refused(L, 1, "icrl_ppo_lag_train_sde_ws_bytes: .*" + pattern)
    _refused(L, _train(L, pol, buf, hp), "icrl_ppo_lag_train_sde: .*" + pattern)


def test_null_pointers_are_refused_with_the_list_of_required_arguments():
    _, L = _lib()
    pol, buf, hp = _pol(), _buf(), _hp()
    for who in ("pol", "buf", "hp"):
        args = dict(pol=pol, buf=buf, hp=hp)
        args[who] = None
        _refused(L, _train(L, args["pol"], args["buf"], args["hp"]), r"NULL argument \(pol, buf and hp are required\)")
        wb = L.icrl_ppo_lag_train_sde_ws_bytes(*(None if args[k] is None else ctypes.byref(args[k]) for k in ("pol", "buf", "hp")))
        assert wb == 0
        _refused(L, 1, r"icrl_ppo_lag_train_sde_ws_bytes: NULL argument")
    for name in ("exp_avg", "exp_avg_sq", "adam_step", "perms", "nu", "stats", "sync_ws"):
        _refused(L, _train(L, pol, buf, hp, **{name: True}), r"NULL argument \(pol->params, pol->params_t, exp_avg.*sync_ws are required\)")
    _refused(L, _train(L, _pol(params=None), buf, hp), r"NULL argument \(pol->params")
    _refused(L, _train(L, _pol(params_t=None), buf, hp), r"NULL argument \(pol->params, pol->params_t")
    _refused(L, _train(L, pol, _buf(planes=None), hp), r"NULL buffer plane")


@pytest.mark.parametrize("obs,act,T,N,B,E", [(18, 6, 32, 4, 64, 3), (18, 6, 20, 5, 64, 2), (11, 3, 48, 2, 32, 1), (64, 16, 40, 5, 128, 2), (1, 1, 8, 4, 2, 1),
                                              (65, 8, 50, 3, 128, 1), (113, 8, 50, 3, 128, 1), (128, 16, 50, 3, 128, 2)])      # obs 65..128: the LDS images fit (161 920 of 163 840 bytes)
def test_a_served_shape_gets_at_least_the_sync_bytes_of_the_fused_update(obs, act, T, N, B, E):
    _, L = _lib()
    pol, buf, hp = _pol(obs=obs, act=act), _buf(T=T, N=N, obs=obs, act=act), _hp(batch_size=B, n_epochs=E)
    L.icrl_clear_error()
    need = L.icrl_ppo_lag_train_sde_ws_bytes(ctypes.byref(pol), ctypes.byref(buf), ctypes.byref(hp))
    assert L.icrl_last_error().decode() == ""
    assert need >= _sync_bytes(E, -(-T * N // B), T * N) > 0
    # the agent's update workspace (ppo_lag.py: _train_begin) is sized by the same macro: a served call never lacks room
    n_words = 96 + 6 * E * (-(-T * N // B)) + (E * T * N + 1) // 2 + 32 + 2560 * 1024 // 8
    assert need <= 8 * n_words
