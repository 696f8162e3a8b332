"""CPU: the additive C ABI of the training-episode statistics (icrl_monitor_t, icrl_monitor_scan, the `_mon` rollout entry points) and
the host-side arithmetic on the ring of finished episodes — no kernel runs here."""
import ctypes
import os
from collections import deque

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from icrl_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L


def test_monitor_struct_layout():
    """icrl_monitor_t in include/icrl_hip.h: seven pointers (raw_rewards, ep_ret, ep_len, win_ret, win_len, win_state, ws) at offsets
    0, 8, ... 48 and one long long (ws_bytes) at 56 — 64 bytes, 8-byte aligned, no padding."""
    from icrl_amd.structs import MonitorT
    assert ctypes.sizeof(MonitorT) == 7 * 8 + 8 == 64
    assert ctypes.alignment(MonitorT) == 8
    names = [f[0] for f in MonitorT._fields_]
    assert names == ["raw_rewards", "ep_ret", "ep_len", "win_ret", "win_len", "win_state", "ws", "ws_bytes"]
    assert [getattr(MonitorT, n).offset for n in names] == [0, 8, 16, 24, 32, 40, 48, 56]
    src = open(os.path.join(ROOT, "include", "icrl_hip.h")).read()
    body = src[src.index("double* raw_rewards;"):src.index("} icrl_monitor_t;")]
    assert [ln.split(";")[0].split()[-1].lstrip("*") for ln in body.strip().splitlines()] == names


def test_new_entry_points_are_exported_and_the_abi_version_stays():
    L = _lib()
    lib = L.lib()
    for name in ("icrl_monitor_scan", "icrl_monitor_ws_bytes", "icrl_rollout_collect_ex_mon", "icrl_rollout_collect_batch_mon", "icrl_host_step_mon"):
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES, name
    # the descriptor sits directly before the stream; everything before it is the signature of the entry point without the suffix
    assert L.SIGNATURES["icrl_rollout_collect_ex_mon"] == L.SIGNATURES["icrl_rollout_collect_ex"][:-1] + [ctypes.c_void_p] * 2
    assert L.SIGNATURES["icrl_host_step_mon"] == L.SIGNATURES["icrl_host_step"][:-1] + [ctypes.c_void_p] * 2
    b, bm = L.SIGNATURES["icrl_rollout_collect_batch"], L.SIGNATURES["icrl_rollout_collect_batch_mon"]
    assert bm == b[:2] + [ctypes.c_void_p] + b[2:]
    assert L.SIGNATURES["icrl_monitor_scan"] == [ctypes.c_void_p] * 3 + [ctypes.c_int] * 3 + [ctypes.c_void_p]
    assert lib.icrl_abi_version() == 107
    # scratch of the scan: 4 ints + one count per row + one prefix per row and 64-column chunk
    assert lib.icrl_monitor_ws_bytes(64, 2048) == 4 * (4 + 64 + 64 * 32)
    assert lib.icrl_monitor_ws_bytes(2048, 64) == 4 * (4 + 2048 + 2048)
    assert lib.icrl_monitor_ws_bytes(5, 65) == 4 * (4 + 5 + 5 * 2)
    assert lib.icrl_monitor_ws_bytes(0, 4) == 0


def test_monitor_scan_refuses_bad_arguments_with_text():
    """host arithmetic before any launch: a NULL descriptor, rows outside 1..T, missing arrays, a workspace that is too small."""
    from icrl_amd.structs import MonitorT
    L = _lib()
    lib = L.lib()
    err = lib.icrl_monitor_scan(None, None, None, 8, 4, 8, None)
    assert err == 1
    with pytest.raises(ValueError, match="icrl_monitor_scan: NULL descriptor"):
        L.check(err, "icrl_monitor_scan")
    m = MonitorT(0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000, 1 << 20)      # (never dereferenced: every case below is refused)
    for rows in (0, -1, 9):
        err = lib.icrl_monitor_scan(ctypes.byref(m), 0x8000, 0x9000, 8, 4, rows, None)
        assert err == 1
        with pytest.raises(ValueError, match=rf"rows = {rows} of T = 8 \(1\.\.T\)"):
            L.check(err, "icrl_monitor_scan")
    err = lib.icrl_monitor_scan(ctypes.byref(m), None, 0x9000, 8, 4, 8, None)
    with pytest.raises(ValueError, match="dones plane and last_dones are all required"):
        L.check(err, "icrl_monitor_scan")
    small = MonitorT(0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000, 16)
    err = lib.icrl_monitor_scan(ctypes.byref(small), 0x8000, 0x9000, 8, 4, 8, None)
    with pytest.raises(ValueError, match=r"workspace of 80 B needed \(icrl_monitor_ws_bytes\), got 16"):
        L.check(err, "icrl_monitor_scan")
    # a descriptor without a plane is refused by the rollout entry points before they look at anything else
    empty = MonitorT()
    err = lib.icrl_rollout_collect_ex_mon(None, None, None, None, None, None, None, None, None, 0.99, 0.95, 0.99, 0.95, 1, ctypes.byref(empty), None)
    with pytest.raises(ValueError, match="icrl_rollout_collect_ex_mon: icrl_monitor_t.raw_rewards is NULL"):
        L.check(err, "icrl_rollout_collect_ex_mon")
    err = lib.icrl_host_step_mon(None, None, None, None, None, None, None, None, None, 0, ctypes.byref(empty), None)
    with pytest.raises(ValueError, match="icrl_host_step_mon: icrl_monitor_t.raw_rewards is NULL"):
        L.check(err, "icrl_host_step_mon")
    assert lib.icrl_last_error() == b""


@pytest.mark.parametrize("count", [0, 1, 99, 100, 101, 250])
def test_window_arithmetic_against_a_deque(count):
    """the host's reading of the ring (record i lies in slot i % 100, win_state[0] counts all records): order, rounding and means
    against the reference's deque(maxlen=100) of {"r": round(sum, 6), "l": len}."""
    from icrl_amd.ppo_lag import PPOLagrangian
    rng = np.random.RandomState(count)
    rets = rng.randn(count) * 37.0 + rng.randint(-3, 3, count) + 1e-7 * rng.randn(count)
    lens = rng.randint(1, 1001, count)
    ring_r, ring_l = np.full(100, np.nan), np.full(100, -7, np.int32)      # (slots never written must never be read)
    dq = deque(maxlen=100)
    for i in range(count):
        ring_r[i % 100], ring_l[i % 100] = rets[i], lens[i]
        dq.append({"r": round(float(rets[i]), 6), "l": int(lens[i])})
    idx = PPOLagrangian._window_order(count)
    assert len(idx) == min(count, 100) == len(dq)
    if count:
        assert idx[0] == (0 if count <= 100 else count % 100) and idx[-1] == (count - 1) % 100
    rs, ls = PPOLagrangian._window_records(count, ring_r, ring_l)
    assert rs == [e["r"] for e in dq] and ls == [e["l"] for e in dq]
    assert all(type(r) is float for r in rs) and all(type(v) is int for v in ls)
    if count:
        assert np.mean(rs) == np.mean([e["r"] for e in dq]) and np.mean(ls) == np.mean([e["l"] for e in dq])
        assert not np.isnan(np.mean(rs))


def test_cli_flag_parses_on_all_three_sub_commands():
    from icrl_amd import cpg, gail, icrl
    for mod in (icrl, cpg, gail):
        parser = mod.build_parser()
        assert parser.parse_args(["--episode_stats"]).episode_stats is True
        assert parser.parse_args([]).episode_stats is None      # None: the environment switch decides
