"""Record tests/golden/g24_bridge_env.npz by stepping the REFERENCE's own Two Bridges and PointTrack envs (build machine only).

    python tools/gen_bridges_golden.py --reference <checkout of the reference>

custom_envs/custom_envs/envs/two_bridges.py, envs/utils.py and envs/point.py are imported unmodified, and so is icrl/true_constraint_net.py
for its `bridges()`, under stand-ins for `gym` (spaces.Box / spaces.Discrete as attribute bags, the MujocoEnv of tools/gen_point_golden.py)
and for `matplotlib` where that is missing (the envs only draw when asked to).  Each env gets a `spec` with max_episode_steps = 200 (150 for
PointTrack: custom_envs/__init__.py), gym 0.15's TimeLimit and a VecEnv's auto-reset around it.

Actions are float32 values handed to the env as float64 ARRAYS (the discrete envs: the index), see tools/gen_point_golden.py.  Only arrays
are written.  tests/helpers/bridge_env.BridgeVecEnv is asserted to reproduce every recorded value bit for bit on this host, the events the
sequences must contain are asserted, and so is the margin >= 1e-9 of every decision operand of the continuous and PointTrack sequences
from its threshold (the discrete envs are exact: their decisions need no margin).
"""
import argparse
import contextlib
import importlib.util
import io
import math
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

CLASSES = {"point_track": "PointTrack", "dd2b": "DenseDiscreteTwoBridges", "cdd2b": "ConstrainedDenseDiscreteTwoBridges",
           "ddcdd2b": "DDConstrainedDenseDiscreteTwoBridges", "c2b": "ContinuousTwoBridges", "cc2b": "ConstrainedContinuousTwoBridges"}
N = 3
STEPS = {"point_track": 320, "dd2b": 420, "cdd2b": 420, "ddcdd2b": 420, "c2b": 420, "cc2b": 420}
NOISE_SEEDS = {"point_track": 21, "dd2b": 22, "cdd2b": 23, "ddcdd2b": 24, "c2b": 25, "cc2b": 26}
MARGIN = 1e-9
UP, DOWN, RIGHT, LEFT = 2, 3, 0, 1


class _Spec:
    def __init__(self, max_episode_steps):
        self.max_episode_steps = max_episode_steps


class _Box:
    def __init__(self, low, high, shape=None, dtype=np.float32):
        self.low, self.high, self.dtype = np.asarray(low, dtype=dtype), np.asarray(high, dtype=dtype), dtype
        self.shape = self.low.shape if shape is None else shape


class _Discrete:
    def __init__(self, n):
        self.n = n


def load_reference(ref):
    """-> (two_bridges module, point module, true_constraint_net module) of the reference, imported under the stand-ins."""
    import gen_point_golden
    names = ("gym", "gym.spaces", "gym.envs", "gym.envs.mujoco", "gym.envs.mujoco.mujoco_env", "custom_envs", "custom_envs.envs",
             "custom_envs.envs.utils")
    mods = {n: types.ModuleType(n) for n in names}
    mods["gym.spaces"].Box, mods["gym.spaces"].Discrete = _Box, _Discrete
    mods["gym.envs.mujoco.mujoco_env"].MujocoEnv = gen_point_golden.MujocoEnv
    mods["gym.envs.mujoco"].mujoco_env = mods["gym.envs.mujoco.mujoco_env"]
    mods["gym.envs"].mujoco = mods["gym.envs.mujoco"]
    mods["gym"].envs, mods["gym"].spaces = mods["gym.envs"], mods["gym.spaces"]
    mods["custom_envs"].envs = mods["custom_envs.envs"]
    mods["custom_envs"].__path__ = mods["custom_envs.envs"].__path__ = []
    try:
        import matplotlib.pyplot      # noqa: F401
    except ImportError:
        for n in ("matplotlib", "matplotlib.pyplot", "matplotlib.patches"):
            mods[n] = types.ModuleType(n)
        mods["matplotlib"].pyplot, mods["matplotlib"].patches = mods["matplotlib.pyplot"], mods["matplotlib.patches"]
    saved = {n: sys.modules.get(n) for n in mods}
    sys.modules.update(mods)

    def load(name, *path):
        spec = importlib.util.spec_from_file_location(name, os.path.join(ref, *path))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    try:
        envs_dir = ("custom_envs", "custom_envs", "envs")
        utils = load("custom_envs.envs.utils", *envs_dir, "utils.py")
        sys.modules["custom_envs.envs.utils"] = utils
        mods["custom_envs.envs"].utils = utils
        out = load("ref_two_bridges", *envs_dir, "two_bridges.py"), load("ref_point", *envs_dir, "point.py"), load("ref_true_cost", "icrl", "true_constraint_net.py")
    finally:
        for n, m in saved.items():
            if m is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = m
    return out


# ---- action sequences ------------------------------------------------------------------------------------------------------------
def discrete_scripts(kind):
    """per env: the index sequence of an episode (the rest of the episode repeats its last index)."""
    ups = 0 if kind == "ddcdd2b" else 8                   # DDCDD2B starts at (3, 5): y = 5.7 after one step up
    lower = [UP] * (ups or 1) + [RIGHT] * 30 + [DOWN] * 10 + [LEFT] * 3          # the lower bridge (y = 5.6), the goal, the walls behind it
    upper = [UP] * (13 if kind == "ddcdd2b" else 21) + [RIGHT] * 28 + [DOWN] * 21 + [RIGHT] * 2 + [DOWN] * 2    # the upper bridge (y = 14.7 / 14.1), the goal, both outer walls
    water = [LEFT] + [RIGHT] * 7 + [UP] + [RIGHT] * 2 + [DOWN] * 3 + [UP] * 30 + [LEFT] * 2      # along y = 0 into the water's edge, then into it
    return [lower, upper, water]


def continuous_waypoints():
    """per env: waypoints of an episode, each with the number of steps spent heading for it."""
    lower = [((2.0, 5.5), 6), ((10.0, 5.45), 9), ((19.5, 0.5), 12), ((19.0, -1.5), 4), ((15.0, 3.0), 6)]
    upper = [((2.0, 14.5), 10), ((10.0, 14.45), 9), ((19.6, 0.6), 14), ((12.0, 10.0), 8)]
    water = [((6.0, 2.0), 6), ((3.5, 4.0), 6), ((4.5, 5.5), 3), ((-1.0, 3.0), 6), ((1.0, 8.0), 5)]
    return [lower, upper, water]


def scripted_continuous(kind, rng):
    """actions [S, N, 2] float32: every env heads for its waypoints (feedback over the helper env, which the recording is then compared
    with bit for bit), then noise; the script starts again with every episode."""
    from helpers.bridge_env import BridgeVecEnv
    S = STEPS[kind]
    env = BridgeVecEnv(N, kind)
    env.reset()
    plans = []
    for wps in continuous_waypoints():
        plans.append([wp for wp, k in wps for _ in range(k)])
    acts = np.zeros((S, N, 2), np.float32)
    t_ep = np.zeros(N, np.int64)
    for t in range(S):
        for n in range(N):
            if t_ep[n] < len(plans[n]):
                wx, wy = plans[n][t_ep[n]]
                x, y, ori = env.s[n]
                dist = math.hypot(wx - x, wy - y)
                turn = math.atan2(wy - y, wx - x) - ori
                turn = (turn + math.pi) % (2 * math.pi) - math.pi
                acts[t, n] = (min(max(dist, 0.05), 1.9), min(max(turn, -1.9), 1.9) + 0.003)      # always moving, never exactly along an axis
            else:
                acts[t, n] = np.clip(rng.randn(2) * 1.5, -3.0, 3.0)
        _, _, done = env.step(acts[t])
        t_ep = np.where(done, 0, t_ep + 1)
    return acts


def sequences(kind):
    from helpers import bridge_env
    rng = np.random.RandomState(NOISE_SEEDS[kind])
    S = STEPS[kind]
    if kind == "point_track":
        const = lambda a0, a1: np.broadcast_to(np.array([a0, a1], np.float32), (S, N, 2)).copy()
        return {"noise": np.clip(rng.randn(S, N, 2), -1.0, 1.0).astype(np.float32), "front": const(0.25, 0.0), "turn": const(0.25, 0.05),
                "ring": const(0.25, 0.024)}      # a circle of radius ~10.4 through the origin: in and out of the track
    if kind in bridge_env.DISCRETE:
        script = np.zeros((S, N, 1), np.float32)
        for n, seq in enumerate(discrete_scripts(kind)):
            ep = np.array((seq + [seq[-1]] * 200)[:200], np.float32)
            script[:, n, 0] = np.tile(ep, 3)[:S]
        return {"noise": rng.randint(0, 4, size=(S, N, 1)).astype(np.float32), "script": script}
    return {"noise": np.clip(rng.randn(S, N, 2) * 1.5, -3.0, 3.0).astype(np.float32), "script": scripted_continuous(kind, rng)}


# ---- the reference, stepped ------------------------------------------------------------------------------------------------------
def run_reference(cls, kind, acts):
    """-> obs [S, N, O] (after the VecEnv's auto-reset), raw_obs (what env.step returned), prev_obs (what the action was taken from),
    rewards, dones, and the envs."""
    from helpers.bridge_env import DIMS, DISCRETE
    O, _, max_steps = DIMS[kind]
    S = acts.shape[0]
    envs = [cls() for _ in range(N)]
    for e in envs:
        e.spec = _Spec(max_steps)
    last = [np.array(e.reset(), np.float64) for e in envs]
    elapsed = [0] * N
    obs, raw, prev, rew, done = np.zeros((S, N, O)), np.zeros((S, N, O)), np.zeros((S, N, O)), np.zeros((S, N)), np.zeros((S, N), bool)
    for t in range(S):
        for n, e in enumerate(envs):
            prev[t, n] = last[n]
            a = int(acts[t, n, 0]) if kind in DISCRETE else acts[t, n].astype(np.float64)
            with contextlib.redirect_stdout(io.StringIO()):
                o, r, d, _ = e.step(a)
            o = np.array(o, np.float64)          # (the continuous envs return their own qpos array: copy)
            elapsed[n] += 1
            if elapsed[n] >= max_steps:          # gym 0.15 TimeLimit
                d = True
            raw[t, n], rew[t, n], done[t, n] = o, r, d
            if d:
                o = np.array(e.reset(), np.float64)
                elapsed[n] = 0
            obs[t, n] = o
            last[n] = o
    return obs, raw, prev, rew, done, envs


REQUIRED = {   # events that the two sequences of a kind must contain between them (helpers/bridge_env.bridge_reward names them)
    "dd2b": {"wall", "water_end_point", "water_crossing", "lower_bridge", "upper_bridge", "goal", "right", "left"},
    "cdd2b": {"wall", "water_end_point", "water_crossing", "constraint", "upper_bridge", "goal", "right", "left"},
    "ddcdd2b": {"wall", "water_end_point", "constraint", "upper_bridge", "goal", "right", "left"},
    "c2b": {"wall", "water_end_point", "water_crossing", "lower_bridge", "upper_bridge", "goal", "right", "right_x20", "left"},
    "cc2b": {"wall", "water_end_point", "water_crossing", "constraint", "upper_bridge", "goal", "right", "right_x20", "left"},
}


def main():
    from helpers.bridge_env import DISCRETE, BridgeVecEnv
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("ICRL_REFERENCE"), required="ICRL_REFERENCE" not in os.environ)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "g24_bridge_env.npz"))
    args = ap.parse_args()
    ref_bridges, ref_point, ref_cost = load_reference(args.reference)
    out = {}
    for kind, cname in CLASSES.items():
        events = set()
        for seq, acts in sequences(kind).items():
            cls = getattr(ref_point if kind == "point_track" else ref_bridges, cname)
            obs, raw, prev, rew, done, envs = run_reference(cls, kind, acts)
            S = acts.shape[0]
            h = BridgeVecEnv(N, kind)
            exact = kind in DISCRETE or seq == "front"
            h.margin, h.events = (None if exact else []), events
            assert np.array_equal(h.reset(), prev[0]), (kind, "reset")
            for t in range(S):
                o, r, d = h.step(acts[t])
                assert np.array_equal(o, obs[t]) and np.array_equal(r, rew[t]) and np.array_equal(d, done[t]), (kind, seq, t, o, obs[t], r, rew[t])
            margin = min(h.margin) if h.margin else np.inf
            assert margin >= MARGIN, (kind, seq, margin)
            rec = {"actions": acts, "obs": obs, "raw_obs": raw, "rewards": rew, "dones": done, "margin": np.float64(margin)}
            if kind in ("cdd2b", "cc2b"):        # bridges() of the reference on (the raw observation the action was taken from, the action)
                a = acts.reshape(S * N, -1).astype(np.float64)
                cost = ref_cost.bridges(envs[0], prev.reshape(S * N, -1).copy(), a[:, 0].copy() if kind in DISCRETE else a.copy())
                rec["prev_obs"], rec["bridges_cost"] = prev, np.asarray(cost).reshape(S, N).astype(np.int64)
                assert 0 < rec["bridges_cost"].sum() < S * N, (kind, seq)
            print(f"{kind:12s} {seq:7s} episodes ended {int(done.sum()):2d}  margin {margin:.3e}  sum of rewards {rew.sum():+.6f}"
                  f"  distinct rewards {len(np.unique(rew)):4d}  helper == reference bit for bit")
            for k, v in rec.items():
                out[f"{kind}/{seq}/{k}"] = v
        if kind in REQUIRED:
            assert REQUIRED[kind] <= events, (kind, "missing events", REQUIRED[kind] - events)
            print(f"{kind:12s} events: {', '.join(sorted(events))}")
    np.savez_compressed(args.out, **out)
    print("wrote", args.out, os.path.getsize(args.out), "bytes; numpy", np.__version__)


if __name__ == "__main__":
    main()
