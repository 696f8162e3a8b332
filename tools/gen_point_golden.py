"""Record tests/golden/g23_point_env.npz by stepping the REFERENCE's own Point envs (build machine only).

    python tools/gen_point_golden.py --reference <checkout of the reference>

custom_envs/custom_envs/envs/point.py is imported unmodified under a stand-in `gym.envs.mujoco.mujoco_env.MujocoEnv` defined here (the
Point envs never call the simulator to move: `set_state` is all they use).  The stand-in rests on two readings of
xmls/point_circle.xml that are not checked against MuJoCo: get_body_com("torso") is (x, y, 0), and qvel stays at init_qvel = 0.

Actions are float32 values handed to the env as a float64 ARRAY (exact conversions): the reference's pinned numpy 1.17 promotes a
float32 action to float64 in `qpos[2] += action[1]` and `math.cos(ori) * action[0]`; numpy 2 would keep float32 scalars in float32.
With float64 arrays both generations compute the same thing.  The 150-step limit is gym's TimeLimit (custom_envs/__init__.py:123-163),
and a finished env is reset as a VecEnv does.  Only arrays are written.  tests/helpers/point_env.PointVecEnv is asserted to reproduce
every recorded value (bit for bit on this host).
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

CLASSES = {"point_circle": "PointCircle", "point_circle_test": "PointCircleTest", "point_circle_test_back": "PointCircleTestBack",
           "point_null": "PointNullReward", "point_null_test": "PointNullRewardTest"}
N, S, MAX_STEPS = 3, 320, 150
NOISE_SEEDS = {"point_circle": 11, "point_circle_test": 12, "point_circle_test_back": 13, "point_null": 14, "point_null_test": 15}


class _Data:
    def __init__(self):
        self.qpos, self.qvel = np.zeros(3), np.zeros(3)


class _Model:
    nq = nv = 3


class MujocoEnv:
    """what point.py uses of gym's MujocoEnv, for a torso at the origin on two slide joints and a z hinge (xmls/point_circle.xml:23-29)."""

    def __init__(self, model_path, frame_skip):
        self.frame_skip, self.model, self.data = frame_skip, _Model(), _Data()
        self.init_qpos, self.init_qvel = np.zeros(3), np.zeros(3)
        self.np_random = np.random.RandomState(0)

    def set_state(self, qpos, qvel):
        assert qpos.shape == (3,) and qvel.shape == (3,)
        self.data.qpos, self.data.qvel = np.array(qpos, np.float64), np.array(qvel, np.float64)

    def get_body_com(self, name):
        assert name == "torso"
        return np.array([self.data.qpos[0], self.data.qpos[1], 0.0])

    def reset(self):
        return self.reset_model()


def load_reference(ref):
    mods = {n: types.ModuleType(n) for n in ("gym", "gym.envs", "gym.envs.mujoco", "gym.envs.mujoco.mujoco_env")}
    mods["gym.envs.mujoco.mujoco_env"].MujocoEnv = MujocoEnv
    mods["gym.envs.mujoco"].mujoco_env = mods["gym.envs.mujoco.mujoco_env"]
    mods["gym.envs"].mujoco = mods["gym.envs.mujoco"]
    mods["gym"].envs = mods["gym.envs"]
    saved = {n: sys.modules.get(n) for n in mods}
    sys.modules.update(mods)
    try:
        spec = importlib.util.spec_from_file_location("ref_point", os.path.join(ref, "custom_envs", "custom_envs", "envs", "point.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for n, m in saved.items():
            if m is None:
                sys.modules.pop(n)
            else:
                sys.modules[n] = m
    return mod


def sequences(kind):
    rng = np.random.RandomState(NOISE_SEEDS[kind])
    const = lambda a0, a1: np.broadcast_to(np.array([a0, a1], np.float32), (S, N, 2)).copy()
    return {"noise": np.clip(rng.randn(S, N, 2), -1.0, 1.0).astype(np.float32),     # clipped standard-normal noise (the env clips to 0.25 again)
            "back": const(-0.25, 0.0), "front": const(0.25, 0.0), "turn": const(0.25, 0.05)}


def run_reference(cls, acts):
    """-> obs [S, N, 9] (after the VecEnv's auto-reset), raw_obs (what env.step returned), rewards, dones."""
    import contextlib
    import io
    envs = [cls() for _ in range(N)]
    elapsed = [0] * N
    for e in envs:
        e.reset()
    obs, raw, rew, done = np.zeros((S, N, 9)), np.zeros((S, N, 9)), np.zeros((S, N)), np.zeros((S, N), bool)
    for t in range(S):
        for n, e in enumerate(envs):
            with contextlib.redirect_stdout(io.StringIO()):      # ("Terminating in True Environment")
                o, r, d, _ = e.step(acts[t, n].astype(np.float64))
            elapsed[n] += 1
            if elapsed[n] >= MAX_STEPS:      # gym 0.15 TimeLimit
                d = True
            raw[t, n], rew[t, n], done[t, n] = o, r, d
            if d:
                o = e.reset()
                elapsed[n] = 0
            obs[t, n] = o
    return obs, raw, rew, done


def main():
    from helpers.point_env import PointVecEnv
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("ICRL_REFERENCE"), required="ICRL_REFERENCE" not in os.environ)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "g23_point_env.npz"))
    args = ap.parse_args()
    ref = load_reference(args.reference)
    out = {}
    for kind, cname in CLASSES.items():
        for seq, acts in sequences(kind).items():
            obs, raw, rew, done = run_reference(getattr(ref, cname), acts)
            # no compared x may sit on a threshold (sequences "back" / "front" do, exactly, and are compared bit for bit)
            margin = np.abs(np.abs(raw[..., 0]) - 3.0).min()
            if seq in ("noise", "turn"):
                assert margin >= 1e-9, (kind, seq, margin)
            h = PointVecEnv(N, kind)
            h.reset()
            for t in range(S):
                o, r, d = h.step(acts[t])
                assert np.array_equal(o, obs[t]) and np.array_equal(r, rew[t]) and np.array_equal(d, done[t]), (kind, seq, t)
            print(f"{kind:24s} {seq:6s} episodes ended {int(done.sum()):3d}  min | |x| - 3 | {margin:.3e}  sum of rewards {rew.sum():+.6f}"
                  "  helper == reference bit for bit")
            for k, v in (("actions", acts), ("obs", obs), ("raw_obs", raw), ("rewards", rew), ("dones", done)):
                out[f"{kind}/{seq}/{k}"] = v
    np.savez_compressed(args.out, **out)
    print("wrote", args.out, os.path.getsize(args.out), "bytes; numpy", np.__version__)


if __name__ == "__main__":
    main()
