"""Worker loop of vec_env.SubprocVecEnv (ref: stable_baselines3/common/vec_env/subproc_vec_env.py:14-50).

Imports only numpy, cloudpickle and the standard library: a worker never loads torch or the HIP library, so it never opens the GPU.
"""
import sys

import cloudpickle
import numpy as np


def space_fields(space):
    """a gym-like space as plain fields (the parent rebuilds icrl_amd.spaces from them; gym need not exist in the parent)."""
    if hasattr(space, "n") and not hasattr(space, "low"):
        return dict(kind="discrete", n=int(space.n))
    return dict(kind="box", low=np.asarray(space.low), high=np.asarray(space.high), shape=tuple(int(x) for x in space.shape),
                dtype=np.dtype(space.dtype).str)


def max_episode_steps(env):
    """the time limit of a (wrapped) env: spec.max_episode_steps, else _max_episode_steps, else None."""
    spec = getattr(env, "spec", None)
    m = getattr(spec, "max_episode_steps", None) if spec is not None else None
    if m is None:
        m = getattr(env, "_max_episode_steps", None)
    return None if m is None else int(m)


def step_env(env, action):
    """one step with the vec-env auto-reset (subproc_vec_env.py:20-26, dummy_vec_env.py:43-58): on done the terminal observation
    goes to info['terminal_observation'] and the returned observation is the reset one."""
    obs, rew, done, info = env.step(action)
    info = dict(info) if info is not None else {}
    if done:
        info["terminal_observation"] = obs
        obs = env.reset()
    return obs, rew, done, info


def worker(remote, parent_remote, env_fn_bytes):
    parent_remote.close()
    env = cloudpickle.loads(env_fn_bytes)()
    try:
        while True:
            cmd, data = remote.recv()
            if cmd == "step":
                remote.send(step_env(env, data))
            elif cmd == "reset":
                remote.send(env.reset())
            elif cmd == "seed":
                remote.send(env.seed(data))
            elif cmd == "spaces":
                remote.send((space_fields(env.observation_space), space_fields(env.action_space), max_episode_steps(env)))
            elif cmd == "env_method":
                name, args, kwargs = data
                remote.send(getattr(env, name)(*args, **kwargs))
            elif cmd == "get_attr":
                remote.send(getattr(env, data))
            elif cmd == "set_attr":
                remote.send(setattr(env, data[0], data[1]))
            elif cmd == "modules":
                remote.send(sorted(m for m in data if m in sys.modules))
            elif cmd == "close":
                if hasattr(env, "close"):
                    env.close()
                remote.close()
                break
            else:
                raise NotImplementedError(f"`{cmd}` is not implemented in the worker")
    except KeyboardInterrupt:
        pass
