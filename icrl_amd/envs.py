"""Named host-side environments (the reference's `gym.register` + `import custom_envs`, custom_envs/__init__.py).

    envs.register("MyEnv-v0", "my_package.my_module:MyEnv", max_episode_steps=1000, kwargs=dict(...))
    envs.make("MyEnv-v0")

A registered id makes utils.make_train_env / make_eval_env build the usual wrapper chain over a host VecEnv (vec_env.SubprocVecEnv /
DummyVecEnv).  The ids of vec_env.ENV_IDS are the device-resident synthetic envs and cannot be registered.  `--env_module MODULE`
on the command line imports a module that calls register().

This module imports only the standard library: the workers of SubprocVecEnv unpickle env factories that point here and must not
load torch or the HIP library.
"""
import importlib

# reference gym ids (custom_envs/__init__.py:43-57,123-163,194-224,357-370) -> (kind, early termination, broken): the device-resident
# synthetic envs of vec_env.HipSynthVecEnv (vec_env.ENV_IDS is this dict)
ENV_IDS = {
    "HCWithPos-v0": ("hc", False, False), "HCWithPosTest-v0": ("hc", True, False),
    "AntWall-v0": ("ant", False, False), "AntWallTest-v0": ("ant", True, False),
    "AntWallBroken-v0": ("ant", False, True), "AntWallBrokenTest-v0": ("ant", True, True),
    "LGW-v0": ("lgw", False, False), "CLGW-v0": ("clgw", True, False),
    # custom_envs/__init__.py:123-163 — the Point envs, stepped exactly; the three Test ids end an episode at the wall
    "PointCircle-v0": ("point_circle", False, False), "PointCircleTest-v0": ("point_circle_test", True, False),
    "PointCircleTestBack-v0": ("point_circle_test_back", True, False),
    "PointNullReward-v0": ("point_null", False, False), "PointNullRewardTest-v0": ("point_null_test", True, False),
    "PointTrack-v0": ("point_track", False, False),
    # custom_envs/__init__.py — the dense Two Bridges envs, stepped exactly; none ends an episode before the 200-step limit
    "DD2B-v0": ("dd2b", False, False), "CDD2B-v0": ("cdd2b", False, False), "DDCDD2B-v0": ("ddcdd2b", False, False),
    "C2B-v0": ("c2b", False, False), "CC2B-v0": ("cc2b", False, False),
}

_REGISTRY = {}


class EnvSpec:
    def __init__(self, id, entry_point, max_episode_steps=None, kwargs=None):
        self.id, self.entry_point = id, entry_point
        self.max_episode_steps = None if max_episode_steps is None else int(max_episode_steps)
        self.kwargs = dict(kwargs or {})

    def _key(self):
        return (self.entry_point, self.max_episode_steps, sorted(self.kwargs.items(), key=lambda kv: kv[0]))

    def make(self):
        ep = self.entry_point
        if isinstance(ep, str):
            mod, _, attr = ep.partition(":")
            if not attr:
                raise ValueError(f"entry_point {ep!r}: expected 'module:attr'")
            ep = getattr(importlib.import_module(mod), attr)
        env = ep(**self.kwargs)
        if self.max_episode_steps is not None:
            env = TimeLimit(env, self.max_episode_steps)
        env.spec = self
        return env

    __call__ = make        # (an EnvSpec is the env factory a VecEnv takes; it pickles by value into SubprocVecEnv's workers)


class TimeLimit:
    """gym 0.15's TimeLimit: done after max_episode_steps steps; info['TimeLimit.truncated'] when the limit, not the env, ended it."""

    def __init__(self, env, max_episode_steps):
        self.env, self._max_episode_steps, self._elapsed_steps = env, int(max_episode_steps), None

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        return getattr(self.env, name)

    def step(self, action):
        assert self._elapsed_steps is not None, "Cannot call env.step() before calling reset()"
        obs, rew, done, info = self.env.step(action)
        self._elapsed_steps += 1
        if self._elapsed_steps >= self._max_episode_steps:
            info["TimeLimit.truncated"] = not done
            done = True
        return obs, rew, done, info

    def reset(self, **kwargs):
        self._elapsed_steps = 0
        return self.env.reset(**kwargs)

    def seed(self, seed=None):
        return self.env.seed(seed)

    @property
    def unwrapped(self):
        return getattr(self.env, "unwrapped", self.env)


def register(id, entry_point, max_episode_steps=None, kwargs=None):
    if id in ENV_IDS:
        raise ValueError(f"{id!r} is a device-resident env of this build (vec_env.ENV_IDS) and cannot be registered")
    if not (callable(entry_point) or (isinstance(entry_point, str) and ":" in entry_point)):
        raise ValueError(f"entry_point {entry_point!r}: a 'module:attr' string or a callable")
    spec = EnvSpec(id, entry_point, max_episode_steps, kwargs)
    old = _REGISTRY.get(id)
    if old is not None:
        if old._key() == spec._key():
            return old             # importing a registering module twice (e.g. under two names) is a no-op
        raise ValueError(f"{id!r} is already registered with another entry point / settings")
    _REGISTRY[id] = spec
    return spec


def spec(id):
    if id not in _REGISTRY:
        known = sorted(_REGISTRY) + sorted(ENV_IDS)
        raise KeyError(f"unknown env id {id!r}; known ids: {', '.join(known)} (a module that registers host envs is imported "
                       f"with --env_module)")
    return _REGISTRY[id]


def registered(id):
    return id in _REGISTRY


def make(id):
    return spec(id).make()


def import_modules(names):
    """--env_module: import every named module (each calls register())."""
    for name in names or ():
        importlib.import_module(name)
