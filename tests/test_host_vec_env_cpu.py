"""CPU: host VecEnvs (vec_env.DummyVecEnv / SubprocVecEnv, numpy layer), the env registry (icrl_amd.envs) and the new flags."""
import ctypes
import os
import re

import numpy as np
import pytest

import tests.helpers.host_envs  # noqa: F401  (registers the Host* ids)
from icrl_amd import envs
from icrl_amd.vec_env import ENV_IDS, DummyVecEnv, SubprocVecEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Counter:
    """a do-nothing env whose episode ends after `length` steps; obs = [t, seed]; reward 0.1 + 1e-12 (survives float64 only)."""

    def __init__(self, length=3):
        self.length, self.t, self.s = length, 0, -1
        from icrl_amd import spaces
        self.observation_space = spaces.Box(-np.inf, np.inf, (2,), np.float64)
        self.action_space = spaces.Box(-1.0, 1.0, (1,), np.float32)

    def seed(self, s=None):
        self.s = s
        return [s]

    def reset(self):
        self.t = 0
        return np.array([0.0, self.s], np.float64)

    def step(self, a):
        self.t += 1
        return np.array([float(self.t), self.s], np.float64), 0.1 + 1e-12, self.t >= self.length, {"t": self.t}


def _dummy(n=3, length=3, offset=0):
    return DummyVecEnv([lambda: _Counter(length)] * n, device="cpu", env_index_offset=offset)


def test_auto_reset_keeps_the_terminal_observation():
    v = _dummy(2, 3)
    v.seed(0)
    v.reset_host()
    for t in range(1, 4):
        obs, rew, done, infos = v.step_host(np.zeros((2, 1), np.float32))
    assert done.all() and np.array_equal(obs[:, 0], [0.0, 0.0])                 # the returned observation is the reset one
    assert [i["terminal_observation"][0] for i in infos] == [3.0, 3.0] and infos[0]["t"] == 3


def test_seeds_are_seed_plus_offset_plus_index():
    v = _dummy(3, offset=10)
    assert v.seed(5) == [15, 16, 17]
    assert v.get_attr("s") == [15, 16, 17]


def test_attr_and_method_access_with_indices():
    v = _dummy(4)
    v.set_attr("length", 7, indices=[1, 3])
    assert v.get_attr("length") == [3, 7, 3, 7]
    assert v.get_attr("length", indices=2) == [3]
    assert v.env_method("seed", 9, indices=[0]) == [[9]]


def test_float64_observations_and_rewards_are_kept():
    v = _dummy(2)
    v.seed(0); v.reset_host()
    obs, rew, _, _ = v.step_host(np.zeros((2, 1), np.float32))
    assert obs.dtype == np.float64 and rew.dtype == np.float64
    assert rew[0] == 0.1 + 1e-12 and rew[0] != np.float64(np.float32(0.1 + 1e-12))


def test_time_limit_sets_done_and_the_truncation_key():
    envs.register("CounterLimited-v0", _Counter, max_episode_steps=2, kwargs=dict(length=100))
    env = envs.make("CounterLimited-v0")
    env.seed(0); env.reset()
    assert env.step(0)[2] is False
    _, _, done, info = env.step(0)
    assert done and info["TimeLimit.truncated"] is True
    v = DummyVecEnv([envs.spec("CounterLimited-v0")] * 2, device="cpu")
    assert v.max_steps == 2


def test_registry_errors_and_protected_ids():
    with pytest.raises(KeyError, match="HostHCWithPos-v0"):           # unknown ids list the known ones
        envs.make("NoSuchEnv-v0")
    for i in ENV_IDS:
        with pytest.raises(ValueError, match="device-resident"):
            envs.register(i, _Counter)
    with pytest.raises(ValueError, match="already registered"):
        envs.register("HostHCWithPos-v0", _Counter)
    import importlib
    import tests.helpers.host_envs as H
    importlib.reload(H)                                               # registering the same entries again is a no-op
    assert envs.spec("HostHCWithPos-v0").entry_point == "tests.helpers.host_envs:SynthHostEnv"


def test_host_env_matches_the_numpy_oracle():
    """the adapter is one env of the oracle's vectorised env (the device env's definition): same states across episode ends."""
    from oracle.synth_env import SynthVecEnv
    v = DummyVecEnv([envs.spec("HostHCWithPos-v0")] * 3, device="cpu")
    v.seed(4)
    ref = SynthVecEnv(3, "hc", 4)
    assert np.array_equal(v.reset_host(), ref.reset())
    v.env_method("set_t_ep", 990)
    ref.t_ep[:] = 990
    rng = np.random.RandomState(0)
    for _ in range(30):
        a = rng.uniform(-1, 1, (3, 6)).astype(np.float32)
        obs, rew, done, _ = v.step_host(a)
        o2, r2, d2 = ref.step(a)
        assert np.array_equal(obs, o2) and np.array_equal(rew, r2) and np.array_equal(done, d2)


def test_subproc_equals_dummy_across_episode_ends():
    fns = [envs.spec("HostHCWithPosTest-v0")] * 4
    d, s = DummyVecEnv(fns, device="cpu"), SubprocVecEnv(fns, device="cpu")
    try:
        assert d.seed(3) == s.seed(3)
        assert np.array_equal(d.reset_host(), s.reset_host())
        d.env_method("set_t_ep", 700); s.env_method("set_t_ep", 700)
        rng = np.random.RandomState(1)
        n_done = 0
        for _ in range(600):
            a = rng.uniform(-1, 1, (4, 6)).astype(np.float32)
            r1, r2 = d.step_host(a), s.step_host(a)
            for x, y in zip(r1[:3], r2[:3]):
                assert np.array_equal(x, y)
            for i1, i2 in zip(r1[3], r2[3]):
                assert i1.keys() == i2.keys()
                if "terminal_observation" in i1:
                    assert np.array_equal(i1["terminal_observation"], i2["terminal_observation"])
            n_done += int(r1[2].sum())
        assert n_done >= 4
        assert s.worker_modules(["torch", "numpy"]) == [["numpy"]] * 4      # the workers never load torch (nor the HIP library)
        assert s.get_attr("_max_episode_steps", indices=[0, 3]) == [1000, 1000] and s.max_steps == 1000
    finally:
        s.close()
    assert all(p.exitcode == 0 for p in s.processes) and not any(p.is_alive() for p in s.processes)


def test_new_flags_parse_on_every_parser():
    from icrl_amd import cpg, gail, icrl, run_policy
    for m in (icrl, cpg, gail):
        a = m.build_parser().parse_args(["--env_module", "a.b", "--env_module", "c", "--dummy_vec_env"])
        assert a.env_module == ["a.b", "c"] and a.dummy_vec_env is True
        assert m.build_parser().parse_args([]).dummy_vec_env is False
    assert run_policy.build_parser().parse_args(["--env_module", "x"]).env_module == ["x"]


def test_host_step_struct_matches_the_header():
    from icrl_amd import structs as S
    src = open(os.path.join(ROOT, "include", "icrl_hip.h")).read()
    body = re.search(r"typedef struct icrl_host_step_t \{(.*?)\} icrl_host_step_t;", src, re.S).group(1)
    fields = re.findall(r"^\s*(?:const\s+)?(?:long\s+)?(\w+)\s*\*?\s*(\w+);", body, re.M)
    assert [f for _, f in fields] == [f for f, _ in S.HostStepT._fields_]
    assert ctypes.sizeof(S.HostStepT) == 2 * 4 + 4 * 8 + 8
