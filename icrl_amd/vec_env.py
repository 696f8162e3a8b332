"""Vectorised-environment surface of the reference, device-resident.

Mirrors (same names / argument meaning):
  VecEnv, VecEnvWrapper        ref: stable_baselines3/common/vec_env/base_vec_env.py:48-342
  VecCostWrapper               ref: stable_baselines3/common/vec_env/vec_cost_wrapper.py:7-101
  VecNormalize(WithCost)       ref: stable_baselines3/common/vec_env/vec_normalize.py:9-278
  RunningMeanStd               ref: stable_baselines3/common/running_mean_std.py:6-39
  sync_envs_normalization      ref: stable_baselines3/common/vec_env/__init__.py:50-65
  HipSynthVecEnv               stands in for SubprocVecEnv + the MuJoCo envs (subproc_vec_env.py:53-177); spec SURVEY §8d

Observations / rewards / dones are torch tensors in HBM (float64 / float64 / uint8), not numpy arrays: the host only
enqueues kernels.  ``infos`` is a BatchedInfos object that still answers ``infos[i]['cost']`` like the reference's list of
dicts.  Arithmetic lives in libicrl_hip.so (icrl_synth_env_step, icrl_cost_mlp_forward, icrl_vecnorm_step).
"""
import copy
import pickle
from abc import ABC, abstractmethod

import numpy as np
import torch

from . import _lib, spaces
from ._subproc_worker import max_episode_steps, space_fields, step_env
from .envs import ENV_IDS as _ENV_IDS
from .structs import EnvT, NormT, p

# kind -> obs, act (width of the action vector handed to the env), max_episode_steps, reward form (icrl_env_t.reward_form)
KINDS = {"hc": (18, 6, 1000, 0), "ant": (113, 8, 500, 1),
         # LapGridWorld / ConstrainedLapGridWorld restated exactly (custom_envs/envs/lap_grid_world.py:29-240): Discrete(2)
         "lgw": (1, 1, 200, 2), "clgw": (1, 1, 200, 3),
         # the Point envs restated exactly (custom_envs/envs/point.py:22-276, custom_envs/__init__.py:123-163):
         # obs = qpos (x, y, ori), qvel (0, 0, 0), torso position (x, y, 0)
         "point_circle": (9, 2, 150, 4), "point_circle_test": (9, 2, 150, 5), "point_circle_test_back": (9, 2, 150, 6),
         "point_null": (9, 2, 150, 7), "point_null_test": (9, 2, 150, 8), "point_track": (9, 2, 150, 9),
         # the dense Two Bridges envs restated exactly (custom_envs/envs/two_bridges.py, custom_envs/__init__.py): the discrete
         # ones observe (x, y) and take Discrete(4), the continuous ones observe (x, y, ori) and take two actions in [-2, 2]
         "dd2b": (2, 1, 200, 10), "cdd2b": (2, 1, 200, 11), "ddcdd2b": (2, 1, 200, 12), "c2b": (3, 2, 200, 13), "cc2b": (3, 2, 200, 14)}
DISCRETE_ACTIONS = {"lgw": 2, "clgw": 2, "dd2b": 4, "cdd2b": 4, "ddcdd2b": 4}
POINT_KINDS = ("point_circle", "point_circle_test", "point_circle_test_back", "point_null", "point_null_test", "point_track")
POINT_CTRL = 0.25        # the actuators' ctrlrange (xmls/point_circle.xml); the env clips to it again (point.py:167)
BRIDGE_DISCRETE_KINDS = ("dd2b", "cdd2b", "ddcdd2b")
BRIDGE_CONTINUOUS_KINDS = ("c2b", "cc2b")
BRIDGE_SIZE, BRIDGE_CTRL = 20.0, 2.0      # two_bridges.py:16, :339
ENV_IDS = _ENV_IDS   # reference gym ids -> (kind, early termination, broken); defined in envs.py (no torch there)


def dynamics_matrix(kind):
    """B ~ N(0, 0.05^2) drawn once from RandomState(1234)."""
    o, a, _, _ = KINDS[kind]
    if kind in DISCRETE_ACTIONS or kind in POINT_KINDS or kind in BRIDGE_CONTINUOUS_KINDS:
        return np.zeros((o, a), np.float64)      # no linear dynamics: the grid world, the Point and the Two Bridges envs are stepped exactly
    return (np.random.RandomState(1234).randn(o, a) * 0.05).astype(np.float64)


class BatchedInfos:
    """infos[i][key] view over per-key device tensors (the reference returns a list of per-env dicts)."""

    def __init__(self, n):
        self.n, self.batch = n, {}

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return {k: v[i].item() for k, v in self.batch.items()}


class VecEnv(ABC):
    def __init__(self, num_envs, observation_space, action_space):
        self.num_envs, self.observation_space, self.action_space = num_envs, observation_space, action_space

    @abstractmethod
    def reset(self): ...

    @abstractmethod
    def step_async(self, actions): ...

    @abstractmethod
    def step_wait(self): ...

    def step(self, actions):
        self.step_async(actions)
        return self.step_wait()

    def close(self):
        pass

    def seed(self, seed=None):
        return [None] * self.num_envs

    def get_attr(self, attr_name, indices=None):
        return [getattr(self, attr_name)] * self.num_envs

    def set_attr(self, attr_name, value, indices=None):
        setattr(self, attr_name, value)

    def env_method(self, method_name, *a, indices=None, **k):
        return [getattr(self, method_name)(*a, **k)]

    @property
    def unwrapped(self):
        return self.venv.unwrapped if isinstance(self, VecEnvWrapper) else self


class VecEnvWrapper(VecEnv):
    def __init__(self, venv, observation_space=None, action_space=None):
        self.venv = venv
        super().__init__(venv.num_envs, observation_space or venv.observation_space, action_space or venv.action_space)

    def step_async(self, actions):
        self.venv.step_async(actions)

    def reset(self):
        return self.venv.reset()

    def seed(self, seed=None):
        return self.venv.seed(seed)

    def close(self):
        return self.venv.close()

    def __getattr__(self, name):
        if name.startswith("_") or name == "venv":
            raise AttributeError(name)
        return getattr(self.venv, name)


def _as_device_f32(x, device):
    if torch.is_tensor(x):
        return x.to(device=device, dtype=torch.float32).contiguous()
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32), device=device)


class HipSynthVecEnv(VecEnv):
    """N synthetic HCWithPos-/AntWall-shaped envs (or exact LapGridWorlds / Point / Two Bridges envs) stepped by one kernel launch; float64 state in HBM."""

    def __init__(self, n_envs, kind="hc", seed=0, env_index_offset=0, wall_terminate=False, broken=False, device="cuda"):
        self.kind, self.device = kind, torch.device(device)
        o, a, ms, rf = KINDS[kind]
        self.obs_dim, self.act_dim, self.max_steps, self.reward_form = o, a, ms, rf
        self.wall_terminate, self.broken = bool(wall_terminate), bool(broken)
        if kind in BRIDGE_DISCRETE_KINDS:
            # ref: two_bridges.py:70-72, :249 — Box((0, 0), (20, 20)) float32 observations, Discrete(4)
            super().__init__(n_envs, spaces.Box(0.0, BRIDGE_SIZE, (o,), np.float32), spaces.Discrete(DISCRETE_ACTIONS[kind]))
        elif kind in BRIDGE_CONTINUOUS_KINDS:
            # ref: two_bridges.py:336-342 — Box((0, 0, 0), (20, 20, inf)) float32 observations, Box(-2, 2, (2,)) float32 actions
            super().__init__(n_envs, spaces.Box(np.zeros(3, np.float32), np.array([BRIDGE_SIZE, BRIDGE_SIZE, np.inf], np.float32), (o,), np.float32),
                             spaces.Box(-BRIDGE_CTRL, BRIDGE_CTRL, (a,), np.float32))
        elif kind in DISCRETE_ACTIONS:
            # ref: lap_grid_world.py:50-53 — Box(0, 40) float32 observation space (the env itself emits 2 pos / 40 - 1)
            super().__init__(n_envs, spaces.Box(0.0, 40.0, (o,), np.float32), spaces.Discrete(DISCRETE_ACTIONS[kind]))
        elif kind in POINT_KINDS:
            super().__init__(n_envs, spaces.Box(-np.inf, np.inf, (o,), np.float64), spaces.Box(-POINT_CTRL, POINT_CTRL, (a,), np.float32))
        else:
            super().__init__(n_envs, spaces.Box(-np.inf, np.inf, (o,), np.float64), spaces.Box(-1.0, 1.0, (a,), np.float32))
        dev = self.device
        self.B = torch.as_tensor(dynamics_matrix(kind), device=dev)
        self.s = torch.zeros(n_envs, o, dtype=torch.float64, device=dev)
        self.t_ep = torch.zeros(n_envs, dtype=torch.int32, device=dev)
        self.step_count = torch.zeros(n_envs, dtype=torch.int32, device=dev)       # uint32 bits
        self.key = torch.zeros(n_envs, dtype=torch.int32, device=dev)
        self.raw_rew = torch.zeros(n_envs, dtype=torch.float64, device=dev)
        self.dones = torch.zeros(n_envs, dtype=torch.uint8, device=dev)
        self._actions = None
        self._index_offset = int(env_index_offset)
        self.seed(seed)

    @classmethod
    def make(cls, env_id, n_envs, seed=0, device="cuda", env_index_offset=0):
        kind, wall, broken = ENV_IDS[env_id]
        return cls(n_envs, kind, seed, env_index_offset, wall, broken, device)

    def seed(self, seed=None, env_index_offset=None):
        """env i gets stream key seed + (global index of env i) (ref: icrl/utils.py:256-263, subproc_vec_env.py:115-118).  The
        global index is i + the shard offset given at construction (rank * envs per rank on a multi-GPU run), so re-seeding
        through the wrapper chain (PPOLagrangian._setup_model -> env.seed(seed)) keeps every rank on its own shard."""
        seed = 0 if seed is None else int(seed)
        if env_index_offset is not None:
            self._index_offset = int(env_index_offset)
        keys = (np.arange(self.num_envs, dtype=np.int64) + seed + self._index_offset) & 0xFFFFFFFF
        self.key.copy_(torch.as_tensor(keys.astype(np.uint32).view(np.int32), device=self.device))
        self.step_count.zero_(); self.t_ep.zero_(); self.s.zero_()
        return [seed + self._index_offset + i for i in range(self.num_envs)]

    def struct(self):
        return EnvT(self.num_envs, self.obs_dim, self.act_dim, self.max_steps, self.reward_form, int(self.wall_terminate),
                    int(self.broken), 0, p(self.B), p(self.s), p(self.t_ep), p(self.step_count), p(self.key))

    def reset(self):
        e = self.struct()
        _lib.check(_lib.lib().icrl_synth_env_reset(_lib.byref(e), _lib.current_stream()), "icrl_synth_env_reset")
        return self.s.clone()

    def step_async(self, actions):
        self._actions = _as_device_f32(actions, self.device).reshape(self.num_envs, self.act_dim)

    def step_wait(self):
        e = self.struct()
        _lib.check(_lib.lib().icrl_synth_env_step(_lib.byref(e), p(self._actions), p(self.raw_rew), p(self.dones),
                                                  _lib.current_stream()), "icrl_synth_env_step")
        return self.s.clone(), self.raw_rew.clone(), self.dones.clone(), BatchedInfos(self.num_envs)


# ---- host-side envs (Python simulators): the reference's DummyVecEnv / SubprocVecEnv under the device-tensor VecEnv API ----------
def _to_space(fields):
    if fields["kind"] == "discrete":
        return spaces.Discrete(fields["n"])
    dt = np.dtype(fields["dtype"]).type
    return spaces.Box(np.asarray(fields["low"]), np.asarray(fields["high"]), tuple(fields["shape"]), dt)


class HostInfos(BatchedInfos):
    """infos of a host VecEnv: infos[i] is env i's own dict merged with the per-key device tensors of the wrappers (infos[i]['cost'])."""

    def __init__(self, env_infos):
        super().__init__(len(env_infos))
        self.env_infos = env_infos

    def __getitem__(self, i):
        d = dict(self.env_infos[i])
        d.update(super().__getitem__(i))
        return d


class HostVecEnv(VecEnv):
    """N duck-typed envs (reset(), step(a) -> (obs, rew, done, info), seed(s), observation_space, action_space: gym envs qualify)
    stepped on the host.  Two layers:

      numpy:  reset_host() -> obs f64 [N, O];  step_host(actions) -> obs f64 [N, O], rew f64 [N], done bool [N], list of info dicts
      device: reset / step_async / step_wait of VecEnv -> float64 obs, float64 rewards, uint8 dones on `device`, HostInfos

    so that VecCostWrapper, VecNormalize[WithCost], the per-step rollout and SteppedEpisodeRun run over it unchanged; PPOLagrangian
    runs its rollout over such a chain as one kernel launch per env step (ppo_lag._collect_rollouts_host), and sampling / evaluation
    episodes over one such env run the same way (utils.HostEpisodeRun).

    Numerics: what the reference's SubprocVecEnv returns, np.stack of what the envs produced — observations and rewards are kept in
    float64, never rounded through float32 / observation-space-dtype buffers as SB3's DummyVecEnv does (the reference never trains
    through that one).  DummyVecEnv and SubprocVecEnv are therefore interchangeable bit for bit.

    Env i is seeded seed + env_index_offset + i (HipSynthVecEnv.seed; the offset shards envs over ranks).  Device memory (the raw
    observation array `s`, the pinned staging of the host rollout path) is allocated on first device use: the numpy layer runs on a
    machine without a GPU."""

    def __init__(self, num_envs, obs_fields, act_fields, max_steps=None, env_index_offset=0, device="cuda"):
        obs_space, act_space = _to_space(obs_fields), _to_space(act_fields)
        if not isinstance(obs_space, spaces.Box) or len(obs_space.shape) != 1:
            raise NotImplementedError(f"host VecEnv: observation space {obs_space!r}; only 1-D Box observations are supported")
        super().__init__(num_envs, obs_space, act_space)
        self.device = torch.device(device)
        self.obs_dim = int(obs_space.shape[0])
        self.discrete = isinstance(act_space, spaces.Discrete)
        self.act_dim = 1 if self.discrete else int(act_space.shape[0])
        self.max_steps = None if max_steps is None else int(max_steps)
        self._index_offset = int(env_index_offset)
        self._actions = None
        self._s = None
        self._stage = None

    # -- subclass hooks: the N envs
    def _reset_envs(self):
        raise NotImplementedError

    def _step_envs(self, actions):
        raise NotImplementedError

    def _seed_envs(self, seeds):
        raise NotImplementedError

    # -- numpy layer
    def _env_actions(self, actions):
        a = actions.cpu().numpy() if torch.is_tensor(actions) else np.asarray(actions)
        if self.discrete:
            return a.reshape(self.num_envs).astype(np.int64)
        return a.reshape(self.num_envs, self.act_dim).copy()

    def reset_host(self):
        return np.stack(self._reset_envs()).astype(np.float64, copy=False).reshape(self.num_envs, self.obs_dim)

    def step_host(self, actions):
        res = self._step_envs(self._env_actions(actions))
        obs, rews, dones, infos = zip(*res)
        return (np.stack(obs).astype(np.float64, copy=False).reshape(self.num_envs, self.obs_dim), np.stack(rews).astype(np.float64, copy=False),
                np.stack(dones).astype(bool), list(infos))

    def seed(self, seed=None, env_index_offset=None):
        seed = 0 if seed is None else int(seed)
        if env_index_offset is not None:
            self._index_offset = int(env_index_offset)
        seeds = [seed + self._index_offset + i for i in range(self.num_envs)]
        self._seed_envs(seeds)
        return seeds

    # -- device layer
    @property
    def s(self):
        """device float64 [N, O]: the raw observations the envs returned last (HipSynthVecEnv.s)."""
        if self._s is None:
            self._s = torch.zeros(self.num_envs, self.obs_dim, dtype=torch.float64, device=self.device)
        return self._s

    def reset(self):
        self.s.copy_(torch.from_numpy(self.reset_host()))
        return self.s.clone()

    def step_async(self, actions):
        self._actions = actions

    def step_wait(self):
        obs, rew, done, infos = self.step_host(self._actions)
        N, O = self.num_envs, self.obs_dim
        blk = torch.from_numpy(np.concatenate([obs, rew[:, None], done[:, None].astype(np.float64)], axis=1)).to(self.device)
        self.s.copy_(blk[:, :O])
        return self.s.clone(), blk[:, O].contiguous(), blk[:, O + 1].to(torch.uint8), HostInfos(infos)

    def staging(self):
        """the transfer buffers of the host rollout path (icrl_host_step_t) and of the host episode loop (icrl_host_episode_t, which
        copies the observation part only), allocated on first use: a pinned block [obs f64 N x O | rew f64 N |
        done u8 N] copied to its device twin once per env step, and a pinned, device-visible float32 [N, act] the kernel writes the
        clipped actions (Discrete: the index) into — icrl_host_step maps its host address with hipHostGetDevicePointer, which serves
        torch's pinned allocations whether they come from hipHostMalloc or from host registration."""
        if self._stage is None:
            N, O = self.num_envs, self.obs_dim
            nbytes = (8 * N * O + 8 * N + N + 7) // 8 * 8
            pin = torch.zeros(nbytes, dtype=torch.uint8).pin_memory()
            dev = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
            npin = pin.numpy()
            self._stage = dict(pin=pin, dev=dev, nbytes=nbytes,
                               obs=npin[:8 * N * O].view(np.float64).reshape(N, O), rew=npin[8 * N * O:8 * N * O + 8 * N].view(np.float64),
                               done=npin[8 * N * O + 8 * N:8 * N * O + 9 * N],
                               act=torch.zeros(N, self.act_dim, dtype=torch.float32).pin_memory())
        return self._stage


class DummyVecEnv(HostVecEnv):
    """ref: stable_baselines3/common/vec_env/dummy_vec_env.py:13-118 — the envs stepped one after the other in this process (see
    HostVecEnv for the numerics: float64 kept, no float32 buffers)."""

    def __init__(self, env_fns, device="cuda", env_index_offset=0):
        self.envs = [fn() for fn in env_fns]
        e0 = self.envs[0]
        super().__init__(len(self.envs), space_fields(e0.observation_space), space_fields(e0.action_space), max_episode_steps(e0),
                         env_index_offset, device)

    def _reset_envs(self):
        return [env.reset() for env in self.envs]

    def _step_envs(self, actions):
        return [step_env(env, actions[i]) for i, env in enumerate(self.envs)]

    def _seed_envs(self, seeds):
        for env, s in zip(self.envs, seeds):
            env.seed(s)

    def _targets(self, indices):
        if indices is None:
            indices = range(self.num_envs)
        elif isinstance(indices, int):
            indices = [indices]
        return [self.envs[i] for i in indices]

    def get_attr(self, attr_name, indices=None):
        return [getattr(env, attr_name) for env in self._targets(indices)]

    def set_attr(self, attr_name, value, indices=None):
        for env in self._targets(indices):
            setattr(env, attr_name, value)

    def env_method(self, method_name, *method_args, indices=None, **method_kwargs):
        return [getattr(env, method_name)(*method_args, **method_kwargs) for env in self._targets(indices)]

    def close(self):
        for env in self.envs:
            if hasattr(env, "close"):
                env.close()


class SubprocVecEnv(HostVecEnv):
    """ref: stable_baselines3/common/vec_env/subproc_vec_env.py:14-177 — one worker process per env (icrl_amd/_subproc_worker.py:
    numpy + cloudpickle only, no torch, no GPU).  Env factories travel with cloudpickle.  start_method: forkserver where available,
    else spawn; fork is refused once this process has initialised the GPU."""

    def __init__(self, env_fns, start_method=None, device="cuda", env_index_offset=0):
        import multiprocessing as mp
        import cloudpickle
        from . import _subproc_worker
        if start_method is None:
            start_method = "forkserver" if "forkserver" in mp.get_all_start_methods() else "spawn"
        if start_method == "fork" and torch.cuda.is_initialized():
            raise ValueError("SubprocVecEnv: start_method 'fork' after the GPU was initialised in this process; use forkserver or spawn")
        ctx = mp.get_context(start_method)
        self.waiting, self.closed = False, False
        n = len(env_fns)
        self.remotes, work_remotes = zip(*[ctx.Pipe() for _ in range(n)])
        self.processes = []
        for work_remote, remote, fn in zip(work_remotes, self.remotes, env_fns):
            proc = ctx.Process(target=_subproc_worker.worker, args=(work_remote, remote, cloudpickle.dumps(fn)), daemon=True)
            proc.start()
            self.processes.append(proc)
            work_remote.close()
        self.remotes[0].send(("spaces", None))
        obs_fields, act_fields, max_steps = self.remotes[0].recv()
        super().__init__(n, obs_fields, act_fields, max_steps, env_index_offset, device)

    def _reset_envs(self):
        for remote in self.remotes:
            remote.send(("reset", None))
        return [remote.recv() for remote in self.remotes]

    def _step_envs(self, actions):
        for remote, a in zip(self.remotes, actions):
            remote.send(("step", a))
        self.waiting = True
        res = [remote.recv() for remote in self.remotes]
        self.waiting = False
        return res

    def _seed_envs(self, seeds):
        for remote, s in zip(self.remotes, seeds):
            remote.send(("seed", s))
        for remote in self.remotes:
            remote.recv()

    def _targets(self, indices):
        if indices is None:
            indices = range(self.num_envs)
        elif isinstance(indices, int):
            indices = [indices]
        return [self.remotes[i] for i in indices]

    def get_attr(self, attr_name, indices=None):
        targets = self._targets(indices)
        for remote in targets:
            remote.send(("get_attr", attr_name))
        return [remote.recv() for remote in targets]

    def set_attr(self, attr_name, value, indices=None):
        targets = self._targets(indices)
        for remote in targets:
            remote.send(("set_attr", (attr_name, value)))
        for remote in targets:
            remote.recv()

    def env_method(self, method_name, *method_args, indices=None, **method_kwargs):
        targets = self._targets(indices)
        for remote in targets:
            remote.send(("env_method", (method_name, method_args, method_kwargs)))
        return [remote.recv() for remote in targets]

    def worker_modules(self, names):
        """which of `names` are imported in each worker (the tests check that no worker loads torch)."""
        for remote in self.remotes:
            remote.send(("modules", list(names)))
        return [remote.recv() for remote in self.remotes]

    def close(self):
        if self.closed:
            return
        if self.waiting:
            for remote in self.remotes:
                remote.recv()
        for remote in self.remotes:
            remote.send(("close", None))
        for proc in self.processes:
            proc.join()
        self.closed = True

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class VecCostWrapper(VecEnvWrapper):
    """cost = cost_function(previous raw obs, current action) written to infos['cost'] (ref: vec_cost_wrapper.py:51-77)."""

    def __init__(self, venv):
        super().__init__(venv)
        self.cost_function = None
        self.previous_obs = None
        self.actions = None

    def set_cost_function(self, cost_function):
        self.cost_function = cost_function

    def constraint_net(self):
        """the device ConstraintNet behind cost_function, if that is what it is (enables the fused rollout)."""
        owner = getattr(self.cost_function, "__self__", None)
        from .constraint_net import ConstraintNet
        return owner if isinstance(owner, ConstraintNet) and getattr(self.cost_function, "__name__", "") == "cost_function" else None

    def analytic_cost(self):
        """the AnalyticCost behind cost_function, if that is what it is (true_constraint_net.py: evaluated inside the fused rollout like a
        ConstraintNet, by closed form)."""
        from .true_constraint_net import AnalyticCost
        return self.cost_function if isinstance(self.cost_function, AnalyticCost) else None

    def discriminator_cost(self):
        """the DiscriminatorCost behind cost_function, if that is what it is (gail_utils.py: cpg --load_gail; evaluated inside the fused
        rollout by the kernels that read the net as D)."""
        from .gail_utils import DiscriminatorCost
        return self.cost_function if isinstance(self.cost_function, DiscriminatorCost) else None

    def region_cost(self):
        """the RegionCost behind cost_function, if that is what it is (true_constraint_net.py: --cost_spec; evaluated inside the fused
        rollout by the kernels whose cost wave walks the clause table)."""
        from .true_constraint_net import RegionCost
        return self.cost_function if isinstance(self.cost_function, RegionCost) else None

    def cost_struct(self):
        """the descriptor the rollout entry points take for this wrapper's cost (icrl_costnet_t, icrl_cost_fn_t, icrl_cost_disc_t or
        icrl_cost_region_t), or None."""
        cn = self.constraint_net()
        if cn is not None:
            return cn.struct()
        rc = self.region_cost()
        if rc is not None:
            return rc.struct(getattr(self.venv, "device", None))
        dc = self.discriminator_cost()
        if dc is not None:
            return dc.struct()
        ac = self.analytic_cost()
        if ac is None:
            return None
        disc = isinstance(self.action_space, spaces.Discrete)
        return ac.struct(self.observation_space.shape[0], self.action_space.n if disc else self.action_space.shape[0])

    def reset(self):
        obs = self.venv.reset()
        self.previous_obs = obs
        return obs

    def step_async(self, actions):
        self.actions = _as_device_f32(actions, self.venv.device) if hasattr(self.venv, "device") else actions
        self.venv.step_async(actions)

    def step_wait(self):
        obs, rews, news, infos = self.venv.step_wait()
        cn = self.constraint_net()
        if cn is not None:
            cost = cn.cost_function_device(self.previous_obs, self.actions)
        elif (self.analytic_cost() is not None or self.discriminator_cost() is not None or self.region_cost() is not None) and torch.is_tensor(self.previous_obs) and torch.is_tensor(self.actions):
            cost = self.cost_function(self.previous_obs, self.actions)      # icrl_cost_fn_rows / icrl_disc_reward / icrl_cost_region_rows on the device tensors: no host copies
        else:  # arbitrary Python callable: numpy in / numpy out, as in the reference
            po = self.previous_obs.cpu().numpy() if torch.is_tensor(self.previous_obs) else self.previous_obs
            ac = self.actions.cpu().numpy() if torch.is_tensor(self.actions) else self.actions
            cost = torch.as_tensor(np.asarray(self.cost_function(po.copy(), ac.copy()), dtype=np.float32), device=obs.device)
        infos.batch["cost"] = cost
        self.previous_obs = obs.clone()
        return obs, rews, news, infos


class RunningMeanStd:
    """mean / var / count triple living in HBM (float64).  ``.mean`` / ``.var`` / ``.count`` read back numpy values like
    the reference's attributes (ref: running_mean_std.py:6-18)."""

    def __init__(self, epsilon=1e-4, shape=(), device="cuda"):
        self.shape = tuple(shape)
        n = int(np.prod(shape)) if shape else 1
        self.d_mean = torch.zeros(n, dtype=torch.float64, device=device)
        self.d_var = torch.ones(n, dtype=torch.float64, device=device)
        self.d_count = torch.full((1,), float(epsilon), dtype=torch.float64, device=device)

    @property
    def mean(self):
        return self.d_mean.cpu().numpy().reshape(self.shape).copy() if self.shape else float(self.d_mean.item())

    @property
    def var(self):
        return self.d_var.cpu().numpy().reshape(self.shape).copy() if self.shape else float(self.d_var.item())

    @property
    def count(self):
        return float(self.d_count.item())

    def assign(self, mean, var, count):
        self.d_mean.copy_(torch.as_tensor(np.asarray(mean, np.float64).reshape(-1)))
        self.d_var.copy_(torch.as_tensor(np.asarray(var, np.float64).reshape(-1)))
        self.d_count.fill_(float(count))

    def clone(self):
        c = RunningMeanStd(shape=self.shape, device=self.d_mean.device)
        c.d_mean.copy_(self.d_mean); c.d_var.copy_(self.d_var); c.d_count.copy_(self.d_count)
        return c

    def __deepcopy__(self, memo):
        return self.clone()


class _ScalarRms(RunningMeanStd):
    """ret_rms / cost_rms packed as [mean, var, count] in one device array (the layout icrl_norm_t wants)."""

    def __init__(self, epsilon=1e-4, device="cuda"):
        self.shape = ()
        self.d_stats = torch.tensor([0.0, 1.0, float(epsilon)], dtype=torch.float64, device=device)

    mean = property(lambda self: float(self.d_stats[0].item()))
    var = property(lambda self: float(self.d_stats[1].item()))
    count = property(lambda self: float(self.d_stats[2].item()))

    def assign(self, mean, var, count):
        self.d_stats.copy_(torch.tensor([float(mean), float(var), float(count)], dtype=torch.float64))

    def clone(self):
        c = _ScalarRms(device=self.d_stats.device)
        c.d_stats.copy_(self.d_stats)
        return c


class VecNormalize(VecEnvWrapper):
    """ref: vec_normalize.py:9-181 (obs + reward).  See VecNormalizeWithCost for the cost channel."""

    def __init__(self, venv, training=True, norm_obs=True, norm_reward=True, clip_obs=10.0, clip_reward=10.0, gamma=0.99,
                 epsilon=1e-8):
        super().__init__(venv)
        dev = self.device = getattr(venv.unwrapped, "device", torch.device("cuda"))
        o = self.observation_space.shape[0]
        self.obs_rms = RunningMeanStd(shape=(o,), device=dev)
        self.ret_rms = _ScalarRms(device=dev)
        self.cost_rms = _ScalarRms(device=dev)
        self.clip_obs, self.clip_reward, self.clip_cost = clip_obs, clip_reward, 10.0
        self.ret = torch.zeros(self.num_envs, dtype=torch.float64, device=dev)
        self.cost_ret = torch.zeros(self.num_envs, dtype=torch.float64, device=dev)
        self.gamma, self.cost_gamma, self.epsilon = gamma, 0.99, epsilon
        self.training, self.norm_obs, self.norm_reward, self.norm_cost = training, norm_obs, norm_reward, False
        self.old_obs = self.old_reward = self.old_cost = None
        self._obs_out = torch.zeros(self.num_envs, o, dtype=torch.float64, device=dev)
        self._rew_out = torch.zeros(self.num_envs, dtype=torch.float64, device=dev)
        self._cost_out = torch.zeros(self.num_envs, dtype=torch.float64, device=dev)

    def struct(self):
        return NormT(int(self.training), int(self.norm_obs), int(self.norm_reward), int(self.norm_cost),
                     float(self.clip_obs), float(self.clip_reward), float(self.clip_cost), float(self.gamma),
                     float(self.cost_gamma), float(self.epsilon), p(self.obs_rms.d_mean), p(self.obs_rms.d_var),
                     p(self.obs_rms.d_count), p(self.ret_rms.d_stats), p(self.cost_rms.d_stats), p(self.ret), p(self.cost_ret))

    def _norm_call(self, obs, rews, cost, news):
        nm = self.struct()
        _lib.check(_lib.lib().icrl_vecnorm_step(_lib.byref(nm), p(obs), p(rews), p(cost), p(news), self.num_envs,
                                                obs.shape[1], p(self._obs_out), p(self._rew_out),
                                                p(self._cost_out) if cost is not None else None, _lib.current_stream()),
                   "icrl_vecnorm_step")

    def step_wait(self):
        obs, rews, news, infos = self.venv.step_wait()
        self.old_obs, self.old_reward = obs, rews
        cost = infos.batch.get(getattr(self, "cost_str", "cost")) if isinstance(infos, BatchedInfos) else None
        if cost is not None:
            self.old_cost = cost
        self._norm_call(obs.contiguous(), rews.contiguous(), None if cost is None else cost.contiguous(), news.contiguous())
        if cost is not None:
            infos.batch[getattr(self, "cost_str", "cost")] = self._cost_out.clone()
        return self._obs_out.clone(), self._rew_out.clone(), news, infos

    def normalize_obs(self, obs):
        """ref: vec_normalize.py:107-114 (no statistics update)."""
        if not self.norm_obs:
            return obs
        o = torch.as_tensor(obs, dtype=torch.float64, device=self.device)
        return torch.clamp((o - self.obs_rms.d_mean) / torch.sqrt(self.obs_rms.d_var + self.epsilon), -self.clip_obs, self.clip_obs)

    def unnormalize_obs(self, obs):
        """ref: vec_normalize.py:125-128, with the CURRENT statistics: float64(obs) * sqrt(var + eps) + mean, product and sum rounded
        separately (the bits icrl_gail_unnormalize_batch gives)."""
        if not self.norm_obs:
            return obs
        o = torch.as_tensor(obs, device=self.device).to(torch.float64)
        return o * torch.sqrt(self.obs_rms.d_var + self.epsilon) + self.obs_rms.d_mean

    def get_original_obs(self):
        return self.old_obs.clone()

    def get_original_reward(self):
        return self.old_reward.clone()

    def reset(self):
        obs = self.venv.reset()
        self.old_obs = obs
        nm = self.struct()
        _lib.check(_lib.lib().icrl_vecnorm_reset(_lib.byref(nm), p(obs.contiguous()), self.num_envs, obs.shape[1],
                                                 p(self._obs_out), _lib.current_stream()), "icrl_vecnorm_reset")
        return self._obs_out.clone()

    # -- persistence: statistics only, like the reference's pickled wrapper minus venv / ret (vec_normalize.py:42-53,159-181)
    def _state(self):
        return dict(obs_rms=(self.obs_rms.mean, self.obs_rms.var, self.obs_rms.count),
                    ret_rms=(self.ret_rms.mean, self.ret_rms.var, self.ret_rms.count),
                    cost_rms=(self.cost_rms.mean, self.cost_rms.var, self.cost_rms.count),
                    **{k: getattr(self, k) for k in ("clip_obs", "clip_reward", "clip_cost", "gamma", "cost_gamma", "epsilon",
                                                      "training", "norm_obs", "norm_reward", "norm_cost")})

    def save(self, save_path):
        with open(save_path, "wb") as f:
            pickle.dump(self._state(), f)

    @classmethod
    def load(cls, load_path, venv):
        """reads the statistics file written by save() or by the REFERENCE (a pickled VecNormalize[WithCost] object,
        vec_normalize.py:42-64,159-181: its class instances are read as attribute bags, no stable_baselines3 / gym needed)."""
        from .utils import load_reference_pickle
        st = load_reference_pickle(load_path)
        if not isinstance(st, dict):
            ref = st.__dict__
            rms = lambda r: (np.asarray(r.mean), np.asarray(r.var), float(r.count))
            st = dict(obs_rms=rms(ref["obs_rms"]), ret_rms=rms(ref["ret_rms"]),
                      cost_rms=rms(ref["cost_rms"]) if "cost_rms" in ref else (0.0, 1.0, 1e-4))
            for k in ("clip_obs", "clip_reward", "clip_cost", "gamma", "cost_gamma", "epsilon", "training", "norm_obs", "norm_reward",
                      "norm_cost", "cost_str"):
                if k in ref:
                    st[k] = ref[k]
        obj = cls(venv)
        for k in ("obs_rms", "ret_rms", "cost_rms"):
            getattr(obj, k).assign(*st.pop(k))
        for k, v in st.items():
            setattr(obj, k, v)
        return obj


class VecNormalizeWithCost(VecNormalize):
    """ref: vec_normalize.py:184-278."""

    def __init__(self, venv, training=True, norm_obs=True, norm_reward=True, norm_cost=True, cost_info_str="cost",
                 clip_obs=10.0, clip_reward=10.0, clip_cost=10.0, reward_gamma=0.99, cost_gamma=0.99, epsilon=1e-8):
        super().__init__(venv, training, norm_obs, norm_reward, clip_obs, clip_reward, reward_gamma, epsilon)
        self.norm_cost, self.cost_str, self.clip_cost, self.cost_gamma = norm_cost, cost_info_str, clip_cost, cost_gamma

    def get_original_cost(self):
        return self.old_cost.clone()


def sync_envs_normalization(env, eval_env):
    """obs_rms and ret_rms are copied, cost_rms is not (ref: vec_env/__init__.py:50-65)."""
    env_tmp, eval_tmp = env, eval_env
    while isinstance(env_tmp, VecEnvWrapper):
        if isinstance(env_tmp, VecNormalize):
            eval_tmp.obs_rms = copy.deepcopy(env_tmp.obs_rms)
            eval_tmp.ret_rms = copy.deepcopy(env_tmp.ret_rms)
        env_tmp = env_tmp.venv
        if isinstance(env_tmp, VecCostWrapper):
            env_tmp = env_tmp.venv
        eval_tmp = eval_tmp.venv if isinstance(eval_tmp, VecEnvWrapper) else eval_tmp
