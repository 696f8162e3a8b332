"""A small host env whose episodes are short and of different lengths in different envs of a VecEnv, for the episode-statistics tests;
importing this module registers it (`--env_module tests.helpers.short_host_envs`):

    HostShortEpisodes-v0    Box(3) float64 observations, Box(-1, 1, (2,)) float32 actions; the time limit depends on the env's seed
                            (17 + 6 * (seed % 4) steps, so envs seeded s, s + 1, ... end at different steps and envs 4 apart together),
                            and an episode also ends early when the first state component falls below -0.25.  Rewards are float64
                            values that are not exactly representable sums (the order of a float64 sum shows).
"""
import numpy as np

from icrl_amd import envs, spaces

_MOD = "tests.helpers.short_host_envs"


class ShortEpisodeEnv:
    def __init__(self):
        self.observation_space = spaces.Box(-np.inf, np.inf, (3,), np.float64)
        self.action_space = spaces.Box(-1.0, 1.0, (2,), np.float32)
        self.seed(0)

    def seed(self, seed=None):
        seed = 0 if seed is None else int(seed)
        self.limit = 17 + 6 * (seed % 4)
        self._max_episode_steps = self.limit
        self.rng = np.random.RandomState(seed)
        self.t, self.x = 0, np.zeros(3)
        return [seed]

    def reset(self):
        self.t = 0
        self.x = 0.1 * self.rng.randn(3)
        return self.x.copy()

    def step(self, action):
        a = np.asarray(action, np.float64).reshape(-1)
        self.x = 0.9 * self.x + 0.1 * np.array([a[0], a[1], a[0] * a[1]])
        self.t += 1
        rew = float(self.x[0] + 0.3 * self.x[2] - 0.1 * (a * a).sum() + 0.01 * self.t)
        done = bool(self.t >= self.limit or self.x[0] < -0.25)
        return self.x.copy(), rew, done, {}

    def close(self):
        pass


envs.register("HostShortEpisodes-v0", f"{_MOD}:ShortEpisodeEnv")
