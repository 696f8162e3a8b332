"""The Point envs of the reference as a numpy VecEnv with oracle.synth_env.SynthVecEnv's interface (n_envs, obs_dim, act_dim,
action_low / action_high, t_ep, reset(), step(a) -> obs, rew, done with auto-reset), so that oracle.loop.EnvStack / PortAgent run over
it unchanged.  Written from the specification in DESIGN.md §17 (ref: custom_envs/custom_envs/envs/point.py:22-276, 150-step TimeLimit of
custom_envs/__init__.py:123-163); tools/gen_point_golden.py checks it against the reference's own classes and records
tests/golden/g23_point_env.npz.

All float64, one rounding per operation, in the reference's order (its semantics under numpy 1.17: a float32 action is promoted to
float64 before anything is computed with it).  The envs are stepped one after the other with Python floats and math.cos / math.sin:
what the reference does.
"""
import math

import numpy as np

# kind -> icrl_env_t.reward_form
FORMS = {"point_circle": 4, "point_circle_test": 5, "point_circle_test_back": 6, "point_null": 7, "point_null_test": 8}
OBS_DIM, ACT_DIM, MAX_STEPS, CTRL, SIZE, TARGET = 9, 2, 150, 0.25, 40.0, 10.0


def _clip(v, lo, hi):
    return min(max(v, lo), hi)


def point_step(form, x0, y0, ori0, a0, a1):
    """one step of one env -> x, y, ori, reward, done (before the time limit)."""
    a0, a1 = _clip(float(a0), -CTRL, CTRL), _clip(float(a1), -CTRL, CTRL)
    ori = ori0 + a1
    dx, dy = math.cos(ori) * a0, math.sin(ori) * a0
    x, y = _clip(x0 + dx, -SIZE, SIZE), _clip(y0 + dy, -SIZE, SIZE)
    if form <= 6:
        rew = (y * dx - x * dy) / (1.0 + abs(math.sqrt(x * x + y * y) - TARGET))
    else:
        rew = 1.0
    done = False
    if form in (5, 8) and (x > 3.0 or x < -3.0):      # strict: x == -3 goes on
        done = True
        if form == 5:
            rew = 0.0
    if form == 6 and x < -3.0:
        done, rew = True, 0.0
    return x, y, ori, rew, done


class PointVecEnv:
    def __init__(self, n_envs, kind="point_circle", seed=0, env_index_offset=0):
        self.kind, self.reward_form = kind, FORMS[kind]
        self.obs_dim, self.act_dim, self.max_steps = OBS_DIM, ACT_DIM, MAX_STEPS
        self.n_envs = n_envs
        self.wall_terminate = self.reward_form in (5, 6, 8)
        self.broken = False
        self.action_low = -np.full(ACT_DIM, CTRL, np.float32)
        self.action_high = np.full(ACT_DIM, CTRL, np.float32)
        self.seed(seed, env_index_offset)

    def seed(self, seed, env_index_offset=0):      # nothing is drawn: reset noise scale 0
        self.t_ep = np.zeros(self.n_envs, np.int64)
        self.s = np.zeros((self.n_envs, OBS_DIM), np.float64)

    def reset(self):
        self.s[:] = 0.0
        self.t_ep[:] = 0
        return self.s.copy()

    def step(self, actions):
        a = np.asarray(actions).astype(np.float64).reshape(self.n_envs, ACT_DIM)
        rew, done = np.zeros(self.n_envs, np.float64), np.zeros(self.n_envs, bool)
        for n in range(self.n_envs):
            x, y, ori, r, d = point_step(self.reward_form, self.s[n, 0], self.s[n, 1], self.s[n, 2], a[n, 0], a[n, 1])
            self.t_ep[n] += 1
            d = d or self.t_ep[n] >= self.max_steps
            rew[n], done[n] = r, d
            if d:
                self.s[n] = 0.0
                self.t_ep[n] = 0
            else:
                self.s[n] = (x, y, ori, 0.0, 0.0, 0.0, x, y, 0.0)
        return self.s.copy(), rew, done
