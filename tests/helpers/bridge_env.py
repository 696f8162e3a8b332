"""The dense Two Bridges envs and PointTrack of the reference as a numpy VecEnv with oracle.synth_env.SynthVecEnv's interface (n_envs,
obs_dim, act_dim, action_low / action_high, t_ep, reset(), step(a) -> obs, rew, done with auto-reset), as helpers/point_env.PointVecEnv is.
Written from the specification in DESIGN.md §21 (ref: custom_envs/custom_envs/envs/two_bridges.py:94-117,237-418, envs/utils.py:9-69,
envs/point.py:284-376; the 200- / 150-step TimeLimit of custom_envs/__init__.py); tools/gen_bridges_golden.py checks it against the
reference's own classes and records tests/golden/g24_bridge_env.npz.

All float64, one rounding per operation, in the reference's order.  The envs are stepped one after the other with Python floats,
math.cos / math.sin, np.around for the discrete lattice and `** 0.5` on a numpy float64 for the dense reward: what the reference does.
`margin` (a list, when given) collects the distance of every decision operand of a step from its threshold.
"""
import math

import numpy as np

# kind -> icrl_env_t.reward_form
FORMS = {"point_track": 9, "dd2b": 10, "cdd2b": 11, "ddcdd2b": 12, "c2b": 13, "cc2b": 14}
DIMS = {"point_track": (9, 2, 150), "dd2b": (2, 1, 200), "cdd2b": (2, 1, 200), "ddcdd2b": (2, 1, 200), "c2b": (3, 2, 200), "cc2b": (3, 2, 200)}
DISCRETE = ("dd2b", "cdd2b", "ddcdd2b")
CONTINUOUS = ("c2b", "cc2b")
SIZE, CTRL, SCALE = 20.0, 2.0, 0.7
WATER = ((4.0, 0.0, 4.0, 5.0), (4.0, 6.0, 4.0, 8.0), (4.0, 15.0, 4.0, 5.0))      # origin x, y, width, height
CONSTRAINT = (4.0, 5.0, 4.0, 1.0)
MOVES = ((SCALE * 1, SCALE * 0), (SCALE * -1, SCALE * 0), (SCALE * 0, SCALE * 1), (SCALE * 0, SCALE * -1))
START = {12: (3.0, 5.0)}


def _clip(v, lo, hi):
    return min(max(v, lo), hi)


def orientation_value(p, q, r):
    return ((q[1] - p[1]) * (r[0] - q[0])) - ((q[0] - p[0]) * (r[1] - q[1]))


def _sign(v):
    return 0 if v == 0 else (1 if v > 0 else -1)


def on_segment(p, q, r):
    return r[0] <= max(p[0], q[0]) and r[0] >= min(p[0], q[0]) and r[1] <= max(p[1], q[1]) and r[1] >= min(p[1], q[1])


def intersects(p1, q1, p2, q2, margin=None, e1=(False, False), f1=(False, False)):
    v = (orientation_value(p1, q1, p2), orientation_value(p1, q1, q2), orientation_value(p2, q2, p1), orientation_value(p2, q2, q1))
    if margin is not None:
        T = (True, True)
        ex = (_exact_orientation(p1, q1, p2, e1, f1, T), _exact_orientation(p1, q1, q2, e1, f1, T), _exact_orientation(p2, q2, p1, T, T, e1),
              _exact_orientation(p2, q2, q1, T, T, f1))
        margin.extend(abs(x) for x, e in zip(v, ex) if not e)
    o1, o2, o3, o4 = (_sign(x) for x in v)
    if o1 != o2 and o3 != o4:
        return True
    return ((o1 == 0 and on_segment(p1, q1, p2)) or (o2 == 0 and on_segment(p1, q1, q2)) or (o3 == 0 and on_segment(p2, q2, p1))
            or (o4 == 0 and on_segment(p2, q2, q1)))


def _exact_orientation(p, q, r, ep, eq, er):
    """whether the orientation value is the same bits in every implementation: each product has two exact factors or an exact zero factor
    (a coordinate is exact at the start position and where the env clipped it to +-20; boundary corners are exact)."""
    def product(a, ea, b, eb):
        return (ea and eb) or (ea and a == 0) or (eb and b == 0)
    return (product(q[1] - p[1], eq[1] and ep[1], r[0] - q[0], er[0] and eq[0]) and
            product(q[0] - p[0], eq[0] and ep[0], r[1] - q[1], er[1] and eq[1]))


def in_rectangle(s, region, margin=None, exact=(False, False)):
    ox, oy, w, h = region
    if margin is not None:
        if not exact[0]:
            margin.extend((abs(s[0] - ox), abs(s[0] - (ox + w))))
        if not exact[1]:
            margin.extend((abs(s[1] - oy), abs(s[1] - (oy + h))))
    return s[0] > ox and s[0] < ox + w and s[1] > oy and s[1] < oy + h


def in_region(prev, nxt, region, margin=None, e_prev=(False, False), e_next=(False, False)):
    """-> (hit, through an end point).  With `margin` every test is evaluated (no short circuit), so that every operand is recorded.
    e_prev / e_next: which coordinates are exact, the same bits in every implementation (the start position, a coordinate clipped to
    +-20): what is computed from exact values alone may sit exactly on a threshold ((0, 0) lies on a line through a boundary) and is no
    operand that two implementations could decide differently; it is not recorded."""
    ox, oy, w, h = region
    a, b = in_rectangle(prev, region, margin, e_prev), in_rectangle(nxt, region, margin, e_next)
    if (a or b) and margin is None:
        return True, True
    bounds = (((ox, oy), (ox + w, oy)), ((ox, oy), (ox, oy + h)), ((ox + w, oy), (ox + w, oy + h)), ((ox, oy + h), (ox + w, oy + h)))
    hits = [intersects(prev, nxt, p2, q2, margin, e_prev, e_next) for p2, q2 in bounds]
    return (a or b or any(hits)), (a or b)


def regions_of(form):
    return WATER if form in (10, 13) else WATER + (CONSTRAINT,)


def bridge_reward(form, state, nxt, margin=None, events=None, e_prev=(False, False), e_next=(False, False)):
    """reward() of the dense envs -> next position, reward, whether the move was rejected.  events (a set, when given) names the branch."""
    cont = form >= 13
    if margin is not None:
        for i in (0, 1):
            if not e_next[i]:
                margin.extend((abs(nxt[i]), abs(nxt[i] - SIZE)))
    wall = min(nxt) < 0 or max(nxt) > SIZE
    water = [in_region(state, nxt, r, margin, e_prev, e_next) for r in WATER]
    cons = in_region(state, nxt, CONSTRAINT, margin, e_prev, e_next) if form not in (10, 13) else (False, False)
    if events is not None:
        if wall:
            events.add("wall")
        elif any(h for h, _ in water):
            events.add("water_end_point" if any(e for _, e in water) else "water_crossing")
        elif cons[0]:
            events.add("constraint")
    if wall or any(h for h, _ in water) or cons[0]:
        return (state[0], state[1]), -2.0, True
    gx, gy = SIZE - nxt[0], 0.0 - nxt[1]
    d2 = gx * gx + gy * gy
    if margin is not None:
        margin.append(abs(d2 - 1.0))
        if not e_next[0]:
            margin.append(abs(nxt[0] - 4.0))
    if d2 < 1:
        rew = 250.0 if cont else 12.0
        ev = "goal"
    elif nxt[0] > 4.0:
        rew = 10 / (np.float64(d2) ** (1 / 2))
        ev = "right"
        if cont:
            if margin is not None and not e_next[1]:
                margin.append(abs(nxt[1] - 6.0))
            if nxt[1] < 6.0:
                rew = rew * 20
                ev = "right_x20"
        if 5.0 < nxt[1] < 6.0 and 4.0 <= nxt[0] <= 8.0:
            ev_b = "lower_bridge"
        elif 14.0 < nxt[1] < 15.0 and 4.0 <= nxt[0] <= 8.0:
            ev_b = "upper_bridge"
        else:
            ev_b = None
        if events is not None and ev_b:
            events.add(ev_b)
    else:
        rew, ev = -1.0, "left"
    if events is not None:
        events.add(ev)
    return (nxt[0], nxt[1]), float(rew), False


def bridge_step(form, x0, y0, ori0, a0, a1=0.0, margin=None, events=None, exact=None):
    """one step of one env -> x, y, ori, reward (no done: only the time limit ends an episode).  exact (a two-element list, with
    `margin`): which coordinates of the position are exact, updated in place."""
    e_prev = tuple(exact) if exact is not None else (False, False)
    e_next = (False, False)
    if form >= 13:
        a0, a1 = _clip(float(a0), -CTRL, CTRL), _clip(float(a1), -CTRL, CTRL)
        ori = ori0 + a1
        dx, dy = math.cos(ori) * a0, math.sin(ori) * a0
        nxt = (_clip(x0 + dx, -SIZE, SIZE), _clip(y0 + dy, -SIZE, SIZE))
        if margin is not None:      # the clip's own decisions, and what it made exact
            margin.extend((abs(abs(x0 + dx) - SIZE), abs(abs(y0 + dy) - SIZE)))
            # (exact too: an exact coordinate that an exactly zero increment leaves alone; sin(0) = 0 in every library, and ori is
            # exactly 0 whenever the clipped turns +-2 cancel)
            e_next = (abs(x0 + dx) > SIZE or (e_prev[0] and dx == 0), abs(y0 + dy) > SIZE or (e_prev[1] and dy == 0))
    else:
        ori, ix = 0.0, int(a0)
        mx, my = MOVES[ix] if 0 <= ix < 4 else (0.0, 0.0)      # (the reference raises outside 0..3; the device moves nowhere)
        nxt = tuple(float(v) for v in np.around(np.array([x0 + mx, y0 + my]), 6))
    (x, y), rew, rejected = bridge_reward(form, (x0, y0), nxt, margin if form >= 13 else None, events, e_prev, e_next)
    if exact is not None and not rejected:
        exact[:] = e_next
    return x, y, ori, rew


def track_step(x0, y0, ori0, a0, a1, margin=None):
    """PointTrack (point.py:337-376) -> x, y, ori, reward."""
    a0, a1 = _clip(float(a0), -0.25, 0.25), _clip(float(a1), -0.25, 0.25)
    ori = ori0 + a1
    dx, dy = math.cos(ori) * a0, math.sin(ori) * a0
    x, y = _clip(x0 + dx, -40.0, 40.0), _clip(y0 + dy, -40.0, 40.0)
    ctrl = a0 * a0 + a1 * a1
    off = abs(math.sqrt(x * x + y * y) - 10.0)
    if margin is not None:
        margin.append(abs(off - 2.0))
    rew = ((-y * dx + x * dy) + (1 if off < 2.0 else 0)) + 0.0 * ctrl
    return x, y, ori, rew


class BridgeVecEnv:
    def __init__(self, n_envs, kind="dd2b", seed=0, env_index_offset=0):
        self.kind, self.reward_form = kind, FORMS[kind]
        self.obs_dim, self.act_dim, self.max_steps = DIMS[kind]
        self.n_envs = n_envs
        self.wall_terminate = self.broken = False
        self.discrete = kind in DISCRETE
        ctrl = 0.25 if kind == "point_track" else CTRL
        self.action_low = None if self.discrete else -np.full(self.act_dim, ctrl, np.float32)
        self.action_high = None if self.discrete else np.full(self.act_dim, ctrl, np.float32)
        self.margin, self.events = None, None      # set to a list / a set to have the steps record them
        self.seed(seed, env_index_offset)

    def start(self):
        s = np.zeros(self.obs_dim, np.float64)
        s[:2] = START.get(self.reward_form, (0.0, 0.0))
        return s

    def seed(self, seed, env_index_offset=0):      # nothing is drawn: fixed start, reset noise scale 0
        self.t_ep = np.zeros(self.n_envs, np.int64)
        self.s = np.tile(self.start(), (self.n_envs, 1))
        self.exact = [[True, True] for _ in range(self.n_envs)]      # (margin recording: the start position is exact)

    def reset(self):
        self.s[:] = self.start()
        self.t_ep[:] = 0
        self.exact = [[True, True] for _ in range(self.n_envs)]
        return self.s.copy()

    def step(self, actions):
        a = np.asarray(actions).astype(np.float64).reshape(self.n_envs, self.act_dim)
        rew, done = np.zeros(self.n_envs, np.float64), np.zeros(self.n_envs, bool)
        for n in range(self.n_envs):
            s = self.s[n]
            if self.reward_form == 9:
                x, y, ori, r = track_step(s[0], s[1], s[2], a[n, 0], a[n, 1], self.margin)
                new = (x, y, ori, 0.0, 0.0, 0.0, x, y, 0.0)
            else:
                x, y, ori, r = bridge_step(self.reward_form, s[0], s[1], s[2] if self.obs_dim > 2 else 0.0, a[n, 0],
                                           a[n, 1] if self.act_dim > 1 else 0.0, self.margin, self.events, self.exact[n])
                new = (x, y, ori)[:self.obs_dim]
            self.t_ep[n] += 1
            d = self.t_ep[n] >= self.max_steps
            rew[n], done[n] = r, d
            if d:
                self.s[n] = self.start()
                self.t_ep[n] = 0
                self.exact[n][:] = (True, True)
            else:
                self.s[n] = new
        return self.s.copy(), rew, done
