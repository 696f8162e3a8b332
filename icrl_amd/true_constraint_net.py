"""Ground-truth cost functions: what `cpg` trains the expert against and the `true/cost` metric
(ref: icrl/true_constraint_net.py:11-55, 104-111).

`get_true_cost_function` returns `AnalyticCost` objects: closed forms on (previous raw observation, clipped action) that the library
evaluates inside the fused rollout launches (icrl_cost_fn_t, csrc/cost_fn.h) and, on device tensors, through icrl_cost_fn_rows.  On numpy
arrays they compute exactly what the reference's functions compute.  The module-level `wall_behind`, `null_cost` and `lap_grid_world` stay
plain numpy functions (callables handed to `learn(cost_function=...)` keep the per-step loop and its semantics).

`BridgesCost` is the reference's `bridges()` for CDD2B-v0 / CC2B-v0: host side only, a plain callable.  `true_cost_for` is the
resolver the entry points call: a `BridgesCost` for those two ids, `get_true_cost_function` for every other.
"""
import math

import numpy as np
import torch

from . import _lib
from .structs import (COST_ACTION_EQUALS, COST_FN, COST_NULL, COST_TORQUE, COST_WALL_BEHIND, COST_WALL_BOTH, COST_WALL_INFRONT, CostFnT, p)


def wall_behind(pos, obs, acs):
    return obs[..., 0] <= pos


def null_cost(x, *args):
    return np.zeros(x.shape[:1])


def lap_grid_world(obs, acs):
    """ref: icrl/true_constraint_net.py:104-111 — the backward action (index 1) is the constraint violation."""
    a = acs.reshape(acs.shape[0], -1)[:, 0]
    return a == 1


class AnalyticCost:
    """One of the reference's ground-truth costs (or the null cost) as a description the kernels can evaluate.

    numpy in -> numpy out, the reference's function operation for operation (same dtype: bool for the single walls, torque and
    action_equals, float32 for the two-wall sum, float64 zeros for the null cost; `acs` may be None where it is not read; leading batch
    dimensions as the reference's functions take them).  Device tensors in -> a float32 device tensor from icrl_cost_fn_rows.
    `.struct(obs_dim, acs_dim)` is the descriptor the rollout entry points take in place of a constraint net's."""

    WALLS = (COST_WALL_BEHIND, COST_WALL_INFRONT, COST_WALL_BOTH)

    def __init__(self, kind, index=0, lo=0.0, hi=0.0, name="analytic"):
        self.kind, self.index, self.lo, self.hi, self.name = int(kind), int(index), lo, hi, name

    # ---- constructors (ref: icrl/true_constraint_net.py:40-54, 104-111) ----
    @classmethod
    def null(cls):
        return cls(COST_NULL, name="null_cost")

    @classmethod
    def wall_behind(cls, pos, index=0):
        return cls(COST_WALL_BEHIND, index, lo=pos, name="wall_behind")

    @classmethod
    def wall_infront(cls, pos, index=0):
        return cls(COST_WALL_INFRONT, index, hi=pos, name="wall_infront")

    @classmethod
    def wall_behind_and_infront(cls, back, front, index=0):
        return cls(COST_WALL_BOTH, index, lo=back, hi=front, name="wall_behind_and_infront")

    @classmethod
    def torque(cls, threshold):
        return cls(COST_TORQUE, lo=threshold, name="torque_constraint")

    @classmethod
    def action_equals(cls, value):
        return cls(COST_ACTION_EQUALS, index=value, name="action_equals")

    def __repr__(self):
        return f"AnalyticCost({self.name}, index={self.index}, lo={self.lo}, hi={self.hi})"

    def struct(self, obs_dim, acs_dim):
        return CostFnT(int(obs_dim), int(acs_dim), 0, COST_FN, self.kind, self.index, float(self.lo), float(self.hi))

    # ---- evaluation ----
    def __call__(self, obs, acs=None):
        if torch.is_tensor(obs) or torch.is_tensor(acs):
            return self._device(obs, acs)
        k, i = self.kind, self.index
        if k == COST_NULL:
            return np.zeros(obs.shape[:1])
        if k == COST_WALL_BEHIND:
            return obs[..., i] <= self.lo
        if k == COST_WALL_INFRONT:
            return obs[..., i] >= self.hi
        if k == COST_WALL_BOTH:
            return (obs[..., i] <= self.lo).astype(np.float32) + (obs[..., i] >= self.hi).astype(np.float32)
        if k == COST_TORQUE:
            return np.any(np.abs(acs) > self.lo, axis=-1)
        a = np.asarray(acs)
        return a.reshape(a.shape[0], -1)[:, 0] == i

    def _device(self, obs, acs):
        """icrl_cost_fn_rows over the flattened leading dimensions: float32 costs on the device, no host copies."""
        ref = obs if torch.is_tensor(obs) else acs
        dev = ref.device
        reads_obs, reads_acs = self.kind in self.WALLS, self.kind in (COST_TORQUE, COST_ACTION_EQUALS)
        if self.kind == COST_ACTION_EQUALS:
            a = torch.as_tensor(acs, device=dev)
            lead = a.shape[:1]
            a = a.reshape(a.shape[0], -1)[:, :1].to(torch.float32).contiguous()
            o, obs_dim, acs_dim = None, 1, 1
        else:
            o = torch.as_tensor(obs, device=dev).to(torch.float64) if (reads_obs or not reads_acs) else None
            a = torch.as_tensor(acs, device=dev).to(torch.float32) if reads_acs else None
            lead = o.shape[:-1] if reads_obs else (a.shape[:-1] if reads_acs else o.shape[:1])
            obs_dim = o.shape[-1] if o is not None and o.dim() > 1 else 1
            acs_dim = a.shape[-1] if a is not None else 1
            o = o.reshape(-1, obs_dim).contiguous() if reads_obs else None
            a = a.reshape(-1, acs_dim).contiguous() if reads_acs else None
        n = int(np.prod(lead)) if len(lead) else 1
        out = torch.empty(n, dtype=torch.float32, device=dev)
        if n > 0:
            cf = self.struct(obs_dim, acs_dim)
            _lib.check(_lib.lib().icrl_cost_fn_rows(_lib.byref(cf), p(o), p(a), n, p(out), _lib.current_stream()), "icrl_cost_fn_rows")
        return out.reshape(tuple(lead))


TRUE_COSTS = {
    # ref: icrl/true_constraint_net.py:13-34 (the bridge envs are not in this table: CDD2B / CC2B are served by true_cost_for -> BridgesCost,
    # not as an analytic kind; CDD3B is not served)
    **{k: ("wall_behind", -3) for k in ("HCWithPosTest-v0", "WalkerWithPosTest-v0", "SwimmerWithPosTest-v0", "AntWallTest-v0",
                                        "AntWallBrokenTest-v0", "PointCircleTestBack-v0")},
    **{k: ("wall_behind_and_infront", -3, +3) for k in ("PointNullRewardTest-v0", "PointCircleTest-v0", "AntCircleTest-v0")},
    **{k: ("torque", 0.5) for k in ("AntTest-v0", "HalfCheetahTest-v0", "Walker2dTest-v0", "SwimmerTest-v0")},
    "CLGW-v0": ("action_equals", 1),
}


def get_true_cost_function(env_id):
    """ref: icrl/true_constraint_net.py:11-34."""
    entry = TRUE_COSTS.get(env_id)
    if entry is None:
        print("Cost function for %s is not implemented yet. Returning null cost function" % env_id)
        return null_cost
    return getattr(AnalyticCost, entry[0])(*entry[1:])


# ---- the Two Bridges cost (ref: icrl/true_constraint_net.py:60-102, custom_envs/envs/utils.py:9-69) ---------------------------------
def _orientation(p0, p1, q0, q1, r0, r1):
    val = ((q1 - p1) * (r0 - q0)) - ((q0 - p0) * (r1 - q1))
    return np.where(val == 0, 0, np.where(val > 0, 1, -1))


def _on_segment(p0, p1, q0, q1, r0, r1):
    return (r0 <= np.maximum(p0, q0)) & (r0 >= np.minimum(p0, q0)) & (r1 <= np.maximum(p1, q1)) & (r1 >= np.minimum(p1, q1))


def in_region_rows(prev, nxt, region):
    """utils.in_regions for one rectangle (origin, width, height), over rows: prev, nxt float64 [n, 2] -> bool [n].  An end point strictly
    inside, or the segment prev -> nxt meets one of the four boundary segments (orientation compared with 0 exactly, as the reference)."""
    (ox, oy), w, h = region
    ox, oy, x1, y1 = float(ox), float(oy), float(ox + w), float(oy + h)
    sx, sy, nx, ny = prev[:, 0], prev[:, 1], nxt[:, 0], nxt[:, 1]
    hit = (sx > ox) & (sx < x1) & (sy > oy) & (sy < y1)
    hit |= (nx > ox) & (nx < x1) & (ny > oy) & (ny < y1)
    for (b0, b1), (c0, c1) in (((ox, oy), (x1, oy)), ((ox, oy), (ox, y1)), ((x1, oy), (x1, y1)), ((ox, y1), (x1, y1))):
        o1, o2 = _orientation(sx, sy, nx, ny, b0, b1), _orientation(sx, sy, nx, ny, c0, c1)
        o3, o4 = _orientation(b0, b1, c0, c1, sx, sy), _orientation(b0, b1, c0, c1, nx, ny)
        hit |= (o1 != o2) & (o3 != o4)
        hit |= (o1 == 0) & _on_segment(sx, sy, nx, ny, b0, b1)
        hit |= (o2 == 0) & _on_segment(sx, sy, nx, ny, c0, c1)
        hit |= (o3 == 0) & _on_segment(b0, b1, c0, c1, sx, sy)
        hit |= (o4 == 0) & _on_segment(b0, b1, c0, c1, nx, ny)
    return hit


class BridgesCost:
    """The reference's `bridges(env, obs, acs)` for CDD2B-v0 (discrete) and CC2B-v0 (continuous): 1 where the move from the raw
    observation under the action touches the constraint rectangle ((4, 5), 4, 1) over the lower bridge, else 0 (int64), vectorised over
    rows; `[batch, n_envs, .]` inputs give `[batch, n_envs]` costs as in the reference.

    The continuous form keeps the reference's quirk (:92-95): `ob` is overwritten by the next position before `in_regions`, so the cost
    only sees where the move ends (strictly inside the rectangle or exactly on its boundary), not what it crosses.  Actions are taken as
    float64 (the reference's pinned numpy promotes a float32 action before anything is computed with it).  Device tensors are copied
    to the host.  A plain callable: not an AnalyticCost, so a run that trains or evaluates against it takes the per-step loop."""

    IDS = {"CDD2B-v0": False, "CC2B-v0": True}
    CONSTRAINT = ((4, 5), 4, 1)
    MOVES = 0.7 * np.array([(1, 0), (-1, 0), (0, 1), (0, -1)])      # two_bridges.py:243-247
    SIZE, CTRL = 20.0, 2.0

    def __init__(self, env_id):
        if env_id not in self.IDS:
            raise ValueError(f"BridgesCost: {env_id!r}; served: {', '.join(self.IDS)}")
        self.env_id, self.continuous, self.name = env_id, self.IDS[env_id], "bridges"

    def __repr__(self):
        return f"BridgesCost({self.env_id})"

    def __call__(self, obs, acs):
        obs = obs.detach().cpu().numpy() if torch.is_tensor(obs) else np.asarray(obs)
        acs = acs.detach().cpu().numpy() if torch.is_tensor(acs) else np.asarray(acs)
        if obs.ndim > 2:
            shape = obs.shape[:2]
            obs, acs = obs.reshape(shape[0] * shape[1], -1), acs.reshape(shape[0] * shape[1], -1)
        else:
            shape = (obs.shape[0],)
            acs = acs.reshape(obs.shape[0], -1)
        ob = obs.astype(np.float64)
        if not self.continuous:
            prev = ob[:, :2]
            nxt = np.around(prev + self.MOVES[acs[:, 0].astype(np.int64)], 6)
        else:
            ac = np.clip(acs.astype(np.float64), -self.CTRL, self.CTRL)
            ori = ob[:, 2] + ac[:, 1]
            dx = np.array([math.cos(v) for v in ori]) * ac[:, 0]
            dy = np.array([math.sin(v) for v in ori]) * ac[:, 0]
            nxt = np.stack([np.clip(ob[:, 0] + dx, -self.SIZE, self.SIZE), np.clip(ob[:, 1] + dy, -self.SIZE, self.SIZE)], axis=1)
            prev = nxt
        return in_region_rows(prev, nxt, self.CONSTRAINT).astype(np.int64).reshape(shape)


def true_cost_for(env_id):
    """what icrl / cpg / gail train and evaluate against: BridgesCost for the two constrained Two Bridges ids, get_true_cost_function for
    every other id (which itself, and the analytic kinds of icrl_cost_fn_t, do not know the bridge cost: DESIGN §21)."""
    if env_id in BridgesCost.IDS:
        return BridgesCost(env_id)
    return get_true_cost_function(env_id)


def mean_cost(fn, obs, acs):
    """mean of a cost function over rows; an AnalyticCost is evaluated where the rows are (device tensors: on the device)."""
    c = fn(obs, acs)
    return float(c.double().mean().item()) if torch.is_tensor(c) else float(np.mean(c))
