"""Ground-truth cost functions: what `cpg` trains the expert against and the `true/cost` metric
(ref: icrl/true_constraint_net.py:11-55, 104-111).

`get_true_cost_function` returns `AnalyticCost` objects: closed forms on (previous raw observation, clipped action) that the library
evaluates inside the fused rollout launches (icrl_cost_fn_t, csrc/cost_fn.h) and, on device tensors, through icrl_cost_fn_rows.  On numpy
arrays they compute exactly what the reference's functions compute.  The module-level `wall_behind`, `null_cost` and `lap_grid_world` stay
plain numpy functions (callables handed to `learn(cost_function=...)` keep the per-step loop and its semantics).

`RegionCost` is a user-defined ground-truth constraint (`--cost_spec`): 1..8 box / halfspace / ball clauses over observation and action
columns, combined by any / all / sum, evaluated by the rollout kernels themselves (icrl_cost_region_t) and, on device tensors, through
icrl_cost_region_rows.  `cost_for(env_id, cost_spec, env)` is the resolver of the entry points' `--cost_spec` flag.

`BridgesCost` is the reference's `bridges()` for CDD2B-v0 / CC2B-v0: host side only, a plain callable.  `true_cost_for` is the
resolver the entry points call: a `BridgesCost` for those two ids, `get_true_cost_function` for every other.
"""
import math

import numpy as np
import torch

from . import _lib
from .structs import (COST_ACTION_EQUALS, COST_FN, COST_NULL, COST_REGION, COST_TORQUE, COST_WALL_BEHIND, COST_WALL_BOTH, COST_WALL_INFRONT,
                      REGION_ALL, REGION_ANY, REGION_BALL, REGION_BOX, REGION_HALFSPACE, REGION_MAX_CLAUSES, REGION_MAX_TERMS, REGION_SUM,
                      CostFnT, CostRegionT, RegionClauseT, p)


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


class RegionCost:
    """A region cost: `combine` (any | all | sum) over 1..8 clauses, each a box, a halfspace or a ball over 1..8 columns of
    (previous raw observation float64 [obs_dim], clipped action float32 [acs_dim]; one column, the class index, when discrete).
    Column c < obs_dim is observation column c, column obs_dim + j action column j; every value is taken as float64.

        box        true iff for every term  lo_k <= x_k <= hi_k
        halfspace  acc = b; in term order acc = acc + w_k * x_k (each product and each sum rounded once); true iff acc >= 0
        ball       acc = 0; in term order d = x_k - c_k, acc = acc + d * d; true iff acc <= r * r (computed once, here)

    `negate` flips a clause; a NaN makes the un-negated clause false.  numpy in -> float32 numpy out by exactly these operations in this
    order; device tensors in -> a float32 device tensor from icrl_cost_region_rows, no host copies.  `.struct()` is the descriptor the
    rollout entry points take in place of a constraint net's; it keeps the host and the device clause table alive."""

    TYPES = {"box": REGION_BOX, "halfspace": REGION_HALFSPACE, "ball": REGION_BALL}
    COMBINE = {"any": REGION_ANY, "all": REGION_ALL, "sum": REGION_SUM}

    def __init__(self, clauses, combine, obs_dim, acs_dim, discrete=False, name="region_cost"):
        """clauses: [(type, negate, cols, a, b, c)] with resolved column numbers, as from_spec builds them."""
        self.obs_dim, self.acs_dim, self.discrete, self.name = int(obs_dim), (1 if discrete else int(acs_dim)), bool(discrete), name
        if combine not in self.COMBINE.values():
            raise ValueError(f"RegionCost: combine {combine!r} (one of {sorted(self.COMBINE)})")
        if not 1 <= len(clauses) <= REGION_MAX_CLAUSES:
            raise ValueError(f"RegionCost: clauses: {len(clauses)} clauses (1..{REGION_MAX_CLAUSES})")
        self.combine = int(combine)
        self.clauses = [(int(t), bool(ng), [int(c) for c in cols], [float(v) for v in a], [float(v) for v in b], float(c))
                        for t, ng, cols, a, b, c in clauses]
        self._struct = self._table = self._d_table = None

    # ---- the spec format: {"combine": "any|all|sum", "clauses": [{"type": ..., "cols": ["obs:0", "act:2"], ...}]} ----
    @classmethod
    def from_spec(cls, spec, obs_dim, acs_dim, discrete=False):
        """spec: a dict, a JSON string or the path of a JSON file.  `null` (None) is an infinite bound."""
        import json
        import os
        name = "region_cost"
        if isinstance(spec, (str, bytes, os.PathLike)):
            text = os.fspath(spec) if not isinstance(spec, bytes) else spec.decode()
            if not text.lstrip().startswith("{"):
                name = os.path.basename(text)
                with open(text) as f:
                    text = f.read()
            try:
                spec = json.loads(text)
            except json.JSONDecodeError as e:
                raise ValueError(f"RegionCost: the spec is not JSON: {e}") from None
        if not isinstance(spec, dict):
            raise ValueError(f"RegionCost: the spec must be an object with 'combine' and 'clauses', got {type(spec).__name__}")
        unknown = set(spec) - {"combine", "clauses"}
        if unknown:
            raise ValueError(f"RegionCost: unknown field(s) {sorted(unknown)} in the spec ('combine', 'clauses')")
        combine = spec.get("combine", "any")
        if combine not in cls.COMBINE:
            raise ValueError(f"RegionCost: combine: {combine!r} (one of {sorted(cls.COMBINE)})")
        raw = spec.get("clauses")
        if not isinstance(raw, (list, tuple)) or not 1 <= len(raw) <= REGION_MAX_CLAUSES:
            raise ValueError(f"RegionCost: clauses: a list of 1..{REGION_MAX_CLAUSES} clauses is required")
        n_act = 1 if discrete else int(acs_dim)

        def column(ci, text):
            kind, _, idx = text.partition(":") if isinstance(text, str) else ("", "", "")
            if kind not in ("obs", "act") or not idx.isdigit():
                raise ValueError(f"RegionCost: clause {ci}: cols: {text!r} is not 'obs:<i>' or 'act:<j>'")
            i, lim = int(idx), (int(obs_dim) if kind == "obs" else n_act)
            if i >= lim:
                raise ValueError(f"RegionCost: clause {ci}: cols: {text!r} is outside the {lim} {'observation' if kind == 'obs' else 'action'} "
                                 f"column(s){' of a discrete action space' if kind == 'act' and discrete else ''}")
            return i if kind == "obs" else int(obs_dim) + i

        def numbers(ci, c, field, n, default=None, inf=None):
            v = c.get(field, default)
            if v is None and default is None and field not in c:
                raise ValueError(f"RegionCost: clause {ci}: {field}: missing")
            v = list(v) if isinstance(v, (list, tuple)) else [v] * n
            if len(v) != n:
                raise ValueError(f"RegionCost: clause {ci}: {field}: {len(v)} values for {n} cols")
            out = []
            for x in v:
                if x is None and inf is not None:
                    x = inf
                if isinstance(x, bool) or not isinstance(x, (int, float)):
                    raise ValueError(f"RegionCost: clause {ci}: {field}: {x!r} is not a number")
                out.append(float(x))
            return out

        clauses = []
        for ci, c in enumerate(raw):
            if not isinstance(c, dict):
                raise ValueError(f"RegionCost: clause {ci}: an object is required, got {type(c).__name__}")
            t = c.get("type")
            if t not in cls.TYPES:
                raise ValueError(f"RegionCost: clause {ci}: type: {t!r} (one of {sorted(cls.TYPES)})")
            fields = {"box": {"lo", "hi"}, "halfspace": {"w", "b"}, "ball": {"center", "radius"}}[t] | {"type", "cols", "negate"}
            if set(c) - fields:
                raise ValueError(f"RegionCost: clause {ci}: unknown field(s) {sorted(set(c) - fields)} for a {t}")
            cols = c.get("cols")
            if not isinstance(cols, (list, tuple)) or not 1 <= len(cols) <= REGION_MAX_TERMS:
                raise ValueError(f"RegionCost: clause {ci}: cols: a list of 1..{REGION_MAX_TERMS} columns is required")
            cols = [column(ci, x) for x in cols]
            n = len(cols)
            negate = c.get("negate", False)
            if not isinstance(negate, bool):
                raise ValueError(f"RegionCost: clause {ci}: negate: {negate!r} is not true or false")
            if t == "box":
                a = numbers(ci, c, "lo", n, default=[None] * n, inf=-math.inf)
                b = numbers(ci, c, "hi", n, default=[None] * n, inf=math.inf)
                cc = 0.0
            elif t == "halfspace":
                a, b = numbers(ci, c, "w", n), [0.0] * n
                (cc,) = numbers(ci, c, "b", 1, default=0.0)
            else:
                a, b = numbers(ci, c, "center", n), [0.0] * n
                (r,) = numbers(ci, c, "radius", 1)
                if not r >= 0.0:
                    raise ValueError(f"RegionCost: clause {ci}: radius: {r!r} must be >= 0")
                cc = r * r
            clauses.append((cls.TYPES[t], negate, cols, a, b, cc))
        return cls(clauses, cls.COMBINE[combine], obs_dim, acs_dim, discrete, name=name)

    # ---- every analytic kind is a member of the family (the constructors of AnalyticCost) ----
    @classmethod
    def null(cls, obs_dim, acs_dim, discrete=False):
        return cls([(REGION_BOX, True, [0], [-math.inf], [math.inf], 0.0)], REGION_ANY, obs_dim, acs_dim, discrete, name="null_cost")

    @classmethod
    def wall_behind(cls, pos, index, obs_dim, acs_dim, discrete=False):
        return cls([(REGION_BOX, False, [index], [-math.inf], [pos], 0.0)], REGION_ANY, obs_dim, acs_dim, discrete, name="wall_behind")

    @classmethod
    def wall_infront(cls, pos, index, obs_dim, acs_dim, discrete=False):
        return cls([(REGION_BOX, False, [index], [pos], [math.inf], 0.0)], REGION_ANY, obs_dim, acs_dim, discrete, name="wall_infront")

    @classmethod
    def wall_behind_and_infront(cls, back, front, index, obs_dim, acs_dim, discrete=False):
        return cls([(REGION_BOX, False, [index], [-math.inf], [back], 0.0), (REGION_BOX, False, [index], [front], [math.inf], 0.0)],
                   REGION_SUM, obs_dim, acs_dim, discrete, name="wall_behind_and_infront")

    @classmethod
    def torque(cls, threshold, obs_dim, acs_dim):
        """any |a| > threshold over all (<= 8) action columns.  The bounds are the threshold as a float32, which is what numpy compares a
        float32 action with."""
        t = float(np.float32(threshold))
        cols = [obs_dim + j for j in range(acs_dim)]
        return cls([(REGION_BOX, True, cols, [-t] * acs_dim, [t] * acs_dim, 0.0)], REGION_ANY, obs_dim, acs_dim, name="torque_constraint")

    @classmethod
    def action_equals(cls, value, obs_dim):
        return cls([(REGION_BOX, False, [obs_dim], [value], [value], 0.0)], REGION_ANY, obs_dim, 1, True, name="action_equals")

    def __repr__(self):
        return f"RegionCost({self.name}, {len(self.clauses)} clause(s), combine={self.combine}, obs_dim={self.obs_dim}, acs_dim={self.acs_dim})"

    @property
    def reads_obs(self):
        return any(c < self.obs_dim for _, _, cols, _, _, _ in self.clauses for c in cols)

    @property
    def reads_acs(self):
        return any(c >= self.obs_dim for _, _, cols, _, _, _ in self.clauses for c in cols)

    def table(self):
        """the host clause table (RegionClauseT array)"""
        if self._table is None:
            tab = (RegionClauseT * len(self.clauses))()
            for q, (t, ng, cols, a, b, c) in zip(tab, self.clauses):
                q.type, q.negate, q.n_terms, q.c = t, int(ng), len(cols), c
                for k in range(len(cols)):
                    q.col[k], q.a[k], q.b[k] = cols[k], a[k], b[k]
            self._table = tab
        return self._table

    def struct(self, device=None):
        """the descriptor (CostRegionT); the host table and its device copy (uploaded once, on the first call) live as long as this object"""
        if self._struct is None:
            import ctypes
            tab = self.table()
            raw = np.frombuffer(ctypes.string_at(ctypes.addressof(tab), ctypes.sizeof(tab)), dtype=np.uint8).copy()
            self._d_table = torch.from_numpy(raw).to(device if device is not None else "cuda")
            self._struct = CostRegionT(self.obs_dim, self.acs_dim, 0, COST_REGION, len(self.clauses), self.combine, ctypes.addressof(tab),
                                       self._d_table.data_ptr())
        return self._struct

    # ---- evaluation ----
    def _rows(self, obs, acs):
        """(obs [n, obs_dim] or None, acs [n, acs_dim] or None, leading shape) of numpy arrays or tensors"""
        lead = None
        if obs is not None and self.reads_obs:
            if obs.shape[-1] != self.obs_dim:
                raise ValueError(f"RegionCost: observations of {obs.shape[-1]} columns, the cost was built for {self.obs_dim}")
            lead = tuple(obs.shape[:-1])
            obs = obs.reshape(-1, self.obs_dim)
        else:
            obs = None
        if acs is not None and self.reads_acs:
            if self.discrete:
                acs = acs.reshape(acs.shape[0], -1)[:, :1] if lead is None or len(lead) <= 1 else acs.reshape(*lead, -1)[..., :1]
            if acs.shape[-1] != self.acs_dim:
                raise ValueError(f"RegionCost: actions of {acs.shape[-1]} columns, the cost was built for {self.acs_dim}")
            if lead is None:
                lead = tuple(acs.shape[:-1])
            acs = acs.reshape(-1, self.acs_dim)
        else:
            acs = None
        if lead is None:
            ref = obs if obs is not None else acs
            raise ValueError("RegionCost: the rows this cost reads were not given" if ref is None else "RegionCost: no rows")
        return obs, acs, lead

    def __call__(self, obs, acs=None):
        if torch.is_tensor(obs) or torch.is_tensor(acs):
            return self._device(obs, acs)
        o, a, lead = self._rows(None if obs is None else np.asarray(obs), None if acs is None else np.asarray(acs))
        if self.reads_obs and o is None or self.reads_acs and a is None:
            raise ValueError("RegionCost: the rows this cost reads were not given")
        o = None if o is None else o.astype(np.float64)
        a = None if a is None else a.astype(np.float32).astype(np.float64)      # (widening a float32 is exact)
        n = int(np.prod(lead)) if len(lead) else 1

        def col(c):
            return o[:, c] if c < self.obs_dim else a[:, c - self.obs_dim]

        count = np.zeros(n, dtype=np.int32)
        with np.errstate(invalid="ignore", over="ignore"):
            for t, negate, cols, ca, cb, cc in self.clauses:
                if t == REGION_BOX:
                    r = np.ones(n, dtype=bool)
                    for k, c in enumerate(cols):
                        x = col(c)
                        r &= (np.float64(ca[k]) <= x) & (x <= np.float64(cb[k]))
                elif t == REGION_HALFSPACE:
                    acc = np.full(n, cc, dtype=np.float64)
                    for k, c in enumerate(cols):
                        acc = acc + np.float64(ca[k]) * col(c)
                    r = acc >= 0.0
                else:
                    acc = np.zeros(n, dtype=np.float64)
                    for k, c in enumerate(cols):
                        d = col(c) - np.float64(ca[k])
                        acc = acc + d * d
                    r = acc <= np.float64(cc)
                count += (~r if negate else r).astype(np.int32)
        if self.combine == REGION_ANY:
            out = (count > 0).astype(np.float32)
        elif self.combine == REGION_ALL:
            out = (count == len(self.clauses)).astype(np.float32)
        else:
            out = count.astype(np.float32)
        return out.reshape(lead)

    def _device(self, obs, acs):
        """icrl_cost_region_rows over the flattened leading dimensions: float32 costs on the device, no host copies."""
        ref = obs if torch.is_tensor(obs) else acs
        dev = ref.device
        o, a, lead = self._rows(None if obs is None else torch.as_tensor(obs, device=dev), None if acs is None else torch.as_tensor(acs, device=dev))
        if self.reads_obs and o is None or self.reads_acs and a is None:
            raise ValueError("RegionCost: the rows this cost reads were not given")
        o = None if o is None else o.to(torch.float64).contiguous()
        a = None if a is None else a.to(torch.float32).contiguous()
        n = int(np.prod(lead)) if len(lead) else 1
        out = torch.empty(n, dtype=torch.float32, device=dev)
        if n > 0:
            _lib.check(_lib.lib().icrl_cost_region_rows(_lib.byref(self.struct(dev)), p(o), p(a), n, p(out), _lib.current_stream()),
                       "icrl_cost_region_rows")
        return out.reshape(lead)


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


def cost_for(env_id, cost_spec=None, env=None):
    """the ground-truth cost an entry point trains and evaluates against: `true_cost_for(env_id)`, or — with `--cost_spec` — the
    RegionCost the spec describes over the spaces of `env` (a VecEnv or an env: observation_space, action_space), which replaces the id's."""
    if cost_spec is None:
        return true_cost_for(env_id)
    if env is None:
        raise ValueError("--cost_spec: an env is required to size the region cost")
    discrete = not hasattr(env.action_space, "shape") or len(getattr(env.action_space, "shape", ())) == 0 or hasattr(env.action_space, "n")
    obs_dim = int(np.prod(env.observation_space.shape))
    acs_dim = 1 if discrete else int(np.prod(env.action_space.shape))
    return RegionCost.from_spec(cost_spec, obs_dim, acs_dim, discrete)


def check_cost_spec_flags(config):
    """--cost_spec replaces the id's ground-truth cost: it cannot stand beside a cost of another origin."""
    if getattr(config, "cost_spec", None) is None:
        return
    for flag in ("cn_path", "use_null_cost"):
        if getattr(config, flag, None):
            raise ValueError(f"--cost_spec together with --{flag}: the region cost replaces the ground-truth cost, choose one")


def mean_cost(fn, obs, acs):
    """mean of a cost function over rows; an AnalyticCost is evaluated where the rows are (device tensors: on the device)."""
    c = fn(obs, acs)
    return float(c.double().mean().item()) if torch.is_tensor(c) else float(np.mean(c))
