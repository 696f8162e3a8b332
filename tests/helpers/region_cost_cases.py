"""Region costs (true_constraint_net.RegionCost / icrl_cost_region_t): the reference evaluator of the tests and the specs they share.

`evaluate_row` is written straight from the semantics: plain Python floats (IEEE float64, every product and every sum rounded once), one
row at a time, no numpy arithmetic.  The action row is float32 and is widened exactly.  Everything else here builds specs in the JSON
format (`--cost_spec`) and rows that sit exactly on the thresholds, from small dyadic numbers so that every sum is exact."""
import math

import numpy as np

GRID = 8.0      # rows on the dyadic grid: multiples of 1 / 8 in [-2, 2]


def _column(text, obs_dim):
    kind, idx = text.split(":")
    return int(idx) if kind == "obs" else obs_dim + int(idx)


def _bounds(clause, field, n, inf):
    v = clause.get(field)
    v = [None] * n if v is None else (list(v) if isinstance(v, (list, tuple)) else [v] * n)
    return [inf if x is None else float(x) for x in v]


def clause_state(clause, obs_row, acs_row):
    """(truth before `negate`, on_threshold) of one clause of the JSON format on one row"""
    obs_dim = len(obs_row)
    xs = []
    for text in clause["cols"]:
        c = _column(text, obs_dim)
        xs.append(float(obs_row[c]) if c < obs_dim else float(np.float32(acs_row[c - obs_dim])))
    n = len(xs)
    if clause["type"] == "box":
        lo, hi = _bounds(clause, "lo", n, -math.inf), _bounds(clause, "hi", n, math.inf)
        truth, edge = True, False
        for k in range(n):
            truth = truth and (lo[k] <= xs[k] and xs[k] <= hi[k])
            edge = edge or xs[k] == lo[k] or xs[k] == hi[k]
        return truth, edge
    if clause["type"] == "halfspace":
        w = _bounds(clause, "w", n, None)
        acc = float(clause.get("b", 0.0))
        for k in range(n):
            prod = w[k] * xs[k]
            acc = acc + prod
        return acc >= 0.0, acc == 0.0
    if clause["type"] == "ball":
        centre = _bounds(clause, "center", n, None)
        r = float(clause["radius"])
        r2 = r * r
        acc = 0.0
        for k in range(n):
            d = xs[k] - centre[k]
            sq = d * d
            acc = acc + sq
        return acc <= r2, acc == r2
    raise KeyError(clause["type"])


def evaluate_row(spec, obs_row, acs_row):
    """the cost of one row: a Python float equal to the float32 the library stores"""
    truths = []
    for clause in spec["clauses"]:
        t, _ = clause_state(clause, obs_row, acs_row)
        truths.append((not t) if clause.get("negate", False) else t)
    rule = spec.get("combine", "any")
    if rule == "any":
        return 1.0 if any(truths) else 0.0
    if rule == "all":
        return 1.0 if all(truths) else 0.0
    return float(sum(1 for t in truths if t))


def evaluate(spec, obs, acs):
    """float32 [n]: evaluate_row over the rows of obs [n, obs_dim] float64 and acs [n, acs_dim] float32"""
    obs, acs = np.asarray(obs, np.float64), np.asarray(acs, np.float32)
    acs = acs.reshape(obs.shape[0], -1)
    return np.array([evaluate_row(spec, [float(v) for v in obs[i]], acs[i]) for i in range(obs.shape[0])], dtype=np.float32)


def on_threshold(spec, obs_row, acs_row):
    return any(clause_state(c, obs_row, acs_row)[1] for c in spec["clauses"])


# ---- specs ----------------------------------------------------------------------------------------------------------------------------------
def columns(obs_dim, acs_dim):
    """three distinct columns of the shape: the last and the first observation column and the last action column"""
    return [f"obs:{obs_dim - 1}", "obs:0", f"act:{acs_dim - 1}"]


def clause_of(kind, cols, negate=False):
    """the clause of the product test: all numbers dyadic"""
    n = len(cols)
    if kind == "box":
        return dict(type="box", cols=cols, lo=[-0.5, None, -0.25][:n], hi=[0.75, 0.5, 1.0][:n], negate=negate)
    if kind == "halfspace":
        return dict(type="halfspace", cols=cols, w=[0.5, -1.0, 2.0][:n], b=0.25, negate=negate)
    return dict(type="ball", cols=cols, center=[0.25, -0.5, 0.0][:n], radius=1.25, negate=negate)


def product_specs(obs_dim, acs_dim):
    """every type x negate x combine: the clause under test beside a fixed box on the first observation column, so that the rule matters"""
    cols = columns(obs_dim, acs_dim)
    other = dict(type="box", cols=["obs:0"], lo=[-0.375], hi=[None])
    out = []
    for kind in ("box", "halfspace", "ball"):
        for negate in (False, True):
            for rule in ("any", "all", "sum"):
                out.append((f"{kind}-{'neg-' if negate else ''}{rule}", dict(combine=rule, clauses=[clause_of(kind, cols, negate), other])))
    return out


def full_spec(obs_dim, acs_dim):
    """8 clauses of 8 terms each (columns repeat where the shape has fewer than eight), the three types in turn, combine = sum"""
    total = obs_dim + acs_dim
    clauses = []
    for c in range(8):
        idx = [(3 * c + 5 * k) % total for k in range(8)]
        cols = [f"obs:{i}" if i < obs_dim else f"act:{i - obs_dim}" for i in idx]
        kind = ("box", "halfspace", "ball")[c % 3]
        if kind == "box":
            q = dict(type="box", cols=cols, lo=[-1.0 - 0.125 * k for k in range(8)], hi=[1.0 + 0.125 * ((k + c) % 8) for k in range(8)])
        elif kind == "halfspace":
            q = dict(type="halfspace", cols=cols, w=[(0.5, -0.25, 1.0, -2.0)[(k + c) % 4] for k in range(8)], b=0.125 * (c - 4))
        else:
            q = dict(type="ball", cols=cols, center=[0.125 * ((k + c) % 5 - 2) for k in range(8)], radius=2.0 + 0.25 * c)
        q["negate"] = c % 2 == 1
        clauses.append(q)
    return dict(combine="sum", clauses=clauses)


def general_specs(obs_dim, acs_dim, centre=0.0, scale=1.0):
    """the three specs of the rollout tests: a halfspace over two observation columns and an action, a negated ball, `all` of a box and a
    ball.  centre / scale: where the rollout's first observation column lies, so that both outcomes occur (the tests assert it)."""
    a = f"act:{acs_dim - 1}"
    return [("halfspace", dict(combine="any", clauses=[dict(type="halfspace", cols=["obs:0", "obs:1", a], w=[1.0, 0.5, 0.25], b=-centre)])),
            ("neg-ball", dict(combine="any", clauses=[dict(type="ball", cols=["obs:0", a], center=[centre, 0.0], radius=scale, negate=True)])),
            ("box-and-ball", dict(combine="all", clauses=[dict(type="box", cols=["obs:0"], lo=[centre - scale], hi=[centre + scale]),
                                                          dict(type="ball", cols=[a, "act:0"], center=[0.0, 0.0], radius=0.75)]))]


# ---- rows -----------------------------------------------------------------------------------------------------------------------------------
def grid_rows(rng, n, obs_dim, acs_dim, discrete=False):
    """rows on the dyadic grid (every sum of the specs above is exact on them; thresholds are met by chance too)"""
    obs = rng.randint(-16, 17, size=(n, obs_dim)) / GRID
    acs = rng.randint(0, 3, size=(n, 1)).astype(np.float32) if discrete else (rng.randint(-16, 17, size=(n, acs_dim)) / GRID).astype(np.float32)
    return obs, acs


def threshold_rows(spec, rng, obs_dim, acs_dim, discrete=False):
    """one row per clause with distinct columns that lies exactly on that clause's threshold: x_0 == lo_0 (or hi_0), acc == 0, acc == r2"""
    obs, acs = grid_rows(rng, len(spec["clauses"]), obs_dim, acs_dim, discrete)
    keep = []
    for i, q in enumerate(spec["clauses"]):
        cols = [_column(t, obs_dim) for t in q["cols"]]
        if len(set(cols)) != len(cols):
            continue

        def put(k, v):
            if cols[k] < obs_dim:
                obs[i, cols[k]] = v
            else:
                acs[i, cols[k] - obs_dim] = v
        n = len(cols)
        if q["type"] == "box":
            lo, hi = _bounds(q, "lo", n, -math.inf), _bounds(q, "hi", n, math.inf)
            put(0, lo[0] if math.isfinite(lo[0]) else hi[0])
        elif q["type"] == "halfspace":
            w = _bounds(q, "w", n, None)
            for k in range(1, n):
                put(k, 0.0)
            put(0, -float(q.get("b", 0.0)) / w[0])
        else:
            centre = _bounds(q, "center", n, None)
            for k in range(1, n):
                put(k, centre[k])
            put(0, centre[0] + float(q["radius"]))
        keep.append(i)
    return obs[keep], acs[keep]


def rows_for(spec, seed, n, obs_dim, acs_dim, discrete=False):
    """n rows: the threshold rows of the spec, grid rows, then Gaussian rows"""
    rng = np.random.RandomState(seed)
    to, ta = threshold_rows(spec, rng, obs_dim, acs_dim, discrete)
    go, ga = grid_rows(rng, max(n // 2, 1), obs_dim, acs_dim, discrete)
    ro = rng.randn(n, obs_dim) * 0.8
    ra = rng.randint(0, 3, size=(n, 1)).astype(np.float32) if discrete else (rng.randn(n, acs_dim) * 0.6).astype(np.float32)
    obs, acs = np.concatenate([to, go, ro])[:n], np.concatenate([ta, ga, ra])[:n]
    return np.ascontiguousarray(obs), np.ascontiguousarray(acs), min(len(to), n)
