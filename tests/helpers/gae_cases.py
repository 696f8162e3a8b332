"""Inputs of the dual-GAE tests and a numpy statement of the chunked (two-level) scan of csrc/gae.hip.

`random_arrs` is the generator the GPU tests have always used (same draws for the same arguments), with the rate of the `dones`
as an argument.  `CASES` are the parameter sets and done patterns every scan form is run through at T = 300 (300 = 2 x 128 + 44:
ragged chunks, ragged and empty waves; N = 70: two column tiles, six live lanes in the second; N = 72 for the forms that need
N % 4 == 0).  `chunked_scan` composes per-chunk affine maps in float64 the way `gae_dual_split_body` / `gae_dual_regsplit_body` do,
so the CPU suite can state what the re-associated fold may differ by before a GPU is involved (tests/test_gae_fold_cpu.py)."""
import functools

import numpy as np

from oracle import gae as o_gae

F32, F64 = np.float32, np.float64
OUT_KEYS = ("reward_advantages", "cost_advantages", "reward_returns", "cost_returns")

T_FORMS = 300
SEAM_ROWS = (0, 1, 15, 16, 17, 127, 128, 129, 255, 256, 257, T_FORMS - 2, T_FORMS - 1)
# (g_r, l_r, g_c, l_c): all four different (a reward / cost swap shows) | the buffer's default lambda | no decay at all | lambda = 0 (P = 0)
PARAM_SETS = ((0.999, 0.97, 0.5, 0.3), (0.99, 1.0, 0.99, 1.0), (1.0, 1.0, 1.0, 1.0), (0.99, 0.0, 0.9, 0.0))
DONE_PATTERNS = ("none", "all", "random", "seams", "random_last_all", "random_last_none")
# every parameter set with the random pattern, every pattern with the first parameter set
CASES = tuple((p, "random") for p in range(len(PARAM_SETS))) + tuple((0, d) for d in DONE_PATTERNS if d != "random")
SEED = 20


def random_arrs(T, N, seed=None, done_rate=0.002):
    rng = np.random.RandomState(T + N if seed is None else seed)
    arrs = dict(rewards=rng.randn(T, N), costs=rng.rand(T, N), reward_values=rng.randn(T, N), cost_values=rng.randn(T, N),
                dones=(rng.rand(T, N) < done_rate), last_v_r=rng.randn(N), last_v_c=rng.randn(N), last_dones=rng.rand(N) < 0.2)
    return {k: (v.astype(np.float32) if v.dtype != bool else v) for k, v in arrs.items()}


def oracle(arrs, params):
    return o_gae.dual_gae(arrs["rewards"], arrs["costs"], arrs["reward_values"], arrs["cost_values"], arrs["dones"].astype(np.float32),
                          arrs["last_v_r"], arrs["last_v_c"], arrs["last_dones"], *params)


def _frozen(d):
    for v in d.values():
        v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def form_case(N, p, pattern):
    """(arrs, params, oracle outputs) of one entry of CASES at [T_FORMS, N]; computed once, read-only."""
    T = T_FORMS
    arrs = random_arrs(T, N, SEED + 100 * p + DONE_PATTERNS.index(pattern), 0.3)
    if pattern == "none":
        arrs["dones"] = np.zeros((T, N), bool)
    elif pattern == "all":
        arrs["dones"] = np.ones((T, N), bool)
    elif pattern == "seams":
        arrs["dones"] = np.zeros((T, N), bool)
        arrs["dones"][list(SEAM_ROWS)] = True
    elif pattern == "random_last_all":
        arrs["last_dones"] = np.ones(N, bool)
    elif pattern == "random_last_none":
        arrs["last_dones"] = np.zeros(N, bool)
    params = PARAM_SETS[p]
    return _frozen(arrs), params, _frozen(oracle(arrs, params))


def _rows(rewards, values, dones, last_value, last_dones, gamma, gae_lambda):
    """the oracle's own per-row terms (oracle/gae.py:42-54, same dtypes): float32 delta[t], coeff[t] for t < T - 1 and the float64 head."""
    rewards, values, dones = (np.ascontiguousarray(x, dtype=F32) for x in (rewards, values, dones))
    T = rewards.shape[0]
    g32, gl32 = F32(gamma), F32(float(gamma) * float(gae_lambda))
    nnt = (F32(1.0) - dones[1:]).astype(F32)
    gv = ((g32 * values[1:]).astype(F32) * nnt).astype(F32)
    delta = ((rewards[:T - 1] + gv).astype(F32) - values[:T - 1]).astype(F32)
    coeff = (gl32 * nnt).astype(F32)
    nnt_l = F64(1.0) - np.asarray(last_dones).astype(bool).astype(F64)
    head = rewards[T - 1].astype(F64) + (g32 * np.asarray(last_value, F32)).astype(F32).astype(F64) * nnt_l - values[T - 1].astype(F64)
    return delta.astype(F64), coeff.astype(F64), head


def _chain(delta, coeff, head, values, C, W, Tc, sub):
    """one chain of the two-level scan: C chunks of Tc rows, W waves of `sub` rows in each; maps composed latest-first across the waves,
    then across the chunks (gae.hip: gae_dual_split_body), then every wave replays its rows from its carry-in."""
    T, N = values.shape
    rows_of = {}
    P = np.ones((C, W, N)); Q = np.zeros((C, W, N))
    for c in range(C):
        wt0 = min(c * Tc, T); wt1 = min(wt0 + Tc, T)
        for w in range(W):
            t0 = min(wt0 + w * sub, wt1); t1 = min(t0 + sub, wt1)
            rows_of[c, w] = (t0, t1)
            p, q = np.ones(N), np.zeros(N)
            for t in range(t1 - 1, t0 - 1, -1):
                if t == T - 1:
                    q, p = head.copy(), np.zeros(N)          # nothing beyond T feeds in
                else:
                    q = delta[t] + coeff[t] * q
                    p = coeff[t] * p
            P[c, w], Q[c, w] = p, q
    cP = np.ones((C, N)); cQ = np.zeros((C, N))               # what wave 0 of chunk c publishes
    for c in range(C):
        p, q = np.ones(N), np.zeros(N)
        for w in range(W - 1, -1, -1):
            q = Q[c, w] + P[c, w] * q
            p = P[c, w] * p
        cP[c], cQ[c] = p, q
    adv = np.full((T, N), np.nan, F32)
    for c in range(C):
        for w in range(W):
            a = np.zeros(N)
            for j in range(C - 1, c, -1):
                a = cQ[j] + cP[j] * a
            for v in range(W - 1, w, -1):
                a = Q[c, v] + P[c, v] * a
            t0, t1 = rows_of[c, w]
            for t in range(t1 - 1, t0 - 1, -1):
                a = head.copy() if t == T - 1 else delta[t] + coeff[t] * a
                adv[t] = a.astype(F32)
    return adv, (adv + np.ascontiguousarray(values, dtype=F32)).astype(F32)


def chunked_scan(arrs, params, C, W, Tc, sub):
    g_r, l_r, g_c, l_c = params
    d = arrs["dones"].astype(F32)
    a_r, r_r = _chain(*_rows(arrs["rewards"], arrs["reward_values"], d, arrs["last_v_r"], arrs["last_dones"], g_r, l_r), arrs["reward_values"], C, W, Tc, sub)
    a_c, r_c = _chain(*_rows(arrs["costs"], arrs["cost_values"], d, arrs["last_v_c"], arrs["last_dones"], g_c, l_c), arrs["cost_values"], C, W, Tc, sub)
    return dict(reward_advantages=a_r, cost_advantages=a_c, reward_returns=r_r, cost_returns=r_c)


def chunkings(T):
    """name -> (C, W, Tc, sub): the register-resident scan (128-row chunks, 16 rows a wave), the two-pass scan over C = 3 workgroups
    (ceil(T / C) rows a chunk, ceil(Tc / 8) a wave), the one-level scans of 4 and 16 waves, and the sequential scan (no fold at all)."""
    cdiv = lambda a, b: (a + b - 1) // b
    out = {"regsplit": (cdiv(T, 128), 8, 128, 16), "split3": (3, 8, cdiv(T, 3), cdiv(cdiv(T, 3), 8)),
           "waves4": (1, 4, T, cdiv(T, 4)), "waves16": (1, 16, T, cdiv(T, 16)), "sequential": (1, 1, T, T)}
    return out
