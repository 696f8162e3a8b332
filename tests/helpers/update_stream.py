"""The pre-gathered minibatch stream of the update (csrc/ppo_stream.hip) in numpy: its size and every record, from the layout the header
states — one record per 16-row tile of every 64-row chunk in (epoch, minibatch, chunk, tile) order plus one chunk behind the last, a record
= [obs_dim + act_store + 7][16 rows] floats (observations, stored actions, old log-prob, reward / cost advantage, old reward value, reward
return, old cost value, cost return), rows beyond a ragged chunk = the chunk's first row; then {mean_r, istd_r, mean_c, 0} per step (+2)."""
import numpy as np

# name -> (obs_dim, act_dim, act_store, discrete, T, N, batch_size, n_epochs): the smallest shapes at which the stream can go wrong
SHAPES = {
    "hc-b64": (18, 6, 6, 0, 16, 8, 64, 2),          # 128 rows: two full one-chunk minibatches
    "hc-b40": (18, 6, 6, 0, 16, 8, 40, 2),          # minibatches 40, 40, 40, 8: a ragged chunk in every step, a ragged last minibatch
    "hc-b160": (18, 6, 6, 0, 41, 8, 160, 2),        # 328 rows: 160 (chunks 64 + 64 + 32: statistics on four waves), 160, 8
    "hc-35": (18, 6, 6, 0, 7, 5, 64, 2),            # 35 rows: less than one chunk
    "lgw-b64": (1, 2, 1, 1, 16, 8, 64, 2),          # LapGridWorld: one observation, the action index stored as one float
    "lgw-b40": (1, 2, 1, 1, 16, 8, 40, 2),
    "lgw-b160": (1, 2, 1, 1, 41, 8, 160, 2),
    "lgw-35": (1, 2, 1, 1, 7, 5, 64, 2),
}
# continuous widths away from HalfCheetah's (tests/helpers/width_cases.py): one column past the first observation tile with an odd record
# length (17 + 5 + 7), the last width of two tiles with a one-float action (31 + 1 + 7), both tiles and every head position full (32 + 16 + 7)
for _o, _a in ((17, 5), (31, 1), (32, 16)):
    SHAPES[f"o{_o}a{_a}-b40"] = (_o, _a, _a, 0, 16, 8, 40, 2)
    SHAPES[f"o{_o}a{_a}-b160"] = (_o, _a, _a, 0, 41, 8, 160, 2)
PLANES = ("log_probs", "reward_advantages", "cost_advantages", "reward_values", "reward_returns", "cost_values", "cost_returns")


def chunks_of(n, B, E):
    """[(epoch, first position in the epoch's permutation, rows)] of every 64-row chunk in launch order."""
    out = []
    for e in range(E):
        for p in range(0, n, B):
            nb = min(B, n - p)
            out += [(e, p + c, min(64, nb - c)) for c in range(0, nb, 64)]
    return out


def stream_bytes(O, AS, n, B, E):
    rec = 4 * (len(chunks_of(n, B, E)) + 1) * 16 * (O + AS + 7) * 4
    return (rec + 255) // 256 * 256 + 16 * (E * (-(-n // B)) + 2)


def records(buf, perms, T, N, B, E):
    """float32 [4 (chunks + 1), O + AS + 7, 16] from the [T, N, ...] planes of `buf` (numpy) and the flat env-major permutations."""
    n = T * N
    obs = buf["observations"].reshape(n, -1); act = buf["actions"].reshape(n, -1)
    rows = np.concatenate([obs, act] + [buf[k].reshape(n, 1) for k in PLANES], axis=1).astype(np.float32)      # storage order t * N + env
    ch = chunks_of(n, B, E) + [(0, 0, 0)]
    out = np.empty((4 * len(ch), rows.shape[1], 16), np.float32)
    for g, (e, p, nrows) in enumerate(ch):
        pos = np.arange(64); pos[pos >= nrows] = 0
        idx = np.asarray(perms[e])[p + pos]
        sto = (idx % T) * N + idx // T                   # buffers.py:53-65: flat index i -> env = i // T, t = i % T
        out[4 * g:4 * g + 4] = rows[sto].reshape(4, 16, -1).transpose(0, 2, 1)
    return out


def minibatch_stats(buf, perms, T, N, B, E):
    """float64 [steps, 3] mean, 1 / (std + 1e-8) (unbiased std) of the reward advantages and the cost advantages' mean, per optimiser step."""
    n = T * N
    out = []
    for e in range(E):
        for p in range(0, n, B):
            idx = np.asarray(perms[e])[p:p + B]
            sto = (idx % T) * N + idx // T
            ar = buf["reward_advantages"].reshape(n)[sto].astype(np.float64); ac = buf["cost_advantages"].reshape(n)[sto].astype(np.float64)
            out.append((ar.mean(), 1.0 / (ar.std(ddof=1) + 1e-8), ac.mean()))
    return np.asarray(out)
