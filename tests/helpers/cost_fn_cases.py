"""Inputs at the decision boundaries of the analytic costs, shared by tests/test_cost_fn_cpu.py and tests/test_cost_fn_gpu.py."""
import numpy as np


def _around(x):
    x = np.float64(x)
    return [np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf)]


def boundary_obs(lo, hi, index, obs_dim=3):
    """float64 rows whose column `index` holds the thresholds themselves and their neighbours on both sides, plus far values."""
    vals = _around(lo) + _around(hi) + [-1e30, 1e30, 0.0, -0.0]
    obs = np.full((len(vals), obs_dim), 123.0)
    obs[:, index] = vals
    return obs


def boundary_acs(thr, acs_dim=4):
    """float32 rows around the float32-rounded threshold, of either sign, in any column; the other entries are small."""
    t = np.float32(thr)
    vals = [np.nextafter(t, np.float32(-np.inf)), t, np.nextafter(t, np.float32(np.inf))]
    rows = []
    for col in range(acs_dim):
        for v in vals:
            for sign in (1.0, -1.0):
                r = np.full(acs_dim, 0.01, np.float32)
                r[col] = np.float32(sign) * v
                rows.append(r)
    rows.append(np.zeros(acs_dim, np.float32))
    return np.stack(rows).astype(np.float32)
