"""The gSDE cases of tests/golden/g26_sde.npz (tools/gen_sde_golden.py: the reference's own policy and train() at a trained-like state)
and a numpy restatement of the head, written from the formulas alone:

    latent = the policy branch's last tanh layer          mean = action_net(latent)
    var_a  = sum_h latent_h^2 exp(2 log_std[h, a]) + 1e-6
    log_prob = sum_a -(x_a - mean_a)^2 / (2 var_a) - log(var_a) / 2 - log(sqrt(2 pi))        entropy = sum_a 1/2 + log(2 pi) / 2 + log(var_a) / 2
    d log_prob / d var = ((x - mean)^2 / var - 1) / (2 var)      d entropy / d var = 1 / (2 var)      d var / d log_std[h, a] = 2 latent_h^2 exp(2 log_std[h, a])
"""
import os
from collections import OrderedDict

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "g26_sde.npz")
SHAPES = {"hc": (18, 6, dict(pi=[64, 64], vf=[64, 64], cvf=[64, 64])), "pl": (11, 3, dict(pi=[32, 48], vf=[64, 64], cvf=[64, 64]))}
OUTS = ("v_r", "v_c", "log_prob", "entropy")
_gold = None


def gold():
    global _gold
    if _gold is None:
        with np.load(GOLDEN) as z:
            _gold = {k: z[k] for k in z.files}
    return _gold


def names(tag):
    from icrl_amd.policies import state_dict_names
    return state_dict_names(False)


def state(tag, prefix="w"):
    g = gold()
    return OrderedDict((k, g[f"{tag}/{prefix}/{k}"]) for k in names(tag))


def spaces_of(tag):
    from icrl_amd import spaces
    O, A, _ = SHAPES[tag]
    return spaces.Box(-np.inf, np.inf, (O,), np.float64), spaces.Box(-1.0, 1.0, (A,), np.float32)


def policy(tag, device="cuda", use_sde=True, load=True):
    """ActorTwoCriticsPolicy of the case's shape holding g26's weights (the diagonal form: the same network, log_std = the matrix's first row)."""
    import torch
    from icrl_amd.policies import ActorTwoCriticsPolicy
    o, a = spaces_of(tag)
    pol = ActorTwoCriticsPolicy(o, a, net_arch=[dict(SHAPES[tag][2])], device=device, use_sde=use_sde)
    if load:
        sd = state(tag)
        if not use_sde:
            sd["log_std"] = sd["log_std"][0].copy()
        pol.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    return pol


def head_numpy(sd, obs, act, up=None):
    """float64: (outputs dict, d/d log_std of sum(up * outputs) or None)."""
    f = lambda k: np.asarray(sd[k], np.float64)
    x = np.asarray(obs, np.float64)
    lat = {}
    for b in ("policy_net", "value_net", "cost_value_net"):
        h = np.tanh(x @ f(f"mlp_extractor.{b}.0.weight").T + f(f"mlp_extractor.{b}.0.bias"))
        lat[b] = np.tanh(h @ f(f"mlp_extractor.{b}.2.weight").T + f(f"mlp_extractor.{b}.2.bias"))
    mean = lat["policy_net"] @ f("action_net.weight").T + f("action_net.bias")
    l2, e2 = lat["policy_net"] ** 2, np.exp(2.0 * f("log_std"))
    var = l2 @ e2 + 1e-6
    diff = np.asarray(act, np.float64) - mean
    half_log_2pi = 0.5 * np.log(2.0 * np.pi)
    out = dict(v_r=(lat["value_net"] @ f("value_net.weight").T + f("value_net.bias")).ravel(),
               v_c=(lat["cost_value_net"] @ f("cost_value_net.weight").T + f("cost_value_net.bias")).ravel(),
               log_prob=(-(diff ** 2) / (2.0 * var) - 0.5 * np.log(var) - half_log_2pi).sum(axis=1),
               entropy=(0.5 + half_log_2pi + 0.5 * np.log(var)).sum(axis=1), mean=mean, latent=lat["policy_net"], var=var)
    if up is None:
        return out, None
    d_var = (np.asarray(up["d_log_prob"], np.float64)[:, None] * ((diff ** 2 / var - 1.0) / (2.0 * var))
             + np.asarray(up["d_entropy"], np.float64)[:, None] / (2.0 * var))
    return out, 2.0 * e2 * (l2.T @ d_var)


def upstream(tag, n):
    g = gold()
    return {k: g[f"{tag}/up/{k}"][:n] for k in ("d_v_r", "d_v_c", "d_log_prob", "d_entropy")}


def split_grad(pol, flat):
    """flat gradient in the device layout -> (logical blocks by name, the padding entries of every block as one flat array)."""
    out, pads, off = OrderedDict(), [], 0
    flat = np.asarray(flat)
    for k, shp in pol.shapes.items():
        n = int(np.prod(shp))
        block = flat[off:off + n].reshape(shp)
        real = tuple(slice(0, m) for m in pol.logical_shapes[k])
        out[k] = block[real].copy()
        mask = np.ones(shp, bool)
        mask[real] = False
        pads.append(block[mask])
        off += n
    assert off == flat.size
    return out, np.concatenate(pads)
