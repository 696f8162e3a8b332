"""Cases and CPU-measured bounds of the fine-grained entry points (csrc/fine.hip; tests/test_fine_grained_gpu.py).  Everything here runs on the
CPU: the oracle's expressions (oracle/ppo.py, oracle/cn.py) under torch at float32 and float64.

1. icrl_ppo_lag_loss_fwd_bwd: one banded minibatch per row count (helpers/ppo_hparam_cases.py: no row on a kink of the ratio clip or of a value
   clip; the seed of a row count is picked here so that the conditions hold under sets A and B) and, per output gradient,
       dev = max |float32 oracle - float64 oracle|
   stored per n in ROW_GRAD_F32_DEV by
       python tests/helpers/fine_cases.py          (prints the table; torch CPU, default threads)
   loss_fwd_bwd_kernel is one block of 256 threads: n = 64 and 100 stay inside the first trip of its `for (i = tid; i < n; i += 256)` loops,
   n = 300 gives 44 threads a second row, n = 1000 every thread three and 232 threads a fourth.
2. icrl_is_weights: the episode lengths that send every loop of is_weights_kernel (16 waves over episodes, 64 lanes over an episode's steps,
   1024 threads over the rows) past its first trip, its inputs, and the float32 / float64 oracles whose distance is the unit of the bound.
"""
import os
import sys

import numpy as np
import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for _p in (_ROOT, os.path.join(_ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import cn as o_cn, ppo as o_ppo      # noqa: E402

ROW_GRAD_KEYS = ("d_lp", "d_vr", "d_vc", "d_en")
LOSS_ROWS = (64, 100, 300, 1000)
LOSS_NU = 0.731
HPARAM_SEED = {}                                        # n -> seed of hparam_batch; every other n: 100 + n (conditions asserted by the tests)


class Outputs:
    """the networks' outputs as autograd leaves: oracle.ppo.minibatch_loss evaluates policy.evaluate_actions(obs, actions)."""

    def __init__(self, v_r, v_c, lp, ent, dtype):
        self.leaves = [torch.as_tensor(x, dtype=dtype).clone().requires_grad_(True) for x in (v_r, v_c, lp, ent)]

    def evaluate_actions(self, obs, actions):
        return tuple(self.leaves)


def hparam_batch(n):
    """one banded minibatch of n rows (helpers/ppo_hparam_cases.py: no row on a kink of the ratio clip or of a value clip)."""
    from helpers import ppo_hparam_cases as H
    rng = np.random.RandomState(HPARAM_SEED.get(n, 100 + n))
    f = lambda x: np.asarray(x, np.float32)
    out = dict(lp=f(-8 + 0.3 * rng.randn(n)), v_r=f(rng.randn(n)), v_c=f(rng.rand(n)), ent=f(8.5 + 0.1 * rng.randn(n)), adv_r=f(2 * rng.randn(n)),
               adv_c=f(rng.rand(n)), ret_r=f(rng.randn(n)), ret_c=f(rng.rand(n)))
    out["old_lp"], out["old_v_r"], out["old_v_c"] = H.banded(rng, out["lp"], out["v_r"], out["v_c"], H.SET_A["clip_range_reward_vf"], H.SET_A["clip_range_cost_vf"])
    return out


def loss_and_row_grads(b, hp, nu, dtype):
    """oracle.ppo.minibatch_loss on the outputs + autograd: (terms in the library's order, d loss / d (lp, v_r, v_c, entropy))."""
    t = lambda k: torch.as_tensor(b[k], dtype=dtype)
    pol = Outputs(b["v_r"], b["v_c"], b["lp"], b["ent"], dtype)
    loss, tr = o_ppo.minibatch_loss(pol, None, None, t("old_lp"), t("adv_r"), t("adv_c"), t("ret_r"), t("ret_c"), t("old_v_r"), t("old_v_c"), nu, 0.2,
                                    hp["ent_coef"], hp["reward_vf_coef"], hp["cost_vf_coef"], hp["clip_range_reward_vf"], hp["clip_range_cost_vf"])
    loss.backward()
    v_r, v_c, lp, ent = pol.leaves
    terms = [loss.item()] + [tr[k].item() for k in ("policy_loss", "reward_value_loss", "cost_value_loss", "entropy_loss", "approx_kl", "clip_fraction")]
    ratio = torch.exp(lp.detach() - t("old_lp"))
    margins = (float(torch.minimum((ratio - 0.8).abs(), (ratio - 1.2).abs()).min()),
               float(((v_r.detach() - t("old_v_r")).abs() - hp["clip_range_reward_vf"]).abs().min()),
               float(((v_c.detach() - t("old_v_c")).abs() - hp["clip_range_cost_vf"]).abs().min()))
    shares = (tr["clip_fraction"].item(), float(((v_r.detach() - t("old_v_r")).abs() > hp["clip_range_reward_vf"]).double().mean()),
              float(((v_c.detach() - t("old_v_c")).abs() > hp["clip_range_cost_vf"]).double().mean()))
    return terms, dict(d_lp=lp.grad.numpy(), d_vr=v_r.grad.numpy(), d_vc=v_c.grad.numpy(), d_en=ent.grad.numpy()), margins, shares


def banded_conditions_hold(margins, shares):
    from helpers import ppo_hparam_cases as H
    return (margins[0] >= H.RATIO_MARGIN and margins[1] >= H.VALUE_MARGIN and margins[2] >= H.VALUE_MARGIN
            and H.CLIP_FRACTION[0] <= shares[0] <= H.CLIP_FRACTION[1] and all(H.VCLIP_SHARE[0] <= s <= H.VCLIP_SHARE[1] for s in shares[1:]))


def row_grad_dev(n):
    """per output gradient: max over sets A and B of max |float32 oracle - float64 oracle| (and the largest |float64| entry, for scale)."""
    from helpers import ppo_hparam_cases as H
    dev, big = dict.fromkeys(ROW_GRAD_KEYS, 0.0), dict.fromkeys(ROW_GRAD_KEYS, 0.0)
    b = hparam_batch(n)
    for hset in ("A", "B"):
        _, g64, margins, shares = loss_and_row_grads(b, H.hparams(hset), LOSS_NU, torch.float64)
        assert banded_conditions_hold(margins, shares), (n, hset, margins, shares)
        _, g32, _, _ = loss_and_row_grads(b, H.hparams(hset), LOSS_NU, torch.float32)
        for k in ROW_GRAD_KEYS:
            dev[k] = max(dev[k], float(np.abs(g32[k].astype(np.float64) - g64[k]).max()))
            big[k] = max(big[k], float(np.abs(g64[k]).max()))
    return dev, big


# Per-row output gradients: max |float32 oracle - float64 oracle| over sets A and B, measured on the CPU by the command above.  The tests' bound
# is 3 x that: the kernel's reductions (advantage mean and standard deviation) run in another order than torch's.
#   n = 64, 100 (one entry for both, as measured over their four cases): d_lp 3.5e-9 (of values up to 0.025), d_vr 3.4e-9 (of 0.091),
#       d_vc 5.5e-10 (of 0.0087), d_en 3.5e-12 (of 1.6e-4: float32(ent_coef) / n)
#   n = 300, 1000: see the table (ROW_GRAD_BEGIN .. ROW_GRAD_END is what the command prints for them)
_N64_100 = dict(d_lp=3.5e-9, d_vr=3.4e-9, d_vc=5.5e-10, d_en=3.5e-12)
# ROW_GRAD_BEGIN
ROW_GRAD_F32_DEV = {
    64: _N64_100,
    100: _N64_100,
    # 64 measured alone: {'d_lp': 3.46e-09, 'd_vr': 3.35e-09, 'd_vc': 5.5e-10, 'd_en': 3.49e-12}
    # 100 measured alone: {'d_lp': 2.12e-09, 'd_vr': 1.83e-09, 'd_vc': 3.43e-10, 'd_en': 2.53e-12}
    300: {'d_lp': 1.18e-09, 'd_vr': 1.15e-09, 'd_vc': 2.48e-10, 'd_en': 3.71e-13},      # largest entries: d_lp 0.0069, d_vr 0.017, d_vc 0.0017, d_en 3.3e-05
    1000: {'d_lp': 4.76e-10, 'd_vr': 5.86e-10, 'd_vc': 8.02e-11, 'd_en': 2.53e-13},      # largest entries: d_lp 0.0025, d_vr 0.0069, d_vc 0.00057, d_en 1e-05
}
# ROW_GRAD_END


# ---- icrl_is_weights past the first trip of each of its walks
# 20 episodes > 16 waves; 65, 129, 200 .. 1000 steps > 64 lanes (64, 128, 640: whole trips; 65, 129: one live lane in the last trip;
# 1, 2, 7, 17, 33, 63: inside one trip, after longer ones on the same wave); N = 6489 rows > 1024 threads
IS_LENGTHS = (1000, 65, 64, 1, 200, 129, 1000, 63, 500, 7, 300, 128, 2, 1000, 90, 33, 640, 17, 250, 1000)
IS_EPS = 1e-5
IS_UNITS = 4.0


def is_weights_inputs():
    """old ~ U(0.2, 0.9), new = clip(old + U(-0.02, 0.02), 0.01, 0.99), float32 [N, 1]: the episode products stay in [0.14, 1.93]."""
    rng = np.random.RandomState(3)
    n = sum(IS_LENGTHS)
    old = torch.as_tensor(rng.uniform(0.2, 0.9, (n, 1)).astype(np.float32))
    new = (old + torch.as_tensor(rng.uniform(-0.02, 0.02, (n, 1)).astype(np.float32))).clamp(0.01, 0.99)
    return old, new


def is_weights_oracles(per_step):
    """oracle.cn.is_weights_and_kls on the float32 inputs at float64 (the reference) and at float32 -> ((w, kl_on, kl_no, prod) as float64
    numpy per dtype, the bounds IS_UNITS x max |oracle32 - oracle64| + 1e-12 of weights and both KLs)."""
    old, new = is_weights_inputs()
    res = []
    for dtype in (torch.float64, torch.float32):
        w, kl_on, kl_no, prod = o_cn.is_weights_and_kls(old.to(dtype), new.to(dtype), list(IS_LENGTHS), IS_EPS, per_step, with_prod=True)
        assert w.dtype == dtype and prod.dtype == dtype
        res.append(dict(w=w.double().numpy().ravel(), kl_on=float(kl_on), kl_no=float(kl_no), prod=prod.double().numpy()))
    r64, r32 = res
    bounds = dict(w=IS_UNITS * float(np.abs(r32["w"] - r64["w"]).max()) + 1e-12, kl_on=IS_UNITS * abs(r32["kl_on"] - r64["kl_on"]) + 1e-12,
                  kl_no=IS_UNITS * abs(r32["kl_no"] - r64["kl_no"]) + 1e-12)
    return r64, r32, bounds


if __name__ == "__main__":
    print("ROW_GRAD_F32_DEV = {\n    64: _N64_100,\n    100: _N64_100,")
    for n in LOSS_ROWS:
        dev, big = row_grad_dev(n)
        line = "{" + ", ".join(f"{k!r}: {dev[k]:.3g}" for k in ROW_GRAD_KEYS) + "}"
        scale = ", ".join(f"{k} {big[k]:.2g}" for k in ROW_GRAD_KEYS)
        print(f"    {n}: {line},      # largest entries: {scale}" if n > 100 else f"    # {n} measured alone: {line}")
    print("}")
    for per_step in (False, True):
        r64, r32, bounds = is_weights_oracles(per_step)
        print(f"# is_weights per_step={per_step}: products in [{r64['prod'].min():.3g}, {r64['prod'].max():.3g}], largest weight {r64['w'].max():.3g}, "
              f"bounds {bounds}")
