"""GPU: the persistent PPO-Lagrangian update (icrl_ppo_lag_train) at the observation and action widths between HalfCheetah's 18 x 6 and
AntWall's 113 x 8 — the instantiations that handle the width at run time (OBS = 0), which every other kernel-level test passes by: wave quads
and halves at obs <= 32 away from 18, wave pairs at 33..64, the four-workgroup kernels at 65..128 away from 113, and the row-owning and tiles
kernels behind them (tests/helpers/width_cases.py has the matrix; the route of every case is asserted behind its train()).

Every case runs at the `shaped` policy state on a banded buffer under hyper-parameter set A or B; its inputs' conditions are asserted from the
oracle alone (tests/test_width_cases_cpu.py runs the same list on the CPU).  The comparison is test_ppo_train_gpu._compare_with_oracle,
unchanged: every parameter within ADAM_DEV_BOUND x lr x steps + 2e-7, the seven train/* scalars, the per-epoch KLs.  On top of it: both Adam
moments against the oracle's optimiser state, and the flat buffers sit between guard zones that must keep their bits.

Moments: a parameter travels lr m^ / (sqrt(v^) + eps) per step, and the parameter bound allows 5e-4 of a full step; that is a relative error of
5e-4 in m and of 1e-3 in v (under the root) at the scale of the tensor — so |m - oracle| <= ADAM_DEV_BOUND max|m| and |v - oracle| <= 2
ADAM_DEV_BOUND max|v| per tensor.  The measured ratios are printed (ADAM_MOMENTS)."""
import numpy as np
import pytest
import torch

from helpers import routes, width_cases as W

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 256, 7.0      # floats on either side of every flat buffer (1 KiB: the buffers keep their alignment)


def _agent(obs, act, N, T, **kw):
    from icrl_amd import spaces
    from icrl_amd.ppo_lag import PPOLagrangian
    from icrl_amd.vec_env import HipSynthVecEnv, VecCostWrapper, VecNormalizeWithCost
    senv = HipSynthVecEnv(N, "hc", 0)      # (nothing steps it: the buffer is filled by hand, only its spaces count)
    senv.observation_space = spaces.Box(-np.inf, np.inf, (obs,), np.float64)
    senv.action_space = spaces.Box(-1.0, 1.0, (act,), np.float32)
    return PPOLagrangian("TwoCriticsMlpPolicy", VecNormalizeWithCost(VecCostWrapper(senv)), n_steps=T, seed=0, **kw)


def _guard(pol):
    """the policy's flat buffers moved between two guard zones each; returns name -> the enlarged tensor."""
    big = {}
    for name in ("params", "params_t", "exp_avg", "exp_avg_sq"):
        old = getattr(pol, name)
        big[name] = torch.full((old.numel() + 2 * GUARD,), SENTINEL, device=old.device)
        big[name][GUARD:GUARD + old.numel()].copy_(old)
        setattr(pol, name, big[name][GUARD:GUARD + old.numel()])
    return big


def _real_mask(pol):
    parts = []
    for k, shp in pol.shapes.items():
        m = np.zeros(shp, bool)
        m[tuple(slice(0, n) for n in pol.logical_shapes[k])] = True
        parts.append(m.ravel())
    return np.concatenate(parts)


@pytest.mark.parametrize("case", W.UPDATE_CASES, ids=[W.update_id(c) for c in W.UPDATE_CASES])
def test_update_vs_oracle_at_width(case):
    import test_ppo_train_gpu as tp
    from icrl_amd import logger
    obs, act, layout, hset, kernel, kind = case
    N, T, B, E = W.LAYOUTS[layout]
    c, sd0 = W.check_update_inputs(obs, act, layout, hset)      # check_trace on every step, C1, C6 — from the oracle, before a kernel runs
    hp, lr = c["hp"], c["lr"]
    agent = _agent(obs, act, N, T, batch_size=B, n_epochs=E, target_kl=None, learning_rate=lr, clip_range=0.2, **hp)
    if kernel is not None:
        agent.train_kernel = kernel
    pol = agent.policy
    assert (pol.obs_dim, pol.act_dim, pol.wide) == (obs, act, False) and agent.dual.nu().item() == c["nu"]
    big = _guard(pol)
    pol.load_state_dict(sd0)
    tp._fill(agent, c["buf"])
    mask = _real_mask(pol)
    before = {k: v.cpu().numpy().copy() for k, v in big.items()}
    logger.configure()
    agent.train(perms=c["perms"])
    routes.check_update(dict(kind=kind, n_runs=1), W.update_id(case))
    assert float(agent._train_ws["stats"][11]) == 0.0, "inter-workgroup exchange timed out"
    after = {k: v.cpu().numpy() for k, v in big.items()}
    for k in ("params", "exp_avg", "exp_avg_sq"):
        assert np.isfinite(after[k]).all(), k
        # everything outside the logical tensors keeps its bits: the guard zones and the padding entries of the layout
        outside = np.concatenate([np.ones(GUARD, bool), ~mask, np.ones(GUARD, bool)])
        assert np.array_equal(after[k][outside].view(np.uint32), before[k][outside].view(np.uint32)), (k, int((after[k][outside] != before[k][outside]).sum()))
    for side in (slice(0, GUARD), slice(-GUARD, None)):
        assert np.array_equal(after["params_t"][side], before["params_t"][side])
    assert pol.adam_step == W.n_steps(layout)
    rel = tp._compare_with_oracle(agent, c["params"], c["out"], f"o{obs}a{act}", B, lr)
    print(f"ADAM_DEV_WIDTH {W.update_id(case)} band {W.band(obs)} kind {kind}: {rel:.3g} x lr x steps = {rel / tp.ADAM_DEV_BOUND:.3f} of the bound")
    worst = {}
    for name, ref, units in (("exp_avg", c["exp_avg"], 1.0), ("exp_avg_sq", c["exp_avg_sq"], 2.0)):
        got = pol._split(getattr(pol, name).detach().cpu())
        worst[name] = max(float(np.abs(got[k].numpy() - ref[k]).max() / (units * tp.ADAM_DEV_BOUND * np.abs(ref[k]).max())) for k in ref)
    print(f"ADAM_MOMENTS {W.update_id(case)}: exp_avg {worst['exp_avg']:.3f}, exp_avg_sq {worst['exp_avg_sq']:.3f} of their bounds")
    assert worst["exp_avg"] <= 1.0 and worst["exp_avg_sq"] <= 1.0, worst
