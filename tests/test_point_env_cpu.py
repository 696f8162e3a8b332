"""CPU: the Point envs (PointCircle / PointCircleTest / PointCircleTestBack / PointNullReward / PointNullRewardTest).

tests/golden/g23_point_env.npz holds what the REFERENCE's own classes (custom_envs/envs/point.py under a 150-step TimeLimit) returned
on four action sequences per class (tools/gen_point_golden.py); tests/helpers/point_env.PointVecEnv is the numpy definition the GPU
tests run the CPU port over.

Bounds (same float32 actions on both sides; derived in DESIGN §17, none fitted):
  ori      bit for bit: one correctly rounded add per step, same order
  x, y     k * 2^-46 after k steps of an episode: per step 4 ulp(1) * 0.25 from cos / sin of two libms plus one ulp at |x| < 64
  reward   4 * k * 2^-46 absolute (denominator >= 1, numerator error |dy| |Dx| + |dx| |Dy| plus ulps at magnitude <= 20)
  dones    equal, where no x sits within 1e-9 of a threshold (asserted)
Sequences "back" and "front" (constant (-/+0.25, 0): every value exact in binary, cos(0) = 1) are compared bit for bit everywhere.
"""
import os

import numpy as np
import pytest

from helpers import point_env

HERE = os.path.dirname(os.path.abspath(__file__))
KINDS = ("point_circle", "point_circle_test", "point_circle_test_back", "point_null", "point_null_test")
IDS = {"PointCircle-v0": ("point_circle", False), "PointCircleTest-v0": ("point_circle_test", True),
       "PointCircleTestBack-v0": ("point_circle_test_back", True), "PointNullReward-v0": ("point_null", False),
       "PointNullRewardTest-v0": ("point_null_test", True)}
SEQS = ("noise", "back", "front", "turn")
EXACT = ("back", "front")
ULP46 = 2.0 ** -46


def episode_step(dones):
    """k[t, n]: the index (1-based) of step t within its episode, from the recorded dones."""
    S, N = dones.shape
    k = np.zeros((S, N), np.int64)
    run = np.zeros(N, np.int64)
    for t in range(S):
        run += 1
        k[t] = run
        run[dones[t]] = 0
    return k


def compare_with_golden(g, kind, seq, obs, rew, done):
    """obs [S, N, 9] (after auto-reset), rew, done of some implementation against the recorded reference."""
    p = f"{kind}/{seq}/"
    robs, rraw, rrew, rdone = g[p + "obs"], g[p + "raw_obs"], g[p + "rewards"], g[p + "dones"]
    if seq in EXACT:
        assert np.array_equal(done, rdone) and np.array_equal(obs, robs) and np.array_equal(rew, rrew), (kind, seq)
        return 0.0, 0.0
    assert np.abs(np.abs(rraw[..., 0]) - 3.0).min() >= 1e-9, "an x of the reference sits on a threshold: dones are not comparable"
    assert np.array_equal(done, rdone), (kind, seq, np.argwhere(done != rdone)[:4])
    k = episode_step(rdone).astype(np.float64)
    assert np.array_equal(obs[..., 2], robs[..., 2]), (kind, seq, "ori")
    assert np.array_equal(obs[..., 3:6], robs[..., 3:6]) and np.array_equal(obs[..., 8], robs[..., 8])
    assert np.array_equal(obs[..., 6:8], obs[..., 0:2])
    ex = np.abs(obs[..., 0:2] - robs[..., 0:2]) / (k[..., None] * ULP46)
    er = np.abs(rew - rrew) / (4.0 * k * ULP46)
    assert ex.max() <= 1.0, (kind, seq, "x / y", ex.max())
    assert er.max() <= 1.0, (kind, seq, "reward", er.max())
    return float(ex.max()), float(er.max())


@pytest.mark.parametrize("kind", KINDS)
def test_helper_env_vs_reference_recording(golden, kind):
    g = golden("g23_point_env")
    for seq in SEQS:
        acts = g[f"{kind}/{seq}/actions"]
        assert acts.dtype == np.float32 and acts.shape == (320, 3, 2)
        env = point_env.PointVecEnv(3, kind)
        assert np.array_equal(env.reset(), np.zeros((3, 9)))
        obs, rew, done = (np.stack(v) for v in zip(*(env.step(acts[t]) for t in range(acts.shape[0]))))
        compare_with_golden(g, kind, seq, obs, rew, done)
        assert (done.sum(axis=0) >= 2).all()      # 320 steps: every env crosses at least two episode ends


def test_back_wall_ends_at_step_13_not_12(golden):
    """constant (-0.25, 0): x is exactly -3.0 after 12 steps (no end: the reference tests x < -3) and -3.25 after 13."""
    g = golden("g23_point_env")
    for kind in KINDS:
        p = f"{kind}/back/"
        raw, done, rew = g[p + "raw_obs"], g[p + "dones"], g[p + "rewards"]
        assert (raw[11, :, 0] == -3.0).all() and (raw[12, :, 0] == -3.25).all()
        ends = kind in ("point_circle_test", "point_circle_test_back", "point_null_test")
        assert not done[:12].any() and done[12].all() == ends and (done[12].any() == ends)
        if ends:
            assert (g[p + "obs"][12] == 0.0).all()                       # auto-reset to zeros
            assert (rew[12] == (1.0 if kind == "point_null_test" else 0.0)).all()
            assert done[12::13].all() and done.sum() == 3 * (320 // 13)
        # the analytic wall cost obs[0] <= -3 is already 1 on the observation the 13th action is taken from
        assert (raw[11, :, 0] <= -3.0).all()
    # the front wall: PointCircleTestBack has none
    assert g["point_circle_test/front/dones"][12].all() and g["point_null_test/front/dones"][12].all()
    assert not g["point_circle_test_back/front/dones"][:149].any() and g["point_circle_test_back/front/dones"][149].all()


def test_turn_sequence_collects_a_reward(golden):
    g = golden("g23_point_env")
    r = g["point_circle/turn/rewards"]
    assert np.abs(r).max() > 0.1 and len(np.unique(r)) > 100
    assert (g["point_null/turn/rewards"] == 1.0).all()


def test_env_tables():
    from icrl_amd import envs
    from icrl_amd.true_constraint_net import TRUE_COSTS
    for env_id, (kind, ends) in IDS.items():
        assert envs.ENV_IDS[env_id] == (kind, ends, False)
        k, early, broken = envs.ENV_IDS[env_id]                 # 3-tuples
        with pytest.raises(ValueError, match="device-resident"):
            envs.register(env_id, "m:a")
    for env_id in ("PointCircleTestBack-v0", "PointCircleTest-v0", "PointNullRewardTest-v0"):
        assert env_id in TRUE_COSTS


def test_vec_env_tables_and_spaces():
    torch = pytest.importorskip("torch")
    from icrl_amd import vec_env
    assert vec_env.ENV_IDS is __import__("icrl_amd.envs", fromlist=["ENV_IDS"]).ENV_IDS
    for kind in KINDS:
        assert vec_env.KINDS[kind] == (9, 2, 150, point_env.FORMS[kind])
        B = vec_env.dynamics_matrix(kind)
        assert B.shape == (9, 2) and not B.any()
    assert [vec_env.KINDS[k][3] for k in ("hc", "ant", "lgw", "clgw")] == [0, 1, 2, 3]
    # the spaces (construction allocates only: no kernel is launched until reset / step)
    for env_id, (kind, ends) in IDS.items():
        env = vec_env.HipSynthVecEnv.make(env_id, 3, device="cpu")
        assert (env.obs_dim, env.act_dim, env.max_steps, env.reward_form) == (9, 2, 150, point_env.FORMS[kind])
        assert env.wall_terminate is ends and env.broken is False
        a, o = env.action_space, env.observation_space
        assert a.shape == (2,) and a.dtype == np.float32 and (a.low == np.float32(-0.25)).all() and (a.high == np.float32(0.25)).all()
        assert o.shape == (9,) and o.dtype == np.float64 and np.isinf(o.low).all() and np.isinf(o.high).all()
        assert env.B.shape == (9, 2) and not env.B.any() and env.s.dtype == torch.float64
        h = point_env.PointVecEnv(3, kind)
        assert np.array_equal(h.action_low, a.low) and np.array_equal(h.action_high, a.high) and h.wall_terminate is ends


def test_point_constraint_net_fixture():
    """the reference's committed Point transfer checkpoint: trained on AntWall (obs 113, act 8) on the x / y position alone."""
    torch = pytest.importorskip("torch")
    sd = torch.load(os.path.join(HERE, "golden", "ref_artifacts", "point_best_cn_model.pt"), map_location="cpu", weights_only=False)
    assert (sd["obs_dim"], sd["acs_dim"], bool(sd["is_discrete"])) == (113, 8, False)
    assert list(sd["obs_select_dim"]) == [0, 1] and list(sd["acs_select_dim"]) == [-1]
    assert list(sd["hidden_sizes"]) == [40, 40] and sd["clip_obs"] == 20
    shapes = [tuple(v.shape) for v in sd["cn_network"].values()]
    assert shapes == [(40, 2), (40,), (40, 40), (40,), (1, 40), (1,)]
